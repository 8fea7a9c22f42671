"""games_hip: the reference's workflow on the HIP kernels.  The evaluation surface (games_hip.evaluate) is also reachable from the
package itself, and so are LPIPS (games_hip.lpips) and the guide-mesh estimate (games_hip.guide_mesh); all are imported on first use,
so `import games_hip` stays as cheap as it was."""
_EVALUATE = ("MetricTable", "metrics_from_rows", "evaluate_views", "training_report", "render_set", "write_png")
_LPIPS = ("LpipsVgg", "lpips", "lpips_rows")
_GUIDE_MESH = ("DensityGrid", "density_grid", "surface_nets", "grid_components", "clean_grid", "estimate_guide_mesh", "create_dummy_mesh")
__all__ = list(_EVALUATE) + list(_LPIPS) + list(_GUIDE_MESH)


def __getattr__(name):
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    if name in _LPIPS or name in _GUIDE_MESH:
        import importlib
        return getattr(importlib.import_module(".lpips" if name in _LPIPS else ".guide_mesh", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
