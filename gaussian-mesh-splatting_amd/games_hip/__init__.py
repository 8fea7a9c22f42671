"""games_hip: the reference's workflow on the HIP kernels.  The evaluation surface (games_hip.evaluate) is also reachable from the
package itself, and so is LPIPS (games_hip.lpips); both are imported on first use, so `import games_hip` stays as cheap as it was."""
_EVALUATE = ("MetricTable", "metrics_from_rows", "evaluate_views", "training_report", "render_set", "write_png")
_LPIPS = ("LpipsVgg", "lpips", "lpips_rows")
__all__ = list(_EVALUATE) + list(_LPIPS)


def __getattr__(name):
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    if name in _LPIPS:
        import importlib
        return getattr(importlib.import_module(".lpips", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
