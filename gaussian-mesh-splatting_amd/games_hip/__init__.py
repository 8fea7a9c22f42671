"""games_hip: the reference's workflow on the HIP kernels.  The evaluation surface (games_hip.evaluate) is also reachable from the
package itself; it is imported on first use, so `import games_hip` stays as cheap as it was."""
_EVALUATE = ("MetricTable", "metrics_from_rows", "evaluate_views", "training_report", "render_set", "write_png")
__all__ = list(_EVALUATE)


def __getattr__(name):
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
