"""MI355X-native Animatable Gaussians.  The modules are imported by name (``from animatablegaussians_amd import losses``); the two
loader-facing functions of ``targets`` are also reachable from the package, resolved on first use so that importing the package stays
free of side effects."""

__all__ = ["prepare_targets", "boundary_mask"]


def __getattr__(name):
    if name in __all__:
        from . import targets
        return getattr(targets, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
