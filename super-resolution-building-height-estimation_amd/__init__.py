"""MI355X-native hot path of lauraset/Super-resolution-building-height-estimation.

The directory name follows the build contract (``<repo-name>_amd``) and is not a valid Python
identifier, so it is imported through the alias package ``srbh_amd`` (see ``srbh_amd.py`` at the
repo root), e.g. ``from srbh_amd.rrdbnet import RRDBNet``.  The reference's own import paths
(``SR.rrdbnet_arch``, ``SR.HRfuse``, ``mymodels``, ``aggregate_utils``) are provided by the shim
directory ``dropin/`` (put it on ``sys.path`` ahead of the reference checkout).
"""
__version__ = "0.1.0"

# the reference's stats_dataset_globe names (dataset_stats.py), resolved on first use: importing the package stays free of torch
_DATASET_STATS = ("cal_mean_std", "cal_min_max", "main_stats_merge", "main_stats_buildheight_merge")


def __getattr__(name):
    if name in _DATASET_STATS:
        import importlib
        return getattr(importlib.import_module("srbh_amd.dataset_stats"), name)
    raise AttributeError(f"module 'srbh_amd' has no attribute {name!r}")
