"""shim for the reference import path stats_dataset_globe (the host arithmetic over the per-image tables and the region merges;
the per-image pass itself is srbh_amd.dataset_stats.DatasetStats / HeightStats on the device)."""
import _bootstrap  # noqa: F401
from srbh_amd.dataset_stats import cal_mean_std, cal_min_max, main_stats_merge, main_stats_buildheight_merge  # noqa: F401,E402
