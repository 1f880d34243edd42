from ._pt import PTBatchAugment, PTBatchPipeline, PTInterpolate, PinnedPrefetcher, crop_geometry
from ._mri import compress_series, fit_t2_map, t2_map_series
