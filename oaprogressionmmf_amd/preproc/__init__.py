from ._pt import PTBatchAugment, PTInterpolate, PinnedPrefetcher
from ._mri import compress_series, fit_t2_map, t2_map_series
