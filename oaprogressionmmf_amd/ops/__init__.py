"""Tensor-level wrappers over the libkoaf C ABI, one module per kernel family.

Every function takes/returns `torch.Tensor`s that live on a HIP device (torch is used for device
memory and streams only) and launches hand-written gfx950 kernels on torch's current stream.
Activations are NHWC fp32.  Nothing here falls back to torch math: a CPU tensor or a missing
library raises.

Callers use `ops.<name>`: everything is re-exported here, and this package and `_lib.py` are the only code that calls the library.
"""
# Optional live profiler (bench.py): when a list is installed here every MFMA-GEMM based call is bracketed
# by two events recorded on the stream the kernel is launched on (torch's current stream) and logged as
# (family, algorithmic_flops, start_event, end_event, tag, algorithmic_bytes, mpp) -- see _base._prof_end.
PROFILE = None

from .._lib import KoafBnApply, KoafBnb, KoafEmit, KoafError, KoafGemm, KoafLaunchRec, KoafTail, KoafWImg, KoafWPlane, check, defines, lib
from . import _base, bn, calib, clin, conv, dense, explain, inputs, metrics, mriprep, train
from ._base import (_STATUS_BY_DEV, _a16, _empty, _i32, _prof_begin, _prof_end, _ptr, _status_buffer, _stream, check_numerics, conv_out,
                    numerics_status)
from .bn import (BnApply, _bn_bwd_tail, _colpart_rows, _dy_args, _reduce_ws, bn_add_relu, bn_bwd, bn_bwd_from_part, bn_finalize, colstats,
                 gap_bwd, gap_fwd, maxpool_bwd, maxpool_fwd)
from .calib import (CALIB_EPS, CALIB_FLAG_TEXT, CALIB_MAX_BINS, CALIB_MAX_THR, RECALIB_KINDS, RECALIB_MAX_ITER, RECALIB_MODES,
                    RECALIB_STATUS, calib_edges, calib_flag, calib_metrics, calib_raise, recalib_apply, recalib_fit)
from .clin import CLIN_FLAG_TEXT, LOGREG_MAX_P, clin_design, clin_flag, clin_raise, logreg_fit, logreg_predict
from .conv import (ACT_SCALE, CONV_F16, _dy_planes, _img, _rup, _slab_ws, act_planes, build_weight_planes, conv2d_dgrad, conv2d_fwd,
                   conv2d_wgrad, gconv3x3_dgrad, gconv3x3_fwd, gconv3x3_wgrad, gconv_compress_dw, gconv_expand_w, gemm, launch_log,
                   launch_log_read, set_conv3x3_halo, set_stream, stem_dgrad, stem_fold_w, stem_fwd, stem_wgrad, use_aplanes, wplane_entry,
                   wplanes_build)
from .dense import (add, attention_bwd, attention_fwd, colsum, counter_add, dropout, dropout2d, gelu_bwd, gelu_fwd, layernorm_bwd,
                    layernorm_fwd, linear_dgrad, linear_fwd, linear_wgrad, relu_bwd, relu_fwd, softmax_rows_)
from .explain import (ATTN_MODES, ATTR_MAX_J, CAM_NORMALIZE, COAL_MAX_M, _attr_coefs, _attr_rows, attn_apply, attn_layer, attn_segsum,
                      attr_fold, cam, cam_upsample, coal_tokens, occl_fold, occl_points, occl_rows, occl_slices, path_points, shapley_fold,
                      shapley_weights)
from .inputs import (HostWindowTable, _STORED, _WIDEN, _upload_bytes, _window_ws, augment, downscale2, input_pipeline, minmax, resize,
                     rowdot, slice_fold, slice_unfold, widen, window_minmax, window_rows, window_table)
from .metrics import (METRICS_FLAG_TEXT, METRICS_MAX_N, _metric_scores, confusion, curve_metrics, curve_points, curve_points_len,
                      metrics_flag, metrics_raise, pair_ranks, parse_curve_points, perm_metrics, point_metrics, range_metrics, score_ranks)
from .mriprep import (SERIES_FLAG_TEXT, _SERIES_DTYPE, _series_shift, _series_volume, percentile_index, series_flag, series_hist,
                      series_pack, series_quantiles, series_raise, t2_fit)
from .train import (_BCE_REDUCTIONS, _flat32, adam_hyper, adam_step, bce_loss, focal_loss, grad_fold, grad_norm_final, grad_norm_part,
                    grad_norm_ws, grad_scale, norm_kind, optim_hyper, rmsprop_step, sgd_step)


def __getattr__(name):
    """the status globals that _base rebinds as the process moves between devices: read through, never copied here"""
    if name in ("_STATUS", "_STATUS_DEV"):
        return getattr(_base, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
