"""Mirror of koafusion/various/__init__.py:1-11 for the hot-path pieces."""
from ._calibration import (Recalibrator, brier_score_loss, calc_calibration, calibration_curve, calibration_slope_intercept,
                           decision_curve, expected_calibration_error, fit_temperature, log_loss)
from ._checkpoint import CheckpointHandler, load_train_state, save_train_state
from ._clip import clip_grad_norm_
from ._losses import dict_losses
from ._metrics import (average_precision_score_calib, avg_precision_at_recall_range, bestf1score_calib, bootstrap_indices,
                       calc_bootstrap, calc_metrics_curves, calc_metrics_v2, f1score_calib, mc_bacc, precision_recall_curve,
                       precision_recall_curve_calib, roc_curve, summarize_bootstrap)
from ._logreg import LogisticRegression, fit_logreg_folds
from ._permtest import compare_predictions, permutation_test_paired, swap_masks
from ._optimizers import dict_optimizers, dict_schedulers
from ._seed import set_ultimate_seed
