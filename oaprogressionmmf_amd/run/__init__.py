"""Step bodies and regimes of the reference's drivers (koafusion/run/train_prog_fus.py, eval_prog_fus.py) on the MI355X
path: train, validation (with its metrics table, various.calc_metrics_v2), evaluation and explanation, and the logistic-regression baselines of train_prog_clin.py.  The drivers' shell
(hydra, data loaders, tensorboard, fit()'s checkpoint bookkeeping) stays the reference's."""
from ._steps import downscale_inputs, train_epoch, train_step, predict_batch, val_epoch
from ._eval import eval_epoch, ensemble_eval_foldw, InferenceTimer
from ._graph import GraphedPredictor, GraphedTrainStep
from ._accum import GradientFold, micro_batch_weights, train_step_accum
from ._explain import (explain_epoch, ensemble_explain_foldw, modal_ablation, ablation_percent, input_gradients,
                       saliency_maps)
from ._gradcam import GradCam, cam_strides, gradcam
from ._attr import attribution_totals, integrated_gradients, quadrature, smoothgrad
from ._attnrel import AttnRelevance, attention_relevance
from ._occlusion import occlusion, occlusion_windows, touched_images
from ._coalitions import ModalShapley, coalition_masks, modal_coalitions, modal_shapley, player_masks
from ._clin import clin_design, clin_fit, clin_vars

__all__ = ["downscale_inputs", "train_epoch", "train_step", "predict_batch", "val_epoch", "eval_epoch", "ensemble_eval_foldw",
           "InferenceTimer", "GraphedPredictor", "GraphedTrainStep", "explain_epoch", "ensemble_explain_foldw", "modal_ablation",
           "ablation_percent", "input_gradients", "saliency_maps", "GradientFold", "micro_batch_weights", "train_step_accum", "GradCam",
           "cam_strides", "gradcam", "attribution_totals", "integrated_gradients", "quadrature", "smoothgrad", "clin_design", "clin_fit",
           "clin_vars", "AttnRelevance", "attention_relevance", "occlusion", "occlusion_windows", "touched_images", "ModalShapley",
           "coalition_masks", "modal_coalitions", "modal_shapley", "player_masks"]
