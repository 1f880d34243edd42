"""Explanation regime of koafusion/run/eval_prog_fus.py (explain_epoch :410-479, ensemble_explain_foldw :481-512):
modality ablation.  The reference drives captum's FeatureAblation with one feature id per input tensor, no
baselines (= zeros) and one perturbation per evaluation; for that call captum's rule reduces to

    attr[b, m] = f(x)[b, target_b] - f(x with modality m zeroed)[b, target_b]

replicated over every element of input m (so the reference's mean over elements returns the difference itself).
Here the M + 1 forwards run on the HIP path and only the (B, M) differences leave the device.

Not in the reference: input gradients.  input_gradients / saliency_maps return d logit[b, target_b] / d x_m for every input
(one forward and one backward through the HIP path, the trunks' data gradient down to the image included), and
explain_epoch(explain_fn="input_x_grad") accumulates the per-modality totals sum(x_m * grad_m) -- the first-order estimate of
what the ablation measures with M + 1 forwards.  Class-activation maps (run/_gradcam.py): explain_epoch(explain_fn="gradcam")
accumulates the per-slice map sums and hands the Grad-CAM volumes to the sink.  Path attributions (run/_attr.py):
explain_epoch(explain_fn="integrated_gradients" | "smoothgrad") accumulates the per-modality totals of the maps and hands the
maps to the sink.  Occlusion maps (run/_occlusion.py): explain_epoch(explain_fn="occlusion"), in the same way.  Modality Shapley
values (run/_coalitions.py): explain_epoch(explain_fn="modal_shapley") accumulates them with their interactions."""
from collections import defaultdict

import numpy as np
import torch

from .. import ops
from ._eval import _extract_modal
from ._steps import downscale_inputs


def _forward_main(model, xs):
    out = model(*xs)
    out = out["main"] if isinstance(out, dict) else out            # output_type "dict" / "main" (the captum path)
    return out.reshape(out.shape[0], -1)


def modal_ablation(model, xs, target):
    """(B, M) fp32 device tensor of the attributions above; `target` (B,) or (B, 1) integer class per sample."""
    tgt = torch.as_tensor(target).to(xs[0].device).long().reshape(-1, 1)
    if tgt.shape[0] == 1 and xs[0].shape[0] > 1:                   # a squeezed single target applies to every row
        tgt = tgt.expand(xs[0].shape[0], 1)
    with torch.no_grad():
        base = _forward_main(model, xs).gather(1, tgt)
        cols = []
        for m in range(len(xs)):
            ablated = tuple(torch.zeros_like(x) if j == m else x for j, x in enumerate(xs))
            cols.append(base - _forward_main(model, ablated).gather(1, tgt))
    return torch.cat(cols, dim=1)


def _targets(target, xs):
    tgt = torch.as_tensor(target).to(xs[0].device).long().reshape(-1, 1)
    if tgt.shape[0] == 1 and xs[0].shape[0] > 1:                   # a squeezed single target applies to every row
        tgt = tgt.expand(xs[0].shape[0], 1)
    return tgt


def input_gradients(model, xs, target):
    """tuple shaped like `xs` of d logit[b, target_b] / d x_m (fp32 device tensors), in whatever mode the model is in
    (explanations: eval()).  The gradients are with respect to what the model receives.  Parameters are frozen for the call:
    no weight gradient is formed and no p.grad is touched."""
    tgt = _targets(target, xs)
    leaves = tuple(x.detach().requires_grad_(True) for x in xs)
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.requires_grad_(False)
    try:
        with torch.enable_grad():
            sel = _forward_main(model, leaves).gather(1, tgt).sum()
            grads = torch.autograd.grad(sel, leaves)
    finally:
        for p in params:
            p.requires_grad_(True)
    return tuple(g.detach() for g in grads)


SALIENCY_KINDS = ("grad", "input_x_grad")


def saliency_maps(model, xs, target, kind="grad"):
    """per input, the gradient map ("grad") or gradient x input ("input_x_grad"), shaped like the input"""
    if kind not in SALIENCY_KINDS:
        raise ValueError(f"Unknown saliency kind: {kind}")
    grads = input_gradients(model, xs, target)
    if kind == "grad":
        return grads
    return tuple(x.detach() * g for x, g in zip(xs, grads))


def input_x_grad_totals(xs, grads):
    """(B, M) fp32 device tensor of sum(x_m * grad_m) per sample and modality (koaf_rowdot: fixed summation order)"""
    return torch.stack([ops.rowdot(x.detach().float(), g) for x, g in zip(xs, grads)], dim=1)


def ablation_percent(attrs):
    """eval_prog_fus.py:456-459: rows normalised to unit L1, absolute value, per cent rounded to 3 decimals
    (fp32 arithmetic on the CPU copy, as there)."""
    t = torch.as_tensor(attrs, dtype=torch.float32).to("cpu")
    t = t / torch.sum(torch.abs(t), dim=1, keepdim=True)
    return np.round(np.abs(t.numpy()) * 100., decimals=3)


EXPLAIN_FNS = ("modal_abl", "modal_shapley", "input_x_grad", "gradcam", "integrated_gradients", "smoothgrad", "attn_rollout", "attn_grad",
               "occlusion")


def explain_epoch(model, loader, modals, downscale=None, device="cuda", explain_fn="modal_abl", sink=None, explain_kwargs=None):
    """One pass of an eval()-mode model over `loader`; returns the reference's accumulator dict: exam_knee_id,
    target, modal_names, modal_abl_attrs, modal_abl_percent (python lists, loader order).
    explain_fn="input_x_grad" (not in the reference): the same dict with ixg_attrs = sum(x_m * grad_m) per modality and
    ixg_percent (ablation_percent of those) instead, for one forward and one backward per batch.  The gradient x input maps
    themselves (device tensors shaped like the inputs the model receives, i.e. after `downscale`) go to
    sink(exam_knee_ids, modals, maps) when a sink is given, and never into the returned lists.
    explain_fn="gradcam" (not in the reference): exam_knee_id, target, modal_names and gradcam_slice_scores -- per sample, one list
    per modality of the K per-slice sums of the un-normalised ReLU'd low-resolution Grad-CAM map ([] for a modality without an
    encoder trunk).  The maps (run.gradcam defaults: normalised per sample, shaped like the inputs; None for a trunk-less
    modality) go to the sink in the same way.
    explain_fn="integrated_gradients" (not in the reference): ig_attrs = the per-modality sums of the run.integrated_gradients
    maps, ig_percent (ablation_percent of those) and ig_delta = the per-sample completeness residual sum_m ig_attrs - (F(x) -
    F(baseline)).  explain_fn="smoothgrad": sg_attrs = sum(x_m * map_m) of the run.smoothgrad maps and sg_percent.  Both hand
    their maps to the sink as "input_x_grad" does, and both pass `explain_kwargs` (a dict: n_steps, method, baselines, chunk /
    n_samples, noise_level, seed, kind, chunk) to the function; the other keys take no keywords.
    explain_fn="attn_rollout" | "attn_grad" (not in the reference; run/_attnrel.py): attn_attrs = the per-modality totals of the
    attention relevance of the fusion transformers, attn_percent (ablation_percent of those) and attn_slice_scores -- per sample, one
    list per modality of the K per-slice relevances.  The AttnRelevance tuples go to the sink.  explain_kwargs: `fuse` (rollout).
    explain_fn="occlusion" (the recipe's third key; run/_occlusion.py): occl_attrs = the per-modality sums of the run.occlusion maps
    (0 for an input whose window is None) and occl_percent (ablation_percent of those).  The maps go to the sink as the other map
    keys' do.  explain_kwargs: sliding_window_shapes (required), strides, baselines, chunk, sparse.
    explain_fn="modal_shapley" (not in the reference; run/_coalitions.py): shap_attrs = the Shapley values of the modalities (or of
    the `players`) over the 2^P coalitions of inputs, shap_percent (ablation_percent of those), shap_interactions (per sample the
    P x P Shapley interaction index), shap_loo = v(N) - v(N - i), shap_solo = v({i}) - v({}) and shap_delta = the per-sample
    efficiency residual sum_i phi_i - (v(N) - v({})).  The ModalShapley tuples go to the sink.  explain_kwargs: baselines, players,
    chunk, sparse."""
    if explain_fn not in EXPLAIN_FNS:
        raise ValueError(f"Unknown explain_fn: {explain_fn}")
    kwargs = dict(explain_kwargs or {})
    attn_kw = explain_fn in ("attn_rollout", "attn_grad") and set(kwargs) == {"fuse"}
    if kwargs and explain_fn not in ("integrated_gradients", "smoothgrad", "occlusion", "modal_shapley") and not attn_kw:
        raise ValueError(f"explain_fn {explain_fn} takes no explain_kwargs, got {sorted(kwargs)}")
    kwargs.pop("return_delta", None)
    kwargs.pop("return_deltas", None)
    field = {"modal_abl": "modal_abl", "integrated_gradients": "ig", "smoothgrad": "sg", "attn_rollout": "attn",
             "attn_grad": "attn", "occlusion": "occl", "modal_shapley": "shap"}.get(explain_fn, "ixg")
    acc = defaultdict(list)
    modals = list(modals)
    for batch in loader:
        xs = tuple(_extract_modal(batch, m).to(device) for m in modals)
        ys = torch.as_tensor(batch["target"])
        with torch.no_grad():
            xs = tuple(downscale_inputs(xs, downscale))
        if explain_fn == "gradcam":
            from ._gradcam import gradcam
            cams = gradcam(model, xs, ys.squeeze())
            scores = [c.slice_scores.to("cpu").numpy().tolist() if c is not None else None for c in cams]
            if sink is not None:
                sink(list(batch[("-", "exam_knee_id")]), modals, tuple(c.map if c is not None else None for c in cams))
            nb = xs[0].shape[0]
            acc["exam_knee_id"].extend(batch[("-", "exam_knee_id")])
            acc["target"].extend(ys.to("cpu").numpy().tolist())
            acc["modal_names"].extend([modals, ] * nb)
            acc["gradcam_slice_scores"].extend([[s[b] if s is not None else [] for s in scores] for b in range(nb)])
            continue
        delta = scores = shap = None
        if explain_fn in ("attn_rollout", "attn_grad"):
            from ._attnrel import attention_relevance
            rel, totals, _ = attention_relevance(model, xs, ys.squeeze(), method=explain_fn[5:], **kwargs)
            attrs = totals.to("cpu")
            scores = [r.slices.to("cpu").numpy().tolist() for r in rel]
            if sink is not None:
                sink(list(batch[("-", "exam_knee_id")]), modals, rel)
        elif explain_fn == "modal_abl":
            attrs = modal_ablation(model, xs, ys.squeeze()).to("cpu")
        elif explain_fn == "modal_shapley":
            from ._coalitions import modal_shapley
            shap = modal_shapley(model, xs, ys.squeeze(), **kwargs)
            attrs = shap.phi.float().to("cpu")
            if sink is not None:
                sink(list(batch[("-", "exam_knee_id")]), modals, shap)
        elif explain_fn == "integrated_gradients":
            from ._attr import attribution_totals, integrated_gradients
            maps, delta = integrated_gradients(model, xs, ys.squeeze(), return_delta=True, **kwargs)
            attrs = attribution_totals(maps).to("cpu")
            if sink is not None:
                sink(list(batch[("-", "exam_knee_id")]), modals, maps)
        elif explain_fn == "smoothgrad":
            from ._attr import smoothgrad
            maps = smoothgrad(model, xs, ys.squeeze(), **kwargs)
            attrs = input_x_grad_totals(xs, maps).to("cpu")
            if sink is not None:
                sink(list(batch[("-", "exam_knee_id")]), modals, maps)
        elif explain_fn == "occlusion":
            from ._occlusion import occlusion, occlusion_totals
            maps = occlusion(model, xs, ys.squeeze(), **kwargs)
            attrs = occlusion_totals(maps, xs).to("cpu")
            if sink is not None:
                sink(list(batch[("-", "exam_knee_id")]), modals, maps)
        else:
            grads = input_gradients(model, xs, ys.squeeze())
            attrs = input_x_grad_totals(xs, grads).to("cpu")
            if sink is not None:
                sink(list(batch[("-", "exam_knee_id")]), modals, tuple(x.detach() * g for x, g in zip(xs, grads)))
        acc["exam_knee_id"].extend(batch[("-", "exam_knee_id")])
        acc["target"].extend(ys.to("cpu").numpy().tolist())
        acc["modal_names"].extend([modals, ] * attrs.shape[0])
        acc[f"{field}_attrs"].extend(attrs.numpy().tolist())
        acc[f"{field}_percent"].extend(ablation_percent(attrs).tolist())
        if scores is not None:
            acc["attn_slice_scores"].extend([[sc[b] for sc in scores] for b in range(attrs.shape[0])])
        if shap is not None:
            acc["shap_interactions"].extend(shap.interaction.to("cpu").numpy().tolist())
            acc["shap_loo"].extend(shap.loo.to("cpu").numpy().tolist())
            acc["shap_solo"].extend(shap.solo.to("cpu").numpy().tolist())
            acc["shap_delta"].extend((shap.phi.sum(dim=1) - (shap.v_full.double() - shap.v_empty.double())).to("cpu").numpy().tolist())
        if delta is not None:
            acc["ig_delta"].extend(delta.to("cpu").numpy().tolist())
    return dict(acc)


def ensemble_explain_foldw(raw_foldw, prefix="modal_abl"):
    """Inner 1:1 merge of the folds on exam_knee_id (first fold's order; target / modal_names from the first fold),
    per-fold columns modal_abl_attrs__k / modal_abl_percent__k, and modal_abl_percent = fold mean of the per-fold
    per-cent rows renormalised to sum 1 (a fraction, as the reference leaves it; float64).
    prefix: the field family to merge -- "modal_abl" (the reference's), or "ixg" for explain_epoch(explain_fn="input_x_grad"), "ig" / "sg"
    for "integrated_gradients" / "smoothgrad", "attn" for "attn_rollout" / "attn_grad", "occl" for "occlusion", "shap" for
    "modal_shapley"."""
    folds = list(raw_foldw)
    if not folds:
        raise ValueError("no folds to ensemble")
    pos = {}
    for k in folds:
        ids = raw_foldw[k]["exam_knee_id"]
        pos[k] = dict(zip(ids, range(len(ids))))
        if len(pos[k]) != len(ids):
            raise ValueError(f"fold {k}: exam_knee_id values are not unique (1:1 merge)")
    k0 = folds[0]
    common = set(pos[k0]).intersection(*(pos[k].keys() for k in folds[1:]))
    ids = [e for e in raw_foldw[k0]["exam_knee_id"] if e in common]
    ens = {"exam_knee_id": ids}
    for field in ("target", "modal_names"):
        ens[field] = [raw_foldw[k0][field][pos[k0][e]] for e in ids]
    stack = []
    for k in folds:
        rows = [pos[k][e] for e in ids]
        ens[f"{prefix}_attrs__{k}"] = [raw_foldw[k][f"{prefix}_attrs"][r] for r in rows]
        ens[f"{prefix}_percent__{k}"] = [raw_foldw[k][f"{prefix}_percent"][r] for r in rows]
        if ids:
            stack.append(np.asarray(ens[f"{prefix}_percent__{k}"], dtype=np.float64).reshape(len(ids), -1))
    if not ids:
        ens[f"{prefix}_percent"] = []
        return ens
    mean = np.mean(np.stack(stack, axis=1), axis=1)                  # samples x modals
    ens[f"{prefix}_percent"] = (mean / np.sum(mean, axis=1, keepdims=True)).tolist()
    return ens
