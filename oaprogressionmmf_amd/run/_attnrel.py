"""Attention relevance of the FeaT fusion (not in the reference): which slices of a volume the fusion attends to, and how the CLS
token's information is drawn from the modalities -- read from the model's own routing, not from an ablation.

Two published rules, both a chain of per-layer matrices (koaf_attn_layer) that the model path only ever carries a row through from
the left (koaf_attn_apply):
    rollout (Abnar & Zuidema 2020)       A^_l = rows of (fuse_h(A_l) + I) divided by their sum;   R = A^_L ... A^_1
    grad    (Chefer et al. 2021, the     Abar_l = mean_h relu(dA_l * A_l);                         R = (I + Abar_L) ... (I + Abar_1)
             self-attention rule)
The final FeaT starts from the CLS row; the segment of an MRI with its own aggregator (no CLS token: state s is final token s of the
segment) is carried on through that aggregator's chain.  Rollout needs one forward; grad one forward and the backward of the fusion
transformers only (the autograd graph is cut at the trunk outputs, as run.gradcam cuts it).  koaf_attn_segsum forms the per-slice
and per-input totals.  No arithmetic runs in torch ops."""
from typing import NamedTuple

import torch

from .. import functional as KF
from .. import ops
from ..models import KoafTrunk
from ..models._common import token_layout
from ._explain import _forward_main, _targets

METHODS = ("rollout", "grad")


class AttnRelevance(NamedTuple):
    """tokens (B, n_i): the relevance of every token of input i; slices (B, K_i): summed over a slice's tokens (K = 1 for a
    radiograph or the clinical vector)"""
    tokens: torch.Tensor
    slices: torch.Tensor


def _layers(tape, feats, method, fuse):
    """{FeaT: [M_1 .. M_L]} from the taped calls; every FeaT in `feats` ran each of its layers exactly once"""
    where = {}
    for f in feats:
        for l in range(f.transformer.depth):
            where[getattr(f.transformer, f"attn_{l}")] = (f, l)
    main = torch.cuda.current_stream()
    mats = {f: [None] * f.transformer.depth for f in feats}
    for rec in tape.calls:
        if rec["module"] not in where:
            continue
        f, l = where[rec["module"]]
        if mats[f][l] is not None:
            raise RuntimeError("attention_relevance: an attention layer ran twice in one forward")
        if rec["stream"] != main:
            main.wait_stream(rec["stream"])                 # (an aggregator's lane: its tensors are read on this stream)
        attn, qkv, dout = rec["attn"], rec["qkv"], rec["dout"]
        for t in (attn, qkv, dout):
            if t is not None:
                t.record_stream(main)
        if method == "rollout":
            mats[f][l] = ops.attn_layer(attn, fuse)
        else:
            if dout is None:
                raise RuntimeError("attention_relevance: no gradient reached an attention layer's output")
            mats[f][l] = ops.attn_layer(attn, "grad", dout=dout.contiguous(), qkv=qkv.contiguous())
    for f in feats:
        if any(m is None for m in mats[f]):
            raise RuntimeError("attention_relevance: a fusion transformer of the token layout did not run")
    return mats


def _carry(r, mats, add_identity):
    for M in reversed(mats):
        r = ops.attn_apply(M, r_in=r, add_identity=add_identity)
    return r


def _record(model, xs, target, method):
    """one forward (method grad: and the backward of the fusion transformers) with the tape installed -> the AttnTape"""
    tape = KF.AttnTape()
    if KF.ATTN_TAPE is not None:
        raise RuntimeError("attention_relevance: a tape is already installed")
    KF.ATTN_TAPE = tape
    try:
        if method == "rollout":
            with torch.no_grad():
                _forward_main(model, tuple(x.detach() for x in xs))
        else:
            tgt = _targets(target, xs)
            leaves = []

            def hook(mod, args, out):
                leaves.append(out.detach().requires_grad_(True))
                return leaves[-1]
            params = [p for p in model.parameters() if p.requires_grad]
            handles = []
            try:
                for p in params:
                    p.requires_grad_(False)
                handles = [tr.register_forward_hook(hook) for tr in model.modules() if isinstance(tr, KoafTrunk)]
                with torch.enable_grad():
                    sel = _forward_main(model, tuple(x.detach() for x in xs)).gather(1, tgt).sum()
                    torch.autograd.grad(sel, leaves)
            finally:
                for h in handles:
                    h.remove()
                for p in params:
                    p.requires_grad_(True)
    finally:
        KF.ATTN_TAPE = None
    return tape


def attention_relevance(model, xs, target=None, *, method="rollout", fuse="mean"):
    """-> (tuple of AttnRelevance shaped like `xs`, totals (B, len(xs)), cls_self (B,)), in whatever mode the model is in
    (explanations: eval()).  method "rollout": class-agnostic, `target` is ignored, one forward under no_grad; fuse "mean" | "max" |
    "min" over heads.  method "grad": the relevance of logit[b, target_b]; parameters are frozen for the call and the graph is cut
    at the trunk outputs: the trunks keep nothing, no p.grad is touched.  totals: the per-input sums of the token relevances;
    cls_self: what the CLS row keeps on the CLS column(s).  With several CLS tokens the first one's row is followed."""
    if method not in METHODS:
        raise ValueError(f"Unknown method: {method}")
    if fuse not in ops.ATTN_MODES[:3]:
        raise ValueError(f"Unknown fuse: {fuse}")
    if method == "grad":
        if fuse != "mean":
            raise ValueError("attention_relevance: method grad averages the heads (fuse stays 'mean')")
        if target is None:
            raise ValueError("attention_relevance: method grad needs a target")
    lay = token_layout(model)                   # (ValueError for a model without a FeaT)
    if lay.ncls < 1:
        raise ValueError("attention_relevance: the final FeaT has no CLS token to start from")
    xs = tuple(xs)
    if sorted(s.input for s in lay.segments) != list(range(len(xs))):
        raise ValueError(f"attention_relevance: the model takes {len(lay.segments)} inputs, got {len(xs)}")
    feats = [lay.feat] + [s.agg for s in lay.segments if s.agg is not None]
    tape = _record(model, xs, target, method)
    mats = _layers(tape, feats, method, fuse)
    tape.calls = []
    add = method == "grad"
    B, n = int(mats[lay.feat][0].shape[0]), int(mats[lay.feat][0].shape[1])
    if sum(s.length for s in lay.segments) != n - lay.ncls:
        raise RuntimeError(f"attention_relevance: the token layout holds {sum(s.length for s in lay.segments)} tokens, the final FeaT "
                           f"ran on {n} - {lay.ncls}")
    e = torch.zeros((B, 1, n), device=mats[lay.feat][0].device, dtype=torch.float32)
    e[:, 0, 0] = 1.0
    r = _carry(e, mats[lay.feat], add)                                      # (B, 1, n): the CLS row of the final chain
    res, totals = [None] * len(xs), [None] * len(xs)
    for s in lay.segments:
        t = r[:, :, lay.ncls + s.offset:lay.ncls + s.offset + s.length].contiguous()
        if s.agg is not None:
            if int(mats[s.agg][0].shape[1]) != s.length:
                raise RuntimeError(f"attention_relevance: the aggregator of input {s.input} ran on {int(mats[s.agg][0].shape[1])} tokens, "
                                   f"its segment holds {s.length}")
            t = _carry(t, mats[s.agg], add)
        t = t.view(B, s.length)
        res[s.input] = AttnRelevance(t, ops.attn_segsum(t, 0, s.length // s.per_slice, s.per_slice))
        totals[s.input] = ops.attn_segsum(t, 0, 1, s.length)
    cls_self = ops.attn_segsum(r.view(B, n), 0, 1, lay.ncls).view(B)
    return tuple(res), torch.cat(totals, dim=1), cls_self
