"""Modality coalitions and their Shapley values (not in the reference).  With the inputs as players -- or groups of
inputs, `players` -- and

    v(S)[b] = F(x with every input outside S at its baseline)[b, t_b]

run.modal_coalitions returns all 2^P values and run.modal_shapley folds them into the Shapley values phi_i (which sum to
v(N) - v({})), the Shapley interaction index I_ij, the leave-one-out differences v(N) - v(N - i) (modal_ablation's number when the
baselines are zeros) and the stand-alone differences v({i}) - v({}).

Every multi-input model ends in feat(cat([tokens of input 0 | ... | tokens of input M - 1])) and C.finish, and in eval() mode the
token block of input m depends on input m only (models.token_layout names the blocks).  The sparse pass therefore runs the
encoders twice -- on the intact inputs and on the baselines, the latter at batch 1 when no baseline is a tensor -- keeps the two
token tensors, and gets every other coalition from koaf_coal_tokens (the splice) and the final FeaT alone.  sparse=False calls the
model on full copies: the yardstick.  Nothing here reads a value back to the host."""
from typing import NamedTuple

import torch

from .. import ops
from ._attr import _check_chunk, _inputs, resolve_baselines
from ._explain import _forward_main, _targets


class ModalShapley(NamedTuple):
    """phi (B, P), interaction (B, P, P), loo (B, P), solo (B, P): fp64 device tensors; values (2^P, B): the fp32 coalition values, row
    s = the coalition whose bit p says player p is present; v_full = values[-1], v_empty = values[0]: (B,)"""
    phi: torch.Tensor
    interaction: torch.Tensor
    loo: torch.Tensor
    solo: torch.Tensor
    values: torch.Tensor
    v_full: torch.Tensor
    v_empty: torch.Tensor


def player_masks(players, M):
    """the input-bit mask of every player.  players None: every one of the M inputs is its own player; else a partition of
    range(M) into P <= ops.COAL_MAX_M non-empty groups, e.g. [[0, 1, 2, 3], [4]] for imaging against clinical."""
    if players is None:
        groups = [[i] for i in range(M)]
    else:
        try:
            groups = [[int(i) for i in g] for g in players]
        except TypeError:
            raise ValueError(f"coalitions: players is None or a partition of the {M} input indices into groups, got {players!r}") from None
        flat = sorted(i for g in groups for i in g)
        if flat != list(range(M)) or any(len(g) == 0 for g in groups):
            raise ValueError(f"coalitions: players is a partition of the input indices 0 .. {M - 1} into non-empty groups, got {players!r}")
    if not 1 <= len(groups) <= ops.COAL_MAX_M:
        raise ValueError(f"coalitions: 1 <= players <= {ops.COAL_MAX_M}, got {len(groups)}")
    return [sum(1 << i for i in g) for g in groups]


def coalition_masks(pmasks):
    """the 2^P input-bit masks of the coalitions of players, row s = the union of the players whose bit is set in s"""
    return [sum(pm for p, pm in enumerate(pmasks) if s >> p & 1) for s in range(1 << len(pmasks))]


def _layout(model, M):
    """(the final FeaT, seg_off) of a model whose token layout has one block per input, in input order"""
    from ..models._common import token_layout
    try:
        lay = token_layout(model)
    except ValueError:
        raise ValueError(f"coalitions: {type(model).__name__} has no token layout (no final FeaT over per-input token blocks) for the "
                         f"sparse pass to splice: use sparse=False") from None
    if [s.input for s in lay.segments] != list(range(M)):
        raise ValueError(f"coalitions: the token layout names the inputs {[s.input for s in lay.segments]}, the call has {M}: use sparse=False")
    return lay.feat, [s.offset for s in lay.segments] + [lay.segments[-1].offset + lay.segments[-1].length]


def _base_tensor(x, b, rows=None):
    shape = tuple(x.shape) if rows is None else (rows,) + tuple(x.shape[1:])
    if torch.is_tensor(b):
        return b
    return torch.zeros(shape, dtype=x.dtype, device=x.device) if b is None else torch.full(shape, b, dtype=x.dtype, device=x.device)


def modal_coalitions(model, xs, target, baselines=None, players=None, chunk=8, sparse=True):
    """-> (values (S, B) fp32 device tensor, masks: the S = 2^P input-bit masks): values[s, b] = logit[b, target_b] of the model with
    the inputs outside masks[s] at their baselines; masks[0] = 0 (all baselines), masks[-1] = every input.  players: player_masks.
    baselines: resolve_baselines (None = zeros, a number, a tensor per input).  chunk: coalitions per model (sparse: final FeaT)
    pass, folded into the batch dimension (exact in eval() mode, refused in training mode).
    sparse (default): one forward of the intact inputs and one of the baselines -- at batch 1 when no baseline is a tensor -- keep
    the final FeaT's input tokens; every other coalition is ops.coal_tokens -> the final FeaT -> C.finish.  Valid only where the
    token block of an input depends on that input alone, so sparse=True needs model.eval() and a models.token_layout.
    sparse=False calls the model on full copies, the absent inputs replaced by their baselines: the yardstick.
    No parameter and no p.grad is touched; nothing is read back to the host."""
    xs_in = tuple(xs)
    M = len(xs_in)
    masks = coalition_masks(player_masks(players, M))
    S = len(masks)
    if sparse and model.training:
        raise ValueError("coalitions: sparse=True keeps encoder features across model passes, which is valid only where samples do not "
                         "interact: put the model in eval() mode, or use sparse=False with chunk=1")
    chunk = _check_chunk(model, chunk, S)
    if sparse:
        feat, seg_off = _layout(model, M)
    xs = _inputs(xs_in)
    bases = resolve_baselines(xs, baselines)
    B, dev = int(xs[0].shape[0]), xs[0].device
    tgt = _targets(target, xs)
    values = torch.empty((S, B), device=dev, dtype=torch.float32)
    if not sparse:
        bts = tuple(_base_tensor(x, b) for x, b in zip(xs, bases))
        with torch.no_grad():
            for k0 in range(0, S, chunk):
                J = min(chunk, S - k0)
                pts = tuple((x if masks[k0] >> m & 1 else bt) if J == 1 else
                            torch.cat([x if masks[k0 + j] >> m & 1 else bt for j in range(J)]) for m, (x, bt) in enumerate(zip(xs, bts)))
                values[k0:k0 + J] = _forward_main(model, pts).float().gather(1, tgt.repeat(J, 1)).reshape(J, B)
                del pts
        return values, masks
    from ..models import _common as C
    kept = []
    handle = feat.register_forward_pre_hook(lambda mod, args: kept.append(args[0].detach().float().contiguous()))
    try:
        with torch.no_grad():
            values[S - 1] = _forward_main(model, xs).float().gather(1, tgt).reshape(B)
            B0 = B if any(torch.is_tensor(b) for b in bases) else 1
            F0 = _forward_main(model, tuple(_base_tensor(x, b, rows=B0) for x, b in zip(xs, bases))).float()
            values[0] = F0.expand(B, -1).gather(1, tgt).reshape(B)
    finally:
        handle.remove()
    if len(kept) != 2 or kept[0].dim() != 3 or tuple(kept[1].shape) != (B0,) + tuple(kept[0].shape[1:]):
        raise RuntimeError(f"coalitions: the final FeaT ran {len(kept)} times in two forwards, or not on [B, L, D] tokens")
    tx, t0 = kept
    with torch.no_grad():
        for k0 in range(1, S - 1, chunk):
            J = min(chunk, S - 1 - k0)
            toks = ops.coal_tokens(tx, t0, seg_off, masks[k0:k0 + J])
            res = feat(toks.reshape((J * B,) + tuple(tx.shape[1:])))[0].reshape(J * B, -1)
            del toks
            out = C.finish(model.config, res)
            out = out["main"] if isinstance(out, dict) else out
            values[k0:k0 + J] = out.reshape(J * B, -1).float().gather(1, tgt.repeat(J, 1)).reshape(J, B)
    return values, masks


def modal_shapley(model, xs, target, baselines=None, players=None, chunk=8, sparse=True):
    """ModalShapley of logit[b, target_b] over the players (modal_coalitions' arguments): the 2^P coalition values folded by
    ops.shapley_fold.  phi.sum(1) equals v_full - v_empty up to fp64 rounding of the fp32 values (efficiency)."""
    values, masks = modal_coalitions(model, xs, target, baselines=baselines, players=players, chunk=chunk, sparse=sparse)
    phi, inter, loo, solo = ops.shapley_fold(values, len(masks).bit_length() - 1)
    return ModalShapley(phi, inter, loo, solo, values, values[-1], values[0])
