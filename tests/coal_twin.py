"""numpy float64 brute force of the modality coalitions (koaf_coal.hip, run/_coalitions.py), independent of the subset-weight
formula the kernel is handed.

The Shapley value is the mean of a player's marginal contribution over all P! orderings of the players.  The orderings are
enumerated, and what is counted is how many of them put exactly the set T in front of player i; phi_i is then the exactly rounded
(math.fsum) sum of count / P! * (v(T + i) - v(T)).  No factorial of a subset size appears anywhere.  The Shapley interaction index
of the pair (i, j) is, by its definition (Grabisch & Roubens 1999), the Shapley value of the merged player [ij] in the reduced game
of P - 1 players, taken of the pair's joint marginal contribution delta_ij(T) = v(T + i + j) - v(T + i) - v(T + j) + v(T): the same
enumeration over the orderings of the P - 2 other players and [ij]."""
import functools
import itertools
import math

import numpy as np


@functools.lru_cache(maxsize=None)
def _prefix_counts(n):
    """{bit mask of the n - 1 other items: the number of the n! orderings of n items that put exactly that set in front of item 0}"""
    counts = {}
    for perm in itertools.permutations(range(n)):
        at = perm.index(0)
        mask = sum(1 << (q - 1) for q in perm[:at])
        counts[mask] = counts.get(mask, 0) + 1
    assert sum(counts.values()) == math.factorial(n) and len(counts) == 1 << (n - 1)
    return counts


def _spread(mask, others):
    """the mask over `others` (a list of player indices) as a mask over the players"""
    return sum(1 << p for q, p in enumerate(others) if mask >> q & 1)


def shapley(v):
    """v [2^P, B] -> (phi [B, P], inter [B, P, P], loo [B, P], solo [B, P]) in float64"""
    v = np.asarray(v, dtype=np.float64)
    S, B = v.shape
    P = S.bit_length() - 1
    assert S == 1 << P and P >= 1
    phi, inter = np.zeros((B, P)), np.zeros((B, P, P))
    loo, solo = np.zeros((B, P)), np.zeros((B, P))
    total = math.factorial(P)
    for i in range(P):
        others = [p for p in range(P) if p != i]
        terms = [(c, _spread(m, others)) for m, c in _prefix_counts(P).items()]
        for b in range(B):
            phi[b, i] = math.fsum(c / total * (v[T | 1 << i, b] - v[T, b]) for c, T in terms)
        loo[:, i] = v[S - 1] - v[(S - 1) & ~(1 << i)]
        solo[:, i] = v[1 << i] - v[0]
    if P >= 2:
        total = math.factorial(P - 1)
        for i in range(P):
            for j in range(P):
                if i == j:
                    continue
                others = [p for p in range(P) if p not in (i, j)]
                terms = [(c, _spread(m, others)) for m, c in _prefix_counts(P - 1).items()]
                bi, bj = 1 << i, 1 << j
                for b in range(B):
                    inter[b, i, j] = math.fsum(c / total * (v[T | bi | bj, b] - v[T | bi, b] - v[T | bj, b] + v[T, b]) for c, T in terms)
    return phi, inter, loo, solo


def segment_of(seg_off, L):
    """[L] the input every token belongs to"""
    seg = np.zeros(L, dtype=np.int64)
    for i in range(len(seg_off) - 1):
        seg[seg_off[i]:seg_off[i + 1]] = i
    return seg


def tokens(tx, t0, seg_off, masks):
    """out [J, B, L, D]: tx where bit seg(l) of masks[j] is set, else t0 (B0 = 1 broadcasts)"""
    tx, t0 = np.asarray(tx), np.asarray(t0)
    B, L, D = tx.shape
    seg = segment_of(seg_off, L)
    t0 = np.broadcast_to(t0, tx.shape) if t0.shape[0] == 1 else t0
    present = (np.asarray(masks, dtype=np.int64)[:, None] >> seg[None, :]) & 1           # [J, L]
    return np.where(present[:, None, :, None].astype(bool), tx[None], t0[None]).astype(tx.dtype)
