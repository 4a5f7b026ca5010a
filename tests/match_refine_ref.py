"""Numpy oracle of skp_match_refine (include/skp.h): skp_match_field's norms, dots and keys
(tests/match_field_ref.py: the exact fmaf, the chains in token order) restricted to the window that a
coarse field gives each pixel, with the same tie and unusable rules.

The dots of every pair are formed, whether or not the pair lies in a window: the window only decides
which keys take part, so a key here is the key of match_field_ref bit for bit.
"""
import numpy as np

import match_field_ref as R

F32 = R.F32
NEG_INF = R.NEG_INF


def windows(coarse, S, f, w):
    """coarse (Sc, Sc) int -> (has_prior (S²,), allowed (S², S²) bool): allowed[p, q] where q lies in W(p)."""
    Sc = S // f
    coarse = np.asarray(coarse).reshape(Sc, Sc).astype(np.int64)
    r, c = np.divmod(np.arange(S * S), S)
    m = coarse[r // f, c // f]
    prior = (m >= 0) & (m < Sc * Sc)
    ms = np.where(prior, m, 0)
    cr, cc = (ms // Sc) * f + r % f, (ms % Sc) * f + c % f
    qr, qc = np.divmod(np.arange(S * S), S)
    allowed = (np.abs(qr[None, :] - cr[:, None]) <= w) & (np.abs(qc[None, :] - cc[:, None]) <= w)
    return prior, allowed & prior[:, None]


def match_refine_one(x, y, coarse, f, w, dot=None):
    """One image: x, y (n, S, S) float32, coarse (Sc, Sc) -> (index (S, S) int32, score (S, S) float32)."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    n, S = x.shape[0], x.shape[-1]
    x, y = x.reshape(n, S * S), y.reshape(n, S * S)
    rx, okx = R.recip_norm(R.chain_norm(x))
    ry, oky = R.recip_norm(R.chain_norm(y))
    if dot is None:
        dot = R.chain_dot(x, y)
    with np.errstate(all="ignore"):
        key = (dot * ry[None, :]).astype(F32)
    key = np.where(np.isnan(key), NEG_INF, key)
    _, allowed = windows(coarse, S, f, w)
    allowed = allowed & oky[None, :]
    best = np.where(allowed, key, NEG_INF).max(axis=1)
    first = np.argmax(allowed & (key == best[:, None]), axis=1)      # the lowest q among the window's greatest keys
    with np.errstate(all="ignore"):
        sc = (key[np.arange(S * S), first] * rx).astype(F32)
    ok = okx & allowed.any(axis=1)
    index = np.where(ok, first, -1).astype(np.int32)
    score = np.where(ok, sc, NEG_INF).astype(F32)
    return index.reshape(S, S), score.reshape(S, S)


def match_refine(x, y, coarse, w):
    """x, y (B or 1, n, S, S), coarse (B, Sc, Sc) -> (index (B, S, S), score (B, S, S))."""
    B, S = coarse.shape[0], x.shape[-1]
    f = S // coarse.shape[-1]
    out = [match_refine_one(x[b if x.shape[0] > 1 else 0], y[b if y.shape[0] > 1 else 0], coarse[b], f, w)
           for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def pool(a, f):
    """(n, S, S) -> (n, S / f, S / f): the mean of each f × f cell, summed in float64 and rounded once."""
    n, S = a.shape[0], a.shape[-1]
    return a.astype(np.float64).reshape(n, S // f, f, S // f, f).mean(axis=(2, 4)).astype(F32)
