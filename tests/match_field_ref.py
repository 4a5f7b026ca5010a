"""Numpy oracle of skp_match_field (include/skp.h): norms and dots as fp32 fmaf chains in token
order, the keys, the tie and unusable rules.

The fp32 fmaf is emulated exactly.  The product of two float32 is exact in float64 (48 significant
bits, exponents within float64's normal range).  TwoSum gives the float64 sum of product and addend
with its exact error; where the sum is inexact its last bit is forced odd (round to odd), which the
final rounding float64 -> float32 cannot round the wrong way, since 53 >= 2·24 + 2.
"""
import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def fmaf(a, b, c):
    """fmaf(a, b, c) of float32 arrays (broadcast), one rounding, as float32."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
        c = np.asarray(c, F32).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        step = np.where((err > 0) == (s > 0), 1, -1).astype(np.int64)   # away from zero when err has s's sign
        s = np.where(fix, (s.view(np.int64) + step).view(np.float64), s)
        return s.astype(F32)


def chain_norm(v):
    """(n, cols) -> (cols,) c_n with c_0 = 0, c_{t+1} = fmaf(v[t], v[t], c_t)."""
    c = np.zeros(v.shape[1], F32)
    for t in range(v.shape[0]):
        c = fmaf(v[t], v[t], c)
    return c


def chain_dot(x, y, rows=512):
    """(n, P), (n, Q) -> (P, Q) d_n with d_0 = 0, d_{t+1} = fmaf(x[t,p], y[t,q], d_t); ``rows`` of P at a
    time, so that the float64 temporaries stay small."""
    out = np.empty((x.shape[1], y.shape[1]), F32)
    for p0 in range(0, x.shape[1], rows):
        d = np.zeros((min(rows, x.shape[1] - p0), y.shape[1]), F32)
        for t in range(x.shape[0]):
            d = fmaf(x[t, p0:p0 + rows, None], y[t][None, :], d)
        out[p0:p0 + rows] = d
    return out


def recip_norm(nrm):
    """1 / sqrt(norm), both correctly rounded (sqrt through float64 is exact for float32), and the
    usable mask 0 < norm < inf."""
    with np.errstate(all="ignore"):
        ok = (nrm > 0) & (nrm < np.inf)
        root = np.sqrt(nrm.astype(np.float64)).astype(F32)
        return (F32(1.0) / root).astype(F32), ok


def match_field_one(x, y, dot=None):
    """One image: x (n, P), y (n, Q) float32 -> (index (P,) int32, score (P,) float32)."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    rx, okx = recip_norm(chain_norm(x))
    ry, oky = recip_norm(chain_norm(y))
    if dot is None:
        dot = chain_dot(x, y)
    with np.errstate(all="ignore"):
        key = (dot * ry[None, :]).astype(F32)
    key = np.where(np.isnan(key), NEG_INF, key)
    index = np.full(x.shape[1], -1, np.int32)
    score = np.full(x.shape[1], NEG_INF, F32)
    if oky.any():
        cols = np.flatnonzero(oky)
        sub = key[:, cols]
        first = np.argmax(sub, axis=1)   # numpy: the first of equal maxima, no NaN left in key
        with np.errstate(all="ignore"):
            sc = (sub[np.arange(len(first)), first] * rx).astype(F32)
        index = np.where(okx, cols[first], -1).astype(np.int32)
        score = np.where(okx, sc, NEG_INF).astype(F32)
    return index, score


def match_field(x, y):
    """x (B or 1, n, P), y (B or 1, n, Q) -> (index (B, P), score (B, P)); a shared operand's
    products are formed once per distinct pair."""
    B = max(x.shape[0], y.shape[0])
    out = [match_field_one(x[b if x.shape[0] > 1 else 0], y[b if y.shape[0] > 1 else 0]) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def bits_equal(a, b):
    """Bit for bit with −0.0 and +0.0 counted as equal (NaN never occurs in a score)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.int32) == b.view(np.int32)) | ((a == 0) & (b == 0))))
