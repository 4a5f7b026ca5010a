"""float64 numpy restatement of the cross-image correspondence selection (eval.find_corresponding_points,
reference eval.py:159-195) and of the entropy skp_tta_reduce_entropy leaves, with the planted cases
that tests/test_corr_cpu.py, tests/test_gpu_corr.py and tests/golden/make_corr_golden.py share.

Independent of product code.
"""
import numpy as np

import tta_ref

# (B, C, n, S) of the selection cases and the number of tokens kept
CASES = ((3, 3, 12, 37), (2, 10, 12, 64), (4, 2, 16, 37))
K = 5


def entropy_ref(avg, scale=1.0):
    """(..., S, S) -> (...) float64: −Σ p·log p of softmax(scale · avg) over each plane, directly, with
    0·log 0 = 0.  A plane whose maximum is +inf gives NaN."""
    z = np.asarray(avg, np.float64) * float(scale)
    z = z.reshape(z.shape[:-2] + (-1,))
    m = z.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(z - m)                      # m = +inf: inf − inf = NaN
        p = e / e.sum(axis=-1, keepdims=True)
        plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), np.where(np.isnan(p), np.nan, 0.0))
    return -plogp.sum(axis=-1)


def sum_in_order(per_image):
    """(M, N) -> (N,): image 0's row, then image 1's added, and so on."""
    total = np.array(per_image[0], np.float64)
    for row in per_image[1:]:
        total = total + row
    return total


def rank(total, k):
    """The first k of a stable ascending argsort, NaN last."""
    return np.argsort(total, kind="stable")[:k].astype(np.int64)


def argmax_pos(planes):
    """(..., h, w) -> (..., 2) float32 (row + 0.5, col + 0.5) of the first row-major maximum."""
    planes = np.asarray(planes)
    w = planes.shape[-1]
    idx = planes.reshape(planes.shape[:-2] + (-1,)).argmax(axis=-1)
    return np.stack([idx // w + 0.5, idx % w + 0.5], axis=-1).astype(np.float32)


def corresponding_ref(maps, k):
    """maps (M, N, h, w) -> (points (M, k, 2) float32, indices (k,) int64, summed entropies (N,) float64)."""
    maps = np.asarray(maps)
    total = sum_in_order(entropy_ref(maps))
    idx = rank(total, k)
    return argmax_pos(maps[:, idx]), idx, total


def planted(shape, seed=0):
    """Seeded inputs of one selection case: (maps (B, C, n, S, S) float32, theta_inv (B, C, 2, 3)).

    tta_ref.make_case's noise (non-negative multiples of 1/4, four levels) plus, per image and token,
    a Gaussian bump of sigma 2 pixels, the same in every copy, at a seeded position in the middle
    third of the plane; token t's amplitude is 1 + 0.5·π(t) with π a seeded permutation, so every
    token has its own sharpness.  Copy c of image b takes the identity when b + c is even, else the
    rotation."""
    B, C, n, S = shape
    g = np.random.default_rng([seed, 159, B, C, n, S])
    maps = (g.integers(0, 4, (B, C, n, S, S)) / 4.0).astype(np.float32)
    amp = 1.0 + 0.5 * g.permutation(n)
    lo, hi = S // 3, S - S // 3
    rows, cols = g.integers(lo, hi, (B, n)), g.integers(lo, hi, (B, n))
    yy, xx = np.mgrid[0:S, 0:S]
    for b in range(B):
        for t in range(n):
            bump = amp[t] * np.exp(-((yy - rows[b, t]) ** 2 + (xx - cols[b, t]) ** 2) / (2.0 * 2.0 ** 2))
            maps[b, :, t] += bump.astype(np.float32)
    theta = np.stack([np.stack([tta_ref.IDENTITY if (b + c) % 2 == 0 else tta_ref.ROTATED for c in range(C)])
                      for b in range(B)])
    return maps, np.ascontiguousarray(theta, np.float32)


_AVG = {}


def planted_average(shape):
    """The float32 cast of the float64 TTA average of ``planted(shape)``: (B, n, S, S).  Computed once."""
    shape = tuple(shape)
    if shape not in _AVG:
        maps, theta = planted(shape)
        _AVG[shape] = tta_ref.tta_ref(maps, theta)[1].astype(np.float32)
        _AVG[shape].setflags(write=False)
    return _AVG[shape]
