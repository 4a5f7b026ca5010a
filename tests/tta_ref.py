"""float64 numpy restatement of skp_tta_reduce (include/skp.h, A18) and the shared cases of
tests/test_tta_cpu.py and tests/test_gpu_tta.py.

Independent of product code: affine grid (align_corners=False), bilinear taps with zero padding,
the ones-warp, the ratio with NaN -> 0 and the first-occurrence row-major argmax.
"""
import math

import numpy as np


def affine_grid(theta, S):
    """theta (2, 3) -> source pixel coordinates (ix, iy), each (S, S) float64, of every output pixel."""
    base = (2.0 * np.arange(S, dtype=np.float64) + 1.0) / S - 1.0      # linspace(-1, 1, S)·(S−1)/S
    bx, by = base[None, :], base[:, None]
    th = np.asarray(theta, np.float64)
    gx = th[0, 0] * bx + th[0, 1] * by + th[0, 2]
    gy = th[1, 0] * bx + th[1, 1] * by + th[1, 2]
    return ((gx + 1.0) * S - 1.0) / 2.0, ((gy + 1.0) * S - 1.0) / 2.0


def warp(planes, theta):
    """planes (n, S, S) -> grid_sample(planes, affine_grid(theta)), bilinear, zeros, in float64."""
    planes = np.asarray(planes, np.float64)
    S = planes.shape[-1]
    ix, iy = affine_grid(theta, S)
    x0, y0 = np.floor(ix), np.floor(iy)
    we, wn = ix - x0, iy - y0
    out = np.zeros(planes.shape, np.float64)
    for dy, dx, w in ((0, 0, (1 - wn) * (1 - we)), (0, 1, (1 - wn) * we), (1, 0, wn * (1 - we)), (1, 1, wn * we)):
        xx, yy = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
        ok = (xx >= 0) & (xx < S) & (yy >= 0) & (yy < S)
        v = planes[:, np.clip(yy, 0, S - 1), np.clip(xx, 0, S - 1)]
        with np.errstate(invalid="ignore"):     # an inf value under a zero weight is NaN, as in fp32
            out += np.where(ok, v, 0.0) * np.where(ok, w, 0.0)
    return out


def tta_ref(maps, theta_inv):
    """maps (B, C, n, S, S), theta_inv (B, C, 2, 3) -> (pos (B, n, 2), avg (B, n, S, S), num (B, S, S)),
    float64: avg = Σ_c warp(maps) / Σ_c warp(ones) with NaN -> 0, pos = (row + 0.5, col + 0.5) of its
    first row-major maximum."""
    B, C, n, S, _ = maps.shape
    avg = np.zeros((B, n, S, S), np.float64)
    num = np.zeros((B, S, S), np.float64)
    for b in range(B):
        tot = np.zeros((n, S, S), np.float64)
        for c in range(C):
            tot += warp(maps[b, c], theta_inv[b, c])
            num[b] += warp(np.ones((1, S, S)), theta_inv[b, c])[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            a = tot / num[b]
        avg[b] = np.where(np.isnan(a), 0.0, a)
    idx = avg.reshape(B, n, -1).argmax(axis=2)      # numpy: the first occurrence
    pos = np.stack([idx // S + 0.5, idx % S + 0.5], axis=-1).astype(np.float64)
    return pos, avg, num


# ------------------------------------------------------------------------------------------ cases
def theta_of(deg, scale, tx, ty):
    """The forward theta of invertable_transform.create_affine_matrix."""
    a = math.radians(deg)
    return np.array([[math.cos(a) * scale, math.sin(a) * scale, tx],
                     [-math.sin(a) * scale, math.cos(a) * scale, ty]], np.float32)


IDENTITY = theta_of(0.0, 1.0, 0.0, 0.0)
ROTATED = theta_of(30.0, 0.8, 0.25, -0.25)
OUT_OF_VIEW = theta_of(0.0, 1.0, 3.0, 0.0)      # a translate of 3.0: no source pixel in view
THETAS = (IDENTITY, ROTATED, OUT_OF_VIEW)

# (B, C, n, S): S = 37 is odd (S² a multiple of neither 4 nor 64), S = 64 spans several row bands
SHAPES = ((1, 1, 1, 37), (2, 3, 5, 37), (1, 3, 2, 64), (2, 10, 3, 64))
ALL_OUT_OF_VIEW = (2, 3, 5, 37)     # the case whose last image has every copy out of view


def make_case(shape, seed=0, special=True):
    """Seeded inputs of one shape: maps are non-negative multiples of 1/4 (4 levels, so ties are
    common); copy c of image b takes theta (b + c) mod 3, so every image mixes the identity, the
    rotation and an out-of-view copy.  With ``special``: the last image of ``ALL_OUT_OF_VIEW`` has every
    copy out of view, token 0 of image 0 is all zero in every copy, and (n > 2) token 1 of image 0
    holds a NaN pixel and a +inf pixel in copy 0.  Returns (maps, theta_inv, finite) with
    ``finite`` (B, n) False for the NaN/inf token."""
    shape = tuple(shape)
    B, C, n, S = shape
    g = np.random.default_rng([seed, B, C, n, S])
    maps = (g.integers(0, 4, (B, C, n, S, S)) / 4.0).astype(np.float32)
    theta = np.stack([np.stack([THETAS[(b + c) % 3] for c in range(C)]) for b in range(B)])
    finite = np.ones((B, n), bool)
    if special:
        if shape == ALL_OUT_OF_VIEW:
            theta[B - 1] = OUT_OF_VIEW
        if n > 1 or B > 1:
            maps[0, :, 0] = 0.0
        if n > 2:
            maps[0, 0, 1, S // 3, S // 2] = np.nan
            maps[0, 0, 1, S // 2, S // 3] = np.inf
            finite[0, 1] = False
    return maps, np.ascontiguousarray(theta, np.float32), finite
