"""numpy restatement of the k-peak selection of skp_tta_reduce_peaks (include/skp.h) and the
shared cases of tests/test_tta_peaks_cpu.py and tests/test_gpu_tta_peaks.py.

Independent of product code: ``num`` rounds of first-occurrence, NaN-first argmax, each followed by
the multiply with the (squared distance > radius²) mask in float32 (eval.py:62-111).
"""
import numpy as np

import tta_ref

F32 = np.float32


def argmax_nan_first(flat):
    """Index of the first NaN of a 1-D array, else of its first maximum (torch.argmax)."""
    nan = np.flatnonzero(np.isnan(flat))
    return int(nan[0]) if nan.size else int(np.argmax(flat))


def peaks_ref(avg, num, radius):
    """avg (T, S, S) float32 -> (pos (T, num, 2), values (T, num)) float32.  Round j takes the
    argmax of the map (position = (row + 0.5, col + 0.5), value = the map there), then multiplies
    the map by (dx² + dy² > radius²) as 1.0 / 0.0, dx = col − (col_j + 0.5), dy likewise, all in
    float32: a masked pixel is 0 (and can win), a masked inf is NaN (and wins)."""
    avg = np.asarray(avg)
    assert avg.dtype == F32 and avg.ndim == 3
    T, S, _ = avg.shape
    r2 = F32(radius ** 2)
    cols = np.arange(S, dtype=F32)[None, :]
    rows = np.arange(S, dtype=F32)[:, None]
    pos = np.zeros((T, num, 2), F32)
    val = np.zeros((T, num), F32)
    for t in range(T):
        m = avg[t].copy()
        for j in range(num):
            i = argmax_nan_first(m.reshape(-1))
            pos[t, j] = (F32(i // S) + F32(0.5), F32(i % S) + F32(0.5))
            val[t, j] = m.reshape(-1)[i]
            dx, dy = cols - pos[t, j, 1], rows - pos[t, j, 0]
            mask = ((dx * dx + dy * dy) > r2).astype(F32)
            with np.errstate(invalid="ignore"):
                m = (m * mask).astype(F32)
    return pos, val


# ------------------------------------------------------------------------------------------ cases
# Continuous cases (B, C, n, S): copy 0 is the identity and carries the planted bumps, copy 1 is
# rotated.  The other values are uniform in [0, 1), so an average elsewhere is below 1; a bump of
# height h averages to at least h / 2 and at most h + 1.
#   S = 96 (radius 4.8): per token (row, col, height) of bump 1, bump 2 and a third bump INSIDE the
#   disc of bump 1, higher than anything but bump 1 and (nearly) bump 2: it must not be picked.
#   Token 0's bump 1 at (3, 63): its disc spans rows 0..8 (three four-row bands, clipped at the top)
#   and columns 59..68 (both sides of the 64-column tile boundary).  Token 1's sits in the corner.
#   S = 512 (radius 25.6, the workload's): the disc spans 14 bands; bump 1 is within the radius of
#   the right edge, so its box is clipped.
CONTINUOUS = {
    (1, 2, 2, 96): (((3, 63, 8.0), (40, 20, 3.0), (5, 66, 2.9)),
                    ((93, 2, 8.0), (30, 70, 3.0), (91, 4, 2.9))),
    (1, 2, 1, 512): (((200, 500, 8.0), (300, 100, 3.0)),),
}


def make_continuous(shape):
    """-> (maps (B, C, n, S, S) float32, theta_inv (B, C, 2, 3) float32, plan) of a CONTINUOUS shape."""
    B, C, n, S = shape
    plan = CONTINUOUS[tuple(shape)]
    assert B == 1 and C == 2 and len(plan) == n
    g = np.random.default_rng([7, B, C, n, S])
    maps = g.random((B, C, n, S, S), dtype=np.float32)
    for t, bumps in enumerate(plan):
        for r, c, h in bumps:
            maps[0, 0, t, r, c] = h
    theta = np.stack([tta_ref.IDENTITY, tta_ref.ROTATED])[None]
    return maps, np.ascontiguousarray(theta, np.float32), plan


# (kind, shape): the quarter-valued shared shapes (ties are the rule; an all-zero token, an
# all-out-of-view image, a +inf pixel whose masked rounds are NaN) and the continuous ones
CASES = [("quarters", s) for s in tta_ref.SHAPES] + [("continuous", s) for s in CONTINUOUS]


def make(kind, shape):
    """-> (maps, theta_inv, plan or None)."""
    if kind == "quarters":
        maps, theta, _ = tta_ref.make_case(shape)
        return maps, theta, None
    return make_continuous(shape)
