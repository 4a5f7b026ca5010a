"""float64 numpy restatement of the scores and the refined position of skp_tta_reduce_scored
(include/skp.h, A18) on a given average, and the planted cases of tests/test_gpu_tta_score.py.

Independent of product code.  For one (S, S) average ``a`` with first row-major maximum at
(r*, c*) and K the pixels with sqrt((r − r*)² + (c − c*)²) <= distance:
  peak = a[r*, c*];  concentration = Σ_K a / (Σ a + 1e-6);  coverage = num[r*, c*] / C;
  refined = (Σ_K r·a / (Σ_K a + 1e-6) + 0.5, Σ_K c·a / (Σ_K a + 1e-6) + 0.5).
"""
import numpy as np

import tta_ref


def disc(S, r, c, distance):
    """(S, S) bool: the pixels within ``distance`` of (r, c)."""
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    return np.sqrt((y - r) ** 2 + (x - c) ** 2) <= float(distance)


def scores_ref(avg, num, C, distance):
    """avg (B, n, S, S), num (B, S, S) -> dict of float64 arrays: peak, concentration, coverage
    (B, n), refined (B, n, 2), and disc_share (B, n) = (disc pixels inside the plane) / S²."""
    avg = np.asarray(avg, np.float64)
    B, n, S, _ = avg.shape
    out = dict(peak=np.zeros((B, n)), concentration=np.zeros((B, n)), coverage=np.zeros((B, n)),
               refined=np.zeros((B, n, 2)), disc_share=np.zeros((B, n)))
    rows, cols = np.mgrid[0:S, 0:S].astype(np.float64)
    for b in range(B):
        for t in range(n):
            a = avg[b, t]
            k = int(a.reshape(-1).argmax())      # numpy: the first occurrence
            r, c = divmod(k, S)
            keep = disc(S, r, c, distance)
            with np.errstate(invalid="ignore", over="ignore"):
                win = np.where(keep, a, 0.0)
                tot = win.sum()
                out["peak"][b, t] = a[r, c]
                out["concentration"][b, t] = tot / (a.sum() + 1e-6)
                out["coverage"][b, t] = np.asarray(num, np.float64)[b, r, c] / C
                out["refined"][b, t] = ((rows * win).sum() / (tot + 1e-6) + 0.5, (cols * win).sum() / (tot + 1e-6) + 0.5)
            out["disc_share"][b, t] = keep.sum() / float(S * S)
    return out


# ------------------------------------------------------------------------------------------ planted cases
# (B, C, n, S): S = 80 has two tile columns, the second partly outside the plane; S = 37 is odd.
PLANTED = ((1, 3, 6, 80), (2, 4, 6, 37))
# Per image: which copies are the identity (the others are out of view), and per token
# (kind, row, col) with kind "sharp" (a narrow bump on zero), "diffuse" (a near-constant plane
# with one slightly larger pixel) or "zero".  Rows 3 and 4 meet at a row-band edge, columns 63 and
# 64 at a tile-column edge; the corners clip the window on two sides, (0, S // 2) on one.
_PLAN = {
    (1, 3, 6, 80): [((True, False, True),
                     (("sharp", 0, 0), ("diffuse", 79, 79), ("sharp", 0, 40), ("diffuse", 3, 64),
                      ("sharp", 40, 63), ("diffuse", 41, 64)))],
    (2, 4, 6, 37): [((True, True, False, True),
                     (("sharp", 0, 0), ("diffuse", 36, 36), ("sharp", 0, 18), ("diffuse", 3, 20),
                      ("sharp", 4, 20), ("zero", 0, 0))),
                    ((False, True, False, False),
                     (("diffuse", 0, 0), ("sharp", 36, 36), ("diffuse", 0, 18), ("sharp", 3, 5),
                      ("diffuse", 4, 33), ("sharp", 18, 18)))],
}


def make_planted(shape):
    """Returns (maps, theta_inv, plan) with plan[b] = (identity flags of the copies, tokens).  An
    identity copy holds the token's base map, an out-of-view copy random values nobody sees."""
    shape = tuple(shape)
    B, C, n, S = shape
    plan = _PLAN[shape]
    g = np.random.default_rng([7, B, C, n, S])
    maps = g.random((B, C, n, S, S)).astype(np.float32)
    theta = np.zeros((B, C, 2, 3), np.float32)
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    for b, (ident, tokens) in enumerate(plan):
        for t, (kind, r, c) in enumerate(tokens):
            if kind == "sharp":      # a Gaussian of sigma 1 cut at distance 3, peak 1
                d2 = (y - r) ** 2 + (x - c) ** 2
                base = np.where(d2 <= 9.0, np.exp(-d2 / 2.0), 0.0)
            elif kind == "diffuse":  # 1% above the plane: far above the fp32 rounding of the identity grid
                base = np.full((S, S), 0.5)
                base[r, c] = 0.505
            else:
                base = np.zeros((S, S))
            for k in range(C):
                if ident[k]:
                    maps[b, k, t] = base.astype(np.float32)
        for k in range(C):
            theta[b, k] = tta_ref.IDENTITY if ident[k] else tta_ref.OUT_OF_VIEW
    return maps, theta, plan
