"""float64 numpy restatements of the objective kernels (A4-A7, A11, A12 and the bilinear resize), and
the inputs that tests/test_loss_ref_cpu.py, tests/test_gpu_losses.py and tests/test_gpu_resize.py share.

Independent of product code.  Discrete decisions are taken exactly and everything after them is float64:
  peaks          the k-max positions are the oracle's (argmax compares input values only; the mask
                 distances are sums of squared half-integers, exact in fp32, and never equal (0.05·h)²);
  warp           the sampling coordinates are the oracle's fp32 ``_grid`` (they are the definition: a
                 float64 grid moves samples by 1e-5); floor, the four weights, the zero padding and the
                 sums are float64;
  resize         ``O.bilinear_matrix``'s taps, products and sums in float64;
  weighted_avg   the argmax and the cut sqrt(dr² + dc²) > distance (integers: exact), then float64.
Positions are (row, col) pixel centres (index + 0.5), as in the oracle.
"""
import math

import numpy as np

from oracle import skp_oracle as O

F32 = np.float32
F64 = np.float64


# ------------------------------------------------------------------------------------------ restatements
def peaks(A, num):
    """(num, T, 2) float32: O.find_k_max_pixels' positions (pixels, +0.5)."""
    return O.find_k_max_pixels(np.asarray(A, F32), num)


def peaks_masked(A, num):
    """peaks and the map after its num masks (what ops.find_k_max_pixels(return_masked=True) returns)."""
    m = np.asarray(A, F32)
    pos = peaks(m, num)
    for q in range(num):
        m = O.mask_radius(m, pos[q], 0.05 * m.shape[1])
    return pos, m


def _gauss_mean(centres, size, sigma):
    """centres (num, T, 2) float64 pixels -> (T, size, size): mean over num of exp(−d²/2σ²)."""
    g = np.arange(size, dtype=F64) + 0.5
    di = g[None, None, :, None] - centres[:, :, 0, None, None]
    dj = g[None, None, None, :] - centres[:, :, 1, None, None]
    return np.exp(-(di * di + dj * dj) / (2.0 * float(sigma) ** 2)).mean(axis=0)


def gaussian_targets(pos, size, sigma):
    """pos (num, T, 2) or (T, 2) in units of the map side -> (T, size, size) float64."""
    pos = np.asarray(pos, F64)
    if pos.ndim == 2:
        pos = pos[None]
    return _gauss_mean(pos * float(size), size, sigma)


def sharpening(A, sigma, num, gout=1.0):
    """mean((A − target)²) with the target centred on the peaks; square maps only.  gout: the upstream
    gradient, a scalar or one value per row.  Returns (loss, dA (T, S, S), pos (num, T, 2) float32 pixels)."""
    A = np.asarray(A, F32)
    T, S, S2 = A.shape
    if S != S2:
        raise ValueError(f"sharpening is defined for square maps, got {S}x{S2}")
    pos = peaks(A, num)
    diff = A.astype(F64) - _gauss_mean(pos.astype(F64) + 0.0, S, sigma)
    g = np.asarray(gout, F64).reshape(-1, 1, 1)
    return (diff ** 2).mean(), (2.0 / diff.size) * diff * g, pos


def _taps64(ix, iy, H, W):
    """The four bilinear taps of fp32 coordinates (H, W): (row, col, weight·in_range) in float64."""
    ix, iy = ix.astype(F64), iy.astype(F64)
    x0, y0 = np.floor(ix), np.floor(iy)
    we, wn = ix - x0, iy - y0
    out = []
    for dy, dx, w in ((0, 0, (1 - wn) * (1 - we)), (0, 1, (1 - wn) * we), (1, 0, wn * (1 - we)), (1, 1, wn * we)):
        yy, xx = (y0 + dy).astype(np.int64), (x0 + dx).astype(np.int64)
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        out.append((np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), w * ok))
    return out


def warp(img, theta):
    """grid_sample(img, affine_grid(theta)), bilinear, zeros, align_corners=False.  img (B, C, H, W)."""
    img = np.asarray(img, F64)
    B, C, H, W = img.shape
    ix, iy = O._grid(np.asarray(theta, F32).reshape(B, 2, 3), H, W)
    out = np.zeros((B, C, H, W), F64)
    for b in range(B):
        for yy, xx, w in _taps64(ix[b], iy[b], H, W):
            out[b] += img[b][:, yy, xx] * w[None]
    return out


def warp_adjoint(g, theta, H, W):
    """Adjoint of warp with respect to its image: g (B, C, H, W) -> (B, C, H, W)."""
    g = np.asarray(g, F64)
    B, C = g.shape[:2]
    ix, iy = O._grid(np.asarray(theta, F32).reshape(B, 2, 3), H, W)
    gin = np.zeros((B, C, H, W), F64)
    for b in range(B):
        for yy, xx, w in _taps64(ix[b], iy[b], H, W):
            for c in range(C):
                np.add.at(gin[b, c], (yy, xx), g[b, c] * w)
    return gin


def equivariance(A, At, theta_inv, gout=1.0):
    """mean((A − warp(At, θ⁻¹))²): (loss, dA, dAt).  theta_inv (2, 3) as ops.equivariance_loss_single takes it."""
    A = np.asarray(A, F32)
    ti = np.asarray(theta_inv, F32).reshape(1, 2, 3)
    diff = A.astype(F64) - warp(np.asarray(At, F32)[None], ti)[0]
    dA = (2.0 / diff.size) * diff * float(gout)
    return (diff ** 2).mean(), dA, warp_adjoint(-dA[None], ti, A.shape[1], A.shape[2])[0]


def per_image(fn, nb, gouts, *stacks):
    """A batched loss as its nb single-image losses: stacks of (nb·T, S, S) rows, fn(rows..., b, gout) ->
    (loss, grads...).  Returns ((nb,) losses, the grads concatenated over the images)."""
    T = stacks[0].shape[0] // nb
    res = [fn(*(s[b * T:(b + 1) * T] for s in stacks), b, gouts[b]) for b in range(nb)]
    return (np.array([r[0] for r in res]),) + tuple(np.concatenate([r[k] for r in res]) for k in range(1, len(res[0])))


def weighted_avg(m, distance):
    """eval.pixel_from_weighted_avg: (pos (T, 2) float64, the mutated float32 map)."""
    m = np.asarray(m, F32).copy()
    T, h, w = m.shape
    r, c = np.mgrid[0:h, 0:w]
    if distance != -1:
        p = O.find_max_pixel(m).astype(np.int64)
        d2 = (r[None] - p[:, 0, None, None]) ** 2 + (c[None] - p[:, 1, None, None]) ** 2   # integers
        m[np.sqrt(d2.astype(F64)) > float(distance)] = 0.0
    v = m.astype(F64)
    nm = v / (v.sum(axis=(1, 2), keepdims=True) + 1e-6)
    return np.stack([(r[None] * nm).sum(axis=(1, 2)), (c[None] * nm).sum(axis=(1, 2))], axis=-1) + 0.5, m


def resize(x, Ro):
    """(C, R, R) -> (C, Ro, Ro): F.interpolate(bilinear, align_corners=False)."""
    M = O.bilinear_matrix(x.shape[-1], Ro).astype(F64)
    return np.einsum("yi,cij,xj->cyx", M, np.asarray(x, F64), M)


def resize_adjoint(g, R):
    """(C, Ro, Ro) -> (C, R, R): the adjoint of resize."""
    M = O.bilinear_matrix(R, g.shape[-1]).astype(F64)
    return np.einsum("yi,cyx,xj->cij", M, np.asarray(g, F64), M)


def aggregate_bwd(shape, n_layers, dmap, Ro, indices):
    """d collect_maps / d each of n_layers captured layers of ``shape`` (BH, R², N) for dmap (n, Ro, Ro) at
    the tokens ``indices`` (duplicates add): the resize adjoint, the mean's 1 / (layers·BH), the gather's
    scatter, broadcast over BH.  (BH, R², N) float64, the same for every layer."""
    BH, RR, N = shape
    R = int(round(RR ** 0.5))
    g = resize_adjoint(dmap, R) / float(n_layers * BH)
    full = np.zeros((N, R, R), F64)
    np.add.at(full, np.asarray(indices), g)
    return np.broadcast_to(full.reshape(N, RR).T[None], (BH, RR, N))


def err(got, ref):
    """max|got − ref| / max(1, max|ref|): the figure every tolerance of these tests is stated in."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


# ------------------------------------------------------------------------------------------ shared inputs
# Map sides chosen against the kernels (one 1024-thread workgroup per row, float4 loads when HW % 4 == 0
# and the row is 16-B aligned, 256-thread elementwise blocks): 3 has fewer pixels than 16 subjects (and, like 7, a mask radius that holds no pixel); 7 is
# one partial wave and odd (rows alternate alignment: the scalar path); 30 stays below 1024 threads with
# HW % 4 == 0; 33 is just past one trip, scalar; 64 is one float4 per thread; 68 is two float4 trips, the
# second partial.  128 is the production side, used once per operation with T = 2.
SIZES = (3, 7, 30, 33, 64, 68)
PROD = 128
TS = (1, 5)
KINDS = ("peaky", "signed", "ties")
NUMS = (1, 2, 3, 16)
SIGMAS = (1.0, 2.0, 9.0)
WEIGHTS = (1.0, -2.0, 0.0)      # the batch forms' upstream gradient per image; the zero must reach dA


def maps(kind, T, S, salt=0, W=None):
    """(T, S, W or S) float32.  peaky: attention-like; signed: masked zeros beat unmasked negatives; ties:
    integers 0..2; special: ties with a NaN row, a +inf row and an all −inf row (exact-output tests only)."""
    rng = np.random.default_rng([("peaky", "signed", "ties", "special").index(kind), T, S, salt])
    shape = (T, S, W or S)
    if kind == "peaky":
        return (rng.random(shape) ** 8).astype(F32)
    if kind == "signed":
        return rng.standard_normal(shape).astype(F32)
    m = rng.integers(0, 3, shape).astype(F32)
    if kind == "special":
        m[1 % T, S // 2, S // 3] = np.nan
        m[1 % T, S - 1, S - 1] = np.nan
        m[2 % T, 0, S - 1] = np.inf
        if T > 3:
            m[3] = -np.inf
    return m


def upstream(T, S):
    """The scalar upstream gradient of the loss tests: 0.375·T·S² (exact in fp32), so that
    dA = 2/(T·S²)·diff·gout = 0.75·diff is of the maps' own magnitude at every size and the error
    figure's max(1, ·) denominator hides nothing."""
    return 0.375 * T * S * S


def sharpening_cases(S):
    """(kind, T, num, sigma) of the single-image sharpening tests at side S: kinds × T × subjects, with
    sigma cycling so that every sigma meets every kind and every subject count over the sizes."""
    if S == PROD:
        return [("peaky", 2, 3, 2.0)]
    out = []
    for T in TS:
        for ki, kind in enumerate(KINDS):
            for ni, num in enumerate(NUMS):
                out.append((kind, T, num, SIGMAS[(ki + ni + T + SIZES.index(S)) % 3]))
    return out


def batch_cases(S):
    """(kind, T, num, sigma) of the nb = 3 batch forms at side S."""
    i = SIZES.index(S)
    return [(KINDS[(i + T) % 3], T, NUMS[(i + T) % 4], SIGMAS[(i + T) % 3]) for T in TS]


def thetas(H, W):
    """name -> θ (2, 3) float32, the affine cases of the warp and equivariance tests."""
    c, s = 0.8 * math.cos(math.radians(30.0)), 0.8 * math.sin(math.radians(30.0))
    t = {
        "identity": [[1, 0, 0], [0, 1, 0]],
        "shift": [[1, 0, 2.0 / W], [0, 1, -4.0 / H]],      # whole pixels: weights 0 or 1, taps on the border
        "rot30": [[c, s, 0.1], [-s, c, -0.2]],
        "zoomout": [[2.5, 0, 0], [0, 2.5, 0]],             # most taps outside
        "outside": [[1, 0, 3], [0, 1, 0]],                 # every tap outside
        "reflect": [[-1, 0, 0], [0, 1, 0]],
        "rot90": [[0, 1, 0], [-1, 0, 0]],
    }
    return {k: np.array(v, F32) for k, v in t.items()}


THETA_NAMES = ("identity", "shift", "rot30", "zoomout", "outside", "reflect", "rot90")
BATCH_THETAS = ("rot30", "shift", "zoomout")


def equiv_cases(S):
    """(T, θ name, kind of A, kind of At) of the single-replica equivariance tests at side S."""
    if S == PROD:
        return [(2, "rot30", "peaky", "peaky")]
    i = SIZES.index(S)
    return [(T, name, KINDS[(i + k) % 3], KINDS[(i + k + T) % 3]) for T in TS for k, name in enumerate(THETA_NAMES)]


def equiv_inputs(kind_a, kind_at, T, S):
    return maps(kind_a, T, S, salt=1), maps(kind_at, T, S, salt=2)

WARP_SHAPES = ((2, 3, 37, 53), (1, 1, 1, 1), (1, 2, 1, 9), (1, 2, 9, 1), (3, 1, 16, 16), (1, 4, 64, 48))


def warp_case(shape, k):
    """(img, theta (B, 2, 3), g) of warp shape ``shape`` with image b warped by θ number k + b."""
    B, C, H, W = shape
    rng = np.random.default_rng([B, C, H, W, k])
    th = thetas(H, W)
    theta = np.stack([th[THETA_NAMES[(k + b) % len(THETA_NAMES)]] for b in range(B)])
    return rng.standard_normal(shape).astype(F32), theta, rng.standard_normal(shape).astype(F32)


GAUSS_CASES = tuple((num, size) for num in (1, 3, 16) for size in (7, 33, PROD))


def gauss_case(num, size):
    """(pos (num, 5, 2) float32, sigma): random positions, with 0, 1 and points slightly outside [0, 1]."""
    rng = np.random.default_rng([num, size])
    pos = rng.random((num, 5, 2)).astype(F32)
    pos[0, 0] = (0.0, 1.0)
    pos[0, 1] = (1.0, 0.0)
    pos[-1, 2] = (-0.05, 1.05)
    pos[-1, 3] = (1.02, 0.5)
    return pos, SIGMAS[(num + size) % 3]


KMAX_SIZES = (3, 7, 33, 68)
KMAX_NUMS = (1, 4, 16)
WAVG_SIZES = (7, 33, 68)
WAVG_DISTANCES = (5, 0, -1)


def wavg_case(kind, S):
    """(5, S, S) heat-maps of ``kind`` whose row 2 is all zero (the denominator is only the 1e-6 guard)."""
    m = maps(kind, 5, S, salt=7)
    m[2] = 0.0
    return m


RESIZE_CASES = ((3, 16, 40), (5, 32, 128), (2, 40, 16), (1, 7, 7), (4, 1, 5), (4, 5, 1), (3, 33, 100), (1, 100, 33))


def resize_case(C, R, Ro):
    rng = np.random.default_rng([C, R, Ro])
    return rng.standard_normal((C, R, R)).astype(F32), rng.standard_normal((C, Ro, Ro)).astype(F32)


AGG = dict(shape=(2, 32 * 32, 12), n_layers=2, Ro=80, indices=(3, 0, 7, 3, 11))


def aggregate_case():
    """Two captured layers (2, 32·32, 12), the gathered tokens (one twice) and d map (5, 80, 80)."""
    rng = np.random.default_rng(80)
    layers = [rng.random(AGG["shape"]).astype(F32) for _ in range(AGG["n_layers"])]
    return layers, rng.standard_normal((len(AGG["indices"]), AGG["Ro"], AGG["Ro"])).astype(F32)
