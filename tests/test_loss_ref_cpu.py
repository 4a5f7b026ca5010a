"""tests/loss_ref.py against the oracle and the goldens, on every input of tests/test_gpu_losses.py and
tests/test_gpu_resize.py, and the measurement that sets those files' tolerances (no GPU).

e_cpu = max|oracle_fp32 − loss_ref_float64| / max(1, max|loss_ref_float64|) per compared quantity over the
GPU tests' own inputs: what an fp32 evaluation of the same formula costs there.  Neither side is the
kernel.  The GPU bound is 4·e_cpu, written in the GPU files' BOUND tables; each test here asserts that the
oracle stays within a quarter of it, so the recorded figure cannot drift.  Measured (two digits, rounded up):
  sharpening loss 1.6e-7, dA 2.3e-7;  equivariance loss 8.4e-8, dA 1.7e-7, dAt 2.1e-7;
  warp 1.1e-7, adjoint 2.0e-7;  Gaussian targets 2.2e-7;  weighted-average position 7.6e-8;
  resize 1.1e-7, adjoint 1.1e-7;  aggregate backward 1.1e-7.
Exact outputs (peaks, masked and mutated maps) must be equal.
"""
import numpy as np
import pytest

import loss_ref as L
import test_gpu_losses as GL
import test_gpu_resize as GR
from conftest import load_golden
from oracle import skp_oracle as O

F32 = np.float32


class Worst:
    """The largest e_cpu of one quantity, held to a quarter of the GPU bound."""

    def __init__(self, name, table):
        self.name, self.bound, self.e = name, table[name], 0.0

    def add(self, oracle, ref):
        self.e = max(self.e, L.err(oracle, ref))


def check(*worst):
    for w in worst:
        print(f"e_cpu {w.name} {w.e:.3e} (GPU bound {w.bound:.2e})")
    for w in worst:
        assert 0 < w.e <= w.bound / 4, (w.name, w.e, w.bound)   # 0: fp32 equal to float64 would measure nothing


# ----------------------------------------------------------------------------- sharpening
def _oracle_sharpening(A, sigma, num, gout):
    l, dA = O.sharpening_loss(A, sigma, num)
    return l, dA * F32(gout)


def test_sharpening_oracle_and_bound():
    wl, wd = Worst("sharp_loss", GL.BOUND), Worst("sharp_dA", GL.BOUND)
    for S in L.SIZES + (L.PROD,):
        for kind, Tn, num, sigma in L.sharpening_cases(S):
            A = L.maps(kind, Tn, S)
            g = L.upstream(Tn, S)
            assert F32(g) == g
            l, dA, pos = L.sharpening(A, sigma, num, g)
            ol, odA = _oracle_sharpening(A, sigma, num, g)
            wl.add(ol, l)
            wd.add(odA, dA)
            assert np.array_equal(pos, O.find_k_max_pixels(A, num))
    for S in L.SIZES:
        for kind, Tn, num, sigma in L.batch_cases(S):
            A = L.maps(kind, 3 * Tn, S, salt=3)
            w = np.array(L.WEIGHTS) * L.upstream(Tn, S)
            l, dA = L.per_image(lambda a, b, g: L.sharpening(a, sigma, num, g)[:2], 3, w, A)
            ol, odA = L.per_image(lambda a, b, g: _oracle_sharpening(a, sigma, num, g), 3, w, A)
            wl.add(ol, l)
            wd.add(odA, dA)
            assert not dA[2 * Tn:].any()
    for A, Tn, S, num, sigma in ((L.maps("signed", 5, 64, salt=4), 5, 64, 3, 2.0),      # the unaligned view
                                 (L.maps("peaky", 5, 30, salt=5), 5, 30, 2, 1.0)):      # the strided view
        l, dA, _ = L.sharpening(A, sigma, num, L.upstream(Tn, S))
        ol, odA = _oracle_sharpening(A, sigma, num, L.upstream(Tn, S))
        wl.add(ol, l)
        wd.add(odA, dA)
    check(wl, wd)


def test_sharpening_vs_golden():
    g = load_golden("losses")
    for ns in (1, 2):
        l, dA, _ = L.sharpening(g["A"], 2.0, ns)
        assert np.allclose(l, g[f"sharp_ns{ns}"], rtol=1e-5, atol=0)
        assert np.allclose(dA, g[f"dA_sharp_ns{ns}"], atol=1e-9, rtol=1e-5)
    with pytest.raises(ValueError):
        L.sharpening(np.zeros((2, 4, 5), F32), 1.0, 1)


def test_peaks_vs_golden_and_masks():
    g = load_golden("argmax")
    assert np.array_equal(L.peaks(g["edge"], 3), g["edge_k3"], equal_nan=True)
    assert np.array_equal(L.peaks(g["maps32"], 3), g["maps32_k3"])
    for S in L.KMAX_SIZES:
        for kind in L.KINDS + ("special",):
            m = L.maps(kind, 5, S, salt=6)
            for num in L.KMAX_NUMS:
                pos, masked = L.peaks_masked(m, num)
                assert np.array_equal(pos, O.find_k_max_pixels(m, num), equal_nan=True)
                # the mask rule restated: pixel INDEX (r, c) against the peak's centre (index + 0.5), so
                # the distances are half-integers; what is outside every disc is unchanged, what is
                # inside is zero (NaN where the value was not finite)
                keep = np.ones_like(m, bool)
                rr, cc = np.mgrid[0:S, 0:S]
                for q in range(num):
                    d2 = (rr[None] - pos[q][:, 0, None, None]) ** 2 + (cc[None] - pos[q][:, 1, None, None]) ** 2
                    keep &= d2 > (0.05 * S) ** 2
                assert np.array_equal(masked[keep], m[keep], equal_nan=True)
                assert not masked[~keep & np.isfinite(m)].any()
                assert keep.all() == (S < 15)        # (0.05·S)² < 0.5: the disc holds no pixel, the peaks repeat
                if S < 15:
                    assert np.array_equal(pos, np.broadcast_to(pos[:1], pos.shape), equal_nan=True)
    # a masked zero beats every unmasked negative: the second peak is the first masked pixel in row-major order
    neg = -np.ones((1, 33, 33), F32)
    neg[0, 4, 2] = -0.5
    assert np.array_equal(L.peaks(neg, 2)[:, 0], F32([[4.5, 2.5], [3.5, 2.5]]))


# ----------------------------------------------------------------------------- equivariance, warp
def _oracle_equivariance(A, At, ti, gout):
    """O.equivariance_loss with θ⁻¹ given directly (the oracle's own pieces, in its order)."""
    ti = np.asarray(ti, F32).reshape(1, 2, 3)
    diff = (A - O.affine_warp(At[None], ti)[0]).astype(F32)
    loss = F32((diff.astype(np.float64) ** 2).mean())
    g = (F32(2.0 / diff.size) * diff).astype(F32) * F32(gout)
    return loss, g, O.affine_warp_bwd(-g[None], ti, A.shape[1], A.shape[2])[0]


def test_equivariance_oracle_and_bound():
    wl, wa, wt = (Worst(n, GL.BOUND) for n in ("equiv_loss", "equiv_dA", "equiv_dAt"))

    def both(A, At, th, g):
        for w, o, r in zip((wl, wa, wt), _oracle_equivariance(A, At, th, g), L.equivariance(A, At, th, g)):
            w.add(o, r)

    for S in L.SIZES + (L.PROD,):
        th = L.thetas(S, S)
        for Tn, name, ka, kat in L.equiv_cases(S):
            A, At = L.equiv_inputs(ka, kat, Tn, S)
            both(A, At, th[name], L.upstream(Tn, S))
            if name == "outside":
                l, _, dAt = L.equivariance(A, At, th[name], 3.0)
                assert l == (A.astype(np.float64) ** 2).mean() and not dAt.any()
    for S in L.SIZES:
        thb = np.stack([L.thetas(S, S)[n] for n in L.BATCH_THETAS])
        for kind, Tn, _, _ in L.batch_cases(S):
            A, At = L.equiv_inputs(kind, "peaky", 3 * Tn, S)
            w = np.array(L.WEIGHTS) * L.upstream(Tn, S)
            ref = L.per_image(lambda a, at, b, g: L.equivariance(a, at, thb[b], g), 3, w, A, At)
            ora = L.per_image(lambda a, at, b, g: _oracle_equivariance(a, at, thb[b], g), 3, w, A, At)
            for wst, o, r in zip((wl, wa, wt), ora, ref):
                wst.add(o, r)
        for name in ("shift", "rot30"):                                # the gradient-subset cases
            both(*L.equiv_inputs("signed", "peaky", 5, S), L.thetas(S, S)[name], L.upstream(5, S))
    both(*L.equiv_inputs("signed", "signed", 5, 64), L.thetas(64, 64)["rot30"], L.upstream(5, 64))
    check(wl, wa, wt)


def test_equivariance_and_warp_vs_golden():
    g = load_golden("losses")
    assert np.abs(L.warp(g["img"], g["theta"]) - g["warped"]).max() <= 1e-6
    ti = O.theta_inverse(g["theta"])
    assert np.abs(L.warp(np.repeat(g["At"][None], 2, 0), ti) - g["inv_At"]).max() <= 1e-6
    l, dA, dAt = L.equivariance(g["A"], g["At"], ti[1])
    assert np.allclose(l, g["equiv"], rtol=1e-4, atol=0)
    for ours, ref in ((dA, g["dA_equiv"]), (dAt, g["dAt_equiv"])):
        assert np.abs(ours - ref).max() <= 1e-6 * np.abs(ref).max()


def test_warp_oracle_and_bound():
    wf, wb = Worst("warp", GL.BOUND), Worst("warp_adjoint", GL.BOUND)
    for shape in L.WARP_SHAPES:
        B, C, H, W = shape
        for k in range(len(L.THETA_NAMES)):
            img, theta, g = L.warp_case(shape, k)
            wf.add(O.affine_warp(img, theta), L.warp(img, theta))
            wb.add(O.affine_warp_bwd(g, theta, H, W), L.warp_adjoint(g, theta, H, W))
    check(wf, wb)


def test_warp_adjoint_is_the_adjoint_and_outside_is_zero():
    for shape in ((2, 3, 37, 53), (1, 2, 1, 9)):
        img, theta, g = L.warp_case(shape, 2)
        lhs = (L.warp(img, theta) * g).sum()
        rhs = (img.astype(np.float64) * L.warp_adjoint(g, theta, shape[2], shape[3])).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    img, _, g = L.warp_case((1, 2, 9, 1), 0)
    out = L.thetas(9, 1)["outside"][None]
    assert not L.warp(img, out).any() and not L.warp_adjoint(g, out, 9, 1).any()
    ident = L.thetas(16, 16)["identity"][None]
    img, _, _ = L.warp_case((1, 2, 16, 16), 0)
    assert np.abs(L.warp(img, ident) - img).max() <= 1e-5      # the fp32 grid is the definition: not exact


# ----------------------------------------------------------------------------- targets, weighted average
def test_gaussian_oracle_golden_and_bound():
    w = Worst("gaussian", GL.BOUND)
    for num, size in L.GAUSS_CASES:
        pos, sigma = L.gauss_case(num, size)
        w.add(O.gaussian_circles(pos, size, sigma), L.gaussian_targets(pos, size, sigma))
    check(w)
    g = load_golden("gaussian")
    for size, sigma in ((32, 2.0), (128, 2.0), (20, 3.0)):
        assert np.abs(L.gaussian_targets(g["pos"], size, sigma) - g[f"circles_{size}_{sigma}"]).max() <= 1e-6
    assert np.abs(L.gaussian_targets(g["pos"][0], 32, 2.0) - g["circle_32_2.0"]).max() <= 1e-6


def test_weighted_avg_oracle_golden_and_bound():
    w = Worst("wavg_pos", GL.BOUND)
    for S in L.WAVG_SIZES:
        for kind in ("peaky", "ties"):
            m = L.wavg_case(kind, S)
            for distance in L.WAVG_DISTANCES:
                pos, mut = L.weighted_avg(m, distance)
                opos, omut = O.pixel_from_weighted_avg(m, distance)
                assert np.array_equal(mut, omut)
                assert np.array_equal(pos[2], [0.5, 0.5])
                w.add(opos, pos)
    check(w)
    g = load_golden("argmax")
    pos, mut = L.weighted_avg(g["maps32"], 5)
    assert np.allclose(pos, g["maps32_wavg"], atol=1e-4) and np.array_equal(mut, g["maps32_wavg_mutated"])
    assert np.allclose(L.weighted_avg(g["maps32"], -1)[0], g["maps32_wavg_nodist"], atol=1e-4)


# ----------------------------------------------------------------------------- resize
def test_resize_oracle_and_bound():
    wf, wb = Worst("resize", GR.BOUND), Worst("resize_adjoint", GR.BOUND)
    for C, R, Ro in L.RESIZE_CASES:
        x, g = L.resize_case(C, R, Ro)
        wf.add(O.resize(x, Ro, "bilinear"), L.resize(x, Ro))
        wb.add(O.resize_adjoint(g, R, "bilinear"), L.resize_adjoint(g, R))
        # the adjoint identity, and a constant image resizes to the constant
        lhs, rhs = (L.resize(x, Ro) * g).sum(), (x.astype(np.float64) * L.resize_adjoint(g, R)).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
        assert np.abs(L.resize(np.ones((1, R, R), F32), Ro) - 1.0).max() <= 1e-6
    check(wf, wb)


def test_aggregate_backward_oracle_and_bound():
    w = Worst("aggregate_bwd", GR.BOUND)
    layers, dmap = L.aggregate_case()
    idx = list(L.AGG["indices"])
    ref = L.aggregate_bwd(L.AGG["shape"], L.AGG["n_layers"], dmap, L.AGG["Ro"], idx)
    ora = O.collect_maps_bwd([L.AGG["shape"]] * L.AGG["n_layers"], dmap, upsample_res=L.AGG["Ro"], indices=idx)
    assert len(ora) == L.AGG["n_layers"]
    for o in ora:
        w.add(o, ref)
    check(w)
