"""The objective kernels against float64 (tests/loss_ref.py), through stablekeypoints_amd.ops with autograd,
at map sides chosen against the kernels' tiling and not the workload: sharpening and equivariance losses
(single and batched) with their gradients, the affine warp and its adjoint, the Gaussian targets, the k-max
family and pixel_from_weighted_avg.

Exact outputs (positions, masked maps, the mutated map, the all-outside dAt) are compared for equality.
Every other bound is 4·e_cpu, where e_cpu = max|oracle_fp32 − float64| / max(1, max|float64|) over the
very inputs of the test, measured and asserted by tests/test_loss_ref_cpu.py (neither side is the kernel):
the kernel is another fp32 evaluation of the same formula, and differs from the oracle in summation order,
in expf and division roundings and, for dAt and the warp's adjoint, in atomic-add order.  Measured e_cpu
(rounded up to two digits) → bound:
  sharpening loss 1.6e-7, dA 2.3e-7;  equivariance loss 8.4e-8, dA 1.7e-7, dAt 2.1e-7;
  warp 1.1e-7, its adjoint 2.0e-7;  Gaussian targets 2.2e-7;  weighted-average position 7.6e-8.
The loss tests backpropagate an upstream gradient of 0.375·T·S² (L.upstream), so that dA = 0.75·(A − target)
keeps the maps' magnitude at every size and the figure's max(1, ·) denominator hides nothing.

The k-max mask compares the pixel INDEX with the peak's centre (index + 0.5), as the reference does, so the
nearest pixels lie at d² = 0.5: below S = 15 the radius 0.05·S holds no pixel, nothing is masked and all the
subjects share one peak (S = 3, 7); from S = 15 on the masked zeros outrank negative values.
"""
import numpy as np
import pytest
import torch

import loss_ref as L
from oracle import skp_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32

# 4 · e_cpu per compared quantity (tests/test_loss_ref_cpu.py holds the oracle to a quarter of each)
BOUND = {
    "sharp_loss": 6.4e-7,
    "sharp_dA": 9.2e-7,
    "equiv_loss": 3.36e-7,
    "equiv_dA": 6.8e-7,
    "equiv_dAt": 8.4e-7,
    "warp": 4.4e-7,
    "warp_adjoint": 8.0e-7,
    "gaussian": 8.8e-7,
    "wavg_pos": 3.04e-7,
}
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    yield
    print("\nlargest GPU error per quantity: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(SEEN.items())))


def T(a, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).requires_grad_(grad)


def N(t):
    return t.detach().cpu().numpy()


def close(name, got, ref):
    e = L.err(got, ref)
    SEEN[name] = max(SEEN.get(name, 0.0), e)
    assert e <= BOUND[name], (name, e, BOUND[name])


# ----------------------------------------------------------------------------- sharpening
def _sharpen(A, A_np, sigma, num, gout):
    """One single-image run on the leaf ``A`` (whose values are A_np): loss, (gradient left in the leaf)."""
    from stablekeypoints_amd import ops
    ref_l, ref_dA, ref_pos = L.sharpening(A_np, sigma, num, gout)
    l = ops.sharpening_loss(A, sigma, num)
    (l * gout).backward()
    close("sharp_loss", N(l), ref_l)
    return ref_dA, ref_pos


@pytest.mark.parametrize("S", L.SIZES + (L.PROD,))
def test_sharpening_vs_float64(S):
    from stablekeypoints_amd import ops
    for kind, Tn, num, sigma in L.sharpening_cases(S):
        A_np = L.maps(kind, Tn, S)
        A = T(A_np, grad=True)
        ref_dA, ref_pos = _sharpen(A, A_np, sigma, num, L.upstream(Tn, S))
        close("sharp_dA", N(A.grad), ref_dA)
        assert np.array_equal(N(ops.find_k_max_pixels(A.detach(), num)), ref_pos), (kind, Tn, num)


@pytest.mark.parametrize("S", L.SIZES)
def test_sharpening_batch_vs_float64(S):
    """nb = 3 images with upstream gradients (1, −2, 0)·c: gout[t / seg] multiplies each image's rows."""
    from stablekeypoints_amd import ops
    for kind, Tn, num, sigma in L.batch_cases(S):
        A_np = L.maps(kind, 3 * Tn, S, salt=3)
        w = np.array(L.WEIGHTS) * L.upstream(Tn, S)
        ref_l, ref_dA = L.per_image(lambda a, b, g: L.sharpening(a, sigma, num, g)[:2], 3, w, A_np)
        A = T(A_np, grad=True)
        l = ops.sharpening_loss_batch(A, 3, sigma, num)
        pos = N(l.grad_fn.saved_tensors[1])        # the kernel's own peaks, in units of the side
        (l * T(w.astype(F32))).sum().backward()
        close("sharp_loss", N(l), ref_l)
        close("sharp_dA", N(A.grad), ref_dA)
        assert not N(A.grad)[2 * Tn:].any()        # the zero-weight image
        assert np.array_equal(pos, L.peaks(A_np, num) / F32(S))


def test_sharpening_unaligned_view():
    """A contiguous view one float into its storage: no row is 16-B aligned, every row is read scalar."""
    S, Tn, num, sigma = 64, 5, 3, 2.0
    A_np = L.maps("signed", Tn, S, salt=4)
    base = torch.zeros(Tn * S * S + 1, device=DEV)
    base[1:] = T(A_np).reshape(-1)
    A = base[1:].view(Tn, S, S).detach().requires_grad_(True)
    assert A.is_contiguous() and A.data_ptr() % 16 == 4
    ref_dA, _ = _sharpen(A, A_np, sigma, num, L.upstream(Tn, S))
    close("sharp_dA", N(A.grad), ref_dA)


def test_sharpening_noncontiguous():
    """Every second row of a taller tensor: the gradient lands in those rows, zero in the others."""
    S, Tn, num, sigma = 30, 5, 2, 1.0
    A_np = L.maps("peaky", Tn, S, salt=5)
    tall = torch.full((Tn, 2 * S, S), 7.0, device=DEV)
    tall[:, ::2] = T(A_np)
    tall.requires_grad_(True)
    A = tall[:, ::2]
    assert not A.is_contiguous()
    ref_dA, _ = _sharpen(A, A_np, sigma, num, L.upstream(Tn, S))
    close("sharp_dA", N(tall.grad)[:, ::2], ref_dA)
    assert not N(tall.grad)[:, 1::2].any()


def test_sharpening_rejects_17_subjects_and_rectangles():
    from stablekeypoints_amd import ops
    A = T(L.maps("peaky", 3, 7))
    with pytest.raises(RuntimeError, match="num_subjects"):
        ops.sharpening_loss(A, 1.0, 17)
    with pytest.raises(RuntimeError, match="num_subjects"):
        ops.sharpening_loss_batch(A, 3, 1.0, 17)
    rect = T(L.maps("peaky", 3, 7, W=9))
    with pytest.raises(ValueError, match=r"\bA\b.*square"):
        ops.sharpening_loss(rect, 1.0, 1)
    with pytest.raises(ValueError, match=r"\bA\b.*square"):
        ops.sharpening_loss_batch(rect, 3, 1.0, 1)
    with pytest.raises(ValueError, match=r"\bmaps\b.*square"):
        ops.find_top_k_gaussian(rect, 2)
    with pytest.raises(ValueError, match=r"\bmaps\b.*square"):
        ops.find_top_k_gaussian_batch(rect[None], 2)


# ----------------------------------------------------------------------------- equivariance
@pytest.mark.parametrize("S", L.SIZES + (L.PROD,))
def test_equivariance_vs_float64(S):
    from stablekeypoints_amd import ops
    th = L.thetas(S, S)
    for Tn, name, ka, kat in L.equiv_cases(S):
        A_np, At_np = L.equiv_inputs(ka, kat, Tn, S)
        gout = L.upstream(Tn, S)
        ref_l, ref_dA, ref_dAt = L.equivariance(A_np, At_np, th[name], gout)
        A, At = T(A_np, grad=True), T(At_np, grad=True)
        l = ops.equivariance_loss_single(A, At, T(th[name]))
        (l * gout).backward()
        close("equiv_loss", N(l), ref_l)
        close("equiv_dA", N(A.grad), ref_dA)
        close("equiv_dAt", N(At.grad), ref_dAt)
        if name == "outside":     # nothing is sampled: the loss is mean(A²) and no gradient reaches At
            close("equiv_loss", N(l), (A_np.astype(np.float64) ** 2).mean())
            assert not N(At.grad).any()


@pytest.mark.parametrize("S", L.SIZES)
def test_equivariance_batch_vs_float64(S):
    """nb = 3 replicas, three different θ⁻¹ (th + 6·(t / seg)) and upstream gradients (1, −2, 0)·c."""
    from stablekeypoints_amd import ops
    th = np.stack([L.thetas(S, S)[n] for n in L.BATCH_THETAS])
    for kind, Tn, _, _ in L.batch_cases(S):
        A_np, At_np = L.equiv_inputs(kind, "peaky", 3 * Tn, S)
        w = np.array(L.WEIGHTS) * L.upstream(Tn, S)
        ref_l, ref_dA, ref_dAt = L.per_image(lambda a, at, b, g: L.equivariance(a, at, th[b], g), 3, w, A_np, At_np)
        A, At = T(A_np, grad=True), T(At_np, grad=True)
        l = ops.equivariance_loss_batch(A, At, T(th), 3)
        (l * T(w.astype(F32))).sum().backward()
        close("equiv_loss", N(l), ref_l)
        close("equiv_dA", N(A.grad), ref_dA)
        close("equiv_dAt", N(At.grad), ref_dAt)
        assert not N(A.grad)[2 * Tn:].any() and not N(At.grad)[2 * Tn:].any()


@pytest.mark.parametrize("S", L.SIZES)
@pytest.mark.parametrize("name", ["shift", "rot30"])
def test_equivariance_gradient_subsets(S, name):
    """Only A, only At (equiv_bwd_kernel's dA == nullptr branch) and both: the same gradients."""
    from stablekeypoints_amd import ops
    Tn = 5
    th = L.thetas(S, S)[name]
    A_np, At_np = L.equiv_inputs("signed", "peaky", Tn, S)
    gout = L.upstream(Tn, S)
    ref_l, ref_dA, ref_dAt = L.equivariance(A_np, At_np, th, gout)
    for ga, gat in ((True, False), (False, True), (True, True)):
        A, At = T(A_np, grad=ga), T(At_np, grad=gat)
        l = ops.equivariance_loss_single(A, At, T(th))
        (l * gout).backward()
        close("equiv_loss", N(l), ref_l)
        if ga:
            close("equiv_dA", N(A.grad), ref_dA)
        else:
            assert A.grad is None
        if gat:
            close("equiv_dAt", N(At.grad), ref_dAt)
        else:
            assert At.grad is None


def test_equivariance_unaligned_and_noncontiguous():
    from stablekeypoints_amd import ops
    S, Tn = 64, 5
    th = L.thetas(S, S)["rot30"]
    A_np, At_np = L.equiv_inputs("signed", "signed", Tn, S)
    gout = L.upstream(Tn, S)
    ref_l, ref_dA, ref_dAt = L.equivariance(A_np, At_np, th, gout)
    base = torch.zeros(Tn * S * S + 1, device=DEV)
    base[1:] = T(A_np).reshape(-1)
    A = base[1:].view(Tn, S, S).detach().requires_grad_(True)
    tall = torch.zeros(Tn, 2 * S, S, device=DEV)
    tall[:, ::2] = T(At_np)
    tall.requires_grad_(True)
    l = ops.equivariance_loss_single(A, tall[:, ::2], T(th))
    (l * gout).backward()
    close("equiv_loss", N(l), ref_l)
    close("equiv_dA", N(A.grad), ref_dA)
    close("equiv_dAt", N(tall.grad)[:, ::2], ref_dAt)
    assert not N(tall.grad)[:, 1::2].any()


# ----------------------------------------------------------------------------- affine warp
@pytest.mark.parametrize("shape", L.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_affine_warp_vs_float64(shape):
    """Forward and input gradient at H ≠ W, H = 1, W = 1 and a different θ per image, every θ case."""
    from stablekeypoints_amd import ops
    B, C, H, W = shape
    for k in range(len(L.THETA_NAMES)):
        img, theta, g = L.warp_case(shape, k)
        x = T(img, grad=True)
        out = ops.affine_warp(x, T(theta))
        out.backward(T(g))
        close("warp", N(out), L.warp(img, theta))
        close("warp_adjoint", N(x.grad), L.warp_adjoint(g, theta, H, W))


# ----------------------------------------------------------------------------- targets, k-max family
@pytest.mark.parametrize("num,size", L.GAUSS_CASES)
def test_gaussian_circles_vs_float64(num, size):
    from stablekeypoints_amd import ops
    pos, sigma = L.gauss_case(num, size)
    close("gaussian", N(ops.gaussian_circles(T(pos), size, sigma)), L.gaussian_targets(pos, size, sigma))


def test_gaussian_circles_rejects_17():
    from stablekeypoints_amd import ops
    with pytest.raises(RuntimeError, match="num"):
        ops.gaussian_circles(torch.zeros(17, 2, 2, device=DEV), 7, 1.0)


@pytest.mark.parametrize("S", L.KMAX_SIZES)
@pytest.mark.parametrize("kind", L.KINDS + ("special",))
def test_k_max_and_masks_exact(kind, S):
    """Positions and masked maps equal the oracle's: with negative values a masked pixel (v·0) outranks
    every unmasked one (S = 33, 68); at S = 3 and 7 the disc holds no pixel and the peaks repeat; NaN / ±inf
    rows survive as NaN."""
    from stablekeypoints_amd import ops
    m = L.maps(kind, 5, S, salt=6)
    nan = kind == "special"
    for num in L.KMAX_NUMS:
        ref_pos, ref_masked = L.peaks_masked(m, num)
        pos, masked = ops.find_k_max_pixels(T(m), num, return_masked=True)
        assert np.array_equal(N(pos), ref_pos), (kind, S, num)
        assert np.array_equal(N(masked), ref_masked, equal_nan=nan), (kind, S, num)
        assert np.array_equal(N(ops.find_k_max_pixels(T(m), num)), ref_pos)
    p = O.find_max_pixel(m)
    for radius in (0.05 * S, 0.15 * S, 0.0):
        assert np.array_equal(N(ops.mask_radius(T(m), T(p), radius)), O.mask_radius(m, p, radius), equal_nan=nan)


@pytest.mark.parametrize("S", L.WAVG_SIZES)
@pytest.mark.parametrize("kind", ["peaky", "ties"])
def test_pixel_from_weighted_avg_vs_float64(kind, S):
    from stablekeypoints_amd import ops
    m = L.wavg_case(kind, S)
    for distance in L.WAVG_DISTANCES:
        ref_pos, ref_m = L.weighted_avg(m, distance)
        work = T(m).clone()
        pos = ops.pixel_from_weighted_avg(work, distance)
        assert np.array_equal(N(work), ref_m), (kind, S, distance)      # mutated in place, exactly
        close("wavg_pos", N(pos), ref_pos)
        assert np.array_equal(N(pos)[2], F32([0.5, 0.5]))              # the all-zero row: 0 / 1e-6
