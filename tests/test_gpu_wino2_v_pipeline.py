"""The V-staged Winograd pair's register-prefetch pipeline and its lane-major V layout.

skp_conv3x3_wino2_v loads the A operand of stage t from V straight into a ring of three register
buffers and its weights into a ring of three LDS slots, both two stages ahead, with one in-order
vmcnt counting both.  What can go wrong there shows at the pipeline's edges: fewer stages than the
lead (1, 2), exactly the lead, every residue of the ring period with the tail, and a split that
leaves one stage per part.  The arithmetic is skp_conv3x3_wino2's, so every case is held to
torch.equal against it at the same nsplit, and to the project's 3e-5-of-max bar against an fp64
conv2d (tests/test_gpu_conv.py).

V is B·C·(H/4)·(W/4)·36 floats with no padding (include/skp.h): the transform pass must write all
of it and nothing after it, and the convolution must read nothing after it.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V_PER_TILE = 36   # floats of V per (channel, 4×4 tile): the documented size, no pads


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture
def fused(monkeypatch):
    from stablekeypoints_amd import ops
    monkeypatch.setattr(ops, "WINO_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(ops, "WINO_GEMM_MAX_HW", 0)
    return ops


def _conv(name, x, U, bias, res, B, C, K, H, W, nsplit, gn):
    from stablekeypoints_amd._lib import call, ptr, stream
    y = torch.empty(B, K, H, W, device=DEV)
    ws = torch.empty(nsplit, B, K, H, W, device=DEV) if nsplit > 1 else None
    gnp = torch.zeros(B, K, (H // 16) * (W // 32), 2, device=DEV) if gn else None
    call(name, ptr(x), ptr(U), ptr(bias), ptr(res), ptr(y), B, C, K, H, W, nsplit, ptr(ws), ptr(gnp), stream(DEV))
    return y, gnp


def _v_size(B, C, H, W):
    return B * C * (H // 4) * (W // 4) * V_PER_TILE


def _vtransform(x, V=None):
    from stablekeypoints_amd._lib import call, ptr, stream
    B, C, H, W = x.shape
    if V is None:
        V = torch.empty(_v_size(B, C, H, W), device=DEV)
    call("skp_wino2_vtransform", ptr(x), ptr(V), B, C, H, W, stream(DEV))
    return V


def _inputs(B, C, K, H, W, epi, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = (torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(DEV)
    b = torch.randn(K, generator=g).to(DEV) if epi else None
    r = torch.randn(B, K, H, W, generator=g).to(DEV) if epi else None
    return x, w, b, r


def _fp64_error(y, x, w, b, r):
    ref = F.conv2d(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu(), 1, 1)
    if r is not None:
        ref = ref + r.double().cpu()
    return ((y.double().cpu() - ref).abs().max() / ref.abs().max()).item()


# nst = C / 4 = 1 … 7 stages, each plain and with bias + residual + GroupNorm partials; K, (H, W)
# and B walk through {32, 64}, {(32, 32), (64, 32), (32, 64)} and {1, 2}
_SHAPES = [(32, 32), (64, 32), (32, 64)]
_EDGES = [(1 + (i + e) % 2, 4 * (i + 1), (32, 64)[(i + e) % 2], *_SHAPES[(i + 2 * e) % 3], bool(e), 1)
          for i in range(7) for e in (0, 1)]
_EDGES += [(1, 8, 32, 32, 64, True, 2),     # one stage per split: below the lead in both
           (2, 24, 64, 64, 32, True, 2)]    # three per split: exactly one ring period


@pytest.mark.parametrize("B,C,K,H,W,epi,nsplit", _EDGES)
def test_pipeline_edges_bit_for_bit(fused, B, C, K, H, W, epi, nsplit):
    ops = fused
    x, w, b, r = _inputs(B, C, K, H, W, epi, 1000 * C + 10 * K + H + nsplit)
    U = ops._wino_u(w, False, True)
    gn = epi and nsplit == 1   # the epilogue writes the partials of an unsplit convolution only
    y0, p0 = _conv("skp_conv3x3_wino2_gn", x, U, b, r, B, C, K, H, W, nsplit, gn)
    y1, p1 = _conv("skp_conv3x3_wino2_v_gn", _vtransform(x), U, b, r, B, C, K, H, W, nsplit, gn)
    torch.cuda.synchronize()
    e = _fp64_error(y1, x, w, b, r)
    print(f"stages {C // 4} / {nsplit}: max |Δ| {(y0 - y1).abs().max().item():.3e}   vs fp64 {e:.3e}")
    assert torch.equal(y0, y1)
    if gn:
        assert torch.equal(p0, p1)
    assert e < 3e-5


@pytest.mark.parametrize("B,C,K,H,W", [
    (1, 8, 32, 32, 32),     # one block row and column: every border zero-padded
    (2, 12, 32, 64, 32),    # H != W, two images, three stages
])
def test_v_bounds(fused, B, C, K, H, W):
    ops = fused
    x, w, _, _ = _inputs(B, C, K, H, W, False, 77 + C)
    U = ops._wino_u(w, False, True)
    n, tail, sentinel = _v_size(B, C, H, W), 8192, 12345.678
    V = torch.full((n + tail,), sentinel, device=DEV)
    _vtransform(x, V)
    torch.cuda.synchronize()
    assert (V[n:] == sentinel).all(), "the transform pass wrote past the documented size"
    assert (V[:n] != sentinel).all(), "the layout has no pads: every documented float is written"
    V[n:] = float("nan")
    y0, _ = _conv("skp_conv3x3_wino2_gn", x, U, None, None, B, C, K, H, W, 1, False)
    y1, _ = _conv("skp_conv3x3_wino2_v_gn", V, U, None, None, B, C, K, H, W, 1, False)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1), "the convolution read past the documented size"
    assert _fp64_error(y1, x, w, None, None) < 3e-5


def test_groupnorm_fused_pair_per_sample_shift(fused):
    """Eight stages and a per-sample shift through ops.gn_conv3x3 against ops.group_norm_act +
    ops.conv3x3: ≤ 1e-5 of the maximum between the paths, 3e-5 against fp64."""
    ops = fused
    B, C, G, K, H, W, eps = 2, 32, 8, 64, 32, 64, 1e-6
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(B, 8, H, W, generator=g).to(DEV)
    w0 = (torch.randn(C, 8, 3, 3, generator=g) / (3 * 8 ** 0.5)).to(DEV)
    w = (torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(DEV)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.2 * torch.randn(C, generator=g)).to(DEV)
    shift = (0.5 * torch.randn(B, C, generator=g)).to(DEV)
    with torch.no_grad():
        x = ops.conv3x3(x0, w0)
        y_new = ops.gn_conv3x3(x, gamma, beta, G, eps, True, shift, w)
        y_old = ops.conv3x3(ops.group_norm_act(x, gamma, beta, G, eps, True, shift), w)
    xd = x.double().cpu() + shift.double().cpu()[:, :, None, None]
    ref = F.conv2d(F.silu(F.group_norm(xd, G, gamma.double().cpu(), beta.double().cpu(), eps)), w.double().cpu(), None, 1, 1)
    m = ref.abs().max().item()
    e_ref = (y_new.double().cpu() - ref).abs().max().item() / m
    e_old = (y_new - y_old).abs().max().item() / m
    print(f"vs fp64 {e_ref:.3e}   vs group_norm_act + conv3x3 {e_old:.3e}")
    assert e_ref < 3e-5
    assert e_old <= 1e-5
