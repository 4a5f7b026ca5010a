"""The V-staged Winograd pair: skp_wino2_vtransform(_gn) + skp_conv3x3_wino2_v(_gn).

The transform pass writes V = Bᵀ d B of every input tile once (d = x, or act(GroupNorm(x + shift))
applied on load) and the convolution kernel reads V instead of transforming its region itself.
The transform arithmetic, the stage order and the MFMA order are those of skp_conv3x3_wino2, so
the plain pair must reproduce it bit for bit at the same split; the GroupNorm-fused pair is held
to the bars of tests/test_gpu_conv.py (3e-5 of the output's maximum against fp64, 1e-5 between
two Winograd paths).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def _vtransform(x):
    from stablekeypoints_amd._lib import call, ptr, stream
    B, C, H, W = x.shape
    V = torch.empty(B * C * (H // 4) * (W // 4) * 40, device=DEV)
    call("skp_wino2_vtransform", ptr(x), ptr(V), B, C, H, W, stream(DEV))
    return V


@pytest.mark.parametrize("B,C,K,H,W,epi,nsplit", [
    (1, 4, 32, 32, 32, False, 1),     # one stage, every border
    (2, 12, 64, 64, 32, False, 1),    # 3 stages (odd ring parity), two channel blocks, H != W
    (1, 32, 32, 32, 64, True, 1),     # bias, residual and GroupNorm partials
    (1, 32, 32, 32, 64, True, 2),     # bias and residual through the split-K reduction
])
def test_plain_pair_equals_wino2_bit_for_bit(fused, B, C, K, H, W, epi, nsplit):
    ops = fused
    g = torch.Generator().manual_seed(100 * C + K + H + nsplit)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = (torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(DEV)
    b = torch.randn(K, generator=g).to(DEV) if epi else None
    r = torch.randn(B, K, H, W, generator=g).to(DEV) if epi else None
    U = ops._wino_u(w, False, True)
    gn = epi and nsplit == 1   # the epilogue writes the partials of an unsplit convolution only
    y0, p0 = _conv("skp_conv3x3_wino2_gn", x, U, b, r, B, C, K, H, W, nsplit, gn)
    y1, p1 = _conv("skp_conv3x3_wino2_v_gn", _vtransform(x), U, b, r, B, C, K, H, W, nsplit, gn)
    torch.cuda.synchronize()
    print("max |Δ|", (y0 - y1).abs().max().item())
    assert torch.equal(y0, y1)
    if gn:
        assert torch.equal(p0, p1)
    ref = F.conv2d(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu(), 1, 1)
    if r is not None:
        ref = ref + r.double().cpu()
    assert ((y1.double().cpu() - ref).abs().max() / ref.abs().max()).item() < 3e-5


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("with_shift", [False, True])
@pytest.mark.parametrize("from_parts", [True, False])
def test_groupnorm_fused_pair(fused, monkeypatch, act, with_shift, from_parts):
    ops = fused
    B, C, G, K, H, W, eps = 2, 64, 32, 32, 32, 32, 1e-6
    monkeypatch.setattr(ops, "GN_EPI", from_parts)
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(B, 8, H, W, generator=g).to(DEV)
    w0 = (torch.randn(C, 8, 3, 3, generator=g) / (3 * 8 ** 0.5)).to(DEV)
    w = (torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(DEV)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.2 * torch.randn(C, generator=g)).to(DEV)
    shift = (0.5 * torch.randn(B, C, generator=g)).to(DEV) if with_shift else None
    with torch.no_grad():
        x = ops.conv3x3(x0, w0)   # the producing convolution: x carries its statistics partials
        assert (ops._gn_parts_of(x) is not None) == from_parts
        y_new = ops.gn_conv3x3(x, gamma, beta, G, eps, act, shift, w)
        y_old = ops.conv3x3(ops.group_norm_act(x, gamma, beta, G, eps, act, shift), w)
    xd = x.double().cpu()
    if shift is not None:
        xd = xd + shift.double().cpu()[:, :, None, None]
    n = F.group_norm(xd, G, gamma.double().cpu(), beta.double().cpu(), eps)
    ref = F.conv2d(F.silu(n) if act else n, w.double().cpu(), None, 1, 1)
    m = ref.abs().max().item()
    e_ref = (y_new.double().cpu() - ref).abs().max().item() / m
    e_old = (y_new - y_old).abs().max().item() / m
    print(f"vs fp64 {e_ref:.3e}   vs group_norm_act + conv3x3 {e_old:.3e}   equal {torch.equal(y_new, y_old)}")
    assert e_ref < 3e-5
    assert e_old <= 1e-5
    # the next GroupNorm's statistics partials ride on the output exactly where conv3x3 leaves
    # them (an unsplit convolution with GN_EPI on)
    pn, po = ops._gn_parts_of(y_new), ops._gn_parts_of(y_old)
    assert (pn is None) == (po is None)
    if pn is not None:
        assert torch.equal(pn[0], po[0])


class _Names:
    """A kernel timer that only records the launched names."""

    def __init__(self):
        self.names = []

    def record(self, name, nbytes=0, flops=0, cycles=0):
        self.names.append(name)

        class _Ctx:
            def __enter__(self_):
                return self_

            def __exit__(self_, *a):
                return False
        return _Ctx()


def test_resnet_block_routing(fused, monkeypatch):
    ops = fused
    from stablekeypoints_amd.sd.unet import ResnetBlock2D
    torch.manual_seed(3)
    blk = ResnetBlock2D(64, 64, temb_channels=None, groups=32, eps=1e-6).to(DEV).eval().requires_grad_(False)
    x = torch.randn(2, 64, 32, 32, device=DEV)
    rec = _Names()
    ops.set_kernel_timer(rec)
    try:
        with torch.no_grad():
            y_old = blk(x)
        assert "skp_conv3x3_wino2" in rec.names and "skp_conv3x3_wino2_v" not in rec.names
        monkeypatch.setattr(ops, "WINO_V_SHAPES", {(64, 64, 32, 32)})
        monkeypatch.setattr(ops, "WINO_V_MIN_BATCH", 1)
        rec.names.clear()
        with torch.no_grad():
            y_new = blk(x)
        assert rec.names == ["skp_wino2_vtransform_gn", "skp_conv3x3_wino2_v"] * 2
        rec.names.clear()
        xg = x.clone().requires_grad_(True)   # a gradient-carrying call keeps the old path
        y_grad = blk(xg)
        assert "skp_conv3x3_wino2" in rec.names
        assert "skp_conv3x3_wino2_v" not in rec.names and "skp_wino2_vtransform_gn" not in rec.names
        y_grad.sum().backward()
        assert xg.grad is not None and torch.isfinite(xg.grad).all()
    finally:
        ops.set_kernel_timer(None)
    m = y_old.abs().max().item()
    d = (y_new - y_old).abs().max().item() / m
    print(f"block: new vs old {d:.3e}   equal {torch.equal(y_new, y_old)}")
    assert d <= 1e-5
    assert torch.equal(y_grad.detach(), y_old)


def test_new_entry_points_reject_bad_shapes():
    """C % 4, K % 32 and H, W % 32 are refused with an error return before any launch (the
    pointers are aligned dummies that no kernel may touch)."""
    from stablekeypoints_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(256)
    for C, H, W, msg in ((6, 32, 32, b"multiple of 4"), (8, 48, 32, b"multiples of 32"), (8, 32, 16, b"multiples of 32")):
        assert L.skp_wino2_vtransform(a, a, 1, C, H, W, None) == -1 and msg in L.skp_last_error()
        assert L.skp_wino2_vtransform_gn(a, a, a, a, None, 2, 1, a, 1, C, H, W, None) == -1
        assert msg in L.skp_last_error()
    for C, K, H, W, msg in ((6, 32, 32, 32, b"multiple of 4"), (8, 48, 32, 32, b"multiple of 32"),
                            (8, 32, 48, 32, b"multiples of 32"), (8, 32, 32, 16, b"multiples of 32")):
        assert L.skp_conv3x3_wino2_v(a, a, None, None, a, 1, C, K, H, W, 1, None, None) == -1
        assert msg in L.skp_last_error()
        assert L.skp_conv3x3_wino2_v_gn(a, a, None, None, a, 1, C, K, H, W, 1, None, None, None) == -1
        assert msg in L.skp_last_error()
