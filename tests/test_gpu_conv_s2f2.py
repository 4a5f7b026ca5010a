"""skp_conv3x3s2_f2 through ops.conv3x3_s2: the VAE's Downsample2D(padding=0) as 2×2 output tiles of
25 products, against F.pad(x, (0, 1, 0, 1)) + conv2d(stride=2) in fp64.  The bound is the one
tests/test_gpu_conv.py sets for this operation (relative error < 3e-5).  Measured on MI355X:
1.1e-7 … 2.1e-7 over these cases, against 6.0e-7 … 1.1e-6 for the sampled F(4×4, 3×3) kernel this
one replaced, on the same inputs."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = 3e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture
def ops(monkeypatch):
    from stablekeypoints_amd import ops
    monkeypatch.setattr(ops, "WINO_MIN_WORKGROUPS", 1)
    monkeypatch.setattr(ops, "WINO_S2_MIN_PIXELS", 1)
    return ops


def _rel(a, b):
    return ((a.double() - b).abs().max() / b.abs().max()).item()


def _case(B, C, K, H, W, bias, big_edge=False):
    g = torch.Generator().manual_seed(B * 1000 + C + K + H + W)
    x = torch.randn(B, C, H, W, generator=g)
    if big_edge:   # a wrong pad or an off-by-one at the right / bottom edge cannot hide
        x[:, :, -1, :] *= 100.0
        x[:, :, :-1, -1] *= 100.0
    w = torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b = torch.randn(K, generator=g) if bias else None
    return x, w, b


def _ref(x, w, b):
    return F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), None if b is None else b.double(), stride=2)


def _check(ops, x, w, b, label):
    ref = _ref(x, w, b)
    with torch.no_grad():
        y = ops.conv3x3_s2(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV))
    assert y.shape == ref.shape
    err = _rel(y.cpu(), ref)
    print(f"{label}: rel err {err:.3e}")
    assert err < BOUND


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,C,K,H,W,nsplit", [
    (1, 4, 32, 32, 32, 0),     # one stage, one block column
    (2, 8, 64, 64, 32, 0),     # two stages, two channel blocks, four half-height blocks per image
    (1, 12, 32, 32, 96, 0),    # three stages, non-square
    (1, 32, 32, 32, 32, 2),    # split-K: four stages per split
    (1, 32, 32, 32, 32, 4),    # two stages per split
])
def test_conv3x3_s2_f2_vs_fp64(ops, monkeypatch, B, C, K, H, W, nsplit, bias):
    if nsplit:
        monkeypatch.setattr(ops, "WINO_NSPLIT_FORCE", nsplit)
        assert ops._wino_plan(B, C, K, H, W)[1] == nsplit
    x, w, b = _case(B, C, K, H, W, bias)
    _check(ops, x, w, b, f"{(B, C, K, H, W)} nsplit {nsplit} bias {bias}")


def test_conv3x3_s2_f2_large_last_row_and_column(ops):
    x, w, b = _case(2, 8, 64, 64, 32, True, big_edge=True)
    _check(ops, x, w, b, "large last row / column")


def test_vae_downsample_takes_fused_path(ops, monkeypatch):
    from stablekeypoints_amd.sd.unet import Downsample2D
    torch.manual_seed(0)
    m = Downsample2D(128, padding=0).to(DEV)
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.randn(1, 128, 64, 64, device=DEV)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: names.append(name) or real(name, *a))
    with torch.no_grad():
        y = m(x)
    assert "skp_conv3x3s2_f2" in names, "Downsample2D did not take the fused stride-2 path"
    ref = _ref(x.cpu(), m.conv.weight.cpu(), m.conv.bias.cpu())
    err = _rel(y.cpu(), ref)
    print(f"Downsample2D(128) at 64x64: rel err {err:.3e}")
    assert y.shape == (1, 128, 32, 32) and err < BOUND


def test_modified_frozen_weight_rebuilds_u(ops):
    x, w, b = _case(1, 8, 32, 32, 32, True)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    with torch.no_grad():
        y0 = ops.conv3x3_s2(xd, wd, bd)
        assert _rel(y0.cpu(), _ref(x, w, b)) < BOUND
        wd.mul_(-0.5).add_(0.01)           # in place: same tensor, new version
        y1 = ops.conv3x3_s2(xd, wd, bd)
    err = _rel(y1.cpu(), _ref(x, wd.cpu(), b))
    print(f"after the in-place weight update: rel err {err:.3e}")
    assert err < BOUND
