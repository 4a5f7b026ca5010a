"""skp_map_range / skp_render_sheet (A17) on the GPU against the numpy restatement (render_ref.py).

``map_range`` is bit-exact.  ``render_sheet``: the byte equals the float64 restatement's byte
everywhere, except that a difference of one count is allowed where the restatement's
pre-rounding value lies within τ = 0.01 counts of a half-integer.  τ is derived: the chain is
about twenty fp32 operations on magnitudes <= 255 and the LUT is continuous by construction,
which is well under 1e-3 counts of rounding drift for maps whose range is >= 1e-3; τ is ten times
that.  Padding, the empty tile, disc and outline pixels and no-overlay pixels at f = 1 are
exact with no exemption.  The conditions that keep the rule honest (map range, distance of
every pixel centre to the marker circles, share of bytes inside the band) are asserted on the
restatement alone.
"""
import numpy as np
import pytest
import torch

import render_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def T(a, **kw):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _range_maps(shape, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal(shape) * 3).astype(np.float32)


def test_map_range_vector_path_special_maps():
    from stablekeypoints_amd import ops
    maps = _range_maps((5, 16, 16), 1)
    maps[1] = -1.5              # constant
    maps[2, 7, 3] = np.nan
    maps[3, 15, 15] = np.inf
    got = ops.map_range(T(maps)).cpu().numpy()
    ref = R.map_range_ref(maps)
    assert np.isnan(ref[1:4]).all() and np.isfinite(ref[[0, 4]]).all()
    assert np.array_equal(_bits(got), _bits(ref))


def test_map_range_odd_size_scalar_path():
    from stablekeypoints_amd import ops
    maps = _range_maps((3, 7, 9), 2)
    assert np.array_equal(_bits(ops.map_range(T(maps)).cpu().numpy()), _bits(R.map_range_ref(maps)))


def test_map_range_misaligned_view_and_many_waves():
    from stablekeypoints_amd import ops
    buf = _range_maps((1 + 4 * 40 * 40,), 3)
    view = T(buf)[1:].view(4, 40, 40)     # starts one float into the buffer: the scalar path
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ref = R.map_range_ref(buf[1:].reshape(4, 40, 40))
    assert np.array_equal(_bits(ops.map_range(view).cpu().numpy()), _bits(ref))
    big = _range_maps((2, 64, 64), 4)     # several loads per thread on the 16-B path
    assert np.array_equal(_bits(ops.map_range(T(big)).cpu().numpy()), _bits(R.map_range_ref(big)))


@pytest.fixture(scope="module")
def lut():
    from stablekeypoints_amd import ops
    return ops.fallback_lut().numpy()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_render_sheet_matches_restatement(name, lut):
    from stablekeypoints_amd import ops
    case = R.make_case(name, lut)
    ref = R.reference(case)
    R.check_conditions(case, ref)
    opt = lambda a, **kw: None if a is None else T(a, **kw)   # noqa: E731
    got = ops.render_sheet(T(case["images"]), opt(case["maps"]), opt(case["points"]), rows=R.ROWS, cols=R.COLS,
                           downscale=case["f"], pad=case["pad"], alpha=R.ALPHA, radius=R.RADIUS,
                           colors=torch.from_numpy(R.COLORS), lut=T(lut), overlay=case["overlay"])
    assert got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().numpy()
    diff = got.astype(np.int64) != ref[0].astype(np.int64)
    print(f"{name}: sheet {got.shape}, {int(diff.sum())} of {diff.size} bytes differ, "
          f"{float(R.in_band(ref[1]).mean()):.4f} of the bytes in the band")
    R.check(got, ref, case["f"])


def test_render_sheet_downscale4_float4_path(lut):
    """f = 4 takes the 16-byte source loads; a 2-marker, 3-image 2 × 2 sheet at H = W = 32."""
    from stablekeypoints_amd import ops
    g = np.random.default_rng(7)
    images = (g.integers(0, 4097, (3, 3, 32, 32)) / 4096.0).astype(np.float32)
    maps = g.random((3, 8, 8)).astype(np.float32)
    rng = R.map_range_ref(maps)
    ref = R.render_ref(images, maps, rng, lut, R.ALPHA, None, None, R.COLORS, 2, 2, 4, 2)
    assert R.in_band(ref[1]).mean() < R.MAX_BAND
    got = ops.render_sheet(T(images), T(maps), None, rows=2, cols=2, downscale=4, pad=2, alpha=R.ALPHA, lut=T(lut))
    R.check(got.cpu().numpy(), ref, 4)
    plain = ops.render_sheet(T(images), None, None, rows=2, cols=2, downscale=4, pad=2)
    ref_plain = R.render_ref(images, None, None, lut, R.ALPHA, None, None, R.COLORS, 2, 2, 4, 2)
    assert np.array_equal(plain.cpu().numpy(), ref_plain[0])    # 12-bit images: the 4×4 mean is exact


def test_render_sheet_defaults_and_determinism(lut):
    """Default radius, colours and LUT run; two calls give the same bytes."""
    from stablekeypoints_amd import ops
    case = R.make_case("a_f1_maps16", lut)
    args = (T(case["images"]), T(case["maps"]), T(case["points"]))
    a = ops.render_sheet(*args, rows=2, cols=3)
    b = ops.render_sheet(*args, rows=2, cols=3)
    assert tuple(a.shape) == ops.sheet_shape(16, 16, 2, 3) + (3,) and torch.equal(a, b)
    with pytest.raises(RuntimeError, match="rows\\*cols"):
        ops.render_sheet(args[0], rows=1, cols=3)
