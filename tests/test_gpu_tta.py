"""skp_tta_reduce / ops.tta_reduce, eval.predict_keypoints and the CLI's predict stage on the GPU.

The kernel is held to the sequential composition of the existing ops bit for bit (its arithmetic
is fixed to that end), to the float64 restatement tests/tta_ref.py within twice the composition's
own error, and to the chunked sums of run_image_with_context_augmented within the reordering bound
of two C-term sums of non-negative fp32 terms plus one division, (2C + 2)·2⁻²³.
"""
import numpy as np
import pytest
import torch

import tta_ref
import tta_tiny
from tta_tiny import AUG, DEV, S_UP, cli as _cli, predict as _predict, seed as _seed, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _chunked(maps, theta):
    """run_image_with_context_augmented's form: inverse(maps).sum(0) / inverse(ones).sum(0), NaN -> 0."""
    from stablekeypoints_amd import ops
    out, nums = [], []
    for b in range(maps.shape[0]):
        num = ops.affine_warp(torch.ones_like(maps[b]), theta[b]).sum(dim=0)
        a = ops.affine_warp(maps[b], theta[b]).sum(dim=0) / num
        a[a != a] = 0
        out.append(a)
        nums.append(num)
    return torch.stack(out), torch.stack(nums)


@pytest.fixture(scope="module", params=tta_ref.SHAPES, ids=lambda s: "B{}_C{}_n{}_S{}".format(*s))
def case(request):
    """One shape's inputs and every reference, computed once and left unchanged."""
    from stablekeypoints_amd import ops
    maps_np, theta_np, finite = tta_ref.make_case(request.param)
    maps, theta = torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV)
    seq_pos, seq_avg, _ = tta_tiny.sequential(maps, theta)
    ref_pos, ref_avg, ref_num = tta_ref.tta_ref(np.where(finite[:, None, :, None, None], maps_np, 0.0), theta_np)
    pos, avg = ops.tta_reduce(maps, theta, return_avg=True)
    pos_only, none = ops.tta_reduce(maps, theta)
    assert none is None
    torch.cuda.synchronize()
    return dict(shape=request.param, maps=maps, theta=theta, finite=finite, seq_pos=seq_pos, seq_avg=seq_avg,
                ref_avg=ref_avg, ref_num=ref_num, pos=pos, avg=avg, pos_only=pos_only)


def test_bit_equal_to_the_sequential_composition(case):
    assert case["avg"].shape == case["seq_avg"].shape and case["pos"].shape == case["seq_pos"].shape
    assert not torch.isnan(case["seq_avg"]).any()
    assert torch.equal(case["avg"], case["seq_avg"])
    assert torch.equal(case["pos"], case["seq_pos"])


def test_degenerate_cases(case):
    B, C, n, S = case["shape"]
    if case["shape"] == tta_ref.ALL_OUT_OF_VIEW:
        assert (case["avg"][-1] == 0).all() and (case["pos"][-1] == 0.5).all()
    if n > 1 or B > 1:   # token 0 of image 0 is all zero in every copy
        assert (case["avg"][0, 0] == 0).all() and (case["pos"][0, 0] == 0.5).all()
    else:
        assert (case["maps"][0, :, 0] != 0).any()


def test_against_float64_restatement(case):
    """avg within twice the largest error the sequential composition of the existing ops shows
    against tta_ref on the same inputs (NaN/inf tokens left to the bit-equality check)."""
    fin = torch.from_numpy(case["finite"]).to(DEV)
    ref = torch.from_numpy(case["ref_avg"]).to(DEV)
    own = float((case["seq_avg"].double() - ref)[fin].abs().max())
    got = float((case["avg"].double() - ref)[fin].abs().max())
    print(f"{case['shape']}: sequential composition vs float64 {own:.3e}, skp_tta_reduce vs float64 {got:.3e}")
    assert got <= 2 * own


def test_pos_does_not_depend_on_avg(case):
    assert torch.equal(case["pos"], case["pos_only"])


def test_against_the_chunked_legacy_sum(case):
    B, C, n, S = case["shape"]
    legacy, num = _chunked(case["maps"], case["theta"])
    fin = torch.from_numpy(case["finite"]).to(DEV)[:, :, None, None].expand_as(legacy)
    rtol = (2 * C + 2) * 2.0 ** -23
    some = fin & (num > 0)
    none = fin & (num == 0)
    a, l = case["avg"].double(), legacy.double()
    rel = float(((a - l).abs()[some] / l.abs()[some].clamp_min(1e-300)).max()) if some.any() else 0.0
    print(f"{case['shape']}: max relative difference to the chunked sum {rel:.3e} (bound {rtol:.3e})")
    assert ((a - l).abs()[some] <= rtol * l.abs()[some]).all()
    assert (case["avg"][none] == 0).all() and (legacy[none] == 0).all()


def test_tta_reduce_rejects_bad_shapes():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="theta_inv"):
        ops.tta_reduce(torch.zeros(1, 2, 1, 8, 8, device=DEV), torch.zeros(1, 3, 2, 3, device=DEV))
    with pytest.raises(ValueError, match="maps must be"):
        ops.tta_reduce(torch.zeros(1, 2, 1, 8, 4, device=DEV), torch.zeros(1, 2, 2, 3, device=DEV))


# ------------------------------------------------------------------------------------------ end to end
def test_predict_keypoints_tiny(tiny):
    from stablekeypoints_amd import eval as ev
    images = tiny[2]
    n = len(tiny[4])
    kp, maps = _predict(tiny, images, augmentation_iterations=3, return_maps=True)
    assert kp.shape == (2, n, 2) and maps.shape == (2, n, S_UP, S_UP)
    assert torch.isfinite(maps).all() and float(maps.max()) > 0
    assert torch.equal(kp, (ev.find_max_pixel(maps.reshape(2 * n, S_UP, S_UP)) / S_UP).reshape(2, n, 2))
    kp2, maps2 = _predict(tiny, images, augmentation_iterations=3, return_maps=True)
    assert torch.equal(kp, kp2) and torch.equal(maps, maps2)
    assert torch.equal(_predict(tiny, images, augmentation_iterations=3), kp)          # no maps asked for
    # one image per pass (the noise draws differ from the two-image pass, so only the shapes are pinned)
    assert _predict(tiny, images, augmentation_iterations=3, image_batch=1, return_maps=True)[1].shape == maps.shape
    wkp, wmaps = _predict(tiny, images, augmentation_iterations=3, max_loc_strategy="weighted_avg", return_maps=True)
    assert torch.equal(wmaps, maps)
    ref = ev.pixel_from_weighted_avg(maps.clone().reshape(2 * n, S_UP, S_UP)) / S_UP
    assert torch.equal(wkp, ref.reshape(2, n, 2))
    W = torch.randn(2 * n, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    kp3, reg = _predict(tiny, images, augmentation_iterations=3, regressor=W)
    assert torch.equal(kp3, kp) and reg.shape == (2, 4, 2)
    assert torch.equal(reg, ((kp.reshape(2, -1) - 0.5) @ W + 0.5).reshape(2, -1, 2))
    assert _predict(tiny, images[0], augmentation_iterations=3).shape == (1, n, 2)     # a single (3, H, W) image


def test_predict_keypoints_matches_legacy_tta(tiny):
    """B = 1, same seeds, both capturing the same three copies in one pass: the averages agree
    within the reordering bound (2C + 2)·2⁻²³ of the kernel test."""
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, indices = tiny
    C = 3
    _, maps = _predict(tiny, images[:1], augmentation_iterations=C, image_batch=1, return_maps=True)
    _seed()
    legacy = ev.run_image_with_context_augmented(ldm, images[0], ctx, indices, device=DEV, layers=[0, 1, 2, 3],
                                                 augmentation_iterations=C, controllers=controllers, num_gpus=1,
                                                 upscale_size=S_UP, augmentation_batch=C, **AUG)
    a, l = maps[0].double(), legacy.double()
    rtol = (2 * C + 2) * 2.0 ** -23
    rel = float(((a - l).abs() / l.abs().clamp_min(1e-300))[l != 0].max())
    print(f"predict_keypoints vs run_image_with_context_augmented: max relative difference {rel:.3e} (bound {rtol:.3e})")
    assert ((a - l).abs() <= rtol * l.abs()).all()


def test_predict_keypoints_refuses_a_process_group(tiny, monkeypatch):
    from stablekeypoints_amd import optimize
    monkeypatch.setattr(optimize, "_world", lambda: (2, 0))
    with pytest.raises(ValueError, match="single process"):
        _predict(tiny, tiny[2], augmentation_iterations=1)


def test_cli_predict_stage_tiny(tmp_path):
    import csv
    out = tmp_path / "run"
    kp = _cli(out)
    assert kp.shape == (5, 5, 2) and kp.dtype == torch.float32
    assert (kp > 0).all() and (kp < 1).all()
    rows = list(csv.reader(open(out / "keypoints.csv")))
    assert len(rows) == 5 and [r[0] for r in rows] == [str(i) for i in range(5)]
    assert np.array_equal(np.array(rows, dtype=np.float64)[:, 1:].astype(np.float32), kp.reshape(5, -1).numpy())
    assert not (out / "all_errors.pt").exists() and not (out / "regressed_keypoints.pt").exists()
    assert not (out / "regressor.pt").exists() and not (out / "source_keypoints.pt").exists()
    # with a saved regressor the regressed keypoints are written too
    torch.save(torch.randn(10, 30, generator=torch.Generator().manual_seed(8)), out / "regressor.pt")
    _cli(out)
    reg = torch.load(out / "regressed_keypoints.pt", weights_only=True)
    assert reg.shape == (5, 15, 2) and torch.load(out / "keypoints.pt", weights_only=True).shape == kp.shape
    assert len(list(csv.reader(open(out / "keypoints.csv")))[0]) == 1 + 10 + 30
