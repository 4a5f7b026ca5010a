"""skp_tta_reduce_entropy / ops.tta_reduce_entropy, eval.find_corresponding_points,
eval.correspond_images and the CLI's predict stage with --correspond on the GPU.

The kernel's pos and avg are held to ops.tta_reduce bit for bit, its entropy to the direct float64
entropy of tests/corr_ref.py on that average read back: both sides are double arithmetic on the same
fp32 values, so they differ by summation order and the two-ulp exp / log, about S²·2⁻⁵³·log S² ≈ 1e-11
at S = 96; the bound is 1e-9.  The selections are held to what the reference's
find_corresponding_points returned (tests/golden/corresponding_points.npz); tests/test_corr_cpu.py shows
that those rankings have gaps of 3e-3 and more, which entitles an fp32 average to the same answer.
"""
import math
import os

import numpy as np
import pytest
import torch

import corr_ref
import tta_ref
import tta_tiny
from tta_tiny import DEV, N_TOK, bits as _bits, cli as _cli, correspond as _correspond, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1, 37), (2, 3, 5, 37), (2, 10, 23, 64), (1, 2, 41, 96))
SCALES = (1.0, 7.5)
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corresponding_points.npz"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ------------------------------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "B{}_C{}_n{}_S{}".format(*s))
def case(request):
    """One shape's inputs, the plain reduce, and the entropy reduce at every scale with and without
    the average, computed once."""
    from stablekeypoints_amd import ops
    shape = request.param
    maps_np, theta_np, finite = tta_ref.make_case(shape)
    maps, theta = torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV)
    plain_pos, plain_avg = ops.tta_reduce(maps, theta, return_avg=True)
    got = {s: ops.tta_reduce_entropy(maps, theta, scale=s, return_avg=True) for s in SCALES}
    got_noavg = {s: ops.tta_reduce_entropy(maps, theta, scale=s) for s in SCALES}
    torch.cuda.synchronize()
    return dict(shape=shape, maps=maps, theta=theta, finite=finite, plain_pos=plain_pos, plain_avg=plain_avg,
                avg_np=plain_avg.cpu().numpy(), got=got, got_noavg=got_noavg)


def test_pos_and_avg_are_tta_reduce_s(case):
    B, C, n, S = case["shape"]
    for s in SCALES:
        pos, ent, avg = case["got"][s]
        assert pos.shape == (B, n, 2) and avg.shape == (B, n, S, S)
        assert ent.shape == (B, n) and ent.dtype == torch.float64
        assert torch.equal(_bits(pos), _bits(case["plain_pos"]))
        assert torch.equal(_bits(avg), _bits(case["plain_avg"]))


def test_entropy_is_the_direct_entropy_of_the_average(case):
    for s in SCALES:
        ent = case["got"][s][1].cpu().numpy()
        want = corr_ref.entropy_ref(case["avg_np"], s)
        assert np.array_equal(np.isnan(ent), np.isnan(want))
        err = np.nanmax(np.abs(ent - want)) if not np.isnan(want).all() else 0.0
        print(case["shape"], "scale", s, "max |entropy - ref|", err)
        assert err <= 1e-9


def test_degenerate_tokens(case):
    B, C, n, S = case["shape"]
    for s in SCALES:
        ent = case["got"][s][1]
        if case["shape"] == tta_ref.ALL_OUT_OF_VIEW:     # the last image: every copy out of view, the average is 0
            assert (case["plain_avg"][-1] == 0).all()
            assert ((ent[-1] - math.log(S * S)).abs() <= 1e-12).all()
        if n > 1 or B > 1:                               # token 0 of image 0 is all zero in every copy
            assert abs(float(ent[0, 0]) - math.log(S * S)) <= 1e-12
        if n > 2:                                        # token 1 of image 0 holds +inf: its average does too
            assert torch.isinf(case["plain_avg"][0, 1]).any() and torch.isnan(ent[0, 1])
        assert torch.isfinite(ent[torch.from_numpy(case["finite"]).to(ent.device)]).all()


def test_results_do_not_depend_on_return_avg(case):
    for s in SCALES:
        pos, ent, _ = case["got"][s]
        pos2, ent2, none = case["got_noavg"][s]
        assert none is None
        assert torch.equal(_bits(pos), _bits(pos2))
        assert torch.equal(ent.view(torch.int64), ent2.view(torch.int64))


def test_workspace_reuse_across_scales(case):
    from stablekeypoints_amd import ops
    ops.tta_reduce_entropy(case["maps"], case["theta"], scale=SCALES[1])
    pos, ent, _ = ops.tta_reduce_entropy(case["maps"], case["theta"], scale=SCALES[0])
    want_pos, want_ent, _ = case["got"][SCALES[0]]
    assert torch.equal(_bits(pos), _bits(want_pos)) and torch.equal(ent.view(torch.int64), want_ent.view(torch.int64))


def test_tta_reduce_entropy_rejects_bad_arguments():
    from stablekeypoints_amd import ops
    m, th = torch.zeros(1, 2, 1, 8, 8, device=DEV), torch.zeros(1, 2, 2, 3, device=DEV)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            ops.tta_reduce_entropy(m, th, scale=bad)
    with pytest.raises(ValueError, match="theta_inv"):
        ops.tta_reduce_entropy(m, torch.zeros(1, 3, 2, 3, device=DEV))
    with pytest.raises(ValueError, match="maps must be"):
        ops.tta_reduce_entropy(torch.zeros(1, 2, 1, 8, 4, device=DEV), th)


# ------------------------------------------------------------------------------------------ the selection
@pytest.fixture(scope="module", params=corr_ref.CASES, ids=lambda s: "x".join(map(str, s)))
def planted(request):
    from stablekeypoints_amd import ops
    shape = request.param
    maps_np, theta_np = corr_ref.planted(shape)
    maps, theta = torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV)
    tag = "x".join(map(str, shape))
    return dict(shape=shape, maps=maps, theta=theta, avg=ops.tta_reduce(maps, theta, return_avg=True)[1],
                indices=GOLDEN[f"{tag}_indices"], points=GOLDEN[f"{tag}_points"])


def test_find_corresponding_points_is_the_reference(planted):
    from stablekeypoints_amd import eval as ev
    points, indices = ev.find_corresponding_points(planted["avg"], corr_ref.K)
    assert indices.dtype == torch.int64 and indices.shape == (corr_ref.K,)
    assert np.array_equal(indices.cpu().numpy(), planted["indices"])
    assert points.shape == (planted["shape"][0], corr_ref.K, 2)
    assert np.array_equal(points.cpu().numpy(), planted["points"])


def test_fused_selection_is_the_reference(planted):
    """tta_reduce_entropy -> the in-order sum -> skp_topk_keys picks the reference's tokens, and the
    fused reduce's positions at those tokens are the reference's points."""
    from stablekeypoints_amd import eval as ev, ops
    pos, ent, _ = ops.tta_reduce_entropy(planted["maps"], planted["theta"])
    total = ev._sum_in_order(ent)
    indices = ev._rank_ascending(total, corr_ref.K)
    assert np.array_equal(indices.cpu().numpy(), planted["indices"])
    assert np.array_equal(pos[:, indices].cpu().numpy(), planted["points"])
    want = corr_ref.sum_in_order(corr_ref.entropy_ref(planted["avg"].cpu().numpy()))
    assert np.abs(total.cpu().numpy() - want).max() <= 1e-9 * planted["shape"][0]


# ------------------------------------------------------------------------------------------ end to end
def test_correspond_images_tiny(tiny):
    from stablekeypoints_amd import eval as ev
    M, k = 2, 4
    corr = _correspond(tiny, num_points=k)
    assert isinstance(corr, ev.Correspondences)
    assert corr.indices.shape == (k,) and corr.indices.dtype == torch.int64
    assert corr.points.shape == (M, k, 2) and corr.points.dtype == torch.float32
    assert corr.entropy.shape == (N_TOK,) and corr.entropy.dtype == torch.float64
    assert corr.image_entropy.shape == (M, N_TOK) and corr.image_entropy.dtype == torch.float64
    every = tiny[:4] + (torch.arange(N_TOK),)
    kp, maps = tta_tiny.predict(every, tiny[2], augmentation_iterations=3, image_batch=2, return_maps=True)
    want = corr_ref.entropy_ref(maps.cpu().numpy())
    image_entropy = corr.image_entropy.cpu().numpy()
    print("max |image_entropy - ref|", np.abs(image_entropy - want).max())
    assert np.abs(image_entropy - want).max() <= 1e-9
    assert np.abs(corr.entropy.cpu().numpy() - corr_ref.sum_in_order(want)).max() <= 1e-9 * M
    order = np.argsort(corr.entropy.cpu().numpy(), kind="stable")[:k]
    assert np.array_equal(corr.indices.cpu().numpy(), order)
    assert torch.equal(corr.points, kp[:, corr.indices])
    # a second call from the same seed gives the same bits
    again = _correspond(tiny, num_points=k)
    assert all(torch.equal(a, b) for a, b in zip(corr, again))


def test_correspond_images_candidates_tiny(tiny):
    cand = [3, 7, 0, 12, 5]
    corr = _correspond(tiny, num_points=3, candidates=cand)
    assert corr.entropy.shape == (5,) and corr.image_entropy.shape == (2, 5) and corr.points.shape == (2, 3, 2)
    order = np.argsort(corr.entropy.cpu().numpy(), kind="stable")[:3]
    assert corr.indices.tolist() == [cand[i] for i in order]
    # tiny's own indices are `cand`
    kp, maps = tta_tiny.predict(tiny, tiny[2], augmentation_iterations=3, image_batch=2, return_maps=True)
    assert np.abs(corr.image_entropy.cpu().numpy() - corr_ref.entropy_ref(maps.cpu().numpy())).max() <= 1e-9
    assert torch.equal(corr.points, kp[:, torch.from_numpy(order).to(kp.device)])
    many = _correspond(tiny, num_points=9, candidates=cand)     # more points than candidates: all of them, ranked
    assert sorted(many.indices.tolist()) == sorted(cand) and many.indices.tolist()[:3] == corr.indices.tolist()


def test_cli_correspond_tiny(tmp_path):
    from PIL import Image
    from stablekeypoints_amd import ops

    def run(folder, *extra, indices=None):
        return _cli(folder, "--top_k", "3", *extra, indices=indices)

    out = tmp_path / "correspond"
    kp = run(out, "--correspond", "--correspond_size", "64", "--visualize")     # no indices.pt in the folder
    idx = torch.load(out / "correspondence_indices.pt", weights_only=True)
    ent = torch.load(out / "correspondence_entropy.pt", weights_only=True)
    pts = torch.load(out / "correspondence_points.pt", weights_only=True)
    assert idx.shape == (3,) and idx.dtype == torch.int64 and len(set(idx.tolist())) == 3
    assert ent.shape == (N_TOK,) and ent.dtype == torch.float64 and torch.isfinite(ent).all()
    assert pts.shape == (5, 3, 2) and pts.dtype == torch.float32 and ((pts > 0) & (pts < 1)).all()
    assert idx.tolist() == np.argsort(ent.numpy(), kind="stable")[:3].tolist()
    assert kp.shape == (5, 3, 2)
    assert not (out / "indices.pt").exists()
    sheet = Image.open(out / "correspondences.png")
    assert sheet.size[::-1] == ops.sheet_shape(512, 512, 1, 5, downscale=2)
    plain = tmp_path / "plain"
    kp_plain = run(plain, indices=idx)
    assert torch.equal(kp_plain, kp)
    assert open(plain / "keypoints.csv").read() == open(out / "keypoints.csv").read()
    assert not (plain / "correspondence_indices.pt").exists()
