"""skp_tta_reduce_scored / ops.tta_reduce_scored, eval.predict_keypoints(return_scores=True) and
the CLI's --keypoint_scores on the GPU.

The reference of every kernel check is the sequential composition of the ops that existed before
the scored reduce (affine_warp per copy, sums in copy order, the division, NaN -> 0,
find_max_pixel; here it also keeps the sum of the warped ones) plus torch float64 on its result,
ops.pixel_from_weighted_avg on it, and the float64 restatement tests/tta_score_ref.py.  Only
the token that make_case marks non-finite (NaN and inf planted in its maps) is left out of the
checks on the scores and the refined position: for it the call has to return, no more.
"""
import csv

import numpy as np
import pytest
import torch

import tta_ref
import tta_score_ref
from tta_tiny import DEV, S_UP, cli as _cli, predict as _predict, sequential as _sequential, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# (kind, shape, distance): the shared shapes at 5, the planted ones at 5, one of them at 1.5 and 16
CASES = ([("random", s, 5.0) for s in tta_ref.SHAPES] + [("planted", s, 5.0) for s in tta_score_ref.PLANTED] +
         [("planted", tta_score_ref.PLANTED[0], 1.5), ("planted", tta_score_ref.PLANTED[0], 16.0)])


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "{}_B{}_C{}_n{}_S{}_d{}".format(c[0], *c[1], c[2]))
def case(request):
    """One case's inputs, the outputs under test and every reference, computed once and left unchanged."""
    from stablekeypoints_amd import ops
    kind, shape, distance = request.param
    B, C, n, S = shape
    if kind == "random":
        maps_np, theta_np, finite = tta_ref.make_case(shape)
        plan = None
    else:
        maps_np, theta_np, plan = tta_score_ref.make_planted(shape)
        finite = np.ones((B, n), bool)
    maps, theta = torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV)
    seq_pos, seq_avg, seq_num = _sequential(maps, theta)
    plain_pos, plain_avg = ops.tta_reduce(maps, theta, return_avg=True)
    pos, refined, scores, avg = ops.tta_reduce_scored(maps, theta, distance=distance, return_avg=True)
    pos2, refined2, scores2, none = ops.tta_reduce_scored(maps, theta, distance=distance)
    assert none is None
    op_refined = ops.pixel_from_weighted_avg(seq_avg.clone().reshape(B * n, S, S), distance).reshape(B, n, 2)
    torch.cuda.synchronize()
    ref = tta_score_ref.scores_ref(np.where(finite[:, :, None, None], seq_avg.cpu().numpy(), 0.0),
                                   seq_num.cpu().numpy(), C, distance)
    return dict(kind=kind, shape=shape, distance=distance, plan=plan, fin=torch.from_numpy(finite).to(DEV),
                seq_pos=seq_pos, seq_avg=seq_avg, seq_num=seq_num, plain_pos=plain_pos, plain_avg=plain_avg,
                pos=pos, refined=refined, scores=scores, avg=avg, pos2=pos2, refined2=refined2, scores2=scores2,
                op_refined=op_refined, ref=ref)


def _peak_index(case):
    B, C, n, S = case["shape"]
    p = (case["seq_pos"] - 0.5).long()
    return p[..., 0], p[..., 1]


def test_pos_and_avg_are_tta_reduce(case):
    assert case["pos"].shape == case["plain_pos"].shape and case["scores"].shape == case["pos"].shape[:2] + (3,)
    assert case["refined"].shape == case["pos"].shape
    assert torch.equal(case["pos"], case["plain_pos"]) and torch.equal(case["avg"], case["plain_avg"])
    assert torch.equal(case["pos"], case["seq_pos"]) and torch.equal(case["avg"], case["seq_avg"])
    assert torch.equal(case["pos2"], case["pos"])     # the same without the average


def test_two_calls_give_equal_bits(case):
    """With and without the average written: the same launches otherwise, so the same bits (NaN
    compared as bits too, the non-finite token included)."""
    for a, b in (("refined", "refined2"), ("scores", "scores2"), ("pos", "pos2")):
        assert torch.equal(case[a].view(torch.int32), case[b].view(torch.int32))
    from stablekeypoints_amd import ops
    B, C, n, S = case["shape"]
    if case["kind"] == "planted" and case["distance"] == 5.0:   # a third call, all four outputs
        maps_np, theta_np, _ = tta_score_ref.make_planted(case["shape"])
        out = ops.tta_reduce_scored(torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV),
                                    distance=5.0, return_avg=True)
        for got, name in zip(out, ("pos", "refined", "scores", "avg")):
            assert torch.equal(got.view(torch.int32), case[name].view(torch.int32))


def test_peak_is_the_maximum_of_the_sequential_average(case):
    fin = case["fin"]
    assert torch.equal(case["scores"][..., 0][fin], case["seq_avg"].amax(dim=(2, 3))[fin])


def test_coverage_is_num_at_the_peak_over_C(case):
    B, C, n, S = case["shape"]
    r, c = _peak_index(case)
    b = torch.arange(B, device=DEV)[:, None].expand(B, n)
    # the IEEE fp32 quotient, formed by numpy (torch divides a device tensor by a scalar through its reciprocal)
    want = case["seq_num"][b, r, c].cpu().numpy() / np.float32(C)
    fin = case["fin"].cpu().numpy()
    assert want.dtype == np.float32 and np.array_equal(case["scores"][..., 2].cpu().numpy()[fin], want[fin])


def test_concentration_against_float64_sums(case):
    """Σ_disc / (Σ_all + 1e-6) of the sequential average, both sums in torch float64; both sides
    sum the same fp32 values in double, so what remains is the final rounding to fp32: 2⁻²²."""
    B, C, n, S = case["shape"]
    a = case["seq_avg"].double()
    r, c = _peak_index(case)
    rows = torch.arange(S, device=DEV, dtype=torch.float32)[None, None, :, None]
    cols = torch.arange(S, device=DEV, dtype=torch.float32)[None, None, None, :]
    dx, dy = rows - r[..., None, None].float(), cols - c[..., None, None].float()
    keep = (dx * dx + dy * dy).double().sqrt().float() <= case["distance"]
    want = (a * keep).sum(dim=(2, 3)) / (a.sum(dim=(2, 3)) + 1e-6)
    got = case["scores"][..., 1].double()
    fin = case["fin"]
    err = (got - want).abs()[fin]
    rel = float((err / want.abs()[fin].clamp_min(1e-300)).max())
    print(f"{case['kind']} {case['shape']} d={case['distance']}: concentration, max relative error {rel:.3e} "
          f"(bound {2.0 ** -22:.3e})")
    assert (err <= 2.0 ** -22 * want.abs()[fin]).all()
    # and the float64 restatement, which shares no code with the line above
    assert np.allclose(want[fin].cpu().numpy(), case["ref"]["concentration"][fin.cpu().numpy()], rtol=1e-12, atol=0)


def test_refined_against_the_existing_op(case):
    """ops.pixel_from_weighted_avg on the sequential average: both are double sums of at most
    (2·16 + 1)² identical fp32 products in different orders, rounded to fp32 at magnitude <= S."""
    B, C, n, S = case["shape"]
    fin = case["fin"]
    d = float((case["refined"].double() - case["op_refined"].double()).abs()[fin].max())
    print(f"{case['kind']} {case['shape']} d={case['distance']}: refined vs pixel_from_weighted_avg {d:.3e} "
          f"(bound {S * 2.0 ** -22:.3e})")
    assert d <= S * 2.0 ** -22


def test_refined_against_float64_restatement(case):
    """Within twice the error the existing op itself shows against the restatement on the same inputs."""
    fin = case["fin"]
    ref = torch.from_numpy(case["ref"]["refined"]).to(DEV)
    own = float((case["op_refined"].double() - ref).abs()[fin].max())
    got = float((case["refined"].double() - ref).abs()[fin].max())
    print(f"{case['kind']} {case['shape']} d={case['distance']}: pixel_from_weighted_avg vs float64 {own:.3e}, "
          f"skp_tta_reduce_scored vs float64 {got:.3e}")
    assert got <= 2 * own


def test_degenerate_tokens(case):
    B, C, n, S = case["shape"]
    if case["kind"] != "random":
        return
    if case["shape"] == tta_ref.ALL_OUT_OF_VIEW:     # the last image: every copy out of view
        assert (case["scores"][-1, :, 2] == 0).all() and (case["scores"][-1, :, 0] == 0).all()
        assert (case["scores"][-1, :, 1] == 0).all() and (case["refined"][-1] == 0.5).all()
    if n > 1 or B > 1:   # token 0 of image 0 is all zero in every copy
        assert case["scores"][0, 0, 0] == 0 and case["scores"][0, 0, 1] == 0
        assert (case["refined"][0, 0] == 0.5).all() and (case["pos"][0, 0] == 0.5).all()


def test_planted(case):
    if case["kind"] != "planted":
        return
    B, C, n, S = case["shape"]
    pos, scores, refined, ref = case["pos"].cpu(), case["scores"].cpu(), case["refined"].cpu(), case["ref"]
    sharp, diffuse = [], []
    for b, (ident, tokens) in enumerate(case["plan"]):
        want_cov = torch.tensor(float(sum(ident)), dtype=torch.float32) / C
        for t, (kind, r, c) in enumerate(tokens):
            assert tuple(pos[b, t].tolist()) == (r + 0.5, c + 0.5)
            # identity copies: num is their count up to the fp32 rounding of the identity grid
            assert abs(float(scores[b, t, 2]) - float(want_cov)) <= 1e-4
            if kind == "zero":
                assert scores[b, t, 0] == 0 and scores[b, t, 1] == 0 and tuple(refined[b, t].tolist()) == (0.5, 0.5)
                continue
            (sharp if kind == "sharp" else diffuse).append(float(scores[b, t, 1]))
            if kind == "diffuse":
                assert abs(float(scores[b, t, 1]) / ref["disc_share"][b, t] - 1) <= 0.1
            else:
                assert abs(float(scores[b, t, 0]) - 1.0) <= 1e-4
    print(f"planted {case['shape']} d={case['distance']}: sharp concentrations >= {min(sharp):.4f}, "
          f"diffuse <= {max(diffuse):.4f}")
    assert min(sharp) > max(diffuse)


def test_tta_reduce_scored_rejects_bad_arguments():
    from stablekeypoints_amd import ops
    m, th = torch.zeros(1, 2, 1, 8, 8, device=DEV), torch.zeros(1, 2, 2, 3, device=DEV)
    with pytest.raises(ValueError, match="theta_inv"):
        ops.tta_reduce_scored(m, torch.zeros(1, 3, 2, 3, device=DEV))
    with pytest.raises(ValueError, match="maps must be"):
        ops.tta_reduce_scored(torch.zeros(1, 2, 1, 8, 4, device=DEV), th)
    for bad in (0, -1, 17):
        with pytest.raises(ValueError, match="distance"):
            ops.tta_reduce_scored(m, th, distance=bad)


# ------------------------------------------------------------------------------------------ end to end
def test_predict_keypoints_scores_tiny(tiny, monkeypatch):
    """kp and the maps are what they are without the scores.  The scores are those of
    ops.tta_reduce_scored on the pass's captured maps (recorded here as predict_keypoints calls
    it), and they are the scores of the returned averages: the peak is their maximum, the
    concentration their float64 mass ratio within 2⁻²², the refined point ops.pixel_from_weighted_avg
    of them within S·2⁻²² pixels."""
    from stablekeypoints_amd import eval as ev, ops
    images, n, C, dist = tiny[2], len(tiny[4]), 3, 5
    kp, maps = _predict(tiny, images, augmentation_iterations=C, return_maps=True)
    calls = []
    real = ops.tta_reduce_scored

    def spy(m, th, **kw):
        out = real(m, th, **kw)
        calls.append((kw, out, real(m.clone(), th.clone(), **kw)))
        return out

    monkeypatch.setattr(ops, "tta_reduce_scored", spy)
    kp_s, maps_s, sc = _predict(tiny, images, augmentation_iterations=C, return_maps=True, return_scores=True,
                                score_distance=dist)
    monkeypatch.undo()
    assert torch.equal(kp_s, kp) and torch.equal(maps_s, maps)
    assert isinstance(sc, ev.KeypointScores)
    assert sc.peak.shape == sc.concentration.shape == sc.coverage.shape == (2, n) and sc.refined.shape == (2, n, 2)
    assert len(calls) == 1 and calls[0][0] == dict(distance=dist, return_avg=True)
    for (pos, refined, scores, avg) in calls[0][1:]:     # the call itself, and the same op on copies of its inputs
        assert torch.equal(pos / S_UP, kp) and torch.equal(avg, maps)
        assert torch.equal(sc.peak, scores[..., 0]) and torch.equal(sc.concentration, scores[..., 1])
        assert torch.equal(sc.coverage, scores[..., 2]) and torch.equal(sc.refined, refined / S_UP)
    # against the returned averages
    assert torch.equal(sc.peak, maps.amax(dim=(2, 3)))
    ref = tta_score_ref.scores_ref(maps.cpu().numpy(), np.ones((2, S_UP, S_UP)), 1, dist)
    want = torch.from_numpy(ref["concentration"]).to(DEV)
    assert ((sc.concentration.double() - want).abs() <= 2.0 ** -22 * want).all()
    op = ops.pixel_from_weighted_avg(maps.clone().reshape(2 * n, S_UP, S_UP), dist).reshape(2, n, 2)
    assert float((sc.refined * S_UP - op).abs().max()) <= S_UP * 2.0 ** -22
    assert ((sc.coverage > 0) & (sc.coverage <= 1)).all()
    assert ((sc.refined - kp).abs() <= dist / S_UP).all()
    # without the maps, with a regressor, and with weighted_avg: the scores come last and kp is unchanged
    kp2, sc2 = _predict(tiny, images, augmentation_iterations=C, return_scores=True)
    assert torch.equal(kp2, kp) and all(torch.equal(a, b) for a, b in zip(sc2, sc))
    W = torch.randn(2 * n, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    kp3, reg, sc3 = _predict(tiny, images, augmentation_iterations=C, regressor=W, return_scores=True)
    assert torch.equal(kp3, kp) and reg.shape == (2, 4, 2) and all(torch.equal(a, b) for a, b in zip(sc3, sc))
    wkp = _predict(tiny, images, augmentation_iterations=C, max_loc_strategy="weighted_avg")
    wkp_s, wsc = _predict(tiny, images, augmentation_iterations=C, max_loc_strategy="weighted_avg", return_scores=True)
    assert torch.equal(wkp_s, wkp) and all(torch.equal(a, b) for a, b in zip(wsc, sc))


def test_cli_keypoint_scores_tiny(tmp_path):
    names = ("keypoint_scores.pt", "refined_keypoints.pt", "keypoint_scores.csv")
    plain = _cli(tmp_path / "plain")
    assert not any((tmp_path / "plain" / f).exists() for f in names)
    out = tmp_path / "scored"
    kp = _cli(out, "--keypoint_scores")
    assert torch.equal(kp, plain)
    assert open(out / "keypoints.csv").read() == open(tmp_path / "plain" / "keypoints.csv").read()
    scores = torch.load(out / "keypoint_scores.pt", weights_only=True)
    refined = torch.load(out / "refined_keypoints.pt", weights_only=True)
    assert scores.shape == (5, 5, 3) and refined.shape == (5, 5, 2)
    assert scores.dtype == torch.float32 and refined.dtype == torch.float32
    assert torch.isfinite(scores).all() and (scores[..., 1] > 0).all() and (scores[..., 1] <= 1).all()
    assert (scores[..., 2] > 0).all() and (scores[..., 2] <= 1).all()
    assert ((refined - kp).abs() <= 5 / 512).all()
    rows = list(csv.reader(open(out / "keypoint_scores.csv")))
    assert len(rows) == 5 and [r[0] for r in rows] == [str(i) for i in range(5)] and len(rows[0]) == 1 + 5 * 5
    table = np.array(rows, dtype=np.float64)[:, 1:].astype(np.float32).reshape(5, 5, 5)
    assert np.array_equal(table[..., :2], refined.numpy()) and np.array_equal(table[..., 2:], scores.numpy())
