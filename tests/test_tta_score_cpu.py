"""CPU-side checks of the scored TTA reduce (no GPU needed): the float64 restatement
tests/tta_score_ref.py against the numpy oracle, the parser, and the argument checks of
skp_tta_reduce_scored through the C ABI."""
import numpy as np
import pytest
import torch

import tta_abi
import tta_ref
import tta_score_ref


def test_centroid_matches_the_oracle_exactly_representable_map():
    """oracle.skp_oracle.pixel_from_weighted_avg works in fp32, the restatement in float64, so
    1e-12 can hold only where the oracle's arithmetic is exact: the kept values are k·2⁴⁰ with
    the k summing to 16, so the total (2⁴⁴) absorbs the 1e-6 in fp32, every quotient is k/16 and
    every product and sum is a short dyadic number.  The restatement keeps the 1e-6: a relative
    2⁻⁴⁴·1e-6 ≈ 6e-20.  Pixels at distance exactly 5 (offset (3, 4), kept) and √26 (offset
    (5, 1), dropped) sit on either side of the predicate."""
    from oracle import skp_oracle as O
    S, u = 24, 2.0 ** 40
    m = np.zeros((2, S, S), np.float32)
    # token 0: peak (10, 12); kept (10, 13), (12, 12), (13, 16) at distance 5; dropped (15, 13), (3, 3)
    for (r, c), k in {(10, 12): 6, (10, 13): 4, (12, 12): 3, (13, 16): 3, (15, 13): 5, (3, 3): 2}.items():
        m[0, r, c] = k * u
    # token 1: peak in the corner (0, 0), the disc clipped on two sides; kept (0, 5), (3, 4); dropped (1, 5)
    for (r, c), k in {(0, 0): 8, (0, 5): 4, (3, 4): 4, (1, 5): 7, (20, 20): 1}.items():
        m[1, r, c] = k * u
    ref = tta_score_ref.scores_ref(m[None], np.ones((1, S, S)), 1, 5)
    pos, mutated = O.pixel_from_weighted_avg(m, 5)
    assert mutated[0, 15, 13] == 0 and mutated[0, 13, 16] != 0 and mutated[1, 1, 5] == 0 and mutated[1, 3, 4] != 0
    d = float(np.abs(ref["refined"][0] - pos.astype(np.float64)).max())
    print(f"max |restatement - oracle| = {d:.3e}")
    assert d <= 1e-12
    assert np.array_equal(ref["refined"][0], [[(10 * 10 + 12 * 3 + 13 * 3) / 16 + 0.5, (12 * 9 + 13 * 4 + 16 * 3) / 16 + 0.5],
                                              [(3 * 4) / 16 + 0.5, (5 * 4 + 4 * 4) / 16 + 0.5]])
    assert np.array_equal(ref["peak"][0], [6 * u, 8 * u])
    assert np.allclose(ref["concentration"][0], [16 / 23, 16 / 24], rtol=1e-15)


def test_centroid_matches_the_oracle_on_a_random_map():
    """A continuous map: the oracle rounds the total, the total + 1e-6, each quotient and each
    product to fp32 (4·2⁻²⁴ relative per term, the terms summing to at most S), then the result
    (S·2⁻²⁴): S·2⁻²¹ bounds the difference."""
    from oracle import skp_oracle as O
    S = 37
    m = np.random.default_rng(5).random((4, S, S)).astype(np.float32)
    ref = tta_score_ref.scores_ref(m[None], np.ones((1, S, S)), 1, 5)
    pos, _ = O.pixel_from_weighted_avg(m, 5)
    d = float(np.abs(ref["refined"][0] - pos.astype(np.float64)).max())
    print(f"max |restatement - oracle| = {d:.3e} (bound {S * 2.0 ** -21:.3e})")
    assert d <= S * 2.0 ** -21


def test_planted_cases_in_float64():
    """The planted cases are what they claim, through the float64 restatements alone."""
    for shape in tta_score_ref.PLANTED:
        B, C, n, S = shape
        maps, theta, plan = tta_score_ref.make_planted(shape)
        pos, avg, num = tta_ref.tta_ref(maps, theta)
        ref = tta_score_ref.scores_ref(avg, num, C, 5)
        sharp, diffuse = [], []
        for b, (ident, tokens) in enumerate(plan):
            for t, (kind, r, c) in enumerate(tokens):
                assert tuple(pos[b, t]) == (r + 0.5, c + 0.5)
                assert abs(ref["coverage"][b, t] - sum(ident) / C) <= 1e-12
                if kind == "zero":
                    assert ref["peak"][b, t] == 0 and ref["concentration"][b, t] == 0
                    assert tuple(ref["refined"][b, t]) == (0.5, 0.5)
                else:
                    (sharp if kind == "sharp" else diffuse).append(ref["concentration"][b, t])
                if kind == "diffuse":
                    assert abs(ref["concentration"][b, t] / ref["disc_share"][b, t] - 1) <= 0.1
        assert min(sharp) > max(diffuse)


def test_parser_accepts_keypoint_scores():
    from stablekeypoints_amd.main import build_parser
    p = build_parser()
    assert p.parse_args([]).keypoint_scores is False
    assert p.parse_args(["--start_from_stage", "predict", "--keypoint_scores"]).keypoint_scores is True
    action = next(a for a in p._actions if a.dest == "start_from_stage")
    assert list(action.choices) == ["optimize", "find_indices", "precompute", "evaluate", "predict"]


def test_ops_tta_reduce_scored_refuses_cpu_tensors():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tta_reduce_scored(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 2, 3))


def test_keypoint_scores_fields():
    import stablekeypoints_amd.eval as ev
    assert ev.KeypointScores._fields == ("peak", "concentration", "coverage", "refined")


def test_tta_reduce_scored_rejects_bad_arguments_without_gpu():
    """The distance and the workspace query; the checks every reduce shares are in tests/test_tta_cpu.py."""
    L = tta_abi.library()
    for bad in (0.0, -1.0, 17.0, float("nan")):     # slot 6 of skp_tta_reduce_scored
        assert tta_abi.rc_with(L, "skp_tta_reduce_scored", a6=bad) == -1 and b"distance" in L.skp_last_error()
    # the workspace query: the partials of skp_tta_reduce, a double per tile, and the merged results
    for B, n, S in ((1, 10, 512), (2, 5, 37), (1, 1, 2), (4, 10, 512)):
        assert L.skp_tta_reduce_scored_workspace(B, n, S) >= L.skp_tta_reduce_workspace(B, n, S) > 0
    assert L.skp_tta_reduce_scored_workspace(1, 10, 512) == 10 * ((8 * 128) * 16 + 16)
    assert L.skp_tta_reduce_scored_workspace(0, 1, 8) == -1 and L.skp_tta_reduce_scored_workspace(1, 1, -3) == -1
    assert L.skp_tta_reduce_scored_workspace(1, 0, 8) == -1 and L.skp_tta_reduce_scored_workspace(1, 1, 1) == -1
