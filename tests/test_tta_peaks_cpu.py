"""CPU-side checks of the k-peak TTA reduce (no GPU needed): the numpy restatement
tests/tta_peaks_ref.py against the numpy oracle, the planted cases through the float64 average, the
parser and CLI, and the argument checks of skp_tta_reduce_peaks through the C ABI."""
import inspect

import numpy as np
import pytest
import torch

import tta_abi
import tta_peaks_ref
import tta_ref

SMALL = [c for c in tta_peaks_ref.CASES if c[1][3] <= 96]


def _avg32(kind, shape):
    """The float64 average of tta_ref.tta_ref cast to float32, one (T, S, S) stack."""
    maps, theta, plan = tta_peaks_ref.make(kind, shape)
    B, C, n, S = shape
    _, avg, _ = tta_ref.tta_ref(maps, theta)
    return avg.astype(np.float32).reshape(B * n, S, S), plan


@pytest.mark.parametrize("kind,shape", SMALL, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_peaks_ref_is_the_oracle(kind, shape):
    """Positions against oracle find_k_max_pixels, values against the oracle's find_max_pixel /
    mask_radius chain; the token with a +inf pixel gives NaN from round 1 on (equal_nan)."""
    from oracle import skp_oracle as O
    S, num = shape[3], 4
    avg, _ = _avg32(kind, shape)
    pos, val = tta_peaks_ref.peaks_ref(avg, num, 0.05 * S)
    assert pos.dtype == np.float32 and val.dtype == np.float32
    assert np.array_equal(pos.transpose(1, 0, 2), O.find_k_max_pixels(avg, num))
    m, saw_nan = avg, False
    for j in range(num):
        p = O.find_max_pixel(m)
        assert np.array_equal(pos[:, j], p)
        want = m[np.arange(len(m)), (p[:, 0] - 0.5).astype(int), (p[:, 1] - 0.5).astype(int)]
        assert np.array_equal(val[:, j], want, equal_nan=True)
        saw_nan |= bool(np.isnan(want).any())
        m = O.mask_radius(m, p, 0.05 * S)
    if kind == "quarters" and shape[2] > 2:   # the +inf pixel of make_case: inf · 0 = NaN wins the later rounds
        assert np.isinf(val[1, 0]) and np.isnan(val[1, 1:]).all() and (pos[1, 1:] == pos[1, 0]).all() and saw_nan


@pytest.mark.parametrize("shape", list(tta_peaks_ref.CONTINUOUS), ids=lambda s: "x".join(map(str, s)))
def test_planted_cases_behave_as_planned(shape):
    """Under the float64 average cast to float32: the picks are bump 1, then bump 2; the third
    round lands in neither masked disc (so not on the bump planted inside the first); every round
    j >= 1 with a positive value is farther than the radius from all earlier picks."""
    S, num = shape[3], 4
    radius = 0.05 * S
    avg, plan = _avg32("continuous", shape)
    pos, val = tta_peaks_ref.peaks_ref(avg, num, radius)
    for t, bumps in enumerate(plan):
        assert tuple(pos[t, 0]) == (bumps[0][0] + 0.5, bumps[0][1] + 0.5)
        assert tuple(pos[t, 1]) == (bumps[1][0] + 0.5, bumps[1][1] + 0.5)
        assert val[t, 0] >= bumps[0][2] / 2 - 1e-3 and bumps[1][2] / 2 - 1e-3 <= val[t, 1] < val[t, 0]
        for r, c, _ in bumps[2:]:     # inside the first disc, and the highest value left in round 1
            assert np.hypot(r - bumps[0][0], c - bumps[0][1]) < radius and avg[t, r, c] > 1.0
            assert not any(tuple(pos[t, j]) == (r + 0.5, c + 0.5) for j in range(num))
        for j in range(1, num):
            if val[t, j] > 0:     # measured as the mask does: pixel (row, col) to pick (row + 0.5, col + 0.5)
                d = np.hypot(*((pos[t, j] - 0.5)[None] - pos[t, :j]).T)
                assert (d > radius).all()
        assert val[t, 2] > 0 and val[t, 2] < 1.0     # round 2: the continuous background
    if shape[3] == 512:     # bump 1 within the radius of the right edge: its box is clipped there
        assert plan[0][0][1] + radius > S - 1
    else:                   # token 0's first disc crosses a four-row band and the 64-column tile boundary
        r, c, _ = plan[0][0]
        assert (r - radius < 0 < 4 < r + radius) and (c - radius < 64 <= c + radius) and c < 64


def test_ops_tta_reduce_peaks_refuses_cpu_tensors():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tta_reduce_peaks(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 2, 3), 2)


def test_tta_reduce_peaks_rejects_bad_arguments_without_gpu():
    """num, radius2 and the workspace query; the checks every reduce shares are in tests/test_tta_cpu.py."""
    L = tta_abi.library()
    r2 = tta_abi.R2
    for bad in (0, 17, -1):                                 # slot 6 of skp_tta_reduce_peaks
        assert tta_abi.rc_with(L, "skp_tta_reduce_peaks", a6=bad) == -1 and b"num" in L.skp_last_error()
    for bad in (0.0, float("nan"), -1.0, float("inf")):     # slot 7
        assert tta_abi.rc_with(L, "skp_tta_reduce_peaks", a7=bad) == -1 and b"radius2" in L.skp_last_error()
    # the workspace query: the partials of skp_tta_reduce and an index per image, token and round
    for B, n, S in ((1, 10, 512), (2, 5, 37), (1, 1, 2), (4, 10, 512)):
        for num in (1, 3, 16):
            assert L.skp_tta_reduce_peaks_workspace(B, n, S, num, r2) >= L.skp_tta_reduce_workspace(B, n, S) > 0
    assert L.skp_tta_reduce_peaks_workspace(1, 10, 512, 3, r2) == 10 * (8 * 128) * 8 + 10 * 3 * 4
    assert L.skp_tta_reduce_peaks_workspace(1, 1, 8, 1, r2) % 8 == 0
    for bad in ((0, 1, 8, 2, r2), (1, 0, 8, 2, r2), (1, 1, -3, 2, r2), (1, 1, 1, 2, r2), (1, 1, 8, 0, r2),
                (1, 1, 8, 17, r2), (1, 1, 8, 2, 0.0), (1, 1, 8, 2, float("nan"))):
        assert L.skp_tta_reduce_peaks_workspace(*bad) == -1


def test_cli_refuses_subjects_with_scores_before_the_model(monkeypatch, capsys):
    from stablekeypoints_amd import main as cli, optimize_token

    def no_model(*a, **k):
        raise AssertionError("the model was built")

    monkeypatch.setattr(optimize_token, "load_ldm", no_model)
    with pytest.raises(SystemExit) as e:
        cli.main(["--start_from_stage", "predict", "--num_subjects", "2", "--keypoint_scores", "--model_type", "tiny",
                  "--dataset_name", "synthetic"])
    assert e.value.code not in (0, None)
    err = capsys.readouterr().err
    assert "--num_subjects" in err and "--keypoint_scores" in err
    with pytest.raises(SystemExit):
        cli.main(["--start_from_stage", "predict", "--num_subjects", "0", "--model_type", "tiny"])
    args = cli.build_parser().parse_args(["--start_from_stage", "predict", "--num_subjects", "2"])
    assert args.num_subjects == 2 and args.keypoint_scores is False
    assert cli.build_parser().parse_args([]).num_subjects == 1


def test_predict_keypoints_signature_and_alias():
    import stablekeypoints_amd.eval as ev
    import unsupervised_keypoints.eval as alias
    assert alias.predict_keypoints is ev.predict_keypoints
    assert inspect.signature(alias.predict_keypoints).parameters["num_subjects"].default == 1
    assert ev.KeypointPeaks._fields == ("pos", "value")
