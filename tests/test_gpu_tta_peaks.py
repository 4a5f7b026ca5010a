"""skp_tta_reduce_peaks / ops.tta_reduce_peaks, eval.predict_keypoints(num_subjects=k) and the CLI's
predict stage with --num_subjects on the GPU.

The reference of every kernel check is the composition of the ops that existed before the k-peak
reduce: ops.tta_reduce with the average written, then ops.find_k_max_pixels on it (positions) and the
progressive ops.find_max_pixel / gather / ops.mask_radius chain (the value that won each round).
Everything is compared for equality; NaN values (a masked +inf) must sit in the same places.
"""
import csv

import numpy as np
import pytest
import torch

import tta_peaks_ref
import tta_ref
import tta_tiny
from tta_tiny import DEV, S_UP, cli as _cli, same_values as _same, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

NUMS = (1, 2, 3, 4)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _chain(avg, num, radius):
    """(T, S, S) -> the positions (T, num, 2) and winning values (T, num) of num rounds of
    find_max_pixel, each followed by mask_radius."""
    from stablekeypoints_amd import ops
    T, S, _ = avg.shape
    m, pos, val = avg, [], []
    for _ in range(num):
        p = ops.find_max_pixel(m)
        idx = ((p[:, 0] - 0.5) * S + (p[:, 1] - 0.5)).long()
        pos.append(p)
        val.append(m.reshape(T, S * S).gather(1, idx[:, None])[:, 0])
        m = ops.mask_radius(m, p, radius)
    return torch.stack(pos, dim=1), torch.stack(val, dim=1)


@pytest.fixture(scope="module", params=tta_peaks_ref.CASES, ids=lambda c: "{}_B{}_C{}_n{}_S{}".format(c[0], *c[1]))
def case(request):
    """One case's inputs, the outputs under test for every num and every reference, computed once."""
    from stablekeypoints_amd import ops
    kind, shape = request.param
    B, C, n, S = shape
    maps_np, theta_np, plan = tta_peaks_ref.make(kind, shape)
    maps, theta = torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV)
    plain_pos, plain_avg = ops.tta_reduce(maps, theta, return_avg=True)
    flat = plain_avg.reshape(B * n, S, S)
    got, got_noavg, kmax = {}, {}, {}
    for num in NUMS:
        got[num] = ops.tta_reduce_peaks(maps, theta, num, return_avg=True)
        got_noavg[num] = ops.tta_reduce_peaks(maps, theta, num)
        kmax[num] = ops.find_k_max_pixels(flat, num)
    chain_pos, chain_val = _chain(flat, max(NUMS), 0.05 * S)
    torch.cuda.synchronize()
    return dict(kind=kind, shape=shape, plan=plan, maps=maps, theta=theta, plain_pos=plain_pos, plain_avg=plain_avg,
                got=got, got_noavg=got_noavg, kmax=kmax, chain_pos=chain_pos, chain_val=chain_val)


def test_equals_the_composition(case):
    B, C, n, S = case["shape"]
    for num in NUMS:
        pos, values, avg = case["got"][num]
        assert pos.shape == (B, n, num, 2) and values.shape == (B, n, num) and avg.shape == (B, n, S, S)
        assert torch.equal(avg.view(torch.int32), case["plain_avg"].view(torch.int32))     # bit for bit
        kmax = case["kmax"][num]                                                            # (num, B·n, 2)
        for j in range(num):
            assert torch.equal(pos[:, :, j].reshape(B * n, 2), kmax[j]), (num, j)
        assert torch.equal(pos.reshape(B * n, num, 2), case["chain_pos"][:, :num])
        assert _same(values.reshape(B * n, num), case["chain_val"][:, :num]), num
    pos1, values1, _ = case["got"][1]
    assert torch.equal(pos1[:, :, 0], case["plain_pos"])
    assert torch.equal(values1[:, :, 0], case["plain_avg"].amax(dim=(2, 3)))


def test_equals_the_numpy_restatement(case):
    """The same outputs against tests/tta_peaks_ref.py on the average read back: a reference that
    shares no code with the ops above."""
    B, C, n, S = case["shape"]
    num = max(NUMS)
    ref_pos, ref_val = tta_peaks_ref.peaks_ref(case["plain_avg"].reshape(B * n, S, S).cpu().numpy(), num, 0.05 * S)
    pos, values, _ = case["got"][num]
    assert np.array_equal(pos.reshape(B * n, num, 2).cpu().numpy(), ref_pos)
    assert np.array_equal(values.reshape(B * n, num).cpu().numpy(), ref_val, equal_nan=True)
    if case["kind"] == "quarters" and n > 2:     # the +inf pixel: inf, then inf · 0 = NaN wins where it was
        assert torch.isinf(values[0, 1, 0]) and torch.isnan(values[0, 1, 1:]).all()
        assert (pos[0, 1, 1:] == pos[0, 1, 0]).all()
    if case["plan"] is not None:
        for t, bumps in enumerate(case["plan"]):
            assert tuple(pos[0, t, 0].tolist()) == (bumps[0][0] + 0.5, bumps[0][1] + 0.5)
            assert tuple(pos[0, t, 1].tolist()) == (bumps[1][0] + 0.5, bumps[1][1] + 0.5)


def test_pos_and_values_do_not_depend_on_return_avg(case):
    for num in NUMS:
        pos, values, _ = case["got"][num]
        pos2, values2, none = case["got_noavg"][num]
        assert none is None
        assert torch.equal(pos.view(torch.int32), pos2.view(torch.int32))
        assert torch.equal(values.view(torch.int32), values2.view(torch.int32))


def test_degenerate_tokens(case):
    B, C, n, S = case["shape"]
    if case["kind"] != "quarters":
        return
    pos, values, _ = case["got"][max(NUMS)]
    if case["shape"] == tta_ref.ALL_OUT_OF_VIEW:     # the last image: every copy out of view
        assert (pos[-1] == 0.5).all() and (values[-1] == 0).all()
    if n > 1 or B > 1:   # token 0 of image 0 is all zero in every copy
        assert (pos[0, 0] == 0.5).all() and (values[0, 0] == 0).all()


def test_workspace_reuse(case):
    """num = 4 and then num = 2 on the same shape: what the first num = 2 call of the module gave."""
    from stablekeypoints_amd import ops
    ops.tta_reduce_peaks(case["maps"], case["theta"], 4)
    pos, values, _ = ops.tta_reduce_peaks(case["maps"], case["theta"], 2)
    want_pos, want_values, _ = case["got"][2]
    assert torch.equal(pos.view(torch.int32), want_pos.view(torch.int32))
    assert torch.equal(values.view(torch.int32), want_values.view(torch.int32))


def test_explicit_radius(case):
    """radius = 0.05 · S is the default, and another radius follows the chain at that radius."""
    from stablekeypoints_amd import ops
    B, C, n, S = case["shape"]
    pos, values, _ = ops.tta_reduce_peaks(case["maps"], case["theta"], 3, radius=0.05 * S)
    assert torch.equal(pos, case["got"][3][0]) and _same(values, case["got"][3][1])
    radius = 0.11 * S
    pos, values, _ = ops.tta_reduce_peaks(case["maps"], case["theta"], 3, radius=radius)
    want_pos, want_val = _chain(case["plain_avg"].reshape(B * n, S, S), 3, radius)
    assert torch.equal(pos.reshape(B * n, 3, 2), want_pos) and _same(values.reshape(B * n, 3), want_val)


def test_tta_reduce_peaks_rejects_bad_arguments():
    from stablekeypoints_amd import ops
    m, th = torch.zeros(1, 2, 1, 8, 8, device=DEV), torch.zeros(1, 2, 2, 3, device=DEV)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="num"):
            ops.tta_reduce_peaks(m, th, bad)
    with pytest.raises(ValueError, match="theta_inv"):
        ops.tta_reduce_peaks(m, torch.zeros(1, 3, 2, 3, device=DEV), 2)
    with pytest.raises(ValueError, match="maps must be"):
        ops.tta_reduce_peaks(torch.zeros(1, 2, 1, 8, 4, device=DEV), th, 2)
    for bad in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            ops.tta_reduce_peaks(m, th, 2, radius=bad)


# ------------------------------------------------------------------------------------------ end to end
def _predict(tiny, **kw):
    return tta_tiny.predict(tiny, tiny[2], augmentation_iterations=3, **kw)


def test_predict_keypoints_subjects_tiny(tiny):
    from stablekeypoints_amd import eval as ev
    n, k = len(tiny[4]), 3
    W = torch.randn(2 * n, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    one = _predict(tiny, regressor=W, return_maps=True)
    assert len(one) == 3                                  # num_subjects = 1: today's outputs, nothing more
    one_explicit = _predict(tiny, regressor=W, return_maps=True, num_subjects=1)
    assert len(one_explicit) == 3 and all(torch.equal(a, b) for a, b in zip(one, one_explicit))
    kp1, reg1, maps1 = one
    kp, reg, maps, peaks = _predict(tiny, regressor=W, return_maps=True, num_subjects=k)
    assert isinstance(peaks, ev.KeypointPeaks)
    assert kp.shape == (2, n, 2) and peaks.pos.shape == (2, n, k, 2) and peaks.value.shape == (2, n, k)
    assert torch.equal(kp, kp1) and torch.equal(reg, reg1) and torch.equal(maps, maps1)
    assert torch.equal(peaks.pos[:, :, 0], kp)
    want = ev.find_k_max_pixels(maps.reshape(2 * n, S_UP, S_UP), num=k)     # (k, 2n, 2)
    assert torch.equal(peaks.pos, want.permute(1, 0, 2).reshape(2, n, k, 2) / S_UP)
    assert torch.equal(peaks.value[:, :, 0], maps.amax(dim=(2, 3)))
    assert (peaks.value[:, :, 1:] <= peaks.value[:, :, :-1]).all()
    # alone, and with weighted_avg: the peaks come last and are the same
    kp2, peaks2 = _predict(tiny, num_subjects=k)
    assert torch.equal(kp2, kp) and all(torch.equal(a, b) for a, b in zip(peaks2, peaks))
    wkp = _predict(tiny, max_loc_strategy="weighted_avg")
    wkp_k, wpeaks = _predict(tiny, max_loc_strategy="weighted_avg", num_subjects=k)
    assert torch.equal(wkp_k, wkp) and all(torch.equal(a, b) for a, b in zip(wpeaks, peaks))
    with pytest.raises(ValueError, match="return_scores"):
        _predict(tiny, num_subjects=k, return_scores=True)


def test_cli_num_subjects_tiny(tmp_path):
    names = ("subject_keypoints.pt", "subject_peak_values.pt", "subject_keypoints.csv")
    plain = _cli(tmp_path / "plain", "--num_subjects", "1")
    assert not any((tmp_path / "plain" / f).exists() for f in names)
    out = tmp_path / "two"
    kp = _cli(out, "--num_subjects", "2")
    assert torch.equal(kp, plain)
    assert open(out / "keypoints.csv").read() == open(tmp_path / "plain" / "keypoints.csv").read()
    pos = torch.load(out / "subject_keypoints.pt", weights_only=True)
    val = torch.load(out / "subject_peak_values.pt", weights_only=True)
    assert pos.shape == (5, 5, 2, 2) and val.shape == (5, 5, 2)
    assert pos.dtype == torch.float32 and val.dtype == torch.float32
    assert torch.equal(pos[:, :, 0], kp)
    assert torch.isfinite(val).all() and (val[..., 1] <= val[..., 0]).all()
    # a second peak with mass lies outside the first disc, measured as the mask does: from the
    # pixel's integer (row, col) to the first pick's (row + 0.5, col + 0.5)
    far = ((pos[:, :, 1] * 512 - 0.5) - pos[:, :, 0] * 512).norm(dim=-1) > 0.05 * 512
    assert (far | (val[..., 1] == 0)).all()
    rows = list(csv.reader(open(out / "subject_keypoints.csv")))
    assert len(rows) == 5 and [r[0] for r in rows] == [str(i) for i in range(5)] and len(rows[0]) == 1 + 5 * 2 * 3
    table = np.array(rows, dtype=np.float64)[:, 1:].astype(np.float32).reshape(5, 5, 2, 3)
    assert np.array_equal(table[..., :2], pos.numpy()) and np.array_equal(table[..., 2], val.numpy())
