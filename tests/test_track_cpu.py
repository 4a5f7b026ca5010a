"""The keypoint tracker without a GPU: the numpy reference (tests/track_ref.py) against a brute-force
search over every path of a tiny grid and on the issue's synthetic sequence, what the C ABI rejects
before any launch, and ops.track_weights."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import track_ref as R


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("seed", range(20))
def test_reference_path_is_a_brute_force_optimum(seed):
    """T = 4, S = 4, r = 1, w = (1, 0.5), emissions powers of two in [2^-6, 1]: every product and every
    division is exact, so a path's value does not depend on the order it is multiplied in.  Among all
    16^4 paths the reference's has the optimal value, and it is the optimal path where that is unique."""
    T, S = 4, 4
    rng = np.random.default_rng(seed)
    frames = np.ldexp(np.float32(1.0), -rng.integers(0, 7, size=(T, 1, S, S))).astype(np.float32)
    w = np.array([1.0, 0.5], dtype=np.float32)
    states, pos = R.track(frames, w)
    path = tuple(int(y) * S + int(x) for y, x in np.floor(pos[:, 0]))
    best, optimal = R.brute_force(frames[:, 0], w)
    value = float(frames[0, 0].reshape(-1)[path[0]])
    for t in range(1, T):
        dy, dx = abs(path[t] // S - path[t - 1] // S), abs(path[t] % S - path[t - 1] % S)
        assert dy <= 1 and dx <= 1
        value *= float(w[dx]) * float(w[dy]) * float(frames[t, 0].reshape(-1)[path[t]])
    assert value == best
    assert path in optimal
    if len(optimal) == 1:
        assert path == optimal[0]


def test_brute_force_optimum_is_unique_for_some_seeds():
    """The uniqueness branch above is not vacuous."""
    w = np.array([1.0, 0.5], dtype=np.float32)
    unique = 0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        frames = np.ldexp(np.float32(1.0), -rng.integers(0, 7, size=(4, 1, 4, 4))).astype(np.float32)
        unique += len(R.brute_force(frames[:, 0], w)[1]) == 1
    assert 0 < unique < 20, unique


def test_synthetic_sequence_track_beats_per_frame_argmax():
    """S = 48, T = 12, the distractor in frames 3, 4 and 8, σ = 3, r = 8: the per-frame argmax is off by
    at least 20 pixels somewhere, the track stays within 2 pixels everywhere."""
    frames, truth = R.synthetic(48, 12, (3, 4, 8))
    states, pos = R.track(frames, R.weights(3.0, 8))
    independent = np.stack([np.array(divmod(int(R.first_max(f)[1][0]), 48)) for f in frames])
    tracked = np.floor(pos[:, 0]).astype(np.int64)
    d_ind = np.sqrt(((independent - truth) ** 2).sum(axis=1))
    d_trk = np.sqrt(((tracked - truth) ** 2).sum(axis=1))
    print("per-frame argmax worst", d_ind.max(), "track worst", d_trk.max())
    assert d_ind.max() >= 20
    assert d_trk.max() <= 2
    assert set(np.flatnonzero(d_ind > 2)) == {3, 4, 8}


def test_reference_restarts_after_a_blank_plane_and_keeps_ties_first():
    frames = np.ones((3, 1, 5, 5), dtype=np.float32)
    frames[1] = 0
    states, pos = R.track(frames, R.weights(1.0, 2))
    assert states[1][1][0] == 0 and states[1][2][0] == 0          # blank: max 0 at the first pixel
    assert np.array_equal(states[2][0], frames[2])                # m̃ ≡ 1, w[0] = 1: the score is the emission
    assert (states[2][3] == 2 * 5 + 2).all()                      # and staying put beats every step
    # flat weights on constant planes: every candidate ties, the smallest in-plane (dy, dx) wins
    states, pos = R.track(frames, np.ones(3, dtype=np.float32))
    back = states[2][3][0]
    for y in range(5):
        for x in range(5):
            assert back[y, x] == (max(-2, -y) + 2) * 5 + (max(-2, -x) + 2)
    assert np.array_equal(pos[:, 0], np.full((3, 2), 0.5, dtype=np.float32))


# ------------------------------------------------------------------------------------------ the C ABI
A = ctypes.c_void_p(256)
W = (ctypes.c_float * 4)(1.0, 0.8, 0.5, 0.1)
WP = ctypes.cast(W, ctypes.c_void_p)
#       avg prev pmax n  S   w   r  score smax best back ws stream
STEP = (A,  A,   A,   3, 37, WP, 3, A,    A,   A,   A,   A, None)
#       back best T  n  S   r  pos stream
BACK = (A,   A,   4, 3, 37, 3, A,  None)


def _library():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built")
    return _lib.lib()


def _rc(f, valid, **kw):
    args = list(valid)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return f(*args)


@pytest.mark.parametrize("slot", [0, 5, 7, 8, 9, 10, 11])
def test_step_rejects_null_pointers(slot):
    L = _library()
    assert _rc(L.skp_track_step, STEP, **{f"a{slot}": None}) == -1 and b"null" in L.skp_last_error()


@pytest.mark.parametrize("slot", [1, 2])
def test_step_rejects_half_of_the_frame0_pair(slot):
    L = _library()
    assert _rc(L.skp_track_step, STEP, **{f"a{slot}": None}) == -1 and b"null together" in L.skp_last_error()


def _weights(*v):
    arr = (ctypes.c_float * len(v))(*v)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


@pytest.mark.parametrize("kw,word", [
    (dict(a3=0), b"at least 1"), (dict(a3=-2), b"at least 1"), (dict(a4=0), b"at least 1"), (dict(a4=4097), b"4096"),
    (dict(a6=0), b"[1, 32]"), (dict(a6=33), b"[1, 32]"), (dict(a6=-1), b"[1, 32]"),
    (dict(a11=ctypes.c_void_p(260)), b"aligned"),
])
def test_step_rejects_bad_shapes_before_any_launch(kw, word):
    L = _library()
    assert _rc(L.skp_track_step, STEP, **kw) == -1 and word in L.skp_last_error(), L.skp_last_error()


@pytest.mark.parametrize("table", [(1.0, 0.5, 0.0, 0.1), (1.0, float("nan"), 0.5, 0.1), (1.0, 0.5, 0.2, float("inf")),
                                   (1.5, 0.5, 0.2, 0.1), (1.0, -0.5, 0.2, 0.1)])
def test_step_rejects_weights_outside_0_1(table):
    L = _library()
    keep, p = _weights(*table)
    assert _rc(L.skp_track_step, STEP, a5=p) == -1 and b"(0, 1]" in L.skp_last_error(), L.skp_last_error()


@pytest.mark.parametrize("slot", [0, 1, 6])
def test_backtrace_rejects_null_pointers(slot):
    L = _library()
    assert _rc(L.skp_track_backtrace, BACK, **{f"a{slot}": None}) == -1 and b"null" in L.skp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(a2=0), b"at least 1"), (dict(a3=0), b"at least 1"), (dict(a4=0), b"at least 1"), (dict(a4=4097), b"4096"),
    (dict(a5=0), b"[1, 32]"), (dict(a5=33), b"[1, 32]"),
])
def test_backtrace_rejects_bad_shapes_before_any_launch(kw, word):
    L = _library()
    assert _rc(L.skp_track_backtrace, BACK, **kw) == -1 and word in L.skp_last_error(), L.skp_last_error()


def test_workspace_query():
    L = _library()
    ws = L.skp_track_step_workspace
    assert ws(10, 128, 8) == 2 * 4 * 10 * 16 and ws(1, 1, 1) == 16 and ws(3, 37, 32) == 2 * 4 * 3 * 4
    assert ws(3, 33, 3) == 2 * 8 * ((4 * 3 * 4 + 7) // 8)
    for bad in ((0, 8, 3), (-1, 8, 3), (3, 0, 3), (3, 4097, 3), (3, 8, 0), (3, 8, 33), (65536, 8, 3)):
        assert ws(*bad) == -1, bad


# ------------------------------------------------------------------------------------------ ops and the CLI
def test_track_weights():
    from stablekeypoints_amd import ops
    for sigma, r in ((2.0, 6), (3.0, 9), (0.1, 1), (0.3, 1), (20.0, 32), (10.67, 32), (2.5, 8)):
        w = ops.track_weights(sigma)
        assert w.dtype == torch.float32 and not w.is_cuda and w.numel() == r + 1 == min(max(math.ceil(3 * sigma), 1), 32) + 1
        assert float(w[0]) == 1.0 and bool((w > 0).all()) and bool((w <= 1).all())
        assert np.array_equal(w.numpy(), R.weights(sigma, r))
    w = ops.track_weights(3.0, 8)
    assert w.numel() == 9 and np.array_equal(w.numpy(), R.weights(3.0, 8))
    assert bool((w[1:] < w[:-1]).all())
    for bad in (dict(sigma=0.0), dict(sigma=float("nan")), dict(sigma=-1.0), dict(sigma=2.0, radius=0),
                dict(sigma=2.0, radius=33), dict(sigma=0.5, radius=32)):
        with pytest.raises(ValueError, match="track_weights"):
            ops.track_weights(**bad)


def test_ops_check_their_arguments_before_the_device():
    from stablekeypoints_amd import ops
    w = ops.track_weights(1.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.track_step(torch.zeros(2, 4, 4), None, w)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.track_backtrace(torch.zeros(3, 2, 4, 4, dtype=torch.int16), torch.zeros(2, dtype=torch.int32), 3)
    assert ops.track_step_bytes(10, 128) == 14 * 10 * 128 * 128


def test_parser_has_the_track_flags():
    from stablekeypoints_amd.main import build_parser
    a = build_parser().parse_args(["--start_from_stage", "predict", "--track"])
    assert a.track and a.track_sigma == 2.0 and a.track_radius is None and a.track_size == 128
    a = build_parser().parse_args(["--track", "--track_sigma", "3", "--track_radius", "8", "--track_size", "64"])
    assert (a.track_sigma, a.track_radius, a.track_size) == (3.0, 8, 64)
    assert not build_parser().parse_args([]).track
