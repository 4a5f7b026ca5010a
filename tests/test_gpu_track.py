"""ops.track_step / ops.track_backtrace and eval.track_keypoints on the device against the numpy
restatement of the definition (tests/track_ref.py), bit for bit: score, score_max, best and back of
every frame and pos of the backtrace, over whole sequences.

The shapes (T, n, S, r) are the smallest at which the kernel can go wrong: a window wider than the
plane, an odd side with ragged 32 × 32 tiles, the largest radius with halos that span tiles, the
smallest radius; then, uniform random alone, each radius at which the LDS footprint changes (8 | 9,
16 | 17), the largest, and S = 100: 4 × 4 tiles, of which the inner ones take the path that tests no
candidate against the plane's border, along x, along y and along both.  In the first four, token 0 carries besides uniform random planes a plane
with one non-zero pixel in the last corner, then an all-zero plane in mid-sequence (the restart rule),
then a constant plane (ties everywhere: the tie rule decides every back-pointer)."""
import numpy as np
import pytest
import torch

import track_ref as R
from tta_tiny import DEV, same_bits

pytestmark = pytest.mark.gpu

SPECIAL = ((4, 3, 5, 8), (3, 2, 37, 3), (3, 1, 70, 32), (5, 2, 64, 1))
RANDOM = ((2, 2, 45, 9), (2, 1, 45, 16), (2, 1, 45, 17), (2, 2, 70, 32), (2, 1, 100, 3), (2, 1, 100, 17))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _frames(T, n, S, special):
    rng = np.random.default_rng(1000 * S + 10 * T + n)
    f = rng.random((T, n, S, S), dtype=np.float32)
    if special:
        mid = T // 2
        f[mid - 1, 0] = 0
        f[mid - 1, 0, S - 1, S - 1] = 0.75
        f[mid, 0] = 0
        f[mid + 1, 0] = 0.375
    return f


_CACHE = {}


def _case(shape):
    """(frames, weights (numpy), the reference's per-frame states and pos), computed once per shape."""
    if shape not in _CACHE:
        T, n, S, r = shape
        f = _frames(T, n, S, shape in SPECIAL)
        w = R.weights(r / 2.5, r)
        states, pos = R.track(f, w)
        for a in (f, pos, *[x for s in states for x in s]):
            a.setflags(write=False)
        _CACHE[shape] = (f, w, states, pos)
    return _CACHE[shape]


def _run(frames, w):
    """The device's states and pos for ``frames`` (numpy (T, n, S, S))."""
    from stablekeypoints_amd import ops
    wt = torch.from_numpy(np.array(w))
    states, state = [], None
    for a in frames:
        state = ops.track_step(torch.from_numpy(np.array(a)).to(DEV), state, wt)
        states.append(state)
    stack = torch.stack([s[3] for s in states])
    return states, ops.track_backtrace(stack, states[-1][2], len(w) - 1)


@pytest.mark.parametrize("shape", SPECIAL + RANDOM, ids=lambda s: "T%d-n%d-S%d-r%d" % s)
def test_sequence_equals_the_reference_bit_for_bit(shape):
    from stablekeypoints_amd import ops
    T, n, S, r = shape
    f, w, want, want_pos = _case(shape)
    assert np.array_equal(ops.track_weights(r / 2.5, r).numpy(), w)
    got, pos = _run(f, w)
    side = 2 * r + 1
    for t in range(T):
        for k, name in enumerate(("score", "score_max", "best", "back")):
            assert same_bits(got[t][k], want[t][k]), f"frame {t}: {name}"
        back = got[t][3].cpu().numpy().astype(np.int64)
        y, x = np.mgrid[0:S, 0:S]
        assert (back >= 0).all() and (back < side * side).all()
        assert ((y + back // side - r >= 0) & (y + back // side - r < S)).all(), f"frame {t}: a back-pointer leaves the plane"
        assert ((x + back % side - r >= 0) & (x + back % side - r < S)).all(), f"frame {t}: a back-pointer leaves the plane"
    assert same_bits(pos, want_pos)
    if shape in SPECIAL:
        mid = T // 2
        assert float(want[mid][1][0]) == 0.0 and int(want[mid][2][0]) == 0          # the blank plane
        assert np.array_equal(want[mid + 1][0][0], f[mid + 1, 0])                   # the restart: m̃ ≡ 1, w[0] = 1
        assert (want[mid + 1][3][0] == r * side + r).all()                          # and w[0] beats every other step
        # the corner plane's successor: 0 · w ties everywhere out of the corner's reach, the smallest offsets win
        if S - 1 > 2 * r:
            assert want[mid][3][0][0, 0] == r * side + r and want[mid][3][0][r, r] == 0


def test_flat_weights_ties_take_the_smallest_offsets():
    """Constant planes under w ≡ 1: every candidate ties, so every back-pointer is the tie rule's."""
    T, n, S, r = 2, 1, 37, 3
    f = np.full((T, n, S, S), 0.625, dtype=np.float32)
    w = np.ones(r + 1, dtype=np.float32)
    want, want_pos = R.track(f, w)
    got, pos = _run(f, w)
    for t in range(T):
        for k in range(4):
            assert same_bits(got[t][k], want[t][k]), (t, k)
    assert same_bits(pos, want_pos)
    y, x = np.mgrid[0:S, 0:S]
    assert np.array_equal(want[1][3][0], (np.maximum(-r, -y) + r) * (2 * r + 1) + np.maximum(-r, -x) + r)


@pytest.mark.parametrize("shape", [(3, 2, 37, 3), (4, 3, 5, 8), (2, 2, 70, 32)], ids=lambda s: "T%d-n%d-S%d-r%d" % s)
def test_a_token_does_not_depend_on_the_batch(shape):
    T, n, S, r = shape
    f, w, _, _ = _case(shape)
    whole, pos = _run(f, w)
    for j in range(n):
        alone, pos_j = _run(f[:, j:j + 1], w)
        for t in range(T):
            for k in range(4):
                assert same_bits(alone[t][k], whole[t][k][j:j + 1].cpu().numpy()), (j, t, k)
        assert same_bits(pos_j, pos[:, j:j + 1].contiguous().cpu().numpy())


def test_back_may_be_a_slice_of_the_callers_stack():
    from stablekeypoints_amd import ops
    f, w, want, _ = _case((3, 2, 37, 3))
    wt = torch.from_numpy(np.array(w))
    stack = torch.full((3, 2, 37, 37), -7, device=DEV, dtype=torch.int16)
    state = None
    for t in range(3):
        state = ops.track_step(torch.from_numpy(np.array(f[t])).to(DEV), state, wt, back=stack[t])
        assert state[3].data_ptr() == stack[t].data_ptr()
    assert same_bits(stack, np.stack([s[3] for s in want]))


def _want_tracks(frames, sigma, r):
    """KeypointTracks of the reference, as numpy."""
    T, n, S, _ = frames.shape
    states, pos = R.track(frames, R.weights(sigma, r))
    px = np.floor(pos).astype(np.int64)
    flat = frames.reshape(T, n, S * S)
    at = np.take_along_axis(flat, (px[..., 0] * S + px[..., 1])[..., None], axis=2)[..., 0]
    own = flat.argmax(axis=2)
    peak = np.take_along_axis(flat, own[..., None], axis=2)[..., 0]
    live = (peak != 0) & np.isfinite(peak)
    support = np.where(live, at / np.where(live, peak, np.float32(1)), np.float32(0)).astype(np.float32)
    independent = (np.stack([own // S, own % S], axis=-1).astype(np.float32) + np.float32(0.5)) / np.float32(S)
    return (pos / np.float32(S)).astype(np.float32), support, independent.astype(np.float32)


def test_track_keypoints_synthetic_from_a_device_tensor_and_from_cpu_frames():
    from stablekeypoints_amd import eval as ev
    frames, truth = R.synthetic(48, 12, (3, 4, 8))
    want = _want_tracks(frames, 3.0, 8)
    on_device = ev.track_keypoints(torch.from_numpy(frames).to(DEV), sigma=3.0, radius=8)
    from_list = ev.track_keypoints([torch.from_numpy(a) for a in frames], sigma=3.0, radius=8, device=DEV)
    from_generator = ev.track_keypoints((torch.from_numpy(a) for a in frames), sigma=3.0, radius=8, device=DEV)
    assert isinstance(on_device, ev.KeypointTracks)
    for got in (on_device, from_list, from_generator):
        assert [tuple(t.shape) for t in got] == [(12, 1, 2), (12, 1), (12, 1, 2)]
        for g, w_, name in zip(got, want, got._fields):
            assert g.device == torch.device(DEV) and same_bits(g, w_), name
    pos = on_device.pos.cpu().numpy()[:, 0] * 48 - 0.5
    assert np.sqrt(((pos - truth) ** 2).sum(axis=1)).max() <= 2
    ind = on_device.independent.cpu().numpy()[:, 0] * 48 - 0.5
    assert np.sqrt(((ind - truth) ** 2).sum(axis=1)).max() >= 20
    sup = on_device.support.cpu().numpy()[:, 0]
    # the distractor is 1.5 times the blob: 2/3 where it flashes, else the blob's own peak or a pixel beside it
    assert (sup[[3, 4, 8]] < 0.7).all() and (np.delete(sup, [3, 4, 8]) > 0.85).all()


def test_track_keypoints_blank_plane_has_no_support_and_default_radius():
    from stablekeypoints_amd import eval as ev
    f = _frames(5, 2, 64, True)                       # token 0: corner, blank, constant in frames 1, 2, 3
    want = _want_tracks(f, 2.0, 6)                    # the default radius: ceil(3 · 2)
    got = ev.track_keypoints(torch.from_numpy(f).to(DEV))
    for g, w_, name in zip(got, want, got._fields):
        assert same_bits(g, w_), name
    assert float(got.support[2, 0]) == 0.0 and float(got.support[3, 0]) == 1.0
    with pytest.raises(ValueError, match="at least one frame"):
        ev.track_keypoints([])
    with pytest.raises(ValueError, match="frame 1 is"):
        ev.track_keypoints([torch.zeros(2, 8, 8), torch.zeros(2, 9, 9)], device=DEV)
