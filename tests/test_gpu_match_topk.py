"""ops.match_topk (skp_match_topk) against the numpy oracle of its definition, tests/propagate_ref.py:
``index`` equal, ``score`` bit for bit (−0.0 and +0.0 counted as equal), in every slot.

Shapes (B, n, S, w, K): (2, 5, 24, 3, 5), every border clipped, n no multiple of the 8-token panel, S a
multiple of the 4-pixel tile; (1, 33, 20, 8, 16), whole panels plus one token and K at its cap;
(3, 7, 16, 16, 4), whose window is the plane; (1, 1, 9, 1, 9), partial tiles on two sides and K the
full window's size, so border pixels leave −1 slots; (2, 3, 40, 12, 1), two passes of the region,
which must equal ops.match_refine with the identity prior.  Beside these (1, 4, 36, 16, 16): the
36 × 36 region takes three passes of 512 pixels, so lists at K's cap are merged across passes.
"""
import functools

import numpy as np
import pytest
import torch

import propagate_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ((2, 5, 24, 3, 5), (1, 33, 20, 8, 16), (3, 7, 16, 16, 4), (1, 1, 9, 1, 9), (2, 3, 40, 12, 1))
MORE = ((1, 4, 36, 16, 16),)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def signed(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def run(x, y, w, K):
    from stablekeypoints_amd import ops
    i, s = ops.match_topk(torch.as_tensor(x, device=DEV), torch.as_tensor(y, device=DEV), w, K)
    torch.cuda.synchronize()
    assert i.dtype == torch.int32 and s.dtype == torch.float32
    return i.cpu().numpy(), s.cpu().numpy()


def same_bits(a, b):
    return (a.view(np.int32) == b.view(np.int32)) | ((a == 0) & (b == 0))


def check(x, y, w, K, what):
    """Device result against the oracle; returns the oracle's (index, score)."""
    gi, gs = run(x, y, w, K)
    ri, rs = P.match_topk(x, y, w, K)
    assert gi.shape == ri.shape and gs.shape == rs.shape, (what, gi.shape, ri.shape)
    bad = np.argwhere(gi != ri)
    assert not len(bad), (f"{what}: {len(bad)} indices differ, first at {bad[0].tolist()}: {gi[tuple(bad[0])]} vs the "
                          f"oracle's {ri[tuple(bad[0])]}")
    bad = np.argwhere(~same_bits(gs, rs))
    assert not len(bad), (f"{what}: {len(bad)} scores differ in their bits, first at {bad[0].tolist()}: "
                          f"{gs[tuple(bad[0])]!r} vs the oracle's {rs[tuple(bad[0])]!r}")
    return ri, rs


@functools.lru_cache(maxsize=None)
def random_case(B, n, S):
    return signed([1, B, n, S], B, n, S, S), signed([2, B, n, S], B, n, S, S)


@pytest.mark.parametrize("B,n,S,w,K", CASES + MORE, ids=lambda v: str(v))
def test_random_values(B, n, S, w, K):
    x, y = random_case(B, n, S)
    ri, rs = check(x, y, w, K, f"B={B} n={n} S={S} w={w} K={K}")
    r, c = np.mgrid[0:S, 0:S]
    size = (np.minimum(r + w, S - 1) - np.maximum(r - w, 0) + 1) * (np.minimum(c + w, S - 1) - np.maximum(c - w, 0) + 1)
    assert np.array_equal((ri >= 0).sum(axis=1), np.broadcast_to(np.minimum(size, K), (B, S, S)))
    if (B, n, S, w, K) == CASES[3]:
        assert ri[0, 8, 0, 0] == -1 and ri[0, 3, 0, 0] >= 0 and ri[0, 4, 0, 0] == -1 and (ri[0, :, 4, 4] >= 0).all()


@pytest.mark.parametrize("B,n,S,w,K", CASES + MORE, ids=lambda v: str(v))
def test_slot_0_is_match_refine_with_the_identity_prior_and_shorter_lists_are_prefixes(B, n, S, w, K):
    from stablekeypoints_amd import ops
    x, y = random_case(B, n, S)
    x, y = x.copy(), y.copy()
    x[0, :, 1, 2] = 0
    y[-1, 0, S // 2, S // 2] = np.nan
    gi, gs = run(x, y, w, K)
    prior = torch.arange(S * S, dtype=torch.int32, device=DEV).reshape(1, S, S).repeat(B, 1, 1).contiguous()
    fi, fs = ops.match_refine(torch.as_tensor(x, device=DEV), torch.as_tensor(y, device=DEV), prior, w)
    assert np.array_equal(gi[:, 0], fi.cpu().numpy())
    assert np.array_equal(gs[:, 0].view(np.int32), fs.cpu().numpy().view(np.int32))
    assert gi[0, 0, 1, 2] == -1
    for k in sorted({1, (K + 1) // 2}):
        si, ss = run(x, y, w, k)
        assert np.array_equal(si, gi[:, :k]) and np.array_equal(ss.view(np.int32), gs[:, :k].view(np.int32)), k


@pytest.mark.parametrize("B,n,S,w,K", CASES[:2] + CASES[3:4], ids=lambda v: str(v))
def test_unusable_columns_of_x_and_of_y(B, n, S, w, K):
    x, y = signed(12, B, n, S, S), signed(13, B, n, S, S)
    x[0, :, 5, 7] = 0
    x[0, n // 2, S - 1, 0] = np.nan
    x[-1, 0, 3, 3] = np.inf
    spoilt = ((0, 0), (S // 2, S // 2 + 1), (S - 1, S - 1), (3, S - 2), (S // 2 + 1, 2))
    for j, (r, c) in enumerate(spoilt):
        if j % 3 == 0:
            y[:, :, r, c] = 0
        else:
            y[:, j % n, r, c] = np.nan if j % 3 == 1 else (np.inf if j % 2 else -np.inf)
    ri, rs = check(x, y, w, K, "unusable columns")
    for b, r, c in ((0, 5, 7), (0, S - 1, 0), (B - 1, 3, 3)):
        assert (ri[b, :, r, c] == -1).all() and np.isneginf(rs[b, :, r, c]).all()
    assert not np.isin(ri, [r * S + c for r, c in spoilt]).any()


@pytest.mark.parametrize("fill", [0.0, np.nan])
@pytest.mark.parametrize("B,n,S,w,K", CASES[:2] + CASES[3:4], ids=lambda v: str(v))
def test_a_window_without_a_usable_pixel(B, n, S, w, K, fill):
    """The windows of the first corner pixel, [0, w]², and (w = 1) of its neighbours hold nothing usable."""
    x, y = signed(17, B, n, S, S), signed(18, B, n, S, S)
    y[:, 0, :w + 2, :w + 2] = fill
    if fill == 0.0:
        y[:, :, :w + 2, :w + 2] = 0
    ri, rs = check(x, y, w, K, f"a window without a usable pixel ({fill})")
    assert (ri[:, :, :2, :2] == -1).all() and np.isneginf(rs[:, :, :2, :2]).all()
    assert (ri[:, 0, 2:, 2:] >= 0).all()


@pytest.mark.parametrize("B,n,S,w,K", CASES[:2] + CASES[4:] + MORE, ids=lambda v: str(v))
def test_duplicate_y_columns_inside_a_window_the_lower_q_comes_first(B, n, S, w, K):
    x, y = signed(20, B, n, S, S), signed(21, B, n, S, S)
    c0 = S // 2
    pairs = (((c0, c0), (c0 + 1, c0 - 1)), ((2, 3), (2, 4)), ((S - 2, 1), (S - 2, 1 + w)))
    for j, ((r1, c1), (r2, c2)) in enumerate(pairs):
        y[:, :, r2, c2] = y[:, :, r1, c1]
        x[:, :, r1, c1] = y[:, :, r1, c1] * (2.0 ** (j - 1))
    ri, rs = check(x, y, w, K, "duplicate columns")
    if n >= 3:
        assert [int(ri[0, 0, r1, c1]) for (r1, c1), _ in pairs] == [r1 * S + c1 for (r1, c1), _ in pairs]
        if K >= 2:
            assert [int(ri[0, 1, r1, c1]) for (r1, c1), _ in pairs] == [r2 * S + c2 for _, (r2, c2) in pairs]
            assert all(rs[0, 0, r1, c1] == rs[0, 1, r1, c1] for (r1, c1), _ in pairs)


def test_a_shared_x_against_three_context_frames():
    n, S, w, K = 5, 24, 3, 5
    x, y = signed(22, 1, n, S, S), signed(23, 3, n, S, S)
    ri, _ = check(x, y, w, K, "B=3, x shared")
    assert not np.array_equal(ri[0], ri[1])
    ri, _ = check(y, x, w, K, "B=3, y shared")
    assert not np.array_equal(ri[0], ri[1])


@pytest.mark.parametrize("B,n,S,w,K", CASES[:2], ids=lambda v: str(v))
def test_magnitudes_that_show_a_reordered_sum(B, n, S, w, K):
    """Values of 1e-20 and 1e18 mixed, both signs: a chain in another order, or split, rounds differently."""
    rng = np.random.default_rng(25)

    def mixed(*shape):
        v = rng.standard_normal(shape) * np.where(rng.random(shape) < 0.5, 1e-20, 1e18)
        return v.astype(np.float32)
    x, y = mixed(B, n, S, S), mixed(B, n, S, S)
    check(x, y, w, K, "mixed magnitudes")
    check(x * np.float32(1e-18), y, w, K, "mixed magnitudes, x scaled down")


def test_an_image_alone_and_at_either_place_in_a_batch_and_two_runs():
    n, S, w, K = 5, 24, 3, 5
    x, y = signed(28, 2, n, S, S), signed(29, 2, n, S, S)
    gi, gs = run(x, y, w, K)
    again = run(x, y, w, K)
    assert np.array_equal(gi, again[0]) and np.array_equal(gs.view(np.int32), again[1].view(np.int32))
    flip = run(x[::-1].copy(), y[::-1].copy(), w, K)
    for b in range(2):
        ai, a_s = run(x[b:b + 1], y[b:b + 1], w, K)
        assert np.array_equal(ai[0], gi[b]) and np.array_equal(a_s[0].view(np.int32), gs[b].view(np.int32)), b
        assert np.array_equal(flip[0][1 - b], gi[b]) and np.array_equal(flip[1][1 - b].view(np.int32), gs[b].view(np.int32)), b


def test_argument_errors_name_the_argument():
    from stablekeypoints_amd import ops
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="x must be"):
        ops.match_topk(x[0], x, 3, 5)
    with pytest.raises(ValueError, match="y must be float32"):
        ops.match_topk(x, x.double(), 3, 5)
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.match_topk(torch.zeros(1, 3, 8, 16, device=DEV)[..., ::2], x, 3, 5)
    with pytest.raises(ValueError, match="y is 4 tokens"):
        ops.match_topk(x, torch.zeros(1, 4, 8, 8, device=DEV), 3, 5)
    with pytest.raises(ValueError, match="x has 2 images"):
        ops.match_topk(torch.zeros(2, 3, 8, 8, device=DEV), torch.zeros(3, 3, 8, 8, device=DEV), 3, 5)
    with pytest.raises(ValueError, match="radius must be"):
        ops.match_topk(x, x, 17, 5)
    with pytest.raises(ValueError, match="k must be"):
        ops.match_topk(x, x, 3, 17)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.match_topk(x.cpu(), x, 3, 5)
