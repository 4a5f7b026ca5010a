"""ops.match_refine (skp_match_refine) against the numpy oracle of its definition,
tests/match_refine_ref.py: ``index`` equal, ``score`` bit for bit (−0.0 and +0.0 counted as equal).

Shapes (B, n, S, f, w): (2, 5, 24, 4, 5) with a random incoherent prior, every border clipped and n no
multiple of the 16-token panel; (1, 33, 32, 8, 8), two panels plus one token and a 64-pixel cell;
(2, 1, 20, 2, 1); (3, 7, 16, 1, 16), whose window is the plane, so the result is ops.match_field's; and
(1, 3, 40, 8, 16), a window wider than the cell grid's pitch, whose 40 × 40 region takes 25 passes.
Between them every kernel variant (f = 1, 2, 4, 8) runs, with one pass and with several.
"""
import numpy as np
import pytest
import torch

import match_field_ref as R
import match_refine_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ((2, 5, 24, 4, 5), (1, 33, 32, 8, 8), (2, 1, 20, 2, 1), (3, 7, 16, 1, 16), (1, 3, 40, 8, 16))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def signed(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def prior(seed, B, S, f):
    """A random incoherent prior: every cell points anywhere."""
    Sc = S // f
    return np.random.default_rng(seed).integers(0, Sc * Sc, (B, Sc, Sc)).astype(np.int32)


def run(x, y, coarse, w):
    from stablekeypoints_amd import ops
    i, s = ops.match_refine(torch.as_tensor(x, device=DEV), torch.as_tensor(y, device=DEV),
                            torch.as_tensor(coarse, device=DEV), w)
    torch.cuda.synchronize()
    assert i.dtype == torch.int32 and s.dtype == torch.float32
    return i.cpu().numpy(), s.cpu().numpy()


def check(x, y, coarse, w, what):
    """Device result against the oracle; returns the oracle's (index, score)."""
    gi, gs = run(x, y, coarse, w)
    ri, rs = W.match_refine(x, y, coarse, w)
    assert gi.shape == ri.shape and gs.shape == rs.shape, (what, gi.shape, ri.shape)
    bad = np.argwhere(gi != ri)
    assert not len(bad), (f"{what}: {len(bad)} indices differ, first at {bad[0].tolist()}: {gi[tuple(bad[0])]} vs the "
                          f"oracle's {ri[tuple(bad[0])]}")
    same = (gs.view(np.int32) == rs.view(np.int32)) | ((gs == 0) & (rs == 0))
    bad = np.argwhere(~same)
    assert not len(bad), (f"{what}: {len(bad)} scores differ in their bits, first at {bad[0].tolist()}: "
                          f"{gs[tuple(bad[0])]!r} vs the oracle's {rs[tuple(bad[0])]!r}")
    return ri, rs


@pytest.mark.parametrize("B,n,S,f,w", CASES, ids=lambda v: str(v))
def test_random_values_and_an_incoherent_prior(B, n, S, f, w):
    x, y = signed([1, B, n, S], B, n, S, S), signed([2, B, n, S], B, n, S, S)
    ri, _ = check(x, y, prior([3, S, f], B, S, f), w, f"B={B} n={n} S={S} f={f} w={w}")
    assert (ri >= 0).all()


def test_a_window_that_covers_the_plane_equals_match_field():
    from stablekeypoints_amd import ops
    B, n, S, f, w = CASES[3]
    x, y = signed(4, B, n, S, S), signed(5, B, n, S, S)
    y[0, :, 9, 2] = y[0, :, 1, 8]
    x[1, :, 3, 3] = 0
    gi, gs = run(x, y, prior(6, B, S, f), w)
    fi, fs = ops.match_field(torch.as_tensor(x, device=DEV).reshape(B, n, S * S),
                             torch.as_tensor(y, device=DEV).reshape(B, n, S * S))
    assert np.array_equal(gi.reshape(B, -1), fi.cpu().numpy())
    assert np.array_equal(gs.reshape(B, -1).view(np.int32), fs.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("B,n,S,f,w", CASES[:3], ids=lambda v: str(v))
def test_priors_outside_the_grid_give_no_match(B, n, S, f, w):
    """A prior of −1, of Sc², above it and far outside int16: −1 / −inf over the whole cell, nothing read."""
    Sc = S // f
    x, y, coarse = signed(7, B, n, S, S), signed(8, B, n, S, S), prior(9, B, S, f)
    coarse[0, 0, 0], coarse[0, 1, 2], coarse[0, 2, 1], coarse[-1, Sc - 1, Sc - 1] = -1, Sc * Sc, 2 ** 31 - 1, -2 ** 31
    ri, rs = check(x, y, coarse, w, "priors outside the grid")
    for b, cr, cc in ((0, 0, 0), (0, 1, 2), (0, 2, 1), (B - 1, Sc - 1, Sc - 1)):
        cell = (b, slice(cr * f, cr * f + f), slice(cc * f, cc * f + f))
        assert (ri[cell] == -1).all() and np.isneginf(rs[cell]).all(), (b, cr, cc)
    assert (ri >= 0).sum() == B * S * S - 4 * f * f


@pytest.mark.parametrize("corner", ["first", "last"])
@pytest.mark.parametrize("B,n,S,f,w", CASES[:3], ids=lambda v: str(v))
def test_a_constant_prior_every_cell_points_at_one_corner_cell(B, n, S, f, w, corner):
    Sc = S // f
    x, y = signed(10, B, n, S, S), signed(11, B, n, S, S)
    coarse = np.full((B, Sc, Sc), 0 if corner == "first" else Sc * Sc - 1, np.int32)
    ri, _ = check(x, y, coarse, w, f"constant prior, {corner} corner")
    lo, hi = (0, f - 1 + w) if corner == "first" else (S - f - w, S - 1)
    assert (ri // S >= lo).all() and (ri // S <= hi).all() and (ri % S >= lo).all() and (ri % S <= hi).all()


@pytest.mark.parametrize("B,n,S,f,w", CASES[:2], ids=lambda v: str(v))
def test_a_zero_column_and_a_nan_column_in_x(B, n, S, f, w):
    x, y = signed(12, B, n, S, S), signed(13, B, n, S, S)
    x[0, :, 5, 7] = 0
    x[0, n // 2, S - 1, 0] = np.nan
    x[-1, 0, 9, 9] = np.inf
    ri, rs = check(x, y, prior(14, B, S, f), w, "unusable columns of x")
    for b, r, c in ((0, 5, 7), (0, S - 1, 0), (B - 1, 9, 9)):
        assert ri[b, r, c] == -1 and np.isneginf(rs[b, r, c])
    assert (ri >= 0).sum() == B * S * S - 3


@pytest.mark.parametrize("B,n,S,f,w", CASES[:3], ids=lambda v: str(v))
def test_zero_nan_and_inf_columns_in_y_inside_windows(B, n, S, f, w):
    """The identity prior: the window of (r, c) is centred on (r, c), so every spoilt pixel of y lies
    in the windows around it; it is never the match, and the pixels around it still have one."""
    Sc = S // f
    x, y = signed(15, B, n, S, S), signed(16, B, n, S, S)
    coarse = np.broadcast_to(np.arange(Sc * Sc, dtype=np.int32).reshape(Sc, Sc), (B, Sc, Sc)).copy()
    spoilt = ((0, 0), (S // 2, S // 2 + 1), (S - 1, S - 1), (3, S - 2), (S // 2 + 1, 2))
    for j, (r, c) in enumerate(spoilt):
        if j % 3 == 0:
            y[:, :, r, c] = 0
        else:
            y[:, j % n, r, c] = np.nan if j % 3 == 1 else (np.inf if j % 2 else -np.inf)
    ri, _ = check(x, y, coarse, w, "unusable columns of y")
    assert (ri >= 0).all()
    assert not np.isin(ri, [r * S + c for r, c in spoilt]).any()


@pytest.mark.parametrize("fill", [0.0, np.nan, np.inf])
@pytest.mark.parametrize("B,n,S,f,w", CASES[:3], ids=lambda v: str(v))
def test_a_window_whose_every_pixel_is_unusable(B, n, S, f, w, fill):
    """Every cell of image 0 points at the first corner cell, whose whole region is spoilt; in the last
    image one cell does, and the rest go on matching."""
    Sc = S // f
    x, y, coarse = signed(17, B, n, S, S), signed(18, B, n, S, S), prior(19, B, S, f)
    coarse[0], coarse[-1, Sc - 1, 0] = 0, 0
    y[:, 0, :f + w, :f + w] = fill
    if fill == 0.0:
        y[:, :, :f + w, :f + w] = 0
    ri, rs = check(x, y, coarse, w, f"a window without a usable pixel ({fill})")
    assert (ri[0] == -1).all() and np.isneginf(rs[0]).all()
    assert (ri[-1, S - f:, :f] == -1).all() and np.isneginf(rs[-1, S - f:, :f]).all()


@pytest.mark.parametrize("B,n,S,f,w", CASES[:2] + CASES[4:], ids=lambda v: str(v))
def test_duplicate_y_columns_inside_a_window_the_lowest_wins(B, n, S, f, w):
    """Pairs of equal y columns one row apart, one column apart and w apart, all inside the windows of
    the x pixels that are multiples of them; with n >= 3 nothing else ties them."""
    Sc = S // f
    x, y = signed(20, B, n, S, S), signed(21, B, n, S, S)
    coarse = np.broadcast_to(np.arange(Sc * Sc, dtype=np.int32).reshape(Sc, Sc), (B, Sc, Sc)).copy()
    c0 = S // 2
    pairs = (((c0, c0), (c0 + 1, c0 - 1)), ((2, 3), (2, 4)), ((S - 2, 1), (S - 2, 1 + w)))
    for j, ((r1, c1), (r2, c2)) in enumerate(pairs):
        y[:, :, r2, c2] = y[:, :, r1, c1]
        x[:, :, r1, c1] = y[:, :, r1, c1] * (2.0 ** (j - 1))
    ri, _ = check(x, y, coarse, w, "duplicate columns")
    if n >= 3:
        assert [int(ri[0, r1, c1]) for (r1, c1), _ in pairs] == [r1 * S + c1 for (r1, c1), _ in pairs]


@pytest.mark.parametrize("shared", ["x", "y"])
def test_shared_operands(shared):
    """B = 3 with x given once (a leading 1), and with y given once."""
    n, S, f, w = 5, 24, 4, 5
    x, y = signed(22, 1 if shared == "x" else 3, n, S, S), signed(23, 1 if shared == "y" else 3, n, S, S)
    coarse = prior(24, 3, S, f)
    ri, _ = check(x, y, coarse, w, f"B=3 shared={shared}")
    assert not np.array_equal(ri[0], ri[1])


@pytest.mark.parametrize("B,n,S,f,w", CASES[:2], ids=lambda v: str(v))
def test_magnitudes_that_show_a_reordered_sum(B, n, S, f, w):
    """Values of 1e-20 and 1e18 mixed, both signs: a chain in another order, or split, rounds differently."""
    rng = np.random.default_rng(25)
    def mixed(*shape):
        v = rng.standard_normal(shape) * np.where(rng.random(shape) < 0.5, 1e-20, 1e18)
        return v.astype(np.float32)
    x, y = mixed(B, n, S, S), mixed(B, n, S, S)
    check(x, y, prior(26, B, S, f), w, "mixed magnitudes")
    check(x * np.float32(1e-18), y, prior(27, B, S, f), w, "mixed magnitudes, x scaled down")


def test_an_image_alone_and_at_either_place_in_a_batch_and_two_runs():
    n, S, f, w = 5, 24, 4, 5
    x, y, coarse = signed(28, 2, n, S, S), signed(29, 2, n, S, S), prior(30, 2, S, f)
    gi, gs = run(x, y, coarse, w)
    again = run(x, y, coarse, w)
    assert np.array_equal(gi, again[0]) and np.array_equal(gs.view(np.int32), again[1].view(np.int32))
    flip = run(x[::-1].copy(), y[::-1].copy(), coarse[::-1].copy(), w)
    for b in range(2):
        ai, a_s = run(x[b:b + 1], y[b:b + 1], coarse[b:b + 1], w)
        assert np.array_equal(ai[0], gi[b]) and np.array_equal(a_s[0].view(np.int32), gs[b].view(np.int32)), b
        assert np.array_equal(flip[0][1 - b], gi[b]) and np.array_equal(flip[1][1 - b].view(np.int32), gs[b].view(np.int32)), b


def test_argument_errors_name_the_argument():
    from stablekeypoints_amd import ops
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    c = torch.zeros(1, 2, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="x must be"):
        ops.match_refine(x[0], x, c, 3)
    with pytest.raises(ValueError, match="y must be float32"):
        ops.match_refine(x, x.double(), c, 3)
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.match_refine(torch.zeros(1, 3, 8, 16, device=DEV)[..., ::2], x, c, 3)
    with pytest.raises(ValueError, match="y is 4 tokens"):
        ops.match_refine(x, torch.zeros(1, 4, 8, 8, device=DEV), c, 3)
    with pytest.raises(ValueError, match="coarse must be"):
        ops.match_refine(x, x, c.long(), 3)
    with pytest.raises(ValueError, match="x has 2 images"):
        ops.match_refine(torch.zeros(2, 3, 8, 8, device=DEV), x, torch.zeros(3, 2, 2, dtype=torch.int32, device=DEV), 3)
    with pytest.raises(ValueError, match="must divide S"):
        ops.match_refine(x, x, torch.zeros(1, 3, 3, dtype=torch.int32, device=DEV), 3)
    with pytest.raises(ValueError, match="radius must be"):
        ops.match_refine(x, x, c, 17)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.match_refine(x.cpu(), x, c, 3)
