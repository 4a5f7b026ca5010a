"""ops.match_field (skp_match_field) against the numpy oracle of its definition, tests/match_field_ref.py:
``index`` equal, ``score`` bit for bit (−0.0 and +0.0 counted as equal).

Shapes: n in {1, 2, 3, 29, 33} (odd n, one 32-token panel plus one token) with (P, Q) in {(1, 1),
(1, 1369), (1369, 1), (200, 1369), (1369, 1369)} (ragged last tiles; 1369 is odd, so the scalar
loader), two shapes whose P and Q are multiples of 4 (the float4 loader, the one S² takes) and one whose
splits of Q hold two tiles each.  Q = 1369 is 11 tiles of 128 and, on all these shapes but the last,
11 splits: "a tile apart" is "a split apart".
"""
import numpy as np
import pytest
import torch

import match_field_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS = (1, 2, 3, 29, 33)
PQ = ((1, 1), (1, 1369), (1369, 1), (200, 1369), (1369, 1369))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def signed(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def on_grid(seed, *shape):
    """Non-negative multiples of 1/256 below 1: every product and every sum of up to 64 of them is exact."""
    return (np.random.default_rng(seed).integers(0, 256, shape) / 256.0).astype(np.float32)


def run(x, y):
    from stablekeypoints_amd import ops
    i, s = ops.match_field(torch.as_tensor(x, device=DEV), torch.as_tensor(y, device=DEV))
    torch.cuda.synchronize()
    assert i.dtype == torch.int32 and s.dtype == torch.float32
    return i.cpu().numpy(), s.cpu().numpy()


def check(x, y, what):
    """Device result against the oracle; returns the oracle's (index, score)."""
    gi, gs = run(x, y)
    ri, rs = R.match_field(x, y)
    assert gi.shape == ri.shape and gs.shape == rs.shape, (what, gi.shape, ri.shape)
    bad = np.argwhere(gi != ri)
    assert not len(bad), (f"{what}: {len(bad)} indices differ, first at {bad[0].tolist()}: {gi[tuple(bad[0])]} vs the "
                          f"oracle's {ri[tuple(bad[0])]}")
    same = (gs.view(np.int32) == rs.view(np.int32)) | ((gs == 0) & (rs == 0))
    bad = np.argwhere(~same)
    assert not len(bad), (f"{what}: {len(bad)} scores differ in their bits, first at {bad[0].tolist()}: "
                          f"{gs[tuple(bad[0])]!r} vs the oracle's {rs[tuple(bad[0])]!r}")
    return ri, rs


@pytest.mark.parametrize("P,Q", PQ, ids=lambda v: str(v))
@pytest.mark.parametrize("n", NS)
def test_signed_normal_values(n, P, Q):
    check(signed([1, n, P, Q], 1, n, P), signed([2, n, P, Q], 1, n, Q), f"signed n={n} P={P} Q={Q}")


@pytest.mark.parametrize("n,P,Q", [(1, 1369, 1369), (3, 200, 1369), (33, 1369, 1), (33, 200, 1369), (29, 1369, 1369)])
def test_exact_sums_on_a_grid(n, P, Q):
    check(on_grid([3, n, P, Q], 1, n, P), on_grid([4, n, P, Q], 1, n, Q), f"grid n={n} P={P} Q={Q}")


@pytest.mark.parametrize("n,P,Q", [(33, 260, 1028), (7, 1028, 260)])
def test_float4_loader(n, P, Q):
    check(signed([5, n, P, Q], 1, n, P), signed([6, n, P, Q], 1, n, Q), f"float4 n={n} P={P} Q={Q}")


def test_two_tiles_per_split():
    """B · ⌈P / 128⌉ = 55 rows of workgroups: Q's 11 tiles go to 6 splits of two."""
    x, y = signed(7, 5, 2, 1369), signed(8, 5, 2, 1369)
    y[:, :, 1000] = y[:, :, 3]                  # tiles 7 and 0: splits 3 and 0
    y[:, :, 200] = y[:, :, 130]                 # both in tile 1
    y[:, :, 300] = y[:, :, 140]                 # tiles 2 and 1: splits 1 and 0
    x[:, :, 0], x[:, :, 1], x[:, :, 2] = y[:, :, 3] * 2, y[:, :, 130] * 0.5, y[:, :, 140]
    ri, _ = check(x, y, "two tiles per split")
    assert (ri[:, 0] == 3).all() and (ri[:, 1] == 130).all()   # in two dimensions another column may tie the third


def test_x_equals_y():
    """The index is the lowest duplicate and the score rounds 1."""
    x = signed(9, 1, 33, 1369)
    x[0, :, 700] = x[0, :, 5]
    x[0, :, 1368] = x[0, :, 140] * 4
    ri, rs = check(x, x, "x == y")
    want = np.arange(1369)
    want[700], want[1368] = 5, 140
    assert (ri[0] == want).all()
    assert np.abs(rs.astype(np.float64) - 1).max() <= 4 * 2.0 ** -24


def test_repeated_columns_the_lowest_wins():
    """Columns of y repeated more than one tile (= one split of Q) apart, and within one tile."""
    n, P, Q = 29, 200, 1369
    y = signed(10, 1, n, Q)
    pairs = ((40, 1300), (41, 41 + 3 * 128), (500, 501), (127, 128), (0, 1368))
    x = signed(11, 1, n, P)
    for j, (lo, hi) in enumerate(pairs):
        y[0, :, hi] = y[0, :, lo]
        x[0, :, 7 * j] = y[0, :, lo] * (2.0 ** (j - 2))
    ri, _ = check(x, y, "repeated columns")
    assert [int(ri[0, 7 * j]) for j in range(len(pairs))] == [lo for lo, _ in pairs]


def _spoil(a, seed):
    """Zero, NaN-holding and inf-holding columns, the first and the last among them."""
    cols = a.shape[-1]
    pick = np.unique(np.concatenate([[0, cols - 1], np.random.default_rng(seed).integers(0, cols, 24)]))
    for j, c in enumerate(pick):
        if j % 3 == 0:
            a[..., :, c] = 0
        else:
            a[..., j % a.shape[-2], c] = np.nan if j % 3 == 1 else (np.inf if j % 2 else -np.inf)
    return pick


@pytest.mark.parametrize("n,P,Q", [(1, 200, 1369), (33, 200, 1369), (3, 1369, 1369), (33, 1369, 1)])
def test_unusable_columns(n, P, Q):
    x, y = signed([12, n], 1, n, P), signed([13, n], 1, n, Q)
    px, py = _spoil(x, 14), _spoil(y, 15)
    ri, rs = check(x, y, f"unusable n={n} P={P} Q={Q}")
    assert (ri[0, px] == -1).all() and np.isneginf(rs[0, px]).all()
    if len(py) < Q:
        assert not np.isin(ri[0], py).any()
    else:
        assert (ri == -1).all()


@pytest.mark.parametrize("fill", [0.0, np.nan, np.inf])
def test_no_usable_column_in_y(fill):
    x, y = signed(16, 1, 3, 200), signed(17, 1, 3, 1369)
    y[0, 1, :] = fill
    if fill == 0.0:
        y[:] = 0
    ri, rs = check(x, y, f"y without a usable column ({fill})")
    assert (ri == -1).all() and np.isneginf(rs).all()


@pytest.mark.parametrize("shared", ["none", "x", "y"])
def test_batches_and_shared_operands(shared):
    """B = 3 with each operand per image or shared; an image alone gives what it gives in the batch,
    and a second run gives the same bits."""
    n, P, Q = 29, 200, 1369
    x, y = signed(18, 1 if shared == "x" else 3, n, P), signed(19, 1 if shared == "y" else 3, n, Q)
    ri, rs = check(x, y, f"B=3 shared={shared}")
    gi, gs = run(x, y)
    assert (gi == ri).all() and (gs.view(np.int32) == rs.view(np.int32)).all()
    for b in range(3):
        ai, a_s = run(x[min(b, len(x) - 1)][None], y[min(b, len(y) - 1)][None])
        assert (ai[0] == gi[b]).all() and (a_s[0].view(np.int32) == gs[b].view(np.int32)).all(), b


def test_argument_errors_name_the_argument():
    from stablekeypoints_amd import ops
    x, y = torch.zeros(1, 3, 8, device=DEV), torch.zeros(1, 3, 9, device=DEV)
    with pytest.raises(ValueError, match="x must be"):
        ops.match_field(x[0], y)
    with pytest.raises(ValueError, match="y must be float32"):
        ops.match_field(x, y.double())
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.match_field(x.transpose(1, 2).contiguous().transpose(1, 2), y)
    with pytest.raises(ValueError, match="y has 4 tokens"):
        ops.match_field(x, torch.zeros(1, 4, 9, device=DEV))
    with pytest.raises(ValueError, match="x has 2 images"):
        ops.match_field(torch.zeros(2, 3, 8, device=DEV), torch.zeros(3, 3, 9, device=DEV))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.match_field(x.cpu(), y)
