"""CPU-side checks of the dense match field: the oracle's emulated fmaf against exact rational
arithmetic, the oracle's rules on hand-made cases, the C ABI's argument checks (no device needed), the
label and point transfer of eval on CPU tensors, and the CLI's flags."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import match_field_ref as R

F32 = np.float32


def _round_f32(v):
    """The float32 nearest to the rational ``v`` (ties to even, subnormals included; no overflow here)."""
    if v == 0:
        return F32(0)
    sign, v = (-1.0 if v < 0 else 1.0), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    e = e if Fraction(2) ** e <= v else e - 1          # 2^e <= v < 2^(e+1)
    e = max(e, -126)
    q = v / Fraction(2) ** (e - 23)                    # in units of the last place
    m, rem = divmod(q.numerator, q.denominator)
    twice = 2 * rem
    if twice > q.denominator or (twice == q.denominator and m & 1):
        m += 1
    return F32(sign * float(m) * 2.0 ** (e - 23))


def _fma_cases():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(1500).astype(F32), rng.standard_normal(1500).astype(F32)
    c = rng.standard_normal(1500).astype(F32)
    near = (-(a.astype(np.float64) * b)).astype(F32)                     # cancellation: the product's low bits decide
    half = rng.integers(1, 2 ** 12, 1500)
    a2, b2 = (half * 2 + 1).astype(F32), F32(2.0 ** -13) * np.ones(1500, F32)
    c2 = rng.integers(2 ** 23, 2 ** 24, 1500).astype(F32)               # a2·b2 ends in exactly half an ulp of c2
    tiny = (rng.standard_normal(1500) * 1e-20).astype(F32)              # subnormal results
    return (np.concatenate([a, a, a2, tiny, a]), np.concatenate([b, b, b2, tiny, b]),
            np.concatenate([c, near, c2, (tiny * 1e-20).astype(F32), np.zeros(1500, F32)]))


def test_emulated_fmaf_is_exact():
    a, b, c = _fma_cases()
    got = R.fmaf(a, b, c)
    for i in range(len(a)):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


def test_chains_are_in_token_order():
    x = np.array([[2.0 ** 24], [1.0], [1.0], [-2.0 ** 24]], F32)       # (n, 1): 2^24 + 1 + 1 − 2^24
    one = np.ones((4, 1), F32)
    assert R.chain_dot(x, one)[0, 0] == 0.0                            # each + 1 is lost; pairwise would give 2
    assert R.chain_dot(x[::-1].copy(), one)[0, 0] == 2.0               # −2^24 + 1 + 1 is exact
    assert R.chain_dot(np.array([[1.0], [1.0], [2.0 ** 24], [-2.0 ** 24]], F32), one)[0, 0] == 2.0
    assert R.chain_norm(np.array([[3.0], [4.0]], F32))[0] == 25.0


def test_oracle_tie_goes_to_the_lowest_column():
    y = np.array([[1, 2, 1, 0.5], [0, 0, 0, 0]], F32)                   # columns 0, 1, 2, 3 all point along e0
    x = np.array([[3, 0], [0, 5]], F32)                                 # p 0 along e0, p 1 along e1
    idx, sc = R.match_field_one(x, y)
    assert idx.tolist() == [0, 0] and sc[0] == 1.0 and sc[1] == 0.0     # p 1: every key is 0, the lowest wins


def test_oracle_unusable_columns():
    nan, inf = np.nan, np.inf
    y = np.array([[0, nan, inf, 1, 1], [0, 1, 1, 1, -1]], F32)          # zero, NaN, inf, usable, usable
    x = np.array([[1, 0, nan, 1e30], [-1, 0, 1, 1e30]], F32)            # usable, zero, NaN, norm overflows
    idx, sc = R.match_field_one(x, y)
    assert idx.tolist() == [4, -1, -1, -1]
    assert np.isneginf(sc[1:]).all() and abs(float(sc[0]) - 1.0) <= 2.0 ** -23
    idx, sc = R.match_field_one(x, y[:, :3])                            # no usable column in y
    assert (idx == -1).all() and np.isneginf(sc).all()
    assert R.bits_equal(np.array([0.0, 1.0], F32), np.array([-0.0, 1.0], F32))
    assert not R.bits_equal(np.array([1.0], F32), np.array([np.nextafter(F32(1), F32(2))], F32))


def test_oracle_batches_and_shared_operands():
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((3, 4, 6)).astype(F32), rng.standard_normal((1, 4, 9)).astype(F32)
    idx, sc = R.match_field(x, y)
    assert idx.shape == (3, 6) and sc.shape == (3, 6)
    for b in range(3):
        i1, s1 = R.match_field_one(x[b], y[0])
        assert (i1 == idx[b]).all() and R.bits_equal(s1, sc[b])
    cos = np.einsum("btp,tq->bpq", x.astype(np.float64), y[0].astype(np.float64))
    cos /= np.linalg.norm(x, axis=1)[:, :, None] * np.linalg.norm(y[0], axis=0)[None, None, :]
    assert (cos.argmax(axis=2) == idx).all() and np.abs(cos.max(axis=2) - sc).max() < 1e-6


# ------------------------------------------------------------------------------------------ the C ABI
A = ctypes.c_void_p(256)
#        x  x_stride P    y  y_stride  Q    B  n  index score ws stream
VALID = (A, 5 * 200, 200, A, 5 * 1369, 1369, 2, 5, A, A, A, None)


def _library():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built")
    return _lib.lib()


def _rc(L, **kw):
    args = list(VALID)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return L.skp_match_field(*args)


@pytest.mark.parametrize("slot", [0, 3, 8, 9, 10])
def test_null_pointers_are_rejected(slot):
    L = _library()
    assert _rc(L, **{f"a{slot}": None}) == -1 and b"null" in L.skp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(a6=0), b"at least 1"), (dict(a7=0), b"at least 1"), (dict(a2=0), b"at least 1"), (dict(a5=0), b"at least 1"),
    (dict(a6=-1), b"at least 1"), (dict(a7=4097, a1=0, a4=0), b"4096"),
    (dict(a2=2 ** 20 + 1, a1=0), b"2^20"), (dict(a5=2 ** 20 + 1, a4=0), b"2^20"),
    (dict(a1=5 * 200 - 1), b"x_stride"), (dict(a4=5 * 1369 - 1), b"y_stride"), (dict(a1=-1000), b"x_stride"),
    (dict(a10=ctypes.c_void_p(260)), b"aligned"),
])
def test_bad_arguments_are_rejected_before_any_launch(kw, word):
    L = _library()
    assert _rc(L, **kw) == -1 and word in L.skp_last_error(), L.skp_last_error()


def test_workspace_query():
    L = _library()
    ws = L.skp_match_field_workspace
    big = ws(1, 500, 16384, 16384)
    assert 0 < big < 8 * 2 ** 20 and big % 8 == 0
    assert 0 < ws(2, 5, 200, 1369) < 10 * 4 * 2 * (200 + 1369) * 8 and ws(1, 1, 1, 1) >= 16
    for bad in ((0, 5, 8, 8), (1, 0, 8, 8), (1, 5, 0, 8), (1, 5, 8, 0), (1, 4097, 8, 8), (1, 5, 2 ** 20 + 1, 8),
                (1, 5, 8, 2 ** 20 + 1), (-3, 5, 8, 8)):
        assert ws(*bad) == -1, bad
    assert ws(2 ** 12, 5, 2 ** 20, 8) == -1                             # 2^31 bytes and more
    # never of the order of P·Q: doubling Q leaves it where it is once the device is full
    assert ws(1, 500, 16384, 2 ** 20) == ws(1, 500, 16384, 2 ** 19)


def test_op_checks_its_arguments_before_the_device():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.match_field(torch.zeros(1, 3, 8), torch.zeros(1, 3, 8))
    assert ops.match_field_flops(4, 500, 16384, 16384) == 2 * 4 * 500 * 16384 ** 2
    assert ops.match_field_bytes(4, 500, 16384, 16384, 4, 1) == 8 * 500 * (4 * 16384 + 16384) + 8 * 4 * 16384


# ------------------------------------------------------------------------------------------ eval on CPU tensors
def _match(S=4, M=2):
    from stablekeypoints_amd.eval import DenseMatch
    P = S * S
    index = torch.arange(P, dtype=torch.int32).repeat(M, 1)
    index[0, 3], index[1, 0], index[1, 5] = -1, 7, 9
    score = torch.linspace(0.1, 0.9, P).repeat(M, 1)
    score[0, 3] = float("-inf")
    back = torch.arange(P, dtype=torch.int32).repeat(M, 1)
    back[1, 9], back[1, 7], back[0, 2] = 6, -1, 14
    bscore = torch.linspace(0.9, 0.2, P).repeat(M, 1)
    bscore[1, 7] = float("-inf")
    from stablekeypoints_amd.eval import _cycle_distance
    cycle = _cycle_distance(index, back, S)
    shape = lambda t: t.reshape(M, S, S)
    return DenseMatch(shape(index), shape(score), shape(back), shape(bscore), shape(cycle), torch.zeros(M, 3, 2))


def test_cycle_distance():
    m = _match()
    c = m.cycle.reshape(2, 16)
    assert torch.isinf(c[0, 3]) and torch.isinf(c[1, 0])                # index −1; back_index −1 at the matched pixel
    assert c[0, 0] == 0 and c[0, 2] == float(np.float32(np.sqrt(3 ** 2 + 0 ** 2)))   # 2 -> 2 -> 14: (0, 2) to (3, 2)
    assert c[1, 5] == float(np.float32(np.sqrt(0 ** 2 + 1 ** 2)))       # 5 -> 9 -> 6: (1, 1) to (1, 2)
    assert c.dtype == torch.float32


def test_transfer_labels_and_its_gates():
    from stablekeypoints_amd.eval import transfer_labels
    m = _match()
    labels = torch.arange(16).reshape(4, 4) % 5 - 1                     # −1 … 3
    out = transfer_labels(m, labels)
    assert out.dtype == torch.int16 and tuple(out.shape) == (2, 4, 4)
    flat, lab = out.reshape(2, 16), labels.reshape(16)
    assert flat[0, 3] == -1 and flat[1, 0] == lab[7] and flat[1, 5] == lab[9] and flat[0, 6] == lab[6]
    gated = transfer_labels(m, labels, max_cycle=0.5).reshape(2, 16)
    assert gated[0, 2] == -1 and gated[1, 5] == -1 and gated[1, 0] == -1 and gated[0, 6] == lab[6]
    assert transfer_labels(m, labels, max_cycle=1.0).reshape(2, 16)[1, 5] == lab[9]      # cycle == max_cycle stays
    low = transfer_labels(m, labels, min_score=0.5).reshape(2, 16)
    keep = m.score.reshape(2, 16) >= 0.5
    assert (low[~keep] == -1).all() and (low[keep] == flat[keep]).all()
    with pytest.raises(ValueError, match="labels must be"):
        transfer_labels(m, labels.float())
    with pytest.raises(ValueError, match="labels must be"):
        transfer_labels(m, labels[:3])
    with pytest.raises(ValueError, match="32767"):
        transfer_labels(m, labels + 40000)


def test_transfer_points_dense():
    from stablekeypoints_amd.eval import transfer_points_dense
    m = _match()
    nan = float("nan")
    pts = torch.tensor([[0.0, 0.6], [nan, 0.5], [0.5, 0.3], [1.0, 1.0], [0.49, 0.99]])   # pixels 2, -, 9, 15, 7
    pos, sc = transfer_points_dense(m, pts)
    assert tuple(pos.shape) == (2, 5, 2) and tuple(sc.shape) == (2, 5)
    assert pos[0, 0].tolist() == [3 / 4, 2 / 4] and pos[1, 0].tolist() == [0.0, 2 / 4]   # back_index 14 and 2
    assert torch.isnan(pos[:, 1]).all() and torch.isneginf(sc[:, 1]).all()
    assert pos[1, 2].tolist() == [1 / 4, 2 / 4] and sc[1, 2] == m.back_score.reshape(2, 16)[1, 9]
    assert pos[0, 3].tolist() == [3 / 4, 3 / 4]                                          # clamped to S − 1
    assert torch.isnan(pos[1, 4]).all() and torch.isneginf(sc[1, 4]) and pos[0, 4].tolist() == [1 / 4, 3 / 4]
    many = torch.rand(1000, 2)
    assert tuple(transfer_points_dense(m, many)[0].shape) == (2, 1000, 2)                # Q is not limited
    with pytest.raises(ValueError, match="points must be"):
        transfer_points_dense(m, pts[:, :1])


def test_parser_has_the_dense_flags():
    from stablekeypoints_amd.main import build_parser
    a = build_parser().parse_args([])
    assert a.dense_transfer is None and a.dense_size == 128 and a.dense_tokens == "all"
    assert a.dense_max_cycle is None and a.dense_min_score is None
    a = build_parser().parse_args(["--dense_transfer", "mask", "--dense_size", "64", "--dense_tokens", "indices",
                                   "--dense_max_cycle", "2.5", "--dense_min_score", "0.3"])
    assert (a.dense_transfer, a.dense_size, a.dense_tokens, a.dense_max_cycle, a.dense_min_score) == \
        ("mask", 64, "indices", 2.5, 0.3)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--dense_tokens", "some"])
