"""CPU-side checks of the windowed refine: the oracle (tests/match_refine_ref.py) against the brute-force
oracle, a synthetic displacement recovered through pool, coarse field and refine, the C ABI's argument
checks (no device needed), ops' checks before the device, and the CLI's flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

import match_field_ref as R
import match_refine_ref as W

F32 = np.float32


def signed(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


# ------------------------------------------------------------------------------------------ the oracle
def test_oracle_agrees_with_brute_force_inside_the_window():
    n, S, f, w = 3, 12, 3, 2
    x, y = signed(1, n, S, S), signed(2, n, S, S)
    y[:, 4, 5] = 0
    y[1, 7, 7] = np.nan
    x[:, 0, 1] = 0
    coarse = np.random.default_rng(3).integers(0, (S // f) ** 2, (S // f, S // f))
    dot = R.chain_dot(x.reshape(n, -1), y.reshape(n, -1))
    bi, bs = R.match_field_one(x.reshape(n, -1), y.reshape(n, -1), dot)
    ri, rs = W.match_refine_one(x, y, coarse, f, w, dot)
    _, allowed = W.windows(coarse, S, f, w)
    inside = (bi >= 0) & allowed[np.arange(S * S), np.maximum(bi, 0)]
    assert 5 < inside.sum() < S * S                                      # both kinds of pixel occur
    assert np.array_equal(ri.reshape(-1)[inside], bi[inside])
    assert R.bits_equal(rs.reshape(-1)[inside], bs[inside])
    assert ri[0, 1] == -1 and np.isneginf(rs[0, 1])
    # outside: a match of the window, never a better key than the brute-force one
    out = ~inside & (ri.reshape(-1) >= 0)
    assert allowed[np.flatnonzero(out), ri.reshape(-1)[out]].all()
    assert (rs.reshape(-1)[out] <= bs[out]).all()


def test_oracle_with_a_window_that_covers_the_plane_is_the_brute_force_oracle():
    n, S = 4, 12
    x, y = signed(4, n, S, S), signed(5, n, S, S)
    y[:, 3, 3], y[0, 11, 0], x[:, 5, 5], x[2, 0, 0] = 0, np.inf, 0, np.nan
    y[:, 9, 2] = y[:, 1, 8]                                              # a tie: the lowest wins in both
    x[:, 6, 6] = y[:, 1, 8] * 3
    identity = np.arange(S * S).reshape(S, S)
    ri, rs = W.match_refine_one(x, y, identity, 1, 16)
    bi, bs = R.match_field_one(x.reshape(n, -1), y.reshape(n, -1))
    assert np.array_equal(ri.reshape(-1), bi) and R.bits_equal(rs.reshape(-1), bs)
    assert ri[6, 6] == 1 * S + 8 and ri[5, 5] == -1 and ri[0, 0] == -1


def test_oracle_priors_outside_the_grid_and_windows_without_a_usable_pixel():
    n, S, f, w = 2, 8, 2, 1
    x, y = signed(6, n, S, S), signed(7, n, S, S)
    coarse = np.full((4, 4), 5)                                          # cell (1, 1): the centre of (r, c) is (2 + r % 2, 2 + c % 2)
    coarse[0, 0], coarse[0, 1], coarse[3, 3] = -1, 16, 0
    y[:, 0:3, 0:3] = 0                                                   # the windows of x's cell (3, 3), which points at cell 0
    ri, rs = W.match_refine_one(x, y, coarse, f, w)
    assert (ri[0:2, 0:4] == -1).all() and np.isneginf(rs[0:2, 0:4]).all()
    assert ri[6, 6] == -1 and np.isneginf(rs[6, 6])                      # window rows 0-1, columns 0-1: all zero
    assert ri[7, 7] == -1 and ri[6, 7] == -1 and ri[7, 6] == -1          # centre (1, 1): rows 0-2, columns 0-2, clipped, all zero
    assert ri[2, 2] >= 0 and abs(ri[2, 2] // S - 2) <= 1 and abs(ri[2, 2] % S - 2) <= 1
    assert ri[3, 5] >= 0 and abs(ri[3, 5] // S - 3) <= 1 and abs(ri[3, 5] % S - 3) <= 1


SEEDS = (0, 1, 2, 3)


@pytest.mark.parametrize("seed", SEEDS)
def test_synthetic_displacement_is_recovered(seed):
    """48 Gaussian blobs (σ = 5) on a 64 × 64 canvas; x is the window [16:48, 16:48] and y the same window
    displaced so that the true match of (r, c) is (r + 3, c − 5).  Pool by 4, the brute-force oracle at
    8 × 8, the refine oracle with w = 5: at each of the 783 pixels whose true match lies in the plane
    the refined index is the true one.  Seeds 0-3 pass with the fp32 oracle (confirmed before this test
    was committed), as they did in the float64 check of the definition."""
    S, f, w, n = 32, 4, 5, 48
    rng = np.random.default_rng(seed)
    cy, cx = rng.uniform(0, 64, n), rng.uniform(0, 64, n)
    gy, gx = np.mgrid[0:64, 0:64]
    canvas = np.exp(-((gy[None] - cy[:, None, None]) ** 2 + (gx[None] - cx[:, None, None]) ** 2) / (2 * 5.0 ** 2)).astype(F32)
    x, y = canvas[:, 16:48, 16:48], canvas[:, 13:45, 21:53]             # y[r + 3, c − 5] == x[r, c]
    assert np.array_equal(y[:, 3:, :27], x[:, :29, 5:])
    xl, yl = W.pool(x, f), W.pool(y, f)
    coarse, _ = R.match_field_one(xl.reshape(n, -1), yl.reshape(n, -1))
    index, score = W.match_refine_one(x, y, coarse.reshape(S // f, S // f), f, w)
    r, c = np.divmod(np.arange(S * S), S)
    known = (r + 3 < S) & (c - 5 >= 0)
    assert known.sum() == 783
    want = (r + 3) * S + (c - 5)
    wrong = np.flatnonzero(known & (index.reshape(-1) != want))
    assert not len(wrong), (len(wrong), wrong[:5], index.reshape(-1)[wrong[:5]], want[wrong[:5]])
    assert np.abs(score.reshape(-1)[known].astype(np.float64) - 1).max() <= 8 * 2.0 ** -24


# ------------------------------------------------------------------------------------------ the C ABI
A = ctypes.c_void_p(256)
#        x  x_stride       y  y_stride      B  n  S   coarse f  w  index score ws stream
VALID = (A, 5 * 24 * 24, A, 5 * 24 * 24, 2, 5, 24, A, 4, 5, A, A, A, None)


def _library():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built")
    return _lib.lib()


def _rc(L, **kw):
    args = list(VALID)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return L.skp_match_refine(*args)


@pytest.mark.parametrize("slot", [0, 2, 7, 10, 11, 12])
def test_null_pointers_are_rejected(slot):
    L = _library()
    assert _rc(L, **{f"a{slot}": None}) == -1 and b"null" in L.skp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(a4=0), b"at least 1"), (dict(a4=-2), b"at least 1"), (dict(a5=0), b"at least 1"), (dict(a6=0), b"at least 1"),
    (dict(a5=4097, a1=0, a3=0), b"4096"), (dict(a6=1028, a1=0, a3=0), b"1024"),
    (dict(a8=0), b"[1, 8]"), (dict(a8=9), b"[1, 8]"), (dict(a8=5), b"multiple of f"), (dict(a8=7), b"multiple of f"),
    (dict(a9=0), b"[1, 16]"), (dict(a9=17), b"[1, 16]"), (dict(a9=-1), b"[1, 16]"),
    (dict(a1=5 * 24 * 24 - 1), b"x_stride"), (dict(a3=5 * 24 * 24 - 1), b"y_stride"), (dict(a1=-5 * 24 * 24), b"x_stride"),
    (dict(a12=ctypes.c_void_p(260)), b"aligned"),
])
def test_bad_arguments_are_rejected_before_any_launch(kw, word):
    L = _library()
    assert _rc(L, **kw) == -1 and word in L.skp_last_error(), L.skp_last_error()


def test_workspace_query():
    L = _library()
    ws = L.skp_match_refine_workspace
    for good in ((2, 5, 24, 4, 5), (1, 1, 1, 1, 1), (1, 4096, 1024, 8, 16), (4, 500, 512, 4, 5), (3, 7, 16, 1, 16)):
        got = ws(*good)
        assert got > 0 and got % 8 == 0, good
    for bad in ((0, 5, 24, 4, 5), (-1, 5, 24, 4, 5), (2, 0, 24, 4, 5), (2, 5, 0, 4, 5), (2, 4097, 24, 4, 5),
                (2, 5, 1028, 4, 5), (2, 5, 24, 0, 5), (2, 5, 24, 9, 5), (2, 5, 24, 5, 5), (2, 5, 24, 4, 0),
                (2, 5, 24, 4, 17)):
        assert ws(*bad) == -1, bad
    # never of the order of S²·(2w + 1)²: the widest window and the narrowest ask for the same
    assert ws(1, 500, 512, 4, 16) == ws(1, 500, 512, 4, 1) < 4 * 512 * 512


def test_op_checks_its_arguments_before_the_device():
    from stablekeypoints_amd import ops
    x, c = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.match_refine(x, x, c, 3)
    B, n, S, f, w = 4, 500, 512, 4, 5
    assert ops.match_refine_flops(B, n, S, f, w) == 2 * B * n * S * S * 121
    assert ops.match_refine_bytes(B, n, S, f, w, 4, 1) == 4 * n * S * S * 5 + 4 * B * 128 * 128 + 8 * B * S * S
    assert ops.match_refine_bytes(B, n, S, f, w) == 4 * n * S * S * 8 + 4 * B * 128 * 128 + 8 * B * S * S


# ------------------------------------------------------------------------------------------ the CLI
def test_parser_has_the_refine_flags_and_main_refuses_bad_ones(capsys, monkeypatch):
    from stablekeypoints_amd import main as cli, optimize_token
    a = cli.build_parser().parse_args([])
    assert a.dense_coarse is None and a.dense_radius is None
    a = cli.build_parser().parse_args(["--dense_transfer", "mask", "--dense_size", "64", "--dense_coarse", "16",
                                       "--dense_radius", "6"])
    assert (a.dense_size, a.dense_coarse, a.dense_radius) == (64, 16, 6)

    def no_model(*a, **k):
        raise AssertionError("the model was built")

    monkeypatch.setattr(optimize_token, "load_ldm", no_model)
    head = ["--start_from_stage", "predict", "--model_type", "tiny", "--dataset_name", "synthetic", "--dense_transfer", "mask"]
    for extra, word in ((["--dense_size", "64", "--dense_coarse", "24"], "--dense_coarse must divide --dense_size"),
                        (["--dense_size", "64", "--dense_coarse", "0"], "--dense_coarse must divide --dense_size"),
                        (["--dense_size", "64", "--dense_coarse", "64"], "must be in [2, 8]"),
                        (["--dense_size", "64", "--dense_coarse", "4"], "must be in [2, 8]"),
                        (["--dense_size", "64", "--dense_coarse", "16", "--dense_radius", "0"], "--dense_radius must be in [1, 16]"),
                        (["--dense_size", "64", "--dense_coarse", "16", "--dense_radius", "17"], "--dense_radius must be in [1, 16]"),
                        (["--dense_size", "64", "--dense_radius", "3"], "--dense_radius belongs to --dense_coarse")):
        with pytest.raises(SystemExit) as e:
            cli.main(head + extra)
        assert e.value.code not in (0, None)
        assert word in capsys.readouterr().err, extra
