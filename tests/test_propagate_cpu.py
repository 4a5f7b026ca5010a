"""CPU-side checks of label propagation: the oracles (tests/propagate_ref.py) against the existing
oracles and against hand cases, the synthetic sequence through the fp32 oracle, the C ABIs' argument
checks (no device needed), ops' checks before the device, and the CLI's flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

import match_field_ref as R
import match_refine_ref as W
import propagate_ref as P

F32 = np.float32


def signed(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


# ------------------------------------------------------------------------------------------ the match oracle
def spoilt(n, S, seed):
    x, y = signed([seed, 1], n, S, S), signed([seed, 2], n, S, S)
    y[:, 4, 5] = 0
    y[n // 2, 7, 7] = np.nan
    x[:, 0, 1] = 0
    y[:, 9, 2] = y[:, 8, 3]          # a tie inside the windows around it
    x[:, 8, 2] = y[:, 8, 3] * 3
    return x, y


@pytest.mark.parametrize("K", [1, 5])
def test_slot_0_is_the_refine_oracle_with_an_identity_prior(K):
    n, S, w = 3, 12, 2
    x, y = spoilt(n, S, 1)
    dot = R.chain_dot(x.reshape(n, -1), y.reshape(n, -1))
    index, score = P.match_topk_one(x, y, w, K, dot)
    ri, rs = W.match_refine_one(x, y, np.arange(S * S).reshape(S, S), 1, w, dot)
    assert index.shape == (K, S, S) and index.dtype == np.int32 and score.dtype == F32
    assert np.array_equal(index[0], ri) and R.bits_equal(score[0], rs)
    assert index[0, 0, 1] == -1 and np.isneginf(score[:, 0, 1]).all() and (index[:, 0, 1] == -1).all()
    assert index[0, 8, 2] == 8 * S + 3 and (K == 1 or index[1, 8, 2] == 9 * S + 2)      # the tie: the lower q first


def test_a_window_that_covers_the_plane_gives_the_brute_force_oracle_in_slot_0():
    n, S = 4, 12
    x, y = spoilt(n, S, 2)
    index, score = P.match_topk_one(x, y, 16, 3)
    bi, bs = R.match_field_one(x.reshape(n, -1), y.reshape(n, -1))
    assert np.array_equal(index[0].reshape(-1), bi) and R.bits_equal(score[0].reshape(-1), bs)


def test_lists_are_sorted_nested_and_inside_the_window():
    n, S, w, K = 3, 10, 2, 16
    x, y = spoilt(n, S, 3)
    index, score = P.match_topk_one(x, y, w, K)
    short, short_score = P.match_topk_one(x, y, w, 4)
    assert np.array_equal(index[:4], short) and R.bits_equal(score[:4], short_score)
    r, c = np.mgrid[0:S, 0:S]
    live = index >= 0
    assert (np.abs(index // S - r)[live] <= w).all() and (np.abs(index % S - c)[live] <= w).all()
    assert (live[1:] <= live[:-1]).all()                                   # empty slots come last
    both = live[1:]
    assert (score[1:][both] <= score[:-1][both]).all()
    assert (index[9] == -1)[0, 0] and live[8, 0, 0]                        # the corner's window holds 9 pixels
    for p in ((3, 3), (0, 9)):                                             # no q twice
        got = index[:, p[0], p[1]]
        assert len(set(got[got >= 0].tolist())) == (got >= 0).sum()
    # the spoilt pixels of y are in no list
    assert not np.isin(index, [4 * S + 5, 7 * S + 7]).any()


def test_window_dot_is_chain_dot_inside_the_windows():
    n, S, w = 5, 9, 2
    x, y = signed(4, n, S, S), signed(5, n, S, S)
    full, part, inside = R.chain_dot(x.reshape(n, -1), y.reshape(n, -1)), P.window_dot(x, y, w), P.window(S, w)
    assert np.array_equal(full[inside].view(np.int32), part[inside].view(np.int32))
    a, b = P.match_topk(x[None], y[None], w, 4), P.match_topk(x[None], y[None], w, 4, windowed=True)
    assert np.array_equal(a[0], b[0]) and R.bits_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ the vote oracle
def test_vote_one_candidate_gives_back_its_label_exactly():
    S, Cl = 3, 4
    index = np.full((2, 3, S, S), -1, np.int32)
    score = np.full((2, 3, S, S), -np.inf, F32)
    labels = np.random.default_rng(6).random((2, Cl, S, S)).astype(F32)
    index[1, 0, 1, 2], score[1, 0, 1, 2] = 7, 0.25
    soft, label, conf, source = P.label_vote(index, score, labels, P.inv_tau32(0.07), 3)
    assert np.array_equal(soft[:, 1, 2], labels[1, :, 2, 1].astype(np.float64))      # q = 7 = (2, 1)
    assert label[1, 2] == int(labels[1, :, 2, 1].argmax()) and conf[1, 2] == labels[1, :, 2, 1].max()
    assert source[:, 1, 2].tolist() == [1 * S * S + 7, -1, -1]
    # no candidate: 0 / −1 / 0
    assert (soft[:, 0, 0] == 0).all() and label[0, 0] == -1 and conf[0, 0] == 0 and (source[:, 0, 0] == -1).all()


def test_vote_equal_scores_give_the_mean_in_rank_order():
    S, Cl = 2, 3
    index = np.zeros((2, 2, S, S), np.int32)
    score = np.full((2, 2, S, S), 0.5, F32)
    index[0, 0], index[0, 1], index[1, 0], index[1, 1] = 0, 1, 2, 3
    labels = np.random.default_rng(7).random((2, Cl, S, S)).astype(F32)
    soft, label, conf, source = P.label_vote(index, score, labels, P.inv_tau32(0.02), 3)
    want = (labels[0, :, 0, 0].astype(np.float64) + labels[0, :, 0, 1] + labels[1, :, 1, 0]) / 3
    assert np.allclose(soft[:, 1, 1], want, rtol=1e-15, atol=0)
    assert source[:, 1, 1].tolist() == [0, 1, S * S + 2]                              # (j, i) ascending among equals
    # a greater score in the second context comes first; out-of-range indices and NaN scores are no candidates
    score[1, 1, 0, 0], index[0, 0, 0, 0], index[0, 1, 0, 0] = 0.75, S * S, -5
    score[1, 0, 0, 0] = np.nan
    _, _, _, source = P.label_vote(index, score, labels, P.inv_tau32(0.02), 2)
    assert source[:, 0, 0].tolist() == [S * S + 3, -1]


def test_vote_weights_follow_the_definition():
    """Two contexts of one pixel, the first labelled class 0 and the second class 1, scores 0.9 and 0.8."""
    index = np.zeros((2, 1, 1, 1), np.int32)
    score = np.array([0.9, 0.8], F32).reshape(2, 1, 1, 1)
    labels = np.array([[1.0, 0.0], [0.0, 1.0]], F32).reshape(2, 2, 1, 1)
    it = P.inv_tau32(0.1)
    e = np.exp(np.float64(F32(F32(F32(0.8) - F32(0.9)) * it)))             # a_2 in fp32, then exact
    soft, label, conf, _ = P.label_vote(index, score, labels, it, 1)
    assert soft[:, 0, 0].tolist() == [1.0, 0.0] and label[0, 0] == 0 and conf[0, 0] == 1.0
    soft, label, conf, _ = P.label_vote(index[::-1], score[::-1], labels[::-1], it, 1)
    assert soft[:, 0, 0].tolist() == [1.0, 0.0] and label[0, 0] == 0      # the best score, wherever its context lies
    tall = np.concatenate([index, index], axis=1)                          # K = 2 with an empty second slot
    tall[:, 1] = -1
    soft, label, conf, _ = P.label_vote(tall, np.concatenate([score, score], axis=1), labels, it, 2)
    assert np.allclose(soft[:, 0, 0], [1 / (1 + e), e / (1 + e)], rtol=1e-15, atol=0)
    assert label[0, 0] == 0 and conf[0, 0] == soft[0, 0, 0] and 0.26 < soft[1, 0, 0] < 0.28


# ------------------------------------------------------------------------------------------ the sequence
SEEDS = (0, 1, 2, 3)


def test_context_frames():
    assert [P.context_of(t, 2) for t in (1, 2, 3, 4, 7)] == [[0], [0, 1], [0, 1, 2], [0, 2, 3], [0, 5, 6]]
    assert P.context_of(5, 0) == [0] and P.context_of(2, 5) == [0, 1]
    hot = P.one_hot(np.array([[0, 2], [-1, 1]]))
    assert hot.shape == (3, 2, 2) and hot[:, 1, 0].tolist() == [0, 0, 0] and hot[:, 0, 1].tolist() == [0, 0, 1]


@pytest.mark.parametrize("seed", SEEDS)
def test_synthetic_sequence_carries_the_disk(seed):
    """48 Gaussian blobs (σ = 3) on a 96² canvas, frames the 32² windows sliding by (1, −1) per frame, T = 8;
    the label is a disk of radius 7 (class 1 on class 0); w = 3, k = 5, τ = 0.02, memory = 2.  At the last
    frame the propagated foreground's IoU against the true shifted disk is at least 0.5 and at least 0.3
    above the IoU of frame 0's mask left in place (0.096).  With the fp32 oracle, confirmed before this
    test was committed: seed 0 0.644, seed 1 0.649, seed 2 0.678, seed 3 0.713 (the float64 prototype of
    the definition gave 0.65-0.78); every pixel of the last frame has a label."""
    frames, masks = P.sequence(seed)
    assert frames.shape == (8, 48, 32, 32) and masks.all(axis=0).sum() < masks[0].sum()
    label, conf, soft = P.propagate(frames, masks[0].astype(np.int64), P.SEQ["w"], P.SEQ["k"], P.SEQ["tau"], P.SEQ["memory"])
    got, still = P.iou(label[-1] == 1, masks[-1]), P.iou(masks[0], masks[-1])
    print(f"seed {seed}: propagated {got:.4f}, left in place {still:.4f}")
    assert still < 0.11
    assert got >= 0.5 and got >= still + 0.3
    assert (label[-1] >= 0).all() and np.array_equal(label[0], masks[0].astype(np.int32))
    assert np.abs(soft.sum(axis=1).astype(np.float64) - 1).max() <= 1e-5


# ------------------------------------------------------------------------------------------ the C ABIs
A = ctypes.c_void_p(256)
#        x  x_stride       y  y_stride      B  n  S   w  K  index score ws stream
TOPK = (A, 5 * 24 * 24, A, 5 * 24 * 24, 2, 5, 24, 3, 5, A, A, A, None)
#        index score M  K  S   labels Cl inv_tau           Kv soft label conf source stream
VOTE = (A, A, 3, 5, 24, A, 2, ctypes.c_float(14.0), 5, A, A, A, A, None)


def _library():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built")
    return _lib.lib()


def _rc(L, name, valid, **kw):
    args = list(valid)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return getattr(L, name)(*args)


def test_the_new_symbols_are_exported():
    L = _library()
    assert all(hasattr(L, s) for s in ("skp_match_topk", "skp_match_topk_workspace", "skp_label_vote"))


@pytest.mark.parametrize("slot", [0, 2, 9, 10, 11])
def test_match_topk_null_pointers_are_rejected(slot):
    L = _library()
    assert _rc(L, "skp_match_topk", TOPK, **{f"a{slot}": None}) == -1 and b"null" in L.skp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(a4=0), b"at least 1"), (dict(a4=-2), b"at least 1"), (dict(a5=0), b"at least 1"), (dict(a6=0), b"at least 1"),
    (dict(a5=4097, a1=0, a3=0), b"4096"), (dict(a6=1028, a1=0, a3=0), b"1024"),
    (dict(a7=0), b"w must be in [1, 16]"), (dict(a7=17), b"w must be in [1, 16]"), (dict(a7=-1), b"w must be in [1, 16]"),
    (dict(a8=0), b"K must be in [1, 16]"), (dict(a8=17), b"K must be in [1, 16]"), (dict(a8=-3), b"K must be in [1, 16]"),
    (dict(a1=5 * 24 * 24 - 1), b"x_stride"), (dict(a3=5 * 24 * 24 - 1), b"y_stride"), (dict(a1=-5 * 24 * 24), b"x_stride"),
    (dict(a11=ctypes.c_void_p(260)), b"aligned"),
])
def test_match_topk_bad_arguments_are_rejected_before_any_launch(kw, word):
    L = _library()
    assert _rc(L, "skp_match_topk", TOPK, **kw) == -1 and word in L.skp_last_error(), L.skp_last_error()


def test_match_topk_workspace_query():
    L = _library()
    ws = L.skp_match_topk_workspace
    for good in ((2, 5, 24, 3, 5), (1, 1, 1, 1, 1), (1, 4096, 1024, 16, 16), (3, 500, 128, 8, 5), (1, 1, 9, 1, 9)):
        got = ws(*good)
        assert got > 0 and got % 8 == 0, good
    for bad in ((0, 5, 24, 3, 5), (-1, 5, 24, 3, 5), (2, 0, 24, 3, 5), (2, 5, 0, 3, 5), (2, 4097, 24, 3, 5),
                (2, 5, 1028, 3, 5), (2, 5, 24, 0, 5), (2, 5, 24, 17, 5), (2, 5, 24, 3, 0), (2, 5, 24, 3, 17)):
        assert ws(*bad) == -1, bad
    # never of the order of S²·(2w + 1)², nor of K: the widest window and the narrowest ask for the same
    assert ws(3, 500, 512, 16, 16) == ws(3, 500, 512, 1, 1) < 4 * 512 * 512


@pytest.mark.parametrize("slot", [0, 1, 5, 9, 10, 11])
def test_label_vote_null_pointers_are_rejected(slot):
    L = _library()
    assert _rc(L, "skp_label_vote", VOTE, **{f"a{slot}": None}) == -1 and b"null" in L.skp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(a2=0), b"at least 1"), (dict(a3=0), b"at least 1"), (dict(a4=0), b"at least 1"), (dict(a6=0), b"at least 1"),
    (dict(a2=-1), b"at least 1"), (dict(a2=65), b"M > 64"), (dict(a3=17, a8=17), b"K > 16"),
    (dict(a8=0), b"Kv must be in [1, K]"), (dict(a8=6), b"Kv must be in [1, K]"), (dict(a8=-1), b"Kv must be in [1, K]"),
    (dict(a6=257), b"Cl > 256"), (dict(a4=1025), b"S > 1024"),
    (dict(a7=ctypes.c_float(0.0)), b"inv_tau"), (dict(a7=ctypes.c_float(-2.0)), b"inv_tau"),
    (dict(a7=ctypes.c_float(float("inf"))), b"inv_tau"), (dict(a7=ctypes.c_float(float("nan"))), b"inv_tau"),
])
def test_label_vote_bad_arguments_are_rejected_before_any_launch(kw, word):
    L = _library()
    assert _rc(L, "skp_label_vote", VOTE, **kw) == -1 and word in L.skp_last_error(), L.skp_last_error()


# ------------------------------------------------------------------------------------------ ops and eval
def test_ops_check_their_arguments_before_the_device():
    from stablekeypoints_amd import ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.match_topk(x, x, 3, 5)
    i, s, l = torch.zeros(2, 5, 8, 8, dtype=torch.int32), torch.zeros(2, 5, 8, 8), torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.label_vote(i, s, l, 0.07)
    B, n, S, w, k = 3, 500, 128, 8, 5
    assert ops.match_topk_flops(B, n, S, w) == 2 * B * n * S * S * 289
    assert ops.match_topk_bytes(B, n, S, w, k, 1, 3) == 4 * n * S * S * 4 + 8 * B * k * S * S
    assert ops.match_topk_bytes(B, n, S, w, k) == 4 * n * S * S * 6 + 8 * B * k * S * S
    assert ops.label_vote_bytes(3, 5, 128, 2, 5) == 128 * 128 * (8 * 15 + 4 * 2 * 5 + 4 * 2 + 8)
    assert ops.label_vote_bytes(3, 5, 128, 2, 4, source=True) == 128 * 128 * (8 * 15 + 4 * 2 * 4 + 4 * 2 + 8 + 16)


def test_propagate_labels_checks_its_arguments_before_the_device():
    from stablekeypoints_amd import eval as ev
    sig, lab = torch.zeros(2, 3, 8, 8), torch.zeros(8, 8, dtype=torch.int64)
    for kw, word in ((dict(radius=0), "radius"), (dict(radius=17), "radius"), (dict(k=0), "k must"), (dict(k=17), "k must"),
                     (dict(tau=0.0), "tau"), (dict(tau=float("inf")), "tau"), (dict(memory=-1), "memory"),
                     (dict(memory=64), "memory")):
        with pytest.raises(ValueError, match=word):
            ev.propagate_labels(sig, lab, **kw)
    with pytest.raises(ValueError, match="labels0 must be"):
        ev.propagate_labels(sig, torch.zeros(8, 8), device="cpu")
    with pytest.raises(ValueError, match="at least -1"):
        ev.propagate_labels(sig, lab - 2)
    with pytest.raises(ValueError, match="finite and non-negative"):
        ev.propagate_labels(sig, -torch.ones(2, 8, 8))
    with pytest.raises(ValueError, match="signatures must be"):
        ev.propagate_labels(sig[0], lab)
    with pytest.raises(ValueError, match="like labels0"):
        ev.propagate_labels(torch.zeros(2, 3, 6, 6), lab, device="cpu")
    assert ev.PropagatedLabels._fields == ("label", "confidence", "soft")


# ------------------------------------------------------------------------------------------ the CLI
def test_parser_has_the_propagate_flags_and_main_refuses_bad_ones(capsys, monkeypatch):
    from stablekeypoints_amd import main as cli, optimize_token
    a = cli.build_parser().parse_args([])
    assert a.propagate is None
    assert (a.propagate_size, a.propagate_radius, a.propagate_k, a.propagate_tau, a.propagate_memory,
            a.propagate_tokens) == (128, 8, 5, 0.07, 2, "all")
    a = cli.build_parser().parse_args(["--propagate", "mask", "--propagate_size", "64", "--propagate_radius", "4",
                                       "--propagate_k", "3", "--propagate_tau", "0.02", "--propagate_memory", "1",
                                       "--propagate_tokens", "indices"])
    assert (a.propagate, a.propagate_size, a.propagate_radius, a.propagate_k, a.propagate_tau, a.propagate_memory,
            a.propagate_tokens) == ("mask", 64, 4, 3, 0.02, 1, "indices")

    def no_model(*a, **k):
        raise AssertionError("the model was built")

    monkeypatch.setattr(optimize_token, "load_ldm", no_model)
    head = ["--start_from_stage", "predict", "--model_type", "tiny", "--dataset_name", "synthetic", "--propagate", "mask"]
    for argv, word in ((head + ["--propagate_size", "1"], "--propagate_size must be at least 2"),
                       (head + ["--propagate_size", "2048"], "--propagate_size must be at most 1024"),
                       (head + ["--propagate_radius", "0"], "--propagate_radius must be in [1, 16]"),
                       (head + ["--propagate_radius", "17"], "--propagate_radius must be in [1, 16]"),
                       (head + ["--propagate_k", "0"], "--propagate_k must be in [1, 16]"),
                       (head + ["--propagate_k", "17"], "--propagate_k must be in [1, 16]"),
                       (head + ["--propagate_tau", "0"], "--propagate_tau must be positive"),
                       (head + ["--propagate_tau", "inf"], "--propagate_tau must be positive"),
                       (head + ["--propagate_memory", "-1"], "--propagate_memory must be in [0, 63]"),
                       (head + ["--propagate_memory", "64"], "--propagate_memory must be in [0, 63]"),
                       (head + ["--propagate_tokens", "some"], "invalid choice"),
                       (["--model_type", "tiny", "--dataset_name", "synthetic", "--propagate", "mask"],
                        "--propagate belongs to --start_from_stage predict")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code not in (0, None)
        assert word in capsys.readouterr().err, argv
