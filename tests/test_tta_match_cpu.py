"""CPU-side checks of the match reduce and the predict stage's --transfer (no GPU needed): the numpy
restatement tests/tta_match_ref.py by hand and against a direct einsum, the conditions its cases must keep
meeting, the parser, the aliases, the byte model, the argument checks and the workspace size of
skp_tta_reduce_match through the C ABI, and eval.describe_points on a hand-made average."""
import ctypes

import numpy as np
import pytest
import torch

import tta_abi
import tta_match_ref
import tta_ref
from tta_match_ref import CHUNKED_SHAPES, MATCH_SHAPES, QS, match_ref, queries_of, sequential_scores

_ids = lambda s: "B{}_C{}_n{}_S{}".format(*s)


@pytest.fixture(scope="module")
def averages():
    """Every shape's float64 restatement of the GPU tests' (special) inputs, computed once."""
    out = {}
    for shape in MATCH_SHAPES:
        maps, theta, _ = tta_ref.make_case(shape)
        _, avg, num = tta_ref.tta_ref(maps, theta)
        out[shape] = (avg, num)
    return out


def test_match_ref_by_hand():
    """Twelve tokens at 2 x 2 pixels: the chunked and the sequential sums differ in fp32, and the scores with them."""
    avg = np.zeros((1, 12, 2, 2), np.float32)
    avg[0, :, 0, 0] = [4096, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]         # nrm: 2^24 + 1 + 1 rounds to 2^24 in chunk 0
    avg[0, :, 0, 1] = [3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]            # |a| = 5
    #                 row 1: all-zero signatures
    q = np.zeros((2, 12), np.float32)
    q[0, :2] = [0.6, 0.8]
    q[1, 0], q[1, 10], q[1, 11] = 4096, 1, 1
    nrm, dot = tta_match_ref.sums(avg, q)
    assert nrm.dtype == np.float32 and dot.dtype == np.float32
    assert nrm[0, 0, 0] == 2.0 ** 24 + 2.0                             # chunk 0 holds 2^24, chunk 1 holds 2
    assert tta_match_ref.sums(avg, q, chunk=12)[0][0, 0, 0] == 2.0 ** 24          # the sequential sum loses all four ones
    assert dot[0, 1, 0, 0] == 2.0 ** 24 + 2.0 and tta_match_ref.sums(avg, q, chunk=12)[1][0, 1, 0, 0] == 2.0 ** 24
    pos, score, smap = match_ref(avg, q)
    seq = sequential_scores(avg, q)
    assert smap[0, 1, 0, 0] != seq[0, 1, 0, 0]
    assert smap[0, 1, 0, 0] == np.float32(2.0 ** 24 + 2.0) / np.sqrt(np.float32(2.0 ** 24 + 2.0))
    assert seq[0, 1, 0, 0] == np.float32(4096.0)
    assert smap[0, 0, 0, 1] == np.float32(np.float32(np.float32(3) * np.float32(0.6)) + np.float32(4) * np.float32(0.8)) / np.float32(5)
    assert np.isneginf(smap[0, :, 1, :]).all()
    assert pos.tolist() == [[[0.5, 1.5], [0.5, 0.5]]] and score[0, 0] == smap[0, 0, 0, 1] and score[0, 1] == smap[0, 1, 0, 0]
    # up to one chunk the two orders are the same
    assert np.array_equal(match_ref(avg[:, :10], q[:, :10])[2], sequential_scores(avg[:, :10], q[:, :10]))
    # nothing to match: (0.5, 0.5) and −inf; an infinite average: −inf, never NaN
    pos, score, smap = match_ref(np.zeros((2, 3, 4, 4), np.float32), np.ones((1, 3), np.float32))
    assert (pos == 0.5).all() and np.isneginf(score).all() and np.isneginf(smap).all()
    bad = np.ones((1, 2, 2, 2), np.float32)
    bad[0, 0, 0, 0] = np.inf
    pos, score, smap = match_ref(bad, np.ones((1, 2), np.float32))
    assert np.isneginf(smap[0, 0, 0, 0]) and pos.tolist() == [[[0.5, 1.5]]] and not np.isnan(smap).any()


@pytest.mark.parametrize("shape", MATCH_SHAPES, ids=_ids)
def test_match_ref_in_float64_is_the_direct_cosine(averages, shape):
    avg = averages[shape][0]
    q, _ = queries_of(avg.astype(np.float32), 16)
    pos, score, smap = match_ref(avg, q)
    assert pos.dtype == np.float64 and score.dtype == np.float64 and smap.dtype == np.float64
    q64 = q.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        direct = np.einsum("bnyx,qn->bqyx", avg, q64) / np.sqrt(np.einsum("bnyx,bnyx->byx", avg, avg))[:, None]
    ok = np.isfinite(direct) & np.isfinite(smap)
    assert np.array_equal(np.isneginf(smap), ~np.isfinite(direct) | (np.einsum("bnyx,bnyx->byx", avg, avg) <= 0)[:, None])
    bound = avg.shape[1] * 2.0 ** -50                      # sums of n float64 terms, reordered; |score| <= 1 or so
    err = float(np.abs(smap - direct)[ok].max())
    print(f"{shape}: max |match_ref - einsum| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    B, n, S, _ = avg.shape
    idx = np.where(np.isneginf(smap), -np.inf, smap).reshape(B, 16, -1).argmax(axis=2)
    assert np.array_equal(pos, np.stack([idx // S + 0.5, idx % S + 0.5], axis=-1))
    assert np.array_equal(score, np.take_along_axis(smap.reshape(B, 16, -1), idx[..., None], 2)[..., 0])
    p32, s32, m32 = match_ref(avg.astype(np.float32), q)
    assert p32.dtype == np.float32 and s32.dtype == np.float32 and m32.dtype == np.float32


@pytest.mark.parametrize("shape", CHUNKED_SHAPES, ids=_ids)
def test_cases_tell_the_chunked_sums_from_the_sequential(averages, shape):
    a32 = averages[shape][0].astype(np.float32)
    for Q in QS:
        q, _ = queries_of(a32, Q)
        differ = float((match_ref(a32, q)[2].view(np.int32) != sequential_scores(a32, q).view(np.int32)).mean())
        print(shape, Q, "chunked score differs in bits from the sequential at", differ, "of the (query, pixel) pairs")
        assert differ > 0.1


@pytest.mark.parametrize("shape", [s for s in MATCH_SHAPES if s[2] >= 3], ids=_ids)
def test_winners_spread_over_the_tiles(averages, shape):
    avg, num = averages[shape]
    a32 = avg.astype(np.float32)
    q, pix = queries_of(a32, 16)
    assert len(set(pix.tolist())) == 16
    pos, score, _ = match_ref(a32, q)
    for b in range(shape[0]):
        if not (num[b] > 0).any():
            continue                                       # every copy out of view: one winner, pixel 0
        tiles = len(set(tta_match_ref.tiles_of(pos[b], shape[3]).tolist()))
        print(shape, "image", b, "winners in", tiles, "tiles")
        assert tiles >= 4


def test_uncovered_pixels_score_minus_infinity(averages):
    for shape in ((2, 3, 5, 37), (2, 2, 26, 37)):
        avg, num = averages[shape]
        a32 = avg.astype(np.float32)
        uncovered = num == 0
        print(shape, "uncovered pixels per image", uncovered.sum(axis=(1, 2)).tolist())
        assert uncovered.any()
        q, _ = queries_of(a32, 3)
        pos, score, smap = match_ref(a32, q)
        assert np.isneginf(smap[np.broadcast_to(uncovered[:, None], smap.shape)]).all()
        assert not np.isnan(smap).any()
    avg, num = averages[tta_ref.ALL_OUT_OF_VIEW]
    assert (num[-1] == 0).all()
    pos, score, _ = match_ref(avg.astype(np.float32), queries_of(avg.astype(np.float32), 3)[0])
    assert (pos[-1] == 0.5).all() and np.isneginf(score[-1]).all() and np.isfinite(score[0]).all()


def test_parser_transfer(capsys):
    from stablekeypoints_amd.main import build_parser, main
    p = build_parser()
    a = p.parse_args([])
    assert a.transfer is None and a.transfer_points is None and a.transfer_size == 128 and a.transfer_tokens == "all"
    a = p.parse_args(["--start_from_stage", "predict", "--transfer", "2", "--transfer_points", "x.pt", "--transfer_size",
                      "64", "--transfer_tokens", "indices"])
    assert a.transfer == 2 and a.transfer_points == "x.pt" and a.transfer_size == 64 and a.transfer_tokens == "indices"
    with pytest.raises(SystemExit):
        p.parse_args(["--transfer_tokens", "some"])
    capsys.readouterr()
    for argv, message in (
            (["--transfer", "2"], "--transfer belongs to --start_from_stage predict"),
            (["--start_from_stage", "predict", "--transfer", "0"], "--transfer must be at least 1"),
            (["--start_from_stage", "predict", "--transfer", "-3"], "--transfer must be at least 1"),
            (["--start_from_stage", "predict", "--transfer_points", "x.pt"], "--transfer_points belongs to --transfer"),
            (["--start_from_stage", "predict", "--transfer", "2", "--transfer_size", "1"],
             "--transfer_size must be at least 2")):
        with pytest.raises(SystemExit):
            main(argv)
        assert message in capsys.readouterr().err


def test_transfer_is_reachable_through_the_reference_names():
    import stablekeypoints_amd.eval as ev
    import unsupervised_keypoints.eval as ref_ev
    assert ref_ev.describe_points is ev.describe_points and ref_ev.transfer_keypoints is ev.transfer_keypoints
    assert ev.Transferred._fields == ("points", "score", "token_points", "score_maps")


def test_ops_tta_reduce_match_refuses_cpu_tensors():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tta_reduce_match(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 2, 3), torch.zeros(1, 1))


def test_byte_model():
    from stablekeypoints_amd import ops
    B, C, n, S, Q = 4, 10, 10, 512, 16
    plain = 4 * B * C * n * S * S
    assert ops.tta_reduce_match_bytes(B, C, n, S, Q) == plain + 4 * Q * n + 12 * B * Q
    assert ops.tta_reduce_match_bytes(B, C, n, S, Q, scores=True, avg=True) == (
        plain + 4 * B * n * S * S + 4 * Q * n + 12 * B * Q + 4 * B * Q * S * S)
    B, C, n, S, Q = 4, 10, 500, 128, 16
    assert ops.tta_reduce_match_bytes(B, C, n, S, Q) == (
        4 * B * C * n * S * S + 4 * Q * n + 12 * B * Q + 2 * 4 * (Q + 1) * B * 50 * S * S)
    assert ops.tta_reduce_match_bytes(1, 2, 11, 8, 3, scores=True) == (
        4 * 2 * 11 * 64 + 4 * 3 * 11 + 12 * 3 + 2 * 4 * 4 * 2 * 64 + 4 * 3 * 64)
    # the per-chunk sums are about 17 % of the maps' bytes each way at Q = 16, n = 500
    assert abs(4 * 17 * B * 50 * S * S / (4 * B * C * n * S * S) - 0.17) < 1e-9


# ------------------------------------------------------------------------------------------ the C ABI
A = tta_abi.A
#        maps B  C  n  S  theta queries Q  pos mpos mscore smap avg  ws stream
VALID = (A, 2, 3, 5, 37, A, A, 3, A, A, A, None, None, A, None)
REQUIRED = (0, 5, 6, 8, 9, 10, 13)


def _rc(L, **kw):
    args = list(VALID)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return L.skp_tta_reduce_match(*args)


def test_tta_reduce_match_rejects_bad_arguments_without_gpu():
    L = tta_abi.library()
    for slot in REQUIRED:
        assert _rc(L, **{f"a{slot}": None}) == -1, slot
        assert b"null pointer" in L.skp_last_error()
    for Q in (0, 17, -1):
        assert _rc(L, a7=Q) == -1
        assert b"Q must be in [1, 16]" in L.skp_last_error()
    assert _rc(L, a13=ctypes.c_void_p(260)) == -1 and b"8-byte aligned" in L.skp_last_error()
    assert _rc(L, a4=1) == -1 and b"at least 2" in L.skp_last_error()
    assert _rc(L, a1=0) == -1 and b"non-positive" in L.skp_last_error()
    assert _rc(L, a2=40000, a3=500, a4=512) == -1 and b"2^31 elements" in L.skp_last_error()


def _closed_form(B, n, S, Q):
    """skp_tta_reduce's partials; with more than one chunk of 10 tokens Q + 1 floats per image, chunk and pixel; a
    (score, pixel) partial per image, query and tile (one chunk) or 64 pixels (more); each array rounded up to 8 bytes."""
    T = -(-S // 64) * -(-S // 4)
    chunks = -(-n // 10)
    r8 = lambda x: (x + 7) // 8 * 8
    R = T if chunks == 1 else -(-S * S // 64)
    return 8 * B * n * T + (r8(4 * (Q + 1) * B * chunks * S * S) if chunks > 1 else 0) + 2 * r8(4 * B * Q * R)


@pytest.mark.parametrize("B,n,S,Q", [(2, 5, 37, 3), (1, 29, 37, 16), (4, 500, 128, 16), (1, 1, 2, 1), (1, 10, 512, 7)])
def test_match_workspace_equals_its_closed_form(B, n, S, Q):
    assert tta_abi.library().skp_tta_reduce_match_workspace(B, n, S, Q) == _closed_form(B, n, S, Q)


def test_match_workspace_refuses_bad_shapes():
    W = tta_abi.library().skp_tta_reduce_match_workspace
    assert W(0, 1, 8, 1) == -1 and W(1, 0, 8, 1) == -1 and W(1, 1, 1, 1) == -1 and W(1, 1, -3, 1) == -1
    assert W(1, 5, 8, 0) == -1 and W(1, 5, 8, 17) == -1
    # 2^31 bytes: 20 chunks of 4096² pixels are 17 · 20 · 2^26 bytes of sums
    assert _closed_form(1, 200, 4096, 16) >= 2 ** 31 and W(1, 200, 4096, 16) == -1
    assert W(1, 10, 4096, 16) == _closed_form(1, 10, 4096, 16)


# ------------------------------------------------------------------------------------------ describe_points
def _describe(monkeypatch, avg, points, **kw):
    """eval.describe_points on a hand-made (K, n, S, S) average: the passes yield one exemplar each with
    placeholder maps, and the reduce returns that exemplar's average."""
    from stablekeypoints_amd import eval as ev
    avg = torch.as_tensor(avg, dtype=torch.float32)
    K, n, S, _ = avg.shape

    def passes(name, ldm, images, context, indices, device, layers, noise_level, degrees, scale, translate, C,
               controllers, size, image_batch):
        assert name == "describe_points" and size == S and len(indices) == n
        for k in range(images.shape[0]):
            yield k, 1, torch.full((1, C, n, S, S), float(k)), torch.zeros(1, C, 2, 3)

    def reduce(maps, th_inv, return_avg=False):
        assert return_avg
        return torch.zeros(1, n, 2), avg[int(maps[0, 0, 0, 0, 0])][None]

    monkeypatch.setattr(ev, "_tta_passes", passes)
    monkeypatch.setattr(ev.ops, "tta_reduce", reduce)
    return ev.describe_points(None, torch.zeros(K, 3, 8, 8), points, torch.zeros(1, n, 4), device="cpu", upscale_size=S,
                              augmentation_iterations=2, **kw)


def test_describe_points_normalises_and_skips(monkeypatch):
    nan = float("nan")
    avg = np.zeros((2, 3, 4, 4), np.float32)
    avg[0, :, 1, 2] = [3, 0, 4]             # exemplar 0, pixel (1, 2)
    avg[0, :, 3, 3] = [0, 0, 2]             # exemplar 0, the last pixel
    avg[1, :, 3, 0] = [0, 10, 0]            # exemplar 1, pixel (3, 0)
    avg[1, :, 0, 0] = [np.inf, 1, 1]        # exemplar 1, pixel (0, 0): a signature that is not finite
    points = torch.tensor([
        # 0: on both     1: on exemplar 1 only  2: a zero signature, then a good one  3: past the edge (clamped),
        #                                                                            then half a NaN  4: good, then not finite
        [[0.30, 0.60], [nan, nan], [0.0, 0.0], [1.0, 1.0], [0.30, 0.60]],
        [[0.99, 0.01], [0.80, 0.20], [0.99, 0.01], [nan, 0.5], [0.1, 0.2]]])
    d = _describe(monkeypatch, avg, points)
    assert d.shape == (5, 3) and d.dtype == torch.float32
    # landmark 0: (0.6, 0, 0.8) + (0, 1, 0), then unit length again
    want0 = np.array([3 / 5, 1.0, 4 / 5]) / np.sqrt(2.0)
    assert np.allclose(d[0].numpy(), want0, rtol=0, atol=1e-7)
    assert d[1].tolist() == [0.0, 1.0, 0.0]
    assert d[2].tolist() == [0.0, 1.0, 0.0]                                   # the zero signature added nothing
    assert d[3].tolist() == [0.0, 0.0, 1.0]                                   # floor(1.0 · 4) = 4 -> 3
    assert d[4].tolist() == [np.float32(3 / 5), 0.0, np.float32(4 / 5)]       # the infinite signature added nothing
    # a landmark whose only annotations read a zero and a non-finite signature has no descriptor
    with pytest.raises(ValueError, match=r"landmark\(s\) \[1\]"):
        _describe(monkeypatch, avg, torch.tensor([[[0.30, 0.60], [0.0, 0.0]], [[0.99, 0.01], [0.1, 0.2]]]))
    assert _describe(monkeypatch, avg, points, indices=torch.tensor([5, 1, 2])).shape == (5, 3)


def test_describe_points_rejects_bad_points(monkeypatch):
    avg = np.ones((2, 3, 4, 4), np.float32)
    with pytest.raises(ValueError, match=r"points must be \(2, Q, 2\)"):
        _describe(monkeypatch, avg, torch.zeros(1, 2, 2))
    with pytest.raises(ValueError, match=r"points must be \(2, Q, 2\)"):
        _describe(monkeypatch, avg, torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match=r"landmark\(s\) \[0, 2\]"):
        _describe(monkeypatch, avg, torch.tensor([[[float("nan")] * 2, [0.5, 0.5], [float("nan")] * 2]] * 2))
