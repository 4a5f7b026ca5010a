"""skp_tta_reduce_match / ops.tta_reduce_match, eval.describe_points, eval.transfer_keypoints and the CLI's
predict stage with --transfer on the GPU.

The kernel's pos and avg are held to ops.tta_reduce bit for bit, and its matches and score map, bit for
bit too, to the numpy restatement tests/tta_match_ref.py applied to that average read back: the average
is the parent's kernel, not the code under test, and the restatement's chunk-ordered unfused fp32 sums,
its correctly rounded square root and quotient and its first-occurrence argmax are the contract's.  The
queries are signatures read from that same average.  tests/test_tta_match_cpu.py asserts that the chunked
cases tell the chunked sums from the sequential ones and that the winners spread over the tiles.  Against
the float64 restatement (tests/tta_ref.py, then match_ref in float64) on the finite tokens, the finite
scores stay within twice the error the fp32 numpy restatement on the parent's average shows (the rule of
tests/test_gpu_tta.py), and positions are compared where the float64 winner leads the runner-up by more
than four times that error; at least half of all (image, query) pairs of the suite must do so.
"""
import numpy as np
import pytest
import torch

import tta_ref
import tta_tiny
from tta_match_ref import MATCH_SHAPES, QS, match_ref, queries_of
from tta_tiny import DEV, N_TOK, S_UP, bits as _bits, cli as _cli, same_bits as _same, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
CASES = [(s, q) for s in MATCH_SHAPES for q in QS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    """Every (shape, Q): the inputs, the plain reduce, the match reduce in its four variants and the
    references, computed once and left unchanged.  The float64 average is shared by a shape's three Q."""
    from stablekeypoints_amd import ops
    out = {}
    for shape in MATCH_SHAPES:
        maps_np, theta_np, finite = tta_ref.make_case(shape)
        maps, theta = _dev(maps_np), _dev(theta_np)
        plain_pos, plain_avg = ops.tta_reduce(maps, theta, return_avg=True)
        avg_np = plain_avg.cpu().numpy()
        # the finite tokens alone (the others' maps zeroed), for the float64 comparison
        fin_np = np.where(finite[:, None, :, None, None], maps_np, 0.0).astype(np.float32)
        fin = _dev(fin_np)
        fin_avg_np = ops.tta_reduce(fin, theta, return_avg=True)[1].cpu().numpy()
        avg64 = tta_ref.tta_ref(fin_np, theta_np)[1]
        for Q in QS:
            q_np, _ = queries_of(avg_np, Q)
            q = _dev(q_np)
            out[shape, Q] = dict(
                shape=shape, Q=Q, maps=maps, theta=theta, q=q, plain_pos=plain_pos, plain_avg=plain_avg,
                both=ops.tta_reduce_match(maps, theta, q, return_scores=True, return_avg=True),
                neither=ops.tta_reduce_match(maps, theta, q),
                scores=ops.tta_reduce_match(maps, theta, q, return_scores=True),
                avg=ops.tta_reduce_match(maps, theta, q, return_avg=True),
                ref=match_ref(avg_np, q_np), fin_got=ops.tta_reduce_match(fin, theta, q, return_scores=True),
                fin_ref=match_ref(fin_avg_np, q_np), ref64=match_ref(avg64, q_np))
    torch.cuda.synchronize()
    return out


@pytest.fixture(params=CASES, ids=lambda c: "B{}_C{}_n{}_S{}_Q{}".format(*c[0], c[1]))
def case(request, cases):
    return cases[request.param]


# ------------------------------------------------------------------------------------------ the kernel
def test_pos_and_avg_are_tta_reduce_s(case):
    (B, C, n, S), Q = case["shape"], case["Q"]
    pos, mpos, mscore, smap, avg = case["both"]
    assert pos.shape == (B, n, 2) and avg.shape == (B, n, S, S)
    assert mpos.shape == (B, Q, 2) and mpos.dtype == torch.float32
    assert mscore.shape == (B, Q) and mscore.dtype == torch.float32
    assert smap.shape == (B, Q, S, S) and smap.dtype == torch.float32
    for got in (case["both"], case["neither"], case["scores"], case["avg"]):
        assert torch.equal(_bits(got[0]), _bits(case["plain_pos"]))
    for got in (case["both"], case["avg"]):
        assert torch.equal(_bits(got[4]), _bits(case["plain_avg"]))


def test_matches_are_the_restatement_on_the_average(case):
    _, mpos, mscore, smap, _ = case["both"]
    want_pos, want_score, want_map = case["ref"]
    assert want_pos.dtype == np.float32 and want_score.dtype == np.float32 and want_map.dtype == np.float32
    assert not np.isnan(want_map).any()
    print(case["shape"], case["Q"], "scores differ at", int((smap.cpu().numpy().view(np.int32) != want_map.view(np.int32)).sum()),
          "of", want_map.size, "pixels, positions at", int((mpos.cpu().numpy() != want_pos).any(-1).sum()), "of",
          want_score.size, "pairs")
    assert _same(smap, want_map)
    assert _same(mscore, want_score)
    assert _same(mpos, want_pos)


def test_results_do_not_depend_on_what_is_asked_for(case):
    assert case["neither"][3] is None and case["neither"][4] is None
    assert case["scores"][4] is None and case["avg"][3] is None
    for other in (case["neither"], case["scores"], case["avg"]):
        for a, b in zip(case["both"][:3], other[:3]):
            assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(case["both"][3]), _bits(case["scores"][3]))


def test_workspace_reuse_after_another_shape(case):
    from stablekeypoints_amd import ops
    other = MATCH_SHAPES[-1] if case["shape"] != MATCH_SHAPES[-1] else MATCH_SHAPES[1]
    maps_np, theta_np, _ = tta_ref.make_case(other, seed=1)
    q = torch.ones(16 if case["Q"] != 16 else 3, other[2], device=DEV)
    ops.tta_reduce_match(_dev(maps_np), _dev(theta_np), q, return_scores=True)
    again = ops.tta_reduce_match(case["maps"], case["theta"], case["q"], return_scores=True)
    for a, b in zip(case["both"][:4], again[:4]):
        assert torch.equal(_bits(a), _bits(b))


def test_no_score_is_nan_and_degenerate_images(case):
    (B, C, n, S), Q = case["shape"], case["Q"]
    _, mpos, mscore, smap, avg = case["both"]
    assert not torch.isnan(smap).any() and not torch.isnan(mscore).any()
    if case["shape"] == tta_ref.ALL_OUT_OF_VIEW:        # the last image: every copy out of view
        assert (avg[-1] == 0).all() and torch.isneginf(smap[-1]).all()
        assert torch.isneginf(mscore[-1]).all() and (mpos[-1] == 0.5).all()
    # the queries were read at pixels of image 0: there each finds a cosine of 1 up to rounding
    assert float(mscore[0].min()) > 1 - 1e-5 and float(mscore[0].max()) < 1 + 1e-5
    assert float(mpos.min()) >= 0.5 and float(mpos.max()) <= S - 0.5


def _clear_pairs(case):
    """The float64 comparison of one case -> (pairs whose float64 winner leads by more than four times
    the restatement's error, all pairs)."""
    _, mpos, mscore, smap, _ = case["fin_got"]
    own_pos, own_score, own_map = case["fin_ref"]
    ref_pos, ref_score, ref_map = case["ref64"]
    got_map = smap.cpu().numpy()
    both = np.isfinite(ref_map) & np.isfinite(own_map)
    assert np.array_equal(np.isfinite(got_map), np.isfinite(own_map))
    with np.errstate(invalid="ignore"):                 # −inf − −inf where both are −inf: masked out
        own_err = float(np.abs(own_map.astype(np.float64) - ref_map)[both].max()) if both.any() else 0.0
        got_err = float(np.abs(got_map.astype(np.float64) - ref_map)[both].max()) if both.any() else 0.0
    B, Q = ref_score.shape
    top = np.sort(ref_map.reshape(B, Q, -1), axis=2)[..., -2:]
    with np.errstate(invalid="ignore"):
        gap = top[..., 1] - top[..., 0]                 # NaN where both are −inf: not clear
    clear = gap > 4 * own_err
    print(f"{case['shape']} Q={Q}: numpy on the average vs float64 {own_err:.3e}, skp_tta_reduce_match vs float64 "
          f"{got_err:.3e}; {int(clear.sum())} of {clear.size} pairs lead by more than 4x that (smallest lead "
          f"{np.nanmin(gap) if np.isfinite(gap).any() else float('nan'):.3e})")
    assert got_err <= 2 * own_err
    assert np.array_equal(mpos.cpu().numpy().astype(np.float64)[clear], ref_pos[clear])
    return int(clear.sum()), clear.size


def test_against_float64_restatement(case):
    _clear_pairs(case)


def test_half_of_all_pairs_have_a_clear_winner(cases):
    found = [_clear_pairs(c) for c in cases.values()]
    clear, pairs = sum(f[0] for f in found), sum(f[1] for f in found)
    print(f"{clear} of {pairs} (image, query) pairs have a clear float64 winner")
    assert 2 * clear >= pairs


def test_tta_reduce_match_rejects_bad_arguments():
    from stablekeypoints_amd import ops
    m, th = torch.zeros(1, 2, 3, 8, 8, device=DEV), torch.zeros(1, 2, 2, 3, device=DEV)
    q = torch.zeros(2, 3, device=DEV)
    with pytest.raises(ValueError, match="theta_inv"):
        ops.tta_reduce_match(m, torch.zeros(1, 3, 2, 3, device=DEV), q)
    with pytest.raises(ValueError, match="maps must be"):
        ops.tta_reduce_match(torch.zeros(1, 2, 3, 8, 4, device=DEV), th, q)
    with pytest.raises(ValueError, match="queries must be"):
        ops.tta_reduce_match(m, th, torch.zeros(2, 4, device=DEV))
    with pytest.raises(ValueError, match="queries must be"):
        ops.tta_reduce_match(m, th, torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match=r"Q must be in \[1, 16\]"):
        ops.tta_reduce_match(m, th, torch.zeros(0, 3, device=DEV))
    with pytest.raises(ValueError, match=r"Q must be in \[1, 16\]"):
        ops.tta_reduce_match(m, th, torch.zeros(17, 3, device=DEV))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tta_reduce_match(m, th, torch.zeros(2, 3))
    with pytest.raises(ValueError, match="bad shape"):
        ops.tta_reduce_match(torch.zeros(1, 1, 1, 1, 1, device=DEV), torch.zeros(1, 1, 2, 3, device=DEV),
                             torch.zeros(1, 1, device=DEV))


# ------------------------------------------------------------------------------------------ end to end
KW = dict(device=DEV, layers=[0, 1, 2, 3], upscale_size=S_UP, augmentation_iterations=3, image_batch=2, **tta_tiny.AUG)


def _describe(tiny, points, indices):
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, _ = tiny
    tta_tiny.seed()
    return ev.describe_points(ldm, images[:points.shape[0]], points, ctx, indices, controllers=controllers, **KW)


def _transfer(tiny, desc, indices, **kw):
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, _ = tiny
    tta_tiny.seed()
    return ev.transfer_keypoints(ldm, images, ctx, desc, indices, controllers=controllers, **KW, **kw)


def _points(K, Q):
    g = torch.Generator().manual_seed(3)
    return 0.1 + 0.8 * torch.rand(K, Q, 2, generator=g)


@pytest.mark.parametrize("every", [False, True], ids=["five_indices", "all_tokens"])
def test_transfer_keypoints_tiny(tiny, every):
    """The five indices are one chunk of tokens, the whole context (n = 16) two; 17 landmarks are two calls."""
    from stablekeypoints_amd import eval as ev
    M, S = 2, S_UP
    indices = None if every else tiny[4]
    n = N_TOK if every else len(tiny[4])
    points = _points(1, 17)
    desc = _describe(tiny, points, indices)
    assert desc.shape == (17, n) and desc.dtype == torch.float32
    assert torch.allclose(desc.double().pow(2).sum(1), torch.ones(17, dtype=torch.float64, device=desc.device), atol=1e-6)
    got = _transfer(tiny, desc, indices, return_score_maps=True)
    assert isinstance(got, ev.Transferred)
    assert got.points.shape == (M, 17, 2) and got.score.shape == (M, 17) and got.token_points.shape == (M, n, 2)
    assert got.score_maps.shape == (M, 17, S, S)
    # the averages of predict_keypoints from the same seed: the descriptors are read from image 0's, and the
    # matches are the restatement on them
    model = tiny[:4] + (torch.arange(N_TOK) if every else tiny[4],)
    kp, maps = tta_tiny.predict(model, tiny[2], augmentation_iterations=3, image_batch=2, return_maps=True)
    assert torch.equal(got.token_points, kp)
    want_pos, want_score, want_map = match_ref(maps.cpu().numpy(), desc.cpu().numpy())
    assert _same(got.points, want_pos / np.float32(S)) and _same(got.score, want_score)
    assert _same(got.score_maps, want_map)
    pix = torch.floor(points[0] * S).clamp(0, S - 1).long()
    sig = maps[0][:, pix[:, 0], pix[:, 1]].T.double().cpu()
    assert torch.allclose(desc.double().cpu(), sig / sig.pow(2).sum(1, keepdim=True).sqrt(), atol=1e-6)
    assert float(got.score[0].min()) > 1 - 1e-5        # the exemplar finds its own landmarks
    # 17 landmarks = 16 + 1
    first, last = _transfer(tiny, desc[:16], indices), _transfer(tiny, desc[16:], indices)
    assert first.score_maps is None
    assert torch.equal(_bits(got.points), _bits(torch.cat([first.points, last.points], dim=1)))
    assert torch.equal(_bits(got.score), _bits(torch.cat([first.score, last.score], dim=1)))
    assert torch.equal(first.token_points, kp) and torch.equal(last.token_points, kp)
    # a second call from the same seed gives the same bits
    again = _transfer(tiny, desc, indices, return_score_maps=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    assert torch.equal(_bits(_describe(tiny, points, indices)), _bits(desc))


def test_transfer_refuses_a_process_group_and_bad_descriptors(tiny, monkeypatch):
    from stablekeypoints_amd import optimize
    with pytest.raises(ValueError, match="descriptors must be"):
        _transfer(tiny, torch.zeros(2, 4), tiny[4])
    monkeypatch.setattr(optimize, "_world", lambda: (2, 0))
    with pytest.raises(ValueError, match="single process"):
        _transfer(tiny, torch.ones(2, 5), tiny[4])
    with pytest.raises(ValueError, match="single process"):
        _describe(tiny, _points(1, 2), tiny[4])


def test_cli_transfer_tiny(tmp_path):
    from PIL import Image
    from stablekeypoints_amd import ops
    plain = tmp_path / "plain"
    kp_plain = _cli(plain)
    assert not (plain / "transferred_keypoints.pt").exists() and not (plain / "transfer.png").exists()
    K, Q, M, S = 2, 3, 5, 64
    points = _points(K, Q)
    points[1, 2] = float("nan")             # landmark 2 is annotated on the first exemplar only
    torch.save(points, tmp_path / "points.pt")
    out = tmp_path / "transfer"
    kp = _cli(out, "--transfer", str(K), "--transfer_points", str(tmp_path / "points.pt"), "--transfer_size", str(S),
              "--visualize")
    assert torch.equal(kp.view(torch.int32), kp_plain.view(torch.int32))
    assert open(plain / "keypoints.csv").read() == open(out / "keypoints.csv").read()
    desc = torch.load(out / "transfer_descriptors.pt", weights_only=True)
    pts = torch.load(out / "transferred_keypoints.pt", weights_only=True)
    score = torch.load(out / "transfer_scores.pt", weights_only=True)
    assert desc.shape == (Q, N_TOK) and desc.dtype == torch.float32          # --transfer_tokens all
    assert pts.shape == (M, Q, 2) and pts.dtype == torch.float32 and ((pts > 0) & (pts < 1)).all()
    assert score.shape == (M, Q) and score.dtype == torch.float32 and torch.isfinite(score).all()
    # a cosine of non-negative vectors (the maps are softmax outputs), up to the rounding of 16-term fp32 sums; the
    # exemplars need not reach 1: the transfer draws its own thetas, so their averages are not the descriptors'
    assert float(score.min()) >= 0 and float(score.max()) <= 1 + 1e-5
    rows = open(out / "transferred_keypoints.csv").read().splitlines()
    assert len(rows) == M and all(len(r.split(",")) == 1 + 3 * Q for r in rows)
    assert [float(v) for v in rows[1].split(",")[1:]] == torch.cat([pts[1], score[1, :, None]], dim=-1).flatten().tolist()
    assert not (out / "transfer_error.pt").exists()     # the annotations were not the dataset's
    sheet = Image.open(out / "transfer.png")
    assert sheet.size[::-1] == ops.sheet_shape(512, 512, 1, 5, downscale=2)
    assert np.asarray(sheet).std() > 0
    with pytest.raises(ValueError, match="--transfer 6"):
        _cli(tmp_path / "many", "--transfer", "6", "--transfer_points", str(tmp_path / "points.pt"))


def test_cli_transfer_tokens_indices_tiny(tmp_path):
    torch.save(_points(1, 2), tmp_path / "one.pt")
    out = tmp_path / "indices"
    kp = _cli(out, "--transfer", "1", "--transfer_points", str(tmp_path / "one.pt"), "--transfer_size", "64",
              "--transfer_tokens", "indices")
    assert kp.shape == (5, 5, 2)
    assert torch.load(out / "transfer_descriptors.pt", weights_only=True).shape == (2, 5)
    assert torch.load(out / "transferred_keypoints.pt", weights_only=True).shape == (5, 2, 2)
    assert not (out / "transfer.png").exists() and not (out / "transfer_error.pt").exists()


def test_transfer_stage_with_the_datasets_own_annotations(tmp_path, monkeypatch, capsys):
    """The items' kpts are the annotations, visibility 0 is NaN, and transfer_error.pt is the distance to them
    (describe_points and transfer_keypoints replaced: this is the stage's own arithmetic)."""
    from stablekeypoints_amd import eval as ev, main
    M, K, Q = 4, 2, 3
    g = torch.Generator().manual_seed(0)
    kpts = torch.rand(M, Q, 2, generator=g)
    vis = torch.ones(M, Q)
    vis[0, 1] = vis[3, 2] = 0
    data = [{"img": torch.rand(3, 8, 8, generator=g), "kpts": kpts[i], "visibility": vis[i]} for i in range(M)]
    moved = torch.rand(M, Q, 2, generator=g)
    seen = {}

    def describe(ldm, images, points, context, **kw):
        seen["points"], seen["K"], seen["kw"] = points.clone(), images.shape[0], kw
        return torch.eye(Q, 4)

    def transfer(ldm, images, context, desc, **kw):
        assert images.shape[0] == M and kw == seen["kw"]
        return ev.Transferred(moved, torch.ones(M, Q), torch.zeros(M, 4, 2), None)

    monkeypatch.setattr(ev, "describe_points", describe)
    monkeypatch.setattr(ev, "transfer_keypoints", transfer)
    args = main.build_parser().parse_args(["--start_from_stage", "predict", "--transfer", str(K), "--save_folder",
                                           str(tmp_path), "--device", DEV, "--transfer_size", "32"])
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    main.transfer_stage(args, None, None, torch.zeros(1, 4, 8), torch.arange(4), data)
    assert torch.equal(cpu, torch.get_rng_state()) and torch.equal(dev, torch.cuda.get_rng_state(DEV))
    assert seen["K"] == K and seen["kw"]["indices"] is None and seen["kw"]["upscale_size"] == 32
    want = kpts.clone()
    want[vis == 0] = float("nan")
    assert tta_tiny.same_values(seen["points"], want[:K])
    err = torch.load(tmp_path / "transfer_error.pt", weights_only=True)
    assert err.shape == (M, Q) and tta_tiny.same_values(err, (moved - want).pow(2).sum(-1).sqrt())
    assert torch.isnan(err[0, 1]) and torch.isnan(err[3, 2]) and int(torch.isnan(err).sum()) == 2
    rest = err[K:][~torch.isnan(err[K:])]
    assert f"mean distance to the annotations {float(rest.mean()):.4f} over 5 visible" in capsys.readouterr().out
    with pytest.raises(ValueError, match="--transfer 5"):
        args.transfer = 5
        main.transfer_stage(args, None, None, torch.zeros(1, 4, 8), torch.arange(4), data)
