"""eval.match_images coarse to fine on the tiny model of tests/tta_tiny.py at S = 32 with three copies
per image: without the keywords nothing changes; with ``coarse_size=8`` every field is the composition of
the public ops (pool, ops.match_field, ops.match_refine, the cycle) on the averages that
predict_keypoints(return_maps=True) gives for the same seed and draw order; labels and points ride on
the result; and the CLI's ``--dense_coarse`` writes its files at the fine size."""
import pytest
import torch

import tta_tiny
from tta_tiny import DEV, cli as _cli, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

S, SC = 32, 8
KW = dict(device=DEV, layers=[0, 1, 2, 3], upscale_size=S, augmentation_iterations=3, **tta_tiny.AUG)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _match(tiny, **kw):
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, indices = tiny
    tta_tiny.seed()
    return ev.match_images(ldm, images[0], images, ctx, indices, controllers=controllers, image_batch=2, **KW, **kw)


def _same(a, b):
    return all(torch.equal(tta_tiny.bits(s), tta_tiny.bits(t)) for s, t in zip(a, b))


def test_without_a_coarse_size_nothing_changes(tiny):
    plain = _match(tiny)
    assert _same(plain, _match(tiny, coarse_size=None, refine_radius=None))
    assert tuple(plain.index.shape) == (2, S, S)


@pytest.mark.parametrize("radius", [None, 3])
def test_coarse_to_fine_is_the_composition_of_the_public_ops(tiny, radius):
    from stablekeypoints_amd import eval as ev, ops
    ldm, controllers, images, ctx, indices = tiny
    M, n, f = 2, len(indices), S // SC
    w = f + 1 if radius is None else radius
    got = _match(tiny, coarse_size=SC, refine_radius=radius)
    assert isinstance(got, ev.DenseMatch)
    for t, dt in zip(got[:5], (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32)):
        assert tuple(t.shape) == (M, S, S) and t.dtype == dt
    # the same draws: the source's pass alone, then the images' pass of two, without seeding in between
    tta_tiny.seed()
    _, src = ev.predict_keypoints(ldm, images[:1], ctx, indices, controllers=controllers, image_batch=1,
                                  return_maps=True, **KW)
    kp, maps = ev.predict_keypoints(ldm, images, ctx, indices, controllers=controllers, image_batch=2, return_maps=True,
                                    **KW)
    assert torch.equal(got.token_points, kp)
    src, maps = src.reshape(1, n, S, S).contiguous(), maps.reshape(M, n, S, S).contiguous()
    lo_s = torch.nn.functional.avg_pool2d(src, f).contiguous()
    lo_m = torch.nn.functional.avg_pool2d(maps, f).contiguous()
    there, _ = ops.match_field(lo_m.reshape(M, n, SC * SC), lo_s.reshape(1, n, SC * SC))
    back, _ = ops.match_field(lo_s.reshape(1, n, SC * SC), lo_m.reshape(M, n, SC * SC))
    index, score = ops.match_refine(maps, src, there.reshape(M, SC, SC), w)
    back_index, back_score = ops.match_refine(src, maps, back.reshape(M, SC, SC), w)
    cycle = ev._cycle_distance(index.reshape(M, -1), back_index.reshape(M, -1), S).reshape(M, S, S)
    assert _same(got[:5], (index, score, back_index, back_score, cycle))
    assert (got.index >= 0).any() and torch.isfinite(got.cycle).any()
    # every match lies in its window
    centre = there.reshape(M, SC, SC).long().repeat_interleave(f, 1).repeat_interleave(f, 2)
    p = torch.arange(S, device=DEV)
    cr, cc = centre // SC * f + (p % f)[None, :, None], centre % SC * f + (p % f)[None, None, :]
    ok = got.index >= 0
    q = got.index.long()
    assert ((q // S - cr).abs()[ok] <= w).all() and ((q % S - cc).abs()[ok] <= w).all()
    # labels and points ride on the field
    labels = (torch.arange(S * S).reshape(S, S) % 7 - 1).to(DEV)
    moved = ev.transfer_labels(got, labels)
    assert moved.dtype == torch.int16 and torch.equal(moved[ok].long(), labels.reshape(-1)[q[ok]])
    assert (moved[~ok] == -1).all()
    pos, sc = ev.transfer_points_dense(got, torch.rand(40, 2, generator=torch.Generator().manual_seed(5)))
    assert tuple(pos.shape) == (M, 40, 2) and tuple(sc.shape) == (M, 40)


def test_bad_coarse_sizes_and_radii_are_refused(tiny):
    for kw, word in ((dict(coarse_size=12), "coarse_size must divide"), (dict(coarse_size=32), "coarse_size must divide"),
                     (dict(coarse_size=2), "coarse_size must divide"), (dict(coarse_size=8, refine_radius=17), "refine_radius"),
                     (dict(coarse_size=8, refine_radius=0), "refine_radius"), (dict(refine_radius=3), "belongs to coarse_size")):
        with pytest.raises(ValueError, match=word):
            _match(tiny, **kw)


def test_cli_dense_coarse_writes_its_files_at_the_fine_size(tmp_path):
    M = 5
    labels = torch.full((128, 128), -1, dtype=torch.int64)      # nearest-resized to 32
    labels[32:96, 32:96] = 0
    torch.save(labels, tmp_path / "labels.pt")
    plain, out = tmp_path / "plain", tmp_path / "dense"
    kp_plain = _cli(plain)
    kp = _cli(out, "--dense_transfer", str(tmp_path / "labels.pt"), "--dense_size", str(S), "--dense_coarse", str(SC))
    assert torch.equal(kp.view(torch.int32), kp_plain.view(torch.int32))
    index, score, cycle, moved = (torch.load(out / f"dense_{k}.pt", weights_only=True)
                                  for k in ("index", "score", "cycle", "labels"))
    for t, dt in ((index, torch.int32), (score, torch.float32), (cycle, torch.float32), (moved, torch.int16)):
        assert tuple(t.shape) == (M, S, S) and t.dtype == dt
    assert int(index.max()) < S * S and int(index.min()) >= -1 and bool((index >= 0).any())
    small = labels[::4, ::4].reshape(-1)
    keep = index >= 0
    assert torch.equal(moved[keep].long(), small[index[keep].long()])
    with pytest.raises(SystemExit):
        _cli(tmp_path / "bad", "--dense_transfer", str(tmp_path / "labels.pt"), "--dense_size", str(S), "--dense_coarse", "12")
