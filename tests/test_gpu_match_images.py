"""eval.match_images end to end on the tiny model of tests/tta_tiny.py at S = 64 with three copies per
image, against the numpy oracle (tests/match_field_ref.py) applied to the averages that
predict_keypoints(return_maps=True) gives for the same seed and draw order; and the CLI's
``--dense_transfer`` on the synthetic dataset."""
import numpy as np
import pytest
import torch

import match_field_ref as R
import tta_tiny
from tta_tiny import DEV, N_TOK, S_UP, cli as _cli, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

KW = dict(device=DEV, layers=[0, 1, 2, 3], upscale_size=S_UP, augmentation_iterations=3, **tta_tiny.AUG)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _match(tiny, **kw):
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, indices = tiny
    tta_tiny.seed()
    return ev.match_images(ldm, images[0], images, ctx, indices, controllers=controllers, image_batch=2, **KW, **kw)


def test_match_images_tiny(tiny):
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, indices = tiny
    M, S, n = 2, S_UP, len(indices)
    got = _match(tiny)
    assert isinstance(got, ev.DenseMatch)
    for t, dt in zip(got[:5], (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32)):
        assert tuple(t.shape) == (M, S, S) and t.dtype == dt
    assert tuple(got.token_points.shape) == (M, n, 2)
    # the same draws: the source's pass alone, then the images' pass of two, without seeding in between
    _, src = tta_tiny.predict(tiny, images[:1], augmentation_iterations=3, image_batch=1, return_maps=True)
    kp, maps = ev.predict_keypoints(ldm, images, ctx, indices, controllers=controllers, image_batch=2, return_maps=True,
                                    **KW)
    assert torch.equal(got.token_points, kp)
    y = src.reshape(n, S * S).cpu().numpy()
    # image 1 in full (the backward dots are the forward ones transposed: the same chains); of image 0
    # every eighth pixel each way, which keeps the oracle to a few seconds
    for b, step in ((1, 1), (0, 8)):
        x = maps[b].reshape(n, S * S).cpu().numpy()
        if step == 1:
            dot = R.chain_dot(x, y)
            want = (R.match_field_one(x, y, dot), R.match_field_one(y, x, dot.T))
        else:
            want = (R.match_field_one(x[:, ::step], y), R.match_field_one(y[:, ::step], x))
        for field, score, (ri, rs) in ((got.index, got.score, want[0]), (got.back_index, got.back_score, want[1])):
            assert np.array_equal(field[b].reshape(-1)[::step].cpu().numpy(), ri), b
            assert R.bits_equal(score[b].reshape(-1)[::step].cpu().numpy(), rs), b
    # cycle, recomputed
    idx, back = got.index.reshape(M, -1).cpu().numpy().astype(np.int64), got.back_index.reshape(M, -1).cpu().numpy()
    hop = np.take_along_axis(back, np.maximum(idx, 0), axis=1).astype(np.int64)
    p = np.arange(S * S)[None]
    d2 = (p // S - np.maximum(hop, 0) // S) ** 2 + (p % S - np.maximum(hop, 0) % S) ** 2
    want = np.where((idx < 0) | (hop < 0), np.inf, np.sqrt(d2.astype(np.float64))).astype(np.float32)
    assert np.array_equal(got.cycle.reshape(M, -1).cpu().numpy(), want)
    assert (idx >= 0).any() and np.isfinite(want).any()
    # a second call from the same seed gives the same bits
    again = _match(tiny)
    assert all(torch.equal(tta_tiny.bits(a), tta_tiny.bits(b)) for a, b in zip(got, again))
    # labels and points ride on the field
    labels = (torch.arange(S * S).reshape(S, S) % 7 - 1).to(DEV)
    moved = ev.transfer_labels(got, labels)
    ok = got.index >= 0
    assert moved.dtype == torch.int16 and torch.equal(moved[ok].long(), labels.reshape(-1)[got.index[ok].long()])
    assert (moved[~ok] == -1).all()
    pos, sc = ev.transfer_points_dense(got, torch.rand(40, 2, generator=torch.Generator().manual_seed(5)))
    assert tuple(pos.shape) == (M, 40, 2) and tuple(sc.shape) == (M, 40)


def test_match_images_refuses_a_process_group_and_a_bad_source(tiny, monkeypatch):
    from stablekeypoints_amd import eval as ev, optimize
    ldm, controllers, images, ctx, indices = tiny
    with pytest.raises(ValueError, match="source must be"):
        ev.match_images(ldm, images, images, ctx, indices, controllers=controllers, **KW)
    monkeypatch.setattr(optimize, "_world", lambda: (2, 0))
    with pytest.raises(ValueError, match="single process"):
        _match(tiny)


def test_cli_dense_transfer_tiny(tmp_path):
    plain = tmp_path / "plain"
    kp_plain = _cli(plain)
    assert not (plain / "dense_index.pt").exists()
    M, S = 5, 64
    labels = torch.full((128, 128), -1, dtype=torch.int64)      # nearest-resized to 64
    labels[32:96, 32:96] = 0
    labels[48:80, 48:80] = 3
    torch.save(labels, tmp_path / "labels.pt")
    out = tmp_path / "dense"
    kp = _cli(out, "--dense_transfer", str(tmp_path / "labels.pt"), "--dense_size", str(S), "--dense_max_cycle", "8")
    assert torch.equal(kp.view(torch.int32), kp_plain.view(torch.int32))
    assert open(plain / "keypoints.csv").read() == open(out / "keypoints.csv").read()
    index, score, cycle, moved = (torch.load(out / f"dense_{k}.pt", weights_only=True)
                                  for k in ("index", "score", "cycle", "labels"))
    for t, dt in ((index, torch.int32), (score, torch.float32), (cycle, torch.float32), (moved, torch.int16)):
        assert tuple(t.shape) == (M, S, S) and t.dtype == dt
    assert int(index.max()) < S * S and int(index.min()) >= -1
    assert set(moved.unique().tolist()) <= {-1, 0, 3}
    assert (moved[cycle > 8] == -1).all() and (moved[index < 0] == -1).all()
    small = labels[::2, ::2].reshape(-1)
    keep = (index >= 0) & ~(cycle > 8)
    assert torch.equal(moved[keep].long(), small[index[keep].long()])
    assert not (out / "dense_fg_iou.pt").exists() and not (out / "dense.png").exists()   # no masks, no --visualize
    with pytest.raises(ValueError, match="carry no mask"):
        _cli(tmp_path / "mask", "--dense_transfer", "mask", "--dense_size", str(S))
