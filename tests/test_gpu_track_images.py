"""eval.track_images end to end on the tiny model of tests/tta_tiny.py at S = 64 with three copies per
frame, against eval.track_keypoints on the averages that predict_keypoints(return_maps=True) gives for
the same seed and draw order; and the CLI's ``--track`` on the synthetic dataset."""
import pytest
import torch

import tta_tiny
from tta_tiny import DEV, S_UP, bits, cli as _cli, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

KW = dict(device=DEV, layers=[0, 1, 2, 3], upscale_size=S_UP, augmentation_iterations=3, **tta_tiny.AUG)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x.cpu()), bits(y.cpu())) for x, y in zip(a, b))


def test_track_images_equals_track_keypoints_of_the_predicted_maps(tiny):
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, indices = tiny
    frames = torch.cat([images, images.flip(0), images[:1]])          # five frames, a pass of two at a time
    T, n = frames.shape[0], len(indices)
    tta_tiny.seed()
    got = ev.track_images(ldm, frames, ctx, indices, controllers=controllers, image_batch=2, sigma=1.5, radius=5, **KW)
    assert isinstance(got, ev.KeypointTracks)
    assert [tuple(t.shape) for t in got] == [(T, n, 2), (T, n), (T, n, 2)]
    kp, maps = tta_tiny.predict(tiny, frames, augmentation_iterations=3, image_batch=2, return_maps=True)
    want = ev.track_keypoints(maps, sigma=1.5, radius=5)
    assert _same(got, want)
    assert torch.equal(bits(got.independent.cpu()), bits(kp.cpu()))   # the per-frame argmax is predict's keypoint
    assert bool(((got.support >= 0) & (got.support <= 1)).all())
    # a step of at most `radius` pixels per frame and axis
    step = (got.pos[1:] - got.pos[:-1]).abs() * S_UP
    assert float(step.max()) <= 5


def test_track_images_refuses_a_process_group(tiny, monkeypatch):
    from stablekeypoints_amd import eval as ev, optimize
    ldm, controllers, images, ctx, indices = tiny
    monkeypatch.setattr(optimize, "_world", lambda: (2, 0))
    with pytest.raises(ValueError, match="single process"):
        ev.track_images(ldm, images, ctx, indices, controllers=controllers, **KW)


def test_cli_track_tiny(tmp_path, monkeypatch):
    from stablekeypoints_amd import eval as ev
    plain = tmp_path / "plain"
    kp_plain = _cli(plain)
    assert not (plain / "tracked_keypoints.pt").exists()
    # what the stage hands to track_images, and the generators' states at that moment
    seen = {}
    real = ev.track_images

    def spy(ldm, images, context, indices, **kw):
        seen.update(ldm=ldm, images=images, context=context, indices=indices, kw=kw, cpu=torch.get_rng_state(),
                    dev=torch.cuda.get_rng_state(kw["device"]))
        return real(ldm, images, context, indices, **kw)

    monkeypatch.setattr(ev, "track_images", spy)
    out = tmp_path / "track"
    kp = _cli(out, "--track", "--track_size", "64")
    M, n = 5, len(tta_tiny.INDICES)
    assert torch.equal(kp.view(torch.int32), kp_plain.view(torch.int32))
    assert open(plain / "keypoints.csv").read() == open(out / "keypoints.csv").read()
    pos = torch.load(out / "tracked_keypoints.pt", weights_only=True)
    support = torch.load(out / "track_support.pt", weights_only=True)
    assert tuple(pos.shape) == (M, n, 2) and pos.dtype == torch.float32
    assert tuple(support.shape) == (M, n) and support.dtype == torch.float32
    rows = open(out / "tracked_keypoints.csv").read().strip().split("\n")
    assert len(rows) == M and all(len(r.split(",")) == 1 + 3 * n for r in rows)
    assert [float(v) for v in rows[2].split(",")[1:]] == pos[2].reshape(-1).tolist() + support[2].tolist()
    assert not (out / "track.png").exists()                            # no --visualize
    # the same maps from the same generator states, tracked by track_keypoints
    kw = dict(seen["kw"])
    assert kw.pop("upscale_size") == 64 and kw.pop("sigma") == 2.0 and kw.pop("radius") is None
    torch.set_rng_state(seen["cpu"])
    torch.cuda.set_rng_state(seen["dev"], kw["device"])
    _, maps = ev.predict_keypoints(seen["ldm"], seen["images"], seen["context"], seen["indices"], upscale_size=64,
                                   return_maps=True, **kw)
    want = ev.track_keypoints(maps)
    assert torch.equal(bits(pos), bits(want.pos.cpu())) and torch.equal(bits(support), bits(want.support.cpu()))
