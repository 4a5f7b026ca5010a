"""eval._tta_passes, the capture-pass loop of predict_keypoints, correspond_images and part_maps, on
the CPU (no GPU and no libskp.so needed): the pass sizes, the order of the theta draws, which theta
warps which copy of which image, the inverse thetas of each pass and the refusals.

The capture and the warp are stubs, as in tests/test_distributed_gloo.py: the warp is
``img * θ[0, 0] + θ[0, 2]``, so a warped copy shows which theta it met, and a captured map is its
copy's mean plus the token id.
"""
import pytest
import torch

M, C, N, S = 3, 2, 3, 8
AUG = dict(degrees=30, scale=(0.9, 1.1), translate=(0.1, 0.1))
INDICES = torch.tensor([1, 3, 5])


@pytest.fixture
def stubs(monkeypatch):
    """The stubbed capture and warp; returns what they saw: the warp's thetas and the capture's
    batches, one entry per pass, and cudnn.deterministic as each capture found it."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    seen = dict(theta=[], batch=[], deterministic=[], controllers=1)

    def capture(ldm, images, context, indices=None, upsample_res=None, **kw):
        seen["batch"].append(images.clone())
        seen["deterministic"].append(torch.backends.cudnn.deterministic)
        tok = torch.as_tensor(indices).float().reshape(-1, 1, 1)
        one = [images[b].mean() + tok.expand(-1, upsample_res, upsample_res) for b in range(images.shape[0])]
        return [one] * seen["controllers"]

    def warp(self, img, theta=None):
        assert theta is not None     # the loop draws its thetas itself, one draw_theta(1) at a time
        self.last_params = {"theta": theta}
        seen["theta"].append(theta.clone())
        return img * theta[:, 0, 0].reshape(-1, 1, 1, 1) + theta[:, 0, 2].reshape(-1, 1, 1, 1)

    monkeypatch.setattr(ptp_utils, "run_and_find_attn_per_image", capture)
    monkeypatch.setattr(RandomAffineWithInverse, "__call__", warp)
    return seen


def _images(m=M):
    return torch.rand(m, 3, 8, 8, generator=torch.Generator().manual_seed(5))


def _passes(images, iterations=C, image_batch=None, indices=INDICES, size=S, name="predict_keypoints"):
    from stablekeypoints_amd import eval as ev
    return list(ev._tta_passes(name, None, images, None, indices, "cpu", (0, 1), -1, AUG["degrees"], AUG["scale"],
                               AUG["translate"], iterations, {"cpu": None}, size, image_batch))


def _plain_draws(count):
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    T = RandomAffineWithInverse(**AUG)
    return torch.cat([T.draw_theta(1) for _ in range(count)])


def test_pass_sizes(stubs, monkeypatch):
    from stablekeypoints_amd import eval as ev
    images = _images()
    monkeypatch.setattr(ev, "AUG_BATCH_PIXELS", 2 * C * 64)
    assert [(i0, nb) for i0, nb, _, _ in _passes(images)] == [(0, 2), (2, 1)]
    assert [(i0, nb) for i0, nb, _, _ in _passes(images, image_batch=1)] == [(0, 1), (1, 1), (2, 1)]
    assert [(i0, nb) for i0, nb, _, _ in _passes(images, image_batch=5)] == [(0, 3)]
    for i0, nb, maps, th_inv in _passes(images):
        assert maps.shape == (nb, C, N, S, S) and th_inv.shape == (nb, C, 2, 3)
        assert th_inv.device.type == "cpu" and th_inv.dtype == torch.float32
    assert _passes(images[0])[0][:2] == (0, 1)      # a single (3, 8, 8) image is M = 1
    assert stubs["batch"][-1].shape == (C, 3, 8, 8)


def test_thetas_are_the_plain_draws_in_order_and_meet_their_copies(stubs, monkeypatch):
    from stablekeypoints_amd import eval as ev
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    images = _images()
    monkeypatch.setattr(ev, "AUG_BATCH_PIXELS", 2 * C * 64)
    torch.manual_seed(77)
    want = _plain_draws(M * C)
    state = torch.get_rng_state()
    was = torch.backends.cudnn.deterministic
    torch.manual_seed(77)
    passes = _passes(images)
    assert torch.equal(torch.get_rng_state(), state)       # M·C draws and nothing else from the CPU generator
    assert torch.equal(torch.cat(stubs["theta"]), want)
    assert stubs["deterministic"] == [True, True] and torch.backends.cudnn.deterministic == was
    for (i0, nb, maps, th_inv), theta, batch in zip(passes, stubs["theta"], stubs["batch"]):
        assert torch.equal(theta, want[i0 * C:(i0 + nb) * C])
        for j in range(nb):
            for c in range(C):
                th = want[(i0 + j) * C + c]     # copy c of image i is warped by theta i·C + c
                assert torch.equal(batch[j * C + c], images[i0 + j] * th[0, 0] + th[0, 2])
                for t, tok in enumerate(INDICES.tolist()):
                    assert torch.equal(maps[j, c, t], (batch[j * C + c].mean() + float(tok)).expand(S, S))
        T = RandomAffineWithInverse(**AUG)
        T.last_params = {"theta": theta}
        assert torch.equal(th_inv, T.theta_inverse().reshape(nb, C, 2, 3))


def test_default_pass_keeps_the_maps_below_2_31_elements(stubs, monkeypatch):
    """(2^31 − 1) // (C·n·S²) = 1 while the pixel bound allows 3: one image per pass; ``image_batch``
    is taken as given; and the loop asks ``_images_per_pass`` with its own C, n and S."""
    from stablekeypoints_amd import eval as ev
    monkeypatch.setattr(ev, "AUG_BATCH_PIXELS", 3 * 2 * 64)
    C_, n_, S_ = 2, 600, 1024
    assert (2 ** 31 - 1) // (C_ * n_ * S_ * S_) == 1 and ev.AUG_BATCH_PIXELS // (64 * C_) == 3
    assert ev._images_per_pass(None, 64, C_, n_, S_) == 1
    assert ev._images_per_pass(None, 64, C_, 3, 8) == 3
    assert ev._images_per_pass(None, 64, 1000, 3, 8) == 1          # never less than one image
    assert ev._images_per_pass(7, 64, C_, n_, S_) == 7 and ev._images_per_pass(0, 64, C_, 3, 8) == 1
    asked = []
    monkeypatch.setattr(ev, "_images_per_pass", lambda *a: (asked.append(a), 1)[1])
    assert [(i0, nb) for i0, nb, _, _ in _passes(_images())] == [(0, 1), (1, 1), (2, 1)]
    assert asked == [(None, 64, C, N, S)]


def test_refusals(stubs, monkeypatch):
    from stablekeypoints_amd import optimize
    images = _images()
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match=r"images must be \(M, 3, H, W\) or \(3, H, W\)"):
        _passes(torch.zeros(2, 4, 8, 8))
    with pytest.raises(ValueError, match="augmentation_iterations must be at least 1"):
        _passes(images, iterations=0)
    monkeypatch.setattr(optimize, "_world", lambda: (2, 0))
    with pytest.raises(ValueError, match=r"part_maps runs in a single process \(world size must be 1\)"):
        _passes(images, name="part_maps")
    assert torch.equal(torch.get_rng_state(), state) and not stubs["theta"]     # refused before any draw
    monkeypatch.setattr(optimize, "_world", lambda: (1, 0))
    stubs["controllers"] = 2
    with pytest.raises(ValueError, match=r"\(one controller\)"):
        _passes(images)
