"""What the GPU tests of the TTA reduces share: the sequential composition of the existing ops that
they are all held to, the bit comparisons, and the tiny model of their end-to-end tests with its
seeded predict_keypoints, correspond_images and part_maps calls and its predict-stage CLI run."""
import numpy as np
import pytest
import torch

DEV = "cuda:0"
R, S_UP, N_TOK = 32, 64, 16
AUG = dict(augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1))


def sequential(maps, theta):
    """The existing ops, one copy at a time: acc = acc + affine_warp(copy) for the maps and for
    ones, the division, NaN -> 0, find_max_pixel.  Returns (pos, avg, num (B, S, S))."""
    from stablekeypoints_amd import ops
    B, C, n, S, _ = maps.shape
    ones = torch.ones(1, n, S, S, device=maps.device)
    avg = torch.empty(B, n, S, S, device=maps.device)
    nums = torch.empty(B, S, S, device=maps.device)
    pos = torch.empty(B, n, 2, device=maps.device)
    for b in range(B):
        acc = torch.zeros(n, S, S, device=maps.device)
        num = torch.zeros(n, S, S, device=maps.device)
        for c in range(C):
            acc = acc + ops.affine_warp(maps[b, c][None], theta[b, c][None])[0]
            num = num + ops.affine_warp(ones, theta[b, c][None])[0]
        a = acc / num
        a[a != a] = 0
        avg[b] = a
        nums[b] = num[0]
        pos[b] = ops.find_max_pixel(a)
    return pos, avg, nums


def bits(t):
    """fp32 as its int32 bits (NaN compares as bits); any other dtype as it is."""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(got, want_np):
    """A device tensor against a numpy array of the same dtype, bit for bit."""
    got = got.cpu().numpy()
    assert got.dtype == want_np.dtype and got.shape == want_np.shape
    return np.array_equal(got.view(np.uint8), np.ascontiguousarray(want_np).view(np.uint8))


def same_values(a, b):
    """Two tensors equal, with NaN in the same places (whatever the NaNs' bits)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros((), device=a.device, dtype=a.dtype)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


def build_tiny():
    """(ldm, controllers, two images, context, token indices) of the tiny model on DEV."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.sd import TINY_CONFIG, TINY_IMAGE, build_sd15
    ldm = build_sd15(seed=0, config=TINY_CONFIG).to(DEV)
    ldm.feature_upsample_res = R
    ctl = ptp_utils.AttentionStore(early_exit=True)
    ptp_utils.register_attention_control(ldm.unet, ctl, feature_upsample_res=R)
    g = torch.Generator().manual_seed(11)
    images = torch.rand(2, 3, TINY_IMAGE, TINY_IMAGE, generator=g)
    ctx = torch.randn(1, N_TOK, 32, generator=g).to(DEV)
    return ldm, {torch.device(DEV): ctl}, images, ctx, torch.tensor([3, 7, 0, 12, 5])


@pytest.fixture(scope="module")
def tiny():
    """``build_tiny()`` once per test module that imports this fixture."""
    return build_tiny()


def seed():
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)


def predict(tiny, images, **kw):
    """predict_keypoints on the tiny model from a fixed seed."""
    from stablekeypoints_amd import eval as ev
    ldm, controllers, _, ctx, indices = tiny
    seed()
    return ev.predict_keypoints(ldm, images, ctx, indices, device=DEV, layers=[0, 1, 2, 3], controllers=controllers,
                                upscale_size=S_UP, **AUG, **kw)


def correspond(tiny, **kw):
    """correspond_images on the tiny model's two images from a fixed seed, both in one pass."""
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, _ = tiny
    seed()
    return ev.correspond_images(ldm, images, ctx, device=DEV, layers=[0, 1, 2, 3], controllers=controllers,
                                upscale_size=S_UP, augmentation_iterations=3, image_batch=2, **AUG, **kw)


def part_maps(tiny, indices, **kw):
    """part_maps on the tiny model's two images from a fixed seed, both in one pass."""
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, _ = tiny
    seed()
    return ev.part_maps(ldm, images, ctx, indices, device=DEV, layers=[0, 1, 2, 3], controllers=controllers,
                        upscale_size=S_UP, augmentation_iterations=3, image_batch=2, **AUG, **kw)


INDICES = torch.tensor([3, 7, 0, 12, 5])


def cli(folder, *extra, indices=INDICES):
    """The CLI's predict stage on the tiny model and five synthetic images, from ``embedding.pt`` and (unless
    ``indices`` is None) ``indices.pt`` written to ``folder`` -> the ``keypoints.pt`` it wrote."""
    from stablekeypoints_amd import main
    folder.mkdir(exist_ok=True)
    g = torch.Generator().manual_seed(7)
    torch.save(torch.randn(1, N_TOK, 32, generator=g), folder / "embedding.pt")
    if indices is not None:
        torch.save(indices, folder / "indices.pt")
    main.main(["--model_type", "tiny", "--dataset_name", "synthetic", "--max_len", "5", "--num_tokens", str(N_TOK),
               "--feature_upsample_res", str(R), "--augmentation_iterations", "2", "--start_from_stage", "predict",
               "--save_folder", str(folder), "--device", DEV, *extra])
    return torch.load(folder / "keypoints.pt", weights_only=True)
