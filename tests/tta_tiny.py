"""What the GPU tests of the three TTA reduces share: the sequential composition of the existing
ops that they are all held to, and the tiny model of their end-to-end tests with its seeded
predict_keypoints call."""
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
