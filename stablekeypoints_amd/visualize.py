"""Visualisation stage (mirror of reference ``visualize.py``): keypoint and heat-map sheets.

``visualize_attn_maps`` (``visualize.py:141-264``) and ``create_vid`` (``:268-387``) keep the
reference's signatures.  The reference draws with matplotlib on the host; here every sheet is
composited on the device by ``ops.render_sheet`` (``skp_render_sheet``) straight from the TTA
maps and images, and Python only encodes the PNG.
"""
import os

import torch

from . import ops
from .eval import find_max_pixel, pixel_from_weighted_avg, run_image_with_context_augmented


def save_png(sheet, path):
    """Write a (Hs, Ws, 3) uint8 tensor as PNG."""
    from PIL import Image
    Image.fromarray(sheet.cpu().numpy()).save(path, format="PNG")


def _rank0():
    from .optimize import _world
    return _world()[1] == 0


def _dataset(dataset, dataset_name, dataset_loc, validation):
    if dataset is not None:
        return dataset
    from .datasets import make_dataset
    return make_dataset(dataset_name, dataset_loc, validation=validation, split="test")


@torch.no_grad()
def visualize_attn_maps(ldm, context, indices, device="cuda", from_where=("down_cross", "mid_cross", "up_cross"),
                        upsample_res=32, layers=(0, 1, 2, 3, 4, 5), lr=5e-3, noise_level=-1, num_tokens=1000,
                        num_points=30, num_images=100, regressor=None, augment_degrees=30, augment_scale=(0.9, 1.1),
                        augment_translate=(0.1, 0.1), augmentation_iterations=20, dataset_loc="~",
                        save_folder="outputs", visualize=False, dataset_name="celeba_aligned", controllers=None,
                        num_gpus=1, max_loc_strategy="argmax", height=11, width=9, validation=False, dataset=None,
                        upscale_size=512, downscale=4):
    """visualize.py:141-264: the TTA maps of ``indices`` on ``height·width`` randomly chosen test
    images (``torch.randperm`` from the CPU generator, image ``randperm[i % len(dataset)]``),
    their maxima / ``upscale_size``, and the sheets, written by rank 0 to ``save_folder``:

    * ``unsupervised_keypoints.png``: ``height × width`` images, one marker per keypoint;
    * ``keypoint_{i:03d}.png`` per index: 2 × 10, the first ten images over the same images under
      token i's map at alpha 0.7 (2 × ``height·width`` when there are fewer than ten images),
      at half of ``downscale`` (the reference's 256-pixel tiles at the defaults);
    * with ``regressor``: ``estimated_keypoints.png`` (``((points − 0.5) @ regressor) + 0.5``) and
      ``gt_keypoints.png`` (the dataset's ``kpts``).

    Returns the (``height·width``, ``num_points``, 2) points, normalised (row, col).  Extras:
    ``dataset`` overrides the lookup, ``upscale_size`` is the TTA map size, ``downscale`` the
    source pixels per sheet pixel.  With torch.distributed initialised every rank runs the TTA
    (it holds collectives).  ``visualize`` is accepted and never passed on: the TTA debug figure
    of eval.py:230-353 is not built.

    Departures from the reference: the files are PNG sheets (the reference writes PDF figures
    and JPEG data under a ``.png`` name); the regressor branch reshapes by ``height·width``,
    where the reference uses the unrelated ``num_images`` (visualize.py:252, which only works
    when the two agree).
    """
    dataset = _dataset(dataset, dataset_name, dataset_loc, validation)
    count = height * width
    randperm = torch.randperm(len(dataset))
    imgs, maps, gt_kpts = [], [], []
    for i in range(count):
        batch = dataset[randperm[i % len(dataset)].item()]
        img = torch.as_tensor(batch["img"]).to(device, torch.float32)
        gt_kpts.append(torch.as_tensor(batch["kpts"]))
        imgs.append(img)
        maps.append(run_image_with_context_augmented(
            ldm, img, context, indices.cpu(), device=device, from_where=from_where, layers=layers,
            noise_level=noise_level, augment_degrees=augment_degrees, augment_scale=augment_scale,
            augment_translate=augment_translate, augmentation_iterations=augmentation_iterations, visualize=False,
            controllers=controllers, num_gpus=num_gpus, save_folder=save_folder, upscale_size=upscale_size))
    imgs = torch.stack(imgs)
    maps = torch.stack(maps)   # (count, num_points, S, S), on the device
    num_points = maps.shape[1]
    flat = maps.reshape(count * num_points, upscale_size, upscale_size)
    if max_loc_strategy == "argmax":
        points = find_max_pixel(flat) / float(upscale_size)
    else:   # pixel_from_weighted_avg zeroes its input in place (eval.py:137): the sheets keep the maps
        points = pixel_from_weighted_avg(flat.clone()) / float(upscale_size)
    points = points.reshape(count, num_points, 2)
    if not _rank0():
        return points
    os.makedirs(save_folder, exist_ok=True)
    grid = dict(rows=height, cols=width, downscale=downscale)
    save_png(ops.render_sheet(imgs, None, points, **grid), os.path.join(save_folder, "unsupervised_keypoints.png"))
    m = min(10, count)
    two = torch.cat([imgs[:m], imgs[:m]])
    over = [False] * m + [True] * m
    for i in range(num_points):
        heat = maps[:m, i]
        sheet = ops.render_sheet(two, torch.cat([heat, heat]), None, rows=2, cols=m, downscale=max(1, downscale // 2),
                                 overlay=over)
        save_png(sheet, os.path.join(save_folder, f"keypoint_{i:03d}.png"))
    if regressor is not None:
        est = ((points.reshape(count, -1) - 0.5) @ regressor.to(points.device, points.dtype)) + 0.5
        save_png(ops.render_sheet(imgs, None, est.reshape(count, -1, 2), **grid),
                 os.path.join(save_folder, "estimated_keypoints.png"))
        gt = torch.stack(gt_kpts).to(device, torch.float32)
        save_png(ops.render_sheet(imgs, None, gt, **grid), os.path.join(save_folder, "gt_keypoints.png"))
    return points


@torch.no_grad()
def create_vid(ldm, contexts, indices, device="cuda", from_where=("down_cross", "mid_cross", "up_cross"),
               layers=(0, 1, 2, 3, 4, 5), noise_level=-1, num_points=30, num_images=100, augment_degrees=30,
               augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), augment_shear=(0.0, 0.0),
               augmentation_iterations=20, dataset_loc="~", save_folder="outputs", controllers=None, num_gpus=1,
               max_loc_strategy="argmax", dataset_name="celeba_aligned", validation=False, max_num_frames=1_000,
               dataset=None, render_frames=False):
    """visualize.py:268-387: per test image, in index order, the mean over ``contexts`` of the TTA
    maps at ``upscale_size=128`` and ``find_max_pixel(map) / 512``; rank 0 writes ``keypoints.pt``
    ((len(dataset), num_points, 2)) and ``saved_maps.pt`` (a list of CPU maps) to ``save_folder``.
    Returns the keypoints.

    The reference's quirks are kept: the divisor stays 512 although the maps are 128 pixels wide
    (so the points span [0, 0.25]); ``max_num_frames`` (like ``augment_shear``, ``num_points``,
    ``num_images`` and ``max_loc_strategy``) is accepted and unused.  Extras: ``dataset``
    overrides the lookup; ``render_frames`` also writes ``frame_{i:04d}.png``, a 1 × 1 sheet of
    the image with its markers (what the reference's commented-out ``plot_point_single`` drew;
    the markers are placed on the 128-pixel scale the maps have).
    """
    dataset = _dataset(dataset, dataset_name, dataset_loc, validation)
    rank0 = _rank0()
    if rank0:
        os.makedirs(save_folder, exist_ok=True)
    keypoints, saved_maps = [], []
    for i in range(len(dataset)):
        img = torch.as_tensor(dataset[i]["img"]).to(device, torch.float32)
        maps = torch.stack([run_image_with_context_augmented(
            ldm, img, ctx, indices.cpu(), device=device, from_where=from_where, layers=layers,
            noise_level=noise_level, augment_degrees=augment_degrees, augment_scale=augment_scale,
            augment_translate=augment_translate, augmentation_iterations=augmentation_iterations,
            controllers=controllers, num_gpus=num_gpus, save_folder=save_folder, upscale_size=128)
            for ctx in contexts])
        mean = torch.mean(maps, dim=0)
        saved_maps.append(mean.cpu())
        point = find_max_pixel(mean) / 512.0
        keypoints.append(point)
        if render_frames and rank0:
            sheet = ops.render_sheet(img[None], None, (point * 4.0)[None], rows=1, cols=1, pad=0)
            save_png(sheet, os.path.join(save_folder, f"frame_{i:04d}.png"))
    keypoints = torch.stack(keypoints)
    if rank0:
        torch.save(keypoints, os.path.join(save_folder, "keypoints.pt"))
        torch.save(saved_maps, os.path.join(save_folder, "saved_maps.pt"))
    return keypoints
