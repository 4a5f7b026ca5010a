"""Keypoint extraction: argmax / soft-argmax and test-time augmentation (mirror of reference ``eval.py``).

``find_max_pixel``, ``find_k_max_pixels``, ``mask_radius`` and
``pixel_from_weighted_avg`` (``eval.py:39-155``) run as HIP kernels with the
reference's semantics (first-occurrence argmax, NaN is max, in-place mutation in
``pixel_from_weighted_avg``).  ``run_image_with_context_augmented`` (``:197-355``) is the
test-time-augmentation average on the same kernels; ``evaluate`` (``:374-539``) regresses
keypoints from it and scores them with the reference's five metrics (``keypoint_error``).
``predict_keypoints`` (extra) returns the keypoints of a batch of unlabelled images: batched
captures and the whole TTA reduce (inverse warps, sums, ratio, argmax) in one kernel,
``skp_tta_reduce``; with ``num_subjects`` = k > 1 also the k peaks per token of
``find_k_max_pixels`` on the average, from ``skp_tta_reduce_peaks``.
``find_corresponding_points`` (``:159-195``) picks the tokens whose maps are jointly sharpest on a
set of images; ``correspond_images`` (extra) does so on the TTA averages of unlabelled images, with
each average's argmax and softmax entropy from ``skp_tta_reduce_entropy``.
``part_maps`` (extra) says which of the chosen tokens owns each pixel of unlabelled images: per pixel
the greatest of the tokens' TTA averages, the token that attains it and the tokens' sum from
``skp_tta_reduce_parts``; ``foreground_iou`` scores the labelled pixels against a foreground mask.
``describe_points`` and ``transfer_keypoints`` (extra) carry points annotated on a few exemplar images
over to unlabelled ones: at a pixel the tokens' TTA averages are a signature, an annotated pixel's
signature is its landmark's descriptor, and ``skp_tta_reduce_match`` finds in every other image the
pixel whose signature has the greatest cosine with it.
``match_images`` (extra) matches EVERY pixel of unlabelled images against a source image and back
(``skp_match_field``, the (S², S²) product never in memory; with ``coarse_size`` coarse to fine, the
fine pixels matched inside windows around a coarse field by ``skp_match_refine``); ``transfer_labels`` and
``transfer_points_dense`` read masks, part segmentations and any number of points off that field.
``track_keypoints`` and ``track_images`` (extra) turn the per-frame TTA averages of a video into one
track per token: exact Viterbi over the pixel grid under a truncated Gaussian random walk, a fused
separable max-product per frame (``skp_track_step``) and one walk back (``skp_track_backtrace``).
"""
import collections
import contextlib
import os

import torch

from . import ops, ptp_utils
from .invertable_transform import RandomAffineWithInverse


def find_max_pixel(map):
    """eval.py:39-60: (T, h, w) -> (T, 2) float (row + 0.5, col + 0.5)."""
    return ops.find_max_pixel(map)


def find_k_max_pixels(map, num=3):
    """eval.py:62-81: (num, T, 2)."""
    return ops.find_k_max_pixels(map, num=num)


def mask_radius(map, max_coords, radius):
    """eval.py:83-111."""
    return ops.mask_radius(map, max_coords, radius)


def pixel_from_weighted_avg(heatmaps, distance=5):
    """eval.py:113-155 (zeros pixels beyond ``distance`` IN PLACE, like the reference)."""
    return ops.pixel_from_weighted_avg(heatmaps, distance=distance)


@contextlib.contextmanager
def _reproducible_convolutions():
    """MIOpen restricted to its deterministic solvers while the TTA captures run.  The library's
    default choice for the VAE encoder's stride-2 3×3 convolution at 128² sums in a run-dependent
    order (first seen there: two same-seed TTA calls differed by 2e-8 … 4.5e-8 on map values of
    3e-2), so maps written by one run (``create_vid``'s ``saved_maps.pt``) could not be
    reproduced bit for bit by the next.  The training path does not pass through here."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


# default TTA batch bound: warped copies per capture pass × pixels per copy (10 copies at 512², the
# measured TTA setting, profiles/r03ao_bench_tta.json)
AUG_BATCH_PIXELS = 10 * 512 * 512


def _copy_major(per, copies):
    """``run_and_find_attn_per_image``'s ``per[controller][copy]`` maps as one tensor, copy by copy."""
    return torch.stack([per[k][b] for b in range(copies) for k in range(len(per))])


@torch.no_grad()
def run_image_with_context_augmented(ldm, image, context, indices, device="cuda",
                                     from_where=("down_cross", "mid_cross", "up_cross"), layers=(0, 1, 2, 3, 4, 5),
                                     augmentation_iterations=20, noise_level=-1, augment_degrees=30,
                                     augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), visualize=False,
                                     controllers=None, num_gpus=1, save_folder="outputs", upscale_size=512,
                                     augmentation_batch=None):
    """eval.py:197-355 (hot part 221-266, 327-330): TTA-averaged maps of the chosen tokens.

    ``image`` is (3, H, W) in [0, 1] (torch or numpy HWC).  Each of the
    ``augmentation_iterations // num_gpus`` iterations draws ``num_gpus`` thetas from the CPU
    generator in the reference's order (one per replica, eval.py:238-242).  Replica r's warped
    copy is captured (``indices`` gathered, bilinear to ``upscale_size``: collect_maps), then its
    map and a ones map are inverse-warped and summed.  Returns Σmaps / Σones with NaN → 0.

    ``augmentation_batch`` (extra; None = as many iterations as ``AUG_BATCH_PIXELS`` allows: 10
    at 512², 2 at SDXL's 1024²): how many iterations' warped copies go through ONE batched
    VAE/UNet capture pass.  Peak activation memory grows linearly with it (the reference's loop
    holds one copy at a time), so the default is bounded by image area.  Every copy is captured on its
    own (per-image maps, ``run_and_find_attn_per_image``), the thetas are drawn iteration by
    iteration exactly as the reference draws them, and the copies' contributions are summed in
    iteration order, so this is the reference's loop up to fp32 summation order and the GPU
    noise draw (one ``randn_like`` per batch instead of per copy; the reference's CUDA noise is
    not reproducible on another device anyway).  At batch 1 a 64² latent UNet pass cannot fill
    256 CUs; 10 copies in one pass do.

    Replicas: with torch.distributed initialised and ``num_gpus`` equal to the world size,
    rank r runs replica r of every iteration and the two (n, S, S) sums are all-reduced (SUM)
    once at the end; every rank must hold the same CPU RNG state (same seed) so that all draw
    the same thetas.  In one process, the ``num_gpus`` copies of an iteration are captured in
    the same batched pass.
    """
    if visualize:
        raise NotImplementedError("visualisation is outside the hot path")
    from .optimize import _world
    img = image if torch.is_tensor(image) else torch.as_tensor(image)
    if img.dim() == 3 and img.shape[-1] == 3 and img.shape[0] != 3:
        img = img.permute(2, 0, 1)
    img = img.to(device, torch.float32)
    world, rank = _world()
    if world > 1 and num_gpus != world:
        raise ValueError(f"num_gpus={num_gpus} must equal the world size {world} (one replica per rank)")
    n = len(indices)
    num_samples = torch.zeros(n, upscale_size, upscale_size, device=device)
    sum_samples = torch.zeros(n, upscale_size, upscale_size, device=device)
    T = RandomAffineWithInverse(degrees=augment_degrees, scale=augment_scale, translate=augment_translate)
    iters = augmentation_iterations // num_gpus
    if augmentation_batch is None:
        augmentation_batch = max(1, AUG_BATCH_PIXELS // (img.shape[-1] * img.shape[-2] * max(1, num_gpus // world)))
    chunk = max(1, int(augmentation_batch))
    done = 0
    while done < iters:
        c = min(chunk, iters - done)
        # every rank draws all replicas' thetas, iteration by iteration (eval.py:238-242)
        theta = torch.cat([T.draw_theta(num_gpus) for _ in range(c)])
        if world > 1:
            theta = theta.reshape(c, num_gpus, 2, 3)[:, rank]
        aug = T(img[None].expand(theta.shape[0], -1, -1, -1), theta=theta)
        with _reproducible_convolutions():
            if aug.shape[0] == 1:
                maps = torch.stack(ptp_utils.run_and_find_attn(
                    ldm, aug, context, layers=layers, noise_level=noise_level, from_where=from_where,
                    upsample_res=upscale_size, device=device, controllers=controllers, indices=indices))
            else:
                per = ptp_utils.run_and_find_attn_per_image(ldm, aug, context, noise_level=noise_level,
                                                            device=device, layers=layers, upsample_res=upscale_size,
                                                            indices=indices, controllers=controllers)
                maps = _copy_major(per, aug.shape[0])
        num_samples += T.inverse(torch.ones_like(maps)).sum(dim=0)
        sum_samples += T.inverse(maps).sum(dim=0)
        done += c
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(num_samples)
        dist.all_reduce(sum_samples)
    attention_maps = sum_samples / num_samples
    attention_maps[attention_maps != attention_maps] = 0
    return attention_maps


def swap_points(points):
    """eval.py:358-370: left/right keypoint permutation of Human3.6M (B, K, D)."""
    pairs = [(1, 6), (2, 7), (3, 8), (4, 9), (5, 10), (17, 25), (18, 26), (19, 27), (20, 28), (21, 28), (22, 30),
             (23, 31)]
    perm = list(range(points.shape[1]))
    for a, b in pairs:
        perm[a], perm[b] = b, a
    return points[:, perm, :]


METRICS = ("inter_eye_distance", "visible", "mean_average_error", "pck", "orientation_invariant")


def keypoint_error(highest_indices, regressor, gt_kpts, evaluation_method="inter_eye_distance", visible=None):
    """One image's error (eval.py:467-513): regress (row, col)/512 maxima of the chosen tokens
    to keypoints, ``((p − 0.5) @ W) + 0.5``, and score them against ``gt_kpts`` (K, 2).

    inter_eye_distance: mean L2 / |gt₀ − gt₁|; visible: Σ L2·v / Σ v; mean_average_error:
    Σ L2·v at 256 px scale; pck: fraction within 6 px at 256 px scale; orientation_invariant:
    min over the left/right swap of the mean L2, × 128.
    """
    if evaluation_method not in METRICS:
        raise ValueError(f"evaluation_method must be one of {METRICS}")
    est = ((highest_indices.reshape(1, -1) - 0.5) @ regressor) + 0.5
    est = est.reshape(-1, 2)
    gt = gt_kpts.to(est.device, est.dtype)
    if evaluation_method in ("mean_average_error", "pck"):
        est = est * 256
        gt = gt * 256
    l2 = (est - gt).norm(dim=-1)
    if evaluation_method == "inter_eye_distance":
        eye = torch.sqrt(torch.sum((gt[0] - gt[1]) ** 2, dim=-1))
        return torch.mean(l2 / eye)
    if evaluation_method in ("visible", "mean_average_error"):
        vis = torch.ones_like(l2) if visible is None else visible.to(l2.device, l2.dtype)
        err = (l2 * vis).sum()
        return err / vis.sum() if evaluation_method == "visible" else err
    if evaluation_method == "pck":
        return (l2 < 6).float().mean()
    err = l2.mean()
    swapped = (swap_points(est[None])[0] - gt).norm(dim=-1).mean()
    return torch.minimum(err, swapped) * 128


@torch.no_grad()
def evaluate(ldm, context, indices, regressor, device="cuda", from_where=("down_cross", "mid_cross", "up_cross"),
             upsample_res=32, layers=(0, 1, 2, 3, 4, 5), noise_level=-1, num_tokens=1000, augment_degrees=30,
             augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), augmentation_iterations=20, dataset_loc="~",
             save_folder="outputs", wandb_log=False, visualize=False, dataset_name="celeba_aligned",
             evaluation_method="inter_eye_distance", controllers=None, num_gpus=1, max_loc_strategy="argmax",
             validation=False, dataset=None, upscale_size=512):
    """eval.py:374-539: per test image (shuffled loader, batch 1) the TTA maps of ``indices``,
    their maxima / 512, the regressed keypoints and ``keypoint_error``; writes
    ``all_errors.pt`` (per-image errors) to ``save_folder`` and returns the mean error.
    ``dataset`` (extra) overrides the lookup; ``visualize``/``wandb_log`` are not supported.
    """
    from .datasets import make_dataset
    if evaluation_method not in METRICS:
        raise ValueError(f"evaluation_method must be one of {METRICS}")
    if dataset is None:
        dataset = make_dataset(dataset_name, dataset_loc, validation=validation, split="test")
    loader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=True, drop_last=True)
    it = iter(loader)
    regressor = regressor.to(device, torch.float32)
    values = []
    for _ in range(len(dataset)):
        batch = next(it)
        maps = run_image_with_context_augmented(
            ldm, batch["img"][0], context, indices.cpu(), device=device, from_where=from_where, layers=layers,
            noise_level=noise_level, augmentation_iterations=augmentation_iterations, augment_degrees=augment_degrees,
            augment_scale=augment_scale, augment_translate=augment_translate, controllers=controllers,
            num_gpus=num_gpus, save_folder=save_folder, upscale_size=upscale_size)
        if max_loc_strategy == "argmax":
            highest = find_max_pixel(maps) / 512.0
        else:
            highest = pixel_from_weighted_avg(maps) / 512.0
        vis = batch["visibility"][0] if "visibility" in batch else None
        values.append(float(keypoint_error(highest, regressor, batch["kpts"][0], evaluation_method, vis)))
    os.makedirs(save_folder, exist_ok=True)
    torch.save(torch.tensor(values), os.path.join(save_folder, "all_errors.pt"))
    mean = float(torch.tensor(values).mean()) if values else float("nan")
    print(f"mean distance: {mean}", flush=True)
    return mean


def _images_per_pass(image_batch, pixels, C, n, S):
    """How many images' copies one capture pass holds: ``image_batch`` as given, else what
    ``AUG_BATCH_PIXELS`` allows and what keeps the pass's maps below 2^31 elements; at least 1."""
    if image_batch is not None:
        return max(1, int(image_batch))
    return max(1, min(AUG_BATCH_PIXELS // (pixels * C), (2 ** 31 - 1) // max(1, C * n * S * S)))


def _tta_passes(name, ldm, images, context, indices, device, layers, noise_level, augment_degrees, augment_scale,
                augment_translate, augmentation_iterations, controllers, upscale_size, image_batch):
    """The capture passes of ``predict_keypoints``, ``correspond_images``, ``part_maps``,
    ``describe_points`` and ``transfer_keypoints`` (``name``
    is the caller's, for the messages).  ``images`` (M, 3, H, W) or (3, H, W) in [0, 1]; for image 0,
    then image 1, … C = ``augmentation_iterations`` thetas are drawn, each by one ``draw_theta(1)`` on
    the global CPU generator.  A pass warps the C copies of ``_images_per_pass`` whole images, captures
    the maps of ``indices`` per copy at ``upscale_size`` under ``_reproducible_convolutions`` and yields
    ``(i0, nb, maps, th_inv)``: the pass's first image and image count, its maps (nb, C, n, S, S) and
    the copies' inverse thetas (nb, C, 2, 3) on ``device``.  The generator keeps no reference to a
    pass's maps; a caller that drops its own before asking for the next pass holds one pass at a time."""
    from .optimize import _world
    if _world()[0] > 1:
        raise ValueError(f"{name} runs in a single process (world size must be 1)")
    imgs = images if torch.is_tensor(images) else torch.as_tensor(images)
    if imgs.dim() == 3:
        imgs = imgs[None]
    if imgs.dim() != 4 or imgs.shape[1] != 3:
        raise ValueError(f"images must be (M, 3, H, W) or (3, H, W), got {tuple(imgs.shape)}")
    imgs = imgs.to(device, torch.float32)
    M, C, S, n = imgs.shape[0], int(augmentation_iterations), int(upscale_size), len(indices)
    if C < 1:
        raise ValueError("augmentation_iterations must be at least 1")
    T = RandomAffineWithInverse(degrees=augment_degrees, scale=augment_scale, translate=augment_translate)
    theta = torch.cat([T.draw_theta(1) for _ in range(M * C)]).reshape(M, C, 2, 3)
    per_pass = _images_per_pass(image_batch, imgs.shape[-1] * imgs.shape[-2], C, n, S)
    for i0 in range(0, M, per_pass):
        nb = min(per_pass, M - i0)
        aug = T(imgs[i0:i0 + nb].repeat_interleave(C, dim=0), theta=theta[i0:i0 + nb].reshape(nb * C, 2, 3))
        with _reproducible_convolutions():
            per = ptp_utils.run_and_find_attn_per_image(ldm, aug, context, noise_level=noise_level, device=device,
                                                        layers=layers, upsample_res=S, indices=indices,
                                                        controllers=controllers)
        maps = _copy_major(per, nb * C)
        del per, aug
        if tuple(maps.shape) != (nb * C, n, S, S):
            raise ValueError(f"captured maps {tuple(maps.shape)}, expected {(nb * C, n, S, S)} (one controller)")
        yield i0, nb, maps.reshape(nb, C, n, S, S), T.theta_inverse().reshape(nb, C, 2, 3).to(device)
        del maps


KeypointScores = collections.namedtuple("KeypointScores", ["peak", "concentration", "coverage", "refined"])
KeypointPeaks = collections.namedtuple("KeypointPeaks", ["pos", "value"])


@torch.no_grad()
def predict_keypoints(ldm, images, context, indices, regressor=None, device="cuda", layers=(0, 1, 2, 3, 4, 5),
                      noise_level=-1, augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1),
                      augmentation_iterations=20, max_loc_strategy="argmax", controllers=None, upscale_size=512,
                      image_batch=None, return_maps=False, return_scores=False, score_distance=5, num_subjects=1):
    """Keypoints of a batch of unlabelled images (extra: the use the reference's demo ends in,
    ``visualize_keypoints``: TTA maps → ``find_max_pixel(map) / 512``, which draws the points and
    does not return them).

    ``images`` is (B, 3, H, W) in [0, 1] (a single (3, H, W) image is B = 1).  For image 0, then
    image 1, … ``augmentation_iterations`` thetas are drawn with ``draw_theta(1)`` — the order in
    which successive ``run_image_with_context_augmented`` calls would draw them.  The warped copies
    are captured per copy (``run_and_find_attn_per_image``), whole images' worth of copies per pass
    as ``AUG_BATCH_PIXELS`` allows (``image_batch`` overrides the images per pass; an image whose
    copies exceed the bound gets a pass of its own), and each pass is reduced by ``ops.tta_reduce``:
    inverse warps, sums in copy order, ratio, NaN → 0 and argmax in one kernel, without the
    full-size average in memory unless it is asked for.

    Returns the (B, n, 2) keypoints (row, col) = position / ``upscale_size``: the argmax, or with
    ``max_loc_strategy="weighted_avg"`` ``pixel_from_weighted_avg`` of the averages.  With a
    ``regressor`` (2n, 2K) also ``((p.reshape(B, -1) − 0.5) @ W + 0.5).reshape(B, -1, 2)``; with
    ``return_maps`` also the (B, n, S, S) averages.  More than one output comes as a tuple in that
    order.  With ``return_scores`` each pass is reduced by ``ops.tta_reduce_scored`` and a
    ``KeypointScores(peak, concentration, coverage, refined)`` comes last: per image and token the
    average's peak value, its mass within ``score_distance`` pixels of the peak over its whole mass,
    the share of the copies that saw the peak pixel (each (B, n)), and the
    ``pixel_from_weighted_avg`` centroid around the peak / ``upscale_size`` (B, n, 2); the other
    outputs are what they are without it.

    With ``num_subjects`` = k > 1 (images that show several instances of the object) each pass is
    reduced by ``ops.tta_reduce_peaks`` and a ``KeypointPeaks(pos, value)`` comes last: ``pos``
    (B, n, k, 2) holds per token the k peaks of ``find_k_max_pixels`` on the average (round j is
    the argmax after the discs of radius 0.05 · ``upscale_size`` around rounds 0 … j − 1 were
    multiplied by 0) / ``upscale_size``, ``value`` (B, n, k) the value that won each round.  The
    rounds are per token: round j of one token and round j of another need not belong to the same
    instance, and grouping the peaks into subjects is left to the caller.  So the first output stays
    (B, n, 2) (round 0, or the ``weighted_avg`` centroid) and the ``regressor`` is applied to it
    alone; ``return_maps`` gives the unmasked averages.  ``return_scores`` together with
    ``num_subjects`` > 1 raises: each needs its own reduce.  Single process only: under a process
    group of more than one rank it raises.

    Like ``correspond_images`` and ``part_maps``, the default images per pass also keep a pass's
    captured maps below 2^31 elements.  That splits only a default pass that the reduce refused
    ("maps of 2^31 elements or more"): every call that succeeded before runs the same passes.
    """
    if max_loc_strategy not in ("argmax", "weighted_avg"):
        raise ValueError("max_loc_strategy must be 'argmax' or 'weighted_avg'")
    k = int(num_subjects)
    if k < 1:
        raise ValueError("num_subjects must be at least 1")
    if k > 1 and return_scores:
        raise ValueError("return_scores and num_subjects > 1 each need their own reduce: ask for one of them")
    S, n = int(upscale_size), len(indices)
    weighted = max_loc_strategy == "weighted_avg"
    want_avg = weighted or return_maps
    pos, avgs, refs, scos, pks, vals = [], [], [], [], [], []
    for _, nb, maps, th_inv in _tta_passes("predict_keypoints", ldm, images, context, indices, device, layers,
                                           noise_level, augment_degrees, augment_scale, augment_translate,
                                           augmentation_iterations, controllers, S, image_batch):
        if return_scores:
            p, ref, sco, avg = ops.tta_reduce_scored(maps, th_inv, distance=score_distance, return_avg=want_avg)
            refs.append(ref)
            scos.append(sco)
        elif k > 1:
            pk, val, avg = ops.tta_reduce_peaks(maps, th_inv, k, return_avg=want_avg)
            p = pk[:, :, 0].contiguous()
            pks.append(pk)
            vals.append(val)
        else:
            p, avg = ops.tta_reduce(maps, th_inv, return_avg=want_avg)
        del maps
        if weighted:   # pixel_from_weighted_avg zeroes its input in place: the returned maps stay whole
            p = pixel_from_weighted_avg(avg.clone().reshape(nb * n, S, S) if return_maps else
                                        avg.reshape(nb * n, S, S)).reshape(nb, n, 2)
        pos.append(p)
        if return_maps:
            avgs.append(avg)
    kp = torch.cat(pos) / S
    B = kp.shape[0]
    out = [kp]
    if regressor is not None:
        W = regressor.to(kp.device, torch.float32)
        out.append(((kp.reshape(B, -1) - 0.5) @ W + 0.5).reshape(B, -1, 2))
    if return_maps:
        out.append(torch.cat(avgs))
    if return_scores:
        sco = torch.cat(scos)
        out.append(KeypointScores(sco[..., 0], sco[..., 1], sco[..., 2], torch.cat(refs) / S))
    if k > 1:
        out.append(KeypointPeaks(torch.cat(pks) / S, torch.cat(vals)))
    return out[0] if len(out) == 1 else tuple(out)


def _rank_ascending(keys, k):
    """The first ``k`` of a stable ascending argsort of (N,) float64 device keys, NaN last
    (skp_topk_keys): (k,) int64."""
    from ._lib import call, ptr, stream
    N = keys.shape[0]
    if N > 8192:
        raise ValueError(f"at most 8192 tokens can be ranked, got {N}")
    out = torch.empty(k, device=keys.device, dtype=torch.int64)
    if k > 0:
        call("skp_topk_keys", ptr(keys), 1, N, k, ptr(out), stream(keys.device))
    return out


def _sum_in_order(per_image):
    """(M, N) -> (N,): image 0's row, then image 1's added, and so on (a fixed order)."""
    total = per_image[0].clone()
    for i in range(1, per_image.shape[0]):
        total += per_image[i]
    return total


@torch.no_grad()
def find_corresponding_points(maps, num_points=10):
    """eval.py:159-195: the ``num_points`` tokens whose maps are jointly sharpest on these images.

    ``maps`` (num_images, num_tokens, h, w) on the device.  Per image and token the entropy of
    ``softmax(map)`` (``ops.entropy_keys_batch``: the reference's fp32 arithmetic, accumulated in
    double), summed over the images image by image; the tokens with the lowest sums, ascending, ties
    by index and NaN last (skp_topk_keys); ``find_max_pixel`` of each chosen map in every image.
    Returns ``(highest_indices (num_images, num_points, 2), indices (num_points,) int64)``; like the
    reference's slice, at most ``num_tokens`` points come back.
    """
    if maps.dim() != 4:
        raise ValueError(f"maps must be (num_images, num_tokens, h, w), got {tuple(maps.shape)}")
    M, N, h, w = maps.shape
    k = max(0, min(int(num_points), N))
    entropy = _sum_in_order(ops.entropy_keys_batch(maps))
    indices = _rank_ascending(entropy, k)
    chosen = maps[:, indices].contiguous()
    highest = find_max_pixel(chosen.view(M * k, h, w)) if k else maps.new_zeros(0, 2)
    return highest.reshape(M, k, 2), indices


Correspondences = collections.namedtuple("Correspondences", ["indices", "points", "entropy", "image_entropy"])


@torch.no_grad()
def correspond_images(ldm, images, context, num_points=10, candidates=None, device="cuda", layers=(0, 1, 2, 3, 4, 5),
                      noise_level=-1, augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1),
                      augmentation_iterations=20, controllers=None, upscale_size=128, entropy_scale=1.0,
                      image_batch=None):
    """Which tokens of ``context`` are jointly sharp on these unlabelled images, and where (extra:
    ``find_corresponding_points``, eval.py:159-195, on the TTA averages of eval.py:327-355, without
    the averages in memory).

    ``images`` is (M, 3, H, W) in [0, 1].  The thetas are drawn as ``predict_keypoints`` draws them
    (image 0's ``augmentation_iterations`` draws, then image 1's, …), every pass of whole images'
    copies is captured by ``run_and_find_attn_per_image`` for the ``candidates`` (token ids; default
    every token of ``context``) at ``upscale_size`` and reduced by ``ops.tta_reduce_entropy``: the
    argmax of each candidate's average and the entropy of ``softmax(entropy_scale · average)`` in
    one pass.  Images per pass: what ``AUG_BATCH_PIXELS`` allows and what keeps the captured maps
    below 2^31 elements, or ``image_batch``.  The entropies are summed over the images image by
    image, in order, and ranked ascending (ties by position among the candidates, NaN last).

    Returns ``Correspondences(indices, points, entropy, image_entropy)``: ``indices`` (k,) int64 the
    ids of the k = min(``num_points``, candidates) tokens with the lowest summed entropy, ``points``
    (M, k, 2) their (row, col) = position / ``upscale_size`` in every image, ``entropy`` (n_cand,)
    float64 the sums and ``image_entropy`` (M, n_cand) float64, both in candidate order.  Single
    process only: under a process group of more than one rank it raises.
    """
    C, S = int(augmentation_iterations), int(upscale_size)
    if S < 2:
        raise ValueError("upscale_size must be at least 2")
    if candidates is None:
        candidates = torch.arange(context.shape[-2])
    candidates = torch.as_tensor(candidates, dtype=torch.int64).reshape(-1).cpu()
    n = len(candidates)
    if n < 1:
        raise ValueError("at least one candidate token is needed")
    if C * n * S * S >= 2 ** 31:
        raise ValueError(f"one image's captured maps ({C} x {n} x {S} x {S}) reach 2^31 elements: rank fewer "
                         "candidates at a time or lower upscale_size")
    k = max(0, min(int(num_points), n))
    pos, ents = [], []
    for _, _, maps, th_inv in _tta_passes("correspond_images", ldm, images, context, candidates, device, layers,
                                          noise_level, augment_degrees, augment_scale, augment_translate, C,
                                          controllers, S, image_batch):
        p, e, _ = ops.tta_reduce_entropy(maps, th_inv, scale=entropy_scale)
        del maps
        pos.append(p)
        ents.append(e)
    if not pos:
        raise ValueError("at least one image is needed")
    image_entropy = torch.cat(ents)
    entropy = _sum_in_order(image_entropy)
    order = _rank_ascending(entropy, k)
    points = torch.cat(pos)[:, order] / S
    return Correspondences(candidates.to(order.device)[order], points, entropy, image_entropy)


PartMaps = collections.namedtuple("PartMaps", ["label", "value", "mass", "points", "area"])


@torch.no_grad()
def part_maps(ldm, images, context, indices=None, device="cuda", layers=(0, 1, 2, 3, 4, 5), noise_level=-1,
              augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), augmentation_iterations=20,
              controllers=None, upscale_size=128, part_threshold=0.0, image_batch=None):
    """Which of the chosen tokens owns each pixel of these unlabelled images (extra: the unsupervised
    part label; the captured maps are a softmax over the tokens at every pixel, so at a pixel the
    tokens' TTA averages of eval.py:327-355 are comparable), without the averages in memory.

    ``images`` is (M, 3, H, W) in [0, 1].  The thetas are drawn as ``predict_keypoints`` draws them
    (image 0's ``augmentation_iterations`` draws, then image 1's, …), every pass of whole images'
    copies is captured by ``run_and_find_attn_per_image`` for ``indices`` (token ids; default every
    token of ``context``) at ``upscale_size`` and reduced by one ``ops.tta_reduce_parts``: each
    token's argmax and, per pixel, the greatest average, the lowest token that attains it and the
    tokens' sum.  Images per pass: what ``AUG_BATCH_PIXELS`` allows and what keeps the captured maps
    below 2^31 elements, or ``image_batch``.

    Returns ``PartMaps(label, value, mass, points, area)``: ``label`` (M, S, S) int16 the position
    among ``indices`` of the token that owns the pixel, −1 (background) where ``mass <=
    part_threshold`` — with the default exactly the pixels that carry no attention, those that no
    copy covers among them; ``value`` and ``mass`` (M, S, S) the owner's average and the tokens'
    sum as the kernel left them; ``points`` (M, n, 2) each token's (row, col) = position /
    ``upscale_size``, ``predict_keypoints``' keypoints; ``area`` (M, n) int64 the pixels each token
    owns.  Single process only: under a process group of more than one rank it raises.
    """
    C, S = int(augmentation_iterations), int(upscale_size)
    if S < 2:
        raise ValueError("upscale_size must be at least 2")
    if indices is None:
        indices = torch.arange(context.shape[-2])
    indices = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
    n = len(indices)
    if n < 1:
        raise ValueError("at least one token is needed")
    if n > 32767:
        raise ValueError(f"at most 32767 tokens can be labelled (the label is int16), got {n}")
    if C * n * S * S >= 2 ** 31:
        raise ValueError(f"one image's captured maps ({C} x {n} x {S} x {S}) reach 2^31 elements: label fewer "
                         "tokens at a time or lower upscale_size")
    pos, labels, values, masses = [], [], [], []
    for _, _, maps, th_inv in _tta_passes("part_maps", ldm, images, context, indices, device, layers, noise_level,
                                          augment_degrees, augment_scale, augment_translate, C, controllers, S,
                                          image_batch):
        p, lab, val, mas, _ = ops.tta_reduce_parts(maps, th_inv)
        del maps
        pos.append(p)
        labels.append(lab)
        values.append(val)
        masses.append(mas)
    if not pos:
        raise ValueError("at least one image is needed")
    mass = torch.cat(masses)
    M = mass.shape[0]
    label = torch.cat(labels).masked_fill(mass <= float(part_threshold), -1)
    # the pixels of each label, the background in column 0 (integer adds: any order gives the same counts)
    owner = (label.long() + 1).reshape(M, S * S)
    area = torch.zeros(M, n + 1, device=owner.device, dtype=torch.int64).scatter_add_(1, owner, torch.ones_like(owner))
    return PartMaps(label, torch.cat(values), mass, torch.cat(pos) / S, area[:, 1:].contiguous())


def foreground_iou(label, mask):
    """Per-image intersection over union of the labelled pixels against a foreground mask.

    ``label`` (M, S, S): a pixel is foreground where ``label >= 0`` (``part_maps``' background is
    −1).  ``mask`` (M, h, w) or (M, h, w, 1) in [0, 1] (the CUB parts reader's ``mask``), resized to
    (S, S) by nearest neighbour when its size differs; foreground where ``mask > 0.5``.  Returns
    (M,) float64 on ``label``'s device: |A ∩ B| / |A ∪ B|, and 1.0 where both are empty.
    """
    label = torch.as_tensor(label)
    mask = torch.as_tensor(mask).to(label.device)
    if mask.dim() == 4 and mask.shape[-1] == 1:
        mask = mask[..., 0]
    if label.dim() != 3 or mask.dim() != 3 or mask.shape[0] != label.shape[0]:
        raise ValueError(f"label must be (M, S, S) and mask (M, h, w) or (M, h, w, 1), got {tuple(label.shape)} "
                         f"and {tuple(mask.shape)}")
    if tuple(mask.shape[1:]) != tuple(label.shape[1:]):
        mask = torch.nn.functional.interpolate(mask[:, None].to(torch.float32), size=tuple(label.shape[1:]),
                                               mode="nearest")[:, 0]
    fg, gt = label >= 0, mask > 0.5
    inter = (fg & gt).flatten(1).sum(1).to(torch.float64)
    union = (fg | gt).flatten(1).sum(1).to(torch.float64)
    return torch.where(union > 0, inter / union.clamp_min(1.0), torch.ones_like(union))


def _tokens_of(indices, context, C, S, what):
    """``indices`` (default every token of ``context``) as (n,) int64 on the CPU, after the checks
    ``part_maps`` makes of the shapes."""
    if S < 2:
        raise ValueError("upscale_size must be at least 2")
    if indices is None:
        indices = torch.arange(context.shape[-2])
    indices = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
    n = len(indices)
    if n < 1:
        raise ValueError("at least one token is needed")
    if C * n * S * S >= 2 ** 31:
        raise ValueError(f"one image's captured maps ({C} x {n} x {S} x {S}) reach 2^31 elements: {what} fewer "
                         "tokens at a time or lower upscale_size")
    return indices


@torch.no_grad()
def describe_points(ldm, images, points, context, indices=None, device="cuda", layers=(0, 1, 2, 3, 4, 5),
                    noise_level=-1, augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1),
                    augmentation_iterations=20, controllers=None, upscale_size=128, image_batch=None):
    """Descriptors of landmarks annotated on a few exemplar images (extra: the captured maps are a
    softmax over the tokens at every pixel, so the n tokens' TTA averages of eval.py:327-355 at a
    pixel are a signature of what is there).

    ``images`` is (K, 3, H, W) in [0, 1], the exemplars; ``points`` (K, Q, 2) holds landmark j's
    (row, col) in [0, 1] on each of them, NaN where it is not annotated on that exemplar.  The
    thetas are drawn as ``predict_keypoints`` draws them, every pass is captured for ``indices``
    (token ids; default every token of ``context``) at ``upscale_size`` = S and reduced by
    ``ops.tta_reduce(..., return_avg=True)`` (the exemplars are few: their averages may be in memory).
    An annotation reads the pixel ``clamp(floor(point · S), 0, S − 1)``; the n averages there, in
    float64, are scaled to unit length (a zero or non-finite vector contributes nothing).  A
    landmark's descriptor is the sum of its exemplars' unit vectors in exemplar order, scaled to
    unit length again.  Returns the (Q, n) float32 descriptors on ``device``, what
    ``transfer_keypoints`` takes.  A landmark without any contribution raises ``ValueError``.
    Single process only: under a process group of more than one rank it raises.
    """
    C, S = int(augmentation_iterations), int(upscale_size)
    indices = _tokens_of(indices, context, C, S, "describe with")
    pts = torch.as_tensor(points, dtype=torch.float64).cpu()
    K = images.shape[0] if torch.as_tensor(images).dim() == 4 else 1
    if pts.dim() != 3 or pts.shape[0] != K or pts.shape[2] != 2:
        raise ValueError(f"points must be ({K}, Q, 2), got {tuple(pts.shape)}")
    Q, n = pts.shape[1], len(indices)
    if Q < 1:
        raise ValueError("at least one landmark is needed")
    annotated = ~torch.isnan(pts).any(dim=-1)                                   # (K, Q)
    pixel = torch.nan_to_num(torch.floor(pts * S), nan=0.0).clamp(0, S - 1).long()
    total = torch.zeros(Q, n, dtype=torch.float64)
    for i0, nb, maps, th_inv in _tta_passes("describe_points", ldm, images, context, indices, device, layers,
                                            noise_level, augment_degrees, augment_scale, augment_translate, C,
                                            controllers, S, image_batch):
        _, avg = ops.tta_reduce(maps, th_inv, return_avg=True)
        del maps
        for k in range(nb):             # exemplar order
            rows, cols = pixel[i0 + k, :, 0].to(avg.device), pixel[i0 + k, :, 1].to(avg.device)
            sig = avg[k][:, rows, cols].T.to(torch.float64).cpu()               # (Q, n)
            length = (sig * sig).sum(dim=1).sqrt()
            use = annotated[i0 + k] & torch.isfinite(length) & (length > 0)
            unit = sig / torch.where(use, length, torch.ones_like(length))[:, None]
            total += torch.where(use[:, None], unit, torch.zeros_like(unit))
    length = (total * total).sum(dim=1).sqrt()
    empty = [j for j in range(Q) if not (bool(torch.isfinite(length[j])) and float(length[j]) > 0)]
    if empty:
        raise ValueError(f"describe_points: landmark(s) {empty} have no descriptor: not annotated on any exemplar, "
                         "or only at pixels whose signature is zero or not finite")
    return (total / length[:, None]).to(torch.float32).to(device)


Transferred = collections.namedtuple("Transferred", ["points", "score", "token_points", "score_maps"])
MATCH_QUERIES = 16      # landmarks per ops.tta_reduce_match call


@torch.no_grad()
def transfer_keypoints(ldm, images, context, descriptors, indices=None, device="cuda", layers=(0, 1, 2, 3, 4, 5),
                       noise_level=-1, augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1),
                       augmentation_iterations=20, controllers=None, upscale_size=128, return_score_maps=False,
                       image_batch=None):
    """Where the landmarks of ``describe_points`` are in these unlabelled images (extra: few-shot
    annotation transfer, without a regressor, a labelled set or the averages in memory).

    ``images`` is (M, 3, H, W) in [0, 1]; ``descriptors`` (Q, n) are ``describe_points``' for the same
    ``indices`` (token ids; default every token of ``context``) and ``upscale_size`` = S.  The thetas
    are drawn as ``predict_keypoints`` draws them, and every pass is reduced by
    ``ops.tta_reduce_match``: per image and landmark the pixel whose signature has the greatest
    cosine with the descriptor.  More than 16 landmarks run in groups of 16, one call per group on
    the same pass's maps.  Images per pass: what ``AUG_BATCH_PIXELS`` allows and what keeps the
    captured maps below 2^31 elements, or ``image_batch``.

    Returns ``Transferred(points, score, token_points, score_maps)``: ``points`` (M, Q, 2) the
    landmarks' (row, col) = position / S, ``score`` (M, Q) their cosine (−inf where no pixel of the
    image has a usable signature; the point is then (0.5, 0.5) / S), ``token_points`` (M, n, 2)
    ``predict_keypoints``' points of those tokens, and ``score_maps`` (M, Q, S, S) every pixel's
    score when ``return_score_maps``, else None.  Single process only: under a process group of more
    than one rank it raises.
    """
    C, S = int(augmentation_iterations), int(upscale_size)
    indices = _tokens_of(indices, context, C, S, "match")
    n = len(indices)
    desc = torch.as_tensor(descriptors, dtype=torch.float32)
    if desc.dim() != 2 or desc.shape[0] < 1 or desc.shape[1] != n:
        raise ValueError(f"descriptors must be (Q, {n}) with Q >= 1, got {tuple(desc.shape)}")
    desc = desc.to(device).contiguous()
    groups = [desc[g:g + MATCH_QUERIES] for g in range(0, desc.shape[0], MATCH_QUERIES)]
    pos, points, scores, score_maps = [], [], [], []
    for _, _, maps, th_inv in _tta_passes("transfer_keypoints", ldm, images, context, indices, device, layers,
                                          noise_level, augment_degrees, augment_scale, augment_translate, C,
                                          controllers, S, image_batch):
        got = [ops.tta_reduce_match(maps, th_inv, d, return_scores=return_score_maps) for d in groups]
        del maps
        pos.append(got[0][0])
        points.append(torch.cat([g[1] for g in got], dim=1))
        scores.append(torch.cat([g[2] for g in got], dim=1))
        if return_score_maps:
            score_maps.append(torch.cat([g[3] for g in got], dim=1))
    if not pos:
        raise ValueError("at least one image is needed")
    return Transferred(torch.cat(points) / S, torch.cat(scores), torch.cat(pos) / S,
                       torch.cat(score_maps) if return_score_maps else None)


DenseMatch = collections.namedtuple("DenseMatch", ["index", "score", "back_index", "back_score", "cycle",
                                                   "token_points"])


def _cycle_distance(index, back_index, S):
    """(M, S²) forward and backward fields -> (M, S²) float32 distance in pixels between p and
    ``back_index[index[p]]``, +inf where either index is −1."""
    hop = torch.gather(back_index.long(), 1, index.long().clamp_min(0))
    p = torch.arange(S * S, device=index.device)[None]
    dr, dc = p // S - hop.clamp_min(0) // S, p % S - hop.clamp_min(0) % S
    dist = (dr * dr + dc * dc).to(torch.float64).sqrt().to(torch.float32)
    return dist.masked_fill((index < 0) | (hop < 0), float("inf"))


@torch.no_grad()
def match_images(ldm, source, images, context, indices=None, device="cuda", layers=(0, 1, 2, 3, 4, 5),
                 noise_level=-1, augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1),
                 augmentation_iterations=20, controllers=None, upscale_size=128, image_batch=None, coarse_size=None,
                 refine_radius=None):
    """The dense field between one source image and unlabelled images (extra: everything an exemplar
    carries — a mask, a part segmentation, any number of points — transfers through one operation: for
    every pixel of one image the pixel of the other whose signature, the n tokens' TTA averages, has
    the greatest cosine).

    ``source`` is (3, H, W) and ``images`` (M, 3, H, W), in [0, 1].  The source's
    ``augmentation_iterations`` thetas are drawn first, then the images' as ``predict_keypoints`` draws
    them; every pass is reduced by ``ops.tta_reduce(..., return_avg=True)`` and the source's averages
    are kept for the whole call.  Per pass two ``ops.match_field`` calls: the images' pixels against
    the source's, and the source's pixels against each image's.

    ``coarse_size=Sc`` matches coarse to fine instead: Sc divides S by f = S / Sc in [2, 8]; the passes and
    the draws are the same.  The coarse signatures are ``avg_pool2d(avg, f)`` of the fine averages, of
    the source and of the images; the coarse fields come from ``ops.match_field`` on them, in both
    directions, and the fine fields from ``ops.match_refine``, which matches every pixel inside a window
    of ``refine_radius`` pixels (default f + 1, at most 16: a correct coarse match places the window's
    centre within f of the true match on each axis) around its cell's coarse match.  The result is at
    S, ``cycle`` on the fine fields; a fine pixel whose cell has no coarse match gets −1 and −inf.  How
    well refined fields agree with brute-force ones on real images has not been measured.

    Returns ``DenseMatch(index, score, back_index, back_score, cycle, token_points)``, the first five
    (M, S, S) with S = ``upscale_size``: ``index`` int32 the source pixel (row · S + col) matched to
    each image pixel and ``score`` its cosine, −1 and −inf where the pixel's signature is not usable
    (a pixel no copy covers) or no source pixel's is; ``back_index`` / ``back_score`` the image pixel
    matched to each SOURCE pixel; ``cycle`` float32 the distance in pixels between p and
    ``back_index[index[p]]``, +inf where either index is −1; ``token_points`` (M, n, 2)
    ``predict_keypoints``' points of those tokens.  Single process only: under a process group of
    more than one rank it raises.
    """
    C, S = int(augmentation_iterations), int(upscale_size)
    indices = _tokens_of(indices, context, C, S, "match")
    n = len(indices)
    src = torch.as_tensor(source)
    if src.dim() != 3 or src.shape[0] != 3:
        raise ValueError(f"source must be (3, H, W), got {tuple(src.shape)}")
    f = w = None
    if coarse_size is not None:
        Sc = int(coarse_size)
        if Sc < 1 or S % Sc != 0 or not 2 <= S // Sc <= 8:
            raise ValueError(f"coarse_size must divide upscale_size = {S} by a factor in [2, 8], got {coarse_size}")
        f = S // Sc
        w = f + 1 if refine_radius is None else int(refine_radius)
        if not 1 <= w <= 16:
            raise ValueError(f"refine_radius must be in [1, 16], got {w}")
    elif refine_radius is not None:
        raise ValueError("refine_radius belongs to coarse_size")

    def both_ways(avg, nb):
        """(index, score, back_index, back_score), each (nb, S²), of ``avg`` (nb, n, S, S) and the source."""
        if f is None:
            sig = avg.reshape(nb, n, S * S)
            return ops.match_field(sig, src_sig) + ops.match_field(src_sig, sig)
        low = torch.nn.functional.avg_pool2d(avg, f).contiguous()
        there, _ = ops.match_field(low.reshape(nb, n, Sc * Sc), src_low.reshape(1, n, Sc * Sc))
        back, _ = ops.match_field(src_low.reshape(1, n, Sc * Sc), low.reshape(nb, n, Sc * Sc))
        got = (ops.match_refine(avg, src_avg, there.reshape(nb, Sc, Sc), w)
               + ops.match_refine(src_avg, avg, back.reshape(nb, Sc, Sc), w))
        return tuple(t.reshape(nb, S * S) for t in got)

    common = (noise_level, augment_degrees, augment_scale, augment_translate, C, controllers, S)
    src_avg = None
    for _, _, maps, th_inv in _tta_passes("match_images", ldm, src, context, indices, device, layers, *common, 1):
        _, src_avg = ops.tta_reduce(maps, th_inv, return_avg=True)
        del maps
    src_sig = src_avg.reshape(1, n, S * S)
    src_low = None if f is None else torch.nn.functional.avg_pool2d(src_avg, f).contiguous()
    pos, fields = [], ([], [], [], [])
    for _, nb, maps, th_inv in _tta_passes("match_images", ldm, images, context, indices, device, layers, *common,
                                           image_batch):
        p, avg = ops.tta_reduce(maps, th_inv, return_avg=True)
        del maps
        got = both_ways(avg.reshape(nb, n, S, S), nb)
        del avg
        pos.append(p)
        for acc, t in zip(fields, got):
            acc.append(t)
    if not pos:
        raise ValueError("at least one image is needed")
    index, score, back_index, back_score = (torch.cat(f) for f in fields)
    M = index.shape[0]
    cycle = _cycle_distance(index, back_index, S)
    return DenseMatch(*(t.reshape(M, S, S) for t in (index, score, back_index, back_score, cycle)),
                      torch.cat(pos) / S)


def transfer_labels(match, labels, max_cycle=None, min_score=None):
    """The source's labels carried to every image of a ``DenseMatch``.

    ``labels`` is (S, S) integer on the source's grid, −1 for unlabelled and at most 32767.  Returns
    (M, S, S) int16: the label of the matched source pixel, and −1 where ``index`` is −1, where
    ``cycle > max_cycle`` or where ``score < min_score`` (each gate only where it is given).
    """
    index = torch.as_tensor(match.index)
    M, S = index.shape[0], index.shape[-1]
    lab = torch.as_tensor(labels)
    if lab.is_floating_point() or lab.dtype == torch.bool or tuple(lab.shape) != (S, S):
        raise ValueError(f"labels must be ({S}, {S}) integer, got {tuple(lab.shape)} {lab.dtype}")
    if lab.numel() and (int(lab.min()) < -1 or int(lab.max()) > 32767):
        raise ValueError("labels must lie in [-1, 32767]")
    lab = lab.to(index.device, torch.int16).reshape(-1)
    keep = index >= 0
    if max_cycle is not None:
        keep &= ~(torch.as_tensor(match.cycle).to(index.device) > float(max_cycle))
    if min_score is not None:
        keep &= ~(torch.as_tensor(match.score).to(index.device) < float(min_score))
    out = lab[index.long().clamp_min(0).reshape(-1)].reshape(M, S, S)
    return torch.where(keep, out, torch.full_like(out, -1))


def transfer_points_dense(match, points):
    """Points annotated on the source, read off a ``DenseMatch``'s backward field.

    ``points`` is (Q, 2) (row, col) in [0, 1] on the source, NaN where not annotated; Q is not
    limited.  A point reads the source pixel ``clamp(floor(point · S), 0, S − 1)``.  Returns
    ``(positions (M, Q, 2), scores (M, Q))``: the matched image pixel's (row, col) / S and its cosine
    from ``back_index`` and ``back_score``; NaN and −inf for a NaN point, and for a source pixel
    without a match (``back_index`` −1).
    """
    back = torch.as_tensor(match.back_index)
    M, S = back.shape[0], back.shape[-1]
    dev = back.device
    pts = torch.as_tensor(points, dtype=torch.float64)
    if pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError(f"points must be (Q, 2), got {tuple(pts.shape)}")
    pts = pts.to(dev)
    annotated = ~torch.isnan(pts).any(dim=-1)
    pixel = torch.nan_to_num(torch.floor(pts * S), nan=0.0).clamp(0, S - 1).long()
    flat = pixel[:, 0] * S + pixel[:, 1]                                          # (Q,)
    hit = back.reshape(M, S * S)[:, flat].long()                                  # (M, Q)
    sc = torch.as_tensor(match.back_score).to(dev).reshape(M, S * S)[:, flat]
    ok = annotated[None] & (hit >= 0)
    pos = torch.stack([hit.clamp_min(0) // S, hit.clamp_min(0) % S], dim=-1).to(torch.float32) / S
    pos = torch.where(ok[..., None], pos, torch.full_like(pos, float("nan")))
    return pos, torch.where(ok, sc, torch.full_like(sc, float("-inf")))


KeypointTracks = collections.namedtuple("KeypointTracks", ["pos", "support", "independent"])


class _Tracker:
    """The frames of one sequence, one ``push`` per frame in order, then ``finish``.  Holds the int16
    back-pointers of every frame (one (T, n, S, S) stack where the frame count is known beforehand, else
    a plane per frame that ``finish`` stacks), the last frame's state and, while a step runs, the new
    score plane beside the previous one; per frame besides that only each token's own argmax and peak."""

    def __init__(self, weights, device, frames=None):
        self.w, self.r, self.device = weights, weights.numel() - 1, torch.device(device)
        self.T, self.t, self.state, self.stack, self.backs, self.own, self.peak = frames, 0, None, None, [], [], []

    def push(self, frame):
        a = torch.as_tensor(frame)
        if a.dim() != 3 or a.shape[-1] != a.shape[-2]:
            raise ValueError(f"a frame must be (n, S, S), got {tuple(a.shape)}")
        a = a.to(self.device, torch.float32).contiguous()
        if self.t == 0:
            self.n, self.S = a.shape[0], a.shape[-1]
            if self.T is not None:
                self.stack = torch.empty(self.T, self.n, self.S, self.S, device=self.device, dtype=torch.int16)
        elif tuple(a.shape) != (self.n, self.S, self.S):
            raise ValueError(f"frame {self.t} is {tuple(a.shape)}, frame 0 was {(self.n, self.S, self.S)}")
        if self.stack is not None and self.t >= self.T:
            raise ValueError(f"more than the {self.T} frames announced")
        self.state = ops.track_step(a, self.state, self.w, back=None if self.stack is None else self.stack[self.t])
        if self.stack is None:
            self.backs.append(self.state[3])
        own = ops.argmax_index(a)
        self.own.append(own)
        self.peak.append(a.reshape(self.n, -1).gather(1, own[:, None])[:, 0])
        self.t += 1

    def finish(self, frames):
        """``frames``: the pushed frames once more, in order (a (T, n, S, S) tensor or an iterable of
        (n, S, S) frames, on any device): only the tracked pixel of each plane is read."""
        if self.t < 1:
            raise ValueError("at least one frame is needed")
        if self.stack is not None and self.t != self.T:
            raise ValueError(f"{self.t} frames came, {self.T} were announced")
        T, n, S = self.t, self.n, self.S
        stack = self.stack if self.stack is not None else torch.stack(self.backs)
        self.backs = []
        pos = ops.track_backtrace(stack, self.state[2], self.r)               # (T, n, 2), pixel centres
        flat = pos[..., 0].long() * S + pos[..., 1].long()                    # (T, n)
        if torch.is_tensor(frames):
            at = frames.reshape(T, n, S * S).gather(2, flat.to(frames.device)[..., None])[..., 0]
        else:
            flat_cpu, at = flat.cpu(), []
            for t, f in enumerate(frames):
                f = torch.as_tensor(f).reshape(n, S * S)
                at.append(f.gather(1, (flat[t] if f.is_cuda else flat_cpu[t])[:, None])[:, 0].to(self.device))
            at = torch.stack(at)
        # the three quotients on the host: one IEEE division each, whatever device the frames were on
        at, peak = at.to(torch.float32).cpu(), torch.stack(self.peak).cpu()
        live = (peak != 0) & torch.isfinite(peak)
        support = torch.where(live, at / torch.where(live, peak, torch.ones_like(peak)), torch.zeros_like(at))
        own = torch.stack(self.own).cpu()
        independent = torch.stack([own // S, own % S], dim=-1).to(torch.float32) + 0.5
        size = torch.tensor(float(S))
        return KeypointTracks((pos.cpu() / size).to(self.device), support.to(self.device),
                              (independent / size).to(self.device))


@torch.no_grad()
def track_keypoints(maps, sigma=2.0, radius=None, device="cuda"):
    """Keypoint tracks over a video from its per-frame TTA averages (extra: ``visualize.create_vid``
    takes ``find_max_pixel`` frame by frame, and a per-frame argmax jumps whenever a second mode of a
    token's map briefly wins).  Per token the track is the MAP path of a hidden Markov model over the
    pixel grid: the emission is the frame's average, the transition a Gaussian random walk of
    ``sigma`` pixels truncated at ``radius`` (``ops.track_weights``; default ``ceil(3·sigma)`` clipped
    to [1, 32]).  Exact Viterbi, one ``ops.track_step`` per frame and one ``ops.track_backtrace``.

    ``maps`` is a (T, n, S, S) tensor or any iterable of (n, S, S) frames in frame order: what
    ``predict_keypoints(return_maps=True)`` returns, or the list that ``create_vid`` saved in
    ``saved_maps.pt``.  CPU frames are uploaded to ``device`` one at a time (a tensor on a HIP device
    stays where it is); an iterable without a length is first made a list.  Only the int16
    back-pointers of all frames and two score planes are held besides the caller's frames, which are
    read once more at the tracked pixels.

    Returns ``KeypointTracks(pos, support, independent)``: ``pos`` (T, n, 2) the track's (row, col) =
    position / S; ``support`` (T, n) the frame's average at the tracked pixel over that average's
    maximum, 1 where the track agrees with the frame's own peak and 0 where the plane is blank;
    ``independent`` (T, n, 2) the per-frame argmax / S, for comparison.  Planes that hold NaN, an
    infinity or a negative value give that token unspecified tracks.
    """
    weights = ops.track_weights(sigma, radius)
    if torch.is_tensor(maps):
        if maps.dim() != 4:
            raise ValueError(f"maps must be (T, n, S, S) or an iterable of (n, S, S) frames, got {tuple(maps.shape)}")
        if maps.is_cuda:
            device = maps.device
    elif not hasattr(maps, "__len__"):
        maps = list(maps)
    if len(maps) < 1:
        raise ValueError("at least one frame is needed")
    tracker = _Tracker(weights, device, len(maps))
    for frame in maps:
        tracker.push(frame)
    return tracker.finish(maps)


@torch.no_grad()
def track_images(ldm, images, context, indices, device="cuda", layers=(0, 1, 2, 3, 4, 5), noise_level=-1,
                 augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), augmentation_iterations=20,
                 controllers=None, upscale_size=128, image_batch=None, sigma=2.0, radius=None):
    """``track_keypoints`` of the frames of a video: ``images`` (T, 3, H, W) in [0, 1], in frame order.

    The thetas are drawn and the passes captured as ``predict_keypoints`` does (``_tta_passes``); each
    pass's averages, from ``ops.tta_reduce(return_avg=True)``, are fed to the tracker frame by frame as
    they come and then kept on the host for the read at the tracked pixels, so no more than one pass
    of captured maps and one pass of averages is on the device at a time.  The result is what
    ``track_keypoints`` gives on ``predict_keypoints(..., return_maps=True)``'s maps from the same
    seed, bit for bit.  Single process only: under a process group of more than one rank it raises.
    """
    C, S = int(augmentation_iterations), int(upscale_size)
    indices = _tokens_of(indices, context, C, S, "track")
    weights = ops.track_weights(sigma, radius)
    imgs = torch.as_tensor(images)
    tracker = _Tracker(weights, device, imgs.shape[0] if imgs.dim() == 4 else 1)
    kept = []
    for _, nb, maps, th_inv in _tta_passes("track_images", ldm, imgs, context, indices, device, layers, noise_level,
                                           augment_degrees, augment_scale, augment_translate, C, controllers, S,
                                           image_batch):
        _, avg = ops.tta_reduce(maps, th_inv, return_avg=True)
        del maps
        for b in range(nb):
            tracker.push(avg[b])
        kept.append(avg.cpu())
        del avg
    return tracker.finish([f for a in kept for f in a])


PropagatedLabels = collections.namedtuple("PropagatedLabels", ["label", "confidence", "soft"])


class _Propagator:
    """The frames of one sequence, one ``push`` per frame in order, then ``finish``.  Keeps on the device
    the signatures and soft labels of frame 0 and of the last ``memory`` frames, nothing else of the
    sequence; every frame's label and confidence (and its soft map, where asked for) wait on the host."""

    def __init__(self, labels0, radius, k, tau, memory, device, keep_soft):
        self.w, self.k, self.tau, self.memory = int(radius), int(k), float(tau), int(memory)
        if not 1 <= self.w <= 16:
            raise ValueError(f"radius must be in [1, 16], got {radius}")
        if not 1 <= self.k <= 16:
            raise ValueError(f"k must be in [1, 16], got {k}")
        if not 0.0 < self.tau < float("inf"):
            raise ValueError(f"tau must be positive and finite, got {tau}")
        if self.memory < 0 or self.memory + 1 > 64:
            raise ValueError(f"memory must be in [0, 63], got {memory}")
        lab = torch.as_tensor(labels0)
        if lab.dim() == 2 and not lab.is_floating_point() and lab.dtype != torch.bool:
            if lab.shape[0] != lab.shape[1]:
                raise ValueError(f"labels0 must be (S, S) integers or (Cl, S, S) floating point, got {tuple(lab.shape)}")
            if lab.numel() and int(lab.min()) < -1:
                raise ValueError("integer labels0 must be at least -1 (-1: the pixel casts no vote)")
            Cl = max(int(lab.max()) + 1, 1) if lab.numel() else 1
            soft = (lab[None] == torch.arange(Cl, device=lab.device)[:, None, None]).to(torch.float32)
            label, conf = lab.to(torch.int32), (lab >= 0).to(torch.float32)
        elif lab.dim() == 3 and lab.is_floating_point() and lab.shape[1] == lab.shape[2]:
            soft = lab.to(torch.float32)
            if not bool(torch.isfinite(soft).all()) or bool((soft < 0).any()):
                raise ValueError("a soft labels0 must be finite and non-negative")
            conf, label = soft.max(dim=0)       # the lowest class among equal maxima
            label = label.to(torch.int32)
        else:
            raise ValueError(f"labels0 must be (S, S) integers or (Cl, S, S) floating point, got {tuple(lab.shape)} "
                             f"{lab.dtype}")
        if not 1 <= soft.shape[0] <= 256:
            raise ValueError(f"labels0 has {soft.shape[0]} classes; at most 256")
        self.device, self.keep_soft = torch.device(device), keep_soft
        self.S, self.t, self.n = soft.shape[-1], 0, None
        self.first = soft.to(self.device).contiguous()
        self.context = []            # (frame number, signatures (n, S, S), soft labels (Cl, S, S)) in frame order
        self.labels, self.confs, self.softs = [label.cpu()], [conf.cpu()], [soft.cpu()] if keep_soft else []

    def push(self, frame):
        a = torch.as_tensor(frame)
        if a.dim() != 3 or tuple(a.shape[1:]) != (self.S, self.S):
            raise ValueError(f"frame {self.t} must be (n, {self.S}, {self.S}) like labels0, got {tuple(a.shape)}")
        a = a.to(self.device, torch.float32).contiguous()
        if a.untyped_storage().nbytes() > a.numel() * a.element_size():
            a = a.clone()        # a slice of a pass or of the whole video: the context must not keep that alive
        if self.t == 0:
            self.n = a.shape[0]
            soft = self.first
        else:
            if a.shape[0] != self.n:
                raise ValueError(f"frame {self.t} has {a.shape[0]} tokens, frame 0 had {self.n}")
            index, score = ops.match_topk(a[None], torch.stack([c[1] for c in self.context]), self.w, self.k)
            soft, label, conf = ops.label_vote(index, score, torch.stack([c[2] for c in self.context]), self.tau)
            self.labels.append(label.cpu())
            self.confs.append(conf.cpu())
            if self.keep_soft:
                self.softs.append(soft.cpu())
        # frame 0 and the last `memory` frames, in frame order
        self.context = [c for c in self.context if c[0] == 0 or c[0] > self.t - self.memory]
        if self.t == 0 or self.memory > 0:
            self.context.append((self.t, a, soft))
        self.t += 1

    def finish(self):
        if self.t < 1:
            raise ValueError("at least one frame is needed")
        return PropagatedLabels(torch.stack(self.labels).to(self.device), torch.stack(self.confs).to(self.device),
                                torch.stack(self.softs).to(self.device) if self.keep_soft else None)


@torch.no_grad()
def propagate_labels(signatures, labels0, radius=8, k=5, tau=0.07, memory=2, device="cuda", return_soft=False):
    """A mask or part segmentation of a video's first frame carried through the remaining frames (extra:
    the label-propagation protocol that dense self-supervised features are judged by).  For every pixel
    of frame t the ``k`` most similar pixels within ``radius`` of it in each context frame are found
    (``ops.match_topk``, the signatures' cosines); the ``k`` best of them all, weighted by
    ``softmax(cosine / tau)``, vote with their own soft labels (``ops.label_vote``).  The context of
    frame t is frame 0 and the last ``memory`` frames, distinct and in frame order; frame 0 keeps its
    given labels, and each later frame's soft output is its label map for the frames after it.

    ``signatures`` is a (T, n, S, S) tensor or any iterable of (n, S, S) frames in frame order: what
    ``predict_keypoints(return_maps=True)`` returns for all tokens.  Frames are uploaded to ``device`` one
    at a time (a tensor on a HIP device stays where it is); only the context's signatures and soft
    labels stay there.  ``labels0`` is (S, S) integers — class c >= 0 becomes a one-hot plane, and a −1
    is not background: it becomes an all-zero column, so that pixel casts no vote — or a (Cl, S, S)
    soft map, finite and non-negative.  ``radius`` and ``k`` in [1, 16], ``memory`` in [0, 63].

    Returns ``PropagatedLabels(label, confidence, soft)``: ``label`` (T, S, S) int32 the lowest class with
    the greatest soft value (−1 where no context pixel could be matched; frame 0: the given integers, or
    the soft map's argmax), ``confidence`` (T, S, S) float32 that value, ``soft`` (T, Cl, S, S) with
    ``return_soft``, else None.  The defaults are DINO's protocol (radius 12, k 5, temperature 0.07 at
    stride-8 features of 480p video) scaled to 128²; their suitability for these signatures has not
    been measured, nor has the quality of propagated labels on real video.
    """
    if torch.is_tensor(signatures):
        if signatures.dim() != 4:
            raise ValueError(f"signatures must be (T, n, S, S) or an iterable of (n, S, S) frames, got "
                             f"{tuple(signatures.shape)}")
        if signatures.is_cuda:
            device = signatures.device
    prop = _Propagator(labels0, radius, k, tau, memory, device, return_soft)
    for frame in signatures:
        prop.push(frame)
    return prop.finish()


@torch.no_grad()
def propagate_images(ldm, images, context, labels0, indices=None, device="cuda", layers=(0, 1, 2, 3, 4, 5),
                     noise_level=-1, augment_degrees=30, augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1),
                     augmentation_iterations=20, controllers=None, upscale_size=128, image_batch=None, radius=8, k=5,
                     tau=0.07, memory=2, return_soft=False):
    """``propagate_labels`` of the frames of a video: ``images`` (T, 3, H, W) in [0, 1], in frame order,
    ``labels0`` frame 0's labels at ``upscale_size``, ``indices`` the tokens that describe a pixel
    (default every token of ``context``).

    The thetas are drawn and the passes captured as ``predict_keypoints`` does (``_tta_passes``); each
    pass's averages, from ``ops.tta_reduce(return_avg=True)``, are fed to the propagation frame by frame
    as they come, so no more than one pass of captured maps, one pass of averages and the context is on
    the device at a time.  The result is what ``propagate_labels`` gives on
    ``predict_keypoints(..., return_maps=True)``'s maps from the same seed, bit for bit.  Single process
    only: under a process group of more than one rank it raises.
    """
    C, S = int(augmentation_iterations), int(upscale_size)
    indices = _tokens_of(indices, context, C, S, "propagate with")
    prop = _Propagator(labels0, radius, k, tau, memory, device, return_soft)
    if prop.S != S:
        raise ValueError(f"labels0 is {prop.S} x {prop.S}, upscale_size is {S}")
    for _, nb, maps, th_inv in _tta_passes("propagate_images", ldm, images, context, indices, device, layers,
                                           noise_level, augment_degrees, augment_scale, augment_translate, C,
                                           controllers, S, image_batch):
        _, avg = ops.tta_reduce(maps, th_inv, return_avg=True)
        del maps
        for b in range(nb):
            prop.push(avg[b])
        del avg
    return prop.finish()
