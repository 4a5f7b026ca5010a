"""CLI with the reference's flags and stages (``unsupervised_keypoints/main.py:23-416``).

optimize (``optimize_embedding`` → ``embedding.pt``) → find_indices (``find_best_indices`` →
``indices.pt``) → precompute (``precompute_all_keypoints`` → ``source_keypoints.pt``,
``target_keypoints.pt``, ``visible.pt``) → regressor (``regressor.pt``) → evaluate
(``all_errors.pt``).  ``--start_from_stage`` resumes from the saved files; ``--start_from_stage predict``
(extra) instead writes the keypoints of the dataset's images — the stage for unlabelled ``custom``
folders — from ``embedding.pt`` and ``indices.pt`` (``keypoints.pt``, ``keypoints.csv``, and
``regressed_keypoints.pt`` when ``regressor.pt`` is there; with ``--num_subjects k`` > 1 also the k peaks per token,
``subject_keypoints.pt``, ``subject_peak_values.pt`` and ``subject_keypoints.csv``) and stops, in one process.  With
``--correspond`` the stage needs no ``indices.pt``: it first picks the ``--top_k`` tokens of the embedding that are jointly
sharpest on the dataset's own images (``eval.correspond_images``: lowest summed softmax entropy of the TTA averages at
``--correspond_size``, scaled by ``--entropy_scale``), writes ``correspondence_indices.pt`` (k,),
``correspondence_entropy.pt`` (N,) and ``correspondence_points.pt`` (M, k, 2) (with ``--visualize`` also
``correspondences.png``), and predicts with those tokens; ``regressor.pt`` is then ignored.  With
``--part_maps`` it also writes which token owns each pixel of every image (``eval.part_maps`` at ``--part_size``:
``part_labels.pt`` (M, S, S) int16, −1 = background, ``part_mass.pt``, ``part_area.pt``, ``part_points.pt``, ``part_fg_iou.pt``
where the dataset has foreground masks, and with ``--visualize`` ``parts.png``).  With ``--transfer K`` it also carries
landmarks annotated on the dataset's first K images (``--transfer_points FILE``, or the items' own ``kpts``) over to every
image (``eval.describe_points`` and ``eval.transfer_keypoints`` at ``--transfer_size``: ``transfer_descriptors.pt``,
``transferred_keypoints.pt``, ``transfer_scores.pt``, ``transferred_keypoints.csv``, ``transfer_error.pt`` where the annotations
are the dataset's, and with ``--visualize`` ``transfer.png``).  With ``--dense_transfer SRC`` it also matches every pixel of
every image against the dataset's first image and carries that image's labels over (``eval.match_images`` and
``eval.transfer_labels`` at ``--dense_size``, with ``--dense_coarse SC`` and ``--dense_radius W`` coarse to fine:
a field at SC refined inside windows at ``--dense_size``: ``dense_index.pt``, ``dense_score.pt``, ``dense_cycle.pt``, ``dense_labels.pt``,
``dense_fg_iou.pt`` where the dataset has foreground masks, and with ``--visualize`` ``dense.png``).  With ``--track`` the
dataset's items in index order are the frames of a video and it also writes one track per token (``eval.track_images`` at
``--track_size``, ``--track_sigma`` and ``--track_radius``: ``tracked_keypoints.pt``, ``track_support.pt``,
``tracked_keypoints.csv``, and with ``--visualize`` ``track.png``).  With ``--propagate SRC`` the items are frames likewise and
the first frame's labels are carried through them (``eval.propagate_images`` at ``--propagate_size`` with ``--propagate_radius``,
``--propagate_k``, ``--propagate_tau`` and ``--propagate_memory``: ``propagated_labels.pt``, ``propagated_confidence.pt``,
``propagated_fg_iou.pt`` where the dataset has foreground masks, and with ``--visualize`` ``propagate.png``).  With ``--visualize``,
``visualize_attn_maps`` writes its sheets after find_indices and again, with the regressor, once
that is fitted (``main.py:271-292``, ``:370-391``); the reference calls both unconditionally, here
they are opt-in so that a run without the flag does what it always did.  Multi-GPU: like the
reference, one command uses every visible GPU — it starts one rank per GPU under ``torch.distributed.run`` (``--num_gpus`` to pick
fewer); launching it under ``torch.distributed.run`` yourself works too (every rank seeded alike:
``--seed``).
"""
import argparse
import contextlib
import csv
import os
import sys

import torch


STAGES = ("optimize", "find_indices", "precompute", "evaluate")


def build_parser():
    p = argparse.ArgumentParser(description="optimize a class embedding")
    p.add_argument("--model_type", type=str, default="runwayml/stable-diffusion-v1-5",
                   help="local directory of diffusers-0.8.0 UNet/VAE weights, a hub name in the local Hugging Face "
                        "cache, or 'random' / 'random-xl' / 'tiny' for seeded random weights (anything else raises)")
    p.add_argument("--dataset_loc", type=str, default="~")
    p.add_argument("--save_folder", type=str, default="outputs")
    p.add_argument("--wandb_name", type=str, default="temp")
    p.add_argument("--dataset_name", type=str, default="celeba_aligned",
                   choices=["celeba_aligned", "celeba_wild", "cub_aligned", "cub_001", "cub_002", "cub_003", "cub_all",
                            "deepfashion", "taichi", "human3.6m", "unaligned_human3.6m", "custom", "synthetic"])
    p.add_argument("--max_len", type=int, default=-1)
    p.add_argument("--start_from_stage", choices=list(STAGES) + ["predict"], default="optimize",
                   help="resume the pipeline from this stage's saved files; 'predict' only writes the keypoints of "
                        "the dataset's images (keypoints.pt, keypoints.csv) from embedding.pt and indices.pt")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--wandb", action="store_true")
    p.add_argument("--lr", type=float, default=5e-3)
    p.add_argument("--num_steps", type=int, default=500)
    p.add_argument("--num_tokens", type=int, default=500)
    p.add_argument("--feature_upsample_res", type=int, default=128)
    p.add_argument("--batch_size", type=int, default=4)
    p.add_argument("--top_k_strategy", type=str, default="gaussian", choices=["entropy", "gaussian", "consistent"])
    p.add_argument("--max_loc_strategy", type=str, default="argmax", choices=["argmax", "weighted_avg"])
    p.add_argument("--evaluation_method", type=str, default="inter_eye_distance",
                   choices=["inter_eye_distance", "visible", "mean_average_error", "pck", "orientation_invariant"])
    p.add_argument("--min_dist", type=float, default=0.1)
    p.add_argument("--furthest_point_num_samples", type=int, default=25)
    p.add_argument("--num_indices", type=int, default=100)
    p.add_argument("--num_subjects", type=int, default=1,
                   help="instances of the object per image: the targets of the optimisation take this many maxima "
                        "per map, and the predict stage also writes this many peaks per token "
                        "(subject_keypoints.pt (M, n, k, 2), subject_peak_values.pt (M, n, k), subject_keypoints.csv)")
    p.add_argument("--sharpening_loss_weight", type=float, default=100)
    p.add_argument("--equivariance_attn_loss_weight", type=float, default=1000.0)
    p.add_argument("--layers", type=int, nargs="+", default=[0, 1, 2, 3])
    p.add_argument("--noise_level", type=int, default=-1)
    p.add_argument("--max_num_points", type=int, default=50_000)
    p.add_argument("--sigma", type=float, default=2.0)
    p.add_argument("--augment_degrees", type=float, default=15.0)
    p.add_argument("--augment_scale", type=float, nargs="+", default=[0.8, 1.0])
    p.add_argument("--augment_translate", type=float, nargs="+", default=[0.25, 0.25])
    p.add_argument("--augmentation_iterations", type=int, default=10)
    p.add_argument("--visualize", action="store_true")
    p.add_argument("--validation", action="store_true")
    p.add_argument("--top_k", type=int, default=10)
    p.add_argument("--seed", type=int, default=0, help="CPU/GPU RNG seed, identical on every rank")
    p.add_argument("--num_gpus", type=int, default=-1,
                   help="ranks to start, one per GPU (-1 = every visible GPU, as the reference's DataParallel "
                        "over torch.cuda.device_count(), optimize_token.py:42-50); ignored under a launcher")
    p.add_argument("--keypoint_scores", action="store_true",
                   help="predict stage only: also write keypoint_scores.pt (M, n, 3) = peak, concentration and "
                        "coverage per keypoint, refined_keypoints.pt (M, n, 2), the sub-pixel centroid around each "
                        "peak, and keypoint_scores.csv")
    p.add_argument("--correspond", action="store_true",
                   help="predict stage only: instead of reading indices.pt, pick the --top_k tokens of embedding.pt with "
                        "the lowest softmax entropy of their TTA averages, summed over the dataset's images "
                        "(correspondence_indices.pt, correspondence_entropy.pt, correspondence_points.pt), and "
                        "predict with them")
    p.add_argument("--correspond_size", type=int, default=128,
                   help="--correspond: side of the TTA averages the entropies are taken on")
    p.add_argument("--entropy_scale", type=float, default=1.0,
                   help="--correspond: the averages are multiplied by this before the softmax")
    p.add_argument("--part_maps", action="store_true",
                   help="predict stage only: also write which token owns each pixel of every image's TTA averages "
                        "(part_labels.pt (M, S, S) int16 with -1 = background, part_mass.pt, part_area.pt, "
                        "part_points.pt, and part_fg_iou.pt where the dataset has foreground masks)")
    p.add_argument("--part_size", type=int, default=128, help="--part_maps: side S of the part maps")
    p.add_argument("--part_tokens", type=str, default="indices", choices=["indices", "all"],
                   help="--part_maps: label with the prediction's tokens, or with every token of embedding.pt")
    p.add_argument("--part_threshold", type=float, default=0.0,
                   help="--part_maps: a pixel whose tokens' attention sums to this or less is background")
    p.add_argument("--transfer", type=int, default=None, metavar="K",
                   help="predict stage only: the dataset's first K images are exemplars; the landmarks annotated on "
                        "them are located in every image by the cosine of the tokens' TTA averages "
                        "(transfer_descriptors.pt (Q, n), transferred_keypoints.pt (M, Q, 2), transfer_scores.pt (M, Q), "
                        "transferred_keypoints.csv, and transfer_error.pt where the annotations are the dataset's kpts)")
    p.add_argument("--transfer_points", type=str, default=None, metavar="FILE",
                   help="--transfer: a saved (K, Q, 2) tensor of (row, col) in [0, 1], NaN where a landmark is not "
                        "annotated on an exemplar; default: the exemplars' own kpts (visibility 0 = not annotated)")
    p.add_argument("--transfer_size", type=int, default=128, help="--transfer: side S of the averages that are matched")
    p.add_argument("--transfer_tokens", type=str, default="all", choices=["all", "indices"],
                   help="--transfer: describe a pixel by every token of embedding.pt, or by the prediction's tokens")
    p.add_argument("--dense_transfer", type=str, default=None, metavar="SRC",
                   help="predict stage only: the dataset's first image is the source; every pixel of every image is matched "
                        "to the source pixel whose tokens' TTA averages have the greatest cosine, and the source's labels "
                        "are carried over (dense_index.pt, dense_score.pt, dense_cycle.pt (M, S, S), dense_labels.pt (M, S, S) "
                        "int16, and dense_fg_iou.pt where the dataset has foreground masks).  SRC: 'mask' (the first item's "
                        "mask: foreground 0, background -1) or a saved integer tensor of labels for the source, -1 = "
                        "unlabelled, nearest-resized to --dense_size")
    p.add_argument("--dense_size", type=int, default=128, help="--dense_transfer: side S of the averages that are matched")
    p.add_argument("--dense_coarse", type=int, default=None, metavar="SC",
                   help="--dense_transfer: coarse to fine.  The averages, pooled to SC x SC, are matched pixel against "
                        "pixel and every pixel of --dense_size is then matched inside a window around its cell's coarse "
                        "match (eval.match_images(coarse_size=SC)).  SC divides --dense_size by a factor in [2, 8]; the "
                        "files are the same, at --dense_size.  Default: every pixel against every pixel at --dense_size")
    p.add_argument("--dense_radius", type=int, default=None, metavar="W",
                   help="--dense_coarse: the window reaches W pixels of --dense_size to each side of the coarse match, "
                        "W in [1, 16] (default: the factor + 1)")
    p.add_argument("--dense_tokens", type=str, default="all", choices=["all", "indices"],
                   help="--dense_transfer: describe a pixel by every token of embedding.pt, or by the prediction's tokens")
    p.add_argument("--dense_max_cycle", type=float, default=None,
                   help="--dense_transfer: no label where the match does not come back within this many pixels")
    p.add_argument("--dense_min_score", type=float, default=None,
                   help="--dense_transfer: no label where the match's cosine is below this")
    p.add_argument("--track", action="store_true",
                   help="predict stage only: the dataset's items in index order are the frames of a video; also write one "
                        "track per token, the most probable path of its TTA averages' peak under a Gaussian random walk "
                        "(tracked_keypoints.pt (M, n, 2), track_support.pt (M, n), tracked_keypoints.csv)")
    p.add_argument("--track_sigma", type=float, default=2.0,
                   help="--track: standard deviation of the walk's step, in pixels of --track_size")
    p.add_argument("--track_radius", type=int, default=None,
                   help="--track: the longest step per frame and axis, 1 to 32 pixels (default ceil(3 sigma), clipped)")
    p.add_argument("--track_size", type=int, default=128, help="--track: side S of the averages that are tracked")
    p.add_argument("--propagate", type=str, default=None, metavar="SRC",
                   help="--start_from_stage predict: the dataset's items in index order are the frames of a video; also "
                        "carry the first frame's labels through them: every pixel's k most similar pixels in a window of "
                        "the first and the last few frames vote (propagated_labels.pt (M, S, S) int32, "
                        "propagated_confidence.pt (M, S, S), and propagated_fg_iou.pt where the dataset has foreground "
                        "masks).  SRC: 'mask' (the first item's mask: foreground 1, background 0) or a saved (h, w) "
                        "integer tensor for the first frame, -1 = casts no vote, nearest-resized to --propagate_size")
    p.add_argument("--propagate_size", type=int, default=128, help="--propagate: side S of the averages that are matched")
    p.add_argument("--propagate_radius", type=int, default=8,
                   help="--propagate: the window reaches this many pixels of --propagate_size to each side, 1 to 16")
    p.add_argument("--propagate_k", type=int, default=5, help="--propagate: the matches that vote per pixel, 1 to 16")
    p.add_argument("--propagate_tau", type=float, default=0.07, help="--propagate: the temperature of the votes' softmax")
    p.add_argument("--propagate_memory", type=int, default=2,
                   help="--propagate: the context is the first frame and this many of the last frames, 0 to 63")
    p.add_argument("--propagate_tokens", type=str, default="all", choices=["all", "indices"],
                   help="--propagate: describe a pixel by every token of embedding.pt, or by the prediction's tokens")
    return p


def ranks_to_start(args, visible, env):
    """How many ranks this command starts: 1 when already running as a rank (``env``) or with at
    most one GPU, and for the single-process ``predict`` stage, else ``--num_gpus`` (every visible GPU by
    default)."""
    if env is not None or args.start_from_stage == "predict":   # predict runs in this process, on --device
        return 1
    n = visible if args.num_gpus < 0 else args.num_gpus
    if n > max(visible, 1):
        raise SystemExit(f"--num_gpus {n} but {visible} GPU(s) are visible")
    return max(n, 1)


def _load(folder, name, device=None):
    t = torch.load(os.path.join(folder, name), weights_only=True)
    return t.to(device) if (device is not None and t is not None) else t


def _image_names(dataset):
    """File name per dataset index where the reader has ``image_files`` (``custom``), else None."""
    if isinstance(dataset, torch.utils.data.Subset):
        names = _image_names(dataset.dataset)
        return None if names is None else [names[i] for i in dataset.indices]
    names = getattr(dataset, "image_files", None)
    return None if names is None else list(names)


@contextlib.contextmanager
def _rng_restored(device):
    """The CPU and ``device`` RNG states are on exit what they were on entry, also when the body raises."""
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(device)
    try:
        yield
    finally:
        torch.set_rng_state(cpu_state)
        torch.cuda.set_rng_state(dev_state, device)


def _write_rows(path, names, values):
    """A CSV without header, one row per entry of ``values`` (M, …): the index, the entry's name where
    ``names`` has them, then the entry's values flattened, each as ``repr(float(v))``."""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        for i in range(values.shape[0]):
            row = [i] + ([names[i]] if names is not None else [])
            w.writerow(row + [repr(float(v)) for v in values[i].reshape(-1)])


def _save_row_sheet(path, images, points, device):
    """``path``: the first 12 of ``images`` at most in one row with their ``points``, point j in colour j,
    downscaled by 2 when both sides are even."""
    from . import ops
    from .visualize import save_png
    m = min(12, images.shape[0])
    f = 2 if images.shape[-1] % 2 == 0 and images.shape[-2] % 2 == 0 else 1
    sheet = ops.render_sheet(images[:m].to(device, torch.float32), None, points[:m], rows=1, cols=m, downscale=f)
    save_png(sheet, path)


def correspond_stage(args, ldm, controllers, embedding, dataset):
    """``--correspond``: ``eval.correspond_images`` over every image of ``dataset`` for ``--top_k`` of the
    embedding's tokens.  Writes ``correspondence_indices.pt`` (k,) int64, ``correspondence_entropy.pt``
    (N,) float64 (per token, summed over the images) and ``correspondence_points.pt`` (M, k, 2), and with
    ``--visualize`` ``correspondences.png``: the first 12 images at most in one row with their k points,
    keypoint j in colour j in every image.  The CPU and device RNG states are what they were on entry
    when it returns, so the prediction that follows draws what a plain predict run draws.  Returns
    the indices."""
    from .eval import correspond_images
    folder = args.save_folder
    with _rng_restored(args.device):
        images = torch.stack([torch.as_tensor(dataset[i]["img"]) for i in range(len(dataset))])
        corr = correspond_images(ldm, images, embedding, num_points=args.top_k, device=args.device, layers=args.layers,
                                 noise_level=args.noise_level, augment_degrees=args.augment_degrees,
                                 augment_scale=args.augment_scale, augment_translate=args.augment_translate,
                                 augmentation_iterations=args.augmentation_iterations, controllers=controllers,
                                 upscale_size=args.correspond_size, entropy_scale=args.entropy_scale)
        torch.save(corr.indices.cpu(), os.path.join(folder, "correspondence_indices.pt"))
        torch.save(corr.entropy.cpu(), os.path.join(folder, "correspondence_entropy.pt"))
        torch.save(corr.points.cpu(), os.path.join(folder, "correspondence_points.pt"))
        if args.visualize:
            _save_row_sheet(os.path.join(folder, "correspondences.png"), images, corr.points, args.device)
        print("correspond: indices", corr.indices.tolist(), flush=True)
    return corr.indices


def parts_stage(args, ldm, controllers, embedding, indices, dataset):
    """``--part_maps``: ``eval.part_maps`` over every image of ``dataset`` at ``--part_size``, for the
    prediction's ``indices`` or (``--part_tokens all``) every token of the embedding.  Writes
    ``part_labels.pt`` (M, S, S) int16 (the token's position among those tokens, −1 = background: the
    tokens' attention sums to ``--part_threshold`` or less), ``part_mass.pt`` (M, S, S), ``part_area.pt``
    (M, n) int64 and ``part_points.pt`` (M, n, 2); where the dataset's items carry ``mask`` also
    ``part_fg_iou.pt`` (M,) float64, ``eval.foreground_iou`` of the labels against it, and prints its mean.
    With ``--visualize`` ``parts.png``: the first 12 images at most in one row, every non-background pixel
    blended with its token's colour (``ops.default_colors``, the labels nearest-upsampled to the image
    size) and the tokens' points on top, token j in colour j.  The CPU and device RNG states are what they
    were on entry when it returns, so the prediction that follows draws what a plain predict run draws."""
    from . import ops
    from .eval import foreground_iou, part_maps
    folder = args.save_folder
    with _rng_restored(args.device):
        items = [dataset[i] for i in range(len(dataset))]
        images = torch.stack([torch.as_tensor(it["img"]) for it in items])
        parts = part_maps(ldm, images, embedding, None if args.part_tokens == "all" else indices.cpu(),
                          device=args.device, layers=args.layers, noise_level=args.noise_level,
                          augment_degrees=args.augment_degrees, augment_scale=args.augment_scale,
                          augment_translate=args.augment_translate,
                          augmentation_iterations=args.augmentation_iterations, controllers=controllers,
                          upscale_size=args.part_size, part_threshold=args.part_threshold)
        torch.save(parts.label.cpu(), os.path.join(folder, "part_labels.pt"))
        torch.save(parts.mass.cpu(), os.path.join(folder, "part_mass.pt"))
        torch.save(parts.area.cpu(), os.path.join(folder, "part_area.pt"))
        torch.save(parts.points.cpu(), os.path.join(folder, "part_points.pt"))
        if items and all("mask" in it for it in items):
            masks = torch.stack([torch.as_tensor(it["mask"], dtype=torch.float32) for it in items])
            iou = foreground_iou(parts.label, masks).cpu()
            torch.save(iou, os.path.join(folder, "part_fg_iou.pt"))
            print(f"part_maps: mean foreground IoU {float(iou.mean()):.4f} over {iou.shape[0]} images", flush=True)
        if args.visualize:
            m = min(12, images.shape[0])
            shown = images[:m].to(args.device, torch.float32)
            label = torch.nn.functional.interpolate(parts.label[:m, None].float(), size=tuple(images.shape[-2:]),
                                                    mode="nearest")[:, 0].long()
            colors = ops.default_colors(parts.points.shape[1]).to(args.device)
            tint = (colors.float() / 255.0)[label.clamp_min(0)].permute(0, 3, 1, 2)
            shown = torch.where((label >= 0)[:, None], 0.5 * shown + 0.5 * tint, shown)
            _save_row_sheet(os.path.join(folder, "parts.png"), shown, parts.points, args.device)
        print(f"part_maps: {images.shape[0]} images, {parts.points.shape[1]} tokens at {args.part_size} -> "
              f"{os.path.join(folder, 'part_labels.pt')}", flush=True)


def transfer_stage(args, ldm, controllers, embedding, indices, dataset):
    """``--transfer K``: the dataset's first K images are the exemplars.  Their annotations are
    ``--transfer_points`` (a saved (K, Q, 2) tensor, (row, col) in [0, 1], NaN = not annotated) or the items' own
    ``kpts`` (a landmark whose ``visibility`` is 0 counts as not annotated).  ``eval.describe_points`` turns them into
    descriptors over every token of the embedding or (``--transfer_tokens indices``) the prediction's, at
    ``--transfer_size``, and ``eval.transfer_keypoints`` locates them in every image of ``dataset``, the exemplars
    included.  Writes ``transfer_descriptors.pt`` (Q, n), ``transferred_keypoints.pt`` (M, Q, 2), ``transfer_scores.pt``
    (M, Q) and ``transferred_keypoints.csv`` (no header: index, file name where the reader has one, then per landmark
    row, col, score); where the annotations came from ``kpts`` also ``transfer_error.pt`` (M, Q), the Euclidean distance
    to the image's own annotation in normalised coordinates (NaN where the landmark is not visible), and prints its
    mean over the non-exemplar images.  With ``--visualize`` ``transfer.png``: the first 12 images at most in one row,
    landmark j in colour j.  The CPU and device RNG states are what they were on entry when it returns, so the
    prediction that follows draws what a plain predict run draws."""
    from .eval import describe_points, transfer_keypoints
    folder, K, M = args.save_folder, int(args.transfer), len(dataset)
    if not 1 <= K <= M:
        raise ValueError(f"--transfer {K}: the exemplars are the dataset's first K images, and it has {M}")
    with _rng_restored(args.device):
        items = [dataset[i] for i in range(M)]
        images = torch.stack([torch.as_tensor(it["img"]) for it in items])
        own = args.transfer_points is None
        if own:
            if not all("kpts" in it for it in items):
                raise ValueError("--transfer: the dataset's items carry no kpts; give --transfer_points")
            kpts = torch.stack([torch.as_tensor(it["kpts"], dtype=torch.float32) for it in items])           # (M, Q, 2)
            seen = torch.stack([torch.as_tensor(it["visibility"]) != 0 if "visibility" in it else
                                torch.ones(kpts.shape[1], dtype=torch.bool) for it in items])                # (M, Q)
            kpts = torch.where(seen[..., None], kpts, torch.full_like(kpts, float("nan")))
            points = kpts[:K]
        else:
            points = torch.as_tensor(torch.load(args.transfer_points, weights_only=True), dtype=torch.float32)
            if points.dim() != 3 or points.shape[0] != K or points.shape[2] != 2:
                raise ValueError(f"--transfer_points must hold a ({K}, Q, 2) tensor, got {tuple(points.shape)}")
        common = dict(indices=None if args.transfer_tokens == "all" else indices.cpu(), device=args.device,
                      layers=args.layers, noise_level=args.noise_level, augment_degrees=args.augment_degrees,
                      augment_scale=args.augment_scale, augment_translate=args.augment_translate,
                      augmentation_iterations=args.augmentation_iterations, controllers=controllers,
                      upscale_size=args.transfer_size)
        desc = describe_points(ldm, images[:K], points, embedding, **common)
        moved = transfer_keypoints(ldm, images, embedding, desc, **common)
        pts, score = moved.points.cpu(), moved.score.cpu()
        torch.save(desc.cpu(), os.path.join(folder, "transfer_descriptors.pt"))
        torch.save(pts, os.path.join(folder, "transferred_keypoints.pt"))
        torch.save(score, os.path.join(folder, "transfer_scores.pt"))
        _write_rows(os.path.join(folder, "transferred_keypoints.csv"), _image_names(dataset),
                    torch.cat([pts, score[..., None]], dim=-1))
        if own:
            error = (pts - kpts).pow(2).sum(dim=-1).sqrt()      # NaN where the landmark is not visible
            torch.save(error, os.path.join(folder, "transfer_error.pt"))
            rest = error[K:]
            rest = rest[~torch.isnan(rest)]
            mean = float(rest.mean()) if rest.numel() else float("nan")
            print(f"transfer: mean distance to the annotations {mean:.4f} over {rest.numel()} visible landmarks of "
                  f"{M - K} images", flush=True)
        if args.visualize:
            _save_row_sheet(os.path.join(folder, "transfer.png"), images, moved.points, args.device)
        print(f"transfer: {K} exemplars, {desc.shape[0]} landmarks, {desc.shape[1]} tokens at {args.transfer_size} -> "
              f"{os.path.join(folder, 'transferred_keypoints.pt')}", flush=True)


def dense_stage(args, ldm, controllers, embedding, indices, dataset):
    """``--dense_transfer SRC``: the dataset's first image is the source.  ``eval.match_images`` matches every
    pixel of every image of ``dataset`` (the source included) against it and back at ``--dense_size`` = S, over
    every token of the embedding or (``--dense_tokens indices``) the prediction's, with ``--dense_coarse SC`` coarse
    to fine (every pixel against every pixel at SC, then inside a window of ``--dense_radius`` at S; a pixel whose
    cell has no coarse match gets −1); ``eval.transfer_labels`` carries
    the source's labels over, gated by ``--dense_max_cycle`` and ``--dense_min_score`` where given.  The labels are
    ``SRC``: ``mask`` (the first item's ``mask``: foreground 0, background −1) or a saved integer tensor for the
    source (−1 = unlabelled), either nearest-resized to (S, S).  Writes ``dense_index.pt`` (M, S, S) int32,
    ``dense_score.pt`` and ``dense_cycle.pt`` (M, S, S) float32 and ``dense_labels.pt`` (M, S, S) int16; where the
    dataset's items carry ``mask`` also ``dense_fg_iou.pt`` (M,) float64, ``eval.foreground_iou`` of the transferred
    labels, and prints its mean over the non-source images.  With ``--visualize`` ``dense.png``, tinted as
    ``parts.png`` is.  The CPU and device RNG states are what they were on entry when it returns, so the prediction
    that follows draws what a plain predict run draws."""
    from . import ops
    from .eval import foreground_iou, match_images, transfer_labels
    folder, S, M = args.save_folder, int(args.dense_size), len(dataset)
    if M < 1:
        raise ValueError("--dense_transfer: the dataset is empty")
    with _rng_restored(args.device):
        items = [dataset[i] for i in range(M)]
        images = torch.stack([torch.as_tensor(it["img"]) for it in items])
        have_masks = all("mask" in it for it in items)
        if args.dense_transfer == "mask":
            if "mask" not in items[0]:
                raise ValueError("--dense_transfer mask: the dataset's items carry no mask; give a file of labels")
            mask = torch.as_tensor(items[0]["mask"], dtype=torch.float32)
            mask = mask[..., 0] if mask.dim() == 3 and mask.shape[-1] == 1 else mask
            labels = torch.where(mask > 0.5, 0, -1)
        else:
            labels = torch.as_tensor(torch.load(args.dense_transfer, weights_only=True))
            if labels.dim() != 2 or labels.is_floating_point() or labels.dtype == torch.bool:
                raise ValueError(f"--dense_transfer: the file must hold an (h, w) integer tensor, got "
                                 f"{tuple(labels.shape)} {labels.dtype}")
        if tuple(labels.shape) != (S, S):
            labels = torch.nn.functional.interpolate(labels[None, None].to(torch.float32), size=(S, S),
                                                     mode="nearest")[0, 0]
        labels = labels.to(torch.int64)
        match = match_images(ldm, images[0], images, embedding,
                             None if args.dense_tokens == "all" else indices.cpu(), device=args.device,
                             layers=args.layers, noise_level=args.noise_level, augment_degrees=args.augment_degrees,
                             augment_scale=args.augment_scale, augment_translate=args.augment_translate,
                             augmentation_iterations=args.augmentation_iterations, controllers=controllers,
                             upscale_size=S, coarse_size=args.dense_coarse, refine_radius=args.dense_radius)
        moved = transfer_labels(match, labels, max_cycle=args.dense_max_cycle, min_score=args.dense_min_score)
        torch.save(match.index.cpu(), os.path.join(folder, "dense_index.pt"))
        torch.save(match.score.cpu(), os.path.join(folder, "dense_score.pt"))
        torch.save(match.cycle.cpu(), os.path.join(folder, "dense_cycle.pt"))
        torch.save(moved.cpu(), os.path.join(folder, "dense_labels.pt"))
        if have_masks:
            masks = torch.stack([torch.as_tensor(it["mask"], dtype=torch.float32) for it in items])
            iou = foreground_iou(moved, masks).cpu()
            torch.save(iou, os.path.join(folder, "dense_fg_iou.pt"))
            rest = iou[1:]
            mean = float(rest.mean()) if rest.numel() else float("nan")
            print(f"dense_transfer: mean foreground IoU {mean:.4f} over {rest.numel()} non-source images", flush=True)
        if args.visualize:
            m = min(12, M)
            shown = images[:m].to(args.device, torch.float32)
            label = torch.nn.functional.interpolate(moved[:m, None].float(), size=tuple(images.shape[-2:]),
                                                    mode="nearest")[:, 0].long()
            colors = ops.default_colors(int(moved.max().clamp_min(0)) + 1).to(args.device)
            tint = (colors.float() / 255.0)[label.clamp_min(0)].permute(0, 3, 1, 2)
            shown = torch.where((label >= 0)[:, None], 0.5 * shown + 0.5 * tint, shown)
            _save_row_sheet(os.path.join(folder, "dense.png"), shown, match.token_points[:, :0], args.device)
        print(f"dense_transfer: {M} images against the first at {S}, {match.token_points.shape[1]} tokens -> "
              f"{os.path.join(folder, 'dense_labels.pt')}", flush=True)


def track_stage(args, ldm, controllers, embedding, indices, dataset):
    """``--track``: the dataset's items in index order are the frames of a video.  ``eval.track_images`` tracks the
    prediction's tokens through them at ``--track_size`` with ``--track_sigma`` and ``--track_radius``.  Writes
    ``tracked_keypoints.pt`` (M, n, 2) = (row, col) / S, ``track_support.pt`` (M, n) (each frame's average at the
    tracked pixel over its maximum) and ``tracked_keypoints.csv`` (no header: index, file name where the reader has
    one, the n (row, col) pairs, then the n supports); with ``--visualize`` ``track.png``, the first 12 frames at most
    in one row with their tracked points.  The CPU and device RNG states are what they were on entry when it returns,
    so the prediction that follows draws what a plain predict run draws."""
    from .eval import track_images
    folder, M = args.save_folder, len(dataset)
    if M < 1:
        raise ValueError("--track: the dataset is empty")
    with _rng_restored(args.device):
        images = torch.stack([torch.as_tensor(dataset[i]["img"]) for i in range(M)])
        tracks = track_images(ldm, images, embedding, indices.cpu(), device=args.device, layers=args.layers,
                              noise_level=args.noise_level, augment_degrees=args.augment_degrees,
                              augment_scale=args.augment_scale, augment_translate=args.augment_translate,
                              augmentation_iterations=args.augmentation_iterations, controllers=controllers,
                              upscale_size=args.track_size, sigma=args.track_sigma, radius=args.track_radius)
        pos, support = tracks.pos.cpu(), tracks.support.cpu()
        torch.save(pos, os.path.join(folder, "tracked_keypoints.pt"))
        torch.save(support, os.path.join(folder, "track_support.pt"))
        _write_rows(os.path.join(folder, "tracked_keypoints.csv"), _image_names(dataset),
                    torch.cat([pos.flatten(1), support], dim=1))
        if args.visualize:
            _save_row_sheet(os.path.join(folder, "track.png"), images, tracks.pos, args.device)
        print(f"track: {M} frames, {pos.shape[1]} tokens at {args.track_size} -> "
              f"{os.path.join(folder, 'tracked_keypoints.pt')}", flush=True)


def propagate_stage(args, ldm, controllers, embedding, indices, dataset):
    """``--propagate SRC``: the dataset's items in index order are the frames of a video.  ``eval.propagate_images``
    carries the first frame's labels through them at ``--propagate_size`` = S over every token of the embedding or
    (``--propagate_tokens indices``) the prediction's, with ``--propagate_radius``, ``--propagate_k``, ``--propagate_tau``
    and ``--propagate_memory``.  The labels are ``SRC``: ``mask`` (the first item's ``mask``: foreground 1, background 0) or
    a saved integer tensor for the first frame (−1 = the pixel casts no vote), either nearest-resized to (S, S).
    Writes ``propagated_labels.pt`` (M, S, S) int32 and ``propagated_confidence.pt`` (M, S, S) float32; where the
    dataset's items carry ``mask`` also ``propagated_fg_iou.pt`` (M,) float64, ``eval.foreground_iou`` of the pixels whose
    label is at least 1 (with ``mask``: the foreground), and prints its mean over the later frames.  With ``--visualize``
    ``propagate.png``, tinted as ``parts.png`` is.  The CPU and device RNG states are what they were on entry when it
    returns, so the prediction that follows draws what a plain predict run draws."""
    from . import ops
    from .eval import foreground_iou, propagate_images
    folder, S, M = args.save_folder, int(args.propagate_size), len(dataset)
    if M < 1:
        raise ValueError("--propagate: the dataset is empty")
    with _rng_restored(args.device):
        items = [dataset[i] for i in range(M)]
        images = torch.stack([torch.as_tensor(it["img"]) for it in items])
        have_masks = all("mask" in it for it in items)
        if args.propagate == "mask":
            if "mask" not in items[0]:
                raise ValueError("--propagate mask: the dataset's items carry no mask; give a file of labels")
            mask = torch.as_tensor(items[0]["mask"], dtype=torch.float32)
            mask = mask[..., 0] if mask.dim() == 3 and mask.shape[-1] == 1 else mask
            labels = torch.where(mask > 0.5, 1, 0)
        else:
            labels = torch.as_tensor(torch.load(args.propagate, weights_only=True))
            if labels.dim() != 2 or labels.is_floating_point() or labels.dtype == torch.bool:
                raise ValueError(f"--propagate: the file must hold an (h, w) integer tensor, got "
                                 f"{tuple(labels.shape)} {labels.dtype}")
        if tuple(labels.shape) != (S, S):
            labels = torch.nn.functional.interpolate(labels[None, None].to(torch.float32), size=(S, S),
                                                     mode="nearest")[0, 0]
        labels = labels.to(torch.int64)
        got = propagate_images(ldm, images, embedding, labels,
                               None if args.propagate_tokens == "all" else indices.cpu(), device=args.device,
                               layers=args.layers, noise_level=args.noise_level, augment_degrees=args.augment_degrees,
                               augment_scale=args.augment_scale, augment_translate=args.augment_translate,
                               augmentation_iterations=args.augmentation_iterations, controllers=controllers,
                               upscale_size=S, radius=args.propagate_radius, k=args.propagate_k, tau=args.propagate_tau,
                               memory=args.propagate_memory)
        torch.save(got.label.cpu(), os.path.join(folder, "propagated_labels.pt"))
        torch.save(got.confidence.cpu(), os.path.join(folder, "propagated_confidence.pt"))
        if have_masks:
            masks = torch.stack([torch.as_tensor(it["mask"], dtype=torch.float32) for it in items])
            iou = foreground_iou(torch.where(got.label >= 1, 0, -1), masks).cpu()
            torch.save(iou, os.path.join(folder, "propagated_fg_iou.pt"))
            rest = iou[1:]
            mean = float(rest.mean()) if rest.numel() else float("nan")
            print(f"propagate: mean foreground IoU {mean:.4f} over {rest.numel()} later frames", flush=True)
        if args.visualize:
            m = min(12, M)
            shown = images[:m].to(args.device, torch.float32)
            label = torch.nn.functional.interpolate(got.label[:m, None].float(), size=tuple(images.shape[-2:]),
                                                    mode="nearest")[:, 0].long()
            colors = ops.default_colors(int(got.label.max().clamp_min(0)) + 1).to(args.device)
            tint = (colors.float() / 255.0)[label.clamp_min(0)].permute(0, 3, 1, 2)
            shown = torch.where((label >= 0)[:, None], 0.5 * shown + 0.5 * tint, shown)
            _save_row_sheet(os.path.join(folder, "propagate.png"), shown, torch.zeros(m, 0, 2, device=args.device),
                            args.device)
        print(f"propagate: {M} frames at {S}, radius {args.propagate_radius}, k {args.propagate_k} -> "
              f"{os.path.join(folder, 'propagated_labels.pt')}", flush=True)


def predict_stage(args, ldm, controllers, batch=4):
    """``--start_from_stage predict``: the keypoints of every image of the dataset (built as
    ``evaluate`` builds it: ``split="test"``, the whole folder for ``custom``), in index order, from
    the saved ``embedding.pt`` and ``indices.pt``.  Writes ``keypoints.pt`` (M, n, 2) = (row, col) / 512,
    ``regressed_keypoints.pt`` when ``regressor.pt`` is there, and ``keypoints.csv`` (one row per image and no
    header: index, file name where the reader has one, the n (row, col) pairs, then the regressed pairs).
    With ``--keypoint_scores`` also ``keypoint_scores.pt`` (M, n, 3) = (peak, concentration, coverage),
    ``refined_keypoints.pt`` (M, n, 2) and ``keypoint_scores.csv`` (no header: index, file name where the
    reader has one, then per token refined row, refined col, peak, concentration, coverage).
    With ``--num_subjects k`` > 1 also ``subject_keypoints.pt`` (M, n, k, 2), the k peaks per token of
    ``find_k_max_pixels`` on the TTA average / 512 (round 0 is ``keypoints.pt``'s argmax),
    ``subject_peak_values.pt`` (M, n, k), the value that won each round, and ``subject_keypoints.csv``
    (no header: index, file name where the reader has one, then per token and round row, col, value).
    Round j of two tokens need not belong to the same instance; the regressor sees round 0 only.
    With ``--correspond`` the indices come from ``correspond_stage`` on the same images, not from
    ``indices.pt``, and ``regressor.pt`` is not applied (it was fitted to other tokens).
    With ``--part_maps`` ``parts_stage`` first writes the part maps of the same images; the keypoints are
    the same bits with and without it.  With ``--transfer K`` ``transfer_stage`` does the same for the transferred
    landmarks, with ``--dense_transfer SRC`` ``dense_stage`` for the dense field and the transferred labels, and with
    ``--track`` ``track_stage`` for the tokens' tracks through the images as frames."""
    from .datasets import make_dataset
    from .eval import predict_keypoints
    folder = args.save_folder
    embedding = _load(folder, "embedding.pt", args.device).detach()
    dataset = make_dataset(args.dataset_name, args.dataset_loc, max_len=args.max_len, validation=args.validation,
                           split="test")
    have_regressor = os.path.exists(os.path.join(folder, "regressor.pt"))
    if args.correspond:
        indices = correspond_stage(args, ldm, controllers, embedding, dataset)
        if have_regressor:
            print("predict: --correspond ignores regressor.pt (it was fitted to other tokens)", flush=True)
        regressor = None
    else:
        indices = _load(folder, "indices.pt", args.device).detach()
        regressor = _load(folder, "regressor.pt", args.device) if have_regressor else None
    if args.part_maps:
        parts_stage(args, ldm, controllers, embedding, indices, dataset)
    if args.transfer is not None:
        transfer_stage(args, ldm, controllers, embedding, indices, dataset)
    if args.dense_transfer is not None:
        dense_stage(args, ldm, controllers, embedding, indices, dataset)
    if args.track:
        track_stage(args, ldm, controllers, embedding, indices, dataset)
    if args.propagate is not None:
        propagate_stage(args, ldm, controllers, embedding, indices, dataset)
    names = _image_names(dataset)
    k = int(args.num_subjects)
    kps, regs, scos, refs, pks, vals = [], [], [], [], [], []
    for i0 in range(0, len(dataset), batch):
        images = torch.stack([dataset[i]["img"] for i in range(i0, min(i0 + batch, len(dataset)))])
        out = predict_keypoints(ldm, images, embedding, indices.cpu(), regressor=regressor, device=args.device,
                                layers=args.layers, noise_level=args.noise_level,
                                augment_degrees=args.augment_degrees, augment_scale=args.augment_scale,
                                augment_translate=args.augment_translate,
                                augmentation_iterations=args.augmentation_iterations,
                                max_loc_strategy=args.max_loc_strategy, controllers=controllers,
                                return_scores=args.keypoint_scores, num_subjects=k)
        out = list(out) if isinstance(out, tuple) else [out]
        # predict_keypoints refuses num_subjects > 1 with return_scores: at most one trailing output
        last = out.pop() if k > 1 or args.keypoint_scores else None
        if k > 1:
            pks.append(last.pos.cpu())
            vals.append(last.value.cpu())
        if args.keypoint_scores:
            scos.append(torch.stack([last.peak, last.concentration, last.coverage], dim=-1).cpu())
            refs.append(last.refined.cpu())
        kps.append(out[0].cpu())
        if regressor is not None:
            regs.append(out[1].cpu())
    n = len(indices)
    kps = torch.cat(kps) if kps else torch.zeros(0, n, 2)
    torch.save(kps, os.path.join(folder, "keypoints.pt"))
    if regressor is not None:
        regs = torch.cat(regs) if regs else torch.zeros(0, regressor.shape[1] // 2, 2)
        torch.save(regs, os.path.join(folder, "regressed_keypoints.pt"))
    _write_rows(os.path.join(folder, "keypoints.csv"), names,
                kps.flatten(1) if regressor is None else torch.cat([kps.flatten(1), regs.flatten(1)], dim=1))
    if args.keypoint_scores:
        scos = torch.cat(scos) if scos else torch.zeros(0, n, 3)
        refs = torch.cat(refs) if refs else torch.zeros(0, n, 2)
        torch.save(scos, os.path.join(folder, "keypoint_scores.pt"))
        torch.save(refs, os.path.join(folder, "refined_keypoints.pt"))
        _write_rows(os.path.join(folder, "keypoint_scores.csv"), names, torch.cat([refs, scos], dim=-1))
    if k > 1:
        pks = torch.cat(pks) if pks else torch.zeros(0, n, k, 2)
        vals = torch.cat(vals) if vals else torch.zeros(0, n, k)
        torch.save(pks, os.path.join(folder, "subject_keypoints.pt"))
        torch.save(vals, os.path.join(folder, "subject_peak_values.pt"))
        _write_rows(os.path.join(folder, "subject_keypoints.csv"), names, torch.cat([pks, vals[..., None]], dim=-1))
    print(f"predict: {kps.shape[0]} images, {n} keypoints each -> {os.path.join(folder, 'keypoints.pt')}", flush=True)


def main(argv=None):
    import numpy as np
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.start_from_stage == "predict":
        if args.num_subjects < 1:
            parser.error("--num_subjects must be at least 1")
        if args.num_subjects > 1 and args.keypoint_scores:
            parser.error("--start_from_stage predict: --num_subjects > 1 and --keypoint_scores each need their own "
                         "TTA reduce; run the stage once with each")
    if args.correspond and args.start_from_stage != "predict":
        parser.error("--correspond belongs to --start_from_stage predict")
    if not 0.0 < args.entropy_scale < float("inf"):
        parser.error("--entropy_scale must be positive and finite")
    if args.correspond_size < 2:
        parser.error("--correspond_size must be at least 2")
    if args.part_maps and args.start_from_stage != "predict":
        parser.error("--part_maps belongs to --start_from_stage predict")
    if args.part_size < 2:
        parser.error("--part_size must be at least 2")
    if args.transfer is None and args.transfer_points is not None:
        parser.error("--transfer_points belongs to --transfer K")
    if args.transfer is not None and args.start_from_stage != "predict":
        parser.error("--transfer belongs to --start_from_stage predict")
    if args.transfer is not None and args.transfer < 1:
        parser.error("--transfer must be at least 1 (the number of exemplar images)")
    if args.transfer_size < 2:
        parser.error("--transfer_size must be at least 2")
    if args.dense_transfer is not None and args.start_from_stage != "predict":
        parser.error("--dense_transfer belongs to --start_from_stage predict")
    if args.dense_size < 2:
        parser.error("--dense_size must be at least 2")
    if args.dense_coarse is not None:
        if args.dense_coarse < 1 or args.dense_size % args.dense_coarse != 0:
            parser.error(f"--dense_coarse must divide --dense_size ({args.dense_size})")
        if not 2 <= args.dense_size // args.dense_coarse <= 8:
            parser.error("--dense_size / --dense_coarse must be in [2, 8]")
    if args.dense_radius is not None:
        if args.dense_coarse is None:
            parser.error("--dense_radius belongs to --dense_coarse SC")
        if not 1 <= args.dense_radius <= 16:
            parser.error("--dense_radius must be in [1, 16]")
    if args.track and args.start_from_stage != "predict":
        parser.error("--track belongs to --start_from_stage predict")
    if args.track_size < 2:
        parser.error("--track_size must be at least 2")
    if not 0.0 < args.track_sigma < float("inf"):
        parser.error("--track_sigma must be positive and finite")
    if args.track_radius is not None and not 1 <= args.track_radius <= 32:
        parser.error("--track_radius must be in [1, 32]")
    if args.propagate is not None and args.start_from_stage != "predict":
        parser.error("--propagate belongs to --start_from_stage predict")
    if args.propagate_size < 2:
        parser.error("--propagate_size must be at least 2")
    if args.propagate_size > 1024:
        parser.error("--propagate_size must be at most 1024")
    if not 1 <= args.propagate_radius <= 16:
        parser.error("--propagate_radius must be in [1, 16]")
    if not 1 <= args.propagate_k <= 16:
        parser.error("--propagate_k must be in [1, 16]")
    if not 0.0 < args.propagate_tau < float("inf"):
        parser.error("--propagate_tau must be positive and finite")
    if not 0 <= args.propagate_memory <= 63:
        parser.error("--propagate_memory must be in [0, 63]")
    from .launch import launcher_env, spawn_ranks
    # torch.cuda.device_count() does not initialise HIP on this image, so the ranks can still start
    n = ranks_to_start(args, torch.cuda.device_count(), launcher_env())
    if n > 1:
        sys.exit(spawn_ranks(n, ["-m", "stablekeypoints_amd.main"], sys.argv[1:] if argv is None else list(argv)))
    from .eval import evaluate
    from .keypoint_regressor import (find_best_indices, precompute_all_keypoints, return_regressor,
                                     return_regressor_human36m, return_regressor_visible)
    from .optimize import optimize_embedding
    from .optimize_token import load_ldm
    from .visualize import visualize_attn_maps
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        args.device = f"cuda:{local}"
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    ldm, controllers, num_gpus = load_ldm(args.device, args.model_type, feature_upsample_res=args.feature_upsample_res)
    os.makedirs(args.save_folder, exist_ok=True)
    rank0 = int(os.environ.get("RANK", "0")) == 0
    if args.start_from_stage == "predict":
        return predict_stage(args, ldm, controllers)
    stage = STAGES.index(args.start_from_stage)
    common = dict(noise_level=args.noise_level, device=args.device, layers=args.layers, dataset_loc=args.dataset_loc,
                  dataset_name=args.dataset_name, controllers=controllers, num_gpus=num_gpus,
                  validation=args.validation)
    aug = dict(augment_degrees=args.augment_degrees, augment_scale=args.augment_scale,
               augment_translate=args.augment_translate)
    if stage <= 0:
        embedding = optimize_embedding(
            ldm, top_k_strategy=args.top_k_strategy, wandb_log=args.wandb, lr=args.lr, num_steps=int(args.num_steps),
            num_tokens=args.num_tokens, top_k=args.top_k, sigma=args.sigma,
            sharpening_loss_weight=args.sharpening_loss_weight,
            equivariance_attn_loss_weight=args.equivariance_attn_loss_weight, batch_size=args.batch_size,
            max_len=args.max_len, furthest_point_num_samples=args.furthest_point_num_samples, min_dist=args.min_dist,
            num_subjects=args.num_subjects, **common, **aug)
        if rank0:
            torch.save(embedding, os.path.join(args.save_folder, "embedding.pt"))
    else:
        embedding = _load(args.save_folder, "embedding.pt", args.device).detach()
    if stage <= 1:
        indices = find_best_indices(
            ldm, embedding, num_steps=args.num_indices, num_tokens=args.num_tokens, top_k=args.top_k,
            min_dist=args.min_dist, top_k_strategy=args.top_k_strategy,
            furthest_point_num_samples=args.furthest_point_num_samples, sigma=args.sigma,
            num_subjects=args.num_subjects, **common)
        if rank0:
            torch.save(indices, os.path.join(args.save_folder, "indices.pt"))
            print("indices:", indices.tolist(), flush=True)
        if args.visualize:   # main.py:271-292
            visualize_attn_maps(
                ldm, embedding, indices, noise_level=args.noise_level, num_tokens=args.num_tokens, layers=args.layers,
                num_points=args.top_k, augmentation_iterations=args.augmentation_iterations,
                dataset_loc=args.dataset_loc, save_folder=args.save_folder, visualize=args.visualize,
                device=args.device, dataset_name=args.dataset_name, controllers=controllers, num_gpus=num_gpus,
                max_loc_strategy=args.max_loc_strategy, validation=args.validation, **aug)
    else:
        indices = _load(args.save_folder, "indices.pt", args.device).detach()
    if stage <= 2:
        source, target, visible = precompute_all_keypoints(
            ldm, embedding, indices, augmentation_iterations=args.augmentation_iterations,
            max_num_points=args.max_num_points, max_loc_strategy=args.max_loc_strategy,
            save_folder=args.save_folder, **common, **aug)
        if rank0:
            torch.save(source, os.path.join(args.save_folder, "source_keypoints.pt"))
            torch.save(target, os.path.join(args.save_folder, "target_keypoints.pt"))
            torch.save(visible, os.path.join(args.save_folder, "visible.pt"))
    else:
        source = _load(args.save_folder, "source_keypoints.pt", args.device)
        target = _load(args.save_folder, "target_keypoints.pt", args.device)
        visible = _load(args.save_folder, "visible.pt", args.device)
    # regressor (main.py:334-367)
    X = source.cpu().numpy().reshape(source.shape[0], -1).astype(np.float64)
    Y = target.cpu().numpy().reshape(target.shape[0], -1).astype(np.float64)
    if args.evaluation_method in ("visible", "mean_average_error"):
        if visible is None:
            vis = np.ones_like(Y)
        else:
            vis = visible.unsqueeze(-1).repeat(1, 1, 2).reshape(visible.shape[0], -1).cpu().numpy().astype(np.float64)
        regressor = return_regressor_visible(X, Y, vis)
    elif args.evaluation_method == "orientation_invariant":
        regressor = return_regressor_human36m(X, Y)
    else:
        regressor = return_regressor(X, Y)
    regressor = torch.tensor(regressor).to(torch.float32)
    if rank0:
        torch.save(regressor, os.path.join(args.save_folder, "regressor.pt"))
    if args.visualize:   # main.py:370-391
        visualize_attn_maps(
            ldm, embedding, indices, num_tokens=args.num_tokens, layers=args.layers, noise_level=args.noise_level,
            num_points=args.top_k, regressor=regressor.to(args.device), dataset_loc=args.dataset_loc,
            save_folder=args.save_folder, device=args.device, dataset_name=args.dataset_name,
            controllers=controllers, num_gpus=num_gpus, max_loc_strategy=args.max_loc_strategy,
            validation=args.validation, augmentation_iterations=args.augmentation_iterations, **aug)
    evaluate(ldm, embedding, indices, regressor.to(args.device), num_tokens=args.num_tokens,
             augmentation_iterations=args.augmentation_iterations, save_folder=args.save_folder,
             evaluation_method=args.evaluation_method, max_loc_strategy=args.max_loc_strategy, **common, **aug)


if __name__ == "__main__":
    main()
