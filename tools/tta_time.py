"""Dev probe: the TTA reduces at the TTA job sizes, one subcommand each.

Shapes (B, C, n, S) = (1, 10, 10, 512) and (4, 10, 10, 512); ``entropy`` takes the selection's shapes.  Each row is the median of ``--iters``
after ``--warmup``, the launches between two HIP events, in one process.

``reduce``: skp_tta_reduce with and without the average written, against the byte model and against
the composition run_image_with_context_augmented performs today.  The floor is 4·B·C·n·S² bytes
read (+ 4·B·n·S² written with the average) at the measured copy rate (DESIGN: 6.29 TB/s).  The
composition on the same inputs, per image: the two ``inverse`` warps (maps and ones), the two sums
over the copies, the divide, the NaN fix and find_max_pixel.

``scored`` (distance 5) and ``peaks`` (num 2 and 3, the reference's radius 0.05 · S), no average
written by (a) or (b):
  (a) skp_tta_reduce;
  (b) skp_tta_reduce_scored, or skp_tta_reduce_peaks;
  (c) the composition that yields (b)'s outputs from the ops that exist without it.  scored:
      ops.tta_reduce(return_avg=True), ops.pixel_from_weighted_avg on a clone (which leaves the
      disc), the float64 sums of the average and of the disc, the peak gathered from the average and
      num (the summed warps of a plane of ones) gathered at the peak.  peaks:
      ops.tta_reduce(return_avg=True), then ops.find_k_max_pixels on the average (the positions
      only; whether (b)'s positions equal them is recorded beside the times).
``entropy`` (scale 1) at (1, 10, 500, 128), (4, 10, 500, 128) (a whole embedding at the selection's
size) and (1, 10, 10, 512), the same scheme: (b) skp_tta_reduce_entropy, (c) ops.tta_reduce(
return_avg=True) then ops.entropy_keys_batch on the average (the entropy of the reference's fp32
arithmetic; how far (b)'s double one-pass entropy is from it is recorded beside the times).
``parts`` at (1, 10, 10, 512), (4, 10, 10, 512), (1, 10, 500, 128) and (4, 10, 500, 128), the same scheme:
(b) skp_tta_reduce_parts, (c) ops.tta_reduce(return_avg=True), then ``avg.max(dim=1)`` and the sum over the
tokens chunk by chunk in torch (one reduction over each chunk's 10 tokens, one over the chunks); whether
(b)'s labels, values and positions equal (c)'s, and how far its mass is from (c)'s, is recorded beside the
times.
``match`` (Q = 16 unit queries) at the same four shapes, the same scheme: (b) skp_tta_reduce_match without the
score map, (c) ops.tta_reduce(return_avg=True), then in torch the (Q × n)·(n × S²) product, the norm over the
tokens, the division, the −inf rule and the argmax; whether (b)'s positions equal (c)'s and how far its
scores are from (c)'s (torch sums in its own order) is recorded beside the times, and each row of the
summary carries the byte model's floor and the share of the per-chunk sums in the maps' bytes.
(a) is timed twice, before and after (b): the difference of its two medians is the run-to-run
spread that (b) − (a), and (b) against (c), are read with.

Kernel times of ``scored`` and ``peaks`` come from a run of their own: under ``rocprofv3
--kernel-trace`` with ``--trace-only`` the subcommand only launches (a) and (b) a few times per
shape (and num), and ``--kernel-trace FILE.csv`` folds that trace's per-kernel medians into the
result.
Usage: python tools/tta_time.py {reduce,scored,peaks,entropy,parts,match} [--out FILE.json] [--kernel-trace kernel_trace.csv]
       rocprofv3 --kernel-trace -d DIR -o tta --output-format csv -- python tools/tta_time.py scored --trace-only
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stablekeypoints_amd import ops
from stablekeypoints_amd._lib import call, lib, ptr, stream

COPY_RATE = 6.29e12   # B/s, DESIGN.md
DEV = "cuda:0"
SHAPES = ((1, 10, 10, 512), (4, 10, 10, 512))
DISTANCE = 5.0
NUMS = (2, 3)
ENTROPY_SHAPES = ((1, 10, 500, 128), (4, 10, 500, 128), (1, 10, 10, 512))
PARTS_SHAPES = ((1, 10, 10, 512), (4, 10, 10, 512), (1, 10, 500, 128), (4, 10, 500, 128))
# kernel and template argument -> the name its medians go by in each subcommand's result
SCORED_KERNELS = {"tta_window_kernel": "window", "tta_merge_kernel<kScored>": "merge_scored",
                  "tta_merge_kernel<kPlain>": "merge_plain", "tta_tile_kernel<true>": "tile_scored",
                  "tta_tile_kernel<false>": "tile_plain"}
PEAKS_KERNELS = {"tta_masked_tile_kernel": "tta_masked_tile_kernel", "tta_merge_kernel<kPeaks>": "tta_merge_peaks_kernel",
                 "tta_merge_kernel<kPlain>": "tta_merge_kernel", "tta_tile_kernel<false>": "tta_tile_kernel"}
ENTROPY_KERNELS = {"tta_tile_entropy_kernel": "tile_entropy", "tta_merge_kernel<kEntropy>": "merge_entropy",
                   "tta_merge_kernel<kPlain>": "merge_plain", "tta_tile_kernel<false>": "tile_plain"}
PARTS_KERNELS = {"tta_tile_parts_kernel": "tile_parts", "tta_parts_merge_kernel": "merge_parts",
                 "tta_merge_kernel<kPlain>": "merge_plain", "tta_tile_kernel<false>": "tile_plain"}
MATCH_QUERIES = 16
MATCH_KERNELS = {"tta_tile_match_kernel": "tile_match", "tta_match_merge_kernel": "merge_match",
                 "tta_merge_kernel<kPlain>": "merge_plain", "tta_tile_kernel<false>": "tile_plain"}


def median_us(f, warmup, iters):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        f()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return statistics.median(t), min(t), max(t)


def record(a, rows, name, f, nbytes, floor=False):
    med, lo, hi = median_us(f, a.warmup, a.iters)
    row = dict(name=name, median_us=round(med, 2), min_us=round(lo, 2), max_us=round(hi, 2), bytes=nbytes)
    if floor:
        us = nbytes / COPY_RATE * 1e6
        row.update(floor_us=round(us, 2), ratio_to_floor=round(med / us, 2), achieved_TBps=round(nbytes / med / 1e6, 3))
    rows.append(row)
    print(json.dumps(row), flush=True)
    return med


def cases(shapes=SHAPES):
    """Per shape: the shape, random maps, the inverse thetas of seeded random affines, and the plain
    reduce's workspace and position buffer."""
    torch.manual_seed(0)
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    T = RandomAffineWithInverse(degrees=30, scale=(0.9, 1.1), translate=(0.1, 0.1))
    for B, C, n, S in shapes:
        maps = torch.rand(B, C, n, S, S, device=DEV)
        T.last_params = {"theta": T.draw_theta(B * C)}
        theta = T.theta_inverse().reshape(B, C, 2, 3).to(DEV)
        ws = torch.empty(lib().skp_tta_reduce_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        yield (B, C, n, S), maps, theta, ws, torch.empty(B, n, 2, device=DEV)


def kernel_medians(path, names):
    """Per kernel of ``names`` and grid (work-items; the two shapes differ in it): the median duration in µs."""
    by = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            kernel = next((k for k in ("tta_window_kernel", "tta_masked_tile_kernel", "tta_merge_kernel",
                                       "tta_tile_kernel", "tta_tile_entropy_kernel", "tta_tile_parts_kernel",
                                       "tta_parts_merge_kernel", "tta_tile_match_kernel", "tta_match_merge_kernel")
                           if k in name), None)
            if kernel == "tta_tile_kernel":     # the template argument, demangled or mangled
                kernel += "<true>" if ("<true>" in name or "ILb1" in name) else "<false>"
            elif kernel == "tta_merge_kernel":
                kernel += "<" + ("kPlain", "kScored", "kPeaks", "kEntropy")[int(re.search(r"Variant\)?E?([0123])", name).group(1))] + ">"
            if kernel not in names:
                continue
            grid = "x".join(str(row.get(f"Grid_Size_{d}", "?")) for d in ("XYZ" if "entropy" in kernel or "parts" in kernel or "match" in kernel else "XY"))
            by.setdefault(f"{names[kernel]}_grid{grid}", []).append(
                (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(median_us=round(statistics.median(v), 2), launches=len(v)) for k, v in sorted(by.items())}


def write(a, res, names=None):
    if names and a.kernel_trace:
        res["kernels"] = kernel_medians(a.kernel_trace, names)
        print(json.dumps(res["kernels"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


# ------------------------------------------------------------------------------------------ reduce
def reduce_composition(maps, theta):
    """What run_image_with_context_augmented does with one image's captured maps (eval.py:327-355)
    and its callers do next (find_max_pixel), image by image."""
    out = []
    for b in range(maps.shape[0]):
        num = ops.affine_warp(torch.ones_like(maps[b]), theta[b]).sum(dim=0)
        a = ops.affine_warp(maps[b], theta[b]).sum(dim=0) / num
        a[a != a] = 0
        out.append(ops.find_max_pixel(a))
    return out


def run_reduce(a):
    rows = []
    for (B, C, n, S), maps, theta, ws, pos in cases():
        avg = torch.empty(B, n, S, S, device=DEV)
        tag = f"B{B}_C{C}_n{n}_S{S}"
        fused = {}
        for with_avg in (False, True):
            fused[with_avg] = record(
                a, rows, f"skp_tta_reduce_{tag}" + ("_avg" if with_avg else ""),
                lambda: call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos),
                             ptr(avg) if with_avg else None, ptr(ws), stream(DEV)),
                ops.tta_reduce_bytes(B, C, n, S, with_avg), floor=True)
        # the composition moves: maps read, warped written and read back by the sum; ones written, read,
        # warped written and read back; then the (n, S, S) sums through divide, NaN fix and argmax
        comp_bytes = B * (4 * C * n * S * S * 7 + 4 * n * S * S * 9)
        comp = record(a, rows, f"composition_{tag}", lambda: reduce_composition(maps, theta), comp_bytes, floor=True)
        rows[-1]["fused_over_composition"] = round(fused[False] / comp, 3)
        rows[-1]["fused_avg_over_composition"] = round(fused[True] / comp, 3)
        same = all(torch.equal(p, q) for p, q in zip(reduce_composition(maps, theta), ops.tta_reduce(maps, theta)[0]))
        rows[-1]["same_keypoints"] = bool(same)
        print(json.dumps(rows[-1]), flush=True)
    write(a, dict(device=torch.cuda.get_device_name(0), copy_rate_Bps=COPY_RATE, warmup=a.warmup, iters=a.iters,
                  note="skp_tta_reduce rows: the two launches between two HIP events, median of iters; bytes = "
                       "4·B·C·n·S² read (+ 4·B·n·S² with avg).  composition rows: per image, two affine_warp "
                       "launches, two sum(0), divide, NaN fix, find_max_pixel (host time between launches included); "
                       "bytes = its own traffic model (7 passes over the copies' maps and ones, 9 over the sums)",
                  rows=rows))


# ------------------------------------------------------------------------------------------ scored and peaks
def a_b_a_c(a, rows, tag, b_name, plain, fused, composition, plain_bytes, fused_bytes, comp_bytes):
    """(a), (b), (a) again, (c) -> the lower (a), the spread of the two, (b), (c)."""
    a1 = record(a, rows, f"a_skp_tta_reduce_{tag}", plain, plain_bytes)
    b_ = record(a, rows, f"b_{b_name}_{tag}", fused, fused_bytes)
    a2 = record(a, rows, f"a_again_skp_tta_reduce_{tag}", plain, plain_bytes)
    c_ = record(a, rows, f"c_composition_{tag}", composition, comp_bytes)
    return min(a1, a2), abs(a1 - a2), b_, c_


def trace(plain, fused):
    for _ in range(20):
        plain()
        fused()
    torch.cuda.synchronize()


def scored_composition(maps, theta, distance):
    """The outputs of tta_reduce_scored from the ops that exist without it."""
    B, C, n, S, _ = maps.shape
    pos, avg = ops.tta_reduce(maps, theta, return_avg=True)
    disc = avg.clone().reshape(B * n, S, S)
    refined = ops.pixel_from_weighted_avg(disc, distance).reshape(B, n, 2)     # zeroes `disc` outside the disc
    total = avg.sum(dim=(2, 3), dtype=torch.float64)
    conc = (disc.sum(dim=(1, 2), dtype=torch.float64).reshape(B, n) / (total + 1e-6)).float()
    idx = ((pos[..., 0] - 0.5) * S + (pos[..., 1] - 0.5)).long()
    peak = avg.reshape(B, n, S * S).gather(2, idx[..., None])[..., 0]
    ones = torch.ones(1, 1, S, S, device=maps.device)
    num = torch.stack([sum(ops.affine_warp(ones, theta[b, c][None])[0, 0] for c in range(C)) for b in range(B)])
    cov = num.reshape(B, 1, S * S).expand(B, n, S * S).gather(2, idx[..., None])[..., 0] / C
    return pos, refined, torch.stack([peak, conc, cov], dim=-1)


def run_scored(a):
    rows, summary = [], []
    for (B, C, n, S), maps, theta, ws, pos in cases():
        wss = torch.empty(lib().skp_tta_reduce_scored_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        refined, scores = torch.empty(B, n, 2, device=DEV), torch.empty(B, n, 3, device=DEV)

        def plain():
            call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos), None, ptr(ws), stream(DEV))

        def scored():
            call("skp_tta_reduce_scored", ptr(maps), B, C, n, S, ptr(theta), DISTANCE, ptr(pos), ptr(refined),
                 ptr(scores), None, ptr(wss), stream(DEV))

        if a.trace_only:
            trace(plain, scored)
            continue
        # (c) moves the fused reduce with the average written, then the average: cloned (read + write), read twice
        # and partly zeroed by the centroid op, read by the two sums and the gathers; and the C warps of ones
        comp_bytes = ops.tta_reduce_bytes(B, C, n, S, True) + 4 * B * n * S * S * 6 + 4 * B * C * S * S * 4
        a_, spread, b_, c_ = a_b_a_c(a, rows, f"B{B}_C{C}_n{n}_S{S}", "skp_tta_reduce_scored", plain, scored,
                                     lambda: scored_composition(maps, theta, DISTANCE), ops.tta_reduce_bytes(B, C, n, S),
                                     ops.tta_reduce_scored_bytes(B, C, n, S, DISTANCE), comp_bytes)
        got = ops.tta_reduce_scored(maps, theta, distance=DISTANCE)
        want = scored_composition(maps, theta, DISTANCE)
        same = dict(pos=bool(torch.equal(got[0], want[0])),
                    refined_max_abs=float((got[1] - want[1]).abs().max()),
                    peak=bool(torch.equal(got[2][..., 0], want[2][..., 0])),
                    concentration_max_rel=float(((got[2][..., 1] - want[2][..., 1]).abs() / want[2][..., 1]).max()),
                    coverage_max_abs=float((got[2][..., 2] - want[2][..., 2]).abs().max()))
        summary.append(dict(shape=[B, C, n, S], a_us=round(a_, 2), a_spread_us=round(spread, 2), b_us=round(b_, 2),
                            c_us=round(c_, 2), b_minus_a_us=round(b_ - a_, 2), b_over_c=round(b_ / c_, 3),
                            b_no_slower_than_c=bool(b_ <= c_), agreement=same))
        print(json.dumps(summary[-1]), flush=True)
    if a.trace_only:
        return
    write(a, dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, distance=DISTANCE,
                  note="median of iters, launches between two HIP events; a = skp_tta_reduce (the lower of two medians, "
                       "their difference = a_spread), b = skp_tta_reduce_scored, c = the composition (host time between "
                       "its launches included); no average written by a or b; kernels = per-kernel medians of a "
                       "kernel trace taken in a run of its own",
                  summary=summary, rows=rows), SCORED_KERNELS)


def peaks_composition(maps, theta, num):
    """The positions of tta_reduce_peaks from the ops that exist without it: (B, n, num, 2)."""
    B, C, n, S, _ = maps.shape
    _, avg = ops.tta_reduce(maps, theta, return_avg=True)
    return ops.find_k_max_pixels(avg.reshape(B * n, S, S), num).permute(1, 0, 2).reshape(B, n, num, 2)


def run_peaks(a):
    rows, summary = [], []
    for (B, C, n, S), maps, theta, ws, pos in cases():
        radius2 = ops._radius2(S)

        def plain():
            call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos), None, ptr(ws), stream(DEV))

        for num in NUMS:
            wsp = torch.empty(lib().skp_tta_reduce_peaks_workspace(B, n, S, num, radius2) // 8, device=DEV,
                              dtype=torch.int64)
            ppos, pval = torch.empty(B, n, num, 2, device=DEV), torch.empty(B, n, num, device=DEV)

            def peaks():
                call("skp_tta_reduce_peaks", ptr(maps), B, C, n, S, ptr(theta), num, radius2, ptr(ppos), ptr(pval),
                     None, ptr(wsp), stream(DEV))

            if a.trace_only:
                trace(plain, peaks)
                continue
            # (c) moves the fused reduce with the average written, then reads the average num times
            comp_bytes = ops.tta_reduce_bytes(B, C, n, S, True) + 4 * B * n * S * S * num
            a_, spread, b_, c_ = a_b_a_c(a, rows, f"B{B}_C{C}_n{n}_S{S}_num{num}", "skp_tta_reduce_peaks", plain, peaks,
                                         lambda: peaks_composition(maps, theta, num), ops.tta_reduce_bytes(B, C, n, S),
                                         ops.tta_reduce_peaks_bytes(B, C, n, S, num), comp_bytes)
            got = ops.tta_reduce_peaks(maps, theta, num)[0]
            same = bool(torch.equal(got, peaks_composition(maps, theta, num)))
            summary.append(dict(shape=[B, C, n, S], num=num, a_us=round(a_, 2), a_spread_us=round(spread, 2),
                                b_us=round(b_, 2), c_us=round(c_, 2), b_minus_a_us=round(b_ - a_, 2),
                                b_over_c=round(b_ / c_, 3), b_no_slower_than_c=bool(b_ <= c_ + spread),
                                positions_agree=same))
            print(json.dumps(summary[-1]), flush=True)
    if a.trace_only:
        return
    write(a, dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters,
                  note="median of iters, launches between two HIP events; a = skp_tta_reduce (the lower of two medians, "
                       "their difference = a_spread), b = skp_tta_reduce_peaks, c = the composition ops.tta_reduce("
                       "return_avg=True) + ops.find_k_max_pixels (host time between its launches included); no average "
                       "written by a or b; b_no_slower_than_c: b <= c + a_spread; kernels = per-kernel medians of a kernel "
                       "trace taken in a run of its own",
                  summary=summary, rows=rows), PEAKS_KERNELS)


# ------------------------------------------------------------------------------------------ entropy
def entropy_composition(maps, theta):
    """The outputs of tta_reduce_entropy from the ops that exist without it: the average written, then
    its softmax entropies (four passes over it)."""
    pos, avg = ops.tta_reduce(maps, theta, return_avg=True)
    return pos, ops.entropy_keys_batch(avg)


def run_entropy(a):
    rows, summary = [], []
    for (B, C, n, S), maps, theta, ws, pos in cases(ENTROPY_SHAPES):
        wse = torch.empty(lib().skp_tta_reduce_entropy_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        ent = torch.empty(B, n, device=DEV, dtype=torch.float64)

        def plain():
            call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos), None, ptr(ws), stream(DEV))

        def entropy():
            call("skp_tta_reduce_entropy", ptr(maps), B, C, n, S, ptr(theta), 1.0, ptr(pos), ptr(ent), None, ptr(wse),
                 stream(DEV))

        if a.trace_only:
            trace(plain, entropy)
            continue
        # (c) moves the fused reduce with the average written, then reads the average four times
        comp_bytes = ops.tta_reduce_bytes(B, C, n, S, True) + 4 * B * n * S * S * 4
        a_, spread, b_, c_ = a_b_a_c(a, rows, f"B{B}_C{C}_n{n}_S{S}", "skp_tta_reduce_entropy", plain, entropy,
                                     lambda: entropy_composition(maps, theta), ops.tta_reduce_bytes(B, C, n, S),
                                     ops.tta_reduce_entropy_bytes(B, C, n, S), comp_bytes)
        got_pos, got_ent, _ = ops.tta_reduce_entropy(maps, theta)
        want_pos, want_ent = entropy_composition(maps, theta)
        summary.append(dict(shape=[B, C, n, S], a_us=round(a_, 2), a_spread_us=round(spread, 2), b_us=round(b_, 2),
                            c_us=round(c_, 2), b_minus_a_us=round(b_ - a_, 2), b_over_c=round(b_ / c_, 3),
                            b_below_c_by_more_than_spread=bool(b_ < c_ - spread),
                            pos_agree=bool(torch.equal(got_pos, want_pos)),
                            entropy_max_abs_vs_fp32_order=float((got_ent - want_ent).abs().max())))
        print(json.dumps(summary[-1]), flush=True)
    if a.trace_only:
        return
    write(a, dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, scale=1.0,
                  note="median of iters, launches between two HIP events; a = skp_tta_reduce (the lower of two medians, "
                       "their difference = a_spread), b = skp_tta_reduce_entropy, c = the composition ops.tta_reduce("
                       "return_avg=True) + ops.entropy_keys_batch (host time between its launches included); no average "
                       "written by a or b; kernels = per-kernel medians of a kernel trace taken in a run of its own",
                  summary=summary, rows=rows), ENTROPY_KERNELS)


# ------------------------------------------------------------------------------------------ parts
def parts_composition(maps, theta, chunk=10):
    """The outputs of tta_reduce_parts from the ops that exist without it: the average written, its
    maximum and argmax over the tokens, and the tokens' sum chunk by chunk (each chunk's tokens in one
    reduction, then the chunks in one: the fewest launches that keep the chunked order of the adds)."""
    B, C, n, S, _ = maps.shape
    pos, avg = ops.tta_reduce(maps, theta, return_avg=True)
    value, label = avg.max(dim=1)
    if n % chunk == 0:
        mass = avg.view(B, n // chunk, chunk, S, S).sum(dim=2).sum(dim=1)
    else:
        mass = torch.stack([avg[:, t:t + chunk].sum(dim=1) for t in range(0, n, chunk)], dim=1).sum(dim=1)
    return pos, label, value, mass


def run_parts(a):
    rows, summary = [], []
    for (B, C, n, S), maps, theta, ws, pos in cases(PARTS_SHAPES):
        wsp = torch.empty(lib().skp_tta_reduce_parts_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        label = torch.empty(B, S, S, device=DEV, dtype=torch.int16)
        value, mass = torch.empty(B, S, S, device=DEV), torch.empty(B, S, S, device=DEV)

        def plain():
            call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos), None, ptr(ws), stream(DEV))

        def parts():
            call("skp_tta_reduce_parts", ptr(maps), B, C, n, S, ptr(theta), ptr(pos), ptr(label), ptr(value), ptr(mass),
                 None, ptr(wsp), stream(DEV))

        if a.trace_only:
            trace(plain, parts)
            continue
        # (c) moves the fused reduce with the average written, then reads the average twice (max, sum)
        comp_bytes = ops.tta_reduce_bytes(B, C, n, S, True) + 4 * B * n * S * S * 2
        a_, spread, b_, c_ = a_b_a_c(a, rows, f"B{B}_C{C}_n{n}_S{S}", "skp_tta_reduce_parts", plain, parts,
                                     lambda: parts_composition(maps, theta), ops.tta_reduce_bytes(B, C, n, S),
                                     ops.tta_reduce_parts_bytes(B, C, n, S), comp_bytes)
        got = ops.tta_reduce_parts(maps, theta)
        want = parts_composition(maps, theta)
        summary.append(dict(shape=[B, C, n, S], a_us=round(a_, 2), a_spread_us=round(spread, 2), b_us=round(b_, 2),
                            c_us=round(c_, 2), b_minus_a_us=round(b_ - a_, 2), b_over_a=round(b_ / a_, 3),
                            b_over_c=round(b_ / c_, 3), b_below_c_by_more_than_spread=bool(b_ < c_ - spread),
                            b_below_a=bool(b_ < a_),
                            pos_agree=bool(torch.equal(got[0], want[0])),
                            label_agree=bool(torch.equal(got[1].long(), want[1])),
                            value_agree=bool(torch.equal(got[2], want[2])),
                            mass_max_rel_vs_torch_order=float(((got[3] - want[3]).abs() / want[3].abs().clamp_min(1e-30)).max())))
        print(json.dumps(summary[-1]), flush=True)
    if a.trace_only:
        return
    write(a, dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters,
                  note="median of iters, launches between two HIP events; a = skp_tta_reduce (the lower of two medians, "
                       "their difference = a_spread), b = skp_tta_reduce_parts, c = the composition ops.tta_reduce("
                       "return_avg=True) + avg.max(dim=1) + the sum over the tokens chunk by chunk in torch (host time "
                       "between its launches included); no average written by a or b; label_agree compares with "
                       "torch.max's index, which is the first maximum on these continuous random maps; kernels = "
                       "per-kernel medians of a kernel trace taken in a run of its own",
                  summary=summary, rows=rows), PARTS_KERNELS)


# ------------------------------------------------------------------------------------------ match
def match_composition(maps, theta, queries):
    """The outputs of tta_reduce_match from the ops that exist without it: the average written, then in
    torch the queries' product with it, the norm over the tokens, the quotient, the −inf rule and the
    first maximum of every (image, query)."""
    B, C, n, S, _ = maps.shape
    pos, avg = ops.tta_reduce(maps, theta, return_avg=True)
    flat = avg.view(B, n, S * S)
    dot = torch.matmul(queries, flat)
    nrm = (flat * flat).sum(dim=1)
    score = dot / nrm.sqrt()[:, None]
    score = torch.where((nrm > 0)[:, None] & ~torch.isnan(score), score, torch.full_like(score, float("-inf")))
    value, idx = score.max(dim=2)
    return pos, torch.stack([idx // S + 0.5, idx % S + 0.5], dim=-1), value


def run_match(a):
    rows, summary = [], []
    Q = MATCH_QUERIES
    for (B, C, n, S), maps, theta, ws, pos in cases(PARTS_SHAPES):
        wsm = torch.empty(lib().skp_tta_reduce_match_workspace(B, n, S, Q) // 8, device=DEV, dtype=torch.int64)
        queries = torch.rand(Q, n, generator=torch.Generator().manual_seed(1)).to(DEV)
        queries = (queries / queries.norm(dim=1, keepdim=True)).contiguous()
        mpos, mscore = torch.empty(B, Q, 2, device=DEV), torch.empty(B, Q, device=DEV)

        def plain():
            call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos), None, ptr(ws), stream(DEV))

        def match():
            call("skp_tta_reduce_match", ptr(maps), B, C, n, S, ptr(theta), ptr(queries), Q, ptr(pos), ptr(mpos),
                 ptr(mscore), None, None, ptr(wsm), stream(DEV))

        if a.trace_only:
            trace(plain, match)
            continue
        # (c) moves the fused reduce with the average written, then reads the average twice (product, norm) and
        # passes six times over the (B, Q, S²) scores (product out, quotient in and out, −inf rule in and out, max in)
        comp_bytes = ops.tta_reduce_bytes(B, C, n, S, True) + 4 * B * n * S * S * 2 + 4 * B * Q * S * S * 6
        fused_bytes = ops.tta_reduce_match_bytes(B, C, n, S, Q)
        a_, spread, b_, c_ = a_b_a_c(a, rows, f"B{B}_C{C}_n{n}_S{S}", "skp_tta_reduce_match", plain, match,
                                     lambda: match_composition(maps, theta, queries), ops.tta_reduce_bytes(B, C, n, S),
                                     fused_bytes, comp_bytes)
        got = ops.tta_reduce_match(maps, theta, queries)
        want = match_composition(maps, theta, queries)
        chunks = (n + 9) // 10
        summary.append(dict(shape=[B, C, n, S], Q=Q, a_us=round(a_, 2), a_spread_us=round(spread, 2), b_us=round(b_, 2),
                            c_us=round(c_, 2), b_minus_a_us=round(b_ - a_, 2), b_over_a=round(b_ / a_, 3),
                            b_over_c=round(b_ / c_, 3), b_below_c_by_more_than_spread=bool(b_ < c_ - spread),
                            b_floor_us=round(fused_bytes / COPY_RATE * 1e6, 2),
                            b_over_floor=round(b_ / (fused_bytes / COPY_RATE * 1e6), 2),
                            chunk_sums_share_of_maps_bytes_each_way=round(
                                (Q + 1) * chunks / (C * n) if chunks > 1 else 0.0, 4),
                            pos_agree=bool(torch.equal(got[0], want[0])),
                            match_pos_agree=float((got[1] == want[1]).all(dim=-1).float().mean()),
                            match_score_max_abs_vs_torch_order=float((got[2] - want[2]).abs().max())))
        print(json.dumps(summary[-1]), flush=True)
    if a.trace_only:
        return
    write(a, dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, copy_rate_Bps=COPY_RATE,
                  note="median of iters, launches between two HIP events; a = skp_tta_reduce (the lower of two medians, "
                       "their difference = a_spread), b = skp_tta_reduce_match with Q = 16 queries and no score map, c = "
                       "the composition ops.tta_reduce(return_avg=True) + matmul, norm, quotient, -inf rule and max in "
                       "torch (host time between its launches included); no average written by a or b; b_floor = "
                       "ops.tta_reduce_match_bytes at the copy rate; match_pos_agree = the share of (image, query) "
                       "pairs whose position equals the composition's (torch sums in its own order); kernels = "
                       "per-kernel medians of a kernel trace taken in a run of its own",
                  summary=summary, rows=rows), MATCH_KERNELS)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="which", required=True)
    for name, run in (("reduce", run_reduce), ("scored", run_scored), ("peaks", run_peaks), ("entropy", run_entropy),
                      ("parts", run_parts), ("match", run_match)):
        p = sub.add_parser(name)
        p.set_defaults(run=run)
        p.add_argument("--out", default=None)
        p.add_argument("--warmup", type=int, default=10)
        p.add_argument("--iters", type=int, default=100)
        if name != "reduce":
            p.add_argument("--trace-only", action="store_true", help="launch (a) and (b) 20 times per shape and exit")
            p.add_argument("--kernel-trace", default=None, help="kernel trace CSV of a --trace-only run")
    a = ap.parse_args()
    a.run(a)


if __name__ == "__main__":
    main()
