"""Dev probe: skp_tta_reduce_scored at the TTA job sizes, against skp_tta_reduce and against the
composition that yields the same outputs without it.

Shapes (B, C, n, S) = (1, 10, 10, 512) and (4, 10, 10, 512), distance 5, no average written.  Each
row is the median of ``--iters`` after ``--warmup``, the launches between two HIP events, in one
process:
  (a) skp_tta_reduce;
  (b) skp_tta_reduce_scored;
  (c) the composition: ops.tta_reduce(return_avg=True), ops.pixel_from_weighted_avg on a clone
      (which leaves the disc), the float64 sums of the average and of the disc, the peak gathered
      from the average and num (the summed warps of a plane of ones) gathered at the peak.
(a) is timed twice, before and after (b): the difference of its two medians is the run-to-run
spread that (b) − (a) is read against.

Kernel times come from a run of their own: under ``rocprofv3 --kernel-trace`` with ``--trace-only``
this tool only launches (a) and (b) a few times per shape, and ``--kernel-trace FILE.csv`` folds that
trace's per-kernel medians into the result.
Usage: python tools/tta_score_time.py [--out FILE.json] [--kernel-trace kernel_trace.csv]
       rocprofv3 --kernel-trace -d DIR -o tta --output-format csv -- python tools/tta_score_time.py --trace-only
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stablekeypoints_amd import ops
from stablekeypoints_amd._lib import call, lib, ptr, stream

DEV = "cuda:0"
SHAPES = ((1, 10, 10, 512), (4, 10, 10, 512))
DISTANCE = 5.0


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


def composition(maps, theta, distance):
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


def kernel_medians(path):
    """Per kernel and grid (work-items; the two shapes differ in it): the median duration in µs."""
    by = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            if "tta_window_kernel" in name:
                key = "window"
            elif "tta_merge_scored_kernel" in name:
                key = "merge_scored"
            elif "tta_merge_kernel" in name:
                key = "merge_plain"
            elif "tta_tile_kernel" in name:
                key = "tile_scored" if ("<true>" in name or "ILb1" in name) else "tile_plain"
            else:
                continue
            grid = "x".join(str(row.get(f"Grid_Size_{d}", "?")) for d in "XY")
            by.setdefault(f"{key}_grid{grid}", []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(median_us=round(statistics.median(v), 2), launches=len(v)) for k, v in sorted(by.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--trace-only", action="store_true", help="launch (a) and (b) 20 times per shape and exit")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of a --trace-only run")
    a = ap.parse_args()
    torch.manual_seed(0)
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    T = RandomAffineWithInverse(degrees=30, scale=(0.9, 1.1), translate=(0.1, 0.1))
    rows, summary = [], []

    def record(name, f, nbytes, **extra):
        med, lo, hi = median_us(f, a.warmup, a.iters)
        rows.append(dict(name=name, median_us=round(med, 2), min_us=round(lo, 2), max_us=round(hi, 2), bytes=nbytes, **extra))
        print(json.dumps(rows[-1]), flush=True)
        return med

    for B, C, n, S in SHAPES:
        maps = torch.rand(B, C, n, S, S, device=DEV)
        T.last_params = {"theta": T.draw_theta(B * C)}
        theta = T.theta_inverse().reshape(B, C, 2, 3).to(DEV)
        ws = torch.empty(lib().skp_tta_reduce_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        wss = torch.empty(lib().skp_tta_reduce_scored_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        pos, refined, scores = (torch.empty(B, n, k, device=DEV) for k in (2, 2, 3))

        def plain():
            call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos), None, ptr(ws), stream(DEV))

        def scored():
            call("skp_tta_reduce_scored", ptr(maps), B, C, n, S, ptr(theta), DISTANCE, ptr(pos), ptr(refined),
                 ptr(scores), None, ptr(wss), stream(DEV))

        if a.trace_only:
            for _ in range(20):
                plain()
                scored()
            torch.cuda.synchronize()
            continue
        tag = f"B{B}_C{C}_n{n}_S{S}"
        a1 = record(f"a_skp_tta_reduce_{tag}", plain, ops.tta_reduce_bytes(B, C, n, S))
        b_ = record(f"b_skp_tta_reduce_scored_{tag}", scored, ops.tta_reduce_scored_bytes(B, C, n, S, DISTANCE))
        a2 = record(f"a_again_skp_tta_reduce_{tag}", plain, ops.tta_reduce_bytes(B, C, n, S))
        # (c) moves the fused reduce with the average written, then the average: cloned (read + write), read twice
        # and partly zeroed by the centroid op, read by the two sums and the gathers; and the C warps of ones
        comp_bytes = ops.tta_reduce_bytes(B, C, n, S, True) + 4 * B * n * S * S * 6 + 4 * B * C * S * S * 4
        c_ = record(f"c_composition_{tag}", lambda: composition(maps, theta, DISTANCE), comp_bytes)
        got = ops.tta_reduce_scored(maps, theta, distance=DISTANCE)
        want = composition(maps, theta, DISTANCE)
        same = dict(pos=bool(torch.equal(got[0], want[0])),
                    refined_max_abs=float((got[1] - want[1]).abs().max()),
                    peak=bool(torch.equal(got[2][..., 0], want[2][..., 0])),
                    concentration_max_rel=float(((got[2][..., 1] - want[2][..., 1]).abs() / want[2][..., 1]).max()),
                    coverage_max_abs=float((got[2][..., 2] - want[2][..., 2]).abs().max()))
        a_ = min(a1, a2)
        summary.append(dict(shape=[B, C, n, S], a_us=round(a_, 2), a_spread_us=round(abs(a1 - a2), 2), b_us=round(b_, 2),
                            c_us=round(c_, 2), b_minus_a_us=round(b_ - a_, 2), b_over_c=round(b_ / c_, 3),
                            b_no_slower_than_c=bool(b_ <= c_), agreement=same))
        print(json.dumps(summary[-1]), flush=True)
        del maps
    if a.trace_only:
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, distance=DISTANCE,
               note="median of iters, launches between two HIP events; a = skp_tta_reduce (the lower of two medians, "
                    "their difference = a_spread), b = skp_tta_reduce_scored, c = the composition (host time between "
                    "its launches included); no average written by a or b; kernels = per-kernel medians of a "
                    "kernel trace taken in a run of its own",
               summary=summary, rows=rows)
    if a.kernel_trace:
        res["kernels"] = kernel_medians(a.kernel_trace)
        print(json.dumps(res["kernels"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
