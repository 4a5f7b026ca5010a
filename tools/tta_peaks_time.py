"""Dev probe: skp_tta_reduce_peaks at the TTA job sizes, against skp_tta_reduce and against the
composition that yields the same outputs without it.

Shapes (B, C, n, S) = (1, 10, 10, 512) and (4, 10, 10, 512), num 2 and 3, the reference's radius
0.05 · S, no average written by (a) or (b).  Each row is the median of ``--iters`` after
``--warmup``, the launches between two HIP events, in one process:
  (a) skp_tta_reduce;
  (b) skp_tta_reduce_peaks;
  (c) the composition: ops.tta_reduce(return_avg=True), then ops.find_k_max_pixels on the average.
(a) is timed twice, before and after (b): the difference of its two medians is the run-to-run
spread that (b) against (c) is read with.  (c) yields the positions only; whether (b)'s positions
equal them is recorded beside the times.

Kernel times come from a run of their own: under ``rocprofv3 --kernel-trace`` with ``--trace-only``
this tool only launches (a) and (b) a few times per shape and num, and ``--kernel-trace FILE.csv``
folds that trace's per-kernel medians into the result.
Usage: python tools/tta_peaks_time.py [--out FILE.json] [--kernel-trace kernel_trace.csv]
       rocprofv3 --kernel-trace -d DIR -o tta --output-format csv -- python tools/tta_peaks_time.py --trace-only
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
NUMS = (2, 3)


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


def composition(maps, theta, num):
    """The positions of tta_reduce_peaks from the ops that exist without it: (B, n, num, 2)."""
    B, C, n, S, _ = maps.shape
    _, avg = ops.tta_reduce(maps, theta, return_avg=True)
    return ops.find_k_max_pixels(avg.reshape(B * n, S, S), num).permute(1, 0, 2).reshape(B, n, num, 2)


def kernel_medians(path):
    """Per kernel and grid (work-items; the two shapes differ in it): the median duration in µs."""
    by = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            key = next((k for k in ("tta_masked_tile_kernel", "tta_merge_peaks_kernel", "tta_merge_kernel",
                                    "tta_tile_kernel") if k in name), None)
            if key is None:
                continue
            grid = "x".join(str(row.get(f"Grid_Size_{d}", "?")) for d in "XY")
            by.setdefault(f"{key}_grid{grid}", []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(median_us=round(statistics.median(v), 2), launches=len(v)) for k, v in sorted(by.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="launch (a) and (b) 20 times per shape and num and exit")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of a --trace-only run")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
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
        radius2 = ops._radius2(S)
        ws = torch.empty(lib().skp_tta_reduce_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        pos = torch.empty(B, n, 2, device=DEV)

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
                for _ in range(20):
                    plain()
                    peaks()
                torch.cuda.synchronize()
                continue
            tag = f"B{B}_C{C}_n{n}_S{S}_num{num}"
            a1 = record(f"a_skp_tta_reduce_{tag}", plain, ops.tta_reduce_bytes(B, C, n, S))
            b_ = record(f"b_skp_tta_reduce_peaks_{tag}", peaks, ops.tta_reduce_peaks_bytes(B, C, n, S, num))
            a2 = record(f"a_again_skp_tta_reduce_{tag}", plain, ops.tta_reduce_bytes(B, C, n, S))
            # (c) moves the fused reduce with the average written, then reads the average num times
            comp_bytes = ops.tta_reduce_bytes(B, C, n, S, True) + 4 * B * n * S * S * num
            c_ = record(f"c_composition_{tag}", lambda: composition(maps, theta, num), comp_bytes)
            got = ops.tta_reduce_peaks(maps, theta, num)[0]
            same = bool(torch.equal(got, composition(maps, theta, num)))
            a_, spread = min(a1, a2), abs(a1 - a2)
            summary.append(dict(shape=[B, C, n, S], num=num, a_us=round(a_, 2), a_spread_us=round(spread, 2),
                                b_us=round(b_, 2), c_us=round(c_, 2), b_minus_a_us=round(b_ - a_, 2),
                                b_over_c=round(b_ / c_, 3), b_no_slower_than_c=bool(b_ <= c_ + spread),
                                positions_agree=same))
            print(json.dumps(summary[-1]), flush=True)
        del maps
    if a.trace_only:
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters,
               note="median of iters, launches between two HIP events; a = skp_tta_reduce (the lower of two medians, "
                    "their difference = a_spread), b = skp_tta_reduce_peaks, c = the composition ops.tta_reduce("
                    "return_avg=True) + ops.find_k_max_pixels (host time between its launches included); no average "
                    "written by a or b; b_no_slower_than_c: b <= c + a_spread; kernels = per-kernel medians of a kernel "
                    "trace taken in a run of its own",
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
