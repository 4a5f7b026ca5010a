"""Dev probe: skp_tta_reduce at the TTA job sizes, against the byte model and against the composition
run_image_with_context_augmented performs today.

Shapes (B, C, n, S) = (1, 10, 10, 512) and (4, 10, 10, 512), with and without the average written.
Each launch pair sits between two HIP events; the median of ``--iters`` after ``--warmup`` is
reported next to the floor 4·B·C·n·S² bytes read (+ 4·B·n·S² written with ``avg``) at the measured
copy rate (DESIGN: 6.29 TB/s).  The composition on the same inputs, per image: the two ``inverse``
warps (maps and ones), the two sums over the copies, the divide, the NaN fix and find_max_pixel.
Usage: python tools/tta_time.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stablekeypoints_amd import ops
from stablekeypoints_amd._lib import call, lib, ptr, stream

COPY_RATE = 6.29e12   # B/s, DESIGN.md
DEV = "cuda:0"


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


def composition(maps, theta):
    """What run_image_with_context_augmented does with one image's captured maps (eval.py:327-355)
    and its callers do next (find_max_pixel), image by image."""
    out = []
    for b in range(maps.shape[0]):
        num = ops.affine_warp(torch.ones_like(maps[b]), theta[b]).sum(dim=0)
        a = ops.affine_warp(maps[b], theta[b]).sum(dim=0) / num
        a[a != a] = 0
        out.append(ops.find_max_pixel(a))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    torch.manual_seed(0)
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    T = RandomAffineWithInverse(degrees=30, scale=(0.9, 1.1), translate=(0.1, 0.1))
    rows = []

    def record(name, f, nbytes, **extra):
        med, lo, hi = median_us(f, a.warmup, a.iters)
        floor = nbytes / COPY_RATE * 1e6
        rows.append(dict(name=name, median_us=round(med, 2), min_us=round(lo, 2), max_us=round(hi, 2), bytes=nbytes,
                         floor_us=round(floor, 2), ratio_to_floor=round(med / floor, 2),
                         achieved_TBps=round(nbytes / med / 1e6, 3), **extra))
        print(json.dumps(rows[-1]), flush=True)
        return med

    for B, C, n, S in ((1, 10, 10, 512), (4, 10, 10, 512)):
        maps = torch.rand(B, C, n, S, S, device=DEV)
        T.last_params = {"theta": T.draw_theta(B * C)}
        theta = T.theta_inverse().reshape(B, C, 2, 3).to(DEV)
        ws = torch.empty(lib().skp_tta_reduce_workspace(B, n, S) // 8, device=DEV, dtype=torch.int64)
        pos = torch.empty(B, n, 2, device=DEV)
        avg = torch.empty(B, n, S, S, device=DEV)
        tag = f"B{B}_C{C}_n{n}_S{S}"
        fused = {}
        for with_avg in (False, True):
            fused[with_avg] = record(
                f"skp_tta_reduce_{tag}" + ("_avg" if with_avg else ""),
                lambda: call("skp_tta_reduce", ptr(maps), B, C, n, S, ptr(theta), ptr(pos),
                             ptr(avg) if with_avg else None, ptr(ws), stream(DEV)),
                ops.tta_reduce_bytes(B, C, n, S, with_avg))
        # the composition moves: maps read, warped written and read back by the sum; ones written, read,
        # warped written and read back; then the (n, S, S) sums through divide, NaN fix and argmax
        comp_bytes = B * (4 * C * n * S * S * 7 + 4 * n * S * S * 9)
        comp = record(f"composition_{tag}", lambda: composition(maps, theta), comp_bytes)
        rows[-1]["fused_over_composition"] = round(fused[False] / comp, 3)
        rows[-1]["fused_avg_over_composition"] = round(fused[True] / comp, 3)
        same = all(torch.equal(p, q) for p, q in zip(composition(maps, theta), ops.tta_reduce(maps, theta)[0]))
        rows[-1]["same_keypoints"] = bool(same)
        print(json.dumps(rows[-1]), flush=True)
        del maps, avg
    res = dict(device=torch.cuda.get_device_name(0), copy_rate_Bps=COPY_RATE, warmup=a.warmup, iters=a.iters,
               note="skp_tta_reduce rows: the two launches between two HIP events, median of iters; bytes = "
                    "4·B·C·n·S² read (+ 4·B·n·S² with avg).  composition rows: per image, two affine_warp "
                    "launches, two sum(0), divide, NaN fix, find_max_pixel (host time between launches included); "
                    "bytes = its own traffic model (7 passes over the copies' maps and ones, 9 over the sums)",
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
