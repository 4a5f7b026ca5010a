"""Dev probe: skp_render_sheet / skp_map_range at the reference's job sizes, against the byte model.

Keypoint sheet: 99 tiles (11 × 9) of 512² at downscale 4 with ten markers (visualize.py:105-138).
Heat sheet: 2 × 10 tiles of 512² at downscale 1, the bottom row under a 512² map (:40-73).
Each launch sits between two HIP events; the median of ``--iters`` launches after ``--warmup`` is
reported next to the floor: bytes read per source pixel plus bytes written per output pixel, at
the measured copy rate (DESIGN: 6.29 TB/s).  Variants without markers / without the overlay show
which phase costs.  Usage: python tools/render_time.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stablekeypoints_amd import ops
from stablekeypoints_amd._lib import call, ptr, stream

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


def sheet_bytes(n, H, W, f, rows, cols, pad, heat_tiles=0, map_bytes_per_px=4):
    Hs, Ws = ops.sheet_shape(H, W, rows, cols, f, pad)
    return n * H * W * 12 + heat_tiles * H * W * map_bytes_per_px + Hs * Ws * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    torch.manual_seed(0)
    rows = []

    def record(name, f, nbytes):
        med, lo, hi = median_us(f, a.warmup, a.iters)
        floor = nbytes / COPY_RATE * 1e6
        rows.append(dict(name=name, median_us=round(med, 2), min_us=round(lo, 2), max_us=round(hi, 2), bytes=nbytes,
                         floor_us=round(floor, 2), ratio_to_floor=round(med / floor, 2),
                         achieved_TBps=round(nbytes / med / 1e6, 3)))
        print(json.dumps(rows[-1]), flush=True)

    def sheet(images, maps, points, rows_, cols_, f, overlay=None, pad=2):
        """The bare skp_render_sheet launch on prepared buffers (range from skp_map_range, once)."""
        n, _, H, W = images.shape
        rng = lut = colors = None
        h = w = K = 0
        if maps is not None:
            h, w = maps.shape[1:]
            rng = ops.map_range(maps)
            if overlay is not None:
                rng[~torch.tensor(overlay, device=DEV)] = float("nan")
            lut = ops.default_lut().to(DEV)
        if points is not None:
            K = points.shape[1]
            colors = ops.default_colors(K).to(DEV)
        Hs, Ws = ops.sheet_shape(H, W, rows_, cols_, f, pad)
        out = torch.empty(Hs, Ws, 3, device=DEV, dtype=torch.uint8)
        radius = max(2.0, (H // f) / 32.0)
        keep.append((rng, lut, colors, out))
        return lambda: call("skp_render_sheet", ptr(images), n, H, W, ptr(maps), h, w, ptr(rng), ptr(lut), 0.7,
                            ptr(points), K, radius, ptr(colors), rows_, cols_, f, pad, ptr(out), stream(DEV))

    keep = []
    # keypoint sheet
    imgs = torch.rand(99, 3, 512, 512, device=DEV)
    pts = torch.rand(99, 10, 2, device=DEV)
    nb = sheet_bytes(99, 512, 512, 4, 11, 9, 2)
    record("keypoint_sheet_99x512_f4_10markers", sheet(imgs, None, pts, 11, 9, 4), nb)
    record("keypoint_sheet_99x512_f4_no_markers", sheet(imgs, None, None, 11, 9, 4), nb)
    del imgs, pts
    keep.clear()
    # heat sheet
    ten = torch.rand(10, 3, 512, 512, device=DEV)
    two = torch.cat([ten, ten])
    maps = torch.rand(20, 512, 512, device=DEV)
    over = [False] * 10 + [True] * 10
    record("heat_sheet_2x10x512_f1", sheet(two, maps, None, 2, 10, 1, over),
           sheet_bytes(20, 512, 512, 1, 2, 10, 2, heat_tiles=10))
    record("heat_sheet_2x10x512_f1_plain", sheet(two, None, None, 2, 10, 1), sheet_bytes(20, 512, 512, 1, 2, 10, 2))
    record("heat_sheet_2x10x512_f1_all_overlaid", sheet(two, maps, None, 2, 10, 1),
           sheet_bytes(20, 512, 512, 1, 2, 10, 2, heat_tiles=20))
    half = maps[:, ::2, ::2].contiguous()
    record("heat_sheet_2x10x512_f1_map256_upsampled", sheet(two, half, None, 2, 10, 1, over),
           sheet_bytes(20, 512, 512, 1, 2, 10, 2, heat_tiles=10, map_bytes_per_px=1))
    rng = torch.empty(20, 2, device=DEV)
    record("map_range_20x512x512", lambda: call("skp_map_range", ptr(maps), 20, 512, 512, ptr(rng), stream(DEV)),
           20 * 512 * 512 * 4)
    record("ops_render_sheet_heat_2x10x512_f1_whole_wrapper",
           lambda: ops.render_sheet(two, maps, None, rows=2, cols=10, overlay=over),
           sheet_bytes(20, 512, 512, 1, 2, 10, 2, heat_tiles=10) + 20 * 512 * 512 * 4)
    res = dict(device=torch.cuda.get_device_name(0), copy_rate_Bps=COPY_RATE, warmup=a.warmup, iters=a.iters,
               note="one launch between two HIP events, median of iters; bytes = 12 per source pixel + 4 per "
                    "overlaid source pixel (1 for the 256² map) + 3 per sheet pixel; the last row is the whole "
                    "ops.render_sheet wrapper (skp_map_range over 20 maps + mask + launch, host time included)",
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
