"""Dev probe: one frame of the keypoint tracker, ops.track_step (skp_track_step), against the same step
composed from torch ops.

Shapes (n, S, r) = (10, 128, 3), (10, 128, 8) and (10, 512, 8): a later frame (prev_score given), the case
every frame but the first is.  Each time is the median of ``--iters`` after ``--warmup``, the launches
between two HIP events, in one process (as tools/match_field_time.py takes them).

  (b) ops.track_step: the tile kernel (division, row stage and column stage from LDS, multiply, the
      tile's maximum) and the merge.  Timed twice, before and after (c)'s second run; the difference of
      its two medians is its run-to-run spread.
  (c) the composition: the division with the restart rule, the plane padded with the sentinel −1 and
      ``unfold``-ed along x, times the weights, ``max(dim=-1)``; the same along y; the gather of dx,
      the multiply, the code, and the plane's ``max``.  It writes and reads two (n, S, S, 2r + 1)
      products.  Timed before and after (b); the difference of its two medians is its spread.

Both are checked to agree bit for bit (score, score_max, best, back) on the timed inputs; the program
exits with status 1 after writing its result where they do not.  Beside the times: the byte-model
floor ``ops.track_step_bytes`` at 8 TB/s and the peak of ``torch.cuda.max_memory_allocated`` above
the inputs for (b) and (c).

Usage: python tools/track_time.py [--out profiles/track_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from stablekeypoints_amd import ops

DEV = "cuda:0"
SHAPES = ((10, 128, 3), (10, 128, 8), (10, 512, 8))
PEAK_BYTES = 8.0e12   # HBM3E, MI355X


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


def composition(avg, prev, prev_max, w):
    """(score, score_max, best, back) of track_step from torch: ``w`` (r + 1,) on the device."""
    n, S, _ = avg.shape
    r = w.numel() - 1
    side = 2 * r + 1
    ww = torch.cat([w.flip(0), w[1:]])                                         # ww[d + r] = w[|d|]
    live = (prev_max != 0) & torch.isfinite(prev_max)
    mt = torch.where(live[:, None, None], prev / prev_max[:, None, None], torch.ones_like(prev))
    g, kx = (F.pad(mt, (r, r), value=-1.0).unfold(2, side, 1) * ww).max(dim=-1)                # (n, S, S)
    h, ky = (F.pad(g, (0, 0, r, r), value=-1.0).unfold(1, side, 1) * ww).max(dim=-1)
    rows = torch.arange(S, device=avg.device)[None, :, None] + ky - r
    dx = torch.gather(kx, 1, rows)
    score = avg * h
    back = (ky * side + dx).to(torch.int16)
    score_max, best = score.reshape(n, -1).max(dim=1)
    return score, score_max, best.int(), back


def peak_extra_bytes(f):
    """The peak of the allocator above what is allocated before ``f`` runs."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8).reshape(-1),
                                                                     b.contiguous().view(torch.uint8).reshape(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    rows, summary = [], []
    for n, S, r in SHAPES:
        g = torch.Generator().manual_seed(S + r)
        # softmax-like planes: non-negative, a few strong pixels
        avg = torch.rand(n, S, S, generator=g).pow_(8).to(DEV)
        prev = torch.rand(n, S, S, generator=g).pow_(8).to(DEV)
        prev_max = prev.reshape(n, -1).max(dim=1).values.contiguous()
        w = ops.track_weights(r / 3.0, r)
        w_dev = w.to(DEV)
        state = (prev, prev_max, None, None)
        tag = f"n{n}_S{S}_r{r}"

        def record(name, f):
            med, lo, hi = median_us(f, a.warmup, a.iters)
            rows.append(dict(name=f"{name}_{tag}", median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1)))
            print(json.dumps(rows[-1]), flush=True)
            return med

        c1 = record("c_composition", lambda: composition(avg, prev, prev_max, w_dev))
        b1 = record("b_track_step", lambda: ops.track_step(avg, state, w))
        c2 = record("c_again_composition", lambda: composition(avg, prev, prev_max, w_dev))
        b2 = record("b_again_track_step", lambda: ops.track_step(avg, state, w))
        b_, b_spread, c_, c_spread = min(b1, b2), abs(b1 - b2), min(c1, c2), abs(c1 - c2)
        nbytes = ops.track_step_bytes(n, S)
        floor = nbytes / PEAK_BYTES * 1e6
        ops._TTA_WS.clear()   # (b)'s workspace is allocated anew inside the measurement
        mem_b = peak_extra_bytes(lambda: ops.track_step(avg, state, w))
        mem_c = peak_extra_bytes(lambda: composition(avg, prev, prev_max, w_dev))
        got, want = ops.track_step(avg, state, w), composition(avg, prev, prev_max, w_dev)
        agree = {k: bool(same_bits(x, y)) for k, x, y in zip(("score", "score_max", "best", "back"), got, want)}
        summary.append(dict(shape=[n, S, r], b_us=round(b_, 1), b_spread_us=round(b_spread, 1), c_us=round(c_, 1),
                            c_spread_us=round(c_spread, 1), c_over_b=round(c_ / b_, 2),
                            b_faster_than_c_by_more_than_the_spread=bool(b_ + b_spread + c_spread < c_),
                            model_bytes=nbytes, byte_floor_us=round(floor, 2), b_share_of_floor=round(floor / b_, 3),
                            b_peak_extra_bytes=mem_b, c_peak_extra_bytes=mem_c, bit_equal=agree))
        print(json.dumps(summary[-1]), flush=True)
        del avg, prev
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, peak_bytes_per_s=PEAK_BYTES,
               note="median of iters, launches between two HIP events, host time between launches included; b = "
                    "ops.track_step of a later frame (two launches; its cached workspace allocated in the warm-up), c = "
                    "the composition in torch (division, pad with the sentinel and unfold along x, times the weights, "
                    "max; the same along y; gather, multiply, code, the plane's max); each timed twice, alternating, "
                    "the lower median quoted and the difference of the two = its spread; byte floor = "
                    "ops.track_step_bytes at the HBM peak; *_peak_extra_bytes = torch.cuda.max_memory_allocated above "
                    "the inputs during one call; bit_equal: b and c on the timed inputs, output by output",
               summary=summary, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not all(all(s["bit_equal"].values()) for s in summary):
        sys.exit(1)


if __name__ == "__main__":
    main()
