"""Dev probe: ops.match_field (skp_match_field) against its composition from torch.

Shapes (B, n, S) = (1, 500, 128), (4, 500, 128) and (1, 500, 64): B images' signatures (B, n, S²) against
one shared source (1, n, S²), P = Q = S².  Each time is the median of ``--iters`` after ``--warmup``, the
launches between two HIP events, in one process (as tools/tta_time.py takes them).

  (b) ops.match_field: the MFMA field kernel (norms included) and the merge; the (P, Q) product stays in
      registers.
  (c) the composition from what exists without it: the norms over the tokens, ``torch.matmul`` of the
      transposed signatures with the shared source (one (B·P, n)·(n, Q) GEMM), the multiply by ry and the
      usable mask in place, ``max(dim=2)`` and the score.  It writes and reads the (B, P, Q) product.
      Timed before and after (b): the difference of its two medians is the spread the comparison is
      read with.

Beside the times: the flop floor 2·B·n·P·Q / 157.3 TF/s and (b)'s share of it, the peak of
``torch.cuda.max_memory_allocated`` above the inputs for (b) and for (c), and how many indices differ
between the two (torch sums in its own order, (b) in token order).

``--launch-only`` launches (b) three times per shape and exits: the program of a counter run, e.g.
    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES -d DIR -o mf --output-format csv -- \\
        python tools/match_field_time.py --launch-only
Usage: python tools/match_field_time.py [--out profiles/match_field_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stablekeypoints_amd import ops

DEV = "cuda:0"
SHAPES = ((1, 500, 128), (4, 500, 128), (1, 500, 64))
PEAK_FLOPS = 157.3e12   # f32 MFMA, MI355X


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


def composition(x, y):
    """(index, score) of match_field from torch: x (B, n, P), y (1, n, Q) shared."""
    inf = float("inf")
    nx, ny = (x * x).sum(dim=1), (y * y).sum(dim=1)
    okx, oky = (nx > 0) & (nx < inf), (ny > 0) & (ny < inf)
    key = torch.matmul(x.transpose(1, 2), y[0])                  # (B, P, Q)
    key.mul_((1.0 / ny.sqrt())[:, None, :])
    key.masked_fill_(~oky[:, None, :], -inf)
    value, idx = key.max(dim=2)
    ok = okx & oky.any()
    return (torch.where(ok, idx, torch.full_like(idx, -1)).int(),
            torch.where(ok, value * (1.0 / nx.sqrt()), torch.full_like(value, -inf)))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--launch-only", action="store_true", help="launch (b) three times per shape and exit")
    a = ap.parse_args()
    rows, summary = [], []
    for B, n, S in SHAPES:
        P = Q = S * S
        g = torch.Generator().manual_seed(S + B)
        # softmax-like signatures: non-negative, a few tokens strong at every pixel
        x = torch.rand(B, n, P, generator=g).pow_(8).to(DEV)
        y = torch.rand(1, n, Q, generator=g).pow_(8).to(DEV)
        if a.launch_only:
            for _ in range(3):
                ops.match_field(x, y)
            torch.cuda.synchronize()
            continue
        tag = f"B{B}_n{n}_S{S}"

        def record(name, f):
            med, lo, hi = median_us(f, a.warmup, a.iters)
            rows.append(dict(name=f"{name}_{tag}", median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1)))
            print(json.dumps(rows[-1]), flush=True)
            return med

        c1 = record("c_composition", lambda: composition(x, y))
        b_ = record("b_match_field", lambda: ops.match_field(x, y))
        c2 = record("c_again_composition", lambda: composition(x, y))
        c_, spread = min(c1, c2), abs(c1 - c2)
        flops = ops.match_field_flops(B, n, P, Q)
        floor = flops / PEAK_FLOPS * 1e6
        ops._TTA_WS.clear()   # (b)'s workspace is allocated anew inside the measurement
        mem_b = peak_extra_bytes(lambda: ops.match_field(x, y))
        mem_c = peak_extra_bytes(lambda: composition(x, y))
        (bi, bs), (ci, cs) = ops.match_field(x, y), composition(x, y)
        summary.append(dict(shape=[B, n, S], P=P, Q=Q, b_us=round(b_, 1), c_us=round(c_, 1), c_spread_us=round(spread, 1),
                            b_over_c=round(b_ / c_, 3), b_no_slower_than_c=bool(b_ <= c_ + spread),
                            flops=flops, flop_floor_us=round(floor, 1), b_share_of_peak=round(floor / b_, 3),
                            b_TFps=round(flops / b_ / 1e6, 1), c_TFps=round(flops / c_ / 1e6, 1),
                            b_model_bytes=ops.match_field_bytes(B, n, P, Q, B, 1),
                            b_peak_extra_bytes=mem_b, c_peak_extra_bytes=mem_c,
                            indices_differ=int((bi != ci).sum()), pixels=B * P,
                            score_max_abs_diff=float((bs - cs).abs().max())))
        print(json.dumps(summary[-1]), flush=True)
        del x, y
    if a.launch_only:
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, peak_flops=PEAK_FLOPS,
               note="median of iters, launches between two HIP events; b = ops.match_field (its cached workspace "
                    "allocated in the warm-up), c = the composition in torch (norms, one matmul against the shared "
                    "source, multiply by ry and usable mask in place, max(dim=2); host time between its launches "
                    "included), the lower of two medians taken before and after b, their difference = c_spread; "
                    "b_no_slower_than_c: b <= c + c_spread; flop floor = 2·B·n·P·Q at the f32 MFMA peak; "
                    "*_peak_extra_bytes = torch.cuda.max_memory_allocated above the inputs during one call (b's "
                    "with its workspace allocated anew); "
                    "indices_differ: pixels whose index differs between b (token-order fmaf chain) and c (torch's order)",
               summary=summary, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
