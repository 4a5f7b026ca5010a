"""Dev probe: coarse-to-fine dense matching, ops.match_refine (skp_match_refine), against brute force
and against the same refine composed in torch.

Inputs: 500 tokens; x is a smooth non-negative field (random values on an S / 8 grid, bicubically
enlarged), y the same field displaced by (3, −5) pixels plus 1 % noise, so the coarse field, taken from
the pooled signatures by ops.match_field, is coherent.  Sizes S = 256 (coarse 64) and S = 512 (coarse
128), f = 4, w = 5, one image.  Each time is the median of ``--iters`` after ``--warmup``, the launches
between two HIP events, in one process (as tools/match_field_time.py takes them).

  (a) ops.match_refine alone, on the coarse field of (b).
  (b) the whole path: avg_pool2d of both operands, ops.match_field at S / 4, ops.match_refine.
  (c) S = 256 only: brute force, ops.match_field at S.  (b) must reproduce its result wherever the
      brute-force match lies inside the pixel's window: counted, and the run fails if it does not.
  (d) the refine composed in torch: the (2w + 1)² window indices of a chunk of pixels, a gather of y's
      columns, ``einsum`` over the tokens, the multiply by ry, the masks, ``max``.  It is chunked over
      the pixels so that a gathered copy stays below ``--chunk-bytes``.  Timed before and after (a): the
      difference of its two medians is the spread the comparison is read with.

Beside the times: the flop model 2·n·S²·(2w + 1)² and the byte model of ops, the rates (a) reaches
against them, the peak of ``torch.cuda.max_memory_allocated`` above the inputs for (a) and (d), and how
many indices differ between (a) and (d) (torch sums in its own order).

``--launch-only`` launches (a) three times per size and exits: the program of a counter run, e.g.
    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INST_CYCLES_VMEM -d DIR -o mr \\
        --output-format csv -- python tools/match_refine_time.py --launch-only
Usage: python tools/match_refine_time.py [--out profiles/match_refine_time.json]
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
N_TOK, FACTOR, RADIUS = 500, 4, 5
SIZES = (256, 512)
PEAK_FLOPS = 157.3e12   # f32 VALU = f32 MFMA, MI355X
PEAK_BYTES = 8.0e12     # HBM3E


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


def inputs(S):
    g = torch.Generator().manual_seed(S)
    low = torch.rand(1, N_TOK, S // 8 + 2, S // 8 + 2, generator=g).to(DEV)
    big = F.interpolate(low, size=(S + 16, S + 16), mode="bicubic", align_corners=False).clamp_min_(0).pow_(4)
    x = big[:, :, 8:8 + S, 8:8 + S].contiguous()
    y = big[:, :, 5:5 + S, 13:13 + S].contiguous()          # y[r + 3, c − 5] == x[r, c]
    y.mul_(1 + 0.01 * torch.randn(y.shape, generator=g).to(DEV))
    return x, y


def whole_path(x, y):
    S = x.shape[-1]
    Sc = S // FACTOR
    xl, yl = F.avg_pool2d(x, FACTOR), F.avg_pool2d(y, FACTOR)
    coarse, _ = ops.match_field(xl.reshape(1, N_TOK, Sc * Sc), yl.reshape(1, N_TOK, Sc * Sc))
    return ops.match_refine(x, y, coarse.reshape(1, Sc, Sc), RADIUS) + (coarse.reshape(1, Sc, Sc),)


def composition(x, y, coarse, w, chunk_bytes):
    """(index, score) of match_refine from torch, one image."""
    inf = float("inf")
    n, S = x.shape[1], x.shape[-1]
    f, Sc, P = S // coarse.shape[-1], coarse.shape[-1], S * S
    xs, ys = x.reshape(n, P), y.reshape(n, P)
    nx, ny = (xs * xs).sum(dim=0), (ys * ys).sum(dim=0)
    okx, oky = (nx > 0) & (nx < inf), (ny > 0) & (ny < inf)
    ry = 1.0 / ny.sqrt()
    p = torch.arange(P, device=x.device)
    r, c = p // S, p % S
    m = coarse.reshape(-1).long()[(r // f) * Sc + c // f]
    prior = (m >= 0) & (m < Sc * Sc)
    m = m.clamp(0, Sc * Sc - 1)
    cr, cc = (m // Sc) * f + r % f, (m % Sc) * f + c % f
    d = torch.arange(-w, w + 1, device=x.device)
    dr, dc = d.repeat_interleave(2 * w + 1), d.repeat(2 * w + 1)           # ascending q
    index = torch.empty(P, device=x.device, dtype=torch.int32)
    score = torch.empty(P, device=x.device)
    step = max(1, chunk_bytes // (4 * n * (2 * w + 1) ** 2))
    for p0 in range(0, P, step):
        s = slice(p0, min(P, p0 + step))
        qr, qc = cr[s, None] + dr[None], cc[s, None] + dc[None]
        inside = (qr >= 0) & (qr < S) & (qc >= 0) & (qc < S)
        q = qr.clamp(0, S - 1) * S + qc.clamp(0, S - 1)                    # (Pc, K)
        yw = ys[:, q]                                                      # the gathered copy: (n, Pc, K)
        key = torch.einsum("np,npk->pk", xs[:, s], yw)
        del yw
        key.mul_(ry[q])
        take = inside & oky[q] & prior[s, None]
        key.masked_fill_(~take, -inf)
        value, k = key.max(dim=1)
        ok = okx[s] & take.any(dim=1)
        index[s] = torch.where(ok, q.gather(1, k[:, None])[:, 0], torch.full_like(k, -1)).int()
        score[s] = torch.where(ok, value / nx[s].sqrt(), torch.full_like(value, -inf))
    return index.reshape(1, S, S), score.reshape(1, S, S)


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
    ap.add_argument("--chunk-bytes", type=int, default=4 << 30)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--launch-only", action="store_true", help="launch (a) three times per size and exit")
    a = ap.parse_args()
    rows, summary = [], []
    for S in a.sizes:
        n, f, w, Sc = N_TOK, FACTOR, RADIUS, S // FACTOR
        x, y = inputs(S)
        index, score, coarse = whole_path(x, y)
        if a.launch_only:
            for _ in range(3):
                ops.match_refine(x, y, coarse, w)
            torch.cuda.synchronize()
            continue
        tag = f"n{n}_S{S}_f{f}_w{w}"

        def record(name, fn, iters=a.iters):
            med, lo, hi = median_us(fn, a.warmup, iters)
            rows.append(dict(name=f"{name}_{tag}", median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1)))
            print(json.dumps(rows[-1]), flush=True)
            return med

        few = max(3, a.iters // 4)   # (c) and (d) take tens of milliseconds and more per call
        d1 = record("d_composition", lambda: composition(x, y, coarse, w, a.chunk_bytes), few)
        a_ = record("a_match_refine", lambda: ops.match_refine(x, y, coarse, w))
        b_ = record("b_whole_path", lambda: whole_path(x, y))
        d2 = record("d_again_composition", lambda: composition(x, y, coarse, w, a.chunk_bytes), few)
        d_, spread = min(d1, d2), abs(d1 - d2)
        flops, model_bytes = ops.match_refine_flops(1, n, S, f, w), ops.match_refine_bytes(1, n, S, f, w)
        floor = max(flops / PEAK_FLOPS, model_bytes / PEAK_BYTES) * 1e6
        ops._TTA_WS.clear()   # (a)'s workspace is allocated anew inside the measurement
        mem_a = peak_extra_bytes(lambda: ops.match_refine(x, y, coarse, w))
        mem_d = peak_extra_bytes(lambda: composition(x, y, coarse, w, a.chunk_bytes))
        di, ds = composition(x, y, coarse, w, a.chunk_bytes)
        # the displacement that the inputs were made with, where it stays in the plane
        r, c = torch.arange(S, device=DEV)[:, None], torch.arange(S, device=DEV)[None, :]
        known = ((r + 3 < S) & (c - 5 >= 0))[None]
        truth = ((r + 3) * S + (c - 5))[None]
        row = dict(S=S, coarse=Sc, f=f, w=w, n=n, a_us=round(a_, 1), b_us=round(b_, 1), d_us=round(d_, 1),
                   d_spread_us=round(spread, 1), d_over_a=round(d_ / a_, 1), a_faster_than_d=bool(a_ < d_ - spread),
                   flops=flops, model_bytes=model_bytes, floor_us=round(floor, 1),
                   floor_bound="flops" if flops / PEAK_FLOPS >= model_bytes / PEAK_BYTES else "bytes",
                   a_share_of_floor=round(floor / a_, 3), a_TFps=round(flops / a_ / 1e6, 1),
                   a_model_GBps=round(model_bytes / a_ / 1e3, 1),
                   a_peak_extra_bytes=mem_a, d_peak_extra_bytes=mem_d, d_chunk_bytes=a.chunk_bytes,
                   a_vs_d_indices_differ=int((index != di).sum()), pixels=S * S,
                   a_vs_d_score_max_abs_diff=float((score - ds).abs().max()),
                   pixels_with_known_match=int(known.sum()), known_match_recovered=int(((index == truth) & known).sum()))
        if S == 256:
            P = S * S
            c_ = record("c_brute_force", lambda: ops.match_field(x.reshape(1, n, P), y.reshape(1, n, P)), few)
            bi, bs = ops.match_field(x.reshape(1, n, P), y.reshape(1, n, P))
            bi, bs = bi.reshape(1, S, S), bs.reshape(1, S, S)
            centre = coarse.long().repeat_interleave(f, 1).repeat_interleave(f, 2)
            cr, cc = centre // Sc * f + r % f, centre % Sc * f + c % f
            inside = (bi >= 0) & ((bi // S - cr).abs() <= w) & ((bi % S - cc).abs() <= w)
            same = (index == bi) & (score.view(torch.int32) == bs.view(torch.int32))
            row.update(c_us=round(c_, 1), c_over_b=round(c_ / b_, 1), b_faster_than_c=bool(b_ < c_),
                       c_flops=ops.match_field_flops(1, n, P, P), c_TFps=round(ops.match_field_flops(1, n, P, P) / c_ / 1e6, 1),
                       brute_force_inside_window=int(inside.sum()), b_equals_c_inside_window=int((same & inside).sum()),
                       b_equals_c_everywhere=int(same.sum()))
            assert bool((same | ~inside).all()), "the refined field differs from brute force inside a window"
        summary.append(row)
        print(json.dumps(row), flush=True)
        del x, y
    if a.launch_only:
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, peak_flops=PEAK_FLOPS,
               peak_bytes=PEAK_BYTES,
               note="median of iters, launches between two HIP events, one image, 500 tokens, f = 4, w = 5; "
                    "a = ops.match_refine alone, b = avg_pool2d of both operands + ops.match_field at S / 4 + "
                    "ops.match_refine, c = ops.match_field at S (brute force; iters / 4 repeats), d = the refine "
                    "composed in torch (window gather, einsum, scale, masks, max; chunked over the pixels below "
                    "d_chunk_bytes per gathered copy; host time between its launches included; iters / 4 repeats), the "
                    "lower of two medians taken before and after a, their difference = d_spread; flops = "
                    "2·n·S²·(2w + 1)², the dots of the definition; model_bytes = both operands once + coarse + "
                    "index + score; floor = the larger of flops at the f32 peak and model_bytes at the HBM peak; "
                    "*_peak_extra_bytes = torch.cuda.max_memory_allocated above the inputs during one call; "
                    "b_equals_c_inside_window counts pixels whose brute-force match lies in the window and whose index "
                    "and score bits b reproduces; known_match_recovered: pixels where b returns the displacement the "
                    "inputs were made with.  Synthetic inputs: the quality of refined fields on real data has not been "
                    "measured.",
               summary=summary, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
