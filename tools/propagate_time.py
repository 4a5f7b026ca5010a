"""Dev probe: one frame of label propagation, ops.match_topk (skp_match_topk) + ops.label_vote
(skp_label_vote), against the same step composed in torch and against ops.match_refine with f = 1.

Inputs: x is a smooth non-negative field (random values on an S / 8 grid, bicubically enlarged, to the
fourth power), the M = 3 context frames are the same field displaced by (j, −j) pixels, j = 1 … 3, plus
1 % noise; the context labels are two soft planes (a disk and its complement, displaced likewise).
K = 5, tau = 0.07.  Sizes (n, S, w): (500, 128, 8), (10, 128, 8), (500, 256, 12).  Each time is the
median of ``--iters`` after ``--warmup``, the launches between two HIP events, in one process (as
tools/match_refine_time.py takes them).

  (k) ops.match_topk + ops.label_vote: the frame's step.  Also each of the two alone.
  (a) the same step composed in torch: per context the (2w + 1)² window indices of a chunk of pixels, a
      gather of y's columns, ``einsum`` over the tokens, the multiply by ry, the masks, ``topk``; then
      ``topk`` over the M·K candidates, softmax, a gather of the labels and the weighted sum.  Chunked
      over the pixels so that a gathered copy stays below ``--chunk-bytes``.  Timed before and after
      (k): the difference of its two medians is the spread the comparison is read with.
  (b) ops.match_refine with f = 1 and the identity prior over the same contexts: one (key, q) per
      pixel.  (k's match_topk) − (b) is the price of K lists over one.

Beside the times: the flop model 2·M·n·S²·(2w + 1)² and the rates against it, the peak of
``torch.cuda.max_memory_allocated`` above the inputs for (k), (a) and (b), how many list entries and
labels differ between (k) and (a) (torch sums in its own order), and whether slot 0 of (k) equals (b)
bit for bit.

``--launch-only`` launches (k) three times per size and exits: the program of a counter run, e.g.
    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INST_CYCLES_VMEM -d DIR -o pt \\
        --output-format csv -- python tools/propagate_time.py --launch-only
Usage: python tools/propagate_time.py [--out profiles/propagate_time.json]
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
M_CTX, K_LIST, TAU = 3, 5, 0.07
SIZES = ((500, 128, 8), (10, 128, 8), (500, 256, 12))     # (n, S, w)
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


def inputs(n, S):
    """x (1, n, S, S), y (M, n, S, S), labels (M, 2, S, S)."""
    g = torch.Generator().manual_seed(S + n)
    pad = 8
    low = torch.rand(1, n, S // 8 + 2, S // 8 + 2, generator=g).to(DEV)
    big = F.interpolate(low, size=(S + 2 * pad, S + 2 * pad), mode="bicubic", align_corners=False).clamp_min_(0).pow_(4)
    x = big[:, :, pad:pad + S, pad:pad + S].contiguous()
    y = torch.cat([big[:, :, pad - j:pad - j + S, pad + j:pad + j + S] for j in range(1, M_CTX + 1)]).contiguous()
    y.mul_(1 + 0.01 * torch.randn(y.shape, generator=g).to(DEV))   # y_j[r + j, c − j] == x[r, c] up to the noise
    r, c = torch.arange(S, device=DEV)[:, None], torch.arange(S, device=DEV)[None, :]
    disks = torch.stack([((r - S // 2 - j) ** 2 + (c - S // 2 + j) ** 2 <= (S // 4) ** 2) for j in range(1, M_CTX + 1)])
    labels = torch.stack([~disks, disks], dim=1).to(torch.float32).contiguous()
    return x, y, labels


def step(x, y, labels, w):
    index, score = ops.match_topk(x, y, w, K_LIST)
    return ops.label_vote(index, score, labels, TAU) + (index, score)


def refine(x, y, prior, w):
    return ops.match_refine(x, y, prior, w)


def composition(x, y, labels, w, chunk_bytes):
    """(soft, label, confidence, index, score) of ``step`` from torch."""
    inf = float("inf")
    n, S = x.shape[1], x.shape[-1]
    M, P, Wn = y.shape[0], S * S, (2 * w + 1) ** 2
    xs = x.reshape(n, P)
    nx = (xs * xs).sum(dim=0)
    okx = (nx > 0) & (nx < inf)
    p = torch.arange(P, device=x.device)
    r, c = p // S, p % S
    d = torch.arange(-w, w + 1, device=x.device)
    dr, dc = d.repeat_interleave(2 * w + 1), d.repeat(2 * w + 1)           # ascending q
    index = torch.full((M, K_LIST, P), -1, device=x.device, dtype=torch.int32)
    score = torch.full((M, K_LIST, P), -inf, device=x.device)
    step_px = max(1, chunk_bytes // (4 * n * Wn))
    kk = min(K_LIST, Wn)
    for j in range(M):
        ys = y[j].reshape(n, P)
        ny = (ys * ys).sum(dim=0)
        oky, ry = (ny > 0) & (ny < inf), 1.0 / ny.sqrt()
        for p0 in range(0, P, step_px):
            s = slice(p0, min(P, p0 + step_px))
            qr, qc = r[s, None] + dr[None], c[s, None] + dc[None]
            inside = (qr >= 0) & (qr < S) & (qc >= 0) & (qc < S)
            q = qr.clamp(0, S - 1) * S + qc.clamp(0, S - 1)                # (Pc, Wn)
            yw = ys[:, q]                                                  # the gathered copy: (n, Pc, Wn)
            key = torch.einsum("np,npk->pk", xs[:, s], yw)
            del yw
            key.mul_(ry[q])
            take = inside & oky[q]
            key.masked_fill_(~take, -inf)
            value, k = key.topk(kk, dim=1)                                 # (Pc, K)
            found = take.gather(1, k) & okx[s, None]
            index[j, :kk, s] = torch.where(found, q.gather(1, k), torch.full_like(k, -1)).int().T
            score[j, :kk, s] = torch.where(found, value / nx[s, None].sqrt(), torch.full_like(value, -inf)).T
    # the vote
    Cl = labels.shape[1]
    cand_s = score.reshape(M * K_LIST, P).T                                # (P, M·K), c = j·K + i
    cand_q = index.reshape(M * K_LIST, P).T.long()
    top_s, top_c = cand_s.topk(K_LIST, dim=1)
    top_q = cand_q.gather(1, top_c)
    live = top_q >= 0
    e = torch.where(live, ((top_s - top_s[:, :1]) * (1.0 / TAU)).exp(), torch.zeros_like(top_s))
    wgt = e / e.sum(dim=1, keepdim=True).clamp_min(1e-30)
    lab = labels.reshape(M, Cl, P)[(top_c // K_LIST)[:, :, None], torch.arange(Cl, device=x.device)[None, None, :],
                                   top_q.clamp_min(0)[:, :, None]]         # (P, K, Cl)
    soft = (wgt[:, :, None] * lab).sum(dim=1)                              # (P, Cl)
    conf, label = soft.max(dim=1)
    label = torch.where(live.any(dim=1), label, torch.full_like(label, -1)).int()
    return (soft.T.reshape(Cl, S, S), label.reshape(S, S), conf.reshape(S, S), index.reshape(M, K_LIST, S, S),
            score.reshape(M, K_LIST, S, S))


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
    ap.add_argument("--chunk-bytes", type=int, default=2 << 30)
    ap.add_argument("--sizes", type=int, nargs="+", default=None, help="indices into SIZES")
    ap.add_argument("--launch-only", action="store_true", help="launch (k) three times per size and exit")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("propagate_time: no HIP device (times are taken on the GPU only)")
    rows, summary = [], []
    for n, S, w in (SIZES if a.sizes is None else [SIZES[i] for i in a.sizes]):
        x, y, labels = inputs(n, S)
        M = y.shape[0]
        if a.launch_only:
            for _ in range(3):
                step(x, y, labels, w)
            torch.cuda.synchronize()
            continue
        tag = f"n{n}_S{S}_w{w}"
        prior = torch.arange(S * S, dtype=torch.int32, device=DEV).reshape(1, S, S).repeat(M, 1, 1).contiguous()
        index, score = ops.match_topk(x, y, w, K_LIST)

        def record(name, fn, iters=a.iters):
            med, lo, hi = median_us(fn, a.warmup, iters)
            rows.append(dict(name=f"{name}_{tag}", median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1)))
            print(json.dumps(rows[-1]), flush=True)
            return med

        few = max(3, a.iters // 4)   # (a) takes tens of milliseconds and more per call
        a1 = record("a_composition", lambda: composition(x, y, labels, w, a.chunk_bytes), few)
        k_ = record("k_step", lambda: step(x, y, labels, w))
        kt = record("k_match_topk", lambda: ops.match_topk(x, y, w, K_LIST))
        kv = record("k_label_vote", lambda: ops.label_vote(index, score, labels, TAU))
        b_ = record("b_match_refine_f1", lambda: refine(x, y, prior, w))
        a2 = record("a_again_composition", lambda: composition(x, y, labels, w, a.chunk_bytes), few)
        a_, spread = min(a1, a2), abs(a1 - a2)
        flops = ops.match_topk_flops(M, n, S, w)
        model_bytes = ops.match_topk_bytes(M, n, S, w, K_LIST, 1, M) + ops.label_vote_bytes(M, K_LIST, S, 2, K_LIST)
        floor = max(flops / PEAK_FLOPS, model_bytes / PEAK_BYTES) * 1e6
        ops._TTA_WS.clear()   # the workspaces are allocated anew inside the measurement
        mem_k = peak_extra_bytes(lambda: step(x, y, labels, w))
        mem_b = peak_extra_bytes(lambda: refine(x, y, prior, w))
        mem_a = peak_extra_bytes(lambda: composition(x, y, labels, w, a.chunk_bytes))
        ks, kl, kc, ki, ksc = step(x, y, labels, w)
        cs, cl, cc, ci, csc = composition(x, y, labels, w, a.chunk_bytes)
        bi, bs = refine(x, y, prior, w)
        # the displacement that the inputs were made with, where it stays in the plane: context j at (r + j, c − j)
        r, c = torch.arange(S, device=DEV)[:, None], torch.arange(S, device=DEV)[None, :]
        known = torch.stack([(r + j < S) & (c - j >= 0) for j in range(1, M + 1)])
        truth = torch.stack([(r + j) * S + (c - j) for j in range(1, M + 1)])
        row = dict(n=n, S=S, w=w, M=M, K=K_LIST, k_us=round(k_, 1), k_match_topk_us=round(kt, 1),
                   k_label_vote_us=round(kv, 1), b_us=round(b_, 1), a_us=round(a_, 1), a_spread_us=round(spread, 1),
                   a_over_k=round(a_ / k_, 1), k_faster_than_a=bool(k_ < a_ - spread),
                   topk_over_b=round(kt / b_, 2), topk_minus_b_us=round(kt - b_, 1),
                   flops=flops, model_bytes=model_bytes, floor_us=round(floor, 1),
                   floor_bound="flops" if flops / PEAK_FLOPS >= model_bytes / PEAK_BYTES else "bytes",
                   k_share_of_floor=round(floor / k_, 3), k_TFps=round(flops / k_ / 1e6, 1),
                   topk_TFps=round(flops / kt / 1e6, 1), b_TFps=round(flops / b_ / 1e6, 1),
                   k_peak_extra_bytes=mem_k, a_peak_extra_bytes=mem_a, b_peak_extra_bytes=mem_b,
                   a_chunk_bytes=a.chunk_bytes, list_entries=int(ki.numel()),
                   k_vs_a_list_entries_differ=int((ki != ci).sum()), pixels=S * S,
                   k_vs_a_labels_differ=int((kl != cl).sum()),
                   k_vs_a_soft_max_abs_diff=float((ks - cs).abs().max()),
                   slot0_equals_b_bit_for_bit=bool(torch.equal(ki[:, 0], bi)
                                                   and torch.equal(ksc[:, 0].view(torch.int32), bs.view(torch.int32))),
                   pixels_with_known_match=int(known.sum()), known_match_in_slot0=int(((ki[:, 0] == truth) & known).sum()))
        summary.append(row)
        print(json.dumps(row), flush=True)
        del x, y, labels
    if a.launch_only:
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters, peak_flops=PEAK_FLOPS,
               peak_bytes=PEAK_BYTES,
               note="median of iters, launches between two HIP events, one frame against M = 3 context frames, K = 5, "
                    "tau = 0.07; k = ops.match_topk + ops.label_vote (k_match_topk, k_label_vote: each alone), b = "
                    "ops.match_refine with f = 1 and the identity prior over the same contexts, a = the step composed in "
                    "torch (window gather, einsum, scale, masks, topk; topk over the M·K candidates, softmax, label "
                    "gather; chunked over the pixels below a_chunk_bytes per gathered copy; host time between its launches "
                    "included; iters / 4 repeats), the lower of two medians taken before and after k, their difference = "
                    "a_spread; flops = 2·M·n·S²·(2w + 1)², the dots of the definition; model_bytes = x once, the M "
                    "contexts once, the lists written and read, the labels gathered and the results; floor = the larger of "
                    "flops at the f32 peak and model_bytes at the HBM peak; *_peak_extra_bytes = "
                    "torch.cuda.max_memory_allocated above the inputs during one call; known_match_in_slot0: list heads "
                    "that are the displacement the inputs were made with.  Synthetic inputs: the quality of propagated "
                    "labels on real video has not been measured.",
               summary=summary, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
