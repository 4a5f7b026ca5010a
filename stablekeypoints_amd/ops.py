"""Torch-facing ops over libskp (HIP, gfx950): autograd Functions and plain wrappers.

Every function here launches the HIP kernels through the C ABI (``_lib``) on the
current HIP stream; there is no CPU or eager-torch fallback for the hot path.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import call, ptr, stream

F32 = torch.float32

# Optional per-kernel timer (bench.py): an object with record(name, nbytes) returning a
# context manager that brackets one launch with HIP events on the current stream.
_TIMER = None


def set_kernel_timer(timer):
    global _TIMER
    _TIMER = timer


class _NoTimer:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _timed(name, nbytes=0, flops=0, cycles=0):
    return _TIMER.record(name, nbytes, flops, cycles) if _TIMER is not None else _NoTimer()


def _c(t, dtype=F32):
    return t.contiguous() if t.dtype == dtype else t.to(dtype).contiguous()


def _c16(t):
    """Contiguous fp32 with a 16-B aligned base (the float4 paths of libskp require it): a view
    at an odd storage offset is copied."""
    t = _c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _rows16(t):
    """fp32 with unit-stride, 16-B aligned rows (row stride a multiple of 4 floats, e.g. a column
    block of a fused projection's output) as it is; anything else through _c16."""
    if (t.dtype == F32 and t.stride(-1) == 1 and t.stride(-2) % 4 == 0 and t.data_ptr() % 16 == 0
            and (t.dim() < 3 or t.shape[0] == 1 or t.stride(0) % 4 == 0)):
        return t
    return _c16(t)


# --------------------------------------------------------------------------- Q·Kᵀ on MFMA
def bgemm(a, b, alpha=1.0, out=None, accumulate=False):
    """out[z] = alpha · a[z] @ b[z] for 3-D fp32 tensors of any strides (skp_bgemm_f32)."""
    _lib.require_device(a, b)
    Z, M, K = a.shape
    Z2, K2, N = b.shape
    assert Z == Z2 and K == K2, (a.shape, b.shape)
    if out is None:
        out = torch.empty(Z, M, N, device=a.device, dtype=F32)
    call("skp_bgemm_f32", ptr(a), a.stride(0), a.stride(1), a.stride(2), ptr(b), b.stride(0), b.stride(1),
         b.stride(2), ptr(out), out.stride(0), out.stride(1), out.stride(2), Z, M, N, K, float(alpha),
         int(accumulate), stream(a.device))
    return out


def bgemm_2b(a, sa, b, sb, out, so, batch, hb, M, N, K, alpha=1.0, accumulate=False):
    """skp_bgemm_f32_2b: for z = o·hb + i, out_z = alpha · a_z @ b_z with operand X_z at
    X + o·sX[0] + i·sX[1], row / column strides sX[2], sX[3] (elements; a: (M, K), b: (K, N),
    out: (M, N))."""
    call("skp_bgemm_f32_2b", ptr(a), *sa, ptr(b), *sb, ptr(out), *so, int(batch), int(hb), int(M), int(N), int(K),
         float(alpha), int(accumulate), stream(a.device))
    return out


class CaptureLogitsHeads(torch.autograd.Function):
    """z = q kᵀ · scale for the B·H heads of a captured layer read in place: q the layer's (B, S, H·d)
    to_q projection, k the ONE (1, N, H·d) to_k projection of the token embedding the batch shares
    (ptp_utils.py:493 / 534) — no head-permute copy of q and no batch-expanded copy of k.  Output
    (B·H, S, N), the head-major layout the capture consumes.  Backward: dq straight into the (B, S,
    H·d) layout; dk per image into a (B, N, H·d) scratch summed over the images (the expand's
    reduction)."""

    @staticmethod
    def forward(ctx, qf, k1, H, scale):
        qf, k1 = _c16(qf), _rows16(k1)
        B, S, C = qf.shape
        N, d, rk = k1.shape[1], C // H, k1.stride(1)
        z = torch.empty(B * H, S, N, device=qf.device, dtype=F32)
        bgemm_2b(qf, (S * C, d, C, 1), k1, (0, d, 1, rk), z, (H * S * N, S * N, N, 1), B * H, H, S, N, d, scale)
        ctx.save_for_backward(qf, k1)
        ctx.meta = (H, float(scale))
        return z

    @staticmethod
    def backward(ctx, dz):
        qf, k1 = ctx.saved_tensors
        H, scale = ctx.meta
        B, S, C = qf.shape
        N, d, rk = k1.shape[1], C // H, k1.stride(1)
        dz = _c16(dz)
        dq = dk1 = None
        if ctx.needs_input_grad[0]:
            dq = torch.empty_like(qf)
            bgemm_2b(dz, (H * S * N, S * N, N, 1), k1, (0, d, rk, 1), dq, (S * C, d, C, 1), B * H, H, S, d, N, scale)
        if ctx.needs_input_grad[1]:
            dkb = torch.empty(B, N, C, device=qf.device, dtype=F32)
            bgemm_2b(dz, (H * S * N, S * N, 1, N), qf, (S * C, d, C, 1), dkb, (N * C, d, C, 1), B * H, H, N, d, S,
                     scale)
            dk1 = dkb.sum(dim=0, keepdim=True) if B > 1 else dkb
        return dq, dk1, None, None


class AttnPVHeads(torch.autograd.Function):
    """out = P v per head into the (B, S, H·d) layout to_out reads: P (B·H, S, N) the captured layer's
    softmax, v the ONE (1, N, H·d) to_v projection of the shared token embedding (ptp_utils.py:
    500-502 / 540-541, the normal-path output of a captured layer) — no batch-expanded copy of v and
    no heads-to-batch permute of the output.  Backward: dP = dout vᵀ; dv per image summed over the
    images."""

    @staticmethod
    def forward(ctx, P, v1, H):
        P, v1 = _c16(P), _rows16(v1)
        BH, S, N = P.shape
        B, C = BH // H, v1.shape[2]
        d, rv = C // H, v1.stride(1)
        out = torch.empty(B, S, C, device=P.device, dtype=F32)
        bgemm_2b(P, (H * S * N, S * N, N, 1), v1, (0, d, rv, 1), out, (S * C, d, C, 1), BH, H, S, d, N)
        ctx.save_for_backward(P, v1)
        ctx.H = H
        return out

    @staticmethod
    def backward(ctx, dout):
        P, v1 = ctx.saved_tensors
        H = ctx.H
        BH, S, N = P.shape
        B, C = BH // H, v1.shape[2]
        d, rv = C // H, v1.stride(1)
        dout = _c16(dout)
        dP = dv1 = None
        if ctx.needs_input_grad[0]:
            dP = torch.empty_like(P)
            bgemm_2b(dout, (S * C, d, C, 1), v1, (0, d, 1, rv), dP, (H * S * N, S * N, N, 1), BH, H, S, N, d)
        if ctx.needs_input_grad[1]:
            dvb = torch.empty(B, N, C, device=P.device, dtype=F32)
            bgemm_2b(P, (H * S * N, S * N, 1, N), dout, (S * C, d, C, 1), dvb, (N * C, d, C, 1), BH, H, N, d, S)
            dv1 = dvb.sum(dim=0, keepdim=True) if B > 1 else dvb
        return dP, dv1, None


def capture_logits_heads(qf, k1, heads, scale):
    """(B·H, S, N) logits of a captured layer from its (B, S, H·d) query projection and the shared
    (1, N, H·d) key projection (CaptureLogitsHeads)."""
    _lib.require_device(qf, k1)
    return CaptureLogitsHeads.apply(qf, k1, int(heads), float(scale))


def attn_pv_heads(P, v1, heads):
    """(B, S, H·d) = per-head P v with the shared (1, N, H·d) value projection (AttnPVHeads)."""
    _lib.require_device(P, v1)
    return AttnPVHeads.apply(P, v1, int(heads))


def heads_eligible(qf, k1, heads):
    """The in-place head GEMMs take fp32 (B, S, H·d) / (1, N, H·d) projections with d, S·H·d and N
    multiples of 4 (16-B aligned heads for the vector loads)."""
    C = qf.shape[-1]
    return (qf.dtype == F32 and k1.dtype == F32 and qf.dim() == 3 and k1.dim() == 3 and k1.shape[0] == 1
            and C % heads == 0 and (C // heads) % 4 == 0 and k1.shape[1] % 4 == 0 and k1.shape[2] == C)


class CaptureLogits(torch.autograd.Function):
    """z = q kᵀ · scale — the layer's cross-attention logits (ptp_utils.py:493 / 534)."""

    @staticmethod
    def forward(ctx, q, k, scale):
        q, k = _c(q), _c(k)
        ctx.save_for_backward(q, k)
        ctx.scale = scale
        return bgemm(q, k.transpose(1, 2), scale)

    @staticmethod
    def backward(ctx, dz):
        q, k = ctx.saved_tensors
        dz = _c(dz)
        dq = dk = None
        if ctx.needs_input_grad[0]:
            dq = bgemm(dz, k, ctx.scale)
        if ctx.needs_input_grad[1]:
            dk = bgemm(dz.transpose(1, 2), q, ctx.scale)
        return dq, dk, None


def capture_logits(q, k, scale):
    return CaptureLogits.apply(q, k, float(scale))


# --------------------------------------------------------------------------- A1 capture
def _layer_ptrs(tensors, offset=0):
    """The C ABI's array of per-layer device pointers (void* const*), each ``offset`` bytes in."""
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() + offset for t in tensors])
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))


def _layer_sizes(sizes):
    """The C ABI's array of per-layer sizes (const int*)."""
    return (ctypes.c_int * len(sizes))(*[int(s) for s in sizes])


def _capture_fwd_run(z, s, R, with_stats=False):
    """skp_capture_fwd: (attn (BH, R², N), the per-pixel softmax (max, 1/Σ) (BH, R², 2) or None)."""
    BH, S, N = z.shape
    assert S == s * s
    attn = torch.empty(BH, R * R, N, device=z.device, dtype=F32)
    stats = torch.empty(BH, R * R, 2, device=z.device, dtype=F32) if with_stats else None
    with _timed("skp_capture_fwd", (BH * R * R * N + BH * S * N) * 4):
        call("skp_capture_fwd", ptr(z), BH, s, N, R, ptr(attn), ptr(stats), stream(z.device))
    return attn, stats


class CaptureAttn(torch.autograd.Function):
    """attn = softmax_N(bicubic_{s→R}(z_low)) — the captured map (ptp_utils.py:513-536)."""

    @staticmethod
    def forward(ctx, z, s, R):
        z = _c(z)
        attn, _ = _capture_fwd_run(z, s, R)
        ctx.save_for_backward(z)
        ctx.s, ctx.R = s, R
        return attn

    @staticmethod
    def backward(ctx, dattn):
        (z,) = ctx.saved_tensors
        return capture_bwd(z, ctx.s, ctx.R, dattn), None, None


def capture_bwd(z, s, R, dattn, gscale=1.0, group=1, strides=None, stats=None):
    """dz_low for g = gscale·dattn; ``dattn`` (BH, R², N) of any strides, or with ``group``/
    ``strides`` = (sb, sp, sn) a per-group gradient (row b uses group b // group).  ``stats``:
    the forward's per-pixel softmax (max, 1/Σ), (BH, R², 2), or None (recomputed)."""
    BH, S, N = z.shape
    if dattn.dtype != F32:
        dattn = dattn.float()
    if strides is None:
        sb, sp, sn = dattn.stride()
        if dattn.shape[0] == 1 and BH > 1:
            sb = 0
    else:
        sb, sp, sn = strides
    ws = torch.empty(capture_bwd_ws_floats(BH, s, N, R), device=z.device, dtype=F32)
    dz = torch.empty_like(z)
    with _timed("skp_capture_bwd", (BH * S * N * 2 + BH * R * s * N * 2) * 4):
        call("skp_capture_bwd", ptr(z), BH, s, N, R, ptr(dattn), int(group), sb, sp, sn, float(gscale),
             ptr(stats), ptr(dz), ptr(ws), stream(z.device))
    return dz


def capture_attn(z, s, R):
    return CaptureAttn.apply(z, int(s), int(R))


# --------------------------------------------------------------------------- A3 aggregate
class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, indices, upsample_res, *layers):
        layers = [_c(t) for t in layers]
        BH, RR, N = layers[0].shape
        R = int(round(RR ** 0.5))
        for t in layers:
            if t.shape != layers[0].shape:
                raise ValueError("collect_maps: captured layers must share (BH, R*R, N); got "
                                 f"{[tuple(x.shape) for x in layers]}")
        n_out = N if indices is None else int(indices.numel())
        out = torch.empty(n_out, R, R, device=layers[0].device, dtype=F32)
        idx = None if indices is None else indices.to(device=out.device, dtype=torch.int64).contiguous()
        with _timed("skp_aggregate", (len(layers) * BH * RR * N + n_out * RR) * 4):
            call("skp_aggregate", _layer_ptrs(layers), len(layers), BH, RR, N, ptr(idx), n_out, ptr(out),
                 stream(out.device))
        ctx.meta = (BH, RR, N, R, len(layers))
        ctx.idx = idx
        ctx.upsample_res = upsample_res
        if upsample_res != -1 and upsample_res != R:
            up = torch.empty(n_out, upsample_res, upsample_res, device=out.device, dtype=F32)
            call("skp_resize_bilinear", ptr(out), n_out, R, upsample_res, ptr(up), stream(out.device))
            out = up
        return out

    @staticmethod
    def backward(ctx, dmap):
        BH, RR, N, R, L = ctx.meta
        dmap = _c(dmap)
        if ctx.upsample_res != -1 and ctx.upsample_res != R:
            g = torch.empty(dmap.shape[0], R, R, device=dmap.device, dtype=F32)
            call("skp_resize_bilinear_bwd", ptr(dmap), dmap.shape[0], R, ctx.upsample_res, ptr(g), stream(dmap.device))
            dmap = g
        dmap = dmap.reshape(-1, RR) / float(L * BH)
        if ctx.idx is not None:
            full = torch.zeros(N, RR, device=dmap.device, dtype=F32)
            full.index_add_(0, ctx.idx, dmap)
            dmap = full
        # d attn_l[b, p, n] = dmap[n, p] / (L·BH): a stride-0 broadcast view, never materialised
        g = dmap.t().unsqueeze(0).expand(BH, RR, N)
        return (None, None) + tuple(g for _ in range(L))


def aggregate(layers, indices=None, upsample_res=-1):
    return _Aggregate.apply(indices, int(upsample_res), *layers)


FUSED_MAPS = True   # tests switch it: False = skp_capture_fwd + skp_aggregate (the AttentionStore path)


def capture_maps_bytes(B, H, N, R, sizes):
    """Algorithmic HBM bytes of one skp_capture_maps_fwd launch: every z_low read once, the
    (B, N, R²) maps and the (B·H, R², 2) per-layer stats written once."""
    RR = R * R
    return 4 * (sum(B * H * s * s * N for s in sizes) + B * N * RR + len(sizes) * B * H * RR * 2)


def capture_maps_flops(B, H, N, R, sizes):
    """Algorithmic fp32 VALU work of one skp_capture_maps_fwd launch: per
    (image, head, layer, pixel, token) 15 FLOP — horizontal bicubic 4 multiply-adds (8), softmax
    max 1 + (z − m)·log2e as an FMA 2 + exp 1 + Σ 1, normalise-and-accumulate FMA 2 — and per
    (image, head, layer, output row, low-res column, token) 8 for the vertical bicubic pass."""
    return sum(B * H * N * (15 * R * R + 8 * R * s) for s in sizes)


# VALU issue cost on gfx950 (MI355X_MICROARCH.md, "vector-instruction ISSUE cost"): a wave64
# instruction occupies its SIMD 4 cycles (v_fma_f32 / v_pk_fma_f32 / v_max3_f32 …), 8 for the
# transcendentals (v_exp_f32); a packed f32 instruction does 2 elements per lane.  SIMD-cycles per
# element of one f32 op: packed 4/128, transcendental 8/64.
_PK, _TR = 4.0 / 128, 8.0 / 64


def capture_maps_issue_cycles(B, H, N, R, sizes):
    """Minimal VALU issue cycles (summed over SIMDs) of one skp_capture_maps_fwd launch: per (image,
    head, layer, pixel, token) the 4 horizontal taps (4 packed FMA), the max (½ v_max3), the exp
    argument (1 packed FMA), v_exp_f32 (transcendental), Σ (1 packed add) and the normalised
    accumulate (1 packed FMA); per (row, low-res column, token) the 4 vertical taps."""
    per_px = 4 * _PK + 0.5 * 4.0 / 64 + _PK + _TR + _PK + _PK
    return sum(B * H * N * (per_px * R * R + 4 * _PK * R * s) for s in sizes)


def capture_maps_sel_bwd_issue_cycles(B, H, N, R, sizes):
    """Minimal VALU issue cycles of the dense part of skp_capture_maps_bwd_sel: per (image, head,
    layer, pixel, token) 4 horizontal taps, the exp argument, v_exp_f32, ×(−dot) and the 4-tap
    horizontal adjoint (packed f32 except the exp); per (row, low-res column, token) the vertical
    pass and the vertical adjoint (4 + 4 packed FMA)."""
    per_px = 4 * _PK + _PK + _TR + _PK + 4 * _PK
    return sum(B * H * N * (per_px * R * R + 8 * _PK * R * s) for s in sizes)


def capture_maps_bwd_flops(B, H, N, R, sizes):
    """Algorithmic fp32 VALU work of one skp_capture_maps_bwd call: per (image, head, layer,
    pixel, token) 24 FLOP — rebuild the softmax row (taps 8, exp argument 2, exp 1, ×1/Σ 1), a·g 1,
    Σ a·g 1, dZ = a·g − a·dot 2, horizontal adjoint 4 multiply-adds (8) — and per (row, low-res
    column, token) 8 each for the vertical pass and the vertical adjoint."""
    return sum(B * H * N * (24 * R * R + 16 * R * s) for s in sizes)


def capture_maps_bwd_bytes(B, H, N, R, sizes):
    """Algorithmic HBM bytes of one skp_capture_maps_bwd call: the map gradient read once (and
    its pixel-major copy written and read once), every z_low and stats read once, the row
    partials written and read once, dz_low written once."""
    RR = R * R
    return 4 * (3 * B * N * RR + sum(2 * B * H * s * s * N + 2 * B * H * RR + 2 * B * H * R * s * N for s in sizes))


def capture_bwd_ws_floats(BH, s, N, R):
    """Floats of skp_capture_bwd's workspace: the (BH, R, s, N) row partials."""
    return BH * R * s * N


def capture_maps_bwd_ws_floats(B, H, N, R, sizes):
    """Floats of skp_capture_maps_bwd's workspace: the (B, R², N) gradient, then the widest row partials."""
    return B * R * R * N + capture_bwd_ws_floats(B * H, max(sizes), N, R)


class CaptureMaps(torch.autograd.Function):
    """Per-image maps straight from the captured layers' logits (fused capture + aggregate).

    zs[l]: (B·H, s_l², N) logits of captured layer l.  Output (B, N, R, R):
    map[b] = mean over layers and the H heads of image b of softmax(bicubic(z)).
    One launch of skp_capture_maps_fwd: the (B·H, R², N) attention is never written; only the
    per-pixel softmax stats are kept for the backward, which hands each layer's kernel the
    per-image map gradient as a broadcast (group = H), so no (B·H, R², N) gradient is
    materialised either.
    """

    @staticmethod
    def forward(ctx, B, R, sizes, *zs):
        zs = [_c16(z) for z in zs]
        BH, _, N = zs[0].shape
        H, L = BH // B, len(zs)
        dev, RR = zs[0].device, R * R
        if FUSED_MAPS:
            out, stats = _capture_maps_run(zs, sizes, B, R)
        else:
            # every layer's attention and softmax stats (kept for the backward), then each image's map
            attn, stats = zip(*[_capture_fwd_run(z, s, R, with_stats=True) for z, s in zip(zs, sizes)])
            out = torch.empty(B, N, R, R, device=dev, dtype=F32)
            for b in range(B):
                with _timed("skp_aggregate", (L * H * RR * N + N * RR) * 4):
                    call("skp_aggregate", _layer_ptrs(attn, b * H * RR * N * 4), L, H, RR, N, None, N, ptr(out[b]),
                         stream(dev))
        ctx.save_for_backward(*zs, *stats)
        ctx.meta = (B, H, R, N, list(sizes))
        return out

    @staticmethod
    def backward(ctx, dmaps):
        saved = ctx.saved_tensors
        L = len(saved) // 2
        return (None, None, None) + tuple(CaptureMaps._dense_bwd(saved[:L], saved[L:], ctx.meta, dmaps))

    @staticmethod
    def _dense_bwd(zs, stats, meta, dmaps):
        """dz_low of every layer for a dense per-image map gradient dmaps (B, N, R, R)."""
        B, H, R, N, sizes = meta
        dmaps = _c(dmaps)                       # (B, N, R, R)
        RR, L = R * R, len(zs)
        scale = 1.0 / float(L * H)
        if FUSED_MAPS and N % 4 == 0:
            dzs = [torch.empty_like(z) for z in zs]
            ws = torch.empty(capture_maps_bwd_ws_floats(B, H, N, R, sizes), device=dmaps.device, dtype=F32)
            with _timed("skp_capture_maps_bwd", capture_maps_bwd_bytes(B, H, N, R, sizes),
                        capture_maps_bwd_flops(B, H, N, R, sizes)):
                call("skp_capture_maps_bwd", _layer_ptrs(zs), _layer_sizes(sizes), L, B, H, N, R, ptr(dmaps), scale,
                     _layer_ptrs(stats), _layer_ptrs(dzs), ptr(ws), stream(dmaps.device))
        else:
            dzs = [capture_bwd(z, s, R, dmaps, gscale=scale, group=H, strides=(N * RR, 1, RR), stats=st)
                   for z, s, st in zip(zs, sizes, stats)]
        return dzs


def capture_maps(zs, sizes, B, R):
    """Per-image (B, N, R, R) maps from captured logits (see CaptureMaps)."""
    return CaptureMaps.apply(int(B), int(R), tuple(int(s) for s in sizes), *zs)


# A/B: 0 = the selected rows' gradient goes through the dense (B, N, R²) map gradient and
# skp_capture_maps_bwd, as in r02
SEL_BWD = True   # tests switch it: False = the dense map gradient + skp_capture_maps_bwd
# skp_capture_maps_bwd_sel's per-image row limit (32-bit lane masks in csrc/skp_capture_sel.hip);
# more selected rows per image (a user --top_k > 32) take the dense backward
SEL_MAXK = 32


def capture_maps_sel_bwd_bytes(B, H, N, R, sizes, K):
    """Algorithmic HBM bytes of one skp_capture_maps_bwd_sel call (fast path), per layer: z_low read
    and dz_low written once, the stats read once, the per-pixel (mb, d) pairs and the K selected
    rows' e = a·g written and read once, the K gradient rows read once."""
    RR = R * R
    BH = B * H
    return 4 * sum(2 * BH * s * s * N + 2 * BH * RR + 4 * BH * RR + 2 * BH * K * RR + B * K * RR for s in sizes)


def capture_maps_sel_bwd_flops(B, H, N, R, sizes):
    """Algorithmic fp32 VALU work of the dense part of skp_capture_maps_bwd_sel: per (image, head,
    layer, pixel, token) 20 FLOP — rebuild a (taps 8, exp argument 2, exp 1), ×(−dot) 1, horizontal
    adjoint 8 — and per (row, low-res column, token) 8 each for the vertical pass and the vertical
    adjoint.  (The sparse part, K tokens per pixel, is not counted.)"""
    return sum(B * H * N * (20 * R * R + 16 * R * s) for s in sizes)


class CapturedMaps:
    """The fused capture's per-image maps (B, N, R, R) — computed without an autograd graph —
    plus what the backward needs (the logits ``zs`` with their graph, the per-pixel softmax stats).

    ``maps`` feeds the selection (no gradient, as in the reference: top-k / FPS run on detached
    maps); ``select(rows)`` gathers the selected token rows of every image as ONE differentiable
    (M, R, R) tensor whose backward is the sparse ``skp_capture_maps_bwd_sel``: the K selected rows'
    gradient goes straight to the kernel, and no (B, N, R²) map gradient is ever formed
    (reference optimize.py:403-424 only differentiates maps[top_embedding_indices])."""

    def __init__(self, zs, sizes, B, R):
        self.zs = list(zs)
        # called once by select()'s backward right after the capture backward is enqueued (on the
        # autograd thread, the main stream current), then cleared
        self.after_backward = None
        self.sizes = tuple(int(s) for s in sizes)
        self.B, self.R = int(B), int(R)
        with torch.no_grad():
            self.maps, self.stats = _capture_maps_run([z.detach() for z in self.zs], self.sizes, self.B, self.R)
        BH, _, N = self.zs[0].shape
        self.H, self.N = BH // self.B, N

    def select(self, rows):
        """rows: per image a 1-D int64 tensor of token ids (or None) -> cat_b maps[b, rows[b]]."""
        if len(rows) != self.B:
            raise ValueError(f"select: {len(rows)} row lists for {self.B} images")
        counts = [0 if r is None else int(r.numel()) for r in rows]
        toks = [r.to(device=self.maps.device, dtype=torch.int64).reshape(-1) for r, c in zip(rows, counts) if c]
        tok = torch.cat(toks) if toks else torch.empty(0, dtype=torch.int64, device=self.maps.device)
        return _SelectMaps.apply(self, tok, tuple(counts), *self.zs)


def _capture_maps_run(zs, sizes, B, R):
    """skp_capture_maps_fwd: (maps (B, N, R, R), per-layer stats (B·H, R², 2))."""
    zs = [_c16(z) for z in zs]
    BH, _, N = zs[0].shape
    H, L = BH // B, len(zs)
    dev, RR = zs[0].device, R * R
    stats = [torch.empty(BH, RR, 2, device=dev, dtype=F32) for _ in range(L)]
    out = torch.empty(B, N, R, R, device=dev, dtype=F32)
    with _timed("skp_capture_maps_fwd", capture_maps_bytes(B, H, N, R, sizes), capture_maps_flops(B, H, N, R, sizes),
                capture_maps_issue_cycles(B, H, N, R, sizes)):
        call("skp_capture_maps_fwd", _layer_ptrs(zs), _layer_sizes(sizes), L, B, H, N, R, ptr(out), _layer_ptrs(stats),
             stream(dev))
    return out, stats


def capture_maps_bwd_sel(zs, sizes, B, R, tok_table, gsel, gscale, stats):
    """dz_low of every layer for a sparse per-image map gradient: image b's gradient is
    gsel[b, k] (R²) at token tok_table[b, k] (−1 = unused), zero elsewhere (skp_capture_maps_bwd_sel)."""
    zs = [_c16(z) for z in zs]
    BH, _, N = zs[0].shape
    H, L = BH // B, len(zs)
    K, dev = tok_table.shape[1], zs[0].device
    sp = _layer_sizes(sizes)
    nws = _lib.lib().skp_capture_maps_bwd_sel_workspace(sp, L, B, H, N, R, K)
    if nws < 0:
        raise ValueError(f"capture_maps_bwd_sel: bad shape B={B} H={H} N={N} R={R} K={K} sizes={sizes}")
    ws = torch.empty(int(nws), device=dev, dtype=F32)
    dzs = [torch.empty_like(z) for z in zs]
    tok_table = tok_table.to(device=dev, dtype=torch.int64).contiguous()
    gsel = _c(gsel)
    with _timed("skp_capture_maps_bwd_sel", capture_maps_sel_bwd_bytes(B, H, N, R, sizes, K),
                capture_maps_sel_bwd_flops(B, H, N, R, sizes), capture_maps_sel_bwd_issue_cycles(B, H, N, R, sizes)):
        call("skp_capture_maps_bwd_sel", _layer_ptrs(zs), sp, L, B, H, N, R, ptr(tok_table), K, ptr(gsel),
             float(gscale), _layer_ptrs(stats), _layer_ptrs(dzs), ptr(ws), stream(dev))
    return dzs


class _SelectMaps(torch.autograd.Function):
    """cat_b maps[b, rows_b] with the sparse capture backward (see CapturedMaps.select)."""

    @staticmethod
    def forward(ctx, cm, tok, counts, *zs):
        B, N, R = cm.B, cm.N, cm.R
        img = torch.cat([torch.full((c,), b, dtype=torch.int64, device=tok.device) for b, c in enumerate(counts) if c]) \
            if tok.numel() else tok
        flat = img * N + tok   # every selected row's index in the (B·N, R²) view of the maps
        out = cm.maps.view(B * N, R * R)[flat].view(-1, R, R)
        ctx.cm, ctx.counts = cm, counts
        ctx.save_for_backward(tok, flat)
        return out

    @staticmethod
    def backward(ctx, g):
        cm, counts = ctx.cm, ctx.counts
        tok, flat = ctx.saved_tensors
        B, N, R, L = cm.B, cm.N, cm.R, len(cm.zs)
        RR = R * R
        K = max(max(counts), 1)
        g = _c(g).view(-1, RR)
        scale = 1.0 / float(L * cm.H)
        if SEL_BWD and N % 4 == 0 and K <= SEL_MAXK:
            # (B, K) token table (−1 pads) and the (B, K, R²) gradient rows, in row order per image
            tt = torch.full((B, K), -1, dtype=torch.int64, device=g.device)
            gs = torch.zeros(B, K, RR, dtype=F32, device=g.device)
            off = 0
            for b, c in enumerate(counts):
                if c:
                    tt[b, :c] = tok[off:off + c]
                    gs[b, :c] = g[off:off + c]
                    off += c
            dzs = capture_maps_bwd_sel(cm.zs, cm.sizes, B, R, tt, gs, scale, cm.stats)
        else:
            dense = torch.zeros(B * N, RR, dtype=F32, device=g.device)
            dense.index_add_(0, flat, g)
            dzs = CaptureMaps._dense_bwd([_c(z) for z in cm.zs], cm.stats, (B, cm.H, R, N, list(cm.sizes)),
                                         dense.view(B, N, R, R))
        cb, cm.after_backward = cm.after_backward, None
        if cb is not None:    # e.g. TokenOptimizer's VAE prefetch, enqueued behind the capture backward
            cb()
        return (None, None, None) + tuple(dzs)


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ro):
        x = _c(x)
        C, R, _ = x.shape
        out = torch.empty(C, Ro, Ro, device=x.device, dtype=F32)
        call("skp_resize_bilinear", ptr(x), C, R, Ro, ptr(out), stream(x.device))
        ctx.R = R
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        C, Ro, _ = g.shape
        gin = torch.empty(C, ctx.R, ctx.R, device=g.device, dtype=F32)
        call("skp_resize_bilinear_bwd", ptr(g), C, ctx.R, Ro, ptr(gin), stream(g.device))
        return gin, None


def resize_bilinear(x, Ro):
    """(C, R, R) -> (C, Ro, Ro), F.interpolate(bilinear, align_corners=False) (optimize.py:63-70)."""
    _lib.require_device(x)
    return _Resize.apply(x, int(Ro))


# --------------------------------------------------------------------------- A4-A6 argmax family
def find_max_pixel(maps):
    _lib.require_device(maps)
    maps = _c(maps)
    T, h, w = maps.shape
    pos = torch.empty(T, 2, device=maps.device, dtype=F32)
    call("skp_argmax2d", ptr(maps), T, h, w, None, 0, ptr(pos), None, stream(maps.device))
    return pos


def argmax_index(maps):
    maps = _c(maps)
    T, h, w = maps.shape
    idx = torch.empty(T, device=maps.device, dtype=torch.int64)
    call("skp_argmax2d", ptr(maps), T, h, w, None, 0, None, ptr(idx), stream(maps.device))
    return idx


def _square(name, t):
    """Sharpening and the KL target are defined for square maps only (the reference builds an h×h
    target for an (h, w) map and fails on the mismatch); the kernels mix /w and ·h."""
    if t.shape[-2] != t.shape[-1]:
        raise ValueError(f"{name} must hold square maps (h == w), got {tuple(t.shape)}")


def _radius2(h):
    r = 0.05 * h
    return float(r ** 2)


def find_k_max_pixels(maps, num=3, return_masked=False):
    _lib.require_device(maps)
    maps = _c(maps)
    T, h, w = maps.shape
    pos = torch.empty(num, T, 2, device=maps.device, dtype=F32)
    masked = torch.empty_like(maps) if return_masked else None
    call("skp_k_max_pixels", ptr(maps), T, h, w, int(num), _radius2(h), ptr(pos), ptr(masked), stream(maps.device))
    return (pos, masked) if return_masked else pos


def mask_radius(maps, max_coords, radius):
    _lib.require_device(maps)
    maps = _c(maps)
    T, h, w = maps.shape
    out = torch.empty_like(maps)
    call("skp_mask_radius", ptr(maps), T, h, w, ptr(_c(max_coords)), float(radius) ** 2, ptr(out),
         stream(maps.device))
    return out


def pixel_from_weighted_avg(heatmaps, distance=5):
    """Mutates ``heatmaps`` in place like the reference (eval.py:137) when it is contiguous fp32."""
    _lib.require_device(heatmaps)
    T, h, w = heatmaps.shape
    work = heatmaps if (heatmaps.is_contiguous() and heatmaps.dtype == F32) else heatmaps.float().contiguous()
    pos = torch.empty(T, 2, device=heatmaps.device, dtype=F32)
    call("skp_weighted_avg", ptr(work), T, h, w, float(distance) if distance != -1 else -1.0, 1, ptr(pos),
         stream(heatmaps.device))
    if work is not heatmaps:
        heatmaps.copy_(work)
    return pos


# --------------------------------------------------------------------------- A7 targets
def gaussian_circles(pos, size, sigma):
    """pos (num, T, 2) in [0,1] -> (T, size, size); (T, 2) is treated as num = 1."""
    _lib.require_device(pos)
    pos = _c(pos)
    if pos.dim() == 2:
        pos = pos.unsqueeze(0)
    num, T, _ = pos.shape
    out = torch.empty(T, size, size, device=pos.device, dtype=F32)
    call("skp_gaussian_target", ptr(pos), num, T, int(size), float(sigma), ptr(out), stream(pos.device))
    return out


# --------------------------------------------------------------------------- A8-A10 selection
def find_top_k_gaussian(maps, top_k, sigma=3, epsilon=1e-5, num_subjects=1, return_kl=False):
    _lib.require_device(maps)
    _square("maps", maps)
    maps = _c(maps)
    T, h, w = maps.shape
    top_k = min(int(top_k), T)   # argsort(kl)[:top_k] (ptp_utils.py:110): at most T candidates
    out = torch.empty(top_k, device=maps.device, dtype=torch.int64)
    kl = torch.empty(T, device=maps.device, dtype=torch.float64)
    call("skp_topk_gaussian", ptr(maps), T, h, w, int(top_k), float(sigma), float(epsilon), int(num_subjects),
         ptr(out), ptr(kl), ptr(kl), stream(maps.device))
    return (out, kl) if return_kl else out


# the A8 top-k as its own ranking launch behind the KL kernel (the fused one-launch form measured
# 2.5× slower, profiles/r05w_a8_fused_ab.txt, and was removed in r06)
def find_top_k_gaussian_batch(maps, top_k, sigma=3, epsilon=1e-5, num_subjects=1):
    """find_top_k_gaussian of every image of a (nb, T, h, w) stack in one launch each for the KL
    ranking and the sort: (nb, top_k) int64, row b = find_top_k_gaussian(maps[b], ...)."""
    _lib.require_device(maps)
    _square("maps", maps)
    maps = _c(maps)
    nb, T, h, w = maps.shape
    top_k = min(int(top_k), T)
    out = torch.empty(nb, top_k, device=maps.device, dtype=torch.int64)
    kl = torch.empty(nb, T, device=maps.device, dtype=torch.float64)
    # the whole A8 call (algorithmic bytes: every map read once, the keys written) in one timed
    # scope: the KL ranking launch and the ranking of the keys
    with _timed("skp_topk_gaussian_batch", maps.numel() * 4 + nb * T * 8):
        # the KL ranking launch, then (top_k > 0) the ranking of its keys, both on this stream
        call("skp_topk_gaussian_batch", ptr(maps), nb, T, h, w, int(top_k), float(sigma), float(epsilon),
             int(num_subjects), ptr(out), ptr(kl), ptr(kl), stream(maps.device))
    return out


def furthest_point_sampling_batch(maps, top_k, candidates):
    """furthest_point_sampling of every image of a (nb, T, h, w) stack, candidates (nb, C) token
    ids per image, in one argmax and one FPS launch.  Returns ((nb, top_k) int64, (nb,) int32)."""
    _lib.require_device(maps)
    maps = _c(maps)
    nb, T, h, w = maps.shape
    cand = candidates.to(device=maps.device, dtype=torch.int64).contiguous()
    if cand.dim() != 2 or cand.shape[0] != nb:
        raise ValueError(f"candidates {tuple(cand.shape)} for {nb} images")
    out = torch.empty(nb, top_k, device=maps.device, dtype=torch.int64)
    n_out = torch.empty(nb, device=maps.device, dtype=torch.int32)
    ws = torch.empty(2 * cand.numel(), device=maps.device, dtype=F32)
    call("skp_fps_batch", ptr(maps), nb, T, h, w, ptr(cand), cand.shape[1], int(top_k), ptr(out), ptr(n_out),
         ptr(ws), stream(maps.device))
    return out, n_out


def fps_from_keys_batch(keys, maps, n_cand, top_k):
    """Per image b: the n_cand tokens of smallest keys[b] (torch.argsort order: NaN last, ties by
    index), then furthest_point_sampling(maps[b], top_k, those candidates) — skp_fps_keys_batch:
    the ranking and the candidates' argmax in one launch, then FPS.  keys (nb, T) float64, maps
    (nb, T, h, w).  Returns ((nb, top_k) int64, (nb,) int32 counts, (nb, n_cand) candidates)."""
    _lib.require_device(maps)
    maps = _c(maps)
    nb, T, h, w = maps.shape
    keys = keys.to(device=maps.device, dtype=torch.float64).contiguous()
    if tuple(keys.shape) != (nb, T):
        raise ValueError(f"keys {tuple(keys.shape)} for maps {tuple(maps.shape)}")
    n_cand = min(int(n_cand), T)
    dev = maps.device
    cand = torch.empty(nb, n_cand, device=dev, dtype=torch.int64)
    out = torch.empty(nb, top_k, device=dev, dtype=torch.int64)
    n_out = torch.empty(nb, device=dev, dtype=torch.int32)
    ws = torch.empty(2 * nb * n_cand, device=dev, dtype=F32)
    call("skp_fps_keys_batch", ptr(keys), ptr(maps), nb, T, h, w, n_cand, int(top_k), ptr(cand), ptr(out), ptr(n_out),
         ptr(ws), stream(dev))
    return out, n_out, cand


def gaussian_fps_batch(maps, maps_t, n_cand, top_k, sigma=3, epsilon=1e-5, num_subjects=1):
    """The training pass's selection for every image of a stack (optimize.py:403-410 per replica):
    candidates = find_top_k_gaussian(maps[b], n_cand), then
    furthest_point_sampling(maps_t[b], top_k, candidates) — maps (nb, T, h, w) the images' maps,
    maps_t the maps the FPS reads (the warps').  Three launches: the KL keys
    (skp_topk_gaussian_batch, top_k 0), the ranking + the candidates' argmax on maps_t, FPS.
    Returns what fps_from_keys_batch returns: identical to find_top_k_gaussian_batch +
    furthest_point_sampling_batch."""
    _lib.require_device(maps)
    maps = _c(maps)
    nb, T, h, w = maps.shape
    if tuple(maps_t.shape) != (nb, T, h, w):
        raise ValueError(f"maps_t {tuple(maps_t.shape)} for maps {tuple(maps.shape)}")
    kl = torch.empty(nb, T, device=maps.device, dtype=torch.float64)
    # one timed scope for the pass's whole selection chain (bench: `selection`)
    with _timed("skp_selection", maps.numel() * 4 + nb * T * 8 + nb * min(int(n_cand), T) * h * w * 4):
        with _timed("skp_topk_gaussian_batch", maps.numel() * 4 + nb * T * 8):
            call("skp_topk_gaussian_batch", ptr(maps), nb, T, h, w, 0, float(sigma), float(epsilon),
                 int(num_subjects), ptr(kl), ptr(kl), ptr(kl), stream(maps.device))
        return fps_from_keys_batch(kl, maps_t, n_cand, top_k)


def entropy_keys_batch(maps):
    """The softmax entropies of every row of a (nb, T, h, w) stack (ptp_utils.py:179-182) in one
    launch: (nb, T) float64, the keys entropy_sort ranks ascending."""
    _lib.require_device(maps)
    maps = _c(maps)
    nb, T, h, w = maps.shape
    ent = torch.empty(nb, T, device=maps.device, dtype=torch.float64)
    call("skp_entropy_sort", ptr(maps), nb * T, h, w, 0, ptr(ent), ptr(ent), ptr(ent), stream(maps.device))
    return ent


def entropy_sort_batch(maps, top_k):
    """entropy_sort of every image of a (nb, T, h, w) stack: the entropies of all nb·T rows in one
    launch (skp_entropy_sort's kernel, no ranking), then the per-image ascending top_k of them in
    one skp_topk_keys launch.  (nb, top_k) int64, row b = entropy_sort(maps[b], top_k)."""
    _lib.require_device(maps)
    maps = _c(maps)
    nb, T, h, w = maps.shape
    top_k = min(int(top_k), T)
    out = torch.empty(nb, top_k, device=maps.device, dtype=torch.int64)
    ent = torch.empty(nb, T, device=maps.device, dtype=torch.float64)
    call("skp_entropy_sort", ptr(maps), nb * T, h, w, 0, ptr(out), ptr(ent), ptr(ent), stream(maps.device))
    if top_k > 0:
        call("skp_topk_keys", ptr(ent), nb, T, int(top_k), ptr(out), stream(maps.device))
    return out


def entropy_sort(maps, top_k, return_entropy=False):
    _lib.require_device(maps)
    maps = _c(maps)
    T, h, w = maps.shape
    top_k = min(int(top_k), T)   # argsort(entropy)[:top_k] (ptp_utils.py:185): at most T candidates
    out = torch.empty(top_k, device=maps.device, dtype=torch.int64)
    ent = torch.empty(T, device=maps.device, dtype=torch.float64)
    call("skp_entropy_sort", ptr(maps), T, h, w, int(top_k), ptr(out), ptr(ent), ptr(ent), stream(maps.device))
    return (out, ent) if return_entropy else out


def furthest_point_sampling(maps, top_k, candidates):
    """Returns (selected int64 (top_k,), count int32 device scalar)."""
    _lib.require_device(maps)
    maps = _c(maps)
    T, h, w = maps.shape
    cand = candidates.to(device=maps.device, dtype=torch.int64).contiguous()
    out = torch.empty(top_k, device=maps.device, dtype=torch.int64)
    n_out = torch.empty(1, device=maps.device, dtype=torch.int32)
    ws = torch.empty(2 * cand.numel(), device=maps.device, dtype=F32)
    call("skp_fps", ptr(maps), T, h, w, ptr(cand), cand.numel(), int(top_k), ptr(out), ptr(n_out), ptr(ws),
         stream(maps.device))
    return out, n_out


# --------------------------------------------------------------------------- A11 / A12 losses
class SharpeningLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, sigma, num_subjects):
        A = _c(A)
        T, h, w = A.shape
        pos = torch.empty(num_subjects, T, 2, device=A.device, dtype=F32)
        part = torch.empty(T, device=A.device, dtype=torch.float64)
        loss = torch.empty((), device=A.device, dtype=F32)
        call("skp_sharpen_fwd", ptr(A), T, h, w, float(sigma), int(num_subjects), ptr(pos), ptr(part), ptr(loss),
             stream(A.device))
        ctx.save_for_backward(A, pos)
        ctx.sigma, ctx.num = sigma, num_subjects
        return loss

    @staticmethod
    def backward(ctx, g):
        A, pos = ctx.saved_tensors
        T, h, w = A.shape
        dA = torch.empty_like(A)
        call("skp_sharpen_bwd", ptr(A), T, h, w, float(ctx.sigma), int(ctx.num), ptr(pos), ptr(_c(g.reshape(1))),
             ptr(dA), stream(A.device))
        return dA, None, None


def sharpening_loss(A, sigma=1.0, num_subjects=1):
    _lib.require_device(A)
    _square("A", A)
    return SharpeningLoss.apply(A, float(sigma), int(num_subjects))


class SharpeningLossBatch(torch.autograd.Function):
    """SharpeningLoss of nb images' selected rows at once: A (nb·T, h, w) → (nb,) losses, each the
    single-image loss (skp_sharpen_fwd_batch / _bwd_batch: one launch per direction)."""

    @staticmethod
    def forward(ctx, A, nb, sigma, num_subjects):
        A = _c(A)
        R, h, w = A.shape
        T = R // nb
        pos = torch.empty(num_subjects, R, 2, device=A.device, dtype=F32)
        part = torch.empty(R, device=A.device, dtype=torch.float64)
        loss = torch.empty(nb, device=A.device, dtype=F32)
        call("skp_sharpen_fwd_batch", ptr(A), nb, T, h, w, float(sigma), int(num_subjects), ptr(pos), ptr(part),
             ptr(loss), stream(A.device))
        ctx.save_for_backward(A, pos)
        ctx.meta = (nb, T, sigma, num_subjects)
        return loss

    @staticmethod
    def backward(ctx, g):
        A, pos = ctx.saved_tensors
        nb, T, sigma, num = ctx.meta
        _, h, w = A.shape
        dA = torch.empty_like(A)
        call("skp_sharpen_bwd_batch", ptr(A), nb, T, h, w, float(sigma), int(num), ptr(pos), ptr(_c(g.reshape(nb))),
             ptr(dA), stream(A.device))
        return dA, None, None, None


def sharpening_loss_batch(A, nb, sigma=1.0, num_subjects=1):
    """(nb,) sharpening losses of nb images whose T selected rows each are stacked in A (nb·T, h, w)."""
    _lib.require_device(A)
    _square("A", A)
    if A.shape[0] % nb:
        raise ValueError(f"{A.shape[0]} rows for {nb} images")
    return SharpeningLossBatch.apply(A, int(nb), float(sigma), int(num_subjects))


class AffineWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, theta):
        x = _c(x)
        B, C, H, W = x.shape
        th = _c(theta.to(x.device))
        out = torch.empty_like(x)
        call("skp_affine_warp", ptr(x), B, C, H, W, ptr(th), ptr(out), stream(x.device))
        ctx.save_for_backward(th)
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        (th,) = ctx.saved_tensors
        B, C, H, W = ctx.shape
        gin = torch.empty(B, C, H, W, device=g.device, dtype=F32)
        call("skp_affine_warp_bwd", ptr(_c(g)), B, C, H, W, ptr(th), ptr(gin), stream(g.device))
        return gin, None


def affine_warp(x, theta):
    """grid_sample(x, affine_grid(theta)) (bilinear, zeros, align_corners=False); x (B,C,H,W)."""
    _lib.require_device(x)
    return AffineWarp.apply(x, theta)


class EquivarianceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, At, theta_inv):
        A, At = _c(A), _c(At)
        T, h, w = A.shape
        th = _c(theta_inv.to(A.device)).reshape(6)
        part = torch.empty(T, device=A.device, dtype=torch.float64)
        loss = torch.empty((), device=A.device, dtype=F32)
        call("skp_equiv_fwd", ptr(A), ptr(At), T, h, w, ptr(th), ptr(part), ptr(loss), stream(A.device))
        ctx.save_for_backward(A, At, th)
        return loss

    @staticmethod
    def backward(ctx, g):
        A, At, th = ctx.saved_tensors
        T, h, w = A.shape
        dA = torch.empty_like(A) if ctx.needs_input_grad[0] else None
        dAt = torch.empty_like(At)
        call("skp_equiv_bwd", ptr(A), ptr(At), T, h, w, ptr(th), ptr(_c(g.reshape(1))), ptr(dA), ptr(dAt),
             stream(A.device))
        return dA, (dAt if ctx.needs_input_grad[1] else None), None


def equivariance_loss_single(A, At, theta_inv):
    """mean((A − warp(At, theta_inv))²) with gradients into A and At."""
    _lib.require_device(A, At)
    return EquivarianceLoss.apply(A, At, theta_inv)


class EquivarianceLossBatch(torch.autograd.Function):
    """EquivarianceLoss of nb replicas at once: A, At (nb·T, h, w), theta_inv (nb, 2, 3) → (nb,)
    losses, each the single-replica loss (skp_equiv_fwd_batch / _bwd_batch)."""

    @staticmethod
    def forward(ctx, A, At, theta_inv, nb):
        A, At = _c(A), _c(At)
        R, h, w = A.shape
        T = R // nb
        th = _c(theta_inv.to(A.device)).reshape(nb * 6)
        part = torch.empty(R, device=A.device, dtype=torch.float64)
        loss = torch.empty(nb, device=A.device, dtype=F32)
        call("skp_equiv_fwd_batch", ptr(A), ptr(At), nb, T, h, w, ptr(th), ptr(part), ptr(loss), stream(A.device))
        ctx.save_for_backward(A, At, th)
        ctx.meta = (nb, T)
        return loss

    @staticmethod
    def backward(ctx, g):
        A, At, th = ctx.saved_tensors
        nb, T = ctx.meta
        _, h, w = A.shape
        dA = torch.empty_like(A) if ctx.needs_input_grad[0] else None
        dAt = torch.empty_like(At)
        call("skp_equiv_bwd_batch", ptr(A), ptr(At), nb, T, h, w, ptr(th), ptr(_c(g.reshape(nb))), ptr(dA), ptr(dAt),
             stream(A.device))
        return dA, (dAt if ctx.needs_input_grad[1] else None), None, None


def equivariance_loss_batch(A, At, theta_inv, nb):
    """(nb,) equivariance losses of nb replicas (T selected rows each, stacked in A / At)."""
    _lib.require_device(A, At)
    if A.shape[0] % nb or theta_inv.numel() != 6 * nb:
        raise ValueError(f"{A.shape[0]} rows / theta_inv {tuple(theta_inv.shape)} for {nb} images")
    return EquivarianceLossBatch.apply(A, At, theta_inv, int(nb))


# --------------------------------------------------------------------------- UNet-side GroupNorm(+SiLU)
# GN_EPI (tests set False to compare): the Winograd convolution's epilogue writes per-segment (mean, M2) of
# its output (skp_conv3x3_wino2_gn) and a GroupNorm reading that output takes its statistics from
# them (skp_groupnorm_fwd_part) instead of a pass over the activation.
GN_EPI = True   # tests switch it: False = GroupNorm computes its own statistics


def _gn_parts_of(x):
    """The (mean, M2) segment partials the producing convolution left on ``x`` (None: none, or x was
    modified in place since)."""
    ent = getattr(x, "_skp_gn", None)
    if ent is None or ent[0] != x._version:
        return None
    return ent[1], ent[2]


def _gn_fwd(x, gamma, beta, shift, groups, eps, act):
    """act(GroupNorm(x + shift)) forward: (y, stats, g, b, nws) — skp_groupnorm_fwd, or
    skp_groupnorm_fwd_part when x carries its producer's statistics partials."""
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    nws = _lib.lib().skp_groupnorm_workspace(B, C, HW, groups)
    if nws < 0:
        raise ValueError(f"groupnorm: bad shape {tuple(x.shape)} groups={groups}")
    part = torch.empty(nws, device=x.device, dtype=torch.float64)
    stats = torch.empty(B * groups * 2, device=x.device, dtype=F32)
    y = torch.empty_like(x)
    g, b = _c(gamma.detach()), _c(beta.detach())
    pre = _gn_parts_of(x) if GN_EPI else None
    if pre is not None:
        call("skp_groupnorm_fwd_part", ptr(x), ptr(g), ptr(b), ptr(shift), ptr(pre[0]), pre[1], B, C, HW,
             int(groups), float(eps), int(act), ptr(y), ptr(stats), ptr(part), stream(x.device))
    else:
        call("skp_groupnorm_fwd", ptr(x), ptr(g), ptr(b), ptr(shift), B, C, HW, int(groups), float(eps), int(act),
             ptr(y), ptr(stats), ptr(part), stream(x.device))
    return y, stats, g, b, nws


class GroupNormAct(torch.autograd.Function):
    """y = act(GroupNorm(x + shift)) with frozen affine parameters (dx only) — skp_groupnorm_fwd/bwd.
    ``shift`` (B, C) or None: a per-(sample, channel) input offset (conv bias + time embedding)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, act, shift):
        x = _c(x)
        B, C = x.shape[:2]
        HW = x[0, 0].numel()
        if shift is not None:
            shift = _c(shift.detach().expand(B, C))
        y, stats, g, b, nws = _gn_fwd(x, gamma, beta, shift, groups, eps, act)
        ctx.save_for_backward(x, g, b, stats, shift)
        ctx.meta = (B, C, HW, int(groups), int(act), nws)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, b, stats, shift = ctx.saved_tensors
        B, C, HW, G, act, nws = ctx.meta
        dy = _c(dy)
        dx = torch.empty_like(x)
        part = torch.empty(nws, device=x.device, dtype=torch.float64)
        call("skp_groupnorm_bwd", ptr(x), ptr(dy), ptr(g), ptr(b), ptr(shift), ptr(stats), B, C, HW, G, act, ptr(dx),
             ptr(part), stream(x.device))
        return dx, None, None, None, None, None, None


class GroupNormActRes(torch.autograd.Function):
    """GroupNormAct that also hands x on (``x_pass``, the same values) to its other consumer — the
    residual or shortcut of a ResNet block / spatial transformer — so that consumer's gradient
    comes back to THIS node and is added inside the backward kernel (skp_groupnorm_bwd_add) instead
    of by a separate autograd accumulation pass over the activation."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, act, shift):
        xc = _c(x)
        B, C = xc.shape[:2]
        HW = xc[0, 0].numel()
        if shift is not None:
            shift = _c(shift.detach().expand(B, C))
        y, stats, g, b, nws = _gn_fwd(xc, gamma, beta, shift, groups, eps, act)
        ctx.save_for_backward(xc, g, b, stats, shift)
        ctx.meta = (B, C, HW, int(groups), int(act), nws)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dpass):
        x, g, b, stats, shift = ctx.saved_tensors
        B, C, HW, G, act, nws = ctx.meta
        dy = _c(dy)
        dres = None if dpass is None else _c16(dpass)
        dx = torch.empty_like(x)
        part = torch.empty(nws, device=x.device, dtype=torch.float64)
        call("skp_groupnorm_bwd_add", ptr(x), ptr(dy), ptr(g), ptr(b), ptr(shift), ptr(stats), B, C, HW, G, act,
             ptr(dres), ptr(dx), ptr(part), stream(x.device))
        return dx, None, None, None, None, None, None


def group_norm_act_res(x, gamma, beta, groups, eps, act):
    """(act(GroupNorm(x)), x) where the second output is x for the node's other consumer: its
    gradient is added by the GroupNorm backward kernel (GroupNormActRes)."""
    _lib.require_device(x)
    return GroupNormActRes.apply(x, gamma, beta, int(groups), float(eps), bool(act), None)


def group_norm_act(x, gamma, beta, groups, eps, act, shift=None):
    """Fused GroupNorm(x + shift) (+SiLU when act) on the HIP device; frozen gamma/beta.
    ``shift``: None or a (B, C) / (1, C) / (C,) per-channel input offset without gradient."""
    _lib.require_device(x)
    if shift is not None:
        shift = shift.reshape(-1, x.shape[1]).to(x.device, F32)
    return GroupNormAct.apply(x, gamma, beta, int(groups), float(eps), bool(act), shift)


class ResidualBiasAdd(torch.autograd.Function):
    """out = a + (h + bias[c]) (bias frozen): gradients pass through to a and h."""

    @staticmethod
    def forward(ctx, a, h, bias):
        a, h = _c(a), _c(h)
        B, C = a.shape[:2]
        out = torch.empty_like(a)
        call("skp_residual_bias_add", ptr(a), ptr(h), ptr(_c(bias.detach())), B, C, a[0, 0].numel(), ptr(out),
             stream(a.device))
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g, None


def residual_bias_add(a, h, bias):
    """a + (h + bias[:, None, None]) for NCHW a, h on the HIP device."""
    _lib.require_device(a, h)
    if a.shape != h.shape:
        raise ValueError(f"residual_bias_add: shapes {tuple(a.shape)} and {tuple(h.shape)} differ")
    return ResidualBiasAdd.apply(a, h, bias)


def softmax_(s):
    """In-place row softmax of a contiguous fp32 (…, cols) tensor (skp_softmax_fwd), torch
    semantics; falls back to torch's when cols is not a multiple of 4."""
    if s.dtype != F32 or not s.is_contiguous() or s.shape[-1] % 4 or s.shape[-1] > 16384 or \
            s.data_ptr() % 16:
        return s.copy_(s.softmax(dim=-1))
    call("skp_softmax_fwd", ptr(s), s.numel() // s.shape[-1], s.shape[-1], stream(s.device))
    return s


def attention_probs(q, k, scale):
    """softmax(q kᵀ·scale) for (B·H, S, D) q and (B·H, S', D) k: hipBLASLt baddbmm, then the
    softmax in place (skp_softmax_fwd)."""
    sim = torch.baddbmm(torch.empty(q.shape[0], q.shape[1], k.shape[1], dtype=q.dtype, device=q.device),
                        q, k.transpose(1, 2), beta=0, alpha=scale)
    return softmax_(sim)


def attention_nograd(q, k, v, scale):
    """softmax(q kᵀ·scale) v when no gradient is needed: the fused online-softmax kernel
    (skp_attn_fwd, no score tensor; any key count) where the shapes allow, else the scores +
    in-place softmax."""
    BH, S, d = q.shape
    L = k.shape[1]
    if (q.dtype == F32 and S % 64 == 0 and d in (40, 64, 80) and q.is_contiguous()
            and k.is_contiguous() and v.is_contiguous()):
        out = torch.empty_like(q)
        call("skp_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(out), None, BH, S, L, d, float(scale), stream(q.device))
        return out
    return torch.bmm(attention_probs(q, k, scale), v)


# head dims routed to skp_attn_bwd_kv: d = 40 measured faster end to end (2 waves per SIMD fit);
# d = 64 / 80 run at one wave per SIMD and measured slower than the unfused path.
# (tests route every supported head dim through it, or none)
ATTN_FUSED_KV = (40,)


class MathAttention(torch.autograd.Function):
    """softmax(q kᵀ·scale) v over (B·H, S, D) (diffusers-0.8.0 math path): hipBLASLt GEMMs and
    the in-place skp_softmax_fwd.  Backward: dV = Pᵀ dO (hipBLASLt), then the score gradient
    with baddbmm's scale folded in — one skp_attn_dscore pass over P (dO·Vᵀ on the matrix
    cores, never materialised; D = rowsum(dO ⊙ O)) where the shapes allow, else dP = dO Vᵀ and
    one skp_softmax_bwd pass written over it — then dQ = dS K, dK = dSᵀ Q.  When K needs a
    gradient and d ∈ ATTN_FUSED_KV, skp_attn_bwd_kv produces dS, dV and dK in one pass over P
    (dV, dK accumulated on the matrix cores per key block); only dQ = dS K stays a GEMM."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        p = attention_probs(q, k, scale)
        out = torch.bmm(p, v)
        ctx.save_for_backward(q, k, v, p, out)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, p, out = ctx.saved_tensors
        dout = dout.contiguous()
        BH, S, L = p.shape
        d = q.shape[2]
        if (d in ATTN_FUSED_KV and S % 64 == 0 and L % 64 == 0 and ctx.needs_input_grad[1]
                and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (q, v, dout))):
            D = (dout * out).sum(-1)
            ds, dv, dk = torch.empty_like(p), torch.empty_like(v), torch.empty_like(k)
            call("skp_attn_bwd_kv", ptr(p), ptr(dout), ptr(q), ptr(v), ptr(D), ptr(ds), ptr(dv), ptr(dk),
                 BH, S, L, d, float(ctx.scale), stream(p.device))
            dq = torch.bmm(ds, k) if ctx.needs_input_grad[0] else None
            return dq, dk, dv if ctx.needs_input_grad[2] else None, None
        dv = torch.bmm(p.transpose(1, 2), dout) if ctx.needs_input_grad[2] else None
        dq = dk = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            if S % 64 == 0 and L % 64 == 0 and d in (40, 64, 80, 160) and v.is_contiguous():
                D = (dout * out).sum(-1)
                ds = torch.empty_like(p)
                call("skp_attn_dscore", ptr(p), ptr(dout), ptr(v), ptr(D), ptr(ds), BH, S, L, d,
                     float(ctx.scale), stream(p.device))
            else:
                ds = torch.bmm(dout, v.transpose(1, 2))             # dP, overwritten by scale·dS
                call("skp_softmax_bwd", ptr(p), ptr(ds), p.shape[0] * p.shape[1], p.shape[2], float(ctx.scale),
                     stream(p.device))
            dq = torch.bmm(ds, k) if ctx.needs_input_grad[0] else None
            dk = torch.bmm(ds.transpose(1, 2), q) if ctx.needs_input_grad[1] else None
        return dq, dk, dv, None


class LayerNormFn(torch.autograd.Function):
    """LayerNorm over the last dimension with frozen γ, β (input gradient only) —
    skp_layernorm_fwd/bwd, one wave per row."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = _c(x)
        C = x.shape[-1]
        rows = x.numel() // C
        y = torch.empty_like(x)
        stats = torch.empty(rows, 2, device=x.device, dtype=F32)
        w, b = _c(weight.detach()), _c(bias.detach())
        call("skp_layernorm_fwd", ptr(x), ptr(w), ptr(b), rows, C, float(eps), ptr(y), ptr(stats), stream(x.device))
        ctx.save_for_backward(x, w, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, stats = ctx.saved_tensors
        dy = _c(dy)
        C = x.shape[-1]
        dx = torch.empty_like(x)
        call("skp_layernorm_bwd", ptr(x), ptr(dy), ptr(w), ptr(stats), x.numel() // C, C, ptr(dx), stream(x.device))
        return dx, None, None, None


class LayerNormRes(torch.autograd.Function):
    """LayerNormFn that also hands x on (``x_pass``) to the transformer block's residual add, so the
    residual's gradient is added inside the backward kernel (skp_layernorm_bwd_add) rather than by
    a separate autograd accumulation pass (h = attn(norm(h)) + h, diffusers attention.py)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        xc = _c(x)
        C = xc.shape[-1]
        rows = xc.numel() // C
        y = torch.empty_like(xc)
        stats = torch.empty(rows, 2, device=xc.device, dtype=F32)
        w, b = _c(weight.detach()), _c(bias.detach())
        call("skp_layernorm_fwd", ptr(xc), ptr(w), ptr(b), rows, C, float(eps), ptr(y), ptr(stats), stream(xc.device))
        ctx.save_for_backward(xc, w, stats)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dpass):
        x, w, stats = ctx.saved_tensors
        dy = _c(dy)
        dres = None if dpass is None else _c16(dpass)
        C = x.shape[-1]
        dx = torch.empty_like(x)
        call("skp_layernorm_bwd_add", ptr(x), ptr(dy), ptr(w), ptr(stats), x.numel() // C, C, ptr(dres), ptr(dx),
             stream(x.device))
        return dx, None, None, None


def layer_norm_res(x, weight, bias, eps):
    """(F.layer_norm(x, …), x) with the second output for the residual add: its gradient joins the
    LayerNorm backward kernel (LayerNormRes).  Shapes the kernel does not take: torch's LayerNorm
    and x itself."""
    _lib.require_device(x)
    C = x.shape[-1]
    if (x.dtype != F32 or C % 4 or C > 2048 or weight is None or bias is None or weight.requires_grad
            or bias.requires_grad or x.numel() == 0 or x.numel() // C < LN_MIN_ROWS):
        return torch.nn.functional.layer_norm(x, (C,), weight, bias, eps), x
    return LayerNormRes.apply(x, weight, bias, float(eps))


# kernel time at batch 8 (tools/ln_time.py): 32768 rows × 320: 15.4 µs = 5.4 TB/s (ATen 40.8);
# 8192 × 640: 7.6 (13.8); 2048 × 1280: 7.1 (7.5).  Fewer rows than this stay on ATen.
LN_MIN_ROWS = 2048


def layer_norm(x, weight, bias, eps):
    """F.layer_norm(x, (C,), weight, bias, eps) with frozen affine parameters on the HIP device
    (skp_layernorm_*) for ≥ LN_MIN_ROWS rows; torch's form for fewer rows, other dtypes / widths."""
    _lib.require_device(x)
    C = x.shape[-1]
    if (x.dtype != F32 or C % 4 or C > 2048 or weight is None or bias is None or weight.requires_grad
            or bias.requires_grad or x.numel() == 0 or x.numel() // C < LN_MIN_ROWS):
        return torch.nn.functional.layer_norm(x, (C,), weight, bias, eps)
    return LayerNormFn.apply(x, weight, bias, float(eps))


class Geglu(torch.autograd.Function):
    """x · gelu(gate) over the two halves of a (…, 2I) projection (diffusers GEGLU): one fused
    pass each way (skp_geglu_fwd / skp_geglu_bwd)."""

    @staticmethod
    def forward(ctx, h):
        h = _c(h)
        I = h.shape[-1] // 2
        out = torch.empty(*h.shape[:-1], I, device=h.device, dtype=F32)
        call("skp_geglu_fwd", ptr(h), h.numel() // h.shape[-1], I, ptr(out), stream(h.device))
        ctx.save_for_backward(h)
        return out

    @staticmethod
    def backward(ctx, dout):
        (h,) = ctx.saved_tensors
        dout = _c(dout)
        dh = torch.empty_like(h)
        call("skp_geglu_bwd", ptr(h), ptr(dout), h.numel() // h.shape[-1], h.shape[-1] // 2, ptr(dh),
             stream(h.device))
        return dh


def geglu(h):
    """diffusers GEGLU's `x, gate = h.chunk(2, -1); x * gelu(gate)` (exact GELU) on the HIP
    device; torch's form where the half width is not a multiple of 4."""
    _lib.require_device(h)
    if h.dtype != F32 or h.shape[-1] % 8:
        x, gate = h.chunk(2, dim=-1)
        return x * torch.nn.functional.gelu(gate)
    return Geglu.apply(h)


# head dims whose grad-needing attention keeps no probability tensor (FlashAttention below);
# (tests route every supported head dim through it, or none)
ATTN_FLASH = (40, 64)


class FlashAttention(torch.autograd.Function):
    """softmax(q kᵀ·scale) v without a saved (B·H, S, L) probability tensor: the forward is the
    online-softmax skp_attn_fwd emitting per-row (max, 1/sum); the backward skp_attn_bwd_flash
    rebuilds P per key block from q kᵀ and those stats and produces dS, dV, dK in one pass
    (dQ = dS k stays a GEMM).  Same result as MathAttention within fp32 rounding."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        BH, S, d = q.shape
        L = k.shape[1]
        out = torch.empty_like(q)
        stats = torch.empty(BH, S, 2, device=q.device, dtype=F32)
        call("skp_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(out), ptr(stats), BH, S, L, d, float(scale),
             stream(q.device))
        ctx.save_for_backward(q, k, v, out, stats)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, stats = ctx.saved_tensors
        dout = dout.contiguous()
        BH, S, d = q.shape
        L = k.shape[1]
        D = (dout * out).sum(-1)
        ds = torch.empty(BH, S, L, device=q.device, dtype=F32)
        dv, dk = torch.empty_like(v), torch.empty_like(k)
        call("skp_attn_bwd_flash", ptr(q), ptr(k), ptr(v), ptr(dout), ptr(stats), ptr(D), ptr(ds), ptr(dv), ptr(dk),
             BH, S, L, d, float(ctx.scale), stream(q.device))
        dq = torch.bmm(ds, k) if ctx.needs_input_grad[0] else None
        return dq, dk if ctx.needs_input_grad[1] else None, dv if ctx.needs_input_grad[2] else None, None


def math_attention(q, k, v, scale):
    """softmax(q kᵀ·scale) v with a fused backward (HIP device): FlashAttention for the head
    dims in ATTN_FLASH when S is a multiple of 64 (any key count: the last key block is
    masked), else MathAttention."""
    _lib.require_device(q, k, v)
    BH, S, d = q.shape
    L = k.shape[1]
    if (d in ATTN_FLASH and S % 64 == 0 and q.dtype == F32
            and all(t.dtype == F32 and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (q, k, v))):
        return FlashAttention.apply(q, k, v, float(scale))
    return MathAttention.apply(q, k, v, float(scale))


# --------------------------------------------------------------------------- attention on (B, S, H·d) projections
# A/B: 0 = permute q / k / v / out between (B, S, H·d) and (B·H, S, d) around the attention kernels (r02)
ATTN_BSHD = True


def _lay(t):
    """(batch stride, row stride) of a (B, S, H·d) operand whose last dimension is unit-stride."""
    return int(t.stride(0)), int(t.stride(1))


def _bshd_ok(q, k, v, H):
    B, S, C = q.shape
    if not ATTN_BSHD or C % H or S % 64 or k.shape[-1] != C or v.shape[-1] != C:
        return False
    return all(t.is_cuda and t.dtype == F32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) % 4 == 0
               and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in (q, k, v))


class FlashAttentionBSHD(torch.autograd.Function):
    """FlashAttention on the projections' own (B, S, H·d) layout: skp_attn_fwd_bshd reads q / k / v
    and writes the output with head strides (no reshape_heads_to_batch_dim / _to_heads copies, a
    batch-shared k / v read through a zero batch stride), skp_attn_bwd_flash_bshd reads dO, q, k, v
    the same way and writes dV, dK per image in (B, L, H·d) (summed over a shared batch by the
    expand's backward).  dQ = dS·K is one torch.matmul per head (its operands are the only permutes
    left)."""

    @staticmethod
    def forward(ctx, q, k, v, H, scale):
        B, S, C = q.shape
        L = k.shape[1]
        d = C // H
        out = torch.empty(B, S, C, device=q.device, dtype=F32)
        stats = torch.empty(B * H, S, 2, device=q.device, dtype=F32)
        call("skp_attn_fwd_bshd", ptr(q), *_lay(q), ptr(k), *_lay(k), ptr(v), *_lay(v), ptr(out), S * C, C, ptr(stats),
             B, H, S, L, d, float(scale), stream(q.device))
        ctx.save_for_backward(q, k, v, out, stats)
        ctx.H, ctx.scale = H, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, stats = ctx.saved_tensors
        H, scale = ctx.H, ctx.scale
        dout = _c16(dout)
        B, S, C = q.shape
        L = k.shape[1]
        d = C // H
        D = (dout.view(B, S, H, d) * out.view(B, S, H, d)).sum(-1).transpose(1, 2).contiguous()   # (B, H, S)
        ds = torch.empty(B * H, S, L, device=q.device, dtype=F32)
        dv = torch.empty(B, L, C, device=q.device, dtype=F32)
        dk = torch.empty(B, L, C, device=q.device, dtype=F32)
        call("skp_attn_bwd_flash_bshd", ptr(q), *_lay(q), ptr(k), *_lay(k), ptr(v), *_lay(v), ptr(dout), S * C, C,
             ptr(stats), ptr(D), ptr(ds), ptr(dv), L * C, C, ptr(dk), L * C, C, B, H, S, L, d, float(scale),
             stream(q.device))
        dq = None
        if ctx.needs_input_grad[0]:
            k4 = k.view(k.shape[0], L, H, d).transpose(1, 2).expand(B, H, L, d)
            dq = torch.matmul(ds.view(B, H, S, L), k4).transpose(1, 2).reshape(B, S, C)
        return (dq, dk if ctx.needs_input_grad[1] else None, dv if ctx.needs_input_grad[2] else None, None, None)


def attention_heads(q, k, v, H, scale):
    """softmax(q kᵀ·scale) v per head for (B, S, H·d) q and (B or stride-0 B, L, H·d) k, v, output
    (B, S, H·d) — diffusers' CrossAttention between to_q/to_k/to_v and to_out without the head
    permutes.  None when the shape is not covered (the caller keeps the permuting path): the
    gradient-needing form for a batch-shared context and head dims in ATTN_FLASH, the no-grad
    online-softmax form for d ∈ {40, 64, 80}, S a multiple of 64."""
    if not _bshd_ok(q, k, v, H):
        return None
    B, S, C = q.shape
    d = C // H
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        # gradient-needing self-attention keeps the head-major copies: both kernels re-read K / V once
        # per 64-row block, and a head's 160-B rows strided by H·d touch 1.6× the cache lines; at the
        # 64² shape that costs more than the permutes (measured: 2.05 + 3.85 ms vs 1.85 + 3.38 ms for
        # the kernels, tools/attn_bshd_time.py); a batch-shared context (cross-attention) is small and
        # takes this path (0.95 vs 1.00 ms per call)
        if d not in ATTN_FLASH or k.stride(0) != 0:
            return None
        return FlashAttentionBSHD.apply(q, k, v, int(H), float(scale))
    if d not in (40, 64, 80):
        return None
    out = torch.empty(B, S, C, device=q.device, dtype=F32)
    call("skp_attn_fwd_bshd", ptr(q), *_lay(q), ptr(k), *_lay(k), ptr(v), *_lay(v), ptr(out), S * C, C, None,
         B, H, S, k.shape[1], d, float(scale), stream(q.device))
    return out


# --------------------------------------------------------------------------- UNet-side: token projections
_QKV_W = {}   # (id wq, id wk, id wv) -> ((versions), weakref(wq), [wq; wk; wv])


def _qkv_weight(*ws):
    """[w0; w1; …] of frozen projection weights, built once per weight set (and its versions): the
    entry is reused only while EVERY weight is still the object it was built from (a weakref per
    weight, so a replaced to_k / to_v never meets a stale concatenation through a reused id) with
    the same storage and version; it is dropped when any of them is collected."""
    key = tuple(id(w) for w in ws)
    sig = tuple((w._version, w.data_ptr()) for w in ws)
    ent = _QKV_W.get(key)
    if ent is not None and ent[0] == sig and all(r() is w for r, w in zip(ent[1], ws)):
        return ent[2]
    w3 = torch.cat([w.detach() for w in ws], 0).contiguous()
    drop = lambda _r, key=key: _QKV_W.pop(key, None)   # noqa: E731
    _QKV_W[key] = (sig, tuple(_weakref.ref(w, drop) for w in ws), w3)
    return w3


class QKVProjection(torch.autograd.Function):
    """q, k, v = to_q(x), to_k(x), to_v(x) of a self-attention (diffusers CrossAttention with
    context = x, bias-free, frozen) as ONE GEMM against [Wq; Wk; Wv] (x read once; q, k, v are
    column views of the (B, S, 3C) product).  Backward: dx = dq Wq, then dk Wk and dv Wv
    accumulated into it by the GEMM (beta = 1): no separate gradient-sum passes over dx."""

    @staticmethod
    def forward(ctx, x, w3, C):
        out = torch.matmul(x, w3.t())
        ctx.save_for_backward(w3)
        ctx.C = C
        ctx.x_shape = x.shape
        ctx.set_materialize_grads(False)   # an unused projection's gradient stays None (skipped)
        return tuple(out[..., i * C:(i + 1) * C] for i in range(w3.shape[0] // C))

    @staticmethod
    def backward(ctx, *grads):
        (w3,) = ctx.saved_tensors
        C = ctx.C
        dx = None
        for i, g in enumerate(grads):
            if g is None:
                continue
            g2 = g.reshape(-1, C)
            wi = w3[i * C:(i + 1) * C]
            if dx is None:
                dx = torch.mm(g2, wi)
            else:
                dx.addmm_(g2, wi)
        if dx is None:   # no projection received a gradient
            return None, None, None
        return dx.view(ctx.x_shape), None, None


# (QKV_FUSED = False: three nn.Linear calls and autograd's gradient sum)
QKV_FUSED = True


def qkv_projection(x, *ws):
    """(x W0ᵀ, x W1ᵀ, …) of bias-free projections with equal output widths on the HIP device in
    one GEMM (QKVProjection): q, k, v of a self-attention, or k, v of the shared context."""
    _lib.require_device(x)
    return QKVProjection.apply(x, _qkv_weight(*ws), int(ws[0].shape[0]))


class TokensProjIn(torch.autograd.Function):
    """Transformer2DModel.proj_in (1×1 conv) + NCHW→(B, HW, C') as ONE strided batched GEMM:
    h[b] = x[b]ᵀ Wᵀ + bias, x (B, C, HW) read through a transposed view (no permute copy, no
    NHWC conversion); the input gradient comes back in NCHW the same way (W frozen)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        B, C, HW = x.shape
        h = torch.bmm(x.transpose(1, 2), w.t().expand(B, C, w.shape[0]))
        if bias is not None:
            h.add_(bias)
        ctx.save_for_backward(w)
        return h

    @staticmethod
    def backward(ctx, dh):
        (w,) = ctx.saved_tensors
        B = dh.shape[0]
        dx = torch.bmm(w.t().expand(B, w.shape[1], w.shape[0]), dh.transpose(1, 2))   # (B, C, HW)
        return dx, None, None


class TokensProjOut(torch.autograd.Function):
    """Transformer2DModel.proj_out (1×1 conv) on (B, HW, C') tokens back to NCHW as one strided
    batched GEMM, y[b] = W h[b]ᵀ; the bias and the residual follow in one residual_bias_add."""

    @staticmethod
    def forward(ctx, h, w):
        B = h.shape[0]
        ctx.save_for_backward(w)
        return torch.bmm(w.expand(B, *w.shape), h.transpose(1, 2))                     # (B, C, HW)

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        B = dy.shape[0]
        return torch.bmm(dy.transpose(1, 2), w.expand(B, *w.shape)), None             # (B, HW, C')


def tokens_proj_in(x, weight, bias):
    """(B, C, H, W) → (B, HW, C') = 1×1 conv (weight (C', C, 1, 1)) + bias, flattened to tokens."""
    B, C = x.shape[:2]
    return TokensProjIn.apply(x.reshape(B, C, -1), weight.detach().reshape(weight.shape[0], C),
                              None if bias is None else bias.detach())


def tokens_proj_out(h, weight, bias, residual):
    """(B, HW, C') → residual + 1×1 conv(h) + bias in NCHW (residual's shape)."""
    B, C = residual.shape[:2]
    y = TokensProjOut.apply(h, weight.detach().reshape(C, h.shape[-1]))
    return residual_bias_add(residual, y.view(residual.shape), bias)


# --------------------------------------------------------------------------- 3×3 convolution
# Transformed weights per frozen weight tensor (U = G g Gᵀ; built once per form, on first use, on
# the weight's device and stream).
import weakref as _weakref

_WINO_U = {}   # id(weight) -> (weakref(weight), {(flip, form): (version, U)})
# Shapes whose grid stays below this even after splitting go to MIOpen.
WINO_MIN_WORKGROUPS = 128
# Which kernel takes an eligible shape: "auto" = skp_conv3x3_wino2 where H and W are multiples
# of 32 (every VAE-encoder layer, the UNet's 64² and 32² layers) or 16×16 with the batch a
# multiple of 4 (the UNet's 16² layers), skp_conv3x3_wino elsewhere (8²);
# "v1" forces the first kernel (tests).  WINO_SPLIT = False disables split-K; WINO_NSPLIT_FORCE
# (tests, tools/wino_time.py) measures one given split.
WINO_KERNEL = "auto"
WINO_SPLIT = True
WINO_NSPLIT_FORCE = 0


def _wino_v2(H, W, B=None):
    """skp_conv3x3_wino2 takes H, W multiples of 32, and 16×16 images four at a time."""
    if WINO_KERNEL == "v1":
        return False
    return (H % 32 == 0 and W % 32 == 0) or (H == 16 and W == 16 and B is not None and B % 4 == 0)


def _wino_u_cached(weight, flip, form, build):
    """The (flip, form) entry of ``weight``'s transformed weights, ``build()`` on first use and again
    after an in-place change of the weight (``_version``); the weight's entries leave with it."""
    key = id(weight)
    ent = _WINO_U.get(key)
    if ent is None or ent[0]() is not weight:
        ent = _WINO_U[key] = (_weakref.ref(weight, lambda _r: _WINO_U.pop(key, None)), {})
    hit = ent[1].get((flip, form))
    if hit is None or hit[0] != weight._version:
        hit = ent[1][(flip, form)] = (weight._version, build())
    return hit[1]


def _wino_u(weight, flip, v2=False):
    def build():
        w = _c(weight.detach())
        K, C = (w.shape[0], w.shape[1]) if not flip else (w.shape[1], w.shape[0])
        if v2 == "s2":   # the stride-2 form's 25 positions in rows of 28 (skp_wino2s2_weights; never flipped)
            U = torch.empty(K * C * 28, device=w.device, dtype=F32)
            call("skp_wino2s2_weights", ptr(w), K, C, ptr(U), stream(w.device))
        else:
            U = torch.empty(K * C * (40 if v2 else 36), device=w.device, dtype=F32)
            call("skp_wino2_weights" if v2 else "skp_wino_weights", ptr(w), K, C, int(flip), ptr(U), stream(w.device))
        return U
    return _wino_u_cached(weight, flip, v2, build)


def _batch_chunks(B, per_img_bytes):
    """(b0, b1) ranges of a batch whose inputs each stay below 2 GiB: the kernels address x through
    32-bit buffer offsets."""
    bmax = max(1, (2 ** 31 - 1) // per_img_bytes)
    for b0 in range(0, B, bmax):
        yield b0, min(B, b0 + bmax)


def _wino_plan_uncached(B, C, K, H, W, force):
    """(v2, nsplit, workgroups) for a (B, C, H, W) → (B, K, H, W) convolution.

    Splitting the input channels S ways shortens a workgroup S-fold and adds (S + 1) passes over the
    output for the partial sums; the split with the least modelled time wins (measured at batch 8:
    64² × 320 and 32² × 640 channels at 4 and 8 splits instead of 1.25 and 0.63 rounds).
    skp_conv3x3_wino2 (v2; the V-staged and stride-2 forms are planned as it): 2·wgs half-height
    workgroups, two co-resident per CU; a CU holding k of them runs ⌊k/2⌋ pairs at ≈1.72 µs per stage
    and a lone one at ≈1.48, the partial sums move at ≈2 TB/s (profiles/r03am_split_sweep.txt).
    skp_conv3x3_wino: one workgroup per CU (its LDS), ⌈workgroups / 256⌉ rounds of
    (stages × ≈2.4 µs + ≈5 µs); the partial sums move at ≈5 TB/s."""
    v2 = _wino_v2(H, W, B)
    if v2:
        wgs = (B // 4 if H == 16 else B * (H // 32) * (W // 32)) * (K // 32)
    elif B * (H // 4) * (W // 4) <= 32 and K % 64 == 0:
        wgs = K // 64   # one 32-tile × 64-channel block per channel block (libskp's rule, skp_conv.hip)
    else:
        wgs = -(-(B * (H // 4) * (W // 4)) // 64) * (K // 32)
    out_bytes = B * K * H * W * 4

    def cost(s):
        if v2:
            k = -(-2 * wgs * s // 256)
            st = C // s // 4
            return (k // 2) * st * 1.72e-6 + (k % 2) * st * 1.48e-6 + (s > 1) * (s + 1) * out_bytes / 2e12
        rounds = -(-wgs * s // 256)
        return rounds * ((C // s // 4) * 2.4e-6 + 5e-6) + (s > 1) * (s + 1) * out_bytes / 5e12

    nsplit = 1
    if WINO_SPLIT:
        cands = [s for s in range(1, 33) if C % (4 * s) == 0 and (s == 1 or C // s >= 32)]
        nsplit = min(cands, key=cost)
        if force and C % (4 * force) == 0:   # dev: WINO_NSPLIT_FORCE measures a given split
            nsplit = force
    return v2, nsplit, wgs * nsplit


_WINO_PLANS = {}


def _wino_plan(B, C, K, H, W):
    """_wino_plan_uncached, memoised per shape (and the module switches it reads): the planner's
    32-candidate cost loop ran in Python on every convolution call, ~1500 launches per step."""
    force = int(WINO_NSPLIT_FORCE)
    key = (B, C, K, H, W, force, WINO_KERNEL, WINO_SPLIT)
    plan = _WINO_PLANS.get(key)
    if plan is None:
        plan = _WINO_PLANS[key] = _wino_plan_uncached(B, C, K, H, W, force)
    return plan


def wino_eligible(B, C, K, H, W, min_workgroups=None):
    """Whether a Winograd kernel takes a (B, C, H, W) → (B, K, H, W) 3×3 convolution."""
    if C % 4 or K % 32 or H % 4 or W % 4:
        return False
    wgs = _wino_plan(B, C, K, H, W)[2]
    return wgs >= (WINO_MIN_WORKGROUPS if min_workgroups is None else min_workgroups)


# Small-image, many-channel convolutions (the UNet's 8²-32² layers) as Winograd transforms + 36
# batched library GEMMs (skp_wino_in_transform → torch.bmm → skp_wino_out_transform) instead of the
# fused kernels: at these sizes the fused grids are a few hundred latency-bound workgroups.
# WINO_GEMM_MAX_HW = the largest H·W that takes it (tests set 0 to cover the fused kernels).
WINO_GEMM_MAX_HW = 1024
WINO_GEMM_MIN_CH = 256
# G of F(4×4, 3×3) at the points (0, 1, −1, 1/2, −2, ∞) (skp_conv.hip's kG)
_WINO_G = ((1.0, 0.0, 0.0), (1 / 3, 1 / 3, 1 / 3), (-1 / 3, 1 / 3, -1 / 3), (-16 / 15, -8 / 15, -4 / 15),
           (1 / 15, -2 / 15, 4 / 15), (0.0, 0.0, 1.0))


def _wino_gemm_ok(B, C, K, H, W):
    return (0 < H * W <= WINO_GEMM_MAX_HW and C >= WINO_GEMM_MIN_CH and K >= WINO_GEMM_MIN_CH
            and H % 4 == 0 and W % 4 == 0 and B * (H // 4) * (W // 4) <= 65535)


def _wino_u_gemm(weight, flip):
    """U[p = 6i + j] (36, C, K) = (G g Gᵀ)[i][j] in fp64 → fp32, g = w[k][c] (flip 0) or
    rot180(w[c][k]) (flip 1, the input-gradient convolution); cached per frozen weight like
    _wino_u."""
    def build():
        w = weight.detach().double()
        g = w.flip(2, 3).transpose(0, 1) if flip else w                 # (K, C, 3, 3) of this convolution
        G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
        return torch.einsum("iu,kcuv,jv->ijck", G, g, G).reshape(36, g.shape[1], g.shape[0]).float().contiguous()
    return _wino_u_cached(weight, flip, "gemm", build)


# The product as (36, K, T), so the output transform reads it and writes the tiles coalesced (and
# leaves the next GroupNorm's statistics partials, as the fused kernel does); r04 measured it ahead
# of the (36, T, K) product with per-lane scattered tile stores (skp_wino_out_transform, kept in
# the ABI).
def _wino_gemm_conv(x, weight, flip, bias, residual, K, gn=False):
    B, C, H, W = x.shape
    T = B * (H // 4) * (W // 4)
    U = _wino_u_gemm(weight, flip)
    V = torch.empty(36, C, T, device=x.device, dtype=F32)
    call("skp_wino_in_transform", ptr(x), B, C, H, W, ptr(V), stream(x.device))
    y = torch.empty(B, K, H, W, device=x.device, dtype=F32)
    bp, rp = ptr(bias) if bias is not None else None, ptr(residual) if residual is not None else None
    M = torch.bmm(U.transpose(1, 2), V)                              # (36, K, T)
    P = (H // 4) * (W // 4)
    gnp = None
    if gn and GN_EPI and (P in (16, 32) or P % 64 == 0):
        nseg = P // min(P, 64)
        gnp = torch.empty(B, K, nseg, 2, device=x.device, dtype=F32)
    call("skp_wino_out_transform_kt", ptr(M), B, K, H, W, bp, rp, ptr(y), ptr(gnp), stream(x.device))
    if gnp is not None:
        y._skp_gn = (y._version, gnp, gnp.shape[2])
    return y


def _wino_conv(x, weight, flip, bias, residual, K, gn=False):
    """``gn``: also leave the output's GroupNorm statistics partials on it (``y._skp_gn``) where the
    kernel can write them (skp_conv3x3_wino2_gn: one split, H and W multiples of 32)."""
    B, C, H, W = x.shape
    if _wino_gemm_ok(B, C, K, H, W):
        return _wino_gemm_conv(x, weight, flip, bias, residual, K, gn)
    y = torch.empty(B, K, H, W, device=x.device, dtype=F32)
    chunks = list(_batch_chunks(B, C * H * W * 4))
    gnp = None
    if gn and GN_EPI and H % 32 == 0 and W % 32 == 0 and all(
            _wino_plan(b1 - b0, C, K, H, W)[:2] == (True, 1) for b0, b1 in chunks):
        nseg = (H // 16) * (W // 32)
        gnp = torch.empty(B, K, nseg, 2, device=x.device, dtype=F32)
    for b0, b1 in chunks:
        _wino_launch(x[b0:b1], weight, flip, bias, None if residual is None else residual[b0:b1], y[b0:b1], K,
                     None if gnp is None else gnp[b0:b1])
    if gnp is not None:
        y._skp_gn = (y._version, gnp, gnp.shape[2])
    return y


def _wino_launch(x, weight, flip, bias, residual, y, K, gnp=None):
    B, C, H, W = x.shape
    v2, nsplit, _ = _wino_plan(B, C, K, H, W)
    U = _wino_u(weight, flip, v2)
    ws = torch.empty(nsplit, B, K, H, W, device=x.device, dtype=F32) if nsplit > 1 else None
    name = "skp_conv3x3_wino2" if v2 else "skp_conv3x3_wino"
    args = (ptr(x), ptr(U), ptr(bias) if bias is not None else None,
            ptr(residual) if residual is not None else None, ptr(y), B, C, K, H, W, nsplit,
            ptr(ws) if ws is not None else None)
    with _timed(name, 0):
        if gnp is not None:
            call("skp_conv3x3_wino2_gn", *args, ptr(gnp), stream(x.device))
        else:
            call(name, *args, stream(x.device))


class Conv3x3(torch.autograd.Function):
    """y = conv2d(x, w, bias, padding=1) (+ residual) with a frozen 3×3 weight; the input
    gradient is the same Winograd kernel on the flipped weight (MIOpen when its shape is not
    eligible).  Gradients: x and residual only."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        x = _c(x)
        K = weight.shape[0]
        y = _wino_conv(x, weight, False, None if bias is None else _c(bias.detach()),
                       None if residual is None else _c(residual), K, gn=True)
        ctx.weight = weight
        ctx.xshape = x.shape
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        w = ctx.weight
        B, C, H, W = ctx.xshape
        K = w.shape[0]
        dx = None
        if ctx.needs_input_grad[0]:
            dy = _c(dy)
            if wino_eligible(B, K, C, H, W):
                dx = _wino_conv(dy, w, True, None, None, C)
            else:
                dx = torch.nn.grad.conv2d_input(ctx.xshape, w.detach(), dy, padding=1)
        return dx, None, None, (dy if ctx.has_res else None)


class Conv1x1(torch.autograd.Function):
    """y[b] = W x[b] for a frozen 1×1 convolution (K, C) on NCHW x viewed as (B, C, H·W): ONE strided
    batched GEMM with the weight broadcast over the batch (zero batch stride), straight between NCHW
    tensors — no NCHW↔NHWC transposes around a MIOpen 1×1 kernel; dx[b] = Wᵀ dy[b] the same way."""

    @staticmethod
    def forward(ctx, x, w):
        B, C, H, W = x.shape
        K = w.shape[0]
        y = torch.bmm(w.expand(B, K, C), x.reshape(B, C, H * W))
        ctx.save_for_backward(w)
        ctx.shape = (B, C, H, W)
        return y.view(B, K, H, W)

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        B, C, H, W = ctx.shape
        K = w.shape[0]
        dx = torch.bmm(w.t().expand(B, C, K), dy.reshape(B, K, H * W)) if ctx.needs_input_grad[0] else None
        return (None if dx is None else dx.view(B, C, H, W)), None


# A/B (default off): 1 = the resnets' 1×1 shortcuts as Conv1x1's batched GEMM.  Measured at the
# bench's shortcut shapes (tools/conv1x1_time.py, batch 8, fwd + input grad): within ±3% of MIOpen's
# 1×1 kernels at 8², 16² and 32² (2560→1280 @16²: 274 vs 272 us; 960→640 @32²: 186 vs 201 us;
# 1280→640 @32²: 290 vs 249 us), the VAE's 128→256 @256² 318 vs 343 us — no net gain, so MIOpen stays
CONV1X1_GEMM = False   # tests switch it: True = 1×1 shortcuts as one GEMM (measured neutral)


def conv1x1(x, weight):
    """Bias-free 1×1 convolution of NCHW fp32 x with a frozen weight (K, C, 1, 1) (the caller folds
    the bias into the next epilogue): Conv1x1's batched GEMM, or F.conv2d with CONV1X1_GEMM off."""
    _lib.require_device(x)
    if weight.requires_grad:
        raise ValueError("conv1x1: the weight must be frozen (requires_grad=False)")
    if not CONV1X1_GEMM or x.dtype != F32:
        return torch.nn.functional.conv2d(x, weight)
    return Conv1x1.apply(_c(x), weight.detach().reshape(weight.shape[0], weight.shape[1]))


# A/B: 0 = the VAE's stride-2 downsampling convolutions run as F.pad + MIOpen (r02)
WINO_S2 = True
WINO_S2_MIN_PIXELS = 128 * 128   # the smallest level measured (profiles/r09a_s2f2_kernels.txt)


def conv3x3_s2_eligible(x, weight):
    B, C, H, W = x.shape
    K = weight.shape[0]
    # measured at batch 8 (tools/conv_s2_time.py, three alternating repeats, ms; profiles/r09a_s2f2_kernels.txt):
    #                   skp_conv3x3s2_f2   sampled F(4×4, 3×3)   edge-pad copy + MIOpen
    #   512² × 128 ch   1.33-1.34          1.91-1.93             2.47-2.48
    #   256² × 256 ch   1.24-1.25          1.78-1.80             1.85
    #   128² × 512 ch   1.20-1.22          1.74-1.75             1.55-1.56
    # every repeat of the 25-product kernel is below every repeat of both alternatives at all three
    # VAE levels, so all of them take it (the sampled kernel it replaced is gone from the library)
    return (WINO_S2 and x.is_cuda and x.dtype == F32 and tuple(weight.shape[1:]) == (C, 3, 3) and C % 4 == 0
            and K % 32 == 0 and H % 32 == 0 and W % 32 == 0 and H * W >= WINO_S2_MIN_PIXELS
            and not weight.requires_grad and not (torch.is_grad_enabled() and x.requires_grad))


def conv3x3_s2(x, weight, bias=None):
    """diffusers' Downsample2D(padding=0) — F.pad(x, (0, 1, 0, 1)) then a 3×3 / stride-2 conv2d —
    forward only (the frozen VAE encoder runs without gradient): skp_conv3x3s2_f2, the stride-2
    minimal-product form (2×2 output tiles of 25 products on the stride-1 kernel's staged regions,
    whose out-of-range row / column is the zero pad past the bottom-right edge) with the bias in
    its epilogue.  (B, C, H, W) → (B, K, H/2, W/2)."""
    _lib.require_device(x)
    if not conv3x3_s2_eligible(x, weight):
        raise ValueError(f"conv3x3_s2: unsupported x {tuple(x.shape)} / weight {tuple(weight.shape)}")
    x = _c16(x)
    B, C, H, W = x.shape
    K = weight.shape[0]
    y = torch.empty(B, K, H // 2, W // 2, device=x.device, dtype=F32)
    U = _wino_u(weight, False, "s2")
    b = None if bias is None else _c(bias.detach())
    for b0, b1 in _batch_chunks(B, C * H * W * 4):
        _, nsplit, _ = _wino_plan(b1 - b0, C, K, H, W)
        ws = torch.empty(nsplit, b1 - b0, K, H // 2, W // 2, device=x.device, dtype=F32) if nsplit > 1 else None
        with _timed("skp_conv3x3s2_f2", 0):
            call("skp_conv3x3s2_f2", ptr(x[b0:b1]), ptr(U), ptr(b), ptr(y[b0:b1]), b1 - b0, C, K, H, W, nsplit,
                 ptr(ws), stream(x.device))
    return y


def conv3x3(x, weight, bias=None, residual=None):
    """3×3 / stride 1 / pad 1 convolution (+ bias, + residual) of NCHW fp32 ``x`` with a frozen
    ``weight`` (K, C, 3, 3): the Winograd F(4×4, 3×3) kernel when the shape is eligible, else
    MIOpen (F.conv2d) with the bias and residual added after."""
    _lib.require_device(x)
    if weight.requires_grad:
        raise ValueError("conv3x3: the weight must be frozen (requires_grad=False)")
    B, C, H, W = x.shape
    K = weight.shape[0]
    if tuple(weight.shape[1:]) != (C, 3, 3):
        raise ValueError(f"conv3x3: weight {tuple(weight.shape)} does not fit input {tuple(x.shape)}")
    if residual is not None and tuple(residual.shape) != (B, K, H, W):
        raise ValueError(f"conv3x3: residual {tuple(residual.shape)} is not ({B}, {K}, {H}, {W})")
    if C % 4 and C < 16 and x.dtype == F32 and wino_eligible(B, C + 4 - C % 4, K, H, W):
        # input layers (RGB: 3 channels): one zero channel makes them Winograd-eligible; the
        # padded weight's transform is rebuilt per call (K·4 entries)
        pad = 4 - C % 4
        xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, pad))
        wp = torch.nn.functional.pad(weight.detach(), (0, 0, 0, 0, 0, pad))
        return Conv3x3.apply(xp, wp, bias, residual)
    if x.dtype != F32 or not wino_eligible(B, C, K, H, W):
        y = torch.nn.functional.conv2d(x, weight, bias, 1, 1)
        return y if residual is None else residual + y
    return Conv3x3.apply(x, weight, bias, residual)


# --------------------------------------------------------------------------- GroupNorm → 3×3 conv, V-staged
# The gradient-free GroupNorm(+SiLU) → 3×3 convolution pairs of the frozen VAE encoder as
# skp_groupnorm_stats → skp_wino2_vtransform_gn → skp_conv3x3_wino2_v: the normalised activation is
# never stored and every input tile is transformed once instead of K/32 times.  Per-shape choice,
# measured (tools/wino_time.py --pair, batch 8, each side in a process of its own): a
# (C, K, H, W) is listed only where the new pair beat gn_apply + wino2 by more than the spread
# of its own repeats.  Tests add entries to force the path.
#   (C, K, H, W)          old pair µs  new pair µs   (profiles/r08a_vst_pair_ab.txt, medians of 3)
#   512→512 @ 64²            592.1        505.6  +14.6%
#   256→512 @ 128²          1203.4       1034.8  +14.0%
#   512→512 @ 128²          2165.3       1767.0  +18.4%
#   128→256 @ 256²          1376.3       1239.1  +10.0%
#   256→256 @ 256²          2319.7       2062.9  +11.1%
#   128→128 @ 512²          2716.3       2615.1   +3.7%   not listed: the pair wins in isolation, but in the bench
#       step its 2.4 GB of V cost the layers after it more than that (88.898 ms per step without the entry,
#       89.014 with it, every repeat; profiles/r08a_vst_pair_ab.txt)
WINO_V_SHAPES = {(512, 512, 64, 64), (256, 512, 128, 128), (512, 512, 128, 128), (128, 256, 256, 256),
                 (256, 256, 256, 256)}
WINO_V_MIN_BATCH = 4   # the table was measured at batch 8: grids of at least half that size


def gn_conv3x3_wins(B, C, K, H, W):
    """Whether the planner routes act(GroupNorm(x)) → conv3x3 of this shape to the V-staged pair."""
    return ((C, K, H, W) in WINO_V_SHAPES and B >= WINO_V_MIN_BATCH and C % 4 == 0 and K % 32 == 0
            and H % 32 == 0 and W % 32 == 0 and WINO_KERNEL == "auto" and not _wino_gemm_ok(B, C, K, H, W))


def gn_conv3x3(x, gamma, beta, groups, eps, act, shift, weight, bias=None, residual=None):
    """conv3x3(act(GroupNorm(x + shift)), weight, bias, residual) without gradient, through the
    V-staged Winograd pair.  Shapes the kernels do not take are an error (the caller asks
    gn_conv3x3_wins first); the output carries its GroupNorm statistics partials like conv3x3's."""
    _lib.require_device(x)
    if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)):
        raise ValueError("gn_conv3x3: forward only (no gradient reaches the normalised activation)")
    if weight.requires_grad or gamma.requires_grad or beta.requires_grad:
        raise ValueError("gn_conv3x3: the parameters must be frozen")
    pre = _gn_parts_of(x) if GN_EPI else None   # the producing convolution's partials ride on x itself
    x = _c16(x.detach())
    B, C, H, W = x.shape
    K = weight.shape[0]
    if tuple(weight.shape[1:]) != (C, 3, 3):
        raise ValueError(f"gn_conv3x3: weight {tuple(weight.shape)} does not fit input {tuple(x.shape)}")
    if residual is not None:
        if tuple(residual.shape) != (B, K, H, W):
            raise ValueError(f"gn_conv3x3: residual {tuple(residual.shape)} is not ({B}, {K}, {H}, {W})")
        residual = _c16(residual.detach())
    if shift is not None:
        shift = _c(shift.detach().reshape(-1, C).to(x.device, F32).expand(B, C))
    dev = x.device
    nws = _lib.lib().skp_groupnorm_workspace(B, C, H * W, int(groups))
    if nws < 0:
        raise ValueError(f"gn_conv3x3: bad shape {tuple(x.shape)} groups={groups}")
    part = torch.empty(nws, device=dev, dtype=torch.float64)
    stats = torch.empty(B * groups * 2, device=dev, dtype=F32)
    g, b = _c(gamma.detach()), _c(beta.detach())
    if pre is not None:
        call("skp_groupnorm_stats_part", ptr(pre[0]), pre[1], ptr(shift), B, C, H * W, int(groups), float(eps),
             ptr(stats), ptr(part), stream(dev))
    else:
        call("skp_groupnorm_stats", ptr(x), ptr(shift), B, C, H * W, int(groups), float(eps), ptr(stats), ptr(part),
             stream(dev))
    V = torch.empty(B * C * (H // 4) * (W // 4) * 36, device=dev, dtype=F32)
    with _timed("skp_wino2_vtransform_gn", 0):
        call("skp_wino2_vtransform_gn", ptr(x), ptr(stats), ptr(g), ptr(b), ptr(shift), int(groups), int(bool(act)),
             ptr(V), B, C, H, W, stream(dev))
    _, nsplit, _ = _wino_plan(B, C, K, H, W)
    U = _wino_u(weight, False, True)
    y = torch.empty(B, K, H, W, device=dev, dtype=F32)
    ws = torch.empty(nsplit, B, K, H, W, device=dev, dtype=F32) if nsplit > 1 else None
    gnp = torch.empty(B, K, (H // 16) * (W // 32), 2, device=dev, dtype=F32) if GN_EPI and nsplit == 1 else None
    bias = None if bias is None else _c(bias.detach())
    with _timed("skp_conv3x3_wino2_v", 0):
        call("skp_conv3x3_wino2_v_gn", ptr(V), ptr(U), ptr(bias), ptr(residual), ptr(y), B, C, K, H, W, nsplit,
             ptr(ws), ptr(gnp), stream(dev))
    if gnp is not None:
        y._skp_gn = (y._version, gnp, gnp.shape[2])
    return y


# --------------------------------------------------------------------------- A17 visualisation sheets
TAB10 = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75),
         (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207))
# viridis at 0, 32, …, 224, 255 of 256 (the fallback table joins them linearly)
_VIRIDIS_ANCHORS = ((0, (0.267004, 0.004874, 0.329415)), (32, (0.278826, 0.175490, 0.483397)),
                    (64, (0.229739, 0.322361, 0.545706)), (96, (0.172719, 0.448791, 0.557885)),
                    (128, (0.127568, 0.566949, 0.550556)), (160, (0.157851, 0.683765, 0.501686)),
                    (192, (0.369214, 0.788888, 0.382914)), (224, (0.678489, 0.863742, 0.189503)),
                    (255, (0.993248, 0.906157, 0.143936)))
_LUT_CACHE = {}


def default_colors(K):
    """(K, 3) uint8 marker colours: the ten "tab10" colours for K <= 10, else K evenly spaced hues."""
    if K <= 10:
        rows = TAB10[:K]
    else:
        import colorsys
        rows = [tuple(int(round(255 * c)) for c in colorsys.hsv_to_rgb(j / K, 0.9, 1.0)) for j in range(K)]
    return torch.tensor(rows, dtype=torch.uint8).reshape(K, 3)


def fallback_lut():
    """(256, 3) fp32 in [0, 1]: piecewise-linear through nine viridis anchor colours."""
    lut = torch.empty(256, 3, dtype=F32)
    for (i0, c0), (i1, c1) in zip(_VIRIDIS_ANCHORS[:-1], _VIRIDIS_ANCHORS[1:]):
        t = torch.arange(i0, i1 + 1, dtype=torch.float64).sub(i0).div(i1 - i0)[:, None]
        lut[i0:i1 + 1] = (torch.tensor(c0, dtype=torch.float64) * (1 - t) + torch.tensor(c1, dtype=torch.float64) * t).float()
    return lut.clamp_(0.0, 1.0)


def default_lut():
    """matplotlib's viridis sampled at 256 points when matplotlib imports, else ``fallback_lut``."""
    try:
        import matplotlib
        import numpy as np
        cm = matplotlib.colormaps["viridis"]
        return torch.tensor(np.asarray(cm(np.linspace(0.0, 1.0, 256)))[:, :3], dtype=F32).contiguous()
    except ImportError:
        return fallback_lut()


def map_range(maps):
    """(n, h, w) -> (n, 2) per-map (min, max); (NaN, NaN) = "no overlay" for a map that holds a
    non-finite value or is constant (skp_map_range)."""
    _lib.require_device(maps)
    maps = _c(maps)
    n, h, w = maps.shape
    out = torch.empty(n, 2, device=maps.device, dtype=F32)
    call("skp_map_range", ptr(maps), n, h, w, ptr(out), stream(maps.device))
    return out


def sheet_shape(H, W, rows, cols, downscale=1, pad=2):
    """(Hs, Ws) of a rows × cols sheet of (H, W) images."""
    return rows * (H // downscale + pad) + pad, cols * (W // downscale + pad) + pad


def render_sheet(images, maps=None, points=None, *, rows, cols, downscale=1, pad=2, alpha=0.7, radius=None,
                 colors=None, lut=None, overlay=None):
    """One (Hs, Ws, 3) uint8 sheet of rows × cols tiles (skp_render_sheet; visualize.py:40-73, 105-138).

    ``images`` (n, 3, H, W) in [0, 1]; ``maps`` (n, h, w) heat overlay at ``alpha`` through
    ``lut`` ((256, 3) in [0, 1], default viridis); ``points`` (n, K, 2) normalised (row, col)
    markers of ``radius`` output pixels (default max(2, th/32)) in ``colors`` ((K, 3) uint8,
    default ``default_colors``); ``overlay`` (n,) bool, False = that tile shows the plain image.
    """
    _lib.require_device(images, maps, points)
    images = _c(images)
    n, C, H, W = images.shape
    if C != 3:
        raise ValueError(f"render_sheet: images must be (n, 3, H, W), got {tuple(images.shape)}")
    dev = images.device
    f = int(downscale)
    h = w = 0
    rng = None
    if maps is not None:
        maps = _c(maps)
        if maps.dim() != 3 or maps.shape[0] != n:
            raise ValueError(f"render_sheet: maps must be ({n}, h, w), got {tuple(maps.shape)}")
        h, w = maps.shape[1:]
        rng = map_range(maps)
        if overlay is not None:
            keep = torch.as_tensor(overlay, dtype=torch.bool).to(dev)
            if keep.shape != (n,):
                raise ValueError(f"render_sheet: overlay must be ({n},), got {tuple(keep.shape)}")
            rng[~keep] = float("nan")
        if lut is None:
            if dev not in _LUT_CACHE:
                _LUT_CACHE[dev] = default_lut().to(dev)
            lut = _LUT_CACHE[dev]
        lut = _c(lut.to(dev))
        if tuple(lut.shape) != (256, 3):
            raise ValueError(f"render_sheet: lut must be (256, 3), got {tuple(lut.shape)}")
    K = 0
    if points is not None:
        points = _c(points)
        if points.dim() != 3 or points.shape[0] != n or points.shape[2] != 2:
            raise ValueError(f"render_sheet: points must be ({n}, K, 2), got {tuple(points.shape)}")
        K = points.shape[1]
    if K:
        colors = default_colors(K) if colors is None else torch.as_tensor(colors)
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (K, 3):
            raise ValueError(f"render_sheet: colors must be ({K}, 3) uint8")
        colors = colors.to(dev).contiguous()
        if radius is None:
            radius = max(2.0, (H // max(f, 1)) / 32.0)
    else:
        points = colors = None
    Hs, Ws = sheet_shape(H, W, rows, cols, max(f, 1), pad)
    out = torch.empty(Hs, Ws, 3, device=dev, dtype=torch.uint8)
    call("skp_render_sheet", ptr(images), n, H, W, ptr(maps), h, w, ptr(rng), ptr(lut) if maps is not None else None,
         float(alpha), ptr(points), K, float(radius or 0.0), ptr(colors), int(rows), int(cols), f, int(pad), ptr(out),
         stream(dev))
    return out


# --------------------------------------------------------------------------- A18 TTA reduce
_TTA_WS = {}   # (query name, device, query arguments) -> workspace of that query's bytes


def _tta_inputs(op, maps, theta_inv):
    """The checks every TTA reduce makes of its inputs -> (maps, theta_inv, B, C, n, S, device), both
    tensors contiguous on ``maps``' device."""
    _lib.require_device(maps, theta_inv)
    if maps.dim() != 5 or maps.shape[-1] != maps.shape[-2]:
        raise ValueError(f"{op}: maps must be (B, C, n, S, S), got {tuple(maps.shape)}")
    maps = _c(maps)
    B, C, n, S, _ = maps.shape
    if tuple(theta_inv.shape) != (B, C, 2, 3):
        raise ValueError(f"{op}: theta_inv must be ({B}, {C}, 2, 3), got {tuple(theta_inv.shape)}")
    dev = maps.device
    return maps, _c(theta_inv.to(dev)), B, C, n, S, dev


# the first of a workspace query's further arguments, as the "bad shape" message names it
_TTA_WS_ARG = {"tta_reduce_peaks": "num", "tta_reduce_match": "Q"}


def _tta_workspace(op, dev, B, n, S, *args):
    """The cached workspace of ``skp_<op>``, sized by ``skp_<op>_workspace(B, n, S, *args)``.  ``args``
    are that query's further arguments in its order.  The size depends on the first of them alone
    (``num`` of the k-peak query, not its ``radius2``; ``Q`` of the match query), so that one is part
    of the cache's key."""
    first = args[0] if args else None
    key = (op, dev, B, n, S, first)
    ws = _TTA_WS.get(key)
    if ws is None:
        nbytes = getattr(_lib.lib(), f"skp_{op}_workspace")(B, n, S, *args)
        if nbytes <= 0:
            raise ValueError(f"{op}: bad shape B={B}, n={n}, S={S}" + (f", {_TTA_WS_ARG[op]}={first}" if args else ""))
        ws = _TTA_WS[key] = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.int64)
    return ws


def _tta_call(op, maps, theta_inv, return_avg, query):
    """What the TTA reduces share around their one ``skp_<op>`` call.  After ``_tta_inputs``,
    ``query(B, C, n, S)`` checks the query's own arguments and returns ``(scalars, pos_shape, extras,
    nbytes, ws_args)``: the arguments that ``skp_<op>`` takes after ``theta_inv`` (scalars, or
    device tensors passed as pointers), the shape of ``pos``, a ``(shape, dtype)`` per further output
    in the entry point's order (None for an optional output that is not asked for: a null pointer,
    and None in the result), the byte model's value and the workspace query's further arguments.
    Returns ``(pos, *extras, avg)``: ``avg`` (B, n, S, S) when ``return_avg``, else None."""
    maps, th, B, C, n, S, dev = _tta_inputs(op, maps, theta_inv)
    scalars, pos_shape, extras, nbytes, ws_args = query(B, C, n, S)
    ws = _tta_workspace(op, dev, B, n, S, *ws_args)
    outs = [None if e is None else torch.empty(*e[0], device=dev, dtype=e[1]) for e in [(pos_shape, F32), *extras]]
    avg = torch.empty(B, n, S, S, device=dev, dtype=F32) if return_avg else None
    own = [ptr(a) if torch.is_tensor(a) else a for a in scalars]   # `scalars` keeps its tensors alive
    with _timed(f"skp_{op}", nbytes):
        call(f"skp_{op}", ptr(maps), B, C, n, S, ptr(th), *own, *map(ptr, outs), ptr(avg), ptr(ws), stream(dev))
    return (*outs, avg)


def tta_reduce_bytes(B, C, n, S, avg=False):
    """Byte model of skp_tta_reduce: every captured map read once, the average written on request."""
    return 4 * B * C * n * S * S + (4 * B * n * S * S if avg else 0)


def tta_reduce(maps, theta_inv, return_avg=False):
    """The TTA reduce of B images in one call (skp_tta_reduce; eval.py:327-355 then :39-60).

    ``maps`` (B, C, n, S, S): n token maps of C warped copies per image; ``theta_inv`` (B, C, 2, 3)
    each copy's inverse theta.  Returns ``(pos, avg)``: ``pos`` (B, n, 2) = (row + 0.5, col + 0.5)
    of the first-occurrence argmax of Σ_c warp(maps) / Σ_c warp(ones) with NaN → 0, and that
    average (B, n, S, S) when ``return_avg``, else None.  Bit-identical to ``affine_warp`` per
    copy, sums in copy order, the division, the NaN fix and ``find_max_pixel``.
    """
    def query(B, C, n, S):
        return (), (B, n, 2), [], tta_reduce_bytes(B, C, n, S, return_avg), ()

    return _tta_call("tta_reduce", maps, theta_inv, return_avg, query)


def tta_reduce_scored_bytes(B, C, n, S, distance=5, avg=False):
    """Byte model of skp_tta_reduce_scored: ``tta_reduce_bytes`` plus the window kernel's re-reads,
    two 8-byte pairs per copy for each of the at most (2⌊distance⌋ + 1)² pixels around a peak."""
    side = 2 * int(distance) + 1
    return tta_reduce_bytes(B, C, n, S, avg) + 16 * B * n * C * side * side


def tta_reduce_scored(maps, theta_inv, distance=5, return_avg=False):
    """``tta_reduce`` with confidence scores and a sub-pixel position (skp_tta_reduce_scored).

    Returns ``(pos, refined, scores, avg)``: ``pos`` and ``avg`` are ``tta_reduce``'s, bit for bit;
    ``refined`` (B, n, 2) is the ``pixel_from_weighted_avg`` centroid of the average's pixels
    within ``distance`` of its peak; ``scores`` (B, n, 3) holds per token the peak value
    (``[..., 0]``), the concentration (``[..., 1]``: the average's mass within ``distance`` of
    the peak over its whole mass) and the coverage (``[..., 2]``: the share of the C copies that
    saw the peak pixel).  The average is not written unless ``return_avg``.  ``0 < distance <= 16``.
    """
    def query(B, C, n, S):
        d = float(distance)
        if not 0.0 < d <= 16.0:
            raise ValueError(f"tta_reduce_scored: distance must be in (0, 16], got {d}")
        refined_scores = [((B, n, 2), F32), ((B, n, 3), F32)]
        return (d,), (B, n, 2), refined_scores, tta_reduce_scored_bytes(B, C, n, S, d, return_avg), ()

    return _tta_call("tta_reduce_scored", maps, theta_inv, return_avg, query)


def tta_reduce_peaks_bytes(B, C, n, S, num, radius=None, avg=False):
    """Byte model of skp_tta_reduce_peaks: ``tta_reduce_bytes`` plus, for each round after the
    first, the masked-tile kernel's re-reads: two 8-byte pairs per copy for each pixel of the
    64 × 4 tiles that the (2(⌊radius⌋ + 1) + 1)² box around a pick can meet."""
    R = int(0.05 * S if radius is None else radius) + 1
    span = lambda tile: (2 * R + 2 * tile - 1) // tile
    tiles = min(span(4), (S + 3) // 4) * min(span(64), (S + 63) // 64)
    return tta_reduce_bytes(B, C, n, S, avg) + 16 * B * n * C * (num - 1) * tiles * 256


def tta_reduce_peaks(maps, theta_inv, num, radius=None, return_avg=False):
    """``tta_reduce`` with ``num`` peaks per token (skp_tta_reduce_peaks; eval.py:327-355 then :62-111).

    Returns ``(pos, values, avg)``: ``pos`` (B, n, num, 2) holds round j's (row + 0.5, col + 0.5),
    ``values`` (B, n, num) the value that won round j (read after j masks), ``avg`` the unmasked
    average (B, n, S, S) when ``return_avg``, else None.  Bit-identical to ``tta_reduce(...,
    return_avg=True)`` followed by ``find_k_max_pixels`` of the average: round 0 is ``tta_reduce``'s
    ``pos``, and before round j each earlier pick has multiplied the map by 0 within ``radius`` of
    itself (``mask_radius``: a masked pixel is 0 and can still win, +inf · 0 is NaN and NaN wins).
    ``radius=None`` is the reference's 0.05 · S.  ``1 <= num <= 16``.  The average is not in memory
    unless ``return_avg``.
    """
    def query(B, C, n, S):
        k = int(num)
        if not 1 <= k <= 16:
            raise ValueError(f"tta_reduce_peaks: num must be in [1, 16], got {k}")
        radius2 = _radius2(S) if radius is None else float(radius) ** 2
        if not 0.0 < radius2 < float("inf"):
            raise ValueError(f"tta_reduce_peaks: radius must be positive and finite, got {radius}")
        nbytes = tta_reduce_peaks_bytes(B, C, n, S, k, radius, return_avg)
        return (k, radius2), (B, n, k, 2), [((B, n, k), F32)], nbytes, (k, radius2)

    return _tta_call("tta_reduce_peaks", maps, theta_inv, return_avg, query)


def tta_reduce_entropy_bytes(B, C, n, S, avg=False):
    """Byte model of skp_tta_reduce_entropy: ``tta_reduce_bytes`` plus the entropy partials, two
    doubles per image, token and 64 × 4-pixel tile, written once and read once."""
    tiles = ((S + 63) // 64) * ((S + 3) // 4)
    return tta_reduce_bytes(B, C, n, S, avg) + 32 * B * n * tiles


def tta_reduce_entropy(maps, theta_inv, scale=1.0, return_avg=False):
    """``tta_reduce`` with the softmax entropy of every averaged plane (skp_tta_reduce_entropy;
    eval.py:327-355, then the key of eval.find_corresponding_points, eval.py:159-195).

    Returns ``(pos, entropy, avg)``: ``pos`` and ``avg`` are ``tta_reduce``'s, bit for bit;
    ``entropy`` (B, n) float64 is the Shannon entropy of ``softmax(scale · a)`` over the S² pixels
    of each average ``a``, reduced in one pass (log S0 − T / S0 about the maximum, in double, fixed
    orders).  A plane whose maximum is +inf gives NaN.  The average is not in memory unless
    ``return_avg``.  ``scale`` must be positive and finite.
    """
    def query(B, C, n, S):
        s = float(scale)
        if not 0.0 < s < float("inf"):
            raise ValueError(f"tta_reduce_entropy: scale must be positive and finite, got {s}")
        return (s,), (B, n, 2), [((B, n), torch.float64)], tta_reduce_entropy_bytes(B, C, n, S, return_avg), ()

    return _tta_call("tta_reduce_entropy", maps, theta_inv, return_avg, query)


def tta_reduce_parts_bytes(B, C, n, S, avg=False):
    """Byte model of skp_tta_reduce_parts: ``tta_reduce_bytes`` plus 10 bytes per image and pixel
    (a float value, an int16 label, a float mass) and, with more than one chunk of 10 tokens, the
    same 10 bytes per image, chunk and pixel written once and read once (an upper bound: the merge
    reads the label of the winning chunk only)."""
    chunks = (n + 9) // 10
    return tta_reduce_bytes(B, C, n, S, avg) + 10 * B * S * S + (20 * B * chunks * S * S if chunks > 1 else 0)


def tta_reduce_parts(maps, theta_inv, return_avg=False):
    """``tta_reduce`` with the per-pixel reduction over the tokens (skp_tta_reduce_parts).

    Returns ``(pos, label, value, mass, avg)``: ``pos`` and ``avg`` are ``tta_reduce``'s, bit for
    bit; at every pixel of every image ``value`` (B, S, S) is the greatest of the n averages,
    ``label`` (B, S, S) int16 the lowest token that attains it, and ``mass`` (B, S, S) the tokens'
    sum in a fixed order (chunks of 10 tokens: each chunk's sum from 0 in token order, the chunks'
    sums from 0 in chunk order; the plain sequential sum for n <= 10).  A pixel that no copy
    covers has label 0, value 0 and mass 0.  The average is not in memory unless ``return_avg``.
    ``n <= 32767``.
    """
    def query(B, C, n, S):
        if n > 32767:
            raise ValueError(f"tta_reduce_parts: at most 32767 tokens (the label is int16), got {n}")
        label_value_mass = [((B, S, S), torch.int16), ((B, S, S), F32), ((B, S, S), F32)]
        return (), (B, n, 2), label_value_mass, tta_reduce_parts_bytes(B, C, n, S, return_avg), ()

    return _tta_call("tta_reduce_parts", maps, theta_inv, return_avg, query)


def tta_reduce_match_bytes(B, C, n, S, Q, scores=False, avg=False):
    """Byte model of skp_tta_reduce_match: ``tta_reduce_bytes`` plus the queries (4·Q·n), the matches
    (12 bytes per image and query: a position and a score), with more than one chunk of 10 tokens the
    Q + 1 floats per image, chunk and pixel written once and read once, and the score map where it is
    asked for."""
    chunks = (n + 9) // 10
    return (tta_reduce_bytes(B, C, n, S, avg) + 4 * Q * n + 12 * B * Q
            + (2 * 4 * (Q + 1) * B * chunks * S * S if chunks > 1 else 0) + (4 * B * Q * S * S if scores else 0))


def tta_reduce_match(maps, theta_inv, queries, return_scores=False, return_avg=False):
    """``tta_reduce`` with query signatures matched against every pixel (skp_tta_reduce_match).

    At a pixel the n tokens' averages are a signature of what is there; ``queries`` (Q, n) float32 on
    the maps' device holds Q of them, ``1 <= Q <= 16``.  Returns ``(pos, match_pos, match_score,
    score_map, avg)``: ``pos`` and ``avg`` are ``tta_reduce``'s, bit for bit; ``match_pos`` (B, Q, 2)
    is (row + 0.5, col + 0.5) of the first row-major maximum over the pixels of the cosine score
    dot / sqrt(nrm), ``match_score`` (B, Q) that maximum, and ``score_map`` (B, Q, S, S) every score
    when ``return_scores``, else None.  nrm = Σ_t a² and dot = Σ_t a·d in a fixed order (chunks of 10
    tokens: each chunk's sums from 0 in token order, the chunks' sums from 0 in chunk order, no fma;
    the plain sequential sums for n <= 10).  A score is −inf where nrm is not > 0 (a pixel that no copy
    covers) or the quotient is NaN, never NaN; an image whose scores are all −inf gives (0.5, 0.5) and
    −inf.  Neither the average nor the scores are in memory unless asked for.
    """
    _lib.require_device(queries)

    def query(B, C, n, S):
        if queries.dim() != 2 or queries.shape[1] != n or queries.dtype != F32:
            raise ValueError(f"tta_reduce_match: queries must be (Q, {n}) float32, got {tuple(queries.shape)} "
                             f"{queries.dtype}")
        Q = queries.shape[0]
        if not 1 <= Q <= 16:
            raise ValueError(f"tta_reduce_match: Q must be in [1, 16], got {Q}")
        if queries.device != maps.device:
            raise ValueError(f"tta_reduce_match: queries on {queries.device}, maps on {maps.device}")
        outs = [((B, Q, 2), F32), ((B, Q), F32), ((B, Q, S, S), F32) if return_scores else None]
        nbytes = tta_reduce_match_bytes(B, C, n, S, Q, return_scores, return_avg)
        return (_c(queries), Q), (B, n, 2), outs, nbytes, (Q,)

    return _tta_call("tta_reduce_match", maps, theta_inv, return_avg, query)


# --------------------------------------------------------------------------- A19 dense match field
def match_field_flops(B, n, P, Q):
    """Flop model of skp_match_field: the (P, Q) products over n tokens of B images."""
    return 2 * B * n * P * Q


def match_field_bytes(B, n, P, Q, bx=None, by=None):
    """Byte model of skp_match_field: what must cross the memory interface once — each distinct
    operand read for its norms and once more for the products (``bx``, ``by`` operands: 1 where one
    is shared, default B) and the index and score written.  The panels' re-reads by other workgroups
    are cache traffic, and the (P, Q) product is never in memory."""
    bx, by = B if bx is None else bx, B if by is None else by
    return 2 * 4 * n * (bx * P + by * Q) + 8 * B * P


def match_field(x, y):
    """The dense nearest-pixel field (skp_match_field): for every column p of ``x`` the column q of
    ``y`` with the greatest cosine, on the exact-f32 matrix cores; the (P, Q) product is never in memory.

    ``x`` (B or 1, n, P) and ``y`` (B or 1, n, Q): float32, contiguous, on one device; a leading 1
    beside a B is one operand shared by the B images.  A (B, n, S, S) TTA average is such an operand
    as ``avg.view(B, n, S * S)``.  Returns ``(index (B, P) int32, score (B, P) float32)``: the lowest
    usable q with the greatest key dot · (1 / |y_q|) and that key times 1 / |x_p|; −1 and −inf where
    the column p is not usable (zero, or holding a NaN or an infinity) or no q is.  Norms and dots
    are fmaf chains in token order (include/skp.h), so the result is defined bit for bit.
    """
    _lib.require_device(x, y)
    for name, t in (("x", x), ("y", y)):
        if t.dim() != 3:
            raise ValueError(f"match_field: {name} must be (B or 1, n, pixels), got {tuple(t.shape)}")
        if t.dtype != F32:
            raise ValueError(f"match_field: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"match_field: {name} must be contiguous, got strides {t.stride()}")
    if y.device != x.device:
        raise ValueError(f"match_field: y on {y.device}, x on {x.device}")
    (bx, n, P), (by, ny, Q) = x.shape, y.shape
    if ny != n:
        raise ValueError(f"match_field: y has {ny} tokens, x has {n}")
    B = max(bx, by)
    if bx not in (1, B):
        raise ValueError(f"match_field: x has {bx} images, y has {by}")
    if by not in (1, B):
        raise ValueError(f"match_field: y has {by} images, x has {bx}")
    dev = x.device
    key = ("match_field", dev, B, n, P, Q)
    ws = _TTA_WS.get(key)
    if ws is None:
        nbytes = _lib.lib().skp_match_field_workspace(B, n, P, Q)
        if nbytes <= 0:
            raise ValueError(f"match_field: bad shape B={B}, n={n}, P={P}, Q={Q}")
        ws = _TTA_WS[key] = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.int64)
    index = torch.empty(B, P, device=dev, dtype=torch.int32)
    score = torch.empty(B, P, device=dev, dtype=F32)
    with _timed("skp_match_field", match_field_bytes(B, n, P, Q, bx, by), match_field_flops(B, n, P, Q)):
        call("skp_match_field", ptr(x), n * P if bx == B and B > 1 else 0, P, ptr(y), n * Q if by == B and B > 1 else 0,
             Q, B, n, ptr(index), ptr(score), ptr(ws), stream(dev))
    return index, score


def match_refine_flops(B, n, S, f, w):
    """Flop model of skp_match_refine: the dots of the definition, 2·n·Σ_p |W(p)| over the B images,
    taken at its bound 2·B·n·S²·(2w + 1)² (windows clipped at the borders hold fewer pixels; the dots
    that a cell's workgroup forms outside a pixel's window are not counted)."""
    return 2 * B * n * S * S * (2 * w + 1) ** 2


def match_refine_bytes(B, n, S, f, w, bx=None, by=None):
    """Byte model of skp_match_refine: each distinct operand once (``bx``, ``by`` operands: 1 where one
    is shared, default B) plus ``coarse``, ``index`` and ``score``.  The regions' re-reads by
    neighbouring cells are cache traffic."""
    bx, by = B if bx is None else bx, B if by is None else by
    return 4 * n * S * S * (bx + by) + 4 * B * (S // f) ** 2 + 8 * B * S * S


def match_refine(x, y, coarse, radius):
    """The windowed refine of a coarse field (skp_match_refine): for every pixel p of ``x`` the pixel q
    of ``y`` with the greatest cosine inside a (2·radius + 1)² window whose centre ``coarse`` gives.

    ``x`` and ``y`` (B or 1, n, S, S): float32, contiguous, on one device; a leading 1 beside a B is one
    operand shared by the B images.  ``coarse`` (B, Sc, Sc) int32 with Sc dividing S and f = S / Sc in
    [1, 8]: per f × f cell of x's grid a cell of y's grid (row · Sc + col); the window of pixel (r, c)
    is centred on ((m / Sc)·f + r % f, (m % Sc)·f + c % f) and clipped to the plane.  ``radius`` in
    [1, 16].  Returns ``(index (B, S, S) int32, score (B, S, S) float32)`` with ``match_field``'s keys
    bit for bit: the lowest usable q of the window with the greatest key and that key times 1 / |x_p|;
    −1 and −inf where p is not usable, where its cell's prior is outside [0, Sc²) or where no q of the
    window is usable (include/skp.h).
    """
    _lib.require_device(x, y, coarse)
    for name, t in (("x", x), ("y", y)):
        if t.dim() != 4 or t.shape[-1] != t.shape[-2]:
            raise ValueError(f"match_refine: {name} must be (B or 1, n, S, S), got {tuple(t.shape)}")
        if t.dtype != F32:
            raise ValueError(f"match_refine: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"match_refine: {name} must be contiguous, got strides {t.stride()}")
    if y.device != x.device or coarse.device != x.device:
        raise ValueError(f"match_refine: y on {y.device}, coarse on {coarse.device}, x on {x.device}")
    (bx, n, S, _), (by, ny, Sy, _) = x.shape, y.shape
    if ny != n or Sy != S:
        raise ValueError(f"match_refine: y is {ny} tokens of {Sy} x {Sy}, x is {n} tokens of {S} x {S}")
    if coarse.dim() != 3 or coarse.shape[-1] != coarse.shape[-2] or coarse.dtype != torch.int32:
        raise ValueError(f"match_refine: coarse must be (B, Sc, Sc) int32, got {tuple(coarse.shape)} {coarse.dtype}")
    if not coarse.is_contiguous():
        raise ValueError(f"match_refine: coarse must be contiguous, got strides {coarse.stride()}")
    B, Sc = coarse.shape[0], coarse.shape[-1]
    if bx not in (1, B):
        raise ValueError(f"match_refine: x has {bx} images, coarse has {B}")
    if by not in (1, B):
        raise ValueError(f"match_refine: y has {by} images, coarse has {B}")
    if Sc < 1 or S % Sc != 0 or not 1 <= S // Sc <= 8:
        raise ValueError(f"match_refine: coarse is {Sc} x {Sc}, which must divide S = {S} by a factor in [1, 8]")
    f, w = S // Sc, int(radius)
    if not 1 <= w <= 16:
        raise ValueError(f"match_refine: radius must be in [1, 16], got {w}")
    dev = x.device
    key = ("match_refine", dev, B, n, S, f, w)
    ws = _TTA_WS.get(key)
    if ws is None:
        nbytes = _lib.lib().skp_match_refine_workspace(B, n, S, f, w)
        if nbytes <= 0:
            raise ValueError(f"match_refine: bad shape B={B}, n={n}, S={S}, f={f}, radius={w}")
        ws = _TTA_WS[key] = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.int64)
    index = torch.empty(B, S, S, device=dev, dtype=torch.int32)
    score = torch.empty(B, S, S, device=dev, dtype=F32)
    with _timed("skp_match_refine", match_refine_bytes(B, n, S, f, w, bx, by), match_refine_flops(B, n, S, f, w)):
        call("skp_match_refine", ptr(x), n * S * S if bx == B and B > 1 else 0, ptr(y),
             n * S * S if by == B and B > 1 else 0, B, n, S, ptr(coarse), f, w, ptr(index), ptr(score), ptr(ws),
             stream(dev))
    return index, score


# --------------------------------------------------------------------------- A21 label propagation
def match_topk_flops(B, n, S, w):
    """Flop model of skp_match_topk: the dots of the definition at their bound, 2·B·n·S²·(2w + 1)²
    (windows clipped at the borders hold fewer pixels; the dots that a tile's workgroup forms outside a
    pixel's window, and the selection, are not counted)."""
    return 2 * B * n * S * S * (2 * w + 1) ** 2


def match_topk_bytes(B, n, S, w, k, bx=None, by=None):
    """Byte model of skp_match_topk: each distinct operand once (``bx``, ``by`` operands: 1 where one is
    shared, default B) plus the k slots of ``index`` and ``score``.  The regions' re-reads by
    neighbouring tiles are cache traffic."""
    bx, by = B if bx is None else bx, B if by is None else by
    return 4 * n * S * S * (bx + by) + 8 * B * k * S * S


def match_topk(x, y, radius, k):
    """The k best matches of a window centred on the pixel (skp_match_topk): for every pixel p of ``x``
    the ``k`` pixels q of ``y`` with the greatest cosine among those within ``radius`` of p on each axis.

    ``x`` and ``y`` (B or 1, n, S, S): float32, contiguous, on one device; a leading 1 beside a B is one
    operand shared by the B images (in label propagation x is the current frame and y its context
    frames).  ``radius`` in [1, 16], ``k`` in [1, 16].  Returns ``(index (B, k, S, S) int32, score
    (B, k, S, S) float32)`` with ``match_field``'s keys bit for bit: slot i holds the i-th usable q of the
    window in the order (key descending, q ascending) and that key times 1 / |x_p|; −1 and −inf where
    p is not usable or the window holds fewer usable pixels (include/skp.h).  Slot 0 is
    ``match_refine`` with an identity prior.
    """
    _lib.require_device(x, y)
    for name, t in (("x", x), ("y", y)):
        if t.dim() != 4 or t.shape[-1] != t.shape[-2]:
            raise ValueError(f"match_topk: {name} must be (B or 1, n, S, S), got {tuple(t.shape)}")
        if t.dtype != F32:
            raise ValueError(f"match_topk: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"match_topk: {name} must be contiguous, got strides {t.stride()}")
    if y.device != x.device:
        raise ValueError(f"match_topk: y on {y.device}, x on {x.device}")
    (bx, n, S, _), (by, ny, Sy, _) = x.shape, y.shape
    if ny != n or Sy != S:
        raise ValueError(f"match_topk: y is {ny} tokens of {Sy} x {Sy}, x is {n} tokens of {S} x {S}")
    B = max(bx, by)
    if bx not in (1, B):
        raise ValueError(f"match_topk: x has {bx} images, y has {by}")
    if by not in (1, B):
        raise ValueError(f"match_topk: y has {by} images, x has {bx}")
    w, K = int(radius), int(k)
    if not 1 <= w <= 16:
        raise ValueError(f"match_topk: radius must be in [1, 16], got {w}")
    if not 1 <= K <= 16:
        raise ValueError(f"match_topk: k must be in [1, 16], got {K}")
    dev = x.device
    key = ("match_topk", dev, B, n, S, w, K)
    ws = _TTA_WS.get(key)
    if ws is None:
        nbytes = _lib.lib().skp_match_topk_workspace(B, n, S, w, K)
        if nbytes <= 0:
            raise ValueError(f"match_topk: bad shape B={B}, n={n}, S={S}, radius={w}, k={K}")
        ws = _TTA_WS[key] = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.int64)
    index = torch.empty(B, K, S, S, device=dev, dtype=torch.int32)
    score = torch.empty(B, K, S, S, device=dev, dtype=F32)
    with _timed("skp_match_topk", match_topk_bytes(B, n, S, w, K, bx, by), match_topk_flops(B, n, S, w)):
        call("skp_match_topk", ptr(x), n * S * S if bx == B and B > 1 else 0, ptr(y),
             n * S * S if by == B and B > 1 else 0, B, n, S, w, K, ptr(index), ptr(score), ptr(ws), stream(dev))
    return index, score


def label_vote_bytes(M, K, S, Cl, kv, source=False):
    """Byte model of skp_label_vote: the M·K slots of ``index`` and ``score`` once (the kv scans re-read
    them from the caches), kv gathered labels per class, and ``soft``, ``label``, ``confidence`` and
    ``source`` written."""
    return S * S * (8 * M * K + 4 * Cl * kv + 4 * Cl + 8 + (4 * kv if source else 0))


def label_vote(index, score, labels, tau, k=None, return_source=False):
    """The vote of label propagation (skp_label_vote): per pixel the ``k`` best entries of M context
    frames' match lists, weighted by ``softmax(score / tau)``, vote with their own soft labels.

    ``index`` (M, K, S, S) int32 and ``score`` (M, K, S, S) float32: ``match_topk``'s with B = M <= 64.
    ``labels`` (M, Cl, S, S) float32, non-negative and finite, Cl <= 256: the context frames' soft
    labels.  ``tau`` positive; the kernel takes ``1 / tau`` rounded once to float32.  ``k`` in [1, K],
    default K.  Returns ``(soft (Cl, S, S) float32, label (S, S) int32, confidence (S, S) float32)``
    and with ``return_source`` also ``source`` (k, S, S) int32, j · S² + q of each rank or −1:
    ``label`` is the lowest class with the greatest ``soft`` value and ``confidence`` that value; a pixel
    without a candidate gets 0, −1, 0 (include/skp.h has the order of every operation).
    """
    _lib.require_device(index, score, labels)
    if index.dim() != 4 or index.shape[-1] != index.shape[-2] or index.dtype != torch.int32:
        raise ValueError(f"label_vote: index must be (M, K, S, S) int32, got {tuple(index.shape)} {index.dtype}")
    if tuple(score.shape) != tuple(index.shape) or score.dtype != F32:
        raise ValueError(f"label_vote: score must be {tuple(index.shape)} float32, got {tuple(score.shape)} {score.dtype}")
    M, K, S, _ = index.shape
    if labels.dim() != 4 or labels.shape[0] != M or tuple(labels.shape[2:]) != (S, S) or labels.dtype != F32:
        raise ValueError(f"label_vote: labels must be ({M}, Cl, {S}, {S}) float32, got {tuple(labels.shape)} {labels.dtype}")
    for name, t in (("index", index), ("score", score), ("labels", labels)):
        if not t.is_contiguous():
            raise ValueError(f"label_vote: {name} must be contiguous, got strides {t.stride()}")
    if score.device != index.device or labels.device != index.device:
        raise ValueError(f"label_vote: score on {score.device}, labels on {labels.device}, index on {index.device}")
    Cl = labels.shape[1]
    if not 1 <= M <= 64 or not 1 <= K <= 16 or not 1 <= Cl <= 256 or not 1 <= S <= 1024:
        raise ValueError(f"label_vote: M in [1, 64], K in [1, 16], Cl in [1, 256] and S in [1, 1024], got M={M}, K={K}, "
                         f"Cl={Cl}, S={S}")
    kv = K if k is None else int(k)
    if not 1 <= kv <= K:
        raise ValueError(f"label_vote: k must be in [1, {K}], got {kv}")
    t = float(tau)
    inv_tau = float(torch.tensor(1.0 / t if t > 0.0 else float("nan"), dtype=torch.float64).to(F32))
    if not 0.0 < inv_tau < float("inf"):
        raise ValueError(f"label_vote: tau must be positive with a finite float32 inverse, got {tau}")
    dev = index.device
    soft = torch.empty(Cl, S, S, device=dev, dtype=F32)
    label = torch.empty(S, S, device=dev, dtype=torch.int32)
    conf = torch.empty(S, S, device=dev, dtype=F32)
    source = torch.empty(kv, S, S, device=dev, dtype=torch.int32) if return_source else None
    with _timed("skp_label_vote", label_vote_bytes(M, K, S, Cl, kv, return_source)):
        call("skp_label_vote", ptr(index), ptr(score), M, K, S, ptr(labels), Cl, inv_tau, kv, ptr(soft), ptr(label),
             ptr(conf), ptr(source), stream(dev))
    return (soft, label, conf, source) if return_source else (soft, label, conf)


# --------------------------------------------------------------------------- A20 keypoint tracks
def track_weights(sigma, radius=None):
    """The transition table of ``track_step``: ``w[k] = exp(−k² / (2σ²))`` for k = 0 … radius, evaluated
    in double on the host and rounded once to float32 (a CPU tensor; ``w[0] == 1``).  ``radius=None`` is
    ``ceil(3σ)`` clipped to [1, 32]; a given radius must lie in [1, 32].  A table whose last entry
    rounds to 0 is refused (the kernel takes weights in (0, 1]): lower the radius or raise sigma."""
    import math
    s = float(sigma)
    if not 0.0 < s < float("inf"):
        raise ValueError(f"track_weights: sigma must be positive and finite, got {s}")
    r = min(max(int(math.ceil(3.0 * s)), 1), 32) if radius is None else int(radius)
    if not 1 <= r <= 32:
        raise ValueError(f"track_weights: radius must be in [1, 32], got {r}")
    w = torch.tensor([math.exp(-(k * k) / (2.0 * s * s)) for k in range(r + 1)], dtype=torch.float64).to(F32)
    if not float(w[-1]) > 0.0:
        raise ValueError(f"track_weights: exp(-{r}^2 / (2 * {s}^2)) rounds to 0 in float32: lower the radius")
    return w


def track_step_bytes(n, S):
    """Byte model of skp_track_step: per pixel three planes of 4 bytes (the average and the previous
    score read, the score written) and one of 2 (the back-pointer).  The halo's re-reads are cache
    traffic."""
    return (3 * 4 + 2) * n * S * S


def track_step(avg, state=None, weights=None, back=None):
    """One frame of the keypoint tracker (skp_track_step): the Viterbi step of include/skp.h, per token
    an exact max-product over the (2r + 1)² window in two separable stages from an LDS tile.

    ``avg`` (n, S, S): the frame's TTA averages, float32, contiguous, on the device.  ``state``: what
    the previous frame's call returned, None for frame 0.  ``weights``: the float32 CPU table of
    ``track_weights`` (r + 1 entries, r in [1, 32]).  ``back``: an (n, S, S) int16 contiguous buffer
    to write the back-pointers into (a slice of the caller's (T, n, S, S) stack), else a new one.
    Returns the state ``(score (n, S, S), score_max (n), best (n) int32, back (n, S, S) int16)``.
    """
    _lib.require_device(avg)
    if avg.dim() != 3 or avg.shape[-1] != avg.shape[-2]:
        raise ValueError(f"track_step: avg must be (n, S, S), got {tuple(avg.shape)}")
    if avg.dtype != F32:
        raise ValueError(f"track_step: avg must be float32, got {avg.dtype}")
    if not avg.is_contiguous():
        raise ValueError(f"track_step: avg must be contiguous, got strides {avg.stride()}")
    if (not torch.is_tensor(weights) or weights.is_cuda or weights.dtype != F32 or weights.dim() != 1
            or not weights.is_contiguous() or not 2 <= weights.numel() <= 33):
        raise ValueError("track_step: weights must be the float32 CPU table of track_weights (2 to 33 entries)")
    n, S, _ = avg.shape
    r, dev = weights.numel() - 1, avg.device
    prev, prev_max = (None, None) if state is None else (state[0], state[1])
    for name, t, shape in (("state's score", prev, (n, S, S)), ("state's score_max", prev_max, (n,))):
        if t is None:
            continue
        if tuple(t.shape) != shape or t.dtype != F32 or not t.is_contiguous():
            raise ValueError(f"track_step: the {name} must be {shape} float32 contiguous, got {tuple(t.shape)} {t.dtype}")
        if t.device != dev:
            raise ValueError(f"track_step: the {name} on {t.device}, avg on {dev}")
    if back is None:
        back = torch.empty(n, S, S, device=dev, dtype=torch.int16)
    elif (tuple(back.shape) != (n, S, S) or back.dtype != torch.int16 or not back.is_contiguous()
          or back.device != dev):
        raise ValueError(f"track_step: back must be ({n}, {S}, {S}) int16 contiguous on {dev}")
    key = ("track_step", dev, n, S, r)
    ws = _TTA_WS.get(key)
    if ws is None:
        nbytes = _lib.lib().skp_track_step_workspace(n, S, r)
        if nbytes <= 0:
            raise ValueError(f"track_step: bad shape n={n}, S={S}, r={r}")
        ws = _TTA_WS[key] = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.int64)
    score = torch.empty(n, S, S, device=dev, dtype=F32)
    score_max = torch.empty(n, device=dev, dtype=F32)
    best = torch.empty(n, device=dev, dtype=torch.int32)
    with _timed("skp_track_step", track_step_bytes(n, S)):
        call("skp_track_step", ptr(avg), ptr(prev), ptr(prev_max), n, S, ctypes.c_void_p(weights.data_ptr()), r,
             ptr(score), ptr(score_max), ptr(best), ptr(back), ptr(ws), stream(dev))
    return score, score_max, best, back


def track_backtrace(back_stack, best_last, radius):
    """The tracks of ``track_step``'s frames (skp_track_backtrace): ``back_stack`` (T, n, S, S) int16 the
    frames' back-pointers in frame order, ``best_last`` (n) int32 the last frame's ``best``, ``radius``
    the steps'.  Returns ``pos`` (T, n, 2) = (row + 0.5, col + 0.5) of the path's pixel in every frame."""
    _lib.require_device(back_stack, best_last)
    if back_stack.dim() != 4 or back_stack.shape[-1] != back_stack.shape[-2] or back_stack.dtype != torch.int16:
        raise ValueError(f"track_backtrace: back_stack must be (T, n, S, S) int16, got {tuple(back_stack.shape)} "
                         f"{back_stack.dtype}")
    if not back_stack.is_contiguous():
        raise ValueError(f"track_backtrace: back_stack must be contiguous, got strides {back_stack.stride()}")
    T, n, S, _ = back_stack.shape
    if tuple(best_last.shape) != (n,) or best_last.dtype != torch.int32 or not best_last.is_contiguous():
        raise ValueError(f"track_backtrace: best_last must be ({n},) int32, got {tuple(best_last.shape)} {best_last.dtype}")
    if best_last.device != back_stack.device:
        raise ValueError(f"track_backtrace: best_last on {best_last.device}, back_stack on {back_stack.device}")
    dev = back_stack.device
    pos = torch.empty(T, n, 2, device=dev, dtype=F32)
    with _timed("skp_track_backtrace", 2 * T * n + 8 * T * n + 4 * n):
        call("skp_track_backtrace", ptr(back_stack), ptr(best_last), T, n, S, int(radius), ptr(pos), stream(dev))
    return pos
