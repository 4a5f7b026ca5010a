"""Where every op writes, and whether its result depends on what its buffers held before.

include/skp.h: "caller owns every buffer; the library keeps no global state", with a documented size
for every output and workspace.  Each case below runs one op (forward and, where it has one,
backward) three times — plainly, then with every ``torch.empty`` / ``torch.empty_like`` buffer of
stablekeypoints_amd.ops carved out of a poisoned allocation with guard bands (tests/guarded_alloc.py)
under the poisons 0xFF and 0x7F — and asserts

1. no guard byte changed (no store before the start or past the end of an output or workspace), and
   at least one buffer was guarded;
2. the defined outputs are bit-equal across the three runs (no element left unwritten, no workspace
   slot read before it is written).  The one atomicAdd of the library is the warp adjoint's scatter
   (skp_warp.hip): the gradients it produces — affine_warp's dx and the equivariance losses' dAt,
   and only those results — agree within 1e-6 of the largest magnitude instead, the bound
   test_losses_batched_equal_per_image holds dAt to, and hold no NaN and nothing above 1e30;
3. every input is bit-unchanged (the documented in-place operands excepted);
4. the HIP entry points the case is about were the ones called.

Three ops (qkv_projection, tokens_proj_in, conv1x1) are torch GEMMs that own no buffer and call no
libskp entry; their cases assert exactly that, besides 2 and 3.

Out-of-bounds reads are out of reach of this file.
"""
import numpy as np
import pytest
import torch

import recipes
import render_ref
import tta_ref
from guarded_alloc import POISONS, GuardedAlloc, bit_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def T(a, **kw):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, **kw)


def rnd(seed, *shape, scale=1.0):
    """Seeded, finite, O(1) normal values on the device."""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def grads(loss_terms, leaves):
    """Backward of Σ (out · weight) and the leaves' gradients."""
    sum((o * w).sum() for o, w in loss_terms).backward()
    return [t.grad for t in leaves]


class Case:
    """``make()`` -> dict of input tensors (or lists of them); ``run(ops, inp, g)`` -> list of result
    tensors, ``g`` the active GuardedAlloc (None in the plain run) for buffers the CALLER allocates;
    ``defined(results)`` -> the part skp.h says is written (default: all of it); ``inexact``: the
    indices of the results scattered with atomicAdd (every other result is bit-compared);
    ``mutates``: inputs the op documents as written in place; ``patch``: module switches of ops;
    ``kernels``: HIP entry points that must have been called; ``results_guarded`` False where no
    result is a buffer of ops' own making (stated per case); ``owns_no_buffer``: the op is torch's
    GEMM alone — it must allocate nothing through ops and call no libskp entry."""

    def __init__(self, name, make, run, *, defined=None, inexact=(), mutates=(), patch=None, kernels=(),
                 results_guarded=True, owns_no_buffer=False):
        self.name, self.make, self.run = name, make, run
        self.results_guarded, self.owns_no_buffer = results_guarded, owns_no_buffer
        self.defined, self.inexact, self.mutates = defined, tuple(inexact), tuple(mutates)
        self.patch, self.kernels = dict(patch or {}), tuple(kernels)


CASES = []


def case(name, make, run, **kw):
    marks = kw.pop("marks", ())
    CASES.append(pytest.param(Case(name, make, run, **kw), id=name, marks=marks))


FUSED_CONV = dict(WINO_MIN_WORKGROUPS=1, WINO_GEMM_MAX_HW=0)     # as tests/test_gpu_conv.py's all_shapes


# =========================================================================================== GEMM
def _bgemm_cases():
    case("bgemm-3x37x53x19", lambda: dict(a=rnd(1, 3, 37, 19), b=rnd(2, 3, 19, 53)),
         lambda ops, i, g: [ops.bgemm(i["a"], i["b"], 0.7)], kernels=["skp_bgemm_f32"])

    def run_acc(ops, i, g):
        out = g.guarded((2, 70, 45), F32) if g is not None else torch.empty(2, 70, 45, device=DEV)
        out.copy_(i["c0"])
        return [ops.bgemm(i["a"], i["bt"].transpose(1, 2), 0.5, out=out, accumulate=True)]
    case("bgemm-2x70x45x37-strided-b-accumulate",
         lambda: dict(a=rnd(3, 2, 70, 37), bt=rnd(4, 2, 45, 37), c0=rnd(5, 2, 70, 45)), run_acc,
         kernels=["skp_bgemm_f32"])
    case("bgemm-stride0-batch", lambda: dict(a=rnd(6, 3, 37, 19), b1=rnd(7, 1, 19, 53)),
         lambda ops, i, g: [ops.bgemm(i["a"], i["b1"].expand(3, 19, 53))], kernels=["skp_bgemm_f32"])

    # the smallest case of tests/test_gpu_heads.py (H = 4, d = 8) with B, S, N = 2, 64, 37
    B, S, N, H, d = 2, 64, 37, 4, 8
    C = H * d

    def heads_in():
        return dict(q=rnd(8, B, S, C), k=rnd(9, 1, N, C), v=rnd(10, 1, N, C), wz=rnd(11, B * H, S, N),
                    wo=rnd(12, B, S, C))

    def run_2b(ops, i, g):
        z = g.guarded((B * H, S, N), F32) if g is not None else torch.empty(B * H, S, N, device=DEV)
        ops.bgemm_2b(i["q"], (S * C, d, C, 1), i["k"], (0, d, 1, C), z, (H * S * N, S * N, N, 1), B * H, H, S, N, d,
                     d ** -0.5)
        return [z]
    case("bgemm_2b-heads-2x64x37", heads_in, run_2b, kernels=["skp_bgemm_f32_2b"])

    def run_heads(ops, i, g):
        q, k, v = (i[n].requires_grad_() for n in "qkv")
        z = ops.capture_logits_heads(q, k, H, d ** -0.5)
        out = ops.attn_pv_heads(z.softmax(dim=-1), v, H)
        return [z, out] + grads([(z, i["wz"]), (out, i["wo"])], (q, k, v))
    case("capture_logits_heads+attn_pv_heads-2x64x37", heads_in, run_heads, kernels=["skp_bgemm_f32_2b"])

    # torch.matmul / torch.bmm on hipBLASLt alone (ops.QKVProjection, TokensProjIn, Conv1x1): no buffer
    # of ops' making and no libskp entry — asserted, with the runs' agreement and the inputs
    def run_qkv(ops, i, g):
        x = i["x"].requires_grad_()
        q, k, v = ops.qkv_projection(x, i["w0"], i["w1"], i["w2"])
        return [q, k, v] + grads([(q, i["g0"]), (k, i["g1"]), (v, i["g2"])], (x,))
    case("qkv_projection-2x64x96",
         lambda: dict(x=rnd(13, 2, 64, 96), w0=rnd(14, 96, 96, scale=0.1), w1=rnd(15, 96, 96, scale=0.1),
                      w2=rnd(16, 96, 96, scale=0.1), g0=rnd(17, 2, 64, 96), g1=rnd(18, 2, 64, 96),
                      g2=rnd(19, 2, 64, 96)),
         run_qkv, owns_no_buffer=True)

    # (B, C, K, H, W) = (3, 96, 32, 8, 12): 96 channels -> 32, 96 pixels
    def proj_in(ops, i, g):
        x = i["x"].requires_grad_()
        h = ops.tokens_proj_in(x, i["w"], i["b"])
        return [h] + grads([(h, i["gh"])], (x,))
    case("tokens_proj_in-3x96x32x8x12",
         lambda: dict(x=rnd(20, 3, 96, 8, 12), w=rnd(21, 32, 96, 1, 1, scale=0.1), b=rnd(22, 32),
                      gh=rnd(23, 3, 96, 32)),
         proj_in, owns_no_buffer=True)

    def proj_out(ops, i, g):
        h, res = i["h"].requires_grad_(), i["res"].requires_grad_()
        y = ops.tokens_proj_out(h, i["w"], i["b"], res)
        return [y] + grads([(y, i["gy"])], (h, res))
    case("tokens_proj_out-3x96x32x8x12",
         lambda: dict(h=rnd(24, 3, 96, 32), w=rnd(25, 96, 32, 1, 1, scale=0.1), b=rnd(26, 96),
                      res=rnd(27, 3, 96, 8, 12), gy=rnd(28, 3, 96, 8, 12)),
         proj_out, kernels=["skp_residual_bias_add"])

    def c1x1(ops, i, g):
        x = i["x"].requires_grad_()
        y = ops.conv1x1(x, i["w"])
        return [y] + grads([(y, i["gy"])], (x,))
    case("conv1x1-3x96x32x8x12",
         lambda: dict(x=rnd(29, 3, 96, 8, 12), w=rnd(30, 32, 96, 1, 1, scale=0.1), gy=rnd(31, 3, 32, 8, 12)),
         c1x1, patch=dict(CONV1X1_GEMM=True), owns_no_buffer=True)


_bgemm_cases()


# =========================================================================================== capture
def _capture_fwd_stats(ops, z, s, R):
    """skp_capture_fwd with its per-pixel softmax stats, as CaptureMaps' two-kernel path calls it."""
    BH, _, N = z.shape
    attn = torch.empty(BH, R * R, N, device=z.device, dtype=F32)
    st = torch.empty(BH, R * R, 2, device=z.device, dtype=F32)
    ops.call("skp_capture_fwd", ops.ptr(z), BH, s, N, R, ops.ptr(attn), ops.ptr(st), ops.stream(z.device))
    return attn, st


def _capture_cases():
    for BH, s, R, N in ((3, 5, 13, 70), (2, 8, 32, 77)):
        def mk(BH=BH, s=s, R=R, N=N):
            return dict(z=T(recipes.random_logits(40 + N, (BH, s * s, N), scale=2.0)), go=rnd(41, BH, R * R, N))

        def run(ops, i, g, s=s, R=R):
            z = i["z"].requires_grad_()
            attn = ops.capture_attn(z, s, R)
            return [attn] + grads([(attn, i["go"])], (z,))
        case(f"capture_attn+capture_bwd-{BH}x{s}x{R}x{N}", mk, run, kernels=["skp_capture_fwd", "skp_capture_bwd"])

        def run_st(ops, i, g, s=s, R=R):
            attn, st = _capture_fwd_stats(ops, i["z"], s, R)
            return [attn, st, ops.capture_bwd(i["z"], s, R, i["go"], gscale=0.5, stats=st)]
        case(f"capture_fwd+capture_bwd-stats-{BH}x{s}x{R}x{N}", mk, run_st,
             kernels=["skp_capture_fwd", "skp_capture_bwd"])

    # N = 36 is not in the issue's list: a multiple of 4, so the backward is the one-launch
    # skp_capture_maps_bwd with its own workspace (N = 37 and 130 take skp_capture_bwd per layer)
    for B, H, sizes, R, N in ((1, 3, (5, 3), 40, 37), (3, 1, (1, 2), 8, 130), (1, 3, (5, 3), 40, 36)):
        def mk(B=B, H=H, sizes=sizes, R=R, N=N):
            return dict(zs=[T(recipes.random_logits(50 + l, (B * H, s * s, N), scale=2.0))
                            for l, s in enumerate(sizes)], go=rnd(51, B, N, R, R))

        def run(ops, i, g, B=B, sizes=sizes, R=R):
            zs = [z.requires_grad_() for z in i["zs"]]
            m = ops.capture_maps(zs, sizes, B, R)
            return [m] + grads([(m, i["go"])], zs)
        case(f"capture_maps-fwd+bwd-B{B}-H{H}-R{R}-N{N}", mk, run,
             kernels=["skp_capture_maps_fwd", "skp_capture_maps_bwd" if N % 4 == 0 else "skp_capture_bwd"])

    # tests/test_gpu_sel_bwd.py's cases: a duplicated token, N past one 128-token chunk, the dense
    # fallback with ragged rows
    for B, H, sizes, R, N, K, dup, ragged in ((2, 4, (4, 8), 32, 64, 5, True, False),
                                              (1, 2, (8,), 128, 132, 3, False, False),
                                              (2, 3, (5, 3), 40, 36, 4, True, True)):
        def mk(B=B, H=H, sizes=sizes, R=R, N=N, K=K, dup=dup, ragged=ragged):
            rng = np.random.default_rng(500 + N + R)
            zs = [recipes.random_logits(500 + N + R + 3 * l, (B * H, s * s, N), scale=2.0) for l, s in enumerate(sizes)]
            tok = np.stack([rng.choice(N, size=K, replace=False) for _ in range(B)]).astype(np.int64)
            if dup:
                tok[:, -1] = tok[:, 0]
            if ragged:
                tok[0, K // 2:] = -1
                if B > 1:
                    tok[-1, :] = -1
            gsel = rng.standard_normal((B, K, R, R)).astype(np.float32)
            gsel[tok < 0] = 0.0
            return dict(zs=[T(z) for z in zs], tok=T(tok), gsel=T(gsel))

        def run(ops, i, g, B=B, H=H, sizes=sizes, R=R):
            maps, stats = ops._capture_maps_run(i["zs"], sizes, B, R)
            dzs = ops.capture_maps_bwd_sel(i["zs"], sizes, B, R, i["tok"], i["gsel"], 1.0 / (len(sizes) * H), stats)
            return [maps] + list(stats) + list(dzs)
        # skp_capture_sel.hip: "one owner and a fixed summation order: deterministic, no atomics"
        case(f"capture_maps_bwd_sel-B{B}-H{H}-R{R}-N{N}-K{K}", mk, run,
             kernels=["skp_capture_maps_fwd", "skp_capture_maps_bwd_sel"])

    for with_idx in (False, True):
        for up in (-1, 32):
            def mk():
                return dict(l0=T(recipes.uniform(60, (3, 13 * 13, 70))), l1=T(recipes.uniform(61, (3, 13 * 13, 70))),
                            idx=torch.tensor([5, 0, 69, 5], device=DEV), go=rnd(62, 70, 32, 32))

            def run(ops, i, g, with_idx=with_idx, up=up):
                ls = [i["l0"].requires_grad_(), i["l1"].requires_grad_()]
                m = ops.aggregate(ls, i["idx"] if with_idx else None, up)
                return [m] + grads([(m, i["go"][:m.shape[0], :m.shape[1], :m.shape[2]])], ls)
            case(f"aggregate-idx{int(with_idx)}-up{up}", mk, run,
                 kernels=["skp_aggregate"] + (["skp_resize_bilinear", "skp_resize_bilinear_bwd"] if up > 0 else []))

    for R, Ro in ((5, 13), (16, 32)):
        def run(ops, i, g, Ro=Ro):
            x = i["x"].requires_grad_()
            y = ops.resize_bilinear(x, Ro)
            return [y] + grads([(y, i["go"])], (x,))
        case(f"resize_bilinear-3x{R}to{Ro}", lambda R=R, Ro=Ro: dict(x=rnd(63, 3, R, R), go=rnd(64, 3, Ro, Ro)), run,
             kernels=["skp_resize_bilinear", "skp_resize_bilinear_bwd"])


_capture_cases()


# =========================================================================================== argmax family
def _argmax_cases():
    for Tn, S in ((7, 37), (3, 64)):
        def mk(Tn=Tn, S=S):
            return dict(maps=T(recipes.attention_like_maps(70 + S, Tn, S)), pos=T(recipes.uniform(71, (3, Tn, 2))))
        tag = f"{Tn}x{S}x{S}"
        case(f"find_max_pixel-{tag}", mk, lambda ops, i, g: [ops.find_max_pixel(i["maps"])], kernels=["skp_argmax2d"])
        case(f"argmax_index-{tag}", mk, lambda ops, i, g: [ops.argmax_index(i["maps"])], kernels=["skp_argmax2d"])
        case(f"find_k_max_pixels-{tag}", mk,
             lambda ops, i, g: list(ops.find_k_max_pixels(i["maps"], num=3, return_masked=True)),
             kernels=["skp_k_max_pixels"])
        case(f"mask_radius-{tag}", mk,
             lambda ops, i, g, S=S: [ops.mask_radius(i["maps"], i["pos"][0] * S, 0.15 * S)], kernels=["skp_mask_radius"])
        for dist in (5, -1):
            # mutates its heat maps in place like the reference (skp.h, skp_weighted_avg: mutate != 0)
            case(f"pixel_from_weighted_avg-d{dist}-{tag}", mk,
                 lambda ops, i, g, dist=dist: [ops.pixel_from_weighted_avg(i["maps"], dist), i["maps"]],
                 mutates=["maps"], kernels=["skp_weighted_avg"])
        case(f"gaussian_circles-{tag}", mk, lambda ops, i, g, S=S: [ops.gaussian_circles(i["pos"], S, 2.0)],
             kernels=["skp_gaussian_target"])


_argmax_cases()


# =========================================================================================== selection
NB, TOK, SZ, NCAND, TOPK = 3, 37, 32, 11, 4


def _fps_tail(res):
    """skp.h, skp_fps: "out[n_out:] = -1" — every entry of out is defined and compared; this only
    adds the documented tail value to what the three runs must agree on."""
    out, n_out = res[0], res[1]
    rows = out.reshape(n_out.numel(), -1)
    for b in range(rows.shape[0]):
        k = int(n_out.reshape(-1)[b])
        assert 0 <= k <= rows.shape[1] and bool((rows[b, k:] == -1).all()) and bool((rows[b, :k] >= 0).all()), (b, k, rows[b])
    return res


def _selection_cases():
    def mk():
        rng = np.random.default_rng(80)
        maps = np.stack([recipes.attention_like_maps(81 + b, TOK, SZ) for b in range(NB)])
        maps_t = np.stack([recipes.attention_like_maps(91 + b, TOK, SZ) for b in range(NB)])
        cand = np.stack([rng.permutation(TOK)[:NCAND] for _ in range(NB)]).astype(np.int64)
        keys = rng.standard_normal((NB, TOK))
        return dict(maps=T(maps), maps_t=T(maps_t), cand=T(cand), keys=T(keys))

    for ns in (1, 2):
        case(f"find_top_k_gaussian-subjects{ns}", mk,
             lambda ops, i, g, ns=ns: list(ops.find_top_k_gaussian(i["maps"][0], NCAND, sigma=3, num_subjects=ns,
                                                                   return_kl=True)),
             kernels=["skp_topk_gaussian"])
        case(f"find_top_k_gaussian_batch-subjects{ns}", mk,
             lambda ops, i, g, ns=ns: [ops.find_top_k_gaussian_batch(i["maps"], NCAND, sigma=3, num_subjects=ns)],
             kernels=["skp_topk_gaussian_batch"])
        case(f"gaussian_fps_batch-subjects{ns}", mk,
             lambda ops, i, g, ns=ns: list(ops.gaussian_fps_batch(i["maps"], i["maps_t"], NCAND, TOPK, sigma=3,
                                                                  num_subjects=ns)),
             defined=_fps_tail, kernels=["skp_topk_gaussian_batch", "skp_fps_keys_batch"])
    case("entropy_sort", mk, lambda ops, i, g: list(ops.entropy_sort(i["maps"][0], NCAND, return_entropy=True)),
         kernels=["skp_entropy_sort"])
    case("entropy_sort_batch", mk, lambda ops, i, g: [ops.entropy_sort_batch(i["maps"], NCAND)],
         kernels=["skp_entropy_sort", "skp_topk_keys"])
    case("entropy_keys_batch", mk, lambda ops, i, g: [ops.entropy_keys_batch(i["maps"])], kernels=["skp_entropy_sort"])
    case("furthest_point_sampling", mk,
         lambda ops, i, g: list(ops.furthest_point_sampling(i["maps"][0], TOPK, i["cand"][0])),
         defined=_fps_tail, kernels=["skp_fps"])
    case("furthest_point_sampling_batch", mk,
         lambda ops, i, g: list(ops.furthest_point_sampling_batch(i["maps"], TOPK, i["cand"])),
         defined=_fps_tail, kernels=["skp_fps_batch"])
    case("fps_from_keys_batch", mk, lambda ops, i, g: list(ops.fps_from_keys_batch(i["keys"], i["maps"], NCAND, TOPK)),
         defined=_fps_tail, kernels=["skp_fps_keys_batch"])


_selection_cases()


# =========================================================================================== losses and warp
THETA3 = [[[0.9, -0.1, 0.05], [0.12, 0.95, -0.2]], [[1.1, 0.0, 0.1], [0.0, 1.05, 0.0]],
          [[0.97, 0.2, -0.15], [-0.2, 0.97, 0.1]]]


def _loss_cases():
    n, nb, S = 5, 3, 32

    def mk():
        A = np.stack([recipes.attention_like_maps(100 + b, n, S) for b in range(nb)]).reshape(nb * n, S, S)
        At = np.stack([recipes.attention_like_maps(110 + b, n, S) for b in range(nb)]).reshape(nb * n, S, S)
        return dict(A=T(A), At=T(At), A1=T(A[:n]), At1=T(At[:n]), th=torch.tensor(THETA3, device=DEV),
                    w=torch.tensor([1.0, -2.0, 0.5], device=DEV))

    for ns in (1, 2):
        def run1(ops, i, g, ns=ns):
            A = i["A1"].requires_grad_()
            loss = ops.sharpening_loss(A, sigma=2.0, num_subjects=ns)
            return [loss] + grads([(loss, i["w"][1])], (A,))
        case(f"sharpening_loss-subjects{ns}", mk, run1, kernels=["skp_sharpen_fwd", "skp_sharpen_bwd"])

        def runb(ops, i, g, ns=ns):
            A = i["A"].requires_grad_()
            loss = ops.sharpening_loss_batch(A, nb, sigma=2.0, num_subjects=ns)
            return [loss] + grads([(loss, i["w"])], (A,))
        case(f"sharpening_loss_batch-subjects{ns}", mk, runb, kernels=["skp_sharpen_fwd_batch", "skp_sharpen_bwd_batch"])

    # results (loss, dA, dAt): dAt alone scatters through the warp adjoint's atomicAdd (skp_warp.hip);
    # the loss and dA are bit-compared, as in test_losses_batched_equal_per_image
    def eq1(ops, i, g):
        A, At = i["A1"].requires_grad_(), i["At1"].requires_grad_()
        loss = ops.equivariance_loss_single(A, At, i["th"][0])
        return [loss] + grads([(loss, i["w"][1])], (A, At))
    case("equivariance_loss_single", mk, eq1, inexact=[2], kernels=["skp_equiv_fwd", "skp_equiv_bwd"])

    def eqb(ops, i, g):
        A, At = i["A"].requires_grad_(), i["At"].requires_grad_()
        loss = ops.equivariance_loss_batch(A, At, i["th"], nb)
        return [loss] + grads([(loss, i["w"])], (A, At))
    case("equivariance_loss_batch", mk, eqb, inexact=[2], kernels=["skp_equiv_fwd_batch", "skp_equiv_bwd_batch"])

    for B, C, H, W in ((2, 3, 37, 41), (1, 1, 64, 64)):
        def run(ops, i, g):
            x = i["x"].requires_grad_()
            y = ops.affine_warp(x, i["th"])
            return [y] + grads([(y, i["go"])], (x,))
        case(f"affine_warp-{B}x{C}x{H}x{W}",
             lambda B=B, C=C, H=H, W=W: dict(x=rnd(120, B, C, H, W), go=rnd(121, B, C, H, W),
                                             th=torch.tensor(THETA3[:B], device=DEV)),
             run, inexact=[1], kernels=["skp_affine_warp", "skp_affine_warp_bwd"])   # (y, dx): dx is the scatter


_loss_cases()


# =========================================================================================== norms, elementwise
def _norm_cases():
    for B, C, H, W, G, act, shifted in ((2, 12, 5, 7, 4, True, True), (1, 64, 16, 16, 8, False, False)):
        def mk(B=B, C=C, H=H, W=W, shifted=shifted):
            d = dict(x=rnd(130, B, C, H, W), gamma=1 + rnd(131, C, scale=0.2), beta=rnd(132, C, scale=0.2),
                     go=rnd(133, B, C, H, W), gp=rnd(134, B, C, H, W))
            if shifted:
                d["shift"] = rnd(135, B, C, scale=0.5)
            return d

        def run(ops, i, g, G=G, act=act):
            x = i["x"].requires_grad_()
            y = ops.group_norm_act(x, i["gamma"], i["beta"], G, 1e-5, act, i.get("shift"))
            return [y] + grads([(y, i["go"])], (x,))
        case(f"group_norm_act-{B}x{C}x{H}x{W}-G{G}", mk, run, kernels=["skp_groupnorm_fwd", "skp_groupnorm_bwd"])

        def run_res(ops, i, g, G=G, act=act):
            x = i["x"].requires_grad_()
            y, xp = ops.group_norm_act_res(x, i["gamma"], i["beta"], G, 1e-5, act)
            return [y, xp] + grads([(y, i["go"]), (xp, i["gp"])], (x,))
        case(f"group_norm_act_res-{B}x{C}x{H}x{W}-G{G}", mk, run_res,
             kernels=["skp_groupnorm_fwd", "skp_groupnorm_bwd_add"])

    for shape in ((7, 12), (5, 2048)):
        def run(ops, i, g):
            x = i["x"].requires_grad_()
            y = ops.layer_norm(x, i["w"], i["b"], 1e-5)
            return [y] + grads([(y, i["go"])], (x,))
        case(f"layer_norm-{shape[0]}x{shape[1]}",
             lambda shape=shape: dict(x=rnd(140, *shape), w=1 + rnd(141, shape[1], scale=0.2),
                                      b=rnd(142, shape[1], scale=0.2), go=rnd(143, *shape)),
             run, patch=dict(LN_MIN_ROWS=1), kernels=["skp_layernorm_fwd", "skp_layernorm_bwd"])

    def run_lnr(ops, i, g):
        x = i["x"].requires_grad_()
        y, xp = ops.layer_norm_res(x, i["w"], i["b"], 1e-5)
        return [y, xp] + grads([(y, i["go"]), (xp, i["gp"])], (x,))
    case("layer_norm_res-13x96",
         lambda: dict(x=rnd(144, 13, 96), w=1 + rnd(145, 96, scale=0.2), b=rnd(146, 96, scale=0.2),
                      go=rnd(147, 13, 96), gp=rnd(148, 13, 96)),
         run_lnr, patch=dict(LN_MIN_ROWS=1), kernels=["skp_layernorm_fwd", "skp_layernorm_bwd_add"])

    def run_geglu(ops, i, g):
        h = i["h"].requires_grad_()
        y = ops.geglu(h)
        return [y] + grads([(y, i["go"])], (h,))
    case("geglu-3x7x16", lambda: dict(h=rnd(150, 3, 7, 16), go=rnd(151, 3, 7, 8)), run_geglu,
         kernels=["skp_geglu_fwd", "skp_geglu_bwd"])

    case("residual_bias_add-2x12x5x7", lambda: dict(a=rnd(152, 2, 12, 5, 7), h=rnd(153, 2, 12, 5, 7), b=rnd(154, 12)),
         lambda ops, i, g: [ops.residual_bias_add(i["a"], i["h"], i["b"])], kernels=["skp_residual_bias_add"])

    # in place on the caller's tensor: the caller's buffer is the guarded one
    def run_softmax(ops, i, g):
        s = g.guarded((33, 500), F32) if g is not None else torch.empty(33, 500, device=DEV)
        s.copy_(i["s"])
        return [ops.softmax_(s)]
    case("softmax_-33x500", lambda: dict(s=rnd(155, 33, 500, scale=3.0)), run_softmax, kernels=["skp_softmax_fwd"])

    # skp_softmax_bwd overwrites dP with scale·dS in place; in MathAttention that tensor is torch.bmm's,
    # so here it is called as MathAttention.backward calls it, on a caller-guarded ds — at the key
    # counts of the P-saving attention cases that reach it (129 and 1) and a multiple of 4
    for rows, cols in ((2 * 64, 129), (3 * 128, 1), (33, 500)):
        def run_sbwd(ops, i, g, rows=rows, cols=cols):
            ds = g.guarded((rows, cols), F32) if g is not None else torch.empty(rows, cols, device=DEV)
            ds.copy_(i["dp"])
            ops.call("skp_softmax_bwd", ops.ptr(i["p"]), ops.ptr(ds), rows, cols, 0.125, ops.stream(ds.device))
            return [ds]
        case(f"softmax_bwd-{rows}x{cols}",
             lambda rows=rows, cols=cols: dict(p=rnd(156, rows, cols, scale=3.0).softmax(-1), dp=rnd(157, rows, cols)),
             run_sbwd, kernels=["skp_softmax_bwd"])


_norm_cases()


# =========================================================================================== attention
def _attention_cases():
    def mk(BH, S, L, D):
        return lambda: dict(q=rnd(160, BH, S, D, scale=1.5), k=rnd(161, BH, L, D, scale=1.5),
                            v=rnd(162, BH, L, D, scale=1.5), go=rnd(163, BH, S, D))

    def run(ops, i, g):
        q, k, v = (i[n].requires_grad_() for n in "qkv")
        out = ops.math_attention(q, k, v, q.shape[-1] ** -0.5)
        return [out] + grads([(out, i["go"])], (q, k, v))

    # (2, 64, 128, 40) is not in the issue's list: a key count the fused kv backward and the fused
    # score gradient take (L a multiple of 64; L = 129 and L = 1 run skp_softmax_bwd)
    for BH, S, L, D in ((2, 64, 129, 80), (3, 128, 1, 40), (2, 64, 128, 40)):
        # L = 129 and L = 1: MathAttention's only buffer is baddbmm's ignored beta = 0 operand; the
        # output and every gradient are torch.bmm's, and skp_softmax_bwd works in place on one of
        # those, so the poisons reach no result there (only the three runs' agreement is checked)
        blocked = L % 64 == 0
        case(f"math_attention-psaving-fusedkv-{BH}x{S}x{L}x{D}", mk(BH, S, L, D), run,
             patch=dict(ATTN_FLASH=(), ATTN_FUSED_KV=(40, 64, 80)), results_guarded=blocked,
             kernels=["skp_attn_bwd_kv" if blocked else "skp_softmax_bwd"])
        case(f"math_attention-psaving-unfused-{BH}x{S}x{L}x{D}", mk(BH, S, L, D), run,
             patch=dict(ATTN_FLASH=(), ATTN_FUSED_KV=()), results_guarded=False,   # ds is guarded; dq, dk are bmm's of it
             kernels=["skp_attn_dscore" if blocked else "skp_softmax_bwd"])
        case(f"math_attention-flash-{BH}x{S}x{L}x{D}", mk(BH, S, L, D), run, patch=dict(ATTN_FLASH=(40, 64, 80)),
             kernels=["skp_attn_fwd", "skp_attn_bwd_flash"])

    def run_ng(ops, i, g):
        with torch.no_grad():
            return [ops.attention_nograd(i["q"], i["k"], i["v"], i["q"].shape[-1] ** -0.5)]
    for BH, S, L, D in ((2, 64, 77, 40), (2, 128, 1, 64)):
        case(f"attention_nograd-{BH}x{S}x{L}x{D}", mk(BH, S, L, D), run_ng, kernels=["skp_attn_fwd"])

    for B, H, S, L, d, shared in ((2, 5, 64, 77, 64, True), (2, 4, 64, 64, 40, False)):
        C = H * d

        def mkb(B=B, S=S, L=L, C=C, shared=shared):
            return dict(q=rnd(164, B, S, C), k=rnd(165, 1 if shared else B, L, C), v=rnd(166, 1 if shared else B, L, C),
                        go=rnd(167, B, S, C))

        def runb(ops, i, g, B=B, H=H, L=L, C=C, d=d):
            q, k, v = (i[n].requires_grad_() for n in "qkv")
            out = ops.FlashAttentionBSHD.apply(q, k.expand(B, L, C), v.expand(B, L, C), H, d ** -0.5)
            return [out] + grads([(out, i["go"])], (q, k, v))
        case(f"FlashAttentionBSHD-{'shared' if shared else 'per-image'}-{B}x{H}x{S}x{L}x{d}", mkb, runb,
             kernels=["skp_attn_fwd_bshd", "skp_attn_bwd_flash_bshd"])

    def run_heads(ops, i, g):
        with torch.no_grad():
            out = ops.attention_heads(i["q"], i["k"], i["v"], 3, 80 ** -0.5)
        assert out is not None
        return [out]
    case("attention_heads-nograd-d80", lambda: dict(q=rnd(168, 2, 64, 240), k=rnd(169, 2, 77, 240),
                                                     v=rnd(170, 2, 77, 240)),
         run_heads, kernels=["skp_attn_fwd_bshd"])


_attention_cases()


# =========================================================================================== convolutions
def _conv_in(B, C, K, H, W, bias=True, res=True, seed=180):
    def mk():
        d = dict(x=rnd(seed, B, C, H, W), w=rnd(seed + 1, K, C, 3, 3, scale=1 / (3 * C ** 0.5)),
                 go=rnd(seed + 2, B, K, H, W))
        if bias:
            d["b"] = rnd(seed + 3, K)
        if res:
            d["r"] = rnd(seed + 4, B, K, H, W)
        return d
    return mk


def _conv_cases():
    def parts_of(ops, y, gnp):
        """The GroupNorm statistics partials the convolution left on ``y`` as one more result; ``gnp``
        says whether this case's kernel writes them."""
        parts = ops._gn_parts_of(y)
        assert (parts is not None) == gnp, f"GroupNorm partials on the output: {parts is not None}, expected {gnp}"
        return [] if parts is None else [parts[0]]

    def fwd(gnp=False):
        def run(ops, i, g):
            with torch.no_grad():
                y = ops.conv3x3(i["x"], i["w"], i.get("b"), i.get("r"))
            return [y] + parts_of(ops, y, gnp)
        return run

    def fwd_bwd(gnp=False):
        def run(ops, i, g):
            x = i["x"].requires_grad_()
            y = ops.conv3x3(x, i["w"], i.get("b"), i.get("r"))
            return [y] + grads([(y, i["go"])], (x,)) + parts_of(ops, y, gnp)
        return run

    for B, C, K, H, W in ((2, 4, 32, 20, 20), (1, 32, 96, 12, 28)):
        case(f"conv3x3-v1-{B}x{C}x{K}x{H}x{W}", _conv_in(B, C, K, H, W), fwd(), patch=FUSED_CONV,
             kernels=["skp_wino_weights", "skp_conv3x3_wino"])
    # (2, 8, 32, 16, 16) is not a skp_conv3x3_wino2 shape (16 × 16 images go four at a time,
    # ops._wino_v2): the nearest one it takes is batch 4
    case("conv3x3-v2-4x8x32x16x16", _conv_in(4, 8, 32, 16, 16), fwd(), patch=FUSED_CONV,
         kernels=["skp_wino2_weights", "skp_conv3x3_wino2"])
    # H, W multiples of 32, one split: skp_conv3x3_wino2_gn leaves the partials
    case("conv3x3-v2-1x8x32x32x32", _conv_in(1, 8, 32, 32, 32), fwd(gnp=True), patch=FUSED_CONV,
         kernels=["skp_wino2_weights", "skp_conv3x3_wino2_gn"])

    def split(ops, i, g):
        assert ops._wino_plan(2, 256, 64, 16, 16)[1] > 1      # the ws slab is live
        return fwd_bwd()(ops, i, g)
    case("conv3x3-splitk-2x256x64x16x16", _conv_in(2, 256, 64, 16, 16), split, patch=FUSED_CONV,
         kernels=["skp_conv3x3_wino"])
    case("conv3x3-wide-3x64x192x4x12", _conv_in(3, 64, 192, 4, 12), fwd(), patch=FUSED_CONV, kernels=["skp_conv3x3_wino"])
    case("conv3x3-c3-zero-padded-2x3x32x20x20", _conv_in(2, 3, 32, 20, 20, res=False), fwd(), patch=FUSED_CONV,
         kernels=["skp_conv3x3_wino"])
    case("conv3x3-input-gradient-1x32x64x12x20", _conv_in(1, 32, 64, 12, 20, bias=False, res=False), fwd_bwd(),
         patch=FUSED_CONV, kernels=["skp_conv3x3_wino"])

    # the Winograd-GEMM form: the smallest channel counts _wino_gemm_ok takes (256 -> 256) at 16 × 16,
    # 16 tiles per image, where the output transform can leave the GroupNorm partials (P = 16)
    for gn in (True, False):
        case(f"conv3x3-wino-gemm-1x256x256x16x16-gnp{int(gn)}", _conv_in(1, 256, 256, 16, 16), fwd_bwd(gnp=gn),
             patch=dict(WINO_MIN_WORKGROUPS=1, WINO_GEMM_MAX_HW=1024, WINO_GEMM_MIN_CH=256, GN_EPI=gn),
             kernels=["skp_wino_in_transform", "skp_wino_out_transform_kt"])

    def s2(ops, i, g):
        with torch.no_grad():
            return [ops.conv3x3_s2(i["x"], i["w"], i.get("b"))]
    case("conv3x3_s2-1x4x32x32x32", _conv_in(1, 4, 32, 32, 32, res=False), s2,
         patch=dict(WINO_S2_MIN_PIXELS=1), kernels=["skp_wino2s2_weights", "skp_conv3x3s2_f2"])
    case("conv3x3_s2-1x32x32x32x32-nsplit2", _conv_in(1, 32, 32, 32, 32, res=False), s2,
         patch=dict(WINO_S2_MIN_PIXELS=1, WINO_NSPLIT_FORCE=2), kernels=["skp_wino2s2_weights", "skp_conv3x3s2_f2"])

    for B, C, K, H, W, G, force in ((1, 8, 32, 32, 32, 4, 0), (2, 12, 32, 64, 32, 4, 0), (1, 8, 32, 32, 32, 4, 2)):
        def mk(B=B, C=C, K=K, H=H, W=W):
            d = _conv_in(B, C, K, H, W, seed=190)()
            d.update(gamma=1 + rnd(196, C, scale=0.2), beta=rnd(197, C, scale=0.2), shift=rnd(198, B, C, scale=0.5))
            return d

        def run(ops, i, g, G=G, force=force):
            with torch.no_grad():
                y = ops.gn_conv3x3(i["x"], i["gamma"], i["beta"], G, 1e-6, True, i["shift"], i["w"], i["b"], i["r"])
            parts = ops._gn_parts_of(y)
            assert (parts is None) == bool(force)      # the gnp partials ride on an unsplit output
            return [y] + ([] if parts is None else [parts[0]])
        case(f"gn_conv3x3-{B}x{C}x{K}x{H}x{W}" + (f"-nsplit{force}" if force else ""), mk, run,
             patch=dict(FUSED_CONV, WINO_NSPLIT_FORCE=force),
             kernels=["skp_groupnorm_stats", "skp_wino2_vtransform_gn", "skp_conv3x3_wino2_v_gn"])


_conv_cases()


# =========================================================================================== render
def _render_cases():
    case("map_range-3x7x9", lambda: dict(maps=rnd(200, 3, 7, 9, scale=3.0)),
         lambda ops, i, g: [ops.map_range(i["maps"])], kernels=["skp_map_range"])

    name = min(render_ref.CASES, key=lambda n: (render_ref.CASES[n]["H"], n))    # g_h10_…: 10 × 10 images

    def mk():
        from stablekeypoints_amd import ops
        lut = ops.fallback_lut().numpy()
        c = render_ref.make_case(name, lut)
        return dict(images=T(c["images"]), maps=T(c["maps"]), points=T(c["points"]), lut=T(lut),
                    colors=torch.from_numpy(render_ref.COLORS).to(DEV))

    def run(ops, i, g):
        spec = render_ref.CASES[name]
        return [ops.render_sheet(i["images"], i["maps"], i["points"], rows=render_ref.ROWS, cols=render_ref.COLS,
                                 downscale=spec["f"], pad=spec["pad"], alpha=render_ref.ALPHA, radius=render_ref.RADIUS,
                                 colors=i["colors"], lut=i["lut"])]
    case(f"render_sheet-{name}", mk, run, kernels=["skp_map_range", "skp_render_sheet"])


_render_cases()


# =========================================================================================== TTA
def _tta_cases():
    fns = dict(tta_reduce=lambda ops, m, th, avg: ops.tta_reduce(m, th, return_avg=avg),
               tta_reduce_scored=lambda ops, m, th, avg: ops.tta_reduce_scored(m, th, distance=5, return_avg=avg),
               tta_reduce_peaks=lambda ops, m, th, avg: ops.tta_reduce_peaks(m, th, 3, return_avg=avg),
               tta_reduce_entropy=lambda ops, m, th, avg: ops.tta_reduce_entropy(m, th, scale=1.0, return_avg=avg))
    for shape in tta_ref.SHAPES[:2]:
        def mk(shape=shape):
            # special=False: every token finite (skp.h leaves a NaN / inf token's scores unspecified)
            maps, th, _ = tta_ref.make_case(shape, special=False)
            return dict(maps=T(maps), th=T(th))
        for op, fn in fns.items():
            for avg in (False, True):
                def run(ops, i, g, fn=fn, avg=avg):
                    res = fn(ops, i["maps"], i["th"], avg)
                    assert (res[-1] is not None) == avg
                    return list(res)
                case(f"{op}-{'x'.join(map(str, shape))}-avg{int(avg)}", mk, run, kernels=[f"skp_{op}"])


_tta_cases()


# =========================================================================================== the test
def _flat(v):
    if v is None:
        return []
    if isinstance(v, torch.Tensor):
        return [v]
    return [t for x in v for t in _flat(x)]


def _clone(inp):
    return {k: ([t.clone() for t in v] if isinstance(v, (list, tuple)) else v.clone()) for k, v in inp.items()}


def _one_run(ops, c, inp, poison, names):
    """One invocation on fresh clones of the inputs -> (results, GuardedAlloc or None).  Asserts the
    inputs came back bit-unchanged."""
    mine = _clone(inp)
    del names[:]
    if poison is None:
        g, res = None, c.run(ops, mine, None)
    else:
        with GuardedAlloc(poison, "cuda", op=c.name, caches=[(ops, "_TTA_WS"), (ops, "_WINO_U")]) as g:
            res = c.run(ops, mine, g)
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    if c.owns_no_buffer:
        assert not names, f"{c.name}: expected no libskp call, got {sorted(set(names))}"
    missing = [k for k in c.kernels if k not in names]
    assert not missing, f"{c.name}: expected HIP entry points {missing} were not called (called: {sorted(set(names))})"
    for k, v in inp.items():
        if k in c.mutates:
            continue
        for j, (a, b) in enumerate(zip(_flat(v), _flat(mine[k]))):
            assert bit_equal(a, b), f"{c.name}: input {k}[{j}] was modified (poison {poison})"
    res = list(res)
    part = list(c.defined(res)) if c.defined is not None else res
    if g is not None:      # the results really are the poisoned buffers: at least one lies inside a guarded allocation
        spans = [(r.buf.data_ptr() + g.guard, r.buf.data_ptr() + g.guard + r.nbytes) for r in g.records]
        g.result_inside = any(lo <= t.data_ptr() < hi for t in part if t is not None and t.numel() for lo, hi in spans)
    return [None if t is None else t.detach().clone() for t in part], g


def _agree(c, name_a, a, name_b, b):
    assert len(a) == len(b), f"{c.name}: {len(a)} results under {name_a}, {len(b)} under {name_b}"
    for j, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), f"{c.name}: result {j} is None under one of {name_a} / {name_b}"
        if x is None:
            continue
        assert x.shape == y.shape and x.dtype == y.dtype, f"{c.name}: result {j} {x.shape} vs {y.shape}"
        if j not in c.inexact:
            if not bit_equal(x, y):
                diff = (x.reshape(-1).cpu().view(torch.uint8).reshape(x.numel(), -1)
                        != y.reshape(-1).cpu().view(torch.uint8).reshape(y.numel(), -1)).any(dim=1).nonzero().reshape(-1)
                first = int(diff[0])
                raise AssertionError(
                    f"{c.name}: result {j} {tuple(x.shape)} {x.dtype} differs between {name_a} and {name_b} in "
                    f"{diff.numel()} elements, first at flat index {first}: {x.reshape(-1)[first].item()!r} vs "
                    f"{y.reshape(-1)[first].item()!r}")
        else:
            for nm, t in ((name_a, x), (name_b, y)):
                assert torch.isfinite(t).all() and float(t.abs().max()) <= 1e30, \
                    f"{c.name}: result {j} under {nm} holds a NaN or a magnitude above 1e30"
            scale = max(float(x.abs().max()), float(y.abs().max()))
            err = float((x.double() - y.double()).abs().max())
            assert err <= 1e-6 * scale, f"{c.name}: result {j} differs by {err:.3e} (largest magnitude {scale:.3e}) " \
                                        f"between {name_a} and {name_b}"


@pytest.mark.parametrize("c", CASES)
def test_memory_contract(c, monkeypatch):
    from stablekeypoints_amd import ops
    for k, v in c.patch.items():
        monkeypatch.setattr(ops, k, v)
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    inp = c.make()
    runs = {}
    try:
        base, _ = _one_run(ops, c, inp, None, names)
        for poison in POISONS:
            runs[poison] = _one_run(ops, c, inp, poison, names)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # the device is in an error state: nothing that follows in this process would mean anything
            pytest.exit(f"{c.name}: GPU fault, session ended: {e}", returncode=3)
        raise

    reports = "\n".join(g.report() for _, g in runs.values())
    print(reports)
    for poison, (_, g) in runs.items():
        v = g.violations()
        assert not v, "guard bytes changed:\n" + "\n".join(v) + "\n" + reports
        assert not g.passed_on("cuda"), f"{c.name}: device buffers passed through unguarded\n" + reports
    (ra, _), (rb, _) = runs[POISONS[0]], runs[POISONS[1]]
    _agree(c, "poison 0xFF", ra, "poison 0x7F", rb)
    _agree(c, "the plain run", base, "poison 0xFF", ra)
    _agree(c, "the plain run", base, "poison 0x7F", rb)
    for poison, (_, g) in runs.items():
        if c.owns_no_buffer:
            assert not g.records and not g.passed, f"{c.name}: expected no buffer of ops' making\n" + reports
            continue
        assert g.records, f"{c.name}: no allocation was guarded\n" + reports
        assert g.result_inside == c.results_guarded, \
            f"{c.name}: a result inside a guarded allocation: {g.result_inside}, expected {c.results_guarded}\n" + reports


def test_negative_control_on_the_device():
    """A float written just past a guarded tensor's payload, with torch indexing into the backing
    buffer (allocated memory), is reported."""
    with GuardedAlloc(0xFF, "cuda", op="control") as g:
        t = torch.empty(5, 7, device=DEV)
        t.zero_()
    assert g.violations() == [] and len(g.records) == 1
    r = g.records[0]
    assert t.data_ptr() == r.buf.data_ptr() + g.guard and r.nbytes == 5 * 7 * 4
    r.buf[g.guard + r.nbytes:g.guard + r.nbytes + 4].view(F32)[0] = 1.0
    v = g.violations()
    assert len(v) == 1 and "back guard" in v[0] and "offset +0 from the payload's end" in v[0] and "(5, 7)" in v[0], v
    r.buf[g.guard - 4:g.guard].view(F32)[0] = 1.0
    assert any("front guard" in m and "offset -4" in m for m in g.violations())
