"""HIP kernels (through the C ABI) vs the CPU oracle and the reference's golden vectors.

Tolerances (stated per test): index/argmax outputs bit-exact; fp32 maps/losses/grads
within 1e-4 (north_star) — most are far tighter.
"""
import numpy as np
import pytest
import torch

import recipes
from conftest import load_golden
from oracle import skp_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def T(a, **kw):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, **kw)


def N(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- MFMA GEMM
@pytest.mark.parametrize("Z,M,Nn,K", [(1, 32, 32, 2), (8, 256, 500, 160), (8, 1024, 500, 80), (3, 37, 53, 19)])
def test_bgemm_matches_fp64(Z, M, Nn, K):
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(M + Nn + K)
    a = torch.randn(Z, M, K, generator=g)
    b = torch.randn(Z, K, Nn, generator=g)
    out = ops.bgemm(a.to(DEV), b.to(DEV), alpha=0.5)
    ref = 0.5 * (a.double() @ b.double())
    assert torch.allclose(out.cpu().double(), ref, atol=1e-4, rtol=1e-5)
    # transposed operand views (strided, as used for q kᵀ and dzᵀ q)
    out2 = ops.bgemm(a.to(DEV), b.transpose(1, 2).contiguous().to(DEV).transpose(1, 2))
    assert torch.allclose(out2.cpu().double(), ref * 2, atol=1e-4, rtol=1e-5)


def _layouts(x):
    """x (Z, R, C) as three device views with equal values: contiguous, transposed storage
    (unit stride along the other axis) and a generic strided view (no unit stride)."""
    d = x.to(DEV)
    t = x.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    big = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], device=DEV)
    big[:, :, ::2] = d
    return {"contig": d, "trans": t, "strided": big[:, :, ::2]}


@pytest.mark.parametrize("Z,M,Nn,K", [(2, 70, 45, 37), (64, 256, 500, 160)])
def test_bgemm_all_operand_layouts_accumulate_shared_batch(Z, M, Nn, K):
    """Every operand layout pair the loader distinguishes (k unit stride, m/n unit stride,
    generic), accumulate=True, and a stride-0 batch operand (the shared token embedding's
    projected keys); (64, 256, 500, 160) is the bench's q kᵀ, 2048 tiles over a persistent
    grid of 1024 workgroups (several tiles per workgroup, pipeline across tile boundaries)."""
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(Z + M + K)
    a = torch.randn(Z, M, K, generator=g)
    b = torch.randn(Z, K, Nn, generator=g)
    ref = (a.double() @ b.double())
    for na, av in _layouts(a).items():
        for nb, bv in _layouts(b).items():
            out = ops.bgemm(av, bv, alpha=0.25)
            err = (out.cpu().double() - 0.25 * ref).abs().max().item()
            assert err < 1e-4, (na, nb, err)
    c0 = torch.randn(Z, M, Nn, generator=g)
    out = c0.to(DEV)
    ops.bgemm(a.to(DEV), b.to(DEV), alpha=2.0, out=out, accumulate=True)
    assert torch.allclose(out.cpu().double(), c0.double() + 2 * ref, atol=2e-4, rtol=1e-5)
    b1 = b[:1]
    shared = ops.bgemm(a.to(DEV), b1.to(DEV).expand(Z, K, Nn))
    assert torch.allclose(shared.cpu().double(), a.double() @ b1.double(), atol=1e-4, rtol=1e-5)


def test_bgemm_layout_identity_asymmetric():
    from stablekeypoints_amd import ops
    a = torch.eye(40).unsqueeze(0)
    b = torch.arange(40 * 33, dtype=torch.float32).reshape(1, 40, 33)
    out = ops.bgemm(a.to(DEV), b.to(DEV))
    assert torch.equal(out.cpu(), b)


# ----------------------------------------------------------------------------- A1 capture
@pytest.mark.parametrize("H,s,R,Nn", [(8, 4, 32, 16), (8, 8, 32, 16), (2, 16, 128, 500), (2, 32, 128, 500),
                                      (3, 5, 13, 70), (1, 16, 128, 1), (1, 16, 256, 40), (1, 8, 32, 1000),
                                      (2, 1, 8, 20), (1, 32, 16, 9), (1, 4, 16, 256), (1, 4, 16, 257), (1, 4, 16, 512),
                                      (1, 4, 16, 513), (1, 4, 16, 1024)])
def test_capture_fwd_vs_oracle(H, s, R, Nn):
    """Includes R=256 (the reference's default feature_upsample_res), N=1000 (its default token
    count, two tokens per lane), a 1×1 low-res layer, a downsampling R < s, and both ends of every
    token width (1, 2, 4 quads per lane: N up to 256, 512, 1024)."""
    from stablekeypoints_amd import ops
    z = recipes.random_logits(H * 1000 + s, (H, s * s, Nn), scale=3.0)
    got = N(ops.capture_attn(T(z), s, R))
    ref = O.capture_fwd(z, s, R)
    # fp32 reordering: |δattn| ≈ attn·|δz| with |z| up to ~15 here
    assert np.abs(got - ref).max() < 1e-5
    assert np.allclose(got.sum(-1), 1.0, atol=1e-5)


@pytest.mark.parametrize("H,s,R,Nn", [(8, 4, 32, 16), (2, 16, 128, 500), (2, 32, 128, 300), (3, 5, 13, 70),
                                      (1, 16, 256, 40), (1, 8, 32, 1000), (2, 1, 8, 20), (1, 32, 16, 9),
                                      (1, 4, 16, 512), (1, 4, 16, 513), (1, 4, 16, 1024)])   # 1 | 2 tokens per thread
def test_capture_bwd_dense_and_broadcast(H, s, R, Nn):
    from stablekeypoints_amd import ops
    z = recipes.random_logits(7 + s, (H, s * s, Nn), scale=2.0)
    g = recipes.random_logits(9 + s, (H, R * R, Nn))
    got = N(ops.capture_bwd(T(z), s, R, T(g)))
    ref = O.capture_bwd(z, s, R, g)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    # broadcast gradient: the layer-mean backward of collect_maps (stride-0 over heads, token-major)
    dmap = recipes.random_logits(11 + s, (Nn, R * R))
    gb = torch.as_tensor(dmap, device=DEV).t().unsqueeze(0).expand(H, R * R, Nn)
    got_b = N(ops.capture_bwd(T(z), s, R, gb))
    ref_b = O.capture_bwd(z, s, R, np.broadcast_to(dmap.T[None], (H, R * R, Nn)).astype(np.float32))
    assert np.abs(got_b - ref_b).max() < 1e-4 * max(1.0, np.abs(ref_b).max())


# ----------------------------------------------------------------------------- A3 aggregate
def test_aggregate_variants_vs_oracle():
    from stablekeypoints_amd import ops
    layers = [recipes.uniform(20 + i, (8, 32 * 32, 50)) for i in range(4)]
    tl = [T(a) for a in layers]
    assert np.allclose(N(ops.aggregate(tl)), O.collect_maps(layers), atol=1e-6)
    assert np.allclose(N(ops.aggregate(tl[:3])), O.collect_maps(layers[:3], layers=(0, 1, 2)), atol=1e-6)
    idx = np.array([5, 0, 49, 5])
    got = N(ops.aggregate(tl, indices=torch.as_tensor(idx), upsample_res=80))
    ref = O.collect_maps(layers, indices=idx, upsample_res=80)
    assert np.allclose(got, ref, atol=1e-6)
    # unaligned token count (scalar path)
    odd = [recipes.uniform(40 + i, (2, 16 * 16, 37)) for i in range(2)]
    assert np.allclose(N(ops.aggregate([T(a) for a in odd])), O.collect_maps(odd, layers=(0, 1)), atol=1e-6)


def test_aggregate_full_shape_properties():
    """N=500, R=128, 4 layers × 8 heads: every pixel's token distribution sums to 1."""
    from stablekeypoints_amd import ops
    zs = [recipes.random_logits(60 + i, (8, s * s, 500), scale=2.0) for i, s in enumerate((16, 16, 16, 32))]
    attn = [ops.capture_attn(T(z), s, 128) for z, s in zip(zs, (16, 16, 16, 32))]
    m = N(ops.aggregate(attn))
    assert m.shape == (500, 128, 128)
    assert np.allclose(m.sum(0), 1.0, atol=1e-4)
    ref = O.collect_maps([O.capture_fwd(z, s, 128) for z, s in zip(zs, (16, 16, 16, 32))])
    assert np.abs(m - ref).max() < 1e-6


# ----------------------------------------------------------------------------- A4-A7
def test_argmax_family_vs_golden():
    from stablekeypoints_amd import ops
    g = load_golden("argmax")
    assert np.array_equal(N(ops.find_max_pixel(T(g["edge"]))), g["edge_max"])
    assert np.array_equal(N(ops.find_k_max_pixels(T(g["edge"]), 3)), g["edge_k3"], equal_nan=True)
    assert np.array_equal(N(ops.find_k_max_pixels(T(g["maps32"]), 3)), g["maps32_k3"])
    pt = ops.find_max_pixel(T(g["maps32"]))
    assert np.array_equal(N(ops.mask_radius(T(g["maps32"]), pt, 0.05 * 32 * 3)), g["maps32_mask"])
    wa = T(g["maps32"])
    pos = ops.pixel_from_weighted_avg(wa, 5)
    assert np.allclose(N(pos), g["maps32_wavg"], atol=1e-5)
    assert np.array_equal(N(wa), g["maps32_wavg_mutated"])
    assert np.allclose(N(ops.pixel_from_weighted_avg(T(g["maps32"]), -1)), g["maps32_wavg_nodist"], atol=1e-4)
    big = recipes.attention_like_maps(12, 10, 512)
    assert recipes.sha256(big) == str(g["maps512_sha"])
    assert np.array_equal(N(ops.find_max_pixel(T(big))), g["maps512_max"])
    assert np.allclose(N(ops.pixel_from_weighted_avg(T(big))), g["maps512_wavg"], atol=1e-4)


def test_argmax_random_ties_nan_bitexact():
    from stablekeypoints_amd import ops
    rng = np.random.default_rng(5)
    m = rng.integers(0, 4, (64, 37, 29)).astype(np.float32)     # heavy ties
    m[3, 10, 10] = np.nan
    m[7, 0, 0] = np.nan
    m[7, 5, 5] = np.nan
    m[9] = -np.inf
    assert np.array_equal(N(ops.find_max_pixel(T(m))), O.find_max_pixel(m))
    assert np.array_equal(N(ops.find_k_max_pixels(T(m), 4)), O.find_k_max_pixels(m, 4), equal_nan=True)


def test_gaussian_targets_vs_golden():
    from stablekeypoints_amd import ops
    g = load_golden("gaussian")
    for size, sigma in ((32, 2.0), (128, 2.0), (20, 3.0)):
        assert np.allclose(N(ops.gaussian_circles(T(g["pos"]), size, sigma)), g[f"circles_{size}_{sigma}"], atol=1e-6)


# ----------------------------------------------------------------------------- A8-A10
def test_selection_vs_golden_full_shape():
    from stablekeypoints_amd import ops
    g = load_golden("select")
    maps = recipes.attention_like_maps(31, 500, 128)
    maps_t = recipes.attention_like_maps(32, 500, 128)
    cand = ops.find_top_k_gaussian(T(maps), 25, sigma=2.0)
    assert np.array_equal(N(cand), g["topk_gauss25"])
    assert np.array_equal(N(ops.find_top_k_gaussian(T(maps), 25, sigma=2.0, num_subjects=2)), g["topk_gauss25_s2"])
    assert np.array_equal(N(ops.entropy_sort(T(maps * 100.0), 25)), g["entropy25_sharp"])
    sel, n = ops.furthest_point_sampling(T(maps_t), 10, cand)
    assert int(n.item()) == 10 and np.array_equal(N(sel), g["fps10"])
    sel2, _ = ops.furthest_point_sampling(T(maps), 10, cand)
    assert np.array_equal(N(sel2), g["fps10_same"])


@pytest.mark.parametrize("num_subjects", [1, 2])
def test_selection_batched_equals_per_image(num_subjects):
    """skp_topk_gaussian_batch / skp_fps_batch (one launch over the images of a pass) select what
    the per-image calls select, image by image; image 0 carries the reference golden's maps."""
    from stablekeypoints_amd import ops
    g = load_golden("select")
    maps = np.stack([recipes.attention_like_maps(31, 500, 128)] +
                    [recipes.attention_like_maps(40 + i, 500, 128) for i in range(3)])
    maps_t = np.stack([recipes.attention_like_maps(32, 500, 128)] +
                      [recipes.attention_like_maps(50 + i, 500, 128) for i in range(3)])
    cand = ops.find_top_k_gaussian_batch(T(maps), 25, sigma=2.0, num_subjects=num_subjects)
    for i in range(4):
        one = ops.find_top_k_gaussian(T(maps[i]), 25, sigma=2.0, num_subjects=num_subjects)
        assert torch.equal(cand[i], one)
    gold = g["topk_gauss25"] if num_subjects == 1 else g["topk_gauss25_s2"]
    assert np.array_equal(N(cand[0]), gold)
    sel, n = ops.furthest_point_sampling_batch(T(maps_t), 10, cand)
    assert N(n).tolist() == [10] * 4
    for i in range(4):
        one, _ = ops.furthest_point_sampling(T(maps_t[i]), 10, cand[i])
        assert torch.equal(sel[i], one)
    if num_subjects == 1:
        assert np.array_equal(N(sel[0]), g["fps10"])


@pytest.mark.parametrize("nb,Tn,top_k", [(4, 500, 25), (1, 1, 1), (2, 8192, 8192), (3, 777, 100), (2, 64, 64)])
def test_topk_keys_rank_kernel_vs_stable_argsort(nb, Tn, top_k):
    """skp_topk_keys (the ranking kernel: out[rank_i] = i) against numpy's stable ascending argsort
    — NaN last, ties by index, as the r04 bitonic sort (key_less) — on keys with many exact ties,
    NaNs and ±inf: bit-exact indices (torch.argsort(keys)[:k], ptp_utils.py:110-112, 185)."""
    import ctypes
    from stablekeypoints_amd._lib import call, ptr, stream
    rng = np.random.default_rng(Tn + top_k)
    keys = np.round(rng.standard_normal((nb, Tn)) * 4) / 4   # coarse: many exact ties
    keys[:, ::17] = np.nan
    keys[:, 5::23] = np.inf
    keys[:, 7::29] = -np.inf
    out = torch.full((nb, top_k), -7, dtype=torch.int64, device=DEV)
    call("skp_topk_keys", ptr(T(keys)), nb, Tn, top_k, ptr(out), stream(DEV))
    torch.cuda.synchronize()
    ref = np.argsort(keys, axis=1, kind="stable")[:, :top_k]
    assert np.array_equal(N(out), ref)


@pytest.mark.parametrize("nb,Tn,R,n_cand,top_k", [(4, 500, 128, 25, 10), (3, 129, 32, 25, 10), (2, 37, 64, 37, 5),
                                                  (1, 500, 256, 25, 10)])
def test_fps_keys_batch_equals_rank_then_fps(nb, Tn, R, n_cand, top_k):
    """r06 selection chain: ops.gaussian_fps_batch — KL keys, then the ranking and
    the candidates' argmax in ONE launch (skp_fps_keys_batch), then FPS — selects exactly what the
    r05 chain (find_top_k_gaussian_batch's KL + rank launches, furthest_point_sampling_batch's argmax +
    FPS launches) selects: picks, counts and candidates, with FPS on different maps than the ranking
    (the warps', optimize.py:403-410), duplicated rows (equal keys: ties by index), a NaN row (last)
    and a flat row (argmax ties); and the entropy strategy's keys through the same launch."""
    from stablekeypoints_amd import ops
    maps = np.stack([recipes.attention_like_maps(400 + i, Tn, R) for i in range(nb)]).astype(np.float32)
    maps_t = np.stack([recipes.attention_like_maps(500 + i, Tn, R) for i in range(nb)]).astype(np.float32)
    maps[:, 3] = maps[:, 1]
    maps[:, min(10, Tn - 1)] = np.nan
    maps_t[:, 2] = 0.5
    m, mt = T(maps), T(maps_t)
    sel, n, cand = ops.gaussian_fps_batch(m, mt, n_cand, top_k, sigma=2.0)
    cand0 = ops.find_top_k_gaussian_batch(m, n_cand, sigma=2.0)
    sel0, n0 = ops.furthest_point_sampling_batch(mt, top_k, cand0)
    assert torch.equal(cand, cand0) and torch.equal(sel, sel0) and torch.equal(n, n0)
    ent = np.abs(maps_t) * 50.0   # finite rows for the entropies
    e = T(ent)
    sel_e, n_e, cand_e = ops.fps_from_keys_batch(ops.entropy_keys_batch(e), e, n_cand, top_k)
    cand_e0 = ops.entropy_sort_batch(e, n_cand)
    sel_e0, n_e0 = ops.furthest_point_sampling_batch(e, top_k, cand_e0)
    assert torch.equal(cand_e, cand_e0) and torch.equal(sel_e, sel_e0) and torch.equal(n_e, n_e0)


@pytest.mark.parametrize("n_cand,top_k", [(25, 10), (64, 64), (80, 70), (2, 2)])
def test_fps_both_kernels_vs_oracle(n_cand, top_k):
    """skp_fps: the one-lane-per-candidate kernel (r06, C ≤ 64 and top_k ≤ 64: running minima in
    registers) and the LDS kernel it falls back to (C = 80) against the oracle's FPS
    (ptp_utils.py:115-159): candidates with duplicated tokens, maps with tied argmax positions, all
    rounds run (top_k = C − duplicates) — bit-exact picks and counts."""
    from stablekeypoints_amd import ops
    rng = np.random.default_rng(n_cand * 100 + top_k)
    maps = rng.random((120, 24, 24), dtype=np.float32)
    maps[7] = maps[9]                       # tied positions
    maps[11, 3, 3] = maps[11].max() + 1.0   # edge-ish positions
    cand = rng.choice(120, size=n_cand, replace=False).astype(np.int64)
    if n_cand > 4:
        cand[3] = cand[1]                   # a duplicated token: skipped once selected
    sel, n = ops.furthest_point_sampling(T(maps), top_k, torch.from_numpy(cand).to(DEV))
    ref = O.furthest_point_sampling(maps, top_k, cand)
    k = int(n.item())
    assert k == len(ref) and np.array_equal(N(sel)[:k], ref)
    assert (N(sel)[k:] == -1).all()


def test_entropy_sort_batch_equals_per_image():
    """ops.entropy_sort_batch (the entropies of all images' rows in one launch, the per-image
    top-k in one skp_topk_keys launch: the batched `entropy` strategy of find_best_indices,
    keypoint_regressor.py:104-105) equals entropy_sort image by image; image 0 is the golden's."""
    from stablekeypoints_amd import ops
    g = load_golden("select")
    maps = np.stack([recipes.attention_like_maps(31, 500, 128) * 100.0] +
                    [recipes.attention_like_maps(80 + i, 500, 128) * 100.0 for i in range(2)]).astype(np.float32)
    got = ops.entropy_sort_batch(T(maps), 25)
    for i in range(3):
        assert torch.equal(got[i], ops.entropy_sort(T(maps[i]), 25))
    assert np.array_equal(N(got[0]), g["entropy25_sharp"])
    # find_best_indices' batched selection with the entropy strategy: candidates + FPS per image
    from stablekeypoints_amd import keypoint_regressor as kr
    sel, n = kr._select_stack(T(maps), 10, 25, "entropy", 2.0, 1)
    for i in range(3):
        one, k = ops.furthest_point_sampling(T(maps[i]), 10, ops.entropy_sort(T(maps[i]), 25))
        assert int(n[i]) == int(k) and torch.equal(sel[i, :int(k)], one[:int(k)])


@pytest.mark.parametrize("num_subjects", [1, 2])
def test_losses_batched_equal_per_image(num_subjects):
    """ops.sharpening_loss_batch / equivariance_loss_batch (one launch per direction for the pass's
    images) against the per-image losses: each image's loss and dA bit-identical, dAt (the
    warp adjoint scatters with atomics) within 1e-6 of its largest magnitude."""
    from stablekeypoints_amd import ops
    k, n = 4, 10
    A = T(np.stack([recipes.attention_like_maps(60 + i, n, 128) for i in range(k)]).reshape(k * n, 128, 128))
    At = T(np.stack([recipes.attention_like_maps(70 + i, n, 128) for i in range(k)]).reshape(k * n, 128, 128))
    th = torch.tensor([[[0.9, -0.1, 0.05], [0.12, 0.95, -0.2]], [[1.1, 0.0, 0.1], [0.0, 1.05, 0.0]],
                       [[0.97, 0.2, -0.15], [-0.2, 0.97, 0.1]], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]],
                      device=A.device)
    w = torch.tensor([1.0, -2.0, 0.5, 3.0], device=A.device)
    a1, at1 = A.clone().requires_grad_(), At.clone().requires_grad_()
    sh = ops.sharpening_loss_batch(a1, k, sigma=2.0, num_subjects=num_subjects)
    eq = ops.equivariance_loss_batch(a1, at1, th, k)
    ((sh + 1000.0 * eq) * w).sum().backward()
    for i in range(k):
        a2, at2 = A[i * n:(i + 1) * n].clone().requires_grad_(), At[i * n:(i + 1) * n].clone().requires_grad_()
        s2 = ops.sharpening_loss(a2, sigma=2.0, num_subjects=num_subjects)
        e2 = ops.equivariance_loss_single(a2, at2, th[i])
        ((s2 + 1000.0 * e2) * w[i]).backward()
        assert torch.equal(sh[i], s2) and torch.equal(eq[i], e2)
        assert torch.equal(a1.grad[i * n:(i + 1) * n], a2.grad)
        err = float((at1.grad[i * n:(i + 1) * n] - at2.grad).abs().max() / at2.grad.abs().max())
        assert err < 1e-6, err


@pytest.mark.parametrize("hw", [(64, 64), (90, 90), (128, 128), (256, 256)])
def test_topk_gaussian_window_kernel_vs_per_pixel(hw):
    """One subject on 16-B aligned rows takes the windowed KL kernel (skp_select.hip
    kl_gauss_win_kernel: one exp per pixel, the Gaussian and its logs over the argmax's window
    only); a misaligned copy of the same rows takes the per-pixel four-pass kernel.  Same
    ranking, KL within 1e-6 relative (fp32 rounding of the closed form), both within 1e-6 of the
    fp64 oracle.  Two subjects take the register-resident per-pixel kernel, bit-identical to the
    four-pass one.  (256, 256) = find_best_indices' upsample_res: the 1024-thread window form."""
    from stablekeypoints_amd import ops
    h, w = hw
    rng = np.random.default_rng(h)
    maps = rng.random((3, 40, h, w), dtype=np.float32) ** 8
    a = T(maps)
    buf = torch.empty(a.numel() + 1, device=a.device, dtype=torch.float32)
    mis = buf[1:].view_as(a)
    mis.copy_(a)
    for i in range(3):
        idx_r, kl_r = ops.find_top_k_gaussian(a[i], 12, sigma=2.0, return_kl=True)
        idx_m, kl_m = ops.find_top_k_gaussian(mis[i], 12, sigma=2.0, return_kl=True)
        assert torch.equal(idx_r, idx_m)
        assert torch.allclose(kl_r, kl_m, rtol=1e-6, atol=0), float((kl_r - kl_m).abs().max())
        if i == 0:
            ko = O.kl_to_gaussian(maps[0], 2.0)
            assert np.allclose(N(kl_r), ko, rtol=1e-6, atol=0)
        idx2, kl2 = ops.find_top_k_gaussian(a[i], 12, sigma=2.0, num_subjects=2, return_kl=True)
        idx2m, kl2m = ops.find_top_k_gaussian(mis[i], 12, sigma=2.0, num_subjects=2, return_kl=True)
        assert torch.equal(idx2, idx2m) and torch.allclose(kl2, kl2m, rtol=1e-12, atol=0)
    batch = ops.find_top_k_gaussian_batch(a, 12, sigma=2.0)
    for i in range(3):
        assert torch.equal(batch[i], ops.find_top_k_gaussian(a[i], 12, sigma=2.0))


@pytest.mark.parametrize("hw", [(128, 128), (64, 64), (88, 88)])   # square only: h != w raises (88² ≈ the former 96×80)
def test_topk_gaussian_streamed_kernel_vs_per_pixel(hw):
    """The streamed KL kernel (the default for 16-B aligned rows up to 128²: running max + rescaled
    exp sum, Σu as Σx − HW·max) against the per-pixel kernel (a misaligned copy of the same rows) with
    a NaN row, an all-equal row (argmax ties) and a row with +inf: identical selections, KL within
    1e-6 relative, NaN exactly where the per-pixel form gives NaN.  (r05 checked the streamed form
    against the held register form the same way; the held form now serves rows above 128² only.)"""
    from stablekeypoints_amd import ops
    h, w = hw
    rng = np.random.default_rng(h + w)
    maps = rng.random((2, 60, h, w), dtype=np.float32) ** 8
    maps[0, 5, 3, 7] = np.nan
    maps[0, 6] = 0.25
    maps[1, 9, h - 1, w - 1] = np.inf
    a = T(maps)
    buf = torch.empty(a.numel() + 1, device=a.device, dtype=torch.float32)
    mis = buf[1:].view_as(a)
    mis.copy_(a)
    for i in range(2):
        i1, k1 = ops.find_top_k_gaussian(a[i], 20, sigma=2.0, return_kl=True)
        i0, k0 = ops.find_top_k_gaussian(mis[i], 20, sigma=2.0, return_kl=True)
        assert torch.equal(i1, i0)
        n1, n0 = torch.isnan(k1), torch.isnan(k0)
        assert torch.equal(n1, n0)
        assert torch.allclose(k1[~n1], k0[~n0], rtol=1e-6, atol=0), float((k1[~n1] - k0[~n0]).abs().max())


def test_topk_gaussian_window_edges_and_sigma():
    """The window clipped at every border (argmax in corners and on edges), σ large enough that
    the window covers the whole row, and a non-default epsilon: KL within 1e-6 relative of the
    fp64 oracle and the same ranking."""
    from stablekeypoints_amd import ops
    rng = np.random.default_rng(9)
    maps = rng.random((24, 64, 64), dtype=np.float32) * 0.5
    spots = [(0, 0), (0, 63), (63, 0), (63, 63), (0, 30), (30, 0), (63, 30), (30, 63), (2, 2), (61, 5)]
    for t, (r, c) in enumerate(spots):
        maps[t, r, c] = 3.0
    for sigma, eps in ((2.0, 1e-5), (3.0, 1e-5), (9.0, 1e-5), (2.0, 1e-3)):
        idx, kl = ops.find_top_k_gaussian(T(maps), 24, sigma=sigma, epsilon=eps, return_kl=True)
        ko = O.kl_to_gaussian(maps, sigma, epsilon=eps)
        assert np.allclose(N(kl), ko, rtol=1e-6, atol=0), (sigma, eps, np.abs(N(kl) - ko).max())
        assert np.array_equal(N(idx), np.argsort(ko, kind="stable")), (sigma, eps)


def test_entropy_sort_raw_maps_vs_reference_ties():
    """entropy_sort on raw (near-uniform) maps (ptp_utils.py:165-187) against the reference's OWN
    fp32 entropies (recorded from the reference, tests/golden/entropy_ref.npz).  25/25 is
    unreachable by construction: the reference's 25th and 26th smallest fp32 entropies are the
    same float (asserted), and it keeps whichever torch.argsort's unspecified order among equal
    keys puts first.  skp_entropy_sort ranks by fp64-accumulated entropy (ties by token id).
    Recorded margin: at every position our token and the reference's have reference entropies
    within the reference's own fp32 rounding noise (max |H32 − H64| over the 500 tokens,
    2.25e-6), every token in only one of the two sets is tied with the reference's 25th value to
    that noise, and against the fp64 oracle the order differs only inside the kernel's own exp
    noise (1e-7)."""
    from stablekeypoints_amd import ops
    ge = load_golden("entropy_ref")
    h32, ref = ge["entropy_f32"], ge["entropy25"]
    maps = recipes.attention_like_maps(31, 500, 128)
    ours = N(ops.entropy_sort(T(maps), 25))
    h64 = O.entropy_values(maps)
    s = np.sort(h32)
    assert s[24] == s[25]
    noise = float(np.abs(h32 - h64).max())
    same_pos = int((ours == ref).sum())
    diff_set = set(ours.tolist()) ^ set(ref.tolist())
    d_ref = float(np.abs(h32[ours] - h32[ref]).max())
    orc = O.entropy_sort(maps, 25)
    d_orc = float(np.abs(h64[ours] - h64[orc]).max())
    print(f"\nentropy_sort on raw maps vs the reference: {same_pos}/25 same positions, "
          f"{25 - len(diff_set) // 2}/25 same tokens, max reference-entropy gap at any position {d_ref:.1e} "
          f"(noise {noise:.1e}); vs the fp64 oracle: {int((ours == orc).sum())}/25 positions, gap {d_orc:.1e}")
    assert noise < 2.5e-6
    assert d_ref <= noise
    assert all(abs(h32[t] - s[24]) <= noise for t in diff_set)
    assert d_orc <= 1e-7
    assert np.all(np.diff(h64[ours]) >= -1e-7)   # ascending up to the kernel's noise


def test_selection_small_and_ties_vs_golden():
    from stablekeypoints_amd import ops
    g = load_golden("select")
    c = ops.find_top_k_gaussian(T(g["maps_small"]), 12, sigma=2.0)
    assert np.array_equal(N(c), g["small_topk12"])
    sel, _ = ops.furthest_point_sampling(T(g["maps_small"]), 5, c)
    assert np.array_equal(N(sel), g["small_fps5"])
    sel, _ = ops.furthest_point_sampling(T(g["tie_maps"]), 4, torch.tensor([5, 2, 4, 0, 1]))
    assert np.array_equal(N(sel), g["tie_fps4"])


def test_kl_values_vs_oracle():
    from stablekeypoints_amd import ops
    maps = recipes.attention_like_maps(34, 64, 64)
    _, kl = ops.find_top_k_gaussian(T(maps), 10, sigma=2.0, return_kl=True)
    assert np.allclose(N(kl), O.kl_to_gaussian(maps, 2.0), rtol=1e-6, atol=1e-7)


# ----------------------------------------------------------------------------- A11/A12
def test_losses_vs_golden():
    from stablekeypoints_amd import ops
    g = load_golden("losses")
    for ns in (1, 2):
        A = T(g["A"]).requires_grad_(True)
        l = ops.sharpening_loss(A, 2.0, ns)
        l.backward()
        assert np.allclose(N(l), g[f"sharp_ns{ns}"], rtol=1e-5)
        assert np.allclose(N(A.grad), g[f"dA_sharp_ns{ns}"], atol=1e-9, rtol=1e-4)
    dw = float(np.abs(N(ops.affine_warp(T(g["img"]), T(g["theta"]))) - g["warped"]).max())
    assert dw <= 1e-6, dw   # torch-CPU grid rounding reproduced (tests/test_oracle_golden.py)
    ti = O.theta_inverse(g["theta"])
    A = T(g["A"]).requires_grad_(True)
    At = T(g["At"]).requires_grad_(True)
    l = ops.equivariance_loss_single(A, At, T(ti[1]))
    l.backward()
    print(f"\nwarp max|Δ| {dw:.1e}, equivariance loss rel {abs(float(l) / float(g['equiv']) - 1):.1e}")
    assert np.allclose(N(l), g["equiv"], rtol=1e-5)
    for ours, ref in ((N(A.grad), g["dA_equiv"]), (N(At.grad), g["dAt_equiv"])):
        assert np.abs(ours - ref).max() <= 1e-4 * np.abs(ref).max()


def test_random_affine_inverse_vs_reference():
    """RandomAffineWithInverse.inverse (invertable_transform.py:72-92) — the product's own path, θ⁻¹
    computed on this host (fp32 torch.inverse of the augmented 3×3, as the reference) and the GPU
    inverse warp — against what the reference recorded (theta_inv.npz at the training and TTA
    augmentation ranges; losses.npz inv_At, the reference's inverse warp of its 2 replicas' maps,
    optimize.py:159).  MKL's LU takes a CPU-dependent code path, so θ⁻¹ may differ in the last bits
    from the recording host (38 ulp measured on the GPU box in r04): bounded by absolute error
    ≤ 1e-6; the inverse-warped images and maps within 1e-5 (3.8e-6 measured in r04)."""
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    g = load_golden("losses")
    tr = RandomAffineWithInverse(degrees=15, scale=(0.8, 1.0), translate=(0.25, 0.25))
    gi = load_golden("theta_inv")
    dth, ulp, dimg = 0.0, 0.0, 0.0
    for name in ("train", "tta"):
        tr.last_params = {"theta": torch.from_numpy(gi[f"{name}_theta"])}
        ti = N(tr.theta_inverse())
        ref = gi[f"{name}_theta_inv"]
        dth = max(dth, float(np.abs(ti - ref).max()))
        ulp = max(ulp, float((np.abs(ti - ref) / np.spacing(np.abs(ref).astype(np.float32))).max()))
        out = N(tr.inverse(T(gi["img"])))
        dimg = max(dimg, float(np.abs(out - gi[f"{name}_inv_img"]).max()))
    tr.last_params = {"theta": torch.from_numpy(g["theta"])}
    inv_at = N(tr.inverse(T(np.repeat(g["At"][None], 2, 0))))
    dmap = float(np.abs(inv_at - g["inv_At"]).max())
    print(f"\nθ⁻¹ on this host vs the reference's: max|Δ| {dth:.1e} ({ulp:.0f} ulp); inverse warp vs the "
          f"reference: images max|Δ| {dimg:.1e}, maps (inv_At) max|Δ| {dmap:.1e}")
    assert dth <= 1e-6, dth
    assert dimg <= 1e-5, dimg
    assert dmap <= 1e-5, dmap


def test_affine_warp_adjoint():
    """<warp(x), y> == <x, warpᵀ(y)> (linearity/adjoint property at full image size)."""
    from stablekeypoints_amd import ops
    x = torch.rand(2, 3, 512, 512, device=DEV, requires_grad=True)
    th = torch.tensor([[[0.9, 0.1, 0.05], [-0.1, 0.9, -0.2]], [[0.8, -0.2, 0.2], [0.2, 0.8, 0.1]]], device=DEV)
    y = torch.rand(2, 3, 512, 512, device=DEV)
    out = ops.affine_warp(x, th)
    (out * y).sum().backward()
    lhs = (out.double() * y.double()).sum()
    rhs = (x.double() * x.grad.double()).sum()
    assert abs(float(lhs - rhs)) < 1e-6 * abs(float(lhs))


# ----------------------------------------------------------------------------- composed paths
def test_capture_hook_end_to_end_small():
    """register_attention_control + collect_maps + backward == reference (capture_small golden)."""
    from stablekeypoints_amd import ptp_utils, optimize
    from stablekeypoints_amd.sd.unet import CrossAttention
    g = load_golden("capture_small")
    R = int(g["R"])
    shapes = [(4, 64), (4, 64), (4, 64), (8, 32)]

    class Tree(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.up_blocks = torch.nn.ModuleList()
            for i, (s, c) in enumerate(shapes):
                m = CrossAttention(c, cross_attention_dim=24, heads=8, dim_head=c // 8)
                m.load_state_dict({k.split(".", 1)[1]: torch.from_numpy(g[k]) for k in g.files
                                   if k.startswith(f"w{i}.")})
                self.up_blocks.append(m)
    tree = Tree().to(DEV)
    ctl = ptp_utils.AttentionStore()
    ptp_utils.register_attention_control(tree, ctl, feature_upsample_res=R)
    xs = [T(g[f"x{i}"]).requires_grad_(True) for i in range(4)]
    ctx = T(g["ctx"]).requires_grad_(True)
    outs = [m(x, context=ctx) for m, x in zip(tree.up_blocks, xs)]
    for i in range(4):
        assert np.allclose(N(ctl.step_store["attn"][i]), g[f"attn{i}"], atol=1e-6)
        assert np.allclose(N(outs[i]), g[f"out{i}"], atol=1e-5)
    maps = optimize.collect_maps(ctl, upsample_res=-1, layers=[0, 1, 2, 3])
    assert np.allclose(N(maps), g["map"], atol=1e-6)
    (maps * T(g["wsel"])).sum().backward()
    for i in range(4):
        assert np.allclose(N(xs[i].grad), g[f"dx{i}"], atol=1e-5, rtol=1e-4)
    assert np.allclose(N(ctx.grad), g["dctx"], atol=1e-5, rtol=1e-4)


def test_token_opt_step_tiny_vs_reference():
    """One optimize.py:362-445 micro-iteration on the tiny SD-1.5-shaped model vs the reference."""
    from stablekeypoints_amd import optimize, ptp_utils
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    from stablekeypoints_amd.sd import build_sd15, TINY_CONFIG
    g = load_golden("step_tiny")
    R = int(g["R"])
    ldm = build_sd15(seed=0, config=TINY_CONFIG)
    psum = float(sum(p.double().sum() for p in list(ldm.unet.parameters()) + list(ldm.vae.parameters())))
    assert abs(psum - float(g["param_sum"])) < 1e-6, "tiny model regeneration differs from the golden's"
    ldm.to(DEV)
    noises = [T(g["noise0"]), T(g["noise1"])]
    inner = ldm.scheduler

    class Sched:
        timesteps = inner.timesteps

        def add_noise(self, x, noise, t):
            return inner.add_noise(x, noises.pop(0), t)
    ldm.scheduler = Sched()
    ctl = ptp_utils.AttentionStore(early_exit=True)
    ptp_utils.register_attention_control(ldm.unet, ctl, feature_upsample_res=R)
    controllers = {torch.device(DEV): ctl}
    ctx = T(g["ctx"]).requires_grad_(True)
    kw = dict(layers=[0, 1, 2, 3], upsample_res=-1, device=DEV, controllers=controllers)
    with torch.no_grad():
        lat0 = ptp_utils.image2latent(ldm, T(g["img"]), DEV)
    assert np.allclose(N(lat0), g["latent0"], atol=1e-4)
    Tr = RandomAffineWithInverse(degrees=15, scale=(0.8, 1.0), translate=(0.25, 0.25))
    timg = Tr(T(g["img"]), theta=torch.from_numpy(g["theta"]))
    # skp_affine_warp rounds the grid as torch-CPU does (fma(y, θ1, x·θ0) + θ2, the CPU sampler's
    # fma(g + 1, n/2, −0.5)): the reference's warp to 2 ulp
    dtimg = float(np.abs(N(timg) - g["timg"]).max())
    assert dtimg <= 1e-6, dtimg
    # The UNet passes start from the reference's latents (identical inputs): the VAE's conv
    # algorithms differ from torch-CPU's at ~1e-6, which is checked just above.
    maps = ptp_utils.run_and_find_attn(ldm, T(g["latent0"]), ctx, **kw)
    maps_t = ptp_utils.run_and_find_attn(ldm, T(g["latent1"]), ctx, **kw)
    assert np.allclose(N(maps[0]), g["map"], atol=1e-5)
    assert np.allclose(N(maps_t[0]), g["map_t"], atol=1e-5)
    cand = ptp_utils.find_top_k_gaussian(maps[0], 8, sigma=2.0)
    idx = ptp_utils.furthest_point_sampling(maps_t[0], 4, cand)
    assert np.array_equal(N(cand), g["cand"]) and np.array_equal(N(idx), g["idx"])
    sharp = optimize.sharpening_loss(maps[0][idx], sigma=2.0)
    eq = optimize.equivariance_loss(maps[0][idx], maps_t[0][idx][None], Tr, 0)
    loss = (eq * 1000.0 + sharp * 100.0) / 4
    loss.backward()
    rs, re = abs(float(sharp) / float(g["sharp"]) - 1), abs(float(eq) / float(g["eq"]) - 1)
    dc = N(ctx.grad)
    rg = float(np.linalg.norm(dc - g["dctx"]) / np.linalg.norm(g["dctx"]))
    print(f"\nstep vs reference: timg max|Δ| {dtimg:.1e}, sharp rel {rs:.1e}, eq rel {re:.1e}, "
          f"context.grad rel-L2 {rg:.1e}")
    assert rs <= 1e-4 and re <= 1e-4, (rs, re)   # north_star: losses within 1e-4
    assert rg <= 1e-4, rg
    assert np.allclose(dc, g["dctx"], rtol=1e-4, atol=1e-7)


# ----------------------------------------------------------------------------- fused per-image path
def test_capture_maps_per_image_fwd_bwd():
    """CaptureMaps (B=2 images × 8 heads, 4 layers) == per-image capture+aggregate, fwd and bwd."""
    from stablekeypoints_amd import ops
    B, H, R, Nn = 2, 8, 32, 40
    sizes = (4, 4, 4, 8)
    zs = [recipes.random_logits(80 + i, (B * H, s * s, Nn), scale=2.0) for i, s in enumerate(sizes)]
    zt = [T(z).requires_grad_(True) for z in zs]
    maps = ops.capture_maps(zt, sizes, B, R)
    attn = [O.capture_fwd(z, s, R) for z, s in zip(zs, sizes)]
    for b in range(B):
        ref = O.collect_maps([a[b * H:(b + 1) * H] for a in attn])
        assert np.abs(N(maps[b]) - ref).max() < 1e-6
    w = recipes.random_logits(90, (B, Nn, R, R))
    (maps * T(w)).sum().backward()
    for i, (z, s) in enumerate(zip(zs, sizes)):
        dattn = np.concatenate([O.collect_maps_bwd([(H, R * R, Nn)] * 4, w[b])[i] for b in range(B)])
        ref = O.capture_bwd(z, s, R, dattn)
        assert np.abs(N(zt[i].grad) - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


def _capture_maps_abi(zs, sizes, B, H, R, with_stats=True):
    """skp_capture_maps_fwd through the C ABI: maps (B, N, R, R) and per-layer stats."""
    import ctypes
    from stablekeypoints_amd._lib import call, ptr, stream
    L = len(zs)
    Nn = zs[0].shape[-1]
    maps = torch.full((B, Nn, R, R), float("nan"), device=DEV)
    stats = [torch.full((B * H, R * R, 2), float("nan"), device=DEV) for _ in range(L)]
    zp = (ctypes.c_void_p * L)(*[z.data_ptr() for z in zs])
    sp = (ctypes.c_int * L)(*sizes)
    stp = (ctypes.c_void_p * L)(*[st.data_ptr() for st in stats])
    call("skp_capture_maps_fwd", ctypes.cast(zp, ctypes.POINTER(ctypes.c_void_p)), sp, L, B, H, Nn, R, ptr(maps),
         ctypes.cast(stp, ctypes.POINTER(ctypes.c_void_p)) if with_stats else None, stream(zs[0].device))
    torch.cuda.synchronize()
    return maps, stats


@pytest.mark.parametrize("B,H,sizes,R,Nn", [(2, 8, (4, 4, 4, 8), 32, 40), (1, 3, (5, 3), 40, 37), (2, 2, (16, 32), 128, 1),
                                            (1, 2, (8,), 32, 1000), (3, 1, (1, 2), 8, 130), (1, 8, (16, 16, 16, 32), 128, 500),
                                            (1, 4, (7, 13), 100, 256), (1, 2, (6,), 72, 129), (1, 1, (12,), 24, 8),
                                            (1, 2, (32, 64), 128, 500), (1, 2, (9, 20), 31, 64)]
                         # both ends of every token width (1, 2, 4, 8, 16 quads per lane) not reached above
                         + [(1, 1, (4,), 16, n) for n in (65, 128, 257, 512, 513, 1024)])
def test_capture_maps_fwd_vs_oracle(B, H, sizes, R, Nn):
    """skp_capture_maps_fwd (fused capture + per-image layer/head mean) vs the oracle's
    capture_fwd + collect_maps per image (ptp_utils.py:508-538, optimize.py:27-79): maps within
    1e-6 absolute, every stats entry (row max, 1/Σ) within fp32 rounding of the oracle's row."""
    zs = [recipes.random_logits(300 + 7 * i + Nn, (B * H, s * s, Nn), scale=2.0) for i, s in enumerate(sizes)]
    maps, stats = _capture_maps_abi([T(z) for z in zs], list(sizes), B, H, R)
    m = N(maps)
    assert np.isfinite(m).all()
    for b in range(B):
        attn = [O.capture_fwd(z[b * H:(b + 1) * H], s, R) for z, s in zip(zs, sizes)]
        ref = O.collect_maps(attn)
        assert np.abs(m[b] - ref).max() < 1e-6, (b, np.abs(m[b] - ref).max())
    for z, s, st in zip(zs, sizes, stats):
        zu = O.resize(z.reshape(B * H, s, s, Nn).transpose(0, 3, 1, 2), R, "bicubic")
        zu = zu.transpose(0, 2, 3, 1).reshape(B * H, R * R, Nn).astype(np.float64)
        st = N(st).astype(np.float64)
        zmax = zu.max(-1)
        assert (np.abs(st[..., 0] - zmax) / np.maximum(1.0, np.abs(zmax))).max() < 4e-6   # fp32 rounding
        assert np.abs(st[..., 1] * np.exp(zu - st[..., :1]).sum(-1) - 1).max() < 2e-5


def test_capture_maps_fwd_equals_two_kernel_path_full_size():
    """At the bench shape (B=8 images × 8 heads, s = 16,16,16,32, R=128, N=500) the fused launch
    equals skp_capture_fwd + skp_aggregate per image (the r01 path, itself oracle-pinned) to
    1e-7 on the maps and to fp32 rounding on the stats; the backward fed with either stats agrees."""
    import ctypes
    from stablekeypoints_amd import ops
    from stablekeypoints_amd._lib import call, ptr, stream
    B, H, R, Nn, sizes = 8, 8, 128, 500, (16, 16, 16, 32)
    g = torch.Generator().manual_seed(5)
    zs = [(torch.randn(B * H, s * s, Nn, generator=g) * 3).to(DEV) for s in sizes]
    maps, stats = _capture_maps_abi(zs, list(sizes), B, H, R)
    RR = R * R
    ref = torch.empty(B, Nn, R, R, device=DEV)
    attn = []
    for z, s in zip(zs, sizes):
        a = torch.empty(B * H, RR, Nn, device=DEV)
        st = torch.empty(B * H, RR, 2, device=DEV)
        call("skp_capture_fwd", ptr(z), B * H, s, Nn, R, ptr(a), ptr(st), stream(z.device))
        attn.append((a, st))
    for b in range(B):
        arr = (ctypes.c_void_p * 4)(*[a.data_ptr() + b * H * RR * Nn * 4 for a, _ in attn])
        call("skp_aggregate", ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), 4, H, RR, Nn, None, Nn, ptr(ref[b]),
             stream(DEV))
    torch.cuda.synchronize()
    d = (maps - ref).abs().max().item()
    print(f"\nfused vs two-kernel maps: max|Δ| {d:.2e} (max {ref.max().item():.3e})")
    assert d < 1e-7
    for (a, st_ref), st in zip(attn, stats):
        # the row max of the same bicubic values, summed with and without FMA contraction
        assert ((st[..., 0] - st_ref[..., 0]).abs() / st_ref[..., 0].abs().clamp(min=1)).max().item() < 2e-6
        assert ((st[..., 1] - st_ref[..., 1]).abs() / st_ref[..., 1]).max().item() < 1e-5   # exp2 vs __expf, Σ order
    del attn
    gmap = torch.randn(B, Nn, R, R, generator=g).to(DEV)
    for z, s, st in zip(zs[:1], sizes, stats):
        d0 = ops.capture_bwd(z, s, R, gmap, gscale=1 / 32, group=H, strides=(Nn * RR, 1, RR))
        d1 = ops.capture_bwd(z, s, R, gmap, gscale=1 / 32, group=H, strides=(Nn * RR, 1, RR), stats=st)
        assert (d1 - d0).abs().max().item() < 1e-5 * max(1.0, d0.abs().max().item())


def _capture_maps_bwd_abi(zs, sizes, B, H, R, dmaps, gscale, stats):
    import ctypes
    from stablekeypoints_amd._lib import call, ptr, stream
    L = len(zs)
    Nn = zs[0].shape[-1]
    dzs = [torch.full_like(z, float("nan")) for z in zs]
    ws = torch.empty(B * R * R * Nn + B * H * R * max(sizes) * Nn, device=DEV)
    arr = lambda ts: ctypes.cast((ctypes.c_void_p * L)(*[t.data_ptr() for t in ts]), ctypes.POINTER(ctypes.c_void_p))
    call("skp_capture_maps_bwd", arr(zs), (ctypes.c_int * L)(*sizes), L, B, H, Nn, R, ptr(dmaps), float(gscale),
         arr(stats) if stats is not None else None, arr(dzs), ptr(ws), stream(DEV))
    torch.cuda.synchronize()
    return dzs


@pytest.mark.parametrize("B,H,sizes,R,Nn,with_stats", [(2, 8, (4, 4, 4, 8), 32, 40, True), (1, 3, (5, 3), 40, 36, True),
                                                       (2, 2, (16, 32), 128, 4, False), (1, 2, (8,), 32, 1000, True),
                                                       (3, 1, (1, 2), 8, 128, False), (1, 4, (7, 13), 100, 256, True),
                                                       (1, 2, (6, 64), 64, 260, True), (2, 4, (16, 32), 128, 500, True),
                                                       # the row kernel's 2 | 4 quads per lane, and its widest N
                                                       (1, 1, (4,), 16, 512, True), (1, 1, (4,), 16, 516, True),
                                                       (1, 1, (4,), 16, 1024, True)])
def test_capture_maps_bwd_vs_oracle(B, H, sizes, R, Nn, with_stats):
    """skp_capture_maps_bwd (one wave per (layer, head, row), V/W windows in registers) vs the
    oracle's capture_bwd of the per-image broadcast gradient (collect_maps_bwd, optimize.py:27-79,
    then the capture branch's softmax + bicubic adjoint, ptp_utils.py:513-536): relative 1e-4."""
    zs = [recipes.random_logits(400 + 5 * i + Nn, (B * H, s * s, Nn), scale=2.0) for i, s in enumerate(sizes)]
    zt = [T(z) for z in zs]
    _, stats = _capture_maps_abi(zt, list(sizes), B, H, R)
    w = recipes.random_logits(77 + Nn, (B, Nn, R, R))
    L = len(sizes)
    dzs = _capture_maps_bwd_abi(zt, list(sizes), B, H, R, T(w), 1.0 / (L * H), stats if with_stats else None)
    for i, (z, s) in enumerate(zip(zs, sizes)):
        dattn = np.concatenate([O.collect_maps_bwd([(H, R * R, Nn)] * L, w[b], layers=tuple(range(L)))[i]
                                for b in range(B)])
        ref = O.capture_bwd(z, s, R, dattn)
        got = N(dzs[i])
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() < 1e-4 * max(1e-3, np.abs(ref).max()), (i, np.abs(got - ref).max(), np.abs(ref).max())


def test_capture_maps_bwd_equals_per_layer_kernel_full_size():
    """Bench shape (B=8 × 8 heads, s = 16,16,16,32, R=128, N=500): the fused backward equals the
    per-layer skp_capture_bwd (the r01 path, oracle-pinned) to fp32 rounding, and is
    deterministic (bitwise equal on a second run)."""
    from stablekeypoints_amd import ops
    B, H, R, Nn, sizes = 8, 8, 128, 500, (16, 16, 16, 32)
    g = torch.Generator().manual_seed(9)
    zs = [(torch.randn(B * H, s * s, Nn, generator=g) * 3).to(DEV) for s in sizes]
    _, stats = _capture_maps_abi(zs, list(sizes), B, H, R)
    gmap = torch.randn(B, Nn, R, R, generator=g).to(DEV)
    d1 = _capture_maps_bwd_abi(zs, list(sizes), B, H, R, gmap, 1 / 32, stats)
    d2 = _capture_maps_bwd_abi(zs, list(sizes), B, H, R, gmap, 1 / 32, stats)
    for z, s, st, a, a2 in zip(zs, sizes, stats, d1, d2):
        ref = ops.capture_bwd(z, s, R, gmap, gscale=1 / 32, group=H, strides=(Nn * R * R, 1, R * R), stats=st)
        err = (a - ref).abs().max().item() / ref.abs().max().item()
        print(f"\ns={s}: fused bwd vs per-layer rel-max {err:.2e}")
        assert err < 1e-5
        assert torch.equal(a, a2)


def test_batched_captures_match_sequential_tiny():
    """TokenOptimizer: one B=2 pass (LogitStore, fused maps) == the reference's two passes."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize import TokenOptimizer
    from stablekeypoints_amd.optimize_token import load_ldm
    from stablekeypoints_amd.sd import TINY_CONFIG, TINY_IMAGE
    res = {}
    for batched in (False, True):
        ldm, ctls, _ = load_ldm(DEV, "random", feature_upsample_res=32, config=TINY_CONFIG)
        inner = ldm.scheduler
        noises = [torch.randn(1, 4, TINY_IMAGE // 8, TINY_IMAGE // 8, generator=torch.Generator().manual_seed(i))
                  .to(DEV) for i in range(2)]

        class Sched:
            timesteps = inner.timesteps

            def add_noise(self, x, noise, t):
                nz = torch.cat(noises[:x.shape[0]]) if x.shape[0] == 2 else noises.pop(0)
                return inner.add_noise(x, nz, t)
        ldm.scheduler = Sched()
        ctx = torch.from_numpy(recipes.random_logits(52, (1, 16, 32))).to(DEV)
        opt = TokenOptimizer(ldm, ctls, ctx, top_k=4, furthest_point_num_samples=8, accum=4, device=DEV,
                             batch_captures=batched)
        img = torch.from_numpy(recipes.uniform(51, (1, 3, TINY_IMAGE, TINY_IMAGE))).to(DEV)
        th = torch.tensor([[[0.88, -0.14, -0.2], [0.14, 0.88, 0.19]]])
        opt.transform.draw_theta = lambda batch: th
        idx = opt.micro_step(img)
        res[batched] = (N(idx), float(opt.run_tot), N(opt.context.grad))
    assert np.array_equal(res[False][0], res[True][0])
    assert abs(res[False][1] - res[True][1]) < 1e-5 * abs(res[False][1])
    assert np.allclose(res[False][2], res[True][2], rtol=1e-3, atol=1e-8)


def test_micro_steps_batch_equals_sequential_micro_steps():
    """TokenOptimizer.micro_steps (k images + k warps in ONE pass of 2k, one backward) equals k
    micro_step calls: same indices, loss statistics and context gradient (same noises/thetas)."""
    from stablekeypoints_amd.optimize import TokenOptimizer
    from stablekeypoints_amd.optimize_token import load_ldm
    from stablekeypoints_amd.sd import TINY_CONFIG, TINY_IMAGE
    k = 3
    lat = TINY_IMAGE // 8
    nI = [torch.randn(1, 4, lat, lat, generator=torch.Generator().manual_seed(10 + i)).to(DEV) for i in range(k)]
    nT = [torch.randn(1, 4, lat, lat, generator=torch.Generator().manual_seed(20 + i)).to(DEV) for i in range(k)]
    thetas = torch.tensor([[[0.88, -0.14, -0.2], [0.14, 0.88, 0.19]], [[0.95, 0.1, 0.05], [-0.1, 0.95, -0.1]],
                           [[0.8, 0.0, 0.1], [0.0, 0.8, 0.0]]])
    imgs = [torch.from_numpy(recipes.uniform(60 + i, (1, 3, TINY_IMAGE, TINY_IMAGE))).to(DEV) for i in range(k)]
    res = {}
    for batched in (False, True):
        ldm, ctls, _ = load_ldm(DEV, "tiny", feature_upsample_res=32, config=TINY_CONFIG)
        inner = ldm.scheduler
        cur = {}

        class Sched:
            timesteps = inner.timesteps

            def add_noise(self, x, noise, t):
                return inner.add_noise(x, cur["noise"], t)
        ldm.scheduler = Sched()
        ctx = torch.from_numpy(recipes.random_logits(52, (1, 16, 32))).to(DEV)
        opt = TokenOptimizer(ldm, ctls, ctx, top_k=4, furthest_point_num_samples=8, accum=k, device=DEV)
        if batched:
            cur["noise"] = torch.cat(nI + nT)
            opt.transform.draw_theta = lambda batch: thetas[:batch]
            idx = opt.micro_steps(imgs)
        else:
            idx = []
            for i in range(k):
                cur["noise"] = torch.cat([nI[i], nT[i]])
                opt.transform.draw_theta = lambda batch, i=i: thetas[i:i + 1]
                idx.append(opt.micro_step(imgs[i]))
        res[batched] = ([N(t) for t in idx], float(opt.run_tot), N(opt.context.grad))
    for a, b in zip(res[False][0], res[True][0]):
        assert np.array_equal(a, b)
    assert abs(res[False][1] - res[True][1]) < 1e-5 * abs(res[False][1])
    assert np.allclose(res[False][2], res[True][2], rtol=1e-3, atol=1e-8)


def test_prefetched_vae_pass_equals_inline():
    """TokenOptimizer.prefetch (warp + VAE on a side stream, thetas drawn ahead) then
    micro_steps gives the same indices, loss and gradient as micro_steps alone."""
    from stablekeypoints_amd.optimize import TokenOptimizer
    from stablekeypoints_amd.optimize_token import load_ldm
    from stablekeypoints_amd.sd import TINY_CONFIG, TINY_IMAGE
    lat = TINY_IMAGE // 8
    noise = torch.randn(4, 4, lat, lat, generator=torch.Generator().manual_seed(3)).to(DEV)
    thetas = torch.tensor([[[0.9, -0.1, 0.1], [0.1, 0.9, -0.05]], [[0.85, 0.05, -0.1], [-0.05, 0.85, 0.2]]])
    imgs = [torch.from_numpy(recipes.uniform(80 + i, (1, 3, TINY_IMAGE, TINY_IMAGE))).to(DEV) for i in range(2)]
    res = {}
    for pre in (False, True):
        ldm, ctls, _ = load_ldm(DEV, "tiny", feature_upsample_res=32, config=TINY_CONFIG)
        inner = ldm.scheduler

        class Sched:
            timesteps = inner.timesteps

            def add_noise(self, x, n, t):
                return inner.add_noise(x, noise, t)
        ldm.scheduler = Sched()
        ctx = torch.from_numpy(recipes.random_logits(52, (1, 16, 32))).to(DEV)
        opt = TokenOptimizer(ldm, ctls, ctx, top_k=4, furthest_point_num_samples=8, accum=2, device=DEV)
        opt.transform.draw_theta = lambda batch: thetas[:batch]
        if pre:
            opt.prefetch(imgs)
        idx = opt.micro_steps(imgs)
        assert not opt._prefetched
        res[pre] = ([N(t) for t in idx], float(opt.run_tot), N(opt.context.grad))
    for a, b in zip(res[False][0], res[True][0]):
        assert np.array_equal(a, b)
    assert abs(res[False][1] - res[True][1]) <= 1e-6 * abs(res[False][1])
    # the equivariance adjoint scatters with atomics, so two identical runs differ at ~1e-6
    assert np.allclose(res[False][2], res[True][2], rtol=1e-4, atol=1e-8)


def test_prefetch_behind_capture_backward_equals_prefetch_before_backward():
    """micro_steps(images, prefetch=[next]) with the next pass's VAE enqueued by the sparse capture
    backward's hook (prefetch_at="capture_bwd", the default) or before the backward ("bwd"): the
    same thetas (CPU generator order unchanged), indices, losses and gradients over two passes."""
    from stablekeypoints_amd.optimize import TokenOptimizer
    from stablekeypoints_amd.optimize_token import load_ldm
    from stablekeypoints_amd.sd import TINY_CONFIG, TINY_IMAGE
    lat = TINY_IMAGE // 8
    noise = torch.randn(4, 4, lat, lat, generator=torch.Generator().manual_seed(4)).to(DEV)
    imgs = [torch.from_numpy(recipes.uniform(90 + i, (1, 3, TINY_IMAGE, TINY_IMAGE))).to(DEV) for i in range(4)]
    res = {}
    for where in ("capture_bwd", "bwd"):
        ldm, ctls, _ = load_ldm(DEV, "tiny", feature_upsample_res=32, config=TINY_CONFIG)
        inner = ldm.scheduler

        class Sched:
            timesteps = inner.timesteps

            def add_noise(self, x, n, t):
                return inner.add_noise(x, noise, t)
        ldm.scheduler = Sched()
        ctx = torch.from_numpy(recipes.random_logits(53, (1, 16, 32))).to(DEV)
        torch.manual_seed(7)
        opt = TokenOptimizer(ldm, ctls, ctx, top_k=4, furthest_point_num_samples=8, accum=4, device=DEV)
        opt.prefetch_at = where
        a, b = imgs[:2], imgs[2:]
        opt.prefetch(a)
        i1 = opt.micro_steps(a, prefetch=[b])
        assert len(opt._prefetched) == 1          # b's VAE is queued
        th1 = opt.transform.last_params["theta"].clone()
        i2 = opt.micro_steps(b)
        assert not opt._prefetched
        th2 = opt.transform.last_params["theta"].clone()
        res[where] = ([N(t) for t in i1 + i2], float(opt.run_tot), N(opt.context.grad), N(th1), N(th2))
    x, y = res["capture_bwd"], res["bwd"]
    for p, q in zip(x[0], y[0]):
        assert np.array_equal(p, q)
    assert np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4])
    assert abs(x[1] - y[1]) <= 1e-6 * abs(y[1])
    assert np.allclose(x[2], y[2], rtol=1e-4, atol=1e-8)


# ----------------------------------------------------------------------------- UNet-side GroupNorm(+SiLU)
@pytest.mark.parametrize("B,C,H,W,G,act,shifted", [(2, 320, 64, 64, 32, True, True), (2, 1280, 8, 8, 32, False, False),
                                                   (1, 128, 256, 256, 32, True, False), (2, 12, 5, 7, 4, True, True),
                                                   (1, 64, 16, 16, 8, False, True)])
def test_groupnorm_act_vs_torch_fp64(B, C, H, W, G, act, shifted):
    """Fused GroupNorm(x + shift)(+SiLU) fwd and input-gradient vs a torch fp64 reference."""
    import torch.nn.functional as F
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = (torch.randn(B, C, H, W, generator=g) * 3 + 1).to(DEV).requires_grad_(True)
    gamma = torch.randn(C, generator=g).to(DEV)
    beta = torch.randn(C, generator=g).to(DEV)
    shift = (torch.randn(B, C, generator=g) * 2).to(DEV) if shifted else None
    y = ops.group_norm_act(x, gamma, beta, G, 1e-5, act, shift)
    dy = torch.randn(B, C, H, W, generator=g).to(DEV)
    (y * dy).sum().backward()
    xd = x.detach().double().requires_grad_(True)
    xs = xd + shift.double()[:, :, None, None] if shifted else xd
    yr = F.group_norm(xs, G, gamma.double(), beta.double(), 1e-5)
    yr = F.silu(yr) if act else yr
    (yr * dy.double()).sum().backward()
    assert (y.double() - yr).abs().max().item() < 2e-5
    assert (x.grad.double() - xd.grad).abs().max().item() < 2e-4 * max(1.0, xd.grad.abs().max().item())


@pytest.mark.parametrize("BH,S,L,D", [(16, 256, 256, 40), (4, 1024, 1024, 80), (8, 256, 500, 160), (3, 64, 77, 40),
                                      (2, 256, 256, 160), (2, 1024, 1024, 64), (2, 128, 192, 40),
                                      (2, 4096, 4096, 40)])
def test_math_attention_fused_softmax_backward_vs_fp64(BH, S, L, D):
    """ops.math_attention: forward and (q, k, v) gradients vs torch fp64 autograd."""
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(S + L)
    q = (torch.randn(BH, S, D, generator=g)).to(DEV).requires_grad_(True)
    k = (torch.randn(BH, L, D, generator=g)).to(DEV).requires_grad_(True)
    v = (torch.randn(BH, L, D, generator=g)).to(DEV).requires_grad_(True)
    scale = D ** -0.5
    out = ops.math_attention(q, k, v, scale)
    dout = torch.randn(BH, S, D, generator=g).to(DEV)
    (out * dout).sum().backward()
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    ref = torch.softmax(qd @ kd.transpose(1, 2) * scale, -1) @ vd
    (ref * dout.double()).sum().backward()
    assert (out.double() - ref).abs().max().item() < 1e-5
    for a, b in ((q.grad, qd.grad), (k.grad, kd.grad), (v.grad, vd.grad)):
        assert (a.double() - b).abs().max().item() < 1e-4 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("BH,S,L,D,q_grad", [(2, 256, 320, 64, True), (3, 128, 128, 80, False), (1, 4096, 4096, 40, True),
                                             (5, 64, 640, 40, False)])
def test_attn_bwd_kv_vs_unfused(monkeypatch, BH, S, L, D, q_grad):
    """skp_attn_bwd_kv (dS, dV, dK in one pass) vs the unfused backward (skp_attn_dscore + GEMMs)
    and fp64 autograd, with and without a gradient for q."""
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(S * 7 + L)
    base = [torch.randn(BH, n, D, generator=g).to(DEV) for n in (S, L, L)]
    dout = torch.randn(BH, S, D, generator=g).to(DEV)
    grads = {}
    monkeypatch.setattr(ops, "ATTN_FLASH", ())
    for fused in (True, False):
        monkeypatch.setattr(ops, "ATTN_FUSED_KV", (40, 64, 80) if fused else ())
        q, k, v = (t.clone().requires_grad_(rg) for t, rg in zip(base, (q_grad, True, True)))
        (ops.math_attention(q, k, v, D ** -0.5) * dout).sum().backward()
        grads[fused] = [t.grad for t in (q, k, v)]
    qd, kd, vd = (t.double().requires_grad_(True) for t in base)
    (torch.softmax(qd @ kd.transpose(1, 2) * D ** -0.5, -1) @ vd * dout.double()).sum().backward()
    for i, ref in enumerate((qd.grad, kd.grad, vd.grad)):
        if i == 0 and not q_grad:
            assert grads[True][0] is None
            continue
        tol = 1e-4 * max(1.0, ref.abs().max().item())
        assert (grads[True][i].double() - ref).abs().max().item() < tol
        assert (grads[True][i] - grads[False][i]).abs().max().item() < tol


@pytest.mark.parametrize("BH,S,L,D,q_grad", [(2, 256, 320, 64, True), (3, 128, 128, 80, False), (1, 4096, 4096, 40, True),
                                             (5, 64, 640, 40, True), (4, 1024, 1024, 40, True), (4, 512, 500, 40, True),
                                             (2, 256, 77, 64, False), (3, 128, 1, 40, True), (2, 64, 129, 80, True)])
def test_flash_attention_vs_math_and_fp64(monkeypatch, BH, S, L, D, q_grad):
    """FlashAttention (skp_attn_fwd with row stats + skp_attn_bwd_flash rebuilding P) vs the
    P-saving MathAttention and fp64 autograd: output and (q, k, v) gradients."""
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(S * 3 + L + D)
    base = [(torch.randn(BH, n, D, generator=g) * 1.5).to(DEV) for n in (S, L, L)]
    dout = torch.randn(BH, S, D, generator=g).to(DEV)
    res = {}
    for flash in (True, False):
        monkeypatch.setattr(ops, "ATTN_FLASH", (40, 64, 80) if flash else ())
        q, k, v = (t.clone().requires_grad_(rg) for t, rg in zip(base, (q_grad, True, True)))
        out = ops.math_attention(q, k, v, D ** -0.5)
        assert (out.grad_fn.__class__.__name__ == "FlashAttentionBackward") == flash
        (out * dout).sum().backward()
        res[flash] = [out.detach()] + [t.grad for t in (q, k, v)]
    qd, kd, vd = (t.double().requires_grad_(True) for t in base)
    ref = torch.softmax(qd @ kd.transpose(1, 2) * D ** -0.5, -1) @ vd
    (ref * dout.double()).sum().backward()
    # online softmax with the fast exp: within 2e-5 like attention_nograd (north_star bar: 1e-4)
    assert (res[True][0].double() - ref).abs().max().item() < 2e-5
    assert (res[True][0] - res[False][0]).abs().max().item() < 2e-5
    for i, r in enumerate((qd.grad, kd.grad, vd.grad), start=1):
        if i == 1 and not q_grad:
            assert res[True][1] is None
            continue
        tol = 1e-4 * max(1.0, r.abs().max().item())
        assert (res[True][i].double() - r).abs().max().item() < tol
        assert (res[True][i] - res[False][i]).abs().max().item() < tol


@pytest.mark.parametrize("shape", [(8, 4096, 320), (8, 1024, 640), (3, 85, 1280), (5, 2048), (7, 12), (2, 3, 4),
                                   (1, 1, 1024)])
def test_layer_norm_vs_fp64(monkeypatch, shape):
    """ops.layer_norm (skp_layernorm_fwd/bwd, one wave per row) vs fp64 autograd of
    F.layer_norm: output within 2e-6 of its scale, input gradient within 1e-5 (rows of 4 to
    2048 floats, row counts not a multiple of the 4 rows per block)."""
    from stablekeypoints_amd import ops
    monkeypatch.setattr(ops, "LN_MIN_ROWS", 1)
    g = torch.Generator().manual_seed(sum(shape))
    C = shape[-1]
    x = (torch.randn(*shape, generator=g) * 3 + 1).to(DEV).requires_grad_(True)
    w = torch.randn(C, generator=g).to(DEV)
    b = torch.randn(C, generator=g).to(DEV)
    dy = torch.randn(*shape, generator=g).to(DEV)
    y = ops.layer_norm(x, w, b, 1e-5)
    assert y.grad_fn.__class__.__name__ == "LayerNormFnBackward"
    (y * dy).sum().backward()
    xd = x.detach().double().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xd, (C,), w.double(), b.double(), 1e-5)
    (ref * dy.double()).sum().backward()
    assert (y.double() - ref).abs().max().item() < 2e-6 * max(1.0, ref.abs().max().item())
    assert (x.grad.double() - xd.grad).abs().max().item() < 1e-5 * max(1.0, xd.grad.abs().max().item())


@pytest.mark.parametrize("rows,cols", [(64, 4096), (33, 500), (128, 1024), (7, 77), (5, 16384), (9, 12)])
def test_softmax_fwd_in_place_vs_torch(rows, cols):
    """skp_softmax_fwd (in place) vs torch.softmax: within 2 ulp-level (1e-6 relative to the row
    max) including large-magnitude and -inf entries; non-multiple-of-4 rows fall back to torch."""
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(rows * cols)
    s = (torch.randn(rows, cols, generator=g) * 8).to(DEV)
    s[0, : cols // 2] = float("-inf")
    ref = torch.softmax(s.double(), -1)
    out = ops.softmax_(s.clone())
    assert (out.double() - ref).abs().max().item() < 1e-6
    assert torch.allclose(out.sum(-1).double(), torch.ones(rows, dtype=torch.float64, device=DEV), atol=1e-5)


@pytest.mark.parametrize("shape", [(2, 64, 2560), (3, 7, 16), (1, 5, 24)])
def test_geglu_fused_vs_torch(shape):
    """ops.geglu (skp_geglu_fwd/_bwd) vs torch's chunk · gelu and its autograd, fp32."""
    import torch.nn.functional as F
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(shape[-1])
    h = (torch.randn(*shape, generator=g) * 3).to(DEV).requires_grad_(True)
    out = ops.geglu(h)
    dout = torch.randn(*out.shape, generator=g).to(DEV)
    (out * dout).sum().backward()
    hr = h.detach().clone().requires_grad_(True)
    x, gate = hr.chunk(2, dim=-1)
    ref = x * F.gelu(gate)
    (ref * dout).sum().backward()
    assert (out - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())
    assert (h.grad - hr.grad).abs().max().item() < 1e-5 * max(1.0, hr.grad.abs().max().item())


@pytest.mark.parametrize("BH,s,R,N", [(4, 16, 128, 500), (2, 8, 32, 77), (3, 32, 64, 1000)])
def test_capture_bwd_with_forward_stats_equals_recomputed(BH, s, R, N):
    """skp_capture_fwd's per-pixel (max, 1/Σ) stats: equal to the attention's own row max /
    normaliser, and the backward fed with them equals the backward that recomputes them."""
    from stablekeypoints_amd import ops
    from stablekeypoints_amd._lib import call, ptr, stream
    g = torch.Generator().manual_seed(BH * s + N)
    z = (torch.randn(BH, s * s, N, generator=g) * 2).to(DEV)
    attn = torch.empty(BH, R * R, N, device=DEV)
    stats = torch.empty(BH, R * R, 2, device=DEV)
    call("skp_capture_fwd", ptr(z), BH, s, N, R, ptr(attn), ptr(stats), stream(z.device))
    ref = ops.capture_attn(z, s, R)
    assert torch.equal(attn, ref)
    zu = torch.nn.functional.interpolate(z.view(BH, s, s, N).permute(0, 3, 1, 2), size=(R, R), mode="bicubic",
                                         align_corners=False).permute(0, 2, 3, 1).reshape(BH, R * R, N)
    assert (stats[..., 0] - zu.max(-1).values).abs().max().item() < 1e-4
    assert (stats[..., 1] * torch.exp(zu - stats[..., :1]).sum(-1) - 1).abs().max().item() < 1e-5
    gr = torch.randn(BH, R * R, N, generator=g).to(DEV)
    d0 = ops.capture_bwd(z, s, R, gr)
    d1 = ops.capture_bwd(z, s, R, gr, stats=stats)
    assert (d1 - d0).abs().max().item() < 1e-5 * max(1.0, d0.abs().max().item())


@pytest.mark.parametrize("BH,S,L,D", [(8, 4096, 4096, 40), (4, 256, 192, 40), (3, 128, 512, 64), (2, 1024, 1024, 80),
                                      (2, 64, 77, 40), (8, 4096, 500, 40), (2, 128, 1, 64)])
def test_attention_nograd_fused_vs_fp64(BH, S, L, D):
    """ops.attention_nograd (skp_attn_fwd: online softmax, no score tensor, ragged last key
    block when L is not a multiple of 64) vs torch fp64, including large-magnitude logits."""
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(S + L + D)
    q = (torch.randn(BH, S, D, generator=g) * 2).to(DEV)
    k = (torch.randn(BH, L, D, generator=g) * 2).to(DEV)
    v = torch.randn(BH, L, D, generator=g).to(DEV)
    scale = D ** -0.5
    out = ops.attention_nograd(q, k, v, scale)
    ref = torch.softmax(q.double() @ k.double().transpose(1, 2) * scale, -1) @ v.double()
    assert (out.double() - ref).abs().max().item() < 2e-5


def test_residual_bias_add_bitexact():
    """a + (h + bias[c]) equals torch's two adds bit for bit; gradients pass through."""
    from stablekeypoints_amd import ops
    g = torch.Generator().manual_seed(9)
    for shape in ((2, 320, 64, 64), (2, 12, 5, 7)):
        a = torch.randn(*shape, generator=g).to(DEV).requires_grad_(True)
        h = torch.randn(*shape, generator=g).to(DEV).requires_grad_(True)
        b = torch.randn(shape[1], generator=g).to(DEV)
        out = ops.residual_bias_add(a, h, b)
        assert torch.equal(out, a + (h + b[:, None, None]))
        out.sum().backward()
        assert torch.equal(a.grad, torch.ones_like(a)) and torch.equal(h.grad, torch.ones_like(h))


def test_unet_fused_groupnorm_matches_torch_groupnorm():
    """The SD UNet forward/backward with the fused GroupNorm (+ folded conv biases / time
    embedding, fused residual+bias) equals the plain-torch one."""
    from stablekeypoints_amd.sd import build_sd15, TINY_CONFIG, unet as unet_mod
    ldm = build_sd15(seed=0, config=TINY_CONFIG, device=DEV)
    lat = torch.randn(2, 4, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    outs = []
    for fused in (False, True):
        unet_mod.USE_FUSED_GROUPNORM = fused
        ctx = torch.randn(1, 16, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        ctx.requires_grad_(True)
        out = ldm.unet(lat, torch.tensor(0, device=DEV).repeat(2), ctx.repeat(2, 1, 1))["sample"]
        out.square().mean().backward()
        outs.append((out.detach(), ctx.grad.detach()))
    unet_mod.USE_FUSED_GROUPNORM = True
    assert (outs[0][0] - outs[1][0]).abs().max().item() < 1e-4
    assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-3, atol=1e-6)


# ----------------------------------------------------------------------------- A16: SDXL shapes
def test_sdxl_shaped_capture_path():
    """SURVEY §8 A16 (SDXL, config 5): up_blocks[0] at 32², C=1280, 20 heads × hd 64, context 2048.
    The reference's SDXL patch is inert (parity unpinned), so the capture path is checked at SDXL
    shapes against the oracle (N=100 to keep the oracle fast) plus full-N properties."""
    from stablekeypoints_amd import ops
    H, s, R, d = 20, 32, 128, 64
    g = torch.Generator().manual_seed(5)
    for Nn in (100, 500):
        q = torch.randn(1 * H, s * s, d, generator=g) * 0.5
        k = torch.randn(1 * H, Nn, d, generator=g) * 0.5
        z = ops.capture_logits(q.to(DEV), k.to(DEV), d ** -0.5)
        zr = (q.double() @ k.double().transpose(1, 2) * d ** -0.5).float()
        assert torch.allclose(z.cpu(), zr, atol=1e-4)
        maps = ops.capture_maps([z] * 4, [s] * 4, 1, R)          # (1, N, 128, 128)
        m = N(maps[0])
        assert np.allclose(m.sum(0), 1.0, atol=1e-4)
        if Nn == 100:
            ref = O.collect_maps([O.capture_fwd(N(z), s, R)] * 4)
            assert np.abs(m - ref).max() < 1e-6
            w = recipes.random_logits(3, (Nn, R * R))
            dz = N(ops.capture_bwd(z, s, R, T(w).t().unsqueeze(0).expand(H, R * R, Nn)))
            dref = O.capture_bwd(N(z), s, R, np.broadcast_to(w.T[None], (H, R * R, Nn)).astype(np.float32))
            assert np.abs(dz - dref).max() < 1e-4 * max(1.0, np.abs(dref).max())


def test_sdxl_tiny_token_opt_step_runs_and_captures_sdxl_layers():
    """SDXL UNet (toy widths, same structure): the capture hook finds the up_blocks[0]
    cross-attention layers (the SDXL capture site), the batched step runs and the context
    gradient is finite and nonzero."""
    from stablekeypoints_amd.optimize import TokenOptimizer
    from stablekeypoints_amd.optimize_token import load_ldm
    from stablekeypoints_amd.sd import SDXLUNet
    ldm, ctls, _ = load_ldm(DEV, "tiny-xl", feature_upsample_res=32)
    assert isinstance(ldm.unet, SDXLUNet)
    ctx = torch.randn(1, 12, ldm.unet.cross_attention_dim, generator=torch.Generator().manual_seed(0)).to(DEV)
    opt = TokenOptimizer(ldm, ctls, ctx, top_k=4, furthest_point_num_samples=8, accum=2, device=DEV)
    imgs = [torch.from_numpy(recipes.uniform(70 + i, (1, 3, 256, 256))).to(DEV) for i in range(2)]
    idx = opt.micro_steps(imgs)
    assert len(idx) == 2 and all(i.numel() == 4 for i in idx)
    g = opt.context.grad
    assert torch.isfinite(g).all() and g.abs().sum() > 0
    assert opt.controllers[next(iter(opt.controllers))].heads == 64 // 16   # toy head dim 16 at 64 channels
