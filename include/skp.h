/*
 * skp.h — C ABI of libskp.so, the MI355X (gfx950) hot path of StableKeypoints.
 *
 * The reference (damaggu/StableKeypoints) has no FFI: its hot path is Python/torch
 * (SURVEY.md §8b).  Each entry point below replaces one reference function or the
 * torch-op sequence inside it; the reference file:line is cited per function.
 * The Python mirror of the reference API (stablekeypoints_amd/) binds these with
 * ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - All pointers are DEVICE pointers to row-major fp32 / int64 buffers that the
 *     caller allocates (caller owns every buffer; the library keeps no global state
 *     and is safe to call concurrently on different streams).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - Return 0 on success, SKP_EBADARG (-1) for invalid arguments, SKP_ELAUNCH (-2)
 *     when a kernel launch fails.  skp_last_error() gives the thread-local message.
 *   - "maps" are (T, h, w) fp32; "positions" are (row + 0.5, col + 0.5) fp32 pairs;
 *     "attn" is one captured layer (BH, R*R, N) fp32 in the reference layout
 *     (ptp_utils.py:534-536: (batch*heads, pixels, tokens)).
 */
#ifndef SKP_H
#define SKP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SKP_OK 0
#define SKP_EBADARG (-1)
#define SKP_ELAUNCH (-2)
#define SKP_MAX_LAYERS 16

const char* skp_last_error(void);
int skp_version(void);

/* ---------------------------------------------------------------- A1 capture
 * Replaces the capture branch of the patched CrossAttention.forward,
 * ptp_utils.py:508-538 (bicubic(x) -> to_q -> q kᵀ·scale -> softmax).  With
 * z_low = the layer's normal-path logits q kᵀ·scale at s×s (ptp_utils.py:493),
 * attn[b,p,n] = softmax_n(bicubic_{s->R}(z_low[b,:,n])[p]).
 *   z_low (BH, s*s, N) -> attn (BH, R*R, N).  `stats` (may be NULL): (BH, R*R, 2) floats
 *   receive each pixel's softmax row max and 1/Σexp, which the backward can reuse.     */
int skp_capture_fwd(const float* z_low, int BH, int s, int N, int R, float* attn, float* stats, void* stream);

/* Backward of skp_capture_fwd: dz_low = bicubicᵀ( a ⊙ (g − Σ_n a g) ), g = gscale·dattn.
 * Row b of g starts at dattn + (b / group)·sb and is read with strides (sp, sn), so a
 * broadcast gradient needs no materialisation: the layer/head mean of collect_maps gives
 * group = BH, sb = 0; a per-image map gradient (B, N, R²) gives group = heads,
 * sb = N·R², sp = 1, sn = R².  `workspace` holds BH*R*s*N floats (row-adjoint partials).
 * `stats`: the forward's per-pixel (max, 1/Σ) or NULL (recomputed by two row reductions). */
int skp_capture_bwd(const float* z_low, int BH, int s, int N, int R, const float* dattn, int group, long long sb,
                    long long sp, long long sn, float gscale, const float* stats, float* dz_low, float* workspace,
                    void* stream);

/* Fused capture + per-image aggregate: the capture branch (ptp_utils.py:508-538) of L
 * layers followed by collect_maps' mean over layers and heads (optimize.py:27-79), per image,
 * with no (B·H, R², N) attention in memory:
 *   maps[b, n, p] = (1/(L·H)) Σ_l Σ_h softmax_n(bicubic_{s_l->R}(z_l[b·H + h, :, n])[p]).
 * z_low: host array of L device pointers, layer l (B·H, s_l², N), 16-B aligned when N % 4 == 0;
 * sizes: host array of the L s_l (1 <= s_l <= R); maps (B, N, R*R).
 * stats: NULL or a host array of L device pointers (entries may be NULL), layer l
 * (B·H, R*R, 2) receiving each pixel's softmax (max, 1/Σexp) exactly as skp_capture_fwd's
 * `stats`, for skp_capture_bwd.                                                   */
int skp_capture_maps_fwd(const float* const* z_low, const int* sizes, int L, int B, int H, int N, int R, float* maps,
                         float* const* stats, void* stream);

/* Backward of skp_capture_maps_fwd for all L layers: dz_low[l] = bicubicᵀ(a ⊙ (g − Σ_n a g))
 * per (b·H + h) with g = gscale · dmaps[b] (the per-image map gradient broadcast over heads,
 * gscale = 1/(L·H) for the mean) and a rebuilt from the forward's stats (NULL: recomputed).
 * dmaps (B, N, R*R) token-major; dz_low: host array of L device pointers, (B·H, s_l², N).
 * N % 4 == 0.  workspace: B·R²·N + B·H·R·max(s_l)·N floats, 16-B aligned (pixel-major gradient
 * copy + row partials).  Deterministic (no atomics).                                   */
int skp_capture_maps_bwd(const float* const* z_low, const int* sizes, int L, int B, int H, int N, int R,
                         const float* dmaps, float gscale, const float* const* stats, float* const* dz_low,
                         float* workspace, void* stream);

/* Backward of skp_capture_maps_fwd for a SPARSE per-image map gradient — the token-opt losses
 * read only the selected token rows maps[b, tok] (optimize.py:403-424 sharpening / equivariance
 * on top_embedding_indices), so image b's gradient is gsel[b, k] (R*R) at token sel_tok[b, k]
 * (int64, −1 = unused slot; duplicates add), zero elsewhere.  Same result as
 * skp_capture_maps_bwd on the scattered dense gradient, without forming it:
 *   dZ = a ⊙ (g − dot) = [a_k·g_k at the K selected tokens] − dot·a,  dot = Σ_k a_k·g_k,
 * the dense part needing one scalar per pixel.  K <= 32, N % 4 == 0, stats REQUIRED (the
 * forward's), dz_low / z_low 16-B aligned.  workspace: skp_capture_maps_bwd_sel_workspace()
 * floats, 16-B aligned (returns -1 on a bad shape).  R = s·{4, 8, 16} for R in {32, 64, 128}
 * take the fast kernels; other shapes scatter into a dense gradient and run
 * skp_capture_maps_bwd.  Deterministic (no atomics).                                   */
long long skp_capture_maps_bwd_sel_workspace(const int* sizes, int L, int B, int H, int N, int R, int K);
int skp_capture_maps_bwd_sel(const float* const* z_low, const int* sizes, int L, int B, int H, int N, int R,
                             const long long* sel_tok, int K, const float* gsel, float gscale,
                             const float* const* stats, float* const* dz_low, float* workspace, void* stream);
/* Per-phase device time of skp_capture_maps_bwd_sel's fast path (measurement only, not on the
 * reference's interface): skp_sel_bwd_timing(1) makes every later single-stream call record HIP
 * events between its phases on its stream (at most 256 calls), skp_sel_bwd_timing(0) stops;
 * skp_sel_bwd_timing_read waits for the recorded calls and returns the summed ms of
 * ms[0] sel_gather, ms[1] sel_doth (sel_dot), ms[2] the adjoint's vertical pass (sel_adjw), ms[3]
 * sel_dense, and the number of calls, then clears the record.                              */
int skp_sel_bwd_timing(int enable);
int skp_sel_bwd_timing_read(double* ms, int* calls);

/* ---------------------------------------------------------------- A3 aggregate
 * optimize.collect_maps (optimize.py:27-79), token-major output:
 * out[m, p] = (1/(L·BH)) Σ_l Σ_b attn_l[b, p, idx(m)], idx = indices[m] or m.
 * layers: host array of L device pointers, each (BH, RR, N).                  */
int skp_aggregate(const float* const* layers, int L, int BH, int RR, int N, const long long* indices,
                  int n_out, float* out, void* stream);

/* Bilinear resize (F.interpolate mode="bilinear", align_corners=False; optimize.py:63-70)
 * of C square planes R×R -> Ro×Ro, and its adjoint.                            */
int skp_resize_bilinear(const float* in, int C, int R, int Ro, float* out, void* stream);
int skp_resize_bilinear_bwd(const float* gout, int C, int R, int Ro, float* gin, void* stream);

/* ---------------------------------------------------------------- A4-A6 argmax family
 * eval.find_max_pixel (eval.py:39-60): first-occurrence argmax, NaN is max.
 * rows: optional device list of n_rows row ids (NULL = rows 0..T-1).
 * pos (n_rows, 2) = (idx / w + 0.5, idx % w + 0.5); idx (n_rows) optional.     */
int skp_argmax2d(const float* maps, int T, int h, int w, const long long* rows, int n_rows, float* pos,
                 long long* idx, void* stream);

/* eval.find_k_max_pixels + mask_radius (eval.py:62-111): `num` rounds of argmax,
 * each followed by map *= (squared distance > radius2).  pos (num, T, 2).
 * masked (T, h, w) optional: the map after the last round's mask.             */
int skp_k_max_pixels(const float* maps, int T, int h, int w, int num, float radius2, float* pos,
                     float* masked, void* stream);

/* eval.mask_radius (eval.py:83-111): out = map * (squared distance to pos > radius2). */
int skp_mask_radius(const float* maps, int T, int h, int w, const float* pos, float radius2, float* out,
                    void* stream);

/* eval.pixel_from_weighted_avg (eval.py:113-155): zero pixels farther than
 * `distance` from the argmax (in place when mutate != 0, like the reference),
 * then the normalised centroid + 0.5.  distance < 0 disables the cut.          */
int skp_weighted_avg(float* maps, int T, int h, int w, float distance, int mutate, float* pos, void* stream);

/* ---------------------------------------------------------------- A7 target
 * optimize_token.gaussian_circles (optimize_token.py:204-242):
 * out[t,i,j] = mean_q exp(-((j+.5-P[q,t,1]·size)² + (i+.5-P[q,t,0]·size)²)/(2σ²)),
 * P = pos (num, T, 2) in [0, 1].                                               */
int skp_gaussian_target(const float* pos, int num, int T, int size, float sigma, float* out, void* stream);

/* ---------------------------------------------------------------- A8-A10 select
 * ptp_utils.find_top_k_gaussian (ptp_utils.py:86-112): per-token
 * KL(normalised G(argmax)+eps ‖ softmax(map+eps)), ascending, first top_k
 * (ties by token id).  kl (T) doubles optional; workspace >= 8*T bytes, 8-B aligned: it
 * holds the keys when kl is NULL and is not touched otherwise (it may then be kl itself). */
int skp_topk_gaussian(const float* maps, int T, int h, int w, int top_k, float sigma, float epsilon,
                      int num_subjects, long long* out, double* kl, void* workspace, void* stream);

/* skp_topk_gaussian for nb images in one launch (each image's top-k chosen as the reference's
 * find_top_k_gaussian on that image, ptp_utils.py:86-112; optimize.py:403-410 per replica):
 * maps (nb, T, h, w), out (nb, top_k), kl (nb, T) optional, workspace >= 8*nb*T bytes (as
 * skp_topk_gaussian's: the keys when kl is NULL).                                            */
int skp_topk_gaussian_batch(const float* maps, int nb, int T, int h, int w, int top_k, float sigma,
                            float epsilon, int num_subjects, long long* out, double* kl, void* workspace,
                            void* stream);

/* The ranking step of find_top_k_gaussian / entropy_sort (`torch.argsort(keys)[:top_k]`,
 * ptp_utils.py:110-112 and :185) for nb segments of T fp64 keys: ascending, NaN last, ties by
 * index; keys (nb, T), out (nb, top_k).  skp_topk_gaussian_batch with top_k = 0 and this call
 * together are skp_topk_gaussian_batch with top_k > 0.                                        */
int skp_topk_keys(const double* keys, int nb, int T, int top_k, long long* out, void* stream);

/* ptp_utils.entropy_sort (ptp_utils.py:165-187): ascending softmax entropy.  ent (T)
 * doubles optional; workspace >= 8*T bytes, 8-B aligned (the keys when ent is NULL,
 * not touched otherwise); out is not written when top_k == 0.                   */
int skp_entropy_sort(const float* maps, int T, int h, int w, int top_k, long long* out, double* ent,
                     void* workspace, void* stream);

/* ptp_utils.furthest_point_sampling (ptp_utils.py:115-159) on the argmax positions
 * of the candidate rows; strict '>' first-wins, IEEE sqrt distances.
 * out[top_k] (int64); n_out (device int, optional) = how many were selected;
 * out[n_out:] = -1 (every entry of out is written).
 * workspace >= 8 * n_cand bytes (skp_fps_batch's with nb = 1: the candidates'
 * argmax positions, two floats each), 4-B aligned.                             */
int skp_fps(const float* maps, int T, int h, int w, const long long* cand, int n_cand, int top_k,
            long long* out, int* n_out, void* workspace, void* stream);
/* skp_fps for nb images in one launch (ptp_utils.py:115-159 per replica, optimize.py:419-424):
 * maps (nb, T, h, w), cand (nb, n_cand) token ids of each image, out (nb, top_k), n_out (nb),
 * workspace >= 8 * nb * n_cand bytes.                                                        */
int skp_fps_batch(const float* maps, int nb, int T, int h, int w, const long long* cand, int n_cand, int top_k,
                  long long* out, int* n_out, void* workspace, void* stream);
/* The ranking of skp_topk_keys and the candidates' argmax of skp_fps_batch in one launch, then the
   FPS launch: per image b, cand[b] = the n_cand tokens of smallest keys[b] (ascending; NaN last,
   ties by index — torch.argsort(keys)[:n_cand] of find_top_k_gaussian, ptp_utils.py:110-112), and
   out[b] / n_out[b] = furthest_point_sampling(maps[b], top_k, cand[b]) (ptp_utils.py:115-159) on the
   (nb, T, h, w) maps the FPS reads (the warped image's, optimize.py:403-410).  workspace: 2·nb·n_cand
   floats. */
int skp_fps_keys_batch(const double* keys, const float* maps, int nb, int T, int h, int w, int n_cand, int top_k,
                       long long* cand, long long* out, int* n_out, void* workspace, void* stream);

/* ---------------------------------------------------------------- A11 sharpening
 * optimize.sharpening_loss (optimize.py:166-206): pos = k-max of A / w,
 * G = gaussian_circles(pos, h, σ), loss = mean((A-G)²).
 * pos (num, T, 2) is written for the backward; partial >= T doubles.          */
int skp_sharpen_fwd(const float* A, int T, int h, int w, float sigma, int num_subjects, float* pos,
                     double* partial, float* loss, void* stream);
/* dA = gout[0] · 2(A − G)/numel.                                               */
int skp_sharpen_bwd(const float* A, int T, int h, int w, float sigma, int num_subjects, const float* pos,
                     const float* gout, float* dA, void* stream);
/* The sharpening loss of nb images at once (optimize.py:425-437 per replica): A (nb, T, h, w),
 * loss (nb) = each image's mean, pos (num, nb·T, 2), partial >= nb·T doubles; backward with
 * gout (nb).  Each image's loss and gradient are the single-image call's, bit for bit.        */
int skp_sharpen_fwd_batch(const float* A, int nb, int T, int h, int w, float sigma, int num_subjects, float* pos,
                          double* partial, float* loss, void* stream);
int skp_sharpen_bwd_batch(const float* A, int nb, int T, int h, int w, float sigma, int num_subjects,
                          const float* pos, const float* gout, float* dA, void* stream);

/* ---------------------------------------------------------------- A12 warp / equivariance
 * F.grid_sample(x, F.affine_grid(theta), bilinear, zeros, align_corners=False)
 * (invertable_transform.py:64-70, 86-90).  x (B, C, H, W), theta (B, 2, 3) device. */
int skp_affine_warp(const float* x, int B, int C, int H, int W, const float* theta, float* out, void* stream);
/* Adjoint w.r.t. x; gin is OVERWRITTEN (zeroed then accumulated).               */
int skp_affine_warp_bwd(const float* gout, int B, int C, int H, int W, const float* theta, float* gin,
                        void* stream);

/* optimize.equivariance_loss (optimize.py:157-163) for one replica:
 * loss = mean((A − warp(At, theta_inv))²), theta_inv (2,3) the inverse of that
 * replica's theta (invertable_transform.py:72-92).  partial >= T doubles.        */
int skp_equiv_fwd(const float* A, const float* At, int T, int h, int w, const float* theta_inv,
                  double* partial, float* loss, void* stream);
/* dA = gout·2(A−A')/numel (optional), dAt = warpᵀ(−dA) (overwritten).          */
int skp_equiv_bwd(const float* A, const float* At, int T, int h, int w, const float* theta_inv,
                  const float* gout, float* dA, float* dAt, void* stream);
/* The equivariance loss of nb replicas at once: A, At (nb, T, h, w), theta_inv (nb, 2, 3),
 * loss (nb), partial >= nb·T doubles; backward with gout (nb).  Same per-image values.       */
int skp_equiv_fwd_batch(const float* A, const float* At, int nb, int T, int h, int w, const float* theta_inv,
                        double* partial, float* loss, void* stream);
int skp_equiv_bwd_batch(const float* A, const float* At, int nb, int T, int h, int w, const float* theta_inv,
                        const float* gout, float* dA, float* dAt, void* stream);

/* ---------------------------------------------------------------- Winograd as batched GEMMs
 * The frozen UNet's small-image 3×3 convolutions (SD-1.5 ResnetBlock2D conv1/conv2 at 8²-32²):
 * F(4×4, 3×3) with the fused kernels' points, as V = Bᵀ d B → M[p] = V[p]ᵀ U[p] (36 batched
 * library GEMMs, host side) → y = Aᵀ M A (+ bias[k]) (+ residual).
 * V (36, C, T) and M (36, T, K), T = B·(H/4)·(W/4) tiles, t = (b·H/4 + ty)·W/4 + tx.          */
int skp_wino_in_transform(const float* x, int B, int C, int H, int W, float* V, void* stream);
int skp_wino_out_transform(const float* M, int B, int K, int H, int W, const float* bias, const float* residual,
                           float* y, void* stream);
/* skp_wino_out_transform with the GEMM product laid out M[p][k][t] (the operands swapped: M[p] =
 * U[p]ᵀ · V[p]), so the tiles leave as coalesced image-row runs; gn_part (optional): the next
 * GroupNorm's (mean, M2) per (image, channel, segment of min(P, 64) tiles), P = (H/4)·(W/4) tiles per
 * plane (16, 32 or a multiple of 64), nseg = P / min(P, 64) — the layout skp_groupnorm_fwd_part
 * reads. */
int skp_wino_out_transform_kt(const float* M, int B, int K, int H, int W, const float* bias, const float* residual,
                              float* y, float* gn_part, void* stream);

/* ---------------------------------------------------------------- Q·Kᵀ (fp32 MFMA)
 * C[b,m,n] = alpha · Σ_k A[b,m,k] · B[b,k,n] (+ C if accumulate), arbitrary element
 * strides; exact-f32 v_mfma_f32_32x32x2_f32.  Used for the capture logits
 * z = q kᵀ·scale (ptp_utils.py:493/534) and their gradients.                   */
int skp_bgemm_f32(const float* A, long long sAb, long long sAm, long long sAk, const float* B, long long sBb,
                  long long sBk, long long sBn, float* C, long long sCb, long long sCm, long long sCn, int batch,
                  int M, int N, int K, float alpha, int accumulate, void* stream);
/* skp_bgemm_f32 with a two-level batch: batch index z = o·hb + i, operand X's base X + o·sXo + i·sXb.
 * Reads attention heads in place from the (B, S, H·d) projections (sXo = S·H·d, sXb = d, row stride
 * H·d) and an operand shared by the B images with sXo = 0 — the captured layers' q·kᵀ and P·v with
 * the batch-shared token embedding (ptp_utils.py:481-536) without head-permute or batch-expand copies.
 * skp_bgemm_f32 is the hb = batch, sXo = 0 case. */
int skp_bgemm_f32_2b(const float* A, long long sAo, long long sAb, long long sAm, long long sAk, const float* B,
                     long long sBo, long long sBb, long long sBk, long long sBn, float* C, long long sCo, long long sCb,
                     long long sCm, long long sCn, int batch, int hb, int M, int N, int K, float alpha, int accumulate,
                     void* stream);

/* ---------------------------------------------------------------- UNet-side: GroupNorm (+SiLU)
 * The token-opt backward runs through the frozen SD-1.5 UNet; its
 * GroupNorm → SiLU pairs (diffusers-0.8.0 ResnetBlock2D / Transformer2DModel.norm /
 * VAE encoder) run fused here.  x, y, dx: (B, C, HW) NCHW fp32; act = 1 applies SiLU.
 * shift (B*C floats, or NULL) is added to x on load: GroupNorm(x + shift[b, c]) — the
 * preceding convolution's bias and the resnet's time embedding, never materialised.
 * stats (B*G*2 floats) = (mean, rstd) per group, written by fwd and read by bwd.
 * partial: skp_groupnorm_workspace(B, C, HW, G) doubles.  Parameters are frozen, so the
 * backward returns dx only.                                                      */
int skp_groupnorm_workspace(int B, int C, long long HW, int G);
int skp_groupnorm_fwd(const float* x, const float* gamma, const float* beta, const float* shift, int B, int C,
                      long long HW, int G, float eps, int act, float* y, float* stats, double* partial,
                      void* stream);
int skp_groupnorm_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* shift,
                      const float* stats, int B, int C, long long HW, int G, int act, float* dx, double* partial,
                      void* stream);
/* skp_groupnorm_fwd with the statistics pass replaced by the producing convolution's per-segment
 * statistics: part (B, C, nseg) float2 (mean, M2 = Σ(x − mean)²) per segment of n = HW / nseg
 * pixels, as skp_conv3x3_wino2_gn / skp_wino_out_transform_kt write them; combined in fp64 by
 * Chan's formula with the shift folded into each segment mean.  Same output and saved
 * (mean, rstd) layout. */
int skp_groupnorm_fwd_part(const float* x, const float* gamma, const float* beta, const float* shift, const float* part,
                           int nseg, int B, int C, long long HW, int G, float eps, int act, float* y, float* stats,
                           double* partial, void* stream);
/* The statistics of skp_groupnorm_fwd / skp_groupnorm_fwd_part without the apply pass: stats
 * (B*G*2 floats) = the same (mean, rstd), for a consumer that normalises on load
 * (skp_wino2_vtransform_gn).  partial as above. */
int skp_groupnorm_stats(const float* x, const float* shift, int B, int C, long long HW, int G, float eps, float* stats,
                        double* partial, void* stream);
int skp_groupnorm_stats_part(const float* part, int nseg, const float* shift, int B, int C, long long HW, int G,
                             float eps, float* stats, double* partial, void* stream);
/* skp_groupnorm_bwd plus dres (may be null): dx = GroupNorm-backward(dy) + dres, the gradient of x's
 * other consumer (the ResNet block's residual or shortcut, the spatial transformer's residual) added
 * in the same pass instead of by the autograd engine (diffusers resnet.py / attention.py residuals). */
int skp_groupnorm_bwd_add(const float* x, const float* dy, const float* gamma, const float* beta, const float* shift,
                          const float* stats, int B, int C, long long HW, int G, int act, const float* dres, float* dx,
                          double* partial, void* stream);
/* Softmax backward of the UNet's math attention (diffusers-0.8.0 CrossAttention,
 * softmax(q kᵀ·scale) v): per row of P (rows × cols), dS = alpha·P ⊙ (dP − Σ P ⊙ dP),
 * written over dP (alpha = the logits' scale, baddbmm's backward folded in).  cols ≤ 16384. */
int skp_softmax_bwd(const float* P, float* dP, long long rows, int cols, float alpha, void* stream);
/* Its forward, in place: S (rows × cols, cols % 4 == 0, ≤ 16384) ← softmax over each row
 * (torch order: max-subtracted exp, divided by the row sum).  One read and one write of S
 * (the (B·H, 4096, 4096) scores of the 64²-token layers are 4.3 GB at batch 8).           */
int skp_softmax_fwd(float* S, long long rows, int cols, void* stream);
/* Fused score gradient of the math attention's backward: out = alpha·P ⊙ (dO·Vᵀ − D) with
 * dO·Vᵀ on the f32 matrix cores (never materialised) and D[row] = dO_row·O_row (the forward
 * output); P (BH, S, L), dO (BH, S, d), V (BH, L, d), D (BH, S).  out may alias P.
 * S, L multiples of 64; d ∈ {40, 64, 80, 160}.                                         */
int skp_attn_dscore(const float* P, const float* dO, const float* V, const float* D, float* out, int BH, int S, int L,
                    int d, float alpha, void* stream);
/* Fused attention backward over key blocks: dS = alpha·P⊙(dO·Vᵀ − D) written to dS (as
 * skp_attn_dscore) and, from the same registers, dV = Pᵀ·dO and dK = dSᵀ·Q (so dK carries
 * alpha).  P, dS (BH, S, L); dO, Q (BH, S, d); V, dV, dK (BH, L, d); D = rowsum(dO⊙O) (BH, S).
 * S, L multiples of 64; d ∈ {40, 64, 80}; dO, Q, V, dV, dK 16-byte aligned.  Replaces the
 * autograd backward of diffusers' CrossAttention baddbmm → softmax → bmm (attention.py).     */
int skp_attn_bwd_kv(const float* P, const float* dO, const float* Q, const float* V, const float* D, float* dS,
                    float* dV, float* dK, int BH, int S, int L, int d, float alpha, void* stream);
/* Fused attention O = softmax(scale·Q Kᵀ) V (online softmax; no score tensor); with stats
 * non-null also the per-row (max, 1/sum) pairs (BH, S, 2) that skp_attn_bwd_flash consumes.
 * Q (BH, S, d), K, V (BH, L, d), O (BH, S, d); S a multiple of 64, L any (the last key block
 * is masked); d ∈ {40, 64, 80}.                                                  */
int skp_attn_fwd(const float* Q, const float* K, const float* V, float* O, float* stats, int BH, int S, int L, int d,
                 float scale, void* stream);
/* Attention backward that rebuilds P = exp(scale·Q Kᵀ − m) · (1/l) per key block from the
 * forward's row stats (stats from skp_attn_fwd, (BH, S) × (m, 1/l)) instead of reading a saved P:
 * dS (BH, S, L) = scale·P⊙(dO·Vᵀ − D), dV = Pᵀ·dO, dK = dSᵀ·Q; dQ = dS·K is left to a GEMM.
 * Q, dO (BH, S, d); K, V, dV, dK (BH, L, d); D = rowsum(dO⊙O) (BH, S).  S a multiple of 64,
 * L any; d ∈ {40, 64, 80}; 16-byte aligned (stats 8).                                                  */
int skp_attn_bwd_flash(const float* Q, const float* K, const float* V, const float* dO, const float* stats,
                       const float* D, float* dS, float* dV, float* dK, int BH, int S, int L, int d, float scale,
                       void* stream);
/* skp_attn_fwd / skp_attn_bwd_flash on the projections' own layout, without the head permutes of
 * diffusers' reshape_heads_to_batch_dim / reshape_batch_dim_to_heads (CrossAttention.forward,
 * reference ptp_utils.py:481-506 for the layers the capture does not patch): element (b, h, s, j)
 * of Q / K / V / O / dO / dV / dK sits at base + b·sb + s·rs + h·d + j (a (B, S, H·d) tensor:
 * sb = S·H·d, rs = H·d; a context shared by the batch: sb = 0 — then dK / dV still get their own
 * per-image rows and the caller sums them).  stats (B·H, S, 2), D (B·H, S), dS (B·H, S, L)
 * contiguous, as in the (B·H, S, d) entries; strides multiples of 4, 16-byte aligned.         */
int skp_attn_fwd_bshd(const float* Q, long long q_sb, int q_rs, const float* K, long long k_sb, int k_rs,
                      const float* V, long long v_sb, int v_rs, float* O, long long o_sb, int o_rs, float* stats, int B,
                      int H, int S, int L, int d, float scale, void* stream);
int skp_attn_bwd_flash_bshd(const float* Q, long long q_sb, int q_rs, const float* K, long long k_sb, int k_rs,
                            const float* V, long long v_sb, int v_rs, const float* dO, long long o_sb, int o_rs,
                            const float* stats, const float* D, float* dS, float* dV, long long dv_sb, int dv_rs,
                            float* dK, long long dk_sb, int dk_rs, int B, int H, int S, int L, int d, float scale,
                            void* stream);
/* LayerNorm over the last dimension (the UNet transformer blocks' norm1/2/3; frozen γ, β):
 * x, y (rows, C), C a multiple of 4 ≤ 2048; stats (rows, 2) = (mean, 1/sqrt(var + eps)) for the
 * backward, which gives dx = rstd·(dy·γ − mean(dy·γ) − x̂·mean(dy·γ·x̂)).  Replaces
 * torch.nn.LayerNorm inside diffusers' BasicTransformerBlock (attention.py).               */
int skp_layernorm_fwd(const float* x, const float* gamma, const float* beta, long long rows, int C, float eps, float* y,
                      float* stats, void* stream);
int skp_layernorm_bwd(const float* x, const float* dy, const float* gamma, const float* stats, long long rows, int C,
                      float* dx, void* stream);
/* skp_layernorm_bwd plus dres (may be null): dx = LayerNorm-backward(dy) + dres, the transformer
 * block's residual gradient (h = attn(norm(h)) + h, diffusers attention.py) added in the same pass. */
int skp_layernorm_bwd_add(const float* x, const float* dy, const float* gamma, const float* stats, long long rows,
                          int C, const float* dres, float* dx, void* stream);
/* diffusers GEGLU (the UNet FeedForward's proj → chunk(2) → x·gelu(gate), exact-erf GELU):
 * h (rows, 2I) → out (rows, I), and its backward dh (rows, 2I) from dout (rows, I).
 * I % 4 == 0, 16-byte aligned.                                                 */
int skp_geglu_fwd(const float* h, long long rows, int I, float* out, void* stream);
int skp_geglu_bwd(const float* h, const float* dout, long long rows, int I, float* dh, void* stream);
/* out = a + (h + bias[c]) over (B, C, HW): diffusers ResnetBlock2D `x + conv2(...)` with the
 * convolution's bias folded into the residual add (same rounding order).         */
int skp_residual_bias_add(const float* a, const float* h, const float* bias, int B, int C, long long HW,
                          float* out, void* stream);
/* 3×3 / stride-1 / pad-1 convolution of the frozen VAE encoder and UNet (diffusers Conv2d in
 * Encoder / ResnetBlock2D / Upsample2D, run by ptp_utils.py:289-304 image2latent and the UNet
 * forward/backward of optimize.py:173-190) as Winograd F(4×4, 3×3) on the fp32 matrix cores.
 * skp_wino_weights: transformed weights U (K·C·36 floats, layout [K/32][C][32][36]) from
 *   w (K, C, 3, 3) (flip 0), or, for the input gradient, from the forward weight w (C, K, 3, 3)
 *   rotated 180° and transposed (flip 1).  K % 32 == 0.
 * skp_conv3x3_wino: y (B, K, H, W) = conv(x (B, C, H, W), w) + bias[k] (bias may be NULL)
 *   + residual (B, K, H, W) (may be NULL).  C % 4 == 0, K % 32 == 0, H % 4 == W % 4 == 0,
 *   16-byte aligned tensors.  nsplit > 1 splits the input channels over nsplit workgroup sets
 *   (C % (4·nsplit) == 0) for grids too small to fill the chip: partial sums go to ws
 *   (nsplit·B·K·H·W floats) and one pass adds them (in split order), the bias and the
 *   residual into y.  nsplit == 1: ws unused (may be NULL).                     */
int skp_wino_weights(const float* w, int K, int C, int flip, float* U, void* stream);
int skp_conv3x3_wino(const float* x, const float* U, const float* bias, const float* residual, float* y, int B, int C,
                     int K, int H, int W, int nsplit, float* ws, void* stream);
/* The same convolution for H % 32 == W % 32 == 0 (workgroup = 32×32 output pixels × 32
 * channels, three stages of input region and weights in flight, transforms straight into the
 * MFMA operands).  skp_wino2_weights writes U as [K/32][C][32][40] (positions 0..17 at 0..17,
 * 18..35 at 20..37, zero pads); flip as above.  Also 16×16 images with B % 4 == 0 (four
 * whole images per workgroup).  */
int skp_wino2_weights(const float* w, int K, int C, int flip, float* U, void* stream);
int skp_conv3x3_wino2(const float* x, const float* U, const float* bias, const float* residual, float* y, int B,
                      int C, int K, int H, int W, int nsplit, float* ws, void* stream);
/* skp_conv3x3_wino2 that also writes the next GroupNorm's statistics from its epilogue: gn_part
 * (B, K, H/16 · W/32) float2 = (mean, M2 = Σ(y − mean)²) of the final output (bias and residual
 * included) per channel over each 16-row × 32-pixel segment, accumulated around a pivot value of
 * the segment (nsplit = 1, H and W multiples of 32; may be null).  The
 * consumer is skp_groupnorm_fwd_part: the frozen UNet / VAE's GroupNorm(+SiLU) after a 3×3 convolution
 * (diffusers resnet.py) then reads its input once instead of twice. */
int skp_conv3x3_wino2_gn(const float* x, const float* U, const float* bias, const float* residual, float* y, int B,
                         int C, int K, int H, int W, int nsplit, float* ws, float* gn_part, void* stream);
/* The same convolution with the input transform done once instead of by each of the K/32 channel-block
 * workgroups: the V-staged pair for the frozen, gradient-free VAE encoder's GroupNorm → SiLU → 3×3
 * convolution (diffusers ResnetBlock2D inside Encoder, ptp_utils.py:289-304 image2latent).
 * skp_wino2_vtransform: V = Bᵀ d B of every 4×4 tile of d = x (B, C, H, W), zero padded; H, W
 *   multiples of 32, C % 4 == 0.  V holds B·C·H·W/16·36 floats, no padding: per half-height block
 *   (8 × 4 tiles, blocks in image, row, column order) and 4-channel stage one 18-KB slab
 *   [wave q][chunk j][lane L], lane-major for the wave that consumes it: q = 2·half + wm (half 0 /
 *   1 = transform rows 0-2 / 3-5, i.e. positions 0..17 / 18..35; wm = tile rows 2wm, 2wm + 1 of the
 *   block), lane L = (stage channel L >> 4, tile 16·wm + (L & 15) of the block's 32), and the
 *   lane's 18 positions as chunks j = 0..3 of 16 B (64 lanes × 16 B = 1 KB each, positions
 *   4j..4j + 3 of the half) and chunk 4 of 8 B (512 B, positions 16, 17): 4.5 KB per wave.
 * skp_wino2_vtransform_gn: the same with d = act(GroupNorm(x + shift)) computed on load from
 *   stats (B·G·2 floats (mean, rstd), from skp_groupnorm_stats / _stats_part or a forward),
 *   gamma, beta and shift (B·C floats or NULL): bit for bit the values skp_groupnorm_fwd writes,
 *   never stored; the padding is of d, not of x.  One pass: reads x (4 B per element), writes V
 *   (36 floats per 16 = 9 B per element); the convolution's first read of V is 9 B per element.
 * skp_conv3x3_wino2_v / _v_gn: skp_conv3x3_wino2 / _gn with V in place of x; same U, epilogues,
 *   nsplit / ws and gn_part, and the same bits as skp_conv3x3_wino2 on d at the same nsplit. */
int skp_wino2_vtransform(const float* x, float* V, int B, int C, int H, int W, void* stream);
int skp_wino2_vtransform_gn(const float* x, const float* stats, const float* gamma, const float* beta,
                            const float* shift, int G, int act, float* V, int B, int C, int H, int W, void* stream);
int skp_conv3x3_wino2_v(const float* V, const float* U, const float* bias, const float* residual, float* y, int B,
                        int C, int K, int H, int W, int nsplit, float* ws, void* stream);
int skp_conv3x3_wino2_v_gn(const float* V, const float* U, const float* bias, const float* residual, float* y, int B,
                           int C, int K, int H, int W, int nsplit, float* ws, float* gn_part, void* stream);
/* diffusers' Downsample2D(padding=0) of the VAE encoder (F.pad(x, (0, 1, 0, 1)) then a 3×3 stride-2
 * convolution; the encoder behind ptp_utils.image2latent, reference ptp_utils.py:289-304):
 * y (B, K, H/2, W/2), + bias, in the stride-2 minimal-product form: 2×2 output tiles (input pitch 4,
 * the 5×5 sub-patch of rows / columns 1..5 of skp_conv3x3_wino2's 6×6 patch) from 25 products, against
 * 36 per 4 kept outputs for the stride-1 kernel sampled at the odd positions; every input-transform
 * coefficient is 0 or ±1.
 *   V = Bs2ᵀ d Bs2, U = Gs2 g Gs2ᵀ, Y = As2ᵀ (Σc U ⊙ V) As2 with
 *   Bs2ᵀ = [1 0 −1 0 0; 0 0 1 0 0; 0 0 1 0 −1; 0 1 0 0 0; 0 0 0 1 0], Gs2 = [1 0 0; 1 0 1; 0 0 1; 0 1 0; 0 1 0],
 *   As2ᵀ = [1 1 0 1 0; 0 1 −1 0 1].
 * skp_wino2s2_weights writes U (fp64 → fp32) as [K/32][C][32][28]: positions 5i + j of rows i = 0..2
 * at 0..14, of rows 3..4 at 16..25, zero pads.  skp_conv3x3s2_f2: H, W multiples of 32; C % 4 == 0,
 * K % 32 == 0; nsplit as skp_conv3x3_wino2 (workspace nsplit·B·K·(H/2)·(W/2) floats).            */
int skp_wino2s2_weights(const float* w, int K, int C, float* U, void* stream);
int skp_conv3x3s2_f2(const float* x, const float* U, const float* bias, float* y, int B, int C, int K, int H, int W,
                     int nsplit, float* ws, void* stream);

/* ---------------------------------------------------------------- A17 visualisation sheets
 * Per-map (min, max) for the heat overlay: the normalisation of visualize.py:60-61
 * (save_grid: map − min, then / max).  maps (n, h, w) -> range (n, 2).  A map that holds a NaN
 * or ±inf, or whose max equals its min, gets (NaN, NaN), which the sheet reads as "no
 * overlay".  16-B loads when h·w % 4 == 0 and maps is 16-B aligned, scalar loads otherwise;
 * bit-exact (min/max do not depend on the order).                                          */
int skp_map_range(const float* maps, int n, int h, int w, float* range, void* stream);
/* One uint8 RGB sheet of rows × cols tiles, replacing the matplotlib figures of
 * visualize.py:105-138 (plot_point_correspondences: images with one marker per keypoint) and
 * visualize.py:40-73 (save_grid: images under the normalised map at alpha 0.7).
 *   images (n, 3, H, W) in [0, 1]; maps (n, h, w) or NULL; range (n, 2) from skp_map_range;
 *   lut (256, 3) in [0, 1]; points (n, K, 2) normalised (row, col) or NULL / K == 0;
 *   colors (K, 3) uint8; out (rows·(th+pad)+pad, cols·(tw+pad)+pad, 3) uint8, th = H/f,
 *   tw = W/f.  Tile t (row-major) shows image t; tiles t >= n and all padding are 255.
 * Output pixel (y, x) of tile t, in fp32: the mean over its f×f source pixels of
 * comp = img (no map, or range[t] NaN) or (1−alpha)·img + alpha·LUT(v),
 * v = clamp((m − mn)/(mx − mn), 0, 1), m = the map sampled bilinearly (align_corners=False, as
 * skp_resize_bilinear) at the source pixel, LUT(v) linear between entries floor(255v) and the
 * next; byte = floor(clamp(c, 0, 1)·255 + 0.5).  Then markers j = 0 … K−1 in order (the last
 * wins) with centre (py·th, px·tw): d² = (y+0.5−py·th)² + (x+0.5−px·tw)² <= radius² paints
 * colors[j], else d² <= (radius+1)² paints white; a NaN coordinate paints nothing; a marker
 * never leaves its tile.  A gather (one thread per output pixel, no atomics): deterministic.
 * Rejected: H % f or W % f != 0, n > rows·cols, maps without range or lut, K > 64, a sheet
 * of 2^31 bytes or more.                                                                   */
int skp_render_sheet(const float* images, int n, int H, int W, const float* maps, int h, int w, const float* range,
                     const float* lut, float alpha, const float* points, int K, float radius,
                     const unsigned char* colors, int rows, int cols, int f, int pad, unsigned char* out,
                     void* stream);

/* ---------------------------------------------------------------- A18 test-time-augmentation reduce
 * The tail of eval.run_image_with_context_augmented (eval.py:327-355: sum_samples +=
 * inverse(maps), num_samples += inverse(ones), sum / num, NaN -> 0) followed by eval.find_max_pixel
 * (eval.py:39-60), for B images at once without the full-size sums in memory.
 *   maps (B, C, n, S, S): n token maps of C warped copies of each image; theta_inv (B, C, 2, 3):
 *   each copy's inverse theta; pos (B, n, 2) = (row + 0.5, col + 0.5); avg (B, n, S, S) or NULL.
 * For image b, token t and pixel p, with the grid and bilinear sample of skp_affine_warp:
 *   sum = Σ_c sample(maps[b,c,t], grid(theta_inv[b,c], p)),  num = Σ_c sample(ones, …),
 *   a = sum / num with NaN -> 0;  pos[b,t] = first-occurrence row-major argmax of a;  avg[b,t,p] = a.
 * Both sums start from 0.0f and add in copy order c = 0 … C−1, the quotient is IEEE: bit-identical
 * to skp_affine_warp per copy, `acc = acc + warped`, the division, the NaN fix and skp_argmax2d.
 * workspace: skp_tta_reduce_workspace(B, n, S) bytes (−1 on a bad shape), 8-B aligned: one
 * (value, index) partial per image, token and 64 × 4-pixel tile.  Two launches (tiles, then one
 * merge per image and token; the greater value wins, on equal values the lower index), no atomics:
 * deterministic.
 * Rejected before any launch: null pointers (avg excepted), non-positive sizes, S < 2,
 * B·C·n·S² >= 2^31, B > 65535, a misaligned workspace.                                                       */
int skp_tta_reduce_workspace(int B, int n, int S);
int skp_tta_reduce(const float* maps, int B, int C, int n, int S, const float* theta_inv, float* pos, float* avg,
                   void* workspace, void* stream);

/* The scored TTA reduce: skp_tta_reduce (eval.py:327-355, then eval.find_max_pixel, eval.py:39-60)
 * and, in the same passes and without the average in memory, three scores per image and token and
 * the eval.pixel_from_weighted_avg centroid (eval.py:113-155) around the peak.
 *   pos, avg: skp_tta_reduce's, bit for bit.  refined (B, n, 2), scores (B, n, 3).  With a the
 *   average of image b and token t, (r*, c*) its argmax and K the pixels (r, c) with
 *   sqrt((r − r*)² + (c − c*)²) <= distance in float:
 *   scores[b,t,0] = a[r*, c*]                                         (the peak)
 *   scores[b,t,1] = (float)(Σ_K a / (Σ a + 1e-6)), both sums in double   (the concentration)
 *   scores[b,t,2] = num[r*, c*] / C, num = Σ_c sample(ones, …)          (the coverage)
 *   refined[b,t]  = (Σ_K r·(a / denom) + 0.5, Σ_K c·(a / denom) + 0.5), denom = (float)Σ_K a + 1e-6f,
 *                   the products in float, their sums in double: skp_weighted_avg's arithmetic.
 * Three launches, no atomics: the tile kernel also leaves each tile's Σ a (double from the lane
 * upward, a fixed tree), the merge sums them in a fixed order, and one workgroup per image and
 * token recomputes a on the box r* ± ⌊distance⌋, c* ± ⌊distance⌋ (clipped to the plane) with the
 * tile kernel's arithmetic.  Deterministic.  A token whose maps hold NaN or inf gets unspecified
 * scores.
 * workspace: skp_tta_reduce_scored_workspace(B, n, S) bytes (−1 on a bad shape), 8-B aligned.
 * Rejected before any launch: what skp_tta_reduce rejects, a null refined or scores, and a
 * distance outside (0, 16].                                                                    */
int skp_tta_reduce_scored_workspace(int B, int n, int S);
int skp_tta_reduce_scored(const float* maps, int B, int C, int n, int S, const float* theta_inv, float distance,
                          float* pos, float* refined, float* scores, float* avg, void* workspace, void* stream);

/* The k-peak TTA reduce: skp_tta_reduce (eval.py:327-355) then eval.find_k_max_pixels with its
 * mask_radius (eval.py:62-111) on the average, without the average in memory.
 *   pos (B, n, num, 2): round j's (row + 0.5, col + 0.5); values (B, n, num): the value that won
 *   round j, read from the average after j masks; avg (B, n, S, S) optional: the unmasked average,
 *   skp_tta_reduce's bit for bit.
 * Equal to skp_tta_reduce(…, avg) followed by skp_k_max_pixels(avg, num, radius2), and to
 * skp_argmax2d and skp_mask_radius in turn: round 0 is the first-occurrence row-major argmax; before
 * round j every earlier pick p has multiplied the map by (dx² + dy² > radius2) ? 1.0f : 0.0f,
 * dx = (float)col − (col_p + 0.5f), dy likewise.  A multiply, not a fill: a masked pixel is 0 and
 * can still win, +inf · 0 is NaN, NaN wins an argmax and the lowest index wins among NaNs.
 * Round 0 is skp_tta_reduce's two launches; each later round recomputes only the 64 × 4-pixel tiles
 * that meet the box around the newest pick (at S = 512 and radius 25.6 at most 28 of 1024) and
 * merges again: 2 + 2(num − 1) launches, no atomics, deterministic.
 * workspace: skp_tta_reduce_peaks_workspace(B, n, S, num, radius2) bytes (−1 on a bad shape, num
 * or radius2), 8-B aligned: skp_tta_reduce's partials and one index per image, token and round.
 * Rejected before any launch: what skp_tta_reduce rejects, a null values, num outside [1, 16], a
 * radius2 that is not positive and finite.                                                     */
int skp_tta_reduce_peaks_workspace(int B, int n, int S, int num, float radius2);
int skp_tta_reduce_peaks(const float* maps, int B, int C, int n, int S, const float* theta_inv, int num,
                         float radius2, float* pos, float* values, float* avg, void* workspace, void* stream);

/* The entropy TTA reduce: skp_tta_reduce (eval.py:327-355, then eval.find_max_pixel, eval.py:39-60)
 * and, in the same pass and without the average in memory, the key eval.find_corresponding_points
 * (eval.py:159-195) ranks tokens by: the Shannon entropy of the softmax of each averaged plane.
 *   pos, avg: skp_tta_reduce's, bit for bit.  entropy (B, n) double.  With a the fp32 average of
 *   image b and token t (after NaN -> 0), z = (double)scale · (double)a over its S² pixels and
 *   m = max z:   entropy[b,t] = −Σ p·log p,  p = e^{z−m} / Σ e^{z−m}
 *              = log S0 − T / S0,  S0 = Σ e^{z−m},  T = Σ (z−m)·e^{z−m},
 *   in double; a pixel with e^{z−m} == 0 (a = −inf among them) adds 0 to T, and a maximum of +inf
 *   gives NaN.  A plane of equal values gives log S².
 * Two launches, no atomics: the tile kernel (grid tiles × B × chunks of 10 tokens) leaves (S0, T)
 * about each tile's maximum beside its partial — lanes about their wave's maximum in a fixed tree,
 * then the four waves in order, rescaled by e^{scale·(m_wave − m_tile)} — and the merge takes in the
 * tiles about the plane's maximum the same way (lane k tiles k, k + 64, … in order, then the tree).
 * Deterministic, and the same whether or not avg is asked for.
 * workspace: skp_tta_reduce_entropy_workspace(B, n, S) bytes (−1 on a bad shape), 8-B aligned:
 * skp_tta_reduce's partials and two doubles per image, token and tile.
 * Rejected before any launch: what skp_tta_reduce rejects, a null entropy, a scale that is not
 * positive and finite, n > 655350.                                                             */
int skp_tta_reduce_entropy_workspace(int B, int n, int S);
int skp_tta_reduce_entropy(const float* maps, int B, int C, int n, int S, const float* theta_inv, float scale,
                           float* pos, double* entropy, float* avg, void* workspace, void* stream);

/* The part TTA reduce: skp_tta_reduce (eval.py:327-355, then eval.find_max_pixel, eval.py:39-60)
 * and, in the same pass and without the average in memory, the reduction over the TOKEN axis at
 * every pixel: which token holds the greatest average there, that average, and the tokens' sum.
 *   pos, avg: skp_tta_reduce's, bit for bit.  label (B, S, S) int16, value (B, S, S), mass (B, S, S).
 *   With a[b,t,p] the fp32 average of image b, token t and pixel p (after NaN -> 0):
 *   value[b,p] = max_t a[b,t,p];
 *   label[b,p] = the lowest t with a[b,t,p] == value[b,p]: a strict > walking t = 0 … n−1 (a holds
 *                no NaN, so this is a total order; ±inf are ordinary values);
 *   mass[b,p]  = Σ_t a[b,t,p] in this order: chunk k holds tokens 10k … min(10k + 9, n−1); each
 *                chunk's sum starts from 0.0f and adds in token order; the chunks' sums are added in
 *                chunk order, again from 0.0f; every add rounded on its own.  For n <= 10 this is
 *                the plain sequential sum.  The order is what lets the chunks run in different
 *                workgroups and give the same bits.
 * No background decision is made here: a pixel that no copy covers has a = 0 for every token and
 * gets label 0, value 0, mass 0.
 * Two or three launches, no atomics: the tile kernel (grid tiles × B × chunks of 10 tokens) leaves
 * skp_tta_reduce's partials, and each thread carries its pixel's (value, label, mass) through its
 * chunk's passes; with one chunk it stores the three outputs, with more it stores a partial per
 * image, chunk and pixel, and a per-pixel merge walks the chunks in order (strict >, the earlier
 * chunk keeps a tie); then the merge for pos.  Deterministic, and the same whether or not avg is
 * asked for.
 * workspace: skp_tta_reduce_parts_workspace(B, n, S) bytes (−1 on a bad shape or at 2^31 bytes),
 * 8-B aligned: skp_tta_reduce's partials and, with chunks = ⌈n / 10⌉ > 1 and Q = B·chunks·S², two
 * floats and an int16 per partial, each array rounded up to 8 bytes: 8·B·n·T + 2·r8(4Q) + r8(2Q).
 * Rejected before any launch: what skp_tta_reduce rejects, a null label, value or mass, n > 32767,
 * more than 65535 chunks.                                                                      */
int skp_tta_reduce_parts_workspace(int B, int n, int S);
int skp_tta_reduce_parts(const float* maps, int B, int C, int n, int S, const float* theta_inv, float* pos,
                         short* label, float* value, float* mass, float* avg, void* workspace, void* stream);

/* The match TTA reduce: skp_tta_reduce (eval.py:327-355, then eval.find_max_pixel, eval.py:39-60)
 * and, in the same pass and without the average in memory, the combination ACROSS the tokens with the
 * caller's weights: at every pixel the n averages are a signature, and each of Q query signatures is
 * matched against every pixel by its cosine score (no reference function: few-shot transfer of
 * annotated points).
 *   pos, avg: skp_tta_reduce's, bit for bit.  queries (Q, n) row-major, 1 <= Q <= 16.  match_pos
 *   (B, Q, 2), match_score (B, Q), score_map (B, Q, S, S) or NULL.
 *   With a[b,t,p] the fp32 average of image b, token t and pixel p (after NaN -> 0) and d = queries:
 *   nrm[b,p]     = Σ_t a·a,   dot[b,q,p] = Σ_t a·d[q,t],  both in this order: chunk k holds tokens
 *                  10k … min(10k + 9, n−1); each chunk's sums start from 0.0f and add in token order;
 *                  the chunks' sums are added in chunk order, again from 0.0f; every product and
 *                  every add rounded on its own (no fma).  The part reduce's mass order.
 *   score[b,q,p] = dot / sqrt(nrm), both correctly rounded; −inf where nrm is not > 0 (a pixel that
 *                  no copy covers, an all-zero signature) and where the quotient is NaN (an infinite
 *                  average): a score is never NaN, the order is total.
 *   match_pos[b,q] = (row + 0.5, col + 0.5) of the first row-major maximum of score[b,q] over the S²
 *                  pixels, match_score[b,q] that maximum; (0.5, 0.5) and −inf where every score is
 *                  −inf.  score_map[b,q,p] = score[b,q,p] where it is given.
 * Three or four launches, no atomics: the tile kernel (grid tiles × B × chunks of 10 tokens) leaves
 * skp_tta_reduce's partials, and each thread carries its pixel's nrm and Q dots through its chunk's
 * passes; with one chunk it forms the scores and the workgroup leaves one (score, pixel) partial per
 * image, query and tile, with more it stores Q + 1 floats per image, chunk and pixel, and a
 * per-pixel merge walks the chunks in order, forms the scores and leaves one partial per image,
 * query and 64 pixels; then the merge for pos, and the same merge over the queries' partials.
 * Deterministic, and the same whether or not score_map or avg is asked for.
 * workspace: skp_tta_reduce_match_workspace(B, n, S, Q) bytes (−1 on a bad shape or Q, or at 2^31
 * bytes), 8-B aligned: skp_tta_reduce's partials, with chunks = ⌈n / 10⌉ > 1 the (Q + 1)·B·chunks·S²
 * floats, and two arrays of B·Q·R words, R = T tiles (one chunk) or ⌈S² / 64⌉, each array rounded
 * up to 8 bytes: 8·B·n·T + [chunks > 1] r8(4(Q + 1)·B·chunks·S²) + 2·r8(4·B·Q·R).
 * Rejected before any launch: what skp_tta_reduce rejects, a null queries, match_pos or
 * match_score, Q outside [1, 16], more than 65535 chunks.                                       */
int skp_tta_reduce_match_workspace(int B, int n, int S, int Q);
int skp_tta_reduce_match(const float* maps, int B, int C, int n, int S, const float* theta_inv, const float* queries,
                         int Q, float* pos, float* match_pos, float* match_score, float* score_map, float* avg,
                         void* workspace, void* stream);

/* The dense nearest-pixel field (no reference function: transfer of everything an exemplar carries):
 * for every pixel p of X the pixel q of Y whose signature has the greatest cosine, on the exact-f32
 * matrix cores, the (P, Q) product never leaving registers.
 *   x: image b's signatures at x + b·x_stride, token-major (n, P): element (t, p) at t·P + p, an
 *   (n, S, S) TTA average as it lies in memory; a stride of 0 is one operand shared by the B images.
 *   y likewise with Q columns.  index (B, P) int32, score (B, P) float32.
 *   Per image, every operation fp32 and rounded on its own:
 *   nx[p]     = c_n with c_0 = 0.0f, c_{t+1} = fmaf(x[t,p], x[t,p], c_t); ny[q] likewise.  A column is
 *               usable where 0 < norm < +inf (not a zero column, nor one holding a NaN or an infinity).
 *   rx[p]     = 1.0f / sqrt(nx[p]), both correctly rounded; ry[q] likewise.
 *   dot[p,q]  = d_n with d_0 = 0.0f, d_{t+1} = fmaf(x[t,p], y[t,q], d_t), in token order: one
 *               accumulator per (p, q), no split over the tokens.
 *   key[p,q]  = dot · ry[q]; a NaN key counts as −inf.
 *   index[p]  = the lowest usable q with the greatest key, for a usable p;
 *   score[p]  = key[p,index[p]] · rx[p];  index = −1 and score = −inf where p is not usable or no q is.
 * A key depends neither on the tile of p or q, nor on the split of Q, nor on the image's place in the
 * batch.  Two launches, no atomics: the field kernel (one workgroup per image, 128 p and split of Q;
 * it forms the norms from the panels it streams and leaves one (key, q) partial per p) and the merge
 * over the splits in split order (the greater key wins, on equal keys the lower q).
 * workspace: skp_match_field_workspace(B, n, P, Q) bytes (−1 on a bad shape, or at 2^31 bytes), 8-B
 * aligned: r8(4·B·P) + 2·r8(4·B·splits·P) with splits <= 32 — never of the order of P·Q.
 * Rejected before any launch: a null pointer; B, n, P or Q below 1; n > 4096; P or Q above 2^20; a
 * non-zero stride below n·P or n·Q.                                                             */
int skp_match_field_workspace(int B, int n, int P, int Q);
int skp_match_field(const float* x, long long x_stride, int P, const float* y, long long y_stride, int Q, int B,
                    int n, int* index, float* score, void* workspace, void* stream);

/* The windowed refine of a coarse field (no reference function: coarse-to-fine dense matching): for
 * every pixel p of X's S × S grid the best pixel q of Y's grid inside a (2w + 1)² window whose centre
 * a coarse field gives, one prior per f × f cell of X's grid.  With f = 1 it re-matches around any
 * prior field.
 *   x, y, x_stride, y_stride, index (B, S²) int32 and score (B, S²) float32: skp_match_field's with
 *   P = Q = S², token-major (n, S²), a stride of 0 one operand shared by the B images.
 *   coarse (B, Sc²) int32, Sc = S / f: per cell of X's grid a cell of Y's grid, row·Sc + col.
 *   Per image, every operation fp32 and rounded on its own:
 *   nx, ny, usable, rx, ry, dot[p,q] (the fmaf chain in token order, one accumulator per (p, q), no
 *   split over the tokens) and key[p,q] = dot · ry[q], a NaN key counting as −inf, are skp_match_field's
 *   word for word: a key here is bit for bit the key there.
 *   Window: for p = (r, c), m = coarse[b, (r / f)·Sc + c / f]; p has no prior where m < 0 or m >= Sc².
 *               (cr, cc) = ((m / Sc)·f + r % f, (m % Sc)·f + c % f); W(p) = every q = (qr, qc) of the
 *               plane with |qr − cr| <= w and |qc − cc| <= w: clipped at the borders, never empty.
 *   index[p]  = the lowest usable q in W(p) with the greatest key;  score[p] = that key · rx[p];
 *               −1 and −inf where p is not usable, where p has no prior, or where no q in W(p) is
 *               usable.  Nothing outside the two planes is read, whatever coarse holds.
 * A result depends neither on how pixels are grouped into workgroups nor on the image's place in the
 * batch.  One launch, no atomics: one workgroup per image and cell takes the (f + 2w)² region of y that
 * the cell's windows share through LDS in passes, a register-blocked fmaf kernel with the norms
 * riding along and the (key, q) fold in registers.  Two runs give the same bits.
 * workspace: skp_match_refine_workspace(B, n, S, f, w) bytes (−1 on a bad shape, or at 2^31 bytes),
 * 8-B aligned: 8 — the kernel keeps nothing in memory, no copy of y and nothing of the order of
 * S²·(2w + 1)²; the pointer is checked and otherwise unused.
 * Rejected before any launch: a null pointer; B, n or S below 1; n > 4096; S > 1024; f outside [1, 8]
 * or S % f != 0; w outside [1, 16]; a non-zero stride below n·S²; B·Sc² of 2^31 or more.          */
int skp_match_refine_workspace(int B, int n, int S, int f, int w);
int skp_match_refine(const float* x, long long x_stride, const float* y, long long y_stride, int B, int n, int S,
                     const int* coarse, int f, int w, int* index, float* score, void* workspace, void* stream);

/* The k best matches of a window centred on the pixel (no reference function: the search of label
 * propagation through a video, where x is the current frame and the B images are its context frames).
 *   x, y, x_stride, y_stride: skp_match_refine's, token-major (n, S²), a stride of 0 one operand shared
 *   by the B images.  index (B, K, S²) int32 and score (B, K, S²) float32.
 *   Per image, every operation fp32 and rounded on its own:
 *   nx, ny, usable, rx, ry, dot[p,q] (the fmaf chain in token order, one accumulator per (p, q), no
 *   split over the tokens) and key[p,q] = dot · ry[q], a NaN key counting as −inf, are skp_match_field's
 *   word for word: a key here is bit for bit the key there.
 *   Window: for p = (r, c), W(p) = every q = (qr, qc) of the plane with |qr − r| <= w and |qc − c| <= w:
 *               clipped at the borders, never empty.
 *   Slot i of pixel p: the i-th usable q of W(p) in the order (key descending, q ascending) in
 *               index[b, i, p] and that key · rx[p] in score[b, i, p]; −1 and −inf where p is not
 *               usable or fewer than i + 1 usable q lie in W(p).
 *   So slot 0 is skp_match_refine with f = 1 and coarse[p] = p bit for bit, whatever K, and the first
 *   K' slots of a K-list are the K'-list.  A result depends neither on how pixels are grouped into
 *   workgroups, nor on the image's place in the batch, nor on what the buffers held before.  Nothing
 *   outside the two planes is read.
 * One launch, no atomics: one workgroup per image and 4 × 4 tile of x takes the (4 + 2w)² region of y
 * that the tile's windows share through LDS in passes, a register-blocked fmaf kernel with the norms
 * riding along; each pass's scaled keys go to LDS and the waves fold them into the tile's K-lists by K
 * rounds of (key, q) maxima, pairs compared in full.  Two runs give the same bits.
 * workspace: skp_match_topk_workspace(B, n, S, w, K) bytes (−1 on a bad shape, or at 2^31 bytes), 8-B
 * aligned: 8 — the kernel keeps nothing in memory, no copy of y and nothing of the order of
 * S²·(2w + 1)²; the pointer is checked and otherwise unused.
 * Rejected before any launch: a null pointer; B, n or S below 1; n > 4096; S > 1024; w outside
 * [1, 16]; K outside [1, 16]; a non-zero stride below n·S²; B·⌈S / 4⌉² of 2^31 or more.             */
int skp_match_topk_workspace(int B, int n, int S, int w, int K);
int skp_match_topk(const float* x, long long x_stride, const float* y, long long y_stride, int B, int n, int S,
                   int w, int K, int* index, float* score, void* workspace, void* stream);

/* The vote of label propagation (no reference function): per pixel the Kv best of M context frames'
 * K-lists, weighted by a softmax of their scores, vote with their own soft labels.
 *   index, score (M, K, S²): what skp_match_topk wrote with B = M.  An index outside [−1, S²) is
 *   treated as −1, and so is an entry whose score is NaN (skp_match_topk writes neither).
 *   labels (M, Cl, S²) float32: the context frames' soft labels, non-negative and finite; anything
 *   else gives unspecified values, never a read outside the buffers.
 *   Per pixel p: the candidates are the (j, i) with index[j, i, p] >= 0; ranks 1 … m, m <= Kv, are the
 *   first in the order (score descending, j ascending, i ascending); (j_i, q_i, s_i) is rank i's
 *   context, index and score.  Every operation fp32 and rounded on its own, no fma:
 *   d_i = s_i − s_1;  a_i = d_i · inv_tau;  e_i = expf(a_i);
 *   Z = (…(e_1 + e_2) + …) + e_m;  soft[c, p] = ((…(e_1·l_1 + e_2·l_2) + …) + e_m·l_m) / Z with
 *   l_i = labels[j_i, c, q_i], products and sums in rank order.
 *   expf is the HIP device library's (ocml) single-precision exp, whose documented error bound is
 *   1 ulp; everything else is correctly rounded.  Scores that are all finite are assumed: s_1 = ±inf
 *   gives NaN weights.
 *   label[p] = the lowest c with the greatest soft[c, p]; confidence[p] = that value.
 *   source (Kv, S²) int32, or null: j_i · S² + q_i at rank i, −1 from rank m on.
 *   A pixel without a candidate gets soft 0, label −1, confidence 0.
 * soft (Cl, S²), label (S²) int32, confidence (S²).  One launch, one thread per pixel, Kv scans of the
 * M·K candidates; no atomics, no workspace.
 * Rejected before any launch: a null pointer except source; M, K, S or Cl below 1; M > 64; K > 16; Kv
 * outside [1, K]; Cl > 256; S > 1024; inv_tau not finite or not positive.                           */
int skp_label_vote(const int* index, const float* score, int M, int K, int S, const float* labels, int Cl,
                   float inv_tau, int Kv, float* soft, int* label, float* confidence, int* source, void* stream);

/* Keypoint tracks over a sequence of frames (no reference function: visualize.create_vid takes
 * find_max_pixel frame by frame): per token the MAP path of a hidden Markov model over the pixel grid,
 * the emission a frame's TTA average, the transition a truncated Gaussian random walk.  One
 * skp_track_step per frame, in frame order, then one skp_track_backtrace.
 *   Per token, frames t = 0 … T−1, a_t (S, S) the frame's average, w[0..r] the caller's table.  Every
 *   operation fp32 and rounded on its own, no fma:
 *   frame 0:  m_0 = a_0, back_0 = the centre code everywhere.
 *   M_t       = max_p m_t(p); best_t = the first row-major index attaining it.
 *   m̃(q)      = m_{t−1}(q) / M_{t−1}; where M_{t−1} is 0 or not finite (a blank plane) m̃ ≡ 1.0f: the
 *               track restarts.
 *   row stage:    g(y', x) = max over dx ∈ [−r, r] with 0 <= x + dx < S of m̃(y', x + dx) · w[|dx|],
 *                 gdx(y', x) the smallest dx that attains it.
 *   column stage: h(y, x) = max over dy ∈ [−r, r] with 0 <= y + dy < S of g(y + dy, x) · w[|dy|],
 *                 dy* the smallest dy that attains it, dx* = gdx(y + dy*, x).
 *   m_t(y, x)    = a_t(y, x) · h(y, x);   back_t(y, x) = (dy* + r)·(2r + 1) + (dx* + r), int16.
 *   The two stages are the definition: a one-stage maximum over (dy, dx) has the same value (the
 *   Gaussian is a product of one factor per axis) but can break ties inside a row differently.
 *   A back-pointer always names a pixel of the plane.  Planes that hold NaN, an infinity or a
 *   negative value give that token unspecified tracks, never a back-pointer outside the plane.
 *   Backtrace: p_{T−1} = best_{T−1}, p_{t−1} = p_t + the (dy, dx) that back_t(p_t) encodes;
 *   pos[t, j] = (row + 0.5, col + 0.5) of p_t, skp_argmax2d's convention.
 * skp_track_step: avg, prev_score, score (n, S, S); prev_max, score_max (n); best (n) int32; back
 *   (n, S, S) int16.  prev_score and prev_max are null together for frame 0.  w_host: r + 1 floats in
 *   HOST memory, read during the call and passed to the kernel by value.  Two launches, no atomics:
 *   the tile kernel (one workgroup per token and 32 × 32 pixels: the tile of prev_score and its halo
 *   of r to LDS, divided on the way in; the row stage to LDS; the column stage from it; times avg)
 *   leaves one (max, first index) partial per tile, and the merge takes each token's.  Deterministic.
 *   workspace: skp_track_step_workspace(n, S, r) bytes (−1 on a bad shape, or at 2^31 bytes), 8-B
 *   aligned: 2·r8(4·n·tiles), tiles = ⌈S / 32⌉².
 * skp_track_backtrace: back (T, n, S, S) — the steps' back planes in frame order; best_last (n) the
 *   last step's best; pos (T, n, 2).  One launch, one thread per token walks the T dependent loads.  A
 *   code or an index outside its range (a buffer the steps did not write) is clamped into it.
 * Rejected before any launch: a null pointer, except the frame-0 pair; exactly one of prev_score and
 * prev_max null; n, S or T below 1; S > 4096; n > 65535 (the step); r outside [1, 32]; a weight that is
 * not finite or not in (0, 1].                                                                   */
int skp_track_step_workspace(int n, int S, int r);
int skp_track_step(const float* avg, const float* prev_score, const float* prev_max, int n, int S,
                   const float* w_host, int r, float* score, float* score_max, int* best, short* back,
                   void* workspace, void* stream);
int skp_track_backtrace(const short* back, const int* best_last, int T, int n, int S, int r, float* pos,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SKP_H */
