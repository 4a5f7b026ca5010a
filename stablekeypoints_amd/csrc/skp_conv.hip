// 3×3 / stride-1 / pad-1 convolution of the frozen SD VAE and UNet as Winograd F(4×4, 3×3) on
// the gfx950 fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulate).
//
// The hot path encodes every image and its warp with the VAE each optimiser step
// (reference ptp_utils.py:289-304 image2latent, called from optimize.py:173-180) and runs the
// UNet forward and its input-gradient backward; their 3×3 convolutions are ≈60% of the step.
// gfx950 has no reduced-precision f32 MFMA (no xf32), so the f32 matrix rate (157 TF/s, the
// same as the vector rate) is the ceiling for a direct convolution.  F(4×4, 3×3) computes a
// 4×4 output tile from a 6×6 input tile with 36 multiplies per (input, output) channel pair
// instead of 144: a 4× cut of the matrix-core work, paid for with transforms on the VALU.
//
// Interpolation points (0, 1, -1, 1/2, -2, ∞): all input/output transform coefficients are
// dyadic (exact in fp32) and the fp32 error is ≈3× a direct sequential fp32 sum (the classic
// (0, ±1, ±2, ∞) points give ≈6×); tests/test_gpu_conv.py bounds it against fp64.
//
//   V = Bᵀ d B   (6×6 input tile d of one channel, on the VALU, into LDS)
//   U = G g Gᵀ   (6×6 per (out, in) channel pair; precomputed once per frozen weight, fp64)
//   M_p = Σ_c U_p[c][k] · V_p[c][t]   for each of the 36 positions p: 36 GEMMs on MFMA
//   Y = Aᵀ M A   (4×4 output tile, in registers, + bias + residual in the same epilogue)
//
// Workgroup: 64 output tiles × 32 output channels, 8 waves (two per SIMD); wave w owns tiles
// 16(w&3)..+15 × channels 16(w>>2)..+15 as one 16×16 MFMA block per position, so each lane
// ends holding all 36 positions of 4 tiles × 1 channel (144 accumulator registers) and runs
// the output transform without any data exchange.  Input channels are walked four at a time;
// the stage pipeline keeps no loads in registers (LDS-DMA, buffer_load … lds):
//   waves 0-3 (wave w = channel w of a stage, lane = tile): transform the raw 6×6 patches of
//     stage s+1 (already in LDS) into V[s+1], then DMA stage s+2's raw patches into the same
//     per-wave LDS area, then their MFMAs on stage s;
//   waves 4-7: DMA stage s+1's U slice into U[s+1], then their MFMAs on stage s;
// one barrier per stage.  The two waves of a SIMD are one of each kind, so one's transform
// runs under the other's MFMAs.  The workgroup → (tile block, channel block) map keeps the
// work that shares operands on one XCD's L2: tile-major when the whole U fits an L2 slice
// (every channel block of a tile block back to back), channel-block-major otherwise.
//
// The backward of the same convolution w.r.t. its input is the same correlation of dy with
// the 180°-rotated, in/out-transposed kernel: skp_wino_weights(flip=1) builds that U.
#include <cstdlib>
#include <initializer_list>
#include <type_traits>

#include "skp_common.h"
#include "skp_gn.h"   // gn_coef, gn_elem: the GroupNorm(+SiLU) fused into the transform pass

using namespace skp;

// Timing-probe builds only (tools/build_variant.sh, e.g. EXTRA=-DSKP_WINO2_DEBUG=8); the shipped
// library is built with 0.  wino_f4_kernel: 1 drop x loads, 2 drop U loads, 4 skip transforms,
// 8 skip MFMAs.  wino2_kernel: 1 skip transforms, 2 skip MFMAs, 4 skip input DMA, 8 skip weight
// DMA, 16 skip the stage loop, 32 skip the epilogue, 64 skip its global stores.
#ifndef SKP_WINO_DEBUG
#define SKP_WINO_DEBUG 0
#endif
#ifndef SKP_WINO2_DEBUG
#define SKP_WINO2_DEBUG 0
#endif

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMT = 64;                       // output tiles per workgroup
constexpr int kNC = 32;                       // output channels per workgroup
constexpr int kCK = 4;                        // input channels per LDS stage (= MFMA k)
constexpr int kP = 36;                        // transform positions (6×6)
constexpr int kThreads = 512;                 // 8 waves, two per SIMD
// V stage: kCK · MT · kP floats (9216 at MT = 64)
constexpr int kUs = kCK * kNC * kP;           // floats per U stage  (4608)
constexpr int kUChunks = kUs * 4 / 1024;      // 1-KB DMA chunks per U stage (18)
constexpr int kRawRow = 64 * 16 + 64 * 4 + 64 * 4;   // bytes per patch row per wave: middle, left, right
constexpr int kRawWave = 6 * kRawRow;         // 9216 B: one wave's 64 raw patches
// LDS: V 2 × 36 KB + U 2 × 18 KB + raw patches 36 KB = 147.5 KB (static)

static_assert(kMT == 64 && kCK == 4, "wave w of 0..3 = stage channel w, lane = tile");
static_assert(kUs * 4 % 1024 == 0, "U stage in whole 1-KB chunks");

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// y = Bᵀ x for the points (0, 1, -1, 1/2, -2, ∞)
__device__ __forceinline__ void bt6(float a0, float a1, float a2, float a3, float a4, float a5, float* y, int s) {
  y[0 * s] = a0 - 1.5f * a1 - 2.0f * a2 + 1.5f * a3 + a4;
  y[1 * s] = -a1 + 0.5f * a2 + 2.5f * a3 + a4;
  y[2 * s] = a1 - 2.5f * a2 + 0.5f * a3 + a4;
  y[3 * s] = -2.0f * a1 - a2 + 2.0f * a3 + a4;
  y[4 * s] = 0.5f * a1 - a2 - 0.5f * a3 + a4;
  y[5 * s] = a1 - 1.5f * a2 - 2.0f * a3 + 1.5f * a4 + a5;
}

// y = Aᵀ m (4 outputs from 6 positions)
__device__ __forceinline__ void at6(float m0, float m1, float m2, float m3, float m4, float m5, float* y, int s) {
  const float p = m1 + m2, q = m1 - m2;
  y[0 * s] = m0 + p + m3 + m4;
  y[1 * s] = q + 0.5f * m3 - 2.0f * m4;
  y[2 * s] = p + 0.25f * m3 + 4.0f * m4;
  y[3 * s] = q + 0.125f * m3 - 8.0f * m4 + m5;
}

// V = Bᵀ d B, d and v row-major 6×6
__device__ __forceinline__ void input_transform(const float* d, float* v) {
  float t[36];
#pragma unroll
  for (int c = 0; c < 6; ++c) bt6(d[c], d[6 + c], d[12 + c], d[18 + c], d[24 + c], d[30 + c], t + c, 6);
#pragma unroll
  for (int r = 0; r < 6; ++r) bt6(t[6 * r], t[6 * r + 1], t[6 * r + 2], t[6 * r + 3], t[6 * r + 4], t[6 * r + 5], v + 6 * r, 1);
}

// Y = Aᵀ M A, m row-major 6×6, y row-major 4×4
__device__ __forceinline__ void output_transform(const float* m, float* y) {
  float s[24];
#pragma unroll
  for (int c = 0; c < 6; ++c) at6(m[c], m[6 + c], m[12 + c], m[18 + c], m[24 + c], m[30 + c], s + c, 6);
#pragma unroll
  for (int r = 0; r < 4; ++r) at6(s[6 * r], s[6 * r + 1], s[6 * r + 2], s[6 * r + 3], s[6 * r + 4], s[6 * r + 5], y + 4 * r, 1);
}

// DMA one wave's 64 raw 6×6 patches (lane = tile) of one channel plane into its LDS area:
// per patch row, the aligned middle four columns (16 B), the left and the right column (4 B
// each), each as one buffer_load … lds with lane-linear destinations.  Source rows are clamped
// into the plane and the left/right columns into the tensor; the zero padding is applied at
// transform time from the per-lane mask (bits 0..5 row inside, 6 left, 7 right column).
struct PatchAddr {
  unsigned row[6];   // byte offset of (row y0-1+r clamped, col x0) from the stage's channel-0 plane
  unsigned dl;       // 4 when the left column exists (x0 > 0), else 0
  unsigned mask;
};

__device__ __forceinline__ void dma_patches(__amdgpu_buffer_rsrc_t rs, const PatchAddr& pa, char* raw) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    char* dst = raw + r * kRawRow;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst, 16, pa.row[r], 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(dst + 1024), 4, pa.row[r] - pa.dl, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(dst + 1280), 4, pa.row[r] + 16, 0, 0, 0);
  }
}

// This lane's raw patch (LDS) → masked → V = Bᵀ d B → V stage row (ch, tile), 6 positions per row
__device__ __forceinline__ void transform_patch(const char* raw, unsigned mask, int lane, float* vd, bool store = true) {
  float d[36];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const char* row = raw + r * kRawRow;
    const float4 m = *reinterpret_cast<const float4*>(row + lane * 16);
    const float l = *reinterpret_cast<const float*>(row + 1024 + lane * 4);
    const float rr = *reinterpret_cast<const float*>(row + 1280 + lane * 4);
    const bool ok = (mask >> r) & 1u;
    d[6 * r + 0] = (ok && (mask & 64u)) ? l : 0.0f;
    d[6 * r + 1] = ok ? m.x : 0.0f;
    d[6 * r + 2] = ok ? m.y : 0.0f;
    d[6 * r + 3] = ok ? m.z : 0.0f;
    d[6 * r + 4] = ok ? m.w : 0.0f;
    d[6 * r + 5] = (ok && (mask & 128u)) ? rr : 0.0f;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float t[6];
    bt6(d[c], d[6 + c], d[12 + c], d[18 + c], d[24 + c], d[30 + c], t, 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) d[6 * i + c] = t[i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float v[6];
    bt6(d[6 * i], d[6 * i + 1], d[6 * i + 2], d[6 * i + 3], d[6 * i + 4], d[6 * i + 5], v, 1);
    if (store) {
      *reinterpret_cast<float2*>(vd + 6 * i) = make_float2(v[0], v[1]);
      *reinterpret_cast<float2*>(vd + 6 * i + 2) = make_float2(v[2], v[3]);
      *reinterpret_cast<float2*>(vd + 6 * i + 4) = make_float2(v[4], v[5]);
    }
  }
}

// EPI bit 0: + bias[k]; bit 1: + residual (same layout as y).
// MT = output tiles per workgroup: 64 (× 32 output channels), or 32 (× 64 output channels) for
// grids of at most 32 tiles (the UNet's 8² layers at batch 8), where a 64-tile block would run
// half of its MFMAs on empty tiles; lanes 32-63 of the patch waves then only idle.
template <int EPI, int MT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void wino_f4_kernel(
    const float* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
    const float* __restrict__ res, float* __restrict__ y, int nimg, int C, int K, int H, int W, int tw, int tpi,
    int ntiles, int ntb, int nkb, int kb_major, int csplit, int dbg) {
  // separate LDS objects per buffer, so the compiler can tell a DMA into one buffer from a
  // ds_read of another and does not wait for the DMA before every LDS read
  constexpr int NC = kMT * kNC / MT;                // output channels per workgroup
  constexpr int VS = kCK * MT * kP, US = kCK * NC * kP;
  constexpr int NWM = MT / 16;                      // 16-tile MFMA row blocks
  __shared__ __attribute__((aligned(16))) float V0[VS], V1[VS];   // [kCK][MT][kP]
  __shared__ __attribute__((aligned(16))) float U0[US], U1[US];   // [NC / 32][kCK][32][kP]
  __shared__ __attribute__((aligned(16))) char Raw[4 * kRawWave];   // [4 waves][6 rows][mid | left | right]

  // workgroup → (input-channel split, tile block, channel block); consecutive logical ids share
  // one XCD.  With csplit < C the workgroup sums input channels [sp·csplit, (sp+1)·csplit) only
  // and writes its partial to slab sp of y (the caller's workspace).
  const int G = gridDim.x;
  const int g = blockIdx.x;
  const int Lg = (G % 8 == 0) ? (g % 8) * (G / 8) + g / 8 : g;
  const int sp = Lg / (ntb * nkb);
  const int L = Lg - sp * (ntb * nkb);
  int tb, kb;
  if (kb_major) {
    kb = L / ntb;
    tb = L - kb * ntb;
  } else {
    tb = L / nkb;
    kb = L - tb * nkb;
  }
  const int c0 = sp * csplit;
  y += (size_t)sp * nimg * K * H * W;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv % NWM, wn = wv / NWM;   // this wave's 16 tiles × 16 channels
  const bool patcher = wv < 4;            // waves 0-3: patches of stage channel wv; 4-7: U slices
  const size_t plane = (size_t)H * W;
  PatchAddr pa;
  {
    const int pt = tb * MT + lane;
    const bool pvalid = lane < MT && pt < ntiles;
    int pb = 0, py0 = 0, px0 = 0;
    if (pvalid) {
      pb = pt / tpi;
      const int r = pt - pb * tpi;
      const int ty = r / tw;
      py0 = 4 * ty;
      px0 = 4 * (r - ty * tw);
    }
    const unsigned base = (unsigned)(((size_t)pb * C + (wv & 3)) * plane);
    pa.mask = (px0 > 0 ? 64u : 0u) | (px0 + 4 < W ? 128u : 0u);
    pa.dl = px0 > 0 ? 4u : 0u;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const int yy = py0 - 1 + r;
      if (pvalid && yy >= 0 && yy < H) pa.mask |= 1u << r;
      const int yc = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
      pa.row[r] = (base + (unsigned)(yc * W + px0)) * 4u;
    }
  }
  // U is stored in 32-channel slices [K / 32][C][32][kP]; a 64-channel block reads two
  const float* Ub = U + ((size_t)(kb * (NC / kNC)) * C + c0) * kNC * kP;
  const size_t uhalf = (size_t)C * kNC * kP;   // floats between consecutive 32-channel slices
  const int nst = csplit / kCK;
  const size_t xfloats = (size_t)nimg * C * plane;
  char* raw = Raw + (wv & 3) * kRawWave;
  const bool vstore = lane < MT;
  const int vrow = ((wv & 3) * MT + (vstore ? lane : 0)) * kP;   // this patcher lane's V row
  // per-stage descriptors: x from the stage's first channel plane, U from the stage's slice
  auto xrsrc = [&](int s) {
    const size_t off = ((size_t)c0 + (size_t)s * kCK) * plane;
    return __builtin_amdgcn_make_buffer_rsrc((void*)(x + off), (short)0, (dbg & 1) ? 0 : (int)((xfloats - off) * 4), 0x00020000);
  };
  auto dma_u = [&](int s, float* ubuf) {
    char* dst = reinterpret_cast<char*>(ubuf);
#pragma unroll
    for (int h = 0; h < NC / kNC; ++h) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(Ub + h * uhalf + (size_t)s * kUs), (short)0, (dbg & 2) ? 0 : kUs * 4, 0x00020000);
#pragma unroll
      for (int c = wv - 4; c < kUChunks; c += 4)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(dst + h * kUs * 4 + c * 1024), 16, lane * 16, c * 1024,
                                                 0, 0);
    }
  };

  f32x4 acc[kP];
#pragma unroll
  for (int p = 0; p < kP; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: V[0] and U[0] ready, stage 1's raw patches in flight
  if (patcher) {
    dma_patches(xrsrc(0), pa, raw);
    __builtin_amdgcn_s_waitcnt(0);   // vmcnt(0) & lgkmcnt(0): this wave's DMA landed
    transform_patch(raw, pa.mask, lane, V0 + vrow, vstore);
    if (nst > 1) dma_patches(xrsrc(1), pa, raw);
  } else {
    dma_u(0, U0);
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  // MFMA operands: A = V[k = lane>>4][tile 16·wm + (lane&15)], B = U[k][channel 16·wn + (lane&15)]
  const int aoff = ((lane >> 4) * MT + wm * 16 + (lane & 15)) * kP;
  const int boff = (wn >> 1) * kUs + ((lane >> 4) * kNC + (wn & 1) * 16 + (lane & 15)) * kP;
  // one stage: prepare stage s+1 into (vn, un), MFMAs on (vc, uc); the loop is unrolled by two
  // so every buffer is a fixed LDS object in each half
  auto phase = [&](int s, const float* vc, const float* uc, float* vn, float* un) {
    if (s + 1 < nst) {
      if (patcher) {
        if (!(dbg & 4)) transform_patch(raw, pa.mask, lane, vn + vrow, vstore);
        if (s + 2 < nst) dma_patches(xrsrc(s + 2), pa, raw);
      } else {
        dma_u(s + 1, un);
      }
    }
    const float* va = vc + aoff;
    const float* ub = uc + boff;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      if (dbg & 8) break;
      const float4 a = *reinterpret_cast<const float4*>(va + 4 * q);
      const float4 b = *reinterpret_cast<const float4*>(ub + 4 * q);
      acc[4 * q + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[4 * q + 0], 0, 0, 0);
      acc[4 * q + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[4 * q + 1], 0, 0, 0);
      acc[4 * q + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[4 * q + 2], 0, 0, 0);
      acc[4 * q + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[4 * q + 3], 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0);   // this wave's DMA for the next stage has landed
    __syncthreads();
  };
  for (int s = 0; s < nst; s += 2) {
    phase(s, V0, U0, V1, U1);
    if (s + 1 < nst) phase(s + 1, V1, U1, V0, U0);
  }

  // epilogue: lane holds rows 4·(lane>>4)+r (tiles) × column lane&15 (channel) of every position
  const int k = kb * NC + wn * 16 + (lane & 15);
  const float bv = (EPI & 1) ? bias[k] : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = tb * MT + wm * 16 + 4 * (lane >> 4) + r;
    if (t >= ntiles) continue;
    float m[36], o[16];
#pragma unroll
    for (int p = 0; p < kP; ++p) m[p] = acc[p][r];
    output_transform(m, o);
    const int b = t / tpi;
    const int rr = t - b * tpi;
    const int ty = rr / tw;
    const int tx = rr - ty * tw;
    const size_t off = ((size_t)b * K + k) * plane + (size_t)(4 * ty) * W + 4 * tx;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float4 val = make_float4(o[4 * i] + bv, o[4 * i + 1] + bv, o[4 * i + 2] + bv, o[4 * i + 3] + bv);
      if (EPI & 2) {
        const float4 rv = *reinterpret_cast<const float4*>(res + off + (size_t)i * W);
        val.x += rv.x;
        val.y += rv.y;
        val.z += rv.z;
        val.w += rv.w;
      }
      *reinterpret_cast<float4*>(y + off + (size_t)i * W) = val;
    }
  }
}

// G of F(4×4, 3×3) at the points (0, 1, −1, 1/2, −2, ∞)
__device__ constexpr double kG[6][3] = {{1.0, 0.0, 0.0},
                                        {1.0 / 3, 1.0 / 3, 1.0 / 3},
                                        {-1.0 / 3, 1.0 / 3, -1.0 / 3},
                                        {-16.0 / 15, -8.0 / 15, -4.0 / 15},
                                        {1.0 / 15, -2.0 / 15, 4.0 / 15},
                                        {0.0, 0.0, 1.0}};

// U[kb][c][k%32][ROW] = G g Gᵀ in fp64, g = w[k][c] (flip 0) or rot180(w[c][k]) (flip 1).
// ROW 36 (wino_f4_kernel): the 36 positions; ROW 40 (wino2_kernel): positions 0..17 at 0..17,
// 18..35 at 20..37, the rest zero.
template <int ROW>
__global__ void wino_weights_kernel(const float* __restrict__ w, int K, int C, int flip, float* __restrict__ U) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)K * C) return;
  const int k = (int)(i / C), c = (int)(i - (long long)k * C);
  double g[9];
  for (int u = 0; u < 3; ++u)
    for (int v = 0; v < 3; ++v)
      g[3 * u + v] = flip ? (double)w[((size_t)c * K + k) * 9 + (2 - u) * 3 + (2 - v)]
                          : (double)w[((size_t)k * C + c) * 9 + u * 3 + v];
  double t[6][3];
  for (int a = 0; a < 6; ++a)
    for (int v = 0; v < 3; ++v) t[a][v] = kG[a][0] * g[v] + kG[a][1] * g[3 + v] + kG[a][2] * g[6 + v];
  float* out = U + (((size_t)(k / kNC) * C + c) * kNC + (k % kNC)) * ROW;
  if (ROW != kP)
    for (int p = 0; p < ROW; ++p) out[p] = 0.0f;
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      const int p = 6 * a + b;
      out[(ROW == kP || p < 18) ? p : p + 2] = (float)(t[a][0] * kG[b][0] + t[a][1] * kG[b][1] + t[a][2] * kG[b][2]);
    }
}

bool all_aligned16(std::initializer_list<const void*> ps) {   // absent (null) optional tensors pass
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

// ---------------------------------------------------------------- argument checks
// The entry points check their arguments through these and report the first failing check with
// one SKP_CHECK_ARG (which prefixes the entry's name); nullptr = every check passed.
const char* weights_args_error(const float* w, const float* U, int K, int C) {
  if (!(w && U)) return "null pointer";
  if (!(K > 0 && C > 0)) return "non-positive shape";
  if (K % kNC != 0) return "output channels must be a multiple of 32";
  return nullptr;
}

// What the convolution and vtransform entries differ in:
enum : unsigned {
  kHW32 = 1,       // H and W multiples of 32 (otherwise of 4) ...
  kOr16x16 = 2,    // ... or 16×16 images with B a multiple of 4
  kStride2 = 4,    // the output (and the split-K workspace) is (H/2, W/2)
  kOffsets32 = 8,  // x is addressed through 32-bit buffer offsets: at most 2 GiB
};
struct ConvArgs {
  bool ptrs, aligned;            // every required tensor is there; every tensor given is 16-byte aligned
  const void *ws, *gn_part;      // optional: split-K workspace, GroupNorm partials of the output
  int B, C, K, H, W, nsplit, G;  // an entry without K, nsplit or G passes 32, 1, 1
};
const char* conv_args_error(unsigned form, const ConvArgs& a) {
  const bool hw32 = a.H % 32 == 0 && a.W % 32 == 0;
  if (!a.ptrs) return "null pointer";
  if (a.gn_part) {
    const bool ok = a.nsplit == 1 && (reinterpret_cast<uintptr_t>(a.gn_part) & 7) == 0;
    if (form & kOr16x16) {
      if (!(ok && hw32)) return "gn_part: one split, H and W multiples of 32, 8-byte aligned";
    } else if (!ok) {
      return "gn_part: one split, 8-byte aligned";
    }
  }
  if (!(a.B > 0 && a.C > 0 && a.K > 0 && a.H > 0 && a.W > 0)) return "non-positive shape";
  if (a.C % kCK != 0) return "input channels must be a multiple of 4";
  if (!(a.G > 0 && a.C % a.G == 0)) return "C must be divisible by G";
  if (a.K % kNC != 0) return "output channels must be a multiple of 32";
  if (form & kOr16x16) {
    if (!(hw32 || (a.H == 16 && a.W == 16 && a.B % 4 == 0)))
      return "H and W must be multiples of 32, or 16×16 with B a multiple of 4";
  } else if (form & kHW32) {
    if (!hw32) return "H and W must be multiples of 32";
  } else if (!(a.H % 4 == 0 && a.W % 4 == 0)) {
    return "H and W must be multiples of 4";
  }
  if (!(a.nsplit >= 1 && a.C % (kCK * a.nsplit) == 0)) return "nsplit must divide C into multiples of 4";
  if (!(a.nsplit == 1 || a.ws))
    return (form & kStride2) ? "split-K needs a workspace of nsplit·B·K·(H/2)·(W/2) floats"
                             : "split-K needs a workspace of nsplit·B·K·H·W floats";
  if (!a.aligned) return "tensors must be 16-byte aligned";
  if (!(form & kHW32) && (long long)a.B * (a.H / 4) * (a.W / 4) > 0x7fffffffLL - kMT) return "too many tiles";
  if ((form & kOffsets32) && !((long long)a.B * a.C * a.H * a.W * 4 < 0x7fffffffLL))
    return "input larger than 2 GiB (32-bit buffer offsets)";
  return nullptr;
}
constexpr long long kMaxGrid = 0x7fffffffLL;

}  // namespace

extern "C" int skp_wino_weights(const float* w, int K, int C, int flip, float* U, void* stream) {
  const char* err = weights_args_error(w, U, K, C);
  SKP_CHECK_ARG(!err, err);
  const long long n = (long long)K * C;
  hipLaunchKernelGGL(wino_weights_kernel<kP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), w, K,
                     C, flip, U);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

namespace {

// y = Σ_s ws[s] + bias[k] + residual over (B, K, HW), float4 lanes (HW % 4 == 0)
__global__ void splitk_reduce_kernel(const float4* __restrict__ ws, int nsplit, long long n4, int K, int hw4,
                                     const float* __restrict__ bias, const float4* __restrict__ res,
                                     float4* __restrict__ y) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n4) return;
  float4 v = ws[i];
  for (int s = 1; s < nsplit; ++s) {
    const float4 p = ws[(long long)s * n4 + i];
    v.x += p.x;
    v.y += p.y;
    v.z += p.z;
    v.w += p.w;
  }
  if (bias) {
    const float b = bias[(i / hw4) % K];
    v.x += b;
    v.y += b;
    v.z += b;
    v.w += b;
  }
  if (res) {
    const float4 r = res[i];
    v.x += r.x;
    v.y += r.y;
    v.z += r.z;
    v.w += r.w;
  }
  y[i] = v;
}

int splitk_reduce(const float* ws, int nsplit, int B, int K, int HW, const float* bias, const float* residual,
                  float* y, hipStream_t st) {
  const long long n4 = (long long)B * K * HW / 4;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(ws), nsplit, n4, K, HW / 4, bias,
                     reinterpret_cast<const float4*>(residual), reinterpret_cast<float4*>(y));
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

// flag 128 of the region-staged kernels' flag word: non-temporal output stores, for outputs of at
// least 256 MB (larger than the Infinity Cache: the next layer re-reads them from HBM either way, and
// the stream then does not evict the input regions / weights the other workgroups re-read from L2)
int wino_nt_flag(long long out_bytes, int nsplit) {
  if (nsplit > 1) return 0;   // split-K partials are re-read by the reduction
  return out_bytes >= (256LL << 20) ? 128 : 0;
}

// f(std::integral_constant<int, epi>), instantiated for the NEPI epilogues 0..NEPI−1 the entry can ask for
template <int NEPI, class F>
auto with_epi(int epi, F&& f) {
  static_assert(NEPI == 2 || NEPI == 4, "bias only, or bias and residual");
  if constexpr (NEPI == 4) {
    if (epi == 2) return f(std::integral_constant<int, 2>{});
    if (epi == 3) return f(std::integral_constant<int, 3>{});
  }
  return epi == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}

// What every convolution entry does around its launch: one split writes y with bias and residual in
// the kernel's epilogue (EPI bit 0 / 1); split-K writes its partial sums to the workspace's slabs
// with a plain epilogue and splitk_reduce adds bias and residual.  launch(epi, out, flags) starts the
// kernel; hw = pixels per output plane; nt = the kernel knows the non-temporal store flag.
template <class Launch>
int conv_launch(const char* entry, const float* bias, const float* residual, float* y, float* ws, int nsplit, int B, int K,
                int hw, int dbg, bool nt, hipStream_t st, Launch&& launch) {
  const int epi = nsplit > 1 ? 0 : (bias ? 1 : 0) | (residual ? 2 : 0);
  launch(epi, nsplit > 1 ? ws : y, dbg | (nt ? wino_nt_flag((long long)B * K * hw * 4, nsplit) : 0));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string(entry) + ": launch failed: " + hipGetErrorString(e));
    return SKP_ELAUNCH;
  }
  if (nsplit > 1) return splitk_reduce(ws, nsplit, B, K, hw, bias, residual, y, st);
  return SKP_OK;
}

}  // namespace

extern "C" int skp_conv3x3_wino(const float* x, const float* U, const float* bias, const float* residual, float* y,
                                int B, int C, int K, int H, int W, int nsplit, float* ws, void* stream) {
  const ConvArgs a{x && U && y, all_aligned16({x, U, y, residual, ws}), ws, nullptr, B, C, K, H, W, nsplit, 1};
  const char* err = conv_args_error(kOffsets32, a);
  const int tw = W / 4, tpi = (H / 4) * tw;
  const long long ntiles = (long long)B * tpi;
  // at most 32 tiles (8² at batch 8): 32-tile × 64-channel workgroups (ops.wino_conv's planner
  // mirrors this rule)
  const bool wide = ntiles <= 32 && K % 64 == 0;
  const int mt = wide ? 32 : kMT;
  const int ntb = (int)((ntiles + mt - 1) / mt), nkb = K / (wide ? 64 : kNC);
  if (!err && (long long)ntb * nkb * nsplit > kMaxGrid) err = "grid too large";
  SKP_CHECK_ARG(!err, err);
  // one channel block's U slice is C·32·36·4 B; keep all of U on an L2 slice when it fits
  const long long ubytes = (long long)K * C * kP * 4;
  const int kb_major = ubytes > (2LL << 20);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(ntb * nkb * nsplit));
  return conv_launch(__func__, bias, residual, y, ws, nsplit, B, K, H * W, SKP_WINO_DEBUG, false, st,
                     [&](int epi, float* out, int dbg) {
                       const auto kernel = with_epi<4>(
                           epi, [&](auto E) { return wide ? wino_f4_kernel<E(), 32> : wino_f4_kernel<E(), 64>; });
                       hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, x, U, bias, residual, out, B, C, K, H, W, tw,
                                          tpi, (int)ntiles, ntb, nkb, kb_major, C / nsplit, dbg);
                     });
}

// ================================================================================================
// Winograd F(4×4, 3×3), region-staged version for H and W multiples of 32 (every VAE-encoder
// layer at 512² input and the UNet's 64² / 32² layers) and for 16×16 images.
//
// The kernel above is bound by its one-deep pipeline: every stage waits for LDS-DMA it issued
// in the same stage (≈1 µs under load, about one stage of MFMA work), and with neither
// transforms nor MFMAs it still takes half its time.  This one keeps its loads a stage or two
// ahead of use:
//   - a workgroup of 4 waves owns a half-height block of 8 × 4 output tiles (32 × 16 pixels) × 32
//     output channels; its LDS (76 KB at most) leaves room for a second workgroup on the CU, so one's
//     prologue / epilogue overlaps the other's stage loop.  Per stage of 4 input channels it DMAs
//     the block's 18-row × 40-pixel input region as rows of ten 16-byte chunks (columns x0-4 …
//     x0+35; rows and chunks outside the image load as zeros — out-of-range buffer offsets — so
//     the zero padding costs no masking) and the stage's U slice into LDS rings: the raw input
//     into 3 slots, two stages ahead of use (it streams from HBM), the weights into 2 slots, one
//     stage ahead (every tile block re-reads them and they hit L2).  The 16×16 geometry (two whole
//     images per workgroup) and the V-staged form differ in the rings only, see wino2_body;
//   - the transformed input never goes through LDS: lane (tile, channel) of a wave reads its
//     own 6×6 patch (three ds_read_b128 per row) and computes the V values that are exactly its
//     MFMA A operand.  Partner waves w and w+2 share 16 tiles and split the 36 positions by
//     transform rows (0-2 / 3-5), so no transform work is repeated: each runs half of the column
//     pass and half of the row pass;
//   - a wave owns 16 tiles × 32 channels × 18 positions (2 MFMA blocks, 144 accumulators) and
//     transforms stage s+1 while its MFMAs run on stage s (the A operands are double-buffered
//     in registers);
//   - one barrier per stage; the epilogue applies the output transform to each half's rows, the
//     partner waves add their halves in LDS planes (16 channels at a time) and every thread then
//     stores whole rows.
// ================================================================================================
namespace {
namespace w2 {

constexpr int kNC = 32;                    // output channels per workgroup
constexpr int kCK = 4;                     // input channels per stage
constexpr int kNW = 4;                     // waves per workgroup: halves 0 / 1 = waves 0-1 / 2-3
// Block geometry: a workgroup's 32 output tiles are NI images' regions of RR rows × RC 16-byte chunks.
//   TXB 8: a half-height block, 8 × 4 tiles = 32 × 16 pixels of one image (H, W multiples of 32);
//          region 18 rows × 10 chunks
//   TXB 4: two whole 16×16 images (4 × 4 tiles each); region 18 rows × 6 chunks per image
// The channel stride CHF (floats) makes the patch reads' ds_read_b128 lane groups conflict-free:
// CHF/4 ≡ 0 (TXB 8), 12 (TXB 4) mod 16.
template <int TXB>
struct GeoN;
template <>
struct GeoN<8> {
  static constexpr int NI = 1, RR = 18, RC = 10, CHF = 768;
};
template <>
struct GeoN<4> {
  static constexpr int NI = 2, RR = 18, RC = 6, CHF = 880;
};
template <int TXB>
struct GeoT : GeoN<TXB> {
  using GeoN<TXB>::NI;
  using GeoN<TXB>::RR;
  using GeoN<TXB>::RC;
  using GeoN<TXB>::CHF;
  static constexpr int RF = 4 * RC;                                   // floats per region row
  static constexpr int RAWF = (4 * CHF + 255) / 256 * 256;            // raw slot, whole 1-KB chunks
  static constexpr int RAW_INSTR = RAWF / 256;
  static_assert(NI * RR * RF <= CHF, "channel region");
};
constexpr int kUP = 40;                    // floats per (input, output channel) U row
constexpr int kUF = kCK * kNC * kUP;       // 5120 floats = 20 KB per U slot
constexpr int kUInstr = kUF / 256;         // 20
constexpr unsigned kOOB = 0x80000000u;     // buffer offset past any num_records (< 2 GiB): loads 0
// V of the V-staged form: per (half-height block, stage) a slab [wave 2HH + wm][chunk j][lane] of
// the lanes' A operands a[18] — four 16-B chunks (1 KB per wave) and one 8-B chunk (512 B)
constexpr int kVWF = 4 * 256 + 128;        // 1152 floats = 4.5 KB per wave
constexpr int kVF = 4 * kVWF;              // 4608 floats = 18 KB per slab (36 per tile and channel)
// the stride-2 form (S2): 25 positions per (input, output channel), transform rows 0-2 at 0..14 and
// rows 3-4 at 16..25 of a 28-float row (16-B aligned halves; 28·lane mod 64 banks are distinct)
constexpr int kUP2 = 28;
constexpr int kUF2 = kCK * kNC * kUP2;     // 3584 floats = 14 KB per U slot
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
static_assert(kUF % 256 == 0 && kUF2 % 256 == 0, "whole 1-KB chunks");
static_assert((3 * GeoT<8>::RAWF + 2 * kUF) * 4 <= 80 * 1024 && 2 * (GeoT<4>::RAWF + kUF) * 4 <= 80 * 1024,
              "rings of two workgroups per CU");

// Aᵀ (4 outputs × 6 positions)
__device__ constexpr float kAt[4][6] = {{1.f, 1.f, 1.f, 1.f, 1.f, 0.f},
                                        {0.f, 1.f, -1.f, 0.5f, -2.f, 0.f},
                                        {0.f, 1.f, 1.f, 0.25f, 4.f, 0.f},
                                        {0.f, 1.f, -1.f, 0.125f, -8.f, 1.f}};

// s_waitcnt vmcnt(n) with expcnt / lgkmcnt left alone (gfx9 encoding)
#define W2_VMCNT(n) __builtin_amdgcn_s_waitcnt(((n) & 15) | (((n) >> 4) << 14) | (7 << 4) | (15 << 8))

typedef float f2 __attribute__((ext_vector_type(2)));

// y = Bᵀ x with shared differences: 16 operations instead of 20 (e, f, g, h reused)
template <typename T>
__device__ __forceinline__ void bt6_shared(T a0, T a1, T a2, T a3, T a4, T a5, T* y) {
  const T e = a4 - a2, f = a3 - a1, g = a2 + a3, h = a3 - a2;
  y[0] = __builtin_elementwise_fma((T)1.5f, f, (a0 + e) - a2);
  y[1] = __builtin_elementwise_fma((T)1.5f, g, e + f);
  y[2] = __builtin_elementwise_fma((T)1.5f, h, e - f);
  y[3] = __builtin_elementwise_fma((T)2.0f, f, e);
  y[4] = __builtin_elementwise_fma((T)-0.5f, f, e);
  y[5] = __builtin_elementwise_fma((T)1.5f, e, __builtin_elementwise_fma((T)-2.0f, f, a5 - a1));
}

// Transform rows 3H..3H+2 of V = Bᵀ d B for this lane's patch (region rows at `raw`, the patch's
// first row; columns: .w of chunk 0, chunk 1, .x of chunk 2) → a[18] = V[3H+ii][j], on the packed
// f32 VALU (v_pk_*): the column pass runs on column pairs
// (1,2), (3,4), (0,5) — the first two are halves of the middle 16-B chunk, the third one
// v_pk_mov per row — streaming the patch rows through shared differences (9 / 7 operations
// per pair for rows 0-2 / 3-5 instead of 10); the row pass packs transform rows 3H and 3H+1
// (pairs re-formed per column) and runs row 3H+2 unpacked, both with the shared-difference
// Bᵀ.  ≈80 VALU instructions per patch half and stage (≈109 unpacked).
template <int H, int RF>
__device__ __forceinline__ void half_transform_pk(const float* raw, float* a) {
  f2 t[3][3];   // t[ii][p]: column pair p of transform row 3H+ii
  f2 k0[3], k1[3], k2[3], k3[3];   // streamed partial terms (per column pair)
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    if (H == 1 && r == 0) continue;   // Bᵀ rows 3-5 do not read patch row 0
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(raw + r * RF);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>(raw + r * RF + 4);
    const f32x4 c2 = *reinterpret_cast<const f32x4*>(raw + r * RF + 8);
    const f2 d[3] = {__builtin_shufflevector(c1, c1, 0, 1), __builtin_shufflevector(c1, c1, 2, 3),
                     __builtin_shufflevector(c0, c2, 3, 4)};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      if (H == 0) {
        // s = −a2 + 1.5a3 + a4, q = −a1 + 1.5a2 + a3: rows 1, 2 = s ± q, row 0 = a0 − 1.5a1 + (s − a2)
        if (r == 0) k0[p] = d[p];
        if (r == 1) { k1[p] = d[p]; k0[p] = __builtin_elementwise_fma((f2)-1.5f, d[p], k0[p]); }
        if (r == 2) { k2[p] = d[p]; k3[p] = __builtin_elementwise_fma((f2)1.5f, d[p], -k1[p]); }
        if (r == 3) { k1[p] = __builtin_elementwise_fma((f2)1.5f, d[p], -k2[p]); k3[p] = k3[p] + d[p]; }
        if (r == 4) {
          const f2 sv = k1[p] + d[p];
          t[0][p] = k0[p] + (sv - k2[p]);
          t[1][p] = sv + k3[p];
          t[2][p] = sv - k3[p];
        }
      } else {
        // e = a4 − a2, f = a3 − a1: row 3 = e + 2f, row 4 = e − f/2, row 5 = 1.5e − 2f − a1 + a5
        if (r == 1) k0[p] = d[p];
        if (r == 2) k1[p] = d[p];
        if (r == 3) { k2[p] = d[p] - k0[p]; k3[p] = __builtin_elementwise_fma((f2)-2.0f, k2[p], -k0[p]); }
        if (r == 4) {
          const f2 e = d[p] - k1[p];
          t[0][p] = __builtin_elementwise_fma((f2)2.0f, k2[p], e);
          t[1][p] = __builtin_elementwise_fma((f2)-0.5f, k2[p], e);
          k3[p] = __builtin_elementwise_fma((f2)1.5f, e, k3[p]);
        }
        if (r == 5) t[2][p] = k3[p] + d[p];
      }
    }
    // keep chunks 0 and 2 whole: with one component used the compiler narrows them to
    // ds_read_b32, 4-way bank-conflicted at this layout (ds_read_b128 is conflict-free)
    asm volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c0.z), "v"(c2.y), "v"(c2.z), "v"(c2.w));
  }
  // row pass: column b of row ii is t[ii][0] = (b1, b2), t[ii][1] = (b3, b4), t[ii][2] = (b0, b5)
  const f2 u0 = __builtin_shufflevector(t[0][2], t[1][2], 0, 2), u1 = __builtin_shufflevector(t[0][0], t[1][0], 0, 2);
  const f2 u2 = __builtin_shufflevector(t[0][0], t[1][0], 1, 3), u3 = __builtin_shufflevector(t[0][1], t[1][1], 0, 2);
  const f2 u4 = __builtin_shufflevector(t[0][1], t[1][1], 1, 3), u5 = __builtin_shufflevector(t[0][2], t[1][2], 1, 3);
  f2 y01[6];
  bt6_shared<f2>(u0, u1, u2, u3, u4, u5, y01);
  float y2[6];
  bt6_shared<float>(t[2][2].x, t[2][0].x, t[2][0].y, t[2][1].x, t[2][1].y, t[2][2].y, y2);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    a[j] = y01[j].x;
    a[6 + j] = y01[j].y;
    a[12 + j] = y2[j];
  }
}

// partial output tile of rows 3H..3H+2 of M (m[18] = M[3H+ii][j]) → y[16] (row-major 4×4)
template <int H>
__device__ __forceinline__ void half_output(const float* m, float* y) {
  float s[3][4];
#pragma unroll
  for (int ii = 0; ii < 3; ++ii) at6(m[6 * ii], m[6 * ii + 1], m[6 * ii + 2], m[6 * ii + 3], m[6 * ii + 4], m[6 * ii + 5], s[ii], 1);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = 0.0f;
      bool first = true;
#pragma unroll
      for (int ii = 0; ii < 3; ++ii) {
        const float a = kAt[r][3 * H + ii];
        if (a == 0.0f) continue;
        v = first ? ((a == 1.0f) ? s[ii][c] : a * s[ii][c]) : fmaf(a, s[ii][c], v);
        first = false;
      }
      y[4 * r + c] = v;
    }
}

// The stride-2 form: F.pad(x, (0, 1, 0, 1)) then a 3×3 / stride-2 convolution as 2×2 output tiles
// of 25 products.  In one dimension two outputs read d0..d4 = rows / columns 1..5 of the 6×6
// patch: (d0 − d2)g0, d2(g0 + g2), (d2 − d4)g2 (F(2, 2) on the even inputs) and d1 g1, d3 g1:
//   Bs2ᵀ = [1 0 −1 0 0; 0 0 1 0 0; 0 0 1 0 −1; 0 1 0 0 0; 0 0 0 1 0],  As2ᵀ = [1 1 0 1 0; 0 1 −1 0 1].
// Half H = 0 holds transform rows 0-2 (the even patch rows, 15 positions), H = 1 rows 3-4 (the
// odd ones, 10 positions): a[5 ii + j] = V[3H + ii][j].  Two ds_read_b128 per patch row.
template <int H, int RF>
__device__ __forceinline__ void s2_transform(const float* raw, float* a) {
  constexpr int NR = H ? 2 : 3;
  float d[NR][5];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const float* rp = raw + (H ? 2 + 2 * i : 1 + 2 * i) * RF;
    const float4 c1 = *reinterpret_cast<const float4*>(rp + 4);
    const float4 c2 = *reinterpret_cast<const float4*>(rp + 8);
    d[i][0] = c1.x;
    d[i][1] = c1.y;
    d[i][2] = c1.z;
    d[i][3] = c1.w;
    d[i][4] = c2.x;
    // keep chunk 2 whole (see half_transform_pk)
    asm volatile("" ::"v"(c2.y), "v"(c2.z), "v"(c2.w));
  }
#pragma unroll
  for (int ii = 0; ii < NR; ++ii) {
    float t[5];
#pragma unroll
    for (int b = 0; b < 5; ++b)
      t[b] = H ? d[ii][b] : ii == 0 ? d[0][b] - d[1][b] : ii == 1 ? d[1][b] : d[1][b] - d[2][b];
    a[5 * ii] = t[0] - t[2];
    a[5 * ii + 1] = t[2];
    a[5 * ii + 2] = t[2] - t[4];
    a[5 * ii + 3] = t[1];
    a[5 * ii + 4] = t[3];
  }
}

// partial 2×2 output tile of half H's rows of M (m[5 ii + j] = M[3H + ii][j]) → y[4] (row-major)
template <int H>
__device__ __forceinline__ void s2_output(const float* m, float* y) {
  constexpr int NR = H ? 2 : 3;
  float s[NR][2];
#pragma unroll
  for (int ii = 0; ii < NR; ++ii) {
    s[ii][0] = (m[5 * ii] + m[5 * ii + 1]) + m[5 * ii + 3];
    s[ii][1] = (m[5 * ii + 1] - m[5 * ii + 2]) + m[5 * ii + 4];
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    y[c] = H ? s[0][c] : s[0][c] + s[1][c];
    y[2 + c] = H ? s[1][c] : s[1][c] - s[NR - 1][c];
  }
}

}  // namespace w2

struct W2Smem {
  float *R0, *R1, *R2, *U0, *U1, *U2;   // ring slots; a form without a slot passes nullptr
};

// s_waitcnt vmcnt(n) for a wave-uniform n (the per-wave DMA instruction counts differ)
__device__ __forceinline__ void w2_vmcnt(int n) {
  switch (n) {
    case 0: W2_VMCNT(0); break;
    case 1: W2_VMCNT(1); break;
    case 2: W2_VMCNT(2); break;
    case 3: W2_VMCNT(3); break;
    case 4: W2_VMCNT(4); break;
    case 5: W2_VMCNT(5); break;
    case 6: W2_VMCNT(6); break;
    case 7: W2_VMCNT(7); break;
    case 8: W2_VMCNT(8); break;
    case 9: W2_VMCNT(9); break;
    case 10: W2_VMCNT(10); break;
    case 11: W2_VMCNT(11); break;
    case 12: W2_VMCNT(12); break;
    case 13: W2_VMCNT(13); break;
    case 14: W2_VMCNT(14); break;
    case 15: W2_VMCNT(15); break;
    default: W2_VMCNT(0); break;
  }
}

// One wave's whole program for transform half HH (rows 3HH..3HH+2); the kernel branches once
// on the wave's half so the stage loop is straight-line code for each.
//
// Rings: TXB 8 (and its S2 form) a raw-input ring of 3 slots (R0-R2, lead 2: the input streams
// from HBM) and a weight ring of 2 (U0, U1, lead 1: every tile block re-reads the weights, which
// hit L2); TXB 4 a raw ring of 2 (R0, R1) and a weight ring of 2; VST no raw ring and a weight ring
// of 3 (below).  Every form leaves room for a second workgroup on the CU.
//
// VST (the V-staged form, skp_conv3x3_wino2_v): `x` is not the image but its transform V from
// skp_wino2_vtransform, one 18-KB slab [wave][chunk][lane] per (half-height block, stage): lane L
// of wave wv finds its own a[18] there, written by lane L of wave wv of the transform pass.  LDS
// would give V no reuse (every element goes to one lane of one wave), so the raw ring and the
// per-lane transform are replaced by buffer loads straight into a ring of three A-operand register
// buffers, two stages ahead of use; the LDS that frees lets U's ring be three slots deep as well
// (60 KB: still two workgroups per CU).  sm.R0 / sm.R1 are only the epilogue's plane buffers here,
// carved from the U ring.  MFMA order, accumulators and the epilogue are the same code.
//
// S2 (the stride-2 form, skp_conv3x3s2_f2): the same staging, rings and barriers; each tile's 5×5
// sub-patch gives a 2×2 tile of the (H/2, W/2) output from 25 products (s2_transform above), U
// rows are 28 floats (14 KB per slot) and the epilogue exchanges 8 × 16-pixel planes.
template <int EPI, int HH, int TXB, bool VST = false, bool S2 = false>
__device__ __forceinline__ void wino2_body(const W2Smem& sm, const float* __restrict__ x, const float* __restrict__ U,
                                           const float* __restrict__ bias, const float* __restrict__ res,
                                           float* __restrict__ y, int C, int K, int H, int W, int img, int x0,
                                           int y0, int kb, int c0, int csplit, int wv, int dbg,
                                           float2* __restrict__ gnp) {
  using Geo = w2::GeoT<TXB>;
  constexpr int NW = w2::kNW;
  constexpr int kChF = Geo::CHF, kRowF = Geo::RF, kRawInstr = Geo::RAW_INSTR, NI = Geo::NI, RR = Geo::RR,
                RC = Geo::RC;
  static_assert(!S2 || (TXB == 8 && !VST && (EPI & ~1) == 0), "stride-2 form: half-height blocks, bias only");
  constexpr int kUP = S2 ? w2::kUP2 : w2::kUP, kUF = S2 ? w2::kUF2 : w2::kUF, kUInstr = kUF / 256;
  constexpr int NP = S2 ? (HH ? 10 : 15) : 18;   // positions of this half
  constexpr int kInstr = kRawInstr + kUInstr;
  constexpr int kMaxRaw = (kRawInstr + NW - 1) / NW;
  constexpr int kMaxU = (kUInstr + NW - 1) / NW + 1;
  constexpr int NT = NW * WAVE;
  static_assert(!VST || TXB == 8, "V-staged form: half-height blocks");
  // raw-input ring of RS slots (lead RS − 1 stages); VST has none, RS = 2 there only picks the
  // epilogue's third plane buffer
  constexpr int RS = (VST || TXB == 4) ? 2 : 3;
  float *R0 = sm.R0, *R1 = sm.R1, *R2 = sm.R2, *U0 = sm.U0, *U1 = sm.U1, *U2 = sm.U2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wm = wv % (NW / 2);
  const size_t plane = (size_t)H * W;
  const size_t ximg = (size_t)img * C * plane;

  // this wave's DMA chunks of a stage: chunk g = wv + 4m (the raw slot's chunks, then U's);
  // raw chunk → (channel, image of the block, region row, 16-B column chunk)
  unsigned voff[kMaxRaw];
  int nraw = 0;
#pragma unroll
  for (int m = 0; m < kMaxRaw; ++m) {
    const int gi = wv + NW * m;
    voff[m] = w2::kOOB;
    if (gi < kRawInstr) {
      ++nraw;
      const int f = 64 * gi + lane;   // 16-B chunk of the slot
      const int ch = f / (kChF / 4);
      const int e = f - ch * (kChF / 4);
      const int ii = e / (RR * RC), rem = e - ii * (RR * RC);
      const int row = rem / RC, c4 = rem - row * RC;
      const int yy = y0 - 1 + row, xx = x0 - 4 + 4 * c4;
      if (ch < w2::kCK && ii < NI && yy >= 0 && yy < H && xx >= 0 && xx < W)
        voff[m] = (unsigned)((ximg + ((size_t)ii * C + ch) * plane + (size_t)yy * W + xx) * 4);
    }
  }
  const int nuw = (kInstr - 1 - wv) / NW + 1 - nraw;  // U chunks of this wave
  const int ufirst = wv + NW * nraw - kRawInstr;      // its first U chunk
  // vmcnt allowances (in-order counter).  The top of step s needs U(s) and raw(s+1) landed, the
  // prologue raw(0).
  // RS = 3: per step the wave issues U(s+1) then raw(s+3), so raw(s+2) may stay in flight at the
  //   top of step s; the prologue issues raw(0), U(0), raw(1), raw(2).
  // RS = 2: per step U(s+1) then raw(s+2), and the top of step s waits for both of the previous
  //   step's; the prologue issues raw(0), U(0), raw(1).
  const int allow_step = RS == 2 ? 0 : nraw;
  const int allow_pro = RS == 2 ? nuw + nraw : nuw + 2 * nraw;
  const size_t xend = (size_t)(img + NI) * C * plane; // the buffer ends with the block's last image
  const float* Ub = U + ((size_t)kb * C + c0) * w2::kNC * kUP;
  const int nst = csplit / w2::kCK;

  // raw(t) → raw slot t % RS, U(t) → U slot t % 2 (VST: t % 3)
  auto issue_raw = [&](int t, float* rs_lds) {
    const bool ok = t < nst;
    const size_t off = ((size_t)c0 + (size_t)(ok ? t : 0) * w2::kCK) * plane;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(x + off), (short)0, ok ? (int)((xend - off) * 4) : 0, 0x00020000);
#pragma unroll
    for (int m = 0; m < kMaxRaw; ++m)
      if (m < nraw && !(dbg & 4))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)(rs_lds + 256 * (wv + NW * m)), 16, voff[m], 0, 0, 0);
  };
  auto issue_u = [&](int t, float* us_lds) {
    const __amdgpu_buffer_rsrc_t ru =
        __builtin_amdgcn_make_buffer_rsrc((void*)(Ub + (size_t)t * kUF), (short)0, kUF * 4, 0x00020000);
#pragma unroll
    for (int m = 0; m < kMaxU; ++m)
      if (m < nuw && !(dbg & 8)) {
        const int q = ufirst + NW * m;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ru, (lds_ptr_t)(us_lds + 256 * q), 16, lane * 16, q * 1024, 0, 0);
      }
  };

  // lane → (tile, stage channel) = its A-operand row; the patch's first row in the region.
  // TXB 8: wave wm has tile rows 2wm, 2wm+1; TXB 4: wave wm has image wm of the block.
  const int kc = lane >> 4;
  const int tx = lane & (TXB - 1);
  const int ty = TXB == 8 ? 2 * wm + ((lane >> 3) & 1) : (lane >> 2) & 3;
  const int roff = kc * kChF + (TXB == 8 ? 0 : wm * RR * kRowF) + 4 * ty * kRowF + 4 * tx;
  // B operand: U[kc][16 blk + (lane & 15)][18 HH + q] (rows padded to 40, halves at 0 and 20)
  // (S2: rows of 28, halves at 0 and 16)
  const int uoff = (kc * w2::kNC + (lane & 15)) * kUP + (S2 ? 16 : 20) * HH;

  f32x4 acc[2][NP];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int q = 0; q < NP; ++q) acc[b][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  float a0[NP], a1[NP];   // A operands of the even / odd stages (no copies between stages)

  auto mfmas = [&](const float* us, const float (&acur)[NP]) {
    constexpr int N4 = (NP + 1) / 4;   // 18: 4 × 16 B + 8 B; 15: 4 × 16 B; 10: 2 × 16 B + 8 B
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float* ub = us + uoff + b * 16 * kUP;
      float u[4 * N4 + 2];
#pragma unroll
      for (int j = 0; j < N4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(ub + 4 * j);
        u[4 * j] = v.x;
        u[4 * j + 1] = v.y;
        u[4 * j + 2] = v.z;
        u[4 * j + 3] = v.w;
      }
      if constexpr (NP % 4 == 2) {
        const float2 v2 = *reinterpret_cast<const float2*>(ub + 4 * N4);
        u[4 * N4] = v2.x;
        u[4 * N4 + 1] = v2.y;
      }
#pragma unroll
      for (int q = 0; q < NP; ++q) acc[b][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(acur[q], u[q], acc[b][q], 0, 0, 0);
    }
  };
  // the lane's patch of a raw slot → its A operands
  auto transform = [&](const float* raw, float (&an)[NP]) {
    if constexpr (S2) w2::s2_transform<HH, kRowF>(raw + roff, an);
    else w2::half_transform_pk<HH, kRowF>(raw + roff, an);
  };

  if constexpr (VST) {
    // slab of (tile block, stage t): V + ((tb · C/4) + c0/4 + t) · kVF; wave wv's 4.5 KB of it is
    // [chunk j][lane]: four 16-B chunks and one 8-B chunk per lane = that lane's a[18]
    using w2::kVF;
    using w2::kVWF;
    const int bw = W >> 5;
    const size_t tb = (size_t)img * ((H >> 4) * bw) + (size_t)(y0 >> 4) * bw + (x0 >> 5);
    const float* Vb = x + (tb * (size_t)(C / w2::kCK) + (size_t)(c0 / w2::kCK)) * kVF + wv * kVWF;
    // V is a read-only __restrict__ argument, whose loads the compiler may move anywhere, across
    // barriers and the memory fences below too; the explicit vmcnt allowance counts on every
    // stage's loads staying in the step that issues them, so the pointer is made opaque
    asm volatile("" : "+s"(Vb));
    struct AReg {
      u32x4 c[4];
      w2::u32x2 d;
    };
    // V(t) → registers, U(t) → LDS slot t % 3: five buffer loads and five DMAs per wave, issued
    // whether or not stage t exists (past the last stage both resources are zero-length: nothing
    // is fetched and the in-order vmcnt counts stay the same every stage)
    auto issue_vu = [&](int t, AReg& an, float* us_lds) {
      const bool ok = t < nst;
      const size_t tt = ok ? (size_t)t : 0;
      const __amdgpu_buffer_rsrc_t rv =
          __builtin_amdgcn_make_buffer_rsrc((void*)(Vb + tt * kVF), (short)0, ok ? kVWF * 4 : 0, 0x00020000);
      const __amdgpu_buffer_rsrc_t ru =
          __builtin_amdgcn_make_buffer_rsrc((void*)(Ub + tt * kUF), (short)0, ok ? kUF * 4 : 0, 0x00020000);
#pragma unroll
      for (int j = 0; j < 4; ++j) an.c[j] = __builtin_amdgcn_raw_buffer_load_b128(rv, lane * 16, j * 1024, 0);
      an.d = __builtin_amdgcn_raw_buffer_load_b64(rv, lane * 8, 4096, 0);
#pragma unroll
      for (int m = 0; m < w2::kUInstr / NW; ++m) {
        const int q = wv + NW * m;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ru, (lds_ptr_t)(us_lds + 256 * q), 16, lane * 16, q * 1024, 0, 0);
      }
    };
    static_assert(w2::kUInstr % NW == 0, "whole chunks per wave");
    constexpr int kPerStage = 5 + w2::kUInstr / NW;   // vector-memory instructions per wave and stage
    // stage s: wait for this wave's U(s) DMAs (everything but the kPerStage instructions of V(s+1),
    // U(s+1) — V(s) precedes U(s) in the in-order counter); barrier (every wave's U(s) has landed and
    // everyone is past stage s−1, whose U slot is free); issue V(s+2), U(s+2); MFMAs on A(s), slot s % 3
    // The loads are ordinary (compiler-counted) buffer loads.  Each step uses A(s) unconditionally
    // (the empty asm) in a block every path runs through, so the loads can be neither sunk into a
    // conditional block nor waited for with anything but a counted vmcnt, which the step's own
    // explicit one already covers; only the MFMAs of a step past the last stage are skipped.
    auto vstep = [&](int s, const AReg& ac, const float* Us, AReg& ai, float* Ui) {
      // A bare s_barrier between compiler-only memory fences, not __syncthreads(): its release
      // fence waits vmcnt(0) for the DMAs in flight and would take the lead back to one stage.
      // This wave's LDS reads of stage s−1 have returned (lgkmcnt(0)) before it signals.
      W2_VMCNT(kPerStage);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0) alone
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      asm volatile("" ::"v"(ac.c[0]), "v"(ac.c[1]), "v"(ac.c[2]), "v"(ac.c[3]), "v"(ac.d));
      issue_vu(s + 2, ai, Ui);
      __builtin_amdgcn_sched_barrier(0);   // the loads stay ahead of the stage's MFMAs
      if (s < nst) {
        float a[18];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const unsigned v = ac.c[j][i];   // by value: a bit_cast of the element lvalue reads element 0
            a[4 * j + i] = __uint_as_float(v);
          }
        const unsigned d0 = ac.d[0], d1 = ac.d[1];
        a[16] = __uint_as_float(d0);
        a[17] = __uint_as_float(d1);
        mfmas(Us, a);
      }
    };
    // A-operand ring of three register buffers and U ring of three LDS slots: lead 2, the loop
    // unrolled by the ring period.  With fewer stages than the lead, and in the steps that round
    // the stage count up to the period, the extra issues are the empty ones above.
    AReg A0, A1, A2;
    issue_vu(0, A0, U0);
    asm volatile("" ::: "memory");   // stage 0's instructions stay ahead of stage 1's in the counter
    __builtin_amdgcn_sched_barrier(0);
    issue_vu(1, A1, U1);
    for (int s0 = 0; s0 < nst; s0 += 3) {
      vstep(s0, A0, U0, A2, U2);
      vstep(s0 + 1, A1, U1, A0, U0);
      vstep(s0 + 2, A2, U2, A1, U1);
    }
  } else {
    // prologue: the DMAs of "steps" −RS..−1 (raw(0..RS−1), U(0)) in step order; wait for
    // raw(0) and transform it
    issue_raw(0, R0);
    issue_u(0, U0);
    issue_raw(1, R1);
    if (RS == 3) issue_raw(2, R2);
    w2_vmcnt(nst > 1 ? allow_pro : 0);
    __syncthreads();
    transform(R0, a0);

    // stage s: wait for U(s) and raw(s+1); barrier; issue U(s+1) and raw(s+RS) into the slots
    // freed by stage s-1; transform raw(s+1) (slot (s+1)%RS) and run the MFMAs on U(s) (slot
    // s%2).  The partner waves w, w+2 (the two halves) do these in opposite orders.
    auto step = [&](int s, float* Rn, float* Us, float* Ri, float* Ui, const float (&acur)[NP], float (&anext)[NP]) {
      w2_vmcnt(s + 1 < nst ? allow_step : 0);
      __syncthreads();
      if (s + 1 < nst) issue_u(s + 1, Ui);
      issue_raw(s + RS, Ri);   // past the last stage: empty (zero-length) loads keep the counts
      const bool tr = s + 1 < nst && !(dbg & 1);
      if (HH == 0) {
        if (tr) transform(Rn, anext);
        if (!(dbg & 2)) mfmas(Us, acur);
      } else {
        if (!(dbg & 2)) mfmas(Us, acur);
        if (tr) transform(Rn, anext);
      }
    };
    // unrolled by lcm(RS, 2): raw slot s%RS, U slot and A-operand buffer s%2
    constexpr int PER = RS == 2 ? 2 : 6;
    // (the table keeps a fourth, unused entry: with three the compiler allocates the TXB 8 stage
    // loop's registers differently, and this code is held to its measured instruction stream)
    float* const Rsl[4] = {R0, R1, R2, nullptr};
    float* const Usl[2] = {U0, U1};
    for (int s0 = 0; s0 < ((dbg & 16) ? 0 : nst); s0 += PER) {
      step(s0, Rsl[1], Usl[0], Rsl[0], Usl[1], a0, a1);
  #pragma unroll
      for (int j = 1; j < PER; ++j) {
        if (s0 + j < nst) {
          if ((j & 1) == 0) step(s0 + j, Rsl[(j + 1) % RS], Usl[j % 2], Rsl[j % RS], Usl[(j + 1) % 2], a0, a1);
          else step(s0 + j, Rsl[(j + 1) % RS], Usl[j % 2], Rsl[j % RS], Usl[(j + 1) % 2], a1, a0);
        }
      }
    }

  }

  // epilogue: lane holds tiles 4(lane>>4)+r of the wave's 16 (ty = 2wm + (lane>>5),
  // tx = 4((lane>>4)&1) + r) × channel 16 blk + (lane&15), rows 3HH..3HH+2 of M.  Per block of 16
  // channels: the other half's waves stage their partial tiles in LDS ([ch][16 rows][32 px]),
  // this half's waves add theirs in place, then every thread stores whole 128-B rows.
  W2_VMCNT(0);
  __syncthreads();
  if (dbg & 32) return;
  if constexpr (S2) {
    // lane holds tiles (ty = 2wm + (lane>>5), tx = 4((lane>>4)&1) + r), r = 0..3, × channel 16 blk +
    // (lane&15): its half's share of Y = As2ᵀ M As2, two output rows of 8 contiguous pixels.  Per
    // block of 16 channels the other half's waves stage theirs in R0 as [ch][8 rows][16 px] planes
    // (stride 132: the 16 channels of a store hit distinct banks), this half's add in place, then
    // every thread stores two float4 of the (H/2, W/2) output.
    constexpr int PLS2 = 8 * 16 + 4;
    static_assert(16 * PLS2 <= Geo::RAWF, "stride-2 exchange planes fit one raw slot");
    const int Ho = H / 2, Wo = W / 2;
    float* pl = R0 + (lane & 15) * PLS2 + 2 * (2 * wm + (lane >> 5)) * 16 + 8 * ((lane >> 4) & 1);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      float o[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) m[q] = acc[blk][q][r];
        w2::s2_output<HH>(m, o[r]);
      }
      if (HH != blk) {
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<float4*>(pl + f * 16 + 4 * h) =
                make_float4(o[2 * h][2 * f], o[2 * h][2 * f + 1], o[2 * h + 1][2 * f], o[2 * h + 1][2 * f + 1]);
      }
      __syncthreads();
      if (HH == blk) {
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float4* d = reinterpret_cast<float4*>(pl + f * 16 + 4 * h);
            const float4 p = *d;
            *d = make_float4(o[2 * h][2 * f] + p.x, o[2 * h][2 * f + 1] + p.y, o[2 * h + 1][2 * f] + p.z,
                             o[2 * h + 1][2 * f + 1] + p.w);
          }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 16 * 32 / NT; ++i) {
        const int idx = i * NT + tid;
        const int c = idx >> 5, row = (idx >> 2) & 7, c4 = idx & 3;
        const float4 p = *reinterpret_cast<const float4*>(R0 + c * PLS2 + row * 16 + 4 * c4);
        const int k = kb * w2::kNC + 16 * blk + c;
        const float bv = (EPI & 1) ? bias[k] : 0.0f;
        const size_t o4 = (((size_t)img * K + k) * Ho + y0 / 2 + row) * Wo + x0 / 2 + 4 * c4;
        const float4 v = make_float4(p.x + bv, p.y + bv, p.z + bv, p.w + bv);
        if (dbg & 128) __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(y + o4));
        else if (!(dbg & 64)) *reinterpret_cast<float4*>(y + o4) = v;
      }
      if (blk == 0) __syncthreads();
    }
  } else {
    // channel c of a block: a 512-float plane in R0/R1/R2/U0 (four channels each, skewed by 16
    // floats per buffer so the 8-lane store groups hit distinct banks)
    constexpr int PH = 16;   // TXB 8: plane rows = the block's pixel rows
    // plane stride: TXB 8 the block's PH × 32 pixels, TXB 4 its NI 16×16 images (+4 skew); with a
    // 2-slot raw ring the third plane buffer is U1 (no R2)
    constexpr int PLS = (TXB == 8 ? PH * 32 : NI * 256) + 4;
    float* const P2 = RS == 2 ? U1 : R2;
    auto plane_of = [&](int c) -> float* {
      float* b = (c >> 2) == 0 ? R0 : (c >> 2) == 1 ? R1 : (c >> 2) == 2 ? P2 : U0;
      return b + (c & 3) * PLS + (c >> 2) * 16;
    };
    // this lane's output tile row within the plane: TXB 8: tiles (2wm + lane>>5, 4((lane>>4)&1)
    // + r) of the 32×16 block; TXB 4: image wm (256 floats), tile row lane>>4, tiles r = 0..3
    float* pl = plane_of(lane & 15);
    const int pbase = TXB == 8 ? (4 * (2 * wm + (lane >> 5))) * 32 + 4 * (4 * ((lane >> 4) & 1))
                               : wm * 256 + (4 * (lane >> 4)) * 16;
    constexpr int PW = TXB == 8 ? 32 : 16;   // plane row width
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      if (HH != blk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float m[18], o[16];
#pragma unroll
          for (int q = 0; q < 18; ++q) m[q] = acc[blk][q][r];
          w2::half_output<HH>(m, o);
#pragma unroll
          for (int f = 0; f < 4; ++f)
            *reinterpret_cast<float4*>(pl + pbase + f * PW + 4 * r) =
                make_float4(o[4 * f], o[4 * f + 1], o[4 * f + 2], o[4 * f + 3]);
        }
      }
      __syncthreads();
      if (HH == blk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float m[18], o[16];
#pragma unroll
          for (int q = 0; q < 18; ++q) m[q] = acc[blk][q][r];
          w2::half_output<HH>(m, o);
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            float4* d = reinterpret_cast<float4*>(pl + pbase + f * PW + 4 * r);
            const float4 p = *d;
            *d = make_float4(o[4 * f] + p.x, o[4 * f + 1] + p.y, o[4 * f + 2] + p.z, o[4 * f + 3] + p.w);
          }
        }
      }
      __syncthreads();
      // 16 channels × 512 floats in 16-B chunks; a wave instruction = 1 KB of one channel:
      // TXB 8: 8 whole rows of the 32×16 block; TXB 4: one whole 16×16 image plane
      constexpr int PCF = TXB == 8 ? PH * 8 : NI * 64;   // float4 per channel plane
      constexpr int NIT = 16 * PCF / NT;                  // wave instructions per wave
      // TXB 8: wave w takes wave instructions 8w … 8w + 7 (1 KB = 8 rows of one channel each), so
      // each consecutive pair is one 16-row × 32-pixel segment of one channel: the GroupNorm
      // statistics below accumulate a pair in registers and reduce the wave's 4 segments together
      static_assert(TXB != 8 || NIT == 8, "TXB 8: eight wave instructions per wave");
      // (Σd, Σd²) of d = v − p around a pivot p per segment (a value of the segment: its first wave
      // instruction's lane-0 x), so a channel whose mean is far from 0 relative to its spread loses
      // nothing to cancellation; the segment leaves as (mean, M2) for Chan's combine (r05)
      float g1[4] = {0.f, 0.f, 0.f, 0.f}, g2[4] = {0.f, 0.f, 0.f, 0.f}, piv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        const int idx = TXB == 8 ? (((tid >> 6) * NIT + i) << 6) + (tid & 63) : i * NT + tid;
        const int c = idx / PCF, q = idx % PCF;
        const float4 v0 = *reinterpret_cast<const float4*>(plane_of(c) + 4 * q);
        const int k = kb * w2::kNC + 16 * blk + c;
        const float bv = (EPI & 1) ? bias[k] : 0.0f;
        size_t o;
        if (TXB == 8) {
          const int row = q >> 3, c4 = q & 7;
          o = (((size_t)img * K + k) * H + y0 + row) * W + x0 + 4 * c4;
        } else {
          o = ((size_t)(img + (q >> 6)) * K + k) * 256 + 4 * (q & 63);
        }
        float4 v = make_float4(v0.x + bv, v0.y + bv, v0.z + bv, v0.w + bv);
        if (EPI & 2) {
          const float4 rv = *reinterpret_cast<const float4*>(res + o);
          v.x += rv.x;
          v.y += rv.y;
          v.z += rv.z;
          v.w += rv.w;
        }
        if (dbg & 128) __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(y + o));
        else if (!(dbg & 64)) *reinterpret_cast<float4*>(y + o) = v;
        if (TXB == 8 && gnp) {   // the next GroupNorm's statistics: this lane's share of (Σd, Σd²)
          if ((i & 1) == 0) piv[i >> 1] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v.x)));
          const float p = piv[i >> 1];
          const float dx = v.x - p, dy = v.y - p, dz = v.z - p, dw = v.w - p;
          g1[i >> 1] += (dx + dy) + (dz + dw);
          g2[i >> 1] += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
      }
      if (TXB == 8 && gnp) {
        // Reduce the wave's 8 values (Σ, Σ² of its 4 segments) over its 64 lanes together:
        // a permlane32 swap + add leaves 4 registers whose lane halves hold different values, a
        // permlane16 swap + add 2 whose 16-lane rows do, a row-mirror exchange 1 whose 8-lane
        // halves do; three DPP steps then finish each 8-lane group: group (row r, half h) = value
        // 2r + h, i.e. segment r's Σ (h 0) or Σ² (h 1).  (≈20 VALU instead of 8 full reductions.)
        float a[4] = {g1[0], g2[0], g1[1], g2[1]}, b[4] = {g1[2], g2[2], g1[3], g2[3]};
        float u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a[j]), "+v"(b[j]));
          u[j] = a[j] + b[j];   // lanes 0-31: value j's partial, 32-63: value j + 4's
        }
        float w[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float x0 = u[j], x1 = u[j + 2];
          asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x0), "+v"(x1));
          w[j] = x0 + x1;       // row r: value j + 2r
        }
        const int lane = tid & 63;
        const bool hi = (lane & 8) != 0;
        const float keep = hi ? w[1] : w[0], send = hi ? w[0] : w[1];
        float x = keep + dpp_read<0x140>(send);   // row_mirror: lane i <-> 15 - i
        x += dpp_read<0x141>(x);                  // row_half_mirror
        x += dpp_read<0x4E>(x);                   // quad_perm [2,3,0,1]
        x += dpp_read<0xB1>(x);                   // quad_perm [1,0,3,2]
        const float x2 = __shfl_xor(x, 8, 64);    // lane 16r: Σd of segment r, x2 its Σd²
        if ((lane & 15) == 0) {
          const int r = lane >> 4;
          const int J = (tid >> 6) * NIT + 2 * r;   // the segment's first wave instruction
          const int c = (J << 6) / PCF, piece = ((J << 6) % PCF) >> 6;
          const int k = kb * w2::kNC + 16 * blk + c;
          const int seg = ((y0 + 8 * piece) >> 4) * (W >> 5) + (x0 >> 5);
          const float p = r == 0 ? piv[0] : r == 1 ? piv[1] : r == 2 ? piv[2] : piv[3];
          constexpr float inv_n = 1.0f / 512.0f;   // 16 rows × 32 pixels
          gnp[((size_t)img * K + k) * (size_t)((H >> 4) * (W >> 5)) + seg] =
              make_float2(p + x * inv_n, fmaxf(x2 - x * (x * inv_n), 0.0f));
        }
      }
      if (blk == 0) __syncthreads();
    }
  }
}

template <int EPI, int TXB, bool S2 = false>
__global__ __launch_bounds__(w2::kNW * WAVE) __attribute__((amdgpu_waves_per_eu(2, 2))) void wino2_kernel(
    const float* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
    const float* __restrict__ res, float* __restrict__ y, int nimg, int C, int K, int H, int W, int bw, int bpi,
    int nblk, int nkb, int kb_major, int csplit, int dbg, float2* __restrict__ gnp) {
  // separate LDS objects per ring slot: the compiler tells a DMA into one slot from a ds_read of
  // another and does not wait for outstanding DMAs before every LDS read
  // (TXB 4 has no third raw slot: its R2 is an unused stub that the compiler drops)
  constexpr int RAWF = w2::GeoT<TXB>::RAWF;
  __shared__ __attribute__((aligned(16))) float R0[RAWF], R1[RAWF], R2[TXB == 4 ? 4 : RAWF];
  constexpr int UF = S2 ? w2::kUF2 : w2::kUF;
  __shared__ __attribute__((aligned(16))) float U0[UF], U1[UF];
  // workgroup → (input-channel split, half-height block, channel block); consecutive logical ids
  // share one XCD.  A split sums its csplit input channels into slab sp of y (the workspace).
  const int G = gridDim.x;
  const int g = blockIdx.x;
  const int Lg = (G % 8 == 0) ? (g % 8) * (G / 8) + g / 8 : g;
  const int sp = Lg / (nblk * nkb);
  const int L = Lg - sp * (nblk * nkb);
  y += (size_t)sp * nimg * K * (S2 ? (H / 2) * (W / 2) : H * W);   // S2: stride-2 output
  int tb, kb;
  if (kb_major) {
    kb = L / nblk;
    tb = L - kb * nblk;
  } else {
    tb = L / nkb;
    kb = L - tb * nkb;
  }
  // TXB 8: block = 32×16 pixels of one image; TXB 4: images 2tb, 2tb+1 whole
  int img, x0 = 0, y0 = 0;
  if (TXB == 8) {
    img = tb / bpi;
    const int br = tb - img * bpi;
    const int by = br / bw;
    x0 = 32 * (br - by * bw);
    y0 = 16 * by;
  } else {
    img = 2 * tb;
  }
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const W2Smem sm{R0, R1, R2, U0, U1, nullptr};
  const int c0 = sp * csplit;
  if (wv < w2::kNW / 2)
    wino2_body<EPI, 0, TXB, false, S2>(sm, x, U, bias, res, y, C, K, H, W, img, x0, y0, kb, c0, csplit, wv, dbg, gnp);
  else wino2_body<EPI, 1, TXB, false, S2>(sm, x, U, bias, res, y, C, K, H, W, img, x0, y0, kb, c0, csplit, wv, dbg, gnp);
}

// The stride-2 form's U = Gs2 g Gs2ᵀ, Gs2 = [1 0 0; 1 0 1; 0 0 1; 0 1 0; 0 1 0], in fp64 → fp32:
// U[kb][c][k%32][28], positions 0..14 at 0..14, 15..24 at 16..25, the rest zero
__global__ void wino2s2_weights_kernel(const float* __restrict__ w, int K, int C, float* __restrict__ U) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)K * C) return;
  const int k = (int)(i / C), c = (int)(i - (long long)k * C);
  double g[9];
  for (int u = 0; u < 9; ++u) g[u] = (double)w[((size_t)k * C + c) * 9 + u];
  const double Gm[5][3] = {{1.0, 0.0, 0.0}, {1.0, 0.0, 1.0}, {0.0, 0.0, 1.0}, {0.0, 1.0, 0.0}, {0.0, 1.0, 0.0}};
  double t[5][3];
  for (int a = 0; a < 5; ++a)
    for (int v = 0; v < 3; ++v) t[a][v] = Gm[a][0] * g[v] + Gm[a][1] * g[3 + v] + Gm[a][2] * g[6 + v];
  float* out = U + (((size_t)(k / w2::kNC) * C + c) * w2::kNC + (k % w2::kNC)) * w2::kUP2;
  for (int p = 0; p < w2::kUP2; ++p) out[p] = 0.0f;
  for (int a = 0; a < 5; ++a)
    for (int b = 0; b < 5; ++b) {
      const int p = 5 * a + b;
      out[p < 15 ? p : p + 1] = (float)(t[a][0] * Gm[b][0] + t[a][1] * Gm[b][1] + t[a][2] * Gm[b][2]);
    }
}

// The V-staged form of wino2_kernel<EPI, 8>: half-height blocks, 4 waves, V in registers and a
// three-slot U ring of 20 KB each (60 KB: two workgroups per CU); grid order as wino2_kernel.
template <int EPI>
__global__ __launch_bounds__(w2::kNW * WAVE) __attribute__((amdgpu_waves_per_eu(2, 2))) void wino2v_kernel(
    const float* __restrict__ V, const float* __restrict__ U, const float* __restrict__ bias,
    const float* __restrict__ res, float* __restrict__ y, int nimg, int C, int K, int H, int W, int bw, int bpi,
    int nblk, int nkb, int kb_major, int csplit, int dbg, float2* __restrict__ gnp) {
  __shared__ __attribute__((aligned(16))) float U0[w2::kUF], U1[w2::kUF], U2[w2::kUF];
  static_assert(3 * w2::kUF * 4 <= 80 * 1024, "two workgroups per CU");
  // the epilogue's four plane buffers (4 planes of 16 × 32 + 4 floats, skewed by up to 48): the
  // halves of U0 and U1
  static_assert(4 * (16 * 32 + 4) + 48 <= w2::kUF / 2, "a plane buffer per half U slot");
  const int G = gridDim.x;
  const int g = blockIdx.x;
  const int Lg = (G % 8 == 0) ? (g % 8) * (G / 8) + g / 8 : g;
  const int sp = Lg / (nblk * nkb);
  const int L = Lg - sp * (nblk * nkb);
  y += (size_t)sp * nimg * K * H * W;
  int tb, kb;
  if (kb_major) {
    kb = L / nblk;
    tb = L - kb * nblk;
  } else {
    tb = L / nkb;
    kb = L - tb * nkb;
  }
  const int img = tb / bpi;
  const int br = tb - img * bpi;
  const int by = br / bw;
  const int x0 = 32 * (br - by * bw), y0 = 16 * by;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const W2Smem sm{U0 + w2::kUF / 2, U1 + w2::kUF / 2, nullptr, U0, U1, U2};
  const int c0 = sp * csplit;
  if (wv < w2::kNW / 2)
    wino2_body<EPI, 0, 8, true>(sm, V, U, bias, res, y, C, K, H, W, img, x0, y0, kb, c0, csplit, wv, dbg, gnp);
  else wino2_body<EPI, 1, 8, true>(sm, V, U, bias, res, y, C, K, H, W, img, x0, y0, kb, c0, csplit, wv, dbg, gnp);
}

// V = Bᵀ d B of every (image, channel, 4×4 tile) once, d = x or act(GroupNorm(x + shift)) with the
// zero padding applied to d.  One workgroup per (half-height block of 8 × 4 tiles, 4-channel
// stage): the 18 × 40-float region rows of the 4 channels go through LDS in wino2_kernel's raw-slot
// layout (so the patch reads and the transform are that kernel's, bit for bit), each wave
// transforms one half (rows 3HH..3HH+2) of 16 tiles × 4 channels, and each lane stores its a[18]
// straight from registers into the 18-KB slab [wave][chunk][lane] (coalesced wave stores), where
// the same lane of the same wave of wino2v_kernel loads it.
// GN: 0 plain, 1 GroupNorm, 2 GroupNorm + SiLU.
template <int GN>
__global__ __launch_bounds__(4 * WAVE) void wino2_vtransform_kernel(
    const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ shift, int G, float* __restrict__ V, int C, int H, int W,
    int bw, int bpi) {
  using Geo = w2::GeoT<8>;
  constexpr int RR = Geo::RR, RC = Geo::RC, kChF = Geo::CHF, kRowF = Geo::RF;
  __shared__ __attribute__((aligned(16))) float R[Geo::RAWF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nst = C / w2::kCK;
  const int tb = blockIdx.x / nst, st = blockIdx.x - tb * nst;
  const int img = tb / bpi;
  const int br = tb - img * bpi;
  const int by = br / bw;
  const int x0 = 32 * (br - by * bw), y0 = 16 * by;
  const int cpg = C / (G > 0 ? G : 1);
  for (int f = tid; f < w2::kCK * RR * RC; f += 4 * WAVE) {
    const int ch = f / (RR * RC), e = f - ch * (RR * RC);
    const int row = e / RC, c4 = e - row * RC;
    const int yy = y0 - 1 + row, xx = x0 - 4 + 4 * c4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const int c = w2::kCK * st + ch;
      v = *reinterpret_cast<const float4*>(x + (((size_t)img * C + c) * H + yy) * W + xx);
      if (GN) {
        const int grp = img * G + c / cpg;
        const GNCoef k = gn_coef(gamma[c], beta[c], stats[2 * grp], stats[2 * grp + 1]);
        const float t = shift ? shift[(size_t)img * C + c] : 0.0f;
        v.x = gn_elem<GN == 2>(v.x, t, k); v.y = gn_elem<GN == 2>(v.y, t, k);
        v.z = gn_elem<GN == 2>(v.z, t, k); v.w = gn_elem<GN == 2>(v.w, t, k);
      }
    }
    *reinterpret_cast<float4*>(R + ch * kChF + row * kRowF + 4 * c4) = v;
  }
  __syncthreads();
  // wino2_body's lane → (stage channel, tile) map: wave (half HH, wm) has tile rows 2wm, 2wm + 1
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int HH = wv >> 1, wm = wv & 1;
  const int kc = lane >> 4, tx = lane & 7, ty = 2 * wm + ((lane >> 3) & 1);
  const int roff = kc * kChF + 4 * ty * kRowF + 4 * tx;
  float a[18];
  if (HH == 0) w2::half_transform_pk<0, kRowF>(R + roff, a);
  else w2::half_transform_pk<1, kRowF>(R + roff, a);
  // the lane's a[18] as wave stores of 1 KB (four) and 512 B (one) into the wave's [chunk][lane] part
  float* o = V + (size_t)blockIdx.x * w2::kVF + wv * w2::kVWF;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<float4*>(o + 256 * j + 4 * lane) = make_float4(a[4 * j], a[4 * j + 1], a[4 * j + 2], a[4 * j + 3]);
  *reinterpret_cast<float2*>(o + 1024 + 2 * lane) = make_float2(a[16], a[17]);
}

}  // namespace

extern "C" int skp_wino2_weights(const float* w, int K, int C, int flip, float* U, void* stream) {
  const char* err = weights_args_error(w, U, K, C);
  SKP_CHECK_ARG(!err, err);
  const long long n = (long long)K * C;
  hipLaunchKernelGGL(wino_weights_kernel<w2::kUP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), w,
                     K, C, flip, U);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_wino2s2_weights(const float* w, int K, int C, float* U, void* stream) {
  const char* err = weights_args_error(w, U, K, C);
  SKP_CHECK_ARG(!err, err);
  const long long n = (long long)K * C;
  hipLaunchKernelGGL(wino2s2_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), w, K,
                     C, U);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

namespace {
// The launch of the three region-staged forms, which take the same kernel arguments: half-height
// blocks of 32 × 16 pixels (or nblk pairs of 16×16 images) × K/32 channel blocks × nsplit.
// kernel_of(E) → the form's kernel with epilogue E; hw = pixels per output plane.
// Tile-major grid order (kb_major 0: the K/32 channel blocks of one pixel block are consecutive
// logical workgroups of one XCD, sharing its input region — or its V slab, fetched from HBM once —
// in L2) measured 1-2% ahead of channel-block-major at every VAE / UNet shape, U size regardless.
using W2Kernel = void (*)(const float*, const float*, const float*, const float*, float*, int, int, int, int, int, int,
                          int, int, int, int, int, int, float2*);
template <int NEPI, class KernelOf>
int wino2_launch(const char* entry, KernelOf&& kernel_of, const float* x, const float* U, const float* bias,
                 const float* residual, float* y, int B, int C, int K, int H, int W, long long nblk, int hw, int nsplit,
                 float* ws, float* gn_part, void* stream) {
  const int bw = W / 32, bpi = (H / 16) * bw, nkb = K / w2::kNC;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(nblk * nkb * nsplit));
  return conv_launch(entry, bias, residual, y, ws, nsplit, B, K, hw, SKP_WINO2_DEBUG, true, st,
                     [&](int epi, float* out, int flags) {
                       const W2Kernel kernel = with_epi<NEPI>(epi, kernel_of);
                       hipLaunchKernelGGL(kernel, grid, dim3(w2::kNW * WAVE), 0, st, x, U, bias, residual, out, B, C, K, H,
                                          W, bw, bpi, (int)nblk, nkb, 0, C / nsplit, flags,
                                          reinterpret_cast<float2*>(gn_part));
                     });
}
}  // namespace

// The VAE's Downsample2D (diffusers: F.pad(x, (0, 1, 0, 1)) then a 3×3 stride-2 convolution; reference
// ptp_utils.py:289-304 encodes through it): y[oy, ox] taps rows 2oy..2oy+2 and columns 2ox..2ox+2 with a
// zero row / column past the bottom-right edge.  The S2 form of wino2_body computes it as 2×2 output tiles of
// 25 products (U from skp_wino2s2_weights) on the stride-1 kernel's staged regions, whose out-of-range row /
// column is that zero pad, with the bias in its epilogue: no padded copy, no NCHW↔NHWC transposes, no bias pass.
extern "C" int skp_conv3x3s2_f2(const float* x, const float* U, const float* bias, float* y, int B, int C, int K,
                                int H, int W, int nsplit, float* ws, void* stream) {
  const ConvArgs a{x && U && y, all_aligned16({x, U, y, ws}), ws, nullptr, B, C, K, H, W, nsplit, 1};
  const char* err = conv_args_error(kHW32 | kStride2 | kOffsets32, a);
  const long long nblk = (long long)B * (H / 16) * (W / 32);
  if (!err && nblk * (K / w2::kNC) * nsplit > kMaxGrid) err = "grid too large";
  SKP_CHECK_ARG(!err, err);
  return wino2_launch<2>(
      __func__, [](auto E) -> W2Kernel { return wino2_kernel<E(), 8, true>; }, x, U, bias, nullptr, y, B, C, K, H, W, nblk,
      (H / 2) * (W / 2), nsplit, ws, nullptr, stream);
}

extern "C" int skp_conv3x3_wino2_gn(const float* x, const float* U, const float* bias, const float* residual, float* y,
                                    int B, int C, int K, int H, int W, int nsplit, float* ws, float* gn_part,
                                    void* stream) {
  const ConvArgs a{x && U && y, all_aligned16({x, U, y, residual, ws}), ws, gn_part, B, C, K, H, W, nsplit, 1};
  const char* err = conv_args_error(kHW32 | kOr16x16 | kOffsets32, a);
  // half-height blocks (32 × 16 pixels, 4 waves, two workgroups per CU: one's prologue / epilogue
  // overlaps the other's stage loop), 5-11% faster than the 32 × 32 one-workgroup-per-CU form (since
  // removed) at every VAE / UNet shape (profiles/r03al_wino_half_ab.txt); the 16×16 geometry as two images per
  // 4-wave workgroup, two workgroups per CU (profiles/r03ap_wino_half16_ab.txt)
  const bool g16 = H == 16 && W == 16;
  const long long nblk = g16 ? B / 2 : (long long)B * (H / 16) * (W / 32);
  if (!err && nblk * (K / w2::kNC) * nsplit > kMaxGrid) err = "grid too large";
  SKP_CHECK_ARG(!err, err);
  return wino2_launch<4>(
      __func__, [g16](auto E) -> W2Kernel { return g16 ? wino2_kernel<E(), 4> : wino2_kernel<E(), 8>; }, x, U, bias,
      residual, y, B, C, K, H, W, nblk, H * W, nsplit, ws, gn_part, stream);
}

extern "C" int skp_conv3x3_wino2(const float* x, const float* U, const float* bias, const float* residual, float* y,
                                 int B, int C, int K, int H, int W, int nsplit, float* ws, void* stream) {
  return skp_conv3x3_wino2_gn(x, U, bias, residual, y, B, C, K, H, W, nsplit, ws, nullptr, stream);
}

// ---------------------------------------------------------------- V-staged form (transform once)
// skp_wino2_vtransform(_gn) writes V = Bᵀ d B of every input tile once; skp_conv3x3_wino2_v(_gn)
// is skp_conv3x3_wino2(_gn) reading V instead of x.  V layout (include/skp.h): per (half-height
// block, 4-channel stage) one 18-KB slab [wave 2·half + wm][chunk j][lane], each lane's a[18] as
// four 16-B chunks and one 8-B chunk, so that a wave stores / loads whole contiguous 1-KB (512-B)
// pieces and lane L of wave q reads exactly what lane L of wave q wrote; no pad floats.  Bytes
// model of the transform pass at (B, C, H, W): reads x once from HBM (4 B per element; the halo
// rows / columns of a block, 1.4× the block in all, come from L2) and writes 36 floats per 4×4
// tile (9 B per element): 4 + 9 = 13 B per element against the 8 B of the gn_apply pass it
// replaces; the convolution then fetches 9 B per element once from HBM (its other K/32 − 1 reads
// hit L2) instead of 4.
namespace {
int vtransform_launch(const float* x, const float* stats, const float* gamma, const float* beta, const float* shift,
                      int G, int act, float* V, int B, int C, int H, int W, void* stream) {
  const int bw = W / 32, bpi = (H / 16) * bw;
  const long long nwg = (long long)B * bpi * (C / w2::kCK);
  if (nwg > kMaxGrid) return -2;
  const dim3 grid((unsigned)nwg), block(4 * WAVE);
  hipStream_t st = as_stream(stream);
  if (!stats) hipLaunchKernelGGL(wino2_vtransform_kernel<0>, grid, block, 0, st, x, stats, gamma, beta, shift, G, V, C, H, W, bw, bpi);
  else if (!act) hipLaunchKernelGGL(wino2_vtransform_kernel<1>, grid, block, 0, st, x, stats, gamma, beta, shift, G, V, C, H, W, bw, bpi);
  else hipLaunchKernelGGL(wino2_vtransform_kernel<2>, grid, block, 0, st, x, stats, gamma, beta, shift, G, V, C, H, W, bw, bpi);
  return 0;
}
}  // namespace

extern "C" int skp_wino2_vtransform(const float* x, float* V, int B, int C, int H, int W, void* stream) {
  const ConvArgs a{x && V, all_aligned16({x, V}), nullptr, nullptr, B, C, w2::kNC, H, W, 1, 1};
  const char* err = conv_args_error(kHW32, a);
  if (!err && vtransform_launch(x, nullptr, nullptr, nullptr, nullptr, 0, 0, V, B, C, H, W, stream) != 0)
    err = "grid too large";
  SKP_CHECK_ARG(!err, err);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_wino2_vtransform_gn(const float* x, const float* stats, const float* gamma, const float* beta,
                                       const float* shift, int G, int act, float* V, int B, int C, int H, int W,
                                       void* stream) {
  const ConvArgs a{x && V && stats && gamma && beta, all_aligned16({x, V}), nullptr, nullptr, B, C, w2::kNC, H, W, 1, G};
  const char* err = conv_args_error(kHW32, a);
  if (!err && vtransform_launch(x, stats, gamma, beta, shift, G, act, V, B, C, H, W, stream) != 0)
    err = "grid too large";
  SKP_CHECK_ARG(!err, err);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_conv3x3_wino2_v_gn(const float* V, const float* U, const float* bias, const float* residual,
                                      float* y, int B, int C, int K, int H, int W, int nsplit, float* ws,
                                      float* gn_part, void* stream) {
  const ConvArgs a{V && U && y, all_aligned16({V, U, y, residual, ws}), ws, gn_part, B, C, K, H, W, nsplit, 1};
  const char* err = conv_args_error(kHW32, a);
  const long long nblk = (long long)B * (H / 16) * (W / 32);
  if (!err && nblk * (K / w2::kNC) * nsplit > kMaxGrid) err = "grid too large";
  SKP_CHECK_ARG(!err, err);
  return wino2_launch<4>(
      __func__, [](auto E) -> W2Kernel { return wino2v_kernel<E()>; }, V, U, bias, residual, y, B, C, K, H, W, nblk, H * W,
      nsplit, ws, gn_part, stream);
}

extern "C" int skp_conv3x3_wino2_v(const float* V, const float* U, const float* bias, const float* residual, float* y,
                                   int B, int C, int K, int H, int W, int nsplit, float* ws, void* stream) {
  return skp_conv3x3_wino2_v_gn(V, U, bias, residual, y, B, C, K, H, W, nsplit, ws, nullptr, stream);
}
