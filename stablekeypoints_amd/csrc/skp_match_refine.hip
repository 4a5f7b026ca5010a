// Windowed refine of a coarse match field (skp_match_refine): for every pixel p of X the best pixel q
// of Y inside a (2w + 1)² window whose centre the coarse field gives, with skp_match_field's keys bit
// for bit.  A register-blocked fmaf kernel: on gfx950 the f32 VALU rate equals the f32 MFMA rate, and
// fmaf(x, y, d) per token with one accumulator per (p, q) is the defined chain itself.
//
// Arithmetic (include/skp.h states it in full): norms and dots are fmaf chains in token order, one
// accumulator per (p, q), no split over the tokens.  Tokens past n are fed as zeros in both operands
// (fmaf(0, 0, d) = d), so a key depends neither on the pass or slot its q falls in nor on the image's
// place in the batch.
//
// Tile scheme: one 256-thread workgroup owns one f × f cell of one image's x grid.  Its f² pixels share
// one prior, so together they need one (f + 2w)² region of y, clipped to the plane: RH × RW pixels,
// numbered row-major (ascending in q).  The region goes through the workgroup in passes of YC pixels;
// a thread owns one y pixel of the pass and A x pixels of the cell (acc[A] in registers), TX threads
// share a y pixel:
//     f = 1      A = 1,  TX = 1, YC = 256        f = 3, 4    A = 16, TX = 1, YC = 256
//     f = 2      A = 4,  TX = 1, YC = 256        f = 5 … 8   A = 16, TX = 4, YC = 64
// (x slots past f² hold zeros and lie in no window).  Both operands pass through LDS in panels of 16
// tokens, [k][pixel], loaded to registers one panel ahead of the fmafs; a thread reads its y value
// once per token and its x values as broadcast float4.  The y norm rides along in the thread that owns
// the pixel, the x norms in the first pass.  After a pass's last panel the thread scales its dots by
// 1 / |y_q|, drops the (p, q) outside p's window and folds the rest into its running (key, q) per x
// pixel; q ascends over the passes, so that fold is a strict >.  At the end the lanes of a wave meet by
// shuffles and the waves in LDS, comparing (key, q) pairs in full, and f² threads write index and
// score.  A cell whose prior is outside [0, Sc²) writes −1 / −inf and reads nothing else.
//
// LDS: 16·(YC + A·TX) floats and a few words: 17.6 KB (A = 16, TX = 1), 9.0 KB (TX = 4).  Occupancy is
// bound by registers: 188 VGPRs at A = 16, TX = 1 (16 accumulators, 16 (key, q) pairs, 17 words in
// flight and the unrolled panel's operands), so two workgroups per CU, two waves per SIMD; 160 VGPRs
// and three at TX = 4, 101 and four at f = 1.  DESIGN.md 5.8 has what was measured and what bounds it.
//
// Grid: workgroup g runs on XCD g % 8; the cells are numbered image, cell row, cell column and XCD x
// takes a contiguous range of them, so the cells of a band of rows, whose regions overlap wherever the
// coarse field is coherent, share an L2.  One launch, no atomics, no workspace traffic: two runs give
// the same bits.
#include "skp_common.h"

using namespace skp;

namespace {

constexpr int BK = 16;          // tokens per LDS panel
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE;

// What both entry points reject, and the number of cells.
const char* plan(int B, int n, int S, int f, int w, long long& units) {
  if (B < 1 || n < 1 || S < 1) return "B, n and S must be at least 1";
  if (n > 4096) return "n > 4096";
  if (S > 1024) return "S > 1024";
  if (f < 1 || f > 8) return "f must be in [1, 8]";
  if (S % f != 0) return "S must be a multiple of f";
  if (w < 1 || w > 16) return "w must be in [1, 16]";
  units = (long long)B * (S / f) * (S / f);
  if (units + 8 >= (1LL << 31)) return "B * (S / f)^2 of 2^31 or more";
  return nullptr;
}

// 1 / sqrt(norm), both correctly rounded; NaN where the column is not usable (norm not in (0, +inf))
__device__ __forceinline__ float recip_norm(float s) {
  return (s > 0.0f && s < INFINITY) ? __fdiv_rn(1.0f, sqrt_rn(s)) : __int_as_float(0x7fc00000);
}

// (k1, q1) beats (k0, q0): a pair with q < 0 holds nothing; the greater key wins, on equal keys the lower q
__device__ __forceinline__ bool match_better(float k1, int q1, float k0, int q0) {
  return q1 >= 0 && (q0 < 0 || k1 > k0 || (k1 == k0 && q1 < q0));
}

struct RefineArgs {
  const float *x, *y;
  long long xs, ys;    // per-image strides of x and y (0: shared)
  const int* coarse;   // (B, Sc²)
  int* index;          // (B, S²)
  float* score;
  int S, Sc, n, f, w, units;
};

template <int A, int TX>
__global__ __launch_bounds__(kThreads) void match_refine_kernel(const RefineArgs P) {
  constexpr int YC = kThreads / TX;                              // y pixels per pass
  constexpr int XP = A * TX;                                     // x slots (>= f²)
  constexpr int NY = BK / TX;                                    // y loads per thread and panel
  constexpr int NX = (BK * XP + kThreads - 1) / kThreads;        // x loads per thread and panel
  __shared__ __attribute__((aligned(16))) float Ys[BK * YC];
  __shared__ __attribute__((aligned(16))) float Xs[BK * XP];
  __shared__ float s_rx[XP];
  __shared__ int s_off[XP];   // (row, column) of x slot i inside the cell, packed; far away past f²
  __shared__ float s_k[kWaves][A];
  __shared__ int s_q[kWaves][A];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int per_x = (P.units + 7) >> 3;   // cells per XCD; the grid is 8 · per_x
  const int u = ((int)blockIdx.x & 7) * per_x + ((int)blockIdx.x >> 3);
  if (u >= P.units) return;
  const int S = P.S, Sc = P.Sc, f = P.f, w = P.w, n = P.n, ff = f * f;
  const int cells = Sc * Sc, b = u / cells, cell = u - b * cells;
  const int r0 = (cell / Sc) * f, c0 = (cell % Sc) * f;   // the cell's first pixel
  const size_t plane = (size_t)S * S;
  const int m = P.coarse[(size_t)b * cells + cell];
  if (m < 0 || m >= cells) {   // no prior: uniform over the workgroup
    if (tid < ff) {
      const size_t o = (size_t)b * plane + (size_t)(r0 + tid / f) * S + c0 + tid % f;
      P.index[o] = -1;
      P.score[o] = -INFINITY;
    }
    return;
  }
  const int cr0 = (m / Sc) * f, cc0 = (m % Sc) * f;   // the centre of the cell's pixel (0, 0)
  const int R0 = max(cr0 - w, 0), C0 = max(cc0 - w, 0);
  const int RH = min(cr0 + f - 1 + w, S - 1) - R0 + 1, RW = min(cc0 + f - 1 + w, S - 1) - C0 + 1;
  const int RN = RH * RW, npass = (RN + YC - 1) / YC, npanel = (n + BK - 1) / BK;
  const float* __restrict__ X = P.x + b * P.xs;
  const float* __restrict__ Y = P.y + b * P.ys;

  if (tid < XP) s_off[tid] = tid < ff ? (tid / f) | ((tid % f) << 16) : 0x40004000;
  // this thread's x loads: element e = tid + i·256 of a panel is token e / XP, slot e % XP = tid % XP
  const int xslot = tid % XP, xk = tid / XP;
  const bool xin = xslot < ff && (NX > 1 || tid < BK * XP);
  const size_t xoff = xin ? (size_t)(r0 + xslot / f) * S + c0 + xslot % f : 0;
  const int j = tid % YC, g = tid / YC;   // the y pixel of a pass and the group of A x slots

  float bk[A], xn = 0.0f;
  int bq[A];
#pragma unroll
  for (int a = 0; a < A; ++a) bk[a] = -INFINITY, bq[a] = -1;

  for (int pass = 0; pass < npass; ++pass) {
    const int jj = pass * YC + j;
    const bool yin = jj < RN;
    const int ry = yin ? jj / RW : 0, qr = R0 + ry, qc = C0 + (yin ? jj - ry * RW : 0);
    const size_t yoff = (size_t)qr * S + qc;
    float ly[NY], lx[NX];
    auto issue = [&](int k0) {
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        const int k = k0 + g + i * TX;
        ly[i] = (yin && k < n) ? Y[(size_t)k * plane + yoff] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int k = k0 + xk + i * (kThreads / XP);
        lx[i] = (xin && k < n) ? X[(size_t)k * plane + xoff] : 0.0f;
      }
    };
    float acc[A], nrm = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) acc[a] = 0.0f;
    issue(0);
    for (int p = 0; p < npanel; ++p) {
#pragma unroll
      for (int i = 0; i < NY; ++i) Ys[(g + i * TX) * YC + j] = ly[i];
#pragma unroll
      for (int i = 0; i < NX; ++i)
        if (NX > 1 || tid < BK * XP) Xs[(xk + i * (kThreads / XP)) * XP + xslot] = lx[i];
      __syncthreads();
      if (p + 1 < npanel) issue((p + 1) * BK);
      if (pass == 0 && tid < XP) {
#pragma unroll
        for (int k = 0; k < BK; ++k) xn = __fmaf_rn(Xs[k * XP + tid], Xs[k * XP + tid], xn);
      }
#pragma unroll
      for (int k = 0; k < BK; ++k) {
        const float yv = Ys[k * YC + j];
        nrm = __fmaf_rn(yv, yv, nrm);
        if constexpr (A >= 4) {
#pragma unroll
          for (int v = 0; v < A / 4; ++v) {
            const float4 xv = *reinterpret_cast<const float4*>(Xs + k * XP + g * A + 4 * v);
            acc[4 * v + 0] = __fmaf_rn(xv.x, yv, acc[4 * v + 0]);
            acc[4 * v + 1] = __fmaf_rn(xv.y, yv, acc[4 * v + 1]);
            acc[4 * v + 2] = __fmaf_rn(xv.z, yv, acc[4 * v + 2]);
            acc[4 * v + 3] = __fmaf_rn(xv.w, yv, acc[4 * v + 3]);
          }
        } else {
#pragma unroll
          for (int a = 0; a < A; ++a) acc[a] = __fmaf_rn(Xs[k * XP + g * A + a], yv, acc[a]);
        }
      }
      __syncthreads();
    }
    // this pass's y pixel against the A x slots: the key, the window, the fold (q ascends over the passes)
    const float rv = recip_norm(nrm);
    if (yin && rv == rv) {
      const int q = qr * S + qc, dqr = qr - cr0, dqc = qc - cc0;
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const int off = s_off[g * A + a];
        float key = acc[a] * rv;
        key = key == key ? key : -INFINITY;
        const bool in = abs(dqr - (off & 0xffff)) <= w && abs(dqc - (off >> 16)) <= w;
        if (in && (bq[a] < 0 || key > bk[a])) bk[a] = key, bq[a] = q;
      }
    }
  }
  if (tid < XP) s_rx[tid] = recip_norm(xn);

  // the lanes of a wave hold different q of the same x slots; then the waves meet in LDS
#pragma unroll
  for (int a = 0; a < A; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk[a], o, 64);
      const int oq = __shfl_xor(bq[a], o, 64);
      if (match_better(ok, oq, bk[a], bq[a])) bk[a] = ok, bq[a] = oq;
    }
    if (lane == 0) s_k[wid][a] = bk[a], s_q[wid][a] = bq[a];
  }
  __syncthreads();
  if (tid < ff) {
    const int a = tid % A, grp = tid / A;   // TX == 1: every wave holds slot a; else wave grp alone
    float k = -INFINITY;
    int q = -1;
#pragma unroll
    for (int v = 0; v < kWaves; ++v)
      if ((TX == 1 || v == grp) && match_better(s_k[v][a], s_q[v][a], k, q)) k = s_k[v][a], q = s_q[v][a];
    const float rv = s_rx[tid];
    const bool ok = rv == rv && q >= 0;
    const size_t o = (size_t)b * plane + (size_t)(r0 + tid / f) * S + c0 + tid % f;
    P.index[o] = ok ? q : -1;
    P.score[o] = ok ? k * rv : -INFINITY;
  }
}

}  // namespace

extern "C" int skp_match_refine_workspace(int B, int n, int S, int f, int w) {
  long long units;
  return plan(B, n, S, f, w, units) ? -1 : 8;
}

extern "C" int skp_match_refine(const float* x, long long x_stride, const float* y, long long y_stride, int B, int n,
                                int S, const int* coarse, int f, int w, int* index, float* score, void* workspace,
                                void* stream) {
  SKP_CHECK_ARG(x && y && coarse && index && score && workspace, "null pointer");
  long long units;
  const char* bad = plan(B, n, S, f, w, units);
  SKP_CHECK_ARG(!bad, bad);
  const long long per = (long long)n * S * S;
  SKP_CHECK_ARG(x_stride == 0 || x_stride >= per, "x_stride must be 0 or at least n*S*S");
  SKP_CHECK_ARG(y_stride == 0 || y_stride >= per, "y_stride must be 0 or at least n*S*S");
  SKP_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "workspace must be 8-byte aligned");
  RefineArgs A;
  A.x = x, A.y = y, A.xs = x_stride, A.ys = y_stride;
  A.coarse = coarse, A.index = index, A.score = score;
  A.S = S, A.Sc = S / f, A.n = n, A.f = f, A.w = w, A.units = (int)units;
  const dim3 grid(8 * (unsigned)((units + 7) / 8)), block(kThreads);
  hipStream_t st = as_stream(stream);
  if (f == 1) hipLaunchKernelGGL((match_refine_kernel<1, 1>), grid, block, 0, st, A);
  else if (f == 2) hipLaunchKernelGGL((match_refine_kernel<4, 1>), grid, block, 0, st, A);
  else if (f <= 4) hipLaunchKernelGGL((match_refine_kernel<16, 1>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((match_refine_kernel<16, 4>), grid, block, 0, st, A);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}
