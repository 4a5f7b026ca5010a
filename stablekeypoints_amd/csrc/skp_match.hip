// Dense nearest-pixel field between two sets of pixel signatures (skp_match_field): for every column
// p of X (n, P) the column q of Y (n, Q) with the greatest cosine, on the exact-f32 matrix cores
// (v_mfma_f32_32x32x2_f32).  It is a GEMM whose product never leaves registers: the epilogue of a
// 128×128 block of dots scales them by 1/|y_q| and folds them into a running (key, q) per pixel p.
//
// Arithmetic (include/skp.h states it in full): norms and dots are fmaf chains in token order with one
// accumulator per (p, q) and no split over the tokens.  The MFMA is bit for bit such a chain over its
// two k, lanes 0-31 feeding the first and lanes 32-63 the second, so MFMA i of a panel takes tokens
// 2i and 2i + 1 and consecutive MFMAs continue the chain.  Tokens past n are fed as zeros in both
// operands (fmaf(0, 0, d) = d), so a key depends neither on the tile its p or q falls in, nor on the
// split of Q, nor on the image's place in the batch.
//
// Tile scheme: one 256-thread workgroup owns 128 pixels p of one image and a contiguous range of
// 128-wide q tiles (Q is split over workgroups only as far as filling the device needs).  Y is the
// MFMA's row operand and X its column operand: a lane's 16 accumulators of a 32×32 block are 16 q of
// ONE p, so the running (key, q) of that p lives in two registers through the whole q loop and the
// lane halves and the two q-waves meet once, at the end.  Both operands have unit stride along their
// pixels: the [k][pixel] LDS layout of skp_gemm.hip, filled through registers one panel of 32 tokens
// ahead of the MFMAs.  A lane walks its q in ascending order, so "the lowest q with the greatest key"
// is a strict > there; the merges (lane halves, waves, splits) compare (key, q) pairs in full.
//
// The norms ride along: the panels pass through LDS in token order anyway, so 128 threads carry the
// fmaf chain of one Y column each through a q tile's panels (and, in a workgroup's first q tile, the
// other 128 that of an X column), and the tile's epilogue reads 1/|y_q| from LDS.  No pass over the
// operands besides the products'.
//
// Grid: workgroup w runs on XCD w % 8; the units (image, p tile, split) are numbered with the split
// fastest and XCD x takes a contiguous range of them, so the workgroups that re-read one X panel
// share an L2.  Partials go to the workspace as (image, split, p); match_merge_kernel walks them in
// split order and writes index and score (rx, 1/|x_p|, is left by each p tile's first split).  No
// atomics: two runs give the same bits.
#include <algorithm>

#include "skp_common.h"

using namespace skp;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BK = 32;          // tokens per LDS panel
constexpr int BT = 128;         // pixels of X and of Y per workgroup tile
constexpr int LDT = BT + 4;     // [k][pixel] row stride (floats)
constexpr int kThreads = 256;   // 2×2 waves of 64 q × 64 p
constexpr int kSlots = 512;     // workgroups that fill the device: 256 CUs × 2 (67.6 KB of LDS each)
constexpr int kMaxSplit = 32;

// The workspace and the split of Q, stated once: the query returns `bytes`, the entry point takes
// the offsets.  rx is the reciprocal norm of every x column (NaN where it is not usable), part_k and
// part_q one (key, q) per (image, split, p).
struct Plan {
  int pt, qt, splits, per;   // p tiles, q tiles, splits of Q, q tiles per split
  long long units;           // B · pt · splits workgroups with work
  long long rx, part_k, part_q, bytes;
};

long long r8(long long b) { return (b + 7) & ~7LL; }

const char* plan(int B, int n, int P, int Q, Plan& L) {
  if (B < 1 || n < 1 || P < 1 || Q < 1) return "B, n, P and Q must be at least 1";
  if (n > 4096) return "n > 4096";
  if (P > (1 << 20) || Q > (1 << 20)) return "P or Q above 2^20";
  L.pt = (P + BT - 1) / BT, L.qt = (Q + BT - 1) / BT;
  const long long rows = (long long)B * L.pt;
  const long long want = std::min<long long>({(kSlots + rows - 1) / rows, (long long)L.qt, (long long)kMaxSplit});
  L.per = (int)((L.qt + want - 1) / want);
  L.splits = (L.qt + L.per - 1) / L.per;   // no split is empty
  L.units = rows * L.splits;
  L.rx = 0;
  L.part_k = L.rx + r8(4LL * B * P);
  L.part_q = L.part_k + r8(4LL * B * L.splits * P);
  L.bytes = L.part_q + r8(4LL * B * L.splits * P);
  if (L.bytes >= (1LL << 31) || L.units + 8 >= (1LL << 31)) return "workspace of 2^31 bytes or more";
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

// One panel (BK tokens × BT pixels) of an operand through registers: BK·BT/4 float4 slots over the
// workgroup.  Branch-free as skp_gemm.hip's loader: a slot outside the operand loads a clamped
// in-range address and is zeroed on its way to LDS.  VEC: pixels % 4 == 0 and 16-B aligned rows, so a
// quad is all in or all out; otherwise four scalar loads with a mask each.
template <bool VEC>
struct PanelLoader {
  static constexpr int NS = BK * BT / 4 / kThreads;
  static constexpr int QT = BT / 4;   // float4 slots per token row
  float4 r[NS];
  int keep[NS][VEC ? 1 : 4];
  __device__ __forceinline__ void load(const float* __restrict__ base, int cols, int c0, int k0, int n) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int e = (int)threadIdx.x + i * kThreads;
      const int k = k0 + e / QT, c = c0 + 4 * (e % QT);
      const float* row = base + (size_t)min(k, n - 1) * cols;
      if (VEC) {
        r[i] = *reinterpret_cast<const float4*>(row + min(c, cols - 4));
        keep[i][0] = -(int)(k < n && c < cols);
      } else {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          keep[i][u] = -(int)(k < n && c + u < cols);
          v[u] = row[min(c + u, cols - 1)];
        }
        r[i] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ S) const {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int e = (int)threadIdx.x + i * kThreads;
      const int m0 = keep[i][0], m1 = keep[i][VEC ? 0 : 1], m2 = keep[i][VEC ? 0 : 2], m3 = keep[i][VEC ? 0 : 3];
      *reinterpret_cast<float4*>(S + (e / QT) * LDT + 4 * (e % QT)) =
          make_float4(__int_as_float(__float_as_int(r[i].x) & m0), __int_as_float(__float_as_int(r[i].y) & m1),
                      __int_as_float(__float_as_int(r[i].z) & m2), __int_as_float(__float_as_int(r[i].w) & m3));
    }
  }
};

struct FieldArgs {
  const float *x, *y;
  long long xs, ys;   // per-image strides of x and y (0: shared)
  float* rx;          // (B, P)
  float* part_k;
  int* part_q;
  int P, Q, n, pt, qt, splits, per, units;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void match_field_kernel(const FieldArgs A) {
  __shared__ __attribute__((aligned(16))) float Xs[2][BK * LDT];
  __shared__ __attribute__((aligned(16))) float Ys[2][BK * LDT];
  __shared__ float s_ry[2][BT];   // 1 / |y_q| of the q tile, by the tile's parity
  __shared__ float s_k[BT];
  __shared__ int s_q[BT];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int h = lane >> 5, r = lane & 31;
  const int wq = (wid >> 1) * 64, wp = (wid & 1) * 64;
  const int per_x = (A.units + 7) >> 3;   // units per XCD; the grid is 8 · per_x
  const int u = ((int)blockIdx.x & 7) * per_x + ((int)blockIdx.x >> 3);
  if (u >= A.units) return;
  const int split = u % A.splits, ptile = (u / A.splits) % A.pt, b = u / (A.splits * A.pt);
  const int t_lo = split * A.per, mine = min(A.qt, t_lo + A.per) - t_lo;
  const float* __restrict__ X = A.x + b * A.xs;
  const float* __restrict__ Y = A.y + b * A.ys;
  const int p0 = ptile * BT, npanel = (A.n + BK - 1) / BK;

  // the loads run one (q tile, panel) step ahead of the MFMAs; the last step re-loads itself
  PanelLoader<VEC> lx, ly;
  int lt = 0, lp = 0;
  auto issue = [&]() {
    lx.load(X, A.P, p0, lp * BK, A.n);
    ly.load(Y, A.Q, (t_lo + lt) * BT, lp * BK, A.n);
  };
  auto advance = [&]() {
    if (lp + 1 < npanel) ++lp;
    else if (lt + 1 < mine) ++lt, lp = 0;
  };
  issue();
  advance();
  lx.store(Xs[0]);
  ly.store(Ys[0]);
  __syncthreads();

  float bk[2] = {-INFINITY, -INFINITY};   // this lane's best of p = p0 + wp + 32·pi + r
  int bq[2] = {-1, -1};
  // the norm chains: threads 128-255 (waves 2, 3) one Y column of the q tile each, threads 0-127 one X
  // column of the p tile in the workgroup's first q tile; tokens past n and columns outside are zeros
  const bool ycol = threadIdx.x >= BT;
  const int ncol = threadIdx.x & (BT - 1);
  float nrm = 0.0f;
  int s = 0;
  for (int t = 0; t < mine; ++t) {
    f32x16 acc[2][2];   // [qi][pi]
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
#pragma unroll
      for (int pi = 0; pi < 2; ++pi)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[qi][pi][i] = 0.0f;
    for (int p = 0; p < npanel; ++p, ++s) {
      const int cur = s & 1;
      issue();
      advance();
      __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the MFMAs
      if (ycol || t == 0) {
        const float* col = (ycol ? Ys[cur] : Xs[cur]) + ncol;
#pragma unroll
        for (int k = 0; k < BK; ++k) nrm = __fmaf_rn(col[k * LDT], col[k * LDT], nrm);
        if (p == npanel - 1) {
          const float rv = recip_norm(nrm);
          if (ycol) s_ry[t & 1][ncol] = rv;
          else if (split == 0 && p0 + ncol < A.P) A.rx[(size_t)b * A.P + p0 + ncol] = rv;
          nrm = 0.0f;
        }
      }
      const float* ys = Ys[cur] + h * LDT + wq + r;
      const float* xs = Xs[cur] + h * LDT + wp + r;
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) {   // tokens 2kk (lanes 0-31) and 2kk + 1 (lanes 32-63)
        const float a0 = ys[2 * kk * LDT], a1 = ys[2 * kk * LDT + 32];
        const float b0 = xs[2 * kk * LDT], b1 = xs[2 * kk * LDT + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      lx.store(Xs[cur ^ 1]);
      ly.store(Ys[cur ^ 1]);
      __syncthreads();
    }
    // the tile's 64 q of this wave, ascending within the lane: row = 32·qi + 8·(i / 4) + 4·h + i % 4
    // (a column past Q is zeros: its 1 / |y_q| is NaN, not usable)
    const int ql = wq + 4 * h, qb = (t_lo + t) * BT + ql;
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int o = 32 * qi + 8 * (i >> 2) + (i & 3), q = qb + o;
        const float rv = s_ry[t & 1][ql + o];
        const bool usable = rv == rv;
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) {
          float key = acc[qi][pi][i] * rv;
          key = key == key ? key : -INFINITY;
          if (usable && (bq[pi] < 0 || key > bk[pi])) bk[pi] = key, bq[pi] = q;
        }
      }
  }

  // the lane halves hold the same p with interleaved q; then the two q-waves of each p meet in LDS
#pragma unroll
  for (int pi = 0; pi < 2; ++pi) {
    const float ok = __shfl_xor(bk[pi], 32, 64);
    const int oq = __shfl_xor(bq[pi], 32, 64);
    if (match_better(ok, oq, bk[pi], bq[pi])) bk[pi] = ok, bq[pi] = oq;
  }
  if (wq != 0 && h == 0) {
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) s_k[wp + 32 * pi + r] = bk[pi], s_q[wp + 32 * pi + r] = bq[pi];
  }
  __syncthreads();
  if (wq == 0 && h == 0) {
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) {
      const int c = wp + 32 * pi + r, p = p0 + c;
      if (match_better(s_k[c], s_q[c], bk[pi], bq[pi])) bk[pi] = s_k[c], bq[pi] = s_q[c];
      if (p < A.P) {
        const size_t o = ((size_t)b * A.splits + split) * A.P + p;
        A.part_k[o] = bk[pi];
        A.part_q[o] = bq[pi];
      }
    }
  }
}

// The splits of every (image, p) in split order, then score = key · rx; −1 and −inf where p is not
// usable or no q is.
__global__ __launch_bounds__(kThreads) void match_merge_kernel(const float* __restrict__ part_k,
                                                               const int* __restrict__ part_q,
                                                               const float* __restrict__ rx, int P,
                                                               int splits, int blocks_per, int* __restrict__ index,
                                                               float* __restrict__ score) {
  const int b = (int)blockIdx.x / blocks_per;
  const int p = ((int)blockIdx.x % blocks_per) * kThreads + (int)threadIdx.x;
  if (p >= P) return;
  float bk = -INFINITY;
  int bq = -1;
  for (int s = 0; s < splits; ++s) {
    const size_t o = ((size_t)b * splits + s) * P + p;
    const float k = part_k[o];
    const int q = part_q[o];
    if (match_better(k, q, bk, bq)) bk = k, bq = q;
  }
  const float rv = rx[(size_t)b * P + p];
  const bool ok = rv == rv && bq >= 0;
  index[(size_t)b * P + p] = ok ? bq : -1;
  score[(size_t)b * P + p] = ok ? bk * rv : -INFINITY;
}

template <class T>
T* at(void* workspace, long long offset) {
  return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset);
}

}  // namespace

extern "C" int skp_match_field_workspace(int B, int n, int P, int Q) {
  Plan L;
  return plan(B, n, P, Q, L) ? -1 : (int)L.bytes;
}

extern "C" int skp_match_field(const float* x, long long x_stride, int P, const float* y, long long y_stride, int Q,
                               int B, int n, int* index, float* score, void* workspace, void* stream) {
  SKP_CHECK_ARG(x && y && index && score && workspace, "null pointer");
  Plan L;
  const char* bad = plan(B, n, P, Q, L);
  SKP_CHECK_ARG(!bad, bad);
  SKP_CHECK_ARG(x_stride == 0 || x_stride >= (long long)n * P, "x_stride must be 0 or at least n*P");
  SKP_CHECK_ARG(y_stride == 0 || y_stride >= (long long)n * Q, "y_stride must be 0 or at least n*Q");
  SKP_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "workspace must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  FieldArgs A;
  A.x = x, A.y = y, A.rx = at<float>(workspace, L.rx);
  A.xs = x_stride, A.ys = y_stride;
  A.part_k = at<float>(workspace, L.part_k), A.part_q = at<int>(workspace, L.part_q);
  A.P = P, A.Q = Q, A.n = n, A.pt = L.pt, A.qt = L.qt, A.splits = L.splits, A.per = L.per, A.units = (int)L.units;
  const int grid = 8 * (int)((L.units + 7) / 8);
  const bool vec = P % 4 == 0 && Q % 4 == 0 && x_stride % 4 == 0 && y_stride % 4 == 0 &&
                   (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
  if (vec) hipLaunchKernelGGL(match_field_kernel<true>, dim3(grid), dim3(kThreads), 0, st, A);
  else hipLaunchKernelGGL(match_field_kernel<false>, dim3(grid), dim3(kThreads), 0, st, A);
  const int pb = (P + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(match_merge_kernel, dim3(B * pb), dim3(kThreads), 0, st, A.part_k, A.part_q, A.rx,
                     P, L.splits, pb, index, score);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}
