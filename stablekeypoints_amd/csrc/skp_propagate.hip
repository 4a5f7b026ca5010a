// Label propagation through a video: the k best matches of a window centred on the pixel
// (skp_match_topk) and the vote of several context frames' lists (skp_label_vote).  include/skp.h
// states both definitions in full; DESIGN.md 5.9 has what was measured and what bounds the kernels.
//
// skp_match_topk.  Norms, dots and keys are skp_match_field's: fmaf chains in token order, one
// accumulator per (p, q), tokens past n fed as zeros in both operands (fmaf(0, 0, d) = d), so a key
// depends neither on the pass or slot its q falls in nor on the image's place in the batch.  The
// panel loop is skp_match_refine's at A = 16, TX = 1, with two y pixels per thread.
//
// Tile scheme: one 256-thread workgroup owns one 4 × 4 tile of one image's x grid (tiles past the
// plane's edge are partial: their x slots outside the plane hold zeros, lie in no window and write
// nothing).  The tile's 16 windows share one (4 + 2w)² region of y, clipped to the plane: RH × RW
// pixels, numbered row-major (ascending in q).  The region goes through the workgroup in passes of
// 512 pixels; a thread owns two y pixels of the pass and the 16 x pixels (acc[2][16] in registers):
// per token it reads its two y values and the x values as four broadcast float4, 6 LDS reads for 34
// fmafs where one y pixel per thread needs 5 for 17, and the x operand's broadcast reads are what
// set skp_match_refine's pace.  Both operands pass through LDS in panels of 8 tokens,
// [k][pixel], loaded to registers one panel ahead of the fmafs (panels of 16 would need 286
// registers); the y norms ride along in the thread that owns the pixel, the x norms in the first
// pass.
//
// Selection (the design decision): 32 accumulators beside 16 sorted K-lists do not fit in registers,
// and per-thread lists would have to be merged over 256 threads anyway.  So the lists live in LDS,
// one (key, q)[K] per x pixel, and each pass is folded into them by waves: after a pass's last panel
// every thread scales its dots by 1 / |y_q| and writes the keys into the y panel's LDS, which is free
// then ([x pixel][y pixel of the pass]; a NaN marks a pair outside the window or an unusable q, a key
// itself is never NaN), and its q beside them.  Wave v then takes x pixels 4v … 4v + 3 in turn: a
// lane holds eight of the pass's 512 candidates and lanes 0 … K − 1 one entry of the running list
// each, and K rounds of (lane maximum, six-step butterfly, strike the winner) extract the new list in
// order.  Pairs are compared in full, (key, q): the greater key, on equal keys the lower q; every q
// occurs once, so the winner's lane knows itself by q.  A round that finds nothing ends the rounds.
// Cost per pass and wave: 4 · K rounds of about 130 instructions against 32 · n fmafs per lane, so
// 2600 against 16000 at K = 5, n = 500 — and the selection dominates below about 80 tokens.
//
// One variant, <YPT = 2, BK = 8>: 230 VGPRs, no scratch, 37440 B of LDS (32 KB panel / keys, 0.5 KB x
// panel, 2 KB q, 2 KB lists): two workgroups per CU by registers, two waves per SIMD.  One y pixel
// per thread with panels of 16 (176 VGPRs, 20.5 KB, also two waves per SIMD) was measured 1.28× slower
// at n = 500 and 1.46× at n = 10.  One launch, no atomics, no workspace traffic (the query returns 8):
// two runs give the same bits.
//
// Grid: workgroup g runs on XCD g % 8; the tiles are numbered image, tile row, tile column and XCD x
// takes a contiguous range of them, so neighbouring tiles, whose regions overlap, share an L2.
//
// skp_label_vote.  One thread per pixel, coalesced over p.  The Kv best of the M · K candidates are
// taken by Kv scans in the order (score descending, j ascending, i ascending): round r takes the
// first candidate in that order that lies strictly after round r − 1's, so nothing is kept but the
// previous winner; the winners' (j, q) and weights wait in LDS, [rank][thread], for the loop over the
// classes.  Every operation is an _rn intrinsic (no contraction into fma); exp is expf.  One launch,
// 29 VGPRs, 32 KB of LDS, which allows five waves per SIMD.
#include "skp_common.h"

using namespace skp;

namespace {

constexpr int kThreads = 256;
constexpr int TS = 4;           // the x tile's side
constexpr int XP = TS * TS;     // x pixels per workgroup, the accumulators per thread
constexpr int KMAX = 16;

// What both entry points of skp_match_topk reject, and the number of tiles.
const char* plan(int B, int n, int S, int w, int K, long long& units) {
  if (B < 1 || n < 1 || S < 1) return "B, n and S must be at least 1";
  if (n > 4096) return "n > 4096";
  if (S > 1024) return "S > 1024";
  if (w < 1 || w > 16) return "w must be in [1, 16]";
  if (K < 1 || K > KMAX) return "K must be in [1, 16]";
  const long long tiles = (S + TS - 1) / TS;
  units = (long long)B * tiles * tiles;
  if (units + 8 >= (1LL << 31)) return "B * ceil(S / 4)^2 of 2^31 or more";
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

struct TopkArgs {
  const float *x, *y;
  long long xs, ys;    // per-image strides of x and y (0: shared)
  int* index;          // (B, K, S²)
  float* score;
  int S, n, w, K, tiles, units;
};

template <int YPT, int BK>   // y pixels per thread, tokens per LDS panel
__global__ __launch_bounds__(kThreads) void match_topk_kernel(const TopkArgs P) {
  constexpr int YC = kThreads * YPT;   // y pixels per pass; a thread owns pixels tid + 256·i of it
  __shared__ __attribute__((aligned(16))) float Ys[(BK > XP ? BK : XP) * YC];   // the y panel; after a pass's last panel its keys, [XP][YC]
  __shared__ __attribute__((aligned(16))) float Xs[BK * XP];
  __shared__ float s_rx[XP];
  __shared__ int s_qp[YC];          // q of the pass's y pixel, −1 where it is not usable
  __shared__ float s_lk[XP][KMAX];  // the running lists, (key descending, q ascending)
  __shared__ int s_lq[XP][KMAX];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int per_x = (P.units + 7) >> 3;   // tiles per XCD; the grid is 8 · per_x
  const int u = ((int)blockIdx.x & 7) * per_x + ((int)blockIdx.x >> 3);
  if (u >= P.units) return;
  const int S = P.S, w = P.w, n = P.n, K = P.K;
  const int tt = P.tiles * P.tiles, b = u / tt, t = u - b * tt;
  const int r0 = (t / P.tiles) * TS, c0 = (t % P.tiles) * TS;   // the tile's first pixel, inside the plane
  const size_t plane = (size_t)S * S;
  const int R0 = max(r0 - w, 0), C0 = max(c0 - w, 0);
  const int RH = min(r0 + TS - 1 + w, S - 1) - R0 + 1, RW = min(c0 + TS - 1 + w, S - 1) - C0 + 1;
  const int RN = RH * RW, npass = (RN + YC - 1) / YC, npanel = (n + BK - 1) / BK;
  const float* __restrict__ X = P.x + b * P.xs;
  const float* __restrict__ Y = P.y + b * P.ys;

  s_lk[tid >> 4][tid & 15] = -INFINITY;   // XP · KMAX = 256 entries; the panel loop's barriers come before their use
  s_lq[tid >> 4][tid & 15] = -1;
  // this thread's x load: element tid of a panel is token tid / 16, slot tid % 16
  const int xslot = tid & (XP - 1), xk = tid / XP;
  const bool xin = xk < BK && r0 + xslot / TS < S && c0 + xslot % TS < S;
  const size_t xoff = xin ? (size_t)(r0 + xslot / TS) * S + c0 + xslot % TS : 0;

  float xn = 0.0f;
  for (int pass = 0; pass < npass; ++pass) {
    bool yin[YPT];
    int qr[YPT], qc[YPT];
    size_t yoff[YPT];
#pragma unroll
    for (int i = 0; i < YPT; ++i) {
      const int jj = pass * YC + tid + kThreads * i;
      yin[i] = jj < RN;
      const int ry = yin[i] ? jj / RW : 0;
      qr[i] = R0 + ry, qc[i] = C0 + (yin[i] ? jj - ry * RW : 0);
      yoff[i] = (size_t)qr[i] * S + qc[i];
    }
    float ly[YPT][BK], lx;
    auto issue = [&](int k0) {
#pragma unroll
      for (int i = 0; i < YPT; ++i)
#pragma unroll
        for (int k = 0; k < BK; ++k) ly[i][k] = (yin[i] && k0 + k < n) ? Y[(size_t)(k0 + k) * plane + yoff[i]] : 0.0f;
      lx = (xin && k0 + xk < n) ? X[(size_t)(k0 + xk) * plane + xoff] : 0.0f;
    };
    float acc[YPT][XP], nrm[YPT];
#pragma unroll
    for (int i = 0; i < YPT; ++i) {
      nrm[i] = 0.0f;
#pragma unroll
      for (int a = 0; a < XP; ++a) acc[i][a] = 0.0f;
    }
    issue(0);
    for (int p = 0; p < npanel; ++p) {
#pragma unroll
      for (int i = 0; i < YPT; ++i)
#pragma unroll
        for (int k = 0; k < BK; ++k) Ys[k * YC + tid + kThreads * i] = ly[i][k];
      if (xk < BK) Xs[xk * XP + xslot] = lx;
      __syncthreads();
      if (p + 1 < npanel) issue((p + 1) * BK);
      if (pass == 0 && tid < XP) {
#pragma unroll
        for (int k = 0; k < BK; ++k) xn = __fmaf_rn(Xs[k * XP + tid], Xs[k * XP + tid], xn);
      }
#pragma unroll
      for (int k = 0; k < BK; ++k) {
        float yv[YPT];
#pragma unroll
        for (int i = 0; i < YPT; ++i) {
          yv[i] = Ys[k * YC + tid + kThreads * i];
          nrm[i] = __fmaf_rn(yv[i], yv[i], nrm[i]);
        }
#pragma unroll
        for (int v = 0; v < XP / 4; ++v) {
          const float4 xv = *reinterpret_cast<const float4*>(Xs + k * XP + 4 * v);
#pragma unroll
          for (int i = 0; i < YPT; ++i) {
            acc[i][4 * v + 0] = __fmaf_rn(xv.x, yv[i], acc[i][4 * v + 0]);
            acc[i][4 * v + 1] = __fmaf_rn(xv.y, yv[i], acc[i][4 * v + 1]);
            acc[i][4 * v + 2] = __fmaf_rn(xv.z, yv[i], acc[i][4 * v + 2]);
            acc[i][4 * v + 3] = __fmaf_rn(xv.w, yv[i], acc[i][4 * v + 3]);
          }
        }
      }
      __syncthreads();
    }
    // the pass's keys to LDS, [x pixel][y pixel]: NaN where the pair takes no part
#pragma unroll
    for (int i = 0; i < YPT; ++i) {
      const float rv = recip_norm(nrm[i]);
      const bool yok = yin[i] && rv == rv;
      s_qp[tid + kThreads * i] = yok ? qr[i] * S + qc[i] : -1;
#pragma unroll
      for (int a = 0; a < XP; ++a) {
        const int pr = r0 + a / TS, pc = c0 + a % TS;
        float key = acc[i][a] * rv;
        key = key == key ? key : -INFINITY;
        const bool in = yok && pr < S && pc < S && abs(qr[i] - pr) <= w && abs(qc[i] - pc) <= w;
        Ys[a * YC + tid + kThreads * i] = in ? key : __int_as_float(0x7fc00000);
      }
    }
    __syncthreads();
    // wave wid folds the pass into the lists of x pixels 4·wid … 4·wid + 3
    constexpr int NC = YC / WAVE + 1;   // a lane's candidates: its share of the pass and one entry of the list
    for (int s = 0; s < XP / 4; ++s) {
      const int a = wid * (XP / 4) + s;
      float ck[NC];
      int cq[NC];
#pragma unroll
      for (int i = 0; i < NC - 1; ++i) {
        ck[i] = Ys[a * YC + lane + WAVE * i];
        cq[i] = ck[i] == ck[i] ? s_qp[lane + WAVE * i] : -1;
      }
      ck[NC - 1] = lane < K ? s_lk[a][lane & (KMAX - 1)] : -INFINITY;
      cq[NC - 1] = lane < K ? s_lq[a][lane & (KMAX - 1)] : -1;
      for (int r = 0; r < K; ++r) {
        float bk = -INFINITY;
        int bq = -1;
#pragma unroll
        for (int i = 0; i < NC; ++i)
          if (match_better(ck[i], cq[i], bk, bq)) bk = ck[i], bq = cq[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ok = __shfl_xor(bk, o, 64);
          const int oq = __shfl_xor(bq, o, 64);
          if (match_better(ok, oq, bk, bq)) bk = ok, bq = oq;
        }
        if (bq < 0) {   // nothing left, uniform over the wave: the slots from r on hold nothing
          if (lane >= r && lane < K) s_lk[a][lane] = -INFINITY, s_lq[a][lane] = -1;
          break;
        }
        if (lane == r) s_lk[a][r] = bk, s_lq[a][r] = bq;
#pragma unroll
        for (int i = 0; i < NC; ++i)
          if (cq[i] == bq) cq[i] = -1;
      }
    }
    __syncthreads();   // the next pass's first panel overwrites the keys
  }
  if (tid < XP) s_rx[tid] = recip_norm(xn);
  __syncthreads();
  if (tid < XP * K) {
    const int a = tid & (XP - 1), i = tid / XP, pr = r0 + a / TS, pc = c0 + a % TS;
    if (pr < S && pc < S) {
      const float rv = s_rx[a], k = s_lk[a][i];
      const int q = s_lq[a][i];
      const bool ok = rv == rv && q >= 0;
      const size_t o = ((size_t)b * K + i) * plane + (size_t)pr * S + pc;
      P.index[o] = ok ? q : -1;
      P.score[o] = ok ? k * rv : -INFINITY;
    }
  }
}

struct VoteArgs {
  const int* index;      // (M, K, S²)
  const float* score;
  const float* labels;   // (M, Cl, S²)
  float *soft, *confidence;
  int *label, *source;   // source null: not written
  int M, K, Kv, Cl, plane;
  float inv_tau;
};

__global__ __launch_bounds__(kThreads) void label_vote_kernel(const VoteArgs P) {
  __shared__ int s_jq[KMAX][kThreads];    // rank r's context and pixel, j << 20 | q (q < 2^20, j < 64)
  __shared__ float s_e[KMAX][kThreads];   // its weight
  const int tid = threadIdx.x, plane = P.plane;
  const int p = (int)blockIdx.x * kThreads + tid;
  if (p >= plane) return;   // no barrier below: a thread reads only its own column of the two arrays
  const int MK = P.M * P.K, K = P.K;
  float ps = 0.0f, s1 = 0.0f, Z = 0.0f;
  int pc = -1, cnt = 0;
  for (int r = 0; r < P.Kv; ++r) {
    float bs = 0.0f;
    int bc = -1, bq = -1;
    for (int c = 0; c < MK; ++c) {   // c = j·K + i ascends in (j, i)
      const int q = P.index[(size_t)c * plane + p];
      if ((unsigned)q >= (unsigned)plane) continue;
      const float s = P.score[(size_t)c * plane + p];
      if (!(s == s)) continue;
      const bool after = r == 0 || s < ps || (s == ps && c > pc);
      if (after && (bc < 0 || s > bs)) bs = s, bc = c, bq = q;
    }
    if (bc < 0) break;
    if (r == 0) s1 = bs;
    const float e = expf(__fmul_rn(__fsub_rn(bs, s1), P.inv_tau));
    Z = __fadd_rn(Z, e);
    s_jq[r][tid] = ((bc / K) << 20) | bq;
    s_e[r][tid] = e;
    ps = bs, pc = bc, cnt = r + 1;
  }
  float best = 0.0f;
  int arg = -1;
  for (int c = 0; c < P.Cl; ++c) {
    float acc = 0.0f;
    for (int r = 0; r < cnt; ++r) {
      const int jq = s_jq[r][tid];
      const float l = P.labels[((size_t)(jq >> 20) * P.Cl + c) * plane + (jq & 0xfffff)];
      acc = __fadd_rn(acc, __fmul_rn(s_e[r][tid], l));
    }
    const float v = cnt ? __fdiv_rn(acc, Z) : 0.0f;
    P.soft[(size_t)c * plane + p] = v;
    if (cnt && (arg < 0 || v > best)) best = v, arg = c;
  }
  P.label[p] = arg;
  P.confidence[p] = best;
  if (P.source) {
    for (int r = 0; r < P.Kv; ++r) {
      const int jq = r < cnt ? s_jq[r][tid] : 0;
      P.source[(size_t)r * plane + p] = r < cnt ? (jq >> 20) * plane + (jq & 0xfffff) : -1;
    }
  }
}

}  // namespace

extern "C" int skp_match_topk_workspace(int B, int n, int S, int w, int K) {
  long long units;
  return plan(B, n, S, w, K, units) ? -1 : 8;
}

extern "C" int skp_match_topk(const float* x, long long x_stride, const float* y, long long y_stride, int B, int n,
                              int S, int w, int K, int* index, float* score, void* workspace, void* stream) {
  SKP_CHECK_ARG(x && y && index && score && workspace, "null pointer");
  long long units;
  const char* bad = plan(B, n, S, w, K, units);
  SKP_CHECK_ARG(!bad, bad);
  const long long per = (long long)n * S * S;
  SKP_CHECK_ARG(x_stride == 0 || x_stride >= per, "x_stride must be 0 or at least n*S*S");
  SKP_CHECK_ARG(y_stride == 0 || y_stride >= per, "y_stride must be 0 or at least n*S*S");
  SKP_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "workspace must be 8-byte aligned");
  TopkArgs A;
  A.x = x, A.y = y, A.xs = x_stride, A.ys = y_stride;
  A.index = index, A.score = score;
  A.S = S, A.n = n, A.w = w, A.K = K, A.tiles = (S + TS - 1) / TS, A.units = (int)units;
  const dim3 grid(8 * (unsigned)((units + 7) / 8)), block(kThreads);
  hipLaunchKernelGGL((match_topk_kernel<2, 8>), grid, block, 0, as_stream(stream), A);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_label_vote(const int* index, const float* score, int M, int K, int S, const float* labels, int Cl,
                              float inv_tau, int Kv, float* soft, int* label, float* confidence, int* source,
                              void* stream) {
  SKP_CHECK_ARG(index && score && labels && soft && label && confidence, "null pointer");
  SKP_CHECK_ARG(M >= 1 && K >= 1 && S >= 1 && Cl >= 1, "M, K, S and Cl must be at least 1");
  SKP_CHECK_ARG(M <= 64, "M > 64");
  SKP_CHECK_ARG(K <= KMAX, "K > 16");
  SKP_CHECK_ARG(Kv >= 1 && Kv <= K, "Kv must be in [1, K]");
  SKP_CHECK_ARG(Cl <= 256, "Cl > 256");
  SKP_CHECK_ARG(S <= 1024, "S > 1024");
  SKP_CHECK_ARG(inv_tau > 0.0f && inv_tau < INFINITY, "inv_tau must be positive and finite");
  VoteArgs A;
  A.index = index, A.score = score, A.labels = labels;
  A.soft = soft, A.confidence = confidence, A.label = label, A.source = source;
  A.M = M, A.K = K, A.Kv = Kv, A.Cl = Cl, A.plane = S * S, A.inv_tau = inv_tau;
  const dim3 grid((unsigned)((A.plane + kThreads - 1) / kThreads)), block(kThreads);
  hipLaunchKernelGGL(label_vote_kernel, grid, block, 0, as_stream(stream), A);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}
