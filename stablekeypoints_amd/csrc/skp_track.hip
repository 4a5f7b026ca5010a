// Keypoint tracks over a sequence of frames: one Viterbi step of a hidden Markov model over the pixel
// grid per token (skp_track_step) and the walk back along the stored back-pointers
// (skp_track_backtrace).  The emission is a frame's TTA average, the transition a truncated Gaussian
// random walk, and the max-product with a Gaussian is exactly separable: w[|dy|]·w[|dx|] is a product
// of one factor per axis, so the maximum over the (2r + 1)² window is a maximum over dx inside each
// row followed by a maximum over dy down each column, 2(2r + 1) products per pixel.
//
// Arithmetic (include/skp.h states it in full): every product and the division are fp32 and rounded
// on their own; there is no addition anywhere, so nothing can contract into an fma.  Each maximum
// walks its offsets in ascending order and takes a candidate with a strict >, so the smallest offset
// that attains it wins; only offsets whose pixel lies in the plane are candidates, so a back-pointer
// names a pixel of the plane whatever the values are (NaN never compares greater: the first
// candidate stays).
//
// Tile scheme: one 256-thread workgroup owns 32 × 32 pixels of one token's plane.
//   1. the tile of prev_score with its halo of r, (32 + 2r)², goes to LDS divided by prev_max (1.0f
//      everywhere where prev_max is 0 or not finite; 0 outside the plane, never a candidate);
//   2. the row stage: for each of the 32 + 2r rows and 32 columns the best (value, dx) to LDS;
//   3. the column stage from LDS: the best dy, and the dx stored at that row;
//   4. times avg; score and back are written a 128-byte row segment per half wave;
//   5. the workgroup leaves one (max, first row-major index) partial for its tile.
// The LDS arrays are sized by a compile-time cap on r (8, 16 or 32: 17, 27 and 52 KB), so a small
// radius does not pay for the largest one's footprint: at r = 32 three workgroups share a CU's
// 160 KB, at r <= 8 the wave slots bound the occupancy, not LDS.  The weights are a kernel argument
// (r + 1 floats by value) indexed by the loop counter, which is uniform: scalar loads.
// track_merge_kernel: one workgroup per token over its tiles' partials; (value, index) pairs are
// compared in full, so the result is the first row-major maximum whatever the order.  No atomics.
#include "skp_common.h"

using namespace skp;

namespace {

constexpr int TY = 32, TX = 32;      // pixels per workgroup tile
constexpr int kThreads = 256;
constexpr int kRows = kThreads / TX; // tile rows that one sweep of the workgroup covers
constexpr int kMaxR = 32;

struct Weights {
  float w[kMaxR + 1];
};

struct StepArgs {
  const float *avg, *prev, *prev_max;
  float* score;
  short* back;
  float* part_v;
  int* part_i;
  int S, r, xt, tiles;   // plane side, radius, tiles per row, tiles per plane
  Weights w;
};

long long r8(long long b) { return (b + 7) & ~7LL; }

// the workspace: one (max, index) partial per token and tile
struct Plan {
  int xt, tiles;
  long long part_v, part_i, bytes;
};

const char* plan(int n, int S, int r, Plan& L) {
  if (n < 1 || S < 1) return "n and S must be at least 1";
  if (S > 4096) return "S > 4096";
  if (n > 65535) return "n > 65535";
  if (r < 1 || r > kMaxR) return "r must be in [1, 32]";
  L.xt = (S + TX - 1) / TX;
  L.tiles = L.xt * ((S + TY - 1) / TY);
  L.part_v = 0;
  L.part_i = r8(4LL * n * L.tiles);
  L.bytes = 2 * L.part_i;
  if (L.bytes >= (1LL << 31)) return "workspace of 2^31 bytes or more";
  return nullptr;
}

// One stage's maximum for one output: the candidates c[d · stride] · w[|d|], d = −r … r ascending, the
// first one in the plane, then any strictly greater one.  EDGE: the window may leave the plane along
// this axis (pos + d outside [0, S) is no candidate); otherwise every d is one and nothing is tested.
template <bool EDGE>
__device__ __forceinline__ void stage_max(const float* c, int stride, int pos, int S, int r, const Weights& w, float& bv,
                                          int& bo) {
  if (EDGE) {
    bool have = false;
    bv = 0.0f, bo = 0;
    for (int d = -r; d <= r; ++d) {
      const float v = __fmul_rn(c[d * stride], w.w[d < 0 ? -d : d]);
      const bool in = (unsigned)(pos + d) < (unsigned)S;
      const bool take = in && (!have || v > bv);
      bv = take ? v : bv;
      bo = take ? d : bo;
      have = have || in;
    }
  } else {
    bv = __fmul_rn(c[-r * stride], w.w[r]), bo = -r;
    for (int d = -r + 1; d <= r; ++d) {
      const float v = __fmul_rn(c[d * stride], w.w[d < 0 ? -d : d]);
      const bool take = v > bv;
      bv = take ? v : bv;
      bo = take ? d : bo;
    }
  }
}

template <int RC>
__global__ __launch_bounds__(kThreads) void track_tile_kernel(const StepArgs A) {
  constexpr int H = TY + 2 * RC, W = TX + 2 * RC;
  __shared__ float s_m[H * W];           // prev_score / prev_max, tile and halo
  __shared__ float s_g[H * TX];          // the row stage's value
  __shared__ signed char s_dx[H * TX];   // and its dx
  __shared__ float s_rv[kThreads / 64];
  __shared__ int s_ri[kThreads / 64];
  const int S = A.S, r = A.r;
  const int tile = (int)blockIdx.x, j = (int)blockIdx.y;
  const int y0 = (tile / A.xt) * TY, x0 = (tile % A.xt) * TX;
  const int tx = (int)threadIdx.x % TX, ty = (int)threadIdx.x / TX;
  const int x = x0 + tx;
  const size_t plane = (size_t)j * S * S;
  const float* __restrict__ avg = A.avg + plane;
  float* __restrict__ score = A.score + plane;
  short* __restrict__ back = A.back + plane;
  const int side = 2 * r + 1;
  float mv = -INFINITY;   // this thread's best of the tile, rows ascending: a strict > keeps the first
  int mi = 0x7fffffff;

  if (A.prev == nullptr) {   // frame 0: the score is the emission, every back-pointer the centre
    for (int yy = ty; yy < TY; yy += kRows) {
      const int y = y0 + yy;
      if (y < S && x < S) {
        const int o = y * S + x;
        const float m = avg[o];
        score[o] = m;
        back[o] = (short)(r * side + r);
        if (argmax_better(m, o, mv, mi)) mv = m, mi = o;
      }
    }
  } else {
    const float* __restrict__ prev = A.prev + plane;
    const float M = A.prev_max[j];
    const bool live = M != 0.0f && fabsf(M) < INFINITY;   // a blank plane (or NaN): the track restarts
    const int hr = TY + 2 * r, wr = TX + 2 * r;
    // a tile whose window stays inside the plane along an axis tests no candidate of that axis
    const bool x_edge = x0 < r || x0 + TX + r > S, y_edge = y0 < r || y0 + TY + r > S;
    for (int row = ty; row < hr; row += kRows) {
      const int y = y0 - r + row;
      for (int col = tx; col < wr; col += TX) {
        const int xx = x0 - r + col;
        float v = 0.0f;
        if ((unsigned)y < (unsigned)S && (unsigned)xx < (unsigned)S)
          v = live ? __fdiv_rn(prev[(size_t)y * S + xx], M) : 1.0f;
        s_m[row * W + col] = v;
      }
    }
    __syncthreads();
    // row stage: g(y', x) = max over dx of m̃(y', x + dx) · w[|dx|], the smallest dx that attains it
    for (int row = ty; row < hr; row += kRows) {
      const float* m = s_m + row * W + tx + r;
      float bv;
      int bo;
      if (x_edge) stage_max<true>(m, 1, x, S, r, A.w, bv, bo);
      else stage_max<false>(m, 1, x, S, r, A.w, bv, bo);
      s_g[row * TX + tx] = bv;
      s_dx[row * TX + tx] = (signed char)bo;
    }
    __syncthreads();
    // column stage: h(y, x) = max over dy of g(y + dy, x) · w[|dy|], the smallest dy that attains it
    for (int yy = ty; yy < TY; yy += kRows) {
      const int y = y0 + yy;
      const float* g = s_g + (yy + r) * TX + tx;
      float bv;
      int bo;
      if (y_edge) stage_max<true>(g, TX, y, S, r, A.w, bv, bo);
      else stage_max<false>(g, TX, y, S, r, A.w, bv, bo);
      if (y < S && x < S) {
        const int dx = s_dx[(yy + r + bo) * TX + tx];
        const int o = y * S + x;
        const float m = __fmul_rn(avg[o], bv);
        score[o] = m;
        back[o] = (short)((bo + r) * side + (dx + r));
        if (argmax_better(m, o, mv, mi)) mv = m, mi = o;
      }
    }
  }
  block_argmax(mv, mi, s_rv, s_ri);
  if (threadIdx.x == 0) {
    const size_t o = (size_t)j * A.tiles + tile;
    A.part_v[o] = mv;
    A.part_i[o] = mi;
  }
}

// One workgroup per token: its tiles' partials -> (score_max, best).  Every tile holds a pixel of the
// plane, so best is one too.
__global__ __launch_bounds__(kThreads) void track_merge_kernel(const float* __restrict__ part_v,
                                                               const int* __restrict__ part_i, int tiles,
                                                               float* __restrict__ score_max, int* __restrict__ best) {
  __shared__ float s_rv[kThreads / 64];
  __shared__ int s_ri[kThreads / 64];
  const int j = (int)blockIdx.x;
  float mv = -INFINITY;
  int mi = 0x7fffffff;
  for (int t = (int)threadIdx.x; t < tiles; t += kThreads) {
    const float v = part_v[(size_t)j * tiles + t];
    const int i = part_i[(size_t)j * tiles + t];
    if (argmax_better(v, i, mv, mi)) mv = v, mi = i;
  }
  block_argmax(mv, mi, s_rv, s_ri);
  if (threadIdx.x == 0) {
    score_max[j] = mv;
    best[j] = mi;
  }
}

// One thread per token walks the T dependent loads.  A code or an index that the step kernel cannot
// have written (a caller's own buffer) is clamped, so no load leaves the plane.
__global__ __launch_bounds__(kThreads) void track_backtrace_kernel(const short* __restrict__ back,
                                                                   const int* __restrict__ best_last, int T, int n,
                                                                   int S, int r, float* __restrict__ pos) {
  const int j = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (j >= n) return;
  const int side = 2 * r + 1;
  const int p = min(max(best_last[j], 0), S * S - 1);
  int y = p / S, x = p % S;
  for (int t = T - 1; t >= 0; --t) {
    float* o = pos + ((size_t)t * n + j) * 2;
    o[0] = (float)y + 0.5f;
    o[1] = (float)x + 0.5f;
    if (t > 0) {
      const int code = min(max((int)back[((size_t)t * n + j) * S * S + (size_t)y * S + x], 0), side * side - 1);
      y = min(max(y + code / side - r, 0), S - 1);
      x = min(max(x + code % side - r, 0), S - 1);
    }
  }
}

template <class T>
T* at(void* workspace, long long offset) {
  return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset);
}

}  // namespace

extern "C" int skp_track_step_workspace(int n, int S, int r) {
  Plan L;
  return plan(n, S, r, L) ? -1 : (int)L.bytes;
}

extern "C" int skp_track_step(const float* avg, const float* prev_score, const float* prev_max, int n, int S,
                              const float* w_host, int r, float* score, float* score_max, int* best, short* back,
                              void* workspace, void* stream) {
  SKP_CHECK_ARG(avg && w_host && score && score_max && best && back && workspace, "null pointer");
  SKP_CHECK_ARG((prev_score == nullptr) == (prev_max == nullptr),
                "prev_score and prev_max must be null together (frame 0) or both given");
  Plan L;
  const char* bad = plan(n, S, r, L);
  SKP_CHECK_ARG(!bad, bad);
  SKP_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "workspace must be 8-byte aligned");
  StepArgs A;
  for (int k = 0; k <= kMaxR; ++k) A.w.w[k] = 0.0f;
  for (int k = 0; k <= r; ++k) {
    SKP_CHECK_ARG(w_host[k] > 0.0f && w_host[k] <= 1.0f, "every weight must be finite and in (0, 1]");
    A.w.w[k] = w_host[k];
  }
  A.avg = avg, A.prev = prev_score, A.prev_max = prev_max, A.score = score, A.back = back;
  A.part_v = at<float>(workspace, L.part_v), A.part_i = at<int>(workspace, L.part_i);
  A.S = S, A.r = r, A.xt = L.xt, A.tiles = L.tiles;
  hipStream_t st = as_stream(stream);
  const dim3 grid(L.tiles, n);
  if (r <= 8) hipLaunchKernelGGL(track_tile_kernel<8>, grid, dim3(kThreads), 0, st, A);
  else if (r <= 16) hipLaunchKernelGGL(track_tile_kernel<16>, grid, dim3(kThreads), 0, st, A);
  else hipLaunchKernelGGL(track_tile_kernel<32>, grid, dim3(kThreads), 0, st, A);
  hipLaunchKernelGGL(track_merge_kernel, dim3(n), dim3(kThreads), 0, st, A.part_v, A.part_i, L.tiles, score_max, best);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_track_backtrace(const short* back, const int* best_last, int T, int n, int S, int r, float* pos,
                                   void* stream) {
  SKP_CHECK_ARG(back && best_last && pos, "null pointer");
  SKP_CHECK_ARG(T >= 1 && n >= 1 && S >= 1, "T, n and S must be at least 1");
  SKP_CHECK_ARG(S <= 4096, "S > 4096");
  SKP_CHECK_ARG(r >= 1 && r <= kMaxR, "r must be in [1, 32]");
  hipLaunchKernelGGL(track_backtrace_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream),
                     back, best_last, T, n, S, r, pos);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}
