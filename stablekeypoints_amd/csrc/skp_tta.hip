// A18: the test-time-augmentation reduce — the inverse warps, the two sums over the copies, the
// ratio, the NaN fix and the argmax of eval.run_image_with_context_augmented in one pass, for gfx950.
//
// Reference: eval.py:327-355 (sum_samples += inverse(maps), num_samples += inverse(ones),
// attention_maps = sum / num, NaN -> 0) and eval.py:39-60 (find_max_pixel: first-occurrence
// row-major argmax, position = (row + 0.5, col + 0.5)).  The reference holds the full-size average
// only to read its argmax; here every captured map is read once and the keypoints leave directly
// (the average is written only on request).
//
// Arithmetic is the sequential composition's, bit for bit: grid_point and sample_ones of skp_warp.h,
// its sample() restated on paired loads (sample_taps: the same products and sums, unfused), both
// sums from 0.0f in copy order with __fadd_rn, __fdiv_rn, NaN -> 0 before the argmax.
//
// Two launches, no atomics: the tile kernel (one workgroup per image and 64 x 4-pixel piece of a
// four-row band) leaves one (value, linear index) partial per token and tile; the merge kernel
// (tta_merge_kernel, the one merge of all three reduces) reduces each (image, token)'s partials
// (the greater value wins, on equal values the lower index).
//
// The scored reduce (skp_tta_reduce_scored) adds, without the average in memory: the tile kernel's
// scored instantiation leaves the sum of each tile's averaged values beside its partial (double
// from the lane upward, a fixed tree), the merge's kScored instantiation sums them in a fixed order
// and leaves the peak's value and index, and a third launch (one workgroup per image and token)
// recomputes the average on the box around the peak with the same functions, hence the same bits,
// for the centroid of eval.py:113-155, the concentration and the coverage.  Three launches, no
// atomics.
//
// The k-peak reduce (skp_tta_reduce_peaks) adds eval.find_k_max_pixels (eval.py:62-111) on that
// average, again without it in memory: round 0 is the tile kernel and the merge, which also leaves
// the winning index and value; the masks are cumulative, so in round j only the tiles that meet the
// bounding box of the newest disc (pick j − 1) can change, and a masked-tile kernel recomputes
// those (average_at: the tile kernel's bits), applies all j masks (the predicate and the multiply
// of row_argmax_masked, skp_select.hip) and overwrites their partials in place; then the merge
// again.  2 + 2(num − 1) launches, no atomics.
//
// The entropy reduce (skp_tta_reduce_entropy) adds the Shannon entropy of softmax(scale · average)
// over the plane (eval.find_corresponding_points, eval.py:159-195, ranks tokens by it), again without
// the average in memory.  One pass: H = log S0 − T / S0 with S0 = Σ e^{z−m} and T = Σ (z−m)·e^{z−m},
// z = scale · a, about a maximum m.  A wave sums about its own maximum; the tile kernel's entropy
// instantiation combines its four waves about the tile's maximum and leaves (S0, T) beside the
// partial, and the merge's kEntropy instantiation combines the tiles about the plane's maximum
// (entropy_add: a partial about m_k enters sums about m >= m_k scaled by e^{scale·(m_k−m)}).  All in
// double, every order fixed: lanes in the wave tree, waves in wave order, tiles k, k + 64, … per
// lane and then the wave tree.  Its grid has a third dimension over chunks of kTok tokens: the
// selection reduces every token of an embedding (n = 500 at S = 128 is 64 tiles per image).  Two
// launches, no atomics.
//
// The part reduce (skp_tta_reduce_parts) reduces over the token axis instead: at every pixel the
// greatest of the tokens' averages, the lowest token that attains it, and the tokens' sum.  A thread
// owns its pixel, so the three ride along in registers through its chunk's passes (Carry) and leave
// as 10 bytes per pixel.  The grid has the entropy reduce's third dimension over chunks of kTok
// tokens; with one chunk the threads write the outputs, with more they write one partial per (image,
// chunk, pixel) and a per-pixel merge walks the chunks in order (strict >, so the earlier chunk
// keeps a tie; the masses added in chunk order).  The mass is defined in that order, each chunk's
// sum from 0.0f in token order and the chunks' sums from 0.0f in chunk order, so that the chunks can
// run in different workgroups and give the same bits.  Two or three launches, no atomics.
//
// The match reduce (skp_tta_reduce_match) combines across the tokens with the caller's weights: at
// every pixel the n averages are a signature, and for each of Q <= 16 query signatures the cosine
// score dot / sqrt(nrm) with nrm = Σ_t a_t² and dot = Σ_t a_t·d[t], then the first row-major maximum
// of each query's scores over the plane.  A thread owns its pixel, so nrm and the Q dots ride along
// in registers through its chunk's passes (MatchCarry), the chunk's rows of the queries staged in
// LDS.  The sums have the part reduce's mass order (each chunk from 0.0f in token order, the chunks
// from 0.0f in chunk order, every product and sum rounded on its own).  With one chunk the tile
// kernel forms the scores and leaves one (value, index) partial per (image, query, tile); with more
// the threads store Q + 1 floats per (image, chunk, pixel) and a per-pixel merge walks the chunks in
// order, forms the scores and leaves one partial per (image, query, 64 pixels).  tta_merge_kernel
// reduces those as it reduces the tokens' partials.  Three or four launches, no atomics.
//
// Host side: layout() is the one statement of the workspace (the queries return its size, the entry
// points take their pointers from its offsets), check_common() the checks the entry points
// share, launch_tile() the tile kernel's launch.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "skp_warp.h"

using namespace skp;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE;
// Tokens per pass over a pixel's copies: the pixel's C grid records (theta is wave-uniform, the
// record depends on pixel and copy only) are formed once per pass and serve all its tokens; the
// sums stay in registers.  10 = the pipeline's top_k, so its maps take one pass.
constexpr int kTok = 10;
static_assert(kTok <= 15, "the rest after the kTok passes is split into passes of 8, 4, 2 and 1");
constexpr int kNoIndex = 0x7fffffff;
constexpr int kMaxPeaks = 16;   // kMaxSubjects of skp_select.hip

__device__ __forceinline__ bool better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// In-wave argmax of NaN-free values: the maximum through the DPP reduction, then the lowest index
// among the lanes that hold it.  Every lane ends with the result.
__device__ __forceinline__ void wave_best(float& v, int& i) {
  const float m = wave_max(v);
  int c = v == m ? i : kNoIndex;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c = min(c, __shfl_xor(c, o, 64));
  v = m;
  i = c;
}

// Full-wave double sum in wave_reduce's tree (skp_common.h): the same DPP controls and row swaps on
// the two halves of the value, so a step costs VALU moves and no LDS crossbar.  Every lane ends
// with the same bits, and two runs give the same bits.  Needs all 64 lanes active.
template <int CTRL>
__device__ __forceinline__ double dpp_read(double v) {
  const long long q = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)q, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(q >> 32), CTRL, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_sum_tree(double v) {
  v += dpp_read<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_read<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_read<0x141>(v);   // row_half_mirror
  v += dpp_read<0x140>(v);   // row_mirror
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long long q = __builtin_bit_cast(long long, v);
    int lo = (int)q, hi = (int)(q >> 32), wlo = lo, whi = hi;
    if (s == 0) {
      asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(lo), "+v"(wlo));
      asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(hi), "+v"(whi));
    } else {
      asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(lo), "+v"(wlo));
      asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(hi), "+v"(whi));
    }
    v = __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo) +
        __builtin_bit_cast(double, ((long long)whi << 32) | (unsigned)wlo);
  }
  return v;
}

// A workgroup takes a tile of kTileW x kTileH pixels, one pixel per thread, each wave a 16 x 4
// block of it: a rotated copy's taps of a 16 x 4 block fall on about 4-12 source rows, those of 64
// pixels of one row on up to 32, and every source row a wave instruction touches is a cache line
// of its own.
constexpr int kTileW = 64, kTileH = 4;
__host__ __device__ inline int tiles_x(int S) { return (S + kTileW - 1) / kTileW; }
__host__ __device__ inline int tiles_y(int S) { return (S + kTileH - 1) / kTileH; }
// This thread's pixel of tile (tx, ty).
__device__ __forceinline__ void tile_pixel(int tx, int ty, int& x, int& y) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  x = tx * kTileW + wid * 16 + (lane & 15);
  y = ty * kTileH + (lane >> 4);
}

// The plane's pixel of linear index `index` (0 where it is none: the callers' indices come from
// partials, and every tile holds a pixel, so it is one; the loads around it rely on that) and the
// box of rows r0 ± R and columns c0 ± R around it, clipped to the plane.
struct Box {
  int r0, c0, ylo, yhi, xlo, xhi;
};
__device__ __forceinline__ Box clipped_box(int index, int S, int R) {
  index = (unsigned)index < (unsigned)(S * S) ? index : 0;
  Box b;
  b.r0 = index / S, b.c0 = index % S;
  b.ylo = max(b.r0 - R, 0), b.yhi = min(b.r0 + R, S - 1);
  b.xlo = max(b.c0 - R, 0), b.xhi = min(b.c0 + R, S - 1);
  return b;
}

// A grid record ready for many planes.  The two taps of a row are neighbours in memory, so each
// row goes as ONE 8-byte load at a column clamped into [0, S − 2] (every load lands inside the
// plane and needs no branch, so all of a pass's 2·NT loads are in flight together; the tile kernel
// is bound by the number of gather instructions, not by bytes).  `swap`: the clamp moved the pair
// by one column (x0 = −1 or S − 1), so the tap that is in range sits in the other half.  S >= 2.
struct Taps {
  int off[2];     // north and south row: offset of the pair
  bool swap;
  bool ok[4];     // the tap counts (is inside the plane)
  float w[4];
};
struct __attribute__((packed, aligned(4))) Pair {
  float a, b;
};
__device__ __forceinline__ Taps taps_of(const Bilin& b, int S) {
  Taps t;
  const int xb = max(min(b.x0, S - 2), 0);
  t.swap = xb != b.x0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = b.x0 + (k & 1), yy = b.y0 + (k >> 1);
    t.ok[k] = xx >= 0 && xx < S && yy >= 0 && yy < S;
    t.w[k] = b.w[k];
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) t.off[r] = min(max(b.y0 + r, 0), S - 1) * S + xb;
  return t;
}
// sample() of skp_warp.h on a Taps record and its two loaded pairs: ((v_nw·nw + v_ne·ne) + v_sw·sw)
// + v_se·se with every product and sum rounded on its own.  __fmul_rn / __fadd_rn are plain * and +
// to the compiler, which may contract them (it does not in skp_affine_warp's kernel, and did here),
// so the products and sums stand under contract(off).
__device__ __forceinline__ float sample_taps(const Pair (&raw)[2], const Taps& t) {
#pragma clang fp contract(off)
  float out = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const Pair& r = raw[k >> 1];
    const float at = (k & 1) ? (t.swap ? r.a : r.b) : (t.swap ? r.b : r.a);
    const float v = t.ok[k] ? at : 0.0f;
    const float prod = v * t.w[k];
    out = k == 0 ? prod : out + prod;
  }
  return out;
}

struct TileArgs {
  const float* maps;        // (B, C, n, S, S)
  const float* theta_inv;   // (B, C, 2, 3)
  float* avg;               // (B, n, S, S) or null
  float* part_v;            // (B, n, tiles)
  int* part_i;
  int C, n, S;
};
struct ScoredTileArgs : TileArgs {
  double* part_m;           // (B, n, tiles): the sum of the tile's averaged values
};
template <bool SCORED>
using TileArgsOf = std::conditional_t<SCORED, ScoredTileArgs, TileArgs>;
struct EntropyTileArgs : TileArgs {
  double* part_s0;          // (B, n, tiles): Σ e^{z−m} and Σ (z−m)·e^{z−m} over the tile, z = scale · a,
  double* part_t;           // m = scale · the tile's maximum (part_v)
  float scale;
};
struct PartsTileArgs : TileArgs {
  float* out_v;             // (B, chunks, S, S): the chunk's greatest average of the pixel,
  short* out_l;             // the lowest token of the chunk that attains it,
  float* out_m;             // and the chunk's sum (the outputs themselves where chunks == 1)
};
constexpr int kMaxQueries = 16;
struct MatchTileArgs : TileArgs {
  const float* queries;     // (Q, n)
  float* chunk;             // (B, chunks, Q + 1, S, S): the chunk's nrm, then its Q dots (chunks > 1)
  float* score_map;         // (B, Q, S, S) or null      (chunks == 1: the tile kernel finishes the scores
  float* qpart_v;           // (B, Q, tiles)              and leaves each query's partial of the tile)
  int* qpart_i;
  int Q;
};
// The match reduce's tile kernel is instantiated on a bucket of queries (4, 8 or 16 accumulators).
enum Tile { kTilePlain, kTileScored, kTileEntropy, kTileParts, kTileMatch4, kTileMatch8, kTileMatch16 };
constexpr int match_width(Tile K) { return K == kTileMatch4 ? 4 : K == kTileMatch8 ? 8 : K == kTileMatch16 ? 16 : 0; }
template <Tile K>
using ArgsOfTile = std::conditional_t<
    match_width(K) != 0, MatchTileArgs,
    std::conditional_t<K == kTileParts, PartsTileArgs,
                       std::conditional_t<K == kTileEntropy, EntropyTileArgs, TileArgsOf<K == kTileScored>>>>;

// What a thread of the part reduce carries through its chunk's passes: the greatest average so far
// of its pixel, the lowest token that attains it and the sum so far.  A thread of the match reduce
// carries its pixel's Σ a² and the QB dots so far; `rows` is the chunk's slice of the queries in LDS,
// (kTok, QB) with zeros past Q.  The other reduces carry nothing.
struct NoCarry {};
struct Carry {
  float v, mass;
  int tok;
};
template <int QB>
struct MatchCarry {
  float nrm, dot[QB > 0 ? QB : 1];
  const float4* rows;
};
template <Tile K>
using CarryOf = std::conditional_t<match_width(K) != 0, MatchCarry<match_width(K)>,
                                   std::conditional_t<K == kTileParts, Carry, NoCarry>>;
// Token `tok`'s average `a` enters the carry: strict >, so the earlier token keeps a tie (a holds no
// NaN: a total order); the add rounded on its own.
__device__ __forceinline__ void carry_take(Carry& c, float a, int tok) {
#pragma clang fp contract(off)
  if (a > c.v) {
    c.v = a;
    c.tok = tok;
  }
  c.mass = c.mass + a;
}
// The average `a` of the chunk's token `local` enters the match carry: nrm + a·a and, per query,
// dot + a·d, every product and sum rounded on its own.  Four queries' weights come as one LDS read at
// a wave-uniform address; a group of four past Q is skipped (uniform).
template <int QB>
__device__ __forceinline__ void match_take(MatchCarry<QB>& c, float a, int local, int Q) {
#pragma clang fp contract(off)
  const float sq = a * a;
  c.nrm = c.nrm + sq;
#pragma unroll
  for (int g = 0; g < QB / 4; ++g)
    if (4 * g < Q) {
      const float4 d = c.rows[local * (QB / 4) + g];
      const float p0 = a * d.x, p1 = a * d.y, p2 = a * d.z, p3 = a * d.w;
      c.dot[4 * g] = c.dot[4 * g] + p0;
      c.dot[4 * g + 1] = c.dot[4 * g + 1] + p1;
      c.dot[4 * g + 2] = c.dot[4 * g + 2] + p2;
      c.dot[4 * g + 3] = c.dot[4 * g + 3] + p3;
    }
}
// The cosine score of a pixel: dot / sqrt(nrm), both correctly rounded (sqrt_rn: __fsqrt_rn is the
// native approximation in this build); −inf where nrm is not > 0 and where the quotient is NaN.
__device__ __forceinline__ float match_score(float dot, float nrm) {
  const float s = __fdiv_rn(dot, sqrt_rn(nrm));
  return (nrm > 0.0f && s == s) ? s : -INFINITY;
}

// Sums (s0, t) about the maximum m take in a partial (sk, tk) about mk <= m:
// Σ (z−m)·e^{z−m} = e^d · (Σ (z−mk)·e^{z−mk} + d · Σ e^{z−mk}) with d = scale · (mk − m) <= 0.  A
// partial with no pixel above −inf (mk = −inf: sk = tk = 0) and one that e^d takes to 0 add nothing,
// which is the limit; mk = m = +inf gives d = NaN and NaN sums.
__device__ __forceinline__ void entropy_add(double& s0, double& t, float mk, double sk, double tk, float m,
                                            float scale) {
  if (!(mk > -INFINITY)) return;
  const double d = (double)scale * ((double)mk - (double)m);
  const double r = exp(d);
  if (r == 0.0) return;
  s0 += sk * r;
  t += (tk + d * sk) * r;
}

// Tokens t0 … t0 + NT − 1 of this thread's pixel: one pass over the copies, the sums in registers.
// SCORED: each token's averaged value also goes, as it is produced, into the tile's mass: lane
// value (0 outside the plane) -> wave tree -> the four waves in order, all in double.
// kTileEntropy: once the pass's averages exist, token by token: each lane's e = exp(z − m) about its
// wave's maximum (the double exp; a pixel outside the plane or at −inf has e = 0, and e = 0 adds 0
// to T), S0 and T through the wave tree into s_m[j] and s_m[kTok + j], then the four waves in order
// about the tile's maximum.
// kTileParts, kTileMatch*: each token's averaged value also enters the thread's carry, in token order.
template <int NT, Tile K>
__device__ __forceinline__ void tile_pass(const ArgsOfTile<K>& A, int t0, int b, int x, int y, bool inside, int p,
                                          float (*s_v)[kWaves], int (*s_i)[kWaves], double (*s_m)[kWaves],
                                          [[maybe_unused]] CarryOf<K>& carry) {
  const int S = A.S, SS = S * S;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float bv[NT];
  int bi[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    bv[j] = -INFINITY;
    bi[j] = kNoIndex;
  }
  if (inside) {
    const float* th = A.theta_inv + (size_t)b * A.C * 6;
    float sum[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) sum[j] = 0.0f;
    float num = 0.0f;
    for (int c = 0; c < A.C; ++c) {
      const Bilin g = grid_point(th + 6 * c, y, x, S, S);
      num = __fadd_rn(num, sample_ones(g, S, S));
      const Taps t = taps_of(g, S);
      const float* plane = A.maps + (((size_t)b * A.C + c) * A.n + t0) * SS;
      Pair raw[NT][2];   // every load of the pass before the first use
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 2; ++r) raw[j][r] = *reinterpret_cast<const Pair*>(plane + (size_t)j * SS + t.off[r]);
#pragma unroll
      for (int j = 0; j < NT; ++j) sum[j] = __fadd_rn(sum[j], sample_taps(raw[j], t));
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      float a = __fdiv_rn(sum[j], num);
      a = a != a ? 0.0f : a;
      if (A.avg) A.avg[((size_t)b * A.n + t0 + j) * SS + p] = a;
      if constexpr (K == kTileParts) carry_take(carry, a, t0 + j);
      if constexpr (match_width(K) != 0) match_take(carry, a, t0 + j - (int)blockIdx.z * kTok, A.Q);
      bv[j] = a;
      bi[j] = p;
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if constexpr (K == kTileScored) {
      const double m = wave_sum_tree(inside ? (double)bv[j] : 0.0);
      if (lane == 0) s_m[j][wid] = m;
    }
    const float a = bv[j];
    wave_best(bv[j], bi[j]);
    if (lane == 0) {
      s_v[j][wid] = bv[j];
      s_i[j][wid] = bi[j];
    }
    if constexpr (K == kTileEntropy) {
      double e = 0.0, t = 0.0;
      if (a > -INFINITY) {
        const double d = (double)A.scale * ((double)a - (double)bv[j]);
        e = exp(d);
        t = e == 0.0 ? 0.0 : d * e;
      }
      e = wave_sum_tree(e);
      t = wave_sum_tree(t);
      if (lane == 0) {
        s_m[j][wid] = e;
        s_m[kTok + j][wid] = t;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < NT) {
    const int j = threadIdx.x;
    float v = s_v[j][0];
    int i = s_i[j][0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k)
      if (better(s_v[j][k], s_i[j][k], v, i)) {
        v = s_v[j][k];
        i = s_i[j][k];
      }
    const size_t o = ((size_t)b * A.n + t0 + j) * gridDim.x + blockIdx.x;
    A.part_v[o] = v;
    A.part_i[o] = i;
    if constexpr (K == kTileScored) {
      double m = s_m[j][0];
#pragma unroll
      for (int k = 1; k < kWaves; ++k) m += s_m[j][k];
      A.part_m[o] = m;
    }
    if constexpr (K == kTileEntropy) {
      double s0 = 0.0, t = 0.0;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) entropy_add(s0, t, s_v[j][k], s_m[j][k], s_m[kTok + j][k], v, A.scale);
      A.part_s0[o] = s0;
      A.part_t[o] = t;
    }
  }
  __syncthreads();
}

// Tokens t0 … t1 − 1 of this thread's pixel: in passes of kTok, the rest in passes of 8, 4, 2, 1
// (compile-time counts: no branch between a pass's loads).
template <Tile K>
__device__ __forceinline__ void tile_tokens(const ArgsOfTile<K>& A, int t0, int t1, int b, int x, int y, bool inside,
                                            int p, float (*s_v)[kWaves], int (*s_i)[kWaves], double (*s_m)[kWaves],
                                            CarryOf<K>& carry) {
  for (; t0 + kTok <= t1; t0 += kTok) tile_pass<kTok, K>(A, t0, b, x, y, inside, p, s_v, s_i, s_m, carry);
  const int rest = t1 - t0;   // < kTok <= 15
  if (rest & 8) {
    tile_pass<8, K>(A, t0, b, x, y, inside, p, s_v, s_i, s_m, carry);
    t0 += 8;
  }
  if (rest & 4) {
    tile_pass<4, K>(A, t0, b, x, y, inside, p, s_v, s_i, s_m, carry);
    t0 += 4;
  }
  if (rest & 2) {
    tile_pass<2, K>(A, t0, b, x, y, inside, p, s_v, s_i, s_m, carry);
    t0 += 2;
  }
  if (rest & 1) tile_pass<1, K>(A, t0, b, x, y, inside, p, s_v, s_i, s_m, carry);
}

// grid (tiles_x · tiles_y, B), every token in turn (tile_tokens).  Four waves per SIMD are asked for, not
// eight: a pass holds 4·kTok loaded values, and one image of 512² is four waves per SIMD anyway.
template <bool SCORED>
__global__ __launch_bounds__(kThreads, 4) void tta_tile_kernel(const TileArgsOf<SCORED> A) {
  __shared__ float s_v[kTok][kWaves];
  __shared__ int s_i[kTok][kWaves];
  __shared__ double s_m[SCORED ? kTok : 1][kWaves];
  const int b = blockIdx.y, tile = blockIdx.x, S = A.S;
  int x, y;
  tile_pixel(tile % tiles_x(S), tile / tiles_x(S), x, y);
  const bool inside = x < S && y < S;
  const int p = inside ? y * S + x : 0;
  NoCarry none;
  tile_tokens<SCORED ? kTileScored : kTilePlain>(A, 0, A.n, b, x, y, inside, p, s_v, s_i, s_m, none);
}

// The entropy reduce's tile kernel: grid (tiles_x · tiles_y, B, ⌈n / kTok⌉), workgroup z takes the
// tokens of chunk z, so that a selection over a whole embedding (n = 500, S = 128: 64 tiles per
// image) fills the device.  The partial of (image, token, tile) is where the other reduces have it.
__global__ __launch_bounds__(kThreads, 4) void tta_tile_entropy_kernel(const EntropyTileArgs A) {
  __shared__ float s_v[kTok][kWaves];
  __shared__ int s_i[kTok][kWaves];
  __shared__ double s_m[2 * kTok][kWaves];
  const int b = blockIdx.y, tile = blockIdx.x, S = A.S;
  int x, y;
  tile_pixel(tile % tiles_x(S), tile / tiles_x(S), x, y);
  const bool inside = x < S && y < S;
  const int p = inside ? y * S + x : 0;
  const int t0 = blockIdx.z * kTok;
  NoCarry none;
  tile_tokens<kTileEntropy>(A, t0, min(t0 + kTok, A.n), b, x, y, inside, p, s_v, s_i, s_m, none);
}

// The part reduce's tile kernel: the entropy reduce's grid (tiles_x · tiles_y, B, ⌈n / kTok⌉).  Each
// thread carries its pixel's (greatest average, lowest token that attains it, sum) through the
// passes of chunk z, a full pass of kTok or the sub-passes of 8, 4, 2 and 1 of a shorter last chunk,
// and stores them at (image, chunk, pixel): the outputs where there is one chunk, else the partials
// of tta_parts_merge_kernel.  A chunk whose averages are all −inf keeps its first token.
__global__ __launch_bounds__(kThreads, 4) void tta_tile_parts_kernel(const PartsTileArgs A) {
  __shared__ float s_v[kTok][kWaves];
  __shared__ int s_i[kTok][kWaves];
  __shared__ double s_m[1][kWaves];
  const int b = blockIdx.y, tile = blockIdx.x, S = A.S;
  int x, y;
  tile_pixel(tile % tiles_x(S), tile / tiles_x(S), x, y);
  const bool inside = x < S && y < S;
  const int p = inside ? y * S + x : 0;
  const int t0 = blockIdx.z * kTok;
  Carry carry = {-INFINITY, 0.0f, t0};
  tile_tokens<kTileParts>(A, t0, min(t0 + kTok, A.n), b, x, y, inside, p, s_v, s_i, s_m, carry);
  if (inside) {
    const size_t o = ((size_t)b * gridDim.z + blockIdx.z) * ((size_t)S * S) + p;
    A.out_v[o] = carry.v;
    A.out_l[o] = (short)carry.tok;
    A.out_m[o] = carry.mass;
  }
}

// The part reduce's merge over the chunks, one thread per pixel, grid (⌈S² / 64⌉, B): the chunks in
// order, strict > (the earlier chunk keeps a tie, and chunk 0's first token an all −inf pixel), the
// masses added from 0.0f in chunk order.  A thread's loads depend on nothing it computes, so kAhead
// chunks' values and masses are in flight together; the label is read once, from the chunk that won.
// One wave per workgroup: at 128² that is 256 workgroups and not 64.  Measured for 50 chunks of 128²:
// 6.4 µs, against 34.9 µs for a load per step in workgroups of 256, which was all latency.
__global__ __launch_bounds__(WAVE) void tta_parts_merge_kernel(const float* __restrict__ part_v,
                                                               const short* __restrict__ part_l,
                                                               const float* __restrict__ part_m, int chunks, int SS,
                                                               float* __restrict__ value, short* __restrict__ label,
                                                               float* __restrict__ mass) {
  constexpr int kAhead = 8;
  const int p = blockIdx.x * WAVE + threadIdx.x;
  if (p >= SS) return;
  const size_t o = (size_t)blockIdx.y * chunks * SS + p;
  float v = -INFINITY, m = 0.0f;
  int best = 0;
  for (int k0 = 0; k0 < chunks; k0 += kAhead) {
    float pv[kAhead], pm[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const size_t q = o + (size_t)min(k0 + u, chunks - 1) * SS;   // past the last chunk: the last one again, not used
      pv[u] = part_v[q];
      pm[u] = part_m[q];
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
      if (k0 + u < chunks) {
        if (pv[u] > v) {
          v = pv[u];
          best = k0 + u;
        }
        m = __fadd_rn(m, pm[u]);
      }
  }
  const size_t d = (size_t)blockIdx.y * SS + p;
  value[d] = v;
  label[d] = part_l[o + (size_t)best * SS];
  mass[d] = m;
}

// The match reduce's tile kernel: the entropy reduce's grid (tiles_x · tiles_y, B, ⌈n / kTok⌉).  The
// workgroup stages its chunk's rows of the queries in LDS, (kTok, QB) with zeros past Q and past the
// chunk's last token; each thread carries its pixel's nrm and dots through the chunk's passes.  With
// more than one chunk it stores them at (image, chunk, component, pixel) for tta_match_merge_kernel.
// With one chunk (SINGLE; two instantiations, so that neither holds the other's pointers in SGPRs:
// together they left a spill slot in the Q = 16 kernel's frame) it forms the Q scores itself, writes them where the score map is
// asked for, and the workgroup leaves each query's best (score, pixel) of the tile: wave_best, then
// the four waves as tile_pass combines them.  A thread outside the plane enters with (−inf, no index).
template <int QB, bool SINGLE>
__global__ __launch_bounds__(kThreads, 4) void tta_tile_match_kernel(const MatchTileArgs A) {
  constexpr Tile K = QB == 4 ? kTileMatch4 : QB == 8 ? kTileMatch8 : kTileMatch16;
  __shared__ float s_v[kTok][kWaves];
  __shared__ int s_i[kTok][kWaves];
  __shared__ double s_m[1][kWaves];
  __shared__ float4 s_rows[kTok * (QB / 4)];
  __shared__ float s_qv[QB][kWaves];
  __shared__ int s_qi[QB][kWaves];
  static_assert(kTok * QB <= kThreads, "one thread stages one weight");
  const int b = blockIdx.y, tile = blockIdx.x, S = A.S, SS = S * S, Q = A.Q;
  int x, y;
  tile_pixel(tile % tiles_x(S), tile / tiles_x(S), x, y);
  const bool inside = x < S && y < S;
  const int p = inside ? y * S + x : 0;
  const int t0 = blockIdx.z * kTok, t1 = min(t0 + kTok, A.n);
  if (threadIdx.x < kTok * QB) {
    const int j = threadIdx.x / QB, q = threadIdx.x % QB;
    reinterpret_cast<float*>(s_rows)[threadIdx.x] = (q < Q && t0 + j < t1) ? A.queries[(size_t)q * A.n + t0 + j] : 0.0f;
  }
  __syncthreads();
  MatchCarry<QB> carry;
  carry.nrm = 0.0f;
#pragma unroll
  for (int q = 0; q < QB; ++q) carry.dot[q] = 0.0f;
  carry.rows = s_rows;
  tile_tokens<K>(A, t0, t1, b, x, y, inside, p, s_v, s_i, s_m, carry);
  if constexpr (!SINGLE) {
    if (inside) {
      float* out = A.chunk + ((size_t)b * gridDim.z + blockIdx.z) * (Q + 1) * SS + p;
      out[0] = carry.nrm;
#pragma unroll
      for (int q = 0; q < QB; ++q)
        if (q < Q) out[(size_t)(q + 1) * SS] = carry.dot[q];
    }
    return;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < QB; ++q)
    if (q < Q) {   // uniform
      float v = inside ? match_score(carry.dot[q], carry.nrm) : -INFINITY;
      int i = inside ? p : kNoIndex;
      if (A.score_map && inside) A.score_map[((size_t)b * Q + q) * SS + p] = v;
      wave_best(v, i);
      if (lane == 0) {
        s_qv[q][wid] = v;
        s_qi[q][wid] = i;
      }
    }
  __syncthreads();
  if (threadIdx.x < Q) {
    const int q = threadIdx.x;
    float v = s_qv[q][0];
    int i = s_qi[q][0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k)
      if (better(s_qv[q][k], s_qi[q][k], v, i)) {
        v = s_qv[q][k];
        i = s_qi[q][k];
      }
    const size_t o = ((size_t)b * Q + q) * gridDim.x + blockIdx.x;
    A.qpart_v[o] = v;
    A.qpart_i[o] = i;
  }
}

// The match reduce's merge over the chunks, grid (⌈S² / 64⌉, B, ⌈Q / 4⌉), one wave per workgroup as
// tta_parts_merge_kernel: wave z takes its 64 pixels' nrm and the dots of queries 4z … 4z + 3, added
// from 0.0f in chunk order, kAhead chunks' five values in flight together; then those queries'
// scores, written where the score map is asked for, and each one's best (score, pixel) of the 64
// pixels.  The waves of a pixel block each add nrm themselves, in the same order, hence to the same
// bits: at Q = 16 that is 3/17 more loads for four times the waves and a quarter of the steps.  It
// first took all Q + 1 values per wave, two chunks in flight: 38.2 µs for 50 chunks of 128² at
// Q = 16, where the bytes are 9 µs.  Every lane stays to the end (wave_best needs the full wave): a
// lane past the plane loads the last pixel's values and enters with (−inf, no index); a query past Q
// loads the last query's and is not used.
__global__ __launch_bounds__(WAVE) void tta_match_merge_kernel(const float* __restrict__ chunk, int chunks, int SS, int Q,
                                                               float* __restrict__ score_map,
                                                               float* __restrict__ qpart_v, int* __restrict__ qpart_i) {
  constexpr int kAhead = 8, kGroup = 4;
  const int p = blockIdx.x * WAVE + threadIdx.x, b = blockIdx.y, q0 = blockIdx.z * kGroup;
  const bool inside = p < SS;
  const float* in = chunk + (size_t)b * chunks * (Q + 1) * SS + min(p, SS - 1);
  float nrm = 0.0f, dot[kGroup];
#pragma unroll
  for (int g = 0; g < kGroup; ++g) dot[g] = 0.0f;
  for (int k0 = 0; k0 < chunks; k0 += kAhead) {
    float vn[kAhead], vd[kAhead][kGroup];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const float* at = in + (size_t)min(k0 + u, chunks - 1) * (Q + 1) * SS;   // past the last chunk: the last one again, not used
      vn[u] = at[0];
#pragma unroll
      for (int g = 0; g < kGroup; ++g) vd[u][g] = at[(size_t)(1 + min(q0 + g, Q - 1)) * SS];
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
      if (k0 + u < chunks) {
        nrm = __fadd_rn(nrm, vn[u]);
#pragma unroll
        for (int g = 0; g < kGroup; ++g) dot[g] = __fadd_rn(dot[g], vd[u][g]);
      }
  }
#pragma unroll
  for (int g = 0; g < kGroup; ++g)
    if (q0 + g < Q) {   // uniform
      const int q = q0 + g;
      float s = inside ? match_score(dot[g], nrm) : -INFINITY;
      int i = inside ? p : kNoIndex;
      if (score_map && inside) score_map[((size_t)b * Q + q) * SS + p] = s;
      wave_best(s, i);
      if (threadIdx.x == 0) {
        const size_t o = ((size_t)b * Q + q) * gridDim.x + blockIdx.x;
        qpart_v[o] = s;
        qpart_i[o] = i;
      }
    }
}

// The merge of all three reduces, one wave per (image, token): the best of its `parts` partials
// -> round `round`'s pos (row + 0.5, col + 0.5) at 2·(bt·num + round); plain and scored have num 1
// and round 0.  The winning value goes to `value` (stride `value_stride`: the scores' first column,
// or the peaks' values) and its linear index to `index` (the window kernel's peak, or the pick the
// next round masks) where they are given.  kScored: the mass partials are summed too, in a fixed
// order (lane k takes partials k, k + 64, … in order, then the wave tree), into `total`.  kEntropy:
// part_m and part_t hold the tiles' (S0, T) about their own maxima; once every lane has the plane's
// maximum, lane k takes in partials k, k + 64, … in order (entropy_add), the wave tree sums both, and
// `total` gets log S0 − T / S0.
//
// kPeaks reduces in torch.argmax's order (argmax_better: a masked +inf is NaN, and NaN wins), which
// its rounds after the first need.  Round-0 partials hold no NaN (the tile kernel turns NaN into 0
// before its argmax), and on NaN-free values argmax_better is `better`: the greater value, on equal
// values the lower index, a total order, so every variant's round 0 picks the same partial.  The
// NaN-free reduction stays for kPlain and kScored because it is faster there: measured in their
// place, the argmax-order merge took 8.3 µs against 6.9 µs (640 waves) and 9.1 against 7.8 (2560).
enum Variant { kPlain, kScored, kPeaks, kEntropy, kParts, kMatch };   // kParts, kMatch: layouts only, their merges are kPlain's
template <Variant V>
__global__ __launch_bounds__(WAVE) void tta_merge_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i,
                                                         const double* __restrict__ part_m, int parts, int S, int num,
                                                         int round, float* __restrict__ pos, float* __restrict__ value,
                                                         int value_stride, int* __restrict__ index,
                                                         double* __restrict__ total,
                                                         const double* __restrict__ part_t, float scale) {
  constexpr bool MASS = V == kScored, NAN_WINS = V == kPeaks;
  const size_t o = (size_t)blockIdx.x * parts;
  float v = -INFINITY;
  int i = kNoIndex;
  double m = 0.0;
  for (int k = threadIdx.x; k < parts; k += WAVE) {
    if (NAN_WINS ? argmax_better(part_v[o + k], part_i[o + k], v, i) : better(part_v[o + k], part_i[o + k], v, i)) {
      v = part_v[o + k];
      i = part_i[o + k];
    }
    if constexpr (MASS) m += part_m[o + k];
  }
  if constexpr (NAN_WINS) wave_argmax(v, i);
  else wave_best(v, i);
  if constexpr (MASS) m = wave_sum_tree(m);
  [[maybe_unused]] double t = 0.0;
  if constexpr (V == kEntropy) {
    for (int k = threadIdx.x; k < parts; k += WAVE)
      entropy_add(m, t, part_v[o + k], part_m[o + k], part_t[o + k], v, scale);
    m = wave_sum_tree(m);
    t = wave_sum_tree(t);
  }
  if (threadIdx.x == 0) {
    const size_t q = (size_t)blockIdx.x * num + round;
    pos[2 * q] = (float)(i / S) + 0.5f;
    pos[2 * q + 1] = (float)(i % S) + 0.5f;
    if (value) value[q * value_stride] = v;
    if (index) index[q] = i;
    if constexpr (MASS) total[blockIdx.x] = m;
    if constexpr (V == kEntropy) total[blockIdx.x] = log(m) - t / m;
  }
}

// The TTA average of one pixel of one token, as the tile kernel forms it: the same functions in
// the same order, so the same bits.  `num` is the pixel's sum of the warped ones.
__device__ __forceinline__ float average_at(const float* __restrict__ maps, const float* __restrict__ th, int C,
                                            size_t copy_stride, int y, int x, int S, float& num) {
#pragma clang fp contract(off)
  constexpr int kAhead = 4;   // copies whose loads are in flight together; the sums stay in copy order
  float sum = 0.0f;
  num = 0.0f;
  for (int c0 = 0; c0 < C; c0 += kAhead) {
    Taps t[kAhead];
    Pair raw[kAhead][2];
    float ones[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      const int c = min(c0 + k, C - 1);   // past the last copy: the last one again, loaded and not added
      const Bilin g = grid_point(th + 6 * c, y, x, S, S);
      ones[k] = sample_ones(g, S, S);
      t[k] = taps_of(g, S);
      const float* plane = maps + c * copy_stride;
#pragma unroll
      for (int r = 0; r < 2; ++r) raw[k][r] = *reinterpret_cast<const Pair*>(plane + t[k].off[r]);
    }
#pragma unroll
    for (int k = 0; k < kAhead; ++k)
      if (c0 + k < C) {
        num = __fadd_rn(num, ones[k]);
        sum = __fadd_rn(sum, sample_taps(raw[k], t[k]));
      }
  }
  const float a = __fdiv_rn(sum, num);
  return a != a ? 0.0f : a;
}

// One workgroup per (image, token): the box of rows r* ± ⌊distance⌋ and columns c* ± ⌊distance⌋
// around the merged peak, clipped to the plane; the average recomputed on it; of the pixels within
// `distance` of the peak (weighted_avg_kernel's predicate and arithmetic, skp_select.hip) the mass,
// the centroid, and the mass over the total; the share of the copies that saw the peak pixel.
constexpr int kMaxDistance = 16;
constexpr int kMaxBox = (2 * kMaxDistance + 1) * (2 * kMaxDistance + 1);
__global__ __launch_bounds__(kThreads) void tta_window_kernel(const float* __restrict__ maps,
                                                              const float* __restrict__ theta_inv, int C, int n, int S,
                                                              float distance, const int* __restrict__ peak_i,
                                                              const double* __restrict__ total,
                                                              float* __restrict__ refined, float* __restrict__ scores) {
  __shared__ float s_val[kMaxBox];
  __shared__ double sd[kWaves];
  __shared__ float s_num;
  const int SS = S * S, b = blockIdx.x / n, tok = blockIdx.x % n;
  const Box box = clipped_box(peak_i[blockIdx.x], S, (int)distance);
  const int r0 = box.r0, c0 = box.c0, ylo = box.ylo, yhi = box.yhi, xlo = box.xlo, xhi = box.xhi;
  const int bw = xhi - xlo + 1, cnt = bw * (yhi - ylo + 1);   // <= kMaxBox: distance <= kMaxDistance
  const float* th = theta_inv + (size_t)b * C * 6;
  const float* plane0 = maps + ((size_t)b * C * n + tok) * SS;
  const float r = (float)r0, c = (float)c0;
  double tot = 0.0;
  for (int e = threadIdx.x; e < cnt; e += kThreads) {
    const int y = ylo + e / bw, x = xlo + e % bw;
    const float dx = (float)y - r, dy = (float)x - c;
    float v = 0.0f;
    if (sqrt_rn(dx * dx + dy * dy) <= distance) {
      float num;
      v = average_at(plane0, th, C, (size_t)n * SS, y, x, S, num);
      if (y == r0 && x == c0) s_num = num;
    }
    s_val[e] = v;
    tot += (double)v;
  }
  tot = block_sum(tot, sd);
  const float denom = (float)tot + 1e-6f;
  double xs = 0.0, ys = 0.0;
  for (int e = threadIdx.x; e < cnt; e += kThreads) {
    const float y = (float)(ylo + e / bw), x = (float)(xlo + e % bw);
    const float nv = s_val[e] / denom;
    xs += (double)(y * nv);
    ys += (double)(x * nv);
  }
  xs = block_sum(xs, sd);
  ys = block_sum(ys, sd);
  if (threadIdx.x == 0) {
    refined[2 * (size_t)blockIdx.x] = (float)xs + 0.5f;
    refined[2 * (size_t)blockIdx.x + 1] = (float)ys + 0.5f;
    scores[3 * (size_t)blockIdx.x + 1] = (float)(tot / (total[blockIdx.x] + 1e-6));
    scores[3 * (size_t)blockIdx.x + 2] = __fdiv_rn(s_num, (float)C);
  }
}

// Tiles a span of `len` pixels can meet, wherever it starts.
__host__ __device__ inline int span_tiles(int len, int tile) { return (len + 2 * tile - 2) / tile; }

// Round `round` >= 1 of the k-peak reduce.  grid (B · n · slots): workgroup `slot` of an (image,
// token) takes the slot-th tile, row-major, of those that meet the box of rows r ± R and columns
// c ± R around the newest pick (r, c), clipped to the plane; R is such that no pixel outside the box
// is within the radius (the host picks it), and slots >= the tiles such a box can meet, so slots
// past the actual count leave at once.  A thread takes the tile kernel's pixel of the tile, forms
// its average with average_at, multiplies by every pick's mask in pick order and the workgroup
// overwrites the tile's partial.
__global__ __launch_bounds__(kThreads) void tta_masked_tile_kernel(const float* __restrict__ maps,
                                                                   const float* __restrict__ theta_inv, int C, int n,
                                                                   int S, int num, int round, float radius2, int R,
                                                                   int slots, const int* __restrict__ picks,
                                                                   float* __restrict__ part_v,
                                                                   int* __restrict__ part_i) {
  __shared__ float s_v[kWaves];
  __shared__ int s_i[kWaves];
  const int SS = S * S, bt = blockIdx.x / slots, slot = blockIdx.x % slots;
  const int b = bt / n, tok = bt % n;
  const int* pk = picks + (size_t)bt * num;
  const Box box = clipped_box(pk[round - 1], S, R);   // around the newest pick
  const int ty0 = box.ylo / kTileH, ty1 = box.yhi / kTileH, tx0 = box.xlo / kTileW, tx1 = box.xhi / kTileW;
  const int ntx = tx1 - tx0 + 1;
  if (slot >= ntx * (ty1 - ty0 + 1)) return;   // uniform
  const int ty = ty0 + slot / ntx, tx = tx0 + slot % ntx;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int x, y;
  tile_pixel(tx, ty, x, y);
  float v = -INFINITY;
  int p = kNoIndex;
  if (x < S && y < S) {
    float ones;
    v = average_at(maps + ((size_t)b * C * n + tok) * SS, theta_inv + (size_t)b * C * 6, C, (size_t)n * SS, y, x, S,
                   ones);
    p = y * S + x;
    const float fx = (float)x, fy = (float)y;
    for (int q = 0; q < round; ++q) {
      const int pq = pk[q];
      const float dx = fx - ((float)(pq % S) + 0.5f), dy = fy - ((float)(pq / S) + 0.5f);
      v = v * ((dx * dx + dy * dy > radius2) ? 1.0f : 0.0f);
    }
  }
  wave_argmax(v, p);
  if (lane == 0) {
    s_v[wid] = v;
    s_i[wid] = p;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kWaves; ++k)
      if (argmax_better(s_v[k], s_i[k], v, p)) {
        v = s_v[k];
        p = s_i[k];
      }
    const size_t o = (size_t)bt * (tiles_x(S) * tiles_y(S)) + (size_t)ty * tiles_x(S) + tx;
    part_v[o] = v;
    part_i[o] = p;
  }
}

// The box half-width of a mask: the least R with every pixel more than R rows (or columns) from a
// pick's outside its disc, (R + 0.5)² > radius2 with room for the float rounding of the predicate;
// a box wider than the plane is the plane.
inline int mask_box(float radius2, int S) {
  const double r = std::sqrt((double)radius2);
  return r >= (double)S ? S : (int)r + 1;
}

// The workspace of every reduce, stated once: the queries return `bytes`, the entry points take
// their pointers from the offsets.  With T tiles per plane and P = B·n·T partials:
//   part_v  P floats, part_i  P ints                  (all variants; 8·P bytes)
//   part_m  P doubles, total  B·n doubles, peak_i  B·n ints in B·n·8 bytes    (scored)
//   picks   B·n·num ints, rounded up to 8 bytes                               (peaks)
//   part_m  P doubles (the tiles' S0), part_t  P doubles (their T)            (entropy)
//   with chunks = ⌈n / kTok⌉ > 1 and Q = B·chunks·S²: cv  Q floats, cm  Q floats, cl  Q shorts,
//   each rounded up to 8 bytes                                                (parts)
//   with `num` = the queries, chunks = ⌈n / kTok⌉ and R = T (chunks == 1) or ⌈S² / 64⌉ partials per
//   (image, query): chunk  (num + 1)·B·chunks·S² floats (chunks > 1 only), qpart_v  B·num·R floats,
//   qpart_i  B·num·R ints, each rounded up to 8 bytes                         (match)
// `bytes` is −1 for a shape no reduce takes (the queries' answer) and for 2^31 bytes or more.
struct Layout {
  long long part_v, part_i, part_m, part_t, total, peak_i, picks, cv, cm, cl, chunk, qpart_v, qpart_i;   // byte offsets; 0 where the
                                                                                         // variant has none
  long long bytes;
};
Layout layout(int B, int n, int S, Variant variant, int num) {
  Layout L = {};
  L.bytes = -1;
  if (B <= 0 || n <= 0 || S < 2 || (variant == kPeaks && (num < 1 || num > kMaxPeaks)) ||
      (variant == kMatch && (num < 1 || num > kMaxQueries)))
    return L;
  const long long bt = (long long)B * n, tiles = (long long)tiles_x(S) * tiles_y(S), big = 1ll << 28;
  if (bt >= big || tiles >= big || bt * tiles >= big) return L;   // 8·bt·tiles bytes of partials alone
  const long long parts = bt * tiles;
  long long end = 0;
  auto take = [&end](long long nbytes) {
    const long long at = end;
    end += nbytes;
    return at;
  };
  L.part_v = take(4 * parts);
  L.part_i = take(4 * parts);
  if (variant == kScored) {
    L.part_m = take(8 * parts);
    L.total = take(8 * bt);
    L.peak_i = take(8 * bt);
  }
  if (variant == kEntropy) {
    L.part_m = take(8 * parts);
    L.part_t = take(8 * parts);
  }
  if (variant == kPeaks) L.picks = take((4 * bt * num + 7) & ~7ll);
  if (variant == kParts && n > kTok) {
    const long long Q = (long long)B * ((n + kTok - 1) / kTok) * S * S;   // <= B·n·S² <= 256·parts < 2^36
    L.cv = take((4 * Q + 7) & ~7ll);
    L.cm = take((4 * Q + 7) & ~7ll);
    L.cl = take((2 * Q + 7) & ~7ll);
  }
  if (variant == kMatch) {
    const long long chunks = (n + kTok - 1) / kTok, SS = (long long)S * S;
    // (num + 1)·B·chunks·S² <= 17·B·n·S² <= 17·256·parts < 2^41
    if (chunks > 1) L.chunk = take((4 * (num + 1) * B * chunks * SS + 7) & ~7ll);
    const long long R = chunks > 1 ? (SS + WAVE - 1) / WAVE : tiles;
    L.qpart_v = take((4 * B * num * R + 7) & ~7ll);
    L.qpart_i = take((4 * B * num * R + 7) & ~7ll);
  }
  if (end < (1ll << 31)) L.bytes = end;
  return L;
}
template <class T>
T* at(void* workspace, long long offset) {
  return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset);
}

// The checks the entry points share, in the order each of them always made them; `own` is
// the message of the variant's failed checks that come before the workspace's (num and radius2 of
// the k-peak reduce), or null.  Returns the first failure's message, or null.
const char* check_common(bool pointers, int B, int C, int n, int S, const char* own, const Layout& L,
                         const void* workspace) {
  if (!pointers) return "null pointer";
  if (!(B > 0 && C > 0 && n > 0 && S > 0)) return "non-positive shape";
  if (S < 2) return "S must be at least 2 (the two taps of a row are loaded as a pair)";
  if (!(S < 46341 && (long long)B * C * n * S * S < (1ll << 31))) return "maps of 2^31 elements or more";
  if (B > 65535) return "more than 65535 images";
  if (own) return own;
  if (L.bytes <= 0) return "workspace of 2^31 bytes or more";
  if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return "workspace must be 8-byte aligned";
  return nullptr;
}

// The tile kernel's launch: grid (tiles, B), the partials where `L` puts them.
template <bool SCORED>
void launch_tile(const float* maps, int B, int C, int n, int S, const float* theta_inv, float* avg, void* workspace,
                 const Layout& L, hipStream_t st) {
  TileArgsOf<SCORED> A;
  A.maps = maps, A.theta_inv = theta_inv, A.avg = avg;
  A.part_v = at<float>(workspace, L.part_v), A.part_i = at<int>(workspace, L.part_i);
  if constexpr (SCORED) A.part_m = at<double>(workspace, L.part_m);
  A.C = C, A.n = n, A.S = S;
  hipLaunchKernelGGL(tta_tile_kernel<SCORED>, dim3(tiles_x(S) * tiles_y(S), B), dim3(kThreads), 0, st, A);
}

// The match reduce's tile kernel on its bucket of queries, grid (tiles, B, chunks), and with more than
// one chunk the per-pixel merge over them (not launched where the tile kernel's launch failed: the
// caller's check reports that error).
template <int QB>
void launch_match(const MatchTileArgs& A, int B, int chunks, hipStream_t st) {
  const int S = A.S, SS = S * S;
  const dim3 grid(tiles_x(S) * tiles_y(S), B, chunks);
  if (chunks == 1) {
    hipLaunchKernelGGL((tta_tile_match_kernel<QB, true>), grid, dim3(kThreads), 0, st, A);
    return;
  }
  hipLaunchKernelGGL((tta_tile_match_kernel<QB, false>), grid, dim3(kThreads), 0, st, A);
  if (hipPeekAtLastError() == hipSuccess)
    hipLaunchKernelGGL(tta_match_merge_kernel, dim3((SS + WAVE - 1) / WAVE, B, (A.Q + 3) / 4), dim3(WAVE), 0, st, A.chunk,
                       chunks, SS, A.Q, A.score_map, A.qpart_v, A.qpart_i);
}

}  // namespace

extern "C" int skp_tta_reduce_workspace(int B, int n, int S) { return (int)layout(B, n, S, kPlain, 1).bytes; }

extern "C" int skp_tta_reduce(const float* maps, int B, int C, int n, int S, const float* theta_inv, float* pos,
                              float* avg, void* workspace, void* stream) {
  const Layout L = layout(B, n, S, kPlain, 1);
  const char* bad = check_common(maps && theta_inv && pos && workspace, B, C, n, S, nullptr, L, workspace);
  SKP_CHECK_ARG(!bad, bad);
  hipStream_t st = as_stream(stream);
  launch_tile<false>(maps, B, C, n, S, theta_inv, avg, workspace, L, st);
  SKP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_merge_kernel<kPlain>, dim3(B * n), dim3(WAVE), 0, st, at<float>(workspace, L.part_v),
                     at<int>(workspace, L.part_i), nullptr, tiles_x(S) * tiles_y(S), S, 1, 0, pos, nullptr, 0, nullptr,
                     nullptr, nullptr, 0.0f);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_tta_reduce_scored_workspace(int B, int n, int S) { return (int)layout(B, n, S, kScored, 1).bytes; }

extern "C" int skp_tta_reduce_scored(const float* maps, int B, int C, int n, int S, const float* theta_inv,
                                     float distance, float* pos, float* refined, float* scores, float* avg,
                                     void* workspace, void* stream) {
  const Layout L = layout(B, n, S, kScored, 1);
  const char* bad =
      check_common(maps && theta_inv && pos && refined && scores && workspace, B, C, n, S, nullptr, L, workspace);
  SKP_CHECK_ARG(!bad, bad);
  SKP_CHECK_ARG(distance > 0.0f && distance <= (float)kMaxDistance, "distance must be in (0, 16]");
  double* total = at<double>(workspace, L.total);
  int* peak_i = at<int>(workspace, L.peak_i);
  hipStream_t st = as_stream(stream);
  launch_tile<true>(maps, B, C, n, S, theta_inv, avg, workspace, L, st);
  SKP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_merge_kernel<kScored>, dim3(B * n), dim3(WAVE), 0, st, at<float>(workspace, L.part_v),
                     at<int>(workspace, L.part_i), at<double>(workspace, L.part_m), tiles_x(S) * tiles_y(S), S, 1, 0, pos,
                     scores, 3, peak_i, total, nullptr, 0.0f);
  SKP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_window_kernel, dim3(B * n), dim3(kThreads), 0, st, maps, theta_inv, C, n, S, distance, peak_i,
                     total, refined, scores);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_tta_reduce_peaks_workspace(int B, int n, int S, int num, float radius2) {
  if (!(radius2 > 0.0f) || !std::isfinite(radius2)) return -1;
  return (int)layout(B, n, S, kPeaks, num).bytes;
}

extern "C" int skp_tta_reduce_peaks(const float* maps, int B, int C, int n, int S, const float* theta_inv, int num,
                                    float radius2, float* pos, float* values, float* avg, void* workspace,
                                    void* stream) {
  const char* own = !(num >= 1 && num <= kMaxPeaks)                ? "num must be in [1, 16]"
                    : !(radius2 > 0.0f && std::isfinite(radius2)) ? "radius2 must be positive and finite"
                                                                  : nullptr;
  const Layout L = layout(B, n, S, kPeaks, num);
  const char* bad = check_common(maps && theta_inv && pos && values && workspace, B, C, n, S, own, L, workspace);
  SKP_CHECK_ARG(!bad, bad);
  const int tiles = tiles_x(S) * tiles_y(S);
  const int R = mask_box(radius2, S);
  const int slots =
      std::min(span_tiles(2 * R + 1, kTileH), tiles_y(S)) * std::min(span_tiles(2 * R + 1, kTileW), tiles_x(S));
  SKP_CHECK_ARG(num == 1 || (long long)B * n * slots < (1ll << 31), "masked-tile grid of 2^31 workgroups or more");
  float* part_v = at<float>(workspace, L.part_v);
  int* part_i = at<int>(workspace, L.part_i);
  int* picks = at<int>(workspace, L.picks);
  hipStream_t st = as_stream(stream);
  launch_tile<false>(maps, B, C, n, S, theta_inv, avg, workspace, L, st);
  SKP_LAUNCH_CHECK();
  for (int round = 0; round < num; ++round) {
    if (round) {
      hipLaunchKernelGGL(tta_masked_tile_kernel, dim3(B * n * slots), dim3(kThreads), 0, st, maps, theta_inv, C, n, S,
                         num, round, radius2, R, slots, picks, part_v, part_i);
      SKP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tta_merge_kernel<kPeaks>, dim3(B * n), dim3(WAVE), 0, st, part_v, part_i, nullptr, tiles, S, num,
                       round, pos, values, 1, picks, nullptr, nullptr, 0.0f);
    SKP_LAUNCH_CHECK();
  }
  return SKP_OK;
}

extern "C" int skp_tta_reduce_entropy_workspace(int B, int n, int S) { return (int)layout(B, n, S, kEntropy, 1).bytes; }

extern "C" int skp_tta_reduce_entropy(const float* maps, int B, int C, int n, int S, const float* theta_inv,
                                      float scale, float* pos, double* entropy, float* avg, void* workspace,
                                      void* stream) {
  const char* own = !(scale > 0.0f && std::isfinite(scale)) ? "scale must be positive and finite" : nullptr;
  const Layout L = layout(B, n, S, kEntropy, 1);
  const char* bad = check_common(maps && theta_inv && pos && entropy && workspace, B, C, n, S, own, L, workspace);
  SKP_CHECK_ARG(!bad, bad);
  const int tiles = tiles_x(S) * tiles_y(S), chunks = (n + kTok - 1) / kTok;
  SKP_CHECK_ARG(chunks <= 65535, "more than 65535 chunks of tokens");
  EntropyTileArgs A;
  A.maps = maps, A.theta_inv = theta_inv, A.avg = avg;
  A.part_v = at<float>(workspace, L.part_v), A.part_i = at<int>(workspace, L.part_i);
  A.part_s0 = at<double>(workspace, L.part_m), A.part_t = at<double>(workspace, L.part_t);
  A.C = C, A.n = n, A.S = S, A.scale = scale;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(tta_tile_entropy_kernel, dim3(tiles, B, chunks), dim3(kThreads), 0, st, A);
  SKP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_merge_kernel<kEntropy>, dim3(B * n), dim3(WAVE), 0, st, A.part_v, A.part_i, A.part_s0, tiles,
                     S, 1, 0, pos, nullptr, 0, nullptr, entropy, A.part_t, scale);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_tta_reduce_parts_workspace(int B, int n, int S) { return (int)layout(B, n, S, kParts, 1).bytes; }

extern "C" int skp_tta_reduce_parts(const float* maps, int B, int C, int n, int S, const float* theta_inv, float* pos,
                                    short* label, float* value, float* mass, float* avg, void* workspace,
                                    void* stream) {
  const int tiles = tiles_x(S) * tiles_y(S), chunks = (n + kTok - 1) / kTok;
  const char* own = n > 32767        ? "more than 32767 tokens (the label is int16)"
                    : chunks > 65535 ? "more than 65535 chunks of tokens"
                                     : nullptr;
  const Layout L = layout(B, n, S, kParts, 1);
  const char* bad =
      check_common(maps && theta_inv && pos && label && value && mass && workspace, B, C, n, S, own, L, workspace);
  SKP_CHECK_ARG(!bad, bad);
  const bool direct = chunks == 1;
  PartsTileArgs A;
  A.maps = maps, A.theta_inv = theta_inv, A.avg = avg;
  A.part_v = at<float>(workspace, L.part_v), A.part_i = at<int>(workspace, L.part_i);
  A.out_v = direct ? value : at<float>(workspace, L.cv);
  A.out_l = direct ? label : at<short>(workspace, L.cl);
  A.out_m = direct ? mass : at<float>(workspace, L.cm);
  A.C = C, A.n = n, A.S = S;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(tta_tile_parts_kernel, dim3(tiles, B, chunks), dim3(kThreads), 0, st, A);
  SKP_LAUNCH_CHECK();
  if (!direct) {
    hipLaunchKernelGGL(tta_parts_merge_kernel, dim3((S * S + WAVE - 1) / WAVE, B), dim3(WAVE), 0, st,
                       A.out_v, A.out_l, A.out_m, chunks, S * S, value, label, mass);
    SKP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(tta_merge_kernel<kPlain>, dim3(B * n), dim3(WAVE), 0, st, A.part_v, A.part_i, nullptr, tiles, S, 1,
                     0, pos, nullptr, 0, nullptr, nullptr, nullptr, 0.0f);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_tta_reduce_match_workspace(int B, int n, int S, int Q) { return (int)layout(B, n, S, kMatch, Q).bytes; }

extern "C" int skp_tta_reduce_match(const float* maps, int B, int C, int n, int S, const float* theta_inv,
                                    const float* queries, int Q, float* pos, float* match_pos, float* match_score,
                                    float* score_map, float* avg, void* workspace, void* stream) {
  const int tiles = tiles_x(S) * tiles_y(S), chunks = (n + kTok - 1) / kTok;
  const char* own = !(Q >= 1 && Q <= kMaxQueries) ? "Q must be in [1, 16]"
                    : chunks > 65535              ? "more than 65535 chunks of tokens"
                                                  : nullptr;
  const Layout L = layout(B, n, S, kMatch, Q);
  const char* bad = check_common(maps && theta_inv && queries && pos && match_pos && match_score && workspace, B, C, n, S,
                                 own, L, workspace);
  SKP_CHECK_ARG(!bad, bad);
  MatchTileArgs A;
  A.maps = maps, A.theta_inv = theta_inv, A.avg = avg;
  A.part_v = at<float>(workspace, L.part_v), A.part_i = at<int>(workspace, L.part_i);
  A.queries = queries, A.chunk = at<float>(workspace, L.chunk), A.score_map = score_map;
  A.qpart_v = at<float>(workspace, L.qpart_v), A.qpart_i = at<int>(workspace, L.qpart_i);
  A.C = C, A.n = n, A.S = S, A.Q = Q;
  hipStream_t st = as_stream(stream);
  if (Q <= 4) launch_match<4>(A, B, chunks, st);
  else if (Q <= 8) launch_match<8>(A, B, chunks, st);
  else launch_match<16>(A, B, chunks, st);
  SKP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_merge_kernel<kPlain>, dim3(B * n), dim3(WAVE), 0, st, A.part_v, A.part_i, nullptr, tiles, S, 1,
                     0, pos, nullptr, 0, nullptr, nullptr, nullptr, 0.0f);
  SKP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tta_merge_kernel<kPlain>, dim3(B * Q), dim3(WAVE), 0, st, A.qpart_v, A.qpart_i, nullptr,
                     chunks > 1 ? (S * S + WAVE - 1) / WAVE : tiles, S, 1, 0, match_pos, match_score, 1, nullptr, nullptr,
                     nullptr, 0.0f);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}
