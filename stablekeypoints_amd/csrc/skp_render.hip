// A17: the visualisation sheets (keypoint markers and heat-map overlays on a grid of image tiles),
// composited on the device into one uint8 RGB image, for gfx950.
//
// Reference: visualize.py:105-138 (plot_point_correspondences: a height×width grid of images with
// one marker per keypoint) and visualize.py:40-73 (save_grid: images and the same images under the
// min/max-normalised map at alpha 0.7).  The reference draws both with matplotlib on the host;
// here every output pixel is gathered by exactly one thread (no atomics, no painter passes), so
// the sheet is deterministic and can be restated number for number.
#include "skp_common.h"

using namespace skp;

namespace {

constexpr int kThreads = 256;
constexpr int kRangeThreads = 1024;   // one workgroup per map: as many loads in flight as a workgroup holds
constexpr int kMaxMarkers = 64;

// ------------------------------------------------------------------------------------ map range
// One workgroup per map: (min, max), or (NaN, NaN) when the map holds a non-finite value or is
// constant.  min/max do not depend on the order of combination, so the result is bit-exact.
struct RangeAcc {
  float mn, mx, bad;
  __device__ __forceinline__ void add(float v) {
    bad = fabsf(v) < INFINITY ? bad : 1.0f;   // NaN compares false
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
};

__global__ __launch_bounds__(kRangeThreads) void map_range_kernel(const float* __restrict__ maps, int hw, int vec,
                                                            float* __restrict__ range) {
  __shared__ float s_mn[kRangeThreads / WAVE], s_mx[kRangeThreads / WAVE], s_bad[kRangeThreads / WAVE];
  const float* m = maps + (size_t)blockIdx.x * hw;
  RangeAcc a{INFINITY, -INFINITY, 0.0f};
  if (vec) {   // hw % 4 == 0 and a 16-B aligned base: every map starts 16-B aligned
    const float4* m4 = reinterpret_cast<const float4*>(m);
    for (int i = threadIdx.x; i < hw / 4; i += kRangeThreads) {
      const float4 v = m4[i];
      a.add(v.x);
      a.add(v.y);
      a.add(v.z);
      a.add(v.w);
    }
  } else {
    for (int i = threadIdx.x; i < hw; i += kRangeThreads) a.add(m[i]);
  }
  a.mn = wave_reduce(a.mn, [](float x, float y) { return fminf(x, y); });
  a.mx = wave_max(a.mx);
  a.bad = wave_max(a.bad);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    s_mn[wid] = a.mn;
    s_mx[wid] = a.mx;
    s_bad[wid] = a.bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mn = s_mn[0], mx = s_mx[0], bad = s_bad[0];
#pragma unroll
    for (int k = 1; k < kRangeThreads / WAVE; ++k) {
      mn = fminf(mn, s_mn[k]);
      mx = fmaxf(mx, s_mx[k]);
      bad = fmaxf(bad, s_bad[k]);
    }
    const bool none = bad != 0.0f || !(mx > mn);
    range[2 * blockIdx.x] = none ? NAN : mn;
    range[2 * blockIdx.x + 1] = none ? NAN : mx;
  }
}

// ------------------------------------------------------------------------------------ the sheet
struct Sheet {
  const float* images;   // (n, 3, H, W)
  const float* maps;     // (n, h, w) or null
  const float* range;    // (n, 2)
  const float* lut;      // (256, 3)
  const float* points;   // (n, K, 2) normalised (row, col) or null
  const unsigned char* colors;   // (K, 3)
  unsigned char* out;    // (Hs, Ws, 3)
  int n, H, W, h, w, K, cols, f, pad;
  int th, tw, Hs, Ws;    // tile and sheet size
  int vec4;              // f % 4 == 0 and 16-B aligned image rows: float4 source loads
  float alpha, r2, ro2;  // marker radius², outline radius²
  float sy, sx;          // (float)h / H, (float)w / W
  float inv_ff;          // 1 / f²
};

// torch bilinear, align_corners=False (bilinear_taps of skp_common.h with the quotient passed in)
__device__ __forceinline__ Taps2 taps_s(int dst, int n_in, float scale) {
  float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  Taps2 r;
  r.i0 = min((int)src, n_in - 1);
  r.i1 = r.i0 + (r.i0 < n_in - 1 ? 1 : 0);
  r.w1 = src - (float)r.i0;
  r.w0 = 1.0f - r.w1;
  return r;
}

// LUT(v), v in [0, 1]: linear between entries floor(255v) and the next (continuous in v)
__device__ __forceinline__ void lut_at(const float* __restrict__ lut, float v, float& r, float& g, float& b) {
  const float x = 255.0f * v;
  const int i0 = min(max((int)x, 0), 255), i1 = min(i0 + 1, 255);
  const float fr = x - (float)i0;
  const float *a = lut + 3 * i0, *c = lut + 3 * i1;
  r = __builtin_fmaf(fr, c[0] - a[0], a[0]);
  g = __builtin_fmaf(fr, c[1] - a[1], a[1]);
  b = __builtin_fmaf(fr, c[2] - a[2], a[2]);
}

__device__ __forceinline__ unsigned to_byte(float c) {
  c = fminf(fmaxf(c, 0.0f), 1.0f);
  return (unsigned)floorf(__builtin_fmaf(c, 255.0f, 0.5f));
}

// One output pixel as 0x00BBGGRR.  s_lut: the LUT in LDS (HEAT only).
template <bool HEAT>
__device__ __forceinline__ unsigned sheet_pixel(const Sheet& S, const float* __restrict__ s_lut, int y, int x) {
  const unsigned white = 0x00FFFFFFu;
  const int ph = S.th + S.pad, pw = S.tw + S.pad;
  const int ty = y / ph, tx = x / pw;
  const int ry = y - ty * ph - S.pad, rx = x - tx * pw - S.pad;   // position inside the tile
  if (ry < 0 || rx < 0 || tx >= S.cols) return white;             // padding (the last pad row/column too)
  const int t = ty * S.cols + tx;
  if (t >= S.n) return white;                                      // empty tile (or the bottom pad row)
  // markers: the last one that covers the pixel wins; NaN coordinates fail every comparison
  if (S.points) {
    int hit = -1;
    const float* p = S.points + (size_t)t * S.K * 2;
    const float cy = (float)ry + 0.5f, cx = (float)rx + 0.5f;
    for (int j = 0; j < S.K; ++j) {
      const float dy = cy - p[2 * j] * (float)S.th, dx = cx - p[2 * j + 1] * (float)S.tw;
      const float d2 = __builtin_fmaf(dy, dy, dx * dx);
      if (d2 <= S.r2) hit = j;
      else if (d2 <= S.ro2) hit = kMaxMarkers;
    }
    if (hit == kMaxMarkers) return white;
    if (hit >= 0) {
      const unsigned char* c = S.colors + 3 * hit;
      return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
    }
  }
  const size_t plane = (size_t)S.H * S.W;
  const float* img = S.images + (size_t)t * 3 * plane;
  bool heat = false;
  float mn = 0.0f, span = 1.0f;
  const float* map = nullptr;
  if (HEAT) {
    mn = S.range[2 * t];
    const float mx = S.range[2 * t + 1];
    heat = mn == mn && mx == mx;
    span = mx - mn;
    map = S.maps + (size_t)t * S.h * S.w;
  }
  const float ia = 1.0f - S.alpha;
  float ar = 0.0f, ag = 0.0f, ab = 0.0f;
  for (int dy = 0; dy < S.f; ++dy) {
    const int sy = ry * S.f + dy;
    const float* row = img + (size_t)sy * S.W + (size_t)rx * S.f;
    Taps2 ty2{};
    if (HEAT && heat) ty2 = taps_s(sy, S.h, S.sy);
    for (int dx0 = 0; dx0 < S.f; dx0 += 4) {
      float pr[4], pg[4], pb[4];
      int cnt;
      if (S.vec4) {
        const float4 vr = *reinterpret_cast<const float4*>(row + dx0);
        const float4 vg = *reinterpret_cast<const float4*>(row + plane + dx0);
        const float4 vb = *reinterpret_cast<const float4*>(row + 2 * plane + dx0);
        pr[0] = vr.x, pr[1] = vr.y, pr[2] = vr.z, pr[3] = vr.w;
        pg[0] = vg.x, pg[1] = vg.y, pg[2] = vg.z, pg[3] = vg.w;
        pb[0] = vb.x, pb[1] = vb.y, pb[2] = vb.z, pb[3] = vb.w;
        cnt = 4;
      } else {
        cnt = min(4, S.f - dx0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = k < cnt;
          pr[k] = in ? row[dx0 + k] : 0.0f;
          pg[k] = in ? row[plane + dx0 + k] : 0.0f;
          pb[k] = in ? row[2 * plane + dx0 + k] : 0.0f;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= cnt) break;
        float r = pr[k], g = pg[k], b = pb[k];
        if (HEAT && heat) {
          const Taps2 tx2 = taps_s(rx * S.f + dx0 + k, S.w, S.sx);
          const float* m0 = map + (size_t)ty2.i0 * S.w;
          const float* m1 = map + (size_t)ty2.i1 * S.w;
          const float m = ty2.w0 * (tx2.w0 * m0[tx2.i0] + tx2.w1 * m0[tx2.i1]) +
                          ty2.w1 * (tx2.w0 * m1[tx2.i0] + tx2.w1 * m1[tx2.i1]);
          const float v = fminf(fmaxf(__fdiv_rn(m - mn, span), 0.0f), 1.0f);
          float lr, lg, lb;
          lut_at(s_lut, v, lr, lg, lb);
          r = __builtin_fmaf(S.alpha, lr, ia * r);
          g = __builtin_fmaf(S.alpha, lg, ia * g);
          b = __builtin_fmaf(S.alpha, lb, ia * b);
        }
        ar += r;
        ag += g;
        ab += b;
      }
    }
  }
  return to_byte(ar * S.inv_ff) | (to_byte(ag * S.inv_ff) << 8) | (to_byte(ab * S.inv_ff) << 16);
}

// Thread g < nvec composites the four pixels 4g … 4g+3 of the sheet taken as one flat row-major
// array (horizontally adjacent; a group only crosses a row end when Ws % 4 != 0) and stores their
// 12 bytes as three dwords; the threads after those take the total % 4 pixels left, one each,
// with byte stores.
template <bool HEAT>
__global__ __launch_bounds__(kThreads) void render_sheet_kernel(const Sheet S, int nvec, int total) {
  __shared__ float s_lut[HEAT ? 768 : 1];
  if (HEAT) {
    for (int i = threadIdx.x; i < 768; i += kThreads) s_lut[i] = S.lut[i];
    __syncthreads();
  }
  const int g = blockIdx.x * kThreads + threadIdx.x;
  if (g < nvec) {
    const int p0 = 4 * g;
    int y = p0 / S.Ws, x = p0 - y * S.Ws;
    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = sheet_pixel<HEAT>(S, s_lut, y, x);
      if (++x == S.Ws) {
        x = 0;
        ++y;
      }
    }
    uint3 o;
    o.x = px[0] | (px[1] << 24);
    o.y = (px[1] >> 8) | (px[2] << 16);
    o.z = (px[2] >> 16) | (px[3] << 8);
    *reinterpret_cast<uint3*>(S.out + (size_t)p0 * 3) = o;
  } else {
    const int p = 4 * nvec + (g - nvec);
    if (p >= total) return;
    const int y = p / S.Ws, x = p - y * S.Ws;
    const unsigned v = sheet_pixel<HEAT>(S, s_lut, y, x);
    unsigned char* o = S.out + (size_t)p * 3;
    o[0] = (unsigned char)(v & 0xFF);
    o[1] = (unsigned char)((v >> 8) & 0xFF);
    o[2] = (unsigned char)((v >> 16) & 0xFF);
  }
}

}  // namespace

extern "C" int skp_map_range(const float* maps, int n, int h, int w, float* range, void* stream) {
  SKP_CHECK_ARG(maps && range, "null pointer");
  SKP_CHECK_ARG(n > 0 && h > 0 && w > 0, "non-positive shape");
  SKP_CHECK_ARG((long long)h * w < (1ll << 31), "map of 2^31 elements or more");
  const int hw = h * w;
  const int vec = hw % 4 == 0 && reinterpret_cast<uintptr_t>(maps) % 16 == 0;
  hipLaunchKernelGGL(map_range_kernel, dim3(n), dim3(kRangeThreads), 0, as_stream(stream), maps, hw, vec, range);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}

extern "C" int skp_render_sheet(const float* images, int n, int H, int W, const float* maps, int h, int w,
                                const float* range, const float* lut, float alpha, const float* points, int K,
                                float radius, const unsigned char* colors, int rows, int cols, int f, int pad,
                                unsigned char* out, void* stream) {
  SKP_CHECK_ARG(images && out, "null pointer (images, out)");
  SKP_CHECK_ARG(n > 0 && H > 0 && W > 0 && rows > 0 && cols > 0 && f > 0 && pad >= 0, "non-positive shape");
  SKP_CHECK_ARG(H % f == 0 && W % f == 0, "H and W must be a multiple of f");
  SKP_CHECK_ARG((long long)n <= (long long)rows * cols, "more images than rows*cols tiles");
  if (maps) {
    SKP_CHECK_ARG(range && lut, "maps need range (skp_map_range) and lut");
    SKP_CHECK_ARG(h > 0 && w > 0, "non-positive map shape");
    SKP_CHECK_ARG(alpha >= 0.0f && alpha <= 1.0f, "alpha outside [0, 1]");
  }
  SKP_CHECK_ARG(K >= 0 && K <= kMaxMarkers, "K must be at most 64 markers");
  const bool markers = points && K > 0;
  if (markers) {
    SKP_CHECK_ARG(colors, "null pointer (colors)");
    SKP_CHECK_ARG(radius >= 0.0f && radius < 32768.0f, "radius outside [0, 32768)");
  }
  const int th = H / f, tw = W / f;
  const long long Hs = (long long)rows * (th + pad) + pad, Ws = (long long)cols * (tw + pad) + pad;
  SKP_CHECK_ARG(Hs < (1ll << 31) && Ws < (1ll << 31) && Hs * Ws * 3 < (1ll << 31), "sheet of 2^31 bytes or more");
  Sheet S;
  S.images = images;
  S.maps = maps;
  S.range = range;
  S.lut = lut;
  S.points = markers ? points : nullptr;
  S.colors = colors;
  S.out = out;
  S.n = n, S.H = H, S.W = W, S.h = h, S.w = w, S.K = K, S.cols = cols, S.f = f, S.pad = pad;
  S.th = th, S.tw = tw, S.Hs = (int)Hs, S.Ws = (int)Ws;
  S.vec4 = f % 4 == 0 && reinterpret_cast<uintptr_t>(images) % 16 == 0;   // then W % 4 == 0 too
  S.alpha = alpha;
  S.r2 = radius * radius;
  S.ro2 = (radius + 1.0f) * (radius + 1.0f);
  S.sy = maps ? (float)h / (float)H : 1.0f;
  S.sx = maps ? (float)w / (float)W : 1.0f;
  S.inv_ff = 1.0f / ((float)f * (float)f);
  const int total = (int)(Hs * Ws);
  const int nvec = reinterpret_cast<uintptr_t>(out) % 4 == 0 ? total / 4 : 0;
  const int threads = nvec + (total - 4 * nvec);
  const dim3 grid((threads + kThreads - 1) / kThreads);
  if (maps)
    hipLaunchKernelGGL(render_sheet_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), S, nvec, total);
  else
    hipLaunchKernelGGL(render_sheet_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), S, nvec, total);
  SKP_LAUNCH_CHECK();
  return SKP_OK;
}
