// The affine-grid sample shared by the warp / equivariance kernels (skp_warp.hip) and the fused
// test-time-augmentation reduce (skp_tta.hip): one definition, so every kernel that warps rounds
// alike, bit for bit.
#pragma once
#include "skp_common.h"

namespace skp {

struct Bilin {
  int x0, y0;
  float w[4];  // nw, ne, sw, se
};

// Rounding follows torch-CPU exactly (the reference warps images on the CPU, optimize.py:386, and
// its goldens are CPU runs): affine_grid's bmm of [x, y, 1] by θᵀ rounds as
// fma(y, θ1, x·θ0) + θ2 (measured against F.affine_grid: bit-equal on every grid point), the CPU
// grid sampler unnormalises as fma(g + 1, n/2, −0.5) and forms the bilinear weights from
// w = ix − floor(ix), e = 1 − w (nw = s·e, ne = s·w, sw = n·e, se = n·w), and the sample as
// ((v_nw·nw + v_ne·ne) + v_sw·sw) + v_se·se without fused multiply-adds.
__device__ __forceinline__ Bilin grid_point(const float* th, int y, int x, int H, int W) {
  const float bx = affine_base(x, W), by = affine_base(y, H);
  const float gx = __fadd_rn(__fmaf_rn(by, th[1], __fmul_rn(bx, th[0])), th[2]);
  const float gy = __fadd_rn(__fmaf_rn(by, th[4], __fmul_rn(bx, th[3])), th[5]);
  const float ix = __fmaf_rn(__fadd_rn(gx, 1.0f), (float)W * 0.5f, -0.5f);
  const float iy = __fmaf_rn(__fadd_rn(gy, 1.0f), (float)H * 0.5f, -0.5f);
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float we = __fsub_rn(ix, x0), ee = __fsub_rn(1.0f, we);   // distance to the west / east side
  const float wn = __fsub_rn(iy, y0), ws = __fsub_rn(1.0f, wn);   // distance to the north / south side
  Bilin b;
  b.x0 = (int)x0;
  b.y0 = (int)y0;
  b.w[0] = __fmul_rn(ws, ee);
  b.w[1] = __fmul_rn(ws, we);
  b.w[2] = __fmul_rn(wn, ee);
  b.w[3] = __fmul_rn(wn, we);
  return b;
}

__device__ __forceinline__ float sample(const float* __restrict__ p, const Bilin& b, int H, int W) {
  float out = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = b.x0 + (k & 1), yy = b.y0 + (k >> 1);
    const float v = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? p[yy * W + xx] : 0.0f;
    out = k == 0 ? __fmul_rn(v, b.w[0]) : __fadd_rn(out, __fmul_rn(v, b.w[k]));
  }
  return out;
}

// sample() of a plane of ones, without the plane: ((nw + ne) + sw) + se over the in-range taps,
// formed by the same operations in the same order (1·w and 0·w are what sample computes there).
__device__ __forceinline__ float sample_ones(const Bilin& b, int H, int W) {
  float out = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = b.x0 + (k & 1), yy = b.y0 + (k >> 1);
    const float v = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? 1.0f : 0.0f;
    out = k == 0 ? __fmul_rn(v, b.w[0]) : __fadd_rn(out, __fmul_rn(v, b.w[k]));
  }
  return out;
}

}  // namespace skp
