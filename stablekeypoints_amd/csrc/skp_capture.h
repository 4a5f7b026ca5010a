// Host-side pieces skp_capture.hip and skp_capture_sel.hip share: the argument checks of the
// skp_capture_maps_* entry points and the dense backward's workspace.
#pragma once
#include <algorithm>
#include <cstdint>

#include "skp_common.h"

namespace skp {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Each returns the message of its first failing check, or null.  ptrs: every required pointer is set.
inline const char* maps_shape_error(bool ptrs, int L, int B, int H, int N, int R) {
  if (!ptrs) return "null pointer";
  if (!(L > 0 && L <= SKP_MAX_LAYERS)) return "L out of range";
  return B > 0 && H > 0 && N > 0 && R > 0 ? nullptr : "non-positive shape";
}

// Per layer: its pointers (stats / dz: null where the entry point requires no entries), its size,
// the 16-B alignment of z (and of dz where align_dz).  `after`: the forward judges the alignment
// behind the loop, and only where N % 4 == 0 (it has a scalar path).
inline const char* maps_layers_error(const float* const* z, const float* const* stats, float* const* dz,
                                     const int* sizes, int L, int N, int R, bool align_dz, bool after) {
  const char* unaligned = align_dz ? "z_low / dz_low pointers must be 16-B aligned" : "z_low pointers must be 16-B aligned";
  bool aligned = true;
  for (int l = 0; l < L; ++l) {
    if (!(z[l] && (!dz || dz[l]) && (!stats || stats[l]))) return "null layer pointer";
    if (!(sizes[l] > 0 && sizes[l] <= R)) return "layer size must be in [1, R]";
    const bool al = aligned16(z[l]) && (!align_dz || aligned16(dz[l]));
    if (!al && !after) return unaligned;
    aligned = aligned && al;
  }
  return aligned || N % 4 != 0 ? nullptr : unaligned;
}

inline int widest_layer(const int* sizes, int L) {   // smax (at least 1)
  int smax = 1;
  for (int l = 0; l < L; ++l) smax = std::max(smax, sizes[l]);
  return smax;
}

// skp_capture_maps_bwd's workspace (floats): the pixel-major gradient gT (B, R², N) at 0, then the
// row partials (B·H, R, smax, N), reused per layer
struct MapsBwdWs { size_t rows, total; };
inline MapsBwdWs maps_bwd_ws(const int* sizes, int L, int B, int H, int N, int R) {
  const size_t rows = (size_t)B * R * R * N;
  return {rows, rows + (size_t)B * H * R * widest_layer(sizes, L) * N};
}

}  // namespace skp
