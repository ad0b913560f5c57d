// The pinned half-pixel-centre tap arithmetic shared by the bilinear resize
// ingest kernels (pack_kernels.hip, whose resize section documents the
// formulas) and the resampling loader of the ViT patch-embedding kernel
// (patch_embed.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace mi355x {

// Source index and weight of one output coordinate.
__device__ __forceinline__ void resize_tap(int o, int offset, float ratio,
                                           int n_in, int& i0, int& i1,
                                           float& w) {
  const float s = fmaxf(
      __fsub_rn(__fmul_rn(__fadd_rn(float(o + offset), 0.5f), ratio), 0.5f),
      0.f);
  i0 = min(int(floorf(s)), n_in - 1);
  i1 = min(i0 + 1, n_in - 1);
  w = __fsub_rn(s, float(i0));
}

}  // namespace mi355x
