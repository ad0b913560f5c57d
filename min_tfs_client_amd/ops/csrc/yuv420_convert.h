// The pinned int32 YUV 4:2:0 -> RGB conversion shared by the resize ingest
// kernels (pack_kernels.hip, whose YUV section documents the frame layout
// and the formulas) and the ViT patch-embedding kernel (patch_embed.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mi355x {

struct Yuv420Coef {
  int yoff, yc, rv, gu, gv, bu;
};

// clamp(v >> 8, 0, 255), written clamp first: the same value for every v.
// The shift-then-clamp form is selected as v_ashr_pk_u8_i32 for pairs of
// values by hipcc (ROCm 7.2), and the packed bytes came out wrong on MI355X.
__device__ __forceinline__ uint32_t yuv_clamp8(int v) {
  return uint32_t(min(max(v, 0), 0xffff)) >> 8;
}

}  // namespace mi355x
