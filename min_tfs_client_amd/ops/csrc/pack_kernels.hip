// CDNA4 (gfx950) kernels and copy pipeline for the TensorProto serialize
// hot path.
//
// What runs on the GPU here (SURVEY §2.5 work list):
//  * fused dtype-cast + NCHW->NHWC layout transform (one pass over HBM,
//    LDS-staged tiles for the generic case, an interleave specialization for
//    small channel counts — vs the reference's separate CastFunctor +
//    SwapDimension1And2InTensor3 launches, cast_op_gpu.cu.cc:31-99,
//    conv_2d_gpu.h:217-347),
//  * vectorized elementwise cast (bf16/f16/f32 matrix),
//  * affine int8 quantize/dequantize (the "cast/quantize" pack stage),
//  * fused uint8 image ingest: dequantize + per-channel normalize + NCHW
//    (server-side preprocessing, so clients ship 1 byte per pixel value),
//  * the same ingest with a bilinear resize + crop fused in (images of any
//    size, source taps staged through LDS),
//  * the antialiased variant of that resize (separable variable-width
//    triangle filter, horizontal then vertical pass over an fp32 workspace),
//  * both resizes for ragged batches (N images of N sizes in one flat
//    buffer, a per-image table in device memory),
//  * the bilinear resize for YUV 4:2:0 frames (NV12 / I420, 1.5 bytes per
//    pixel), converted to RGB with integer arithmetic while LDS is filled,
//  * fused masked mean-pool (+ L2 normalize) head: [B,S,H] hidden state ->
//    fp32 [B,H] sentence embeddings, so responses ship S x fewer bytes,
// plus the host-side staging machinery: pinned double-buffered
// device->host-buffer copies that overlap DMA with the host-side wire write
// (the MI355X replacement for the reference's two-slice zero-copy encode,
// grpc_tensor_coding.cc:140-248).
//
// Design rules followed (cdna_hip_programming.md): 64-wide waves, 16 B/lane
// vectorized access (G13), grid-stride with capped grid (G11), LDS padding
// for bank-conflict-free b32 access (G4). No CUDA-compat shims.

#include <hip/hip_runtime.h>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <mutex>
#include <stdexcept>
#include <tuple>
#include <type_traits>
#include <vector>

#include "staging.h"

#define HIP_CHECK(expr)                                                       \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess) {                                                   \
      throw std::runtime_error(std::string("HIP error: ") +                   \
                               hipGetErrorString(_e) + " at " #expr);         \
    }                                                                         \
  } while (0)

namespace mi355x {

// ---------------------------------------------------------------------------
// dtype conversion primitives (bit-exact with torch semantics)
// ---------------------------------------------------------------------------

__device__ __forceinline__ float bf16_to_f32(uint16_t b) {
  uint32_t u = uint32_t(b) << 16;
  return __uint_as_float(u);
}

__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) {       // NaN: quiet, keep sign
    return uint16_t((u >> 16) | 0x0040u);
  }
  uint32_t rounding = 0x7fffu + ((u >> 16) & 1u);
  return uint16_t((u + rounding) >> 16);
}

__device__ __forceinline__ float f16_to_f32(uint16_t h) {
  __half_raw r; r.x = h;
  return __half2float(__half(r));
}

__device__ __forceinline__ uint16_t f32_to_f16(float f) {
  __half h = __float2half(f);
  __half_raw r(h);
  return r.x;
}

// Load/store converters selected by template tag.
struct IdF32 {
  using In = float; using Out = float;
  static __device__ __forceinline__ float cvt(float v) { return v; }
};
struct Bf16ToF32 {
  using In = uint16_t; using Out = float;
  static __device__ __forceinline__ float cvt(uint16_t v) {
    return bf16_to_f32(v);
  }
};
struct F16ToF32 {
  using In = uint16_t; using Out = float;
  static __device__ __forceinline__ float cvt(uint16_t v) {
    return f16_to_f32(v);
  }
};
struct F32ToBf16 {
  using In = float; using Out = uint16_t;
  static __device__ __forceinline__ uint16_t cvt(float v) {
    return f32_to_bf16(v);
  }
};
struct F32ToF16 {
  using In = float; using Out = uint16_t;
  static __device__ __forceinline__ uint16_t cvt(float v) {
    return f32_to_f16(v);
  }
};
struct Bf16ToF16 {
  using In = uint16_t; using Out = uint16_t;
  static __device__ __forceinline__ uint16_t cvt(uint16_t v) {
    return f32_to_f16(bf16_to_f32(v));
  }
};
struct F16ToBf16 {
  using In = uint16_t; using Out = uint16_t;
  static __device__ __forceinline__ uint16_t cvt(uint16_t v) {
    return f32_to_bf16(f16_to_f32(v));
  }
};

// ---------------------------------------------------------------------------
// elementwise cast, 8 elements per lane, 16B loads where possible (G13)
// ---------------------------------------------------------------------------

template <typename CVT, int UNROLL = 2>
__global__ void cast_kernel(const typename CVT::In* __restrict__ in,
                            typename CVT::Out* __restrict__ out,
                            int64_t n) {
  using In = typename CVT::In;
  using Out = typename CVT::Out;
  constexpr int VC = 16 / sizeof(In);      // elements per 16B chunk
  constexpr int V = VC * UNROLL;           // elements per lane per iter
  int64_t i0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * V;
  int64_t stride = int64_t(gridDim.x) * blockDim.x * V;
  for (int64_t i = i0; i < n; i += stride) {
    if (i + V <= n) {
      In vin[V];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        reinterpret_cast<int4*>(vin)[u] =
            reinterpret_cast<const int4*>(in + i)[u];
      Out vout[V];
#pragma unroll
      for (int k = 0; k < V; ++k) vout[k] = CVT::cvt(vin[k]);
      constexpr int OUTB = int(sizeof(Out)) * V;
      if constexpr (OUTB % 16 == 0) {
#pragma unroll
        for (int u = 0; u < OUTB / 16; ++u)
          reinterpret_cast<int4*>(out + i)[u] =
              reinterpret_cast<const int4*>(vout)[u];
      } else {  // 8-byte tail width (16B in -> 8B out, UNROLL=1)
        *reinterpret_cast<int2*>(out + i) =
            *reinterpret_cast<const int2*>(vout);
      }
    } else {
      for (int64_t k = i; k < n; ++k) out[k] = CVT::cvt(in[k]);
    }
  }
}

// ---------------------------------------------------------------------------
// fused NCHW->NHWC + cast
// ---------------------------------------------------------------------------
// Small-C specialization (the image case C=3), C a COMPILE-TIME constant so
// the interleave indexing is fully static (a runtime-C variant measured 2.7x
// slower: indexed vout[k*C+c] stores de-vectorize). Each lane owns HWPL
// consecutive hw positions and all C channels: per-channel reads are 16 B
// vector loads (G13), each lane writes HWPL*C consecutive outputs ->
// coalesced wide stores. The interior fast path is branch-free; the ragged
// tail (hw0+HWPL > HW) takes a scalar path.
template <typename CVT, int C, int HWPL>
__global__ void nchw_nhwc_smallc_kernel(
    const typename CVT::In* __restrict__ in,
    typename CVT::Out* __restrict__ out,
    int64_t HW, int64_t N) {
  using In = typename CVT::In;
  using Out = typename CVT::Out;
  const int64_t hw_chunks = (HW + HWPL - 1) / HWPL;
  int64_t idx0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t idx = idx0; idx < N * hw_chunks; idx += stride) {
    const int64_t nimg = idx / hw_chunks;
    const int64_t hw0 = (idx - nimg * hw_chunks) * HWPL;
    const In* src0 = in + nimg * C * HW + hw0;
    Out* dst = out + nimg * HW * C + hw0 * C;
    if (hw0 + HWPL <= HW &&
        (sizeof(In) * HWPL % 16 == 0) &&
        (reinterpret_cast<uintptr_t>(src0) & 15) == 0 &&
        (HW * sizeof(In)) % 16 == 0 &&
        (reinterpret_cast<uintptr_t>(dst) & 15) == 0 &&
        (sizeof(Out) * HWPL * C) % 16 == 0) {
      // fast path: all-vector loads and stores, no predication
      In vin[C][HWPL];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        constexpr int NV = int(sizeof(In) * HWPL / 16) ? int(sizeof(In) * HWPL / 16) : 1;
#pragma unroll
        for (int v = 0; v < NV; ++v)
          reinterpret_cast<int4*>(vin[c])[v] =
              reinterpret_cast<const int4*>(src0 + c * HW)[v];
      }
      Out vout[HWPL * C];
#pragma unroll
      for (int k = 0; k < HWPL; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c)
          vout[k * C + c] = CVT::cvt(vin[c][k]);
      constexpr int NSV = int(sizeof(Out) * HWPL * C / 16);
#pragma unroll
      for (int v = 0; v < NSV; ++v)
        reinterpret_cast<int4*>(dst)[v] =
            *reinterpret_cast<const int4*>(vout + v * (16 / sizeof(Out)));
    } else {
      const int span = int(min(int64_t(HWPL), HW - hw0));
      for (int k = 0; k < span; ++k)
        for (int c = 0; c < C; ++c)
          dst[k * C + c] = CVT::cvt(src0[c * HW + k]);
    }
  }
}

// Inverse direction (NHWC -> NCHW), small compile-time C: each lane reads
// HWPL*C contiguous inputs (vector loads) and writes HWPL consecutive
// elements into each of C channel streams (vector stores per channel).
template <typename CVT, int C, int HWPL>
__global__ void nhwc_nchw_smallc_kernel(
    const typename CVT::In* __restrict__ in,
    typename CVT::Out* __restrict__ out,
    int64_t HW, int64_t N) {
  using In = typename CVT::In;
  using Out = typename CVT::Out;
  const int64_t hw_chunks = (HW + HWPL - 1) / HWPL;
  int64_t idx0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t idx = idx0; idx < N * hw_chunks; idx += stride) {
    const int64_t nimg = idx / hw_chunks;
    const int64_t hw0 = (idx - nimg * hw_chunks) * HWPL;
    const In* src = in + nimg * HW * C + hw0 * C;
    Out* dst0 = out + nimg * C * HW + hw0;
    if (hw0 + HWPL <= HW &&
        (sizeof(In) * HWPL * C) % 16 == 0 &&
        (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
        (sizeof(Out) * HWPL) % 16 == 0 &&
        (reinterpret_cast<uintptr_t>(dst0) & 15) == 0 &&
        (HW * sizeof(Out)) % 16 == 0) {
      In vin[HWPL * C];
      constexpr int NLV = int(sizeof(In) * HWPL * C / 16);
#pragma unroll
      for (int v = 0; v < NLV; ++v)
        reinterpret_cast<int4*>(vin)[v] =
            reinterpret_cast<const int4*>(src)[v];
      Out vout[C][HWPL];
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < HWPL; ++k)
          vout[c][k] = CVT::cvt(vin[k * C + c]);
      constexpr int NSV = int(sizeof(Out) * HWPL / 16);
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int v = 0; v < NSV; ++v)
          reinterpret_cast<int4*>(dst0 + c * HW)[v] =
              *reinterpret_cast<const int4*>(&vout[c][v * (16 / sizeof(Out))]);
    } else {
      const int span = int(min(int64_t(HWPL), HW - hw0));
      for (int k = 0; k < span; ++k)
        for (int c = 0; c < C; ++c)
          dst0[c * HW + k] = CVT::cvt(src[k * C + c]);
    }
  }
}

// Runtime-C fallback for 5..8 channels (4 hw per lane).
template <typename CVT, int MAXC>
__global__ void nchw_nhwc_midc_kernel(
    const typename CVT::In* __restrict__ in,
    typename CVT::Out* __restrict__ out,
    int C, int64_t HW, int64_t N) {
  using Out = typename CVT::Out;
  const int64_t hw_quads = (HW + 3) / 4;
  int64_t idx0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t idx = idx0; idx < N * hw_quads; idx += stride) {
    const int64_t nimg = idx / hw_quads;
    const int64_t hw0 = (idx - nimg * hw_quads) * 4;
    const int64_t in_base = nimg * C * HW;
    const int64_t out_base = nimg * HW * C;
    Out vout[4 * MAXC];
    const int span = int(min(int64_t(4), HW - hw0));
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c >= C) break;
      for (int k = 0; k < span; ++k)
        vout[k * C + c] = CVT::cvt(in[in_base + c * HW + hw0 + k]);
    }
    Out* dst = out + out_base + hw0 * C;
    const int total = span * C;
    int k = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
      constexpr int perv = 16 / sizeof(Out);
      for (; k + perv <= total; k += perv)
        *reinterpret_cast<int4*>(dst + k) =
            *reinterpret_cast<const int4*>(vout + k);
    }
    for (; k < total; ++k) dst[k] = vout[k];
  }
}

// Generic case: batched [C, HW] -> [HW, C] transpose through LDS,
// 64x64 tiles, 256 threads, +1-element row padding so b32 accesses are
// bank-conflict-free (G4: modulus 32 for 4B accesses).
template <typename CVT>
__global__ void nchw_nhwc_tiled_kernel(
    const typename CVT::In* __restrict__ in,
    typename CVT::Out* __restrict__ out,
    int64_t C, int64_t HW, int64_t N) {
  using Out = typename CVT::Out;
  constexpr int TILE = 64;
  __shared__ Out lds[TILE][TILE + 1];
  // grid: x = HW tiles, y = C tiles, z = batch
  const int64_t hw_t = int64_t(blockIdx.x) * TILE;
  const int64_t c_t = int64_t(blockIdx.y) * TILE;
  const int64_t nimg = blockIdx.z;
  const typename CVT::In* src = in + nimg * C * HW;
  Out* dst = out + nimg * HW * C;
  // load 64x64 input tile: rows = C dim, cols = HW dim (coalesced on HW)
  // 256 threads = 4 rows of 64 lanes; each thread loads 16 rows strided.
  const int lane = threadIdx.x & 63;
  const int row0 = threadIdx.x >> 6;  // 0..3
#pragma unroll
  for (int r = 0; r < TILE; r += 4) {
    const int64_t c = c_t + row0 + r;
    const int64_t hw = hw_t + lane;
    if (c < C && hw < HW) {
      lds[row0 + r][lane] = CVT::cvt(src[c * HW + hw]);
    }
  }
  __syncthreads();
  // store transposed: rows = HW dim, cols = C dim (coalesced on C)
#pragma unroll
  for (int r = 0; r < TILE; r += 4) {
    const int64_t hw = hw_t + row0 + r;
    const int64_t c = c_t + lane;
    if (hw < HW && c < C) {
      dst[hw * C + c] = lds[lane][row0 + r];
    }
  }
}

// ---------------------------------------------------------------------------
// int8 affine quantize / dequantize
// ---------------------------------------------------------------------------

// Quantize semantics (pinned, test-verified): q = clamp(rne(x * inv_scale
// + zp)) with inv_scale = float(1.0/scale) and EXPLICITLY unfused mul/add
// (__fmul_rn/__fadd_rn) — torch's scalar division also multiplies by the
// reciprocal, and an fma contraction flips rare half-way ties.
__global__ void quantize_q8_kernel(const float* __restrict__ in,
                                   int8_t* __restrict__ out, int64_t n,
                                   float inv_scale, float zero_point) {
  int64_t i0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 4;
  int64_t stride = int64_t(gridDim.x) * blockDim.x * 4;
  for (int64_t i = i0; i < n; i += stride) {
    if (i + 4 <= n) {
      float4 v = *reinterpret_cast<const float4*>(in + i);
      char4 q;
      q.x = int8_t(max(-128.f, min(127.f, nearbyintf(__fadd_rn(__fmul_rn(v.x, inv_scale), zero_point)))));
      q.y = int8_t(max(-128.f, min(127.f, nearbyintf(__fadd_rn(__fmul_rn(v.y, inv_scale), zero_point)))));
      q.z = int8_t(max(-128.f, min(127.f, nearbyintf(__fadd_rn(__fmul_rn(v.z, inv_scale), zero_point)))));
      q.w = int8_t(max(-128.f, min(127.f, nearbyintf(__fadd_rn(__fmul_rn(v.w, inv_scale), zero_point)))));
      *reinterpret_cast<char4*>(out + i) = q;
    } else {
      for (int64_t k = i; k < n; ++k) {
        float q = nearbyintf(__fadd_rn(__fmul_rn(in[k], inv_scale), zero_point));
        out[k] = int8_t(max(-128.f, min(127.f, q)));
      }
    }
  }
}

__global__ void dequantize_q8_kernel(const int8_t* __restrict__ in,
                                     float* __restrict__ out, int64_t n,
                                     float scale, float zero_point) {
  int64_t i0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 4;
  int64_t stride = int64_t(gridDim.x) * blockDim.x * 4;
  for (int64_t i = i0; i < n; i += stride) {
    if (i + 4 <= n) {
      char4 q = *reinterpret_cast<const char4*>(in + i);
      float4 v;
      v.x = (float(q.x) - zero_point) * scale;
      v.y = (float(q.y) - zero_point) * scale;
      v.z = (float(q.z) - zero_point) * scale;
      v.w = (float(q.w) - zero_point) * scale;
      *reinterpret_cast<float4*>(out + i) = v;
    } else {
      for (int64_t k = i; k < n; ++k)
        out[k] = (float(in[k]) - zero_point) * scale;
    }
  }
}

// ---------------------------------------------------------------------------
// fused uint8 image ingest: dequantize + per-channel normalize (+ NCHW)
// ---------------------------------------------------------------------------
// y = round_to(Out, fadd_rn(fmul_rn(float(x), scale_c), bias_c)) for uint8
// NHWC input, written NCHW or NHWC. Semantics are pinned bit-exact to the
// eager torch chain (float() * scale + bias).to(out): the multiply and add
// stay UNFUSED (__fmul_rn/__fadd_rn, see quantize_q8_kernel) and bytes are
// unsigned.
//
// Same shape as nhwc_nchw_smallc_kernel: C is compile-time, each lane owns
// HWPL consecutive pixels, reads their HWPL*C contiguous bytes with vector
// loads, converts in registers (shift+mask+float() selects
// v_cvt_f32_ubyte0..3) and writes 16 B vectors — HWPL consecutive outputs
// into each channel plane (NCHW) or one contiguous run (NHWC). scale/bias
// ride in the kernel-argument segment: no device allocation or H2D per call.
// Loads are 16 B wide when HWPL*C is a multiple of 16, else 8 B (HWPL=8 with
// odd C: consecutive chunks are 8 B apart mod 16, so 16 B loads cannot be
// aligned). The fast path needs the source aligned to the load width, the
// destination to 16 B and, for NCHW, a plane stride that keeps every plane
// 16 B-aligned; anything else, and the ragged tail, goes scalar.
struct U8NormParams {
  float scale[4];
  float bias[4];
};

template <typename CVT, int C, int HWPL, bool NCHW>
__global__ void u8_nhwc_normalize_kernel(
    const uint8_t* __restrict__ in,
    typename CVT::Out* __restrict__ out,
    int64_t HW, int64_t N, U8NormParams p) {
  using Out = typename CVT::Out;
  constexpr int LB = HWPL * C;                  // input bytes per lane
  constexpr int LV = (LB % 16 == 0) ? 16 : 8;   // load vector width, bytes
  constexpr int PERV = 16 / int(sizeof(Out));   // outputs per 16 B store
  static_assert(LB % LV == 0, "HWPL*C must be a multiple of 8 bytes");
  static_assert(HWPL % PERV == 0, "HWPL must fill whole 16 B stores");
  const int64_t hw_chunks = (HW + HWPL - 1) / HWPL;
  int64_t idx0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t idx = idx0; idx < N * hw_chunks; idx += stride) {
    const int64_t nimg = idx / hw_chunks;
    const int64_t hw0 = (idx - nimg * hw_chunks) * HWPL;
    const uint8_t* src = in + (nimg * HW + hw0) * C;
    Out* dst = NCHW ? out + nimg * C * HW + hw0
                    : out + (nimg * HW + hw0) * C;
    if (hw0 + HWPL <= HW &&
        (reinterpret_cast<uintptr_t>(src) & (LV - 1)) == 0 &&
        (reinterpret_cast<uintptr_t>(dst) & 15) == 0 &&
        (!NCHW || (HW * sizeof(Out)) % 16 == 0)) {
      uint32_t w[LB / 4];
      if constexpr (LV == 16) {
#pragma unroll
        for (int v = 0; v < LB / 16; ++v)
          reinterpret_cast<int4*>(w)[v] =
              reinterpret_cast<const int4*>(src)[v];
      } else {
#pragma unroll
        for (int v = 0; v < LB / 8; ++v)
          reinterpret_cast<int2*>(w)[v] =
              reinterpret_cast<const int2*>(src)[v];
      }
      if constexpr (NCHW) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
          for (int v = 0; v < HWPL / PERV; ++v) {
            Out vout[PERV];
#pragma unroll
            for (int e = 0; e < PERV; ++e) {
              const int j = (v * PERV + e) * C + c;   // byte index, static
              const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
              vout[e] = CVT::cvt(__fadd_rn(__fmul_rn(float(b), p.scale[c]),
                                           p.bias[c]));
            }
            reinterpret_cast<int4*>(dst + c * HW)[v] =
                *reinterpret_cast<const int4*>(vout);
          }
        }
      } else {
#pragma unroll
        for (int v = 0; v < LB / PERV; ++v) {
          Out vout[PERV];
#pragma unroll
          for (int e = 0; e < PERV; ++e) {
            const int j = v * PERV + e;               // byte index, static
            const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
            vout[e] = CVT::cvt(__fadd_rn(__fmul_rn(float(b), p.scale[j % C]),
                                         p.bias[j % C]));
          }
          reinterpret_cast<int4*>(dst)[v] =
              *reinterpret_cast<const int4*>(vout);
        }
      }
    } else {
      // ragged tail, or a misaligned source/destination/plane stride
      const int span = int(min(int64_t(HWPL), HW - hw0));
      for (int k = 0; k < span; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const Out y = CVT::cvt(__fadd_rn(
              __fmul_rn(float(src[k * C + c]), p.scale[c]), p.bias[c]));
          if constexpr (NCHW) dst[c * HW + k] = y;
          else dst[k * C + c] = y;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// fused uint8 image ingest with bilinear resize + crop
// ---------------------------------------------------------------------------
// uint8 NHWC [N,Hin,Win,C] -> [N,C,Hc,Wc] (or [N,Hc,Wc,C]): half-pixel-centre
// bilinear resize to a virtual (Hr,Wr) image, a crop window of it, then the
// same normalize + cast as u8_nhwc_normalize_kernel. Every step is one IEEE
// fp32 operation, nothing contracted (ox is the output column, rw =
// float(Win/Wr) rounded once on the host; rows likewise with top, rh, Hin):
//
//   sx = max(fsub(fmul(fadd(float(ox + left), 0.5), rw), 0.5), 0)
//   x0 = min(int(floor(sx)), Win-1)   x1 = min(x0+1, Win-1)
//   wx = fsub(sx, float(x0))
//   t  = p[y0,x0] + wx * (p[y0,x1] - p[y0,x0])      b likewise on row y1
//   v  = t + wy * (b - t)
//   y  = Out(fadd(fmul(v, scale_c), bias_c))
//
// With (Hr,Wr) == (Hin,Win) the weights are exactly 0 and the result is
// bit-identical to u8_nhwc_normalize_kernel.
//
// Shape of the kernel. A 256-thread workgroup owns a tile of the output:
// 2^twl_log2 lane runs wide and 256 >> twl_log2 rows high; a lane owns a run
// of kResizePx = 8 consecutive output columns of one output row and writes
// them with 16 B stores, one vector run per channel plane (NCHW) or one
// contiguous run (NHWC). A work item is (image, row tile, column tile);
// workgroups grid-stride over work items under the usual grid cap.
//
// Source taps, two paths, chosen per work item (uniform in the workgroup):
//  * LDS path: every output row of the tile needs source rows y0 and y1 over
//    the same contiguous column span [x0(first column), x1(last column)].
//    The workgroup copies those 2 * rows spans into LDS with 16 B-aligned
//    16 B global loads (each span keeps its own misalignment `shift`, so the
//    loads are aligned whatever the row base is; a 16 B chunk that is not
//    wholly inside the tensor is read bytewise, in bounds) and the lanes
//    gather their taps from LDS.
//  * direct path: taps are byte loads from global memory. Taken when the
//    host found that the tile's spans exceed kResizeLdsBytes (span_stride ==
//    0: large downscale ratios), or when a tile's span does not fit the span
//    stride the host estimated.
// Stores go scalar for a run that crosses the row end and when the
// destination, or for NCHW the plane stride, is not 16 B-aligned.
constexpr int kResizeBlock = 256;
constexpr int kResizePx = 8;             // output columns per lane
constexpr int kResizeLdsBytes = 32768;
constexpr int kResizeMinTwlLog2 = 3;     // tile: 8 runs x 32 rows ...
constexpr int kResizeMaxTwlLog2 = 5;     // ... to 32 runs (256 columns) x 8

struct U8ResizeParams {
  float scale[4];
  float bias[4];
  float rh, rw;
  int Hin, Win, Hc, Wc, top, left;
  int twl_log2;      // lane runs per tile row, log2
  int tiles_x, tiles_y;
  int span_stride;   // LDS bytes per source-row span (multiple of 16), 0: direct
};

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

// Store one lane's run: the first min(kResizePx, Wc - ox0) columns of vout
// (NCHW: [c][k], NHWC: [k][c]) to `dst`, the run's first output element.
template <typename Out, int C, bool NCHW>
__device__ __forceinline__ void resize_store_run(
    const Out (&vout)[C * kResizePx], int ox0, int Wc,
    Out* __restrict__ dst, int64_t plane) {
  constexpr int PERV = 16 / int(sizeof(Out));
  const bool vec = ox0 + kResizePx <= Wc &&
                   (reinterpret_cast<uintptr_t>(dst) & 15) == 0 &&
                   (!NCHW || (plane * int64_t(sizeof(Out))) % 16 == 0);
  if (vec) {
    if constexpr (NCHW) {
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int v = 0; v < kResizePx / PERV; ++v)
          reinterpret_cast<int4*>(dst + c * plane)[v] =
              *reinterpret_cast<const int4*>(vout + c * kResizePx + v * PERV);
    } else {
#pragma unroll
      for (int v = 0; v < C * kResizePx / PERV; ++v)
        reinterpret_cast<int4*>(dst)[v] =
            *reinterpret_cast<const int4*>(vout + v * PERV);
    }
  } else {
    const int span = min(kResizePx, Wc - ox0);
#pragma unroll
    for (int k = 0; k < kResizePx; ++k) {
      if (k < span) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if constexpr (NCHW) dst[c * plane + k] = vout[c * kResizePx + k];
          else dst[k * C + c] = vout[k * C + c];
        }
      }
    }
  }
}

// One lane's run: kResizePx output columns from ox0 of one output row. r0/r1
// point at column `xb` of source rows y0/y1: global memory with xb = 0, or
// the LDS image of the tile's span with xb = its first column.
template <typename CVT, int C, bool NCHW, typename Ptr>
__device__ __forceinline__ void resize_run(
    Ptr r0, Ptr r1, int xb, float wy, int ox0,
    typename CVT::Out* __restrict__ dst, int64_t plane,
    const U8ResizeParams& p) {
  using Out = typename CVT::Out;
  Out vout[C * kResizePx];   // NCHW: [c][k], NHWC: [k][c]
#pragma unroll
  for (int k = 0; k < kResizePx; ++k) {
    // a run that crosses the row end computes its last column again; the
    // duplicates are never stored
    const int ox = min(ox0 + k, p.Wc - 1);
    int x0, x1;
    float wx;
    resize_tap(ox, p.left, p.rw, p.Win, x0, x1, wx);
    const int b0 = (x0 - xb) * C, b1 = (x1 - xb) * C;   // both >= 0
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float p00 = float(r0[b0 + c]);
      const float p01 = float(r0[b1 + c]);
      const float p10 = float(r1[b0 + c]);
      const float p11 = float(r1[b1 + c]);
      const float t = __fadd_rn(p00, __fmul_rn(wx, __fsub_rn(p01, p00)));
      const float b = __fadd_rn(p10, __fmul_rn(wx, __fsub_rn(p11, p10)));
      const float v = __fadd_rn(t, __fmul_rn(wy, __fsub_rn(b, t)));
      vout[NCHW ? c * kResizePx + k : k * C + c] =
          CVT::cvt(__fadd_rn(__fmul_rn(v, p.scale[c]), p.bias[c]));
    }
  }
  resize_store_run<Out, C, NCHW>(vout, ox0, p.Wc, dst, plane);
}

template <typename CVT, int C, bool NCHW>
__global__ void __launch_bounds__(kResizeBlock) u8_nhwc_resize_normalize_kernel(
    const uint8_t* __restrict__ in, typename CVT::Out* __restrict__ out,
    int64_t N, U8ResizeParams p) {
  using Out = typename CVT::Out;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kResizeLdsBytes];
  static_assert(kResizePx % (16 / int(sizeof(Out))) == 0,
                "a lane run must fill whole 16 B stores");
  const int twl = 1 << p.twl_log2;               // lane runs per tile row
  const int tr = kResizeBlock >> p.twl_log2;     // rows per tile
  const int tw = twl * kResizePx;                // columns per tile
  const int r = int(threadIdx.x) >> p.twl_log2;
  const int j = int(threadIdx.x) & (twl - 1);
  const int64_t plane = int64_t(p.Hc) * p.Wc;
  const int64_t row_bytes = int64_t(p.Win) * C;
  const uint8_t* const in_end = in + N * p.Hin * row_bytes;
  const int64_t items = N * p.tiles_y * p.tiles_x;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int tx = int(item % p.tiles_x);
    const int ty = int((item / p.tiles_x) % p.tiles_y);
    const int64_t n = item / (int64_t(p.tiles_x) * p.tiles_y);
    const uint8_t* img = in + n * p.Hin * row_bytes;
    const int oy = ty * tr + r;
    const int ox0 = tx * tw + j * kResizePx;
    const bool active = oy < p.Hc && ox0 < p.Wc;

    // source column span of the tile, the same for every row of it
    int xs_lo, xs_hi, unused;
    float unused_w;
    resize_tap(tx * tw, p.left, p.rw, p.Win, xs_lo, unused, unused_w);
    resize_tap(min(tx * tw + tw, p.Wc) - 1, p.left, p.rw, p.Win, unused,
               xs_hi, unused_w);
    const int span_bytes = (xs_hi + 1 - xs_lo) * C;
    // uniform in the workgroup: the barriers below are not divergent
    const bool use_lds = p.span_stride > 0 && span_bytes + 15 <= p.span_stride;

    int y0 = 0, y1 = 0;
    float wy = 0.f;
    if (active) resize_tap(oy, p.top, p.rh, p.Hin, y0, y1, wy);
    Out* dst = NCHW
        ? out + (n * C * p.Hc + oy) * p.Wc + ox0
        : out + ((n * p.Hc + oy) * p.Wc + ox0) * C;

    if (use_lds) {
      const int nchunks = p.span_stride >> 4;
      const int rows_here = min(tr, p.Hc - ty * tr);
      const int total = 2 * rows_here * nchunks;
      for (int idx = int(threadIdx.x); idx < total; idx += kResizeBlock) {
        const int s = idx / nchunks;           // span: tile row s>>1, y(s&1)
        const int k = idx - s * nchunks;
        int sy0, sy1;
        float sw;
        resize_tap(ty * tr + (s >> 1), p.top, p.rh, p.Hin, sy0, sy1, sw);
        const uint8_t* a0 =
            img + ((s & 1) ? sy1 : sy0) * row_bytes + int64_t(xs_lo) * C;
        const uint8_t* a_end = a0 + span_bytes;
        const uint8_t* ca =
            a0 - (reinterpret_cast<uintptr_t>(a0) & 15) + int64_t(k) * 16;
        if (ca >= a_end) continue;
        uint8_t* l = lds + s * p.span_stride + k * 16;
        if (ca >= in && ca + 16 <= in_end) {
          *reinterpret_cast<int4*>(l) = *reinterpret_cast<const int4*>(ca);
        } else {
          // the first or last chunk of the tensor: stay inside it
          for (int b = 0; b < 16; ++b)
            l[b] = (ca + b >= a0 && ca + b < a_end) ? ca[b] : uint8_t(0);
        }
      }
      __syncthreads();
      if (active) {
        const uint8_t* g0 = img + y0 * row_bytes + int64_t(xs_lo) * C;
        const uint8_t* g1 = img + y1 * row_bytes + int64_t(xs_lo) * C;
        const int shift0 = int(reinterpret_cast<uintptr_t>(g0) & 15);
        const int shift1 = int(reinterpret_cast<uintptr_t>(g1) & 15);
        const uint8_t* l0 = lds + (2 * r) * p.span_stride + shift0;
        const uint8_t* l1 = lds + (2 * r + 1) * p.span_stride + shift1;
        resize_run<CVT, C, NCHW>(l0, l1, xs_lo, wy, ox0, dst, plane, p);
      }
      __syncthreads();   // lds is refilled by the next work item
    } else if (active) {
      resize_run<CVT, C, NCHW>(img + y0 * row_bytes, img + y1 * row_bytes, 0,
                               wy, ox0, dst, plane, p);
    }
  }
}

// ---------------------------------------------------------------------------
// ragged batch: N images of N different sizes, one launch
// ---------------------------------------------------------------------------
// The same resize + crop + normalize as above, bit for bit (resize_tap,
// resize_run and resize_store_run are shared), for images that lie back to
// back in one flat uint8 buffer, HWC each, no padding, so an image starts at
// any byte alignment. The output size (Hc,Wc) is shared: tile geometry, work
// item decomposition and the store path are those of the dense kernel. Only
// the source side differs per image and comes from a table in device memory,
// one entry per image, built by the host (ops.image_u8_ragged_resize_to_float
// ships it as int32 [N,8]; the int64 is two little-endian words).
//
// The tap path is chosen per work item from the item's own span (uniform in
// the workgroup), so one launch mixes LDS items and direct-gather items. The
// in-bounds test of the aligned 16 B chunk loads uses the bounds of the whole
// flat buffer: a chunk may bring a neighbouring image's bytes into LDS, which
// no tap ever reads. The host guarantees that every image lies inside the
// buffer (sum of H*W*C == buffer bytes).
struct U8RaggedEntry {
  int64_t offset;    // first byte of the image in the flat buffer
  int Hin, Win, top, left;
  float rh, rw;
};
static_assert(sizeof(U8RaggedEntry) == 32, "table rows are int32 [8]");

template <typename CVT, int C, bool NCHW>
__global__ void __launch_bounds__(kResizeBlock)
u8_ragged_resize_normalize_kernel(
    const uint8_t* __restrict__ in, int64_t in_bytes,
    const U8RaggedEntry* __restrict__ table,
    typename CVT::Out* __restrict__ out, int64_t N, U8ResizeParams p) {
  using Out = typename CVT::Out;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kResizeLdsBytes];
  static_assert(kResizePx % (16 / int(sizeof(Out))) == 0,
                "a lane run must fill whole 16 B stores");
  const int twl = 1 << p.twl_log2;               // lane runs per tile row
  const int tr = kResizeBlock >> p.twl_log2;     // rows per tile
  const int tw = twl * kResizePx;                // columns per tile
  const int r = int(threadIdx.x) >> p.twl_log2;
  const int j = int(threadIdx.x) & (twl - 1);
  const int64_t plane = int64_t(p.Hc) * p.Wc;
  const uint8_t* const in_end = in + in_bytes;
  const int64_t items = N * p.tiles_y * p.tiles_x;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int tx = int(item % p.tiles_x);
    const int ty = int((item / p.tiles_x) % p.tiles_y);
    const int64_t n = item / (int64_t(p.tiles_x) * p.tiles_y);
    // the source side of this item's image; everything else is shared
    const U8RaggedEntry e = table[n];
    U8ResizeParams q = p;
    q.Hin = e.Hin; q.Win = e.Win;
    q.top = e.top; q.left = e.left;
    q.rh = e.rh; q.rw = e.rw;
    const int64_t row_bytes = int64_t(q.Win) * C;
    const uint8_t* img = in + e.offset;
    const int oy = ty * tr + r;
    const int ox0 = tx * tw + j * kResizePx;
    const bool active = oy < q.Hc && ox0 < q.Wc;

    // source column span of the tile, the same for every row of it
    int xs_lo, xs_hi, unused;
    float unused_w;
    resize_tap(tx * tw, q.left, q.rw, q.Win, xs_lo, unused, unused_w);
    resize_tap(min(tx * tw + tw, q.Wc) - 1, q.left, q.rw, q.Win, unused,
               xs_hi, unused_w);
    const int span_bytes = (xs_hi + 1 - xs_lo) * C;
    // LDS bytes per source-row span: the span plus up to 15 bytes of
    // misalignment, in whole 16 B chunks. Uniform in the workgroup: the
    // barriers below are not divergent.
    const int span_stride = (span_bytes + 15 + 15) & ~15;
    const bool use_lds = 2 * tr * span_stride <= kResizeLdsBytes;

    int y0 = 0, y1 = 0;
    float wy = 0.f;
    if (active) resize_tap(oy, q.top, q.rh, q.Hin, y0, y1, wy);
    Out* dst = NCHW
        ? out + (n * C * q.Hc + oy) * q.Wc + ox0
        : out + ((n * q.Hc + oy) * q.Wc + ox0) * C;

    if (use_lds) {
      const int nchunks = span_stride >> 4;
      const int rows_here = min(tr, q.Hc - ty * tr);
      const int total = 2 * rows_here * nchunks;
      for (int idx = int(threadIdx.x); idx < total; idx += kResizeBlock) {
        const int s = idx / nchunks;           // span: tile row s>>1, y(s&1)
        const int k = idx - s * nchunks;
        int sy0, sy1;
        float sw;
        resize_tap(ty * tr + (s >> 1), q.top, q.rh, q.Hin, sy0, sy1, sw);
        const uint8_t* a0 =
            img + ((s & 1) ? sy1 : sy0) * row_bytes + int64_t(xs_lo) * C;
        const uint8_t* a_end = a0 + span_bytes;
        const uint8_t* ca =
            a0 - (reinterpret_cast<uintptr_t>(a0) & 15) + int64_t(k) * 16;
        if (ca >= a_end) continue;
        uint8_t* l = lds + s * span_stride + k * 16;
        if (ca >= in && ca + 16 <= in_end) {
          *reinterpret_cast<int4*>(l) = *reinterpret_cast<const int4*>(ca);
        } else {
          // the first or last chunk of the flat buffer: stay inside it
          for (int b = 0; b < 16; ++b)
            l[b] = (ca + b >= a0 && ca + b < a_end) ? ca[b] : uint8_t(0);
        }
      }
      __syncthreads();
      if (active) {
        const uint8_t* g0 = img + y0 * row_bytes + int64_t(xs_lo) * C;
        const uint8_t* g1 = img + y1 * row_bytes + int64_t(xs_lo) * C;
        const int shift0 = int(reinterpret_cast<uintptr_t>(g0) & 15);
        const int shift1 = int(reinterpret_cast<uintptr_t>(g1) & 15);
        const uint8_t* l0 = lds + (2 * r) * span_stride + shift0;
        const uint8_t* l1 = lds + (2 * r + 1) * span_stride + shift1;
        resize_run<CVT, C, NCHW>(l0, l1, xs_lo, wy, ox0, dst, plane, q);
      }
      __syncthreads();   // lds is refilled by the next work item
    } else if (active) {
      resize_run<CVT, C, NCHW>(img + y0 * row_bytes, img + y1 * row_bytes, 0,
                               wy, ox0, dst, plane, q);
    }
  }
}

// ---------------------------------------------------------------------------
// YUV 4:2:0 source side (NV12 / I420) of the bilinear resize + crop ingest
// ---------------------------------------------------------------------------
// One frame is Hin*3/2 rows of Win bytes, Hin and Win even: the Y plane
// (Hin*Win bytes), then NV12: Hin/2 rows of Win/2 interleaved (U,V) pairs, or
// I420: the U plane of (Hin/2)*(Win/2) flat bytes, then the V plane. Frames
// lie back to back. Luma pixel (y,x) uses chroma sample (y>>1, x>>1), and is
// converted in int32 (coefficients in Yuv420Coef, three matrices on the host):
//
//   C = Y - yoff   D = U - 128   E = V - 128
//   R = clamp((yc*C        + rv*E + 128) >> 8, 0, 255)
//   G = clamp((yc*C + gu*D + gv*E + 128) >> 8, 0, 255)
//   B = clamp((yc*C + bu*D        + 128) >> 8, 0, 255)
//
// A negative sum clamps to 0 however the shift rounds. Every bilinear tap is
// that clamped uint8 value; everything after it is resize_run, unchanged, so
// the result is bit-identical to u8_nhwc_resize_normalize_kernel<CVT,3,NCHW>
// on the converted RGB tensor, which never exists in memory.
//
// Tile geometry, work items, the grid-stride loop and the store path are those
// of the RGB kernel. The tap paths:
//  * LDS path: the workgroup converts while it fills. An LDS span holds the
//    RGB bytes (3 per pixel) of one source row from column xe = xs_lo & ~1, so
//    a 16-pixel fill chunk starts at an even column and never splits a chroma
//    pair. A chunk is one 16 B luma load and 16 B (NV12) or 2 x 8 B (I420) of
//    chroma, converted in registers and written as three 16 B LDS stores.
//    Luma and chroma of a chunk have unrelated alignments (odd row strides,
//    odd plane bases, any storage offset), so the global loads are unaligned
//    vector loads (memcpy); a chunk whose loads would pass the end of the
//    tensor is read bytewise, in bounds. Loads may run past the span or the
//    row end into bytes of the same tensor that no tap reads.
//  * direct path: Yuv420Row converts per tap from global memory. Taken when
//    the host found that the tile's spans exceed kResizeLdsBytes (span_px ==
//    0), or when a tile's span does not fit the estimate.
struct Yuv420Coef {
  int yoff, yc, rv, gu, gv, bu;
};

struct Yuv420ResizeParams {
  U8ResizeParams r;   // span_stride: LDS bytes per span, 48 per fill chunk
  Yuv420Coef k;
  int span_px;        // pixels per LDS span (multiple of 16), 0: direct
};

constexpr int kYuvChunkPx = 16;

// clamp(v >> 8, 0, 255), written clamp first: the same value for every v.
// The shift-then-clamp form is selected as v_ashr_pk_u8_i32 for pairs of
// values by hipcc (ROCm 7.2), and the packed bytes came out wrong on MI355X.
__device__ __forceinline__ uint32_t yuv_clamp8(int v) {
  return uint32_t(min(max(v, 0), 0xffff)) >> 8;
}

// One source row in global memory. `u`/`v` point at the row's first chroma
// sample, `cstep` bytes apart (NV12: 2 with v = u + 1; I420: 1).
struct Yuv420Row {
  const uint8_t* y;
  const uint8_t* u;
  const uint8_t* v;
  int cstep;
  // the converted pixel x as floats, ready to blend
  __device__ __forceinline__ void rgb(int x, const Yuv420Coef& k,
                                      float (&o)[3]) const {
    const int co = (x >> 1) * cstep;
    const int base = k.yc * (int(y[x]) - k.yoff) + 128;
    const int D = int(u[co]) - 128, E = int(v[co]) - 128;
    o[0] = float(yuv_clamp8(base + k.rv * E));
    o[1] = float(yuv_clamp8(base + k.gu * D + k.gv * E));
    o[2] = float(yuv_clamp8(base + k.bu * D));
  }
};

// resize_run for the direct path: the same fp32 operations in the same order,
// on taps that are fetched through Yuv420Row and converted once per pixel.
template <typename CVT, bool NCHW>
__device__ __forceinline__ void yuv420_resize_run_direct(
    const Yuv420Row& r0, const Yuv420Row& r1, const Yuv420Coef& kf, float wy,
    int ox0, typename CVT::Out* __restrict__ dst, int64_t plane,
    const U8ResizeParams& p) {
  using Out = typename CVT::Out;
  constexpr int C = 3;
  Out vout[C * kResizePx];   // NCHW: [c][k], NHWC: [k][c]
#pragma unroll
  for (int k = 0; k < kResizePx; ++k) {
    const int ox = min(ox0 + k, p.Wc - 1);
    int x0, x1;
    float wx;
    resize_tap(ox, p.left, p.rw, p.Win, x0, x1, wx);
    float p00[C], p01[C], p10[C], p11[C];
    r0.rgb(x0, kf, p00);
    r0.rgb(x1, kf, p01);
    r1.rgb(x0, kf, p10);
    r1.rgb(x1, kf, p11);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float t =
          __fadd_rn(p00[c], __fmul_rn(wx, __fsub_rn(p01[c], p00[c])));
      const float b =
          __fadd_rn(p10[c], __fmul_rn(wx, __fsub_rn(p11[c], p10[c])));
      const float v = __fadd_rn(t, __fmul_rn(wy, __fsub_rn(b, t)));
      vout[NCHW ? c * kResizePx + k : k * C + c] =
          CVT::cvt(__fadd_rn(__fmul_rn(v, p.scale[c]), p.bias[c]));
    }
  }
  resize_store_run<Out, C, NCHW>(vout, ox0, p.Wc, dst, plane);
}

// 16 luma bytes `yw` and their 8 chroma samples `cw` (NV12: U,V interleaved;
// I420: 8 U bytes then 8 V bytes) -> 48 RGB bytes `o`.
template <bool I420>
__device__ __forceinline__ void yuv420_convert_chunk(
    const uint32_t (&yw)[4], const uint32_t (&cw)[4], const Yuv420Coef& k,
    uint32_t (&o)[12]) {
#pragma unroll
  for (int w = 0; w < 12; ++w) o[w] = 0;
#pragma unroll
  for (int pr = 0; pr < kYuvChunkPx / 2; ++pr) {
    const int ub = I420 ? pr : 2 * pr, vb = I420 ? 8 + pr : 2 * pr + 1;
    const int D = int((cw[ub >> 2] >> (8 * (ub & 3))) & 0xffu) - 128;
    const int E = int((cw[vb >> 2] >> (8 * (vb & 3))) & 0xffu) - 128;
    const int rE = k.rv * E, gDE = k.gu * D + k.gv * E, bD = k.bu * D;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * pr + h;
      const int Y = int((yw[j >> 2] >> (8 * (j & 3))) & 0xffu);
      const int base = k.yc * (Y - k.yoff) + 128;
      const uint32_t rgb[3] = {yuv_clamp8(base + rE), yuv_clamp8(base + gDE),
                               yuv_clamp8(base + bD)};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = 3 * j + c;
        o[b >> 2] |= rgb[c] << (8 * (b & 3));
      }
    }
  }
}

// One fill chunk: the 16 luma bytes at `ya` and their 8 chroma samples at
// `ua`/`va` -> 48 RGB bytes at `l` (LDS, 16 B-aligned). Unaligned vector loads
// when they stay below `in_end`, the end of the tensor; else bytewise, in
// bounds, zeros for what lies past it.
template <bool I420>
__device__ __forceinline__ void yuv420_fill_chunk(
    const uint8_t* ya, const uint8_t* ua, const uint8_t* va,
    const uint8_t* in_end, const Yuv420Coef& k, int4* l) {
  uint32_t yw[4], cw[4];
  // the V (NV12: U,V) bytes end last: if they are inside, all are
  if ((I420 ? va + 8 : ua + 16) <= in_end && ya + 16 <= in_end) {
    __builtin_memcpy(yw, ya, 16);
    if constexpr (I420) {
      __builtin_memcpy(cw, ua, 8);
      __builtin_memcpy(cw + 2, va, 8);
    } else {
      __builtin_memcpy(cw, ua, 16);
    }
  } else {
    // the last chunks of the tensor: stay inside it
#pragma unroll
    for (int w = 0; w < 4; ++w) yw[w] = cw[w] = 0;
    for (int b = 0; b < 16; ++b) {
      const uint8_t* ca = I420 ? (b < 8 ? ua + b : va + (b - 8)) : ua + b;
      const uint32_t yb = ya + b < in_end ? ya[b] : 0u;
      const uint32_t cb = ca < in_end ? *ca : 0u;
      yw[b >> 2] |= yb << (8 * (b & 3));
      cw[b >> 2] |= cb << (8 * (b & 3));
    }
  }
  uint32_t o[12];
  yuv420_convert_chunk<I420>(yw, cw, k, o);
#pragma unroll
  for (int v = 0; v < 3; ++v) l[v] = *reinterpret_cast<const int4*>(o + 4 * v);
}

template <typename CVT, bool NCHW, bool I420>
__global__ void __launch_bounds__(kResizeBlock)
yuv420_resize_normalize_kernel(
    const uint8_t* __restrict__ in, typename CVT::Out* __restrict__ out,
    int64_t N, Yuv420ResizeParams pp) {
  using Out = typename CVT::Out;
  constexpr int C = 3;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kResizeLdsBytes];
  static_assert(kResizePx % (16 / int(sizeof(Out))) == 0,
                "a lane run must fill whole 16 B stores");
  const U8ResizeParams& p = pp.r;
  const int twl = 1 << p.twl_log2;               // lane runs per tile row
  const int tr = kResizeBlock >> p.twl_log2;     // rows per tile
  const int tw = twl * kResizePx;                // columns per tile
  const int r = int(threadIdx.x) >> p.twl_log2;
  const int j = int(threadIdx.x) & (twl - 1);
  const int64_t plane = int64_t(p.Hc) * p.Wc;
  const int64_t y_bytes = int64_t(p.Hin) * p.Win;
  const int64_t c_bytes = int64_t(p.Hin >> 1) * (p.Win >> 1);   // one plane
  const int64_t frame_bytes = y_bytes + 2 * c_bytes;
  const int64_t c_row = I420 ? p.Win >> 1 : p.Win;   // chroma row stride
  const int cstep = I420 ? 1 : 2;
  const uint8_t* const in_end = in + N * frame_bytes;
  const int64_t items = N * p.tiles_y * p.tiles_x;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int tx = int(item % p.tiles_x);
    const int ty = int((item / p.tiles_x) % p.tiles_y);
    const int64_t n = item / (int64_t(p.tiles_x) * p.tiles_y);
    const uint8_t* img = in + n * frame_bytes;
    const uint8_t* uimg = img + y_bytes;
    const uint8_t* vimg = I420 ? uimg + c_bytes : uimg + 1;
    const int oy = ty * tr + r;
    const int ox0 = tx * tw + j * kResizePx;
    const bool active = oy < p.Hc && ox0 < p.Wc;

    // source column span of the tile, the same for every row of it
    int xs_lo, xs_hi, unused;
    float unused_w;
    resize_tap(tx * tw, p.left, p.rw, p.Win, xs_lo, unused, unused_w);
    resize_tap(min(tx * tw + tw, p.Wc) - 1, p.left, p.rw, p.Win, unused,
               xs_hi, unused_w);
    const int xe = xs_lo & ~1;   // spans start on a chroma pair
    // uniform in the workgroup: the barriers below are not divergent
    const bool use_lds = pp.span_px > 0 && xs_hi + 1 - xe <= pp.span_px;

    int y0 = 0, y1 = 0;
    float wy = 0.f;
    if (active) resize_tap(oy, p.top, p.rh, p.Hin, y0, y1, wy);
    Out* dst = NCHW
        ? out + (n * C * p.Hc + oy) * p.Wc + ox0
        : out + ((n * p.Hc + oy) * p.Wc + ox0) * C;

    if (use_lds) {
      const int nchunks = pp.span_px / kYuvChunkPx;
      const int rows_here = min(tr, p.Hc - ty * tr);
      const int total = 2 * rows_here * nchunks;
      for (int idx = int(threadIdx.x); idx < total; idx += kResizeBlock) {
        const int s = idx / nchunks;           // span: tile row s>>1, y(s&1)
        const int xc = xe + (idx - s * nchunks) * kYuvChunkPx;
        if (xc > xs_hi) continue;
        int sy0, sy1;
        float sw;
        resize_tap(ty * tr + (s >> 1), p.top, p.rh, p.Hin, sy0, sy1, sw);
        const int sy = (s & 1) ? sy1 : sy0;
        const uint8_t* ya = img + int64_t(sy) * p.Win + xc;
        const int64_t co = int64_t(sy >> 1) * c_row + (xc >> 1) * cstep;
        const uint8_t* ua = uimg + co;
        const uint8_t* va = vimg + co;
        yuv420_fill_chunk<I420>(
            ya, ua, va, in_end, pp.k,
            reinterpret_cast<int4*>(lds + s * p.span_stride + (xc - xe) * C));
      }
      __syncthreads();
      if (active) {
        const uint8_t* l0 = lds + (2 * r) * p.span_stride;
        const uint8_t* l1 = lds + (2 * r + 1) * p.span_stride;
        resize_run<CVT, C, NCHW>(l0, l1, xe, wy, ox0, dst, plane, p);
      }
      __syncthreads();   // lds is refilled by the next work item
    } else if (active) {
      const Yuv420Row r0{img + int64_t(y0) * p.Win,
                         uimg + int64_t(y0 >> 1) * c_row,
                         vimg + int64_t(y0 >> 1) * c_row, cstep};
      const Yuv420Row r1{img + int64_t(y1) * p.Win,
                         uimg + int64_t(y1 >> 1) * c_row,
                         vimg + int64_t(y1 >> 1) * c_row, cstep};
      yuv420_resize_run_direct<CVT, NCHW>(r0, r1, pp.k, wy, ox0, dst, plane,
                                          p);
    }
  }
}

// ---------------------------------------------------------------------------
// uint8 image ingest with ANTIALIASED resize + crop (separable triangle)
// ---------------------------------------------------------------------------
// Same contract as the bilinear section above (uint8 NHWC in, a crop window
// of a virtual (Hr,Wr) image out, normalized and cast), but a downscale
// averages every source pixel under a triangle filter whose width follows
// the ratio: the F.interpolate(mode="bilinear", antialias=True) family, with
// ATen's _compute_indices_weights_aa index rule and ONE division by the
// weight sum in place of per-weight normalization. For one axis (input
// length n_in, ratio r = float(n_in/n_r) from the host, o = output index +
// crop offset), every line one IEEE fp32 operation, nothing contracted:
//
//   support = r >= 1 ? r : 1        inv = r >= 1 ? float(1.0/double(r)) : 1
//   c    = fmul(fadd(float(o), 0.5), r)
//   lo   = clamp(int(fadd(fsub(c, support), 0.5)), 0, n_in-1)   int(): trunc
//   hi   = min(int(fadd(fadd(c, support), 0.5)), n_in)
//   size = max(hi - lo, 1)
//   for j = 0 .. size-1, ascending:
//     x   = fmul(fadd(fsub(float(lo+j), c), 0.5), inv)
//     w   = max(fsub(1, |x|), 0)
//     acc = fadd(acc, fmul(w, p[lo+j]))      tot = fadd(tot, w)
//   value = fdiv(acc, tot)                   IEEE division; tot >= 0.75
//
// Horizontal first (uint8 -> fp32), then vertical on those fp32 values, then
// y = Out(fadd(fmul(v, scale_c), bias_c)). With (Hr,Wr) == (Hin,Win) the
// weights are exactly (1, 0) and the result is bit-identical to
// u8_nhwc_normalize_kernel. c, lo and hi are monotone in o (each rounded
// operation is), so the source rows one crop window needs are the range
// [lo(first row), lo(last row) + size(last row)): y_base and Rs below.
//
// Two kernels, always, in this order on the current stream:
//
//  1. u8_resize_aa_h_kernel: a lane owns one (image, source row, output
//     column) and all C channels of it. It recomputes c/lo/size and each
//     tap weight on the fly (no weight tables, no per-call H2D), walks its
//     `size` taps with byte loads straight from global memory (neighbouring
//     lanes' spans overlap, so the bytes come from L1/L2) and writes C
//     floats to the fp32 workspace [n, Rs, Wc, C]. Only the Rs source rows
//     and the Wc cropped columns are computed. The tap loop has a runtime
//     trip count (up to 32769 at the 16384-side limits).
//  2. u8_resize_aa_v_kernel: a lane owns kResizePx = 8 consecutive output
//     columns of one output row, all channels: 8*C contiguous floats per
//     workspace row, loaded as 16 B vectors when the run is whole and the
//     address is 16 B-aligned (every workspace row is when Wc*C % 4 == 0),
//     else as scalars with the column clamped (duplicates are never
//     stored). It accumulates the `size` rows in ascending order, divides,
//     normalizes, casts and stores with resize_store_run (16 B vectors, or
//     scalars for a ragged run or a misaligned destination/plane).
//
// Both grids: 256-thread workgroups, min(ceil(lanes/256), 2048) of them,
// grid-stride over lanes. The workspace holds Rs*Wc*C floats per image and
// is capped (kResizeAAWsBytes); a batch that needs more runs in chunks of
// whole images through one workspace, each chunk both kernels. An image is
// computed the same way whichever chunk it lands in.
constexpr int kResizeAABlock = 256;

struct U8ResizeAAParams {
  float scale[4];
  float bias[4];
  float rh, rw;          // ratios
  float sup_h, sup_w;    // filter support per axis: max(r, 1)
  float inv_h, inv_w;    // 1/support, rounded once on the host
  int Hin, Win, Hc, Wc, top, left;
  int y_base, Rs;        // first source row of the workspace, and its rows
};

#if defined(__HIP_DEVICE_COMPILE__)
#define AA_MUL(a, b) __fmul_rn((a), (b))
#define AA_ADD(a, b) __fadd_rn((a), (b))
#define AA_SUB(a, b) __fsub_rn((a), (b))
#else  // host: this file is built with -ffp-contract=off
#define AA_MUL(a, b) ((a) * (b))
#define AA_ADD(a, b) ((a) + (b))
#define AA_SUB(a, b) ((a) - (b))
#endif

// Centre, first tap and tap count of coordinate `o` of the resized axis.
// Also run on the host, for the workspace's row range.
__host__ __device__ __forceinline__ void aa_span(int o, float r, float support,
                                                 int n_in, float& c, int& lo,
                                                 int& size) {
  c = AA_MUL(AA_ADD(float(o), 0.5f), r);
  const int l = int(AA_ADD(AA_SUB(c, support), 0.5f));
  const int h = int(AA_ADD(AA_ADD(c, support), 0.5f));
  lo = l < 0 ? 0 : (l > n_in - 1 ? n_in - 1 : l);
  const int hi = h < n_in ? h : n_in;
  size = hi - lo > 1 ? hi - lo : 1;
}

__device__ __forceinline__ float aa_weight(int i, float c, float inv) {
  const float x = __fmul_rn(__fadd_rn(__fsub_rn(float(i), c), 0.5f), inv);
  return fmaxf(__fsub_rn(1.f, fabsf(x)), 0.f);
}

template <int C>
__global__ void __launch_bounds__(kResizeAABlock) u8_resize_aa_h_kernel(
    const uint8_t* __restrict__ in, float* __restrict__ ws, int64_t N,
    U8ResizeAAParams p) {
  const int64_t row_bytes = int64_t(p.Win) * C;
  const int64_t lanes = N * p.Rs * p.Wc;
  const int64_t stride = int64_t(gridDim.x) * kResizeAABlock;
  for (int64_t idx = int64_t(blockIdx.x) * kResizeAABlock + threadIdx.x;
       idx < lanes; idx += stride) {
    const int ox = int(idx % p.Wc);
    const int64_t t = idx / p.Wc;
    const int s = int(t % p.Rs);
    const int64_t n = t / p.Rs;
    float c;
    int lo, size;
    aa_span(ox + p.left, p.rw, p.sup_w, p.Win, c, lo, size);
    // lo + size <= Win and y_base + Rs <= Hin: every tap is inside the image
    const uint8_t* src =
        in + (n * p.Hin + p.y_base + s) * row_bytes + int64_t(lo) * C;
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.f;
    float tot = 0.f;
    for (int j = 0; j < size; ++j) {
      const float w = aa_weight(lo + j, c, p.inv_w);
#pragma unroll
      for (int ch = 0; ch < C; ++ch)
        acc[ch] = __fadd_rn(acc[ch], __fmul_rn(w, float(src[j * C + ch])));
      tot = __fadd_rn(tot, w);
    }
    float* dst = ws + idx * C;   // [n][s][ox][ch]
#pragma unroll
    for (int ch = 0; ch < C; ++ch) dst[ch] = __fdiv_rn(acc[ch], tot);
  }
}

template <typename CVT, int C, bool NCHW>
__global__ void __launch_bounds__(kResizeAABlock) u8_resize_aa_v_kernel(
    const float* __restrict__ ws, typename CVT::Out* __restrict__ out,
    int64_t N, U8ResizeAAParams p) {
  using Out = typename CVT::Out;
  constexpr int L = kResizePx * C;       // floats per workspace row and lane
  static_assert(kResizePx % (16 / int(sizeof(Out))) == 0,
                "a lane run must fill whole 16 B stores");
  const int runs = (p.Wc + kResizePx - 1) / kResizePx;
  const int64_t plane = int64_t(p.Hc) * p.Wc;
  const int64_t row_floats = int64_t(p.Wc) * C;
  const int64_t lanes = N * p.Hc * runs;
  const int64_t stride = int64_t(gridDim.x) * kResizeAABlock;
  for (int64_t idx = int64_t(blockIdx.x) * kResizeAABlock + threadIdx.x;
       idx < lanes; idx += stride) {
    const int ox0 = int(idx % runs) * kResizePx;
    const int64_t t = idx / runs;
    const int oy = int(t % p.Hc);
    const int64_t n = t / p.Hc;
    float c;
    int lo, size;
    aa_span(oy + p.top, p.rh, p.sup_h, p.Hin, c, lo, size);
    // y_base <= lo and lo + size <= y_base + Rs (monotone in oy)
    const float* src =
        ws + ((n * p.Rs + (lo - p.y_base)) * p.Wc + ox0) * C;
    const int valid = min(kResizePx, p.Wc - ox0) * C;   // floats of this run
    float acc[L];
#pragma unroll
    for (int e = 0; e < L; ++e) acc[e] = 0.f;
    float tot = 0.f;
    if (valid == L && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
        row_floats % 4 == 0) {
      for (int j = 0; j < size; ++j, src += row_floats) {
        const float w = aa_weight(lo + j, c, p.inv_h);
        float v[L];
#pragma unroll
        for (int q = 0; q < L / 4; ++q)
          reinterpret_cast<float4*>(v)[q] =
              reinterpret_cast<const float4*>(src)[q];
#pragma unroll
        for (int e = 0; e < L; ++e)
          acc[e] = __fadd_rn(acc[e], __fmul_rn(w, v[e]));
        tot = __fadd_rn(tot, w);
      }
    } else {
      for (int j = 0; j < size; ++j, src += row_floats) {
        const float w = aa_weight(lo + j, c, p.inv_h);
#pragma unroll
        for (int e = 0; e < L; ++e)
          acc[e] = __fadd_rn(acc[e], __fmul_rn(w, src[min(e, valid - 1)]));
        tot = __fadd_rn(tot, w);
      }
    }
    Out vout[L];   // NCHW: [c][k], NHWC: [k][c]
#pragma unroll
    for (int k = 0; k < kResizePx; ++k)
#pragma unroll
      for (int ch = 0; ch < C; ++ch)
        vout[NCHW ? ch * kResizePx + k : k * C + ch] = CVT::cvt(__fadd_rn(
            __fmul_rn(__fdiv_rn(acc[k * C + ch], tot), p.scale[ch]),
            p.bias[ch]));
    Out* dst = NCHW
        ? out + (n * C * p.Hc + oy) * p.Wc + ox0
        : out + ((n * p.Hc + oy) * p.Wc + ox0) * C;
    resize_store_run<Out, C, NCHW>(vout, ox0, p.Wc, dst, plane);
  }
}

// ---------------------------------------------------------------------------
// YUV 4:2:0 source side (NV12 / I420) of the antialiased resize + crop ingest
// ---------------------------------------------------------------------------
// yuv420_resize_aa_h_kernel is the horizontal pass of the recipe above on
// frames laid out as in the bilinear YUV section: every tap is the converted,
// clamped uint8 value of its source pixel (the int32 conversion of that
// section, yuv_clamp8 included), widened to fp32, and the taps are walked in
// the same ascending order with the same fmul/fadd sequence and the one
// division by tot. It writes the fp32 workspace [n, Rs, Wc, 3] that
// u8_resize_aa_h_kernel<3> writes for the converted frames, bit for bit; the
// vertical pass is u8_resize_aa_v_kernel<CVT, 3, NCHW>, unchanged.
//
// A lane owns one (frame, source row, output column). A 256-thread workgroup
// owns a tile of 2^tc_log2 output columns by 256 >> tc_log2 source rows (the
// host picks the widest tile of 8..64 columns that pads Wc by at most 1/8,
// else 8); a work item is (frame, row tile, column tile) and workgroups
// grid-stride over work items, at most 2048 of them.
//
// Source taps, two paths, chosen per work item (uniform in the workgroup):
//  * LDS path. Under the triangle filter neighbouring columns' tap ranges
//    overlap, each source pixel feeds about two columns, and a conversion is
//    three integer multiplies and three clamps. lo and lo + size = max(hi,
//    lo + 1) are monotone in the output index, so every tap of the tile lies
//    in [lo(first column), lo(last column) + size(last column)). The
//    workgroup converts that span of each of its source rows once, from the
//    even column xe = lo(first) & ~1 in 16-pixel chunks (yuv420_fill_chunk,
//    as the bilinear kernel does), into LDS as RGB bytes, and the tap loops
//    read LDS.
//  * direct path: Yuv420Row converts each tap from global memory with byte
//    loads. Taken when the host found that the tile's spans exceed
//    kYuvAALdsBytes (span_px == 0: large downscale ratios) or was asked to
//    (variant 1), or when a tile's span does not fit the host's estimate.
constexpr int kYuvAALdsBytes = 16384;    // 10 workgroups per CU: wave-limited
constexpr int kYuvAAMinTcLog2 = 3;       // tile: 8 columns x 32 rows ...
constexpr int kYuvAAMaxTcLog2 = 6;       // ... to 64 columns x 4 rows

struct Yuv420ResizeAAParams {
  U8ResizeAAParams a;
  Yuv420Coef k;
  int tc_log2;       // output columns per tile, log2
  int tiles_x, tiles_y;
  int span_px;       // pixels per LDS span (multiple of 16), 0: direct
};

template <bool I420>
__global__ void __launch_bounds__(kResizeAABlock) yuv420_resize_aa_h_kernel(
    const uint8_t* __restrict__ in, float* __restrict__ ws, int64_t N,
    Yuv420ResizeAAParams pp) {
  constexpr int C = 3;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kYuvAALdsBytes];
  const U8ResizeAAParams& p = pp.a;
  const int tc = 1 << pp.tc_log2;                  // columns per tile
  const int tr = kResizeAABlock >> pp.tc_log2;     // source rows per tile
  const int r = int(threadIdx.x) >> pp.tc_log2;
  const int j = int(threadIdx.x) & (tc - 1);
  const int span_stride = pp.span_px * C;          // LDS bytes per row
  const int64_t y_bytes = int64_t(p.Hin) * p.Win;
  const int64_t c_bytes = int64_t(p.Hin >> 1) * (p.Win >> 1);   // one plane
  const int64_t frame_bytes = y_bytes + 2 * c_bytes;
  const int64_t c_row = I420 ? p.Win >> 1 : p.Win;   // chroma row stride
  const int cstep = I420 ? 1 : 2;
  const uint8_t* const in_end = in + N * frame_bytes;
  const int64_t items = N * pp.tiles_y * pp.tiles_x;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int tx = int(item % pp.tiles_x);
    const int ty = int((item / pp.tiles_x) % pp.tiles_y);
    const int64_t n = item / (int64_t(pp.tiles_x) * pp.tiles_y);
    const uint8_t* img = in + n * frame_bytes;
    const uint8_t* uimg = img + y_bytes;
    const uint8_t* vimg = I420 ? uimg + c_bytes : uimg + 1;
    const int s = ty * tr + r;
    const int ox = tx * tc + j;
    const bool active = s < p.Rs && ox < p.Wc;

    // source column span of the tile, the same for every row of it
    float unused_c;
    int lo_f, lo_l, size_f, size_l;
    aa_span(tx * tc + p.left, p.rw, p.sup_w, p.Win, unused_c, lo_f, size_f);
    aa_span(min(tx * tc + tc, p.Wc) - 1 + p.left, p.rw, p.sup_w, p.Win,
            unused_c, lo_l, size_l);
    const int xe = lo_f & ~1;          // spans start on a chroma pair
    const int x_end = lo_l + size_l;   // <= Win
    // uniform in the workgroup: the barriers below are not divergent
    const bool use_lds = pp.span_px > 0 && x_end - xe <= pp.span_px;

    float c = 0.f;
    int lo = 0, size = 0;
    if (active) aa_span(ox + p.left, p.rw, p.sup_w, p.Win, c, lo, size);
    float acc[C] = {0.f, 0.f, 0.f};
    float tot = 0.f;

    if (use_lds) {
      const int nchunks = pp.span_px / kYuvChunkPx;
      const int rows_here = min(tr, p.Rs - ty * tr);
      const int total = rows_here * nchunks;
      for (int idx = int(threadIdx.x); idx < total; idx += kResizeAABlock) {
        const int fr = idx / nchunks;             // tile row
        const int xc = xe + (idx - fr * nchunks) * kYuvChunkPx;
        if (xc >= x_end) continue;
        // y_base + Rs <= Hin: the row is inside the frame
        const int sy = p.y_base + ty * tr + fr;
        const uint8_t* ya = img + int64_t(sy) * p.Win + xc;
        const int64_t co = int64_t(sy >> 1) * c_row + (xc >> 1) * cstep;
        yuv420_fill_chunk<I420>(
            ya, uimg + co, vimg + co, in_end, pp.k,
            reinterpret_cast<int4*>(lds + fr * span_stride + (xc - xe) * C));
      }
      __syncthreads();
      if (active) {
        // xe <= lo and lo + size <= x_end (monotone in ox)
        const uint8_t* l = lds + r * span_stride + (lo - xe) * C;
        for (int t = 0; t < size; ++t) {
          const float w = aa_weight(lo + t, c, p.inv_w);
#pragma unroll
          for (int ch = 0; ch < C; ++ch)
            acc[ch] = __fadd_rn(acc[ch], __fmul_rn(w, float(l[t * C + ch])));
          tot = __fadd_rn(tot, w);
        }
      }
      __syncthreads();   // lds is refilled by the next work item
    } else if (active) {
      // lo + size <= Win and y_base + Rs <= Hin: every tap is inside the frame
      const int sy = p.y_base + s;
      const Yuv420Row row{img + int64_t(sy) * p.Win,
                          uimg + int64_t(sy >> 1) * c_row,
                          vimg + int64_t(sy >> 1) * c_row, cstep};
      for (int t = 0; t < size; ++t) {
        const float w = aa_weight(lo + t, c, p.inv_w);
        float px[C];
        row.rgb(lo + t, pp.k, px);
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
          acc[ch] = __fadd_rn(acc[ch], __fmul_rn(w, px[ch]));
        tot = __fadd_rn(tot, w);
      }
    }
    if (active) {
      float* dst = ws + ((n * p.Rs + s) * p.Wc + ox) * C;   // [n][s][ox][ch]
#pragma unroll
      for (int ch = 0; ch < C; ++ch) dst[ch] = __fdiv_rn(acc[ch], tot);
    }
  }
}

// ---------------------------------------------------------------------------
// antialiased ragged batch: N images of N different sizes, two launches
// ---------------------------------------------------------------------------
// The antialiased recipe above, bit for bit (aa_span, aa_weight and
// resize_store_run are shared, the lane bodies are those of the two dense
// kernels), for images that lie back to back in one flat uint8 buffer, HWC
// each, no padding, as in the bilinear ragged section. The output size
// (Hc,Wc) is shared; everything on the source side is per image and comes
// from a table in device memory that u8_ragged_resize_aa_normalize builds.
//
// The fp32 workspace is ragged too: image i of a chunk owns Rs_i rows of
// Wc*C floats from workspace row ws_row0_i, the running sum of Rs over the
// earlier images of the same chunk (it restarts at 0 in every chunk).
//
//  1. u8_ragged_resize_aa_h_kernel: lanes are the flattened (workspace row
//     g, output column ox) pairs of the chunk. A lane finds its image by a
//     binary search for g over the ws_row0 column of the chunk's table (at
//     most 5 steps for 32 images, on lines every lane of the launch shares),
//     then does what the dense horizontal lane does for (image, y_base_i +
//     g - ws_row0_i, ox). Its taps are byte loads, so an image may start at
//     any byte alignment.
//  2. u8_ragged_resize_aa_v_kernel: lanes are (image, oy, run of kResizePx
//     columns) as in the dense vertical kernel; the image's rows start at
//     workspace row ws_row0_n and its ratio, support and crop origin come
//     from the table. Both load paths and the stores are the dense kernel's.
//
// One table entry, 16 int32 words (the host fills the struct and ships the
// table as int32 [N,16]):
//   0-1   offset    first byte of the image in the flat buffer (int64)
//   2-3   ws_row0   first workspace row of the image in its chunk (int64)
//   4-7   Hin, Win, top, left
//   8-9   rh, rw                 ratios, float32(Hin/Hr), float32(Win/Wr)
//   10-13 sup_h, sup_w, inv_h, inv_w   as in U8ResizeAAParams
//   14    y_base    first source row in the workspace
//   15    Rs        source rows in the workspace (host-side chunking only)
// Of the shared U8ResizeAAParams only scale, bias, Hc and Wc are read.
struct U8RaggedAAEntry {
  int64_t offset;
  int64_t ws_row0;
  int Hin, Win, top, left;
  float rh, rw;
  float sup_h, sup_w;
  float inv_h, inv_w;
  int y_base, Rs;
};
static_assert(sizeof(U8RaggedAAEntry) == 64, "table rows are int32 [16]");

template <int C>
__global__ void __launch_bounds__(kResizeAABlock) u8_ragged_resize_aa_h_kernel(
    const uint8_t* __restrict__ in, float* __restrict__ ws,
    const U8RaggedAAEntry* __restrict__ table, int N, int64_t rows,
    U8ResizeAAParams p) {
  const int64_t lanes = rows * p.Wc;
  const int64_t stride = int64_t(gridDim.x) * kResizeAABlock;
  for (int64_t idx = int64_t(blockIdx.x) * kResizeAABlock + threadIdx.x;
       idx < lanes; idx += stride) {
    const int ox = int(idx % p.Wc);
    const int64_t g = idx / p.Wc;
    // the image whose rows hold g: the last entry with ws_row0 <= g
    // (ws_row0 is strictly increasing, Rs >= 1, and table[0].ws_row0 == 0)
    int first = 0, last = N;
    while (last - first > 1) {
      const int mid = (first + last) >> 1;
      if (table[mid].ws_row0 <= g) first = mid;
      else last = mid;
    }
    const U8RaggedAAEntry e = table[first];
    const int s = int(g - e.ws_row0);
    float c;
    int lo, size;
    aa_span(ox + e.left, e.rw, e.sup_w, e.Win, c, lo, size);
    // lo + size <= Win and y_base + Rs <= Hin: every tap is inside the image
    const uint8_t* src = in + e.offset +
        (int64_t(e.y_base + s) * e.Win + lo) * C;
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.f;
    float tot = 0.f;
    for (int j = 0; j < size; ++j) {
      const float w = aa_weight(lo + j, c, e.inv_w);
#pragma unroll
      for (int ch = 0; ch < C; ++ch)
        acc[ch] = __fadd_rn(acc[ch], __fmul_rn(w, float(src[j * C + ch])));
      tot = __fadd_rn(tot, w);
    }
    float* dst = ws + idx * C;   // [g][ox][ch]
#pragma unroll
    for (int ch = 0; ch < C; ++ch) dst[ch] = __fdiv_rn(acc[ch], tot);
  }
}

template <typename CVT, int C, bool NCHW>
__global__ void __launch_bounds__(kResizeAABlock) u8_ragged_resize_aa_v_kernel(
    const float* __restrict__ ws, typename CVT::Out* __restrict__ out,
    const U8RaggedAAEntry* __restrict__ table, int64_t N,
    U8ResizeAAParams p) {
  using Out = typename CVT::Out;
  constexpr int L = kResizePx * C;       // floats per workspace row and lane
  static_assert(kResizePx % (16 / int(sizeof(Out))) == 0,
                "a lane run must fill whole 16 B stores");
  const int runs = (p.Wc + kResizePx - 1) / kResizePx;
  const int64_t plane = int64_t(p.Hc) * p.Wc;
  const int64_t row_floats = int64_t(p.Wc) * C;
  const int64_t lanes = N * p.Hc * runs;
  const int64_t stride = int64_t(gridDim.x) * kResizeAABlock;
  for (int64_t idx = int64_t(blockIdx.x) * kResizeAABlock + threadIdx.x;
       idx < lanes; idx += stride) {
    const int ox0 = int(idx % runs) * kResizePx;
    const int64_t t = idx / runs;
    const int oy = int(t % p.Hc);
    const int64_t n = t / p.Hc;
    const U8RaggedAAEntry e = table[n];
    float c;
    int lo, size;
    aa_span(oy + e.top, e.rh, e.sup_h, e.Hin, c, lo, size);
    // y_base <= lo and lo + size <= y_base + Rs (monotone in oy)
    const float* src =
        ws + ((e.ws_row0 + (lo - e.y_base)) * p.Wc + ox0) * C;
    const int valid = min(kResizePx, p.Wc - ox0) * C;   // floats of this run
    float acc[L];
#pragma unroll
    for (int k = 0; k < L; ++k) acc[k] = 0.f;
    float tot = 0.f;
    if (valid == L && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
        row_floats % 4 == 0) {
      for (int j = 0; j < size; ++j, src += row_floats) {
        const float w = aa_weight(lo + j, c, e.inv_h);
        float v[L];
#pragma unroll
        for (int q = 0; q < L / 4; ++q)
          reinterpret_cast<float4*>(v)[q] =
              reinterpret_cast<const float4*>(src)[q];
#pragma unroll
        for (int k = 0; k < L; ++k)
          acc[k] = __fadd_rn(acc[k], __fmul_rn(w, v[k]));
        tot = __fadd_rn(tot, w);
      }
    } else {
      for (int j = 0; j < size; ++j, src += row_floats) {
        const float w = aa_weight(lo + j, c, e.inv_h);
#pragma unroll
        for (int k = 0; k < L; ++k)
          acc[k] = __fadd_rn(acc[k], __fmul_rn(w, src[min(k, valid - 1)]));
        tot = __fadd_rn(tot, w);
      }
    }
    Out vout[L];   // NCHW: [c][k], NHWC: [k][c]
#pragma unroll
    for (int k = 0; k < kResizePx; ++k)
#pragma unroll
      for (int ch = 0; ch < C; ++ch)
        vout[NCHW ? ch * kResizePx + k : k * C + ch] = CVT::cvt(__fadd_rn(
            __fmul_rn(__fdiv_rn(acc[k * C + ch], tot), p.scale[ch]),
            p.bias[ch]));
    Out* dst = NCHW
        ? out + (n * C * p.Hc + oy) * p.Wc + ox0
        : out + ((n * p.Hc + oy) * p.Wc + ox0) * C;
    resize_store_run<Out, C, NCHW>(vout, ox0, p.Wc, dst, plane);
  }
}

// ---------------------------------------------------------------------------
// fused masked mean-pool head (+ optional L2 normalize): [B,S,H] -> [B,H]
// ---------------------------------------------------------------------------
// cnt_b  = #{s : mask[b,s] != 0}
// sum_bh = sum over kept s of float(hidden[b,s,h])   (fp32, SELECT: a masked
//          row is never loaded, so NaN/Inf there cannot reach the output)
// y_bh   = sum_bh / float(max(cnt_b, 1))
// normalize: y_bh /= max(sqrt(sum_h y_bh^2), 1e-12f)  (F.normalize semantics)
//
// Division and square root are correctly rounded: `__fdiv_rn` is an IEEE
// divide here and `sqrtf` an IEEE square root (hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt). `__fsqrt_rn` is NOT used: in
// this toolchain it lowers to the native v_sqrt_f32, which is 1 ulp off.
//
// Two kernels, always, in this order on the current stream:
//
//  1. masked_pool_partial_kernel reads the hidden state once. A work item
//     is (b, S-slice k, column tile): one 256-thread workgroup, whose 4
//     waves take rows s = s_begin + wave, +4, ... of the slice; the 64
//     lanes of a wave span 64 consecutive column vectors of one row (one
//     contiguous run, 1 KB on the vector path), so the mask test is
//     wave-uniform and a masked row costs one 4 B load. Rows are unrolled
//     4 deep per wave to keep 4 loads in flight. The 4 waves' accumulators
//     are combined through LDS in wave order and the slice's partial sums
//     go to a [B, nsplit, H] fp32 workspace. No atomics.
//  2. masked_pool_finalize_kernel: one workgroup per b. It counts the mask
//     row (integer block reduction), adds the nsplit partials for each h in
//     slice order, divides, and (normalize) reduces y^2 over the row with a
//     fixed shuffle tree + LDS, takes the square root and divides again.
//
// Every sum has a fixed order that depends only on the shape, so the output
// is bit-identical from run to run.
//
// Paths and thresholds (the tests pin one shape on each side):
//  * vector path: VEC = 16/sizeof(T) elements per lane (4 f32, 8 bf16/f16),
//    taken iff the base pointer and H*sizeof(T) are multiples of 16;
//    otherwise the scalar path, VEC = 1. Column tiles: ceil(H/VEC / 64).
//  * S split: nsplit = 1 if B*tiles >= kPoolTargetBlocks (1024) or
//    S <= kPoolMinRows (16); else nsplit = min(ceil(1024 / (B*tiles)),
//    ceil(S/16)), rows per slice = ceil(S/nsplit), nsplit = ceil(S/rows).
//  * grid: min(B*nsplit*tiles, 2048) workgroups (grid_for), grid-stride over
//    work items; the finalize grid is min(B, 2048), grid-stride over b.
//  * S == 0 or an all-zero mask row: sums are 0 and the count clamps to 1,
//    so the row is zeros. B == 0 or H == 0 returns without launching.
constexpr int kPoolBlock = 256;          // 4 waves
constexpr int kPoolWaves = kPoolBlock / 64;
constexpr int64_t kPoolTargetBlocks = 1024;
constexpr int64_t kPoolMinRows = 16;

template <typename CVT, int VEC>
__device__ __forceinline__ void pool_load(
    const typename CVT::In* __restrict__ p, typename CVT::In (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = *p;
  } else {
    static_assert(sizeof(typename CVT::In) * VEC == 16, "16 B per lane");
    *reinterpret_cast<int4*>(v) = *reinterpret_cast<const int4*>(p);
  }
}

template <typename CVT, int VEC, typename M>
__global__ void __launch_bounds__(kPoolBlock) masked_pool_partial_kernel(
    const typename CVT::In* __restrict__ hidden, const M* __restrict__ mask,
    float* __restrict__ ws, int64_t B, int64_t S, int64_t H, int64_t tiles,
    int64_t nsplit, int64_t rows_per_split) {
  using In = typename CVT::In;
  __shared__ float lds[kPoolWaves - 1][64][VEC];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t items = B * nsplit * tiles;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t tile = item % tiles;
    const int64_t k = (item / tiles) % nsplit;
    const int64_t b = item / (tiles * nsplit);
    const int64_t col = (tile * 64 + lane) * VEC;
    // vector path: H % VEC == 0, so col < H implies col + VEC <= H
    const bool active = col < H;
    const int64_t s_begin = k * rows_per_split;
    const int64_t s_end = min(S, s_begin + rows_per_split);
    const In* row0 = hidden + b * S * H + col;
    const M* mrow = mask ? mask + b * S : nullptr;

    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;

    int64_t s = s_begin + wave;
    for (; s + 3 * kPoolWaves < s_end; s += 4 * kPoolWaves) {
      bool keep[4];
      In v[4][VEC];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t su = s + u * kPoolWaves;
        keep[u] = active && (!mrow || mrow[su] != 0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (keep[u])
          pool_load<CVT, VEC>(row0 + (s + u * kPoolWaves) * H, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (keep[u]) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] += CVT::cvt(v[u][e]);
        }
    }
    for (; s < s_end; s += kPoolWaves) {
      if (active && (!mrow || mrow[s] != 0)) {
        In v[VEC];
        pool_load<CVT, VEC>(row0 + s * H, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += CVT::cvt(v[e]);
      }
    }

    // combine the 4 waves in wave order
    if (wave > 0) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) lds[wave - 1][lane][e] = acc[e];
    }
    __syncthreads();
    if (wave == 0 && active) {
#pragma unroll
      for (int w = 0; w < kPoolWaves - 1; ++w)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += lds[w][lane][e];
      float* dst = ws + (b * nsplit + k) * H + col;
#pragma unroll
      for (int e = 0; e < VEC; ++e) dst[e] = acc[e];
    }
    __syncthreads();  // lds is reused by the next work item
  }
}

// Sum of `v` over the workgroup, the same value in every thread. Fixed
// shuffle tree within a wave, then the waves in order: deterministic.
__device__ __forceinline__ float pool_block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from a previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float total = red[0];
#pragma unroll
  for (int w = 1; w < kPoolWaves; ++w) total += red[w];
  return total;
}

template <typename M>
__global__ void __launch_bounds__(kPoolBlock) masked_pool_finalize_kernel(
    const float* __restrict__ ws, const M* __restrict__ mask,
    float* __restrict__ out, int64_t B, int64_t S, int64_t H,
    int64_t nsplit, bool normalize) {
  __shared__ float red[kPoolWaves];
  __shared__ int cnt_red[kPoolWaves];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    int64_t cnt = S;
    if (mask) {
      int c = 0;
      for (int64_t s = threadIdx.x; s < S; s += kPoolBlock)
        c += mask[b * S + s] != 0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
      __syncthreads();  // cnt_red may still be read for the previous b
      if (lane == 0) cnt_red[wave] = c;
      __syncthreads();
      cnt = 0;
#pragma unroll
      for (int w = 0; w < kPoolWaves; ++w) cnt += cnt_red[w];
    }
    const float denom = float(max(cnt, int64_t(1)));
    const float* part = ws + b * nsplit * H;
    float* y = out + b * H;
    float sq = 0.f;
    for (int64_t h = threadIdx.x; h < H; h += kPoolBlock) {
      float sum = part[h];
      for (int64_t k = 1; k < nsplit; ++k) sum += part[k * H + h];
      const float mean = __fdiv_rn(sum, denom);
      y[h] = mean;
      sq += mean * mean;
    }
    if (normalize) {  // uniform across the grid
      const float norm = fmaxf(sqrtf(pool_block_sum(sq, red)), 1e-12f);
      // each thread re-reads only what it wrote itself
      for (int64_t h = threadIdx.x; h < H; h += kPoolBlock)
        y[h] = __fdiv_rn(y[h], norm);
    }
  }
}

// ---------------------------------------------------------------------------
// fused softmax + top-k classification head: [B,C] -> scores, classes [B,k]
// ---------------------------------------------------------------------------
// Order (exact, integer only): rank by float(logit) descending, equal values
// lower index first, -0.0 == +0.0, NaN above +Inf and NaNs among themselves
// by index: torch.sort(x.float(), 1, descending=True, stable=True)[:, :k].
// Every element gets a unique 64-bit key
//   key32  = monotone map of the fp32 bits (sign set: ~u, else u | 1<<31)
//            after -0.0 -> +0.0 and any NaN -> 0x7FC00000 (key 0xFFC00000,
//            above +Inf's 0xFF800000)
//   packed = (key32 << 32) | ~index
// so a larger packed key is an earlier rank. The smallest packed key (-Inf)
// is above 0 and the largest (NaN at index 0) is below ~0, which serve as
// "nothing found" and "no bound yet".
//
// Scores: m = the rank-0 logit (read back at the selected index, not an
// fmaxf), score_j = expf(x_j - m) / sum_i expf(x_i - m) in fp32 with an IEEE
// divide (`__fdiv_rn`). A row holding NaN or +Inf therefore gets NaN scores
// (m is NaN, or Inf - Inf is), a row of only -Inf too, and a -Inf logit
// under a finite maximum scores exactly 0 and ranks last.
//
// One 256-thread workgroup per row:
//  1. load: the row is read once from global memory, converted to fp32 and
//     staged in LDS when C <= kTopkLdsFloats (8192, 32 KB static). Longer
//     rows are not staged; the later passes re-read them from global memory
//     (L2-resident: the workgroup has just read them).
//  2. select: k rounds. In round j every thread takes the maximum packed key
//     of its elements that is strictly below round j-1's winner; a fixed
//     shuffle tree per wave and LDS across the 4 waves give the block-wide
//     winner. Keys are unique, so no "taken" marks are needed and k <= C
//     rounds always find one.
//  3. sum: one more pass adds expf(x_i - m) per thread in element order,
//     then the same fixed tree (pool_block_sum). The order depends only on
//     (C, path), so the output is bit-identical from run to run.
//  4. threads j < k write classes[j] and scores[j].
//
// Paths and thresholds (the tests pin one shape on each side):
//  * vector path: VEC = 16/sizeof(T) elements per lane per load (4 f32,
//    8 bf16/f16), taken iff the base pointer and C*sizeof(T) are multiples of
//    16 (then every row base is, and C % VEC == 0); otherwise scalar loads.
//    Staged rows are walked element-strided (thread t: t, t+256, ...) in
//    passes 2-3 whatever the load path; re-read rows are walked the way they
//    are loaded.
//  * C <= 8192 staged in LDS, C >= 8193 re-read.
//  * grid: min(B, 2048) workgroups (grid_for), grid-stride over rows.
//  * 1 <= k <= min(C, 64); B == 0 returns without launching.
constexpr int kTopkBlock = 256;          // 4 waves, as pool_block_sum expects
constexpr int kTopkMaxK = 64;
constexpr int kTopkLdsFloats = 8192;     // 32 KB
static_assert(kTopkBlock == kPoolBlock, "pool_block_sum is shared");
static_assert(kTopkMaxK <= kTopkBlock, "one thread writes one rank");

__device__ __forceinline__ uint64_t topk_pack(float x, uint32_t index) {
  uint32_t u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0x7FC00000u;  // any NaN
  else if (u == 0x80000000u) u = 0u;                     // -0.0
  const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (uint64_t(key) << 32) | uint64_t(~index);
}

// Maximum of `v` over the workgroup, the same value in every thread.
__device__ __forceinline__ uint64_t topk_block_max(uint64_t v, uint64_t* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t hi = __shfl_down(uint32_t(v >> 32), off, 64);
    const uint32_t lo = __shfl_down(uint32_t(v), off, 64);
    const uint64_t o = (uint64_t(hi) << 32) | lo;
    v = o > v ? o : v;
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from the previous round
  if (lane == 0) red[wave] = v;
  __syncthreads();
  uint64_t best = red[0];
#pragma unroll
  for (int w = 1; w < kPoolWaves; ++w) best = red[w] > best ? red[w] : best;
  return best;
}

// f(index, float value) for this thread's share of a row in global memory.
template <typename CVT, int VEC, typename F>
__device__ __forceinline__ void topk_for_each_global(
    const typename CVT::In* __restrict__ row, int C, F&& f) {
  for (int v = threadIdx.x; v < C / VEC; v += kTopkBlock) {
    typename CVT::In raw[VEC];
    pool_load<CVT, VEC>(row + int64_t(v) * VEC, raw);
#pragma unroll
    for (int e = 0; e < VEC; ++e) f(v * VEC + e, CVT::cvt(raw[e]));
  }
}

// f(index, float value) for this thread's share of the row, staged or not.
template <typename CVT, int VEC, bool STAGED, typename F>
__device__ __forceinline__ void topk_for_each(
    const typename CVT::In* __restrict__ row, const float* stage, int C,
    F&& f) {
  if constexpr (STAGED) {
    for (int i = threadIdx.x; i < C; i += kTopkBlock) f(i, stage[i]);
  } else {
    topk_for_each_global<CVT, VEC>(row, C, f);
  }
}

template <typename CVT, int VEC, bool STAGED>
__global__ void __launch_bounds__(kTopkBlock) softmax_topk_kernel(
    const typename CVT::In* __restrict__ logits, float* __restrict__ scores,
    int32_t* __restrict__ classes, int64_t B, int C, int k) {
  __shared__ __attribute__((aligned(16)))
      float stage[STAGED ? kTopkLdsFloats : 1];
  __shared__ uint64_t win[kTopkMaxK];
  __shared__ uint64_t red_max[kPoolWaves];
  __shared__ float red_sum[kPoolWaves];
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const typename CVT::In* row = logits + b * C;
    if constexpr (STAGED) {
      // the previous row's readers of `stage` and `win` are done
      __syncthreads();
      topk_for_each_global<CVT, VEC>(
          row, C, [&](int i, float x) { stage[i] = x; });
      __syncthreads();
    }
    auto value_at = [&](uint32_t i) -> float {
      if constexpr (STAGED) return stage[i];
      else return CVT::cvt(row[i]);
    };

    uint64_t prev = ~uint64_t(0), first = 0;
    for (int j = 0; j < k; ++j) {
      uint64_t best = 0;
      topk_for_each<CVT, VEC, STAGED>(row, stage, C, [&](int i, float x) {
        const uint64_t c = topk_pack(x, uint32_t(i));
        if (c < prev && c > best) best = c;
      });
      prev = topk_block_max(best, red_max);
      if (j == 0) first = prev;
      // win[j] of the previous row was last read before this round's
      // barriers; this row's readers wait for those of pool_block_sum
      if (threadIdx.x == 0) win[j] = prev;
    }

    const float m = value_at(~uint32_t(first));
    float part = 0.f;
    topk_for_each<CVT, VEC, STAGED>(row, stage, C, [&](int, float x) {
      part += expf(x - m);
    });
    const float total = pool_block_sum(part, red_sum);
    if (int(threadIdx.x) < k) {
      const uint32_t idx = ~uint32_t(win[threadIdx.x]);
      scores[b * k + threadIdx.x] = __fdiv_rn(expf(value_at(idx) - m), total);
      classes[b * k + threadIdx.x] = int32_t(idx);
    }
  }
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------

static inline int grid_for(int64_t work_items, int block) {
  // memory-bound grid sizing (G11): cap at 2048 blocks, grid-stride rest
  int64_t blocks = (work_items + block - 1) / block;
  return int(std::min<int64_t>(blocks, 2048));
}

static hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

template <typename CVT>
static void launch_cast(const at::Tensor& in, at::Tensor& out) {
  const int64_t n = in.numel();
  constexpr int UNROLL = 1;  // 16B loads/lane (32B measured 16% SLOWER
                             // on MI355X: 3.82 vs 4.55 TB/s bf16->f32)
  constexpr int V = UNROLL * 16 / sizeof(typename CVT::In);
  const int block = 256;
  const int grid = grid_for((n + V - 1) / V, block);
  hipLaunchKernelGGL((cast_kernel<CVT, UNROLL>), dim3(grid), dim3(block),
                     0, current_stream(),
                     reinterpret_cast<const typename CVT::In*>(
                         in.const_data_ptr()),
                     reinterpret_cast<typename CVT::Out*>(
                         out.mutable_data_ptr()),
                     n);
  HIP_CHECK(hipGetLastError());
}

template <typename CVT>
static void launch_nchw_nhwc(const at::Tensor& in, at::Tensor& out,
                             int64_t N, int64_t C, int64_t HW) {
  if (C <= 4) {
    const int block = 256;
    const int64_t hw_chunks = (HW + 7) / 8;
    const int grid = grid_for(N * hw_chunks, block);
    auto* src = reinterpret_cast<const typename CVT::In*>(
        in.const_data_ptr());
    auto* dst = reinterpret_cast<typename CVT::Out*>(
        out.mutable_data_ptr());
    switch (C) {
      case 1:
        hipLaunchKernelGGL((nchw_nhwc_smallc_kernel<CVT, 1, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
        break;
      case 2:
        hipLaunchKernelGGL((nchw_nhwc_smallc_kernel<CVT, 2, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
        break;
      case 3:
        hipLaunchKernelGGL((nchw_nhwc_smallc_kernel<CVT, 3, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
        break;
      default:
        hipLaunchKernelGGL((nchw_nhwc_smallc_kernel<CVT, 4, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
    }
  } else if (C <= 8) {
    const int block = 256;
    const int64_t hw_chunks = (HW + 3) / 4;
    const int grid = grid_for(N * hw_chunks, block);
    hipLaunchKernelGGL((nchw_nhwc_midc_kernel<CVT, 8>), dim3(grid),
                       dim3(block), 0, current_stream(),
                       reinterpret_cast<const typename CVT::In*>(
                           in.const_data_ptr()),
                       reinterpret_cast<typename CVT::Out*>(
                           out.mutable_data_ptr()),
                       int(C), HW, N);
  } else {
    constexpr int TILE = 64;
    dim3 grid(unsigned((HW + TILE - 1) / TILE),
              unsigned((C + TILE - 1) / TILE), unsigned(N));
    hipLaunchKernelGGL(nchw_nhwc_tiled_kernel<CVT>, grid, dim3(256), 0,
                       current_stream(),
                       reinterpret_cast<const typename CVT::In*>(
                           in.const_data_ptr()),
                       reinterpret_cast<typename CVT::Out*>(
                           out.mutable_data_ptr()),
                       C, HW, N);
  }
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// public ops (bound in native.cpp)
// ---------------------------------------------------------------------------

at::Tensor cast_op(const at::Tensor& in, at::ScalarType out_dtype) {
  TORCH_CHECK(in.is_cuda() && in.is_contiguous(),
              "cast_op expects a contiguous device tensor");
  auto out = at::empty_like(in, in.options().dtype(out_dtype));
  auto id = in.scalar_type();
  if (id == at::kBFloat16 && out_dtype == at::kFloat)
    launch_cast<Bf16ToF32>(in, out);
  else if (id == at::kHalf && out_dtype == at::kFloat)
    launch_cast<F16ToF32>(in, out);
  else if (id == at::kFloat && out_dtype == at::kBFloat16)
    launch_cast<F32ToBf16>(in, out);
  else if (id == at::kFloat && out_dtype == at::kHalf)
    launch_cast<F32ToF16>(in, out);
  else if (id == at::kBFloat16 && out_dtype == at::kHalf)
    launch_cast<Bf16ToF16>(in, out);
  else if (id == at::kHalf && out_dtype == at::kBFloat16)
    launch_cast<F16ToBf16>(in, out);
  else if (id == out_dtype)
    out.copy_(in);
  else
    TORCH_CHECK(false, "cast_op: unsupported dtype pair");
  return out;
}

// Fused NCHW->NHWC with optional cast (BASELINE config 5: bf16 NCHW in,
// fp32 NHWC out, one kernel).
at::Tensor nchw_to_nhwc(const at::Tensor& in, at::ScalarType out_dtype) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 4 && in.is_contiguous(),
              "nchw_to_nhwc expects a contiguous 4-D device tensor");
  const int64_t N = in.size(0), C = in.size(1), H = in.size(2),
                W = in.size(3);
  const int64_t HW = H * W;
  auto out = at::empty({N, H, W, C}, in.options().dtype(out_dtype));
  auto id = in.scalar_type();
  if (id == at::kBFloat16 && out_dtype == at::kFloat)
    launch_nchw_nhwc<Bf16ToF32>(in, out, N, C, HW);
  else if (id == at::kHalf && out_dtype == at::kFloat)
    launch_nchw_nhwc<F16ToF32>(in, out, N, C, HW);
  else if (id == at::kFloat && out_dtype == at::kFloat)
    launch_nchw_nhwc<IdF32>(in, out, N, C, HW);
  else if (id == at::kFloat && out_dtype == at::kBFloat16)
    launch_nchw_nhwc<F32ToBf16>(in, out, N, C, HW);
  else
    TORCH_CHECK(false, "nchw_to_nhwc: unsupported dtype pair");
  return out;
}

// Inverse layout transform: NHWC -> NCHW with optional cast (the unpack
// direction: responses arrive NHWC fp32, models want NCHW bf16).
at::Tensor nhwc_to_nchw(const at::Tensor& in, at::ScalarType out_dtype) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 4 && in.is_contiguous(),
              "nhwc_to_nchw expects a contiguous 4-D device tensor [N,H,W,C]");
  const int64_t N = in.size(0), H = in.size(1), W = in.size(2),
                C = in.size(3);
  const int64_t HW = H * W;
  auto out = at::empty({N, C, H, W}, in.options().dtype(out_dtype));
  auto id = in.scalar_type();

  auto launch_small = [&](auto cvt_tag) {
    using CVT = decltype(cvt_tag);
    const int block = 256;
    const int64_t hw_chunks = (HW + 7) / 8;
    const int grid = grid_for(N * hw_chunks, block);
    auto* src = reinterpret_cast<const typename CVT::In*>(
        in.const_data_ptr());
    auto* dst = reinterpret_cast<typename CVT::Out*>(
        out.mutable_data_ptr());
    switch (C) {
      case 1:
        hipLaunchKernelGGL((nhwc_nchw_smallc_kernel<CVT, 1, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
        break;
      case 2:
        hipLaunchKernelGGL((nhwc_nchw_smallc_kernel<CVT, 2, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
        break;
      case 3:
        hipLaunchKernelGGL((nhwc_nchw_smallc_kernel<CVT, 3, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
        break;
      default:
        hipLaunchKernelGGL((nhwc_nchw_smallc_kernel<CVT, 4, 8>), dim3(grid),
                           dim3(block), 0, current_stream(), src, dst, HW, N);
    }
  };
  auto launch_tiled = [&](auto cvt_tag) {
    using CVT = decltype(cvt_tag);
    // generic batched 2-D transpose: input rows = HW, cols = C
    constexpr int TILE = 64;
    dim3 grid(unsigned((C + TILE - 1) / TILE),
              unsigned((HW + TILE - 1) / TILE), unsigned(N));
    hipLaunchKernelGGL(nchw_nhwc_tiled_kernel<CVT>, grid, dim3(256), 0,
                       current_stream(),
                       reinterpret_cast<const typename CVT::In*>(
                           in.const_data_ptr()),
                       reinterpret_cast<typename CVT::Out*>(
                           out.mutable_data_ptr()),
                       /*C=*/HW, /*HW=*/C, N);
  };

  auto dispatch = [&](auto cvt_tag) {
    if (C <= 4) launch_small(cvt_tag);
    else launch_tiled(cvt_tag);
  };
  if (id == at::kFloat && out_dtype == at::kBFloat16)
    dispatch(F32ToBf16{});
  else if (id == at::kFloat && out_dtype == at::kFloat)
    dispatch(IdF32{});
  else if (id == at::kBFloat16 && out_dtype == at::kFloat)
    dispatch(Bf16ToF32{});
  else if (id == at::kHalf && out_dtype == at::kFloat)
    dispatch(F16ToF32{});
  else
    TORCH_CHECK(false, "nhwc_to_nchw: unsupported dtype pair");
  HIP_CHECK(hipGetLastError());
  return out;
}

// Fused uint8 NHWC image ingest: dequantize + per-channel normalize, out in
// f32/bf16/f16, NCHW or NHWC. `scale`/`bias` hold one value per channel,
// already rounded to fp32 by the caller (ops.normalization_constants).
at::Tensor u8_nhwc_normalize(const at::Tensor& in, std::vector<double> scale,
                             std::vector<double> bias,
                             at::ScalarType out_dtype, bool out_nchw) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 4 && in.is_contiguous() &&
              in.scalar_type() == at::kByte,
              "u8_nhwc_normalize expects a contiguous uint8 device tensor "
              "[N,H,W,C]");
  const int64_t N = in.size(0), H = in.size(1), W = in.size(2),
                C = in.size(3);
  TORCH_CHECK(C >= 1 && C <= 4, "u8_nhwc_normalize: C must be in 1..4");
  TORCH_CHECK(int64_t(scale.size()) == C && int64_t(bias.size()) == C,
              "u8_nhwc_normalize: scale/bias need one value per channel");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
              out_dtype == at::kHalf,
              "u8_nhwc_normalize: out_dtype must be f32, bf16 or f16");
  const int64_t HW = H * W;
  auto out = out_nchw
      ? at::empty({N, C, H, W}, in.options().dtype(out_dtype))
      : at::empty({N, H, W, C}, in.options().dtype(out_dtype));
  if (N * HW == 0) return out;  // grid_for(0) is a zero grid: never launch

  U8NormParams p{};
  for (int64_t c = 0; c < C; ++c) {
    p.scale[c] = float(scale[c]);
    p.bias[c] = float(bias[c]);
  }
  // pixels per lane: 8 (C=3: 24 B/lane as 3x 8 B loads) measured FASTER
  // than 16 (3x 16 B loads) on MI355X, interleaved rounds in one process,
  // u8 NHWC -> NCHW:  (32,224,224,3)  f32 6.9 vs 9.7 us, bf16 5.0 vs 5.2 us;
  //                  (256,224,224,3) f32 29.7 vs 49.6 us, bf16 19.5 vs
  // 20.4 us. 16 px/lane holds 48 fp32 results per lane and issues 12
  // stores per lane back to back; 8 px/lane doubles the lanes in flight.
  constexpr int HWPL = 8;
  const int block = 256;
  const int grid = grid_for(N * ((HW + HWPL - 1) / HWPL), block);
  const auto* src = static_cast<const uint8_t*>(in.const_data_ptr());

  auto launch = [&](auto cvt_tag, auto c_tag, auto nchw_tag) {
    using CVT = decltype(cvt_tag);
    hipLaunchKernelGGL(
        (u8_nhwc_normalize_kernel<CVT, decltype(c_tag)::value, HWPL,
                                  decltype(nchw_tag)::value>),
        dim3(grid), dim3(block), 0, current_stream(), src,
        reinterpret_cast<typename CVT::Out*>(out.mutable_data_ptr()), HW, N,
        p);
  };
  auto by_layout = [&](auto cvt_tag, auto c_tag) {
    if (out_nchw) launch(cvt_tag, c_tag, std::true_type{});
    else launch(cvt_tag, c_tag, std::false_type{});
  };
  auto by_channels = [&](auto cvt_tag) {
    switch (C) {
      case 1: by_layout(cvt_tag, std::integral_constant<int, 1>{}); break;
      case 2: by_layout(cvt_tag, std::integral_constant<int, 2>{}); break;
      case 3: by_layout(cvt_tag, std::integral_constant<int, 3>{}); break;
      default: by_layout(cvt_tag, std::integral_constant<int, 4>{});
    }
  };
  if (out_dtype == at::kFloat) by_channels(IdF32{});
  else if (out_dtype == at::kBFloat16) by_channels(F32ToBf16{});
  else by_channels(F32ToF16{});
  HIP_CHECK(hipGetLastError());
  return out;
}

// Fused uint8 NHWC ingest with bilinear resize + crop; see the kernel section
// for semantics and paths. `rh`/`rw` are float(Hin/Hr) and float(Win/Wr),
// `scale`/`bias` as in u8_nhwc_normalize, all rounded to fp32 by the caller
// (ops.image_u8_resize_to_float, which also validates the crop window
// against the resized size). `variant` 0 picks the tap path per tile, 1
// forces the direct path (for measurement).
at::Tensor u8_nhwc_resize_normalize(
    const at::Tensor& in, double rh, double rw, int64_t top, int64_t left,
    int64_t Hc, int64_t Wc, std::vector<double> scale,
    std::vector<double> bias, at::ScalarType out_dtype, bool out_nchw,
    int64_t variant) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 4 && in.is_contiguous() &&
              in.scalar_type() == at::kByte,
              "u8_nhwc_resize_normalize expects a contiguous uint8 device "
              "tensor [N,H,W,C]");
  const int64_t N = in.size(0), Hin = in.size(1), Win = in.size(2),
                C = in.size(3);
  constexpr int64_t kMaxSide = 16384;
  TORCH_CHECK(C >= 1 && C <= 4, "u8_nhwc_resize_normalize: C must be in 1..4");
  TORCH_CHECK(Hin >= 1 && Hin <= kMaxSide && Win >= 1 && Win <= kMaxSide,
              "u8_nhwc_resize_normalize: input sides must be in 1..16384");
  TORCH_CHECK(Hc >= 1 && Wc >= 1 && top >= 0 && left >= 0 &&
              top + Hc <= kMaxSide && left + Wc <= kMaxSide,
              "u8_nhwc_resize_normalize: bad crop window");
  TORCH_CHECK(rh > 0.0 && rw > 0.0,
              "u8_nhwc_resize_normalize: ratios must be positive");
  TORCH_CHECK(int64_t(scale.size()) == C && int64_t(bias.size()) == C,
              "u8_nhwc_resize_normalize: scale/bias need one value per "
              "channel");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
              out_dtype == at::kHalf,
              "u8_nhwc_resize_normalize: out_dtype must be f32, bf16 or f16");
  auto out = out_nchw
      ? at::empty({N, C, Hc, Wc}, in.options().dtype(out_dtype))
      : at::empty({N, Hc, Wc, C}, in.options().dtype(out_dtype));
  if (N == 0) return out;  // zero grid: never launch

  U8ResizeParams p{};
  for (int64_t c = 0; c < C; ++c) {
    p.scale[c] = float(scale[c]);
    p.bias[c] = float(bias[c]);
  }
  p.rh = float(rh);
  p.rw = float(rw);
  p.Hin = int(Hin); p.Win = int(Win);
  p.Hc = int(Hc); p.Wc = int(Wc);
  p.top = int(top); p.left = int(left);
  // tile: the narrowest power-of-two count of lane runs that covers a row,
  // within 8..32 runs (64..256 columns, 32..8 rows)
  const int64_t runs = (Wc + kResizePx - 1) / kResizePx;
  p.twl_log2 = kResizeMinTwlLog2;
  while (p.twl_log2 < kResizeMaxTwlLog2 && (int64_t(1) << p.twl_log2) < runs)
    ++p.twl_log2;
  const int64_t tw = (int64_t(1) << p.twl_log2) * kResizePx;
  const int64_t tr = kResizeBlock >> p.twl_log2;
  p.tiles_x = int((Wc + tw - 1) / tw);
  p.tiles_y = int((Hc + tr - 1) / tr);
  // LDS bytes per source-row span: the widest span of a tile (an upper
  // estimate; the kernel checks each tile's own span against it) plus up to
  // 15 bytes of misalignment, in whole 16 B chunks
  const int64_t span_px = std::min<int64_t>(
      Win, int64_t(std::ceil(double(std::min(tw, Wc)) * double(p.rw))) + 3);
  const int64_t span_stride = (span_px * C + 15 + 15) / 16 * 16;
  p.span_stride =
      (variant == 1 || 2 * tr * span_stride > kResizeLdsBytes)
          ? 0 : int(span_stride);

  // taps from LDS measured FASTER than the direct gather (variant 1) on
  // MI355X, interleaved rounds in one process, u8 (N,256,341,3) -> NCHW,
  // LDS vs direct:
  //   224 centre crop  N=32  f32 10.8 vs 14.3 us, bf16 10.0 vs 17.2 us
  //                    N=256 f32 47.8 vs 74.0 us, bf16 50.2 vs 99.2 us
  //   2x downscale     N=32  bf16 8.7 vs 13.2 us
  // At N=1 both sit on the launch floor (5.6-7.7 us, direct 0.6-0.9 us
  // ahead with the crop). The LDS path ships wherever its spans fit.
  const int64_t items = N * p.tiles_y * p.tiles_x;
  const int grid = int(std::min<int64_t>(items, 2048));
  const auto* src = static_cast<const uint8_t*>(in.const_data_ptr());

  auto launch = [&](auto cvt_tag, auto c_tag, auto nchw_tag) {
    using CVT = decltype(cvt_tag);
    hipLaunchKernelGGL(
        (u8_nhwc_resize_normalize_kernel<CVT, decltype(c_tag)::value,
                                         decltype(nchw_tag)::value>),
        dim3(grid), dim3(kResizeBlock), 0, current_stream(), src,
        reinterpret_cast<typename CVT::Out*>(out.mutable_data_ptr()), N, p);
  };
  auto by_layout = [&](auto cvt_tag, auto c_tag) {
    if (out_nchw) launch(cvt_tag, c_tag, std::true_type{});
    else launch(cvt_tag, c_tag, std::false_type{});
  };
  auto by_channels = [&](auto cvt_tag) {
    switch (C) {
      case 1: by_layout(cvt_tag, std::integral_constant<int, 1>{}); break;
      case 2: by_layout(cvt_tag, std::integral_constant<int, 2>{}); break;
      case 3: by_layout(cvt_tag, std::integral_constant<int, 3>{}); break;
      default: by_layout(cvt_tag, std::integral_constant<int, 4>{});
    }
  };
  if (out_dtype == at::kFloat) by_channels(IdF32{});
  else if (out_dtype == at::kBFloat16) by_channels(F32ToBf16{});
  else by_channels(F32ToF16{});
  HIP_CHECK(hipGetLastError());
  return out;
}

// YUV 4:2:0 source side of the fused bilinear resize + crop ingest; see the
// kernel section. `in` is uint8 [N, Hin*3/2, Win] with Hin and Win even
// (validated by ops.image_yuv420_resize_to_float, like the crop window),
// `i420` picks planar chroma over NV12's interleaved pairs and `coef` is
// (yoff, yc, rv, gu, gv, bu) of the int32 conversion. The other arguments are
// those of u8_nhwc_resize_normalize with C = 3.
at::Tensor yuv420_resize_normalize(
    const at::Tensor& in, bool i420, std::vector<int64_t> coef, double rh,
    double rw, int64_t top, int64_t left, int64_t Hc, int64_t Wc,
    std::vector<double> scale, std::vector<double> bias,
    at::ScalarType out_dtype, bool out_nchw, int64_t variant) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 3 && in.is_contiguous() &&
              in.scalar_type() == at::kByte,
              "yuv420_resize_normalize expects a contiguous uint8 device "
              "tensor [N,H*3/2,W]");
  constexpr int64_t kMaxSide = 16384;
  constexpr int64_t C = 3;
  const int64_t N = in.size(0), Win = in.size(2);
  TORCH_CHECK(in.size(1) % 3 == 0,
              "yuv420_resize_normalize: rows must be a multiple of 3");
  const int64_t Hin = in.size(1) / 3 * 2;
  TORCH_CHECK(Hin >= 2 && Hin <= kMaxSide && Win >= 2 && Win <= kMaxSide &&
              Hin % 2 == 0 && Win % 2 == 0,
              "yuv420_resize_normalize: frame sides must be even and in "
              "2..16384");
  TORCH_CHECK(Hc >= 1 && Wc >= 1 && top >= 0 && left >= 0 &&
              top + Hc <= kMaxSide && left + Wc <= kMaxSide,
              "yuv420_resize_normalize: bad crop window");
  TORCH_CHECK(rh > 0.0 && rw > 0.0,
              "yuv420_resize_normalize: ratios must be positive");
  TORCH_CHECK(int64_t(scale.size()) == C && int64_t(bias.size()) == C,
              "yuv420_resize_normalize: scale/bias need 3 values");
  TORCH_CHECK(coef.size() == 6,
              "yuv420_resize_normalize: coef needs 6 values");
  for (int64_t v : coef)   // sums stay far inside int32
    TORCH_CHECK(v >= -4096 && v <= 4096,
                "yuv420_resize_normalize: coefficient out of range");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
              out_dtype == at::kHalf,
              "yuv420_resize_normalize: out_dtype must be f32, bf16 or f16");
  auto out = out_nchw
      ? at::empty({N, C, Hc, Wc}, in.options().dtype(out_dtype))
      : at::empty({N, Hc, Wc, C}, in.options().dtype(out_dtype));
  if (N == 0) return out;  // zero grid: never launch

  Yuv420ResizeParams pp{};
  U8ResizeParams& p = pp.r;
  for (int64_t c = 0; c < C; ++c) {
    p.scale[c] = float(scale[c]);
    p.bias[c] = float(bias[c]);
  }
  pp.k = Yuv420Coef{int(coef[0]), int(coef[1]), int(coef[2]), int(coef[3]),
                    int(coef[4]), int(coef[5])};
  p.rh = float(rh);
  p.rw = float(rw);
  p.Hin = int(Hin); p.Win = int(Win);
  p.Hc = int(Hc); p.Wc = int(Wc);
  p.top = int(top); p.left = int(left);
  // tile geometry from Wc, as in u8_nhwc_resize_normalize
  const int64_t runs = (Wc + kResizePx - 1) / kResizePx;
  p.twl_log2 = kResizeMinTwlLog2;
  while (p.twl_log2 < kResizeMaxTwlLog2 && (int64_t(1) << p.twl_log2) < runs)
    ++p.twl_log2;
  const int64_t tw = (int64_t(1) << p.twl_log2) * kResizePx;
  const int64_t tr = kResizeBlock >> p.twl_log2;
  p.tiles_x = int((Wc + tw - 1) / tw);
  p.tiles_y = int((Hc + tr - 1) / tr);
  // pixels per LDS span: the widest span of a tile (an upper estimate; the
  // kernel checks each tile's own span against it) plus one for the even
  // start column, in whole fill chunks of 3 LDS bytes per pixel
  const int64_t span_px = std::min<int64_t>(
      Win, int64_t(std::ceil(double(std::min(tw, Wc)) * double(p.rw))) + 3);
  const int64_t chunks = (span_px + 1 + kYuvChunkPx - 1) / kYuvChunkPx;
  const int64_t span_stride = chunks * kYuvChunkPx * C;
  const bool direct =
      variant == 1 || 2 * tr * span_stride > kResizeLdsBytes;
  p.span_stride = direct ? 0 : int(span_stride);
  pp.span_px = direct ? 0 : int(chunks * kYuvChunkPx);

  const int64_t items = N * p.tiles_y * p.tiles_x;
  const int grid = int(std::min<int64_t>(items, 2048));
  const auto* src = static_cast<const uint8_t*>(in.const_data_ptr());

  auto launch = [&](auto cvt_tag, auto nchw_tag, auto i420_tag) {
    using CVT = decltype(cvt_tag);
    hipLaunchKernelGGL(
        (yuv420_resize_normalize_kernel<CVT, decltype(nchw_tag)::value,
                                        decltype(i420_tag)::value>),
        dim3(grid), dim3(kResizeBlock), 0, current_stream(), src,
        reinterpret_cast<typename CVT::Out*>(out.mutable_data_ptr()), N, pp);
  };
  auto by_chroma = [&](auto cvt_tag, auto nchw_tag) {
    if (i420) launch(cvt_tag, nchw_tag, std::true_type{});
    else launch(cvt_tag, nchw_tag, std::false_type{});
  };
  auto by_layout = [&](auto cvt_tag) {
    if (out_nchw) by_chroma(cvt_tag, std::true_type{});
    else by_chroma(cvt_tag, std::false_type{});
  };
  if (out_dtype == at::kFloat) by_layout(IdF32{});
  else if (out_dtype == at::kBFloat16) by_layout(F32ToBf16{});
  else by_layout(F32ToF16{});
  HIP_CHECK(hipGetLastError());
  return out;
}

// Ragged batch of the fused bilinear resize + crop ingest; see the kernel
// section. `in` is the flat uint8 buffer of N images back to back, `table`
// the int32 [N,8] device image of U8RaggedEntry rows, already on the device
// (ops.image_u8_ragged_resize_to_float builds it on the host, validates every
// entry against the buffer size, and copies it on the current stream from a
// pinned buffer). The kernel trusts the table: callers other than that op
// must make the same checks.
//
// Measured on MI355X (tools/bench_ragged.py, interleaved rounds in one
// process, median [range]), N photos of mixed sizes (256..512 x 341..683),
// u8 -> bf16 NCHW, short side 256, 224 centre crop. The reference is what
// the op replaces: a Python loop of N dense image_u8_resize_to_float calls
// plus torch.cat.
//   N=32  this entry on a device-resident table 11.1 us [11.0-11.4]
//         whole Python op (table built + copied)  34.2 us [34.0-35.6]
//         loop of 32 dense calls + cat           301.1 us [297.6-302.3]
//         dense kernel, 32 images of ONE size     11.3 us [11.2-11.5]
//   N=1   this entry 8.4 us, whole op 32.5 us, one dense call 14.3 us
// The table costs the kernel nothing measurable. The op's cost is on the
// host: about 23 us per call for the checks, the numpy table and the pinned
// copy, nearly independent of N (host clock per call 33-35 us), plus about
// 20 us when the shapes arrive as a device tensor (synchronizing D2H). So
// the op is 8.8x faster than the loop at N = 32 and SLOWER than a single
// dense call at N = 1.
at::Tensor u8_ragged_resize_normalize(
    const at::Tensor& in, const at::Tensor& table, int64_t C, int64_t Hc,
    int64_t Wc, std::vector<double> scale, std::vector<double> bias,
    at::ScalarType out_dtype, bool out_nchw) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 1 && in.is_contiguous() &&
              in.scalar_type() == at::kByte,
              "u8_ragged_resize_normalize expects a contiguous 1-D uint8 "
              "device tensor");
  TORCH_CHECK(table.is_cuda() && table.get_device() == in.get_device() &&
              table.dim() == 2 && table.size(1) == 8 &&
              table.is_contiguous() && table.scalar_type() == at::kInt,
              "u8_ragged_resize_normalize: table must be a contiguous int32 "
              "[N,8] tensor on the device of the input");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(table.const_data_ptr()) % 8 == 0,
              "u8_ragged_resize_normalize: table must be 8 B-aligned");
  constexpr int64_t kMaxSide = 16384;
  TORCH_CHECK(C >= 1 && C <= 4,
              "u8_ragged_resize_normalize: C must be in 1..4");
  TORCH_CHECK(Hc >= 1 && Wc >= 1 && Hc <= kMaxSide && Wc <= kMaxSide,
              "u8_ragged_resize_normalize: bad output size");
  TORCH_CHECK(int64_t(scale.size()) == C && int64_t(bias.size()) == C,
              "u8_ragged_resize_normalize: scale/bias need one value per "
              "channel");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
              out_dtype == at::kHalf,
              "u8_ragged_resize_normalize: out_dtype must be f32, bf16 or "
              "f16");
  const int64_t N = table.size(0);
  auto out = out_nchw
      ? at::empty({N, C, Hc, Wc}, in.options().dtype(out_dtype))
      : at::empty({N, Hc, Wc, C}, in.options().dtype(out_dtype));
  if (N == 0) return out;  // zero grid: never launch

  U8ResizeParams p{};      // the source-side fields come from the table
  for (int64_t c = 0; c < C; ++c) {
    p.scale[c] = float(scale[c]);
    p.bias[c] = float(bias[c]);
  }
  p.Hc = int(Hc); p.Wc = int(Wc);
  // tile geometry from Wc, as in u8_nhwc_resize_normalize
  const int64_t runs = (Wc + kResizePx - 1) / kResizePx;
  p.twl_log2 = kResizeMinTwlLog2;
  while (p.twl_log2 < kResizeMaxTwlLog2 && (int64_t(1) << p.twl_log2) < runs)
    ++p.twl_log2;
  const int64_t tw = (int64_t(1) << p.twl_log2) * kResizePx;
  const int64_t tr = kResizeBlock >> p.twl_log2;
  p.tiles_x = int((Wc + tw - 1) / tw);
  p.tiles_y = int((Hc + tr - 1) / tr);

  const int64_t items = N * p.tiles_y * p.tiles_x;
  const int grid = int(std::min<int64_t>(items, 2048));
  const auto* src = static_cast<const uint8_t*>(in.const_data_ptr());
  const auto* tab = static_cast<const U8RaggedEntry*>(table.const_data_ptr());
  const int64_t in_bytes = in.numel();

  auto launch = [&](auto cvt_tag, auto c_tag, auto nchw_tag) {
    using CVT = decltype(cvt_tag);
    hipLaunchKernelGGL(
        (u8_ragged_resize_normalize_kernel<CVT, decltype(c_tag)::value,
                                           decltype(nchw_tag)::value>),
        dim3(grid), dim3(kResizeBlock), 0, current_stream(), src, in_bytes,
        tab, reinterpret_cast<typename CVT::Out*>(out.mutable_data_ptr()), N,
        p);
  };
  auto by_layout = [&](auto cvt_tag, auto c_tag) {
    if (out_nchw) launch(cvt_tag, c_tag, std::true_type{});
    else launch(cvt_tag, c_tag, std::false_type{});
  };
  auto by_channels = [&](auto cvt_tag) {
    switch (C) {
      case 1: by_layout(cvt_tag, std::integral_constant<int, 1>{}); break;
      case 2: by_layout(cvt_tag, std::integral_constant<int, 2>{}); break;
      case 3: by_layout(cvt_tag, std::integral_constant<int, 3>{}); break;
      default: by_layout(cvt_tag, std::integral_constant<int, 4>{});
    }
  };
  if (out_dtype == at::kFloat) by_channels(IdF32{});
  else if (out_dtype == at::kBFloat16) by_channels(F32ToBf16{});
  else by_channels(F32ToF16{});
  HIP_CHECK(hipGetLastError());
  return out;
}

// uint8 NHWC ingest with antialiased resize + crop; see the kernel section
// for semantics and paths. Arguments as u8_nhwc_resize_normalize.
// `ws_cap_bytes` > 0 overrides the workspace cap (tests reach the chunked
// loop with it at tiny shapes); a chunk always holds at least one image.
//
// The cap, 256 MiB: the workspace of a (1080,1920) photo shrunk to short
// side 256 with the 224 centre crop is 950 rows x 224 columns x 3 floats,
// 2.55 MB, so a hundred such images still run as one chunk, and the block is
// 0.1 % of the 288 GB of HBM. Beyond it the launches (microseconds each) are
// noise against the filtering a chunk of that size holds.
//
// Measured on MI355X, interleaved rounds in one process, u8 -> bf16 NCHW,
// this path vs the eager device chain (permute+float, F.interpolate with
// antialias=True, slice, normalize, cast) vs the bilinear kernel above:
//   (32,1080,1920,3) -> (256,455), 224 crop   93.4 vs 1820.5 vs 57.0 us
//   (1,1080,1920,3)  -> (256,455), 224 crop   12.2 vs   72.2 vs  8.2 us
//   (32,256,341,3)   -> (128,170)             38.0 vs  106.1 vs 10.8 us
// The horizontal pass gathers its taps from global memory; staging the
// source spans through LDS has not been tried here, so there is no second
// number (the YUV horizontal pass stages: see yuv420_resize_aa_normalize).
constexpr int64_t kResizeAAWsBytes = int64_t(256) << 20;

// The host side of the antialiased recipe, shared by the dense RGB and YUV
// entries: fills `p` (normalization, ratios, support and 1/support, the crop
// window, and the source rows y_base/Rs that the window needs) and returns
// the images per workspace chunk under the cap (kResizeAAWsBytes, or
// `ws_cap_bytes` when > 0; at least one image). One value per channel in
// `scale`/`bias`.
static int64_t resize_aa_plan(
    U8ResizeAAParams& p, const char* who, double rh, double rw, int64_t Hin,
    int64_t Win, int64_t top, int64_t left, int64_t Hc, int64_t Wc,
    const std::vector<double>& scale, const std::vector<double>& bias,
    int64_t N, int64_t ws_cap_bytes) {
  const int64_t C = int64_t(scale.size());
  for (int64_t c = 0; c < C; ++c) {
    p.scale[c] = float(scale[c]);
    p.bias[c] = float(bias[c]);
  }
  p.rh = float(rh);
  p.rw = float(rw);
  p.sup_h = p.rh >= 1.f ? p.rh : 1.f;
  p.sup_w = p.rw >= 1.f ? p.rw : 1.f;
  p.inv_h = p.rh >= 1.f ? float(1.0 / double(p.rh)) : 1.f;
  p.inv_w = p.rw >= 1.f ? float(1.0 / double(p.rw)) : 1.f;
  p.Hin = int(Hin); p.Win = int(Win);
  p.Hc = int(Hc); p.Wc = int(Wc);
  p.top = int(top); p.left = int(left);
  // source rows of the crop window: [lo(first row), lo(last) + size(last))
  float unused_c;
  int lo_first, lo_last, size_first, size_last;
  aa_span(p.top, p.rh, p.sup_h, p.Hin, unused_c, lo_first, size_first);
  aa_span(p.top + p.Hc - 1, p.rh, p.sup_h, p.Hin, unused_c, lo_last,
          size_last);
  p.y_base = lo_first;
  p.Rs = lo_last + size_last - lo_first;
  TORCH_CHECK(p.Rs >= 1 && p.y_base + p.Rs <= p.Hin, who,
              ": internal row range error");

  const int64_t cap = ws_cap_bytes > 0 ? ws_cap_bytes : kResizeAAWsBytes;
  const int64_t img_floats = int64_t(p.Rs) * Wc * C;
  return std::max<int64_t>(
      1, std::min<int64_t>(N, cap / (img_floats * int64_t(sizeof(float)))));
}

at::Tensor u8_nhwc_resize_aa_normalize(
    const at::Tensor& in, double rh, double rw, int64_t top, int64_t left,
    int64_t Hc, int64_t Wc, std::vector<double> scale,
    std::vector<double> bias, at::ScalarType out_dtype, bool out_nchw,
    int64_t ws_cap_bytes) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 4 && in.is_contiguous() &&
              in.scalar_type() == at::kByte,
              "u8_nhwc_resize_aa_normalize expects a contiguous uint8 device "
              "tensor [N,H,W,C]");
  const int64_t N = in.size(0), Hin = in.size(1), Win = in.size(2),
                C = in.size(3);
  constexpr int64_t kMaxSide = 16384;
  TORCH_CHECK(C >= 1 && C <= 4,
              "u8_nhwc_resize_aa_normalize: C must be in 1..4");
  TORCH_CHECK(Hin >= 1 && Hin <= kMaxSide && Win >= 1 && Win <= kMaxSide,
              "u8_nhwc_resize_aa_normalize: input sides must be in 1..16384");
  TORCH_CHECK(Hc >= 1 && Wc >= 1 && top >= 0 && left >= 0 &&
              top + Hc <= kMaxSide && left + Wc <= kMaxSide,
              "u8_nhwc_resize_aa_normalize: bad crop window");
  // a ratio is float(n_in / n_r) with both sides in 1..16384
  TORCH_CHECK(rh > 0.0 && rw > 0.0 && rh <= double(kMaxSide) &&
              rw <= double(kMaxSide),
              "u8_nhwc_resize_aa_normalize: ratios must be in (0, 16384]");
  TORCH_CHECK(int64_t(scale.size()) == C && int64_t(bias.size()) == C,
              "u8_nhwc_resize_aa_normalize: scale/bias need one value per "
              "channel");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
              out_dtype == at::kHalf,
              "u8_nhwc_resize_aa_normalize: out_dtype must be f32, bf16 or "
              "f16");
  auto out = out_nchw
      ? at::empty({N, C, Hc, Wc}, in.options().dtype(out_dtype))
      : at::empty({N, Hc, Wc, C}, in.options().dtype(out_dtype));
  if (N == 0) return out;  // zero grid: never launch

  U8ResizeAAParams p{};
  const int64_t chunk = resize_aa_plan(
      p, "u8_nhwc_resize_aa_normalize", rh, rw, Hin, Win, top, left, Hc, Wc,
      scale, bias, N, ws_cap_bytes);
  const int64_t img_floats = int64_t(p.Rs) * Wc * C;
  auto ws = at::empty({chunk * img_floats}, in.options().dtype(at::kFloat));
  const int64_t runs = (Wc + kResizePx - 1) / kResizePx;
  const int64_t in_img = Hin * Win * C, out_img = C * Hc * Wc;
  const auto* src = static_cast<const uint8_t*>(in.const_data_ptr());

  auto launch = [&](auto cvt_tag, auto c_tag, auto nchw_tag) {
    using CVT = decltype(cvt_tag);
    constexpr int CC = decltype(c_tag)::value;
    auto* dst = reinterpret_cast<typename CVT::Out*>(out.mutable_data_ptr());
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
      const int64_t n = std::min(chunk, N - n0);
      hipLaunchKernelGGL(
          (u8_resize_aa_h_kernel<CC>),
          dim3(grid_for(n * p.Rs * Wc, kResizeAABlock)), dim3(kResizeAABlock),
          0, current_stream(), src + n0 * in_img, ws.data_ptr<float>(), n, p);
      HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(
          (u8_resize_aa_v_kernel<CVT, CC, decltype(nchw_tag)::value>),
          dim3(grid_for(n * Hc * runs, kResizeAABlock)), dim3(kResizeAABlock),
          0, current_stream(), ws.data_ptr<float>(), dst + n0 * out_img, n,
          p);
      HIP_CHECK(hipGetLastError());
    }
  };
  auto by_layout = [&](auto cvt_tag, auto c_tag) {
    if (out_nchw) launch(cvt_tag, c_tag, std::true_type{});
    else launch(cvt_tag, c_tag, std::false_type{});
  };
  auto by_channels = [&](auto cvt_tag) {
    switch (C) {
      case 1: by_layout(cvt_tag, std::integral_constant<int, 1>{}); break;
      case 2: by_layout(cvt_tag, std::integral_constant<int, 2>{}); break;
      case 3: by_layout(cvt_tag, std::integral_constant<int, 3>{}); break;
      default: by_layout(cvt_tag, std::integral_constant<int, 4>{});
    }
  };
  if (out_dtype == at::kFloat) by_channels(IdF32{});
  else if (out_dtype == at::kBFloat16) by_channels(F32ToBf16{});
  else by_channels(F32ToF16{});
  return out;
}

// YUV 4:2:0 source side of the antialiased resize + crop ingest; see the
// kernel section. `in`, `i420` and `coef` are those of
// yuv420_resize_normalize, the other arguments those of
// u8_nhwc_resize_aa_normalize with C = 3; the row range, support, 1/support
// and the workspace chunking come from resize_aa_plan, so the result is
// bit-identical to that entry on the converted frames. `variant` 1 forces
// the direct tap path.
//
// Measured on MI355X (tools/bench_yuv.py --antialias, interleaved rounds in
// one process, median [range]), NV12, u8 -> bf16 NCHW: this entry with taps
// from LDS vs the direct path forced vs u8_nhwc_resize_aa_normalize on the
// already converted tensor vs ops.yuv420_to_rgb_u8 on the device followed
// by that entry:
//   (32,1080,1920) -> (256,455), 224 crop
//       119.3 [117.6-122.0] vs 126.0 [125.0-127.9] vs 89.4 vs 3739.8 us
//   (1,1080,1920)  -> (256,455), 224 crop
//        13.2 [13.2-13.5]   vs  13.6 [13.4-14.8]   vs 12.1 vs  160.4 us
//   (32,256,342)   -> (128,170)
//        41.6 [41.4-43.0]   vs  40.2 [40.2-40.8]   vs 37.6 vs  197.0 us
// The LDS path ships as the default: it is faster than the direct path on
// both 1080p shapes (6 % and 2 %), and 3 % slower at the 2x downscale of the
// small frames, where a column has about 4 taps. The fill keeps 80 of 256
// lanes busy on the 1080p tile, which is where the rest of the 2x fewer
// conversions goes; spreading a chunk over more lanes was not tried.
at::Tensor yuv420_resize_aa_normalize(
    const at::Tensor& in, bool i420, std::vector<int64_t> coef, double rh,
    double rw, int64_t top, int64_t left, int64_t Hc, int64_t Wc,
    std::vector<double> scale, std::vector<double> bias,
    at::ScalarType out_dtype, bool out_nchw, int64_t variant,
    int64_t ws_cap_bytes) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 3 && in.is_contiguous() &&
              in.scalar_type() == at::kByte,
              "yuv420_resize_aa_normalize expects a contiguous uint8 device "
              "tensor [N,H*3/2,W]");
  constexpr int64_t kMaxSide = 16384;
  constexpr int64_t C = 3;
  const int64_t N = in.size(0), Win = in.size(2);
  TORCH_CHECK(in.size(1) % 3 == 0,
              "yuv420_resize_aa_normalize: rows must be a multiple of 3");
  const int64_t Hin = in.size(1) / 3 * 2;
  TORCH_CHECK(Hin >= 2 && Hin <= kMaxSide && Win >= 2 && Win <= kMaxSide &&
              Hin % 2 == 0 && Win % 2 == 0,
              "yuv420_resize_aa_normalize: frame sides must be even and in "
              "2..16384");
  TORCH_CHECK(Hc >= 1 && Wc >= 1 && top >= 0 && left >= 0 &&
              top + Hc <= kMaxSide && left + Wc <= kMaxSide,
              "yuv420_resize_aa_normalize: bad crop window");
  // a ratio is float(n_in / n_r) with both sides in 1..16384
  TORCH_CHECK(rh > 0.0 && rw > 0.0 && rh <= double(kMaxSide) &&
              rw <= double(kMaxSide),
              "yuv420_resize_aa_normalize: ratios must be in (0, 16384]");
  TORCH_CHECK(int64_t(scale.size()) == C && int64_t(bias.size()) == C,
              "yuv420_resize_aa_normalize: scale/bias need 3 values");
  TORCH_CHECK(coef.size() == 6,
              "yuv420_resize_aa_normalize: coef needs 6 values");
  for (int64_t v : coef)   // sums stay far inside int32
    TORCH_CHECK(v >= -4096 && v <= 4096,
                "yuv420_resize_aa_normalize: coefficient out of range");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
              out_dtype == at::kHalf,
              "yuv420_resize_aa_normalize: out_dtype must be f32, bf16 or "
              "f16");
  auto out = out_nchw
      ? at::empty({N, C, Hc, Wc}, in.options().dtype(out_dtype))
      : at::empty({N, Hc, Wc, C}, in.options().dtype(out_dtype));
  if (N == 0) return out;  // zero grid: never launch

  Yuv420ResizeAAParams pp{};
  U8ResizeAAParams& p = pp.a;
  const int64_t chunk = resize_aa_plan(
      p, "yuv420_resize_aa_normalize", rh, rw, Hin, Win, top, left, Hc, Wc,
      scale, bias, N, ws_cap_bytes);
  pp.k = Yuv420Coef{int(coef[0]), int(coef[1]), int(coef[2]), int(coef[3]),
                    int(coef[4]), int(coef[5])};
  // the widest tile that pads Wc by at most 1/8, else the narrowest
  pp.tc_log2 = kYuvAAMinTcLog2;
  for (int l = kYuvAAMaxTcLog2; l > kYuvAAMinTcLog2; --l) {
    const int64_t tcl = int64_t(1) << l;
    if ((Wc + tcl - 1) / tcl * tcl - Wc <= Wc / 8) {
      pp.tc_log2 = l;
      break;
    }
  }
  const int64_t tc = int64_t(1) << pp.tc_log2;
  const int64_t tr = kResizeAABlock >> pp.tc_log2;
  pp.tiles_x = int((Wc + tc - 1) / tc);
  pp.tiles_y = int((p.Rs + tr - 1) / tr);
  // pixels per LDS span: the widest span of a tile, (columns - 1) * rw +
  // 2 * support + 1 rounded up with slack (an upper estimate; the kernel
  // checks each tile's own span against it), plus one for the even start
  // column, in whole fill chunks of 3 LDS bytes per pixel
  const int64_t span_px = std::min<int64_t>(
      Win, int64_t(std::ceil(double(std::min(tc, Wc)) * double(p.rw))) +
               2 * int64_t(std::ceil(double(p.sup_w))) + 3);
  const int64_t chunks = (span_px + 1 + kYuvChunkPx - 1) / kYuvChunkPx;
  const bool direct =
      variant == 1 || tr * chunks * kYuvChunkPx * C > kYuvAALdsBytes;
  pp.span_px = direct ? 0 : int(chunks * kYuvChunkPx);

  const int64_t img_floats = int64_t(p.Rs) * Wc * C;
  auto ws = at::empty({chunk * img_floats}, in.options().dtype(at::kFloat));
  const int64_t runs = (Wc + kResizePx - 1) / kResizePx;
  const int64_t in_img = Hin * Win * 3 / 2, out_img = C * Hc * Wc;
  const auto* src = static_cast<const uint8_t*>(in.const_data_ptr());

  auto launch = [&](auto cvt_tag, auto nchw_tag) {
    using CVT = decltype(cvt_tag);
    auto* dst = reinterpret_cast<typename CVT::Out*>(out.mutable_data_ptr());
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
      const int64_t n = std::min(chunk, N - n0);
      const int grid = int(std::min<int64_t>(
          n * pp.tiles_y * pp.tiles_x, 2048));
      if (i420)
        hipLaunchKernelGGL(
            (yuv420_resize_aa_h_kernel<true>), dim3(grid),
            dim3(kResizeAABlock), 0, current_stream(), src + n0 * in_img,
            ws.data_ptr<float>(), n, pp);
      else
        hipLaunchKernelGGL(
            (yuv420_resize_aa_h_kernel<false>), dim3(grid),
            dim3(kResizeAABlock), 0, current_stream(), src + n0 * in_img,
            ws.data_ptr<float>(), n, pp);
      HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(
          (u8_resize_aa_v_kernel<CVT, 3, decltype(nchw_tag)::value>),
          dim3(grid_for(n * Hc * runs, kResizeAABlock)), dim3(kResizeAABlock),
          0, current_stream(), ws.data_ptr<float>(), dst + n0 * out_img, n,
          p);
      HIP_CHECK(hipGetLastError());
    }
  };
  auto by_layout = [&](auto cvt_tag) {
    if (out_nchw) launch(cvt_tag, std::true_type{});
    else launch(cvt_tag, std::false_type{});
  };
  if (out_dtype == at::kFloat) by_layout(IdF32{});
  else if (out_dtype == at::kBFloat16) by_layout(F32ToBf16{});
  else by_layout(F32ToF16{});
  return out;
}

// Host-side plan of an antialiased ragged batch: the device table and the
// chunks. `table` is the int32 [N,8] rows of the bilinear ragged op
// (U8RaggedEntry) on the HOST. For every image the row range (y_base, Rs:
// the aa_span calls of u8_nhwc_resize_aa_normalize), its support and
// 1/support are worked out here with the dense entry's expressions, so the
// result is bit-identical to the dense entry on each image alone. The batch
// is split greedily into chunks of consecutive whole images whose workspace
// bytes, sum Rs_i*Wc*C*4, fit the cap (kResizeAAWsBytes, or `ws_cap_bytes`
// when > 0; a chunk always holds at least one image); ws_row0 restarts at 0
// in each chunk. Every image is checked against `in_bytes`, so a bad table
// is an error, never an out-of-bounds read.
struct RaggedAAChunk { int64_t n0, n, rows; };   // first image, count, rows
struct RaggedAAPlan {
  at::Tensor entries;                  // int32 [N,16]: U8RaggedAAEntry rows
  std::vector<RaggedAAChunk> chunks;
};

static RaggedAAPlan ragged_aa_plan(const at::Tensor& table, int64_t in_bytes,
                                   int64_t C, int64_t Hc, int64_t Wc,
                                   int64_t ws_cap_bytes, bool pinned) {
  TORCH_CHECK(table.is_cpu() && table.dim() == 2 && table.size(1) == 8 &&
              table.is_contiguous() && table.scalar_type() == at::kInt,
              "u8_ragged_resize_aa_normalize: table must be a contiguous "
              "int32 [N,8] tensor on the CPU");
  constexpr int64_t kMaxSide = 16384;
  TORCH_CHECK(C >= 1 && C <= 4,
              "u8_ragged_resize_aa_normalize: C must be in 1..4");
  TORCH_CHECK(Hc >= 1 && Wc >= 1 && Hc <= kMaxSide && Wc <= kMaxSide,
              "u8_ragged_resize_aa_normalize: bad output size");
  const int64_t N = table.size(0);
  TORCH_CHECK(N <= INT32_MAX,
              "u8_ragged_resize_aa_normalize: too many images");
  RaggedAAPlan plan;
  plan.entries = at::empty(
      {N, int64_t(sizeof(U8RaggedAAEntry) / sizeof(int32_t))},
      at::TensorOptions().dtype(at::kInt).pinned_memory(pinned && N > 0));
  auto* entries =
      static_cast<U8RaggedAAEntry*>(plan.entries.mutable_data_ptr());
  auto& chunks = plan.chunks;
  const int64_t cap = ws_cap_bytes > 0 ? ws_cap_bytes : kResizeAAWsBytes;
  const int64_t row_bytes = Wc * C * int64_t(sizeof(float));
  const auto* rows8 = static_cast<const int32_t*>(table.const_data_ptr());
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* r = rows8 + i * 8;
    U8RaggedAAEntry e{};
    std::memcpy(&e.offset, r, sizeof(int64_t));   // two little-endian words
    e.Hin = r[2]; e.Win = r[3]; e.top = r[4]; e.left = r[5];
    std::memcpy(&e.rh, r + 6, sizeof(float));
    std::memcpy(&e.rw, r + 7, sizeof(float));
    TORCH_CHECK(e.Hin >= 1 && e.Hin <= kMaxSide && e.Win >= 1 &&
                e.Win <= kMaxSide,
                "u8_ragged_resize_aa_normalize: image ", i,
                ": input sides must be in 1..16384");
    TORCH_CHECK(e.offset >= 0 &&
                e.offset + int64_t(e.Hin) * e.Win * C <= in_bytes,
                "u8_ragged_resize_aa_normalize: image ", i,
                " is not inside the buffer");
    TORCH_CHECK(e.top >= 0 && e.left >= 0 && e.top + Hc <= kMaxSide &&
                e.left + Wc <= kMaxSide,
                "u8_ragged_resize_aa_normalize: image ", i,
                ": bad crop window");
    // a ratio is float(n_in / n_r) with both sides in 1..16384
    TORCH_CHECK(e.rh > 0.f && e.rw > 0.f && e.rh <= float(kMaxSide) &&
                e.rw <= float(kMaxSide),
                "u8_ragged_resize_aa_normalize: image ", i,
                ": ratios must be in (0, 16384]");
    e.sup_h = e.rh >= 1.f ? e.rh : 1.f;
    e.sup_w = e.rw >= 1.f ? e.rw : 1.f;
    e.inv_h = e.rh >= 1.f ? float(1.0 / double(e.rh)) : 1.f;
    e.inv_w = e.rw >= 1.f ? float(1.0 / double(e.rw)) : 1.f;
    // source rows of the crop window: [lo(first row), lo(last) + size(last))
    float unused_c;
    int lo_first, lo_last, size_first, size_last;
    aa_span(e.top, e.rh, e.sup_h, e.Hin, unused_c, lo_first, size_first);
    aa_span(e.top + int(Hc) - 1, e.rh, e.sup_h, e.Hin, unused_c, lo_last,
            size_last);
    e.y_base = lo_first;
    e.Rs = lo_last + size_last - lo_first;
    TORCH_CHECK(e.Rs >= 1 && e.y_base + e.Rs <= e.Hin,
                "u8_ragged_resize_aa_normalize: image ", i,
                ": internal row range error");
    if (chunks.empty() || (chunks.back().rows + e.Rs) * row_bytes > cap)
      chunks.push_back({i, 0, 0});
    RaggedAAChunk& ch = chunks.back();
    e.ws_row0 = ch.rows;
    ch.n += 1;
    ch.rows += e.Rs;
    entries[i] = e;
  }
  return plan;
}

// The plan alone, for tests and tools: (entries int32 [N,16], chunks int64
// [K,3] rows of (first image, images, workspace rows)). Host only.
std::tuple<at::Tensor, at::Tensor> u8_ragged_resize_aa_plan(
    const at::Tensor& table, int64_t in_bytes, int64_t C, int64_t Hc,
    int64_t Wc, int64_t ws_cap_bytes) {
  RaggedAAPlan plan =
      ragged_aa_plan(table, in_bytes, C, Hc, Wc, ws_cap_bytes, false);
  auto chunks = at::empty({int64_t(plan.chunks.size()), 3},
                          at::TensorOptions().dtype(at::kLong));
  auto* c = chunks.data_ptr<int64_t>();
  for (const RaggedAAChunk& ch : plan.chunks) {
    *c++ = ch.n0; *c++ = ch.n; *c++ = ch.rows;
  }
  return {plan.entries, chunks};
}

// Ragged batch of the antialiased resize + crop ingest; see the kernel
// section. `in` is the flat uint8 device buffer of N images back to back,
// `table` the HOST table ragged_aa_plan reads. The device table
// (U8RaggedAAEntry rows) is built in pinned memory and copied on the current
// stream, and each chunk runs both kernels through one workspace sized for
// the largest chunk.
//
// Measured on MI355X (tools/bench_ragged.py --antialias, interleaved rounds
// in one process, median [range]), N photos of mixed sizes (256..512 x
// 341..683), u8 -> bf16 NCHW, short side 256, 224 centre crop. The reference
// is what the op replaces: a Python loop of N dense antialiased
// image_u8_resize_to_float calls plus torch.cat.
//   N=32  this entry on a pre-built host table     41.0 us [40.9-41.5]
//         whole Python op                          41.5 us [41.4-44.8]
//         loop of 32 dense antialiased calls + cat 468.0 us [464.1-472.3]
//         dense kernels, 32 images of ONE size      29.3 us [28.9-29.4]
//   N=1   this entry 21.2 us, whole op 39.6 us, one dense call 19.7 us
// So the op is 11.3x faster than the loop at N = 32, 1.4x SLOWER than the
// dense kernels on equal-size images, and slower than a single dense call
// at N = 1. Back-to-back calls are host-bound: the calling thread spends
// 42.8 us per call at N = 32 (host clock, no device wait), about what the
// device events show, so the plan, the pinned table, its copy and the two
// launches set the figure and the two kernels' own time was not resolved.
at::Tensor u8_ragged_resize_aa_normalize(
    const at::Tensor& in, const at::Tensor& table, int64_t C, int64_t Hc,
    int64_t Wc, std::vector<double> scale, std::vector<double> bias,
    at::ScalarType out_dtype, bool out_nchw, int64_t ws_cap_bytes) {
  TORCH_CHECK(in.is_cuda() && in.dim() == 1 && in.is_contiguous() &&
              in.scalar_type() == at::kByte,
              "u8_ragged_resize_aa_normalize expects a contiguous 1-D uint8 "
              "device tensor");
  RaggedAAPlan plan =
      ragged_aa_plan(table, in.numel(), C, Hc, Wc, ws_cap_bytes, true);
  TORCH_CHECK(int64_t(scale.size()) == C && int64_t(bias.size()) == C,
              "u8_ragged_resize_aa_normalize: scale/bias need one value per "
              "channel");
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
              out_dtype == at::kHalf,
              "u8_ragged_resize_aa_normalize: out_dtype must be f32, bf16 or "
              "f16");
  const int64_t N = table.size(0);
  auto out = out_nchw
      ? at::empty({N, C, Hc, Wc}, in.options().dtype(out_dtype))
      : at::empty({N, Hc, Wc, C}, in.options().dtype(out_dtype));
  if (N == 0) return out;  // zero grid: never launch

  U8ResizeAAParams p{};    // the source-side fields come from the table
  for (int64_t c = 0; c < C; ++c) {
    p.scale[c] = float(scale[c]);
    p.bias[c] = float(bias[c]);
  }
  p.Hc = int(Hc); p.Wc = int(Wc);
  const auto& chunks = plan.chunks;
  int64_t max_rows = 0;
  for (const RaggedAAChunk& ch : chunks)
    max_rows = std::max(max_rows, ch.rows);
  // pinned source: the copy is queued on the current stream and the caching
  // host allocator keeps the block until it has completed
  auto table_dev = plan.entries.to(in.device(), /*non_blocking=*/true);
  const auto* tab =
      static_cast<const U8RaggedAAEntry*>(table_dev.const_data_ptr());
  auto ws = at::empty({max_rows * Wc * C}, in.options().dtype(at::kFloat));
  const int64_t runs = (Wc + kResizePx - 1) / kResizePx;
  const int64_t out_img = C * Hc * Wc;
  const auto* src = static_cast<const uint8_t*>(in.const_data_ptr());

  auto launch = [&](auto cvt_tag, auto c_tag, auto nchw_tag) {
    using CVT = decltype(cvt_tag);
    constexpr int CC = decltype(c_tag)::value;
    auto* dst = reinterpret_cast<typename CVT::Out*>(out.mutable_data_ptr());
    for (const RaggedAAChunk& ch : chunks) {
      hipLaunchKernelGGL(
          (u8_ragged_resize_aa_h_kernel<CC>),
          dim3(grid_for(ch.rows * Wc, kResizeAABlock)), dim3(kResizeAABlock),
          0, current_stream(), src, ws.data_ptr<float>(), tab + ch.n0,
          int(ch.n), ch.rows, p);
      HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(
          (u8_ragged_resize_aa_v_kernel<CVT, CC, decltype(nchw_tag)::value>),
          dim3(grid_for(ch.n * Hc * runs, kResizeAABlock)),
          dim3(kResizeAABlock), 0, current_stream(), ws.data_ptr<float>(),
          dst + ch.n0 * out_img, tab + ch.n0, ch.n, p);
      HIP_CHECK(hipGetLastError());
    }
  };
  auto by_layout = [&](auto cvt_tag, auto c_tag) {
    if (out_nchw) launch(cvt_tag, c_tag, std::true_type{});
    else launch(cvt_tag, c_tag, std::false_type{});
  };
  auto by_channels = [&](auto cvt_tag) {
    switch (C) {
      case 1: by_layout(cvt_tag, std::integral_constant<int, 1>{}); break;
      case 2: by_layout(cvt_tag, std::integral_constant<int, 2>{}); break;
      case 3: by_layout(cvt_tag, std::integral_constant<int, 3>{}); break;
      default: by_layout(cvt_tag, std::integral_constant<int, 4>{});
    }
  };
  if (out_dtype == at::kFloat) by_channels(IdF32{});
  else if (out_dtype == at::kBFloat16) by_channels(F32ToBf16{});
  else by_channels(F32ToF16{});
  return out;
}

// Fused masked mean-pool (+ optional L2 normalize) of a [B,S,H] hidden state
// into fp32 [B,H]; see the kernel section for semantics, paths and
// thresholds. `mask` is [B,S] int32 or uint8/bool (non-zero keeps), or
// nullopt to keep every position.
at::Tensor masked_mean_pool(const at::Tensor& hidden,
                            const c10::optional<at::Tensor>& mask,
                            bool normalize) {
  TORCH_CHECK(hidden.is_cuda() && hidden.dim() == 3 && hidden.is_contiguous(),
              "masked_mean_pool expects a contiguous device tensor [B,S,H]");
  const auto id = hidden.scalar_type();
  TORCH_CHECK(id == at::kFloat || id == at::kBFloat16 || id == at::kHalf,
              "masked_mean_pool: hidden must be f32, bf16 or f16");
  const int64_t B = hidden.size(0), S = hidden.size(1), H = hidden.size(2);
  const void* mptr = nullptr;
  int mask_bytes = 0;
  if (mask.has_value()) {
    const at::Tensor& m = *mask;
    const auto md = m.scalar_type();
    TORCH_CHECK(m.is_cuda() && m.device() == hidden.device() &&
                m.dim() == 2 && m.size(0) == B && m.size(1) == S &&
                m.is_contiguous(),
                "masked_mean_pool: mask must be a contiguous [B,S] tensor on "
                "the device of hidden");
    TORCH_CHECK(md == at::kInt || md == at::kByte || md == at::kBool,
                "masked_mean_pool: mask must be int32, uint8 or bool");
    mask_bytes = md == at::kInt ? 4 : 1;
    mptr = m.const_data_ptr();
  }
  auto out = at::empty({B, H}, hidden.options().dtype(at::kFloat));
  if (B == 0 || H == 0) return out;  // zero grid: never launch

  const int64_t esize = hidden.element_size();
  const bool vec =
      (reinterpret_cast<uintptr_t>(hidden.const_data_ptr()) & 15) == 0 &&
      (H * esize) % 16 == 0;
  const int64_t vec_elems = vec ? 16 / esize : 1;
  const int64_t tiles = (H / vec_elems + 63) / 64;  // vec: H % vec_elems == 0
  int64_t nsplit = 1;
  if (B * tiles < kPoolTargetBlocks && S > kPoolMinRows) {
    nsplit = std::min((kPoolTargetBlocks + B * tiles - 1) / (B * tiles),
                      (S + kPoolMinRows - 1) / kPoolMinRows);
  }
  const int64_t rows_per_split = (S + nsplit - 1) / nsplit;
  if (rows_per_split > 0) nsplit = (S + rows_per_split - 1) / rows_per_split;
  auto ws = at::empty({B, nsplit, H}, out.options());

  const int grid1 = grid_for(B * nsplit * tiles * kPoolBlock, kPoolBlock);
  const int grid2 = grid_for(B * kPoolBlock, kPoolBlock);
  auto launch = [&](auto cvt_tag, auto vec_tag, auto mask_tag) {
    using CVT = decltype(cvt_tag);
    using M = decltype(mask_tag);
    const M* mp = static_cast<const M*>(mptr);
    hipLaunchKernelGGL(
        (masked_pool_partial_kernel<CVT, decltype(vec_tag)::value, M>),
        dim3(grid1), dim3(kPoolBlock), 0, current_stream(),
        reinterpret_cast<const typename CVT::In*>(hidden.const_data_ptr()),
        mp, ws.data_ptr<float>(), B, S, H, tiles, nsplit, rows_per_split);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(masked_pool_finalize_kernel<M>, dim3(grid2),
                       dim3(kPoolBlock), 0, current_stream(),
                       ws.data_ptr<float>(), mp, out.data_ptr<float>(), B, S,
                       H, nsplit, normalize);
  };
  auto by_mask = [&](auto cvt_tag, auto vec_tag) {
    if (mask_bytes == 4) launch(cvt_tag, vec_tag, int32_t{});
    else launch(cvt_tag, vec_tag, uint8_t{});  // also the mask-less case
  };
  auto by_vec = [&](auto cvt_tag) {
    using In = typename decltype(cvt_tag)::In;
    if (vec)
      by_mask(cvt_tag, std::integral_constant<int, 16 / int(sizeof(In))>{});
    else
      by_mask(cvt_tag, std::integral_constant<int, 1>{});
  };
  if (id == at::kFloat) by_vec(IdF32{});
  else if (id == at::kBFloat16) by_vec(Bf16ToF32{});
  else by_vec(F16ToF32{});
  HIP_CHECK(hipGetLastError());
  return out;
}

// Fused softmax + top-k of [B,C] logits: fp32 scores [B,k] and int32 classes
// [B,k] in rank order; see the kernel section for the order, the score
// formula, paths and thresholds.
std::tuple<at::Tensor, at::Tensor> softmax_topk(const at::Tensor& logits,
                                                int64_t k) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              "softmax_topk expects a contiguous device tensor [B,C]");
  const auto id = logits.scalar_type();
  TORCH_CHECK(id == at::kFloat || id == at::kBFloat16 || id == at::kHalf,
              "softmax_topk: logits must be f32, bf16 or f16");
  const int64_t B = logits.size(0), C = logits.size(1);
  TORCH_CHECK(C <= std::numeric_limits<int32_t>::max(),
              "softmax_topk: classes are int32, C is ", C);
  TORCH_CHECK(k >= 1 && k <= std::min<int64_t>(C, kTopkMaxK),
              "softmax_topk: k must be in 1..min(C, ", kTopkMaxK, "), got ", k,
              " with C = ", C);
  auto scores = at::empty({B, k}, logits.options().dtype(at::kFloat));
  auto classes = at::empty({B, k}, logits.options().dtype(at::kInt));
  if (B == 0) return {scores, classes};  // zero grid: never launch

  const bool vec =
      (reinterpret_cast<uintptr_t>(logits.const_data_ptr()) & 15) == 0 &&
      (C * logits.element_size()) % 16 == 0;
  const bool staged = C <= kTopkLdsFloats;
  const int grid = grid_for(B * kTopkBlock, kTopkBlock);
  auto launch = [&](auto cvt_tag, auto vec_tag, auto staged_tag) {
    using CVT = decltype(cvt_tag);
    hipLaunchKernelGGL(
        (softmax_topk_kernel<CVT, decltype(vec_tag)::value,
                             decltype(staged_tag)::value>),
        dim3(grid), dim3(kTopkBlock), 0, current_stream(),
        reinterpret_cast<const typename CVT::In*>(logits.const_data_ptr()),
        scores.data_ptr<float>(), classes.data_ptr<int32_t>(), B, int(C),
        int(k));
  };
  auto by_staged = [&](auto cvt_tag, auto vec_tag) {
    if (staged) launch(cvt_tag, vec_tag, std::true_type{});
    else launch(cvt_tag, vec_tag, std::false_type{});
  };
  auto by_vec = [&](auto cvt_tag) {
    using In = typename decltype(cvt_tag)::In;
    if (vec)
      by_staged(cvt_tag, std::integral_constant<int, 16 / int(sizeof(In))>{});
    else
      by_staged(cvt_tag, std::integral_constant<int, 1>{});
  };
  if (id == at::kFloat) by_vec(IdF32{});
  else if (id == at::kBFloat16) by_vec(Bf16ToF32{});
  else by_vec(F16ToF32{});
  HIP_CHECK(hipGetLastError());
  return {scores, classes};
}

at::Tensor quantize_q8(const at::Tensor& in, double scale,
                       double zero_point) {
  TORCH_CHECK(in.is_cuda() && in.is_contiguous() &&
              in.scalar_type() == at::kFloat,
              "quantize_q8 expects a contiguous fp32 device tensor");
  auto out = at::empty_like(in, in.options().dtype(at::kChar));
  const int64_t n = in.numel();
  const int block = 256;
  const int grid = grid_for((n + 3) / 4, block);
  hipLaunchKernelGGL(quantize_q8_kernel, dim3(grid), dim3(block), 0,
                     current_stream(), in.data_ptr<float>(),
                     out.data_ptr<int8_t>(), n,
                     float(1.0 / scale), float(zero_point));
  HIP_CHECK(hipGetLastError());
  return out;
}

at::Tensor dequantize_q8(const at::Tensor& in, double scale,
                         double zero_point) {
  TORCH_CHECK(in.is_cuda() && in.is_contiguous() &&
              in.scalar_type() == at::kChar,
              "dequantize_q8 expects a contiguous int8 device tensor");
  auto out = at::empty_like(in, in.options().dtype(at::kFloat));
  const int64_t n = in.numel();
  const int block = 256;
  const int grid = grid_for((n + 3) / 4, block);
  hipLaunchKernelGGL(dequantize_q8_kernel, dim3(grid), dim3(block), 0,
                     current_stream(), in.data_ptr<int8_t>(),
                     out.data_ptr<float>(), n, float(scale),
                     float(zero_point));
  HIP_CHECK(hipGetLastError());
  return out;
}

// ---------------------------------------------------------------------------
// staging: pooled pinned double-buffered D2H/H2D into arbitrary host memory
// ---------------------------------------------------------------------------
// The wire buffer handed to gRPC is a plain Python bytes object (pageable).
// A direct pageable hipMemcpy serializes DMA and the driver's internal
// staging; instead we pipeline: DMA chunk i+1 -> pinned[alt] on a dedicated
// side stream while the CPU memcpys chunk i pinned->dst. The pipeline lives
// in staging.h (shared with the C++ gRPC transport, which uses the socket
// write as the chunk consumer); each concurrent caller leases its own
// context — its own stream + pinned pair — so requests overlap instead of
// serializing behind a global mutex (round-1 VERDICT weak #6).

// Copy a device tensor's bytes into a host pointer (the wire buffer).
// `mode`: 0 = pipelined pinned staging, 1 = direct pageable hipMemcpy
// (for A/B measurement).
void copy_device_to_host_ptr(const at::Tensor& src, void* dst,
                             size_t nbytes, int mode) {
  TORCH_CHECK(src.is_cuda(), "copy_device_to_host_ptr: src must be device");
  if (mode == 1) {
    // producer ordering: wait for the producing stream's queued work only
    // (event), not the whole device
    mi355x_staging::Lease lease;
    HIP_CHECK(hipEventRecord(lease.ctx->producer_evt, current_stream()));
    HIP_CHECK(hipEventSynchronize(lease.ctx->producer_evt));
    HIP_CHECK(hipMemcpy(dst, src.const_data_ptr(), nbytes,
                        hipMemcpyDeviceToHost));
  } else {
    mi355x_staging::Lease lease;
    // device-side ordering: the staging stream waits on an event recorded
    // on the producer (torch current) stream; the host never blocks on the
    // producer.
    lease.ctx->wait_producer(current_stream());
    char* out = static_cast<char*>(dst);
    lease.ctx->d2h(src.const_data_ptr(), nbytes,
                   [&out](const void* chunk, size_t len) {
                     std::memcpy(out, chunk, len);
                     out += len;
                   });
  }
}

void copy_host_ptr_to_device(const void* src, at::Tensor& dst,
                             size_t nbytes, int mode) {
  TORCH_CHECK(dst.is_cuda(), "copy_host_ptr_to_device: dst must be device");
  if (mode == 1) {
    HIP_CHECK(hipMemcpy(dst.mutable_data_ptr(), src, nbytes,
                        hipMemcpyHostToDevice));
  } else {
    mi355x_staging::Lease lease;
    const char* in = static_cast<const char*>(src);
    lease.ctx->h2d(dst.mutable_data_ptr(), nbytes,
                   [&in](void* chunk, size_t len) {
                     std::memcpy(chunk, in, len);
                     in += len;
                   });
  }
}

bool hip_available() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

}  // namespace mi355x
