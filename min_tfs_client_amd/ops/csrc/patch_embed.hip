// CDNA4 (gfx950) fused ViT patch embedding: raw uint8 NHWC pixels in, token
// matrix out, one launch, matrix cores.
//
//   images uint8 [N,H,W,3]      wk bf16 [D,Kp]     bias fp32 [D]
//   pos fp32 [T,D] or null      cls fp32 [D] or null
//   out[n, t0+tok, d] = cvt( sum_k u8(n,tok,k) * wk[d,k] + bias[d] + pos )
//   out[n, 0, d]      = cvt( cls[d] + pos[0,d] )          (cls given: t0 = 1)
//
// This is a GEMM, C[M,D] = A[M,K] * B[K,D] with M = N*Hp*Wp tokens. The
// per-channel normalization is folded into wk and bias on the host, so A is
// the raw pixel: every integer 0..255 is exact in bf16 and A carries no
// rounding. K runs in (py, px, c) order, so one patch row of the K axis is
// 3*P contiguous bytes of the NHWC image and no im2col buffer exists.
//
// Work split. 256 threads = 4 waves in a 2x2 arrangement; a wave owns
// TM x TN accumulator blocks of v_mfma_f32_16x16x32_bf16 (16x16 outputs,
// 32 K values, fp32 accumulate), so a workgroup owns a BM x BN = 32*TM x
// 32*TN tile. Workgroups are numbered with the D tiles fastest: the
// workgroups that share an A tile run close together, the weights (1.2 MB
// for ViT-B) stay in every L2. M tiles are cut from the flat token index, so
// a tile spans image boundaries; the (n, hp, wp) of each tile row is worked
// out once per workgroup and kept in LDS (pixel offset, token, image).
//
// Two tiles:
//   kPeLargeM x kPeLargeN = 128 x 128  (TM = TN = 4, 64 accumulator VGPRs)
//   kPeSmallM x kPeSmallN =  32 x  32  (TM = TN = 1)
// Rule: the large tile is used iff it yields at least kPeLargeMinTiles = 256
// workgroups (one per CU of an MI355X), i.e. ceil(M/128) * ceil(D/128) >=
// 256; otherwise the small one. One 224x224 image into ViT-B is 196 x 768
// outputs: 12 large tiles for 256 CUs, but 168 small ones. Measured on an
// MI355X (ViT-B/16, bf16 out): 8 images (78 large tiles) 19 us small against
// 39 us large; 32 images (294 large tiles) 67 us small against 49 us large.
//
// K loop, kPeBK = 64 bytes of K per step (two MFMA slabs):
//  * A: each thread loads its share of the BM x 64 byte tile from global
//    memory into registers one step ahead, then stores it to one of two LDS
//    buffers AS BYTES (a quarter of the LDS traffic of staged bf16). Loads
//    are 16 bytes wide for P = 16 and 32 (a patch row is 48 / 96 bytes and
//    16-byte aligned); P = 14 rows are 42 bytes and only 2-byte aligned, so
//    they are filled with 2-byte loads. Every byte of the tile is written on
//    every step: rows past M and K positions past K = 3*P*P (the tail up to
//    Kp, and the rest of the last step) are zeros, never stale LDS, because
//    garbage widened to bf16 may be Inf/NaN and Inf * 0 is NaN.
//    The row stride is kPeLdsStride = 80 = 16 * 5 bytes: a fragment read is
//    8 bytes per lane (row = lane % 16, K offset = 8 * (lane / 16)), and
//    with an odd number of 16-byte slots per row the 16 rows of a half-wave
//    fall into 16 different slots of the 64 banks: conflict-free.
//    The 8 bytes are widened in registers: v_cvt_f32_ubyte, then the high
//    halves of two floats are packed into one bf16 pair (exact: 8 bits).
//  * B: direct global -> register loads, no LDS. A lane's fragment is the 8
//    K-contiguous bf16 of row d = lane % 16 at K offset 8 * (lane / 16): one
//    16-byte load that is already in MFMA layout. B is reused by only the
//    two wave rows of a workgroup and is L2/L1 resident, so an LDS tile would
//    buy a 2x cut of L1 traffic for a second staged operand, more barriers
//    and a padded layout; it is not worth it here. The next step's fragments
//    are loaded while the current ones feed the MFMAs.
//  * one barrier per step (double-buffered A).
//
// Epilogue from the accumulator registers in fp32: (acc + bias[d]) + pos,
// unfused, then one round-to-nearest-even conversion. A lane holds rows
// 4 * (lane / 16) + 0..3 of column lane % 16 of each 16x16 block. The class
// token rows are written by the workgroups whose tile holds an image's first
// token, for their own BN columns: still one launch, every output element is
// written by exactly one lane, no atomics, no split K: bit-identical reruns.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace mi355x {
namespace {

constexpr int kPeThreads = 256;
constexpr int kPeBK = 64;
constexpr int kPeLdsStride = 80;
constexpr int kPeLargeM = 128, kPeLargeN = 128;
constexpr int kPeSmallM = 32, kPeSmallN = 32;
constexpr int64_t kPeLargeMinTiles = 256;

typedef __bf16 pe_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pe_f32x4 __attribute__((ext_vector_type(4)));

struct PatchEmbedParams {
  const uint8_t* img;
  const uint16_t* wk;
  const float* bias;
  const float* pos;   // may be null
  const float* cls;   // may be null
  void* out;
  int M;              // N * Hp * Wp
  int H, W, Wp, HW;   // HW = Hp * Wp
  int D, K, Kp, T, t0;
  int tiles_n;
};

struct PeOutF32 {
  using T = float;
  static __device__ __forceinline__ float cvt(float v) { return v; }
};
struct PeOutBf16 {
  using T = uint16_t;
  static __device__ __forceinline__ uint16_t cvt(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u)          // NaN: quiet, keep sign
      return uint16_t((u >> 16) | 0x0040u);
    return uint16_t((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  }
};
struct PeOutF16 {
  using T = uint16_t;
  static __device__ __forceinline__ uint16_t cvt(float f) {
    __half_raw r(__float2half(f));                // round to nearest even
    return r.x;
  }
};

// two bytes -> one register holding two bf16 (low half: the lower address)
__device__ __forceinline__ uint32_t pe_widen2(uint32_t lo, uint32_t hi) {
  return (__float_as_uint(float(lo)) >> 16) |
         (__float_as_uint(float(hi)) & 0xffff0000u);
}

__device__ __forceinline__ pe_bf16x8 pe_widen8(uint2 v) {
  union { uint32_t w[4]; pe_bf16x8 f; } u;
  u.w[0] = pe_widen2(v.x & 0xffu, (v.x >> 8) & 0xffu);
  u.w[1] = pe_widen2((v.x >> 16) & 0xffu, v.x >> 24);
  u.w[2] = pe_widen2(v.y & 0xffu, (v.y >> 8) & 0xffu);
  u.w[3] = pe_widen2((v.y >> 16) & 0xffu, v.y >> 24);
  return u.f;
}

template <int P, int TM, int TN, typename OUT>
__global__ void __launch_bounds__(kPeThreads)
u8_patch_embed_kernel(const PatchEmbedParams p) {
  constexpr int BM = 32 * TM, BN = 32 * TN;
  constexpr int VEC = (P % 16 == 0) ? 16 : 2;      // bytes per A load
  constexpr int ROWB = 3 * P;                      // bytes of one patch row
  constexpr int UPR = kPeBK / VEC;                 // load units per tile row
  constexpr int UNITS = BM * UPR;
  constexpr int UPT = (UNITS + kPeThreads - 1) / kPeThreads;
  using AVec = std::conditional_t<VEC == 16, uint4, uint16_t>;
  using OutT = typename OUT::T;

  __shared__ __attribute__((aligned(16))) uint8_t a_lds[2][BM * kPeLdsStride];
  __shared__ int64_t row_pix[BM];   // byte offset of the patch's first pixel
  __shared__ int row_tok[BM];       // token index inside the image, -1: past M
  __shared__ int row_img[BM];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 15, lgrp = lane >> 4;
  const int tile_n = int(blockIdx.x % uint32_t(p.tiles_n));
  const int m0 = int(blockIdx.x / uint32_t(p.tiles_n)) * BM;
  const int d0 = tile_n * BN;

  if (tid < BM) {
    const int m = m0 + tid;
    int tok = -1, n = 0;
    int64_t pix = 0;
    if (m < p.M) {
      n = m / p.HW;
      tok = m - n * p.HW;
      const int hp = tok / p.Wp, wp = tok - hp * p.Wp;
      pix = ((int64_t(n) * p.H + int64_t(hp) * P) * p.W + int64_t(wp) * P) * 3;
    }
    row_pix[tid] = pix;
    row_tok[tid] = tok;
    row_img[tid] = n;
  }
  __syncthreads();

  AVec a_reg[UPT];
  auto load_a = [&](int k0) {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + i * kPeThreads;
      AVec v{};
      if (UNITS % kPeThreads == 0 || u < UNITS) {
        const int r = u / UPR, k = k0 + (u % UPR) * VEC;
        // K and ROWB are multiples of VEC: a unit is inside one patch row
        // and either wholly below K or wholly padding
        if (row_tok[r] >= 0 && k < p.K) {
          const int py = k / ROWB;
          const int64_t off =
              row_pix[r] + int64_t(py) * p.W * 3 + (k - py * ROWB);
          v = *reinterpret_cast<const AVec*>(p.img + off);
        }
      }
      a_reg[i] = v;
    }
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + i * kPeThreads;
      if (UNITS % kPeThreads == 0 || u < UNITS)
        *reinterpret_cast<AVec*>(
            &a_lds[buf][(u / UPR) * kPeLdsStride + (u % UPR) * VEC]) =
            a_reg[i];
    }
  };

  // B rows of this lane; a block past D reads row D-1 and is never stored
  const uint16_t* b_row[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    int d = d0 + (wn * TN + tn) * 16 + lrow;
    d = d < p.D ? d : p.D - 1;
    b_row[tn] = p.wk + int64_t(d) * p.Kp + lgrp * 8;
  }
  uint4 b_next[2][TN], b_cur[2][TN];
  auto load_b = [&](int k0) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int k = k0 + ks * 32;
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
        b_next[ks][tn] = k < p.Kp
            ? *reinterpret_cast<const uint4*>(b_row[tn] + k)
            : uint4{0u, 0u, 0u, 0u};
    }
  };

  pe_f32x4 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = pe_f32x4{0.f, 0.f, 0.f, 0.f};

  const int steps = (p.Kp + kPeBK - 1) / kPeBK;
  load_a(0);
  load_b(0);
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    store_a(buf);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) b_cur[ks][tn] = b_next[ks][tn];
    // one barrier per step: buffer buf was last read two steps ago, and
    // every thread has passed the barrier of the step in between
    __syncthreads();
    if (s + 1 < steps) {
      load_a((s + 1) * kPeBK);
      load_b((s + 1) * kPeBK);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      pe_bf16x8 a[TM];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const int r = (wm * TM + tm) * 16 + lrow;
        a[tm] = pe_widen8(*reinterpret_cast<const uint2*>(
            &a_lds[buf][r * kPeLdsStride + ks * 32 + lgrp * 8]));
      }
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        union { uint4 u; pe_bf16x8 f; } b;
        b.u = b_cur[ks][tn];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[tm], b.f, acc[tm][tn], 0, 0, 0);
      }
    }
  }

  OutT* out = reinterpret_cast<OutT*>(p.out);
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int d = d0 + (wn * TN + tn) * 16 + lrow;
    if (d >= p.D) continue;
    const float bias = p.bias[d];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = (wm * TM + tm) * 16 + lgrp * 4 + i;
        const int tok = row_tok[r];
        if (tok < 0) continue;
        const int t = p.t0 + tok;
        float v = acc[tm][tn][i] + bias;
        if (p.pos) v = v + p.pos[int64_t(t) * p.D + d];
        out[(int64_t(row_img[r]) * p.T + t) * p.D + d] = OUT::cvt(v);
      }
    }
  }

  if (p.cls) {
    const int d_end = d0 + BN < p.D ? d0 + BN : p.D;
    for (int r = wave; r < BM; r += kPeThreads / 64) {
      if (row_tok[r] != 0) continue;               // an image's first token
      OutT* dst = out + int64_t(row_img[r]) * p.T * p.D;
      for (int d = d0 + lane; d < d_end; d += 64) {
        float v = p.cls[d];
        if (p.pos) v = v + p.pos[d];
        dst[d] = OUT::cvt(v);
      }
    }
  }
}

template <int P, int TM, int TN, typename OUT>
void launch_patch_embed(const PatchEmbedParams& p, int64_t tiles,
                        hipStream_t stream) {
  hipLaunchKernelGGL((u8_patch_embed_kernel<P, TM, TN, OUT>),
                     dim3(uint32_t(tiles)), dim3(kPeThreads), 0, stream, p);
}

template <int P, int TM, int TN>
void launch_patch_embed_out(at::ScalarType out_dtype,
                            const PatchEmbedParams& p, int64_t tiles,
                            hipStream_t stream) {
  if (out_dtype == at::kFloat)
    launch_patch_embed<P, TM, TN, PeOutF32>(p, tiles, stream);
  else if (out_dtype == at::kBFloat16)
    launch_patch_embed<P, TM, TN, PeOutBf16>(p, tiles, stream);
  else
    launch_patch_embed<P, TM, TN, PeOutF16>(p, tiles, stream);
}

template <int P>
void launch_patch_embed_tile(bool large, at::ScalarType out_dtype,
                             const PatchEmbedParams& p, int64_t tiles,
                             hipStream_t stream) {
  if (large)
    launch_patch_embed_out<P, kPeLargeM / 32, kPeLargeN / 32>(
        out_dtype, p, tiles, stream);
  else
    launch_patch_embed_out<P, kPeSmallM / 32, kPeSmallN / 32>(
        out_dtype, p, tiles, stream);
}

}  // namespace

// Fused ViT patch embedding, see the header of this file. ``tile``: 0 picks
// by the rule there, 1 forces the small tile, 2 the large one (tests reach
// both at small shapes). Arguments the kernel cannot serve are ValueError.
at::Tensor u8_patch_embed(const at::Tensor& images, const at::Tensor& wk,
                          const at::Tensor& bias, int64_t patch,
                          const c10::optional<at::Tensor>& pos,
                          const c10::optional<at::Tensor>& cls,
                          at::ScalarType out_dtype, int64_t tile) {
  const char* who = "u8_patch_embed";
  TORCH_CHECK_VALUE(images.is_cuda() && images.dim() == 4 &&
                    images.is_contiguous() &&
                    images.scalar_type() == at::kByte && images.size(3) == 3,
                    who, " expects a contiguous uint8 device tensor [N,H,W,3]");
  TORCH_CHECK_VALUE(patch == 14 || patch == 16 || patch == 32, who,
                    ": patch must be 14, 16 or 32, got ", patch);
  TORCH_CHECK_VALUE(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
                    out_dtype == at::kHalf,
                    who, ": out_dtype must be f32, bf16 or f16");
  TORCH_CHECK_VALUE(tile >= 0 && tile <= 2, who, ": tile must be 0, 1 or 2");
  const int64_t N = images.size(0), H = images.size(1), W = images.size(2);
  TORCH_CHECK_VALUE(H >= patch && W >= patch && H % patch == 0 &&
                    W % patch == 0, who, ": H and W must be positive "
                    "multiples of patch ", patch, ", got ", H, "x", W);
  const int64_t Hp = H / patch, Wp = W / patch, HW = Hp * Wp, M = N * HW;
  const int64_t K = 3 * patch * patch, Kp = (K + 31) / 32 * 32;
  auto on_device = [&](const at::Tensor& t) {
    return t.is_cuda() && t.get_device() == images.get_device() &&
           t.is_contiguous();
  };
  TORCH_CHECK_VALUE(on_device(wk) && wk.scalar_type() == at::kBFloat16 &&
                    wk.dim() == 2 && wk.size(1) == Kp && wk.size(0) >= 16 &&
                    wk.size(0) % 16 == 0, who, ": wk must be contiguous "
                    "bf16 [D,", Kp, "] with D a multiple of 16");
  const int64_t D = wk.size(0);
  TORCH_CHECK_VALUE(on_device(bias) && bias.scalar_type() == at::kFloat &&
                    bias.dim() == 1 && bias.size(0) == D, who,
                    ": bias must be contiguous fp32 [", D, "]");
  const int64_t t0 = cls.has_value() ? 1 : 0, T = HW + t0;
  if (pos.has_value())
    TORCH_CHECK_VALUE(on_device(*pos) && pos->scalar_type() == at::kFloat &&
                      pos->dim() == 2 && pos->size(0) == T &&
                      pos->size(1) == D, who,
                      ": pos must be contiguous fp32 [", T, ",", D, "]");
  if (cls.has_value())
    TORCH_CHECK_VALUE(on_device(*cls) && cls->scalar_type() == at::kFloat &&
                      cls->dim() == 1 && cls->size(0) == D, who,
                      ": cls must be contiguous fp32 [", D, "]");
  TORCH_CHECK_VALUE(M <= std::numeric_limits<int32_t>::max() - kPeLargeM &&
                    D <= (1 << 20) && H <= (1 << 20) && W <= (1 << 20), who,
                    ": too many tokens or too large a side");
  // 16-byte loads of pixels (P = 16, 32) and of weight fragments
  TORCH_CHECK_VALUE(
      reinterpret_cast<uintptr_t>(images.const_data_ptr()) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(wk.const_data_ptr()) % 16 == 0, who,
      ": images and wk must be 16-byte aligned");

  auto out = at::empty({N, T, D}, images.options().dtype(out_dtype));
  if (N == 0) return out;                 // zero grid: never launch

  auto tiles_of = [&](int64_t bm, int64_t bn) {
    return ((M + bm - 1) / bm) * ((D + bn - 1) / bn);
  };
  const bool large = tile == 2 ||
      (tile == 0 && tiles_of(kPeLargeM, kPeLargeN) >= kPeLargeMinTiles);
  const int64_t bn = large ? kPeLargeN : kPeSmallN;
  const int64_t tiles = large ? tiles_of(kPeLargeM, kPeLargeN)
                              : tiles_of(kPeSmallM, kPeSmallN);
  TORCH_CHECK_VALUE(tiles <= std::numeric_limits<int32_t>::max(), who,
                    ": too many tiles");

  PatchEmbedParams p;
  p.img = static_cast<const uint8_t*>(images.const_data_ptr());
  p.wk = static_cast<const uint16_t*>(wk.const_data_ptr());
  p.bias = static_cast<const float*>(bias.const_data_ptr());
  p.pos = pos.has_value()
      ? static_cast<const float*>(pos->const_data_ptr()) : nullptr;
  p.cls = cls.has_value()
      ? static_cast<const float*>(cls->const_data_ptr()) : nullptr;
  p.out = out.mutable_data_ptr();
  p.M = int(M);
  p.H = int(H); p.W = int(W); p.Wp = int(Wp); p.HW = int(HW);
  p.D = int(D); p.K = int(K); p.Kp = int(Kp); p.T = int(T); p.t0 = int(t0);
  p.tiles_n = int((D + bn - 1) / bn);

  hipStream_t stream = at::hip::getCurrentHIPStream().stream();
  if (patch == 14)
    launch_patch_embed_tile<14>(large, out_dtype, p, tiles, stream);
  else if (patch == 16)
    launch_patch_embed_tile<16>(large, out_dtype, p, tiles, stream);
  else
    launch_patch_embed_tile<32>(large, out_dtype, p, tiles, stream);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(err) + " at u8_patch_embed");
  return out;
}

}  // namespace mi355x
