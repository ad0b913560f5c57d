// CDNA4 (gfx950) fused ViT patch embedding: raw uint8 NHWC pixels, or YUV
// 4:2:0 frames (NV12 / I420), in, token matrix out, one launch, matrix cores.
//
//   images uint8 [N,H,W,3]      wk bf16 [D,Kp]     bias fp32 [D]
//   (or frames uint8 [N,H*3/2,W], converted to those pixels on the way in)
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
// One kernel body, patch_embed_kernel, and three A loaders (a template
// parameter: PeRgbLoader, PeYuvLoader, PeResizeLoader: images of any size,
// resized and cropped on the way in, see the end of this header; its large
// tile is 64 x 128). The loader owns the A side of a K
// step: how many bytes of K a step is (BK), the LDS row stride (STRIDE), the
// per-row offsets, the global -> register prefetch and the register -> LDS
// store. The MFMA loop, the B fragments, the epilogue and the class-token
// rows are written once, so an output element accumulates the same 32-wide K
// slabs in the same ascending order into one accumulator whatever the loader:
// tile shape and bytes of K per barrier do not enter that order.
//
// K loop of the RGB loader, BK = 64 bytes of K per step (two MFMA slabs):
//  * A: each thread loads its share of the BM x 64 byte tile from global
//    memory into registers one step ahead, then stores it to one of two LDS
//    buffers AS BYTES (a quarter of the LDS traffic of staged bf16). Loads
//    are 16 bytes wide for P = 16 and 32 (a patch row is 48 / 96 bytes and
//    16-byte aligned); P = 14 rows are 42 bytes and only 2-byte aligned, so
//    they are filled with 2-byte loads. Every byte of the tile is written on
//    every step: rows past M and K positions past K = 3*P*P (the tail up to
//    Kp, and the rest of the last step) are zeros, never stale LDS, because
//    garbage widened to bf16 may be Inf/NaN and Inf * 0 is NaN.
//    The row stride is STRIDE = 80 = 16 * 5 bytes: a fragment read is
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
//
// YUV 4:2:0 loader (P = 16 and 32; a 42-byte P = 14 row fits neither the K
// step nor the loads). Frames are laid out as in the YUV section of
// pack_kernels.hip and converted with its int32 arithmetic (yuv420_convert.h:
// Yuv420Coef, clamp-first yuv_clamp8). The converted pixel is a uint8 value,
// so A stays exact in bf16, wk is the RGB path's tensor (K keeps its
// (py, px, c) order) and the result is bit-identical to the RGB kernel on the
// converted frames, which never exist in memory.
//  * BK = 96 bytes of K per step (three MFMA slabs) = 32 pixels per tile row,
//    the luma rows that share one chroma row: P = 16: patch rows 2s and 2s+1
//    with chroma row s of the patch, K = 768 in 8 steps; P = 32: patch row s
//    with chroma row s >> 1, K = 3072 in 32 steps. Kp = K: no K tail.
//  * The 32 * BM pixels of a step are 256 work units, one per thread:
//      BM = 128, P = 16: 8 pixels x 2 luma rows. Loads 2 x 8 B luma and 8 B
//                        of NV12 pairs / 2 x 4 B of I420; stores 2 x 24 B.
//      BM = 128, P = 32: 16 pixels x 1 row. Loads 16 B luma and 16 B NV12 /
//                        2 x 8 B I420; stores 48 B.
//      BM = 32:          4 pixels x 1 row (all 256 threads convert, chroma is
//                        read twice for P = 16). Loads 4 B luma and 4 B NV12
//                        / 2 x 2 B I420; stores 12 B.
//    A unit is loaded into registers one step ahead, like the RGB loader's,
//    converted at store time and written to the LDS tile as RGB bytes at its
//    K offset; the tile stays bytes, widened at the fragment read. H and W
//    are multiples of 16 and the tensor is 16-byte aligned, so every luma and
//    chroma offset of a unit is a multiple of its load width in both layouts
//    (frame: 384 | H*W*3/2; chroma planes: 64 | H*W/4; rows: 8 | W/2), and a
//    unit lies inside its patch, so no byte outside the tensor is read. Rows
//    past M load nothing and store zeros on every step (the conversion of
//    zeros is not zero). Frame bases are int64.
//  * STRIDE = 112 = 16 * 7 bytes: seven slots, odd, so the fragment reads are
//    conflict-free by the argument above. Stores, by bank arithmetic (64
//    banks, a pass is 64 / 32 / 16 lanes of 4 / 8 / 16 B), not counters:
//    the 8-byte stores of the 128-row P = 16 tile are conflict-free (units
//    of a row sit 24 B apart: words 0,1 and 2,3 of the row's 16-byte slots);
//    the 16-byte stores of the 128-row P = 32 tile and the 4-byte stores of
//    the 32-row tiles are two-way. That is 3 extra store passes per thread
//    and step, next to 3 * TM fragment reads and 3 * TM * TN MFMAs.
//  * LDS: 2 x 128 x 112 B + tables = 31 KB (large), 7.8 KB (small). gfx950
//    resource use (hipcc, ROCm 7.2): large tile 162-168 VGPRs + 64 AGPRs,
//    small tile 50-52 + 4, no scratch; occupancy 2 / 8 waves per SIMD, as
//    the RGB instantiations (130-136 + 64, 44 + 4).
//  * Tiles, the tile rule and the workgroup order are the RGB path's. The
//    measured crossover is the same (MI355X, ViT-B/16, NV12, bf16 out: 8
//    images 20 us small against 41 us large; 32 images 65 us small against
//    49 us large), and the fused op takes 0.93-1.10 of the RGB kernel's time
//    on converted frames (profiles/README.md).
//
// Resampling loader (PeResizeLoader, P = 16 and 32): images of any size,
// [N,Hin,Win,3]; the K values of a token are the pixels of its patch in the
// crop window of the bilinearly resized image, which never exists in memory.
// A resized pixel is the fp32 blend v of the resize ingest (resize_tap.h and
// the unfused t, b, v chain of pack_kernels.hip), not a bf16 number, so A is
// two bf16 pieces, hi = bf16_rne(v) and lo = bf16_rne(v - hi) (v - hi is
// exact, |v - (hi + lo)| <= 2^-16 |v|), and the loop issues the hi MFMA, then
// the lo MFMA of every 32-wide slab into the one accumulator (PIECES = 2;
// `frag` hands the loop a piece's fragment, the byte loaders widen there).
// At the identity size the weights are 0, lo is 0 and the result is the RGB
// kernel's, bit for bit.
//  * A step is 32 pixels = 96 K values = 3 slabs per tile row, as for YUV
//    (P = 16: patch rows 2s, 2s+1; P = 32: patch row s); K = Kp, no tail.
//    The 32 * BM pixels are 256 units, one per thread: 8 (BM = 64) or 4
//    (BM = 32) consecutive output columns of one output row. The tile rows'
//    table holds token, image, the image's byte offset (int64) and the
//    patch's first pixel in the resized image (row, column; top / left
//    added: the taps depend on that sum alone).
//  * Gathers are issued a step ahead, before the MFMAs, like the other
//    loaders' loads: y0, y1, wy once per unit, x0 per pixel, then ONE 8-byte
//    load per pixel and source row at the byte of pixel x0 (any alignment):
//    x1 is x0 or x0 + 1, so both taps are in its first 6 bytes. resize_tap
//    clamps every index into the image, and a load that would pass the end
//    of the tensor starts at its last 8 bytes instead and is shifted down
//    when it is used (a batch under 8 bytes is copied into 8), so no byte
//    outside `images` is read for any ratio. Source spans are NOT staged in
//    LDS: the gathers hit L1/L2, which the workgroups that share an A tile
//    (D tiles run fastest) keep warm. Rows past M gather nothing and blend
//    zero registers: +0 in both pieces.
//  * The blend, the split (v_cvt_pk_bf16_f32) and the stores happen at store
//    time. The fp32 chain is kept out of v_pk_*_f32 (pe_alone).
//  * LDS tile: bf16, 4 bytes per K value. A row is 96 hi (192 B), 96 lo
//    (192 B) and 16 B of padding: STRIDE = 400 B = 25 16-byte slots, odd. A
//    lane's fragment of a piece is one 16-byte read (row lane % 16, K offset
//    8 * (lane / 16)) already in MFMA layout; the 16 rows of a pass fall
//    into 16 different slots of the 64 banks (25 r mod 16 is a permutation):
//    conflict-free. Stores: 6 x 16 B per thread (BM = 64; a pass of 16 lanes
//    is 4 rows x 4 units at slots 25 r + 3 q + const: 13 of 16 slots,
//    two-way on three of them) or 6 x 8 B (BM = 32).
//  * LDS budget: a 128-row double-buffered tile would be 100 KB. The large
//    tile of this loader is kPeResizeLargeM x kPeLargeN = 64 x 128 (TM = 2,
//    TN = 4), double-buffered, one barrier per step: 2 x 64 x 400 B + tables
//    = 51.5 KB; the small tile 25.8 KB. The alternative, a single-buffered
//    128-row tile with two barriers per step, was not built or measured.
//  * gfx950 resource use (hipcc, ROCm 7.2): large tile 186 VGPRs + 32 AGPRs,
//    small tile 80 + 4, no scratch; occupancy 2 / 5 waves per SIMD.
//  * Measured on an MI355X (ViT-B/16, bf16 out, 480x640 -> 256 -> crop 224):
//    8 images (150 large tiles) 40 us small against 52 us large; 32 images
//    (588 large tiles) 130 us small against 112 us large (from 1080x1920:
//    136 against 142, inside the spread). The crossover sits where the other
//    loaders' does: kPeResizeLargeMinTiles = 256. One launch takes 0.20-0.81
//    of the time of image_u8_resize_to_float + VisionTransformer.embed; the
//    identity size costs 1.6-2.0 of the RGB kernel (the second MFMA piece,
//    the bf16 tile and the blend). profiles/README.md.
//
// Ragged batches into the resampling loader (PeGeomRagged, P = 16 and 32): N
// RGB images of N sizes, HWC, back to back in one flat buffer; the crop
// window Hc x Wc is shared, so M = N*Hp*Wp, the flat token index, the tiles,
// the tile rule and the workgroup order are the dense loader's. What the
// dense loader reads from the kernel arguments (Hin, Win, rh, rw, top, left,
// n * Hin * Win * 3) is per image here, in a device table of int32 [N,8] rows
// (PeRaggedEntry, the table of the ragged resize ingest in pack_kernels.hip).
// The loader body is one: its geometry is a policy (PeGeomDense /
// PeGeomRagged), and the dense instantiations compile to what they were
// (same registers, LDS and occupancy as above).
//  * Work split: the prologue thread of a tile row (tid < BM) works out the
//    row's image from the flat token index, as before, and reads that image's
//    32-byte entry once. Offset and crop origin go where the dense loader
//    keeps them (row_pix, row_aux); (Hin, Win, rh, rw) go to a 16-byte slot
//    of a fourth row table in LDS. Geometry is per ROW, not per tile: a tile
//    of one-patch images has a different image on every row. After the
//    barrier each thread, which owns one unit of one row for the whole K
//    loop, lifts its row's slot into four registers in init(); load() and
//    store() never touch the table again. Rows past M keep a 1 x 1 geometry,
//    gather nothing and blend zero registers, as in the dense loader.
//  * Cost (hipcc, ROCm 7.2): large tile 206 VGPRs + 32 AGPRs (dense 186 +
//    32: the four values, and address arithmetic that was scalar and is now
//    per lane), small tile 84 + 4 (dense 80 + 4), no scratch; occupancy 2 / 5
//    waves per SIMD, the dense instantiations' (238 of the 256 registers of
//    occupancy 2). LDS: 64 x 16 B more, 52.5 KB (large), 26.3 KB (small).
//  * Reads stay inside the buffer: src_last is the last 8 bytes of the WHOLE
//    packed buffer. resize_tap clamps y into [0, Hin_i) and x0 into
//    [0, Win_i), so a gather starts at a = off_i + (y * Win_i + x0) * 3 <=
//    off_i + Hin_i * Win_i * 3 - 3 <= bytes - 3; min(a, src_last) keeps the 8
//    bytes inside the buffer and store() shifts by a - src_last <= 5. The
//    first 3 bytes used are always pixel x0 of image i. The next 3 are pixel
//    x0 + 1 of the same row when x1 = x0 + 1. When x1 == x0 (the right edge)
//    they are the next row's, at an image's last pixel now the NEXT IMAGE's
//    first bytes, or zeros shifted in at the end of the buffer: finite in
//    every case, and the weight is replaced by 0, so the blend is p00, what
//    p00 + wx * (p00 - p00) gives. A batch under 8 bytes is copied into 8 on
//    the host. The host op validates every entry against the buffer size
//    (sum of H_i * W_i * 3 == bytes) before the launch; the kernel trusts
//    the table.
//  * Every image's tokens are those of the dense launch on that image alone,
//    bit for bit, at every tile: the taps depend on the image's own entry and
//    the position in its resized image alone, and the MFMA loop, the B
//    fragments and the epilogue are untouched, so an output element still
//    accumulates hi then lo of ascending 32-wide slabs into one accumulator.
//  * Measured on an MI355X (ViT-B/16, bf16 out, photos of mixed sizes,
//    256..512 x 341..683 -> shorter side 256 -> crop 224; the launch alone on
//    a device-resident table / the Python op with its host-built table): N =
//    1: 16.3 / 34 us against 18 us for one dense call; N = 8: 41 / 47 us
//    against 142 us for 8 dense launches + cat and 110-120 us for the ragged
//    fp32 resize + embed; N = 32: 99 / 105 us against 561 us and 147 us. So
//    the one launch wins from a few images on (3.0x and 5.3x against the
//    loop at 8 and 32, 1.4-2.5x against resize-then-embed) and loses at N = 1
//    to a single dense call, by the op's host-side table (about 18 us). On
//    uniform batches (N x 384x512) this launch takes 0.99-1.03 of the dense
//    resampling launch, inside the 4-8 % spread of the rounds; what remains
//    is the op's table, 6-18 us per call, which same-size requests save by
//    staying with the dense entry. profiles/README.md.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "resize_tap.h"
#include "yuv420_convert.h"

namespace mi355x {
namespace {

constexpr int kPeThreads = 256;
constexpr int kPeLargeM = 128, kPeLargeN = 128;
constexpr int kPeSmallM = 32, kPeSmallN = 32;
constexpr int64_t kPeLargeMinTiles = 256;
// the resampling loader's large tile, see the header
constexpr int kPeResizeLargeM = 64;
constexpr int64_t kPeResizeLargeMinTiles = 256;

typedef __bf16 pe_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pe_f32x4 __attribute__((ext_vector_type(4)));

// One image of a ragged batch: a row of the int32 [N,8] table that
// ops.image_u8_ragged_resize_to_float defines (U8RaggedEntry of
// pack_kernels.hip), built and checked on the host.
struct PeRaggedEntry {
  int64_t offset;    // first byte of the image in the packed buffer
  int Hin, Win, top, left;
  float rh, rw;
};
static_assert(sizeof(PeRaggedEntry) == 32, "table rows are int32 [8]");

struct PatchEmbedParams {
  const uint8_t* img;   // RGB pixels, or YUV 4:2:0 frames
  const uint16_t* wk;
  const float* bias;
  const float* pos;   // may be null
  const float* cls;   // may be null
  void* out;
  int M;              // N * Hp * Wp
  int H, W, Wp, HW;   // HW = Hp * Wp
  int D, K, Kp, T, t0;
  int tiles_n;
  // YUV loaders only
  int64_t frame;      // bytes of one frame, H*W*3/2
  int64_t vplane;     // I420: bytes from a U sample to its V, (H/2)*(W/2)
  Yuv420Coef k;
  // resampling loader only: H x W above is the crop window of the resized
  // image, img holds N source images of Hin x Win pixels
  int Hin, Win, top, left;
  float rh, rw;
  int64_t src_last;   // offset of the last 8 bytes of img
  // ragged resampling loader only: img is the packed buffer, and Hin, Win,
  // top, left, rh, rw above are unused: they are per image, in this table
  const PeRaggedEntry* table;
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

// one lane's A fragment of a byte tile: 8 bytes of row `row`, widened
template <int STRIDE>
__device__ __forceinline__ pe_bf16x8 pe_byte_frag(const uint8_t* buf, int row,
                                                  int ks, int lgrp) {
  return pe_widen8(*reinterpret_cast<const uint2*>(
      &buf[row * STRIDE + ks * 32 + lgrp * 8]));
}

// ---------------------------------------------------------------------------
// A loaders. A loader is one thread's share of the A side of the K loop: the
// geometry of a step (BK values of K, STRIDE bytes per LDS tile row, PIECES
// bf16 pieces whose sum is the operand), the offsets kept per tile row,
// `load(p, s)`: global memory -> registers for step s, `store(buf)`:
// registers -> the BM-row tile at `buf`, and `frag(buf, row, ks, lgrp,
// piece)`: a lane's 8 K values of slab ks of that tile, in MFMA layout.
// ---------------------------------------------------------------------------

// RGB: the K bytes of a step are contiguous pixels of one or two patch rows.
template <int P, int BM_>
struct PeRgbLoader {
  static constexpr int BM = BM_, BK = 64, STRIDE = 80, PIECES = 1;
  static constexpr bool kAux = false, kGeom = false;
  static constexpr int VEC = (P % 16 == 0) ? 16 : 2;   // bytes per A load
  static constexpr int ROWB = 3 * P;                   // bytes of a patch row
  static constexpr int UPR = BK / VEC;                 // load units per row
  static constexpr int UNITS = BM * UPR;
  static constexpr int UPT = (UNITS + kPeThreads - 1) / kPeThreads;
  using AVec = std::conditional_t<VEC == 16, uint4, uint16_t>;

  const int64_t* row_pix;
  const int* row_tok;
  int tid;
  AVec a_reg[UPT];

  // byte offset of the first pixel of patch (hp, wp) of image n
  static __device__ __forceinline__ void offsets(
      const PatchEmbedParams& p, int n, int hp, int wp, int64_t& pix,
      int64_t&, int4&) {
    pix = ((int64_t(n) * p.H + int64_t(hp) * P) * p.W + int64_t(wp) * P) * 3;
  }
  __device__ __forceinline__ void init(const PatchEmbedParams&, int tid_,
                                       const int64_t* pix, const int64_t*,
                                       const int4*, const int* tok) {
    row_pix = pix;
    row_tok = tok;
    tid = tid_;
  }
  __device__ __forceinline__ void load(const PatchEmbedParams& p, int s) {
    const int k0 = s * BK;
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
  }
  __device__ __forceinline__ void store(const PatchEmbedParams&,
                                        uint8_t* buf) const {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + i * kPeThreads;
      if (UNITS % kPeThreads == 0 || u < UNITS)
        *reinterpret_cast<AVec*>(&buf[(u / UPR) * STRIDE + (u % UPR) * VEC]) =
            a_reg[i];
    }
  }
  static __device__ __forceinline__ pe_bf16x8 frag(const uint8_t* buf, int row,
                                                  int ks, int lgrp, int) {
    return pe_byte_frag<STRIDE>(buf, row, ks, lgrp);
  }
};

// NB aligned bytes -> the low bytes of d[0..]
template <int NB>
__device__ __forceinline__ void pe_load_bytes(const uint8_t* a, uint32_t* d) {
  if constexpr (NB == 2) {
    d[0] = *reinterpret_cast<const uint16_t*>(a);
  } else if constexpr (NB == 4) {
    d[0] = *reinterpret_cast<const uint32_t*>(a);
  } else if constexpr (NB == 8) {
    const uint2 v = *reinterpret_cast<const uint2*>(a);
    d[0] = v.x; d[1] = v.y;
  } else {
    static_assert(NB == 16, "load width");
    const uint4 v = *reinterpret_cast<const uint4*>(a);
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
}

__device__ __forceinline__ int pe_byte(const uint32_t* w, int b) {
  return int((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
}

// YUV 4:2:0 (NV12 / I420): a step is 96 bytes of K = 32 pixels per tile row,
// the luma rows that share ONE chroma row: P = 16: patch rows 2s and 2s+1
// (chroma row s of the patch), P = 32: patch row s (chroma row s >> 1). The
// 32 * BM pixels of a step are cut into 256 units, one per thread, of NR luma
// rows x PX pixels with the chroma pairs below them:
//   BM = 128, P = 16: 2 x 8     BM = 128, P = 32: 1 x 16     BM = 32: 1 x 4
// A unit is loaded into registers one step ahead (luma: NR loads of PX bytes;
// chroma: PX bytes of NV12 pairs, or PX/2 bytes each of U and V), converted
// in int32 at store time and written as RGB bytes at its K offset.
template <int P, int BM_, bool I420>
struct PeYuvLoader {
  static_assert(P == 16 || P == 32, "a 42-byte patch row fits no unit");
  static constexpr int BM = BM_, BK = 96, STRIDE = 112, PIECES = 1;
  static constexpr bool kAux = true;       // the chroma offsets
  static constexpr bool kGeom = false;
  static constexpr int UPR = kPeThreads / BM;          // units per tile row
  static_assert(UPR == 2 || UPR == 8, "one unit per thread");
  static constexpr int NR = (P == 16 && UPR == 2) ? 2 : 1;
  static constexpr int PX = 32 / UPR / NR;             // 4, 8 or 16
  static constexpr int PXW = PX / 4;                   // words of PX bytes
  static constexpr int LROWS = (P == 16) ? 2 : 1;      // luma rows per step

  const uint8_t* ya;     // luma of the unit at step 0; null: row past M
  const uint8_t* ua;     // its first U sample (NV12: first (U,V) pair)
  int lds_off, W;
  uint32_t y[NR][PXW];
  uint32_t c[PXW];       // NV12: U,V interleaved; I420: PX/2 U, then PX/2 V

  // luma offset of the first pixel of patch (hp, wp) of frame n, and the
  // offset of its first chroma sample (I420: in the U plane)
  static __device__ __forceinline__ void offsets(
      const PatchEmbedParams& p, int n, int hp, int wp, int64_t& pix,
      int64_t& chr, int4&) {
    const int64_t fb = int64_t(n) * p.frame;
    const int64_t crow = int64_t(hp) * (P / 2);
    pix = fb + int64_t(hp) * P * p.W + int64_t(wp) * P;
    chr = fb + int64_t(p.H) * p.W +
          (I420 ? crow * (p.W / 2) + int64_t(wp) * (P / 2)
                : crow * p.W + int64_t(wp) * P);
  }
  __device__ __forceinline__ void init(const PatchEmbedParams& p, int tid,
                                       const int64_t* row_pix,
                                       const int64_t* row_chr, const int4*,
                                       const int* row_tok) {
    const int r = tid / UPR, q = tid % UPR;
    const int kp = q * PX;                             // pixel of K in a step
    const int j0 = (P == 16) ? kp / 16 : 0, px0 = (P == 16) ? kp % 16 : kp;
    W = p.W;
    lds_off = r * STRIDE + kp * 3;
    ya = ua = nullptr;
    if (row_tok[r] >= 0) {
      ya = p.img + row_pix[r] + int64_t(j0) * p.W + px0;
      ua = p.img + row_chr[r] + (I420 ? px0 / 2 : px0);
    }
  }
  __device__ __forceinline__ void load(const PatchEmbedParams& p, int s) {
#pragma unroll
    for (int w = 0; w < PXW; ++w) c[w] = 0;
#pragma unroll
    for (int jr = 0; jr < NR; ++jr)
#pragma unroll
      for (int w = 0; w < PXW; ++w) y[jr][w] = 0;
    if (ya == nullptr) return;
    const int crow = (P == 16) ? s : s >> 1;
#pragma unroll
    for (int jr = 0; jr < NR; ++jr)
      pe_load_bytes<PX>(ya + (int64_t(s) * LROWS + jr) * W, y[jr]);
    if constexpr (I420) {
      const uint8_t* u = ua + int64_t(crow) * (W / 2);
      if constexpr (PX == 4) {
        uint32_t uu, vv;
        pe_load_bytes<2>(u, &uu);
        pe_load_bytes<2>(u + p.vplane, &vv);
        c[0] = uu | (vv << 16);
      } else {
        pe_load_bytes<PX / 2>(u, c);
        pe_load_bytes<PX / 2>(u + p.vplane, c + PXW / 2);
      }
    } else {
      pe_load_bytes<PX>(ua + int64_t(crow) * W, c);
    }
  }
  __device__ __forceinline__ void store(const PatchEmbedParams& p,
                                        uint8_t* buf) const {
    uint32_t o[NR][3 * PXW];
#pragma unroll
    for (int jr = 0; jr < NR; ++jr)
#pragma unroll
      for (int w = 0; w < 3 * PXW; ++w) o[jr][w] = 0;
    const Yuv420Coef& k = p.k;
#pragma unroll
    for (int pr = 0; pr < PX / 2; ++pr) {
      const int D = pe_byte(c, I420 ? pr : 2 * pr) - 128;
      const int E = pe_byte(c, I420 ? PX / 2 + pr : 2 * pr + 1) - 128;
      const int rE = k.rv * E, gDE = k.gu * D + k.gv * E, bD = k.bu * D;
#pragma unroll
      for (int jr = 0; jr < NR; ++jr) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int j = 2 * pr + h;
          const int base = k.yc * (pe_byte(y[jr], j) - k.yoff) + 128;
          const uint32_t rgb[3] = {yuv_clamp8(base + rE),
                                   yuv_clamp8(base + gDE),
                                   yuv_clamp8(base + bD)};
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const int b = 3 * j + ch;
            o[jr][b >> 2] |= rgb[ch] << (8 * (b & 3));
          }
        }
      }
    }
    // a row past M is zeros, not the conversion of zeros
    const uint32_t keep = ya != nullptr ? 0xffffffffu : 0u;
#pragma unroll
    for (int jr = 0; jr < NR; ++jr) {
      uint8_t* dst = buf + lds_off + jr * 48;
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const uint32_t* w = &o[jr][v * PXW];
        if constexpr (PXW == 1)
          *reinterpret_cast<uint32_t*>(dst + 4 * v) = w[0] & keep;
        else if constexpr (PXW == 2)
          *reinterpret_cast<uint2*>(dst + 8 * v) =
              uint2{w[0] & keep, w[1] & keep};
        else
          *reinterpret_cast<uint4*>(dst + 16 * v) =
              uint4{w[0] & keep, w[1] & keep, w[2] & keep, w[3] & keep};
      }
    }
  }
  static __device__ __forceinline__ pe_bf16x8 frag(const uint8_t* buf, int row,
                                                  int ks, int lgrp, int) {
    return pe_byte_frag<STRIDE>(buf, row, ks, lgrp);
  }
};

// two floats -> one register holding two bf16, round to nearest even (low
// half: the first)
__device__ __forceinline__ uint32_t pe_bf16_pair(float a, float b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  union { bf16x2 h; uint32_t u; } r;
  r.h = __builtin_convertvector(f32x2{a, b}, bf16x2);
  return r.u;
}

// One fp32 result on its own: the empty asm hides it from the compiler's
// pairing of independent fp32 operations into v_pk_*_f32, so the blend below
// is scalar v_sub / v_mul / v_add, one IEEE operation each (checked in the
// ISA: no packed fp32 instruction in this file's kernels).
__device__ __forceinline__ float pe_alone(float x) {
  asm("" : "+v"(x));
  return x;
}

// Bilinear resize + crop (resize_tap.h; the blend chain of resize_run in
// pack_kernels.hip): the K values of a step are 32 pixels of the crop window
// of the resized image, which never exists in memory. A step is 96 K values
// per tile row, as for YUV: P = 16: patch rows 2s and 2s+1, P = 32: patch
// row s. The 32 * BM pixels of a step are cut into 256 units, one per thread,
// of PX consecutive output columns of one output row:
//   BM = 64: 8 pixels     BM = 32: 4 pixels
// load(): y0, y1, wy once per unit, x0 per pixel, and one 8-byte gather per
// pixel and source row: x1 is x0 or x0 + 1, so both taps of a row lie in the
// 6 bytes at pixel x0. The gather may start at any byte; it is moved back to
// the last 8 bytes of the tensor where it would run past them and shifted
// down again in store(). store(): x0, x1, wx again (cheaper than 8 more
// registers), the unfused fp32 blend v, then hi = bf16_rne(v),
// lo = bf16_rne(v - hi), both to the tile. A tile row is 96 hi values, then
// 96 lo values, then padding: STRIDE = 400 bytes.
// Where x1 == x0 (the right edge) the second tap in the 8 bytes is not the
// pixel; the weight is then replaced by 0, and p00 + 0 * (g - p00) is p00
// for any finite g, which is what p00 + wx * (p00 - p00) gives. A row past M
// gathers nothing and keeps zero registers: their blend is +0 in both pieces
// for any weights.
//
// GEO is where the source geometry (Hin, Win, rh, rw, and in the prologue the
// image's offset and crop origin) comes from: PeGeomDense, one size per
// launch, or PeGeomRagged, one size per tile row. The loader body is the same.

// Dense: the geometry is launch-uniform, read from the kernel arguments where
// it is used (scalar registers); the loader holds nothing.
struct PeGeomDense {
  static constexpr bool kTable = false;
  // pix: byte offset of image n; aux: the output pixel (row << 32 | column)
  // of the first pixel of the patch at (py0, px0) of the crop window
  static __device__ __forceinline__ void offsets(
      const PatchEmbedParams& p, int n, int py0, int px0, int64_t& pix,
      int64_t& aux, int4&) {
    pix = int64_t(n) * p.Hin * p.Win * 3;
    aux = (int64_t(py0 + p.top) << 32) | int64_t(px0 + p.left);
  }
  __device__ __forceinline__ void set(const int4&) {}
  __device__ __forceinline__ int Hin(const PatchEmbedParams& p) const {
    return p.Hin;
  }
  __device__ __forceinline__ int Win(const PatchEmbedParams& p) const {
    return p.Win;
  }
  __device__ __forceinline__ float rh(const PatchEmbedParams& p) const {
    return p.rh;
  }
  __device__ __forceinline__ float rw(const PatchEmbedParams& p) const {
    return p.rw;
  }
};

// Ragged: image n of the packed buffer is described by p.table[n]. The
// prologue thread of a tile row reads its image's entry once and leaves
// (Hin, Win, bits of rh, bits of rw) in the row's slot of an LDS table; a
// thread lifts its row's slot into four registers in init(). A row past M
// keeps a 1 x 1 geometry that nothing reads through.
struct PeGeomRagged {
  static constexpr bool kTable = true;
  int hin = 1, win = 1;
  float rh_ = 1.f, rw_ = 1.f;
  static __device__ __forceinline__ void offsets(
      const PatchEmbedParams& p, int n, int py0, int px0, int64_t& pix,
      int64_t& aux, int4& geo) {
    const PeRaggedEntry e = p.table[n];
    pix = e.offset;
    aux = (int64_t(py0 + e.top) << 32) | int64_t(px0 + e.left);
    geo = int4{e.Hin, e.Win, __float_as_int(e.rh), __float_as_int(e.rw)};
  }
  __device__ __forceinline__ void set(const int4& geo) {
    hin = geo.x;
    win = geo.y;
    rh_ = __int_as_float(geo.z);
    rw_ = __int_as_float(geo.w);
  }
  __device__ __forceinline__ int Hin(const PatchEmbedParams&) const {
    return hin;
  }
  __device__ __forceinline__ int Win(const PatchEmbedParams&) const {
    return win;
  }
  __device__ __forceinline__ float rh(const PatchEmbedParams&) const {
    return rh_;
  }
  __device__ __forceinline__ float rw(const PatchEmbedParams&) const {
    return rw_;
  }
};

template <int P, int BM_, typename GEO>
struct PeResizeLoader {
  static_assert(P == 16 || P == 32, "a 14-pixel patch row fits no unit");
  static constexpr int BM = BM_, BK = 96, PIECES = 2;
  static constexpr int PIECE = 2 * BK;                 // bytes of one piece
  static constexpr int STRIDE = 2 * PIECE + 16;        // 25 16-byte slots
  static constexpr bool kAux = true;                   // the pixel origins
  static constexpr bool kGeom = GEO::kTable;           // per-row geometry
  static constexpr int UPR = kPeThreads / BM;          // units per tile row
  static_assert(UPR == 4 || UPR == 8, "one unit per thread");
  static constexpr int PX = 32 / UPR;                  // 8 or 4
  static constexpr int LROWS = (P == 16) ? 2 : 1;      // output rows per step

  int64_t img;           // byte offset of the unit's image; -1: row past M
  int oy0, ox0;          // the unit's output pixel at step 0
  int lds_off;
  float wy;
  int d[2];              // (offset of source row y0 / y1) - src_last, clamped
  uint2 tap[2][PX];
  GEO g;

  static __device__ __forceinline__ void offsets(
      const PatchEmbedParams& p, int n, int hp, int wp, int64_t& pix,
      int64_t& aux, int4& geo) {
    GEO::offsets(p, n, hp * P, wp * P, pix, aux, geo);
  }
  __device__ __forceinline__ void init(const PatchEmbedParams&, int tid,
                                       const int64_t* row_pix,
                                       const int64_t* row_aux,
                                       const int4* row_geo,
                                       const int* row_tok) {
    const int r = tid / UPR, q = tid % UPR;
    const int kp = q * PX;                             // pixel of K in a step
    const int j0 = (P == 16) ? kp / 16 : 0, px0 = (P == 16) ? kp % 16 : kp;
    lds_off = r * STRIDE + kp * 6;
    img = row_tok[r] >= 0 ? row_pix[r] : int64_t(-1);
    if constexpr (GEO::kTable)
      if (img >= 0) g.set(row_geo[r]);
    oy0 = int(row_aux[r] >> 32) + j0;
    ox0 = int(row_aux[r] & 0xffffffff) + px0;
    wy = 0.f;
    d[0] = d[1] = -(1 << 30);                          // no shift
  }
  __device__ __forceinline__ void load(const PatchEmbedParams& p, int s) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < PX; ++i) tap[j][i] = uint2{0u, 0u};
    if (img < 0) return;
    int y[2];
    resize_tap(oy0 + s * LROWS, 0, g.rh(p), g.Hin(p), y[0], y[1], wy);
    int64_t row[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      row[j] = img + int64_t(y[j]) * g.Win(p) * 3;
      const int64_t over = row[j] - p.src_last;
      d[j] = int(over > -(int64_t(1) << 30) ? over : -(int64_t(1) << 30));
    }
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      int x0, x1;
      float wx;
      resize_tap(ox0 + i, 0, g.rw(p), g.Win(p), x0, x1, wx);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // row + x0*3 + 3 <= bytes of img, src_last >= 0: inside the tensor
        const int64_t a = row[j] + x0 * 3;
        __builtin_memcpy(&tap[j][i],
                         p.img + (a < p.src_last ? a : p.src_last), 8);
      }
    }
  }
  __device__ __forceinline__ void store(const PatchEmbedParams& p,
                                        uint8_t* buf) const {
    uint32_t hi[3 * PX / 2], lo[3 * PX / 2];
    float v[3 * PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      int x0, x1;
      float wx;
      resize_tap(ox0 + i, 0, g.rw(p), g.Win(p), x0, x1, wx);
      wx = x1 == x0 ? 0.f : wx;
      uint32_t w[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int sh = 8 * max(d[j] + x0 * 3, 0);      // 0 .. 40
        const uint64_t t =
            ((uint64_t(tap[j][i].y) << 32) | tap[j][i].x) >> sh;
        w[j][0] = uint32_t(t);
        w[j][1] = uint32_t(t >> 32);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p00 = float(pe_byte(w[0], c));
        const float p01 = float(pe_byte(w[0], 3 + c));
        const float p10 = float(pe_byte(w[1], c));
        const float p11 = float(pe_byte(w[1], 3 + c));
        const float t = pe_alone(__fadd_rn(p00, pe_alone(__fmul_rn(
            wx, pe_alone(__fsub_rn(p01, p00))))));
        const float b = pe_alone(__fadd_rn(p10, pe_alone(__fmul_rn(
            wx, pe_alone(__fsub_rn(p11, p10))))));
        v[3 * i + c] = pe_alone(__fadd_rn(t, pe_alone(__fmul_rn(
            wy, pe_alone(__fsub_rn(b, t))))));
      }
    }
#pragma unroll
    for (int k = 0; k < 3 * PX / 2; ++k) {
      const float a = v[2 * k], b = v[2 * k + 1];
      hi[k] = pe_bf16_pair(a, b);
      // v - hi is exact: hi keeps the leading 8 bits of v
      lo[k] = pe_bf16_pair(
          pe_alone(__fsub_rn(a, __uint_as_float(hi[k] << 16))),
          pe_alone(__fsub_rn(b, __uint_as_float(hi[k] & 0xffff0000u))));
    }
    uint8_t* dst = buf + lds_off;
    if constexpr (PX == 8) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        *reinterpret_cast<uint4*>(dst + 16 * q) =
            uint4{hi[4 * q], hi[4 * q + 1], hi[4 * q + 2], hi[4 * q + 3]};
        *reinterpret_cast<uint4*>(dst + PIECE + 16 * q) =
            uint4{lo[4 * q], lo[4 * q + 1], lo[4 * q + 2], lo[4 * q + 3]};
      }
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        *reinterpret_cast<uint2*>(dst + 8 * q) =
            uint2{hi[2 * q], hi[2 * q + 1]};
        *reinterpret_cast<uint2*>(dst + PIECE + 8 * q) =
            uint2{lo[2 * q], lo[2 * q + 1]};
      }
    }
  }
  // 8 K-contiguous bf16 of one piece: one 16-byte read, already MFMA layout
  static __device__ __forceinline__ pe_bf16x8 frag(const uint8_t* buf, int row,
                                                  int ks, int lgrp,
                                                  int piece) {
    return *reinterpret_cast<const pe_bf16x8*>(
        &buf[row * STRIDE + piece * PIECE + ks * 64 + lgrp * 16]);
  }
};

// A source: its loader for a tile of BM rows, and the rows of its large tile
template <int P>
struct PeRgb {
  static constexpr int kLargeM = kPeLargeM;
  template <int BM> using Loader = PeRgbLoader<P, BM>;
};
template <int P, bool I420>
struct PeYuv {
  static constexpr int kLargeM = kPeLargeM;
  template <int BM> using Loader = PeYuvLoader<P, BM, I420>;
};
template <int P>
struct PeResize {
  static constexpr int kLargeM = kPeResizeLargeM;
  template <int BM> using Loader = PeResizeLoader<P, BM, PeGeomDense>;
};
template <int P>
struct PeRagged {
  static constexpr int kLargeM = kPeResizeLargeM;
  template <int BM> using Loader = PeResizeLoader<P, BM, PeGeomRagged>;
};

// a second int64 per tile row (chroma offset, pixel origin): LDS only in
// kernels whose loader asks
template <int BM>
__device__ __forceinline__ int64_t* pe_aux_table() {
  __shared__ int64_t row_aux[BM];
  return row_aux;
}

// the source geometry of a tile row's image (ragged loader only)
template <int BM>
__device__ __forceinline__ int4* pe_geo_table() {
  __shared__ int4 row_geo[BM];
  return row_geo;
}

template <typename LD, int TN, typename OUT>
__global__ void __launch_bounds__(kPeThreads)
patch_embed_kernel(const PatchEmbedParams p) {
  constexpr int BM = LD::BM, TM = BM / 32, BN = 32 * TN;
  constexpr int KS = LD::BK / 32;                  // MFMA slabs per step
  using OutT = typename OUT::T;

  __shared__ __attribute__((aligned(16))) uint8_t a_lds[2][BM * LD::STRIDE];
  __shared__ int64_t row_pix[BM];   // byte offset of the patch's first pixel
  __shared__ int row_tok[BM];       // token index inside the image, -1: past M
  __shared__ int row_img[BM];
  int64_t* row_aux = nullptr;       // first chroma offset / pixel origin
  if constexpr (LD::kAux) row_aux = pe_aux_table<BM>();
  int4* row_geo = nullptr;          // source geometry of the row's image
  if constexpr (LD::kGeom) row_geo = pe_geo_table<BM>();

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 15, lgrp = lane >> 4;
  const int tile_n = int(blockIdx.x % uint32_t(p.tiles_n));
  const int m0 = int(blockIdx.x / uint32_t(p.tiles_n)) * BM;
  const int d0 = tile_n * BN;

  if (tid < BM) {
    const int m = m0 + tid;
    int tok = -1, n = 0;
    int64_t pix = 0, aux = 0;
    int4 geo{0, 0, 0, 0};
    if (m < p.M) {
      n = m / p.HW;
      tok = m - n * p.HW;
      const int hp = tok / p.Wp, wp = tok - hp * p.Wp;
      LD::offsets(p, n, hp, wp, pix, aux, geo);
    }
    row_pix[tid] = pix;
    if constexpr (LD::kAux) row_aux[tid] = aux;
    if constexpr (LD::kGeom) row_geo[tid] = geo;
    row_tok[tid] = tok;
    row_img[tid] = n;
  }
  __syncthreads();

  LD ld;
  ld.init(p, tid, row_pix, row_aux, row_geo, row_tok);

  // B rows of this lane; a block past D reads row D-1 and is never stored
  const uint16_t* b_row[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    int d = d0 + (wn * TN + tn) * 16 + lrow;
    d = d < p.D ? d : p.D - 1;
    b_row[tn] = p.wk + int64_t(d) * p.Kp + lgrp * 8;
  }
  uint4 b_next[KS][TN], b_cur[KS][TN];
  auto load_b = [&](int k0) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
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

  const int steps = (p.Kp + LD::BK - 1) / LD::BK;
  ld.load(p, 0);
  load_b(0);
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    ld.store(p, a_lds[buf]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) b_cur[ks][tn] = b_next[ks][tn];
    // one barrier per step: buffer buf was last read two steps ago, and
    // every thread has passed the barrier of the step in between
    __syncthreads();
    if (s + 1 < steps) {
      ld.load(p, s + 1);
      load_b((s + 1) * LD::BK);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // the pieces of a slab in order (hi, then lo) into the one accumulator
#pragma unroll
      for (int piece = 0; piece < LD::PIECES; ++piece) {
        pe_bf16x8 a[TM];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          a[tm] = LD::frag(a_lds[buf], (wm * TM + tm) * 16 + lrow, ks, lgrp,
                           piece);
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

template <typename LD, int TN, typename OUT>
void launch_patch_embed(const PatchEmbedParams& p, int64_t tiles,
                        hipStream_t stream) {
  hipLaunchKernelGGL((patch_embed_kernel<LD, TN, OUT>),
                     dim3(uint32_t(tiles)), dim3(kPeThreads), 0, stream, p);
}

template <typename LD, int TN>
void launch_patch_embed_out(at::ScalarType out_dtype,
                            const PatchEmbedParams& p, int64_t tiles,
                            hipStream_t stream) {
  if (out_dtype == at::kFloat)
    launch_patch_embed<LD, TN, PeOutF32>(p, tiles, stream);
  else if (out_dtype == at::kBFloat16)
    launch_patch_embed<LD, TN, PeOutBf16>(p, tiles, stream);
  else
    launch_patch_embed<LD, TN, PeOutF16>(p, tiles, stream);
}

// SRC: PeRgb<P>, PeYuv<P, I420>, PeResize<P> or PeRagged<P>
template <typename SRC>
void launch_patch_embed_tile(bool large, at::ScalarType out_dtype,
                             const PatchEmbedParams& p, int64_t tiles,
                             hipStream_t stream) {
  if (large)
    launch_patch_embed_out<typename SRC::template Loader<SRC::kLargeM>,
                           kPeLargeN / 32>(out_dtype, p, tiles, stream);
  else
    launch_patch_embed_out<typename SRC::template Loader<kPeSmallM>,
                           kPeSmallN / 32>(out_dtype, p, tiles, stream);
}

enum class PeSource { kRgb, kNv12, kI420, kResize, kRagged };

// kResize: the source geometry, checked by the caller; kRagged: the device
// table that holds it per image
struct PeResizeArgs {
  int64_t Hin = 0, Win = 0, top = 0, left = 0;
  float rh = 0.f, rw = 0.f;
  const PeRaggedEntry* table = nullptr;
};

// The part of the entry points below that does not depend on the pixel
// format: `in` holds N images that give H x W pixels each (kResize and
// kRagged: H x W is the crop window, `rz` the source side) and was checked by
// the caller.
at::Tensor patch_embed_run(const char* who, const at::Tensor& in,
                           PeSource src, const Yuv420Coef& coef, int64_t N,
                           int64_t H, int64_t W, const at::Tensor& wk,
                           const at::Tensor& bias, int64_t patch,
                           const c10::optional<at::Tensor>& pos,
                           const c10::optional<at::Tensor>& cls,
                           at::ScalarType out_dtype, int64_t tile,
                           const PeResizeArgs& rz = PeResizeArgs{}) {
  TORCH_CHECK_VALUE(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
                    out_dtype == at::kHalf,
                    who, ": out_dtype must be f32, bf16 or f16");
  TORCH_CHECK_VALUE(tile >= 0 && tile <= 2, who, ": tile must be 0, 1 or 2");
  TORCH_CHECK_VALUE(H >= patch && W >= patch && H % patch == 0 &&
                    W % patch == 0, who, ": H and W must be positive "
                    "multiples of patch ", patch, ", got ", H, "x", W);
  const int64_t Hp = H / patch, Wp = W / patch, HW = Hp * Wp, M = N * HW;
  const int64_t K = 3 * patch * patch, Kp = (K + 31) / 32 * 32;
  auto on_device = [&](const at::Tensor& t) {
    return t.is_cuda() && t.get_device() == in.get_device() &&
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
  // 16-byte loads of pixels (P = 16, 32) and of weight fragments; the YUV
  // units' narrower loads are aligned to their width when the frames are;
  // the resampling loader gathers at any byte
  const bool ragged = src == PeSource::kRagged;
  const bool resize = src == PeSource::kResize || ragged;
  TORCH_CHECK_VALUE(
      (resize ||
       reinterpret_cast<uintptr_t>(in.const_data_ptr()) % 16 == 0) &&
      reinterpret_cast<uintptr_t>(wk.const_data_ptr()) % 16 == 0, who,
      ": images and wk must be 16-byte aligned");

  auto out = at::empty({N, T, D}, in.options().dtype(out_dtype));
  if (N == 0) return out;                 // zero grid: never launch

  auto tiles_of = [&](int64_t bm, int64_t bn) {
    return ((M + bm - 1) / bm) * ((D + bn - 1) / bn);
  };
  const int64_t large_m = resize ? kPeResizeLargeM : kPeLargeM;
  const bool large = tile == 2 ||
      (tile == 0 && tiles_of(large_m, kPeLargeN) >=
           (resize ? kPeResizeLargeMinTiles : kPeLargeMinTiles));
  const int64_t bn = large ? kPeLargeN : kPeSmallN;
  const int64_t tiles = large ? tiles_of(large_m, kPeLargeN)
                              : tiles_of(kPeSmallM, kPeSmallN);
  TORCH_CHECK_VALUE(tiles <= std::numeric_limits<int32_t>::max(), who,
                    ": too many tiles");

  PatchEmbedParams p;
  p.img = static_cast<const uint8_t*>(in.const_data_ptr());
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
  p.frame = H * W * 3 / 2;
  p.vplane = (H / 2) * (W / 2);
  p.k = coef;
  p.Hin = int(rz.Hin); p.Win = int(rz.Win);
  p.top = int(rz.top); p.left = int(rz.left);
  p.rh = rz.rh; p.rw = rz.rw;
  p.src_last = in.numel() - 8;            // resize: the caller saw to >= 0
  p.table = rz.table;

  hipStream_t stream = at::hip::getCurrentHIPStream().stream();
  const bool p16 = patch == 16;
  if (ragged) {
    if (p16)
      launch_patch_embed_tile<PeRagged<16>>(large, out_dtype, p, tiles,
                                            stream);
    else
      launch_patch_embed_tile<PeRagged<32>>(large, out_dtype, p, tiles,
                                            stream);
  } else if (resize) {
    if (p16)
      launch_patch_embed_tile<PeResize<16>>(large, out_dtype, p, tiles,
                                            stream);
    else
      launch_patch_embed_tile<PeResize<32>>(large, out_dtype, p, tiles,
                                            stream);
  } else if (src == PeSource::kNv12) {
    if (p16)
      launch_patch_embed_tile<PeYuv<16, false>>(large, out_dtype, p, tiles,
                                                stream);
    else
      launch_patch_embed_tile<PeYuv<32, false>>(large, out_dtype, p, tiles,
                                                stream);
  } else if (src == PeSource::kI420) {
    if (p16)
      launch_patch_embed_tile<PeYuv<16, true>>(large, out_dtype, p, tiles,
                                               stream);
    else
      launch_patch_embed_tile<PeYuv<32, true>>(large, out_dtype, p, tiles,
                                               stream);
  } else if (patch == 14) {
    launch_patch_embed_tile<PeRgb<14>>(large, out_dtype, p, tiles, stream);
  } else if (p16) {
    launch_patch_embed_tile<PeRgb<16>>(large, out_dtype, p, tiles, stream);
  } else {
    launch_patch_embed_tile<PeRgb<32>>(large, out_dtype, p, tiles, stream);
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(err) + " at " + who);
  return out;
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
  return patch_embed_run(who, images, PeSource::kRgb, Yuv420Coef{},
                         images.size(0), images.size(1), images.size(2), wk,
                         bias, patch, pos, cls, out_dtype, tile);
}

// The same from YUV 4:2:0 frames: ``frames`` is uint8 [N, H*3/2, W], NV12 or
// (``i420``) I420 as laid out in the YUV section of pack_kernels.hip, and
// ``coef`` is (yoff, yc, rv, gu, gv, bu) of the int32 conversion. The result
// is bit-identical to u8_patch_embed on the converted RGB frames, which never
// exist in memory. Patches are 16 and 32.
at::Tensor yuv420_patch_embed(const at::Tensor& frames, const at::Tensor& wk,
                              const at::Tensor& bias, int64_t patch,
                              const c10::optional<at::Tensor>& pos,
                              const c10::optional<at::Tensor>& cls,
                              at::ScalarType out_dtype, int64_t tile,
                              bool i420, std::vector<int64_t> coef) {
  const char* who = "yuv420_patch_embed";
  constexpr int64_t kMaxSide = 16384;
  TORCH_CHECK_VALUE(frames.is_cuda() && frames.dim() == 3 &&
                    frames.is_contiguous() &&
                    frames.scalar_type() == at::kByte,
                    who, " expects a contiguous uint8 device tensor "
                    "[N,H*3/2,W]");
  TORCH_CHECK_VALUE(patch == 16 || patch == 32, who,
                    ": patch must be 16 or 32, got ", patch);
  TORCH_CHECK_VALUE(frames.size(1) % 3 == 0, who,
                    ": rows must be a multiple of 3");
  const int64_t H = frames.size(1) / 3 * 2, W = frames.size(2);
  TORCH_CHECK_VALUE(H >= 2 && H <= kMaxSide && W >= 2 && W <= kMaxSide &&
                    H % 2 == 0 && W % 2 == 0, who,
                    ": frame sides must be even and in 2..16384");
  TORCH_CHECK_VALUE(coef.size() == 6, who, ": coef needs 6 values");
  for (int64_t v : coef)   // sums stay far inside int32
    TORCH_CHECK_VALUE(v >= -4096 && v <= 4096, who,
                      ": coefficient out of range");
  const Yuv420Coef k{int(coef[0]), int(coef[1]), int(coef[2]), int(coef[3]),
                     int(coef[4]), int(coef[5])};
  return patch_embed_run(who, frames, i420 ? PeSource::kI420 : PeSource::kNv12,
                         k, frames.size(0), H, W, wk, bias, patch, pos, cls,
                         out_dtype, tile);
}

// The same from images of any size: ``images`` is uint8 [N,Hin,Win,3]; the
// tokens are those of the Hc x Wc window at (top, left) of the bilinear
// resize whose ratios ``rh`` / ``rw`` are float(Hin/Hr) / float(Win/Wr),
// rounded by the caller exactly as for u8_nhwc_resize_normalize
// (ops.image_u8_resize_patch_embed, which also validates the window against
// the resized size). The operand is the fp32 blend as two bf16 pieces, see
// the header. Patches are 16 and 32.
at::Tensor u8_resize_patch_embed(const at::Tensor& images, double rh,
                                 double rw, int64_t top, int64_t left,
                                 int64_t Hc, int64_t Wc, const at::Tensor& wk,
                                 const at::Tensor& bias, int64_t patch,
                                 const c10::optional<at::Tensor>& pos,
                                 const c10::optional<at::Tensor>& cls,
                                 at::ScalarType out_dtype, int64_t tile) {
  const char* who = "u8_resize_patch_embed";
  constexpr int64_t kMaxSide = 16384;
  TORCH_CHECK_VALUE(images.is_cuda() && images.dim() == 4 &&
                    images.is_contiguous() &&
                    images.scalar_type() == at::kByte && images.size(3) == 3,
                    who, " expects a contiguous uint8 device tensor "
                    "[N,Hin,Win,3]");
  TORCH_CHECK_VALUE(patch == 16 || patch == 32, who,
                    ": patch must be 16 or 32, got ", patch);
  const int64_t N = images.size(0), Hin = images.size(1),
                Win = images.size(2);
  TORCH_CHECK_VALUE(Hin >= 1 && Hin <= kMaxSide && Win >= 1 &&
                    Win <= kMaxSide, who,
                    ": input sides must be in 1..16384");
  TORCH_CHECK_VALUE(Hc >= 1 && Wc >= 1 && top >= 0 && left >= 0 &&
                    top + Hc <= kMaxSide && left + Wc <= kMaxSide, who,
                    ": bad crop window");
  TORCH_CHECK_VALUE(rh > 0.0 && rw > 0.0 && rh <= double(kMaxSide) &&
                    rw <= double(kMaxSide), who,
                    ": ratios must be in (0, 16384]");
  // the loader gathers 8 bytes at a time: a smaller batch gets a tail
  at::Tensor src = images;
  if (N > 0 && images.numel() < 8) {
    src = at::zeros({8}, images.options());
    src.narrow(0, 0, images.numel()).copy_(images.view({-1}));
  }
  PeResizeArgs rz;
  rz.Hin = Hin; rz.Win = Win; rz.top = top; rz.left = left;
  rz.rh = float(rh); rz.rw = float(rw);
  return patch_embed_run(who, src, PeSource::kResize, Yuv420Coef{}, N, Hc, Wc,
                         wk, bias, patch, pos, cls, out_dtype, tile, rz);
}

// The same from a ragged batch: ``data`` is the flat uint8 buffer of N RGB
// images of N different sizes, HWC, back to back with no padding; ``table``
// is the int32 [N,8] device image of PeRaggedEntry rows, one per image (its
// offset, size, crop origin and ratios; the layout of
// u8_ragged_resize_normalize), already on the device. Every image gives the
// tokens of its own Hc x Wc window, exactly those of u8_resize_patch_embed on
// that image alone. ops.image_u8_ragged_resize_patch_embed builds the table
// on the host, validates every entry against the buffer size and copies it
// on the current stream from a pinned buffer. The kernel trusts the table:
// callers other than that op must make the same checks. Patches are 16 and
// 32.
at::Tensor u8_ragged_resize_patch_embed(
    const at::Tensor& data, const at::Tensor& table, int64_t Hc, int64_t Wc,
    const at::Tensor& wk, const at::Tensor& bias, int64_t patch,
    const c10::optional<at::Tensor>& pos,
    const c10::optional<at::Tensor>& cls, at::ScalarType out_dtype,
    int64_t tile) {
  const char* who = "u8_ragged_resize_patch_embed";
  constexpr int64_t kMaxSide = 16384;
  TORCH_CHECK_VALUE(data.is_cuda() && data.dim() == 1 &&
                    data.is_contiguous() && data.scalar_type() == at::kByte,
                    who, " expects a contiguous 1-D uint8 device tensor");
  TORCH_CHECK_VALUE(table.is_cuda() &&
                    table.get_device() == data.get_device() &&
                    table.dim() == 2 && table.size(1) == 8 &&
                    table.is_contiguous() && table.scalar_type() == at::kInt,
                    who, ": table must be a contiguous int32 [N,8] tensor on "
                    "the device of the input");
  TORCH_CHECK_VALUE(
      reinterpret_cast<uintptr_t>(table.const_data_ptr()) % 8 == 0, who,
      ": table must be 8-byte aligned");
  TORCH_CHECK_VALUE(patch == 16 || patch == 32, who,
                    ": patch must be 16 or 32, got ", patch);
  TORCH_CHECK_VALUE(Hc >= 1 && Wc >= 1 && Hc <= kMaxSide && Wc <= kMaxSide,
                    who, ": bad crop window");
  const int64_t N = table.size(0);
  // an image is at least one pixel
  TORCH_CHECK_VALUE(data.numel() >= 3 * N, who, ": table has ", N,
                    " images but data only ", data.numel(), " bytes");
  // the loader gathers 8 bytes at a time: a smaller batch gets a tail
  at::Tensor src = data;
  if (N > 0 && data.numel() < 8) {
    src = at::zeros({8}, data.options());
    src.narrow(0, 0, data.numel()).copy_(data);
  }
  PeResizeArgs rz;
  rz.table = static_cast<const PeRaggedEntry*>(table.const_data_ptr());
  return patch_embed_run(who, src, PeSource::kRagged, Yuv420Coef{}, N, Hc, Wc,
                         wk, bias, patch, pos, cls, out_dtype, tile, rz);
}

}  // namespace mi355x
