// Fused length-masked multi-head self-attention for gfx950 (CDNA4, wave64):
// the qkv projection in, the attention output out, one launch, matrix cores.
//
//   qkv [B,S,3*H] bf16 / f16, last axis ordered (3, heads, 64), as the
//                 encoder's nn.Linear wrote it          lengths int32 [B] / null
//   L = clamp(lengths[b], 0, S)                          (null: L = S)
//   out[b,s,h*64+d] = sum_{j<L} softmax_{j<L}((q_s . k_j) * scale) v_j[d], s < L
//   out[b,s,:]      = +0.0                                        L <= s < S
//
// A mask here is always a prefix given by a length, so nothing at or past L
// is ever loaded: not a q row, not a k row, not a v row. A NaN or Inf stored
// there cannot reach a kept output. Padded keys of a partial tile are zeros in
// LDS (0 x NaN is NaN in an MFMA, so V has to be clean, not just P) and their
// scores are REPLACED by -inf before the maximum and by 0 after the exp.
//
// Work split. A workgroup of 4 waves owns a 64-row query tile of one
// (b, head); a wave owns 16 query rows. The grid is flat, blockIdx.x =
// (b * heads + head) * ceil(S/64) + tile, so B * heads may pass 65535 and the
// workgroups that share one head's K and V run next to each other. A
// workgroup whose tile starts at or past L stores 64 rows of zeros and
// leaves; the others walk ceil(L/64) key tiles of BN = 64 keys. A wave whose
// 16 rows are all padding takes part in the staging and the barriers and
// skips the arithmetic.
//
// Packed (varlen) form, a value of the template parameter FORM of the one
// body. qkv is
// [T,3*H] and out [T,H], sequences back to back with no padding, and an int32
// table [ntiles,4] holds one row (row0, L, q0, seq) per 64-row query tile:
// the sequence's first packed row, its length, the tile's first query (a
// multiple of 64 below L) and the sequence's index (not read here). The grid
// is exact, blockIdx.x = entry * heads + head with ntiles * heads workgroups:
// none exits empty, head-minor keeps the table's order as the dispatch order,
// and the q tiles of one (sequence, head) are `heads` workgroups apart, so
// they still run at the same time and share K and V through L2. A workgroup
// reads its entry once (16 bytes, scalar), addresses row row0 + s where the
// padded form addresses b * S + s, and from there on runs the same code: the
// tile alignment relative to the sequence start is the same, so a sequence's
// output is bit-identical to the padded form's.
//  * Store rule: only rows q0 .. min(q0 + 64, L) - 1 are stored. There are no
//    padded rows, so no zero-fill, and a store at or past row0 + L would
//    overwrite the next sequence. "Nothing at or past L is loaded" now also
//    means that no row of a neighbouring sequence is loaded.
//  * Clamps: row0 to 0..T, L to 0..T - row0, q0 to >= 0; an entry with
//    q0 >= L does nothing. No table can make the kernel touch a row outside
//    0..T, the policy of the on-device clamp of `lengths`. Rows of out that
//    no entry covers are unspecified.
//  * Entry order: a workgroup walks ceil(L/64) key tiles, so its cost grows
//    with L. The host helper emits the longest sequence first (stable, tiles
//    ascending inside a sequence), so a batch's long sequences start first
//    and do not form the tail. Measured on an MI355X (bf16, 12 heads, 128
//    sequences of 16..512 tokens, 6528 workgroups, 7 interleaved rounds of
//    200 calls, median and range): longest first 93.4 us (93.2-95.8),
//    sequence order 97.9 us (97.3-99.5), the padded form 145.8 us; a second
//    run gave 94.2 (92.8-95.1) against 98.6 (98.2-101.0). The ranges do not
//    overlap, so longest first is kept and sequence order is not an option.
//    At full length (274 us) and at 8 x 128 (5.9 us, launch bound) the order
//    makes no measurable difference.
//
// Keys form, the third value of the template parameter FORM: an arbitrary
// key mask [B,S], as a dense request's attention_mask is. A mask with c kept
// keys is the prefix case behind one indirection: attention_keys_kernel (one
// launch per request, one wave per sequence) writes the ascending list of
// kept positions index[b, :c] and c = count[b], every block of the model
// shares the pair, and this kernel walks ceil(c/64) key tiles and loads K and
// V row index[b, j] where the padded form loads row j. Only the last tile is
// partial, exactly as there, and cost follows the kept keys wherever they
// lie. The grid is the padded form's.
//  * Every query row s < S is loaded, computed and stored: a padded query
//    attends to the kept keys, which is what the additive finfo.min mask of
//    the library path gives, so the encoder's output matches that path at
//    padded positions too. K and V rows of masked positions are never
//    loaded.
//  * c == 0: under the additive mask every score rounds to finfo.min and the
//    softmax is uniform over ALL S keys. Here: c = S, identity index (no
//    table read), score scale 0.
//  * Clamps: count to 0..S, each index to 0..S-1, on the device: no table
//    can make the kernel touch a row outside the sequence.
//  * A query's result depends only on its own row and on the order and
//    tiling of the keys, so out[b, kept] is bit-identical to the padded form
//    run on the compacted sequence qkv[b, kept].
//  * The new cost is a dependent load, index then row. The thread's four
//    indices of tile t + 2 are fetched right after the row loads of tile
//    t + 1 are issued, one whole tile of arithmetic before they are used, so
//    no row load waits on an index load of its own step (only tile 0 does).
//    That is 4 more VGPRs. The alternative, staging the sequence's whole
//    list in LDS once, was not built: the 4 KB left under the 40 KB that
//    keep four workgroups per CU hold 1024 indices, so S > 1024 would need
//    a second path, and it adds a barrier before the first tile. Neither has
//    been timed on an MI355X yet; profiles/README.md says what to measure.
//
// Small problems. There is one tile. B = 1, S = 128 is 24 workgroups of 2 key
// tiles on 256 CUs, and such a launch is bound by the launch itself: measured
// on an MI355X (bf16, 12 heads, calls back to back), B = 8, S = 128 (192
// workgroups) and B = 1, S = 32 (12 workgroups) both take 5.4 us per call,
// against 17 us for the library chain. A 16-row tile would raise the
// workgroup count without shortening what is measured, so there is no second
// tile and no rule to pick one.
//
// Layouts. v_mfma_f32_16x16x32_{bf16,f16} computes D[16x16] += A[16x32] *
// B[32x16]: lane l gives A row l % 16 and B column l % 16, both at k = 8 *
// (l / 16) .. + 7, and gets D column l % 16, rows 4 * (l / 16) + 0..3. Write
// r = l % 16 and g = l / 16.
//  * Scores are computed transposed, S^T = K Q^T: A is a 16-key block of the
//    K tile, B is the wave's Q fragment (query r, d = 32 * slab + 8g .. + 7:
//    two 16-byte global loads that stay in registers for the whole key loop).
//    Four key blocks x two d slabs = 8 MFMAs per tile, and lane (r, g) holds
//    the scores of ONE query, r, against keys 16 * kb + 4g + i (kb, i < 4).
//    So the row maximum and the row sum are 16 values in the lane and two
//    butterfly steps (xor 16, 32) across g; the running maximum, sum and
//    rescale factor of query r live in the lanes that hold query r.
//  * The output is computed transposed as well, O^T = V^T P^T: A is V^T
//    (row d, k = keys), B is P^T (column = query r, k = keys), and the lane
//    gets query r again, d = 16 * db + 4g + 0..3. The rescale by
//    exp(m_old - m_new) and the final division are per lane, no shuffle, and
//    the store is 4 contiguous values (8 bytes).
//  * P goes from accumulator to operand layout WITHOUT a round trip: the lane
//    already holds 8 keys of its query per 32-key slab ks, keys 32ks + 4g + i
//    and 32ks + 16 + 4g + i. They become k = 8g + i and 8g + 4 + i of that
//    slab. The contraction index is a dummy, so any order works as long as V
//    uses the same one: key 32ks + 16b + 4g + i sits at column 32ks + 8g + 4b
//    + i of the V^T tile in LDS. That permutation is applied once, by the
//    staging stores.
//  * V is transposed on the way into LDS. A thread loads 16 bytes (8 d) of
//    two neighbouring keys and stores 8 words, each the pair (key 2j, key
//    2j+1) of one d; a pair stays a pair under the permutation above.
//
// K loop. K and V tiles are loaded from global memory into registers one
// tile ahead (4 x 16 bytes per thread), then stored to one of two LDS buffers;
// one barrier per tile (buffer t & 1 was last read two tiles ago, and every
// wave has passed the barrier in between). Per tile and wave: 8 MFMAs for
// S^T, the online softmax in fp32 (scale * log2(e) folded into one multiply,
// v_exp_f32), P rounded once to the input dtype, 8 MFMAs for O^T.
//
// LDS. K tile [64 keys][64 d] and V^T tile [64 d][64 key slots], both with a
// row stride of 144 bytes = 36 words = 9 slots of 16 bytes. Fragment reads
// are 16 bytes per lane at row r (+ 16g bytes): 36 r mod 64 for r = 0..15 is
// 0, 36, 8, 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20, 56, 28, sixteen
// different multiples of 4, so the 16 lanes of a group cover all 64 banks
// once: conflict-free, for K and V^T alike. K stores are 16 bytes, 8
// neighbouring lanes fill one row. V^T stores are words: lanes 0..31 of a
// wave hold the 32 key pairs of d chunk 2 * wave, lanes 32..63 those of chunk
// 2 * wave + 1; at step i the first half writes row 8c + i, where the 32
// pairs are a permutation of words 0..31, and the second half writes row
// 8c + 8 + i, 8 * 36 = 288 = 32 (mod 64) banks further: 64 different banks.
// 2 buffers x 2 tiles x 64 x 144 B = 36 KB.
//
// Arithmetic. 16-bit products are exact in fp32 and the MFMA accumulates in
// fp32. Scale, maximum, exp and sum are fp32; the sum adds the unrounded P.
// One IEEE division by the row sum and one round-to-nearest-even conversion
// at the store. No split of the key axis, no atomics; every output element is
// written by one lane and every reduction has a fixed order, so reruns are
// bit-identical and a sequence does not see its batch neighbours.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off
// --cuda-device-only -Rpass-analysis=kernel-resource-usage; the build does
// not pass the last two):
//   dtype  form    VGPRs  AGPRs  SGPRs  LDS bytes  scratch  occupancy (waves/SIMD)
//   bf16   padded     99     16     60      36864        0     4
//   f16    padded     99     16     60      36864        0     4
//   bf16   packed     97     16     61      36864        0     4
//   f16    packed     97     16     61      36864        0     4
//   bf16   keys      103     16     68      36864        0     4
//   f16    keys      103     16     68      36864        0     4
// 4 waves/SIMD is 4 workgroups per CU, 144 KB of its 160 KB of LDS. The
// key-index kernel (both mask widths): 6 VGPRs, 21 SGPRs, no LDS, 0 scratch.
#include <hip/hip_runtime.h>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <tuple>

namespace mi355x {
namespace {

constexpr int kAtThreads = 256;             // 4 waves
constexpr int kAtBM = 64;                   // query rows per workgroup
constexpr int kAtBN = 64;                   // keys per tile
constexpr int kAtD = 64;                    // head_dim
constexpr int kAtStride = 144;              // LDS row stride, bytes
constexpr int kAtTileBytes = 64 * kAtStride;
constexpr int kAtBufBytes = 2 * kAtTileBytes;         // K tile + V^T tile

typedef float at_f32x4 __attribute__((ext_vector_type(4)));

struct AtBf16 {
  using E = __bf16;
  typedef __bf16 V8 __attribute__((ext_vector_type(8)));
  typedef __bf16 V4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ at_f32x4 mfma(V8 a, V8 b, at_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

struct AtF16 {
  using E = _Float16;
  typedef _Float16 V8 __attribute__((ext_vector_type(8)));
  typedef _Float16 V4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ at_f32x4 mfma(V8 a, V8 b, at_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

struct AttnParams {
  const void* qkv;          // [B,S,3H], packed: [T,3H]
  const int32_t* lengths;   // [B] or null (padded form only)
  const int32_t* tiles;     // packed: [ntiles,4] of (row0, L, q0, seq)
  const int32_t* index;     // keys: [B,S] kept key positions, ascending
  const int32_t* count;     // keys: [B] number of kept keys
  void* out;                // [B,S,H], packed: [T,H]
  int S, heads, qtiles;     // packed: S is T, qtiles is unused
  float scale_log2e;        // scale * log2(e)
};

enum AtForm { kAtPadded, kAtPacked, kAtKeys };

// FORM selects where a workgroup finds its work and which row a key slot
// names, nothing else: the padded form derives (b, head, tile) from
// blockIdx.x and reads lengths[b]; the packed form reads one row of the tile
// table; the keys form has the padded form's grid, reads count[b] and looks
// key slot j up in index[b, j]. From `q0`, `L` (keys), `QL` (queries that
// are computed), `S` (the first row index that is not stored) and the two
// base pointers on, the body is one.
template <typename T, int FORM>
__global__ __launch_bounds__(kAtThreads)
void attention_kernel(const AttnParams p) {
  constexpr bool PACKED = FORM == kAtPacked;
  constexpr bool KEYS = FORM == kAtKeys;
  using E = typename T::E;
  using V8 = typename T::V8;
  using V4 = typename T::V4;
  __shared__ uint4 lds[2 * kAtBufBytes / 16];
  char* const smem = reinterpret_cast<char*>(lds);

  const int tid = int(threadIdx.x);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;

  const uint32_t wg = blockIdx.x;
  const int H = p.heads * kAtD;
  const int64_t row3 = int64_t(3) * H;          // elements per qkv row
  int head, L, S, q0;
  int64_t first;                                // row of the sequence's s = 0
  float scale_log2e = p.scale_log2e;
  const int32_t* index = nullptr;               // keys form: slot -> key row
  if constexpr (PACKED) {
    head = int(wg % uint32_t(p.heads));
    // one 16-byte scalar read; the clamps make any table harmless
    const int4 e =
        reinterpret_cast<const int4*>(p.tiles)[wg / uint32_t(p.heads)];
    const int total = p.S;                      // T, the packed row count
    const int row0 = e.x < 0 ? 0 : (e.x > total ? total : e.x);
    L = e.y < 0 ? 0 : (e.y > total - row0 ? total - row0 : e.y);
    q0 = e.z < 0 ? 0 : e.z;
    if (q0 >= L) return;                        // nothing of this entry exists
    S = L;                  // no padded rows: nothing at or past L is stored
    first = row0;
  } else {
    const int qt = int(wg % uint32_t(p.qtiles));
    const uint32_t bh = wg / uint32_t(p.qtiles);
    head = int(bh % uint32_t(p.heads));
    const int64_t b = int64_t(bh / uint32_t(p.heads));
    S = p.S;
    L = p.lengths ? p.lengths[b] : S;
    L = L < 0 ? 0 : (L > S ? S : L);
    q0 = qt * kAtBM;
    first = b * S;
    if constexpr (KEYS) {
      L = p.count[b];
      L = L < 0 ? 0 : (L > S ? S : L);
      index = p.index + b * S;
      if (L == 0) {
        // nothing kept: what the additive finfo.min mask gives, the uniform
        // softmax over all S keys (every score is 0, the index the identity)
        L = S;
        scale_log2e = 0.f;
        index = nullptr;
      }
    }
  }
  // the keys form computes and stores every query row; the others stop at L
  const int QL = KEYS ? S : L;

  const E* const qkv = static_cast<const E*>(p.qkv) + first * row3 +
                       head * kAtD;
  E* const out = static_cast<E*>(p.out) + first * H + head * kAtD;

  if (FORM == kAtPadded && q0 >= L) {
    // the whole tile is padding: 64 rows x 128 bytes of zeros, rows < S only
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int s = q0 + (tid >> 3) + 32 * i;
      if (s < S)
        *reinterpret_cast<uint4*>(out + int64_t(s) * H + (tid & 7) * 8) =
            make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }

  // Q fragment of query qs: d = 32 * slab + 8g .. + 7
  const int qs = q0 + wave * 16 + r;
  union Frag { uint4 u; V8 f; };
  Frag qf[2];
  qf[0].u = qf[1].u = make_uint4(0u, 0u, 0u, 0u);
  if (qs < QL) {
    const E* src = qkv + int64_t(qs) * row3 + g * 8;
    qf[0].u = *reinterpret_cast<const uint4*>(src);
    qf[1].u = *reinterpret_cast<const uint4*>(src + 32);
  }
  const bool live = q0 + wave * 16 < QL;        // wave-uniform

  // staging roles. K: row (tid / 8) + 32 i, 16-byte chunk tid % 8.
  // V: key pair lane % 32 (keys 2kp, 2kp + 1), d chunk 2 * wave + lane / 32.
  const int k_key = tid >> 3, k_chunk = tid & 7;
  const int v_key = 2 * (lane & 31), v_chunk = 2 * wave + (lane >> 5);
  // column of key v_key in the permuted V^T tile (see the header)
  const int v_col = (v_key & 32) + 8 * ((v_key >> 2) & 3) +
                    4 * ((v_key >> 4) & 1) + (v_key & 3);
  uint4 kr[2], vr[2];
  // rows of the thread's two K and two V slots of one tile. Padded and
  // packed: the slot itself. Keys: index[slot], clamped to 0..S-1, fetched
  // one tile ahead of the rows (see "Keys form" in the header); slots at or
  // past L are not looked up and not loaded.
  int krow[2], vrow[2];
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int kj = t * kAtBN + k_key + 32 * i;
      const int vj = t * kAtBN + v_key + i;
      krow[i] = kj;
      vrow[i] = vj;
      if constexpr (KEYS) {
        if (index != nullptr) {                 // workgroup-uniform
          const int a = kj < L ? index[kj] : 0;
          const int c = vj < L ? index[vj] : 0;
          krow[i] = a < 0 ? 0 : (a >= S ? S - 1 : a);
          vrow[i] = c < 0 ? 0 : (c >= S ? S - 1 : c);
        }
      }
    }
  };
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int kj = t * kAtBN + k_key + 32 * i;
      kr[i] = make_uint4(0u, 0u, 0u, 0u);
      if (kj < L)
        kr[i] = *reinterpret_cast<const uint4*>(
            qkv + int64_t(krow[i]) * row3 + H + k_chunk * 8);
      const int vj = t * kAtBN + v_key + i;
      vr[i] = make_uint4(0u, 0u, 0u, 0u);
      if (vj < L)
        vr[i] = *reinterpret_cast<const uint4*>(
            qkv + int64_t(vrow[i]) * row3 + 2 * H + v_chunk * 8);
    }
  };
  auto store = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<uint4*>(buf + (k_key + 32 * i) * kAtStride +
                                k_chunk * 16) = kr[i];
    char* vt = buf + kAtTileBytes + (8 * v_chunk) * kAtStride + v_col * 2;
    const uint32_t a[4] = {vr[0].x, vr[0].y, vr[0].z, vr[0].w};
    const uint32_t c[4] = {vr[1].x, vr[1].y, vr[1].z, vr[1].w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      // low half: key 2kp, high half: key 2kp + 1
      *reinterpret_cast<uint32_t*>(vt + (2 * w) * kAtStride) =
          (a[w] & 0xffffu) | (c[w] << 16);
      *reinterpret_cast<uint32_t*>(vt + (2 * w + 1) * kAtStride) =
          (a[w] >> 16) | (c[w] & 0xffff0000u);
    }
  };

  at_f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = at_f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -std::numeric_limits<float>::infinity();
  float l = 0.f;

  const int ntiles = (L + kAtBN - 1) / kAtBN;
  fetch(0);
  load(0);
  fetch(1);
  for (int t = 0; t < ntiles; ++t) {
    char* const buf = smem + (t & 1) * kAtBufBytes;
    store(buf);
    __syncthreads();
    if (t + 1 < ntiles) {
      load(t + 1);      // its rows were looked up a whole tile ago
      fetch(t + 2);
    }
    if (!live) continue;

    // S^T: lane (r, g) gets query r against keys k0 + 16 kb + 4g + i
    at_f32x4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s[kb] = at_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int slab = 0; slab < 2; ++slab) {
        const V8 kf = *reinterpret_cast<const V8*>(
            buf + (kb * 16 + r) * kAtStride + slab * 64 + g * 16);
        s[kb] = T::mfma(kf, qf[slab].f, s[kb]);
      }
    }
    const int k0 = t * kAtBN;
    const bool partial = k0 + kAtBN > L;        // uniform: the last tile only
    float mx = -std::numeric_limits<float>::infinity();
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x = s[kb][i] * scale_log2e;
        if (partial && k0 + kb * 16 + g * 4 + i >= L)
          x = -std::numeric_limits<float>::infinity();
        s[kb][i] = x;
        mx = fmaxf(mx, x);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // key k0 is kept (k0 < L), so mx and m_new are not -inf
    const float m_new = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);   // first tile: 0
    m = m_new;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float e = __builtin_amdgcn_exp2f(s[kb][i] - m_new);
        if (partial && k0 + kb * 16 + g * 4 + i >= L) e = 0.f;
        s[kb][i] = e;
        psum += e;
      }
    l = l * alpha + psum;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[db][i] *= alpha;

    // O^T += V^T P^T over the two 32-key slabs
    const char* const vt = buf + kAtTileBytes;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 pf;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        pf[i] = static_cast<E>(s[2 * ks][i]);
        pf[4 + i] = static_cast<E>(s[2 * ks + 1][i]);
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const V8 vf = *reinterpret_cast<const V8*>(
            vt + (db * 16 + r) * kAtStride + ks * 64 + g * 16);
        o[db] = T::mfma(vf, pf, o[db]);
      }
    }
  }

  // the four lanes of a query add the same two numbers at every step
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qs < S) {
    E* dst = out + int64_t(qs) * H + g * 4;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      V4 y;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        y[i] = qs < QL ? static_cast<E>(__fdiv_rn(o[db][i], l))
                       : static_cast<E>(0.f);
      *reinterpret_cast<V4*>(dst + db * 16) = y;
    }
  }
}

// Key-index kernel of the keys form: one wave per sequence compacts the kept
// positions of mask[b, :] (non-zero keeps) into index[b, :count[b]],
// ascending. 64 positions per step: the ballot of the step's keep bits, the
// popcount of the lower lanes gives a kept lane its slot after the running
// base, which is wave-uniform and stays in an SGPR. Slots at and past
// count[b] are not written. Every slot is written by one lane: deterministic.
template <typename M>
__global__ __launch_bounds__(64)
void attention_keys_kernel(const M* __restrict__ mask,
                           int32_t* __restrict__ index,
                           int32_t* __restrict__ count, int S) {
  const int lane = int(threadIdx.x);
  const int64_t row = int64_t(blockIdx.x) * S;
  const M* const m = mask + row;
  int32_t* const dst = index + row;
  int base = 0;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    const bool keep = s < S && m[s] != M(0);
    const uint64_t bits = __ballot(keep);
    const int below = int(__builtin_amdgcn_mbcnt_hi(
        uint32_t(bits >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bits), 0u)));
    if (keep) dst[base + below] = s;
    base += __popcll(bits);
  }
  if (lane == 0) count[blockIdx.x] = base;
}

}  // namespace

// The key table of the keys form, see attention_keys_kernel: `mask` is a
// contiguous device [B,S] of int32, uint8 or bool; returns (index int32
// [B,S], count int32 [B]). One launch, no host synchronization.
std::tuple<at::Tensor, at::Tensor> attention_keys(const at::Tensor& mask) {
  const char* who = "attention_keys";
  const at::ScalarType md = mask.scalar_type();
  TORCH_CHECK_VALUE(mask.is_cuda() && mask.dim() == 2 && mask.is_contiguous(),
                    who, " expects a contiguous device [B,S] mask");
  TORCH_CHECK_VALUE(md == at::kInt || md == at::kByte || md == at::kBool, who,
                    ": mask must be int32, uint8 or bool, got ", md);
  const int64_t B = mask.size(0), S = mask.size(1);
  TORCH_CHECK_VALUE(S < (int64_t(1) << 30) && B < (int64_t(1) << 31), who,
                    ": S must be below 2^30 and B below 2^31, got B=", B,
                    " S=", S);
  auto index = at::empty({B, S}, mask.options().dtype(at::kInt));
  auto count = at::empty({B}, mask.options().dtype(at::kInt));
  if (B == 0) return {index, count};            // zero grid: never launch
  const dim3 grid{uint32_t(B)}, block(64);
  hipStream_t stream = at::hip::getCurrentHIPStream().stream();
  int32_t* const ip = static_cast<int32_t*>(index.mutable_data_ptr());
  int32_t* const cp = static_cast<int32_t*>(count.mutable_data_ptr());
  if (md == at::kInt)
    hipLaunchKernelGGL(attention_keys_kernel<int32_t>, grid, block, 0, stream,
                       static_cast<const int32_t*>(mask.const_data_ptr()), ip,
                       cp, int(S));
  else
    hipLaunchKernelGGL(attention_keys_kernel<uint8_t>, grid, block, 0, stream,
                       static_cast<const uint8_t*>(mask.const_data_ptr()), ip,
                       cp, int(S));
  hipError_t err = hipGetLastError();
  if (err != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(err) + " at " + who);
  return {index, count};
}

// Length-masked self-attention, see the header of this file. Padded form:
// `qkv` is [B,S,3*heads*64] bf16 or f16, `lengths` int32 [B] on its device or
// absent (every sequence is S long); returns [B,S,heads*64] of qkv's dtype.
// The lengths are clamped to 0..S on the device and never read back. Packed
// form: `qkv` is [T,3*heads*64], `tiles` the int32 [n,4] device table of
// (row0, L, q0, seq) rows and `lengths` is absent; returns [T,heads*64],
// whose rows outside every entry are unspecified. The entries are clamped on
// the device and never read back. Keys form: `qkv` is [B,S,3*H], `index`
// int32 [B,S] and `count` int32 [B] come from attention_keys, `lengths` and
// `tiles` are absent; every row of the [B,S,H] result is computed. Counts
// and indices are clamped on the device and never read back. Arguments the
// kernel cannot serve are ValueError.
at::Tensor masked_self_attention(const at::Tensor& qkv,
                                 const c10::optional<at::Tensor>& lengths,
                                 int64_t heads, double scale,
                                 const c10::optional<at::Tensor>& tiles,
                                 const c10::optional<at::Tensor>& index,
                                 const c10::optional<at::Tensor>& count) {
  const char* who = "masked_self_attention";
  const at::ScalarType dt = qkv.scalar_type();
  TORCH_CHECK_VALUE(dt == at::kBFloat16 || dt == at::kHalf, who,
                    " expects bfloat16 or float16 qkv, got ", dt);
  TORCH_CHECK_VALUE(qkv.is_cuda() && (qkv.dim() == 3 || qkv.dim() == 2) &&
                    qkv.is_contiguous(), who,
                    " expects a contiguous device [B,S,3*H] or [T,3*H] "
                    "tensor");
  const bool packed = qkv.dim() == 2;
  // packed: one "batch" of T rows
  const int64_t B = packed ? 1 : qkv.size(0), S = qkv.size(-2),
                H3 = qkv.size(-1);
  TORCH_CHECK_VALUE(heads >= 1 && H3 % (3 * heads) == 0, who,
                    ": the last axis (", H3, ") must be 3 * heads (", heads,
                    ") * head_dim");
  TORCH_CHECK_VALUE(H3 / (3 * heads) == kAtD, who, ": head_dim must be ",
                    kAtD, ", got ", H3 / (3 * heads));
  TORCH_CHECK_VALUE(std::isfinite(scale), who, ": scale must be finite");
  const int64_t H = H3 / 3;
  TORCH_CHECK_VALUE(packed == tiles.has_value() &&
                    !(packed && lengths.has_value()), who,
                    ": a [T,3*H] qkv takes tiles and no lengths, a [B,S,3*H] "
                    "qkv takes no tiles");
  if (lengths.has_value())
    TORCH_CHECK_VALUE(lengths->is_cuda() &&
                      lengths->get_device() == qkv.get_device() &&
                      lengths->scalar_type() == at::kInt &&
                      lengths->dim() == 1 && lengths->size(0) == B &&
                      lengths->is_contiguous(), who,
                      ": lengths must be a contiguous int32 [", B,
                      "] on qkv's device");
  const bool keys = index.has_value();
  TORCH_CHECK_VALUE(keys == count.has_value() &&
                    !(keys && (packed || lengths.has_value())), who,
                    ": index and count go together, with a [B,S,3*H] qkv and "
                    "no lengths");
  if (keys)
    for (const at::Tensor* t : {&*index, &*count})
      TORCH_CHECK_VALUE(t->is_cuda() &&
                        t->get_device() == qkv.get_device() &&
                        t->scalar_type() == at::kInt && t->is_contiguous() &&
                        t->dim() == (t == &*index ? 2 : 1) &&
                        t->size(0) == B && (t != &*index || t->size(1) == S),
                        who, ": keys must be contiguous int32 [", B, ",", S,
                        "] and [", B, "] on qkv's device");
  int64_t ntiles = 0;
  if (packed) {
    TORCH_CHECK_VALUE(tiles->is_cuda() &&
                      tiles->get_device() == qkv.get_device() &&
                      tiles->scalar_type() == at::kInt && tiles->dim() == 2 &&
                      tiles->size(1) == 4 && tiles->is_contiguous(), who,
                      ": tiles must be a contiguous int32 [n,4] on qkv's "
                      "device");
    ntiles = tiles->size(0);
  }
  auto out = packed ? at::empty({S, H}, qkv.options())
                    : at::empty({B, S, H}, qkv.options());
  if (B == 0 || S == 0 || (packed && ntiles == 0)) return out;
  TORCH_CHECK_VALUE(
      reinterpret_cast<uintptr_t>(qkv.const_data_ptr()) % 16 == 0, who,
      ": qkv must be 16-byte aligned");
  const int64_t qtiles = (S + kAtBM - 1) / kAtBM;
  // a launch holds fewer than 2^32 threads: 2^24 workgroups of 256
  int64_t groups;
  if (packed) {
    TORCH_CHECK_VALUE(
        reinterpret_cast<uintptr_t>(tiles->const_data_ptr()) % 16 == 0, who,
        ": tiles must be 16-byte aligned");
    TORCH_CHECK_VALUE(S < (int64_t(1) << 30) &&
                      ntiles < (int64_t(1) << 24) &&
                      ntiles * heads < (int64_t(1) << 24), who,
                      ": T must be below 2^30 and n * heads below 2^24, got "
                      "T=", S, " n=", ntiles, " heads=", heads);
    groups = ntiles * heads;
  } else {
    TORCH_CHECK_VALUE(S < (int64_t(1) << 30) &&
                      B * heads < (int64_t(1) << 24) &&
                      B * heads * qtiles < (int64_t(1) << 24), who,
                      ": B * heads * ceil(S/64) must be below 2^24, got B=",
                      B, " heads=", heads, " S=", S);
    groups = B * heads * qtiles;
  }

  AttnParams p;
  p.qkv = qkv.const_data_ptr();
  p.lengths = lengths.has_value()
                  ? static_cast<const int32_t*>(lengths->const_data_ptr())
                  : nullptr;
  p.tiles = packed ? static_cast<const int32_t*>(tiles->const_data_ptr())
                   : nullptr;
  p.index = keys ? static_cast<const int32_t*>(index->const_data_ptr())
                 : nullptr;
  p.count = keys ? static_cast<const int32_t*>(count->const_data_ptr())
                 : nullptr;
  p.out = out.mutable_data_ptr();
  p.S = int(S);
  p.heads = int(heads);
  p.qtiles = int(qtiles);
  p.scale_log2e = float(scale * 1.4426950408889634);

  const dim3 grid{uint32_t(groups)}, block(kAtThreads);
  hipStream_t stream = at::hip::getCurrentHIPStream().stream();
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    if (packed)
      hipLaunchKernelGGL((attention_kernel<T, kAtPacked>), grid, block, 0,
                         stream, p);
    else if (keys)
      hipLaunchKernelGGL((attention_kernel<T, kAtKeys>), grid, block, 0,
                         stream, p);
    else
      hipLaunchKernelGGL((attention_kernel<T, kAtPadded>), grid, block, 0,
                         stream, p);
  };
  if (dt == at::kBFloat16) launch(AtBf16{});
  else launch(AtF16{});
  hipError_t err = hipGetLastError();
  if (err != hipSuccess)
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(err) + " at " + who);
  return out;
}

}  // namespace mi355x
