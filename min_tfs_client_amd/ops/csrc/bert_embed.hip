// Fused BERT embedding ingest for gfx950 (CDNA4, wave64): token ids in,
// LayerNorm'd encoder input and additive attention mask out, one launch.
//
//   x[b,s,:]   = float(tok[id]) + float(pos[s]) + float(typ[t])     (fp32)
//   mean       = sum_h x / H
//   var        = sum_h (x - mean)^2 / H             (biased, two passes)
//   hidden     = OUT(((x - mean) * rstd) * gamma + beta)
//   rstd       = 1 / sqrt(var + eps): an IEEE square root (`sqrtf`, hipcc's
//                default -fhip-fp32-correctly-rounded-divide-sqrt) and an
//                IEEE divide (`__fdiv_rn`), no rsqrt approximation
//   mask[b,s]  = kept ? +0.0 : finfo(OUT).min                  [B,1,1,S]
//
// Every product and sum above is one unfused fp32 operation (the file is built
// with -ffp-contract=off) and there is ONE rounding to the output dtype, at
// the store.
//
// Work split. One wavefront owns one token row (b,s); a workgroup is 4 waves
// and the grid is persistent: at most kBeMaxGroups workgroups, wave w of
// group g takes rows g*4+w, g*4+w + 4*grid, ... The wave index goes through
// readfirstlane, so the row, its id, its type and its table bases are scalar.
// gamma and beta are loaded once per wave, before the row loop, and stay in
// registers as the 16-byte words they were loaded as.
//
// Data movement. H is cut into chunks of VEC = 16 bytes / sizeof(table
// element) values (4 for f32 tables, 8 for bf16 / f16). Lane l owns chunks
// l, l+64, ...; CPL = ceil(H/VEC/64) of them, a template parameter (1, 2, 4,
// 8 or 16: H <= 4096), so the loop is unrolled and the row lives in CPL*VEC
// fp32 registers from the loads through both statistics passes to the store.
// A chunk index past H/VEC is skipped by a guard, which covers H/VEC not a
// multiple of 64 and H/VEC < 64 alike. Each table byte is read once per row,
// with 16-byte loads; stores are 16 bytes per VEC/4 or VEC/8 values. No LDS,
// no atomics on the data path.
//
// Statistics. Each lane adds its values in chunk order, the wave adds the 64
// partials with an xor butterfly (__shfl_xor 32, 16, 8, 4, 2, 1). Both
// operands of every butterfly add are the same two numbers in every lane
// pair, so all lanes hold the same bits and the result does not depend on
// the grid: the kernel is bit-deterministic, a row's bits depend on its id,
// position and type only, and the ragged form equals the dense form.
//
// Validation. An id outside [0, vocab) or a type outside [0, type_vocab)
// never indexes a table: the row reads index 0 and lane 0 sends
// row*2 + (0: id, 1: type) through a global atomicMin to an int32 slot that
// holds INT32_MAX when the batch is clean. The host reads the slot after the
// launch (one 4-byte D2H copy) and hands the lowest bad row to the caller;
// a slot that reported is reset before it is used again.
//
// Ragged form: the same body. `table` holds (offset, length) per sequence and
// row (b,s) takes ids[offset+s] (and types[offset+s]) when s < length, else
// pad_id (type 0); "kept" is s < length. Dense form: "kept" is mask != 0.
//
// Packed output (ragged form only): a row with s >= length is skipped before
// any load, a kept row is stored at row offset + s of a [total,H] tensor, and
// there is no mask. The skip is per wave (the row is scalar), the arithmetic
// of a kept row is untouched, so the result is the kept rows of the padded
// output bit for bit. The error code stays row * 2 + kind in (b, s) space.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage), scratch is 0 bytes/lane in every
// of the 78 instantiations and none uses LDS (int32 ids; int64 ids differ by
// at most 4 registers). The build does not pass that flag: to refresh the
// table, compile this file alone with the build's flags plus
// `--cuda-device-only -Rpass-analysis=kernel-resource-usage`.
//   tables  out   CPL  H up to   VGPRs  SGPRs  occupancy (waves/SIMD)
//   f32     f32     1      256      44     84     8
//   bf16    bf16    1      512      60     92     8
//   bf16    bf16    2     1024      80    104     6    (BERT-base: H = 768)
//   f32     f32     4     1024      78    104     6    (BERT-base: H = 768)
//   bf16    bf16    8     4096     233    106     2
//   f32     f32    16     4096     237    106     2
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cstdint>
#include <limits>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

namespace mi355x {
namespace {

constexpr int kBeWaves = 4;                 // waves per workgroup
constexpr int kBeThreads = kBeWaves * 64;
constexpr int kBeMaxGroups = 2048;          // persistent grid cap
constexpr int kBeMaxH = 4096;
constexpr int kBeClean = std::numeric_limits<int32_t>::max();

struct BertEmbedParams {
  const void* ids;          // ID [B,S], ragged: [total]
  const void* types;        // ID, same layout as ids, or null (all zero)
  const int32_t* table;     // ragged: (offset, length) per sequence, else null
  const void* mask;         // dense: [B,S] of mask_bytes-wide integers, or null
  const void* tok;          // [vocab, H]
  const void* pos;          // [>= S, H]
  const void* typ;          // [type_vocab, H]
  const void* gamma;        // [H]
  const void* beta;         // [H]
  void* out;                // OUT [B,S,H], packed: [total,H]
  void* mask_out;           // OUT [B,S] or null
  int32_t* err;             // error slot or null (no report)
  int64_t pad_id;
  int rows, S, H, vocab, type_vocab, mask_bytes;
  int packed;               // ragged only: store kept rows at offset + s
  float eps;
};

struct BeF32 {
  using T = float;
  static constexpr int kVec = 4;
  static __device__ __forceinline__ void unpack(const uint4& w, float* v) {
    v[0] = __uint_as_float(w.x); v[1] = __uint_as_float(w.y);
    v[2] = __uint_as_float(w.z); v[3] = __uint_as_float(w.w);
  }
  static __device__ __forceinline__ float to(float f) { return f; }
  static __device__ __forceinline__ float lowest() {
    return -std::numeric_limits<float>::max();
  }
};

struct BeBf16 {
  using T = uint16_t;
  static constexpr int kVec = 8;
  static __device__ __forceinline__ void unpack(const uint4& w, float* v) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(u[i] << 16);
      v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ uint16_t to(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u)          // NaN: quiet, keep sign
      return uint16_t((u >> 16) | 0x0040u);
    return uint16_t((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);   // nearest even
  }
  static __device__ __forceinline__ uint16_t lowest() { return 0xff7fu; }
};

struct BeF16 {
  using T = uint16_t;
  static constexpr int kVec = 8;
  static __device__ __forceinline__ float half_bits(uint32_t h) {
    __half_raw r; r.x = uint16_t(h);
    return __half2float(__half(r));
  }
  static __device__ __forceinline__ void unpack(const uint4& w, float* v) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = half_bits(u[i] & 0xffffu);
      v[2 * i + 1] = half_bits(u[i] >> 16);
    }
  }
  static __device__ __forceinline__ uint16_t to(float f) {
    __half_raw r(__float2half(f));                // round to nearest even
    return r.x;
  }
  static __device__ __forceinline__ uint16_t lowest() { return 0xfbffu; }
};

__device__ __forceinline__ float be_wave_sum(float v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  return v;
}

// N values of one chunk to `dst` (OUT elements), in 16-byte stores where the
// chunk has that many bytes (8 for 4 values of a 16-bit type)
template <typename OUT, int N>
__device__ __forceinline__ void be_store(typename OUT::T* dst, const float* y) {
  if constexpr (sizeof(typename OUT::T) == 4) {
#pragma unroll
    for (int i = 0; i < N; i += 4)
      *reinterpret_cast<float4*>(dst + i) =
          make_float4(y[i], y[i + 1], y[i + 2], y[i + 3]);
  } else {
    uint32_t w[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i)
      w[i] = uint32_t(OUT::to(y[2 * i])) |
             (uint32_t(OUT::to(y[2 * i + 1])) << 16);
    if constexpr (N == 8)
      *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    else
      *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
  }
}

template <typename TAB, typename OUT, typename ID, int CPL>
__global__ __launch_bounds__(kBeThreads)
void bert_embed_kernel(const BertEmbedParams p) {
  constexpr int VEC = TAB::kVec;
  using TabT = typename TAB::T;
  using OutT = typename OUT::T;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int chunks = p.H / VEC;
  const float fH = float(p.H);

  uint4 g[CPL], bt[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      g[i] = *reinterpret_cast<const uint4*>(
          static_cast<const TabT*>(p.gamma) + c * VEC);
      bt[i] = *reinterpret_cast<const uint4*>(
          static_cast<const TabT*>(p.beta) + c * VEC);
    }
  }

  const ID* ids = static_cast<const ID*>(p.ids);
  const ID* types = static_cast<const ID*>(p.types);
  const int step = int(gridDim.x) * kBeWaves;          // rows < 2^30
  for (int row = int(blockIdx.x) * kBeWaves + wave; row < p.rows;
       row += step) {
    const int b = row / p.S, s = row - b * p.S;
    int64_t id, t = 0;
    int64_t out_row = row;
    bool keep = true;
    if (p.table) {
      const int off = p.table[2 * b], len = p.table[2 * b + 1];
      keep = s < len;
      if (p.packed) {
        if (!keep) continue;                    // wave-uniform
        out_row = off + s;
      }
      id = keep ? int64_t(ids[off + s]) : p.pad_id;
      if (keep && types) t = int64_t(types[off + s]);
    } else {
      id = int64_t(ids[row]);
      if (types) t = int64_t(types[row]);
      if (p.mask_bytes == 4)
        keep = static_cast<const int32_t*>(p.mask)[row] != 0;
      else if (p.mask_bytes == 8)
        keep = static_cast<const int64_t*>(p.mask)[row] != 0;
      else if (p.mask_bytes == 1)
        keep = static_cast<const uint8_t*>(p.mask)[row] != 0;
    }
    const bool bad_id = id < 0 || id >= p.vocab;
    const bool bad_t = t < 0 || t >= p.type_vocab;
    if (bad_id || bad_t) {
      if (lane == 0 && p.err) atomicMin(p.err, row * 2 + (bad_id ? 0 : 1));
      if (bad_id) id = 0;
      if (bad_t) t = 0;
    }
    const TabT* tok = static_cast<const TabT*>(p.tok) + id * p.H;
    const TabT* pos = static_cast<const TabT*>(p.pos) + int64_t(s) * p.H;
    const TabT* typ = static_cast<const TabT*>(p.typ) + t * p.H;

    float x[CPL][VEC];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + 64 * i;
      if (c < chunks) {
        const uint4 wt = *reinterpret_cast<const uint4*>(tok + c * VEC);
        const uint4 wp = *reinterpret_cast<const uint4*>(pos + c * VEC);
        const uint4 wy = *reinterpret_cast<const uint4*>(typ + c * VEC);
        float a[VEC], q[VEC], y[VEC];
        TAB::unpack(wt, a); TAB::unpack(wp, q); TAB::unpack(wy, y);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          x[i][v] = (a[v] + q[v]) + y[v];
          sum += x[i][v];
        }
      }
    }
    const float mean = __fdiv_rn(be_wave_sum(sum), fH);
    float ssd = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      if (lane + 64 * i < chunks) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          x[i][v] -= mean;
          ssd += x[i][v] * x[i][v];
        }
      }
    }
    const float var = __fdiv_rn(be_wave_sum(ssd), fH);
    const float rstd = __fdiv_rn(1.0f, sqrtf(var + p.eps));

    OutT* out = static_cast<OutT*>(p.out) + out_row * p.H;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + 64 * i;
      if (c < chunks) {
        float gv[VEC], bv[VEC], y[VEC];
        TAB::unpack(g[i], gv); TAB::unpack(bt[i], bv);
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          y[v] = (x[i][v] * rstd) * gv[v] + bv[v];
        be_store<OUT, VEC>(out + c * VEC, y);
      }
    }
    if (lane == 0 && p.mask_out)
      static_cast<OutT*>(p.mask_out)[row] = keep ? OutT(0) : OUT::lowest();
  }
}

template <typename TAB, typename OUT, typename ID>
void launch_bert_embed_cpl(const BertEmbedParams& p, int groups,
                           hipStream_t stream) {
  const int cpl = (p.H / TAB::kVec + 63) / 64;
  const dim3 grid(groups), block(kBeThreads);
  if (cpl <= 1)
    hipLaunchKernelGGL((bert_embed_kernel<TAB, OUT, ID, 1>), grid, block, 0,
                       stream, p);
  else if (cpl <= 2)
    hipLaunchKernelGGL((bert_embed_kernel<TAB, OUT, ID, 2>), grid, block, 0,
                       stream, p);
  else if (cpl <= 4)
    hipLaunchKernelGGL((bert_embed_kernel<TAB, OUT, ID, 4>), grid, block, 0,
                       stream, p);
  else if (cpl <= 8 || TAB::kVec == 8)      // 16-bit tables: H/8/64 <= 8
    hipLaunchKernelGGL((bert_embed_kernel<TAB, OUT, ID, 8>), grid, block, 0,
                       stream, p);
  else if constexpr (TAB::kVec == 4)
    hipLaunchKernelGGL((bert_embed_kernel<TAB, OUT, ID, 16>), grid, block, 0,
                       stream, p);
}

template <typename TAB, typename OUT>
void launch_bert_embed_id(bool id64, const BertEmbedParams& p, int groups,
                          hipStream_t stream) {
  if (id64)
    launch_bert_embed_cpl<TAB, OUT, int64_t>(p, groups, stream);
  else
    launch_bert_embed_cpl<TAB, OUT, int32_t>(p, groups, stream);
}

template <typename TAB>
void launch_bert_embed_out(at::ScalarType out_dtype, bool id64,
                           const BertEmbedParams& p, int groups,
                           hipStream_t stream) {
  if (out_dtype == at::kFloat)
    launch_bert_embed_id<TAB, BeF32>(id64, p, groups, stream);
  else if (out_dtype == at::kBFloat16)
    launch_bert_embed_id<TAB, BeBf16>(id64, p, groups, stream);
  else
    launch_bert_embed_id<TAB, BeF16>(id64, p, groups, stream);
}

// Error slots: one int32 per call in flight, INT32_MAX while clean. A call
// owns its slot from the launch to the D2H read, then hands it back; a slot
// that reported is refilled first. The list is never destroyed (device
// memory must not be freed after the runtime has gone).
struct BeSlots {
  std::mutex mu;
  std::vector<std::vector<at::Tensor>> free_list;   // per device
};

BeSlots& be_slots() {
  static BeSlots* s = new BeSlots;
  return *s;
}

at::Tensor be_take_slot(const at::Tensor& like) {
  BeSlots& s = be_slots();
  const size_t dev = size_t(like.get_device());
  {
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.free_list.size() <= dev) s.free_list.resize(dev + 1);
    auto& fl = s.free_list[dev];
    if (!fl.empty()) {
      at::Tensor t = fl.back();
      fl.pop_back();
      return t;
    }
  }
  return at::full({1}, kBeClean, like.options().dtype(at::kInt));
}

void be_give_slot(const at::Tensor& slot) {
  BeSlots& s = be_slots();
  std::lock_guard<std::mutex> lock(s.mu);
  s.free_list[size_t(slot.get_device())].push_back(slot);
}

}  // namespace

// Fused BERT embedding, see the header of this file. Dense form: `ids` is
// [B,S] and `table` is absent; ragged form: `ids` is [total], `table` is the
// device int32 [B,2] of (offset, length) rows that the caller checked against
// `total` and `S`. Returns (hidden [B,S,H], additive mask [B,1,1,S] or an
// undefined tensor, error code): the code is -1 for a clean batch, else
// row*2 + (0: id, 1: type) of the lowest bad row; `check=false` skips the
// report and the D2H read (the kernel still never indexes with a bad value).
// `packed` (ragged form only): hidden is [total,H], the kept rows back to
// back, and there is no mask; the caller checked that the table's rows tile
// 0..total. Arguments the kernel cannot serve are ValueError.
std::tuple<at::Tensor, c10::optional<at::Tensor>, int64_t> bert_embed(
    const at::Tensor& ids, const c10::optional<at::Tensor>& table, int64_t B,
    int64_t S, const c10::optional<at::Tensor>& mask,
    const c10::optional<at::Tensor>& types, const at::Tensor& tok,
    const at::Tensor& pos, const at::Tensor& typ, const at::Tensor& gamma,
    const at::Tensor& beta, double eps, int64_t pad_id,
    at::ScalarType out_dtype, bool check, bool packed) {
  const char* who = "bert_embed";
  const bool ragged = table.has_value();
  TORCH_CHECK_VALUE(ragged || !packed, who,
                    ": packed output needs the ragged form");
  TORCH_CHECK_VALUE(out_dtype == at::kFloat || out_dtype == at::kBFloat16 ||
                    out_dtype == at::kHalf,
                    who, ": out_dtype must be f32, bf16 or f16");
  TORCH_CHECK_VALUE(ids.is_cuda() && ids.is_contiguous() &&
                    (ids.scalar_type() == at::kInt ||
                     ids.scalar_type() == at::kLong),
                    who, " expects contiguous int32 or int64 device ids");
  auto on_device = [&](const at::Tensor& t) {
    return t.is_cuda() && t.get_device() == ids.get_device() &&
           t.is_contiguous();
  };
  const at::ScalarType tab = tok.scalar_type();
  TORCH_CHECK_VALUE(tab == at::kFloat || tab == at::kBFloat16 ||
                    tab == at::kHalf, who,
                    ": tables must be f32, bf16 or f16");
  TORCH_CHECK_VALUE(on_device(tok) && tok.dim() == 2 && tok.size(0) >= 1,
                    who, ": tok must be a contiguous device [vocab,H]");
  const int64_t H = tok.size(1);
  TORCH_CHECK_VALUE(H % 8 == 0 && H >= 8 && H <= kBeMaxH, who,
                    ": H must be a multiple of 8 in 8..", kBeMaxH, ", got ",
                    H);
  for (const at::Tensor* t : {&pos, &typ})
    TORCH_CHECK_VALUE(on_device(*t) && t->scalar_type() == tab &&
                      t->dim() == 2 && t->size(1) == H && t->size(0) >= 1,
                      who, ": pos and typ must be contiguous device [n,", H,
                      "] tables of tok's dtype");
  for (const at::Tensor* t : {&gamma, &beta})
    TORCH_CHECK_VALUE(on_device(*t) && t->scalar_type() == tab &&
                      t->dim() == 1 && t->size(0) == H, who,
                      ": gamma and beta must be contiguous device [", H,
                      "] of tok's dtype");
  for (const at::Tensor* t : {&tok, &pos, &typ, &gamma, &beta})
    TORCH_CHECK_VALUE(
        reinterpret_cast<uintptr_t>(t->const_data_ptr()) % 16 == 0, who,
        ": tables, gamma and beta must be 16-byte aligned");
  TORCH_CHECK_VALUE(B >= 1 && S >= 1 && S <= pos.size(0) &&
                    B * S < (int64_t(1) << 30), who,
                    ": need 1 <= S <= max_pos and 1 <= B*S < 2^30, got B=", B,
                    " S=", S, " max_pos=", pos.size(0));
  TORCH_CHECK_VALUE(tok.size(0) <= std::numeric_limits<int32_t>::max() &&
                    typ.size(0) <= std::numeric_limits<int32_t>::max(), who,
                    ": too many table rows");
  TORCH_CHECK_VALUE(pad_id >= 0 && pad_id < tok.size(0), who,
                    ": pad_id ", pad_id, " is outside [0, ", tok.size(0),
                    ")");
  if (ragged) {
    TORCH_CHECK_VALUE(on_device(*table) && table->scalar_type() == at::kInt &&
                      table->dim() == 2 && table->size(0) == B &&
                      table->size(1) == 2 && ids.dim() == 1 &&
                      !mask.has_value(), who,
                      ": ragged form takes ids [total], an int32 device "
                      "table [B,2] and no mask");
  } else {
    TORCH_CHECK_VALUE(ids.dim() == 2 && ids.size(0) == B && ids.size(1) == S,
                      who, ": ids must be [B,S]");
  }
  if (types.has_value())
    TORCH_CHECK_VALUE(on_device(*types) &&
                      types->scalar_type() == ids.scalar_type() &&
                      types->sizes() == ids.sizes(), who,
                      ": types must match ids in shape, dtype and device");
  int mask_bytes = 0;
  if (mask.has_value()) {
    const at::ScalarType mt = mask->scalar_type();
    TORCH_CHECK_VALUE(on_device(*mask) && mask->dim() == 2 &&
                      mask->size(0) == B && mask->size(1) == S &&
                      (mt == at::kInt || mt == at::kLong || mt == at::kByte ||
                       mt == at::kBool), who,
                      ": mask must be a contiguous device [B,S] of int32, "
                      "int64, uint8 or bool");
    mask_bytes = int(mask->element_size());
  }

  auto out = packed
                 ? at::empty({ids.size(0), H}, tok.options().dtype(out_dtype))
                 : at::empty({B, S, H}, tok.options().dtype(out_dtype));
  c10::optional<at::Tensor> mask_out;
  if (!packed && (ragged || mask.has_value()))
    mask_out = at::empty({B, 1, 1, S}, out.options());
  at::Tensor slot;
  if (check) slot = be_take_slot(ids);

  BertEmbedParams p;
  p.ids = ids.const_data_ptr();
  p.types = types.has_value() ? types->const_data_ptr() : nullptr;
  p.table = ragged ? static_cast<const int32_t*>(table->const_data_ptr())
                   : nullptr;
  p.mask = mask.has_value() ? mask->const_data_ptr() : nullptr;
  p.tok = tok.const_data_ptr();
  p.pos = pos.const_data_ptr();
  p.typ = typ.const_data_ptr();
  p.gamma = gamma.const_data_ptr();
  p.beta = beta.const_data_ptr();
  p.out = out.mutable_data_ptr();
  p.mask_out = mask_out.has_value() ? mask_out->mutable_data_ptr() : nullptr;
  p.err = check ? static_cast<int32_t*>(slot.mutable_data_ptr()) : nullptr;
  p.pad_id = pad_id;
  p.rows = int(B * S);
  p.S = int(S);
  p.H = int(H);
  p.vocab = int(tok.size(0));
  p.type_vocab = int(typ.size(0));
  p.mask_bytes = mask_bytes;
  p.packed = packed ? 1 : 0;
  p.eps = float(eps);

  const int groups =
      int(std::min<int64_t>((B * S + kBeWaves - 1) / kBeWaves, kBeMaxGroups));
  hipStream_t stream = at::hip::getCurrentHIPStream().stream();
  const bool id64 = ids.scalar_type() == at::kLong;
  if (tab == at::kFloat)
    launch_bert_embed_out<BeF32>(out_dtype, id64, p, groups, stream);
  else if (tab == at::kBFloat16)
    launch_bert_embed_out<BeBf16>(out_dtype, id64, p, groups, stream);
  else
    launch_bert_embed_out<BeF16>(out_dtype, id64, p, groups, stream);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    if (check) be_give_slot(slot);          // the kernel did not run
    throw std::runtime_error(std::string("HIP error: ") +
                             hipGetErrorString(err) + " at " + who);
  }
  int64_t code = -1;
  if (check) {
    const int v = slot.item<int>();          // the one small D2H copy
    if (v != kBeClean) {
      code = v;
      slot.fill_(kBeClean);
      // the next owner may launch on another stream
      if (hipStreamSynchronize(stream) != hipSuccess)
        throw std::runtime_error(std::string("HIP error at ") + who);
    }
    be_give_slot(slot);
  }
  return {out, mask_out, code};
}

}  // namespace mi355x
