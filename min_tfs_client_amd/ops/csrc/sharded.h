// Sharded Predict planning: how one logical request is split along dim 0
// into `shards` ordinary PredictRequests, what each shard's wire skeleton
// and payload regions are, and which channel each shard rides.
//
// Header-only on top of wire.h — no pybind, no torch, no HIP — so the
// planning logic compiles stand-alone and runs under ASAN/UBSAN
// (tests/cpp/sharded_test.cpp). The transport (grpc_transport.cpp
// predict_sharded) only orchestrates existing sends/waits around it.
#pragma once

#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "wire.h"

namespace tfsshard {

// Host spans smaller than this are copied into the skeleton instead of
// becoming iovec regions (fewer regions beats the copy at that size).
// Shared by the streaming serializer (native.cpp) and the sharded planner:
// both must inline the same spans so the wire bytes stay identical.
constexpr size_t kStreamMinSpan = 64 * 1024;

// Fixed size of the transport's persistent sender pool (never derived from
// the CPU count: a request has a handful of shards, and more threads only
// contend on the sockets).
constexpr int kSenderPoolSize = 8;

// dim-0 rows per shard: divmod(batch, shards), the first `rem` shards get
// one extra row (the rule of TurboPredictClient.predict_sharded).
inline std::vector<int64_t> shard_sizes(int64_t batch, int shards) {
  if (shards < 1 || batch < shards)
    throw std::invalid_argument("shard_sizes: need 1 <= shards <= batch");
  const int64_t base = batch / shards;
  const int64_t rem = batch % shards;
  std::vector<int64_t> sizes(static_cast<size_t>(shards));
  for (int i = 0; i < shards; ++i)
    sizes[size_t(i)] = base + (i < rem ? 1 : 0);
  return sizes;
}

// One whole (unsharded) contiguous input tensor.
struct Input {
  int dtype = 0;                // tensorflow.DataType enum value
  std::vector<int64_t> shape;   // rank >= 1; shape[0] is the batch
  size_t elem_size = 0;
  const uint8_t* data = nullptr;  // host or device address of row 0
  bool device = false;

  uint64_t row_bytes() const {
    uint64_t n = elem_size;
    for (size_t d = 1; d < shape.size(); ++d) n *= uint64_t(shape[d]);
    return n;
  }
};

// Payload location inside a shard's message (same fields as the
// transport's WireRegion; kept separate so this header stands alone).
struct Region {
  size_t offset;
  size_t nbytes;
  uintptr_t ptr;
  bool device;
};

struct ShardPlan {
  // the full message with the region holes left UNWRITTEN (and, being
  // default-initialized storage, untouched: a multi-MB hole costs no
  // memset and no page faults)
  std::unique_ptr<uint8_t[]> skeleton;
  size_t size = 0;
  std::vector<Region> regions;  // ascending offsets
};

// Skeleton + regions of the PredictRequest carrying rows
// [row_off, row_off + rows) of every input — byte-identical to what the
// streaming serializer emits for the same narrow(0, row_off, rows) views:
// device spans and host spans >= kStreamMinSpan become regions, smaller
// host spans are copied into the skeleton, empty spans are skipped.
inline ShardPlan plan_shard(const std::string& model_name, int64_t version,
                            const std::string& signature,
                            const std::vector<std::string>& names,
                            const std::vector<Input>& inputs,
                            int64_t row_off, int64_t rows) {
  if (names.size() != inputs.size())
    throw std::invalid_argument("plan_shard: names/inputs mismatch");
  std::vector<tfswire::TensorMeta> metas(inputs.size());
  for (size_t i = 0; i < inputs.size(); ++i) {
    const Input& in = inputs[i];
    if (in.shape.empty() || row_off < 0 || rows < 0 ||
        row_off + rows > in.shape[0])
      throw std::invalid_argument("plan_shard: rows out of range for '" +
                                  names[i] + "'");
    metas[i].dtype = in.dtype;
    metas[i].shape = in.shape;
    metas[i].shape[0] = rows;
    metas[i].content_bytes = uint64_t(rows) * in.row_bytes();
    // protobuf bytes fields cap at 2GB (TF enforces the same limit)
    if (metas[i].content_bytes >= (uint64_t(1) << 31))
      throw std::invalid_argument(
          "tensor '" + names[i] + "' exceeds the 2GB tensor_content limit "
          "of the protobuf wire format");
  }
  auto plan = tfswire::plan_predict_message(true, model_name, version,
                                            signature, names, metas);
  ShardPlan out;
  out.size = size_t(plan.total_size);
  out.skeleton.reset(new uint8_t[out.size ? out.size : 1]);
  tfswire::write_predict_message(out.skeleton.get(), plan, true, model_name,
                                 version, signature, names, metas);
  // write_predict_message emits tensors in input order, so span offsets
  // already ascend
  for (size_t i = 0; i < inputs.size(); ++i) {
    const auto& span = plan.spans[i];
    if (span.nbytes == 0) continue;
    const uint8_t* src =
        inputs[i].data + uint64_t(row_off) * inputs[i].row_bytes();
    if (inputs[i].device || span.nbytes >= kStreamMinSpan) {
      out.regions.push_back(Region{size_t(span.offset), size_t(span.nbytes),
                                   reinterpret_cast<uintptr_t>(src),
                                   inputs[i].device});
    } else {
      std::memcpy(out.skeleton.get() + span.offset, src, span.nbytes);
    }
  }
  return out;
}

// First channel of the next request. Consecutive requests start `shards`
// channels apart, so a request's shards ride distinct channels (when
// shards <= n_channels) and successive requests rotate over ALL channels:
// with 8 channels and 4 shards, requests alternate 0-3 / 4-7 instead of
// piling onto 0-3. Shard i of the request uses (start + i) % n_channels.
inline uint32_t next_start_channel(std::atomic<uint32_t>& counter,
                                   uint32_t n_channels, uint32_t shards) {
  if (n_channels == 0) throw std::invalid_argument("no channels");
  uint32_t k = counter.fetch_add(1, std::memory_order_relaxed);
  return uint32_t((uint64_t(k) * shards) % n_channels);
}

inline uint32_t shard_channel(uint32_t start, uint32_t shard,
                              uint32_t n_channels) {
  return (start + shard) % n_channels;
}

}  // namespace tfsshard
