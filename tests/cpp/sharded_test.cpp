// Standalone unit test for the sharded-Predict planner (ops/csrc/sharded.h)
// — no torch, no python, no HIP. Built and run under ASAN/UBSAN by
// tools/run_sanitizers.sh: the planner slices caller memory by row offsets
// and copies small spans into the skeleton, so an off-by-one here is an
// out-of-bounds read that the sanitizers catch.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../min_tfs_client_amd/ops/csrc/sharded.h"

using namespace tfsshard;

static int tests_run = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++tests_run;                                                           \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__,       \
                   #cond);                                                 \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int test_shard_sizes() {
  for (int64_t batch : {4, 5, 7, 33}) {
    for (int shards : {2, 3, 4}) {
      auto sizes = shard_sizes(batch, shards);
      CHECK(int(sizes.size()) == shards);
      // the divmod rule of TurboPredictClient.predict_sharded
      const int64_t base = batch / shards, rem = batch % shards;
      int64_t sum = 0;
      for (int i = 0; i < shards; ++i) {
        CHECK(sizes[size_t(i)] == base + (i < rem ? 1 : 0));
        CHECK(sizes[size_t(i)] >= 1);
        sum += sizes[size_t(i)];
      }
      CHECK(sum == batch);
    }
  }
  bool threw = false;
  try {
    shard_sizes(3, 4);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  return 0;
}

// Reference bytes of one shard: write_predict_message over the slice's
// metas, then every payload copied in (what the buffered serializer puts
// on the wire for the same narrow() view).
static std::vector<uint8_t> reference_message(
    const std::string& model, int64_t version, const std::string& sig,
    const std::vector<std::string>& names, const std::vector<Input>& inputs,
    int64_t row_off, int64_t rows) {
  std::vector<tfswire::TensorMeta> metas(inputs.size());
  for (size_t i = 0; i < inputs.size(); ++i) {
    metas[i].dtype = inputs[i].dtype;
    metas[i].shape = inputs[i].shape;
    metas[i].shape[0] = rows;
    metas[i].content_bytes = uint64_t(rows) * inputs[i].row_bytes();
  }
  auto plan =
      tfswire::plan_predict_message(true, model, version, sig, names, metas);
  std::vector<uint8_t> buf(plan.total_size);
  tfswire::write_predict_message(buf.data(), plan, true, model, version, sig,
                                 names, metas);
  for (size_t i = 0; i < inputs.size(); ++i)
    if (plan.spans[i].nbytes)
      std::memcpy(buf.data() + plan.spans[i].offset,
                  inputs[i].data + uint64_t(row_off) * inputs[i].row_bytes(),
                  plan.spans[i].nbytes);
  return buf;
}

// Assembles skeleton + regions the way the transport sends them.
static std::vector<uint8_t> assemble(const ShardPlan& p) {
  // holes start as 0xEE so an unfilled byte cannot pass for payload
  std::vector<uint8_t> out(p.size, 0xEE);
  size_t pos = 0;
  for (const auto& r : p.regions) {
    std::memcpy(out.data() + pos, p.skeleton.get() + pos, r.offset - pos);
    pos = r.offset + r.nbytes;
  }
  std::memcpy(out.data() + pos, p.skeleton.get() + pos, p.size - pos);
  for (const auto& r : p.regions)
    std::memcpy(out.data() + r.offset, reinterpret_cast<const void*>(r.ptr),
                r.nbytes);
  return out;
}

static int check_plans(const std::string& model, int64_t version,
                       const std::string& sig,
                       const std::vector<std::string>& names,
                       const std::vector<Input>& inputs, int shards,
                       size_t* regions_seen, size_t* inlined_seen) {
  auto sizes = shard_sizes(inputs[0].shape[0], shards);
  int64_t row = 0;
  for (int s = 0; s < shards; ++s) {
    ShardPlan p = plan_shard(model, version, sig, names, inputs, row,
                             sizes[size_t(s)]);
    auto ref = reference_message(model, version, sig, names, inputs, row,
                                 sizes[size_t(s)]);
    CHECK(p.size == ref.size());
    size_t prev_end = 0;
    for (const auto& r : p.regions) {
      CHECK(r.offset >= prev_end);  // ascending, non-overlapping
      CHECK(r.offset + r.nbytes <= p.size);
      CHECK(r.nbytes >= kStreamMinSpan);  // host spans below it are inlined
      CHECK(!r.device);
      prev_end = r.offset + r.nbytes;
    }
    *regions_seen += p.regions.size();
    *inlined_seen += inputs.size() - p.regions.size();
    CHECK(assemble(p) == ref);
    // parses back to the slice's shape
    auto parsed =
        tfswire::parse_predict_message(ref.data(), ref.size(), true);
    CHECK(parsed.tensors.size() == inputs.size());
    for (size_t i = 0; i < inputs.size(); ++i)
      CHECK(parsed.tensors[i].shape[0] == sizes[size_t(s)]);
    row += sizes[size_t(s)];
  }
  CHECK(row == inputs[0].shape[0]);
  return 0;
}

int test_plan_one_fp32_input() {
  // 33 rows x 6000 fp32 = 24000 B/row: shards of 16/17 rows are regions
  // (>= 64 KiB), shards of 8/9 rows too; with batch 4 (below) they inline
  size_t regions = 0, inlined = 0;
  for (int64_t batch : {4, 5, 7, 33}) {
    std::vector<float> data(size_t(batch) * 6000);
    for (size_t i = 0; i < data.size(); ++i) data[i] = float(i % 8191) * 0.5f;
    Input in;
    in.dtype = 1;
    in.shape = {batch, 3, 2000};
    in.elem_size = 4;
    in.data = reinterpret_cast<const uint8_t*>(data.data());
    for (int shards : {2, 3, 4})
      if (check_plans("resnet", 7, "serving_default", {"images"}, {in},
                      shards, &regions, &inlined))
        return 1;
  }
  CHECK(regions > 0);  // both the region and the inline branch ran
  CHECK(inlined > 0);
  return 0;
}

int test_plan_two_int32_inputs() {
  // one input crosses kStreamMinSpan per shard (region), one stays small
  // (inlined): ids rows are 8192 B, mask rows 64 B
  size_t regions = 0, inlined = 0;
  for (int64_t batch : {4, 5, 7, 33}) {
    std::vector<int32_t> ids(size_t(batch) * 2048), mask(size_t(batch) * 16);
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = int32_t(i * 7 + 1);
    for (size_t i = 0; i < mask.size(); ++i) mask[i] = int32_t(i & 1);
    Input a, b;
    a.dtype = b.dtype = 3;
    a.elem_size = b.elem_size = 4;
    a.shape = {batch, 2048};
    b.shape = {batch, 16};
    a.data = reinterpret_cast<const uint8_t*>(ids.data());
    b.data = reinterpret_cast<const uint8_t*>(mask.data());
    for (int shards : {2, 3, 4})
      if (check_plans("bert", -1, "", {"input_ids", "attention_mask"},
                      {a, b}, shards, &regions, &inlined))
        return 1;
  }
  CHECK(regions > 0);
  CHECK(inlined > 0);
  return 0;
}

int test_device_spans_are_always_regions() {
  // a device address is never dereferenced by the planner: even a tiny
  // span must become a (device) region, with the slice's address
  Input in;
  in.dtype = 1;
  in.shape = {5, 3};
  in.elem_size = 4;
  in.data = reinterpret_cast<const uint8_t*>(uintptr_t(0x7f0000000000ull));
  in.device = true;
  auto sizes = shard_sizes(5, 4);  // 2,1,1,1
  int64_t row = 0;
  for (size_t s = 0; s < sizes.size(); ++s) {
    ShardPlan p = plan_shard("m", 1, "sig", {"x"}, {in}, row, sizes[s]);
    CHECK(p.regions.size() == 1);
    CHECK(p.regions[0].device);
    CHECK(p.regions[0].nbytes == size_t(sizes[s]) * 12);
    CHECK(p.regions[0].ptr == uintptr_t(0x7f0000000000ull) + uint64_t(row) * 12);
    row += sizes[s];
  }
  bool threw = false;
  try {
    plan_shard("m", 1, "sig", {"x"}, {in}, 4, 2);  // rows 4..5 of 5
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  return 0;
}

int test_rotation_visits_all_channels() {
  for (uint32_t shards : {2u, 3u, 4u, 8u}) {
    std::atomic<uint32_t> counter{0};
    std::set<uint32_t> seen;
    for (int req = 0; req < 8; ++req) {
      uint32_t start = next_start_channel(counter, 8, shards);
      std::set<uint32_t> mine;
      for (uint32_t i = 0; i < shards; ++i) {
        uint32_t ch = shard_channel(start, i, 8);
        CHECK(ch < 8);
        mine.insert(ch);
        seen.insert(ch);
      }
      CHECK(mine.size() == shards);  // one request: distinct channels
    }
    CHECK(seen.size() == 8);
  }
  // 4 shards over 8 channels: consecutive requests use disjoint halves
  std::atomic<uint32_t> counter{0};
  CHECK(next_start_channel(counter, 8, 4) == 0);
  CHECK(next_start_channel(counter, 8, 4) == 4);
  CHECK(next_start_channel(counter, 8, 4) == 0);
  // fewer channels than shards still maps into range
  CHECK(shard_channel(next_start_channel(counter, 2, 4), 3, 2) < 2);
  return 0;
}

int main() {
  if (test_shard_sizes()) return 1;
  if (test_plan_one_fp32_input()) return 1;
  if (test_plan_two_int32_inputs()) return 1;
  if (test_device_spans_are_always_regions()) return 1;
  if (test_rotation_visits_all_channels()) return 1;
  std::printf("sharded_test: %d checks passed\n", tests_run);
  return 0;
}
