// Native gRPC (HTTP/2 cleartext) transport: server + client + bindings.
//
// From-scratch C++ replacement for python-grpcio on the Predict data plane.
// Speaks standard gRPC-over-HTTP/2 (interop-tested against grpcio peers in
// tests/integration/test_native_transport.py) with ~2 copies per hop:
//  * send: writev gathers DATA frames straight out of the wire-bytes buffer
//    (no serialize copy) — the analogue of the reference's two-slice
//    zero-copy encode (grpc_tensor_coding.cc:140-248);
//  * receive: DATA payloads are read from the socket directly into the
//    message buffer at their final offset (no reassembly pass);
//  * the identity-echo Predict path runs entirely in C++ (no GIL), parsing
//    the request in place and gathering the response from request payload
//    spans.
// Scope: unary-unary RPCs (the only kind PredictionService/ModelService
// use — reference prediction_service.proto:15-31); h2c only (TLS stays on
// the grpcio client path, client.py).
#include <pybind11/eval.h>
#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "h2core.h"
#include "hpack.h"
#include "sharded.h"
#include "staging.h"
#include "wire.h"

namespace py = pybind11;

namespace {

using h2::Buf;
using h2::Conn;
using h2::ConnError;
using h2::FrameHeader;

// ---------------------------------------------------------------------------
// streaming send: skeleton buffer + payload regions
// ---------------------------------------------------------------------------
// A streaming message is the wire skeleton (tensor_content holes unwritten)
// plus an ascending list of payload regions. Host regions are written
// straight from tensor memory (zero-copy send — the reference's two-slice
// encode, grpc_tensor_coding.cc:140-248, as iovec gathers); device regions
// are staged through the pooled pinned pipeline (staging.h) with the
// socket write as the chunk consumer, so the hipMemcpyAsync of chunk i+1
// overlaps the DATA-frame send of chunk i.
struct WireRegion {
  size_t offset;
  size_t nbytes;
  uintptr_t ptr;
  bool device;
};

void write_message_with_regions(Conn& conn, uint32_t stream,
                                const uint8_t* buf, size_t len,
                                const std::vector<WireRegion>& regions,
                                bool end_stream) {
  h2::DataMessageWriter w(conn, stream, len, end_stream);
  size_t pos = 0;
  for (const auto& r : regions) {
    if (r.offset < pos || r.nbytes > len || r.offset > len - r.nbytes)
      throw ConnError("bad streaming region");
    if (r.offset > pos) w.write(buf + pos, r.offset - pos);
    if (!r.device) {
      w.write(reinterpret_cast<const uint8_t*>(r.ptr), r.nbytes);
    } else {
      mi355x_staging::Lease lease;
      lease.ctx->d2h(reinterpret_cast<const void*>(r.ptr), r.nbytes,
                     [&w](const void* chunk, size_t n) {
                       w.write(static_cast<const uint8_t*>(chunk), n);
                     });
    }
    pos = r.offset + r.nbytes;
  }
  if (pos < len) w.write(buf + pos, len - pos);
  w.finish();
}

// GIL must be held. Returns true when `result` is a streaming reply
// (duck-typed on ._wire_regions), filling the skeleton buffer view and
// region list. The buffer_info pins the skeleton; the python object itself
// keeps the region tensors alive (.keepalive).
bool extract_streaming_reply(py::handle result,
                             std::unique_ptr<py::buffer_info>* info,
                             const uint8_t** buf, size_t* len,
                             std::vector<WireRegion>* regions) {
  if (!py::hasattr(result, "_wire_regions")) return false;
  py::object buffer = result.attr("buffer");
  *info = std::make_unique<py::buffer_info>(py::buffer(buffer).request());
  *buf = static_cast<const uint8_t*>((*info)->ptr);
  *len = size_t((*info)->size) * size_t((*info)->itemsize);
  for (auto item : result.attr("_wire_regions")) {
    auto t = py::reinterpret_borrow<py::tuple>(item);
    regions->push_back(WireRegion{
        t[0].cast<size_t>(), t[1].cast<size_t>(),
        uintptr_t(t[2].cast<uint64_t>()), t[3].cast<bool>()});
  }
  return true;
}

// ---------------------------------------------------------------------------
// grpc status error (translated to min_tfs_client_amd NativeRpcError)
// ---------------------------------------------------------------------------
struct RpcCallError : std::runtime_error {
  int code;
  RpcCallError(int code_, const std::string& msg)
      : std::runtime_error(msg), code(code_) {}
};

constexpr int GRPC_OK = 0;
constexpr int GRPC_CANCELLED = 1;
constexpr int GRPC_UNKNOWN = 2;
constexpr int GRPC_INVALID_ARGUMENT = 3;
constexpr int GRPC_DEADLINE_EXCEEDED = 4;
constexpr int GRPC_RESOURCE_EXHAUSTED = 8;
constexpr int GRPC_UNIMPLEMENTED = 12;
constexpr int GRPC_INTERNAL = 13;
constexpr int GRPC_UNAVAILABLE = 14;

// ---------------------------------------------------------------------------
// zero-copy response holder exposed to python via the buffer protocol
// ---------------------------------------------------------------------------
struct OwnedBuf {
  Buf buf;
  explicit OwnedBuf(Buf&& b) : buf(std::move(b)) {}
};

// ---------------------------------------------------------------------------
// pinned receive pool
// ---------------------------------------------------------------------------
// Large gRPC messages (tensor payloads) are read from the socket into
// POOLED PINNED buffers, so the subsequent H2D unpack to the GPU is a
// true DMA at link speed instead of a pageable staged copy. Buffers
// recycle through a size-classed freelist (hipHostMalloc is ~ms-scale, so
// per-message allocation would erase the win); cached bytes are capped.
// On hosts without a GPU (or if pinning fails) callers fall back to
// malloc transparently.
class PinnedPool {
 public:
  static PinnedPool& instance() {
    static PinnedPool* pool = new PinnedPool();  // leaked: outlives HIP
    return *pool;
  }

  static constexpr size_t kMinPinned = 1u << 20;    // pool only >=1MB
  static constexpr size_t kMaxCached = 512u << 20;  // freelist cap

  bool available() {
    int state = state_.load(std::memory_order_acquire);
    if (state == 0) {
      int n = 0;
      bool ok = hipGetDeviceCount(&n) == hipSuccess && n > 0;
      state = ok ? 1 : -1;
      state_.store(state, std::memory_order_release);
    }
    return state > 0;
  }

  // rounded-up pinned buffer or nullptr (caller falls back to malloc)
  uint8_t* get(size_t n, size_t* cap_out) {
    if (n < kMinPinned || !available()) return nullptr;
    size_t cap = size_class(n);
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto& fl = free_[cap];
      if (!fl.empty()) {
        uint8_t* p = fl.back();
        fl.pop_back();
        cached_ -= cap;
        *cap_out = cap;
        return p;
      }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, cap) != hipSuccess) return nullptr;
    *cap_out = cap;
    return static_cast<uint8_t*>(p);
  }

  void put(uint8_t* p, size_t cap) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (cached_ + cap <= kMaxCached) {
        free_[cap].push_back(p);
        cached_ += cap;
        return;
      }
    }
    (void)hipHostFree(p);
  }

  static void deleter(void* ctx, uint8_t* p, size_t cap) {
    static_cast<PinnedPool*>(ctx)->put(p, cap);
  }

 private:
  static size_t size_class(size_t n) {
    size_t cap = kMinPinned;
    while (cap < n) cap <<= 1;
    return cap;
  }
  std::atomic<int> state_{0};  // 0 unknown, 1 available, -1 unavailable
  std::mutex mu_;
  std::map<size_t, std::vector<uint8_t*>> free_;
  size_t cached_ = 0;
};

// ---------------------------------------------------------------------------
// progressive device parse (receive-side overlap)
// ---------------------------------------------------------------------------
// While a PredictResponse is still streaming in off the socket, the client
// reader walks the canonical wire layout (model_spec, then outputs map
// entries whose dtype/shape headers precede their tensor_content) and
// issues hipMemcpyAsync H2D for each content span's already-received bytes
// straight out of the pinned receive buffer — by the time the trailers
// arrive, the output tensors are already (mostly) resident in HBM. Any
// non-canonical layout (typed *_val fields, unknown fields, repeat-fill
// shapes) flips `failed` and the caller falls back to the ordinary
// post-receive parse; correctness never depends on the prospector.

inline bool tf_dtype_to_scalar(int dt, at::ScalarType* st) {
  switch (dt) {
    case 1: *st = at::kFloat; return true;
    case 2: *st = at::kDouble; return true;
    case 3: *st = at::kInt; return true;
    case 4: *st = at::kByte; return true;
    case 5: *st = at::kShort; return true;
    case 6: *st = at::kChar; return true;
    case 8: *st = at::kComplexFloat; return true;
    case 9: *st = at::kLong; return true;
    case 10: *st = at::kBool; return true;
    case 14: *st = at::kBFloat16; return true;
    case 17: *st = at::kUInt16; return true;
    case 18: *st = at::kComplexDouble; return true;
    case 19: *st = at::kHalf; return true;
    case 22: *st = at::kUInt32; return true;
    case 23: *st = at::kUInt64; return true;
    default: return false;
  }
}


// Record the calling thread's current stream as a user of every
// prospected tensor: their blocks are associated with the pool copy
// stream, so without this the allocator could hand a freed block back
// to the copy stream while the consumer's reads are still in flight.
inline void record_consumer_stream(
    std::vector<std::pair<std::string, at::Tensor>>& outs, int device) {
  if (outs.empty()) return;
  auto cur = c10::hip::getCurrentHIPStream(
      static_cast<c10::DeviceIndex>(device));
  for (auto& kv : outs)
    c10::hip::HIPCachingAllocator::recordStream(
        kv.second.storage().data_ptr(), cur);
}

struct MsgAssemblyFwd;  // below

// Small immortal pool of prospect copy streams per device. Connections
// and channels BORROW a stream round-robin instead of creating their
// own: per-connection hipStreamCreate/Destroy churn (thousands per
// minute under client churn) stresses the driver — a box died under
// tools/soak_churn.py before this pool existed. Streams are never
// destroyed, so DeviceParse::quiesce can always sync its handle.
class ProspectStreams {
 public:
  static ProspectStreams& instance() {
    static ProspectStreams* p = new ProspectStreams();  // leaked: immortal
    return *p;
  }

  static constexpr int kPerDevice = 4;

  hipStream_t get(int device) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = per_dev_.find(device);
    if (it == per_dev_.end()) {
      std::vector<hipStream_t> v;
      if (hipSetDevice(device) == hipSuccess) {
        for (int i = 0; i < kPerDevice; ++i) {
          hipStream_t s = nullptr;
          if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) !=
              hipSuccess)
            break;
          v.push_back(s);
        }
      }
      it = per_dev_.emplace(device, std::move(v)).first;
    }
    if (it->second.empty()) return nullptr;
    return it->second[rr_++ % it->second.size()];
  }

 private:
  std::mutex mu_;
  std::unordered_map<int, std::vector<hipStream_t>> per_dev_;
  size_t rr_ = 0;
};

struct DeviceParse {
  bool enabled = false;
  bool failed = false;
  bool done = false;
  int device = 0;
  hipStream_t stream = nullptr;  // owned by the channel / connection
  // message layout: response (spec=2, entries=1) by default; requests
  // (server side) flip to spec=1, entries=2 and may carry output_filter
  int spec_field = 2;
  int map_field = 1;
  // captured model_spec (server-side request prospecting needs it)
  std::string spec_name, spec_signature, spec_label;
  int64_t spec_version = -1;
  std::vector<std::string> out_filter;
  // server-side: skip prospecting for models served by the C++ echo
  // fast path (their payloads never touch the GPU)
  std::function<bool(const std::string&)> skip_model;
  // structural state
  size_t pos = 0;       // absolute offset parsed so far
  int state = 0;        // 0 TOP, 1 ENTRY, 2 TENSOR
  size_t entry_end = 0, tp_end = 0;
  std::string cur_name;
  int cur_dtype = 0;
  std::vector<int64_t> cur_shape;
  bool cur_has_tensor = false;
  at::Tensor cur_tensor;
  // content copy state
  bool in_content = false;
  size_t content_off = 0, content_len = 0, content_copied = 0;
  bool copies_issued = false;
  std::vector<std::pair<std::string, at::Tensor>> outs;

  static constexpr size_t kCopyBatch = 1u << 20;  // batch tiny arrivals

  void fail() {
    failed = true;
    in_content = false;
  }

  // RAII: every destruction path (stream reset, connection death, failed
  // prospect, task teardown) must drain in-flight H2D copies BEFORE the
  // source buffer and the destination tensors are freed — a pinned
  // receive buffer hipHostFree'd with a pending SDMA read (or a tensor
  // freed with a pending write) is a crash/corruption. The dtor body
  // runs before member (outs) destruction; the stream itself is an
  // immortal ProspectStreams handle, so syncing it here is always valid.
  void quiesce() {
    if (copies_issued && stream != nullptr) {
      (void)hipStreamSynchronize(stream);
      copies_issued = false;
    }
  }

  DeviceParse() = default;
  DeviceParse(const DeviceParse&) = delete;
  DeviceParse& operator=(const DeviceParse&) = delete;
  DeviceParse(DeviceParse&& o) noexcept { *this = std::move(o); }
  DeviceParse& operator=(DeviceParse&& o) noexcept {
    if (this != &o) {
      quiesce();
      enabled = o.enabled; failed = o.failed; done = o.done;
      device = o.device; stream = o.stream;
      spec_field = o.spec_field; map_field = o.map_field;
      spec_name = std::move(o.spec_name);
      spec_signature = std::move(o.spec_signature);
      spec_label = std::move(o.spec_label);
      spec_version = o.spec_version;
      out_filter = std::move(o.out_filter);
      skip_model = std::move(o.skip_model);
      pos = o.pos; state = o.state;
      entry_end = o.entry_end; tp_end = o.tp_end;
      cur_name = std::move(o.cur_name);
      cur_dtype = o.cur_dtype;
      cur_shape = std::move(o.cur_shape);
      cur_has_tensor = o.cur_has_tensor;
      cur_tensor = std::move(o.cur_tensor);
      in_content = o.in_content;
      content_off = o.content_off;
      content_len = o.content_len;
      content_copied = o.content_copied;
      copies_issued = o.copies_issued;
      outs = std::move(o.outs);
      o.copies_issued = false;
      o.enabled = false;
      o.stream = nullptr;
    }
    return *this;
  }
  ~DeviceParse() { quiesce(); }
};

// ---------------------------------------------------------------------------
// in-flight message assembly (shared shape between server request streams
// and client response streams)
// ---------------------------------------------------------------------------
struct MsgAssembly {
  uint8_t prefix[5];
  size_t prefix_have = 0;
  Buf msg;
  size_t msg_have = 0;
  bool have_len = false;

  // feeds `n` DATA bytes straight from the socket into the right place;
  // returns after consuming exactly n bytes from fd
  void feed_from_socket(int fd, size_t n) {
    while (n > 0) {
      if (prefix_have < 5) {
        size_t take = 5 - prefix_have < n ? 5 - prefix_have : n;
        h2::read_full(fd, prefix + prefix_have, take);
        prefix_have += take;
        n -= take;
        if (prefix_have == 5) {
          if (prefix[0] != 0)
            throw RpcCallError(GRPC_UNIMPLEMENTED,
                               "compressed gRPC messages not supported");
          uint32_t len = h2::be32(prefix + 1);
          // match the grpcio servers' max_receive_message_length (1GB):
          // an attacker-declared length must not drive the allocation
          if (len > (1u << 30))
            throw RpcCallError(
                GRPC_RESOURCE_EXHAUSTED,
                "received message larger than max (" +
                    std::to_string(len) + " vs 1073741824)");
          size_t cap = 0;
          auto& pool = PinnedPool::instance();
          uint8_t* pinned = pool.get(len, &cap);
          if (pinned != nullptr)
            msg.adopt(pinned, cap, &PinnedPool::deleter, &pool);
          else
            msg.alloc(len);
          msg.len = len;
          have_len = true;
        }
        continue;
      }
      if (!have_len || msg_have + n > msg.len)
        throw ConnError("DATA overruns gRPC message length");
      h2::read_full(fd, msg.p + msg_have, n);
      msg_have += n;
      n = 0;
    }
  }

  bool complete() const { return have_len && msg_have == msg.len; }
};

// One incremental step of the receive-side device parse. Called by the
// client reader after every DATA feed; transactional — a structural
// element that is only partially received is retried on the next feed.
inline void device_parse_advance(DeviceParse& dp, MsgAssembly& body) {
  if (!dp.enabled || dp.failed || dp.done) return;
  if (!body.have_len) return;
  if (dp.pos == 0 && dp.outs.empty() && !dp.in_content) {
    // async H2D needs a pinned source; small messages skip the machinery
    if (body.msg.deleter == nullptr || body.msg.len < (1u << 20)) {
      dp.enabled = false;
      return;
    }
  }
  const uint8_t* base = body.msg.p;
  const size_t watermark = body.msg_have;
  const size_t total = body.msg.len;

  auto issue_copies = [&]() -> bool {
    // returns true when the current span finished copying
    size_t span_end = dp.content_off + dp.content_len;
    size_t have_end = watermark < span_end ? watermark : span_end;
    size_t done_abs = dp.content_off + dp.content_copied;
    if (have_end > done_abs) {
      size_t n = have_end - done_abs;
      bool flush = have_end == span_end || body.complete();
      if (n >= DeviceParse::kCopyBatch || flush) {
        if (hipSetDevice(dp.device) != hipSuccess) { dp.fail(); return false; }
        char* dst = static_cast<char*>(dp.cur_tensor.data_ptr())
                    + dp.content_copied;
        if (hipMemcpyAsync(dst, base + done_abs, n, hipMemcpyHostToDevice,
                           dp.stream) != hipSuccess) {
          dp.fail();
          return false;
        }
        dp.copies_issued = true;
        dp.content_copied += n;
      }
    }
    return dp.content_copied == dp.content_len;
  };

  try {
    while (true) {
      if (dp.in_content) {
        if (!issue_copies()) return;  // need more bytes (or failed)
        if (dp.failed) return;
        dp.in_content = false;
        dp.pos = dp.content_off + dp.content_len;
        dp.cur_has_tensor = true;
      }
      tfswire::Cursor c{base + dp.pos, base + watermark};
      const uint8_t* step_start = c.p;
      try {
        if (dp.state == 0) {  // TOP level of the Predict message
          if (dp.pos == total) {
            dp.done = true;
            return;
          }
          int wt = 0;
          int f = c.read_tag(&wt);
          if (f == dp.spec_field && wt == tfswire::WT_LEN) {  // model_spec
            tfswire::Cursor spec = c.read_len_delim();  // waits if partial
            while (!spec.done()) {
              int swt = 0;
              int sf = spec.read_tag(&swt);
              if (sf == 1 && swt == tfswire::WT_LEN) {
                tfswire::Cursor v = spec.read_len_delim();
                dp.spec_name.assign(reinterpret_cast<const char*>(v.p),
                                    size_t(v.end - v.p));
              } else if (sf == 2 && swt == tfswire::WT_LEN) {
                tfswire::Cursor v = spec.read_len_delim();  // Int64Value
                while (!v.done()) {
                  int vwt = 0;
                  int vf = v.read_tag(&vwt);
                  if (vf == 1 && vwt == tfswire::WT_VARINT)
                    dp.spec_version = int64_t(v.read_varint());
                  else
                    v.skip(vwt);
                }
              } else if (sf == 3 && swt == tfswire::WT_LEN) {
                tfswire::Cursor v = spec.read_len_delim();
                dp.spec_signature.assign(
                    reinterpret_cast<const char*>(v.p),
                    size_t(v.end - v.p));
              } else if (sf == 4 && swt == tfswire::WT_LEN) {
                tfswire::Cursor v = spec.read_len_delim();
                dp.spec_label.assign(reinterpret_cast<const char*>(v.p),
                                     size_t(v.end - v.p));
              } else {
                spec.skip(swt);
              }
            }
            if (dp.skip_model && dp.skip_model(dp.spec_name)) {
              dp.enabled = false;  // echo fast path: stay off the GPU
              return;
            }
            dp.pos = size_t(c.p - base);
          } else if (f == dp.map_field && wt == tfswire::WT_LEN) {
            uint64_t len = c.read_varint();
            size_t body_off = size_t(c.p - base);
            if (body_off + len > total) { dp.fail(); return; }
            dp.entry_end = body_off + len;
            dp.pos = body_off;
            dp.state = 1;
          } else if (dp.spec_field == 1 && f == 3 &&
                     wt == tfswire::WT_LEN) {  // request output_filter
            tfswire::Cursor v = c.read_len_delim();
            dp.out_filter.emplace_back(
                reinterpret_cast<const char*>(v.p), size_t(v.end - v.p));
            dp.pos = size_t(c.p - base);
          } else {
            dp.fail();
            return;
          }
        } else if (dp.state == 1) {  // entry: key then value(TensorProto)
          int wt = 0;
          int f = c.read_tag(&wt);
          if (f != 1 || wt != tfswire::WT_LEN) { dp.fail(); return; }
          tfswire::Cursor key = c.read_len_delim();
          dp.cur_name.assign(reinterpret_cast<const char*>(key.p),
                             size_t(key.end - key.p));
          f = c.read_tag(&wt);
          if (f != 2 || wt != tfswire::WT_LEN) { dp.fail(); return; }
          uint64_t len = c.read_varint();
          size_t body_off = size_t(c.p - base);
          if (body_off + len > dp.entry_end) { dp.fail(); return; }
          dp.tp_end = body_off + len;
          dp.pos = body_off;
          dp.state = 2;
          dp.cur_dtype = 0;
          dp.cur_shape.clear();
          dp.cur_has_tensor = false;
          dp.cur_tensor = at::Tensor();
        } else {  // state 2: inside TensorProto
          if (dp.pos == dp.tp_end) {
            // finalize this output
            if (!dp.cur_has_tensor) {
              int64_t numel = 1;
              for (int64_t d : dp.cur_shape) numel *= d;
              at::ScalarType st;
              if (numel == 0 && tf_dtype_to_scalar(dp.cur_dtype, &st)) {
                c10::hip::HIPStreamGuard g(c10::hip::getStreamFromExternal(
                    dp.stream, static_cast<c10::DeviceIndex>(dp.device)));
                dp.cur_tensor = at::empty(
                    dp.cur_shape, at::TensorOptions().dtype(st).device(
                                      at::kCUDA, dp.device));
                dp.cur_has_tensor = true;
              } else {
                dp.fail();
                return;
              }
            }
            dp.outs.emplace_back(dp.cur_name, dp.cur_tensor);
            dp.cur_tensor = at::Tensor();
            if (dp.pos != dp.entry_end) { dp.fail(); return; }
            dp.state = 0;
            continue;
          }
          int wt = 0;
          int f = c.read_tag(&wt);
          if (f == 1 && wt == tfswire::WT_VARINT) {
            dp.cur_dtype = int(c.read_varint());
          } else if (f == 2 && wt == tfswire::WT_LEN) {
            tfswire::Cursor sh = c.read_len_delim();
            dp.cur_shape.clear();
            while (!sh.done()) {
              int swt = 0;
              int sf = sh.read_tag(&swt);
              if (sf == 2 && swt == tfswire::WT_LEN) {
                tfswire::Cursor dim = sh.read_len_delim();
                int64_t size = 0;
                while (!dim.done()) {
                  int dwt = 0;
                  int df = dim.read_tag(&dwt);
                  if (df == 1 && dwt == tfswire::WT_VARINT)
                    size = int64_t(dim.read_varint());
                  else
                    dim.skip(dwt);
                }
                dp.cur_shape.push_back(size);
              } else if (sf == 3) {  // unknown_rank: cannot preallocate
                dp.fail();
                return;
              } else {
                sh.skip(swt);
              }
            }
          } else if (f == 3 && wt == tfswire::WT_VARINT) {
            (void)c.read_varint();  // version_number
          } else if (f == 4 && wt == tfswire::WT_LEN) {  // tensor_content
            uint64_t len = c.read_varint();
            size_t off = size_t(c.p - base);
            if (off + len > dp.tp_end) { dp.fail(); return; }
            at::ScalarType st;
            if (!tf_dtype_to_scalar(dp.cur_dtype, &st)) { dp.fail(); return; }
            int64_t numel = 1;
            for (int64_t d : dp.cur_shape) numel *= d;
            size_t esize = at::elementSize(st);
            if (uint64_t(numel) * esize != len) { dp.fail(); return; }
            {
              // allocate ON the copy stream: the caching allocator then
              // orders block reuse against S, so our H2D never lands in
              // a block another stream is still reading (the cross-
              // stream reuse race tools/soak_churn.py exposed)
              c10::hip::HIPStreamGuard g(c10::hip::getStreamFromExternal(
                  dp.stream, static_cast<c10::DeviceIndex>(dp.device)));
              dp.cur_tensor = at::empty(
                  dp.cur_shape,
                  at::TensorOptions().dtype(st).device(at::kCUDA,
                                                       dp.device));
            }
            dp.content_off = off;
            dp.content_len = size_t(len);
            dp.content_copied = 0;
            dp.in_content = true;
            dp.pos = off;
            continue;  // enter the copy loop
          } else {
            dp.fail();  // typed *_val or unknown field
            return;
          }
          dp.pos = size_t(c.p - base);
        }
      } catch (const std::exception&) {
        // truncated inside a structural element: if the message is
        // complete this is malformed, else retry on the next feed
        (void)step_start;
        if (body.complete()) dp.fail();
        return;
      }
    }
  } catch (...) {
    dp.fail();
  }
}

// ---------------------------------------------------------------------------
// header-block assembly (HEADERS + CONTINUATION)
// ---------------------------------------------------------------------------
struct HeaderBlock {
  std::string block;
  bool end_stream = false;
  bool done = false;
};

// reads one HEADERS frame's block fragment (handling PADDED/PRIORITY)
inline void read_headers_fragment(int fd, const FrameHeader& fh,
                                  std::string* out) {
  uint32_t len = fh.length;
  uint8_t pad = 0;
  if (fh.flags & h2::FL_PADDED) {
    h2::read_full(fd, &pad, 1);
    if (len < 1u + pad) throw ConnError("bad padding");
    len -= 1;
  }
  if (fh.flags & h2::FL_PRIORITY) {
    uint8_t prio[5];
    if (len < 5) throw ConnError("bad priority");
    h2::read_full(fd, prio, 5);
    len -= 5;
  }
  len -= pad;
  size_t off = out->size();
  out->resize(off + len);
  h2::read_full(fd, reinterpret_cast<uint8_t*>(&(*out)[off]), len);
  if (pad) h2::discard(fd, pad);
}

inline const std::string* find_header(const std::vector<h2::Header>& hs,
                                      const char* name) {
  for (auto& h : hs)
    if (h.first == name) return &h.second;
  return nullptr;
}

// ---------------------------------------------------------------------------
// response header/trailer blocks (hpack encode, stateless)
// ---------------------------------------------------------------------------
inline std::string make_response_headers_block() {
  h2::HpackEncoder enc;
  std::string block;
  enc.add_indexed(&block, 8);  // :status: 200
  enc.add_literal(&block, 31, "application/grpc");  // content-type
  return block;
}

inline std::string make_trailers_block(int status, const std::string& msg) {
  h2::HpackEncoder enc;
  std::string block;
  enc.add_literal(&block, "grpc-status", std::to_string(status));
  if (!msg.empty())
    enc.add_literal(&block, "grpc-message", h2::percent_encode(msg));
  return block;
}

inline std::string make_trailers_only_block(int status,
                                            const std::string& msg) {
  h2::HpackEncoder enc;
  std::string block;
  enc.add_indexed(&block, 8);  // :status: 200
  enc.add_literal(&block, 31, "application/grpc");
  enc.add_literal(&block, "grpc-status", std::to_string(status));
  if (!msg.empty())
    enc.add_literal(&block, "grpc-message", h2::percent_encode(msg));
  return block;
}

// ---------------------------------------------------------------------------
// C++ identity echo (no GIL): parse request in place, emit the response
// gathering payloads from the request spans. Mirrors identity_servable
// (server.py): aliases '*_input' -> '*_output', else key unchanged.
// ---------------------------------------------------------------------------
inline bool echo_eligible(const tfswire::ParsedPredict& req,
                          const std::map<std::string, std::set<int64_t>>&
                              models) {
  if (!req.output_filter.empty()) return false;
  auto it = models.find(req.model_spec.name);
  if (it == models.end()) return false;
  if (req.model_spec.version >= 0 &&
      it->second.find(req.model_spec.version) == it->second.end())
    return false;
  if (!req.model_spec.version_label.empty()) return false;
  for (auto& t : req.tensors)
    if (t.content == nullptr) return false;
  return true;
}

// Zero-copy echo: only the response SKELETON is materialized; payload
// spans >= 64KB stay in the request buffer and are sent as host regions
// (iovec straight from the request bytes). Small spans are copied into
// the skeleton — fewer frames beats the copy at that size. The caller
// must keep the request buffer alive through the send (Task::msg does).
struct EchoResponse {
  Buf skeleton;
  std::vector<WireRegion> regions;
};

inline EchoResponse build_echo_response(const tfswire::ParsedPredict& req) {
  constexpr size_t kEchoMinRegion = 64 * 1024;
  std::vector<std::string> names;
  std::vector<tfswire::TensorMeta> metas;
  std::vector<const uint8_t*> payloads;
  names.reserve(req.tensors.size());
  for (auto& t : req.tensors) {
    std::string name = t.name;
    const std::string suffix = "_input";
    if (name.size() > suffix.size() &&
        name.compare(name.size() - suffix.size(), suffix.size(), suffix) ==
            0) {
      name = name.substr(0, name.size() - suffix.size()) + "_output";
    }
    names.push_back(std::move(name));
    metas.push_back({t.dtype, t.shape, t.content_bytes});
    payloads.push_back(t.content);
  }
  const std::string sig = req.model_spec.signature_name.empty()
                              ? "serving_default"
                              : req.model_spec.signature_name;
  auto plan = tfswire::plan_predict_message(false, req.model_spec.name,
                                            req.model_spec.version, sig,
                                            names, metas);
  EchoResponse r;
  r.skeleton = Buf(plan.total_size);
  r.skeleton.len = plan.total_size;
  tfswire::write_predict_message(r.skeleton.p, plan, false,
                                 req.model_spec.name,
                                 req.model_spec.version, sig, names, metas);
  // spans are emitted in tensor order; offsets ascend within the message
  for (size_t i = 0; i < payloads.size(); ++i) {
    const auto& span = plan.spans[i];
    if (span.nbytes >= kEchoMinRegion) {
      r.regions.push_back(WireRegion{
          span.offset, span.nbytes,
          reinterpret_cast<uintptr_t>(payloads[i]), false});
    } else if (span.nbytes > 0) {
      std::memcpy(r.skeleton.p + span.offset, payloads[i], span.nbytes);
    }
  }
  std::sort(r.regions.begin(), r.regions.end(),
            [](const WireRegion& a, const WireRegion& b) {
              return a.offset < b.offset;
            });
  return r;
}

// ===========================================================================
// Server
// ===========================================================================

class GrpcServer {
 public:
  GrpcServer(std::string address, int workers)
      : address_(std::move(address)),
        n_workers_(workers > 0 ? workers : 8) {}

  ~GrpcServer() {
    // joining worker threads (which may be waiting for the GIL) must not
    // happen while this thread holds the GIL
    if (Py_IsInitialized() && PyGILState_Check()) {
      py::gil_scoped_release release;
      stop_internal(true);
    } else {
      stop_internal(true);
    }
  }

  // extra listen addresses (e.g. --grpc_socket_path); call before start()
  void add_address(const std::string& address) {
    extra_addresses_.push_back(address);
  }

  std::string start() {
    listen_fds_.push_back(make_listener(address_, &bound_address_));
    for (auto& extra : extra_addresses_) {
      std::string bound;
      listen_fds_.push_back(make_listener(extra, &bound));
    }
    for (int i = 0; i < n_workers_; ++i)
      workers_.emplace_back([this] { worker_loop(); });
    for (int fd : listen_fds_)
      accept_threads_.emplace_back([this, fd] { accept_loop(fd); });
    running_ = true;
    return bound_address_;
  }

  void register_handler(const std::string& path, py::object fn) {
    std::lock_guard<std::mutex> lk(handler_mu_);
    py_handlers_[path] = std::move(fn);
  }

  // handler called as fn(view, spec_dict_or_None, outs_dict_or_None):
  // requests on `path` are prospected while they stream in and their
  // tensor_content spans H2D'd to `device` (see DeviceParse)
  void register_handler_parsed(const std::string& path, py::object fn,
                               int device) {
    std::lock_guard<std::mutex> lk(handler_mu_);
    py_handlers_[path] = std::move(fn);
    parsed_paths_[path] = device;
  }

  void set_echo_models(
      const std::string& path,
      const std::map<std::string, std::set<int64_t>>& models) {
    std::lock_guard<std::mutex> lk(handler_mu_);
    if (models.empty())
      echo_models_.erase(path);
    else
      echo_models_[path] = models;
  }

  void stop() { stop_internal(true); }

  // per-path stats for requests handled entirely in C++ (the echo fast
  // path — python handlers do their own MetricsRegistry accounting)
  py::dict stats() {
    py::dict out;
    std::lock_guard<std::mutex> lk(stats_mu_);
    for (auto& kv : stats_) {
      py::dict d;
      d["count"] = kv.second.count;
      d["total_s"] = kv.second.total_s;
      d["bytes_rx"] = kv.second.bytes_rx;
      d["bytes_tx"] = kv.second.bytes_tx;
      py::list samples;
      for (double s : kv.second.samples) samples.append(s);
      d["samples_s"] = samples;
      out[py::str(kv.first)] = d;
    }
    return out;
  }

 private:
  struct PathStats {
    uint64_t count = 0;
    double total_s = 0.0;
    uint64_t bytes_rx = 0;
    uint64_t bytes_tx = 0;
    std::vector<double> samples;  // capped reservoir
  };
  std::mutex stats_mu_;
  std::unordered_map<std::string, PathStats> stats_;

  void record_stats(const std::string& path, double secs, uint64_t rx,
                    uint64_t tx) {
    std::lock_guard<std::mutex> lk(stats_mu_);
    auto& s = stats_[path];
    s.count += 1;
    s.total_s += secs;
    s.bytes_rx += rx;
    s.bytes_tx += tx;
    if (s.samples.size() < 8192) s.samples.push_back(secs);
  }
  std::string address_;
  std::string bound_address_;
  std::vector<std::string> extra_addresses_;
  int n_workers_;
  std::vector<int> listen_fds_;
  std::atomic<bool> running_{false};
  std::atomic<bool> stopping_{false};
  std::vector<std::thread> accept_threads_;
  std::vector<std::thread> workers_;
  // connections are keyed so finished ones can be REAPED while the
  // server runs: a churning client must not accumulate dead fds and
  // threads until EMFILE (found by tools/soak_churn.py)
  std::mutex conns_mu_;
  uint64_t conn_serial_ = 0;
  std::map<uint64_t, std::thread> conn_threads_;
  std::map<uint64_t, std::shared_ptr<Conn>> conns_;
  std::deque<uint64_t> finished_conns_;
  std::vector<std::string> unix_paths_;  // unlink on stop

  // joins connection threads whose loops have exited (called from the
  // accept loops; never called for the caller's own thread)
  void reap_finished_conns() {
    std::vector<std::thread> done;
    {
      std::lock_guard<std::mutex> lk(conns_mu_);
      while (!finished_conns_.empty()) {
        uint64_t id = finished_conns_.front();
        finished_conns_.pop_front();
        auto it = conn_threads_.find(id);
        if (it != conn_threads_.end()) {
          done.push_back(std::move(it->second));
          conn_threads_.erase(it);
        }
      }
    }
    for (auto& th : done)
      if (th.joinable()) th.join();
  }

  std::mutex handler_mu_;
  std::unordered_map<std::string, py::object> py_handlers_;
  std::unordered_map<std::string, int> parsed_paths_;
  std::unordered_map<std::string, std::map<std::string, std::set<int64_t>>>
      echo_models_;

  struct Task {
    std::shared_ptr<Conn> conn;
    uint32_t stream = 0;
    std::string path;
    Buf msg;
    DeviceParse dparse;  // dtor quiesces before msg's buffer is freed
  };
  std::mutex q_mu_;
  std::condition_variable q_cv_;
  std::deque<Task> queue_;

  int make_listener(const std::string& address, std::string* bound) {
    if (address.rfind("unix:", 0) == 0) {
      std::string path = address.substr(5);
      while (path.size() >= 2 && path[0] == '/' && path[1] == '/')
        path = path.substr(1);
      ::unlink(path.c_str());
      int fd = ::socket(AF_UNIX, SOCK_STREAM, 0);
      if (fd < 0) throw ConnError("socket: " + std::string(strerror(errno)));
      sockaddr_un addr{};
      addr.sun_family = AF_UNIX;
      if (path.size() >= sizeof(addr.sun_path))
        throw ConnError("unix path too long");
      std::memcpy(addr.sun_path, path.c_str(), path.size() + 1);
      if (::bind(fd, reinterpret_cast<sockaddr*>(&addr), sizeof(addr)) < 0 ||
          ::listen(fd, 128) < 0) {
        int e = errno;
        ::close(fd);
        throw ConnError("bind/listen " + path + ": " + strerror(e));
      }
      unix_paths_.push_back(path);
      *bound = address;
      return fd;
    }
    auto colon = address.rfind(':');
    std::string host =
        colon == std::string::npos ? address : address.substr(0, colon);
    int port = colon == std::string::npos
                   ? 0
                   : std::atoi(address.c_str() + colon + 1);
    if (host.empty() || host == "localhost") host = "127.0.0.1";
    int fd = ::socket(AF_INET, SOCK_STREAM, 0);
    if (fd < 0) throw ConnError("socket: " + std::string(strerror(errno)));
    int one = 1;
    ::setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    sockaddr_in addr{};
    addr.sin_family = AF_INET;
    addr.sin_port = htons(uint16_t(port));
    if (::inet_pton(AF_INET, host.c_str(), &addr.sin_addr) != 1) {
      ::close(fd);
      throw ConnError("bad host " + host);
    }
    if (::bind(fd, reinterpret_cast<sockaddr*>(&addr), sizeof(addr)) < 0 ||
        ::listen(fd, 128) < 0) {
      int e = errno;
      ::close(fd);
      throw ConnError("bind/listen " + address + ": " + strerror(e));
    }
    socklen_t alen = sizeof(addr);
    ::getsockname(fd, reinterpret_cast<sockaddr*>(&addr), &alen);
    *bound = host + ":" + std::to_string(ntohs(addr.sin_port));
    return fd;
  }

  void accept_loop(int listen_fd) {
    while (!stopping_) {
      int cfd = ::accept(listen_fd, nullptr, nullptr);
      if (cfd < 0) {
        if (errno == EINTR) continue;
        break;  // listener closed
      }
      int one = 1;
      ::setsockopt(cfd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
      h2::tune_socket(cfd);
      auto conn = std::make_shared<Conn>(cfd);
      reap_finished_conns();
      {
        std::lock_guard<std::mutex> lk(conns_mu_);
        if (stopping_) {
          break;
        }
        uint64_t id = ++conn_serial_;
        conns_[id] = conn;
        conn_threads_[id] = std::thread(
            [this, conn, id] { connection_loop(conn, id); });
      }
    }
  }

  void connection_loop(std::shared_ptr<Conn> conn, uint64_t serial) {
    struct SrvStream {
      std::string path;
      HeaderBlock hb;
      bool headers_done = false;
      MsgAssembly body;
      DeviceParse dparse;  // dtor quiesces before body's buffer is freed
    };
    std::unordered_map<uint32_t, SrvStream> streams;
    h2::HpackDecoder decoder;
    uint32_t continuation_stream = 0;

    try {
      uint8_t preface[h2::kPrefaceLen];
      h2::read_full(conn->fd, preface, h2::kPrefaceLen);
      if (std::memcmp(preface, h2::kPreface, h2::kPrefaceLen) != 0)
        throw ConnError("bad client preface");
      conn->send_initial_settings();

      while (!stopping_) {
        FrameHeader fh = h2::read_frame_header(conn->fd);
        switch (fh.type) {
          case h2::F_DATA: {
            auto it = streams.find(fh.stream);
            uint32_t len = fh.length;
            uint8_t pad = 0;
            if (fh.flags & h2::FL_PADDED) {
              h2::read_full(conn->fd, &pad, 1);
              if (len < 1u + pad) throw ConnError("bad padding");
              len -= 1;
            }
            uint32_t body_len = len - pad;
            if (it == streams.end()) {
              h2::discard(conn->fd, len);
            } else {
              it->second.body.feed_from_socket(conn->fd, body_len);
              if (it->second.dparse.enabled)
                device_parse_advance(it->second.dparse, it->second.body);
              if (pad) h2::discard(conn->fd, pad);
            }
            conn->account_received(fh.length);
            if ((fh.flags & h2::FL_END_STREAM) && it != streams.end()) {
              dispatch(conn, fh.stream, it->second);
              streams.erase(it);
            }
            break;
          }
          case h2::F_HEADERS: {
            auto& st = streams[fh.stream];
            read_headers_fragment(conn->fd, fh, &st.hb.block);
            st.hb.end_stream = (fh.flags & h2::FL_END_STREAM) != 0;
            if (fh.flags & h2::FL_END_HEADERS) {
              finish_headers(conn, fh.stream, st, decoder);
              if (st.hb.end_stream) {
                dispatch(conn, fh.stream, st);
                streams.erase(fh.stream);
              }
            } else {
              continuation_stream = fh.stream;
            }
            break;
          }
          case h2::F_CONTINUATION: {
            auto it = streams.find(continuation_stream);
            if (it == streams.end()) throw ConnError("orphan CONTINUATION");
            auto& st = it->second;
            size_t off = st.hb.block.size();
            st.hb.block.resize(off + fh.length);
            h2::read_full(conn->fd,
                          reinterpret_cast<uint8_t*>(&st.hb.block[off]),
                          fh.length);
            if (fh.flags & h2::FL_END_HEADERS) {
              finish_headers(conn, continuation_stream, st, decoder);
              if (st.hb.end_stream) {
                dispatch(conn, continuation_stream, st);
                streams.erase(continuation_stream);
              }
              continuation_stream = 0;
            }
            break;
          }
          case h2::F_SETTINGS: {
            if (fh.flags & h2::FL_ACK) {
              h2::discard(conn->fd, fh.length);
            } else {
              std::vector<uint8_t> payload(fh.length);
              if (fh.length)
                h2::read_full(conn->fd, payload.data(), fh.length);
              conn->apply_peer_settings(payload.data(), fh.length);
              conn->send_settings_ack();
            }
            break;
          }
          case h2::F_PING: {
            uint8_t opaque[8];
            if (fh.length != 8) throw ConnError("bad PING");
            h2::read_full(conn->fd, opaque, 8);
            if (!(fh.flags & h2::FL_ACK)) conn->send_ping_ack(opaque);
            break;
          }
          case h2::F_WINDOW_UPDATE: {
            uint8_t buf4[4];
            if (fh.length != 4) throw ConnError("bad WINDOW_UPDATE");
            h2::read_full(conn->fd, buf4, 4);
            conn->apply_window_update(fh.stream, h2::be32(buf4) & 0x7fffffff);
            break;
          }
          case h2::F_RST_STREAM: {
            h2::discard(conn->fd, fh.length);
            auto it = streams.find(fh.stream);
            if (it != streams.end()) {
              conn->close_send_stream(fh.stream);
              streams.erase(it);
            }
            break;
          }
          case h2::F_GOAWAY:
          case h2::F_PRIORITY:
          case h2::F_PUSH_PROMISE:
          default:
            h2::discard(conn->fd, fh.length);
            break;
        }
      }
    } catch (const std::exception& e) {
      conn->mark_broken(e.what());
    }
    {
      std::lock_guard<std::mutex> lk(conns_mu_);
      conns_.erase(serial);  // fd closes when the last Task releases it
      finished_conns_.push_back(serial);
    }
  }

  template <typename SrvStreamT>
  void finish_headers(const std::shared_ptr<Conn>& conn, uint32_t stream,
                      SrvStreamT& st, h2::HpackDecoder& decoder) {
    auto headers = decoder.decode(
        reinterpret_cast<const uint8_t*>(st.hb.block.data()),
        st.hb.block.size());
    st.hb.block.clear();
    st.hb.done = true;
    st.headers_done = true;
    const std::string* path = find_header(headers, ":path");
    st.path = path ? *path : "";
    conn->open_send_stream(stream);
    int device = -1;
    {
      std::lock_guard<std::mutex> lk(handler_mu_);
      auto it = parsed_paths_.find(st.path);
      if (it != parsed_paths_.end()) device = it->second;
    }
    if (device >= 0) {
      hipStream_t ps = ProspectStreams::instance().get(device);
      if (ps != nullptr) {
        st.dparse.enabled = true;
        st.dparse.device = device;
        st.dparse.stream = ps;
        st.dparse.spec_field = 1;  // request layout
        st.dparse.map_field = 2;
        st.dparse.skip_model = [this](const std::string& name) {
          std::lock_guard<std::mutex> lk(handler_mu_);
          for (auto& kv : echo_models_)
            if (kv.second.count(name)) return true;
          return false;
        };
      }
    }
  }

  template <typename SrvStreamT>
  void dispatch(const std::shared_ptr<Conn>& conn, uint32_t stream,
                SrvStreamT& st) {
    Task t;
    t.conn = conn;
    t.stream = stream;
    t.path = std::move(st.path);
    t.msg = std::move(st.body.msg);
    t.dparse = std::move(st.dparse);
    if (!st.body.have_len) {
      t.msg.alloc(0);  // empty request message (e.g. empty proto)
      t.msg.len = 0;
    }
    {
      std::lock_guard<std::mutex> lk(q_mu_);
      queue_.push_back(std::move(t));
    }
    q_cv_.notify_one();
  }

  void worker_loop() {
    while (true) {
      Task t;
      {
        std::unique_lock<std::mutex> lk(q_mu_);
        q_cv_.wait(lk, [this] { return stopping_ || !queue_.empty(); });
        if (stopping_ && queue_.empty()) return;
        t = std::move(queue_.front());
        queue_.pop_front();
      }
      try {
        handle_request(t);
      } catch (const std::exception&) {
        // connection died mid-response; reader will clean up
      }
    }
  }

  void handle_request(Task& t) {
    // 1) C++ echo fast path (no GIL)
    {
      std::map<std::string, std::set<int64_t>> const* models = nullptr;
      std::map<std::string, std::set<int64_t>> models_copy;
      {
        std::lock_guard<std::mutex> lk(handler_mu_);
        auto it = echo_models_.find(t.path);
        if (it != echo_models_.end()) {
          models_copy = it->second;
          models = &models_copy;
        }
      }
      if (models) {
        try {
          auto parsed =
              tfswire::parse_predict_message(t.msg.p, t.msg.len, true);
          if (echo_eligible(parsed, *models)) {
            auto t0 = std::chrono::steady_clock::now();
            EchoResponse resp = build_echo_response(parsed);
            t.conn->send_headers(t.stream, make_response_headers_block(),
                                 false);
            write_message_with_regions(*t.conn, t.stream, resp.skeleton.p,
                                       resp.skeleton.len, resp.regions,
                                       false);
            t.conn->send_headers(t.stream,
                                 make_trailers_block(GRPC_OK, ""), true);
            t.conn->close_send_stream(t.stream);
            double secs = std::chrono::duration<double>(
                              std::chrono::steady_clock::now() - t0)
                              .count();
            record_stats(t.path, secs, t.msg.len, resp.skeleton.len);
            return;
          }
        } catch (const RpcCallError& e) {
          send_error_response(t, e.code, e.what());
          return;
        } catch (const std::exception& e) {
          send_error_response(t, GRPC_INVALID_ARGUMENT, e.what());
          return;
        }
      }
    }
    // 2) python handler. py::object copies/destruction are refcount ops
    // and MUST happen under the GIL — only an existence check (count()
    // touches no refcounts) outside it; the actual handler reference
    // lives inside the GIL block below.
    bool have_handler;
    {
      std::lock_guard<std::mutex> lk(handler_mu_);
      have_handler = py_handlers_.count(t.path) != 0;
    }
    if (!have_handler) {
      send_error_response(t, GRPC_UNIMPLEMENTED,
                          "unknown service method " + t.path);
      return;
    }
    bool parsed_path;
    {
      std::lock_guard<std::mutex> lk(handler_mu_);
      parsed_path = parsed_paths_.count(t.path) != 0;
    }
    bool have_parse = parsed_path && t.dparse.enabled &&
                      !t.dparse.failed && t.dparse.done;
    t.dparse.quiesce();  // drain copies even for failed/partial prospects
    if (!Py_IsInitialized() || _Py_IsFinalizing()) {
      // interpreter going down (abnormal teardown): acquiring the GIL
      // now is fatal; shed the request instead
      send_error_response(t, GRPC_UNAVAILABLE, "server shutting down");
      return;
    }
    int err_code = 0;
    std::string err_msg;
    py::object result;
    {
      py::gil_scoped_acquire gil;
      py::object fn;
      {
        std::lock_guard<std::mutex> lk(handler_mu_);
        auto it = py_handlers_.find(t.path);
        if (it != py_handlers_.end()) fn = it->second;
      }
      if (!fn) {
        err_code = GRPC_UNIMPLEMENTED;
        err_msg = "service method unregistered: " + t.path;
      } else
      try {
        py::memoryview view = py::memoryview::from_memory(
            t.msg.p, py::ssize_t(t.msg.len));
        if (parsed_path) {
          py::object spec = py::none();
          py::object outs = py::none();
          if (have_parse) {
            record_consumer_stream(t.dparse.outs, t.dparse.device);
            py::dict sd;
            sd["name"] = t.dparse.spec_name;
            sd["version"] = t.dparse.spec_version;
            sd["signature_name"] = t.dparse.spec_signature;
            sd["version_label"] = t.dparse.spec_label;
            py::list filt;
            for (auto& f2 : t.dparse.out_filter) filt.append(py::str(f2));
            sd["output_filter"] = filt;
            py::dict od;
            for (auto& kv : t.dparse.outs)
              od[py::str(kv.first)] = kv.second;
            spec = std::move(sd);
            outs = std::move(od);
          }
          result = fn(view, spec, outs);
        } else {
          result = fn(view);
        }
        // drop tensor refs before the send (outs were copied into python)
        t.dparse.outs.clear();
      } catch (py::error_already_set& e) {
        err_code = GRPC_UNKNOWN;
        try {
          py::object exc = e.value();
          if (py::hasattr(exc, "grpc_code"))
            err_code = exc.attr("grpc_code").cast<int>();
          if (py::hasattr(exc, "grpc_details"))
            err_msg = exc.attr("grpc_details").cast<std::string>();
          else
            err_msg = py::str(exc).cast<std::string>();
        } catch (...) {
          err_msg = "handler error";
        }
        e.restore();
        PyErr_Clear();
      }
    }
    if (err_code != 0) {
      send_error_response(t, err_code, err_msg);
      return;
    }
    // zero-copy send from the python result's buffer; the view pins it.
    // Streaming replies (skeleton + payload regions) take the overlapped
    // region path; plain buffers are sent whole.
    std::unique_ptr<py::buffer_info> info;
    const uint8_t* ptr = nullptr;
    size_t len = 0;
    bool streaming = false;
    std::vector<WireRegion> regions;
    {
      py::gil_scoped_acquire gil;
      try {
        streaming = extract_streaming_reply(result, &info, &ptr, &len,
                                            &regions);
        if (!streaming) {
          info = std::make_unique<py::buffer_info>(
              py::buffer(result).request());
          ptr = static_cast<const uint8_t*>(info->ptr);
          len = size_t(info->size) * size_t(info->itemsize);
        }
      } catch (...) {
        info.reset();
        ptr = nullptr;
      }
    }
    if (!ptr) {
      send_error_response(t, GRPC_INTERNAL,
                          "handler returned a non-buffer object");
    } else {
      try {
        if (streaming) {
          t.conn->send_headers(t.stream, make_response_headers_block(),
                               false);
          write_message_with_regions(*t.conn, t.stream, ptr, len, regions,
                                     false);
          t.conn->send_headers(t.stream, make_trailers_block(GRPC_OK, ""),
                               true);
          t.conn->close_send_stream(t.stream);
        } else {
          send_ok_response(t, ptr, len);
        }
      } catch (...) {
        py::gil_scoped_acquire gil;
        info.reset();
        result = py::object();
        throw;
      }
    }
    py::gil_scoped_acquire gil;
    info.reset();
    result = py::object();
  }

  void send_ok_response(Task& t, const uint8_t* data, size_t n) {
    t.conn->send_headers(t.stream, make_response_headers_block(), false);
    t.conn->send_data_message(t.stream, data, n, false);
    t.conn->send_headers(t.stream, make_trailers_block(GRPC_OK, ""), true);
    t.conn->close_send_stream(t.stream);
  }

  void send_error_response(Task& t, int code, const std::string& msg) {
    t.conn->send_headers(t.stream, make_trailers_only_block(code, msg),
                         true);
    t.conn->close_send_stream(t.stream);
  }

  void stop_internal(bool wait) {
    bool was_running = running_.exchange(false);
    stopping_ = true;
    for (int fd : listen_fds_) {
      ::shutdown(fd, SHUT_RDWR);
      ::close(fd);
    }
    listen_fds_.clear();
    {
      std::lock_guard<std::mutex> lk(conns_mu_);
      for (auto& kv : conns_) kv.second->mark_broken("server stopping");
    }
    q_cv_.notify_all();
    if (!was_running && !wait) return;
    for (auto& th : accept_threads_)
      if (th.joinable()) th.join();
    accept_threads_.clear();
    {
      std::map<uint64_t, std::thread> threads;
      {
        std::lock_guard<std::mutex> lk(conns_mu_);
        threads.swap(conn_threads_);
      }
      for (auto& kv : threads)
        if (kv.second.joinable()) kv.second.join();
      std::lock_guard<std::mutex> lk(conns_mu_);
      conns_.clear();
      finished_conns_.clear();
    }
    for (auto& w : workers_)
      if (w.joinable()) w.join();
    workers_.clear();
    for (auto& up : unix_paths_) ::unlink(up.c_str());
    unix_paths_.clear();
    // release python handlers with the GIL held
    if (Py_IsInitialized()) {
      py::gil_scoped_acquire gil;
      py_handlers_.clear();
    }
  }
};

// ===========================================================================
// Client channel
// ===========================================================================

class GrpcChannel {
 public:
  explicit GrpcChannel(const std::string& target,
                       std::string authority = "")
      : authority_(std::move(authority)) {
    if (authority_.empty()) {
      authority_ = target.rfind("unix:", 0) == 0 ? "localhost" : target;
    }
    int fd = h2::connect_target(target);
    conn_ = std::make_shared<Conn>(fd);
    h2::write_all(fd, reinterpret_cast<const uint8_t*>(h2::kPreface),
                  h2::kPrefaceLen);
    conn_->send_initial_settings();
    reader_ = std::thread([this] { reader_loop(); });
  }

  ~GrpcChannel() { close(); }

  void close() {
    bool was = closed_.exchange(true);
    if (was) return;
    conn_->mark_broken("channel closed");
    if (reader_.joinable()) reader_.join();
    fail_all_pending(GRPC_UNAVAILABLE, "channel closed");
  }

  // opens a new stream and sends its HEADERS; shared by both call styles
  uint32_t begin_stream(const std::string& path, double timeout_s) {
    auto p = std::make_shared<Pending>();
    uint32_t id;
    {
      std::unique_lock<std::mutex> lk(mu_);
      // respect peer MAX_CONCURRENT_STREAMS
      cv_.wait(lk, [&] {
        int64_t maxs;
        {
          std::lock_guard<std::mutex> flk(conn_->fc_mu);
          maxs = conn_->peer_max_streams;
          if (conn_->broken) return true;
        }
        return maxs < 0 || int64_t(pending_.size()) < maxs;
      });
      {
        std::lock_guard<std::mutex> flk(conn_->fc_mu);
        if (conn_->broken)
          throw RpcCallError(GRPC_UNAVAILABLE,
                             "channel broken: " + conn_->broken_why);
      }
      id = next_stream_;
      next_stream_ += 2;
      streams_started_.fetch_add(1, std::memory_order_relaxed);
      pending_[id] = p;
      conn_->open_send_stream(id);
      // HEADERS must hit the wire in stream-id order: send under mu_
      std::string block = make_request_headers(path, timeout_s);
      try {
        conn_->send_headers(id, block, false);
      } catch (const std::exception& e) {
        pending_.erase(id);
        conn_->close_send_stream(id);
        throw RpcCallError(GRPC_UNAVAILABLE, e.what());
      }
    }
    return id;
  }

  // starts a unary call; returns the stream id used as a handle
  uint32_t start_call(const std::string& path, const uint8_t* data,
                      size_t len, double timeout_s) {
    uint32_t id = begin_stream(path, timeout_s);
    try {
      conn_->send_data_message(id, data, len, true);
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> lk(mu_);
      pending_.erase(id);
      conn_->close_send_stream(id);
      throw RpcCallError(GRPC_UNAVAILABLE, e.what());
    }
    return id;
  }

  // streaming variant: the request payload is a skeleton plus regions
  // (see write_message_with_regions) — device regions overlap DMA with
  // the send, host regions go out zero-copy straight from tensor memory
  // borrowed immortal prospect stream (see ProspectStreams); nullptr
  // when the device is unavailable (caller falls back to plain receive)
  hipStream_t device_stream(int dev) {
    return ProspectStreams::instance().get(dev);
  }

  uint32_t start_call_streaming(const std::string& path, const uint8_t* buf,
                                size_t len,
                                const std::vector<WireRegion>& regions,
                                double timeout_s, int parse_device = -1) {
    uint32_t id = begin_stream(path, timeout_s);
    if (parse_device >= 0) {
      hipStream_t ds = device_stream(parse_device);
      if (ds != nullptr) {
        auto p = find_pending(id);
        if (p) {
          std::lock_guard<std::mutex> lk(p->m);
          p->dparse.enabled = true;
          p->dparse.device = parse_device;
          p->dparse.stream = ds;
        }
      }
    }
    try {
      write_message_with_regions(*conn_, id, buf, len, regions, true);
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> lk(mu_);
      pending_.erase(id);
      conn_->close_send_stream(id);
      throw RpcCallError(GRPC_UNAVAILABLE, e.what());
    }
    return id;
  }

  struct ParsedResult {
    Buf resp;
    bool parsed_ok = false;
    std::vector<std::pair<std::string, at::Tensor>> outs;
  };

  // wait() variant for device-parse calls: quiesces the copy stream in
  // EVERY exit path (in-flight H2D references the response buffer) and
  // hands back the prospected device tensors when the full message
  // parsed canonically.
  ParsedResult wait_parsed(uint32_t id, double timeout_s) {
    std::shared_ptr<Pending> p;
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto it = pending_.find(id);
      if (it == pending_.end())
        throw RpcCallError(GRPC_INTERNAL, "unknown call handle");
      p = it->second;
    }
    auto quiesce = [&] {
      std::lock_guard<std::mutex> lk(p->m);
      if (p->dparse.enabled && p->dparse.stream != nullptr)
        (void)hipStreamSynchronize(p->dparse.stream);
    };
    std::unique_lock<std::mutex> lk(p->m);
    bool ok = true;
    if (timeout_s > 0) {
      ok = p->cv.wait_for(lk, std::chrono::duration<double>(timeout_s),
                          [&] { return p->done; });
    } else {
      p->cv.wait(lk, [&] { return p->done; });
    }
    if (!ok) {
      lk.unlock();
      quiesce();
      {
        std::lock_guard<std::mutex> glk(mu_);
        pending_.erase(id);
      }
      try {
        conn_->send_rst_stream(id, 8 /* CANCEL */);
      } catch (...) {
      }
      conn_->close_send_stream(id);
      cv_.notify_all();
      throw RpcCallError(GRPC_DEADLINE_EXCEEDED, "Deadline Exceeded");
    }
    ParsedResult r;
    r.resp = std::move(p->body.msg);
    int status = p->grpc_status;
    std::string msg = p->message;
    bool parsed = p->dparse.enabled && !p->dparse.failed && p->dparse.done;
    if (parsed) r.outs = std::move(p->dparse.outs);
    bool need_sync = p->dparse.enabled && p->dparse.stream != nullptr;
    hipStream_t ds = p->dparse.stream;
    lk.unlock();
    if (need_sync && hipStreamSynchronize(ds) != hipSuccess) parsed = false;
    if (parsed) record_consumer_stream(r.outs, r.outs.empty() ? 0 :
        r.outs.front().second.get_device());
    {
      std::lock_guard<std::mutex> glk(mu_);
      pending_.erase(id);
    }
    conn_->close_send_stream(id);
    cv_.notify_all();
    if (status != GRPC_OK)
      throw RpcCallError(status < 0 ? GRPC_INTERNAL : status, msg);
    r.parsed_ok = parsed;
    return r;
  }

  // streams opened on this channel so far (read-only diagnostic: shows
  // how requests spread over a multi-channel client)
  uint64_t streams_started() const {
    return streams_started_.load(std::memory_order_relaxed);
  }

  Buf wait(uint32_t id, double timeout_s) {
    std::shared_ptr<Pending> p;
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto it = pending_.find(id);
      if (it == pending_.end())
        throw RpcCallError(GRPC_INTERNAL, "unknown call handle");
      p = it->second;
    }
    std::unique_lock<std::mutex> lk(p->m);
    bool ok = true;
    if (timeout_s > 0) {
      ok = p->cv.wait_for(lk, std::chrono::duration<double>(timeout_s),
                          [&] { return p->done; });
    } else {
      p->cv.wait(lk, [&] { return p->done; });
    }
    if (!ok) {
      lk.unlock();
      {
        std::lock_guard<std::mutex> glk(mu_);
        pending_.erase(id);
      }
      try {
        conn_->send_rst_stream(id, 8 /* CANCEL */);
      } catch (...) {
      }
      conn_->close_send_stream(id);
      cv_.notify_all();
      throw RpcCallError(GRPC_DEADLINE_EXCEEDED, "Deadline Exceeded");
    }
    Buf resp = std::move(p->body.msg);
    int status = p->grpc_status;
    std::string msg = p->message;
    lk.unlock();
    {
      std::lock_guard<std::mutex> glk(mu_);
      pending_.erase(id);
    }
    conn_->close_send_stream(id);
    cv_.notify_all();
    if (status != GRPC_OK)
      throw RpcCallError(status < 0 ? GRPC_INTERNAL : status, msg);
    return resp;
  }

 private:
  struct Pending {
    std::mutex m;
    std::condition_variable cv;
    bool done = false;
    int grpc_status = -1;
    std::string message;
    std::vector<h2::Header> resp_headers;
    HeaderBlock hb;
    MsgAssembly body;
    DeviceParse dparse;
  };

  std::shared_ptr<Conn> conn_;
  std::thread reader_;
  std::string authority_;
  std::atomic<bool> closed_{false};
  std::mutex mu_;
  std::condition_variable cv_;
  std::unordered_map<uint32_t, std::shared_ptr<Pending>> pending_;
  uint32_t next_stream_ = 1;
  std::atomic<uint64_t> streams_started_{0};

  std::string make_request_headers(const std::string& path,
                                   double timeout_s) {
    h2::HpackEncoder enc;
    std::string block;
    enc.add_indexed(&block, 3);  // :method: POST
    enc.add_indexed(&block, 6);  // :scheme: http
    enc.add_literal(&block, 4, path, true);  // :path (huffman if shorter)
    enc.add_literal(&block, 1, authority_);  // :authority
    enc.add_literal(&block, "te", "trailers");
    enc.add_literal(&block, 31, "application/grpc");  // content-type
    if (timeout_s > 0) {
      long ms = long(timeout_s * 1000.0);
      if (ms < 1) ms = 1;
      enc.add_literal(&block, "grpc-timeout", std::to_string(ms) + "m");
    }
    return block;
  }

  std::shared_ptr<Pending> find_pending(uint32_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = pending_.find(id);
    return it == pending_.end() ? nullptr : it->second;
  }

  void complete(const std::shared_ptr<Pending>& p, int status,
                std::string msg) {
    {
      std::lock_guard<std::mutex> lk(p->m);
      if (p->done) return;
      p->grpc_status = status;
      p->message = std::move(msg);
      p->done = true;
    }
    p->cv.notify_all();
  }

  void fail_all_pending(int status, const std::string& msg) {
    std::vector<std::shared_ptr<Pending>> ps;
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (auto& kv : pending_) ps.push_back(kv.second);
    }
    for (auto& p : ps) complete(p, status, msg);
    cv_.notify_all();
  }

  void process_headers(uint32_t stream, const std::shared_ptr<Pending>& p,
                       std::vector<h2::Header>&& headers, bool end_stream) {
    const std::string* gs = find_header(headers, "grpc-status");
    if (gs != nullptr || end_stream) {
      int status = GRPC_UNKNOWN;
      std::string msg = "missing grpc-status";
      if (gs) {
        status = std::atoi(gs->c_str());
        const std::string* gm = find_header(headers, "grpc-message");
        msg = gm ? h2::percent_decode(*gm) : "";
      }
      complete(p, status, std::move(msg));
    } else {
      std::lock_guard<std::mutex> lk(p->m);
      p->resp_headers = std::move(headers);
    }
  }

  void reader_loop() {
    h2::HpackDecoder decoder;
    uint32_t continuation_stream = 0;
    try {
      while (true) {
        FrameHeader fh = h2::read_frame_header(conn_->fd);
        switch (fh.type) {
          case h2::F_DATA: {
            auto p = find_pending(fh.stream);
            uint32_t len = fh.length;
            uint8_t pad = 0;
            if (fh.flags & h2::FL_PADDED) {
              h2::read_full(conn_->fd, &pad, 1);
              if (len < 1u + pad) throw ConnError("bad padding");
              len -= 1;
            }
            uint32_t body_len = len - pad;
            if (!p) {
              h2::discard(conn_->fd, len);
            } else {
              std::lock_guard<std::mutex> lk(p->m);
              p->body.feed_from_socket(conn_->fd, body_len);
              if (p->dparse.enabled)
                device_parse_advance(p->dparse, p->body);
              if (pad) h2::discard(conn_->fd, pad);
            }
            conn_->account_received(fh.length);
            if ((fh.flags & h2::FL_END_STREAM) && p)
              complete(p, GRPC_UNKNOWN, "stream ended without trailers");
            break;
          }
          case h2::F_HEADERS: {
            auto p = find_pending(fh.stream);
            HeaderBlock hb;
            std::string* block_dst = p ? &p->hb.block : &hb.block;
            {
              FrameHeader tmp = fh;
              read_headers_fragment(conn_->fd, tmp, block_dst);
            }
            bool end_stream = (fh.flags & h2::FL_END_STREAM) != 0;
            if (p) p->hb.end_stream = end_stream;
            if (fh.flags & h2::FL_END_HEADERS) {
              auto headers = decoder.decode(
                  reinterpret_cast<const uint8_t*>(block_dst->data()),
                  block_dst->size());
              block_dst->clear();
              if (p)
                process_headers(fh.stream, p, std::move(headers),
                                end_stream);
            } else {
              continuation_stream = fh.stream;
            }
            break;
          }
          case h2::F_CONTINUATION: {
            auto p = find_pending(continuation_stream);
            std::string scratch;
            std::string* block_dst = p ? &p->hb.block : &scratch;
            size_t off = block_dst->size();
            block_dst->resize(off + fh.length);
            h2::read_full(conn_->fd,
                          reinterpret_cast<uint8_t*>(&(*block_dst)[off]),
                          fh.length);
            if (fh.flags & h2::FL_END_HEADERS) {
              auto headers = decoder.decode(
                  reinterpret_cast<const uint8_t*>(block_dst->data()),
                  block_dst->size());
              block_dst->clear();
              if (p)
                process_headers(continuation_stream, p, std::move(headers),
                                p->hb.end_stream);
              continuation_stream = 0;
            }
            break;
          }
          case h2::F_SETTINGS: {
            if (fh.flags & h2::FL_ACK) {
              h2::discard(conn_->fd, fh.length);
            } else {
              std::vector<uint8_t> payload(fh.length);
              if (fh.length)
                h2::read_full(conn_->fd, payload.data(), fh.length);
              conn_->apply_peer_settings(payload.data(), fh.length);
              conn_->send_settings_ack();
            }
            break;
          }
          case h2::F_PING: {
            uint8_t opaque[8];
            if (fh.length != 8) throw ConnError("bad PING");
            h2::read_full(conn_->fd, opaque, 8);
            if (!(fh.flags & h2::FL_ACK)) conn_->send_ping_ack(opaque);
            break;
          }
          case h2::F_WINDOW_UPDATE: {
            uint8_t buf4[4];
            if (fh.length != 4) throw ConnError("bad WINDOW_UPDATE");
            h2::read_full(conn_->fd, buf4, 4);
            conn_->apply_window_update(fh.stream,
                                       h2::be32(buf4) & 0x7fffffff);
            break;
          }
          case h2::F_RST_STREAM: {
            uint8_t buf4[4];
            if (fh.length != 4) throw ConnError("bad RST_STREAM");
            h2::read_full(conn_->fd, buf4, 4);
            auto p = find_pending(fh.stream);
            if (p)
              complete(p, GRPC_UNAVAILABLE,
                       "stream reset by server (http2 code " +
                           std::to_string(h2::be32(buf4)) + ")");
            break;
          }
          case h2::F_GOAWAY:
          default:
            h2::discard(conn_->fd, fh.length);
            break;
        }
      }
    } catch (const std::exception& e) {
      conn_->mark_broken(e.what());
      fail_all_pending(GRPC_UNAVAILABLE,
                       std::string("connection lost: ") + e.what());
    }
  }
};

// ===========================================================================
// Sharded Predict: one native call per logical request
// ===========================================================================
// TurboPredictClient.predict_sharded used to orchestrate every shard from
// python: per shard one serialize call, one stream synchronize, one
// thread-pool job and one wait, all trading the GIL with the other
// in-flight requests. Here the whole request runs behind ONE GIL release:
// plan the shards (sharded.h), synchronize the producer stream once, send
// the shards in parallel (caller thread + persistent sender pool), wait
// for every reply and concatenate the device-parsed outputs. No new
// socket, framing or receive code: only start_call_streaming / wait /
// wait_parsed are orchestrated.

inline int scalar_to_tf_dtype(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return 1;
    case at::kDouble: return 2;
    case at::kInt: return 3;
    case at::kByte: return 4;
    case at::kShort: return 5;
    case at::kChar: return 6;
    case at::kComplexFloat: return 8;
    case at::kLong: return 9;
    case at::kBool: return 10;
    case at::kBFloat16: return 14;
    case at::kUInt16: return 17;
    case at::kComplexDouble: return 18;
    case at::kHalf: return 19;
    case at::kUInt32: return 22;
    case at::kUInt64: return 23;
    default:
      throw std::invalid_argument("unsupported torch dtype for TensorProto");
  }
}

// Persistent pool of tfsshard::kSenderPoolSize threads that run blocking
// shard sends. Created lazily on first use, never per call; its threads
// never touch python. shutdown() takes the threads out under the lock and
// joins them outside it (queued jobs are drained first); a later submit
// simply starts a fresh set, so one client's close() cannot strand
// another client's request.
class SenderPool {
 public:
  static SenderPool& instance() {
    static SenderPool* pool = new SenderPool();  // leaked: immortal
    return *pool;
  }

  // false while shutting down: the caller then runs the job itself
  bool submit(std::function<void()> job) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (stopping_) return false;
      if (threads_.empty())
        for (int i = 0; i < tfsshard::kSenderPoolSize; ++i)
          threads_.emplace_back([this] { loop(); });
      queue_.push_back(std::move(job));
    }
    cv_.notify_one();
    return true;
  }

  void shutdown() {
    std::vector<std::thread> threads;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (threads_.empty()) return;
      stopping_ = true;
      threads.swap(threads_);
    }
    cv_.notify_all();
    for (auto& t : threads)
      if (t.joinable()) t.join();
    std::lock_guard<std::mutex> lk(mu_);
    stopping_ = false;
  }

 private:
  void loop() {
    for (;;) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return stopping_ || !queue_.empty(); });
        if (queue_.empty()) return;  // stopping and drained
        job = std::move(queue_.front());
        queue_.pop_front();
      }
      job();  // jobs record their own errors; they never throw
    }
  }

  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> queue_;
  std::vector<std::thread> threads_;
  bool stopping_ = false;
};

std::atomic<uint32_t> g_shard_rotation{0};

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now() - t0)
      .count();
}

// Shared between the calling thread and the sender-pool jobs of one
// request. Every shard is sent by whoever CLAIMS it first: the pool jobs
// claim theirs when a pool thread picks them up, and the caller — after
// sending shard 0 — claims whatever is still unclaimed, so a saturated
// (or stopping) pool delays nothing and cannot deadlock a request.
struct ShardedCall {
  struct Shard {
    tfsshard::ShardPlan plan;
    std::vector<WireRegion> regions;
    GrpcChannel* ch = nullptr;
    std::atomic<bool> claimed{false};
    bool started = false;
    uint32_t id = 0;
    std::exception_ptr err;
    double send_start_ms = 0.0, send_ms = 0.0;
  };

  std::string path;
  double timeout = 0.0;
  int parse_device = -1;
  std::chrono::steady_clock::time_point t0;
  std::vector<Shard> shards;
  std::mutex m;
  std::condition_variable cv;
  size_t sends_pending = 0;

  explicit ShardedCall(size_t n) : shards(n), sends_pending(n) {}

  // true when this thread won the shard and sent it (or recorded its error)
  bool try_send(size_t i) {
    Shard& s = shards[i];
    if (s.claimed.exchange(true)) return false;
    s.send_start_ms = ms_since(t0);
    try {
      s.id = s.ch->start_call_streaming(path, s.plan.skeleton.get(),
                                        s.plan.size, s.regions,
                                        timeout, parse_device);
      s.started = true;
    } catch (...) {
      s.err = std::current_exception();
    }
    s.send_ms = ms_since(t0) - s.send_start_ms;
    std::lock_guard<std::mutex> lk(m);
    --sends_pending;
    cv.notify_all();
    return true;
  }

  void wait_sends() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [this] { return sends_pending == 0; });
  }
};

struct ShardedResult {
  bool merged = false;
  std::vector<std::pair<std::string, at::Tensor>> outs;  // merged == true
  std::vector<GrpcChannel::ParsedResult> parts;          // merged == false
};

// Runs WITHOUT the GIL. `contig` (kept alive by the caller for the whole
// call) backs every region pointer in `inputs`.
ShardedResult run_predict_sharded(
    const std::vector<GrpcChannel*>& channels, const std::string& path,
    const std::string& model_name, int64_t version,
    const std::string& signature, const std::vector<std::string>& names,
    const std::vector<tfsshard::Input>& inputs,
    const std::vector<int>& input_devices, int shards, int parse_device,
    double timeout) {
  static const char* trace_path = std::getenv("MI355X_SHARDED_TRACE");
  const auto t0 = std::chrono::steady_clock::now();
  const size_t n = size_t(shards);
  auto call = std::make_shared<ShardedCall>(n);
  call->path = path;
  call->timeout = timeout;
  call->parse_device = parse_device;
  call->t0 = t0;

  // plan: per-shard skeleton + regions, and the request's channels
  const auto sizes = tfsshard::shard_sizes(inputs[0].shape[0], shards);
  const uint32_t n_ch = uint32_t(channels.size());
  const uint32_t start =
      tfsshard::next_start_channel(g_shard_rotation, n_ch, uint32_t(shards));
  int64_t row = 0;
  for (size_t i = 0; i < n; ++i) {
    auto& s = call->shards[i];
    s.plan = tfsshard::plan_shard(model_name, version, signature, names,
                                  inputs, row, sizes[i]);
    row += sizes[i];
    s.regions.reserve(s.plan.regions.size());
    for (const auto& r : s.plan.regions)
      s.regions.push_back(WireRegion{r.offset, r.nbytes, r.ptr, r.device});
    s.ch = channels[tfsshard::shard_channel(start, uint32_t(i), n_ch)];
  }
  const double plan_ms = ms_since(t0);

  // producer ordering: the staging DMA must see everything the CALLER's
  // current stream has queued on the inputs — one host sync per input
  // device per request, on the caller's own thread
  for (int dev : input_devices) {
    hipStream_t cur = c10::hip::getCurrentHIPStream(
                          static_cast<c10::DeviceIndex>(dev))
                          .stream();
    if (hipStreamSynchronize(cur) != hipSuccess)
      throw RpcCallError(GRPC_INTERNAL,
                         "producer stream synchronize failed");
  }
  const double sync_ms = ms_since(t0) - plan_ms;

  // sends: shard 0 here, the rest offered to the pool (and reclaimed by
  // this thread if the pool has not picked them up by then)
  for (size_t i = 1; i < n; ++i)
    (void)SenderPool::instance().submit([call, i] { call->try_send(i); });
  for (size_t i = 0; i < n; ++i) call->try_send(i);
  call->wait_sends();
  const double sends_done_ms = ms_since(t0);

  // completion: EVERY started stream is waited on (wait/wait_parsed RST
  // the stream and quiesce its copy stream on deadline) before the first
  // error is rethrown
  ShardedResult res;
  res.parts.resize(n);
  std::exception_ptr first_err;
  for (size_t i = 0; i < n; ++i) {
    auto& s = call->shards[i];
    if (!s.started) {
      if (!first_err) first_err = s.err;
      continue;
    }
    double remaining = 0.0;
    if (timeout > 0) {
      remaining = timeout - ms_since(t0) * 1e-3;
      if (remaining < 1e-3) remaining = 1e-3;
    }
    try {
      if (parse_device >= 0) {
        res.parts[i] = s.ch->wait_parsed(s.id, remaining);
      } else {
        res.parts[i].resp = s.ch->wait(s.id, remaining);
      }
    } catch (...) {
      if (!first_err) first_err = std::current_exception();
    }
  }
  const double wait_ms = ms_since(t0) - sends_done_ms;
  if (first_err) {
    res.parts.clear();
    try {
      std::rethrow_exception(first_err);
    } catch (const RpcCallError&) {
      throw;
    } catch (const std::exception& e) {
      throw RpcCallError(GRPC_INTERNAL, e.what());
    }
  }

  // merge: only when every shard was device-parsed with the same outputs
  const auto t_merge = std::chrono::steady_clock::now();
  bool all_parsed = parse_device >= 0;
  for (auto& p : res.parts) all_parsed = all_parsed && p.parsed_ok;
  if (all_parsed) {
    const auto& first = res.parts[0].outs;
    for (auto& p : res.parts) {
      all_parsed = all_parsed && p.outs.size() == first.size();
      for (size_t k = 0; all_parsed && k < first.size(); ++k)
        all_parsed = p.outs[k].first == first[k].first;
    }
  }
  if (all_parsed) {
    const auto& first = res.parts[0].outs;
    for (size_t k = 0; k < first.size(); ++k) {
      if (first[k].second.dim() == 0) {
        res.outs.emplace_back(first[k].first, first[k].second);
        continue;
      }
      std::vector<at::Tensor> pieces;
      pieces.reserve(n);
      for (auto& p : res.parts) pieces.push_back(p.outs[k].second);
      // on the caller's current stream; wait_parsed recorded that stream
      // on every piece, so the allocator orders their reuse after the cat
      res.outs.emplace_back(first[k].first, at::cat(pieces, 0));
    }
    res.merged = true;
    res.parts.clear();
  }

  if (trace_path) {
    // one JSON line per request (diagnostic; same style as
    // MI355X_STAGING_TRACE)
    std::string line = "{\"shards\": " + std::to_string(n) +
                       ", \"start_channel\": " + std::to_string(start) +
                       ", \"plan_ms\": " + std::to_string(plan_ms) +
                       ", \"sync_ms\": " + std::to_string(sync_ms) +
                       ", \"send_start_ms\": [";
    for (size_t i = 0; i < n; ++i)
      line += (i ? "," : "") + std::to_string(call->shards[i].send_start_ms);
    line += "], \"send_ms\": [";
    for (size_t i = 0; i < n; ++i)
      line += (i ? "," : "") + std::to_string(call->shards[i].send_ms);
    line += "], \"sends_done_ms\": " + std::to_string(sends_done_ms) +
            ", \"wait_ms\": " + std::to_string(wait_ms) +
            ", \"merge_ms\": " + std::to_string(ms_since(t_merge)) +
            ", \"merged\": " + (res.merged ? "true" : "false") +
            ", \"total_ms\": " + std::to_string(ms_since(t0)) + "}\n";
    FILE* f = std::fopen(trace_path, "a");
    if (f) {
      std::fputs(line.c_str(), f);
      std::fclose(f);
    }
  }
  return res;
}

}  // namespace

// ===========================================================================
// bindings
// ===========================================================================

PYBIND11_MODULE(_transport, m) {
  m.doc() = "Native gRPC (HTTP/2) transport for the MI355X serving stack";

  py::class_<OwnedBuf>(m, "OwnedBuf", py::buffer_protocol())
      .def_buffer([](OwnedBuf& b) -> py::buffer_info {
        return py::buffer_info(b.buf.p, 1,
                               py::format_descriptor<uint8_t>::format(),
                               1, {py::ssize_t(b.buf.len)}, {py::ssize_t(1)},
                               true /* readonly */);
      })
      .def("__len__", [](const OwnedBuf& b) { return b.buf.len; })
      .def("tobytes", [](const OwnedBuf& b) {
        return py::bytes(reinterpret_cast<const char*>(b.buf.p), b.buf.len);
      });

  // exception type with .code_int / .details attributes
  static py::object rpc_error_cls = [&m]() {
    py::dict ns;
    py::exec(R"(
class NativeRpcError(Exception):
    """gRPC call failure from the native transport (code_int, details)."""
    def __init__(self, code, details):
        super().__init__(code, details)
        self.code_int = code
        self.details = details
)",
             ns, ns);
    py::object cls = ns["NativeRpcError"];
    m.attr("NativeRpcError") = cls;
    return cls;
  }();

  py::register_exception_translator([](std::exception_ptr ep) {
    try {
      if (ep) std::rethrow_exception(ep);
    } catch (const RpcCallError& e) {
      py::object exc = rpc_error_cls(e.code, e.what());
      PyErr_SetObject(rpc_error_cls.ptr(), exc.ptr());
    }
  });

  py::class_<GrpcServer>(m, "GrpcServer")
      .def(py::init<std::string, int>(), py::arg("address"),
           py::arg("workers") = 8)
      .def("start", &GrpcServer::start,
           py::call_guard<py::gil_scoped_release>())
      .def("register_handler", &GrpcServer::register_handler,
           py::arg("path"), py::arg("fn"))
      .def("register_handler_parsed", &GrpcServer::register_handler_parsed,
           py::arg("path"), py::arg("fn"), py::arg("device"),
           "Like register_handler, but fn is called as fn(view, spec, "
           "outs): requests are prospected while streaming in and their "
           "tensor_content spans H2D'd to `device`; spec/outs are None "
           "when the request was non-canonical.")
      .def("add_address", &GrpcServer::add_address, py::arg("address"),
           "Add an extra listen address (call before start()).")
      .def("set_echo_models", &GrpcServer::set_echo_models, py::arg("path"),
           py::arg("models"),
           "Enable the all-C++ identity-echo fast path for `path` for the "
           "given {model_name: {versions}} table (empty dict disables).",
           py::call_guard<py::gil_scoped_release>())
      .def("stop", &GrpcServer::stop,
           py::call_guard<py::gil_scoped_release>())
      .def("stats", &GrpcServer::stats,
           "Per-path counters/latency samples for requests handled "
           "entirely in C++ (echo fast path).");

  py::class_<GrpcChannel>(m, "GrpcChannel")
      .def(py::init<const std::string&, std::string>(), py::arg("target"),
           py::arg("authority") = "")
      .def(
          "call",
          [](GrpcChannel& ch, const std::string& path, py::buffer data,
             double timeout) {
            py::buffer_info info = data.request();
            const uint8_t* ptr = static_cast<const uint8_t*>(info.ptr);
            size_t len = size_t(info.size) * size_t(info.itemsize);
            py::gil_scoped_release release;
            uint32_t id = ch.start_call(path, ptr, len, timeout);
            Buf resp = ch.wait(id, timeout);
            return OwnedBuf(std::move(resp));
          },
          py::arg("path"), py::arg("data"), py::arg("timeout") = 0.0)
      .def(
          "call_streaming",
          [](GrpcChannel& ch, const std::string& path, py::buffer data,
             py::list region_list, double timeout) {
            py::buffer_info info = data.request();
            const uint8_t* ptr = static_cast<const uint8_t*>(info.ptr);
            size_t len = size_t(info.size) * size_t(info.itemsize);
            std::vector<WireRegion> regions;
            regions.reserve(py::len(region_list));
            for (auto item : region_list) {
              auto t = py::reinterpret_borrow<py::tuple>(item);
              regions.push_back(WireRegion{
                  t[0].cast<size_t>(), t[1].cast<size_t>(),
                  uintptr_t(t[2].cast<uint64_t>()), t[3].cast<bool>()});
            }
            py::gil_scoped_release release;
            uint32_t id =
                ch.start_call_streaming(path, ptr, len, regions, timeout);
            Buf resp = ch.wait(id, timeout);
            return OwnedBuf(std::move(resp));
          },
          py::arg("path"), py::arg("data"), py::arg("regions"),
          py::arg("timeout") = 0.0,
          "Unary call whose request payload is a skeleton buffer plus "
          "(offset, nbytes, ptr, is_device) regions: device regions "
          "overlap staging DMA with the send; host regions are sent "
          "zero-copy from tensor memory. Caller must keep region memory "
          "alive for the duration of the call.")
      .def(
          "call_streaming_parsed",
          [](GrpcChannel& ch, const std::string& path, py::buffer data,
             py::list region_list, int parse_device, double timeout) {
            py::buffer_info info = data.request();
            const uint8_t* ptr = static_cast<const uint8_t*>(info.ptr);
            size_t len = size_t(info.size) * size_t(info.itemsize);
            std::vector<WireRegion> regions;
            regions.reserve(py::len(region_list));
            for (auto item : region_list) {
              auto t = py::reinterpret_borrow<py::tuple>(item);
              regions.push_back(WireRegion{
                  t[0].cast<size_t>(), t[1].cast<size_t>(),
                  uintptr_t(t[2].cast<uint64_t>()), t[3].cast<bool>()});
            }
            GrpcChannel::ParsedResult r;
            {
              py::gil_scoped_release release;
              uint32_t id = ch.start_call_streaming(path, ptr, len, regions,
                                                    timeout, parse_device);
              r = ch.wait_parsed(id, timeout);
            }
            py::object outs = py::none();
            if (r.parsed_ok) {
              py::dict d;
              for (auto& kv : r.outs) d[py::str(kv.first)] = kv.second;
              outs = std::move(d);
            }
            return py::make_tuple(outs, OwnedBuf(std::move(r.resp)));
          },
          py::arg("path"), py::arg("data"), py::arg("regions"),
          py::arg("parse_device"), py::arg("timeout") = 0.0,
          "call_streaming + receive-side progressive unpack: the reader "
          "issues async H2D for tensor_content spans while the response "
          "is still arriving. Returns ({name: device tensor}, raw buf); "
          "the dict is None when the response was non-canonical — parse "
          "the raw buffer instead.")
      .def(
          "wait_parsed",
          [](GrpcChannel& ch, uint32_t id, double timeout) {
            GrpcChannel::ParsedResult r;
            {
              py::gil_scoped_release release;
              r = ch.wait_parsed(id, timeout);
            }
            py::object outs = py::none();
            if (r.parsed_ok) {
              py::dict d;
              for (auto& kv : r.outs) d[py::str(kv.first)] = kv.second;
              outs = std::move(d);
            }
            return py::make_tuple(outs, OwnedBuf(std::move(r.resp)));
          },
          py::arg("id"), py::arg("timeout") = 0.0,
          "wait() for calls started with parse_device >= 0: returns "
          "({name: device tensor} | None, raw buf).")
      .def(
          "start_streaming",
          [](GrpcChannel& ch, const std::string& path, py::buffer data,
             py::list region_list, double timeout, int parse_device) {
            py::buffer_info info = data.request();
            const uint8_t* ptr = static_cast<const uint8_t*>(info.ptr);
            size_t len = size_t(info.size) * size_t(info.itemsize);
            std::vector<WireRegion> regions;
            regions.reserve(py::len(region_list));
            for (auto item : region_list) {
              auto t = py::reinterpret_borrow<py::tuple>(item);
              regions.push_back(WireRegion{
                  t[0].cast<size_t>(), t[1].cast<size_t>(),
                  uintptr_t(t[2].cast<uint64_t>()), t[3].cast<bool>()});
            }
            py::gil_scoped_release release;
            return ch.start_call_streaming(path, ptr, len, regions,
                                           timeout, parse_device);
          },
          py::arg("path"), py::arg("data"), py::arg("regions"),
          py::arg("timeout") = 0.0, py::arg("parse_device") = -1,
          "Streaming-region variant of start(); the send completes before "
          "this returns (region memory may be released), the response is "
          "collected with wait().")
      .def(
          "start",
          [](GrpcChannel& ch, const std::string& path, py::buffer data,
             double timeout) {
            py::buffer_info info = data.request();
            const uint8_t* ptr = static_cast<const uint8_t*>(info.ptr);
            size_t len = size_t(info.size) * size_t(info.itemsize);
            py::gil_scoped_release release;
            return ch.start_call(path, ptr, len, timeout);
          },
          py::arg("path"), py::arg("data"), py::arg("timeout") = 0.0)
      .def(
          "wait",
          [](GrpcChannel& ch, uint32_t id, double timeout) {
            py::gil_scoped_release release;
            Buf resp = ch.wait(id, timeout);
            return OwnedBuf(std::move(resp));
          },
          py::arg("id"), py::arg("timeout") = 0.0)
      .def_property_readonly(
          "streams_started", &GrpcChannel::streams_started,
          "Number of streams (calls) opened on this channel so far.")
      .def("close", &GrpcChannel::close,
           py::call_guard<py::gil_scoped_release>());

  m.def(
      "predict_sharded",
      [](const std::vector<GrpcChannel*>& channels, const std::string& path,
         const std::string& model_name, int64_t version,
         const std::string& signature,
         const std::vector<std::string>& names,
         const std::vector<at::Tensor>& tensors, int shards,
         int parse_device, double timeout) -> py::object {
        // with the GIL: validate, make contiguous; `contig` keeps every
        // payload alive in C++ until the last send has returned
        if (channels.empty()) throw py::value_error("no channels");
        for (auto* ch : channels)
          if (ch == nullptr) throw py::value_error("channel is None");
        if (names.size() != tensors.size() || tensors.empty())
          throw py::value_error("names/tensors mismatch");
        if (shards < 1) throw py::value_error("shards must be >= 1");
        std::vector<at::Tensor> contig(tensors.size());
        std::vector<tfsshard::Input> inputs(tensors.size());
        std::vector<int> input_devices;
        for (size_t i = 0; i < tensors.size(); ++i) {
          const at::Tensor& t = tensors[i];
          if (t.dim() == 0)
            throw py::value_error("sharded inputs need a batch dimension");
          if (!t.is_cuda() && !t.is_cpu())
            throw py::value_error("inputs must be CPU or GPU tensors");
          if (t.size(0) != tensors[0].size(0))
            throw py::value_error("inputs disagree on the dim-0 size");
          contig[i] = t.contiguous();
          auto& in = inputs[i];
          in.dtype = scalar_to_tf_dtype(contig[i].scalar_type());
          auto sz = contig[i].sizes();
          in.shape.assign(sz.begin(), sz.end());
          in.elem_size = size_t(contig[i].element_size());
          in.data = static_cast<const uint8_t*>(contig[i].const_data_ptr());
          in.device = contig[i].is_cuda();
          if (in.device) {
            int dev = int(contig[i].get_device());
            if (std::find(input_devices.begin(), input_devices.end(), dev) ==
                input_devices.end())
              input_devices.push_back(dev);
          }
        }
        if (tensors[0].size(0) < shards)
          throw py::value_error("batch is smaller than the shard count");
        ShardedResult r;
        {
          py::gil_scoped_release release;
          r = run_predict_sharded(channels, path, model_name, version,
                                  signature, names, inputs, input_devices,
                                  shards, parse_device, timeout);
        }
        if (r.merged) {
          py::dict d;
          for (auto& kv : r.outs) d[py::str(kv.first)] = kv.second;
          return std::move(d);
        }
        py::list parts;
        for (auto& p : r.parts) {
          py::object outs = py::none();
          if (p.parsed_ok) {
            py::dict d;
            for (auto& kv : p.outs) d[py::str(kv.first)] = kv.second;
            outs = std::move(d);
          }
          parts.append(py::make_tuple(outs, OwnedBuf(std::move(p.resp))));
        }
        return std::move(parts);
      },
      py::arg("channels"), py::arg("path"), py::arg("model_name"),
      py::arg("version"), py::arg("signature"), py::arg("names"),
      py::arg("tensors"), py::arg("shards"), py::arg("parse_device") = -1,
      py::arg("timeout") = 0.0,
      "One logical Predict split along dim 0 into `shards` PredictRequests "
      "sent in parallel over distinct channels (rotating between "
      "requests), behind a single GIL release. Returns the merged "
      "{name: device tensor} dict when every shard was device-parsed, "
      "else the per-shard [(outs | None, raw buf), ...] list.");

  m.def(
      "shutdown_sender_pool", [] { SenderPool::instance().shutdown(); },
      py::call_guard<py::gil_scoped_release>(),
      "Drain and join the sharded-send thread pool (restarted lazily by "
      "the next sharded call).");
  m.attr("SENDER_POOL_SIZE") = tfsshard::kSenderPoolSize;
  py::module_::import("atexit").attr("register")(
      m.attr("shutdown_sender_pool"));
}
