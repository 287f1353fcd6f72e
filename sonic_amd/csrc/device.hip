// Library state of libsonic_hip.so: the thread-local error string, the per-kernel profiler, the device contexts and scopes every entry
// point runs in (internal.hpp, "devices"), and the entry points that concern the library or a device rather than a handle: sonic_init,
// sonic_device_*, sonic_hip_versions, sonic_last_error, sonic_abi_version, sonic_dev_* and sonic_profile_*.
#include <stdarg.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "internal.hpp"

namespace sonic {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

Profiler& profiler() { static Profiler p; return p; }
void Profiler::collect() {
  std::lock_guard<std::mutex> g(mu);
  for (auto& kv : recs) {
    auto& tot = totals[kv.first];
    for (auto& r : kv.second) {
      hipEventSynchronize(r.b);
      float ms = 0;
      hipEventElapsedTime(&ms, r.a, r.b);
      tot.first += ms; tot.second += 1;
      hipEventDestroy(r.a); hipEventDestroy(r.b);
    }
    kv.second.clear();
  }
}
void Profiler::reset() { collect(); std::lock_guard<std::mutex> g(mu); totals.clear(); }

// ---- devices ----------------------------------------------------------------------------------------------------------------------
static std::mutex g_init_mu;
static int g_device = -1;                    // the default device: sonic_init, else LOCAL_RANK % count, else 0
static int g_device_count = -1;
static std::vector<DeviceCtx*> g_ctx;        // by ordinal; entries are made on first use and live as long as the process
static thread_local DeviceCtx* t_ctx = nullptr;

static int device_count_locked() {
  if (g_device_count >= 0) return g_device_count;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device available (%s): libsonic_hip has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    throw HipFail{SONIC_ERR_NO_DEVICE};
  }
  g_device_count = n;
  g_ctx.assign((size_t)n, nullptr);
  return n;
}
// caller holds g_init_mu and has made `dev` the thread's HIP device
static DeviceCtx* ctx_locked(int dev) {
  if (!g_ctx[(size_t)dev]) {
    std::unique_ptr<DeviceCtx> c(new DeviceCtx());
    c->dev = dev;
    HIP_OK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    g_ctx[(size_t)dev] = c.release();
  }
  return g_ctx[(size_t)dev];
}
int default_device_ordinal() { std::lock_guard<std::mutex> g(g_init_mu); return g_device; }
void unlink_one_shot_of(const sonic_srs* s) {
  std::lock_guard<std::mutex> g(g_init_mu);
  for (DeviceCtx* c : g_ctx) {
    if (!c) continue;
    std::lock_guard<std::mutex> g2(c->one_shot_mu);
    for (size_t i = 0; i < c->one_shot.size();) {
      if (static_cast<OneShotShell*>(c->one_shot[i])->srs == s) c->one_shot.erase(c->one_shot.begin() + (long)i);      // (leaked: its device is out of reach)
      else i++;
    }
  }
}

DeviceScope::DeviceScope(int dev) : ctx_(nullptr), prev_ctx_(t_ctx), prev_dev_(-1) {
  if (t_ctx && (dev < 0 || t_ctx->dev == dev)) { ctx_ = t_ctx; return; }      // nested call: a handle-less callee inherits the caller's device
  std::lock_guard<std::mutex> g(g_init_mu);
  const int n = device_count_locked();
  if (dev < 0) {
    if (g_device < 0) {
      const char* lr = getenv("LOCAL_RANK");
      g_device = lr ? atoi(lr) % n : 0;
      if (g_device < 0) g_device = 0;
    }
    dev = g_device;
  }
  if (dev >= n) { set_error("device %d out of range (%d device%s)", dev, n, n == 1 ? "" : "s"); throw HipFail{SONIC_ERR_INVALID_ARG}; }
  if (hipGetDevice(&prev_dev_) != hipSuccess) { (void)hipGetLastError(); prev_dev_ = -1; }
  if (prev_dev_ != dev) HIP_OK(hipSetDevice(dev));
  try { ctx_ = ctx_locked(dev); } catch (...) { if (prev_dev_ >= 0 && prev_dev_ != dev) (void)hipSetDevice(prev_dev_); throw; }
  t_ctx = ctx_;
}
DeviceScope::~DeviceScope() {
  if (ctx_ == prev_ctx_) return;                       // nested on the same device: nothing was changed
  t_ctx = prev_ctx_;
  if (prev_dev_ >= 0 && prev_dev_ != ctx_->dev) (void)hipSetDevice(prev_dev_);
}
const NttTables& device_ntt_tables(int log2n) {
  DeviceCtx& c = current_ctx();
  std::lock_guard<std::mutex> g(c.pool_mu);
  NttTables*& t = c.prover_ntt[log2n];
  if (!t) {
    std::unique_ptr<NttTables> nt(new NttTables());
    hipStream_t st = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    try { nt->ensure(st, log2n); HIP_OK(hipStreamSynchronize(st)); } catch (...) { (void)hipStreamDestroy(st); throw; }
    (void)hipStreamDestroy(st);
    t = nt.release();
  }
  return *t;
}
int device_prover_streams() {
  DeviceCtx& c = current_ctx();
  std::lock_guard<std::mutex> g(c.pool_mu);
  if (c.prover_streams < 0) {
    // (the number of queues is READ: the variable counts only when it is set before the process's first HIP call -- stream_pool.hpp)
    const int n = pool_size_of_env(getenv("GPU_MAX_HW_QUEUES"), getenv("SONIC_STREAM_POOL"));
    if (n > 0) c.prover_stream[0] = c.stream;
    for (int i = 1; i < n; i++) HIP_OK(hipStreamCreateWithFlags(&c.prover_stream[i], hipStreamNonBlocking));
    c.prover_streams = n;
  }
  return c.prover_streams;
}
DeviceCtx& current_ctx() {
  if (!t_ctx) { set_error("internal: no device scope on this thread"); throw HipFail{SONIC_ERR_HIP}; }
  return *t_ctx;
}

CallLease::CallLease() : c_(nullptr), owner_(&current_ctx()) {
  {
    std::lock_guard<std::mutex> g(owner_->pool_mu);
    if (!owner_->pool.empty()) { c_ = owner_->pool.back(); owner_->pool.pop_back(); }
  }
  if (!c_) {
    std::unique_ptr<CallCtx> c(new CallCtx());
    HIP_OK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    c_ = c.release();
  }
}
CallLease::~CallLease() {
  (void)hipStreamSynchronize(c_->st);        // nothing of this call may still be running when the context is handed on
  std::lock_guard<std::mutex> g(owner_->pool_mu);
  owner_->pool.push_back(c_);
}

}  // namespace sonic

using namespace sonic;

extern "C" {

int sonic_init(int device_ordinal) {
  API_HOST_BEGIN                  // (the scope is opened below, once the default device has been chosen)
  {
    std::lock_guard<std::mutex> g(g_init_mu);
    const int n = device_count_locked();
    if (device_ordinal >= n) { set_error("device %d out of range (%d device%s)", device_ordinal, n, n == 1 ? "" : "s"); return SONIC_ERR_INVALID_ARG; }
    if (g_device < 0 && device_ordinal >= 0) g_device = device_ordinal;       // the first choice of a default device stands
  }
  int dev;
  { DeviceScope scope(-1); dev = scope.ctx().dev; }
  // the default device stays the calling thread's HIP device after sonic_init (a caller with a HIP binding of its own, e.g. torch
  // tensors handed to the _dev entry points, allocates there)
  HIP_OK(hipSetDevice(dev));
  API_END
}

int sonic_device_count(int* out) {
  if (!out) return SONIC_ERR_INVALID_ARG;
  // (a tail of its own: without a device the count is written as 0 beside the status)
  try { std::lock_guard<std::mutex> g(g_init_mu); *out = device_count_locked(); } catch (const HipFail& f) { *out = 0; return f.code; }
  return SONIC_OK;
}

// the HIP the library was built against and the HIP runtime that got mapped into this process (they differ when another
// component, e.g. a PyTorch-ROCm wheel, brought its own libamdhip64 first); no device needed
int sonic_hip_versions(int* build, int* runtime) {
  if (build) *build = HIP_VERSION;
  if (runtime) { int v = 0; if (hipRuntimeGetVersion(&v) != hipSuccess) v = 0; *runtime = v; }
  return SONIC_OK;
}

int sonic_last_error(char* buf, size_t cap) {
  if (!buf || cap == 0) return SONIC_ERR_INVALID_ARG;
  strncpy(buf, g_err, cap - 1);
  buf[cap - 1] = 0;
  return SONIC_OK;
}

int sonic_device_sync(void) { API_BEGIN HIP_OK(hipStreamSynchronize(default_stream())); HIP_OK(hipDeviceSynchronize()); API_END }

int sonic_abi_version(void) { return SONIC_ABI_VERSION; }

// device memory for callers without a HIP binding: _on allocates on a named GPU; free / upload / download find the pointer's device
static int device_of_pointer(const void* p) {
  hipPointerAttribute_t a;
  if (p && hipPointerGetAttributes(&a, p) == hipSuccess) return a.device;
  (void)hipGetLastError();
  return -1;
}
int sonic_dev_alloc(size_t bytes, void** out) { return sonic_dev_alloc_on(-1, bytes, out); }
int sonic_dev_alloc_on(int device, size_t bytes, void** out) { API_BEGIN_ON(device) if (!out) return SONIC_ERR_INVALID_ARG; HIP_OK(hipMalloc(out, bytes ? bytes : 16)); API_END }
int sonic_dev_free(void* p) { API_BEGIN_ON(device_of_pointer(p)) HIP_OK(hipFree(p)); API_END }
int sonic_dev_upload(void* dst, const void* src, size_t bytes) { API_BEGIN_ON(device_of_pointer(dst)) HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); API_END }
int sonic_dev_download(void* dst, const void* src, size_t bytes) { API_BEGIN_ON(device_of_pointer(src)) HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); API_END }

int sonic_profile_enable(int on) { profiler().on = on != 0; return SONIC_OK; }
int sonic_profile_reset(void) { profiler().reset(); return SONIC_OK; }
int sonic_profile_get(const char* kernel, double* total_ms, int64_t* launches) {
  if (!kernel) return SONIC_ERR_INVALID_ARG;
  profiler().collect();
  std::lock_guard<std::mutex> g(profiler().mu);
  auto it = profiler().totals.find(kernel);
  if (total_ms) *total_ms = it == profiler().totals.end() ? 0.0 : it->second.first;
  if (launches) *launches = it == profiler().totals.end() ? 0 : it->second.second;
  return SONIC_OK;
}
int sonic_profile_names(char* buf, size_t cap) {
  if (!buf || cap == 0) return SONIC_ERR_INVALID_ARG;
  profiler().collect();
  std::lock_guard<std::mutex> g(profiler().mu);
  std::string s;
  for (auto& kv : profiler().totals) { s += kv.first; s += "\n"; }
  strncpy(buf, s.c_str(), cap - 1);
  buf[cap - 1] = 0;
  return SONIC_OK;
}

}  // extern "C"
