// The context behind the C ABI (include/klsh.h): device state and its allocation, the hyperplane
// window, the waits for the counters the kernels publish, and the entry points that create, load,
// snapshot and restore a context.  The arithmetic of the path runs only in the gfx950 kernels;
// there is no CPU fallback — without a gfx950 device klsh_create fails.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cstring>

#include "klsh_ctx.h"

using klsh::Counters;
using klsh::Snapshot;

static thread_local std::string g_err;  // klsh_last_error() of this thread

namespace klsh {
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hip_fail(const char* call, hipError_t e) {
  return fail(KLSH_E_HIP, std::string(call) + " -> " + hipGetErrorString(e));
}
}  // namespace klsh

void klsh_ctx::release_shard() {
  dfree(sbuf); dfree(rbuf); dfree(mark); dfree(dslots); dfree(bins); dfree(bins_all);
  dfree(owner); dfree(cntmat); dfree(small); dfree(drec); dfree(drec_all);
  if (h_small) (void)hipHostFree(h_small);
  h_small = nullptr;
  if (shp_host) (void)hipHostFree(shp_host);
  shp_host = shp_dev = nullptr;
  drec_cap = drec_all_cap = 0;
  shard_cap = 0;
}

int klsh_ctx::reserve_shard() {
  const int W = world();
  if (shard_cap >= cap_slots && sbuf) return 0;
  release_shard();
  const uint64_t s = std::max<uint64_t>(cap_slots, 1);
  const size_t nb = (size_t)1 << klsh::kMaxBinBits;
  auto bail = [&](int e) {  // nothing half-allocated stays
    release_shard();
    return e;
  };
  int e = 0;
  if ((e = dalloc(&sbuf, s)) || (e = dalloc(&rbuf, s)) || (e = dalloc(&mark, s)) ||
      (e = dalloc(&dslots, s)) || (e = dalloc(&bins, nb)) || (e = dalloc(&bins_all, nb * W)) ||
      (e = dalloc(&owner, nb)) || (e = dalloc(&cntmat, (size_t)W * W)) ||
      (e = dalloc(&small, (size_t)(W + 1) * 4)))
    return bail(e);
  if (hipHostMalloc((void**)&h_small, sizeof(uint32_t) * std::max(W * W, (W + 1) * 4),
                    hipHostMallocDefault) != hipSuccess)
    return bail(fail(KLSH_E_NOMEM, "pinned exchange buffer"));
  {
    const size_t words = 16 + std::max<size_t>((size_t)W * W, 4 * (size_t)W + sizeof(Counters) / 4);
    void *hp = nullptr, *dp = nullptr;
    if (hipHostMalloc(&hp, sizeof(uint32_t) * words, hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess ||
        hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
      if (hp) (void)hipHostFree(hp);
      return bail(fail(KLSH_E_NOMEM, "mapped exchange buffer"));
    }
    memset(hp, 0, sizeof(uint32_t) * words);
    shp_host = static_cast<uint32_t*>(hp);
    shp_dev = static_cast<uint32_t*>(dp);
    shp_seq = 0;
  }
  if (hipMemset(mark, 0, sizeof(uint32_t) * s) != hipSuccess)
    return bail(fail(KLSH_E_HIP, "mark init"));
  stamp = 0;
  shard_cap = s;
  return 0;
}

int klsh_ctx::reserve_words(uint32_t** p, size_t* cap, size_t words) {
  if (words <= *cap && *p) return 0;
  dfree(*p);
  *cap = 0;
  const size_t w = std::max<size_t>(words + words / 4, 1 << 16);
  if (int e = dalloc(p, w)) return e;
  *cap = w;
  return 0;
}

void klsh_ctx::release_state() {
  dfree(rows.x); dfree(rows.nrm); dfree(rows.cnt); dfree(rows.head); dfree(rows.tail);
  dfree(rows.nxt); dfree(order); dfree(alt); dfree(keys); dfree(keys2); dfree(nk1);
  dfree(nk2); dfree(nv2); dfree(hist); dfree(tile_sums); dfree(mp.lists.over); dfree(mp.run_ws);
  dfree(mp.lists.huge);
  dfree(mp.lists.long_P);
  mp.long_groups = 0;
  dfree(pp.v.fix);
  dfree(pp.v.ws);
  pp.v.cap = 0;
  for (auto& c : mp.lists.big) dfree(c);
  for (auto& c : mp.lists.cls) dfree(c);
  for (auto& c : mp.lists.act) dfree(c);
  dfree(kstamp);
  dfree(lb.status);
  dfree(xh_alloc);
  rows.xh = nullptr;
  cap_slots = cap_members = 0;
  cap_dp = 0;
  drop_snapshot();
}

void klsh_ctx::drop_snapshot() {
  dfree(snap.x); dfree(snap.nrm); dfree(snap.cnt); dfree(snap.head); dfree(snap.tail);
  dfree(snap.nxt); dfree(snap.order);
  snap.valid = false;
}

void klsh_ctx::join_drawer() {
  if (drawer.joinable()) {
    draw_stop.store(true);
    drawer.join();
    draw_stop.store(false);
  }
  w_target = 0;
}

void klsh_ctx::release() {
  join_drawer();
  if (w_pin) (void)hipHostFree(w_pin);
  w_pin = nullptr;
  w_pin_floats = 0;
  release_shard();
  delete comm;
  comm = nullptr;
  release_state();
  dfree(W);
  dfree(ctr);
  dfree(rc);
  mp.lists.rc = nullptr;
  if (h_ctr) (void)hipHostFree(h_ctr);
  h_ctr = nullptr;
  dfree(n_next_dev);
  if (pub_host) (void)hipHostFree(pub_host);
  pub_host = nullptr;
  pub_dev = nullptr;
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e), e = nullptr;
  for (auto& e : sev)
    if (e) (void)hipEventDestroy(e), e = nullptr;
  if (counts_ev) (void)hipEventDestroy(counts_ev);
  counts_ev = nullptr;
  for (int i = 0; i < klsh::kMergeStreams; ++i) {
    if (mp.join[i]) (void)hipEventDestroy(mp.join[i]);
    if (mp.aux[i]) (void)hipStreamDestroy(mp.aux[i]);
    mp.join[i] = nullptr;
    mp.aux[i] = nullptr;
  }
  if (mp.fork) (void)hipEventDestroy(mp.fork);
  mp.fork = nullptr;
  if (stream) (void)hipStreamDestroy(stream);
  stream = nullptr;
}

int klsh_ctx::ensure_long(uint64_t s, int d_) {
  const uint32_t want = klsh::long_ok(d_) && s >= 897 && mp.long_off != 1u
                            ? (uint32_t)std::min<uint64_t>(256, s / 897 + 1)
                            : 0u;
  if (want && want <= mp.long_groups) return 0;
  dfree(mp.lists.long_P);
  mp.long_groups = 0;
  if (!want) return 0;
  if (int e = dalloc(&mp.lists.long_P, (size_t)want * klsh::kLongRows * (klsh::kLongRows / 64)))
    return e;
  mp.long_groups = want;
  return 0;
}

int klsh_ctx::reserve(uint64_t ns, uint64_t nm, int d_) {
  if (ns >= 0xFFFFFFF0ull || nm >= 0xFFFFFFF0ull) return fail(KLSH_E_RANGE, "rows >= 2^32");
  if (d_ <= 0 || d_ > 4096) return fail(KLSH_E_RANGE, "d must be in [1, 4096]");
  const int dp_ = (d_ + 3) & ~3;
  if (ns <= cap_slots && nm <= cap_members && dp_ <= cap_dp) {
    d = d_;
    dp = dp_;
    rows.d = d;
    rows.dp = dp;
    if (shadow_wanted(d) && !xh_alloc)  // (an earlier load at a width without the image)
      if (int e = dalloc(&xh_alloc, cap_slots * (uint64_t)cap_dp)) return e;
    rows.xh = shadow_wanted(d) ? xh_alloc : nullptr;
    drop_snapshot();
    return ensure_long(cap_slots, d_);
  }
  release_state();
  auto bail = [&](int e) {  // nothing half-allocated stays
    release_state();
    return e;
  };
  const uint64_t s = std::max<uint64_t>(ns, 1), m = std::max<uint64_t>(nm, 1);
  int e = 0;
  if ((e = dalloc(&rows.x, s * dp_)) || (e = dalloc(&rows.nrm, s)) || (e = dalloc(&rows.cnt, s)) ||
      (e = dalloc(&rows.head, s)) || (e = dalloc(&rows.tail, s)) || (e = dalloc(&rows.nxt, m)) ||
      (e = dalloc(&order, s)) || (e = dalloc(&alt, s)) || (e = dalloc(&keys, s)) ||
      (e = dalloc(&keys2, s)) || (e = dalloc(&nk1, s + 64)) || (e = dalloc(&nk2, s)) ||
      (e = dalloc(&nv2, s)) ||
      (e = dalloc(&hist, klsh::sort_ws_words(s))) ||
      (e = dalloc(&tile_sums, klsh::scan_ws_words(s))) ||
      (e = dalloc(&mp.lists.over, s + 64)) || (e = dalloc(&mp.run_ws, klsh::run_ws_words(s))) ||
      (e = dalloc(&pp.v.fix, s)) || (e = dalloc(&pp.v.ws, 64)) ||
      (e = dalloc(&mp.lists.big[0], s / 65 + 64)) || (e = dalloc(&mp.lists.big[1], s / 129 + 64)) ||
      (e = dalloc(&mp.lists.big[2], s / 193 + 64)) || (e = dalloc(&mp.lists.big[3], s / 385 + 64)) ||
      (e = dalloc(&mp.lists.huge, s / 897 + 64)))
    return bail(e);
  if (shadow_wanted(d_))  // (in the large-buffer group: see below)
    if ((e = dalloc(&xh_alloc, s * dp_))) return bail(e);
  if ((e = ensure_long(s, d_))) return bail(e);
  for (int c = 0; c < klsh::kGroupClasses; ++c)
    if ((e = dalloc(&mp.lists.cls[c], klsh::group_class_capacity(c, s))) ||
        (e = dalloc(&mp.lists.act[c], klsh::group_class_capacity(c, s))))
      return bail(e);
  // the look-back workspaces start zeroed (tickets, done counters, epochs, histograms) and the
  // kernels return them to zero; they are never cleared again
  pp.v.cap = (uint32_t)s;
  if (hipMemset(pp.v.ws, 0, sizeof(uint32_t) * 64) != hipSuccess ||
      hipMemset(hist, 0, sizeof(uint32_t) * klsh::sort_ws_words(s)) != hipSuccess ||
      hipMemset(tile_sums, 0, sizeof(uint32_t) * klsh::scan_ws_words(s)) != hipSuccess)
    return bail(fail(KLSH_E_HIP, "workspace init"));
  // The stamp block and the look-back status words: small buffers allocated AFTER the rows and
  // workspaces.  (Allocated at context creation, ahead of the multi-GB state, they cost a C2 step
  // 252 -> 330 ms on MI355X: every random-access kernel slowed, the sort scatter 2.5x — the
  // large buffers evidently lost their large-page backing; A/B in DESIGN.md §6.)
  {
    std::vector<unsigned char> init(sizeof(klsh::KStampBlock), 0);
    auto* b = reinterpret_cast<klsh::KStampBlock*>(init.data());
    for (auto& st : b->set)
      for (auto& cls : st.t0)
        for (auto& ln : cls) ln.v = ~0ull;  // every start line ~0, every end line and total 0
    if ((e = dalloc(&kstamp, 1)) || (e = dalloc(&lb.status, 256))) return bail(e);
    if (hipMemcpy(kstamp, init.data(), init.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(lb.status, 0, sizeof(unsigned long long) * 256) != hipSuccess)
      return bail(fail(KLSH_E_HIP, "stamp / look-back init"));
    lb.epoch = 0;
  }
  mp.tile_sums = tile_sums;
  cap_slots = s;
  cap_members = m;
  cap_dp = dp_;
  d = d_;
  dp = dp_;
  rows.d = d;
  rows.dp = dp;
  rows.xh = shadow_wanted(d) ? xh_alloc : nullptr;
  return 0;
}

int klsh_ctx::apply_projection_variant() {
  if (!cap_slots) return 0;  // nothing reserved yet: reserve() decides
  if (shadow_wanted(d)) {
    if (!xh_alloc) {
      if (int e = dalloc(&xh_alloc, cap_slots * (uint64_t)cap_dp)) return e;
    }
    rows.xh = xh_alloc;
    klsh::launch_shadow_build(rows, slots, stream);  // merges did not keep it while it was off
    KLSH_HIP(hipGetLastError());
    KLSH_HIP(hipStreamSynchronize(stream));
  } else {
    rows.xh = nullptr;
  }
  return 0;
}

int klsh_ctx::restart_window(uint32_t base, uint64_t k0, uint64_t rows) {
  const uint64_t floats = std::max<uint64_t>(rows, 4096) * (uint64_t)dp;
  if (!W || floats > w_alloc) {
    dfree(W);
    if (int e = dalloc(&W, floats)) return e;
    w_alloc = floats;
  }
  w_cap = w_alloc / (uint64_t)dp;
  w_k0 = k0;
  w_count = 0;
  w_base = base;
  w_dp = dp;
  w_d = d;
  return 0;
}

int klsh_ctx::ensure_hyperplanes(uint32_t base, uint64_t k0, uint64_t count, double* host_ms) {
  if (count == 0) return 0;
  const bool same_stream = W && w_base == base && w_dp == dp && w_d == d;
  if (same_stream && k0 >= w_k0 && k0 + count <= w_k0 + w_count) return 0;
  const double t0 = now_ms();
  if (lazy_covers(base, k0, count)) {  // wait for the drawer, then append what it has
    const uint64_t need = k0 + count - w_k0;
    while (w_drawn.load(std::memory_order_acquire) < need) std::this_thread::yield();
    const uint64_t avail = w_drawn.load(std::memory_order_acquire);
    KLSH_HIP(hipMemcpyAsync(W + w_count * dp, w_pin + w_count * dp,
                            sizeof(float) * (avail - w_count) * dp, hipMemcpyHostToDevice,
                            stream));
    w_count = avail;
    if (host_ms) *host_ms += now_ms() - t0;
    return 0;
  }
  join_drawer();
  if (!(same_stream && k0 >= w_k0 && k0 + count <= w_k0 + w_cap)) {
    // (the window's row capacity carries over only for the same row width: w_cap rows of
    // another dp would scale the allocation by the width ratio on every change of d)
    if (int e = restart_window(base, k0, std::max(count, same_stream ? w_cap : 0))) return e;
  }
  const uint64_t start = w_k0 + w_count, n = k0 + count - start;
  std::vector<float> host((size_t)n * dp, 0.0f);
  klsh_host_hyperplanes(base, start, n, d, dp, host.data(), 0);
  KLSH_HIP(hipMemcpyAsync(W + (start - w_k0) * dp, host.data(), sizeof(float) * host.size(),
                          hipMemcpyHostToDevice, stream));
  KLSH_HIP(hipStreamSynchronize(stream));
  w_count += n;
  if (host_ms) *host_ms += now_ms() - t0;
  return 0;
}

// The hyperplanes of the first iterations of a call, drawn up front: every iteration's h_t
// (<= hmax) for all of them when that fits in 64 Mi floats (256 MB: C2 draws 11.5 K rows of 64),
// else the first 64 iterations' worth — ensure_hyperplanes extends the window when the loop
// gets there (-I 10000 at d = 4096 would otherwise need ~3.8 GB up front, host and device).
// The window is drawn by a background thread (see `drawer`) when it holds every iteration's rows;
// a smaller window (option hyperplane_window, or a call too long for 64 Mi floats) is drawn here
// and extended in place as before.
int klsh_ctx::predraw_hyperplanes(uint32_t base, uint64_t k0, uint64_t hmax, int iterations,
                                  double* host_ms) {
  join_drawer();
  const uint64_t want = hmax * (uint64_t)iterations;
  const uint64_t cap = hyperplane_window ? hyperplane_window
                                         : std::max<uint64_t>(hmax * 64, (64ull << 20) / (uint64_t)dp);
  const uint64_t count = std::min(want, cap);
  if (count == 0) return 0;
  if (hyperplane_window || count < want || !hyperplane_async)
    return ensure_hyperplanes(base, k0, count, host_ms);
  const double t0 = now_ms();
  if (!w_pin || count * (uint64_t)dp > w_pin_floats) {
    if (w_pin) (void)hipHostFree(w_pin);
    w_pin = nullptr;
    w_pin_floats = 0;
    if (hipHostMalloc((void**)&w_pin, sizeof(float) * count * (uint64_t)dp,
                      hipHostMallocDefault) != hipSuccess)
      return fail(KLSH_E_HIP, "pinned hyperplane window");
    w_pin_floats = count * (uint64_t)dp;
  }
  w_drawn.store(0);
  float* out = w_pin;
  const int dd = d, ddp = dp;
  // TODO: start the drawer after the stream sync below (a copy from w_pin still queued would race)
  drawer = std::thread([this, base, k0, count, out, dd, ddp] {
    // the first iterations' rows first (the loop starts on them), then larger chunks over the
    // host's worker threads
    uint64_t r = 0, chunk = 64;
    while (r < count && !draw_stop.load(std::memory_order_relaxed)) {
      const uint64_t n = std::min(chunk, count - r);
      if (ddp != dd) std::memset(out + r * ddp, 0, sizeof(float) * n * ddp);  // row padding
      klsh_host_hyperplanes(base, k0 + r, n, dd, ddp, out + r * ddp, chunk <= 64 ? 1 : 0);
      r += n;
      w_drawn.store(r, std::memory_order_release);
      chunk = 2048;
    }
  });
  // (the drawer runs meanwhile) a queued launch of an earlier call may still read the device
  // window, which is rewritten from its first row
  KLSH_HIP(hipStreamSynchronize(stream));
  if (int e = restart_window(base, k0, count)) return e;
  w_target = count;
  if (host_ms) *host_ms += now_ms() - t0;
  return 0;
}

int klsh_ctx::reset_counters() {
  KLSH_HIP(hipMemsetAsync(ctr, 0, sizeof(Counters), stream));
  KLSH_HIP(hipMemsetAsync(rc, 0, sizeof(klsh::RunCounters), stream));
  return 0;
}

int klsh_ctx::sync_counters() {
  ctr_clean = false;
  KLSH_HIP(hipMemcpyAsync(h_ctr, ctr, sizeof(Counters), hipMemcpyDeviceToHost, stream));
  KLSH_HIP(hipStreamSynchronize(stream));
  return check_device_err();
}

// Spin on the mapped sequence word until reached(word); every few thousand polls the stream is
// queried, so a failed kernel is reported instead of waited for.
template <class Reached>
static int poll_published(const klsh_ctx* ctx, Reached reached) {
  volatile uint32_t* p = ctx->pub_seq_host;
  uint64_t spins = 0;
  while (!reached(*p)) {
    __builtin_ia32_pause();
    if ((++spins & 0xFFFu) == 0) {
      const hipError_t q = hipStreamQuery(ctx->stream);
      if (q == hipSuccess) {
        std::atomic_thread_fence(std::memory_order_seq_cst);
        if (!reached(*p)) return fail(KLSH_E_HIP, "counters not published by a finished stream");
        break;
      }
      if (q != hipErrorNotReady) return fail(KLSH_E_HIP, std::string("stream: ") + hipGetErrorString(q));
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

int klsh_ctx::wait_published(uint32_t seq) {
  if (int e = poll_published(this, [seq](uint32_t w) { return w == seq; })) return e;
  memcpy(h_ctr, (const void*)pub_host, sizeof(Counters));
  ctr_clean = true;
  return check_device_err();
}

int klsh_ctx::wait_seq(uint32_t seq) {
  return poll_published(this, [seq](uint32_t w) { return (int32_t)(w - seq) >= 0; });
}

int klsh_ctx::check_device_err() const {
  if (h_ctr->err)
    return fail(KLSH_E_HIP, "device protocol failure (look-back wait limit), code " +
                                std::to_string(h_ctr->err));
  return 0;
}

int klsh_ctx::check_device_ptr(const void* p, const char* what) const {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (an unregistered host pointer is an error of the query itself)
    return fail(KLSH_E_ARG, std::string(what) + " is not device memory");
  }
  if (a.type != hipMemoryTypeDevice)
    return fail(KLSH_E_ARG, std::string(what) + " is not device memory");
  if (a.device != device)
    return fail(KLSH_E_ARG, std::string(what) + " belongs to another device");
  return 0;
}

// ===================================================================================== C ABI ===
extern "C" {

const char* klsh_last_error(void) { return g_err.c_str(); }
const char* klsh_version(void) { return "klsh-mi355x 0.2 (gfx950)"; }
int klsh_abi_version(void) { return KLSH_ABI_VERSION; }

klsh_ctx* klsh_create(int device, int* err) {
  auto refuse = [&](int code, const std::string& msg) -> klsh_ctx* {
    fail(code, msg);
    if (err) *err = code;
    return nullptr;
  };
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return refuse(KLSH_E_NODEVICE, "no HIP device visible (the engine has no CPU fallback)");
  if (device < 0 || device >= count) return refuse(KLSH_E_ARG, "device ordinal out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess ||
      std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return refuse(KLSH_E_NODEVICE, std::string("device is not gfx950: ") + prop.gcnArchName);
  if (hipSetDevice(device) != hipSuccess) return refuse(KLSH_E_HIP, "hipSetDevice");
  klsh_ctx* c = new klsh_ctx();
  c->device = device;
  // The big-run merge streams (aux 0 and the main stream, which carries the >384-row and
  // >896-row runs) get the highest priority: their workgroups need most of a CU's LDS and would
  // otherwise wait behind the small-run waves — on C4, where the >896-row runs are the critical
  // path, a normal-priority main stream doubled their time (KLSH_BIG_PRIORITY=0: all equal)
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  const bool big_prio = true;
  bool ok = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking,
                                        big_prio ? prio_hi : prio_lo) == hipSuccess;
  // Every event here only times work or orders streams of this device: none makes device
  // writes visible to the host (the counters come back through the published mapped line, with
  // its own system-scope release).  A default event ends with a system-scope release — an L2
  // writeback of everything the kernel before it wrote, 6-16 us of stream time per event on C2
  // (the projection -> sort and fork / join gaps of the round-3 trace) — so timing events skip
  // the fence and the fork / join events release at device scope.
  const unsigned tflags = hipEventDisableSystemFence;
  const unsigned oflags = hipEventDisableTiming | hipEventReleaseToDevice;
  for (auto& e : c->ev) ok = ok && hipEventCreateWithFlags(&e, tflags) == hipSuccess;
  for (auto& e : c->sev) ok = ok && hipEventCreateWithFlags(&e, tflags) == hipSuccess;
  for (int i = 0; i < klsh::kMergeStreams; ++i) {
    const bool hi = i == 0;  // (the 65..192-row stream high too: measured equal)
    ok = ok && hipStreamCreateWithPriority(&c->mp.aux[i], hipStreamNonBlocking,
                                           (hi && big_prio) ? prio_hi : prio_lo) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->mp.join[i], oflags) == hipSuccess;
  }
  ok = ok && hipEventCreateWithFlags(&c->mp.fork, oflags) == hipSuccess;
  ok = ok && hipMalloc((void**)&c->ctr, sizeof(Counters)) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->h_ctr, sizeof(Counters), hipHostMallocDefault) == hipSuccess;
  ok = ok && hipMemset(c->ctr, 0, sizeof(Counters)) == hipSuccess;  // err starts clear
  ok = ok && hipMalloc((void**)&c->rc, sizeof(klsh::RunCounters)) == hipSuccess &&
       hipMemset(c->rc, 0, sizeof(klsh::RunCounters)) == hipSuccess;
  c->mp.lists.rc = c->rc;
  ok = ok && hipMalloc((void**)&c->n_next_dev, 64) == hipSuccess &&
       hipMemset(c->n_next_dev, 0, 64) == hipSuccess;
  if (ok && c->zero_copy) {
    void* hp = nullptr;
    void* dp = nullptr;
    // [published counters][sequence word, 64 B][kRing ring slots]
    const size_t ring_at = sizeof(Counters) + 64;
    const size_t bytes = ring_at + sizeof(Counters) * klsh_ctx::kRing;
    if (hipHostMalloc(&hp, bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
        hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
      memset(hp, 0, bytes);
      c->pub_host = static_cast<Counters*>(hp);
      c->pub_dev = static_cast<Counters*>(dp);
      c->pub_seq_host = reinterpret_cast<uint32_t*>(static_cast<char*>(hp) + sizeof(Counters));
      c->pub_seq_dev = reinterpret_cast<uint32_t*>(static_cast<char*>(dp) + sizeof(Counters));
      c->ring_host = reinterpret_cast<Counters*>(static_cast<char*>(hp) + ring_at);
      c->ring_dev = reinterpret_cast<Counters*>(static_cast<char*>(dp) + ring_at);
    } else {
      if (hp) (void)hipHostFree(hp);
      c->zero_copy = false;  // fall back to copy + sync
    }
  }
  if (!ok) {
    delete c;
    return refuse(KLSH_E_HIP, "stream/event/counter allocation failed");
  }
  memset(c->h_ctr, 0, sizeof(Counters));
  if (err) *err = KLSH_OK;
  return c;
}

void klsh_destroy(klsh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  delete ctx;
}

int klsh_load_rows(klsh_ctx* ctx, const float* rows, uint64_t n, int d,
                   const uint64_t* member_offsets, const uint64_t* member_ids) {
  if (!ctx || (!rows && n)) return fail(KLSH_E_ARG, "null argument");
  KLSH_HIP(hipSetDevice(ctx->device));
  const uint64_t m = member_offsets ? member_offsets[n] : n;
  if (int e = ctx->reserve(n, m, d)) return e;
  hipStream_t s = ctx->stream;
  if (n) {
    KLSH_HIP(hipMemsetAsync(ctx->rows.x, 0, sizeof(float) * n * ctx->dp, s));
    KLSH_HIP(hipMemcpy2DAsync(ctx->rows.x, sizeof(float) * ctx->dp, rows, sizeof(float) * d,
                              sizeof(float) * d, n, hipMemcpyHostToDevice, s));
  }
  std::vector<uint32_t> cnt(n), head(n), tail(n), nxt(m), ord(n);
  ctx->ids.assign(m, 0);
  ctx->set_ids_linear(!member_ids, 0);
  for (uint64_t i = 0; i < n; ++i) {
    ord[i] = (uint32_t)i;
    if (member_offsets) {
      const uint64_t a = member_offsets[i], b = member_offsets[i + 1];
      cnt[i] = (uint32_t)(b - a);
      head[i] = b > a ? (uint32_t)a : klsh::kNil;
      tail[i] = b > a ? (uint32_t)(b - 1) : klsh::kNil;
      for (uint64_t k = a; k < b; ++k) {
        nxt[k] = k + 1 < b ? (uint32_t)(k + 1) : klsh::kNil;
        ctx->ids[k] = member_ids ? member_ids[k] : k;
      }
    } else {
      cnt[i] = 1;
      head[i] = tail[i] = (uint32_t)i;
      nxt[i] = klsh::kNil;
      ctx->ids[i] = member_ids ? member_ids[i] : i;
    }
  }
  if (n) {
    KLSH_HIP(hipMemcpyAsync(ctx->rows.cnt, cnt.data(), 4 * n, hipMemcpyHostToDevice, s));
    KLSH_HIP(hipMemcpyAsync(ctx->rows.head, head.data(), 4 * n, hipMemcpyHostToDevice, s));
    KLSH_HIP(hipMemcpyAsync(ctx->rows.tail, tail.data(), 4 * n, hipMemcpyHostToDevice, s));
    KLSH_HIP(hipMemcpyAsync(ctx->order, ord.data(), 4 * n, hipMemcpyHostToDevice, s));
  }
  if (m) KLSH_HIP(hipMemcpyAsync(ctx->rows.nxt, nxt.data(), 4 * m, hipMemcpyHostToDevice, s));
  klsh::launch_norms(ctx->rows, (uint32_t)n, s);
  KLSH_HIP(hipGetLastError());
  KLSH_HIP(hipStreamSynchronize(s));
  ctx->slots = n;
  ctx->members = m;
  klsh::launch_shadow_build(ctx->rows, ctx->slots, s);
  KLSH_HIP(hipGetLastError());
  ctx->n_live = n;
  ctx->loaded = true;
  return 0;
}

// klsh_load_rows for rows that are on the device already: the same state (every row a singleton),
// the member arrays set by a kernel instead of four uploads.
int klsh_load_rows_device(klsh_ctx* ctx, const float* d_rows, uint64_t n, int d,
                          uint64_t row_stride, const uint64_t* member_ids) {
  if (!ctx || (!d_rows && n)) return fail(KLSH_E_ARG, "null argument");
  if (d <= 0 || d > 4096) return fail(KLSH_E_RANGE, "d must be in [1, 4096]");
  if (row_stride < (uint64_t)d) return fail(KLSH_E_ARG, "row_stride is smaller than d");
  KLSH_HIP(hipSetDevice(ctx->device));
  if (n)
    if (int e = ctx->check_device_ptr(d_rows, "d_rows")) return e;
  if (int e = ctx->reserve(n, n, d)) return e;
  hipStream_t s = ctx->stream;
  ctx->loaded = false;  // (the state below replaces the previous load's, step by step)
  if (n) {
    KLSH_HIP(hipMemsetAsync(ctx->rows.x, 0, sizeof(float) * n * ctx->dp, s));
    KLSH_HIP(hipMemcpy2DAsync(ctx->rows.x, sizeof(float) * ctx->dp, d_rows,
                              sizeof(float) * row_stride, sizeof(float) * d, n,
                              hipMemcpyDeviceToDevice, s));
  }
  klsh::launch_init_singletons(ctx->rows, ctx->order, (uint32_t)n, s, ctx->grid_cap);
  klsh::launch_norms(ctx->rows, (uint32_t)n, s);
  KLSH_HIP(hipGetLastError());
  ctx->ids.resize(n);
  for (uint64_t i = 0; i < n; ++i) ctx->ids[i] = member_ids ? member_ids[i] : i;
  ctx->set_ids_linear(!member_ids, 0);
  ctx->slots = n;
  ctx->members = n;
  klsh::launch_shadow_build(ctx->rows, ctx->slots, s);
  KLSH_HIP(hipGetLastError());
  KLSH_HIP(hipStreamSynchronize(s));  // the caller may release d_rows
  ctx->n_live = n;
  ctx->loaded = true;
  return 0;
}

// The checks of klsh_load_clusters_device that need the lists themselves, into scratch of the
// call alone (nothing of the context is written): offsets strictly increasing, m <= M, every node
// below M and listed once.  Leaves *m_out = off[n] - off[0], *base_out = off[0] and the start
// map the link pass reads.
static int check_clusters(klsh_ctx* ctx, uint64_t n, const uint32_t* d_off, const uint32_t* d_nodes,
                          uint64_t M, klsh::DevBuf<uint8_t>& start, uint64_t* m_out,
                          uint32_t* base_out) {
  hipStream_t s = ctx->stream;
  const uint32_t cap = ctx->grid_cap;
  klsh::DevBuf<unsigned long long> err;
  klsh::DevBuf<uint32_t> owner;
  if (int e = dalloc(err, 1)) return e;
  uint32_t ends[2] = {0, 0};
  KLSH_HIP(hipMemsetAsync(err, 0xFF, sizeof(unsigned long long), s));
  KLSH_HIP(hipMemcpyAsync(&ends[0], d_off, 4, hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipMemcpyAsync(&ends[1], d_off + n, 4, hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipStreamSynchronize(s));
  // what m is if the offsets increase; if they do not, the row check below refuses the load
  const uint64_t m = ends[1] > ends[0] ? (uint64_t)ends[1] - ends[0] : 0;
  const bool fits = m && m <= M;
  if (fits) {
    if (int e = dalloc(start, m)) return e;
    KLSH_HIP(hipMemsetAsync(start, 0, m, s));
  }
  unsigned long long bad = 0;
  auto read_err = [&]() -> int {
    KLSH_HIP(hipGetLastError());
    KLSH_HIP(hipMemcpyAsync(&bad, err, sizeof(bad), hipMemcpyDeviceToHost, s));
    KLSH_HIP(hipStreamSynchronize(s));
    return 0;
  };
  klsh::launch_clusters_check_rows(d_off, (uint32_t)n, (uint32_t)m, fits ? start.get() : nullptr,
                                   err, s, cap);
  if (int e = read_err()) return e;
  if (bad != ~0ull)
    return fail(KLSH_E_ARG, "d_member_offsets is not strictly increasing at row " +
                                std::to_string(bad >> 2) + " (a row needs a member)");
  if (m > M)
    return fail(KLSH_E_ARG, "the lists hold " + std::to_string(m) + " entries, more than the " +
                                std::to_string(M) + " nodes");
  if (d_nodes) {
    if (int e = dalloc(owner, M)) return e;
    KLSH_HIP(hipMemsetAsync(owner, 0xFF, sizeof(uint32_t) * M, s));
    klsh::launch_clusters_check_nodes(d_nodes + ends[0], (uint32_t)m, (uint32_t)M, owner, err, s,
                                      cap);
    if (int e = read_err()) return e;
    if (bad != ~0ull) {
      const uint64_t q = bad >> 2;  // (an entry of the window; the caller's index adds off[0])
      uint32_t node = 0, first = 0;
      KLSH_HIP(hipMemcpy(&node, d_nodes + ends[0] + q, 4, hipMemcpyDeviceToHost));
      const std::string at = "entry " + std::to_string(ends[0] + q) + " of d_member_nodes";
      if ((bad & 3) == klsh::kLcErrRange)
        return fail(KLSH_E_ARG, at + " is node " + std::to_string(node) + ", not below the " +
                                    std::to_string(M) + " nodes");
      KLSH_HIP(hipMemcpy(&first, owner + node, 4, hipMemcpyDeviceToHost));
      return fail(KLSH_E_ARG, at + " lists node " + std::to_string(node) + " twice (first at entry " +
                                  std::to_string((uint64_t)ends[0] + first) + ")");
    }
  }
  *m_out = m;
  *base_out = ends[0];
  return 0;
}

// Rows with their member lists from device memory: the state klsh_load_rows
// leaves for the same rows and lists, the lists linked by kernels, the nodes the caller's numbers.
int klsh_load_clusters_device(klsh_ctx* ctx, const float* d_rows, uint64_t n, int d,
                              uint64_t row_stride, const uint32_t* d_member_offsets,
                              const uint32_t* d_member_nodes, uint64_t n_nodes,
                              const uint64_t* member_ids) {
  if (!ctx || (n && (!d_rows || !d_member_offsets))) return fail(KLSH_E_ARG, "null argument");
  if (d <= 0 || d > 4096) return fail(KLSH_E_RANGE, "d must be in [1, 4096]");
  if (row_stride < (uint64_t)d) return fail(KLSH_E_ARG, "row_stride is smaller than d");
  if (n >= 0xFFFFFFF0ull || n_nodes >= 0xFFFFFFF0ull)
    return fail(KLSH_E_RANGE, "rows or nodes >= 2^32");
  const bool keep = n_nodes == 0;  // the node space and the ids of the current load stay
  if (keep && member_ids)
    return fail(KLSH_E_ARG, "member_ids given with n_nodes = 0 (the loaded ids are kept)");
  if (keep && !ctx->loaded) return fail(KLSH_E_STATE, "n_nodes = 0 keeps a load, and nothing is loaded");
  KLSH_HIP(hipSetDevice(ctx->device));
  const uint64_t M = keep ? ctx->members : n_nodes;
  klsh::DevBuf<uint8_t> start;
  uint64_t m = 0;
  uint32_t base = 0;
  if (n) {
    if (int e = ctx->check_device_ptr(d_rows, "d_rows")) return e;
    if (int e = ctx->check_device_ptr(d_member_offsets, "d_member_offsets")) return e;
    if (d_member_nodes)
      if (int e = ctx->check_device_ptr(d_member_nodes, "d_member_nodes")) return e;
    if (int e = check_clusters(ctx, n, d_member_offsets, d_member_nodes, M, start, &m, &base))
      return e;
  }
  if (int e = ctx->reserve(n, M, d)) return e;
  hipStream_t s = ctx->stream;
  ctx->loaded = false;  // (the state below replaces the previous load's, step by step)
  if (n) {
    KLSH_HIP(hipMemsetAsync(ctx->rows.x, 0, sizeof(float) * n * ctx->dp, s));
    KLSH_HIP(hipMemcpy2DAsync(ctx->rows.x, sizeof(float) * ctx->dp, d_rows,
                              sizeof(float) * row_stride, sizeof(float) * d, n,
                              hipMemcpyDeviceToDevice, s));
  }
  klsh::launch_clusters_link(ctx->rows, ctx->order, d_member_offsets,
                             d_member_nodes ? d_member_nodes + base : nullptr, start, (uint32_t)n,
                             (uint32_t)m, (uint32_t)M, s, ctx->grid_cap);
  klsh::launch_norms(ctx->rows, (uint32_t)n, s);
  KLSH_HIP(hipGetLastError());
  if (!keep) {
    ctx->ids.resize(M);
    for (uint64_t k = 0; k < M; ++k) ctx->ids[k] = member_ids ? member_ids[k] : k;
    ctx->set_ids_linear(!member_ids, 0);
  }
  ctx->slots = n;
  ctx->members = M;
  klsh::launch_shadow_build(ctx->rows, ctx->slots, s);
  KLSH_HIP(hipGetLastError());
  KLSH_HIP(hipStreamSynchronize(s));  // the caller may release its three arrays
  ctx->n_live = n;
  ctx->loaded = true;
  return 0;
}

int klsh_load_counts(klsh_ctx* ctx, const uint16_t* counts, uint64_t n_total,
                     uint64_t batch_offset, uint64_t batch_size, int d, const float* v_kmers) {
  if (!ctx || !counts || !v_kmers) return fail(KLSH_E_ARG, "null argument");
  if (batch_offset + batch_size > n_total) return fail(KLSH_E_ARG, "batch outside the matrix");
  KLSH_HIP(hipSetDevice(ctx->device));
  const uint64_t bs = batch_size;
  if (int e = ctx->reserve(bs, bs, d)) return e;
  hipStream_t s = ctx->stream;
  // float(log(c + 1.0)) for every uint16 count: glibc double log on the host, exact.
  static std::vector<float> lut;
  if (lut.empty()) {
    lut.resize(65536);
    for (int c = 0; c < 65536; ++c) lut[c] = (float)std::log((double)c + 1.0);
  }
  klsh::DevBuf<uint16_t> dcounts;
  klsh::DevBuf<float> dlut, dv;
  if (int e = dalloc(dcounts, (size_t)bs * d)) return e;
  if (int e = dalloc(dlut, 65536)) return e;
  if (int e = dalloc(dv, d)) return e;
  auto convert = [&]() -> int {
    if (bs && hipMemcpy2DAsync(dcounts, sizeof(uint16_t) * bs, counts + batch_offset,
                               sizeof(uint16_t) * n_total, sizeof(uint16_t) * bs, d,
                               hipMemcpyHostToDevice, s) != hipSuccess)
      return fail(KLSH_E_HIP, "count upload");
    if (hipMemcpyAsync(dlut, lut.data(), sizeof(float) * 65536, hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        hipMemcpyAsync(dv, v_kmers, sizeof(float) * d, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail(KLSH_E_HIP, "lut upload");
    if (ctx->reset_counters()) return fail(KLSH_E_HIP, "counter reset");
    klsh::launch_convert(ctx->rows, dcounts, (uint32_t)bs, dlut, dv, ctx->keys, ctx->order,
                         ctx->tile_sums, ctx->ctr, s);
    if (hipGetLastError() != hipSuccess) return fail(KLSH_E_HIP, "convert launch");
    return ctx->sync_counters();
  };
  const int rc = convert();
  (void)hipStreamSynchronize(s);
  if (rc) return rc;
  ctx->ids.resize(bs);
  for (uint64_t i = 0; i < bs; ++i) ctx->ids[i] = batch_offset + i;
  ctx->set_ids_linear(true, batch_offset);
  ctx->slots = bs;
  ctx->members = bs;
  klsh::launch_shadow_build(ctx->rows, ctx->slots, s);
  KLSH_HIP(hipGetLastError());
  ctx->n_live = bs ? ctx->h_ctr->total : 0;
  ctx->loaded = true;
  return 0;
}

// The row state and the live order, device to device: `to_snapshot` copies them into the
// snapshot, else back out of it.
static int copy_state(klsh_ctx* ctx, bool to_snapshot, uint64_t n_order) {
  Snapshot& sn = ctx->snap;
  klsh::Rows& r = ctx->rows;
  hipStream_t st = ctx->stream;
  const uint64_t s = ctx->slots, m = ctx->members;
  const struct {
    void *live, *saved;
    uint64_t bytes;
  } parts[] = {{r.x, sn.x, 4 * s * ctx->dp}, {r.nrm, sn.nrm, 4 * s},   {r.cnt, sn.cnt, 4 * s},
               {r.head, sn.head, 4 * s},     {r.tail, sn.tail, 4 * s}, {r.nxt, sn.nxt, 4 * m},
               {ctx->order, sn.order, 4 * n_order}};
  for (const auto& p : parts)
    KLSH_HIP(hipMemcpyAsync(to_snapshot ? p.saved : p.live, to_snapshot ? p.live : p.saved,
                            p.bytes, hipMemcpyDeviceToDevice, st));
  KLSH_HIP(hipStreamSynchronize(st));
  return 0;
}

int klsh_snapshot(klsh_ctx* ctx) {
  if (!ctx || !ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  KLSH_HIP(hipSetDevice(ctx->device));
  Snapshot& sn = ctx->snap;
  if (!sn.valid) {
    int e = 0;
    const uint64_t s = std::max<uint64_t>(ctx->slots, 1), m = std::max<uint64_t>(ctx->members, 1);
    if ((e = dalloc(&sn.x, s * ctx->dp)) || (e = dalloc(&sn.nrm, s)) || (e = dalloc(&sn.cnt, s)) ||
        (e = dalloc(&sn.head, s)) || (e = dalloc(&sn.tail, s)) || (e = dalloc(&sn.nxt, m)) ||
        (e = dalloc(&sn.order, s))) {
      ctx->drop_snapshot();
      return e;
    }
  }
  if (int e = copy_state(ctx, true, ctx->n_live)) return e;
  sn.n_live = ctx->n_live;
  sn.valid = true;
  return 0;
}

int klsh_restore(klsh_ctx* ctx) {
  if (!ctx || !ctx->snap.valid) return fail(KLSH_E_STATE, "no snapshot");
  KLSH_HIP(hipSetDevice(ctx->device));
  if (int e = copy_state(ctx, false, ctx->snap.n_live)) return e;
  klsh::launch_shadow_build(ctx->rows, ctx->slots, ctx->stream);  // (rebuilt, not snapshotted)
  KLSH_HIP(hipGetLastError());
  ctx->n_live = ctx->snap.n_live;
  return 0;
}

}  // extern "C"
