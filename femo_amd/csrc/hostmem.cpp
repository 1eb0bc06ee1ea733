// Host boundary of the engine: where NumPy arrays of the CSDL operators meet HBM.
//
// Replaces the reference's array <-> PETSc Vec copies (utils_dolfinx.py:155-167 getFuncArray /
// setFuncArray, :300-311 update), which on a GPU engine are PCIe transfers of up to 477 MB
// (the DG0 source of the 10 M-DOF cube) per call.  Three mechanisms:
//
//  1. Pinned host blocks (femo_host_alloc / femo_host_register).  A transfer from or to a pinned
//     block is one DMA at PCIe rate.  The library hands its own results out in such blocks.  Released blocks are recycled;
//     one released while a DMA still owns it is parked and recycled by a later pool call, never waited for (g_limbo).
//  2. Pageable user memory goes through a ring of pinned staging slots: a pool of host threads
//     copies chunk i+1 into (out of) a slot while the DMA engine moves chunk i, instead of the HIP
//     runtime's single-threaded pageable path (measured 3-5 GB/s in round 1).
//  3. Provenance.  Every device vector carries a generation counter that every writing entry
//     point bumps; a pinned block remembers "I am an exact copy of vector uid @ generation g"
//     when the library fills it (D2H) or uploads it (H2D).  femo_vec_set_host from such a block
//     is then skipped (the vector still holds that content) or replaced by a device-to-device copy
//     (another live vector does).  The reference re-sends unchanged inputs in every operator method
//     ("might be redundant", state_model.py:168-173); with provenance those re-sends cost nothing
//     and stay exact: host-side writers must announce themselves (femo_host_touch), which is why
//     the Python layer returns read-only arrays.  FEMO_HOST_VERIFY=1 checks every elision against
//     a real comparison (tests).  Only blocks of femo_host_alloc are ever recorded: caller memory pinned in place
//     (femo_host_register, which the Python layer does by itself for arrays it is handed repeatedly) can be written by
//     its owner at any time and is never trusted as a mirror.
//  4. Asynchronous results (femo_vec_get_host_async).  The copy-out of a result runs on a second stream
//     and the call returns at once; the block carries an event until the bytes have landed.  Every library
//     entry that touches such a block waits first (or needs no bytes at all: an elided upload), a caller that
//     reads it with its own code calls femo_host_wait / femo_host_sync.  The next kernel that writes the
//     vector waits for the copy on the device (femo_vec_touch).  With it the 477 MB of dJ/df travel while the
//     adjoint system is assembled and solved.
//  5. Accumulate on the device.  femo_vec_add_to_host into a block that still mirrors a live vector G forms
//     G + v in a scratch vector and copies the sum out at DMA rate, instead of adding on the host while the
//     chunks arrive (same bits: one IEEE addition per entry either way).
//  6. The streamed tail (femo_dRdf_cell_apply_T_add_to_host).  The last statement of a reverse sweep, dJ/df += (dR/df)^T psi
//     into such a block, forms the sum range by range -- product and addition in one kernel, no round trip of the product
//     through HBM -- and sends each range down on the copy stream while the next one is computed.  Its ranges grow from a
//     short first one, the pieces of the chunked upload of f shrink to a short last one (range_plan.h).
//  7. Promised results (femo_vec_get_host_promised).  A block is recorded as the copy of a vector and marked pending, but
//     nothing travels until somebody asks for the bytes (femo_host_wait, femo_host_sync, any entry that reads the block) or
//     the vector is about to change.  Handed back to femo_vec_set_host it is elided like any mirror; femo_host_forget drops
//     it.  The multiplier of the adjoint solve is consumed on the device and never read on the host: its 8 n_vert bytes
//     stay off the link that carries the gradient.  So do the partials of an output operator (FEMO_PROMISE_OUTPUT): dJ/du
//     goes back into the adjoint solve -- femo_host_axpby(-1, x, 0, y) from a promised x promises y the product -- and the
//     explicit dJ/df is the block the streamed tail overwrites from the device.
#include <sched.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "femo_internal.h"
#include "range_plan.h"

namespace {

// ------------------------------------------------------------------ thread pool ----
int usable_cores() {
  int n = 1;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  std::ifstream f("/sys/fs/cgroup/cpu.max");
  std::string quota, period;
  if (f >> quota >> period && quota != "max") {
    const long q = atol(quota.c_str()), p = atol(period.c_str());
    if (q > 0 && p > 0) n = std::max(1, std::min<int>(n, (int)(q / p)));
  }
  return n;
}

// fork-join pool: run(nparts, fn) calls fn(part) for part in [0, nparts) on the workers and the caller.
// Every job has its own state object (function, part count, counters): a worker that is preempted between taking a
// part index and reading the job can never see the fields of the NEXT job, and the caller's wait is
// tied to its own job object.
class HostPool {
 public:
  static HostPool& get() {
    // never destroyed: the workers wait on its condition variable until the process ends, and destroying a
    // condition variable with waiters blocks in glibc (an interpreter exiting would hang)
    static HostPool* p = new HostPool();
    return *p;
  }
  int threads() const { return nthreads_; }
  void run(int nparts, const std::function<void(int)>& fn) {
    if (nparts <= 1 || nthreads_ <= 1) {
      for (int i = 0; i < nparts; ++i) fn(i);
      return;
    }
    std::lock_guard<std::mutex> serial(run_mu_);      // one job at a time (contexts on several host threads)
    auto job = std::make_shared<Job>();
    job->fn = &fn;
    job->nparts = nparts;
    job->left.store(nparts);
    {
      std::lock_guard<std::mutex> lk(mu_);
      cur_ = job;
      ++job_;
    }
    cv_.notify_all();
    work(*job);
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return job->left.load() == 0; });   // every part of THIS job has returned: fn may go
    cur_.reset();
  }

 private:
  struct Job {
    const std::function<void(int)>* fn = nullptr;
    int nparts = 0;
    std::atomic<int> next{0}, left{0};
  };
  HostPool() {
    nthreads_ = std::min(usable_cores(), 16);
    if (const char* e = getenv("FEMO_HOST_THREADS")) nthreads_ = std::max(1, atoi(e));
    for (int i = 1; i < nthreads_; ++i) workers_.emplace_back([this] { loop(); });
    for (auto& t : workers_) t.detach();              // live until the process exits
  }
  void work(Job& j) {
    for (;;) {
      const int i = j.next.fetch_add(1);
      if (i >= j.nparts) return;
      (*j.fn)(i);                                      // fn outlives the job: run() waits for left == 0
      if (j.left.fetch_sub(1) == 1) {
        std::lock_guard<std::mutex> lk(mu_);
        done_cv_.notify_all();
      }
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      std::shared_ptr<Job> j;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return job_ != seen; });
        seen = job_;
        j = cur_;                                      // may already be finished and reset: nothing to do then
      }
      if (j) work(*j);
    }
  }
  int nthreads_ = 1;
  std::vector<std::thread> workers_;
  std::mutex mu_, run_mu_;
  std::condition_variable cv_, done_cv_;
  std::shared_ptr<Job> cur_;
  uint64_t job_ = 0;
};

// op: 0 copy, 1 dst += src, 2 dst = a*src + b*dst
void par_stream(double* dst, const double* src, int64_t n, int op, double a = 1.0, double b = 0.0) {
  if (n <= 0) return;
  HostPool& P = HostPool::get();
  const int64_t grain = 1 << 16;                      // 512 KiB per part at least
  int parts = (int)std::min<int64_t>(P.threads(), (n + grain - 1) / grain);
  if (parts < 1) parts = 1;
  P.run(parts, [&](int p) {
    const int64_t lo = n * p / parts, hi = n * (p + 1) / parts;
    if (op == 0) {
      memcpy(dst + lo, src + lo, (size_t)(hi - lo) * sizeof(double));
    } else if (op == 1) {
      for (int64_t i = lo; i < hi; ++i) dst[i] += src[i];
    } else {
      if (a == 0.0 && b == 0.0) memset(dst + lo, 0, (size_t)(hi - lo) * sizeof(double));   // no 0 * NaN
      else if (b == 0.0) for (int64_t i = lo; i < hi; ++i) dst[i] = a * src[i];
      else for (int64_t i = lo; i < hi; ++i) dst[i] = a * src[i] + b * dst[i];
    }
  });
}

// ----------------------------------------------------------------- block registry ----
struct HostBlock {
  char* base = nullptr;
  size_t bytes = 0;
  bool pooled = false;       // hipHostMalloc'ed by femo_host_alloc (else: hipHostRegister'ed user memory)
  // provenance: the first src_n doubles are an exact copy of device vector src_uid at generation src_gen
  // times src_scale (1 unless the block was filled by femo_host_axpby(a, x, 0, y) from a block that mirrors a vector:
  // the library then knows y = a * vector without looking at the bytes)
  uint64_t src_uid = 0, src_gen = 0;
  int64_t src_n = 0;
  double src_scale = 1.0;
  // ... or every one of the first const_n doubles equals const_value (femo_host_fill): sending the block is a device fill
  int64_t const_n = 0;
  double const_value = 0.0;
  // an asynchronous copy-out into the block is (or was) in flight: recorded on a copy stream after the DMA
  // (pend_ctx: the context whose copy stream carries it -- deferred host work is queued behind it there)
  hipEvent_t ready = nullptr;
  bool pending = false;
  femo_ctx* pend_ctx = nullptr;
  // promised (femo_vec_get_host_promised): pending, recorded as the mirror of (src_uid, src_gen, src_n), and the copy is
  // not enqueued yet -- `ready` has not been recorded for it.  Whoever needs the bytes sends it first (send_promised).
  bool promised = false;
};

std::mutex g_mu;
std::map<uintptr_t, HostBlock> g_blocks;                 // by base address
std::multimap<size_t, void*> g_free;                     // released pool blocks, kept pinned for reuse
size_t g_free_bytes = 0;
constexpr size_t FREE_CAP = size_t(6) << 30;
std::unordered_map<uint64_t, femo_vec*> g_live;          // uid -> vector (owned vectors only)
std::atomic<uint64_t> g_next_uid{0};
femo_host_stats g_stats = {};

HostBlock* find_block(const void* p, size_t bytes) {     // g_mu held
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = g_blocks.upper_bound(a);
  if (it == g_blocks.begin()) return nullptr;
  --it;
  HostBlock& b = it->second;
  if (a + bytes <= reinterpret_cast<uintptr_t>(b.base) + b.bytes) return &b;
  return nullptr;
}

// Does [p, p + bytes) share a byte with any known block?  (Blocks never intersect, so the only candidates are the first
// block that starts at or after p and the one before it.)
bool overlaps_block(const void* p, size_t bytes) {       // g_mu held
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = g_blocks.lower_bound(a);
  if (it != g_blocks.end() && it->first < a + bytes) return true;          // starts inside the range (or at its base)
  if (it == g_blocks.begin()) return false;
  --it;
  return a < reinterpret_cast<uintptr_t>(it->second.base) + it->second.bytes;   // the block before reaches into it
}

bool verify_enabled() { return getenv("FEMO_HOST_VERIFY") != nullptr; }

// Entries per chunk of a deferred upload (femo_vec_set_host_deferred), a multiple of 256; 0: one copy.  FEMO_H2D_CHUNK_MB
// in MiB, fractions allowed (the tests cut an 8 MB array into 1 MiB pieces); read once per upload, never per chunk.
constexpr double H2D_CHUNK_MB_DEFAULT = 64.0;             // the best of 16 / 32 / 64 at n = 215 (DESIGN_LOG.md R16)
int64_t h2d_chunk_entries() {
  double mb = H2D_CHUNK_MB_DEFAULT;
  if (const char* e = getenv("FEMO_H2D_CHUNK_MB")) {
    char* end = nullptr;
    const double v = strtod(e, &end);
    if (end != e && v >= 0.0 && v <= 65536.0) mb = v;
  }
  if (mb == 0.0) return 0;
  const int64_t n = (int64_t)(mb * 1048576.0 / sizeof(double)) / 256 * 256;
  return std::max<int64_t>(n, 256);
}

// The same for the streamed tail (femo_dRdf_cell_apply_T_add_to_host): FEMO_D2H_CHUNK_MB, read once per call; 0: the product
// and femo_vec_add_to_host as two steps.
constexpr double D2H_CHUNK_MB_DEFAULT = 64.0;
int64_t d2h_chunk_entries() {
  double mb = D2H_CHUNK_MB_DEFAULT;
  if (const char* e = getenv("FEMO_D2H_CHUNK_MB")) {
    char* end = nullptr;
    const double v = strtod(e, &end);
    if (end != e && v >= 0.0 && v <= 65536.0) mb = v;
  }
  if (mb == 0.0) return 0;
  const int64_t n = (int64_t)(mb * 1048576.0 / sizeof(double)) / 256 * 256;
  return std::max<int64_t>(n, 256);
}

// The taper of both plans (range_plan.h), read once per transfer.  FEMO_RANGE_FLOOR_MB: the size of the upload's last and of
// the download's first piece in MiB (fractions allowed; 0, or at least the chunk size: equal pieces as before);
// FEMO_RANGE_FACTOR: the ratio of neighbouring pieces inside the taper (below 2: equal pieces); FEMO_D2H_MAX_CHUNK_MB: up to
// where the download's ranges grow beyond FEMO_D2H_CHUNK_MB once they taper.  Defaults: DESIGN_LOG.md R30.
constexpr double RANGE_FLOOR_MB_DEFAULT = 8.0, D2H_MAX_CHUNK_MB_DEFAULT = 128.0;
constexpr int64_t RANGE_FACTOR_DEFAULT = 4;
struct RangeTaper { int64_t floor, factor, d2h_cap; };
int64_t mb_entries(const char* name, double mb) {
  if (const char* e = getenv(name)) {
    char* end = nullptr;
    const double v = strtod(e, &end);
    if (end != e && v >= 0.0 && v <= 65536.0) mb = v;
  }
  return (int64_t)(mb * 1048576.0 / sizeof(double));
}
RangeTaper range_taper() {
  RangeTaper t;
  t.floor = mb_entries("FEMO_RANGE_FLOOR_MB", RANGE_FLOOR_MB_DEFAULT);
  if (t.floor <= 0) t.floor = INT64_MAX / 2;             // no taper
  t.factor = RANGE_FACTOR_DEFAULT;
  if (const char* e = getenv("FEMO_RANGE_FACTOR")) t.factor = std::max(0, atoi(e));
  t.d2h_cap = mb_entries("FEMO_D2H_MAX_CHUNK_MB", D2H_MAX_CHUNK_MB_DEFAULT);
  return t;
}

// A copy-out is promised only from this size on.  Below it the copy costs no more than its own launch (1 MiB takes 19 us at
// the link's 56 GB/s), so keeping it off the link saves nothing, while a promise that has to be kept in front of a writer
// would put the copy and a wait of the compute stream where the eager copy had long landed; and a small result keeps
// arriving by itself for a caller that reads it at once.  (The threshold of the in-place pinning of caller arrays,
// engine.AUTO_REGISTER_MIN_BYTES; the deferred upload has one of its own, 8 MiB.)
constexpr int64_t PROMISE_MIN_BYTES = int64_t(1) << 20;

bool on_demand_enabled() {
  const char* e = getenv("FEMO_D2H_ON_DEMAND");
  return e == nullptr || strcmp(e, "0") != 0;
}

// The switch of the promises an output operator asks for (FEMO_PROMISE_OUTPUT: dJ/du, which goes straight back into the adjoint
// solve, and the explicit dJ/df, which the streamed tail overwrites from the device).  Its own switch, so that
// FEMO_D2H_ON_DEMAND=0 still measures the multiplier's copy alone.
bool promise_outputs_enabled() {
  const char* e = getenv("FEMO_D2H_PROMISE_OUTPUTS");
  return e == nullptr || strcmp(e, "0") != 0;
}

// events of blocks that left the registry, kept for the next block that needs one
std::vector<hipEvent_t> g_ev_free;

// Blocks released while a DMA still owned them (an array dropped with its copy-out or upload in flight).  femo_host_free
// does not wait for the transfer -- it would hold up the interpreter thread, and under g_mu every other caller of the
// pool: the block waits here, out of the registry, and the next pool call whose query finds the event complete recycles
// it.  A block never reaches g_free, and so never a new owner, before its last DMA is over.
struct LimboBlock { void* p; size_t bytes; hipEvent_t ready; };
std::vector<LimboBlock> g_limbo;

int64_t now_us() {
  return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Return block p to the recycled ones, making room under the cap first.  g_mu held; what has to be hipHostFree'd (outside the
// lock) goes to `evict`.
void recycle_block(void* p, size_t bytes, std::vector<void*>& evict);

void sweep_limbo(std::vector<void*>& evict) {            // g_mu held
  for (size_t i = 0; i < g_limbo.size();) {
    if (hipEventQuery(g_limbo[i].ready) != hipSuccess) { ++i; continue; }
    const LimboBlock lb = g_limbo[i];
    g_limbo[i] = g_limbo.back();
    g_limbo.pop_back();
    g_ev_free.push_back(lb.ready);
    recycle_block(lb.p, lb.bytes, evict);
  }
}

hipEvent_t take_event() {                                // g_mu held
  if (!g_ev_free.empty()) { hipEvent_t e = g_ev_free.back(); g_ev_free.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
  return e;
}

int ensure_copy_stream(femo_ctx* c) {
  if (c->copy_stream) return 0;
  FEMO_HIP_CHECK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  FEMO_HIP_CHECK(hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming));
  return 0;
}

// promised copy-outs ------------------------------------------------------------------
// (scale: the block was promised scale * v, femo_host_axpby(a, x, 0, y) from a promised x: the factor is applied on the host
// behind the copy, as it would have been had x travelled)
struct PromisedCopy { double* host; femo_vec* v; int64_t n; hipEvent_t ready; double scale; };
struct DeferredScale { double* y; const double* x; int64_t n; double a; };
void run_deferred_scale(void* p) {                       // hipLaunchHostFunc callback: host work only, no HIP calls
  DeferredScale* d = static_cast<DeferredScale*>(p);
  par_stream(d->y, d->x, d->n, 2, d->a, 0.0);
  delete d;
}

// The promise leaves block b: its copy is about to be enqueued (out != null) or will never be.  g_mu held.
bool take_promise(HostBlock& b, PromisedCopy* out) {
  if (!b.promised) return false;
  b.promised = false;
  auto it = g_live.find(b.src_uid);
  femo_vec* v = it != g_live.end() ? it->second : nullptr;
  if (v != nullptr && v->promises > 0) --v->promises;
  if (out != nullptr) *out = PromisedCopy{reinterpret_cast<double*>(b.base), v, b.src_n, b.ready, b.src_scale};
  return true;
}

// Nobody will read the block under p: the promise is dropped, the block holds nothing the library knows of.
void drop_promise(const void* p) {
  std::lock_guard<std::mutex> lk(g_mu);
  HostBlock* b = p ? find_block(p, 1) : nullptr;
  if (b != nullptr && take_promise(*b, nullptr)) { b->pending = false; b->src_uid = 0; }
}

// Exactly the copy the lazy branch of get_host_impl enqueues: behind everything on the compute stream so far, on the copy
// stream, followed by the block's and the vector's events.  The block stays pending; not under g_mu.
int send_promised(const PromisedCopy& pc) {
  femo_vec* v = pc.v;
  // every writer and femo_vec_destroy send a vector's promises first, so the vector of a promise is live and unchanged
  FEMO_REQUIRE(v != nullptr && pc.ready != nullptr, "a promised copy-out has lost its vector");
  femo_ctx* c = v->ctx;
  FEMO_HIP_CHECK(hipSetDevice(c->device));
  FEMO_TRY(ensure_copy_stream(c));
  FEMO_TRY(femo_vec_await(v));
  if (v->d2h_ev == nullptr) FEMO_HIP_CHECK(hipEventCreateWithFlags(&v->d2h_ev, hipEventDisableTiming));
  FEMO_HIP_CHECK(hipEventRecord(c->ev_copy, c->stream));
  FEMO_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0));
  FEMO_HIP_CHECK(hipMemcpyAsync(pc.host, v->d, pc.n * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
  FEMO_HIP_CHECK(hipEventRecord(v->d2h_ev, c->copy_stream));
  // (in place on the block, y == x: every entry is read and written once by the same thread of par_stream's op 2 with b = 0)
  if (pc.scale != 1.0) FEMO_HIP_CHECK(hipLaunchHostFunc(c->copy_stream, run_deferred_scale, new DeferredScale{pc.host, pc.host, pc.n, pc.scale}));
  FEMO_HIP_CHECK(hipEventRecord(pc.ready, c->copy_stream));
  v->d2h_pending = true;
  std::lock_guard<std::mutex> lk(g_mu);
  ++g_stats.d2h_async; g_stats.d2h_async_bytes += pc.n * 8;
  return 0;
}

// The bytes of the block under p are needed: if they were only promised, they leave now.
int resolve_block(const void* p) {
  PromisedCopy pc{};
  {
    std::lock_guard<std::mutex> lk(g_mu);
    HostBlock* b = p ? find_block(p, 1) : nullptr;
    if (b == nullptr || !take_promise(*b, &pc)) return 0;
  }
  return send_promised(pc);
}

// Wait until the asynchronous copy-out into the block containing p (if any) has landed.
int wait_block(const void* p) {
  FEMO_TRY(resolve_block(p));
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    HostBlock* b = p ? find_block(p, 1) : nullptr;
    if (b == nullptr || !b->pending) return 0;
    ev = b->ready;
  }
  FEMO_HIP_CHECK(hipEventSynchronize(ev));               // not under the lock: it can take milliseconds
  std::lock_guard<std::mutex> lk(g_mu);
  HostBlock* b = find_block(p, 1);
  if (b != nullptr && b->ready == ev && hipEventQuery(ev) == hipSuccess) b->pending = false;
  return 0;
}

// staging ring of the context -------------------------------------------------------
constexpr int64_t STAGE_DOUBLES = int64_t(1) << 20;     // 8 MiB per slot

int ensure_stage(femo_ctx* c) {
  if (c->stage[0]) return 0;
  for (int k = 0; k < FEMO_STAGE_SLOTS; ++k) {
    FEMO_HIP_CHECK(hipHostMalloc(&c->stage[k], STAGE_DOUBLES * sizeof(double), hipHostMallocDefault));
    FEMO_HIP_CHECK(hipEventCreateWithFlags(&c->stage_ev[k], hipEventDisableTiming));
  }
  return 0;
}

int h2d(femo_vec* v, const double* host, int64_t n, bool pinned) {
  femo_ctx* c = v->ctx;
  hipStream_t st = c->stream;
  if (pinned) {
    FEMO_HIP_CHECK(hipMemcpyAsync(v->d, host, n * sizeof(double), hipMemcpyHostToDevice, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
  }
  FEMO_TRY(ensure_stage(c));
  int64_t off = 0;
  for (int i = 0; off < n; ++i, off += STAGE_DOUBLES) {
    const int k = i % FEMO_STAGE_SLOTS;
    const int64_t len = std::min(STAGE_DOUBLES, n - off);
    if (i >= FEMO_STAGE_SLOTS) FEMO_HIP_CHECK(hipEventSynchronize(c->stage_ev[k]));   // the slot's previous DMA is done
    par_stream(c->stage[k], host + off, len, 0);
    FEMO_HIP_CHECK(hipMemcpyAsync(v->d + off, c->stage[k], len * sizeof(double), hipMemcpyHostToDevice, st));
    FEMO_HIP_CHECK(hipEventRecord(c->stage_ev[k], st));
  }
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

// host (op) device: op 0 assign, 1 accumulate
int d2h(const femo_vec* v, double* host, int64_t n, bool pinned, int op) {
  femo_ctx* c = v->ctx;
  hipStream_t st = c->stream;
  if (pinned && op == 0) {
    FEMO_HIP_CHECK(hipMemcpyAsync(host, v->d, n * sizeof(double), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
  }
  FEMO_TRY(ensure_stage(c));
  const int64_t nchunk = (n + STAGE_DOUBLES - 1) / STAGE_DOUBLES;
  auto issue = [&](int64_t i) -> int {
    const int k = (int)(i % FEMO_STAGE_SLOTS);
    const int64_t off = i * STAGE_DOUBLES, len = std::min(STAGE_DOUBLES, n - off);
    FEMO_HIP_CHECK(hipMemcpyAsync(c->stage[k], v->d + off, len * sizeof(double), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipEventRecord(c->stage_ev[k], st));
    return 0;
  };
  const int64_t ahead = FEMO_STAGE_SLOTS - 1;            // DMAs in flight while the host drains a slot
  for (int64_t i = 0; i < std::min(ahead, nchunk); ++i) FEMO_TRY(issue(i));
  for (int64_t i = 0; i < nchunk; ++i) {
    const int k = (int)(i % FEMO_STAGE_SLOTS);
    const int64_t off = i * STAGE_DOUBLES, len = std::min(STAGE_DOUBLES, n - off);
    FEMO_HIP_CHECK(hipEventSynchronize(c->stage_ev[k]));
    par_stream(host + off, c->stage[k], len, op);
    if (i + ahead < nchunk) FEMO_TRY(issue(i + ahead));  // the slot drained one step ago is free again
  }
  return 0;
}

}  // namespace

// -------------------------------------------------------- vector bookkeeping ----
void femo_vec_register(femo_vec* v) {
  v->uid = v->owned ? ++g_next_uid : 0;                  // wrapped memory has other writers: never trusted
  v->gen = 1;
  if (v->uid) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_live[v->uid] = v;
  }
}

void femo_vec_wait_readers(femo_vec* v) {
  // called by femo_vec_touch before a kernel that writes v is launched on the compute stream
  if (v->d2h_ev != nullptr) (void)hipStreamWaitEvent(v->ctx->stream, v->d2h_ev, 0);
  v->d2h_pending = false;
}

void femo_vec_resolve_promises(femo_vec* v) {
  // called by femo_vec_touch in front of a writer of v and by femo_vec_destroy: the content the blocks were promised leaves
  // first (the writer then waits for the copies through d2h_pending like for any copy-out in flight)
  std::vector<PromisedCopy> todo;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_blocks) {
      PromisedCopy pc{};
      if (kv.second.promised && kv.second.src_uid == v->uid && take_promise(kv.second, &pc)) todo.push_back(pc);
    }
    v->promises = 0;
  }
  for (const PromisedCopy& pc : todo) (void)send_promised(pc);
}

void femo_vec_unregister(femo_vec* v) {
  if (!v->uid) return;
  std::lock_guard<std::mutex> lk(g_mu);
  g_live.erase(v->uid);
}

femo_vec* femo_vec_live(uint64_t uid) {
  if (!uid) return nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_live.find(uid);
  return it == g_live.end() ? nullptr : it->second;
}

extern "C" {

// ------------------------------------------------------------ pinned blocks ----
int femo_host_alloc(int64_t bytes, void** out) {
  FEMO_REQUIRE(out != nullptr && bytes >= 0, "bad argument");
  *out = nullptr;
  const size_t need = (size_t)std::max<int64_t>(bytes, 8);
  std::vector<void*> evict;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_limbo.empty()) sweep_limbo(evict);
    auto it = g_free.find(need);
    if (it != g_free.end()) {
      *out = it->second;
      g_free.erase(it);
      g_free_bytes -= need;
      HostBlock b;
      b.base = static_cast<char*>(*out); b.bytes = need; b.pooled = true;
      g_blocks[reinterpret_cast<uintptr_t>(*out)] = b;
    }
  }
  for (void* q : evict) (void)hipHostFree(q);
  if (*out != nullptr) return 0;
  void* p = nullptr;
  const int64_t t0 = now_us();
  FEMO_HIP_CHECK(hipHostMalloc(&p, need, hipHostMallocDefault));
  const int64_t dt = now_us() - t0;
  HostBlock b;
  b.base = static_cast<char*>(p); b.bytes = need; b.pooled = true;
  std::lock_guard<std::mutex> lk(g_mu);
  ++g_stats.pool_fresh; g_stats.pool_fresh_us += dt;
  g_blocks[reinterpret_cast<uintptr_t>(p)] = b;
  *out = p;
  return 0;
}

namespace {
void recycle_block(void* p, size_t bytes, std::vector<void*>& evict) {
  // Over the cap: make room by dropping recycled blocks of OTHER sizes, largest first -- the size being freed now is the
  // one the running workload allocates again.  (Round 3 dropped the freed block itself: after a 10 M-DOF run had filled
  // the pool with 477 MB blocks, every result block of a smaller problem was hipHostMalloc'ed and hipHostFree'd again,
  // 50 ms per cycle of the 5 M-DOF configuration in bench.py.)
  while (g_free_bytes + bytes > FREE_CAP && !g_free.empty()) {
    auto victim = g_free.end();
    for (auto jt = g_free.rbegin(); jt != g_free.rend(); ++jt)
      if (jt->first != bytes) { victim = std::next(jt).base(); break; }
    if (victim == g_free.end()) break;
    evict.push_back(victim->second);
    g_free_bytes -= victim->first;
    g_free.erase(victim);
  }
  if (g_free_bytes + bytes <= FREE_CAP) {
    g_free.emplace(bytes, p);
    g_free_bytes += bytes;
  } else {
    evict.push_back(p);
  }
}
}  // namespace

int femo_host_free(void* p) {
  if (!p) return 0;
  std::vector<void*> evict;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_blocks.find(reinterpret_cast<uintptr_t>(p));
    FEMO_REQUIRE(it != g_blocks.end() && it->second.pooled, "femo_host_free: not a block of femo_host_alloc");
    const size_t bytes = it->second.bytes;
    if (take_promise(it->second, nullptr)) it->second.pending = false;   // nobody can read the block any more
    const hipEvent_t ready = it->second.ready;
    // the DMA still owns the block: it comes back through g_limbo, never by waiting here under the lock
    const bool in_flight = ready != nullptr && it->second.pending && hipEventQuery(ready) != hipSuccess;
    g_blocks.erase(it);
    if (!g_limbo.empty()) sweep_limbo(evict);
    if (in_flight) {
      g_limbo.push_back(LimboBlock{p, bytes, ready});
      ++g_stats.pool_free_deferred;
    } else {
      if (ready != nullptr) g_ev_free.push_back(ready);
      recycle_block(p, bytes, evict);
    }
  }
  for (void* q : evict) (void)hipHostFree(q);
  return 0;
}

int femo_host_trim(void) {
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_limbo.empty()) sweep_limbo(drop);             // (blocks still in flight stay: their DMA owns them)
    for (auto& kv : g_free) drop.push_back(kv.second);
    g_free.clear();
    g_free_bytes = 0;
  }
  for (void* p : drop) (void)hipHostFree(p);
  return 0;
}

int femo_host_register(void* p, int64_t bytes) {
  FEMO_REQUIRE(p != nullptr && bytes > 0, "bad argument");
  {
    std::lock_guard<std::mutex> lk(g_mu);
    FEMO_REQUIRE(!overlaps_block(p, (size_t)bytes), "femo_host_register: range is already pinned");
  }
  FEMO_HIP_CHECK(hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault));
  HostBlock b;
  b.base = static_cast<char*>(p); b.bytes = (size_t)bytes; b.pooled = false;
  std::lock_guard<std::mutex> lk(g_mu);
  g_blocks[reinterpret_cast<uintptr_t>(p)] = b;
  return 0;
}

int femo_host_unregister(void* p) {
  hipEvent_t in_flight = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_blocks.find(reinterpret_cast<uintptr_t>(p));
    FEMO_REQUIRE(it != g_blocks.end() && !it->second.pooled, "femo_host_unregister: not a registered range");
    if (it->second.ready != nullptr && it->second.pending) in_flight = it->second.ready;
  }
  if (in_flight != nullptr) {
    // not under the lock: the range's owner is the one who waits (caller memory cannot be parked: it is about to be freed)
    const int64_t t0 = now_us();
    (void)hipEventSynchronize(in_flight);
    const int64_t dt = now_us() - t0;
    std::lock_guard<std::mutex> lk(g_mu);
    ++g_stats.pool_free_waited; g_stats.pool_free_waited_us += dt;
  }
  // The record goes only once the runtime has let go of the range: if it refuses, the range is still pinned for it, and a
  // registry that had forgotten it would hand the next array at this address to the staged path as if it were pageable.
  FEMO_HIP_CHECK(hipHostUnregister(p));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_blocks.find(reinterpret_cast<uintptr_t>(p));
  if (it != g_blocks.end() && !it->second.pooled) {
    if (it->second.ready != nullptr) g_ev_free.push_back(it->second.ready);
    g_blocks.erase(it);
  }
  return 0;
}

int femo_host_touch(void* p) {
  if (!p) return 0;
  FEMO_TRY(wait_block(p));                               // the caller is about to write (or has read) the block
  std::lock_guard<std::mutex> lk(g_mu);
  if (HostBlock* b = find_block(p, 1)) { b->src_uid = 0; b->const_n = 0; }
  return 0;
}

int femo_host_is_pinned(const void* p, int64_t bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  return find_block(p, (size_t)std::max<int64_t>(bytes, 1)) != nullptr ? 1 : 0;
}

int femo_host_threads(void) { return HostPool::get().threads(); }

int femo_host_fill(double* p, int64_t n, double value) {
  FEMO_REQUIRE(p || n == 0, "null argument");
  if (n == 0) return 0;
  FEMO_TRY(wait_block(p));
  HostPool& P = HostPool::get();
  const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(P.threads(), n >> 16));
  P.run(parts, [&](int k) {
    const int64_t lo = n * k / parts, hi = n * (k + 1) / parts;
    for (int64_t i = lo; i < hi; ++i) p[i] = value;
  });
  std::lock_guard<std::mutex> lk(g_mu);
  if (HostBlock* b = find_block(p, (size_t)n * sizeof(double))) {
    b->src_uid = 0;
    if (reinterpret_cast<char*>(p) == b->base && b->pooled) { b->const_n = n; b->const_value = value; }
    else b->const_n = 0;
  }
  return 0;
}

int femo_host_copy(double* dst, const double* src, int64_t n) {
  FEMO_REQUIRE((dst && src) || n == 0, "null argument");
  FEMO_TRY(wait_block(src));
  FEMO_TRY(wait_block(dst));
  par_stream(dst, src, n, 0);
  femo_host_touch(dst);
  return 0;
}

int femo_host_axpby(int64_t n, double a, const double* x, double b, double* y) {
  FEMO_REQUIRE((x && y) || n == 0, "null argument");
  if (n == 0) return 0;
  if (b == 0.0 && x != y) drop_promise(y);               // overwritten whole: what it was promised need not travel
  FEMO_TRY(wait_block(y));
  // y = a x with x a block that was only PROMISED the content of a live vector: y is promised a times that vector, and
  // nothing is read or sent.  (The reverse sweep negates dJ/du this way; the adjoint solve takes the seed from the device.)
  if (b == 0.0 && a != 0.0 && x != y) {
    std::lock_guard<std::mutex> lk(g_mu);
    HostBlock* bx = find_block(x, (size_t)n * sizeof(double));
    HostBlock* by = find_block(y, (size_t)n * sizeof(double));
    if (bx && by && bx != by && by->pooled && bx->promised && !by->pending && reinterpret_cast<const char*>(x) == bx->base &&
        reinterpret_cast<char*>(y) == by->base && bx->src_uid != 0 && bx->src_n == n) {
      auto it = g_live.find(bx->src_uid);
      if (it != g_live.end() && it->second->gen == bx->src_gen && by->ready == nullptr) by->ready = take_event();
      if (it != g_live.end() && it->second->gen == bx->src_gen && by->ready != nullptr) {
        by->src_uid = bx->src_uid; by->src_gen = bx->src_gen; by->src_n = n; by->src_scale = a * bx->src_scale; by->const_n = 0;
        by->pending = true; by->pend_ctx = bx->pend_ctx; by->promised = true;
        ++it->second->promises;
        return 0;
      }
    }
  }
  FEMO_TRY(resolve_block(x));                            // x is read below, at once or behind its copy
  // y = a x with x a block that mirrors a device vector: y is then known to be a * that vector without its bytes
  // (femo_vec_set_host from y becomes a device-side scale).  If x is still on its way down the host pass is queued
  // behind the copy on the same stream instead of waiting for it here -- the reverse sweep negates dJ/du this way
  // and goes on to enqueue the adjoint solve.
  if (b == 0.0 && a != 0.0 && x != y) {
    uint64_t uid = 0, gen = 0;
    double scale = 1.0;
    bool x_pending = false;
    femo_ctx* pctx = nullptr;
    hipEvent_t y_ready = nullptr, x_ready = nullptr;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      HostBlock* bx = find_block(x, (size_t)n * sizeof(double));
      HostBlock* by = find_block(y, (size_t)n * sizeof(double));
      if (bx && by && by->pooled && reinterpret_cast<const char*>(x) == bx->base && reinterpret_cast<char*>(y) == by->base && bx->src_uid != 0 &&
          bx->src_n >= n) {
        auto it = g_live.find(bx->src_uid);
        if (it != g_live.end() && it->second->gen == bx->src_gen) {
          uid = bx->src_uid; gen = bx->src_gen; scale = bx->src_scale;
          x_pending = bx->pending && bx->pend_ctx != nullptr && bx->pend_ctx->copy_stream != nullptr;
          pctx = bx->pend_ctx;
          if (x_pending) {
            if (by->ready == nullptr) by->ready = take_event();
            y_ready = by->ready;
            x_ready = bx->ready;
          }
        }
      }
    }
    if (uid != 0) {
      if (x_pending && y_ready != nullptr) {
        FEMO_HIP_CHECK(hipSetDevice(pctx->device));
        FEMO_HIP_CHECK(hipLaunchHostFunc(pctx->copy_stream, run_deferred_scale, new DeferredScale{y, x, n, a}));
        FEMO_HIP_CHECK(hipEventRecord(y_ready, pctx->copy_stream));
        // x stays "in flight" until the pass that reads it has run: freeing its block waits for this event
        if (x_ready != nullptr) FEMO_HIP_CHECK(hipEventRecord(x_ready, pctx->copy_stream));
      } else {
        FEMO_TRY(wait_block(x));
        par_stream(y, x, n, 2, a, 0.0);
      }
      std::lock_guard<std::mutex> lk(g_mu);
      if (HostBlock* by = find_block(y, (size_t)n * sizeof(double))) {
        by->src_uid = uid; by->src_gen = gen; by->src_n = n; by->src_scale = a * scale; by->const_n = 0;
        if (x_pending && y_ready != nullptr) { by->pending = true; by->pend_ctx = pctx; }
      }
      return 0;
    }
  }
  FEMO_TRY(wait_block(x));
  par_stream(y, x, n, 2, a, b);
  femo_host_touch(y);
  return 0;
}

int femo_host_get_stats(femo_host_stats* out) {
  FEMO_REQUIRE(out != nullptr, "null argument");
  std::lock_guard<std::mutex> lk(g_mu);
  *out = g_stats;
  return 0;
}

int femo_host_reset_stats(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_stats = femo_host_stats{};
  return 0;
}

// ----------------------------------------------------------------- transfers ----
int femo_vec_set_host(femo_vec* v, const double* host, int64_t n) {
  FEMO_REQUIRE(v && host, "null argument");
  FEMO_REQUIRE(n == v->n, "size mismatch: vector has %lld entries, host array %lld", (long long)v->n, (long long)n);
  if (n == 0) return 0;
  FEMO_HIP_CHECK(hipSetDevice(v->ctx->device));
  bool pinned = false, exact_base = false, is_const = false;
  double const_value = 0.0;
  uint64_t src_uid = 0, src_gen = 0;
  double src_scale = 1.0;
  femo_vec* src = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) {
      pinned = true;
      exact_base = reinterpret_cast<const char*>(host) == b->base;
      if (exact_base && b->const_n >= n) { is_const = true; const_value = b->const_value; }
      if (exact_base && b->src_uid != 0 && b->src_n >= n) {
        src_uid = b->src_uid; src_gen = b->src_gen; src_scale = b->src_scale;
        auto it = g_live.find(src_uid);
        if (it != g_live.end() && it->second->gen == src_gen && it->second->ctx->device == v->ctx->device) src = it->second;
      }
    }
  }
  int elided = 0;
  if (src != nullptr && src == v && src_scale == 1.0) {
    elided = 1;                                          // v still holds exactly this content
  } else if (is_const && (src == nullptr || src != v)) {
    femo_vec_touch(v);
    FEMO_TRY(femo_launch_fill(v->d, const_value, n, v->ctx->stream));   // the block is a constant: fill on the device
    src = nullptr;
    elided = 2;
  } else if (src != nullptr && src == v) {
    src = nullptr;                                       // a * v into v itself: not worth a special case, upload
  } else if (src != nullptr && src_scale != 1.0) {
    femo_vec_touch(v);
    FEMO_TRY(femo_launch_scale(v->d, src_scale, src->d, n, v->ctx->stream));   // host = scale * src: the same product on the device
    if (src->ctx != v->ctx) FEMO_HIP_CHECK(hipStreamSynchronize(v->ctx->stream));
    elided = 2;
  } else if (src != nullptr) {
    femo_vec_touch(v);                                   // before the write: a copy-out of v may be in flight
    FEMO_HIP_CHECK(hipMemcpyAsync(v->d, src->d, n * sizeof(double), hipMemcpyDeviceToDevice, v->ctx->stream));
    if (src->ctx != v->ctx) FEMO_HIP_CHECK(hipStreamSynchronize(v->ctx->stream));
    elided = 2;
  }
  if (!elided || verify_enabled()) FEMO_TRY(wait_block(host));   // the bytes themselves are needed
  if (elided && verify_enabled()) {
    std::vector<double> chk((size_t)n);
    FEMO_HIP_CHECK(hipStreamSynchronize(v->ctx->stream));   // the fill / scale / copy above runs on a non-blocking stream
    FEMO_HIP_CHECK(hipMemcpy(chk.data(), v->d, n * sizeof(double), hipMemcpyDeviceToHost));
    FEMO_REQUIRE(memcmp(chk.data(), host, (size_t)n * sizeof(double)) == 0,
                 "FEMO_HOST_VERIFY: an elided upload (kind %d) would have changed the vector", elided);
  }
  if (!elided) {
    femo_vec_touch(v);
    FEMO_TRY(h2d(v, host, n, pinned));
  }
  std::lock_guard<std::mutex> lk(g_mu);
  if (elided == 1) { ++g_stats.h2d_skipped; g_stats.h2d_skipped_bytes += n * 8; }
  else if (elided == 2) { ++g_stats.h2d_as_d2d; g_stats.h2d_as_d2d_bytes += n * 8; }
  else if (pinned) { ++g_stats.h2d_pinned; g_stats.h2d_pinned_bytes += n * 8; }
  else { ++g_stats.h2d_staged; g_stats.h2d_staged_bytes += n * 8; }
  if (exact_base && v->uid != 0) {                       // the block is now an exact copy of v
    if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) {
      // (a promised block keeps the vector that owes it the bytes)
      if (reinterpret_cast<const char*>(host) == b->base && b->pooled && !b->promised) { b->src_uid = v->uid; b->src_gen = v->gen; b->src_n = n; b->src_scale = 1.0; }
    }
  }
  return 0;
}

// Deferred upload: the copy runs on the context's copy stream and the call returns at once.  Only from a whole pooled
// block of femo_host_alloc (its writers announce themselves, and femo_host_touch / femo_host_free wait for the copy);
// every other case -- elisions, caller-owned memory, pageable memory -- is the synchronous femo_vec_set_host.  The compute
// stream waits in femo_vec_await, which every writer of v calls through femo_vec_touch and which the assembly entry points
// call for their inputs; a driver that defers uploads awaits them before anything else reads the vector
// (engine.deferred_uploads).  Replaces the same copy of utils_dolfinx.py:300-311.
int femo_vec_set_host_deferred(femo_vec* v, const double* host, int64_t n) {
  FEMO_REQUIRE(v && host, "null argument");
  FEMO_REQUIRE(n == v->n, "size mismatch: vector has %lld entries, host array %lld", (long long)v->n, (long long)n);
  bool ok = false;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) {
      const bool exact = reinterpret_cast<const char*>(host) == b->base;
      bool mirrors_live = false;
      if (exact && b->src_uid != 0 && b->src_n >= n) {
        auto it = g_live.find(b->src_uid);
        mirrors_live = it != g_live.end() && it->second->gen == b->src_gen;
      }
      ok = exact && b->pooled && !b->pending && b->const_n < n && !mirrors_live && n * (int64_t)sizeof(double) >= (8 << 20);
    }
  }
  if (!ok || verify_enabled()) return femo_vec_set_host(v, host, n);
  femo_ctx* c = v->ctx;
  FEMO_HIP_CHECK(hipSetDevice(c->device));
  FEMO_TRY(ensure_copy_stream(c));
  femo_vec_touch(v);                                     // earlier copy-outs / uploads of v first; new generation
  if (v->h2d_ev == nullptr) FEMO_HIP_CHECK(hipEventCreateWithFlags(&v->h2d_ev, hipEventDisableTiming));
  // The copy travels in chunks, each followed by an event of its own, so that a reader which needs only a prefix of v can
  // start on it (femo_vec_await_prefix: the streamed head of femo_newton_rhs_linear).  The last chunk's event is h2d_ev:
  // femo_vec_await, the block's `ready` event and the provenance below see one upload that is over when all of it is.
  // ... and the pieces shrink towards the end (range_plan.h): only the last one's kernels stand behind the last byte.
  const RangeTaper tp = range_taper();
  const auto plan = femo_range_plan(n, h2d_chunk_entries(), FEMO_TAPER_HEAD, tp.floor, tp.factor, 0);
  const int n_chunks = (int)plan.size();
  while ((int)v->h2d_chunk_ev.size() < n_chunks - 1) {   // kept with the vector: none is created in a warmed-up cycle
    hipEvent_t e = nullptr;
    FEMO_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    v->h2d_chunk_ev.push_back(e);
  }
  hipEvent_t ready = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    HostBlock* b = find_block(host, (size_t)n * sizeof(double));
    if (b->ready == nullptr) b->ready = take_event();
    ready = b->ready;
  }
  FEMO_REQUIRE(ready != nullptr, "could not create an event");
  FEMO_HIP_CHECK(hipEventRecord(c->ev_copy, c->stream));           // kernels enqueued so far may still read v
  FEMO_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0));
  v->h2d_ends.clear();
  for (int k = 0; k < n_chunks; ++k) {
    const int64_t lo = plan[(size_t)k].first, hi = plan[(size_t)k].second;
    FEMO_HIP_CHECK(hipMemcpyAsync(v->d + lo, host + lo, (hi - lo) * sizeof(double), hipMemcpyHostToDevice, c->copy_stream));
    if (k < n_chunks - 1) FEMO_HIP_CHECK(hipEventRecord(v->h2d_chunk_ev[k], c->copy_stream));
    v->h2d_ends.push_back(hi);
  }
  FEMO_HIP_CHECK(hipEventRecord(ready, c->copy_stream));
  FEMO_HIP_CHECK(hipEventRecord(v->h2d_ev, c->copy_stream));
  v->h2d_chunks = n_chunks;
  v->h2d_pending = true;
  std::lock_guard<std::mutex> lk(g_mu);
  ++g_stats.h2d_pinned; g_stats.h2d_pinned_bytes += n * 8;
  ++g_stats.h2d_deferred; g_stats.h2d_deferred_bytes += n * 8;
  g_stats.h2d_chunks += n_chunks;
  if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) {
    b->pending = true; b->pend_ctx = c;
    if (v->uid != 0) { b->src_uid = v->uid; b->src_gen = v->gen; b->src_n = n; b->src_scale = 1.0; }
  }
  return 0;
}

int femo_vec_await(const femo_vec* v_) {
  femo_vec* v = const_cast<femo_vec*>(v_);
  if (!v || !v->h2d_pending) return 0;
  v->h2d_pending = false;
  FEMO_HIP_CHECK(hipStreamWaitEvent(v->ctx->stream, v->h2d_ev, 0));
  return 0;
}

int femo_vec_await_prefix(const femo_vec* v_, int64_t n_entries) {
  femo_vec* v = const_cast<femo_vec*>(v_);
  if (!v || !v->h2d_pending || n_entries <= 0) return 0;
  // the first chunk that ends at or behind entry n_entries
  const int64_t k = v->h2d_chunks > 1 ? std::lower_bound(v->h2d_ends.begin(), v->h2d_ends.end(), n_entries) - v->h2d_ends.begin() : 0;
  if (k >= v->h2d_chunks - 1) return femo_vec_await(v);  // the last chunk, or a single copy: all of it
  FEMO_HIP_CHECK(hipStreamWaitEvent(v->ctx->stream, v->h2d_chunk_ev[(size_t)k], 0));
  return 0;
}

int femo_vec_await_upload(const femo_vec* v) {
  FEMO_REQUIRE(v != nullptr, "null argument");
  return femo_vec_await(v);
}

// op 0: host = v; op 1: host += v.  lazy: return before the bytes have landed (pinned blocks, op 0 only).
static int get_host_impl(const femo_vec* v, double* host, int64_t n, int op, bool lazy) {
  FEMO_REQUIRE(v && host, "null argument");
  FEMO_REQUIRE(n <= v->n, "size mismatch: vector has %lld entries, host array %lld", (long long)v->n, (long long)n);
  if (n == 0) return 0;
  femo_ctx* c = v->ctx;
  FEMO_HIP_CHECK(hipSetDevice(c->device));
  FEMO_TRY(femo_vec_await(v));                           // a deferred upload of v must have landed before it is read back
  if (op == 0) {
    drop_promise(host);                                  // overwritten whole: what it was promised need not travel
  } else if (!verify_enabled()) {                        // (the verifier compares the block's bytes: it keeps the promise)
    // accumulate into a block that was only promised the unscaled content of a live vector of this context: the sum below is
    // formed from that vector on the device, so the promise is dropped, not kept (the record stays for the mirror test below)
    std::lock_guard<std::mutex> lk(g_mu);
    HostBlock* b = find_block(host, (size_t)n * sizeof(double));
    if (b != nullptr && b->promised && b->pooled && reinterpret_cast<char*>(host) == b->base && b->src_n >= n && b->src_scale == 1.0) {
      auto it = g_live.find(b->src_uid);
      if (it != g_live.end() && it->second->gen == b->src_gen && it->second->ctx == c && take_promise(*b, nullptr)) b->pending = false;
    }
  }
  FEMO_TRY(wait_block(host));                            // an earlier copy-out into the block must not land after this one
  bool pinned = false, exact_base = false;
  femo_vec* mirror = nullptr;                            // live vector the block is an exact copy of (op 1)
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) {
      pinned = true;
      exact_base = reinterpret_cast<char*>(host) == b->base;
      // only an UNSCALED mirror: a block recorded as a * vector (femo_host_axpby) holds a * mirror, not mirror
      if (op == 1 && exact_base && b->src_uid != 0 && b->src_n >= n && b->src_scale == 1.0) {
        auto it = g_live.find(b->src_uid);
        if (it != g_live.end() && it->second->gen == b->src_gen && it->second->ctx == c) mirror = it->second;
      }
      b->src_uid = 0;                                    // being overwritten
      b->const_n = 0;
    }
  }
  if (op == 1 && mirror != nullptr) {
    // host holds exactly mirror's content: host + v = mirror + v, formed on the device and copied out at DMA rate
    if (verify_enabled()) {
      std::vector<double> chk((size_t)n);
      FEMO_HIP_CHECK(hipStreamSynchronize(c->stream));
      FEMO_HIP_CHECK(hipMemcpy(chk.data(), mirror->d, n * sizeof(double), hipMemcpyDeviceToHost));
      FEMO_REQUIRE(memcmp(chk.data(), host, (size_t)n * sizeof(double)) == 0,
                   "FEMO_HOST_VERIFY: the block no longer holds the vector it is recorded to mirror");
    }
    if (c->accum_n < n) {
      FEMO_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (c->d_accum) FEMO_HIP_CHECK(hipFree(c->d_accum));
      c->d_accum = nullptr; c->accum_n = 0;
      FEMO_HIP_CHECK(hipMalloc(&c->d_accum, (size_t)n * sizeof(double)));
      c->accum_n = n;
    }
    FEMO_TRY(femo_launch_sum(c->d_accum, mirror->d, v->d, n, c->stream));
    FEMO_HIP_CHECK(hipMemcpyAsync(host, c->d_accum, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEMO_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lk(g_mu);
    ++g_stats.d2h_device_sum; g_stats.d2h_device_sum_bytes += n * 8;
    return 0;
  }
  if (lazy && pinned && op == 0) {
    FEMO_TRY(ensure_copy_stream(c));
    femo_vec* vv = const_cast<femo_vec*>(v);
    if (vv->d2h_ev == nullptr) FEMO_HIP_CHECK(hipEventCreateWithFlags(&vv->d2h_ev, hipEventDisableTiming));
    hipEvent_t ready = nullptr;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      HostBlock* b = find_block(host, (size_t)n * sizeof(double));
      if (b->ready == nullptr) b->ready = take_event();
      ready = b->ready;
    }
    FEMO_REQUIRE(ready != nullptr, "could not create an event");
    FEMO_HIP_CHECK(hipEventRecord(c->ev_copy, c->stream));           // everything enqueued so far produced v
    FEMO_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0));
    FEMO_HIP_CHECK(hipMemcpyAsync(host, v->d, n * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
    FEMO_HIP_CHECK(hipEventRecord(ready, c->copy_stream));
    FEMO_HIP_CHECK(hipEventRecord(vv->d2h_ev, c->copy_stream));
    vv->d2h_pending = true;
    std::lock_guard<std::mutex> lk(g_mu);
    ++g_stats.d2h_async; g_stats.d2h_async_bytes += n * 8;
    if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) {
      b->pending = true;
      b->pend_ctx = c;
      if (exact_base && v->uid != 0 && b->pooled) { b->src_uid = v->uid; b->src_gen = v->gen; b->src_n = n; b->src_scale = 1.0; }   // true once landed
    }
    return 0;
  }
  FEMO_TRY(d2h(v, host, n, pinned, op));
  std::lock_guard<std::mutex> lk(g_mu);
  if (pinned && op == 0) { ++g_stats.d2h_pinned; g_stats.d2h_pinned_bytes += n * 8; }
  else { ++g_stats.d2h_staged; g_stats.d2h_staged_bytes += n * 8; }
  if (pinned && op == 0 && v->uid != 0) {
    if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) {
      if (reinterpret_cast<char*>(host) == b->base && b->pooled) { b->src_uid = v->uid; b->src_gen = v->gen; b->src_n = n; b->src_scale = 1.0; }
    }
  }
  return 0;
}

int femo_vec_get_host(const femo_vec* v, double* host, int64_t n) { return get_host_impl(v, host, n, 0, false); }

int femo_vec_get_host_async(const femo_vec* v, double* host, int64_t n) { return get_host_impl(v, host, n, 0, true); }

int femo_vec_add_to_host(const femo_vec* v, double* host, int64_t n) { return get_host_impl(v, host, n, 1, false); }

// host = v, but only on demand: the block is recorded as the copy of v at its present generation and marked pending, and the
// copy itself is enqueued by whoever first needs the bytes (wait_block, femo_host_sync) or is about to change v
// (femo_vec_touch, femo_vec_destroy).  Only into a whole pooled block from an owned vector, from PROMISE_MIN_BYTES on; anything
// else, and FEMO_D2H_ON_DEMAND=0, is femo_vec_get_host_async.
static int get_host_promised_impl(const femo_vec* v, double* host, int64_t n, int flags) {
  FEMO_REQUIRE(v && host, "null argument");
  FEMO_REQUIRE(n <= v->n, "size mismatch: vector has %lld entries, host array %lld", (long long)v->n, (long long)n);
  if (n == 0) return 0;
  const bool enabled = (flags & FEMO_PROMISE_OUTPUT) ? promise_outputs_enabled() : on_demand_enabled();
  bool ok = v->uid != 0 && enabled && n * (int64_t)sizeof(double) >= PROMISE_MIN_BYTES;
  if (ok) {
    std::lock_guard<std::mutex> lk(g_mu);
    HostBlock* b = find_block(host, (size_t)n * sizeof(double));
    ok = b != nullptr && b->pooled && reinterpret_cast<char*>(host) == b->base;
  }
  if (!ok) return get_host_impl(v, host, n, 0, true);
  drop_promise(host);                                    // the target of another copy-out: what it was promised before need not travel
  FEMO_TRY(wait_block(host));                            // an earlier copy-out into the block must not land after this one
  femo_vec* vv = const_cast<femo_vec*>(v);
  std::lock_guard<std::mutex> lk(g_mu);
  HostBlock* b = find_block(host, (size_t)n * sizeof(double));
  FEMO_REQUIRE(b != nullptr, "the block left the registry");
  if (b->ready == nullptr) b->ready = take_event();
  FEMO_REQUIRE(b->ready != nullptr, "could not create an event");
  b->src_uid = v->uid; b->src_gen = v->gen; b->src_n = n; b->src_scale = 1.0; b->const_n = 0;
  b->pending = true; b->pend_ctx = v->ctx; b->promised = true;
  ++vv->promises;
  return 0;
}

int femo_vec_get_host_promised(const femo_vec* v, double* host, int64_t n) { return get_host_promised_impl(v, host, n, 0); }

int femo_vec_get_host_promised_ex(const femo_vec* v, double* host, int64_t n, int flags) {
  FEMO_REQUIRE((flags & ~FEMO_PROMISE_OUTPUT) == 0, "femo_vec_get_host_promised_ex: unknown flag");
  return get_host_promised_impl(v, host, n, flags);
}

int femo_host_forget(const void* p) {
  drop_promise(p);
  return 0;
}

int femo_host_wait(const void* p) { return wait_block(p); }

// host += (dR/df)^T x for the one-value-per-cell dR/df (femo_dRdf_cell_apply, transposed), the statement that ends a reverse
// sweep.  Where host is a whole pooled block that is the unscaled exact copy of a live vector e of this context -- the condition
// of the device sum in get_host_impl -- and the mesh lives on one rank, the cells are walked in ranges of FEMO_D2H_CHUNK_MB:
// one launch forms e + (dR/df)^T x for a range in d_accum, an event follows it on the compute stream, and the range's
// copy goes out on the copy stream behind that event while the next range is computed.  One wait at the end.  Everything
// else is the product into y followed by femo_vec_add_to_host, as before; y is scratch either way.
int femo_dRdf_cell_apply_T_add_to_host(femo_mesh* m, const femo_vec* cvals, const femo_vec* x, femo_vec* y, double* host, int64_t n) {
  FEMO_REQUIRE(m && cvals && x && y && host, "null argument");
  FEMO_REQUIRE(n == m->n_cell && cvals->n >= n && y->n >= n && x->n >= m->n_vert, "vector size mismatch in dRdf^T apply");
  femo_ctx* c = m->ctx;
  const int64_t chunk_env = d2h_chunk_entries();         // read once per call
  femo_vec* mirror = nullptr;
  if (chunk_env > 0 && n > 0 && c->nranks == 1 && m->n_nbr == 0 && cvals->ctx == c && x->ctx == c) {
    std::lock_guard<std::mutex> lk(g_mu);
    HostBlock* b = find_block(host, (size_t)n * sizeof(double));
    if (b != nullptr && b->pooled && reinterpret_cast<char*>(host) == b->base && b->src_uid != 0 && b->src_n >= n && b->src_scale == 1.0) {
      auto it = g_live.find(b->src_uid);
      if (it != g_live.end() && it->second->gen == b->src_gen && it->second->ctx == c) mirror = it->second;
    }
  }
  if (mirror == nullptr) {
    ++m->tail_plain;
    FEMO_TRY(femo_dRdf_cell_apply(m, cvals, 1, x, y, 0));
    return femo_vec_add_to_host(y, host, n);
  }
  FEMO_HIP_CHECK(hipSetDevice(c->device));
  FEMO_TRY(femo_vec_await(cvals));
  FEMO_TRY(femo_vec_await(x));
  FEMO_TRY(femo_vec_await(mirror));
  if (!verify_enabled()) drop_promise(host);             // its content is read from the vector it mirrors, never from the block
  FEMO_TRY(wait_block(host));                            // an earlier copy-out into the block must not land after this one
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (HostBlock* b = find_block(host, (size_t)n * sizeof(double))) { b->src_uid = 0; b->const_n = 0; }   // being overwritten
  }
  if (verify_enabled()) {
    std::vector<double> chk((size_t)n);
    FEMO_HIP_CHECK(hipStreamSynchronize(c->stream));
    FEMO_HIP_CHECK(hipMemcpy(chk.data(), mirror->d, n * sizeof(double), hipMemcpyDeviceToHost));
    FEMO_REQUIRE(memcmp(chk.data(), host, (size_t)n * sizeof(double)) == 0,
                 "FEMO_HOST_VERIFY: the block no longer holds the vector it is recorded to mirror");
  }
  if (c->accum_n < n) {
    FEMO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->d_accum) FEMO_HIP_CHECK(hipFree(c->d_accum));
    c->d_accum = nullptr; c->accum_n = 0;
    FEMO_HIP_CHECK(hipMalloc(&c->d_accum, (size_t)n * sizeof(double)));
    c->accum_n = n;
  }
  FEMO_TRY(ensure_copy_stream(c));
  // short ranges first, so that the first byte leaves early, then longer ones than a chunk: fewer gaps (range_plan.h)
  const RangeTaper tp = range_taper();
  const auto plan = femo_range_plan(n, chunk_env, FEMO_TAPER_TAIL, tp.floor, tp.factor, tp.d2h_cap);
  const int n_ranges = (int)plan.size();
  while ((int)c->d2h_chunk_ev.size() < n_ranges) {       // kept with the context: none is created in a warmed-up cycle
    hipEvent_t e = nullptr;
    FEMO_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->d2h_chunk_ev.push_back(e);
  }
  for (int k = 0; k < n_ranges; ++k) {
    const int64_t lo = plan[(size_t)k].first, hi = plan[(size_t)k].second;
    FEMO_TRY(femo_launch_dRdf_cell_apply_T_sum(m, cvals->d, x->d, mirror->d, c->d_accum, lo, hi));
    FEMO_HIP_CHECK(hipEventRecord(c->d2h_chunk_ev[(size_t)k], c->stream));
    FEMO_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, c->d2h_chunk_ev[(size_t)k], 0));
    FEMO_HIP_CHECK(hipMemcpyAsync(host + lo, c->d_accum + lo, (hi - lo) * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
  }
  // the one wait: every range has landed, and d_accum may be rewritten by the next call
  FEMO_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
  ++m->tail_streamed; m->tail_ranges += n_ranges;
  std::lock_guard<std::mutex> lk(g_mu);
  ++g_stats.d2h_device_sum; g_stats.d2h_device_sum_bytes += n * 8;
  return 0;
}

int femo_host_sync(void) {
  std::vector<PromisedCopy> todo;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_blocks) {
      PromisedCopy pc{};
      if (take_promise(kv.second, &pc)) todo.push_back(pc);
    }
  }
  for (const PromisedCopy& pc : todo) FEMO_TRY(send_promised(pc));
  std::vector<hipEvent_t> evs;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_blocks) if (kv.second.pending) evs.push_back(kv.second.ready);
  }
  for (hipEvent_t e : evs) FEMO_HIP_CHECK(hipEventSynchronize(e));
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto& kv : g_blocks) if (kv.second.pending && hipEventQuery(kv.second.ready) == hipSuccess) kv.second.pending = false;
  return 0;
}

}  // extern "C"

extern "C" int femo_range_plan_host(int64_t n, int64_t chunk, int taper, int64_t floor, int64_t factor, int64_t cap, int64_t* bounds,
                                    int64_t room) {
  FEMO_REQUIRE(bounds != nullptr || room == 0, "null argument");
  const auto plan = femo_range_plan(n, chunk, taper, floor, factor, cap);
  for (size_t k = 0; k < plan.size() && (int64_t)(2 * k + 1) < room; ++k) { bounds[2 * k] = plan[k].first; bounds[2 * k + 1] = plan[k].second; }
  return (int)plan.size();
}

int femo_vec_upload_chunks(const femo_vec* v, std::vector<int64_t>& ends) {
  ends.clear();
  if (!v || !v->h2d_pending || v->h2d_chunks <= 1) return 0;
  ends = v->h2d_ends;
  return v->h2d_chunks;
}
