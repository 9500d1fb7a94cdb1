// plat_hip.inc — the HIP implementation of the platform layer (plat.h) under the C ABI of asched_host.inc: the per-handle context (device, stream, events,
// helper mailbox, cancel word), the run-time RCCL binding and exchange areas, memory and copies, and every kernel launch.  Host code only.  Included by
// armada_sched.hip after the kernels it launches (round_kernel.h, k_control, kernels_*.h) and after plat.h; the other code objects' kernels are reached
// through the hidden extern "C" launch wrappers declared here.  tests/hostsim/hostsim.cpp implements the same plat.h serially for the CPU build.
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the functions are bound with dlsym at asched_comm_init (no link-time dependency on librccl)

// ------------------------------------------------------------------------------------------------ platform layer
// Everything a handle needs from the HIP runtime lives in its PlatCtx: device ordinal, launch stream, events, the helper mailbox, the
// host-mapped cancel word.  Handles are independent — two pools on two GPUs in one process, one thread per handle (include/armada_sched.h).
// Every ABI entry starts with plat_enter(handle context): hipSetDevice for the calling thread (the current device is thread-local in HIP,
// and a goroutine may run on any OS thread) and the thread-local pointer the plat_* helpers below work on.
struct HelpBox;
// one per family of plat.h's kPassFamilies: the events are created at the first timed call of the handle and destroyed in plat_close
constexpr int PASS_MAX_EVENTS = 8;
constexpr int passEvents(int f) { return kPassFamilies[f].layout == PASS_PAIRS ? 2 * kPassFamilies[f].passes : kPassFamilies[f].passes + 1; }
constexpr bool passEventsFit() { for (int f = 0; f < PASS_FAMILIES; f++) if (passEvents(f) > PASS_MAX_EVENTS) return false; return true; }
static_assert(passEventsFit(), "a family of kPassFamilies records more events than a PassTimer holds");
struct PassTimer {
  hipEvent_t ev[PASS_MAX_EVENTS] = {};
  unsigned timed = 0;   // bit 0: the last call ran to its end with events around its passes (PASS_PAIRS: bit k, for pass k of the last round)
};
struct PlatCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, fitEv0 = nullptr, fitEv1 = nullptr, litEvMid = nullptr;
  HelpBox* helpBox = nullptr;
  int helpers = -1, cus = 0, wallClockKHz = 100000;
  float lastControlMs = 0.f, lastFitMs = 0.f;
  int lastControlLaunches = 0;
  int32_t* progress = nullptr;      // ASCHED_PROGRESS=1: host-visible heartbeat of the round kernel
  int32_t* cancelHost = nullptr;    // host-mapped, coherent: written by the host (deadline / asched_cancel), polled by the round kernel
  int32_t* cancelDev = nullptr;
  double deadlineS = 0;             // maxSchedulingDuration for every following round launch; 0 = none
  bool inRound = false;             // between plat_round_begin / plat_round_end: the deadline runs from the begin, the cancel word is consumed at the end
  std::chrono::steady_clock::time_point roundT0;
  hipEvent_t rEv0 = nullptr, rEv1 = nullptr;
  PassTimer pass[PASS_FAMILIES];   // ASCHED_*_TIMES=1: the events around the passes of the table calls and of the evictor report, and which of them the last call timed
  float roundTotalMs = 0.f, roundControlMs = 0.f; int roundLaunches = 0;
  int32_t* cmpScratch = nullptr; size_t cmpScratchInts = 0;   // block counts + total of the grid-wide compaction
  int optIndexN = -1, optIndexM = -1;   // sizes the optimiser's node -> jobs index in the scratch was built for (asched_host.inc decides when it may be reused)
  void* fitScratch = nullptr; size_t fitScratchBytes = 0;   // keys + shape list of a fit batch
  void* litScratch = nullptr; size_t litScratchBytes = 0;   // index, sort scratch, row list and results of a literal fit batch (kernels_fit_lit.h): its own buffer, the index outlives packed-key passes in between
  void* optSel = nullptr; size_t optSelBytes = 0;   // block partials + result of the device-side candidate selection
  void* optScratch = nullptr; size_t optScratchBytes = 0;     // node -> jobs index, queue costs and per-node scores of the fairness optimiser, kept across calls
  std::string err;
  bool failed = false;              // sticky: an allocation / copy / memset failed since the last plat_take_failure()
  // the handle's communicator (asched_comm_init: RCCL over xGMI; asched_comm_init_external: the caller's transport)
  ncclComm_t comm = nullptr; int commRank = 0, commWorld = 1;
  unsigned long long* xArea = nullptr; unsigned long long** xPeerTable = nullptr; bool xDirect = false;   // GPU-to-GPU exchange of sharded passes (asched_shard_area / asched_shard_peers)
  hipStream_t xStream = nullptr; long long* xBuf = nullptr;   // sharded wide passes (dev.h shardWorld) over RCCL: the exchanged words' all-reduce runs here, beside the persistent kernel
  long lastShardExchanges = 0;
  asched_allreduce_fn extFn = nullptr; void* extCtx = nullptr;
};
static thread_local PlatCtx* t_ctx = nullptr;
static std::string g_noCtxErr;

static bool hipOk(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  if (t_ctx) { t_ctx->err = m; t_ctx->failed = true; } else g_noCtxErr = m;
  return false;
}
static const char* plat_last_error() { return t_ctx ? t_ctx->err.c_str() : g_noCtxErr.c_str(); }
// true (once) when an upload / download / memset / allocation failed since the last call: input-build entry points return ASCHED_ERR_DEVICE
static bool plat_take_failure() { if (!t_ctx) return true; bool f = t_ctx->failed; t_ctx->failed = false; return f; }
static void plat_enter(PlatCtx* c) { t_ctx = c; if (c) (void)hipSetDevice(c->device); }
static PlatCtx* plat_open(std::string& err, int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { err = "no HIP device: libarmada_sched.so is the gfx950 implementation and has no CPU path"; return nullptr; }
  if (device >= n) { err = "device ordinal out of range"; return nullptr; }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) { err = "hipGetDevice failed"; return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return nullptr; }
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) { err = "hipGetDeviceProperties failed"; return nullptr; }
  if (std::string(p.gcnArchName).find("gfx950") == std::string::npos) { err = std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only"; return nullptr; }
  auto* c = new PlatCtx();
  c->device = device;
  c->cus = p.multiProcessorCount;
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) c->wallClockKHz = khz;
  bool ok = hipStreamCreate(&c->stream) == hipSuccess && hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess &&
            hipEventCreate(&c->fitEv0) == hipSuccess && hipEventCreate(&c->fitEv1) == hipSuccess && hipEventCreate(&c->litEvMid) == hipSuccess && hipEventCreate(&c->rEv0) == hipSuccess && hipEventCreate(&c->rEv1) == hipSuccess;
  // the mailbox is written from both sides across XCDs: it must not live in an XCD-private L2 -> fine-grained (uncached, device-coherent) memory
  ok = ok && hipExtMallocWithFlags((void**)&c->helpBox, sizeof(HelpBox), hipDeviceMallocFinegrained) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->cancelHost, 256, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;   // [0] the cancel word; from byte 64: the exchange words of sharded passes (dev.h XCHG_WORD0)
  if (ok) { memset(c->cancelHost, 0, 256); ok = hipHostGetDevicePointer((void**)&c->cancelDev, c->cancelHost, 0) == hipSuccess; }
  if (!ok) { err = "HIP resource creation failed (stream / events / mailbox / cancel word)"; delete c; return nullptr; }
  // helper workgroups of a round launch: one per CU, an eighth of the device by default — measured flat between 15 and 63 (ASCHED_HELPERS overrides; 0 = none)
  c->helpers = c->cus >= 16 ? c->cus / 8 - 1 : 0;
  if (const char* e = getenv("ASCHED_HELPERS")) c->helpers = atoi(e);
  if (c->helpers > c->cus - 1) c->helpers = c->cus - 1;
  if (c->helpers < 0) c->helpers = 0;
  if (getenv("ASCHED_PROGRESS")) {
    if (hipHostMalloc((void**)&c->progress, 64 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) c->progress = nullptr;
    if (c->progress) for (int i = 0; i < 64; i++) c->progress[i] = 0;
  }
  t_ctx = c;
  return c;
}
// ---- RCCL, bound at run time.  dlopen by soname: when the process already holds an RCCL (torch bundles one and loads it before this library in the Python
// harness) the loader hands back THAT copy — one RCCL per process, on the HIP runtime the process already uses; a Go scheduler gets /opt/rocm/lib's.
struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) getUniqueId = nullptr;
  decltype(&ncclCommInitRank) commInitRank = nullptr;
  decltype(&ncclCommDestroy) commDestroy = nullptr;
  decltype(&ncclAllReduce) allReduce = nullptr;
  decltype(&ncclGetErrorString) errorString = nullptr;
};
static RcclApi* rcclApi(std::string& err) {
  static RcclApi api; static bool tried = false; static std::string why;
  if (!tried) {
    tried = true;
    const char* names[] = {getenv("ASCHED_RCCL_PATH"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) { if (!n || !*n) continue; api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (api.lib) break; why = dlerror(); }
    if (api.lib) {
      api.getUniqueId = (decltype(api.getUniqueId))dlsym(api.lib, "ncclGetUniqueId");
      api.commInitRank = (decltype(api.commInitRank))dlsym(api.lib, "ncclCommInitRank");
      api.commDestroy = (decltype(api.commDestroy))dlsym(api.lib, "ncclCommDestroy");
      api.allReduce = (decltype(api.allReduce))dlsym(api.lib, "ncclAllReduce");
      api.errorString = (decltype(api.errorString))dlsym(api.lib, "ncclGetErrorString");
      if (!api.getUniqueId || !api.commInitRank || !api.commDestroy || !api.allReduce) { why = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllReduce"; dlclose(api.lib); api.lib = nullptr; }
    }
  }
  if (!api.lib) { err = "RCCL is not available: " + why; return nullptr; }
  return &api;
}
static bool rcclOk(RcclApi* a, ncclResult_t r, const char* what) {
  if (r == ncclSuccess) return true;
  std::string m = std::string(what) + ": " + (a->errorString ? a->errorString(r) : "RCCL error");
  if (t_ctx) { t_ctx->err = m; t_ctx->failed = true; } else g_noCtxErr = m;
  return false;
}
static int plat_comm_unique_id(char* out128) {
  std::string err; RcclApi* a = rcclApi(err);
  if (!a) { g_noCtxErr = err; if (t_ctx) t_ctx->err = err; return -1; }
  ncclUniqueId id;
  static_assert(sizeof(id) == 128, "asched_unique_id carries an ncclUniqueId");
  if (!rcclOk(a, a->getUniqueId(&id), "ncclGetUniqueId")) return -1;
  memcpy(out128, &id, sizeof id);
  return 0;
}
static void plat_comm_destroy_ctx(PlatCtx* c) {
  if (c->comm) { std::string err; if (RcclApi* a = rcclApi(err)) (void)a->commDestroy(c->comm); c->comm = nullptr; }
  c->extFn = nullptr; c->extCtx = nullptr; c->commRank = 0; c->commWorld = 1;
}
static int plat_comm_init(const char* id128, int rank, int world) {
  PlatCtx* c = t_ctx;
  std::string err; RcclApi* a = rcclApi(err);
  if (!a) { c->err = err; return -1; }
  plat_comm_destroy_ctx(c);
  ncclUniqueId id; memcpy(&id, id128, sizeof id);
  if (!rcclOk(a, a->commInitRank(&c->comm, world, id, rank), "ncclCommInitRank")) { c->comm = nullptr; return -1; }
  c->commRank = rank; c->commWorld = world;
  return 0;
}
static int plat_comm_init_external(asched_allreduce_fn fn, void* ctx, int rank, int world) {
  PlatCtx* c = t_ctx;
  plat_comm_destroy_ctx(c);
  c->extFn = fn; c->extCtx = ctx; c->commRank = rank; c->commWorld = world;
  return 0;
}
static void plat_comm_destroy() { if (t_ctx) { (void)hipStreamSynchronize(t_ctx->stream); plat_comm_destroy_ctx(t_ctx); } }
static void plat_comm_info(int* rank, int* world) { *rank = t_ctx ? t_ctx->commRank : 0; *world = t_ctx ? t_ctx->commWorld : 1; }
static bool plat_comm_live() { return t_ctx && (t_ctx->comm || t_ctx->extFn); }
// in-place all-reduce of `count` int64 words in memory of this handle's GPU, on the handle's stream: behind whatever produced the words there, in front of
// whatever the caller enqueues next.  op: 0 SUM, 1 MIN, 2 MAX.
static int plat_allreduce(long long* dbuf, size_t count, int op) {
  PlatCtx* c = t_ctx;
  if (c->commWorld <= 1 && !c->comm && !c->extFn) return 0;
  if (c->comm) {
    std::string err; RcclApi* a = rcclApi(err);
    if (!a) { c->err = err; return -1; }
    ncclRedOp_t o = op == 0 ? ncclSum : op == 1 ? ncclMin : ncclMax;
    if (!rcclOk(a, a->allReduce(dbuf, dbuf, count, ncclInt64, o, c->comm, c->stream), "ncclAllReduce")) return -1;
    return 0;
  }
  if (!hipOk(hipStreamSynchronize(c->stream), "all-reduce (external transport): stream sync")) return -1;   // the transport sees finished words and an idle stream
  if (c->extFn(c->extCtx, dbuf, (int64_t)count, op) != 0) { c->err = "the external all-reduce transport failed"; return -1; }
  return 0;
}
// all-reduce MIN of a few UNSIGNED 64-bit words that live in HOST memory, while the handle's stream is busy with the persistent kernel that waits for the answer
// (shardReduce): RCCL on a side stream through a device staging buffer, or the caller's transport with ASCHED_ALLREDUCE_HOST_WORDS in `op` (the words are host memory: reduce
// them where they are, do not synchronise the device).  The collectives compare int64: the sign bit is flipped around them.
static int plat_allreduce_host_min(unsigned long long* w, int count) {
  PlatCtx* c = t_ctx;
  long long v[8];
  if (count > 8) return -1;
  for (int i = 0; i < count; i++) v[i] = (long long)(w[i] ^ 0x8000000000000000ull);
  if (c->comm) {
    std::string err; RcclApi* a = rcclApi(err);
    if (!a) { c->err = err; return -1; }
    if (!c->xStream && !hipOk(hipStreamCreateWithFlags(&c->xStream, hipStreamNonBlocking), "hipStreamCreate (exchange)")) return -1;
    if (!c->xBuf && !hipOk(hipMalloc((void**)&c->xBuf, 8 * sizeof(long long)), "hipMalloc (exchange)")) return -1;
    if (!hipOk(hipMemcpyAsync(c->xBuf, v, count * sizeof(long long), hipMemcpyHostToDevice, c->xStream), "exchange h2d")) return -1;
    if (!rcclOk(a, a->allReduce(c->xBuf, c->xBuf, count, ncclInt64, ncclMin, c->comm, c->xStream), "ncclAllReduce (exchange)")) return -1;
    if (!hipOk(hipMemcpyAsync(v, c->xBuf, count * sizeof(long long), hipMemcpyDeviceToHost, c->xStream), "exchange d2h") || !hipOk(hipStreamSynchronize(c->xStream), "exchange sync")) return -1;
  } else if (c->extFn) {
    if (c->extFn(c->extCtx, v, (int64_t)count, 1 | ASCHED_ALLREDUCE_HOST_WORDS) != 0) { c->err = "the external all-reduce transport failed"; return -1; }
  }
  for (int i = 0; i < count; i++) w[i] = (unsigned long long)v[i] ^ 0x8000000000000000ull;
  return 0;
}
static long plat_last_shard_exchanges() { return t_ctx ? t_ctx->lastShardExchanges : 0; }
#define XCHG_AREA_BYTES (64 + 2 * 256 * 32)
// this handle's exchange area (device memory, fine-grained where the runtime offers it: remote GPUs store into it) and its IPC handle for replicas in other processes
static int plat_shard_area(void** ptr, char* ipc64) {
  PlatCtx* c = t_ctx;
  if (!c->xArea) {
    void* p = nullptr;
    if (hipExtMallocWithFlags(&p, XCHG_AREA_BYTES, hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); if (!hipOk(hipMalloc(&p, XCHG_AREA_BYTES), "hipMalloc (exchange area)")) return -1; }
    if (!hipOk(hipMemset(p, 0, XCHG_AREA_BYTES), "exchange area reset")) { (void)hipFree(p); return -1; }
    c->xArea = (unsigned long long*)p;
  }
  *ptr = c->xArea;
  if (ipc64) {
    hipIpcMemHandle_t h; memset(&h, 0, sizeof h);
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "IPC handle");
    memset(ipc64, 0, 64);
    if (hipIpcGetMemHandle(&h, c->xArea) == hipSuccess) memcpy(ipc64, &h, sizeof h); else (void)hipGetLastError();   // (all zero: not exportable here; in-process peers still work)
  }
  return 0;
}
static int plat_shard_open(const char* ipc64, void** out) {
  hipIpcMemHandle_t h; memcpy(&h, ipc64, sizeof h);
  return hipOk(hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle (exchange area)") ? 0 : -1;
}
static int plat_shard_peers(void* const* areas, int world, int rank) {
  PlatCtx* c = t_ctx;
  if (!areas) { c->xDirect = false; return 0; }
  if (!c->xArea || areas[rank] != (void*)c->xArea) { c->err = "shard_peers: areas[rank] must be this handle's own area (asched_shard_area)"; return -1; }
  for (int r = 0; r < world; r++) {   // a peer area on another GPU of this process: let this GPU store into it
    hipPointerAttribute_t at; memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, areas[r]) == hipSuccess && at.device != c->device) { hipError_t e = hipDeviceEnablePeerAccess(at.device, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { hipOk(e, "hipDeviceEnablePeerAccess"); return -1; } (void)hipGetLastError(); }
    else (void)hipGetLastError();
  }
  if (!c->xPeerTable && !hipOk(hipMalloc((void**)&c->xPeerTable, 256 * sizeof(void*)), "hipMalloc (peer table)")) return -1;
  if (!hipOk(hipMemcpy(c->xPeerTable, areas, world * sizeof(void*), hipMemcpyHostToDevice), "peer table upload")) return -1;
  c->xDirect = true;
  return 0;
}
static void plat_close(PlatCtx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->xStream) (void)hipStreamDestroy(c->xStream);
  if (c->xBuf) (void)hipFree(c->xBuf);
  if (c->xArea) (void)hipFree(c->xArea);
  if (c->xPeerTable) (void)hipFree(c->xPeerTable);
  plat_comm_destroy_ctx(c);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  for (hipEvent_t e : {c->ev0, c->ev1, c->fitEv0, c->fitEv1, c->litEvMid, c->rEv0, c->rEv1}) if (e) (void)hipEventDestroy(e);
  for (PassTimer& t : c->pass) for (hipEvent_t e : t.ev) if (e) (void)hipEventDestroy(e);
  if (c->helpBox) (void)hipFree(c->helpBox);
  if (c->cmpScratch) (void)hipFree(c->cmpScratch);
  if (c->optScratch) (void)hipFree(c->optScratch);
  if (c->optSel) (void)hipFree(c->optSel);
  if (c->fitScratch) (void)hipFree(c->fitScratch);
  if (c->litScratch) (void)hipFree(c->litScratch);
  if (c->cancelHost) (void)hipHostFree(c->cancelHost);
  if (c->progress) (void)hipHostFree(c->progress);
  if (t_ctx == c) t_ctx = nullptr;
  delete c;
}
static int plat_wall_clock_khz() { return t_ctx ? t_ctx->wallClockKHz : 100000; }
static void plat_set_deadline(double s) { if (t_ctx) t_ctx->deadlineS = s > 0 ? s : 0; }
static void plat_cancel(PlatCtx* c) { if (c && c->cancelHost) __atomic_store_n(c->cancelHost, 1, __ATOMIC_RELEASE); }  // any thread: a plain store to host memory
static void plat_cancel_clear(PlatCtx* c) { if (c && c->cancelHost) __atomic_store_n(c->cancelHost, 0, __ATOMIC_RELEASE); }
static void* plat_malloc(size_t n) { void* p = nullptr; if (!hipOk(hipMalloc(&p, n), "hipMalloc")) return nullptr; return p; }
static void plat_free(void* p) { if (p) (void)hipFree(p); }
static void plat_memset(void* p, int v, size_t n) { if (!p) { hipOk(hipErrorInvalidValue, "memset of a failed allocation"); return; } hipOk(hipMemsetAsync(p, v, n, t_ctx->stream), "hipMemsetAsync"); }
static void plat_h2d(void* d, const void* s, size_t n) {
  if (!d) { hipOk(hipErrorInvalidValue, "upload into a failed allocation"); return; }
  if (hipOk(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, t_ctx->stream), "hipMemcpyAsync (h2d)")) hipOk(hipStreamSynchronize(t_ctx->stream), "h2d sync");
}
static void plat_d2d(void* d, const void* s, size_t n) {
  if (!d || !s) { hipOk(hipErrorInvalidValue, "device copy of a failed allocation"); return; }
  if (n) hipOk(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, t_ctx->stream), "hipMemcpyAsync (d2d)");
}
// pinned host memory + asynchronous downloads on the handle's stream (the round's result arrays: one wait for all of them)
static void* plat_pinned(size_t n) { void* p = nullptr; if (!hipOk(hipHostMalloc(&p, n, hipHostMallocDefault), "hipHostMalloc")) return nullptr; return p; }
static void plat_pinned_free(void* p) { if (p) (void)hipHostFree(p); }
static void plat_d2h_async(void* d, const void* s, size_t n) {
  if (!s) { hipOk(hipErrorInvalidValue, "download from a failed allocation"); std::memset(d, 0, n); return; }
  hipOk(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, t_ctx->stream), "hipMemcpyAsync (d2h)");
}
static void plat_sync() { hipOk(hipStreamSynchronize(t_ctx->stream), "stream sync"); }
static void plat_d2h(void* d, const void* s, size_t n) {
  if (!s) { hipOk(hipErrorInvalidValue, "download from a failed allocation"); std::memset(d, 0, n); return; }
  if (hipOk(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, t_ctx->stream), "hipMemcpyAsync (d2h)")) hipOk(hipStreamSynchronize(t_ctx->stream), "d2h sync");
}

// device time of the last control-kernel launch (HIP events recorded on the launch stream) — bench.py's roofline input
static double plat_last_control_ms() { return t_ctx ? (double)t_ctx->lastControlMs : 0.0; }
static int plat_last_control_launches() { return t_ctx ? t_ctx->lastControlLaunches : 0; }

extern "C" int asched_internal_aux_launch(const Dev* dev, int cmd, hipStream_t stream, void* helpBox, const MktDev* mk);  // armada_sched_aux.hip
extern "C" int asched_internal_wk_launch(const Dev* dev, int cmd, hipStream_t stream, void* helpBox, int H, const MktDev* mk);               // armada_sched_wk.hip: handles with a two-word order key
extern "C" int asched_internal_wk_bulk(const Dev* dev, int kind, int n, int grid, hipStream_t stream);
extern "C" int asched_internal_wk_fit_batch(const Dev* dev, const int32_t* shapes, int ns, int level, unsigned long long* out, int tiles, int ysplit, hipStream_t stream);
// market-driven rounds: the market state the next auxiliary launch of this thread's handle runs with (asched_host.inc sets it around CMD_MARKET_ROUND)
static thread_local const MktDev* t_mkt = nullptr;
static void plat_set_market_dev(const MktDev* m) { t_mkt = m; }
static int plat_run_control(Dev& dev, int cmd) {
  PlatCtx* c = t_ctx;
  if (c->failed) return -1;  // an earlier upload failed: the kernel would read unset pointers
  static_assert(sizeof(HelpBox) == 256 + HELP_MAX * 32, "mailbox allocation");
  bool isRound = cmd == CMD_ROUND || cmd == CMD_QUEUES_ONLY || cmd == CMD_PASS1 || cmd == CMD_PASS2;
  int H = isRound ? c->helpers : 0;
  // the wide queries of the generic path (plane scan, fair-share evaluation) are one node per thread: from ~50k nodes on half of the CUs pay off (measured at 100k
  // nodes x 1M jobs 95% occupied: 29.5 -> 23.0 s per round with 127 helpers, 24.6 s with 255; flat between 15 and 63 at 20k nodes)
  if (isRound && !getenv("ASCHED_HELPERS") && dev.cfg.N >= 50000 && c->cus >= 128) H = c->cus / 2 - 1;
  // more than QCAPF queues (round_wide.h): the merge of a wide run is a bulk rank over all queues' entries — work for every workgroup the launch can bring
  if (isRound && !getenv("ASCHED_HELPERS") && dev.f.iterOk == 2 && c->cus >= 128) H = c->cus / 2 - 1;
  dev.progress = ((cmd == CMD_ROUND || cmd == CMD_PASS1 || cmd == CMD_PASS2) && c->progress) ? c->progress : nullptr;
  dev.cancel = c->cancelDev;
  if (!hipOk(hipMemsetAsync(c->helpBox, 0, sizeof(HelpBox), c->stream), "help box reset")) return -1;
  (void)hipEventRecord(c->ev0, c->stream);
  const bool shard = dev.cfg.shardWorld > 1;
  volatile unsigned long long* X = (volatile unsigned long long*)c->cancelHost;
  const bool direct = shard && c->xDirect;   // GPU-to-GPU exchange (asched_shard_peers): the kernel finds the peer table's address in the block; no proxy
  if (shard) { for (int i = 0; i < 6; i++) X[XCHG_WORD0 + i] = 0; X[XCHG_WORD0 + 6] = direct ? (unsigned long long)c->xPeerTable : 0; X[XCHG_WORD0 + 7] = 0; __atomic_thread_fence(__ATOMIC_SEQ_CST); if (!c->inRound) c->lastShardExchanges = 0; }
  if (dev.cfg.keyWords == 2 || shard) {   // a two-word order key, or wide passes sharded across GPUs: every control command on the kernel built for them (armada_sched_wk.hip)
    if (asched_internal_wk_launch(&dev, cmd, c->stream, c->helpBox, H, t_mkt)) { c->err = "k_control_wk launch failed"; return -1; }
  } else if (cmd >= CMD_AUX_FIRST) {  // submit-check commands: their kernel lives in its own code object (armada_sched_aux.hip)
    if (asched_internal_aux_launch(&dev, cmd, c->stream, c->helpBox, t_mkt)) { c->err = "k_control_aux launch failed"; return -1; }
  } else
  hipLaunchKernelGGL(k_control, dim3(1 + H), dim3(CTL_THREADS), 0, c->stream, dev, cmd, c->helpBox, H);
  (void)hipEventRecord(c->ev1, c->stream);
  if (!hipOk(hipGetLastError(), "k_control launch")) return -1;
  static const double safetyS = [] { const char* e = getenv("ASCHED_SAFETY_DEADLINE_S"); return e ? atof(e) : 0.0; }();   // test / measurement runs of new builds: no launch outlives this
  double deadlineS = c->deadlineS > 0 ? c->deadlineS : safetyS;
  if (shard && !direct) {
    // the exchange proxy of sharded passes: the kernel posts (generation, two words), this thread runs the all-reduce on the handle's communicator and answers (dev.h XCHG_WORD0)
    auto t0 = c->inRound ? c->roundT0 : std::chrono::steady_clock::now();
    unsigned long long served = 0; unsigned int idle = 0; bool failed = false;
    for (;;) {
      // (the stream is asked only now and then: a query costs microseconds of the runtime's time on the path of every exchange; the request word is a load of host memory)
      if ((idle & 63) == 0 && hipStreamQuery(c->stream) != hipErrorNotReady) break;
      unsigned long long g = __atomic_load_n(&X[XCHG_WORD0], __ATOMIC_ACQUIRE);
      if (g != served && !failed) {
        unsigned long long w[2] = {X[XCHG_WORD0 + 1], X[XCHG_WORD0 + 2]};
        if (plat_allreduce_host_min(w, 2)) { failed = true; plat_cancel(c); continue; }   // (the kernel's wait ends on the cancel word: ASCHED_ERR_TIMEOUT 903, reported as a device error below)
        X[XCHG_WORD0 + 4] = w[0]; X[XCHG_WORD0 + 5] = w[1];
        __atomic_store_n(&X[XCHG_WORD0 + 3], g, __ATOMIC_RELEASE);
        served = g; c->lastShardExchanges++; idle = 1;
        continue;
      }
      if ((++idle & 0xfff) == 0 && isRound && deadlineS > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > deadlineS) plat_cancel(c);
    }
    if (failed) { (void)hipStreamSynchronize(c->stream); if (!c->inRound) __atomic_store_n(c->cancelHost, 0, __ATOMIC_RELEASE); return -1; }
  } else
  if (dev.progress || (isRound && deadlineS > 0)) {
    // hard timeout (scheduling_algo.go:130-134): the kernel polls the cancel word; the host sets it when the deadline passes
    auto t0 = c->inRound ? c->roundT0 : std::chrono::steady_clock::now();
    int ticks = 0;
    volatile int32_t* progress = c->progress;
    while (hipStreamQuery(c->stream) == hipErrorNotReady) {
      usleep(dev.progress ? 100000 : 100);
      double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (isRound && deadlineS > 0 && el > deadlineS) plat_cancel(c);
      if (dev.progress && ++ticks % 10 == 0) { fprintf(stderr, "[asched progress] t=%ds iterations=%d generic=%d phase=%d op=%d ops=%d | wait: done=%d H=%d gen=%d box.gen=%d box.op=%d | helpers:", ticks / 10, progress[0], progress[4], progress[1], progress[2], progress[3], progress[5], progress[6], progress[7], progress[8], progress[9]); for (int i = 17; i < 56; i++) fprintf(stderr, " %x", progress[i]); fprintf(stderr, "\n"); }
    }
  }
  if (!hipOk(hipStreamSynchronize(c->stream), "k_control")) return -1;
  if (direct) c->lastShardExchanges += (long)X[XCHG_WORD0 + 7];   // (written by the kernel at its end: the GPU-to-GPU exchanges of this launch)
  if (isRound && !c->inRound) __atomic_store_n(c->cancelHost, 0, __ATOMIC_RELEASE);  // a cancel request is consumed by the round it hit (or the next one, if it came between rounds)
  (void)hipEventElapsedTime(&c->lastControlMs, c->ev0, c->ev1);
  c->lastControlLaunches = 1;
  if (c->inRound) { c->roundControlMs += c->lastControlMs; c->roundLaunches++; }
  return 0;
}

// ---- the split round: grid-wide kernels between the persistent passes, all on the handle's stream (no host sync except where a count is needed)
static void plat_round_begin() {
  PlatCtx* c = t_ctx;
  c->inRound = true; c->roundT0 = std::chrono::steady_clock::now(); c->roundControlMs = 0.f; c->roundLaunches = 0; c->lastShardExchanges = 0;
  (void)hipEventRecord(c->rEv0, c->stream);
}
static void plat_round_end() {
  PlatCtx* c = t_ctx;
  (void)hipEventRecord(c->rEv1, c->stream);
  (void)hipStreamSynchronize(c->stream);
  (void)hipEventElapsedTime(&c->roundTotalMs, c->rEv0, c->rEv1);
  c->inRound = false;
  __atomic_store_n(c->cancelHost, 0, __ATOMIC_RELEASE);
}
static void plat_round_times(double* out) { PlatCtx* c = t_ctx; out[0] = c->roundTotalMs; out[1] = c->roundControlMs; out[2] = c->roundLaunches; }
static int bulkGrid(int n) { int b = (n + 255) / 256; int cap = (t_ctx->cus > 0 ? t_ctx->cus : 256) * 8; return b < 1 ? 1 : (b > cap ? cap : b); }
static int plat_bulk(Dev& d, int kind, int n) {
  if (n <= 0) return 0;
  if (d.cfg.keyWords == 2) { if (asched_internal_wk_bulk(&d, kind, n, bulkGrid(n), t_ctx->stream)) { t_ctx->err = "k_bulk_wk launch failed"; return -1; } }
  else
  hipLaunchKernelGGL(k_bulk, dim3(bulkGrid(n)), dim3(256), 0, t_ctx->stream, d, kind, n);
  t_ctx->roundLaunches++;
  return hipOk(hipGetLastError(), "k_bulk launch") ? 0 : -1;
}
static int plat_small(Dev& d, int what, int arg) {
  hipLaunchKernelGGL(k_round_small, dim3(1), dim3(64), 0, t_ctx->stream, d, what, arg);
  t_ctx->roundLaunches++;
  return hipOk(hipGetLastError(), "k_round_small launch") ? 0 : -1;
}
static int plat_agg(Dev& d, int queued, int total) {
  if (total <= 0) return 0;
  hipLaunchKernelGGL(k_agg, dim3(bulkGrid(total)), dim3(256), 0, t_ctx->stream, d, queued, total);
  return hipOk(hipGetLastError(), "k_agg launch") ? 0 : -1;
}
static int plat_evict_apply(Dev& d, int phase3, int total) {
  if (total <= 0) return 0;
  hipLaunchKernelGGL(k_evict_apply, dim3(bulkGrid(total)), dim3(256), 0, t_ctx->stream, d, phase3, total);
  t_ctx->roundLaunches++;
  return hipOk(hipGetLastError(), "k_evict_apply launch") ? 0 : -1;
}
// fairness optimiser: every node scored for one job (k_opt_score), scores downloaded; detailNode >= 0: that node's preemption list as well
static float g_lastOptMs = 0.f;
static int plat_opt_score(Dev& d, const OptArgs& a, std::vector<OptNodeOut>& scores, double* jobCost, int detailNode, OptNodeOut* detail, std::vector<int32_t>* pre, bool detailOnly,
                          bool reuseIndex) {   // detailOnly: the index and scores of the previous call are still in the scratch; reuseIndex: so is the node -> jobs index (nothing was bound since)
  PlatCtx* c = t_ctx;
  int N = d.cfg.N, M = d.cfg.M, Q = d.cfg.Q;
  // one allocation, carved: [scores N+1][queue costs Q+1][cnt N+1][off N+2][cursor N+1][jobs M][pre OPT_MAXJ]
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t bOut = up(sizeof(OptNodeOut) * (size_t)(N + 1)), bQ = up(sizeof(double) * (size_t)(Q + 1)), bN = up(sizeof(int32_t) * (size_t)(N + 2)), bM = up(sizeof(int32_t) * 2 * (size_t)std::max(M, 1)), bP = up(sizeof(int32_t) * 64);
  size_t need = bOut + bQ + 3 * bN + bM + bP;
  bool ok = true;
  if (c->optScratchBytes < need) {
    if (c->optScratch) (void)hipFree(c->optScratch);
    c->optScratch = nullptr; c->optScratchBytes = 0; c->optIndexN = c->optIndexM = -1;
    ok = hipOk(hipMalloc(&c->optScratch, need), "optimiser scratch");
    if (ok) c->optScratchBytes = need;
  }
  char* base = (char*)c->optScratch;
  OptNodeOut* out = (OptNodeOut*)base; double* qCost = (double*)(base + bOut);
  int32_t* cnt = (int32_t*)(base + bOut + bQ); int32_t* off = (int32_t*)(base + bOut + bQ + bN); int32_t* cursor = (int32_t*)(base + bOut + bQ + 2 * bN);
  int32_t* jobs = (int32_t*)(base + bOut + bQ + 3 * bN); int32_t* dPre = (int32_t*)(base + bOut + bQ + 3 * bN + bM);
  // the preemption list of one node: the private entry list when its job count fits, an HBM list otherwise
  auto runDetail = [&]() -> bool {
    int32_t o2[2] = {0, 0};
    if (!hipOk(hipMemcpy(o2, off + detailNode, sizeof o2, hipMemcpyDeviceToHost), "opt detail")) return false;
    int cnt = o2[1] - o2[0];
    static const bool perThread = [] { const char* e = getenv("ASCHED_OPT_PER_THREAD"); return e && e[0] == '1'; }();
    if (cnt <= (perThread ? OPT_MAXJ : 64)) {
      pre->assign(64, -1);
      if (perThread) hipLaunchKernelGGL(k_opt_detail, dim3(1), dim3(64), 0, c->stream, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, detailNode, out + N, dPre);
      else hipLaunchKernelGGL(k_opt_detail_wave, dim3(1), dim3(64), 0, c->stream, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, detailNode, out + N, dPre);
      return hipOk(hipGetLastError(), "optimiser launch") && hipOk(hipMemcpyAsync(detail, out + N, sizeof(OptNodeOut), hipMemcpyDeviceToHost, c->stream), "opt detail") &&
             hipOk(hipMemcpyAsync(pre->data(), dPre, sizeof(int32_t) * 64, hipMemcpyDeviceToHost, c->stream), "opt detail") && hipOk(hipStreamSynchronize(c->stream), "optimiser kernels");
    }
    pre->assign((size_t)cnt, -1);
    OptEntry* es = nullptr; int32_t* dp = nullptr;
    bool k = hipOk(hipMalloc(&es, sizeof(OptEntry) * (size_t)cnt), "optimiser scratch") && hipOk(hipMalloc(&dp, sizeof(int32_t) * (size_t)cnt), "optimiser scratch");
    if (k) {
      hipLaunchKernelGGL(k_opt_detail_big, dim3(1), dim3(64), 0, c->stream, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, detailNode, out + N, dp, es);
      k = hipOk(hipGetLastError(), "optimiser launch") && hipOk(hipMemcpyAsync(detail, out + N, sizeof(OptNodeOut), hipMemcpyDeviceToHost, c->stream), "opt detail") &&
          hipOk(hipMemcpyAsync(pre->data(), dp, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream), "opt detail") && hipOk(hipStreamSynchronize(c->stream), "optimiser kernels");
    }
    (void)hipFree(es); (void)hipFree(dp);
    return k;
  };
  if (ok && detailOnly) return runDetail() ? 0 : -1;
  if (ok) {
    if (!(reuseIndex && c->optIndexN == N && c->optIndexM == M)) {
      (void)hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(N + 1), c->stream);
      hipLaunchKernelGGL(k_opt_count, dim3(bulkGrid(M)), dim3(256), 0, c->stream, d, cnt);
      hipLaunchKernelGGL(k_opt_scan, dim3(1), dim3(1024), 0, c->stream, (const int32_t*)cnt, off, cursor, N);
      hipLaunchKernelGGL(k_opt_scatter, dim3(bulkGrid(M)), dim3(256), 0, c->stream, d, cursor, jobs);
      c->optIndexN = N; c->optIndexM = M;
    }
    hipLaunchKernelGGL(k_opt_qcost, dim3((Q + 1 + 63) / 64), dim3(64), 0, c->stream, d, a.job, qCost);
    (void)hipEventRecord(c->fitEv0, c->stream);
    static const bool perThread = [] { const char* e = getenv("ASCHED_OPT_PER_THREAD"); return e && e[0] == '1'; }();   // A/B: the one-node-per-thread kernel of rounds 2-3
    if (perThread) hipLaunchKernelGGL(k_opt_score, dim3((N + 127) / 128), dim3(128), 0, c->stream, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, out);
    else hipLaunchKernelGGL(k_opt_score_wave, dim3((N + 3) / 4), dim3(256), 0, c->stream, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, out);
    (void)hipEventRecord(c->fitEv1, c->stream);
    ok = hipOk(hipGetLastError(), "optimiser launch") && hipOk(hipStreamSynchronize(c->stream), "optimiser kernels");
    (void)hipEventElapsedTime(&g_lastOptMs, c->fitEv0, c->fitEv1);
  }
  if (ok) {
    scores.resize(N);
    if (N) ok = hipOk(hipMemcpy(scores.data(), out, sizeof(OptNodeOut) * (size_t)N, hipMemcpyDeviceToHost), "opt scores");
    if (ok) ok = hipOk(hipMemcpy(jobCost, qCost + Q, sizeof(double), hipMemcpyDeviceToHost), "opt job cost");
  }
  if (ok) {   // nodes whose candidates did not fit the private list: scored again with a list in HBM (one thread per such node; they are few)
    std::vector<int32_t> big;
    for (int n = 0; n < N; n++) if (scores[n].scheduled < 0) big.push_back(n);
    if (!big.empty()) {
      std::vector<int32_t> hOff((size_t)N + 2);
      ok = hipOk(hipMemcpy(hOff.data(), off, sizeof(int32_t) * (size_t)(N + 1), hipMemcpyDeviceToHost), "opt index");
      std::vector<long long> eOff(big.size());
      long long total = 0;
      for (size_t i = 0; i < big.size(); i++) { eOff[i] = total; total += hOff[big[i] + 1] - hOff[big[i]]; }
      OptEntry* es = nullptr; int32_t* dn = nullptr; long long* de = nullptr;
      ok = ok && hipOk(hipMalloc(&es, sizeof(OptEntry) * (size_t)std::max<long long>(total, 1)), "optimiser scratch") && hipOk(hipMalloc(&dn, sizeof(int32_t) * big.size()), "optimiser scratch") &&
           hipOk(hipMalloc(&de, sizeof(long long) * big.size()), "optimiser scratch");
      if (ok) {
        (void)hipMemcpyAsync(dn, big.data(), sizeof(int32_t) * big.size(), hipMemcpyHostToDevice, c->stream);
        (void)hipMemcpyAsync(de, eOff.data(), sizeof(long long) * big.size(), hipMemcpyHostToDevice, c->stream);
        hipLaunchKernelGGL(k_opt_score_big, dim3(((int)big.size() + 63) / 64), dim3(64), 0, c->stream, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, (const int32_t*)dn, (const long long*)de,
                           (int)big.size(), es, out);
        ok = hipOk(hipGetLastError(), "optimiser launch") && hipOk(hipStreamSynchronize(c->stream), "optimiser kernels");
        for (size_t i = 0; ok && i < big.size(); i++) ok = hipOk(hipMemcpy(&scores[big[i]], out + big[i], sizeof(OptNodeOut), hipMemcpyDeviceToHost), "opt scores");
      }
      (void)hipFree(es); (void)hipFree(dn); (void)hipFree(de);
    }
  }
  if (ok && detailNode >= 0) ok = runDetail();
  return ok ? 0 : -1;
}
static double plat_last_opt_ms() { return (double)g_lastOptMs; }
// asched_optimiser_schedule_job without per-node scores: index (when stale), queue costs, scores, selection and the selected node's victims as ONE stream-ordered sequence.
// Returns 1 when a node overflowed the wave kernel (the caller takes plat_opt_score's path), 0 on success, -1 on a device error.
static int plat_opt_select(Dev& d, const OptArgs& a, double minPct, bool reuseIndex, int32_t* node, int32_t* npre, double* cost, double* impact, std::vector<int32_t>* pre) {
  static const bool perThread = [] { const char* e = getenv("ASCHED_OPT_PER_THREAD"); return e && e[0] == '1'; }();
  if (perThread) return 1;   // A/B runs of the round-2 kernel take the host-side selection as well
  PlatCtx* c = t_ctx;
  int N = d.cfg.N, M = d.cfg.M, Q = d.cfg.Q;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t bOut = up(sizeof(OptNodeOut) * (size_t)(N + 1)), bQ = up(sizeof(double) * (size_t)(Q + 1)), bN = up(sizeof(int32_t) * (size_t)(N + 2)), bM = up(sizeof(int32_t) * 2 * (size_t)std::max(M, 1)), bP = up(sizeof(int32_t) * 64);
  size_t need = bOut + bQ + 3 * bN + bM + bP;
  if (c->optScratchBytes < need) {
    if (c->optScratch) (void)hipFree(c->optScratch);
    c->optScratch = nullptr; c->optScratchBytes = 0; c->optIndexN = c->optIndexM = -1;
    if (!hipOk(hipMalloc(&c->optScratch, need), "optimiser scratch")) return -1;
    c->optScratchBytes = need;
  }
  int nb = (N + 255) / 256;
  size_t selBytes = up(sizeof(OptSelKey) * (size_t)std::max(nb, 1)) + 256;
  if (c->optSelBytes < selBytes) {
    if (c->optSel) (void)hipFree(c->optSel);
    c->optSel = nullptr; c->optSelBytes = 0;
    if (!hipOk(hipMalloc(&c->optSel, selBytes), "optimiser selection scratch")) return -1;
    c->optSelBytes = selBytes;
  }
  char* base = (char*)c->optScratch;
  OptNodeOut* out = (OptNodeOut*)base; double* qCost = (double*)(base + bOut);
  int32_t* cnt = (int32_t*)(base + bOut + bQ); int32_t* off = (int32_t*)(base + bOut + bQ + bN); int32_t* cursor = (int32_t*)(base + bOut + bQ + 2 * bN);
  int32_t* jobs = (int32_t*)(base + bOut + bQ + 3 * bN); int32_t* dPre = (int32_t*)(base + bOut + bQ + 3 * bN + bM);
  OptSelKey* partial = (OptSelKey*)c->optSel; OptSel* dSel = (OptSel*)((char*)c->optSel + selBytes - 256); int32_t* dOver = (int32_t*)((char*)c->optSel + selBytes - 128);
  hipStream_t st = c->stream;
  if (!(reuseIndex && c->optIndexN == N && c->optIndexM == M)) {
    (void)hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(N + 1), st);
    hipLaunchKernelGGL(k_opt_count, dim3(bulkGrid(M)), dim3(256), 0, st, d, cnt);
    hipLaunchKernelGGL(k_opt_scan, dim3(1), dim3(1024), 0, st, (const int32_t*)cnt, off, cursor, N);
    hipLaunchKernelGGL(k_opt_scatter, dim3(bulkGrid(M)), dim3(256), 0, st, d, cursor, jobs);
    c->optIndexN = N; c->optIndexM = M;
  }
  (void)hipMemsetAsync(dOver, 0, sizeof(int32_t), st);
  hipLaunchKernelGGL(k_opt_qcost, dim3((Q + 1 + 63) / 64), dim3(64), 0, st, d, a.job, qCost);
  (void)hipEventRecord(c->fitEv0, st);
  hipLaunchKernelGGL(k_opt_score_wave, dim3((N + 3) / 4), dim3(256), 0, st, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, out);
  (void)hipEventRecord(c->fitEv1, st);
  hipLaunchKernelGGL(k_opt_select, dim3(std::max(nb, 1)), dim3(256), 0, st, d, (const OptNodeOut*)out, (const uint8_t*)nullptr, (const double*)(qCost + Q), minPct, partial, dOver);
  hipLaunchKernelGGL(k_opt_select_final, dim3(1), dim3(256), 0, st, (const OptSelKey*)partial, nb, (const int32_t*)dOver, dSel);
  hipLaunchKernelGGL(k_opt_detail_sel, dim3(1), dim3(64), 0, st, d, a, (const double*)qCost, (const int32_t*)off, (const int32_t*)jobs, dSel, out + N, dPre);
  OptSel hs; pre->assign(64, -1);
  bool ok = hipOk(hipGetLastError(), "optimiser launch") && hipOk(hipMemcpyAsync(&hs, dSel, sizeof hs, hipMemcpyDeviceToHost, st), "opt selection") &&
            hipOk(hipMemcpyAsync(pre->data(), dPre, sizeof(int32_t) * 64, hipMemcpyDeviceToHost, st), "opt victims") && hipOk(hipStreamSynchronize(st), "optimiser kernels");
  (void)hipEventElapsedTime(&g_lastOptMs, c->fitEv0, c->fitEv1);
  if (!ok) return -1;
  if (hs.overflow || hs.big) return 1;
  *node = hs.node; *npre = hs.node >= 0 ? hs.npre : 0; *cost = hs.node >= 0 ? hs.cost : 0; *impact = hs.node >= 0 ? hs.impact : 0;
  return 0;
}
// indicative pricer: every node priced for one job (k_price_score over the node -> jobs index of the current binding state); detailNode >= 0: that node's victims in order
static int plat_price_score(Dev& d, const PriceArgs& a, std::vector<PriceNodeOut>& scores, int detailNode, std::vector<int32_t>* pre) {
  PlatCtx* c = t_ctx;
  int N = d.cfg.N, M = d.cfg.M;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t bOut = up(sizeof(PriceNodeOut) * (size_t)(N + 1)), bN = up(sizeof(int32_t) * (size_t)(N + 2)), bM = up(sizeof(int32_t) * 2 * (size_t)std::max(M, 1)),
         bE = up(sizeof(PriceEntry) * 2 * (size_t)std::max(M, 1));
  char* base = nullptr;
  if (!hipOk(hipMalloc(&base, bOut + 3 * bN + 2 * bM + bE), "pricer scratch")) return -1;
  PriceNodeOut* out = (PriceNodeOut*)base;
  int32_t* cnt = (int32_t*)(base + bOut); int32_t* off = (int32_t*)(base + bOut + bN); int32_t* cursor = (int32_t*)(base + bOut + 2 * bN);
  int32_t* jobs = (int32_t*)(base + bOut + 3 * bN); int32_t* dPre = (int32_t*)(base + bOut + 3 * bN + bM); PriceEntry* entries = (PriceEntry*)(base + bOut + 3 * bN + 2 * bM);
  (void)hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(N + 1), c->stream);
  hipLaunchKernelGGL(k_opt_count, dim3(bulkGrid(M)), dim3(256), 0, c->stream, d, cnt);
  hipLaunchKernelGGL(k_opt_scan, dim3(1), dim3(1024), 0, c->stream, (const int32_t*)cnt, off, cursor, N);
  hipLaunchKernelGGL(k_opt_scatter, dim3(bulkGrid(M)), dim3(256), 0, c->stream, d, cursor, jobs);
  (void)hipEventRecord(c->fitEv0, c->stream);
  hipLaunchKernelGGL(k_price_score, dim3((N + 127) / 128), dim3(128), 0, c->stream, d, a, (const int32_t*)off, (const int32_t*)jobs, entries, out);
  (void)hipEventRecord(c->fitEv1, c->stream);
  if (detailNode >= 0) hipLaunchKernelGGL(k_price_detail, dim3(1), dim3(64), 0, c->stream, d, a, (const int32_t*)off, (const int32_t*)jobs, entries, detailNode, out + N, dPre);
  bool ok = hipOk(hipGetLastError(), "pricer launch") && hipOk(hipStreamSynchronize(c->stream), "pricer kernels");
  (void)hipEventElapsedTime(&g_lastOptMs, c->fitEv0, c->fitEv1);
  if (ok) {
    scores.resize(N);
    if (N) ok = hipOk(hipMemcpy(scores.data(), out, sizeof(PriceNodeOut) * (size_t)N, hipMemcpyDeviceToHost), "pricer scores");
    if (ok && detailNode >= 0) {
      int npre = scores[detailNode].npre;
      pre->assign((size_t)std::max(npre, 1), -1);
      if (npre > 0) ok = hipOk(hipMemcpy(pre->data(), dPre, sizeof(int32_t) * (size_t)npre, hipMemcpyDeviceToHost), "pricer victims");
    }
  }
  (void)hipFree(base);
  return ok ? 0 : -1;
}
// the queue costs the last plat_opt_score evaluated (QueueContext.CurrentCost per queue)
static int plat_opt_qcosts(Dev& d, double* out, int Q) {
  PlatCtx* c = t_ctx;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t bOut = up(sizeof(OptNodeOut) * (size_t)(d.cfg.N + 1));
  return hipOk(hipMemcpy(out, (char*)c->optScratch + bOut, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost), "opt queue costs") ? 0 : -1;
}

// grid-wide order-preserving compaction; *total comes back to the host (the next launches are sized by it)
static int plat_compact(Dev& d, const int32_t* order, int n, const uint8_t* flag, int32_t* dst, uint32_t* prefix, const int32_t* segOff, int nseg, int32_t* outSegOff, int* total) {
  (void)d;
  PlatCtx* c = t_ctx;
  *total = 0;
  int nb = (n + CMP_CHUNK - 1) / CMP_CHUNK;
  size_t need = (size_t)nb + 8;
  if (c->cmpScratchInts < need) {
    if (c->cmpScratch) (void)hipFree(c->cmpScratch);
    c->cmpScratch = nullptr; c->cmpScratchInts = 0;
    if (!hipOk(hipMalloc((void**)&c->cmpScratch, need * 2 * sizeof(int32_t)), "compaction scratch")) return -1;
    c->cmpScratchInts = need * 2;
  }
  int32_t* blockCount = c->cmpScratch; int32_t* dTotal = c->cmpScratch + c->cmpScratchInts - 1;
  if (nb > 0) {
    hipLaunchKernelGGL(k_cmp_count, dim3(nb), dim3(256), 0, c->stream, order, n, flag, blockCount);
    hipLaunchKernelGGL(k_cmp_scan, dim3(1), dim3(64), 0, c->stream, blockCount, nb, dTotal);
    hipLaunchKernelGGL(k_cmp_write, dim3(nb), dim3(256), 0, c->stream, order, n, flag, dst, prefix, (const int32_t*)blockCount);
    c->roundLaunches += 3;
  } else (void)hipMemsetAsync(dTotal, 0, sizeof(int32_t), c->stream);
  if (segOff) { hipLaunchKernelGGL(k_seg_off, dim3((nseg + 256) / 256), dim3(256), 0, c->stream, segOff, nseg, n, (const uint32_t*)prefix, (const int32_t*)dTotal, outSegOff); c->roundLaunches++; }
  if (!hipOk(hipGetLastError(), "compaction launch")) return -1;
  int32_t t = 0;
  if (!hipOk(hipMemcpyAsync(&t, dTotal, sizeof t, hipMemcpyDeviceToHost, c->stream), "compaction total") || !hipOk(hipStreamSynchronize(c->stream), "compaction")) return -1;
  *total = t;
  return 0;
}
static int plat_build_base(Dev& d) {
  int N = d.cfg.N;
  int nb2 = 64; while (nb2 < N) nb2 <<= 1;
  hipLaunchKernelGGL(k_base_fill, dim3((nb2 + 255) / 256), dim3(256), 0, t_ctx->stream, d, nb2);
  unsigned long long* a = (unsigned long long*)d.baseKey;
  if (nb2 <= 4096) {
    // k_bitonic_step has no bound on its index and baseKey holds exactly nb2 keys (buildFast): the launch is exactly nb2 threads — one workgroup of 64 or 128
    // for pools of <= 128 nodes, whole workgroups of 256 above.  (The tile kernel is only used when the array is a multiple of 4096.)
    const int tpb = std::min(nb2, 256);
    for (int k = 2; k <= nb2; k <<= 1) for (int j = k >> 1; j > 0; j >>= 1) hipLaunchKernelGGL(k_bitonic_step, dim3(nb2 / tpb), dim3(tpb), 0, t_ctx->stream, a, j, k);
  } else {
    int tiles = nb2 / 4096;
    hipLaunchKernelGGL(k_bitonic_tile, dim3(tiles), dim3(1024), 0, t_ctx->stream, a, 2, 4096, 1);  // all steps with k <= 4096
    for (int k = 8192; k <= nb2; k <<= 1) {
      int j = k >> 1;
      for (; j >= 4096; j >>= 1) hipLaunchKernelGGL(k_bitonic_step, dim3((nb2 + 255) / 256), dim3(256), 0, t_ctx->stream, a, j, k);
      hipLaunchKernelGGL(k_bitonic_tile, dim3(tiles), dim3(1024), 0, t_ctx->stream, a, k, k, 2048);      // remaining steps j = 2048..1 inside tiles
    }
  }
  hipLaunchKernelGGL(k_base_finish, dim3((N + 255) / 256), dim3(256), 0, t_ctx->stream, d);
  if (d.fitBits) { size_t total = (size_t)d.f.F * d.fitW; hipLaunchKernelGGL(k_base_fitbits, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, t_ctx->stream, d); }
  if (!hipOk(hipGetLastError(), "base build launch")) return -1;
  if (!hipOk(hipStreamSynchronize(t_ctx->stream), "base build")) return -1;
  return 0;
}
static int plat_run_shape_mask(Dev& d, const uint64_t* classMask, const int32_t* shapeClass) {
  size_t total = (size_t)d.cfg.S * d.cfg.W;
  if (total == 0) return 0;
  hipLaunchKernelGGL(k_shape_mask, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, t_ctx->stream, d, classMask, shapeClass);
  if (!hipOk(hipGetLastError(), "k_shape_mask launch")) return -1;
  if (!hipOk(hipStreamSynchronize(t_ctx->stream), "k_shape_mask")) return -1;
  return 0;
}

// kernel duration of the last fit batch, measured with HIP events on the launch stream
static double plat_last_fit_ms() { return t_ctx ? (double)t_ctx->lastFitMs : 0.0; }

// (the scratch of a fit batch is kept across calls and the rank -> node table is the host's own copy: the call is launch + one small download, nothing else)
static int plat_run_fit_batch(Dev& d, const std::vector<int32_t>& shapes, int level, std::vector<int32_t>& out, const int32_t* nodeByRankHost) {
  int ns = (int)shapes.size();
  if (ns == 0) return 0;
  PlatCtx* c = t_ctx;
  size_t need = (size_t)ns * (sizeof(int32_t) + FIT_OSTR * sizeof(unsigned long long)) + 16;
  if (c->fitScratchBytes < need) {
    if (c->fitScratch) (void)hipFree(c->fitScratch);
    c->fitScratch = nullptr; c->fitScratchBytes = 0;
    if (!hipOk(hipMalloc(&c->fitScratch, need * 2), "hipMalloc")) return -1;
    c->fitScratchBytes = need * 2;
  }
  unsigned long long* dOut = (unsigned long long*)c->fitScratch; int32_t* dShapes = (int32_t*)(dOut + (size_t)ns * FIT_OSTR);
  (void)hipMemcpyAsync(dShapes, shapes.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, t_ctx->stream);
  (void)hipMemsetAsync(dOut, 0xff, (size_t)ns * FIT_OSTR * sizeof(unsigned long long), t_ctx->stream);
  int tiles = (d.cfg.N + FIT_TILE - 1) / FIT_TILE;
  int ysplit = std::max(1, std::min(ns, (2048 + tiles - 1) / tiles));  // >= ~2048 workgroups when the node count alone cannot fill 256 CUs
  hipEvent_t e0 = t_ctx->fitEv0, e1 = t_ctx->fitEv1;
  (void)hipEventRecord(e0, t_ctx->stream);
  const bool two = d.cfg.keyWords == 2;   // a two-word order key: one launch per word (armada_sched_wk.hip k_fit_batch_wk), the low word of the minimum in word 1
  if (two) { if (asched_internal_wk_fit_batch(&d, dShapes, ns, level, dOut, tiles, ysplit, t_ctx->stream)) { c->err = "k_fit_batch_wk launch failed"; return -1; } }
  else
  hipLaunchKernelGGL(k_fit_batch, dim3(tiles, ysplit), dim3(FIT_TILE), 0, t_ctx->stream, d, dShapes, ns, level, dOut);
  (void)hipEventRecord(e1, t_ctx->stream);
  std::vector<unsigned long long> wide((size_t)ns * FIT_OSTR), keys(ns);
  bool ok = hipOk(hipGetLastError(), "k_fit_batch launch") && hipOk(hipMemcpyAsync(wide.data(), dOut, wide.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, t_ctx->stream), "hipMemcpy") &&
            hipOk(hipStreamSynchronize(t_ctx->stream), "k_fit_batch");
  (void)hipEventElapsedTime(&t_ctx->lastFitMs, e0, e1);
  if (!ok) return -1;
  for (int i = 0; i < ns; i++) keys[i] = (two && wide[(size_t)i * FIT_OSTR] != ~0ull) ? wide[(size_t)i * FIT_OSTR + 1] : wide[(size_t)i * FIT_OSTR];
  std::vector<int32_t> nodeByRank;
  if (!nodeByRankHost) { nodeByRank.resize(d.cfg.N); if (d.cfg.N) (void)hipMemcpy(nodeByRank.data(), d.nodeByRank, d.cfg.N * sizeof(int32_t), hipMemcpyDeviceToHost); nodeByRankHost = nodeByRank.data(); }
  unsigned long long mask = (1ull << d.cfg.idxBits) - 1;
  for (int i = 0; i < ns; i++) out[i] = keys[i] == ~0ull ? -1 : nodeByRankHost[keys[i] & mask];
  return 0;
}
// ---- one pool on several GPUs: the kernels live in armada_sched_mgpu.hip (their own code object)
#include "mgpu.h"
extern "C" int asched_internal_mgpu_pack(const Dev* d, const GlobalKeyLayout* L, int level, const unsigned long long* keys, const int32_t* slot, int nq, long long* out, int32_t* bad, hipStream_t s);
extern "C" int asched_internal_mgpu_delta(const Dev* d, long long* buf, int ns, int np, hipStream_t s);
extern "C" int asched_internal_mgpu_resolve(const Dev* d, const long long* red, long long* freeC, uint8_t* ownPre, uint8_t* conflict, uint8_t* gangReplay,
                                            int32_t* node, int32_t* prio, uint8_t* replay, int32_t* counts, int ns, int np, hipStream_t s);
// the handle's scratch buffer of the fit / capacity / gang-unit launches (kept across calls: an allocation per call showed up as a 13 ms outlier among 0.06 ms calls)
static void* plat_fit_scratch(size_t need) {
  PlatCtx* c = t_ctx;
  if (c->fitScratchBytes < need) {
    if (c->fitScratch) (void)hipFree(c->fitScratch);
    c->fitScratch = nullptr; c->fitScratchBytes = 0;
    if (!hipOk(hipMalloc(&c->fitScratch, need * 2), "hipMalloc")) return nullptr;
    c->fitScratchBytes = need * 2;
  }
  return c->fitScratch;
}
// the submit check's gang units, one workgroup per unit (submit_gang.h; the kernel lives in armada_sched_mgpu.hip).  out: 4 words per unit; the kernel time goes to lastFitMs
extern "C" int asched_internal_submit_gangs(const Dev* d, const int32_t* off, const int32_t* jobs, int nu, int32_t* out, hipStream_t s);
#define SG_MAX_NODES 262144   // the workgroup's node bitmap lives in LDS (32 KB at this size)
static int plat_run_submit_gangs(Dev& d, const std::vector<int32_t>& off, const std::vector<int32_t>& jobs, std::vector<int32_t>& out) {
  int nu = (int)off.size() - 1;
  out.assign((size_t)std::max(nu, 0) * 4, 0);
  if (nu <= 0) return 0;
  hipStream_t st = t_ctx->stream;
  size_t nOff = (off.size() + 3) & ~(size_t)3, nJobs = (std::max<size_t>(jobs.size(), 1) + 3) & ~(size_t)3;
  int32_t* base = (int32_t*)plat_fit_scratch((nOff + nJobs + out.size()) * 4);
  bool ok = base != nullptr;
  int32_t *dOff = base, *dJobs = base + nOff, *dOut = base + nOff + nJobs;
  if (ok) {
    (void)hipMemcpyAsync(dOff, off.data(), off.size() * 4, hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(dJobs, jobs.data(), jobs.size() * 4, hipMemcpyHostToDevice, st);
    (void)hipEventRecord(t_ctx->fitEv0, st);
    ok = asched_internal_submit_gangs(&d, dOff, dJobs, nu, dOut, st) == 0;
    (void)hipEventRecord(t_ctx->fitEv1, st);
    ok = ok && hipOk(hipMemcpyAsync(out.data(), dOut, out.size() * 4, hipMemcpyDeviceToHost, st), "hipMemcpy") && hipOk(hipStreamSynchronize(st), "k_submit_gangs");
    (void)hipEventElapsedTime(&t_ctx->lastFitMs, t_ctx->fitEv0, t_ctx->fitEv1);
  }
  return ok ? 0 : -1;
}
// the evicted table by rank (replay_rank.h; kernels in armada_sched_mgpu.hip): three launches on the handle's stream, no read-back
extern "C" int asched_internal_replay_rank(const Dev* d, int n, int keepPending, hipStream_t s);
static int plat_replay_rank(Dev& d, int n, int keepPending) {
  if (n <= 0) return 0;
  t_ctx->roundLaunches += 3;
  return asched_internal_replay_rank(&d, n, keepPending, t_ctx->stream) == 0 && hipOk(hipGetLastError(), "k_replay_rank launch") ? 0 : -1;
}
// uniform submit-check units (submit_gang.h): per shape {first node or -1, members all nodes take together}
extern "C" int asched_internal_fit_capacity(const Dev* d, const int32_t* shapes, int ns, unsigned long long* out, hipStream_t s);
static int plat_run_fit_capacity(Dev& d, const std::vector<int32_t>& shapes, std::vector<int32_t>& firstNode, std::vector<long long>& capacity, const int32_t* nodeByRankHost) {
  int ns = (int)shapes.size();
  firstNode.assign(ns, -1); capacity.assign(ns, 0);
  if (ns == 0 || d.cfg.N == 0) return 0;
  hipStream_t st = t_ctx->stream;
  size_t words = (size_t)ns * FIT_OSTR;
  unsigned long long* dOut = (unsigned long long*)plat_fit_scratch(words * 8 + (size_t)ns * 4 + 16);
  int32_t* dShapes = (int32_t*)(dOut + words);
  bool ok = dOut != nullptr;
  std::vector<unsigned long long> init(words, 0), got(words);
  for (int i = 0; i < ns; i++) init[(size_t)i * FIT_OSTR] = ~0ull;
  if (ok) {
    (void)hipMemcpyAsync(dOut, init.data(), words * 8, hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(dShapes, shapes.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st);
    (void)hipEventRecord(t_ctx->fitEv0, st);
    ok = asched_internal_fit_capacity(&d, dShapes, ns, dOut, st) == 0;
    (void)hipEventRecord(t_ctx->fitEv1, st);
    ok = ok && hipOk(hipMemcpyAsync(got.data(), dOut, words * 8, hipMemcpyDeviceToHost, st), "hipMemcpy") && hipOk(hipStreamSynchronize(st), "k_fit_capacity");
    (void)hipEventElapsedTime(&t_ctx->lastFitMs, t_ctx->fitEv0, t_ctx->fitEv1);
  }
  if (!ok) return -1;
  unsigned long long mask = (1ull << d.cfg.idxBits) - 1;
  for (int i = 0; i < ns; i++) {
    unsigned long long k = got[(size_t)i * FIT_OSTR];
    firstNode[i] = k == ~0ull ? -1 : nodeByRankHost[k & mask];
    capacity[i] = (long long)got[(size_t)i * FIT_OSTR + 1];
  }
  return 0;
}
// the literal batched first fit (kernels_fit_lit.h; kernels in armada_sched_mgpu.hip): index build (fill, bitonic sort by (type, key), finish) then one wave per query.
// ASCHED_FIT_LIT_TIMES=1 prints the two device times of every call (tools/probe_fit_literal.py).
#include "kernels_fit_lit.h"
extern "C" int asched_internal_fit_lit_build(const Dev* d, const FitLitIdx* x, const int32_t* nodeType, FlPair* a, int nb2, hipStream_t s);
extern "C" int asched_internal_fit_lit_query(const Dev* d, const FitLitIdx* x, const int32_t* rows, int nq, int32_t* out, hipStream_t s);
static int plat_run_fit_batch_lit(Dev& d, const int32_t* nodeType, int nTypes, const std::vector<int32_t>& rows, int level, std::vector<int32_t>& out, bool reuseIndex, double addMs) {
  int nq = (int)rows.size(), N = d.cfg.N;
  if (nq == 0) return 0;
  if (N <= 0) { for (int i = 0; i < nq; i++) out[i] = -1; return 0; }
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  size_t nb2 = FL_TILE; while (nb2 < (size_t)N) nb2 <<= 1;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  // layout: [index: key | node | planes | typeBeg | typeEnd] [sort scratch] [rows | results]: the index part depends on N, R and the type count only, so a reused index stays where it is
  size_t oKey = 0, oNode = oKey + up((size_t)N * 8), oAl = oNode + up((size_t)N * 4), oBeg = oAl + up((size_t)d.cfg.R * N * 8), oEnd = oBeg + up((size_t)std::max(nTypes, 1) * 4),
         oPair = oEnd + up((size_t)std::max(nTypes, 1) * 4), oRows = oPair + up(nb2 * sizeof(FlPair)), oOut = oRows + up((size_t)nq * 4), need = oOut + up((size_t)nq * 4);
  if (c->litScratchBytes < need) {
    reuseIndex = false;   // (the index moves with the buffer: build it again)
    if (c->litScratch) (void)hipFree(c->litScratch);
    c->litScratch = nullptr; c->litScratchBytes = 0;
    if (!hipOk(hipMalloc(&c->litScratch, need * 2), "hipMalloc")) return -1;
    c->litScratchBytes = need * 2;
  }
  char* base = (char*)c->litScratch;
  FitLitIdx x;
  x.key = (unsigned long long*)(base + oKey); x.node = (int32_t*)(base + oNode); x.al = (int64_t*)(base + oAl); x.typeBeg = (int32_t*)(base + oBeg); x.typeEnd = (int32_t*)(base + oEnd);
  x.n = N; x.stride = N; x.level = level; x.pad = 0;
  int32_t *dRows = (int32_t*)(base + oRows), *dOut = (int32_t*)(base + oOut);
  (void)hipMemcpyAsync(dRows, rows.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st);
  bool ok = true;
  (void)hipEventRecord(c->fitEv0, st);
  if (!reuseIndex) {
    (void)hipMemsetAsync(base + oBeg, 0, oPair - oBeg, st);
    ok = asched_internal_fit_lit_build(&d, &x, nodeType, (FlPair*)(base + oPair), (int)nb2, st) == 0;
  }
  (void)hipEventRecord(c->litEvMid, st);
  ok = ok && asched_internal_fit_lit_query(&d, &x, dRows, nq, dOut, st) == 0;
  (void)hipEventRecord(c->fitEv1, st);
  ok = ok && hipOk(hipGetLastError(), "k_fit_lit launch") && hipOk(hipMemcpyAsync(out.data(), dOut, (size_t)nq * 4, hipMemcpyDeviceToHost, st), "hipMemcpy") && hipOk(hipStreamSynchronize(st), "k_fit_lit");
  if (!ok) { if (c->err.empty()) c->err = "k_fit_lit launch failed"; return -1; }
  float buildMs = 0.f, queryMs = 0.f;
  (void)hipEventElapsedTime(&buildMs, c->fitEv0, c->litEvMid); (void)hipEventElapsedTime(&queryMs, c->litEvMid, c->fitEv1);
  c->lastFitMs = buildMs + queryMs + (float)addMs;
  if (const char* e = getenv("ASCHED_FIT_LIT_TIMES")) if (e[0] == '1') fprintf(stderr, "[asched fit_lit] nodes %d queries %d level %d: index build %.4f ms, query %.4f ms\n", N, nq, level, (double)buildMs, (double)queryMs);
  return 0;
}
// ---- the pass timer of plat.h's measurement hooks (kPassFamilies), and the end every table call shares
// A family's variable is read at the first call of the family in the process.  passBegin: the family's events, created at the first timed call of the handle, or nullptr
// when the family is off or an event could not be created (that call runs untimed: the events that exist stay, nothing is latched); it clears the timed flag, so a
// call that returns early reports zeros.  Untimed, a call pays one null test per passRecord and issues no HIP call of the timer's.
static bool passTimesOn(int f) {
  static std::atomic<signed char> on[PASS_FAMILIES];   // 0: not read yet, 1: off, 2: on
  signed char v = on[f].load(std::memory_order_relaxed);
  if (!v) { v = plat_pass_printed((PassFamily)f) ? 2 : 1; on[f].store(v, std::memory_order_relaxed); }
  return v == 2;
}
static hipEvent_t* passBegin(int f, int pass = 0) {
  PassTimer& t = t_ctx->pass[f];
  t.timed &= ~(1u << pass);
  if (!passTimesOn(f)) return nullptr;
  const int n = passEvents(f);
  if (!t.ev[n - 1]) for (int i = 0; i < n; i++) if (!t.ev[i] && hipEventCreate(&t.ev[i]) != hipSuccess) { t.ev[i] = nullptr; return nullptr; }
  return t.ev;
}
static inline void passRecord(hipEvent_t* ev, int i, hipStream_t st) { if (ev) (void)hipEventRecord(ev[i], st); }
static inline void passTimed(int f, hipEvent_t* ev, int pass = 0) { if (ev) t_ctx->pass[f].timed |= 1u << pass; }
static void plat_pass_ms(PassFamily f, double* out) {
  const PassFamilyInfo& fam = kPassFamilies[f]; const PassTimer& t = t_ctx->pass[f];
  for (int k = 0; k < fam.passes; k++) {
    const int e = fam.layout == PASS_PAIRS ? 2 * k : fam.layout == PASS_REV ? fam.passes - 1 - k : k, bit = fam.layout == PASS_PAIRS ? k : 0;
    float ms = 0.f; if (((t.timed >> bit) & 1) && hipEventElapsedTime(&ms, t.ev[e], t.ev[e + 1]) != hipSuccess) ms = 0.f; out[k] = ms; }
}
// the end of a synchronous call: the last launch error ("<k> launch"), the wait for the stream ("<k>"), "<failed> launch failed" where nothing said more, and the family's
// timed flag (f < 0: the call has no timer)
static int launchTail(bool ok, const char* k, const char* failed, int f = -1, hipEvent_t* ev = nullptr) {
  PlatCtx* c = t_ctx;
  if (ok) { const hipError_t e = hipGetLastError(); if (e != hipSuccess) ok = hipOk(e, (std::string(k) + " launch").c_str()); }
  if (ok) { const hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess) ok = hipOk(e, k); }
  if (!ok) { if (c->err.empty()) c->err = std::string(failed) + " launch failed"; return -1; }
  if (f >= 0) passTimed(f, ev);
  return 0;
}
// the preemption-cause join (kernels_preempt_join.h; kernels in armada_sched_mgpu.hip).  ASCHED_PJOIN_TIMES=1 prints the device time of every call (tools/probe_preemption_causes.py).
#include "kernels_preempt_join.h"
extern "C" int asched_internal_preempt_join(const Dev* d, const PjArgs* a, hipStream_t s);
static int plat_preempt_join(Dev& d, const PjArgs& a) {
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  (void)hipEventRecord(c->fitEv0, st);
  bool ok = asched_internal_preempt_join(&d, &a, st) == 0;
  (void)hipEventRecord(c->fitEv1, st);
  if (launchTail(ok, "k_pj", "k_pj")) return -1;
  (void)hipEventElapsedTime(&c->lastFitMs, c->fitEv0, c->fitEv1);
  if (const char* e = getenv("ASCHED_PJOIN_TIMES")) if (e[0] == '1') fprintf(stderr, "[asched preempt_join] nodes %d scheduled %d preempted %d: %.4f ms\n", a.N, a.ns, a.np, (double)c->lastFitMs);
  return 0;
}
// the evictor report of a round's phase 1 (kernels_evict_report.h; kernels in armada_sched_mgpu.hip): one launch per pass on the round's stream.  PASS_EVR puts a pair
// of events around every pass, with a flag per pass; they are read once the round is over (tools/probe_evictor_report.py).
#include "kernels_evict_report.h"
extern "C" int asched_internal_evict_report(const Dev* d, const EvrArgs* a, int pass, hipStream_t s);
static int plat_evict_report(Dev& d, const EvrArgs& a, int pass) {
  if ((pass == EVR_PASS_JOBS && a.M <= 0) || (pass == EVR_PASS_NODES && a.N <= 0)) return 0;
  PlatCtx* c = t_ctx;
  hipEvent_t* ev = passBegin(PASS_EVR, pass);
  passRecord(ev, 2 * pass, c->stream);
  bool ok = asched_internal_evict_report(&d, &a, pass, c->stream) == 0;
  passRecord(ev, 2 * pass + 1, c->stream);
  passTimed(PASS_EVR, ev, pass);
  c->roundLaunches++;
  if (!ok) { c->err = "k_evr launch failed"; return -1; }
  return 0;
}
// the run-state patch of the resident job table (kernels_jobs_patch.h; kernels in armada_sched_mgpu.hip): scatter + keys, the compaction of the untouched rows (its count
// comes back to the host: the merge is sized by it), the sort, the merge.  PASS_JP (tools/probe_jobs_patch.py).
#include "kernels_jobs_patch.h"
extern "C" int asched_internal_jp_scatter(const Dev* d, const JpArgs* a, hipStream_t s);
extern "C" int asched_internal_jp_sort(const JpArgs* a, hipStream_t s);
extern "C" int asched_internal_jp_merge(const Dev* d, const JpArgs* a, hipStream_t s);
// the four passes behind one another; scatter: the launch of the caller's scatter (the patch's or the reprioritise's), launched between the first two events
template <class Scatter> static int jpPasses(Dev& d, JpArgs& a, int32_t* keptBuf, Scatter scatter) {
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  hipEvent_t* ev = passBegin(PASS_JP);
  passRecord(ev, 0, st);
  bool ok = scatter(st) == 0;
  passRecord(ev, 1, st);
  a.kept = keptBuf; a.nKept = 0;
  if (ok && a.nT > 0) {
    int nk = 0;
    if (plat_compact(d, d.ordAll, a.total, a.keep, keptBuf, nullptr, nullptr, 0, nullptr, &nk)) return -1;
    a.nKept = nk;
    if (a.nT + a.nKept != a.total) { c->err = "jobs_patch: the job order lost or gained rows"; return -1; }
    passRecord(ev, 2, st);
    ok = asched_internal_jp_sort(&a, st) == 0;
  } else passRecord(ev, 2, st);
  passRecord(ev, 3, st);
  ok = ok && asched_internal_jp_merge(&d, &a, st) == 0;
  passRecord(ev, 4, st);
  return launchTail(ok, "k_jp", "k_jp", PASS_JP, ev);
}
static int plat_jobs_patch(Dev& d, JpArgs& a, int32_t* keptBuf) { return jpPasses(d, a, keptBuf, [&](hipStream_t st) { return asched_internal_jp_scatter(&d, &a, st); }); }
// queue priorities of resident jobs change (kernels_jobs_reprioritise.h; k_jr_scatter in armada_sched_mgpu.hip): its own scatter, then the patch's remove, sort and
// merge.  The events are the patch's (PASS_JP; tools/probe_jobs_reprioritise.py).
#include "kernels_jobs_reprioritise.h"
extern "C" int asched_internal_jr_scatter(const Dev* d, const JrArgs* a, hipStream_t s);
static int plat_jobs_reprioritise(Dev& d, JrArgs& a, int32_t* keptBuf) { return jpPasses(d, a.p, keptBuf, [&](hipStream_t st) { return asched_internal_jr_scatter(&d, &a, st); }); }
// a round's result applied to the resident jobs (kernels_round_commit.h; k_rc_scatter in armada_sched_mgpu.hip): its own scatter, then the patch's remove, sort and
// merge.  The events are the patch's (PASS_JP; tools/probe_round_commit.py).
#include "kernels_round_commit.h"
extern "C" int asched_internal_rc_scatter(const Dev* d, const RcArgs* a, hipStream_t s);
static int plat_round_commit(Dev& d, RcArgs& a, int32_t* keptBuf) { return jpPasses(d, a.p, keptBuf, [&](hipStream_t st) { return asched_internal_rc_scatter(&d, &a, st); }); }
// retried jobs change class and request in place (kernels_jobs_respec.h; k_js_scatter in armada_sched_mgpu.hip): one launch on the handle's stream, waited for
#include "kernels_jobs_respec.h"
extern "C" int asched_internal_js_scatter(const Dev* d, const JsArgs* a, hipStream_t s);
static int plat_jobs_respec(Dev& d, JsArgs& a) { return launchTail(asched_internal_js_scatter(&d, &a, t_ctx->stream) == 0, "k_js", "k_js_scatter"); }
// newly submitted jobs behind the resident job table (kernels_jobs_append.h; k_ja_fill in armada_sched_mgpu.hip, the sort and the merge are the patch's kernels).
// PASS_JA (tools/probe_jobs_append.py).
#include "kernels_jobs_append.h"
extern "C" int asched_internal_ja_fill(const Dev* d, const JaArgs* a, hipStream_t s);
static int plat_jobs_append(Dev& d, JaArgs& a) {
  hipStream_t st = t_ctx->stream;
  hipEvent_t* ev = passBegin(PASS_JA);
  passRecord(ev, 0, st);
  bool ok = asched_internal_ja_fill(&d, &a, st) == 0;
  passRecord(ev, 1, st);
  if (ok && a.p.nT > 0) ok = asched_internal_jp_sort(&a.p, st) == 0;
  passRecord(ev, 2, st);
  if (ok && a.p.nT > 0) ok = asched_internal_jp_merge(&d, &a.p, st) == 0;
  passRecord(ev, 3, st);
  return launchTail(ok, "k_ja", "k_ja", PASS_JA, ev);
}
// new rows join a mask whose resident rows move into a fresh block: the shape mask (kernels_shapes_append.h; k_sa_mask in armada_sched_mgpu.hip; PASS_SA, switched by
// the job append's variable; tools/probe_jobs_append_shapes.py) and the class mask (kernels_req_classes_append.h; k_ca_rows; PASS_CA; tools/probe_req_classes_append.py).
// The row copies between events 0 and 1, the launch of the new rows between 1 and 2.
#include "kernels_shapes_append.h"
#include "kernels_req_classes_append.h"
extern "C" int asched_internal_sa_mask(const SaArgs* a, hipStream_t s);
extern "C" int asched_internal_ca_rows(const CaArgs* a, hipStream_t s);
template <class Args> static int maskRowsAppend(Args& a, int (*rows)(const Args*, hipStream_t), PassFamily f, const char* k, const char* failed) {
  hipStream_t st = t_ctx->stream;
  hipEvent_t* ev = passBegin(f);
  passRecord(ev, 0, st);
  if (a.copy0 > 0) plat_d2d(a.outMask, a.inMask, (size_t)a.copy0 * 8);
  if (a.copy1 > 0) plat_d2d(a.outMask + a.dst1, a.inMask + a.src1, (size_t)a.copy1 * 8);
  passRecord(ev, 1, st);
  bool ok = rows(&a, st) == 0;
  passRecord(ev, 2, st);
  return launchTail(ok, k, failed, f, ev);
}
static int plat_shapes_append(Dev&, SaArgs& a) { return maskRowsAppend(a, asched_internal_sa_mask, PASS_SA, "k_sa", "k_sa_mask"); }
static int plat_req_classes_append(Dev&, CaArgs& a) { return maskRowsAppend(a, asched_internal_ca_rows, PASS_CA, "k_ca", "k_ca_rows"); }
// dead shapes and classes leave the resident tables (kernels_shapes_compact.h; k_sc_* in armada_sched_mgpu.hip).  PASS_SC (tools/probe_shapes_compact.py).
#include "kernels_shapes_compact.h"
extern "C" int asched_internal_sc_rows(const ScArgs* a, hipStream_t s);
extern "C" int asched_internal_sc_gather(const ScArgs* a, hipStream_t s);
extern "C" int asched_internal_sc_clsbits(const ScArgs* a, hipStream_t s);
static int plat_shapes_compact(Dev&, ScArgs& a) {
  hipStream_t st = t_ctx->stream;
  hipEvent_t* ev = passBegin(PASS_SC);
  passRecord(ev, 0, st);
  bool ok = asched_internal_sc_rows(&a, st) == 0;
  passRecord(ev, 1, st);
  ok = ok && asched_internal_sc_gather(&a, st) == 0;
  passRecord(ev, 2, st);
  ok = ok && asched_internal_sc_clsbits(&a, st) == 0;
  passRecord(ev, 3, st);
  return launchTail(ok, "k_sc", "k_sc", PASS_SC, ev);
}
// rows leave the resident job table (kernels_jobs_delete.h; k_jd_* in armada_sched_mgpu.hip, the scans are plat_compact's).  Each compaction brings its count back to the
// host, which checks it against what the host counted before the next pass is sized by it.  PASS_JD (tools/probe_jobs_delete.py).
#include "kernels_jobs_delete.h"
extern "C" int asched_internal_jd_mark(const JdArgs* a, int value, hipStream_t s);
extern "C" int asched_internal_jd_gather(const JdArgs* a, hipStream_t s);
extern "C" int asched_internal_jd_remap(const JdArgs* a, int32_t* list, int n, hipStream_t s);
static int plat_jobs_delete(Dev& d, JdArgs& a) {
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  hipEvent_t* ev = passBegin(PASS_JD);
  passRecord(ev, 0, st);
  if (asched_internal_jd_mark(&a, 0, st)) { c->err = "k_jd_mark launch failed"; return -1; }
  passRecord(ev, 1, st);
  int m1 = 0;
  if (plat_compact(d, nullptr, a.M, a.keep, a.src, a.newId, nullptr, 0, nullptr, &m1)) return -1;
  if (m1 != a.M1) { c->err = "jobs_delete: the scan kept another number of rows than the host counted"; return -1; }
  passRecord(ev, 2, st);
  if (asched_internal_jd_gather(&a, st)) { c->err = "k_jd_gather launch failed"; return -1; }
  passRecord(ev, 3, st);
  if (a.total > 0) {
    int t1 = 0;
    if (plat_compact(d, a.ordIn, a.total, a.keep, a.ordOut, nullptr, nullptr, 0, nullptr, &t1)) return -1;
    if (t1 != a.total1) { c->err = "jobs_delete: the job order lost or gained rows"; return -1; }
    if (asched_internal_jd_remap(&a, a.ordOut, a.total1, st)) { c->err = "k_jd_remap launch failed"; return -1; }
  }
  passRecord(ev, 4, st);
  if (a.gangLen > 0) {
    int g1 = 0;
    if (plat_compact(d, a.gangIn, a.gangLen, a.keep, a.gangOut, nullptr, nullptr, 0, nullptr, &g1)) return -1;
    if (g1 != a.gangLen1) { c->err = "jobs_delete: the gang lists lost or gained rows"; return -1; }
    if (asched_internal_jd_remap(&a, a.gangOut, a.gangLen1, st)) { c->err = "k_jd_remap launch failed"; return -1; }
  }
  passRecord(ev, 5, st);
  return launchTail(asched_internal_jd_mark(&a, 1, st) == 0, "k_jd", "k_jd", PASS_JD, ev);
}
// cordons and capacity changes of resident nodes (kernels_nodes_patch.h; k_np_scatter / k_np_mask in armada_sched_mgpu.hip).  PASS_NP (tools/probe_nodes_patch.py).
#include "kernels_nodes_patch.h"
extern "C" int asched_internal_np_scatter(const Dev* d, const NpArgs* a, hipStream_t s);
extern "C" int asched_internal_np_mask(const Dev* d, const NpArgs* a, hipStream_t s);
static int plat_nodes_patch(Dev& d, const NpArgs& a) {
  hipStream_t st = t_ctx->stream;
  hipEvent_t* ev = passBegin(PASS_NP);
  passRecord(ev, 0, st);
  bool ok = asched_internal_np_scatter(&d, &a, st) == 0;
  passRecord(ev, 1, st);
  ok = ok && asched_internal_np_mask(&d, &a, st) == 0;
  passRecord(ev, 2, st);
  return launchTail(ok, "k_np", "k_np", PASS_NP, ev);
}
// rows leave the resident node table (kernels_nodes_delete.h; k_nd_* in armada_sched_mgpu.hip, the scans are plat_compact's).  The check brings its word back to the host
// before anything is written; each compaction brings its count back.  PASS_ND spans both calls: the check clears the flag and records events 0 and 1, the delete
// records 2 to 7 and sets it (tools/probe_nodes_delete.py).
#include "kernels_nodes_delete.h"
extern "C" int asched_internal_nd_mark(const NdArgs* a, int value, hipStream_t s);
extern "C" int asched_internal_nd_check(const NdArgs* a, hipStream_t s);
extern "C" int asched_internal_nd_gather(const NdArgs* a, hipStream_t s);
extern "C" int asched_internal_nd_rank(const NdArgs* a, hipStream_t s);
extern "C" int asched_internal_nd_mask(const NdArgs* a, hipStream_t s);
extern "C" int asched_internal_nd_job(const NdArgs* a, hipStream_t s);
static int plat_nodes_delete_check(Dev&, NdArgs& a, int32_t* bad) {
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  hipEvent_t* ev = passBegin(PASS_ND);
  *bad = ND_NONE;
  const int32_t none = ND_NONE;
  passRecord(ev, 0, st);
  if (!hipOk(hipMemcpyAsync(a.bad, &none, sizeof none, hipMemcpyHostToDevice, st), "nodes_delete check word")) return -1;
  if (asched_internal_nd_mark(&a, 0, st)) { c->err = "k_nd_mark launch failed"; return -1; }
  if (asched_internal_nd_check(&a, st)) { c->err = "k_nd_check launch failed"; return -1; }
  passRecord(ev, 1, st);
  int32_t t = ND_NONE;
  if (!hipOk(hipMemcpyAsync(&t, a.bad, sizeof t, hipMemcpyDeviceToHost, st), "nodes_delete check word") || !hipOk(hipStreamSynchronize(st), "k_nd_check")) return -1;
  *bad = t;
  if (t != ND_NONE) {
    if (asched_internal_nd_mark(&a, 1, st) || !hipOk(hipStreamSynchronize(st), "k_nd_mark")) { if (c->err.empty()) c->err = "k_nd_mark launch failed"; return -1; }
  }
  return 0;
}
static int plat_nodes_delete(Dev& d, NdArgs& a) {
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  hipEvent_t* ev = passBegin(PASS_ND);
  int n1 = 0;
  if (plat_compact(d, nullptr, a.N, a.keep, a.src, a.newId, nullptr, 0, nullptr, &n1)) return -1;
  if (n1 != a.N1) { c->err = "nodes_delete: the scan kept another number of rows than the host counted"; return -1; }
  passRecord(ev, 2, st);
  if (!a.jobsOnly && asched_internal_nd_gather(&a, st)) { c->err = "k_nd_gather launch failed"; return -1; }
  passRecord(ev, 3, st);
  if (!a.jobsOnly) {
    int r1 = 0;
    if (plat_compact(d, a.rankIn, a.N, a.keep, a.rankOut, nullptr, nullptr, 0, nullptr, &r1)) return -1;
    if (r1 != a.N1) { c->err = "nodes_delete: the index order lost or gained rows"; return -1; }
    if (asched_internal_nd_rank(&a, st)) { c->err = "k_nd_rank launch failed"; return -1; }
  }
  passRecord(ev, 4, st);
  if (!a.jobsOnly && asched_internal_nd_mask(&a, st)) { c->err = "k_nd_mask launch failed"; return -1; }
  passRecord(ev, 5, st);
  if (asched_internal_nd_job(&a, st)) { c->err = "k_nd_job launch failed"; return -1; }
  passRecord(ev, 6, st);
  bool ok = asched_internal_nd_mark(&a, 1, st) == 0;
  passRecord(ev, 7, st);
  return launchTail(ok, "k_nd", "k_nd", PASS_ND, ev);
}
// new rows join the resident node table (kernels_nodes_append.h; k_na_* in armada_sched_mgpu.hip).  PASS_NA (tools/probe_nodes_append.py).
#include "kernels_nodes_append.h"
extern "C" int asched_internal_na_planes(const NaArgs* a, hipStream_t s);
extern "C" int asched_internal_na_narrow(const NaArgs* a, hipStream_t s);
extern "C" int asched_internal_na_rank(const NaArgs* a, hipStream_t s);
extern "C" int asched_internal_na_mask(const NaArgs* a, hipStream_t s);
static int plat_nodes_append(Dev&, NaArgs& a) {
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  hipEvent_t* ev = passBegin(PASS_NA);
  passRecord(ev, 0, st);
  if (asched_internal_na_planes(&a, st)) { c->err = "k_na_plane launch failed"; return -1; }
  passRecord(ev, 1, st);
  if (asched_internal_na_narrow(&a, st)) { c->err = "k_na_narrow launch failed"; return -1; }
  passRecord(ev, 2, st);
  if (asched_internal_na_rank(&a, st)) { c->err = "k_na_rank launch failed"; return -1; }
  passRecord(ev, 3, st);
  bool ok = asched_internal_na_mask(&a, st) == 0;
  passRecord(ev, 4, st);
  return launchTail(ok, "k_na", "k_na", PASS_NA, ev);
}
// the queued lists of a round from the resident job order (kernels_queued_lists.h; k_ql_mark / k_ql_hold in armada_sched_mgpu.hip, the compaction is plat_compact,
// which brings the total back to the host: the call ends without a further wait, or, timed, with the wait for its last event).  PASS_QL (tools/probe_round_prepare_resident.py).
#include "kernels_queued_lists.h"
extern "C" int asched_internal_ql_mark(const QlArgs* a, hipStream_t s);
extern "C" int asched_internal_ql_hold(const QlArgs* a, hipStream_t s);
static int plat_queued_lists(Dev& d, const QlArgs& a, int ordTotal, int32_t* list, uint32_t* prefix, int32_t* off, int* total) {
  PlatCtx* c = t_ctx;
  hipStream_t st = c->stream;
  hipEvent_t* ev = passBegin(PASS_QL);
  passRecord(ev, 0, st);
  if (asched_internal_ql_mark(&a, st)) { c->err = "k_ql_mark launch failed"; return -1; }
  passRecord(ev, 1, st);
  if (asched_internal_ql_hold(&a, st)) { c->err = "k_ql_hold launch failed"; return -1; }
  passRecord(ev, 2, st);
  if (plat_compact(d, d.ordAll, ordTotal, a.flag, list, prefix, d.ordAllOff, a.Q, off, total)) return -1;
  passRecord(ev, 3, st);
  if (ev && !hipOk(hipEventSynchronize(ev[3]), "queued-list events")) return -1;
  passTimed(PASS_QL, ev);
  return 0;
}
// a caller-side buffer may be memory of this handle's GPU (a tensor the collective reduces in place: used directly) or host memory (staged)
static bool plat_is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice && a.device == t_ctx->device;
}
static int plat_run_fit_batch_global(Dev& d, const std::vector<int32_t>& shapes, const std::vector<int32_t>& slot, int level, GlobalKeyLayout L, const int32_t* globalRank, long long* out, int* badOut) {
  int ns = (int)shapes.size(), nq = (int)slot.size();
  bool direct = plat_is_device_ptr(out);
  int32_t *dShapes = nullptr, *dSlot = nullptr, *dRank = nullptr, *dBad = nullptr; unsigned long long* dKeys = nullptr; long long* dWords = direct ? out : nullptr;
  bool ok = hipOk(hipMalloc(&dShapes, ns * sizeof(int32_t)), "hipMalloc") && hipOk(hipMalloc(&dKeys, (size_t)ns * FIT_OSTR * sizeof(unsigned long long)), "hipMalloc") &&
            hipOk(hipMalloc(&dSlot, nq * sizeof(int32_t)), "hipMalloc") && hipOk(hipMalloc(&dBad, sizeof(int32_t)), "hipMalloc") &&
            (direct || hipOk(hipMalloc(&dWords, nq * sizeof(long long)), "hipMalloc")) && (!globalRank || hipOk(hipMalloc(&dRank, std::max(d.cfg.N, 1) * sizeof(int32_t)), "hipMalloc"));
  if (ok) {
    hipStream_t st = t_ctx->stream;
    (void)hipMemcpyAsync(dShapes, shapes.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(dSlot, slot.data(), nq * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (globalRank) (void)hipMemcpyAsync(dRank, globalRank, d.cfg.N * sizeof(int32_t), hipMemcpyHostToDevice, st);
    (void)hipMemsetAsync(dKeys, 0xff, (size_t)ns * FIT_OSTR * sizeof(unsigned long long), st);
    (void)hipMemsetAsync(dBad, 0, sizeof(int32_t), st);
    L.globalRank = dRank;
    int tiles = (d.cfg.N + FIT_TILE - 1) / FIT_TILE;
    int ysplit = std::max(1, std::min(ns, (2048 + tiles - 1) / tiles));
    (void)hipEventRecord(t_ctx->fitEv0, st);
    if (d.cfg.N > 0) hipLaunchKernelGGL(k_fit_batch, dim3(tiles, ysplit), dim3(FIT_TILE), 0, st, d, dShapes, ns, level, dKeys);
    ok = asched_internal_mgpu_pack(&d, &L, level, dKeys, dSlot, nq, dWords, dBad, st) == 0;
    (void)hipEventRecord(t_ctx->fitEv1, st);
    ok = ok && hipOk(hipGetLastError(), "fit_select_batch_global launch") && hipOk(hipStreamSynchronize(st), "fit_select_batch_global");
    (void)hipEventElapsedTime(&t_ctx->lastFitMs, t_ctx->fitEv0, t_ctx->fitEv1);
    int32_t bad = 0;
    if (ok) ok = hipOk(hipMemcpy(&bad, dBad, sizeof bad, hipMemcpyDeviceToHost), "hipMemcpy");
    if (ok && !direct) ok = hipOk(hipMemcpy(out, dWords, nq * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
    *badOut = bad;
  }
  (void)hipFree(dShapes); (void)hipFree(dKeys); (void)hipFree(dSlot); (void)hipFree(dBad); (void)hipFree(dRank); if (!direct) (void)hipFree(dWords);
  return ok ? 0 : -1;
}
static int plat_round_delta(Dev& d, int ns, int np, long long* buf) {
  size_t words = (size_t)d.cfg.N * d.cfg.R + d.cfg.M;
  bool direct = plat_is_device_ptr(buf);
  long long* dBuf = direct ? buf : nullptr;
  if (!direct && !hipOk(hipMalloc(&dBuf, std::max<size_t>(words, 1) * 8), "hipMalloc")) return -1;
  hipStream_t st = t_ctx->stream;
  bool ok = hipOk(hipMemsetAsync(dBuf, 0, words * 8, st), "hipMemsetAsync") && asched_internal_mgpu_delta(&d, dBuf, ns, np, st) == 0 && hipOk(hipStreamSynchronize(st), "round_delta");
  if (ok && !direct) ok = hipOk(hipMemcpy(buf, dBuf, words * 8, hipMemcpyDeviceToHost), "hipMemcpy");
  if (!direct) (void)hipFree(dBuf);
  return ok ? 0 : -1;
}
static int plat_delta_resolve(Dev& d, const long long* red, int ns, int np, int32_t* counts, int32_t* node, int32_t* prio, uint8_t* replay) {
  int N = d.cfg.N, M = d.cfg.M, R = d.cfg.R, G = std::max(d.cfg.G, 1);
  size_t words = (size_t)N * R + M;
  bool direct = plat_is_device_ptr(red);
  long long *dRed = nullptr, *freeC = nullptr; uint8_t* bytes = nullptr; int32_t* ints = nullptr;
  size_t nb = (size_t)M + N + G + M, ni = 4 + 2 * (size_t)M;   // ownPre | conflict | gangReplay | replay ; counts | node | prio
  bool ok = (direct || hipOk(hipMalloc(&dRed, std::max<size_t>(words, 1) * 8), "hipMalloc")) && hipOk(hipMalloc(&freeC, std::max<size_t>((size_t)N * R, 1) * 8), "hipMalloc") &&
            hipOk(hipMalloc(&bytes, nb), "hipMalloc") && hipOk(hipMalloc(&ints, ni * 4), "hipMalloc");
  if (ok) {
    hipStream_t st = t_ctx->stream;
    if (!direct) (void)hipMemcpyAsync(dRed, red, words * 8, hipMemcpyHostToDevice, st);
    (void)hipMemsetAsync(bytes, 0, nb, st); (void)hipMemsetAsync(ints, 0, 16, st);
    uint8_t *ownPre = bytes, *conflict = bytes + M, *gangReplay = conflict + N, *rp = gangReplay + G;
    ok = asched_internal_mgpu_resolve(&d, direct ? red : dRed, freeC, ownPre, conflict, gangReplay, ints + 4, ints + 4 + M, rp, ints, ns, np, st) == 0 && hipOk(hipStreamSynchronize(st), "round_delta_resolve");
    if (ok) ok = hipOk(hipMemcpy(counts, ints, 16, hipMemcpyDeviceToHost), "hipMemcpy");
    if (ok && M) ok = hipOk(hipMemcpy(node, ints + 4, (size_t)M * 4, hipMemcpyDeviceToHost), "hipMemcpy") && hipOk(hipMemcpy(prio, ints + 4 + M, (size_t)M * 4, hipMemcpyDeviceToHost), "hipMemcpy") &&
                     hipOk(hipMemcpy(replay, rp, M, hipMemcpyDeviceToHost), "hipMemcpy");
  }
  if (!direct) (void)hipFree(dRed);
  (void)hipFree(freeC); (void)hipFree(bytes); (void)hipFree(ints);
  return ok ? 0 : -1;
}
static int plat_run_drf(Dev& dev, const std::vector<int64_t>& a, const std::vector<int64_t>& t, double* out) {
  Dev d = dev;
  for (int r = 0; r < d.cfg.R; r++) d.cfg.totalResources[r] = t[r];
  int64_t* da = nullptr; double* dout = nullptr;
  (void)hipMalloc(&da, MAXR * sizeof(int64_t)); (void)hipMalloc(&dout, sizeof(double));
  (void)hipMemcpy(da, a.data(), a.size() * sizeof(int64_t), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_drf, dim3(1), dim3(64), 0, t_ctx->stream, d, da, dout);
  (void)hipStreamSynchronize(t_ctx->stream);
  (void)hipMemcpy(out, dout, sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(da); (void)hipFree(dout);
  return 0;
}
static int plat_run_fair_shares(Dev& dev, int q, const int32_t* nameRank, const double* weight, const double* cds, double* fair, double* dc, double* uc) {
  Dev d = dev;
  d.cfg.Q = q;
  size_t nb = (size_t)std::max(q, 1);
  double *dw, *df, *ddc, *duc, *dpp, *dpc, *dcds; int32_t *dnr, *dnx; uint8_t* dih;
  (void)hipMalloc(&dw, nb * 8); (void)hipMalloc(&df, nb * 8); (void)hipMalloc(&ddc, nb * 8); (void)hipMalloc(&duc, nb * 8);
  (void)hipMalloc(&dpp, nb * 8); (void)hipMalloc(&dpc, nb * 8); (void)hipMalloc(&dcds, nb * 8);
  (void)hipMalloc(&dnr, nb * 4); (void)hipMalloc(&dnx, nb * 4); (void)hipMalloc(&dih, nb);
  (void)hipMemcpy(dw, weight, q * 8, hipMemcpyHostToDevice); (void)hipMemcpy(dcds, cds, q * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(dnr, nameRank, q * 4, hipMemcpyHostToDevice);
  d.qWeight = dw; d.qNameRank = dnr; d.qFair = df; d.qDc = ddc; d.qUc = duc; d.pqProposed = dpp; d.pqCurrent = dpc; d.pqInHeap = dih; d.itNext = dnx;
  hipLaunchKernelGGL(k_fair, dim3(1), dim3(64), 0, t_ctx->stream, d, dcds);
  bool ok = hipOk(hipStreamSynchronize(t_ctx->stream), "k_fair");
  (void)hipMemcpy(fair, df, q * 8, hipMemcpyDeviceToHost); (void)hipMemcpy(dc, ddc, q * 8, hipMemcpyDeviceToHost); (void)hipMemcpy(uc, duc, q * 8, hipMemcpyDeviceToHost);
  (void)hipFree(dw); (void)hipFree(df); (void)hipFree(ddc); (void)hipFree(duc); (void)hipFree(dpp); (void)hipFree(dpc); (void)hipFree(dcds);
  (void)hipFree(dnr); (void)hipFree(dnx); (void)hipFree(dih);
  return ok ? 0 : -1;
}
