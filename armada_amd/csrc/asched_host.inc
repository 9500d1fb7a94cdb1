// asched_host.inc — host side of the C ABI (include/armada_sched.h): input marshalling (string-free static
// matching per (requirement class x node), scheduling-key shapes, pre-sorted job order, key packing), upload
// to HBM, kernel launches and result download.  All scheduling arithmetic runs in the kernels
// (round_ctl.h / round_run.h / round_kernel.h); nothing here computes a placement.
//
// Included by armada_sched.hip (the product, HIP/gfx950) and by tests/hostsim/hostsim.cpp (debug build of the
// same control code for a GPU-less container).  The platform layer (plat_*) is declared in plat.h and defined by
// the includer before this file: plat_hip.inc in the product, hostsim.cpp itself in the CPU build.

#include <algorithm>
#include <cmath>
#include <numeric>
#include <cstdio>
#include <cstring>
#include <array>
#include <climits>
#include <map>
#include <tuple>
#include <unordered_map>
#include <memory>
#include <set>
#include <string>
#include <vector>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include "kernels_fit_lit.h"   // FitLitIdx and, in the CPU build of the tests, plat_run_fit_batch_lit
#include "kernels_preempt_join.h"   // PjArgs and, in the CPU build of the tests, plat_preempt_join
#include "kernels_evict_report.h"   // EvrArgs and, in the CPU build of the tests, plat_evict_report
#include "kernels_jobs_patch.h"     // JpArgs and, in the CPU build of the tests, plat_jobs_patch
#include "kernels_jobs_reprioritise.h"   // JrArgs and, in the CPU build of the tests, plat_jobs_reprioritise
#include "kernels_round_commit.h"        // RcArgs and, in the CPU build of the tests, plat_round_commit
#include "kernels_jobs_respec.h"         // JsArgs and, in the CPU build of the tests, plat_jobs_respec
#include "kernels_jobs_append.h"    // JaArgs and, in the CPU build of the tests, plat_jobs_append
#include "kernels_shapes_append.h"  // SaArgs and, in the CPU build of the tests, plat_shapes_append
#include "kernels_req_classes_append.h"   // CaArgs and, in the CPU build of the tests, plat_req_classes_append
#include "kernels_shapes_compact.h"   // ScArgs and, in the CPU build of the tests, plat_shapes_compact
#include "kernels_jobs_delete.h"    // JdArgs and, in the CPU build of the tests, plat_jobs_delete
#include "kernels_nodes_patch.h"    // NpArgs and, in the CPU build of the tests, plat_nodes_patch
#include "kernels_nodes_delete.h"   // NdArgs and, in the CPU build of the tests, plat_nodes_delete
#include "kernels_nodes_append.h"   // NaArgs and, in the CPU build of the tests, plat_nodes_append
#include "kernels_queued_lists.h"   // QlArgs and, in the CPU build of the tests, plat_queued_lists

// plat_try_malloc (plat.h) for a platform layer that defines none of its own (PLAT_TRY_MALLOC_OWN: the CPU build of the tests, which can fail any one of them): what a
// resident call did by hand, plat_malloc with the failure it latches taken back
#ifndef PLAT_TRY_MALLOC_OWN
static void* plat_try_malloc(size_t n) { void* p = plat_malloc(n); if (!p) (void)plat_take_failure(); return p; }
#endif

namespace {

// The input build touches every job a few times (scheduling-key shapes, SchedulingOrderCompare order, one JobRec per job): the loops
// that are independent per job / per queue run on a few host threads.  ASCHED_HOST_THREADS=n overrides the count (1 = serial).
static int hostThreads() {
  static int n = [] {
    int v = (int)std::thread::hardware_concurrency();
    if (const char* e = getenv("ASCHED_HOST_THREADS")) v = atoi(e);
    return std::max(1, std::min(v, 16));
  }();
  return n;
}
// fn(begin, end) over [0, n) in `chunks` pieces handed out dynamically
template <class F> static void parallelChunks(size_t n, size_t chunks, F fn) {
  int T = hostThreads();
  chunks = std::max<size_t>(1, std::min(chunks, n));
  if (T <= 1 || chunks <= 1 || n < 4096) { fn((size_t)0, n); return; }
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (;;) {
      size_t c = next.fetch_add(1);
      if (c >= chunks) return;
      fn(n * c / chunks, n * (c + 1) / chunks);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
}

// ASCHED_HOSTPROF=1: wall time of the phases of the host-side input build (jobs_set / round_prepare) on stderr
struct HostProf {
  bool on; const char* what; std::chrono::steady_clock::time_point t0;
  explicit HostProf(const char* w) : on(getenv("ASCHED_HOSTPROF") != nullptr), what(w), t0(std::chrono::steady_clock::now()) {}
  void lap(const char* phase) {
    if (!on) return;
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[asched hostprof] %s / %s: %.1f ms\n", what, phase, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

struct HTaint { int32_t key, value, effect; };
struct HTol { int32_t key, op, value, effect; };
struct HSel { int32_t key, value; };
struct OrdKey { uint64_t a, b, t1, t2; int32_t idx; };   // packed SchedulingOrderCompare key of one job (jobs_set)
struct HAffExpr { int32_t key, op; std::vector<int32_t> values; };
struct HAffinity { bool present = false; std::vector<std::vector<HAffExpr>> terms; };
struct HType { std::vector<HTaint> taints; std::vector<HSel> labels; std::vector<int32_t> unset; int numNodes = 0; };

constexpr int32_t kUnschedulableTaintKey = -2;
constexpr int32_t kNoSuchLabelKey = INT32_MIN + 7;  // a node-selector key no node carries (interned ids are >= 0)

struct DevBufs {
  std::vector<std::pair<void*, size_t>> ptrs;
  // recycle(): blocks go to a free list keyed by their exact size instead of back to the driver — round_prepare allocates the same ~50 per-queue arrays every cycle, and
  // hipFree synchronises the device (advisor, round 4).  Every block handed out is zeroed either way.  Bounded: 256 blocks / 512 MB, larger or later ones are freed.
  std::multimap<size_t, void*> cache; size_t cacheBytes = 0;
  // a block of exactly this size from the cache, else from the driver — and when the driver has none left, the idle cached blocks go back to it first (sizes that no
  // longer occur — another Q — would otherwise sit there while the allocation fails: round-5 advisor)
  void* take(size_t bytes) {
    auto it = cache.find(bytes);
    if (it != cache.end()) { void* p = it->second; cache.erase(it); cacheBytes -= bytes; return p; }
    void* p = plat_malloc(bytes);
    if (!p && !cache.empty()) { for (auto& c : cache) plat_free(c.second); cache.clear(); cacheBytes = 0; p = plat_malloc(bytes); }
    return p;
  }
  template <class T> T* alloc(size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void* p = take(bytes);
    plat_memset(p, 0, bytes);
    ptrs.push_back({p, bytes});
    return (T*)p;
  }
  template <class T> T* allocRaw(size_t n) {   // not zeroed: large scratch arrays every element of which is written before it is read (stream keys, the bulk merge's arrays)
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void* p = take(bytes);
    ptrs.push_back({p, bytes});
    return (T*)p;
  }
  template <class T> T* upload(const std::vector<T>& v) {
    T* p = alloc<T>(v.size());
    if (!v.empty()) plat_h2d(p, v.data(), v.size() * sizeof(T));
    return p;
  }
  void recycle() {
    for (auto& b : ptrs) {
      if (b.first && cache.size() < 256 && cacheBytes + b.second <= ((size_t)512 << 20)) { cache.insert({b.second, b.first}); cacheBytes += b.second; }
      else plat_free(b.first);
    }
    ptrs.clear();
  }
  void freeAll() { for (auto& b : ptrs) plat_free(b.first); ptrs.clear(); for (auto& c : cache) plat_free(c.second); cache.clear(); cacheBytes = 0; }
  void release(void* p) {   // one block back to the driver
    for (size_t k = 0; k < ptrs.size(); k++) if (ptrs[k].first == p) { ptrs.erase(ptrs.begin() + k); break; }
    plat_free(p);
  }
};

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }   // the parts of a scratch block start at multiples of 256 bytes

// The device blocks a resident table call (asched_jobs_patch ... asched_nodes_append) replaces.  The rule they enforce: every device block the call needs is obtained
// before the first byte of the handle changes, so a call that cannot get one is refused with the handle as it was.  stage() names a block: the DevBufs that will own it,
// the pointer it replaces (a member of the handle, or a local variable of the call with keepOld), its size, the bytes to copy into it from the old block or from
// `host`, a fill byte (-1: none).  allocate() gets all of them or none.  fill() queues the fills and copies; commit() releases each old block that is not kept, swaps the
// fresh one in and registers it with its owner — the call decides when the device has been waited for; drop() is for a refusal or failure after allocate().
struct StagedBlocks {
  struct Entry { DevBufs* owner; void** slot; size_t bytes, copyBytes; const void* host; int fill; bool keepOld; void* fresh; };
  std::vector<Entry> blocks;
  void stage(DevBufs* owner, void* slot, size_t bytes, size_t copyBytes, const void* host, int fill, bool keepOld = false) {
    blocks.push_back({owner, (void**)slot, std::max<size_t>(bytes, 1), copyBytes, host, fill, keepOld, nullptr});
  }
  void stage(DevBufs* owner, void* slot, size_t bytes, int fill = 0) { stage(owner, slot, bytes, 0, nullptr, fill); }
  bool allocate() {
    for (auto& b : blocks) if (!(b.fresh = plat_try_malloc(b.bytes))) { drop(); return false; }
    return true;
  }
  void drop() { for (auto& b : blocks) { plat_free(b.fresh); b.fresh = nullptr; } }
  void* fresh(void* slot) const { for (auto& b : blocks) if ((void*)b.slot == slot) return b.fresh; return nullptr; }
  void fill() const {
    for (auto& b : blocks) {
      if (b.fill >= 0) plat_memset(b.fresh, b.fill, b.bytes);
      if (b.host) { if (b.copyBytes) plat_h2d(b.fresh, b.host, b.copyBytes); }
      else if (b.copyBytes && *b.slot) plat_d2d(b.fresh, *b.slot, b.copyBytes);
    }
  }
  void commit() {
    for (auto& b : blocks) {
      if (!b.keepOld && *b.slot) b.owner->release(*b.slot);
      *b.slot = b.fresh;
      b.owner->ptrs.push_back({b.fresh, b.bytes});
    }
  }
};

// A device block a call keeps between calls and only ever grows: its entry scratch (a quarter larger than asked for), asched_nodes_delete's keep flags (exact).
// tryGrow() asks for the larger block and changes nothing, for a call that must first know every other block can be had; adopt() releases the old block and takes the
// new one.  grow() is both, for a call with nothing else to ask for.
template <class T> struct KeptBlock {
  DevBufs& owner; T*& p; size_t& bytes;
  void* fresh = nullptr; size_t freshBytes = 0;
  bool tryGrow(size_t need, bool slack = true) {
    if (bytes >= need) return true;
    freshBytes = slack ? need + need / 4 : need;
    return (fresh = plat_try_malloc(freshBytes)) != nullptr;
  }
  void drop() { plat_free(fresh); fresh = nullptr; }
  bool adopt() {
    if (!fresh) return false;
    if (p) owner.release(p);
    p = (T*)fresh; bytes = freshBytes; owner.ptrs.push_back({fresh, freshBytes});
    fresh = nullptr;
    return true;
  }
  bool grow(size_t need) { return tryGrow(need) && (adopt(), true); }
};

}  // namespace

struct asched {
  PlatCtx* plat = nullptr;   // device ordinal, launch stream, events, mailbox, cancel word of THIS handle (plat_hip.inc)
  // ---- config
  int R = 0, K = 0, P = 0, npc = 0;
  std::vector<int32_t> indexedCol; std::vector<int64_t> indexedRes;
  std::vector<int32_t> pcPriority; std::vector<uint8_t> pcPreemptible;
  std::vector<std::vector<std::pair<int32_t, int32_t>>> pcAway;
  // AwayNodeType.NodeTypes per away entry (same indexing as pcAway) and the whole-unit size of each resource column
  struct AwayCond { int32_t resource, op; int64_t value; };
  struct AwayEntry { int32_t wkt; std::vector<AwayCond> conds; };
  std::vector<std::vector<std::vector<AwayEntry>>> pcAwayNodeTypes;
  std::vector<int64_t> resourceUnit;
  std::vector<double> drfMult, maxFraction;
  bool indexAllTaints = false;
  std::set<int32_t> indexedTaints, indexedLabels;
  std::vector<int32_t> prios;
  std::vector<uint8_t> disallowed;
  std::map<int32_t, int64_t> valueInts;  // interned label values that parse as integers (node-affinity Gt / Lt)
  std::vector<int64_t> floatingLimit;   // [R], -1 = the column is not a floating resource
  bool floatingInTotal = false;
  Dev dev;
  std::string err;
  // ---- nodes (host copies needed for static matching)
  int N = 0;
  std::vector<std::vector<HTaint>> nodeTaints; std::vector<std::vector<HSel>> nodeLabels;
  std::vector<int> nodeType; std::vector<HType> types; std::vector<int64_t> typeId;   // typeId: node_type_override of a type (-1 = derived from taints / labels)
  std::vector<int64_t> nodeTotal;  // [N][R]
  std::vector<int32_t> nodeByRank;
  bool allocAligned = true, idRankMonotone = true, hasAllocByPrio = false, allocLeTotal = true;
  bool idRanksGiven = false;   // nodes_upsert was given id ranks (without them id order == index order by definition and nodeIdRank holds the row order: asched_nodes_append)
  int64_t keyMaxV[MAXK] = {0}, keyGcdV[MAXK] = {0};    // per indexed column: the largest value any node offers, the gcd of every node value (layoutKeys: the coarser divisor)
  bool keyCoarse = false;                              // the order key's fields are quotients by a COARSER divisor than the index resolution (layoutKeys): dev.cfg.indexedRes holds it
  int64_t keyMaxQ[MAXK] = {0}, keyMinQ[MAXK] = {0};   // per indexed column: largest / smallest (value / resolution) any node offers (order-key layout, layoutKeys)
  // the experimental fairness optimiser as part of the round (asched_set_optimiser)
  struct OptCfg { bool enabled = false; double minPct = 0; int maxJobs = 0; bool hasMaxSize = false, hasMinSize = false; int64_t maxSize[MAXR] = {0}, minSize[MAXR] = {0}; std::vector<double> maxFraction; int64_t nowMs = 0; } opt;
  bool keyWide = false;                                // the wide (oversubscription-proof) field layout is in use: some request on an indexed column is negative
  DevBufs fastBufs;
  DevBufs pjBufs;                                  // lists and scratch of the preemption-cause join (kernels_preempt_join.h), kept between calls
  // ---- the evictor report of a round's phase 1 (asched_set_evictor_report; kernels_evict_report.h)
  enum EvrState { EVR_NONE = 0, EVR_VALID, EVR_MARKET, EVR_SINGLE };
  bool evrOn = false;                              // the switch
  bool evrSized = false;                           // evr's buffers fit the handle's N, M, Q, R (round_prepare, or the first round after the switch was turned on)
  int evrState = EVR_NONE;                         // what the last schedule_round left: a report, nothing (no round, a failed one), or a round that cannot have one
  DevBufs evrBufs; EvrArgs evr; void* evrZero = nullptr; size_t evrZeroBytes = 0;   // the words the passes add into are ONE block: one memset per round
  std::vector<uint8_t> nodeUnsched;                // [N] asched_nodes.unschedulable (nodeFlags bit 0 is unschedulable && overAllocated)
  std::vector<uint8_t> evrNodePre, evrNodeReasons; std::vector<int32_t> evrNodeEvicted, evrQJobs, evrQOff, evrJob, evrNode; std::vector<int64_t> evrQRes;   // the downloaded report
  double evrMs[kPassFamilies[PASS_EVR].passes] = {};                     // device ms of the three passes of the last round (ASCHED_EVR_TIMES=1; asched_round_timing)
  std::vector<int32_t> labelSlots;                 // sorted indexed label keys
  std::vector<std::vector<int32_t>> slotValues;    // per slot: sorted values present on nodes
  std::vector<int32_t> uniOffHost;
  DevBufs nodeBufs, jobBufs, queueBufs, maskBufs, exclBufs;
  int exclCap = 1024;           // asched_set_excluded_nodes: failed node selections kept per round / job table (0 = recording off)
  ExclDev exclHost;             // the device's ExclDev as uploaded (pointers, capacities)
  // ---- jobs
  int M = 0, S = 0, G = 0, C = 0;
  std::vector<int32_t> jQueue, jPc, jReqClass, jShape, jNode, jRunPrio, jGangDense;
  std::vector<uint8_t> jAway; bool anyAway = false;   // cross-pool away jobs (asched_jobs.away)
  std::vector<int64_t> jReq;
  std::vector<std::vector<HTol>> clsTol; std::vector<std::vector<HSel>> clsSel;
  std::vector<HAffinity> clsAff;  // required node affinity per requirement class (derived away classes inherit their base's)
  std::vector<int32_t> shapeClass; std::vector<int64_t> shapeReq;
  // away node types: derived requirement classes (class + tolerations of a well-known node type) live after the C real ones in
  // clsTol / clsSel; mask rows S.. of shapeMask belong to (shape, away entry of its priority class)
  std::vector<std::vector<HTaint>> wktTaints;
  std::vector<int32_t> shapePc, awayRowOff, awayRowClass, awayRowShape;
  int Cext = 0;
  std::vector<uint8_t> rowLiteral;      // per mask row: the literal iterator restatement is needed (round_ctl.h selectAtLevelLiteral)
  int32_t* dNodeType = nullptr;         // [N] node type per node on the device: the literal batched first fit sorts its index by it (kernels_fit_lit.h)
  std::vector<uint8_t> shapeUnaligned;  // per shape: some indexed request is not a multiple of its resolution
  std::vector<int32_t> nodeIdRank;
  bool jobsSet = false, nodesSet = false, prepared = false;
  // the NodeDb is "pristine": every priority plane equals allocatable (fresh upsert without alloc_by_prio, or ClearAllocated) and the
  // evicted table is empty — the state the submit checker keeps its NodeDbs in, in which node selection is a pure function of the
  // scheduling key and the individual checks of a batch can go through the wide fit kernel (asched_submit_check)
  bool allocPristine = false, evictedDirty = false;   // allocPristine: every plane is in its initial (upsert / ClearAllocated) state — no job bound, evicted or unbound since
  int equalLevels = 0;           // how many leading priority levels have planes equal to level 0's in that state (P without an alloc_by_prio table: every plane == allocatable)
  int Q = 0;
  // ---- results
  // the round's result arrays live in ONE pinned host arena (downloadResult): every piece is copied asynchronously on the handle's stream and the host waits once
  // (round 4: eleven staged copies through pageable vectors, ~35 us each — a third of a small round, profiles/r05g_small_round_timeline.txt)
  void* resPin = nullptr; size_t resPinBytes = 0; int resNs = 0, resNp = 0;
  const int32_t *resSJob = nullptr, *resSNode = nullptr, *resSPrio = nullptr, *resPJob = nullptr;   // the last round's lists in resPin (downloadResult), read by asched_round_commit
  RoundScalars rsHost;
  double roundMs = 0; int roundLaunches = 0;
  double submitMs = 0;
  // market-driven rounds (asched_set_market; round_mkt.h)
  struct { bool enabled = false; double spotCutoff = 0.0; } market;
  bool mkJobsBuilt = false;     // the job set carries the market order (jobs_set saw bid prices or market mode)
  std::vector<int32_t> jGangUniKey;   // [M] uniformity label key of a gang member, -1
  MktDev mk{};                  // device arrays of the market round (dev.h MktDev): passed to the auxiliary kernel as its own argument, not part of Dev
  std::vector<int64_t> resBillable; std::vector<double> resOverride; std::vector<uint8_t> resHasOverride;
  uint64_t stateEpoch = 1, optIndexEpoch = 0;   // stateEpoch: bumped by everything that can change which job sits on which node (control launches, round phases, uploads); the optimiser's
                                                // node -> jobs index is rebuilt when it is older
  bool argsOverflow = false;     // the last setArgs did not fit the command mailbox: runControl refuses the command
  long long* commStatus = nullptr;   // one device word: the status all-reduce in front of every collective (collectiveAgree)
  struct { bool valid = false; EvKey* key = nullptr; QsIn* in = nullptr; int64_t* part = nullptr; int32_t* len = nullptr; QsSave* save = nullptr; } qsOrig;   // the QCAPF-sized stream buffers of jobs_set while a wide round uses Q-sized ones
  bool roundExchanged = false;   // round_exchange resolved the last round against the other replicas: the per-job preemption record is not the resolved round's
  bool haveRoundResult = false;  // d.resJob / resNode / resPreJob hold the last round's lists (round_delta reads them on the device)
  bool lastWideWasOpt = false;   // kernel_times out[1] reports the optimiser's k_opt_score instead of k_fit_batch
  // host staging reused across jobs_set calls (a fresh 200 MB / 60 MB allocation costs more in first-touch page faults than the fill)
  std::unique_ptr<unsigned char[]> stageRecs; size_t stageRecsBytes = 0;
  std::vector<OrdKey> stageKeys;
  int ordQueues = 0;   // number of queue segments in the pre-sorted job order (max queue index of the job table + 1)
  std::vector<int32_t> ordOffHost;   // host copy of dev.ordAllOff (segment offsets of the pre-sorted order)
  // ---- asched_jobs_patch (kernels_jobs_patch.h).  jobs_set keeps the order-key inputs only the host sees (queue priority, submit time, run timestamp) as host copies;
  // the first patch of a job table uploads them and allocates the keep flags and the second order buffer (all in jobBufs: gone with the job table)
  std::vector<uint32_t> jQPrioHost; std::vector<int64_t> jSubmitHost, jRunTsHost;
  struct { bool built = false; uint8_t* keep = nullptr; uint32_t* qprio = nullptr; int64_t* submit = nullptr; int64_t* runTs = nullptr; int32_t* ordSpare = nullptr; } jp;
  std::vector<uint8_t> jpSeen;       // [M] all zero between calls: a row named twice in one patch
  // ---- asched_jobs_append (kernels_jobs_append.h).  Capacities of the job table's device arrays, in elements: jobs_set allocates exactly what the table needs (capacity ==
  // size); an append that does not fit grows to max(needed, 1.25 x capacity).  ordCap / ordSpareCap: dev.ordAll and jp.ordSpare (they swap).
  size_t jobCap = 0, gangCap = 0, gangArrCap = 0, gangJobsCap = 0, gangOffCap = 0, ordCap = 0, ordSpareCap = 0, ordOffCap = 0;
  std::map<std::pair<int32_t, int32_t>, int32_t> gangMap;   // (queue, gang id) -> dense gang id, as jobs_set numbered them
  std::vector<int32_t> gangOffHost;  // host copy of dev.gangOff [G + 2]
  std::vector<int32_t> shapeRow;     // [S] first row of each scheduling-key shape (a new row's JobRec is copied from it on the device)
  std::vector<int32_t> shapeTable; std::vector<uint64_t> shapeHash;   // open-addressing table over the shapes, built by the first append of a job table
  int32_t jaStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_jobs_append_stats
  // ---- the in-place path of asched_jobs_append for new shapes (asched_set_append_in_place; kernels_shapes_append.h).  What buildFast derives per scheduling-key shape
  // stays on the handle (host only), so that an append can extend it: key delta / smallest key fields / "fits nowhere" per shape, the fit-shape ids in order of first
  // occurrence with their table, and the two minima before they are packed (INT64_MAX: no shape yet)
  bool appendInPlace = false;        // the switch: a property of the handle, survives jobs_set and nodes_upsert
  int32_t jasStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_jobs_append_shape_stats
  double saMs[kPassFamilies[PASS_SA].passes] = {};           // device ms of the new mask rows / the row copies of the last in-place append (ASCHED_JA_TIMES=1)
  std::vector<uint64_t> fsDelta, fsMin; std::vector<uint8_t> fsNever; std::vector<int32_t> fitOf; std::vector<ShapeReq> fitTab;
  std::map<std::tuple<uint64_t, uint64_t, int64_t, int64_t, int32_t, int32_t>, int32_t> fitIds;
  int64_t fsMinField[MAXK] = {0}, fsMinExtra[MAXE] = {0};
  // ---- asched_req_classes_append (kernels_req_classes_append.h): new requirement classes behind the C resident ones
  int32_t caStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_req_classes_append_stats
  double caMs[kPassFamilies[PASS_CA].passes] = {}, caHostMs[2] = {0, 0};   // device ms of the new rows / the row copies; host ms of the taint scan / the tier-2 rows of the last call (ASCHED_CA_TIMES=1)
  // ---- asched_shapes_compact (kernels_shapes_compact.h): dead shapes, fit shapes and requirement classes leave the resident tables
  int32_t scStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_shapes_compact_stats
  double scMs[kPassFamilies[PASS_SC].passes] = {}, scHostMs = 0;        // device ms of rows / gathers / class bits, host ms of the mirror remap of the last call (ASCHED_SC_TIMES=1)
  double jaMs[kPassFamilies[PASS_JA].passes] = {};        // device ms of row fill / sort / merge of the last append (ASCHED_JA_TIMES=1)
  DevBufs jpBufs; char* jpScratch = nullptr; size_t jpScratchBytes = 0;   // the entries, the sort array and the kept list of a patch: one block, kept between calls and only ever grown
  double jpMs[kPassFamilies[PASS_JP].passes] = {};     // device ms of the four passes of the last patch (ASCHED_JP_TIMES=1)
  int32_t jrStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_jobs_reprioritise_stats (kernels_jobs_reprioritise.h)
  int32_t rcStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_round_commit_stats (kernels_round_commit.h)
  int32_t jsStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_jobs_respec_stats (kernels_jobs_respec.h)
  // ---- asched_jobs_delete (kernels_jobs_delete.h).  A scheduling-key shape that lost its last row keeps its id with shapeRow[s] == -1 (an append that uses it goes
  // through the rebuild path); a gang that lost its last row keeps its dense id with no members and leaves gangMap
  int32_t jdStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_jobs_delete_stats
  double jdMs[kPassFamilies[PASS_JD].passes] = {};  // device ms of mark / scan / gather / order / gang lists of the last delete (ASCHED_JD_TIMES=1)
  double jdHostMs = 0;               // wall ms of the host's compaction of its mirrors in the last delete
  // ---- asched_nodes_patch (kernels_nodes_patch.h).  What nodes_upsert was given and no other mirror holds (index, allocatable, over_allocated: N x (9 + 8R) bytes;
  // total, id_rank, unschedulable, taints and labels are nodeTotal, nodeIdRank, nodeUnsched, nodeTaints and nodeLabels above): the rebuild path of a patch runs
  // nodes_upsert's own code on the patched table.  typeByCanon: canonical string of a node type -> position in `types`
  std::vector<uint64_t> nodeIndexHost; std::vector<int64_t> nodeAllocHost; std::vector<uint8_t> nodeOverAlloc;
  std::unordered_map<std::string, int> typeByCanon;
  bool hasTypeOverride = false, uploadedAllocByPrio = false;   // the table came with node_type_override / alloc_by_prio: asched_nodes_patch refuses it
  uint64_t* dClassMask = nullptr; int32_t* dShapeClass = nullptr;   // [Cext][W], [Sext] in maskBufs (rebuildMasks): the resident class mask and the class of every mask row
  std::vector<uint8_t> npSeen;       // [N] all zero between calls: a node named twice in one patch
  DevBufs npBufs; char* npScratch = nullptr; size_t npScratchBytes = 0;   // the entries of a patch: one block, kept between calls and only ever grown
  int32_t npStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_nodes_patch_stats
  double npMs[kPassFamilies[PASS_NP].passes] = {};           // device ms of scatter / mask words of the last patch (ASCHED_NP_TIMES=1)
  // ---- asched_nodes_delete (kernels_nodes_delete.h).  slotValueCount: nodes that carry slotValues[s][k] — a value that loses its last node takes the rebuild path, as a
  // node type that loses its last node does (types[].numNodes).  The keep flags are a block of their own, all 1 between calls; the rest of the scratch is kept and only grown
  std::vector<std::vector<int32_t>> slotValueCount;
  DevBufs ndBufs; uint8_t* ndKeep = nullptr; size_t ndKeepCap = 0; char* ndScratch = nullptr; size_t ndScratchBytes = 0;
  std::vector<int32_t> ndMap;        // [N] the old -> new map of the last delete on the host (the remap of the jNode mirror)
  int32_t ndStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_nodes_delete_stats
  double ndMs[kPassFamilies[PASS_ND].passes] = {};   // device ms of the passes of the last delete (ASCHED_ND_TIMES=1)
  // ---- asched_nodes_append (kernels_nodes_append.h).  The entries of an append: one block, kept between calls and only ever grown
  DevBufs naBufs; char* naScratch = nullptr; size_t naScratchBytes = 0;
  int32_t naStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // asched_nodes_append_stats
  double naMs[kPassFamilies[PASS_NA].passes] = {};     // device ms of planes / narrow arrays / index order / mask rows of the last append (ASCHED_NA_TIMES=1)
  // ---- asched_round_prepare_resident (kernels_queued_lists.h).  The flag bytes, the prefix words, the lists and their offsets belong to the handle: sized from the
  // capacities of the job table (jobCap rows, ordCap order entries), kept across rounds and only ever grown; the held rows of a call in a block of their own
  struct { DevBufs bufs; uint8_t* flag = nullptr; uint32_t* prefix = nullptr; int32_t* list = nullptr; int32_t* off = nullptr; size_t rowCap = 0, ordCap = 0;
           DevBufs heldBufs; int32_t* held = nullptr; size_t heldCap = 0; } ql;
  double qlMs[kPassFamilies[PASS_QL].passes] = {};        // device ms of mark / hold / compact of the last round_prepare_resident (ASCHED_QL_TIMES=1)
  bool queuedValid = false; int queuedTotal = 0;   // dev.queuedOff / dev.queuedJobs are what the last round_prepare / round_prepare_resident left (asched_round_queued)
  double roundTotalMs = 0, roundControlMs = 0, roundPhaseMs[4] = {0, 0, 0, 0};   // split round: whole sequence / persistent passes / evict-1, evict-3, final bulk phases (host clock)
  int submitWideUnits = 0, submitWidePasses = 0, submitSeqUnits = 0, submitGangUnits = 0, submitNodePasses = 0, submitLitUnits = 0;   // how the last submit_check ran (submit_stats)
};

namespace {

int fail(asched* h, int code, const std::string& msg) { h->err = msg; return code; }

int runControl(asched* h, int cmd) {
  if (h->argsOverflow) { h->argsOverflow = false; return fail(h, ASCHED_ERR_UNSUPPORTED, "command arguments exceed the device mailbox (a gang / victim list of more than 131 088 words)"); }
  h->stateEpoch++;
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());   // an upload / allocation since the last launch failed (ADVICE r1: no silent HIP errors)
  int rc = plat_run_control(h->dev, cmd);
  if (rc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  plat_d2h(&h->rsHost, h->dev.rs, sizeof(RoundScalars));
  if (h->rsHost.error) {
    int e = h->rsHost.error;
    char buf[128]; snprintf(buf, sizeof buf, "device raised error %d (detail %d)", e, h->rsHost.errorDetail);
    int32_t zero[2] = {0, 0};
    plat_h2d(&h->dev.rs->error, zero, sizeof zero);
    if (e == ASCHED_ERR_TIMEOUT) { h->prepared = false; return fail(h, e, "scheduling round cancelled: hard timeout / context done (queue_scheduler.go:105-112); no result, round_prepare again"); }
    return fail(h, e, buf);
  }
  return 0;
}

// the command mailbox holds CMDIO_ARG_WORDS argument words behind its 16 header words (asched_create sizes it); a variable-length command (a gang's members, the victims of an
// optimiser placement) that does not fit is refused, never written past the buffer: the flag makes the next runControl fail with ASCHED_ERR_UNSUPPORTED
#define CMDIO_ARG_WORDS (2 * 65536 + 16)
void setArgs(asched* h, const std::vector<int32_t>& a) {
  if (a.size() > (size_t)CMDIO_ARG_WORDS) { h->argsOverflow = true; return; }
  plat_h2d(h->dev.cmdIO + 16, a.data(), a.size() * sizeof(int32_t));
}
void getIO(asched* h, int32_t* out, int n) { plat_d2h(out, h->dev.cmdIO, n * sizeof(int32_t)); }

bool tolerates(const HTol& t, const HTaint& x) {  // k8s Toleration.ToleratesTaint (SURVEY A.8)
  if (t.effect != 0 && t.effect != x.effect) return false;
  if (t.key != -1 && t.key != x.key) return false;
  if (t.op == ASCHED_TOLERATION_OP_EXISTS) return true;
  return t.value == x.value;
}

// StaticJobRequirementsMet without the resource check (nodematching.go:161-183), per requirement class
bool classMatchesNode(asched* h, int cls, int n) {
  for (auto& x : h->nodeTaints[n]) {
    bool ok = false;
    for (auto& t : h->clsTol[cls]) if (tolerates(t, x)) { ok = true; break; }
    if (!ok) return false;
  }
  for (auto& s : h->clsSel[cls]) {
    bool found = false;
    for (auto& l : h->nodeLabels[n]) if (l.key == s.key) { found = true; if (l.value != s.value) return false; }
    if (!found) return false;
  }
  // NodeAffinityRequirementsMet (nodematching.go:242-255) -> component-helpers nodeaffinity: any term matches; a term matches when it
  // has expressions and all of them hold; NotIn / DoesNotExist accept a missing label
  if (cls < (int)h->clsAff.size() && h->clsAff[cls].present) {
    bool any = false;
    for (auto& term : h->clsAff[cls].terms) {
      if (term.empty()) continue;
      bool all = true;
      for (auto& x : term) {
        bool has = false; int32_t val = 0;
        for (auto& l : h->nodeLabels[n]) if (l.key == x.key) { has = true; val = l.value; }
        bool in = has && std::find(x.values.begin(), x.values.end(), val) != x.values.end();
        bool ok;
        if (x.op == ASCHED_AFFINITY_OP_GT || x.op == ASCHED_AFFINITY_OP_LT) {
          // labels.Requirement.Matches: the label must exist and parse, there must be exactly one requirement value and it must parse
          auto lv = has ? h->valueInts.find(val) : h->valueInts.end();
          auto rv = x.values.size() == 1 ? h->valueInts.find(x.values[0]) : h->valueInts.end();
          ok = lv != h->valueInts.end() && rv != h->valueInts.end() && (x.op == ASCHED_AFFINITY_OP_GT ? lv->second > rv->second : lv->second < rv->second);
        } else ok = x.op == ASCHED_AFFINITY_OP_IN ? in : x.op == ASCHED_AFFINITY_OP_NOT_IN ? !in : x.op == ASCHED_AFFINITY_OP_EXISTS ? has : !has;
        if (!ok) { all = false; break; }
      }
      if (all) { any = true; break; }
    }
    if (!any) return false;
  }
  return true;
}
// NodeTypeJobRequirementsMet (nodematching.go:127-139)
bool classMatchesType(asched* h, int cls, const HType& t) {
  for (auto& x : t.taints) {
    bool ok = false;
    for (auto& tol : h->clsTol[cls]) if (tolerates(tol, x)) { ok = true; break; }
    if (!ok) return false;
  }
  for (auto& s : h->clsSel[cls]) {
    bool found = false;
    for (auto& l : t.labels) if (l.key == s.key) { found = true; if (l.value != s.value) return false; }
    if (!found) for (auto k : t.unset) if (k == s.key) return false;
  }
  return true;
}

int buildFast(asched* h, const std::vector<uint64_t>& classMask);
int bitsFor(uint64_t range);
int buildRowTables(asched* h, const std::vector<int32_t>& shapeClassExt, std::vector<int32_t>& rowTypeOff, std::vector<int32_t>& rowTypes);

// ---- NumExcludedNodesByReason (asched_excluded_nodes).  The device records what depends on the round's state (dev.h ExclDev); the reasons that are functions of the inputs
// alone are worked out here, when asked: the checks of classMatchesType / classMatchesNode above, returning WHAT failed (nodematching.go:199-267).  Where the reference is
// order-dependent — a node selector is a Go map — the smallest label key is reported (include/armada_sched.h).
struct ExclKeyH { int32_t kind = 0, a = 0, b = 0, c = 0; int64_t required = 0, available = 0;
  bool operator<(const ExclKeyH& o) const { return std::tie(kind, a, b, c, required, available) < std::tie(o.kind, o.a, o.b, o.c, o.required, o.available); } };
static bool exclTaint(asched* h, int cls, const std::vector<HTaint>& taints, ExclKeyH* k) {   // FindMatchingUntoleratedTaint (taint.go:44-58): the first in the list's order
  for (auto& x : taints) {
    bool ok = false;
    for (auto& t : h->clsTol[cls]) if (tolerates(t, x)) { ok = true; break; }
    if (!ok) { k->kind = ASCHED_EXCL_UNTOLERATED_TAINT; k->a = x.key; k->b = x.value; k->c = x.effect; return true; }
  }
  return false;
}
static bool exclSelectors(std::vector<HSel> sels, const std::vector<HSel>& labels, const std::vector<int32_t>* unset, ExclKeyH* k) {   // NodeSelectorRequirementsMet (:216-243)
  std::sort(sels.begin(), sels.end(), [](const HSel& a, const HSel& b) { return a.key < b.key; });
  for (auto& s : sels) {
    bool found = false;
    for (auto& l : labels) if (l.key == s.key) {
      found = true;
      if (l.value != s.value) { k->kind = ASCHED_EXCL_UNMATCHED_LABEL; k->a = s.key; k->b = s.value; k->c = l.value; return true; }
    }
    if (!found) {
      bool missing = !unset;
      if (unset) for (auto u : *unset) if (u == s.key) missing = true;
      if (missing) { k->kind = ASCHED_EXCL_MISSING_LABEL; k->a = s.key; return true; }
    }
  }
  return false;
}
// the device's record store: sized by the node and job tables, rebuilt with the masks
static void exclSetup(asched* h) {
  h->exclBufs.freeAll();
  h->dev.excl = nullptr;
  memset(&h->exclHost, 0, sizeof h->exclHost);
  if (h->exclCap <= 0 || h->M <= 0 || h->N <= 0) return;
  ExclDev& x = h->exclHost;
  x.cap = h->exclCap; x.W = h->dev.cfg.W;
  x.dynCap = (int32_t)std::min<long long>((long long)1 << 20, std::max<long long>(4096, 4ll * h->N));
  const size_t jcap = std::max((size_t)h->M, h->jobCap);   // (room for the rows asched_jobs_append may still add: the job table's capacity)
  char* base = h->exclBufs.alloc<char>(EXCL_HDR + jcap * 4);   // the header, then the per-job slots (dev.h EXCL())
  x.jobSlot = (int32_t*)(base + EXCL_HDR);
  plat_memset(x.jobSlot, 0xff, jcap * 4);
  x.rec = h->exclBufs.alloc<ExclRec>(x.cap);
  x.bits = h->exclBufs.alloc<uint64_t>((size_t)x.cap * x.W);
  x.fbits = (h->dev.cfg.disableUrgency && !h->dev.cfg.disableFair) ? h->exclBufs.alloc<uint64_t>((size_t)x.cap * x.W) : x.bits;   // (gate-passed records exist only with urgency preemption disabled; never read otherwise)
  x.dyn = h->exclBufs.alloc<ExclDyn>(x.dynCap);
  x.pinAvail = h->exclBufs.alloc<int64_t>(jcap);
  static_assert(sizeof(ExclDev) <= EXCL_HDR, "ExclDev header");
  plat_h2d(base, &x, sizeof x);
  h->dev.excl = x.jobSlot;
}

// Layout of the packed order key (dev.h keys; encoding.go:37-54 as one integer compare): field_c = clamp(alloc_c / res_c, -1 ..) + 1 in width_c bits per
// indexed column, the node-index rank in the low bits.  Requests are non-negative, so a node whose column is negative at some level fits nothing there and
// its position among the other such nodes is never observed: every negative quotient shares field value 0 ("does not fit"), which keeps a field as wide
// as allocatable needs instead of (P + 2) times that for the oversubscription urgency preemption can cause — the reference's default indexedResources
// (config/scheduler/config.yaml:121-129) on 64-cpu / 1 TiB / 4 TiB-ephemeral / 8-gpu nodes pack into 58 bits at 100 000 nodes.  Keys are recomputed from
// the planes (round_ctl.h packKey clamps) wherever a column may be negative; the packed subtraction of a bind is only used where it cannot borrow (a job that
// fits at priority -2 fits at every level; an evicted job returning while no priority -2 column is negative), else a per-field saturating one (keySatSub).
// The wide layout of rounds 1-2 (lo = minq - (P + 1)(maxq + 1): every quotient urgency preemption can produce has its own field value) is kept where the
// order among such nodes CAN be observed and the key has room for it: a job table with a negative request on an indexed column (it is required then), and
// mask rows on the literal iterator path (round_ctl.h selectAtLevelLiteral: a deficient node met earlier or later moves a seek; wide when it fits).
int layoutKeys(asched* h) {
  Dev& d = h->dev;
  int K = h->K, N = h->N, P = h->P;
  bool negReq = false, anyLiteral = false;
  if (h->jobsSet) {
    for (size_t j = 0; j < (size_t)h->M && !negReq; j++) for (int c = 0; c < K; c++) if (h->jReq[j * h->R + h->indexedCol[c]] < 0) { negReq = true; break; }
    for (uint8_t u : h->shapeUnaligned) anyLiteral = anyLiteral || u;
    if (h->types.size() > 1 && !(h->allocAligned && h->idRankMonotone)) anyLiteral = true;   // (conservative: rebuildMasks decides per requirement class)
  }
  int idxBits = bitsFor(N > 1 ? (uint64_t)(N - 1) : 1);
  auto fieldsFor = [&](bool wide, int* widths, int64_t* los) {
    int total = idxBits;
    for (int c = 0; c < K; c++) {
      int64_t maxq = h->keyMaxQ[c], minq = h->keyMinQ[c];
      los[c] = wide ? std::min<int64_t>(minq, 0) - (int64_t)(P + 1) * (maxq + 1) : -1;  // wide: oversubscription by urgency preemption is bounded by P x allocatable
      widths[c] = bitsFor((uint64_t)(maxq + 1 - los[c]));
      total += widths[c];
    }
    return total;
  };
  int widths[MAXK]; int64_t los[MAXK];
  bool wideFits = fieldsFor(true, widths, los) <= 64;
  h->keyWide = negReq || (anyLiteral && wideFits);
  if (const char* e = getenv("ASCHED_KEY_LAYOUT")) { if (e[0] == 'w' && wideFits) h->keyWide = true; if (e[0] == 'n' && !negReq) h->keyWide = false; }   // A/B and tests: "wide" / "narrow"
  int totalBits = fieldsFor(h->keyWide, widths, los);
  d.cfg.keyClamp = h->keyWide ? 0 : 1;
  d.cfg.idxBits = idxBits;
  for (int c = 0; c < K; c++) { d.cfg.keyLo[c] = los[c]; d.cfg.keyWidth[c] = widths[c]; }
  // A COARSER DIVISOR before a second word.  The key orders nodes by (floor(alloc_c / res_c))_c.  Let g_c be the gcd of everything that can ever be added to or taken from
  // column c of a node — every node's allocatable there and every job's request (running and queued) — so every value the column can take is a multiple of g_c.  If g_c is a
  // multiple of res_c, v -> v / g_c and v -> floor(v / res_c) are both strictly increasing on those values: two nodes compare the same under either, column by column, so the
  // merged iterator order is the same and a field can hold v / g_c — exact, log2(g_c / res_c) bits narrower.  (cpu @1m with requests in quarter cores: 8 bits; memory @1Mi with
  // requests and nodes in 32Mi units: 5.)  Taken only where one word would otherwise not do, where no row iterates literally (those functions reason in res_c) and no request
  // or initial plane is negative; the handle's dev.cfg.indexedRes then holds g_c (packKey, buildFast and the gang units divide by it), h->indexedRes the reference's res_c.
  // ASCHED_KEY_GCD=1 takes it wherever it applies (soaks: the whole fast path on scaled fields), =0 never.
  {
    for (int c = 0; c < K; c++) d.cfg.indexedRes[c] = h->indexedRes[c];
    h->keyCoarse = false;
    const char* ge = getenv("ASCHED_KEY_GCD");
    // (also where the fields fit but their guard bits do not — totalBits + K > 64: without guard bits the split node engine is off, engine_hc.h)
    bool want = (totalBits + K > 64 || (ge && ge[0] == '1')) && !(ge && ge[0] == '0') && !getenv("ASCHED_KEY_WORDS");
    if (want && h->jobsSet && !anyLiteral && !negReq && !h->keyWide && !h->hasAllocByPrio) {
      int64_t eff[MAXK]; bool any = false;
      for (int c = 0; c < K; c++) {
        int64_t g = h->keyGcdV[c];
        const int col = h->indexedCol[c];
        for (size_t j = 0; j < (size_t)h->M && g != 1; j++) g = std::gcd(g, h->jReq[j * h->R + col]);
        eff[c] = (g > h->indexedRes[c] && g % h->indexedRes[c] == 0) ? g : h->indexedRes[c];
        any = any || eff[c] != h->indexedRes[c];
      }
      if (any) {
        int w2[MAXK]; int total2 = idxBits;
        for (int c = 0; c < K; c++) { w2[c] = bitsFor((uint64_t)(h->keyMaxV[c] / eff[c] + 1 - (-1))); total2 += w2[c]; }
        if (total2 <= 64 && total2 < totalBits) {
          for (int c = 0; c < K; c++) { d.cfg.indexedRes[c] = eff[c]; widths[c] = w2[c]; d.cfg.keyWidth[c] = w2[c]; }
          totalBits = total2; h->keyCoarse = true;
          if (getenv("ASCHED_PRINT_LAYOUT")) { fprintf(stderr, "[asched layout] coarser key divisors:"); for (int c = 0; c < K; c++) fprintf(stderr, " %lld (res %lld, %d bits)", (long long)eff[c], (long long)h->indexedRes[c], w2[c]); fprintf(stderr, " -> %d bits\n", total2); }
        }
      }
    }
  }
  // TWO-WORD keys (dev.h keyWords; the reference's key is one 8-byte word per indexed resource, encoding.go:22-54): when the fields need more than 64 bits the key is ONE
  // 128-bit integer with the same field order (round_ctl.h packKey2), stored as two words.  Such a handle is served by the generic path of the round kernel built for it
  // (armada_sched_wk.hip).  ASCHED_KEY_WORDS=2 forces the layout where one word would do, with the fields moved up so that they lie across the word boundary (tests, soaks).
  bool two = totalBits > 64;
  int forced = 0;
  if (const char* e = getenv("ASCHED_KEY_WORDS")) if (e[0] == '2' && K >= 1) { two = true; forced = 1; }
  if (two) {
    int shift = idxBits;
    if (forced && totalBits <= 64) shift = std::max(idxBits, 64 - (totalBits - idxBits) / 2);   // (the bits between the rank and the first field are zero in every key: the order is the same)
    for (int c = K - 1; c >= 0; c--) { d.cfg.keyShift[c] = shift; shift += widths[c]; }
    if (shift > 128) return fail(h, ASCHED_ERR_UNSUPPORTED, "packed order key needs more than 128 bits for these resolutions / capacities / node count");
    d.cfg.keyGuard = 0; d.cfg.keyWords = 2;
    return 0;
  }
  d.cfg.keyWords = 1;
  int shift = idxBits;
  // a spare zero bit above every field when the key has room: order unchanged, and a per-field >= becomes one subtraction (FastCfg.guardMask)
  d.cfg.keyGuard = totalBits + K <= 64 ? 1 : 0;
  if (const char* e = getenv("ASCHED_NO_KEY_GUARD")) if (e[0] == '1') d.cfg.keyGuard = 0;
  for (int c = K - 1; c >= 0; c--) {
    d.cfg.keyShift[c] = shift;
    shift += widths[c] + d.cfg.keyGuard;
  }
  return 0;
}

// the per-row tables of the shape mask's rows (the S shape rows, then the away rows; shapeClassExt: the class of each): which rows take the literal iterator restatement
// (h->rowLiteral) and the populated node types each row's class matches.  rebuildMasks, and the in-place path of asched_jobs_append over the grown shape table: an old
// row's entries depend on its class, its shape and the node table only, so they come out as they were.
int buildRowTables(asched* h, const std::vector<int32_t>& shapeClassExt, std::vector<int32_t>& rowTypeOff, std::vector<int32_t>& rowTypes) {
  const int Sext = h->S + (int)h->awayRowClass.size();
  // Exactness of the packed-key argmin: (A) the request is a multiple of the index resolution on every indexed column (else the
  // skip-scan can jump over fitting nodes), (B) a requirement class that matches more than one populated node type needs
  // resolution-aligned allocatable and id order == index order (else the heap merge is not the key order; SURVEY hard part 2).
  // Mask rows that violate either take the literal iterator restatement on the device (slower, exact).
  std::vector<std::vector<int32_t>> clsTypes(h->Cext);
  std::vector<uint8_t> clsLiteral(h->Cext, 0);
  for (int c = 0; c < h->Cext; c++) {
    for (size_t t = 0; t < h->types.size(); t++) if (h->types[t].numNodes > 0 && classMatchesType(h, c, h->types[t])) clsTypes[c].push_back((int32_t)t);
    if (clsTypes[c].size() > 1 && !(h->allocAligned && h->idRankMonotone)) clsLiteral[c] = 1;
  }
  h->rowLiteral.assign(std::max(Sext, 1), 0);
  rowTypeOff.assign(Sext + 1, 0); rowTypes.clear();
  for (int row = 0; row < Sext; row++) {
    int shape = row < h->S ? row : h->awayRowShape[row - h->S];
    int cls = shapeClassExt[row];
    rowTypeOff[row] = (int32_t)rowTypes.size();
    rowTypes.insert(rowTypes.end(), clsTypes[cls].begin(), clsTypes[cls].end());
    h->rowLiteral[row] = h->shapeUnaligned[shape] || clsLiteral[cls];
#ifdef ASCHED_HOSTSIM
    if (getenv("HOSTSIM_NO_LITERAL")) h->rowLiteral[row] = 0;  // negative control for the tests: the packed-key argmin is NOT exact for these rows
#endif
    if (h->rowLiteral[row] && clsTypes[cls].size() > LIT_TMAX)
      return fail(h, ASCHED_ERR_UNSUPPORTED, "a requirement class on the literal iteration path matches more than LIT_TMAX node types");
  }
  rowTypeOff[Sext] = (int32_t)rowTypes.size();
  return 0;
}

// (re)build the per-shape node masks once both nodes and jobs are known
int rebuildMasks(asched* h) {
  if (!h->nodesSet || !h->jobsSet) return 0;
  h->maskBufs.freeAll();
  h->dClassMask = nullptr; h->dShapeClass = nullptr;
  Dev& d = h->dev;
  int W = d.cfg.W;
  std::vector<uint64_t> classMask((size_t)h->Cext * W, 0);
  for (int c = 0; c < h->Cext; c++)
    for (int n = 0; n < h->N; n++)
      if (classMatchesNode(h, c, n)) classMask[(size_t)c * W + (n >> 6)] |= 1ull << (n & 63);
  uint64_t* dClassMask = h->dClassMask = h->maskBufs.upload(classMask);   // (kept: asched_nodes_patch rewrites the words of patched nodes)
  int Sext = h->S + (int)h->awayRowClass.size();
  d.shapeMask = h->maskBufs.alloc<uint64_t>((size_t)std::max(Sext, 1) * W);
  std::vector<int32_t> shapeClassExt = h->shapeClass;
  std::vector<int64_t> shapeReqExt = h->shapeReq;
  for (size_t k = 0; k < h->awayRowClass.size(); k++) {
    shapeClassExt.push_back(h->awayRowClass[k]);
    for (int r = 0; r < h->R; r++) shapeReqExt.push_back(h->shapeReq[(size_t)h->awayRowShape[k] * h->R + r]);
  }
  int32_t* dShapeClass = h->dShapeClass = h->maskBufs.upload(shapeClassExt);
  d.shapeReq = h->maskBufs.upload(shapeReqExt);
  d.awayRowOff = h->maskBufs.upload(h->awayRowOff);
  {
    std::vector<int32_t> rowTypeOff, rowTypes;
    if (int rc = buildRowTables(h, shapeClassExt, rowTypeOff, rowTypes)) return rc;
    std::vector<uint64_t> typeMask(std::max<size_t>(h->types.size(), 1) * W, 0);
    for (int n = 0; n < h->N; n++) typeMask[(size_t)h->nodeType[n] * W + (n >> 6)] |= 1ull << (n & 63);
    d.rowLiteral = h->maskBufs.upload(h->rowLiteral);
    d.rowTypeOff = h->maskBufs.upload(rowTypeOff);
    d.rowTypes = h->maskBufs.upload(rowTypes);
    d.typeMask = h->maskBufs.upload(typeMask);
    h->dNodeType = h->maskBufs.upload(std::vector<int32_t>(h->nodeType.begin(), h->nodeType.end()));
  }
  // uniformity label masks
  std::vector<uint64_t> labelMask;
  h->uniOffHost.assign(1, 0);
  for (size_t s = 0; s < h->labelSlots.size(); s++) {
    for (int32_t v : h->slotValues[s]) {
      size_t base = labelMask.size();
      labelMask.resize(base + W, 0);
      for (int n = 0; n < h->N; n++)
        for (auto& l : h->nodeLabels[n]) if (l.key == h->labelSlots[s] && l.value == v) labelMask[base + (n >> 6)] |= 1ull << (n & 63);
    }
    h->uniOffHost.push_back((int32_t)(labelMask.size() / W));
  }
  d.labelMask = h->maskBufs.upload(labelMask);
  d.uniOff = h->maskBufs.upload(h->uniOffHost);
  exclSetup(h);
  int rc;
  { Dev dm = d; dm.cfg.S = Sext; rc = plat_run_shape_mask(dm, dClassMask, dShapeClass); }  // all rows, away rows included
  if (rc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return buildFast(h, classMask);
}

// What the fast structure holds per scheduling-key shape `s` (the next one: s == h->fsDelta.size()), from the handle's key layout, f.E / f.extraCol and h->rowLiteral:
// the key delta of a bind, the smallest key fields the shape fits on, "fits nowhere" (a quotient the field cannot hold), its fit shape — scheduling-key shapes that
// agree in everything a fit at priority -2 looks at (key fields, extras, requirement class, "never") share one, and ids are given in order of first occurrence, so a
// shape added later never renumbers an earlier one — and its part in the two minima.  buildFast over all shapes; asched_jobs_append's in-place path for the new ones.
static void fastShapeAdd(asched* h, int s) {
  Dev& d = h->dev; FastCfg& f = d.f;
  const int R = h->R, K = h->K;
  const bool twoWords = d.cfg.keyWords == 2;
  uint64_t delta = 0, mn = 0; uint8_t never = 0;
  if (!twoWords) {
    for (int c = 0; c < K; c++) {
      int64_t q = h->shapeReq[(size_t)s * R + h->indexedCol[c]] / d.cfg.indexedRes[c];   // (the key's divisor: the index resolution, or layoutKeys' coarser one)
      int64_t fm = q - d.cfg.keyLo[c];
      int w = d.cfg.keyWidth[c];
      if (w < 63 && (fm >= ((int64_t)1 << w) || q >= ((int64_t)1 << w))) { never = 1; continue; }
      delta |= (uint64_t)q << d.cfg.keyShift[c];
      mn |= (uint64_t)fm << d.cfg.keyShift[c];
    }
    if (!never) {
      for (int c = 0; c < K; c++) h->fsMinField[c] = std::min(h->fsMinField[c], h->shapeReq[(size_t)s * R + h->indexedCol[c]] / d.cfg.indexedRes[c] - d.cfg.keyLo[c]);
      for (int e = 0; e < f.E; e++) h->fsMinExtra[e] = std::min(h->fsMinExtra[e], h->shapeReq[(size_t)s * R + f.extraCol[e]]);
    }
  }
  h->fsDelta.push_back(delta); h->fsMin.push_back(mn); h->fsNever.push_back(never);
  ShapeReq q; q.fieldMin = mn; q.ex0 = f.E > 0 ? h->shapeReq[(size_t)s * R + f.extraCol[0]] : 0; q.ex1 = f.E > 1 ? h->shapeReq[(size_t)s * R + f.extraCol[1]] : 0;
  q.cls = h->shapeClass[s]; q.never = (never || h->rowLiteral[s]) ? 1 : 0;
  auto key = std::make_tuple(q.fieldMin, delta, q.ex0, q.ex1, q.cls, q.never);   // (the key delta is what a bind subtracts: same key fields => same delta)
  auto it = h->fitIds.find(key);
  if (it == h->fitIds.end()) { it = h->fitIds.emplace(key, (int32_t)h->fitTab.size()).first; h->fitTab.push_back(q); }
  h->fitOf.push_back(it->second);
  f.F = (int)h->fitTab.size();
}
// f.minFieldMin / f.minExtra from the handle's running minima
static void fastMinimaPack(asched* h) {
  Dev& d = h->dev; FastCfg& f = d.f;
  f.minFieldMin = 0;
  for (int c = 0; c < h->K && d.cfg.keyWords != 2; c++) if (h->fsMinField[c] != INT64_MAX) f.minFieldMin |= (uint64_t)h->fsMinField[c] << d.cfg.keyShift[c];
  for (int e = 0; e < MAXE; e++) f.minExtra[e] = h->fsMinExtra[e] == INT64_MAX ? 0 : h->fsMinExtra[e];
}
// the JobRec of a row of scheduling-key shape s (buildFast's fill of every row; one template per shape in asched_jobs_append's in-place path)
static void fastRecFill(asched* h, JobRec& r, int s, const int64_t* req, int32_t pc, int32_t gang, int32_t node0, int32_t runPrio) {
  const FastCfg& f = h->dev.f;
  memset(&r, 0, sizeof r);
  for (int x = 0; x < h->R; x++) r.req[x] = req[x];
  // literal rows: the generic path decides.  bit 1: some indexed request is not a multiple of its resolution — keyDelta (its quotients) is then NOT what a
  // bind takes off a node's key fields, so no fast path may bind / unbind such a job by key arithmetic (the evicted job returning to its node included)
  r.keyDelta = h->fsDelta[s]; r.fieldMin = h->fsMin[s]; r.never = ((h->fsNever[s] || h->rowLiteral[s]) ? 1 : 0) | (h->shapeUnaligned[s] ? 2 : 0);
  r.pc = pc; r.shape = h->fitOf[s]; r.gang = gang; r.node0 = node0; r.runPrio = runPrio; r.cls = h->shapeClass[s];
  r.pcPrio = h->pcPriority[r.pc]; r.preemptible = h->pcPreemptible[r.pc] ? 1 : 0;
  auto levels = [&](int32_t cutoff) { int nl = 0; while (nl < h->P && h->prios[nl] <= cutoff) nl++; return (uint8_t)nl; };
  r.nlPc = levels(r.preemptible ? r.pcPrio : INT32_MAX); r.nlRun = levels(r.preemptible ? r.runPrio : INT32_MAX);
  r.ex0 = f.E > 0 ? r.req[f.extraCol[0]] : 0; r.ex1 = f.E > 1 ? r.req[f.extraCol[1]] : 0;
}

// Fast path tables (round_fast.h): exactness conditions, per-shape packed key deltas, JobRec array, node class bits, base buffers.
// Called from rebuildMasks once nodes and jobs are both known.
int buildFast(asched* h, const std::vector<uint64_t>& classMask) {
  Dev& d = h->dev;
  FastCfg& f = d.f;
  memset(&f, 0, sizeof f);
  h->fastBufs.freeAll();
  h->qsOrig.valid = false;   // the parked QCAPF-sized stream buffers of a wide round lived in fastBufs: gone with it (a later round_prepare must not put them back)
  d.baseKey = nullptr; d.jrec = nullptr;
  // (and everything else that lived in fastBufs: a table that loses the fast structure — allocatable above total after a nodes_upsert or the rebuild path of
  //  asched_nodes_patch — must not leave pointers behind that the round tests for existence, d.evCheap in evictPhaseSplit)
  d.shapeTab = nullptr; d.nodeCls = nullptr; d.baseNode = nullptr; d.baseExtra = nullptr; d.baseCls = nullptr; d.baseRemoved = nullptr; d.posOf = nullptr; d.l0Slot = nullptr;
  d.evIdxByPos = nullptr; d.evKey = nullptr; d.evCheap = nullptr; d.evPart = nullptr; d.evMono = nullptr; d.evEdge = nullptr; d.l0Save = nullptr; d.candPosSave = nullptr;
  d.qsKey = nullptr; d.qsIn = nullptr; d.qsPart = nullptr; d.qsLen = nullptr; d.qsSave = nullptr; d.mg = nullptr; d.fitBits = nullptr;
  int R = h->R, K = h->K, N = h->N, M = h->M, S = h->S, W = d.cfg.W;
  std::vector<int> extra;
  for (int r = 0; r < R; r++) { bool idx = false; for (int c = 0; c < K; c++) idx = idx || h->indexedCol[c] == r; if (!idx) extra.push_back(r); }
  bool reqNonNeg = true;
  for (int64_t v : h->jReq) if (v < 0) reqNonNeg = false;
  std::set<int32_t> distinctIdx(h->indexedCol.begin(), h->indexedCol.end());
  // (allocatable need not be a multiple of the index resolution: the key arithmetic of a bind is exact for aligned requests, round_ctl.h fastKeyOf; a
  //  requirement class that matches several node types over unaligned allocatable is on the literal path, rebuildMasks)
  bool ok = N > 0 && M > 0 && S > 0 && !h->hasAllocByPrio && h->allocLeTotal && h->C <= 64 && reqNonNeg &&
            (int)extra.size() <= MAXE && (int)distinctIdx.size() == K;
  f.E = std::min<int>((int)extra.size(), MAXE);
  for (int e = 0; e < f.E; e++) f.extraCol[e] = extra[e];
  // one multi-level plane pass for the gate + urgency sweep: planes monotone in the level, and room for a level tag above the packed key
  const bool twoWords = d.cfg.keyWords == 2;   // two-word order keys (layoutKeys): the generic path of k_control_wk serves the handle — no fast structure, no fused pass
  if (twoWords) ok = false;
  f.cascadeFuse = !twoWords && !h->hasAllocByPrio && reqNonNeg && K > 0 && d.cfg.keyShift[0] + d.cfg.keyWidth[0] + d.cfg.keyGuard <= SCAN_LEVEL_SHIFT && h->P <= 15;
  if (const char* e = getenv("ASCHED_NO_CASCADE_FUSE")) if (e[0] == '1') f.cascadeFuse = 0;
  for (int c = 0; c < K && !twoWords; c++) {
    int w = d.cfg.keyWidth[c];
    f.fieldMask[c] = (w >= 64 ? ~0ull : ((1ull << w) - 1)) << d.cfg.keyShift[c];
    if (d.cfg.keyGuard) f.guardMask |= 1ull << (d.cfg.keyShift[c] + w);
  }
  // per shape: key delta of a bind and the smallest key fields it fits on; fit shapes: scheduling-key shapes that agree in everything a fit at priority -2 looks
  // at (fastShapeAdd).  Kept on the handle: the in-place path of asched_jobs_append goes on from here
  h->fsDelta.clear(); h->fsMin.clear(); h->fsNever.clear(); h->fitOf.clear(); h->fitTab.clear(); h->fitIds.clear();
  for (int c = 0; c < MAXK; c++) h->fsMinField[c] = INT64_MAX;
  for (int e = 0; e < MAXE; e++) h->fsMinExtra[e] = INT64_MAX;
  for (int s = 0; s < S; s++) fastShapeAdd(h, s);
  fastMinimaPack(h);
  if (f.F > SMAX) ok = false;   // more fit shapes than candidate slots: the generic scan serves the round
  if (!ok) return 0;
  static_assert(sizeof(JobRec) == 128, "JobRec is one 128-byte burst");
  HostProf prof("buildFast");
  size_t recBytes = sizeof(JobRec) * (size_t)std::max(M, 1);
  if (h->stageRecsBytes < recBytes) { h->stageRecs.reset(new unsigned char[recBytes]); h->stageRecsBytes = recBytes; }   // not value-initialised: every record is written below
  JobRec* recs = (JobRec*)h->stageRecs.get();
  parallelChunks((size_t)M, 64, [&](size_t lo, size_t hi) {
    for (size_t j = lo; j < hi; j++) fastRecFill(h, recs[j], h->jShape[j], &h->jReq[j * R], h->jPc[j], h->jGangDense[j], h->jNode[j], h->jRunPrio[j]);
  });
  prof.lap("JobRec fill");
  const size_t jcap = std::max((size_t)M, h->jobCap);   // (the job table's capacity: asched_jobs_append writes the records of new rows behind the M uploaded here)
  d.jrec = (JobRec*)h->fastBufs.alloc<unsigned char>(sizeof(JobRec) * std::max<size_t>(jcap, 1));
  if (M) plat_h2d(d.jrec, recs, sizeof(JobRec) * (size_t)M);
  prof.lap("JobRec upload");
  d.shapeTab = h->fastBufs.upload(h->fitTab);
  f.maskMode = 0;   // decided below, once the fit bitmaps exist
  std::vector<uint64_t> nodeCls(N, 0);
  for (int c = 0; c < h->C; c++) for (int n = 0; n < N; n++) if ((classMask[(size_t)c * W + (n >> 6)] >> (n & 63)) & 1) nodeCls[n] |= 1ull << c;
  d.nodeCls = h->fastBufs.upload(nodeCls);
  size_t Npad = d.cfg.Npad, Nb2 = 64;
  while (Nb2 < (size_t)N) Nb2 <<= 1;
  d.baseKey = h->fastBufs.alloc<uint64_t>(Nb2);
  d.baseNode = h->fastBufs.alloc<int32_t>(Npad); d.baseExtra = h->fastBufs.alloc<int64_t>(Npad * MAXE); d.baseCls = h->fastBufs.alloc<uint64_t>(Npad);
  d.baseRemoved = h->fastBufs.alloc<uint8_t>(Npad); d.posOf = h->fastBufs.alloc<int32_t>(Npad); d.l0Slot = h->fastBufs.alloc<int32_t>(Npad);
  d.evIdxByPos = h->fastBufs.alloc<int32_t>(jcap); d.evKey = h->fastBufs.alloc<EvKey>(jcap); d.evCheap = h->fastBufs.alloc<uint8_t>(4104 + jcap + 8);   // [0, 4098): per queue; from 4104: per evicted-list position (round_fast.h EV_EXCL)
  d.evChunks = 1024; d.evPart = h->fastBufs.alloc<int64_t>((size_t)d.evChunks * (2 * MAXR + 4));
  d.evMono = h->fastBufs.alloc<uint8_t>(4096 + 2); d.evEdge = h->fastBufs.alloc<uint64_t>((size_t)d.evChunks * 8); d.l0Save = h->fastBufs.alloc<int32_t>(L0CAP); d.candPosSave = h->fastBufs.alloc<int32_t>(SMAX);
  d.qsKey = nullptr; d.qsIn = nullptr; d.qsPart = nullptr; d.qsLen = nullptr; d.qsSave = nullptr;
  { const char* e = getenv("ASCHED_STREAM");   // ASCHED_STREAM=0: no stream runs (every queued-job iteration takes the two-wave path)
    if (!(e && e[0] == '0')) {
      d.qsKey = h->fastBufs.allocRaw<EvKey>((size_t)QCAPF * QS_CMAX); d.qsIn = h->fastBufs.alloc<QsIn>(QCAPF);
      d.qsPart = h->fastBufs.alloc<int64_t>((size_t)QCAPF * QS_CPQ * (MAXR + 2)); d.qsLen = h->fastBufs.alloc<int32_t>(2 * QCAPF); d.qsSave = h->fastBufs.alloc<QsSave>(QCAPF); plat_memset(d.qsSave, 0, sizeof(QsSave) * QCAPF);
    } }
  d.mg = nullptr;
  { const char* e = getenv("ASCHED_MERGE");   // ASCHED_MERGE=0: every stream run is merged by the control wave (rounds 2-5)
    if (d.qsKey && !(e && e[0] == '0')) {
      MgDev m; memset(&m, 0, sizeof m);
      m.cap = QCAPF * QS_CMAX + QCAPF;
      { const char* l = getenv("ASCHED_STREAM_LIMIT"); m.limitOff = (l && l[0] == '0') ? 1 : 0; }   // ASCHED_STREAM_LIMIT=0: a bulk-merged run ends where a queue's stream ends at its rate-limit tokens (round 6)
      m.q = h->fastBufs.alloc<MgQ>(QCAPF); m.key = h->fastBufs.allocRaw<WideKey>((size_t)m.cap); m.own = h->fastBufs.allocRaw<int32_t>((size_t)m.cap); m.rank = h->fastBufs.allocRaw<int32_t>((size_t)m.cap);
      m.merged = h->fastBufs.allocRaw<MgEnt>((size_t)m.cap); m.cmax = h->fastBufs.allocRaw<WideKey>((size_t)QCAPF * MG_CPQ); m.stop = h->fastBufs.alloc<uint32_t>(4); m.cut = h->fastBufs.alloc<WideKey>(1); m.cutPick = h->fastBufs.alloc<uint32_t>(1);
      d.mg = h->fastBufs.upload(std::vector<MgDev>{m});
    } }
  d.fitBits = nullptr; d.fitW = (N + 63) / 64;
  { const char* e = getenv("ASCHED_PREP_ONE");   // ASCHED_PREP_ONE=1 / 0: after a gang its queue's next stretch of single jobs becomes a stream at once (round_run.h fastStreamPrepareOne)
    // off by default: since round 5 a run goes on across gangs (round_fast.h streamNest), which keeps the bulk-prepared streams of ALL queues alive — configs[3] 981 ms ->
    // 781 ms with this off against 807 ms with it on (profiles/r05l_nested_gang_runs.txt); in round 4 it was -4 % on that shape and +80 % on the headline
    d.fitPad_ = (e && e[0] == '1') ? 1 : 0; }
  { const char* e = getenv("ASCHED_FIT_BITS");   // ASCHED_FIT_BITS=0: base rescans walk the base tiles (round-1 scheme)
    if (!(e && e[0] == '0')) d.fitBits = h->fastBufs.alloc<uint64_t>((size_t)f.F * d.fitW + 64);
    const char* m = getenv("ASCHED_SHAPE_MASK");   // ASCHED_SHAPE_MASK=1: the L0 list carries per-node fit masks (one bit test per entry in the L0 search, one mask recomputation per bind).
    // Off by default: measured on configs[2] (128 fit shapes) the recomputation costs more than the search saves (597 vs 573 ms per round in one call)
    if (d.fitBits && f.F <= 128 && m && m[0] == '1') f.maskMode = f.F <= 64 ? 1 : 2; }
  prof.lap("fast-structure allocations");
  f.structOk = 1;
  return 0;
}

int bitsFor(uint64_t range) { int b = 1; while (b < 64 && (range >> b)) b++; return b; }

}  // namespace

extern "C" {

asched_t* asched_create(const asched_config* c) {
  if (!c || c->num_resources < 1 || c->num_resources > MAXR || c->num_indexed < 1 || c->num_indexed > MAXK || c->num_priority_classes < 1 ||
      c->num_priority_classes > MAXPC)
    return nullptr;
  std::string perr;
  PlatCtx* pctx = plat_open(perr, c->device);
  if (!pctx) { fprintf(stderr, "asched_create: %s\n", perr.c_str()); return nullptr; }
  auto* h = new asched();
  h->plat = pctx;
  if (const char* e = getenv("ASCHED_EXCLUDED_NODES")) h->exclCap = std::max(0, atoi(e));   // (measurement: the default number of failed-selection records; asched_set_excluded_nodes is the API)
  h->R = c->num_resources; h->K = c->num_indexed; h->npc = c->num_priority_classes;
  h->indexedCol.assign(c->indexed_col, c->indexed_col + h->K);
  h->indexedRes.assign(c->indexed_resolution, c->indexed_resolution + h->K);
  for (auto r : h->indexedRes) if (r <= 0) { asched_destroy(h); return nullptr; }
  h->pcPriority.assign(c->pc_priority, c->pc_priority + h->npc);
  h->pcPreemptible.assign(c->pc_preemptible, c->pc_preemptible + h->npc);
  h->pcAway.assign(h->npc, {});
  std::set<int32_t> ps;
  for (int i = 0; i < h->npc; i++) {
    ps.insert(h->pcPriority[i]);
    if (c->pc_away_off)
      for (int k = c->pc_away_off[i]; k < c->pc_away_off[i + 1]; k++) {
        h->pcAway[i].push_back({c->away_priority[k], c->away_well_known[k]}); ps.insert(c->away_priority[k]);
        if (c->away_nt_off) {
          h->pcAwayNodeTypes.resize(h->npc);
          h->pcAwayNodeTypes[i].resize(h->pcAway[i].size());
          for (int t = c->away_nt_off[k]; t < c->away_nt_off[k + 1]; t++) {
            asched::AwayEntry ent; ent.wkt = c->away_nt_well_known[t];
            if (ent.wkt < 0 || ent.wkt >= c->num_well_known_types) { asched_destroy(h); return nullptr; }  // "unknown well-known node type" (nodedb.go:664-667)
            for (int q = c->away_nt_cond_off[t]; q < c->away_nt_cond_off[t + 1]; q++) {
              if (c->away_cond_resource[q] >= h->R) { asched_destroy(h); return nullptr; }
              ent.conds.push_back({c->away_cond_resource[q], c->away_cond_op[q], c->away_cond_value[q]});
            }
            h->pcAwayNodeTypes[i].back().push_back(ent);
          }
        }
      }
  }
  if (c->resource_unit) { h->resourceUnit.assign(c->resource_unit, c->resource_unit + h->R); for (int64_t u : h->resourceUnit) if (u <= 0) { asched_destroy(h); return nullptr; } }
  h->wktTaints.assign(std::max(c->num_well_known_types, 0), {});
  if (c->wkt_taint_off)
    for (int i = 0; i < c->num_well_known_types; i++)
      for (int k = c->wkt_taint_off[i]; k < c->wkt_taint_off[i + 1]; k++) h->wktTaints[i].push_back({c->wkt_taint_key[k], c->wkt_taint_value[k], c->wkt_taint_effect[k]});
  {
    int tot = 0;
    for (int i = 0; i < h->npc; i++)
      for (auto& aw : h->pcAway[i]) { tot++; if (aw.second < -1 || aw.second >= (int)h->wktTaints.size()) { asched_destroy(h); return nullptr; } }  // -1: WellKnownNodeTypeName ""
    if (tot > MAXAWAY) { asched_destroy(h); return nullptr; }
  }
  h->drfMult.assign(c->drf_multiplier, c->drf_multiplier + h->R);
  h->indexAllTaints = c->num_indexed_taints < 0;
  for (int i = 0; i < c->num_indexed_taints; i++) h->indexedTaints.insert(c->indexed_taint_keys[i]);
  for (int i = 0; i < c->num_indexed_labels; i++) h->indexedLabels.insert(c->indexed_label_keys[i]);
  h->maxFraction.assign(h->R, INFINITY);
  if (c->max_fraction_to_schedule) h->maxFraction.assign(c->max_fraction_to_schedule, c->max_fraction_to_schedule + h->R);
  h->disallowed.assign(h->R, 0);
  if (c->disallowed_resource) h->disallowed.assign(c->disallowed_resource, c->disallowed_resource + h->R);
  h->prios = {ASCHED_EVICTED_PRIORITY, ASCHED_CROSS_POOL_PRIORITY};
  for (int32_t p : ps) h->prios.push_back(p);
  h->P = (int)h->prios.size();
  if (h->P > MAXP) { asched_destroy(h); return nullptr; }
  memset(&h->dev, 0, sizeof(Dev));
  DevCfg& dc = h->dev.cfg;
  dc.R = h->R; dc.K = h->K; dc.P = h->P; dc.npc = h->npc;
  for (int i = 0; i < h->P; i++) dc.prios[i] = h->prios[i];
  for (int i = 0; i < h->K; i++) { dc.indexedCol[i] = h->indexedCol[i]; dc.indexedRes[i] = h->indexedRes[i]; }
  for (int i = 0; i < h->npc; i++) { dc.pcPriority[i] = h->pcPriority[i]; dc.pcPreemptible[i] = h->pcPreemptible[i]; }
  {
    int k = 0;
    for (int i = 0; i < h->npc; i++) {
      dc.pcAwayOff[i] = k;
      for (size_t ai = 0; ai < h->pcAway[i].size(); ai++) {
        auto& aw = h->pcAway[i][ai];
        // "no extra taints to tolerate" (nodedb.go:703-706) decided per entry here when it cannot depend on the job; an entry whose
        // NodeTypes conditions leave a particular shape without taints gets an all-zero mask row for that shape instead (jobs_set)
        bool usable = aw.second >= 0 && !h->wktTaints[aw.second].empty();
        if (i < (int)h->pcAwayNodeTypes.size() && ai < h->pcAwayNodeTypes[i].size())
          for (auto& nt : h->pcAwayNodeTypes[i][ai]) if (!h->wktTaints[nt.wkt].empty()) usable = true;
        dc.awayPrio[k] = aw.first; dc.awayUsable[k] = usable; k++;
      }
    }
    for (int i = h->npc; i <= MAXPC; i++) dc.pcAwayOff[i] = k;
  }
  for (int i = 0; i < h->R; i++) { dc.drfMult[i] = h->drfMult[i]; dc.disallowed[i] = h->disallowed[i]; }
  dc.preferLarge = c->prefer_large_job_ordering; dc.protectUncapped = c->protect_uncapped_adjusted_fair_share;
  dc.disableHome = c->disable_home_scheduling; dc.disableAway = c->disable_away_scheduling; dc.disableGangAway = c->disable_gang_away_scheduling;
  dc.disableFair = c->disable_fairshare_scheduling; dc.disableUrgency = c->disable_urgency_scheduling;
  dc.preferHome = c->preempt_cross_pool_jobs_first != 0;
  dc.protectedFraction = c->protected_fraction_of_fair_share; dc.maxLookback = c->max_queue_lookback;
  dc.evLevel = 0;
  // floating resources: per column, the pool's total (>= 0) or -1 = not floating (floatingresources/floating_resource_types.go)
  h->floatingLimit.assign(h->R, -1);
  if (c->floating_resource_limit) h->floatingLimit.assign(c->floating_resource_limit, c->floating_resource_limit + h->R);
  h->floatingInTotal = c->floating_counts_in_total != 0;
  for (int i = 0; i < h->R; i++) {
    dc.isFloating[i] = h->floatingLimit[i] >= 0; dc.floatingLimit[i] = std::max<int64_t>(h->floatingLimit[i], 0);
    if (dc.isFloating[i]) { dc.anyFloating = 1; if (dc.floatingLimit[i] != 0) dc.floatingConfigured = 1; }
    for (int k = 0; k < h->K; k++) if (dc.isFloating[i] && h->indexedCol[k] == i) { asched_destroy(h); return nullptr; }  // floating resources are not on nodes: they cannot be indexed
  }
  dc.maxNewJobNs = c->max_new_job_scheduling_duration_ns; dc.maxNewJobPerQueueNs = c->max_new_job_scheduling_duration_per_queue_ns;
  dc.clockStepNs = c->clock_step_ns; dc.wallClockKHz = plat_wall_clock_khz();
  h->dev.rs = (RoundScalars*)plat_malloc(sizeof(RoundScalars));
  plat_memset(h->dev.rs, 0, sizeof(RoundScalars));
  h->dev.cmdIO = (int32_t*)plat_malloc(sizeof(int32_t) * (16 + CMDIO_ARG_WORDS));
  h->dev.scanResult = (uint64_t*)plat_malloc(sizeof(uint64_t) * 8);
  h->dev.undoCap = 1 << 20;
  h->dev.undo = (int32_t*)plat_malloc(sizeof(int32_t) * 4 * h->dev.undoCap);
  if (plat_take_failure()) { fprintf(stderr, "asched_create: %s\n", plat_last_error()); asched_destroy(h); return nullptr; }
  return h;
}

void asched_destroy(asched_t* h) {
  if (!h) return;
  plat_enter(h->plat);
  h->nodeBufs.freeAll(); h->jobBufs.freeAll(); h->queueBufs.freeAll(); h->maskBufs.freeAll(); h->fastBufs.freeAll(); h->pjBufs.freeAll(); h->evrBufs.freeAll(); h->exclBufs.freeAll(); h->jpBufs.freeAll(); h->npBufs.freeAll(); h->ndBufs.freeAll(); h->naBufs.freeAll(); h->ql.bufs.freeAll(); h->ql.heldBufs.freeAll();
  plat_pinned_free(h->resPin); plat_free(h->commStatus); plat_free(h->dev.rs); plat_free(h->dev.cmdIO); plat_free(h->dev.scanResult); plat_free(h->dev.undo);
  plat_close(h->plat);
  delete h;
}
const char* asched_last_error(asched_t* h) { plat_enter(h ? h->plat : nullptr); return h ? h->err.c_str() : "null handle"; }
int32_t asched_priorities(asched_t* h, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); for (int i = 0; i < h->P; i++) out[i] = h->prios[i]; return h->P; }

static void fastDeactivate(asched* h) {  // the fast structure stays (structOk) and is not in use: round_prepare decides iterOk again
  h->dev.f.iterOk = 0;
  int32_t zero = 0;
  plat_h2d(&h->dev.rs->fastActive, &zero, sizeof zero);
  plat_h2d(&h->dev.rs->l0SaveCount, &zero, sizeof zero);
}
static void fastInvalidate(asched* h) {  // inputs are being replaced: the level-0 fast structure no longer describes them
  h->dev.f.structOk = 0;
  fastDeactivate(h);
}
// What jobs_set resets, for a resident call on the job table, from its point of no return on (a device failure after it leaves the table half changed: asched_jobs_set
// before anything else).  fastGoes: the call ends with the tail of jobs_set (rebuildMasks), which builds the fast structure anew.  sizesStay: M and the capacities are
// what they were, so the evictor report's buffers still fit (asched_jobs_patch, asched_jobs_reprioritise)
static void residentTouchJobs(asched* h, bool fastGoes = false, bool sizesStay = false) {
  h->haveRoundResult = false; h->stateEpoch++;
  if (fastGoes) fastInvalidate(h); else fastDeactivate(h);
  h->prepared = false;
  if (!sizesStay) h->evrSized = false;
}
// What nodes_upsert resets, for a resident call on the node table: the above, and every priority level's planes are equal again
static void residentTouchNodes(asched* h) {
  residentTouchJobs(h);
  h->equalLevels = h->P;
}

}  // extern "C"
namespace {
// NewNodeType (internaltypes/node_type.go:68-131) of a node with these taints (the unschedulable taint included) and labels: the type and its canonical string
void nodeTypeOf(asched* h, const std::vector<HTaint>& taints, const std::vector<HSel>& labels, HType& t, std::string& canon) {
  for (auto& x : taints) if (h->indexAllTaints || h->indexedTaints.count(x.key)) t.taints.push_back(x);
  std::stable_sort(t.taints.begin(), t.taints.end(), [](const HTaint& a, const HTaint& b) { return a.key < b.key; });
  for (auto& l : labels) if (h->indexedLabels.count(l.key)) t.labels.push_back(l);
  std::sort(t.labels.begin(), t.labels.end(), [](const HSel& a, const HSel& b) { return a.key < b.key; });
  for (int32_t k : h->indexedLabels) { bool has = false; for (auto& l : t.labels) if (l.key == k) has = true; if (!has) t.unset.push_back(k); }
  for (auto& x : t.taints) canon += "t" + std::to_string(x.key) + "=" + std::to_string(x.value) + ":" + std::to_string(x.effect) + "$";
  canon += "&";
  for (auto& l : t.labels) canon += std::to_string(l.key) + "=" + std::to_string(l.value) + "$";
}

// What nodesUpsertBody would refuse for a table of `N` rows with these populated node types and this allocatable [N][R], decided before anything changes: the key
// layout of that table (layoutKeys) and LIT_TMAX for a row on the literal iteration path.  Everything the decision touches is saved and put back: the handle is as it
// was on return.  The rebuild paths of asched_nodes_patch and asched_nodes_delete share it.  0, or the code with the reason in rwhy
int rebuildRefusal(asched* h, std::vector<HType>& typesAfter, const int64_t* alloc, int N, std::string& rwhy) {
  Dev& d = h->dev;
  const int R = h->R, K = h->K;
  const DevCfg cfgSaved = d.cfg; const bool keyWideSaved = h->keyWide, keyCoarseSaved = h->keyCoarse, alignedSaved = h->allocAligned;
  const int nSaved = h->N;
  const std::string errSaved = h->err;
  int64_t maxQ[MAXK], minQ[MAXK], gcdV[MAXK], maxV[MAXK];
  for (int c = 0; c < MAXK; c++) { maxQ[c] = h->keyMaxQ[c]; minQ[c] = h->keyMinQ[c]; gcdV[c] = h->keyGcdV[c]; maxV[c] = h->keyMaxV[c]; }
  h->types.swap(typesAfter);
  h->N = N;
  h->allocAligned = true;
  for (int c = 0; c < K; c++) {
    const int64_t res = h->indexedRes[c]; const int col = h->indexedCol[c];
    int64_t q = 0, g = 0, mv = 0;
    for (int v = 0; v < N; v++) { const int64_t a = alloc[(size_t)v * R + col]; if (a % res) h->allocAligned = false; q = std::max(q, a / res); g = std::gcd(g, a < 0 ? -a : a); mv = std::max(mv, a); }
    h->keyMaxQ[c] = q; h->keyMinQ[c] = 0; h->keyGcdV[c] = g; h->keyMaxV[c] = mv;
  }
  int rrc = layoutKeys(h);
  rwhy = rrc ? h->err : std::string();
  if (!rrc && h->jobsSet) {
    const int Sext = h->S + (int)h->awayRowClass.size();
    for (int row = 0; row < Sext && !rrc; row++) {
      const int shape = row < h->S ? row : h->awayRowShape[row - h->S], cls = row < h->S ? h->shapeClass[row] : h->awayRowClass[row - h->S];
      size_t nTypes = 0;
      for (auto& t : h->types) if (classMatchesType(h, cls, t)) nTypes++;
      const bool literal = h->shapeUnaligned[shape] || (nTypes > 1 && !(h->allocAligned && h->idRankMonotone));
      if (literal && nTypes > LIT_TMAX) { rrc = ASCHED_ERR_UNSUPPORTED; rwhy = "a requirement class on the literal iteration path matches more than LIT_TMAX node types"; }
    }
  }
  h->types.swap(typesAfter); h->N = nSaved; h->allocAligned = alignedSaved; d.cfg = cfgSaved; h->keyWide = keyWideSaved; h->keyCoarse = keyCoarseSaved; h->err = errSaved;
  for (int c = 0; c < MAXK; c++) { h->keyMaxQ[c] = maxQ[c]; h->keyMinQ[c] = minQ[c]; h->keyGcdV[c] = gcdV[c]; h->keyMaxV[c] = maxV[c]; }
  return rrc;
}

// asched_nodes_upsert, and the rebuild path of asched_nodes_patch on the patched table
int nodesUpsertBody(asched* h, const asched_nodes* in) {
  h->haveRoundResult = false; h->stateEpoch++;
  fastInvalidate(h);
  h->nodeBufs.freeAll();
  Dev& d = h->dev;
  int N = h->N = in->n, R = h->R, P = h->P, K = h->K;
  int Npad = ((N + 63) / 64) * 64; if (Npad == 0) Npad = 64;
  d.cfg.N = N; d.cfg.Npad = Npad; d.cfg.W = Npad / 64;
  h->nodeTaints.assign(N, {}); h->nodeLabels.assign(N, {}); h->nodeType.assign(N, 0); h->types.clear(); h->typeId.clear();
  h->nodeTotal.assign(in->total, in->total + (size_t)N * R);
  h->nodeAllocHost.assign(in->allocatable, in->allocatable + (size_t)N * R); h->nodeIndexHost.assign(in->index, in->index + N);
  if (in->over_allocated) h->nodeOverAlloc.assign(in->over_allocated, in->over_allocated + N); else h->nodeOverAlloc.assign(N, 0);
  h->hasTypeOverride = in->node_type_override != nullptr; h->uploadedAllocByPrio = in->alloc_by_prio != nullptr;
  auto& typeByCanon = h->typeByCanon; typeByCanon.clear();
  std::vector<int64_t> totalRes((size_t)R * Npad, 0), allocatable((size_t)R * Npad, 0), alloc0;
  if (in->alloc_by_prio) alloc0.assign((size_t)P * R * Npad, 0);
  std::vector<uint8_t> flags(N, 0);
  h->nodeUnsched.assign(N, 0); h->evrSized = false;
  int64_t total[MAXR] = {0};
  for (int i = 0; i < N; i++) {
    bool unsched = in->unschedulable && in->unschedulable[i];
    if (in->taint_off) for (int k = in->taint_off[i]; k < in->taint_off[i + 1]; k++) h->nodeTaints[i].push_back({in->taint_key[k], in->taint_value[k], in->taint_effect[k]});
    if (unsched) h->nodeTaints[i].push_back({kUnschedulableTaintKey, 0, ASCHED_EFFECT_NO_SCHEDULE});  // node.go:127-129
    if (in->label_off) for (int k = in->label_off[i]; k < in->label_off[i + 1]; k++) h->nodeLabels[i].push_back({in->label_key[k], in->label_value[k]});
    flags[i] = (unsched && in->over_allocated && in->over_allocated[i]) ? 1 : 0;
    h->nodeUnsched[i] = unsched ? 1 : 0;
    HType t; std::string canon;
    int64_t ov = in->node_type_override ? in->node_type_override[i] : -1;
    if (ov >= 0) canon = "o" + std::to_string(ov);
    else nodeTypeOf(h, h->nodeTaints[i], h->nodeLabels[i], t, canon);
    auto it = typeByCanon.find(canon);
    if (it == typeByCanon.end()) { it = typeByCanon.emplace(canon, (int)h->types.size()).first; h->types.push_back(t); h->typeId.push_back(ov); }
    h->nodeType[i] = it->second;
    h->types[it->second].numNodes++;
    for (int r = 0; r < R; r++) {
      if (d.cfg.isFloating[r]) {  // not a node resource: the planes carry a capacity no request can exhaust, so the column never constrains a node
        totalRes[(size_t)r * Npad + i] = allocatable[(size_t)r * Npad + i] = FLOATING_NODE_CAPACITY;
        if (in->alloc_by_prio) for (int l = 0; l < P; l++) alloc0[((size_t)l * R + r) * Npad + i] = FLOATING_NODE_CAPACITY;
        continue;
      }
      totalRes[(size_t)r * Npad + i] = in->total[(size_t)i * R + r];
      allocatable[(size_t)r * Npad + i] = in->allocatable[(size_t)i * R + r];
      total[r] += in->allocatable[(size_t)i * R + r];  // addNodeToStats nodedb.go:44-55
      if (in->alloc_by_prio)
        for (int l = 0; l < P; l++) alloc0[((size_t)l * R + r) * Npad + i] = in->alloc_by_prio[((size_t)i * P + l) * R + r];
    }
  }
  // sctx.TotalResources = NodeDb total + the pool's floating totals (scheduling_algo.go:890); the gang scheduler tests use the NodeDb total alone
  for (int r = 0; r < R; r++) d.cfg.totalResources[r] = d.cfg.isFloating[r] ? (h->floatingInTotal ? d.cfg.floatingLimit[r] : 0) : total[r];
  h->hasAllocByPrio = in->alloc_by_prio != nullptr;
  h->allocLeTotal = true;
  for (size_t i = 0; i < (size_t)N * R; i++) if (!d.cfg.isFloating[i % R] && (in->allocatable[i] > in->total[i] || in->allocatable[i] < 0)) h->allocLeTotal = false;
  // node.index rank + id order check
  std::vector<int32_t> order(N), idxRank(N);
  for (int i = 0; i < N; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return in->index[a] < in->index[b]; });
  for (int i = 1; i < N; i++) if (in->index[order[i]] == in->index[order[i - 1]]) return fail(h, ASCHED_ERR_INVALID, "duplicate node index");
  h->nodeByRank = order;
  h->idRankMonotone = true; h->idRanksGiven = in->id_rank != nullptr;
  for (int i = 0; i < N; i++) { idxRank[order[i]] = i; if (i > 0 && in->id_rank && in->id_rank[order[i]] < in->id_rank[order[i - 1]]) h->idRankMonotone = false; }
  // key packing: field_c = alloc_c/res_c - lo_c in width_c bits; the node-index rank in the low bits (layoutKeys)
  h->allocAligned = true;
  for (int c = K - 1; c >= 0; c--) {
    int64_t res = h->indexedRes[c], maxq = 0, minq = 0;
    int col = h->indexedCol[c];
    for (int i = 0; i < N; i++) {
      int64_t a = in->allocatable[(size_t)i * R + col];
      if (a % res) h->allocAligned = false;
      maxq = std::max(maxq, a / res);
      if (in->alloc_by_prio)
        for (int l = 0; l < P; l++) {
          int64_t v = in->alloc_by_prio[((size_t)i * P + l) * R + col];
          if (v % res) h->allocAligned = false;
          maxq = std::max(maxq, v / res); minq = std::min(minq, v / res);
        }
    }
    h->keyMaxQ[c] = maxq; h->keyMinQ[c] = minq;
    {
      int64_t g = 0, mv = 0;
      for (int i = 0; i < N; i++) {
        int64_t a = in->allocatable[(size_t)i * R + col];
        g = std::gcd(g, a < 0 ? -a : a); mv = std::max(mv, a);
        if (in->alloc_by_prio) for (int l = 0; l < P; l++) { int64_t v = in->alloc_by_prio[((size_t)i * P + l) * R + col]; g = std::gcd(g, v < 0 ? -v : v); mv = std::max(mv, v); }
      }
      h->keyGcdV[c] = g; h->keyMaxV[c] = mv;
    }
  }
  if (int rc = layoutKeys(h)) return rc;
  // uniformity labels: values present on nodes, per indexed label (nodedb.go:143, addNodeToStats)
  h->labelSlots.assign(h->indexedLabels.begin(), h->indexedLabels.end());
  h->slotValues.assign(h->labelSlots.size(), {});
  h->slotValueCount.assign(h->labelSlots.size(), {});
  for (size_t s = 0; s < h->labelSlots.size(); s++) {
    std::map<int32_t, int32_t> vals;   // value -> nodes that carry it (asched_nodes_delete keeps the counts)
    for (int i = 0; i < N; i++) for (auto& l : h->nodeLabels[i]) if (l.key == h->labelSlots[s]) vals[l.value]++;
    for (auto& kv : vals) { h->slotValues[s].push_back(kv.first); h->slotValueCount[s].push_back(kv.second); }
  }
  d.totalRes = h->nodeBufs.upload(totalRes);
  d.allocatable = h->nodeBufs.upload(allocatable);
  d.alloc0 = in->alloc_by_prio ? h->nodeBufs.upload(alloc0) : nullptr;
  d.alloc = h->nodeBufs.alloc<int64_t>((size_t)P * R * Npad);
  d.keys = h->nodeBufs.alloc<uint64_t>((size_t)2 * P * Npad);   // (room for the low words of a two-word layout: the job table can still change the layout, layoutKeys)
  plat_memset(d.keys, 0xff, (size_t)2 * P * Npad * sizeof(uint64_t));
  d.nodeFlags = h->nodeBufs.upload(flags);
  d.idxRank = h->nodeBufs.upload(idxRank);
  d.nodeByRank = h->nodeBufs.upload(order);
  h->nodeIdRank.resize(N);
  for (int i = 0; i < N; i++) h->nodeIdRank[i] = in->id_rank ? in->id_rank[i] : i;
  d.nodeIdRank = h->nodeBufs.upload(h->nodeIdRank);
  d.lit = (LitIt*)h->nodeBufs.alloc<unsigned char>(LITIT_BYTES * LIT_TMAX);   // (room for the low bound word of a two-word key: dev.h LitIt)
  d.accAvail = h->nodeBufs.alloc<int64_t>((size_t)Npad * R);
  d.accStamp = h->nodeBufs.alloc<int32_t>(Npad);
  d.accStaticFailed = h->nodeBufs.alloc<uint8_t>(Npad);
  d.fairOff = h->nodeBufs.alloc<int32_t>((size_t)Npad + 2); d.fairPart = h->nodeBufs.alloc<int32_t>(FAIR_CHUNKS + 1);
  d.nodeOver = h->nodeBufs.alloc<int32_t>(Npad);
  h->nodesSet = true; h->prepared = false;
  h->allocPristine = true;
  h->equalLevels = P;
  if (in->alloc_by_prio) {   // e.g. testfixtures.WithUsedResourcesNodes: resources used at some priority lower the planes at and below it — the levels up to the first one that differs still agree
    int eq = 1;
    for (; eq < P; eq++) {
      bool same = true;
      for (int i = 0; i < N && same; i++) for (int r = 0; r < R; r++) if (in->alloc_by_prio[((size_t)i * P + eq) * R + r] != in->alloc_by_prio[((size_t)i * P) * R + r]) { same = false; break; }
      if (!same) break;
    }
    h->equalLevels = eq;
  }
  int rc = runControl(h, CMD_UPSERT_RESET);
  if (rc) return rc;
  return rebuildMasks(h);
}

// node and job dynamic state as at the end of jobs_set: everything unbound until round_prepare — what CMD_UPSERT_RESET and CMD_RESET_JOBS do (round_run.h controlMain), with
// their per-element passes on the whole grid instead of the control workgroup (B_RESET_JOBS also forgets the failed-selection records: asched_excluded_nodes).  The tail of
// asched_jobs_patch, asched_jobs_append and asched_nodes_patch; M: rows of the job table
int resetDynamicState(asched* h, int M) {
  Dev& d = h->dev;
  h->stateEpoch++;
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (plat_bulk(d, B_INIT_ALLOC, h->N) || plat_bulk(d, B_KEYS_ALL, h->N) || plat_bulk(d, B_RESET_JOBS, M)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  plat_d2h(&h->rsHost, d.rs, sizeof(RoundScalars));
  if (h->rsHost.error) {
    int e = h->rsHost.error;
    char buf[128]; snprintf(buf, sizeof buf, "device raised error %d (detail %d)", e, h->rsHost.errorDetail);
    int32_t zero[2] = {0, 0};
    plat_h2d(&d.rs->error, zero, sizeof zero);
    return fail(h, e, buf);
  }
  h->rsHost.fastActive = 0; h->rsHost.evictedTableSize = 0; h->rsHost.fairIndexValid = 0; h->rsHost.ftValid = 0; h->rsHost.txnActive = 0; h->rsHost.undoCount = 0;
  plat_h2d(d.rs, &h->rsHost, sizeof(RoundScalars));
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  h->allocPristine = h->nodesSet;
  h->evictedDirty = false;
  return 0;
}
}  // namespace
extern "C" {

int32_t asched_nodes_upsert(asched_t* h, const asched_nodes* in) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  memset(h->npStats, 0, sizeof h->npStats); memset(h->ndStats, 0, sizeof h->ndStats); memset(h->naStats, 0, sizeof h->naStats);
  return nodesUpsertBody(h, in);
}

// the per-job state of a round (everything indexed by job or by a position of a per-job list), zeroed, with room for `cap` rows: jobs_set takes exactly M,
// asched_jobs_append a capacity (DESIGN 3.10).  Static per-job arrays (what jobs_set uploads) are not here: an append moves them.
static void allocJobState(asched* h, size_t cap) {
  Dev& d = h->dev;
  auto A32 = [&](size_t n) { return h->jobBufs.alloc<int32_t>(n); };
  auto A8 = [&](size_t n) { return h->jobBufs.alloc<uint8_t>(n); };
  const size_t M = cap;
  d.schedAtPrio = A32(M); d.jobNode = A32(M); d.jobCutoff = A32(M); d.jobEvictedOnNode = A8(M); d.jobFlags = A8(M);
  d.optSched = A8(M); d.optPre = A8(M); d.optGhost = A32(M);
  d.jcEvicted = A8(M); d.jcAssigned = A32(M); d.jcReason = A32(M); d.jcHasPctx = A8(M);
  d.pcNode = A32(M); d.pcSap = A32(M); d.pcPap = A32(M); d.pcMethod = A32(M); d.jcGangCard = A32(M); d.jcPreempted = A8(M);
  d.jcUniValue = A32(M); d.jcStagedBy = A32(M); d.jcPreSib = A32(M);
  d.inPreempted = A8(M); d.inScheduled = A8(M); d.inSchedAndEvicted = A8(M); d.preemptedNode = A32(M);
  d.evList = A32(M); d.evSortKey = h->jobBufs.alloc<uint32_t>(M + 1); d.evTabJob = A32(M); d.evTabAlive = A8(M); d.evIndexOfJob = A32(M);
  d.fairEnt = A32(M); d.fairEntJob = A32(M);
  d.evFlag = A8(M); d.preList = A32(M);
  d.resJob = A32(M); d.resNode = A32(M); d.resPrio = A32(M); d.resMethod = A32(M); d.resPreJob = A32(M); d.resPreNode = A32(M);
}
// the per-gang state: G gangs + the scratch gang of schedule_many; arrLen: gangOff[G + 1], the members of every gang and of the scratch gang
static void allocGangState(asched* h, size_t G, size_t arrLen) {
  Dev& d = h->dev;
  d.gangSeen = h->jobBufs.alloc<int32_t>(G + 1); d.gangArr = h->jobBufs.alloc<int32_t>(arrLen); d.gangTotal = h->jobBufs.alloc<int64_t>((G + 1) * (size_t)h->R);
  d.gangAllEvicted = h->jobBufs.alloc<uint8_t>(G + 1);
}
// the away rows of the shape table (jobs_set, and jobs_append when a new shape arrives): the derived requirement classes behind the C real ones, one mask row per
// (shape, away entry of its priority class).  Derived classes are numbered in shape order, so the same shape table gives the same rows.
static void deriveAwayRows(asched* h, bool anyAway) {
  const int R = h->R;
  // away attempts (nodedb.go:677-722) match statically with the job's tolerations + one toleration per taint of the well-known
  // node type: a derived requirement class per (class, well-known type), one extra mask row per (shape, away entry)
  h->clsTol.resize(h->C); h->clsSel.resize(h->C); if (!h->clsAff.empty()) h->clsAff.resize(h->C);
  h->awayRowOff.assign(h->S + 1, 0); h->awayRowClass.clear(); h->awayRowShape.clear();
  {
    // matchesCondition (nodedb.go:632-648), literally: the loop returns at the first condition whose operator it knows
    auto matches = [&](const std::vector<asched::AwayCond>& conds, const int64_t* req) {
      for (auto& cd : conds) {
        int64_t raw = cd.resource >= 0 ? req[cd.resource] : 0;  // GetByNameZeroIfMissing
        int64_t unit = cd.resource >= 0 && !h->resourceUnit.empty() ? h->resourceUnit[cd.resource] : 1;
        int64_t v = raw >= 0 ? (raw + unit - 1) / unit : -((-raw + unit - 1) / unit);  // Quantity.Value(): whole units, away from zero
        if (cd.op == ASCHED_AWAY_COND_GT) return v > cd.value;
        if (cd.op == ASCHED_AWAY_COND_LT) return v < cd.value;
        if (cd.op == ASCHED_AWAY_COND_EQ) return v == cd.value;
      }
      return true;
    };
    typedef std::vector<std::array<int32_t, 3>> TaintKey;
    std::map<std::pair<int32_t, TaintKey>, int32_t> derived;
    for (int sidx = 0; sidx < h->S; sidx++) {
      h->awayRowOff[sidx] = (int32_t)h->awayRowClass.size();
      if (!anyAway) continue;
      int pc = h->shapePc[sidx];
      for (size_t ai = 0; ai < h->pcAway[pc].size(); ai++) {
        auto& aw = h->pcAway[pc][ai];
        // getEffectiveAwayNodeTaints (nodedb.go:650-675): the conditions read the job's requests, i.e. they are a property of the shape
        std::vector<HTaint> taints;
        if (aw.second >= 0) taints = h->wktTaints[aw.second];
        if (pc < (int)h->pcAwayNodeTypes.size() && ai < h->pcAwayNodeTypes[pc].size())
          for (auto& nt : h->pcAwayNodeTypes[pc][ai])
            if (matches(nt.conds, &h->shapeReq[(size_t)sidx * R])) taints.insert(taints.end(), h->wktTaints[nt.wkt].begin(), h->wktTaints[nt.wkt].end());
        TaintKey tk;
        for (auto& t : taints) tk.push_back({t.key, t.value, t.effect});
        auto key = std::make_pair(h->shapeClass[sidx], tk);
        auto it = derived.find(key);
        if (it == derived.end()) {
          int32_t id = (int32_t)h->clsTol.size();
          std::vector<HTol> tol = h->clsTol[key.first];
          std::vector<HSel> sel = h->clsSel[key.first];
          for (auto& t : taints) {  // :708-717
            HTol x{t.key, ASCHED_TOLERATION_OP_EQUAL, t.value, t.effect};
            if (t.value == -1) { x.op = ASCHED_TOLERATION_OP_EXISTS; x.value = 0; }
            tol.push_back(x);
          }
          // no taints for this shape: the reference returns "no node" for the entry (:703-706) — a class no node satisfies
          if (taints.empty()) sel.push_back({kNoSuchLabelKey, 0});
          h->clsTol.push_back(tol); h->clsSel.push_back(sel);
          if (!h->clsAff.empty()) h->clsAff.push_back(h->clsAff[key.first]);
          it = derived.emplace(key, id).first;
        }
        h->awayRowClass.push_back(it->second); h->awayRowShape.push_back(sidx);
      }
    }
    h->awayRowOff[h->S] = (int32_t)h->awayRowClass.size();
  }
  h->Cext = (int)h->clsTol.size();
}

int32_t asched_set_label_value_ints(asched_t* h, int32_t n, const int32_t* ids, const int64_t* ints) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (n < 0 || (n > 0 && (!ids || !ints))) return fail(h, ASCHED_ERR_INVALID, "set_label_value_ints: bad arguments");
  h->valueInts.clear();
  for (int i = 0; i < n; i++) h->valueInts[ids[i]] = ints[i];
  return 0;
}
// class i of an asched_req_classes: its tolerations, node selector and required node affinity (asched_jobs_set, asched_req_classes_append)
static int reqClassParse(asched* h, const asched_req_classes* c, int i, std::vector<HTol>& tol, std::vector<HSel>& sel, HAffinity& aff) {
  if (c->tol_off) for (int k = c->tol_off[i]; k < c->tol_off[i + 1]; k++) tol.push_back({c->tol_key[k], c->tol_op[k], c->tol_value[k], c->tol_effect[k]});
  if (c->sel_off) for (int k = c->sel_off[i]; k < c->sel_off[i + 1]; k++) sel.push_back({c->sel_key[k], c->sel_value[k]});
  if (c->has_affinity && c->has_affinity[i]) {
    aff.present = true;
    for (int t = c->aff_term_off[i]; t < c->aff_term_off[i + 1]; t++) {
      std::vector<HAffExpr> term;
      for (int x = c->aff_expr_off[t]; x < c->aff_expr_off[t + 1]; x++) {
        HAffExpr ex; ex.key = c->aff_expr_key[x]; ex.op = c->aff_expr_op[x];
        if (ex.op < ASCHED_AFFINITY_OP_IN || ex.op > ASCHED_AFFINITY_OP_LT) return fail(h, ASCHED_ERR_UNSUPPORTED, "unknown node affinity operator");
        ex.values.assign(c->aff_values + c->aff_value_off[x], c->aff_values + c->aff_value_off[x + 1]);
        term.push_back(ex);
      }
      aff.terms.push_back(term);
    }
  }
  return 0;
}
int32_t asched_jobs_set(asched_t* h, const asched_jobs* j, const asched_req_classes* c) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (h) { h->haveRoundResult = false; h->stateEpoch++; }
  fastInvalidate(h);
  h->jobBufs.freeAll();
  h->jp = {};   // (its buffers lived in jobBufs)
  HostProf prof("jobs_set");
  Dev& d = h->dev;
  int M = h->M = j->m, R = h->R;
  d.cfg.M = M;
  auto cp32 = [&](const int32_t* s, int32_t def) { std::vector<int32_t> v(M, def); if (s) v.assign(s, s + M); return v; };
  h->jQueue = cp32(j->queue, 0); h->jPc = cp32(j->pc, 0); h->jReqClass = cp32(j->req_class, 0);
  std::vector<int32_t> gangId = cp32(j->gang_id, -1), gangCard = cp32(j->gang_cardinality, 1), gangUni = cp32(j->gang_uniformity_label, -1);
  h->jNode = cp32(j->node, -1); h->jRunPrio = cp32(j->scheduled_at_priority, 0);
  h->jAway.assign(M, 0); h->anyAway = false;
  if (j->away) for (int i = 0; i < M; i++) if (j->away[i]) { h->jAway[i] = 1; h->anyAway = true; }
  std::vector<uint32_t> qprio(M, 0); if (j->queue_priority) qprio.assign(j->queue_priority, j->queue_priority + M);
  std::vector<int64_t> submit(M, 0), runTs(M, 0);
  if (j->submit_time) submit.assign(j->submit_time, j->submit_time + M);
  if (j->run_timestamp) runTs.assign(j->run_timestamp, j->run_timestamp + M);
  h->jReq.assign(j->req, j->req + (size_t)M * R);
  int nc = c ? c->n : 0;
  h->C = std::max(nc, 1);
  h->clsTol.assign(h->C, {}); h->clsSel.assign(h->C, {}); h->clsAff.clear();
  if (c && c->has_affinity) h->clsAff.assign(h->C, {});
  for (int i = 0; i < nc; i++) {
    HAffinity aff;
    if (int prc = reqClassParse(h, c, i, h->clsTol[i], h->clsSel[i], aff)) return prc;
    if (aff.present) h->clsAff[i] = aff;
  }
  d.cfg.C = h->C;
  prof.lap("copy-in + classes");
  // scheduling-key shapes (podutils.go:52-72): (requirement class, priority class, requests)
  // (first occurrence numbers the shape; an open-addressing table over (class, priority class, requests) replaces an ordered map)
  h->jShape.assign(M, 0); h->shapeClass.clear(); h->shapeReq.clear(); h->shapePc.clear(); h->shapeRow.clear(); h->shapeTable.clear(); h->shapeHash.clear();
  std::vector<uint8_t> aligned(M, 1);
  bool anyAway = false;
  int maxQueue = -1;
  {
    size_t cap = 1024;
    std::vector<int32_t> table(cap, -1);
    auto hashOf = [&](int i) {
      uint64_t x = 0x9e3779b97f4a7c15ull ^ ((uint64_t)(uint32_t)h->jReqClass[i] << 32 | (uint32_t)h->jPc[i]);
      for (int r = 0; r < R; r++) { x ^= (uint64_t)h->jReq[(size_t)i * R + r]; x *= 0xff51afd7ed558ccdull; x ^= x >> 29; }
      return x;
    };
    auto same = [&](int sidx, int i) {
      if (h->shapeClass[sidx] != h->jReqClass[i] || h->shapePc[sidx] != h->jPc[i]) return false;
      for (int r = 0; r < R; r++) if (h->shapeReq[(size_t)sidx * R + r] != h->jReq[(size_t)i * R + r]) return false;
      return true;
    };
    std::vector<uint64_t> shapeHash;
    for (int i = 0; i < M; i++) {
      if (h->jReqClass[i] < 0 || h->jReqClass[i] >= h->C) return fail(h, ASCHED_ERR_INVALID, "req_class out of range");
      if (h->jPc[i] < 0 || h->jPc[i] >= h->npc) return fail(h, ASCHED_ERR_INVALID, "pc out of range");
      if (h->jNode[i] >= h->N && h->nodesSet) return fail(h, ASCHED_ERR_INVALID, "running job on unknown node");
      if (!h->pcAway[h->jPc[i]].empty()) anyAway = true;
      uint64_t hv = hashOf(i);
      size_t pos = hv & (cap - 1);
      while (table[pos] >= 0 && !(shapeHash[table[pos]] == hv && same(table[pos], i))) pos = (pos + 1) & (cap - 1);
      if (table[pos] < 0) {
        int32_t sidx = (int32_t)h->shapeClass.size();
        table[pos] = sidx;
        shapeHash.push_back(hv);
        h->shapeClass.push_back(h->jReqClass[i]); h->shapePc.push_back(h->jPc[i]); h->shapeRow.push_back(i);
        for (int r = 0; r < R; r++) h->shapeReq.push_back(h->jReq[(size_t)i * R + r]);
        if ((size_t)(sidx + 1) * 2 > cap) {  // keep the load factor under one half
          cap *= 4;
          table.assign(cap, -1);
          for (int32_t t = 0; t <= sidx; t++) { size_t p2 = shapeHash[t] & (cap - 1); while (table[p2] >= 0) p2 = (p2 + 1) & (cap - 1); table[p2] = t; }
          pos = hv & (cap - 1);
          while (table[pos] != sidx) pos = (pos + 1) & (cap - 1);
        }
      }
      h->jShape[i] = table[pos];
      for (int cix = 0; cix < h->K; cix++)
        if (h->jReq[(size_t)i * R + h->indexedCol[cix]] % h->indexedRes[cix]) aligned[i] = 0;
      maxQueue = std::max(maxQueue, h->jQueue[i]);
    }
  }
  prof.lap("shapes");
  d.cfg.hasAway = anyAway ? 1 : 0;
  h->S = (int)h->shapeClass.size(); d.cfg.S = h->S;
  h->shapeUnaligned.assign(h->S, 0);
  for (int i = 0; i < M; i++) if (!aligned[i]) h->shapeUnaligned[h->jShape[i]] = 1;
  deriveAwayRows(h, anyAway);
  // gangs: dense id per (queue, gang id), CSR of members (jobRepo.GetGangJobsByGangId)
  std::map<std::pair<int32_t, int32_t>, int32_t>& gmap = h->gangMap; gmap.clear();   // (kept: asched_jobs_append numbers new gangs behind these)
  h->jGangDense.assign(M, -1);
  for (int i = 0; i < M; i++) if (gangId[i] >= 0) {
    auto k = std::make_pair(h->jQueue[i], gangId[i]);
    auto it = gmap.find(k);
    if (it == gmap.end()) it = gmap.emplace(k, (int32_t)gmap.size()).first;
    h->jGangDense[i] = it->second;
  }
  h->G = (int)gmap.size(); d.cfg.G = h->G;
  std::vector<int32_t> gangOff(h->G + 2, 0), gangJobs;
  for (int i = 0; i < M; i++) if (h->jGangDense[i] >= 0) gangOff[h->jGangDense[i] + 1]++;
  for (int g = 0; g < h->G; g++) gangOff[g + 1] += gangOff[g];
  gangJobs.assign(gangOff[h->G], 0);
  { std::vector<int32_t> fill(gangOff.begin(), gangOff.end() - 1);
    for (int i = 0; i < M; i++) if (h->jGangDense[i] >= 0) gangJobs[fill[h->jGangDense[i]]++] = i; }
  gangOff[h->G + 1] = gangOff[h->G] + std::max(M, 1);  // scratch gang slot for schedule_many
  // uniformity label -> slot
  std::vector<int32_t> uniSlot(M, -1);
  h->jGangUniKey.assign(M, -1);
  for (int i = 0; i < M; i++) if (gangId[i] >= 0 && gangUni[i] >= 0) h->jGangUniKey[i] = gangUni[i];   // (the pricer groups nodes by the label itself)
  for (int i = 0; i < M; i++) if (gangId[i] >= 0 && gangUni[i] >= 0) {
    auto it = std::find(h->labelSlots.begin(), h->labelSlots.end(), gangUni[i]);
    uniSlot[i] = h->indexedLabels.count(gangUni[i]) && it != h->labelSlots.end() ? (int32_t)(it - h->labelSlots.begin()) : -2;
  }
  prof.lap("away rows + gangs");
  // pre-sorted job order: per queue, running jobs then queued jobs, each in SchedulingOrderCompare order (jobdb/comparison.go:49-107)
  int Qj = maxQueue + 1;
  // jobs are bucketed by queue (counting sort), then every queue's bucket is sorted on packed keys — queues are independent, so the
  // buckets are sorted on several host threads
  std::vector<int32_t> ord;
  {
    auto keyLess = [](const OrdKey& x, const OrdKey& y) {
      if (x.a != y.a) return x.a < y.a;
      if (x.b != y.b) return x.b < y.b;
      if (x.t1 != y.t1) return x.t1 < y.t1;
      if (x.t2 != y.t2) return x.t2 < y.t2;
      return x.idx < y.idx;
    };
    std::vector<size_t> off(Qj + 1, 0);
    for (int i = 0; i < M; i++) if (h->jQueue[i] >= 0) off[h->jQueue[i] + 1]++;
    for (int q = 0; q < Qj; q++) off[q + 1] += off[q];
    std::vector<OrdKey>& keys = h->stageKeys;
    keys.resize(off[Qj]);
    {
      std::vector<size_t> fill(off.begin(), off.end() - 1);
      for (int i = 0; i < M; i++) {
        int q = h->jQueue[i];
        if (q < 0) continue;
        bool active = h->jNode[i] >= 0;
        OrdKey k;
        // active run first; priority-class priority descending; queue priority ascending (comparison.go:49-79)
        k.a = ((uint64_t)(active ? 0 : 1) << 32) | (uint32_t)~((uint32_t)h->pcPriority[h->jPc[i]] ^ 0x80000000u);
        k.b = qprio[i];
        // both active: run timestamp, then submit time; otherwise submit time (:83-97); then the id order (:99-105)
        k.t1 = (uint64_t)(active ? runTs[i] : submit[i]) ^ (1ull << 63);
        k.t2 = (uint64_t)submit[i] ^ (1ull << 63);
        k.idx = i;
        keys[fill[q]++] = k;
      }
    }
    std::vector<int> byCount(Qj);
    for (int q = 0; q < Qj; q++) byCount[q] = q;
    std::sort(byCount.begin(), byCount.end(), [&](int x, int y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });  // big buckets first
    std::atomic<int> nextQ{0};
    auto work = [&] {
      for (;;) {
        int c = nextQ.fetch_add(1);
        if (c >= Qj) return;
        int q = byCount[c];
        std::sort(keys.begin() + off[q], keys.begin() + off[q + 1], keyLess);
      }
    };
    int T = keys.size() < 65536 ? 1 : hostThreads();
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    ord.resize(keys.size());
    for (size_t i = 0; i < keys.size(); i++) ord[i] = keys[i].idx;
  }
  prof.lap("scheduling-order sort");
  // market-driven pools: every job's rank under jobdb.MarketSchedulingOrderCompare (jobdb/comparison.go:113-170: priority class, bid price, active run first, run age,
  // submit time, id) over the whole job set, and the per-queue job order sorted by it (what InMemoryJobRepository holds on such a pool, pqs.go:292-295)
  std::vector<int32_t> mkOrd, mkRank;
  h->mkJobsBuilt = j->bid_price != nullptr || h->market.enabled;
  if (h->mkJobsBuilt) {
    std::vector<int32_t> all(M);
    for (int i = 0; i < M; i++) all[i] = i;
    const double* bid = j->bid_price;
    std::sort(all.begin(), all.end(), [&](int32_t a, int32_t b) {
      int32_t pa = h->pcPriority[h->jPc[a]], pb = h->pcPriority[h->jPc[b]];
      if (pa != pb) return pa > pb;
      double ba = bid ? bid[a] : 0.0, bb = bid ? bid[b] : 0.0;
      if (ba != bb) return ba > bb;
      bool aa = h->jNode[a] >= 0, ab = h->jNode[b] >= 0;
      if (aa || ab) { if (!ab) return true; if (!aa) return false; if (runTs[a] != runTs[b]) return runTs[a] < runTs[b]; }
      if (submit[a] != submit[b]) return submit[a] < submit[b];
      return a < b;
    });
    mkRank.resize(M);
    for (int i = 0; i < M; i++) mkRank[all[i]] = i;
    std::vector<size_t> off(Qj + 1, 0);
    for (int i = 0; i < M; i++) if (h->jQueue[i] >= 0) off[h->jQueue[i] + 1]++;
    for (int q = 0; q < Qj; q++) off[q + 1] += off[q];
    mkOrd.resize(off[Qj]);
    for (int i = 0; i < M; i++) { int q = h->jQueue[all[i]]; if (q >= 0) mkOrd[off[q]++] = all[i]; }   // stable bucketing of the sorted order: per queue, market order
  }
  std::vector<int32_t> ordOff(Qj + 2, 0);
  for (int i : ord) ordOff[h->jQueue[i] + 1]++;
  for (int q = 0; q < Qj; q++) ordOff[q + 1] += ordOff[q];
  ordOff[Qj + 1] = ordOff[Qj];
  d.jQueue = h->jobBufs.upload(h->jQueue); d.jPc = h->jobBufs.upload(h->jPc); d.jShape = h->jobBufs.upload(h->jShape);
  d.jGang = h->jobBufs.upload(h->jGangDense); d.jGangCard = h->jobBufs.upload(gangCard); d.jGangUni = h->jobBufs.upload(uniSlot);
  d.jNode0 = h->jobBufs.upload(h->jNode); d.jRunPrio = h->jobBufs.upload(h->jRunPrio);
  d.jAway = h->anyAway ? h->jobBufs.upload(h->jAway) : nullptr;
  d.jReq = h->jobBufs.upload(h->jReq); d.jAligned = h->jobBufs.upload(aligned);
  { std::vector<int64_t> lease(M); for (int i = 0; i < M; i++) lease[i] = runTs[i] / 1000000; d.jLeaseMs = h->jobBufs.upload(lease); }   // ns -> ms (optimiser job ages)
  d.gangOff = h->jobBufs.upload(gangOff); d.gangJobs = h->jobBufs.upload(gangJobs);
  d.ordAll = h->jobBufs.upload(ord);
  memset(&h->mk, 0, sizeof h->mk);
  if (h->mkJobsBuilt) {
    h->mk.ord = h->jobBufs.upload(mkOrd); h->mk.jRank = h->jobBufs.upload(mkRank);
    h->mk.jSubmit = h->jobBufs.upload(submit); h->mk.jRunTs = h->jobBufs.upload(runTs);
    if (j->bid_price) { std::vector<double> b(j->bid_price, j->bid_price + M); h->mk.jBid = h->jobBufs.upload(b); }
    h->mk.jobBillable = h->jobBufs.alloc<uint8_t>((size_t)M + 1);
  }
  h->ordQueues = Qj;
  {  // offsets padded so that any Q <= Qj+? can index them
    std::vector<int32_t> off(std::max(Qj, 1) + 4096 + 2, ordOff[Qj]);
    for (int q = 0; q <= Qj; q++) off[q] = ordOff[q];
    d.ordAllOff = h->jobBufs.upload(off);
    h->ordOffHost = off;
  }
  allocJobState(h, (size_t)M);
  allocGangState(h, (size_t)h->G, (size_t)gangOff[h->G + 1]);
  d.unfeasible = h->jobBufs.alloc<uint8_t>(std::max(h->S, 1)); d.unfeasibleReason = h->jobBufs.alloc<int32_t>(std::max(h->S, 1));
  h->jobCap = M; h->gangCap = h->G; h->gangArrCap = (size_t)gangOff[h->G + 1]; h->gangJobsCap = gangJobs.size(); h->gangOffCap = gangOff.size();
  h->ordCap = ord.size(); h->ordSpareCap = 0; h->ordOffCap = h->ordOffHost.size(); h->gangOffHost = gangOff;
  memset(h->jaStats, 0, sizeof h->jaStats); memset(h->jasStats, 0, sizeof h->jasStats); memset(h->jdStats, 0, sizeof h->jdStats); memset(h->jrStats, 0, sizeof h->jrStats); memset(h->rcStats, 0, sizeof h->rcStats); memset(h->jsStats, 0, sizeof h->jsStats); memset(h->caStats, 0, sizeof h->caStats);
  memset(h->scStats, 0, sizeof h->scStats);
  h->jobsSet = true; h->prepared = false;
  h->jQPrioHost.swap(qprio); h->jSubmitHost.swap(submit); h->jRunTsHost.swap(runTs);   // (asched_jobs_patch uploads them when it is first called; nothing is copied here)
  prof.lap("uploads + per-job state allocation");
  if (h->nodesSet) if (int lrc = layoutKeys(h)) return lrc;   // (a negative request on an indexed column needs the wide field layout; the keys themselves are rebuilt by CMD_UPSERT_RESET below)
  int rc = rebuildMasks(h);
  prof.lap("masks + fast structure (JobRec table)");
  if (rc) return rc;
  // job dynamic state: everything unbound until round_prepare (NodeDb-level tests bind explicitly)
  // (a standalone reset so that the NodeDb-level API works without a round)
  d.cfg.Q = 0;
  rc = runControl(h, CMD_UPSERT_RESET);
  if (rc) return rc;
  rc = runControl(h, CMD_RESET_JOBS);
  h->allocPristine = h->nodesSet;   // CMD_UPSERT_RESET put every plane back to its initial state (equalLevels describes it), the evicted table is empty
  h->evictedDirty = false;
  prof.lap("state reset launches");
  return rc;
}

// the first incremental call on a job table that is a patch or a reprioritise: the order-key inputs become resident as the host mirrors hold them, with the keep flags
// and the second order buffer (all in jobBufs: gone with the job table).  total: length of ordAll
static void jpMakeResident(asched* h, int total) {
  const size_t M = (size_t)h->M;
  h->jp.qprio = h->jobBufs.upload(h->jQPrioHost); h->jp.submit = h->jobBufs.upload(h->jSubmitHost); h->jp.runTs = h->jobBufs.upload(h->jRunTsHost);
  h->jp.keep = h->jobBufs.allocRaw<uint8_t>(h->jobCap); plat_memset(h->jp.keep, 1, M);
  h->jp.ordSpare = h->jobBufs.allocRaw<int32_t>(std::max<size_t>((size_t)total, h->ordCap)); h->ordSpareCap = std::max<size_t>((size_t)total, h->ordCap);   // (as long as the order: the two swap)
  h->jp.built = true;
}

// ---- what the two run-state calls share (asched_jobs_patch; asched_round_commit, whose entries are these plus the lists of the round)
// the entries a caller gives, checked before anything changes: nullptr, or the reason without the call's name (code: its error code).  nT grows by the entries that name
// a row of a queue >= 0.  h->jpSeen [M] is all zero on return but for what the caller marked (2) before: the rows another source of the same call names
static const char* jpCheckEntries(asched* h, int n, const int32_t* job, const int32_t* node, int& nT, int& code) {
  const int M = h->M;
  if (h->jpSeen.size() != (size_t)M) h->jpSeen.assign(M, 0);
  int seen = 0;
  const char* why = nullptr;
  for (int i = 0; i < n && !why; i++) {
    const int j = job[i];
    if (j < 0 || j >= M) { why = "a row outside the job table"; break; }
    if (h->jpSeen[j]) { why = h->jpSeen[j] == 2 ? "an extra row that the round's scheduled or preempted list names (send that change with a later jobs_patch)" : "a row named twice"; break; }
    h->jpSeen[j] = 1; seen = i + 1;
    if (node[i] < -1 || node[i] >= (h->nodesSet ? h->N : 0)) why = "node outside [-1, N)";   // (no node table: only -1)
    else if (node[i] >= 0 && h->jAway[j]) { why = "a cross-pool away row may only lose its run"; code = ASCHED_ERR_UNSUPPORTED; }
    else if (h->jQueue[j] >= 0) nT++;
  }
  for (int i = 0; i < seen; i++) h->jpSeen[job[i]] = 0;
  return why;
}
// one scratch block, kept and only ever grown: the rows of the n entries | node and priority of the nx uploaded ones | their timestamps | the sort array | the kept rows
struct JpPlan { int n, nx, nT, total, nb2; size_t oNode, oTs, oKeys, oKept, need; };
static JpPlan jpPlan(asched* h, int n, int nx, int nT) {
  JpPlan p;
  p.n = n; p.nx = nx; p.nT = nT;
  p.total = h->ordOffHost.empty() ? 0 : h->ordOffHost[std::min<size_t>((size_t)h->ordQueues, h->ordOffHost.size() - 1)];
  p.nb2 = n;
  if (nT > 0) { p.nb2 = JP_TILE; while (p.nb2 < n) p.nb2 <<= 1; }
  p.oNode = up256(sizeof(int32_t) * (size_t)n); p.oTs = p.oNode + up256(sizeof(int32_t) * 2 * (size_t)nx); p.oKeys = p.oTs + up256(sizeof(int64_t) * (size_t)nx);
  p.oKept = p.oKeys + (nT > 0 ? up256(sizeof(JpKey) * (size_t)p.nb2) : 0);
  p.need = p.oKept + (nT > 0 ? up256(sizeof(int32_t) * (size_t)p.total) : 0);
  return p;
}
// the host mirrors of the entries a caller gives (round_prepare's host aggregation path reads jNode); prio / ts nullptr: zeros
static void jpMirror(asched* h, int n, const int32_t* job, const int32_t* node, const int32_t* prio, const int64_t* ts) {
  for (int i = 0; i < n; i++) {
    const int j = job[i];
    h->jNode[j] = node[i]; h->jRunPrio[j] = prio ? prio[i] : 0; h->jRunTsHost[j] = ts ? ts[i] : 0;
  }
}
// after the mirrors hold the call's values, p.n > 0: the order-key inputs become resident with the first incremental call on the job table, the p.nx uploaded entries go
// into the scratch (prio / ts nullptr: zeros), and `a` describes the call to the platform layer
static void jpStage(asched* h, const JpPlan& p, JpArgs& a, int32_t*& keptBuf, const int32_t* job, const int32_t* node, const int32_t* prio, const int64_t* ts) {
  if (!h->jp.built) jpMakeResident(h, p.total);
  memset(&a, 0, sizeof a);
  a.M = h->M; a.n = p.n; a.nT = p.nT; a.total = p.total; a.nb2 = p.nb2;
  const size_t nx = (size_t)p.nx;
  int32_t *eJob = (int32_t*)h->jpScratch, *eNode = (int32_t*)(h->jpScratch + p.oNode), *ePrio = eNode + nx; int64_t* eTs = (int64_t*)(h->jpScratch + p.oTs);
  if (nx) {
    plat_h2d(eJob, job, sizeof(int32_t) * nx); plat_h2d(eNode, node, sizeof(int32_t) * nx);
    if (prio) plat_h2d(ePrio, prio, sizeof(int32_t) * nx); else plat_memset(ePrio, 0, sizeof(int32_t) * nx);
    if (ts) plat_h2d(eTs, ts, sizeof(int64_t) * nx); else plat_memset(eTs, 0, sizeof(int64_t) * nx);
  }
  a.pJob = eJob; a.pNode = eNode; a.pPrio = ePrio; a.pTs = eTs;
  a.keep = h->jp.keep; a.jQPrio = h->jp.qprio; a.jSubmit = h->jp.submit; a.jRunTs = h->jp.runTs;
  keptBuf = nullptr;
  if (p.nT > 0) { a.keys = (JpKey*)(h->jpScratch + p.oKeys); keptBuf = (int32_t*)(h->jpScratch + p.oKept); a.out = h->jp.ordSpare; }
}
// the platform layer ended well: the merged order is the order, and the pass times are the call's
static void jpSeated(asched* h, const JpPlan& p, const char* who) {
  if (p.nT > 0) { std::swap(h->dev.ordAll, h->jp.ordSpare); std::swap(h->ordCap, h->ordSpareCap); }
  plat_pass_ms(PASS_JP, h->jpMs);
  if (plat_pass_printed(PASS_JP))
    fprintf(stderr, "[asched %s] jobs %d entries %d in the order %d: scatter %.4f ms, remove %.4f ms, sort %.4f ms, merge %.4f ms\n", who, h->M, p.n, p.nT, h->jpMs[0], h->jpMs[1], h->jpMs[2], h->jpMs[3]);
}

// jobdb.Txn.Upsert for run-state changes (scheduling/scheduling_algo.go:280-283 with the jobs of :956-981; jobdb/jobdb.go:572-700): the named rows get a new active run
// or lose theirs, on the device (kernels_jobs_patch.h).  Leaves the handle as asched_jobs_set would have, given the table with those rows replaced — without the static
// masks, the JobRec upload, the sort of all jobs or a new fast structure: none of them depends on run state.
int32_t asched_jobs_patch(asched_t* h, int32_t n, const int32_t* job, const int32_t* node, const int32_t* scheduled_at_priority, const int64_t* run_timestamp) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  const int M = h->M;
  // ---- every refusal before anything changes
  if (!h->jobsSet || h->jQPrioHost.size() != (size_t)M || h->jSubmitHost.size() != (size_t)M || h->jRunTsHost.size() != (size_t)M || h->jNode.size() != (size_t)M)
    return fail(h, ASCHED_ERR_INVALID, "jobs_patch: no job table on this handle (jobs_set first)");
  if (n < 0 || (n > 0 && (!job || !node))) return fail(h, ASCHED_ERR_INVALID, "jobs_patch: bad arguments");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_patch: the job set carries the market order, which depends on run state too (jobs_set instead)");
  if (n > (1 << 29)) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_patch: more than 2^29 entries");
  int nT = 0, code = ASCHED_ERR_INVALID;
  if (const char* why = jpCheckEntries(h, n, job, node, nT, code)) return fail(h, code, std::string("jobs_patch: ") + why);
  // sized before anything changes: running out of device memory here is a refusal too
  const JpPlan p = jpPlan(h, n, n, nT);
  KeptBlock<char> scratch{h->jpBufs, h->jpScratch, h->jpScratchBytes};
  if (n > 0 && !scratch.grow(p.need)) return fail(h, ASCHED_ERR_DEVICE, "jobs_patch: out of device memory for the patch scratch; the handle is as it was");
  // ---- what jobs_set resets (the job table half patched).  evrSized stays, on purpose: a patch changes no size
  residentTouchJobs(h, false, true);
  Dev& d = h->dev;
  plat_pass_clear(PASS_JP, h->jpMs);
  if (n > 0) {
    jpMirror(h, n, job, node, scheduled_at_priority, run_timestamp);
    JpArgs a; int32_t* keptBuf = nullptr;
    jpStage(h, p, a, keptBuf, job, node, scheduled_at_priority, run_timestamp);   // first patch of this job table: the order-key inputs become resident (the run timestamps as patched above)
    int prc = plat_take_failure() ? -1 : plat_jobs_patch(d, a, keptBuf);
    if (prc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    jpSeated(h, p, "jobs_patch");
  }
  // job dynamic state: everything unbound until round_prepare, as at the end of jobs_set
  d.cfg.Q = 0;
  return resetDynamicState(h, M);
}

// the result of the round the handle holds, applied to the resident jobs with the caller's other run-state changes of the cycle (scheduling/scheduling_algo.go:276-285:
// txn.Upsert(preemptedJobs) / txn.Upsert(scheduledJobs), the jobs of :956-981): asched_jobs_patch of (the scheduled list ++ the preempted list ++ the extras) without
// the lists leaving the device (kernels_round_commit.h).  The host's mirrors follow the copies downloadResult left in pinned memory: nothing is read back.
int32_t asched_round_commit(asched_t* h, int64_t run_timestamp, int64_t run_timestamp_step, int32_t n_extra, const int32_t* job, const int32_t* node,
                            const int32_t* scheduled_at_priority, const int64_t* run_timestamp_extra) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  const int M = h->M, nx = n_extra;
  // ---- every refusal before anything changes
  if (!h->jobsSet || h->jQPrioHost.size() != (size_t)M || h->jSubmitHost.size() != (size_t)M || h->jRunTsHost.size() != (size_t)M || h->jNode.size() != (size_t)M)
    return fail(h, ASCHED_ERR_INVALID, "round_commit: no job table on this handle (jobs_set first)");
  if (nx < 0 || (nx > 0 && (!job || !node))) return fail(h, ASCHED_ERR_INVALID, "round_commit: bad arguments");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "round_commit: the job set carries the market order, which depends on run state too (jobs_set instead)");
  const int ns = h->resNs, np = h->resNp;
  if (!h->haveRoundResult || (ns + np > 0 && !h->resPin))
    return fail(h, ASCHED_ERR_INVALID, "round_commit: no round result on this handle (schedule_round first; every call that changes the handle drops the result)");
  if (h->roundExchanged) return fail(h, ASCHED_ERR_UNSUPPORTED, "round_commit: not after round_exchange (the lists on this handle are this replica's own round, not the resolved one)");
  if ((long long)nx + ns + np > (1 << 29)) return fail(h, ASCHED_ERR_UNSUPPORTED, "round_commit: more than 2^29 entries");
  const int n = nx + ns + np;
  const int32_t *sJob = h->resSJob, *sNode = h->resSNode, *sPrio = h->resSPrio, *pJob = h->resPJob;
  if (h->jpSeen.size() != (size_t)M) h->jpSeen.assign(M, 0);
  // the rows the result names: marked (2) while the extras are checked against them
  int nT = 0, code = ASCHED_ERR_INVALID, marked = 0;
  const char* why = nullptr;
  for (int i = 0; i < ns + np && !why; i++) {
    const int j = i < ns ? sJob[i] : pJob[i - ns];
    if (j < 0 || j >= M || h->jpSeen[j] || (i < ns && (sNode[i] < 0 || sNode[i] >= (h->nodesSet ? h->N : 0)))) { why = "the round result held does not describe this job table"; break; }
    h->jpSeen[j] = 2; marked = i + 1;
    if (i < ns && h->jAway[j]) { why = "a cross-pool away row may only lose its run"; code = ASCHED_ERR_UNSUPPORTED; }
    else if (h->jQueue[j] >= 0) nT++;
  }
  if (!why) why = jpCheckEntries(h, nx, job, node, nT, code);
  for (int i = 0; i < marked; i++) h->jpSeen[i < ns ? sJob[i] : pJob[i - ns]] = 0;
  if (why) return fail(h, code, std::string("round_commit: ") + why);
  // sized before anything changes: running out of device memory here is a refusal too
  const JpPlan p = jpPlan(h, n, nx, nT);
  KeptBlock<char> scratch{h->jpBufs, h->jpScratch, h->jpScratchBytes};
  if (n > 0 && !scratch.grow(p.need)) return fail(h, ASCHED_ERR_DEVICE, "round_commit: out of device memory for the scratch; the handle is as it was");
  // ---- what jobs_set resets (the job table half patched).  The lists stay where they are, on the device and in pinned memory: only haveRoundResult goes
  residentTouchJobs(h, false, true);
  Dev& d = h->dev;
  plat_pass_clear(PASS_JP, h->jpMs);
  const bool madeResident = n > 0 && !h->jp.built;
  if (n > 0) {
    jpMirror(h, nx, job, node, scheduled_at_priority, run_timestamp_extra);
    for (int i = 0; i < ns; i++) {
      const int j = sJob[i];
      h->jNode[j] = sNode[i]; h->jRunPrio[j] = sPrio[i]; h->jRunTsHost[j] = (int64_t)((uint64_t)run_timestamp + (uint64_t)i * (uint64_t)run_timestamp_step);
    }
    for (int i = 0; i < np; i++) { const int j = pJob[i]; h->jNode[j] = -1; h->jRunPrio[j] = 0; h->jRunTsHost[j] = 0; }
    RcArgs a; memset(&a, 0, sizeof a);
    int32_t* keptBuf = nullptr;
    jpStage(h, p, a.p, keptBuf, job, node, scheduled_at_priority, run_timestamp_extra);
    a.nx = nx; a.ns = ns; a.np = np; a.ts0 = run_timestamp; a.tsStep = run_timestamp_step; a.pJobW = (int32_t*)h->jpScratch;
    int prc = plat_take_failure() ? -1 : plat_round_commit(d, a, keptBuf);
    if (prc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    jpSeated(h, p, "round_commit");
  }
  { int32_t* t = h->rcStats;
    t[0] = ns; t[1] = np; t[2] = nx; t[3] = nT; t[4] = madeResident ? 1 : 0;
    t[5] = (int32_t)(h->jpMs[0] * 1000.0 + 0.5); t[6] = (int32_t)((h->jpMs[1] + h->jpMs[2]) * 1000.0 + 0.5); t[7] = (int32_t)(h->jpMs[3] * 1000.0 + 0.5); }
  // job dynamic state: everything unbound until round_prepare, as at the end of jobs_set
  d.cfg.Q = 0;
  return resetDynamicState(h, M);
}
int32_t asched_round_commit_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->rcStats[k];
  return 0;
}

// `armadactl reprioritize` for resident jobs (jobdb/reconciliation.go:198-200 records the requested priority, scheduler.go:1198-1199 applies it with job.WithPriority,
// jobdb/job.go:523; Txn.Upsert re-seats the job in its queue's sorted set, jobdb/jobdb.go:583-587 and :695-699): the named rows get a new queue priority, the second word
// of the order key (jobdb/comparison.go:70-79), on the device (kernels_jobs_reprioritise.h).  Leaves the handle as asched_jobs_set would have, given the table with
// queue_priority replaced in those rows.  Only ordAll depends on it: the scatter of this call, then the remove / sort / merge passes of the patch.
int32_t asched_jobs_reprioritise(asched_t* h, int32_t n, const int32_t* job, const uint32_t* queue_priority) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  const int M = h->M;
  // ---- every refusal before anything changes
  if (!h->jobsSet || h->jQPrioHost.size() != (size_t)M || h->jSubmitHost.size() != (size_t)M || h->jRunTsHost.size() != (size_t)M || h->jNode.size() != (size_t)M)
    return fail(h, ASCHED_ERR_INVALID, "jobs_reprioritise: no job table on this handle (jobs_set first)");
  if (n < 0 || (n > 0 && (!job || !queue_priority))) return fail(h, ASCHED_ERR_INVALID, "jobs_reprioritise: bad arguments");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_reprioritise: the job set carries the market order (jobs_set instead)");
  if (n > (1 << 29)) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_reprioritise: more than 2^29 entries");
  if (h->jpSeen.size() != (size_t)M) h->jpSeen.assign(M, 0);
  int seen = 0, nT = 0, nSame = 0;
  const char* why = nullptr;
  for (int i = 0; i < n; i++) {
    const int j = job[i];
    if (j < 0 || j >= M) { why = "jobs_reprioritise: a row outside the job table"; break; }
    if (h->jpSeen[j]) { why = "jobs_reprioritise: a row named twice"; break; }
    h->jpSeen[j] = 1; seen = i + 1;
    if (h->jQueue[j] >= 0) nT++;
    if (h->jQPrioHost[j] == queue_priority[i]) nSame++;
  }
  for (int i = 0; i < seen; i++) h->jpSeen[job[i]] = 0;
  if (why) return fail(h, ASCHED_ERR_INVALID, why);
  // the patch's scratch block, kept and only ever grown: the entries | the sort array | the kept rows.  Sized before anything changes: running out of device memory here is a refusal too
  const int total = h->ordOffHost.empty() ? 0 : h->ordOffHost[std::min<size_t>((size_t)h->ordQueues, h->ordOffHost.size() - 1)];
  int nb2 = n;
  if (nT > 0) { nb2 = JP_TILE; while (nb2 < n) nb2 <<= 1; }
  const size_t oKeys = up256(sizeof(int32_t) * 2 * (size_t)n), oKept = oKeys + (nT > 0 ? up256(sizeof(JpKey) * (size_t)nb2) : 0), need = oKept + (nT > 0 ? up256(sizeof(int32_t) * (size_t)total) : 0);
  KeptBlock<char> scratch{h->jpBufs, h->jpScratch, h->jpScratchBytes};
  if (n > 0 && !scratch.grow(need)) return fail(h, ASCHED_ERR_DEVICE, "jobs_reprioritise: out of device memory for the scratch; the handle is as it was");
  // ---- what jobs_set resets (the order half built).  evrSized stays, as in asched_jobs_patch and for its reason
  residentTouchJobs(h, false, true);
  Dev& d = h->dev;
  plat_pass_clear(PASS_JP, h->jpMs);
  const bool madeResident = n > 0 && !h->jp.built;
  if (n > 0) {
    // the host mirror: jobs_append and jobs_delete stage and squeeze it, and a later first build uploads it
    for (int i = 0; i < n; i++) h->jQPrioHost[job[i]] = queue_priority[i];
    if (!h->jp.built) jpMakeResident(h, total);   // first incremental call on this job table: the order-key inputs become resident (the priorities as replaced above)
    JrArgs a; memset(&a, 0, sizeof a);
    a.p.M = M; a.p.n = n; a.p.nT = nT; a.p.total = total; a.p.nb2 = nb2;
    int32_t* e32 = (int32_t*)h->jpScratch;
    plat_h2d(e32, job, sizeof(int32_t) * (size_t)n); plat_h2d(e32 + n, queue_priority, sizeof(uint32_t) * (size_t)n);
    a.p.pJob = e32; a.pQPrio = (const uint32_t*)(e32 + n);
    a.jQPrio = h->jp.qprio;
    a.p.keep = h->jp.keep; a.p.jQPrio = h->jp.qprio; a.p.jSubmit = h->jp.submit; a.p.jRunTs = h->jp.runTs;
    int32_t* keptBuf = nullptr;
    if (nT > 0) { a.p.keys = (JpKey*)(h->jpScratch + oKeys); keptBuf = (int32_t*)(h->jpScratch + oKept); a.p.out = h->jp.ordSpare; }
    int prc = plat_take_failure() ? -1 : plat_jobs_reprioritise(d, a, keptBuf);
    if (prc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    if (nT > 0) { std::swap(d.ordAll, h->jp.ordSpare); std::swap(h->ordCap, h->ordSpareCap); }
    plat_pass_ms(PASS_JP, h->jpMs);
    if (plat_pass_printed(PASS_JP))
      fprintf(stderr, "[asched jobs_reprioritise] jobs %d entries %d in the order %d: scatter %.4f ms, remove %.4f ms, sort %.4f ms, merge %.4f ms\n", M, n, nT, h->jpMs[0], h->jpMs[1], h->jpMs[2], h->jpMs[3]);
  }
  { int32_t* t = h->jrStats;
    t[0] = n; t[1] = nT; t[2] = nSame; t[3] = madeResident ? 1 : 0;
    for (int k = 0; k < 4; k++) t[4 + k] = (int32_t)(h->jpMs[k] * 1000.0 + 0.5); }
  // job dynamic state: everything unbound until round_prepare, as at the end of jobs_set
  d.cfg.Q = 0;
  return resetDynamicState(h, M);
}
int32_t asched_jobs_reprioritise_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->jrStats[k];
  return 0;
}

// ---- asched_jobs_append (kernels_jobs_append.h): syncState's upsert of the newly submitted jobs (scheduler.go:478-535; jobdb/jobdb.go:572-700, the insertion into the
// per-queue sorted set at :691-700).  Rows M .. M+m-1 behind the resident ones, on the device; the handle is left as asched_jobs_set of the concatenated table would
// leave it.  Two paths, chosen per call: every row's scheduling-key shape is already in the table — nothing jobs_set derives per shape changes, so no mask is rebuilt and
// the fast structure stays; or some row brings a new shape — the per-row work is the same and the shape-dependent tables are re-derived by the code jobs_set ends with.
// With asched_set_append_in_place on, the second case takes a third path where its conditions hold (DESIGN 3.16): nothing a new shape adds depends on the old rows — mask
// rows (kernels_shapes_append.h), perhaps a derived away class and a fit shape, two minima, its own rows' records — so the tables GROW, the records of the resident rows
// stay where they are, and the call ends like the first case.  Exact provided the key layout of the grown table is the one in force, which is checked first.
static uint64_t jaShapeHash(int32_t cls, int32_t pc, const int64_t* req, int R) {   // (jobs_set's hash over (requirement class, priority class, requests))
  uint64_t x = 0x9e3779b97f4a7c15ull ^ ((uint64_t)(uint32_t)cls << 32 | (uint32_t)pc);
  for (int r = 0; r < R; r++) { x ^= (uint64_t)req[r]; x *= 0xff51afd7ed558ccdull; x ^= x >> 29; }
  return x;
}
static void jaShapeTableBuild(asched* h, size_t room) {   // over the shapes the handle holds, with a load factor under one half for `room` shapes
  const int R = h->R; const size_t S = h->shapeClass.size();
  size_t cap = 1024; while (cap < 2 * (std::max(room, S) + 1)) cap *= 4;
  h->shapeTable.assign(cap, -1); h->shapeHash.resize(S);
  for (size_t s = 0; s < S; s++) {
    h->shapeHash[s] = jaShapeHash(h->shapeClass[s], h->shapePc[s], &h->shapeReq[s * R], R);
    size_t pos = h->shapeHash[s] & (cap - 1);
    while (h->shapeTable[pos] >= 0) pos = (pos + 1) & (cap - 1);
    h->shapeTable[pos] = (int32_t)s;
  }
}
// ---- what asched_jobs_append and asched_jobs_respec (kernels_jobs_respec.h) share: a call whose rows bring new shapes, or shapes without a resident row.  The state of
// one such call between its steps, then the steps in the order both calls take them: the shape lookup, what the rebuild would refuse, the in-place decision, the staged
// shape-dependent blocks, what fills them, the template records, and `undo` for a refusal after the lookup.  M0 / S0 / A0 / Cext0 / F0: rows, shapes, away rows, classes
// with the derived ones, and fit shapes before the call.
struct JaShapes {
  int M0 = 0, S0 = 0, A0 = 0, Cext0 = 0, F0 = 0;
  DevCfg cfgSaved; bool keyWideSaved = false, keyCoarseSaved = false;
  std::vector<int32_t> revived, shapeRowSaved;   // shapes without a resident row that this call gives one, and shapeRow as it was (for `undo`)
  bool mirrorsGrown = false;
  // the in-place path extends what buildFast left on the handle before it knows that every block can be had: `undo` takes it back
  bool fastGrown = false; std::vector<uint8_t> rowLiteralSaved; int64_t minFieldSaved[MAXK], minExtraSaved[MAXE];
  bool inPlace = false; int inWhy = 0;   // inWhy: why the rebuild is taken although the switch is on
  std::vector<int32_t> shapeClassExt1, rowTypeOff1, rowTypes1; std::vector<int64_t> shapeReqExt1; std::vector<uint64_t> classRows1;
  uint64_t* shapeMask1 = nullptr;   // the grown shape mask [old shape rows | new shape rows | old away rows | new away rows]: filled by plat_shapes_append
  void begin(asched* h) {
    M0 = h->M; S0 = h->S; A0 = (int)h->awayRowClass.size(); Cext0 = h->Cext; F0 = h->dev.f.F;
    cfgSaved = h->dev.cfg; keyWideSaved = h->keyWide; keyCoarseSaved = h->keyCoarse;
  }
};
// the shape (cls, pc, req) in the handle's shape table; one the table does not hold gets the next id, with firstRow as its first row
static int32_t jaShapeFind(asched* h, int32_t cls, int32_t pc, const int64_t* req, int32_t firstRow) {
  const int R = h->R;
  const uint64_t hv = jaShapeHash(cls, pc, req, R);
  size_t cap = h->shapeTable.size(), pos = hv & (cap - 1);
  auto same = [&](int32_t s) {
    if (h->shapeHash[s] != hv || h->shapeClass[s] != cls || h->shapePc[s] != pc) return false;
    for (int r = 0; r < R; r++) if (h->shapeReq[(size_t)s * R + r] != req[r]) return false;
    return true;
  };
  while (h->shapeTable[pos] >= 0 && !same(h->shapeTable[pos])) pos = (pos + 1) & (cap - 1);
  if (h->shapeTable[pos] >= 0) return h->shapeTable[pos];
  const int32_t s = (int32_t)h->shapeClass.size();
  h->shapeTable[pos] = s; h->shapeHash.push_back(hv);
  h->shapeClass.push_back(cls); h->shapePc.push_back(pc); h->shapeRow.push_back(firstRow); h->shapeUnaligned.push_back(0);
  for (int r = 0; r < R; r++) h->shapeReq.push_back(req[r]);
  if ((size_t)(s + 1) * 2 > cap) jaShapeTableBuild(h, (size_t)(s + 1) * 2);
  return s;
}
// a refusal after the shape lookup: the handle exactly as it was (the caller puts back what it wrote into the rows of jReq below M0)
static void jaShapesUndo(asched* h, JaShapes& g) {
  Dev& d = h->dev;
  const int S0 = g.S0, R = h->R, M = g.M0;
  if (g.fastGrown) {
    h->fsDelta.resize(S0); h->fsMin.resize(S0); h->fsNever.resize(S0); h->fitOf.resize(S0); h->fitTab.resize(g.F0);
    for (auto it = h->fitIds.begin(); it != h->fitIds.end();) it = it->second >= g.F0 ? h->fitIds.erase(it) : std::next(it);
    memcpy(h->fsMinField, g.minFieldSaved, sizeof g.minFieldSaved); memcpy(h->fsMinExtra, g.minExtraSaved, sizeof g.minExtraSaved);
    d.f.F = g.F0; h->rowLiteral = g.rowLiteralSaved;
  }
  if (!g.revived.empty()) h->shapeRow = g.shapeRowSaved;
  h->shapeClass.resize(S0); h->shapePc.resize(S0); h->shapeReq.resize((size_t)S0 * R); h->shapeRow.resize(S0); h->shapeUnaligned.resize(S0);
  h->shapeTable.clear(); h->shapeHash.clear();
  if (g.mirrorsGrown) {
    h->jReq.resize((size_t)M * R); h->M = M; h->S = S0;
    d.cfg = g.cfgSaved; h->keyWide = g.keyWideSaved; h->keyCoarse = g.keyCoarseSaved;
    deriveAwayRows(h, g.cfgSaved.hasAway != 0);
  }
}
// what the rebuild can refuse, checked on the host first: the key layout of the table with its new shapes (layoutKeys) and LIT_TMAX for a new row on the literal
// iteration path.  h->jReq, h->M and h->S are the table's after the call (g.mirrorsGrown).  0, or the code with the reason in why
static int jaShapesRefusal(asched* h, JaShapes& g, bool anyAway, std::string& why) {
  const int S1 = h->S;
  deriveAwayRows(h, anyAway);
  if (h->nodesSet) {
    if (int lrc = layoutKeys(h)) { why = h->err; return lrc; }
    for (int s = g.S0; s < S1; s++) {
      std::vector<int32_t> classes{h->shapeClass[s]};
      for (int k = h->awayRowOff[s]; k < h->awayRowOff[s + 1]; k++) classes.push_back(h->awayRowClass[k]);
      for (int32_t c : classes) {
        size_t nTypes = 0;
        for (size_t t = 0; t < h->types.size(); t++) if (h->types[t].numNodes > 0 && classMatchesType(h, c, h->types[t])) nTypes++;
        const bool literal = h->shapeUnaligned[s] || (nTypes > 1 && !(h->allocAligned && h->idRankMonotone));
        if (literal && nTypes > LIT_TMAX) { why = "a requirement class on the literal iteration path matches more than LIT_TMAX node types"; return ASCHED_ERR_UNSUPPORTED; }
      }
    }
  }
  return 0;
}
// the in-place path for new shapes (asched_set_append_in_place): decided before anything changes.  negNew: the call brings a negative request.  Sets g.inPlace or
// g.inWhy and, in place, extends the per-shape tables of buildFast; 0, or the code with the reason in why
static int jaInPlaceDecide(asched* h, JaShapes& g, bool anyAway, bool negNew, std::string& why) {
  Dev& d = h->dev;
  const int R = h->R, M = g.M0, S0 = g.S0, S1 = h->S, A1 = (int)h->awayRowClass.size(), Wm = d.cfg.W;
  const DevCfg& cfgSaved = g.cfgSaved;
  bool layoutSame = h->keyWide == g.keyWideSaved && h->keyCoarse == g.keyCoarseSaved && d.cfg.keyClamp == cfgSaved.keyClamp && d.cfg.idxBits == cfgSaved.idxBits &&
                    d.cfg.keyGuard == cfgSaved.keyGuard && d.cfg.keyWords == cfgSaved.keyWords;
  for (int c = 0; c < h->K; c++) layoutSame = layoutSame && d.cfg.keyLo[c] == cfgSaved.keyLo[c] && d.cfg.keyWidth[c] == cfgSaved.keyWidth[c] && d.cfg.keyShift[c] == cfgSaved.keyShift[c] &&
                                              d.cfg.indexedRes[c] == cfgSaved.indexedRes[c];
  if (M <= 0 || S0 <= 0) g.inWhy = 6;   // (buildFast's predicate can turn true)
  else if (!h->nodesSet || !h->dClassMask || !h->dShapeClass || !d.shapeMask || h->fitOf.size() != (size_t)S0 || h->fsDelta.size() != (size_t)S0) g.inWhy = 1;
  else if (!layoutSame) g.inWhy = 2;
  else if (anyAway && !cfgSaved.hasAway) g.inWhy = 3;
  else if (negNew && (d.f.structOk || d.f.cascadeFuse)) g.inWhy = 5;   // (buildFast's reqNonNeg: the structure and the fused pass go with the first negative request)
  else {
    // the row tables of the grown shape table, then per new shape what buildFast derives (it reads h->rowLiteral)
    g.shapeClassExt1 = h->shapeClass; g.shapeReqExt1 = h->shapeReq;
    for (int k = 0; k < A1; k++) {
      g.shapeClassExt1.push_back(h->awayRowClass[k]);
      for (int r = 0; r < R; r++) g.shapeReqExt1.push_back(h->shapeReq[(size_t)h->awayRowShape[k] * R + r]);
    }
    g.rowLiteralSaved = h->rowLiteral; memcpy(g.minFieldSaved, h->fsMinField, sizeof g.minFieldSaved); memcpy(g.minExtraSaved, h->fsMinExtra, sizeof g.minExtraSaved);
    g.fastGrown = true;
    if (int rrc = buildRowTables(h, g.shapeClassExt1, g.rowTypeOff1, g.rowTypes1)) { why = h->err; return rrc; }
    for (int s = S0; s < S1; s++) fastShapeAdd(h, s);
    if (d.f.structOk && d.f.F > SMAX) g.inWhy = 4;   // (the rebuild that follows derives all of it again)
    else g.inPlace = true;
  }
  if (g.inPlace) {
    // the rows of the derived away classes this call adds: ids behind the old ones (deriveAwayRows numbers them in shape order)
    g.classRows1.assign((size_t)(h->Cext - g.Cext0) * Wm, 0);
    for (int c = g.Cext0; c < h->Cext; c++)
      for (int n = 0; n < h->N; n++) if (classMatchesNode(h, c, n)) g.classRows1[(size_t)(c - g.Cext0) * Wm + (n >> 6)] |= 1ull << (n & 63);
  }
  return 0;
}
// the template of shape s among those of one call: its position in tplShape, added on first use (128 bytes a shape, not a row)
static int32_t jaTemplateOf(std::unordered_map<int32_t, int32_t>& tplOf, std::vector<int32_t>& tplShape, int32_t s) {
  auto it = tplOf.find(s);
  if (it == tplOf.end()) { it = tplOf.emplace(s, (int32_t)tplShape.size()).first; tplShape.push_back(s); }
  return it->second;
}
// the template records of those shapes, as buildFast would fill a row of each (gang, node and run are the row's own), into platform memory at dst
static void jaTemplatesUpload(asched* h, const std::vector<int32_t>& tplShape, void* dst) {
  const int R = h->R;
  std::vector<JobRec> tpl(tplShape.size());
  for (size_t t = 0; t < tpl.size(); t++) fastRecFill(h, tpl[t], tplShape[t], &h->shapeReq[(size_t)tplShape[t] * R], h->shapePc[tplShape[t]], -1, -1, 0);
  plat_h2d(dst, tpl.data(), sizeof(JobRec) * tpl.size());
}
// the shape-dependent blocks of a call with new shapes, staged before anything changes: the unfeasible-key arrays for S1 shapes and, in place, the grown mask tables
static void jaStageShapes(asched* h, JaShapes& g, StagedBlocks& sb) {
  Dev& d = h->dev;
  const int S1 = h->S, Sext0 = g.S0 + g.A0, Sext1 = S1 + (int)h->awayRowClass.size(), Wm = d.cfg.W;
  sb.stage(&h->jobBufs, &d.unfeasible, (size_t)S1, 0, nullptr, 0); sb.stage(&h->jobBufs, &d.unfeasibleReason, (size_t)S1 * 4, 0, nullptr, 0);
  if (!g.inPlace) return;
  if (Sext1 > Sext0) {
    sb.stage(&h->maskBufs, &g.shapeMask1, 8 * (size_t)Sext1 * Wm, 0, nullptr, -1, true);
    sb.stage(&h->maskBufs, &h->dShapeClass, 4 * g.shapeClassExt1.size(), 4 * g.shapeClassExt1.size(), g.shapeClassExt1.data(), 0);
    sb.stage(&h->maskBufs, &d.shapeReq, 8 * g.shapeReqExt1.size(), 8 * g.shapeReqExt1.size(), g.shapeReqExt1.data(), 0);
    sb.stage(&h->maskBufs, &d.awayRowOff, 4 * h->awayRowOff.size(), 4 * h->awayRowOff.size(), h->awayRowOff.data(), 0);
    sb.stage(&h->maskBufs, &d.rowLiteral, h->rowLiteral.size(), h->rowLiteral.size(), h->rowLiteral.data(), 0);
    sb.stage(&h->maskBufs, &d.rowTypeOff, 4 * g.rowTypeOff1.size(), 4 * g.rowTypeOff1.size(), g.rowTypeOff1.data(), 0);
    sb.stage(&h->maskBufs, &d.rowTypes, 4 * g.rowTypes1.size(), 4 * g.rowTypes1.size(), g.rowTypes1.data(), 0);
  }
  if (h->Cext > g.Cext0) sb.stage(&h->maskBufs, &h->dClassMask, 8 * (size_t)h->Cext * Wm, 8 * (size_t)g.Cext0 * Wm, nullptr, -1);   // (the old rows device to device; the new ones are uploaded below)
  if (d.f.structOk && d.f.F > g.F0) {
    sb.stage(&h->fastBufs, &d.shapeTab, sizeof(ShapeReq) * h->fitTab.size(), sizeof(ShapeReq) * h->fitTab.size(), h->fitTab.data(), 0);
    if (d.fitBits) sb.stage(&h->fastBufs, &d.fitBits, 8 * ((size_t)d.f.F * d.fitW + 64), 0, nullptr, 0);   // (scratch the next base build fills, as in asched_nodes_append)
  }
}
// in place, once the staged blocks are committed: the packed minima, the class-mask rows of the new derived classes and the new rows of the shape mask
// (plat_shapes_append; saScratch: platform memory for request / class / output row of each).  0, or -1 with the platform's error
static int jaInPlaceApply(asched* h, JaShapes& g, char* saScratch) {
  Dev& d = h->dev;
  const int R = h->R, S0 = g.S0, S1 = h->S, A0 = g.A0, A1 = (int)h->awayRowClass.size(), Wm = d.cfg.W;
  fastMinimaPack(h);
  if (const char* ms = getenv("ASCHED_SHAPE_MASK")) if (d.fitBits && ms[0] == '1') d.f.maskMode = d.f.F <= 64 ? 1 : d.f.F <= 128 ? 2 : 0;   // (buildFast's rule, for the grown F)
  if (h->Cext > g.Cext0) plat_h2d(h->dClassMask + (size_t)g.Cext0 * Wm, g.classRows1.data(), g.classRows1.size() * 8);
  if (g.shapeMask1) {
    const int nNew = (S1 - S0) + (A1 - A0);
    std::vector<int32_t> rowCls(nNew), rowOut(nNew); std::vector<int64_t> rowReq((size_t)nNew * R);
    for (int k = 0; k < nNew; k++) {
      const int row = k < S1 - S0 ? S0 + k : S1 + A0 + (k - (S1 - S0));
      rowOut[k] = row; rowCls[k] = g.shapeClassExt1[row];
      for (int r = 0; r < R; r++) rowReq[(size_t)k * R + r] = g.shapeReqExt1[(size_t)row * R + r];
    }
    int64_t* dReq = (int64_t*)saScratch; int32_t* dCls = (int32_t*)(dReq + (size_t)nNew * R);
    plat_h2d(dReq, rowReq.data(), rowReq.size() * 8); plat_h2d(dCls, rowCls.data(), (size_t)nNew * 4); plat_h2d(dCls + nNew, rowOut.data(), (size_t)nNew * 4);
    SaArgs sa; memset(&sa, 0, sizeof sa);
    sa.N = h->N; sa.Npad = d.cfg.Npad; sa.W = Wm; sa.R = R; sa.rows = nNew;
    sa.totalRes = d.totalRes; sa.classMask = h->dClassMask;
    sa.rowClass = dCls; sa.rowOut = dCls + nNew; sa.rowReq = dReq;
    sa.outMask = g.shapeMask1; sa.inMask = d.shapeMask;
    sa.copy0 = (long long)S0 * Wm; sa.src1 = (long long)S0 * Wm; sa.dst1 = (long long)S1 * Wm; sa.copy1 = (long long)A0 * Wm;
    int src = plat_take_failure() ? -1 : plat_shapes_append(d, sa);
    if (src) return -1;
    plat_pass_ms(PASS_SA, h->saMs);
    h->maskBufs.release(d.shapeMask);
    d.shapeMask = g.shapeMask1;
  }
  return 0;
}
int32_t asched_jobs_append(asched_t* h, const asched_jobs* rows) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  const int M = h->M, R = h->R;
  Dev& d = h->dev;
  // ---- every refusal before anything changes
  if (!h->jobsSet || h->jQPrioHost.size() != (size_t)M || h->jSubmitHost.size() != (size_t)M || h->jRunTsHost.size() != (size_t)M || h->jNode.size() != (size_t)M)
    return fail(h, ASCHED_ERR_INVALID, "jobs_append: no job table on this handle (jobs_set first)");
  if (!rows || rows->m < 0) return fail(h, ASCHED_ERR_INVALID, "jobs_append: bad arguments");
  const int m = rows->m;
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_append: the job set carries the market order, which ranks every job against every other (jobs_set instead)");
  if (m > 0 && !rows->req) return fail(h, ASCHED_ERR_INVALID, "jobs_append: req is missing");
  if (m > 0 && rows->bid_price) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_append: bid prices belong to the market order (jobs_set instead)");
  if ((long long)M + m > (1ll << 30)) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_append: more than 2^30 rows");
  const int M1 = M + m, S0 = h->S, G0 = h->G;
  std::vector<int32_t> aQueue(m), aPc(m), aCls(m), aShape(m), aGang(m, -1), aGangCard(m, 1), aGangUni(m, -1), aSrc(m, -1), aUniKey(m, -1);
  std::vector<uint8_t> aAligned(m, 1);
  std::map<std::pair<int32_t, int32_t>, int32_t> newGangs;
  int nT = 0, maxQueue = -1;
  bool anyAway = d.cfg.hasAway != 0;
  for (int i = 0; i < m; i++) {
    const int q = rows->queue ? rows->queue[i] : 0, pc = rows->pc ? rows->pc[i] : 0, cls = rows->req_class ? rows->req_class[i] : 0;
    if (cls < 0 || cls >= h->C) return fail(h, ASCHED_ERR_INVALID, "jobs_append: req_class out of range (the requirement classes are those of the last jobs_set)");
    if (pc < 0 || pc >= h->npc) return fail(h, ASCHED_ERR_INVALID, "jobs_append: pc out of range");
    if (q < -1) return fail(h, ASCHED_ERR_INVALID, "jobs_append: a queue below -1");
    if ((rows->node && rows->node[i] != -1) || (rows->scheduled_at_priority && rows->scheduled_at_priority[i] != 0) || (rows->run_timestamp && rows->run_timestamp[i] != 0))
      return fail(h, ASCHED_ERR_INVALID, "jobs_append: a row has a run (append the queued job, then jobs_patch gives it its run)");
    if (rows->away && rows->away[i]) return fail(h, ASCHED_ERR_INVALID, "jobs_append: a row is flagged away (a cross-pool away job is a running job: jobs_set)");
    aQueue[i] = q; aPc[i] = pc; aCls[i] = cls;
    if (q >= 0) nT++;
    maxQueue = std::max(maxQueue, q);
    if (!h->pcAway[pc].empty()) anyAway = true;
    const int32_t gid = rows->gang_id ? rows->gang_id[i] : -1;
    if (rows->gang_cardinality) aGangCard[i] = rows->gang_cardinality[i];
    const int32_t uni = rows->gang_uniformity_label ? rows->gang_uniformity_label[i] : -1;
    if (gid >= 0) {
      auto key = std::make_pair((int32_t)q, gid);
      if (h->gangMap.count(key)) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_append: a row joins a gang that already has rows in the table (a gang is submitted in one piece; jobs_set instead)");
      auto it = newGangs.find(key);
      if (it == newGangs.end()) it = newGangs.emplace(key, G0 + (int32_t)newGangs.size()).first;
      aGang[i] = it->second;
      if (uni >= 0) {
        aUniKey[i] = uni;
        auto ls = std::find(h->labelSlots.begin(), h->labelSlots.end(), uni);
        aGangUni[i] = h->indexedLabels.count(uni) && ls != h->labelSlots.end() ? (int32_t)(ls - h->labelSlots.begin()) : -2;
      }
    }
    for (int c = 0; c < h->K; c++) if (rows->req[(size_t)i * R + h->indexedCol[c]] % h->indexedRes[c]) aAligned[i] = 0;
  }
  const int G1 = G0 + (int)newGangs.size();
  // the shape of every row: a hash over the shapes the handle holds; new shapes get the next ids in order of first occurrence (undone by `undo` on a later refusal)
  if (m > 0 && h->shapeTable.empty()) jaShapeTableBuild(h, (size_t)S0);
  JaShapes g; g.begin(h);
  std::vector<int32_t>& revived = g.revived; std::vector<int32_t>& shapeRowSaved = g.shapeRowSaved;
  for (int i = 0; i < m; i++) {
    aShape[i] = jaShapeFind(h, aCls[i], aPc[i], rows->req + (size_t)i * R, M + i);
    if (!aAligned[i]) h->shapeUnaligned[aShape[i]] = 1;   // (a property of the shape: a resident shape's flag is already what this row says)
    if (aShape[i] < S0) {
      int32_t& first = h->shapeRow[aShape[i]];
      if (first < 0) { if (revived.empty()) shapeRowSaved = h->shapeRow; revived.push_back(aShape[i]); first = M + i; }   // asched_jobs_delete emptied the shape: no resident row to copy a JobRec from
      else if (first < M) aSrc[i] = first;
    }
  }
  const int S1 = (int)h->shapeClass.size();
  const bool newShapes = S1 > S0 || !revived.empty();   // (a revived shape takes the path of a new one: the records are rebuilt from the mirrors, DESIGN 3.12)
  const int Cext0 = g.Cext0, A0 = g.A0;   // derived classes and away rows before the call
  auto undo = [&]() { if (newShapes) jaShapesUndo(h, g); };   // a refusal after the shape lookup: the handle exactly as it was
  if (newShapes) {
    // what the rebuild can refuse, checked on the host first: the key layout of the grown table (layoutKeys) and LIT_TMAX for a new row on the literal iteration path
    h->jReq.insert(h->jReq.end(), rows->req, rows->req + (size_t)m * R); h->M = M1; h->S = S1; g.mirrorsGrown = true;
    std::string why;
    if (int rrc = jaShapesRefusal(h, g, anyAway, why)) { undo(); return fail(h, rrc, "jobs_append: " + why); }
  }
  // ---- the in-place path for new shapes (asched_set_append_in_place): decided here, before anything changes.  inWhy: why the rebuild is taken although the switch is on
  bool& inPlace = g.inPlace; int& inWhy = g.inWhy;
  const int A1 = (int)h->awayRowClass.size(), Sext0 = S0 + A0, Sext1 = S1 + A1;
  std::vector<int32_t> tplShape, aTpl;
  if (newShapes && h->appendInPlace) {
    bool negNew = false;
    for (size_t k = 0; k < (size_t)m * R && !negNew; k++) negNew = rows->req[k] < 0;
    std::string why;
    if (int rrc = jaInPlaceDecide(h, g, anyAway, negNew, why)) { undo(); return fail(h, rrc, "jobs_append: " + why); }
  }
  if (inPlace) {
    // one template record per shape without a resident row below M (new or revived): every row of such a shape has aSrc < 0
    if (d.f.structOk && d.jrec) {
      std::unordered_map<int32_t, int32_t> tplOf;
      aTpl.assign(m, -1);
      for (int i = 0; i < m; i++) if (aSrc[i] < 0) aTpl[i] = jaTemplateOf(tplOf, tplShape, aShape[i]);
    }
  }
  const size_t nTpl = tplShape.size();
  const int nNewRows = inPlace ? (S1 - S0) + (A1 - A0) : 0;
  // ---- sizes, and every new device block before anything changes: running out of device memory here is a refusal too
  const int total = h->ordOffHost.empty() ? 0 : h->ordOffHost[std::min<size_t>((size_t)h->ordQueues, h->ordOffHost.size() - 1)];
  const int total1 = total + nT;
  const int Qj1 = std::max(h->ordQueues, maxQueue + 1);
  int nb2 = m;
  if (nT > 0) { nb2 = JP_TILE; while (nb2 < m) nb2 <<= 1; }
  const bool grow = (size_t)M1 > h->jobCap;
  const size_t cap1 = grow ? std::max<size_t>((size_t)M1, h->jobCap + (h->jobCap + 3) / 4) : h->jobCap;   // max(M + m, 1.25 x capacity)
  // the new gangs' CSR tail
  std::vector<int32_t> gangOff1, gangTail;
  if (m > 0) {
    if (h->gangOffHost.size() != (size_t)G0 + 2) { undo(); return fail(h, ASCHED_ERR_INVALID, "jobs_append: no job table on this handle (jobs_set first)"); }
    gangOff1.assign(h->gangOffHost.begin(), h->gangOffHost.begin() + G0 + 1);
    gangOff1.resize((size_t)G1 + 2, 0);
    std::vector<int32_t> cnt(G1 - G0, 0);
    for (int i = 0; i < m; i++) if (aGang[i] >= 0) cnt[aGang[i] - G0]++;
    for (int g = G0; g < G1; g++) gangOff1[g + 1] = gangOff1[g] + cnt[g - G0];
    gangTail.assign((size_t)(gangOff1[G1] - gangOff1[G0]), 0);
    { std::vector<int32_t> fill2(gangOff1.begin() + G0, gangOff1.begin() + G1);
      for (int i = 0; i < m; i++) if (aGang[i] >= 0) gangTail[(size_t)(fill2[aGang[i] - G0]++ - gangOff1[G0])] = M + i; }
    gangOff1[G1 + 1] = gangOff1[G1] + std::max(M1, 1);   // scratch gang slot for schedule_many
  }
  const size_t o64 = up256(sizeof(int32_t) * 8 * (size_t)m), oReq = o64 + up256(sizeof(int64_t) * (size_t)m), oAl = oReq + up256(sizeof(int64_t) * (size_t)m * R), oKeys = oAl + up256((size_t)m),
               oTplIdx = oKeys + (nT > 0 ? up256(sizeof(JpKey) * (size_t)nb2) : 0), oTpl = oTplIdx + (nTpl ? up256(sizeof(int32_t) * (size_t)m) : 0),
               oSa = oTpl + up256(sizeof(JobRec) * nTpl), need = oSa + up256((size_t)nNewRows * (8 + 8 * (size_t)R));   // (the in-place path for new shapes: each row's template, the template records, and request / class / output row of the new mask rows)
  KeptBlock<char> scratch{h->jpBufs, h->jpScratch, h->jpScratchBytes};
  if (m > 0 && !scratch.tryGrow(need)) { undo(); return fail(h, ASCHED_ERR_DEVICE, "jobs_append: out of device memory for the append scratch; the handle is as it was"); }
  // each staged block is one device array of the job table that moves into a larger (or first) block: allocated before anything changes, filled and swapped in afterwards
  StagedBlocks sb;
  const bool buildJp = m > 0 && !h->jp.built;
  const size_t gangOffCap1 = (size_t)G1 + 2 > h->gangOffCap ? std::max<size_t>((size_t)G1 + 2, h->gangOffCap + h->gangOffCap / 4) : h->gangOffCap;
  const size_t ordOffCap1 = std::max(h->ordOffCap, (size_t)std::max(Qj1, 1) + 4096 + 2);   // (the queue count outgrew the 4 096 padding)
  const bool growRec = grow && d.f.structOk && d.jrec && (!newShapes || inPlace);   // (a new shape off the in-place path: rebuildMasks -> buildFast allocates the fast structure at the new capacity)
  int32_t* ordTarget = nullptr; int32_t* ordNext = nullptr;
  if (m > 0) {
    if (grow) {
      const size_t c = cap1, o = (size_t)M;
      sb.stage(&h->jobBufs, &d.jQueue, c * 4, o * 4, nullptr, -1); sb.stage(&h->jobBufs, &d.jPc, c * 4, o * 4, nullptr, -1); sb.stage(&h->jobBufs, &d.jShape, c * 4, o * 4, nullptr, -1);
      sb.stage(&h->jobBufs, &d.jGang, c * 4, o * 4, nullptr, -1); sb.stage(&h->jobBufs, &d.jGangCard, c * 4, o * 4, nullptr, -1); sb.stage(&h->jobBufs, &d.jGangUni, c * 4, o * 4, nullptr, -1);
      sb.stage(&h->jobBufs, &d.jNode0, c * 4, o * 4, nullptr, -1); sb.stage(&h->jobBufs, &d.jRunPrio, c * 4, o * 4, nullptr, -1);
      if (d.jAway) sb.stage(&h->jobBufs, &d.jAway, c, o, nullptr, -1);
      sb.stage(&h->jobBufs, &d.jReq, c * 8 * R, o * 8 * R, nullptr, -1); sb.stage(&h->jobBufs, &d.jAligned, c, o, nullptr, -1); sb.stage(&h->jobBufs, &d.jLeaseMs, c * 8, o * 8, nullptr, -1);
      if (growRec) {
        sb.stage(&h->fastBufs, &d.jrec, sizeof(JobRec) * c, sizeof(JobRec) * o, nullptr, -1);
        sb.stage(&h->fastBufs, &d.evIdxByPos, c * 4, 0, nullptr, 0); sb.stage(&h->fastBufs, &d.evKey, sizeof(EvKey) * c, 0, nullptr, 0); sb.stage(&h->fastBufs, &d.evCheap, 4104 + c + 8, 0, nullptr, 0);
      }
    }
    if (buildJp) {   // first append or patch of this job table: the order-key inputs become resident
      sb.stage(&h->jobBufs, &h->jp.qprio, cap1 * 4, (size_t)M * 4, h->jQPrioHost.data(), -1); sb.stage(&h->jobBufs, &h->jp.submit, cap1 * 8, (size_t)M * 8, h->jSubmitHost.data(), -1);
      sb.stage(&h->jobBufs, &h->jp.runTs, cap1 * 8, (size_t)M * 8, h->jRunTsHost.data(), -1); sb.stage(&h->jobBufs, &h->jp.keep, cap1, 0, nullptr, 1);
    } else if (grow) {
      sb.stage(&h->jobBufs, &h->jp.qprio, cap1 * 4, (size_t)M * 4, nullptr, -1); sb.stage(&h->jobBufs, &h->jp.submit, cap1 * 8, (size_t)M * 8, nullptr, -1);
      sb.stage(&h->jobBufs, &h->jp.runTs, cap1 * 8, (size_t)M * 8, nullptr, -1); sb.stage(&h->jobBufs, &h->jp.keep, cap1, 0, nullptr, 1);
    }
    // the two order buffers (they swap): the merge's target and the spare it leaves must both hold the grown order
    if (h->ordSpareCap < (size_t)total1 || !h->jp.ordSpare) sb.stage(&h->jobBufs, &ordTarget, cap1 * 4, 0, nullptr, -1, true);
    if (h->ordCap < (size_t)total1) sb.stage(&h->jobBufs, &ordNext, cap1 * 4, 0, nullptr, -1, true);
    if ((size_t)gangOff1[G1] > h->gangJobsCap) sb.stage(&h->jobBufs, &d.gangJobs, std::max<size_t>((size_t)gangOff1[G1], h->gangJobsCap + h->gangJobsCap / 4) * 4, (size_t)gangOff1[G0] * 4, nullptr, -1);
    if (gangOffCap1 > h->gangOffCap) sb.stage(&h->jobBufs, &d.gangOff, gangOffCap1 * 4, 0, nullptr, -1);
    if (ordOffCap1 > h->ordOffCap) sb.stage(&h->jobBufs, &d.ordAllOff, ordOffCap1 * 4, 0, nullptr, -1);
  }
  // the per-job and per-gang state of a round: allocated fresh (zeroed) where the capacity grows, as jobs_set allocates it
  const size_t gangJobsCap1 = m > 0 && (size_t)gangOff1[G1] > h->gangJobsCap ? std::max<size_t>((size_t)gangOff1[G1], h->gangJobsCap + h->gangJobsCap / 4) : h->gangJobsCap;
  const bool growGang = m > 0 && ((size_t)G1 > h->gangCap || (size_t)gangOff1[G1] + (size_t)std::max(M1, 1) > h->gangArrCap);
  const size_t gangCap1 = growGang ? std::max<size_t>((size_t)G1, h->gangCap + (h->gangCap + 3) / 4) : h->gangCap;
  const size_t gangArrCap1 = growGang ? std::max<size_t>(gangJobsCap1 + std::max<size_t>(cap1, 1), (size_t)gangOff1[G1] + (size_t)std::max(M1, 1)) : h->gangArrCap;
  if (growGang) {
    sb.stage(&h->jobBufs, &d.gangSeen, (gangCap1 + 1) * 4, 0, nullptr, 0); sb.stage(&h->jobBufs, &d.gangArr, gangArrCap1 * 4, 0, nullptr, 0);
    sb.stage(&h->jobBufs, &d.gangTotal, (gangCap1 + 1) * (size_t)R * 8, 0, nullptr, 0); sb.stage(&h->jobBufs, &d.gangAllEvicted, gangCap1 + 1, 0, nullptr, 0);
  }
  if (newShapes) jaStageShapes(h, g, sb);   // the unfeasible-key arrays for S1 shapes and, in place, the grown mask tables
  if (grow) {
    const size_t c = cap1;
    void* s32[] = {&d.schedAtPrio, &d.jobNode, &d.jobCutoff, &d.optGhost, &d.jcAssigned, &d.jcReason, &d.pcNode, &d.pcSap, &d.pcPap, &d.pcMethod, &d.jcGangCard, &d.jcUniValue, &d.jcStagedBy, &d.jcPreSib,
                   &d.preemptedNode, &d.evList, &d.evTabJob, &d.evIndexOfJob, &d.fairEnt, &d.fairEntJob, &d.preList, &d.resJob, &d.resNode, &d.resPrio, &d.resMethod, &d.resPreJob, &d.resPreNode};
    void* s8[] = {&d.jobEvictedOnNode, &d.jobFlags, &d.optSched, &d.optPre, &d.jcEvicted, &d.jcHasPctx, &d.jcPreempted, &d.inPreempted, &d.inScheduled, &d.inSchedAndEvicted, &d.evTabAlive, &d.evFlag};
    for (void* sl : s32) sb.stage(&h->jobBufs, sl, c * 4, 0, nullptr, 0);
    for (void* sl : s8) sb.stage(&h->jobBufs, sl, c, 0, nullptr, 0);
    sb.stage(&h->jobBufs, &d.evSortKey, (c + 1) * 4, 0, nullptr, 0);
  }
  if (!sb.allocate()) {
    scratch.drop();
    undo();
    return fail(h, ASCHED_ERR_DEVICE, "jobs_append: out of device memory for the grown job table; the handle is as it was");
  }
  // ---- what jobs_set resets (the job table half appended).  A new shape off the in-place path ends with rebuildMasks: the fast structure goes
  residentTouchJobs(h, newShapes && !inPlace);
  plat_pass_clear(PASS_JA, h->jaMs);
  plat_pass_clear(PASS_SA, h->saMs);
  scratch.adopt();
  if (m > 0) {
    // the blocks: copies and fills queued on the handle's stream, the old blocks released once they are through
    sb.fill();
    plat_sync();
    sb.commit();
    h->jp.built = true;
    h->jobCap = cap1; h->gangCap = gangCap1; h->gangArrCap = gangArrCap1; h->gangJobsCap = gangJobsCap1;
    h->gangOffCap = gangOffCap1; h->ordOffCap = ordOffCap1;
    // the host mirrors
    h->jQueue.insert(h->jQueue.end(), aQueue.begin(), aQueue.end()); h->jPc.insert(h->jPc.end(), aPc.begin(), aPc.end()); h->jReqClass.insert(h->jReqClass.end(), aCls.begin(), aCls.end());
    h->jShape.insert(h->jShape.end(), aShape.begin(), aShape.end()); h->jNode.resize(M1, -1); h->jRunPrio.resize(M1, 0); h->jGangDense.insert(h->jGangDense.end(), aGang.begin(), aGang.end());
    h->jAway.resize(M1, 0); h->jGangUniKey.insert(h->jGangUniKey.end(), aUniKey.begin(), aUniKey.end());
    if (!g.mirrorsGrown) h->jReq.insert(h->jReq.end(), rows->req, rows->req + (size_t)m * R);
    std::vector<uint32_t> aQPrio(m, 0); std::vector<int64_t> aSubmit(m, 0);
    if (rows->queue_priority) aQPrio.assign(rows->queue_priority, rows->queue_priority + m);
    if (rows->submit_time) aSubmit.assign(rows->submit_time, rows->submit_time + m);
    h->jQPrioHost.insert(h->jQPrioHost.end(), aQPrio.begin(), aQPrio.end()); h->jSubmitHost.insert(h->jSubmitHost.end(), aSubmit.begin(), aSubmit.end()); h->jRunTsHost.resize(M1, 0);
    for (auto& g : newGangs) h->gangMap.insert(g);
    h->gangOffHost = gangOff1;
    h->M = M1; h->G = G1; h->S = S1; d.cfg.M = M1; d.cfg.G = G1; d.cfg.S = S1; d.cfg.hasAway = anyAway ? 1 : 0;
    // the per-row inputs: the only upload proportional to anything
    int32_t* e32 = (int32_t*)h->jpScratch; const size_t mm = (size_t)m;
    const std::vector<int32_t>* cols[7] = {&aQueue, &aPc, &aShape, &aGang, &aGangCard, &aGangUni, &aSrc};
    for (int k = 0; k < 7; k++) plat_h2d(e32 + k * mm, cols[k]->data(), mm * 4);
    plat_h2d(e32 + 7 * mm, aQPrio.data(), mm * 4);
    plat_h2d(h->jpScratch + o64, aSubmit.data(), mm * 8); plat_h2d(h->jpScratch + oReq, rows->req, mm * 8 * R); plat_h2d(h->jpScratch + oAl, aAligned.data(), mm);
    if (inPlace && jaInPlaceApply(h, g, h->jpScratch + oSa)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    JaArgs a; memset(&a, 0, sizeof a);
    a.M = M; a.m = m; a.nb2 = nb2; a.R = R; a.writeRec = ((!newShapes || inPlace) && d.f.structOk && d.jrec) ? 1 : 0;
    if (inPlace && nTpl) {
      plat_h2d(h->jpScratch + oTplIdx, aTpl.data(), (size_t)m * 4); jaTemplatesUpload(h, tplShape, h->jpScratch + oTpl);
      a.tpl = (const JobRec*)(h->jpScratch + oTpl); a.aTpl = (const int32_t*)(h->jpScratch + oTplIdx);
    }
    a.aQueue = e32; a.aPc = e32 + mm; a.aShape = e32 + 2 * mm; a.aGang = e32 + 3 * mm; a.aGangCard = e32 + 4 * mm; a.aGangUni = e32 + 5 * mm; a.aSrc = e32 + 6 * mm;
    a.aQPrio = (const uint32_t*)(e32 + 7 * mm); a.aSubmit = (const int64_t*)(h->jpScratch + o64); a.aReq = (const int64_t*)(h->jpScratch + oReq); a.aAligned = (const uint8_t*)(h->jpScratch + oAl);
    a.jQPrio = h->jp.qprio; a.jSubmit = h->jp.submit;
    a.p.M = M1; a.p.n = 0; a.p.nb2 = nb2; a.p.nT = nT; a.p.nKept = total; a.p.total = total1;
    a.p.keep = h->jp.keep; a.p.jQPrio = h->jp.qprio; a.p.jSubmit = h->jp.submit; a.p.jRunTs = h->jp.runTs;
    int32_t* target = ordTarget ? ordTarget : h->jp.ordSpare;
    if (nT > 0) { a.p.keys = (JpKey*)(h->jpScratch + oKeys); a.p.kept = d.ordAll; a.p.out = target; }
    int prc = plat_take_failure() ? -1 : plat_jobs_append(d, a);
    if (prc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    plat_pass_ms(PASS_JA, h->jaMs);
    // the order buffers: the target becomes the order; the spare is the old order where that is long enough, else the second new block
    { int32_t* oldAll = d.ordAll; int32_t* oldSpare = h->jp.ordSpare;
      const size_t oldAllCap = h->ordCap, oldSpareCap = h->ordSpareCap;
      if (nT > 0) {
        d.ordAll = target; h->ordCap = ordTarget ? cap1 : oldSpareCap;
        if (ordTarget && oldSpare) h->jobBufs.release(oldSpare);
        if (ordNext) { h->jp.ordSpare = ordNext; h->ordSpareCap = cap1; h->jobBufs.release(oldAll); }
        else { h->jp.ordSpare = oldAll; h->ordSpareCap = oldAllCap; }
      } else {   // the order stays; the spare is whatever is long enough
        if (ordTarget) { if (oldSpare) h->jobBufs.release(oldSpare); h->jp.ordSpare = ordTarget; h->ordSpareCap = cap1; }
        if (ordNext) { h->jobBufs.release(ordNext); }
      } }
    if (gangTail.size()) plat_h2d(d.gangJobs + gangOff1[G0], gangTail.data(), gangTail.size() * 4);
    plat_h2d(d.gangOff, gangOff1.data(), gangOff1.size() * 4);
    { std::vector<int32_t> off((size_t)std::max(Qj1, 1) + 4096 + 2, total1), add((size_t)Qj1 + 2, 0);
      for (int i = 0; i < m; i++) if (aQueue[i] >= 0) add[(size_t)aQueue[i] + 1]++;
      for (int q = 0; q <= Qj1; q++) {
        if (q > 0) add[q] += add[q - 1];   // new rows of the queues below q
        off[q] = ((size_t)q < h->ordOffHost.size() && q <= h->ordQueues ? h->ordOffHost[q] : total) + add[q];
      }
      plat_h2d(d.ordAllOff, off.data(), off.size() * 4);
      h->ordOffHost.swap(off); h->ordQueues = Qj1; }
    if (plat_pass_printed(PASS_JA))
      fprintf(stderr, "[asched jobs_append] jobs %d rows %d in the order %d: fill %.4f ms, sort %.4f ms, merge %.4f ms; shapes in place %d: mask rows %.4f ms, row copies %.4f ms\n", M, m, nT,
              h->jaMs[0], h->jaMs[1], h->jaMs[2], inPlace ? (S1 - S0) + (int)revived.size() : 0, h->saMs[0], h->saMs[1]);
  }
  h->jaStats[0] = m; h->jaStats[1] = nT; h->jaStats[2] = S1 - S0; h->jaStats[3] = G1 - G0; h->jaStats[4] = (m > 0 && grow) ? 1 : 0; h->jaStats[5] = (newShapes && !inPlace) ? 1 : 0;
  h->jaStats[6] = (int32_t)h->jobCap; h->jaStats[7] = inPlace ? (S1 - S0) + (int32_t)revived.size() : 0;
  { int32_t* t = h->jasStats;
    t[0] = h->appendInPlace ? 1 : 0; t[1] = inPlace ? S1 - S0 : 0; t[2] = inPlace ? (int32_t)revived.size() : 0; t[3] = inPlace ? Sext1 - Sext0 : 0;
    t[4] = inPlace ? h->Cext - Cext0 : 0; t[5] = d.f.F; t[6] = inWhy; t[7] = 0; }
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  d.cfg.Q = 0;
  if (newShapes && !inPlace) {   // the shape-dependent tables, by the code jobs_set ends with (the key layout was decided above)
    int rc = rebuildMasks(h);
    h->jasStats[5] = d.f.F;   // (F after the call: the rebuild derived the fit shapes again)
    if (rc) return rc;
    rc = runControl(h, CMD_UPSERT_RESET);
    if (rc) return rc;
    rc = runControl(h, CMD_RESET_JOBS);
    h->allocPristine = h->nodesSet;
    h->evictedDirty = false;
    return rc;
  }
  if (m > 0 && grow && h->nodesSet) exclSetup(h);   // (the failed-selection records' per-job slots: sized by the capacity)
  // job dynamic state: everything unbound until round_prepare, as asched_jobs_patch leaves it
  return resetDynamicState(h, M1);
}
int32_t asched_jobs_append_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->jaStats[k];
  return 0;
}
int32_t asched_set_append_in_place(asched_t* h, int32_t on) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  h->appendInPlace = on != 0;
  return 0;
}
int32_t asched_jobs_append_shape_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->jasStats[k];
  out[0] = h->appendInPlace ? 1 : 0;
  return 0;
}

// ---- asched_jobs_respec (kernels_jobs_respec.h): a retried job's scheduling requirements are rewritten before it re-enters its queue (scheduler.go:1342-1383 through
// job.WithJobSchedulingInfo: node anti-affinity for every attempted run, :637-658 adopted at :1369-1376 — a new requirement class; the retry policy's memory bump, :683 ff.
// adopted at :1347-1354 — a new request vector).  The named rows, which have no run, take another class and / or request in place; the handle is left as
// asched_jobs_set of the edited table would leave it.  Neither field is part of the order key, so nothing is sorted or merged: per entry the target shape is found in
// the table asched_jobs_append uses, new and revived shapes take the steps of the append (in place with asched_set_append_in_place, else rebuildMasks), and one scatter
// writes shape, request, grid flag and JobRec of each row.  A record comes from a resident row of the target shape that no entry names, else from a template (DESIGN 3.20).
int32_t asched_jobs_respec(asched_t* h, int32_t n, const int32_t* job, const int32_t* req_class, const int64_t* req) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  const int M = h->M, R = h->R;
  Dev& d = h->dev;
  // ---- every refusal before anything changes
  if (!h->jobsSet || h->jShape.size() != (size_t)M || h->jReqClass.size() != (size_t)M || h->jReq.size() != (size_t)M * R || h->jNode.size() != (size_t)M || h->jAway.size() != (size_t)M ||
      h->shapeRow.size() != (size_t)h->S)
    return fail(h, ASCHED_ERR_INVALID, "jobs_respec: no job table on this handle (jobs_set first)");
  if (n < 0 || (n > 0 && (!job || (!req_class && !req)))) return fail(h, ASCHED_ERR_INVALID, "jobs_respec: bad arguments");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_respec: the job set carries the market order (jobs_set instead)");
  if (n > (1 << 29)) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_respec: more than 2^29 entries");
  if (h->jpSeen.size() != (size_t)M) h->jpSeen.assign(M, 0);
  auto unsee = [&](int upTo) { for (int i = 0; i < upTo; i++) h->jpSeen[job[i]] = 0; };
  {
    int seen = 0, code = ASCHED_ERR_INVALID;
    const char* why = nullptr;
    for (int i = 0; i < n && !why; i++) {
      const int j = job[i];
      if (j < 0 || j >= M) { why = "jobs_respec: a row outside the job table"; break; }
      if (h->jpSeen[j]) { why = "jobs_respec: a row named twice"; break; }
      h->jpSeen[j] = 1; seen = i + 1;
      if (req_class && (req_class[i] < 0 || req_class[i] >= h->C)) why = "jobs_respec: req_class out of range (asched_req_classes_append brings a new class first)";
      else if (h->jNode[j] >= 0) why = "jobs_respec: a row has a run (jobs_patch ends the run first)";
      else if (h->jAway[j]) { why = "jobs_respec: a cross-pool away row"; code = ASCHED_ERR_UNSUPPORTED; }
    }
    if (why) { unsee(seen); return fail(h, code, why); }
  }
  // the entries that change something: row, class, request, grid flag
  std::vector<int32_t> cJob, cCls; std::vector<int64_t> cReq; std::vector<uint8_t> cAligned;
  for (int i = 0; i < n; i++) {
    const int j = job[i];
    const int32_t cls = req_class ? req_class[i] : h->jReqClass[j];
    const int64_t* rq = req ? req + (size_t)i * R : &h->jReq[(size_t)j * R];
    if (cls == h->jReqClass[j] && !memcmp(rq, &h->jReq[(size_t)j * R], sizeof(int64_t) * R)) continue;
    uint8_t al = 1;
    for (int c = 0; c < h->K; c++) if (rq[h->indexedCol[c]] % h->indexedRes[c]) al = 0;
    cJob.push_back(j); cCls.push_back(cls); cReq.insert(cReq.end(), rq, rq + R); cAligned.push_back(al);
  }
  const int nc = (int)cJob.size(), S0 = h->S;
  // the target shape of every entry (undone by `undo` on a later refusal) and the source of its record: the first row of a resident shape unless this call names it
  if (nc > 0 && h->shapeTable.empty()) jaShapeTableBuild(h, (size_t)S0);
  JaShapes g; g.begin(h);
  std::vector<int32_t> cShape(nc), cSrc(nc, -1), cTpl(nc, -1), cOld(nc);
  for (int k = 0; k < nc; k++) {
    const int j = cJob[k];
    const int32_t s = cShape[k] = jaShapeFind(h, cCls[k], h->jPc[j], &cReq[(size_t)k * R], j);
    cOld[k] = h->jShape[j];
    if (!cAligned[k]) h->shapeUnaligned[s] = 1;   // (a property of the shape)
    if (s < S0) {
      int32_t& first = h->shapeRow[s];
      if (first < 0) { if (g.revived.empty()) g.shapeRowSaved = h->shapeRow; g.revived.push_back(s); first = j; }   // a delete or an earlier respec emptied the shape
      else if (!h->jpSeen[first]) cSrc[k] = first;
    }
  }
  unsee(n);
  const int S1 = (int)h->shapeClass.size();
  const bool newShapes = S1 > S0 || !g.revived.empty();   // (a revived shape takes the path of a new one, as in asched_jobs_append)
  const bool anyAway = d.cfg.hasAway != 0;   // (the rows keep their priority classes)
  std::vector<int64_t> oldReq;
  auto undo = [&]() {   // a refusal after the shape lookup: the handle exactly as it was
    if (!newShapes) return;
    if (g.mirrorsGrown) for (int k = 0; k < nc; k++) memcpy(&h->jReq[(size_t)cJob[k] * R], &oldReq[(size_t)k * R], sizeof(int64_t) * R);
    jaShapesUndo(h, g);
  };
  auto mirrorReq = [&]() { for (int k = 0; k < nc; k++) memcpy(&h->jReq[(size_t)cJob[k] * R], &cReq[(size_t)k * R], sizeof(int64_t) * R); };
  if (newShapes) {
    // what the rebuild can refuse, checked on the host first, on the request mirror of the edited table
    oldReq.resize((size_t)nc * R);
    for (int k = 0; k < nc; k++) memcpy(&oldReq[(size_t)k * R], &h->jReq[(size_t)cJob[k] * R], sizeof(int64_t) * R);
    mirrorReq(); h->S = S1; g.mirrorsGrown = true;
    std::string why;
    if (int rrc = jaShapesRefusal(h, g, anyAway, why)) { undo(); return fail(h, rrc, "jobs_respec: " + why); }
  }
  if (newShapes && h->appendInPlace) {
    bool negNew = false;
    for (size_t k = 0; k < cReq.size() && !negNew; k++) negNew = cReq[k] < 0;
    std::string why;
    if (int rrc = jaInPlaceDecide(h, g, anyAway, negNew, why)) { undo(); return fail(h, rrc, "jobs_respec: " + why); }
  }
  // one template record per target shape that some entry has no source row for; the per-shape tables of buildFast must cover the shape (else the rebuild)
  bool rebuild = newShapes && !g.inPlace;
  std::vector<int32_t> tplShape;
  if (!rebuild && d.f.structOk && d.jrec) {
    std::unordered_map<int32_t, int32_t> tplOf;
    for (int k = 0; k < nc; k++) if (cSrc[k] < 0) cTpl[k] = jaTemplateOf(tplOf, tplShape, cShape[k]);
    if (!tplShape.empty() && (h->fitOf.size() != (size_t)S1 || h->fsDelta.size() != (size_t)S1 || h->rowLiteral.size() < (size_t)S1)) { rebuild = true; g.inWhy = 1; tplShape.clear(); }
  }
  if (rebuild && g.inPlace) {   // (the tables the in-place decision grew are derived again by the rebuild; the blocks it would have staged are not needed)
    g.inPlace = false; g.shapeMask1 = nullptr;
  }
  const size_t nTpl = tplShape.size();
  const int nNewRows = g.inPlace ? (S1 - S0) + ((int)h->awayRowClass.size() - g.A0) : 0;
  // ---- every device block before anything changes: running out of device memory here is a refusal too
  const size_t oAl = up256(sizeof(int32_t) * 4 * (size_t)nc), oReq = oAl + up256((size_t)nc), oTpl = oReq + up256(sizeof(int64_t) * (size_t)nc * R),
               oSa = oTpl + up256(sizeof(JobRec) * nTpl), need = oSa + up256((size_t)nNewRows * (8 + 8 * (size_t)R));
  KeptBlock<char> scratch{h->jpBufs, h->jpScratch, h->jpScratchBytes};
  if (nc > 0 && !scratch.tryGrow(need)) { undo(); return fail(h, ASCHED_ERR_DEVICE, "jobs_respec: out of device memory for the scratch; the handle is as it was"); }
  StagedBlocks sb;
  if (newShapes) jaStageShapes(h, g, sb);
  if (!sb.allocate()) {
    scratch.drop();
    undo();
    return fail(h, ASCHED_ERR_DEVICE, "jobs_respec: out of device memory for the grown shape tables; the handle is as it was");
  }
  // ---- what jobs_set resets (the job table half edited).  On the rebuild path the call ends with rebuildMasks: the fast structure goes
  residentTouchJobs(h, rebuild, !rebuild);
  plat_pass_clear(PASS_SA, h->saMs);
  scratch.adopt();
  int emptied = 0, fromTpl = 0;
  if (nc > 0) {
    sb.fill();
    plat_sync();
    sb.commit();
    // the host mirrors
    if (!g.mirrorsGrown) mirrorReq();
    for (int k = 0; k < nc; k++) { h->jReqClass[cJob[k]] = cCls[k]; h->jShape[cJob[k]] = cShape[k]; }
    h->S = S1; d.cfg.S = S1;
    // shapeRow: an old shape whose first row left gets its next row in ONE forward pass over the jShape mirror (-1: the shape is left without a row, until
    // asched_shapes_compact); a target shape's first row is the smallest row it now has
    { std::vector<uint8_t> lost; int left = 0;
      for (int k = 0; k < nc; k++) if (h->shapeRow[cOld[k]] == cJob[k]) {
        if (lost.empty()) lost.assign(S1, 0);
        if (!lost[cOld[k]]) { lost[cOld[k]] = 1; left++; }
        h->shapeRow[cOld[k]] = -1;
      }
      for (int i = 0; i < M && left > 0; i++) { const int32_t s = h->jShape[i]; if (lost[s] && h->shapeRow[s] < 0) { h->shapeRow[s] = i; left--; } }
      emptied = left;
      for (int k = 0; k < nc; k++) { int32_t& first = h->shapeRow[cShape[k]]; if (first < 0 || cJob[k] < first) first = cJob[k]; } }
    // the entries: the only upload proportional to anything
    int32_t* e32 = (int32_t*)h->jpScratch; const size_t nn = (size_t)nc;
    plat_h2d(e32, cJob.data(), nn * 4); plat_h2d(e32 + nn, cShape.data(), nn * 4); plat_h2d(e32 + 2 * nn, cSrc.data(), nn * 4); plat_h2d(e32 + 3 * nn, cTpl.data(), nn * 4);
    plat_h2d(h->jpScratch + oAl, cAligned.data(), nn); plat_h2d(h->jpScratch + oReq, cReq.data(), nn * 8 * R);
    if (g.inPlace && jaInPlaceApply(h, g, h->jpScratch + oSa)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    JsArgs a; memset(&a, 0, sizeof a);
    a.n = nc; a.R = R; a.writeRec = (!rebuild && d.f.structOk && d.jrec) ? 1 : 0;
    a.pJob = e32; a.pShape = e32 + nn; a.pSrc = e32 + 2 * nn; a.pTpl = e32 + 3 * nn;
    a.pAligned = (const uint8_t*)(h->jpScratch + oAl); a.pReq = (const int64_t*)(h->jpScratch + oReq);
    if (nTpl) { jaTemplatesUpload(h, tplShape, h->jpScratch + oTpl); a.tpl = (const JobRec*)(h->jpScratch + oTpl); }
    if (a.writeRec) for (int k = 0; k < nc; k++) if (cTpl[k] >= 0) fromTpl++;
    int prc = plat_take_failure() ? -1 : plat_jobs_respec(d, a);
    if (prc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  }
  { int32_t* t = h->jsStats;
    t[0] = n; t[1] = n - nc; t[2] = S1 - S0; t[3] = (int32_t)g.revived.size(); t[4] = emptied; t[5] = rebuild ? 1 : 0; t[6] = g.inWhy; t[7] = fromTpl; }
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  d.cfg.Q = 0;
  if (rebuild) {   // the shape-dependent tables, by the code jobs_set ends with (the key layout was decided above)
    int rc = rebuildMasks(h);
    if (rc) return rc;
    rc = runControl(h, CMD_UPSERT_RESET);
    if (rc) return rc;
    rc = runControl(h, CMD_RESET_JOBS);
    h->allocPristine = h->nodesSet;
    h->evictedDirty = false;
    return rc;
  }
  // job dynamic state: everything unbound until round_prepare, as asched_jobs_patch leaves it
  return resetDynamicState(h, M);
}
int32_t asched_jobs_respec_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->jsStats[k];
  return 0;
}

// ---- asched_req_classes_append (kernels_req_classes_append.h): a submission whose (tolerations, node selector, required node affinity) set the table has not seen —
// the requirement-class part of the scheduling key (internaltypes/podutils.go:52-72) in syncState's upsert.  The n classes get ids C .. C + n - 1 behind the C resident
// real ones; the handle is left as asched_jobs_set of the same job table with the concatenated class list would leave it (DESIGN 3.17).  No resident row names a new
// class, so shapes, shape mask, fit shapes, minima, key layout and job records stay; the class mask grows by n rows in a fresh block, the derived away classes (numbered
// behind C by deriveAwayRows, in shape order) move up by n, and where the fast structure exists every node gains the bits of the new classes that match it.  Where that
// cannot be exact the tail of jobs_set runs on the grown class list (the rebuild path of asched_jobs_append) and the statistics give the reason.
int32_t asched_req_classes_append(asched_t* h, const asched_req_classes* more) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  Dev& d = h->dev;
  const int M = h->M;
  // ---- every refusal before anything changes
  if (!h->jobsSet) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: no job table on this handle (jobs_set first)");
  if (!more || more->n < 0) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: bad arguments");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "req_classes_append: the job set carries the market order (jobs_set instead)");
  const int n = more->n, C0 = h->C, Cext0 = h->Cext;
  if ((long long)Cext0 + n > (1ll << 24)) return fail(h, ASCHED_ERR_UNSUPPORTED, "req_classes_append: more than 2^24 requirement classes");
  const int C1 = C0 + n, W = d.cfg.W;
  if (n > 0) {
    auto ascending = [&](const int32_t* off, int len) { if (off[0] < 0) return false; for (int i = 0; i < len; i++) if (off[i] > off[i + 1]) return false; return true; };
    if (!more->tol_off && (more->tol_key || more->tol_op || more->tol_value || more->tol_effect)) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: toleration values without tol_off");
    if (!more->sel_off && (more->sel_key || more->sel_value)) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: selector values without sel_off");
    if (more->tol_off && !ascending(more->tol_off, n)) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: tol_off is not ascending");
    if (more->sel_off && !ascending(more->sel_off, n)) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: sel_off is not ascending");
    if (more->tol_off && more->tol_off[n] > 0 && !(more->tol_key && more->tol_op && more->tol_value && more->tol_effect)) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: tol_off without the toleration arrays");
    if (more->sel_off && more->sel_off[n] > 0 && !(more->sel_key && more->sel_value)) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: sel_off without the selector arrays");
    if (more->has_affinity) {
      bool any = false;
      for (int i = 0; i < n; i++) any = any || more->has_affinity[i];
      if (any) {
        if (!more->aff_term_off || !more->aff_expr_off) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: has_affinity without the term arrays");
        if (!ascending(more->aff_term_off, n) || !ascending(more->aff_expr_off, more->aff_term_off[n])) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: an affinity offset array is not ascending");
        const int nx = more->aff_expr_off[more->aff_term_off[n]];
        if (nx > 0 && !(more->aff_expr_key && more->aff_expr_op && more->aff_value_off)) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: has_affinity without the expression arrays");
        if (nx > 0 && (!ascending(more->aff_value_off, nx) || (more->aff_value_off[nx] > 0 && !more->aff_values))) return fail(h, ASCHED_ERR_INVALID, "req_classes_append: aff_value_off is not ascending or has no values");
      }
    }
  }
  std::vector<std::vector<HTol>> newTol(n); std::vector<std::vector<HSel>> newSel(n); std::vector<HAffinity> newAff(n);
  bool anyAff = false;
  for (int i = 0; i < n; i++) {
    if (int prc = reqClassParse(h, more, i, newTol[i], newSel[i], newAff[i])) return prc;   // (an unknown affinity operator: jobs_set's own refusal)
    anyAff = anyAff || newAff[i].present;
  }
  // (the rebuild path can refuse nothing here: layoutKeys reads no class, and LIT_TMAX is a property of a mask row — no row names a new class)
  const bool haveMasks = h->nodesSet && h->dClassMask && h->dShapeClass && d.typeMask;
  const bool haveFast = d.f.structOk && d.nodeCls;
  int why = 0;
  if (n > 0 && !haveMasks) why = 1;
  else if (n > 0 && haveFast && C0 <= 64 && C1 > 64) why = 2;   // (buildFast requires C <= 64: the rebuild gives the structure up as jobs_set would)
  const bool inPlace = n > 0 && !why;
  // ---- the host mirrors with the grown class list (saved: a refusal for memory puts them back)
  const auto tolSaved = h->clsTol; const auto selSaved = h->clsSel; const auto affSaved = h->clsAff;
  const auto awayOffSaved = h->awayRowOff, awayClassSaved = h->awayRowClass, awayShapeSaved = h->awayRowShape;
  auto undo = [&]() {
    h->clsTol = tolSaved; h->clsSel = selSaved; h->clsAff = affSaved; h->awayRowOff = awayOffSaved; h->awayRowClass = awayClassSaved; h->awayRowShape = awayShapeSaved;
    h->C = C0; d.cfg.C = C0; h->Cext = Cext0;
  };
  if (n > 0) {
    h->clsTol.resize(C0); h->clsSel.resize(C0);
    if (!h->clsAff.empty()) h->clsAff.resize(C0);
    else if (anyAff) h->clsAff.assign(C0, {});   // (the first class with an affinity: every resident class has none)
    for (int i = 0; i < n; i++) { h->clsTol.push_back(newTol[i]); h->clsSel.push_back(newSel[i]); if (!h->clsAff.empty()) h->clsAff.push_back(newAff[i]); }
    h->C = C1; d.cfg.C = C1;
    deriveAwayRows(h, d.cfg.hasAway != 0);   // (the same derived classes over the unchanged shape table, each id larger by n)
  }
  const int A = (int)h->awayRowClass.size(), Sext = h->S + A;
  // ---- the rows of the new classes: decided per class.  Tier 1: by node type, on the device; tier 2: matched node by node here
  std::vector<int32_t> typeOff(n + 1, 0), typeList, hostRow(n, -1); std::vector<uint64_t> hostRows;
  int nT1 = 0, nT2 = 0;
  h->caHostMs[0] = h->caHostMs[1] = 0;
  if (inPlace) {
    if (h->Cext != Cext0 + n || (int)awayClassSaved.size() != A) { undo(); return fail(h, ASCHED_ERR_INVALID, "req_classes_append: the derived classes of the handle do not follow from its shape table (jobs_set)"); }
    int taintsIndexed = -1;   // every taint a resident node carries is in its node type: decided once, when the call has a candidate
    for (int i = 0; i < n; i++) {
      const int c = C0 + i;
      bool byType = !newAff[i].present && !h->hasTypeOverride;
      for (auto& sl : newSel[i]) byType = byType && h->indexedLabels.count(sl.key);
      if (byType && taintsIndexed < 0) {
        auto t0 = std::chrono::steady_clock::now();
        taintsIndexed = 1;
        if (!h->indexAllTaints) for (int v = 0; v < h->N && taintsIndexed; v++) for (auto& x : h->nodeTaints[v]) if (!h->indexedTaints.count(x.key)) { taintsIndexed = 0; break; }
        h->caHostMs[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
      byType = byType && taintsIndexed == 1;
      typeOff[i] = (int32_t)typeList.size();
      if (byType) {
        for (size_t t = 0; t < h->types.size(); t++) if (h->types[t].numNodes > 0 && classMatchesType(h, c, h->types[t])) typeList.push_back((int32_t)t);
        nT1++;
      } else {
        auto t0 = std::chrono::steady_clock::now();
        hostRow[i] = nT2++;
        hostRows.resize((size_t)nT2 * W, 0);
        uint64_t* row = hostRows.data() + (size_t)hostRow[i] * W;
        for (int v = 0; v < h->N; v++) if (classMatchesNode(h, c, v)) row[v >> 6] |= 1ull << (v & 63);
        h->caHostMs[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
    }
    typeOff[n] = (int32_t)typeList.size();
  }
  // ---- every new device block before anything changes on the device
  const size_t oTypes = up256(4 * (size_t)(n + 1)), oHostRow = oTypes + up256(4 * std::max<size_t>(typeList.size(), 1)), oRows = oHostRow + up256(4 * (size_t)std::max(n, 1)),
               scratchBytes = oRows + up256(8 * std::max<size_t>(hostRows.size(), 1));
  StagedBlocks sb; char* scratch = nullptr;   // the grown class mask; the scratch is this call's alone and freed at its end
  if (inPlace) {
    sb.stage(&h->maskBufs, &h->dClassMask, 8 * (size_t)std::max(h->Cext, 1) * W, -1);
    if (!(sb.allocate() && (scratch = (char*)plat_try_malloc(scratchBytes)))) {
      sb.drop();
      undo();
      return fail(h, ASCHED_ERR_DEVICE, "req_classes_append: out of device memory for the grown class mask; the handle is as it was");
    }
  }
  uint64_t* mask1 = (uint64_t*)sb.fresh(&h->dClassMask);
  // ---- what jobs_set resets (the class tables half grown).  Off the in-place path the call ends with rebuildMasks: the fast structure goes
  residentTouchJobs(h, why != 0);
  memset(h->jaStats, 0, sizeof h->jaStats); memset(h->jasStats, 0, sizeof h->jasStats); memset(h->jdStats, 0, sizeof h->jdStats); memset(h->jrStats, 0, sizeof h->jrStats); memset(h->rcStats, 0, sizeof h->rcStats); memset(h->jsStats, 0, sizeof h->jsStats);
  plat_pass_clear(PASS_CA, h->caMs);
  { int32_t* t = h->caStats;
    t[0] = n; t[1] = nT1; t[2] = nT2; t[3] = inPlace ? Cext0 - C0 : 0; t[4] = why ? 1 : 0; t[5] = why; t[6] = h->C; t[7] = h->Cext; }
  if (inPlace) {
    plat_h2d(scratch, typeOff.data(), 4 * typeOff.size());
    if (!typeList.empty()) plat_h2d(scratch + oTypes, typeList.data(), 4 * typeList.size());
    plat_h2d(scratch + oHostRow, hostRow.data(), 4 * hostRow.size());
    if (!hostRows.empty()) plat_h2d(scratch + oRows, hostRows.data(), 8 * hostRows.size());
    CaArgs a; memset(&a, 0, sizeof a);
    a.N = h->N; a.W = W; a.C0 = C0; a.dC = n;
    a.typeMask = d.typeMask; a.typeOff = (const int32_t*)scratch; a.types = (const int32_t*)(scratch + oTypes);
    a.hostRow = (const int32_t*)(scratch + oHostRow); a.hostRows = (const uint64_t*)(scratch + oRows);
    a.outMask = mask1; a.nodeCls = haveFast && C1 <= 64 ? d.nodeCls : nullptr;
    a.inMask = h->dClassMask; a.copy0 = (long long)C0 * W; a.src1 = (long long)C0 * W; a.dst1 = (long long)C1 * W; a.copy1 = (long long)(Cext0 - C0) * W;
    const int src = plat_take_failure() ? -1 : plat_req_classes_append(d, a);
    if (src) { plat_free(scratch); sb.drop(); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
    plat_pass_ms(PASS_CA, h->caMs);
#ifdef ASCHED_HOSTSIM
    { // the CPU build: every row decided by node type against the node-by-node match
      std::vector<uint64_t> got((size_t)n * W);
      plat_d2h(got.data(), mask1 + (size_t)C0 * W, got.size() * 8);
      for (int i = 0; i < n; i++) if (hostRow[i] < 0)
        for (int v = 0; v < h->N; v++)
          if ((int)((got[(size_t)i * W + (v >> 6)] >> (v & 63)) & 1) != (classMatchesNode(h, C0 + i, v) ? 1 : 0)) {
            fprintf(stderr, "hostsim: req_classes_append: class %d decided by node type differs from classMatchesNode on node %d\n", C0 + i, v); abort(); }
    }
#endif
    sb.commit();
    plat_free(scratch);
    if (Cext0 > C0 && Sext > 0) {   // the class of every mask row: the away rows name derived classes, whose ids moved
      std::vector<int32_t> shapeClassExt = h->shapeClass;
      shapeClassExt.insert(shapeClassExt.end(), h->awayRowClass.begin(), h->awayRowClass.end());
      plat_h2d(h->dShapeClass, shapeClassExt.data(), 4 * shapeClassExt.size());
    }
    if (plat_pass_printed(PASS_CA))
      fprintf(stderr, "[asched req_classes_append] nodes %d classes %d (by node type %d, on the host %d), derived rows moved %d: new rows %.4f ms, row copies %.4f ms; host: taint scan %.4f ms, host rows %.4f ms\n",
              h->N, n, nT1, nT2, Cext0 - C0, h->caMs[0], h->caMs[1], h->caHostMs[0], h->caHostMs[1]);
  }
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  d.cfg.Q = 0;
  if (why) {   // the tail of jobs_set on the grown class list
    int rc = rebuildMasks(h);
    if (rc) return rc;
    rc = runControl(h, CMD_UPSERT_RESET);
    if (rc) return rc;
    rc = runControl(h, CMD_RESET_JOBS);
    h->allocPristine = h->nodesSet;
    h->evictedDirty = false;
    return rc;
  }
  return resetDynamicState(h, M);
}
int32_t asched_req_classes_append_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->caStats[k];
  return 0;
}

// ---- asched_shapes_compact (kernels_shapes_compact.h): the shape and requirement-class tables of a resident handle only grow — asched_jobs_delete keeps an emptied
// shape's id, mask rows and fit shape, the in-place append adds shapes, classes are append-only — while buildFast gives the fast structure up above SMAX fit shapes or 64
// real classes.  This call retires what no resident row names: a shape with shapeRow[s] < 0, a fit shape no live shape maps to and, with ASCHED_COMPACT_CLASSES, a real
// class no live shape names.  The live ones keep their relative order and get dense ids; the handle is left as asched_jobs_set of the same job table (with the reduced
// class list) would leave it (DESIGN 3.19).  What is a bound or a union over rows and shapes stays: the key layout, the two minima, hasAway, the gang tables, the
// capacities — removing shapes can only make the true value tighter, and every consumer reads them as bounds (DESIGN 3.12).
//
// buildFast's predicate without its two counts (F <= SMAX, C <= 64): asked only where one of the counts comes back under its limit on a handle without the structure
static bool scQualifiesButCounts(asched* h) {
  const Dev& d = h->dev;
  int extra = 0;
  for (int r = 0; r < h->R; r++) { bool idx = false; for (int c = 0; c < h->K; c++) idx = idx || h->indexedCol[c] == r; if (!idx) extra++; }
  std::set<int32_t> distinctIdx(h->indexedCol.begin(), h->indexedCol.end());
  if (!(h->N > 0 && h->M > 0 && !h->hasAllocByPrio && h->allocLeTotal && extra <= MAXE && (int)distinctIdx.size() == h->K && d.cfg.keyWords != 2)) return false;
  for (int64_t v : h->jReq) if (v < 0) return false;
  return true;
}
int32_t asched_shapes_compact(asched_t* h, int32_t flags, int32_t* class_new_id) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  Dev& d = h->dev;
  const int M = h->M, R = h->R, W = d.cfg.W;
  // ---- every refusal before anything changes
  if (!h->jobsSet || h->jShape.size() != (size_t)M || h->shapeRow.size() != (size_t)h->S || h->shapeClass.size() != (size_t)h->S || h->awayRowOff.size() != (size_t)h->S + 1)
    return fail(h, ASCHED_ERR_INVALID, "shapes_compact: no job table on this handle (jobs_set first)");
  if (flags & ~(ASCHED_COMPACT_CLASSES | ASCHED_COMPACT_COUNT_ONLY)) return fail(h, ASCHED_ERR_INVALID, "shapes_compact: unknown flag bits");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "shapes_compact: the job set carries the market order (jobs_set instead)");
  if (M <= 0) return fail(h, ASCHED_ERR_UNSUPPORTED, "shapes_compact: the table has no rows, so every shape is dead (a handle holds at least one job: jobs_set of the next table instead)");
  const bool withCls = (flags & ASCHED_COMPACT_CLASSES) != 0, countOnly = (flags & ASCHED_COMPACT_COUNT_ONLY) != 0;
  const int S0 = h->S, C0 = h->C, Cext0 = h->Cext, A0 = (int)h->awayRowClass.size();
  const bool haveMasks = h->nodesSet && h->dClassMask && h->dShapeClass && d.shapeMask && h->fitOf.size() == (size_t)S0 && h->fsDelta.size() == (size_t)S0 &&
                         h->fsMin.size() == (size_t)S0 && h->fsNever.size() == (size_t)S0 && h->awayRowOff.size() == (size_t)S0 + 1;
  const int F0 = haveMasks ? (int)h->fitTab.size() : 0;
  // ---- liveness and the three maps: O(S) on the host, no device pass (jobs_delete and jobs_append maintain shapeRow)
  std::vector<int32_t> shapeNew(S0, -1), fitNew(F0, -1), clsNew(C0, -1), oldShape, oldFit, oldCls;
  std::vector<uint8_t> fitLive(F0, 0), clsLive(C0, withCls ? 0 : 1);
  for (int s = 0; s < S0; s++) if (h->shapeRow[s] >= 0) {
    if (h->shapeClass[s] < 0 || h->shapeClass[s] >= C0 || (haveMasks && (h->fitOf[s] < 0 || h->fitOf[s] >= F0))) return fail(h, ASCHED_ERR_INVALID, "shapes_compact: the shape table of the handle is inconsistent (jobs_set)");
    shapeNew[s] = (int32_t)oldShape.size(); oldShape.push_back(s);
    clsLive[h->shapeClass[s]] = 1;
    if (haveMasks) fitLive[h->fitOf[s]] = 1;
  }
  for (int f = 0; f < F0; f++) if (fitLive[f]) { fitNew[f] = (int32_t)oldFit.size(); oldFit.push_back(f); }
  for (int c = 0; c < C0; c++) if (clsLive[c]) { clsNew[c] = (int32_t)oldCls.size(); oldCls.push_back(c); }
  const int S1 = (int)oldShape.size(), F1 = (int)oldFit.size(), C1 = (int)oldCls.size();
  if (S1 <= 0) return fail(h, ASCHED_ERR_INVALID, "shapes_compact: no resident row names a shape (jobs_set)");
  if (countOnly) {
    int32_t* t = h->scStats;
    t[0] = S0 - S1; t[1] = F0 - F1; t[2] = C0 - C1; t[3] = Cext0 - C0; t[4] = 0; t[5] = 0; t[6] = S0; t[7] = F0;
    return 0;
  }
  const bool anyDead = S1 < S0 || C1 < C0;
  int why = 0;
  if (anyDead && !haveMasks) why = 1;
  else if (anyDead && !d.f.structOk && F1 <= SMAX && C1 <= 64 && (F0 > SMAX || C0 > 64) && scQualifiesButCounts(h)) why = F0 > SMAX ? 2 : 3;   // buildFast's predicate turns true
  const bool inPlace = anyDead && !why;
  const bool haveRec = inPlace && d.f.structOk && d.jrec;
  // ---- the compacted host mirrors (the old ones saved: a refusal below puts them back)
  struct Saved {
    std::vector<int32_t> shapeClass, shapePc, shapeRow, fitOf, awayRowOff, awayRowClass, awayRowShape; std::vector<int64_t> shapeReq; std::vector<uint8_t> shapeUnaligned, fsNever, rowLiteral;
    std::vector<uint64_t> fsDelta, fsMin; std::vector<ShapeReq> fitTab; decltype(asched::fitIds) fitIds;
    std::vector<std::vector<HTol>> clsTol; std::vector<std::vector<HSel>> clsSel; std::vector<HAffinity> clsAff;
  } sv;
  auto undo = [&]() {
    h->shapeClass.swap(sv.shapeClass); h->shapePc.swap(sv.shapePc); h->shapeRow.swap(sv.shapeRow); h->shapeReq.swap(sv.shapeReq); h->shapeUnaligned.swap(sv.shapeUnaligned);
    h->awayRowOff.swap(sv.awayRowOff); h->awayRowClass.swap(sv.awayRowClass); h->awayRowShape.swap(sv.awayRowShape); h->rowLiteral.swap(sv.rowLiteral);
    if (haveMasks) { h->fitOf.swap(sv.fitOf); h->fsNever.swap(sv.fsNever); h->fsDelta.swap(sv.fsDelta); h->fsMin.swap(sv.fsMin); h->fitTab.swap(sv.fitTab); h->fitIds.swap(sv.fitIds); }
    h->clsTol.swap(sv.clsTol); h->clsSel.swap(sv.clsSel); h->clsAff.swap(sv.clsAff);
    h->S = S0; h->C = C0; h->Cext = Cext0;
  };
  std::vector<int32_t> shapeSrc, clsSrc, shapeClassExt1, rowTypeOff1, rowTypes1; std::vector<int64_t> shapeReqExt1;
  bool clsMoves = false;
  if (anyDead) {
    sv.shapeClass = h->shapeClass; sv.shapePc = h->shapePc; sv.shapeRow = h->shapeRow; sv.shapeReq = h->shapeReq; sv.shapeUnaligned = h->shapeUnaligned;
    sv.awayRowOff = h->awayRowOff; sv.awayRowClass = h->awayRowClass; sv.awayRowShape = h->awayRowShape; sv.rowLiteral = h->rowLiteral;
    if (haveMasks) { sv.fitOf = h->fitOf; sv.fsNever = h->fsNever; sv.fsDelta = h->fsDelta; sv.fsMin = h->fsMin; sv.fitTab = h->fitTab; sv.fitIds = h->fitIds; }
    sv.clsTol = h->clsTol; sv.clsSel = h->clsSel; sv.clsAff = h->clsAff;
    for (int s1 = 0; s1 < S1; s1++) {
      const int s = oldShape[s1];
      h->shapeClass[s1] = clsNew[sv.shapeClass[s]]; h->shapePc[s1] = sv.shapePc[s]; h->shapeRow[s1] = sv.shapeRow[s]; h->shapeUnaligned[s1] = sv.shapeUnaligned[s];
      for (int r = 0; r < R; r++) h->shapeReq[(size_t)s1 * R + r] = sv.shapeReq[(size_t)s * R + r];
      if (haveMasks) { h->fitOf[s1] = fitNew[sv.fitOf[s]]; h->fsNever[s1] = sv.fsNever[s]; h->fsDelta[s1] = sv.fsDelta[s]; h->fsMin[s1] = sv.fsMin[s]; }
    }
    h->shapeClass.resize(S1); h->shapePc.resize(S1); h->shapeRow.resize(S1); h->shapeUnaligned.resize(S1); h->shapeReq.resize((size_t)S1 * R);
    if (haveMasks) {
      h->fitOf.resize(S1); h->fsNever.resize(S1); h->fsDelta.resize(S1); h->fsMin.resize(S1);
      h->fitTab.resize(F1); h->fitIds.clear();
      for (int f1 = 0; f1 < F1; f1++) { h->fitTab[f1] = sv.fitTab[oldFit[f1]]; h->fitTab[f1].cls = clsNew[h->fitTab[f1].cls]; }
      for (int s1 = 0; s1 < S1; s1++) { const ShapeReq& q = h->fitTab[h->fitOf[s1]]; h->fitIds.emplace(std::make_tuple(q.fieldMin, h->fsDelta[s1], q.ex0, q.ex1, q.cls, q.never), h->fitOf[s1]); }   // (fastShapeAdd's key)
    }
    if (C1 < C0) {   // the real classes, compacted; deriveAwayRows cuts the derived ones off and derives them again
      for (int c1 = 0; c1 < C1; c1++) { h->clsTol[c1] = sv.clsTol[oldCls[c1]]; h->clsSel[c1] = sv.clsSel[oldCls[c1]]; if (!h->clsAff.empty()) h->clsAff[c1] = sv.clsAff[oldCls[c1]]; }
    }
    h->S = S1; h->C = C1;
    deriveAwayRows(h, d.cfg.hasAway != 0);
    // the source of every mask row and class row of the compacted tables: away rows of a live shape keep their order within the shape (one per away entry of its
    // priority class), derived classes are re-numbered by first occurrence — gathered through these tables, never assumed to be in the old order
    const int A1 = (int)h->awayRowClass.size();
    shapeSrc.assign((size_t)S1 + A1, -1); clsSrc.assign(h->Cext, -1);
    for (int s1 = 0; s1 < S1; s1++) shapeSrc[s1] = oldShape[s1];
    for (int c1 = 0; c1 < C1; c1++) clsSrc[c1] = oldCls[c1];
    bool okRows = true;
    for (int k1 = 0; k1 < A1 && okRows; k1++) {
      const int s1 = h->awayRowShape[k1], s = oldShape[s1], kOld = sv.awayRowOff[s] + (k1 - h->awayRowOff[s1]);
      if (kOld >= sv.awayRowOff[s + 1] || kOld >= A0) { okRows = false; break; }
      shapeSrc[(size_t)S1 + k1] = S0 + kOld;
      int32_t& src = clsSrc[h->awayRowClass[k1]];
      if (src >= 0 && src != sv.awayRowClass[kOld]) okRows = false;
      src = sv.awayRowClass[kOld];
    }
    for (int32_t v : clsSrc) okRows = okRows && v >= 0 && v < Cext0;
    if (!okRows) { undo(); return fail(h, ASCHED_ERR_INVALID, "shapes_compact: the derived classes of the handle do not follow from its shape table (jobs_set)"); }
    clsMoves = h->Cext != Cext0;
    for (int c = 0; c < h->Cext && !clsMoves; c++) clsMoves = clsSrc[c] != c;
    if (inPlace) {
      shapeClassExt1 = h->shapeClass; shapeReqExt1 = h->shapeReq;
      for (int k = 0; k < A1; k++) {
        shapeClassExt1.push_back(h->awayRowClass[k]);
        for (int r = 0; r < R; r++) shapeReqExt1.push_back(h->shapeReq[(size_t)h->awayRowShape[k] * R + r]);
      }
      if (int rrc = buildRowTables(h, shapeClassExt1, rowTypeOff1, rowTypes1)) { std::string msg = h->err; undo(); return fail(h, rrc, "shapes_compact: " + msg); }   // (cannot happen: every row was a row before)
    }
  }
  const int A1 = (int)h->awayRowClass.size(), Sext1 = S1 + A1, Cext1 = h->Cext;
  // ---- the scratch (the maps and the source tables) and the fresh mask blocks before anything changes on the device: running out of memory is a refusal too
  const size_t oFit = up256(4 * (size_t)S0), oCls = oFit + up256(4 * (size_t)std::max(F0, 1)), oSSrc = oCls + up256(4 * (size_t)C0), oCSrc = oSSrc + up256(4 * (size_t)std::max(Sext1, 1)),
               scratchBytes = oCSrc + up256(4 * (size_t)std::max(Cext1, 1));
  StagedBlocks sb; char* scratch = nullptr;   // the compacted masks; the scratch is this call's alone and freed before they are swapped in
  if (anyDead) {
    if (inPlace) sb.stage(&h->maskBufs, &d.shapeMask, 8 * (size_t)std::max(Sext1, 1) * W, -1);
    if (inPlace && clsMoves) sb.stage(&h->maskBufs, &h->dClassMask, 8 * (size_t)std::max(Cext1, 1) * W, -1);
    if (!((scratch = (char*)plat_try_malloc(scratchBytes)) && sb.allocate())) {
      plat_free(scratch);
      undo();
      return fail(h, ASCHED_ERR_DEVICE, "shapes_compact: out of device memory for the compacted mask blocks; the handle is as it was");
    }
  }
  uint64_t* shapeMask1 = (uint64_t*)sb.fresh(&d.shapeMask); uint64_t* classMask1 = (uint64_t*)sb.fresh(&h->dClassMask);
  // ---- what jobs_set resets (the tables half compacted).  Off the in-place path the call ends with rebuildMasks: the fast structure goes
  residentTouchJobs(h, why != 0);
  memset(h->jaStats, 0, sizeof h->jaStats); memset(h->jasStats, 0, sizeof h->jasStats); memset(h->jdStats, 0, sizeof h->jdStats); memset(h->jrStats, 0, sizeof h->jrStats); memset(h->rcStats, 0, sizeof h->rcStats); memset(h->jsStats, 0, sizeof h->jsStats); memset(h->caStats, 0, sizeof h->caStats);
  plat_pass_clear(PASS_SC, h->scMs); h->scHostMs = 0;
  if (anyDead) {
    plat_h2d(scratch, shapeNew.data(), 4 * (size_t)S0);
    if (F0 > 0) plat_h2d(scratch + oFit, fitNew.data(), 4 * (size_t)F0);
    plat_h2d(scratch + oCls, clsNew.data(), 4 * (size_t)C0);
    if (Sext1 > 0) plat_h2d(scratch + oSSrc, shapeSrc.data(), 4 * (size_t)Sext1);
    if (Cext1 > 0) plat_h2d(scratch + oCSrc, clsSrc.data(), 4 * (size_t)Cext1);
    ScArgs a; memset(&a, 0, sizeof a);
    a.M = M; a.S0 = S0; a.F0 = F0; a.C0 = C0; a.W = W; a.N = h->N;
    a.shapeNew = (const int32_t*)scratch; a.jShape = d.jShape;
    if (haveRec) { a.jrec = d.jrec; a.fitNew = (const int32_t*)(scratch + oFit); if (C1 < C0) a.clsNew = (const int32_t*)(scratch + oCls); }
    if (inPlace) {
      a.shapeIn = d.shapeMask; a.shapeOut = shapeMask1; a.shapeSrc = (const int32_t*)(scratch + oSSrc); a.shapeRows = Sext1;
      if (classMask1) { a.clsIn = h->dClassMask; a.clsOut = classMask1; a.clsSrc = (const int32_t*)(scratch + oCSrc); a.clsRows = Cext1; }
      if (C1 < C0 && d.f.structOk && d.nodeCls && C0 <= 64) { a.nodeCls = d.nodeCls; for (int c = 0; c < C0; c++) if (clsLive[c]) a.liveCls |= 1ull << c; }
    }
    const int src = plat_take_failure() ? -1 : plat_shapes_compact(d, a);
    if (src) { plat_free(scratch); sb.drop(); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
    plat_pass_ms(PASS_SC, h->scMs);
    plat_free(scratch);
    if (inPlace) {
      sb.commit();
      // the small tables from the compacted host vectors: each is no longer than the block that holds it
      plat_h2d(h->dShapeClass, shapeClassExt1.data(), 4 * shapeClassExt1.size());
      plat_h2d(d.shapeReq, shapeReqExt1.data(), 8 * shapeReqExt1.size());
      plat_h2d(d.awayRowOff, h->awayRowOff.data(), 4 * h->awayRowOff.size());
      plat_h2d(d.rowLiteral, h->rowLiteral.data(), h->rowLiteral.size());
      plat_h2d(d.rowTypeOff, rowTypeOff1.data(), 4 * rowTypeOff1.size());
      if (!rowTypes1.empty()) plat_h2d(d.rowTypes, rowTypes1.data(), 4 * rowTypes1.size());
      d.f.F = F1;
      if (d.f.structOk && d.shapeTab) {
        plat_h2d(d.shapeTab, h->fitTab.data(), sizeof(ShapeReq) * h->fitTab.size());
        // (d.fitBits [F][fitW] is scratch the next base build fills for the F it finds: the block of the larger F holds it)
        if (const char* ms = getenv("ASCHED_SHAPE_MASK")) if (d.fitBits && ms[0] == '1') d.f.maskMode = F1 <= 64 ? 1 : F1 <= 128 ? 2 : 0;   // (buildFast's rule, for the smaller F)
      }
    }
    // the per-shape results of a round: fresh (zero) for the new shape ids, as jobs_set allocates them
    if (d.unfeasible) plat_memset(d.unfeasible, 0, (size_t)S0);
    if (d.unfeasibleReason) plat_memset(d.unfeasibleReason, 0, 4 * (size_t)S0);
    d.cfg.S = S1; d.cfg.C = C1;
    h->shapeTable.clear(); h->shapeHash.clear();   // (the next append builds them over the compacted shapes)
    // ---- the O(M) host step: the shape (and class) of every row in the mirrors, on the host threads
    const auto t0 = std::chrono::steady_clock::now();
    const bool remapCls = C1 < C0 && h->jReqClass.size() == (size_t)M;
    parallelChunks((size_t)M, 64, [&](size_t lo, size_t hi) {
      for (size_t j = lo; j < hi; j++) { h->jShape[j] = shapeNew[h->jShape[j]]; if (remapCls) h->jReqClass[j] = clsNew[h->jReqClass[j]]; }
    });
    h->scHostMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (plat_pass_printed(PASS_SC))
      fprintf(stderr, "[asched shapes_compact] jobs %d shapes %d -> %d fit %d -> %d classes %d -> %d (ext %d -> %d) %s: rows %.4f ms, gathers %.4f ms, class bits %.4f ms; host mirrors %.4f ms\n",
              M, S0, S1, F0, F1, C0, C1, Cext0, Cext1, why ? "rebuild" : "in place", h->scMs[0], h->scMs[1], h->scMs[2], h->scHostMs);
  }
  if (withCls && class_new_id) for (int c = 0; c < C0; c++) class_new_id[c] = clsNew[c];
  { int32_t* t = h->scStats;
    t[0] = S0 - S1; t[1] = F0 - F1; t[2] = C0 - C1; t[3] = Cext1 - C1; t[4] = why ? 1 : 0; t[5] = why; t[6] = S1; t[7] = haveMasks ? F1 : 0; }
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  d.cfg.Q = 0;
  if (why) {   // the tail of jobs_set on the compacted mirrors
    int rc = rebuildMasks(h);
    if (h->nodesSet) h->scStats[7] = d.f.F;
    if (rc) return rc;
    rc = runControl(h, CMD_UPSERT_RESET);
    if (rc) return rc;
    rc = runControl(h, CMD_RESET_JOBS);
    h->allocPristine = h->nodesSet;
    h->evictedDirty = false;
    return rc;
  }
  return resetDynamicState(h, M);
}
int32_t asched_shapes_compact_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->scStats[k];
  return 0;
}

// ---- asched_jobs_delete (kernels_jobs_delete.h): syncState's delete of the jobs in a terminal state (scheduler.go:539-549; Txn.BatchDelete / delete,
// jobdb/jobdb.go:941-990).  The named rows leave the table, the others keep their order and are renumbered densely; the handle is left as asched_jobs_set of the reduced
// table would leave it.  The device moves every static per-job array, the order and the gang lists; the host compacts its mirrors — the one O(M) host step.  Shape ids,
// dense gang ids, the key layout and the other aggregates of the table stay: wider than the reduced table needs or equal, never wrong (DESIGN 3.12).
int32_t asched_jobs_delete(asched_t* h, int32_t n, const int32_t* job, int32_t* new_id) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  const int M = h->M, R = h->R, G = h->G;
  Dev& d = h->dev;
  // ---- every refusal before anything changes
  if (!h->jobsSet || h->jQPrioHost.size() != (size_t)M || h->jSubmitHost.size() != (size_t)M || h->jRunTsHost.size() != (size_t)M || h->jNode.size() != (size_t)M ||
      h->gangOffHost.size() != (size_t)G + 2)
    return fail(h, ASCHED_ERR_INVALID, "jobs_delete: no job table on this handle (jobs_set first)");
  if (n < 0 || (n > 0 && !job)) return fail(h, ASCHED_ERR_INVALID, "jobs_delete: bad arguments");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_delete: the job set carries the market order, which ranks every job against every other (jobs_set instead)");
  if (h->jpSeen.size() != (size_t)M) h->jpSeen.assign(M, 0);
  std::vector<uint8_t>& gone = h->jpSeen;   // [M] the rows of this call, until the mirrors are compacted
  int nT = 0, nGang = 0;
  { int marked = 0;
    const char* why = nullptr;
    for (int i = 0; i < n; i++) {
      const int j = job[i];
      if (j < 0 || j >= M) { why = "jobs_delete: a row outside the job table"; break; }
      if (gone[j]) { why = "jobs_delete: a row named twice"; break; }
      gone[j] = 1; marked = i + 1;
      if (h->jQueue[j] >= 0) nT++;
      if (h->jGangDense[j] >= 0) nGang++;
    }
    if (why) { for (int i = 0; i < marked; i++) gone[job[i]] = 0; return fail(h, ASCHED_ERR_INVALID, why); }
  }
  if (n > 0 && n == M) {
    for (int i = 0; i < n; i++) gone[job[i]] = 0;
    return fail(h, ASCHED_ERR_UNSUPPORTED, "jobs_delete: every row of the table is named (a handle holds at least one job: jobs_set of the next table instead)");
  }
  const int M1 = M - n;
  const int total = h->ordOffHost.empty() ? 0 : h->ordOffHost[std::min<size_t>((size_t)h->ordQueues, h->ordOffHost.size() - 1)], total1 = total - nT;
  const int gangLen = h->gangOffHost[G], gangLen1 = gangLen - nGang;
  const size_t cap = std::max<size_t>(h->jobCap, (size_t)M);
  const bool haveRec = d.f.structOk && d.jrec;
  // ---- the scratch and every new block before anything changes: running out of device memory here is a refusal too.  The scratch: the entries | the survivors' list |
  // the new ids | the compacted gang lists.  The blocks: one per static per-job array, of the table's capacity (capacities do not shrink); the old ones are released at the end
  const size_t oSrc = up256(sizeof(int32_t) * (size_t)n), oNew = oSrc + up256(sizeof(int32_t) * (size_t)M), oGang = oNew + up256(sizeof(int32_t) * (size_t)M),
               need = oGang + up256(sizeof(int32_t) * (size_t)gangLen);
  StagedBlocks sb;
  KeptBlock<char> scratch{h->jpBufs, h->jpScratch, h->jpScratchBytes};
  const bool buildJp = n > 0 && !h->jp.built;
  const bool needSpare = n > 0 && (!h->jp.ordSpare || h->ordSpareCap < (size_t)total1);
  int32_t* ordSpareNew = nullptr;   // (its block is the one whose slot is this variable: nothing to release in its place)
  if (n > 0) {
    // (fill -1: none of these blocks is filled; the keep flags of a first incremental call are)
    void* s32[] = {&d.jQueue, &d.jPc, &d.jShape, &d.jGang, &d.jGangCard, &d.jGangUni, &d.jNode0, &d.jRunPrio, &h->jp.qprio};
    for (void* sl : s32) sb.stage(&h->jobBufs, sl, cap * 4, -1);
    if (d.jAway) sb.stage(&h->jobBufs, &d.jAway, cap, -1);
    sb.stage(&h->jobBufs, &d.jAligned, cap, -1); sb.stage(&h->jobBufs, &d.jLeaseMs, cap * 8, -1); sb.stage(&h->jobBufs, &h->jp.submit, cap * 8, -1); sb.stage(&h->jobBufs, &h->jp.runTs, cap * 8, -1);
    sb.stage(&h->jobBufs, &d.jReq, cap * 8 * R, -1);
    if (haveRec) sb.stage(&h->fastBufs, &d.jrec, sizeof(JobRec) * cap, -1);
    if (buildJp) sb.stage(&h->jobBufs, &h->jp.keep, cap, 1);   // first incremental call of this job table: the keep flags (the order-key inputs are uploaded below, compacted)
    if (needSpare) sb.stage(&h->jobBufs, &ordSpareNew, std::max<size_t>((size_t)total, h->ordCap) * 4, 0, nullptr, -1, true);
    if (!(scratch.tryGrow(need) && sb.allocate())) {
      scratch.drop();
      for (int i = 0; i < n; i++) gone[job[i]] = 0;
      return fail(h, ASCHED_ERR_DEVICE, "jobs_delete: out of device memory for the scratch and the compacted job table; the handle is as it was");
    }
  }
  // ---- what jobs_set resets (the job table half compacted)
  residentTouchJobs(h);
  plat_pass_clear(PASS_JD, h->jdMs);
  h->jdHostMs = 0;
  int gangsEmptied = 0, shapesEmptied = 0;
  if (n > 0) {
    scratch.adopt();
    if (needSpare) ordSpareNew = (int32_t*)sb.fresh(&ordSpareNew);
    sb.fill();
    JdArgs a; memset(&a, 0, sizeof a);
    a.M = M; a.M1 = M1; a.n = n; a.R = R; a.total = total; a.total1 = total1; a.gangLen = gangLen; a.gangLen1 = gangLen1;
    int32_t* e32 = (int32_t*)h->jpScratch;
    plat_h2d(e32, job, sizeof(int32_t) * (size_t)n);
    a.job = e32; a.keep = buildJp ? (uint8_t*)sb.fresh(&h->jp.keep) : h->jp.keep;
    a.src = (int32_t*)(h->jpScratch + oSrc); a.newId = (uint32_t*)(h->jpScratch + oNew);
    { const int32_t* in[JD_N32] = {d.jQueue, d.jPc, d.jShape, d.jGang, d.jGangCard, d.jGangUni, d.jNode0, d.jRunPrio, buildJp ? nullptr : (const int32_t*)h->jp.qprio};   // (the queue priorities move as the 4-byte words they are)
      void* sl[JD_N32] = {&d.jQueue, &d.jPc, &d.jShape, &d.jGang, &d.jGangCard, &d.jGangUni, &d.jNode0, &d.jRunPrio, &h->jp.qprio};
      for (int k = 0; k < JD_N32; k++) { a.in32[k] = in[k]; a.out32[k] = (int32_t*)sb.fresh(sl[k]); } }
    a.inAway = d.jAway; a.outAway = (uint8_t*)sb.fresh(&d.jAway); a.inAligned = d.jAligned; a.outAligned = (uint8_t*)sb.fresh(&d.jAligned);
    a.inLease = d.jLeaseMs; a.outLease = (int64_t*)sb.fresh(&d.jLeaseMs);
    a.inSubmit = buildJp ? nullptr : h->jp.submit; a.outSubmit = (int64_t*)sb.fresh(&h->jp.submit); a.inRunTs = buildJp ? nullptr : h->jp.runTs; a.outRunTs = (int64_t*)sb.fresh(&h->jp.runTs);
    a.inReq = d.jReq; a.outReq = (int64_t*)sb.fresh(&d.jReq);
    if (haveRec) { a.inRec = d.jrec; a.outRec = (JobRec*)sb.fresh(&d.jrec); }
    a.ordIn = d.ordAll; a.ordOut = ordSpareNew ? ordSpareNew : h->jp.ordSpare;
    a.gangIn = d.gangJobs; a.gangOut = (int32_t*)(h->jpScratch + oGang);
    int prc = plat_take_failure() ? -1 : plat_jobs_delete(d, a);
    if (prc) {
      sb.drop();
      gone.assign(M, 0);
      return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    }
    plat_pass_ms(PASS_JD, h->jdMs);
    if (gangLen1 > 0) plat_d2d(d.gangJobs, a.gangOut, sizeof(int32_t) * (size_t)gangLen1);
    if (new_id) {   // old -> new: the scan's exclusive prefix, -1 for the rows that left
      plat_d2h(new_id, a.newId, sizeof(int32_t) * (size_t)M);
      for (int i = 0; i < n; i++) new_id[job[i]] = -1;
    }
    // the blocks: swapped in, the old ones released (plat_jobs_delete has waited for the device)
    if (ordSpareNew) { if (h->jp.ordSpare) h->jobBufs.release(h->jp.ordSpare); h->jp.ordSpare = nullptr; }
    sb.commit();
    if (ordSpareNew) { h->jp.ordSpare = ordSpareNew; h->ordSpareCap = std::max<size_t>((size_t)total, h->ordCap); }
    if (total > 0) { std::swap(d.ordAll, h->jp.ordSpare); std::swap(h->ordCap, h->ordSpareCap); }
    // ---- the host mirrors, compacted in place (row order is kept: every element moves down or stays), one array per host thread; then what the host derives from them
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> goneOfQueue((size_t)h->ordQueues + 2, 0), goneOfGang((size_t)G + 1, 0);
    for (int i = 0; i < n; i++) {
      const int j = job[i];
      if (h->jQueue[j] >= 0 && h->jQueue[j] < h->ordQueues) goneOfQueue[(size_t)h->jQueue[j] + 1]++;
      if (h->jGangDense[j] >= 0) goneOfGang[h->jGangDense[j]]++;
    }
    { auto squeeze = [&](auto& v, size_t w) {
        size_t o = 0;
        for (size_t i = 0; i < (size_t)M; i++) if (!gone[i]) { if (o != i) for (size_t x = 0; x < w; x++) v[o * w + x] = v[i * w + x]; o++; }
        v.resize((size_t)M1 * w);
      };
      std::vector<std::function<void()>> tasks = {
        [&] { squeeze(h->jQueue, 1); }, [&] { squeeze(h->jPc, 1); }, [&] { squeeze(h->jReqClass, 1); }, [&] { squeeze(h->jShape, 1); }, [&] { squeeze(h->jNode, 1); },
        [&] { squeeze(h->jRunPrio, 1); }, [&] { squeeze(h->jGangDense, 1); }, [&] { squeeze(h->jAway, 1); }, [&] { squeeze(h->jGangUniKey, 1); }, [&] { squeeze(h->jReq, (size_t)R); },
        [&] { squeeze(h->jQPrioHost, 1); }, [&] { squeeze(h->jSubmitHost, 1); }, [&] { squeeze(h->jRunTsHost, 1); }};
      std::atomic<size_t> next{0};
      auto work = [&] { for (;;) { size_t c = next.fetch_add(1); if (c >= tasks.size()) return; tasks[c](); } };
      const int T = M < 65536 ? 1 : std::min<int>(hostThreads(), (int)tasks.size());
      std::vector<std::thread> th;
      for (int t = 1; t < T; t++) th.emplace_back(work);
      work();
      for (auto& x : th) x.join(); }
    gone.assign(M1, 0);
    { std::vector<int32_t> row(h->shapeRow.size(), -1);   // the first surviving row of every shape
      for (int i = 0; i < M1; i++) { int32_t& r = row[h->jShape[i]]; if (r < 0) r = i; }
      for (size_t s = 0; s < row.size(); s++) if (row[s] < 0 && h->shapeRow[s] >= 0) shapesEmptied++;
      h->shapeRow.swap(row); }
    { std::vector<int32_t> off((size_t)G + 2, 0);
      for (int g = 0; g < G; g++) off[g + 1] = off[g] + (h->gangOffHost[g + 1] - h->gangOffHost[g]) - goneOfGang[g];
      off[G + 1] = off[G] + std::max(M1, 1);   // scratch gang slot for schedule_many
      for (auto it = h->gangMap.begin(); it != h->gangMap.end();) {   // an emptied gang: its (queue, gang id) may come again as a new gang
        const int g = it->second;
        if (off[g + 1] == off[g] && h->gangOffHost[g + 1] > h->gangOffHost[g]) { it = h->gangMap.erase(it); gangsEmptied++; } else ++it;
      }
      plat_h2d(d.gangOff, off.data(), off.size() * 4);
      h->gangOffHost.swap(off); }
    { std::vector<int32_t> off(h->ordOffHost.size(), total1);
      int below = 0;
      for (int q = 0; q <= h->ordQueues && (size_t)q < off.size(); q++) { below += goneOfQueue[q]; off[q] = h->ordOffHost[q] - below; }
      plat_h2d(d.ordAllOff, off.data(), off.size() * 4);
      h->ordOffHost.swap(off); }
    if (buildJp) {   // the order-key inputs become resident, already compacted
      plat_h2d(h->jp.qprio, h->jQPrioHost.data(), (size_t)M1 * 4); plat_h2d(h->jp.submit, h->jSubmitHost.data(), (size_t)M1 * 8); plat_h2d(h->jp.runTs, h->jRunTsHost.data(), (size_t)M1 * 8);
      h->jp.built = true;
    }
    h->M = M1; d.cfg.M = M1;
    h->jdHostMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (plat_pass_printed(PASS_JD))
      fprintf(stderr, "[asched jobs_delete] jobs %d entries %d in the order %d: mark %.4f ms, scan %.4f ms, gather %.4f ms, order %.4f ms, gang lists %.4f ms, host mirrors %.4f ms\n", M, n, nT,
              h->jdMs[0], h->jdMs[1], h->jdMs[2], h->jdMs[3], h->jdMs[4], h->jdHostMs);
  }
  if (n == 0 && new_id) for (int i = 0; i < M; i++) new_id[i] = i;   // (no pass ran: every row keeps its id)
  h->jdStats[0] = n; h->jdStats[1] = nT; h->jdStats[2] = gangsEmptied; h->jdStats[3] = shapesEmptied; h->jdStats[4] = M1; h->jdStats[5] = (int32_t)h->jobCap; h->jdStats[6] = h->jdStats[7] = 0;
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  // job dynamic state: everything unbound until round_prepare, as at the end of jobs_set
  d.cfg.Q = 0;
  return resetDynamicState(h, M1);
}
int32_t asched_jobs_delete_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->jdStats[k];
  return 0;
}

// ---- asched_nodes_patch (kernels_nodes_patch.h): what populateNodeDb re-reads per node every cycle (scheduling_algo.go:1069-1095) for a few rows of the resident node
// table.  The handle is left as asched_nodes_upsert of the patched table would leave it.  Two paths, chosen per call: nothing the host derives from the WHOLE table can
// change (the set of populated node types, the aggregates of the key layout) — the entries are scattered on the device and the touched mask words rewritten; or the
// patched table goes through nodes_upsert's own code (nodesUpsertBody).
int32_t asched_nodes_patch(asched_t* h, const asched_nodes_patch_rows* rows) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  if (!rows) return fail(h, ASCHED_ERR_INVALID, "nodes_patch: bad arguments");
  const int N = h->N, R = h->R, K = h->K, n = rows->n;
  Dev& d = h->dev;
  // ---- every refusal before anything changes
  if (!h->nodesSet || h->nodeAllocHost.size() != (size_t)N * R || h->nodeOverAlloc.size() != (size_t)N || h->nodeIndexHost.size() != (size_t)N)
    return fail(h, ASCHED_ERR_INVALID, "nodes_patch: no node table on this handle (nodes_upsert first)");
  if (n < 0 || (n > 0 && !rows->node)) return fail(h, ASCHED_ERR_INVALID, "nodes_patch: bad arguments");
  if (h->uploadedAllocByPrio || h->hasTypeOverride) return fail(h, ASCHED_ERR_UNSUPPORTED, "nodes_patch: the node table was uploaded with alloc_by_prio or node_type_override (nodes_upsert instead)");
  if (rows->taint_off) {
    if (n > 0 && rows->taint_off[0] < 0) return fail(h, ASCHED_ERR_INVALID, "nodes_patch: taint_off is not ascending");
    for (int i = 0; i < n; i++) if (rows->taint_off[i + 1] < rows->taint_off[i]) return fail(h, ASCHED_ERR_INVALID, "nodes_patch: taint_off is not ascending");
    if (n > 0 && rows->taint_off[n] > 0 && (!rows->taint_key || !rows->taint_value || !rows->taint_effect)) return fail(h, ASCHED_ERR_INVALID, "nodes_patch: bad arguments");
  }
  if (h->npSeen.size() != (size_t)N) h->npSeen.assign(N, 0);
  { int bad = 0; const char* why = nullptr;
    for (int i = 0; i < n; i++) {
      const int v = rows->node[i];
      if (v < 0 || v >= N) { why = "nodes_patch: a node outside the node table"; break; }
      if (h->npSeen[v]) { why = "nodes_patch: a node named twice"; break; }
      h->npSeen[v] = 1; bad = i + 1;
    }
    for (int i = 0; i < bad; i++) h->npSeen[rows->node[i]] = 0;
    if (why) return fail(h, ASCHED_ERR_INVALID, why); }
  // ---- the new state of every entry, and which path serves the call
  std::vector<std::vector<HTaint>> eTaints(n);   // the node's taints as nodes_upsert keeps them: the listed ones, then the unschedulable taint
  std::vector<uint8_t> eUns(n), eOver(n);
  std::vector<int64_t> eAlloc((size_t)n * R);
  std::vector<int> eType(n, -1);
  std::vector<HType> newTypes; std::vector<std::string> newCanon;   // node types the table does not have, in order of first occurrence
  std::vector<int> typeDelta(h->types.size(), 0);
  int why = 0, typeChanged = 0;
  for (int i = 0; i < n; i++) {
    const int v = rows->node[i];
    eUns[i] = rows->unschedulable ? (rows->unschedulable[i] ? 1 : 0) : h->nodeUnsched[v];
    eOver[i] = rows->over_allocated ? (rows->over_allocated[i] ? 1 : 0) : h->nodeOverAlloc[v];
    for (int r = 0; r < R; r++) eAlloc[(size_t)i * R + r] = rows->allocatable ? rows->allocatable[(size_t)i * R + r] : h->nodeAllocHost[(size_t)v * R + r];
    if (rows->taint_off) for (int k = rows->taint_off[i]; k < rows->taint_off[i + 1]; k++) eTaints[i].push_back({rows->taint_key[k], rows->taint_value[k], rows->taint_effect[k]});
    else { eTaints[i] = h->nodeTaints[v]; if (h->nodeUnsched[v] && !eTaints[i].empty()) eTaints[i].pop_back(); }
    if (eUns[i]) eTaints[i].push_back({kUnschedulableTaintKey, 0, ASCHED_EFFECT_NO_SCHEDULE});  // node.go:127-129
    HType t; std::string canon;
    nodeTypeOf(h, eTaints[i], h->nodeLabels[v], t, canon);
    auto it = h->typeByCanon.find(canon);
    if (it != h->typeByCanon.end()) eType[i] = it->second;
    else {
      size_t k = 0;
      while (k < newCanon.size() && newCanon[k] != canon) k++;
      if (k == newCanon.size()) { newCanon.push_back(canon); newTypes.push_back(t); }
      newTypes[k].numNodes++;
    }
    if (eType[i] != h->nodeType[v]) { typeChanged++; typeDelta[h->nodeType[v]]--; if (eType[i] >= 0) typeDelta[eType[i]]++; }
  }
  if (!newTypes.empty()) why = 1;
  if (!why) for (size_t t = 0; t < h->types.size(); t++) if ((h->types[t].numNodes > 0) != (h->types[t].numNodes + typeDelta[t] > 0)) { why = 2; break; }
  if (!why && rows->allocatable)
    for (int i = 0; i < n && !why; i++) {
      const int64_t* a = &eAlloc[(size_t)i * R]; const int64_t* tot = &h->nodeTotal[(size_t)rows->node[i] * R];
      if (h->allocLeTotal) for (int r = 0; r < R; r++) if (!d.cfg.isFloating[r] && (a[r] < 0 || a[r] > tot[r])) why = 3;   // (allocLeTotal keeps its value)
      for (int c = 0; c < K; c++) {
        const int64_t v = a[h->indexedCol[c]];
        if (v > h->keyMaxV[c] || v / h->indexedRes[c] > h->keyMaxQ[c]) why = 3;            // (beyond the widths layoutKeys chose)
        if (h->keyCoarse && v % d.cfg.indexedRes[c]) why = 3;                                // (the key's fields are exact quotients by the coarser divisor)
        if (h->allocAligned && v % h->indexedRes[c]) why = 3;                                // (a class matching several types would move to the literal path)
      }
    }
  const int M = h->jobsSet ? h->M : 0;
  if (why) {
    // ---- the rebuild path: the patched table, from the handle's mirrors, through nodes_upsert's own code
    std::vector<int64_t> alloc = h->nodeAllocHost;
    std::vector<uint8_t> uns = h->nodeUnsched, over = h->nodeOverAlloc;
    std::vector<int32_t> ofEntry(N, -1);
    for (int i = 0; i < n; i++) {
      const int v = rows->node[i];
      ofEntry[v] = i; uns[v] = eUns[i]; over[v] = eOver[i];
      for (int r = 0; r < R; r++) alloc[(size_t)v * R + r] = eAlloc[(size_t)i * R + r];
    }
    std::vector<int32_t> tOff(N + 1, 0), tKey, tVal, tEff, lOff(N + 1, 0), lKey, lVal;
    for (int v = 0; v < N; v++) {
      const std::vector<HTaint>& tv = ofEntry[v] >= 0 ? eTaints[ofEntry[v]] : h->nodeTaints[v];
      const size_t cnt = tv.size() - (uns[v] ? 1 : 0);   // (without the unschedulable taint: nodes_upsert adds it)
      for (size_t k = 0; k < cnt; k++) { tKey.push_back(tv[k].key); tVal.push_back(tv[k].value); tEff.push_back(tv[k].effect); }
      tOff[v + 1] = (int32_t)tKey.size();
      for (auto& l : h->nodeLabels[v]) { lKey.push_back(l.key); lVal.push_back(l.value); }
      lOff[v + 1] = (int32_t)lKey.size();
    }
    tKey.push_back(0); tVal.push_back(0); tEff.push_back(0); lKey.push_back(0); lVal.push_back(0);
    // what that code can refuse, decided first, with everything put back (rebuildRefusal)
    {
      std::vector<HType> typesAfter;
      for (size_t t = 0; t < h->types.size(); t++) if (h->types[t].numNodes + typeDelta[t] > 0) typesAfter.push_back(h->types[t]);
      for (auto& t : newTypes) typesAfter.push_back(t);
      std::string rwhy;
      if (int rrc = rebuildRefusal(h, typesAfter, alloc.data(), N, rwhy)) return fail(h, rrc, "nodes_patch: " + rwhy);
    }
    std::vector<uint64_t> index = h->nodeIndexHost; std::vector<int64_t> total = h->nodeTotal; std::vector<int32_t> idRank = h->nodeIdRank;
    asched_nodes in; memset(&in, 0, sizeof in);
    in.n = N; in.index = index.data(); in.id_rank = idRank.data(); in.total = total.data(); in.allocatable = alloc.data();
    in.unschedulable = uns.data(); in.over_allocated = over.data();
    in.taint_off = tOff.data(); in.taint_key = tKey.data(); in.taint_value = tVal.data(); in.taint_effect = tEff.data();
    in.label_off = lOff.data(); in.label_key = lKey.data(); in.label_value = lVal.data();
    memset(h->npStats, 0, sizeof h->npStats); plat_pass_clear(PASS_NP, h->npMs);
    int rc = nodesUpsertBody(h, &in);
    if (rc) return rc;
    h->npStats[0] = n; h->npStats[1] = typeChanged; h->npStats[2] = 1; h->npStats[3] = why;
    return M > 0 ? resetDynamicState(h, M) : 0;   // (both paths leave the per-job state as jobs_set does)
  }
  // ---- the device path.  One scratch block for the entries, kept and only ever grown, sized before anything changes: running out of device memory here is a refusal too
  const bool masks = h->jobsSet && h->dClassMask && h->dShapeClass;
  const int Cext = masks ? h->Cext : 0, CW = std::max(1, (Cext + 63) / 64);
  const size_t oType = up256(sizeof(int32_t) * (size_t)n), oWordOff = oType + up256(sizeof(int32_t) * (size_t)n), oWordIdx = oWordOff + up256(sizeof(int32_t) * ((size_t)n + 1)),
               oFlags = oWordIdx + up256(sizeof(int32_t) * (size_t)n), oAlloc = oFlags + up256((size_t)n), oCls = oAlloc + up256(sizeof(int64_t) * (size_t)n * R),
               need = oCls + up256(sizeof(uint64_t) * (size_t)n * CW);
  KeptBlock<char> scratch{h->npBufs, h->npScratch, h->npScratchBytes};
  if (n > 0 && !scratch.grow(need)) return fail(h, ASCHED_ERR_DEVICE, "nodes_patch: out of device memory for the patch entries; the handle is as it was");
  // ---- what nodes_upsert resets (the node table half patched: asched_nodes_upsert before anything else)
  residentTouchNodes(h);
  memset(h->npStats, 0, sizeof h->npStats); plat_pass_clear(PASS_NP, h->npMs);
  h->npStats[0] = n; h->npStats[1] = typeChanged;
  if (n > 0) {
    // the host mirrors, and the totals by difference (addNodeToStats, nodedb.go:44-55)
    std::vector<int32_t> ord(n);
    for (int i = 0; i < n; i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return rows->node[a] < rows->node[b]; });
    for (int i = 0; i < n; i++) {
      const int v = rows->node[i];
      for (int r = 0; r < R; r++) {
        const int64_t a = eAlloc[(size_t)i * R + r];
        if (!d.cfg.isFloating[r]) d.cfg.totalResources[r] += a - h->nodeAllocHost[(size_t)v * R + r];
        h->nodeAllocHost[(size_t)v * R + r] = a;
      }
      for (int c = 0; c < K; c++) { const int64_t a = eAlloc[(size_t)i * R + h->indexedCol[c]]; h->keyGcdV[c] = std::gcd(h->keyGcdV[c], a < 0 ? -a : a); }   // (stays a common divisor: layoutKeys of a later jobs_set / jobs_append)
      h->nodeTaints[v].swap(eTaints[i]); h->nodeUnsched[v] = eUns[i]; h->nodeOverAlloc[v] = eOver[i];
      h->types[h->nodeType[v]].numNodes--; h->types[eType[i]].numNodes++; h->nodeType[v] = eType[i];
    }
    // the entries, ascending by node and grouped by 64-node word; classMatchesNode for these rows only
    std::vector<int32_t> sNode(n), sType(n), wordOff, wordIdx;
    std::vector<uint8_t> sFlags(n);
    std::vector<int64_t> sAlloc((size_t)n * R);
    std::vector<uint64_t> sCls((size_t)n * CW, 0);
    for (int k = 0; k < n; k++) {
      const int i = ord[k], v = rows->node[i];
      sNode[k] = v; sType[k] = eType[i]; sFlags[k] = (eUns[i] && eOver[i]) ? 1 : 0;
      for (int r = 0; r < R; r++) sAlloc[(size_t)k * R + r] = eAlloc[(size_t)i * R + r];
      for (int c = 0; c < Cext; c++) if (classMatchesNode(h, c, v)) sCls[(size_t)k * CW + (c >> 6)] |= 1ull << (c & 63);
      if (wordIdx.empty() || wordIdx.back() != (v >> 6)) { wordIdx.push_back(v >> 6); wordOff.push_back(k); }
    }
    wordOff.push_back(n);
    NpArgs a; memset(&a, 0, sizeof a);
    a.n = n; a.nW = (int32_t)wordIdx.size(); a.CW = CW;
    char* s = h->npScratch;
    plat_h2d(s, sNode.data(), sizeof(int32_t) * (size_t)n); plat_h2d(s + oType, sType.data(), sizeof(int32_t) * (size_t)n);
    plat_h2d(s + oWordOff, wordOff.data(), sizeof(int32_t) * wordOff.size()); plat_h2d(s + oWordIdx, wordIdx.data(), sizeof(int32_t) * wordIdx.size());
    plat_h2d(s + oFlags, sFlags.data(), (size_t)n); plat_h2d(s + oAlloc, sAlloc.data(), sizeof(int64_t) * (size_t)n * R); plat_h2d(s + oCls, sCls.data(), sizeof(uint64_t) * (size_t)n * CW);
    a.pNode = (const int32_t*)s; a.pType = (const int32_t*)(s + oType); a.wordOff = (const int32_t*)(s + oWordOff); a.wordIdx = (const int32_t*)(s + oWordIdx);
    a.pFlags = (const uint8_t*)(s + oFlags); a.pAlloc = (const int64_t*)(s + oAlloc); a.pCls = (const uint64_t*)(s + oCls);
    if (masks) {
      a.Cext = Cext; a.Sext = h->S + (int)h->awayRowClass.size(); a.T = (int32_t)h->types.size();
      a.classMask = h->dClassMask; a.shapeClass = h->dShapeClass; a.nodeType = h->dNodeType;
      if (d.f.structOk && d.nodeCls) { a.nodeCls = d.nodeCls; a.clsLow = h->C >= 64 ? ~0ull : ((1ull << h->C) - 1); }
    }
    int prc = plat_take_failure() ? -1 : plat_nodes_patch(d, a);
    if (prc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    plat_pass_ms(PASS_NP, h->npMs);
    if (plat_pass_printed(PASS_NP))
      fprintf(stderr, "[asched nodes_patch] nodes %d entries %d words %d mask rows %d: scatter %.4f ms, mask words %.4f ms\n", N, n, a.nW, a.Cext + a.Sext + a.T, h->npMs[0], h->npMs[1]);
  }
  return resetDynamicState(h, M);
}
int32_t asched_nodes_patch_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->npStats[k];
  return 0;
}

// ---- asched_nodes_delete (kernels_nodes_delete.h): rows leave the resident node table — what populateNodeDb does every cycle to an unschedulable node that holds no
// job (scheduling_algo.go:1069-1077) and to the nodes of an executor it filters out (:1100-1169).  The handle is left as asched_nodes_upsert of the table without the
// named rows would leave it, with every run of the resident job table sent through the old -> new map.  Two paths, chosen per call, as in asched_nodes_patch: nothing
// the host derives from the WHOLE table can change (no node type and no value of an indexed label loses its last node) — the per-node arrays are gathered and the mask
// rows bit-compacted on the device; or the reduced table goes through nodes_upsert's own code (nodesUpsertBody) and only the jobs' nodes are remapped on the device.
int32_t asched_nodes_delete(asched_t* h, int32_t n, const int32_t* node, int32_t* new_id) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  const int N = h->N, R = h->R, P = h->P;
  Dev& d = h->dev;
  // ---- every refusal before anything changes
  if (!h->nodesSet || h->nodeAllocHost.size() != (size_t)N * R || h->nodeOverAlloc.size() != (size_t)N || h->nodeIndexHost.size() != (size_t)N)
    return fail(h, ASCHED_ERR_INVALID, "nodes_delete: no node table on this handle (nodes_upsert first)");
  if (n < 0 || (n > 0 && !node)) return fail(h, ASCHED_ERR_INVALID, "nodes_delete: bad arguments");
  if (h->uploadedAllocByPrio || h->hasTypeOverride) return fail(h, ASCHED_ERR_UNSUPPORTED, "nodes_delete: the node table was uploaded with alloc_by_prio or node_type_override (nodes_upsert instead)");
  if (h->npSeen.size() != (size_t)N) h->npSeen.assign(N, 0);
  std::vector<uint8_t>& gone = h->npSeen;   // [N] the rows of this call, until the mirrors are compacted
  auto ungone = [&](int upTo) { for (int i = 0; i < upTo; i++) gone[node[i]] = 0; };
  { int marked = 0; const char* why = nullptr;
    for (int i = 0; i < n; i++) {
      const int v = node[i];
      if (v < 0 || v >= N) { why = "nodes_delete: a row outside the node table"; break; }
      if (gone[v]) { why = "nodes_delete: a row named twice"; break; }
      gone[v] = 1; marked = i + 1;
    }
    if (why) { ungone(marked); return fail(h, ASCHED_ERR_INVALID, why); } }
  if (n > 0 && n == N) { ungone(n); return fail(h, ASCHED_ERR_UNSUPPORTED, "nodes_delete: every row of the table is named (a handle holds at least one node: nodes_upsert of the next table instead)"); }
  const int N1 = N - n, M = h->jobsSet ? h->M : 0;
  const int Npad = d.cfg.Npad, W = d.cfg.W;
  int Npad1 = ((N1 + 63) / 64) * 64; if (Npad1 == 0) Npad1 = 64;
  const int W1 = Npad1 / 64;
  // which path: a node type or a value of an indexed label that loses its last node changes what the host derives from the whole table
  int why = 0;
  std::vector<int> typeGone(h->types.size(), 0);
  std::vector<std::vector<int32_t>> valueGone(h->slotValueCount.size());
  for (size_t s = 0; s < valueGone.size(); s++) valueGone[s].assign(h->slotValueCount[s].size(), 0);
  auto slotValueOf = [&](size_t s, int32_t value) { const auto& vs = h->slotValues[s]; return (size_t)(std::lower_bound(vs.begin(), vs.end(), value) - vs.begin()); };
  for (int i = 0; i < n; i++) {
    const int v = node[i];
    typeGone[h->nodeType[v]]++;
    for (auto& l : h->nodeLabels[v]) for (size_t s = 0; s < h->labelSlots.size(); s++) if (l.key == h->labelSlots[s]) { const size_t k = slotValueOf(s, l.value); if (k < valueGone[s].size()) valueGone[s][k]++; }
  }
  // (an indexed label is part of the node type: a value that loses its last node empties a node type as well — the value is the reason reported then)
  for (size_t s = 0; s < valueGone.size() && !why; s++) for (size_t k = 0; k < valueGone[s].size(); k++) if (valueGone[s][k] > 0 && h->slotValueCount[s][k] - valueGone[s][k] <= 0) { why = 4; break; }
  for (size_t t = 0; t < h->types.size() && !why; t++) if (h->types[t].numNodes > 0 && h->types[t].numNodes - typeGone[t] <= 0) why = 2;
  // the reduced table of the rebuild path, and what nodes_upsert's code would refuse for it
  std::vector<int64_t> rAlloc, rTotal; std::vector<uint8_t> rUns, rOver; std::vector<uint64_t> rIndex; std::vector<int32_t> rIdRank, tOff, tKey, tVal, tEff, lOff, lKey, lVal;
  if (why) {
    tOff.push_back(0); lOff.push_back(0);
    for (int v = 0; v < N; v++) {
      if (gone[v]) continue;
      for (int r = 0; r < R; r++) { rAlloc.push_back(h->nodeAllocHost[(size_t)v * R + r]); rTotal.push_back(h->nodeTotal[(size_t)v * R + r]); }
      rUns.push_back(h->nodeUnsched[v]); rOver.push_back(h->nodeOverAlloc[v]); rIndex.push_back(h->nodeIndexHost[v]); rIdRank.push_back(h->nodeIdRank[v]);
      const std::vector<HTaint>& tv = h->nodeTaints[v];
      const size_t cnt = tv.size() - (h->nodeUnsched[v] ? 1 : 0);   // (without the unschedulable taint: nodes_upsert adds it)
      for (size_t k = 0; k < cnt; k++) { tKey.push_back(tv[k].key); tVal.push_back(tv[k].value); tEff.push_back(tv[k].effect); }
      tOff.push_back((int32_t)tKey.size());
      for (auto& l : h->nodeLabels[v]) { lKey.push_back(l.key); lVal.push_back(l.value); }
      lOff.push_back((int32_t)lKey.size());
    }
    tKey.push_back(0); tVal.push_back(0); tEff.push_back(0); lKey.push_back(0); lVal.push_back(0);
    std::vector<HType> typesAfter;
    for (size_t t = 0; t < h->types.size(); t++) if (h->types[t].numNodes - typeGone[t] > 0) typesAfter.push_back(h->types[t]);
    std::string rwhy;
    if (int rrc = rebuildRefusal(h, typesAfter, rAlloc.data(), N1, rwhy)) { ungone(n); return fail(h, rrc, "nodes_delete: " + rwhy); }
  }
  // ---- the scratch and every fresh block before anything changes: running out of device memory here is a refusal too.  The scratch: the entries | the survivors' list |
  // the new positions | the check word.  The blocks keep the sizes of the ones they replace (block sizes do not shrink); only the strides inside them change
  const bool masks = !why && h->jobsSet && h->dClassMask && h->dShapeClass;
  const bool haveFast = !why && h->jobsSet && d.f.structOk && d.nodeCls;
  const int Sext = masks ? h->S + (int)h->awayRowClass.size() : 0, labelRows = masks && !h->uniOffHost.empty() ? h->uniOffHost.back() : 0;
  const size_t oSrc = up256(sizeof(int32_t) * (size_t)n), oNew = oSrc + up256(sizeof(int32_t) * (size_t)N), oBad = oNew + up256(sizeof(int32_t) * (size_t)N), need = oBad + 256;
  StagedBlocks sb;   // (every block starts as zeros; the keys as 0xff bytes)
  KeptBlock<char> scratch{h->ndBufs, h->ndScratch, h->ndScratchBytes};
  KeptBlock<uint8_t> keep{h->ndBufs, h->ndKeep, h->ndKeepCap};   // the keep flags: [N] exactly, all 1 between calls
  if (n > 0) {
    if (!why) {
      const size_t np = (size_t)Npad;
      sb.stage(&h->nodeBufs, &d.totalRes, 8 * R * np); sb.stage(&h->nodeBufs, &d.allocatable, 8 * R * np); sb.stage(&h->nodeBufs, &d.alloc, 8 * (size_t)P * R * np);
      sb.stage(&h->nodeBufs, &d.keys, 8 * 2 * (size_t)P * np, 0xff);
      sb.stage(&h->nodeBufs, &d.nodeFlags, (size_t)N); sb.stage(&h->nodeBufs, &d.idxRank, 4 * (size_t)N); sb.stage(&h->nodeBufs, &d.nodeByRank, 4 * (size_t)N); sb.stage(&h->nodeBufs, &d.nodeIdRank, 4 * (size_t)N);
      sb.stage(&h->nodeBufs, &d.accAvail, 8 * np * R); sb.stage(&h->nodeBufs, &d.accStamp, 4 * np); sb.stage(&h->nodeBufs, &d.accStaticFailed, np);
      sb.stage(&h->nodeBufs, &d.fairOff, 4 * (np + 2)); sb.stage(&h->nodeBufs, &d.nodeOver, 4 * np);
      if (masks) {
        sb.stage(&h->maskBufs, &h->dClassMask, 8 * (size_t)h->Cext * W); sb.stage(&h->maskBufs, &d.shapeMask, 8 * (size_t)std::max(Sext, 1) * W);
        sb.stage(&h->maskBufs, &d.typeMask, 8 * std::max<size_t>(h->types.size(), 1) * W); sb.stage(&h->maskBufs, &d.labelMask, 8 * (size_t)std::max(labelRows, 1) * W);
        sb.stage(&h->maskBufs, &h->dNodeType, 4 * (size_t)N);
      }
      if (haveFast) sb.stage(&h->fastBufs, &d.nodeCls, 8 * (size_t)N);
    }
    if (!(scratch.tryGrow(need) && keep.tryGrow((size_t)N, false) && sb.allocate())) {
      scratch.drop(); keep.drop();
      ungone(n);
      return fail(h, ASCHED_ERR_DEVICE, "nodes_delete: out of device memory for the scratch and the compacted node table; the handle is as it was");
    }
    scratch.adopt();
    if (keep.adopt()) plat_memset(h->ndKeep, 1, (size_t)N);
  }
  // ---- mark and check: a running job on a named row is the last refusal, read from the device before anything else is written
  NdArgs a; memset(&a, 0, sizeof a);
  if (n > 0) {
    a.N = N; a.N1 = N1; a.n = n; a.R = R; a.M = M; a.Npad = Npad; a.Npad1 = Npad1; a.W = W; a.W1 = W1;
    int32_t* e32 = (int32_t*)h->ndScratch;
    plat_h2d(e32, node, sizeof(int32_t) * (size_t)n);
    a.node = e32; a.keep = h->ndKeep; a.src = (int32_t*)(h->ndScratch + oSrc); a.newId = (uint32_t*)(h->ndScratch + oNew); a.bad = (int32_t*)(h->ndScratch + oBad);
    a.jNode0 = M > 0 ? d.jNode0 : nullptr; a.jrec = (M > 0 && d.f.structOk && d.jrec) ? d.jrec : nullptr;
    int32_t bad = ND_NONE;
    const int crc = plat_take_failure() ? -1 : plat_nodes_delete_check(d, a, &bad);
    if (crc || bad != ND_NONE) {
      sb.drop();
      ungone(n);
      if (crc) { h->ndBufs.freeAll(); h->ndKeep = nullptr; h->ndKeepCap = 0; h->ndScratch = nullptr; h->ndScratchBytes = 0; return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
      return fail(h, ASCHED_ERR_INVALID, "nodes_delete: job row " + std::to_string(bad) + " runs on a named node (say what became of the run first: jobs_patch with node -1, or jobs_delete)");
    }
  }
  // ---- what nodes_upsert resets (the tables half compacted: asched_nodes_upsert and asched_jobs_set before anything else)
  residentTouchNodes(h);
  memset(h->ndStats, 0, sizeof h->ndStats); plat_pass_clear(PASS_ND, h->ndMs);
  int renumbered = 0;
  if (n > 0) {
    sb.fill();
    a.jobsOnly = why ? 1 : 0;
    if (!why) {
      a.inTotal = d.totalRes; a.outTotal = (int64_t*)sb.fresh(&d.totalRes); a.inAlloc = d.allocatable; a.outAlloc = (int64_t*)sb.fresh(&d.allocatable);
      a.inFlags = d.nodeFlags; a.outFlags = (uint8_t*)sb.fresh(&d.nodeFlags); a.inIdRank = d.nodeIdRank; a.outIdRank = (int32_t*)sb.fresh(&d.nodeIdRank);
      a.rankIn = d.nodeByRank; a.rankOut = (int32_t*)sb.fresh(&d.nodeByRank); a.idxRankOut = (int32_t*)sb.fresh(&d.idxRank);
      if (masks) {
        a.inType = h->dNodeType; a.outType = (int32_t*)sb.fresh(&h->dNodeType);
        const uint64_t* in[ND_MASKS] = {h->dClassMask, d.shapeMask, d.typeMask, d.labelMask};
        void* sl[ND_MASKS] = {&h->dClassMask, &d.shapeMask, &d.typeMask, &d.labelMask};
        const int rows[ND_MASKS] = {h->Cext, Sext, (int)h->types.size(), labelRows};
        for (int k = 0; k < ND_MASKS; k++) { a.inMask[k] = in[k]; a.outMask[k] = (uint64_t*)sb.fresh(sl[k]); a.rows[k] = rows[k]; }
      }
      if (haveFast) { a.inCls = d.nodeCls; a.outCls = (uint64_t*)sb.fresh(&d.nodeCls); }
    }
    const int prc = plat_take_failure() ? -1 : plat_nodes_delete(d, a);
    if (prc) {
      sb.drop();
      gone.assign(N, 0);
      h->ndBufs.freeAll(); h->ndKeep = nullptr; h->ndKeepCap = 0; h->ndScratch = nullptr; h->ndScratchBytes = 0;
      return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    }
    plat_pass_ms(PASS_ND, h->ndMs);
    // the old -> new map on the host: the scan's exclusive prefix, -1 for the rows that left
    h->ndMap.resize(N);
    plat_d2h(h->ndMap.data(), a.newId, sizeof(int32_t) * (size_t)N);
    for (int i = 0; i < n; i++) h->ndMap[node[i]] = -1;
    if (new_id) memcpy(new_id, h->ndMap.data(), sizeof(int32_t) * (size_t)N);
    if (M > 0) {   // the jNode mirror, on the host threads asched_jobs_delete uses
      const int first = *std::min_element(node, node + n);
      std::atomic<int> cnt{0};
      parallelChunks((size_t)M, M < 65536 ? 1 : (size_t)hostThreads(), [&](size_t lo, size_t hi) {
        int c = 0;
        for (size_t j = lo; j < hi; j++) { const int v = h->jNode[j]; if (v > first && v < N) { h->jNode[j] = h->ndMap[v]; c++; } }
        cnt += c;
      });
      renumbered = cnt;
    }
    if (why) {
      // ---- the rebuild path: the reduced table, from the handle's mirrors, through nodes_upsert's own code (the job table's nodes are already renumbered)
      gone.assign(N1, 0);
      asched_nodes in; memset(&in, 0, sizeof in);
      in.n = N1; in.index = rIndex.data(); in.id_rank = rIdRank.data(); in.total = rTotal.data(); in.allocatable = rAlloc.data();
      in.unschedulable = rUns.data(); in.over_allocated = rOver.data();
      in.taint_off = tOff.data(); in.taint_key = tKey.data(); in.taint_value = tVal.data(); in.taint_effect = tEff.data();
      in.label_off = lOff.data(); in.label_key = lKey.data(); in.label_value = lVal.data();
      int rc = nodesUpsertBody(h, &in);
      if (rc) return rc;
    } else {
      // ---- the device path: the blocks swapped in, the old ones released (plat_nodes_delete has waited for the device)
      sb.commit();
      // scratch indexed by node that lives in the fast structure: the start a fresh nodes_upsert + jobs_set gives it (zeros), over the whole block
      if (haveFast) {
        void* scr[] = {d.baseKey, d.baseNode, d.baseExtra, d.baseCls, d.baseRemoved, d.posOf, d.l0Slot, d.fitBits};
        for (void* p : scr) if (p) for (auto& e : h->fastBufs.ptrs) if (e.first == p) { plat_memset(p, 0, e.second); break; }
      }
      // the host mirrors, compacted in place (row order is kept: every element moves down or stays); the totals and the counts by difference (addNodeToStats, nodedb.go:44-55)
      for (int i = 0; i < n; i++) {
        const int v = node[i];
        for (int r = 0; r < R; r++) if (!d.cfg.isFloating[r]) d.cfg.totalResources[r] -= h->nodeAllocHost[(size_t)v * R + r];
      }
      for (size_t t = 0; t < h->types.size(); t++) h->types[t].numNodes -= typeGone[t];
      for (size_t s = 0; s < valueGone.size(); s++) for (size_t k = 0; k < valueGone[s].size(); k++) h->slotValueCount[s][k] -= valueGone[s][k];
      { auto squeeze = [&](auto& v, size_t w) {
          size_t o = 0;
          for (size_t i = 0; i < (size_t)N; i++) if (!gone[i]) { if (o != i) for (size_t x = 0; x < w; x++) v[o * w + x] = std::move(v[i * w + x]); o++; }
          v.resize((size_t)N1 * w);
        };
        squeeze(h->nodeTaints, 1); squeeze(h->nodeLabels, 1); squeeze(h->nodeType, 1); squeeze(h->nodeTotal, (size_t)R); squeeze(h->nodeAllocHost, (size_t)R);
        squeeze(h->nodeIndexHost, 1); squeeze(h->nodeOverAlloc, 1); squeeze(h->nodeUnsched, 1); squeeze(h->nodeIdRank, 1); }
      { size_t o = 0;
        for (size_t i = 0; i < (size_t)N; i++) { const int v = h->nodeByRank[i]; if (h->ndMap[v] >= 0) h->nodeByRank[o++] = h->ndMap[v]; }
        h->nodeByRank.resize(N1); }
      gone.assign(N1, 0);
      h->N = N1; d.cfg.N = N1; d.cfg.Npad = Npad1; d.cfg.W = W1;
      if (haveFast) d.fitW = (N1 + 63) / 64;
      if (h->jobsSet) exclSetup(h);   // (the [cap][W] bit rows of the failed-selection store: B_RESET_JOBS forgets the records anyway)
    }
    if (plat_pass_printed(PASS_ND))
      fprintf(stderr, "[asched nodes_delete] nodes %d entries %d jobs %d mask rows %d path %s: mark + check %.4f ms, scan %.4f ms, gather %.4f ms, index order %.4f ms, mask rows %.4f ms, job remap %.4f ms, unmark %.4f ms\n",
              N, n, M, a.rows[0] + a.rows[1] + a.rows[2] + a.rows[3], why ? "rebuild" : "device", h->ndMs[0], h->ndMs[1], h->ndMs[2], h->ndMs[3], h->ndMs[4], h->ndMs[5], h->ndMs[6]);
  }
  if (n == 0 && new_id) for (int i = 0; i < N; i++) new_id[i] = i;   // (no pass ran: every row keeps its position)
  h->ndStats[0] = n; h->ndStats[1] = renumbered; h->ndStats[2] = why ? 1 : 0; h->ndStats[3] = why; h->ndStats[4] = h->N;
  memset(h->npStats, 0, sizeof h->npStats);
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return resetDynamicState(h, M);
}
int32_t asched_nodes_delete_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->ndStats[k];
  return 0;
}

// ---- asched_nodes_append (kernels_nodes_append.h): new rows join the resident node table — what populateNodeDb does every cycle with the nodes the healthy executors
// report (scheduling_algo.go:1019-1098), an executor that returns from the filters at :1100-1169 and a drained node that is uncordoned.  The handle is left as
// asched_nodes_upsert of "the N resident rows in their order, then the m new rows" would leave it.  Two paths, chosen per call, as in asched_nodes_patch and
// asched_nodes_delete: nothing the host derives from the WHOLE table changes — every block that depends on N, Npad or W is written into a fresh block of the new size
// on the device and swapped in; or the grown table goes through nodes_upsert's own code (nodesUpsertBody).
int32_t asched_nodes_append(asched_t* h, const asched_nodes_append_rows* rows) {
  if (!h) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  if (!rows) return fail(h, ASCHED_ERR_INVALID, "nodes_append: bad arguments");
  HostProf prof("nodes_append");   // ASCHED_HOSTPROF=1: where the host's share of the call goes
  const int N = h->N, R = h->R, K = h->K, P = h->P, m = rows->m;
  Dev& d = h->dev;
  // ---- every refusal before anything changes
  if (!h->nodesSet || h->nodeAllocHost.size() != (size_t)N * R || h->nodeOverAlloc.size() != (size_t)N || h->nodeIndexHost.size() != (size_t)N)
    return fail(h, ASCHED_ERR_INVALID, "nodes_append: no node table on this handle (nodes_upsert first)");
  if (m < 0 || (m > 0 && (!rows->index || !rows->total || !rows->allocatable))) return fail(h, ASCHED_ERR_INVALID, "nodes_append: bad arguments");
  if (h->uploadedAllocByPrio || h->hasTypeOverride) return fail(h, ASCHED_ERR_UNSUPPORTED, "nodes_append: the node table was uploaded with alloc_by_prio or node_type_override (nodes_upsert instead)");
  { auto ascending = [&](const int32_t* off) { if (m > 0 && off[0] < 0) return false; for (int i = 0; i < m; i++) if (off[i + 1] < off[i]) return false; return true; };
    if (rows->taint_off) {
      if (!ascending(rows->taint_off)) return fail(h, ASCHED_ERR_INVALID, "nodes_append: taint_off is not ascending");
      if (m > 0 && rows->taint_off[m] > 0 && (!rows->taint_key || !rows->taint_value || !rows->taint_effect)) return fail(h, ASCHED_ERR_INVALID, "nodes_append: bad arguments");
    }
    if (rows->label_off) {
      if (!ascending(rows->label_off)) return fail(h, ASCHED_ERR_INVALID, "nodes_append: label_off is not ascending");
      if (m > 0 && rows->label_off[m] > 0 && (!rows->label_key || !rows->label_value)) return fail(h, ASCHED_ERR_INVALID, "nodes_append: bad arguments");
    } }
  if ((long long)N + m > (1ll << 30)) return fail(h, ASCHED_ERR_UNSUPPORTED, "nodes_append: more than 2^30 nodes");
  if (m > 0 && !h->idRanksGiven && rows->id_rank && !rows->id_rank_all)
    return fail(h, ASCHED_ERR_INVALID, "nodes_append: the node table was uploaded without id ranks, so id_rank has no rank space to lie in (id_rank_all, or no ranks)");
  const int N1 = N + m, M = h->jobsSet ? h->M : 0;
  const int Npad = d.cfg.Npad, W = d.cfg.W;
  int Npad1 = ((N1 + 63) / 64) * 64; if (Npad1 == 0) Npad1 = 64;
  const int W1 = Npad1 / 64;
  // the index order: the new rows ascending by node.index and each one's insertion point among the resident ranks (the resident rows with a smaller index)
  std::vector<int32_t> ord(m), ins(m);
  for (int i = 0; i < m; i++) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return rows->index[a] < rows->index[b]; });
  for (int k = 0; k < m; k++) {
    const uint64_t x = rows->index[ord[k]];
    if (k > 0 && rows->index[ord[k - 1]] == x) return fail(h, ASCHED_ERR_INVALID, "nodes_append: two new rows with the same node index");
    const auto it = std::lower_bound(h->nodeByRank.begin(), h->nodeByRank.end(), x, [&](int32_t v, uint64_t key) { return h->nodeIndexHost[v] < key; });
    if (it != h->nodeByRank.end() && h->nodeIndexHost[*it] == x) return fail(h, ASCHED_ERR_INVALID, "nodes_append: a new row with the node index of a resident row");
    ins[k] = (int32_t)(it - h->nodeByRank.begin());
  }
  // ---- the state of every new row, and which path serves the call
  std::vector<std::vector<HTaint>> eTaints(m); std::vector<std::vector<HSel>> eLabels(m);
  std::vector<uint8_t> eUns(m), eOver(m);
  std::vector<int> eType(m, -1);
  std::vector<int32_t> eIdRank(m);
  std::vector<HType> newTypes; std::vector<std::string> newCanon;   // node types the table does not have, in order of first occurrence
  std::vector<int> typeAdd(h->types.size(), 0);
  std::vector<std::vector<int32_t>> valueAdd(h->slotValueCount.size());
  for (size_t s = 0; s < valueAdd.size(); s++) valueAdd[s].assign(h->slotValueCount[s].size(), 0);
  const size_t L = h->labelSlots.size();
  std::vector<int32_t> eLab((size_t)m * std::max<size_t>(L, 1), -1);   // per entry and label slot: the value's position in slotValues, -1
  bool newValue = false;
  { int32_t behind = 0;
    if (!rows->id_rank && !rows->id_rank_all && m > 0) for (int32_t r : h->nodeIdRank) behind = std::max(behind, r < INT32_MAX ? r + 1 : r);
    for (int i = 0; i < m; i++) {
      eUns[i] = rows->unschedulable && rows->unschedulable[i] ? 1 : 0;
      eOver[i] = rows->over_allocated && rows->over_allocated[i] ? 1 : 0;
      if (rows->taint_off) for (int k = rows->taint_off[i]; k < rows->taint_off[i + 1]; k++) eTaints[i].push_back({rows->taint_key[k], rows->taint_value[k], rows->taint_effect[k]});
      if (eUns[i]) eTaints[i].push_back({kUnschedulableTaintKey, 0, ASCHED_EFFECT_NO_SCHEDULE});  // node.go:127-129
      if (rows->label_off) for (int k = rows->label_off[i]; k < rows->label_off[i + 1]; k++) eLabels[i].push_back({rows->label_key[k], rows->label_value[k]});
      eIdRank[i] = rows->id_rank_all ? rows->id_rank_all[N + i] : rows->id_rank ? rows->id_rank[i] : behind + i;
      HType t; std::string canon;
      nodeTypeOf(h, eTaints[i], eLabels[i], t, canon);
      auto it = h->typeByCanon.find(canon);
      if (it != h->typeByCanon.end()) { eType[i] = it->second; typeAdd[it->second]++; }
      else {
        size_t k = 0;
        while (k < newCanon.size() && newCanon[k] != canon) k++;
        if (k == newCanon.size()) { newCanon.push_back(canon); newTypes.push_back(t); }
        newTypes[k].numNodes++;
      }
      for (auto& l : eLabels[i]) for (size_t s = 0; s < L; s++) if (l.key == h->labelSlots[s]) {
        const auto& vs = h->slotValues[s];
        const size_t k = (size_t)(std::lower_bound(vs.begin(), vs.end(), l.value) - vs.begin());
        if (k < vs.size() && vs[k] == l.value && h->slotValueCount[s][k] > 0) { valueAdd[s][k]++; eLab[(size_t)i * L + s] = (int32_t)k; }
        else newValue = true;
      }
    } }
  int why = 0;
  // (an indexed label is part of the node type: a new value is a new node type as well — the value is the reason reported then, as asched_nodes_delete does)
  if (newValue) why = 4;
  if (!why && !newTypes.empty()) why = 1;
  if (!why) for (size_t t = 0; t < h->types.size(); t++) if (typeAdd[t] > 0 && h->types[t].numNodes <= 0) { why = 2; break; }
  if (!why && N1 > 1 && d.cfg.idxBits < 64 && ((uint64_t)(N1 - 1) >> d.cfg.idxBits)) why = 5;   // (the rank field of the key layout holds N + m - 1)
  if (!why)
    for (int i = 0; i < m && !why; i++) {   // asched_nodes_patch's condition on a new allocatable row
      const int64_t* a = rows->allocatable + (size_t)i * R; const int64_t* tot = rows->total + (size_t)i * R;
      if (h->allocLeTotal) for (int r = 0; r < R; r++) if (!d.cfg.isFloating[r] && (a[r] < 0 || a[r] > tot[r])) why = 3;   // (allocLeTotal keeps its value)
      for (int c = 0; c < K; c++) {
        const int64_t v = a[h->indexedCol[c]];
        if (v > h->keyMaxV[c] || v / h->indexedRes[c] > h->keyMaxQ[c]) why = 3;            // (beyond the widths layoutKeys chose)
        if (h->keyCoarse && v % d.cfg.indexedRes[c]) why = 3;                                // (the key's fields are exact quotients by the coarser divisor)
        if (h->allocAligned && v % h->indexedRes[c]) why = 3;                                // (a class matching several types would move to the literal path)
      }
    }
  // id order == index order on the merged index order, decided before anything changes: with id_rank a new row's rank lies between its neighbours'; with id_rank_all
  // one pass over the N + m ranks
  // monoGiven: what nodes_upsert of the grown table computes (the rebuild path and its refusals go by it); monoAfter: what the device path keeps
  bool monoAfter = h->idRankMonotone, monoGiven = h->idRankMonotone;
  const bool noRanks = !h->idRanksGiven && !rows->id_rank_all;   // the table has no id ranks and gets none: id order == index order by definition, as in nodes_upsert
  if (m > 0 && rows->id_rank_all) {
    monoAfter = true;
    int32_t prev = INT32_MIN; int k = 0;
    for (int r = 0; r <= N && monoAfter; r++) {
      for (; k < m && ins[k] == r; k++) { const int32_t x = rows->id_rank_all[N + ord[k]]; if (x < prev) monoAfter = false; prev = x; }
      if (r < N) { const int32_t x = rows->id_rank_all[h->nodeByRank[r]]; if (x < prev) monoAfter = false; prev = x; }
    }
    monoGiven = monoAfter;
    if (!h->idRankMonotone) monoAfter = false;   // (stays conservative: a layout chosen for literal rows serves the others as well)
  } else if (monoAfter && !noRanks) {
    for (int k = 0; k < m && monoAfter; k++) {
      const int32_t x = eIdRank[ord[k]];
      if (k > 0 && ins[k - 1] == ins[k]) { if (x < eIdRank[ord[k - 1]]) monoAfter = false; }
      else if (ins[k] > 0 && x < h->nodeIdRank[h->nodeByRank[ins[k] - 1]]) monoAfter = false;
      if (!(k + 1 < m && ins[k + 1] == ins[k]) && ins[k] < N && h->nodeIdRank[h->nodeByRank[ins[k]]] < x) monoAfter = false;
    }
    monoGiven = monoAfter;
  }
  if (!why && h->idRankMonotone && !monoAfter) why = 3;
  if (why) {
    // ---- the rebuild path: the grown table, from the handle's mirrors and the new rows, through nodes_upsert's own code
    std::vector<int64_t> alloc = h->nodeAllocHost, total = h->nodeTotal;
    std::vector<uint8_t> uns = h->nodeUnsched, over = h->nodeOverAlloc;
    std::vector<uint64_t> index = h->nodeIndexHost;
    std::vector<int32_t> idRank = h->nodeIdRank;
    alloc.insert(alloc.end(), rows->allocatable, rows->allocatable + (size_t)m * R); total.insert(total.end(), rows->total, rows->total + (size_t)m * R);
    uns.insert(uns.end(), eUns.begin(), eUns.end()); over.insert(over.end(), eOver.begin(), eOver.end());
    index.insert(index.end(), rows->index, rows->index + m);
    if (rows->id_rank_all) idRank.assign(rows->id_rank_all, rows->id_rank_all + N1); else idRank.insert(idRank.end(), eIdRank.begin(), eIdRank.end());
    std::vector<int32_t> tOff(N1 + 1, 0), tKey, tVal, tEff, lOff(N1 + 1, 0), lKey, lVal;
    for (int v = 0; v < N1; v++) {
      const std::vector<HTaint>& tv = v < N ? h->nodeTaints[v] : eTaints[v - N];
      const size_t cnt = tv.size() - (uns[v] ? 1 : 0);   // (without the unschedulable taint: nodes_upsert adds it)
      for (size_t k = 0; k < cnt; k++) { tKey.push_back(tv[k].key); tVal.push_back(tv[k].value); tEff.push_back(tv[k].effect); }
      tOff[v + 1] = (int32_t)tKey.size();
      for (auto& l : (v < N ? h->nodeLabels[v] : eLabels[v - N])) { lKey.push_back(l.key); lVal.push_back(l.value); }
      lOff[v + 1] = (int32_t)lKey.size();
    }
    tKey.push_back(0); tVal.push_back(0); tEff.push_back(0); lKey.push_back(0); lVal.push_back(0);
    // what that code can refuse, decided first, with everything put back (rebuildRefusal).  Unlike for a reduced table it CAN fire here
    {
      std::vector<HType> typesAfter;
      for (size_t t = 0; t < h->types.size(); t++) if (h->types[t].numNodes + typeAdd[t] > 0) typesAfter.push_back(h->types[t]);
      for (auto& t : newTypes) typesAfter.push_back(t);
      std::string rwhy;
      const bool monoSaved = h->idRankMonotone;
      h->idRankMonotone = monoGiven;
      const int rrc = rebuildRefusal(h, typesAfter, alloc.data(), N1, rwhy);
      h->idRankMonotone = monoSaved;
      if (rrc) return fail(h, rrc, "nodes_append: " + rwhy);
    }
    asched_nodes in; memset(&in, 0, sizeof in);
    in.n = N1; in.index = index.data(); in.id_rank = noRanks ? nullptr : idRank.data(); in.total = total.data(); in.allocatable = alloc.data();
    in.unschedulable = uns.data(); in.over_allocated = over.data();
    in.taint_off = tOff.data(); in.taint_key = tKey.data(); in.taint_value = tVal.data(); in.taint_effect = tEff.data();
    in.label_off = lOff.data(); in.label_key = lKey.data(); in.label_value = lVal.data();
    memset(h->naStats, 0, sizeof h->naStats); plat_pass_clear(PASS_NA, h->naMs);
    memset(h->npStats, 0, sizeof h->npStats); memset(h->ndStats, 0, sizeof h->ndStats);
    int rc = nodesUpsertBody(h, &in);
    if (rc) return rc;
    h->naStats[0] = m; h->naStats[1] = Npad1 != Npad ? 1 : 0; h->naStats[2] = 1; h->naStats[3] = why; h->naStats[4] = h->N;
    return M > 0 ? resetDynamicState(h, M) : 0;   // (both paths leave the per-job state as jobs_set does)
  }
  // ---- the device path.  The scratch for the entries and every fresh block before anything changes: running out of device memory here is a refusal too.  Blocks that
  // hold the table are always fresh (nothing is changed in place); blocks of node-indexed scratch that are large enough already (block sizes do not shrink) are zeroed
  prof.lap("refusals and the choice of the path");
  const bool masks = h->jobsSet && h->dClassMask && h->dShapeClass;
  const bool haveFast = h->jobsSet && d.f.structOk && d.nodeCls;
  const int Cext = masks ? h->Cext : 0, CW = std::max(1, (Cext + 63) / 64);
  const int Sext = masks ? h->S + (int)h->awayRowClass.size() : 0, T = masks ? (int)h->types.size() : 0, labelRows = masks && !h->uniOffHost.empty() ? h->uniOffHost.back() : 0;
  const size_t mm = (size_t)m;
  const size_t oAlloc = up256(8 * mm * R), oIdRank = oAlloc + up256(8 * mm * R), oType = oIdRank + up256(4 * mm), oIns = oType + up256(4 * mm), oInsRow = oIns + up256(4 * mm),
               oLab = oInsRow + up256(4 * mm), oCls = oLab + up256(4 * mm * std::max<size_t>(L, 1)), oFlags = oCls + up256(8 * mm * CW), oAll = oFlags + up256(mm),
               need = oAll + (rows->id_rank_all ? up256(4 * (size_t)N1) : 0) + 256;
  StagedBlocks sb; std::vector<std::pair<void*, size_t>> zeroed;   // (every block starts as zeros; the keys as 0xff bytes)
  KeptBlock<char> entries{h->naBufs, h->naScratch, h->naScratchBytes};
  if (m > 0) {
    auto scratch = [&](DevBufs* owner, void* slot, size_t bytes) {   // node-indexed scratch: zeros of at least `bytes`
      void* p = *(void**)slot;
      for (auto& e : owner->ptrs) if (p && e.first == p && e.second >= bytes) { zeroed.push_back({p, e.second}); return; }
      sb.stage(owner, slot, bytes);
    };
    const size_t np = (size_t)Npad1, n1 = (size_t)N1;
    sb.stage(&h->nodeBufs, &d.totalRes, 8 * R * np); sb.stage(&h->nodeBufs, &d.allocatable, 8 * R * np); sb.stage(&h->nodeBufs, &d.alloc, 8 * (size_t)P * R * np);
    sb.stage(&h->nodeBufs, &d.keys, 8 * 2 * (size_t)P * np, 0xff);
    sb.stage(&h->nodeBufs, &d.nodeFlags, n1); sb.stage(&h->nodeBufs, &d.idxRank, 4 * n1); sb.stage(&h->nodeBufs, &d.nodeByRank, 4 * n1); sb.stage(&h->nodeBufs, &d.nodeIdRank, 4 * n1);
    scratch(&h->nodeBufs, &d.accAvail, 8 * np * R); scratch(&h->nodeBufs, &d.accStamp, 4 * np); scratch(&h->nodeBufs, &d.accStaticFailed, np);
    scratch(&h->nodeBufs, &d.fairOff, 4 * (np + 2)); scratch(&h->nodeBufs, &d.nodeOver, 4 * np);
    if (masks) {
      sb.stage(&h->maskBufs, &h->dClassMask, 8 * (size_t)std::max(Cext, 1) * W1); sb.stage(&h->maskBufs, &d.shapeMask, 8 * (size_t)std::max(Sext, 1) * W1);
      sb.stage(&h->maskBufs, &d.typeMask, 8 * (size_t)std::max(T, 1) * W1); sb.stage(&h->maskBufs, &d.labelMask, 8 * (size_t)std::max(labelRows, 1) * W1);
      sb.stage(&h->maskBufs, &h->dNodeType, 4 * n1);
    }
    if (haveFast) {
      size_t Nb2 = 64;
      while (Nb2 < n1) Nb2 <<= 1;
      sb.stage(&h->fastBufs, &d.nodeCls, 8 * n1);
      scratch(&h->fastBufs, &d.baseKey, 8 * Nb2); scratch(&h->fastBufs, &d.baseNode, 4 * np); scratch(&h->fastBufs, &d.baseExtra, 8 * np * MAXE); scratch(&h->fastBufs, &d.baseCls, 8 * np);
      scratch(&h->fastBufs, &d.baseRemoved, np); scratch(&h->fastBufs, &d.posOf, 4 * np); scratch(&h->fastBufs, &d.l0Slot, 4 * np);
      if (d.fitBits) scratch(&h->fastBufs, &d.fitBits, 8 * ((size_t)d.f.F * ((n1 + 63) / 64) + 64));
    }
    if (!(entries.tryGrow(need) && sb.allocate())) {
      entries.drop();
      return fail(h, ASCHED_ERR_DEVICE, "nodes_append: out of device memory for the scratch and the grown node table; the handle is as it was");
    }
    entries.adopt();
  }
  prof.lap("allocations");
  // ---- what nodes_upsert resets (the handle between two tables: asched_nodes_upsert before anything else)
  residentTouchNodes(h);
  memset(h->naStats, 0, sizeof h->naStats); plat_pass_clear(PASS_NA, h->naMs);
  memset(h->npStats, 0, sizeof h->npStats); memset(h->ndStats, 0, sizeof h->ndStats);
  if (m > 0) {
    // the host mirrors first (classMatchesNode reads them); the totals and the counts by addition (addNodeToStats, nodedb.go:44-55)
    h->nodeTaints.resize(N1); h->nodeLabels.resize(N1); h->nodeType.resize(N1);
    for (int i = 0; i < m; i++) {
      h->nodeTaints[N + i].swap(eTaints[i]); h->nodeLabels[N + i].swap(eLabels[i]); h->nodeType[N + i] = eType[i];
      h->types[eType[i]].numNodes++;
      for (int r = 0; r < R; r++) if (!d.cfg.isFloating[r]) d.cfg.totalResources[r] += rows->allocatable[(size_t)i * R + r];
      for (int c = 0; c < K; c++) { const int64_t a = rows->allocatable[(size_t)i * R + h->indexedCol[c]]; h->keyGcdV[c] = std::gcd(h->keyGcdV[c], a < 0 ? -a : a); }   // (stays a common divisor: layoutKeys of a later jobs_set / jobs_append)
    }
    for (size_t s = 0; s < valueAdd.size(); s++) for (size_t k = 0; k < valueAdd[s].size(); k++) h->slotValueCount[s][k] += valueAdd[s][k];
    h->nodeTotal.insert(h->nodeTotal.end(), rows->total, rows->total + (size_t)m * R);
    h->nodeAllocHost.insert(h->nodeAllocHost.end(), rows->allocatable, rows->allocatable + (size_t)m * R);
    h->nodeIndexHost.insert(h->nodeIndexHost.end(), rows->index, rows->index + m);
    h->nodeOverAlloc.insert(h->nodeOverAlloc.end(), eOver.begin(), eOver.end()); h->nodeUnsched.insert(h->nodeUnsched.end(), eUns.begin(), eUns.end());
    if (rows->id_rank_all) h->nodeIdRank.assign(rows->id_rank_all, rows->id_rank_all + N1); else h->nodeIdRank.insert(h->nodeIdRank.end(), eIdRank.begin(), eIdRank.end());
    h->idRankMonotone = monoAfter;
    if (rows->id_rank_all) h->idRanksGiven = true;
    { std::vector<int32_t> merged(N1);   // nodeByRank, merged as the device merges it
      int k = 0, o = 0;
      for (int r = 0; r <= N; r++) { for (; k < m && ins[k] == r; k++) merged[o++] = N + ord[k]; if (r < N) merged[o++] = h->nodeByRank[r]; }
      h->nodeByRank.swap(merged); }
    h->npSeen.assign(N1, 0);
    // the entries: class bits by classMatchesNode for the m rows only, the label rows of each entry
    std::vector<uint8_t> sFlags(m);
    std::vector<int32_t> sType(eType.begin(), eType.end()), insRow(m), sLab((size_t)m * std::max<size_t>(L, 1), -1);
    std::vector<uint64_t> sCls((size_t)m * CW, 0);
    for (int i = 0; i < m; i++) {
      sFlags[i] = (eUns[i] && eOver[i]) ? 1 : 0;
      for (int c = 0; c < Cext; c++) if (classMatchesNode(h, c, N + i)) sCls[(size_t)i * CW + (c >> 6)] |= 1ull << (c & 63);
      if (masks) for (size_t s = 0; s < L; s++) if (eLab[(size_t)i * L + s] >= 0) sLab[(size_t)i * L + s] = h->uniOffHost[s] + eLab[(size_t)i * L + s];
    }
    for (int k = 0; k < m; k++) insRow[k] = N + ord[k];
    NaArgs a; memset(&a, 0, sizeof a);
    a.N = N; a.N1 = N1; a.m = m; a.R = R; a.Npad = Npad; a.Npad1 = Npad1; a.W = W; a.W1 = W1; a.CW = CW; a.L = (int32_t)L;
    for (int r = 0; r < R; r++) if (d.cfg.isFloating[r]) a.floatMask |= 1 << r;
    a.clsLow = h->C >= 64 ? ~0ull : ((1ull << h->C) - 1);
    char* s = h->naScratch;
    plat_h2d(s, rows->total, 8 * mm * R); plat_h2d(s + oAlloc, rows->allocatable, 8 * mm * R); plat_h2d(s + oIdRank, eIdRank.data(), 4 * mm); plat_h2d(s + oType, sType.data(), 4 * mm);
    plat_h2d(s + oIns, ins.data(), 4 * mm); plat_h2d(s + oInsRow, insRow.data(), 4 * mm); plat_h2d(s + oLab, sLab.data(), 4 * sLab.size()); plat_h2d(s + oCls, sCls.data(), 8 * sCls.size());
    plat_h2d(s + oFlags, sFlags.data(), mm);
    if (rows->id_rank_all) { plat_h2d(s + oAll, rows->id_rank_all, 4 * (size_t)N1); a.idRankAll = (const int32_t*)(s + oAll); }
    a.pTotal = (const int64_t*)s; a.pAlloc = (const int64_t*)(s + oAlloc); a.pIdRank = (const int32_t*)(s + oIdRank); a.pType = (const int32_t*)(s + oType);
    a.ins = (const int32_t*)(s + oIns); a.insRow = (const int32_t*)(s + oInsRow); a.pLab = (const int32_t*)(s + oLab); a.pCls = (const uint64_t*)(s + oCls); a.pFlags = (const uint8_t*)(s + oFlags);
    prof.lap("mirrors, class bits and the upload of the entries");
    sb.fill();
    a.inTotal = d.totalRes; a.outTotal = (int64_t*)sb.fresh(&d.totalRes); a.inAlloc = d.allocatable; a.outAlloc = (int64_t*)sb.fresh(&d.allocatable);
    a.inFlags = d.nodeFlags; a.outFlags = (uint8_t*)sb.fresh(&d.nodeFlags); a.inIdRank = d.nodeIdRank; a.outIdRank = (int32_t*)sb.fresh(&d.nodeIdRank);
    a.rankIn = d.nodeByRank; a.rankOut = (int32_t*)sb.fresh(&d.nodeByRank); a.idxRankOut = (int32_t*)sb.fresh(&d.idxRank);
    if (masks) {
      a.inType = h->dNodeType; a.outType = (int32_t*)sb.fresh(&h->dNodeType);
      a.shapeClass = h->dShapeClass; a.shapeReq = d.shapeReq;
      const uint64_t* in[NA_MASKS] = {h->dClassMask, d.shapeMask, d.typeMask, d.labelMask};
      void* sl[NA_MASKS] = {&h->dClassMask, &d.shapeMask, &d.typeMask, &d.labelMask};
      const int nrows[NA_MASKS] = {Cext, Sext, T, labelRows};
      for (int k = 0; k < NA_MASKS; k++) { a.inMask[k] = in[k]; a.outMask[k] = (uint64_t*)sb.fresh(sl[k]); a.rows[k] = nrows[k]; }
    }
    if (haveFast) { a.inCls = d.nodeCls; a.outCls = (uint64_t*)sb.fresh(&d.nodeCls); }
    const int prc = plat_take_failure() ? -1 : plat_nodes_append(d, a);
    if (prc) {
      sb.drop();
      return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    }
    plat_pass_ms(PASS_NA, h->naMs);
    prof.lap("memsets and the passes");
    // the blocks swapped in, the old ones released (plat_nodes_append has waited for the device); the node-indexed scratch that stays gets the start a fresh upload gives it
    sb.commit();
    for (auto& z : zeroed) plat_memset(z.first, 0, z.second);
    h->N = N1; d.cfg.N = N1; d.cfg.Npad = Npad1; d.cfg.W = W1;
    if (haveFast) d.fitW = (N1 + 63) / 64;
    if (h->jobsSet) exclSetup(h);   // (the [cap][W] bit rows of the failed-selection store: B_RESET_JOBS forgets the records anyway)
    prof.lap("releases and exclSetup");
    if (plat_pass_printed(PASS_NA))
      fprintf(stderr, "[asched nodes_append] nodes %d entries %d mask rows %d fresh blocks %zu: planes %.4f ms, narrow arrays %.4f ms, index order %.4f ms, mask rows %.4f ms\n",
              N, m, a.rows[0] + a.rows[1] + a.rows[2] + a.rows[3], sb.blocks.size(), h->naMs[0], h->naMs[1], h->naMs[2], h->naMs[3]);
  }
  h->naStats[0] = m; h->naStats[1] = Npad1 != Npad ? 1 : 0; h->naStats[4] = h->N;
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  const int rc = resetDynamicState(h, M);
  prof.lap("the reset passes");
  return rc;
}
int32_t asched_nodes_append_stats(asched_t* h, int32_t* out) {
  if (!h || !out) return ASCHED_ERR_INVALID;
  plat_enter(h->plat);
  for (int k = 0; k < 8; k++) out[k] = h->naStats[k];
  return 0;
}

int32_t asched_txn_begin(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); h->allocPristine = false; return runControl(h, CMD_TXN_BEGIN); }
int32_t asched_txn_commit(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); return runControl(h, CMD_TXN_COMMIT); }
int32_t asched_txn_abort(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); return runControl(h, CMD_TXN_ABORT); }

static void readPod(asched* h, int job, asched_pod_result* o) {
  int32_t v[4];
  plat_d2h(&v[0], h->dev.pcNode + job, 4); plat_d2h(&v[1], h->dev.pcSap + job, 4);
  plat_d2h(&v[2], h->dev.pcPap + job, 4); plat_d2h(&v[3], h->dev.pcMethod + job, 4);
  o->node = v[0]; o->scheduled_at_priority = v[1]; o->preempted_at_priority = v[2]; o->method = v[3];
}

int32_t asched_select_node(asched_t* h, int32_t job, int32_t pinned, asched_pod_result* out, int32_t* preempted, int32_t cap, int32_t* npre) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "select_node: bad job");
  if (pinned < -1 || pinned >= h->N) return fail(h, ASCHED_ERR_INVALID, "select_node: bad pinned node");
  const bool wasPristine = h->allocPristine;
  h->allocPristine = false;  // fair-share preemption inside a selection removes victims from the returned node
  setArgs(h, {job, pinned});
  int rc = runControl(h, CMD_SELECT);
  if (rc) return rc;
  readPod(h, job, out);
  int32_t io[1]; getIO(h, io, 1);
  int np = io[0];
  if (out->node < 0 && np == 0) h->allocPristine = wasPristine;   // (nil, nil, nil): nothing was touched — e.g. the selection behind a submit check's rejection message (asched_excluded_nodes)
  if (preempted && np > 0) plat_d2h(preempted, h->dev.preList, sizeof(int32_t) * std::min(np, cap));
  if (npre) *npre = np;
  return 0;
}

int32_t asched_schedule_many(asched_t* h, int32_t n, const int32_t* jobs, const int32_t* pinned, asched_pod_result* out, int32_t* ok,
                             int32_t* preempted, int32_t cap, int32_t* npre) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->jobsSet || !h->nodesSet) return fail(h, ASCHED_ERR_INVALID, "schedule_many: nodes_upsert and jobs_set first");
  if (n < 1 || n > 65536 || n > std::max(h->M, 1)) return fail(h, ASCHED_ERR_INVALID, "schedule_many: gang size out of range");
  for (int i = 0; i < n; i++) {
    if (jobs[i] < 0 || jobs[i] >= h->M) return fail(h, ASCHED_ERR_INVALID, "schedule_many: bad job");
    if (pinned && (pinned[i] < -1 || pinned[i] >= h->N)) return fail(h, ASCHED_ERR_INVALID, "schedule_many: bad pinned node");
  }
  h->allocPristine = false;
  std::vector<int32_t> a{n};
  for (int i = 0; i < n; i++) { a.push_back(jobs[i]); a.push_back(pinned ? pinned[i] : -1); }
  setArgs(h, a);
  int rc = runControl(h, CMD_SCHEDULE_MANY);
  if (rc) return rc;
  int32_t io[2]; getIO(h, io, 2);
  *ok = io[0];
  for (int i = 0; i < n; i++) readPod(h, jobs[i], &out[i]);
  int np = io[1];
  if (preempted && np > 0) plat_d2h(preempted, h->dev.preList, sizeof(int32_t) * std::min(np, cap));
  if (npre) *npre = np;
  return 0;
}

int32_t asched_bind(asched_t* h, int32_t job, int32_t node, int32_t prio) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (node < 0 || node >= h->N || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "bind: bad id");
  h->allocPristine = false;
  setArgs(h, {job, node, prio});
  return runControl(h, CMD_BIND);
}
int32_t asched_evict(asched_t* h, int32_t job, int32_t node) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (node < 0 || node >= h->N || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "evict: bad id");
  h->allocPristine = false;
  setArgs(h, {job, node});
  return runControl(h, CMD_EVICT);
}
int32_t asched_unbind(asched_t* h, int32_t job, int32_t node) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (node < 0 || node >= h->N || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "unbind: bad id");
  h->allocPristine = false;
  setArgs(h, {job, node});
  return runControl(h, CMD_UNBIND);
}
int32_t asched_add_evicted(asched_t* h, int32_t index, int32_t job, int32_t node) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (index < 0 || index >= h->M) return fail(h, ASCHED_ERR_INVALID, "add_evicted: index out of range");
  if (job < 0 || job >= h->M || node < 0 || node >= h->N) return fail(h, ASCHED_ERR_INVALID, "add_evicted: bad id");
  h->evictedDirty = true;
  setArgs(h, {index, job, node});
  return runControl(h, CMD_ADD_EVICTED);
}
int32_t asched_reset_evicted(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); h->evictedDirty = false; return runControl(h, CMD_RESET_EVICTED); }

// ClearAllocated (nodedb.go:1178-1199): AllocatableByPriority[p] = allocatableResources for every p — the bulk pass of a fresh
// upsert (every plane := allocatable, order keys rebuilt) with an explicit alloc_by_prio table left out of it
int32_t asched_clear_allocated(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->nodesSet) return fail(h, ASCHED_ERR_INVALID, "clear_allocated: nodes_upsert first");
  h->stateEpoch++;
  h->prepared = false;  // the round state (sctx, sorted base) no longer describes the NodeDb: round_prepare rebuilds both
  // ClearAllocated re-upserts every node with the new AllocatableByPriority: from here on that IS the NodeDb's node state, so an
  // explicit alloc_by_prio table of the upsert is dropped for good (later resets start from allocatable too)
  h->dev.alloc0 = nullptr;
  h->hasAllocByPrio = false;
  int rc = runControl(h, CMD_UPSERT_RESET);
  if (!rc) { h->allocPristine = true; h->equalLevels = h->P; }
  return rc;
}

// The submit checker's per-pool core for a batch of units (submitcheck.go:342-371): the unit tables are uploaded once and
// ONE control launch walks them (each unit = txn + ScheduleManyWithTxn + abort on the device), results come back in one copy.
int32_t asched_submit_check(asched_t* h, int32_t nu, const int32_t* off, const int32_t* jobs, const int32_t* flags, asched_submit_result* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->nodesSet || !h->jobsSet) return fail(h, ASCHED_ERR_INVALID, "submit_check: nodes_upsert and jobs_set first");
  if (nu < 0) return fail(h, ASCHED_ERR_INVALID, "submit_check: negative unit count");
  if (nu == 0) return 0;
  if (off[0] != 0) return fail(h, ASCHED_ERR_INVALID, "submit_check: unit_off[0] must be 0");
  for (int u = 0; u < nu; u++) {
    int n = off[u + 1] - off[u];
    if (n <= 0) return fail(h, ASCHED_ERR_INVALID, "submit_check: empty unit");
    if (n > std::max(h->M, 1)) return fail(h, ASCHED_ERR_INVALID, "submit_check: unit larger than the job table");
  }
  int total = off[nu];
  for (int i = 0; i < total; i++) if (jobs[i] < 0 || jobs[i] >= h->M) return fail(h, ASCHED_ERR_INVALID, "submit_check: bad job");
  Dev& d = h->dev;
  h->submitMs = 0;
  if (h->N == 0) {   // a pool without nodes (no executor reports for it yet): no node for anybody, nothing to launch
    for (int u = 0; u < nu; u++) { out[u].ok = 0; out[u].scheduled_away = 0; out[u].num_schedulable = 0; out[u].first_node = -1; }
    h->submitWideUnits = h->submitWidePasses = 0; h->submitSeqUnits = 0; h->submitGangUnits = 0; h->submitNodePasses = 0; h->submitLitUnits = 0;
    return 0;
  }
  // ---- wide path: individual checks against a pristine NodeDb.  Every priority plane equals allocatable and nothing is evicted, so
  // SelectNodeForJobWithTxn reduces to "first node, in index order, of the job's home mask row that fits — else of its away rows in
  // order" (fit at priority -2 succeeds or every later step of the cascade sees the same numbers, nodedb.go:724-789; no evicted
  // jobs to preempt).  That is the fit kernel's question (k_fit_batch: all shapes x all nodes in one pass over the planes, every CU
  // busy) — the per-unit transaction of the sequential path is pointless here because nothing would be left to abort.
  // A row on the literal iteration path asks the same question of the literal iterators: the rows of a pass are split, the packed-key ones to k_fit_batch, the literal
  // ones to the literal batched first fit (kernels_fit_lit.h; its index of level 0 is built in the first pass that has one and reused by the later passes: nothing
  // changes the NodeDb in between).  Not on a two-word order key, which that kernel does not serve: those units keep the sequential path.
  std::vector<uint8_t> done(nu, 0);
  int widePasses = 0, wideUnits = 0, litUnits = 0, nodePasses = 0;   // nodePasses: how often a launch of this check walks the node set (SURVEY 8d: ONE query per batched pass)
  // "pristine" for a job of priority p: the planes of every level up to p's equal level 0's — what the arguments below rest on (a failed fit at priority -2 is a failed selection)
  auto pristineUpTo = [&](int32_t prio) { int l = 0; while (l < h->P && h->prios[l] != prio) l++; return l < h->equalLevels; };
  const char* wideEnv = getenv("ASCHED_SUBMIT_WIDE");   // ASCHED_SUBMIT_WIDE=0: every unit through the sequential path (debugging / A-B)
  if (h->allocPristine && !h->evictedDirty && !(wideEnv && wideEnv[0] == '0')) {
    struct Pending { int u, job, shape, k, kEnd; };
    std::vector<Pending> pend;
    for (int u = 0; u < nu; u++) {
      if (!(flags && (flags[u] & ASCHED_SUBMIT_STRIP_GANG)) || off[u + 1] - off[u] != 1) continue;
      int j = jobs[off[u]], sidx = h->jShape[j], pc = h->jPc[j];
      int kBeg = d.cfg.pcAwayOff[pc], kEnd = (d.cfg.hasAway && !d.cfg.disableAway) ? d.cfg.pcAwayOff[pc + 1] : kBeg;
      if (!pristineUpTo(h->pcPriority[pc]) || (h->equalLevels < h->P && kEnd > kBeg)) continue;   // planes that differ at or below the job's level (or an away attempt at another one): the sequential path
      bool literal = h->rowLiteral[sidx] != 0;   // a row whose iteration order is not the packed-key order: the literal kernel answers it
      for (int k = kBeg; k < kEnd; k++) literal = literal || h->rowLiteral[h->S + h->awayRowOff[sidx] + (k - kBeg)];
      if (literal && d.cfg.keyWords == 2) continue;
      done[u] = 1; wideUnits++; litUnits += literal;
      out[u].ok = 0; out[u].scheduled_away = 0; out[u].num_schedulable = 0; out[u].first_node = -1;
      bool disallowedReq = false;
      for (int r = 0; r < h->R; r++) if (h->disallowed[r] && h->jReq[(size_t)j * h->R + r] > 0) disallowedReq = true;   // nodedb.go:596-601
      if (disallowedReq) continue;
      pend.push_back({u, j, sidx, d.cfg.disableHome ? kBeg : kBeg - 1, kEnd});   // k == kBeg - 1 stands for the home attempt
    }
    bool litIndexBuilt = false;
    while (!pend.empty()) {   // pass 0: home rows; pass i: the i-th away entry of the units still without a node
      std::vector<int32_t> rows, slotOfRow((size_t)h->S + h->awayRowClass.size(), -1), rowOf(pend.size(), -1);
      for (size_t i = 0; i < pend.size(); i++) {
        Pending& p = pend[i];
        int kBeg = d.cfg.pcAwayOff[h->jPc[p.job]];
        while (p.k >= kBeg && p.k < p.kEnd && !d.cfg.awayUsable[p.k]) p.k++;   // no extra taints to tolerate (:703-706)
        if (p.k >= p.kEnd) continue;
        int row = p.k < kBeg ? p.shape : h->S + h->awayRowOff[p.shape] + (p.k - kBeg);
        if (slotOfRow[row] < 0) { slotOfRow[row] = (int32_t)rows.size(); rows.push_back(row); }
        rowOf[i] = row;
      }
      if (rows.empty()) break;
      std::vector<int32_t> res(rows.size(), -1);
      if (h->N > 0) {   // a pool without nodes (no executor reports for it yet) answers "no node" without a launch
        std::vector<int32_t> packed, lit, packedAt, litAt;
        for (size_t i = 0; i < rows.size(); i++) { bool l = h->rowLiteral[rows[i]] != 0; (l ? lit : packed).push_back(rows[i]); (l ? litAt : packedAt).push_back((int32_t)i); }
        std::vector<int32_t> pr(packed.size(), -1), lr(lit.size(), -1);
        if (!packed.empty()) {
          if (plat_run_fit_batch(d, packed, 0 /* priority -2 */, pr, h->nodeByRank.data())) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
          h->submitMs += plat_last_fit_ms();
        }
        if (!lit.empty()) {
          if (plat_run_fit_batch_lit(d, h->dNodeType, (int)h->types.size(), lit, 0, lr, litIndexBuilt, 0.0)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
          h->submitMs += plat_last_fit_ms();
          if (!litIndexBuilt) nodePasses++;   // (the index build walks the node set; the queries walk the index)
          litIndexBuilt = true;
        }
        if (!packed.empty()) nodePasses++;
        for (size_t i = 0; i < packed.size(); i++) res[packedAt[i]] = pr[i];
        for (size_t i = 0; i < lit.size(); i++) res[litAt[i]] = lr[i];
      }
      widePasses++;
      std::vector<Pending> next;
      for (size_t i = 0; i < pend.size(); i++) {
        Pending& p = pend[i];
        if (rowOf[i] < 0) continue;
        int node = res[slotOfRow[rowOf[i]]];
        int kBeg = d.cfg.pcAwayOff[h->jPc[p.job]];
        if (node >= 0) { out[p.u].ok = 1; out[p.u].scheduled_away = p.k >= kBeg; out[p.u].num_schedulable = 1; out[p.u].first_node = node; }
        else { p.k++; if (p.k < p.kEnd) next.push_back(p); }
      }
      pend.swap(next);
    }
  }
  // ---- gang path: units of several members against a pristine NodeDb, ONE WORKGROUP PER UNIT (submit_gang.h).  Units never see each other (every transaction is aborted) and
  // inside a unit each member's first fit at priority -2 sees the earlier members' binds from the workgroup's own scratch — nothing is written to the NodeDb, nothing to abort.
  // Only what that argument covers is sent: home scheduling on, no usable away type and no disallowed request among the members, no row on the literal iteration path, one
  // priority class per unit, at most SG_TMAX members, the node bitmap fits LDS.  ASCHED_SUBMIT_GANGS=0: these units through the sequential path (A/B, debugging).
  int gangUnits = 0;
  {
    const char* gangEnv = getenv("ASCHED_SUBMIT_GANGS");
    if (h->allocPristine && !h->evictedDirty && !d.cfg.disableHome && h->N <= SG_MAX_NODES && !(wideEnv && wideEnv[0] == '0') && !(gangEnv && gangEnv[0] == '0') &&
        d.cfg.keyWords != 2) {   // (a two-word order key: the gang units take the sequential path — submit_gang.h and the capacity pass compare one-word keys)
      std::vector<int32_t> go(1, 0), gj, gu;
      std::vector<int32_t> uniUnit, uniShapeOf, uniShapes, uniSlot((size_t)h->S, -1);   // uniform units: all members of one scheduling-key shape (submit_gang.h: a sum, not a sequence)
      for (int u = 0; u < nu; u++) {
        if (done[u]) continue;
        int n = off[u + 1] - off[u];
        if (n < 2) continue;
        bool eligible = true, uniform = true;
        for (int i = off[u] + 1; i < off[u + 1]; i++) uniform = uniform && h->jShape[jobs[i]] == h->jShape[jobs[off[u]]];
        if (!uniform && n > SG_TMAX) continue;
        int pc0 = h->jPc[jobs[off[u]]];
        for (int i = off[u]; i < off[u + 1] && eligible; i++) {
          int j = jobs[i], pc = h->jPc[j];
          if (pc != pc0 || h->rowLiteral[h->jShape[j]] || !pristineUpTo(h->pcPriority[pc])) eligible = false;
          if (d.cfg.hasAway && !d.cfg.disableAway && !(h->jGangDense[j] >= 0 && !(flags && (flags[u] & ASCHED_SUBMIT_STRIP_GANG)) && d.cfg.disableGangAway))
            for (int k = d.cfg.pcAwayOff[pc]; k < d.cfg.pcAwayOff[pc + 1]; k++) if (d.cfg.awayUsable[k]) eligible = false;
          for (int r = 0; r < h->R; r++) if (h->disallowed[r] && h->jReq[(size_t)j * h->R + r] > 0) eligible = false;
        }
        if (!eligible) continue;
        if (uniform) {
          int sh = h->jShape[jobs[off[u]]];
          if (uniSlot[sh] < 0) { uniSlot[sh] = (int32_t)uniShapes.size(); uniShapes.push_back(sh); }
          uniUnit.push_back(u); uniShapeOf.push_back(uniSlot[sh]);
          continue;
        }
        gu.push_back(u);
        gj.insert(gj.end(), jobs + off[u], jobs + off[u + 1]);
        go.push_back((int32_t)gj.size());
      }
      if (!uniUnit.empty()) {
        std::vector<int32_t> first; std::vector<long long> capSum;
        if (plat_run_fit_capacity(d, uniShapes, first, capSum, h->nodeByRank.data())) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
        h->submitMs += plat_last_fit_ms(); nodePasses++;
        for (size_t i = 0; i < uniUnit.size(); i++) {
          int u = uniUnit[i]; long long n = off[u + 1] - off[u], cap = capSum[uniShapeOf[i]];
          done[u] = 1; gangUnits++;
          out[u].ok = cap >= n; out[u].scheduled_away = 0; out[u].num_schedulable = (int32_t)std::min(n, cap); out[u].first_node = cap > 0 ? first[uniShapeOf[i]] : -1;
        }
      }
      if (!gu.empty()) {
        std::vector<int32_t> res;
        if (plat_run_submit_gangs(d, go, gj, res)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
        h->submitMs += plat_last_fit_ms(); nodePasses += (int)gj.size();   // every member of such a unit is one walk over the nodes by its workgroup
        for (size_t i = 0; i < gu.size(); i++) {
          if (res[4 * i] < 0) continue;   // a key field left the layout: the sequential path decides (it raises the same condition itself)
          int u = gu[i];
          done[u] = 1; gangUnits++;
          out[u].ok = res[4 * i]; out[u].scheduled_away = res[4 * i + 1]; out[u].num_schedulable = res[4 * i + 2]; out[u].first_node = res[4 * i + 3];
        }
      }
    }
  }
  h->submitGangUnits = gangUnits;
  // ---- sequential path (one control launch): whatever is left — units when the NodeDb is not pristine, gang units with away types or literal rows
  std::vector<int32_t> vo(1, 0), vj, vf, unitOf;
  for (int u = 0; u < nu; u++) {
    if (done[u]) continue;
    unitOf.push_back(u);
    vj.insert(vj.end(), jobs + off[u], jobs + off[u + 1]);
    vo.push_back((int32_t)vj.size());
    vf.push_back(flags ? flags[u] : 0);
  }
  int nd = (int)unitOf.size();
  h->submitWideUnits = wideUnits; h->submitWidePasses = widePasses; h->submitSeqUnits = nd; h->submitNodePasses = nodePasses; h->submitLitUnits = litUnits;
  if (nd == 0) return 0;
  DevBufs tmp;
  SubmitArgs a; memset(&a, 0, sizeof a);
  a.nu = nd; a.off = tmp.upload(vo); a.jobs = tmp.upload(vj); a.flags = tmp.upload(vf); a.out = tmp.alloc<int32_t>((size_t)nd * 4);
  plat_h2d(d.cmdIO + 16, &a, sizeof a);
  int rc = runControl(h, CMD_SUBMIT_CHECK);
  h->submitMs += plat_last_control_ms();
  if (!rc) {
    static_assert(sizeof(asched_submit_result) == 16, "4 result words per unit");
    std::vector<asched_submit_result> r(nd);
    plat_d2h(r.data(), a.out, (size_t)nd * sizeof(asched_submit_result));
    for (int i = 0; i < nd; i++) out[unitOf[i]] = r[i];
  }
  tmp.freeAll();
  return rc;
}

int32_t asched_get_alloc(asched_t* h, int32_t node, int64_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (node < 0 || node >= h->N) return fail(h, ASCHED_ERR_INVALID, "get_alloc: bad node");
  for (int l = 0; l < h->P; l++) for (int r = 0; r < h->R; r++) {
    if (h->dev.cfg.isFloating[r]) { out[l * h->R + r] = 0; continue; }   // node.AllocatableByPriority has nothing in a floating column
    plat_d2h(&out[l * h->R + r], h->dev.alloc + ((size_t)l * h->R + r) * h->dev.cfg.Npad + node, sizeof(int64_t));
  }
  return plat_take_failure() ? fail(h, ASCHED_ERR_DEVICE, plat_last_error()) : 0;
}
int32_t asched_get_scheduled_at_priority(asched_t* h, int32_t job, int32_t* out, int32_t* ok) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->jobsSet || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "get_scheduled_at_priority: bad job");
  int32_t v; plat_d2h(&v, h->dev.schedAtPrio + job, 4);
  *ok = v != NO_PRIORITY; *out = *ok ? v : 0;
  return 0;
}

// NodeTypesIterator order == ascending packed key over the nodes of the given types that pass the *indexed* columns
// (the iterator itself does not apply static or non-indexed checks, nodeiteration.go:318-382).
// Market-driven ordering's iterators on the device (round_market.h): the argument block goes through the command mailbox, the lists through temporary buffers
static int runMarket(asched* h, MarketArgs& a, DevBufs& tmp) {
  static_assert(sizeof(MarketArgs) % 4 == 0 && sizeof(MarketArgs) / 4 < 256, "argument block fits the command mailbox");
  std::vector<int32_t> w(sizeof(MarketArgs) / 4);
  memcpy(w.data(), &a, sizeof a);
  setArgs(h, w);
  int rc = runControl(h, CMD_MARKET);
  if (rc) tmp.freeAll();
  return rc;
}
int32_t asched_market_iterate(asched_t* h, int32_t nq, const int32_t* nameRank, const int32_t* off, const asched_market_job* jobs, int32_t preferHome, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (nq < 0 || (nq > 0 && (!nameRank || !off || !out))) return fail(h, ASCHED_ERR_INVALID, "market_iterate: bad arguments");
  int total = nq > 0 ? off[nq] : 0;
  if (total <= 0) return 0;
  DevBufs tmp;
  MarketArgs a; memset(&a, 0, sizeof a);
  a.op = 0; a.nq = nq; a.preferHome = preferHome;
  a.nameRank = tmp.upload(std::vector<int32_t>(nameRank, nameRank + nq)); a.off = tmp.upload(std::vector<int32_t>(off, off + nq + 1));
  a.jobs = tmp.upload(std::vector<asched_market_job>(jobs, jobs + total));
  a.out = tmp.alloc<int32_t>(total); a.work = tmp.alloc<int32_t>(2 * (size_t)nq);
  if (int rc = runMarket(h, a, tmp)) return rc;
  plat_d2h(out, a.out, sizeof(int32_t) * (size_t)total);
  tmp.freeAll();
  return 0;
}
int32_t asched_market_compare(asched_t* h, const asched_market_cmp_job* x, const asched_market_cmp_job* y, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!x || !y || !out) return fail(h, ASCHED_ERR_INVALID, "market_compare: bad arguments");
  DevBufs tmp;
  MarketArgs a; memset(&a, 0, sizeof a);
  a.op = 1;
  a.l1 = tmp.upload(std::vector<asched_market_cmp_job>(x, x + 1)); a.l2 = tmp.upload(std::vector<asched_market_cmp_job>(y, y + 1));
  a.out = tmp.alloc<int32_t>(1);
  if (int rc = runMarket(h, a, tmp)) return rc;
  plat_d2h(out, a.out, sizeof(int32_t));
  tmp.freeAll();
  return 0;
}
int32_t asched_market_multi_iterate(asched_t* h, int32_t n1, const asched_market_cmp_job* l1, const uint8_t* ev1, int32_t n2, const asched_market_cmp_job* l2, const uint8_t* ev2,
                                    int32_t onlyAfter, int32_t* out, int32_t* nOut) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (n1 < 0 || n2 < 0 || !out || !nOut || (n1 > 0 && (!l1 || !ev1)) || (n2 > 0 && (!l2 || !ev2))) return fail(h, ASCHED_ERR_INVALID, "market_multi_iterate: bad arguments");
  DevBufs tmp;
  MarketArgs a; memset(&a, 0, sizeof a);
  a.op = 2; a.n1 = n1; a.n2 = n2; a.onlyAfter = onlyAfter;
  a.l1 = tmp.upload(std::vector<asched_market_cmp_job>(l1, l1 + n1)); a.l2 = tmp.upload(std::vector<asched_market_cmp_job>(l2, l2 + n2));
  a.ev1 = tmp.upload(std::vector<uint8_t>(ev1, ev1 + n1)); a.ev2 = tmp.upload(std::vector<uint8_t>(ev2, ev2 + n2));
  a.out = tmp.alloc<int32_t>((size_t)n1 + n2 + 1);
  if (int rc = runMarket(h, a, tmp)) return rc;
  std::vector<int32_t> res((size_t)n1 + n2 + 1);
  plat_d2h(res.data(), a.out, sizeof(int32_t) * res.size());
  tmp.freeAll();
  *nOut = res[(size_t)n1 + n2];
  for (int i = 0; i < *nOut; i++) out[i] = res[i];
  return 0;
}
int32_t asched_iterate_nodes(asched_t* h, const int64_t* typeIds, int32_t nt, int32_t prio, const int64_t* ireq, int32_t* out, int32_t cap, int32_t* nout) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  // the literal iterator restatement of the device (round_ctl.h litAdvance, the path rounds take off the index grid), materialised by the auxiliary kernel
  if (!h->nodesSet || !ireq || !nout || (cap > 0 && !out)) return fail(h, ASCHED_ERR_INVALID, "iterate_nodes: nodes_upsert first / null argument");
  int level = -1;
  for (int l = 0; l < h->P; l++) if (h->prios[l] == prio) level = l;
  if (level < 0) return fail(h, ASCHED_ERR_INVALID, "iterate_nodes: unknown priority");
  if (h->keyCoarse) return fail(h, ASCHED_ERR_UNSUPPORTED, "iterate_nodes: the literal iterators reason in the index resolution; this handle's key fields use a coarser divisor (layoutKeys)");
  std::vector<int> tis;
  if (nt < 0) for (size_t i = 0; i < h->types.size(); i++) tis.push_back((int)i);
  else for (int k = 0; k < nt; k++) for (size_t i = 0; i < h->types.size(); i++) if (h->typeId[i] == typeIds[k]) tis.push_back((int)i);
  if ((int)tis.size() > LIT_TMAX) return fail(h, ASCHED_ERR_UNSUPPORTED, "iterate_nodes: more than LIT_TMAX node types");
  Dev& d = h->dev;
  int W = d.cfg.W;
  std::vector<uint64_t> mask(std::max<size_t>(tis.size(), 1) * W, 0);
  for (size_t k = 0; k < tis.size(); k++) for (int n = 0; n < h->N; n++) if (h->nodeType[n] == tis[k]) mask[k * W + (n >> 6)] |= 1ull << (n & 63);
  uint64_t* savedMask = d.typeMask;
  DevBufs tmp;
  d.typeMask = tmp.upload(mask);
  std::vector<int32_t> a{level, (int32_t)tis.size(), std::min(cap, h->N), 0};
  for (int i = 0; i < MAXK; i++) { int64_t v = i < h->K ? ireq[i] : 0; a.push_back((int32_t)(uint32_t)((uint64_t)v & 0xffffffffu)); a.push_back((int32_t)(uint32_t)((uint64_t)v >> 32)); }
  for (size_t k = 0; k < tis.size(); k++) a.push_back((int32_t)k);
  setArgs(h, a);
  int rc = runControl(h, CMD_ITERATE_NODES);
  d.typeMask = savedMask;
  if (rc) { tmp.freeAll(); return rc; }
  int32_t n = 0; getIO(h, &n, 1);
  if (n > 0 && cap > 0) plat_d2h(out, d.nodeOver, sizeof(int32_t) * (size_t)std::min(n, std::min(cap, h->N)));
  tmp.freeAll();
  *nout = n;
  return 0;
}

int32_t asched_fit_select_batch(asched_t* h, int32_t n, const int32_t* jobs, int32_t prio, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  int level = -1;
  for (int i = 0; i < h->P; i++) if (h->prios[i] == prio) level = i;
  if (level < 0) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch: unknown priority");
  // identical (shape, level) queries share one scan (SURVEY 8d: batched passes are counted once).  Shapes whose iteration order is the packed-key order go to k_fit_batch
  // (one pass over the planes for all of them), shapes on the literal iteration path (unaligned request, several unaligned node types) to the literal batched first fit
  // (kernels_fit_lit.h: an index of the level built for this call, one wave per shape): a mixed batch is answered whole.
  std::vector<int32_t> shapeOf(n), uniq, uniqLit; std::vector<int32_t> slot(h->S, -1);   // slot: >= 0 position in uniq, <= -2 position -(slot + 2) in uniqLit
  for (int i = 0; i < n; i++) {
    if (jobs[i] < 0 || jobs[i] >= h->M) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch: job out of range");
    int s = h->jShape[jobs[i]];
    if (slot[s] == -1) {
      if (!h->rowLiteral.empty() && h->rowLiteral[s]) {
        if (h->dev.cfg.keyWords == 2) return fail(h, ASCHED_ERR_UNSUPPORTED, "fit_select_batch: this job's iteration order is not the packed-key order and this handle's order key takes two words, which the literal batched first fit does not serve; use select_node");
        slot[s] = -2 - (int32_t)uniqLit.size(); uniqLit.push_back(s);
      } else { slot[s] = (int32_t)uniq.size(); uniq.push_back(s); }
    }
    shapeOf[i] = slot[s];
  }
  std::vector<int32_t> res(uniq.size(), -1), resLit(uniqLit.size(), -1);
  h->lastWideWasOpt = false;
  if (h->N > 0 && !uniq.empty() && plat_run_fit_batch(h->dev, uniq, level, res, h->nodeByRank.data())) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (h->N > 0 && !uniqLit.empty() && plat_run_fit_batch_lit(h->dev, h->dNodeType, (int)h->types.size(), uniqLit, level, resLit, false, uniq.empty() ? 0.0 : plat_last_fit_ms()))
    return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  for (int i = 0; i < n; i++) out[i] = shapeOf[i] >= 0 ? res[shapeOf[i]] : resLit[-(shapeOf[i] + 2)];
  return 0;
}

// ---- one pool on several GPUs (DESIGN.md 7): the reduced words are produced and consumed on the device (mgpu.h, armada_sched_mgpu.hip)
int32_t asched_fit_select_batch_global(asched_t* h, int32_t n, const int32_t* jobs, int32_t prio, const asched_global_key_layout* lay, int64_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!lay || !out || n < 0) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch_global: null argument");
  int level = -1;
  for (int i = 0; i < h->P; i++) if (h->prios[i] == prio) level = i;
  if (level < 0) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch_global: unknown priority");
  if (h->dev.cfg.keyWords == 2) return fail(h, ASCHED_ERR_UNSUPPORTED, "fit_select_batch_global: this handle's order key takes two words; the exchanged word holds one");
  if (h->keyCoarse) return fail(h, ASCHED_ERR_UNSUPPORTED, "fit_select_batch_global: this handle's key fields are quotients by its own coarser divisor (layoutKeys), not comparable across shards");
  if (lay->n_fields != h->K) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch_global: n_fields must equal the number of indexed resources");
  int bits = lay->rank_bits;
  for (int i = 0; i < h->K; i++) { if (lay->field_bits[i] < 1) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch_global: empty field"); bits += lay->field_bits[i]; }
  if (lay->rank_bits < 1 || bits > 62) return fail(h, ASCHED_ERR_UNSUPPORTED, "fit_select_batch_global: the shared order key needs more than 62 bits");
  std::vector<int32_t> slotOf(n), uniq; std::vector<int32_t> slot(h->S, -1);
  for (int i = 0; i < n; i++) {
    if (jobs[i] < 0 || jobs[i] >= h->M) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch_global: job out of range");
    int s = h->jShape[jobs[i]];
    if (!h->rowLiteral.empty() && h->rowLiteral[s]) return fail(h, ASCHED_ERR_UNSUPPORTED, "fit_select_batch_global: this job's iteration order is not the packed-key order");
    if (slot[s] < 0) { slot[s] = (int32_t)uniq.size(); uniq.push_back(s); }
    slotOf[i] = slot[s];
  }
  if (n == 0) return 0;
  GlobalKeyLayout L; memset(&L, 0, sizeof L);
  L.nFields = h->K; for (int i = 0; i < h->K; i++) L.bits[i] = lay->field_bits[i];
  L.rankBits = lay->rank_bits; L.rankOffset = lay->rank_offset;
  h->lastWideWasOpt = false;
  int bad = 0;
  int rc = plat_run_fit_batch_global(h->dev, uniq, slotOf, level, L, lay->global_rank, (long long*)out, &bad);
  if (rc) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (bad) return fail(h, ASCHED_ERR_INVALID, "fit_select_batch_global: a key field or node rank does not fit the layout the caller gave");
  return 0;
}
int32_t asched_round_delta_words(asched_t* h, int64_t* n) { if (!h || !n) return ASCHED_ERR_INVALID; *n = (int64_t)h->N * h->R + h->M; return 0; }
int32_t asched_round_delta(asched_t* h, int64_t* buf) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!buf) return fail(h, ASCHED_ERR_INVALID, "round_delta: null buffer");
  if (!h->haveRoundResult) return fail(h, ASCHED_ERR_INVALID, "round_delta: no round result on this handle (schedule_round first)");
  if (h->opt.enabled) return fail(h, ASCHED_ERR_UNSUPPORTED, "round_delta: not with the fairness optimiser on");
  if (h->N > (int)MGPU_NODE_MASK - 1) return fail(h, ASCHED_ERR_UNSUPPORTED, "round_delta: node count");
  if (plat_round_delta(h->dev, h->resNs, h->resNp, (long long*)buf)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return 0;
}
int32_t asched_round_delta_resolve(asched_t* h, const int64_t* red, asched_delta_summary* sum, int32_t* jobNode, int32_t* jobPrio, uint8_t* jobReplay) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!red || !sum || !jobNode || !jobPrio || !jobReplay) return fail(h, ASCHED_ERR_INVALID, "round_delta_resolve: null argument");
  if (!h->haveRoundResult) return fail(h, ASCHED_ERR_INVALID, "round_delta_resolve: no round result on this handle");
  int32_t counts[4] = {0, 0, 0, 0};
  if (plat_delta_resolve(h->dev, (const long long*)red, h->resNs, h->resNp, counts, jobNode, jobPrio, jobReplay)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  sum->conflict_nodes = counts[0]; sum->accepted = counts[1]; sum->replay = counts[2]; sum->preempted = counts[3];
  return 0;
}

// ---- the handle's communicator (include/armada_sched.h "The communicator"): RCCL bound at run time in the HIP library, the caller's transport otherwise
int32_t asched_comm_unique_id(asched_unique_id* out) {
  if (!out) return ASCHED_ERR_INVALID;
  return plat_comm_unique_id(out->bytes) ? ASCHED_ERR_DEVICE : 0;
}
// the status word of collectiveAgree exists from the moment there is a communicator: the agree step itself then has no rank-local way to fail in front of its all-reduce (round-5 advisor)
static int32_t commStatusAlloc(asched* h) {
  if (!h->commStatus) h->commStatus = (long long*)plat_malloc(8);
  return h->commStatus ? 0 : fail(h, ASCHED_ERR_DEVICE, plat_last_error());
}
int32_t asched_comm_init(asched_t* h, const asched_unique_id* id, int32_t rank, int32_t world) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(h, ASCHED_ERR_INVALID, "comm_init: rank / world out of range or null id");
  if (plat_comm_init(id->bytes, rank, world)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return commStatusAlloc(h);
}
int32_t asched_comm_init_external(asched_t* h, asched_allreduce_fn fn, void* ctx, int32_t rank, int32_t world) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!fn || world < 1 || rank < 0 || rank >= world) return fail(h, ASCHED_ERR_INVALID, "comm_init_external: rank / world out of range or null transport");
  if (plat_comm_init_external(fn, ctx, rank, world)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return commStatusAlloc(h);
}
int32_t asched_comm_destroy(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); plat_comm_destroy(); return 0; }
// Replicas stay in step because their control flow is a function of their (identical) inputs alone.  The soft time budgets (constraints.go:159-169) read the wall clock: two
// replicas would stop offering new jobs at different iterations and wait for each other's passes forever — refused unless the clock is a stepping one (clock_step_ns).
static int shardRefusal(asched* h) {
  const DevCfg& c = h->dev.cfg;
  if ((c.maxNewJobNs > 0 || c.maxNewJobPerQueueNs > 0) && c.clockStepNs <= 0)
    return fail(h, ASCHED_ERR_UNSUPPORTED, "sharded rounds with wall-clock time budgets (max_new_job_scheduling_duration): the replicas' control flow would depend on their clocks");
  return 0;
}
int32_t asched_shard_round(asched_t* h, int32_t on) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  int rank = 0, world = 1;
  plat_comm_info(&rank, &world);
  if (on && (world <= 1 || !plat_comm_live())) return fail(h, ASCHED_ERR_INVALID, "shard_round: bring the communicator up first (comm_init / comm_init_external, world > 1)");
  if (on && world > 255) return fail(h, ASCHED_ERR_UNSUPPORTED, "shard_round: more than 255 ranks");
  if (on) if (int rc = shardRefusal(h)) return rc;
  (void)plat_shard_peers(nullptr, 0, 0);   // (the exchange through the communicator, not GPU-to-GPU: asched_shard_peers switches that on)
  h->dev.cfg.shardRank = on ? (uint8_t)rank : 0; h->dev.cfg.shardWorld = on ? (uint8_t)world : 0;
  return 0;
}
int32_t asched_shard_area(asched_t* h, asched_shard_area_t* out) { if (!h || !out) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (plat_shard_area(&out->ptr, out->ipc)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return 0;
}
int32_t asched_shard_open(asched_t* h, const char* ipc, void** out) { if (!h || !ipc || !out) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (plat_shard_open(ipc, out)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return 0;
}
int32_t asched_shard_peers(asched_t* h, void* const* areas, int32_t world, int32_t rank) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!areas) { (void)plat_shard_peers(nullptr, 0, 0); h->dev.cfg.shardRank = 0; h->dev.cfg.shardWorld = 0; return 0; }
  if (world < 2 || world > 64 || rank < 0 || rank >= world) return fail(h, ASCHED_ERR_INVALID, "shard_peers: 2 <= world <= 64 (one lane of the control wave per replica), 0 <= rank < world");
  for (int r = 0; r < world; r++) if (!areas[r]) return fail(h, ASCHED_ERR_INVALID, "shard_peers: null area");
  if (int rc = shardRefusal(h)) return rc;
  if (plat_shard_peers(areas, world, rank)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  h->dev.cfg.shardRank = (uint8_t)rank; h->dev.cfg.shardWorld = (uint8_t)world;
  return 0;
}
int64_t asched_shard_exchanges(asched_t* h) { if (!h) return 0; plat_enter(h->plat); return plat_last_shard_exchanges(); }
int32_t asched_comm_rank(asched_t* h, int32_t* rank, int32_t* world) { if (!h || !rank || !world) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  int r = 0, w = 1; plat_comm_info(&r, &w); *rank = r; *world = w; return 0;
}
// A rank-local failure in front of a collective (a row on the literal path on this shard only, a key field outside the shared layout, no round result, an allocation)
// must not leave the peers blocked inside the all-reduce it never enters: every rank first all-reduces (MAX) ONE status word, and all of them either go on or return
// an error — the failing rank its own, the others ASCHED_ERR_PEER.  (Round-4 advisor, medium.)
static int32_t collectiveAgree(asched* h, int32_t rc) {
  int r = 0, w = 1; plat_comm_info(&r, &w);
  if (w <= 1) return rc;
  if (!h->commStatus) h->commStatus = (long long*)plat_malloc(8);
  if (!h->commStatus) return rc ? rc : fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  long long v = rc ? 1 : 0;
  plat_h2d(h->commStatus, &v, 8);
  std::string own = h->err;
  if (plat_allreduce(h->commStatus, 1, 2)) return rc ? rc : fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  plat_d2h(&v, h->commStatus, 8);
  if (plat_take_failure()) return rc ? rc : fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (rc) { h->err = own; return rc; }
  if (v) return fail(h, ASCHED_ERR_PEER, "another rank of the communicator failed in front of the collective (its own call returns the cause); nothing was exchanged");
  return 0;
}
// exact: this rank's rows -> words on the device -> ONE all-reduce MIN on the handle's stream -> winners' global ranks
int32_t asched_fit_select_batch_sharded(asched_t* h, int32_t n, const int32_t* jobs, int32_t prio, const asched_global_key_layout* lay, int32_t* outRank) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  // (every check below is rank-local: its verdict goes through collectiveAgree before anybody enters the data all-reduce; n is the same on every rank by contract)
  if (n == 0) return 0;   // (decided on what every rank shares — n — BEFORE any rank-local check: a rank with a bad pointer and n == 0 used to enter the agree step alone; round-5 advisor)
  int32_t rc = 0;
  if (!lay || !outRank || n < 0 || (n > 0 && !jobs)) rc = fail(h, ASCHED_ERR_INVALID, "fit_select_batch_sharded: null argument");
  for (int i = 0; i < n && rc == 0; i++) if (jobs[i] < 0 || jobs[i] >= h->M) rc = fail(h, ASCHED_ERR_INVALID, "fit_select_batch_sharded: job out of range");
  long long* words = rc == 0 ? (long long*)plat_malloc((size_t)n * 8) : nullptr;
  if (rc == 0 && !words) rc = fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (rc == 0) rc = asched_fit_select_batch_global(h, n, jobs, prio, lay, (int64_t*)words);   // device memory of this handle: filled in place
  rc = collectiveAgree(h, rc);
  if (rc == 0 && plat_allreduce(words, (size_t)n, 1)) rc = fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (rc == 0) {
    std::vector<long long> w(n);
    plat_d2h(w.data(), words, (size_t)n * 8);
    if (plat_take_failure()) rc = fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    const long long mask = (1ll << lay->rank_bits) - 1;
    if (rc == 0) for (int i = 0; i < n; i++) outRank[i] = w[i] == (long long)ASCHED_NO_NODE_WORD ? -1 : (int32_t)(w[i] & mask);
  }
  plat_free(words);
  return rc;
}
// approximate (queue-hash round): delta -> ONE all-reduce SUM -> resolve, all on the handle's stream
int32_t asched_round_exchange(asched_t* h, asched_delta_summary* sum, int32_t* jobNode, int32_t* jobPrio, uint8_t* jobReplay) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  int32_t rc = 0;
  if (!sum || !jobNode || !jobPrio || !jobReplay) rc = fail(h, ASCHED_ERR_INVALID, "round_exchange: null argument");
  size_t words = (size_t)h->N * h->R + h->M;
  long long* buf = rc == 0 ? (long long*)plat_malloc(std::max<size_t>(words, 1) * 8) : nullptr;
  if (rc == 0 && !buf) rc = fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (rc == 0) rc = asched_round_delta(h, (int64_t*)buf);
  rc = collectiveAgree(h, rc);   // (no round result on one rank, an allocation: every rank returns instead of one of them missing in the all-reduce)
  if (rc == 0 && plat_allreduce(buf, words, 0)) rc = fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (rc == 0) rc = asched_round_delta_resolve(h, (const int64_t*)buf, sum, jobNode, jobPrio, jobReplay);
  if (rc == 0) h->roundExchanged = true;
  plat_free(buf);
  return rc;
}

double asched_drf_cost(asched_t* h, const int64_t* alloc, const int64_t* total) { plat_enter(h ? h->plat : nullptr);
  double out = 0;
  if (!h) return out;
  std::vector<int64_t> a(alloc, alloc + h->R), t(total, total + h->R);
  plat_run_drf(h->dev, a, t, &out);
  return out;
}

// QueueCandidateGangIteratorPQ ordering through the round's own Less on the device (round_run.h CMD_PQ_ORDER, auxiliary kernel)
int32_t asched_pq_order(asched_t* h, int32_t n, const asched_pq_item* items, int32_t preferLarge, int32_t comparePrio, int32_t* order, int32_t* packedAgrees) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (n < 0 || n > 64) return fail(h, ASCHED_ERR_INVALID, "pq_order: n out of range");
  if (n == 0) { if (packedAgrees) *packedAgrees = 1; return 0; }
  DevBufs tmp;
  std::vector<double> prop(n), cur(n), bud(n), size(n); std::vector<int32_t> pcp(n), sp(n), nr(n), away(n);
  for (int i = 0; i < n; i++) {
    away[i] = items[i].away != 0;
    prop[i] = items[i].proposed_cost; cur[i] = items[i].current_cost; bud[i] = items[i].budget; size[i] = items[i].item_size;
    pcp[i] = items[i].pc_priority; sp[i] = items[i].scheduling_priority; nr[i] = items[i].name_rank;
  }
  Dev saved = h->dev;   // the per-queue arrays of the descriptor point at a scratch copy for this one launch
  Dev& d = h->dev;
  d.pqProposed = tmp.upload(prop); d.pqCurrent = tmp.upload(cur); d.pqBudget = tmp.upload(bud); d.pqSize = tmp.upload(size);
  d.pqPcPrio = tmp.upload(pcp); d.pqSchedPrio = tmp.upload(sp); d.qNameRank = tmp.upload(nr);
  PqOrderArgs a; memset(&a, 0, sizeof a);
  a.n = n; a.preferLarge = preferLarge != 0; a.compareSchedPrio = (comparePrio & 1) != 0; a.homeFirst = (comparePrio & ASCHED_PQ_HOME_FIRST) != 0; a.out = tmp.alloc<int32_t>((size_t)n + 1);
  a.away = tmp.upload(away);
  plat_h2d(d.cmdIO + 16, &a, sizeof a);
  int rc = runControl(h, CMD_PQ_ORDER);
  h->dev = saved;
  if (!rc) {
    std::vector<int32_t> out(n + 1);
    plat_d2h(out.data(), a.out, sizeof(int32_t) * (n + 1));
    for (int i = 0; i < n; i++) order[i] = out[i];
    if (packedAgrees) *packedAgrees = out[n];
  }
  tmp.freeAll();
  return rc;
}

int32_t asched_fair_shares(asched_t* h, int32_t q, const int32_t* nameRank, const double* weight, const double* cds, double* fair, double* dc, double* uc) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  return plat_run_fair_shares(h->dev, q, nameRank, weight, cds, fair, dc, uc) ? fail(h, ASCHED_ERR_DEVICE, plat_last_error()) : 0;
}

static int64_t multiplyResource(int64_t res, double m) {  // resource_list.go:312-331
  if (m == 1.0) return res;
  if (std::isinf(m)) return ((m < 0) == (res < 0)) ? INT64_MAX : INT64_MIN;
  return (int64_t)((double)res * m);
}

static void evrSize(asched* h);   // (the evictor report's buffers, below)
// the queued lists of round_prepare_resident (kernels_queued_lists.h): mark, hold, compact into the handle's own blocks; dev.queuedOff / dev.queuedJobs point at them
static int deriveQueuedLists(asched* h, int Q, int32_t nHeld, const int32_t* held, int* total) {
  Dev& d = h->dev;
  auto& ql = h->ql;
  const int M = h->M;
  const int ordTotal = h->ordOffHost.empty() ? 0 : h->ordOffHost[std::min<size_t>((size_t)Q, h->ordOffHost.size() - 1)];   // entries of queues < Q in the pre-sorted order
  if (!ql.flag || ql.rowCap < (size_t)M || ql.ordCap < (size_t)ordTotal) {
    const size_t rows = std::max<size_t>(std::max(h->jobCap, (size_t)M), 1), ords = std::max<size_t>(std::max(h->ordCap, (size_t)ordTotal), 1);
    ql.bufs.freeAll(); ql.rowCap = ql.ordCap = 0;
    ql.flag = ql.bufs.allocRaw<uint8_t>(4 * ((rows + 3) / 4)); ql.prefix = ql.bufs.allocRaw<uint32_t>(ords); ql.list = ql.bufs.allocRaw<int32_t>(ords);
    ql.off = ql.bufs.allocRaw<int32_t>(4096 + 2);
    if (!ql.flag || !ql.prefix || !ql.list || !ql.off) { ql.bufs.freeAll(); ql.flag = nullptr; return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
    ql.rowCap = rows; ql.ordCap = ords;
  }
  if (nHeld > 0 && ql.heldCap < (size_t)nHeld) {
    const size_t cap = std::max<size_t>((size_t)nHeld + (size_t)nHeld / 4, 256);
    ql.heldBufs.freeAll(); ql.heldCap = 0;
    ql.held = ql.heldBufs.allocRaw<int32_t>(cap);
    if (!ql.held) { ql.heldBufs.freeAll(); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
    ql.heldCap = cap;
  }
  if (nHeld > 0) plat_h2d(ql.held, held, sizeof(int32_t) * (size_t)nHeld);
  QlArgs a; memset(&a, 0, sizeof a);
  a.M = M; a.Q = Q; a.nHeld = nHeld > 0 ? nHeld : 0; a.jNode0 = d.jNode0; a.jQueue = d.jQueue; a.held = ql.held; a.flag = ql.flag;
  a.vec = (((uintptr_t)d.jNode0 | (uintptr_t)d.jQueue) & 15) == 0;
  if (plat_take_failure() || plat_queued_lists(d, a, ordTotal, ql.list, ql.prefix, ql.off, total)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  d.queuedOff = ql.off; d.queuedJobs = ql.list;
  plat_pass_ms(PASS_QL, h->qlMs);
  if (plat_pass_printed(PASS_QL))
    fprintf(stderr, "[asched round_prepare_resident] rows %d order entries %d queues %d held %d queued %d: mark %.4f ms, hold %.4f ms, compact %.4f ms\n",
            M, ordTotal, Q, a.nHeld, *total, h->qlMs[0], h->qlMs[1], h->qlMs[2]);
  return 0;
}
// everything round_prepare and round_prepare_resident share: the two differ in where dev.queuedOff / dev.queuedJobs come from (the caller's lists, uploaded; or
// deriveQueuedLists).  The entry points have checked what they refuse.
static int roundPrepareBody(asched* h, const asched_queues* in, bool resident, int32_t nHeld, const int32_t* held) {
  h->queuedValid = false;
  h->queueBufs.recycle();
  h->allocPristine = false;   // populateNodeDb binds the running jobs
  HostProf prof("round_prepare");
  Dev& d = h->dev;
  int Q = h->Q = in->q, R = h->R, npc = h->npc, M = h->M;
  if (Q > 4096) return fail(h, ASCHED_ERR_UNSUPPORTED, "more than 4096 queues");
  d.cfg.Q = Q;
  h->evrState = asched::EVR_NONE; h->evrSized = false;
  if (h->evrOn) evrSize(h);
  std::vector<int32_t> nameRank(Q); std::vector<double> weight(in->weight, in->weight + Q);
  for (int q = 0; q < Q; q++) nameRank[q] = in->name_rank ? in->name_rank[q] : q;
  std::vector<int64_t> allocByPc((size_t)Q * npc * R, 0), alloc((size_t)Q * R, 0), demand((size_t)Q * R, 0), penalty((size_t)Q * R, 0), pcLimit((size_t)Q * npc * R, 0);
  // no aggregates from the caller: the round-input builder's sums run on the device (B_AGG_RUN / B_AGG_QUEUED / SM_AGG_FIN below); ASCHED_HOST_AGG=1 or the
  // single-launch prepare keep them on the host
  static const bool hostAgg = [] { const char* e = getenv("ASCHED_HOST_AGG"); const char* s1 = getenv("ASCHED_SINGLE_LAUNCH"); return (e && e[0] == '1') || (s1 && s1[0] == '1'); }();
  const bool devAgg = !in->allocated_by_pc && !in->demand && !hostAgg;
  // the queued lists: the caller's, or derived on the device from the resident order — and read back once where the host sums the queued demand below
  const int32_t *qOffIn = in->queued_off, *qJobsIn = in->queued_jobs;
  std::vector<int32_t> queuedOff, queuedJobs;
  int queuedTotal = 0;
  if (resident) {
    if (int rc = deriveQueuedLists(h, Q, nHeld, held, &queuedTotal)) return rc;
    if (!devAgg && !in->demand) {
      queuedOff.resize((size_t)Q + 1); queuedJobs.resize((size_t)std::max(queuedTotal, 1));
      plat_d2h(queuedOff.data(), d.queuedOff, sizeof(int32_t) * ((size_t)Q + 1));
      if (queuedTotal > 0) plat_d2h(queuedJobs.data(), d.queuedJobs, sizeof(int32_t) * (size_t)queuedTotal);
      if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
      qOffIn = queuedOff.data(); qJobsIn = queuedJobs.data();
    }
    prof.lap("queued lists from the resident order");
  }
  if (in->allocated_by_pc) allocByPc.assign(in->allocated_by_pc, in->allocated_by_pc + (size_t)Q * npc * R);
  else if (!devAgg) for (int j = 0; j < M; j++) if (h->jNode[j] >= 0 && h->jQueue[j] >= 0 && h->jQueue[j] < Q)
    for (int r = 0; r < R; r++) allocByPc[((size_t)h->jQueue[j] * npc + h->jPc[j]) * R + r] += h->jReq[(size_t)j * R + r];
  std::vector<int64_t> sctxAllocated(MAXR, 0);
  for (int q = 0; q < Q; q++) for (int p = 0; p < npc; p++) for (int r = 0; r < R; r++) {
    alloc[(size_t)q * R + r] += allocByPc[((size_t)q * npc + p) * R + r];
    sctxAllocated[r] += allocByPc[((size_t)q * npc + p) * R + r];
  }
  if (in->short_job_penalty) penalty.assign(in->short_job_penalty, in->short_job_penalty + (size_t)Q * R);
  bool totalZero = true;
  for (int r = 0; r < R; r++) { d.cfg.maxToSchedule[r] = multiplyResource(d.cfg.totalResources[r], h->maxFraction[r]); if (d.cfg.totalResources[r]) totalZero = false; }
  d.hasPcLimit = in->pc_resource_limit_fraction && !totalZero;
  if (d.hasPcLimit)
    for (size_t i = 0; i < pcLimit.size(); i++) pcLimit[i] = multiplyResource(d.cfg.totalResources[i % R], in->pc_resource_limit_fraction[i]);
  if (in->demand) demand.assign(in->demand, in->demand + (size_t)Q * R);
  else if (!devAgg) {
    // the round-input builder's constrained demand (scheduling_algo.go:621-632, 805; constraints.go:187-197): requests of every
    // non-terminal job of the pool per (queue, priority class) — the queued jobs of a cordoned queue do not count —, each
    // class capped by the queue's limit for that class, then summed over the classes
    std::vector<int64_t> byPc((size_t)Q * npc * R, 0);
    for (int q = 0; q < Q; q++) {
      if (in->cordoned && in->cordoned[q]) continue;
      for (int k = qOffIn[q]; k < qOffIn[q + 1]; k++) {
        int j = qJobsIn[k];
        for (int r = 0; r < R; r++) byPc[((size_t)q * npc + h->jPc[j]) * R + r] += h->jReq[(size_t)j * R + r];
      }
    }
    for (int j = 0; j < M; j++) if (h->jNode[j] >= 0 && h->jQueue[j] >= 0 && h->jQueue[j] < Q)
      for (int r = 0; r < R; r++) byPc[((size_t)h->jQueue[j] * npc + h->jPc[j]) * R + r] += h->jReq[(size_t)j * R + r];
    for (int q = 0; q < Q; q++) for (int p = 0; p < npc; p++) for (int r = 0; r < R; r++) {
      size_t i = ((size_t)q * npc + p) * R + r;
      demand[(size_t)q * R + r] += d.hasPcLimit ? std::min(byPc[i], pcLimit[i]) : byPc[i];
    }
  }
  prof.lap("per-queue aggregates (allocation, capped demand)");
  std::vector<double> qTokens(Q); std::vector<int64_t> qBurst(Q); std::vector<uint8_t> qRateInf(Q), cordoned(Q, 0);
  for (int q = 0; q < Q; q++) {
    qBurst[q] = in->queue_burst ? in->queue_burst[q] : INT64_MAX;
    qRateInf[q] = in->queue_rate_inf ? in->queue_rate_inf[q] : 1;
    qTokens[q] = in->queue_tokens ? in->queue_tokens[q] : (double)qBurst[q];
    if (in->cordoned) cordoned[q] = in->cordoned[q];
  }
  if (!resident) {
    queuedOff.assign(in->queued_off, in->queued_off + Q + 1);
    queuedJobs.assign(in->queued_jobs, in->queued_jobs + queuedOff[Q]);
    queuedTotal = queuedOff[Q];
  }
  d.qWeight = h->queueBufs.upload(weight); d.qNameRank = h->queueBufs.upload(nameRank);
  d.qAllocByPc = h->queueBufs.upload(allocByPc); d.qAlloc = h->queueBufs.upload(alloc); d.qDemand = h->queueBufs.upload(demand);
  d.qPenalty = h->queueBufs.upload(penalty); d.qPcLimit = h->queueBufs.upload(pcLimit);
  d.qDemandByPc = nullptr;
  if (devAgg) { std::vector<int64_t> z((size_t)Q * npc * R, 0); d.qDemandByPc = h->queueBufs.upload(z); }
  d.qSchedByPc = h->queueBufs.alloc<int64_t>((size_t)Q * npc * R); d.qEvictedByPc = h->queueBufs.alloc<int64_t>((size_t)Q * npc * R);
  d.qTokens = h->queueBufs.upload(qTokens); d.qBurst = h->queueBufs.upload(qBurst); d.qRateInf = h->queueBufs.upload(qRateInf);
  d.qCordoned = h->queueBufs.upload(cordoned);
  d.qFair = h->queueBufs.alloc<double>(Q); d.qDc = h->queueBufs.alloc<double>(Q); d.qUc = h->queueBufs.alloc<double>(Q);
  if (!resident) { d.queuedOff = h->queueBufs.upload(queuedOff); d.queuedJobs = h->queueBufs.upload(queuedJobs); }   // (resident: deriveQueuedLists has set them)
  h->queuedTotal = queuedTotal; h->queuedValid = true;
  d.evOff = h->queueBufs.alloc<int32_t>(Q + 2);
  auto QI = [&]() { return h->queueBufs.alloc<int32_t>(Q + 1); };
  auto Q8 = [&]() { return h->queueBufs.alloc<uint8_t>(Q + 1); };
  auto QD = [&]() { return h->queueBufs.alloc<double>(Q + 1); };
  d.itEi = QI(); d.itQi = QI(); d.itStage = QI(); d.itJobsSeen = QI(); d.itNext = QI(); d.itStashed = QI();
  d.itJobOnlyEv = Q8(); d.itGangOnlyEv = Q8(); d.onlyEvByQueue = Q8(); d.qEvictable = Q8();
  d.pqProposed = QD(); d.pqCurrent = QD(); d.pqBudget = QD(); d.pqSize = QD(); d.pqPcPrio = QI(); d.pqSchedPrio = QI(); d.pqGctx = QI(); d.pqInHeap = Q8();
  d.replayAlloc = h->queueBufs.alloc<int64_t>((size_t)(Q + 1) * R);
  d.qAllocSnap = h->queueBufs.alloc<int64_t>((size_t)(Q + 1) * R);
  d.qNewJobNs = h->queueBufs.alloc<int64_t>((size_t)Q + 1);
  if (h->mkJobsBuilt) {   // MarketIteratorPQ, the market multi-iterator's held values, billing (round_mkt.h)
    MktDev& mk = h->mk;
    mk.heap = QI(); mk.pqPrice = QD(); mk.pqRuntime = h->queueBufs.alloc<int64_t>((size_t)Q + 1); mk.pqSubmit = h->queueBufs.alloc<int64_t>((size_t)Q + 1); mk.pqQueued = Q8();
    mk.itV1 = QI(); mk.itV2 = QI();
    mk.qBillable = h->queueBufs.alloc<int64_t>((size_t)(Q + 1) * R); mk.qOverride = QD(); mk.qHasOverride = Q8();
    mk.s = h->queueBufs.alloc<MktScalars>(1);   // zeroed: market off, no spot price
    plat_memset(mk.jobBillable, 0, (size_t)h->M + 1);
  }
  d.alt.itEi = QI(); d.alt.itQi = QI(); d.alt.itStage = QI(); d.alt.itJobsSeen = QI(); d.alt.itNext = QI(); d.alt.itStashed = QI();
  d.alt.itJobOnlyEv = Q8(); d.alt.itGangOnlyEv = Q8(); d.alt.onlyEvByQueue = Q8();
  d.alt.pqProposed = QD(); d.alt.pqCurrent = QD(); d.alt.pqBudget = QD(); d.alt.pqSize = QD(); d.alt.pqPcPrio = QI(); d.alt.pqSchedPrio = QI(); d.alt.pqGctx = QI(); d.alt.pqInHeap = Q8();
  RoundScalars rs; memset(&rs, 0, sizeof rs);
  for (int r = 0; r < R; r++) rs.allocated[r] = sctxAllocated[r];
  rs.globalTokens = in->global_tokens; rs.globalBurst = in->global_burst; rs.globalRateInf = in->global_rate_inf;
  rs.hasFpLimiter = in->has_fairshare_preemption_limiter; rs.fpTokens = in->fairshare_preemption_tokens;
  plat_h2d(d.rs, &rs, sizeof rs);
  h->prepared = true;
  d.f.iterOk = d.f.structOk && Q >= 1 && Q <= QCAPF;
  // soft time budgets are accounted per gang attempt and floating limits are checked per gang in the generic gang scheduler: no fast iterations
  if (d.cfg.maxNewJobNs > 0 || d.cfg.maxNewJobPerQueueNs > 0 || d.cfg.anyFloating) d.f.iterOk = 0;
  // Cross-pool away jobs (bound at CrossPoolPriority, ordered after home jobs): the node evictor never takes one (pqs.go:102-104), so the FIRST pass never meets one in a queue —
  // they are node state (populate binds them at -1) and possible victims of urgency preemption, both of which the fast path leaves to the generic code anyway.  The second pass
  // (after the oversubscribed evictor, which does evict them) runs on the generic code when the job set holds any: round_run.h controlMain / runRound.  (Round 3: iterOk = 0.)
  { const char* e = getenv("ASCHED_ENGINE"); d.f.engine = !(e && e[0] == '0'); }
  { const char* e = getenv("ASCHED_ENGINE_HC"); d.f.engineHc = d.f.engine && d.fitBits != nullptr && !d.f.maskMode && d.f.guardMask != 0 && d.f.F <= 128 && !(e && e[0] == '0'); }   // (guard bits: its fit test is the one-subtraction form)
  { const char* e = getenv("ASCHED_HC_SHORT"); d.f.hcShort = !(e && e[0] == '0'); }   // (engine_hc.h: off = every shape's clean-side bound reads 0, the per-job loop is the same code)
  { const char* e = getenv("ASCHED_RELOC_ALL"); d.f.relocAll = e && e[0] == '1'; }
  { const char* e = getenv("ASCHED_DEBUG_HANG"); d.f.debugHang = e ? atoi(e) : 0; }
  { const char* e = getenv("ASCHED_MERGE_MIN"); d.f.mgMin = e && atoi(e) >= 16 ? atoi(e) : MG_MIN_ENTRIES_DEFAULT; }
  if (d.f.structOk) {  // loop constants for the fast path: config + the device pointers allocated above
    d.hasPcLimit = d.hasPcLimit ? 1 : 0;
    FastK hk; memset(&hk, 0, sizeof hk);
    fastKInit(d, hk);
    std::vector<FastK> one(1, hk);
    d.fk = h->queueBufs.upload(one);
  }
  for (int q = 0; q < Q; q++) if (!(weight[q] > 0) || !std::isfinite(weight[q])) d.f.iterOk = 0;
  if (const char* e = getenv("ASCHED_NO_FAST_ITER")) if (e[0] == '1') d.f.iterOk = 0;  // debugging: every iteration through the generic code
  // More than QCAPF queues: wide runs (round_wide.h, FastCfg.iterOk == 2) under the conditions of the fast iteration and of its stream runs.  The per-queue state stays
  // in HBM (the bulk passes of a wide run read it on every workgroup); the stream buffers are sized for Q here (the ones jobs_set allocated hold QCAPF queues and are put
  // back when a later round of this handle has few queues).
  if (h->qsOrig.valid) { d.qsKey = h->qsOrig.key; d.qsIn = h->qsOrig.in; d.qsPart = h->qsOrig.part; d.qsLen = h->qsOrig.len; d.qsSave = h->qsOrig.save; h->qsOrig.valid = false; }
  {
    int wideMinQ = QCAPF + 1;
    if (const char* e = getenv("ASCHED_WIDE_MIN_Q")) { int v = atoi(e); if (v >= 1) wideMinQ = v; }   // experiment: wide runs (bulk-ranked merge) for pools of fewer queues too
    bool wide = d.f.structOk && Q >= wideMinQ && Q <= 4096 && d.qsKey != nullptr;   // (qsKey: stream runs are on, ASCHED_STREAM)
    if (d.cfg.maxNewJobNs > 0 || d.cfg.maxNewJobPerQueueNs > 0 || d.cfg.anyFloating || h->anyAway || d.hasPcLimit || h->market.enabled) wide = false;
    for (int r = 0; r < R; r++) if (d.cfg.maxToSchedule[r] != INT64_MAX || d.cfg.disallowed[r]) wide = false;   // round limits, disallowed resources: generic
    if (d.cfg.disableHome) wide = false;
    for (int q = 0; q < Q; q++) if (!(weight[q] > 0) || !std::isfinite(weight[q])) wide = false;
    if (const char* e = getenv("ASCHED_NO_FAST_ITER")) if (e[0] == '1') wide = false;
    if (const char* e = getenv("ASCHED_WIDE")) if (e[0] == '0') wide = false;   // ASCHED_WIDE=0: more than QCAPF queues on the generic path only (A/B, tests)
    if (wide) {
      h->qsOrig.valid = true; h->qsOrig.key = d.qsKey; h->qsOrig.in = d.qsIn; h->qsOrig.part = d.qsPart; h->qsOrig.len = d.qsLen; h->qsOrig.save = d.qsSave;
      d.qsKey = nullptr; d.qsPart = nullptr; d.qsLen = nullptr; d.qsIn = h->queueBufs.alloc<QsIn>(Q);   // (the wide runs have chunked passes and key arrays of their own)
      WideDev wd; memset(&wd, 0, sizeof wd);
      wd.seg = h->queueBufs.alloc<WideSeg>(Q); wd.key = h->queueBufs.alloc<WideKey>((size_t)Q * WIDE_L); wd.cmax = h->queueBufs.alloc<WideKey>((size_t)Q * (WIDE_L / 8)); wd.part = h->queueBufs.alloc<int64_t>((size_t)Q * (WIDE_L / 8) * (MAXR + 2)); wd.rank = h->queueBufs.alloc<int32_t>((size_t)Q * WIDE_L); wd.off = h->queueBufs.alloc<int32_t>(2 * (size_t)Q + 2); wd.own = h->queueBufs.alloc<int32_t>((size_t)Q * WIDE_L);
      wd.merged = h->queueBufs.alloc<WideEnt>((size_t)Q * WIDE_L + Q); wd.cnt = h->queueBufs.alloc<int32_t>(2 * (size_t)Q); wd.cap = h->queueBufs.alloc<int32_t>(Q); wd.tot = h->queueBufs.alloc<int64_t>(3 * MAXR);
      wd.stop = h->queueBufs.alloc<uint32_t>(4); wd.par = h->queueBufs.alloc<WideParams>(1);
      std::vector<WideDev> one(1, wd);
      d.wide = h->queueBufs.upload(one);
      d.f.iterOk = 2; d.f.relocAll = 0;
    }
  }
  prof.lap("uploads + per-queue state allocation");
  // ConstructNodeDb + populateNodeDb + fair shares as grid-wide kernels (every plane := allocatable, per-job state reset, running jobs bound with
  // int64 atomics, order keys rebuilt) — the same per-element bodies CMD_PREPARE runs on one workgroup (kept for ASCHED_SINGLE_LAUNCH=1)
  static const bool singlePrepare = [] { const char* e = getenv("ASCHED_SINGLE_LAUNCH"); return e && e[0] == '1'; }();
  int rc = 0;
  if (singlePrepare) rc = runControl(h, CMD_PREPARE);
  else {
    if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    const int ordTotalAgg = h->ordOffHost.empty() ? 0 : h->ordOffHost[std::min<size_t>((size_t)Q, h->ordOffHost.size() - 1)];   // jobs of queues < Q in the pre-sorted order
    if (devAgg && (plat_agg(d, 0, ordTotalAgg) || plat_agg(d, 1, queuedTotal) || plat_small(d, SM_AGG_FIN, 0))) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    if (plat_bulk(d, B_INIT_ALLOC, h->N) || plat_bulk(d, B_RESET_JOBS, M) || plat_bulk(d, B_POPULATE, M) || plat_bulk(d, B_KEYS_ALL, h->N) ||
        plat_bulk(d, B_CLEAR_UNFEASIBLE, h->S) || plat_small(d, SM_PREPARE_FIN, 0))
      return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    plat_d2h(&h->rsHost, d.rs, sizeof(RoundScalars));
    if (h->rsHost.error) {
      int e = h->rsHost.error;
      char buf[128]; snprintf(buf, sizeof buf, "device raised error %d (detail %d)", e, h->rsHost.errorDetail);
      int32_t zero[2] = {0, 0};
      plat_h2d(&d.rs->error, zero, sizeof zero);
      return fail(h, e, buf);
    }
  }
  prof.lap("populateNodeDb, keys, fair shares on the device");
  if (rc) return rc;
  if (d.f.structOk) {  // the ordered index of the fresh NodeDb (nodedb.go:1164-1175): nodes sorted by their priority -2 key
    if (plat_build_base(d)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    plat_memset(d.candPosSave, 0, sizeof(int32_t) * SMAX);
    int32_t one = 1;
    plat_h2d(&d.rs->fastActive, &one, sizeof one);
    prof.lap("sorted level-0 base");
  }
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return 0;
}
int32_t asched_round_prepare(asched_t* h, const asched_queues* in) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (h) { h->haveRoundResult = false; h->stateEpoch++; }
  if (!h->nodesSet || !h->jobsSet) return fail(h, ASCHED_ERR_INVALID, "round_prepare: nodes_upsert and jobs_set first");
  return roundPrepareBody(h, in, false, 0, nullptr);
}
// round_prepare with the queued lists derived from the resident job order (NewQueuedJobsIterator over repo.QueuedJobs, jobiteration.go:144-160).  Every refusal is
// decided here, before anything on the handle changes
int32_t asched_round_prepare_resident(asched_t* h, const asched_queues* in, int32_t nHeld, const int32_t* held) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!in) return fail(h, ASCHED_ERR_INVALID, "round_prepare_resident: no queues");
  if (in->queued_off || in->queued_jobs) return fail(h, ASCHED_ERR_INVALID, "round_prepare_resident: queued_off and queued_jobs must be NULL (the lists are derived from the resident job order; round_prepare takes explicit ones)");
  if (!h->nodesSet || !h->jobsSet) return fail(h, ASCHED_ERR_INVALID, "round_prepare_resident: nodes_upsert and jobs_set first");
  if (in->q < 0) return fail(h, ASCHED_ERR_INVALID, "round_prepare_resident: q < 0");
  if (in->q > 4096) return fail(h, ASCHED_ERR_UNSUPPORTED, "more than 4096 queues");
  if (h->mkJobsBuilt) return fail(h, ASCHED_ERR_UNSUPPORTED, "round_prepare_resident: the job set carries the market order (uploaded with bid prices or after asched_set_market), which is another order than the resident one the lists are derived from: give round_prepare the lists in that order");
  if (nHeld < 0 || (nHeld > 0 && !held)) return fail(h, ASCHED_ERR_INVALID, "round_prepare_resident: n_held < 0, or n_held > 0 without held");
  for (int32_t i = 0; i < nHeld; i++) if (held[i] < 0 || held[i] >= h->M) {
    char buf[128]; snprintf(buf, sizeof buf, "round_prepare_resident: held[%d] = %d is outside [0, %d)", i, held[i], h->M);
    return fail(h, ASCHED_ERR_INVALID, buf);
  }
  h->haveRoundResult = false; h->stateEpoch++;
  return roundPrepareBody(h, in, true, nHeld, held);
}
// the queued lists the last prepare (either form) left on the device
int32_t asched_round_queued(asched_t* h, int32_t* off, int32_t* jobs, int32_t cap) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->queuedValid) return fail(h, ASCHED_ERR_INVALID, "round_queued: no round_prepare / round_prepare_resident since the handle was created");
  if (!off) return fail(h, ASCHED_ERR_INVALID, "round_queued: off missing");
  const int total = h->queuedTotal;
  plat_d2h(off, h->dev.queuedOff, sizeof(int32_t) * ((size_t)h->Q + 1));
  if (jobs && cap >= total && total > 0) plat_d2h(jobs, h->dev.queuedJobs, sizeof(int32_t) * (size_t)total);
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return total;
}

static int downloadResult(asched* h, asched_round_result* out, const int32_t* io) {
  Dev& d = h->dev;
  int ns = io[2], np = io[3];
  h->haveRoundResult = true; h->roundExchanged = false;
  h->resNs = ns; h->resNp = np;
  const int Q = h->Q; const size_t M = (size_t)h->M, qa = (size_t)Q * h->npc * h->R;
  // carve the arena: [sched job|node|prio|method : 4 x ns i32][pre job|node : 2 x np i32][queue alloc : qa i64][fair|dc|uc|tokens : 4 x Q f64][reason : M i32]
  auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
  size_t oS = 0, oP = oS + up(4 * (size_t)ns * 4), oA = oP + up(2 * (size_t)np * 4), oF = oA + up(qa * 8), oR = oF + up(4 * (size_t)Q * 8), need = oR + up(M * 4) + 64;
  if (h->resPinBytes < need) {
    plat_pinned_free(h->resPin); h->resPin = nullptr; h->resPinBytes = 0;
    size_t cap = need + need / 4;
    h->resPin = plat_pinned(cap);
    if (!h->resPin) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    h->resPinBytes = cap;
  }
  char* b = (char*)h->resPin;
  int32_t* sJob = (int32_t*)(b + oS); int32_t *sNode = sJob + ns, *sPrio = sNode + ns, *sMeth = sPrio + ns;
  int32_t* pJob = (int32_t*)(b + oP); int32_t* pNode = pJob + np;
  int64_t* qAlloc = (int64_t*)(b + oA);
  double* qF = (double*)(b + oF); double *qDc = qF + Q, *qUc = qDc + Q, *qTok = qUc + Q;
  int32_t* reason = (int32_t*)(b + oR);
  h->resSJob = sJob; h->resSNode = sNode; h->resSPrio = sPrio; h->resPJob = pJob;
  if (ns) { plat_d2h_async(sJob, d.resJob, 4 * (size_t)ns); plat_d2h_async(sNode, d.resNode, 4 * (size_t)ns); plat_d2h_async(sPrio, d.resPrio, 4 * (size_t)ns); plat_d2h_async(sMeth, d.resMethod, 4 * (size_t)ns); }
  if (np) { plat_d2h_async(pJob, d.resPreJob, 4 * (size_t)np); plat_d2h_async(pNode, d.resPreNode, 4 * (size_t)np); }
  if (Q) {
    plat_d2h_async(qAlloc, d.qAllocByPc, qa * 8);
    plat_d2h_async(qF, d.qFair, (size_t)Q * 8); plat_d2h_async(qDc, d.qDc, (size_t)Q * 8); plat_d2h_async(qUc, d.qUc, (size_t)Q * 8); plat_d2h_async(qTok, d.qTokens, (size_t)Q * 8);
  }
  if (M) plat_d2h_async(reason, d.jcReason, M * 4);
  plat_sync();
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  memset(out, 0, sizeof *out);
  out->num_scheduled = ns; out->num_preempted = np; out->termination_reason = h->rsHost.terminationReason;
  out->num_evicted_phase1 = io[0]; out->num_evicted_phase3 = io[1];
  out->num_node_queries = h->rsHost.numNodeQueries; out->num_loop_iterations = h->rsHost.loopIterations;
  out->scheduled_job = sJob; out->scheduled_node = sNode; out->scheduled_priority = sPrio; out->scheduled_method = sMeth;
  out->preempted_job = pJob; out->preempted_node = pNode;
  out->queue_allocated_by_pc = qAlloc; out->queue_fair_share = qF;
  out->queue_demand_capped_adjusted_fair_share = qDc; out->queue_uncapped_adjusted_fair_share = qUc;
  out->job_unschedulable_reason = reason;
  out->global_tokens_after = h->rsHost.globalTokens; out->queue_tokens_after = qTok;
  return 0;
}

// ---- the evictor report (kernels_evict_report.h): its buffers, sized for the handle's nodes, jobs, queues and resources
static void evrSize(asched* h) {
  DevBufs& b = h->evrBufs;
  b.recycle();
  EvrArgs& a = h->evr; memset(&a, 0, sizeof a);
  const size_t N = (size_t)h->N, M = (size_t)h->M, Q = (size_t)h->Q, R = (size_t)h->R;
  a.N = h->N; a.M = h->M; a.Q = h->Q; a.R = h->R;
  // [qRes Q x R i64][nodeJobs N][nodeOr N][nodeEvicted N][affected 1]: the words the passes add into
  h->evrZeroBytes = Q * R * 8 + (3 * N + 1) * 4;
  char* z = (char*)b.alloc<char>(h->evrZeroBytes); h->evrZero = z;
  a.qRes = (int64_t*)z; a.nodeJobs = (int32_t*)(z + Q * R * 8); a.nodeOr = a.nodeJobs + N; a.nodeEvicted = a.nodeOr + N; a.affected = a.nodeEvicted + N;
  a.nodePreemptible = b.allocRaw<uint8_t>(N); a.nodeReasons = b.allocRaw<uint8_t>(N);
  a.qJobs = b.allocRaw<int32_t>(Q); a.qOff = b.allocRaw<int32_t>(Q + 1); a.evJob = b.allocRaw<int32_t>(M); a.evNode = b.allocRaw<int32_t>(M);
  uint8_t* u = b.allocRaw<uint8_t>(N);
  if (u && N) plat_h2d(u, h->nodeUnsched.data(), N);
  a.nodeUnsched = u;
  bool ok = true;
  for (auto& p : b.ptrs) if (!p.first) ok = false;
  h->evrSized = ok;
}
// PreemptingQueueScheduler.evict (pqs.go:291-353) for an evictor whose job filter has been evaluated into evFlag — the grid-wide form of
// round_run.h pqsEvict: every step is a kernel over all CUs; the number of evicted jobs comes back to the host (it sizes what follows).
static int evictPhaseSplit(asched* h, bool phase3, int* nOut) {
  Dev& d = h->dev;
  int M = h->M, N = h->N, Q = h->Q, R = h->R;
  int ordTotal = h->ordOffHost.empty() ? 0 : h->ordOffHost[std::min<size_t>((size_t)Q, h->ordOffHost.size() - 1)];
  if (plat_bulk(d, B_GANG_CLOSURE, h->G)) return -1;
  const bool report = !phase3 && h->evrOn && h->evrSized;
  if (report) {   // the evictor report's job and node passes: evFlag is EvictedJctxsByJobId, jobEvictedOnNode still the start-of-round state
    plat_memset(h->evrZero, 0, h->evrZeroBytes);
    if (plat_evict_report(d, h->evr, EVR_PASS_JOBS) || plat_evict_report(d, h->evr, EVR_PASS_NODES)) return -1;
  }
  if (plat_evict_apply(d, phase3 ? 1 : 0, ordTotal)) return -1;
  if (plat_bulk(d, B_KEYS_ALL, N)) return -1;
  // InMemoryJobRepository.EnqueueMany (jobiteration.go:85-108): per-queue lists in SchedulingOrderCompare order == order-preserving compaction of the pre-sorted job order
  int n = 0;
  if (plat_compact(d, d.ordAll, ordTotal, d.evFlag, d.evList, d.evSortKey, d.ordAllOff, Q, d.evOff, &n)) return -1;
  if (report) { h->evr.n1 = n; if (plat_evict_report(d, h->evr, EVR_PASS_QUEUES)) return -1; }   // (before phase 3 reuses evList / evOff)
  if (plat_bulk(d, B_RESET_EVTAB, M)) return -1;   // nodeDb.Reset() (nodedb.go:299-313)
  if (plat_small(d, SM_EVICT_POST, n)) return -1;
  if (plat_bulk(d, B_RESET_GANGSEEN, h->G)) return -1;
  if (plat_bulk(d, B_SNAP, Q * R)) return -1;
  if (d.evCheap) {
    bool fastOnHost = d.f.iterOk && !h->rsHost.apiDirty;
    if (!phase3 && fastOnHost && n > 0) {
      if (plat_bulk(d, B_EVKEYS_ON, Q) || plat_bulk(d, B_EVSUM, d.evChunks) || plat_small(d, SM_STITCH, 0) || plat_bulk(d, B_EVKEYS, d.evChunks) || plat_small(d, SM_MONO, n)) return -1;
      // addEvictedJobsToNodeDb (pqs.go:589-639) by rank instead of by walking the heap merge (replay_rank.h): when SM_MONO left the replay pending and every stream is
      // key-monotone the evicted table is built right here by a grid-wide pass, and nothing is deferred.  ASCHED_REPLAY_RANK=0: the lazy walk of rounds 1-4 (A/B, tests).
      static const bool byRank = [] { const char* e = getenv("ASCHED_REPLAY_RANK"); return !(e && e[0] == '0'); }();
      if (byRank && plat_replay_rank(d, n, 1)) return -1;
    } else {
      // the oversubscribed evictor's jobs (pass 2): the fast loop takes nothing from precomputed costs there (node / priority / bookkeeping are this round's: fastIter's
      // dynamic branch), but the REPLAY of these jobs is the same pure merge — the costs are computed for it alone, the table is built by rank, then they are switched off
      static const bool byRank3 = [] { const char* e = getenv("ASCHED_REPLAY_RANK"); return !(e && e[0] == '0'); }();
      // (not with cross-pool away jobs under preemptCrossPoolJobsFirst: Less puts home gangs before away ones (queue_scheduler.go:744-746), the rank key carries no such
      //  bit, and the oversubscribed evictor does take away jobs — the generic replay, whose pqLess applies the rule, builds the table then)
      if (phase3 && byRank3 && fastOnHost && n > 0 && !(h->anyAway && d.cfg.preferHome)) {
        if (plat_bulk(d, B_EVKEYS_ON, Q) || plat_bulk(d, B_EVSUM, d.evChunks) || plat_small(d, SM_STITCH, 0) || plat_bulk(d, B_EVKEYS, d.evChunks) || plat_small(d, SM_MONO, n) ||
            plat_replay_rank(d, n, 0)) return -1;
      }
      if (plat_bulk(d, B_EVKEYS_OFF, Q)) return -1;
    }
  }
  *nOut = n;
  return 0;
}

// PreemptingQueueScheduler.Schedule (pqs.go:86-289) as the host drives it: the data-parallel phases (evictor filters, eviction, key rebuild,
// compaction of the evicted lists, evicted-stream costs, unbind, result lists) are grid-wide kernels over all 256 CUs; the two sequential
// passes are launches of the persistent round kernel.  Everything is queued on the handle's stream; the host waits three times for a count.
// ASCHED_SINGLE_LAUNCH=1 runs the whole round inside ONE persistent launch instead (round_run.h runRound: bulk phases on one workgroup).
// fairness.go:103-105 on the host: the same IEEE operations in the same order as the device's drf() (-ffp-contract=off on both sides)
static double hostDrf(const asched* h, const int64_t* a) {
  const DevCfg& c = h->dev.cfg;
  double m = -INFINITY;
  for (int i = 0; i < c.R; i++) {
    double f = 0.0;
    if (c.totalResources[i] != 0) f = (double)a[i] / (double)c.totalResources[i];
    double x = f * c.drfMult[i];
    if (x > m) m = x;
  }
  return m > 0 ? m : 0.0;
}
static int64_t multiplyResource(int64_t res, double m);
struct OptPlaced { int32_t job, node; std::vector<int32_t> pre; double cost; };
// FairnessOptimisingGangScheduler.scheduleOnNodes (optimiser/gang_scheduler.go:100-146) for the members of one gang on the nodes of `mask` (empty: all): every member
// against EVERY node by k_opt_score, the candidate selection in node-id order, updateState (:148-190) between the members — applied tentatively to the NodeDb inside
// the caller's transaction (the reference works on node copies: the same sequence of node states) and to a host copy of the queues' CurrentCost
struct OptTentRec { int32_t job, old, node; std::vector<int32_t> ghosts; };
static int optScheduleOnNodes(asched* h, const std::vector<int32_t>& members, const std::vector<uint8_t>& mask, bool tentative, bool* scheduled, double* totalCost, std::vector<OptPlaced>& out,
                              std::vector<OptTentRec>& tent) {
  Dev& d = h->dev;
  const asched::OptCfg& o = h->opt;
  int N = h->N, Q = h->Q;
  *scheduled = false; *totalCost = 0; out.clear();
  std::vector<int32_t> byId(N);
  for (int n = 0; n < N; n++) byId[h->nodeIdRank.empty() ? n : h->nodeIdRank[n]] = n;
  std::vector<double> qCost;          // QueueContext.CurrentCost as of the current member (FromSchedulingContext, then += queueCostChanges per placed member)
  double* dOverride = nullptr; DevBufs tmp;
  for (size_t mi = 0; mi < members.size(); mi++) {
    int32_t job = members[mi];
    OptArgs a; memset(&a, 0, sizeof a);
    a.job = job; a.nowMs = o.nowMs; a.hasMaxSize = o.hasMaxSize;
    for (int r = 0; r < h->R; r++) a.maxSize[r] = o.maxSize[r];
    if (mi > 0) { if (!dOverride) dOverride = tmp.alloc<double>((size_t)Q + 1); plat_h2d(dOverride, qCost.data(), sizeof(double) * (size_t)Q); }
    d.optQDelta = mi > 0 ? dOverride : nullptr;
    std::vector<OptNodeOut> sc; double jobCost = 0;
    int rc = plat_opt_score(d, a, sc, &jobCost, -1, nullptr, nullptr);
    if (!rc && mi == 0 && members.size() > 1) { qCost.resize(Q + 1); rc = plat_opt_qcosts(d, qCost.data(), Q); }
    if (rc || plat_take_failure()) { d.optQDelta = nullptr; tmp.freeAll(); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
    int best = -1;
    for (int k = 0; k < N; k++) {
      int n = byId[k];
      const OptNodeOut& r = sc[n];
      if (r.scheduled < 0) { d.optQDelta = nullptr; tmp.freeAll(); return fail(h, ASCHED_ERR_INTERNAL, "optimiser: a node's candidate list overflowed its HBM scratch"); }
      if (!mask.empty() && !mask[n]) continue;
      if (r.scheduled <= 0) continue;
      if (r.cost == 0 && r.npre == 0) { best = n; break; }                        // no preemption required: the ideal result, exit early (:112-116)
      double improvement = ((jobCost / r.cost) * 100) - 100;                        // :118-121
      if (!(improvement > o.minPct)) continue;
      if (best < 0 || r.cost < sc[best].cost || (r.cost == sc[best].cost && r.impact < sc[best].impact)) best = n;   // nodeCostOrder; equal -> the earlier id
    }
    if (best < 0) { d.optQDelta = nullptr; tmp.freeAll(); return 0; }              // scheduled: false (:129-131)
    OptPlaced pl; pl.job = job; pl.node = best; pl.cost = sc[best].cost;
    if (sc[best].npre > 0) {
      OptNodeOut det; std::vector<int32_t> pre;
      std::vector<OptNodeOut> dummy; double jc2;
      if (plat_opt_score(d, a, dummy, &jc2, best, &det, &pre, true)) { d.optQDelta = nullptr; tmp.freeAll(); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
      pl.pre.assign(pre.begin(), pre.begin() + det.npre);
    }
    *totalCost += pl.cost;
    if (tentative || mi + 1 < members.size()) {   // updateState: the victims leave the node, the job is bound; the victims' queues get cheaper
      std::vector<int32_t> ta{job, best, (int32_t)pl.pre.size()};
      ta.insert(ta.end(), pl.pre.begin(), pl.pre.end());
      setArgs(h, ta);
      rc = runControl(h, CMD_OPT_TENT);
      if (rc) { d.optQDelta = nullptr; tmp.freeAll(); return rc; }
      { int32_t io2[2]; getIO(h, io2, 2);
        OptTentRec tr; tr.job = job; tr.old = io2[0]; tr.node = best;
        if (io2[1] > 0) { tr.ghosts.resize(io2[1]); plat_d2h(tr.ghosts.data(), d.cmdIO + 2, sizeof(int32_t) * (size_t)io2[1]); }
        if (tr.old >= 0 || !tr.ghosts.empty()) tent.push_back(tr); }
      if (!qCost.empty()) {
        std::map<int32_t, double> change;                                           // queueCostChanges: per queue, the victims' costs in preemption order (node_scheduler.go:84-99)
        for (int32_t v : pl.pre) { auto it = change.find(h->jQueue[v]); if (it == change.end()) it = change.emplace(h->jQueue[v], 0.0).first; it->second -= hostDrf(h, &h->jReq[(size_t)v * h->R]); }
        for (auto& kv : change) qCost[kv.first] += kv.second;                       // queue.CurrentCost += costChange (:182-188)
      }
    }
    out.push_back(pl);
  }
  d.optQDelta = nullptr; tmp.freeAll();
  *scheduled = true;
  return 0;
}
// runOptimiser (pqs.go:666-710) -> OptimisingQueueScheduler.Schedule (optimising_queue_scheduler.go:58-180), the loop on the host, one gang per turn
static int runOptimiserPhase(asched* h) {
  Dev& d = h->dev;
  const asched::OptCfg& o = h->opt;
  int R = h->R;
  int rc = runControl(h, CMD_OPT_BEGIN);
  if (rc) return rc;
  OptLoopArgs la; memset(&la, 0, sizeof la);
  la.hasMinSize = o.hasMinSize;
  for (int r = 0; r < R; r++) { la.maxToSchedule[r] = multiplyResource(d.cfg.totalResources[r], o.maxFraction.empty() ? INFINITY : o.maxFraction[r]); la.minSize[r] = o.minSize[r]; }
  int nScheduled = 0; bool first = true;
  while (nScheduled < o.maxJobs) {
    la.first = first ? 1 : 0; first = false;
    std::vector<int32_t> w(sizeof(OptLoopArgs) / 4);
    memcpy(w.data(), &la, sizeof la);
    setArgs(h, w);
    if ((rc = runControl(h, CMD_OPT_NEXT)) != 0) break;
    int32_t io[4]; getIO(h, io, 4);
    if (!io[0]) break;
    int cnt = io[1], q = io[2], uniSlot = io[3];
    std::vector<int32_t> members(cnt);
    plat_d2h(members.data(), d.preList, sizeof(int32_t) * (size_t)cnt);
    // FairnessOptimisingGangScheduler.Schedule (:45-94): node groups by the gang's uniformity label, the cheapest group that takes every member
    int reason = 0;
    std::vector<std::vector<uint8_t>> groups;
    if (uniSlot == -2) reason = ASCHED_REASON_UNIFORMITY_LABEL_NOT_INDEXED;
    else if (uniSlot >= 0) {
      const std::vector<int32_t>& values = h->slotValues[uniSlot];
      if (values.empty()) reason = ASCHED_REASON_NO_NODES_WITH_UNIFORMITY_LABEL;
      for (int32_t v : values) {                                                    // (ascending interned value: the reference iterates a Go map)
        std::vector<uint8_t> m(h->N, 0);
        for (int n = 0; n < h->N; n++) for (auto& l : h->nodeLabels[n]) if (l.key == h->labelSlots[uniSlot] && l.value == v) m[n] = 1;
        groups.push_back(m);
      }
    } else groups.push_back({});
    bool have = false; double bestCost = 0; std::vector<OptPlaced> best;
    bool tentative = groups.size() > 1;
    for (size_t gi = 0; gi < groups.size() && !reason; gi++) {
      bool sch = false; double cost = 0; std::vector<OptPlaced> res; std::vector<OptTentRec> tent;
      bool txn = tentative || cnt > 1;
      if (txn && (rc = runControl(h, CMD_TXN_BEGIN)) != 0) break;
      rc = optScheduleOnNodes(h, members, groups[gi], tentative, &sch, &cost, res, tent);
      if (txn) { int rc2 = runControl(h, CMD_TXN_ABORT); if (!rc) rc = rc2; }       // scheduleOnNodes works on copies: nothing of it stays in the NodeDb
      for (auto it = tent.rbegin(); it != tent.rend() && !rc; ++it) {                 // ... including what the undo log does not cover (ghosts)
        std::vector<int32_t> ua{it->job, it->old, it->node, (int32_t)it->ghosts.size()};
        ua.insert(ua.end(), it->ghosts.begin(), it->ghosts.end());
        setArgs(h, ua);
        rc = runControl(h, CMD_OPT_TENT_UNDO);
      }
      if (rc) break;
      if (sch && (!have || cost < bestCost)) { have = true; bestCost = cost; best = res; }   // sort.Sort(schedulingCostOrder): ties -> the earlier group
    }
    if (rc) break;
    if (!have) {
      if (!reason) reason = cnt > 1 ? ASCHED_REASON_GANG_DOES_NOT_FIT : ASCHED_REASON_JOB_DOES_NOT_FIT;
      if (cnt == 1) { setArgs(h, {members[0], reason}); if ((rc = runControl(h, CMD_OPT_FAIL)) != 0) break; }   // updateUnfeasibleSchedulingKeys: single-job gangs only
      continue;
    }
    std::vector<int32_t> a{cnt, q};
    for (const OptPlaced& pl : best) { a.push_back(pl.job); a.push_back(pl.node); a.push_back((int32_t)pl.pre.size()); a.insert(a.end(), pl.pre.begin(), pl.pre.end()); }
    setArgs(h, a);
    if ((rc = runControl(h, CMD_OPT_APPLY)) != 0) break;
    nScheduled += cnt;
    for (int32_t j : members) for (int r = 0; r < R; r++) la.current[r] += h->jReq[(size_t)j * R + r];
  }
  int rc2 = runControl(h, CMD_OPT_END);   // the optimiser's result lists into the round's sets
  return rc ? rc : rc2;
}
static int runRoundSplit(asched* h, int32_t* io) {
  h->stateEpoch++;
  Dev& d = h->dev;
  int M = h->M, N = h->N;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  plat_round_begin();
  auto t0 = now();
  int n1 = 0, n3 = 0, ns = 0, np = 0, rc = 0;
  do {
    if (plat_small(d, SM_QEVICTABLE, 0) || plat_bulk(d, B_FILTER1, M) || evictPhaseSplit(h, false, &n1)) { rc = -1; break; }
    if (plat_small(d, SM_LVL0_BEGIN, 0) || plat_bulk(d, B_LVL0, N)) { rc = -1; break; }
    h->roundPhaseMs[0] = ms(t0, now());
    setArgs(h, {n1});
    if ((rc = runControl(h, CMD_PASS1)) != 0) break;
    auto t1 = now();
    if (plat_bulk(d, B_NODE_OVER, N) || plat_bulk(d, B_FILTER3, M) || evictPhaseSplit(h, true, &n3)) { rc = -1; break; }
    h->roundPhaseMs[1] = ms(t1, now());
    if (n3 > 0) {
      setArgs(h, {n3});
      if ((rc = runControl(h, CMD_PASS2)) != 0) break;
    }
    if (h->opt.enabled && (rc = runOptimiserPhase(h)) != 0) break;   // pqs.go:224-253: after the second pass, before the unbinding
    auto t2 = now();
    if (plat_bulk(d, B_UNBIND, M) || plat_bulk(d, B_KEYS_ALL, N) || plat_small(d, SM_FINAL, 0)) { rc = -1; break; }
    if (plat_compact(d, nullptr, M, d.inScheduled, d.resJob, nullptr, nullptr, 0, nullptr, &ns) || plat_compact(d, nullptr, M, d.inPreempted, d.resPreJob, nullptr, nullptr, 0, nullptr, &np)) { rc = -1; break; }
    if (plat_bulk(d, B_GATHER_SCHED, ns) || plat_bulk(d, B_GATHER_PRE, np)) { rc = -1; break; }
    h->roundPhaseMs[2] = ms(t2, now());
  } while (false);
  plat_round_end();
  if (rc == -1) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (rc) return rc;
  plat_d2h(&h->rsHost, d.rs, sizeof(RoundScalars));   // SM_FINAL wrote the termination reason after the last control launch
  if (h->rsHost.error) {   // raised by a grid-wide phase (e.g. a packed key field out of range)
    int e = h->rsHost.error;
    int32_t zero[2] = {0, 0};
    plat_h2d(&d.rs->error, zero, sizeof zero);
    char buf[128]; snprintf(buf, sizeof buf, "device raised error %d (detail %d)", e, h->rsHost.errorDetail);
    return fail(h, e, buf);
  }
  double t[3]; plat_round_times(t);
  h->roundTotalMs = t[0]; h->roundControlMs = t[1]; h->roundLaunches = (int)t[2];
  io[0] = n1; io[1] = n3; io[2] = ns; io[3] = np;
  return 0;
}

int32_t asched_schedule_round(asched_t* h, asched_round_result* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h || !out) return ASCHED_ERR_INVALID;
  if (!h->prepared) return fail(h, ASCHED_ERR_INVALID, "schedule_round: round_prepare first");
  static const bool singleEnv = [] { const char* e = getenv("ASCHED_SINGLE_LAUNCH"); return e && e[0] == '1'; }();
  const bool single = singleEnv && !h->opt.enabled;   // (the optimiser's phase sits between the launches of the split round)
  int32_t io[4];
  h->evrState = asched::EVR_NONE;
  if (h->evrOn && !h->evrSized && !h->market.enabled && !single) evrSize(h);   // (the switch was turned on after round_prepare)
  if (h->market.enabled) {
    // a market-driven round (round_mkt.h): the whole of PreemptingQueueScheduler.Schedule in ONE launch of the auxiliary kernel — its code lives in that kernel's
    // code object only, and it is the generic path throughout (a literal container/heap picks the queue: there is no packed key to sort by)
    if (!h->mkJobsBuilt) return fail(h, ASCHED_ERR_INVALID, "schedule_round: market-driven scheduling needs a job set uploaded with bid prices or after asched_set_market");
    MktScalars ms; memset(&ms, 0, sizeof ms);
    ms.market = 1; ms.spotCutoff = h->market.spotCutoff;
    plat_h2d(h->mk.s, &ms, sizeof ms);
    plat_set_market_dev(&h->mk);
    int rc = runControl(h, CMD_MARKET_ROUND);
    plat_set_market_dev(nullptr);
    if (rc) return rc;
    h->roundMs = plat_last_control_ms(); h->roundLaunches = plat_last_control_launches();
    h->roundTotalMs = h->roundControlMs = h->roundMs;
    getIO(h, io, 4);
    if (h->evrOn) h->evrState = asched::EVR_MARKET;
  } else if (single) {
    int rc = runControl(h, CMD_ROUND);
    if (rc) return rc;
    h->roundMs = plat_last_control_ms(); h->roundLaunches = plat_last_control_launches();
    h->roundTotalMs = h->roundControlMs = h->roundMs;
    getIO(h, io, 4);
    if (h->evrOn) h->evrState = asched::EVR_SINGLE;
  } else {
    const bool report = h->evrOn && h->evrSized;
    int rc = runRoundSplit(h, io);
    if (rc) return rc;
    h->roundMs = h->roundTotalMs;
    if (report) { h->evrState = asched::EVR_VALID; plat_pass_ms(PASS_EVR, h->evrMs); }
  }
  return downloadResult(h, out, io);
}
// ---- the indicative gang pricer (scheduling/pricer; round_price.h)
static void priceArgsOf(asched* h, int32_t job, int64_t nowMs, PriceArgs* a) {
  memset(a, 0, sizeof *a);
  a->job = job; a->nowMs = nowMs; a->bid = h->mk.jBid;
  a->gang = h->jGangDense[job];   // excludedJobIds = the gang's own members (gang_pricer.go:121-123); a job outside a gang protects only itself
}
int32_t asched_price_job_on_nodes(asched_t* h, int32_t job, int64_t nowMs, asched_price_node_score* perNode, int32_t detailNode, int32_t* preempted, int32_t cap) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->prepared || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "price_job_on_nodes: round_prepare first / bad job");
  if (detailNode >= h->N) return fail(h, ASCHED_ERR_INVALID, "price_job_on_nodes: bad node");
  PriceArgs a; priceArgsOf(h, job, nowMs, &a);
  a.gang = -1;   // MinPriceNodeScheduler.Schedule(jctx, node, set.New(jctx.JobId)) as the node scheduler's own tests call it
  std::vector<PriceNodeOut> sc; std::vector<int32_t> pre;
  h->lastWideWasOpt = true;
  if (plat_take_failure() || plat_price_score(h->dev, a, sc, detailNode, &pre)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  for (int n = 0; n < h->N && perNode; n++) { perNode[n].scheduled = sc[n].scheduled; perNode[n].num_preempted = sc[n].npre; perNode[n].price = sc[n].price; }
  if (detailNode >= 0 && preempted) for (int i = 0; i < sc[detailNode].npre && i < cap; i++) preempted[i] = pre[i];
  return 0;
}
// GangPricer.Price (gang_pricer.go:48-117): per uniformity group scheduleOnNodes (:119-161) with updateState (:163-195) applied inside a NodeDb transaction that is aborted
int32_t asched_price_gang(asched_t* h, int32_t n, const int32_t* jobs, int64_t nowMs, asched_gang_price* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h || !out) return ASCHED_ERR_INVALID;
  memset(out, 0, sizeof *out);
  if (!h->prepared || n < 1 || !jobs) return fail(h, ASCHED_ERR_INVALID, "price_gang: round_prepare first / empty gang");
  for (int i = 0; i < n; i++) if (jobs[i] < 0 || jobs[i] >= h->M) return fail(h, ASCHED_ERR_INVALID, "price_gang: bad job");
  int N = h->N;
  out->evaluated = 1;
  // gctx.NodeUniformity: the gang's uniformity label (asched_jobs.gang_uniformity_label of its first member); isValidNodeUniformityLabel (:214-225)
  int32_t label = h->jGangDense[jobs[0]] >= 0 && !h->jGangUniKey.empty() ? h->jGangUniKey[jobs[0]] : -1;
  std::vector<std::vector<int32_t>> groups;
  if (label != -1) {
    if (!h->indexedLabels.count(label)) { out->reason = ASCHED_PRICE_REASON_LABEL_NOT_INDEXED; return 0; }
    std::map<int32_t, std::vector<int32_t>> byValue;                       // groupNodesByNodeUniformityLabel :197-212; groups in ascending interned value
    for (int k = 0; k < N; k++) for (auto& l : h->nodeLabels[k]) if (l.key == label) byValue[l.value].push_back(k);
    if (byValue.empty()) { out->reason = ASCHED_PRICE_REASON_NO_NODES_WITH_LABEL; return 0; }
    for (auto& kv : byValue) groups.push_back(kv.second);
  } else { std::vector<int32_t> g(N); for (int k = 0; k < N; k++) g[k] = k; groups.push_back(g); }
  std::vector<int32_t> idRankOf(N);
  for (int k = 0; k < N; k++) idRankOf[k] = h->nodeIdRank.empty() ? k : h->nodeIdRank[k];
  h->lastWideWasOpt = true;
  bool any = false; double best = 0;
  for (auto& g : groups) {
    std::sort(g.begin(), g.end(), [&](int32_t a, int32_t b) { return idRankOf[a] < idRankOf[b]; });   // nodeDb.GetNodes(): the id index
    h->allocPristine = false;
    int rc = runControl(h, CMD_TXN_BEGIN);
    if (rc) return rc;
    bool ok = true; double cost = 0;
    for (int m = 0; m < n && ok; m++) {
      PriceArgs a; priceArgsOf(h, jobs[m], nowMs, &a);
      std::vector<PriceNodeOut> sc; std::vector<int32_t> pre;
      if (plat_take_failure() || plat_price_score(h->dev, a, sc, -1, nullptr)) { runControl(h, CMD_TXN_ABORT); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
      int chosen = -1;
      for (int32_t nd : g) {                                              // :126-141, then sort.Sort(nodeCostOrder): price, random ULID -> the earlier id
        if (!sc[nd].scheduled) continue;
        if (chosen < 0 || sc[nd].price < sc[chosen].price) chosen = nd;
        if (sc[nd].price == 0) break;                                     // no preemption required: exit early
      }
      if (chosen < 0) { ok = false; break; }
      cost = std::max(cost, sc[chosen].price);
      if (sc[chosen].npre > 0) {                                          // the victims of the chosen node, in order
        std::vector<PriceNodeOut> dummy;
        if (plat_price_score(h->dev, a, dummy, chosen, &pre)) { runControl(h, CMD_TXN_ABORT); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
        for (int i = 0; i < sc[chosen].npre; i++) { setArgs(h, {pre[i], chosen}); rc = runControl(h, CMD_UNBIND); if (rc) { runControl(h, CMD_TXN_ABORT); return rc; } }   // UnbindJobsFromNode
      }
      setArgs(h, {jobs[m], chosen, h->pcPriority[h->jPc[jobs[m]]]});      // BindJobToNode at the class priority
      rc = runControl(h, CMD_BIND);
      if (rc) { runControl(h, CMD_TXN_ABORT); return rc; }
    }
    rc = runControl(h, CMD_TXN_ABORT);
    if (rc) return rc;
    if (ok && (!any || cost < best)) { any = true; best = cost; }         // sort.Sort(schedulingCostOrder): cost, random ULID -> the earlier group
  }
  if (!any) { out->reason = n > 1 ? ASCHED_REASON_GANG_DOES_NOT_FIT : ASCHED_REASON_JOB_DOES_NOT_FIT; return 0; }
  out->schedulable = 1; out->price = best;
  return 0;
}
int32_t asched_set_market(asched_t* h, const asched_market_config* c) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h) return ASCHED_ERR_INVALID;
  h->market.enabled = c && c->enabled; h->market.spotCutoff = h->market.enabled ? c->spot_price_cutoff : 0.0;
  return 0;
}
int32_t asched_market_result(asched_t* h, asched_market_outcome* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h || !out) return ASCHED_ERR_INVALID;
  memset(out, 0, sizeof *out);
  int Q = h->Q, R = h->R;
  h->resBillable.assign((size_t)Q * R + 1, 0); h->resOverride.assign((size_t)Q + 1, 0.0); h->resHasOverride.assign((size_t)Q + 1, 0);
  if (h->haveRoundResult && h->market.enabled && h->mk.qBillable && h->mk.s) {
    MktScalars ms; plat_d2h(&ms, h->mk.s, sizeof ms);
    out->has_spot_price = ms.hasSpotPrice; out->spot_price = ms.hasSpotPrice ? ms.spotPrice : 0.0;
    if (Q) {
      plat_d2h(h->resBillable.data(), h->mk.qBillable, (size_t)Q * R * 8);
      plat_d2h(h->resOverride.data(), h->mk.qOverride, (size_t)Q * 8); plat_d2h(h->resHasOverride.data(), h->mk.qHasOverride, (size_t)Q);
      for (auto& v : h->resBillable) if (v < 0) v = 0;   // GetBillableResource: FloorAtZero (context/queue.go:121-123)
    }
  }
  out->queue_billable_resource = h->resBillable.data(); out->queue_billable_price_override = h->resOverride.data(); out->queue_has_price_override = h->resHasOverride.data();
  return 0;
}
// Measurement hook: device time of the last schedule_round.  out = {whole sequence ms (events on the stream), persistent k_control launches ms,
// kernel launches, host ms of the evict-1 / evict-3 / final bulk phases incl. their count read-backs, ms of the evictor report's job + node passes, of its queue
// pass (ASCHED_EVR_TIMES=1 and the report on: events around them; else 0)}
int32_t asched_round_timing(asched_t* h, double* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  out[0] = h->roundTotalMs; out[1] = h->roundControlMs; out[2] = h->roundLaunches; out[3] = h->roundPhaseMs[0]; out[4] = h->roundPhaseMs[1]; out[5] = h->roundPhaseMs[2];
  const bool evr = h->evrState == asched::EVR_VALID;
  out[6] = evr ? h->evrMs[0] + h->evrMs[1] : 0; out[7] = evr ? h->evrMs[2] : 0;
  return 0;
}
int32_t asched_schedule_queues(asched_t* h, asched_round_result* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->prepared) return fail(h, ASCHED_ERR_INVALID, "schedule_queues: round_prepare first");
  int rc;
  if (h->market.enabled) {   // the market iterators and the spot price live in the auxiliary kernel (round_mkt.h)
    if (!h->mkJobsBuilt) return fail(h, ASCHED_ERR_INVALID, "schedule_queues: market-driven scheduling needs a job set uploaded with bid prices or after asched_set_market");
    MktScalars ms; memset(&ms, 0, sizeof ms);
    ms.market = 1; ms.spotCutoff = h->market.spotCutoff;
    plat_h2d(h->mk.s, &ms, sizeof ms);
    plat_set_market_dev(&h->mk);
    rc = runControl(h, CMD_MARKET_QUEUES);
    plat_set_market_dev(nullptr);
  } else rc = runControl(h, CMD_QUEUES_ONLY);
  if (rc) return rc;
  h->roundMs = plat_last_control_ms(); h->roundLaunches = plat_last_control_launches();
  int32_t io[4]; getIO(h, io, 4);
  io[0] = io[1] = 0;
  return downloadResult(h, out, io);
}
// ---- preemption causes (include/armada_sched.h; kernels_preempt_join.h): the scratch of one join, the passes, the download and the size check
static int preemptJoinRun(asched* h, PjArgs& a, const char* who, asched_preemption_cause* out, int32_t cap, int32_t* candidates, int32_t candCap, int32_t* numCandidates) {
  DevBufs& b = h->pjBufs;
  const size_t N = (size_t)a.N, ns = (size_t)a.ns, np = (size_t)a.np;
  a.cnt = b.alloc<int32_t>(N + 1); a.off = b.allocRaw<int32_t>(N + 1); a.cursor = b.allocRaw<int32_t>(N); a.tileSum = b.allocRaw<int32_t>((size_t)pjTiles(a.N));
  a.slot = b.allocRaw<int32_t>(ns); a.cand = b.allocRaw<int32_t>(ns); a.cause = b.allocRaw<asched_preemption_cause>(np); a.info = b.alloc<int32_t>(2);
  if (a.fromRound) { a.pBy = b.allocRaw<int32_t>(np); a.pSib = b.allocRaw<int32_t>(np); a.pGang = b.allocRaw<uint8_t>(np); }
  int rc = 0;
  for (auto& p : b.ptrs) if (!p.first) rc = ASCHED_ERR_DEVICE;
  if (rc || plat_take_failure() || plat_preempt_join(h->dev, a)) { b.recycle(); return fail(h, ASCHED_ERR_DEVICE, plat_last_error()); }
  int32_t total = 0, info[2] = {0, 0};
  plat_d2h(&total, a.off + N, sizeof total); plat_d2h(info, a.info, sizeof info);
  char buf[192];
  if (info[0]) { snprintf(buf, sizeof buf, "%s: %d marked job(s) without a preemptor on record", who, info[0]); rc = ASCHED_ERR_INTERNAL; }
  else if (info[1]) { snprintf(buf, sizeof buf, "%s: %d scheduled entr(ies) name a node outside the handle's nodes", who, info[1]); rc = ASCHED_ERR_INVALID; }
  else if (cap < a.np || candCap < total) {
    snprintf(buf, sizeof buf, "%s: buffers too small: %d cause records and %d candidate words are needed (cap %d, cand_cap %d)", who, a.np, total, cap, candCap);
    rc = ASCHED_ERR_INVALID;
  }
  if (numCandidates) *numCandidates = total;
  if (!rc) {
    if (np) plat_d2h(out, a.cause, np * sizeof(asched_preemption_cause));
    if (total) plat_d2h(candidates, a.cand, (size_t)total * 4);
  }
  b.recycle();
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  return rc ? fail(h, rc, buf) : 0;
}
int32_t asched_round_preemption_causes(asched_t* h, asched_preemption_cause* out, int32_t cap, int32_t* candidates, int32_t candCap, int32_t* numCandidates) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (numCandidates) *numCandidates = 0;
  if (!h->haveRoundResult) return fail(h, ASCHED_ERR_INVALID, "round_preemption_causes: no round result on this handle (schedule_round / schedule_queues first)");
  if (h->roundExchanged) return fail(h, ASCHED_ERR_INVALID, "round_preemption_causes: not after round_exchange (the queue-hash mode resolves preemptions between replicas; the per-job record describes this replica's own round)");
  if (cap < 0 || candCap < 0 || (cap > 0 && !out) || (candCap > 0 && !candidates)) return fail(h, ASCHED_ERR_INVALID, "round_preemption_causes: bad buffer");
  Dev& d = h->dev;
  PjArgs a; memset(&a, 0, sizeof a);
  a.N = h->N; a.ns = h->resNs; a.np = h->resNp; a.fromRound = 1;
  a.sJob = d.resJob; a.sNode = d.resNode; a.sMethod = d.resMethod; a.pNode = d.resPreNode;
  return preemptJoinRun(h, a, "round_preemption_causes", out, cap, candidates, candCap, numCandidates);
}
int32_t asched_preemption_join(asched_t* h, int32_t ns, const int32_t* sJob, const int32_t* sNode, const int32_t* sMethod, int32_t np, const int32_t* pNode, const int32_t* pBy,
                               const int32_t* pSib, const uint8_t* pGang, asched_preemption_cause* out, int32_t* candidates, int32_t candCap, int32_t* numCandidates) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (numCandidates) *numCandidates = 0;
  if (ns < 0 || np < 0 || candCap < 0 || (ns > 0 && (!sJob || !sNode || !sMethod)) || (np > 0 && (!pNode || !pBy || !pSib || !pGang || !out)) || (candCap > 0 && !candidates))
    return fail(h, ASCHED_ERR_INVALID, "preemption_join: bad argument");
  if (!h->nodesSet) return fail(h, ASCHED_ERR_INVALID, "preemption_join: nodes_upsert first");
  DevBufs& b = h->pjBufs;
  auto up32 = [&](const int32_t* p, int n) { int32_t* q = b.allocRaw<int32_t>((size_t)n); if (q && n) plat_h2d(q, p, (size_t)n * 4); return q; };
  PjArgs a; memset(&a, 0, sizeof a);
  a.N = h->N; a.ns = ns; a.np = np; a.fromRound = 0;
  a.sJob = up32(sJob, ns); a.sNode = up32(sNode, ns); a.sMethod = up32(sMethod, ns); a.pNode = up32(pNode, np); a.pBy = up32(pBy, np); a.pSib = up32(pSib, np);
  a.pGang = b.allocRaw<uint8_t>((size_t)np);
  if (a.pGang && np) plat_h2d(a.pGang, pGang, (size_t)np);
  return preemptJoinRun(h, a, "preemption_join", out, np, candidates, candCap, numCandidates);
}
// ---- the evictor report of the last round (include/armada_sched.h; kernels_evict_report.h)
int32_t asched_set_evictor_report(asched_t* h, int32_t on) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if ((on != 0) != h->evrOn) { h->evrOn = on != 0; h->evrState = asched::EVR_NONE; h->evrSized = false; }   // (the buffers are sized at the next round_prepare or round)
  if (!h->evrOn) h->evrBufs.recycle();
  return 0;
}
int32_t asched_round_evictor_report(asched_t* h, asched_evictor_report* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!out) return fail(h, ASCHED_ERR_INVALID, "round_evictor_report: no output struct");
  memset(out, 0, sizeof *out);
  if (!h->evrOn) return fail(h, ASCHED_ERR_INVALID, "round_evictor_report: the report is switched off (asched_set_evictor_report before the round)");
  if (h->market.enabled || h->evrState == asched::EVR_MARKET)
    return fail(h, ASCHED_ERR_UNSUPPORTED, "round_evictor_report: a market-driven round is one launch of the auxiliary kernel: the passes that record the report run between the launches of the split round");
  if (h->evrState == asched::EVR_SINGLE)
    return fail(h, ASCHED_ERR_UNSUPPORTED, "round_evictor_report: ASCHED_SINGLE_LAUNCH=1 runs the round in one launch: the passes that record the report run between the launches of the split round");
  if (h->evrState != asched::EVR_VALID || !h->haveRoundResult)
    return fail(h, ASCHED_ERR_INVALID, "round_evictor_report: no completed schedule_round with the report switched on (none since the switch or round_prepare, or the last one failed or timed out)");
  if (h->roundExchanged)
    return fail(h, ASCHED_ERR_UNSUPPORTED, "round_evictor_report: not after round_exchange (the queue-hash mode resolves preemptions between replicas; the report describes this replica's own round)");
  const EvrArgs& a = h->evr;
  const size_t N = (size_t)a.N, Q = (size_t)a.Q, R = (size_t)a.R, n1 = (size_t)a.n1;
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  int32_t affected = 0;
  h->evrNodePre.assign(N + 1, 0); h->evrNodeReasons.assign(N + 1, 0); h->evrNodeEvicted.assign(N + 1, 0);
  h->evrQJobs.assign(Q + 1, 0); h->evrQRes.assign(Q * R + 1, 0); h->evrQOff.assign(Q + 1, 0); h->evrJob.assign(n1 + 1, 0); h->evrNode.assign(n1 + 1, 0);
  if (N) { plat_d2h(h->evrNodePre.data(), a.nodePreemptible, N); plat_d2h(h->evrNodeReasons.data(), a.nodeReasons, N); }
  plat_d2h(h->evrNodeEvicted.data(), a.nodeEvicted, (N + 1) * 4);   // (the affected-node count sits directly behind the N counters: evrSize)
  if (Q) { plat_d2h(h->evrQJobs.data(), a.qJobs, Q * 4); plat_d2h(h->evrQRes.data(), a.qRes, Q * R * 8); }
  plat_d2h(h->evrQOff.data(), a.qOff, (Q + 1) * 4);
  if (n1) { plat_d2h(h->evrJob.data(), a.evJob, n1 * 4); plat_d2h(h->evrNode.data(), a.evNode, n1 * 4); }
  affected = h->evrNodeEvicted[N];
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  if (h->evrQOff[Q] != a.n1) return fail(h, ASCHED_ERR_INTERNAL, "round_evictor_report: the per-queue offsets do not end at the number of evicted jobs");
  out->num_nodes = a.N; out->num_queues = a.Q; out->num_resources = a.R; out->num_evicted = a.n1; out->num_affected_nodes = affected;
  out->node_preemptible = h->evrNodePre.data(); out->node_reasons = h->evrNodeReasons.data(); out->node_evicted_jobs = h->evrNodeEvicted.data();
  out->queue_evicted_jobs = h->evrQJobs.data(); out->queue_evicted_resources = h->evrQRes.data(); out->queue_evicted_off = h->evrQOff.data();
  out->evicted_job = h->evrJob.data(); out->evicted_node = h->evrNode.data();
  if (plat_pass_printed(PASS_EVR))
    fprintf(stderr, "[asched evict_report] nodes %d jobs %d evicted %d: job pass %.4f ms, node pass %.4f ms, queue pass %.4f ms\n", a.N, a.M, a.n1, h->evrMs[0], h->evrMs[1], h->evrMs[2]);
  return 0;
}
int32_t asched_gang_schedule(asched_t* h, int32_t n, const int32_t* jobs, int32_t* ok, int32_t* reason, asched_pod_result* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->prepared) return fail(h, ASCHED_ERR_INVALID, "gang_schedule: round_prepare first");
  if (n < 1 || n > 65536 || n > std::max(h->M, 1)) return fail(h, ASCHED_ERR_INVALID, "gang_schedule: bad cardinality");
  for (int i = 0; i < n; i++) if (jobs[i] < 0 || jobs[i] >= h->M) return fail(h, ASCHED_ERR_INVALID, "gang_schedule: bad job");
  std::vector<int32_t> a{n};
  for (int i = 0; i < n; i++) a.push_back(jobs[i]);
  setArgs(h, a);
  int rc = runControl(h, CMD_GANG_SCHEDULE);
  if (rc) return rc;
  int32_t io[2]; getIO(h, io, 2);
  *ok = io[0]; *reason = io[1];
  for (int i = 0; i < n; i++) {
    uint8_t has; plat_d2h(&has, h->dev.jcHasPctx + jobs[i], 1);
    if (has) readPod(h, jobs[i], &out[i]);
    else { out[i].node = -1; out[i].scheduled_at_priority = 0; out[i].preempted_at_priority = ASCHED_MIN_PRIORITY; out[i].method = 0; }
  }
  return 0;
}
int32_t asched_round_stats(asched_t* h, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  plat_d2h(&h->rsHost, h->dev.rs, sizeof(RoundScalars));
  const RoundScalars& r = h->rsHost;
  for (int i = 0; i < 25; i++) out[i] = 0;
  out[20] = r.statHybrid;
  out[21] = r.statHcShort;
  out[22] = r.statNestGangs;   // (CPU build only: the device leaves it 0)
  out[23] = r.statOverCap;     // (CPU build only: the device leaves it 0)
  out[24] = (int32_t)(r.statSeg[HC_CLEAN_SEG] / 1000);   // (device only, engine_hc.h; a -DASCHED_FASTPROF build adds segment ticks to the same word: read statSeg[34] there)
  out[0] = r.statFastIters; out[1] = r.statGenericIters; out[2] = r.statScanSteps; out[3] = r.statRefills; out[4] = r.statL0Max;
  out[5] = r.statFastReplay; out[6] = r.fastOverflow; out[7] = r.fastActive;
  out[16] = r.statStreamRuns; out[17] = r.statStreamJobs; out[18] = r.statStreamPrepared; out[19] = r.statStreamEmitted;
  for (int i = 0; i < 8; i++) out[8 + i] = (int32_t)(r.statClk[i] / 1000);  // kilo-ticks of the shader clock per phase (6: plane scans, 7: fair-share selects, both inside the passes)
  if (getenv("ASCHED_PRINT_SEG")) { fprintf(stderr, "two-wave iteration: [0] control-wave ticks waiting for the engine, [1] engine busy ticks, [2] engine jobs (kilo-units; profiling builds: per-segment ticks):"); for (int i = 0; i < 40; i++) fprintf(stderr, " %lld", (long long)(r.statSeg[i] / 1000)); fprintf(stderr, "\n"); }
  return 0;
}
// the library's own pre-sorted order (jobs_set: counting sort by queue + packed keys), read back from the device table the round uses
int32_t asched_scheduling_order(asched_t* h, int32_t queue, int32_t* out, int32_t cap) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->jobsSet || queue < 0) return fail(h, ASCHED_ERR_INVALID, "scheduling_order: jobs_set first / bad queue");
  int32_t off[2] = {0, 0};
  if (queue >= h->ordQueues) return 0;
  plat_d2h(off, h->dev.ordAllOff + queue, sizeof off);
  int n = off[1] - off[0];
  if (n > 0 && cap > 0) plat_d2h(out, h->dev.ordAll + off[0], sizeof(int32_t) * (size_t)std::min(n, cap));
  return n;
}
int32_t asched_num_nodes(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); return h->N; }
int32_t asched_total_resources(asched_t* h, int64_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat); for (int r = 0; r < h->R; r++) out[r] = h->dev.cfg.isFloating[r] ? 0 : h->dev.cfg.totalResources[r]; return 0; }
// NodeTypesMatchingJob (nodedb.go:1118-1133): the host keeps the node types (they only exist to prefilter; the device works on masks)
int32_t asched_node_types_matching_job(asched_t* h, int32_t job, int32_t* nMatch, int32_t* nExcluded) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->jobsSet || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "node_types_matching_job: bad job");
  int m = 0, x = 0;
  for (auto& t : h->types) {
    if (t.numNodes == 0) continue;
    if (classMatchesType(h, h->jReqClass[job], t)) m++; else x += t.numNodes;
  }
  *nMatch = m; *nExcluded = x;
  return 0;
}
int32_t asched_set_excluded_nodes(asched_t* h, int32_t maxFailed) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  h->exclCap = maxFailed < 0 ? 0 : maxFailed;
  if (h->nodesSet && h->jobsSet) exclSetup(h);
  return 0;
}
int32_t asched_excluded_nodes(asched_t* h, int32_t job, asched_excluded_reason* out, int32_t cap) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->jobsSet || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "excluded_nodes: bad job");
  if (!h->dev.excl) return 0;
  const ExclDev& x = h->exclHost;
  int32_t slot = -1;
  plat_d2h(&slot, x.jobSlot + job, 4);
  if (slot == EXCL_S_NONE) return 0;
  if (slot == EXCL_S_DROPPED) return fail(h, ASCHED_ERR_UNSUPPORTED, "excluded_nodes: the record was dropped (more failed selections than asched_set_excluded_nodes keeps)");
  if (slot == EXCL_S_UNSUPPORTED) return fail(h, ASCHED_ERR_UNSUPPORTED, "excluded_nodes: not produced for this selection (see asched_excluded_reason)");
  const int N = h->N, R = h->R;
  std::map<ExclKeyH, int64_t> hist;
  const int64_t* req = h->shapeReq.data() + (size_t)h->jShape[job] * R;
  if (slot == EXCL_S_DISALLOWED) { ExclKeyH k; k.kind = ASCHED_EXCL_DISALLOWED_RESOURCE; hist[k] = N; }
  else if (slot == EXCL_S_NO_ATTEMPT) {}
  else if (slot <= EXCL_S_PINNED0 && slot > EXCL_S_PINNED0 - R) {
    int res = EXCL_S_PINNED0 - slot; int64_t avail = 0;
    plat_d2h(&avail, x.pinAvail + job, 8);
    ExclKeyH k; k.kind = ASCHED_EXCL_INSUFFICIENT_RESOURCES; k.a = res; k.required = req[res]; k.available = avail; hist[k] = 1;
  }
  else if (slot < 0 || slot >= x.cap) return fail(h, ASCHED_ERR_INTERNAL, "excluded_nodes: bad record");
  else {
    ExclRec r;
    plat_d2h(&r, x.rec + slot, sizeof r);
    if (r.job != job) return fail(h, ASCHED_ERR_INTERNAL, "excluded_nodes: record does not belong to the job");
    {

      if (r.flags) return fail(h, ASCHED_ERR_UNSUPPORTED, (r.flags & 2) ? "excluded_nodes: inconsistent record" : "excluded_nodes: more dynamic reasons than the arena holds");
      int cls = r.row < h->S ? h->shapeClass[r.row] : h->awayRowClass[r.row - h->S];
      std::vector<HSel> add;   // jctx.AdditionalNodeSelectors: the gang's uniformity label value (gang_scheduler.go:178-228)
      if (r.uni >= 0) for (size_t sl = 0; sl + 1 < h->uniOffHost.size(); sl++) if (r.uni >= h->uniOffHost[sl] && r.uni < h->uniOffHost[sl + 1]) add.push_back({h->labelSlots[sl], h->slotValues[sl][r.uni - h->uniOffHost[sl]]});
      std::vector<uint64_t> bits(x.W);
      plat_d2h(bits.data(), x.bits + (size_t)slot * x.W, (size_t)x.W * 8);
      int32_t cnt[2] = {0, 0};
      plat_d2h(cnt, (const char*)EXCL(h->dev) + offsetof(ExclDev, count), 8);
      int nd = std::min(cnt[1], x.dynCap);
      std::vector<ExclDyn> dyn(nd);
      if (nd) plat_d2h(dyn.data(), x.dyn, (size_t)nd * sizeof(ExclDyn));
      std::unordered_map<int32_t, const ExclDyn*> dynOf;
      for (auto& e : dyn) if (e.slot == slot) dynOf[e.node] = &e;
      // NodeTypesMatchingJob (nodedb.go:1118-1133): every node of a type the job does not match, under the type-level reason
      std::vector<uint8_t> typeOk(h->types.size(), 0);
      for (size_t t = 0; t < h->types.size(); t++) {
        const HType& ty = h->types[t];
        ExclKeyH k;
        if (exclTaint(h, cls, ty.taints, &k) || exclSelectors(add, ty.labels, &ty.unset, &k) || exclSelectors(h->clsSel[cls], ty.labels, &ty.unset, &k)) { if (ty.numNodes > 0) hist[k] += ty.numNodes; }
        else typeOk[t] = 1;
      }
      // the nodes the iterator yielded (:881-928): StaticJobRequirementsMet's reason (nodematching.go:161-190), else the dynamic one the device kept
      auto staticReasonOf = [&](int n, ExclKeyH& k) {   // StaticJobRequirementsMet's reason (nodematching.go:161-190); false = the node passes
        bool st = exclTaint(h, cls, h->nodeTaints[n], &k) || exclSelectors(add, h->nodeLabels[n], nullptr, &k) || exclSelectors(h->clsSel[cls], h->nodeLabels[n], nullptr, &k);
        if (!st && !classMatchesNode(h, cls, n)) { k = ExclKeyH(); k.kind = ASCHED_EXCL_UNMATCHED_AFFINITY; st = true; }   // (taints and selectors hold: the affinity is what is left)
        if (!st) for (int q = 0; q < R && !st; q++) if (req[q] > h->nodeTotal[(size_t)n * R + q]) { k.kind = ASCHED_EXCL_INSUFFICIENT_RESOURCES; k.a = q; k.required = req[q]; k.available = h->nodeTotal[(size_t)n * R + q]; st = true; }
        return st;
      };
      for (int n = 0; n < N; n++) {
        if (!typeOk[h->nodeType[n]] || !((bits[n >> 6] >> (n & 63)) & 1)) continue;
        ExclKeyH k;
        bool st = staticReasonOf(n, k);
        if (!st) {
          auto it = dynOf.find(n);
          if (it == dynOf.end()) return fail(h, ASCHED_ERR_INTERNAL, "excluded_nodes: a yielded node without a reason");
          k.kind = ASCHED_EXCL_INSUFFICIENT_RESOURCES; k.a = it->second->res; k.required = req[it->second->res]; k.available = it->second->avail;
        }
        hist[k] += 1;
      }
      // a gate-passed record (dev.h ExclRec): the nodes the failed fair-preemption walk found room on and gave up for their static requirements are counted once more (nodedb.go:996-1006)
      if (r.gate > 0 && r.fair) {
        std::vector<uint64_t> fb(x.W);
        plat_d2h(fb.data(), x.fbits + (size_t)slot * x.W, (size_t)x.W * 8);
        for (int n = 0; n < N; n++) { if (!((fb[n >> 6] >> (n & 63)) & 1)) continue; ExclKeyH k; if (staticReasonOf(n, k)) hist[k] += 1; }
      }
    }
  }
  int64_t explicitN = 0;
  for (auto& kv : hist) explicitN += kv.second;
  if (N - explicitN > 0) { ExclKeyH k; k.kind = ASCHED_EXCL_IMPLICIT; hist[k] += N - explicitN; }   // nodedb.go:566-580
  int n = 0;
  for (auto& kv : hist) {
    if (kv.second == 0) continue;
    if (n < cap && out) { asched_excluded_reason o; memset(&o, 0, sizeof o); o.kind = kv.first.kind; o.a = kv.first.a; o.b = kv.first.b; o.c = kv.first.c;
                          o.required = kv.first.required; o.available = kv.first.available; o.count = (int32_t)kv.second; out[n] = o; }
    n++;
  }
  return n;
}
int32_t asched_submit_stats(asched_t* h, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  out[0] = h->submitWideUnits; out[1] = h->submitWidePasses; out[2] = h->submitSeqUnits; out[3] = h->submitGangUnits; out[4] = h->submitNodePasses; out[5] = h->submitLitUnits;
  return 0;
}
int32_t asched_kernel_times(asched_t* h, double* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  out[0] = h->roundMs; out[1] = plat_last_fit_ms(); out[2] = h->roundLaunches; out[3] = h->submitMs;
  if (plat_last_opt_ms() > 0 && h->lastWideWasOpt) out[1] = plat_last_opt_ms();
  return 0;
}
int32_t asched_round_counters(asched_t* h, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  plat_d2h(&h->rsHost, h->dev.rs, sizeof(RoundScalars));
  out[0] = h->rsHost.numScheduledJobs; out[1] = h->rsHost.numScheduledGangs; out[2] = h->rsHost.numEvictedJobs; out[3] = h->rsHost.numUnfeasible;
  return 0;
}
// maxSchedulingDuration (scheduling_algo.go:130-134): every following schedule_round / schedule_queues is cancelled `seconds` after it
// starts (0 = no deadline); asched_cancel is the context's cancel function: callable from any thread, it hits the round in flight or,
// between rounds, the next one (a context that is already done: queue_scheduler_test.go "global hard timeout: returns error")
int32_t asched_set_deadline(asched_t* h, double seconds) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!(seconds >= 0)) return fail(h, ASCHED_ERR_INVALID, "set_deadline: negative or NaN");
  plat_set_deadline(seconds);
  return 0;
}
int32_t asched_cancel(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_cancel(h->plat); return 0; }   // no plat_enter: must not touch the caller's current device
int32_t asched_cancel_clear(asched_t* h) { if (!h) return ASCHED_ERR_INVALID; plat_cancel_clear(h->plat); return 0; }

// IndexedNodeLabelValues (nodedb.go:340-343): the values of an indexed node label present on the nodes, ascending interned id
int32_t asched_indexed_node_label_values(asched_t* h, int32_t label_key, int32_t* out, int32_t cap) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->nodesSet) return fail(h, ASCHED_ERR_INVALID, "indexed_node_label_values: nodes_upsert first");
  for (size_t s = 0; s < h->labelSlots.size(); s++) if (h->labelSlots[s] == label_key) {
    int n = (int)h->slotValues[s].size();
    for (int i = 0; i < n && i < cap; i++) out[i] = h->slotValues[s][i];
    return n;
  }
  return -1;  // ok == false: the label is not indexed
}
// GetNode / GetNodeWithTxn (nodedb.go:358-394): the jobs a node holds (AllocatedByJobId keys) with their evicted flag (EvictedJobRunIds) and
// scheduled-at priority; AllocatableByPriority comes from asched_get_alloc.  Returns the number of jobs on the node.
int32_t asched_get_node_jobs(asched_t* h, int32_t node, int32_t* out_jobs, uint8_t* out_evicted, int32_t* out_priority, int32_t cap) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->nodesSet || node < 0 || node >= h->N) return fail(h, ASCHED_ERR_INVALID, "get_node_jobs: bad node");
  if (!h->jobsSet || h->M == 0) return 0;
  std::vector<int32_t> jn(h->M), sp(h->M); std::vector<uint8_t> ev(h->M);
  plat_d2h(jn.data(), h->dev.jobNode, (size_t)h->M * 4); plat_d2h(ev.data(), h->dev.jobEvictedOnNode, (size_t)h->M); plat_d2h(sp.data(), h->dev.schedAtPrio, (size_t)h->M * 4);
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  int n = 0;
  for (int j = 0; j < h->M; j++) if (jn[j] == node) {
    if (n < cap) { if (out_jobs) out_jobs[n] = j; if (out_evicted) out_evicted[n] = ev[j]; if (out_priority) out_priority[n] = sp[j] == NO_PRIORITY ? 0 : sp[j]; }
    n++;
  }
  return n;
}
// GetNodes / GetNodesWithTxn (nodedb.go:396-415): AllocatableByPriority of many nodes in one download; nodes == NULL: all nodes in creation order
int32_t asched_get_nodes_alloc(asched_t* h, int32_t n, const int32_t* nodes, int64_t* out /*[n][P][R]*/) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->nodesSet || n < 0 || (!nodes && n != h->N)) return fail(h, ASCHED_ERR_INVALID, "get_nodes_alloc: nodes_upsert first / bad count");
  for (int i = 0; i < n; i++) if (nodes && (nodes[i] < 0 || nodes[i] >= h->N)) return fail(h, ASCHED_ERR_INVALID, "get_nodes_alloc: bad node");
  size_t Npad = h->dev.cfg.Npad, PR = (size_t)h->P * h->R;
  std::vector<int64_t> planes(PR * Npad);
  plat_d2h(planes.data(), h->dev.alloc, planes.size() * 8);
  if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  for (int i = 0; i < n; i++) { int nd = nodes ? nodes[i] : i; for (size_t k = 0; k < PR; k++) out[(size_t)i * PR + k] = h->dev.cfg.isFloating[k % h->R] ? 0 : planes[k * Npad + nd]; }
  return 0;
}
// Upsert / UpsertWithTxn of ONE node (nodedb.go:1154-1175): the caller hands back a node whose AllocatableByPriority it changed on its own
// copy (the Go code mutates *Node copies and upserts them); the order keys of the node are rebuilt for every priority.  Job bookkeeping
// (who holds what on the node) is not touched: that travels through bind / evict / unbind.
int32_t asched_node_upsert(asched_t* h, int32_t node, const int64_t* alloc_by_prio /*[P][R]*/) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->nodesSet || node < 0 || node >= h->N || !alloc_by_prio) return fail(h, ASCHED_ERR_INVALID, "node_upsert: bad node");
  h->allocPristine = false; h->prepared = false;   // the sorted base of a prepared round no longer describes the node
  if (h->keyCoarse)   // (the coarser divisor rests on every node value being a multiple of it)
    for (int c = 0; c < h->K; c++) for (int l = 0; l < h->P; l++)
      if (alloc_by_prio[(size_t)l * h->R + h->indexedCol[c]] % h->dev.cfg.indexedRes[c]) return fail(h, ASCHED_ERR_UNSUPPORTED, "node_upsert: a value off the handle's key divisor (layoutKeys): upload the node table again (nodes_upsert)");
  std::vector<int32_t> a{node};
  for (int k = 0; k < h->P * h->R; k++) {
    int64_t v = h->dev.cfg.isFloating[k % h->R] ? FLOATING_NODE_CAPACITY : alloc_by_prio[k];
    a.push_back((int32_t)(uint32_t)((uint64_t)v & 0xffffffffu)); a.push_back((int32_t)(uint32_t)((uint64_t)v >> 32));
  }
  setArgs(h, a);
  return runControl(h, CMD_NODE_UPSERT);
}

// FairnessOptimisingGangScheduler.scheduleOnNodes for one job (optimiser/gang_scheduler.go:100-141) over PreemptingNodeScheduler.Schedule of
// every node (k_opt_score); the selection walks the nodes in id order like nodeDb.GetNodes()
int32_t asched_optimiser_schedule_job(asched_t* h, int32_t job, double minPct, const int64_t* maxSize, int64_t nowMs, asched_opt_result* out,
                                      int32_t* preempted, int32_t cap, asched_opt_node_score* perNode) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->prepared) return fail(h, ASCHED_ERR_INVALID, "optimiser_schedule_job: round_prepare first (queue costs and fair shares are the round's)");
  if (job < 0 || job >= h->M || !out) return fail(h, ASCHED_ERR_INVALID, "optimiser_schedule_job: bad job");
  OptArgs a; memset(&a, 0, sizeof a);
  a.job = job; a.nowMs = nowMs; a.hasMaxSize = maxSize != nullptr;
  for (int r = 0; r < h->R && maxSize; r++) a.maxSize[r] = maxSize[r];
  std::vector<OptNodeOut> sc; double jobCost = 0;
  h->lastWideWasOpt = true;
  bool reuse = h->optIndexEpoch == h->stateEpoch;   // no launch that can bind or unbind a job has run since the node -> jobs index in the scratch was built
  if (!perNode) {   // nobody asked for every node's score: selection and the selected node's victims stay on the device (one sequence, one small download)
    int32_t node = -1, npre = 0; double cost = 0, impact = 0; std::vector<int32_t> pre;
    if (plat_take_failure()) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    int rc = plat_opt_select(h->dev, a, minPct, reuse, &node, &npre, &cost, &impact, &pre);
    if (rc < 0) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    if (rc == 0) {
      h->optIndexEpoch = h->stateEpoch;
      out->node = node; out->num_preempted = npre; out->scheduling_cost = cost; out->maximum_queue_impact = impact;
      for (int i = 0; i < npre && i < cap && preempted; i++) preempted[i] = pre[i];
      return 0;
    }
    reuse = true; h->optIndexEpoch = h->stateEpoch;   // a node overflowed the wave kernel: the long way below, with the index just built
  }
  if (plat_take_failure() || plat_opt_score(h->dev, a, sc, &jobCost, -1, nullptr, nullptr, false, reuse)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
  h->optIndexEpoch = h->stateEpoch;
  int N = h->N;
  std::vector<int32_t> byId(N);
  for (int n = 0; n < N; n++) byId[h->nodeIdRank.empty() ? n : h->nodeIdRank[n]] = n;
  int best = -1;
  for (int k = 0; k < N; k++) {
    int n = byId[k];
    const OptNodeOut& r = sc[n];
    if (perNode) { perNode[n].scheduled = r.scheduled > 0; perNode[n].num_preempted = r.npre; perNode[n].scheduling_cost = r.cost; perNode[n].maximum_queue_impact = r.impact; }
    if (r.scheduled < 0) return fail(h, ASCHED_ERR_INTERNAL, "optimiser_schedule_job: a node's candidate list overflowed its HBM scratch");
  }
  for (int k = 0; k < N; k++) {
    int n = byId[k];
    const OptNodeOut& r = sc[n];
    if (r.scheduled <= 0) continue;
    if (r.cost == 0 && r.npre == 0) { best = n; break; }                        // no preemption required: the ideal result, exit early (:112-116)
    double improvement = ((jobCost / r.cost) * 100) - 100;                        // :118-121 (cost 0 with victims: +Inf)
    if (!(improvement > minPct)) continue;
    if (best < 0 || r.cost < sc[best].cost || (r.cost == sc[best].cost && r.impact < sc[best].impact)) best = n;   // nodeCostOrder; equal -> the earlier id
  }
  out->node = best; out->num_preempted = 0; out->scheduling_cost = 0; out->maximum_queue_impact = 0;
  if (best < 0) return 0;
  out->num_preempted = sc[best].npre; out->scheduling_cost = sc[best].cost; out->maximum_queue_impact = sc[best].impact;
  if (sc[best].npre > 0 && preempted && cap > 0) {
    OptNodeOut det; std::vector<int32_t> pre;
    std::vector<OptNodeOut> dummy; double jc2;
    if (plat_opt_score(h->dev, a, dummy, &jc2, best, &det, &pre, true)) return fail(h, ASCHED_ERR_DEVICE, plat_last_error());
    for (int i = 0; i < det.npre && i < cap; i++) preempted[i] = pre[i];
  }
  return 0;
}

int32_t asched_set_optimiser(asched_t* h, const asched_optimiser_config* c) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h) return ASCHED_ERR_INVALID;
  h->opt = asched::OptCfg();
  if (!c || !c->enabled) return 0;
  if (c->max_jobs_per_round < 0) return fail(h, ASCHED_ERR_INVALID, "set_optimiser: negative max_jobs_per_round");
  h->opt.enabled = true; h->opt.minPct = c->min_fairness_improvement_pct; h->opt.maxJobs = c->max_jobs_per_round; h->opt.nowMs = c->now_ms;
  if (c->max_job_size_to_preempt) { h->opt.hasMaxSize = true; for (int r = 0; r < h->R; r++) h->opt.maxSize[r] = c->max_job_size_to_preempt[r]; }
  if (c->min_job_size_to_schedule) { h->opt.hasMinSize = true; for (int r = 0; r < h->R; r++) h->opt.minSize[r] = c->min_job_size_to_schedule[r]; }
  if (c->max_resource_fraction_to_schedule) h->opt.maxFraction.assign(c->max_resource_fraction_to_schedule, c->max_resource_fraction_to_schedule + h->R);
  return 0;
}
int32_t asched_job_key_unfeasible(asched_t* h, int32_t job, int32_t* out) { if (!h) return ASCHED_ERR_INVALID; plat_enter(h->plat);
  if (!h->jobsSet || job < 0 || job >= h->M) return fail(h, ASCHED_ERR_INVALID, "job_key_unfeasible: bad job");
  uint8_t v; plat_d2h(&v, h->dev.unfeasible + h->jShape[job], 1);
  *out = v;
  return 0;
}

}  // extern "C"
