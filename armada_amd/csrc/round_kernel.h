// round_kernel.h — the device side that every round-kernel code object shares (armada_sched.hip k_control, armada_sched_aux.hip k_control_aux,
// armada_sched_wk.hip k_control_wk; workgroup 0's body of the first and the last is round_body.h): the control code (round_run.h and what it includes), the LDS mailbox of the worker waves, the helper workgroups'
// HBM mailbox, the device primitives the control code calls (scans, bulk passes, compaction, fair-share evaluation), the fast path's primitives and
// node engine, the LDS residency of the per-queue arrays and the helper workgroups' loop.  What a code object carries is decided by the feature
// switches its .hip file sets before it includes this header (ASCHED_MARKET_ROUND, ASCHED_TWO_WORD_KEYS, ASCHED_SHARDED_PASSES: dev.h).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#define ASCHED_PREFIX asched_
#include "round_run.h"
#include "round_opt.h"
#include "round_price.h"

// ------------------------------------------------------------------------------------------------ device primitives
#define CTL_THREADS 256
enum { OP_EXIT = 0, OP_SCAN = 1, OP_BULK = 2, OP_COMPACT = 3, OP_FAIR = 4, OP_ENGINE = 5, OP_BULKW = 6, OP_SCANFAIR = 7, OP_HELPERS_EXIT = 9, OP_WIDE = 10 };
struct BulkWArgs { int32_t kind, n; };   // a bulk pass whose bodies touch HBM only: shared with the helper workgroups

struct Mailbox {
  int op, kind, n;
  ScanArgs scan;
  FairArgs fair;
  unsigned long long partial[16];
  const int32_t* order; const uint8_t* flag; int32_t* dst; uint32_t* prefix;
  int waveCount[16];
  int total;
};
__shared__ Mailbox g_mb;
__shared__ Dev g_dev;
#ifdef ASCHED_MARKET_ROUND
__shared__ MktDev g_mk;   // market-driven rounds (round_mkt.h): this launch's market state, a kernel argument of k_control_aux / k_control_wk
__device__ static inline MktDev* mktDev() { return &g_mk; }
#endif

// Helper workgroups.  A round launch carries H extra workgroups (one per CU) that spin on a mailbox in HBM and take a share of
// the two read-only full-width queries of the generic path: the first-fit plane scan (OP_SCAN) and the per-node evaluation of
// fair-share preemption (OP_FAIR).  They read only HBM state (never the control workgroup's LDS); the hand-shake is a
// generation counter (release store by the control wave, relaxed polls + acquire fence by the helpers) and a completion
// counter (release increments, acquire poll) at agent scope, so it is correct across XCDs (separate L2s).
struct HelpSlot { unsigned long long gen, mn, mx, pad; };   // one per helper workgroup: written by that workgroup alone (plain stores, the generation last with release)
#define HELP_MAX 255
struct HelpBox {
  unsigned long long cmd;      // (generation << 8) | op, published with ONE release store: a helper can never pair a new generation with an old op
  unsigned long long pad[3];
  unsigned long long args[28]; // ScanArgs / FairArgs image (OP_SCANFAIR: ScanArgs at word 0, FairArgs at word HELP_ARGS2), read by the helpers with agent-scope loads
  // Results and completion (round 4): helper h folds its workgroup's minimum / maximum into slot[h] and stores the command's generation there LAST (release); the
  // control wave polls the generations one slot per lane and folds the values across its lanes.  No read-modify-write on a shared word: round 3 counted ~180 clocks
  // of serialised atomics per helper on result / result2 / done (23 k of a pass with 127 helpers, profiles/r03z_fair_index_alive_only.txt).
  HelpSlot slot[HELP_MAX];
};
#define HELP_ARGS2 14
static_assert(sizeof(ScanArgs) <= HELP_ARGS2 * 8 && sizeof(FairArgs) <= (28 - HELP_ARGS2) * 8 && sizeof(ScanArgs) % 8 == 0 && sizeof(FairArgs) % 8 == 0, "HelpBox args image");
__shared__ HelpBox* g_box;
__shared__ int g_H;
__shared__ unsigned int g_gen;

#ifdef HELP_TRACE
// Timeline of the fused wide pass (tools/build_variant.sh trace -DHELP_TRACE; never in the product): the control wave stamps the wall clock (s_memrealtime, 100 MHz, one time base for
// the whole chip) when it issues an OP_SCANFAIR; helper workgroups 1, H/2 and H add (their stamp - the issue stamp) at five points, the control workgroup at two.
__device__ unsigned long long g_traceT0[1024];
__device__ unsigned long long g_traceSum[64];   // [cls * 8 + point]: cls 0 control (0 own share done, 1 wait done), 1..3 helpers (0 seen, 1 args + acquire, 2 scan done, 3 fair done, 4 slot written); [56 + cls] counts
#define TRACE_ADD(cls, pt, gen) atomicAdd(&g_traceSum[(cls) * 8 + (pt)], (unsigned long long)(wall_clock64() - g_traceT0[(gen) & 1023]))
#endif
// 64-bit words of an object of another type: through a may_alias type.  (Round 2 read the argument structs through a plain unsigned long long* — undefined
// under strict aliasing: int64_t is `long`, so the compiler was free to treat the freshly written struct as never written; `minsize` on the callers made it do
// so and the helper workgroups received garbage requests: profiles/r03a_minsize_rootcause.txt.  The device code is also built with -fno-strict-aliasing now.)
typedef unsigned long long __attribute__((may_alias)) ull_alias;
template <class A, class B = A> __device__ static inline void helpIssue(int op, const A* args, const B* args2 = nullptr) {  // one lane of the control wave
  HelpBox* b = g_box;
  if (args) {
    const ull_alias* src = (const ull_alias*)args;
    for (int i = 0; i < (int)(sizeof(A) / 8); i++) __hip_atomic_store(&b->args[i], src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (args2) {
    const ull_alias* src = (const ull_alias*)args2;
    for (int i = 0; i < (int)(sizeof(B) / 8); i++) __hip_atomic_store(&b->args[HELP_ARGS2 + i], src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  g_gen++;
  __hip_atomic_store(&b->cmd, ((unsigned long long)g_gen << 8) | (unsigned)op, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ static inline unsigned long long waveMin64Dpp(unsigned long long v);
// Completion of the command issued last: every helper's slot carries its generation.  Whole control wave, uniformly (no lane-divergent spin): lane l watches
// slots l, l + 64, ...  Returns the folded minimum; the folded maximum goes back through *mxOut — both in REGISTERS, wave-uniform (round 3's slot variants handed
// the maximum back through a new __shared__ word written by lane 0 and read by the wave with nothing in between: profiles/r04a_lds_handback_rootcause.txt).
__device__ static inline unsigned long long helpWait(unsigned long long* mxOut = nullptr) {
  HelpBox* b = g_box;
  int lane = threadIdx.x & 63;
  int H = __builtin_amdgcn_readfirstlane(g_H);
  unsigned long long gen = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)g_gen);   // (written by lane 0 in helpIssue; a workgroup barrier lies between)
  unsigned long long mn = ~0ull, mxInv = ~0ull;
  unsigned int spins = 0;
  bool gaveUp = false;
  for (int base = 0; base < H && !gaveUp; base += 64) {
    int i = base + lane;
    bool mine = i < H;
    for (;;) {
      unsigned long long g = mine ? __hip_atomic_load(&b->slot[mine ? i : 0].gen, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) : gen;
      if (__ballot(g != gen) == 0) break;
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 0xffff) == 0 && cancelRequested(g_dev)) {  // the caller gave up (hard timeout): do not wait for a helper that may never answer
        raise(g_dev, ASCHED_ERR_TIMEOUT, 902);
        gaveUp = true;
        break;
      }
      if ((spins & 0xffff) == 0 && g_dev.progress) { g_dev.progress[5] = __popcll(__ballot(g == gen)); g_dev.progress[6] = H; g_dev.progress[7] = (int)gen; g_dev.progress[8] = (int)(b->cmd >> 8); g_dev.progress[9] = (int)(b->cmd & 255); }
    }
    if (mine && !gaveUp) {
      unsigned long long a = __hip_atomic_load(&b->slot[i].mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned long long m = ~__hip_atomic_load(&b->slot[i].mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mn = a < mn ? a : mn; mxInv = m < mxInv ? m : mxInv;
    }
  }
  mn = waveMin64Dpp(mn);
  if (mxOut) *mxOut = ~waveMin64Dpp(mxInv);   // max(x) = ~min(~x)
  return mn;
}

__device__ static inline void atomicAddI64(int64_t* p, int64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
__device__ static inline void atomicAddI32(int32_t* p, int32_t v) { atomicAdd(p, v); }
__device__ static inline void atomicOrI32(int32_t* p, int32_t v) { atomicOr(p, v); }
__device__ static inline void atomicMinU32(uint32_t* p, uint32_t v) { atomicMin(p, v); }
__device__ static inline int atomicFetchAddI32(int32_t* p, int32_t v) { return atomicAdd(p, v); }
__device__ static inline int waveMax32(int v) {
  for (int off = 32; off; off >>= 1) { int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  return v;
}

__device__ static inline unsigned long long waveMin64(unsigned long long v) {
  for (int off = 32; off; off >>= 1) {
    unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// ---- cross-lane moves on the VALU (DPP) instead of through the LDS crossbar.  __shfl_* compile to ds_bpermute_b32: an LDS round trip (>100 clocks)
// per 32-bit word, which a lone wave cannot hide; a DPP move is one VALU instruction.  gfx9-family controls: row_shr:n = 0x110+n, wave_shl:1 = 0x130,
// row_half_mirror = 0x141, row_bcast:15 = 0x142, row_bcast:31 = 0x143, quad_perm = 0x00..0xff.
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf> __device__ static inline unsigned long long dppMove64(unsigned long long old, unsigned long long v) {
  unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)old, (int)(unsigned)v, CTRL, ROW_MASK, BANK_MASK, false);
  unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(old >> 32), (int)(unsigned)(v >> 32), CTRL, ROW_MASK, BANK_MASK, false);
  return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf> __device__ static inline int dppMove32(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, BANK_MASK, false);
}
// minimum over the 64 lanes, returned wave-uniform.  min is idempotent: a lane without a valid source keeps its own value (old = v).
__device__ static inline unsigned long long waveMin64Dpp(unsigned long long v) {
  unsigned long long t;
  t = dppMove64<0x111>(v, v); v = t < v ? t : v;              // row_shr:1
  t = dppMove64<0x112>(v, v); v = t < v ? t : v;              // row_shr:2
  t = dppMove64<0x114>(v, v); v = t < v ? t : v;              // row_shr:4
  t = dppMove64<0x118>(v, v); v = t < v ? t : v;              // row_shr:8  -> lane 15 of every row of 16 holds the row's minimum
  t = dppMove64<0x142, 0xa>(v, v); v = t < v ? t : v;         // row_bcast:15 into rows 1 and 3
  t = dppMove64<0x143, 0xc>(v, v); v = t < v ? t : v;         // row_bcast:31 into rows 2 and 3 -> lane 63 holds the minimum
  unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// one thread per node (block-stride): reject by mask bit and key first, touch the alloc planes only for improving candidates
__device__ static unsigned long long scanPart(const Dev& d, const ScanArgs& a, int tid, int nthreads) {
  const DevCfg& c = d.cfg;
  unsigned long long best = ~0ull;
  if (a.levelHi > a.level) {  // multi-level mode: per node the lowest level in [level, levelHi] it fits at, tagged key
    for (int n = SHARD_LO(c) + tid; n < SHARD_HI(c); n += nthreads) {
      uint64_t w = a.maskA[n >> 6];
      if (a.maskB) w &= a.maskB[n >> 6];
      if (!((w >> (n & 63)) & 1)) continue;
      for (int l = a.level; l <= a.levelHi; l++) {
        unsigned long long v = ((unsigned long long)l << SCAN_LEVEL_SHIFT) | d.keys[(size_t)l * c.Npad + n];
        if (v >= best) break;   // higher levels only order later
        const int64_t* plane = d.alloc + (size_t)l * c.R * c.Npad;
        bool fits = true;
        for (int r = 0; r < c.R; r++) fits = fits && (a.req[r] <= plane[(size_t)r * c.Npad + n]);
        if (fits) { best = v; break; }
      }
    }
    return waveMin64(best);
  }
  const uint64_t* keys = d.keys + (size_t)a.level * c.Npad;
  const int64_t* plane = d.alloc + (size_t)a.level * c.R * c.Npad;
#ifdef ASCHED_TWO_WORD_KEYS
  if (WIDE_KEYS(c)) {   // two-word keys (dev.h keyWords): pass 1 (a.pad == 0) the minimum HIGH word among the fitting nodes, pass 2 (a.pad == 1, a.lowBound = that word) the minimum LOW word among those that carry it
    const uint64_t* lows = d.keys + ((size_t)c.P + a.level) * c.Npad;
    for (int n = SHARD_LO(c) + tid; n < SHARD_HI(c); n += nthreads) {
      uint64_t w = a.maskA[n >> 6];
      if (a.maskB) w &= a.maskB[n >> 6];
      if (!((w >> (n & 63)) & 1)) continue;
      unsigned long long k = keys[n];
      if (a.pad) { if (k != a.lowBound) continue; k = lows[n]; if (k < a.lowBoundLo) continue; }
      else if (k < a.lowBound || (k == a.lowBound && a.lowBoundLo && lows[n] < a.lowBoundLo)) continue;
      if (k >= best) continue;
      bool fits = true;
      if (!a.noFit) for (int r = 0; r < c.R; r++) fits = fits && (a.req[r] <= plane[(size_t)r * c.Npad + n]);
      if (fits) best = k;
    }
    return waveMin64(best);
  }
#endif
  for (int n = SHARD_LO(c) + tid; n < SHARD_HI(c); n += nthreads) {
    uint64_t w = a.maskA[n >> 6];
    if (a.maskB) w &= a.maskB[n >> 6];
    if (!((w >> (n & 63)) & 1)) continue;
    unsigned long long k = keys[n];
    if (k >= best || k < a.lowBound) continue;
    bool fits = true;
    if (!a.noFit) for (int r = 0; r < c.R; r++) fits = fits && (a.req[r] <= plane[(size_t)r * c.Npad + n]);
    if (fits) best = k;
  }
  return waveMin64(best);
}

#ifdef ASCHED_SHARDED_PASSES
// A sharded wide pass (dev.h shardWorld): the minimum of the word and the maximum of the index over the replicas' shares.  The control wave posts its two words (the
// index as its complement: one MIN all-reduce serves both) in the handle's host-mapped block and waits for the answer of the host thread that drives the launch
// (plat_run_control: the all-reduce runs on the handle's communicator).  A PCIe round trip + the collective per pass: worth it where a pass is long (100 000 nodes and
// up) — measured numbers for one GPU only.  Bounded like every wait of this kernel: the caller's cancel word ends it.
__shared__ unsigned int g_xgen;
__shared__ unsigned long long g_xpeers;   // 0: the exchange goes through the host proxy; else the device address of the peer table (asched_shard_peers): GPU-to-GPU
// The same exchange GPU-to-GPU (asched_shard_peers): every replica owns an exchange area in its HBM (fine-grained; the peers map it: peer access inside a process, hipIpc across
// processes) — word 0 the owner's generation counter (it outlives a launch), from word 8 two banks (generation parity) of one 4-word slot per rank: {generation, word 0, word 1, -}.
// Lane r of the control wave stores this rank's two words and then the generation (release, system scope) into ITS slot of rank r's area — over xGMI for a remote r —, then
// watches slot r of the own area; when every rank's generation is there the words are folded across the lanes.  No host, no PCIe: an exchange is a round of posted stores
// and one polling read of local HBM.  A rank can run at most one exchange ahead of another (it needs the other's words to finish its own), hence two banks.
__device__ static inline void shardReduceDirect(Dev& d, unsigned long long* mn, int* mxIdx) {
  unsigned long long* const* peers = (unsigned long long* const*)g_xpeers;
  const int lane = threadIdx.x & 63, W = d.cfg.shardWorld, me = d.cfg.shardRank;
  unsigned int gen = (unsigned int)__builtin_amdgcn_readfirstlane((int)g_xgen) + 1;
  const size_t bank = (size_t)(gen & 1) * 256;
  unsigned long long w0 = *mn, w1 = ~(unsigned long long)(unsigned int)(*mxIdx + 1);
  unsigned long long* own = peers[me];
  if (lane == 0) { g_xgen = gen; __hip_atomic_store(own, (unsigned long long)gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
  if (lane < W) {
    unsigned long long* slot = peers[lane] + 8 + (bank + me) * 4;
    __hip_atomic_store(slot + 1, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot + 2, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot, (unsigned long long)gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  unsigned long long* mine = own + 8 + (bank + (lane < W ? lane : 0)) * 4;
  unsigned int spins = 0;
  for (;;) {
    bool there = lane >= W || __hip_atomic_load(mine, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == gen;
    if (__ballot(!there) == 0) break;
    __builtin_amdgcn_s_sleep(1);
    if ((++spins & 0xfff) == 0 && cancelRequested(d)) { raise(d, ASCHED_ERR_TIMEOUT, 904); return; }
  }
  unsigned long long v0 = lane < W ? __hip_atomic_load(mine + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : ~0ull;
  unsigned long long v1 = lane < W ? __hip_atomic_load(mine + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : ~0ull;
  v0 = waveMin64Dpp(v0); v1 = waveMin64Dpp(v1);
  *mn = v0; *mxIdx = (int)(unsigned int)~v1 - 1;
}
__device__ static inline void shardReduce(Dev& d, unsigned long long* mn, int* mxIdx) {
  if (__builtin_amdgcn_readfirstlane((int)(g_xpeers != 0))) { shardReduceDirect(d, mn, mxIdx); return; }
  unsigned long long* X = (unsigned long long*)d.cancel;
  if (!X) { raise(d, ASCHED_ERR_INTERNAL, 530); return; }
  int lane = threadIdx.x & 63;
  unsigned int gen = (unsigned int)__builtin_amdgcn_readfirstlane((int)g_xgen) + 1;
  unsigned long long w0 = *mn, w1 = ~(unsigned long long)(unsigned int)(*mxIdx + 1);
  if (lane == 0) {
    g_xgen = gen;
    __hip_atomic_store(&X[XCHG_WORD0 + 1], w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&X[XCHG_WORD0 + 2], w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&X[XCHG_WORD0], (unsigned long long)gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  unsigned int spins = 0;
  for (;;) {
    unsigned long long g = __hip_atomic_load(&X[XCHG_WORD0 + 3], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (g == gen) break;
    __builtin_amdgcn_s_sleep(4);
    if ((++spins & 0x3ff) == 0 && cancelRequested(d)) { raise(d, ASCHED_ERR_TIMEOUT, 903); return; }
  }
  w0 = __hip_atomic_load(&X[XCHG_WORD0 + 4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  w1 = __hip_atomic_load(&X[XCHG_WORD0 + 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  *mn = w0; *mxIdx = (int)(unsigned int)~w1 - 1;
}
#define SHARD_REDUCE(d, mn, idx) do { if (SHARD_ON((d).cfg)) shardReduce(d, &(mn), &(idx)); } while (0)
#define SHARD_REDUCE_MIN(d, mn) do { if (SHARD_ON((d).cfg)) { int none_ = -1; shardReduce(d, &(mn), &none_); } } while (0)
#define SHARD_REDUCE_MAX(d, idx) do { if (SHARD_ON((d).cfg)) { unsigned long long none_ = ~0ull; shardReduce(d, &none_, &(idx)); } } while (0)
#else
#define SHARD_REDUCE(d, mn, idx) do {} while (0)
#define SHARD_REDUCE_MIN(d, mn) do {} while (0)
#define SHARD_REDUCE_MAX(d, idx) do {} while (0)
#endif
#ifdef ASCHED_TWO_WORD_KEYS
__device__ static inline uint64_t wgFirstFitKeyPass(Dev& d, const ScanArgs& a) {
#else
__device__ static inline uint64_t wgFirstFitKey(Dev& d, const ScanArgs& a) {
#endif
  int lane = threadIdx.x & 63;
  if (lane == 0) { g_mb.op = OP_SCAN; g_mb.scan = a; if (g_H) helpIssue(OP_SCAN, &a); }
  __syncthreads();
  unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, (g_H + 1) * (int)blockDim.x);
  if (lane == 0) g_mb.partial[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long best = ~0ull;
  int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; w++) { unsigned long long p = g_mb.partial[w]; best = p < best ? p : best; }
  if (g_H) {
    unsigned long long hb = helpWait();
    best = hb < best ? hb : best;
  }
  SHARD_REDUCE_MIN(d, best);
  d.rs->numScans++;
  return best;
}
#ifdef ASCHED_TWO_WORD_KEYS
// -> the minimum order key among the fitting nodes, ~0 = none.  Two-word keys: the LOW word of the minimum (it carries the node-index rank the callers look at), found in two
// passes — the order is (high word, low word), so the second pass only looks at the nodes that carry the first pass's high word.
__device__ static inline uint64_t wgFirstFitKey(Dev& d, const ScanArgs& a) {
  uint64_t best = wgFirstFitKeyPass(d, a);
  if (WIDE_KEYS(d.cfg)) {
    if (a.levelHi > a.level) { raise(d, ASCHED_ERR_UNSUPPORTED, 520); return ~0ull; }   // (the fused multi-level pass is one-word only: the host never selects it)
    if (best == ~0ull) return best;
    ScanArgs b = a; b.pad = 1; b.lowBound = best; b.lowBoundLo = best == a.lowBound ? a.lowBoundLo : 0;
    best = wgFirstFitKeyPass(d, b);
  }
  return best;
}
#endif
__device__ static inline int wgFirstFit(Dev& d, const ScanArgs& a) {
  unsigned long long best = wgFirstFitKey(d, a);
  if (best == ~0ull) return -1;
  return d.nodeByRank[best & ((1ull << d.cfg.idxBits) - 1)];
}

// one thread per node (grid-stride over the participating workgroups): highest evicted-table Index at which a node covers the request
__device__ static int fairPart(const Dev& d, const FairArgs& a, int tid, int nthreads) {
  int best = -1;
  for (int n = SHARD_LO(d.cfg) + tid; n < SHARD_HI(d.cfg); n += nthreads) { int v = fairNodeBest(d, a, n, best); best = v > best ? v : best; }
  return waveMax32(best);
}
__device__ static inline int wgFairSelect(Dev& d, const FairArgs& a) {
  int lane = threadIdx.x & 63;
  if (lane == 0) { g_mb.op = OP_FAIR; g_mb.fair = a; if (g_H) helpIssue(OP_FAIR, &a); }
  __syncthreads();
  int v = fairPart(d, g_mb.fair, threadIdx.x, (g_H + 1) * (int)blockDim.x);
  if (lane == 0) g_mb.waveCount[threadIdx.x >> 6] = v;
  __syncthreads();
  int best = -1;
  int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; w++) { int p = g_mb.waveCount[w]; best = p > best ? p : best; }
  if (g_H) {
    unsigned long long hmx;
    (void)helpWait(&hmx);
    int h = (int)(unsigned int)hmx - 1;
    best = h > best ? h : best;
  }
  SHARD_REDUCE_MAX(d, best);
  return best;
}

// gate + fair-share evaluation in one pass (selectAtPriority, round_ctl.h): every participating thread walks its nodes once for each question; one
// command, one completion count, two results
__device__ static inline int wgScanFair(Dev& d, const ScanArgs& a, const FairArgs& f, uint64_t* bestKey) {
  int lane = threadIdx.x & 63;
#ifdef HELP_TRACE
  if (lane == 0 && g_H) { g_traceT0[(g_gen + 1) & 1023] = wall_clock64(); __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); }
#endif
  if (lane == 0) { g_mb.op = OP_SCANFAIR; g_mb.scan = a; g_mb.fair = f; if (g_H) helpIssue(OP_SCANFAIR, &a, &f); }
  __syncthreads();
  unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, (g_H + 1) * (int)blockDim.x);
  int w = fairPart(d, g_mb.fair, threadIdx.x, (g_H + 1) * (int)blockDim.x);
  if (lane == 0) { g_mb.partial[threadIdx.x >> 6] = v; g_mb.waveCount[threadIdx.x >> 6] = w; }
  __syncthreads();
#ifdef HELP_TRACE
  if (lane == 0 && g_H) { TRACE_ADD(0, 0, g_gen); atomicAdd(&g_traceSum[56], 1ull); }
#endif
  unsigned long long best = ~0ull; int idx = -1;
  int nw = blockDim.x >> 6;
  for (int k = 0; k < nw; k++) { unsigned long long p = g_mb.partial[k]; best = p < best ? p : best; int q = g_mb.waveCount[k]; idx = q > idx ? q : idx; }
  if (g_H) {
    unsigned long long hmx;
    unsigned long long hb = helpWait(&hmx);
#ifdef HELP_TRACE
    if (lane == 0) TRACE_ADD(0, 1, g_gen);
#endif
    best = hb < best ? hb : best;
    int h = (int)(unsigned int)hmx - 1;
    idx = h > idx ? h : idx;
  }
  SHARD_REDUCE(d, best, idx);
  d.rs->numScans++;
  *bestKey = best;
  return idx;
}

// A bulk pass over n elements on the control workgroup AND the helper workgroups (grid-stride over all of them).  Only for bodies that read and write HBM and
// nothing the control workgroup keeps in LDS (the stream preparation, round_run.h B_QS*): the helpers see the kernel argument's Dev, i.e. the HBM homes.
__device__ static inline void wgBulkWide(Dev& d, int kind, int n) {
  int lane = threadIdx.x & 63;
  if (lane == 0) { g_mb.op = OP_BULKW; g_mb.kind = kind; g_mb.n = n; if (g_H) { BulkWArgs a; a.kind = kind; a.n = n; __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); helpIssue(OP_BULKW, &a); } }
  __syncthreads();
  { int nthreads = (g_H + 1) * (int)blockDim.x; int kd = g_mb.kind, nn = g_mb.n; for (int i = threadIdx.x; i < nn; i += nthreads) bulkElem(d, kd, i); }
  __threadfence();
  __syncthreads();
  if (g_H) { (void)helpWait(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
}

// one pass of a wide run's preparation / commit (round_wide.h): like wgBulkWide, with its own op and an out-of-line body — a call inside bulkElem's switch moves the
// hot loops of the headline round
__device__ static inline void wgWide(Dev& d, int kind, int n) {
  int lane = threadIdx.x & 63;
  if (lane == 0) { g_mb.op = OP_WIDE; g_mb.kind = kind; g_mb.n = n; if (g_H) { BulkWArgs a; a.kind = kind; a.n = n; __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); helpIssue(OP_WIDE, &a); } }
  __syncthreads();
  { int nthreads = (g_H + 1) * (int)blockDim.x; int kd = g_mb.kind, nn = g_mb.n; for (int i = threadIdx.x; i < nn; i += nthreads) wideBulkAny(d, kd, i); }
  __threadfence();
  __syncthreads();
  if (g_H) { (void)helpWait(); }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// Most elements of the per-job passes do nothing (queued jobs have no node, few jobs are flagged for eviction): read the one
// field that decides that for BULK_U elements at once — independent loads, all in flight together — and run the body only for
// the survivors.  The bodies themselves are unchanged (round_run.h bulkElem).
#define BULK_U 8
__device__ static inline int bulkGate(Dev& d, int kind, int i) {
  switch (kind) {
    case B_EVICT_APPLY1: case B_EVICT_APPLY3: return d.evFlag[i];
    case B_UNBIND: return d.inPreempted[i] | d.inSchedAndEvicted[i];
    case B_FILTER1: case B_FILTER3: return d.jobNode[i] >= 0;
  }
  return 1;
}
__device__ static void bulkPart(Dev& d, int kind, int n) {
  int stride = blockDim.x;
  if (kind == B_EVICT_APPLY1 || kind == B_EVICT_APPLY3 || kind == B_UNBIND || kind == B_FILTER1 || kind == B_FILTER3) {
    bool filter = kind == B_FILTER1 || kind == B_FILTER3;
    for (int base = threadIdx.x; base < n; base += stride * BULK_U) {
      int gate[BULK_U];
#pragma unroll
      for (int u = 0; u < BULK_U; u++) { int i = base + u * stride; gate[u] = i < n ? bulkGate(d, kind, i) : -1; }
#pragma unroll
      for (int u = 0; u < BULK_U; u++) {
        int i = base + u * stride;
        if (gate[u] > 0) bulkElem(d, kind, i);
        else if (gate[u] == 0 && filter) d.evFlag[i] = 0;  // a job without a node is never evicted (pqs.go:101-136, eviction.go:158-178)
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += stride) bulkElem(d, kind, i);
  }
  __threadfence();  // int64 atomics land in L2: make them (and the plain stores) visible to the control wave
}
__device__ static inline void wgBulk(Dev& d, int kind, int n) {
  if (n <= 0) return;
  if ((threadIdx.x & 63) == 0) { g_mb.op = OP_BULK; g_mb.kind = kind; g_mb.n = n; }
  __syncthreads();
  bulkPart(d, g_mb.kind, g_mb.n);
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// order-preserving compaction of {order[p] : flag[order[p]]} (order == NULL: identity); prefix[p] = #flagged before p
__device__ static int compactPart(Dev& d) {
  (void)d;
  int n = g_mb.n;
  const int32_t* order = g_mb.order; const uint8_t* flag = g_mb.flag; int32_t* dst = g_mb.dst; uint32_t* prefix = g_mb.prefix;
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int base = 0;
  const int U = 4;  // element / flag loads of U consecutive tiles are issued together; the ordered prefix then runs tile by tile
  for (int start0 = 0; start0 < n; start0 += blockDim.x * U) {
    int vv[U]; bool ff[U];
#pragma unroll
    for (int u = 0; u < U; u++) { int p = start0 + u * (int)blockDim.x + (int)threadIdx.x; vv[u] = p < n ? (order ? order[p] : p) : 0; }
#pragma unroll
    for (int u = 0; u < U; u++) { int p = start0 + u * (int)blockDim.x + (int)threadIdx.x; ff[u] = p < n && flag[vv[u]]; }
#pragma unroll
    for (int u = 0; u < U; u++) {
      int start = start0 + u * (int)blockDim.x;
      if (start >= n) break;
      int p = start + threadIdx.x;
      int v = vv[u];
      bool f = ff[u];
      unsigned long long b = __ballot(f);
      int rank = __popcll(b & ((1ull << lane) - 1));
      if (lane == 0) g_mb.waveCount[wave] = __popcll(b);
      __syncthreads();
      int off = 0, tot = 0;
      for (int w = 0; w < nw; w++) { int cw = g_mb.waveCount[w]; if (w < wave) off += cw; tot += cw; }
      if (p < n && prefix) prefix[p] = base + off + rank;
      if (f) dst[base + off + rank] = v;
      base += tot;
      __syncthreads();
    }
  }
  __threadfence();
  return base;
}
__device__ static inline int wgCompactRun(Dev& d, const int32_t* order, int n, const uint8_t* flag, int32_t* dst, uint32_t* prefix) {
  if ((threadIdx.x & 63) == 0) { g_mb.op = OP_COMPACT; g_mb.n = n; g_mb.order = order; g_mb.flag = flag; g_mb.dst = dst; g_mb.prefix = prefix; }
  __syncthreads();
  int total = compactPart(d);
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return total;
}
__device__ static inline int wgCompactFlagged(Dev& d, const int32_t* order, const int32_t* segOff, int nseg, int n, const uint8_t* flag, int32_t* dst, int32_t* outSegOff) {
  int total = wgCompactRun(d, order, n, flag, dst, d.evSortKey);
  for (int base = 0; base <= nseg; base += 64) {  // same trip count on every lane
    int q = base + (int)(threadIdx.x & 63);
    if (q <= nseg) outSegOff[q] = segOff[q] < n ? (int32_t)d.evSortKey[segOff[q]] : total;
  }
  __threadfence();
  return total;
}
__device__ static inline int wgCompactIota(Dev& d, int n, const uint8_t* flag, int32_t* dst) { return wgCompactRun(d, nullptr, n, flag, dst, nullptr); }

// lane-per-queue argmin under the reference's Less (a strict total order, so argmin == heap top).  Every lane reads its queue's Less inputs once; the
// tournament moves the VALUES between lanes (no memory access per round)
struct PqVal { int q; int32_t prio; double proposed, budget, current, size; int32_t name; int32_t away; };
__device__ static inline bool pqLessV(const Ctl& c, const PqVal& a, const PqVal& b) {   // pqLess (round_ctl.h) on values
  if (a.away != b.away) return !a.away;   // (0 everywhere unless preemptCrossPoolJobsFirst is set and cross-pool away jobs exist)
  if (a.prio != b.prio) return a.prio > b.prio;
  if (c.preferLarge) {
    if (a.proposed <= a.budget && b.proposed <= b.budget) {
      if (a.current == b.current && a.size != b.size) return a.size > b.size;
      if (a.current != b.current) return a.current < b.current;
    } else if (a.proposed > a.budget && b.proposed > b.budget) {
      if (a.proposed != b.proposed) return a.proposed < b.proposed;
    } else if (a.proposed <= a.budget) return true;
    else if (b.proposed <= b.budget) return false;
  } else {
    if (a.proposed != b.proposed) return a.proposed < b.proposed;
  }
  return a.name < b.name;
}
__device__ static inline double shflD(double v, int off) { return __shfl_xor(v, off, 64); }
__device__ static inline int pqTop(Dev& d, const Ctl& c) {
  int lane = threadIdx.x & 63;
  PqVal best; best.q = -1; best.prio = 0; best.proposed = best.budget = best.current = best.size = 0; best.name = 0; best.away = 0;
  int Q = d.cfg.Q;
  const bool homeFirst = d.cfg.preferHome && d.jAway;
  for (int base = 0; base < Q; base += 64) {  // same trip count on every lane: the wave stays converged for the shuffles below
    int q = base + lane;
    bool in = q < Q && d.pqInHeap[q < Q ? q : 0];
    if (in) {
      PqVal v; v.q = q; v.prio = c.compareSchedPrio ? d.pqSchedPrio[q] : d.pqPcPrio[q]; v.proposed = d.pqProposed[q]; v.budget = d.pqBudget[q]; v.current = d.pqCurrent[q]; v.size = d.pqSize[q]; v.name = d.qNameRank[q];
      v.away = homeFirst ? (pqAway(d, q) ? 1 : 0) : 0;
      if (best.q < 0 || pqLessV(c, v, best)) best = v;
    }
  }
  for (int off = 32; off; off >>= 1) {
    PqVal o; o.q = __shfl_xor(best.q, off, 64); o.prio = __shfl_xor(best.prio, off, 64); o.proposed = shflD(best.proposed, off); o.budget = shflD(best.budget, off);
    o.current = shflD(best.current, off); o.size = shflD(best.size, off); o.name = __shfl_xor(best.name, off, 64); o.away = __shfl_xor(best.away, off, 64);
    if (o.q >= 0 && (best.q < 0 || pqLessV(c, o, best))) best = o;
  }
  return best.q;
}


// ------------------------------------------------------------------------------------------------ fast-path primitives (round_fast.h contracts)
// All of these run on wave 0 only (the control wave); results are wave-uniform.  LDS state is reached through the
// __shared__ objects themselves (ds_* instructions), HBM through explicit global-address-space pointers (FastK): no flat
// accesses, so LDS work never waits for the outstanding HBM stores/atomics and vice versa.
__device__ static inline bool keyLess(uint32_t A, unsigned long long X, unsigned long long Y, uint32_t N, uint32_t oA, unsigned long long oX, unsigned long long oY, uint32_t oN) {
  return A != oA ? A < oA : X != oX ? X < oX : Y != oY ? Y < oY : N < oN;
}
// sort the queues in the heap by key across the lanes (rank by counting; Q <= 64, done once per fastRun)
__device__ static inline void pqBuild(PQState& s, int Q) {
  int lane = threadIdx.x & 63;
  bool in = lane < Q && g_fl.inHeap[lane];
  uint32_t A = in ? g_fl.kA[lane] : ~0u, N = lane < Q ? (uint32_t)g_fl.nameRank[lane] : ~0u;
  unsigned long long X = in ? g_fl.kX[lane] : ~0ull, Y = in ? g_fl.kY[lane] : ~0ull;
  int rank = 0;
  for (int j = 0; j < 64; j++) {
    uint32_t jA = __shfl(A, j, 64), jN = __shfl(N, j, 64); unsigned long long jX = __shfl(X, j, 64), jY = __shfl(Y, j, 64);
    int jin = __shfl((int)in, j, 64);
    bool before = jin && !in ? true : (!jin && in ? false : (keyLess(jA, jX, jY, jN, A, X, Y, N) || (jA == A && jX == X && jY == Y && jN == N && j < lane)));
    if (j != lane && before) rank++;
  }
  // scatter by rank through LDS, gather in lane order
  g_fl.tmpA[rank] = A; g_fl.tmpN[rank] = N; g_fl.tmpX[rank] = X; g_fl.tmpY[rank] = Y; g_fl.tmpQ[rank] = in ? lane : -1;
  s.A = g_fl.tmpA[lane]; s.N = g_fl.tmpN[lane]; s.X = g_fl.tmpX[lane]; s.Y = g_fl.tmpY[lane]; s.q = g_fl.tmpQ[lane];
  s.count = __popcll(__ballot(in));
}
__device__ static inline int pqHead(PQState& s, int Q) {
  int q = __builtin_amdgcn_readfirstlane(s.q);
  return (s.count > 0 && q >= 0 && q < Q) ? q : -1;
}
// the head (queue q) was served: drop it and, if it still has a candidate gang, insert it again under its new key
__device__ static inline void pqPopPush(PQState& s, const KeyOut& ko, int q) {
  int lane = threadIdx.x & 63;
  uint32_t hN = __builtin_amdgcn_readfirstlane(s.N);  // the name rank travels with the entry
  // everything after the head moves up one lane
  // wave_shl:1 — lane i takes lane i+1's value; lane 63 has no source and is overwritten below (lane >= cnt)
  uint32_t dA = (uint32_t)dppMove32<0x130>((int)s.A, (int)s.A), dN = (uint32_t)dppMove32<0x130>((int)s.N, (int)s.N);
  unsigned long long dX = dppMove64<0x130>(s.X, s.X), dY = dppMove64<0x130>(s.Y, s.Y);
  int dq = dppMove32<0x130>(s.q, s.q);
  int cnt = s.count - 1;  // entries other than the head
  if (lane >= cnt) { dA = ~0u; dN = ~0u; dX = ~0ull; dY = ~0ull; dq = -1; }
  if (!ko.valid) { s.A = dA; s.N = dN; s.X = dX; s.Y = dY; s.q = dq; s.count = cnt; return; }
  // position of the new key among the others = number of them that order before it
  bool before = lane < cnt && keyLess(dA, dX, dY, dN, ko.A, ko.X, ko.Y, hN);
  int pos = __popcll(__ballot(before));
  // lanes < pos take the shifted entry, lane pos the new key, lanes > pos keep their own (shift up and down cancel)
  if (lane < pos) { s.A = dA; s.N = dN; s.X = dX; s.Y = dY; s.q = dq; }
  else if (lane == pos) { s.A = ko.A; s.N = hN; s.X = ko.X; s.Y = ko.Y; s.q = q; }
  s.count = cnt + 1;
}

// fairness.go:99-105 three times (alloc+req, alloc, req): lane (8*which + r) evaluates one float64 ratio, the max over a
// group of 8 lanes is the dominant share; identical IEEE operations to drf() in round_ctl.h, evaluated side by side.
// Operands come straight from LDS (the queue's resource vectors and the window record), one lane-indexed read each.
__device__ static inline void drf3(Dev& d, int q, int k, bool replay, double w, double* proposed, double* current, double* size) {
  int lane = threadIdx.x & 63;
  int which = lane >> 3, r = lane & 7;
  double x = -INFINITY;
  if (which < 3 && r < d.cfg.R) {
    int64_t a = (replay ? g_fl.qReplay[q][r] : g_fl.qAlloc[q][r]) + g_fl.qPenalty[q][r];
    int64_t rq = g_fl.winRec[q][k].req[r];
    int64_t v = which == 0 ? a + rq : which == 1 ? a : rq;
    int64_t t = d.cfg.totalResources[r];
    double f = 0.0;
    if (t != 0) f = (double)v / (double)t;
    x = f * d.cfg.drfMult[r];
  }
  {  // max over each group of 8 lanes, on every lane of the group (max is idempotent): lane^1, lane^2 inside the quad, then the mirrored quad
    unsigned long long b = __builtin_bit_cast(unsigned long long, x), t; double o;
    t = dppMove64<0xB1>(b, b); o = __builtin_bit_cast(double, t); x = o > x ? o : x; b = __builtin_bit_cast(unsigned long long, x);   // quad_perm [1,0,3,2]
    t = dppMove64<0x4E>(b, b); o = __builtin_bit_cast(double, t); x = o > x ? o : x; b = __builtin_bit_cast(unsigned long long, x);   // quad_perm [2,3,0,1]
    t = dppMove64<0x141>(b, b); o = __builtin_bit_cast(double, t); x = o > x ? o : x;                                                 // row_half_mirror: lane i <-> 7-i of its half row
  }
  double m = x > 0 ? x : 0.0;
  double res = which == 2 ? m * w : m / w;
  {  // lanes 0, 8, 16 hold the three results: scalar reads
    unsigned long long rb = __builtin_bit_cast(unsigned long long, res);
    auto rl = [&](int l) { unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)rb, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(rb >> 32), l); return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo); };
    *proposed = rl(0); *current = rl(8); *size = rl(16);
  }
}

__device__ static inline void fastFence(Ctl& c) {
  if (c.l1Dirty) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); c.l1Dirty = 0; }  // vmcnt(0) + L1 invalidate: the no-return atomics are now what plain loads see
}

__device__ static inline void baseTileRemoved(KREF, FastS&, int) {}   // (the tile walk of ASCHED_FIT_BITS=0 keeps nothing between scans)
// base entry pos is stale from now on: its flag, and its bit in every fit shape's "clean and fits" bitmap (lane f clears row f; no-return atomics at L2 —
// the scans read the bitmaps with agent-scope loads, so every wave sees them)
__device__ static inline void baseMarkRemoved(KREF k, FastS& S, int pos) {
  (void)S;
  int lane = threadIdx.x & 63;
  if (lane == 0) k.baseRemoved[pos] = 1;
  if (k.fitBits) {
    unsigned long long bit = 1ull << (pos & 63);
    for (int f = lane; f < k.S; f += 64) (void)__hip_atomic_fetch_and(&k.fitBits[(size_t)f * k.fitW + (pos >> 6)], ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__device__ static inline void baseScan(KREF k, FastS& S, const JobTail& r) {
  int lane = threadIdx.x & 63;
#ifdef ASCHED_FASTPROF
  if (lane == 0) g_rs.statSeg[3] += 1000;   // profiling: scans
#endif
  int s = r.shape;
  int p0 = UNI32(g_fl.cand[s].pos);
  int N = k.N;
  if (k.fitBits) {
    // find-first-set over the shape's "clean and fits" bitmap: 64 lanes x 64 bits = 4096 base entries per memory round trip, whatever lies between
    // the cursor and the next usable entry (entries used up by other shapes, clean entries this shape does not fit on)
    S.statScanSteps++;
    if (UNI32(g_fl.cand[s].node) == -2 && UNI64(g_fl.cand[s].key) != 0) p0++;   // a stale candidate: the entry at the cursor is the one that was used up (its bit may still be on its way to L2)
    for (;;) {
      if (p0 >= N) { if (lane == 0) { g_fl.cand[s].pos = N; g_fl.cand[s].node = -1; } LANE0_PUBLISHED(); return; }
      int w0 = p0 >> 6, w = w0 + lane;
      unsigned long long word = w < k.fitW ? __hip_atomic_load(&k.fitBits[(size_t)s * k.fitW + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
#ifdef ASCHED_FASTPROF
      if (lane == 0) g_rs.statSeg[4] += 1000;   // profiling: bitmap windows read
#endif
      if (lane == 0) word &= ~0ull << (p0 & 63);
      unsigned long long b = __ballot(word != 0);
      if (!b) { p0 = (w0 + 64) << 6; continue; }
      int L = __ffsll((long long)b) - 1;
      unsigned long long wv = slGet64(word, L);
      int q = ((w0 + L) << 6) + (__ffsll((long long)wv) - 1);
      // the entry itself: one more round trip, four independent loads
      unsigned long long key = k.baseKey[q], cls = k.baseCls[q]; int node = k.baseNode[q];
      long long ex0 = k.E > 0 ? k.baseExtra[q] : 0, ex1 = k.E > 1 ? k.baseExtra[k.Npad + q] : 0;
      if (lane == 0) { CandRec c; c.pos = q; c.node = node; c.key = key; c.cls = cls; c.ex0 = ex0; c.ex1 = ex1; c.pad = 0; g_fl.cand[s] = c; }
      LANE0_PUBLISHED();
      return;
    }
  }
  for (;;) {   // ASCHED_FIT_BITS=0: walk the base 64 entries at a time (keys, removed flags, extras, class bits are stored in base order: coalesced)
    if (p0 >= N) { g_fl.cand[s].pos = N; g_fl.cand[s].node = -1; return; }
#ifdef ASCHED_FASTPROF
    if (lane == 0) g_rs.statSeg[4] += 1000;   // profiling: tile loads
#endif
    int p = p0 + lane;
    unsigned long long tKey = 0, tCls = 0; int tNode = -1, tRem = 1; long long tEx0 = 0, tEx1 = 0;
    if (p < N) {
      tKey = k.baseKey[p]; tCls = k.baseCls[p]; tNode = k.baseNode[p]; tRem = k.baseRemoved[p];
      if (k.E > 0) tEx0 = k.baseExtra[p];
      if (k.E > 1) tEx1 = k.baseExtra[k.Npad + p];
    }
    bool ok = !tRem && entryFits(k, r, tKey, tEx0, tEx1, tCls);
    unsigned long long b = __ballot(ok);
    S.statScanSteps++;
    if (b) {
      int f = __ffsll((long long)b) - 1;
      CandRec c;
      c.pos = p0 + f; c.node = __shfl(tNode, f, 64); c.key = __shfl(tKey, f, 64); c.cls = __shfl(tCls, f, 64); c.ex0 = __shfl(tEx0, f, 64); c.ex1 = __shfl(tEx1, f, 64); c.pad = 0;
      g_fl.cand[s] = c;
      return;
    }
    p0 += 64;
  }
}

// mask mode: which fit shapes fit a node with these level-0 key fields / extras / class bits — lane l evaluates shapes l and l + 64 against the table in LDS
__device__ static inline void capMask2(KREF k, uint64_t clsBits, uint64_t key, int64_t ex0, int64_t ex1, uint64_t* m0, uint64_t* m1) {
  int lane = threadIdx.x & 63;
  bool ok0 = false, ok1 = false;
  if (lane < k.S) { const ShapeReq q = SHT(lane); ok0 = !q.never && ((clsBits >> q.cls) & 1) && fieldsGE(k, key, q.fieldMin) && q.ex0 <= ex0 && q.ex1 <= ex1; }
  if (lane + 64 < k.S) { const ShapeReq q = SHT(lane + 64); ok1 = !q.never && ((clsBits >> q.cls) & 1) && fieldsGE(k, key, q.fieldMin) && q.ex0 <= ex0 && q.ex1 <= ex1; }
  *m0 = __ballot(ok0); *m1 = __ballot(ok1);
}
__device__ static inline uint64_t l0Search(KREF k, const JobTail& r, int* slot) {
  int lane = threadIdx.x & 63;
  unsigned long long best = ~0ull; int bs = -1;
  int cnt = UNI32(g_fl.l0Count);
  int rounds = (cnt + 63) >> 6;   // the same trip count on every lane: the cross-lane reduction below sees a converged wave
  if (k.maskMode) {   // one bit per entry says whether the job's shape fits: key + mask, nothing else
    int sh = r.shape & 63; bool hi = r.shape >= 64;   // (wave-uniform: the mask word that holds the job's fit shape)
    for (int r0 = 0; r0 < rounds; r0 += 8) {   // up to 512 entries per group of loads: the usual list is searched with one LDS latency
      unsigned long long key[8], m[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { int i = ((r0 + u) << 6) + lane, j = i < cnt ? i : 0; key[u] = g_fl.l0Key[j]; m[u] = hi ? g_fl.l0Cls2[j] : g_fl.l0Cls[j]; }
#pragma unroll
      for (int u = 0; u < 8; u++) { int i = ((r0 + u) << 6) + lane; if (i < cnt && ((m[u] >> sh) & 1) && key[u] < best) { best = key[u]; bs = i; } }
    }
    unsigned long long mn = waveMin64Dpp(best);
    if (mn == ~0ull) { *slot = -1; return mn; }
    unsigned long long who = __ballot(best == mn);
    *slot = __builtin_amdgcn_readlane(bs, __ffsll((long long)who) - 1);
    return mn;
  }
  // groups of 4, 2, 1 rounds: the loads of a group are issued together (the LDS latency is paid once per group) and only as many rounds as the list has are
  // loaded and tested — late in a round the list is short (140 entries on average on configs[2], 377 over the first quarter)
  auto group = [&](int r0, auto W) {
    constexpr int G = decltype(W)::value;
    unsigned long long key[G], cls[G]; long long e0[G], e1[G];
#pragma unroll
    for (int u = 0; u < G; u++) {
      int i = ((r0 + u) << 6) + lane, j = i < cnt ? i : 0;
      key[u] = g_fl.l0Key[j]; e0[u] = g_fl.l0Ex0[j]; e1[u] = g_fl.l0Ex1[j]; cls[u] = g_fl.l0Cls[j];
    }
#pragma unroll
    for (int u = 0; u < G; u++) {
      int i = ((r0 + u) << 6) + lane;
      if (i < cnt && key[u] < best && entryFits(k, r, key[u], e0[u], e1[u], cls[u])) { best = key[u]; bs = i; }
    }
  };
  int r0 = 0;
  for (; r0 + 4 <= rounds; r0 += 4) group(r0, std::integral_constant<int, 4>{});
  if (r0 + 2 <= rounds) { group(r0, std::integral_constant<int, 2>{}); r0 += 2; }
  if (r0 < rounds) group(r0, std::integral_constant<int, 1>{});
  unsigned long long mn = waveMin64Dpp(best);   // keys are unique (node-index rank in the low bits): the lane that holds the minimum names the slot
  if (mn == ~0ull) { *slot = -1; return mn; }
  unsigned long long who = __ballot(best == mn);
  *slot = __builtin_amdgcn_readlane(bs, __ffsll((long long)who) - 1);
  return mn;
}

// WIN(=4) records x 16 lanes x 8 bytes: one coalesced 128-byte burst per job record
__device__ static inline void winRefill(KREF k, int q, int kind, int pos, int cnt) {
  int lane = threadIdx.x & 63;
  int i = lane >> 4, part = lane & 15;
  if (i < cnt) {
    int job = kind == 0 ? k.evList[pos + i] : k.queuedJobs[pos + i];
    int idx = kind == 0 ? k.evIdxByPos[pos + i] : -1;
    unsigned long long v = k.jrec[(size_t)job * (sizeof(JobRec) / 8) + part];
    ((unsigned long long*)&g_fl.winRec[q][i])[part] = v;
    if (part == 0) { g_fl.winJob[q][i] = job; g_fl.winIdx[q][i] = idx; }
  }
}
__device__ static inline void loadHeadRec(KREF k, int q, int job) {
  int lane = threadIdx.x & 63;
  if (lane < 16) {
    unsigned long long v = k.jrec[(size_t)job * (sizeof(JobRec) / 8) + lane];
    if (lane < 8) ((unsigned long long*)g_fl.headReq[q])[lane] = v; else ((unsigned long long*)&g_fl.headTail[q])[lane - 8] = v;
  }
}
__device__ static inline void headFromWindow(int q, int w) {
  int lane = threadIdx.x & 63;
  if (lane < 16) {
    unsigned long long v = ((const unsigned long long*)&g_fl.winRec[q][w])[lane];
    if (lane < 8) ((unsigned long long*)g_fl.headReq[q])[lane] = v; else ((unsigned long long*)&g_fl.headTail[q])[lane - 8] = v;
  }
}

// markAllocatable (node.go:539-549) for levels [lo, nl) as no-return HBM atomics, one (level, resource) per lane
__device__ static inline void bindUpdate(KREF k, FastS& S, int n, int lo, int nl, int q, uint64_t keyDelta) {
  int lane = threadIdx.x & 63;
  int l = lo + S.laneL;
  if (l < nl) {  // (nl - lo) * R <= 64 lanes whenever P * R <= 64; larger configurations take the second round below
    int64_t v = g_fl.headReq[q][S.laneX];
    if (v) __hip_atomic_fetch_add(&KAL(k, l, S.laneX, n), -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  int R = k.R;
  for (int i = lane + 64; i < (nl - lo) * R; i += 64) {
    int l2 = lo + i / R, x = i % R;
    int64_t v = g_fl.headReq[q][x];
    if (v) __hip_atomic_fetch_add(&KAL(k, l2, x, n), -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane < nl - lo && keyDelta) __hip_atomic_fetch_add(&KKEY(k, lo + lane, n), 0ull - keyDelta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// per-field saturating subtraction on packed order keys: field 0 stands for every negative quotient, so a field that would drop below it stays there
__device__ static inline uint64_t keyFieldsSatSub(KREF k, uint64_t key, uint64_t delta) {
  uint64_t out = key;
#pragma unroll
  for (int c = 0; c < MAXK; c++) {
    if (c >= k.K) break;
    uint64_t m = k.fieldMask[c], f = key & m, dq = delta & m;
    out = (out & ~m) | (f > dq ? f - dq : 0);
  }
  return out;
}
__device__ static inline void keySatSub(KREF k, int n, int lo, int nl, uint64_t keyDelta) {
  int lane = threadIdx.x & 63;
  if (lane < nl - lo && keyDelta) {   // one level per lane; the bind wave / node engine may be adding to the same word: compare-and-swap
    GP(uint64_t) p = &KKEY(k, lo + lane, n);
    uint64_t old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (!__hip_atomic_compare_exchange_strong(p, &old, keyFieldsSatSub(k, old, keyDelta), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {}
  }
}
// sctx / qctx resource vectors for the head job of queue q: accumulate-only, lane x handles resource x;
// LDS vectors through ds_add_u64, HBM by-priority-class vectors through global atomics, all without a return value
__device__ static inline void accountVectors(Dev& d, KREF k, int q, int pc, bool ev, bool replay) {
  (void)d;
  int lane = threadIdx.x & 63;
  if (lane < k.R) {
    int64_t v = g_fl.headReq[q][lane];
    if (v) {
      if (replay) { LDS_ADD64(g_fl.qReplay[q][lane], v); return; }
      LDS_ADD64(g_fl.qAlloc[q][lane], v); LDS_ADD64(g_rs.allocated[lane], v);
      if (ev) LDS_ADD64(g_rs.evicted[lane], -v); else LDS_ADD64(g_rs.scheduled[lane], v);
      size_t i = ((size_t)q * k.npc + pc) * k.R + lane;
      __hip_atomic_fetch_add(&k.qAllocByPc[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ev) __hip_atomic_fetch_add(&k.qEvictedByPc[i], -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_add(&k.qSchedByPc[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
// ---- two-wave iteration (round_fast.h): LDS mailbox between the control wave (0) and the node engine (wave 1).
// LDS executes one wave's accesses in issue order, so "payload, then sequence number" needs no hardware fence — only the
// compiler must keep the order (wavefront-scope fences emit nothing).  No s_waitcnt vmcnt anywhere on this path: neither wave
// ever waits for its own outstanding HBM atomics.
#define LDS_ORDER() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
// ---- bounded waits (round 6).  Every spin of the control workgroup's protocols (mailbox words, ring counters, the engine's acknowledgements) counts its turns; every
// 16 384 turns (~1 ms) it looks at the caller's cancel word (hard timeout / asched_cancel: a read across PCIe) and at the launch's `abandon` flag, and gives up when either is
// set — or when the wait has lasted ~2^26 turns (seconds: no wait of a healthy launch is that long), which raises ASCHED_ERR_DEVICE.  Giving up sets `abandon`, so the
// waves waiting on the other side give up as well and everybody meets at the end barrier of the engine session; the round then returns its error (the handle wants a
// fresh round_prepare, as after any failed round).  What this cannot bound is a workgroup BARRIER that a wave never reaches (profiles/r05y_bulk_skip_hang.txt): those
// are ruled out by construction (eng.live; the CPU build aborts on a wide op posted with the engine live).
#define SPIN_CHECK 0x3fffu
#define SPIN_LIMIT (1u << 26)
__device__ static inline bool waitExpired(unsigned& spins) {   // (inline, and streamIdle's watch too: out of line — tried for the gang rounds, which pay ~2.5 % for these waits — the callers stop being leaf functions and the headline round loses 7 ms)
  if ((++spins & SPIN_CHECK) != 0) return false;
  bool ab = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.abandon, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 0;
  if (!ab && (spins >= SPIN_LIMIT || cancelRequested(g_dev))) {
    if (spins >= SPIN_LIMIT) raise(g_dev, ASCHED_ERR_DEVICE, 950);
    __hip_atomic_store(&g_fl.eng.abandon, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(&g_fl.eng.cancel, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    ab = true;
  }
  return ab;
}
// The node engine's waits (engine_hc.h) sit inside the per-job loop, whose instruction schedule is the headline (its region holds lane-divergent branches, so every branch
// in it costs exec-mask code: a counter with a test per wait cost 4-20 % of the round, profiles/r06z_bounded_waits.txt).  They carry no counter: a turn reads `abandon`
// in LDS, nothing else.  Setting it is the other waves' business: whenever the engine (or the cold wave, or the bind wave behind it) is stuck the control wave ends up in
// streamIdle (the ring is full, or drains) — which looks at the cancel word and keeps the tick budget for all of them — or in one of its own counted waits.
__device__ static inline bool waitAbandoned() { return __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.abandon, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 0; }
__device__ static inline bool waitGaveUp(unsigned& spins) {   // the cold wave's polls: `abandon` every 1 024 turns
  if ((++spins & 0x3ffu) != 0) return false;
  return waitAbandoned();
}
#define IDLE_BUDGET (1u << 22)   // in units of 1 024 shader-clock ticks: ~2 s without one entry placed or bound while the control wave does nothing but wait
__device__ static inline void streamIdleWatch(unsigned long long clk) {
  const int abV = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.abandon, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  // the tick budget: entries placed + entries bound stand still over a stretch of CONTINUOUS waiting (a visit more than three periods after the last one starts a new stretch)
  const unsigned now = (unsigned)(clk >> 10) | 1u;
  const int prog = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringAck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) + __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  const unsigned since = (unsigned)__builtin_amdgcn_readfirstlane(g_fl.eng.idleSince), last = (unsigned)__builtin_amdgcn_readfirstlane(g_fl.eng.idleLast);
  const bool fresh = since == 0 || prog != __builtin_amdgcn_readfirstlane(g_fl.eng.idleProg) || now - last > (3u << 11);
  bool expired = !fresh && now - since > IDLE_BUDGET;
  if (fresh) { __hip_atomic_store(&g_fl.eng.idleProg, prog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); __hip_atomic_store(&g_fl.eng.idleSince, (int)now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __hip_atomic_store(&g_fl.eng.idleLast, (int)now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (expired && abV == 0) raise(g_dev, ASCHED_ERR_DEVICE, 950);
  if (abV != 0 || expired || cancelRequested(g_dev)) {
    if (abV == 0) __hip_atomic_store(&g_fl.eng.abandon, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(&g_fl.eng.cancel, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringFail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0) __hip_atomic_store(&g_fl.eng.ringFail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}
__device__ static inline void streamIdle() {   // the control wave while the ring is full / drains: its waits look at ringFail every turn, so giving up = a failure posted there
  const unsigned long long clk = __builtin_readcyclecounter();   // (issued BEFORE the sleep: its ~80 clocks pass while the wave sleeps; behind the sleep they delayed every wake-up — gang rounds +3.5 %)
  __builtin_amdgcn_s_sleep(2);
  // No counter in LDS or registers (the macro has no state; a 64-lane LDS add per turn took the LDS from the node engine): the shader clock says when to look — one window
  // of 2 048 ticks in every 2^21 (~1 ms); a turn of any of these waits is shorter than the window, so every period is seen at least once.
  if ((((unsigned)clk) & 0x1fffffu) < 0x800u) streamIdleWatch(clk);
}
__device__ static inline void bindUpdateEng(KREF k, FastS& S, int n, int nl, uint64_t keyDelta, const int64_t* req) {
  int lane = threadIdx.x & 63;
  int l = S.laneL;
  if (l < nl) {
    int64_t v = req[S.laneX];
    if (v) __hip_atomic_fetch_add(&KAL(k, l, S.laneX, n), -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  int R = k.R;
  for (int i = lane + 64; i < nl * R; i += 64) {
    int l2 = i / R, x = i % R;
    int64_t v = req[x];
    if (v) __hip_atomic_fetch_add(&KAL(k, l2, x, n), -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane < nl && keyDelta) __hip_atomic_fetch_add(&KKEY(k, lane, n), 0ull - keyDelta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ static inline void accountVectorsBk(Dev& d, KREF k, int q, int pc, int sign) {
  (void)d;
  int lane = threadIdx.x & 63;
  if (lane < k.R) {
    int64_t v = sign * g_fl.eng.req[lane];
    if (v) {
      LDS_ADD64(g_fl.qAlloc[q][lane], v); LDS_ADD64(g_rs.allocated[lane], v); LDS_ADD64(g_rs.scheduled[lane], v);
      size_t i = ((size_t)q * k.npc + pc) * k.R + lane;
      __hip_atomic_fetch_add(&k.qAllocByPc[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&k.qSchedByPc[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
// One LDS pass, one word per lane: FL.bk := queue q's record and keys (what a rollback restores), FL.eng := the job (record, request,
// parameters); then the sequence number.  The job's record and request are not duplicated in the backup: the engine only reads them.
__device__ static inline void enginePost(Dev& d, KREF k, FastS& S, int job, int q, int pc, int32_t prio, int32_t cutoff, int nl) {
  (void)d; (void)k;
  int lane = threadIdx.x & 63;
  constexpr int HW = sizeof(QHot) / 8, TW = sizeof(JobTail) / 8, B = HW + TW + MAXR;
  static_assert(sizeof(QHot) % 8 == 0 && B + 9 <= 64, "backup + post fit one wave");
  if (lane < HW) ((unsigned long long*)&g_fl.bk.hot)[lane] = ((const unsigned long long*)&g_fl.hot[q])[lane];
  else if (lane < HW + TW) ((unsigned long long*)&g_fl.eng.tail)[lane - HW] = ((const unsigned long long*)&g_fl.headTail[q])[lane - HW];
  else if (lane < B) g_fl.eng.req[lane - HW - TW] = g_fl.headReq[q][lane - HW - TW];
  if (lane == 0) {
    g_fl.bk.kA = g_fl.kA[q]; g_fl.bk.kX = g_fl.kX[q]; g_fl.bk.kY = g_fl.kY[q];
    g_fl.bk.effA = g_fl.effA[q]; g_fl.bk.effX = g_fl.effX[q]; g_fl.bk.effY = g_fl.effY[q];
    g_fl.bk.inHeap = g_fl.inHeap[q]; g_fl.bk.globalTokens = S.globalTokens; g_fl.bk.pc = pc;
    g_fl.eng.job = job; g_fl.eng.prio = prio; g_fl.eng.cutoff = cutoff; g_fl.eng.nl = nl; g_fl.eng.cmd = ENG_JOB;
  }
  S.engSeq++;
  LDS_ORDER();
  if (lane == 0) __hip_atomic_store(&g_fl.eng.seq, S.engSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ static inline void engineRestore(int q) {
  int lane = threadIdx.x & 63;
  constexpr int HW = sizeof(QHot) / 8, TW = sizeof(JobTail) / 8, B = HW + TW + MAXR;
  if (lane < HW) ((unsigned long long*)&g_fl.hot[q])[lane] = ((const unsigned long long*)&g_fl.bk.hot)[lane];
  else if (lane < HW + TW) ((unsigned long long*)&g_fl.headTail[q])[lane - HW] = ((const unsigned long long*)&g_fl.eng.tail)[lane - HW];
  else if (lane < B) g_fl.headReq[q][lane - HW - TW] = g_fl.eng.req[lane - HW - TW];
  else if (lane == B) { g_fl.kA[q] = g_fl.bk.kA; g_fl.kX[q] = g_fl.bk.kX; g_fl.kY[q] = g_fl.bk.kY; }
  else if (lane == B + 1) { g_fl.effA[q] = g_fl.bk.effA; g_fl.effX[q] = g_fl.bk.effX; g_fl.effY[q] = g_fl.bk.effY; g_fl.inHeap[q] = g_fl.bk.inHeap; }
  LANE0_PUBLISHED();   // lanes B, B + 1 wrote fixed words the whole wave reads next (fastRollback's caller rebuilds the heap from them)
}
__device__ static inline int engineWait(const FastS& S) {
  int want = S.engSeq;
  unsigned spins = 0;
  for (;;) {
    int a = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (a == want) break;
    __builtin_amdgcn_s_sleep(1);
    if (waitExpired(spins)) return 0;   // (as if the job had found no node: the caller takes the iteration back and meets the cancel flag)
  }
  LDS_ORDER();
  return __builtin_amdgcn_readfirstlane(g_fl.eng.status);
}

// ---- stream run (round_fast.h): ring between the control wave (merge + record staging) and the node engine
__device__ static inline void qsWinRefill(KREF k, int q, int pos, int cnt) {
  int lane = threadIdx.x & 63;
  if (lane < cnt * 4) ((unsigned long long*)&g_fl.evWin[q][0])[lane] = k.qsKey[((size_t)q * QS_CMAX + pos) * 4 + lane];
}
__device__ static inline void streamBegin(int* engSeq, int hold, int hc) {
  int lane = threadIdx.x & 63;
  if (lane == 0) { g_fl.eng.bindHold = hold; g_fl.eng.ringPub = 0; g_fl.eng.ringAck = 0; g_fl.eng.ringEnd = 0; g_fl.eng.ringFail = 0; g_fl.eng.ringClosed = 0; g_fl.eng.bindDone = 0; g_fl.eng.idleSince = 0; g_fl.eng.cmd = hc ? ENG_STREAM_HC : ENG_STREAM; }
  (*engSeq)++;
  LDS_ORDER();
  if (lane == 0) __hip_atomic_store(&g_fl.eng.bindGen, g_fl.eng.bindGen + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  LDS_ORDER();
  if (lane == 0) __hip_atomic_store(&g_fl.eng.seq, *engSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// records of ring entries [base, base + cnt), cnt <= 4: 16 lanes x 8 bytes each, one coalesced 128-byte burst per record; the value is consumed by
// streamStageCommit one group later, so the HBM latency runs under the merge
__device__ static inline unsigned long long streamStageIssue(KREF k, int base, int cnt) {
  int lane = threadIdx.x & 63;
  int i = lane >> 4, part = lane & 15;
  unsigned long long v = 0;
  if (i < cnt && !(RQ(base + i) & RQ_EV)) { int job = RJOB(base + i); v = k.jrec[(size_t)job * (sizeof(JobRec) / 8) + part]; }
  return v;
}
__device__ static inline void streamStageCommit(Dev& d, KREF k, int base, int cnt, unsigned long long v) {
  (void)d; (void)k;
  int lane = threadIdx.x & 63;
  int i = lane >> 4, part = lane & 15;
  if (i < cnt && !(RQ(base + i) & RQ_EV)) ((unsigned long long*)&RREC(base + i))[part] = v;
  LDS_ORDER();
  if (lane == 0) __hip_atomic_store(&g_fl.eng.ringPub, base + cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ static inline void streamEnd(int engSeq) {
  int lane = threadIdx.x & 63;
  LDS_ORDER();
  if (lane == 0) __hip_atomic_store(&g_fl.eng.ringEnd, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  unsigned spins = 0;
  for (;;) {   // the engine acknowledges the ENG_STREAM command when it has left the ring
    int a = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (a == engSeq) break;
    __builtin_amdgcn_s_sleep(1);
    if (waitExpired(spins)) { LDS_ORDER(); return; }
  }
  if (__builtin_amdgcn_readfirstlane(g_fl.eng.bindHold)) { LDS_ORDER(); return; }   // a gang: the verdict comes first (streamRelease)
  int gen = __builtin_amdgcn_readfirstlane(g_fl.eng.bindGen);
  for (;;) {   // ... and the bind wave has issued (and released) the binds of every entry placed
    int f = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindFin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (f == gen) break;
    __builtin_amdgcn_s_sleep(1);
    if (waitExpired(spins)) break;
  }
  LDS_ORDER();
}
__device__ static inline void streamRelease(Dev& d, KREF k, int go) {
  (void)d; (void)k;
  int lane = threadIdx.x & 63;
  if (lane == 0) __hip_atomic_store(&g_fl.eng.bindHold, go ? 2 : 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  int gen = __builtin_amdgcn_readfirstlane(g_fl.eng.bindGen);
  unsigned spins = 0;
  for (;;) {
    int f = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindFin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (f == gen) break;
    __builtin_amdgcn_s_sleep(1);
    if (waitExpired(spins)) break;
  }
  LDS_ORDER();
}
__device__ static inline int streamBound() { return __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); }
__device__ static inline int streamAcked(int* fail) {
  int a = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringAck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  int f = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringFail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  // a failure flag read together with an older ack count: entries bound before the failing one are all counted when the flag is seen again after the ack
  if (f) a = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringAck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  *fail = f;
  return a;
}
// sctx / qctx accounting of ring entries [i0, i1) once the engine has bound them (accountVectors for a new job): 4 (8 when R > 4) lanes per entry, one per
// resource, so a batch of acknowledgements costs one pass; FL.tmpQ[q] counts queue q's entries.  An entry of an evicted stream only counts: its
// commit is deferred like a cheap evicted head's (applyEvictedRange)
__device__ static inline void streamAccount(Dev& d, KREF k, int i0, int i1) {
  (void)d;
  int lane = threadIdx.x & 63;
  int sh = k.R <= 4 ? 2 : 3, per = 64 >> sh;
  int e = lane >> sh, x = lane & ((1 << sh) - 1);
  for (int b = i0; b < i1; b += per) {
    int i = b + e;
    if (i < i1) {
      int rq = RQ(i), q = rq & 0xff;
      if (x == 0) (void)__hip_atomic_fetch_add(&g_fl.tmpQ[q], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (!(rq & RQ_EV) && x < k.R) {
        const JobRec& r = RREC(i);
        int64_t v = r.req[x];
        if (v) {
          LDS_ADD64(g_fl.qAlloc[q][x], v); LDS_ADD64(g_rs.allocated[x], v); LDS_ADD64(g_rs.scheduled[x], v);
          size_t j = ((size_t)q * k.npc + r.pc) * k.R + x;
          __hip_atomic_fetch_add(&k.qAllocByPc[j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(&k.qSchedByPc[j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
}
// key and name rank of the heap's head entry (queue t): lane 0 of the heap lanes, no LDS access
__device__ static inline void pqHeadKey(PQState& s, int t, PackedKey* key, uint32_t* nameRank) {
  if (__builtin_amdgcn_readfirstlane(s.q) == t) {
    key->A = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.A); *nameRank = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.N);
    key->X = UNI64(s.X); key->Y = UNI64(s.Y);
  } else {
    key->A = UNI32(g_fl.kA[t]); key->X = UNI64(g_fl.kX[t]); key->Y = UNI64(g_fl.kY[t]); *nameRank = (uint32_t)UNI32(g_fl.nameRank[t]);
  }
}
// the engine session is one mailbox op of the control workgroup: wave 1 serves jobs until ENG_QUIT, waves 2.. wait at the end barrier
__device__ static inline void engineStart(Dev& d, FastS& S) {
  (void)d;
  S.engSeq = 0;
  if ((threadIdx.x & 63) == 0) { g_fl.eng.seq = 0; g_fl.eng.ack = 0; g_fl.eng.statScan = 0; g_fl.eng.statL0Max = S.statL0Max; g_fl.eng.busyClk = 0; g_fl.eng.jobs = 0; g_fl.eng.cancel = 0; g_fl.eng.bindQuit = 0; g_fl.eng.bindGen = 0; g_fl.eng.bindFin = 0; g_fl.eng.hcGen = 0; g_fl.eng.idleSince = 0; g_fl.eng.live = 1; g_mb.op = OP_ENGINE; }
  __syncthreads();
}
__device__ static inline void engineStop(Dev& d, FastS& S) {
  (void)d;
  int lane = threadIdx.x & 63;
  if (lane == 0) { g_fl.eng.cmd = ENG_QUIT; __hip_atomic_store(&g_fl.eng.bindQuit, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  LDS_ORDER();
  S.engSeq++;
  if (lane == 0) __hip_atomic_store(&g_fl.eng.seq, S.engSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  (void)engineWait(S);
  if (lane == 0) g_fl.eng.live = 0;
  LANE0_PUBLISHED();
  S.statScanSteps += __builtin_amdgcn_readfirstlane(g_fl.eng.statScan);
  int m = __builtin_amdgcn_readfirstlane(g_fl.eng.statL0Max);
  if (m > S.statL0Max) S.statL0Max = m;
#ifndef ASCHED_FASTPROF
  if (lane == 0) { g_rs.statSeg[1] += g_fl.eng.busyClk; g_rs.statSeg[2] += g_fl.eng.jobs; }
  LANE0_PUBLISHED();
#endif
  __syncthreads();  // end barrier of the OP_ENGINE op
}
#include "engine_hc.h"
__device__ static void engineLoop(Dev& d) {  // wave 1
  const FastK k = fastKRef(d);
  int lane = threadIdx.x & 63;
  FastS ES;
   ES.engLive = 0; ES.engPend = -1;
  ES.laneL = lane / (k.R > 0 ? k.R : 1); ES.laneX = lane % (k.R > 0 ? k.R : 1);
  ES.statScanSteps = 0; ES.statL0Max = __builtin_amdgcn_readfirstlane(g_fl.eng.statL0Max);
  ES.fastActive = 1; ES.engSeq = 0;
  long long busy = 0; int jobs = 0;
  int seen = 0;
#ifdef ASCHED_FASTPROF
  for (int i = 0; i < 8; i++) ES.eseg[i] = 0;
  ES.segT = CLK();
#endif
  unsigned spins = 0;
  for (;;) {
    int sq;
    for (;;) {
      sq = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (sq != seen) break;
      __builtin_amdgcn_s_sleep(1);
      if (waitExpired(spins)) return;   // (to the end barrier of the engine session: the control wave, whose waits give up too, comes there through engineStop)
    }
    spins = 0;
    seen = sq;
    LDS_ORDER();
    int cmd = __builtin_amdgcn_readfirstlane(g_fl.eng.cmd);
    if (cmd == ENG_QUIT) {
#ifdef ASCHED_FASTPROF
      if (lane == 0) for (int i = 0; i < 8; i++) g_rs.statSeg[16 + i] += ES.eseg[i];   // [16] waiting for a job, [17] record, [18] first fit, [19] bind, [20] result fields, [21] L0 upkeep, [22] verdict
#endif
      if (lane == 0) { g_fl.eng.statScan = ES.statScanSteps; g_fl.eng.statL0Max = ES.statL0Max; g_fl.eng.busyClk = busy; g_fl.eng.jobs = jobs; }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this wave's binds and result stores are complete before the generic code reads them
      LDS_ORDER();
      if (lane == 0) __hip_atomic_store(&g_fl.eng.ack, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return;
    }
    if (cmd == ENG_STREAM_HC) {   // a bulk-merged run's ring session on the split level-0 structure (engine_hc.h); same ring contract as below
      long long b0 = (long long)__builtin_readcyclecounter();
      engineStreamHc(d, k, ES);
      busy += (long long)__builtin_readcyclecounter() - b0; jobs += __builtin_amdgcn_readfirstlane(g_fl.eng.ringAck);
      LDS_ORDER();
      if (lane == 0) __hip_atomic_store(&g_fl.eng.ringClosed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (lane == 0) __hip_atomic_store(&g_fl.eng.ack, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      continue;
    }
    if (cmd == ENG_STREAM) {
      // walk the ring: entry i is ready when ringPub > i; stop at the first job that finds no node (ringFail 1), after an L0 overflow (2), or when the
      // control wave has closed the ring and everything staged is bound
      int i = 0, pub = 0;
      for (;;) {
        while (pub <= i) {   // (the counter is read again only when the entries known to be staged are used up)
          pub = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringPub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
          if (pub > i) break;
          int end = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringEnd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
          if (end) { pub = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringPub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); break; }
          __builtin_amdgcn_s_sleep(1);
          if (waitExpired(spins)) return;
        }
        if (pub <= i) break;
        LDS_ORDER();
        if (__builtin_amdgcn_readfirstlane(RQ(i)) & RQ_EV) {   // an evicted job returning to its node: nothing to select or bind here
          i++;
          if (lane == 0) __hip_atomic_store(&g_fl.eng.ringAck, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          continue;
        }
        ESEG(0);
#ifdef ASCHED_FASTPROF
        long long b0 = (long long)__builtin_readcyclecounter();
#endif
        int st = engineServeRing(d, k, ES, i);
#ifdef ASCHED_FASTPROF
        busy += (long long)__builtin_readcyclecounter() - b0;   // (the clock reads sit on the engine's chain: profiling builds only)
#endif
        jobs++;
        if (st == 0) { if (lane == 0) __hip_atomic_store(&g_fl.eng.ringFail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break; }
        i++;
        if (lane == 0) __hip_atomic_store(&g_fl.eng.ringAck, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (st == 2) { LDS_ORDER(); if (lane == 0) __hip_atomic_store(&g_fl.eng.ringFail, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break; }
        ESEG(6);
      }
      LDS_ORDER();
      if (lane == 0) __hip_atomic_store(&g_fl.eng.ringClosed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (lane == 0) __hip_atomic_store(&g_fl.eng.ack, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      continue;
    }
    ESEG(0);
    long long b0 = (long long)__builtin_readcyclecounter();
    int st = engineServe(d, k, ES);
    busy += (long long)__builtin_readcyclecounter() - b0; jobs++;
    if (lane == 0) g_fl.eng.status = st;
    LDS_ORDER();
    if (lane == 0) __hip_atomic_store(&g_fl.eng.ack, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    ESEG(6);
  }
}

// Wave 2 during an engine session: the HBM side of a stream run's placements.  The node engine decides (first fit, L0 upkeep: LDS) and leaves the node in
// the ring entry; this wave follows its acknowledgement counter and issues BindJobToNode's plane / key atomics and the job's result fields.  Nothing on the
// engine's chain reads what is written here (level-0 state lives in the base flags + L0), so the two run concurrently; the release fence at the end of a
// stream orders the writes before whatever the control wave does next.
__device__ static void bindLoop(Dev& d) {
  const FastK k = fastKRef(d);
  int lane = threadIdx.x & 63;
  FastS BS;
   BS.laneL = lane / (k.R > 0 ? k.R : 1); BS.laneX = lane % (k.R > 0 ? k.R : 1);
#ifdef ASCHED_FASTPROF
  for (int i = 0; i < 8; i++) BS.eseg[i] = 0;
  BS.segT = 0;
#endif
  int gen = 0;
  unsigned spins = 0;
  for (;;) {
    for (;;) {
      int g = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindGen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (g != gen) { gen = g; break; }
      if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindQuit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) return;
      __builtin_amdgcn_s_sleep(2);
      if (waitExpired(spins)) return;
    }
    spins = 0;
    int i = 0;
    bool discard = false;
    if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindHold, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {   // a gang: all members or none
      int hmode;
      for (;;) {
        hmode = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.bindHold, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (hmode != 1) break;
        __builtin_amdgcn_s_sleep(1);
        if (waitExpired(spins)) return;
      }
      discard = hmode == 3;
    }
    for (; !discard;) {
      int ack = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringAck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (i >= ack) {
        if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringClosed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
          ack = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_fl.eng.ringAck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
          if (i >= ack) break;
        } else { __builtin_amdgcn_s_sleep(1); if (waitExpired(spins)) return; continue; }
      }
      LDS_ORDER();
      for (; i < ack; i++) {
        if (__builtin_amdgcn_readfirstlane(RQ(i)) & RQ_EV) continue;
        const JobRec& r = RREC(i);
        int n = __builtin_amdgcn_readfirstlane(r.node0), job = __builtin_amdgcn_readfirstlane(RJOB(i));
        int32_t p = __builtin_amdgcn_readfirstlane(r.pcPrio);
        int32_t cutoff = __builtin_amdgcn_readfirstlane((int)r.preemptible) ? p : NONPREEMPTIBLE_CUTOFF;
        FastS& ES = BS;
        bindJob(k, ES, n, __builtin_amdgcn_readfirstlane((int)r.nlPc), UNI64(r.keyDelta), r.req, job, p, cutoff);
      }
      LDS_ORDER();
      if (lane == 0) __hip_atomic_store(&g_fl.eng.bindDone, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    LDS_ORDER();
    if (lane == 0) __hip_atomic_store(&g_fl.eng.bindFin, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// WIN EvKey records (32 B each) of queue q's evicted stream: 4 lanes x 8 bytes per record
__device__ static inline void evWinRefill(KREF k, int q, int pos, int cnt) {
  int lane = threadIdx.x & 63;
  if (lane < cnt * 4) ((unsigned long long*)&g_fl.evWin[q][0])[lane] = k.evKey[(size_t)pos * 4 + lane];
}
// Deferred commits of evicted jobs [p0, p1) of queue q returning to their nodes, one job per lane: the evicted branch of
// fastIter's commit (node.go:416-442 arithmetic, sctx/qctx accounting) as no-return atomics and plain stores.  Node planes are
// hit at distinct addresses; the per-queue / per-priority-class sums are accumulated per lane and reduced across the wave once,
// so that 64 lanes do not serialise on one counter.  Not inlined: a cold, register-hungry path next to the hot loop.
__device__ static inline int64_t waveSum64(int64_t v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
#define APPLY_PCS 4
__device__ static __attribute__((noinline)) void applyEvictedRange(Dev& d, int q, int p0, int p1, int sign) {
  const FastK k = fastKRef(d);
  int lane = threadIdx.x & 63;
  int R = k.R;
  int pending = g_rs.replayPending;
  if (sign < 0 && !pending && lane == 0) g_rs.ftValid = 0;
  LANE0_PUBLISHED();
  int64_t accQ[MAXR], accPc[APPLY_PCS][MAXR];
#pragma unroll
  for (int x = 0; x < MAXR; x++) { accQ[x] = 0;
#pragma unroll
    for (int c = 0; c < APPLY_PCS; c++) accPc[c][x] = 0; }
  for (int p = p0 + lane; p < p1; p += 64) {
    int job = k.evList[p];
    GP(unsigned long long) rec = k.jrec + (size_t)job * (sizeof(JobRec) / 8);
    unsigned long long keyDelta = rec[8];
    unsigned long long w10 = rec[10], w11 = rec[11], w12 = rec[12], w13 = rec[13];
    int pcx = (int)(unsigned)w10, n = (int)(unsigned)(w11 >> 32), prio = (int)(unsigned)w12;
    unsigned flags = (unsigned)(w13 >> 32);
    int preemptible = (flags >> 8) & 255, nlRun = (flags >> 24) & 255;
    int32_t cutoff = preemptible ? prio : NONPREEMPTIBLE_CUTOFF;
#pragma unroll
    for (int x = 0; x < MAXR; x++) {
      if (x >= R) break;
      int64_t v = sign * (int64_t)rec[x];
      if (!v) continue;
      accQ[x] += v;
      if (pcx < APPLY_PCS) {
#pragma unroll
        for (int c = 0; c < APPLY_PCS; c++) if (c == pcx) accPc[c][x] += v;
      } else {
        size_t i = ((size_t)q * k.npc + pcx) * R + x;
        __hip_atomic_fetch_add(&k.qAllocByPc[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&k.qEvictedByPc[i], -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      for (int l = 1; l < nlRun; l++) __hip_atomic_fetch_add(&KAL(k, l, x, n), -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (keyDelta) for (int l = 1; l < nlRun; l++) __hip_atomic_fetch_add(&KKEY(k, l, n), sign > 0 ? 0ull - keyDelta : keyDelta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sign < 0) {  // taken back: the job is evicted again, exactly as the evictor left it (eviction.go:245-260, evictApply)
      k.jcHasPctx[job] = 0; k.pcNode[job] = -1; k.pcSap[job] = 0; k.pcPap[job] = ASCHED_MIN_PRIORITY; k.pcMethod[job] = ASCHED_METHOD_NONE;
      k.jobEvictedOnNode[job] = 1; k.jobFlags[job] = F_EVICTED; k.inPreempted[job] = 1;
      if (!pending) { int idx = k.evIdxByPos[p]; k.evTabAlive[idx] = 1; k.evIndexOfJob[job] = idx; g_rs.fairIndexValid = 0; }   // (an entry comes back: ensureFairIndex)
      continue;
    }
    k.jcReason[job] = 0; k.jcHasPctx[job] = 1; k.pcNode[job] = n; k.pcSap[job] = prio;
    k.jobNode[job] = n; k.jobCutoff[job] = cutoff; k.jobEvictedOnNode[job] = 0; k.schedAtPrio[job] = prio; k.inSchedAndEvicted[job] = 0;
    k.pcPap[job] = prio; k.pcMethod[job] = ASCHED_METHOD_RESCHEDULED; k.jobFlags[job] = F_RESCHEDULED; k.inPreempted[job] = 0;
    if (!pending) { k.evTabAlive[k.evIdxByPos[p]] = 0; k.evIndexOfJob[job] = -1; }
  }
#pragma unroll
  for (int x = 0; x < MAXR; x++) {
    if (x >= R) break;
    int64_t v = waveSum64(accQ[x]);
    if (x == 0) LANE0_PUBLISHED();   // (the loop above: g_rs.fairIndexValid = 0 under a lane-divergent condition)
    if (lane == 0 && v) { LDS_ADD64(g_fl.qAlloc[q][x], v); LDS_ADD64(g_rs.allocated[x], v); LDS_ADD64(g_rs.evicted[x], -v); }
#pragma unroll
    for (int c = 0; c < APPLY_PCS; c++) {
      if (c >= k.npc) break;
      int64_t w = waveSum64(accPc[c][x]);
      if (lane == 0 && w) {
        size_t i = ((size_t)q * k.npc + c) * R + x;
        __hip_atomic_fetch_add(&k.qAllocByPc[i], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&k.qEvictedByPc[i], -w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
__device__ static inline bool roundLimitExceeded(Dev& d, KREF k) {
  int lane = threadIdx.x & 63;
  bool ex = lane < k.R && g_rs.scheduled[lane] > d.cfg.maxToSchedule[lane];
  return __ballot(ex) != 0;  // ballot results are scalar
}
__device__ static inline bool headRequestsDisallowed(Dev& d, KREF k, int q) {
  int lane = threadIdx.x & 63;
  bool bad = lane < k.R && d.cfg.disallowed[lane] && g_fl.headReq[q][lane] > 0;
  return __ballot(bad) != 0;
}

// pinned-node check of a returning evicted job against the node's current allocatable (nodedb.go:897-906): one lane per resource; the planes are
// updated by no-return atomics that execute at L2, so the reads go there too (agent-scope atomic loads, never the L1)
__device__ static inline bool pinnedNodeFits(KREF k, int q, int n, int level) {
  int lane = threadIdx.x & 63;
  if (UNI32((int)k.nodeFlags[n]) & 1) return true;
  bool bad = false;
  if (lane < k.R) {
    int64_t have = __hip_atomic_load(&KAL(k, level, lane, n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bad = g_fl.headReq[q][lane] > have;
  }
  return __ballot(bad) == 0;
}

__device__ static inline void exclPinnedFast(Dev& d, KREF k, int q, int job, int n, int level) {
  int lane = threadIdx.x & 63;
  int64_t have = 0;
  if (lane < k.R) have = __hip_atomic_load(&KAL(k, level, lane, n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  bool bad = lane < k.R && g_fl.headReq[q][lane] > have;
  unsigned long long m = __ballot(bad);
  if (!m) { if (lane == 0) d.excl[job] = EXCL_S_UNSUPPORTED; return; }
  int res = __builtin_ctzll(m);
  if (lane == res) { EXCL(d)->pinAvail[job] = have; d.excl[job] = EXCL_S_PINNED0 - res; }
}
__device__ static inline EvDyn evDynLoad(KREF k, int q, int job, int n, int level, bool wantMark, bool wantPin) {
  int lane = threadIdx.x & 63;
  // three independent loads, issued back to back; the first use below waits for all of them once
  int mark = wantMark ? (int)k.jcPreempted[job] : 0;
  int nf = wantPin ? (int)k.nodeFlags[n] : 0;
  int64_t have = 0;
  if (wantPin && lane < k.R) have = __hip_atomic_load(&KAL(k, level, lane, n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  EvDyn r;
  r.preempted = UNI32(mark);
  bool bad = wantPin && lane < k.R && g_fl.headReq[q][lane] > have;
  r.fits = (!wantPin || (UNI32(nf) & 1) || __ballot(bad) == 0) ? 1 : 0;
  return r;
}

__device__ static inline EvDyn evCleanLoad(KREF k, int job, int n, bool wantMark, bool wantClean) {
  int lane = threadIdx.x & 63;
  int mark = wantMark ? (int)k.jcPreempted[job] : 0;   // independent loads, issued back to back
  int64_t have = 0;
  if (wantClean && lane < k.R) have = __hip_atomic_load(&KAL(k, 0, lane, n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  EvDyn r;
  r.preempted = UNI32(mark);
  r.fits = __ballot(wantClean && lane < k.R && have < 0) == 0 ? 1 : 0;
  return r;
}
__device__ static inline unsigned long long evPendingMask(int Q) {
  int q = threadIdx.x & 63;
  return __ballot(q < Q && g_fl.hot[q].evApplied < g_fl.hot[q].evDone);
}

// ------------------------------------------------------------------------------------------------ LDS residency of the round's small state
// Every per-queue array and the scheduling-context scalars are moved into LDS for the duration of the launch by
// re-pointing the Dev descriptor (which itself lives in LDS): generic and fast code alike then pay LDS latency for them.
#define ARENA_BYTES (16 * 1024)
__shared__ unsigned long long g_arena[ARENA_BYTES / 8];
struct Reloc { void** pp; void* global; int bytes; };
#define MAX_RELOC 48
__shared__ Reloc g_reloc[MAX_RELOC];
__shared__ int g_nreloc;
__shared__ RoundScalars* g_rsGlobal;

__device__ static void relocateIn(Dev& d, int cmd) {
  // executed by every thread; the table is built by thread 0
  if (threadIdx.x == 0) {
    g_nreloc = 0;
    g_rsGlobal = d.rs;
    int Q = d.cfg.Q, R = d.cfg.R, npc = d.cfg.npc;
#ifdef ASCHED_MARKET_ROUND
    const bool marketCmd = cmd == CMD_MARKET_ROUND || cmd == CMD_MARKET_QUEUES;   // (k_control_aux / k_control_wk; k_control's code does not see this)
#else
    const bool marketCmd = false;
#endif
    bool want = (cmd == CMD_ROUND || cmd == CMD_QUEUES_ONLY || cmd == CMD_PASS1 || cmd == CMD_PASS2 || marketCmd) && Q > 0 && d.qWeight != nullptr && (Q <= QCAPF || d.f.relocAll);
    if (want) {
      int off = 0, n = 0; bool fits = true;
      auto add = [&](void** pp, int bytes) {
        if (!*pp || !fits) return;
        int b = (bytes + 7) & ~7;
        if (off + b > ARENA_BYTES || n >= MAX_RELOC) { fits = false; return; }
        g_reloc[n].pp = pp; g_reloc[n].global = *pp; g_reloc[n].bytes = bytes; n++; off += b;
      };
      int q1 = Q + 1;
      add((void**)&d.qWeight, Q * 8); add((void**)&d.qNameRank, Q * 4); add((void**)&d.qTokens, Q * 8); add((void**)&d.qBurst, Q * 8);
      add((void**)&d.qRateInf, Q); add((void**)&d.qCordoned, Q); add((void**)&d.qAlloc, Q * R * 8); add((void**)&d.qPenalty, Q * R * 8);
      // qAllocByPc / qSchedByPc / qEvictedByPc stay in HBM: the fast path accumulates into them with global atomics
      add((void**)&d.queuedOff, q1 * 4); add((void**)&d.evOff, (Q + 2) * 4);
      add((void**)&d.itEi, q1 * 4); add((void**)&d.itQi, q1 * 4); add((void**)&d.itStage, q1 * 4); add((void**)&d.itJobsSeen, q1 * 4);
      add((void**)&d.itNext, q1 * 4); add((void**)&d.itStashed, q1 * 4);
      add((void**)&d.itJobOnlyEv, q1); add((void**)&d.itGangOnlyEv, q1); add((void**)&d.onlyEvByQueue, q1); add((void**)&d.qEvictable, q1);
      add((void**)&d.pqProposed, q1 * 8); add((void**)&d.pqCurrent, q1 * 8); add((void**)&d.pqBudget, q1 * 8); add((void**)&d.pqSize, q1 * 8);
      add((void**)&d.pqPcPrio, q1 * 4); add((void**)&d.pqSchedPrio, q1 * 4); add((void**)&d.pqGctx, q1 * 4); add((void**)&d.pqInHeap, q1);
      add((void**)&d.replayAlloc, q1 * R * 8);
#ifdef ASCHED_MARKET_ROUND
      if (marketCmd && g_mk.s) {   // MarketIteratorPQ's items and heap, the merge iterators' held values, the round's market scalars (round_mkt.h)
        add((void**)&g_mk.s, (int)sizeof(MktScalars));
        add((void**)&g_mk.heap, q1 * 4); add((void**)&g_mk.pqPrice, q1 * 8); add((void**)&g_mk.pqRuntime, q1 * 8); add((void**)&g_mk.pqSubmit, q1 * 8); add((void**)&g_mk.pqQueued, q1);
        add((void**)&g_mk.itV1, q1 * 4); add((void**)&g_mk.itV2, q1 * 4);
        add((void**)&g_mk.qBillable, Q * R * 8); add((void**)&g_mk.qOverride, Q * 8); add((void**)&g_mk.qHasOverride, Q);
      }
#endif
      g_nreloc = fits ? n : 0;
    }
  }
  __syncthreads();
  // scalars
  {
    const int* src = (const int*)g_rsGlobal; int* dst = (int*)&g_rs;
    for (int i = threadIdx.x; i < (int)(sizeof(RoundScalars) / sizeof(int)); i += blockDim.x) dst[i] = src[i];
  }
  int off = 0;
  for (int k = 0; k < g_nreloc; k++) {
    const unsigned char* src = (const unsigned char*)g_reloc[k].global; unsigned char* dst = (unsigned char*)g_arena + off;
    for (int i = threadIdx.x; i < g_reloc[k].bytes; i += blockDim.x) dst[i] = src[i];
    off += (g_reloc[k].bytes + 7) & ~7;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int o = 0;
    for (int k = 0; k < g_nreloc; k++) { *g_reloc[k].pp = (unsigned char*)g_arena + o; o += (g_reloc[k].bytes + 7) & ~7; }
    d.rs = &g_rs;
  }
  __syncthreads();
}
__device__ static void relocateOut() {
  __syncthreads();
  {
    int* dst = (int*)g_rsGlobal; const int* src = (const int*)&g_rs;
    for (int i = threadIdx.x; i < (int)(sizeof(RoundScalars) / sizeof(int)); i += blockDim.x) dst[i] = src[i];
  }
  int off = 0;
  for (int k = 0; k < g_nreloc; k++) {
    unsigned char* dst = (unsigned char*)g_reloc[k].global; const unsigned char* src = (const unsigned char*)g_arena + off;
    for (int i = threadIdx.x; i < g_reloc[k].bytes; i += blockDim.x) dst[i] = src[i];
    off += (g_reloc[k].bytes + 7) & ~7;
  }
  __threadfence();
}

// ------------------------------------------------------------------------------------------------ kernels
template <class A> __device__ static inline A helpArgs(HelpBox* b, int at = 0) {
  A a;
  ull_alias* w = (ull_alias*)&a;
  for (int i = 0; i < (int)(sizeof(A) / 8); i++) w[i] = __hip_atomic_load(&b->args[at + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return a;
}
// Helper workgroup.  Wave 0 polls the command word in HBM (backing off to ~30 us between polls when the round has not asked
// for anything for a while, so an idle helper costs no measurable fabric traffic) and republishes it in LDS; the other waves
// poll that LDS word.  Each wave takes its share of the nodes, folds its result into an LDS word, and the wave that
// arrives last sends the workgroup's result and ONE completion increment to HBM.  Every loop in here is wave-uniform and
// there is no workgroup barrier inside the loop on purpose: a "thread 0 polls, the others wait at the barrier" loop gets
// rotated by the compiler so that the polling lane's tail and head merge across the back edge, and the rest of its wave
// then runs ahead through the barriers without it.
__shared__ unsigned long long g_hCmd, g_hMin, g_hMax;
__shared__ unsigned int g_hArrived;
__device__ static inline unsigned long long waveUniform64(unsigned long long v) {
  return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ static void helperMain(const Dev& d, HelpBox* b, int H) {
  if (threadIdx.x == 0) { g_hCmd = 0; g_hMin = ~0ull; g_hMax = 0; g_hArrived = 0; }
  __syncthreads();
  unsigned long long seen = 0;
  int tid = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x, nthreads = (H + 1) * (int)blockDim.x;
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  for (;;) {
    unsigned long long g;
    if (wave == 0) {
      unsigned int idle = 0;
      for (;;) {
        g = waveUniform64(__hip_atomic_load(&b->cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (g != seen) break;
        idle++;
        if (idle < 2048) __builtin_amdgcn_s_sleep(2);
        else for (int k = 0; k < 8; k++) __builtin_amdgcn_s_sleep(127);
      }
      if (lane == 0) __hip_atomic_store(&g_hCmd, g, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      for (;;) {
        g = waveUniform64(__hip_atomic_load(&g_hCmd, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (g != seen) break;
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the round state written before the command was published
    seen = g;
    unsigned int op = (unsigned int)(seen & 255);
    if (d.progress && threadIdx.x == 0 && blockIdx.x < 40) d.progress[16 + blockIdx.x] = (int)((seen >> 8) * 16 + op);
    if (op == OP_HELPERS_EXIT) return;
    if (op == OP_SCAN) {
      ScanArgs a = helpArgs<ScanArgs>(b);
      unsigned long long v = scanPart(d, a, tid, nthreads);
      if (lane == 0 && v != ~0ull) __hip_atomic_fetch_min(&g_hMin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (op == OP_FAIR) {
      FairArgs a = helpArgs<FairArgs>(b);
      int v = fairPart(d, a, tid, nthreads);
      if (lane == 0 && v >= 0) __hip_atomic_fetch_max(&g_hMax, (unsigned long long)(v + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (op == OP_SCANFAIR) {
#ifdef HELP_TRACE
      const int tcls = (int)blockIdx.x == 1 ? 1 : ((int)blockIdx.x == (H + 1) / 2 ? 2 : ((int)blockIdx.x == H ? 3 : 0));
      const int tgen = (int)(seen >> 8);
      if (tcls && threadIdx.x == 0) { TRACE_ADD(tcls, 0, tgen); atomicAdd(&g_traceSum[56 + tcls], 1ull); }
#endif
      ScanArgs a = helpArgs<ScanArgs>(b);
      FairArgs f = helpArgs<FairArgs>(b, HELP_ARGS2);
#ifdef HELP_TRACE
      if (tcls && threadIdx.x == 0) TRACE_ADD(tcls, 1, tgen);
#endif
      unsigned long long v = scanPart(d, a, tid, nthreads);
#ifdef HELP_TRACE
      if (tcls && threadIdx.x == 0) TRACE_ADD(tcls, 2, tgen);
#endif
      int w = fairPart(d, f, tid, nthreads);
#ifdef HELP_TRACE
      if (tcls && threadIdx.x == 0) TRACE_ADD(tcls, 3, tgen);
#endif
      if (lane == 0 && v != ~0ull) __hip_atomic_fetch_min(&g_hMin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (lane == 0 && w >= 0) __hip_atomic_fetch_max(&g_hMax, (unsigned long long)(w + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (op == OP_BULKW) {
      BulkWArgs a = helpArgs<BulkWArgs>(b);
      Dev& dm = const_cast<Dev&>(d);
      for (int i = tid; i < a.n; i += nthreads) bulkElem(dm, a.kind, i);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // this workgroup's writes before its completion count
    }
    else if (op == OP_WIDE) {
      BulkWArgs a = helpArgs<BulkWArgs>(b);
      Dev& dm = const_cast<Dev&>(d);
      for (int i = tid; i < a.n; i += nthreads) wideBulkAny(dm, a.kind, i);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    }
    if (lane == 0) {
      unsigned int before = __hip_atomic_fetch_add(&g_hArrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (before == (unsigned)(nw - 1)) {  // last wave of the workgroup: forward the folded result, reset the LDS words for the next command
        unsigned long long mn = __hip_atomic_load(&g_hMin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        unsigned long long mx = __hip_atomic_load(&g_hMax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&g_hMin, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&g_hMax, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&g_hArrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        HelpSlot* sl = &b->slot[blockIdx.x - 1];
        __hip_atomic_store(&sl->mn, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sl->mx, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sl->gen, seen >> 8, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);   // completion: this workgroup's results (and, for the bulk ops, its writes) are visible before it
#ifdef HELP_TRACE
        if (op == OP_SCANFAIR) { const int tc2 = (int)blockIdx.x == 1 ? 1 : ((int)blockIdx.x == (H + 1) / 2 ? 2 : ((int)blockIdx.x == H ? 3 : 0)); if (tc2) TRACE_ADD(tc2, 4, (int)(seen >> 8)); }
#endif
      }
    }
  }
}
