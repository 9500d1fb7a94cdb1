// armada_sched_mgpu.hip — third translation unit of libarmada_sched.so: grid kernels outside the round kernel's code object — the ones that produce and consume the words of the
// multi-GPU exchanges, since round 4 the submit check's gang units, one workgroup per unit (submit_gang.h), and the literal batched first fit, one wave per
// query over a per-call index (kernels_fit_lit.h): one element per thread over queries / result rows / nodes / jobs, all plain coalesced streaming
// (the per-element logic is mgpu.h, shared with the CPU build of the tests; launched by plat_hip.inc through the extern "C" wrappers).  A separate code object so that nothing here moves the
// round kernel's code (k_control is placement-sensitive: DESIGN.md 9).
#include <hip/hip_runtime.h>
#include <stdint.h>
#define MGPU_FN __device__ static inline
#define MGPU_ADD64(p, v) atomicAdd((unsigned long long*)(p), (unsigned long long)(v))
#define MGPU_ADD32(p, v) atomicAdd((int*)(p), (int)(v))
#define MGPU_OR8(p) (*(volatile uint8_t*)(p) = 1)   // every writer stores the same value
#include "mgpu.h"

#define MG_THREADS 256
static inline int mgBlocks(long long n) { return (int)((n + MG_THREADS - 1) / MG_THREADS); }
#define MG_IDX() ((long long)blockIdx.x * MG_THREADS + threadIdx.x)

// one atomic per wave: ballot + popcount (a counter every thread bumps serialises the whole grid on one address)
__device__ static inline void waveCount(int32_t* counter, bool pred) {
  unsigned long long m = __ballot(pred);
  if (m && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(counter, (int)__builtin_popcountll(m));
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_pack(Dev d, GlobalKeyLayout L, int level, const unsigned long long* keys, const int32_t* slot, int nq, long long* out, int32_t* bad) {
  long long i = MG_IDX();
  if (i < nq) out[i] = mgpuPackQuery(d, L, level, keys[(size_t)slot[i] * FIT_OSTR], bad);   // (k_fit_batch's result words are FIT_OSTR apart)
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_delta(Dev d, long long* buf, int ns, int np) {
  long long i = MG_IDX();
  if (i < ns) mgpuDeltaScheduled(d, buf, (int)i);
  else if (i < (long long)ns + np) mgpuDeltaPreempted(d, buf, (int)(i - ns));
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_free_init(Dev d, long long* freeC) {
  long long n = MG_IDX();
  if (n < d.cfg.N) mgpuFreeInit(d, freeC, (int)n);
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_own(Dev d, long long* freeC, uint8_t* ownPre, int ns, int np) {
  long long i = MG_IDX();
  if (i < ns) mgpuFreeOwnScheduled(d, freeC, (int)i);
  else if (i < (long long)ns + np) mgpuOwnPreempted(d, ownPre, (int)(i - ns));
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_foreign(Dev d, const long long* red, const uint8_t* ownPre, long long* freeC) {
  long long j = MG_IDX();
  if (j < d.cfg.M) mgpuFreeForeignPreempted(d, red, ownPre, freeC, (int)j);
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_conflict(Dev d, const long long* red, const long long* freeC, uint8_t* conflict, int32_t* counts) {
  long long n = MG_IDX();
  bool over = n < d.cfg.N && mgpuConflict(d, red, freeC, conflict, (int)n);
  waveCount(counts + 0, over);
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_gang(Dev d, const long long* red, const uint8_t* conflict, uint8_t* gangReplay) {
  long long j = MG_IDX();
  if (j < d.cfg.M) mgpuGangConflict(d, red, conflict, gangReplay, (int)j);
}
__global__ __launch_bounds__(MG_THREADS) void k_mgpu_outcome(Dev d, const long long* red, const uint8_t* conflict, const uint8_t* gangReplay, int32_t* node, int32_t* prio, uint8_t* replay, int32_t* counts) {
  long long j = MG_IDX();
  int k = j < d.cfg.M ? mgpuJobOutcome(d, red, conflict, gangReplay, node, prio, replay, (int)j) : 0;
  waveCount(counts + 1, k == 1); waveCount(counts + 2, k == 2); waveCount(counts + 3, k == 3);
}

extern "C" int asched_internal_mgpu_pack(const Dev* d, const GlobalKeyLayout* L, int level, const unsigned long long* keys, const int32_t* slot, int nq, long long* out, int32_t* bad, hipStream_t s) {
  if (nq > 0) hipLaunchKernelGGL(k_mgpu_pack, dim3(mgBlocks(nq)), dim3(MG_THREADS), 0, s, *d, *L, level, keys, slot, nq, out, bad);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_mgpu_delta(const Dev* d, long long* buf, int ns, int np, hipStream_t s) {
  if (ns + np > 0) hipLaunchKernelGGL(k_mgpu_delta, dim3(mgBlocks((long long)ns + np)), dim3(MG_THREADS), 0, s, *d, buf, ns, np);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// freeC [N*R], ownPre [M], conflict [N], gangReplay [max(G,1)], counts [4]: zeroed by the caller
extern "C" int asched_internal_mgpu_resolve(const Dev* d, const long long* red, long long* freeC, uint8_t* ownPre, uint8_t* conflict, uint8_t* gangReplay,
                                            int32_t* node, int32_t* prio, uint8_t* replay, int32_t* counts, int ns, int np, hipStream_t s) {
  int N = d->cfg.N, M = d->cfg.M;
  if (N > 0) hipLaunchKernelGGL(k_mgpu_free_init, dim3(mgBlocks(N)), dim3(MG_THREADS), 0, s, *d, freeC);
  if (ns + np > 0) hipLaunchKernelGGL(k_mgpu_own, dim3(mgBlocks((long long)ns + np)), dim3(MG_THREADS), 0, s, *d, freeC, ownPre, ns, np);
  if (M > 0) hipLaunchKernelGGL(k_mgpu_foreign, dim3(mgBlocks(M)), dim3(MG_THREADS), 0, s, *d, red, ownPre, freeC);
  if (N > 0) hipLaunchKernelGGL(k_mgpu_conflict, dim3(mgBlocks(N)), dim3(MG_THREADS), 0, s, *d, red, freeC, conflict, counts);
  if (M > 0) hipLaunchKernelGGL(k_mgpu_gang, dim3(mgBlocks(M)), dim3(MG_THREADS), 0, s, *d, red, conflict, gangReplay);
  if (M > 0) hipLaunchKernelGGL(k_mgpu_outcome, dim3(mgBlocks(M)), dim3(MG_THREADS), 0, s, *d, red, conflict, gangReplay, node, prio, replay, counts);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ submit check: gang units, one workgroup each (submit_gang.h)
#define SG_FN __device__ static inline
#define SG_TID ((int)threadIdx.x)
#define SG_NT ((int)blockDim.x)
#define SG_SYNC() __syncthreads()
struct SgShared;
__device__ static inline unsigned long long sgWgMin(SgShared& s, unsigned long long v);
#define SG_WGMIN(s, v) sgWgMin(s, v)
#include "submit_gang.h"
__device__ static inline unsigned long long sgWgMin(SgShared& s, unsigned long long v) {
  for (int off = 32; off; off >>= 1) { unsigned long long o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  __syncthreads();                                   // (the previous reduction's readers are done with wmin)
  if ((threadIdx.x & 63) == 0) s.wmin[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = s.wmin[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = s.wmin[w] < r ? s.wmin[w] : r;
  return r;
}
#define SG_THREADS 256
__global__ __launch_bounds__(SG_THREADS) void k_submit_gangs(Dev d, const int32_t* off, const int32_t* jobs, int nu, int32_t* out) {
  extern __shared__ uint32_t sgBits[];               // a bit per node: an earlier member of the unit in flight sits there
  __shared__ SgShared s;
  for (int i = threadIdx.x; i < (d.cfg.N + 31) / 32; i += SG_THREADS) sgBits[i] = 0;
  __syncthreads();
  for (int u = blockIdx.x; u < nu; u += gridDim.x) submitGangUnit(d, jobs + off[u], off[u + 1] - off[u], s, sgBits, out + 4 * (size_t)u);
}
extern "C" int asched_internal_submit_gangs(const Dev* d, const int32_t* off, const int32_t* jobs, int nu, int32_t* out, hipStream_t st) {
  if (nu <= 0) return 0;
  size_t lds = (size_t)((d->cfg.N + 31) / 32) * 4;
  hipLaunchKernelGGL(k_submit_gangs, dim3(nu < 4096 ? nu : 4096), dim3(SG_THREADS), lds, st, *d, off, jobs, nu, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the evicted table by rank (replay_rank.h): check (one thread) -> rank (one thread per evicted-list position) -> finish (one thread).  replayPending == 2 between the
// check and the finish says "by rank"; the round kernel never sees it (the three launches sit back to back on the handle's stream, in front of CMD_PASS1 / CMD_PASS2).
#include "replay_rank.h"
__global__ void k_replay_check(Dev d, int n) { if (threadIdx.x == 0 && blockIdx.x == 0 && rrOk(d, n)) d.rs->replayPending = 2; }
__global__ __launch_bounds__(MG_THREADS) void k_replay_rank(Dev d, int n) {
  if (d.rs->replayPending != 2) return;
  long long i = MG_IDX();
  if (i < n) rrElem(d, (int)i);
}
__global__ void k_replay_fin(Dev d, int n, int keepPending) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (d.rs->replayPending == 2) rrFinish(d, n);
  else if (!keepPending) d.rs->replayPending = 0;   // (pass 2 has no lazy replay: CMD_PASS2 walks when the table was not built here)
}
extern "C" int asched_internal_replay_rank(const Dev* d, int n, int keepPending, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_replay_check, dim3(1), dim3(64), 0, st, *d, n);
  hipLaunchKernelGGL(k_replay_rank, dim3(mgBlocks(n)), dim3(MG_THREADS), 0, st, *d, n);
  hipLaunchKernelGGL(k_replay_fin, dim3(1), dim3(64), 0, st, *d, n, keepPending);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// uniform units: per shape the smallest key among the nodes that take at least one member, and the number of members all nodes take together (submit_gang.h)
__global__ __launch_bounds__(256) void k_fit_capacity(Dev d, const int32_t* shapes, int ns, unsigned long long* out /*[ns][FIT_OSTR]: [0] min key, [1] capacity sum*/) {
  __shared__ unsigned long long wmin[4], wsum[4];
  int n = blockIdx.x * 256 + threadIdx.x;
  for (int i = blockIdx.y; i < ns; i += gridDim.y) {
    long long cap = n < d.cfg.N ? sgNodeCapacity(d, shapes[i], n) : 0;
    unsigned long long key = cap > 0 ? d.keys[n] : ~0ull, sum = (unsigned long long)cap;
    for (int off = 32; off; off >>= 1) { unsigned long long o = __shfl_xor(key, off, 64); key = o < key ? o : key; sum += __shfl_xor(sum, off, 64); }
    if ((threadIdx.x & 63) == 0) { wmin[threadIdx.x >> 6] = key; wsum[threadIdx.x >> 6] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long m = wmin[0], t = wsum[0];
      for (int w = 1; w < 4; w++) { m = wmin[w] < m ? wmin[w] : m; t += wsum[w]; }
      if (m != ~0ull) atomicMin(&out[(size_t)i * FIT_OSTR], m);
      if (t) atomicAdd(&out[(size_t)i * FIT_OSTR + 1], t);
    }
    __syncthreads();
  }
}
extern "C" int asched_internal_fit_capacity(const Dev* d, const int32_t* shapes, int ns, unsigned long long* out, hipStream_t st) {
  if (ns <= 0 || d->cfg.N <= 0) return 0;
  int tiles = (d->cfg.N + 255) / 256;
  int ysplit = ns < 1 ? 1 : (ns < (2048 + tiles - 1) / tiles ? ns : (2048 + tiles - 1) / tiles);
  hipLaunchKernelGGL(k_fit_capacity, dim3(tiles, ysplit < 1 ? 1 : ysplit), dim3(256), 0, st, *d, shapes, ns, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ literal batched first fit (kernels_fit_lit.h)
#define FL_FN __device__ static inline
#define FL_LANE ((int)(threadIdx.x & 63))
#define FL_NL 64
#define FL_BALLOT(p) ((unsigned long long)__ballot(p))
#define FL_SHFL(v, l) __shfl(v, l, 64)
#define FL_UNROLL _Pragma("unroll")
#include "kernels_fit_lit.h"
__global__ __launch_bounds__(MG_THREADS) void k_fit_lit_fill(Dev d, const int32_t* nodeType, int level, FlPair* a, int nb2) {
  long long i = MG_IDX();
  if (i < nb2) flFill(d, nodeType, level, a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_fit_lit_step(FlPair* a, int j, int k) {
  unsigned i = blockIdx.x * MG_THREADS + threadIdx.x;
  unsigned l = i ^ (unsigned)j;
  if (l > i) {
    FlPair x = a[i], y = a[l];
    bool up = (i & (unsigned)k) == 0;
    if (up ? flPairLess(y, x) : flPairLess(x, y)) { a[i] = y; a[l] = x; }
  }
}
// the in-LDS part of the network (k_bitonic_tile's scheme on 16-byte records): every (k, j) step with j < FL_TILE for one tile of FL_TILE records
__global__ __launch_bounds__(1024) void k_fit_lit_tile(FlPair* a, int kStart, int kEnd, int jStart) {
  __shared__ FlPair t[FL_TILE];
  unsigned base = blockIdx.x * (unsigned)FL_TILE;
  for (int i = threadIdx.x; i < FL_TILE; i += 1024) t[i] = a[base + i];
  __syncthreads();
  for (int k = kStart; k <= kEnd; k <<= 1) {
    for (int j = (k == kStart ? jStart : k >> 1); j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < FL_TILE; i += 1024) {
        unsigned l = (unsigned)i ^ (unsigned)j;
        if (l > (unsigned)i) {
          FlPair x = t[i], y = t[l];
          bool up = ((base + i) & (unsigned)k) == 0;
          if (up ? flPairLess(y, x) : flPairLess(x, y)) { t[i] = y; t[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < FL_TILE; i += 1024) a[base + i] = t[i];
}
__global__ __launch_bounds__(MG_THREADS) void k_fit_lit_finish(Dev d, FitLitIdx x, const FlPair* a) {
  long long i = MG_IDX();
  if (i < d.cfg.N) flFinish(d, x, a, (int)i);
}
// one wave per query (a workgroup IS one wave: the queries spread over every CU and no barrier is needed); the iterator states of its node types in LDS
__global__ __launch_bounds__(64) void k_fit_lit(Dev d, FitLitIdx x, const int32_t* rows, int nq, int32_t* out) {
  __shared__ FlIt its[LIT_TMAX];
  for (int q = blockIdx.x; q < nq; q += gridDim.x) {
    int r = flQuery(d, x, rows[q], its);
    if (threadIdx.x == 0) out[q] = r;
  }
}
// a [nb2] sort scratch, nb2 a power of two >= max(N, FL_TILE); typeBeg / typeEnd zeroed by the caller
extern "C" int asched_internal_fit_lit_build(const Dev* d, const FitLitIdx* x, const int32_t* nodeType, FlPair* a, int nb2, hipStream_t st) {
  int N = d->cfg.N;
  if (N <= 0) return 0;
  hipLaunchKernelGGL(k_fit_lit_fill, dim3(mgBlocks(nb2)), dim3(MG_THREADS), 0, st, *d, nodeType, x->level, a, nb2);
  int tiles = nb2 / FL_TILE;
  hipLaunchKernelGGL(k_fit_lit_tile, dim3(tiles), dim3(1024), 0, st, a, 2, FL_TILE, 1);   // all steps with k <= FL_TILE
  for (int k = 2 * FL_TILE; k <= nb2; k <<= 1) {
    for (int j = k >> 1; j >= FL_TILE; j >>= 1) hipLaunchKernelGGL(k_fit_lit_step, dim3(mgBlocks(nb2)), dim3(MG_THREADS), 0, st, a, j, k);
    hipLaunchKernelGGL(k_fit_lit_tile, dim3(tiles), dim3(1024), 0, st, a, k, k, FL_TILE / 2);   // the remaining steps j = FL_TILE / 2 .. 1 inside tiles
  }
  hipLaunchKernelGGL(k_fit_lit_finish, dim3(mgBlocks(N)), dim3(MG_THREADS), 0, st, *d, *x, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_fit_lit_query(const Dev* d, const FitLitIdx* x, const int32_t* rows, int nq, int32_t* out, hipStream_t st) {
  if (nq <= 0 || d->cfg.N <= 0) return 0;
  hipLaunchKernelGGL(k_fit_lit, dim3(nq < 65536 ? nq : 65536), dim3(64), 0, st, *d, *x, rows, nq, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ preemption causes: the join over a round's result lists (kernels_preempt_join.h)
#define PJ_FN __device__ static inline
#define PJ_ADD32(p, v) atomicAdd((int*)(p), (int)(v))
#include "kernels_preempt_join.h"
// exclusive prefix sum of one value per thread over the workgroup of MG_THREADS (4 waves); *total: the workgroup's sum, the same in every thread
__device__ static inline int pjBlockExclusive(int v, int* wsum /*[4] LDS*/, int* total) {
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6, inc = v;
  for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
  __syncthreads();                                   // (the previous scan's readers are done with wsum)
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < MG_THREADS / 64; k++) { int s = wsum[k]; if (k < w) before += s; all += s; }
  *total = all;
  return before + inc - v;
}
__global__ __launch_bounds__(MG_THREADS) void k_pj_count(PjArgs a) {
  long long i = MG_IDX();
  if (i < a.ns) pjCount(a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_pj_tile_sum(PjArgs a) {
  __shared__ int wsum[MG_THREADS / 64];
  long long base = (long long)blockIdx.x * PJ_TILE + (long long)threadIdx.x * 4;
  int v = 0, total;
  for (int k = 0; k < 4; k++) if (base + k < a.N) v += a.cnt[base + k];
  (void)pjBlockExclusive(v, wsum, &total);
  if (threadIdx.x == 0) a.tileSum[blockIdx.x] = total;
}
// one workgroup: the tile sums become tile offsets, MG_THREADS at a time behind a carry; off[N] = the number of candidates
__global__ __launch_bounds__(MG_THREADS) void k_pj_tile_scan(PjArgs a, int tiles) {
  __shared__ int wsum[MG_THREADS / 64];
  int carry = 0;
  for (int base = 0; base < tiles; base += MG_THREADS) {
    int t = base + (int)threadIdx.x, v = t < tiles ? a.tileSum[t] : 0, total;
    int ex = pjBlockExclusive(v, wsum, &total);
    if (t < tiles) a.tileSum[t] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) a.off[a.N] = carry;
}
__global__ __launch_bounds__(MG_THREADS) void k_pj_tile_apply(PjArgs a) {
  __shared__ int wsum[MG_THREADS / 64];
  long long base = (long long)blockIdx.x * PJ_TILE + (long long)threadIdx.x * 4;
  int c[4], v = 0, total;
  for (int k = 0; k < 4; k++) { c[k] = base + k < a.N ? a.cnt[base + k] : 0; v += c[k]; }
  int run = a.tileSum[blockIdx.x] + pjBlockExclusive(v, wsum, &total);
  for (int k = 0; k < 4; k++) if (base + k < a.N) { a.off[base + k] = run; a.cursor[base + k] = run; run += c[k]; }
}
__global__ __launch_bounds__(MG_THREADS) void k_pj_scatter(PjArgs a) {
  long long i = MG_IDX();
  if (i < a.ns) pjScatter(a, (int)i);
}
// (the number of candidates is on the device only: a grid for all ns entries, the slots behind off[N] return)
__global__ __launch_bounds__(MG_THREADS) void k_pj_rank(PjArgs a) {
  long long k = MG_IDX();
  if (k < a.ns && k < a.off[a.N]) pjRank(a, (int)k);
}
__global__ __launch_bounds__(MG_THREADS) void k_pj_gather(Dev d, PjArgs a) {
  long long i = MG_IDX();
  if (i < a.np) pjGather(d, a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_pj_cause(PjArgs a) {
  long long i = MG_IDX();
  if (i < a.np) pjCause(a, (int)i);
}
// cnt [N + 1] and info [2] zeroed by the caller
extern "C" int asched_internal_preempt_join(const Dev* d, const PjArgs* a, hipStream_t st) {
  int tiles = pjTiles(a->N);
  if (a->ns > 0 && a->N > 0) hipLaunchKernelGGL(k_pj_count, dim3(mgBlocks(a->ns)), dim3(MG_THREADS), 0, st, *a);
  if (tiles > 0) hipLaunchKernelGGL(k_pj_tile_sum, dim3(tiles), dim3(MG_THREADS), 0, st, *a);
  hipLaunchKernelGGL(k_pj_tile_scan, dim3(1), dim3(MG_THREADS), 0, st, *a, tiles);
  if (tiles > 0) hipLaunchKernelGGL(k_pj_tile_apply, dim3(tiles), dim3(MG_THREADS), 0, st, *a);
  if (a->ns > 0 && a->N > 0) {
    hipLaunchKernelGGL(k_pj_scatter, dim3(mgBlocks(a->ns)), dim3(MG_THREADS), 0, st, *a);
    hipLaunchKernelGGL(k_pj_rank, dim3(mgBlocks(a->ns)), dim3(MG_THREADS), 0, st, *a);
  }
  if (a->np > 0) {
    if (a->fromRound) hipLaunchKernelGGL(k_pj_gather, dim3(mgBlocks(a->np)), dim3(MG_THREADS), 0, st, *d, *a);
    hipLaunchKernelGGL(k_pj_cause, dim3(mgBlocks(a->np)), dim3(MG_THREADS), 0, st, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ the evictor report of a round's phase 1 (kernels_evict_report.h)
#define EVR_FN __device__ static inline
#include "kernels_evict_report.h"
static_assert(EVR_TILE == MG_THREADS, "the queue pass holds one entry of its tile per thread");
// runs of neighbouring lanes with the same key inside a wave.  head: this lane starts a run.  *start: the first lane of this lane's run; returns whether it is the last
__device__ static inline bool evrRun(bool head, int* start) {
  int lane = threadIdx.x & 63;
  unsigned long long heads = __ballot(head) | 1ull;
  *start = 63 - __builtin_clzll(heads & (lane == 63 ? ~0ull : (2ull << lane) - 1));
  return lane == 63 || ((heads >> (lane + 1)) & 1);
}
__global__ __launch_bounds__(MG_THREADS) void k_evr_jobs(Dev d, EvrArgs a) {
  long long i = MG_IDX();
  int lane = threadIdx.x & 63, n = -1, reason = 0, ev = 0;
  if (i < a.M) evrJobTerms(d, a, (int)i, &n, &reason, &ev);
  int cnt = n >= 0 ? 1 : 0, prev = __shfl_up(n, 1, 64), start;
  bool last = evrRun(lane == 0 || prev != n, &start);
  for (int o = 1; o < 64; o <<= 1) {   // segmented inclusive scan: the last lane of a run ends up with the run's sums
    int c2 = __shfl_up(cnt, o, 64), r2 = __shfl_up(reason, o, 64), e2 = __shfl_up(ev, o, 64);
    if (lane - o >= start) { cnt += c2; reason |= r2; ev += e2; }
  }
  if (last && n >= 0) {
    atomicAdd(a.nodeJobs + n, cnt);
    if (reason) atomicOr(a.nodeOr + n, reason);
    if (ev) atomicAdd(a.nodeEvicted + n, ev);
  }
}
__global__ __launch_bounds__(MG_THREADS) void k_evr_nodes(EvrArgs a) {
  __shared__ int wsum[MG_THREADS / 64];
  long long n = MG_IDX();
  int aff = n < a.N ? evrNode(a, (int)n) : 0;
  unsigned long long m = __ballot(aff);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (int)__builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) { int s = 0; for (int k = 0; k < MG_THREADS / 64; k++) s += wsum[k]; if (s) atomicAdd(a.affected, s); }
}
__global__ __launch_bounds__(MG_THREADS) void k_evr_queues(Dev d, EvrArgs a) {
  constexpr int NW = MG_THREADS / 64;
  __shared__ int qEnds[2], headQ[NW], tailQ[NW];
  __shared__ long long tailSum[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long g = MG_IDX(); g <= a.Q; g += (long long)gridDim.x * MG_THREADS) evrCopyOff(d, a, (int)g);
  const long long base = (long long)blockIdx.x * EVR_TILE;
  if (base >= a.n1) return;   // (the workgroup of an empty list: only the copy above)
  const long long p = base + threadIdx.x;
  const bool valid = p < a.n1;
  if (threadIdx.x < 2) { long long e = threadIdx.x == 0 ? base : (base + EVR_TILE <= a.n1 ? base + EVR_TILE : a.n1) - 1; qEnds[threadIdx.x] = evrQueueOf(d.evOff, (int)e, 0, a.Q - 1); }
  __syncthreads();
  int q = -1, j = 0;
  if (valid) { q = qEnds[0] == qEnds[1] ? qEnds[0] : evrQueueOf(d.evOff, (int)p, qEnds[0], qEnds[1]); j = d.evList[p]; evrGather(d, a, (int)p); }
  int prev = __shfl_up(q, 1, 64), start;
  (void)evrRun(lane == 0 || prev != q, &start);
  if (lane == 0) headQ[w] = q;
  if (lane == 63) tailQ[w] = q;
  __syncthreads();
  // the lane that ends its queue's run inside the tile: the next entry is another queue's, or there is none in this tile
  int next = __shfl_down(q, 1, 64);
  if (lane == 63) next = w + 1 < NW ? headQ[w + 1] : -1;
  const bool ends = valid && next != q, fromLane0 = start == 0;
  for (int r = 0; r < a.R; r++) {
    long long v = valid ? evrReqCol(d, j, r) : 0;
    for (int o = 1; o < 64; o <<= 1) { long long t = __shfl_up(v, o, 64); if (lane - o >= start) v += t; }
    if (lane == 63) tailSum[w] = v;   // the sum of the wave's trailing run
    __syncthreads();
    if (ends) {
      // (evList is sorted by queue: equal queues at the ends of two neighbouring waves are ONE run, and a wave whose head and tail are both q holds nothing else)
      if (fromLane0) for (int k = w - 1; k >= 0 && tailQ[k] == q; k--) { v += tailSum[k]; if (headQ[k] != q) break; }   // the run began in an earlier wave of the tile
      if (v) atomicAdd((unsigned long long*)(a.qRes + (size_t)q * a.R + r), (unsigned long long)v);
    }
    __syncthreads();   // (tailSum is written again for the next column)
  }
}
extern "C" int asched_internal_evict_report(const Dev* d, const EvrArgs* a, int pass, hipStream_t st) {
  if (pass == EVR_PASS_JOBS) hipLaunchKernelGGL(k_evr_jobs, dim3(mgBlocks(a->M)), dim3(MG_THREADS), 0, st, *d, *a);
  else if (pass == EVR_PASS_NODES) hipLaunchKernelGGL(k_evr_nodes, dim3(mgBlocks(a->N)), dim3(MG_THREADS), 0, st, *a);
  else hipLaunchKernelGGL(k_evr_queues, dim3(a->n1 > 0 ? (a->n1 + EVR_TILE - 1) / EVR_TILE : 1), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ the run-state patch of the resident job table (kernels_jobs_patch.h)
#define JP_FN __device__ static inline
#include "kernels_jobs_patch.h"
__global__ __launch_bounds__(MG_THREADS) void k_jp_scatter(Dev d, JpArgs a) {
  long long i = MG_IDX();
  if (i < a.nb2) jpScatter(d, a, (int)i);
}
// one compare-exchange step of the bitonic network in HBM: distance j, direction by bit k of the position
__global__ __launch_bounds__(MG_THREADS) void k_jp_step(JpKey* a, int nb2, int j, int k) {
  unsigned i = blockIdx.x * MG_THREADS + threadIdx.x;
  unsigned l = i ^ (unsigned)j;
  if (i < (unsigned)nb2 && l > i) {
    JpKey x = a[i], y = a[l];
    bool up = (i & (unsigned)k) == 0;
    if (up ? jpLess(y, x) : jpLess(x, y)) { a[i] = y; a[l] = x; }
  }
}
// the in-LDS part of the network (k_fit_lit_tile's scheme on 40-byte records): every (k, j) step with j < JP_TILE for one tile of JP_TILE records.  A thread owns
// the pairs (i, i ^ j) with bit j of i clear: every record is touched by exactly one thread per step
__global__ __launch_bounds__(MG_THREADS) void k_jp_tile(JpKey* a, int kStart, int kEnd, int jStart) {
  __shared__ JpKey t[JP_TILE];
  const unsigned base = blockIdx.x * (unsigned)JP_TILE;
  for (int i = threadIdx.x; i < JP_TILE; i += MG_THREADS) t[i] = a[base + i];
  __syncthreads();
  for (int k = kStart; k <= kEnd; k <<= 1) {
    for (int j = (k == kStart ? jStart : k >> 1); j > 0; j >>= 1) {
      for (int p = threadIdx.x; p < JP_TILE / 2; p += MG_THREADS) {
        unsigned i = (((unsigned)p & ~((unsigned)j - 1)) << 1) | ((unsigned)p & ((unsigned)j - 1)), l = i | (unsigned)j;   // the p-th position with bit j clear
        JpKey x = t[i], y = t[l];
        bool up = ((base + i) & (unsigned)k) == 0;
        if (up ? jpLess(y, x) : jpLess(x, y)) { t[i] = y; t[l] = x; }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < JP_TILE; i += MG_THREADS) a[base + i] = t[i];
}
__global__ __launch_bounds__(MG_THREADS) void k_jp_merge(Dev d, JpArgs a) {
  long long i = MG_IDX();
  if (i < (long long)a.nT + a.nKept + a.n) jpMerge(d, a, i);
}
extern "C" int asched_internal_jp_scatter(const Dev* d, const JpArgs* a, hipStream_t st) {
  if (a->nb2 > 0) hipLaunchKernelGGL(k_jp_scatter, dim3(mgBlocks(a->nb2)), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// a->keys [a->nb2], nb2 a power of two >= JP_TILE
extern "C" int asched_internal_jp_sort(const JpArgs* a, hipStream_t st) {
  const int nb2 = a->nb2, tiles = nb2 / JP_TILE;
  if (tiles <= 0 || (nb2 & (nb2 - 1)) || nb2 % JP_TILE) return -1;
  hipLaunchKernelGGL(k_jp_tile, dim3(tiles), dim3(MG_THREADS), 0, st, a->keys, 2, JP_TILE, 1);   // all steps with k <= JP_TILE
  for (long long k = 2ll * JP_TILE; k <= nb2; k <<= 1) {
    for (long long j = k >> 1; j >= JP_TILE; j >>= 1) hipLaunchKernelGGL(k_jp_step, dim3(mgBlocks(nb2)), dim3(MG_THREADS), 0, st, a->keys, nb2, (int)j, (int)k);
    hipLaunchKernelGGL(k_jp_tile, dim3(tiles), dim3(MG_THREADS), 0, st, a->keys, (int)k, (int)k, JP_TILE / 2);   // the remaining steps j = JP_TILE / 2 .. 1 inside tiles
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_jp_merge(const Dev* d, const JpArgs* a, hipStream_t st) {
  const long long work = (long long)a->nT + a->nKept + a->n;
  if (work > 0) hipLaunchKernelGGL(k_jp_merge, dim3(mgBlocks(work)), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ queue priorities of resident jobs change (kernels_jobs_reprioritise.h)
// scatter + keys: one thread per entry, plain stores; the remove, the sort and the merge by rank are the patch's (plat_compact, asched_internal_jp_sort / _jp_merge on JrArgs::p)
#include "kernels_jobs_reprioritise.h"
__global__ __launch_bounds__(MG_THREADS) void k_jr_scatter(Dev d, JrArgs a) {
  long long i = MG_IDX();
  if (i < a.p.nb2) jrScatter(d, a, (int)i);
}
extern "C" int asched_internal_jr_scatter(const Dev* d, const JrArgs* a, hipStream_t st) {
  if (a->p.nb2 > 0) hipLaunchKernelGGL(k_jr_scatter, dim3(mgBlocks(a->p.nb2)), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ a round's result applied to the resident jobs (kernels_round_commit.h)
// scatter + keys: one thread per entry, the entry read from the uploaded extras or from the lists the round left (neighbouring threads read neighbouring words), plain
// stores; the remove, the sort and the merge by rank are the patch's (plat_compact, asched_internal_jp_sort / _jp_merge on RcArgs::p)
#include "kernels_round_commit.h"
__global__ __launch_bounds__(MG_THREADS) void k_rc_scatter(Dev d, RcArgs a) {
  long long i = MG_IDX();
  if (i < a.p.nb2) rcScatter(d, a, (int)i);
}
extern "C" int asched_internal_rc_scatter(const Dev* d, const RcArgs* a, hipStream_t st) {
  if (a->p.nb2 > 0) hipLaunchKernelGGL(k_rc_scatter, dim3(mgBlocks(a->p.nb2)), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ retried jobs change class and request in place (kernels_jobs_respec.h)
// one thread per entry, plain stores: every row is named at most once and a record's source row is named by no entry
#include "kernels_jobs_respec.h"
__global__ __launch_bounds__(MG_THREADS) void k_js_scatter(Dev d, JsArgs a) {
  long long i = MG_IDX();
  if (i < a.n) jsScatter(d, a, (int)i);
}
extern "C" int asched_internal_js_scatter(const Dev* d, const JsArgs* a, hipStream_t st) {
  if (a->n > 0) hipLaunchKernelGGL(k_js_scatter, dim3(mgBlocks(a->n)), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ newly submitted jobs behind the resident job table (kernels_jobs_append.h)
// row fill + keys; the sort and the merge by rank are the patch's (asched_internal_jp_sort / _jp_merge on JaArgs::p)
#include "kernels_jobs_append.h"
__global__ __launch_bounds__(MG_THREADS) void k_ja_fill(Dev d, JaArgs a) {
  long long i = MG_IDX();
  if (i < a.nb2) jaFill(d, a, (int)i);
}
extern "C" int asched_internal_ja_fill(const Dev* d, const JaArgs* a, hipStream_t st) {
  if (a->nb2 > 0) hipLaunchKernelGGL(k_ja_fill, dim3(mgBlocks(a->nb2)), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ new scheduling-key shapes join the shape mask (kernels_shapes_append.h)
// one wave per 64-node output word, the workgroup's four waves take four consecutive words.  w is wave-uniform, so every lane of a wave takes the same branches and
// the ballot sees all 64 lanes; a lane's totals are loaded once and the new rows are looped inside
#define SA_FN __device__ static inline
#include "kernels_shapes_append.h"
__global__ __launch_bounds__(MG_THREADS) void k_sa_mask(SaArgs a) {
  const long long t = MG_IDX();
  const int w = (int)(t >> 6), lane = (int)(threadIdx.x & 63);
  if (w >= a.W) return;
  const int n = 64 * w + lane;
  const bool live = n < a.N;
  int64_t tot[MAXR];
  if (live) saLoad(a, n, tot);
  for (int row = 0; row < a.rows; row++) {
    const uint64_t cw = a.classMask[(size_t)a.rowClass[row] * a.W + w];
    const bool b = live && saBit(a, row, cw, lane, tot);
    const unsigned long long word = __ballot(b);
    if (lane == 0) a.outMask[(size_t)a.rowOut[row] * a.W + w] = word;
  }
}
extern "C" int asched_internal_sa_mask(const SaArgs* a, hipStream_t st) {
  if (a->rows > 0 && a->W > 0) hipLaunchKernelGGL(k_sa_mask, dim3(mgBlocks((long long)a->W * 64)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ new requirement classes join the class mask (kernels_req_classes_append.h)
// one wave per 64-node word, the workgroup's four waves take four consecutive words.  w is wave-uniform, so the loop over the new classes and the loop over a class's
// node types are uniform and their loads are the same address in every lane; a lane keeps only its own bit of each word
#define CA_FN __device__ static inline
#include "kernels_req_classes_append.h"
__global__ __launch_bounds__(MG_THREADS) void k_ca_rows(CaArgs a) {
  const long long t = MG_IDX();
  const int w = (int)(t >> 6), lane = (int)(threadIdx.x & 63);
  if (w >= a.W) return;
  const int n = 64 * w + lane;
  uint64_t acc = 0;
  for (int c = 0; c < a.dC; c++) {
    const uint64_t word = caWord(a, c, w);
    if (lane == 0) a.outMask[(size_t)(a.C0 + c) * a.W + w] = word;
    acc |= caBit(a, c, word, lane);
  }
  if (a.nodeCls && n < a.N) a.nodeCls[n] |= acc;
}
extern "C" int asched_internal_ca_rows(const CaArgs* a, hipStream_t st) {
  if (a->dC > 0 && a->W > 0) hipLaunchKernelGGL(k_ca_rows, dim3(mgBlocks((long long)a->W * 64)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ dead shapes and classes leave the resident tables (kernels_shapes_compact.h)
// k_sc_rows: SC_RPB rows to a workgroup, thread t takes rows base + t, base + t + 256, ... (coalesced); the three maps from LDS where the launcher found that they fit
// (a.staged: uniform over the grid, so every thread of a workgroup reaches the barrier or none does), else from global memory.  k_sc_gather: one thread per output
// word.  k_sc_clsbits: one thread per node
#define SC_FN __device__ static inline
#include "kernels_shapes_compact.h"
__global__ __launch_bounds__(MG_THREADS) void k_sc_rows(ScArgs a) {
  __shared__ int32_t sS[SC_LDS_CAP], sF[SC_LDS_CAP], sC[SC_LDS_CAP];
  const int32_t* mS = a.shapeNew; const int32_t* mF = a.fitNew; const int32_t* mC = a.clsNew;
  if (a.staged) {
    for (int i = threadIdx.x; i < a.S0 && i < SC_LDS_CAP; i += MG_THREADS) sS[i] = a.shapeNew[i];
    if (a.fitNew) for (int i = threadIdx.x; i < a.F0 && i < SC_LDS_CAP; i += MG_THREADS) sF[i] = a.fitNew[i];
    if (a.clsNew) for (int i = threadIdx.x; i < a.C0 && i < SC_LDS_CAP; i += MG_THREADS) sC[i] = a.clsNew[i];
    __syncthreads();
    mS = sS; if (a.fitNew) mF = sF; if (a.clsNew) mC = sC;
  }
  const long long base = (long long)blockIdx.x * SC_RPB;
  for (int k = threadIdx.x; k < SC_RPB; k += MG_THREADS) {
    const long long j = base + k;
    if (j < a.M) scRow(a, (int)j, mS, mF, mC);
  }
}
__global__ __launch_bounds__(MG_THREADS) void k_sc_gather(const uint64_t* in, uint64_t* out, const int32_t* src, int W, long long words) {
  const long long i = MG_IDX();
  if (i < words) scGather(in, out, src, W, i);
}
__global__ __launch_bounds__(MG_THREADS) void k_sc_clsbits(ScArgs a) {
  const long long n = MG_IDX();
  if (n < a.N) { const uint64_t in = a.nodeCls[n], v = scClsBits(in, a.liveCls); if (v != in) a.nodeCls[n] = v; }
}
extern "C" int asched_internal_sc_rows(const ScArgs* a, hipStream_t st) {
  ScArgs x = *a; x.staged = scFits(x);
  if (x.M > 0 && x.S0 > 0) hipLaunchKernelGGL(k_sc_rows, dim3((unsigned)(((long long)x.M + SC_RPB - 1) / SC_RPB)), dim3(MG_THREADS), 0, st, x);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_sc_gather(const ScArgs* a, hipStream_t st) {
  if (a->shapeOut && a->shapeRows > 0 && a->W > 0)
    hipLaunchKernelGGL(k_sc_gather, dim3(mgBlocks((long long)a->shapeRows * a->W)), dim3(MG_THREADS), 0, st, a->shapeIn, a->shapeOut, a->shapeSrc, a->W, (long long)a->shapeRows * a->W);
  if (a->clsOut && a->clsRows > 0 && a->W > 0)
    hipLaunchKernelGGL(k_sc_gather, dim3(mgBlocks((long long)a->clsRows * a->W)), dim3(MG_THREADS), 0, st, a->clsIn, a->clsOut, a->clsSrc, a->W, (long long)a->clsRows * a->W);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_sc_clsbits(const ScArgs* a, hipStream_t st) {
  if (a->nodeCls && a->N > 0) hipLaunchKernelGGL(k_sc_clsbits, dim3(mgBlocks(a->N)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ rows leave the resident job table (kernels_jobs_delete.h)
// mark / unmark, the three gathers (each reads the survivors' list once), the renumbering of a compacted list; the scans are plat_compact's kernels
#define JD_FN __device__ static inline
#include "kernels_jobs_delete.h"
__global__ __launch_bounds__(MG_THREADS) void k_jd_mark(JdArgs a, int value) {
  long long i = MG_IDX();
  if (i < a.n) jdMark(a, (int)i, (uint8_t)value);
}
__global__ __launch_bounds__(MG_THREADS) void k_jd_narrow(JdArgs a) {
  long long i = MG_IDX();
  if (i < a.M1) jdNarrow(a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_jd_req(JdArgs a) {
  long long e = MG_IDX();
  if (e < (long long)a.M1 * a.R) jdReq(a, e);
}
// eight consecutive lanes move one 128-byte record: a wave reads eight records, each a whole aligned line, and writes 1 KB of consecutive bytes
__global__ __launch_bounds__(MG_THREADS) void k_jd_rec(JdArgs a) {
  long long t = MG_IDX();
  if (t < (long long)a.M1 * 8) jdRec(a, t);
}
__global__ __launch_bounds__(MG_THREADS) void k_jd_remap(JdArgs a, int32_t* list, int n) {
  long long i = MG_IDX();
  if (i < n) jdRemap(a, list, (int)i);
}
extern "C" int asched_internal_jd_mark(const JdArgs* a, int value, hipStream_t st) {
  if (a->n > 0) hipLaunchKernelGGL(k_jd_mark, dim3(mgBlocks(a->n)), dim3(MG_THREADS), 0, st, *a, value);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_jd_gather(const JdArgs* a, hipStream_t st) {
  if (a->M1 <= 0) return 0;
  hipLaunchKernelGGL(k_jd_narrow, dim3(mgBlocks(a->M1)), dim3(MG_THREADS), 0, st, *a);
  hipLaunchKernelGGL(k_jd_req, dim3(mgBlocks((long long)a->M1 * a->R)), dim3(MG_THREADS), 0, st, *a);
  if (a->inRec) hipLaunchKernelGGL(k_jd_rec, dim3(mgBlocks((long long)a->M1 * 8)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_jd_remap(const JdArgs* a, int32_t* list, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_jd_remap, dim3(mgBlocks(n)), dim3(MG_THREADS), 0, st, *a, list, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ cordons and capacity changes of resident nodes (kernels_nodes_patch.h)
#define NP_FN __device__ static inline
#include "kernels_nodes_patch.h"
__global__ __launch_bounds__(MG_THREADS) void k_np_scatter(Dev d, NpArgs a) {
  long long i = MG_IDX();
  if (i < a.n) npScatter(d, a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_np_mask(Dev d, NpArgs a, long long work) {
  long long t = MG_IDX();
  if (t < work) npMaskWord(d, a, t);
}
extern "C" int asched_internal_np_scatter(const Dev* d, const NpArgs* a, hipStream_t st) {
  if (a->n > 0) hipLaunchKernelGGL(k_np_scatter, dim3(mgBlocks(a->n)), dim3(MG_THREADS), 0, st, *d, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_np_mask(const Dev* d, const NpArgs* a, hipStream_t st) {
  const long long work = (long long)(a->Cext + a->Sext + a->T) * a->nW;
  if (work > 0) hipLaunchKernelGGL(k_np_mask, dim3(mgBlocks(work)), dim3(MG_THREADS), 0, st, *d, *a, work);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ rows leave the resident node table (kernels_nodes_delete.h)
// mark / unmark, the check of the running jobs, the two gathers, the renumbering of the index order, the bit compaction of the mask rows and the remap of the running
// jobs' nodes; the scans are plat_compact's kernels
#define ND_FN __device__ static inline
#define ND_MIN32(p, v) atomicMin((p), (v))
#include "kernels_nodes_delete.h"
__global__ __launch_bounds__(MG_THREADS) void k_nd_mark(NdArgs a, int value) {
  long long i = MG_IDX();
  if (i < a.n) ndMark(a, (int)i, (uint8_t)value);
}
__global__ __launch_bounds__(MG_THREADS) void k_nd_check(NdArgs a) {
  long long j = MG_IDX();
  if (j < a.M) ndCheck(a, (int)j);
}
__global__ __launch_bounds__(MG_THREADS) void k_nd_plane(NdArgs a) {
  long long e = MG_IDX();
  if (e < (long long)a.R * a.N1) ndPlane(a, e);
}
__global__ __launch_bounds__(MG_THREADS) void k_nd_narrow(NdArgs a) {
  long long i = MG_IDX();
  if (i < a.N1) ndNarrow(a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_nd_rank(NdArgs a) {
  long long i = MG_IDX();
  if (i < a.N1) ndRank(a, (int)i);
}
// one wave per output word: the workgroup's four waves take four consecutive words.  Every lane of a wave takes the same branches (w is wave-uniform), so the ballot
// sees all 64 lanes; src is loaded once per word and the rows are looped inside
__global__ __launch_bounds__(MG_THREADS) void k_nd_mask(NdArgs a) {
  const long long t = MG_IDX();
  const int w = (int)(t >> 6), lane = (int)(threadIdx.x & 63);
  if (w >= a.W1) return;
  const int nn = 64 * w + lane;
  const int s = nn < a.N1 ? a.src[nn] : -1;
  for (int k = 0; k < ND_MASKS; k++)
    for (int row = 0; row < a.rows[k]; row++) {
      const bool b = s >= 0 && ndBit(a.inMask[k] + (size_t)row * a.W, s);
      const unsigned long long word = __ballot(b);
      if (lane == 0) a.outMask[k][(size_t)row * a.W1 + w] = word;
    }
}
__global__ __launch_bounds__(MG_THREADS) void k_nd_job(NdArgs a) {
  long long j = MG_IDX();
  if (j < a.M) ndJob(a, (int)j);
}
extern "C" int asched_internal_nd_mark(const NdArgs* a, int value, hipStream_t st) {
  if (a->n > 0) hipLaunchKernelGGL(k_nd_mark, dim3(mgBlocks(a->n)), dim3(MG_THREADS), 0, st, *a, value);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_nd_check(const NdArgs* a, hipStream_t st) {
  if (a->M > 0) hipLaunchKernelGGL(k_nd_check, dim3(mgBlocks(a->M)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_nd_gather(const NdArgs* a, hipStream_t st) {
  if (a->N1 <= 0) return 0;
  hipLaunchKernelGGL(k_nd_plane, dim3(mgBlocks((long long)a->R * a->N1)), dim3(MG_THREADS), 0, st, *a);
  hipLaunchKernelGGL(k_nd_narrow, dim3(mgBlocks(a->N1)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_nd_rank(const NdArgs* a, hipStream_t st) {
  if (a->N1 > 0) hipLaunchKernelGGL(k_nd_rank, dim3(mgBlocks(a->N1)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_nd_mask(const NdArgs* a, hipStream_t st) {
  int rows = 0;
  for (int k = 0; k < ND_MASKS; k++) rows += a->rows[k];
  if (rows > 0 && a->W1 > 0) hipLaunchKernelGGL(k_nd_mask, dim3(mgBlocks((long long)a->W1 * 64)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_nd_job(const NdArgs* a, hipStream_t st) {
  if (a->M > 0) hipLaunchKernelGGL(k_nd_job, dim3(mgBlocks(a->M)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ new rows join the resident node table (kernels_nodes_append.h)
// the planes, the narrow arrays, the merge of the index order and the mask rows, all into fresh blocks of the new size.  The mask pass is one THREAD per output word:
// almost every word is a copy, and consecutive lanes copy consecutive words of a row; only the last ceil(m / 64) + 1 words of a row hold new positions, and their
// thread loops over at most 64 entries (a wave per word would spend 64 lanes on one 8-byte copy: DESIGN 3.14)
#define NA_FN __device__ static inline
#include "kernels_nodes_append.h"
__global__ __launch_bounds__(MG_THREADS) void k_na_plane(NaArgs a) {
  long long e = MG_IDX();
  if (e < (long long)a.R * a.N1) naPlane(a, e);
}
__global__ __launch_bounds__(MG_THREADS) void k_na_narrow(NaArgs a) {
  long long i = MG_IDX();
  if (i < a.N1) naNarrow(a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_na_rank(NaArgs a) {
  long long i = MG_IDX();
  if (i < a.N1) naRank(a, (int)i);
}
__global__ __launch_bounds__(MG_THREADS) void k_na_mask(NaArgs a, long long work) {
  long long t = MG_IDX();
  if (t < work) naMaskWord(a, t);
}
extern "C" int asched_internal_na_planes(const NaArgs* a, hipStream_t st) {
  if (a->N1 <= 0) return 0;
  hipLaunchKernelGGL(k_na_plane, dim3(mgBlocks((long long)a->R * a->N1)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_na_narrow(const NaArgs* a, hipStream_t st) {
  if (a->N1 > 0) hipLaunchKernelGGL(k_na_narrow, dim3(mgBlocks(a->N1)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_na_rank(const NaArgs* a, hipStream_t st) {
  if (a->N1 > 0) hipLaunchKernelGGL(k_na_rank, dim3(mgBlocks(a->N1)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_na_mask(const NaArgs* a, hipStream_t st) {
  long long rows = 0;
  for (int k = 0; k < NA_MASKS; k++) rows += a->rows[k];
  const long long work = rows * a->W1;
  if (work > 0) hipLaunchKernelGGL(k_na_mask, dim3(mgBlocks(work)), dim3(MG_THREADS), 0, st, *a, work);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ queued lists from the resident order (kernels_queued_lists.h)
// mark (a thread per four rows: one 32-bit store of four flag bytes) and hold (a thread per held entry); the compaction is plat_compact's kernels
#define QL_FN __device__ static inline
#include "kernels_queued_lists.h"
__global__ __launch_bounds__(MG_THREADS) void k_ql_mark(QlArgs a, int words) {
  long long w = MG_IDX();
  if (w < words) qlMarkWord(a, (int)w);
}
__global__ __launch_bounds__(MG_THREADS) void k_ql_hold(QlArgs a) {
  long long i = MG_IDX();
  if (i < a.nHeld) qlHold(a, (int)i);
}
extern "C" int asched_internal_ql_mark(const QlArgs* a, hipStream_t st) {
  const int words = (a->M + 3) / 4;
  if (words > 0) hipLaunchKernelGGL(k_ql_mark, dim3(mgBlocks(words)), dim3(MG_THREADS), 0, st, *a, words);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asched_internal_ql_hold(const QlArgs* a, hipStream_t st) {
  if (a->nHeld > 0) hipLaunchKernelGGL(k_ql_hold, dim3(mgBlocks(a->nHeld)), dim3(MG_THREADS), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
