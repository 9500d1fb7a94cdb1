// armada_sched.hip — MI355X (gfx950) implementation of the C ABI in include/armada_sched.h.
//
// Kernels in this file:
//   k_control     persistent "round" kernel.  Workgroup 0: wave 0 runs the sequential DRF/gang control flow (round_ctl.h,
//                 round_fast.h), its 4 waves serve the data-parallel requests through an LDS mailbox; workgroups 1..H
//                 (round launches only) are helpers that share OP_SCAN / OP_FAIR through a mailbox in fine-grained HBM:
//                   OP_SCAN    first feasible node = argmin of the packed order key over nodes whose
//                              alloc[level][r][n] >= req[r]  (coalesced SoA planes, wave shuffle + LDS reduction)
//                   OP_BULK    evictors / unbind / populate / key rebuild as block-stride loops with int64 atomics
//                   OP_COMPACT order-preserving stream compaction (wave ballot + LDS prefix) for the per-queue
//                              evicted lists and the result lists
//                   OP_FAIR    fair-share preemption: per-node first covering Index over the evicted-table index, max
//   k_fit_batch   wide kernel: first feasible node for many (shape, level) queries against a fixed node state
//                 (BASELINE config 2, "nodedb fit kernel"): node tile in registers, wave-level min, one atomicMin/wave
//   k_shape_mask  per-shape static mask = requirement-class mask ∧ (total >= request)
//   k_drf / k_fair  float64 goldens (fairness.go / context/scheduling.go) evaluated on the device
//
// There is no CPU compute path in this library: without a gfx950 device asched_create() fails.
//
// Code objects of libarmada_sched.so, one per .hip file:
//   armada_sched.hip       k_control, the grid-wide kernels, the platform layer and the C ABI (asched_host.inc); no optional feature of the round kernel
//   armada_sched_aux.hip   k_control_aux: the submit-check commands and market-driven rounds
//   armada_sched_wk.hip    k_control_wk, k_bulk_wk, k_fit_batch_wk: two-word order keys, sharded wide passes, market-driven rounds
//   armada_sched_mgpu.hip  the multi-GPU exchange, submit-gang and evicted-table-rank kernels
// The device side the three round kernels share is round_kernel.h.
#include "round_kernel.h"

// The round kernel.  Workgroup 0: wave 0 runs the command (controlMain), waves 1..3 serve its LDS mailbox; workgroups 1..H are helpers (helperMain).
__global__ __launch_bounds__(CTL_THREADS) void k_control(Dev dev, int cmd, HelpBox* box, int H) {
  if (blockIdx.x != 0) { helperMain(dev, box, H); return; }
  if (threadIdx.x == 0) { g_box = box; g_H = H; g_gen = 0; g_fl.eng.abandon = 0; g_fl.eng.idleSince = 0; g_fl.eng.idleLast = 0; g_fl.eng.idleProg = 0; }
  // the Dev descriptor (pointers + config) is staged in LDS once; every wave reads it from there
  {
    const int* src = (const int*)&dev; int* dst = (int*)&g_dev;
    for (int i = threadIdx.x; i < (int)(sizeof(Dev) / sizeof(int)); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  Dev& d = g_dev;
  relocateIn(d, cmd);
  if (threadIdx.x >= 64) {  // worker waves: serve mailbox requests until OP_EXIT
    for (;;) {
      __syncthreads();
      int op = g_mb.op;
      if (op == OP_EXIT) break;
      if (op == OP_SCAN) {
        unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, (g_H + 1) * (int)blockDim.x);
        if ((threadIdx.x & 63) == 0) g_mb.partial[threadIdx.x >> 6] = v;
      } else if (op == OP_FAIR) {
        int v = fairPart(d, g_mb.fair, threadIdx.x, (g_H + 1) * (int)blockDim.x);
        if ((threadIdx.x & 63) == 0) g_mb.waveCount[threadIdx.x >> 6] = v;
      } else if (op == OP_SCANFAIR) {
        unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, (g_H + 1) * (int)blockDim.x);
        int w = fairPart(d, g_mb.fair, threadIdx.x, (g_H + 1) * (int)blockDim.x);
        if ((threadIdx.x & 63) == 0) { g_mb.partial[threadIdx.x >> 6] = v; g_mb.waveCount[threadIdx.x >> 6] = w; }
      } else if (op == OP_BULK) {
        bulkPart(d, g_mb.kind, g_mb.n);
      } else if (op == OP_BULKW) {
        int nthreads = (g_H + 1) * (int)blockDim.x; int kd = g_mb.kind, nn = g_mb.n;
        for (int i = threadIdx.x; i < nn; i += nthreads) bulkElem(d, kd, i);
        __threadfence();
      }
      else if (op == OP_WIDE) {
        int nthreads = (g_H + 1) * (int)blockDim.x; int kd = g_mb.kind, nn = g_mb.n;
        for (int i = threadIdx.x; i < nn; i += nthreads) wideBulkAny(d, kd, i);
        __threadfence();
      }
      else if (op == OP_COMPACT) {
        compactPart(d);
      } else if (op == OP_ENGINE) {
        if ((threadIdx.x >> 6) == 1) engineLoop(d); else if ((threadIdx.x >> 6) == 2) bindLoop(d); else if ((threadIdx.x >> 6) == 3 && d.f.engineHc) coldLoop(d);
      }
      __syncthreads();
    }
    relocateOut();
    return;
  }
  controlMain(d, cmd);
  __threadfence();
  if ((threadIdx.x & 63) == 0) { g_mb.op = OP_EXIT; if (g_H) helpIssue(OP_HELPERS_EXIT, (const ScanArgs*)nullptr); }
  __syncthreads();
  relocateOut();
}

// ---- grid-wide kernels of the split round (asched_host.inc runRoundSplit): the data-parallel phases of PreemptingQueueScheduler.Schedule over
// all CUs.  Between launches the authoritative state is in HBM (relocateOut), so the per-element bodies of round_run.h run unchanged.
__global__ __launch_bounds__(256) void k_bulk(Dev d, int kind, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) bulkElem(d, kind, i);
}
__global__ void k_round_small(Dev d, int what, int arg) { if (blockIdx.x == 0 && threadIdx.x == 0) roundSmall(d, what, arg); }

// sum of v over the lanes selected by `sel` (wave-uniform mask), returned on every lane
__device__ static inline int64_t waveSumSel(int64_t v, unsigned long long sel) {
  int lane = threadIdx.x & 63;
  int64_t x = ((sel >> lane) & 1) ? v : 0;
  for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
// Evictor.Evict + sctx.EvictJob for every flagged job (round_run.h evictApply), grid-wide.  Jobs are walked in the pre-sorted (queue, scheduling
// order) list, so the lanes of a wave mostly share a queue: the per-queue / per-priority-class / pool sums are reduced across the wave first and
// leave as ONE atomic per (wave, key, resource) instead of one per job — same integer sums, ~64x fewer same-address atomics.
__global__ __launch_bounds__(256) void k_evict_apply(Dev d, int phase3, int total) {
  const DevCfg& c = d.cfg;
  int lane = threadIdx.x & 63;
  int rounds = (total + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0; it < rounds; it++) {   // wave-uniform trip count: every lane takes part in the reductions
    int i = (it * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    int j = i < total ? d.ordAll[i] : -1;
    bool act = j >= 0 && d.evFlag[j];
    int64_t A[MAXR], S[MAXR], E1[MAXR], E2[MAXR];
    int key = -1, q = 0, pc = 0, cntSched = 0, cntEv = 0;
#pragma unroll
    for (int r = 0; r < MAXR; r++) { A[r] = S[r] = E1[r] = E2[r] = 0; }
    if (act) {
      int n = d.jobNode[j];
      if (d.schedAtPrio[j] == NO_PRIORITY) { raise(d, ASCHED_ERR_INTERNAL, 800); act = false; }   // EvictJobsFromNode nodedb.go:1085-1088
      else {
        const int64_t* req = JREQ(d, j);
        d.jobEvictedOnNode[j] = 1;  // Node.EvictJob node.go:449-474
        atomicMarkAllocatable(d, n, d.jobCutoff[j], req, +1);
        atomicMarkAllocatable(d, n, ASCHED_EVICTED_PRIORITY, req, -1);
        d.jcEvicted[j] = 1; d.jcAssigned[j] = n; d.jcReason[j] = 0; d.jcHasPctx[j] = 0; d.jcUniValue[j] = -1; d.jcStagedBy[j] = -1;   // fresh jctx pinned to the node (eviction.go:246-253)
        int g = d.jGang[j];
        d.jcGangCard[j] = g >= 0 ? d.gangOff[g + 1] - d.gangOff[g] : 1;  // setEvictedGangCardinality pqs.go:462-483
        q = d.jQueue[j]; pc = d.jPc[j]; key = q * c.npc + pc;
        uint8_t f = d.jobFlags[j];
        bool sched = f & F_SUCCESSFUL, resched = f & F_RESCHEDULED;
        if (sched || resched) { if (sched) f &= ~F_SUCCESSFUL; if (resched) f &= ~F_RESCHEDULED; } else f |= F_EVICTED;
        d.jobFlags[j] = f;
        for (int r = 0; r < MAXR; r++) if (r < c.R) { A[r] = -req[r]; S[r] = sched ? -req[r] : 0; E1[r] = (!sched && !resched) ? req[r] : 0; E2[r] = !sched ? req[r] : 0; }
        cntSched = sched ? -1 : 0; cntEv = sched ? 0 : 1;
        if (!phase3) { d.inPreempted[j] = 1; d.preemptedNode[j] = n; }
        else if (d.inScheduled[j]) { d.inScheduled[j] = 0; d.inSchedAndEvicted[j] = 1; d.preemptedNode[j] = n; }
        else { d.inPreempted[j] = 1; d.preemptedNode[j] = n; }
      }
    }
    unsigned long long todo = __ballot(act);
    if (!todo) continue;
    // pool-wide sums: every active lane
    for (int r = 0; r < c.R; r++) {
      int64_t a = waveSumSel(A[r], todo), s2 = waveSumSel(S[r], todo), e2 = waveSumSel(E2[r], todo);
      if (lane == 0) { if (a) atomicAddI64(&d.rs->allocated[r], a); if (s2) atomicAddI64(&d.rs->scheduled[r], s2); if (e2) atomicAddI64(&d.rs->evicted[r], e2); }
    }
    { int cs = (int)waveSumSel(cntSched, todo), ce = (int)waveSumSel(cntEv, todo);
      if (lane == 0) { if (cs) atomicAddI32(&d.rs->numScheduledJobs, cs); if (ce) atomicAddI32(&d.rs->numEvictedJobs, ce); } }
    // per (queue, priority class): one group per distinct key in the wave
    while (todo) {
      int first = __ffsll((long long)todo) - 1;
      int k0 = __shfl(key, first, 64);
      unsigned long long sel = __ballot(act && key == k0) & todo;
      int q0 = k0 / c.npc;
      for (int r = 0; r < c.R; r++) {
        int64_t a = waveSumSel(A[r], sel), s2 = waveSumSel(S[r], sel), e1 = waveSumSel(E1[r], sel);
        if (lane == 0) {
          size_t ix = (size_t)k0 * c.R + r;
          if (a) { atomicAddI64(&d.qAllocByPc[ix], a); atomicAddI64(&d.qAlloc[(size_t)q0 * c.R + r], a); }
          if (s2) atomicAddI64(&d.qSchedByPc[ix], s2);
          if (e1) atomicAddI64(&d.qEvictedByPc[ix], e1);
        }
      }
      todo &= ~sel;
    }
  }
}

// order-preserving compaction of {order[p] : flag[order[p]]} over the whole grid (order == NULL: identity): count per 4096-element block, scan
// of the block counts, ordered write.  prefix[p] = number of flagged elements before p (may be NULL).
#define CMP_CHUNK 4096
__global__ __launch_bounds__(256) void k_cmp_count(const int32_t* order, int n, const uint8_t* flag, int32_t* blockCount) {
  __shared__ int wsum[4];
  int base = blockIdx.x * CMP_CHUNK, cnt = 0;
  for (int o = threadIdx.x; o < CMP_CHUNK; o += 256) { int p = base + o; if (p < n && flag[order ? order[p] : p]) cnt++; }
  for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) blockCount[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ void k_cmp_scan(int32_t* blockCount, int nblocks, int32_t* totalOut) {   // one thread: a few hundred blocks at most
  if (blockIdx.x || threadIdx.x) return;
  int run = 0;
  for (int b = 0; b < nblocks; b++) { int v = blockCount[b]; blockCount[b] = run; run += v; }
  *totalOut = run;
}
__global__ __launch_bounds__(256) void k_cmp_write(const int32_t* order, int n, const uint8_t* flag, int32_t* dst, uint32_t* prefix, const int32_t* blockOffset) {
  __shared__ int wcnt[4];
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int run = blockOffset[blockIdx.x];
  for (int t = 0; t < CMP_CHUNK / 256; t++) {
    int p = blockIdx.x * CMP_CHUNK + t * 256 + threadIdx.x;
    int v = p < n ? (order ? order[p] : p) : 0;
    bool f = p < n && flag[v];
    unsigned long long b = __ballot(f);
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < 4; w++) { int cw = wcnt[w]; if (w < wave) off += cw; tot += cw; }
    int rank = run + off + __popcll(b & ((1ull << lane) - 1));
    if (p < n && prefix) prefix[p] = rank;
    if (f) dst[rank] = v;
    run += tot;
    __syncthreads();
  }
}
__global__ void k_seg_off(const int32_t* segOff, int nseg, int n, const uint32_t* prefix, const int32_t* total, int32_t* outSegOff) {
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q <= nseg) outSegOff[q] = segOff[q] < n ? (int32_t)prefix[segOff[q]] : *total;
}

// ---- fairness optimiser (round_opt.h): per-node job lists (count / scan / scatter), queue costs, then every node scored for one job at once
__global__ __launch_bounds__(256) void k_opt_count(Dev d, int32_t* cnt) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < d.cfg.M; j += gridDim.x * blockDim.x) { int n = d.jobNode[j]; if (n >= 0) atomicAdd(&cnt[n], 1); int g = d.rs->optMode ? d.optGhost[j] : -1; if (g >= 0) atomicAdd(&cnt[g], 1); }   // (ghost: dev.h optGhost)
}
__global__ __launch_bounds__(1024) void k_opt_scan(const int32_t* cnt, int32_t* off, int32_t* cursor, int N) {   // one block: chunk sums, serial scan of 1024 partials, chunk offsets
  __shared__ int part[1024];
  int C = (N + 1023) / 1024, n0 = threadIdx.x * C, n1 = n0 + C < N ? n0 + C : N;
  int sum = 0;
  for (int n = n0; n < n1; n++) sum += cnt[n];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) { int run = 0; for (int i = 0; i < 1024; i++) { int v = part[i]; part[i] = run; run += v; } off[N] = run; }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int n = n0; n < n1; n++) { off[n] = run; cursor[n] = run; run += cnt[n]; }
}
__global__ __launch_bounds__(256) void k_opt_scatter(Dev d, int32_t* cursor, int32_t* jobs) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < d.cfg.M; j += gridDim.x * blockDim.x) { int n = d.jobNode[j]; if (n >= 0) jobs[atomicAdd(&cursor[n], 1)] = j; int g = d.rs->optMode ? d.optGhost[j] : -1; if (g >= 0) jobs[atomicAdd(&cursor[g], 1)] = j; }
}
__global__ void k_opt_qcost(Dev d, int job, double* qCost) {   // QueueContext.CurrentCost per queue (scheduling_context.go:19-24); [Q]: the job's own DRF cost
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < d.cfg.Q) {
    int64_t a[MAXR];
    for (int r = 0; r < MAXR; r++) a[r] = r < d.cfg.R ? QV(d.qAlloc, q)[r] + QV(d.qPenalty, q)[r] : 0;
    qCost[q] = d.optQDelta ? d.optQDelta[q] : drf(d, a);   // (later members of a gang: CurrentCost as updateState left it, kept by the host)
  } else if (q == d.cfg.Q) qCost[q] = drf(d, JREQ(d, job));
}
__global__ __launch_bounds__(128) void k_opt_score(Dev d, OptArgs a, const double* qCost, const int32_t* off, const int32_t* jobs, OptNodeOut* out) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < d.cfg.N) optScoreNode(d, a, qCost, off, jobs, d.jLeaseMs, n, &out[n], nullptr);
}
// ---- k_opt_score_wave: PreemptingNodeScheduler.Schedule (round_opt.h optScoreNodeE) with ONE WAVE per node, one lane per job on the node.
// The one-node-per-thread kernel walks its node's job list serially — a chain of dependent gathers per job and two insertion sorts in private memory (2.4 KB of
// scratch per thread) — and leaves most of the chip idle (20 000 nodes = 313 waves).  Here the gathers of a node are one round trip (lane k loads job k's row), the two
// orderings are rank sorts (lane k counts the entries that order before its own; entries are broadcast with v_readlane, so the loop is wave-uniform and as long as the
// node's job count), the fit prefix is a wave scan of the request vectors and "first prefix that fits" a ballot.  What the reference computes with SEQUENTIAL float
// arithmetic keeps its order: the running queue cost (rounded after every subtraction), the sum of the preemption costs and the per-queue cost changes are serial
// loops over broadcast values — every lane performs the same operations in the same order, so the doubles are the ones the serial routine produces.
// Nodes with more than 64 jobs report overflow (-1) like the private-list kernel and go through k_opt_score_big.
template <class T> __device__ static inline T wvRead(T v, int lane) {   // lane: wave-uniform
  static_assert(sizeof(T) % 4 == 0, "dword multiples");
  int w[sizeof(T) / 4]; T r;
  __builtin_memcpy(w, &v, sizeof(T));
  for (int k = 0; k < (int)(sizeof(T) / 4); k++) w[k] = __builtin_amdgcn_readlane(w[k], lane);
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}
template <class T> __device__ static inline T wvPush(T v, int dstLane) {   // lane dstLane receives this lane's v (ds_permute: dstLane must be a permutation of the lanes)
  int w[sizeof(T) / 4]; T r;
  __builtin_memcpy(w, &v, sizeof(T));
  for (int k = 0; k < (int)(sizeof(T) / 4); k++) w[k] = __builtin_amdgcn_ds_permute(dstLane << 2, w[k]);
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}
template <class T> __device__ static inline T wvPull(T v, int srcLane) {   // this lane receives lane srcLane's v
  int w[sizeof(T) / 4]; T r;
  __builtin_memcpy(w, &v, sizeof(T));
  for (int k = 0; k < (int)(sizeof(T) / 4); k++) w[k] = __builtin_amdgcn_ds_bpermute(srcLane << 2, w[k]);
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}
struct OptLane { int32_t job, queue, sap, ordinal, prioPre, ctpZero; int64_t age; double cost, wcap; };
__device__ static inline bool optInQueueLessL(const OptLane& a, const OptLane& b) {   // round_opt.h optInQueueLess
  if (a.queue != b.queue) return a.queue < b.queue;
  if (a.sap != b.sap) return a.sap < b.sap;
  if (a.cost != b.cost) return a.cost < b.cost;
  if (a.age != b.age) return a.age < b.age;
  return a.job < b.job;
}
__device__ static inline bool optGlobalLessL(const OptLane& a, const OptLane& b) {    // round_opt.h optGlobalLess
  if (a.queue == b.queue) return a.ordinal < b.ordinal;
  if (a.prioPre != b.prioPre) return a.prioPre != 0;
  if (a.wcap > b.wcap) return true;
  if (a.wcap == b.wcap) {
    if (a.sap != b.sap) return a.sap < b.sap;
    if (a.cost != b.cost) return a.cost < b.cost;
    if (a.age != b.age) return a.age < b.age;
    return a.job < b.job;
  }
  return false;
}
// entries to their ranks: valid lanes go to lane `rank` (0 .. m-1), the others fill m .. 63 in lane order, so the move is a permutation
__device__ static inline int optDest(bool valid, int rank, unsigned long long validMask, int lane) {
  int m = __builtin_popcountll(validMask);
  int invalidBefore = __builtin_popcountll(~validMask & ((1ull << lane) - 1));
  return valid ? rank : m + invalidBefore;
}
// one wave, node n: *outp = the node's score (written by lane 0), preOut (optional) = the victims in preemption order
__device__ static void optScoreNodeWave(Dev& d, const OptArgs& a, const double* qCost, const int32_t* off, const int32_t* jobs, int n, OptNodeOut* outp, int32_t* preOut) {
  const DevCfg& c = d.cfg;
  const int lane = threadIdx.x & 63;
  OptNodeOut* out = outp - n;                                                  // (the body below writes out[n])
  OptNodeOut res; res.scheduled = 0; res.npre = 0; res.cost = 0; res.impact = 0;
  const int job = a.job;
  const uint64_t* mask = d.shapeMask + (size_t)d.jShape[job] * c.W;
  if (!((mask[n >> 6] >> (n & 63)) & 1)) { if (lane == 0) out[n] = res; return; }
  const int64_t* req = JREQ(d, job);
  int64_t avail[MAXR];
  bool fits0 = true;
  for (int r = 0; r < MAXR; r++) { avail[r] = r < c.R ? AL(d, c.evLevel, r, n) : 0; if (r < c.R && req[r] > avail[r]) fits0 = false; }
  if (fits0) { res.scheduled = 1; if (lane == 0) out[n] = res; return; }
  const int k0 = off[n], cnt = off[n + 1] - k0;
  if (cnt > 64) { res.scheduled = -1; if (lane == 0) out[n] = res; return; }   // more jobs than lanes: scored by k_opt_score_big
  const int32_t jobPrio = c.pcPriority[d.jPc[job]];
  // ---- one lane per job on the node (node.AllocatedByJobId, node_scheduler.go:137-200)
  OptLane e; e.job = 0x7fffffff; e.queue = 0; e.sap = 0; e.ordinal = 0; e.prioPre = 0; e.ctpZero = 1; e.age = 0; e.cost = 0; e.wcap = 0;
  int64_t jr[MAXR];
  for (int r = 0; r < MAXR; r++) jr[r] = 0;
  bool valid = false;
  if (lane < cnt) {
    int j = jobs[k0 + lane];
    bool ok = c.pcPreemptible[d.jPc[j]] != 0 && d.jGang[j] < 0;
    const int64_t* q = JREQ(d, j);
    if (ok && a.hasMaxSize) for (int r = 0; r < c.R; r++) if (a.maxSize[r] != 0 && q[r] > a.maxSize[r]) ok = false;
    int32_t sap = d.schedAtPrio[j];
    ok = ok && sap != NO_PRIORITY && sap <= jobPrio;
    if (ok) {
      valid = true;
      e.job = j; e.queue = d.jQueue[j]; e.sap = sap;
      e.age = d.jNode0[j] < 0 ? 0 : a.nowMs - d.jLeaseMs[j];
      e.cost = drf(d, q);
      for (int r = 0; r < c.R; r++) jr[r] = q[r];
    }
  }
  unsigned long long vm = __ballot(valid);
  const int m = __builtin_popcountll(vm);
  if (m == 0) { if (lane == 0) out[n] = res; return; }
  // ---- per queue order (optInQueueLess): rank = how many entries order before mine
  {
    int rank = 0;
    for (int i = 0; i < cnt; i++) {
      if (!((vm >> i) & 1)) continue;
      OptLane o = wvRead(e, i);
      if (valid && optInQueueLessL(o, e)) rank++;
    }
    int dst = optDest(valid, rank, vm, lane);
    e = wvPush(e, dst);
    for (int r = 0; r < c.R; r++) jr[r] = wvPush(jr[r], dst);
  }
  valid = lane < m;
  // the queue's cost, weight and capped fair share, one gather per lane (broadcast below)
  double qc = valid ? qCost[e.queue] : 0.0, qw = valid ? d.qWeight[e.queue] : 1.0, qd = valid ? d.qDc[e.queue] : 0.0;
  // ---- populateQueueImpactFields (:203-232): the running queue cost is rounded after every subtraction — in order, on broadcast values
  {
    double updated = 0; int prevQ = -1, ord = 0;
    for (int i = 0; i < m; i++) {
      int qi = wvRead(e.queue, i);
      if (qi != prevQ) { updated = wvRead(qc, i); ord = 0; prevQ = qi; }
      updated = optRound8(updated - wvRead(e.cost, i));
      double w = updated / wvRead(qw, i);
      int sapi = wvRead(e.sap, i);
      int prioPre = sapi < jobPrio, ctpZero = (sapi < jobPrio) || (updated > wvRead(qd, i));
      if (lane == i) { e.wcap = w; e.prioPre = prioPre; e.ctpZero = ctpZero; e.ordinal = ord; }
      ord++;
    }
  }
  // ---- global preemption order (optGlobalLess)
  {
    int rank = 0;
    for (int i = 0; i < m; i++) {
      OptLane o = wvRead(e, i);
      if (valid && optGlobalLessL(o, e)) rank++;
    }
    unsigned long long m2 = m >= 64 ? ~0ull : ((1ull << m) - 1);
    int dst = optDest(valid, rank, m2, lane);
    e = wvPush(e, dst); qc = wvPush(qc, dst);
    for (int r = 0; r < c.R; r++) jr[r] = wvPush(jr[r], dst);
  }
  // ---- preempt one job at a time until the job fits (:84-99): inclusive prefix sums of the victims' requests, first prefix that fits
  for (int r = 0; r < c.R; r++) {
    int64_t v = valid ? jr[r] : 0;
    for (int s = 1; s < 64; s <<= 1) { int64_t o = wvPull(v, lane >= s ? lane - s : lane); if (lane >= s) v += o; }
    jr[r] = v;
  }
  bool f = valid;
  for (int r = 0; r < c.R; r++) if (req[r] > avail[r] + jr[r]) f = false;
  unsigned long long fm = __ballot(f);
  if (fm == 0) { if (lane == 0) out[n] = res; return; }
  const int used = __builtin_ctzll(fm) + 1;
  double total = 0;
  for (int i = 0; i < used; i++) total += wvRead(e.ctpZero, i) ? 0.0 : wvRead(e.cost, i);
  // maximumQueueImpact (:101-113): per queue |sum of the preempted jobs' costs, in preemption order| / CurrentCost
  double change = 0;
  for (int i = 0; i < used; i++) { int qi = wvRead(e.queue, i); double ci = wvRead(e.cost, i); if (qi == e.queue) change -= ci; }
  double imp = lane < used ? fabs(change) / qc : 0.0;
  if (!(imp > 0.0)) imp = 0.0;   // (the serial routine keeps a value only if it compares greater than the running maximum: a NaN never does)
  for (int s = 32; s; s >>= 1) { double o = __shfl_xor(imp, s, 64); imp = o > imp ? o : imp; }
  res.scheduled = 1; res.npre = used; res.cost = total; res.impact = imp;
  if (preOut && lane < used) preOut[lane] = e.job;
  if (lane == 0) out[n] = res;
}
__global__ __launch_bounds__(256) void k_opt_score_wave(Dev d, OptArgs a, const double* qCost, const int32_t* off, const int32_t* jobs, OptNodeOut* out) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= d.cfg.N) return;                                                    // (whole waves leave together: one node per wave)
  optScoreNodeWave(d, a, qCost, off, jobs, n, &out[n], nullptr);
}
__global__ __launch_bounds__(64) void k_opt_detail_wave(Dev d, OptArgs a, const double* qCost, const int32_t* off, const int32_t* jobs, int n, OptNodeOut* out, int32_t* pre) {
  optScoreNodeWave(d, a, qCost, off, jobs, n, out, pre);
}
// ---- the candidate selection of FairnessOptimisingGangScheduler.scheduleOnNodes (gang_scheduler.go:100-141) on the device, so that one asched_optimiser_schedule_job is one
// stream-ordered sequence (queue costs -> scores -> selection -> victims of the selected node) with a single small download instead of 20 000 scores and two round trips.
// Nodes in id order: the first that needs no preemption wins outright; otherwise the smallest (schedulingCost, maximumQueueImpact) among those whose fairness improvement
// exceeds the threshold, the earlier id on a tie (the reference draws a ULID).  `overflow` counts nodes the wave kernel could not score (more than 64 jobs): the host then
// takes the long way (k_opt_score_big + its own loop).
struct OptSel { int32_t node, npre, big, overflow; double cost, impact; };
struct OptSelKey { int32_t cat, rank, node, npre; double cost, impact; };   // cat 0: no preemption needed, 1: candidate, 2: nothing
__device__ static inline bool optSelLess(const OptSelKey& a, const OptSelKey& b) {
  if (a.cat != b.cat) return a.cat < b.cat;
  if (a.cat == 2) return false;
  if (a.cat == 1) { if (a.cost != b.cost) return a.cost < b.cost; if (a.impact != b.impact) return a.impact < b.impact; }
  return a.rank < b.rank;
}
__device__ static inline OptSelKey optSelReduceWave(OptSelKey k) {
  for (int s = 32; s; s >>= 1) {
    OptSelKey o;
    o.cat = __shfl_xor(k.cat, s, 64); o.rank = __shfl_xor(k.rank, s, 64); o.node = __shfl_xor(k.node, s, 64); o.npre = __shfl_xor(k.npre, s, 64);
    o.cost = __shfl_xor(k.cost, s, 64); o.impact = __shfl_xor(k.impact, s, 64);
    if (optSelLess(o, k)) k = o;
  }
  return k;
}
__global__ __launch_bounds__(256) void k_opt_select(Dev d, const OptNodeOut* out, const uint8_t* mask, const double* jobCostPtr, double minPct, OptSelKey* partial, int32_t* overflow) {
  __shared__ OptSelKey wk[4];
  int n = blockIdx.x * 256 + threadIdx.x;
  OptSelKey k; k.cat = 2; k.rank = 0x7fffffff; k.node = -1; k.npre = 0; k.cost = 0; k.impact = 0;
  if (n < d.cfg.N && (!mask || mask[n])) {
    OptNodeOut r = out[n];
    if (r.scheduled < 0) atomicAdd(overflow, 1);
    if (r.scheduled > 0) {
      double jobCost = *jobCostPtr;
      bool ideal = r.cost == 0 && r.npre == 0;                                   // :112-116
      double improvement = ((jobCost / r.cost) * 100) - 100;                     // :118-121 (cost 0 with victims: +Inf)
      if (ideal || improvement > minPct) { k.cat = ideal ? 0 : 1; k.rank = d.nodeIdRank ? d.nodeIdRank[n] : n; k.node = n; k.npre = r.npre; k.cost = r.cost; k.impact = r.impact; }
    }
  }
  k = optSelReduceWave(k);
  if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) { for (int w = 1; w < 4; w++) if (optSelLess(wk[w], k)) k = wk[w]; partial[blockIdx.x] = k; }
}
__global__ __launch_bounds__(256) void k_opt_select_final(const OptSelKey* partial, int nb, const int32_t* overflow, OptSel* sel) {
  __shared__ OptSelKey wk[4];
  OptSelKey k; k.cat = 2; k.rank = 0x7fffffff; k.node = -1; k.npre = 0; k.cost = 0; k.impact = 0;
  for (int i = threadIdx.x; i < nb; i += 256) if (optSelLess(partial[i], k)) k = partial[i];
  k = optSelReduceWave(k);
  if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) if (optSelLess(wk[w], k)) k = wk[w];
    sel->node = k.cat == 2 ? -1 : k.node; sel->npre = k.npre; sel->big = 0; sel->overflow = *overflow; sel->cost = k.cost; sel->impact = k.impact;
  }
}
__global__ __launch_bounds__(64) void k_opt_detail_sel(Dev d, OptArgs a, const double* qCost, const int32_t* off, const int32_t* jobs, OptSel* sel, OptNodeOut* scratchOut, int32_t* pre) {
  int n = sel->node;
  if (n < 0 || sel->npre == 0 || sel->overflow) return;
  if (off[n + 1] - off[n] > 64) { if (threadIdx.x == 0) sel->big = 1; return; }   // (cannot happen while overflow == 0; kept as a guard)
  optScoreNodeWave(d, a, qCost, off, jobs, n, scratchOut, pre);
}
__global__ void k_opt_detail(Dev d, OptArgs a, const double* qCost, const int32_t* off, const int32_t* jobs, int n, OptNodeOut* out, int32_t* pre) {
  if (blockIdx.x == 0 && threadIdx.x == 0) optScoreNode(d, a, qCost, off, jobs, d.jLeaseMs, n, out, pre);
}
// nodes with more than OPT_MAXJ candidates (k_opt_score reported overflow): the same routine with the entry list in an HBM scratch sized by the node's job count
__global__ void k_opt_score_big(Dev d, OptArgs a, const double* qCost, const int32_t* off, const int32_t* jobs, const int32_t* nodes, const long long* eOff, int nb, OptEntry* scratch, OptNodeOut* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) { int n = nodes[i]; optScoreNodeE(d, a, qCost, off, jobs, d.jLeaseMs, n, &out[n], nullptr, scratch + eOff[i], off[n + 1] - off[n]); }
}
__global__ void k_opt_detail_big(Dev d, OptArgs a, const double* qCost, const int32_t* off, const int32_t* jobs, int n, OptNodeOut* out, int32_t* pre, OptEntry* scratch) {
  if (blockIdx.x == 0 && threadIdx.x == 0) optScoreNodeE(d, a, qCost, off, jobs, d.jLeaseMs, n, out, pre, scratch, off[n + 1] - off[n]);
}

// the indicative gang pricer (round_price.h): every node priced for one gang member; the entry list shares the layout of the node -> jobs index
__global__ __launch_bounds__(128) void k_price_score(Dev d, PriceArgs a, const int32_t* off, const int32_t* jobs, PriceEntry* entries, PriceNodeOut* out) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < d.cfg.N) priceScoreNode(d, a, off, jobs, d.jLeaseMs, n, &out[n], nullptr, entries + off[n]);
}
__global__ void k_price_detail(Dev d, PriceArgs a, const int32_t* off, const int32_t* jobs, PriceEntry* entries, int n, PriceNodeOut* out, int32_t* pre) {
  if (blockIdx.x == 0 && threadIdx.x == 0) priceScoreNode(d, a, off, jobs, d.jLeaseMs, n, out, pre, entries + off[n]);
}

__global__ void k_shape_mask(Dev d, const uint64_t* classMask, const int32_t* shapeClass) {
  const DevCfg& c = d.cfg;
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)c.S * c.W) return;
  int s = (int)(t / c.W), w = (int)(t % c.W);
  uint64_t cm = classMask[(size_t)shapeClass[s] * c.W + w], m = 0;
  for (int b = 0; b < 64; b++) {
    int n = w * 64 + b;
    if (n >= c.N) break;
    if (!((cm >> b) & 1)) continue;
    bool ok = true;
    for (int r = 0; r < c.R; r++) ok = ok && d.shapeReq[(size_t)s * c.R + r] <= d.totalRes[(size_t)r * c.Npad + n];  // nodematching.go:184
    if (ok) m |= 1ull << b;
  }
  d.shapeMask[t] = m;
}

// First feasible node for a batch of (shape) queries at one level against the current node state.
// grid.x tiles the nodes (one node per thread, its key and R alloc values stay in registers for the whole
// shape loop), grid.y splits the shape list.  HBM traffic per launch = N*(8 + 8R) bytes + masks.
#define FIT_TILE 256
__global__ __launch_bounds__(FIT_TILE) void k_fit_batch(Dev d, const int32_t* shapes, int nshapes, int level, unsigned long long* out) {
  const DevCfg& c = d.cfg;
  int n = blockIdx.x * FIT_TILE + threadIdx.x;
  bool valid = n < c.N;
  unsigned long long key = valid ? d.keys[(size_t)level * c.Npad + n] : ~0ull;
  int64_t al[MAXR];
  for (int r = 0; r < MAXR; r++) al[r] = (valid && r < c.R) ? d.alloc[((size_t)level * c.R + r) * c.Npad + n] : 0;
  int per = (nshapes + gridDim.y - 1) / gridDim.y;
  int s0 = blockIdx.y * per, s1 = min(nshapes, s0 + per);
  int word = n >> 6, bit = n & 63;
  __shared__ unsigned long long wmin[FIT_TILE / 64];
  for (int i = s0; i < s1; i++) {
    int s = shapes[i];
    bool f = valid && ((d.shapeMask[(size_t)s * c.W + word] >> bit) & 1);
    const int64_t* req = d.shapeReq + (size_t)s * c.R;
    for (int r = 0; r < c.R; r++) f = f && req[r] <= al[r];
    unsigned long long v = __ballot(f) ? waveMin64Dpp(f ? key : ~0ull) : ~0ull;
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = v;
    __syncthreads();
    // ONE look / write per workgroup and shape, at a word that has a cache line of its own.  (Round 3: every wave sent its minimum to out[i], 8 bytes from out[i + 1]: 100 000
    // read-modify-writes on four cache lines at 100 000 nodes x 64 shapes, serialised in one L2 channel — 0.19 ms for a 4 MB problem.)  The word only ever falls, and first fit
    // means it falls early: look first, write only what improves it.
    if (threadIdx.x == 0) {
      unsigned long long m = wmin[0];
      for (int w = 1; w < FIT_TILE / 64; w++) m = wmin[w] < m ? wmin[w] : m;
      if (m != ~0ull && m < __hip_atomic_load(&out[(size_t)i * FIT_OSTR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&out[(size_t)i * FIT_OSTR], m);
    }
    __syncthreads();
  }
}

// ---- sorted base of the level-0 fast structure: the ordered index of the fresh NodeDb (nodedb.go:1164-1175), built in round_prepare
__global__ void k_base_fill(Dev d, int nb2) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb2) d.baseKey[i] = i < d.cfg.N ? fastKeyOf(d, i) : ~0ull;  // level 0 plane of keys (a negative column: field 0, fits nothing)
}
__global__ void k_bitonic_step(unsigned long long* a, int j, int k) {
  unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned l = i ^ (unsigned)j;
  if (l > i) {
    unsigned long long x = a[i], y = a[l];
    bool up = (i & (unsigned)k) == 0;
    if (up ? x > y : x < y) { a[i] = y; a[l] = x; }
  }
}
// the in-LDS part of the network: every (k, j) step with j < 2048 for one 4096-key tile, 1024 threads
__global__ __launch_bounds__(1024) void k_bitonic_tile(unsigned long long* a, int kStart, int kEnd, int jStart) {
  __shared__ unsigned long long t[4096];
  unsigned base = blockIdx.x * 4096u;
  for (int i = threadIdx.x; i < 4096; i += 1024) t[i] = a[base + i];
  __syncthreads();
  for (int k = kStart; k <= kEnd; k <<= 1) {
    for (int j = (k == kStart ? jStart : k >> 1); j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < 4096; i += 1024) {
        unsigned l = (unsigned)i ^ (unsigned)j;
        if (l > (unsigned)i) {
          unsigned long long x = t[i], y = t[l];
          bool up = ((base + i) & (unsigned)k) == 0;
          if (up ? x > y : x < y) { t[i] = y; t[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < 4096; i += 1024) a[base + i] = t[i];
}
__global__ void k_base_finish(Dev d) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  const DevCfg& c = d.cfg;
  if (i >= c.N) return;
  unsigned long long key = d.baseKey[i];
  int node = d.nodeByRank[key & ((1ull << c.idxBits) - 1)];
  d.baseNode[i] = node; d.posOf[node] = i; d.baseRemoved[i] = 0; d.baseCls[i] = d.nodeCls[node]; d.l0Slot[node] = -1;
  for (int e = 0; e < d.f.E; e++) d.baseExtra[(size_t)e * c.Npad + i] = d.alloc[(size_t)d.f.extraCol[e] * c.Npad + node];  // level 0 planes
}


// The round-input builder's sums (round_run.h B_AGG_RUN / B_AGG_QUEUED) grid-wide with the wave-level pre-reduction of k_evict_apply: both walks are
// ordered by queue (the pre-sorted job order; the queued lists), so a wave holds a handful of (queue, class) keys and leaves one atomic per key and resource.
__global__ __launch_bounds__(256) void k_agg(Dev d, int queued, int total) {
  const DevCfg& c = d.cfg;
  int lane = threadIdx.x & 63;
  int rounds = (total + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0; it < rounds; it++) {   // wave-uniform trip count
    int i = (it * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    bool act = false; int key = -1; int64_t V[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; r++) V[r] = 0;
    if (i < total) {
      int j, q;
      if (queued) {
        int lo = 0, hi = c.Q;
        while (lo < hi) { int mid = (lo + hi) >> 1; if (d.queuedOff[mid + 1] <= i) lo = mid + 1; else hi = mid; }
        q = lo; j = d.queuedJobs[i];
        act = q < c.Q && !d.qCordoned[q];
      } else {
        j = d.ordAll[i]; q = d.jQueue[j];
        act = d.jNode0[j] >= 0 && q >= 0 && q < c.Q;
      }
      if (act) { key = q * c.npc + d.jPc[j]; const int64_t* req = JREQ(d, j); for (int r = 0; r < MAXR; r++) if (r < c.R) V[r] = req[r]; }
    }
    unsigned long long todo = __ballot(act);
    while (todo) {
      int first = __ffsll((long long)todo) - 1;
      int k0 = __shfl(key, first, 64);
      unsigned long long sel = __ballot(act && key == k0) & todo;
      for (int r = 0; r < c.R; r++) {
        int64_t v = waveSumSel(V[r], sel);
        if (lane == 0 && v) { size_t ix = (size_t)k0 * c.R + r; atomicAddI64(&d.qDemandByPc[ix], v); if (!queued) atomicAddI64(&d.qAllocByPc[ix], v); }
      }
      todo &= ~sel;
    }
  }
}
// the fit bitmaps of a fresh base (round_fast.h fitBitsWord): one thread per (fit shape, 64 entries)
__global__ void k_base_fitbits(Dev d) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)d.f.F * d.fitW;
  if (i >= total) return;
  d.fitBits[i] = fitBitsWord(d, (int)(i / d.fitW), (int)(i % d.fitW));
}
__global__ void k_drf(Dev d, const int64_t* alloc, double* out) { if (threadIdx.x == 0) *out = drf(d, alloc); }
__global__ void k_fair(Dev d, const double* cds) { if (threadIdx.x == 0) updateFairShares(d, cds); }

// ------------------------------------------------------------------------------------------------ platform layer
// Everything a handle needs from the HIP runtime lives in its PlatCtx: device ordinal, launch stream, events, the helper mailbox, the
// host-mapped cancel word.  Handles are independent — two pools on two GPUs in one process, one thread per handle (include/armada_sched.h).
// Every ABI entry starts with plat_enter(handle context): hipSetDevice for the calling thread (the current device is thread-local in HIP,
// and a goroutine may run on any OS thread) and the thread-local pointer the plat_* helpers below work on.
struct HelpBox;
struct PlatCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, fitEv0 = nullptr, fitEv1 = nullptr;
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
  float roundTotalMs = 0.f, roundControlMs = 0.f; int roundLaunches = 0;
  int32_t* cmpScratch = nullptr; size_t cmpScratchInts = 0;   // block counts + total of the grid-wide compaction
  int optIndexN = -1, optIndexM = -1;   // sizes the optimiser's node -> jobs index in the scratch was built for (asched_host.inc decides when it may be reused)
  void* fitScratch = nullptr; size_t fitScratchBytes = 0;   // keys + shape list of a fit batch
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
            hipEventCreate(&c->fitEv0) == hipSuccess && hipEventCreate(&c->fitEv1) == hipSuccess && hipEventCreate(&c->rEv0) == hipSuccess && hipEventCreate(&c->rEv1) == hipSuccess;
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
  for (hipEvent_t e : {c->ev0, c->ev1, c->fitEv0, c->fitEv1, c->rEv0, c->rEv1}) if (e) (void)hipEventDestroy(e);
  if (c->helpBox) (void)hipFree(c->helpBox);
  if (c->cmpScratch) (void)hipFree(c->cmpScratch);
  if (c->optScratch) (void)hipFree(c->optScratch);
  if (c->optSel) (void)hipFree(c->optSel);
  if (c->fitScratch) (void)hipFree(c->fitScratch);
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
static int plat_opt_score(Dev& d, const OptArgs& a, std::vector<OptNodeOut>& scores, double* jobCost, int detailNode, OptNodeOut* detail, std::vector<int32_t>* pre, bool detailOnly = false,
                          bool reuseIndex = false) {   // detailOnly: the index and scores of the previous call are still in the scratch; reuseIndex: so is the node -> jobs index (nothing was bound since)
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
    // pad region beyond nb2 is never touched: the tile kernel is only used when the array is a multiple of 4096
    for (int k = 2; k <= nb2; k <<= 1) for (int j = k >> 1; j > 0; j >>= 1) hipLaunchKernelGGL(k_bitonic_step, dim3((nb2 + 255) / 256), dim3(256), 0, t_ctx->stream, a, j, k);
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
static int plat_run_fit_batch(Dev& d, const std::vector<int32_t>& shapes, int level, std::vector<int32_t>& out, const int32_t* nodeByRankHost = nullptr) {
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

#include "asched_host.inc"


#ifdef HELP_TRACE
extern "C" int asched_debug_help_trace(unsigned long long* out64) { return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_traceSum), 64 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1; }
#endif
