// kernels_split.h — grid-wide kernels of the split round: bulk passes, the small serial steps, eviction with wave-level pre-reduction, and the
// order-preserving compaction (count / scan / write / segment offsets).  Defined in armada_sched.hip's code object only; launched by plat_hip.inc
// (plat_bulk, plat_small, plat_evict_apply, plat_compact) for asched_host.inc runRoundSplit.  waveSumSel is shared with k_agg (kernels_fit.h).
#pragma once
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
