// kernels_opt.h — grid-wide kernels of the fairness optimiser (round_opt.h: node -> jobs index, queue costs, per-node scores one thread or one wave
// per node, the device-side candidate selection) and of the indicative gang pricer (round_price.h).  Defined in armada_sched.hip's code object only;
// launched by plat_hip.inc (plat_opt_score, plat_opt_select, plat_opt_qcosts, plat_price_score) for the asched_optimiser_* / asched_price_* entries.
#pragma once
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
