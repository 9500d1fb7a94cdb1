// kernels_evict_report.h — the EvictorResult of a round's balancing evictor (scheduling/eviction.go:27-79), recorded while phase 1 of the split round runs
// (asched_set_evictor_report / asched_round_evictor_report).  Nothing here goes through the round kernel: armada_sched_mgpu.hip runs the per-element functions
// below on the whole grid, the CPU build of the tests runs them serially (the driver at the end of this file).
//
// WHAT IS RECORDED, all of it as of the moment the node evictor of phase 1 runs (preempting_queue_scheduler.go:96-138):
//   per node n (Evictor.Evict, eviction.go:197-238): on(n) = the jobs with jobNode == n — node.AllocatedByJobId, the jobs already evicted on the node included (:213).
//     on(n) empty: the node filter of NewNodeEvictor skips the node (eviction.go:89-96): reasons = NODE_EMPTY, plus NODE_UNSCHEDULABLE on an unschedulable node, and
//     preemptible = !unschedulable (:200-208).  Otherwise reasons = the OR of reason(j) over the jobs of on(n) that are NOT evicted on the node (:214: EvictedJobRunIds
//     are passed over), plus NODE_UNSCHEDULABLE (:228-230); no bit: ALL_JOBS_PREEMPTIBLE and preemptible (:233-234), any bit: not preemptible (:236).
//   reason(j), the job filter's tests in the reference's order (preempting_queue_scheduler.go:101-136): a cross-pool away job -> 0 (:102-104: "don't fill in
//     cantPreemptReason"); a queue outside [0, Q) -> INVALID_QUEUE (:105-108); a priority class that is not preemptible -> JOB_NOT_PREEMPTIBLE (:120-122);
//     !qEvictable[queue] -> BELOW_PROTECTED_FAIR_SHARE (:124-134; qEvictable is what round_run.h SM_QEVICTABLE computes, !(actual / fair <= protectedFraction): a NaN
//     ratio counts as evictable, as in Go); anything else -> 0.  missing_annotations / missing_node_selector (:109-116) have no counterpart behind this boundary.
//   the evicted set: EvictedJctxsByJobId after evictGangs has been merged in (preempting_queue_scheduler.go:316-326) == evFlag after B_GANG_CLOSURE of phase 1; the
//     gang evictor's own node stats are discarded by the reference (:322-325 keeps its jobs and nodes only), and here.
//   per queue (GetStatsPerQueue, eviction.go:60-71): EvictedJobCount and EvictedResources = the sum of KubernetesResourceRequirements — the job's request row with
//     the floating columns (cfg.isFloating) as 0.
// The ASCHED_EVR_* bits are numbered in the alphabetical order of the reference's reason strings: ascending bit order is makeNodePreemptiblityStats' sorted,
// comma-joined string (eviction.go:275-285).
//
// THE PASSES (asched_host.inc evictPhaseSplit queues them; the host waits for none of them):
//   jobs, over M, after B_GANG_CLOSURE and before the evictor is applied (jobEvictedOnNode is still the start-of-round state): a job with a node adds itself to the
//     node's job count, ORs its reason (when not 0) into the node's word and, when evFlag is set, adds itself to the node's evicted count.  The job table is not
//     ordered by node and the handle keeps no per-node index of the running jobs at this point (fairOff / fairEnt index the EVICTED table, which the replay fills
//     later; the optimiser's index lives in its scratch and is built only when it runs), so this is a pass over the jobs with integer atomics — exact and
//     independent of their order: two runs give the same bytes.  Neighbouring lanes that name the same node are combined inside the wave first (a segmented scan by
//     shuffles; the last lane of a run touches memory): populateNodeDb's inputs usually come node by node.
//   nodes, over N: reasons and preemptible from the three words of the node; a node with an evicted job is an affected node (AffectedNodesById, eviction.go:261-263):
//     counted per wave by a ballot, per workgroup through LDS, one atomic per workgroup.
//   queues, over the compacted list evList[0, n1) (sorted by queue: evOff) in tiles of EVR_TILE entries, one per thread: the workgroup finds the queues of its first
//     and last entry by a search in evOff (a thread searches only between the two); per column a segmented inclusive scan by shuffles inside the wave, the waves'
//     trailing runs through LDS, and the lane that ends a queue's run inside the tile issues ONE 64-bit atomic add per column for the whole run — never one per job.
//     The same pass gathers evicted_node[p] = jobNode[evList[p]] and copies evList[0, n1) and evOff into the report's own buffers (phase 3 overwrites both).
#pragma once
#include "dev.h"
#include "../../include/armada_sched.h"

#ifndef EVR_FN   // the CPU build: serial
#define EVR_FN static inline
#endif

#define EVR_TILE 256   // entries of the evicted list per workgroup of the queue pass: one per thread of MG_THREADS

enum { EVR_PASS_JOBS = 0, EVR_PASS_NODES = 1, EVR_PASS_QUEUES = 2 };

struct EvrArgs {   // everything in platform memory
  int32_t N, M, Q, R, n1, pad_;
  const uint8_t* nodeUnsched;            // [N] node.IsUnschedulable()
  int32_t *nodeJobs, *nodeOr;            // [N] |on(n)|, OR of reason(j); zeroed by the caller before the job pass
  int32_t* nodeEvicted;                  // [N] jobs evicted from the node; zeroed likewise
  int32_t* affected;                     // [1] zeroed likewise
  uint8_t *nodePreemptible, *nodeReasons;   // [N]
  int32_t* qJobs;                        // [Q]
  int64_t* qRes;                         // [Q][R] zeroed by the caller
  int32_t* qOff;                         // [Q + 1] copy of evOff
  int32_t *evJob, *evNode;               // [n1] copy of evList, node of each entry
};

// the job filter's "why not" of NewNodeEvictor's caller for a job that is on a node and not evicted there
EVR_FN int evrReason(const Dev& d, int j) {
  const DevCfg& c = d.cfg;
  if (d.jAway && d.jAway[j]) return 0;
  int q = d.jQueue[j];
  if (q < 0 || q >= c.Q) return ASCHED_EVR_INVALID_QUEUE;
  if (!c.pcPreemptible[d.jPc[j]]) return ASCHED_EVR_JOB_NOT_PREEMPTIBLE;
  if (!d.qEvictable[q]) return ASCHED_EVR_BELOW_PROTECTED_FAIR_SHARE;
  return 0;
}
// what job j < M contributes to its node: *node = -1 when it is on none
EVR_FN void evrJobTerms(const Dev& d, const EvrArgs& a, int j, int* node, int* reason, int* evicted) {
  int n = d.jobNode[j];
  if (n < 0 || n >= a.N) { *node = -1; *reason = 0; *evicted = 0; return; }
  *node = n;
  *reason = d.jobEvictedOnNode[j] ? 0 : evrReason(d, j);
  *evicted = d.evFlag[j] ? 1 : 0;
}
// node n < N: 1 = an affected node
EVR_FN int evrNode(const EvrArgs& a, int n) {
  int reasons = a.nodeUnsched[n] ? ASCHED_EVR_NODE_UNSCHEDULABLE : 0, pre;
  if (a.nodeJobs[n] == 0) { pre = reasons ? 0 : 1; reasons |= ASCHED_EVR_NODE_EMPTY; }
  else {
    reasons |= a.nodeOr[n];
    pre = reasons ? 0 : 1;
    if (!reasons) reasons = ASCHED_EVR_ALL_JOBS_PREEMPTIBLE;
  }
  a.nodePreemptible[n] = (uint8_t)pre; a.nodeReasons[n] = (uint8_t)reasons;
  return a.nodeEvicted[n] > 0 ? 1 : 0;
}
// the queue of position p of the compacted list, known to lie in [lo, hi]: the last q with off[q] <= p
EVR_FN int evrQueueOf(const int32_t* off, int p, int lo, int hi) {
  while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (off[mid] <= p) lo = mid; else hi = mid - 1; }
  return lo;
}
// KubernetesResourceRequirements of a job, column r
EVR_FN int64_t evrReqCol(const Dev& d, int j, int r) { return d.cfg.isFloating[r] ? 0 : d.jReq[(size_t)j * d.cfg.R + r]; }
EVR_FN void evrGather(const Dev& d, const EvrArgs& a, int p) { int j = d.evList[p]; a.evJob[p] = j; a.evNode[p] = d.jobNode[j]; }   // p < n1
EVR_FN void evrCopyOff(const Dev& d, const EvrArgs& a, int q) { a.qOff[q] = d.evOff[q]; if (q < a.Q) a.qJobs[q] = d.evOff[q + 1] - d.evOff[q]; }   // q <= Q

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_evict_report (plat.h): the same per-element functions, one element after the other
static int plat_evict_report(Dev& d, const EvrArgs& a, int pass) {
  if ((pass == EVR_PASS_JOBS && a.M <= 0) || (pass == EVR_PASS_NODES && a.N <= 0)) return 0;
  if (pass == EVR_PASS_JOBS) {
    for (int j = 0; j < a.M; j++) {
      int n, reason, ev;
      evrJobTerms(d, a, j, &n, &reason, &ev);
      if (n >= 0) { a.nodeJobs[n]++; a.nodeOr[n] |= reason; a.nodeEvicted[n] += ev; }
    }
  } else if (pass == EVR_PASS_NODES) {
    for (int n = 0; n < a.N; n++) *a.affected += evrNode(a, n);
  } else {
    for (int p = 0; p < a.n1; p++) {
      int q = evrQueueOf(d.evOff, p, 0, a.Q - 1);
      for (int r = 0; r < a.R; r++) a.qRes[(size_t)q * a.R + r] += evrReqCol(d, d.evList[p], r);
      evrGather(d, a, p);
    }
    for (int q = 0; q <= a.Q; q++) evrCopyOff(d, a, q);
  }
  t_ctx->launches++;
  return 0;
}
#endif
