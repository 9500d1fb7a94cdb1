// kernels_preempt_join.h — PopulatePreemptionDescriptions (preemption_description.go:21-81) as a grid-wide join over the compacted result lists of a round:
// one record per preempted job (type, preemptor, sibling, slice of candidates) and the candidate list — the jobs scheduled with urgency preemption, grouped
// by node (calculateJobsScheduledWithUrgencyBasedPreemptionByNode :67-81).  Nothing here goes through the round kernel; armada_sched_mgpu.hip runs the
// per-element functions below one element per thread, the CPU build of the tests runs them serially (the driver at the end of this file).
//
// THE PASSES.  count: every scheduled entry with method URGENCY adds one to its node's counter.  scan: exclusive prefix sum of the N counters — per tile of
// PJ_TILE counters a sum, the tile sums scanned by one workgroup (a loop with a carry: any number of tiles), then every tile scanned again behind its offset;
// off[N] is the number of candidates.  scatter: every urgency entry takes the next free slot of its node's segment (an atomic cursor: the slots of a segment
// are filled in whatever order the hardware serves the atomics) and leaves its LIST POSITION there.  rank: every slot counts the positions of its segment
// that are smaller than its own and writes its job at that rank — the segment comes out in list order whatever order the scatter filled it in, so two runs
// give the same bytes.  The result lists of a round are ascending by job, so "list order" is the ABI's rule "ascending job index"; on the caller's own lists
// (asched_preemption_join) it is a stable sort by node.  The rank pass costs the sum of the squared segment lengths: a segment is the jobs ONE node took by
// urgency preemption in one round, tens at most on real nodes; every lane of a wave reads the same word of the segment at a time.
// cause: one record per preempted job, the tests in the reference's order (:25-63) — optimiser victim (its description is already set: :25-27), a
// preemptor on record (fair share, with or without a sibling), the node's slice not empty (urgency), in a gang, otherwise unknown.
#pragma once
#include "dev.h"
#include "../../include/armada_sched.h"

#ifndef PJ_FN   // the CPU build: serial
#define PJ_FN static inline
#define PJ_ADD32(p, v) ((*(p) += (v)) - (v))   // returns the old value, like atomicAdd
#endif

#define PJ_TILE 1024            // counters per tile of the scan: 256 threads x 4 consecutive counters
#define PJ_SIB_OPTIMISER (-2)   // preempted_sibling of an optimiser victim on the way IN (dev.h jcPreSib); the record that goes out carries -1

struct PjArgs {   // everything in platform memory
  int32_t N, ns, np, fromRound;
  const int32_t *sJob, *sNode, *sMethod;   // [ns] scheduled list
  const int32_t* pNode;                    // [np] node of each preempted job
  int32_t *pBy, *pSib; uint8_t* pGang;     // [np] preemptor / sibling / "in a gang": the caller's, or gathered from the round's per-job state (fromRound)
  int32_t *cnt, *off;                      // [N + 1] urgency entries per node (zeroed by the caller), their exclusive prefix sum
  int32_t* cursor;                         // [N] next free slot of each node's segment
  int32_t* tileSum;                        // [tiles] sums, then offsets, of the scan's tiles
  int32_t* slot;                           // [ns] list position of the entry that took a slot
  int32_t* cand;                           // [ns] candidate jobs, grouped by node, list order within a node
  asched_preemption_cause* cause;          // [np]
  int32_t* info;                           // [2], zeroed by the caller: marked jobs without a preemptor on record (an internal error), entries whose node is out of range
};
static inline int pjTiles(int N) { return (N + PJ_TILE - 1) / PJ_TILE; }

PJ_FN bool pjIsCandidate(const PjArgs& a, int i) { return a.sMethod[i] == ASCHED_METHOD_URGENCY && a.sNode[i] >= 0 && a.sNode[i] < a.N; }
PJ_FN void pjCount(const PjArgs& a, int i) {   // i < ns
  if (pjIsCandidate(a, i)) PJ_ADD32(a.cnt + a.sNode[i], 1);
  else if (a.sMethod[i] == ASCHED_METHOD_URGENCY) PJ_ADD32(a.info + 1, 1);
}
PJ_FN void pjScatter(const PjArgs& a, int i) {   // i < ns
  if (pjIsCandidate(a, i)) a.slot[PJ_ADD32(a.cursor + a.sNode[i], 1)] = i;
}
PJ_FN void pjRank(const PjArgs& a, int k) {   // k < off[N]
  int pos = a.slot[k], n = a.sNode[pos], beg = a.off[n], end = a.off[n + 1], r = 0;
  for (int e = beg; e < end; e++) r += a.slot[e] < pos ? 1 : 0;
  a.cand[beg + r] = a.sJob[pos];
}
// the per-job state of the round behind preempted entry i (dev.h jcStagedBy / jcPreSib / jcPreempted, asched_round_result.preempted_job)
PJ_FN void pjGather(const Dev& d, const PjArgs& a, int i) {   // i < np
  int j = d.resPreJob[i];
  int sib = d.jcPreSib[j], by = d.jcStagedBy[j];
  bool marked = d.jcPreempted[j] != 0, opt = sib == PJ_SIB_OPTIMISER;
  if (!marked && !opt) { by = -1; sib = -1; }
  if (marked && by < 0) PJ_ADD32(a.info + 0, 1);
  a.pBy[i] = by; a.pSib[i] = sib; a.pGang[i] = d.jGang[j] >= 0 ? 1 : 0;
}
PJ_FN void pjCause(const PjArgs& a, int i) {   // i < np
  asched_preemption_cause c;
  c.type = ASCHED_PREEMPTION_UNKNOWN; c.preempting_job = -1; c.preempted_sibling = -1; c.cand_off = 0; c.cand_count = 0; c.pad_ = 0;
  int n = a.pNode[i], by = a.pBy[i], sib = a.pSib[i];
  int beg = 0, end = 0;
  if (n >= 0 && n < a.N) { beg = a.off[n]; end = a.off[n + 1]; }
  if (sib == PJ_SIB_OPTIMISER) { c.type = ASCHED_PREEMPTION_OPTIMISER; c.preempting_job = by; }
  else if (by >= 0) { c.type = ASCHED_PREEMPTION_FAIRSHARE; c.preempting_job = by; c.preempted_sibling = sib >= 0 ? sib : -1; }
  else if (end > beg) { c.type = ASCHED_PREEMPTION_URGENCY; c.cand_off = beg; c.cand_count = end - beg; }
  else if (a.pGang[i]) c.type = ASCHED_PREEMPTION_UNKNOWN_GANG;
  a.cause[i] = c;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_preempt_join (plat.h): the same per-element functions serially; the scan is a running sum
static int plat_preempt_join(Dev& d, const PjArgs& a) {
  for (int i = 0; i < a.ns; i++) pjCount(a, i);
  int run = 0;
  for (int n = 0; n < a.N; n++) { a.off[n] = run; a.cursor[n] = run; run += a.cnt[n]; }
  a.off[a.N] = run;
  for (int i = a.ns - 1; i >= 0; i--) pjScatter(a, i);   // (backwards: the rank pass, not the scatter, makes the order)
  for (int k = 0; k < run; k++) pjRank(a, k);
  if (a.fromRound) for (int i = 0; i < a.np; i++) pjGather(d, a, i);
  for (int i = 0; i < a.np; i++) pjCause(a, i);
  return 0;
}
#endif
