// kernels_round_commit.h — asched_round_commit: the result of the round the handle holds is applied to the resident job table (the library's counterpart of the two
// Upserts a pool's cycle ends with, txn.Upsert(preemptedJobs) / txn.Upsert(scheduledJobs), scheduling/scheduling_algo.go:276-285 with the jobs of :956-981: a scheduled
// job gets a new run on its node at GetScheduledAtPriority, a preempted job loses its run).  The lists are the ones the round left on the device — d.resJob / resNode /
// resPrio (B_GATHER_SCHED, round_run.h) and d.resPreJob — so nothing is uploaded but the caller's own entries (the runs that ended, ...).  Nothing here goes through the
// round kernel: armada_sched_mgpu.hip runs rcScatter on the whole grid, the CPU build of the tests runs it serially (the driver at the end of this file).
//
// THE PASSES (asched_host.inc asched_round_commit queues them):
//   scatter + keys, over the n = nx + ns + np entries padded to a power of two: slot i takes its entry from the uploaded extras (i < nx), from the scheduled list with
//     the lease time ts0 + k * tsStep of position k, or from the preempted list (node -1, priority 0, timestamp 0); writes the run fields of its row and of the row's
//     JobRec, clears the row's keep flag and leaves the row's NEW key in the sort array (jpSeat, kernels_jobs_patch.h: the arithmetic of the patch).  The row goes into
//     p.pJob[i] as well: the last leg of jpMerge sets the keep flags again from that array.  Rows are named at most once over the three sources (the host checks the
//     extras against the lists; the lists are compactions of two disjoint flag arrays).
//   remove, sort the touched keys, merge by rank: the passes of the patch (kernels_jobs_patch.h), unchanged.  The host swaps the two order buffers.
#pragma once
#include "kernels_jobs_patch.h"

struct RcArgs {   // everything in platform memory
  int32_t nx, ns, np, pad_;   // extras, scheduled, preempted: p.n = nx + ns + np
  int64_t ts0, tsStep;        // the lease of position k of the scheduled list: ts0 + k * tsStep (ns)
  int32_t* pJobW;             // [p.n] p.pJob, writable: [0, nx) uploaded, the rest written by the scatter
  JpArgs p;                   // the extras p.pJob / pNode / pPrio / pTs [nx], the order-key inputs, the sort array p.keys [p.nb2] and the merge, as for the patch
};

// slot i < nb2 of the sort array; i < n: entry i first
JP_FN void rcScatter(const Dev& d, const RcArgs& a, int i) {
  JpKey k = jpSentinel();
  if (i < a.p.n) {
    int j, node = -1, prio = 0;
    int64_t ts = 0;
    if (i < a.nx) { j = a.p.pJob[i]; node = a.p.pNode[i]; prio = a.p.pPrio[i]; ts = a.p.pTs[i]; }
    else if (i < a.nx + a.ns) {
      const int s = i - a.nx;
      j = d.resJob[s]; node = d.resNode[s]; prio = d.resPrio[s];
      ts = (int64_t)((uint64_t)a.ts0 + (uint64_t)s * (uint64_t)a.tsStep);   // (wraps as the host's mirror does: no signed overflow)
    } else j = d.resPreJob[i - a.nx - a.ns];
    if (i >= a.nx) a.pJobW[i] = j;
    k = jpSeat(d, a.p, j, node, prio, ts);
  }
  if (a.p.keys) a.p.keys[i] = k;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_round_commit (plat.h): the scatter one element after the other, then the patch's remove / sort / merge
// a.p.nT == 0 (no entry names a row of a queue): a.p.keys == nullptr, a.p.nb2 == a.p.n, and the order is left alone
static int plat_round_commit(Dev& d, RcArgs& a, int32_t* keptBuf) {
  for (int i = 0; i < a.p.nb2; i++) rcScatter(d, a, i);
  return plat_jobs_reseat(d, a.p, keptBuf);
}
#endif
