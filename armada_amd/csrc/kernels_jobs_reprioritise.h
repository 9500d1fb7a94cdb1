// kernels_jobs_reprioritise.h — asched_jobs_reprioritise: the priority within its queue (queue_priority) of a few rows of the resident job table changes between two
// scheduling cycles (the library's counterpart of `armadactl reprioritize`: jobdb/reconciliation.go:198-200 records the requested priority, scheduler.go:1198-1199
// applies it with job.WithPriority, jobdb/job.go:523, and Txn.Upsert takes the job out of its queue's sorted set and puts it back under the new key,
// jobdb/jobdb.go:583-587 and :695-699).  Nothing here goes through the round kernel: armada_sched_mgpu.hip runs jrScatter on the whole grid, the CPU build of the tests
// runs it serially (the driver at the end of this file).
//
// WHAT DEPENDS ON THE QUEUE PRIORITY: the second word of the order key (jobdb/comparison.go:70-79), so the pre-sorted job order ordAll and nothing else — no shape, no
// mask, no JobRec, no gang, no key layout; and no segment offset, because neither a row's queue nor its "active run" bit changes.
//
// THE PASSES (asched_host.inc asched_jobs_reprioritise queues them):
//   scatter + keys, over the n entries padded to a power of two: entry i writes the queue priority of its row, clears the row's keep flag and leaves the row's NEW key
//     in the sort array (rows named at most once: the thread reads back only what it wrote).  A row of no queue is in no order: its slot, like the padding, is a
//     sentinel that sorts behind every real key.  No run field and no JobRec is written.
//   remove, sort the touched keys, merge by rank: the passes of the patch (kernels_jobs_patch.h), unchanged — a kept row's key did not change, so what remains of ordAll
//     is still ascending.  The host swaps the two order buffers.
#pragma once
#include "kernels_jobs_patch.h"

struct JrArgs {   // everything in platform memory
  const uint32_t* pQPrio;   // [p.n] the new queue priorities of the rows p.pJob
  uint32_t* jQPrio;         // [M] the patch's order-key input, writable (p.jQPrio is the same array)
  JpArgs p;                 // the entries p.pJob [p.n] (p.pNode / p.pPrio / p.pTs unused), the order-key inputs, the sort array p.keys [p.nb2] and the merge, as for the patch
};

// slot i < nb2 of the sort array; i < n: entry i first
JP_FN void jrScatter(const Dev& d, const JrArgs& a, int i) {
  JpKey k; k.a = ~0ull; k.b = 0; k.t1 = 0; k.t2 = 0; k.idx = INT32_MAX; k.pad_ = 0;   // behind every real key (a queue has 31 bits)
  if (i < a.p.n) {
    const int j = a.p.pJob[i];
    a.jQPrio[j] = a.pQPrio[i];
    a.p.keep[j] = 0;
    if (d.jQueue[j] >= 0) k = jpKeyOf(d, a.p, j);
  }
  if (a.p.keys) a.p.keys[i] = k;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_jobs_reprioritise (plat.h): the scatter one element after the other, then the patch's remove / sort / merge
// a.p.nT == 0 (no entry names a row of a queue): a.p.keys == nullptr, a.p.nb2 == a.p.n, and the order is left alone
static int plat_jobs_reprioritise(Dev& d, JrArgs& a, int32_t* keptBuf) {
  for (int i = 0; i < a.p.nb2; i++) jrScatter(d, a, i);
  return plat_jobs_reseat(d, a.p, keptBuf);
}
#endif
