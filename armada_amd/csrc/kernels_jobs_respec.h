// kernels_jobs_respec.h — asched_jobs_respec: a few queued rows of the resident job table change their requirement class and / or their request vector between two
// scheduling cycles (the library's counterpart of a retry: when a run fails and the job is requeued, scheduler.go:1342-1383 rewrites its scheduling requirements through
// job.WithJobSchedulingInfo — node anti-affinity against every attempted run, createSchedulingInfoWithNodeAntiAffinityForAttemptedRuns :637-658, adopted at :1369-1376;
// the retry policy's memory bump, createSchedulingInfoWithMemoryBump :683 ff., adopted at :1347-1354).  Nothing here goes through the round kernel:
// armada_sched_mgpu.hip runs jsScatter on the whole grid, the CPU build of the tests runs it serially (the driver at the end of this file).
//
// WHAT DEPENDS ON CLASS AND REQUEST OF A QUEUED ROW: its scheduling-key shape (jShape), its request words (jReq), whether the request lies on the index grid
// (jAligned) and, where the fast structure has records, everything of its JobRec that the shape fixes.  NOT the pre-sorted order: the order key is built from queue,
// "has a run", priority-class priority, queue priority, time stamps and row (jpKeyOf, jaFill), so no key is written, nothing is sorted and nothing is merged.  No run
// field either: the rows have no run.  What a NEW shape adds to the shape-dependent tables is the host's business (asched_host.inc: the steps shared with
// asched_jobs_append) and is in place before this pass runs.
//
// THE PASS (asched_host.inc asched_jobs_respec queues it): one entry per row whose (class, request) changes, every row named at most once, so the pass needs no
// atomic.  Entry i writes the three arrays above and the row's JobRec.  The record's source is a resident row of the target shape that NO entry of this call names
// (a.pSrc: no thread reads a record another thread writes) or the template record the host built for the shape (a.tpl / a.pTpl: 128 bytes a shape, not a row); the
// row's own fields — gang, node0, runPrio, nlRun — are read from its old record first and kept.
#pragma once
#include "kernels_jobs_patch.h"

struct JsArgs {   // everything in platform memory
  int32_t n, R;               // n: entries, the rows whose class or request changes
  int32_t writeRec, pad0_;    // writeRec: the fast structure has records and no rebuild follows
  const int32_t *pJob, *pShape, *pSrc, *pTpl;   // [n] the row, its new shape, a resident row of that shape no entry names (-1: none), its template (-1: none)
  const uint8_t* pAligned;    // [n]
  const int64_t* pReq;        // [n][R]
  const JobRec* tpl;          // one template record per shape some entry has no source row for, or NULL
};

JP_FN void jsScatter(const Dev& d, const JsArgs& a, int i) {
  if (i >= a.n) return;
  const int j = a.pJob[i];
  d.jShape[j] = a.pShape[i];
  d.jAligned[j] = a.pAligned[i];
  for (int r = 0; r < a.R; r++) d.jReq[(size_t)j * a.R + r] = a.pReq[(size_t)i * a.R + r];
  const bool fromTpl = a.tpl && a.pSrc[i] < 0 && a.pTpl[i] >= 0;
  if (a.writeRec && d.jrec && (a.pSrc[i] >= 0 || fromTpl)) {
    JobRec r = fromTpl ? a.tpl[a.pTpl[i]] : d.jrec[a.pSrc[i]];   // everything the shape fixes (jaFill)
    const JobRec own = d.jrec[j];
    r.gang = own.gang; r.node0 = own.node0; r.runPrio = own.runPrio; r.nlRun = own.nlRun;
    d.jrec[j] = r;
  }
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_jobs_respec (plat.h): the same per-element function, one entry after the other
static int plat_jobs_respec(Dev& d, JsArgs& a) {
  for (int i = 0; i < a.n; i++) jsScatter(d, a, i);
  return 0;
}
#endif
