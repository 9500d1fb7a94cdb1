// kernels_queued_lists.h — asched_round_prepare_resident: the queued lists of a round derived from the resident job order instead of handed in by the caller (the library's
// counterpart of NewQueuedJobsIterator reading repo.QueuedJobs(queue, pool, sortOrder), scheduling/jobiteration.go:144-160: a view of the resident jobDb, not a list built
// per cycle).  Nothing here goes through the round kernel: armada_sched_mgpu.hip runs the per-element functions below on the whole grid, the CPU build of the tests runs
// them serially (the driver at the end of this file).
//
// WHAT THE LIST IS: dev.ordAll holds, per queue segment [ordAllOff[q], ordAllOff[q + 1]), the running rows and then the queued rows of queue q, each in
// SchedulingOrderCompare order; jobs_patch / jobs_append / jobs_delete keep it exact.  The queued list of queue q is the order-preserving compaction of q's segment by
// "the row has no run and is not held".  Segments are consecutive and ascending in q, so ONE compaction over [0, ordAllOff[Q]) yields all Q lists back to back, and
// queuedOff[q] is the number of flagged entries in front of ordAllOff[q] (plat_compact's prefix at the segment offsets: DESIGN 3.15).
//
// THE PASSES (asched_host.inc roundPrepareBody queues them through plat_queued_lists):
//   mark: one flag byte per row, jNode0[j] < 0 && (unsigned)jQueue[j] < Q.  A thread takes FOUR consecutive rows and stores one 32-bit word (byte k = row 4w + k), so no
//     lane issues a byte store; where both columns are 16-byte aligned (a.vec) it reads each with one 128-bit load.  The flag block is a whole number of words: the bytes
//     of the last word at or beyond M are written as 0 and never read (every entry of ordAll is a row < M).
//   hold: one thread per held entry clears the flag of its row — a plain store of 0, so duplicates are idempotent; a held row that has a run had 0 already.  After mark,
//     on the same stream.
//   compact: plat_compact(ordAll, ordAllOff[Q], flag, list, prefix, ordAllOff, Q, off, &total), the call the evicted lists of every round go through.
#pragma once
#include "dev.h"
#include "../../include/armada_sched.h"

#ifndef QL_FN   // the CPU build: serial
#define QL_FN static inline
#endif

struct QlArgs {   // everything in platform memory
  int32_t M, Q, nHeld, vec;    // vec: jNode0 and jQueue are 16-byte aligned (the 128-bit loads of a full word)
  const int32_t *jNode0, *jQueue;   // [M]
  const int32_t* held;         // [nHeld] rows in [0, M)
  uint8_t* flag;               // [4 * ceil(M / 4)]
};

struct QlRows4 { int32_t v[4]; };

// word w < ceil(M / 4) of the flag block: rows 4w .. 4w + 3
QL_FN void qlMarkWord(const QlArgs& a, int w) {
  const int j0 = 4 * w;
  uint32_t word = 0;
  if (a.vec && j0 + 4 <= a.M) {
    QlRows4 n, q;
    __builtin_memcpy(&n, __builtin_assume_aligned(a.jNode0 + j0, 16), 16);
    __builtin_memcpy(&q, __builtin_assume_aligned(a.jQueue + j0, 16), 16);
    for (int k = 0; k < 4; k++) if (n.v[k] < 0 && (uint32_t)q.v[k] < (uint32_t)a.Q) word |= 1u << (8 * k);
  } else {
    for (int k = 0; k < 4; k++) { const int j = j0 + k; if (j < a.M && a.jNode0[j] < 0 && (uint32_t)a.jQueue[j] < (uint32_t)a.Q) word |= 1u << (8 * k); }   // (the tail M % 4: no row at or beyond M is read)
  }
  ((uint32_t*)a.flag)[w] = word;
}
// held entry i < nHeld
QL_FN void qlHold(const QlArgs& a, int i) { a.flag[a.held[i]] = 0; }

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_queued_lists (plat.h): the same per-element functions, one element after the other, then the CPU build's plat_compact
static int plat_queued_lists(Dev& d, const QlArgs& a, int ordTotal, int32_t* list, uint32_t* prefix, int32_t* off, int* total) {
  for (int w = 0; w < (a.M + 3) / 4; w++) qlMarkWord(a, w);
  for (int i = 0; i < a.nHeld; i++) qlHold(a, i);
  return plat_compact(d, d.ordAll, ordTotal, a.flag, list, prefix, d.ordAllOff, a.Q, off, total);
}
#endif
