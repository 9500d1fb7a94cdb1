// kernels_jobs_patch.h — asched_jobs_patch: the run state of a few rows of the resident job table changes between two scheduling cycles (the library's counterpart of
// jobdb.Txn.Upsert for the jobs a round leased or preempted, scheduling/scheduling_algo.go:280-283; jobdb/jobdb.go:572-700 re-seats only those jobs in the per-queue
// sorted sets).  Nothing here goes through the round kernel: armada_sched_mgpu.hip runs the per-element functions below on the whole grid, the CPU build of the tests
// runs them serially (the driver at the end of this file).
//
// WHAT DEPENDS ON RUN STATE: jNode0 / jRunPrio / jLeaseMs, the three run fields of a JobRec (node0, runPrio, nlRun), and the pre-sorted job order ordAll.  ordAll is the
// jobs of every queue >= 0, queue after queue, each queue in SchedulingOrderCompare order (jobdb/comparison.go:49-107) — as ONE order it is ascending under the key
//   (queue, no active run, priority-class priority descending, queue priority, run timestamp | submit time, submit time, row)
// and a patch changes only the "active run" bit and the run timestamp of the named rows: no job changes queue, so the segment offsets (ordAllOff) stay as they are.
//
// THE PASSES (asched_host.inc asched_jobs_patch queues them):
//   scatter + keys, over the n entries padded to a power of two: entry i writes the run fields of its row, clears the row's keep flag and leaves the row's NEW key in the
//     sort array (rows named at most once: the thread reads back only what it wrote).  A row of no queue is in no order: its slot, like the padding, is a sentinel
//     that sorts behind every real key.
//   remove: the order-preserving compaction of the rows of ordAll whose keep flag is still set (plat_compact).  What remains is still ascending: a kept row's key did
//     not change.
//   sort the touched keys: a bitonic network on the 40-byte records, every step with a distance inside a tile of JP_TILE records in LDS, the others in HBM.  Keys are
//     unique (the row is the last field): the network needs no stability, and two runs give the same bytes.
//   merge by rank: two ascending sequences without a common key — a touched row lands at (its rank among the touched) + (kept rows below it: a binary search that
//     gathers the kept rows' keys), a kept row at (its rank among the kept) + (touched keys below it: a binary search in the sorted records).  Written into the second
//     ordAll buffer; the host swaps the two.  The same launch sets the keep flags again.
#pragma once
#include "dev.h"
#include "../../include/armada_sched.h"

#ifndef JP_FN   // the CPU build: serial
#define JP_FN static inline
#endif

#define JP_TILE 1024   // records of the sort array per workgroup of the in-LDS part of the network: 40 KB

struct JpKey { uint64_t a, b, t1, t2; int32_t idx, pad_; };   // the packed order key of jobs_set with the queue above it; idx: the row

struct JpArgs {   // everything in platform memory
  int32_t M, n, nb2, nT, nKept, total, pad0_, pad1_;   // nb2: n padded to a power of two >= JP_TILE; nT: entries of a queue >= 0; total: length of ordAll = nT + nKept
  const int32_t *pJob, *pNode, *pPrio;   // [n] the entries
  const int64_t* pTs;                    // [n]
  uint8_t* keep;                         // [M] 1 between calls; 0 for the rows of the call in progress (the compaction's flag)
  const uint32_t* jQPrio;                // [M] queue_priority
  const int64_t* jSubmit;                // [M] submit_time
  int64_t* jRunTs;                       // [M] run_timestamp (ns)
  JpKey* keys;                           // [nb2] the sort array
  const int32_t* kept;                   // [nKept] ordAll without the touched rows
  int32_t* out;                          // [total] the new order
};

// number of priority levels a bind at `cutoff` subtracts from (asched_host.inc buildFast: levels with priority <= cutoff, nodedb.go:1321-1334)
JP_FN int jpLevels(const DevCfg& c, int32_t cutoff) { int nl = 0; while (nl < c.P && c.prios[nl] <= cutoff) nl++; return nl; }

// the first word: queue, then active run first, then priority-class priority descending (comparison.go:49-79); queue >= 0
JP_FN uint64_t jpWordA(const Dev& d, int j, int q) {
  return ((uint64_t)(uint32_t)q << 33) | ((uint64_t)(d.jNode0[j] >= 0 ? 0 : 1) << 32) | (uint32_t)~((uint32_t)d.cfg.pcPriority[d.jPc[j]] ^ 0x80000000u);
}
JP_FN JpKey jpKeyOf(const Dev& d, const JpArgs& a, int j) {   // a row of a queue >= 0
  JpKey k;
  k.a = jpWordA(d, j, d.jQueue[j]);
  k.b = a.jQPrio[j];
  // both active: run timestamp, then submit time; otherwise submit time (:83-97); then the id order (:99-105)
  k.t1 = (uint64_t)(d.jNode0[j] >= 0 ? a.jRunTs[j] : a.jSubmit[j]) ^ (1ull << 63);
  k.t2 = (uint64_t)a.jSubmit[j] ^ (1ull << 63);
  k.idx = j; k.pad_ = 0;
  return k;
}
JP_FN bool jpLess(const JpKey& x, const JpKey& y) {
  if (x.a != y.a) return x.a < y.a;
  if (x.b != y.b) return x.b < y.b;
  if (x.t1 != y.t1) return x.t1 < y.t1;
  if (x.t2 != y.t2) return x.t2 < y.t2;
  return x.idx < y.idx;
}
// key(row j) < k, reading only as many of the row's fields as the comparison needs (most end at the first word)
JP_FN bool jpRowLess(const Dev& d, const JpArgs& a, int j, const JpKey& k) {
  uint64_t wa = jpWordA(d, j, d.jQueue[j]);
  if (wa != k.a) return wa < k.a;
  uint64_t b = a.jQPrio[j];
  if (b != k.b) return b < k.b;
  uint64_t t2 = (uint64_t)a.jSubmit[j] ^ (1ull << 63), t1 = d.jNode0[j] >= 0 ? (uint64_t)a.jRunTs[j] ^ (1ull << 63) : t2;
  if (t1 != k.t1) return t1 < k.t1;
  if (t2 != k.t2) return t2 < k.t2;
  return j < k.idx;
}

// the slot of a row of no queue and of the padding: behind every real key (a queue has 31 bits)
JP_FN JpKey jpSentinel() { JpKey k; k.a = ~0ull; k.b = 0; k.t1 = 0; k.t2 = 0; k.idx = INT32_MAX; k.pad_ = 0; return k; }
// row j now runs on `node` (-1: no run) at `prio`, leased at `ts`: its run fields and those of its JobRec, its keep flag, and -> its NEW key (the scatter of the patch
// and of the round commit, kernels_round_commit.h)
JP_FN JpKey jpSeat(const Dev& d, const JpArgs& a, int j, int node, int prio, int64_t ts) {
  d.jNode0[j] = node; d.jRunPrio[j] = prio; d.jLeaseMs[j] = ts / 1000000; a.jRunTs[j] = ts;
  a.keep[j] = 0;
  if (d.jrec) {
    JobRec& r = d.jrec[j];
    r.node0 = node; r.runPrio = prio; r.nlRun = (uint8_t)jpLevels(d.cfg, r.preemptible ? prio : INT32_MAX);
  }
  return d.jQueue[j] >= 0 ? jpKeyOf(d, a, j) : jpSentinel();
}
// slot i < nb2 of the sort array; i < n: entry i first
JP_FN void jpScatter(const Dev& d, const JpArgs& a, int i) {
  JpKey k = jpSentinel();
  if (i < a.n) k = jpSeat(d, a, a.pJob[i], a.pNode[i], a.pPrio[i], a.pTs[i]);
  if (a.keys) a.keys[i] = k;
}
// i < nT + nKept + n: the touched rows, the kept rows, the keep flags
JP_FN void jpMerge(const Dev& d, const JpArgs& a, long long i) {
  if (i < a.nT) {
    const JpKey k = a.keys[i];
    int lo = 0, hi = a.nKept;   // the kept rows below k
    while (lo < hi) { int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (jpRowLess(d, a, a.kept[mid], k)) lo = mid + 1; else hi = mid; }
    a.out[i + lo] = k.idx;
  } else if (i < (long long)a.nT + a.nKept) {
    const int p = (int)(i - a.nT), j = a.kept[p];
    const JpKey k = jpKeyOf(d, a, j);
    int lo = 0, hi = a.nT;      // the touched keys below k
    while (lo < hi) { int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (jpLess(a.keys[mid], k)) lo = mid + 1; else hi = mid; }
    a.out[p + lo] = j;
  } else {
    a.keep[a.pJob[i - a.nT - a.nKept]] = 1;
  }
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_jobs_patch (plat.h): the same per-element functions, one element after the other; the sort is the standard library's
// a.nT == 0 (no entry names a row of a queue): a.keys == nullptr, a.nb2 == a.n, and the order is left alone
// plat_jobs_reseat: everything behind the scatter — remove, sort, merge by rank (asched_jobs_reprioritise, kernels_jobs_reprioritise.h, ends with the same passes)
static int plat_jobs_reseat(Dev& d, JpArgs& a, int32_t* keptBuf) {
  a.kept = keptBuf; a.nKept = 0;
  if (a.nT > 0) {
    int nk = 0;
    if (plat_compact(d, d.ordAll, a.total, a.keep, keptBuf, nullptr, nullptr, 0, nullptr, &nk)) return -1;
    a.nKept = nk;
    if (a.nT + a.nKept != a.total) { g_err = "jobs_patch: the job order lost or gained rows"; return -1; }
    std::sort(a.keys, a.keys + a.nb2, [](const JpKey& x, const JpKey& y) { return jpLess(x, y); });
  }
  const long long work = (long long)a.nT + a.nKept + a.n;
  for (long long i = 0; i < work; i++) jpMerge(d, a, i);
  return 0;
}
static int plat_jobs_patch(Dev& d, JpArgs& a, int32_t* keptBuf) {
  for (int i = 0; i < a.nb2; i++) jpScatter(d, a, i);
  return plat_jobs_reseat(d, a, keptBuf);
}
#endif
