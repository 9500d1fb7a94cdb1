// kernels_jobs_delete.h — asched_jobs_delete: rows leave the resident job table between two scheduling cycles (the library's counterpart of syncState's delete of every
// job in a terminal state from the jobDb, scheduler.go:539-549; Txn.BatchDelete / delete, jobdb/jobdb.go:941-990).  The remaining rows keep their order and are renumbered
// densely: new id = old id - deleted rows below it.  Nothing here goes through the round kernel: armada_sched_mgpu.hip runs the per-element functions below on the whole
// grid, the CPU build of the tests runs them serially (the driver at the end of this file).
//
// WHAT DEPENDS ON A ROW ID: the position of a row in every per-job array, the entries of the pre-sorted order ordAll and the members' list of the gang CSR (gangJobs).  A
// JobRec holds no row id (dev.h): records are moved, never refilled.  Shape ids and dense gang ids stay as they are.
//
// THE PASSES (asched_host.inc asched_jobs_delete queues them through plat_jobs_delete):
//   mark: entry i clears the keep flag of its row (the flags of the patch, all 1 between calls).
//   scan: plat_compact over the M keep flags — the survivors' list src[new] = old, the exclusive prefix (= the new id of a surviving row) and the new M.
//   gather: out[new] = in[src[new]] for every static per-job array, into fresh blocks the host swaps in (a grid cannot compact in place).  Three launches, each reading src
//     once: the narrow arrays (one thread per row), the requests (one thread per 8-byte element, R consecutive threads on one row), the JobRec table (eight lanes to a
//     128-byte record, 16 bytes each: a wave moves eight whole records per instruction).
//   order: plat_compact of ordAll by the keep flag of its entries into the spare order buffer, then every entry through the new-id map.  Relative ids are preserved and no
//     key changes: what remains is still ascending.
//   gang CSR: the same two steps on gangJobs.
//   unmark: entry i sets the keep flag of its row again — the flags are indexed by the OLD id during the call and all 1 over the new M afterwards.
#pragma once
#include "kernels_jobs_patch.h"

#ifndef JD_FN   // the CPU build: serial
#define JD_FN static inline
#endif

#define JD_N32 9   // the 4-byte per-job arrays: jQueue, jPc, jShape, jGang, jGangCard, jGangUni, jNode0, jRunPrio, and the patch's queue priorities

struct alignas(16) JdQuad { uint32_t x, y, z, w; };   // a sixteenth of a cache line: one vector load / store
static_assert(sizeof(JobRec) % sizeof(JdQuad) == 0 && sizeof(JobRec) / sizeof(JdQuad) == 8, "eight lanes move one JobRec");

struct JdArgs {   // everything in platform memory
  int32_t M, M1, n, R;         // M: rows before the call; M1: rows after it (known once the scan is through); n: entries
  int32_t total, total1;       // length of ordAll before / after
  int32_t gangLen, gangLen1;   // gangOff[G] before / after
  const int32_t* job;          // [n] the rows to delete
  uint8_t* keep;               // [M]
  int32_t* src;                // [M] the survivors: src[new] = old
  uint32_t* newId;             // [M] kept rows below a row: the new id of a surviving one
  const int32_t* in32[JD_N32]; int32_t* out32[JD_N32];   // a NULL pair is skipped (the queue priorities of a table no patch or append has touched yet: the host uploads them)
  const uint8_t *inAway, *inAligned; uint8_t *outAway, *outAligned;   // inAway NULL: the table has no away rows
  const int64_t *inLease, *inSubmit, *inRunTs, *inReq; int64_t *outLease, *outSubmit, *outRunTs, *outReq;   // inSubmit / inRunTs NULL: as the queue priorities
  const JobRec* inRec; JobRec* outRec;                   // NULL: no fast structure
  int32_t *ordIn, *ordOut;     // ordAll [total] and the spare order buffer (>= total1)
  int32_t *gangIn, *gangOut;   // gangJobs [gangLen] and a scratch list (>= gangLen1); the host copies the result back over gangJobs
};

JD_FN void jdMark(const JdArgs& a, int i, uint8_t v) { a.keep[a.job[i]] = v; }
// new row i: the narrow arrays
JD_FN void jdNarrow(const JdArgs& a, int i) {
  const int s = a.src[i];
  for (int k = 0; k < JD_N32; k++) if (a.in32[k]) a.out32[k][i] = a.in32[k][s];
  if (a.inAway) a.outAway[i] = a.inAway[s];
  a.outAligned[i] = a.inAligned[s];
  a.outLease[i] = a.inLease[s];
  if (a.inSubmit) a.outSubmit[i] = a.inSubmit[s];
  if (a.inRunTs) a.outRunTs[i] = a.inRunTs[s];
}
// element e < M1 * R of the request table
JD_FN void jdReq(const JdArgs& a, long long e) {
  const long long i = e / a.R; const int r = (int)(e - i * a.R);
  a.outReq[e] = a.inReq[(long long)a.src[i] * a.R + r];
}
// sixteen bytes t < M1 * 8 of the JobRec table
JD_FN void jdRec(const JdArgs& a, long long t) {
  const long long i = t >> 3; const int l = (int)(t & 7);
  ((JdQuad*)(a.outRec + i))[l] = ((const JdQuad*)(a.inRec + a.src[i]))[l];
}
// a compacted list of surviving rows, still in old ids
JD_FN void jdRemap(const JdArgs& a, int32_t* list, int i) { list[i] = (int32_t)a.newId[list[i]]; }

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_jobs_delete (plat.h): the same per-element functions, one element after the other
static int plat_jobs_delete(Dev& d, JdArgs& a) {
  for (int i = 0; i < a.n; i++) jdMark(a, i, 0);
  int m1 = 0;
  if (plat_compact(d, nullptr, a.M, a.keep, a.src, a.newId, nullptr, 0, nullptr, &m1)) return -1;
  if (m1 != a.M1) { g_err = "jobs_delete: the scan kept another number of rows than the host counted"; return -1; }
  for (int i = 0; i < a.M1; i++) jdNarrow(a, i);
  for (long long e = 0; e < (long long)a.M1 * a.R; e++) jdReq(a, e);
  if (a.inRec) for (long long t = 0; t < (long long)a.M1 * 8; t++) jdRec(a, t);
  if (a.total > 0) {
    int t1 = 0;
    if (plat_compact(d, a.ordIn, a.total, a.keep, a.ordOut, nullptr, nullptr, 0, nullptr, &t1)) return -1;
    if (t1 != a.total1) { g_err = "jobs_delete: the job order lost or gained rows"; return -1; }
    for (int i = 0; i < a.total1; i++) jdRemap(a, a.ordOut, i);
  }
  if (a.gangLen > 0) {
    int g1 = 0;
    if (plat_compact(d, a.gangIn, a.gangLen, a.keep, a.gangOut, nullptr, nullptr, 0, nullptr, &g1)) return -1;
    if (g1 != a.gangLen1) { g_err = "jobs_delete: the gang lists lost or gained rows"; return -1; }
    for (int i = 0; i < a.gangLen1; i++) jdRemap(a, a.gangOut, i);
  }
  for (int i = 0; i < a.n; i++) jdMark(a, i, 1);
  return 0;
}
#endif
