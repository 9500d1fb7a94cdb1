// kernels_nodes_delete.h — asched_nodes_delete: rows leave the resident node table between two scheduling cycles (the library's counterpart of populateNodeDb leaving
// an unschedulable node that holds no job out of the NodeDb, scheduling/scheduling_algo.go:1069-1077, and of the executor filters at :1100-1169).  The remaining rows keep
// their order and are renumbered densely: new position = old position - deleted rows below it.  Nothing here goes through the round kernel: armada_sched_mgpu.hip runs
// the per-element functions below on the whole grid, the CPU build of the tests runs them serially (the driver at the end of this file).
//
// WHAT DEPENDS ON A NODE POSITION: the lane of a node in every [..][Npad] plane and per-node array, its bit in every row of the class, shape, type and label masks, the
// entries of nodeByRank and the index of idxRank, and the node every running job names (jNode0, JobRec.node0).  Node types, label-value rows, index ranks relative to
// each other and everything else per job do not.
//
// THE PASSES (asched_host.inc asched_nodes_delete queues them through plat_nodes_delete_check and plat_nodes_delete):
//   mark: entry i clears the keep flag of its row (scratch, all 1 between calls).
//   check: one thread per job row; a running row whose node is a cleared one sends its id into one word with a minimum.  The host reads the word before anything is written.
//   scan: plat_compact over the N keep flags — the survivors' list src[new] = old, the exclusive prefix (= the new position of a surviving row) and the new N.
//   gather: the [R][Npad] planes totalRes and allocatable, one thread per (r, new node): consecutive lanes write consecutive words; then the narrow arrays (flags, id rank,
//     type, class word) in one launch that reads src once per row.  All into fresh blocks with the new stride (a grid cannot compact in place).
//   index rank: plat_compact of nodeByRank by the keep flag of its entries, every entry through the new positions, and idxRank[nodeByRank[i]] = i.
//   mask rows: one wave per output word.  Lane l holds new node 64 w + l and loads src once; for each row of each mask it tests its source bit, and the ballot of the 64
//     lanes IS the output word.  A lane at or beyond the new N contributes 0.  (The CPU build: the serial bit loop over the same ndBit.)
//   job remap: one thread per job row, jNode0[j] and JobRec.node0 through the new positions where they name a node.
//   unmark: entry i sets the keep flag of its row again.
#pragma once
#include "kernels_jobs_patch.h"

#ifndef ND_FN   // the CPU build: serial
#define ND_FN static inline
#endif
#ifndef ND_MIN32   // the CPU build: one element after the other
#define ND_MIN32(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#endif

#define ND_MASKS 4        // class mask, shape mask, type mask, label mask
#define ND_NONE INT32_MAX // the check word: no running job on a named row

struct NdArgs {   // everything in platform memory
  int32_t N, N1, n, R, M;      // N: rows before the call; N1: rows after it; n: entries; M: rows of the job table (0: none)
  int32_t Npad, Npad1, W, W1;  // the stride of the planes and the words of a mask row, before / after
  int32_t jobsOnly;            // the rebuild path: scan, job remap and unmark only (the reduced table goes through nodes_upsert's own code)
  const int32_t* node;         // [n] the rows to delete
  uint8_t* keep;               // [N]
  int32_t* src;                // [N] the survivors: src[new] = old
  uint32_t* newId;             // [N] kept rows below a row: the new position of a surviving one
  int32_t* bad;                // one word: the lowest job row that runs on a named node, ND_NONE
  int32_t* jNode0; JobRec* jrec;   // [M]; jrec NULL: no fast structure
  const int64_t *inTotal, *inAlloc; int64_t *outTotal, *outAlloc;   // [R][Npad] -> [R][Npad1]
  const uint8_t* inFlags; uint8_t* outFlags;
  const int32_t *inIdRank, *inType; int32_t *outIdRank, *outType;   // inType NULL: the handle has no masks yet
  const uint64_t* inCls; uint64_t* outCls;                          // NULL: no fast structure
  const int32_t* rankIn; int32_t *rankOut, *idxRankOut;             // nodeByRank [N] -> [N1], idxRank [N1]
  const uint64_t* inMask[ND_MASKS]; uint64_t* outMask[ND_MASKS]; int32_t rows[ND_MASKS];   // [rows][W] -> [rows][W1]; rows 0: skipped
};

ND_FN void ndMark(const NdArgs& a, int i, uint8_t v) { a.keep[a.node[i]] = v; }
ND_FN void ndCheck(const NdArgs& a, int j) {
  const int nd = a.jNode0[j];
  if (nd >= 0 && nd < a.N && !a.keep[nd]) ND_MIN32(a.bad, (int32_t)j);
}
// element e < R * N1 of a plane
ND_FN void ndPlane(const NdArgs& a, long long e) {
  const int r = (int)(e / a.N1), i = (int)(e - (long long)r * a.N1), s = a.src[i];
  a.outTotal[(size_t)r * a.Npad1 + i] = a.inTotal[(size_t)r * a.Npad + s];
  a.outAlloc[(size_t)r * a.Npad1 + i] = a.inAlloc[(size_t)r * a.Npad + s];
}
// new row i: the narrow arrays
ND_FN void ndNarrow(const NdArgs& a, int i) {
  const int s = a.src[i];
  a.outFlags[i] = a.inFlags[s];
  a.outIdRank[i] = a.inIdRank[s];
  if (a.inType) a.outType[i] = a.inType[s];
  if (a.inCls) a.outCls[i] = a.inCls[s];
}
// entry i < N1 of the compacted nodeByRank, still in old positions
ND_FN void ndRank(const NdArgs& a, int i) {
  const int32_t v = (int32_t)a.newId[a.rankOut[i]];
  a.rankOut[i] = v;
  a.idxRankOut[v] = i;
}
// the bit of old node s in a mask row of W words
ND_FN bool ndBit(const uint64_t* row, int s) { return (row[s >> 6] >> (s & 63)) & 1; }
ND_FN void ndJob(const NdArgs& a, int j) {
  const int nd = a.jNode0[j];
  if (nd < 0 || nd >= a.N) return;
  const int32_t v = (int32_t)a.newId[nd];
  a.jNode0[j] = v;
  if (a.jrec) a.jrec[j].node0 = v;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_nodes_delete_check / plat_nodes_delete (plat.h): the same per-element functions, one element after the other
static int plat_nodes_delete_check(Dev& d, NdArgs& a, int32_t* bad) {
  (void)d;
  for (int i = 0; i < a.n; i++) ndMark(a, i, 0);
  *a.bad = ND_NONE;
  for (int j = 0; j < a.M; j++) ndCheck(a, j);
  *bad = *a.bad;
  if (*bad != ND_NONE) for (int i = 0; i < a.n; i++) ndMark(a, i, 1);
  return 0;
}
static int plat_nodes_delete(Dev& d, NdArgs& a) {
  int n1 = 0;
  if (plat_compact(d, nullptr, a.N, a.keep, a.src, a.newId, nullptr, 0, nullptr, &n1)) return -1;
  if (n1 != a.N1) { g_err = "nodes_delete: the scan kept another number of rows than the host counted"; return -1; }
  if (a.jobsOnly) {
    for (int j = 0; j < a.M; j++) ndJob(a, j);
    for (int i = 0; i < a.n; i++) ndMark(a, i, 1);
    return 0;
  }
  for (long long e = 0; e < (long long)a.R * a.N1; e++) ndPlane(a, e);
  for (int i = 0; i < a.N1; i++) ndNarrow(a, i);
  int r1 = 0;
  if (plat_compact(d, a.rankIn, a.N, a.keep, a.rankOut, nullptr, nullptr, 0, nullptr, &r1)) return -1;
  if (r1 != a.N1) { g_err = "nodes_delete: the index order lost or gained rows"; return -1; }
  for (int i = 0; i < a.N1; i++) ndRank(a, i);
  for (int k = 0; k < ND_MASKS; k++)
    for (int row = 0; row < a.rows[k]; row++)
      for (int w = 0; w < a.W1; w++) {
        uint64_t word = 0;
        for (int l = 0; l < 64; l++) { const int nn = 64 * w + l; if (nn < a.N1 && ndBit(a.inMask[k] + (size_t)row * a.W, a.src[nn])) word |= 1ull << l; }
        a.outMask[k][(size_t)row * a.W1 + w] = word;
      }
  for (int j = 0; j < a.M; j++) ndJob(a, j);
  for (int i = 0; i < a.n; i++) ndMark(a, i, 1);
  return 0;
}
#endif
