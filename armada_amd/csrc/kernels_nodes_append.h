// kernels_nodes_append.h — asched_nodes_append: new rows join the resident node table between two scheduling cycles (the library's counterpart of populateNodeDb
// inserting whatever nodes the healthy executors report, scheduling/scheduling_algo.go:1019-1098: a cluster that scales up, an executor that returns from the filters
// at :1100-1169, a drained node that is uncordoned).  The m new rows take positions N .. N + m - 1; no resident position changes.  Nothing here goes through the round
// kernel: armada_sched_mgpu.hip runs the per-element functions below on the whole grid, the CPU build of the tests runs them serially (the driver at the end of this file).
//
// WHAT DEPENDS ON N, Npad OR W: the stride of every [..][Npad] plane, the length of every per-node array, the words of every row of the class, shape, type and label
// masks, the length of nodeByRank / idxRank.  Nothing is changed in place: every pass writes into a fresh block of the new size (asched_host.inc asched_nodes_append
// allocates all of them before anything changes and swaps them in at the end).
//
// THE PASSES (asched_nodes_append queues them through plat_nodes_append):
//   planes: totalRes and allocatable [R][Npad] -> [R][Npad1], one thread per (r, new position): consecutive lanes write consecutive words.  A position below N copies
//     with the old stride, the others take the uploaded entries (a floating column FLOATING_NODE_CAPACITY); the lanes N1 .. Npad1 stay zero (the block was zeroed).
//   narrow arrays, one launch, one thread per new position: flag byte, id rank (or the whole of id_rank_all), node type, and the class word where the fast structure has one.
//   index order: the host sorted the new rows by node.index and found each one's insertion point ins[k] among the resident ranks (the number of resident rows with a
//     smaller index).  One thread per entry of the merged order: the resident entry at rank r goes to r + (insertion points <= r), a binary search over the m points; new
//     entry k goes to ins[k] + k.  idxRank[nodeByRank[i]] = i is written by the same thread.
//   mask rows [rows][W] -> [rows][W1], ONE THREAD PER OUTPUT WORD (DESIGN 3.14 says why not a wave): a word wholly below N is a copy; a word that holds new positions is
//     the old word's bits (where it existed) OR the new rows' bits — the class bit the host worked out per entry, the shape bit k_np_mask's test, type == row, "the row
//     carries that label value".  Exactly one writer per output word, no atomics.
#pragma once
#include "dev.h"
#include "../../include/armada_sched.h"

#ifndef NA_FN   // the CPU build: serial
#define NA_FN static inline
#endif

#define NA_MASKS 4        // class mask, shape mask, type mask, label mask

struct NaArgs {   // everything in platform memory
  int32_t N, N1, m, R;         // N: rows before the call; N1 = N + m
  int32_t Npad, Npad1, W, W1;  // the stride of the planes and the words of a mask row, before / after
  int32_t CW, L, floatMask, pad0_;   // CW: 64-bit words of class bits per entry; L: indexed label slots per entry; floatMask bit r: column r is a floating resource
  uint64_t clsLow;             // the bits of the C real requirement classes in an entry's first class word (d.nodeCls holds those)
  const int64_t *pTotal, *pAlloc;   // [m][R] the entries, entry e at position N + e
  const uint8_t* pFlags;       // [m]
  const int32_t *pIdRank, *pType;   // [m]
  const int32_t* idRankAll;    // [N1] or NULL: replaces the id rank of every row
  const uint64_t* pCls;        // [m][CW] bit c: requirement class c (derived away classes included) matches the entry statically
  const int32_t* pLab;         // [m][L] the row of the label mask the entry's value of slot l has, -1: the entry does not carry the label
  const int32_t *ins, *insRow; // [m] ascending by node.index: resident rows with a smaller index, and the position of the new row
  const int64_t *inTotal, *inAlloc; int64_t *outTotal, *outAlloc;   // [R][Npad] -> [R][Npad1]
  const uint8_t* inFlags; uint8_t* outFlags;
  const int32_t *inIdRank, *inType; int32_t *outIdRank, *outType;   // inType NULL: the handle has no masks yet
  const uint64_t* inCls; uint64_t* outCls;                          // NULL: no fast structure
  const int32_t* rankIn; int32_t *rankOut, *idxRankOut;             // nodeByRank [N] -> [N1], idxRank [N1]
  const int32_t* shapeClass; const int64_t* shapeReq;               // [rows[1]], [rows[1]][R]
  const uint64_t* inMask[NA_MASKS]; uint64_t* outMask[NA_MASKS]; int32_t rows[NA_MASKS];   // [rows][W] -> [rows][W1]; rows 0: skipped
};

// element e < R * N1 of a plane
NA_FN void naPlane(const NaArgs& a, long long e) {
  const int r = (int)(e / a.N1), i = (int)(e - (long long)r * a.N1);
  const size_t o = (size_t)r * a.Npad1 + i;
  if (i < a.N) { a.outTotal[o] = a.inTotal[(size_t)r * a.Npad + i]; a.outAlloc[o] = a.inAlloc[(size_t)r * a.Npad + i]; return; }
  const bool fl = (a.floatMask >> r) & 1;
  a.outTotal[o] = fl ? FLOATING_NODE_CAPACITY : a.pTotal[(size_t)(i - a.N) * a.R + r];
  a.outAlloc[o] = fl ? FLOATING_NODE_CAPACITY : a.pAlloc[(size_t)(i - a.N) * a.R + r];
}
// position i < N1: the narrow arrays
NA_FN void naNarrow(const NaArgs& a, int i) {
  const int e = i - a.N;
  a.outFlags[i] = e < 0 ? a.inFlags[i] : a.pFlags[e];
  a.outIdRank[i] = a.idRankAll ? a.idRankAll[i] : e < 0 ? a.inIdRank[i] : a.pIdRank[e];
  if (a.inType) a.outType[i] = e < 0 ? a.inType[i] : a.pType[e];
  if (a.inCls) a.outCls[i] = e < 0 ? a.inCls[i] : (a.pCls[(size_t)e * a.CW] & a.clsLow);
}
// entry i < N1 of the merged index order: i < N the resident entry at rank i, else new entry i - N of the sorted list
NA_FN void naRank(const NaArgs& a, int i) {
  int pos, v;
  if (i < a.N) {
    int lo = 0, hi = a.m;   // the insertion points <= i: the first k with ins[k] > i
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.ins[mid] <= i) lo = mid + 1; else hi = mid; }
    pos = i + lo; v = a.rankIn[i];
  } else { const int k = i - a.N; pos = a.ins[k] + k; v = a.insRow[k]; }
  a.rankOut[pos] = v;
  a.idxRankOut[v] = pos;
}
// the bit of entry e (position N + e) in row `row` of mask k
NA_FN bool naBit(const NaArgs& a, int k, int row, int e) {
  if (k == 0) return (a.pCls[(size_t)e * a.CW + (row >> 6)] >> (row & 63)) & 1;
  if (k == 1) {
    const int cls = a.shapeClass[row];
    if (!((a.pCls[(size_t)e * a.CW + (cls >> 6)] >> (cls & 63)) & 1)) return false;
    for (int r = 0; r < a.R; r++) if (a.shapeReq[(size_t)row * a.R + r] > a.outTotal[(size_t)r * a.Npad1 + a.N + e]) return false;   // nodematching.go:184 (k_shape_mask, k_np_mask)
    return true;
  }
  if (k == 2) return a.pType[e] == row;
  for (int l = 0; l < a.L; l++) if (a.pLab[(size_t)e * a.L + l] == row) return true;
  return false;
}
// output word t < (rows[0] + rows[1] + rows[2] + rows[3]) * W1
NA_FN void naMaskWord(const NaArgs& a, long long t) {
  int row = (int)(t / a.W1), k = 0;
  const int w = (int)(t - (long long)row * a.W1);
  while (row >= a.rows[k]) { row -= a.rows[k]; k++; }
  uint64_t word = w < a.W ? a.inMask[k][(size_t)row * a.W + w] : 0;
  const int base = 64 * w;
  if (base + 64 > a.N) {
    if (base >= a.N) word = 0; else word &= (1ull << (a.N - base)) - 1;   // (no bit at or beyond the old N)
    const int hi = a.N1 < base + 64 ? a.N1 : base + 64;
    for (int p = base > a.N ? base : a.N; p < hi; p++) if (naBit(a, k, row, p - a.N)) word |= 1ull << (p - base);
  }
  a.outMask[k][(size_t)row * a.W1 + w] = word;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_nodes_append (plat.h): the same per-element functions, one element after the other
static int plat_nodes_append(Dev& d, NaArgs& a) {
  (void)d;
  for (long long e = 0; e < (long long)a.R * a.N1; e++) naPlane(a, e);
  for (int i = 0; i < a.N1; i++) naNarrow(a, i);
  for (int i = 0; i < a.N1; i++) naRank(a, i);
  long long rows = 0;
  for (int k = 0; k < NA_MASKS; k++) rows += a.rows[k];
  for (long long t = 0; t < rows * a.W1; t++) naMaskWord(a, t);
  return 0;
}
#endif
