// kernels_nodes_patch.h — asched_nodes_patch: a few rows of the resident node table change between two scheduling cycles (the library's counterpart of what populateNodeDb
// re-reads per node every cycle, scheduling/scheduling_algo.go:1069-1095: IsUnschedulable, WithOverAllocated, MarkResourceUnallocatable; now and then a taint).  Nothing
// here goes through the round kernel: armada_sched_mgpu.hip runs the per-element functions below on the whole grid, the CPU build of the tests runs them serially (the
// driver at the end of this file).
//
// WHAT DEPENDS ON A NODE'S PATCHED FIELDS, on the device: the node's column of d.allocatable, its byte of d.nodeFlags, its node type (the type array of the literal
// batched first fit and one bit in every row of d.typeMask), its bit in every row of the resident class mask and of d.shapeMask (StaticJobRequirementsMet:
// a taint decides the class bit, the shape bit is the class bit && request <= total, k_shape_mask), and its word of d.nodeCls where the fast structure exists.  The
// planes and the order keys follow from allocatable: the three k_bulk passes the host queues behind these two (B_INIT_ALLOC, B_KEYS_ALL, B_RESET_JOBS).  Label masks,
// totals, index ranks and everything per job do not depend on them.
//
// THE PASSES (asched_host.inc asched_nodes_patch queues them).  The host sorts the entries by node and groups them by 64-node word: wordIdx[k] is the k-th touched word,
// its entries are wordOff[k] .. wordOff[k + 1].
//   scatter, one thread per entry: the node's allocatable column (a floating column keeps FLOATING_NODE_CAPACITY), flag byte, type and class word.
//   mask words, one thread per (mask row, touched word): the thread reads the word, replaces the bits of the word's patched nodes and writes it back.  Exactly one thread
//     owns a destination word: no atomics.  The rows are the Cext class rows, the Sext shape rows (away rows included) and the T type rows, in that order.
#pragma once
#include "dev.h"
#include "../../include/armada_sched.h"

#ifndef NP_FN   // the CPU build: serial
#define NP_FN static inline
#endif

struct NpArgs {   // everything in platform memory
  int32_t n, nW, Cext, Sext, T, CW, pad0_, pad1_;   // n entries in nW words; CW: 64-bit words of class bits per entry; Cext = Sext = T = 0: the handle has no masks yet
  uint64_t clsLow;                // the bits of the C real requirement classes in an entry's first class word (d.nodeCls holds those)
  const int32_t *pNode, *pType;   // [n] the entries, ascending by node
  const uint8_t* pFlags;          // [n] the new byte of d.nodeFlags
  const int64_t* pAlloc;          // [n][R]
  const uint64_t* pCls;           // [n][CW] bit c: requirement class c (derived away classes included) matches the node statically
  const int32_t *wordOff, *wordIdx;   // [nW + 1], [nW]
  uint64_t* classMask;            // [Cext][W] the resident class mask (rebuildMasks)
  const int32_t* shapeClass;      // [Sext]
  int32_t* nodeType;              // [N]
  uint64_t* nodeCls;              // [N] or nullptr: no fast structure
};

NP_FN void npScatter(const Dev& d, const NpArgs& a, int i) {
  const DevCfg& c = d.cfg;
  const int node = a.pNode[i];
  for (int r = 0; r < c.R; r++) if (!c.isFloating[r]) d.allocatable[(size_t)r * c.Npad + node] = a.pAlloc[(size_t)i * c.R + r];
  d.nodeFlags[node] = a.pFlags[i];
  if (a.nodeType) a.nodeType[node] = a.pType[i];
  if (a.nodeCls) a.nodeCls[node] = a.pCls[(size_t)i * a.CW] & a.clsLow;
}
// the new bit of entry e in mask row `row`
NP_FN bool npBit(const Dev& d, const NpArgs& a, int row, int e) {
  const DevCfg& c = d.cfg;
  if (row < a.Cext) return (a.pCls[(size_t)e * a.CW + (row >> 6)] >> (row & 63)) & 1;
  if (row < a.Cext + a.Sext) {
    const int s = row - a.Cext, cls = a.shapeClass[s], node = a.pNode[e];
    if (!((a.pCls[(size_t)e * a.CW + (cls >> 6)] >> (cls & 63)) & 1)) return false;
    for (int r = 0; r < c.R; r++) if (d.shapeReq[(size_t)s * c.R + r] > d.totalRes[(size_t)r * c.Npad + node]) return false;   // nodematching.go:184 (k_shape_mask)
    return true;
  }
  return a.pType[e] == row - a.Cext - a.Sext;
}
// t < (Cext + Sext + T) * nW
NP_FN void npMaskWord(const Dev& d, const NpArgs& a, long long t) {
  const int row = (int)(t / a.nW), k = (int)(t % a.nW), W = d.cfg.W;
  uint64_t* dst = row < a.Cext ? a.classMask + (size_t)row * W : row < a.Cext + a.Sext ? d.shapeMask + (size_t)(row - a.Cext) * W : d.typeMask + (size_t)(row - a.Cext - a.Sext) * W;
  uint64_t w = dst[a.wordIdx[k]];
  for (int e = a.wordOff[k]; e < a.wordOff[k + 1]; e++) {
    const uint64_t bit = 1ull << (a.pNode[e] & 63);
    w = npBit(d, a, row, e) ? (w | bit) : (w & ~bit);
  }
  dst[a.wordIdx[k]] = w;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_nodes_patch (plat.h): the same per-element functions, one element after the other
static int plat_nodes_patch(Dev& d, const NpArgs& a) {
  for (int i = 0; i < a.n; i++) npScatter(d, a, i);
  const long long work = (long long)(a.Cext + a.Sext + a.T) * a.nW;
  for (long long t = 0; t < work; t++) npMaskWord(d, a, t);
  return 0;
}
#endif
