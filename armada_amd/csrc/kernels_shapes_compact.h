// kernels_shapes_compact.h — asched_shapes_compact: scheduling-key shapes no resident row names (asched_jobs_delete emptied them, shapeRow[s] < 0), the fit shapes only
// they mapped to and, on request, the requirement classes only they named LEAVE the resident tables, instead of asched_jobs_set of the whole job table.  The live
// shapes, fit shapes and real classes keep their relative order and get dense ids (new id = old id minus the dead ones below it); the host works the three maps out
// from its mirrors (O(S)), the device applies them.  Three passes, each with exactly one writer per element, plain stores, no atomics:
//
//   k_sc_rows, IN PLACE, one thread per resident row j < M, SC_RPB rows to a workgroup: jShape[j] <- shapeNew[jShape[j]]; where the job records exist
//   jrec[j].shape <- fitNew[jrec[j].shape] and, with class retirement, jrec[j].cls <- clsNew[jrec[j].cls].  Rows are independent and a row reads only its own words, so
//   in place is exact; a word is stored only where its value changes.  The maps are small: a workgroup stages them in LDS when all three fit SC_LDS_CAP entries
//   each, and reads them from global memory otherwise (`staged` is a launch argument, so the branch is uniform over the grid).
//
//   k_sc_gather, one thread per OUTPUT word of a fresh block: out[row][w] = in[src[row]][w].  The shape mask ([live shape rows | away rows of live shapes]) and, with
//   class retirement, the class mask ([live real classes | re-derived classes]: deriveAwayRows numbers derived classes by first occurrence in the compacted shape
//   table, which can permute them — hence a source table, not a shift).
//
//   k_sc_clsbits, one thread per node, with class retirement where nodeCls exists: bit clsNew[c] of the output is bit c of the input for every live real class c.
//   A loop over the set bits of the live-class word (at most 64 steps, a handful in practice), not a byte-wise table: no LDS, nothing to stage for 8 bytes a node.
#pragma once
#include "dev.h"

#ifndef SC_FN   // the CPU build: serial
#define SC_FN static inline
#endif
#ifndef SC_LDS_CAP
#define SC_LDS_CAP 1024   // entries of each of the three maps a workgroup of k_sc_rows stages in LDS (12 KiB); the CPU build of the tests takes a small -D value
#endif
#define SC_RPB 4096       // rows of k_sc_rows per workgroup: the staging (up to 3 x SC_LDS_CAP loads a workgroup) is spread over 16 rows a thread

struct ScArgs {   // everything in platform memory
  int32_t M, S0, F0, C0;        // resident rows; entries of shapeNew / fitNew / clsNew
  const int32_t* shapeNew;      // [S0] old -> new scheduling-key shape (-1: dead; no resident row names one)
  const int32_t* fitNew;        // [F0] old -> new fit shape, or NULL: no job records
  const int32_t* clsNew;        // [C0] old -> new real requirement class, or NULL: classes stay
  int32_t* jShape;              // [M] in place
  JobRec* jrec;                 // [M] in place, or NULL
  int32_t staged;               // 1: the maps fit SC_LDS_CAP entries each (scFits: set by plat_shapes_compact, whatever the caller wrote)
  // the gathers: rows of W words
  int32_t W;
  const uint64_t* shapeIn; uint64_t* shapeOut; const int32_t* shapeSrc; int32_t shapeRows;   // the fresh shape mask [shapeRows][W], row r from shapeIn[shapeSrc[r]]
  const uint64_t* clsIn; uint64_t* clsOut; const int32_t* clsSrc; int32_t clsRows;           // the fresh class mask, or clsOut == NULL
  // the class bits of the nodes
  int32_t N; uint64_t* nodeCls; uint64_t liveCls;   // nodeCls NULL: no fast structure / classes stay.  liveCls: bit c = real class c stays (C0 <= 64 wherever nodeCls exists)
};

static inline int scFits(const ScArgs& a) { return a.S0 <= SC_LDS_CAP && (!a.fitNew || a.F0 <= SC_LDS_CAP) && (!a.clsNew || a.C0 <= SC_LDS_CAP) ? 1 : 0; }
// row j through maps the caller chose (LDS copies or the global arrays)
SC_FN void scRow(const ScArgs& a, int j, const int32_t* shapeNew, const int32_t* fitNew, const int32_t* clsNew) {
  const int32_t s = a.jShape[j];
  if (s >= 0 && s < a.S0) { const int32_t s1 = shapeNew[s]; if (s1 != s) a.jShape[j] = s1; }
  if (a.jrec && fitNew) {
    const int32_t f = a.jrec[j].shape;
    if (f >= 0 && f < a.F0) { const int32_t f1 = fitNew[f]; if (f1 != f) a.jrec[j].shape = f1; }
    if (clsNew) {
      const int32_t c = a.jrec[j].cls;
      if (c >= 0 && c < a.C0) { const int32_t c1 = clsNew[c]; if (c1 != c) a.jrec[j].cls = c1; }
    }
  }
}
// output word i of a gather
SC_FN void scGather(const uint64_t* in, uint64_t* out, const int32_t* src, int W, long long i) {
  const long long row = i / W; const int w = (int)(i - row * W);
  out[i] = in[(size_t)src[row] * W + w];
}
// the class word of one node, bit-compacted by the live-class word: set bit number k of `live` (from the bottom) is where output bit k comes from
SC_FN uint64_t scClsBits(uint64_t in, uint64_t live) {
  uint64_t out = 0; int k = 0;
  for (uint64_t m = live; m; m &= m - 1, k++) out |= ((in >> __builtin_ctzll(m)) & 1ull) << k;
  return out;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_shapes_compact (plat.h): the same per-element functions, one element after the other.  The staged branch copies the maps into local
// arrays of SC_LDS_CAP entries per SC_RPB rows, as a workgroup does
static int plat_shapes_compact(Dev& d, ScArgs& a) {
  (void)d;
  a.staged = scFits(a);
  for (int lo = 0; lo < a.M; lo += SC_RPB) {
    const int hi = lo + SC_RPB < a.M ? lo + SC_RPB : a.M;
    if (a.staged) {
      int32_t sS[SC_LDS_CAP], sF[SC_LDS_CAP], sC[SC_LDS_CAP];
      for (int i = 0; i < a.S0; i++) sS[i] = a.shapeNew[i];
      for (int i = 0; a.fitNew && i < a.F0; i++) sF[i] = a.fitNew[i];
      for (int i = 0; a.clsNew && i < a.C0; i++) sC[i] = a.clsNew[i];
      for (int j = lo; j < hi; j++) scRow(a, j, sS, a.fitNew ? sF : nullptr, a.clsNew ? sC : nullptr);
    } else {
      for (int j = lo; j < hi; j++) scRow(a, j, a.shapeNew, a.fitNew, a.clsNew);
    }
  }
  if (a.shapeOut) for (long long i = 0; i < (long long)a.shapeRows * a.W; i++) scGather(a.shapeIn, a.shapeOut, a.shapeSrc, a.W, i);
  if (a.clsOut) for (long long i = 0; i < (long long)a.clsRows * a.W; i++) scGather(a.clsIn, a.clsOut, a.clsSrc, a.W, i);
  if (a.nodeCls) for (int n = 0; n < a.N; n++) { const uint64_t v = scClsBits(a.nodeCls[n], a.liveCls); if (v != a.nodeCls[n]) a.nodeCls[n] = v; }
  return 0;
}
#endif
