// kernels_shapes_append.h — the in-place path of asched_jobs_append (asched_set_append_in_place): rows of NEW scheduling-key shapes join the resident job table and
// the shape-dependent tables grow by what the new shapes add, instead of being re-derived for every shape (rebuildMasks -> buildFast).  A scheduling-key shape is the
// whole request vector (jobdb's SchedulingKey, internaltypes/scheduling_key.go), so a submission that asks for one more milli-CPU than anything seen before is a new one.
//
// WHAT A NEW SHAPE ADDS TO THE SHAPE MASK: one row per shape, and one per (shape, away entry of its priority class).  Bit n of a row: the row's requirement class matches
// node n statically (the resident class mask) and the shape's request is <= the node's total on every resource (nodematching.go:184; k_shape_mask, k_np_mask and
// naBit use the same test).  No resident row depends on it.
//
// THE PASS (asched_host.inc asched_jobs_append queues it through plat_shapes_append, behind the device-to-device copies of the resident rows into the fresh block):
//   k_sa_mask, ONE WAVE PER 64-NODE OUTPUT WORD: lane l owns node 64 w + l and loads the node's R totals once — totalRes is [R][Npad], so the 64 lanes read 512
//   consecutive bytes per resource — and keeps them in registers for every new row.  Per row the class word classMask[cls][w] is one wave-uniform load, the request is
//   wave-uniform, and the ballot of saBit over the wave IS the output word: one lane stores it.  Lanes at or beyond N load nothing and vote 0.  Exactly one writer per
//   output word; no atomics, no LDS.  (k_shape_mask, the full rebuild's kernel, is one thread per (row, word) and re-reads the 64 totals of a word for every row with a
//   lane stride of 512 bytes: right for all rows at once, wasteful for a handful.)
#pragma once
#include "dev.h"

#ifndef SA_FN   // the CPU build: serial
#define SA_FN static inline
#endif

struct SaArgs {   // everything in platform memory
  int32_t N, Npad, W, R;
  int32_t rows, pad0_;          // new mask rows: the new shapes' rows, then the new away rows
  const int64_t* totalRes;      // [R][Npad]
  const uint64_t* classMask;    // [Cext][W] the grown class mask
  const int32_t* rowClass;      // [rows] requirement class of a new row (a derived away class for an away row)
  const int32_t* rowOut;        // [rows] the row of outMask a new row is written to
  const int64_t* rowReq;        // [rows][R] the request of the row's shape
  uint64_t* outMask;            // [..][W] the fresh shape mask
  // the resident rows, copied in front of the pass: [0, copy0) words stay where they are, [src1, src1 + copy1) words move to dst1 (the away rows start at cfg.S)
  const uint64_t* inMask; long long copy0, src1, dst1, copy1;
};

// the totals of node n, once: tot[r] for r < R
SA_FN void saLoad(const SaArgs& a, int n, int64_t* tot) {
  for (int r = 0; r < MAXR; r++) if (r < a.R) tot[r] = a.totalRes[(size_t)r * a.Npad + n];
}
// the bit of a node with these totals in new row `row`; cw: the row's class word, b: the node's bit in it
SA_FN bool saBit(const SaArgs& a, int row, uint64_t cw, int b, const int64_t* tot) {
  if (!((cw >> b) & 1)) return false;
  for (int r = 0; r < MAXR; r++) if (r < a.R && a.rowReq[(size_t)row * a.R + r] > tot[r]) return false;
  return true;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_shapes_append (plat.h): the same per-element functions, one node after the other
static int plat_shapes_append(Dev& d, SaArgs& a) {
  (void)d;
  if (a.copy0 > 0) memcpy(a.outMask, a.inMask, (size_t)a.copy0 * 8);
  if (a.copy1 > 0) memcpy(a.outMask + a.dst1, a.inMask + a.src1, (size_t)a.copy1 * 8);
  for (int w = 0; w < a.W; w++)
    for (int row = 0; row < a.rows; row++) {
      const uint64_t cw = a.classMask[(size_t)a.rowClass[row] * a.W + w];
      uint64_t word = 0;
      for (int b = 0; b < 64 && 64 * w + b < a.N; b++) {
        int64_t tot[MAXR];
        saLoad(a, 64 * w + b, tot);
        if (saBit(a, row, cw, b, tot)) word |= 1ull << b;
      }
      a.outMask[(size_t)a.rowOut[row] * a.W + w] = word;
    }
  return 0;
}
#endif
