// kernels_req_classes_append.h — asched_req_classes_append: NEW requirement classes join the resident class table behind the C real ones, instead of asched_jobs_set of
// the whole job table.  A requirement class is the (tolerations, node selector, required node affinity) part of the scheduling key (internaltypes/podutils.go:52-72): a
// submission with a node selector, a hostname pin or a toleration the table has not seen brings one.  No resident row names a new class, so nothing per shape or per
// job changes; what grows is the class mask [Cext][W] and, where the fast structure exists, one bit per new class in nodeCls[N].
//
// WHAT A NEW CLASS ADDS TO THE CLASS MASK: one row.  Bit n: the class matches node n statically (classMatchesNode).  Two tiers, decided per class on the host:
//   tier 1, decided by node type — the row is the OR of typeMask[t] over the populated node types t the class matches (classMatchesType): a CSR of types per new class;
//   tier 2, matched on the host node by node — the row is uploaded (a.hostRows) and copied.
// The derived away classes sat behind the C real ones and keep their order: their rows move up by dC rows, device to device, in front of the pass.
//
// THE PASS (asched_host.inc asched_req_classes_append queues it through plat_req_classes_append, behind the device-to-device copies into the fresh block):
//   k_ca_rows, ONE WAVE PER 64-NODE WORD w, four waves to a workgroup: for each new class the word is assembled from wave-uniform loads (a uniform loop over the class's
//   types, or one load of the uploaded row), one lane stores it into the fresh mask, and every lane keeps its own bit of it as bit C0 + c of an accumulator.  After the
//   loop lane l ORs the accumulator into nodeCls[64 w + l]: one coalesced 512-byte read-modify-write a wave.  Lanes at or beyond N neither load nor store.  Exactly one
//   writer per mask word and per nodeCls element; no atomics, no LDS.
#pragma once
#include "dev.h"

#ifndef CA_FN   // the CPU build: serial
#define CA_FN static inline
#endif

struct CaArgs {   // everything in platform memory
  int32_t N, W, C0, dC;         // dC new classes get ids C0 .. C0 + dC - 1
  const uint64_t* typeMask;     // [T][W] the resident node-type mask
  const int32_t* typeOff;       // [dC + 1] CSR into types: the populated node types a tier-1 class matches (empty: it matches no node)
  const int32_t* types;
  const int32_t* hostRow;       // [dC] the row of hostRows a tier-2 class was matched into, -1 = tier 1
  const uint64_t* hostRows;     // [tier-2 classes][W]
  uint64_t* outMask;            // [Cext0 + dC][W] the fresh class mask
  uint64_t* nodeCls;            // [N] class bits of a node in the fast structure, or NULL (then C0 + dC may exceed 64)
  // the resident rows, copied in front of the pass: [0, copy0) words stay where they are, [src1, src1 + copy1) words (the derived classes) move to dst1
  const uint64_t* inMask; long long copy0, src1, dst1, copy1;
};

// word w of the row of new class c
CA_FN uint64_t caWord(const CaArgs& a, int c, int w) {
  const int hr = a.hostRow[c];
  if (hr >= 0) return a.hostRows[(size_t)hr * a.W + w];
  uint64_t word = 0;
  for (int k = a.typeOff[c]; k < a.typeOff[c + 1]; k++) word |= a.typeMask[(size_t)a.types[k] * a.W + w];
  return word;
}
// what node (lane) b of the word gains in nodeCls for new class c (only asked where nodeCls exists: C0 + dC <= 64)
CA_FN uint64_t caBit(const CaArgs& a, int c, uint64_t word, int b) { return ((word >> b) & 1) << ((a.C0 + c) & 63); }

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_req_classes_append (plat.h): the same per-element functions, one word after the other
static int plat_req_classes_append(Dev& d, CaArgs& a) {
  (void)d;
  if (a.copy0 > 0) memcpy(a.outMask, a.inMask, (size_t)a.copy0 * 8);
  if (a.copy1 > 0) memcpy(a.outMask + a.dst1, a.inMask + a.src1, (size_t)a.copy1 * 8);
  for (int w = 0; w < a.W; w++) {
    uint64_t acc[64] = {0};
    for (int c = 0; c < a.dC; c++) {
      const uint64_t word = caWord(a, c, w);
      a.outMask[(size_t)(a.C0 + c) * a.W + w] = word;
      if (a.nodeCls) for (int b = 0; b < 64; b++) acc[b] |= caBit(a, c, word, b);
    }
    if (a.nodeCls) for (int b = 0; b < 64 && 64 * w + b < a.N; b++) a.nodeCls[64 * w + b] |= acc[b];
  }
  return 0;
}
#endif
