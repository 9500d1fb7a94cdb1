// kernels_jobs_append.h — asched_jobs_append: newly submitted jobs enter the resident job table between two scheduling cycles (the library's counterpart of syncState's
// upsert of the new jobs into the jobDb, scheduler.go:478-535; jobdb/jobdb.go:572-700, the insertion into the per-queue sorted set at :691-700).  Rows M .. M+m-1 are
// written behind the M resident ones; the per-job arrays have room for them (asched_host.inc asched_jobs_append grows them first).  Nothing here goes through the round
// kernel: armada_sched_mgpu.hip runs jaFill on the whole grid, the CPU build of the tests runs it serially (the driver at the end of this file).
//
// WHAT A NEW ROW NEEDS: its slots of the per-job static arrays, the order-key inputs of the patch (kernels_jobs_patch.h), its JobRec where the fast structure has one, and
// its place in the pre-sorted order ordAll.  A new row is queued (no run) and its scheduling-key shape decides everything of its JobRec but the gang: the record of a
// RESIDENT row of the same shape (a.aSrc, a row < M: no thread reads what another writes) is copied and the four own fields put in — no JobRec crosses PCIe.
// A row whose shape has NO resident row — a new shape, or one asched_jobs_delete emptied — on the in-place path (asched_set_append_in_place, kernels_shapes_append.h)
// copies the template record the host built for its shape instead (a.tpl / a.aTpl: 128 bytes a shape, not a row); a.tpl == NULL is the function without that path.
//
// THE PASSES (asched_host.inc asched_jobs_append queues them):
//   row fill + keys, over the m rows padded to a power of two: slot i writes row M+i and leaves the row's order key in the sort array.  A row of no queue is in no order:
//     its slot, like the padding, is a sentinel that sorts behind every real key.
//   sort: the bitonic network of the patch (k_jp_tile / k_jp_step) on the same 40-byte records.
//   merge by rank: jpMerge of the patch with nothing removed — the "kept" sequence is the old ordAll itself, the "touched" one the sorted new keys; written into a spare
//     order buffer of at least total + nT entries, which the host swaps in.  The segment offsets (ordAllOff) come from the host, which knows every new row's queue.
#pragma once
#include "kernels_jobs_patch.h"

struct JaArgs {   // everything in platform memory
  int32_t M, m, nb2, R;       // M: rows before the call; nb2: m padded to a power of two >= JP_TILE (m when no new row is in a queue)
  int32_t writeRec, pad0_;    // writeRec: d.jrec has room for the new rows and every new row's shape has a resident row or a template (no rebuild follows)
  const int32_t *aQueue, *aPc, *aShape, *aGang, *aGangCard, *aGangUni, *aSrc;   // [m] the new rows; aSrc: a resident row of the same scheduling-key shape, -1 = none
  const uint32_t* aQPrio;     // [m]
  const int64_t* aSubmit;     // [m]
  const int64_t* aReq;        // [m][R]
  const uint8_t* aAligned;    // [m]
  const JobRec* tpl;          // the in-place path for new shapes (asched_set_append_in_place): one template record per shape without a resident row below M, or NULL
  const int32_t* aTpl;        // [m] the template of a row with aSrc < 0, -1 = none
  uint32_t* jQPrio;           // the patch's order-key inputs, writable: room for M + m rows (p.jQPrio / p.jSubmit are the same arrays)
  int64_t* jSubmit;
  JpArgs p;                   // the order-key inputs (keep / jQPrio / jSubmit / jRunTs, with room for M + m rows), the sort array p.keys [nb2], and the merge: p.kept = the old ordAll,
                              // p.nKept = its length, p.nT = new rows of a queue >= 0, p.out = the spare order buffer, p.n = 0
};

// slot i < nb2 of the sort array; i < m: row M + i first
JP_FN void jaFill(const Dev& d, const JaArgs& a, int i) {
  JpKey k; k.a = ~0ull; k.b = 0; k.t1 = 0; k.t2 = 0; k.idx = INT32_MAX; k.pad_ = 0;   // behind every real key (a queue has 31 bits)
  if (i < a.m) {
    const int j = a.M + i, q = a.aQueue[i];
    d.jQueue[j] = q; d.jPc[j] = a.aPc[i]; d.jShape[j] = a.aShape[i];
    d.jGang[j] = a.aGang[i]; d.jGangCard[j] = a.aGangCard[i]; d.jGangUni[j] = a.aGangUni[i];
    d.jNode0[j] = -1; d.jRunPrio[j] = 0; d.jLeaseMs[j] = 0;
    if (d.jAway) d.jAway[j] = 0;
    d.jAligned[j] = a.aAligned[i];
    for (int r = 0; r < a.R; r++) d.jReq[(size_t)j * a.R + r] = a.aReq[(size_t)i * a.R + r];
    a.p.keep[j] = 1; a.jQPrio[j] = a.aQPrio[i]; a.jSubmit[j] = a.aSubmit[i]; a.p.jRunTs[j] = 0;
    const bool fromTpl = a.tpl && a.aSrc[i] < 0 && a.aTpl[i] >= 0;   // a shape this call brings or revives: the host built its record once (128 B a shape)
    if (a.writeRec && d.jrec && (a.aSrc[i] >= 0 || fromTpl)) {
      JobRec r = fromTpl ? a.tpl[a.aTpl[i]] : d.jrec[a.aSrc[i]];   // everything the shape fixes: req, keyDelta, fieldMin, never, fit shape, cls, pc, pcPrio, preemptible, nlPc, ex0, ex1
      r.gang = a.aGang[i]; r.node0 = -1; r.runPrio = 0; r.nlRun = (uint8_t)jpLevels(d.cfg, r.preemptible ? 0 : INT32_MAX);
      d.jrec[j] = r;
    }
    if (q >= 0) {   // the key of a queued row, from the inputs (what jpKeyOf reads back once the row is resident)
      k.a = ((uint64_t)(uint32_t)q << 33) | ((uint64_t)1 << 32) | (uint32_t)~((uint32_t)d.cfg.pcPriority[a.aPc[i]] ^ 0x80000000u);
      k.b = a.aQPrio[i];
      k.t1 = k.t2 = (uint64_t)a.aSubmit[i] ^ (1ull << 63);
      k.idx = j;
    }
  }
  if (a.p.keys) a.p.keys[i] = k;
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_jobs_append (plat.h): the same per-element functions, one element after the other; the sort is the standard library's
// a.p.nT == 0 (no new row is in a queue): a.p.keys == nullptr, a.nb2 == a.m, and the order is left alone
static int plat_jobs_append(Dev& d, JaArgs& a) {
  for (int i = 0; i < a.nb2; i++) jaFill(d, a, i);
  if (a.p.nT > 0) {
    std::sort(a.p.keys, a.p.keys + a.nb2, [](const JpKey& x, const JpKey& y) { return jpLess(x, y); });
    const long long work = (long long)a.p.nT + a.p.nKept;
    for (long long i = 0; i < work; i++) jpMerge(d, a.p, i);
  }
  return 0;
}
// (plat.h's device-to-device copy, which only the append uses: the CPU build's other stand-ins sit in tests/hostsim/hostsim.cpp, and this one belongs beside plat_h2d there)
static void plat_d2d(void* dst, const void* src, size_t n) { memcpy(dst, src, n); }
#endif
