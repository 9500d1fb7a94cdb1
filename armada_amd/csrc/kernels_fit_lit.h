// kernels_fit_lit.h — the batched first fit for mask rows on the LITERAL iteration path (a request off the index grid, or several node types whose allocatable
// is off it: asched_host.inc rebuildMasks `rowLiteral`): selectAtLevelLiteral (round_ctl.h; nodedb.go:840-928 over nodeiteration.go:74-185, 318-382) for a whole
// batch of (mask row) queries at one level, grid-wide, with nothing going through the round kernel.  armada_sched_mgpu.hip runs flQuery one WAVE per query;
// the CPU build of the tests runs the same function with one lane (the serial driver at the end of this file).
//
// THE INDEX (FitLitIdx, built per call and level: flFill -> sort -> flFinish).  The nodes sorted by (node type, order key of the level): one segment per node
// type — the reference's per-type memdb index (nodedb.go:1164-1175).  The planes of the level are gathered into index order next to it, so 64 consecutive
// entries are 64 consecutive words of every plane.  "First node of type t at or after a bound" (round_ctl.h litAdvance: a whole plane pass through wgFirstFit
// with noFit) is flLowerBound in t's segment; "strictly after this node" (memdbIterator.Next) is the next entry, because keys are unique (they end in the
// node-index rank).
//
// EXACTNESS.  NodeTypeIterator.NextNode (nodeiteration.go:318-382) looks at one node at a time and does one of three things with it: yield it, seek (raise its
// lower bound `lb` and jump to the first key at or after it), or go on to the next key.  Which of the three depends on the node's own quantities, on the request
// and on `lb` — and `lb` changes only at a seek.  flAdvance classifies up to 64 consecutive entries at once under the CURRENT `lb`: every entry in front of the
// first one that yields or seeks is a plain "go on" under that same `lb`, exactly as the one-at-a-time walk would have found it, so the first such entry in index
// order is the walk's next event.  A seek searches the type's whole segment for the new bound (flBound == round_ctl.h litBound), which is what LowerBound on the
// memdb index does; nothing assumes the bound lies ahead.
// Several node types: NodeTypesIterator (:74-185) pops the iterator whose head is least by (raw indexed quantities, node id) and advances it before the node is
// tested.  The per-type sequences are ordered by ROUNDED quantities, not by that comparison, so the merge is not a sort and is restated pop by pop: the heads of
// the (<= LIT_TMAX = 64, the wavefront size) iterators sit in the wave's LDS, every pop is one flAdvance.
// One node type: the merge yields the iterator's nodes in its own order and a node that fails the static mask or fitsAlloc changes no iterator state, so the
// test moves INTO the classification (a yielded entry that fails is a "go on"): the query ends at the first entry that yields AND passes, without a pass per
// rejected node.  With several types that shortcut would be wrong (a failing head decides which iterator is popped next) and is not taken.
// Not served here: two-word order keys (the host refuses such rows in a batch), more than LIT_TMAX node types for a row (refused at upload, as for rounds).
#pragma once
#include "dev.h"

#ifndef FL_FN   // the CPU build: one lane
#define FL_FN static inline
#define FL_LANE 0
#define FL_NL 1
#define FL_BALLOT(p) ((p) ? 1ull : 0ull)
#define FL_SHFL(v, l) (v)
#define FL_UNROLL
#endif
// (the per-column loops run over MAXK with the column count as a predicate and are unrolled on the device: lb / nlb / ireq stay in registers instead of scratch)

#define FL_TILE 2048   // records of the sort network's in-LDS tile (32 KB); the sort scratch holds a power of two >= max(N, FL_TILE) records
struct FlPair { unsigned long long hi, lo; };   // sort record: (node type, order key); padding records are (~0, ~0)
struct FitLitIdx {
  unsigned long long* key;   // [n] order keys of the level in (type, key) order
  int32_t* node;             // [n] the entry's node
  int64_t* al;               // [R][stride] the level's planes in index order
  int32_t* typeBeg;          // [T] segment of each node type (beg == end: no node)
  int32_t* typeEnd;
  int32_t n, stride, level, pad;
};
struct FlIt { int64_t lb[MAXK]; int32_t pos, beg, end, head; };   // NodeTypeIterator: lower bound (raw quantities), next entry to look at, the type's segment, the entry it yielded last (-1: exhausted)

// ---- index build, per element
FL_FN void flFill(const Dev& d, const int32_t* nodeType, int level, FlPair* a, int i) {
  if (i < d.cfg.N) { a[i].hi = (unsigned long long)nodeType[i]; a[i].lo = d.keys[(size_t)level * d.cfg.Npad + i]; }
  else { a[i].hi = ~0ull; a[i].lo = ~0ull; }
}
FL_FN bool flPairLess(const FlPair& x, const FlPair& y) { return x.hi != y.hi ? x.hi < y.hi : x.lo < y.lo; }
FL_FN void flFinish(const Dev& d, const FitLitIdx& x, const FlPair* a, int i) {   // i < N
  const DevCfg& c = d.cfg;
  int node = d.nodeByRank[a[i].lo & ((1ull << c.idxBits) - 1)];
  x.key[i] = a[i].lo; x.node[i] = node;
  for (int r = 0; r < c.R; r++) x.al[(size_t)r * x.stride + i] = d.alloc[((size_t)x.level * c.R + r) * c.Npad + node];
  int t = (int)a[i].hi;
  if (i == 0 || a[i - 1].hi != a[i].hi) x.typeBeg[t] = i;
  if (i == c.N - 1 || a[i + 1].hi != a[i].hi) x.typeEnd[t] = i + 1;
}

// ---- the iterators
FL_FN int64_t flCeilDiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && a > 0) ? q + 1 : q; }
// round_ctl.h litBound: packed form of memdb LowerBound(NodeIndexKey(type, b)) within one node type (~0: behind every key)
FL_FN unsigned long long flBound(const DevCfg& c, const int64_t* b) {
  unsigned long long acc = 0; int bits = 0; bool stop = false;
  FL_UNROLL
  for (int i = 0; i < MAXK; i++) {
    if (i >= c.K) break;
    int w = c.keyWidth[i], ws = w + c.keyGuard;
    if (stop) { acc <<= ws; bits += ws; continue; }
    int64_t res = c.indexedRes[i];
    bool aligned = b[i] % res == 0;
    int64_t f = (aligned ? b[i] / res : flCeilDiv(b[i], res)) - c.keyLo[i];
    if (f < 0) { f = 0; stop = true; }
    else if (w < 63 && f >= ((int64_t)1 << w)) {
      if (bits == 0) return ~0ull;
      acc += 1;
      if (bits < 64 && acc >= (1ull << bits)) return ~0ull;
      f = 0; stop = true;
    } else if (!aligned) stop = true;
    acc = (acc << ws) | (unsigned long long)f; bits += ws;
  }
  return acc << c.idxBits;
}
FL_FN bool flLbLess(const DevCfg& c, const int64_t* a, const int64_t* b) {
  bool less = false, decided = false;
  FL_UNROLL
  for (int i = 0; i < MAXK; i++) if (i < c.K && !decided && a[i] != b[i]) { less = a[i] < b[i]; decided = true; }
  return less;
}
// first entry of [beg, end) whose key is >= bound: every lane probes one of FL_NL evenly spaced entries per step (one lane: a binary search), so a segment of
// 100 000 entries takes three dependent loads instead of seventeen.  `less` is true for a prefix of the lanes (the probes ascend, the keys are sorted).
FL_FN int flLowerBound(const FitLitIdx& x, int beg, int end, unsigned long long bound) {
  int lo = beg, hi = end;
  while (lo < hi) {
    long long n = hi - lo;
    int q = lo + (int)(((long long)(FL_LANE + 1) * n) / (FL_NL + 1));   // lo <= q < hi
    bool less = x.key[q] < bound;
    int cnt = __builtin_popcountll(FL_BALLOT(less));
    if (cnt == 0) hi = lo + (int)(n / (FL_NL + 1));                                            // the answer is at or before lane 0's probe
    else {
      if (cnt < FL_NL) hi = lo + (int)(((long long)(cnt + 1) * n) / (FL_NL + 1));              // ... at or before the first probe that is not less
      lo = lo + (int)(((long long)cnt * n) / (FL_NL + 1)) + 1;                                 // ... and behind the last one that is
    }
  }
  return lo;
}
// what NextNode does with entry e under the lower bound lb: 0 go on, 1 yield, 2 seek to nlb (:340-378)
FL_FN int flClassify(const DevCfg& c, const FitLitIdx& x, int e, const int64_t* lb, const int64_t* ireq, int64_t* nlb) {
  bool below = false;   // a column in front of this one is below the request: nlb takes the request from that column on
  FL_UNROLL
  for (int i = 0; i < MAXK; i++) {
    if (i >= c.K) break;
    if (!below) {
      int64_t nodeQ = x.al[(size_t)c.indexedCol[i] * x.stride + e];
      nlb[i] = (nodeQ / c.indexedRes[i]) * c.indexedRes[i];   // roundQuantityToResolution (encoding.go:56-58)
      below = nodeQ < ireq[i];
    }
    if (below) nlb[i] = ireq[i];
  }
  if (below) return flLbLess(c, lb, nlb) ? 2 : 0;            // "new lower-bound is not greater than current bound" (:371-376): go on
  return c.K > 0 ? 1 : 0;
}
// static mask and DynamicJobRequirementsMet (nodematching.go:194-197) of entry e
FL_FN bool flPasses(const Dev& d, const FitLitIdx& x, int e, const uint64_t* mask, const int64_t* req) {
  int n = x.node[e];
  if (!((mask[n >> 6] >> (n & 63)) & 1)) return false;
  for (int r = 0; r < d.cfg.R; r++) if (req[r] > x.al[(size_t)r * x.stride + e]) return false;
  return true;
}
// NodeTypeIterator.NextNode.  mask != NULL (a row of ONE node type): a yielded entry that fails flPasses is a "go on" (header).  `it` is the same in every lane.
FL_FN void flAdvance(const Dev& d, const FitLitIdx& x, FlIt& it, const int64_t* ireq, const uint64_t* mask, const int64_t* req) {
  const DevCfg& c = d.cfg;
  for (;;) {
    if (it.pos >= it.end) { it.head = -1; return; }
    int e = it.pos + FL_LANE, cls = 0;
    int64_t nlb[MAXK];
    for (int i = 0; i < MAXK; i++) nlb[i] = 0;
    if (e < it.end) {
      cls = flClassify(c, x, e, it.lb, ireq, nlb);
      if (cls == 1 && mask && !flPasses(d, x, e, mask, req)) cls = 0;
    }
    unsigned long long m = FL_BALLOT(cls != 0);
    if (!m) { it.pos += FL_NL; continue; }
    int first = __builtin_ctzll(m);
    if (FL_SHFL(cls, first) == 1) { it.head = it.pos + first; it.pos += first + 1; return; }
    FL_UNROLL
    for (int i = 0; i < MAXK; i++) if (i < c.K) it.lb[i] = FL_SHFL(nlb[i], first);
    unsigned long long b = flBound(c, it.lb);
    it.pos = b == ~0ull ? it.end : flLowerBound(x, it.beg, it.end, b);
  }
}
FL_FN bool flNodeLess(const Dev& d, const FitLitIdx& x, int a, int b) {   // nodeTypesIteratorPQ.less (:170-185) of two entries
  for (int i = 0; i < d.cfg.K; i++) {
    int64_t qa = x.al[(size_t)d.cfg.indexedCol[i] * x.stride + a], qb = x.al[(size_t)d.cfg.indexedCol[i] * x.stride + b];
    if (qa < qb) return true;
    if (qa > qb) return false;
  }
  return d.nodeIdRank[x.node[a]] < d.nodeIdRank[x.node[b]];
}
// one query: the first node the merged iterators of mask row `row` yield that passes the row's static mask and fitsAlloc at the index's level; -1 none.
// its: LIT_TMAX iterator states of this wave's own (LDS on the device).  Every lane returns the same value.
FL_FN int flQuery(const Dev& d, const FitLitIdx& x, int row, FlIt* its) {
  const DevCfg& c = d.cfg;
  const int64_t* req = d.shapeReq + (size_t)row * c.R;
  const uint64_t* mask = d.shapeMask + (size_t)row * c.W;
  int64_t ireq[MAXK];
  FL_UNROLL
  for (int i = 0; i < MAXK; i++) ireq[i] = i < c.K ? req[c.indexedCol[i]] : 0;
  int t0 = d.rowTypeOff[row], nT = d.rowTypeOff[row + 1] - t0;
  if (nT <= 0 || nT > LIT_TMAX) return -1;   // (more than LIT_TMAX types: refused at upload)
  const bool single = nT == 1;
  for (int k = 0; k < nT; k++) {   // NewNodeTypesIterator (:84-123)
    FlIt it;
    int type = d.rowTypes[t0 + k];
    it.beg = x.typeBeg[type]; it.end = x.typeEnd[type]; it.head = -1;
    for (int i = 0; i < MAXK; i++) it.lb[i] = ireq[i];
    unsigned long long b = flBound(c, it.lb);
    it.pos = b == ~0ull ? it.end : flLowerBound(x, it.beg, it.end, b);
    flAdvance(d, x, it, ireq, single ? mask : nullptr, req);
    its[k] = it;
  }
  if (single) return its[0].head < 0 ? -1 : x.node[its[0].head];
  for (;;) {
    int best = -1;
    for (int k = 0; k < nT; k++) if (its[k].head >= 0 && (best < 0 || flNodeLess(d, x, its[k].head, its[best].head))) best = k;
    if (best < 0) return -1;
    int e = its[best].head;
    FlIt it = its[best];
    flAdvance(d, x, it, ireq, nullptr, req);   // NextNode (:134-149) advances the popped iterator before returning the node
    its[best] = it;
    if (flPasses(d, x, e, mask, req)) return x.node[e];
  }
}

#ifdef ASCHED_HOSTSIM
// ---- the CPU build's plat_run_fit_batch_lit (plat.h): the same per-element functions serially, std::sort for the bitonic network
#include <algorithm>
#include <vector>
static int plat_run_fit_batch_lit(Dev& d, const int32_t* nodeType, int nTypes, const std::vector<int32_t>& rows, int level, std::vector<int32_t>& out, bool reuseIndex, double) {
  static thread_local std::vector<FlPair> pairs;
  static thread_local std::vector<unsigned long long> key;
  static thread_local std::vector<int32_t> node, tb, te;
  static thread_local std::vector<int64_t> al;
  const int N = d.cfg.N;
  FitLitIdx x;
  if (!reuseIndex) {
    pairs.resize((size_t)N + 1); key.resize((size_t)N + 1); node.resize((size_t)N + 1); al.resize((size_t)d.cfg.R * N + 1);
    tb.assign((size_t)nTypes + 1, 0); te.assign((size_t)nTypes + 1, 0);
  }
  x.key = key.data(); x.node = node.data(); x.al = al.data(); x.typeBeg = tb.data(); x.typeEnd = te.data(); x.n = N; x.stride = N; x.level = level; x.pad = 0;
  if (!reuseIndex) {
    for (int i = 0; i <= N; i++) flFill(d, nodeType, level, pairs.data(), i);   // (one padding record behind the last node: flFinish looks at a[i + 1] only for i < N - 1)
    std::sort(pairs.begin(), pairs.begin() + N, flPairLess);
    for (int i = 0; i < N; i++) flFinish(d, x, pairs.data(), i);
  }
  std::vector<FlIt> its(LIT_TMAX);
  for (size_t q = 0; q < rows.size(); q++) out[q] = flQuery(d, x, rows[q], its.data());
  return 0;
}
#endif
