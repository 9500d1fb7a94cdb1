// hc_order.h — the key order among the lanes of the hot set H (engine_hc.h), kept and patched, not recomputed.  Plain integers in, plain integers out: the engine wave
// (device) and tools/hc_order_model.cpp (host, 64 simulated lanes) compile this one text.
//
// Each lane keeps one 64-bit word `below`: bit x is set iff lane x holds an entry whose key is SMALLER than this lane's key.  Keys of entries are unique (the node-index
// rank sits in the low bits), so the order is total: among any set of lanes that hold entries exactly one has no set bit of `below` inside that set — the one with the
// smallest key.  An empty lane has key ~0 and fits nothing: it is in no fit mask, so its bit in another lane's word is never looked at, and its own word is never asked.
// Both are rewritten when the lane next receives a key (hcOrderUpdate with L = that lane), so whatever they hold in between is of no consequence.
//
//   query    fitMask = ballot(fit); the first-fit lane is the one with hcOrderFirst(); no such lane: none fits.
//   update   lane L's key becomes nk (~0: the entry died).  lt = ballot(key < nk), any lane's old or new key in lane L's place: the function masks bit L.
//            Lane L takes lt; every other lane rewrites bit L.
//   release  the lanes of `rb` give their entries away (key ~0): every lane clears their bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HC_ORDER_FN __host__ __device__ static inline
#else
#define HC_ORDER_FN static inline
#endif

// does this lane hold the smallest key among the lanes of fitMask?  (fit: this lane's own bit of fitMask)
HC_ORDER_FN bool hcOrderFirst(bool fit, uint64_t below, uint64_t fitMask) { return fit & ((below & fitMask) == 0); }

// this lane's `below` after lane L's key became nk.  key: this lane's key (lane L's own is not read); lt: the lanes whose key is smaller than nk
HC_ORDER_FN uint64_t hcOrderUpdate(uint64_t below, uint64_t key, int lane, int L, uint64_t nk, uint64_t lt) {
  // (The xor form of the merge is what the device compiler turns into ONE bit-field insert per half under the scalar mask bitL; written as (below & ~bitL) | (nk < key ?
  //  bitL : 0) it became two moves, two selects, two ANDs and two ORs.  profiles/r17_hc_order_matrix.txt)
  const uint64_t bitL = (uint64_t)1 << L;
  const uint64_t sel = (uint64_t)0 - (uint64_t)(nk < key);
  const uint64_t others = below ^ ((below ^ sel) & bitL);   // bit L of `below` replaced by nk < key
  return lane == L ? (lt & ~bitL) : others;
}

// this lane's `below` after the lanes of rb gave their entries away
HC_ORDER_FN uint64_t hcOrderRelease(uint64_t below, uint64_t rb) { return below & ~rb; }
