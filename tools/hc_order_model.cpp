// tools/hc_order_model.cpp — the order words of the hot set (armada_amd/csrc/hc_order.h) on 64 simulated lanes, against the linear minimum.  No HIP, no GPU:
//   c++ -O2 -std=c++17 -o hc_order_model tools/hc_order_model.cpp && ./hc_order_model [seeds [steps]]        (default 200 seeds x 4000 events)
// The engine wave's five events (engine_hc.h), drawn at random, with the ballots computed by loops over the lanes:
//   insert    a key into an empty lane (the free-lane insert: L = that lane)
//   decrease  a lane's key goes down (hcHotBind, the entry stays alive)
//   death     a lane's entry dies: key ~0, class bits 0 (hcHotBind, nk = ~0)
//   release   a set of lanes gives its entries away: key ~0, every lane clears their bits and NOTHING else is rewritten (the released lanes keep stale words)
//   query     a random subset of the lanes that hold entries "fits": the lane the order words name and its key must be the linear scan's
// Keys are unique as the engine's are: the lane number stands in the low six bits as the node rank does there.  The upper part is drawn from a range that changes
// with the seed — from 4 values (nearly every comparison decided by the low bits) to 2^40.  Exit status 1 on the first difference, with the event that showed it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../armada_amd/csrc/hc_order.h"

static uint64_t rngState;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rngState += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

struct Lanes {
  uint64_t key[64], below[64];
  bool live[64];
};

// lane L takes key nk: what hcOrderSet does on the device (the ballot reads the keys as they stand, lane L's old one included)
static void setKey(Lanes& w, int L, uint64_t nk) {
  uint64_t lt = 0;
  for (int x = 0; x < 64; x++) lt |= (uint64_t)(w.key[x] < nk) << x;
  for (int x = 0; x < 64; x++) w.below[x] = hcOrderUpdate(w.below[x], w.key[x], x, L, nk, lt);
  w.key[L] = nk;
  w.live[L] = nk != ~0ull;
}

int main(int argc, char** argv) {
  const int seeds = argc > 1 ? atoi(argv[1]) : 200, steps = argc > 2 ? atoi(argv[2]) : 4000;
  long long queries = 0, events[5] = {0, 0, 0, 0, 0};
  for (int seed = 0; seed < seeds; seed++) {
    rngState = 0x1234567ull + (uint64_t)seed * 0x10001ull;
    const uint64_t range = (uint64_t)1 << (2 + (seed % 20) * 2);   // values of the keys' upper part
    const int target = 8 + (int)(rnd() % 56);                     // how full the set tends to be (the engine: up to 48 entries and the few in flight)
    Lanes w;
    for (int x = 0; x < 64; x++) { w.key[x] = ~0ull; w.below[x] = 0; w.live[x] = false; }   // a session starts empty
    for (int step = 0; step < steps; step++) {
      int nLive = 0;
      for (int x = 0; x < 64; x++) nLive += w.live[x];
      int ev = (int)(rnd() % 10);   // 0-2 insert, 3-4 decrease, 5 death, 6 release, 7-9 query
      if (ev <= 2 && (nLive == 64 || (nLive >= target && rnd() % 4))) ev = 5 + (int)(rnd() % 2);
      if (ev >= 3 && ev <= 6 && nLive == 0) ev = 0;
      if (ev <= 2) {
        int L = (int)(rnd() % 64);
        while (w.live[L]) L = (L + 1) & 63;
        if (rnd() % 2) { L = 0; while (w.live[L]) L++; }   // the engine takes the lowest free lane
        setKey(w, L, ((rnd() % range) << 6) | (uint64_t)L);
        events[0]++;
      } else if (ev <= 5) {
        int L = (int)(rnd() % 64);
        while (!w.live[L]) L = (L + 1) & 63;
        const uint64_t up = w.key[L] >> 6;
        if (ev <= 4 && up > 0) { setKey(w, L, ((rnd() % up) << 6) | (uint64_t)L); events[1]++; }
        else { setKey(w, L, ~0ull); events[2]++; }
      } else if (ev == 6) {
        uint64_t rb = rnd() & rnd();
        if (rnd() % 3 == 0) rb &= rnd();
        for (int x = 0; x < 64; x++) if (!w.live[x]) rb &= ~((uint64_t)1 << x);
        for (int x = 0; x < 64; x++) if ((rb >> x) & 1) { w.key[x] = ~0ull; w.live[x] = false; }
        for (int x = 0; x < 64; x++) w.below[x] = hcOrderRelease(w.below[x], rb);
        events[3]++;
      } else {
        uint64_t fitMask = rnd();
        const int thin = (int)(rnd() % 4);
        if (thin == 1) fitMask &= rnd(); else if (thin == 2) fitMask |= rnd(); else if (thin == 3) fitMask = rnd() % 8 ? ~0ull : 0;
        for (int x = 0; x < 64; x++) if (!w.live[x]) fitMask &= ~((uint64_t)1 << x);   // an empty lane fits nothing
        uint64_t who = 0;
        for (int x = 0; x < 64; x++) who |= (uint64_t)hcOrderFirst((fitMask >> x) & 1, w.below[x], fitMask) << x;
        const int gotLane = who ? __builtin_ctzll(who) : -1;
        const uint64_t gotKey = who ? w.key[gotLane] : ~0ull;
        int wantLane = -1; uint64_t wantKey = ~0ull;
        for (int x = 0; x < 64; x++) if (((fitMask >> x) & 1) && w.key[x] < wantKey) { wantKey = w.key[x]; wantLane = x; }
        if (gotLane != wantLane || gotKey != wantKey || (who & (who - 1)) != 0) {
          fprintf(stderr, "hc_order_model: seed %d step %d: fit mask %016llx: order words name lane %d key %016llx (lanes %016llx), linear scan lane %d key %016llx\n", seed, step,
                  (unsigned long long)fitMask, gotLane, (unsigned long long)gotKey, (unsigned long long)who, wantLane, (unsigned long long)wantKey);
          return 1;
        }
        queries++; events[4]++;
      }
    }
  }
  printf("hc_order_model: %d seeds x %d events: %lld inserts, %lld decreases, %lld deaths, %lld releases, %lld queries, every query equal to the linear scan\n", seeds, steps,
         events[0], events[1], events[2], events[3], queries);
  return 0;
}
