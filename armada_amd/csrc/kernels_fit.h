// kernels_fit.h — grid-wide kernels around the node state: static shape masks, the batched first-fit query, the sorted base of the level-0 fast
// structure (fill / bitonic sort / finish / fit bitmaps), the round-input builder's sums (k_agg: it sits between the base build's kernels because the
// code object's text follows definition order) and the float64 goldens.  Defined in armada_sched.hip's code object only; launched by plat_hip.inc
// (plat_run_shape_mask, plat_run_fit_batch*, plat_build_base, plat_agg, plat_run_drf, plat_run_fair_shares).
#pragma once
__global__ void k_shape_mask(Dev d, const uint64_t* classMask, const int32_t* shapeClass) {
  const DevCfg& c = d.cfg;
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)c.S * c.W) return;
  int s = (int)(t / c.W), w = (int)(t % c.W);
  uint64_t cm = classMask[(size_t)shapeClass[s] * c.W + w], m = 0;
  for (int b = 0; b < 64; b++) {
    int n = w * 64 + b;
    if (n >= c.N) break;
    if (!((cm >> b) & 1)) continue;
    bool ok = true;
    for (int r = 0; r < c.R; r++) ok = ok && d.shapeReq[(size_t)s * c.R + r] <= d.totalRes[(size_t)r * c.Npad + n];  // nodematching.go:184
    if (ok) m |= 1ull << b;
  }
  d.shapeMask[t] = m;
}

// First feasible node for a batch of (shape) queries at one level against the current node state.
// grid.x tiles the nodes (one node per thread, its key and R alloc values stay in registers for the whole
// shape loop), grid.y splits the shape list.  HBM traffic per launch = N*(8 + 8R) bytes + masks.
#define FIT_TILE 256
__global__ __launch_bounds__(FIT_TILE) void k_fit_batch(Dev d, const int32_t* shapes, int nshapes, int level, unsigned long long* out) {
  const DevCfg& c = d.cfg;
  int n = blockIdx.x * FIT_TILE + threadIdx.x;
  bool valid = n < c.N;
  unsigned long long key = valid ? d.keys[(size_t)level * c.Npad + n] : ~0ull;
  int64_t al[MAXR];
  for (int r = 0; r < MAXR; r++) al[r] = (valid && r < c.R) ? d.alloc[((size_t)level * c.R + r) * c.Npad + n] : 0;
  int per = (nshapes + gridDim.y - 1) / gridDim.y;
  int s0 = blockIdx.y * per, s1 = min(nshapes, s0 + per);
  int word = n >> 6, bit = n & 63;
  __shared__ unsigned long long wmin[FIT_TILE / 64];
  for (int i = s0; i < s1; i++) {
    int s = shapes[i];
    bool f = valid && ((d.shapeMask[(size_t)s * c.W + word] >> bit) & 1);
    const int64_t* req = d.shapeReq + (size_t)s * c.R;
    for (int r = 0; r < c.R; r++) f = f && req[r] <= al[r];
    unsigned long long v = __ballot(f) ? waveMin64Dpp(f ? key : ~0ull) : ~0ull;
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = v;
    __syncthreads();
    // ONE look / write per workgroup and shape, at a word that has a cache line of its own.  (Round 3: every wave sent its minimum to out[i], 8 bytes from out[i + 1]: 100 000
    // read-modify-writes on four cache lines at 100 000 nodes x 64 shapes, serialised in one L2 channel — 0.19 ms for a 4 MB problem.)  The word only ever falls, and first fit
    // means it falls early: look first, write only what improves it.
    if (threadIdx.x == 0) {
      unsigned long long m = wmin[0];
      for (int w = 1; w < FIT_TILE / 64; w++) m = wmin[w] < m ? wmin[w] : m;
      if (m != ~0ull && m < __hip_atomic_load(&out[(size_t)i * FIT_OSTR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&out[(size_t)i * FIT_OSTR], m);
    }
    __syncthreads();
  }
}

// ---- sorted base of the level-0 fast structure: the ordered index of the fresh NodeDb (nodedb.go:1164-1175), built in round_prepare
__global__ void k_base_fill(Dev d, int nb2) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb2) d.baseKey[i] = i < d.cfg.N ? fastKeyOf(d, i) : ~0ull;  // level 0 plane of keys (a negative column: field 0, fits nothing)
}
__global__ void k_bitonic_step(unsigned long long* a, int j, int k) {
  unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned l = i ^ (unsigned)j;
  if (l > i) {
    unsigned long long x = a[i], y = a[l];
    bool up = (i & (unsigned)k) == 0;
    if (up ? x > y : x < y) { a[i] = y; a[l] = x; }
  }
}
// the in-LDS part of the network: every (k, j) step with j < 2048 for one 4096-key tile, 1024 threads
__global__ __launch_bounds__(1024) void k_bitonic_tile(unsigned long long* a, int kStart, int kEnd, int jStart) {
  __shared__ unsigned long long t[4096];
  unsigned base = blockIdx.x * 4096u;
  for (int i = threadIdx.x; i < 4096; i += 1024) t[i] = a[base + i];
  __syncthreads();
  for (int k = kStart; k <= kEnd; k <<= 1) {
    for (int j = (k == kStart ? jStart : k >> 1); j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < 4096; i += 1024) {
        unsigned l = (unsigned)i ^ (unsigned)j;
        if (l > (unsigned)i) {
          unsigned long long x = t[i], y = t[l];
          bool up = ((base + i) & (unsigned)k) == 0;
          if (up ? x > y : x < y) { t[i] = y; t[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < 4096; i += 1024) a[base + i] = t[i];
}
__global__ void k_base_finish(Dev d) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  const DevCfg& c = d.cfg;
  if (i >= c.N) return;
  unsigned long long key = d.baseKey[i];
  int node = d.nodeByRank[key & ((1ull << c.idxBits) - 1)];
  d.baseNode[i] = node; d.posOf[node] = i; d.baseRemoved[i] = 0; d.baseCls[i] = d.nodeCls[node]; d.l0Slot[node] = -1;
  for (int e = 0; e < d.f.E; e++) d.baseExtra[(size_t)e * c.Npad + i] = d.alloc[(size_t)d.f.extraCol[e] * c.Npad + node];  // level 0 planes
}


// The round-input builder's sums (round_run.h B_AGG_RUN / B_AGG_QUEUED) grid-wide with the wave-level pre-reduction of k_evict_apply: both walks are
// ordered by queue (the pre-sorted job order; the queued lists), so a wave holds a handful of (queue, class) keys and leaves one atomic per key and resource.
__global__ __launch_bounds__(256) void k_agg(Dev d, int queued, int total) {
  const DevCfg& c = d.cfg;
  int lane = threadIdx.x & 63;
  int rounds = (total + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int it = 0; it < rounds; it++) {   // wave-uniform trip count
    int i = (it * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    bool act = false; int key = -1; int64_t V[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; r++) V[r] = 0;
    if (i < total) {
      int j, q;
      if (queued) {
        int lo = 0, hi = c.Q;
        while (lo < hi) { int mid = (lo + hi) >> 1; if (d.queuedOff[mid + 1] <= i) lo = mid + 1; else hi = mid; }
        q = lo; j = d.queuedJobs[i];
        act = q < c.Q && !d.qCordoned[q];
      } else {
        j = d.ordAll[i]; q = d.jQueue[j];
        act = d.jNode0[j] >= 0 && q >= 0 && q < c.Q;
      }
      if (act) { key = q * c.npc + d.jPc[j]; const int64_t* req = JREQ(d, j); for (int r = 0; r < MAXR; r++) if (r < c.R) V[r] = req[r]; }
    }
    unsigned long long todo = __ballot(act);
    while (todo) {
      int first = __ffsll((long long)todo) - 1;
      int k0 = __shfl(key, first, 64);
      unsigned long long sel = __ballot(act && key == k0) & todo;
      for (int r = 0; r < c.R; r++) {
        int64_t v = waveSumSel(V[r], sel);
        if (lane == 0 && v) { size_t ix = (size_t)k0 * c.R + r; atomicAddI64(&d.qDemandByPc[ix], v); if (!queued) atomicAddI64(&d.qAllocByPc[ix], v); }
      }
      todo &= ~sel;
    }
  }
}
// the fit bitmaps of a fresh base (round_fast.h fitBitsWord): one thread per (fit shape, 64 entries)
__global__ void k_base_fitbits(Dev d) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)d.f.F * d.fitW;
  if (i >= total) return;
  d.fitBits[i] = fitBitsWord(d, (int)(i / d.fitW), (int)(i % d.fitW));
}
__global__ void k_drf(Dev d, const int64_t* alloc, double* out) { if (threadIdx.x == 0) *out = drf(d, alloc); }
__global__ void k_fair(Dev d, const double* cds) { if (threadIdx.x == 0) updateFairShares(d, cds); }
