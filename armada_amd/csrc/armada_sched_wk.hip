// armada_sched_wk.hip — code object of k_control_wk, k_bulk_wk and k_fit_batch_wk: the round kernel once more, for the handles the default kernels do not serve, so
// that nothing of what follows moves an instruction of k_control (tools/kcontrol_isa_hash.sh).  Features: ASCHED_TWO_WORD_KEYS, ASCHED_SHARDED_PASSES, ASCHED_MARKET_ROUND.
//  * ORDER KEYS OF TWO WORDS.  The reference's index key is one 8-byte word per indexed resource plus the node index (internal/scheduler/nodedb/encoding.go:22-54), unbounded; the
//    packed key of the default kernels is one 64-bit word.  When a pool needs more (asched_host.inc layoutKeys: fine resolutions, large nodes, a fifth indexed resource, a million
//    nodes) the key is one 128-bit integer stored as (high word, low word); the handle runs on the generic path — the reference statement by statement, round_ctl.h / round_run.h —
//    and node selection is two plane passes (round_kernel.h wgFirstFitKey).  WIDE_KEYS() is a run-time test here (dev.h), a compile-time `false` in every other code object.
//  * SHARDED WIDE PASSES: one pool's round on several GPUs, exact (asched_shard_round / asched_shard_peers; dev.h SHARD_ON, round_kernel.h shardReduce): the plane scan and the
//    fair-share evaluation look at this replica's share of the node words and exchange their two result words — through the host proxy or GPU-to-GPU.  One-word handles keep
//    their fast path here (the whole round kernel is compiled in).
//  * every control command of such a handle, the auxiliary ones and market-driven rounds included.
// Device code only: workgroup 0's body is round_body.h, shared with k_control; the platform layer that launches these kernels (plat_hip.inc) and the C ABI live in armada_sched.hip.
#define ASCHED_TWO_WORD_KEYS 1
#define ASCHED_SHARDED_PASSES 1
#define ASCHED_MARKET_ROUND 1
#include <cstring>   // the launch wrappers (host code) at the end of this file
#include "round_kernel.h"

__global__ __launch_bounds__(CTL_THREADS) void k_control_wk(Dev dev, int cmd, HelpBox* box, int H, MktDev mk) {
  if (threadIdx.x == 0 && blockIdx.x != 0) g_mk = mk;   // (helper workgroups: the market state's HBM homes — none of the bodies they serve looks at it; never garbage)
  if (threadIdx.x == 0 && blockIdx.x == 0) {   // (market-driven rounds of such a handle run here too: round_mkt.h)
    g_mk = mk; g_xgen = 0; g_xpeers = 0;       // the exchange generation of sharded passes restarts with every launch through the host proxy ...
    if (dev.cfg.shardWorld > 1 && dev.cancel) {
      const unsigned long long* X = (const unsigned long long*)dev.cancel;
      unsigned long long pt = __hip_atomic_load(&X[XCHG_WORD0 + 6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (pt) {                                // ... and goes on where the last launch left it GPU-to-GPU (the peers' counters do not restart either)
        g_xpeers = pt;
        g_xgen = (unsigned int)__hip_atomic_load(((unsigned long long* const*)pt)[dev.cfg.shardRank], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store((unsigned long long*)&X[XCHG_WORD0 + 7], (unsigned long long)g_xgen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (the launch's first generation: its end turns this into a count)
      }
    }
  }
  if (blockIdx.x != 0) { helperMain(dev, box, H); return; }
  if (threadIdx.x == 0) { g_box = box; g_H = H; g_gen = 0; g_fl.eng.abandon = 0; g_fl.eng.idleSince = 0; g_fl.eng.idleLast = 0; g_fl.eng.idleProg = 0; }
#define ROUND_STRIDE ((g_H + 1) * (int)blockDim.x)
#define ROUND_SERVES_WIDE 1
#include "round_body.h"
  if (cmd >= CMD_AUX_FIRST) controlMainAux(d, cmd); else
  controlMain(d, cmd);
  // GPU-to-GPU exchanges of this launch, for asched_shard_exchanges (the host counts the proxy's itself): the counter went on from the area's word
  if (threadIdx.x == 0 && g_xpeers) {
    unsigned long long* X = (unsigned long long*)d.cancel;
    unsigned int start = (unsigned int)__hip_atomic_load(&X[XCHG_WORD0 + 7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&X[XCHG_WORD0 + 7], (unsigned long long)(g_xgen - start), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence();
  if ((threadIdx.x & 63) == 0) { g_mb.op = OP_EXIT; if (g_H) helpIssue(OP_HELPERS_EXIT, (const ScanArgs*)nullptr); }
  __syncthreads();
  relocateOut();
}

__global__ __launch_bounds__(256) void k_bulk_wk(Dev d, int kind, int n) {
  // (the element bodies ask mkOn(): this code object carries the market-driven round, whose state is an LDS copy of a kernel argument of k_control_wk.  A market round is ONE
  //  launch of that kernel — the grid-wide phases never belong to one: no market state here)
  if (threadIdx.x == 0) memset(&g_mk, 0, sizeof g_mk);
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) bulkElem(d, kind, i);
}
// k_fit_batch (kernels_fit.h) for a two-word key, one launch per word: pass 0 leaves the minimum HIGH word among a shape's fitting nodes in out[i][0],
// pass 1 the minimum LOW word among the fitting nodes that carry it in out[i][1] (the node-index rank is in its low bits).
#define FIT_TILE_WK 256
__global__ __launch_bounds__(FIT_TILE_WK) void k_fit_batch_wk(Dev d, const int32_t* shapes, int nshapes, int level, unsigned long long* out, int pass) {
  const DevCfg& c = d.cfg;
  int n = blockIdx.x * FIT_TILE_WK + threadIdx.x;
  bool valid = n < c.N;
  unsigned long long hi = valid ? d.keys[(size_t)level * c.Npad + n] : ~0ull;
  unsigned long long lo = (valid && pass) ? d.keys[((size_t)c.P + level) * c.Npad + n] : ~0ull;
  int64_t al[MAXR];
  for (int r = 0; r < MAXR; r++) al[r] = (valid && r < c.R) ? d.alloc[((size_t)level * c.R + r) * c.Npad + n] : 0;
  int per = (nshapes + gridDim.y - 1) / gridDim.y;
  int s0 = blockIdx.y * per, s1 = min(nshapes, s0 + per);
  int word = n >> 6, bit = n & 63;
  __shared__ unsigned long long wmin[FIT_TILE_WK / 64];
  for (int i = s0; i < s1; i++) {
    int s = shapes[i];
    bool f = valid && ((d.shapeMask[(size_t)s * c.W + word] >> bit) & 1);
    const int64_t* req = d.shapeReq + (size_t)s * c.R;
    for (int r = 0; r < c.R; r++) f = f && req[r] <= al[r];
    unsigned long long key = hi;
    if (pass) { f = f && hi == out[(size_t)i * FIT_OSTR]; key = lo; }   // (word 0 is final: pass 0 completed on this stream)
    unsigned long long v = __ballot(f) ? waveMin64Dpp(f ? key : ~0ull) : ~0ull;
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long m = wmin[0];
      for (int w = 1; w < FIT_TILE_WK / 64; w++) m = wmin[w] < m ? wmin[w] : m;
      unsigned long long* o = &out[(size_t)i * FIT_OSTR + pass];
      if (m != ~0ull && m < __hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(o, m);
    }
    __syncthreads();
  }
}
extern "C" __attribute__((visibility("hidden"))) int asched_internal_wk_fit_batch(const Dev* dev, const int32_t* shapes, int ns, int level, unsigned long long* out, int tiles, int ysplit, hipStream_t stream) {
  for (int pass = 0; pass < 2; pass++) hipLaunchKernelGGL(k_fit_batch_wk, dim3(tiles, ysplit), dim3(FIT_TILE_WK), 0, stream, *dev, shapes, ns, level, out, pass);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" __attribute__((visibility("hidden"))) int asched_internal_wk_launch(const Dev* dev, int cmd, hipStream_t stream, void* helpBox, int H, const MktDev* mk) {
  MktDev none; memset(&none, 0, sizeof none);
  hipLaunchKernelGGL(k_control_wk, dim3(1 + H), dim3(CTL_THREADS), 0, stream, *dev, cmd, (HelpBox*)helpBox, H, mk ? *mk : none);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" __attribute__((visibility("hidden"))) int asched_internal_wk_bulk(const Dev* dev, int kind, int n, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(k_bulk_wk, dim3(grid), dim3(256), 0, stream, *dev, kind, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
