// armada_sched_aux.hip — code object of k_control_aux: the submit-check commands (asched_submit_check; SURVEY 8f-2, internal/scheduler/submitcheck.go:342-371)
// and market-driven rounds (round_mkt.h), one launch of ONE workgroup with no helpers.  Features: ASCHED_MARKET_ROUND.  A separate code object: whatever is
// added to the auxiliary commands can never move a register, an LDS offset or an inlining decision in the round kernel, whose code is the measured one
// (DESIGN.md 3.1, 10).  Device code only: the platform layer that launches it (plat_hip.inc) and the C ABI live in armada_sched.hip.
#define ASCHED_MARKET_ROUND 1
#undef HELP_TRACE   // (the trace variant instruments the round kernel only)
#include <cstring>   // the launch wrappers (host code) at the end of this file
#include "round_kernel.h"

__global__ __launch_bounds__(CTL_THREADS) void k_control_aux(Dev dev, int cmd, HelpBox* box, MktDev mk) {
  // workgroup 0 of k_control without helper workgroups: wave 0 runs the command, the other waves serve its mailbox.  Its own copy of round_body.h with two differences: the stride of a
  // shared pass is blockDim.x, spelled in the OP_BULKW loop, and OP_WIDE is not served.  (Through round_body.h the code is equivalent but the object's register allocation moves.)
  if (threadIdx.x == 0) { g_box = box; g_H = 0; g_gen = 0; g_mk = mk; g_fl.eng.abandon = 0; g_fl.eng.idleSince = 0; g_fl.eng.idleLast = 0; g_fl.eng.idleProg = 0; }
  {
    const int* src = (const int*)&dev; int* dst = (int*)&g_dev;
    for (int i = threadIdx.x; i < (int)(sizeof(Dev) / sizeof(int)); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  Dev& d = g_dev;
  relocateIn(d, cmd);
  if (threadIdx.x >= 64) {
    for (;;) {
      __syncthreads();
      int op = g_mb.op;
      if (op == OP_EXIT) break;
      if (op == OP_SCAN) {
        unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, (int)blockDim.x);
        if ((threadIdx.x & 63) == 0) g_mb.partial[threadIdx.x >> 6] = v;
      } else if (op == OP_FAIR) {
        int v = fairPart(d, g_mb.fair, threadIdx.x, (int)blockDim.x);
        if ((threadIdx.x & 63) == 0) g_mb.waveCount[threadIdx.x >> 6] = v;
      } else if (op == OP_SCANFAIR) {
        unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, (int)blockDim.x);
        int w = fairPart(d, g_mb.fair, threadIdx.x, (int)blockDim.x);
        if ((threadIdx.x & 63) == 0) { g_mb.partial[threadIdx.x >> 6] = v; g_mb.waveCount[threadIdx.x >> 6] = w; }
      } else if (op == OP_BULK) {
        bulkPart(d, g_mb.kind, g_mb.n);
      } else if (op == OP_BULKW) {
        int kd = g_mb.kind, nn = g_mb.n;
        for (int i = threadIdx.x; i < nn; i += (int)blockDim.x) bulkElem(d, kd, i);
        __threadfence();
      } else if (op == OP_COMPACT) {
        compactPart(d);
      } else if (op == OP_ENGINE) {
        if ((threadIdx.x >> 6) == 1) engineLoop(d); else if ((threadIdx.x >> 6) == 2) bindLoop(d); else if ((threadIdx.x >> 6) == 3 && d.f.engineHc) coldLoop(d);
      }
      __syncthreads();
    }
    relocateOut();
    return;
  }
  controlMainAux(d, cmd);
  __threadfence();
  if ((threadIdx.x & 63) == 0) g_mb.op = OP_EXIT;
  __syncthreads();
  relocateOut();
}
extern "C" __attribute__((visibility("hidden"))) int asched_internal_aux_launch(const Dev* dev, int cmd, hipStream_t stream, void* helpBox, const MktDev* mk) {
  MktDev none; memset(&none, 0, sizeof none);
  hipLaunchKernelGGL(k_control_aux, dim3(1), dim3(CTL_THREADS), 0, stream, *dev, cmd, (HelpBox*)helpBox, mk ? *mk : none);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
