// armada_sched.hip — MI355X (gfx950) implementation of the C ABI in include/armada_sched.h: the translation unit of the round kernel, the grid-wide
// kernels, the HIP platform layer and the ABI.  There is no CPU compute path in this library: without a gfx950 device asched_create() fails.
//
// Code objects of libarmada_sched.so, one per .hip file:
//   armada_sched.hip       k_control, the grid-wide kernels, the platform layer and the C ABI; no optional feature of the round kernel
//   armada_sched_aux.hip   k_control_aux: the submit-check commands and market-driven rounds
//   armada_sched_wk.hip    k_control_wk, k_bulk_wk, k_fit_batch_wk: two-word order keys, sharded wide passes, market-driven rounds
//   armada_sched_mgpu.hip  the multi-GPU exchange, submit-gang, evicted-table-rank and literal first-fit (kernels_fit_lit.h) kernels
// What this file is made of, in the order it includes them (kernel definition order is the code object's text order: keep it):
//   round_kernel.h    device code every round kernel shares: the control code (round_run.h ...), the worker waves' LDS mailbox and its ops (OP_SCAN,
//                     OP_BULK, OP_COMPACT, OP_FAIR, OP_ENGINE, ...), the helper workgroups' HBM mailbox, the fast path and node engine
//   round_body.h      workgroup 0 of k_control / k_control_wk as text: stage Dev in LDS, relocateIn, the worker waves' loop, relocateOut
//   kernels_split.h   k_bulk, k_round_small, k_evict_apply, k_cmp_*, k_seg_off: the grid-wide phases of the split round
//   kernels_opt.h     k_opt_*, k_price_*: fairness optimiser and indicative pricer
//   kernels_fit.h     k_shape_mask, k_fit_batch, k_base_* / k_bitonic_* (sorted base), k_agg, k_drf / k_fair (float64 goldens)
//   plat.h            the platform interface asched_host.inc is written against (declarations only)
//   plat_hip.inc      its HIP implementation: PlatCtx, RCCL binding, exchange areas, memory, every kernel launch (host code only)
//   asched_host.inc   the C ABI: marshalling, upload, launches through plat_*, download (shared with the CPU build of the tests)
#include "round_kernel.h"

// The round kernel.  Workgroup 0: wave 0 runs the command (controlMain), waves 1..3 serve its LDS mailbox; workgroups 1..H are helpers (helperMain).
__global__ __launch_bounds__(CTL_THREADS) void k_control(Dev dev, int cmd, HelpBox* box, int H) {
  if (blockIdx.x != 0) { helperMain(dev, box, H); return; }
  if (threadIdx.x == 0) { g_box = box; g_H = H; g_gen = 0; g_fl.eng.abandon = 0; g_fl.eng.idleSince = 0; g_fl.eng.idleLast = 0; g_fl.eng.idleProg = 0; }
#define ROUND_STRIDE ((g_H + 1) * (int)blockDim.x)
#define ROUND_SERVES_WIDE 1
#include "round_body.h"
  controlMain(d, cmd);
  __threadfence();
  if ((threadIdx.x & 63) == 0) { g_mb.op = OP_EXIT; if (g_H) helpIssue(OP_HELPERS_EXIT, (const ScanArgs*)nullptr); }
  __syncthreads();
  relocateOut();
}

#include "kernels_split.h"
#include "kernels_opt.h"
#include "kernels_fit.h"

#include "plat.h"
#include "plat_hip.inc"
#include "asched_host.inc"


#ifdef HELP_TRACE
extern "C" int asched_debug_help_trace(unsigned long long* out64) { return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_traceSum), 64 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1; }
#endif
