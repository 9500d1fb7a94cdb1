// round_body.h — workgroup 0 of a round kernel as TEXT, from staging the Dev descriptor in LDS to the end of the worker waves' branch (relocateIn, the
// loop over the mailbox ops, relocateOut).  Included inside the body of k_control (armada_sched.hip) and k_control_wk (armada_sched_wk.hip) after the kernel
// has dispatched its helper workgroups and set its LDS words; wave 0 leaves at the bottom with `Dev& d` and runs the kernel's own command and exit sequence.
// Text and not a function: as a __forceinline__ template the inliner decides differently and both kernels' code changes (tools/kcontrol_isa_hash.sh).
// The includer defines, and this file #undefs:
//   ROUND_STRIDE       int expression, the threads that share one wide pass: ((g_H + 1) * (int)blockDim.x)
//   ROUND_SERVES_WIDE  0 / 1: whether the worker waves serve OP_WIDE
// A new mailbox op is added here and in k_control_aux's own copy (armada_sched_aux.hip).  No include guard: one inclusion per kernel body.
#if !defined(ROUND_STRIDE) || !defined(ROUND_SERVES_WIDE)
#error "round_body.h: define ROUND_STRIDE and ROUND_SERVES_WIDE before including it"
#endif
  // the Dev descriptor (pointers + config) is staged in LDS once; every wave reads it from there
  {
    const int* src = (const int*)&dev; int* dst = (int*)&g_dev;
    for (int i = threadIdx.x; i < (int)(sizeof(Dev) / sizeof(int)); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  Dev& d = g_dev;
  relocateIn(d, cmd);
  if (threadIdx.x >= 64) {  // worker waves: serve mailbox requests until OP_EXIT
    for (;;) {
      __syncthreads();
      int op = g_mb.op;
      if (op == OP_EXIT) break;
      if (op == OP_SCAN) {
        unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, ROUND_STRIDE);
        if ((threadIdx.x & 63) == 0) g_mb.partial[threadIdx.x >> 6] = v;
      } else if (op == OP_FAIR) {
        int v = fairPart(d, g_mb.fair, threadIdx.x, ROUND_STRIDE);
        if ((threadIdx.x & 63) == 0) g_mb.waveCount[threadIdx.x >> 6] = v;
      } else if (op == OP_SCANFAIR) {
        unsigned long long v = scanPart(d, g_mb.scan, threadIdx.x, ROUND_STRIDE);
        int w = fairPart(d, g_mb.fair, threadIdx.x, ROUND_STRIDE);
        if ((threadIdx.x & 63) == 0) { g_mb.partial[threadIdx.x >> 6] = v; g_mb.waveCount[threadIdx.x >> 6] = w; }
      } else if (op == OP_BULK) {
        bulkPart(d, g_mb.kind, g_mb.n);
      } else if (op == OP_BULKW) {
        int nthreads = ROUND_STRIDE; int kd = g_mb.kind, nn = g_mb.n;
        for (int i = threadIdx.x; i < nn; i += nthreads) bulkElem(d, kd, i);
        __threadfence();
      }
#if ROUND_SERVES_WIDE
      else if (op == OP_WIDE) {
        int nthreads = ROUND_STRIDE; int kd = g_mb.kind, nn = g_mb.n;
        for (int i = threadIdx.x; i < nn; i += nthreads) wideBulkAny(d, kd, i);
        __threadfence();
      }
#endif
      else if (op == OP_COMPACT) {
        compactPart(d);
      } else if (op == OP_ENGINE) {
        if ((threadIdx.x >> 6) == 1) engineLoop(d); else if ((threadIdx.x >> 6) == 2) bindLoop(d); else if ((threadIdx.x >> 6) == 3 && d.f.engineHc) coldLoop(d);
      }
      __syncthreads();
    }
    relocateOut();
    return;
  }
#undef ROUND_STRIDE
#undef ROUND_SERVES_WIDE
