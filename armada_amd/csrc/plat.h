// plat.h — the platform interface asched_host.inc is written against: declarations, and the table of the measurement hooks.  Two implementations, each linked by name inside the one
// translation unit that includes asched_host.inc: plat_hip.inc (the product: HIP streams, kernel launches, RCCL) and tests/hostsim/hostsim.cpp (the CPU
// build of the tests: serial loops over the same per-element device functions).  PlatCtx is defined per build.  Default arguments live here only.
// Included after the control code (round_run.h, round_opt.h, round_price.h: Dev, MktDev, OptArgs, PriceArgs, asched_allreduce_fn) and before the definitions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>
#include "round_opt.h"
#include "round_price.h"

struct PlatCtx;
struct GlobalKeyLayout;   // mgpu.h

// ---- context / errors.  One PlatCtx per handle; every ABI entry starts with plat_enter(handle context) and every other call works on the entered context.
// plat_open leaves the new context entered; on failure it returns nullptr and fills err.  plat_last_error: the text of the last failure.
static PlatCtx* plat_open(std::string& err, int device);
static void plat_close(PlatCtx* c);
static void plat_enter(PlatCtx* c);
static const char* plat_last_error();
static bool plat_take_failure();
static int plat_wall_clock_khz();

// ---- memory and copies.  Device (plat_malloc) and pinned host (plat_pinned) memory; plat_malloc returns nullptr on failure.  Copies and memsets return
// nothing: a failure latches in the context and is read (and cleared) with plat_take_failure.  plat_d2h_async completes at plat_sync.
static void* plat_malloc(size_t n);
static void* plat_try_malloc(size_t n);   // an allocation whose failure the caller handles by refusing the call: nullptr when there is no memory, and nothing latched in the context
                                          // (asched_host.inc defines it over plat_malloc unless the platform layer says PLAT_TRY_MALLOC_OWN and brings its own)
static void plat_free(void* p);
static void plat_memset(void* p, int v, size_t n);
static void plat_h2d(void* d, const void* s, size_t n);
static void plat_d2d(void* d, const void* s, size_t n);   // device to device, ordered with the context's other work (asched_jobs_append moves the static per-job arrays into larger blocks)
static void plat_d2h(void* d, const void* s, size_t n);
static void plat_d2h_async(void* d, const void* s, size_t n);
static void plat_sync();
static void* plat_pinned(size_t n);
static void plat_pinned_free(void* p);

// ---- deadline and cancel.  plat_set_deadline(s): maxSchedulingDuration of every following round launch (0 = none).  plat_cancel / plat_cancel_clear take
// the context explicitly: asched_cancel may come from another thread, without plat_enter.
static void plat_set_deadline(double s);
static void plat_cancel(PlatCtx* c);
static void plat_cancel_clear(PlatCtx* c);

// ---- control launches and the split round.  Everything below that returns int: 0, or -1 with the reason in plat_last_error.  plat_run_control runs one
// command of the control code (controlMain / controlMainAux) to completion; plat_set_market_dev sets the market state of the next launch (nullptr: none).
// Between plat_round_begin / plat_round_end the deadline runs from the begin and the launches are counted and timed (plat_round_times: total ms,
// control ms, launches).  The grid-wide steps of the split round work on the HBM state between control launches.
static void plat_set_market_dev(const MktDev* m);
static int plat_run_control(Dev& dev, int cmd);
static double plat_last_control_ms();
static int plat_last_control_launches();
static void plat_round_begin();
static void plat_round_end();
static void plat_round_times(double* out);
static int plat_bulk(Dev& d, int kind, int n);
static int plat_small(Dev& d, int what, int arg);
static int plat_agg(Dev& d, int queued, int total);
static int plat_evict_apply(Dev& d, int phase3, int total);
static int plat_compact(Dev& d, const int32_t* order, int n, const uint8_t* flag, int32_t* dst, uint32_t* prefix, const int32_t* segOff, int nseg, int32_t* outSegOff, int* total);
static int plat_build_base(Dev& d);

// ---- optimiser and pricer.  plat_opt_score scores every node for one job (detailNode >= 0: that node's preemption list too).  detailOnly: the index and
// scores of the previous call are still valid; reuseIndex: so is the node -> jobs index (nothing was bound since) — asched_host.inc decides, an
// implementation may ignore both.  plat_opt_select: 0 = selected on the platform, 1 = not available, take the host loop over plat_opt_score.
static int plat_opt_score(Dev& d, const OptArgs& a, std::vector<OptNodeOut>& scores, double* jobCost, int detailNode, OptNodeOut* detail, std::vector<int32_t>* pre,
                          bool detailOnly = false, bool reuseIndex = false);
static int plat_opt_select(Dev& d, const OptArgs& a, double minPct, bool reuseIndex, int32_t* node, int32_t* npre, double* cost, double* impact, std::vector<int32_t>* pre);
static int plat_opt_qcosts(Dev& d, double* out, int Q);
static double plat_last_opt_ms();
static int plat_price_score(Dev& d, const PriceArgs& a, std::vector<PriceNodeOut>& scores, int detailNode, std::vector<int32_t>* pre);

// ---- fit, submit check and goldens: queries against a fixed node state, synchronous (results are in the host vectors on return).
static int plat_run_shape_mask(Dev& d, const uint64_t* classMask, const int32_t* shapeClass);
static int plat_run_fit_batch(Dev& d, const std::vector<int32_t>& shapes, int level, std::vector<int32_t>& out, const int32_t* nodeByRankHost = nullptr);
// the literal batched first fit (kernels_fit_lit.h): mask rows on the literal iteration path at one level.  nodeType: [N] node type per node in platform memory.  The index
// of the level is built first; reuseIndex: the one the previous call built still describes the node state and level (the passes of ONE submit check).  addMs: kernel time
// of the same batch's packed-key part, added to what plat_last_fit_ms reports afterwards.  The CPU build's definition sits in kernels_fit_lit.h.
static int plat_run_fit_batch_lit(Dev& d, const int32_t* nodeType, int nTypes, const std::vector<int32_t>& rows, int level, std::vector<int32_t>& out, bool reuseIndex, double addMs);
// the preemption-cause join (kernels_preempt_join.h): count, scan, scatter, rank, (gather,) cause over the lists and scratch of `a`, all platform memory; a.cnt and a.info
// zeroed by the caller.  Synchronous: the outputs are complete on return.  The CPU build's definition sits in kernels_preempt_join.h.
struct PjArgs;
static int plat_preempt_join(Dev& d, const PjArgs& a);
// one pass of the evictor report of a round's phase 1 (kernels_evict_report.h: EVR_PASS_JOBS / _NODES / _QUEUES) over the buffers of `a`, all platform memory, queued behind
// the round's other launches: nothing is waited for.  A pass over no elements (no jobs, no nodes) is not launched.  The CPU build's definition sits in kernels_evict_report.h.
struct EvrArgs;
static int plat_evict_report(Dev& d, const EvrArgs& a, int pass);
// ---- measurement hooks: the device ms of the passes of the calls below.  A family is switched on by its environment variable (= 1, read once per process); the
// HIP build then puts events around the family's passes and plat_pass_ms(family, out) gives out[0 .. passes) of the last call of the entered context, zeros for a
// call that ran no pass or did not end well; without the variable, and in the CPU build, zeros.  plat_pass_printed: asched_host.inc prints the family's line.
enum PassLayout { PASS_SEQ, PASS_REV, PASS_PAIRS };   // out[k] is between events k and k + 1 / the same with out[] in reverse order / between events 2k and 2k + 1, each pass with a flag of its own
enum PassFamily {
  PASS_EVR,   // the evictor report: job pass / node pass / queue pass of the last round (read once the round is over)
  PASS_JP,    // plat_jobs_patch, plat_jobs_reprioritise and plat_round_commit: scatter / remove / sort / merge
  PASS_JA,    // plat_jobs_append: row fill / sort / merge
  PASS_SA,    // plat_shapes_append: the new mask rows / the row copies
  PASS_CA,    // plat_req_classes_append: the new rows / the row copies
  PASS_SC,    // plat_shapes_compact: rows / gathers / class bits
  PASS_JD,    // plat_jobs_delete: mark / scan / gather / order / gang lists
  PASS_NP,    // plat_nodes_patch: scatter / mask words
  PASS_ND,    // plat_nodes_delete_check + plat_nodes_delete: mark + check / scan / gather / index order / mask rows / job remap / unmark
  PASS_NA,    // plat_nodes_append: planes / narrow arrays / index order / mask rows
  PASS_QL,    // plat_queued_lists: mark / hold / compact
  PASS_FAMILIES
};
struct PassFamilyInfo { const char* env; int passes; PassLayout layout; };
static constexpr PassFamilyInfo kPassFamilies[PASS_FAMILIES] = {
  {"ASCHED_EVR_TIMES", 3, PASS_PAIRS}, {"ASCHED_JP_TIMES", 4, PASS_SEQ}, {"ASCHED_JA_TIMES", 3, PASS_SEQ}, {"ASCHED_JA_TIMES", 2, PASS_REV}, {"ASCHED_CA_TIMES", 2, PASS_REV},
  {"ASCHED_SC_TIMES", 3, PASS_SEQ}, {"ASCHED_JD_TIMES", 5, PASS_SEQ}, {"ASCHED_NP_TIMES", 2, PASS_SEQ}, {"ASCHED_ND_TIMES", 7, PASS_SEQ}, {"ASCHED_NA_TIMES", 4, PASS_SEQ},
  {"ASCHED_QL_TIMES", 3, PASS_SEQ},
};
static void plat_pass_ms(PassFamily f, double* out /*[kPassFamilies[f].passes]*/);
static inline bool plat_pass_printed(PassFamily f) { const char* e = getenv(kPassFamilies[f].env); return e && e[0] == '1'; }
static inline void plat_pass_clear(PassFamily f, double* ms) { for (int k = 0; k < kPassFamilies[f].passes; k++) ms[k] = 0; }   // (a call that runs no pass reports zeros)
#ifdef ASCHED_HOSTSIM
// the CPU build's one definition: no device, every pass time is zero.  It sits here, not in tests/hostsim/hostsim.cpp, so that a CPU build made from an older
// tests/ tree (which has no such definition) still links against this layer
static void plat_pass_ms(PassFamily f, double* out) { plat_pass_clear(f, out); }
#endif
// the run-state patch of the resident job table (kernels_jobs_patch.h): scatter + keys, remove (plat_compact into keptBuf [a.total]), sort, merge by rank into a.out;
// fills a.kept / a.nKept.  Synchronous: the new order is complete on return.  The CPU build's definition sits in kernels_jobs_patch.h.
struct JpArgs;
static int plat_jobs_patch(Dev& d, JpArgs& a, int32_t* keptBuf);
// queue priorities of resident jobs change (kernels_jobs_reprioritise.h): its scatter + keys, then the patch's remove, sort and merge by rank into a.p.out; fills
// a.p.kept / a.p.nKept.  Synchronous: the new order is complete on return; PASS_JP reports its passes.  The CPU build's definition sits in kernels_jobs_reprioritise.h.
struct JrArgs;
static int plat_jobs_reprioritise(Dev& d, JrArgs& a, int32_t* keptBuf);
// a round's result applied to the resident jobs (kernels_round_commit.h): its scatter + keys over the caller's entries and the lists the round left in d.resJob /
// resNode / resPrio / resPreJob, then the patch's remove, sort and merge by rank into a.p.out; fills a.p.kept / a.p.nKept.  Synchronous: the new order is complete on
// return; PASS_JP reports its passes.  The CPU build's definition sits in kernels_round_commit.h.
struct RcArgs;
static int plat_round_commit(Dev& d, RcArgs& a, int32_t* keptBuf);
// retried jobs change class and request in place (kernels_jobs_respec.h): one scatter over the entries — shape, request words, grid flag and JobRec of each named row.
// Synchronous: the rows are complete on return.  The CPU build's definition sits in kernels_jobs_respec.h.
struct JsArgs;
static int plat_jobs_respec(Dev& d, JsArgs& a);
// newly submitted jobs behind the resident job table (kernels_jobs_append.h): row fill + keys, the patch's sort, the patch's merge by rank of the old order (a.p.kept) and the
// sorted new keys into a.p.out.  Synchronous: rows and order are complete on return.  The CPU build's definition sits in kernels_jobs_append.h.
struct JaArgs;
static int plat_jobs_append(Dev& d, JaArgs& a);
// new scheduling-key shapes join the shape mask (kernels_shapes_append.h): the resident rows copied device to device into the fresh block a.outMask, then the new rows,
// one wave per 64-node word.  Synchronous: the fresh block is complete on return; nothing the handle points to is written.  The CPU build's definition sits in
// kernels_shapes_append.h.
struct SaArgs;
static int plat_shapes_append(Dev& d, SaArgs& a);
// new requirement classes join the class mask (kernels_req_classes_append.h): the resident rows copied device to device into the fresh block a.outMask (the derived
// classes' rows dC rows further up), then the new rows and, where a.nodeCls is given, the new bits of every node, one wave per 64-node word.  Synchronous: the fresh
// block is complete on return; of what the handle points to only a.nodeCls is written.  The CPU build's definition sits in kernels_req_classes_append.h.
struct CaArgs;
static int plat_req_classes_append(Dev& d, CaArgs& a);
// dead shapes and classes leave the resident tables (kernels_shapes_compact.h): the remap of a.jShape and the job records in place, the gathers of the mask rows into
// the fresh blocks a.shapeOut / a.clsOut, the bit compaction of a.nodeCls in place.  Synchronous: everything is complete on return.  The CPU build's definition sits
// in kernels_shapes_compact.h.
struct ScArgs;
static int plat_shapes_compact(Dev& d, ScArgs& a);
// rows leave the resident job table (kernels_jobs_delete.h): mark, scan (plat_compact over the keep flags into a.src / a.newId; its count must be a.M1), the gather of the
// static per-job arrays into the blocks of a.out*, the compaction and renumbering of the order (a.ordOut) and of the gang lists (a.gangOut), unmark.  Synchronous: everything
// is complete on return.  The CPU build's definition sits in kernels_jobs_delete.h.
struct JdArgs;
static int plat_jobs_delete(Dev& d, JdArgs& a);
// cordons and capacity changes of resident nodes (kernels_nodes_patch.h): the scatter of the entries, then the touched words of the class, shape and type masks.
// Synchronous: node arrays and masks are complete on return.  The CPU build's definition sits in kernels_nodes_patch.h.
struct NpArgs;
static int plat_nodes_patch(Dev& d, const NpArgs& a);
// rows leave the resident node table (kernels_nodes_delete.h).  plat_nodes_delete_check: mark, then the check of the running jobs; *bad is the lowest job row that runs on
// a named node or ND_NONE, and in the first case the flags are set again: nothing else was written.  plat_nodes_delete: the scan (its count must be a.N1), the gathers
// into the blocks of a.out*, the index order, the mask rows, the remap of the running jobs' nodes, unmark.  Synchronous: everything is complete on return.  The CPU
// build's definitions sit in kernels_nodes_delete.h.
struct NdArgs;
static int plat_nodes_delete_check(Dev& d, NdArgs& a, int32_t* bad);
static int plat_nodes_delete(Dev& d, NdArgs& a);
// new rows join the resident node table (kernels_nodes_append.h): the planes, the narrow arrays, the merge of the index order and the mask rows, all into the fresh
// blocks of a.out*; nothing the handle points to is written.  Synchronous: everything is complete on return.  The CPU build's definition sits in kernels_nodes_append.h.
struct NaArgs;
static int plat_nodes_append(Dev& d, NaArgs& a);
// the queued lists of a round from the resident job order (kernels_queued_lists.h): mark (a flag byte per row of a.flag), hold (the rows of a.held cleared), then
// plat_compact of dev.ordAll[0, ordTotal) by the flags with dev.ordAllOff as segment offsets: list [total], prefix [ordTotal] scratch, off [a.Q + 1], all platform memory.
// *total is on the host on return.  The CPU build's definition sits in kernels_queued_lists.h.
struct QlArgs;
static int plat_queued_lists(Dev& d, const QlArgs& a, int ordTotal, int32_t* list, uint32_t* prefix, int32_t* off, int* total);
static int plat_run_fit_capacity(Dev& d, const std::vector<int32_t>& shapes, std::vector<int32_t>& firstNode, std::vector<long long>& capacity, const int32_t* nodeByRankHost);
static int plat_run_submit_gangs(Dev& d, const std::vector<int32_t>& off, const std::vector<int32_t>& jobs, std::vector<int32_t>& out);
static double plat_last_fit_ms();
static int plat_run_drf(Dev& dev, const std::vector<int64_t>& a, const std::vector<int64_t>& t, double* out);
static int plat_run_fair_shares(Dev& dev, int q, const int32_t* nameRank, const double* weight, const double* cds, double* fair, double* dc, double* uc);

// ---- communicator and sharding.  One communicator per context (RCCL, or the caller's transport); without one plat_allreduce is a no-op that returns 0.
// plat_allreduce reduces `count` int64 words in platform memory in place, ordered with the context's other work; op: 0 SUM, 1 MIN, 2 MAX.
// An implementation without RCCL / exchange areas returns -1 from the calls it cannot serve.
static int plat_comm_unique_id(char* out128);
static int plat_comm_init(const char* id128, int rank, int world);
static int plat_comm_init_external(asched_allreduce_fn fn, void* ctx, int rank, int world);
static void plat_comm_destroy();
static void plat_comm_info(int* rank, int* world);
static bool plat_comm_live();
static int plat_allreduce(long long* dbuf, size_t count, int op);
static long plat_last_shard_exchanges();
static int plat_shard_area(void** ptr, char* ipc64);
static int plat_shard_open(const char* ipc64, void** out);
static int plat_shard_peers(void* const* areas, int world, int rank);

// ---- multi-GPU (mgpu.h, replay_rank.h): the words the collectives reduce are produced and consumed per element; buffers are platform memory.
static int plat_run_fit_batch_global(Dev& d, const std::vector<int32_t>& shapes, const std::vector<int32_t>& slot, int level, GlobalKeyLayout L, const int32_t* globalRank, long long* out, int* badOut);
static int plat_round_delta(Dev& d, int ns, int np, long long* buf);
static int plat_delta_resolve(Dev& d, const long long* red, int ns, int np, int32_t* counts, int32_t* node, int32_t* prio, uint8_t* replay);
static int plat_replay_rank(Dev& d, int n, int keepPending);
