// asched_jobs_respec (asched_host.inc + kernels_jobs_respec.h + the steps shared with asched_jobs_append) of the CPU build of the device code, as a stand-alone program
// for AddressSanitizer + UndefinedBehaviorSanitizer: the edge list of tests/test_z_jobs_respec.py on ONE handle, one call after the other — batch sizes, table ends,
// class-only / request-only, no-ops, resident / new / revived targets, an old shape that loses its first and its last row, an exchange, requests off the grid and
// requests no node holds, with the in-place switch on and off — each checked against a fresh handle of the edited table (order, first fit of every row, a round), then
// a refusal followed by a round, and a second job table on the same handle.  Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/jobs_respec_sanitize tools/jobs_respec_sanitize.cpp && /tmp/jobs_respec_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4, Q = 4, N = 70;
static const int32_t pcPrio[3] = {0, 1, 3};
static const int64_t Gi = 1ll << 30;

struct Table {
  int M;
  std::vector<int32_t> queue, pc, node, sap, cls; std::vector<uint32_t> qprio; std::vector<int64_t> req, submit, runTs;
  Table(int m, unsigned seed) : M(m), queue(m), pc(m), node(m), sap(m), cls(m, 0), qprio(m, 0), req((size_t)m * R, 0), submit(m), runTs(m) {
    std::mt19937 rng(seed);
    for (int j = 0; j < M; j++) {
      queue[j] = (int)(rng() % Q); pc[j] = (int)(rng() % 3); submit[j] = j; cls[j] = (int)(rng() % 2);
      bool run = j % 5 == 2;   // rows 0 and M - 1 are queued (M % 5 != 3)
      node[j] = run ? (int)(rng() % N) : -1; sap[j] = run ? pcPrio[pc[j]] : 0; runTs[j] = run ? (int64_t)(1 + rng() % 5) * 1000000000ll : 0;
      req[(size_t)j * R] = (1 + rng() % 3) * Gi; req[(size_t)j * R + 1] = 1000 * (1 + rng() % 2); req[(size_t)j * R + 2] = (rng() % 2) * Gi;
    }
    queue[1] = -1;   // a row of no queue
  }
  int set(asched_t* h) const {
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = M; jb.queue = queue.data(); jb.pc = pc.data(); jb.queue_priority = qprio.data(); jb.submit_time = submit.data(); jb.req = req.data(); jb.req_class = cls.data();
    jb.node = node.data(); jb.scheduled_at_priority = sap.data(); jb.run_timestamp = runTs.data();
    static const int32_t zero3[3] = {0, 0, 0};
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = 2; rc.tol_off = zero3; rc.sel_off = zero3;
    return asched_jobs_set(h, &jb, &rc);
  }
  std::vector<int32_t> queuedRows() const { std::vector<int32_t> v; for (int j = 0; j < M; j++) if (node[j] < 0) v.push_back(j); return v; }
};

static asched_t* create() {
  static const int32_t indexedCol[2] = {1, 0};
  static const int64_t indexedRes[2] = {1000, 128ll << 20};
  static const uint8_t pcPre[3] = {1, 1, 0};
  static const double drf[4] = {1.0, 1.0, 0.0, 1.0};
  asched_config c; memset(&c, 0, sizeof c);
  c.num_resources = R; c.num_indexed = 2; c.indexed_col = indexedCol; c.indexed_resolution = indexedRes;
  c.num_priority_classes = 3; c.pc_priority = pcPrio; c.pc_preemptible = pcPre; c.drf_multiplier = drf; c.device = -1;
  asched_t* h = asched_create(&c);
  if (!h) return nullptr;
  static std::vector<uint64_t> index(N); static std::vector<int32_t> rank(N); static std::vector<int64_t> total((size_t)N * R, 0);
  for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * R] = (i % 2 ? 16 : 8) * Gi; total[(size_t)i * R + 1] = 8000; total[(size_t)i * R + 2] = 4 * Gi; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data();
  if (asched_nodes_upsert(h, &nd)) { asched_destroy(h); return nullptr; }
  return h;
}

struct Answers { std::vector<std::vector<int32_t>> order; std::vector<int32_t> fit; int scheduled = -1, preempted = -1; };

// order and first fit of every row; with `round` also a round (which binds the handle's jobs: the next resident call resets it)
static Answers answers(asched_t* h, const Table& t, bool round) {
  Answers a;
  std::vector<int32_t> got(t.M + 1), rows(t.M);
  for (int q = 0; q < Q; q++) { int n = asched_scheduling_order(h, q, got.data(), t.M); CHECK(n >= 0); a.order.emplace_back(got.begin(), got.begin() + std::max(n, 0)); }
  for (int j = 0; j < t.M; j++) rows[j] = j;
  a.fit.assign(t.M, -7);
  CHECK(asched_fit_select_batch(h, t.M, rows.data(), -2, a.fit.data()) == 0);
  if (round) {
    std::vector<double> weight(Q, 1.0), qTok(Q, 1e18); std::vector<int64_t> qBurst(Q, 1ll << 62); std::vector<uint8_t> qInf(Q, 1); std::vector<int32_t> qOff(Q + 1, 0), queued;
    for (int q = 0; q < Q; q++) { for (int j : a.order[q]) if (t.node[j] < 0) queued.push_back(j); qOff[q + 1] = (int32_t)queued.size(); }
    if (queued.empty()) queued.push_back(0);
    asched_queues qs; memset(&qs, 0, sizeof qs);
    qs.q = Q; qs.weight = weight.data(); qs.global_tokens = 1e18; qs.global_burst = 1ll << 62; qs.global_rate_inf = 1; qs.queue_tokens = qTok.data(); qs.queue_burst = qBurst.data();
    qs.queue_rate_inf = qInf.data(); qs.queued_off = qOff.data(); qs.queued_jobs = queued.data();
    CHECK(asched_round_prepare(h, &qs) == 0);
    asched_round_result res;
    int rc = asched_schedule_round(h, &res);
    CHECK(rc == 0);
    if (rc) fprintf(stderr, "round: %s\n", asched_last_error(h));
    else { a.scheduled = res.num_scheduled; a.preempted = res.num_preempted; }
  }
  return a;
}

static void sameAsFresh(asched_t* h, const Table& t, const char* what, bool round = true) {
  asched_t* f = create();
  CHECK(f != nullptr);
  if (!f) return;
  CHECK(t.set(f) == 0);
  Answers a = answers(h, t, round), b = answers(f, t, round);
  CHECK(a.order == b.order); CHECK(a.fit == b.fit);
  for (int j = 0; j < t.M; j++) if (a.fit[j] != b.fit[j]) { fprintf(stderr, "%s: row %d fits node %d, on the fresh handle %d\n", what, j, a.fit[j], b.fit[j]); break; }
  CHECK(a.scheduled == b.scheduled); CHECK(a.preempted == b.preempted);
  asched_destroy(f);
  printf("%-64s ok (%d scheduled)\n", what, a.scheduled);
}

// the call, the model edited with it, the statistics
static void respec(asched_t* h, Table& t, const std::vector<int32_t>& rows, const std::vector<int32_t>* cls, const std::vector<int64_t>* req, int32_t* st) {
  int rc = asched_jobs_respec(h, (int)rows.size(), rows.data(), cls ? cls->data() : nullptr, req ? req->data() : nullptr);
  CHECK(rc == 0);
  if (rc) fprintf(stderr, "jobs_respec(%d): %s\n", (int)rows.size(), asched_last_error(h));
  for (size_t i = 0; i < rows.size(); i++) {
    if (cls) t.cls[rows[i]] = (*cls)[i];
    if (req) for (int r = 0; r < R; r++) t.req[(size_t)rows[i] * R + r] = (*req)[i * R + r];
  }
  CHECK(asched_jobs_respec_stats(h, st) == 0);
  CHECK(st[0] == (int)rows.size());
}

static std::vector<int64_t> reqs(int n, int64_t mem0, int kinds) {
  std::vector<int64_t> v((size_t)n * R, 0);
  for (int i = 0; i < n; i++) { v[(size_t)i * R] = 2 * Gi; v[(size_t)i * R + 1] = 1000; v[(size_t)i * R + 2] = (mem0 + i % kinds) * (Gi >> 4); }
  return v;
}

int main() {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  asched_t* h = create();
  CHECK(h != nullptr);
  if (!h) return 1;
  int32_t st[8], one = 0;
  { std::vector<int64_t> r1 = reqs(1, 1, 1);
    CHECK(asched_jobs_respec(h, 1, &one, nullptr, r1.data()) == ASCHED_ERR_INVALID); }   // no job table
  for (int table = 0; table < 2; table++) {   // the second table: what the first left on the handle is gone with it
    Table t(table ? 401 : 700, 21 + table);
    CHECK(t.set(h) == 0);
    CHECK(asched_jobs_respec_stats(h, st) == 0 && st[0] == 0 && st[2] == 0 && st[5] == 0);
    for (int on = 1; on >= 0; on--) {
      CHECK(asched_set_append_in_place(h, on) == 0);
      std::vector<int32_t> free = t.queuedRows();
      // batch sizes, onto five new shapes a batch
      static const int sizes[] = {0, 1, 63, 64, 65, 257};
      int64_t mem = 100 + 1000 * table + 500 * (1 - on);
      for (int n : sizes) {
        std::vector<int32_t> rows(free.begin() + 7, free.begin() + 7 + n);
        std::vector<int64_t> rq = reqs(n, mem, 5); mem += 5;
        respec(h, t, rows, nullptr, &rq, st);
        CHECK(st[1] == 0 && st[5] == (n > 0 && !on ? 1 : 0) && st[6] == 0);
        if (on && n > 0) CHECK(st[2] >= 1 && st[7] >= 1);
        char what[96]; snprintf(what, sizeof what, "table %d switch %d: %d rows onto new shapes", table, on, n);
        sameAsFresh(h, t, what, n == 0 || n == 65 || n == 257);
      }
      // rows 0 and M - 1, class only; then a batch of no-ops and mixed no-ops
      { std::vector<int32_t> rows{t.M - 1, 0}, cls{1 - t.cls[t.M - 1], 1 - t.cls[0]};
        respec(h, t, rows, &cls, nullptr, st);
        sameAsFresh(h, t, "rows M - 1 and 0, class only");
        respec(h, t, rows, &cls, nullptr, st);
        CHECK(st[1] == 2 && st[2] == 0 && st[5] == 0 && st[7] == 0);
        std::vector<int32_t> rows3{t.M - 1, free[3], 0}, cls3{t.cls[t.M - 1], 1 - t.cls[free[3]], t.cls[0]};
        respec(h, t, rows3, &cls3, nullptr, st);
        CHECK(st[1] == 2);
        sameAsFresh(h, t, "no-op entries, alone and mixed in"); }
      // the row of no queue; a request off the grid and back; a request no node holds
      { std::vector<int32_t> rows{1, free[4], free[5]};
        std::vector<int64_t> rq{3 * Gi, 1000, 0, 0, 2 * Gi, 1250, Gi, 0, 64 * Gi, 1000, 0, 0}, back{Gi, 1000, 0, 0, Gi, 1000, 0, 0, Gi, 1000, 0, 0};
        respec(h, t, rows, nullptr, &rq, st);
        sameAsFresh(h, t, "no queue / off the grid / no node holds it");
        respec(h, t, rows, nullptr, &back, st);
        sameAsFresh(h, t, "and back onto the grid"); }
      // an old shape loses its first row, then its last; the shape is revived; two rows exchange (class, request)
      { const int a = free[0];
        std::vector<int32_t> same;
        for (int j : free) if (t.cls[j] == t.cls[a] && t.pc[j] == t.pc[a] && !memcmp(&t.req[(size_t)j * R], &t.req[(size_t)a * R], sizeof(int64_t) * R)) same.push_back(j);
        std::vector<int64_t> old(t.req.begin() + (size_t)a * R, t.req.begin() + (size_t)a * R + R), rq = reqs(1, 9000 + table, 1);
        const int32_t oldCls = t.cls[a];
        bool others = false;
        for (int j = 0; j < t.M; j++) if (t.node[j] >= 0 && t.cls[j] == oldCls && t.pc[j] == t.pc[a] && !memcmp(&t.req[(size_t)j * R], old.data(), sizeof(int64_t) * R)) others = true;
        respec(h, t, {a}, nullptr, &rq, st);
        sameAsFresh(h, t, "an old shape loses its first row");
        std::vector<int32_t> rest(same.begin() + 1, same.end());
        if (!rest.empty()) {
          std::vector<int64_t> rqn; for (size_t i = 0; i < rest.size(); i++) rqn.insert(rqn.end(), rq.begin(), rq.end());
          respec(h, t, rest, nullptr, &rqn, st);
          CHECK(others || st[4] == 1);
          sameAsFresh(h, t, "an old shape loses its last row");
        }
        std::vector<int32_t> c1{oldCls};
        respec(h, t, {a}, &c1, &old, st);
        CHECK(others || st[3] == 1);
        sameAsFresh(h, t, "the emptied shape is revived");
        int b = -1;
        for (int j : free) if (t.pc[j] == t.pc[a] && (t.cls[j] != t.cls[a] || memcmp(&t.req[(size_t)j * R], &t.req[(size_t)a * R], sizeof(int64_t) * R))) { b = j; break; }
        if (b >= 0) {
          std::vector<int32_t> rows{a, b}, cls{t.cls[b], t.cls[a]};
          std::vector<int64_t> x(t.req.begin() + (size_t)b * R, t.req.begin() + (size_t)b * R + R);
          x.insert(x.end(), t.req.begin() + (size_t)a * R, t.req.begin() + (size_t)a * R + R);
          respec(h, t, rows, &cls, &x, st);
          sameAsFresh(h, t, "two rows exchange class and request");
        } }
      // refusals: the handle stays as it was, and a round follows
      { std::vector<int32_t> free2 = t.queuedRows();
        int32_t twice[2] = {free2[0], free2[0]}, badRow[1] = {t.M}, negRow[1] = {-1}, running[1] = {2}, badCls[1] = {2}, okRow[1] = {free2[0]};
        std::vector<int64_t> rq = reqs(2, 7, 1);
        int32_t before[8], after[8];
        CHECK(asched_jobs_respec_stats(h, before) == 0);
        CHECK(asched_jobs_respec(h, 2, twice, nullptr, rq.data()) == ASCHED_ERR_INVALID);
        CHECK(asched_jobs_respec(h, 1, badRow, nullptr, rq.data()) == ASCHED_ERR_INVALID);
        CHECK(asched_jobs_respec(h, 1, negRow, nullptr, rq.data()) == ASCHED_ERR_INVALID);
        CHECK(t.node[2] >= 0 && asched_jobs_respec(h, 1, running, nullptr, rq.data()) == ASCHED_ERR_INVALID);
        CHECK(asched_jobs_respec(h, 1, okRow, badCls, nullptr) == ASCHED_ERR_INVALID);
        CHECK(asched_jobs_respec(h, -1, okRow, nullptr, rq.data()) == ASCHED_ERR_INVALID);
        CHECK(asched_jobs_respec(h, 1, nullptr, nullptr, rq.data()) == ASCHED_ERR_INVALID);
        CHECK(asched_jobs_respec(h, 1, okRow, nullptr, nullptr) == ASCHED_ERR_INVALID);
        CHECK(asched_jobs_respec_stats(h, after) == 0 && !memcmp(before, after, sizeof before));
        CHECK(asched_jobs_respec(h, 0, nullptr, nullptr, nullptr) == 0);   // (the refusals left what the last round left: n == 0 performs the resets only)
        CHECK(asched_jobs_respec_stats(h, after) == 0 && after[0] == 0 && after[5] == 0);
        sameAsFresh(h, t, "refusals, the resets of n == 0, then a round"); }
      // a run-state patch gives a respec'd row a run, an append brings a shape the respecs left without a row, then another respec
      { std::vector<int32_t> free2 = t.queuedRows();
        int32_t prow[1] = {free2[9]}, pnode[1] = {1}, psap[1] = {pcPrio[t.pc[free2[9]]]}; int64_t pts[1] = {7000000000ll};
        CHECK(asched_jobs_patch(h, 1, prow, pnode, psap, pts) == 0);
        t.node[free2[9]] = 1; t.sap[free2[9]] = psap[0]; t.runTs[free2[9]] = pts[0];
        std::vector<int64_t> rq = reqs(3, 12000 + table * 10 + on, 3);
        respec(h, t, {free2[10], free2[11], free2[12]}, nullptr, &rq, st);
        sameAsFresh(h, t, "after a jobs_patch"); }
    }
  }
  asched_destroy(h);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("jobs_respec under ASan + UBSan: all calls ok\n");
  return 0;
}
