// asched_jobs_reprioritise (asched_host.inc + kernels_jobs_reprioritise.h + the passes of kernels_jobs_patch.h) of the CPU build of the device code, as a stand-alone
// program for AddressSanitizer + UndefinedBehaviorSanitizer: calls of the sizes of tests/test_z_jobs_reprioritise.py (a) on one handle, one after the other, each checked
// against a restatement of SchedulingOrderCompare written here (std::sort over the edited table), then a round on the handle, the refusals, and a second job table on
// the same handle.  Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/jobs_reprioritise_sanitize tools/jobs_reprioritise_sanitize.cpp && /tmp/jobs_reprioritise_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4, Q = 5, N = 40;
static const int32_t pcPrio[3] = {0, 1, 3};

struct Table {
  int M;
  std::vector<int32_t> queue, pc, node, sap, cls; std::vector<uint32_t> qprio; std::vector<int64_t> req, submit, runTs; std::vector<uint8_t> away;
  Table(int m, unsigned seed) : M(m), queue(m), pc(m), node(m), sap(m), cls(m, 0), qprio(m), req((size_t)m * R, 0), submit(m), runTs(m), away(m, 0) {
    std::mt19937 rng(seed);
    for (int j = 0; j < M; j++) {
      static const int qs[4] = {0, 1, 2, 4};   // queue 3 is empty
      queue[j] = qs[rng() % 4]; pc[j] = (int)(rng() % 3); qprio[j] = rng() % 3; submit[j] = rng() % 40;
      bool run = rng() % 2;
      node[j] = run ? (int)(rng() % N) : -1; sap[j] = run ? pcPrio[pc[j]] : 0; runTs[j] = run ? (int64_t)(1 + rng() % 5) * 1000000000ll : 0;
      req[(size_t)j * R] = 1ll << 30; req[(size_t)j * R + 1] = 1000;
    }
    if (M > 3) { queue[3] = -1; away[2] = node[2] >= 0; }   // a row of no queue; a cross-pool away row when it runs
  }
  std::vector<int32_t> order(int q) const {   // jobdb/comparison.go:49-107
    std::vector<int32_t> ids;
    for (int j = 0; j < M; j++) if (queue[j] == q) ids.push_back(j);
    std::sort(ids.begin(), ids.end(), [&](int a, int b) {
      bool ra = node[a] >= 0, rb = node[b] >= 0;
      if (ra != rb) return ra;
      if (pcPrio[pc[a]] != pcPrio[pc[b]]) return pcPrio[pc[a]] > pcPrio[pc[b]];
      if (qprio[a] != qprio[b]) return qprio[a] < qprio[b];
      if (ra && runTs[a] != runTs[b]) return runTs[a] < runTs[b];
      if (submit[a] != submit[b]) return submit[a] < submit[b];
      return a < b;
    });
    return ids;
  }
  int set(asched_t* h) const {
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = M; jb.queue = queue.data(); jb.pc = pc.data(); jb.queue_priority = qprio.data(); jb.submit_time = submit.data(); jb.req = req.data(); jb.req_class = cls.data();
    jb.node = node.data(); jb.scheduled_at_priority = sap.data(); jb.run_timestamp = runTs.data(); jb.away = away.data();
    static const int32_t zero2[2] = {0, 0};
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = 1; rc.tol_off = zero2; rc.sel_off = zero2;
    return asched_jobs_set(h, &jb, &rc);
  }
};

static void checkOrder(asched_t* h, const Table& t) {
  std::vector<int32_t> got(t.M + 1);
  for (int q = 0; q < Q; q++) {
    std::vector<int32_t> want = t.order(q);
    int n = asched_scheduling_order(h, q, got.data(), t.M);
    CHECK(n == (int)want.size());
    if (n == (int)want.size()) CHECK(std::equal(want.begin(), want.end(), got.begin()));
  }
}

// n random rows to random priorities; now and then one of the two ends of the value range
static void reprioritise(asched_t* h, Table& t, int n, std::mt19937& rng, bool first) {
  std::vector<int32_t> rows(t.M);
  for (int j = 0; j < t.M; j++) rows[j] = j;
  std::shuffle(rows.begin(), rows.end(), rng);
  rows.resize(n);
  std::vector<uint32_t> qp(n);
  int same = 0, inOrder = 0;
  for (int i = 0; i < n; i++) {
    unsigned x = rng() % 16;
    qp[i] = x == 0 ? 0xFFFFFFFFu : x == 1 ? 0u : rng() % 4;
    same += qp[i] == t.qprio[rows[i]]; inOrder += t.queue[rows[i]] >= 0;
    t.qprio[rows[i]] = qp[i];
  }
  int rc = asched_jobs_reprioritise(h, n, rows.data(), qp.data());
  CHECK(rc == 0);
  if (rc) fprintf(stderr, "jobs_reprioritise(%d): %s\n", n, asched_last_error(h));
  int32_t st[8];
  CHECK(asched_jobs_reprioritise_stats(h, st) == 0);
  CHECK(st[0] == n && st[1] == inOrder && st[2] == same && st[3] == (first && n > 0 ? 1 : 0));
  checkOrder(h, t);
}

int main() {
  static const int32_t indexedCol[3] = {1, 0, 3};
  static const int64_t indexedRes[3] = {1000, 128ll << 20, 1};
  static const uint8_t pcPre[3] = {1, 1, 0};
  static const double drf[4] = {1.0, 1.0, 0.0, 1.0};
  asched_config c; memset(&c, 0, sizeof c);
  c.num_resources = R; c.num_indexed = 3; c.indexed_col = indexedCol; c.indexed_resolution = indexedRes;
  c.num_priority_classes = 3; c.pc_priority = pcPrio; c.pc_preemptible = pcPre; c.drf_multiplier = drf; c.device = -1;
  asched_t* h = asched_create(&c);
  CHECK(h != nullptr);
  if (!h) return 1;
  int32_t one = 0; uint32_t prio1 = 1;
  CHECK(asched_jobs_reprioritise(h, 1, &one, &prio1) == ASCHED_ERR_INVALID);   // no job table
  std::vector<uint64_t> index(N); std::vector<int32_t> rank(N); std::vector<int64_t> total((size_t)N * R, 0);
  for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * R] = 1ll << 46; total[(size_t)i * R + 1] = 64000000; total[(size_t)i * R + 2] = 1ll << 46; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data();
  CHECK(asched_nodes_upsert(h, &nd) == 0);
  std::mt19937 rng(7);
  for (int table = 0; table < 2; table++) {   // the second table: the buffers of the first are gone with it
    Table t(table ? 777 : 3011, 11 + table);
    CHECK(t.set(h) == 0);
    checkOrder(h, t);
    static const int sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025};
    bool first = true;
    for (int n : sizes) if (n <= t.M) { reprioritise(h, t, n, rng, first); first = first && n == 0; printf("table %d: reprioritise of %4d rows ok\n", table, n); }
    reprioritise(h, t, t.M, rng, false);
    printf("table %d: reprioritise of every row ok\n", table);
    // refusals: the handle stays as it was
    int32_t rows2[2] = {5, 5}, badRow[1] = {t.M}, negRow[1] = {-1}; uint32_t prios2[2] = {0, 1};
    CHECK(asched_jobs_reprioritise(h, 2, rows2, prios2) == ASCHED_ERR_INVALID);
    CHECK(asched_jobs_reprioritise(h, 1, badRow, prios2) == ASCHED_ERR_INVALID);
    CHECK(asched_jobs_reprioritise(h, 1, negRow, prios2) == ASCHED_ERR_INVALID);
    CHECK(asched_jobs_reprioritise(h, -1, rows2, prios2) == ASCHED_ERR_INVALID);
    CHECK(asched_jobs_reprioritise(h, 1, nullptr, prios2) == ASCHED_ERR_INVALID);
    CHECK(asched_jobs_reprioritise(h, 1, rows2, nullptr) == ASCHED_ERR_INVALID);
    checkOrder(h, t);
    // a round on the handle
    std::vector<double> weight(Q, 1.0), qTok(Q, 1e18); std::vector<int64_t> qBurst(Q, 1ll << 62); std::vector<uint8_t> qInf(Q, 1); std::vector<int32_t> qOff(Q + 1, 0), queued;
    for (int q = 0; q < Q; q++) { for (int j : t.order(q)) if (t.node[j] < 0) queued.push_back(j); qOff[q + 1] = (int32_t)queued.size(); }
    if (queued.empty()) queued.push_back(0);
    asched_queues qs; memset(&qs, 0, sizeof qs);
    qs.q = Q; qs.weight = weight.data(); qs.global_tokens = 1e18; qs.global_burst = 1ll << 62; qs.global_rate_inf = 1; qs.queue_tokens = qTok.data(); qs.queue_burst = qBurst.data();
    qs.queue_rate_inf = qInf.data(); qs.queued_off = qOff.data(); qs.queued_jobs = queued.data();
    CHECK(asched_round_prepare(h, &qs) == 0);
    asched_round_result res;
    int rc = asched_schedule_round(h, &res);
    CHECK(rc == 0);
    if (rc) fprintf(stderr, "round: %s\n", asched_last_error(h));
    else printf("table %d: round on the reprioritised handle: %d scheduled, %d preempted\n", table, res.num_scheduled, res.num_preempted);
    reprioritise(h, t, 100, rng, false);   // and a call after a round
    // a run-state patch between two calls: the two share the resident inputs, the scratch and the passes
    { int32_t prow[3] = {0, 1, 2}, pnode[3] = {-1, -1, -1};
      CHECK(asched_jobs_patch(h, 3, prow, pnode, nullptr, nullptr) == 0);
      for (int j = 0; j < 3; j++) { t.node[j] = -1; t.sap[j] = 0; t.runTs[j] = 0; }
      reprioritise(h, t, 300, rng, false); }
  }
  asched_destroy(h);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("jobs_reprioritise under ASan + UBSan: all calls ok\n");
  return 0;
}
