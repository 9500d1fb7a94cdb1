// asched_round_commit (asched_host.inc + kernels_round_commit.h + the passes of kernels_jobs_patch.h) of the CPU build of the device code, as a stand-alone program for
// AddressSanitizer + UndefinedBehaviorSanitizer: on one handle, one cycle after the other — a round, then the commit of its result with as many extras (runs that end,
// rows named with no run) as bring the total entry count to the sizes of tests/test_z_round_commit.py (a): 1, 2, 1023, 1024, 1025, 2049 — each checked against a
// restatement of SchedulingOrderCompare written here (std::sort over the edited table); then a commit with a step, the refusals, and a second job table on the same
// handle.  The rate limiter's burst sets how many jobs a round schedules.  Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/round_commit_sanitize tools/round_commit_sanitize.cpp && /tmp/round_commit_sanitize
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
      bool run = rng() % 4 == 0;
      node[j] = run ? (int)(rng() % N) : -1; sap[j] = run ? pcPrio[pc[j]] : 0; runTs[j] = run ? (int64_t)(1 + rng() % 5) * 1000000000ll : 0;
      req[(size_t)j * R] = 1ll << 30; req[(size_t)j * R + 1] = 1000;
    }
    if (M > 3) { queue[3] = -1; node[3] = -1; sap[3] = 0; runTs[3] = 0; away[2] = node[2] >= 0; }   // a row of no queue; a cross-pool away row when it runs
  }
  bool less(int a, int b) const {   // jobdb/comparison.go:49-107
    bool ra = node[a] >= 0, rb = node[b] >= 0;
    if (ra != rb) return ra;
    if (pcPrio[pc[a]] != pcPrio[pc[b]]) return pcPrio[pc[a]] > pcPrio[pc[b]];
    if (qprio[a] != qprio[b]) return qprio[a] < qprio[b];
    if (ra && runTs[a] != runTs[b]) return runTs[a] < runTs[b];
    if (submit[a] != submit[b]) return submit[a] < submit[b];
    return a < b;
  }
  std::vector<int32_t> order(int q) const {
    std::vector<int32_t> ids;
    for (int j = 0; j < M; j++) if (queue[j] == q) ids.push_back(j);
    std::sort(ids.begin(), ids.end(), [&](int a, int b) { return less(a, b); });
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

// a round over the queued rows of the table (held: rows without a run that are in a terminal state), at most `burst` jobs scheduled
static int round(asched_t* h, const Table& t, const std::vector<uint8_t>& held, int burst, asched_round_result* res) {
  std::vector<double> weight(Q, 1.0), qTok(Q, (double)burst); std::vector<int64_t> qBurst(Q, burst); std::vector<uint8_t> qInf(Q, 0); std::vector<int32_t> qOff(Q + 1, 0), queued;
  for (int q = 0; q < Q; q++) { for (int j : t.order(q)) if (t.node[j] < 0 && !held[j]) queued.push_back(j); qOff[q + 1] = (int32_t)queued.size(); }
  if (queued.empty()) queued.push_back(0);
  asched_queues qs; memset(&qs, 0, sizeof qs);
  qs.q = Q; qs.weight = weight.data(); qs.global_tokens = (double)burst; qs.global_burst = burst; qs.global_rate_inf = 0; qs.queue_tokens = qTok.data(); qs.queue_burst = qBurst.data();
  qs.queue_rate_inf = qInf.data(); qs.queued_off = qOff.data(); qs.queued_jobs = queued.data();
  int rc = asched_round_prepare(h, &qs);
  if (rc == 0) rc = asched_schedule_round(h, res);
  if (rc) fprintf(stderr, "round: %s\n", asched_last_error(h));
  return rc;
}

// one cycle: a round of at most `burst` placements, then its commit with the extras that bring the entry count to `n` (n < 0: no extras)
static void cycle(asched_t* h, Table& t, std::vector<uint8_t>& held, int burst, int n, int64_t ts0, int64_t step, std::mt19937& rng, bool first) {
  asched_round_result res;
  CHECK(round(h, t, held, burst, &res) == 0);
  const int ns = res.num_scheduled, np = res.num_preempted;
  std::vector<uint8_t> named(t.M, 0);
  int inOrder = 0;
  for (int i = 0; i < ns; i++) { int j = res.scheduled_job[i]; named[j] = 1; inOrder += t.queue[j] >= 0; t.node[j] = res.scheduled_node[i]; t.sap[j] = res.scheduled_priority[i]; t.runTs[j] = ts0 + i * step; }
  for (int i = 0; i < np; i++) { int j = res.preempted_job[i]; named[j] = 1; inOrder += t.queue[j] >= 0; t.node[j] = -1; t.sap[j] = 0; t.runTs[j] = 0; held[j] = 1; }
  // the extras: runs that end first, then rows without a run (named with node -1: they stay where they are), in a shuffled order
  int nx = n < 0 ? 0 : n - ns - np;
  CHECK(nx >= 0);
  if (nx < 0) nx = 0;
  std::vector<int32_t> cand, rest;
  for (int j = 0; j < t.M; j++) if (!named[j]) (t.node[j] >= 0 && !t.away[j] ? cand : rest).push_back(j);
  std::shuffle(cand.begin(), cand.end(), rng);
  std::shuffle(rest.begin(), rest.end(), rng);
  if ((int)cand.size() > nx / 2) cand.resize(nx / 2);
  cand.insert(cand.end(), rest.begin(), rest.begin() + std::min<size_t>(rest.size(), (size_t)nx - cand.size()));
  CHECK((int)cand.size() == nx);
  nx = (int)cand.size();
  std::vector<int32_t> xnode(nx, -1);
  for (int j : cand) { inOrder += t.queue[j] >= 0; if (t.node[j] >= 0) held[j] = 1; t.node[j] = -1; t.sap[j] = 0; t.runTs[j] = 0; }
  int rc = asched_round_commit(h, ts0, step, nx, cand.data(), xnode.data(), nullptr, nullptr);
  CHECK(rc == 0);
  if (rc) fprintf(stderr, "round_commit(%d + %d + %d): %s\n", ns, np, nx, asched_last_error(h));
  int32_t st[8];
  CHECK(asched_round_commit_stats(h, st) == 0);
  CHECK(st[0] == ns && st[1] == np && st[2] == nx && st[3] == inOrder && st[4] == (first && ns + np + nx > 0 ? 1 : 0));
  checkOrder(h, t);
  CHECK(asched_round_commit(h, ts0, step, 0, nullptr, nullptr, nullptr, nullptr) == ASCHED_ERR_INVALID);   // the result went with the commit
  printf("  commit of %4d entries (%d scheduled, %d preempted, %d extras), step %lld: ok\n", ns + np + nx, ns, np, nx, (long long)step);
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
  CHECK(asched_round_commit(h, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == ASCHED_ERR_INVALID);   // no job table
  std::vector<uint64_t> index(N); std::vector<int32_t> rank(N); std::vector<int64_t> total((size_t)N * R, 0);
  for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * R] = 1ll << 46; total[(size_t)i * R + 1] = 64000000; total[(size_t)i * R + 2] = 1ll << 46; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data();
  CHECK(asched_nodes_upsert(h, &nd) == 0);
  std::mt19937 rng(7);
  for (int table = 0; table < 2; table++) {   // the second table: the buffers of the first are gone with it
    Table t(table ? 2777 : 6011, 11 + table);
    std::vector<uint8_t> held(t.M, 0);
    CHECK(t.set(h) == 0);
    checkOrder(h, t);
    CHECK(asched_round_commit(h, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == ASCHED_ERR_INVALID);   // no round result
    printf("table %d (%d rows)\n", table, t.M);
    // the lease times straddle the resident runs' (1 .. 5 s)
    cycle(h, t, held, 1, 1, 3000000000ll, 0, rng, true);
    cycle(h, t, held, 1, 2, 3000000001ll, 1, rng, false);
    cycle(h, t, held, 300, 1023, 2500000000ll, 0, rng, false);
    cycle(h, t, held, 300, 1024, 3500000000ll, 1, rng, false);
    cycle(h, t, held, 300, 1025, 1500000000ll, 7, rng, false);
    if (table == 0) cycle(h, t, held, 500, 2049, 4500000000ll, 1, rng, false);
    cycle(h, t, held, 200, -1, 2000000000ll, 1000, rng, false);   // the result alone
    // refusals on a handle that holds a result: the handle stays as it was, and the commit that follows is the result's
    asched_round_result res;
    CHECK(round(h, t, held, 50, &res) == 0);
    CHECK(res.num_scheduled > 0);
    if (res.num_scheduled > 0) {
      int32_t dup[2] = {3, 3}, bad[1] = {t.M}, neg[1] = {-1}, sched[1] = {res.scheduled_job[0]}, none[2] = {-1, -1}, far[1] = {N}, row3[1] = {3};
      CHECK(asched_round_commit(h, 1, 0, 2, dup, none, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, 1, bad, none, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, 1, neg, none, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, 1, sched, none, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, 1, row3, far, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, -1, row3, none, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, 1, nullptr, none, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, 1, row3, nullptr, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_round_commit(h, 1, 0, (1 << 29) + 1, row3, none, nullptr, nullptr) == ASCHED_ERR_UNSUPPORTED);
      checkOrder(h, t);
      for (int i = 0; i < res.num_scheduled; i++) { int j = res.scheduled_job[i]; t.node[j] = res.scheduled_node[i]; t.sap[j] = res.scheduled_priority[i]; t.runTs[j] = 9000000000ll + 2 * i; }
      for (int i = 0; i < res.num_preempted; i++) { int j = res.preempted_job[i]; t.node[j] = -1; t.sap[j] = 0; t.runTs[j] = 0; held[j] = 1; }
      CHECK(asched_round_commit(h, 9000000000ll, 2, 0, nullptr, nullptr, nullptr, nullptr) == 0);
      checkOrder(h, t);
    }
    // a run-state patch and a reprioritise behind a commit: the three share the resident inputs, the scratch and the passes
    { int32_t prow[3] = {0, 1, 5}, pnode[3] = {-1, -1, -1}; uint32_t qp[3] = {7, 0, 2};
      CHECK(asched_jobs_patch(h, 3, prow, pnode, nullptr, nullptr) == 0);
      for (int j : prow) { t.node[j] = -1; t.sap[j] = 0; t.runTs[j] = 0; held[j] = 1; }
      CHECK(asched_jobs_reprioritise(h, 3, prow, qp) == 0);
      for (int k = 0; k < 3; k++) t.qprio[prow[k]] = qp[k];
      checkOrder(h, t);
      cycle(h, t, held, 100, -1, 9500000000ll, 1, rng, false); }
  }
  asched_destroy(h);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("round_commit under ASan + UBSan: all calls ok\n");
  return 0;
}
