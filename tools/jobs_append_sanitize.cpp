// asched_jobs_append (asched_host.inc + kernels_jobs_append.h) of the CPU build of the device code, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: appends of the sizes of tests/test_z_jobs_append.py (a) each on a fresh table, six growing appends on one handle, an append with a new shape
// and a new gang, an append after a patch, a round on the grown handle, the refusals, a second job table on the same handle, an append that re-allocates and brings new
// shapes at once, and on a pool of LIT_TMAX + 1 node types a refusal that comes after the shape lookup (everything is put back) — every order checked against a
// restatement of SchedulingOrderCompare written here (std::sort over the concatenated table).  In the CPU build the "device" arrays are heap blocks: a per-job array that
// an append did not grow shows up here as a heap overflow.  Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/jobs_append_sanitize tools/jobs_append_sanitize.cpp && /tmp/jobs_append_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4, Q = 8, N = 40;
static const int32_t pcPrio[3] = {0, 1, 3};

struct Table {
  int M = 0;
  std::vector<int32_t> queue, pc, node, sap, cls, gang, card; std::vector<uint32_t> qprio; std::vector<int64_t> req, submit, runTs;
  void add(std::mt19937& rng, int m, bool running, int shapes, int gangBase) {   // m more rows; shapes: distinct request vectors drawn from; gangBase >= 0: the rows form gangs of 4
    static const int qs[4] = {0, 1, 2, 4};   // queue 3 is empty
    for (int i = 0; i < m; i++) {
      bool run = running && rng() % 2;
      int q = qs[rng() % 4];
      if (gangBase >= 0) q = 1;
      queue.push_back(q); pc.push_back((int)(rng() % 3)); qprio.push_back(rng() % 3); submit.push_back(rng() % 40);
      node.push_back(run ? (int)(rng() % N) : -1); sap.push_back(run ? pcPrio[pc.back()] : 0); runTs.push_back(run ? (int64_t)(1 + rng() % 5) * 1000000000ll : 0);
      cls.push_back(0); gang.push_back(gangBase >= 0 ? gangBase + i / 4 : -1); card.push_back(gangBase >= 0 ? 4 : 1);
      int s = (int)(rng() % shapes);
      req.push_back((1ll << 30) * (1 + s % 3)); req.push_back(1000 * (1 + s / 3)); req.push_back(0); req.push_back(0);
      if (gangBase >= 0 && i % 4) { pc.back() = pc[pc.size() - 2]; for (int r = 0; r < R; r++) req[req.size() - R + r] = req[req.size() - 2 * R + r]; }
    }
    M += m;
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
  asched_jobs view(int from, int m) const {
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = m; jb.queue = queue.data() + from; jb.pc = pc.data() + from; jb.queue_priority = qprio.data() + from; jb.submit_time = submit.data() + from;
    jb.req = req.data() + (size_t)from * R; jb.req_class = cls.data() + from; jb.gang_id = gang.data() + from; jb.gang_cardinality = card.data() + from;
    return jb;
  }
  int set(asched_t* h) const {
    asched_jobs jb = view(0, M);
    jb.node = node.data(); jb.scheduled_at_priority = sap.data(); jb.run_timestamp = runTs.data();
    static const int32_t zero2[2] = {0, 0};
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = 1; rc.tol_off = zero2; rc.sel_off = zero2;
    return asched_jobs_set(h, &jb, &rc);
  }
  int append(asched_t* h, int from) const { asched_jobs jb = view(from, M - from); return asched_jobs_append(h, &jb); }
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

static void round(asched_t* h, const Table& t, const char* what) {
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
  else printf("%s: round on the grown handle: %d scheduled, %d preempted\n", what, res.num_scheduled, res.num_preempted);
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
  std::mt19937 rng(7);
  int32_t st[8];
  { Table e; e.add(rng, 1, false, 1, -1); CHECK(e.append(h, 0) == ASCHED_ERR_INVALID); }   // no job table
  std::vector<uint64_t> index(N); std::vector<int32_t> rank(N); std::vector<int64_t> total((size_t)N * R, 0);
  for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * R] = 1ll << 46; total[(size_t)i * R + 1] = 64000000; total[(size_t)i * R + 2] = 1ll << 46; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data();
  CHECK(asched_nodes_upsert(h, &nd) == 0);
  // the batch sizes at which the sort and the merge take another turn, each on a fresh table of the same handle
  static const int sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000};
  for (int m : sizes) {
    Table t; t.add(rng, 3011, true, 1, -1);
    CHECK(t.set(h) == 0);
    t.add(rng, m, false, 1, -1);
    CHECK(t.append(h, 3011) == 0);
    CHECK(asched_jobs_append_stats(h, st) == 0 && st[0] == m && st[2] == 0 && st[5] == 0 && st[6] >= t.M);
    checkOrder(h, t);
    printf("append of %4d rows ok (capacity %d)\n", m, st[6]);
  }
  for (int table = 0; table < 2; table++) {   // the second table: the buffers of the first are gone with it
    Table t; t.add(rng, table ? 777 : 3011, true, 4, -1);
    CHECK(t.set(h) == 0);
    checkOrder(h, t);
    int fits = 0;
    for (int k = 0; k < 6; k++) {   // six growing appends: some re-allocate, some fit
      int before = t.M;
      t.add(rng, 700, false, 4, -1);
      CHECK(t.append(h, before) == 0);
      CHECK(asched_jobs_append_stats(h, st) == 0 && st[0] == 700 && st[5] == 0 && st[6] >= t.M);
      if (st[4]) CHECK(st[6] * 4ll >= before * 5ll); else fits++;
      checkOrder(h, t);
      round(h, t, "growing append");
    }
    if (table == 0) CHECK(fits > 0);   // (777 rows: 700 more outgrow 1.25 x the capacity every time)
    printf("table %d: six growing appends ok, %d fit the capacity\n", table, fits);
    { int before = t.M;   // new shapes and new gangs
      t.add(rng, 40, false, 9, 500 + table);
      t.add(rng, 100, false, 9, -1);
      CHECK(t.append(h, before) == 0);
      CHECK(asched_jobs_append_stats(h, st) == 0 && st[2] > 0 && st[3] == 10 && st[5] == 1);
      checkOrder(h, t);
      round(h, t, "new shapes and gangs"); }
    { // an append after a patch that names old and new rows
      std::vector<int32_t> rows, pnode, psap; std::vector<int64_t> pts;
      for (int j = 0; j < t.M; j += 7) if (t.gang[j] < 0) {
        bool stop = t.node[j] >= 0;
        rows.push_back(j); pnode.push_back(stop ? -1 : j % N); psap.push_back(stop ? 0 : pcPrio[t.pc[j]]); pts.push_back(stop ? 0 : 9000000000ll);
        t.node[j] = pnode.back(); t.sap[j] = psap.back(); t.runTs[j] = pts.back();
      }
      CHECK(asched_jobs_patch(h, (int)rows.size(), rows.data(), pnode.data(), psap.data(), pts.data()) == 0);
      checkOrder(h, t);
      int before = t.M;
      t.add(rng, 333, false, 4, -1);
      CHECK(t.append(h, before) == 0);
      checkOrder(h, t);
      round(h, t, "append after a patch"); }
    // refusals: the handle stays as it was
    { Table b; b.add(rng, 3, false, 1, -1);
      asched_jobs jb = b.view(0, 3);
      int32_t badPc[3] = {0, 3, 0}, badQ[3] = {0, -2, 0}, badCls[3] = {0, 0, 1}, runNode[3] = {-1, 2, -1}, oldGang[3] = {500 + table, 500 + table, 500 + table}, q1[3] = {1, 1, 1};
      uint8_t away[3] = {0, 0, 1}; double bid[3] = {1, 1, 1};
      asched_jobs x = jb; x.pc = badPc; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_INVALID);
      x = jb; x.queue = badQ; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_INVALID);
      x = jb; x.req_class = badCls; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_INVALID);
      x = jb; x.node = runNode; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_INVALID);
      x = jb; x.away = away; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_INVALID);
      x = jb; x.req = nullptr; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_INVALID);
      x = jb; x.m = -1; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_INVALID);
      x = jb; x.bid_price = bid; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_UNSUPPORTED);
      x = jb; x.m = 1 << 30; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_UNSUPPORTED);   // M + m above 2^30: refused before any row is read
      x = jb; x.queue = q1; x.gang_id = oldGang; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_UNSUPPORTED);
      int64_t odd[3 * R] = {12345, 777, 0, 0, 12345, 777, 0, 0, 12345, 777, 0, 0};   // (a request vector the table does not hold: still refused in the validation loop, before any shape is looked up)
      x = jb; x.req = odd; x.queue = q1; x.gang_id = oldGang; CHECK(asched_jobs_append(h, &x) == ASCHED_ERR_UNSUPPORTED);
      checkOrder(h, t);
      round(h, t, "after the refusals"); }
  }
  { // an append that re-allocates AND brings new shapes: the rebuild (masks, fast structure, failed-selection store) runs at the new capacity
    Table t; t.add(rng, 3011, true, 4, -1);
    CHECK(t.set(h) == 0);
    t.add(rng, 40, false, 9, 900);
    t.add(rng, 100, false, 9, -1);
    CHECK(t.append(h, 3011) == 0);
    CHECK(asched_jobs_append_stats(h, st) == 0 && st[2] > 0 && st[4] == 1 && st[5] == 1 && st[6] >= t.M);
    checkOrder(h, t);
    round(h, t, "re-allocating append with new shapes");
    int before = t.M;
    t.add(rng, 500, false, 9, -1);   // and one that fits behind it
    CHECK(t.append(h, before) == 0);
    CHECK(asched_jobs_append_stats(h, st) == 0 && st[4] == 0);
    checkOrder(h, t);
    round(h, t, "append behind it"); }
  asched_destroy(h);
  { // a refusal AFTER the shape lookup (LIT_TMAX + 1 node types and a new request vector off the index grid): the shape table, the grown mirrors, the key layout and
    // the away rows are put back, and the handle goes on as if the call had not been made
    const int N2 = 2 * (LIT_TMAX + 1);
    static const int32_t labelKey[1] = {3};
    c.num_indexed_labels = 1; c.indexed_label_keys = labelKey;
    asched_t* g = asched_create(&c);
    CHECK(g != nullptr);
    if (!g) return 1;
    std::vector<uint64_t> index2(N2); std::vector<int32_t> rank2(N2), lOff(N2 + 1), lKey(N2, 3), lVal(N2); std::vector<int64_t> total2((size_t)N2 * R, 0);
    for (int i = 0; i < N2; i++) { index2[i] = i + 1; rank2[i] = i; lOff[i] = i; lVal[i] = i % (LIT_TMAX + 1); total2[(size_t)i * R] = 1ll << 46; total2[(size_t)i * R + 1] = 64000000; total2[(size_t)i * R + 2] = 1ll << 46; }
    lOff[N2] = N2;
    asched_nodes nd2; memset(&nd2, 0, sizeof nd2);
    nd2.n = N2; nd2.index = index2.data(); nd2.id_rank = rank2.data(); nd2.total = total2.data(); nd2.allocatable = total2.data();
    nd2.label_off = lOff.data(); nd2.label_key = lKey.data(); nd2.label_value = lVal.data();
    CHECK(asched_nodes_upsert(g, &nd2) == 0);
    Table t; t.add(rng, 300, true, 4, -1);
    for (int j = 0; j < t.M; j++) if (t.node[j] >= N) t.node[j] = -1;
    CHECK(t.set(g) == 0);
    checkOrder(g, t);
    { Table b; b.add(rng, 3, false, 1, -1);
      b.req[1] = 7000; b.req[R + 1] = 1500;   // row 0: a new shape on the grid; row 1: a new shape off it (cpu 1 500 at a resolution of 1 000)
      for (int k = 0; k < 2; k++) {
        CHECK(b.append(g, 0) == ASCHED_ERR_UNSUPPORTED);
        CHECK(strstr(asched_last_error(g), "LIT_TMAX") != nullptr);
        checkOrder(g, t);
      } }
    int before = t.M;
    t.add(rng, 200, false, 4, -1);   // known shapes: the device path, rows behind the ones the handle had before the refusals
    CHECK(t.append(g, before) == 0);
    CHECK(asched_jobs_append_stats(g, st) == 0 && st[2] == 0 && st[5] == 0);
    checkOrder(g, t);
    before = t.M;
    t.add(rng, 60, false, 9, -1);    // new shapes on the grid
    CHECK(t.append(g, before) == 0);
    CHECK(asched_jobs_append_stats(g, st) == 0 && st[2] > 0 && st[5] == 1);
    checkOrder(g, t);
    round(g, t, "after a refusal behind the shape lookup");
    asched_destroy(g); }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("jobs_append under ASan + UBSan: all appends ok\n");
  return 0;
}
