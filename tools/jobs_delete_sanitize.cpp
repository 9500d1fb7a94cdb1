// asched_jobs_delete (asched_host.inc + kernels_jobs_delete.h) of the CPU build of the device code, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: deletes of the counts of tests/test_z_jobs_delete.py (a) each on a fresh table, the full-chunk and last-row cases of the compaction on a
// table of three chunks, and delete / append-with-regrow / patch / delete sequences on one handle with rounds in between, whole gangs and every row of a shape among the
// deleted rows, then the refusals — every order and id map checked against a restatement written here (std::sort over the reduced table, a running count of kept rows).
// In the CPU build the "device" arrays are heap blocks: a gather that reads past the old table or writes past a fresh block shows up here as a heap overflow, a block
// released twice or used after its release as such.  Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/jobs_delete_sanitize tools/jobs_delete_sanitize.cpp && /tmp/jobs_delete_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int CMP_CHUNK = 4096;   // armada_amd/csrc/kernels_split.h: elements per workgroup of the device's compaction
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
  // asched_jobs_delete of `rows`, the id map checked against the running count of kept rows, then the table reduced in the same way
  int remove(asched_t* h, const std::vector<int32_t>& rows, bool wantMap = true) {
    std::vector<int32_t> map(M + 1, -7);
    int rc = asched_jobs_delete(h, (int)rows.size(), rows.data(), wantMap ? map.data() : nullptr);
    if (rc) return rc;
    std::vector<uint8_t> gone(M, 0);
    for (int j : rows) gone[j] = 1;
    int o = 0;
    for (int j = 0; j < M; j++) {
      if (wantMap) CHECK(map[j] == (gone[j] ? -1 : o));
      if (gone[j]) continue;
      queue[o] = queue[j]; pc[o] = pc[j]; node[o] = node[j]; sap[o] = sap[j]; cls[o] = cls[j]; gang[o] = gang[j]; card[o] = card[j]; qprio[o] = qprio[j]; submit[o] = submit[j]; runTs[o] = runTs[j];
      for (int r = 0; r < R; r++) req[(size_t)o * R + r] = req[(size_t)j * R + r];
      o++;
    }
    CHECK(map[M] == -7);   // (nothing behind the M entries of the map)
    M = o;
    for (auto* v : {&queue, &pc, &node, &sap, &cls, &gang, &card}) v->resize(M);
    qprio.resize(M); submit.resize(M); runTs.resize(M); req.resize((size_t)M * R);
    return 0;
  }
};

static std::vector<int32_t> draw(std::mt19937& rng, int M, int d) {   // d distinct rows in no particular order
  std::vector<int32_t> all(M);
  for (int j = 0; j < M; j++) all[j] = j;
  std::shuffle(all.begin(), all.end(), rng);
  all.resize(d);
  return all;
}

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
  else printf("%s: round: %d scheduled, %d preempted\n", what, res.num_scheduled, res.num_preempted);
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
  { int32_t row = 0; CHECK(asched_jobs_delete(h, 1, &row, nullptr) == ASCHED_ERR_INVALID); }   // no job table
  std::vector<uint64_t> index(N); std::vector<int32_t> rank(N); std::vector<int64_t> total((size_t)N * R, 0);
  for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * R] = 1ll << 46; total[(size_t)i * R + 1] = 64000000; total[(size_t)i * R + 2] = 1ll << 46; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data();
  CHECK(asched_nodes_upsert(h, &nd) == 0);
  // the counts of the test file, each on a fresh table of the same handle
  static const int counts[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 3010};
  for (int d : counts) {
    Table t; t.add(rng, 3011, true, 4, -1);
    CHECK(t.set(h) == 0);
    CHECK(t.remove(h, draw(rng, t.M, d)) == 0);
    CHECK(asched_jobs_delete_stats(h, st) == 0 && st[0] == d && st[4] == t.M && st[5] >= 3011);
    checkOrder(h, t);
    printf("delete of %4d rows ok (%d left, capacity %d)\n", d, t.M, st[5]);
  }
  // three chunks of the compaction, the last one partly filled: counts around a chunk, a full chunk, the last chunk, the last row, everything but the last row
  { const int MB = 2 * CMP_CHUNK + 517;
    struct Case { const char* what; int lo, hi, d; };
    static const Case cases[] = {{"chunk - 1 random rows", 0, 0, CMP_CHUNK - 1}, {"chunk random rows", 0, 0, CMP_CHUNK}, {"chunk + 1 random rows", 0, 0, CMP_CHUNK + 1},
                                 {"a run across the first chunk boundary", CMP_CHUNK - 100, CMP_CHUNK + 100, 0}, {"exactly the second chunk", CMP_CHUNK, 2 * CMP_CHUNK, 0},
                                 {"the last chunk's rows", 2 * CMP_CHUNK, MB, 0}, {"the last row", MB - 1, MB, 0}, {"row 0", 0, 1, 0}, {"everything but the last row", 0, MB - 1, 0},
                                 {"everything but row 0", 1, MB, 0}};
    for (const Case& k : cases) {
      Table t; t.add(rng, MB, true, 4, -1);
      CHECK(t.set(h) == 0);
      std::vector<int32_t> rows;
      if (k.d) rows = draw(rng, MB, k.d); else for (int j = k.lo; j < k.hi; j++) rows.push_back(j);
      CHECK(t.remove(h, rows) == 0);
      checkOrder(h, t);
      printf("%s ok (%d left)\n", k.what, t.M);
    } }
  for (int table = 0; table < 2; table++) {   // the second table: the buffers of the first are gone with it
    Table t; t.add(rng, table ? 777 : 3011, true, 4, -1);
    t.add(rng, 40, false, 4, 100);             // ten gangs
    CHECK(t.set(h) == 0);
    // delete / append-with-regrow / patch / delete, three times over, rounds in between
    for (int k = 0; k < 3; k++) {
      CHECK(t.remove(h, draw(rng, t.M, t.M / 4), k != 1) == 0);   // (once without the id map)
      checkOrder(h, t);
      round(h, t, "after a delete");
      int before = t.M;
      t.add(rng, before / 2 + 300, false, 4, -1);                 // outgrows 1.25 x the capacity at least once
      CHECK(t.append(h, before) == 0);
      CHECK(asched_jobs_append_stats(h, st) == 0 && st[0] == t.M - before && st[6] >= t.M);
      checkOrder(h, t);
      std::vector<int32_t> rows, pnode, psap; std::vector<int64_t> pts;
      for (int j = 0; j < t.M; j += 7) if (t.gang[j] < 0) {
        bool stop = t.node[j] >= 0;
        rows.push_back(j); pnode.push_back(stop ? -1 : j % N); psap.push_back(stop ? 0 : pcPrio[t.pc[j]]); pts.push_back(stop ? 0 : 9000000000ll);
        t.node[j] = pnode.back(); t.sap[j] = psap.back(); t.runTs[j] = pts.back();
      }
      CHECK(asched_jobs_patch(h, (int)rows.size(), rows.data(), pnode.data(), psap.data(), pts.data()) == 0);
      checkOrder(h, t);
      CHECK(t.remove(h, draw(rng, t.M, 100)) == 0);
      checkOrder(h, t);
      round(h, t, "after delete, append, patch, delete");
    }
    { // whole gangs, and every row of one request vector: an emptied gang's key comes again as a new gang, an emptied shape's rows come again through the rebuild
      std::vector<int32_t> rows;
      for (int j = 0; j < t.M; j++) if (t.gang[j] >= 100 && t.gang[j] < 105) rows.push_back(j);
      const int64_t r0 = t.req[0], r1 = t.req[1];
      for (int j = 0; j < t.M; j++) if (t.gang[j] < 0 && t.req[(size_t)j * R] == r0 && t.req[(size_t)j * R + 1] == r1) rows.push_back(j);
      CHECK(t.remove(h, rows) == 0);
      CHECK(asched_jobs_delete_stats(h, st) == 0 && st[3] > 0);
      checkOrder(h, t);
      round(h, t, "whole gangs and a whole shape gone");
      int before = t.M;
      t.add(rng, 8, false, 4, 100);            // the keys of two of the emptied gangs
      t.add(rng, 50, false, 4, -1);            // every request vector of the draw, the emptied one among them
      CHECK(t.append(h, before) == 0);
      CHECK(asched_jobs_append_stats(h, st) == 0 && st[3] == 2);
      checkOrder(h, t);
      round(h, t, "emptied gangs and shapes appended again"); }
    { // refusals: the handle stays as it was
      std::vector<int32_t> all(t.M);
      for (int j = 0; j < t.M; j++) all[j] = j;
      int32_t outside[2] = {3, t.M}, negative[1] = {-1}, twice[3] = {5, 9, 5};
      CHECK(asched_jobs_delete(h, 2, outside, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_jobs_delete(h, 1, negative, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_jobs_delete(h, 3, twice, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_jobs_delete(h, -1, twice, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_jobs_delete(h, 2, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_jobs_delete(h, t.M, all.data(), nullptr) == ASCHED_ERR_UNSUPPORTED);
      checkOrder(h, t);
      round(h, t, "after the refusals");
      CHECK(t.remove(h, std::vector<int32_t>{0, t.M - 1}) == 0);   // and the handle still deletes
      checkOrder(h, t); }
  }
  asched_destroy(h);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("jobs_delete under ASan + UBSan: all deletes ok\n");
  return 0;
}
