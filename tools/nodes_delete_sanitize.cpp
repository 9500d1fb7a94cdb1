// asched_nodes_delete (asched_host.inc + kernels_nodes_delete.h) of the CPU build of the device code, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: the delete counts and chosen rows of tests/test_z_nodes_delete.py (a) on one handle, one after the other (the device path), both reasons
// for the rebuild path, a table with 65 requirement classes (two words of class bits per node, no node class word), a delete before any job table, a table across the
// compaction's chunks, and every refusal — after each accepted delete the map, every job's first fit at every priority, the totals and a round are compared with a
// second handle that was given the reduced node table by asched_nodes_upsert and the job table with its runs on the new positions by asched_jobs_set.  In the CPU
// build the "device" arrays are heap blocks: a lane, a mask word or a job's node written out of bounds shows up here as a heap overflow.
// Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/nodes_delete_sanitize tools/nodes_delete_sanitize.cpp && /tmp/nodes_delete_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4, Q = 3, N0 = 130, M = 500;
static const int32_t pcPrio[3] = {0, 1, 3};
static const int64_t GI = 1ll << 30, MI128 = 128ll << 20;

struct Nodes {   // the node table as asched_nodes_upsert is given it
  std::vector<uint64_t> index; std::vector<int32_t> rank, lVal; std::vector<int64_t> total, alloc; std::vector<uint8_t> uns, over;
  std::vector<std::vector<std::array<int32_t, 3>>> taints;
  int n() const { return (int)index.size(); }
  explicit Nodes(int N = N0) {
    for (int i = 0; i < N; i++) {
      index.push_back((uint64_t)((i * 7919) % (8 * N + 1)) * N + i + 1); rank.push_back(i); lVal.push_back((i / 2) % 2);
      const int64_t t[R] = {64 * GI, 16000, 512 * GI, i % 9 == 0 ? 4 : 0};
      total.insert(total.end(), t, t + R);
      alloc.insert(alloc.end(), t, t + R);
      if (i % 4 == 0) alloc[(size_t)i * R + 1] -= 1000 * (i % 5);   // every node's planes differ from its neighbours'
      uns.push_back(i % 7 == 3); over.push_back(0);
      taints.push_back({});
      if (i % 5 == 0) taints.back().push_back({7, 1, 1});
    }
  }
  int upsert(asched_t* h) const {
    const int N = n();
    std::vector<int32_t> tOff(1, 0), tKey, tVal, tEff, lOff, lKey(N, 3);
    for (auto& tv : taints) { for (auto& x : tv) { tKey.push_back(x[0]); tVal.push_back(x[1]); tEff.push_back(x[2]); } tOff.push_back((int32_t)tKey.size()); }
    tKey.push_back(0); tVal.push_back(0); tEff.push_back(0);
    for (int i = 0; i <= N; i++) lOff.push_back(i);
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = alloc.data(); nd.unschedulable = uns.data(); nd.over_allocated = over.data();
    nd.taint_off = tOff.data(); nd.taint_key = tKey.data(); nd.taint_value = tVal.data(); nd.taint_effect = tEff.data();
    nd.label_off = lOff.data(); nd.label_key = lKey.data(); nd.label_value = lVal.data();
    return asched_nodes_upsert(h, &nd);
  }
  // the table without `rows` and the old -> new map
  Nodes reduced(const std::vector<int32_t>& rows, std::vector<int32_t>* map) const {
    const int N = n();
    std::vector<uint8_t> gone(N, 0);
    for (int v : rows) gone[v] = 1;
    Nodes t(0);
    map->assign(N, -1);
    for (int i = 0; i < N; i++) {
      if (gone[i]) continue;
      (*map)[i] = t.n();
      t.index.push_back(index[i]); t.rank.push_back(rank[i]); t.lVal.push_back(lVal[i]); t.uns.push_back(uns[i]); t.over.push_back(over[i]); t.taints.push_back(taints[i]);
      t.total.insert(t.total.end(), total.begin() + (size_t)i * R, total.begin() + (size_t)(i + 1) * R);
      t.alloc.insert(t.alloc.end(), alloc.begin() + (size_t)i * R, alloc.begin() + (size_t)(i + 1) * R);
    }
    return t;
  }
  bool sameTypes(const std::vector<int32_t>& rows) const {   // no node type (label value, taint, flag) loses its last node
    int cnt[8] = {0};
    std::vector<uint8_t> gone(n(), 0);
    for (int v : rows) gone[v] = 1;
    for (int i = 0; i < n(); i++) { const int ty = lVal[i] * 4 + (taints[i].empty() ? 0 : 2) + uns[i]; if (!gone[i]) cnt[ty] |= 2; else cnt[ty] |= 1; }
    for (int k = 0; k < 8; k++) if (cnt[k] == 1) return false;
    return true;
  }
};

struct Jobs {
  std::vector<int32_t> queue, pc, cls, node, prio; std::vector<int64_t> req, ts; int ncls;
  Jobs(std::mt19937& rng, int ncls_, int N, int runAbove = 0) : ncls(ncls_) {
    std::vector<int64_t> freeCpu(N, 15000), freeMem(N, 60 * GI);
    for (int j = 0; j < M; j++) {
      queue.push_back((int)(rng() % Q)); pc.push_back((int)(rng() % 3)); cls.push_back((int)(rng() % ncls));
      const int64_t q[R] = {(int64_t)(4 << (rng() % 4)) * GI, (int64_t)(1000 << (rng() % 4)), 0, 0};
      req.insert(req.end(), q, q + R);
      int v = -1;
      if (rng() % 2) { v = runAbove + (int)(rng() % (N - runAbove)); if (q[0] > freeMem[v] || q[1] > freeCpu[v]) v = -1; else { freeMem[v] -= q[0]; freeCpu[v] -= q[1]; } }
      node.push_back(v); prio.push_back(v >= 0 ? pcPrio[pc[j]] : 0); ts.push_back(v >= 0 ? (int64_t)(1 + rng() % 5) * 1000000000ll : 0);
    }
  }
  int set(asched_t* h) const {
    // class 1 tolerates key 7, class 3 the unschedulable taint, class 2 selects label value 1, classes 4.. tolerate (7, 1, NoSchedule) by value
    std::vector<int32_t> tOff(1, 0), tKey, tOp, tVal, tEff, sOff(1, 0), sKey, sVal;
    for (int c = 0; c < ncls; c++) {
      if (c == 1) { tKey.push_back(7); tOp.push_back(ASCHED_TOLERATION_OP_EXISTS); tVal.push_back(0); tEff.push_back(0); }
      if (c == 3) { tKey.push_back(-2); tOp.push_back(ASCHED_TOLERATION_OP_EXISTS); tVal.push_back(0); tEff.push_back(0); }
      if (c >= 4) { tKey.push_back(7); tOp.push_back(0); tVal.push_back(1); tEff.push_back(1); }
      if (c == 2) { sKey.push_back(3); sVal.push_back(1); }
      tOff.push_back((int32_t)tKey.size()); sOff.push_back((int32_t)sKey.size());
    }
    tKey.push_back(0); tOp.push_back(0); tVal.push_back(0); tEff.push_back(0); sKey.push_back(0); sVal.push_back(0);
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = ncls; rc.tol_off = tOff.data(); rc.tol_key = tKey.data(); rc.tol_op = tOp.data(); rc.tol_value = tVal.data(); rc.tol_effect = tEff.data();
    rc.sel_off = sOff.data(); rc.sel_key = sKey.data(); rc.sel_value = sVal.data();
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = M; jb.queue = queue.data(); jb.pc = pc.data(); jb.req = req.data(); jb.req_class = cls.data();
    jb.node = node.data(); jb.scheduled_at_priority = prio.data(); jb.run_timestamp = ts.data();
    return asched_jobs_set(h, &jb, &rc);
  }
  // the runs on `rows` end: the job rows, and the table with them unbound
  std::vector<int32_t> unbind(const std::vector<int32_t>& rows, int N) {
    std::vector<uint8_t> gone(N, 0);
    for (int v : rows) gone[v] = 1;
    std::vector<int32_t> jobs;
    for (int j = 0; j < M; j++) if (node[j] >= 0 && gone[node[j]]) { jobs.push_back(j); node[j] = -1; prio[j] = 0; ts[j] = 0; }
    return jobs;
  }
  int renumber(const std::vector<int32_t>& map, int first) {
    int moved = 0;
    for (int j = 0; j < M; j++) if (node[j] >= 0) { if (node[j] > first) moved++; node[j] = map[node[j]]; }
    return moved;
  }
};

static int roundOf(asched_t* h, const Jobs& t, int* preempted) {
  std::vector<double> weight(Q, 1.0), qTok(Q, 1e18); std::vector<int64_t> qBurst(Q, 1ll << 62); std::vector<uint8_t> qInf(Q, 1); std::vector<int32_t> qOff(Q + 1, 0), queued;
  for (int q = 0; q < Q; q++) {
    for (int p = 2; p >= 0; p--) for (int j = 0; j < M; j++) if (t.queue[j] == q && t.pc[j] == p && t.node[j] < 0) queued.push_back(j);   // priority-class priority descending, then the row
    qOff[q + 1] = (int32_t)queued.size();
  }
  asched_queues qs; memset(&qs, 0, sizeof qs);
  qs.q = Q; qs.weight = weight.data(); qs.global_tokens = 1e18; qs.global_burst = 1ll << 62; qs.global_rate_inf = 1; qs.queue_tokens = qTok.data(); qs.queue_burst = qBurst.data();
  qs.queue_rate_inf = qInf.data(); qs.queued_off = qOff.data(); qs.queued_jobs = queued.data();
  CHECK(asched_round_prepare(h, &qs) == 0);
  asched_round_result res;
  int rc = asched_schedule_round(h, &res);
  CHECK(rc == 0);
  if (rc) { fprintf(stderr, "round: %s\n", asched_last_error(h)); return -1; }
  *preempted = res.num_preempted;
  uint32_t sum = (uint32_t)res.num_scheduled;
  for (int i = 0; i < res.num_scheduled; i++) sum = sum * 31u + (uint32_t)res.scheduled_job[i] * 7u + (uint32_t)res.scheduled_node[i];
  for (int i = 0; i < res.num_preempted; i++) sum = sum * 31u + (uint32_t)res.preempted_job[i] * 7u + (uint32_t)res.preempted_node[i];
  return (int)(sum & 0x7fffffffu);
}

// the handle after a delete against a handle that is given the restated tables by nodes_upsert and jobs_set
static void compare(asched_t* h, asched_t* f, const Nodes& t, const Jobs& jobs, const char* what) {
  CHECK(t.upsert(f) == 0 && jobs.set(f) == 0);
  CHECK(asched_num_nodes(h) == t.n() && asched_num_nodes(f) == t.n());
  std::vector<int32_t> ids(M), a(M), b(M), prios(ASCHED_MAX_PRIORITIES);
  for (int j = 0; j < M; j++) ids[j] = j;
  const int P = asched_priorities(h, prios.data());
  for (int l = 0; l < P; l++) {
    CHECK(asched_fit_select_batch(h, M, ids.data(), prios[l], a.data()) == 0 && asched_fit_select_batch(f, M, ids.data(), prios[l], b.data()) == 0);
    CHECK(a == b);
  }
  int64_t ta[R], tb[R];
  CHECK(asched_total_resources(h, ta) == 0 && asched_total_resources(f, tb) == 0 && std::equal(ta, ta + R, tb));
  std::vector<int64_t> pa_((size_t)t.n() * P * R), pb_((size_t)t.n() * P * R);
  CHECK(asched_get_nodes_alloc(h, t.n(), nullptr, pa_.data()) == 0 && asched_get_nodes_alloc(f, t.n(), nullptr, pb_.data()) == 0 && pa_ == pb_);
  for (int j = 0; j < M; j += 50) {
    int32_t x[2], y[2];
    CHECK(asched_node_types_matching_job(h, j, &x[0], &x[1]) == 0 && asched_node_types_matching_job(f, j, &y[0], &y[1]) == 0 && x[0] == y[0] && x[1] == y[1]);
  }
  int pa = 0, pb = 0;
  const int ra = roundOf(h, jobs, &pa), rb = roundOf(f, jobs, &pb);
  CHECK(ra == rb && pa == pb);
  printf("%s: as nodes_upsert of the reduced table (%d nodes, round checksum %d)\n", what, t.n(), ra);
}

static std::vector<int32_t> rowsOf(std::mt19937& rng, const Nodes& t, int n) {
  const int N = t.n();
  std::vector<int32_t> rest;
  int last[8]; for (int k = 0; k < 8; k++) last[k] = -1;
  for (int i = 0; i < N; i++) last[t.lVal[i] * 4 + (t.taints[i].empty() ? 0 : 2) + t.uns[i]] = i;   // below N - 1 rows the last node of every type stays (f. is the rebuild path)
  for (int i = 0; i < N; i++) if (n >= N - 1 || std::find(last, last + 8, i) == last + 8) rest.push_back(i);
  std::shuffle(rest.begin(), rest.end(), rng);
  rest.resize(n);
  return rest;
}

// the documented sequence on h: the runs on the rows end (jobs_patch with node -1), the rows leave; t and jobs follow; -> the statistics in st
static int deleteRows(asched_t* h, Nodes* t, Jobs* jobs, const std::vector<int32_t>& rows, int32_t* st, bool haveJobs = true) {
  const int N = t->n();
  if (haveJobs) {
    std::vector<int32_t> on = jobs->unbind(rows, N), minus(on.size(), -1), zero(on.size(), 0); std::vector<int64_t> zts(on.size(), 0);
    if (!on.empty()) CHECK(asched_jobs_patch(h, (int32_t)on.size(), on.data(), minus.data(), zero.data(), zts.data()) == 0);
  }
  std::vector<int32_t> got(N, -2), want;
  int rc = asched_nodes_delete(h, (int32_t)rows.size(), rows.data(), got.data());
  if (rc) { fprintf(stderr, "nodes_delete: %s\n", asched_last_error(h)); return rc; }
  Nodes r = t->reduced(rows, &want);
  CHECK(got == want);
  const int first = rows.empty() ? N : *std::min_element(rows.begin(), rows.end());
  const int moved = haveJobs ? jobs->renumber(want, first) : 0;
  CHECK(asched_nodes_delete_stats(h, st) == 0 && st[0] == (int)rows.size() && st[1] == moved && st[4] == r.n() && st[5] == 0 && st[6] == 0 && st[7] == 0);
  *t = r;
  return 0;
}

static asched_t* create(const asched_config& c) { asched_t* h = asched_create(&c); CHECK(h != nullptr); if (!h) exit(1); return h; }

int main() {
  static const int32_t indexedCol[3] = {1, 0, 3}, labelKey[1] = {3};
  static const int64_t indexedRes[3] = {1000, MI128, 1};
  static const uint8_t pcPre[3] = {1, 1, 0};
  static const double drf[4] = {1.0, 1.0, 0.0, 1.0};
  // pc 1 away at priority 0 on well-known type 0, pc 2 away at 2 on type 1 and at 1 on type 0 (mask rows behind the shape rows)
  static const int32_t awayOff[4] = {0, 0, 1, 3}, awayPrio[3] = {0, 2, 1}, awayWkt[3] = {0, 1, 0}, wktOff[3] = {0, 1, 2}, wktKey[2] = {7, 7}, wktVal[2] = {1, -1}, wktEff[2] = {1, 1};
  asched_config c; memset(&c, 0, sizeof c);
  c.num_resources = R; c.num_indexed = 3; c.indexed_col = indexedCol; c.indexed_resolution = indexedRes;
  c.num_priority_classes = 3; c.pc_priority = pcPrio; c.pc_preemptible = pcPre; c.drf_multiplier = drf; c.device = -1;
  c.num_indexed_taints = -1; c.num_indexed_labels = 1; c.indexed_label_keys = labelKey;
  c.pc_away_off = awayOff; c.away_priority = awayPrio; c.away_well_known = awayWkt;
  c.num_well_known_types = 2; c.wkt_taint_off = wktOff; c.wkt_taint_key = wktKey; c.wkt_taint_value = wktVal; c.wkt_taint_effect = wktEff;
  setvbuf(stdout, nullptr, _IONBF, 0);   // (in step with the checks' stderr)
  std::mt19937 rng(11);
  int32_t st[8];
  for (int ncls : {4, 65}) {
    asched_t* h = create(c); asched_t* f = create(c);
    const Jobs jobs0(rng, ncls, N0, ncls == 65 ? 70 : 0);
    { int32_t row = 0; CHECK(asched_nodes_delete(h, 1, &row, nullptr) == ASCHED_ERR_INVALID); }   // no node table
    { Nodes t; Jobs jobs = jobs0;   // before any job table: node arrays and mirrors only
      CHECK(t.upsert(h) == 0);
      CHECK(deleteRows(h, &t, &jobs, rowsOf(rng, t, 5), st, false) == 0 && st[2] == 0);
      std::vector<int32_t> none;
      Jobs queued = jobs0; queued.unbind(rowsOf(rng, Nodes(), N0), N0);   // (every job queued: the runs of jobs0 name rows of the whole table)
      CHECK(queued.set(h) == 0);
      compare(h, f, t, queued, "a delete before the job table"); }
    static const int counts[] = {0, 1, 2, 63, 64, 65, 66, 129};
    for (int n : counts) {   // the counts of (a), every delete on the handle the one before it left (the tables are uploaded again: 129 leaves one node)
      Nodes t; Jobs jobs = jobs0;
      CHECK(t.upsert(h) == 0 && jobs.set(h) == 0 && asched_nodes_delete_stats(h, st) == 0 && st[0] == 0 && st[4] == 0);
      int pre = 0; roundOf(h, jobs, &pre);   // (the delete finds a handle that has run a round)
      const std::vector<int32_t> rows = rowsOf(rng, t, n);
      const bool same = t.sameTypes(rows);
      CHECK(deleteRows(h, &t, &jobs, rows, st) == 0 && st[2] == (same ? 0 : 1) && (n > 66 || st[2] == 0));
      char what[64]; snprintf(what, sizeof what, "%d classes, %3d rows", ncls, n);
      compare(h, f, t, jobs, what);
      if (n == 63) {   // and a second and third delete on top of it, without an upload in between
        CHECK(deleteRows(h, &t, &jobs, rowsOf(rng, t, 3), st) == 0 && st[2] == 0);
        CHECK(deleteRows(h, &t, &jobs, {}, st) == 0 && st[0] == 0);
        compare(h, f, t, jobs, "  and three more, then none");
      }
    }
    { // chosen rows: the first, the last, a whole word, every other row, a run across a word border
      std::vector<std::vector<int32_t>> chosen = {{0}, {129}, {}, {}, {}};
      for (int i = 0; i < 64; i++) chosen[2].push_back(i);
      for (int i = 0; i < N0; i += 2) chosen[3].push_back(i);
      for (int i = 60; i <= 70; i++) chosen[4].push_back(i);
      for (auto& rows : chosen) {
        Nodes t; Jobs jobs = jobs0;
        CHECK(t.upsert(h) == 0 && jobs.set(h) == 0);
        CHECK(t.sameTypes(rows) && deleteRows(h, &t, &jobs, rows, st) == 0 && st[2] == 0 && st[3] == 0);
        char what[64]; snprintf(what, sizeof what, "%d classes, rows %d.. (%zu)", ncls, rows[0], rows.size());
        compare(h, f, t, jobs, what);
      }
    }
    { // the rebuild path: a type emptied; a label value emptied; then the device path again
      Nodes t; Jobs jobs = jobs0;
      CHECK(t.upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(deleteRows(h, &t, &jobs, {10, 115}, st) == 0 && st[2] == 1 && st[3] == 2);   // the only tainted and unschedulable nodes with label value 1
      compare(h, f, t, jobs, "rebuild: a node type emptied");
      t.lVal[77] = 9;   // the only node with value 9 of the indexed label
      CHECK(t.upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(deleteRows(h, &t, &jobs, {77}, st) == 0 && st[2] == 1 && st[3] == 4);
      int32_t vals[8]; CHECK(asched_indexed_node_label_values(h, 3, vals, 8) == 2);
      compare(h, f, t, jobs, "rebuild: a label value emptied");
      CHECK(deleteRows(h, &t, &jobs, {1, 2, 66}, st) == 0 && st[2] == 0);
      compare(h, f, t, jobs, "the device path after the rebuilds");
    }
    { // refusals: the handle stays as it was
      Nodes t; Jobs jobs = jobs0;
      CHECK(t.upsert(h) == 0 && jobs.set(h) == 0);
      const int N = t.n();
      int busy = -1, lowest = -1;
      for (int j = M - 1; j >= 0; j--) if (jobs.node[j] >= 0) { busy = jobs.node[j]; break; }
      for (int j = 0; j < M; j++) if (jobs.node[j] == busy) { lowest = j; break; }
      int32_t two[2] = {0, N}, neg[1] = {-1}, twice[3] = {3, 7, 3}, on[1] = {busy};
      std::vector<int32_t> all(N); for (int i = 0; i < N; i++) all[i] = i;
      CHECK(asched_nodes_delete(h, -1, two, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_nodes_delete(h, 2, nullptr, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_nodes_delete(h, 2, two, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_nodes_delete(h, 1, neg, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_nodes_delete(h, 3, twice, nullptr) == ASCHED_ERR_INVALID);
      CHECK(asched_nodes_delete(h, 1, on, nullptr) == ASCHED_ERR_INVALID);
      { char want[64]; snprintf(want, sizeof want, "job row %d ", lowest); CHECK(strstr(asched_last_error(h), want) != nullptr); }
      CHECK(asched_nodes_delete(h, N, all.data(), nullptr) == ASCHED_ERR_UNSUPPORTED);
      CHECK(asched_nodes_delete(nullptr, 0, nullptr, nullptr) == ASCHED_ERR_INVALID);
      compare(h, f, t, jobs, "after the refusals");
      CHECK(t.upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(deleteRows(h, &t, &jobs, {busy, 3, 7}, st) == 0);   // after jobs_patch with node -1 the same row leaves (a row named twice left no mark)
      compare(h, f, t, jobs, "the busy row, its runs ended first");
    }
    asched_destroy(h); asched_destroy(f);
  }
  { // across the chunks of the grid-wide compaction: 2 x 4096 + 517 nodes
    asched_t* h = create(c); asched_t* f = create(c);
    const int NB = 2 * 4096 + 517;
    const Jobs jobs0(rng, 4, NB);
    for (int n : {1, 4095, 4096, 4097}) {
      Nodes t(NB); Jobs jobs = jobs0;
      CHECK(t.upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(deleteRows(h, &t, &jobs, rowsOf(rng, t, n), st) == 0 && st[2] == 0);
      char what[64]; snprintf(what, sizeof what, "%d nodes, %4d rows", NB, n);
      compare(h, f, t, jobs, what);
    }
    asched_destroy(h); asched_destroy(f);
  }
  { // tables nodes_delete does not serve
    asched_t* h = create(c);
    Nodes t;
    const int N = t.n();
    std::vector<int64_t> ov(N, 1), abp;
    const int P = 2 + 3;
    for (int i = 0; i < N; i++) for (int l = 0; l < P; l++) for (int r = 0; r < R; r++) abp.push_back(t.total[(size_t)i * R + r]);
    int32_t row = 0;
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = N; nd.index = t.index.data(); nd.id_rank = t.rank.data(); nd.total = t.total.data(); nd.allocatable = t.alloc.data();
    nd.node_type_override = ov.data();
    CHECK(asched_nodes_upsert(h, &nd) == 0 && asched_nodes_delete(h, 1, &row, nullptr) == ASCHED_ERR_UNSUPPORTED);
    nd.node_type_override = nullptr; nd.alloc_by_prio = abp.data();
    CHECK(asched_nodes_upsert(h, &nd) == 0 && asched_nodes_delete(h, 1, &row, nullptr) == ASCHED_ERR_UNSUPPORTED);
    nd.alloc_by_prio = nullptr;
    CHECK(asched_nodes_upsert(h, &nd) == 0 && asched_nodes_delete(h, 1, &row, nullptr) == 0 && asched_num_nodes(h) == N - 1);
    asched_destroy(h);
  }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("nodes_delete under ASan + UBSan: all deletes ok\n");
  return 0;
}
