// asched_nodes_append (asched_host.inc + kernels_nodes_append.h) of the CPU build of the device code, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: the geometry counts of tests/test_z_nodes_append.py (a) one after the other on one handle, on 4 and on 65 requirement classes (two words of
// class bits per entry, no node class word), appends on top of each other without an upload in between, an append before any job table, an append after a delete (the
// returning nodes) and after a jobs_delete, tables uploaded without id ranks, each rebuild reason that can be reached, a table of several workgroups, and every refusal — after each step every job's first fit at every priority,
// every plane, the totals, the node types of sampled jobs and a round are compared with a second handle that was given the grown node table by asched_nodes_upsert and
// the job table by asched_jobs_set.  In the CPU build the "device" arrays are heap blocks: a block that was not grown, a lane or a mask word written out of bounds shows
// up here as a heap overflow.
// Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/nodes_append_sanitize tools/nodes_append_sanitize.cpp && /tmp/nodes_append_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4, Q = 3, N0 = 130, M = 500;
static const int32_t pcPrio[3] = {0, 1, 3};
static const int64_t GI = 1ll << 30, MI128 = 128ll << 20;

struct Nodes {   // a node table as asched_nodes_upsert is given it; rows [from, to) of it as asched_nodes_append is
  std::vector<uint64_t> index; std::vector<int32_t> rank, lVal; std::vector<int64_t> total, alloc; std::vector<uint8_t> uns, over;
  std::vector<std::vector<std::array<int32_t, 3>>> taints;
  bool ranked = true;   // false: asched_nodes_upsert is given no id ranks
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
  Nodes rows(int from, int to) const {
    Nodes t(0);
    t.ranked = ranked;
    for (int i = from; i < to; i++) {
      t.index.push_back(index[i]); t.rank.push_back(rank[i]); t.lVal.push_back(lVal[i]); t.uns.push_back(uns[i]); t.over.push_back(over[i]); t.taints.push_back(taints[i]);
      t.total.insert(t.total.end(), total.begin() + (size_t)i * R, total.begin() + (size_t)(i + 1) * R);
      t.alloc.insert(t.alloc.end(), alloc.begin() + (size_t)i * R, alloc.begin() + (size_t)(i + 1) * R);
    }
    return t;
  }
  void add(const Nodes& o) {
    index.insert(index.end(), o.index.begin(), o.index.end()); rank.insert(rank.end(), o.rank.begin(), o.rank.end()); lVal.insert(lVal.end(), o.lVal.begin(), o.lVal.end());
    total.insert(total.end(), o.total.begin(), o.total.end()); alloc.insert(alloc.end(), o.alloc.begin(), o.alloc.end()); uns.insert(uns.end(), o.uns.begin(), o.uns.end());
    over.insert(over.end(), o.over.begin(), o.over.end()); taints.insert(taints.end(), o.taints.begin(), o.taints.end());
  }
  struct Csr { std::vector<int32_t> tOff, tKey, tVal, tEff, lOff, lKey; };
  Csr csr() const {
    Csr c; const int N = n();
    c.tOff.push_back(0); c.lKey.assign(N + 1, 3);
    for (auto& tv : taints) { for (auto& x : tv) { c.tKey.push_back(x[0]); c.tVal.push_back(x[1]); c.tEff.push_back(x[2]); } c.tOff.push_back((int32_t)c.tKey.size()); }
    c.tKey.push_back(0); c.tVal.push_back(0); c.tEff.push_back(0);
    for (int i = 0; i <= N; i++) c.lOff.push_back(i);
    return c;
  }
  int upsert(asched_t* h) const {
    Csr c = csr();
    std::vector<int32_t> lv = lVal; lv.push_back(0);
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = n(); nd.index = index.data(); nd.id_rank = ranked ? rank.data() : nullptr; nd.total = total.data(); nd.allocatable = alloc.data(); nd.unschedulable = uns.data(); nd.over_allocated = over.data();
    nd.taint_off = c.tOff.data(); nd.taint_key = c.tKey.data(); nd.taint_value = c.tVal.data(); nd.taint_effect = c.tEff.data();
    nd.label_off = c.lOff.data(); nd.label_key = c.lKey.data(); nd.label_value = lv.data();
    return asched_nodes_upsert(h, &nd);
  }
  int append(asched_t* h, bool withRank = true) const {   // this table's rows as the new rows
    Csr c = csr();
    std::vector<int32_t> lv = lVal; lv.push_back(0);
    std::vector<uint64_t> ix = index; ix.push_back(0);
    std::vector<int64_t> tt = total, aa = alloc; tt.push_back(0); aa.push_back(0);
    std::vector<int32_t> rk = rank; rk.push_back(0);
    std::vector<uint8_t> u = uns, o = over; u.push_back(0); o.push_back(0);
    asched_nodes_append_rows a; memset(&a, 0, sizeof a);
    a.m = n(); a.index = ix.data(); a.id_rank = withRank ? rk.data() : nullptr; a.total = tt.data(); a.allocatable = aa.data(); a.unschedulable = u.data(); a.over_allocated = o.data();
    a.taint_off = c.tOff.data(); a.taint_key = c.tKey.data(); a.taint_value = c.tVal.data(); a.taint_effect = c.tEff.data();
    a.label_off = c.lOff.data(); a.label_key = c.lKey.data(); a.label_value = lv.data();
    return asched_nodes_append(h, &a);
  }
};

struct Jobs {
  std::vector<int32_t> queue, pc, cls, node, prio; std::vector<int64_t> req, ts; int ncls;
  Jobs(std::mt19937& rng, int ncls_, int N) : ncls(ncls_) {   // half of the jobs run, on nodes below N
    std::vector<int64_t> freeCpu(N, 15000), freeMem(N, 60 * GI);
    for (int j = 0; j < M; j++) {
      queue.push_back((int)(rng() % Q)); pc.push_back((int)(rng() % 3)); cls.push_back((int)(rng() % ncls));
      const int64_t q[R] = {(int64_t)(4 << (rng() % 4)) * GI, (int64_t)(1000 << (rng() % 4)), 0, 0};
      req.insert(req.end(), q, q + R);
      int v = -1;
      if (rng() % 2) { v = (int)(rng() % N); if (q[0] > freeMem[v] || q[1] > freeCpu[v]) v = -1; else { freeMem[v] -= q[0]; freeCpu[v] -= q[1]; } }
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
  std::vector<int32_t> unbind(int from, int to) {   // the runs on rows [from, to) end
    std::vector<int32_t> jobs;
    for (int j = 0; j < M; j++) if (node[j] >= from && node[j] < to) { jobs.push_back(j); node[j] = -1; prio[j] = 0; ts[j] = 0; }
    return jobs;
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

// the handle after an append against a handle that is given the grown table by nodes_upsert and the job table by jobs_set
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
  printf("%s: as nodes_upsert of the grown table (%d nodes, round checksum %d)\n", what, t.n(), ra);
}

static asched_t* create(const asched_config& c) { asched_t* h = asched_create(&c); CHECK(h != nullptr); if (!h) exit(1); return h; }
static bool stats(asched_t* h, int m, int stride, int rebuilt, int why, int n) {
  int32_t st[8];
  if (asched_nodes_append_stats(h, st)) return false;
  const bool ok = st[0] == m && (stride < 0 || st[1] == stride) && st[2] == rebuilt && st[3] == why && st[4] == n && !st[5] && !st[6] && !st[7];
  if (!ok) fprintf(stderr, "stats %d %d %d %d %d, wanted %d %d %d %d %d\n", st[0], st[1], st[2], st[3], st[4], m, stride, rebuilt, why, n);
  return ok;
}

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
  for (int ncls : {4, 65}) {
    asched_t* h = create(c); asched_t* f = create(c);
    { Nodes one = Nodes(N0 + 1).rows(N0, N0 + 1); CHECK(one.append(h) == ASCHED_ERR_INVALID); }   // no node table
    { // before any job table: node arrays and mirrors only
      const Nodes full(N0 + 70);
      Jobs jobs(rng, ncls, N0);
      CHECK(full.rows(0, N0).upsert(h) == 0 && full.rows(N0, N0 + 70).append(h) == 0 && stats(h, 70, 1, 0, 0, N0 + 70));
      CHECK(jobs.set(h) == 0);
      compare(h, f, full, jobs, "an append before the job table"); }
    static const int geometry[][2] = {{130, 0}, {130, 1}, {130, 2}, {130, 62}, {130, 63}, {130, 64}, {130, 65}, {130, 126}, {130, 127}, {128, 1}, {64, 1}, {1, 129}};
    for (auto& g : geometry) {   // the counts of (a), one after the other on one handle (the head table is uploaded again each time)
      const int n0 = g[0], m = g[1];
      const Nodes full(n0 + m);
      Jobs jobs(rng, ncls, n0);
      CHECK(full.rows(0, n0).upsert(h) == 0 && jobs.set(h) == 0 && stats(h, 0, 0, 0, 0, 0));
      int pre = 0; roundOf(h, jobs, &pre);   // (the append finds a handle that has run a round)
      CHECK(full.rows(n0, n0 + m).append(h) == 0);
      const int stride = (n0 + m + 63) / 64 != (n0 + 63) / 64;
      if (n0 == 130 && m <= 126) CHECK(stats(h, m, stride, 0, 0, n0 + m));
      if (n0 == 130 && m == 127) CHECK(stats(h, m, stride, 1, 5, n0 + m));
      char what[64]; snprintf(what, sizeof what, "%d classes, %3d + %3d rows", ncls, n0, m);
      compare(h, f, full, jobs, what);
    }
    { // appends on top of each other, without an upload in between; then the runs on new rows are told with jobs_patch
      const Nodes full(N0 + 70);
      Jobs jobs(rng, ncls, N0);
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      int at = N0;
      for (int m : {2, 0, 63, 5}) {
        CHECK(full.rows(at, at + m).append(h) == 0 && stats(h, m, m == 63, 0, 0, at + m));
        at += m;
        char what[64]; snprintf(what, sizeof what, "%d classes, %d more rows", ncls, m);
        compare(h, f, full.rows(0, at), jobs, what);
      }
      int32_t job[2] = {0, 1}, node[2] = {N0 + 1, at - 1}, pr[2] = {pcPrio[jobs.pc[0]], pcPrio[jobs.pc[1]]}; int64_t ts[2] = {1000000000ll, 2000000000ll};
      CHECK(asched_jobs_patch(h, 2, job, node, pr, ts) == 0);
      for (int k = 0; k < 2; k++) { jobs.node[job[k]] = node[k]; jobs.prio[job[k]] = pr[k]; jobs.ts[job[k]] = ts[k]; }
      compare(h, f, full.rows(0, at), jobs, "  and two runs patched onto new rows");
    }
    { // the returning nodes: rows 60..70 leave and join again with their old indices
      const Nodes full;
      Jobs jobs(rng, ncls, N0);
      CHECK(full.upsert(h) == 0 && jobs.set(h) == 0);
      std::vector<int32_t> on = jobs.unbind(60, 71), minus(on.size(), -1), zero(on.size(), 0), rows, map(N0); std::vector<int64_t> zts(on.size(), 0);
      if (!on.empty()) CHECK(asched_jobs_patch(h, (int32_t)on.size(), on.data(), minus.data(), zero.data(), zts.data()) == 0);
      for (int i = 60; i <= 70; i++) rows.push_back(i);
      CHECK(asched_nodes_delete(h, 11, rows.data(), map.data()) == 0);
      for (int j = 0; j < M; j++) if (jobs.node[j] >= 0) jobs.node[j] = map[jobs.node[j]];
      CHECK(full.rows(60, 71).append(h) == 0 && stats(h, 11, 1, 0, 0, N0));
      Nodes back = full.rows(0, 60); back.add(full.rows(71, N0)); back.add(full.rows(60, 71));
      compare(h, f, back, jobs, "rows 60..70 deleted and appended again");
    }
    { // the rebuild reasons that can be reached (5 is among the counts above), then the device path again
      for (int why : {1, 4, 3, 30}) {
        Nodes full(N0 + 3 + 8);
        if (why == 1) full.taints[N0 + 1] = {{7, 2, 1}};            // another value of the indexed taint
        if (why == 4) full.lVal[N0 + 1] = 9;                         // a new value of the indexed label
        if (why == 3) full.total[(size_t)(N0 + 1) * R] = full.alloc[(size_t)(N0 + 1) * R] = 128 * GI;   // beyond the widths of the key
        if (why == 30) { full.alloc = full.total; full.alloc[(size_t)(N0 + 1) * R + 1] -= 137; }          // the resident rows on the index grid, one new row off it
        Jobs jobs(rng, ncls, N0);
        CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
        CHECK(full.rows(N0, N0 + 3).append(h) == 0 && stats(h, 3, 0, 1, why == 30 ? 3 : why, N0 + 3));
        char what[64]; snprintf(what, sizeof what, "%d classes, rebuild reason %d", ncls, why == 30 ? 3 : why);
        compare(h, f, full.rows(0, N0 + 3), jobs, what);
        CHECK(full.rows(N0 + 3, N0 + 11).append(h) == 0 && stats(h, 8, 0, 0, 0, N0 + 11));
        compare(h, f, full, jobs, "  the device path after the rebuild");
      }
      // id order == index order: ranks in index order, then one new row whose id sorts first (reason 3); without id ranks the new rows sort behind every resident one
      Nodes full(N0 + 5);
      full.alloc = full.total;
      { std::vector<int> ord(full.n()); for (int i = 0; i < full.n(); i++) ord[i] = i;
        std::sort(ord.begin(), ord.end(), [&](int a, int b) { return full.index[a] < full.index[b]; });
        for (int i = 0; i < full.n(); i++) full.rank[ord[i]] = 2 * i; }
      Jobs jobs(rng, ncls, N0);
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(full.rows(N0, N0 + 5).append(h) == 0 && stats(h, 5, 0, 0, 0, N0 + 5));
      compare(h, f, full, jobs, "id ranks between the neighbours'");
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      Nodes broken = full; broken.rank[N0 + 2] = -5;
      CHECK(broken.rows(N0, N0 + 5).append(h) == 0 && stats(h, 5, 0, 1, 3, N0 + 5));
      compare(h, f, broken, jobs, "an id rank that breaks id order == index order");
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      int32_t top = 0; for (int i = 0; i < N0; i++) top = std::max(top, full.rank[i]);
      Nodes behind = full; for (int i = N0; i < N0 + 5; i++) behind.rank[i] = top + 1 + (i - N0);
      CHECK(full.rows(N0, N0 + 5).append(h, false) == 0 && stats(h, 5, 0, 1, 3, N0 + 5));
      compare(h, f, behind, jobs, "no id ranks: behind every resident one");
      // id_rank_all: every rank replaced
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      Nodes all = full; for (int i = 0; i < all.n(); i++) all.rank[i] = full.rank[i] / 2 + 7;
      { Nodes tail = full.rows(N0, N0 + 5); Nodes::Csr cs = tail.csr(); std::vector<int32_t> lv = tail.lVal; lv.push_back(0);
        asched_nodes_append_rows a; memset(&a, 0, sizeof a);
        a.m = 5; a.index = tail.index.data(); a.id_rank_all = all.rank.data(); a.total = tail.total.data(); a.allocatable = tail.alloc.data(); a.unschedulable = tail.uns.data();
        a.taint_off = cs.tOff.data(); a.taint_key = cs.tKey.data(); a.taint_value = cs.tVal.data(); a.taint_effect = cs.tEff.data();
        a.label_off = cs.lOff.data(); a.label_key = cs.lKey.data(); a.label_value = lv.data();
        CHECK(asched_nodes_append(h, &a) == 0 && stats(h, 5, 0, 0, 0, N0 + 5)); }
      compare(h, f, all, jobs, "id_rank_all");
    }
    { // a table uploaded without id ranks: appends without ranks (device path and rebuild), id_rank alone refused, id_rank_all accepted
      Nodes full(N0 + 9); full.ranked = false; full.alloc = full.total;
      Jobs jobs(rng, ncls, N0);
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(full.rows(N0, N0 + 4).append(h, true) == ASCHED_ERR_INVALID);
      compare(h, f, full.rows(0, N0), jobs, "no id ranks: id_rank alone is refused");
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(full.rows(N0, N0 + 4).append(h, false) == 0 && stats(h, 4, 0, 0, 0, N0 + 4));
      compare(h, f, full.rows(0, N0 + 4), jobs, "no id ranks: an append without ranks");
      Nodes other = full; other.lVal[N0 + 5] = 9;
      CHECK(other.rows(N0 + 4, N0 + 9).append(h, false) == 0 && stats(h, 5, 0, 1, 4, N0 + 9));
      compare(h, f, other, jobs, "no id ranks: the rebuild path without ranks");
    }
    { // jobs_delete of a row of the job table, then the append, then the row comes back with jobs_append (the table compared is the M-row one again)
      const Nodes full(N0 + 7);
      Jobs jobs(rng, ncls, N0);
      jobs.node[M - 1] = -1; jobs.prio[M - 1] = 0; jobs.ts[M - 1] = 0;   // (the last row is queued)
      CHECK(full.rows(0, N0).upsert(h) == 0 && jobs.set(h) == 0);
      int32_t gone = M - 1; std::vector<int32_t> map(M);
      CHECK(asched_jobs_delete(h, 1, &gone, map.data()) == 0 && map[M - 1] == -1 && map[M - 2] == M - 2);
      CHECK(full.rows(N0, N0 + 7).append(h) == 0 && stats(h, 7, 0, 0, 0, N0 + 7));
      asched_jobs jb; memset(&jb, 0, sizeof jb);
      jb.m = 1; jb.queue = &jobs.queue[M - 1]; jb.pc = &jobs.pc[M - 1]; jb.req = &jobs.req[(size_t)(M - 1) * R]; jb.req_class = &jobs.cls[M - 1];
      CHECK(asched_jobs_append(h, &jb) == 0);
      compare(h, f, full, jobs, "jobs_delete, nodes_append, jobs_append");
    }
    { // refusals: the handle stays as it was
      const Nodes full(N0 + 2);
      const Nodes head = full.rows(0, N0), tail = full.rows(N0, N0 + 2);
      Jobs jobs(rng, ncls, N0);
      CHECK(head.upsert(h) == 0 && jobs.set(h) == 0);
      Nodes::Csr cs = tail.csr();
      asched_nodes_append_rows ok; memset(&ok, 0, sizeof ok);
      ok.m = 2; ok.index = tail.index.data(); ok.total = tail.total.data(); ok.allocatable = tail.alloc.data();
      asched_nodes_append_rows a = ok;
      a.m = -1; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      a = ok; a.index = nullptr; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      a = ok; a.total = nullptr; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      a = ok; a.allocatable = nullptr; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      uint64_t resident[2] = {tail.index[0], head.index[17]}, twice[2] = {tail.index[0], tail.index[0]};
      a = ok; a.index = resident; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      a = ok; a.index = twice; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      int32_t badOff[3] = {0, 2, 1}, z[4] = {0, 0, 0, 0};
      a = ok; a.taint_off = badOff; a.taint_key = a.taint_value = a.taint_effect = z; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      a = ok; a.label_off = badOff; a.label_key = a.label_value = z; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_INVALID);
      int64_t huge[R] = {1ll << 58, 1ll << 58, 0, 1ll << 58};
      a = ok; a.m = 1; a.total = a.allocatable = huge; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_UNSUPPORTED);   // the rebuild would refuse: a key beyond 128 bits
      a = ok; a.m = (1 << 30) - N0 + 1; CHECK(asched_nodes_append(h, &a) == ASCHED_ERR_UNSUPPORTED);                 // N + m above 2^30: decided before any array is read
      CHECK(asched_nodes_append(h, nullptr) == ASCHED_ERR_INVALID && asched_nodes_append(nullptr, &ok) == ASCHED_ERR_INVALID);
      compare(h, f, head, jobs, "after the refusals");
      CHECK(head.upsert(h) == 0 && jobs.set(h) == 0 && tail.append(h) == 0 && stats(h, 2, 0, 0, 0, N0 + 2));
      compare(h, f, full, jobs, "and the same rows, accepted");
    }
    asched_destroy(h); asched_destroy(f);
  }
  { // a table of several workgroups: 2 x 4096 + 517 resident rows
    asched_t* h = create(c); asched_t* f = create(c);
    const int NB = 2 * 4096 + 517;
    for (int m : {1, 700}) {
      const Nodes full(NB + m);
      Jobs jobs(rng, 4, NB);
      CHECK(full.rows(0, NB).upsert(h) == 0 && jobs.set(h) == 0);
      CHECK(full.rows(NB, NB + m).append(h) == 0 && stats(h, m, -1, 0, 0, NB + m));
      char what[64]; snprintf(what, sizeof what, "%d nodes + %3d rows", NB, m);
      compare(h, f, full, jobs, what);
    }
    asched_destroy(h); asched_destroy(f);
  }
  { // tables nodes_append does not serve
    asched_t* h = create(c);
    const Nodes full(N0 + 1);
    const Nodes t = full.rows(0, N0), one = full.rows(N0, N0 + 1);
    const int N = t.n();
    std::vector<int64_t> ov(N, 1), abp;
    const int P = 2 + 3;
    for (int i = 0; i < N; i++) for (int l = 0; l < P; l++) for (int r = 0; r < R; r++) abp.push_back(t.total[(size_t)i * R + r]);
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = N; nd.index = t.index.data(); nd.id_rank = t.rank.data(); nd.total = t.total.data(); nd.allocatable = t.alloc.data();
    nd.node_type_override = ov.data();
    CHECK(asched_nodes_upsert(h, &nd) == 0 && one.append(h) == ASCHED_ERR_UNSUPPORTED);
    nd.node_type_override = nullptr; nd.alloc_by_prio = abp.data();
    CHECK(asched_nodes_upsert(h, &nd) == 0 && one.append(h) == ASCHED_ERR_UNSUPPORTED);
    nd.alloc_by_prio = nullptr;
    CHECK(asched_nodes_upsert(h, &nd) == 0 && asched_num_nodes(h) == N);
    asched_destroy(h);
  }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("nodes_append under ASan + UBSan: all appends ok\n");
  return 0;
}
