// asched_nodes_patch (asched_host.inc + kernels_nodes_patch.h) of the CPU build of the device code, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: patches of the entry counts of tests/test_z_nodes_patch.py (a) on one handle, one after the other (the device path), the three reasons
// for the rebuild path, a table with 65 requirement classes (two words of class bits per entry, no node class word), a patch before any job table, and every refusal
// — after each accepted patch every job's first fit at every priority, the totals and a round are compared with a second handle that was given the patched table by
// asched_nodes_upsert.  In the CPU build the "device" arrays are heap blocks: a mask word or a node column written out of bounds shows up here as a heap overflow.
// Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/nodes_patch_sanitize tools/nodes_patch_sanitize.cpp && /tmp/nodes_patch_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4, Q = 3, N = 130, M = 500;
static const int32_t pcPrio[3] = {0, 1, 3};
static const int64_t GI = 1ll << 30, MI128 = 128ll << 20;

struct Nodes {   // the node table as asched_nodes_upsert is given it
  std::vector<uint64_t> index; std::vector<int32_t> rank, lOff, lKey, lVal; std::vector<int64_t> total, alloc; std::vector<uint8_t> uns, over;
  std::vector<std::vector<std::array<int32_t, 3>>> taints;
  Nodes() {
    for (int i = 0; i < N; i++) {
      index.push_back(i + 1); rank.push_back(i); lOff.push_back(i); lKey.push_back(3); lVal.push_back(i % 2);
      const int64_t t[R] = {64 * GI, 16000, 512 * GI, i % 9 == 0 ? 4 : 0};
      total.insert(total.end(), t, t + R);
      uns.push_back(i % 7 == 3); over.push_back(0);
      taints.push_back({});
      if (i % 5 == 0) taints.back().push_back({7, 1, 1});
    }
    lOff.push_back(N);
    alloc = total;
  }
  int upsert(asched_t* h) const {
    std::vector<int32_t> tOff(1, 0), tKey, tVal, tEff;
    for (auto& tv : taints) { for (auto& x : tv) { tKey.push_back(x[0]); tVal.push_back(x[1]); tEff.push_back(x[2]); } tOff.push_back((int32_t)tKey.size()); }
    tKey.push_back(0); tVal.push_back(0); tEff.push_back(0);
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = alloc.data(); nd.unschedulable = uns.data(); nd.over_allocated = over.data();
    nd.taint_off = tOff.data(); nd.taint_key = tKey.data(); nd.taint_value = tVal.data(); nd.taint_effect = tEff.data();
    nd.label_off = lOff.data(); nd.label_key = lKey.data(); nd.label_value = lVal.data();
    return asched_nodes_upsert(h, &nd);
  }
};

struct Patch {
  std::vector<int32_t> node; std::vector<int64_t> alloc; std::vector<uint8_t> uns, over; std::vector<std::vector<std::array<int32_t, 3>>> taints;
  bool hasAlloc = false, hasUns = false, hasOver = false, hasTaints = false;
  int apply(asched_t* h, Nodes* t) const {   // t: the restatement follows an accepted patch
    std::vector<int32_t> tOff(1, 0), tKey, tVal, tEff;
    for (auto& tv : taints) { for (auto& x : tv) { tKey.push_back(x[0]); tVal.push_back(x[1]); tEff.push_back(x[2]); } tOff.push_back((int32_t)tKey.size()); }
    tKey.push_back(0); tVal.push_back(0); tEff.push_back(0);
    asched_nodes_patch_rows p; memset(&p, 0, sizeof p);
    p.n = (int32_t)node.size(); p.node = node.data();
    if (hasAlloc) p.allocatable = alloc.data();
    if (hasUns) p.unschedulable = uns.data();
    if (hasOver) p.over_allocated = over.data();
    if (hasTaints) { p.taint_off = tOff.data(); p.taint_key = tKey.data(); p.taint_value = tVal.data(); p.taint_effect = tEff.data(); }
    int rc = asched_nodes_patch(h, &p);
    if (rc == 0 && t)
      for (size_t i = 0; i < node.size(); i++) {
        const int v = node[i];
        if (hasAlloc) for (int r = 0; r < R; r++) t->alloc[(size_t)v * R + r] = alloc[i * R + r];
        if (hasUns) t->uns[v] = uns[i];
        if (hasOver) t->over[v] = over[i];
        if (hasTaints) t->taints[v] = taints[i];
      }
    return rc;
  }
};

struct Jobs {
  std::vector<int32_t> queue, pc, cls; std::vector<int64_t> req; int ncls;
  Jobs(std::mt19937& rng, int ncls_) : ncls(ncls_) {
    for (int j = 0; j < M; j++) {
      queue.push_back((int)(rng() % Q)); pc.push_back((int)(rng() % 3)); cls.push_back((int)(rng() % ncls));
      const int64_t q[R] = {(int64_t)(4 << (rng() % 4)) * GI, (int64_t)(1000 << (rng() % 4)), 0, rng() % 10 == 0 ? 1 : 0};
      req.insert(req.end(), q, q + R);
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
    return asched_jobs_set(h, &jb, &rc);
  }
};

static int roundOf(asched_t* h, const Jobs& t, int* preempted) {
  std::vector<double> weight(Q, 1.0), qTok(Q, 1e18); std::vector<int64_t> qBurst(Q, 1ll << 62); std::vector<uint8_t> qInf(Q, 1); std::vector<int32_t> qOff(Q + 1, 0), queued;
  for (int q = 0; q < Q; q++) {
    for (int p = 2; p >= 0; p--) for (int j = 0; j < M; j++) if (t.queue[j] == q && t.pc[j] == p) queued.push_back(j);   // priority-class priority descending, then the row
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
  return (int)(sum & 0x7fffffffu);
}

// the patched handle against a handle that is given the restated table by nodes_upsert
static void compare(asched_t* h, asched_t* f, const Nodes& t, const Jobs& jobs, const char* what) {
  CHECK(t.upsert(f) == 0);
  std::vector<int32_t> ids(M), a(M), b(M), prios(ASCHED_MAX_PRIORITIES);
  for (int j = 0; j < M; j++) ids[j] = j;
  const int P = asched_priorities(h, prios.data());
  for (int l = 0; l < P; l++) {
    CHECK(asched_fit_select_batch(h, M, ids.data(), prios[l], a.data()) == 0 && asched_fit_select_batch(f, M, ids.data(), prios[l], b.data()) == 0);
    CHECK(a == b);
  }
  int64_t ta[R], tb[R];
  CHECK(asched_total_resources(h, ta) == 0 && asched_total_resources(f, tb) == 0 && std::equal(ta, ta + R, tb));
  for (int j = 0; j < M; j += 50) {
    int32_t x[2], y[2];
    CHECK(asched_node_types_matching_job(h, j, &x[0], &x[1]) == 0 && asched_node_types_matching_job(f, j, &y[0], &y[1]) == 0 && x[0] == y[0] && x[1] == y[1]);
  }
  int pa = 0, pb = 0;
  const int ra = roundOf(h, jobs, &pa), rb = roundOf(f, jobs, &pb);
  CHECK(ra == rb && pa == pb);
  printf("%s: as nodes_upsert of the patched table (round checksum %d)\n", what, ra);
}

static std::vector<int32_t> rowsOf(std::mt19937& rng, int n) {
  std::vector<int32_t> rows = {0, 63, 64, 127, 128, 129}, rest;
  for (int i = 0; i < N; i++) if (std::find(rows.begin(), rows.end(), i) == rows.end() && (n == N || (i != 80 && i != 115))) rest.push_back(i);
  std::shuffle(rest.begin(), rest.end(), rng);
  rows.insert(rows.end(), rest.begin(), rest.end());
  rows.resize(n);
  return rows;
}

// a patch of all four fields that keeps every node type populated and allocatable on the index grid
static Patch devicePatch(std::mt19937& rng, const Nodes& t, const std::vector<int32_t>& rows) {
  Patch p; p.node = rows; p.hasAlloc = p.hasUns = p.hasOver = p.hasTaints = true;
  const bool all = (int)rows.size() == N;
  for (int v : rows) {
    const int src = (v + 2) % N;   // all rows: the state of the next row but one, which has this row's label
    p.uns.push_back(all ? t.uns[src] : !t.uns[v]); p.over.push_back(rng() % 2);
    p.taints.push_back(all ? t.taints[src] : t.taints[v].empty() ? std::vector<std::array<int32_t, 3>>{{7, 1, 1}} : std::vector<std::array<int32_t, 3>>{});
    p.alloc.push_back(t.total[(size_t)v * R] - (int64_t)(rng() % 100) * MI128); p.alloc.push_back(t.total[(size_t)v * R + 1] - (int64_t)(rng() % 9) * 1000);
    p.alloc.push_back(t.total[(size_t)v * R + 2]); p.alloc.push_back(t.total[(size_t)v * R + 3]);
  }
  return p;
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
    Nodes t; Jobs jobs(rng, ncls);
    { Patch p; p.node = {0}; p.hasUns = true; p.uns = {1}; CHECK(p.apply(h, nullptr) == ASCHED_ERR_INVALID); }   // no node table
    CHECK(t.upsert(h) == 0);
    { Patch p = devicePatch(rng, t, rowsOf(rng, 5));   // before any job table: node arrays and mirrors only
      CHECK(p.apply(h, &t) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[0] == 5 && st[2] == 0); }
    CHECK(jobs.set(h) == 0 && jobs.set(f) == 0);
    compare(h, f, t, jobs, "a patch before the job table");
    t = Nodes();
    CHECK(t.upsert(h) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[0] == 0);
    static const int counts[] = {0, 1, 2, 63, 64, 65, 130};
    for (int n : counts) {   // the device path, every patch on what the one before it left
      Nodes base; t = base;
      CHECK(t.upsert(h) == 0);
      int pre = 0; roundOf(h, jobs, &pre);   // (the patch finds a handle that has run a round)
      Patch p = devicePatch(rng, t, rowsOf(rng, n));
      CHECK(p.apply(h, &t) == 0);
      CHECK(asched_nodes_patch_stats(h, st) == 0 && st[0] == n && st[2] == 0 && st[3] == 0 && (n == 0 || st[1] > 0));
      char what[64]; snprintf(what, sizeof what, "%d classes, %3d entries", ncls, n);
      compare(h, f, t, jobs, what);
      Patch q; q.node = p.node; q.hasAlloc = true;   // and one field alone on top of it
      for (int v : q.node) for (int r = 0; r < R; r++) q.alloc.push_back(t.total[(size_t)v * R + r]);
      CHECK(q.apply(h, &t) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[1] == 0 && st[2] == 0);
      compare(h, f, t, jobs, what);
    }
    { // the rebuild path: a taint set never seen; a type emptied; a value beyond the key layout; then the device path again
      Nodes base; t = base;
      CHECK(t.upsert(h) == 0);
      Patch p; p.node = {5, 64}; p.hasTaints = true; p.taints = {{{11, 5, 1}}, {{7, 1, 1}, {11, 5, 1}}};
      CHECK(p.apply(h, &t) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[2] == 1 && st[3] == 1);
      compare(h, f, t, jobs, "rebuild: a taint set never seen");
      Patch e; e.node = {10, 80}; e.hasTaints = true; e.taints = {{}, {}};
      CHECK(e.apply(h, &t) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[2] == 1 && st[3] == 2);
      compare(h, f, t, jobs, "rebuild: a node type emptied");
      Patch b; b.node = {3, 129}; b.hasAlloc = true;
      for (int v : b.node) { b.alloc.push_back(t.total[(size_t)v * R]); b.alloc.push_back(32000); b.alloc.push_back(t.total[(size_t)v * R + 2]); b.alloc.push_back(t.total[(size_t)v * R + 3]); }
      CHECK(b.apply(h, &t) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[2] == 1 && st[3] == 3);
      compare(h, f, t, jobs, "rebuild: an allocatable above the key layout");
      Patch u; u.node = {3, 129, 7}; u.hasAlloc = true;   // off the index grid: every resident value is on it
      for (int v : u.node) { u.alloc.push_back(t.total[(size_t)v * R] - 12345); u.alloc.push_back(15863); u.alloc.push_back(t.total[(size_t)v * R + 2]); u.alloc.push_back(t.total[(size_t)v * R + 3]); }
      CHECK(u.apply(h, &t) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[2] == 1 && st[3] == 3);
      compare(h, f, t, jobs, "rebuild: an allocatable off the index grid");
      Patch d; d.node = {1, 2, 66}; d.hasUns = true; d.uns = {1, 1, 1}; d.hasOver = true; d.over = {1, 0, 1};
      CHECK(d.apply(h, &t) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[2] == 0);
      compare(h, f, t, jobs, "the device path after the rebuilds");
    }
    { // refusals: the handle stays as it was
      const Nodes before = t;
      Patch p; p.hasUns = true;
      p.node = {0, N}; p.uns = {1, 1}; CHECK(p.apply(h, nullptr) == ASCHED_ERR_INVALID);
      p.node = {-1}; p.uns = {1}; CHECK(p.apply(h, nullptr) == ASCHED_ERR_INVALID);
      p.node = {3, 7, 3}; p.uns = {1, 1, 1}; CHECK(p.apply(h, nullptr) == ASCHED_ERR_INVALID);
      asched_nodes_patch_rows raw; memset(&raw, 0, sizeof raw);
      int32_t two[2] = {0, 1}, badOff[3] = {0, 2, 1}, zeros[4] = {0, 0, 0, 0};
      raw.n = -1; raw.node = two; CHECK(asched_nodes_patch(h, &raw) == ASCHED_ERR_INVALID);
      raw.n = 2; raw.node = nullptr; CHECK(asched_nodes_patch(h, &raw) == ASCHED_ERR_INVALID);
      raw.node = two; raw.taint_off = badOff; raw.taint_key = raw.taint_value = raw.taint_effect = zeros; CHECK(asched_nodes_patch(h, &raw) == ASCHED_ERR_INVALID);
      CHECK(asched_nodes_patch(h, nullptr) == ASCHED_ERR_INVALID);
      Patch huge; huge.node = {2}; huge.hasAlloc = true; huge.alloc = {1ll << 58, 1ll << 58, 0, 1ll << 58};   // the rebuild would refuse: an order key beyond 128 bits
      CHECK(huge.apply(h, nullptr) == ASCHED_ERR_UNSUPPORTED);
      int pa = 0, pb = 0;   // (the handle still holds the round of the last comparison: the same round again, then the resets of an empty patch and every answer)
      CHECK(before.upsert(f) == 0);
      const int ra = roundOf(h, jobs, &pa), rb = roundOf(f, jobs, &pb);
      CHECK(ra == rb && pa == pb);
      Patch none; CHECK(none.apply(h, nullptr) == 0 && asched_nodes_patch_stats(h, st) == 0 && st[0] == 0 && st[2] == 0);
      compare(h, f, before, jobs, "after the refusals");
    }
    asched_destroy(h); asched_destroy(f);
  }
  { // tables nodes_patch does not serve
    asched_t* h = create(c);
    Nodes t;
    std::vector<int64_t> ov(N, 1), abp;
    const int P = 2 + 3;
    for (int i = 0; i < N; i++) for (int l = 0; l < P; l++) for (int r = 0; r < R; r++) abp.push_back(t.total[(size_t)i * R + r]);
    Patch p; p.node = {0}; p.hasUns = true; p.uns = {1};
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = N; nd.index = t.index.data(); nd.id_rank = t.rank.data(); nd.total = t.total.data(); nd.allocatable = t.alloc.data();
    nd.node_type_override = ov.data();
    CHECK(asched_nodes_upsert(h, &nd) == 0 && p.apply(h, nullptr) == ASCHED_ERR_UNSUPPORTED);
    nd.node_type_override = nullptr; nd.alloc_by_prio = abp.data();
    CHECK(asched_nodes_upsert(h, &nd) == 0 && p.apply(h, nullptr) == ASCHED_ERR_UNSUPPORTED);
    nd.alloc_by_prio = nullptr;
    CHECK(asched_nodes_upsert(h, &nd) == 0 && p.apply(h, nullptr) == 0);
    asched_destroy(h);
  }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("nodes_patch under ASan + UBSan: all patches ok\n");
  return 0;
}
