// asched_shapes_compact (asched_host.inc + kernels_shapes_compact.h) of the CPU build of the device code, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer, built with room for 8 entries of each map in the staging arrays of the row pass (-DSC_LDS_CAP=8): tables of 7 / 8 / 9 shapes sit on
// both sides of that capacity, the larger ones take the global branch.  Sequences on node tables of 1 .. 320 rows (the word edges of the gathers), with and without
// away node types: new shapes appended in place / deleted / compact / the retired shapes appended again (new once more) / deleted / compact with class retirement,
// then jobs_patch, jobs_delete, nodes_patch and a class append on the compacted handle — every step compared with a fresh handle that was given jobs_set of the
// same table and the reduced class list (every row's first fit at every priority level, the node types matching the last rows).  In the CPU build the "device" arrays
// are heap blocks: a mask block, a small table or a record array the call sized wrongly shows up here as a heap overflow.  Test infrastructure; nothing here is
// linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -DSC_LDS_CAP=8 -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/shapes_compact_sanitize tools/shapes_compact_sanitize.cpp && /tmp/shapes_compact_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4;
static const int32_t pcPrio[3] = {0, 1, 3};

struct Nodes {
  int N = 0;
  std::vector<uint64_t> index; std::vector<int32_t> rank, tOff, tKey, tVal, tEff, lOff, lKey, lVal; std::vector<int64_t> total, alloc;
  void add(int i) {   // node number i: two node types by an indexed label, the odd ones with twice the memory; every fourth carries the well-known type's taint
    index.push_back((uint64_t)i + 1); rank.push_back(i);
    const int64_t row[R] = {(i % 2 ? 128ll : 64ll) << 30, 16000, 512ll << 30, 0};
    total.insert(total.end(), row, row + R); alloc.insert(alloc.end(), row, row + R);
    if (tOff.empty()) { tOff.push_back(0); lOff.push_back(0); }
    if (i % 4 == 0) { tKey.push_back(7); tVal.push_back(1); tEff.push_back(1); }
    tOff.push_back((int32_t)tKey.size());
    lKey.push_back(3); lVal.push_back(i % 2); lOff.push_back((int32_t)lKey.size());
    N++;
  }
  int upsert(asched_t* h) const {
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = alloc.data();
    nd.taint_off = tOff.data(); nd.taint_key = tKey.data(); nd.taint_value = tVal.data(); nd.taint_effect = tEff.data();
    nd.label_off = lOff.data(); nd.label_key = lKey.data(); nd.label_value = lVal.data();
    return asched_nodes_upsert(h, &nd);
  }
};

// the requirement classes: odd ones select the odd nodes.  nClasses of them are given to jobs_set
static int setClasses(asched_t* h, const asched_jobs& jb, int nClasses) {
  std::vector<int32_t> tolOff(nClasses + 1, 0), selOff(1, 0), selKey, selVal;
  for (int c = 0; c < nClasses; c++) { if (c % 2) { selKey.push_back(3); selVal.push_back(1); } selOff.push_back((int32_t)selKey.size()); }
  asched_req_classes rc; memset(&rc, 0, sizeof rc);
  rc.n = nClasses; rc.tol_off = tolOff.data(); rc.sel_off = selOff.data(); rc.sel_key = selKey.data(); rc.sel_value = selVal.data();
  return asched_jobs_set(h, &jb, &rc);
}

struct Table {
  int M = 0;
  std::vector<int32_t> queue, pc, cls; std::vector<int64_t> req, submit;
  void row(int q, int p, int c, int64_t mem, int64_t cpu, int64_t eph) {
    queue.push_back(q); pc.push_back(p); cls.push_back(c); submit.push_back(M);
    req.push_back(mem); req.push_back(cpu); req.push_back(eph); req.push_back(0);
    M++;
  }
  void base(std::mt19937& rng, int m, int shapes) {   // m rows over at most `shapes` shapes; requirement class 2 only ever in priority class 0 (no derived away class of it)
    for (int i = 0; i < m; i++) {
      const int k = (int)(rng() % shapes), c = k % 3, p = c == 2 ? 0 : (k / 3) % 3;
      row((int)(rng() % 3), p, c, (4ll << 30) * (1 + k % 3), 1000 * (1 + k % 4), (10ll << 30) * (1 + k / 12));
    }
  }
  void fresh(int k, int p, int c, int salt) { for (int i = 0; i < k; i++) row(i % 3, p, c, 2ll << 30, 1000, (300ll + salt + i) << 30); }   // k rows of k shapes no base table has
  asched_jobs view(int from, int m) const {
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = m; jb.queue = queue.data() + from; jb.pc = pc.data() + from; jb.submit_time = submit.data() + from; jb.req = req.data() + (size_t)from * R; jb.req_class = cls.data() + from;
    return jb;
  }
  int set(asched_t* h, int nClasses) const { return setClasses(h, view(0, M), nClasses); }
  int append(asched_t* h, int from) const { asched_jobs jb = view(from, M - from); return asched_jobs_append(h, &jb); }
  void truncate(int m) { M = m; queue.resize(m); pc.resize(m); cls.resize(m); submit.resize(m); req.resize((size_t)m * R); }
  int shapes() const { std::set<std::vector<int64_t>> s; for (int j = 0; j < M; j++) s.insert({cls[j], pc[j], req[(size_t)j * R], req[(size_t)j * R + 1], req[(size_t)j * R + 2]}); return (int)s.size(); }
};

static asched_t* create(bool away) {
  static const int32_t indexedCol[3] = {1, 0, 3}, labelKey[1] = {3};
  static const int64_t indexedRes[3] = {1000, 128ll << 20, 1};
  static const uint8_t pcPre[3] = {1, 1, 0};
  static const double drf[4] = {1.0, 1.0, 0.0, 1.0};
  static const int32_t awayOff[4] = {0, 0, 1, 3}, awayPrio[3] = {0, 2, 1}, awayWkt[3] = {0, 1, 0};   // pc 1 away at priority 0; pc 2 away at 2, then at 1
  static const int32_t wktOff[3] = {0, 1, 2}, wktKey[2] = {7, 7}, wktVal[2] = {1, -1}, wktEff[2] = {1, 1};
  asched_config c; memset(&c, 0, sizeof c);
  c.num_resources = R; c.num_indexed = 3; c.indexed_col = indexedCol; c.indexed_resolution = indexedRes;
  c.num_priority_classes = 3; c.pc_priority = pcPrio; c.pc_preemptible = pcPre; c.drf_multiplier = drf; c.device = -1;
  c.num_indexed_labels = 1; c.indexed_label_keys = labelKey;
  if (away) { c.pc_away_off = awayOff; c.away_priority = awayPrio; c.away_well_known = awayWkt; c.num_well_known_types = 2; c.wkt_taint_off = wktOff; c.wkt_taint_key = wktKey; c.wkt_taint_value = wktVal; c.wkt_taint_effect = wktEff; }
  return asched_create(&c);
}

// every row's first fit at every priority level, on the handle and on a fresh handle of the same tables and nClasses classes
static void same(asched_t* h, bool away, const Nodes& nd, const Table& t, int nClasses, const char* what) {
  asched_t* f = create(away);
  CHECK(f && nd.upsert(f) == 0 && t.set(f, nClasses) == 0);
  if (!f) return;
  int32_t prios[ASCHED_MAX_PRIORITIES];
  const int P = asched_priorities(h, prios);
  std::vector<int32_t> jobs(t.M), a(t.M), b(t.M);
  for (int j = 0; j < t.M; j++) jobs[j] = j;
  for (int p = 0; p < P; p++) {
    CHECK(asched_fit_select_batch(h, t.M, jobs.data(), prios[p], a.data()) == 0);
    CHECK(asched_fit_select_batch(f, t.M, jobs.data(), prios[p], b.data()) == 0);
    CHECK(a == b);
    if (a != b) fprintf(stderr, "%s: the first fits at priority %d differ from a fresh handle's\n", what, prios[p]);
  }
  for (int j = std::max(0, t.M - 40); j < t.M; j++) {
    int32_t m1, e1, m2, e2;
    CHECK(asched_node_types_matching_job(h, j, &m1, &e1) == 0 && asched_node_types_matching_job(f, j, &m2, &e2) == 0 && m1 == m2 && e1 == e2);
  }
  asched_destroy(f);
}

// rows of new shapes appended in place and deleted again: the table is as it was, the shapes are dead
static void kill(asched_t* h, Table& t, int k, int p, int c, int salt) {
  const int before = t.M;
  t.fresh(k, p, c, salt);
  int32_t st[8], ds[8];
  CHECK(t.append(h, before) == 0 && asched_jobs_append_stats(h, st) == 0 && st[5] == 0 && st[2] == k);
  std::vector<int32_t> rows;
  for (int j = before; j < t.M; j++) rows.push_back(j);
  CHECK(asched_jobs_delete(h, k, rows.data(), nullptr) == 0 && asched_jobs_delete_stats(h, ds) == 0 && ds[3] == k);
  t.truncate(before);
}

static void compact(asched_t* h, int flags, int32_t* map, int shapes, int classes, int rebuilt, const char* what) {
  int32_t st[8];
  CHECK(asched_shapes_compact(h, flags | ASCHED_COMPACT_COUNT_ONLY, nullptr) == 0 && asched_shapes_compact_stats(h, st) == 0 && st[0] == shapes && st[2] == classes && st[4] == 0);
  CHECK(asched_shapes_compact(h, flags, map) == 0 && asched_shapes_compact_stats(h, st) == 0);
  CHECK(st[0] == shapes && st[2] == classes && st[4] == rebuilt);
  if (st[0] != shapes || st[2] != classes || st[4] != rebuilt) fprintf(stderr, "%s: shapes %d, fit %d, classes %d, rebuilt %d, reason %d\n", what, st[0], st[1], st[2], st[4], st[5]);
}

int main() {
  std::mt19937 rng(23);
  static const int sizes[] = {1, 63, 64, 65, 255, 256, 257, 320};
  for (int away = 0; away < 2; away++)
    for (int n : sizes) {
      Nodes nd;
      for (int i = 0; i < n; i++) nd.add(i);
      asched_t* h = create(away);
      CHECK(h != nullptr);
      if (!h) return 1;
      CHECK(asched_set_append_in_place(h, 1) == 0 && nd.upsert(h) == 0);
      Table t; t.base(rng, 150, 27);
      CHECK(t.set(h, 5) == 0);   // classes 3 and 4 have no rows
      kill(h, t, 5, away ? 1 : 0, 0, 0);
      kill(h, t, 3, away ? 2 : 1, 3, 50);    // (with away node types: class 3 derives away classes of its own, which die with these shapes)
      compact(h, 0, nullptr, 8, 0, 0, "first compact");
      same(h, away, nd, t, 5, "first compact");
      kill(h, t, 5, away ? 1 : 0, 0, 0);     // the retired shapes again: new once more
      kill(h, t, 2, 0, 4, 80);
      int32_t map[5] = {-2, -2, -2, -2, -2};
      compact(h, ASCHED_COMPACT_CLASSES, map, 7, 2, 0, "compact with classes");
      CHECK(map[0] == 0 && map[1] == 1 && map[2] == 2 && map[3] == -1 && map[4] == -1);
      same(h, away, nd, t, 3, "compact with classes");
      compact(h, ASCHED_COMPACT_CLASSES, nullptr, 0, 0, 0, "nothing dead");
      same(h, away, nd, t, 3, "nothing dead");
      asched_destroy(h);
      printf("%s %3d nodes: append / delete / compact / append again / compact with classes ok\n", away ? "away," : "      ", n);
    }
  for (int s0 : {7, 8, 9}) {   // the staging capacity of this build: live + dead shapes on both sides of it, job records included
    Nodes nd;
    for (int i = 0; i < 65; i++) nd.add(i);
    asched_t* h = create(false);
    CHECK(h != nullptr);
    if (!h) return 1;
    CHECK(asched_set_append_in_place(h, 1) == 0 && nd.upsert(h) == 0);
    Table t; t.base(rng, 300, 4);
    const int live = t.shapes();
    CHECK(live <= 4 && t.set(h, 3) == 0);
    kill(h, t, s0 - live, 0, 0, 0);
    compact(h, ASCHED_COMPACT_CLASSES, nullptr, s0 - live, 0, 0, "capacity edge");
    same(h, false, nd, t, 3, "capacity edge");
    asched_destroy(h);
    printf("       %d shapes around the staging capacity of 8 ok\n", s0);
  }
  { // the resident calls on a compacted handle, with away node types
    Nodes nd;
    for (int i = 0; i < 130; i++) nd.add(i);
    asched_t* h = create(true);
    CHECK(h != nullptr);
    if (!h) return 1;
    CHECK(asched_set_append_in_place(h, 1) == 0 && nd.upsert(h) == 0);
    Table t; t.base(rng, 200, 27);
    CHECK(t.set(h, 5) == 0);
    kill(h, t, 6, 1, 3, 0);
    kill(h, t, 6, 2, 0, 0);
    compact(h, ASCHED_COMPACT_CLASSES, nullptr, 12, 2, 0, "before the resident calls");
    same(h, true, nd, t, 3, "before the resident calls");
    { int before = t.M;   // a retired shape and a new one come in place
      t.fresh(2, 2, 0, 0); t.fresh(1, 1, 1, 700);
      int32_t st[8], sh[8];
      CHECK(t.append(h, before) == 0 && asched_jobs_append_stats(h, st) == 0 && asched_jobs_append_shape_stats(h, sh) == 0 && st[5] == 0 && sh[1] == 3 && sh[2] == 0 && sh[6] == 0);
      same(h, true, nd, t, 3, "append after the compact"); }
    { int32_t rows[2] = {t.M - 1, 3}, node[2] = {1, 1}, sap[2] = {pcPrio[t.pc[t.M - 1]], pcPrio[t.pc[3]]}; int64_t ts[2] = {5, 6};
      CHECK(asched_jobs_patch(h, 2, rows, node, sap, ts) == 0);
      int32_t back[2] = {-1, -1}, zero[2] = {0, 0}; int64_t z64[2] = {0, 0};
      CHECK(asched_jobs_patch(h, 2, rows, back, zero, z64) == 0);
      same(h, true, nd, t, 3, "after the patches"); }
    { int32_t rows[5] = {0, 63, 64, 65, 129}; std::vector<int64_t> al;
      for (int k = 0; k < 5; k++) { for (int r = 0; r < R; r++) al.push_back(nd.total[(size_t)rows[k] * R + r]); al[(size_t)k * R + 1] -= 3000; al[(size_t)k * R] -= 8ll << 30; }
      asched_nodes_patch_rows p; memset(&p, 0, sizeof p);
      p.n = 5; p.node = rows; p.allocatable = al.data();
      int32_t ps[8];
      CHECK(asched_nodes_patch(h, &p) == 0 && asched_nodes_patch_stats(h, ps) == 0 && ps[2] == 0);
      for (int k = 0; k < 5; k++) for (int r = 0; r < R; r++) nd.alloc[(size_t)rows[k] * R + r] = al[(size_t)k * R + r];
      same(h, true, nd, t, 3, "after nodes_patch"); }
    { // a class append behind the compacted classes (id 3: a class that selects the odd nodes), rows that name it, then all of it dies and is retired
      static const int32_t tolOff[2] = {0, 0}, selOff[2] = {0, 1}, selKey[1] = {3}, selVal[1] = {1};
      asched_req_classes rc; memset(&rc, 0, sizeof rc);
      rc.n = 1; rc.tol_off = tolOff; rc.sel_off = selOff; rc.sel_key = selKey; rc.sel_value = selVal;
      int32_t cs[8];
      CHECK(asched_req_classes_append(h, &rc) == 0 && asched_req_classes_append_stats(h, cs) == 0 && cs[6] == 4 && cs[4] == 0);
      kill(h, t, 3, 1, 3, 900);
      int32_t map[4] = {-2, -2, -2, -2};
      compact(h, ASCHED_COMPACT_CLASSES, map, 3, 1, 0, "a class that came and went");
      CHECK(map[0] == 0 && map[1] == 1 && map[2] == 2 && map[3] == -1);
      same(h, true, nd, t, 3, "a class that came and went"); }
    asched_destroy(h);
    printf("jobs_append, jobs_patch, nodes_patch, req_classes_append on a compacted handle ok\n");
  }
  { // more than SMAX fit shapes: the compact brings the fast structure back (the rebuild), and a handle without a node table takes the mirrors only
    Nodes nd;
    for (int i = 0; i < 65; i++) nd.add(i);
    asched_t* h = create(false);
    CHECK(h != nullptr);
    if (!h) return 1;
    CHECK(asched_set_append_in_place(h, 1) == 0 && nd.upsert(h) == 0);
    Table t; t.base(rng, 200, 27);
    CHECK(t.set(h, 3) == 0);
    for (int c = 0; c < 6; c++) {
      const int before = t.M;
      t.fresh(50, 0, 0, 50 * c);
      std::vector<int32_t> rows;
      for (int j = before; j < t.M; j++) rows.push_back(j);
      CHECK(t.append(h, before) == 0 && asched_jobs_delete(h, 50, rows.data(), nullptr) == 0);
      t.truncate(before);
    }
    int32_t st[8];
    CHECK(asched_shapes_compact(h, 0, nullptr) == 0 && asched_shapes_compact_stats(h, st) == 0 && st[0] == 300 && st[4] == 1 && st[5] == 2);
    same(h, false, nd, t, 3, "back under SMAX");
    asched_destroy(h);
    h = create(false);
    CHECK(h != nullptr);
    if (!h) return 1;
    const int before = t.M;
    t.fresh(9, 0, 0, 0);
    CHECK(t.set(h, 3) == 0);
    std::vector<int32_t> rows;
    for (int j = before; j < t.M; j++) rows.push_back(j);
    CHECK(asched_jobs_delete(h, 9, rows.data(), nullptr) == 0);
    t.truncate(before);
    CHECK(asched_shapes_compact(h, 0, nullptr) == 0 && asched_shapes_compact_stats(h, st) == 0 && st[0] == 9 && st[4] == 1 && st[5] == 1);
    CHECK(nd.upsert(h) == 0);
    same(h, false, nd, t, 3, "compact before the node table");
    asched_destroy(h);
    printf("the rebuild paths (F back under SMAX, no node table yet) ok\n");
  }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("shapes_compact under ASan + UBSan: all checks passed\n");
  return 0;
}
