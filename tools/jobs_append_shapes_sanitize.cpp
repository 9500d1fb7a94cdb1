// The in-place path of asched_jobs_append for new scheduling-key shapes (asched_set_append_in_place; asched_host.inc + kernels_shapes_append.h) of the CPU build of the
// device code, as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer: node tables of 1 .. 320 rows (the word and four-word edges of the mask
// pass), 1 / 2 / 5 / 64 / 65 new shapes in one call, priority classes with away node types (the old away rows move, derived classes are added), shapes revived after
// asched_jobs_delete emptied them, and jobs_patch / jobs_delete / nodes_patch / nodes_delete / nodes_append after an in-place append — every step compared with a fresh
// handle that was given jobs_set of the same table (every row's first fit at every priority level).  In the CPU build the "device" arrays are heap blocks: a mask
// block, a small shape table or a record array that the path did not grow shows up here as a heap overflow.  Test infrastructure; nothing here is linked into the
// product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/jobs_append_shapes_sanitize tools/jobs_append_shapes_sanitize.cpp && /tmp/jobs_append_shapes_sanitize
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

struct Table {
  int M = 0;
  std::vector<int32_t> queue, pc, cls; std::vector<int64_t> req, submit;
  void row(int q, int p, int c, int64_t mem, int64_t cpu, int64_t eph) {
    queue.push_back(q); pc.push_back(p); cls.push_back(c); submit.push_back(M);
    req.push_back(mem); req.push_back(cpu); req.push_back(eph); req.push_back(0);
    M++;
  }
  void base(std::mt19937& rng, int m) {   // shapes on a small grid; requirement class 2 only ever in priority class 0 (no derived away class of it)
    for (int i = 0; i < m; i++) {
      int c = (int)(rng() % 3), p = (int)(rng() % 3);
      if (c == 2) p = 0;
      row((int)(rng() % 3), p, c, (4ll << 30) * (1 + rng() % 3), 1000 * (1 + rng() % 4), (10ll << 30) * (1 + rng() % 2));
    }
  }
  void fresh(int k, int p, int c, int salt) {   // k rows of k shapes no base table has: the edge shapes first (none / all / one type / equal to an even node's total)
    for (int i = 0; i < k; i++) {
      if (i == 0) row(i % 3, p, c, 4ll << 30, 17000, 0);
      else if (i == 1) row(i % 3, p, c, 1ll << 30, 1000, 1ll << 30);
      else if (i == 2) row(i % 3, p, c, 100ll << 30, 2000, 3ll << 30);
      else if (i == 3) row(i % 3, p, c, 64ll << 30, 16000, 512ll << 30);
      else row(i % 3, p, c, 2ll << 30, 1000, (300ll + salt + i) << 30);
    }
  }
  asched_jobs view(int from, int m) const {
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = m; jb.queue = queue.data() + from; jb.pc = pc.data() + from; jb.submit_time = submit.data() + from; jb.req = req.data() + (size_t)from * R; jb.req_class = cls.data() + from;
    return jb;
  }
  int set(asched_t* h) const {
    asched_jobs jb = view(0, M);
    static const int32_t tolOff[4] = {0, 0, 0, 0}, selOff[4] = {0, 0, 1, 1}, selKey[1] = {3}, selVal[1] = {1};   // class 1 selects the odd nodes
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = 3; rc.tol_off = tolOff; rc.sel_off = selOff; rc.sel_key = selKey; rc.sel_value = selVal;
    return asched_jobs_set(h, &jb, &rc);
  }
  int append(asched_t* h, int from) const { asched_jobs jb = view(from, M - from); return asched_jobs_append(h, &jb); }
  void erase(const std::vector<int32_t>& rows) {
    std::vector<char> gone(M, 0);
    for (int j : rows) gone[j] = 1;
    Table t;
    for (int j = 0; j < M; j++) if (!gone[j]) { t.row(queue[j], pc[j], cls[j], req[(size_t)j * R], req[(size_t)j * R + 1], req[(size_t)j * R + 2]); t.submit.back() = submit[j]; }
    *this = t;
  }
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

// every row's first fit at every priority level, on the handle and on a fresh handle of the same tables
static void same(asched_t* h, bool away, const Nodes& nd, const Table& t, const char* what) {
  asched_t* f = create(away);
  CHECK(f && nd.upsert(f) == 0 && t.set(f) == 0);
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

static void inPlace(asched_t* h, int shapes, int revived, const char* what) {
  int32_t st[8], sh[8];
  CHECK(asched_jobs_append_stats(h, st) == 0 && asched_jobs_append_shape_stats(h, sh) == 0);
  CHECK(st[5] == 0 && st[7] == shapes + revived && sh[0] == 1 && sh[1] == shapes && sh[2] == revived && sh[6] == 0);
  if (st[5] || sh[6]) fprintf(stderr, "%s: rebuilt %d, reason %d\n", what, st[5], sh[6]);
}

int main() {
  std::mt19937 rng(11);
  static const int sizes[] = {1, 63, 64, 65, 255, 256, 257, 320};
  static const int counts[] = {1, 2, 5, 64, 65};
  for (int away = 0; away < 2; away++)
    for (int n : sizes) {
      Nodes nd;
      for (int i = 0; i < n; i++) nd.add(i);
      asched_t* h = create(away);
      CHECK(h != nullptr);
      if (!h) return 1;
      CHECK(asched_set_append_in_place(h, 1) == 0);
      CHECK(nd.upsert(h) == 0);
      Table t; t.base(rng, 150);
      CHECK(t.set(h) == 0);
      int salt = 0;
      for (int k : counts) {   // growing appends on one handle: re-allocations, away rows that move every time
        int before = t.M;
        t.fresh(k, away ? 1 + (k % 2) : k % 3, away && k == 5 ? 2 : 0, salt);   // (k == 5 with away: requirement class 2 gets its first away rows — new derived classes)
        // the edge shapes repeat from the second call on: count what is new
        int32_t st[8];
        CHECK(t.append(h, before) == 0);
        CHECK(asched_jobs_append_stats(h, st) == 0);
        inPlace(h, st[2], 0, "new shapes");
        CHECK(st[2] >= std::max(1, k - 4));
        same(h, away, nd, t, "new shapes");
        salt += 100;
      }
      asched_destroy(h);
      printf("%s %3d nodes: appends of 1 / 2 / 5 / 64 / 65 new shapes in place ok\n", away ? "away," : "      ", n);
    }
  { // revived shapes, then patch / delete / node-table changes after in-place appends, on one handle with away node types
    Nodes nd;
    for (int i = 0; i < 130; i++) nd.add(i);
    asched_t* h = create(true);
    CHECK(h != nullptr);
    if (!h) return 1;
    CHECK(asched_set_append_in_place(h, 1) == 0 && nd.upsert(h) == 0);
    Table t; t.base(rng, 200);
    CHECK(t.set(h) == 0);
    int before = t.M;
    t.fresh(6, 1, 0, 0);
    t.fresh(6, 2, 0, 0);
    CHECK(t.append(h, before) == 0);
    inPlace(h, 12, 0, "twelve new shapes");
    same(h, true, nd, t, "twelve new shapes");
    { // the rows of two of the new shapes leave, and come back with a new shape beside them
      std::vector<int32_t> gone = {before + 1, before + 5};
      int32_t ds[8];
      CHECK(asched_jobs_delete(h, 2, gone.data(), nullptr) == 0 && asched_jobs_delete_stats(h, ds) == 0 && ds[3] == 2);
      t.erase(gone);
      same(h, true, nd, t, "after the delete");
      before = t.M;
      t.row(0, 1, 0, 1ll << 30, 1000, 1ll << 30); t.row(1, 1, 0, 2ll << 30, 1000, 305ll << 30); t.row(2, 1, 0, 2ll << 30, 1000, 999ll << 30);
      CHECK(t.append(h, before) == 0);
      inPlace(h, 1, 2, "revived and new");
      same(h, true, nd, t, "revived and new"); }
    { // jobs_patch naming new rows: they run on node 1 (odd: every class matches it)
      int32_t rows[3] = {t.M - 1, t.M - 2, 3}, node[3] = {1, 1, 1}, sap[3] = {pcPrio[t.pc[t.M - 1]], pcPrio[t.pc[t.M - 2]], pcPrio[t.pc[3]]}; int64_t ts[3] = {5, 6, 7};
      CHECK(asched_jobs_patch(h, 3, rows, node, sap, ts) == 0);
      int32_t back[3] = {-1, -1, -1}, zero[3] = {0, 0, 0}; int64_t z64[3] = {0, 0, 0};
      CHECK(asched_jobs_patch(h, 3, rows, back, zero, z64) == 0);
      same(h, true, nd, t, "after the patches"); }
    { // nodes_patch: capacity cuts at the word edges
      int32_t rows[5] = {0, 63, 64, 65, 129}; std::vector<int64_t> al;
      for (int k = 0; k < 5; k++) { for (int r = 0; r < R; r++) al.push_back(nd.total[(size_t)rows[k] * R + r]); al[(size_t)k * R + 1] -= 3000; al[(size_t)k * R] -= 8ll << 30; }
      asched_nodes_patch_rows p; memset(&p, 0, sizeof p);
      p.n = 5; p.node = rows; p.allocatable = al.data();
      int32_t ps[8];
      CHECK(asched_nodes_patch(h, &p) == 0 && asched_nodes_patch_stats(h, ps) == 0 && ps[2] == 0);
      for (int k = 0; k < 5; k++) for (int r = 0; r < R; r++) nd.alloc[(size_t)rows[k] * R + r] = al[(size_t)k * R + r];
      same(h, true, nd, t, "after nodes_patch"); }
    { // nodes_append: five more nodes; the new shapes' mask rows get bits for them
      Nodes more = nd;
      for (int i = 130; i < 135; i++) more.add(i);
      asched_nodes_append_rows a; memset(&a, 0, sizeof a);
      std::vector<int32_t> tOff, lOff;
      for (int i = 130; i <= 135; i++) { tOff.push_back(more.tOff[i] - more.tOff[130]); lOff.push_back(more.lOff[i] - more.lOff[130]); }
      a.m = 5; a.index = more.index.data() + 130; a.total = more.total.data() + 130 * R; a.allocatable = more.alloc.data() + 130 * R;
      a.taint_off = tOff.data(); a.taint_key = more.tKey.data() + more.tOff[130]; a.taint_value = more.tVal.data() + more.tOff[130]; a.taint_effect = more.tEff.data() + more.tOff[130];
      a.label_off = lOff.data(); a.label_key = more.lKey.data() + more.lOff[130]; a.label_value = more.lVal.data() + more.lOff[130];
      int32_t as[8];
      CHECK(asched_nodes_append(h, &a) == 0 && asched_nodes_append_stats(h, as) == 0 && as[2] == 0);
      nd = more;
      same(h, true, nd, t, "after nodes_append"); }
    { // nodes_delete of three rows (no job runs), then one more in-place append on the changed node table
      int32_t rows[3] = {2, 64, 133}, ns[8];
      CHECK(asched_nodes_delete(h, 3, rows, nullptr) == 0 && asched_nodes_delete_stats(h, ns) == 0 && ns[2] == 0);
      Nodes kept;
      for (int i = 0; i < nd.N; i++) if (i != 2 && i != 64 && i != 133) {
        kept.add(i);   // (node number i keeps its index, label and taint)
        for (int r = 0; r < R; r++) kept.alloc[(size_t)(kept.N - 1) * R + r] = nd.alloc[(size_t)i * R + r];
      }
      for (int i = 0; i < kept.N; i++) kept.rank[i] = i;
      nd = kept;
      same(h, true, nd, t, "after nodes_delete");
      before = t.M;
      t.fresh(7, 2, 2, 500);
      int32_t st[8];
      CHECK(t.append(h, before) == 0 && asched_jobs_append_stats(h, st) == 0);
      inPlace(h, st[2], 0, "after the node-table changes");
      CHECK(st[2] == 7);
      same(h, true, nd, t, "in place after the node-table changes"); }
    asched_destroy(h);
    printf("revived shapes, jobs_patch, jobs_delete, nodes_patch, nodes_append, nodes_delete after in-place appends ok\n");
  }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("jobs_append of new shapes in place under ASan + UBSan: all checks passed\n");
  return 0;
}
