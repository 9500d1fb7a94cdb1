// asched_req_classes_append (asched_host.inc + kernels_req_classes_append.h) of the CPU build of the device code, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: node tables of 1 .. 320 rows (the word and four-wave edges of the pass), with and without away node types (derived classes that move),
// calls that bring classes decided by node type, classes matched on the host and both, up to the 64th class, then rows of the new classes appended in place and
// nodes_patch / nodes_append / nodes_delete on the grown class mask — every step compared with a fresh handle that was given jobs_set of the same table with the whole
// class list (every row's first fit at every priority level, the node types matching the last rows).  In the CPU build the "device" arrays are heap blocks: a class
// mask that did not grow, a row moved past its block or a nodeCls write beyond N shows up here as a heap overflow.  Test infrastructure; nothing here is linked into
// the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/req_classes_append_sanitize tools/req_classes_append_sanitize.cpp && /tmp/req_classes_append_sanitize
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
  void add(int i) {   // node number i: six node types by an indexed label (key 3, three values) and an indexed taint (key 7, every fourth node); label key 5 is not indexed
    index.push_back((uint64_t)i + 1); rank.push_back(i);
    const int64_t row[R] = {64ll << 30, 16000, 512ll << 30, 0};
    total.insert(total.end(), row, row + R); alloc.insert(alloc.end(), row, row + R);
    if (tOff.empty()) { tOff.push_back(0); lOff.push_back(0); }
    if (i % 4 == 0) { tKey.push_back(7); tVal.push_back(1); tEff.push_back(1); }
    tOff.push_back((int32_t)tKey.size());
    lKey.push_back(3); lVal.push_back(i % 3); lKey.push_back(5); lVal.push_back(i % 2); lOff.push_back((int32_t)lKey.size());
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

// requirement classes: (tolerates the taint, selector key or -1, selector value, affinity on key 5 NotIn {0})
struct Cls { bool tol; int32_t selKey, selVal; bool aff; };
struct Classes {
  std::vector<Cls> c;
  std::vector<int32_t> tolOff, tolKey, tolOp, tolVal, tolEff, selOff, selKey, selVal, termOff, exprOff, exprKey, exprOp, valOff, vals; std::vector<uint8_t> has;
  asched_req_classes view(int from) {   // classes from .. as an asched_req_classes
    tolOff = {0}; selOff = {0}; termOff = {0}; exprOff = {0}; valOff = {0};
    tolKey.clear(); tolOp.clear(); tolVal.clear(); tolEff.clear(); selKey.clear(); selVal.clear(); exprKey.clear(); exprOp.clear(); vals.clear(); has.clear();
    bool any = false;
    for (size_t i = from; i < c.size(); i++) {
      if (c[i].tol) { tolKey.push_back(7); tolOp.push_back(ASCHED_TOLERATION_OP_EXISTS); tolVal.push_back(0); tolEff.push_back(0); }
      tolOff.push_back((int32_t)tolKey.size());
      if (c[i].selKey >= 0) { selKey.push_back(c[i].selKey); selVal.push_back(c[i].selVal); }
      selOff.push_back((int32_t)selKey.size());
      has.push_back(c[i].aff ? 1 : 0); any = any || c[i].aff;
      if (c[i].aff) { exprKey.push_back(5); exprOp.push_back(ASCHED_AFFINITY_OP_NOT_IN); vals.push_back(0); valOff.push_back((int32_t)vals.size()); exprOff.push_back((int32_t)exprKey.size()); }
      termOff.push_back((int32_t)exprOff.size() - 1);
    }
    tolKey.push_back(0); tolOp.push_back(0); tolVal.push_back(0); tolEff.push_back(0); selKey.push_back(0); selVal.push_back(0); exprKey.push_back(0); exprOp.push_back(0); vals.push_back(0);
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = (int32_t)(c.size() - from);
    rc.tol_off = tolOff.data(); rc.tol_key = tolKey.data(); rc.tol_op = tolOp.data(); rc.tol_value = tolVal.data(); rc.tol_effect = tolEff.data();
    rc.sel_off = selOff.data(); rc.sel_key = selKey.data(); rc.sel_value = selVal.data();
    if (any) { rc.has_affinity = has.data(); rc.aff_term_off = termOff.data(); rc.aff_expr_off = exprOff.data(); rc.aff_expr_key = exprKey.data(); rc.aff_expr_op = exprOp.data();
               rc.aff_value_off = valOff.data(); rc.aff_values = vals.data(); }
    return rc;
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
  void base(std::mt19937& rng, int m) {   // shapes on a small grid, requirement classes 0 and 1
    for (int i = 0; i < m; i++) row((int)(rng() % 3), (int)(rng() % 3), (int)(rng() % 2), (4ll << 30) * (1 + rng() % 3), 1000 * (1 + rng() % 4), (10ll << 30) * (1 + rng() % 2));
  }
  asched_jobs view(int from, int m) const {
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = m; jb.queue = queue.data() + from; jb.pc = pc.data() + from; jb.submit_time = submit.data() + from; jb.req = req.data() + (size_t)from * R; jb.req_class = cls.data() + from;
    return jb;
  }
  int set(asched_t* h, Classes& cl) const { asched_jobs jb = view(0, M); asched_req_classes rc = cl.view(0); return asched_jobs_set(h, &jb, &rc); }
  int append(asched_t* h, int from) const { asched_jobs jb = view(from, M - from); return asched_jobs_append(h, &jb); }
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
  c.num_indexed_labels = 1; c.indexed_label_keys = labelKey; c.num_indexed_taints = -1;   // every taint is indexed
  if (away) { c.pc_away_off = awayOff; c.away_priority = awayPrio; c.away_well_known = awayWkt; c.num_well_known_types = 2; c.wkt_taint_off = wktOff; c.wkt_taint_key = wktKey; c.wkt_taint_value = wktVal; c.wkt_taint_effect = wktEff; }
  return asched_create(&c);
}

// every row's first fit at every priority level, on the handle and on a fresh handle of the same tables and the whole class list
static void same(asched_t* h, bool away, const Nodes& nd, const Table& t, Classes& cl, const char* what) {
  asched_t* f = create(away);
  CHECK(f && nd.upsert(f) == 0 && t.set(f, cl) == 0);
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

// classes `more` join, then two rows of each (one of them in an away priority class), in place
static void grow(asched_t* h, Table& t, Classes& cl, const std::vector<Cls>& more, int byType, int onHost, int pc, const char* what) {
  const int c0 = (int)cl.c.size(), before = t.M;
  cl.c.insert(cl.c.end(), more.begin(), more.end());
  asched_req_classes rc = cl.view(c0);
  int32_t st[8], ja[8], sh[8];
  CHECK(asched_req_classes_append(h, &rc) == 0 && asched_req_classes_append_stats(h, st) == 0);
  CHECK(st[0] == (int)more.size() && st[1] == byType && st[2] == onHost && st[4] == 0 && st[5] == 0 && st[6] == (int)cl.c.size());
  if (st[4] || st[5]) fprintf(stderr, "%s: rebuilt %d, reason %d\n", what, st[4], st[5]);
  for (int c = c0; c < (int)cl.c.size(); c++) { t.row(c % 3, 0, c, 1ll << 30, 1000, 1ll << 30); t.row(c % 3, pc, c, 8ll << 30, 2000, (20ll + c) << 30); }
  CHECK(t.append(h, before) == 0 && asched_jobs_append_stats(h, ja) == 0 && asched_jobs_append_shape_stats(h, sh) == 0);
  CHECK(ja[5] == 0 && sh[6] == 0);
}

int main() {
  std::mt19937 rng(11);
  static const int sizes[] = {1, 63, 64, 65, 255, 256, 257, 320};
  const Cls T1a{true, 3, 7, false}, T1b{true, -1, 0, false}, T1c{false, 3, 2, false}, T1d{true, 3, 0, false}, T2a{true, 5, 1, false}, T2b{false, -1, 0, true}, T2c{true, 3, 1, true};
  for (int away = 0; away < 2; away++)
    for (int n : sizes) {
      Nodes nd;
      for (int i = 0; i < n; i++) nd.add(i);
      asched_t* h = create(away);
      CHECK(h != nullptr);
      if (!h) return 1;
      CHECK(asched_set_append_in_place(h, 1) == 0 && nd.upsert(h) == 0);
      Classes cl; cl.c = {Cls{true, -1, 0, false}, Cls{true, 3, 1, false}};
      Table t; t.base(rng, 150);
      CHECK(t.set(h, cl) == 0);
      grow(h, t, cl, {T1a, T1b, T1c, T1d}, 4, 0, 0, "decided by node type");
      same(h, away, nd, t, cl, "decided by node type");
      grow(h, t, cl, {T2a, T2b, T2c}, 0, 3, 0, "matched on the host");
      same(h, away, nd, t, cl, "matched on the host");
      grow(h, t, cl, {T1c, T2a, T1d, T2b}, 2, 2, away ? 1 : 0, "both");   // (with away node types the second row of each class brings a derived class behind the moved ones)
      same(h, away, nd, t, cl, "both");
      { std::vector<Cls> many;   // up to the 64th class in one call
        for (int c = (int)cl.c.size(); c < 64; c++) many.push_back(Cls{c % 2 == 0, 3, c % 3, false});
        grow(h, t, cl, many, (int)many.size(), 0, 0, "up to 64 classes");
        same(h, away, nd, t, cl, "up to 64 classes"); }
      asched_destroy(h);
      printf("%s %3d nodes: class appends of both tiers, rows in place ok\n", away ? "away," : "      ", n);
    }
  { // the node mutators on the grown class mask, with away node types (the derived rows moved)
    Nodes nd;
    for (int i = 0; i < 130; i++) nd.add(i);
    asched_t* h = create(true);
    CHECK(h != nullptr);
    if (!h) return 1;
    CHECK(asched_set_append_in_place(h, 1) == 0 && nd.upsert(h) == 0);
    Classes cl; cl.c = {Cls{true, -1, 0, false}, Cls{true, 3, 1, false}};
    Table t; t.base(rng, 200);
    CHECK(t.set(h, cl) == 0);
    grow(h, t, cl, {T1c, T2a, Cls{false, -1, 0, false}}, 2, 1, 1, "before the node mutators");
    same(h, true, nd, t, cl, "before the node mutators");
    { // nodes_patch: node 1 gains the taint, node 4 loses it — the bits of the classes without the toleration flip
      int32_t rows[2] = {1, 4}, tOff[3] = {0, 1, 1}, tKey[1] = {7}, tVal[1] = {1}, tEff[1] = {1}, ps[8];
      asched_nodes_patch_rows p; memset(&p, 0, sizeof p);
      p.n = 2; p.node = rows; p.taint_off = tOff; p.taint_key = tKey; p.taint_value = tVal; p.taint_effect = tEff;
      CHECK(asched_nodes_patch(h, &p) == 0 && asched_nodes_patch_stats(h, ps) == 0 && ps[2] == 0);
      Nodes nn;
      for (int i = 0; i < nd.N; i++) nn.add(i == 1 ? 4 : i == 4 ? 1 : i);   // (the taint of the other; index, rank and labels put back below)
      nn.index = nd.index; nn.rank = nd.rank; nn.lVal = nd.lVal;
      nd = nn;
      same(h, true, nd, t, cl, "after nodes_patch"); }
    { // nodes_append: five more nodes
      Nodes more = nd;
      const int n0 = nd.N;
      for (int i = n0; i < n0 + 5; i++) more.add(i);
      asched_nodes_append_rows a; memset(&a, 0, sizeof a);
      std::vector<int32_t> tOff, lOff;
      for (int i = n0; i <= n0 + 5; i++) { tOff.push_back(more.tOff[i] - more.tOff[n0]); lOff.push_back(more.lOff[i] - more.lOff[n0]); }
      a.m = 5; a.index = more.index.data() + n0; a.total = more.total.data() + (size_t)n0 * R; a.allocatable = more.alloc.data() + (size_t)n0 * R;
      a.taint_off = tOff.data(); a.taint_key = more.tKey.data() + more.tOff[n0]; a.taint_value = more.tVal.data() + more.tOff[n0]; a.taint_effect = more.tEff.data() + more.tOff[n0];
      a.label_off = lOff.data(); a.label_key = more.lKey.data() + more.lOff[n0]; a.label_value = more.lVal.data() + more.lOff[n0];
      int32_t as[8];
      CHECK(asched_nodes_append(h, &a) == 0 && asched_nodes_append_stats(h, as) == 0 && as[2] == 0);
      nd = more;
      same(h, true, nd, t, cl, "after nodes_append"); }
    { // nodes_delete of three rows (no job runs), then one more class append on the changed node table
      int32_t rows[3] = {2, 64, 133}, ns[8];
      CHECK(asched_nodes_delete(h, 3, rows, nullptr) == 0 && asched_nodes_delete_stats(h, ns) == 0 && ns[2] == 0);
      Nodes kept;
      for (int i = 0; i < nd.N; i++) if (i != 2 && i != 64 && i != 133) {
        kept.index.push_back(nd.index[i]); kept.rank.push_back(kept.N);
        for (int r = 0; r < R; r++) { kept.total.push_back(nd.total[(size_t)i * R + r]); kept.alloc.push_back(nd.alloc[(size_t)i * R + r]); }
        if (kept.tOff.empty()) { kept.tOff.push_back(0); kept.lOff.push_back(0); }
        for (int k = nd.tOff[i]; k < nd.tOff[i + 1]; k++) { kept.tKey.push_back(nd.tKey[k]); kept.tVal.push_back(nd.tVal[k]); kept.tEff.push_back(nd.tEff[k]); }
        kept.tOff.push_back((int32_t)kept.tKey.size());
        for (int k = nd.lOff[i]; k < nd.lOff[i + 1]; k++) { kept.lKey.push_back(nd.lKey[k]); kept.lVal.push_back(nd.lVal[k]); }
        kept.lOff.push_back((int32_t)kept.lKey.size());
        kept.N++;
      }
      nd = kept;
      same(h, true, nd, t, cl, "after nodes_delete");
      grow(h, t, cl, {T1d, T2c}, 1, 1, 2, "after the node-table changes");
      same(h, true, nd, t, cl, "after the node-table changes"); }
    asched_destroy(h);
    printf("nodes_patch, nodes_append, nodes_delete after class appends ok\n");
  }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("req_classes_append under ASan + UBSan: all checks passed\n");
  return 0;
}
