// The submit check's gang units (asched_submit_check's gang block in asched_host.inc + submit_gang.h) of the CPU build of the device code, as a stand-alone program for
// AddressSanitizer + UndefinedBehaviorSanitizer: the cases of tests/test_z_submit_gang_edges.py that sit at the edges of the unit's scratch — the node bitmap's last
// word full and partial with a bound node in it (A.1), 255 and 256 members each on a node of its own (A.2: the last tn / td slot), all members on one node (A.3), 255 / 256
// / 257 members (A.4), 8193 units through one SgShared, the later ones built to see what an earlier one left (B.2), and the capacity sums (C.3: an all-zero request at
// SG_CAP_CLAMP per node, a negative free column, the 64 000-member unit).  Every answer is compared with the sequential path of the same handle (ASCHED_SUBMIT_GANGS=0),
// with the value worked out by hand where the test has one, and the counters of asched_submit_stats with what the construction predicts.  In the CPU build SgShared is a
// static object and the bitmap a heap block: a tn / td index or a bitmap word out of bounds shows up here as a global or heap overflow.
// Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/submit_gangs_sanitize tools/submit_gangs_sanitize.cpp && /tmp/submit_gangs_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

typedef std::vector<std::vector<int32_t>> Units;
struct Want { int ok, n, first; };

struct Pool {
  int R, N;
  std::vector<int64_t> alloc, used, req;   // used: taken at priority <= 0 (alloc_by_prio of the upsert, no clear_allocated)
  asched_t* h = nullptr;
  Pool(int n, std::initializer_list<int64_t> row) : R((int)row.size()), N(n) { for (int i = 0; i < n; i++) alloc.insert(alloc.end(), row); }
  ~Pool() { if (h) asched_destroy(h); }
  void node(int n, std::initializer_list<int64_t> row) { std::copy(row.begin(), row.end(), alloc.begin() + (size_t)n * R); }
  int rows(std::initializer_list<int64_t> r, int n = 1) { int first = (int)(req.size() / R); for (int i = 0; i < n; i++) req.insert(req.end(), r); return first; }
  void load() {
    static const int32_t col[1] = {0}, prio[1] = {0}, zero[1] = {0};
    static const int64_t res[1] = {1};
    static const uint8_t pre[1] = {1};
    static const double drf[MAXR] = {1, 1, 1, 1, 1, 1, 1, 1};
    asched_config c; memset(&c, 0, sizeof c);
    c.num_resources = R; c.num_indexed = 1; c.indexed_col = col; c.indexed_resolution = res; c.num_priority_classes = 1; c.pc_priority = prio; c.pc_preemptible = pre;
    c.drf_multiplier = drf; c.device = -1; c.indexed_taint_keys = zero; c.indexed_label_keys = zero;
    h = asched_create(&c);
    CHECK(h != nullptr); if (!h) exit(1);
    std::vector<uint64_t> index(N); std::vector<int32_t> rank(N);
    for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; }
    int32_t prios[ASCHED_MAX_PRIORITIES];
    const int P = asched_priorities(h, prios);
    std::vector<int64_t> abp;
    for (int i = 0; i < N && !used.empty(); i++) for (int l = 0; l < P; l++) for (int r = 0; r < R; r++)
      abp.push_back(alloc[(size_t)i * R + r] - (prios[l] <= 0 ? used[(size_t)i * R + r] : 0));
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = alloc.data(); nd.allocatable = alloc.data();
    if (!used.empty()) nd.alloc_by_prio = abp.data();
    CHECK(asched_nodes_upsert(h, &nd) == 0);
    if (used.empty()) CHECK(asched_clear_allocated(h) == 0);
    const int M = (int)(req.size() / R);
    std::vector<int32_t> z(M, 0); std::vector<int64_t> submit(M);
    for (int i = 0; i < M; i++) submit[i] = i;
    static const int32_t off[2] = {0, 0};
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = 1; rc.tol_off = off; rc.tol_key = rc.tol_op = rc.tol_value = rc.tol_effect = zero; rc.sel_off = off; rc.sel_key = rc.sel_value = zero;
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = M; jb.req = req.data(); jb.queue = z.data(); jb.pc = z.data(); jb.submit_time = submit.data();
    CHECK(asched_jobs_set(h, &jb, &rc) == 0);
  }
  std::vector<asched_submit_result> ask(const Units& units, int32_t* st) {
    std::vector<int32_t> off(1, 0), jobs, flags(units.size(), 0);
    for (auto& u : units) { jobs.insert(jobs.end(), u.begin(), u.end()); off.push_back((int32_t)jobs.size()); }
    std::vector<asched_submit_result> out(units.size());
    int rc = asched_submit_check(h, (int32_t)units.size(), off.data(), jobs.data(), flags.data(), out.data());
    CHECK(rc == 0);
    if (rc) fprintf(stderr, "submit_check: %s\n", asched_last_error(h));
    CHECK(asched_submit_stats(h, st) == 0);
    return out;
  }
  // both gang paths against the sequential path of the same handle; st: {wide units, wide passes, sequential units, gang units, node passes, literal units}
  void pin(const char* what, const Units& units, int gang, int seq, int passes, const std::vector<Want>& want) {
    int32_t st[6], st0[6];
    unsetenv("ASCHED_SUBMIT_GANGS");
    auto a = ask(units, st);
    setenv("ASCHED_SUBMIT_GANGS", "0", 1);
    auto b = ask(units, st0);
    unsetenv("ASCHED_SUBMIT_GANGS");
    int bad = 0;
    for (size_t u = 0; u < units.size(); u++)
      if (a[u].ok != b[u].ok || a[u].scheduled_away != b[u].scheduled_away || a[u].num_schedulable != b[u].num_schedulable || a[u].first_node != b[u].first_node) {
        if (bad++ < 5) fprintf(stderr, "%s: unit %zu (%zu members): {%d %d %d %d}, sequential {%d %d %d %d}\n", what, u, units[u].size(), a[u].ok, a[u].scheduled_away,
                               a[u].num_schedulable, a[u].first_node, b[u].ok, b[u].scheduled_away, b[u].num_schedulable, b[u].first_node);
      }
    CHECK(bad == 0);
    for (size_t u = 0; u < want.size() && u < units.size(); u++)
      CHECK(a[u].ok == want[u].ok && a[u].scheduled_away == 0 && a[u].num_schedulable == want[u].n && a[u].first_node == want[u].first);
    CHECK(st[0] == 0 && st[1] == 0 && st[2] == seq && st[3] == gang && st[4] == passes && st[5] == 0);
    CHECK(st0[3] == 0 && st0[2] == seq + gang);
    printf("%s: %zu units, %d on the gang paths (%d node passes), %d sequential: as the sequential path\n", what, units.size(), gang, passes, seq);
  }
};

static std::vector<int32_t> range(int first, int n) { std::vector<int32_t> v(n); for (int i = 0; i < n; i++) v[i] = first + i; return v; }
static std::vector<int32_t> alternate(int a, int b, int n) { std::vector<int32_t> v; for (int i = 0; i < n; i++) v.push_back(i % 2 == 0 ? a + i / 2 : b + i / 2); return v; }

int main() {
  setvbuf(stdout, nullptr, _IONBF, 0);
  for (int N : {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513}) {   // A.1 "last": the bound node in the bitmap's last word
    const int p = N - 1, q = N >= 2 ? (p + std::max(1, N / 2)) % N : -1;
    Pool t(N, {100, 8});
    t.node(p, {105, 64});
    if (q >= 0) t.node(q, {100, 32});
    const int m0 = t.rows({10, 40}), m1 = t.rows({10, 30}), m2 = t.rows({1, 2}), m3 = t.rows({1, 2}), yes = t.rows({1, 22}), no = t.rows({1, 23});
    t.load();
    char what[64]; snprintf(what, sizeof what, "A.1 %3d nodes", N);
    if (N >= 2) t.pin(what, {{m0, m1, m2, m3, yes}, {m0, m1, m2, m3, no}}, 2, 0, 10, {{1, 5, p}, {0, 4, p}});
    else t.pin(what, {{m0, m1, m2, m3, yes}, {m0, m1, m2, m3, no}}, 2, 0, 10, {{0, 1, 0}, {0, 1, 0}});
  }
  for (int N : {255, 300}) {   // A.2
    Pool t(N, {100, 8});
    const int a = t.rows({100, 1}, 128), b = t.rows({100, 2}, 128);
    t.load();
    auto mem = alternate(a, b, 256);
    t.pin(N == 255 ? "A.2 255 nodes" : "A.2 300 nodes", {std::vector<int32_t>(mem.begin(), mem.begin() + 255), mem}, 2, 0, 511,
          {{1, 255, 0}, N >= 256 ? Want{1, 256, 0} : Want{0, 255, 0}});
  }
  for (int next : {1, 0}) {   // A.3
    Pool t(40, {2000, 0});
    t.node(0, {1000, 1000});
    if (next) t.node(1, {2000, 1000});
    const int a = t.rows({10, 1}, 60), b = t.rows({10, 2}, 60), huge = t.rows({5000, 1});
    t.load();
    auto mem = alternate(a, b, 120);
    Units units = {mem};
    for (int k : {1, 60, 119}) { auto u = mem; u[k] = huge; units.push_back(u); }
    t.pin(next ? "A.3 node 1 takes the rest" : "A.3 nobody takes the rest", units, 4, 0, 480,
          {next ? Want{1, 120, 0} : Want{0, 100, 0}, {0, 1, 0}, {0, 60, 0}, next ? Want{0, 119, 0} : Want{0, 100, 0}});
  }
  {   // A.4
    Pool t(300, {100, 8});
    const int a = t.rows({1, 0}, 129), b = t.rows({2, 0}, 128), uni = t.rows({1, 0}, 257);
    t.load();
    auto mem = alternate(a, b, 257);
    t.pin("A.4 255 / 256 / 257 members", {std::vector<int32_t>(mem.begin(), mem.begin() + 255), std::vector<int32_t>(mem.begin(), mem.begin() + 256), mem, range(uni, 257)},
          3, 1, 255 + 256 + 1, {{1, 255, 0}, {1, 256, 0}, {1, 257, 0}, {1, 257, 0}});
  }
  {   // B.2: 8193 units through one SgShared; X = nodes 3 and 35 (two bitmap words) are the only ones with 64 mem, node 7 is first in key order
    Pool t(40, {100, 8});
    t.node(7, {95, 8}); t.node(3, {100, 64}); t.node(35, {100, 64});
    const std::vector<int32_t> fill = {t.rows({100, 64}), t.rows({100, 63})}, half = {t.rows({100, 64}), t.rows({100, 63}), t.rows({100, 60})}, needx = {t.rows({50, 60}), t.rows({50, 59})};
    std::vector<int32_t> nine;
    for (int i = 0; i < 9; i++) nine.push_back(i % 2 == 0 ? t.rows({10, 8}) : t.rows({10, 7}));
    const int a = t.rows({1, 1}), b = t.rows({2, 1});
    const std::vector<int32_t> f[4] = {{a, b}, {t.rows({96, 1}), b}, {t.rows({10, 9}), b}, {a, t.rows({200, 1})}};
    const Want fw[4] = {{1, 2, 7}, {1, 2, 0}, {1, 2, 3}, {0, 1, 7}};
    t.load();
    const int nu = 8193;
    Units units; std::vector<Want> want;
    for (int i = 0; i < nu; i++) { int k = (i * 7 + i / 13) % 4; units.push_back(f[k]); want.push_back(fw[k]); }
    auto put = [&](int i, const std::vector<int32_t>& u, Want w) { units[i] = u; want[i] = w; };
    put(0, fill, {1, 2, 3}); put(4096, half, {0, 2, 3}); put(8192, needx, {1, 2, 3});
    put(5, fill, {1, 2, 3}); put(6, needx, {1, 2, 3}); put(100, half, {0, 2, 3}); put(101, needx, {1, 2, 3});   // (one SgShared here: the next unit is the one that would see what is left)
    put(4000, nine, {1, 9, 7}); put(4001, f[0], fw[0]); put(4002, half, {0, 2, 3}); put(4003, f[2], fw[2]);
    int members = 0;
    for (auto& u : units) members += (int)u.size();
    t.pin("B.2 8193 units", units, nu, 0, members, want);
  }
  for (int withUsed : {0, 1}) {   // C.3: an all-zero request, a negative free column under a zero request, a node with too little left
    const int N = 260;
    Pool t(N, {100, 8, 0});
    t.node(20, {60, 8, 0});
    if (withUsed) { t.used.assign((size_t)N * 3, 0); t.used[20 * 3 + 2] = 1; t.used[258 * 3 + 0] = 95; }
    const int zero = t.rows({0, 0, 0}, 300), one = t.rows({10, 1, 0}, 8 * N + 1), x = t.rows({10, 1, 0}), y = t.rows({20, 1, 0});
    t.load();
    const int cap = withUsed ? 8 * (N - 2) : 8 * (N - 1) + 6, first = withUsed ? 0 : 20, zfirst = withUsed ? 258 : 20;
    t.pin(withUsed ? "C.3 zero request, used nodes" : "C.3 zero request", {range(zero, 2), range(zero, 300), range(one, cap - 1), range(one, cap), range(one, cap + 1), {x, y}}, 6, 0, 3,
          {{1, 2, zfirst}, {1, 300, zfirst}, {1, cap - 1, first}, {1, cap, first}, {0, cap, first}, {1, 2, first}});
  }
  for (int N : {1999, 2001}) {   // C.3: BenchmarkScheduleMany*'s unit of 64 000 members
    const int J = 64000;
    Pool t(N, {32, 256});
    const int j = t.rows({1, 4}, J);
    t.load();
    t.pin(N == 1999 ? "C.3 64 000 members, 1999 nodes" : "C.3 64 000 members, 2001 nodes", {range(j, J)}, 1, 0, 1, {{32 * N >= J, std::min(J, 32 * N), 0}});
  }
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("submit check gang units under ASan + UBSan: all cases ok\n");
  return 0;
}
