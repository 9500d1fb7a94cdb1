// The preemption-cause join (asched_preemption_join: asched_host.inc preemptJoinRun + kernels_preempt_join.h) of the CPU build of the device code, as a stand-alone
// program for AddressSanitizer + UndefinedBehaviorSanitizer: the shapes of tests/test_z_preemption_causes.py (b) against a stable sort written here.
// Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/preempt_join_sanitize tools/preempt_join_sanitize.cpp && /tmp/preempt_join_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static asched_t* handleWithNodes(int n) {
  static const int32_t indexedCol[3] = {1, 0, 3};
  static const int64_t indexedRes[3] = {1000, 128ll << 20, 1};
  static const int32_t pcPrio[2] = {0, 1};
  static const uint8_t pcPre[2] = {1, 1};
  static const double drf[4] = {1.0, 1.0, 0.0, 1.0};
  asched_config c; memset(&c, 0, sizeof c);
  c.num_resources = 4; c.num_indexed = 3; c.indexed_col = indexedCol; c.indexed_resolution = indexedRes;
  c.num_priority_classes = 2; c.pc_priority = pcPrio; c.pc_preemptible = pcPre; c.drf_multiplier = drf; c.device = -1;
  asched_t* h = asched_create(&c);
  if (!h) return nullptr;
  std::vector<uint64_t> index(n); std::vector<int32_t> rank(n); std::vector<int64_t> total((size_t)n * 4);
  for (int i = 0; i < n; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * 4] = 64ll << 30; total[(size_t)i * 4 + 1] = 16000; total[(size_t)i * 4 + 2] = 512ll << 30; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = n; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data();
  if (asched_nodes_upsert(h, &nd)) { fprintf(stderr, "nodes_upsert: %s\n", asched_last_error(h)); asched_destroy(h); return nullptr; }
  return h;
}

static void shape(int N, int ns, int np, int heavyNode, int heavyCount, unsigned seed) {
  std::mt19937 rng(seed);
  std::vector<int32_t> sj(ns), sn(ns), sm(ns), pn(np), pb(np), ps(np); std::vector<uint8_t> pg(np);
  for (int i = 0; i < ns; i++) { sj[i] = 1000 + (int)(rng() % 100000); sn[i] = (int)(rng() % N); sm[i] = 1 + (int)(rng() % 6); }
  for (int i = 0; i < heavyCount && i < ns; i++) { sn[i * (ns / heavyCount)] = heavyNode; sm[i * (ns / heavyCount)] = ASCHED_METHOD_URGENCY; }
  if (ns >= 2) { sn[0] = 0; sn[ns - 1] = N - 1; sm[0] = sm[ns - 1] = ASCHED_METHOD_URGENCY; }
  for (int i = 0; i < np; i++) {
    int kind = (int)(rng() % 5);
    pn[i] = i == 0 ? N - 1 : i == np - 1 ? 0 : (int)(rng() % N);
    pb[i] = kind >= 2 ? (int)(rng() % 5000) : -1; ps[i] = kind == 3 ? (int)(rng() % 5000) : kind == 4 ? -2 : -1; pg[i] = kind == 3 || (rng() & 1);
  }
  // the restatement: a stable sort by node of the urgency entries
  std::vector<int> idx;
  for (int i = 0; i < ns; i++) if (sm[i] == ASCHED_METHOD_URGENCY) idx.push_back(i);
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return sn[a] < sn[b]; });
  std::vector<int32_t> off(N + 1, 0);
  for (int i : idx) off[sn[i] + 1]++;
  for (int n = 0; n < N; n++) off[n + 1] += off[n];
  asched_t* h = handleWithNodes(N);
  CHECK(h != nullptr);
  if (!h) return;
  for (int rep = 0; rep < 2; rep++) {
    std::vector<asched_preemption_cause> out(np); std::vector<int32_t> cand(idx.size()); int32_t got = -1;   // exactly as many candidate words as needed: an overrun is ASan's
    int rc = asched_preemption_join(h, ns, sj.data(), sn.data(), sm.data(), np, pn.data(), pb.data(), ps.data(), pg.data(), out.data(), cand.data(), (int32_t)cand.size(), &got);
    CHECK(rc == 0); CHECK(got == (int32_t)idx.size());
    if (rc) { fprintf(stderr, "%s\n", asched_last_error(h)); break; }
    for (size_t k = 0; k < idx.size(); k++) CHECK(cand[k] == sj[idx[k]]);
    for (int i = 0; i < np; i++) {
      int b = off[pn[i]], e = off[pn[i] + 1];
      int type = ps[i] == -2 ? ASCHED_PREEMPTION_OPTIMISER : pb[i] >= 0 ? ASCHED_PREEMPTION_FAIRSHARE : e > b ? ASCHED_PREEMPTION_URGENCY : pg[i] ? ASCHED_PREEMPTION_UNKNOWN_GANG : ASCHED_PREEMPTION_UNKNOWN;
      CHECK(out[i].type == type);
      CHECK(out[i].preempting_job == (type == ASCHED_PREEMPTION_OPTIMISER || type == ASCHED_PREEMPTION_FAIRSHARE ? pb[i] : -1));
      CHECK(out[i].preempted_sibling == (type == ASCHED_PREEMPTION_FAIRSHARE && ps[i] >= 0 ? ps[i] : -1));
      if (type == ASCHED_PREEMPTION_URGENCY) { CHECK(out[i].cand_off == b); CHECK(out[i].cand_count == e - b); }
    }
    if (!idx.empty()) {   // a short candidate buffer is refused with the size, nothing is written
      int32_t need = -1;
      CHECK(asched_preemption_join(h, ns, sj.data(), sn.data(), sm.data(), np, pn.data(), pb.data(), ps.data(), pg.data(), out.data(), cand.data(), (int32_t)cand.size() - 1, &need) == ASCHED_ERR_INVALID);
      CHECK(need == (int32_t)idx.size());
    }
  }
  asched_destroy(h);
  printf("N %7d  scheduled %5d  preempted %5d  candidates %5zu: ok\n", N, ns, np, idx.size());
}

int main() {
  shape(4, 0, 0, 0, 0, 1);
  shape(4, 40, 0, 0, 0, 2);
  shape(4, 0, 9, 0, 0, 3);
  shape(1, 37, 11, 0, 0, 4);
  shape(3 * 256 + 1, 300, 200, 0, 0, 5);
  shape(3 * PJ_TILE + 1, 1500, 700, 0, 0, 6);
  shape(256 * PJ_TILE + PJ_TILE + 1, 2000, 700, 0, 0, 7);
  shape(20, 400, 120, 7, 65, 8);
  shape(20, 900, 120, 3, 257, 9);
  shape(130, 1025, 1025, 0, 0, 10);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("preemption join under ASan + UBSan: all shapes ok\n");
  return 0;
}
