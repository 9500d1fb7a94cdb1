// The evictor report (asched_set_evictor_report / asched_round_evictor_report: asched_host.inc + kernels_evict_report.h) of the CPU build of the device code, as a
// stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer: rounds over running jobs only, at the shapes of tests/test_z_evictor_report.py (a), against a
// restatement written here.  The protected fraction is 0 (every queue with a job is above it) or huge (none is), so the restatement needs no fair shares.
// Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/evict_report_sanitize tools/evict_report_sanitize.cpp && /tmp/evict_report_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4;

static void shape(int N, int M, int Q, bool protectAll, int heavyNode, unsigned seed) {
  std::mt19937 rng(seed);
  static const int32_t indexedCol[3] = {1, 0, 3};
  static const int64_t indexedRes[3] = {1000, 128ll << 20, 1};
  static const int32_t pcPrio[3] = {0, 1, 3};
  static const uint8_t pcPre[3] = {1, 1, 0};
  static const double drf[4] = {1.0, 1.0, 0.0, 1.0};
  static const int64_t floating[4] = {-1, -1, 1ll << 50, -1};   // column 2 is a floating resource: summed as 0
  asched_config c; memset(&c, 0, sizeof c);
  c.num_resources = R; c.num_indexed = 3; c.indexed_col = indexedCol; c.indexed_resolution = indexedRes;
  c.num_priority_classes = 3; c.pc_priority = pcPrio; c.pc_preemptible = pcPre; c.drf_multiplier = drf; c.device = -1;
  c.floating_resource_limit = floating; c.protected_fraction_of_fair_share = protectAll ? 1e9 : 0.0;
  asched_t* h = asched_create(&c);
  CHECK(h != nullptr);
  if (!h) return;
  std::vector<uint64_t> index(N); std::vector<int32_t> rank(N); std::vector<int64_t> total((size_t)N * R, 0); std::vector<uint8_t> unsched(N, 0);
  for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * R] = 1ll << 46; total[(size_t)i * R + 1] = 6000000; unsched[i] = rng() % 7 == 0; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data(); nd.unschedulable = unsched.data();
  CHECK(asched_nodes_upsert(h, &nd) == 0);
  std::vector<int32_t> queue(M), pc(M), node(M), sap(M), gang(M, -1), card(M, 1), cls(M, 0); std::vector<int64_t> req((size_t)M * R), submit(M), runTs(M); std::vector<uint8_t> away(M);
  for (int j = 0; j < M; j++) {
    queue[j] = (int)(rng() % Q); pc[j] = (int)(rng() % 3); node[j] = heavyNode >= 0 ? heavyNode : (int)(rng() % N); sap[j] = pcPrio[pc[j]]; away[j] = rng() % 11 == 0;
    req[(size_t)j * R] = (1 + rng() % 8) * (1ll << 30); req[(size_t)j * R + 1] = 1000; req[(size_t)j * R + 2] = (1 + rng() % 3) * (1ll << 30); req[(size_t)j * R + 3] = 0;
    submit[j] = j; runTs[j] = (int64_t)(rng() % 1000);
  }
  if (M >= 4 && N >= 2) { queue[0] = queue[1] = 0; pc[0] = 0; pc[1] = 2; away[0] = away[1] = 0; gang[0] = gang[1] = 0; card[0] = card[1] = 2; }   // a gang of two classes: the closure takes the second
  asched_jobs jb; memset(&jb, 0, sizeof jb);
  jb.m = M; jb.queue = queue.data(); jb.pc = pc.data(); jb.submit_time = submit.data(); jb.req = req.data(); jb.req_class = cls.data(); jb.gang_id = gang.data(); jb.gang_cardinality = card.data();
  jb.node = node.data(); jb.scheduled_at_priority = sap.data(); jb.run_timestamp = runTs.data(); jb.away = away.data();
  static const int32_t zero2[2] = {0, 0};
  asched_req_classes rc; memset(&rc, 0, sizeof rc);
  rc.n = 1; rc.tol_off = zero2; rc.sel_off = zero2;
  CHECK(asched_jobs_set(h, &jb, &rc) == 0);
  std::vector<double> weight(Q, 1.0), qTok(Q, 1e18); std::vector<int64_t> qBurst(Q, 1ll << 62); std::vector<uint8_t> qInf(Q, 1); std::vector<int32_t> qOff(Q + 1, 0);
  asched_queues qs; memset(&qs, 0, sizeof qs);
  qs.q = Q; qs.weight = weight.data(); qs.global_tokens = 1e18; qs.global_burst = 1ll << 62; qs.global_rate_inf = 1; qs.queue_tokens = qTok.data(); qs.queue_burst = qBurst.data();
  qs.queue_rate_inf = qInf.data(); qs.queued_off = qOff.data(); qs.queued_jobs = zero2;
  CHECK(asched_set_evictor_report(h, 1) == 0);
  for (int rep = 0; rep < 2; rep++) {   // twice: the buffers of the first round are recycled by the second round_prepare
    int rcode = asched_round_prepare(h, &qs);
    CHECK(rcode == 0);
    asched_round_result res; asched_evictor_report er;
    if (rcode || asched_schedule_round(h, &res) != 0) { fprintf(stderr, "round: %s\n", asched_last_error(h)); failures++; break; }
    CHECK(asched_round_evictor_report(h, &er) == 0);
    // the restatement
    std::vector<uint8_t> flag(M, 0);
    for (int j = 0; j < M; j++) flag[j] = !protectAll && !away[j] && pcPre[pc[j]];
    if (M >= 4 && N >= 2 && flag[0]) flag[1] = 1;
    std::vector<int> cnt(N, 0), ors(N, 0), ev(N, 0), qJobs(Q, 0); std::vector<int64_t> qRes((size_t)Q * R, 0);
    int n1 = 0;
    for (int j = 0; j < M; j++) {
      cnt[node[j]]++;
      ors[node[j]] |= away[j] ? 0 : !pcPre[pc[j]] ? ASCHED_EVR_JOB_NOT_PREEMPTIBLE : protectAll ? ASCHED_EVR_BELOW_PROTECTED_FAIR_SHARE : 0;
      if (flag[j]) { ev[node[j]]++; n1++; qJobs[queue[j]]++; for (int r = 0; r < R; r++) if (r != 2) qRes[(size_t)queue[j] * R + r] += req[(size_t)j * R + r]; }
    }
    CHECK(er.num_nodes == N && er.num_queues == Q && er.num_resources == R && er.num_evicted == n1 && er.num_evicted == res.num_evicted_phase1);
    int affected = 0;
    for (int n = 0; n < N; n++) {
      int want = unsched[n] ? ASCHED_EVR_NODE_UNSCHEDULABLE : 0;
      if (!cnt[n]) want |= ASCHED_EVR_NODE_EMPTY; else { want |= ors[n]; if (!want) want = ASCHED_EVR_ALL_JOBS_PREEMPTIBLE; }
      CHECK(er.node_reasons[n] == want);
      CHECK(er.node_preemptible[n] == (cnt[n] ? want == ASCHED_EVR_ALL_JOBS_PREEMPTIBLE : !unsched[n]));
      CHECK(er.node_evicted_jobs[n] == ev[n]);
      affected += ev[n] > 0;
    }
    CHECK(er.num_affected_nodes == affected);
    for (int q = 0; q < Q; q++) {
      CHECK(er.queue_evicted_jobs[q] == qJobs[q] && er.queue_evicted_off[q + 1] - er.queue_evicted_off[q] == qJobs[q]);
      for (int r = 0; r < R; r++) CHECK(er.queue_evicted_resources[(size_t)q * R + r] == qRes[(size_t)q * R + r]);
      for (int p = er.queue_evicted_off[q]; p < er.queue_evicted_off[q + 1]; p++) {
        int j = er.evicted_job[p];
        CHECK(j >= 0 && j < M && flag[j] && queue[j] == q && er.evicted_node[p] == node[j]);
        if (p > er.queue_evicted_off[q]) {   // SchedulingOrderCompare among running jobs of one queue: class priority desc, run timestamp, submit time, id
          int i = er.evicted_job[p - 1];
          bool before = pcPrio[pc[i]] != pcPrio[pc[j]] ? pcPrio[pc[i]] > pcPrio[pc[j]] : runTs[i] != runTs[j] ? runTs[i] < runTs[j] : i < j;
          CHECK(before);
        }
      }
    }
    CHECK(er.queue_evicted_off[0] == 0 && er.queue_evicted_off[Q] == n1);
  }
  CHECK(asched_set_evictor_report(h, 0) == 0);
  asched_evictor_report er;
  CHECK(asched_round_evictor_report(h, &er) == ASCHED_ERR_INVALID);
  asched_destroy(h);
  printf("N %5d  running jobs %5d  queues %3d  %s: ok\n", N, M, Q, protectAll ? "nothing evicted" : "every preemptible job evicted");
}

int main() {
  shape(1, 40, 1, false, -1, 1);
  shape(255, 3 * 256 + 17, 3, false, -1, 2);
  shape(256, 3 * 256 + 17, 3, false, -1, 3);
  shape(257, 3 * 256 + 17, 3, true, -1, 4);
  shape(1025, 2000, 5, false, -1, 5);
  shape(40, 5000, 3, false, 7, 6);
  shape(64, 2 * EVR_TILE + 40, 70, false, -1, 7);
  shape(33, 600, 4, true, -1, 8);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("evictor report under ASan + UBSan: all shapes ok\n");
  return 0;
}
