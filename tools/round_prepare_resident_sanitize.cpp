// asched_round_prepare_resident / asched_round_queued (asched_host.inc + kernels_queued_lists.h) of the CPU build of the device code, as a stand-alone program for
// AddressSanitizer + UndefinedBehaviorSanitizer: the table sizes of tests/test_z_round_prepare_resident.py (a) with 1 and 3 queues, held rows (none, duplicates, rows
// with a run, every queued row), more queues than the table has, and patch / append-with-regrow / delete / prepare_resident sequences on one handle with rounds in
// between, then the refusals — every list checked against a restatement written here (std::sort over the table) and every round against the round after round_prepare
// with those lists.  In the CPU build the "device" arrays are heap blocks: a flag word stored past the flag block, a list written past its capacity or a scratch block
// used after a regrow shows up here as a heap error; round_queued is given a buffer of exactly the total it announced.  Test infrastructure; nothing here is linked
// into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/round_prepare_resident_sanitize tools/round_prepare_resident_sanitize.cpp && /tmp/round_prepare_resident_sanitize
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int R = 4, N = 300;
static const int32_t pcPrio[3] = {0, 1, 3};

struct Table {
  int M = 0;
  std::vector<int32_t> queue, pc, node, sap, cls; std::vector<uint32_t> qprio; std::vector<int64_t> req, submit, runTs;
  void add(std::mt19937& rng, int m, bool running, int nq) {
    for (int i = 0; i < m; i++) {
      bool run = running && rng() % 3 == 0;
      queue.push_back((int)(rng() % nq)); pc.push_back((int)(rng() % 3)); qprio.push_back(rng() % 3); submit.push_back(rng() % 40);
      node.push_back(run ? (int)(rng() % N) : -1); sap.push_back(run ? pcPrio[pc.back()] : 0); runTs.push_back(run ? (int64_t)(1 + rng() % 5) * 1000000000ll : 0);
      cls.push_back(0);
      req.push_back(1ll << 30); req.push_back(1000 * (1 + (int)(rng() % 2))); req.push_back(0); req.push_back(0);
    }
    M += m;
  }
  // the queued rows of queue q that are not held: priority-class priority descending, queue priority ascending, submit time ascending, row ascending
  std::vector<int32_t> queued(int q, const std::vector<uint8_t>& hold) const {
    std::vector<int32_t> ids;
    for (int j = 0; j < M; j++) if (queue[j] == q && node[j] < 0 && !hold[j]) ids.push_back(j);
    std::sort(ids.begin(), ids.end(), [&](int a, int b) {
      if (pcPrio[pc[a]] != pcPrio[pc[b]]) return pcPrio[pc[a]] > pcPrio[pc[b]];
      if (qprio[a] != qprio[b]) return qprio[a] < qprio[b];
      if (submit[a] != submit[b]) return submit[a] < submit[b];
      return a < b;
    });
    return ids;
  }
  asched_jobs view(int from, int m) const {
    asched_jobs jb; memset(&jb, 0, sizeof jb);
    jb.m = m; jb.queue = queue.data() + from; jb.pc = pc.data() + from; jb.queue_priority = qprio.data() + from; jb.submit_time = submit.data() + from;
    jb.req = req.data() + (size_t)from * R; jb.req_class = cls.data() + from;
    return jb;
  }
  int set(asched_t* h, const double* bid = nullptr) const {
    asched_jobs jb = view(0, M);
    jb.node = node.data(); jb.scheduled_at_priority = sap.data(); jb.run_timestamp = runTs.data(); jb.bid_price = bid;
    static const int32_t zero2[2] = {0, 0};
    asched_req_classes rc; memset(&rc, 0, sizeof rc);
    rc.n = 1; rc.tol_off = zero2; rc.sel_off = zero2;
    return asched_jobs_set(h, &jb, &rc);
  }
  int append(asched_t* h, int from) const { asched_jobs jb = view(from, M - from); return asched_jobs_append(h, &jb); }
  int remove(asched_t* h, const std::vector<int32_t>& rows) {
    int rc = asched_jobs_delete(h, (int)rows.size(), rows.data(), nullptr);
    if (rc) return rc;
    std::vector<uint8_t> gone(M, 0);
    for (int j : rows) gone[j] = 1;
    int o = 0;
    for (int j = 0; j < M; j++) {
      if (gone[j]) continue;
      queue[o] = queue[j]; pc[o] = pc[j]; node[o] = node[j]; sap[o] = sap[j]; cls[o] = cls[j]; qprio[o] = qprio[j]; submit[o] = submit[j]; runTs[o] = runTs[j];
      for (int r = 0; r < R; r++) req[(size_t)o * R + r] = req[(size_t)j * R + r];
      o++;
    }
    M = o;
    for (auto* v : {&queue, &pc, &node, &sap, &cls}) v->resize(M);
    qprio.resize(M); submit.resize(M); runTs.resize(M); req.resize((size_t)M * R);
    return 0;
  }
};

struct Queues {
  std::vector<double> weight, qTok; std::vector<int64_t> qBurst; std::vector<uint8_t> qInf; asched_queues qs;
  explicit Queues(int Q) : weight(Q, 1.0), qTok(Q, 1e18), qBurst(Q, 1ll << 62), qInf(Q, 1) {
    memset(&qs, 0, sizeof qs);
    qs.q = Q; qs.weight = weight.data(); qs.global_tokens = 1e18; qs.global_burst = 1ll << 62; qs.global_rate_inf = 1; qs.queue_tokens = qTok.data(); qs.queue_burst = qBurst.data();
    qs.queue_rate_inf = qInf.data();
  }
};

// prepare_resident, the lists against the restatement, the round; then round_prepare with the explicit lists: the same lists and the same round
static void residentRound(asched_t* h, const Table& t, int Q, const std::vector<int32_t>& held, const char* what, bool heldNonNull = false) {
  std::vector<uint8_t> hold(t.M, 0);
  for (int j : held) hold[j] = 1;
  std::vector<int32_t> wantOff(Q + 1, 0), want;
  for (int q = 0; q < Q; q++) { for (int j : t.queued(q, hold)) want.push_back(j); wantOff[q + 1] = (int32_t)want.size(); }
  Queues in(Q);
  static const int32_t none = 0;
  int rc = asched_round_prepare_resident(h, &in.qs, (int)held.size(), held.empty() ? (heldNonNull ? &none : nullptr) : held.data());
  CHECK(rc == 0);
  if (rc) { fprintf(stderr, "%s: %s\n", what, asched_last_error(h)); return; }
  int nsA = -1, npA = -1;
  for (int pass = 0; pass < 2; pass++) {   // 0: after prepare_resident; 1: after round_prepare with the explicit lists
    std::vector<int32_t> off(Q + 1, -7);
    int total = asched_round_queued(h, off.data(), nullptr, 0);
    CHECK(total == (int)want.size());
    std::vector<int32_t> jobs(std::max(total, 0), -7);   // exactly the announced total
    CHECK(asched_round_queued(h, off.data(), jobs.data(), total) == total);
    CHECK(off == wantOff); CHECK(jobs == want);
    asched_round_result res;
    rc = asched_schedule_round(h, &res);
    CHECK(rc == 0);
    if (rc) { fprintf(stderr, "%s: round: %s\n", what, asched_last_error(h)); return; }
    if (pass == 0) {
      nsA = res.num_scheduled; npA = res.num_preempted;
      std::vector<int32_t> pad = want; if (pad.empty()) pad.push_back(0);
      in.qs.queued_off = wantOff.data(); in.qs.queued_jobs = pad.data();
      CHECK(asched_round_prepare(h, &in.qs) == 0);
      in.qs.queued_off = nullptr; in.qs.queued_jobs = nullptr;
    } else CHECK(res.num_scheduled == nsA && res.num_preempted == npA);
  }
  printf("%s: M %d Q %d held %zu: %zu queued, round: %d scheduled, %d preempted\n", what, t.M, Q, held.size(), want.size(), nsA, npA);
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
  std::mt19937 rng(11);
  { Queues in(2); int32_t off[3]; CHECK(asched_round_prepare_resident(h, &in.qs, 0, nullptr) == ASCHED_ERR_INVALID); CHECK(asched_round_queued(h, off, nullptr, 0) == ASCHED_ERR_INVALID); }   // nothing set
  std::vector<uint64_t> index(N); std::vector<int32_t> rank(N); std::vector<int64_t> total((size_t)N * R, 0);
  for (int i = 0; i < N; i++) { index[i] = i + 1; rank[i] = i; total[(size_t)i * R] = 1ll << 46; total[(size_t)i * R + 1] = 32000; total[(size_t)i * R + 2] = 1ll << 46; }
  asched_nodes nd; memset(&nd, 0, sizeof nd);
  nd.n = N; nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = total.data();
  CHECK(asched_nodes_upsert(h, &nd) == 0);
  { Queues in(2); CHECK(asched_round_prepare_resident(h, &in.qs, 0, nullptr) == ASCHED_ERR_INVALID); }   // no job table
  // the sizes of the test file: the tail of the flag words, the edges of a workgroup and of a chunk of the compaction; growing and shrinking tables on one handle
  static const int sizes[] = {8193, 1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 5};
  for (int m : sizes) for (int nq : {1, 3}) {
    Table t; t.add(rng, m, true, nq);
    CHECK(t.set(h) == 0);
    residentRound(h, t, nq, {}, "sizes");
  }
  { // held rows, and the queue count against the table
    Table t; t.add(rng, 1201, true, 4);
    CHECK(t.set(h) == 0);
    std::vector<int32_t> q, r;
    for (int j = 0; j < t.M; j++) (t.node[j] < 0 ? q : r).push_back(j);
    residentRound(h, t, 4, {}, "held non-NULL with n_held == 0", true);
    residentRound(h, t, 4, {q[7]}, "one held");
    residentRound(h, t, 4, {q[1], q[1], q[5], q[1], q.back(), q.back()}, "duplicates");
    residentRound(h, t, 4, r, "held rows that have a run");
    residentRound(h, t, 4, q, "every queued row held");
    residentRound(h, t, 2, {}, "fewer queues than the table");
    residentRound(h, t, 9, {}, "more queues than the table");
    residentRound(h, t, 300, {q[3]}, "300 queues");
  }
  { // patch / append-with-regrow / delete / prepare_resident, three times over
    Table t; t.add(rng, 3011, true, 4);
    CHECK(t.set(h) == 0);
    residentRound(h, t, 4, {}, "fresh table");
    for (int k = 0; k < 3; k++) {
      std::vector<int32_t> rows, pnode, psap; std::vector<int64_t> pts;
      for (int j = k; j < t.M; j += 7) {
        bool stop = t.node[j] >= 0;
        rows.push_back(j); pnode.push_back(stop ? -1 : j % N); psap.push_back(stop ? 0 : pcPrio[t.pc[j]]); pts.push_back(stop ? 0 : 9000000000ll);
        t.node[j] = pnode.back(); t.sap[j] = psap.back(); t.runTs[j] = pts.back();
      }
      CHECK(asched_jobs_patch(h, (int)rows.size(), rows.data(), pnode.data(), psap.data(), pts.data()) == 0);
      residentRound(h, t, 4, {}, "after a patch");
      int before = t.M;
      t.add(rng, before / 2 + 300, false, 5 + k);                   // outgrows 1.25 x the capacity at least once; queue indices the table had not seen
      CHECK(t.append(h, before) == 0);
      residentRound(h, t, 5 + k, {(int32_t)t.M - 1, 0}, "after an append");
      std::vector<int32_t> gone;
      for (int j = 2; j < t.M; j += 5) gone.push_back(j);
      CHECK(t.remove(h, gone) == 0);
      residentRound(h, t, 5 + k, {(int32_t)t.M - 1}, "after a delete");
    }
    // the refusals: nothing changes, the next call is right
    Queues in(4);
    int32_t off[5];
    in.qs.queued_off = off;
    CHECK(asched_round_prepare_resident(h, &in.qs, 0, nullptr) == ASCHED_ERR_INVALID);
    in.qs.queued_off = nullptr; in.qs.queued_jobs = off;
    CHECK(asched_round_prepare_resident(h, &in.qs, 0, nullptr) == ASCHED_ERR_INVALID);
    in.qs.queued_jobs = nullptr;
    int32_t bad[2] = {0, -1};
    CHECK(asched_round_prepare_resident(h, &in.qs, 2, bad) == ASCHED_ERR_INVALID);
    bad[1] = t.M;
    CHECK(asched_round_prepare_resident(h, &in.qs, 2, bad) == ASCHED_ERR_INVALID);
    CHECK(asched_round_prepare_resident(h, &in.qs, -1, nullptr) == ASCHED_ERR_INVALID);
    CHECK(asched_round_prepare_resident(h, &in.qs, 1, nullptr) == ASCHED_ERR_INVALID);
    { Queues big(4097); CHECK(asched_round_prepare_resident(h, &big.qs, 0, nullptr) == ASCHED_ERR_UNSUPPORTED); }
    residentRound(h, t, 4, {}, "after the refusals");
    std::vector<double> bid(t.M, 1.0);
    CHECK(t.set(h, bid.data()) == 0);
    CHECK(asched_round_prepare_resident(h, &in.qs, 0, nullptr) == ASCHED_ERR_UNSUPPORTED);
    CHECK(t.set(h) == 0);
    residentRound(h, t, 4, {}, "after the market refusal");
  }
  asched_destroy(h);
  printf(failures ? "%d FAILURES\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
