// The resident table calls of the CPU build of the device code under seeded interleavings, as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer:
// what tests/resident_sequences.py draws in Python, drawn here by a small generator of its own — asched_jobs_append (known, new and revived shapes, whole gangs, the
// in-place switch at random), asched_jobs_delete (random rows, the first and the last, whole shapes, the held rows), the last round applied with asched_jobs_patch,
// asched_jobs_reprioritise, asched_req_classes_append, asched_shapes_compact with and without classes, asched_nodes_patch (cordon, capacity, taint),
// asched_nodes_delete and asched_nodes_append, a few hundred sequences on one handle each, the node count starting at 3 ... 130 and carried across the word edges.
// After every step every row's first fit at every priority level and a round are compared with a second handle that is given the model's tables by
// asched_nodes_upsert and asched_jobs_set.  In the CPU build the "device" arrays are heap blocks: a block sized by a stale capacity (jobCap, ordCap / ordSpareCap,
// ndKeepCap ...) or a stale stride (Npad, W) shows up here as a heap overflow even where the answers stay right.
// Every one of the nine calls is made under the sweep of tests/test_z_resident_out_of_memory.py first: the CPU build's hook refuses its k-th plat_try_malloc for
// k = 0, 1, 2, ... until the hook no longer fires.  Each refused call must return ASCHED_ERR_DEVICE with "the handle is as it was" and leave the table sizes; the call
// that goes through is then compared as above, so a refusal that changed the handle shows there, and a fresh block a refusal did not free is a leak at exit
// (LeakSanitizer: ASAN_OPTIONS=detect_leaks=1, the default on Linux).
// Test infrastructure; nothing here is linked into the product.  From the repository root:
//   g++ -Itests/hostsim -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -fno-strict-aliasing -Wno-unused-function -pthread \
//       -o /tmp/resident_sequences_sanitize tools/resident_sequences_sanitize.cpp && /tmp/resident_sequences_sanitize [sequences [steps [first seed]]]
#include "../tests/hostsim/hostsim.cpp"
#include <cstdio>
#include <random>
#include <set>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s   [seed %d step %d %s]\n", __FILE__, __LINE__, #c, curSeed, curStep, curOp); failures++; } } while (0)
static int curSeed = 0, curStep = 0; static const char* curOp = "";
static int refusals[9] = {0};

// `call` (the same arguments every time) armed at k = 0, 1, 2, ...: refused for memory while the hook fires -> the return code of the call that goes through
template <class F> static int swept(asched_t* h, int op, F call) {
  const int N = asched_num_nodes(h);
  for (int k = 0;; k++) {
    hostsim_try_malloc_fail_at(k);
    const int rc = call();
    const bool fired = hostsim_try_malloc_seen() > k;
    hostsim_try_malloc_fail_at(-1);
    if (!fired) return rc;
    CHECK(rc == ASCHED_ERR_DEVICE && strstr(asched_last_error(h), "the handle is as it was") != nullptr);
    CHECK(asched_num_nodes(h) == N);
    if (rc != ASCHED_ERR_DEVICE) return rc;
    refusals[op]++;
  }
}

static const int R = 4, Q = 3;
static const int32_t pcPrio[3] = {0, 1, 3};
static const int64_t GI = 1ll << 30, MI128 = 128ll << 20;
typedef std::mt19937 Rng;
static int below(Rng& g, int n) { return (int)(g() % (uint32_t)n); }

struct Nodes {   // a node table as asched_nodes_upsert is given it; rows [from, n) of it as asched_nodes_append is
  std::vector<uint64_t> index; std::vector<int32_t> rank, lVal; std::vector<int64_t> total, alloc; std::vector<uint8_t> uns; std::vector<uint8_t> tainted;
  uint64_t nextIndex = 1; int32_t nextRank = 0;
  int n() const { return (int)index.size(); }
  void push(int lv, bool taint) {
    index.push_back(nextIndex++); rank.push_back(nextRank++); lVal.push_back(lv); uns.push_back(0); tainted.push_back(taint);
    const int64_t t[R] = {64 * GI, 16000, 512 * GI, 0};
    total.insert(total.end(), t, t + R); alloc.insert(alloc.end(), t, t + R);
  }
  void keepRows(const std::vector<uint8_t>& keep) {
    size_t k = 0;
    for (size_t i = 0; i < keep.size(); i++) if (keep[i]) {
      index[k] = index[i]; rank[k] = rank[i]; lVal[k] = lVal[i]; uns[k] = uns[i]; tainted[k] = tainted[i];
      for (int r = 0; r < R; r++) { total[k * R + r] = total[i * R + r]; alloc[k * R + r] = alloc[i * R + r]; }
      k++;
    }
    index.resize(k); rank.resize(k); lVal.resize(k); uns.resize(k); tainted.resize(k); total.resize(k * R); alloc.resize(k * R);
  }
  struct Csr { std::vector<int32_t> tOff, tKey, tVal, tEff, lOff, lKey, lVal; };
  Csr csr(const std::vector<int>& rows) const {
    Csr c; c.tOff.push_back(0); c.lOff.push_back(0);
    for (int i : rows) {
      if (tainted[i]) { c.tKey.push_back(7); c.tVal.push_back(1); c.tEff.push_back(1); }
      c.tOff.push_back((int32_t)c.tKey.size());
      c.lKey.push_back(3); c.lVal.push_back(lVal[i]); c.lOff.push_back((int32_t)c.lKey.size());
    }
    c.tKey.push_back(0); c.tVal.push_back(0); c.tEff.push_back(0); c.lKey.push_back(0); c.lVal.push_back(0);
    return c;
  }
  static std::vector<int> range(int a, int b) { std::vector<int> v; for (int i = a; i < b; i++) v.push_back(i); return v; }
  int upsert(asched_t* h) const {
    Csr c = csr(range(0, n()));
    asched_nodes nd; memset(&nd, 0, sizeof nd);
    nd.n = n(); nd.index = index.data(); nd.id_rank = rank.data(); nd.total = total.data(); nd.allocatable = alloc.data(); nd.unschedulable = uns.data();
    nd.taint_off = c.tOff.data(); nd.taint_key = c.tKey.data(); nd.taint_value = c.tVal.data(); nd.taint_effect = c.tEff.data();
    nd.label_off = c.lOff.data(); nd.label_key = c.lKey.data(); nd.label_value = c.lVal.data();
    return asched_nodes_upsert(h, &nd);
  }
  int append(asched_t* h, int from) const {
    Csr c = csr(range(from, n()));
    asched_nodes_append_rows a; memset(&a, 0, sizeof a);
    a.m = n() - from; a.index = index.data() + from; a.id_rank = rank.data() + from; a.total = total.data() + (size_t)from * R; a.allocatable = alloc.data() + (size_t)from * R;
    a.unschedulable = uns.data() + from;
    a.taint_off = c.tOff.data(); a.taint_key = c.tKey.data(); a.taint_value = c.tVal.data(); a.taint_effect = c.tEff.data();
    a.label_off = c.lOff.data(); a.label_key = c.lKey.data(); a.label_value = c.lVal.data();
    return asched_nodes_append(h, &a);
  }
};

struct Cls { bool tolerates; int sel; };   // tolerates the taint of key 7; selects label value sel (-1: none)

struct Table {   // the job table as asched_jobs_set is given it; rows [from, m) of it as asched_jobs_append is
  std::vector<int32_t> queue, pc, cls, node, prio, gang, card; std::vector<uint32_t> qprio; std::vector<int64_t> req, ts, submit; std::vector<uint8_t> held;
  std::vector<Cls> classes;
  int64_t nextSubmit = 0, now = 0; int32_t nextGang = 0; int newReqs = 0;
  int m() const { return (int)queue.size(); }
  void push(int q, int p, int c, const int64_t* rq, int g, int cd) {
    queue.push_back(q); pc.push_back(p); cls.push_back(c); node.push_back(-1); prio.push_back(0); gang.push_back(g); card.push_back(cd); qprio.push_back(0); ts.push_back(0);
    submit.push_back(nextSubmit++); held.push_back(0); req.insert(req.end(), rq, rq + R);
  }
  void keepRows(const std::vector<uint8_t>& keep) {
    size_t k = 0;
    for (size_t j = 0; j < keep.size(); j++) if (keep[j]) {
      queue[k] = queue[j]; pc[k] = pc[j]; cls[k] = cls[j]; node[k] = node[j]; prio[k] = prio[j]; gang[k] = gang[j]; card[k] = card[j]; qprio[k] = qprio[j]; ts[k] = ts[j];
      submit[k] = submit[j]; held[k] = held[j];
      for (int r = 0; r < R; r++) req[k * R + r] = req[j * R + r];
      k++;
    }
    queue.resize(k); pc.resize(k); cls.resize(k); node.resize(k); prio.resize(k); gang.resize(k); card.resize(k); qprio.resize(k); ts.resize(k); submit.resize(k); held.resize(k);
    req.resize(k * R);
  }
  struct CCls { std::vector<int32_t> tOff, tKey, tOp, tVal, tEff, sOff, sKey, sVal; asched_req_classes rc; };
  static void classesOf(const std::vector<Cls>& cl, CCls& c) {
    c.tOff.assign(1, 0); c.sOff.assign(1, 0);
    for (const Cls& x : cl) {
      if (x.tolerates) { c.tKey.push_back(7); c.tOp.push_back(ASCHED_TOLERATION_OP_EXISTS); c.tVal.push_back(0); c.tEff.push_back(0); }
      if (x.sel >= 0) { c.sKey.push_back(3); c.sVal.push_back(x.sel); }
      c.tOff.push_back((int32_t)c.tKey.size()); c.sOff.push_back((int32_t)c.sKey.size());
    }
    c.tKey.push_back(0); c.tOp.push_back(0); c.tVal.push_back(0); c.tEff.push_back(0); c.sKey.push_back(0); c.sVal.push_back(0);
    memset(&c.rc, 0, sizeof c.rc);
    c.rc.n = (int32_t)cl.size(); c.rc.tol_off = c.tOff.data(); c.rc.tol_key = c.tKey.data(); c.rc.tol_op = c.tOp.data(); c.rc.tol_value = c.tVal.data(); c.rc.tol_effect = c.tEff.data();
    c.rc.sel_off = c.sOff.data(); c.rc.sel_key = c.sKey.data(); c.rc.sel_value = c.sVal.data();
  }
  void rows(asched_jobs& jb, int from) const {
    memset(&jb, 0, sizeof jb);
    jb.m = m() - from; jb.queue = queue.data() + from; jb.pc = pc.data() + from; jb.queue_priority = qprio.data() + from; jb.submit_time = submit.data() + from;
    jb.req = req.data() + (size_t)from * R; jb.req_class = cls.data() + from; jb.gang_id = gang.data() + from; jb.gang_cardinality = card.data() + from;
  }
  int set(asched_t* h) const {
    CCls c; classesOf(classes, c);
    asched_jobs jb; rows(jb, 0);
    jb.node = node.data(); jb.scheduled_at_priority = prio.data(); jb.run_timestamp = ts.data();
    return asched_jobs_set(h, &jb, &c.rc);
  }
  int append(asched_t* h, int from) const { asched_jobs jb; rows(jb, from); return asched_jobs_append(h, &jb); }
  bool before(int a, int b) const {   // SchedulingOrderCompare for rows without a run
    if (pc[a] != pc[b]) return pcPrio[pc[a]] > pcPrio[pc[b]];
    if (qprio[a] != qprio[b]) return qprio[a] < qprio[b];
    if (submit[a] != submit[b]) return submit[a] < submit[b];
    return a < b;
  }
};

struct Round { int rc = 0, sum = -1; std::vector<int32_t> sJob, sNode, sPrio, pJob; };
static Round roundOf(asched_t* h, const Table& t) {
  std::vector<double> weight(Q, 1.0), qTok(Q, 1e18); std::vector<int64_t> qBurst(Q, 1ll << 62); std::vector<uint8_t> qInf(Q, 1); std::vector<int32_t> qOff(Q + 1, 0), queued;
  for (int q = 0; q < Q; q++) {
    std::vector<int32_t> l;
    for (int j = 0; j < t.m(); j++) if (t.queue[j] == q && t.node[j] < 0 && !t.held[j]) l.push_back(j);
    std::sort(l.begin(), l.end(), [&](int a, int b) { return t.before(a, b); });
    queued.insert(queued.end(), l.begin(), l.end());
    qOff[q + 1] = (int32_t)queued.size();
  }
  queued.push_back(0);
  asched_queues qs; memset(&qs, 0, sizeof qs);
  qs.q = Q; qs.weight = weight.data(); qs.global_tokens = 1e18; qs.global_burst = 1ll << 62; qs.global_rate_inf = 1; qs.queue_tokens = qTok.data(); qs.queue_burst = qBurst.data();
  qs.queue_rate_inf = qInf.data(); qs.queued_off = qOff.data(); qs.queued_jobs = queued.data();
  Round out;
  CHECK(asched_round_prepare(h, &qs) == 0);
  asched_round_result res;
  out.rc = asched_schedule_round(h, &res);
  CHECK(out.rc == 0);
  if (out.rc) { fprintf(stderr, "round: %s\n", asched_last_error(h)); return out; }
  uint32_t sum = (uint32_t)res.num_scheduled;
  for (int i = 0; i < res.num_scheduled; i++) {
    sum = sum * 31u + (uint32_t)res.scheduled_job[i] * 7u + (uint32_t)res.scheduled_node[i];
    out.sJob.push_back(res.scheduled_job[i]); out.sNode.push_back(res.scheduled_node[i]); out.sPrio.push_back(res.scheduled_priority[i]);
  }
  for (int i = 0; i < res.num_preempted; i++) { sum = sum * 31u + (uint32_t)res.preempted_job[i] * 7u + (uint32_t)res.preempted_node[i]; out.pJob.push_back(res.preempted_job[i]); }
  out.sum = (int)(sum & 0x7fffffffu);
  return out;
}

// the handle after a step against a handle that is given the model's tables by nodes_upsert and jobs_set -> the handle's round
static Round compare(asched_t* h, asched_t* f, const Nodes& nd, const Table& t) {
  CHECK(nd.upsert(f) == 0 && t.set(f) == 0);
  CHECK(asched_num_nodes(h) == nd.n() && asched_num_nodes(f) == nd.n());
  const int M = t.m();
  std::vector<int32_t> ids(M), a(M), b(M), prios(ASCHED_MAX_PRIORITIES);
  for (int j = 0; j < M; j++) ids[j] = j;
  const int P = asched_priorities(h, prios.data());
  for (int l = 0; l < P; l++) {
    CHECK(asched_fit_select_batch(h, M, ids.data(), prios[l], a.data()) == 0 && asched_fit_select_batch(f, M, ids.data(), prios[l], b.data()) == 0);
    CHECK(a == b);
  }
  const Round ra = roundOf(h, t), rb = roundOf(f, t);
  CHECK(ra.sum == rb.sum && ra.sJob == rb.sJob && ra.sNode == rb.sNode && ra.pJob == rb.pJob);
  return ra;
}

static asched_t* create(const asched_config& c) { asched_t* h = asched_create(&c); if (!h) { fprintf(stderr, "asched_create failed\n"); exit(1); } return h; }
static void newReq(int k, int64_t* rq) { rq[0] = 2 * GI; rq[1] = 1000; rq[2] = (int64_t)(300 + k) * GI; rq[3] = 0; }   // a fit shape of its own: the non-indexed column differs

static void sequence(const asched_config& c, int seed, int steps, int counts[16]) {
  Rng g((uint32_t)seed * 2654435761u + 17u);
  curSeed = seed; curStep = 0; curOp = "load";
  asched_t* h = create(c); asched_t* f = create(c);
  static const int starts[8] = {3, 40, 63, 64, 65, 100, 128, 130};
  Nodes nd; Table t;
  const int N0 = starts[below(g, 8)], M0 = 5 + below(g, 196);
  for (int i = 0; i < N0; i++) nd.push(i % 3, i % 4 == 0);
  t.classes = {{true, -1}, {true, 1}};
  for (int j = 0; j < M0; j++) { const int64_t rq[R] = {(int64_t)(4 << below(g, 4)) * GI, (int64_t)(1000 << below(g, 4)), 0, 0}; t.push(below(g, Q), below(g, 3), below(g, 10) < 3, rq, -1, 1); }
  CHECK(nd.upsert(h) == 0 && t.set(h) == 0);
  Round last = compare(h, f, nd, t);
  const int turn = 8 + below(g, 14); const bool outFirst = below(g, 10) < 6;
  for (int step = 1; step <= steps; step++) {
    curStep = step;
    const bool out = (step < turn) == outFirst;
    const int M = t.m(), N = nd.n();
    std::vector<uint8_t> used(N, 0);
    for (int j = 0; j < M; j++) if (t.node[j] >= 0) used[t.node[j]] = 1;
    int nFree = 0; for (int i = 0; i < N; i++) nFree += !used[i];
    int running = 0; for (int j = 0; j < M; j++) running += t.node[j] >= 0;
    // weights of the applicable operations (tests/resident_sequences.py _draw)
    int w[9] = {out ? 3 : 6, M >= 2 ? (out ? 6 : 2) : 0, (last.sJob.size() + last.pJob.size() + running / 5) > 0 ? 3 : 0, 2, (int)t.classes.size() < 12 ? 2 : 0, 3, 3,
                (N >= 2 && nFree > 0) ? (out ? 6 : 1) : 0, N <= 400 ? (out ? 1 : 5) : 0};
    int tot = 0; for (int x : w) tot += x;
    int pick = below(g, tot), op = 0;
    while (pick >= w[op]) pick -= w[op++];
    counts[op]++;
    switch (op) {
    case 0: { curOp = "jobs_append";
      const int k = 1 + below(g, 40), m0 = M;
      for (int i = 0; i < k;) {
        int64_t rq[R]; const int x = below(g, 10);
        if (x < 4) { const int j = below(g, m0); for (int r = 0; r < R; r++) rq[r] = t.req[(size_t)j * R + r]; }
        else if (x < 8 && t.newReqs > 0) newReq(below(g, t.newReqs), rq);
        else newReq(t.newReqs++, rq);
        const int q = below(g, Q), p = below(g, 3), cl = below(g, (int)t.classes.size());
        int cnt = 1, gid = -1;
        if (below(g, 8) == 0 && k - i >= 2) { cnt = 2 + below(g, std::min(5, k - i - 1)); gid = t.nextGang++; }   // a whole new gang: consecutive rows of one queue and shape
        for (int e = 0; e < cnt; e++) t.push(q, p, cl, rq, gid, gid >= 0 ? cnt : 1);
        i += cnt;
      }
      CHECK(asched_set_append_in_place(h, below(g, 10) < 6) == 0);
      CHECK(swept(h, 0, [&] { return t.append(h, m0); }) == 0);
      int32_t st[8]; CHECK(asched_jobs_append_stats(h, st) == 0 && st[0] == t.m() - m0);
      counts[9] += st[5]; counts[10] += st[4];
    } break;
    case 1: { curOp = "jobs_delete";
      const int most = std::max(1, M / 2), how = below(g, 5);
      std::set<int> rows;
      if (how == 0) { rows.insert(0); rows.insert(M - 1); }
      if (how == 1) { const int j0 = below(g, M);   // every row of one shape: the shape dies
        for (int j = 0; j < M; j++) if (t.cls[j] == t.cls[j0] && t.pc[j] == t.pc[j0] && std::equal(t.req.begin() + (size_t)j * R, t.req.begin() + (size_t)(j + 1) * R, t.req.begin() + (size_t)j0 * R)) rows.insert(j); }
      if (how == 2) for (int j = 0; j < M; j++) if (t.held[j]) rows.insert(j);
      if (how == 3) { const int j0 = below(g, M); for (int j = 0; j < M; j++) if (t.gang[j0] >= 0 && t.gang[j] == t.gang[j0] && (j & 1)) rows.insert(j); }   // part of a gang, where the drawn row is in one
      while ((int)rows.size() > most) rows.erase(std::prev(rows.end()));
      int extra = below(g, 10) < 3 ? most - (int)rows.size() : below(g, most - (int)rows.size() + 1);
      if (rows.empty() && extra == 0) extra = 1;
      while (extra > 0) { if (rows.insert(below(g, M)).second) extra--; }
      if ((int)rows.size() >= M) rows.erase(rows.begin());
      std::vector<int32_t> r(rows.begin(), rows.end()), map(M);
      CHECK(swept(h, 1, [&] { return asched_jobs_delete(h, (int32_t)r.size(), r.data(), map.data()); }) == 0);
      std::vector<uint8_t> keep(M, 1); for (int j : r) keep[j] = 0;
      int next = 0; for (int j = 0; j < M; j++) CHECK(map[j] == (keep[j] ? next++ : -1));
      t.keepRows(keep);
    } break;
    case 2: { curOp = "jobs_patch";   // the last round applied: scheduled rows run, preempted rows lose their run, a fifth of the running rows finishes
      std::set<int> rows; t.now += 1000000000ll;
      for (size_t i = 0; i < last.sJob.size(); i++) { const int j = last.sJob[i]; t.node[j] = last.sNode[i]; t.prio[j] = last.sPrio[i]; t.ts[j] = t.now; rows.insert(j); }
      for (int j : last.pJob) { t.node[j] = -1; t.prio[j] = 0; t.ts[j] = 0; t.held[j] = 1; rows.insert(j); }
      std::vector<int> run; for (int j = 0; j < M; j++) if (t.node[j] >= 0) run.push_back(j);
      std::shuffle(run.begin(), run.end(), g);
      for (size_t i = 0; i < run.size() / 5; i++) { const int j = run[i]; t.node[j] = -1; t.prio[j] = 0; t.ts[j] = 0; t.held[j] = 1; rows.insert(j); }
      std::vector<int32_t> jb(rows.begin(), rows.end()), n2, p2; std::vector<int64_t> t2;
      for (int j : jb) { n2.push_back(t.node[j]); p2.push_back(t.prio[j]); t2.push_back(t.ts[j]); }
      CHECK(swept(h, 2, [&] { return asched_jobs_patch(h, (int32_t)jb.size(), jb.data(), n2.data(), p2.data(), t2.data()); }) == 0);
    } break;
    case 3: { curOp = "jobs_reprioritise";
      std::set<int> rows; const int k = 1 + below(g, std::max(1, M / 3));
      while ((int)rows.size() < k) rows.insert(below(g, M));
      std::vector<uint32_t> np(M); for (int j = 0; j < M; j++) np[j] = (uint32_t)below(g, 5);
      for (int j0 : std::vector<int>(rows.begin(), rows.end())) if (t.gang[j0] >= 0)   // a gang moves as a whole and to one priority
        for (int j = 0; j < M; j++) if (t.gang[j] == t.gang[j0]) { rows.insert(j); np[j] = np[j0]; }
      std::vector<int32_t> jb(rows.begin(), rows.end()); std::vector<uint32_t> qp;
      for (int j : jb) { t.qprio[j] = np[j]; qp.push_back(np[j]); }
      CHECK(swept(h, 3, [&] { return asched_jobs_reprioritise(h, (int32_t)jb.size(), jb.data(), qp.data()); }) == 0);
    } break;
    case 4: { curOp = "req_classes_append";
      const Cls cl = {below(g, 2) == 0, below(g, 4) - 1};
      Table::CCls cc; Table::classesOf({cl}, cc);
      CHECK(swept(h, 4, [&] { return asched_req_classes_append(h, &cc.rc); }) == 0);
      t.classes.push_back(cl);
    } break;
    case 5: { curOp = "shapes_compact";
      const bool withClasses = below(g, 2) == 0;
      std::vector<int32_t> map(t.classes.size(), -2);
      CHECK(swept(h, 5, [&] { return asched_shapes_compact(h, withClasses ? ASCHED_COMPACT_CLASSES : 0, withClasses ? map.data() : nullptr); }) == 0);
      int32_t st[8]; CHECK(asched_shapes_compact_stats(h, st) == 0);
      counts[11] += st[0] > 0; counts[12] += st[2] > 0;
      if (withClasses) {   // the class map applied to the model
        std::vector<Cls> live; for (size_t cix = 0; cix < map.size(); cix++) if (map[cix] >= 0) { CHECK(map[cix] == (int32_t)live.size()); live.push_back(t.classes[cix]); }
        for (int j = 0; j < M; j++) { CHECK(map[t.cls[j]] >= 0); t.cls[j] = map[t.cls[j]]; }
        t.classes = live;
      }
    } break;
    case 6: { curOp = "nodes_patch";
      std::set<int> rows; const int k = 1 + below(g, std::min(N, 12));
      while ((int)rows.size() < k) rows.insert(below(g, N));
      std::vector<int32_t> r(rows.begin(), rows.end());
      asched_nodes_patch_rows p; memset(&p, 0, sizeof p);
      p.n = k; p.node = r.data();
      std::vector<uint8_t> u; std::vector<int64_t> al; Nodes::Csr cs;
      const int how = below(g, 3);
      if (how == 0) { for (int i : r) { nd.uns[i] = (uint8_t)below(g, 2); u.push_back(nd.uns[i]); } p.unschedulable = u.data(); }
      if (how == 1) { for (int i : r) { nd.alloc[(size_t)i * R] = nd.total[(size_t)i * R] - below(g, 33) * GI; nd.alloc[(size_t)i * R + 1] = nd.total[(size_t)i * R + 1] - below(g, 9) * 1000;
                                        al.insert(al.end(), nd.alloc.begin() + (size_t)i * R, nd.alloc.begin() + (size_t)(i + 1) * R); } p.allocatable = al.data(); }
      if (how == 2) {   // a node keeps the taint off where a run of a class without the toleration sits
        for (int i : r) { bool closed = false; for (int j = 0; j < M; j++) closed |= t.node[j] == i && !t.classes[t.cls[j]].tolerates; nd.tainted[i] = !(nd.tainted[i] || closed); }
        cs = nd.csr(std::vector<int>(r.begin(), r.end()));
        p.taint_off = cs.tOff.data(); p.taint_key = cs.tKey.data(); p.taint_value = cs.tVal.data(); p.taint_effect = cs.tEff.data(); }
      CHECK(swept(h, 6, [&] { return asched_nodes_patch(h, &p); }) == 0);
    } break;
    case 7: { curOp = "nodes_delete";
      std::vector<int> freeRows; for (int i = 0; i < N; i++) if (!used[i]) freeRows.push_back(i);
      const int most = std::min((int)freeRows.size(), N - 1);
      const int k = below(g, 4) == 0 ? most : 1 + below(g, most);
      std::shuffle(freeRows.begin(), freeRows.end(), g); freeRows.resize(k); std::sort(freeRows.begin(), freeRows.end());
      std::vector<int32_t> r(freeRows.begin(), freeRows.end()), map(N);
      CHECK(swept(h, 7, [&] { return asched_nodes_delete(h, k, r.data(), map.data()); }) == 0);
      std::vector<uint8_t> keep(N, 1); for (int i : r) keep[i] = 0;
      for (int j = 0; j < M; j++) if (t.node[j] >= 0) { CHECK(map[t.node[j]] >= 0); t.node[j] = map[t.node[j]]; }
      nd.keepRows(keep);
      counts[13] += (N > 64 && nd.n() <= 64) + (N > 128 && nd.n() <= 128); counts[15] += nd.n() == 1;
    } break;
    default: { curOp = "nodes_append";
      const int k = 1 + below(g, 70);
      for (int e = 0; e < k; e++) { const int src = below(g, N); nd.push(nd.lVal[src], nd.tainted[src]); }
      CHECK(swept(h, 8, [&] { return nd.append(h, N); }) == 0);
      counts[14] += (N <= 64 && nd.n() > 64) + (N <= 128 && nd.n() > 128);
    } break;
    }
    last = compare(h, f, nd, t);
    if (failures) break;
  }
  asched_destroy(h); asched_destroy(f);
}

int main(int argc, char** argv) {
  const int sequences = argc > 1 ? atoi(argv[1]) : 300, steps = argc > 2 ? atoi(argv[2]) : 30, first = argc > 3 ? atoi(argv[3]) : 0;
  static const int32_t indexedCol[3] = {1, 0, 3}, labelKey[1] = {3};
  static const int64_t indexedRes[3] = {1000, MI128, 1};
  static const uint8_t pcPre[3] = {1, 1, 0};
  static const double drf[4] = {1.0, 1.0, 0.0, 1.0};
  asched_config c; memset(&c, 0, sizeof c);
  c.num_resources = R; c.num_indexed = 3; c.indexed_col = indexedCol; c.indexed_resolution = indexedRes;
  c.num_priority_classes = 3; c.pc_priority = pcPrio; c.pc_preemptible = pcPre; c.drf_multiplier = drf; c.device = -1;
  c.num_indexed_taints = -1; c.num_indexed_labels = 1; c.indexed_label_keys = labelKey;
  setvbuf(stdout, nullptr, _IONBF, 0);
  int counts[16] = {0};
  for (int s = first; s < first + sequences && !failures; s++) sequence(c, s, steps, counts);
  static const char* names[9] = {"jobs_append", "jobs_delete", "jobs_patch", "jobs_reprioritise", "req_classes_append", "shapes_compact", "nodes_patch", "nodes_delete", "nodes_append"};
  for (int i = 0; i < 9; i++) printf("%-20s %d calls, %d refusals for memory\n", names[i], counts[i], refusals[i]);
  for (int i = 0; i < 9; i++) if (sequences >= 20 && refusals[i] == 0) { fprintf(stderr, "%s was never refused for memory\n", names[i]); failures++; }
  printf("appends rebuilt %d, reallocated %d; compacts that retired a shape %d, a class %d; node deletes / appends across a word edge %d / %d; tables of one node %d\n",
         counts[9], counts[10], counts[11], counts[12], counts[13], counts[14], counts[15]);
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("resident sequences under ASan + UBSan: %d sequences of %d steps ok\n", sequences, steps);
  return 0;
}
