"""asched_jobs_patch: the run state of resident jobs changes between two scheduling cycles, on the device (armada_amd/csrc/kernels_jobs_patch.h) — the library's
counterpart of txn.Upsert(preemptedJobs) / txn.Upsert(scheduledJobs) (scheduling/scheduling_algo.go:280-283) and of the re-seating of those jobs in the per-queue
sorted sets (jobdb/jobdb.go:572-700).  The contract: after a patch the handle is what jobs_set of the patched table would have left.

a. the per-queue order, pinned against a numpy.lexsort restatement of SchedulingOrderCompare (jobdb/comparison.go:49-107) and against a fresh handle, at the patch sizes
where the passes take another turn; b. two cycles against a fresh handle and the oracle; c. the simulator fixture until it drains; d. refusals; e. a handle that never
patches.  Every case runs on the CPU build of the device code and, marked gpu, on the HIP library."""
import copy
import os

import numpy as np
import pytest

import scenario
from armada_amd import simulator_input as S
from armada_amd import workloads as W
from armada_amd.binding import SchedError, Scheduler

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulator_basic_input.json")


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


# ---------------------------------------------------------------- a. the order, pinned directly
PCS = ((0, True), (1, True), (3, False))
NQ, NN, M = 5, 40, 3011          # queue 3 is empty
CYCLE_TS = 7_000_000_000


class Table:
    """a job table with deliberate ties: few distinct run timestamps (jobs leased in one cycle share one), few distinct submit times, a few queue priorities"""

    def __init__(self, seed=1):
        rng = np.random.default_rng(seed)
        self.cfg = W._config(list(PCS))
        self.node_total = np.tile(np.array([1 << 46, 64_000_000, 1 << 46, 0], dtype=np.int64), (NN, 1))
        self.queue = rng.choice([0, 1, 2, 4], size=M, p=[0.4, 0.3, 0.2, 0.1]).astype(np.int32)
        self.pc = rng.integers(0, 3, size=M).astype(np.int32)
        self.qprio = rng.integers(0, 3, size=M).astype(np.uint32)
        self.submit = rng.integers(0, 40, size=M).astype(np.int64)
        self.req = np.tile(np.array([W.Gi, 1000, 0, 0], dtype=np.int64), (M, 1))
        running = rng.random(M) < 0.5
        self.node = np.where(running, rng.integers(0, NN, size=M), -1).astype(np.int32)
        self.prio = np.where(running, np.array([p for p, _ in PCS])[self.pc], 0).astype(np.int32)
        self.ts = np.where(running, rng.integers(1, 6, size=M) * 1_000_000_000, 0).astype(np.int64)

    def handle(self, lib):
        s = Scheduler(lib, self.cfg)
        s.nodes_upsert(self.node_total)
        s.jobs_set(self.req, queue=self.queue, pc=self.pc, queue_priority=self.qprio, submit_time=self.submit, node=self.node, scheduled_at_priority=self.prio, run_timestamp=self.ts)
        return s

    def restated_order(self, q):
        """jobdb/comparison.go:49-107 over the table: active run first (:52-60), priority-class priority descending (:62-68), queue priority ascending (:70-79), both
        active: run timestamp (:83-90), submit time (:92-97), id (:99-105)"""
        ids = np.nonzero(self.queue == q)[0]
        active = self.node[ids] >= 0
        pcp = np.array([p for p, _ in PCS], dtype=np.int64)[self.pc[ids]]
        t1 = np.where(active, self.ts[ids], self.submit[ids])
        return ids[np.lexsort((ids, self.submit[ids], t1, self.qprio[ids].astype(np.int64), -pcp, ~active))].tolist()

    def patched(self, rows, node, prio, ts):
        t = copy.copy(self)
        t.node, t.prio, t.ts = self.node.copy(), self.prio.copy(), self.ts.copy()
        t.node[rows], t.prio[rows], t.ts[rows] = node, prio, ts
        return t

    def entries(self, rows, rng, ts=CYCLE_TS):
        """queued -> running; running -> no run, or -> another node with a new timestamp"""
        rows = np.asarray(rows, dtype=np.int32)
        was = self.node[rows] >= 0
        stop = was & (rng.random(len(rows)) < 0.5)
        node = np.where(stop, -1, (np.maximum(self.node[rows], 0) + 1 + rng.integers(0, NN - 1, size=len(rows))) % NN).astype(np.int32)
        prio = np.where(stop, 0, np.array([p for p, _ in PCS])[self.pc[rows]]).astype(np.int32)
        return rows, node, prio, np.where(stop, 0, ts).astype(np.int64)


@pytest.fixture(scope="module")
def table():
    return Table()


def _orders(s):
    return [s.scheduling_order(q) for q in range(NQ)]


def _check_order(lib, s, t, what=""):
    got = _orders(s)
    assert got == [t.restated_order(q) for q in range(NQ)], ("restatement", what)
    f = t.handle(lib)
    assert got == _orders(f), ("fresh handle", what)
    f.close()


def test_restatement_is_the_order_of_jobs_set(lib, table):
    """a pin of this file's own reference, not of the feature: the lexsort restatement, which every case below compares a patched handle with, is the order
    asched_jobs_set builds (and the table has the empty queue and the segment sizes the cases rely on).  It calls no jobs_patch, so it also passes without the feature."""
    s = table.handle(lib)
    assert _orders(s) == [table.restated_order(q) for q in range(NQ)] and _orders(s)[3] == [] and all(len(o) > 64 for q, o in enumerate(_orders(s)) if q != 3)
    s.close()


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, M]


@pytest.mark.parametrize("n", SIZES)
def test_order_after_a_patch_of_n_rows(lib, table, n):
    rng = np.random.default_rng(100 + n)
    rows, node, prio, ts = table.entries(rng.permutation(M)[:n], rng)
    if n >= 63:
        was = table.node[rows] >= 0
        assert (~was).any() and (was & (node < 0)).any() and (was & (node >= 0)).any()          # the three kinds of change
    s = table.handle(lib)
    s.jobs_patch(rows, node, prio, ts)
    _check_order(lib, s, table.patched(rows, node, prio, ts), f"n={n}")
    s.close()


def _shaped(table, name):
    """-> (rows, node): a patch by shape; the new runs start at CYCLE_TS at the class priority"""
    q0 = np.array(table.restated_order(0))
    if name == "all jobs of one queue":
        rows = q0
        node = np.where(table.node[rows] >= 0, -1, rows % NN)
    elif name == "first job of a segment":
        rows, node = q0[:1], np.array([-1])                         # (running: the first of the active group)
    elif name == "last job of a segment":
        rows, node = q0[-1:], np.array([5])                         # (queued: the last of the queued group)
    elif name == "the active group becomes empty":
        rows = np.nonzero((table.queue == 1) & (table.node >= 0))[0]
        node = np.full(len(rows), -1)
    elif name == "the queued group becomes empty":
        rows = np.nonzero((table.queue == 2) & (table.node < 0))[0]
        node = rows % NN
    elif name == "first and last row of the table":
        rows, node = np.array([0, M - 1]), np.array([-1 if table.node[0] >= 0 else 3, -1 if table.node[M - 1] >= 0 else 4])
    else:
        raise KeyError(name)
    node = node.astype(np.int32)
    prio = np.where(node >= 0, np.array([p for p, _ in PCS])[table.pc[rows]], 0).astype(np.int32)
    return rows.astype(np.int32), node, prio, np.where(node >= 0, CYCLE_TS, 0).astype(np.int64)


SHAPES = ["all jobs of one queue", "first job of a segment", "last job of a segment", "the active group becomes empty", "the queued group becomes empty", "first and last row of the table"]


@pytest.mark.parametrize("name", SHAPES)
def test_order_after_a_shaped_patch(lib, table, name):
    rows, node, prio, ts = _shaped(table, name)
    assert len(rows) > 0
    if name == "first job of a segment":
        assert table.node[rows[0]] >= 0
    if name == "last job of a segment":
        assert table.node[rows[0]] < 0
    s = table.handle(lib)
    s.jobs_patch(rows, node, prio, ts)
    t = table.patched(rows, node, prio, ts)
    if name == "the active group becomes empty":
        assert not ((t.queue == 1) & (t.node >= 0)).any()
    if name == "the queued group becomes empty":
        assert not ((t.queue == 2) & (t.node < 0)).any()
    _check_order(lib, s, t, name)
    s.close()


def test_two_patches_in_a_row_equal_one_jobs_set(lib, table):
    rng = np.random.default_rng(5)
    s = table.handle(lib)
    e1 = table.entries(rng.permutation(M)[:700], rng, ts=CYCLE_TS)
    t1 = table.patched(*e1)
    s.jobs_patch(*e1)
    rows2 = np.concatenate([e1[0][:300], np.setdiff1d(np.arange(M), e1[0])[:500]])      # 300 rows again, 500 new ones
    e2 = t1.entries(rows2, rng, ts=CYCLE_TS + 10_000_000_000)
    s.jobs_patch(*e2)
    _check_order(lib, s, t1.patched(*e2), "second patch")
    s.jobs_patch([], [])                                           # n == 0: the resets only
    _check_order(lib, s, t1.patched(*e2), "empty patch")
    s.close()


# ---------------------------------------------------------------- b. two cycles against a fresh handle and the oracle
def _second_cycle(wl, r1, seed):
    """the table and queued lists of the cycle after round r1: scheduled rows run on their node since one cycle timestamp, preempted rows have no run, a seeded tenth
    of the running jobs has finished; the queued lists lose the scheduled jobs.  -> (workload of cycle 2, rows that changed)"""
    rng = np.random.default_rng(seed)
    w2 = copy.copy(wl)
    w2.job_node, w2.job_run_prio, w2.job_run_ts = wl.job_node.copy(), wl.job_run_prio.copy(), wl.job_run_ts.copy()
    ts = int(wl.job_run_ts.max()) + 1_000_000_000
    for j, n in r1.scheduled.items():
        w2.job_node[j], w2.job_run_prio[j], w2.job_run_ts[j] = n, r1.scheduled_priority[j], ts
    for j in r1.preempted:
        w2.job_node[j], w2.job_run_prio[j], w2.job_run_ts[j] = -1, 0, 0
    run = np.nonzero(w2.job_node >= 0)[0]
    fin = rng.permutation(run)[:len(run) // 10]
    w2.job_node[fin], w2.job_run_prio[fin], w2.job_run_ts[fin] = -1, 0, 0
    sched = set(r1.scheduled)
    w2.queued = [np.array([j for j in q if int(j) not in sched], dtype=np.int32) for q in wl.queued]
    rows = np.array(sorted(sched | set(r1.preempted) | set(int(j) for j in fin)), dtype=np.int32)
    return w2, rows


def _round(s, wl):
    W.prepare(s, wl)
    r = s.schedule_round()
    return r, s.round_stats()


def _two_cycles(lib, oracle_lib, wl, seed=0, fast=False):
    a = W.load(lib, wl)
    r1, _ = _round(a, wl)
    w2, rows = _second_cycle(wl, r1, seed)
    a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
    ra, sta = _round(a, w2)
    a.close()
    f = W.load(lib, w2)
    rf, stf = _round(f, w2)
    f.close()
    o = W.load(oracle_lib, w2)
    ro, _ = _round(o, w2)
    o.close()
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert ra.fair_share.tobytes() == rf.fair_share.tobytes() == ro.fair_share.tobytes()
    assert ra.demand_capped_adjusted_fair_share.tobytes() == rf.demand_capped_adjusted_fair_share.tobytes() == ro.demand_capped_adjusted_fair_share.tobytes()
    assert sta["fast_iterations"] == stf["fast_iterations"], "the patched handle did not run the fresh handle's fast iterations"
    if fast:
        assert sta["fast_iterations"] > 0
    return r1, ra, rows


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_two_cycles_small_random(lib, oracle_lib, seed):
    wl = W.small_random(n_nodes=40 + 7 * seed, n_jobs=500 + 130 * seed, n_queues=3 + seed, seed=700 + seed, occupied=[0.6, 0.9, 1.0, 0.8][seed - 1], gangs=3 + seed)
    r1, _, rows = _two_cycles(lib, oracle_lib, wl, seed)
    assert len(r1.scheduled) > 0 and len(rows) > 0


def _with_cross_pool_rows(wl, seed, frac=0.3):
    """tests/test_z_cross_pool_away.py with_away: a share of the running jobs belongs to another pool (asched_jobs.away), in an away context beside its queue"""
    rng = np.random.default_rng(seed)
    q = wl.num_queues
    wl = copy.copy(wl)
    running = np.nonzero(np.asarray(wl.job_node) >= 0)[0]
    pick = running[rng.random(len(running)) < frac]
    wl.job_away = np.zeros(wl.num_jobs, dtype=np.uint8)
    wl.job_away[pick] = 1
    wl.job_queue = np.asarray(wl.job_queue).copy()
    wl.job_queue[pick] += q
    wl.queue_weight = np.array(list(wl.queue_weight) + list(wl.queue_weight))
    wl.queued = [np.asarray(x, dtype=np.int32) for x in wl.queued] + [np.zeros(0, np.int32) for _ in range(q)]
    return wl


def test_two_cycles_with_away_node_types(lib, oracle_lib):
    """small_random(away=True): jobs may be placed on a well-known node type at a reduced priority — the patch carries the round's scheduled_priority"""
    wl = W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=711, occupied=0.9, gangs=4, away=True)
    _two_cycles(lib, oracle_lib, wl, 7)


def test_two_cycles_with_cross_pool_away_rows(lib, oracle_lib):
    wl = _with_cross_pool_rows(W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=712, occupied=0.9, gangs=4), 8)
    assert wl.job_away.any()
    r1, _, rows = _two_cycles(lib, oracle_lib, wl, 8)
    assert not any(wl.job_away[j] for j in r1.scheduled) and wl.job_away[rows].any()          # away rows only lose runs, and some do


def test_two_cycles_preemption_heavy(lib, oracle_lib):
    wl = W.config3(2_000, 20_000, occupied=0.95)
    r1, _, _ = _two_cycles(lib, oracle_lib, wl, 11, fast=True)
    assert len(r1.preempted) > 0


def test_two_cycles_gangs(lib, oracle_lib):
    _two_cycles(lib, oracle_lib, W.config3(2_000, 20_000, gangs=200), 12, fast=True)


def test_two_cycles_130_queues(lib, oracle_lib):
    wl = W.config3(seed=3, n_nodes=300, n_jobs=4_000, n_queues=130, gangs=5, occupied=0.5)
    wl.global_burst, wl.queue_burst = 4_000, 120
    _two_cycles(lib, oracle_lib, wl, 13, fast=True)


def test_two_cycles_two_word_keys(lib, oracle_lib):
    """W.fine_indexed: the order key needs two words — a handle without a JobRec table and without the fast structure"""
    wl = W.fine_indexed(n_nodes=500, n_jobs=5_000)
    _two_cycles(lib, oracle_lib, wl, 14)


# ---------------------------------------------------------------- c. many cycles
def _records(cyc):
    return [(c["scheduled"], c["preempted"], c["termination_reason"]) for c in cyc]


def test_simulator_cycles_patched_equal_rebuilt(lib, oracle_lib):
    sim = S.from_fixture(FIXTURE)
    a, b, o = S.run_cycles_patched(lib, sim), S.run_cycles(lib, sim), S.run_cycles(oracle_lib, sim)
    assert len(a) >= 13 and sum(len(c["scheduled"]) for c in a) == 1000
    assert _records(a) == _records(b) == _records(o)


# ---------------------------------------------------------------- d. refusals
def _refused(s, code, *args):
    with pytest.raises(SchedError) as e:
        s.jobs_patch(*args)
    assert e.value.code == code and str(e.value), (e.value.code, str(e.value))


def _refusal_wl():
    return _with_cross_pool_rows(W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=0.9, gangs=3), 9)


def test_refusals_leave_the_handle_as_it_was(lib):
    wl = _refusal_wl()
    clean = W.load(lib, wl)
    want, _ = _round(clean, wl)
    want_order = [clean.scheduling_order(q) for q in range(wl.num_queues)]
    clean.close()
    away = int(np.nonzero(wl.job_away)[0][0])
    queued = int(np.nonzero(wl.job_node < 0)[0][0])
    m, n = wl.num_jobs, wl.num_nodes
    bad = [(ERR_INVALID, [queued, m], [0, 0]),                     # a row outside [0, M)
           (ERR_INVALID, [queued, -1], [0, 0]),
           (ERR_INVALID, [queued, 5, queued], [0, 1, 2]),          # a row named twice
           (ERR_INVALID, [queued], [n]),                           # node outside [-1, N)
           (ERR_INVALID, [5, queued], [0, -2]),
           (ERR_UNSUPPORTED, [queued, away], [0, 1])]              # an away row gains a run
    for code, rows, node in bad:
        s = W.load(lib, wl)
        _refused(s, code, rows, node, [0] * len(rows), [1] * len(rows))
        assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
        got, _ = _round(s, wl)
        scenario.assert_same_round(want, got)
        s.close()
    s = W.load(lib, wl)                                            # the away row may lose its run
    s.jobs_patch([away], [-1])
    s.close()


def test_no_job_table_is_refused(lib):
    wl = _refusal_wl()
    s = Scheduler(lib, wl.config)
    _refused(s, ERR_INVALID, [0], [-1])
    s.nodes_upsert(wl.node_total)
    _refused(s, ERR_INVALID, [], [])
    s.close()
    s = Scheduler(lib, wl.config)                                  # a job table and no node table: N is 0, only "no run" is inside [-1, N)
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, submit_time=wl.job_submit)
    _refused(s, ERR_INVALID, [0], [0])
    s.jobs_patch([0], [-1])
    s.close()


def _market_wl():
    """tests/test_z_evictor_report.py test_market_driven_handle_is_refused: bid prices uniform inside a gang, the queued lists in price order"""
    wl = W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=1.0, gangs=3)
    bids = np.random.default_rng(11).integers(0, 4, size=wl.num_jobs).astype(np.float64)
    for g in set(int(x) for x in wl.job_gang if x >= 0):
        m = np.nonzero(wl.job_gang == g)[0]
        bids[m] = bids[m[0]]
    bids[(wl.job_node >= 0) & np.array([not wl.config.pc_preemptible[p] for p in wl.job_pc])] = 1_000_000.0
    return wl, bids


def _market_round(s, wl, bids):
    pcp = np.asarray(wl.config.pc_priority)
    queued = [sorted(q, key=lambda j: (-int(pcp[wl.job_pc[j]]), -float(bids[j]), int(wl.job_submit[j]), int(j))) for q in wl.queued]
    nq = wl.num_queues
    s.round_prepare(wl.queue_weight, queued, global_tokens=float(wl.global_burst), global_burst=wl.global_burst, global_rate_inf=wl.rate_inf,
                    queue_tokens=[float(wl.queue_burst)] * nq, queue_burst=[wl.queue_burst] * nq, queue_rate_inf=[wl.rate_inf] * nq)
    s.set_market(True, 0.3)
    return s.schedule_round()


@pytest.mark.parametrize("how", ["uploaded with bid prices", "uploaded after set_market"])
def test_market_ordered_job_set_is_refused(lib, how):
    """the job set carries the market order: refused, and the market round that follows is the round of a handle that never saw the call"""
    wl, bids = _market_wl()
    if how == "uploaded after set_market":
        bids = np.zeros(wl.num_jobs)                               # (no bid prices: every job bids 0)

    def handle():
        s = W.load(lib, wl)
        if how == "uploaded with bid prices":
            W.set_jobs(s, wl, bid_price=bids)
        else:
            s.set_market(True, 0.3)
            W.set_jobs(s, wl)
        return s
    clean = handle()
    want_order = [clean.scheduling_order(q) for q in range(wl.num_queues)]
    want = _market_round(clean, wl, bids)
    clean.close()
    assert len(want.scheduled) + len(want.preempted) > 0
    running, queued = int(np.nonzero(wl.job_node >= 0)[0][0]), int(np.nonzero(wl.job_node < 0)[0][0])
    s = handle()
    _refused(s, ERR_UNSUPPORTED, [running, queued], [-1, 3], [0, 0], [0, CYCLE_TS])
    _refused(s, ERR_UNSUPPORTED, [], [])
    assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
    scenario.assert_same_round(want, _market_round(s, wl, bids))
    s.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    s = W.load(oracle_lib, _refusal_wl())
    with pytest.raises(SchedError) as e:
        s.jobs_patch([0], [-1])
    assert "does not export" in str(e.value)
    s.close()


# ---------------------------------------------------------------- e. a handle that never patches
def test_a_round_issues_the_launches_it_issued_before(lib):
    """the counter tests/test_z_evictor_report.py test_switch_off_launches reads: a patched handle's round is launched like a fresh handle's"""
    wl = W.config3(n_nodes=150, n_jobs=2500, n_queues=4, seed=9000, gangs=4, occupied=0.95)
    a = W.load(lib, wl)
    r1, _ = _round(a, wl)
    n1 = a.round_timing()["launches"]
    w2, rows = _second_cycle(wl, r1, 1)
    a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
    _round(a, w2)
    na = a.round_timing()["launches"]
    a.close()
    f = W.load(lib, w2)
    _round(f, w2)
    nf = f.round_timing()["launches"]
    f.close()
    g = W.load(lib, wl)
    _round(g, wl)
    assert g.round_timing()["launches"] == n1 > 10 and na == nf > 10
    g.close()


def test_patch_resets_what_jobs_set_resets(lib):
    """the failed-selection records and the round result of the handle belong to the table as it was: gone after a patch, as after jobs_set"""
    wl = W.config3(n_nodes=150, n_jobs=2500, n_queues=4, seed=9000, gangs=4, occupied=0.95)
    s = W.load(lib, wl)
    r, _ = _round(s, wl)
    on_record = [int(j) for j in np.nonzero(r.job_unschedulable_reason)[0][:200] if s.excluded_nodes(int(j))]
    assert on_record and len(r.preempted) > 0
    s.preemption_causes()
    s.jobs_patch([], [])
    assert all(s.excluded_nodes(j) == [] for j in on_record)
    with pytest.raises(SchedError) as e:
        s.preemption_causes()
    assert e.value.code == ERR_INVALID
    with pytest.raises(SchedError):
        s.schedule_round()                                         # round_prepare first, as after jobs_set
    r2, _ = _round(s, wl)
    scenario.assert_same_round(r, r2)
    s.close()


# ---------------------------------------------------------------- the other readers of run state on a patched handle
def _optimiser_wl(order):
    """tests/test_z_evictor_report.py test_optimiser_round: a full cluster, one preemptible class, every queue protected — the optimiser's phase runs, and which job
    it preempts depends on the ages of the running jobs (now - run_timestamp: jLeaseMs on the device)"""
    rng = np.random.default_rng(3)
    wl = W.small_random(n_nodes=int(rng.integers(6, 40)), n_jobs=int(rng.integers(100, 600)), n_queues=int(rng.integers(2, 6)), seed=3, occupied=1.0, gangs=int(rng.integers(3, 12)))
    wl.config = copy.copy(wl.config); wl.config.protected_fraction_of_fair_share = 1.0
    wl.job_pc[:] = 0
    ids = np.arange(wl.num_jobs, dtype=np.int64)
    wl.job_run_ts = ((ids if order == 0 else wl.num_jobs - 1 - ids) * 7919 % 100003) * 1_000_000
    return wl


def _optimiser_round(s, wl):
    W.prepare(s, wl)
    s.set_optimiser(True, min_improvement_pct=0.0, max_jobs_per_round=60, now_ms=200_000)
    return s.schedule_round()


def test_optimiser_job_ages_after_a_patch(lib, oracle_lib):
    """only run timestamps change (same node, same priority): the optimiser round of the patched handle is the fresh handle's and the oracle's"""
    w0, w1 = _optimiser_wl(0), _optimiser_wl(1)
    run = np.nonzero(w0.job_node >= 0)[0].astype(np.int32)
    s = W.load(lib, w0)
    r0 = _optimiser_round(s, w0)
    s.jobs_patch(run, w1.job_node[run], w1.job_run_prio[run], w1.job_run_ts[run])
    ra = _optimiser_round(s, w1)
    s.close()
    f, o = W.load(lib, w1), W.load(oracle_lib, w1)
    rf, ro = _optimiser_round(f, w1), _optimiser_round(o, w1)
    f.close(); o.close()
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert 6 in set(ra.scheduled_method.values())                  # ASCHED_METHOD_OPTIMISER: the optimiser's phase ran
    assert ra.preempted != r0.preempted, "the two sets of run timestamps give the same round: the case pins nothing"


def test_nodedb_calls_and_submit_check_after_a_patch(lib):
    """between the patch and round_prepare the handle is the empty NodeDb jobs_set leaves: first fits, a selection with its binding, a submit check"""
    wl = W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=713, occupied=0.9, gangs=4)
    a = W.load(lib, wl)
    r1, _ = _round(a, wl)
    w2, rows = _second_cycle(wl, r1, 3)
    a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
    f = W.load(lib, w2)
    jobs = np.arange(0, wl.num_jobs, 3, dtype=np.int32)
    single = [int(j) for j in jobs if wl.job_gang[j] < 0]
    units = [[j] for j in single[:60]]
    for s in (a, f):
        s.out = [s.fit_select_batch(jobs).tolist(), s.submit_check(units)]
        picked = s.select_node(single[0])
        assert picked[0].node >= 0
        s.out += [repr(picked), s.get_alloc(picked[0].node).tolist(), s.get_alloc(0).tolist()]
    assert a.out == f.out
    ra, _ = _round(a, w2)
    rf, _ = _round(f, w2)
    scenario.assert_same_round(rf, ra)
    a.close(); f.close()
