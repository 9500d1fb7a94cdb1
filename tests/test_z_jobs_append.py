"""asched_jobs_append: newly submitted jobs enter the resident job table between two scheduling cycles, on the device (armada_amd/csrc/kernels_jobs_append.h) — the
library's counterpart of syncState's upsert of the new jobs into the jobDb (scheduler.go:478-535; jobdb/jobdb.go:572-700, the insertion into the per-queue sorted set at
:691-700).  The contract: after an append the handle is what jobs_set of the concatenated table would have left.

a. the per-queue order, pinned against a numpy.lexsort restatement of SchedulingOrderCompare (jobdb/comparison.go:49-107) and against a fresh handle, at the batch sizes
where the sort and the merge take another turn; b. capacity; c. cycles against a fresh handle and the oracle, with known shapes only and with any shape; d. interplay with
jobs_patch, nodes_upsert, jobs_set and the NodeDb-level calls; e. refusals; f. the simulator fixture with its jobs arriving a cycle's worth at a time.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library."""
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
PCP = np.array([p for p, _ in PCS], dtype=np.int64)
NQ, NN, M = 5, 40, 3011          # queue 3 is empty
REQ = np.array([W.Gi, 1000, 0, 0], dtype=np.int64)          # one request shape


class Table:
    """a job table with deliberate ties: few distinct submit times, a few queue priorities, few distinct run timestamps; half of the rows run"""
    FIELDS = ("queue", "pc", "qprio", "submit", "req", "node", "prio", "ts")

    def __init__(self, seed=1, m=M):
        rng = np.random.default_rng(seed)
        self.cfg = W._config(list(PCS))
        self.node_total = np.tile(np.array([1 << 46, 64_000_000, 1 << 46, 0], dtype=np.int64), (NN, 1))
        self.queue = rng.choice([0, 1, 2, 4], size=m, p=[0.4, 0.3, 0.2, 0.1]).astype(np.int32)
        self.pc = rng.integers(0, 3, size=m).astype(np.int32)
        self.qprio = rng.integers(0, 3, size=m).astype(np.uint32)
        self.submit = rng.integers(0, 40, size=m).astype(np.int64)
        self.req = np.tile(REQ, (m, 1))
        running = rng.random(m) < 0.5
        self.node = np.where(running, rng.integers(0, NN, size=m), -1).astype(np.int32)
        self.prio = np.where(running, PCP[self.pc], 0).astype(np.int32)
        self.ts = np.where(running, rng.integers(1, 6, size=m) * 1_000_000_000, 0).astype(np.int64)

    @property
    def m(self):
        return len(self.queue)

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
        t1 = np.where(active, self.ts[ids], self.submit[ids])
        return ids[np.lexsort((ids, self.submit[ids], t1, self.qprio[ids].astype(np.int64), -PCP[self.pc[ids]], ~active))].tolist()

    def batch(self, m, rng, queue=None, pc=None, qprio=None, submit=None):
        """m newly submitted rows: queued, the table's request shape, ties with the resident rows in submit time and queue priority unless said otherwise"""
        pick = lambda v, d: d if v is None else np.broadcast_to(np.asarray(v), (m,))
        return dict(queue=pick(queue, rng.choice([0, 1, 2, 4], size=m)).astype(np.int32), pc=pick(pc, rng.integers(0, 3, size=m)).astype(np.int32),
                    qprio=pick(qprio, rng.integers(0, 3, size=m)).astype(np.uint32), submit=pick(submit, rng.integers(0, 40, size=m)).astype(np.int64),
                    req=np.tile(REQ, (m, 1)))

    def append_to(self, s, b):
        s.jobs_append(b["req"], queue=b["queue"], pc=b["pc"], queue_priority=b["qprio"], submit_time=b["submit"])

    def concatenated(self, b):
        """the table jobs_set would be given: the resident rows, then the batch as queued rows"""
        t = copy.copy(self)
        m = len(b["queue"])
        for f in ("queue", "pc", "qprio", "submit", "req"):
            setattr(t, f, np.concatenate([getattr(self, f), b[f]]))
        t.node = np.concatenate([self.node, np.full(m, -1, np.int32)])
        t.prio = np.concatenate([self.prio, np.zeros(m, np.int32)])
        t.ts = np.concatenate([self.ts, np.zeros(m, np.int64)])
        return t


@pytest.fixture(scope="module")
def table():
    return Table()


def _orders(s, nq=NQ):
    return [s.scheduling_order(q) for q in range(nq)]


def _check_order(lib, s, t, what="", nq=NQ):
    got = _orders(s, nq)
    assert got == [t.restated_order(q) for q in range(nq)], ("restatement", what)
    f = t.handle(lib)
    assert got == _orders(f, nq), ("fresh handle", what)
    f.close()


def test_restatement_is_the_order_of_jobs_set(lib, table):
    """a pin of this file's own reference, not of the feature: the lexsort restatement, which every case below compares an appended handle with, is the order
    asched_jobs_set builds — of the table and of a concatenated one.  It calls no jobs_append, so it also passes without the feature."""
    s = table.handle(lib)
    assert _orders(s) == [table.restated_order(q) for q in range(NQ)] and _orders(s)[3] == [] and all(len(o) > 64 for q, o in enumerate(_orders(s)) if q != 3)
    s.close()
    t = table.concatenated(table.batch(300, np.random.default_rng(2)))
    s = t.handle(lib)
    assert t.m == M + 300 and _orders(s) == [t.restated_order(q) for q in range(NQ)]
    s.close()


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000]


@pytest.mark.parametrize("m", SIZES)
def test_order_after_an_append_of_m_rows(lib, table, m):
    b = table.batch(m, np.random.default_rng(100 + m))
    s = table.handle(lib)
    table.append_to(s, b)
    st = s.jobs_append_stats()
    assert (st["rows"], st["in_order"], st["new_shapes"], st["new_gangs"], st["rebuilt"]) == (m, m, 0, 0, 0) and st["capacity"] >= M + m
    assert s.num_jobs == M + m
    _check_order(lib, s, table.concatenated(b), f"m={m}")
    s.close()


def _shaped(table, name, rng):
    q0 = table.restated_order(0)
    queued0 = [j for j in q0 if table.node[j] < 0]
    if name == "every row into the empty queue":
        return table.batch(200, rng, queue=3)
    if name == "every row into a queue above all earlier ones":
        return table.batch(200, rng, queue=7)
    if name == "rows before and after every queued job of their queue":
        first = table.batch(40, rng, queue=0, pc=2, qprio=0, submit=-5)          # highest class priority, queue priority 0, earliest submit
        last = table.batch(40, rng, queue=0, pc=0, qprio=9, submit=1000)
        return {k: np.concatenate([first[k], last[k]]) for k in first}
    if name == "submit times equal to resident rows'":
        rows = np.array(queued0[:150])
        return table.batch(150, rng, queue=0, pc=table.pc[rows], qprio=table.qprio[rows], submit=table.submit[rows])
    if name == "a batch not sorted by submit time":
        return table.batch(300, rng, submit=np.arange(300, 0, -1) * 7 % 101)
    if name == "rows of no queue only":
        return table.batch(100, rng, queue=-1)
    raise KeyError(name)


SHAPES = ["every row into the empty queue", "every row into a queue above all earlier ones", "rows before and after every queued job of their queue",
          "submit times equal to resident rows'", "a batch not sorted by submit time", "rows of no queue only"]


@pytest.mark.parametrize("name", SHAPES)
def test_order_after_a_shaped_append(lib, table, name):
    b = _shaped(table, name, np.random.default_rng(7))
    s = table.handle(lib)
    before = _orders(s, 8)
    table.append_to(s, b)
    t = table.concatenated(b)
    after = _orders(s, 8)
    if name == "rows of no queue only":
        assert after == before and s.jobs_append_stats()["in_order"] == 0
    if name == "every row into the empty queue":
        assert before[3] == [] and len(after[3]) == 200
    if name == "every row into a queue above all earlier ones":
        assert len(after[7]) == 200 and after[5] == after[6] == []
    if name == "rows before and after every queued job of their queue":
        queued = [j for j in after[0] if t.node[j] < 0]
        assert all(j >= M for j in queued[:40]) and all(j >= M for j in queued[-40:]) and not any(j >= M for j in queued[40:-40])
    _check_order(lib, s, t, name, nq=8)
    s.close()


# ---------------------------------------------------------------- b. capacity
def test_six_growing_appends(lib, table):
    rng = np.random.default_rng(11)
    s = table.handle(lib)
    t = table
    stats = []
    for k in range(6):
        b = t.batch(700, rng)
        rows_before = t.m
        t.append_to(s, b)
        t = t.concatenated(b)
        st = s.jobs_append_stats()
        stats.append(st)
        assert st["capacity"] >= t.m
        if st["reallocated"]:
            assert st["capacity"] >= 1.25 * rows_before, st
        _check_order(lib, s, t, f"append {k}")
    assert stats[0]["reallocated"] == 1, "jobs_set allocates exactly M: the first append cannot fit"
    assert any(not st["reallocated"] for st in stats), stats
    s.close()


def _round(s, wl):
    W.prepare(s, wl)
    r = s.schedule_round()
    return r, s.round_stats()


def test_a_handle_that_never_appends_launches_what_it_launched_before(lib):
    """tests/test_z_jobs_patch.py test_a_round_issues_the_launches_it_issued_before: the launch counter of a round on a handle that was only ever given jobs_set, against
    a handle that appended the tail of the same table"""
    wl = W.config3(n_nodes=150, n_jobs=2500, n_queues=4, seed=9000, gangs=4, occupied=0.95)
    full, head, tail = _split(wl, "known")
    g = W.load(lib, full)
    _round(g, full)
    n_set = g.round_timing()["launches"]
    g.close()
    a = W.load(lib, head)
    _append_tail(a, full, tail)
    _round(a, full)
    n_app = a.round_timing()["launches"]
    a.close()
    assert n_set == n_app > 10


# ---------------------------------------------------------------- c. cycles against a fresh handle and the oracle
def _shape_keys(wl, rows):
    cls = np.zeros(wl.num_jobs, np.int64) if wl.job_req_class is None else np.asarray(wl.job_req_class, dtype=np.int64)
    return [(int(cls[j]), int(wl.job_pc[j])) + tuple(int(x) for x in wl.job_req[j]) for j in rows]


def _permuted(wl, perm):
    """the workload with row perm[k] as row k: every per-job array, the queued lists renumbered and put back into SchedulingOrderCompare order (the row is its last key)"""
    new_of = np.empty(wl.num_jobs, np.int64)
    new_of[perm] = np.arange(wl.num_jobs)
    w = copy.copy(wl)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class", "job_away"):
        v = getattr(wl, f)
        if v is not None:
            setattr(w, f, np.asarray(v)[perm].copy())
    pcp = np.asarray(wl.config.pc_priority)[w.job_pc]
    w.queued = []
    for q in wl.queued:
        ids = new_of[np.asarray(q, dtype=np.int64)]
        w.queued.append(ids[np.lexsort((ids, w.job_submit[ids], -pcp[ids]))].astype(np.int32))
    return w


def _head_of(full, mh):
    w = copy.copy(full)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class", "job_away"):
        v = getattr(full, f)
        if v is not None:
            setattr(w, f, np.asarray(v)[:mh].copy())
    w.queued = [np.asarray(q, dtype=np.int32)[np.asarray(q) < mh] for q in full.queued]
    return w


def _cut(full, near):
    """the first row count >= near that splits no gang (a gang is submitted in one piece)"""
    gk = [(int(q), int(g)) for q, g in zip(full.job_queue, full.job_gang)]
    c = near
    while any(g[1] >= 0 and g in set(gk[:c]) for g in gk[c:]):
        c += 1
    return c


def _split(wl, mode, gangs=False, seed=5):
    """moves a seeded tenth of the queued single jobs (gangs: and a seeded tenth of the queued gangs, whole) to the end of the table.  mode "known": drawn rows whose
    scheduling-key shape has no row left in the head are dropped from the draw.  -> (the whole table, its head, the tail's rows); asserts the tail kept >= 75 % of the draw"""
    rng = np.random.default_rng(seed)
    queued = np.nonzero(np.asarray(wl.job_node) < 0)[0]
    single = queued[np.asarray(wl.job_gang)[queued] < 0]
    drawn = set(int(j) for j in rng.permutation(single)[:max(1, len(single) // 10)])
    if gangs:
        keys = sorted(set((int(wl.job_queue[j]), int(wl.job_gang[j])) for j in queued if wl.job_gang[j] >= 0))
        for k in rng.permutation(len(keys))[:max(1, len(keys) // 10)]:
            drawn |= set(int(j) for j in queued if (int(wl.job_queue[j]), int(wl.job_gang[j])) == keys[k])
    n_drawn = len(drawn)
    if mode == "known":
        rest = set(_shape_keys(wl, [j for j in range(wl.num_jobs) if j not in drawn]))
        keep = set()
        for j in sorted(drawn):
            if all(k in rest for k in _shape_keys(wl, [j])):
                keep.add(j)
        if gangs:      # whole gangs only
            for j in list(keep):
                if wl.job_gang[j] >= 0 and any((int(wl.job_queue[i]), int(wl.job_gang[i])) == (int(wl.job_queue[j]), int(wl.job_gang[j])) and i not in keep for i in drawn):
                    keep.discard(j)
        drawn = keep
    assert len(drawn) >= 0.75 * n_drawn and len(drawn) > 0, (len(drawn), n_drawn)
    tail_old = np.array(sorted(drawn), dtype=np.int64)
    perm = np.concatenate([np.array([j for j in range(wl.num_jobs) if j not in drawn], dtype=np.int64), tail_old])
    full = _permuted(wl, perm)
    mh = wl.num_jobs - len(tail_old)
    return full, _head_of(full, mh), np.arange(mh, wl.num_jobs)


def _append_tail(s, full, tail):
    s.jobs_append(full.job_req[tail], queue=full.job_queue[tail], pc=full.job_pc[tail], submit_time=full.job_submit[tail], gang_id=full.job_gang[tail],
                  gang_cardinality=full.job_gang_card[tail], req_class=None if full.job_req_class is None else np.asarray(full.job_req_class)[tail])
    return s.jobs_append_stats()


def _second_cycle(full, r1, seed):
    """the table and queued lists of the cycle after round r1 (run on the head: its rows are the whole table's first rows): scheduled rows run, preempted rows have no
    run, a seeded tenth of the running jobs has finished.  -> (workload of cycle 2, rows whose run state changed)"""
    rng = np.random.default_rng(seed)
    w2 = copy.copy(full)
    w2.job_node, w2.job_run_prio, w2.job_run_ts = full.job_node.copy(), full.job_run_prio.copy(), full.job_run_ts.copy()
    ts = int(full.job_run_ts.max()) + 1_000_000_000
    for j, n in r1.scheduled.items():
        w2.job_node[j], w2.job_run_prio[j], w2.job_run_ts[j] = n, r1.scheduled_priority[j], ts
    for j in r1.preempted:
        w2.job_node[j], w2.job_run_prio[j], w2.job_run_ts[j] = -1, 0, 0
    run = np.nonzero(w2.job_node >= 0)[0]
    fin = rng.permutation(run)[:len(run) // 10]
    w2.job_node[fin], w2.job_run_prio[fin], w2.job_run_ts[fin] = -1, 0, 0
    sched = set(r1.scheduled)
    w2.queued = [np.array([j for j in q if int(j) not in sched], dtype=np.int32) for q in full.queued]
    rows = np.array(sorted(sched | set(r1.preempted) | set(int(j) for j in fin)), dtype=np.int32)
    return w2, rows


def _arriving_cycle(lib, oracle_lib, wl, mode, seed=0, gangs=False, fast=False):
    full, head, tail = _split(wl, mode, gangs=gangs)
    a = W.load(lib, head)
    r1, _ = _round(a, head)
    w2, rows = _second_cycle(full, r1, seed)
    a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
    st = _append_tail(a, full, tail)
    assert st["rows"] == len(tail)
    if mode == "known":
        assert st["new_shapes"] == 0 and st["rebuilt"] == 0, st
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
    assert sta["fast_iterations"] == stf["fast_iterations"], "the appended handle did not run the fresh handle's fast iterations"
    if fast:
        assert sta["fast_iterations"] > 0
    appended = [j for j in ra.scheduled if j >= len(head.job_queue)]
    assert appended, "no appended job was scheduled in round 2: the case pins nothing"
    if gangs:
        assert any(full.job_gang[j] >= 0 for j in appended), "no appended gang was scheduled in round 2"
    return st


MODES = ["known", "any"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_arriving_cycle_small_random(lib, oracle_lib, seed, mode):
    wl = W.small_random(n_nodes=40 + 7 * seed, n_jobs=500 + 130 * seed, n_queues=3 + seed, seed=700 + seed, occupied=[0.6, 0.9, 1.0, 0.8][seed - 1], gangs=3 + seed)
    st = _arriving_cycle(lib, oracle_lib, wl, mode, seed)
    if mode == "any":
        assert st["new_shapes"] > 0 and st["rebuilt"] == 1, st


@pytest.mark.parametrize("mode", MODES)
def test_arriving_cycle_preemption_heavy(lib, oracle_lib, mode):
    _arriving_cycle(lib, oracle_lib, W.config3(2_000, 20_000, occupied=0.95), mode, 11, fast=True)


@pytest.mark.parametrize("mode", MODES)
def test_arriving_cycle_gangs(lib, oracle_lib, mode):
    st = _arriving_cycle(lib, oracle_lib, W.config3(2_000, 20_000, gangs=200), mode, 12, gangs=True, fast=True)
    assert st["new_gangs"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_arriving_cycle_130_queues(lib, oracle_lib, mode):
    wl = W.config3(seed=3, n_nodes=300, n_jobs=4_000, n_queues=130, gangs=5, occupied=0.5)
    wl.global_burst, wl.queue_burst = 4_000, 120
    _arriving_cycle(lib, oracle_lib, wl, mode, 13, fast=True)


@pytest.mark.parametrize("mode", MODES)
def test_arriving_cycle_two_word_keys(lib, oracle_lib, mode):
    """W.fine_indexed: the order key needs two words — a handle without a JobRec table and without the fast structure"""
    _arriving_cycle(lib, oracle_lib, W.fine_indexed(n_nodes=500, n_jobs=5_000), mode, 14)


@pytest.mark.parametrize("mode", MODES)
def test_arriving_cycle_with_away_node_types(lib, oracle_lib, mode):
    _arriving_cycle(lib, oracle_lib, W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=711, occupied=0.9, gangs=4, away=True), mode, 7)


# ---------------------------------------------------------------- d. interplay
def _interplay_wl():
    return W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=713, occupied=0.9, gangs=4)


def _same_as_fresh(lib, a, w2):
    f = W.load(lib, w2)
    assert [a.scheduling_order(q) for q in range(w2.num_queues)] == [f.scheduling_order(q) for q in range(w2.num_queues)]
    ra, _ = _round(a, w2)
    rf, _ = _round(f, w2)
    scenario.assert_same_round(rf, ra)
    f.close()
    return ra


@pytest.mark.parametrize("first", ["append", "patch"])
def test_append_and_patch_in_either_order(lib, first):
    """append, then a patch that names old and new rows; patch, then append"""
    full, head, tail = _split(_interplay_wl(), "any")
    a = W.load(lib, head)
    r1, _ = _round(a, head)
    w2, rows = _second_cycle(full, r1, 3)
    if first == "append":
        _append_tail(a, full, tail)
        lease = tail[:5].astype(np.int32)                       # some of the new rows start to run as well
        w2.job_node[lease], w2.job_run_prio[lease], w2.job_run_ts[lease] = 1, np.asarray(full.config.pc_priority)[full.job_pc[lease]], int(w2.job_run_ts.max())
        leased = set(int(j) for j in lease)
        w2.queued = [np.array([j for j in q if int(j) not in leased], dtype=np.int32) for q in w2.queued]
        rows = np.concatenate([rows, lease]).astype(np.int32)
        a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
    else:
        a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
        _append_tail(a, full, tail)
    _same_as_fresh(lib, a, w2)
    a.close()


def test_append_then_nodes_upsert(lib):
    """the masks and the fast structure are rebuilt from the grown host mirrors"""
    full, head, tail = _split(_interplay_wl(), "known")
    a = W.load(lib, head)
    _append_tail(a, full, tail)
    a.nodes_upsert(full.node_total, full.node_allocatable, taints=full.node_taints, labels=full.node_labels, id_rank=full.node_id_rank)
    _same_as_fresh(lib, a, full)
    a.close()


def test_append_then_jobs_set_of_a_smaller_table(lib):
    full, head, tail = _split(_interplay_wl(), "any")
    a = W.load(lib, head)
    _append_tail(a, full, tail)
    c1, c2 = _cut(full, 300), _cut(full, 400)
    small = _head_of(full, c1)
    W.set_jobs(a, small)
    assert a.jobs_append_stats()["rows"] == 0
    _same_as_fresh(lib, a, small)
    _append_tail(a, full, np.arange(c1, c2))                     # and the smaller table grows again
    _same_as_fresh(lib, a, _head_of(full, c2))
    a.close()


def test_append_without_a_node_table_then_nodes_upsert(lib):
    full, head, tail = _split(_interplay_wl(), "any")
    a = Scheduler(lib, head.config)
    W.set_jobs(a, head)
    _append_tail(a, full, tail)
    a.nodes_upsert(full.node_total, full.node_allocatable, taints=full.node_taints, labels=full.node_labels, id_rank=full.node_id_rank)
    _same_as_fresh(lib, a, full)
    a.close()


@pytest.mark.parametrize("mode", MODES)
def test_nodedb_calls_and_submit_check_after_an_append(lib, mode):
    """between the append and round_prepare the handle is the empty NodeDb jobs_set leaves: first fits, a selection with its binding, a submit check — old and new rows"""
    full, head, tail = _split(_interplay_wl(), mode)
    a = W.load(lib, head)
    _round(a, head)
    _append_tail(a, full, tail)
    f = W.load(lib, full)
    jobs = np.concatenate([np.arange(0, len(head.job_queue), 3), tail]).astype(np.int32)
    single = [int(j) for j in jobs if full.job_gang[j] < 0]
    units = [[j] for j in single[:40] + single[-20:]]
    for s in (a, f):
        s.out = [s.fit_select_batch(jobs).tolist(), s.submit_check(units)]
        picked = s.select_node(single[-1])
        assert picked[0].node >= 0
        s.out += [repr(picked), s.get_alloc(picked[0].node).tolist(), s.get_alloc(0).tolist()]
    assert a.out == f.out
    _same_as_fresh(lib, a, full)
    a.close(); f.close()


def test_append_resets_what_jobs_set_resets(lib):
    """the failed-selection records and the round result of the handle belong to the table as it was: gone after an append, as after jobs_set"""
    wl = W.config3(n_nodes=150, n_jobs=2500, n_queues=4, seed=9000, gangs=4, occupied=0.95)
    full, head, tail = _split(wl, "known")
    s = W.load(lib, head)
    r, _ = _round(s, head)
    on_record = [int(j) for j in np.nonzero(r.job_unschedulable_reason)[0][:200] if s.excluded_nodes(int(j))]
    assert on_record and len(r.preempted) > 0
    s.preemption_causes()
    for tail_rows in (tail[:0], tail):                            # m == 0: the resets only; then the tail
        _append_tail(s, full, tail_rows)
        assert all(s.excluded_nodes(j) == [] for j in on_record)
        with pytest.raises(SchedError) as e:
            s.preemption_causes()
        assert e.value.code == ERR_INVALID
        with pytest.raises(SchedError):
            s.schedule_round()                                     # round_prepare first, as after jobs_set
        if len(tail_rows) == 0:
            r2, _ = _round(s, head)
            scenario.assert_same_round(r, r2)
            assert [int(j) for j in on_record if s.excluded_nodes(j)]
    _same_as_fresh(lib, s, full)
    s.close()


# ---------------------------------------------------------------- e. refusals
def _refusal_wl():
    return W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=0.9, gangs=3)


def test_refusals_leave_the_handle_as_it_was(lib):
    wl = _refusal_wl()
    clean = W.load(lib, wl)
    want_order = [clean.scheduling_order(q) for q in range(wl.num_queues)]
    want, _ = _round(clean, wl)
    clean.close()
    R = wl.job_req.shape[1]
    ok = wl.job_req[:2]
    gang_row = int(np.nonzero(wl.job_gang >= 0)[0][0])
    new_shape = np.array([[3 * W.Gi + 12345, 7000, 0, 0][:R] + [0] * (R - 4)] * 2, dtype=np.int64)
    bad = [(ERR_INVALID, dict(req=ok, pc=[0, len(wl.config.pc_priority)])),                       # pc out of range
           (ERR_INVALID, dict(req=ok, pc=[-1, 0])),
           (ERR_INVALID, dict(req=ok, req_class=[0, 99])),                                         # req_class out of range
           (ERR_INVALID, dict(req=new_shape, req_class=[0, -1])),                                  # (with a request vector the table does not hold: still refused in the validation loop, before any shape is looked up)
           (ERR_INVALID, dict(req=ok, queue=[0, -2])),                                             # a queue below -1
           (ERR_INVALID, dict(req=ok, node=[-1, 0])),                                              # a row has a run
           (ERR_INVALID, dict(req=ok, scheduled_at_priority=[0, 1])),
           (ERR_INVALID, dict(req=ok, run_timestamp=[5, 0])),
           (ERR_INVALID, dict(req=ok, away=[0, 1])),                                               # a row flagged away
           (ERR_UNSUPPORTED, dict(req=ok, bid_price=[1.0, 2.0])),                                  # bid prices
           (ERR_UNSUPPORTED, dict(req=new_shape, queue=[int(wl.job_queue[gang_row])] * 2, gang_id=[77, int(wl.job_gang[gang_row])], gang_cardinality=[2, 2]))]   # joins a resident gang
    for code, kw in bad:
        s = W.load(lib, wl)
        with pytest.raises(SchedError) as e:
            s.jobs_append(**kw)
        assert e.value.code == code and str(e.value), (kw, e.value.code, str(e.value))
        assert s.num_jobs == wl.num_jobs
        assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
        got, _ = _round(s, wl)
        scenario.assert_same_round(want, got)
        s.jobs_append(new_shape[:1], queue=[0], pc=[0])                                            # and the handle still appends
        s.close()


def test_missing_req_negative_m_and_too_many_rows_are_refused(lib):
    """through the C structure: the binding cannot express them.  M + m above 2^30 is refused before any row is read (the one row behind `req` is all there is)"""
    import ctypes as C
    from armada_amd.binding import CJobs
    wl = _refusal_wl()
    f = W.load(lib, wl)
    want_order = [f.scheduling_order(q) for q in range(wl.num_queues)]
    want, _ = _round(f, wl)
    f.close()
    one = np.ascontiguousarray(wl.job_req[:1], dtype=np.int64)
    for m, req, code in ((2, None, ERR_INVALID),                   # req is missing
                         (-1, one, ERR_INVALID),
                         (1 << 30, one, ERR_UNSUPPORTED),          # M + m exceeds 2^30
                         ((1 << 30) - wl.num_jobs + 1, one, ERR_UNSUPPORTED)):   # by one row
        s = W.load(lib, wl)
        j = CJobs()
        j.m = m
        if req is not None:
            j.req = req.ctypes.data_as(C.POINTER(C.c_int64))
        assert getattr(s.lib, "jobs_append")(s.h, C.byref(j)) == code, m
        assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
        got, _ = _round(s, wl)
        scenario.assert_same_round(want, got)
        s.close()


# a refusal that comes AFTER the shape lookup: the new shape is in the host's shape table, the mirrors are grown and the key layout is re-derived when the host finds
# that the rebuild would refuse — all of it has to be put back
LIT_TMAX = 64   # armada_amd/csrc/dev.h


class ManyTypes:
    """130 nodes of LIT_TMAX + 1 node types (an indexed label), every type populated, allocatable on the index grid and node ids in index order: a request on the grid
    iterates by packed keys whatever the number of types, one off the grid takes the literal iteration path, which serves at most LIT_TMAX types"""

    def __init__(self):
        self.cfg = W._config(list(PCS))
        self.cfg.indexed_label_keys = [3]
        n = 2 * (LIT_TMAX + 1)
        self.node_total = np.tile(np.array([1 << 46, 64_000, 1 << 46, 0], dtype=np.int64), (n, 1))
        self.labels = [[(3, i % (LIT_TMAX + 1))] for i in range(n)]
        m = 50
        self.req = np.tile(REQ, (m, 1))
        self.req[::2, W.CPU] = 2000
        self.queue = (np.arange(m) % 3).astype(np.int32)
        self.pc = (np.arange(m) // 2 % 2).astype(np.int32)          # (both request vectors in both classes)
        self.submit = (np.arange(m) * 7 % 11).astype(np.int64)

    def handle(self, lib, extra=()):
        s = Scheduler(lib, self.cfg)
        s.nodes_upsert(self.node_total, labels=self.labels)
        cat = lambda f: np.concatenate([getattr(self, f)] + [b[f] for b in extra])
        s.jobs_set(cat("req"), queue=cat("queue"), pc=cat("pc"), submit_time=cat("submit"))
        return s

    def batch(self, cpus, queue, submit):
        k = len(cpus)
        req = np.tile(REQ, (k, 1))
        req[:, W.CPU] = cpus
        return dict(req=req, queue=np.full(k, queue, np.int32), pc=np.zeros(k, np.int32), submit=np.full(k, submit, np.int64))

    def view(self, s, nq=4):
        jobs = np.arange(s.num_jobs, dtype=np.int32)
        return [s.scheduling_order(q) for q in range(nq)], s.fit_select_batch(jobs).tolist(), s.num_jobs, s.node_types_matching_job(0)[0]


def test_refusal_after_the_shape_lookup_puts_everything_back(lib):
    t = ManyTypes()
    off_grid = t.batch([3000, 1500, 1000], 1, 3)                   # a new shape on the grid, then one off it, then a resident one
    known, fresh_shape = t.batch([1000, 2000], 2, 1), t.batch([5000, 5000, 1000], 3, 0)
    a = t.handle(lib)
    f = t.handle(lib)
    want = t.view(f)
    assert want[3] == LIT_TMAX + 1
    for _ in range(2):                                             # (twice: the second call finds whatever the first left)
        with pytest.raises(SchedError) as e:
            a.jobs_append(off_grid["req"], queue=off_grid["queue"], pc=off_grid["pc"], submit_time=off_grid["submit"])
        assert e.value.code == ERR_UNSUPPORTED and "LIT_TMAX" in str(e.value), (e.value.code, str(e.value))
        assert t.view(a) == want
    f.close()
    extra = []
    for b, shapes in ((known, 0), (fresh_shape, 1)):               # the handle still appends: known shapes on the device, then a new shape on the grid
        a.jobs_append(b["req"], queue=b["queue"], pc=b["pc"], submit_time=b["submit"])
        st = a.jobs_append_stats()
        assert (st["rows"], st["new_shapes"], st["rebuilt"]) == (len(b["queue"]), shapes, int(shapes > 0)), st
        extra.append(b)
        f = t.handle(lib, extra)
        assert t.view(a) == t.view(f)
        f.close()
    f = t.handle(lib, extra)
    m = a.num_jobs
    queued = [[j for j in a.scheduling_order(q)] for q in range(4)]
    for s in (a, f):
        s.round_prepare(np.ones(4), queued, global_tokens=1e18, global_burst=1 << 62, global_rate_inf=True, queue_tokens=[1e18] * 4, queue_burst=[1 << 62] * 4, queue_rate_inf=[True] * 4)
    ra, rf = a.schedule_round(), f.schedule_round()
    scenario.assert_same_round(rf, ra)
    assert len(ra.scheduled) == m
    a.close(); f.close()


def test_no_job_table_is_refused(lib):
    wl = _refusal_wl()
    s = Scheduler(lib, wl.config)
    for req in (wl.job_req[:1], wl.job_req[:0]):
        with pytest.raises(SchedError) as e:
            s.jobs_append(req)
        assert e.value.code == ERR_INVALID
    s.nodes_upsert(wl.node_total)
    with pytest.raises(SchedError) as e:
        s.jobs_append(wl.job_req[:1])
    assert e.value.code == ERR_INVALID
    s.close()


@pytest.mark.parametrize("how", ["uploaded with bid prices", "uploaded after set_market"])
def test_market_ordered_job_set_is_refused(lib, how):
    wl = _refusal_wl()
    s = W.load(lib, wl)
    if how == "uploaded with bid prices":
        W.set_jobs(s, wl, bid_price=np.ones(wl.num_jobs))
    else:
        s.set_market(True, 0.3)
        W.set_jobs(s, wl)
    want_order = [s.scheduling_order(q) for q in range(wl.num_queues)]
    for req in (wl.job_req[:3], wl.job_req[:0]):
        with pytest.raises(SchedError) as e:
            s.jobs_append(req)
        assert e.value.code == ERR_UNSUPPORTED
    assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order and s.num_jobs == wl.num_jobs
    s.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = _refusal_wl()
    s = W.load(oracle_lib, wl)
    for call in (lambda: s.jobs_append(wl.job_req[:1]), s.jobs_append_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    s.close()


# ---------------------------------------------------------------- f. the simulator fixture, its jobs arriving a cycle's worth at a time
def _records(cyc):
    return [(c["scheduled"], c["preempted"], c["termination_reason"], c["rows"]) for c in cyc]


def test_simulator_cycles_arriving_equal_rebuilt(lib, oracle_lib):
    sim = S.from_fixture(FIXTURE)
    per_cycle = 90                                                 # (the fixture's cluster leases about this many jobs a cycle: arrivals keep up with the rounds)
    a = S.run_cycles_arriving(lib, sim, per_cycle=per_cycle)
    b = S.run_cycles_arriving_rebuilt(lib, sim, per_cycle=per_cycle)
    o = S.run_cycles_arriving_rebuilt(oracle_lib, sim, per_cycle=per_cycle)
    m = sim.workload.num_jobs
    assert a[0]["rows"] == per_cycle and a[-1]["rows"] == m and sum(len(c["scheduled"]) for c in a) == m        # until the workload drains
    assert _records(a) == _records(b) == _records(o)
