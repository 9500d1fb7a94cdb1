"""asched_jobs_reprioritise: the priority of resident jobs within their queue changes between two scheduling cycles, on the device
(armada_amd/csrc/kernels_jobs_reprioritise.h) — the library's counterpart of `armadactl reprioritize` (jobdb/reconciliation.go:198-200, scheduler.go:1198-1199,
job.WithPriority at jobdb/job.go:523) and of the re-seating of those jobs in the per-queue sorted sets (jobdb/jobdb.go:583-587, :695-699).  The contract: after the call
the handle is what jobs_set of the table with the new queue priorities would have left.

a. the per-queue order, pinned against a numpy.lexsort restatement of SchedulingOrderCompare (jobdb/comparison.go:49-107) and against a fresh handle, at the sizes where
the passes take another turn; b. shaped edits; c. composition with jobs_append / jobs_delete / jobs_patch; d. two cycles against a fresh handle and the oracle;
e. the simulator fixture until it drains; f. refusals and resets.  Every case runs on the CPU build of the device code and, marked gpu, on the HIP library.  Every case
but test_restatement_is_the_order_of_jobs_set calls the new entry point."""
import copy
import ctypes as C
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
CYCLE_TS = 7_000_000_000
FIELDS = ("queue", "pc", "qprio", "submit", "req", "node", "prio", "ts", "gang", "card")


class Table:
    """a job table with deliberate ties: three queue priorities, 40 submit times, 5 run timestamps; about half of the rows running; a few rows of no queue; one gang
    of four queued rows in queue 0"""

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
        self.queue[np.nonzero(~running)[0][10:400:30]] = -1                                       # 13 queued rows of no queue
        self.prio = np.where(running, PCP[self.pc], 0).astype(np.int32)
        self.ts = np.where(running, rng.integers(1, 6, size=M) * 1_000_000_000, 0).astype(np.int64)
        self.gang = np.full(M, -1, np.int32)
        self.card = np.ones(M, np.int32)
        members = np.nonzero((self.queue == 0) & ~running & (self.pc == 1))[0][20:24]
        self.gang[members], self.card[members] = 0, 4

    @property
    def m(self):
        return len(self.queue)

    def handle(self, lib):
        s = Scheduler(lib, self.cfg)
        s.nodes_upsert(self.node_total)
        s.jobs_set(self.req, queue=self.queue, pc=self.pc, queue_priority=self.qprio, submit_time=self.submit, node=self.node, scheduled_at_priority=self.prio,
                   run_timestamp=self.ts, gang_id=self.gang, gang_cardinality=self.card)
        return s

    def restated_order(self, q):
        """jobdb/comparison.go:49-107 over the table: active run first (:52-60), priority-class priority descending (:62-68), queue priority ascending (:70-79), both
        active: run timestamp (:83-90), submit time (:92-97), id (:99-105)"""
        ids = np.nonzero(self.queue == q)[0]
        active = self.node[ids] >= 0
        t1 = np.where(active, self.ts[ids], self.submit[ids])
        return ids[np.lexsort((ids, self.submit[ids], t1, self.qprio[ids].astype(np.int64), -PCP[self.pc[ids]], ~active))].tolist()

    def clone(self):
        t = copy.copy(self)
        for f in FIELDS:
            setattr(t, f, getattr(self, f).copy())
        return t

    def reprioritised(self, rows, qprio):
        t = self.clone()
        t.qprio[np.asarray(rows, dtype=np.int64)] = qprio
        return t

    # ---- the other edits of the composition cases, each the table-side twin of one call
    def patch_entries(self, rows, rng, ts=CYCLE_TS):
        """queued -> running; running -> no run, or -> another node with a new timestamp; applied to the table, returned as jobs_patch's arguments"""
        rows = np.asarray(rows, dtype=np.int32)
        stop = (self.node[rows] >= 0) & (rng.random(len(rows)) < 0.5)
        node = np.where(stop, -1, (np.maximum(self.node[rows], 0) + 1 + rng.integers(0, NN - 1, size=len(rows))) % NN).astype(np.int32)
        prio = np.where(stop, 0, PCP[self.pc[rows]]).astype(np.int32)
        ts = np.where(stop, 0, ts).astype(np.int64)
        self.node[rows], self.prio[rows], self.ts[rows] = node, prio, ts
        return rows, node, prio, ts

    def append_rows(self, k, rng, req=(W.Gi, 1000, 0, 0)):
        """k queued rows behind the table; returned as jobs_append's arguments"""
        new = dict(queue=rng.choice([-1, 0, 1, 2, 3, 4], size=k).astype(np.int32), pc=rng.integers(0, 3, size=k).astype(np.int32),
                   queue_priority=rng.integers(0, 3, size=k).astype(np.uint32), submit_time=rng.integers(30, 60, size=k).astype(np.int64))
        r = np.tile(np.array(req, dtype=np.int64), (k, 1))
        for f, v in (("queue", new["queue"]), ("pc", new["pc"]), ("qprio", new["queue_priority"]), ("submit", new["submit_time"]), ("req", r), ("node", np.full(k, -1, np.int32)),
                     ("prio", np.zeros(k, np.int32)), ("ts", np.zeros(k, np.int64)), ("gang", np.full(k, -1, np.int32)), ("card", np.ones(k, np.int32))):
            setattr(self, f, np.concatenate([getattr(self, f), v]))
        return r, new

    def delete_rows(self, rows):
        keep = np.ones(self.m, bool)
        keep[rows] = False
        for f in FIELDS:
            setattr(self, f, getattr(self, f)[keep])


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
    """a pin of this file's own reference, not of the feature: the lexsort restatement, which every case below compares a reprioritised handle with, is the order
    asched_jobs_set builds (and the table has the empty queue, the rows of no queue, the gang and the segment sizes the cases rely on).  It calls no
    jobs_reprioritise, so it also passes without the feature."""
    s = table.handle(lib)
    assert _orders(s) == [table.restated_order(q) for q in range(NQ)] and _orders(s)[3] == [] and all(len(o) > 64 for q, o in enumerate(_orders(s)) if q != 3)
    assert (table.queue == -1).sum() == 13 and (table.gang == 0).sum() == 4 and 0.4 < (table.node >= 0).mean() < 0.6
    s.close()


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, M]


@pytest.mark.parametrize("n", SIZES)
def test_order_after_a_reprioritise_of_n_rows(lib, table, n):
    rng = np.random.default_rng(100 + n)
    rows = rng.permutation(M)[:n].astype(np.int32)
    qprio = rng.integers(0, 4, size=n).astype(np.uint32)
    if n >= 63:
        assert (table.node[rows] >= 0).any() and (table.node[rows] < 0).any() and (qprio != table.qprio[rows]).any() and (qprio == table.qprio[rows]).any()
    s = table.handle(lib)
    s.jobs_reprioritise(rows, qprio)
    st = s.jobs_reprioritise_stats()
    assert (st["entries"], st["in_order"], st["unchanged"]) == (n, int((table.queue[rows] >= 0).sum()), int((qprio == table.qprio[rows]).sum()))
    assert st["made_resident"] == (1 if n > 0 else 0)
    _check_order(lib, s, table.reprioritised(rows, qprio), f"n={n}")
    s.close()


# ---------------------------------------------------------------- b. shaped edits
def _shaped(table, name):
    """-> (rows, queue priorities)"""
    q0 = np.array(table.restated_order(0))
    if name == "every row of one queue to one priority":        # the job-set case: the order falls to the tie-breaks
        return q0, np.full(len(q0), 7, np.uint32)
    if name == "one queue's priorities reversed":
        rows = np.array(table.restated_order(1))
        return rows, (2 - table.qprio[rows]).astype(np.uint32)
    if name == "first and last row of a segment swapped by priority":
        return q0[[0, -1]], np.array([table.qprio[q0[-1]] + 5, 0], np.uint32)
    if name == "only running rows":
        rows = np.nonzero(table.node >= 0)[0][::3]
        return rows, ((table.qprio[rows] + 1 + rows % 2) % 4).astype(np.uint32)
    if name == "only rows of queue -1":
        rows = np.nonzero(table.queue == -1)[0]
        return rows, np.full(len(rows), 9, np.uint32)
    if name == "every entry equal to its current value":
        rows = np.arange(5, M, 7)
        return rows, table.qprio[rows]
    if name == "priorities 0 and 0xFFFFFFFF":
        rows = np.arange(3, M, 5)
        return rows, np.where(rows % 2 == 0, 0, 0xFFFFFFFF).astype(np.uint32)
    if name == "members of one gang moved to both ends of their queue":
        rows = np.nonzero(table.gang == 0)[0]
        return rows, np.array([0xFFFFFFFF, 0, 0xFFFFFFFF, 0], np.uint32)
    raise KeyError(name)


SHAPES = ["every row of one queue to one priority", "one queue's priorities reversed", "first and last row of a segment swapped by priority", "only running rows",
          "only rows of queue -1", "every entry equal to its current value", "priorities 0 and 0xFFFFFFFF", "members of one gang moved to both ends of their queue"]


@pytest.mark.parametrize("name", SHAPES)
def test_order_after_a_shaped_reprioritise(lib, table, name):
    rows, qprio = _shaped(table, name)
    rows = rows.astype(np.int32)
    assert len(rows) > 0
    before = [table.restated_order(q) for q in range(NQ)]
    t = table.reprioritised(rows, qprio)
    after = [t.restated_order(q) for q in range(NQ)]
    s = table.handle(lib)
    s.jobs_reprioritise(rows, qprio)
    st = s.jobs_reprioritise_stats()
    if name in ("only rows of queue -1", "every entry equal to its current value"):
        assert after == before
        assert (st["entries"], st["in_order"], st["unchanged"]) == (len(rows), int((table.queue[rows] >= 0).sum()), 0 if name == "only rows of queue -1" else len(rows))
    else:
        assert after != before, "the edit does not move a row: the case pins nothing"
    if name == "first and last row of a segment swapped by priority":
        assert table.node[rows[0]] >= 0 and table.node[rows[1]] < 0 and after[0][0] != before[0][0] and after[0][-1] != before[0][-1]
    if name == "members of one gang moved to both ends of their queue":
        queued = [j for j in after[0] if t.node[j] < 0 and t.pc[j] == 1]
        head = [j for j in queued if t.qprio[j] == 0]               # (priority 0 is shared with other rows of the class: the front block, not the first places)
        assert set(queued[-2:]) == set(rows[[0, 2]].tolist()) and set(rows[[1, 3]].tolist()) <= set(head) and queued[:len(head)] == head
    _check_order(lib, s, t, name)
    if name == "only rows of queue -1":                            # the stored priority changed although no order did: what a later rebuild of the order reads
        r, new = t.append_rows(50, np.random.default_rng(1), req=(2 * W.Gi, 2000, 0, 0))
        s.jobs_append(r, **new)
        assert s.jobs_append_stats()["rebuilt"] == 1
        s.jobs_reprioritise(rows, t.qprio[rows])
        assert s.jobs_reprioritise_stats()["unchanged"] == len(rows)
        _check_order(lib, s, t, name + ", after an append that rebuilds")
    s.close()


# ---------------------------------------------------------------- c. composition
def _reprioritise(s, t, rows, rng, hi=4):
    rows = np.asarray(rows, dtype=np.int32)
    qprio = rng.integers(0, hi, size=len(rows)).astype(np.uint32)
    s.jobs_reprioritise(rows, qprio)
    t.qprio[rows] = qprio
    return rows


def test_reprioritise_first_then_append_delete_patch_reprioritise(lib, table):
    """the first incremental call on the table is the reprioritise: it makes the order-key inputs resident.  Then an append that re-allocates, a delete, a patch and a
    second reprioritise naming old and new rows: one jobs_set of the final table.  A host mirror of the queue priorities left stale by the first call would come back
    with the delete's squeeze and the later rebuild."""
    rng = np.random.default_rng(31)
    t = table.clone()
    s = t.handle(lib)
    _reprioritise(s, t, rng.permutation(M)[:700], rng)
    assert s.jobs_reprioritise_stats()["made_resident"] == 1
    r, new = t.append_rows(400, rng)
    s.jobs_append(r, **new)
    assert s.jobs_append_stats()["reallocated"] == 1 and s.jobs_append_stats()["rebuilt"] == 0
    _check_order(lib, s, t, "append")
    gone = np.sort(rng.permutation(t.m)[:300]).astype(np.int32)
    s.jobs_delete(gone)
    t.delete_rows(gone)
    s.jobs_patch(*t.patch_entries(rng.permutation(t.m)[:200], rng))
    rows = _reprioritise(s, t, np.concatenate([rng.permutation(M - 300)[:300], np.arange(t.m - 150, t.m)]), rng)
    assert s.jobs_reprioritise_stats()["made_resident"] == 0 and (rows >= M - 300).any() and (rows < M - 300).any()
    _check_order(lib, s, t, "second reprioritise")
    r, new = t.append_rows(60, rng, req=(2 * W.Gi, 2000, 0, 0))     # a new scheduling-key shape: the rebuild of jobs_append reads the host's mirrors
    s.jobs_append(r, **new)
    assert s.jobs_append_stats()["rebuilt"] == 1
    _check_order(lib, s, t, "append that rebuilds")
    s.jobs_reprioritise(rows, t.qprio[rows])
    assert s.jobs_reprioritise_stats()["unchanged"] == len(rows)    # (what the host's mirror says the rows hold)
    _check_order(lib, s, t, "unchanged entries")
    s.close()


def test_patch_first_then_delete_reprioritise_append_reprioritise(lib, table):
    """the same calls in another order: the patch makes the inputs resident, the reprioritise follows a delete and is followed by appends"""
    rng = np.random.default_rng(32)
    t = table.clone()
    s = t.handle(lib)
    s.jobs_patch(*t.patch_entries(rng.permutation(M)[:500], rng))
    gone = np.sort(rng.permutation(t.m)[:257]).astype(np.int32)
    s.jobs_delete(gone)
    t.delete_rows(gone)
    _reprioritise(s, t, rng.permutation(t.m)[:1025], rng)
    assert s.jobs_reprioritise_stats()["made_resident"] == 0
    _check_order(lib, s, t, "reprioritise after a delete")
    r, new = t.append_rows(64, rng, req=(2 * W.Gi, 2000, 0, 0))     # rebuilds
    s.jobs_append(r, **new)
    _check_order(lib, s, t, "append that rebuilds")
    rows = _reprioritise(s, t, np.concatenate([np.arange(0, 900, 3), np.arange(t.m - 64, t.m)]), rng, hi=2)
    r, new = t.append_rows(300, rng)
    s.jobs_append(r, **new)
    s.jobs_patch(*t.patch_entries(rows[::2], rng, ts=CYCLE_TS + 10_000_000_000))
    s.jobs_reprioritise([], [])                                    # n == 0: the resets only
    assert s.jobs_reprioritise_stats()["entries"] == 0
    _check_order(lib, s, t, "end")
    s.close()


def test_delete_first_then_reprioritise(lib, table):
    """the delete is the first incremental call: it uploads the squeezed mirrors; the reprioritise then writes device array and mirror"""
    rng = np.random.default_rng(33)
    t = table.clone()
    s = t.handle(lib)
    gone = np.sort(rng.permutation(M)[:100]).astype(np.int32)
    s.jobs_delete(gone)
    t.delete_rows(gone)
    _reprioritise(s, t, rng.permutation(t.m)[:65], rng)
    gone = np.sort(rng.permutation(t.m)[:100]).astype(np.int32)
    s.jobs_delete(gone)
    t.delete_rows(gone)
    _check_order(lib, s, t)
    s.close()


# ---------------------------------------------------------------- d. rounds: two cycles against a fresh handle and the oracle
def _second_cycle(wl, r1, seed):
    """tests/test_z_jobs_patch.py _second_cycle: the table and queued lists of the cycle after round r1 -> (workload of cycle 2, rows whose run state changed)"""
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


def _limits(wl):
    q = wl.num_queues
    return dict(global_tokens=float(wl.global_burst), global_burst=wl.global_burst, global_rate_inf=wl.rate_inf, queue_tokens=[float(wl.queue_burst)] * q,
                queue_burst=[wl.queue_burst] * q, queue_rate_inf=[wl.rate_inf] * q)


def _load(lib, wl, qprio):
    """W.load with queue priorities"""
    s = Scheduler(lib, wl.config)
    s.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank)
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, queue_priority=qprio, submit_time=wl.job_submit, node=wl.job_node, scheduled_at_priority=wl.job_run_prio,
               run_timestamp=wl.job_run_ts, gang_id=wl.job_gang, gang_cardinality=wl.job_gang_card, req_class=wl.job_req_class, class_tolerations=wl.class_tolerations,
               class_selectors=wl.class_selectors, away=wl.job_away)
    return s


def _restated_queued(wl, qprio):
    """the queued lists of the workload in the restated order: no active run, so priority-class priority descending, queue priority, submit time, id"""
    pcp = np.asarray(wl.config.pc_priority, dtype=np.int64)
    out = []
    for q in wl.queued:
        ids = np.asarray(q, dtype=np.int64)
        out.append(ids[np.lexsort((ids, wl.job_submit[ids], qprio[ids].astype(np.int64), -pcp[wl.job_pc[ids]]))].astype(np.int32))
    return out


def _explicit_round(s, wl, queued):
    s.round_prepare(wl.queue_weight, queued, **_limits(wl))
    return s.schedule_round(), s.round_stats()


def _two_cycles(lib, oracle_lib, wl, seed=0, fast=False, frac=0.3):
    """a round, its result applied with jobs_patch, a reprioritise of queued and running rows, then the round of cycle 2 after round_prepare_resident and after
    explicit lists in the restated order — against a fresh handle and the oracle on the edited workload"""
    rng = np.random.default_rng(1000 + seed)
    a = W.load(lib, wl)
    W.prepare(a, wl)
    r1 = a.schedule_round()
    w2, rows = _second_cycle(wl, r1, seed)
    a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
    m = wl.num_jobs
    named = np.nonzero(rng.random(m) < frac)[0].astype(np.int32)
    gangs = np.nonzero(w2.job_gang >= 0)[0]
    named = np.union1d(named, gangs).astype(np.int32)              # every gang moves as a whole, as `armadactl reprioritize` of a job set would move it
    qprio = np.zeros(m, np.uint32)
    qprio[named] = rng.integers(0, 4, size=len(named))
    for g in np.unique(w2.job_gang[gangs]):                        # (one priority per gang: its members stay adjacent in the queue, as the workloads build them)
        mem = gangs[w2.job_gang[gangs] == g]
        qprio[mem] = qprio[mem[0]]
    assert (w2.job_node[named] >= 0).any() and (w2.job_node[named] < 0).any()
    a.jobs_reprioritise(named, qprio[named])
    queued = _restated_queued(w2, qprio)
    assert any(list(x) != list(y) for x, y in zip(queued, w2.queued)), "the new priorities leave every queued list as it was: the case pins nothing"
    in_list = np.zeros(m, bool)
    for q in queued:
        in_list[q] = True
    held = np.nonzero((w2.job_node < 0) & ~in_list)[0].astype(np.int32)          # finished and preempted rows: no run, in no queued list
    a.round_prepare_resident(w2.queue_weight, held=held, **_limits(w2))
    got = a.round_queued()
    assert [x.tolist() for x in got] == [x.tolist() for x in queued], "round_queued after round_prepare_resident is not the restated queued order"
    ra, sta = a.schedule_round(), a.round_stats()
    rb, stb = _explicit_round(a, w2, queued)
    a.close()
    f = _load(lib, w2, qprio)
    rf, stf = _explicit_round(f, w2, queued)
    f.close()
    o = _load(oracle_lib, w2, qprio)
    ro, _ = _explicit_round(o, w2, queued)
    o.close()
    for r in (ra, rb):
        scenario.assert_same_round(rf, r)
        scenario.assert_same_round(ro, r)
        assert r.fair_share.tobytes() == rf.fair_share.tobytes() == ro.fair_share.tobytes()
        assert r.demand_capped_adjusted_fair_share.tobytes() == rf.demand_capped_adjusted_fair_share.tobytes() == ro.demand_capped_adjusted_fair_share.tobytes()
    assert sta["fast_iterations"] == stb["fast_iterations"] == stf["fast_iterations"], "the reprioritised handle did not run the fresh handle's fast iterations"
    if fast:
        assert sta["fast_iterations"] > 0
    return r1, ra, named


@pytest.mark.parametrize("seed", [1, 2])
def test_two_cycles_small_random(lib, oracle_lib, seed):
    wl = W.small_random(n_nodes=40 + 7 * seed, n_jobs=500 + 130 * seed, n_queues=3 + seed, seed=700 + seed, occupied=[0.6, 0.9][seed - 1], gangs=3 + seed)
    r1, ra, named = _two_cycles(lib, oracle_lib, wl, seed)
    assert len(r1.scheduled) > 0 and len(ra.scheduled) > 0 and len(named) > 0


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


def test_two_cycles_with_cross_pool_away_rows(lib, oracle_lib):
    wl = _with_cross_pool_rows(W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=712, occupied=0.9, gangs=4), 8)
    _, _, named = _two_cycles(lib, oracle_lib, wl, 8)
    assert wl.job_away[named].any()


def test_two_cycles_gangs(lib, oracle_lib):
    wl = W.config3(n_nodes=64, n_jobs=2_000, gangs=40)
    assert (wl.job_gang >= 0).sum() > 40
    _two_cycles(lib, oracle_lib, wl, 12, fast=True)


def test_two_cycles_130_queues(lib, oracle_lib):
    wl = W.config3(seed=3, n_nodes=64, n_jobs=2_000, n_queues=130, gangs=5, occupied=0.5)
    wl.global_burst, wl.queue_burst = 2_000, 60
    _two_cycles(lib, oracle_lib, wl, 13, fast=True)


def test_two_cycles_two_word_keys(lib, oracle_lib):
    """W.fine_indexed: the order key needs two words — a handle without a JobRec table and without the fast structure"""
    wl = W.fine_indexed(n_nodes=64, n_jobs=2_000)
    _two_cycles(lib, oracle_lib, wl, 14)


# ---------------------------------------------------------------- e. the simulator fixture
def _records(cyc):
    return [(c["scheduled"], c["preempted"], c["termination_reason"], c["rows"]) for c in cyc]


def test_simulator_cycles_reprioritising_equal_rebuilt(lib):
    """the fixture until it drains, a few jobs reprioritised every cycle (the first events in cycle 0: the first incremental call on the table), on top of the
    resident cycle: the records of the handle kept by jobs_append / jobs_patch / jobs_reprioritise / jobs_delete are those of jobs_set of the edited table per cycle"""
    sim = S.from_fixture(FIXTURE)
    m = sim.workload.num_jobs
    rng = np.random.default_rng(77)
    events = [(c, rng.permutation(m)[:int(rng.integers(1, 40))], int(rng.integers(0, 4))) for c in range(60)]
    a = S.run_cycles_reprioritising(lib, sim, events)
    b = S.run_cycles_reprioritising_rebuilt(lib, sim, events)
    assert len(a) >= 13 and sum(len(c["scheduled"]) for c in a) == 1000
    assert _records(a) == _records(b)
    plain = S.run_cycles_resident(lib, sim)
    assert [c["scheduled"] for c in a] != [c["scheduled"] for c in plain], "the events change no round: the case pins nothing"


# ---------------------------------------------------------------- f. refusals and resets
def _refused(s, code, rows, qprio):
    with pytest.raises(SchedError) as e:
        s.jobs_reprioritise(rows, qprio)
    assert e.value.code == code and str(e.value), (e.value.code, str(e.value))


def _refusal_wl():
    return _with_cross_pool_rows(W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=0.9, gangs=3), 9)


def _round(s, wl):
    W.prepare(s, wl)
    return s.schedule_round()


def test_refusals_leave_the_handle_as_it_was(lib):
    wl = _refusal_wl()
    clean = W.load(lib, wl)
    want = _round(clean, wl)
    want_order = [clean.scheduling_order(q) for q in range(wl.num_queues)]
    clean.close()
    m = wl.num_jobs
    bad = [([3, m], [1, 1]),                                       # a row outside [0, M)
           ([3, -1], [1, 1]),
           ([3, 5, 3], [1, 2, 3]),                                 # a row named twice
           ([m - 1, 7, 9, 7], [1, 1, 1, 1])]
    for rows, qprio in bad:
        s = W.load(lib, wl)
        _refused(s, ERR_INVALID, rows, qprio)
        i32, u32 = (C.c_int32 * 2)(3, 4), (C.c_uint32 * 2)(1, 1)
        assert s.lib.jobs_reprioritise(s.h, -1, i32, u32) == ERR_INVALID                      # n < 0
        assert s.lib.jobs_reprioritise(s.h, 2, None, u32) == ERR_INVALID                      # null arrays with n > 0
        assert s.lib.jobs_reprioritise(s.h, 2, i32, None) == ERR_INVALID
        assert s.lib.jobs_reprioritise(s.h, (1 << 29) + 1, i32, u32) == ERR_UNSUPPORTED        # more than 2^29 entries (refused before an entry is read)
        assert s.jobs_reprioritise_stats()["entries"] == 0
        assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
        scenario.assert_same_round(want, _round(s, wl))
        s.jobs_reprioritise([3, 5], [1, 2])                        # and the handle still takes the call
        s.close()


def test_no_job_table_is_refused(lib):
    wl = _refusal_wl()
    s = Scheduler(lib, wl.config)
    _refused(s, ERR_INVALID, [0], [1])
    s.nodes_upsert(wl.node_total)
    _refused(s, ERR_INVALID, [], [])
    s.close()
    s = Scheduler(lib, wl.config)                                  # a job table and no node table
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, submit_time=wl.job_submit)
    s.jobs_reprioritise([0, 1], 5)                                 # (a scalar priority is given to every row)
    assert s.jobs_reprioritise_stats()["entries"] == 2
    s.close()


def _market_wl():
    """tests/test_z_jobs_patch.py _market_wl: bid prices uniform inside a gang, the queued lists in price order"""
    wl = W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=1.0, gangs=3)
    bids = np.random.default_rng(11).integers(0, 4, size=wl.num_jobs).astype(np.float64)
    for g in set(int(x) for x in wl.job_gang if x >= 0):
        mem = np.nonzero(wl.job_gang == g)[0]
        bids[mem] = bids[mem[0]]
    bids[(wl.job_node >= 0) & np.array([not wl.config.pc_preemptible[p] for p in wl.job_pc])] = 1_000_000.0
    return wl, bids


def _market_round(s, wl, bids):
    pcp = np.asarray(wl.config.pc_priority)
    queued = [sorted(q, key=lambda j: (-int(pcp[wl.job_pc[j]]), -float(bids[j]), int(wl.job_submit[j]), int(j))) for q in wl.queued]
    s.round_prepare(wl.queue_weight, queued, **_limits(wl))
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
    s = handle()
    _refused(s, ERR_UNSUPPORTED, [3, 4], [1, 2])
    _refused(s, ERR_UNSUPPORTED, [], [])
    assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
    scenario.assert_same_round(want, _market_round(s, wl, bids))
    s.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    s = W.load(oracle_lib, _refusal_wl())
    for call in (lambda: s.jobs_reprioritise([0], [1]), s.jobs_reprioritise_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    s.close()


def test_reprioritise_resets_what_jobs_set_resets(lib):
    """tests/test_z_jobs_patch.py test_patch_resets_what_jobs_set_resets: the failed-selection records and the round result of the handle belong to the table as it
    was — gone after the call, as after jobs_set"""
    wl = W.config3(n_nodes=150, n_jobs=2500, n_queues=4, seed=9000, gangs=4, occupied=0.95)
    s = W.load(lib, wl)
    r = _round(s, wl)
    on_record = [int(j) for j in np.nonzero(r.job_unschedulable_reason)[0][:200] if s.excluded_nodes(int(j))]
    assert on_record and len(r.preempted) > 0
    s.preemption_causes()
    s.jobs_reprioritise([], [])
    assert all(s.excluded_nodes(j) == [] for j in on_record)
    with pytest.raises(SchedError) as e:
        s.preemption_causes()
    assert e.value.code == ERR_INVALID
    with pytest.raises(SchedError):
        s.schedule_round()                                         # round_prepare first, as after jobs_set
    scenario.assert_same_round(r, _round(s, wl))
    s.jobs_reprioritise(np.arange(0, wl.num_jobs, 3), 0)           # every job of the workload has priority 0: nothing moves, and the same holds
    assert s.jobs_reprioritise_stats()["unchanged"] == len(range(0, wl.num_jobs, 3))
    with pytest.raises(SchedError):
        s.schedule_round()
    scenario.assert_same_round(r, _round(s, wl))
    s.close()


def test_a_round_issues_the_launches_it_issued_before(lib):
    """the counter tests/test_z_evictor_report.py test_switch_off_launches reads: a handle that never calls the new entry launches what a fresh handle launches, and so
    does the round of a handle that did"""
    wl = W.config3(n_nodes=150, n_jobs=2500, n_queues=4, seed=9000, gangs=4, occupied=0.95)
    g = W.load(lib, wl)
    _round(g, wl)
    n0 = g.round_timing()["launches"]
    g.close()
    a = W.load(lib, wl)
    a.jobs_reprioritise(np.arange(0, wl.num_jobs, 3), 0)           # (to the values the rows hold: the same table)
    _round(a, wl)
    na = a.round_timing()["launches"]
    a.close()
    assert na == n0 > 10


def test_nodedb_calls_and_submit_check_after_a_reprioritise(lib):
    """between the call and round_prepare the handle is the empty NodeDb jobs_set leaves: first fits, a selection with its binding, a submit check"""
    wl = W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=713, occupied=0.9, gangs=4)
    rng = np.random.default_rng(5)
    qprio = np.zeros(wl.num_jobs, np.uint32)
    named = np.nonzero(wl.job_gang < 0)[0][::2].astype(np.int32)
    qprio[named] = rng.integers(1, 4, size=len(named))
    a = W.load(lib, wl)
    _round(a, wl)
    a.jobs_reprioritise(named, qprio[named])
    f = _load(lib, wl, qprio)
    jobs = np.arange(0, wl.num_jobs, 3, dtype=np.int32)
    single = [int(j) for j in jobs if wl.job_gang[j] < 0]
    units = [[j] for j in single[:60]]
    for s in (a, f):
        s.out = [s.fit_select_batch(jobs).tolist(), s.submit_check(units)]
        picked = s.select_node(single[0])
        assert picked[0].node >= 0
        s.out += [repr(picked), s.get_alloc(picked[0].node).tolist(), s.get_alloc(0).tolist()]
    assert a.out == f.out
    queued = _restated_queued(wl, qprio)
    ra, _ = _explicit_round(a, wl, queued)
    rf, _ = _explicit_round(f, wl, queued)
    scenario.assert_same_round(rf, ra)
    a.close(); f.close()
