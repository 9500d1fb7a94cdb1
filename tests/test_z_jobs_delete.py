"""asched_jobs_delete: rows leave the resident job table between two scheduling cycles, on the device (armada_amd/csrc/kernels_jobs_delete.h) — the library's
counterpart of syncState's delete of the jobs in a terminal state from the jobDb (scheduler.go:539-549; Txn.BatchDelete / delete, jobdb/jobdb.go:941-990).  The contract:
after a delete the handle is what jobs_set of the table without the named rows would have left, the remaining rows renumbered densely and in their old order.

a. the per-queue order and the id map, pinned against a numpy.lexsort restatement of SchedulingOrderCompare (jobdb/comparison.go:49-107) on the reduced table and against
a fresh handle, at the counts and row choices where the compaction takes another turn; b. the request table, gangs and scheduling-key shapes; c. cycles against a fresh
handle and the oracle; d. interplay with jobs_append, jobs_patch, nodes_patch, nodes_upsert, jobs_set and the NodeDb-level calls; e. resets; f. refusals; g. the simulator
fixture with its finished rows deleted.  Every case runs on the CPU build of the device code and, marked gpu, on the HIP library."""
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
CMP_CHUNK = 4096   # armada_amd/csrc/kernels_split.h: elements per workgroup of the grid-wide compaction


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


# ---------------------------------------------------------------- a. the order and the id map, pinned directly
PCS = ((0, True), (1, True), (3, False))
PCP = np.array([p for p, _ in PCS], dtype=np.int64)
NQ, NN, M = 5, 40, 3011          # queue 3 is empty
MBIG = 2 * CMP_CHUNK + 517       # three workgroups of the compaction, the last one partly filled
REQ = np.array([W.Gi, 1000, 0, 0], dtype=np.int64)          # one request shape


class Table:
    """a job table with deliberate ties: few distinct submit times, a few queue priorities, few distinct run timestamps; half of the rows run"""
    FIELDS = ("queue", "pc", "qprio", "submit", "req", "node", "prio", "ts")

    def __init__(self, seed=1, m=M, two_requests=False):
        rng = np.random.default_rng(seed)
        self.cfg = W._config(list(PCS))
        self.node_total = np.tile(np.array([1 << 46, 64_000_000, 1 << 46, 0], dtype=np.int64), (NN, 1))
        self.queue = rng.choice([0, 1, 2, 4], size=m, p=[0.4, 0.3, 0.2, 0.1]).astype(np.int32)
        self.pc = rng.integers(0, 3, size=m).astype(np.int32)
        self.qprio = rng.integers(0, 3, size=m).astype(np.uint32)
        self.submit = rng.integers(0, 40, size=m).astype(np.int64)
        self.req = np.tile(REQ, (m, 1))
        if two_requests:                 # R = 4, every column of a row differs from its neighbours': a wrong stride or a wrong row shows in what a bind takes off a node
            big = rng.random(m) < 0.5
            self.req[big] = np.array([3 * W.Gi, 7000, 5, 0], dtype=np.int64)
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

    def reduced(self, rows):
        """the table jobs_set would be given: without `rows`, the others in their old order -> (table, old -> new id map)"""
        keep = np.ones(self.m, bool)
        keep[np.asarray(rows, dtype=np.int64)] = False
        t = copy.copy(self)
        for f in self.FIELDS:
            setattr(t, f, getattr(self, f)[keep].copy())
        return t, _id_map(keep)


def _id_map(keep):
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


@pytest.fixture(scope="module")
def table():
    return Table()


@pytest.fixture(scope="module")
def big_table():
    return Table(seed=3, m=MBIG)


def _orders(s, nq=NQ):
    return [s.scheduling_order(q) for q in range(nq)]


def _check_order(lib, s, t, what="", nq=NQ):
    got = _orders(s, nq)
    assert got == [t.restated_order(q) for q in range(nq)], ("restatement", what)
    f = t.handle(lib)
    assert got == _orders(f, nq), ("fresh handle", what)
    f.close()


def _delete_and_check(lib, t, rows, what):
    rows = np.asarray(rows, dtype=np.int32)
    s = t.handle(lib)
    got = s.jobs_delete(rows, want_map=True)
    t1, want = t.reduced(rows)
    assert got.dtype == np.int32 and got.tolist() == want.tolist(), ("new_id", what)
    assert s.num_jobs == t.m - len(rows) == t1.m
    st = s.jobs_delete_stats()
    assert (st["rows"], st["in_order"], st["num_jobs"]) == (len(rows), int((t.queue[rows] >= 0).sum()), t1.m) and st["capacity"] >= t.m, st
    _check_order(lib, s, t1, what)
    return s, t1


def test_restatement_is_the_order_of_jobs_set(lib, table, big_table):
    """a pin of this file's own reference, not of the feature: the lexsort restatement, which every case below compares a handle after a delete with, is the order
    asched_jobs_set builds — of the tables and of a reduced one.  It calls no jobs_delete, so it also passes without the feature."""
    for t in (table, big_table, table.reduced(np.arange(0, M, 3))[0]):
        s = t.handle(lib)
        assert _orders(s) == [t.restated_order(q) for q in range(NQ)] and _orders(s)[3] == [] and all(len(o) > 64 for q, o in enumerate(_orders(s)) if q != 3)
        s.close()
    assert table.reduced(np.arange(0, M, 3))[0].m == M - (M + 2) // 3


COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, M - 1]


@pytest.mark.parametrize("d", COUNTS)
def test_order_after_a_delete_of_d_random_rows(lib, table, d):
    rows = np.random.default_rng(100 + d).permutation(M)[:d]          # (in no particular order: the entries need not be sorted)
    s, _ = _delete_and_check(lib, table, rows, f"d={d}")
    s.close()


@pytest.mark.parametrize("d", [CMP_CHUNK - 1, CMP_CHUNK, CMP_CHUNK + 1, MBIG - 1])
def test_order_after_a_delete_of_a_chunk_of_random_rows(lib, big_table, d):
    rows = np.random.default_rng(200 + d).permutation(MBIG)[:d]
    s, _ = _delete_and_check(lib, big_table, rows, f"d={d}")
    s.close()


def _chosen(t, name):
    if name == "row 0":
        return [0]
    if name == "row M - 1":
        return [t.m - 1]
    if name == "rows 0 and M - 1":
        return [t.m - 1, 0]
    if name == "every row of one queue":
        return np.nonzero(t.queue == 1)[0]
    if name == "every running row":
        return np.nonzero(t.node >= 0)[0]
    if name == "every queued row":
        return np.nonzero(t.node < 0)[0]
    if name == "every second row":
        return np.arange(0, t.m, 2)
    raise KeyError(name)


CHOICES = ["row 0", "row M - 1", "rows 0 and M - 1", "every row of one queue", "every running row", "every queued row", "every second row"]


@pytest.mark.parametrize("name", CHOICES)
def test_order_after_a_delete_of_chosen_rows(lib, table, name):
    rows = _chosen(table, name)
    s, t1 = _delete_and_check(lib, table, rows, name)
    if name == "every row of one queue":
        assert _orders(s)[1] == [] and s.jobs_delete_stats()["in_order"] == len(rows)
    if name == "every running row":
        assert (t1.node < 0).all()
    if name == "every queued row":
        assert (t1.node >= 0).all()
    s.close()


BIG_RUNS = {"a run across the first chunk boundary": (CMP_CHUNK - 100, CMP_CHUNK + 100), "exactly the second chunk": (CMP_CHUNK, 2 * CMP_CHUNK),
            "the last chunk's rows": (2 * CMP_CHUNK, MBIG), "everything but one row of each chunk": None}


@pytest.mark.parametrize("name", list(BIG_RUNS))
def test_order_after_a_delete_of_a_contiguous_run(lib, big_table, name):
    if BIG_RUNS[name] is None:
        rows = np.setdiff1d(np.arange(MBIG), [CMP_CHUNK - 1, CMP_CHUNK, MBIG - 1])
    else:
        rows = np.arange(*BIG_RUNS[name])
    s, _ = _delete_and_check(lib, big_table, rows, name)
    s.close()


def test_three_deletes_in_a_row(lib, table):
    """the second and third call find the keep flags, the spare order buffer and the order-key inputs the one before left"""
    rng = np.random.default_rng(5)
    s = table.handle(lib)
    t = table
    for k, d in enumerate((300, 1, 900)):
        rows = rng.permutation(t.m)[:d].astype(np.int32)
        got = s.jobs_delete(rows, want_map=True)
        t, want = t.reduced(rows)
        assert got.tolist() == want.tolist() and s.num_jobs == t.m
        _check_order(lib, s, t, f"delete {k}")
    s.close()


# ---------------------------------------------------------------- b. the request table, gangs, shapes
def _bind_view(s, jobs):
    """what the handle holds of each job's request vector and static matching: a first fit, and a selection with the allocatable it leaves on the picked node"""
    out = [s.fit_select_batch(np.asarray(jobs, dtype=np.int32)).tolist()]
    for j in jobs:
        picked = s.select_node(int(j))
        out.append((repr(picked), s.get_alloc(picked[0].node).tolist() if picked[0].node >= 0 else None))
    return out


def test_request_table_with_two_distinct_rows(lib):
    """R = 4 and two request vectors: a gather with a wrong stride, or one that reads the row of the OLD id, binds another vector than the fresh handle's"""
    t = Table(seed=9, m=1200, two_requests=True)
    rows = np.random.default_rng(1).permutation(t.m)[:417]
    s, t1 = _delete_and_check(lib, t, rows, "two requests")
    f = t1.handle(lib)
    jobs = np.concatenate([np.arange(0, 40), np.arange(t1.m - 40, t1.m)])
    assert len(set(tuple(r) for r in t1.req[jobs])) == 2
    assert _bind_view(s, jobs) == _bind_view(f, jobs)
    s.close(); f.close()


F_JOB = ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class", "job_away")


def _reduced_wl(wl, rows):
    """the workload without `rows`: every per-job array, the queued lists renumbered (relative ids are preserved, so their order stays) -> (workload, old -> new map)"""
    keep = np.ones(wl.num_jobs, bool)
    keep[np.asarray(rows, dtype=np.int64)] = False
    new_id = _id_map(keep)
    w = copy.copy(wl)
    for f in F_JOB:
        v = getattr(wl, f)
        if v is not None:
            setattr(w, f, np.asarray(v)[keep].copy())
    w.queued = [new_id[np.asarray(q, dtype=np.int64)][keep[np.asarray(q, dtype=np.int64)]].astype(np.int32) for q in wl.queued]
    return w, new_id


def _tail_wl(wl, b):
    """the workload with the rows of batch b (a dict of per-job arrays, queued rows) behind it, queued in their queues behind the resident rows (later submit times)"""
    w = copy.copy(wl)
    m0, m = wl.num_jobs, len(b["job_queue"])
    for f in F_JOB:
        v = getattr(wl, f)
        if v is None:
            continue
        d = {"job_node": -1, "job_gang": -1, "job_gang_card": 1}.get(f, 0)
        setattr(w, f, np.concatenate([np.asarray(v), np.asarray(b.get(f, np.full((m,) + np.asarray(v).shape[1:], d)), dtype=np.asarray(v).dtype)]))
    pcp = np.asarray(wl.config.pc_priority)
    w.queued = []
    for q in range(wl.num_queues):
        ids = np.concatenate([np.asarray(wl.queued[q], dtype=np.int64), m0 + np.nonzero(np.asarray(b["job_queue"]) == q)[0]])
        w.queued.append(ids[np.lexsort((ids, w.job_submit[ids], -pcp[w.job_pc[ids]]))].astype(np.int32))
    return w


def _append_rows(s, w, rows):
    s.jobs_append(w.job_req[rows], queue=w.job_queue[rows], pc=w.job_pc[rows], submit_time=w.job_submit[rows], gang_id=w.job_gang[rows], gang_cardinality=w.job_gang_card[rows],
                  req_class=None if w.job_req_class is None else np.asarray(w.job_req_class)[rows])
    return s.jobs_append_stats()


def _round(s, wl):
    W.prepare(s, wl)
    r = s.schedule_round()
    return r, s.round_stats()


def _same_as_fresh(lib, a, w, oracle_lib=None):
    f = W.load(lib, w)
    assert a.num_jobs == w.num_jobs
    assert [a.scheduling_order(q) for q in range(w.num_queues)] == [f.scheduling_order(q) for q in range(w.num_queues)]
    ra, sta = _round(a, w)
    rf, stf = _round(f, w)
    scenario.assert_same_round(rf, ra)
    assert sta["fast_iterations"] == stf["fast_iterations"], "the handle after the delete did not run the fresh handle's fast iterations"
    f.close()
    if oracle_lib is not None:
        o = W.load(oracle_lib, w)
        ro, _ = _round(o, w)
        o.close()
        scenario.assert_same_round(ro, ra)
    return ra


def _gang_wl():
    return W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=713, occupied=0.9, gangs=6)


def _gangs_of(wl):
    """(queue, gang id) -> rows"""
    out = {}
    for j in np.nonzero(np.asarray(wl.job_gang) >= 0)[0]:
        out.setdefault((int(wl.job_queue[j]), int(wl.job_gang[j])), []).append(int(j))
    return out


def test_one_member_of_a_running_gang_deleted(lib, oracle_lib):
    wl0 = _gang_wl()
    a = W.load(lib, wl0)
    r1, _ = _round(a, wl0)                                           # the gangs of the workload are queued: the round leases some, the patch makes them run
    wl, rows = _second_cycle(wl0, r1, 2)
    a.jobs_patch(rows, wl.job_node[rows], wl.job_run_prio[rows], wl.job_run_ts[rows])
    running = [[j for j in g if wl.job_node[j] >= 0] for g in _gangs_of(wl).values()]
    running = [g for g in running if len(g) > 1]
    assert running, "the workload has no running gang: the case pins nothing"
    a.jobs_delete([running[0][1]])
    st = a.jobs_delete_stats()
    assert (st["rows"], st["gangs_emptied"]) == (1, 0)
    w1, _ = _reduced_wl(wl, [running[0][1]])
    _same_as_fresh(lib, a, w1, oracle_lib)
    a.close()


def test_one_member_of_every_gang_deleted(lib, oracle_lib):
    """queued gangs too: what is left of a queued gang can no longer reach its cardinality, on this handle as on a fresh one"""
    wl = _gang_wl()
    rows = [g[len(g) // 2] for g in _gangs_of(wl).values()]
    a = W.load(lib, wl)
    _round(a, wl)
    a.jobs_delete(rows)
    _same_as_fresh(lib, a, _reduced_wl(wl, rows)[0], oracle_lib)
    a.close()


def test_a_whole_gang_deleted_and_appended_again(lib, oracle_lib):
    """the gang's (queue, gang_id) leaves the handle with its last member: the same key comes again as a new gang, as jobs_set of the reduced-then-grown table accepts it"""
    wl = _gang_wl()
    queued = {k: rows for k, rows in _gangs_of(wl).items() if all(wl.job_node[j] < 0 for j in rows)}
    assert queued, "the workload has no queued gang: the case pins nothing"
    key, rows = sorted(queued.items())[0]
    a = W.load(lib, wl)
    with pytest.raises(SchedError) as e:                              # while its rows are in the table the key is taken
        a.jobs_append(wl.job_req[rows], queue=wl.job_queue[rows], pc=wl.job_pc[rows], gang_id=wl.job_gang[rows], gang_cardinality=wl.job_gang_card[rows])
    assert e.value.code == ERR_UNSUPPORTED
    a.jobs_delete(rows[:1])                                           # one member gone: still taken
    w1, m1 = _reduced_wl(wl, rows[:1])
    with pytest.raises(SchedError) as e:
        a.jobs_append(wl.job_req[rows], queue=wl.job_queue[rows], pc=wl.job_pc[rows], gang_id=wl.job_gang[rows], gang_cardinality=wl.job_gang_card[rows])
    assert e.value.code == ERR_UNSUPPORTED
    rest = m1[rows[1:]]
    a.jobs_delete(rest)
    assert a.jobs_delete_stats()["gangs_emptied"] == 1
    w2, _ = _reduced_wl(w1, rest)
    b = {f: np.asarray(getattr(wl, f))[rows] for f in ("job_req", "job_queue", "job_pc", "job_gang", "job_gang_card")}
    b["job_submit"] = np.full(len(rows), int(wl.job_submit.max()) + 1)
    w3 = _tail_wl(w2, b)
    st = _append_rows(a, w3, np.arange(w2.num_jobs, w3.num_jobs))
    assert st["new_gangs"] == 1 and st["rows"] == len(rows)
    _same_as_fresh(lib, a, w3, oracle_lib)
    a.close()


def test_gang_lists_through_a_round_of_the_gang_workload(lib, oracle_lib):
    """many gangs, a third of all rows deleted (whole gangs, parts of gangs, single jobs): the compacted and renumbered members' lists against a fresh handle and the oracle"""
    wl = W.config3(2_000, 20_000, gangs=200)
    rng = np.random.default_rng(21)
    rows = np.nonzero(rng.random(wl.num_jobs) < 0.33)[0]
    whole = [g for k, g in sorted(_gangs_of(wl).items())][::7]
    rows = np.unique(np.concatenate([rows] + [np.asarray(g) for g in whole]))
    a = W.load(lib, wl)
    a.jobs_delete(rows)
    assert a.jobs_delete_stats()["gangs_emptied"] >= len(whole)
    w1, _ = _reduced_wl(wl, rows)
    ra = _same_as_fresh(lib, a, w1, oracle_lib)
    assert any(w1.job_gang[j] >= 0 for j in ra.scheduled), "no gang was scheduled: the case pins nothing"
    a.close()


def _shape_rows(wl):
    """scheduling-key shape (requirement class, priority class, requests) -> rows"""
    cls = np.zeros(wl.num_jobs, np.int64) if wl.job_req_class is None else np.asarray(wl.job_req_class, dtype=np.int64)
    out = {}
    for j in range(wl.num_jobs):
        out.setdefault((int(cls[j]), int(wl.job_pc[j])) + tuple(int(x) for x in wl.job_req[j]), []).append(j)
    return out


@pytest.mark.parametrize("which", ["the first row of a shape", "the only row of a shape", "every row of a shape"])
def test_delete_a_shapes_rows_then_append_that_shape(lib, oracle_lib, which):
    """an append copies the JobRec of a resident row of the same shape: after a delete that row has moved (the first row) or is gone (the last row of the shape — the
    append then takes the rebuild path of a new shape)"""
    wl = W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=713, occupied=0.9, gangs=0)
    shapes = _shape_rows(wl)
    single = lambda rows: all(wl.job_gang[j] < 0 for j in rows)
    if which == "the first row of a shape":
        key, members = next((k, r) for k, r in sorted(shapes.items()) if len(r) >= 3 and single(r))
        rows = members[:1]
    elif which == "the only row of a shape":
        key, members = next((k, r) for k, r in sorted(shapes.items()) if len(r) == 1 and single(r))
        rows = members
    else:
        key, members = next((k, r) for k, r in sorted(shapes.items()) if len(r) >= 2 and single(r))
        rows = members
    a = W.load(lib, wl)
    _round(a, wl)
    a.jobs_delete(rows)
    emptied = len(rows) == len(members)
    assert a.jobs_delete_stats()["shapes_emptied"] == int(emptied)
    w1, _ = _reduced_wl(wl, rows)
    k = 3
    b = dict(job_req=np.tile(np.array(key[2:], dtype=np.int64), (k, 1)), job_queue=np.array([0, 1, 0]), job_pc=np.full(k, key[1]), job_submit=np.full(k, int(wl.job_submit.max()) + 1))
    if wl.job_req_class is not None:
        b["job_req_class"] = np.full(k, key[0])
    w2 = _tail_wl(w1, b)
    st = _append_rows(a, w2, np.arange(w1.num_jobs, w2.num_jobs))
    assert (st["rows"], st["new_shapes"], st["rebuilt"]) == (k, 0, int(emptied)), st
    _same_as_fresh(lib, a, w2, oracle_lib)
    st = _append_rows(a, _tail_wl(w2, b), np.arange(w2.num_jobs, w2.num_jobs + k))     # the shape has rows again: on the device
    assert (st["new_shapes"], st["rebuilt"]) == (0, 0), st
    _same_as_fresh(lib, a, _tail_wl(w2, b), oracle_lib)
    a.close()


# ---------------------------------------------------------------- c. cycles against a fresh handle and the oracle
def _second_cycle(wl, r1, seed):
    """the table and queued lists of the cycle after round r1: scheduled rows run, preempted rows have no run, a seeded tenth of the running jobs has finished.
    -> (workload of cycle 2, rows whose run state changed)"""
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


def _cycle_delete_rows(w2, seed):
    """a seeded third of the rows without a run (finished, preempted and queued ones alike), a twentieth of the running ones, and every fifth gang as a whole"""
    rng = np.random.default_rng(1000 + seed)
    idle, run = np.nonzero(w2.job_node < 0)[0], np.nonzero(w2.job_node >= 0)[0]
    whole = [np.asarray(g, dtype=np.int64) for k, g in sorted(_gangs_of(w2).items())][::5]
    return np.unique(np.concatenate([rng.permutation(idle)[:len(idle) // 3], rng.permutation(run)[:len(run) // 20]] + whole)).astype(np.int32)


def _deleting_cycle(lib, oracle_lib, wl, seed=0, fast=False):
    """round, patch the round's result, delete, round_prepare, round — against a fresh handle and the oracle on the reduced table"""
    a = W.load(lib, wl)
    r1, _ = _round(a, wl)
    w2, rows = _second_cycle(wl, r1, seed)
    a.jobs_patch(rows, w2.job_node[rows], w2.job_run_prio[rows], w2.job_run_ts[rows])
    gone = _cycle_delete_rows(w2, seed)
    got = a.jobs_delete(gone, want_map=True)
    w3, new_id = _reduced_wl(w2, gone)
    assert got.tolist() == new_id.tolist()
    st = a.jobs_delete_stats()
    assert st["rows"] == len(gone) and st["num_jobs"] == w3.num_jobs
    assert any(w2.job_node[j] >= 0 for j in gone) and any(w2.job_node[j] < 0 for j in gone)
    f = W.load(lib, w3)
    assert [a.scheduling_order(q) for q in range(w3.num_queues)] == [f.scheduling_order(q) for q in range(w3.num_queues)]
    ra, sta = _round(a, w3)
    rf, stf = _round(f, w3)
    o = W.load(oracle_lib, w3)
    ro, _ = _round(o, w3)
    o.close()
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert ra.fair_share.tobytes() == rf.fair_share.tobytes() == ro.fair_share.tobytes()
    assert ra.demand_capped_adjusted_fair_share.tobytes() == rf.demand_capped_adjusted_fair_share.tobytes() == ro.demand_capped_adjusted_fair_share.tobytes()
    assert sta["fast_iterations"] == stf["fast_iterations"], "the handle after the delete did not run the fresh handle's fast iterations"
    if fast:
        assert sta["fast_iterations"] > 0
    assert len(ra.scheduled) > 0, "nothing was scheduled in round 2: the case pins nothing"
    # the preemption causes and the evictor report of the round after a delete are the fresh handle's
    assert a.preemption_causes() == f.preemption_causes()
    a.close(); f.close()
    return st


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_deleting_cycle_small_random(lib, oracle_lib, seed):
    wl = W.small_random(n_nodes=40 + 7 * seed, n_jobs=500 + 130 * seed, n_queues=3 + seed, seed=700 + seed, occupied=[0.6, 0.9, 1.0, 0.8][seed - 1], gangs=3 + seed)
    _deleting_cycle(lib, oracle_lib, wl, seed)


@pytest.mark.parametrize("fast_iterations", ["on", "off"])
def test_deleting_cycle_preemption_heavy(lib, oracle_lib, monkeypatch, fast_iterations):
    if fast_iterations == "off":
        monkeypatch.setenv("ASCHED_NO_FAST_ITER", "1")                # every iteration through the generic code, which reads the per-job arrays instead of the JobRec table
    _deleting_cycle(lib, oracle_lib, W.config3(2_000, 20_000, occupied=0.95), 11, fast=fast_iterations == "on")


def test_deleting_cycle_gangs(lib, oracle_lib):
    st = _deleting_cycle(lib, oracle_lib, W.config3(2_000, 20_000, gangs=200), 12, fast=True)
    assert st["gangs_emptied"] > 0


def test_deleting_cycle_130_queues(lib, oracle_lib):
    wl = W.config3(seed=3, n_nodes=300, n_jobs=4_000, n_queues=130, gangs=5, occupied=0.5)
    wl.global_burst, wl.queue_burst = 4_000, 120
    _deleting_cycle(lib, oracle_lib, wl, 13, fast=True)


def test_deleting_cycle_two_word_keys(lib, oracle_lib):
    """W.fine_indexed: the order key needs two words — a handle without a JobRec table and without the fast structure"""
    _deleting_cycle(lib, oracle_lib, W.fine_indexed(n_nodes=500, n_jobs=5_000), 14)


def test_deleting_cycle_with_away_node_types(lib, oracle_lib):
    _deleting_cycle(lib, oracle_lib, W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=711, occupied=0.9, gangs=4, away=True), 7)


# ---------------------------------------------------------------- d. interplay
def _interplay_wl():
    return W.small_random(n_nodes=48, n_jobs=700, n_queues=4, seed=713, occupied=0.9, gangs=4)


def _batch_of(wl, k, seed):
    """k newly submitted single jobs with request vectors the table holds"""
    rng = np.random.default_rng(seed)
    src = rng.permutation(np.nonzero(np.asarray(wl.job_gang) < 0)[0])[:k]
    b = dict(job_req=wl.job_req[src], job_queue=wl.job_queue[src], job_pc=wl.job_pc[src], job_submit=np.full(k, int(wl.job_submit.max()) + 1))
    if wl.job_req_class is not None:
        b["job_req_class"] = np.asarray(wl.job_req_class)[src]
    return b


@pytest.mark.parametrize("order", ["delete, append, patch", "append, delete, patch", "patch, delete, append", "patch, append, delete"])
def test_delete_with_append_and_patch_in_any_order(lib, oracle_lib, order):
    """the three incremental calls of a cycle in the orders a caller may choose; the patch names rows by the ids they have when it is called"""
    wl = _interplay_wl()
    a = W.load(lib, wl)
    r1, _ = _round(a, wl)
    w, rows = _second_cycle(wl, r1, 3)                               # the state the three calls lead to, step by step
    cur = wl                                                         # what the handle holds
    ids = np.arange(wl.num_jobs)                                     # original row -> current id, -1 once deleted (original rows only)
    gone = _cycle_delete_rows(w, 3)
    batch = _batch_of(wl, 40, 8)
    for step in order.split(", "):
        if step == "patch":
            live = rows[ids[rows] >= 0]
            a.jobs_patch(ids[live], w.job_node[live], w.job_run_prio[live], w.job_run_ts[live])
        elif step == "delete":
            a.jobs_delete(ids[gone])
            ids = np.where(np.isin(np.arange(wl.num_jobs), gone), -1, ids)
            ids[ids >= 0] = np.arange((ids >= 0).sum())
        else:
            m0 = a.num_jobs
            s2 = _tail_wl(cur, batch)
            _append_rows(a, s2, np.arange(m0, m0 + 40))
        # the workload the handle must now equal: patched rows (if patched), without the deleted rows (if deleted), with the batch behind (if appended)
        done = order.split(", ")[:order.split(", ").index(step) + 1]
        cur = w if "patch" in done else wl
        if "delete" in done:
            cur = _reduced_wl(cur, gone)[0]
        if "append" in done:
            cur = _tail_wl(cur, batch)
    _same_as_fresh(lib, a, cur, oracle_lib)
    a.close()


def test_delete_then_nodes_patch(lib):
    wl = _interplay_wl()
    a = W.load(lib, wl)
    _round(a, wl)
    gone = _cycle_delete_rows(wl, 5)
    a.jobs_delete(gone)
    w1, _ = _reduced_wl(wl, gone)
    cordoned = np.arange(0, wl.num_nodes, 5, dtype=np.int32)
    a.nodes_patch(cordoned, unschedulable=1)
    f = W.load(lib, w1)
    f.nodes_patch(cordoned, unschedulable=1)
    ra, _ = _round(a, w1)
    rf, _ = _round(f, w1)
    scenario.assert_same_round(rf, ra)
    a.close(); f.close()


def test_delete_then_nodes_upsert_and_jobs_set_of_a_larger_table(lib):
    """the masks and the fast structure are rebuilt from the compacted host mirrors; then the handle takes a larger table and deletes again"""
    wl = _interplay_wl()
    a = W.load(lib, wl)
    gone = _cycle_delete_rows(wl, 6)
    a.jobs_delete(gone)
    w1, _ = _reduced_wl(wl, gone)
    a.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank)
    _same_as_fresh(lib, a, w1)
    larger = _tail_wl(wl, _batch_of(wl, 300, 2))
    W.set_jobs(a, larger)
    st = a.jobs_delete_stats()
    assert (st["rows"], st["num_jobs"]) == (0, 0), "zeros after jobs_set"
    _same_as_fresh(lib, a, larger)
    gone = _cycle_delete_rows(larger, 7)
    a.jobs_delete(gone)
    _same_as_fresh(lib, a, _reduced_wl(larger, gone)[0])
    a.close()


def test_delete_without_a_node_table_then_nodes_upsert(lib):
    wl = _interplay_wl()
    a = Scheduler(lib, wl.config)
    W.set_jobs(a, wl)
    gone = _cycle_delete_rows(wl, 8)
    a.jobs_delete(gone)
    a.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank)
    _same_as_fresh(lib, a, _reduced_wl(wl, gone)[0])
    a.close()


def test_delete_until_an_append_no_longer_reallocates(lib):
    """capacities do not shrink: the rows a delete frees are room for the next append"""
    wl = _interplay_wl()
    a = W.load(lib, wl)
    b = _batch_of(wl, 60, 4)
    w1 = _tail_wl(wl, b)
    st = _append_rows(a, w1, np.arange(wl.num_jobs, w1.num_jobs))
    assert st["reallocated"] == 1, "jobs_set allocates exactly M: the first append cannot fit"
    cap = st["capacity"]
    gone = _cycle_delete_rows(w1, 9)
    a.jobs_delete(gone)
    assert a.jobs_delete_stats()["capacity"] == cap
    w2, _ = _reduced_wl(w1, gone)
    k = cap - w2.num_jobs                                            # exactly the room there is
    assert k > len(gone) // 2
    w3 = _tail_wl(w2, _batch_of(w2, k, 5))                           # (request vectors of surviving rows: no shape comes back from nothing)
    st = _append_rows(a, w3, np.arange(w2.num_jobs, w3.num_jobs))
    assert (st["reallocated"], st["capacity"], st["rebuilt"]) == (0, cap, 0), st
    _same_as_fresh(lib, a, w3)
    a.close()


def test_nodedb_calls_and_submit_check_on_renumbered_ids(lib):
    """between the delete and round_prepare the handle is the empty NodeDb jobs_set leaves: first fits, a selection with its binding, schedule_many of a gang, a submit
    check and the failed-selection records — by the new ids"""
    wl = _interplay_wl()
    a = W.load(lib, wl)
    _round(a, wl)
    gone = _cycle_delete_rows(wl, 10)
    a.jobs_delete(gone)
    w1, _ = _reduced_wl(wl, gone)
    f = W.load(lib, w1)
    jobs = np.arange(0, w1.num_jobs, 3, dtype=np.int32)
    single = [int(j) for j in jobs if w1.job_gang[j] < 0]
    units = [[j] for j in single[:40] + single[-20:]]
    gang = max(_gangs_of(w1).values(), key=len)
    for s in (a, f):
        s.out = [s.fit_select_batch(jobs).tolist(), s.submit_check(units)]
        picked = s.select_node(single[-1])
        assert picked[0].node >= 0
        s.out += [repr(picked), s.get_alloc(picked[0].node).tolist(), s.get_alloc(0).tolist(), repr(s.schedule_many(gang))]
        s.out += [s.excluded_nodes(j) for j in single[:30]]
    assert a.out == f.out
    a.set_evictor_report(True); f.set_evictor_report(True)
    ra, _ = _round(a, w1)
    rf, _ = _round(f, w1)
    scenario.assert_same_round(rf, ra)
    assert repr(a.round_evictor_report()) == repr(f.round_evictor_report()) and a.preemption_causes() == f.preemption_causes()
    a.close(); f.close()


# ---------------------------------------------------------------- e. resets
def test_delete_resets_what_jobs_set_resets(lib):
    """the failed-selection records and the round result of the handle belong to the table as it was: gone after a delete, as after jobs_set"""
    wl = W.config3(n_nodes=150, n_jobs=2500, n_queues=4, seed=9000, gangs=4, occupied=0.95)
    s = W.load(lib, wl)
    r, _ = _round(s, wl)
    on_record = [int(j) for j in np.nonzero(r.job_unschedulable_reason)[0][:200] if s.excluded_nodes(int(j))]
    assert on_record and len(r.preempted) > 0
    s.preemption_causes()
    gone = np.array(on_record[::2], dtype=np.int32)
    w1, new_id = _reduced_wl(wl, gone)
    for rows in (gone[:0], gone):                                   # n == 0: the resets only; then the rows
        s.jobs_delete(rows)
        assert s.jobs_delete_stats()["rows"] == len(rows)
        ids = on_record if len(rows) == 0 else [int(new_id[j]) for j in on_record if new_id[j] >= 0]
        assert all(s.excluded_nodes(j) == [] for j in ids)
        with pytest.raises(SchedError) as e:
            s.preemption_causes()
        assert e.value.code == ERR_INVALID
        with pytest.raises(SchedError):
            s.schedule_round()                                     # round_prepare first, as after jobs_set
        if len(rows) == 0:
            r2, _ = _round(s, wl)
            scenario.assert_same_round(r, r2)
            assert [int(j) for j in on_record if s.excluded_nodes(j)]
    _same_as_fresh(lib, s, w1)
    s.close()


# ---------------------------------------------------------------- f. refusals
def _refusal_wl():
    return W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=0.9, gangs=3)


def test_refusals_leave_the_handle_as_it_was(lib):
    import ctypes as C
    wl = _refusal_wl()
    m = wl.num_jobs
    clean = W.load(lib, wl)
    want_order = [clean.scheduling_order(q) for q in range(wl.num_queues)]
    want, _ = _round(clean, wl)
    clean.close()
    bad = [(ERR_INVALID, [3, m]), (ERR_INVALID, [-1]), (ERR_INVALID, [5, 9, 5]), (ERR_INVALID, list(range(m)) + [0]),   # outside [0, M); named twice
           (ERR_UNSUPPORTED, list(range(m)))]                                                                           # every row
    for code, rows in bad:
        s = W.load(lib, wl)
        with pytest.raises(SchedError) as e:
            s.jobs_delete(rows)
        assert e.value.code == code and str(e.value), (rows[:4], e.value.code, str(e.value))
        assert s.num_jobs == m and s.jobs_delete_stats()["rows"] == 0
        assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
        got, _ = _round(s, wl)
        scenario.assert_same_round(want, got)
        s.jobs_delete(rows[:1] if 0 <= rows[0] < m else [0])         # and the handle still deletes
        assert s.num_jobs == m - 1
        s.close()
    # through the C entry point: the binding cannot express them
    s = W.load(lib, wl)
    one = np.array([1], dtype=np.int32)
    p = one.ctypes.data_as(C.POINTER(C.c_int32))
    null = C.cast(None, C.POINTER(C.c_int32))
    assert s.lib.jobs_delete(s.h, -1, p, null) == ERR_INVALID
    assert s.lib.jobs_delete(s.h, 1, null, null) == ERR_INVALID
    assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order
    got, _ = _round(s, wl)
    scenario.assert_same_round(want, got)
    s.close()


def test_a_refused_delete_after_a_successful_one_keeps_its_stats(lib):
    wl = _refusal_wl()
    s = W.load(lib, wl)
    s.jobs_delete([7, 9])
    st = s.jobs_delete_stats()
    order = [s.scheduling_order(q) for q in range(wl.num_queues)]
    with pytest.raises(SchedError):
        s.jobs_delete([wl.num_jobs - 2])                              # the table has two rows fewer now
    assert s.jobs_delete_stats() == st and [s.scheduling_order(q) for q in range(wl.num_queues)] == order and s.num_jobs == wl.num_jobs - 2
    s.close()


def test_no_job_table_is_refused(lib):
    wl = _refusal_wl()
    s = Scheduler(lib, wl.config)
    for rows in ([0], []):
        with pytest.raises(SchedError) as e:
            s.jobs_delete(rows)
        assert e.value.code == ERR_INVALID
    s.nodes_upsert(wl.node_total)
    with pytest.raises(SchedError) as e:
        s.jobs_delete([0])
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
    for rows in ([1, 2, 3], []):
        with pytest.raises(SchedError) as e:
            s.jobs_delete(rows)
        assert e.value.code == ERR_UNSUPPORTED
    assert [s.scheduling_order(q) for q in range(wl.num_queues)] == want_order and s.num_jobs == wl.num_jobs
    s.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = _refusal_wl()
    s = W.load(oracle_lib, wl)
    for call in (lambda: s.jobs_delete([1]), s.jobs_delete_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    assert s.num_jobs == wl.num_jobs
    s.close()


# ---------------------------------------------------------------- g. the simulator fixture, its finished rows deleted
def _records(cyc):
    return [(c["scheduled"], c["preempted"], c["termination_reason"], c["rows"]) for c in cyc]


@pytest.mark.parametrize("runtime_s", [None, 30.0])
@pytest.mark.parametrize("every", [1, 3])
def test_simulator_cycles_compacting_equal_rebuilt(lib, oracle_lib, every, runtime_s):
    """runtime_s None: the fixture as it is — its jobs run for thirty cycles, so every job has arrived and been leased before the first one finishes and the deletes
    come after the last lease; 30.0: jobs finish after three cycles, rows leave the table while others arrive and are leased"""
    sim = S.from_fixture(FIXTURE)
    if runtime_s is not None:
        sim.job_runtime_s = np.full_like(sim.job_runtime_s, runtime_s)
    per_cycle = 90                                                 # (the fixture's cluster leases about this many jobs a cycle: arrivals keep up with the rounds)
    a = S.run_cycles_compacting(lib, sim, per_cycle=per_cycle, every=every)
    b = S.run_cycles_compacting_rebuilt(lib, sim, per_cycle=per_cycle, every=every)
    o = S.run_cycles_compacting_rebuilt(oracle_lib, sim, per_cycle=per_cycle, every=every)
    m = sim.workload.num_jobs
    assert sum(len(c["scheduled"]) for c in a) == m                # until the workload drains
    assert a[-1]["rows"] < max(c["rows"] for c in a), "the table never shrank: the case pins nothing"
    if runtime_s is not None:
        assert max(c["rows"] for c in a) < m and any(c["scheduled"] and c["rows"] < p["rows"] + per_cycle for p, c in zip(a, a[1:])), "no lease after a delete"
    assert _records(a) == _records(b) == _records(o)
