"""asched_round_prepare_resident / asched_round_queued: the queued lists of a round derived on the device from the resident job order
(armada_amd/csrc/kernels_queued_lists.h) instead of handed in per cycle — what NewQueuedJobsIterator does when it reads repo.QueuedJobs(queue, pool, sortOrder),
a view of the resident jobDb (scheduling/jobiteration.go:144-160).

The expected lists come from nothing of the code under test: for each queue q < Q the ORACLE's scheduling_order(q) of the same uploaded table, filtered to the
rows with node < 0 that are not held; and, as a second statement, a numpy sort of the uploaded columns (priority-class priority descending, queue_priority
ascending, submit_time ascending, row ascending).  The two must agree before either is used.  Every case asserts: round_queued() after round_prepare_resident
equals the expected lists (offsets and jobs); the round after it equals the oracle's round given the explicit expected lists (scenario.assert_same_round) and the
library's own round after round_prepare with those lists; on the GPU every array equals the CPU build's.

a. mark tail and compaction chunk edges; b. queue extremes; c. Q against the table; d. held rows; e. gangs; f. after jobs_patch / jobs_append / jobs_delete with
no jobs_set in between, and the simulator fixture; g. the host aggregate path; h. PQS goldens; i. refusals; j. the launches of a round prepared the old way.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library."""
import ctypes
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scenario
from armada_amd import simulator_input as S
from armada_amd import workloads as W
from armada_amd.binding import SchedError, Scheduler
from golden_io import load

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "simulator_basic_input.json")
CMP_CHUNK, WG = 4096, 256   # armada_amd/csrc/kernels_split.h: elements per workgroup of the compaction, and its width
PCS = ((0, True), (1, True), (3, False))
PCP = np.array([p for p, _ in PCS], dtype=np.int64)
NODE_CPU = 32_000


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def libs(request):
    """(library under test, CPU build to compare its arrays with or None)"""
    hs = request.getfixturevalue("hostsim_lib")
    return (hs, None) if request.param == "hostsim" else (request.getfixturevalue("hip_lib"), hs)


class Table:
    """nodes that the running rows fill exactly plus a few empty ones, and a job table with deliberate ties in every column of the order"""
    FIELDS = ("queue", "pc", "qprio", "submit", "req", "node", "prio", "ts", "gang", "card")

    def __init__(self, m, nq, seed=0, q0=None, run0=None, empty=(), all_run=(), all_queued=(), protected=0.5):
        rng = np.random.default_rng(seed)
        self.cfg = W._config(list(PCS), protected=protected)
        allowed = [q for q in range(nq) if q not in empty]
        self.queue = rng.choice(allowed, size=m).astype(np.int32)
        if q0 is not None and nq > 1:           # queue 0 holds exactly the first q0 rows: its segment of the resident order ends at position q0
            self.queue[:q0] = 0
            self.queue[q0:] = rng.choice([q for q in allowed if q != 0], size=m - q0)
        self.pc = rng.integers(0, 3, size=m).astype(np.int32)
        self.qprio = rng.integers(0, 3, size=m).astype(np.uint32)
        self.submit = rng.integers(0, 40, size=m).astype(np.int64)
        self.req = np.tile(np.array([W.Gi, 1000, 0, 0], dtype=np.int64), (m, 1))
        self.req[rng.random(m) < 0.3, 1] = 2000
        running = rng.random(m) < 0.4
        for q in all_run:
            running[self.queue == q] = True
        for q in all_queued:
            running[self.queue == q] = False
        if run0 is not None:                    # exactly run0 rows of queue 0 run: the running / queued boundary of its segment is at position run0
            r0 = np.nonzero(self.queue == 0)[0]
            running[r0] = False
            running[r0[:run0]] = True
        cpu = np.cumsum(np.where(running, self.req[:, 1], 0))
        self.node = np.where(running, (cpu - 1) // NODE_CPU, -1).astype(np.int32)
        n = int(self.node.max()) + 1 + max(1, m // 512)
        self.node_total = np.tile(np.array([1 << 46, NODE_CPU, 1 << 46, 0], dtype=np.int64), (n, 1))
        self.prio = np.where(running, PCP[self.pc], 0).astype(np.int32)
        self.ts = np.where(running, rng.integers(1, 6, size=m) * 1_000_000_000, 0).astype(np.int64)
        self.gang = np.full(m, -1, np.int32)
        self.card = np.ones(m, np.int32)

    @property
    def m(self):
        return len(self.queue)

    def make_gang(self, rows, gid):
        """`rows` (of one queue) become one queued gang: one shape, one priority class, adjacent in the order"""
        rows = np.asarray(rows)
        for f in ("queue", "pc", "qprio", "submit", "req"):
            getattr(self, f)[rows] = getattr(self, f)[rows[0]]
        self.node[rows], self.prio[rows], self.ts[rows] = -1, 0, 0
        self.gang[rows], self.card[rows] = gid, len(rows)

    def handle(self, lib):
        s = Scheduler(lib, self.cfg)
        s.nodes_upsert(self.node_total)
        s.jobs_set(self.req, queue=self.queue, pc=self.pc, queue_priority=self.qprio, submit_time=self.submit, node=self.node, scheduled_at_priority=self.prio,
                   run_timestamp=self.ts, gang_id=self.gang, gang_cardinality=self.card)
        return s

    def restated(self, q, held=()):
        """the queued rows of queue q that are not held: priority-class priority descending, queue_priority ascending, submit_time ascending, row ascending"""
        hold = np.zeros(self.m, bool)
        hold[np.asarray(held, dtype=np.int64)] = True
        ids = np.nonzero((self.queue == q) & (self.node < 0) & ~hold)[0]
        return ids[np.lexsort((ids, self.submit[ids], self.qprio[ids].astype(np.int64), -PCP[self.pc[ids]]))].astype(np.int32)

    def expected(self, oracle_lib, Q, held=()):
        """per queue q < Q: the oracle's scheduling_order(q) of this table, filtered to rows without a run that are not held — checked against the restatement"""
        o = self.handle(oracle_lib)
        hold = set(int(j) for j in held)
        nq = int(self.queue.max()) + 1
        want = [np.array([j for j in (o.scheduling_order(q) if q < nq else []) if self.node[j] < 0 and j not in hold], dtype=np.int32) for q in range(Q)]
        o.close()
        for q in range(Q):
            assert want[q].tolist() == self.restated(q, held).tolist(), ("the oracle's order and the numpy restatement disagree", q)
        return want


def _weights(Q):
    return 1.0 / (1.0 + np.arange(Q) % 4)


def _same_lists(got, want, what=""):
    assert len(got) == len(want), what
    assert [len(g) for g in got] == [len(w) for w in want], ("offsets", what)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.tolist() == w.tolist(), ("jobs", q, what)


def _resident_round(s, Q, held, **kw):
    s.round_prepare_resident(_weights(Q), held=held, **kw)
    lists = s.round_queued()
    return lists, s.schedule_round()


def check(libs, oracle_lib, t, Q, held=None, handles=None, what="", **kw):
    """the whole statement of this file for one table: lists, round against the oracle and against explicit lists, HIP against the CPU build.  `handles`: the
    handles to use (after resident-table calls), in the order of `libs`, instead of fresh ones.  -> (expected lists, the round)"""
    want = t.expected(oracle_lib, Q, () if held is None else held)
    o = t.handle(oracle_lib)
    o.round_prepare(_weights(Q), want, **kw)
    ro = o.schedule_round()
    o.close()
    outs = []
    for k, lib in enumerate(l for l in libs if l is not None):
        s = handles[k] if handles else t.handle(lib)
        lists, r = _resident_round(s, Q, held, **kw)
        _same_lists(lists, want, what)
        scenario.assert_same_round(r, ro)
        s.round_prepare(_weights(Q), want, **kw)      # the library's own round given the same lists explicitly, and what that prepare leaves
        _same_lists(s.round_queued(), want, ("explicit", what))
        scenario.assert_same_round(s.schedule_round(), r)
        lists2, r2 = _resident_round(s, Q, held, **kw)   # and once more derived: the handle's scratch is reused
        _same_lists(lists2, want, ("second", what))
        scenario.assert_same_round(r2, r)
        outs.append((lists, r))
        if not handles:
            s.close()
    if len(outs) == 2:                                   # the HIP library's arrays against the CPU build's
        _same_lists(outs[0][0], outs[1][0], "HIP against the CPU build")
        scenario.assert_same_round(outs[0][1], outs[1][1])
    return want, ro


# ---------------------------------------------------------------- a. mark tail and compaction chunk edges
def _edge(m):
    """the largest of a chunk, a workgroup and a flag word that lies inside (0, m)"""
    for e in (CMP_CHUNK, WG, 4, 1):
        if e < m:
            return e
    return 0


@pytest.mark.parametrize("split", ["on", "off"])
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_sizes(libs, oracle_lib, m, Q, split):
    """Q = 1: the running / queued boundary of the one segment on the edge (or one off it); Q = 3: the end of queue 0's segment there"""
    e = _edge(m) - (split == "off" and _edge(m) > 0)
    t = Table(m, Q, seed=m + Q, q0=e, run0=e if Q == 1 else None)
    if Q == 1:
        assert int((t.node >= 0).sum()) == e
    else:
        assert int((t.queue == 0).sum()) == e
    want, _ = check(libs, oracle_lib, t, Q)
    assert sum(len(w) for w in want) == int((t.node < 0).sum())


# ---------------------------------------------------------------- b. queue extremes
@pytest.mark.parametrize("name, kw", [("a queue with no job", dict(empty=(2,))), ("a queue whose jobs all run", dict(all_run=(1,))),
                                      ("a queue whose jobs are all queued", dict(all_queued=(1,))), ("the last queue empty", dict(empty=(4,))),
                                      ("the first queue empty", dict(empty=(0,)))])
def test_queue_extremes(libs, oracle_lib, name, kw):
    t = Table(700, 5, seed=11, **kw)
    want, _ = check(libs, oracle_lib, t, 5)
    for q in kw.get("empty", ()) + kw.get("all_run", ()):
        assert len(want[q]) == 0
    for q in kw.get("all_queued", ()):
        assert len(want[q]) == int((t.queue == q).sum()) > 50


# ---------------------------------------------------------------- c. Q against the table
@pytest.mark.parametrize("Q", [2, 8])
def test_Q_smaller_and_larger_than_the_tables_queue_count(libs, oracle_lib, Q):
    t = Table(900, 5, seed=5)
    want, _ = check(libs, oracle_lib, t, Q)
    if Q == 2:
        assert sum(len(w) for w in want) < int((t.node < 0).sum())      # rows of queues >= Q are in no list
    else:
        assert [len(w) for w in want[5:]] == [0, 0, 0] and all(len(w) > 0 for w in want[:5])


@pytest.mark.parametrize("Q", [65, 300])
def test_more_queues_than_the_fast_iteration_takes(libs, oracle_lib, Q):
    """past the queue cap of the fast iteration: the wide runs read the derived lists"""
    t = Table(3000, Q, seed=Q, protected=1.0)
    want, _ = check(libs, oracle_lib, t, Q)
    assert sum(len(w) > 0 for w in want) > 60


# ---------------------------------------------------------------- d. held rows
@pytest.fixture(scope="module")
def held_table():
    return Table(1200, 4, seed=21)


@pytest.mark.parametrize("name", ["none", "one", "every queued row of a queue", "every queued row of the table", "duplicates", "a held row that has a run", "empty array"])
def test_held_rows(libs, oracle_lib, held_table, name):
    t = held_table
    queued, running = np.nonzero(t.node < 0)[0], np.nonzero(t.node >= 0)[0]
    held = {"none": None, "one": queued[7:8], "every queued row of a queue": queued[t.queue[queued] == 2], "every queued row of the table": queued,
            "duplicates": np.concatenate([queued[::5], queued[::10], queued[:3], queued[:3]]), "a held row that has a run": running[::3],
            "empty array": np.zeros(0, np.int32)}[name]      # ("empty array": held non-NULL with n_held == 0)
    want, ro = check(libs, oracle_lib, t, 4, held=held, what=name)
    if name == "every queued row of the table":
        assert all(len(w) == 0 for w in want) and not ro.scheduled
    if name in ("none", "a held row that has a run", "empty array"):
        assert sum(len(w) for w in want) == len(queued)
    if name == "every queued row of a queue":
        assert len(want[2]) == 0 and len(want[1]) > 0


# ---------------------------------------------------------------- e. gangs
def _gang_table():
    t = Table(600, 3, seed=31)
    rows = np.nonzero(t.queue == 1)[0][40:46]
    t.make_gang(rows, 0)
    t.make_gang(np.nonzero((t.queue == 2) & (t.gang < 0))[0][10:13], 1)
    return t, rows


def test_a_queued_gang_stays_adjacent(libs, oracle_lib):
    t, rows = _gang_table()
    want, _ = check(libs, oracle_lib, t, 3)
    pos = [want[1].tolist().index(int(j)) for j in rows]
    assert pos == list(range(pos[0], pos[0] + len(rows)))


def test_a_gang_with_one_member_held(libs, oracle_lib):
    t, rows = _gang_table()
    want, _ = check(libs, oracle_lib, t, 3, held=rows[2:3])
    assert int(rows[2]) not in want[1].tolist() and int(rows[1]) in want[1].tolist()


# ---------------------------------------------------------------- f. after each resident-table call, with no jobs_set in between
def _under_test(libs):
    return [l for l in libs if l is not None]


def _patch(t, hs, rows, node):
    """rows get a run on `node` (or lose theirs, node -1) in the table and, by jobs_patch, on every handle"""
    rows, node = np.asarray(rows, dtype=np.int32), np.asarray(node, dtype=np.int32)
    run = node >= 0
    t.node[rows], t.prio[rows], t.ts[rows] = node, np.where(run, PCP[t.pc[rows]], 0), np.where(run, 7_000_000_000, 0)
    for s in hs:
        s.jobs_patch(rows, t.node[rows], t.prio[rows], t.ts[rows])


def _append(t, hs, k, queue, seed):
    rng = np.random.default_rng(seed)
    new = dict(queue=np.asarray(queue, dtype=np.int32), pc=rng.integers(0, 3, size=k).astype(np.int32), qprio=rng.integers(0, 3, size=k).astype(np.uint32),
               submit=rng.integers(0, 40, size=k).astype(np.int64), req=np.tile(np.array([W.Gi, 1000, 0, 0], dtype=np.int64), (k, 1)), node=np.full(k, -1, np.int32),
               prio=np.zeros(k, np.int32), ts=np.zeros(k, np.int64), gang=np.full(k, -1, np.int32), card=np.ones(k, np.int32))
    for s in hs:
        s.jobs_append(new["req"], queue=new["queue"], pc=new["pc"], queue_priority=new["qprio"], submit_time=new["submit"])
    for f in Table.FIELDS:
        setattr(t, f, np.concatenate([getattr(t, f), new[f]]))


def _delete(t, hs, rows):
    keep = np.ones(t.m, bool)
    keep[np.asarray(rows)] = False
    for s in hs:
        s.jobs_delete(np.asarray(rows, dtype=np.int32))
    for f in Table.FIELDS:
        setattr(t, f, getattr(t, f)[keep].copy())
    return np.where(keep, np.cumsum(keep) - 1, -1)


@pytest.mark.parametrize("call", ["patch leases queued rows", "patch returns running rows", "append", "delete", "all three"])
def test_after_resident_table_calls(libs, oracle_lib, call):
    t = Table(1500, 4, seed=41)
    hs = [t.handle(l) for l in _under_test(libs)]
    check(libs, oracle_lib, t, 4, handles=hs, what="before")
    Q, held = 4, None
    free = int(t.node.max()) + 1                                     # an empty node
    if call in ("patch leases queued rows", "all three"):
        rows = np.nonzero(t.node < 0)[0][3:23]
        _patch(t, hs, rows, np.full(len(rows), free))
        want, _ = check(libs, oracle_lib, t, Q, handles=hs, what="leased")
        assert not set(rows.tolist()) & set(np.concatenate(want).tolist())
    if call in ("patch returns running rows", "all three"):
        rows = np.nonzero(t.node >= 0)[0][5:40:2]
        _patch(t, hs, rows, np.full(len(rows), -1))
        want, _ = check(libs, oracle_lib, t, Q, handles=hs, what="returned")
        assert set(rows.tolist()) <= set(np.concatenate(want).tolist())
    if call in ("append", "all three"):
        _append(t, hs, 37, [0] * 10 + [3] * 10 + [4] * 17, seed=43)   # queue 4: an index the table had not seen
        Q = 5
        want, _ = check(libs, oracle_lib, t, Q, handles=hs, what="appended")
        assert len(want[4]) == 17
    if call in ("delete", "all three"):
        m0 = t.m
        new_id = _delete(t, hs, np.arange(2, m0, 7))
        held = new_id[[1, 4, 5]]                                      # held ids in the new numbering
        assert (held >= 0).all()
        want, _ = check(libs, oracle_lib, t, Q, held=held, handles=hs, what="deleted")
    for s in hs:
        s.close()


@pytest.mark.parametrize("runtime", ["the fixture's", "two cycles"])
@pytest.mark.parametrize("hold_finished", [False, True])
def test_simulator_cycles(libs, oracle_lib, hold_finished, runtime):
    """six cycles of the simulator fixture without any per-cycle list against run_cycles: identical records.  The fixture's jobs run for thirty cycles; with run
    times of two cycles rows finish inside the six, so the delete mode deletes and the held mode holds"""
    sim = S.from_fixture(FIXTURE)
    if runtime == "two cycles":
        sim = dataclasses.replace(sim, job_runtime_s=np.full(sim.workload.num_jobs, 2 * sim.cycle_period_s))
    keys = ("time_s", "scheduled", "preempted", "termination_reason")
    ref = S.run_cycles(oracle_lib, sim, max_cycles=6)
    assert len(ref) == 6 and sum(len(r["scheduled"]) for r in ref) > 0
    arriving = S.run_cycles_compacting_rebuilt(oracle_lib, sim, max_cycles=6)          # the rows arrive by their submit time: jobs_append between the cycles
    assert len(arriving) == 6 and max(r["rows"] for r in arriving) > arriving[0]["rows"]
    for lib in _under_test(libs):
        got = S.run_cycles_resident(lib, sim, per_cycle=sim.workload.num_jobs, max_cycles=6, hold_finished=hold_finished)   # (every row arrives in cycle 0, as in run_cycles)
        assert [{k: r[k] for k in keys} for r in got] == ref
        got = S.run_cycles_resident(lib, sim, max_cycles=6, hold_finished=hold_finished)
        assert [{k: r[k] for k in keys} for r in got] == [{k: r[k] for k in keys} for r in arriving]
        if runtime == "two cycles":
            rows = [r["rows"] for r in got]
            assert (rows[-1] == max(rows)) == hold_finished, rows          # the delete mode's table shrinks when rows finish, the held mode's never does


# ---------------------------------------------------------------- g. the host aggregate path
def _agg_case():
    return Table(1300, 4, seed=51), 4, np.array([3, 9, 9, 400], dtype=np.int32)


def _result_json(lists, r):
    return dict(lists=[l.tolist() for l in lists], scheduled=sorted(r.scheduled.items()), preempted=sorted(r.preempted.items()), alloc=r.queue_allocated_by_pc.tolist(),
                fair=r.fair_share.tolist(), dc=r.demand_capped_adjusted_fair_share.tolist(), tokens=r.queue_tokens_after.tolist(), reason=r.job_unschedulable_reason.tolist())


def test_host_aggregates_in_a_child_process(libs, oracle_lib):
    """ASCHED_HOST_AGG=1 is read once: a fresh child runs the derived round with it and prints what it got"""
    t, Q, held = _agg_case()
    check(libs, oracle_lib, t, Q, held=held)
    lib = libs[0]
    s = t.handle(lib)
    here = _result_json(*_resident_round(s, Q, held))
    s.close()
    env = dict(os.environ, ASCHED_HOST_AGG="1", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), lib.path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == json.loads(json.dumps(here))


def test_allocated_by_pc_without_demand(libs, oracle_lib):
    """allocated_by_pc given, demand not: the host sums the queued demand from the derived lists it reads back"""
    t, Q, held = _agg_case()
    run = t.node >= 0
    alloc = np.zeros((Q, len(PCS), 4), dtype=np.int64)
    np.add.at(alloc, (t.queue[run], t.pc[run]), t.req[run])
    _, ro = check(libs, oracle_lib, t, Q, held=held, allocated_by_pc=alloc)
    _, rd = check(libs, oracle_lib, t, Q, held=held)
    scenario.assert_same_round(ro, rd)


# ---------------------------------------------------------------- h. PQS goldens with their queued lists replaced by derivation
PQS = {c["name"]: c for c in load("pqs")}


@pytest.mark.parametrize("name", ["balancing three queues", "gang preemption"])
def test_pqs_golden_with_derived_lists(libs, monkeypatch, name):
    case = PQS[name]
    assert any(r.get("ExpectedPreemptedIndices") for r in case["Rounds"])
    log = {"explicit": [], "derived": []}
    prepare, schedule = Scheduler.round_prepare, Scheduler.schedule_round

    def derived(self, weight, queued, **kw):
        self.round_prepare_resident(weight, **kw)
        _same_lists(self.round_queued(), [np.asarray(q, dtype=np.int32) for q in queued], name)

    for lib in _under_test(libs):
        for mode in ("explicit", "derived"):
            monkeypatch.setattr(Scheduler, "round_prepare", derived if mode == "derived" else prepare)
            monkeypatch.setattr(Scheduler, "schedule_round", lambda self, *a, _m=mode, **kw: log[_m].append(schedule(self, *a, **kw)) or log[_m][-1])
            try:
                assert scenario.run_pqs_case(lib, case) == "ok"
            finally:
                monkeypatch.setattr(Scheduler, "round_prepare", prepare)
                monkeypatch.setattr(Scheduler, "schedule_round", schedule)
    assert len(log["derived"]) == len(log["explicit"]) == len(case["Rounds"]) * len(_under_test(libs))
    for a, b in zip(log["derived"], log["explicit"]):
        scenario.assert_same_round(a, b)
    assert any(r.preempted for r in log["derived"])


# ---------------------------------------------------------------- i. refusals
def _refused(call, code, *words):
    with pytest.raises(SchedError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def test_refusals(libs, oracle_lib):
    t = Table(400, 3, seed=61)
    lib = libs[0]
    s = t.handle(lib)
    with pytest.raises(SchedError) as e:
        s.round_queued()                                             # before any prepare
    assert e.value.code == ERR_INVALID
    hs = [s] + [t.handle(l) for l in _under_test(libs)[1:]]

    def explicit_lists():
        q, keep = s._queues_struct(_weights(3))
        off = np.zeros(4, np.int32)
        q.queued_off = off.ctypes.data_as(type(q.queued_off))
        assert lib.round_prepare_resident(s.h, ctypes.byref(q), 0, None) == ERR_INVALID and b"queued_off" in lib.last_error(s.h)

    explicit_lists()
    with pytest.raises(SchedError):
        s.round_queued()                                             # the refused call prepared nothing
    for refusal in (explicit_lists,
                    lambda: _refused(lambda: s.round_prepare_resident(_weights(3), held=[-1]), ERR_INVALID, "held[0] = -1"),
                    lambda: _refused(lambda: s.round_prepare_resident(_weights(3), held=[5, t.m]), ERR_INVALID, f"held[1] = {t.m}"),
                    lambda: _refused(lambda: s.round_prepare_resident(np.ones(4097)), ERR_UNSUPPORTED, "4096")):
        refusal()
        check(libs, oracle_lib, t, 3, handles=hs, what="after a refusal")   # a following correct call gives the right round
    _refused(lambda: s.round_prepare_resident(_weights(3), held=[t.m]), ERR_INVALID)
    assert sum(len(l) for l in s.round_queued()) == int((t.node < 0).sum())   # a refusal leaves the last prepare's lists
    for h in hs:
        h.close()
    # a handle uploaded with bid prices carries the market order
    mk = Scheduler(lib, t.cfg)
    mk.nodes_upsert(t.node_total)
    _refused(lambda: mk.round_prepare_resident(_weights(3)), ERR_INVALID, "jobs_set first")      # a call before jobs_set
    mk.jobs_set(t.req, queue=t.queue, pc=t.pc, queue_priority=t.qprio, submit_time=t.submit, node=t.node, scheduled_at_priority=t.prio, run_timestamp=t.ts,
                bid_price=np.ones(t.m))
    _refused(lambda: mk.round_prepare_resident(_weights(3)), ERR_UNSUPPORTED, "market order")
    mk.jobs_set(t.req, queue=t.queue, pc=t.pc, queue_priority=t.qprio, submit_time=t.submit, node=t.node, scheduled_at_priority=t.prio, run_timestamp=t.ts)
    check((lib, None), oracle_lib, t, 3, handles=[mk], what="after the market refusal")
    mk.close()


def test_library_without_the_entry_points_says_so(oracle_lib):
    t = Table(20, 2, seed=1)
    s = t.handle(oracle_lib)
    _refused(lambda: s.round_prepare_resident(_weights(2)), ERR_UNSUPPORTED, "round_prepare_resident")
    _refused(s.round_queued, ERR_UNSUPPORTED, "round_queued")
    s.close()


# ---------------------------------------------------------------- j. launches
def test_launches_of_a_round_prepared_the_old_way(libs, oracle_lib):
    """round_prepare launches nothing new inside the round: a round prepared the old way and one prepared from the resident order count the same launches, and
    the count of the old way is what the parent commit's library counts for the same table (PARENT_LAUNCHES, measured with its CPU build and on the MI355X)"""
    t = Table(900, 4, seed=71)
    want = t.expected(oracle_lib, 4)
    counts = []
    for lib in _under_test(libs):
        s = t.handle(lib)
        s.round_prepare(_weights(4), want)
        s.schedule_round()
        old = s.kernel_times()["round_launches"]
        s.round_prepare_resident(_weights(4))
        s.schedule_round()
        assert s.kernel_times()["round_launches"] == old > 0
        counts.append(old)
        s.close()
    assert counts[0] == PARENT_LAUNCHES[0 if libs[1] is None else 1], counts


PARENT_LAUNCHES = (42, 54)   # (CPU build, HIP library) of the table above on the parent commit


if __name__ == "__main__":   # the child of test_host_aggregates_in_a_child_process: argv[1] = the library file
    sys.path.insert(0, os.path.dirname(HERE))
    from armada_amd.binding import Library
    path = sys.argv[1]
    if not path.endswith("libhostsim.so"):
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
    t_, Q_, held_ = _agg_case()
    s_ = t_.handle(Library(path, "asched_"))
    print(json.dumps(_result_json(*_resident_round(s_, Q_, held_))))
    s_.close()
