"""asched_nodes_delete: rows leave the resident node table between two scheduling cycles, on the device (armada_amd/csrc/kernels_nodes_delete.h) — the library's
counterpart of populateNodeDb leaving an unschedulable node that holds no job out of the NodeDb (scheduling_algo.go:1069-1077) and of the executor filters
(:1100-1169).  The contract: after a delete the handle is what nodes_upsert of the table without the named rows would have left, the remaining rows renumbered densely
and in their old order, with every run of the resident job table sent through that map.  The oracle has no delete: its side is always the reduced table.

a. the map, the NodeDb-level answers and a round against a fresh handle, at the counts and row choices where the compaction and the mask words take another turn;
b. 65 requirement classes; c. a table that iterates literally; d. rounds against a fresh handle and the oracle, and the reference's own rule (a cordoned idle node
dropped is not a cordoned idle node kept); e. interplay with jobs_patch, jobs_append, jobs_delete, nodes_patch, nodes_upsert, jobs_set, the evictor report and the
preemption causes; f. the rebuild path; g. refusals; h. the simulator fixture with nodes drained and dropped; i. a library without the entry point.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library."""
import copy
import os

import numpy as np
import pytest

import scenario
import test_z_jobs_append as JA
import test_z_nodes_patch as NP
from armada_amd import simulator_input as S
from armada_amd import workloads as W
from armada_amd.binding import SchedError, Scheduler

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulator_basic_input.json")
CMP_CHUNK = 4096   # armada_amd/csrc/kernels_split.h: elements per workgroup of the grid-wide compaction
UNSCHED_KEY = NP.UNSCHED_KEY


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


# ---------------------------------------------------------------- the table of a., b., f. and g.
PCS = NP.PCS
PCP = np.array([p for p, _ in PCS], dtype=np.int64)
N, M = 130, 500                           # three mask words, the last one partial
NBIG = 2 * CMP_CHUNK + 517                # three workgroups of the compaction, the last one partly filled
KEPT = (80, 115)                          # with nodes 45 and 10 the only tainted AND unschedulable nodes of their label value


class Table:
    """the table of tests/test_z_nodes_patch.py with half of its jobs running: n nodes of 8 populated node types (every taint is indexed: an indexed label with two
    values x the taint (7, 1, NoSchedule) on every fifth node x unschedulable on every seventh), m jobs of `ncls` requirement classes and three priority classes, two
    of them with away entries (mask rows behind the S shape rows), and two jobs no node can hold.  run_above: running jobs sit on nodes >= run_above only."""

    def __init__(self, n=N, m=M, ncls=4, seed=3, run_above=0):
        rng = np.random.default_rng(seed)
        self.cfg = W._config(list(PCS))
        self.cfg.indexed_taint_keys = None
        self.cfg.indexed_label_keys = [3]
        self.cfg.wkt_taints = [[(7, 1, 1)], [(7, -1, 1)]]
        self.cfg.pc_away = [[], [(0, 0)], [(2, 1), (1, 0)]]
        self.total = np.tile(np.array([64 * W.Gi, 16000, 512 * W.Gi, 0], dtype=np.int64), (n, 1))
        self.total[::9, W.GPU] = 4
        self.allocatable = self.total.copy()
        self.allocatable[::4, W.CPU] -= 1000 * (np.arange(0, n, 4) % 5)   # every node's planes differ from its neighbours': a lane that took another node's column shows
        self.labels = [[(3, (i // 2) % 2)] for i in range(n)]
        self.taints = [[(7, 1, 1)] if i % 5 == 0 else [] for i in range(n)]
        self.unschedulable = (np.arange(n) % 7 == 3).astype(np.uint8)
        self.over_allocated = np.zeros(n, np.uint8)
        self.index = (np.arange(n, dtype=np.uint64) * 7919) % np.uint64(n * 8 + 1) * np.uint64(n) + np.arange(n, dtype=np.uint64) + np.uint64(1)   # distinct, not in row order
        shapes = W._shapes64()[::5]
        self.req = shapes[rng.integers(0, len(shapes), size=m)].copy()
        self.req[rng.random(m) < 0.1, W.GPU] = 1
        self.req[-2:, W.CPU] = 17000                                # more than any node's total
        self.queue = rng.integers(0, 3, size=m).astype(np.int32)
        self.pc = rng.integers(0, 3, size=m).astype(np.int32)
        self.cls = rng.integers(0, ncls, size=m).astype(np.int32)
        self.cls[-2:] = (0, 1)
        self.tolerations = [[], [(7, 1, 0, 0)], [], [(UNSCHED_KEY, 1, 0, 0)]] + [[(7, 0, 1, 1), (100 + c, 1, 0, 0)] for c in range(4, ncls)]
        self.selectors = [[], [], [(3, 1)], []] + [[] for _ in range(4, ncls)]
        self.node = np.full(m, -1, np.int32)
        free = self.allocatable.copy()
        for j in np.nonzero(rng.random(m - 2) < 0.5)[0]:            # half of the jobs run, each on a node that still has room for it
            v = int(rng.integers(run_above, n))
            if (self.req[j] <= free[v]).all():
                free[v] -= self.req[j]
                self.node[j] = v
        self.prio = np.where(self.node >= 0, PCP[self.pc], 0).astype(np.int32)
        self.ts = np.where(self.node >= 0, rng.integers(1, 6, size=m) * 1_000_000_000, 0).astype(np.int64)

    @property
    def n(self):
        return len(self.total)

    @property
    def m(self):
        return len(self.queue)

    def upsert(self, s):
        s.nodes_upsert(self.total, self.allocatable, index=self.index, unschedulable=self.unschedulable, over_allocated=self.over_allocated, taints=self.taints, labels=self.labels)

    def set_jobs(self, s):
        s.jobs_set(self.req, queue=self.queue, pc=self.pc, req_class=self.cls, class_tolerations=self.tolerations, class_selectors=self.selectors,
                   node=self.node, scheduled_at_priority=self.prio, run_timestamp=self.ts)

    def handle(self, lib):
        s = Scheduler(lib, self.cfg)
        self.upsert(s)
        self.set_jobs(s)
        return s

    def unbound(self, rows):
        """the table with the runs on `rows` ended (what the caller says first: jobs_patch with node -1) -> (table, those job rows)"""
        jobs = np.nonzero(np.isin(self.node, np.asarray(rows, dtype=np.int64)))[0].astype(np.int32)
        t = copy.copy(self)
        t.node, t.prio, t.ts = self.node.copy(), self.prio.copy(), self.ts.copy()
        t.node[jobs], t.prio[jobs], t.ts[jobs] = -1, 0, 0
        return t, jobs

    def reduced(self, rows):
        """the tables nodes_upsert and jobs_set would be given: without node rows `rows`, the others in their old order, every run on its node's new position
        -> (table, old -> new map)"""
        keep = np.ones(self.n, bool)
        keep[np.asarray(rows, dtype=np.int64)] = False
        new_id = _id_map(keep)
        assert not np.isin(self.node, np.nonzero(~keep)[0]).any(), "a running job on a deleted row"
        t = copy.copy(self)
        for f in ("total", "allocatable", "unschedulable", "over_allocated", "index"):
            setattr(t, f, getattr(self, f)[keep].copy())
        t.labels = [x for x, k in zip(self.labels, keep) if k]
        t.taints = [x for x, k in zip(self.taints, keep) if k]
        t.node = np.where(self.node >= 0, new_id[np.maximum(self.node, 0)], -1).astype(np.int32)
        return t, new_id

    def types(self, rows=None):
        """the populated node types and label values of the table without `rows`"""
        keep = np.ones(self.n, bool)
        if rows is not None:
            keep[np.asarray(rows, dtype=np.int64)] = False
        ty = {(tuple(self.labels[i]), tuple(self.taints[i]), int(self.unschedulable[i])) for i in np.nonzero(keep)[0]}
        return ty, {v for i in np.nonzero(keep)[0] for _, v in self.labels[i]}

    def round(self, s):
        queued = [np.nonzero((self.queue == q) & (self.node < 0))[0].astype(np.int32) for q in range(3)]
        queued = [q[np.lexsort((q, -PCP[self.pc[q]]))] for q in queued]
        s.round_prepare(np.ones(3), queued, global_tokens=1e18, global_burst=1 << 62, global_rate_inf=True, queue_tokens=[1e18] * 3, queue_burst=[1 << 62] * 3, queue_rate_inf=[True] * 3)
        return s.schedule_round()


def _id_map(keep):
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


def view(s, t, step=1):
    """the NodeDb-level answers of a handle that has nodes and jobs and no round: the node count, the totals, the indexed label's values, every plane of every node, a
    node iteration per priority, every job's first fit at every priority, select_node of every step-th job, the node types that match a job, a submit-check batch and
    the exclusion reasons of the two selections that cannot succeed"""
    jobs = np.arange(t.m, dtype=np.int32)
    out = [s.num_nodes, s.lib.num_nodes(s.h), s.total_resources().tolist(), s.indexed_node_label_values(3), s.get_nodes_alloc().tolist()]
    out += [s.iterate_nodes(p, [4000, 8 * W.Gi, 0]) for p in s.priorities]
    out += [s.fit_select_batch(jobs, p).tolist() for p in s.priorities]
    out.append([(r[0].node, r[0].scheduled_at_priority, r[0].method) for r in (s.select_node(int(j)) for j in jobs[::step])])
    out.append([s.node_types_matching_job(int(j)) for j in jobs[::3]])
    out.append(s.submit_check([[int(j)] for j in jobs[::7]]))
    excl = []
    for j in (t.m - 2, t.m - 1):
        assert s.select_node(int(j))[0].node < 0
        excl.append(s.excluded_nodes(int(j)))
    out.append(excl)
    return out


def _compare(lib, s, t1, what, step=1, round_too=True, oracle=None):
    f = t1.handle(lib)
    got, want = view(s, t1, step), view(f, t1, step)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, "view item", k)
    if round_too:
        rs, rf = t1.round(s), t1.round(f)
        scenario.assert_same_round(rf, rs)
        if oracle is not None:
            o = t1.handle(oracle)
            scenario.assert_same_round(t1.round(o), rs)
            o.close()
    f.close()


def _delete_and_compare(lib, t, rows, what, step=1, oracle=None):
    """the documented sequence: say what became of the runs on the rows (jobs_patch with node -1), then nodes_delete; compared with a fresh handle"""
    rows = np.asarray(rows, dtype=np.int32)
    t2, jobs = t.unbound(rows)
    s = t.handle(lib)
    if len(jobs):
        s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
    got = s.nodes_delete(rows, want_map=True)
    t1, want = t2.reduced(rows)
    keep = np.ones(t.n, bool)
    keep[rows] = False
    assert got.dtype == np.int32 and got.tolist() == want.tolist() == np.where(keep, np.cumsum(keep) - 1, -1).tolist(), ("new_id", what)
    assert s.num_nodes == t.n - len(rows) == t1.n
    st = s.nodes_delete_stats()
    types, values = t.types()
    types1, values1 = t.types(rows)
    why = 4 if values1 != values else 2 if types1 != types else 0
    first = int(rows.min()) if len(rows) else t.n
    assert st == [len(rows), int((t2.node > first).sum()), 1 if why else 0, why, t1.n, 0, 0, 0], (st, what)
    _compare(lib, s, t1, what, step, oracle=oracle)
    return s, t1, st


def test_the_reduced_table_is_what_a_fresh_handle_is_given(lib, oracle_lib):
    """a pin of this file's own reference, not of the feature: Table.unbound and Table.reduced build the tables every case below uploads to its fresh handle — the
    library and the oracle agree on them, the totals are the column sums of what is left and the map is the running count of kept rows.  It calls no nodes_delete, so
    it also passes without the feature."""
    t = Table()
    rows = _rows(65)
    assert len(set(rows.tolist())) == 65 and not set(KEPT) & set(rows.tolist())
    assert (t.node >= 0).sum() > M // 3 and len(t.types()[0]) == 8 and t.types(rows) == t.types()
    t2, jobs = t.unbound(rows)
    assert len(jobs) > 0 and (t2.node[jobs] == -1).all()
    t1, new_id = t2.reduced(rows)
    assert t1.n == N - 65 and (new_id[rows] == -1).all() and sorted(new_id[new_id >= 0].tolist()) == list(range(N - 65))
    assert (t1.total == np.delete(t.total, rows, axis=0)).all() and t1.node.max() < t1.n and ((t1.node >= 0) == (t2.node >= 0)).all()
    s, o = t1.handle(lib), t1.handle(oracle_lib)
    jobs = np.arange(M, dtype=np.int32)
    for prio in s.priorities:
        assert s.fit_select_batch(jobs, prio).tolist() == o.fit_select_batch(jobs, prio).tolist()
    assert s.total_resources().tolist() == t1.allocatable.sum(axis=0).tolist()
    scenario.assert_same_round(t1.round(o), t1.round(s))
    s.close(); o.close()


# ---------------------------------------------------------------- a. geometry
def _rows(d, n=N, seed=42):
    """d random rows; below n - 1 rows never the last node of a node type (a node type that loses its last node is the rebuild path: f.)"""
    t = _TABLES.setdefault(n, Table(n=n, m=4))
    last = {}
    for i in range(n):
        last[(tuple(t.labels[i]), tuple(t.taints[i]), int(t.unschedulable[i]))] = i
    kept = set(last.values()) | set(KEPT)
    perm = [int(k) for k in np.random.default_rng(seed).permutation(n) if d >= n - 1 or int(k) not in kept]
    return np.array(perm[:d], dtype=np.int32)


_TABLES = {}
COUNTS = [0, 1, 2, 63, 64, 65, 66, 129]   # 2 -> 128 nodes: the last word becomes full; 66 -> 64 nodes: exactly one word, Npad 192 -> 64; 129: one node left


@pytest.mark.parametrize("d", COUNTS)
def test_answers_after_a_delete_of_d_random_rows(lib, d):
    t = Table()
    s, t1, st = _delete_and_compare(lib, t, _rows(d), d)
    if d <= 66:
        assert st[2] == 0, ("the device path", st)
    s.close()


CHOSEN = {"row 0": [0], "row 129": [129], "rows 0..63": list(range(64)), "every other row": list(range(0, N, 2)), "rows 60..70": list(range(60, 71))}


@pytest.mark.parametrize("name", list(CHOSEN))
def test_answers_after_a_delete_of_chosen_rows(lib, oracle_lib, name):
    s, t1, st = _delete_and_compare(lib, Table(), CHOSEN[name], name, oracle=oracle_lib)
    assert st[2] == 0, ("the device path", st)
    s.close()


@pytest.fixture(scope="module")
def big_table():
    return Table(n=NBIG, seed=5)


@pytest.mark.parametrize("d", [1, CMP_CHUNK - 1, CMP_CHUNK, CMP_CHUNK + 1])
def test_answers_after_a_delete_across_the_compaction_chunks(lib, big_table, d):
    s, t1, st = _delete_and_compare(lib, big_table, _rows(d, NBIG, seed=d), d, step=25)
    assert st[2] == 0, st
    s.close()


def test_deletes_one_after_the_other_and_nodes_upsert_in_between(lib):
    """every delete finds what the one before it left; n == 0 performs the resets only; nodes_upsert puts the statistics back to zero"""
    t = Table()
    s = t.handle(lib)
    for k, d in enumerate((2, 0, 63, 1)):
        rows = _rows(d, t.n, seed=70 + k) if t.n == N else np.random.default_rng(70 + k).permutation(t.n)[:d].astype(np.int32)
        rows = np.array([r for r in rows if t.types([r]) == t.types()][:d], dtype=np.int32)
        t2, jobs = t.unbound(rows)
        if len(jobs):
            s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
        s.round_prepare(np.ones(3), [[], [], []])
        s.nodes_delete(rows)
        with pytest.raises(SchedError):
            s.schedule_round()                                         # round_prepare first, as after nodes_upsert
        t, _ = t2.reduced(rows)
        assert s.nodes_delete_stats()[0] == len(rows) and s.nodes_delete_stats()[4] == t.n
        _compare(lib, s, t, k, step=5)
    t.upsert(s)
    t.set_jobs(s)
    assert s.nodes_delete_stats() == [0] * 8
    _compare(lib, s, t, "after nodes_upsert", step=5)
    s.close()


# ---------------------------------------------------------------- b. 65 requirement classes
def test_answers_after_a_delete_with_65_requirement_classes(lib):
    """more classes than a node's class word holds: no fast structure, two words of class bits per node; every running job sits above the deleted rows, so every
    one of them is renumbered"""
    t = Table(ncls=65, run_above=70)
    rows = [r for r in range(64) if r not in (10, 45)]
    s, t1, st = _delete_and_compare(lib, t, rows, "65 classes")
    assert st[2] == 0 and st[1] == int((t.node >= 0).sum()) > 100, st
    s.close()


# ---------------------------------------------------------------- c., d. workloads: rounds against a fresh handle and the oracle
def _wl_unbound(wl, rows):
    """the workload with the runs on node rows `rows` ended -> (workload, those job rows)"""
    jobs = np.nonzero(np.isin(wl.job_node, np.asarray(rows, dtype=np.int64)))[0].astype(np.int32)
    w = copy.copy(wl)
    w.job_node, w.job_run_prio, w.job_run_ts = wl.job_node.copy(), wl.job_run_prio.copy(), wl.job_run_ts.copy()
    w.job_node[jobs], w.job_run_prio[jobs], w.job_run_ts[jobs] = -1, 0, 0
    return w, jobs


def _wl_reduced(wl, state, rows):
    """the workload and node state without node rows `rows` -> (workload, state, old -> new map)"""
    keep = np.ones(wl.num_nodes, bool)
    keep[np.asarray(rows, dtype=np.int64)] = False
    new_id = _id_map(keep)
    assert not np.isin(wl.job_node, np.nonzero(~keep)[0]).any()
    w = copy.copy(wl)
    w.node_total = wl.node_total[keep]
    w.node_allocatable = None
    w.node_taints = None if wl.node_taints is None else [x for x, k in zip(wl.node_taints, keep) if k]
    w.node_labels = None if wl.node_labels is None else [x for x, k in zip(wl.node_labels, keep) if k]
    w.node_id_rank = None if wl.node_id_rank is None else np.asarray(wl.node_id_rank)[keep]
    w.job_node = np.where(wl.job_node >= 0, new_id[np.maximum(wl.job_node, 0)], -1).astype(wl.job_node.dtype)
    return w, {k: v[keep].copy() for k, v in state.items()}, new_id


def _state(wl, cordoned=()):
    st = dict(allocatable=wl.node_total.copy() if wl.node_allocatable is None else wl.node_allocatable.copy(),
              unschedulable=np.zeros(wl.num_nodes, np.uint8), over_allocated=np.zeros(wl.num_nodes, np.uint8))
    st["unschedulable"][list(cordoned)] = 1
    return st


def _load(lib, wl, state, uni=False):
    """tests/test_z_nodes_patch.py _load; uni: every gang asks for nodes that agree in the indexed label 3 (a uniformity label: the label masks decide)"""
    if not uni:
        return NP._load(lib, wl, state)
    s = Scheduler(lib, wl.config)
    s.nodes_upsert(wl.node_total, state["allocatable"], unschedulable=state["unschedulable"], over_allocated=state["over_allocated"], taints=wl.node_taints,
                   labels=wl.node_labels, id_rank=wl.node_id_rank)
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, submit_time=wl.job_submit, node=wl.job_node, scheduled_at_priority=wl.job_run_prio, run_timestamp=wl.job_run_ts,
               gang_id=wl.job_gang, gang_cardinality=wl.job_gang_card, gang_uniformity_label=np.where(wl.job_gang >= 0, 3, -1).astype(np.int32), req_class=wl.job_req_class,
               class_tolerations=wl.class_tolerations, class_selectors=wl.class_selectors, away=wl.job_away)
    return s


def _safe_rows(wl, rows):
    """of `rows`, those whose node type and label values other nodes carry as well (the device path)"""
    def ty(i):
        return (tuple(wl.node_labels[i]) if wl.node_labels else (), tuple(wl.node_taints[i]) if wl.node_taints else ())
    rows = [int(r) for r in rows]
    left = {}
    for i in range(wl.num_nodes):
        if i not in rows:
            left[ty(i)] = left.get(ty(i), 0) + 1
    return [r for r in rows if left.get(ty(r), 0) > 0]


def _wl_delete_case(lib, oracle_lib, wl, rows, cordoned=(), device_path=True, uni=False):
    """cycle 1 on the whole table, then the runs on `rows` end, the rows leave, and cycle 2 — against a fresh handle and the oracle given the reduced table"""
    state = _state(wl, cordoned)
    s = _load(lib, wl, state, uni)
    r0, _ = NP._round(s, wl)                                           # (the delete finds a handle that has run a round)
    w2, jobs = _wl_unbound(wl, rows)
    if len(jobs):
        s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
    new_id = s.nodes_delete(rows, want_map=True)
    w1, state1, want = _wl_reduced(w2, state, rows)
    assert new_id.tolist() == want.tolist()
    st = s.nodes_delete_stats()
    assert st[0] == len(rows) and st[4] == w1.num_nodes and (st[2] == 0 or not device_path), st
    with pytest.raises(SchedError):
        s.schedule_round()
    r1, st1 = NP._round(s, w1)
    f, o = _load(lib, w1, state1, uni), _load(oracle_lib, w1, state1, uni)
    rf, stf = NP._round(f, w1)
    ro, _ = NP._round(o, w1)
    scenario.assert_same_round(rf, r1)
    scenario.assert_same_round(ro, r1)
    assert st1["fast_iterations"] == stf["fast_iterations"]
    return s, f, o, w1, state1, r0, r1


def test_literal_iteration_after_a_delete(lib, oracle_lib):
    """W.small_random(ragged=True): a class matching several populated types over unaligned allocatable, id_rank not monotone in index — the rows iterate literally"""
    wl = NP._round_wl("ragged")
    assert wl.node_id_rank is not None and (np.diff(np.asarray(wl.node_id_rank)) < 0).any()
    rows = np.array(_safe_rows(wl, [0, 5, 63, 64, 65, 100, 129]), dtype=np.int32)
    assert len(rows) >= 5
    s, f, o, w1, state1, r0, r1 = _wl_delete_case(lib, oracle_lib, wl, rows)
    for p in s.priorities:
        for req in ([4000, 8 * W.Gi, 0], [1000, W.Gi, 1]):
            assert s.iterate_nodes(p, req) == f.iterate_nodes(p, req) == o.iterate_nodes(p, req), p
    for x in (s, f, o):
        x.close()


def _gang_wl():
    """many queued gangs on a table with an indexed label (W.small_random ragged: label 3 with three values on most nodes); _load(uni=True) makes it every gang's
    uniformity label"""
    return W.small_random(n_nodes=N, n_jobs=1200, n_queues=4, seed=4103, occupied=0.5, gangs=12, ragged=True)


@pytest.mark.parametrize("kind", ["ragged", "offgrid", "gangs with a uniformity label"])
def test_round_after_a_delete(lib, oracle_lib, kind):
    """the round kinds of tests/test_z_nodes_patch.py — "ragged": plain placement by the literal iterators; "offgrid": a preempting round on the fast path — and a gang
    round in which the label masks decide"""
    uni = kind.startswith("gangs")
    wl = _gang_wl() if uni else NP._round_wl(kind)
    rng = np.random.default_rng(11)
    rows = np.array(_safe_rows(wl, rng.permutation(wl.num_nodes)[:17]), dtype=np.int32)
    assert len(rows) >= 10 and rows.min() < 64 <= rows.max()
    s, f, o, w1, state1, r0, r1 = _wl_delete_case(lib, oracle_lib, wl, rows, uni=uni)
    assert NP._different(r0, r1)
    if uni:
        placed = [j for j in r1.scheduled if w1.job_gang[j] >= 0]
        assert placed, "no gang was placed: the uniformity label decided nothing"
        for g in set(int(w1.job_gang[j]) for j in placed):
            vals = {tuple(w1.node_labels[r1.scheduled[j]]) for j in placed if w1.job_gang[j] == g}
            assert len(vals) == 1 and vals != {()}, (g, vals)                 # every member of a gang on nodes of one value of label 3
    elif kind == "offgrid":
        assert r1.preempted, "nothing was preempted"
    for x in (s, f, o):
        x.close()


def _drain_wl():
    """100 busy nodes and 30 idle ones behind them (the last rows: dropping them renumbers nothing, so the cordoned and the dropped round can be compared as they
    are).  The idle nodes' capacity counts towards every fair share while they are in the table."""
    wl = W.small_random(n_nodes=100, n_jobs=1500, n_queues=5, seed=4102, occupied=0.8, gangs=4)
    w = copy.copy(wl)
    w.node_total = np.concatenate([wl.node_total, np.tile(wl.node_total[:1], (30, 1))])
    for f in ("node_taints", "node_labels"):
        if getattr(wl, f) is not None:
            setattr(w, f, list(getattr(wl, f)) + [[] for _ in range(30)])
    if wl.node_id_rank is not None:
        w.node_id_rank = np.concatenate([np.asarray(wl.node_id_rank), 100 + np.arange(30)])
    return w


def test_a_cordoned_idle_node_dropped_is_the_references_rule(lib, oracle_lib):
    """scheduling_algo.go:1069-1077: an unschedulable node that holds no job is not in the NodeDb, "so the resource of the node is not counted for fairshare".  The
    round after the drop is the oracle's on the reduced table, and it is NOT the round with the nodes merely cordoned — by the oracle alone, too"""
    wl = _drain_wl()
    idle = np.arange(100, 130, dtype=np.int32)
    assert not np.isin(wl.job_node, idle).any()
    cordoned = _state(wl, idle)
    s = _load(lib, wl, _state(wl))
    s.nodes_patch(idle, unschedulable=1)                               # the drain: cordon ...
    r_cordoned, _ = NP._round(s, wl)
    s.nodes_delete(idle)                                               # ... and, the nodes holding nothing, drop
    assert s.nodes_delete_stats()[:5] == [30, 0, 0, 0, 100]
    r_dropped, _ = NP._round(s, wl)
    w1, state1, _ = _wl_reduced(wl, cordoned, idle)
    o_cordoned, o_dropped = _load(oracle_lib, wl, cordoned), _load(oracle_lib, w1, state1)
    ro_cordoned, _ = NP._round(o_cordoned, wl)
    ro_dropped, _ = NP._round(o_dropped, w1)
    scenario.assert_same_round(ro_cordoned, r_cordoned)
    scenario.assert_same_round(ro_dropped, r_dropped)
    assert NP._different(ro_cordoned, ro_dropped), "the oracle schedules the same round with the idle nodes cordoned and dropped: the case pins nothing"
    assert NP._different(r_cordoned, r_dropped)
    assert (s.total_resources() == w1.node_total.sum(axis=0)).all()
    for x in (s, o_cordoned, o_dropped):
        x.close()


# ---------------------------------------------------------------- e. interplay
@pytest.mark.parametrize("order", ["jobs_patch, jobs_append, nodes_patch, nodes_delete, jobs_delete", "nodes_delete, jobs_delete, nodes_patch, jobs_append, jobs_patch"])
def test_second_cycle_with_the_other_incremental_calls(lib, oracle_lib, order):
    wl = NP._round_wl("offgrid")
    full, head, tail = JA._split(wl, "any")
    state = _state(full)
    a = _load(lib, head, state)
    r1, _ = NP._round(a, head)
    w2, jrows = JA._second_cycle(full, r1, 5)
    # the nodes that leave hold nothing in the second cycle's table
    held = np.zeros(full.num_nodes, bool)
    held[w2.job_node[w2.job_node >= 0]] = True
    rows = np.array(_safe_rows(full, np.nonzero(~held)[0][:9]), dtype=np.int32)
    if len(rows) < 3:                                                  # (a full cluster: end the runs of three nodes in the second cycle's table)
        rows = np.array(_safe_rows(full, [3, 64, 127]), dtype=np.int32)
        w2, more = _wl_unbound(w2, rows)
        jrows = np.union1d(jrows, more).astype(np.int32)
    keepn = np.ones(full.num_nodes, bool)
    keepn[rows] = False
    new_id = _id_map(keepn)
    patch_old = np.nonzero(keepn)[0][[1, 40]].astype(np.int32)         # two surviving nodes are cordoned, by their position at the time of the call
    gone_jobs = np.nonzero((w2.job_node < 0) & (np.arange(w2.num_jobs) % 97 == 5) & (w2.job_gang < 0))[0].astype(np.int32)
    deleted = {"nodes": False, "jobs": False}

    def node_pos(v):
        return new_id[v] if deleted["nodes"] else v

    def jobs_patch():
        assert not deleted["jobs"]
        nd = w2.job_node[jrows]
        a.jobs_patch(jrows, np.where(nd >= 0, node_pos(np.maximum(nd, 0)), -1).astype(np.int32), w2.job_run_prio[jrows], w2.job_run_ts[jrows])

    def nodes_delete():
        if not patched["jobs"]:                                        # the runs that end in the second cycle may sit on the rows: say so first
            on = np.nonzero(np.isin(head.job_node, rows))[0].astype(np.int32)
            on = on[w2.job_node[on] != head.job_node[on]]
            if len(on):
                a.jobs_patch(on, np.full(len(on), -1, np.int32), 0, 0)
        got = a.nodes_delete(rows, want_map=True)
        assert got.tolist() == new_id.tolist()
        deleted["nodes"] = True

    patched = {"jobs": False}
    calls = {"jobs_patch": lambda: (jobs_patch(), patched.update(jobs=True)), "jobs_append": lambda: JA._append_tail(a, full, tail),
             "nodes_patch": lambda: a.nodes_patch(node_pos(patch_old).astype(np.int32), unschedulable=1), "nodes_delete": nodes_delete,
             "jobs_delete": None}
    names = order.split(", ")
    if names.index("jobs_delete") < names.index("jobs_append") or names.index("jobs_delete") < names.index("jobs_patch"):
        names.remove("jobs_delete"); names.append("jobs_delete")      # (rows of the second cycle's table: it comes once the table has them all, in either order of the node calls)
    for name in names:
        if name == "jobs_delete":
            jmap = a.jobs_delete(gone_jobs, want_map=True)
            deleted["jobs"] = True
        else:
            calls[name]()
    assert a.nodes_delete_stats()[0] == len(rows)
    # the fresh side: the second cycle's workload on the reduced node table, then the same job rows deleted
    st2 = _state(w2)
    st2["unschedulable"][patch_old] = 1
    w1, state1, _ = _wl_reduced(w2, st2, rows)
    ra, sta = _round_deleted(a, w1, jmap)
    f, o = _load(lib, w1, state1), _load(oracle_lib, w1, state1)
    f.jobs_delete(gone_jobs)
    rf, stf = _round_deleted(f, w1, jmap)
    o.close()
    o = _load_without_jobs(oracle_lib, w1, state1, jmap)
    ro, _ = NP._round(o[0], o[1])
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert sta["fast_iterations"] == stf["fast_iterations"]
    for x in (a, f, o[0]):
        x.close()


def _without_jobs(wl, jmap):
    """the workload without the job rows jmap sends to -1 (tests/test_z_jobs_delete.py's reduction, for the fields a round needs)"""
    keep = jmap >= 0
    w = copy.copy(wl)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class", "job_away"):
        v = getattr(wl, f)
        if v is not None:
            setattr(w, f, np.asarray(v)[keep])
    w.queued = [np.array([jmap[j] for j in q if jmap[j] >= 0], dtype=np.int32) for q in wl.queued]
    return w


def _round_deleted(s, wl, jmap):
    return NP._round(s, _without_jobs(wl, jmap))


def _load_without_jobs(lib, wl, state, jmap):
    w = _without_jobs(wl, jmap)
    return _load(lib, w, state), w


def test_delete_on_a_handle_without_a_job_table_then_jobs_set(lib):
    wl = NP._round_wl("offgrid")
    rows = np.array(_safe_rows(wl, [0, 63, 64, 129]), dtype=np.int32)
    w2, _ = _wl_unbound(wl, rows)
    state = _state(wl)
    s = Scheduler(lib, wl.config)
    s.nodes_upsert(wl.node_total, state["allocatable"], taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank)
    got = s.nodes_delete(rows, want_map=True)
    w1, state1, want = _wl_reduced(w2, state, rows)
    assert got.tolist() == want.tolist() and s.nodes_delete_stats()[:5] == [len(rows), 0, 0, 0, w1.num_nodes]
    assert s.total_resources().tolist() == w1.node_total.sum(axis=0).tolist()
    W.set_jobs(s, w1)
    r, _ = NP._round(s, w1)
    f = _load(lib, w1, state1)
    rf, _ = NP._round(f, w1)
    scenario.assert_same_round(rf, r)
    s.close(); f.close()


def test_delete_then_nodes_upsert_and_nodes_patch_of_the_new_last_row(lib):
    t = Table()
    s, t1, _ = _delete_and_compare(lib, t, [0, 64, 129], "before the patch")
    last = t1.n - 1
    assert last == 126
    s.nodes_patch([last], unschedulable=1 - int(t1.unschedulable[last]), allocatable=t1.total[[last]] // 2 // np.array([128 * W.Mi, 1000, 1, 1]) * np.array([128 * W.Mi, 1000, 1, 1]))
    with pytest.raises(SchedError) as e:
        s.nodes_patch([last + 1], unschedulable=1)                     # the old last row is no row any more
    assert e.value.code == ERR_INVALID
    p = copy.copy(t1)
    p.unschedulable, p.allocatable = t1.unschedulable.copy(), t1.allocatable.copy()
    p.unschedulable[last] = 1 - t1.unschedulable[last]
    p.allocatable[last] = t1.total[last] // 2 // np.array([128 * W.Mi, 1000, 1, 1]) * np.array([128 * W.Mi, 1000, 1, 1])
    _compare(lib, s, p, "after the patch")
    t.upsert(s)                                                        # the whole table again: the job table's runs are the caller's to put back
    s.jobs_set(t.req, queue=t.queue, pc=t.pc, req_class=t.cls, class_tolerations=t.tolerations, class_selectors=t.selectors, node=t.node, scheduled_at_priority=t.prio, run_timestamp=t.ts)
    assert s.nodes_delete_stats() == [0] * 8
    _compare(lib, s, t, "after nodes_upsert")
    s.close()


def test_evictor_report_and_preemption_causes_after_a_delete(lib):
    wl = NP._round_wl("offgrid")
    rows = np.array(_safe_rows(wl, [2, 63, 64, 100]), dtype=np.int32)
    w2, jobs = _wl_unbound(wl, rows)
    state = _state(wl, cordoned=[7, 70])
    s = _load(lib, wl, state)
    s.set_evictor_report(True)
    NP._round(s, wl)
    if len(jobs):
        s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
    s.nodes_delete(rows)
    w1, state1, _ = _wl_reduced(w2, state, rows)
    f = _load(lib, w1, state1)
    f.set_evictor_report(True)
    rs, _ = NP._round(s, w1)
    rf, _ = NP._round(f, w1)
    scenario.assert_same_round(rf, rs)
    es, ef = s.round_evictor_report(), f.round_evictor_report()
    assert es.keys() == ef.keys()
    for k in es:
        assert np.array_equal(np.asarray(es[k]), np.asarray(ef[k])), k
    assert len(es["node_reasons"]) == w1.num_nodes
    cs, cf = s.preemption_causes(), f.preemption_causes()
    assert cs.keys() == cf.keys()
    for k in cs:
        assert _plain(cs[k]) == _plain(cf[k]), k
    s.close(); f.close()


def _plain(x):
    return x.tolist() if isinstance(x, np.ndarray) else [_plain(y) for y in x] if isinstance(x, (list, tuple)) else x


# ---------------------------------------------------------------- f. the rebuild path
def _rebuild_case(name):
    t = Table()
    if name == "the last node of a type":
        return t, [10, 115], 2                                         # the only tainted and unschedulable nodes with label value 1 (45 and 80 carry value 0)
    t.labels = [list(x) for x in t.labels]
    t.labels[77] = [(3, 9)]                                            # the only node with value 9 of the indexed label
    return t, [77], 4


@pytest.mark.parametrize("name", ["the last node of a type", "the last node of a label value"])
def test_rebuild_path(lib, oracle_lib, name):
    t, rows, why = _rebuild_case(name)
    s, t1, st = _delete_and_compare(lib, t, rows, name, oracle=oracle_lib)
    assert st[2:4] == [1, why], st
    if why == 4:
        assert sorted(t.types()[1]) == [0, 1, 9] and s.indexed_node_label_values(3) == [0, 1]
    # a later device-path delete still works
    rows2 = _rows(33, t1.n, seed=9)
    assert t1.types(rows2) == t1.types()
    t2, jobs = t1.unbound(rows2)
    if len(jobs):
        s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
    s.nodes_delete(rows2)
    assert s.nodes_delete_stats()[2:4] == [0, 0]
    t3, _ = t2.reduced(rows2)
    _compare(lib, s, t3, "a device-path delete after the rebuild", oracle=oracle_lib)
    s.close()


def test_rebuild_path_on_a_table_at_the_edge_of_what_the_rebuild_refuses(lib):
    """tests/test_z_jobs_append.py ManyTypes: LIT_TMAX + 1 populated node types behind one requirement class, served by packed keys as long as allocatable is on the
    index grid — one step from what nodes_upsert's code refuses (more than LIT_TMAX types on the literal path).  What the rebuild would refuse is decided first by the
    code asched_nodes_patch uses (rebuildRefusal); for a REDUCED table it cannot fire: every aggregate it looks at (the widths of the key, alignment, the number of
    populated types) can only tighten when rows leave, which is why no case here provokes it.  Pinned instead: the rebuild path of a delete goes through that decision
    on this table and leaves what a fresh handle holds"""
    t = JA.ManyTypes()
    n = len(t.labels)
    rows = [3, 3 + n // 2]                                             # both nodes of one type: its label value leaves with them
    s = t.handle(lib)
    got = s.nodes_delete(rows, want_map=True)
    assert s.nodes_delete_stats()[:5] == [2, 0, 1, 4, n - 2] and (got[rows] == -1).all()
    r = copy.copy(t)
    keep = got >= 0
    r.node_total, r.labels = t.node_total[keep], [x for x, k in zip(t.labels, keep) if k]
    f = r.handle(lib)
    assert t.view(s) == t.view(f) and s.node_types_matching_job(0) == f.node_types_matching_job(0) and s.get_nodes_alloc().tolist() == f.get_nodes_alloc().tolist()
    s.close(); f.close()


# ---------------------------------------------------------------- g. refusals
def _raw(s, n, node=None):
    """through the C entry point: what the binding cannot express"""
    import ctypes as C
    a = None if node is None else np.ascontiguousarray(node, dtype=np.int32)
    return s.lib.nodes_delete(s.h, n, None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)), None)


def test_refusals_leave_the_handle_as_it_was(lib):
    t = Table()
    s = t.handle(lib)
    f = t.handle(lib)
    want = view(f, t, 5)
    rwant = t.round(f)
    busy = int(t.node[t.node >= 0].max())
    lowest = int(np.nonzero(np.isin(t.node, [busy, 5]))[0].min())
    bad = [(ERR_INVALID, lambda: _raw(s, -1, node=[0])),                                           # n < 0
           (ERR_INVALID, lambda: _raw(s, 2)),                                                      # n > 0 without node
           (ERR_INVALID, lambda: s.nodes_delete([0, N])),                                          # a row outside [0, N)
           (ERR_INVALID, lambda: s.nodes_delete([-1])),
           (ERR_INVALID, lambda: s.nodes_delete([3, 7, 3])),                                       # a row named twice
           (ERR_INVALID, lambda: s.nodes_delete([busy, 5])),                                       # a resident job whose run is on a named row
           (ERR_UNSUPPORTED, lambda: s.nodes_delete(np.arange(N)))]                                # every row named
    for k, (code, call) in enumerate(bad):
        n_before = s.num_nodes
        try:
            rc = call()
            msg = (s.lib.last_error(s.h) or b"").decode()
        except SchedError as e:
            rc, msg = e.code, str(e)
            s.num_nodes = n_before
        assert rc == code and msg, (k, rc, code)
        if k == 5:
            assert f"job row {lowest} " in msg, msg                                               # the lowest such job row
        assert s.lib.num_nodes(s.h) == N
        got = view(s, t, 5)
        assert got == want, k
    scenario.assert_same_round(rwant, t.round(s))                                                  # (and a round, once: the answers above are those of a handle that has run none)
    # after jobs_patch(node = -1) of the jobs on those rows the same call succeeds
    t2, jobs = t.unbound([busy, 5])
    assert lowest == int(jobs.min())
    s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
    s.nodes_delete([busy, 5])
    t1, _ = t2.reduced([busy, 5])
    _compare(lib, s, t1, "after the refusals")
    s.close(); f.close()


def test_handles_nodes_delete_does_not_serve(lib):
    wl = NP._refusal_wl()
    s = Scheduler(lib, wl.config)
    for rows in ([0], []):
        with pytest.raises(SchedError) as e:
            s.nodes_delete(rows)                                                                    # no node table
        assert e.value.code == ERR_INVALID
    W.set_jobs(s, wl)
    with pytest.raises(SchedError) as e:
        s.nodes_delete([0])
    assert e.value.code == ERR_INVALID
    for kw in (dict(alloc_by_prio=np.repeat(wl.node_total[:, None, :], s.P, axis=1)), dict(node_type_override=np.arange(wl.num_nodes) % 2)):
        s.nodes_upsert(wl.node_total, **kw)
        want, _ = NP._round(s, wl)
        for rows in ([0], []):
            with pytest.raises(SchedError) as e:
                s.nodes_delete(rows)
            assert e.value.code == ERR_UNSUPPORTED
            s.num_nodes = wl.num_nodes
            got, _ = NP._round(s, wl)
            scenario.assert_same_round(want, got)
    s.nodes_upsert(wl.node_total)                                                                  # a plain table again
    s.nodes_delete([])
    assert s.nodes_delete_stats() == [0, 0, 0, 0, wl.num_nodes, 0, 0, 0]
    s.close()


# ---------------------------------------------------------------- h. the simulator fixture with nodes drained and dropped
def test_simulator_cycles_draining(lib, oracle_lib):
    sim = S.from_fixture(FIXTURE)
    per_cycle = 90
    n = sim.workload.num_nodes
    events = [(1, "cordon", k) for k in range(4)] + [(1, "drop", k) for k in range(4)] + [(0, "cordon", n - 1), (0, "drop", n - 1)] + \
             [(3, "cordon", 20), (4, "drop", 20), (6, "drop", 30), (7, "cordon", 30), (9, "cordon", 64), (9, "drop", 64)]
    a = S.run_cycles_draining(lib, sim, events, per_cycle=per_cycle)
    b = S.run_cycles_draining_rebuilt(lib, sim, events, per_cycle=per_cycle)
    o = S.run_cycles_draining_rebuilt(oracle_lib, sim, events, per_cycle=per_cycle)
    cordoned = S.run_cycles_cordoning(lib, sim, [e for e in events if e[1] == "cordon"], per_cycle=per_cycle)
    m = sim.workload.num_jobs
    assert a[-1]["rows"] == m and sum(len(c["scheduled"]) for c in a) - sum(len(c["preempted"]) for c in a) == m     # until the workload drains
    assert JA._records(a) == JA._records(b) == JA._records(o)
    assert [c["nodes"] for c in a] == [c["nodes"] for c in b] == [c["nodes"] for c in o]
    assert a[0]["nodes"] == n - 1 and a[-1]["nodes"] <= n - 6, [c["nodes"] for c in a]           # the idle node left at once, the busy ones once their jobs had finished
    dropped = {0, 1, 2, 3, n - 1}
    assert not any(v in dropped for c in a[1:] for v in c["scheduled"].values())
    assert JA._records(a) != JA._records(cordoned), "dropping the drained nodes changed no cycle: the case pins nothing"


# ---------------------------------------------------------------- i. a library without the entry point
def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = NP._refusal_wl()
    s = W.load(oracle_lib, wl)
    for call in (lambda: s.nodes_delete([0]), s.nodes_delete_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    s.close()
