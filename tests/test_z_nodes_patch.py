"""asched_nodes_patch: cordons, over-allocation flags, allocatable and taints of resident nodes change between two scheduling cycles, on the device
(armada_amd/csrc/kernels_nodes_patch.h) — the library's counterpart of what populateNodeDb re-reads per node every cycle (scheduling_algo.go:1069-1095).  The contract:
after a patch the handle is what nodes_upsert of the patched table would have left.  The oracle has no patch: its side is always nodes_upsert of the patched table.

a. masks and NodeDb-level answers against a fresh handle, at the entry counts where the word grouping takes another turn; b. rounds against a fresh handle and the
oracle, a second cycle with jobs_patch and jobs_append in either order, a patch and its inverse; c. the evictor report after a cordon; d. the rebuild path; e. refusals;
f. the simulator fixture with a schedule of node events.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import scenario
import test_z_jobs_append as JA          # its table splitting and second-cycle helpers: the second cycle here appends and patches jobs as well
from armada_amd import simulator_input as S
from armada_amd import workloads as W
from armada_amd.binding import SchedError, Scheduler

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulator_basic_input.json")
UNSCHED_KEY = -2                          # the taint key the library gives an unschedulable node (include/armada_sched.h)


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


# ---------------------------------------------------------------- the table of a. and d.
PCS = ((0, True), (1, True), (3, False))
N, M = 130, 600                           # three mask words, the last one partial
FIELDS = ("allocatable", "unschedulable", "over_allocated", "taints")
KEPT = (80, 115)                          # never patched below 130 entries: with nodes 10 and 45 the only tainted AND unschedulable nodes of their label


class Table:
    """130 nodes of 8 populated node types (every taint is indexed: an indexed label with two values x the taint (7, 1, NoSchedule) on every fifth node x
    unschedulable on every seventh), 600 queued jobs of `ncls` requirement classes (class 1 tolerates key 7, class 3 the unschedulable taint, class 2 selects a
    label value) and three priority classes, two of them with away entries (mask rows behind the S shape rows), and two jobs no node can hold"""

    def __init__(self, ncls=4, seed=3):
        rng = np.random.default_rng(seed)
        self.cfg = W._config(list(PCS))
        self.cfg.indexed_taint_keys = None
        self.cfg.indexed_label_keys = [3]
        self.cfg.wkt_taints = [[(7, 1, 1)], [(7, -1, 1)]]
        self.cfg.pc_away = [[], [(0, 0)], [(2, 1), (1, 0)]]
        self.total = np.tile(np.array([64 * W.Gi, 16000, 512 * W.Gi, 0], dtype=np.int64), (N, 1))
        self.total[::9, W.GPU] = 4
        self.allocatable = self.total.copy()
        self.labels = [[(3, i % 2)] for i in range(N)]
        self.taints = [[(7, 1, 1)] if i % 5 == 0 else [] for i in range(N)]
        self.unschedulable = (np.arange(N) % 7 == 3).astype(np.uint8)
        self.over_allocated = np.zeros(N, np.uint8)
        shapes = W._shapes64()[::5]
        self.req = shapes[rng.integers(0, len(shapes), size=M)].copy()
        self.req[rng.random(M) < 0.1, W.GPU] = 1
        self.req[-2:, W.CPU] = 17000                                # more than any node's total
        self.queue = rng.integers(0, 3, size=M).astype(np.int32)
        self.pc = rng.integers(0, 3, size=M).astype(np.int32)
        self.cls = rng.integers(0, ncls, size=M).astype(np.int32)
        self.cls[-2:] = (0, 1)
        self.tolerations = [[], [(7, 1, 0, 0)], [], [(UNSCHED_KEY, 1, 0, 0)]] + [[(7, 0, 1, 1), (100 + c, 1, 0, 0)] for c in range(4, ncls)]
        self.selectors = [[], [], [(3, 1)], []] + [[] for _ in range(4, ncls)]

    def handle(self, lib):
        s = Scheduler(lib, self.cfg)
        s.nodes_upsert(self.total, self.allocatable, unschedulable=self.unschedulable, over_allocated=self.over_allocated, taints=self.taints, labels=self.labels)
        s.jobs_set(self.req, queue=self.queue, pc=self.pc, req_class=self.cls, class_tolerations=self.tolerations, class_selectors=self.selectors)
        return s

    def patched(self, rows, **fields):
        """the table nodes_upsert would be given: `fields` replaced in `rows`"""
        t = copy.copy(self)
        for f, v in fields.items():
            if f == "taints":
                t.taints = list(self.taints)
                for r, x in zip(rows, v):
                    t.taints[int(r)] = list(x)
            else:
                a = getattr(self, f).copy()
                a[np.asarray(rows, dtype=np.int64)] = v
                setattr(t, f, a)
        return t

    def new_values(self, rows, fields, seed=0):
        """new values of `fields` for `rows` that keep every node type populated and every allocatable on the index grid, inside [0, total]"""
        rng = np.random.default_rng(1000 + seed)
        rows = np.asarray(rows, dtype=np.int64)
        n = len(rows)
        out = {}
        src = (rows + 2) % N if n == N else None                     # all rows: every row takes the state of the next row but one, which has its label
        for f in fields:
            if f == "allocatable":
                cut = np.stack([rng.integers(0, 100, n) * 128 * W.Mi, rng.integers(0, 9, n) * 1000, np.zeros(n, np.int64), np.zeros(n, np.int64)], axis=1)
                out[f] = self.total[rows] - cut
            elif f == "unschedulable":
                out[f] = self.unschedulable[src] if n == N else 1 - self.unschedulable[rows]
            elif f == "over_allocated":
                out[f] = rng.integers(0, 2, n).astype(np.uint8)
            else:
                out[f] = [self.taints[int(k)] for k in src] if n == N else [[] if self.taints[int(r)] else [(7, 1, 1)] for r in rows]
        return out

    def round(self, s):
        queued = [np.nonzero(self.queue == q)[0].astype(np.int32) for q in range(3)]
        pcp = np.array([p for p, _ in PCS])[self.pc]
        queued = [q[np.lexsort((q, -pcp[q]))] for q in queued]
        s.round_prepare(np.ones(3), queued, global_tokens=1e18, global_burst=1 << 62, global_rate_inf=True, queue_tokens=[1e18] * 3, queue_burst=[1 << 62] * 3, queue_rate_inf=[True] * 3)
        return s.schedule_round()


def rows_of(n):
    """n nodes: the word edges first (two of them in one word from n = 2 on), then a seeded draw of the rest"""
    first = [0, 63, 64, 127, 128, 129]
    rest = [int(k) for k in np.random.default_rng(42).permutation(N) if int(k) not in first and (n == N or int(k) not in KEPT)]
    return np.array((first + rest)[:n], dtype=np.int32)


def view(s):
    """the NodeDb-level answers of a handle that has nodes and jobs and no round: every job's first fit at every priority, the node types that match it, the totals,
    every plane, a node iteration per priority, a submit-check batch, and the exclusion reasons of the two selections that cannot succeed"""
    jobs = np.arange(M, dtype=np.int32)
    out = [s.fit_select_batch(jobs, p).tolist() for p in s.priorities]
    out.append([s.node_types_matching_job(int(j)) for j in jobs[::3]])
    out += [s.total_resources().tolist(), s.get_nodes_alloc().tolist(), s.num_nodes]
    out += [s.iterate_nodes(p, [4000, 8 * W.Gi, 0]) for p in s.priorities]
    out.append(s.submit_check([[int(j)] for j in jobs[::7]]))
    excl = []
    for j in (M - 2, M - 1):
        assert s.select_node(j)[0].node < 0
        excl.append(s.excluded_nodes(j))
    out.append(excl)
    return out, excl


def test_the_patched_table_is_what_nodes_upsert_is_given(lib, oracle_lib):
    """a pin of this file's own helpers, not of the feature: Table.patched and Table.new_values build the table every case below uploads to its fresh handle — the
    library and the oracle agree on it, its totals are the column sums and an unschedulable node is excluded for its taint.  It calls no nodes_patch, so it also
    passes without the feature."""
    t = Table()
    rows = rows_of(65)
    assert len(set(rows.tolist())) == 65 and {0, 63, 64, 127, 128, 129} <= set(rows.tolist()) and not set(KEPT) & set(rows.tolist()) and len(rows_of(N)) == N
    p = t.patched(rows, **t.new_values(rows, FIELDS))
    assert (p.allocatable[rows] <= t.total[rows]).all() and (p.allocatable >= 0).all() and (p.unschedulable[rows] != t.unschedulable[rows]).all()
    assert (np.delete(p.allocatable, rows, axis=0) == np.delete(t.allocatable, rows, axis=0)).all()
    s, o = p.handle(lib), p.handle(oracle_lib)
    jobs = np.arange(M, dtype=np.int32)
    for prio in s.priorities:
        assert s.fit_select_batch(jobs, prio).tolist() == o.fit_select_batch(jobs, prio).tolist()
    assert s.total_resources().tolist() == p.allocatable.sum(axis=0).tolist()
    _, excl = view(s)
    assert any(r[0] == "untolerated_taint" and r[1] == UNSCHED_KEY for r in excl[0])
    s.close(); o.close()


# ---------------------------------------------------------------- a. masks and NodeDb-level answers against a fresh handle
COUNTS = [0, 1, 2, 63, 64, 65, 130]


def _patch_and_compare(lib, t, rows, fields, seed=0):
    new = t.new_values(rows, fields, seed)
    s = t.handle(lib)
    s.nodes_patch(rows, **new)
    st = s.nodes_patch_stats()
    p = t.patched(rows, **new)
    f = p.handle(lib)
    got, excl = view(s)
    want, _ = view(f)
    assert got == want, (fields, len(rows))
    f.close()
    return s, p, st, excl


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("fields", [(f,) for f in FIELDS] + [FIELDS], ids=list(FIELDS) + ["all"])
def test_answers_after_a_patch_of_n_rows(lib, fields, n):
    t = Table()
    rows = rows_of(n)
    s, p, st, excl = _patch_and_compare(lib, t, rows, fields, n)
    assert st[0] == n and st[2] == 0 and st[3] == 0 and st[4:] == [0, 0, 0, 0], st
    if n and ("unschedulable" in fields or "taints" in fields):
        assert st[1] > 0, st                                       # every taint is indexed: these rows moved to another node type
    assert p.unschedulable.any() and any(r[0] == "untolerated_taint" and r[1] == UNSCHED_KEY for r in excl[0]), "the unschedulable taint is reported as a == -2"
    s.close()


@pytest.mark.parametrize("n", [2, 65, 130])
def test_answers_after_a_patch_with_65_requirement_classes(lib, n):
    """more classes than a node's class word holds: no fast structure, two words of class bits per entry"""
    t = Table(ncls=65)
    s, _, st, _ = _patch_and_compare(lib, t, rows_of(n), FIELDS, n)
    assert st[0] == n and st[2] == 0, st
    s.close()


def test_patches_one_after_the_other_and_nodes_upsert_in_between(lib):
    """every patch finds what the one before it left; nodes_upsert puts the statistics back to zero"""
    t = Table()
    s = t.handle(lib)
    for k, n in enumerate((65, 2, 130, 0, 63)):
        rows = rows_of(n)
        new = t.new_values(rows, FIELDS if k % 2 == 0 else ("unschedulable", "allocatable"), 50 + k)
        if n == N:
            new = {f: v for f, v in new.items() if f in ("allocatable", "over_allocated")}   # (the rotation of new_values is defined on the base table only)
        s.nodes_patch(rows, **new)
        assert s.nodes_patch_stats()[:3] == [n, s.nodes_patch_stats()[1], 0]
        t = t.patched(rows, **new)
        f = t.handle(lib)
        assert view(s)[0] == view(f)[0], k
        f.close()
    s.nodes_upsert(t.total, t.allocatable, unschedulable=t.unschedulable, over_allocated=t.over_allocated, taints=t.taints, labels=t.labels)
    assert s.nodes_patch_stats() == [0] * 8
    f = t.handle(lib)
    assert view(s)[0] == view(f)[0]
    s.close(); f.close()


# ---------------------------------------------------------------- b. rounds
def _load(lib, wl, nodes):
    s = Scheduler(lib, wl.config)
    s.nodes_upsert(wl.node_total, nodes["allocatable"], unschedulable=nodes["unschedulable"], over_allocated=nodes["over_allocated"], taints=wl.node_taints,
                   labels=wl.node_labels, id_rank=wl.node_id_rank)
    W.set_jobs(s, wl)
    return s


def _round(s, wl):
    W.prepare(s, wl)
    r = s.schedule_round()
    return r, s.round_stats()


def _different(a, b):
    return a.scheduled != b.scheduled or a.preempted != b.preempted


def _round_wl(kind):
    if kind == "ragged":
        return W.small_random(n_nodes=N, n_jobs=1500, n_queues=5, seed=4101, occupied=0.8, gangs=4, away=True, ragged=True)
    return W.small_random(n_nodes=N, n_jobs=1500, n_queues=5, seed=4102, occupied=0.8, gangs=4, away=True, offgrid=1)


def _node_state(wl, seed):
    """the base node state of a round case (five nodes cordoned) and a patch of it: six nodes that hold running jobs are cordoned, three are uncordoned, four lose
    allocatable (on the index grid), and one more is cut below what its jobs hold, cordoned and flagged over-allocated"""
    rng = np.random.default_rng(seed)
    n = wl.num_nodes
    alloc0 = wl.node_total.copy() if wl.node_allocatable is None else wl.node_allocatable.copy()
    held = np.zeros_like(wl.node_total)
    run = np.nonzero(wl.job_node >= 0)[0]
    np.add.at(held, wl.job_node[run], wl.job_req[run])
    busy = rng.permutation(np.nonzero(held[:, W.CPU] > 0)[0])
    base = dict(allocatable=alloc0, unschedulable=np.zeros(n, np.uint8), over_allocated=np.zeros(n, np.uint8))
    cordoned0, cordon, cut, over = busy[:5], busy[5:11], busy[11:15], busy[15]
    base["unschedulable"][cordoned0] = 1
    rows = np.concatenate([cordon, cordoned0[:3], cut, [over]]).astype(np.int32)
    new = {k: v[rows].copy() for k, v in base.items()}
    new["unschedulable"][:6] = 1
    new["unschedulable"][6:9] = 0
    new["allocatable"][9:13, W.CPU] = np.maximum(new["allocatable"][9:13, W.CPU] // 1000 * 1000 - 4000, 0)
    new["allocatable"][9:13, W.MEM] = np.maximum(new["allocatable"][9:13, W.MEM] // (128 * W.Mi) * (128 * W.Mi) - 16 * W.Gi, 0)
    new["allocatable"][13] = held[over] // 2 // np.array([128 * W.Mi, 1000, 1, 1]) * np.array([128 * W.Mi, 1000, 1, 1])
    new["unschedulable"][13], new["over_allocated"][13] = 1, 1
    assert (new["allocatable"][13] <= held[over]).all() and new["allocatable"][13, W.CPU] < held[over, W.CPU]
    after = {k: v.copy() for k, v in base.items()}
    for k in after:
        after[k][rows] = new[k]
    return base, rows, new, after


@pytest.mark.parametrize("kind", ["ragged", "offgrid"])
def test_round_after_a_patch(lib, oracle_lib, kind):
    wl = _round_wl(kind)
    base, rows, new, after = _node_state(wl, 7)
    s = _load(lib, wl, base)
    r0, _ = _round(s, wl)                                          # (the patch finds a handle that has run a round)
    s.nodes_patch(rows, **new)
    assert s.nodes_patch_stats()[2] == 0, s.nodes_patch_stats()
    with pytest.raises(SchedError):
        s.schedule_round()                                         # round_prepare first, as after nodes_upsert
    r1, st1 = _round(s, wl)
    f = _load(lib, wl, after)
    rf, stf = _round(f, wl)
    o = _load(oracle_lib, wl, after)
    ro, _ = _round(o, wl)
    scenario.assert_same_round(rf, r1)
    scenario.assert_same_round(ro, r1)
    assert _different(r0, r1), "the patched round equals the unpatched one: the case pins nothing"
    assert st1["fast_iterations"] == stf["fast_iterations"]
    if kind == "offgrid":
        assert st1["fast_iterations"] > 0
    # a patch followed by its inverse gives the original round
    s.nodes_patch(rows, **{k: v[rows] for k, v in base.items()})
    assert s.nodes_patch_stats()[2] == 0
    r2, _ = _round(s, wl)
    scenario.assert_same_round(r0, r2)
    for x in (s, f, o):
        x.close()


@pytest.mark.parametrize("order", ["jobs_patch, jobs_append, nodes_patch", "nodes_patch, jobs_append, jobs_patch"])
@pytest.mark.parametrize("kind", ["ragged", "offgrid"])
def test_second_cycle_with_jobs_patch_and_jobs_append(lib, oracle_lib, kind, order):
    wl = _round_wl(kind)
    full, head, tail = JA._split(wl, "any")                        # (rows with new shapes: the append rebuilds the masks from the host mirrors a node patch keeps)
    base, rows1, new1, after1 = _node_state(full, 8)
    a = _load(lib, head, base)
    a.nodes_patch(rows1, **new1)
    r1, _ = _round(a, head)
    w2, jrows = JA._second_cycle(full, r1, 5)
    # the second node patch: two of the cordoned nodes come back, two others are cordoned, one more cut
    rng = np.random.default_rng(9)
    cordoned = np.nonzero(after1["unschedulable"])[0]
    free = rng.permutation(np.nonzero(after1["unschedulable"] == 0)[0])
    rows2 = np.concatenate([cordoned[:2], free[:3]]).astype(np.int32)
    new2 = {k: v[rows2].copy() for k, v in after1.items()}
    new2["unschedulable"][:2], new2["over_allocated"][:2] = 0, 0
    new2["unschedulable"][2:4] = 1
    new2["allocatable"][4, W.CPU] = max(int(new2["allocatable"][4, W.CPU]) // 1000 * 1000 - 3000, 0)
    after2 = {k: v.copy() for k, v in after1.items()}
    for k in after2:
        after2[k][rows2] = new2[k]
    calls = {"jobs_patch": lambda: a.jobs_patch(jrows, w2.job_node[jrows], w2.job_run_prio[jrows], w2.job_run_ts[jrows]),
             "jobs_append": lambda: JA._append_tail(a, full, tail), "nodes_patch": lambda: a.nodes_patch(rows2, **new2)}
    for name in order.split(", "):
        calls[name]()
    assert a.nodes_patch_stats()[:3] == [len(rows2), 0, 0] and a.jobs_append_stats()["rows"] == len(tail)
    ra, sta = _round(a, w2)
    f = _load(lib, w2, after2)
    rf, stf = _round(f, w2)
    o = _load(oracle_lib, w2, after2)
    ro, _ = _round(o, w2)
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert sta["fast_iterations"] == stf["fast_iterations"]
    for x in (a, f, o):
        x.close()


def test_patch_of_a_handle_without_a_job_table_then_jobs_set(lib):
    wl = _round_wl("offgrid")
    base, rows, new, after = _node_state(wl, 7)
    s = Scheduler(lib, wl.config)
    s.nodes_upsert(wl.node_total, base["allocatable"], unschedulable=base["unschedulable"], over_allocated=base["over_allocated"], taints=wl.node_taints, labels=wl.node_labels)
    s.nodes_patch(rows, **new)
    assert s.nodes_patch_stats()[:3] == [len(rows), 0, 0] and s.total_resources().tolist() == after["allocatable"].sum(axis=0).tolist()
    W.set_jobs(s, wl)
    r, _ = _round(s, wl)
    f = _load(lib, wl, after)
    rf, _ = _round(f, wl)
    scenario.assert_same_round(rf, r)
    s.close(); f.close()


# ---------------------------------------------------------------- c. the evictor report after a cordon
def test_evictor_report_after_a_cordon(lib):
    from armada_amd.binding import EVR_NODE_UNSCHEDULABLE
    wl = _round_wl("offgrid")
    base, rows, new, after = _node_state(wl, 7)
    s, f = _load(lib, wl, base), _load(lib, wl, after)
    for x in (s, f):
        x.set_evictor_report(True)
    _round(s, wl)
    s.nodes_patch(rows, **new)
    rs, _ = _round(s, wl)
    rf, _ = _round(f, wl)
    scenario.assert_same_round(rf, rs)
    es, ef = s.round_evictor_report(), f.round_evictor_report()
    assert es.keys() == ef.keys()
    for k in es:
        assert np.array_equal(np.asarray(es[k]), np.asarray(ef[k])), k
    unsched = (es["node_reasons"] & EVR_NODE_UNSCHEDULABLE) != 0
    assert unsched.tolist() == after["unschedulable"].astype(bool).tolist()
    s.close(); f.close()


# ---------------------------------------------------------------- d. the rebuild path
def _rebuild_case(name):
    t = Table()
    if name == "a taint set never seen":
        return t, [5, 64], dict(taints=[[(11, 5, 1)], [(7, 1, 1), (11, 5, 1)]]), 1
    if name == "the last node of a type patched away":
        return t, [10, 80], dict(taints=[[], []]), 2             # the only tainted and unschedulable nodes with label value 0
    if name == "an allocatable above the key layout":
        big = t.total[[3, 129]].copy()
        big[:, W.CPU] = 32000
        return t, [3, 129], dict(allocatable=big), 3
    raise KeyError(name)


@pytest.mark.parametrize("name", ["a taint set never seen", "the last node of a type patched away", "an allocatable above the key layout"])
def test_rebuild_path(lib, oracle_lib, name):
    t, rows, new, why = _rebuild_case(name)
    s = t.handle(lib)
    s.nodes_patch(rows, **new)
    assert s.nodes_patch_stats()[:4] == [len(rows), s.nodes_patch_stats()[1], 1, why]
    p = t.patched(rows, **new)
    f = p.handle(lib)
    assert view(s)[0] == view(f)[0]
    o = p.handle(oracle_lib)
    rs, rf, ro = p.round(s), p.round(f), p.round(o)
    scenario.assert_same_round(rf, rs)
    scenario.assert_same_round(ro, rs)
    f.close(); o.close()
    # a later device-path patch still works
    rows2 = rows_of(64)
    new2 = p.new_values(rows2, ("allocatable", "over_allocated"), 3)
    s.nodes_patch(rows2, **new2)
    assert s.nodes_patch_stats()[:4] == [64, 0, 0, 0]
    q = p.patched(rows2, **new2)
    f = q.handle(lib)
    assert view(s)[0] == view(f)[0]
    scenario.assert_same_round(q.round(f), q.round(s))
    s.close(); f.close()


def test_rebuild_path_for_a_value_off_the_coarse_divisor(lib, oracle_lib):
    """W.fine_indexed(coarse=True): the key's fields are quotients by 250m / 32Mi / 2Gi instead of the index resolutions; a node that loses 100m is off that grid"""
    wl = W.fine_indexed(n_nodes=N, n_jobs=1500, n_queues=4, seed=77, k5=False, coarse=True)
    zeros = dict(unschedulable=np.zeros(N, np.uint8), over_allocated=np.zeros(N, np.uint8))
    s = _load(lib, wl, dict(allocatable=wl.node_total, **zeros))
    r0, st0 = _round(s, wl)
    assert st0["fast_iterations"] > 0, "the coarser divisor did not give this handle a one-word key"
    on = wl.node_total[[0, 64]].copy()
    on[:, W.CPU] -= 8000                                           # on the coarse grid: the device path
    s.nodes_patch([0, 64], allocatable=on)
    assert s.nodes_patch_stats()[:4] == [2, 0, 0, 0]
    off = wl.node_total[[1, 129]].copy()
    off[:, W.CPU] -= 8100
    s.nodes_patch([1, 129], allocatable=off)
    assert s.nodes_patch_stats()[:4] == [2, 0, 1, 3]
    alloc = wl.node_total.copy()
    alloc[[0, 64]], alloc[[1, 129]] = on, off
    rs, _ = _round(s, wl)
    f, o = _load(lib, wl, dict(allocatable=alloc, **zeros)), _load(oracle_lib, wl, dict(allocatable=alloc, **zeros))
    rf, _ = _round(f, wl)
    ro, _ = _round(o, wl)
    scenario.assert_same_round(rf, rs)
    scenario.assert_same_round(ro, rs)
    assert _different(r0, rs)
    # a later device-path patch still works
    alloc[[2, 63], W.MEM] -= 64 * W.Gi
    s.nodes_patch([2, 63], allocatable=alloc[[2, 63]])
    assert s.nodes_patch_stats()[2] == 0
    f.nodes_upsert(wl.node_total, alloc)
    scenario.assert_same_round(_round(f, wl)[0], _round(s, wl)[0])
    for x in (s, f, o):
        x.close()


# ---------------------------------------------------------------- e. refusals
def _refusal_wl():
    return W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=0.9, gangs=3)


def _raw(s, n, node=None, taint_off=None):
    """through the C structure: what the binding cannot express"""
    from armada_amd.binding import CNodesPatch
    p = CNodesPatch()
    p.n = n
    keep = []
    for name, v in (("node", node), ("taint_off", taint_off)):
        if v is not None:
            a = np.ascontiguousarray(v, dtype=np.int32)
            keep.append(a)
            setattr(p, name, a.ctypes.data_as(C.POINTER(C.c_int32)))
    if taint_off is not None:
        z = np.zeros(8, np.int32)
        keep.append(z)
        p.taint_key = p.taint_value = p.taint_effect = z.ctypes.data_as(C.POINTER(C.c_int32))
    return s.lib.nodes_patch(s.h, C.byref(p))


def test_refusals_leave_the_handle_as_it_was(lib):
    wl = _refusal_wl()
    n = wl.num_nodes
    s = W.load(lib, wl)
    want, _ = _round(s, wl)
    huge = np.array([[1 << 58, 1 << 58, 0, 1 << 58]], dtype=np.int64)
    bad = [(ERR_INVALID, lambda: _raw(s, -1, node=[0])),                                           # n < 0
           (ERR_INVALID, lambda: _raw(s, 2)),                                                      # n > 0 without node
           (ERR_INVALID, lambda: _raw(s, 2, node=[0, 1], taint_off=[0, 2, 1])),                    # a taint_off that is not ascending
           (ERR_INVALID, lambda: s.nodes_patch([0, n], unschedulable=1)),                          # a node outside [0, N)
           (ERR_INVALID, lambda: s.nodes_patch([-1], unschedulable=1)),
           (ERR_INVALID, lambda: s.nodes_patch([3, 7, 3], unschedulable=1)),                       # a node named twice
           (ERR_UNSUPPORTED, lambda: s.nodes_patch([2], allocatable=huge))]                        # the rebuild would refuse: an order key beyond 128 bits
    for code, call in bad:
        try:
            rc = call()
        except SchedError as e:
            rc = e.code
            assert str(e)
        assert rc == code, (rc, code)
        assert s.num_nodes == n
        got, _ = _round(s, wl)
        scenario.assert_same_round(want, got)
    s.nodes_patch([3, 7], unschedulable=1)                                                         # and the handle still patches (a row named twice left no mark)
    assert s.nodes_patch_stats()[:3] == [2, 0, 0]
    s.close()


def test_refusal_of_what_the_rebuild_would_refuse_on_the_literal_path(lib):
    """tests/test_z_jobs_append.py ManyTypes: LIT_TMAX + 1 populated node types behind one requirement class, served by packed keys as long as allocatable is on the
    index grid; one node off it would move the class to the literal iteration path, which serves at most LIT_TMAX types"""
    t = JA.ManyTypes()
    s, f = t.handle(lib), t.handle(lib)
    want = t.view(f)
    off = t.node_total[[5]].copy()
    off[:, W.CPU] -= 137
    for _ in range(2):
        with pytest.raises(SchedError) as e:
            s.nodes_patch([5], allocatable=off)
        assert e.value.code == ERR_UNSUPPORTED and "LIT_TMAX" in str(e.value)
        assert t.view(s) == want
    on = t.node_total[[5]].copy()
    on[:, W.CPU] -= 2000
    s.nodes_patch([5], allocatable=on)
    assert s.nodes_patch_stats()[:4] == [1, 0, 0, 0]
    f.nodes_upsert(np.concatenate([t.node_total[:5], on, t.node_total[6:]]), labels=t.labels)
    assert t.view(s) == t.view(f)
    s.close(); f.close()


def test_handles_nodes_patch_does_not_serve(lib):
    wl = _refusal_wl()
    s = Scheduler(lib, wl.config)
    for rows in ([0], []):
        with pytest.raises(SchedError) as e:
            s.nodes_patch(rows, unschedulable=1)                                                    # no node table
        assert e.value.code == ERR_INVALID
    W.set_jobs(s, wl)
    with pytest.raises(SchedError) as e:
        s.nodes_patch([0], unschedulable=1)
    assert e.value.code == ERR_INVALID
    for kw in (dict(alloc_by_prio=np.repeat(wl.node_total[:, None, :], s.P, axis=1)), dict(node_type_override=np.arange(wl.num_nodes) % 2)):
        s.nodes_upsert(wl.node_total, **kw)
        want, _ = _round(s, wl)
        for rows in ([0], []):
            with pytest.raises(SchedError) as e:
                s.nodes_patch(rows, unschedulable=1)
            assert e.value.code == ERR_UNSUPPORTED
            got, _ = _round(s, wl)
            scenario.assert_same_round(want, got)
    s.nodes_upsert(wl.node_total)                                                                  # a plain table again
    s.nodes_patch([0], unschedulable=1)
    s.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = _refusal_wl()
    s = W.load(oracle_lib, wl)
    for call in (lambda: s.nodes_patch([0], unschedulable=1), s.nodes_patch_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    s.close()


# ---------------------------------------------------------------- f. the simulator fixture with a schedule of node events
def test_simulator_cycles_cordoning(lib, oracle_lib):
    sim = S.from_fixture(FIXTURE)
    per_cycle = 90
    half = sim.workload.node_total[10] // 2 // 1000 * 1000
    events = [(1, "cordon", n) for n in range(4)] + [(2, "cut", n, half) for n in range(10, 15)] + [(2, "cordon", 20)] + \
             [(5, "uncordon", n) for n in (0, 1)] + [(5, "cut", 12, sim.workload.node_total[12])] + [(9, "uncordon", 20), (9, "cordon", 99)]
    a = S.run_cycles_cordoning(lib, sim, events, per_cycle=per_cycle)
    b = S.run_cycles_cordoning(lib, sim, events, per_cycle=per_cycle, nodes_patched=False)
    o = S.run_cycles_cordoning(oracle_lib, sim, events, per_cycle=per_cycle, nodes_patched=False, appended=False)
    plain = S.run_cycles_arriving(lib, sim, per_cycle=per_cycle)
    m = sim.workload.num_jobs
    assert a[-1]["rows"] == m and sum(len(c["scheduled"]) for c in a) - sum(len(c["preempted"]) for c in a) == m     # until the workload drains
    assert JA._records(a) == JA._records(b) == JA._records(o)
    assert JA._records(a) != JA._records(plain), "the node events changed no cycle: the case pins nothing"
    cordoned_then = {0, 1, 2, 3}
    assert not any(n in cordoned_then for c in a[1:5] for n in c["scheduled"].values())
