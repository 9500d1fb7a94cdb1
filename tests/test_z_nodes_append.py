"""asched_nodes_append: new rows join the resident node table between two scheduling cycles, on the device (armada_amd/csrc/kernels_nodes_append.h) — the library's
counterpart of populateNodeDb inserting the nodes the healthy executors report (scheduling_algo.go:1019-1098): a cluster that scales up, an executor that returns,
a drained node that is uncordoned.  The contract: after an append the handle is what nodes_upsert of "the resident rows in their order, then the new rows" would have
left; no resident position changes.  The oracle has no append: its side is always the grown table.

a. the NodeDb-level answers and a round against a fresh handle at the counts where the geometry takes another turn (the same word, a new word, a new stride, the
last value the rank field holds and the first it does not); b. the index order and the id ranks; c. 65 requirement classes, a table that iterates literally, a
handle without a job table; d. rounds against a fresh handle and the oracle: a run patched onto a new row, a new row that is unschedulable and over-allocated, the
returning node; e. interplay with jobs_patch, jobs_append, jobs_delete, nodes_patch, nodes_delete, nodes_upsert, the evictor report and the preemption causes;
f. the rebuild reasons; g. refusals; h. the simulator fixture with nodes that join; i. a library without the entry point.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library.

Rebuild reason 2 (a KNOWN node type newly populated) has no case: no sequence of public calls leaves a node type in the handle's list without a node — nodes_upsert
lists populated types only, and a nodes_patch or nodes_delete that empties a type goes through nodes_upsert's code, which rebuilds the list.  The branch is kept
because the list's invariant is not this call's to rely on."""
import copy
import ctypes as C

import numpy as np
import pytest

import scenario
import test_z_jobs_append as JA
import test_z_nodes_delete as ND
import test_z_nodes_patch as NP
from armada_amd import simulator_input as S
from armada_amd import workloads as W
from armada_amd.binding import CNodesAppend, SchedError, Scheduler
from test_z_nodes_delete import Table, lib  # noqa: F401  (the fixture: hostsim, and hip marked gpu)

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
FIXTURE = ND.FIXTURE
N = ND.N
NODE_FIELDS = ("total", "allocatable", "unschedulable", "over_allocated", "index")


def nodes_of(t, rows):
    """the table with node rows `rows` only, in that order (the job table as it is: no run may name a row that is left out)"""
    rows = np.asarray(rows, dtype=np.int64)
    h = copy.copy(t)
    for f in NODE_FIELDS:
        setattr(h, f, getattr(t, f)[rows].copy())
    h.labels = [t.labels[i] for i in rows]
    h.taints = [t.taints[i] for i in rows]
    return h


def split(t, n0):
    """(head, grown): the runs on rows >= n0 ended in both (a run on a new node is told after the append); head has the first n0 node rows, grown all of them"""
    g, _ = t.unbound(np.arange(n0, t.n))
    return nodes_of(g, np.arange(n0)), g


def append_rows(s, t, rows, **kw):
    rows = np.asarray(rows, dtype=np.int64)
    s.nodes_append(t.total[rows], t.allocatable[rows], index=t.index[rows], unschedulable=t.unschedulable[rows], over_allocated=t.over_allocated[rows],
                   taints=[t.taints[i] for i in rows], labels=[t.labels[i] for i in rows], **kw)


def _append_and_compare(lib, t, n0, what, step=1, oracle=None, **kw):
    head, grown = split(t, n0)
    s = head.handle(lib)
    append_rows(s, grown, np.arange(n0, t.n), **kw)
    st = s.nodes_append_stats()
    assert s.num_nodes == t.n == s.lib.num_nodes(s.h)
    assert st[0] == t.n - n0 and st[4] == t.n and st[5:] == [0, 0, 0], (st, what)
    assert st[1] == (1 if -(-t.n // 64) != -(-n0 // 64) else 0), (st, what)
    ND._compare(lib, s, grown, what, step, oracle=oracle)
    return s, grown, st


# ---------------------------------------------------------------- a. geometry
GEOMETRY = [(130, 0), (130, 1), (130, 2), (130, 62), (130, 63), (130, 64), (130, 65), (130, 126), (130, 127), (128, 1), (64, 1), (1, 129)]


@pytest.mark.parametrize("n0,m", GEOMETRY)
def test_answers_after_an_append_of_m_rows(lib, n0, m):
    t = Table(n=n0 + m)
    s, grown, st = _append_and_compare(lib, t, n0, (n0, m))
    if n0 == 130 and m <= 126:
        assert st[2:4] == [0, 0], ("the device path", st)              # 126: N1 = 256, the last value the 8-bit rank field holds
    if (n0, m) == (130, 127):
        assert st[2:4] == [1, 5], st                                   # N1 = 257: the rank field is too narrow
    s.close()


@pytest.fixture(scope="module")
def big_tables():
    return {m: Table(n=ND.NBIG + m, seed=5) for m in (1, 700)}


@pytest.mark.parametrize("m", [1, 700])
def test_answers_after_an_append_to_a_table_of_several_workgroups(lib, big_tables, m):
    s, grown, st = _append_and_compare(lib, big_tables[m], ND.NBIG, m, step=25)
    assert st[2:4] == [0, 0], st
    s.close()


def test_appends_one_after_the_other_and_nodes_upsert_in_between(lib):
    """every append finds what the one before it left; m == 0 performs the resets only; nodes_upsert puts the statistics back to zero"""
    t = Table(n=N + 70)
    g, _ = t.unbound(np.arange(N, t.n))
    n0 = N
    s = nodes_of(g, np.arange(n0)).handle(lib)
    for k, m in enumerate((2, 0, 63, 5)):
        s.round_prepare(np.ones(3), [[], [], []])
        append_rows(s, g, np.arange(n0, n0 + m))
        with pytest.raises(SchedError):
            s.schedule_round()                                         # round_prepare first, as after nodes_upsert
        n0 += m
        assert s.nodes_append_stats()[:5] == [m, 1 if k == 2 else 0, 0, 0, n0]
        ND._compare(lib, s, nodes_of(g, np.arange(n0)), k, step=5)
    g.upsert(s)
    g.set_jobs(s)
    assert s.nodes_append_stats() == [0] * 8
    ND._compare(lib, s, g, "after nodes_upsert", step=5)
    s.close()


# ---------------------------------------------------------------- b. the index order and the id ranks
def _reindexed(t, n0, kind):
    """the table with the node.index of rows >= n0 chosen against the resident ones"""
    t = copy.copy(t)
    t.index = t.index.copy()
    m = t.n - n0
    res = np.sort(t.index[:n0])
    if kind == "below":
        t.index[:n0] += np.uint64(10 * m)
        t.index[n0:] = np.arange(1, m + 1, dtype=np.uint64)
    elif kind == "above":
        t.index[n0:] = res[-1] + np.arange(1, m + 1, dtype=np.uint64)
    elif kind == "one gap":
        t.index[:n0] = t.index[:n0] * np.uint64(m + 1)
        lo = np.sort(t.index[:n0])[n0 // 2]
        t.index[n0:] = lo + np.arange(1, m + 1, dtype=np.uint64)
    elif kind == "descending":
        t.index[n0:] = np.sort(t.index[n0:])[::-1]
    return t


@pytest.mark.parametrize("kind", ["below", "above", "interleaved", "one gap", "descending"])
def test_index_order_after_an_append(lib, oracle_lib, kind):
    t = _reindexed(Table(n=N + 37), N, kind)
    assert len(set(t.index.tolist())) == t.n
    s, grown, st = _append_and_compare(lib, t, N, kind, oracle=oracle_lib)
    assert st[2:4] == [0, 0], st
    s.close()


class Ranked(Table):
    """the table with id ranks: node ids in index order (rank = twice the index rank, so a new row fits between two resident ones), where the packed keys serve a
    class that matches several node types"""

    def __init__(self, n):
        super().__init__(n=n)
        self.allocatable = self.total.copy()                           # (on the index grid)
        self.rank = (2 * np.argsort(np.argsort(self.index))).astype(np.int32)

    def upsert(self, s):
        s.nodes_upsert(self.total, self.allocatable, index=self.index, id_rank=self.rank, unschedulable=self.unschedulable, over_allocated=self.over_allocated,
                       taints=self.taints, labels=self.labels)


def _ranked_case(lib, mode):
    t = Ranked(N + 21)
    head, grown = split(t, N)
    head.rank, grown.rank = t.rank[:N].copy(), t.rank.copy()
    s = head.handle(lib)
    rows = np.arange(N, t.n)
    if mode == "between":
        append_rows(s, grown, rows, id_rank=t.rank[N:])
    elif mode == "all":
        grown.rank = np.argsort(np.argsort(t.index)).astype(np.int32)   # the caller re-ranked its id strings
        append_rows(s, grown, rows, id_rank_all=grown.rank)
    elif mode == "none":
        grown.rank = np.concatenate([t.rank[:N], t.rank[:N].max() + 1 + np.arange(t.n - N)]).astype(np.int32)
        append_rows(s, grown, rows)
    else:                                                              # one new row's id sorts before its index neighbours'
        grown.rank = t.rank.copy()
        grown.rank[N + 3] = -5
        append_rows(s, grown, rows, id_rank=grown.rank[N:])
    return s, grown


@pytest.mark.parametrize("mode", ["between", "all", "none", "breaks the order"])
def test_id_ranks_after_an_append(lib, oracle_lib, mode):
    s, grown = _ranked_case(lib, mode)
    st = s.nodes_append_stats()
    want = [1, 3] if mode in ("none", "breaks the order") else [0, 0]  # (ranks behind every resident one are not in index order either)
    assert st[2:4] == want, (mode, st)
    ND._compare(lib, s, grown, mode, oracle=oracle_lib)
    s.close()


class NoRanks(Table):
    """the table uploaded WITHOUT id ranks (asched_nodes.id_rank NULL, which the binding cannot express: it always sends the row order): id order is index order by
    definition, so the packed keys serve a class that matches several node types although the indices are not in row order"""

    def __init__(self, n):
        super().__init__(n=n)
        self.allocatable = self.total.copy()                           # (on the index grid)

    def upsert(self, s):
        from armada_amd.binding import CNodes, _csr
        n = self.n
        keep = [np.ascontiguousarray(self.total, np.int64), np.ascontiguousarray(self.allocatable, np.int64), np.ascontiguousarray(self.index, np.uint64),
                np.ascontiguousarray(self.unschedulable, np.uint8), np.ascontiguousarray(self.over_allocated, np.uint8)]
        toff, tcols = _csr(self.taints, 3)
        loff, lcols = _csr(self.labels, 2)
        c = CNodes()
        c.n = n
        p = lambda x, ct: x.ctypes.data_as(C.POINTER(ct))
        c.total, c.allocatable, c.index = p(keep[0], C.c_int64), p(keep[1], C.c_int64), p(keep[2], C.c_uint64)
        c.unschedulable, c.over_allocated = p(keep[3], C.c_uint8), p(keep[4], C.c_uint8)
        c.taint_off, c.taint_key, c.taint_value, c.taint_effect = (p(x, C.c_int32) for x in (toff, *tcols))
        c.label_off, c.label_key, c.label_value = (p(x, C.c_int32) for x in (loff, *lcols))
        s._check(s.lib.nodes_upsert(s.h, C.byref(c)))
        s.num_nodes = n


@pytest.mark.parametrize("mode", ["no ranks", "no ranks, rebuilt", "id_rank_all", "id_rank alone"])
def test_append_to_a_table_uploaded_without_id_ranks(lib, oracle_lib, mode):
    """such a table has no rank space: an append without ranks keeps "id order is index order" whatever the new indices (a fresh upload without ranks is the
    reference side), id_rank_all gives every row a rank (the reference side is uploaded with them), id_rank alone is refused with the handle as it was"""
    t = NoRanks(N + 21)
    if mode == "no ranks, rebuilt":
        t.labels = [list(x) for x in t.labels]
        t.labels[N + 1] = [(3, 9)]
    head, grown = split(t, N)
    s = head.handle(lib)
    rows = np.arange(N, t.n)
    if mode == "id_rank alone":
        want = ND.view(s, head, 5)
        with pytest.raises(SchedError) as e:
            append_rows(s, grown, rows, id_rank=np.arange(len(rows)))
        assert e.value.code == ERR_INVALID and s.lib.num_nodes(s.h) == N
        assert ND.view(s, head, 5) == want
        append_rows(s, grown, rows)                                    # and the handle still appends
        assert s.nodes_append_stats()[:5] == [21, 0, 0, 0, t.n]
    elif mode == "id_rank_all":
        r = Ranked(t.n)
        grown.__class__, grown.rank = Ranked, r.rank
        append_rows(s, grown, rows, id_rank_all=r.rank)
        assert s.nodes_append_stats()[:5] == [21, 0, 0, 0, t.n]
    else:
        append_rows(s, grown, rows)
        assert s.nodes_append_stats()[:5] == [21, 0, 0, 0, t.n] if mode == "no ranks" else s.nodes_append_stats()[:5] == [21, 0, 1, 4, t.n]
    # (the oracle only where ranks exist: without them it ties nodes by row order, the library by "id order is index order", on this table as on any fresh upload)
    ND._compare(lib, s, grown, mode, oracle=oracle_lib if mode == "id_rank_all" else None)
    s.close()


# ---------------------------------------------------------------- c. other tables
def test_answers_after_an_append_with_65_requirement_classes(lib):
    """more classes than a node's class word holds: no fast structure, two words of class bits per entry"""
    t = Table(n=N + 70, ncls=65)
    s, grown, st = _append_and_compare(lib, t, N, "65 classes")
    assert st[:4] == [70, 1, 0, 0], st
    s.close()


def _wl_split(wl, n0):
    """a workload's node table cut behind row n0, the runs on the rows behind it ended -> (head, grown, node state of grown)"""
    g, _ = ND._wl_unbound(wl, np.arange(n0, wl.num_nodes))
    state = ND._state(g)
    keep = np.arange(wl.num_nodes) < n0
    head, hstate, _ = ND._wl_reduced(g, state, np.nonzero(~keep)[0])
    return head, hstate, g, state


def _wl_append(s, wl, state, rows, **kw):
    rows = np.asarray(rows, dtype=np.int64)
    s.nodes_append(wl.node_total[rows], state["allocatable"][rows], index=rows + 1, unschedulable=state["unschedulable"][rows], over_allocated=state["over_allocated"][rows],
                   taints=None if wl.node_taints is None else [wl.node_taints[i] for i in rows], labels=None if wl.node_labels is None else [wl.node_labels[i] for i in rows], **kw)


def _wl_append_case(lib, oracle_lib, wl, n0, uni=False, device_path=True):
    """cycle 1 on the head table, then the rows join, and cycle 2 — against a fresh handle and the oracle given the grown table"""
    head, hstate, g, state = _wl_split(wl, n0)
    s = ND._load(lib, head, hstate, uni)
    r0, _ = NP._round(s, head)
    rows = np.arange(n0, wl.num_nodes)
    _wl_append(s, g, state, rows, **({} if wl.node_id_rank is None else dict(id_rank=np.asarray(wl.node_id_rank)[rows])))
    st = s.nodes_append_stats()
    assert st[0] == len(rows) and st[4] == wl.num_nodes and (st[2] == 0 or not device_path), st
    with pytest.raises(SchedError):
        s.schedule_round()
    r1, st1 = NP._round(s, g)
    f, o = ND._load(lib, g, state, uni), ND._load(oracle_lib, g, state, uni)
    rf, stf = NP._round(f, g)
    ro, _ = NP._round(o, g)
    scenario.assert_same_round(rf, r1)
    scenario.assert_same_round(ro, r1)
    assert st1["fast_iterations"] == stf["fast_iterations"]
    return s, f, o, g, state, r0, r1


def test_literal_iteration_after_an_append(lib, oracle_lib):
    """W.small_random(ragged=True): a class matching several populated types over unaligned allocatable, id_rank not monotone in index — the rows iterate literally"""
    wl = NP._round_wl("ragged")
    s, f, o, g, state, r0, r1 = _wl_append_case(lib, oracle_lib, wl, 100, device_path=False)
    for p in s.priorities:
        for req in ([4000, 8 * W.Gi, 0], [1000, W.Gi, 1]):
            assert s.iterate_nodes(p, req) == f.iterate_nodes(p, req) == o.iterate_nodes(p, req), p
    for x in (s, f, o):
        x.close()


def test_append_on_a_handle_without_a_job_table_then_jobs_set(lib):
    wl = NP._round_wl("offgrid")
    head, hstate, g, state = _wl_split(wl, 100)
    s = Scheduler(lib, wl.config)
    s.nodes_upsert(head.node_total, hstate["allocatable"], taints=head.node_taints, labels=head.node_labels, id_rank=head.node_id_rank)
    rows = np.arange(100, wl.num_nodes)
    _wl_append(s, g, state, rows, **({} if wl.node_id_rank is None else dict(id_rank=np.asarray(wl.node_id_rank)[rows])))
    assert s.nodes_append_stats()[0] == len(rows) and s.nodes_append_stats()[4] == wl.num_nodes
    assert s.total_resources().tolist() == g.node_total.sum(axis=0).tolist()
    W.set_jobs(s, g)
    r, _ = NP._round(s, g)
    f = ND._load(lib, g, state)
    rf, _ = NP._round(f, g)
    scenario.assert_same_round(rf, r)
    s.close(); f.close()


# ---------------------------------------------------------------- d. rounds against a fresh handle and the oracle
@pytest.mark.parametrize("kind", ["offgrid", "gangs with a uniformity label"])
def test_round_after_an_append(lib, oracle_lib, kind):
    uni = kind.startswith("gangs")
    wl = ND._gang_wl() if uni else NP._round_wl(kind)
    s, f, o, g, state, r0, r1 = _wl_append_case(lib, oracle_lib, wl, 97, uni=uni, device_path=False)
    assert NP._different(r0, r1)
    assert any(v >= 97 for v in r1.scheduled.values()), "nothing was placed on a new node"
    for x in (s, f, o):
        x.close()


def test_a_run_patched_onto_a_new_row_and_a_new_row_that_is_unschedulable_and_over_allocated(lib, oracle_lib):
    t = Table(n=N + 9)
    t.unschedulable, t.over_allocated = t.unschedulable.copy(), t.over_allocated.copy()
    t.unschedulable[N + 4] = t.over_allocated[N + 4] = 1               # (N + 4 is neither = 3 mod 7 nor = 0 mod 5: the type "unschedulable, untainted" is populated)
    on_new = np.nonzero(t.node >= N)[0].astype(np.int32)
    assert len(on_new) > 0
    head, grown = split(t, N)
    s = head.handle(lib)
    append_rows(s, grown, np.arange(N, t.n))
    assert s.nodes_append_stats()[:4] == [9, 0, 0, 0]
    ND._compare(lib, s, grown, "before the runs are told", oracle=oracle_lib)
    keep = on_new[t.node[on_new] != N + 4]
    s.jobs_patch(keep, t.node[keep], t.prio[keep], t.ts[keep])       # the runs on the new rows, told afterwards
    full = copy.copy(grown)
    full.node, full.prio, full.ts = grown.node.copy(), grown.prio.copy(), grown.ts.copy()
    full.node[keep], full.prio[keep], full.ts[keep] = t.node[keep], t.prio[keep], t.ts[keep]
    ND._compare(lib, s, full, "after jobs_patch onto the new rows", oracle=oracle_lib)
    s.close()


def test_the_returning_node(lib, oracle_lib):
    """rows 60..70 are deleted and join again with their old indices: the fresh side is the reduced table followed by those rows"""
    t = Table()
    rows = np.arange(60, 71)
    t2, jobs = t.unbound(rows)
    s = t.handle(lib)
    if len(jobs):
        s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
    s.nodes_delete(rows)
    assert s.nodes_delete_stats()[2] == 0
    append_rows(s, t2, rows)
    assert s.nodes_append_stats()[:5] == [11, 1, 0, 0, N]              # (119 rows had a stride of 128)
    t1, new_id = t2.reduced(rows)
    back = nodes_of(t2, np.concatenate([np.nonzero(new_id >= 0)[0], rows]))
    back.node = t1.node
    ND._compare(lib, s, back, "the returning nodes", oracle=oracle_lib)
    s.close()


# ---------------------------------------------------------------- e. interplay
ORDERS = ["jobs_patch, jobs_append, nodes_append, nodes_patch, jobs_delete",      # every other call before the append's neighbours; jobs_delete on the whole table
          "jobs_delete, nodes_append, nodes_patch, jobs_append, jobs_patch",      # jobs_delete of rows of the FIRST cycle's table before the append
          "nodes_append, jobs_delete, nodes_patch, jobs_append, jobs_patch"]      # ... and right behind it


@pytest.mark.parametrize("order", ORDERS)
def test_second_cycle_with_the_other_incremental_calls(lib, oracle_lib, order):
    """the calls run in exactly the order the id states.  jobs_delete renumbers the job rows: the calls behind it name rows by the map it returned, and a
    jobs_append behind it puts the tail at the ids that follow the reduced head"""
    wl = NP._round_wl("offgrid")
    n0 = 110
    cut, _ = ND._wl_unbound(wl, np.arange(n0, wl.num_nodes))           # no job runs on the rows that join later
    full, head, tail = JA._split(cut, "any")
    mh, mfull = head.num_jobs, full.num_jobs
    state = ND._state(full)
    keep = np.arange(wl.num_nodes) < n0
    hw, hstate, _ = ND._wl_reduced(head, state, np.nonzero(~keep)[0])
    a = ND._load(lib, hw, hstate)
    r1, _ = NP._round(a, hw)
    w2, jrows = JA._second_cycle(full, r1, 5)
    ids = np.arange(mfull)
    gone_jobs = np.nonzero((w2.job_node < 0) & (ids % 97 == 5) & (w2.job_gang < 0) & (ids < mh) & ~np.isin(ids, jrows))[0].astype(np.int32)   # rows of the head: queued in both cycles
    assert len(gone_jobs) >= 5
    rows = np.arange(n0, wl.num_nodes)
    last = wl.num_nodes - 1
    done = []
    jm = {"map": np.arange(mfull, dtype=np.int32)}                     # row of the whole second-cycle table -> row of the handle's table

    def jobs_delete():
        have = mfull if "jobs_append" in done else mh
        got = a.jobs_delete(jm["map"][gone_jobs], want_map=True)
        assert len(got) == have
        jm["map"] = np.concatenate([got, have - len(gone_jobs) + np.arange(mfull - have)]).astype(np.int32)   # (a tail still to come follows the reduced head)

    calls = {"jobs_patch": lambda: a.jobs_patch(jm["map"][jrows], w2.job_node[jrows], w2.job_run_prio[jrows], w2.job_run_ts[jrows]),
             "jobs_append": lambda: JA._append_tail(a, full, tail),
             "nodes_append": lambda: _wl_append(a, full, state, rows, **({} if wl.node_id_rank is None else dict(id_rank=np.asarray(wl.node_id_rank)[rows]))),
             "nodes_patch": lambda: a.nodes_patch([last, 1], unschedulable=1),       # the new last row and an old one
             "jobs_delete": jobs_delete}
    for name in order.split(", "):
        calls[name]()
        done.append(name)
    assert done == order.split(", ") and a.nodes_append_stats()[0] == len(rows) and a.num_jobs == mfull - len(gone_jobs)
    jmap = jm["map"]
    assert (jmap[gone_jobs] == -1).all() and sorted(jmap[jmap >= 0].tolist()) == list(range(mfull - len(gone_jobs)))
    st2 = ND._state(w2)
    st2["unschedulable"][[last, 1]] = 1
    ra, sta = ND._round_deleted(a, w2, jmap)
    f = ND._load(lib, w2, st2)
    f.jobs_delete(gone_jobs)
    rf, stf = ND._round_deleted(f, w2, jmap)
    o = ND._load_without_jobs(oracle_lib, w2, st2, jmap)
    ro, _ = NP._round(o[0], o[1])
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert sta["fast_iterations"] == stf["fast_iterations"]
    for x in (a, f, o[0]):
        x.close()


def test_append_then_nodes_delete_of_a_new_row_and_of_an_old_one_then_nodes_upsert(lib):
    t = Table(n=N + 20)
    head, grown = split(t, N)
    s = head.handle(lib)
    append_rows(s, grown, np.arange(N, t.n))
    rows = np.array([N + 5, 12], dtype=np.int32)                      # a new row and an old one, neither the last of its node type
    g2, jobs = grown.unbound(rows)
    if len(jobs):
        s.jobs_patch(jobs, np.full(len(jobs), -1, np.int32), 0, 0)
    s.nodes_delete(rows)
    assert s.nodes_delete_stats()[:3] == [2, int((g2.node > 12).sum()), 0]
    t1, _ = g2.reduced(rows)
    ND._compare(lib, s, t1, "after the delete")
    last = t1.n - 1
    s.nodes_patch([last], unschedulable=1 - int(t1.unschedulable[last]))
    p = copy.copy(t1)
    p.unschedulable = t1.unschedulable.copy()
    p.unschedulable[last] = 1 - t1.unschedulable[last]
    ND._compare(lib, s, p, "after the patch of the new last row")
    t.upsert(s)
    t.set_jobs(s)
    assert s.nodes_append_stats() == [0] * 8
    ND._compare(lib, s, t, "after nodes_upsert")
    s.close()


def test_evictor_report_and_preemption_causes_after_an_append(lib):
    wl = NP._round_wl("offgrid")
    head, hstate, g, state = _wl_split(wl, 100)
    state["unschedulable"][[7, 70, 120]] = 1
    hstate["unschedulable"][[7, 70]] = 1
    s = ND._load(lib, head, hstate)
    s.set_evictor_report(True)
    NP._round(s, head)
    rows = np.arange(100, wl.num_nodes)
    _wl_append(s, g, state, rows, **({} if wl.node_id_rank is None else dict(id_rank=np.asarray(wl.node_id_rank)[rows])))
    f = ND._load(lib, g, state)
    f.set_evictor_report(True)
    rs, _ = NP._round(s, g)
    rf, _ = NP._round(f, g)
    scenario.assert_same_round(rf, rs)
    es, ef = s.round_evictor_report(), f.round_evictor_report()
    assert es.keys() == ef.keys()
    for k in es:
        assert np.array_equal(np.asarray(es[k]), np.asarray(ef[k])), k
    assert len(es["node_reasons"]) == wl.num_nodes
    cs, cf = s.preemption_causes(), f.preemption_causes()
    assert cs.keys() == cf.keys()
    for k in cs:
        assert ND._plain(cs[k]) == ND._plain(cf[k]), k
    s.close(); f.close()


# ---------------------------------------------------------------- f. the rebuild reasons
def _rebuild_case(name):
    t = Table(n=N + 3 + 8)
    t.labels = [list(x) for x in t.labels]
    t.taints = [list(x) for x in t.taints]
    t.allocatable, t.total = t.allocatable.copy(), t.total.copy()
    if name == "an unseen node type":
        t.taints[N + 1] = [(7, 2, 1)]                                  # another value of the indexed taint
        return t, 1
    if name == "a new value of an indexed label":
        t.labels[N + 1] = [(3, 9)]
        return t, 4
    if name == "allocatable beyond the key layout":
        t.total[N + 1, W.MEM] = t.allocatable[N + 1, W.MEM] = 128 * W.Gi  # (twice what any resident node offers; on the index grid)
        return t, 3
    assert name == "allocatable off the index grid"
    t.allocatable = t.total.copy()                                     # (the resident rows on the grid ...)
    t.allocatable[N + 1, W.CPU] -= 137                                 # (... and one new row off it)
    return t, 3


@pytest.mark.parametrize("name", ["an unseen node type", "a new value of an indexed label", "allocatable beyond the key layout", "allocatable off the index grid"])
def test_rebuild_path(lib, oracle_lib, name):
    """reason 5 is pinned at its edge in a. (130 + 127), the id order of reason 3 in b.; reason 2 cannot be reached (the module's docstring)"""
    t, why = _rebuild_case(name)
    head, grown = split(t, N)
    s = head.handle(lib)
    append_rows(s, grown, np.arange(N, N + 3))
    assert s.nodes_append_stats() == [3, 0, 1, why, N + 3, 0, 0, 0]
    ND._compare(lib, s, nodes_of(grown, np.arange(N + 3)), name, oracle=oracle_lib)
    if why == 4:
        assert s.indexed_node_label_values(3) == [0, 1, 9]
    append_rows(s, grown, np.arange(N + 3, t.n))                       # a later device-path append still works
    assert s.nodes_append_stats() == [8, 0, 0, 0, t.n, 0, 0, 0]
    ND._compare(lib, s, grown, "a device-path append after the rebuild", oracle=oracle_lib)
    s.close()


# ---------------------------------------------------------------- g. refusals
def _raw(s, m, **arrays):
    """through the C structure: what the binding cannot express"""
    p = CNodesAppend()
    p.m = m
    keep = []
    types = dict(index=(np.uint64, C.c_uint64), total=(np.int64, C.c_int64), allocatable=(np.int64, C.c_int64))
    for name, v in arrays.items():
        dt, ct = types.get(name, (np.int32, C.c_int32))
        a = np.ascontiguousarray(v, dtype=dt)
        keep.append(a)
        setattr(p, name, a.ctypes.data_as(C.POINTER(ct)))
    return s.lib.nodes_append(s.h, C.byref(p))


def test_refusals_leave_the_handle_as_it_was(lib):
    t = Table(n=N + 2)
    head, grown = split(t, N)
    s, f = head.handle(lib), head.handle(lib)
    want = ND.view(f, head, 5)
    rwant = head.round(f)
    two = dict(index=grown.index[N:], total=grown.total[N:], allocatable=grown.allocatable[N:])
    z = np.zeros(8, np.int32)
    huge = np.array([[1 << 58, 1 << 58, 0, 1 << 58]], dtype=np.int64)
    bad = [(ERR_INVALID, lambda: _raw(s, -1, **two)),                                              # m < 0
           (ERR_INVALID, lambda: _raw(s, 2, total=two["total"], allocatable=two["allocatable"])),  # m > 0 without index
           (ERR_INVALID, lambda: _raw(s, 2, index=two["index"], allocatable=two["allocatable"])),  # ... without total
           (ERR_INVALID, lambda: _raw(s, 2, index=two["index"], total=two["total"])),              # ... without allocatable
           (ERR_INVALID, lambda: _raw(s, 2, index=[int(grown.index[N]), int(head.index[17])], total=two["total"], allocatable=two["allocatable"])),   # a resident row's index
           (ERR_INVALID, lambda: _raw(s, 2, index=[int(grown.index[N])] * 2, total=two["total"], allocatable=two["allocatable"])),                    # another new row's index
           (ERR_INVALID, lambda: _raw(s, 2, taint_off=[0, 2, 1], taint_key=z, taint_value=z, taint_effect=z, **two)),                                 # taint_off not ascending
           (ERR_INVALID, lambda: _raw(s, 2, label_off=[0, 2, 1], label_key=z, label_value=z, **two)),                                                 # label_off not ascending
           (ERR_UNSUPPORTED, lambda: _raw(s, (1 << 30) - N + 1, **two)),                                                                              # N + m above 2^30 (decided before any array is read)
           (ERR_UNSUPPORTED, lambda: _raw(s, 1, index=[int(grown.index[N])], total=huge, allocatable=huge))]                                          # the rebuild would refuse: a key beyond 128 bits
    for k, (code, call) in enumerate(bad):
        rc = call()
        msg = (s.lib.last_error(s.h) or b"").decode()
        assert rc == code and msg, (k, rc, code)
        assert s.lib.num_nodes(s.h) == N
        assert ND.view(s, head, 5) == want, k
    scenario.assert_same_round(rwant, head.round(s))
    append_rows(s, grown, np.arange(N, t.n))                                                       # and the handle still appends
    assert s.nodes_append_stats()[:5] == [2, 0, 0, 0, N + 2]
    ND._compare(lib, s, grown, "after the refusals")
    s.close(); f.close()


def test_refusal_of_what_the_rebuild_would_refuse_on_the_literal_path(lib):
    """tests/test_z_jobs_append.py ManyTypes: LIT_TMAX + 1 populated node types behind one requirement class, served by packed keys as long as allocatable is on the
    index grid; one new node off it would move the class to the literal iteration path, which serves at most LIT_TMAX types"""
    t = JA.ManyTypes()
    n = len(t.labels)
    s, f = t.handle(lib), t.handle(lib)
    want = t.view(f)
    off = t.node_total[[5]].copy()
    off[:, W.CPU] -= 137
    for _ in range(2):
        with pytest.raises(SchedError) as e:
            s.nodes_append(t.node_total[[5]], off, index=[n + 1], labels=[t.labels[5]])
        assert e.value.code == ERR_UNSUPPORTED and "LIT_TMAX" in str(e.value)
        assert s.lib.num_nodes(s.h) == n and t.view(s) == want
    on = t.node_total[[5]].copy()
    on[:, W.CPU] -= 2000
    s.nodes_append(t.node_total[[5]], on, index=[n + 1], labels=[t.labels[5]])
    assert s.nodes_append_stats()[:5] == [1, 0, 0, 0, n + 1]
    f.nodes_upsert(np.concatenate([t.node_total, t.node_total[[5]]]), np.concatenate([t.node_total, on]), labels=t.labels + [t.labels[5]])
    assert t.view(s) == t.view(f) and s.get_nodes_alloc().tolist() == f.get_nodes_alloc().tolist()
    s.close(); f.close()


def test_handles_nodes_append_does_not_serve(lib):
    wl = NP._refusal_wl()
    s = Scheduler(lib, wl.config)
    one = dict(index=[wl.num_nodes + 1])
    for m in (1, 0):
        with pytest.raises(SchedError) as e:
            s.nodes_append(wl.node_total[:m], **(one if m else dict(index=[])))                       # no node table
        assert e.value.code == ERR_INVALID
    W.set_jobs(s, wl)
    with pytest.raises(SchedError) as e:
        s.nodes_append(wl.node_total[:1], **one)
    assert e.value.code == ERR_INVALID
    for kw in (dict(alloc_by_prio=np.repeat(wl.node_total[:, None, :], s.P, axis=1)), dict(node_type_override=np.arange(wl.num_nodes) % 2)):
        s.nodes_upsert(wl.node_total, **kw)
        want, _ = NP._round(s, wl)
        for m in (1, 0):
            with pytest.raises(SchedError) as e:
                s.nodes_append(wl.node_total[:m], **(one if m else dict(index=[])))
            assert e.value.code == ERR_UNSUPPORTED
            got, _ = NP._round(s, wl)
            scenario.assert_same_round(want, got)
    s.nodes_upsert(wl.node_total)                                                                  # a plain table again
    s.nodes_append(wl.node_total[:0], index=[])
    assert s.nodes_append_stats() == [0, 0, 0, 0, wl.num_nodes, 0, 0, 0]
    s.close()


# ---------------------------------------------------------------- h. the simulator fixture with nodes that leave and join
def test_simulator_cycles_scaling(lib, oracle_lib):
    sim = S.from_fixture(FIXTURE)
    per_cycle = 90
    n = sim.workload.num_nodes
    absent = [n - 1, n - 2]                                            # not there at the start: n - 1 joins in cycle 2, n - 2 in cycle 5
    events = [(2, "join", n - 1), (5, "join", n - 2)] + [(1, "cordon", k) for k in range(4)] + [(1, "drop", k) for k in range(4)] + [(6, "join", 1), (8, "join", 3)] + \
             [(3, "cordon", 20), (4, "drop", 20), (9, "join", 20)]
    a = S.run_cycles_scaling(lib, sim, events, per_cycle=per_cycle, absent=absent)
    b = S.run_cycles_scaling_rebuilt(lib, sim, events, per_cycle=per_cycle, absent=absent)
    o = S.run_cycles_scaling_rebuilt(oracle_lib, sim, events, per_cycle=per_cycle, absent=absent)
    drained = S.run_cycles_scaling(lib, sim, [e for e in events if e[1] != "join"], per_cycle=per_cycle, absent=absent)
    m = sim.workload.num_jobs
    assert a[-1]["rows"] == m and sum(len(c["scheduled"]) for c in a) - sum(len(c["preempted"]) for c in a) == m     # until the workload drains
    assert JA._records(a) == JA._records(b) == JA._records(o)
    assert [c["nodes"] for c in a] == [c["nodes"] for c in b] == [c["nodes"] for c in o]
    assert a[0]["nodes"] == n - 2 and a[2]["nodes"] > a[1]["nodes"], [c["nodes"] for c in a]
    joined = sum(c.get("joined", 0) for c in a)
    assert joined == 4, joined                                         # two first-time nodes, and nodes 3 and 20 returning (node 1 never left: its join cancelled the drop)
    for v, k in ((3, 8), (20, 9)):                                     # cordoned, dropped, and placed on again from the cycle of the join on
        assert not any(v in c["scheduled"].values() for c in a[2:k]) and any(v in c["scheduled"].values() for c in a[k:]), v
    assert JA._records(a) != JA._records(drained), "the joining nodes changed no cycle: the case pins nothing"


# ---------------------------------------------------------------- i. a library without the entry point
def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = NP._refusal_wl()
    s = W.load(oracle_lib, wl)
    for call in (lambda: s.nodes_append(wl.node_total[:1], index=[wl.num_nodes + 1]), s.nodes_append_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    s.close()
