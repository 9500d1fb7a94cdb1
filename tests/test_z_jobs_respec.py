"""asched_jobs_respec: a retried job changes requirement class and request in place (armada_amd/csrc/kernels_jobs_respec.h) — the library's counterpart of the rewrite
of a requeued job's scheduling requirements (scheduler.go:1342-1383: node anti-affinity for every attempted run, the retry policy's memory bump).  The contract is the
one of the other resident calls: the handle is what jobs_set of the edited table would have left.

Every equivalence case asserts the expected `rebuilt`, new / revived shape counts and reason code — a silent fallback does not pass — and compares the handle with a
fresh handle of the edited table: scheduling_order, the first fit of every row at every priority level, the node types matching the named rows, a submit check with
units of the named rows, a round (also against the oracle's round), the unfeasible keys it left, the fair shares and the fast iterations.
a. batches and table ends; b. which field, no-ops, kinds of row; c. target and old shape, the source rule; d. request edges; e. the retry; f. fallbacks;
g. composition; h. cycles; i. refusals.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library, whose answers must also equal the CPU build's."""
import copy
import ctypes as C

import numpy as np
import pytest

import scenario
from armada_amd import simulator_input as S
from armada_amd import workloads as W
from armada_amd.binding import AFFINITY_OPS, SchedError, Scheduler
from test_z_jobs_append import FIXTURE, _append_tail, _records, _round
from test_z_jobs_append_shapes import SMAX, _after_round, _base, _edge_shapes, _extend, _view

ERR_INVALID, ERR_UNSUPPORTED, ERR_DEVICE = -1, -2, -3
Gi, CPU, MEM, EPH, GPU = W.Gi, W.CPU, W.MEM, W.EPH, W.GPU
NOT_IN = AFFINITY_OPS["NotIn"]
HOST = 77                                  # a label key that is not indexed: every node carries its number under it


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


# ---------------------------------------------------------------- the tables
def _load(L, wl, in_place=True):
    """W.load with the workload's class affinities, if it has any"""
    s = Scheduler(L, wl.config)
    s.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank)
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, submit_time=wl.job_submit, node=wl.job_node, scheduled_at_priority=wl.job_run_prio,
               run_timestamp=wl.job_run_ts, gang_id=wl.job_gang, gang_cardinality=wl.job_gang_card, req_class=wl.job_req_class,
               class_tolerations=wl.class_tolerations, class_selectors=wl.class_selectors, class_affinities=getattr(wl, "class_affinities", None), away=wl.job_away)
    if in_place:
        s.set_append_in_place(True)
    return s


def _requeue(wl):
    """the queued lists of a table whose run fields or queues were edited by hand"""
    w = copy.copy(wl)
    pcp = np.asarray(wl.config.pc_priority)[wl.job_pc]
    rows = np.nonzero((np.asarray(wl.job_node) < 0) & (np.asarray(wl.job_queue) >= 0))[0]
    w.queued = W._sort_queued(wl.job_queue, pcp, wl.job_submit, rows)
    while len(w.queued) < wl.num_queues:
        w.queued.append(np.zeros(0, np.int32))
    return w


def _queued_ends(base):
    """the base table with rows 0 and M - 1 queued single jobs"""
    w = copy.copy(base)
    w.job_node, w.job_run_prio, w.job_run_ts, w.job_gang, w.job_gang_card = (np.asarray(getattr(base, f)).copy() for f in ("job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card"))
    for j in (0, base.num_jobs - 1):
        w.job_node[j], w.job_run_prio[j], w.job_run_ts[j] = -1, 0, 0
        assert w.job_gang[j] < 0
    return _requeue(w)


def _edit(base, rows, cls=None, req=None):
    """the table jobs_set would be given: the named rows with their class and / or request replaced; the queued lists do not depend on either"""
    w = copy.copy(base)
    w.job_req, w.job_req_class = np.asarray(base.job_req).copy(), np.asarray(base.job_req_class).copy()
    rows = np.asarray(rows, dtype=np.int64)
    if cls is not None:
        w.job_req_class[rows] = cls
    if req is not None:
        w.job_req[rows] = np.asarray(req, dtype=np.int64)
    return w


def _free(wl):
    """queued single jobs of a queue: rows any case may name"""
    return np.nonzero((np.asarray(wl.job_node) < 0) & (np.asarray(wl.job_gang) < 0) & (np.asarray(wl.job_queue) >= 0))[0]


def _key(wl, j):
    return (int(wl.job_req_class[j]), int(wl.job_pc[j])) + tuple(int(x) for x in wl.job_req[j])


def _by_shape(wl):
    by = {}
    for j in range(wl.num_jobs):
        by.setdefault(_key(wl, j), []).append(j)
    return by


def _new_req(k, start=300):
    """k requests no base table has, each a fit shape of its own"""
    return np.array([[2 * Gi, 1000, (start + i) * Gi, 0] for i in range(k)], dtype=np.int64)


# ---------------------------------------------------------------- what a handle answers
def _answers(s, wl, rows):
    v = _view(s, wl, rows)
    r, st, u = _after_round(s, wl, rows)
    return v, r, st, u


def _same_as_fresh(lib, oracle_lib, cpu_lib, a, wl, rows, cpu=None):
    """handle `a` (edited in place) against a fresh handle of the edited table, the oracle's round and — on the HIP library — the CPU build's answers"""
    f = _load(lib, wl, in_place=False)
    va, ra, sta, ua = _answers(a, wl, rows)
    vf, rf, stf, uf = _answers(f, wl, rows)
    f.close()
    o = _load(oracle_lib, wl, in_place=False)
    ro, _ = _round(o, wl)
    o.close()
    assert va == vf
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert ua == uf
    assert ra.fair_share.tobytes() == rf.fair_share.tobytes() == ro.fair_share.tobytes()
    assert sta["fast_iterations"] == stf["fast_iterations"], "the edited handle did not run the fresh handle's fast iterations"
    if cpu is None and lib is not cpu_lib:
        c = _load(cpu_lib, wl, in_place=False)
        vc, rc, _, uc = _answers(c, wl, rows)
        c.close()
        cpu = (vc, rc, uc)
    if cpu is not None:
        assert va == cpu[0] and ua == cpu[2]
        scenario.assert_same_round(cpu[1], ra)
    return va, ra, ua


def _respec(s, rows, cls=None, req=None, **expect):
    s.jobs_respec(rows, cls, req)
    st = s.jobs_respec_stats()
    assert st["entries"] == len(rows), st
    for k, v in expect.items():
        assert st[k] == v, (k, v, st)
    return st


def _case(lib, oracle_lib, cpu_lib, base, rows, cls=None, req=None, warm=True, on=True, rebuilt=0, reason=0, **expect):
    """the whole comparison for one call.  warm: the handle ran a round on the base table first (fast structure, records and masks have been used)"""
    out = []
    w = _edit(base, rows, cls, req)
    expect.setdefault("new_shapes", len({_key(w, j) for j in rows} - set(_by_shape(base))))      # (a fresh handle of the base table holds no dead shape)
    for L in ([lib] if lib is cpu_lib else [cpu_lib, lib]):
        a = _load(L, base, in_place=False)
        a.set_append_in_place(on)
        if warm:
            _round(a, base)
        st = _respec(a, rows, cls, req, rebuilt=rebuilt, reason=reason, **expect)
        out.append(_same_as_fresh(L, oracle_lib, cpu_lib, a, w, rows, cpu=out[0] if out else None))
        a.close()
    return st


# ---------------------------------------------------------------- a. batches and table ends
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(lib, oracle_lib, hostsim_lib, n):
    """n entries onto five new shapes (every row its own request where n < 5)"""
    base = _base(65, n_jobs=600)
    rows = _free(base)[:n]
    assert len(rows) == n
    req = _new_req(5)[np.arange(n) % 5]
    st = _case(lib, oracle_lib, hostsim_lib, base, rows, None, req, unchanged=0)
    assert st["from_templates"] == n, st        # (no row of a new shape exists that no entry names)


def test_rows_zero_and_last(lib, oracle_lib, hostsim_lib):
    base = _queued_ends(_base(65))
    rows = np.array([base.num_jobs - 1, 0], dtype=np.int32)
    _case(lib, oracle_lib, hostsim_lib, base, rows, [2, 1], _new_req(2))


# ---------------------------------------------------------------- b. which field changes, no-ops, kinds of row
@pytest.mark.parametrize("what", ["class", "request", "both"])
def test_which_field_changes(lib, oracle_lib, hostsim_lib, what):
    base = _base(129)
    rows = np.array([j for j in _free(base) if base.job_req_class[j] == 0][:7], dtype=np.int32)
    cls = None if what == "request" else np.array([1, 2, 1, 2, 1, 2, 1], dtype=np.int32)       # class 1 selects the odd nodes, class 2 is class 0 under another id
    req = None if what == "class" else _new_req(7)
    _case(lib, oracle_lib, hostsim_lib, base, rows, cls, req)


def test_noop_entries(lib, oracle_lib, hostsim_lib):
    """entries that repeat the row's (class, request) mixed in — and a batch of nothing else, which changes nothing but the resets"""
    base = _base(65)
    rows = _free(base)[:12].astype(np.int32)
    cls, req = base.job_req_class[rows].copy(), base.job_req[rows].copy()
    req[::3] = _new_req(4)
    _case(lib, oracle_lib, hostsim_lib, base, rows, cls, req, unchanged=8)
    _case(lib, oracle_lib, hostsim_lib, base, rows, base.job_req_class[rows], base.job_req[rows], unchanged=12, new_shapes=0, revived=0, emptied=0, from_templates=0)
    _case(lib, oracle_lib, hostsim_lib, base, np.zeros(0, np.int32), None, None, unchanged=0, new_shapes=0)      # n == 0: the resets only


def test_a_gang_member_and_a_row_of_no_queue(lib, oracle_lib, hostsim_lib):
    base = _base(65)
    g = next(j for j in range(base.num_jobs) if base.job_gang[j] >= 0 and base.job_node[j] < 0)
    lone = int(_free(base)[3])
    w = copy.copy(base)
    w.job_queue = np.asarray(base.job_queue).copy()
    w.job_queue[lone] = -1                       # in the table, in no queue and no order
    w = _requeue(w)
    rows = np.array([g, lone], dtype=np.int32)
    _case(lib, oracle_lib, hostsim_lib, w, rows, None, [[1 * Gi, 1000, 1 * Gi, 0], [2 * Gi, 1000, 301 * Gi, 0]])


# ---------------------------------------------------------------- c. target shape, old shape, the source rule
def _two_shapes(base, same_pc=True):
    """two shapes of single queued jobs with at least two rows each (and the same priority class) -> their row lists"""
    by = [rows for rows in _by_shape(base).values() if len(rows) >= 2 and all(base.job_node[j] < 0 and base.job_gang[j] < 0 for j in rows)]
    for i, a in enumerate(by):
        for b in by[i + 1:]:
            if base.job_pc[a[0]] == base.job_pc[b[0]]:
                return a, b
    raise AssertionError("no two such shapes")


def test_target_resident_copies_a_resident_record(lib, oracle_lib, hostsim_lib):
    """a row joins a shape that has rows the call does not name: no template, no new shape"""
    base = _base(65)
    a, b = _two_shapes(base)
    _case(lib, oracle_lib, hostsim_lib, base, np.array([a[-1]], dtype=np.int32), base.job_req_class[b[0]], base.job_req[b[0]], new_shapes=0, revived=0, emptied=0, from_templates=0)


@pytest.mark.parametrize("which", ["one_of_many", "first", "last"])
def test_old_shape_loses_a_row(lib, oracle_lib, hostsim_lib, which):
    """the old shape loses one row of many, its FIRST row (the next row takes over as the shape's record source: pinned by a later call that copies from it), or its
    last row (it stays known without a row)"""
    base = _base(65)
    a, b = _two_shapes(base)
    rows = {"one_of_many": a[-1:], "first": a[:1], "last": a}[which]
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, base)
        _round(s, base)
        _respec(s, np.array(rows, dtype=np.int32), None, _new_req(1), rebuilt=0, reason=0, new_shapes=1, emptied=1 if which == "last" else 0)
        w = _edit(base, rows, None, _new_req(1))
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w, rows)
        # a row of shape b now joins shape a: its record comes from a's first REMAINING row, or — when none remains — the shape is revived through a template
        st = _respec(s, np.array([b[-1]], dtype=np.int32), base.job_req_class[a[0]], base.job_req[a[0]], rebuilt=0, reason=0, new_shapes=0, revived=1 if which == "last" else 0)
        assert st["from_templates"] == (1 if which == "last" else 0), st
        w = _edit(w, [b[-1]], base.job_req_class[a[0]], base.job_req[a[0]])
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w, list(rows) + [b[-1]])
        s.close()


def test_target_revived_after_jobs_delete(lib, oracle_lib, hostsim_lib):
    base = _base(65)
    a, b = _two_shapes(base)
    gone = np.array(a, dtype=np.int32)
    keep = np.array([j for j in range(base.num_jobs) if j not in set(a)], dtype=np.int64)
    red = copy.copy(base)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class"):
        setattr(red, f, np.asarray(getattr(base, f))[keep].copy())
    new_of = np.full(base.num_jobs, -1, np.int64)
    new_of[keep] = np.arange(len(keep))
    red.queued = [new_of[np.asarray([j for j in q if new_of[j] >= 0], dtype=np.int64)].astype(np.int32) for q in base.queued]
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, base)
        _round(s, base)
        s.jobs_delete(gone)
        assert s.jobs_delete_stats()["shapes_emptied"] == 1
        rows = new_of[b[:2]].astype(np.int32)
        _respec(s, rows, base.job_req_class[a[0]], base.job_req[a[0]], rebuilt=0, reason=0, new_shapes=0, revived=1, from_templates=2)
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, _edit(red, rows, base.job_req_class[a[0]], base.job_req[a[0]]), rows)
        s.close()


def test_source_rule_only_other_row_is_named_and_an_exchange(lib, oracle_lib, hostsim_lib):
    """the only row of the target shape is itself named in the call, and two rows that exchange shapes: no thread may read a record another entry writes — both come
    out right through templates"""
    base = _base(65)
    a, b = _two_shapes(base)
    # make shape X with exactly one row x; then ONE call moves x away and another row into X
    x, y = a[0], b[0]
    xreq = _new_req(1, 500)[0]
    s0 = _edit(base, [x], None, xreq)
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, s0)
        _round(s, s0)
        rows = np.array([y, x], dtype=np.int32)
        cls = np.array([s0.job_req_class[x], s0.job_req_class[x]], dtype=np.int32)
        req = np.array([xreq, _new_req(1, 501)[0]], dtype=np.int64)
        st = _respec(s, rows, cls, req, rebuilt=0, reason=0, new_shapes=1, revived=0)
        assert st["from_templates"] == 2, st
        w = _edit(s0, rows, cls, req)
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w, rows)
        # the exchange: the first rows of two shapes swap (class, request)
        p, q = a[1], b[1]
        p, q = min(j for j in range(w.num_jobs) if _key(w, j) == _key(w, p)), min(j for j in range(w.num_jobs) if _key(w, j) == _key(w, q))
        rows = np.array([p, q], dtype=np.int32)
        cls, req = w.job_req_class[[q, p]].copy(), w.job_req[[q, p]].copy()
        st = _respec(s, rows, cls, req, rebuilt=0, reason=0, new_shapes=0, revived=0, emptied=0)
        assert st["from_templates"] == 2, st
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, _edit(w, rows, cls, req), rows)
        s.close()


# ---------------------------------------------------------------- d. request edges
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_request_edges_at_the_mask_word_edges(lib, oracle_lib, hostsim_lib, n):
    """_edge_shapes: no node holds it; every node; only the other node type; a class that matches a strict subset; one resource / every resource equal to a node's total"""
    base = _base(n)
    sh = _edge_shapes()
    rows = np.array([j for j in _free(base) if base.job_pc[j] == 0][:len(sh)], dtype=np.int32)
    assert len(rows) == len(sh)
    st = _case(lib, oracle_lib, hostsim_lib, base, rows, [c for _, c in sh], [r for r, _ in sh], new_shapes=len(sh))
    s = _load(lib, _edit(base, rows, [c for _, c in sh], [r for r, _ in sh]))
    fit = s.fit_select_batch(rows)
    s.close()
    assert fit[0] < 0 and fit[1] == 0 and fit[2] == 1 and fit[3] == 1 and fit[4] == 0, fit


def test_on_grid_to_off_grid_and_back(lib, oracle_lib, hostsim_lib):
    """jAligned and the literal path follow the request.  The base table already has rows off the grid (its key layout does not change)"""
    base = W.small_random(n_nodes=130, n_jobs=240, n_queues=3, seed=35, occupied=0.5, gangs=2, offgrid=1)
    base.job_req_class = np.zeros(base.num_jobs, np.int32)
    on = np.array([j for j in _free(base) if (base.job_req[j, CPU] % 1000 == 0)][:3], dtype=np.int32)
    off = [[4 * Gi, 2125, 7 * Gi, 0], [4 * Gi + 1000, 2000, 7 * Gi, 0], [4 * Gi, 2125, 7 * Gi, 0]]
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, base)
        _round(s, base)
        _respec(s, on, None, off, rebuilt=0, reason=0, new_shapes=len({(int(base.job_pc[j]),) + tuple(r) for j, r in zip(on, off)}))
        w = _edit(base, on, None, off)
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w, on)
        _respec(s, on, None, base.job_req[on], rebuilt=0, reason=0, new_shapes=0)            # and back
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, base, on)
        s.close()


# ---------------------------------------------------------------- e. the retry itself
def test_retry_with_anti_affinity_avoids_the_node(lib, oracle_lib, hostsim_lib):
    """req_classes_append of a class whose affinity excludes the one node the row would otherwise get, then respec: first fit and round avoid that node, as on the
    fresh handle and the oracle"""
    base = _base(65)
    base.node_labels = [list(l) + [(HOST, 1000 + i)] for i, l in enumerate(base.node_labels)]
    base.class_affinities = None
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, base)
        r0, _ = _round(s, base)
        j, n = next((j, n) for j, n in sorted(r0.scheduled.items()) if base.job_gang[j] < 0 and base.job_node[j] < 0)     # the job ran on n and failed
        c0 = len(base.class_tolerations)
        first = s.req_classes_append([[]], selectors=[list(base.class_selectors[base.job_req_class[j]])], affinities=[[[(HOST, NOT_IN, [1000 + n])]]])
        assert first == c0
        rows = np.array([j], dtype=np.int32)
        bumped = base.job_req[j].copy()
        bumped[MEM] += bumped[MEM] // 2
        _respec(s, rows, first, bumped, rebuilt=0, reason=0, new_shapes=1)
        w = _edit(base, rows, first, bumped)
        w.class_tolerations = list(base.class_tolerations) + [[]]
        w.class_selectors = list(base.class_selectors) + [list(base.class_selectors[base.job_req_class[j]])]
        w.class_affinities = [None] * c0 + [[[(HOST, NOT_IN, [1000 + n])]]]
        assert s.fit_select_batch(rows)[0] != n
        _, ra, _ = _same_as_fresh(L, oracle_lib, hostsim_lib, s, w, rows)
        assert ra.scheduled.get(j, -1) != n
        s.close()


# ---------------------------------------------------------------- f. fallbacks: same result, and the statistics say so
def test_fallback_switch_off(lib, oracle_lib, hostsim_lib):
    base = _base(65)
    rows = _free(base)[:3].astype(np.int32)
    _case(lib, oracle_lib, hostsim_lib, base, rows, None, _new_req(3), on=False, rebuilt=1, reason=0)
    a, b = _two_shapes(base)                     # a resident target needs no rebuild, switch or no switch
    _case(lib, oracle_lib, hostsim_lib, base, np.array(a[-1:], dtype=np.int32), base.job_req_class[b[0]], base.job_req[b[0]], on=False, rebuilt=0, reason=0, new_shapes=0)


def test_fallback_key_layout_changes(lib, oracle_lib, hostsim_lib):
    """a negative request on an indexed column: the edited table needs the wide field layout"""
    base = _base(65)
    _case(lib, oracle_lib, hostsim_lib, base, _free(base)[:2].astype(np.int32), None, [[4 * Gi, -1000, 7 * Gi, 0]] * 2, rebuilt=1, reason=2)


def test_fallback_negative_request_off_the_index(lib, oracle_lib, hostsim_lib):
    base = _base(65)
    _case(lib, oracle_lib, hostsim_lib, base, _free(base)[:2].astype(np.int32), None, [[2 * Gi, 1000, -1 * Gi, 0]] * 2, rebuilt=1, reason=5)


def test_fallback_fit_shapes_over_smax(lib, oracle_lib, hostsim_lib):
    base = _base(65, n_jobs=600)
    rows = _free(base)[:SMAX + 1].astype(np.int32)
    assert len(rows) == SMAX + 1
    _case(lib, oracle_lib, hostsim_lib, base, rows, None, _new_req(SMAX + 1), rebuilt=1, reason=4)


# ---------------------------------------------------------------- g. composition: no jobs_set in between
def _drop(wl, gone):
    keep = np.array([j for j in range(wl.num_jobs) if j not in set(int(x) for x in gone)], dtype=np.int64)
    red = copy.copy(wl)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class"):
        setattr(red, f, np.asarray(getattr(wl, f))[keep].copy())
    new_of = np.full(wl.num_jobs, -1, np.int64)
    new_of[keep] = np.arange(len(keep))
    red.queued = [new_of[np.asarray([j for j in q if new_of[j] >= 0], dtype=np.int64)].astype(np.int32) for q in wl.queued]
    return red, new_of


def test_composition_with_the_other_resident_calls(lib, oracle_lib, hostsim_lib):
    base = _base(130)
    a, b = _two_shapes(base)
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, base)
        _round(s, base)
        # a new class that only the respec'd rows name, then the respec: shape a is left without a row
        c_new = s.req_classes_append([[]], selectors=[[(3, 0)]])
        rows = np.array(a, dtype=np.int32)
        _respec(s, rows, c_new, _new_req(1, 600), rebuilt=0, reason=0, new_shapes=1, emptied=1)
        w = _edit(base, rows, c_new, _new_req(1, 600))
        w.class_tolerations, w.class_selectors = list(base.class_tolerations) + [[]], list(base.class_selectors) + [[(3, 0)]]
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w, rows)
        # jobs_append of the OLD shape (revived) and of the new one
        old_req, old_cls, pc = base.job_req[a[0]], int(base.job_req_class[a[0]]), int(base.job_pc[a[0]])
        w2, tail = _extend(w, [old_req, _new_req(1, 600)[0]], pc=pc, cls=[old_cls, c_new])
        st = _append_tail(s, w2, tail)
        assert st["rebuilt"] == 0 and st["in_place"] == 1, st
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w2, np.concatenate([rows, tail]))
        # nodes_patch in between, then a respec back onto a resident shape
        nrows = np.array([0, 63, 64, 65, 129], dtype=np.int32)
        alloc = w2.node_total[nrows].copy()
        alloc[:, CPU] -= 2000
        s.nodes_patch(nrows, allocatable=alloc)
        w3 = copy.copy(w2)
        w3.node_allocatable = w2.node_total.copy()
        w3.node_allocatable[nrows] = alloc
        _respec(s, rows[:1], old_cls, old_req, rebuilt=0, reason=0, new_shapes=0, revived=0, from_templates=0)
        w3 = _edit(w3, rows[:1], old_cls, old_req)
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w3, np.concatenate([rows, tail]))
        # jobs_delete of every row that names the new class; shapes_compact retires the emptied shape and the abandoned class, and the class map is applied
        gone = np.array([j for j in range(w3.num_jobs) if w3.job_req_class[j] == c_new], dtype=np.int32)
        s.jobs_delete(gone)
        w4, new_of = _drop(w3, gone)
        cmap = s.shapes_compact(classes=True, want_map=True)
        sc = s.shapes_compact_stats()
        assert sc["shapes_retired"] >= 1 and sc["classes_retired"] == 1 and cmap[c_new] == -1, sc
        w4.class_tolerations, w4.class_selectors = list(base.class_tolerations), list(base.class_selectors)
        named = new_of[[int(rows[0]), int(tail[0])]]
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w4, named)
        # jobs_patch gives the respec'd row a run; jobs_reprioritise; then a respec of another row on the compacted handle
        j = int(named[0])
        w5 = copy.copy(w4)
        w5.job_node, w5.job_run_prio, w5.job_run_ts = w4.job_node.copy(), w4.job_run_prio.copy(), w4.job_run_ts.copy()
        w5.job_node[j], w5.job_run_prio[j], w5.job_run_ts[j] = 1, int(np.asarray(w4.config.pc_priority)[w4.job_pc[j]]), int(w4.job_run_ts.max()) + 1
        w5 = _requeue(w5)
        s.jobs_patch([j], [1], [w5.job_run_prio[j]], [w5.job_run_ts[j]])
        s.jobs_reprioritise([int(named[1])], 0)
        with pytest.raises(SchedError) as e:         # the row runs now: refused
            s.jobs_respec([j], None, _new_req(1))
        assert e.value.code == ERR_INVALID
        k = int(new_of[b[0]])
        _respec(s, [k], None, _new_req(1, 700), rebuilt=0, reason=0, new_shapes=1)
        w5 = _edit(w5, [k], None, _new_req(1, 700))
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w5, [j, k])
        s.close()


@pytest.mark.parametrize("what", ["append", "delete"])
def test_node_table_changes_after_a_respec(lib, oracle_lib, hostsim_lib, what):
    base = _base(130)
    rows = _free(base)[:6].astype(np.int32)
    req = _new_req(3)[np.arange(6) % 3]
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, base)
        _respec(s, rows, [1, 0, 2, 1, 0, 2], req, rebuilt=0, reason=0)
        w = _edit(base, rows, [1, 0, 2, 1, 0, 2], req)
        n = base.num_nodes
        w.node_taints = [[] for _ in range(n)] if w.node_taints is None else w.node_taints
        if what == "append":
            src = np.array([0, 1, 64, 65, 3], dtype=np.int64)
            s.nodes_append(w.node_total[src], index=n + 1 + np.arange(len(src)), taints=[w.node_taints[i] for i in src], labels=[w.node_labels[i] for i in src])
            assert s.nodes_append_stats()[2] == 0
            w.node_total = np.concatenate([w.node_total, w.node_total[src]])
            w.node_taints = list(w.node_taints) + [w.node_taints[i] for i in src]
            w.node_labels = list(w.node_labels) + [w.node_labels[i] for i in src]
        else:
            busy = set(np.asarray(w.job_node).tolist())
            gone = np.array([i for i in range(n) if i not in busy][:3], dtype=np.int32)
            s.nodes_delete(gone)
            assert s.nodes_delete_stats()[2] == 0
            keep = np.array([i for i in range(n) if i not in set(gone.tolist())])
            new_of = np.full(n, -1, np.int64)
            new_of[keep] = np.arange(len(keep))
            w.node_total = w.node_total[keep]
            w.node_taints = [w.node_taints[i] for i in keep]
            w.node_labels = [w.node_labels[i] for i in keep]
            w.job_node = np.where(w.job_node >= 0, new_of[np.maximum(w.job_node, 0)], -1).astype(np.int32)
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w, rows)
        s.close()


def test_queries_after_a_round_then_respec(lib, hostsim_lib):
    """a round, then respec: the queries answer as on a fresh handle (the call resets what the round left)"""
    base = _base(65)
    rows = _free(base)[:4].astype(np.int32)
    s = _load(lib, base)
    _round(s, base)
    _respec(s, rows, 1, _new_req(4), rebuilt=0, reason=0)
    w = _edit(base, rows, 1, _new_req(4))
    for L in {lib, hostsim_lib}:
        f = _load(L, w)
        assert _view(s, w, rows) == _view(f, w, rows)
        assert [s.job_key_unfeasible(int(j)) for j in rows] == [f.job_key_unfeasible(int(j)) for j in rows]
        f.close()
    s.close()


# ---------------------------------------------------------------- h. cycles
def test_two_cycles_against_a_fresh_handle_and_the_oracle(lib, oracle_lib, hostsim_lib):
    """cycle 1 leases jobs; three of them fail: jobs_patch ends their runs and the others', respec requeues the failed ones with more memory and another class; cycle 2"""
    base = _base(65)
    for L in ([lib] if lib is hostsim_lib else [hostsim_lib, lib]):
        s = _load(L, base)
        r1, _ = _round(s, base)
        w2 = copy.copy(base)
        w2.job_node, w2.job_run_prio, w2.job_run_ts = base.job_node.copy(), base.job_run_prio.copy(), base.job_run_ts.copy()
        ts = int(base.job_run_ts.max()) + 1_000_000_000
        leased = [j for j in sorted(r1.scheduled) if base.job_gang[j] < 0 and base.job_node[j] < 0]
        failed = np.array(leased[:3], dtype=np.int32)
        assert len(failed) == 3
        touched = []
        for j, n in r1.scheduled.items():
            if j not in set(failed.tolist()) and base.job_node[j] < 0:
                w2.job_node[j], w2.job_run_prio[j], w2.job_run_ts[j] = n, r1.scheduled_priority[j], ts
                touched.append(j)
        for j in r1.preempted:
            w2.job_node[j], w2.job_run_prio[j], w2.job_run_ts[j] = -1, 0, 0
            touched.append(j)
        touched = np.array(sorted(set(touched)), dtype=np.int32)
        s.jobs_patch(touched, w2.job_node[touched], w2.job_run_prio[touched], w2.job_run_ts[touched])
        req = base.job_req[failed].copy()
        req[:, MEM] += req[:, MEM] // 2
        _respec(s, failed, 2, req, rebuilt=0, reason=0)
        w2 = _requeue(_edit(w2, failed, 2, req))
        _same_as_fresh(L, oracle_lib, hostsim_lib, s, w2, failed)
        s.close()


def test_simulator_cycles_retrying_equal_rebuilt(lib, oracle_lib):
    sim = S.from_fixture(FIXTURE)
    kw = dict(per_cycle=90, fail_share=0.15, bump_share=0.5, seed=5)
    a = S.run_cycles_retrying(lib, sim, **kw)
    b = S.run_cycles_retrying_rebuilt(lib, sim, **kw)
    o = S.run_cycles_retrying_rebuilt(oracle_lib, sim, **kw)
    assert _records(a) == _records(b) == _records(o)
    assert a[-1]["rows"] == sim.workload.num_jobs and a[-1]["retried"] == b[-1]["retried"] > 10 and 0 < a[-1]["bumped"] < a[-1]["retried"] and a[-1]["classes"] > 5, a[-1]
    assert sum(len(c["scheduled"]) for c in a) == sim.workload.num_jobs + a[-1]["retried"]        # until the workload drains: every failed run was leased again
    assert a[-1]["respecs_rebuilt"] == 0, a[-1]


# ---------------------------------------------------------------- i. refusals: the handle is as it was
def test_refusals(lib, hostsim_lib):
    base = _base(65, away=True)
    run = next(j for j in range(base.num_jobs) if base.job_node[j] >= 0)
    free = _free(base).astype(np.int32)
    s = _load(lib, base)
    _respec(s, free[:2], None, _new_req(2), rebuilt=0, reason=0, new_shapes=2)
    w = _edit(base, free[:2], None, _new_req(2))
    stats, before = s.jobs_respec_stats(), _view(s, w, free[:4])
    i32 = np.zeros(4, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    i64 = np.zeros(4 * W.R, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    raw = [(-1, i32, i32, i64), (2, None, i32, i64), (2, i32, None, None), ((1 << 29) + 1, i32, i32, i64)]
    for (n, jb, rc, rq), code in zip(raw, [ERR_INVALID, ERR_INVALID, ERR_INVALID, ERR_UNSUPPORTED]):
        assert s.lib.jobs_respec(s.h, n, jb, rc, rq) == code
    calls = [(([base.num_jobs], None, _new_req(1)), ERR_INVALID),               # a row outside [0, M)
             (([-1], None, _new_req(1)), ERR_INVALID),
             (([int(free[5]), int(free[6]), int(free[5])], None, _new_req(3)), ERR_INVALID),      # a row named twice
             (([int(free[5])], 3, None), ERR_INVALID),                          # a class out of range
             (([int(free[5])], -1, None), ERR_INVALID),
             (([int(free[5]), run], None, _new_req(2)), ERR_INVALID)]           # a row that has a run
    for args, code in calls:
        with pytest.raises(SchedError) as e:
            s.jobs_respec(*args)
        assert e.value.code == code, (args, str(e.value))
        assert s.jobs_respec_stats() == stats
    assert _view(s, w, free[:4]) == before
    _respec(s, free[5:7], None, _new_req(2), rebuilt=0, reason=0)     # and the handle still takes the call
    w = _edit(w, free[5:7], None, _new_req(2))
    vs = _view(s, w, free[:8])
    rs, _ = _round(s, w)
    for L in {lib, hostsim_lib}:
        f = _load(L, w)
        assert vs == _view(f, w, free[:8])
        rf, _ = _round(f, w)
        scenario.assert_same_round(rf, rs)
        f.close()
    s.close()
    # no job table
    s = Scheduler(lib, base.config)
    with pytest.raises(SchedError) as e:
        s.jobs_respec([0], None, _new_req(1))
    assert e.value.code == ERR_INVALID
    s.close()


def test_refusal_of_an_away_row_and_of_a_market_job_set(lib):
    base = _base(65, away=True)
    w = copy.copy(base)
    away = np.zeros(base.num_jobs, np.uint8)
    j = int(_free(base)[0])
    away[j] = 1
    w.job_away = away
    s = _load(lib, w)
    with pytest.raises(SchedError) as e:
        s.jobs_respec([j], None, _new_req(1))
    assert e.value.code == ERR_UNSUPPORTED and "away" in str(e.value)
    s.jobs_respec([int(_free(base)[1])], None, _new_req(1))
    s.close()
    s = Scheduler(lib, base.config)
    s.nodes_upsert(base.node_total, base.node_allocatable, taints=base.node_taints, labels=base.node_labels, id_rank=base.node_id_rank)
    W.set_jobs(s, base, bid_price=np.ones(base.num_jobs))
    with pytest.raises(SchedError) as e:
        s.jobs_respec([j], None, _new_req(1))
    assert e.value.code == ERR_UNSUPPORTED and "market" in str(e.value)
    s.close()


def test_refusal_by_the_rebuild_leaves_the_handle_as_it_was(lib, hostsim_lib):
    """test_z_jobs_append's table of LIT_TMAX + 1 node types: a request off the grid whose class matches them all is refused after the shape lookup, and everything
    the in-place path had looked at is put back"""
    from test_z_jobs_append import ManyTypes
    t = ManyTypes()
    s = t.handle(lib)
    s.set_append_in_place(True)
    before = t.view(s)
    for _ in range(2):
        with pytest.raises(SchedError) as e:
            s.jobs_respec([3, 4], None, [[W.Gi, 3000, 0, 0], [W.Gi, 1500, 0, 0]])
        assert e.value.code == ERR_UNSUPPORTED and "LIT_TMAX" in str(e.value)
        assert t.view(s) == before and s.jobs_respec_stats()["entries"] == 0
    s.jobs_respec([3, 4], None, [[W.Gi, 3000, 0, 0], [W.Gi, 5000, 0, 0]])
    assert s.jobs_respec_stats()["rebuilt"] == 0 and s.jobs_respec_stats()["new_shapes"] >= 1
    s.close()


def test_out_of_device_memory_leaves_the_handle_as_it_was(hostsim_lib):
    """the CPU build's allocation hook (tests/test_z_resident_out_of_memory.py): the k-th device allocation of the call fails, for every k the call makes"""
    import test_z_resident_out_of_memory as oom
    base = _base(65)
    rows = _free(base)[:3].astype(np.int32)
    s = _load(hostsim_lib, base)
    before = _view(s, base, rows)
    s.set_append_in_place(True)
    arm, seen = oom._hook(hostsim_lib)
    refused, done = 0, False
    for k in range(40):
        arm(k)
        try:
            s.jobs_respec(rows, 1, _new_req(3))
            made, err = seen(), None
        except SchedError as e:
            made, err = seen(), e
        finally:
            arm(-1)
        if made <= k:                # the hook did not fire: the call went through
            assert err is None, err
            done = True
            break
        assert err is not None and err.code == ERR_DEVICE and "the handle is as it was" in str(err), (k, err)
        refused += 1
        assert _view(s, base, rows) == before and s.jobs_respec_stats()["entries"] == 0
    assert done and refused >= 3, refused        # the scratch, and a first and a last staged block
    assert s.jobs_respec_stats()["rebuilt"] == 0 and s.jobs_respec_stats()["new_shapes"] == 3
    w = _edit(base, rows, 1, _new_req(3))
    f = _load(hostsim_lib, w)
    assert _view(s, w, rows) == _view(f, w, rows)
    f.close(); s.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = _base(20, n_jobs=60)
    o = W.load(oracle_lib, wl)
    for call in (lambda: o.jobs_respec([0], None, _new_req(1)), o.jobs_respec_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    o.close()
