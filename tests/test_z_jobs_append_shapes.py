"""asched_set_append_in_place: an asched_jobs_append whose rows bring NEW scheduling-key shapes (or shapes asched_jobs_delete left without a resident row) grows the
shape-dependent tables by what those shapes add — mask rows on the device (armada_amd/csrc/kernels_shapes_append.h), perhaps a derived away class and a fit shape, the
two minima of the fast structure, one record template per shape — instead of re-deriving them for every shape.  The contract is jobs_append's: the handle is what
jobs_set of the concatenated table would have left.

Every equivalence case asserts rebuilt == 0, in_place == the expected count and reason code 0 — a silent fallback does not pass for the new path — and compares the handle
with a fresh handle given the concatenated table: scheduling_order, the first fit of every row at every priority level, a submit check with units of the new shapes, the
node types matching the new rows, a round (also against the oracle's round) and the unfeasible keys the round left for the new rows.
a. mask edges; b. away rows; c. records and fit shapes; d. interplay; e. fallbacks; f. refusals; g. the switch off; h. the simulator fixture.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library, whose answers must also equal the CPU build's."""
import copy
import os

import numpy as np
import pytest

import scenario
from armada_amd import simulator_input as S
from armada_amd import workloads as W
from armada_amd.binding import SchedError, Scheduler
from test_z_jobs_append import FIXTURE, ManyTypes, _append_tail, _records, _round

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
SMAX = 256                                 # armada_amd/csrc/dev.h: fit shapes with a cached base candidate
Gi, CPU, MEM, EPH, GPU = W.Gi, W.CPU, W.MEM, W.EPH, W.GPU


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


# ---------------------------------------------------------------- the tables
def _base(n_nodes, n_jobs=240, seed=31, away=False, offgrid=0, occupied=0.5):
    """W.small_random with two node types (an indexed label; the odd nodes have twice the memory) and three requirement classes: class 1 selects the odd nodes, class 2
    is class 0 again and only ever has rows of priority class 0 (so no derived away class of it exists in the base table)"""
    wl = W.small_random(n_nodes=n_nodes, n_jobs=n_jobs, n_queues=3, seed=seed, occupied=occupied, gangs=2, away=away, offgrid=offgrid)
    wl.config.indexed_label_keys = [3]
    wl.node_labels = [[(3, i % 2)] for i in range(n_nodes)]
    wl.node_total = wl.node_total.copy()
    wl.node_total[1::2, MEM] = 128 * Gi
    rng = np.random.default_rng(seed)
    cls = rng.choice(3, size=wl.num_jobs, p=[0.6, 0.25, 0.15]).astype(np.int32)
    cls[np.asarray(wl.job_node) >= 0] = 0                      # (a running job of class 1 on an even node would not be a valid table)
    cls[np.asarray(wl.job_gang) >= 0] = 0                      # (gang members share one shape)
    cls[(cls == 2) & (np.asarray(wl.job_pc) != 0)] = 0
    wl.job_req_class = cls
    wl.class_tolerations = [[], [], []]
    wl.class_selectors = [[], [(3, 1)], []]
    return wl


def _extend(base, req, pc=None, cls=None, queue=None, gang=None, card=None):
    """the table jobs_set would be given: the base rows, then the new rows as queued jobs, and the queued lists in SchedulingOrderCompare order"""
    req = np.asarray(req, dtype=np.int64).reshape(-1, base.job_req.shape[1])
    m, m0 = len(req), base.num_jobs
    pick = lambda v, d: np.full(m, d, np.int32) if v is None else np.broadcast_to(np.asarray(v, dtype=np.int32), (m,)).copy()
    w = copy.copy(base)
    w.job_req = np.concatenate([base.job_req, req])
    w.job_pc = np.concatenate([base.job_pc, pick(pc, 0)]).astype(np.int32)
    w.job_req_class = np.concatenate([base.job_req_class if base.job_req_class is not None else np.zeros(m0, np.int32), pick(cls, 0)]).astype(np.int32)
    w.job_queue = np.concatenate([base.job_queue, pick(queue, 0) if queue is not None else (np.arange(m) % base.num_queues).astype(np.int32)]).astype(np.int32)
    w.job_submit = np.concatenate([base.job_submit, m0 + np.arange(m, dtype=np.int64)])
    w.job_node = np.concatenate([base.job_node, np.full(m, -1, np.int32)]).astype(np.int32)
    w.job_run_prio = np.concatenate([base.job_run_prio, np.zeros(m, np.int32)]).astype(np.int32)
    w.job_run_ts = np.concatenate([base.job_run_ts, np.zeros(m, np.int64)])
    w.job_gang = np.concatenate([base.job_gang, pick(gang, -1)]).astype(np.int32)
    w.job_gang_card = np.concatenate([base.job_gang_card, pick(card, 1)]).astype(np.int32)
    if base.job_req_class is None:
        w.job_req_class = None if cls is None else w.job_req_class
    pcp = np.asarray(base.config.pc_priority)[w.job_pc]
    w.queued = W._sort_queued(w.job_queue, pcp, w.job_submit, np.nonzero(w.job_node < 0)[0])
    while len(w.queued) < base.num_queues:
        w.queued.append(np.zeros(0, np.int32))
    return w, np.arange(m0, m0 + m)


def _shape_count(wl, rows=None):
    rows = range(wl.num_jobs) if rows is None else rows
    cls = np.zeros(wl.num_jobs, np.int64) if wl.job_req_class is None else wl.job_req_class
    return len({(int(cls[j]), int(wl.job_pc[j])) + tuple(int(x) for x in wl.job_req[j]) for j in rows})


def _edge_shapes():
    """(request, requirement class): no node holds it; every node holds it; only the odd nodes (the other node type) hold it; its class matches a strict subset of the
    nodes; one resource — every resource — EQUAL to an even node's total (<=, not <)"""
    return [([4 * Gi, 17000, 0, 0], 0), ([1 * Gi, 1000, 1 * Gi, 0], 0), ([100 * Gi, 2000, 3 * Gi, 0], 0), ([2 * Gi, 3000, 5 * Gi, 0], 1), ([64 * Gi, 16000, 512 * Gi, 0], 0)]


def _new_shapes(k):
    """k distinct shapes no base table has: the edge shapes first, then requests that differ in the non-indexed column (each a fit shape of its own)"""
    sh = _edge_shapes()[:k]
    sh += [([2 * Gi, 1000, (300 + j) * Gi, 0], j % 2) for j in range(k - len(sh))]
    return np.array([r for r, _ in sh], dtype=np.int64), np.array([c for _, c in sh], dtype=np.int32)


# ---------------------------------------------------------------- what a handle answers
def _view(s, wl, tail):
    """everything of a handle that has nodes and jobs and no round: the order, every row's first fit at every priority level, the node types matching the new rows, and
    a submit check whose units include the new rows"""
    jobs = np.arange(wl.num_jobs, dtype=np.int32)
    single = [int(j) for j in jobs if wl.job_gang[j] < 0]
    new = [int(j) for j in tail if wl.job_gang[j] < 0]
    out = [[s.scheduling_order(q) for q in range(wl.num_queues)]]
    out += [s.fit_select_batch(jobs, p).tolist() for p in s.priorities]
    out.append([s.node_types_matching_job(int(j)) for j in tail])
    out.append(s.submit_check([[j] for j in single[:30] + new[:70]] + ([new[:3]] if len(new) >= 3 else [])))
    return out


def _after_round(s, wl, tail):
    r, st = _round(s, wl)
    return r, st, [s.job_key_unfeasible(int(j)) for j in tail]


def _same_as_fresh(lib, oracle_lib, cpu_lib, a, wl, tail, cpu=None):
    """handle `a` (appended in place) against a fresh handle of the whole table, the oracle's round, and — on the HIP library — the CPU build's answers `cpu`"""
    f = W.load(lib, wl)
    va, vf = _view(a, wl, tail), _view(f, wl, tail)
    assert va == vf
    ra, sta, ua = _after_round(a, wl, tail)
    rf, stf, uf = _after_round(f, wl, tail)
    f.close()
    o = W.load(oracle_lib, wl)
    ro, _ = _round(o, wl)
    o.close()
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert ua == uf
    assert ra.fair_share.tobytes() == rf.fair_share.tobytes() == ro.fair_share.tobytes()
    assert sta["fast_iterations"] == stf["fast_iterations"], "the appended handle did not run the fresh handle's fast iterations"
    if cpu is None and lib is not cpu_lib:            # on the HIP library: the CPU build's answers for the same table, from a fresh handle of it
        c = W.load(cpu_lib, wl)
        vc = _view(c, wl, tail)
        rc, _, uc = _after_round(c, wl, tail)
        c.close()
        cpu = (vc, rc, uc)
    if cpu is not None:
        assert va == cpu[0] and ua == cpu[2]
        scenario.assert_same_round(cpu[1], ra)
    return va, ra, ua


def _in_place(s, full, tail, expect, added=None, revived=0):
    s.set_append_in_place(True)
    st = _append_tail(s, full, tail)
    sh = s.jobs_append_shape_stats()
    assert st["rows"] == len(tail) and st["rebuilt"] == 0 and st["in_place"] == expect and sh["reason"] == 0 and sh["on"] == 1, (st, sh)
    assert sh["added"] == (expect - revived if added is None else added) and sh["revived"] == revived and st["new_shapes"] == sh["added"], (st, sh)
    return st, sh


def _check(lib, oracle_lib, cpu_lib, base, full, tail, expect, warm=True, **kw):
    """the whole comparison for one append.  warm: the handle ran a round on the base table first (the fast structure, the records and the masks have been used)"""
    out = []
    for L in ([lib] if lib == cpu_lib else [cpu_lib, lib]):
        a = W.load(L, base)
        if warm:
            _round(a, base)
        st, sh = _in_place(a, full, tail, expect, **kw)
        out.append(_same_as_fresh(L, oracle_lib, cpu_lib, a, full, tail, cpu=out[0] if out else None))
        a.close()
    return st, sh


# ---------------------------------------------------------------- a. mask edges
NODES = [1, 63, 64, 65, 255, 256, 257, 320]       # a lone lane, the word edge, the four-word block edge, a partial last word


def test_the_extended_table_is_a_table_of_new_shapes(lib, oracle_lib):
    """a pin of this file's own helpers, not of the feature: _extend builds the table every case uploads to its fresh handle — the library and the oracle agree on its
    round — and _new_shapes are k new distinct shapes whose first five hit the edges they name.  It calls no jobs_append, so it also passes without the feature."""
    base = _base(65)
    req, cls = _new_shapes(65)
    full, tail = _extend(base, req, cls=cls)
    assert _shape_count(full) == _shape_count(base) + 65 and _shape_count(full, tail) == 65
    s, o = W.load(lib, full), W.load(oracle_lib, full)
    fit = s.fit_select_batch(tail.astype(np.int32))
    assert fit.tolist() == o.fit_select_batch(tail.astype(np.int32)).tolist()
    assert fit[0] < 0 and fit[1] == 0 and fit[2] == 1 and fit[3] == 1 and fit[4] == 0, fit[:5]      # none / all / the odd nodes by size / by class / equal to the total
    rs, _ = _round(s, full)
    ro, _ = _round(o, full)
    scenario.assert_same_round(ro, rs)
    s.close(); o.close()


@pytest.mark.parametrize("n", NODES)
def test_mask_rows_at_the_word_edges(lib, oracle_lib, hostsim_lib, n):
    base = _base(n, n_jobs=200)
    req, cls = _new_shapes(5)
    full, tail = _extend(base, np.repeat(req, 2, axis=0), cls=np.repeat(cls, 2), pc=[0, 1] * 5)      # two priority classes of each: ten shapes
    _, sh = _check(lib, oracle_lib, hostsim_lib, base, full, tail, 10)
    assert sh["mask_rows"] == 10 and sh["derived_classes"] == 0


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("k", [1, 2, 5, 64, 65])
def test_k_new_shapes_in_one_call(lib, oracle_lib, hostsim_lib, n, k):
    base = _base(n, n_jobs=200)
    req, cls = _new_shapes(k)
    full, tail = _extend(base, req, cls=cls)
    _check(lib, oracle_lib, hostsim_lib, base, full, tail, k)


# ---------------------------------------------------------------- b. away rows
@pytest.mark.parametrize("derived", [False, True])
def test_new_shapes_with_away_rows(lib, oracle_lib, hostsim_lib, derived):
    """W.small_random(away=True): priority class 1 has one away entry, class 2 two.  The new away rows go behind the old ones, which move (they start at the number of
    shapes); derived: the new shapes are of requirement class 2, which had no away rows — its derived classes are new, and get ids behind the old ones"""
    base = _base(130, away=True, seed=33)
    assert (base.job_pc[base.job_req_class == 2] == 0).all() and (base.job_pc[base.job_req_class == 0] > 0).any()
    req, _ = _new_shapes(4)
    full, tail = _extend(base, np.concatenate([req, req[:2]]), cls=2 if derived else 0, pc=[1, 2, 1, 2, 0, 0])
    _, sh = _check(lib, oracle_lib, hostsim_lib, base, full, tail, 6)
    assert sh["mask_rows"] == 6 + 1 + 2 + 1 + 2, sh
    assert sh["derived_classes"] == (2 if derived else 0), sh      # (class 2, well-known type 0) and (class 2, well-known type 1)
    away = [j for j in range(base.num_jobs) if base.job_pc[j] > 0]
    assert away, "no resident row has away rows: the case does not move any"


# ---------------------------------------------------------------- c. records and fit shapes
def _fit_shapes(s):
    """F of a handle: an append of no rows reports it"""
    s.jobs_append(np.zeros((0, W.R), np.int64))
    return s.jobs_append_shape_stats()["fit_shapes"]


def test_fit_shape_reused_or_added(lib, oracle_lib, hostsim_lib):
    """a new shape that equals an old one in everything a fit looks at (another priority class) shares its fit shape; one with another request is a fit shape more"""
    base = _base(130)
    have = {(int(c), int(p)) + tuple(int(x) for x in r) for c, p, r in zip(base.job_req_class, base.job_pc, base.job_req)}
    j = next(j for j in range(base.num_jobs) if base.job_gang[j] < 0 and any((int(base.job_req_class[j]), p) + tuple(int(x) for x in base.job_req[j]) not in have for p in range(3)))
    p = next(p for p in range(3) if (int(base.job_req_class[j]), p) + tuple(int(x) for x in base.job_req[j]) not in have)
    s = W.load(lib, base)
    f0 = _fit_shapes(s)
    s.close()
    assert 0 < f0 < SMAX
    full, tail = _extend(base, [base.job_req[j]] * 3, cls=base.job_req_class[j], pc=p)
    _, sh = _check(lib, oracle_lib, hostsim_lib, base, full, tail, 1)
    assert sh["fit_shapes"] == f0, (sh, f0)
    full, tail = _extend(base, [[2 * Gi, 1000, 333 * Gi, 0]] * 3)
    _, sh = _check(lib, oracle_lib, hostsim_lib, base, full, tail, 1)
    assert sh["fit_shapes"] == f0 + 1, (sh, f0)


def test_fit_shapes_reach_smax_exactly_and_one_more_falls_back(lib, oracle_lib, hostsim_lib):
    base = _base(65)
    s = W.load(lib, base)
    f0 = _fit_shapes(s)
    s.close()
    k = SMAX - f0
    req = np.array([[2 * Gi, 1000, (300 + j) * Gi, 0] for j in range(k + 1)], dtype=np.int64)
    full, tail = _extend(base, req[:k])
    _, sh = _check(lib, oracle_lib, hostsim_lib, base, full, tail, k)
    assert sh["fit_shapes"] == SMAX
    # 257 distinct fit shapes: the rebuild, which gives the handle up to the generic scan as jobs_set does
    full, tail = _extend(base, req)
    a = W.load(lib, base)
    a.set_append_in_place(True)
    st = _append_tail(a, full, tail)
    sh = a.jobs_append_shape_stats()
    assert st["rebuilt"] == 1 and st["in_place"] == 0 and sh["reason"] == 4 and sh["added"] == 0, (st, sh)
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_an_unaligned_new_shape(lib, oracle_lib, hostsim_lib):
    """a request off the index grid: a literal row.  The base table (W.small_random(offgrid=1): one node type, the fast structure next to literal rows) has such rows
    already; the first one of a table changes the key layout"""
    base = W.small_random(n_nodes=130, n_jobs=240, n_queues=3, seed=35, occupied=0.5, gangs=2, offgrid=1)
    assert (base.job_req[:, CPU] % 1000 != 0).any()
    full, tail = _extend(base, [[4 * Gi, 2125, 7 * Gi, 0]] * 2 + [[4 * Gi + 1000, 2000, 7 * Gi, 0]] * 2)
    _check(lib, oracle_lib, hostsim_lib, base, full, tail, 2)


def _emptied(lib, base, n_shapes=1):
    """a handle of `base` minus every row of n_shapes of its shapes (single queued jobs), deleted on the device with the switch on -> (handle, reduced table, the deleted rows' fields)"""
    key = lambda j: (int(base.job_req_class[j]), int(base.job_pc[j])) + tuple(int(x) for x in base.job_req[j])
    by = {}
    for j in range(base.num_jobs):
        by.setdefault(key(j), []).append(j)
    pick = [rows for rows in by.values() if all(base.job_node[j] < 0 and base.job_gang[j] < 0 for j in rows)][:n_shapes]
    assert len(pick) == n_shapes
    gone = np.array(sorted(j for rows in pick for j in rows), dtype=np.int32)
    keep = np.array([j for j in range(base.num_jobs) if j not in set(gone.tolist())], dtype=np.int64)
    red = copy.copy(base)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class"):
        setattr(red, f, np.asarray(getattr(base, f))[keep].copy())
    new_of = np.full(base.num_jobs, -1, np.int64)
    new_of[keep] = np.arange(len(keep))
    red.queued = [new_of[np.asarray([j for j in q if new_of[j] >= 0], dtype=np.int64)].astype(np.int32) for q in base.queued]
    s = W.load(lib, base)
    s.set_append_in_place(True)
    _round(s, base)
    s.jobs_delete(gone)
    assert s.jobs_delete_stats()["shapes_emptied"] == n_shapes
    return s, red, gone


def test_revived_shapes_alone_and_with_new_ones(lib, oracle_lib, hostsim_lib):
    base = _base(130)
    for with_new in (False, True):
        s, red, gone = _emptied(lib, base, 2)
        req, cls, pc = base.job_req[gone], base.job_req_class[gone], base.job_pc[gone]
        if with_new:
            req, cls, pc = np.concatenate([req, [[2 * Gi, 1000, 301 * Gi, 0]] * 2]), np.concatenate([cls, [0, 0]]), np.concatenate([pc, [0, 0]])
        full, tail = _extend(red, req, cls=cls, pc=pc)
        _in_place(s, full, tail, 3 if with_new else 2, revived=2)
        _same_as_fresh(lib, oracle_lib, hostsim_lib, s, full, tail)
        s.close()


def test_a_second_append_of_the_same_new_shape_copies_the_resident_row(lib, oracle_lib, hostsim_lib):
    base = _base(65)
    full1, tail1 = _extend(base, [[2 * Gi, 1000, 301 * Gi, 0]] * 2)
    full2, tail2 = _extend(full1, [[2 * Gi, 1000, 301 * Gi, 0]] * 3)
    a = W.load(lib, base)
    _in_place(a, full1, tail1, 1)
    st = _append_tail(a, full2, tail2)
    sh = a.jobs_append_shape_stats()
    assert st["in_place"] == 0 and st["rebuilt"] == 0 and st["new_shapes"] == 0 and sh["reason"] == 0 and sh["added"] == 0, (st, sh)
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, full2, np.concatenate([tail1, tail2]))
    a.close()


def test_six_growing_appends_of_new_shapes(lib, oracle_lib, hostsim_lib):
    """jobs_set allocates exactly M: the first append re-allocates, later ones fit the 1.25 x capacity or re-allocate again — the records of the resident rows move device
    to device and the new rows' come from their templates, every time"""
    base = _base(65, n_jobs=120)
    a = W.load(lib, base)
    cur, stats, tails = base, [], []
    for k in range(6):
        m = [7, 40, 3, 90, 11, 200][k]
        cur, tail = _extend(cur, np.array([[2 * Gi, 1000 * (1 + i % 3), (400 + 10 * k + i % 4) * Gi, 0] for i in range(m)], dtype=np.int64), pc=k % 3)
        st, _ = _in_place(a, cur, tail, _shape_count(cur, tail))
        stats.append(st); tails.append(tail)
        if k in (0, 3):
            _round(a, cur)
    assert stats[0]["reallocated"] == 1 and sum(st["reallocated"] for st in stats) >= 2 and any(not st["reallocated"] for st in stats), stats
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, cur, np.concatenate(tails))
    a.close()


# ---------------------------------------------------------------- d. interplay: no jobs_set in between
def _appended(lib, n=130, away=True):
    base = _base(n, away=away, seed=37)
    req, cls = _new_shapes(7)
    full, tail = _extend(base, np.repeat(req, 2, axis=0), cls=np.repeat(cls, 2), pc=[1, 2] * 7 if away else [0, 1] * 7)
    a = W.load(lib, base)
    _round(a, base)
    _in_place(a, full, tail, 14)
    return a, full, tail


def test_jobs_patch_naming_new_rows_then_jobs_delete(lib, oracle_lib, hostsim_lib):
    a, full, tail = _appended(lib)
    w2 = copy.copy(full)
    w2.job_node, w2.job_run_prio, w2.job_run_ts = full.job_node.copy(), full.job_run_prio.copy(), full.job_run_ts.copy()
    lease = np.array([int(tail[2]), int(tail[5]), int(tail[12])], dtype=np.int32)      # an "every node" row, an "odd nodes" row, a filler: they start to run on node 1
    w2.job_node[lease], w2.job_run_prio[lease], w2.job_run_ts[lease] = 1, np.asarray(full.config.pc_priority)[full.job_pc[lease]], int(full.job_run_ts.max()) + 1
    leased = set(lease.tolist())
    w2.queued = [np.array([j for j in q if int(j) not in leased], dtype=np.int32) for q in full.queued]
    a.jobs_patch(lease, w2.job_node[lease], w2.job_run_prio[lease], w2.job_run_ts[lease])
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, w2, tail)
    # ... and rows leave: a new shape loses all its rows, old rows go as well
    gone = np.array(sorted({int(tail[0]), int(tail[3]), 5, 17} | {int(j) for j in tail if (w2.job_req[j] == w2.job_req[tail[8]]).all() and w2.job_pc[j] == w2.job_pc[tail[8]]}), dtype=np.int32)
    gone = np.array([j for j in gone if w2.job_gang[j] < 0 and j not in leased], dtype=np.int32)
    keep = np.array([j for j in range(w2.num_jobs) if j not in set(gone.tolist())], dtype=np.int64)
    red = copy.copy(w2)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class"):
        setattr(red, f, np.asarray(getattr(w2, f))[keep].copy())
    new_of = np.full(w2.num_jobs, -1, np.int64)
    new_of[keep] = np.arange(len(keep))
    red.queued = [new_of[np.asarray([j for j in q if new_of[j] >= 0], dtype=np.int64)].astype(np.int32) for q in w2.queued]
    a.jobs_delete(gone)
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, red, new_of[[j for j in tail if new_of[j] >= 0]])
    a.close()


def test_round_prepare_resident_after_an_in_place_append(lib, hostsim_lib):
    a, full, tail = _appended(lib)
    kw = dict(global_tokens=float(full.global_burst), global_burst=full.global_burst, global_rate_inf=True, queue_tokens=[float(full.queue_burst)] * full.num_queues,
              queue_burst=[full.queue_burst] * full.num_queues, queue_rate_inf=[True] * full.num_queues)
    a.round_prepare_resident(full.queue_weight, **kw)
    assert [q.tolist() for q in a.round_queued()] == [np.asarray(q).tolist() for q in full.queued]
    ra = a.schedule_round()
    for L in {lib, hostsim_lib}:                                 # a fresh handle of the same library and, on the HIP library, of the CPU build
        f = W.load(L, full)
        rf, _ = _round(f, full)
        scenario.assert_same_round(rf, ra)
        f.close()
    assert any(j >= tail[0] for j in ra.scheduled), "no appended job was scheduled"
    a.close()


@pytest.mark.parametrize("what", ["patch", "delete", "append", "upsert"])
def test_node_table_changes_after_an_in_place_append(lib, oracle_lib, hostsim_lib, what):
    """nodes_patch / nodes_delete / nodes_append read the mask blocks through the handle: they find the grown ones — the right number of class and shape rows, the
    swapped blocks — and write the new rows' bits of changed and new nodes"""
    a, full, tail = _appended(lib, n=130)
    n = full.num_nodes
    w = copy.copy(full)
    free = np.array([i for i in range(n) if i not in set(np.asarray(full.job_node).tolist())][:3] + [n - 1], dtype=np.int32)
    if what == "patch":
        rows = np.array([0, 63, 64, 65, 128, 129], dtype=np.int32)
        alloc = full.node_total[rows].copy()
        alloc[:, CPU] -= 2000
        alloc[::2, MEM] -= 8 * Gi
        a.nodes_patch(rows, allocatable=alloc)
        assert a.nodes_patch_stats()[2] == 0, "the patch took its rebuild path: the case does not read the grown blocks"
        w.node_allocatable = full.node_total.copy()
        w.node_allocatable[rows] = alloc
    elif what == "delete":
        rows = np.array(sorted(set(free.tolist()) - {n - 1}), dtype=np.int32)
        a.nodes_delete(rows)
        assert a.nodes_delete_stats()[2] == 0, "the delete took its rebuild path"
        keep = np.array([i for i in range(n) if i not in set(rows.tolist())])
        new_of = np.full(n, -1, np.int64)
        new_of[keep] = np.arange(len(keep))
        w.node_total = full.node_total[keep]
        w.node_taints = [full.node_taints[i] for i in keep]
        w.node_labels = [full.node_labels[i] for i in keep]
        w.job_node = np.where(full.job_node >= 0, new_of[np.maximum(full.job_node, 0)], -1).astype(np.int32)
    elif what == "append":
        src = np.array([0, 1, 64, 65, 3], dtype=np.int64)
        a.nodes_append(full.node_total[src], index=n + 1 + np.arange(len(src)), taints=[full.node_taints[i] for i in src], labels=[full.node_labels[i] for i in src])
        assert a.nodes_append_stats()[2] == 0, "the append of nodes took its rebuild path"
        w.node_total = np.concatenate([full.node_total, full.node_total[src]])
        w.node_taints = list(full.node_taints) + [full.node_taints[i] for i in src]
        w.node_labels = list(full.node_labels) + [full.node_labels[i] for i in src]
    else:
        a.nodes_upsert(full.node_total, full.node_allocatable, taints=full.node_taints, labels=full.node_labels, id_rank=full.node_id_rank)
    assert a.jobs_append_shape_stats()["on"] == 1
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, w, tail)
    # the switch survives: another in-place append on the changed node table
    w3, tail3 = _extend(w, [[3 * Gi, 2000, 77 * Gi, 0]] * 2, pc=1)
    st = _append_tail(a, w3, tail3)
    assert st["rebuilt"] == 0 and st["in_place"] == 1, (st, a.jobs_append_shape_stats())
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, w3, tail3)
    a.close()


def test_a_handle_without_the_fast_structure_takes_the_mask_part(lib, oracle_lib, hostsim_lib):
    """W.fine_indexed: two-word order keys — no JobRec table, no fit shapes in use; the masks grow in place all the same"""
    base = W.fine_indexed(n_nodes=130, n_jobs=400)
    req = base.job_req[np.nonzero(base.job_node < 0)[0][:3]].copy()
    req[:, CPU] += np.array([1, 2, 3]) * int(base.config.indexed_resolution[list(base.config.indexed_col).index(CPU)])
    full, tail = _extend(base, np.repeat(req, 2, axis=0))
    k = _shape_count(full) - _shape_count(base)
    assert k >= 1
    a = W.load(lib, base)
    _round(a, base)
    st, sh = _in_place(a, full, tail, k)
    assert sh["mask_rows"] == k
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


# ---------------------------------------------------------------- e. fallbacks: each reason code once, and a correct round after it
def _falls_back(lib, oracle_lib, hostsim_lib, a, full, tail, reason):
    a.set_append_in_place(True)
    st = _append_tail(a, full, tail)
    sh = a.jobs_append_shape_stats()
    assert st["rebuilt"] == 1 and st["in_place"] == 0 and sh["reason"] == reason and sh["added"] == sh["revived"] == sh["mask_rows"] == 0, (st, sh)
    f = W.load(lib, full)
    assert sh["fit_shapes"] == _fit_shapes(f), "fit shapes AFTER the call: what the rebuild derived"
    f.close()
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_fallback_key_layout_changes(lib, oracle_lib, hostsim_lib):
    """a negative request on an indexed column: the grown table needs the wide field layout"""
    base = _base(65)
    full, tail = _extend(base, [[4 * Gi, -1000, 7 * Gi, 0]] * 2)
    _falls_back(lib, oracle_lib, hostsim_lib, W.load(lib, base), full, tail, 2)


def test_fallback_first_away_rows(lib, oracle_lib, hostsim_lib):
    """priority classes with away entries are configured, but no resident row has one: the table has no away rows, and the batch turns them on"""
    base = _base(65, away=True)
    base.job_pc = np.zeros_like(base.job_pc)
    base.job_run_prio = np.where(base.job_node >= 0, 0, 0).astype(np.int32)
    base.queued = W._sort_queued(base.job_queue, np.zeros(base.num_jobs, np.int64), base.job_submit, np.nonzero(base.job_node < 0)[0])
    while len(base.queued) < base.num_queues:
        base.queued.append(np.zeros(0, np.int32))
    full, tail = _extend(base, [[2 * Gi, 1000, 301 * Gi, 0]] * 2, pc=1)
    _falls_back(lib, oracle_lib, hostsim_lib, W.load(lib, base), full, tail, 3)


def test_fallback_before_nodes_upsert(lib, oracle_lib, hostsim_lib):
    base = _base(65)
    full, tail = _extend(base, [[2 * Gi, 1000, 301 * Gi, 0]] * 2)
    a = Scheduler(lib, base.config)
    W.set_jobs(a, base)
    a.set_append_in_place(True)
    st = _append_tail(a, full, tail)
    sh = a.jobs_append_shape_stats()
    assert st["in_place"] == 0 and sh["reason"] == 1, (st, sh)
    a.nodes_upsert(full.node_total, full.node_allocatable, taints=full.node_taints, labels=full.node_labels, id_rank=full.node_id_rank)
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_fallback_negative_request_off_the_index(lib, oracle_lib, hostsim_lib):
    """the fast structure does not serve a table with a negative request: the rebuild takes it away, as jobs_set would"""
    base = _base(65)
    full, tail = _extend(base, [[2 * Gi, 1000, -1 * Gi, 0]] * 2)
    _falls_back(lib, oracle_lib, hostsim_lib, W.load(lib, base), full, tail, 5)


def test_fallback_table_without_rows(lib, oracle_lib, hostsim_lib):
    """jobs_set of an empty table: no rows and no shapes — the fast structure's predicate can turn true with the first rows, which is the rebuild's to decide"""
    base = _base(65)
    empty = copy.copy(base)
    for f in ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class"):
        setattr(empty, f, np.asarray(getattr(base, f))[:0].copy())
    empty.queued = [np.zeros(0, np.int32) for _ in range(base.num_queues)]
    rows = np.nonzero((base.job_node < 0) & (base.job_gang < 0))[0][:60]
    full, tail = _extend(empty, base.job_req[rows], pc=base.job_pc[rows], cls=base.job_req_class[rows], queue=base.job_queue[rows])
    _falls_back(lib, oracle_lib, hostsim_lib, W.load(lib, empty), full, tail, 6)


# ---------------------------------------------------------------- f. refusals leave the handle as it was, with the switch on
def test_refusals_with_the_switch_on(lib, hostsim_lib):
    base = _base(65)
    a = W.load(lib, base)
    a.set_append_in_place(True)
    full, tail = _extend(base, [[2 * Gi, 1000, 301 * Gi, 0]] * 2)
    before = _view(a, base, [0, 1])
    g = next(j for j in range(base.num_jobs) if base.job_gang[j] >= 0)
    for kw, code in ((dict(req_class=[0, 3]), ERR_INVALID),                                                       # beyond the classes of the last jobs_set
                     (dict(queue=[int(base.job_queue[g])] * 2, gang_id=[int(base.job_gang[g])] * 2, gang_cardinality=[2, 2]), ERR_UNSUPPORTED)):   # a resident gang
        with pytest.raises(SchedError) as e:
            a.jobs_append(full.job_req[tail], **kw)
        assert e.value.code == code
        assert _view(a, base, [0, 1]) == before and a.num_jobs == base.num_jobs
    _in_place(a, full, tail, 1)                                  # and the handle still serves the path
    if lib is not hostsim_lib:                                   # the HIP library's answers are the CPU build's
        c = W.load(hostsim_lib, full)
        assert _view(a, full, tail) == _view(c, full, tail)
        c.close()
    a.close()


def test_lit_tmax_refusal_with_the_switch_on(lib, hostsim_lib):
    """test_z_jobs_append's table of LIT_TMAX + 1 node types under unaligned allocatable: a new shape whose class matches them all is refused after the shape lookup, and
    everything the in-place path had looked at is put back"""
    t = ManyTypes()
    off_grid = t.batch([3000, 1500, 1000], 1, 3)                   # a new shape on the grid, then one off it, then a resident one
    s = t.handle(lib)
    s.set_append_in_place(True)
    before = t.view(s)
    for _ in range(2):
        with pytest.raises(SchedError) as e:
            s.jobs_append(off_grid["req"], queue=off_grid["queue"], pc=off_grid["pc"], submit_time=off_grid["submit"])
        assert e.value.code == ERR_UNSUPPORTED and "LIT_TMAX" in str(e.value)
        assert t.view(s) == before
    b = t.batch([5000, 5000, 1000], 3, 0)                          # the handle still appends, and in place
    s.jobs_append(b["req"], queue=b["queue"], pc=b["pc"], submit_time=b["submit"])
    st, sh = s.jobs_append_stats(), s.jobs_append_shape_stats()
    assert st["rebuilt"] == 0 and st["in_place"] == 1 and sh["reason"] == 0, (st, sh)
    f, c = t.handle(lib, [b]), t.handle(hostsim_lib, [b])        # (on the HIP library also against the CPU build)
    assert t.view(s) == t.view(f) == t.view(c)
    s.close(); f.close(); c.close()


# ---------------------------------------------------------------- g. the switch
def test_switch_off_is_the_rebuild_and_the_switch_survives_jobs_set(lib, oracle_lib, hostsim_lib):
    """off: an append with a new shape reports rebuilt == 1, in_place == 0, reason 0 and no shape statistics, and leaves what jobs_set leaves; the switch survives
    jobs_set, the statistics do not; turned off again the next new shape rebuilds.  What is compared in launches is the ROUND after either kind of append, through
    round_timing — the library keeps no count of what an append itself launches, so that part of the contract rests on the code: with the switch off no branch of
    asched_jobs_append differs from the one before the switch existed."""
    base = _base(65)
    full, tail = _extend(base, [[2 * Gi, 1000, 301 * Gi, 0]] * 2)
    a = W.load(lib, base)
    assert a.jobs_append_shape_stats() == dict(on=0, added=0, revived=0, mask_rows=0, derived_classes=0, fit_shapes=0, reason=0)
    st = _append_tail(a, full, tail)
    sh = a.jobs_append_shape_stats()
    assert st["rebuilt"] == 1 and st["in_place"] == 0 and st["new_shapes"] == 1 and sh["on"] == 0 and sh["reason"] == 0 and sh["added"] == 0, (st, sh)
    _same_as_fresh(lib, oracle_lib, hostsim_lib, a, full, tail)
    n_off = a.round_timing()["launches"]
    a.set_append_in_place(True)
    W.set_jobs(a, base)                                          # jobs_set: the statistics are zero, the switch stays
    sh = a.jobs_append_shape_stats()
    assert sh == dict(on=1, added=0, revived=0, mask_rows=0, derived_classes=0, fit_shapes=0, reason=0) and a.jobs_append_stats()["in_place"] == 0
    _in_place(a, full, tail, 1)
    _round(a, full)
    assert a.round_timing()["launches"] == n_off, "a ROUND after an in-place append launches what a round after the rebuild launches (the append's own launches are not counted by the library)"
    a.set_append_in_place(False)
    full2, tail2 = _extend(full, [[2 * Gi, 1000, 302 * Gi, 0]])
    st = _append_tail(a, full2, tail2)
    assert st["rebuilt"] == 1 and st["in_place"] == 0
    a.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = _base(20, n_jobs=60)
    o = W.load(oracle_lib, wl)
    for call in (lambda: o.set_append_in_place(True), o.jobs_append_shape_stats):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    o.close()


# ---------------------------------------------------------------- h. the simulator fixture, its jobs arriving a cycle's worth at a time
def _sim_with_a_shape_per_cycle(per_cycle, period):
    """the simulator fixture (one scheduling-key shape, 300 s jobs) made to bring shapes: the rows that arrive in cycle c ask for (10 + c % period) GiB, and every job runs
    for 15 s, a cycle and a half — so with period 3 the rows of cycle c have finished and been deleted by the time cycle c + 3 brings their shape again"""
    import dataclasses
    sim = S.from_fixture(FIXTURE)
    wl = copy.copy(sim.workload)
    cyc = S.arrival_cycles(sim, per_cycle)
    wl.job_req = wl.job_req.copy()
    wl.job_req[:, MEM] = (10 + cyc % period) * Gi
    return dataclasses.replace(sim, workload=wl, job_runtime_s=np.full(wl.num_jobs, 15.0))


def test_simulator_cycles_in_place_equal_rebuilt(lib, oracle_lib):
    """eight cycles of 40 arrivals.  run_cycles_arriving, a new shape in every cycle after the first: seven in place, no append rebuilt.  run_cycles_resident, where the
    finished rows are deleted every cycle, three shapes in turn: two new ones, then five that the deletes had emptied come back — in place as well"""
    sim = _sim_with_a_shape_per_cycle(40, 1000)
    assert len(np.unique(sim.workload.job_req[:320], axis=0)) == 8
    got = S.run_cycles_arriving(lib, sim, per_cycle=40, max_cycles=8, in_place=True)
    want = S.run_cycles_arriving_rebuilt(oracle_lib, sim, per_cycle=40, max_cycles=8)
    assert len(got) == len(want) == 8 and got[-1]["rows"] == 320 and all(len(c["scheduled"]) == 40 for c in got)
    assert _records(got) == _records(want)
    assert [c["shapes_in_place"] for c in got] == list(range(8)) and all(c["appends_rebuilt"] == 0 for c in got), [(c["shapes_in_place"], c["appends_rebuilt"]) for c in got]
    off = S.run_cycles_arriving(lib, sim, per_cycle=40, max_cycles=8)                      # the default: every one of those appends rebuilds, same records
    assert _records(off) == _records(want) and "shapes_in_place" not in off[0]
    sim = _sim_with_a_shape_per_cycle(40, 3)
    assert len(np.unique(sim.workload.job_req[:320], axis=0)) == 3
    res = S.run_cycles_resident(lib, sim, per_cycle=40, max_cycles=8, in_place=True)
    assert _records(res) == _records(S.run_cycles_compacting_rebuilt(oracle_lib, sim, per_cycle=40, max_cycles=8))
    assert len(res) == 8 and res[-1]["rows"] < 160, "the finished rows were not deleted: no shape was emptied"
    assert [c["shapes_in_place"] for c in res] == list(range(8)) and all(c["appends_rebuilt"] == 0 for c in res), [(c["shapes_in_place"], c["appends_rebuilt"]) for c in res]
