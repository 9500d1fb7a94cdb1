"""asched_req_classes_append: NEW requirement classes — a node selector, a hostname pin, a toleration or a required node affinity the table has not seen — join the
resident class table behind the C real ones (armada_amd/csrc/kernels_req_classes_append.h) instead of asched_jobs_set of the whole job table.  The contract: the handle
is what jobs_set of the same job table with the concatenated class list would have left; rows of the new classes then arrive by jobs_append.

Every equivalence case asserts the exact statistics — rebuilt == 0, reason 0, the rows decided by node type on the device, the rows matched on the host, the derived rows
moved — so a silent fallback does not pass, and compares the handle with a fresh handle given the same table and the whole class list: scheduling_order, the first fit
of every row at every priority level, the node types matching the rows of the new classes, a submit check with units of them, a round (also against the oracle's round),
the unfeasible keys and the excluded nodes the round left for them, the fair shares bit for bit and the number of fast iterations.
a. mask and lane edges; b. classes matched on the host; c. derived classes move; d. the class bits of the nodes; e. interplay; f. refusals; g. the gap this closes.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library, whose answers must also equal the CPU build's.
(asched_nodes_patch takes taints, not labels: case c flips a new class's bit on a node by its taints.)"""
import copy
import ctypes as C

import numpy as np
import pytest

import scenario
from armada_amd import workloads as W
from armada_amd.binding import AFFINITY_OPS, CReqClasses, SchedError, Scheduler
from test_z_jobs_append import _append_tail, _round
from test_z_jobs_append_shapes import _extend, _view

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
Gi = W.Gi
EXISTS9 = (9, 1, 0, 0)            # toleration: Exists on taint key 9
EQUAL9 = (9, 0, 1, 1)             # toleration: key 9 == 1, NoSchedule
IN, NOT_IN, EX, GT, LT = (AFFINITY_OPS[k] for k in ("In", "NotIn", "Exists", "Gt", "Lt"))
INTS = {100: 0, 101: 1, 102: 2, 103: 3}   # interned label values that parse as integers (label key 6)


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


# ---------------------------------------------------------------- the tables
def _tbl(n, n_jobs=200, seed=41, away=False, n_classes=2, indexed_taints=None, stray_taint=False, override=False):
    """W.small_random with six node types — an indexed label (key 3) with three values, an indexed taint (key 9) on every fourth node — a label key that is not
    indexed (5) and one whose values parse as integers (6).  Every resident class tolerates the taint; class 1 selects label value 1; classes beyond 1 have no rows.
    stray_taint: node 2 carries a taint whose key is not indexed (the config then indexes key 9 only); override: the table is uploaded with node_type_override"""
    wl = W.small_random(n_nodes=n, n_jobs=n_jobs, n_queues=3, seed=seed, occupied=0.5, gangs=2, away=away)
    wl.config.indexed_label_keys = [3]
    wl.config.indexed_taint_keys = [9] if stray_taint else indexed_taints
    wl.node_labels = [[(3, i % 3), (5, i % 2), (6, 100 + i % 4)] for i in range(n)]
    taints = [list(t) for t in wl.node_taints] if wl.node_taints is not None else [[] for _ in range(n)]
    for i in range(0, n, 4):
        taints[i].append((9, 1, 1))
    if stray_taint:
        taints[min(2, n - 1)].append((11, 1, 1))
    wl.node_taints = taints
    rng = np.random.default_rng(seed)
    cls = rng.choice(2, size=wl.num_jobs, p=[0.7, 0.3]).astype(np.int32) if n_classes > 1 else np.zeros(wl.num_jobs, np.int32)
    cls[np.asarray(wl.job_node) >= 0] = 0
    cls[np.asarray(wl.job_gang) >= 0] = 0
    wl.job_req_class = cls
    wl.class_tolerations = [[EXISTS9] for _ in range(n_classes)]
    wl.class_selectors = [[(3, 1)] if c == 1 else ([(3, c % 3)] if c > 1 else []) for c in range(n_classes)]
    wl.class_affinities = None
    wl.type_override = (np.arange(n) % 2).astype(np.int64) if override else None
    return wl


def _load(L, wl, nodes=True):
    s = Scheduler(L, wl.config)
    s.set_label_value_ints(INTS)
    if nodes:
        _nodes(s, wl)
    _jobs(s, wl)
    return s


def _nodes(s, wl):
    s.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank, node_type_override=wl.type_override)


def _jobs(s, wl):
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, submit_time=wl.job_submit, node=wl.job_node, scheduled_at_priority=wl.job_run_prio,
               run_timestamp=wl.job_run_ts, gang_id=wl.job_gang, gang_cardinality=wl.job_gang_card, req_class=wl.job_req_class,
               class_tolerations=wl.class_tolerations, class_selectors=wl.class_selectors, class_affinities=wl.class_affinities, away=wl.job_away)


# (tolerations, selector, affinity) of a new class.  Decided by node type:
NONE = ([EXISTS9], [(3, 7)], None)              # a selector value no type has: no node
EVERY = ([EXISTS9], [], None)                   # every node
ONE_TYPE = ([], [(3, 2)], None)                 # the untainted nodes of label value 2: one type
OPENS = ([EXISTS9], [(3, 0)], None)             # the toleration opens the tainted type of label value 0: two types
ALL_TYPES = ([EQUAL9], [], None)                # every type, by another toleration than EVERY
PLAIN = ([], [], None)                          # the untainted nodes: three types
TIER1 = [NONE, EVERY, ONE_TYPE, OPENS, ALL_TYPES]
# matched on the host:
NON_INDEXED = ([EXISTS9], [(5, 1)], None)
AFF_IN = ([EXISTS9], [], [[(3, IN, [0, 1])]])
AFF_NOT_IN = ([], [], [[(5, NOT_IN, [0])]])
AFF_EXISTS = ([EXISTS9], [(3, 1)], [[(6, EX, [])]])
AFF_GT = ([EXISTS9], [], [[(6, GT, [101])]])
AFF_LT_OR = ([EXISTS9], [], [[(6, LT, [102]), (3, IN, [0])], [(3, IN, [2])]])      # two terms
TIER2 = [NON_INDEXED, AFF_IN, AFF_NOT_IN, AFF_EXISTS, AFF_GT, AFF_LT_OR]


def _with_classes(wl, classes):
    """the table jobs_set would be given: the same rows, the class list with `classes` behind it"""
    w = copy.copy(wl)
    c0 = len(wl.class_tolerations)
    w.class_tolerations = list(wl.class_tolerations) + [list(t) for t, _, _ in classes]
    w.class_selectors = list(wl.class_selectors) + [list(s) for _, s, _ in classes]
    aff = list(wl.class_affinities) if wl.class_affinities is not None else [None] * c0
    aff += [a for _, _, a in classes]
    w.class_affinities = aff if any(a is not None for a in aff) else None
    return w


def _rows_of(wl, first, k, pcs=(0,)):
    """rows of classes first .. first + k - 1 behind the table: per class and priority class a small request every node holds, and one only the large shapes hold"""
    req, cls, pc = [], [], []
    for c in range(first, first + k):
        for p in pcs:
            req += [[1 * Gi, 1000, 1 * Gi, 0], [8 * Gi, 2000, (20 + c) * Gi, 0]]
            cls += [c, c]
            pc += [p, p]
    return _extend(wl, np.array(req, dtype=np.int64), cls=np.array(cls, dtype=np.int32), pc=np.array(pc, dtype=np.int32))


def _append_classes(s, classes, first, by_type, on_host, moved):
    got = s.req_classes_append([t for t, _, _ in classes], [x for _, x, _ in classes], [a for _, _, a in classes])
    st = s.req_classes_append_stats()
    assert got == first, (got, first)
    assert st["added"] == len(classes) and st["rebuilt"] == 0 and st["reason"] == 0 and st["by_type"] == by_type and st["on_host"] == on_host and st["moved"] == moved, st
    assert st["classes"] == first + len(classes), st
    return st


def _append_rows(s, full, tail, in_place=True):
    s.set_append_in_place(in_place)
    st = _append_tail(s, full, tail)
    assert st["rows"] == len(tail) and st["rebuilt"] == (0 if in_place else 1), st
    return st


def _derived(wl):
    """derived away classes of a W.small_random(away=True) table: priority class 1 is away on well-known type 0, class 2 on types 1 and 0"""
    keys = set()
    for c, p in zip(wl.job_req_class, wl.job_pc):
        if p >= 1:
            keys.add((int(c), 0))
        if p == 2:
            keys.add((int(c), 1))
    return len(keys)


# ---------------------------------------------------------------- what a handle answers
def _answers(s, wl, tail):
    v = _view(s, wl, tail)
    r, st = _round(s, wl)
    after = [[s.job_key_unfeasible(int(j)) for j in tail], [s.excluded_nodes(int(j)) for j in tail]]
    return v, r, st, after


def _same(L, oracle_lib, cpu_lib, a, wl, tail, cpu=None):
    """handle `a` against a fresh handle of the whole table and class list, the oracle's round and — on the HIP library — the CPU build's answers"""
    f = _load(L, wl)
    va, ra, sta, xa = _answers(a, wl, tail)
    vf, rf, stf, xf = _answers(f, wl, tail)
    f.close()
    assert va == vf
    o = _load(oracle_lib, wl)
    ro, _ = _round(o, wl)
    o.close()
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert xa == xf
    assert ra.fair_share.tobytes() == rf.fair_share.tobytes() == ro.fair_share.tobytes()
    assert sta["fast_iterations"] == stf["fast_iterations"], "the handle did not run the fresh handle's fast iterations"
    if cpu is None and L is not cpu_lib:
        c = _load(cpu_lib, wl)
        vc, rc, _, xc = _answers(c, wl, tail)
        c.close()
        cpu = (vc, rc, xc)
    if cpu is not None:
        assert va == cpu[0] and xa == cpu[2]
        scenario.assert_same_round(cpu[1], ra)
    return (va, ra, xa), sta


def _libs(lib, cpu_lib):
    return [lib] if lib is cpu_lib else [cpu_lib, lib]


def _case(lib, oracle_lib, cpu_lib, base, classes, by_type, on_host, moved=0, warm=True, pcs=(0,), in_place=True):
    """one class append, then the rows of the new classes by jobs_append, compared with the fresh handle"""
    c0 = len(base.class_tolerations)
    full, tail = _rows_of(_with_classes(base, classes), c0, len(classes), pcs)
    out, sta = None, None
    for L in _libs(lib, cpu_lib):
        a = _load(L, base)
        if warm:
            _round(a, base)
        _append_classes(a, classes, c0, by_type, on_host, moved)
        _append_rows(a, full, tail, in_place)
        res, sta = _same(L, oracle_lib, cpu_lib, a, full, tail, cpu=out)
        out = out or res
        a.close()
    return sta


# ---------------------------------------------------------------- g. the gap this closes
def test_a_row_of_an_unknown_class_is_refused_until_the_class_is_appended(lib, oracle_lib, hostsim_lib):
    base = _tbl(65)
    full, tail = _rows_of(_with_classes(base, [ONE_TYPE]), 2, 1)
    a = _load(lib, base)
    with pytest.raises(SchedError) as e:
        _append_tail(a, full, tail)
    assert e.value.code == ERR_INVALID
    _append_classes(a, [ONE_TYPE], 2, 1, 0, 0)
    _append_rows(a, full, tail)
    _same(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    base = _tbl(8, n_jobs=20)
    o = _load(oracle_lib, base)
    with pytest.raises(SchedError) as e:
        o.req_classes_append([[]])
    assert e.value.code == ERR_UNSUPPORTED
    o.close()


# ---------------------------------------------------------------- a. mask and lane edges
NODES = [1, 63, 64, 65, 255, 256, 257, 320]       # a lone lane, the word edge, the four-wave block edge, a partial last word


@pytest.mark.parametrize("n", NODES)
def test_rows_decided_by_node_type_at_the_word_edges(lib, oracle_lib, hostsim_lib, n):
    _case(lib, oracle_lib, hostsim_lib, _tbl(n), TIER1, 5, 0)


def test_the_classes_match_what_they_are_named_for(lib):
    """a pin of this file's own classes: which nodes the rows of each class can go to, from the first fit of a request every node holds"""
    base = _tbl(65, n_jobs=40)
    classes = TIER1 + [PLAIN] + TIER2
    full, tail = _rows_of(_with_classes(base, classes), 2, len(classes))
    s = _load(lib, full)
    m = dict(zip(range(len(classes)), [s.node_types_matching_job(int(j))[0] for j in tail[::2]]))
    s.close()
    assert [m[k] for k in range(6)] == [0, 6, 1, 2, 6, 3], m      # none, every type, one, two, every type, the three untainted types


# ---------------------------------------------------------------- b. classes matched on the host
@pytest.mark.parametrize("n", [65, 257])
def test_rows_matched_on_the_host(lib, oracle_lib, hostsim_lib, n):
    _case(lib, oracle_lib, hostsim_lib, _tbl(n), TIER2, 0, 6)


def test_mixed_calls(lib, oracle_lib, hostsim_lib):
    _case(lib, oracle_lib, hostsim_lib, _tbl(130), [ONE_TYPE, AFF_GT, OPENS, NON_INDEXED], 2, 2, warm=False)


def test_a_taint_that_is_not_indexed_sends_every_class_to_the_host(lib, oracle_lib, hostsim_lib):
    _case(lib, oracle_lib, hostsim_lib, _tbl(130, stray_taint=True), [ONE_TYPE, EVERY, AFF_IN], 0, 3)


def test_a_table_with_node_type_override_sends_every_class_to_the_host(lib, oracle_lib, hostsim_lib):
    _case(lib, oracle_lib, hostsim_lib, _tbl(130, override=True), [ONE_TYPE, OPENS], 0, 2)


# ---------------------------------------------------------------- c. derived classes move
def _node_tables(wl):
    return dict(node_total=wl.node_total.copy(), node_taints=[list(t) for t in wl.node_taints], node_labels=[list(x) for x in wl.node_labels])


@pytest.mark.parametrize("k", [1, 2])
def test_derived_classes_move_and_the_node_mutators_find_them(lib, oracle_lib, hostsim_lib, k):
    base = _tbl(130, away=True, seed=43)
    moved = _derived(base)
    assert moved >= 2
    classes = [PLAIN, AFF_IN][:k]
    c0 = 2
    wl, tail0 = _rows_of(_with_classes(base, classes), c0, k)
    idle = [i for i in range(130) if not (np.asarray(base.job_node) == i).any()]
    flip_off = next(i for i in range(130) if not base.node_taints[i])                # PLAIN matches it: a taint takes the bit away
    flip_on = next(i for i in range(130) if base.node_taints[i] == [(9, 1, 1)])      # PLAIN does not: without the taint it does
    drop = sorted([i for i in idle if i not in (flip_off, flip_on)][:2] + [131, 133])   # rows without a running job: resident ones where there are any, and two of the appended
    outs = []
    for L in _libs(lib, hostsim_lib):
        cur, step, tail = copy.copy(wl), 0, tail0
        a = _load(L, base)
        _round(a, base)
        _append_classes(a, classes, c0, 1, k - 1, moved)
        _append_rows(a, cur, tail)

        def check():
            nonlocal step
            res, _ = _same(L, oracle_lib, hostsim_lib, a, cur, tail, cpu=outs[step] if L is not hostsim_lib else None)
            if L is hostsim_lib:
                outs.append(res)
            step += 1
        check()
        # nodes_patch: the bit of PLAIN flips on two nodes
        cur = copy.copy(cur)
        cur.node_taints = [list(t) for t in cur.node_taints]
        cur.node_taints[flip_off] = [(9, 1, 1)]
        cur.node_taints[flip_on] = []
        a.nodes_patch([flip_off, flip_on], taints=[cur.node_taints[flip_off], cur.node_taints[flip_on]])
        assert a.nodes_patch_stats()[2] == 0
        check()
        # nodes_append: five nodes of known types
        cur = copy.copy(cur)
        src = [0, 1, 2, 3, 5]
        cur.node_total = np.concatenate([cur.node_total, cur.node_total[src]])
        cur.node_taints = cur.node_taints + [list(cur.node_taints[i]) for i in src]
        cur.node_labels = list(cur.node_labels) + [list(cur.node_labels[i]) for i in src]
        a.nodes_append(cur.node_total[-5:], index=np.arange(131, 136), taints=cur.node_taints[-5:], labels=cur.node_labels[-5:])
        check()
        # nodes_delete: rows without a running job
        cur = copy.copy(cur)
        keep = np.array([i for i in range(135) if i not in drop])
        new_of = np.full(135, -1, np.int32)
        new_of[keep] = np.arange(len(keep), dtype=np.int32)
        cur.node_total = cur.node_total[keep]
        cur.node_taints = [cur.node_taints[i] for i in keep]
        cur.node_labels = [cur.node_labels[i] for i in keep]
        cur.job_node = np.where(cur.job_node >= 0, new_of[np.maximum(cur.job_node, 0)], -1).astype(np.int32)
        a.nodes_delete(drop)
        check()
        # a shape of a new class in an away priority class: a newly derived class behind the moved ones
        cur, tail2 = _extend(cur, [[1 * Gi, 1000, 2 * Gi, 0]] * 2, cls=c0, pc=1)
        _append_rows(a, cur, tail2)
        sh = a.jobs_append_shape_stats()
        assert sh["reason"] == 0 and sh["added"] == 1 and sh["derived_classes"] == 1, sh
        tail = np.concatenate([tail, tail2])
        check()
        a.close()


# ---------------------------------------------------------------- d. the class bits of the nodes
def _many(k, first):
    """k classes decided by node type, every one textually different: the selector value cycles, the toleration changes with the id"""
    return [([EXISTS9, (9, 0, 100 + first + i, 1)], [(3, (first + i) % 3)] if (first + i) % 4 else [], None) for i in range(k)]


@pytest.mark.parametrize("k", [1, 2, 63])
def test_k_classes_in_one_call_up_to_64(lib, oracle_lib, hostsim_lib, k):
    base = _tbl(130, n_classes=1)
    classes = _many(k, 1)
    full, tail = _rows_of(_with_classes(base, classes), 1 + k - 1, 1)        # rows of the LAST class: bit k
    for L in _libs(lib, hostsim_lib):
        a = _load(L, base)
        _round(a, base)
        _append_classes(a, classes, 1, k, 0, 0)
        _append_rows(a, full, tail)
        _, sta = _same(L, oracle_lib, hostsim_lib, a, full, tail)
        assert sta["fast_iterations"] > 0
        a.close()


def test_two_calls_in_a_row(lib, oracle_lib, hostsim_lib):
    base = _tbl(130)
    first, second = [ONE_TYPE, AFF_GT], [OPENS, NON_INDEXED, PLAIN]
    full, tail = _rows_of(_with_classes(base, first + second), 2, 5)
    a = _load(lib, base)
    _append_classes(a, first, 2, 1, 1, 0)
    _append_classes(a, second, 4, 2, 1, 0)
    _append_rows(a, full, tail)
    _, sta = _same(lib, oracle_lib, hostsim_lib, a, full, tail)
    assert sta["fast_iterations"] > 0
    a.close()


def test_the_65th_class_rebuilds(lib, oracle_lib, hostsim_lib):
    base = _tbl(130, n_classes=64)
    full, tail = _rows_of(_with_classes(base, [ONE_TYPE]), 64, 1)
    a = _load(lib, base)
    _, st0 = _round(a, base)
    assert st0["fast_iterations"] > 0
    assert a.req_classes_append([ONE_TYPE[0]], [ONE_TYPE[1]]) == 64
    st = a.req_classes_append_stats()
    assert st["rebuilt"] == 1 and st["reason"] == 2 and st["added"] == 1 and st["classes"] == 65 and st["by_type"] == 0 and st["on_host"] == 0, st
    _append_rows(a, full, tail)
    _same(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_more_than_64_classes_from_the_start(lib, oracle_lib, hostsim_lib):
    sta = _case(lib, oracle_lib, hostsim_lib, _tbl(130, n_classes=70), [ONE_TYPE, AFF_IN], 1, 1)
    assert sta["fast_iterations"] == 0


# ---------------------------------------------------------------- e. interplay
@pytest.mark.parametrize("warm", [False, True])
def test_warm_and_cold_handles(lib, oracle_lib, hostsim_lib, warm):
    _case(lib, oracle_lib, hostsim_lib, _tbl(257), [PLAIN, AFF_NOT_IN], 1, 1, warm=warm, pcs=(0, 1))


def test_class_append_then_jobs_patch(lib, oracle_lib, hostsim_lib):
    base = _tbl(130)
    full, tail = _rows_of(_with_classes(base, [EVERY]), 2, 1)
    a = _load(lib, base)
    _append_classes(a, [EVERY], 2, 1, 0, 0)
    _append_rows(a, full, tail)
    full = copy.copy(full)
    full.job_node, full.job_run_prio, full.job_run_ts = full.job_node.copy(), full.job_run_prio.copy(), full.job_run_ts.copy()
    j = int(tail[0])
    full.job_node[j], full.job_run_prio[j], full.job_run_ts[j] = 5, 0, 77
    full.queued = [np.array([x for x in q if int(x) != j], dtype=np.int32) for q in full.queued]
    a.jobs_patch([j], [5], 0, 77)
    _same(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_the_rows_of_a_new_class_leave_and_come_back(lib, oracle_lib, hostsim_lib):
    base = _tbl(130)
    full, tail = _rows_of(_with_classes(base, [OPENS]), 2, 1)
    a = _load(lib, base)
    _append_classes(a, [OPENS], 2, 1, 0, 0)
    _append_rows(a, full, tail)
    a.jobs_delete(tail.astype(np.int32))
    assert a.jobs_delete_stats()["shapes_emptied"] == 2
    _append_rows(a, full, tail)
    sh = a.jobs_append_shape_stats()
    assert sh["revived"] == 2 and sh["reason"] == 0, sh
    _same(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_with_the_in_place_switch_off_the_row_append_rebuilds(lib, oracle_lib, hostsim_lib):
    _case(lib, oracle_lib, hostsim_lib, _tbl(130), [ONE_TYPE, AFF_IN], 1, 1, in_place=False)


def test_classes_appended_before_any_node_table(lib, oracle_lib, hostsim_lib):
    base = _tbl(130)
    classes = [ONE_TYPE, AFF_GT]
    full, tail = _rows_of(_with_classes(base, classes), 2, 2)
    a = _load(lib, base, nodes=False)
    assert a.req_classes_append([t for t, _, _ in classes], [s for _, s, _ in classes], [x for _, _, x in classes]) == 2
    st = a.req_classes_append_stats()
    assert st["rebuilt"] == 1 and st["reason"] == 1 and st["added"] == 2 and st["classes"] == 4, st
    _nodes(a, base)
    _append_rows(a, full, tail)
    _same(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.close()


def test_no_classes_performs_the_resets_only(lib, oracle_lib, hostsim_lib):
    base = _tbl(130)
    a = _load(lib, base)
    _round(a, base)
    assert a.req_classes_append([]) == 2
    st = a.req_classes_append_stats()
    assert st == dict(added=0, by_type=0, on_host=0, moved=0, rebuilt=0, reason=0, classes=2, classes_ext=2), st
    _same(lib, oracle_lib, hostsim_lib, a, base, np.arange(base.num_jobs - 4, base.num_jobs))
    a.close()


def test_statistics_are_zero_after_jobs_set(lib):
    base = _tbl(65)
    a = _load(lib, base)
    _append_classes(a, [ONE_TYPE], 2, 1, 0, 0)
    _jobs(a, base)
    assert set(a.req_classes_append_stats().values()) == {0}
    a.close()


# ---------------------------------------------------------------- f. refusals
def _raw(s, **fields):
    """asched_req_classes_append with exactly these fields of the struct set -> return code"""
    c = CReqClasses()
    keep = []
    for name, val in fields.items():
        if name == "n":
            c.n = val
            continue
        arr = np.ascontiguousarray(val, dtype=np.uint8 if name == "has_affinity" else np.int32)
        keep.append(arr)
        setattr(c, name, arr.ctypes.data_as(C.POINTER(C.c_uint8 if name == "has_affinity" else C.c_int32)))
    return s.lib.req_classes_append(s.h, C.byref(c))


REFUSALS = {
    "n_below_zero": (dict(n=-1), ERR_INVALID),
    "toleration_values_without_offsets": (dict(n=1, tol_key=[9], tol_op=[1], tol_value=[0], tol_effect=[0]), ERR_INVALID),
    "selector_values_without_offsets": (dict(n=1, sel_key=[3], sel_value=[1]), ERR_INVALID),
    "toleration_offsets_not_ascending": (dict(n=2, tol_off=[0, 2, 1], tol_key=[9, 9], tol_op=[1, 1], tol_value=[0, 0], tol_effect=[0, 0]), ERR_INVALID),
    "selector_offsets_not_ascending": (dict(n=2, sel_off=[1, 0, 1], sel_key=[3], sel_value=[1]), ERR_INVALID),
    "affinity_without_the_term_arrays": (dict(n=1, has_affinity=[1]), ERR_INVALID),
    "affinity_term_offsets_not_ascending": (dict(n=2, has_affinity=[1, 1], aff_term_off=[0, 1, 0], aff_expr_off=[0, 0]), ERR_INVALID),
    "unknown_affinity_operator": (dict(n=1, has_affinity=[1], aff_term_off=[0, 1], aff_expr_off=[0, 1], aff_expr_key=[3], aff_expr_op=[17], aff_value_off=[0, 0], aff_values=[0]), ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_leave_the_handle_as_it_was(lib, name):
    base = _tbl(65, n_jobs=120)
    tail = np.arange(base.num_jobs - 4, base.num_jobs)
    a = _load(lib, base)
    before = _view(a, base, tail)
    fields, code = REFUSALS[name]
    assert _raw(a, **fields) == code
    assert a.req_classes_append_stats()["added"] == 0
    assert _view(a, base, tail) == before
    with pytest.raises(SchedError):                        # and no class joined: a row of class 2 is still refused
        a.jobs_append([[1 * Gi, 1000, 1 * Gi, 0]], req_class=[2])
    a.close()


def test_refusals_without_arguments_or_a_job_table(lib):
    base = _tbl(65, n_jobs=120)
    tail = np.arange(base.num_jobs - 4, base.num_jobs)
    a = _load(lib, base)
    before = _view(a, base, tail)
    assert a.lib.req_classes_append(a.h, None) == ERR_INVALID
    assert _view(a, base, tail) == before
    a.close()
    s = Scheduler(lib, base.config)
    _nodes(s, base)
    with pytest.raises(SchedError) as e:
        s.req_classes_append([[]])
    assert e.value.code == ERR_INVALID
    _jobs(s, base)                                          # the handle goes on as a fresh one
    assert _view(s, base, tail) == before
    s.close()
