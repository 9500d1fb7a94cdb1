"""asched_shapes_compact: the scheduling-key shapes no resident row names (asched_jobs_delete emptied them), the fit shapes only they mapped to and, on request, the
requirement classes only they named leave the resident tables (armada_amd/csrc/kernels_shapes_compact.h) instead of asched_jobs_set of the whole job table.  The
contract: the handle is what jobs_set of the same job table (with the class list reduced to the live classes, where classes were retired) would have left.

Every equivalence case asserts the exact statistics — shapes, fit shapes and classes retired, rebuilt, reason — so a silent fallback does not pass, and compares the
handle with a fresh handle given the same table: scheduling_order, the first fit of every row at every priority level, the node types matching rows, a submit check, a
round (also against the oracle's round), the unfeasible keys the round left, the fair shares bit for bit and the number of fast iterations.
a. the cliff this closes; b. edges of the row pass and of the map staging; c. edges of the mask gather; d. classes; e. interplay on the compacted handle;
f. COUNT_ONLY; g. resets and refusals; h. the simulator drivers.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library, whose answers must also equal the CPU build's.  The staging capacity of the row
pass (SC_LDS_CAP) is 8 in tests/hostsim/libhostsim_sc8.so and 1024 in the product: on the GPU a table of that many shapes has more than SMAX fit shapes and therefore no
job records, so there the capacity edge covers the shape ids of the rows and the CPU build covers the records on both sides of the capacity."""
import copy
import fcntl
import os
import subprocess

import numpy as np
import pytest

import scenario
import test_z_req_classes_append as rc
from armada_amd import simulator_input as SI
from armada_amd import workloads as W
from armada_amd.binding import Library, SchedError, Scheduler
from test_z_jobs_append import _append_tail, _permuted, _records, _round, _shape_keys
from test_z_jobs_append_shapes import _base, _extend, _sim_with_a_shape_per_cycle, _view
from test_z_jobs_reprioritise import _restated_queued

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
SMAX = 256                                 # armada_amd/csrc/dev.h
SC_LDS_CAP = 1024                          # armada_amd/csrc/kernels_shapes_compact.h
Gi = W.Gi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


@pytest.fixture(scope="session")
def sc8_lib():
    """the CPU build with room for 8 entries of each map in the staging arrays of the row pass"""
    here = os.path.join(ROOT, "tests", "hostsim")
    with open(os.path.join(here, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", here, "-f", "sc8.mk"])
    return Library(os.path.join(here, "libhostsim_sc8.so"), "asched_")


# ---------------------------------------------------------------- loading and comparing
def _up_nodes(s, wl):
    s.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank, node_type_override=getattr(wl, "type_override", None))


def _set_jobs(s, wl):
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, queue_priority=getattr(wl, "qprio", None), submit_time=wl.job_submit, node=wl.job_node,
               scheduled_at_priority=wl.job_run_prio, run_timestamp=wl.job_run_ts, gang_id=wl.job_gang, gang_cardinality=wl.job_gang_card, req_class=wl.job_req_class,
               class_tolerations=wl.class_tolerations, class_selectors=wl.class_selectors, class_affinities=getattr(wl, "class_affinities", None), away=wl.job_away)


def _ld(L, wl, nodes=True):
    s = Scheduler(L, wl.config)
    s.set_label_value_ints(rc.INTS)
    if nodes:
        _up_nodes(s, wl)
    _set_jobs(s, wl)
    return s


def _answers(s, wl, tail):
    v = _view(s, wl, tail)
    r, st = _round(s, wl)
    return v, r, st, [s.job_key_unfeasible(int(j)) for j in tail]


def _same(L, oracle_lib, cpu_lib, a, wl, tail=None, cpu=None):
    """handle `a` against a fresh handle of the table `wl`, the oracle's round and — on the HIP library — the CPU build's answers"""
    tail = np.arange(max(wl.num_jobs - 8, 0), wl.num_jobs) if tail is None else tail
    f = _ld(L, wl)
    va, ra, sta, ua = _answers(a, wl, tail)
    vf, rf, stf, uf = _answers(f, wl, tail)
    f.close()
    assert va == vf
    o = _ld(oracle_lib, wl)
    ro, _ = _round(o, wl)
    o.close()
    scenario.assert_same_round(rf, ra)
    scenario.assert_same_round(ro, ra)
    assert ua == uf
    assert ra.fair_share.tobytes() == rf.fair_share.tobytes() == ro.fair_share.tobytes()
    assert sta["fast_iterations"] == stf["fast_iterations"], "the compacted handle did not run the fresh handle's fast iterations"
    if cpu is None and L is not cpu_lib:
        c = _ld(cpu_lib, wl)
        vc, rcpu, _, uc = _answers(c, wl, tail)
        c.close()
        cpu = (vc, rcpu, uc)
    if cpu is not None:
        assert va == cpu[0] and ua == cpu[2]
        scenario.assert_same_round(cpu[1], ra)
    return (va, ra, ua), sta


def _new_reqs(k, first=0):
    """k request vectors no table of this file has, each a fit shape of its own (they differ in a non-indexed column)"""
    return np.array([[2 * Gi, 1000, (300 + first + i) * Gi, 0] for i in range(k)], dtype=np.int64)


def _kill(s, wl, req, cls=None, pc=None, in_place=True):
    """rows of new shapes are appended and deleted again: the table is `wl` once more, their shapes are dead"""
    full, tail = _extend(wl, req, cls=cls, pc=pc)
    s.set_append_in_place(in_place)
    _append_tail(s, full, tail)
    s.jobs_delete(tail.astype(np.int32))
    assert s.jobs_delete_stats()["shapes_emptied"] == len({(int(full.job_req_class[j]) if full.job_req_class is not None else 0, int(full.job_pc[j])) + tuple(full.job_req[j]) for j in tail})


def _compact(s, shapes, fit, ncls=0, rebuilt=0, reason=0, **kw):
    """shapes_compact(**kw) with the exact statistics: shapes, fit shapes and classes retired, rebuilt, reason -> (the class map or None, the statistics)"""
    got = s.shapes_compact(**kw)
    st = s.shapes_compact_stats()
    assert (st["shapes_retired"], st["fit_retired"], st["classes_retired"], st["rebuilt"], st["reason"]) == (shapes, fit, ncls, rebuilt, reason), st
    return got, st


def _libs(lib, cpu_lib):
    return [lib] if lib is cpu_lib else [cpu_lib, lib]


# ---------------------------------------------------------------- a. the cliff
def _cliff_table():
    return W.small_random(n_nodes=130, n_jobs=240, n_queues=3, seed=31, occupied=0.5, gangs=0)


@pytest.mark.parametrize("cycles", [6, 3])
def test_dead_fit_shapes_walk_a_resident_handle_over_smax_and_compact_brings_it_back(lib, oracle_lib, hostsim_lib, cycles):
    """six cycles of 50 new fit shapes appended and deleted: F = 383, the round runs no fast iteration; shapes_compact rebuilds (reason 2), F = 83 and the fast
    iterations are the fresh handle's.  Three cycles stop at F = 233 <= SMAX: the in-place path, 150 shapes retired"""
    wl = _cliff_table()
    a = W.load(lib, wl)
    for c in range(cycles):
        _kill(a, wl, _new_reqs(50, 50 * c))
    _, st0 = _round(a, wl)
    a.shapes_compact(count_only=True)
    before = a.shapes_compact_stats()
    assert before["fit_shapes"] == 83 + 50 * cycles and before["fit_retired"] == 50 * cycles, before
    if cycles == 6:
        assert st0["fast_iterations"] == 0, st0
        _, st = _compact(a, 300, 300, rebuilt=1, reason=2)
    else:
        assert st0["fast_iterations"] > 0, st0
        _, st = _compact(a, 150, 150)
    assert st["fit_shapes"] == 83 and st["shapes"] == before["shapes"] - 50 * cycles, st
    _, sta = _same(lib, oracle_lib, hostsim_lib, a, wl)
    assert sta["fast_iterations"] > 0
    if lib is hostsim_lib:
        assert sta["fast_iterations"] == 222, sta
    a.close()


# ---------------------------------------------------------------- b. edges of the row pass
VEC = np.array([[1 * Gi, 1000, 1 * Gi, 0], [2 * Gi, 2000, 3 * Gi, 0]], dtype=np.int64)      # R = 4, two request vectors


def _interleaved(M, n_dead=None, n_nodes=20):
    """a table of M queued rows over two request vectors (a few live shapes: vector x priority class) and the table jobs_set is first given: a row of a shape of its own
    in front of the first row of every live shape and one behind the last row, so that in shape-id order the first, the last and every other shape are to die.
    n_dead: that many rows to die instead (the extra ones behind the table) -> (base, the table with the rows to die, their row ids)"""
    base = W.small_random(n_nodes=n_nodes, n_jobs=M, n_queues=3, seed=5, occupied=0.0, gangs=0)
    assert (np.asarray(base.job_node) < 0).all()
    base.job_req = VEC[np.arange(M) % 2].copy()
    keys = _shape_keys(base, range(M))
    first = sorted({k: j for j, k in reversed(list(enumerate(keys)))}.values())
    nd = len(first) + 1 if n_dead is None else n_dead
    full, dead = _extend(base, _new_reqs(nd))
    perm, d = [], 0
    for j in range(M):
        if j in first and d < nd - 1:
            perm.append(int(dead[d])); d += 1
        perm.append(j)
    perm += [int(x) for x in dead[d:]]
    full = _permuted(full, np.array(perm, dtype=np.int64))
    rows = np.array([i for i, p in enumerate(perm) if p >= M], dtype=np.int32)
    return base, full, rows, len(first)


def _interleaved_case(L, oracle_lib, cpu_lib, M, n_dead=None, cpu=None):
    base, full, rows, live = _interleaved(M, n_dead)
    a = W.load(L, full)
    _round(a, full)
    a.jobs_delete(rows)
    _, st = _compact(a, len(rows), len(rows))
    assert st["shapes"] == live
    res, sta = _same(L, oracle_lib, cpu_lib, a, base, cpu=cpu)
    assert sta["fast_iterations"] > 0
    a.close()
    return res, live + len(rows)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257])
def test_row_pass_at_the_block_edges_with_dead_shapes_between_live_ones(lib, oracle_lib, hostsim_lib, M):
    _interleaved_case(lib, oracle_lib, hostsim_lib, M)


@pytest.mark.parametrize("s0", [7, 8, 9])
def test_maps_around_the_staging_capacity_on_the_cpu_build(sc8_lib, oracle_lib, s0):
    """capacity - 1, capacity, capacity + 1 entries of the shape map in the build whose staging arrays hold 8: the staged and the global branch, records included"""
    base, _, _, live = _interleaved(65)
    _, total = _interleaved_case(sc8_lib, oracle_lib, sc8_lib, 65, n_dead=s0 - live)
    assert total == s0


@pytest.mark.gpu
@pytest.mark.parametrize("s0", [SC_LDS_CAP - 1, SC_LDS_CAP, SC_LDS_CAP + 1])
def test_maps_around_the_staging_capacity_on_the_gpu(hip_lib, oracle_lib, hostsim_lib, s0):
    """the smallest tables that cross the shipped capacity: that many shapes are more than SMAX fit shapes, so the handle has no job records before the call and the
    compaction brings the fast structure back (reason 2); the row pass remaps the shape ids through the staged (s0 <= capacity) and the global branch"""
    base, full, rows, live = _interleaved(65, n_dead=s0 - 6)
    assert live == 6
    a = W.load(hip_lib, full)
    a.jobs_delete(rows)
    _, st = _compact(a, len(rows), len(rows), rebuilt=1, reason=2)
    assert st["shapes"] == live
    _same(hip_lib, oracle_lib, hostsim_lib, a, base)
    a.close()


# ---------------------------------------------------------------- c. edges of the mask gather
@pytest.mark.parametrize("n", rc.NODES)
def test_mask_rows_and_away_rows_gathered_at_the_word_edges(lib, oracle_lib, hostsim_lib, n):
    """away node types on: the dead shapes of requirement class 2 had away rows of their own and were the only ones to derive the away classes of class 2"""
    base = _base(n, n_jobs=200, away=True, seed=33)
    a = W.load(lib, base)
    _round(a, base)
    a.shapes_compact(count_only=True)
    d0 = a.shapes_compact_stats()["derived_classes"]
    req = _new_reqs(4)
    _kill(a, base, np.concatenate([req, req[:2]]), cls=2, pc=[1, 2, 1, 2, 0, 0])
    a.shapes_compact(count_only=True)
    assert a.shapes_compact_stats()["derived_classes"] == d0 + 2
    _, st = _compact(a, 6, 4)          # (the two priority classes of a request share its fit shape)
    assert st["derived_classes"] == d0, st
    _same(lib, oracle_lib, hostsim_lib, a, base)
    a.close()


def test_a_dead_shape_was_the_first_to_derive_an_away_class_a_live_shape_derives_too(lib, oracle_lib, hostsim_lib):
    """row 0 (class 2, an away priority class) derives (class 2, well-known type 0) before any shape of class 0 derives its class; the last row derives it again.  With
    row 0 gone the derived classes are numbered in another order: the class mask is gathered through the source table"""
    base = _base(130, away=True, seed=33)
    assert (base.job_pc[base.job_req_class == 0] > 0).any() and (base.job_pc[base.job_req_class == 2] == 0).all()
    full, tail = _extend(base, _new_reqs(2), cls=2, pc=1, queue=[0, 1])
    m = base.num_jobs
    first = _permuted(full, np.array([m] + list(range(m)) + [m + 1], dtype=np.int64))
    want, _ = _extend(base, _new_reqs(2)[1:], cls=2, pc=1, queue=[1])
    want.job_submit = want.job_submit.copy()
    want.job_submit[-1] = full.job_submit[-1]              # (the surviving row as it was submitted: behind the row that left)
    a = W.load(lib, first)
    _round(a, first)
    a.jobs_delete(np.array([0], dtype=np.int32))
    a.shapes_compact(count_only=True)
    d0 = a.shapes_compact_stats()["derived_classes"]
    _, st = _compact(a, 1, 1)
    assert st["derived_classes"] == d0, st
    _same(lib, oracle_lib, hostsim_lib, a, want)
    a.close()


# ---------------------------------------------------------------- d. classes
def _class_table(n_classes, live, aff=None, n=130):
    """rc._tbl with n_classes classes of which `live` have rows: the running and the gang rows take live[0] (given the empty selector), the queued single rows go
    round the live classes.  aff: {class: required node affinity}"""
    wl = rc._tbl(n, n_classes=n_classes)
    wl.class_selectors = [list(x) for x in wl.class_selectors]
    wl.class_selectors[live[0]] = []
    cls = np.full(wl.num_jobs, live[0], np.int32)
    free = np.nonzero((np.asarray(wl.job_node) < 0) & (np.asarray(wl.job_gang) < 0))[0]
    cls[free] = np.asarray(live, np.int32)[np.arange(len(free)) % len(live)]
    wl.job_req_class = cls
    assert set(int(c) for c in cls) == set(live)
    if aff:
        wl.class_affinities = [aff.get(c) for c in range(n_classes)]
    return wl


def _reduced(wl, cmap):
    """the table a fresh handle is given after classes were retired: the live classes only, req_class renumbered"""
    w = copy.copy(wl)
    keep = [c for c in range(len(cmap)) if cmap[c] >= 0]
    assert [int(cmap[c]) for c in keep] == list(range(len(keep)))
    w.class_tolerations = [wl.class_tolerations[c] for c in keep]
    w.class_selectors = [wl.class_selectors[c] for c in keep]
    if getattr(wl, "class_affinities", None) is not None:
        w.class_affinities = [wl.class_affinities[c] for c in keep]
        if all(x is None for x in w.class_affinities):
            w.class_affinities = None
    w.job_req_class = np.asarray(cmap, np.int32)[wl.job_req_class]
    return w


def test_65_classes_of_which_10_are_dead_rebuild_and_the_fast_iterations_come_back(lib, oracle_lib, hostsim_lib):
    live = list(range(2, 57))
    wl = _class_table(65, live)
    a = _ld(lib, wl)
    _, st0 = _round(a, wl)
    assert st0["fast_iterations"] == 0
    cmap, _ = _compact(a, 0, 0, ncls=10, rebuilt=1, reason=3, classes=True, want_map=True)
    assert cmap.tolist() == [-1, -1] + list(range(55)) + [-1] * 8
    _, sta = _same(lib, oracle_lib, hostsim_lib, a, _reduced(wl, cmap))
    assert sta["fast_iterations"] > 0
    a.close()


def test_70_classes_of_which_3_are_dead_stay_over_the_limit_and_are_compacted_in_place(lib, oracle_lib, hostsim_lib):
    """C goes from 70 to 67: buildFast's predicate stays false, so the masks and tables are compacted in place on a handle without the fast structure"""
    wl = _class_table(70, list(range(2, 69)))
    a = _ld(lib, wl)
    _round(a, wl)
    _kill(a, wl, _new_reqs(4), cls=[0, 1, 69, 5])
    cmap, _ = _compact(a, 4, 4, ncls=3, classes=True, want_map=True)
    assert cmap.tolist() == [-1, -1] + list(range(67)) + [-1]
    _, sta = _same(lib, oracle_lib, hostsim_lib, a, _reduced(wl, cmap))
    assert sta["fast_iterations"] == 0
    a.close()


def test_dead_classes_at_the_bit_edges_and_new_classes_behind_the_compacted_ones(lib, oracle_lib, hostsim_lib):
    """classes 0, 1, 62 and 63 of 64 are dead: every node's class word is bit-compacted in place, the records' classes remapped; classes with affinities move.  Then
    a class append and rows that name the new id"""
    live = list(range(2, 62))
    wl = _class_table(64, live, aff={5: rc.AFF_IN[2], 61: rc.AFF_GT[2]})
    out = None
    for L in _libs(lib, hostsim_lib):
        a = _ld(L, wl)
        _, st0 = _round(a, wl)
        assert st0["fast_iterations"] > 0
        cmap, _ = _compact(a, 0, 0, ncls=4, classes=True, want_map=True)
        assert cmap.tolist() == [-1, -1] + list(range(60)) + [-1, -1]
        red = _reduced(wl, cmap)
        res, sta = _same(L, oracle_lib, hostsim_lib, a, red, cpu=out)
        out = out or res
        assert sta["fast_iterations"] > 0
        full, tail = rc._rows_of(rc._with_classes(red, [rc.ONE_TYPE, rc.AFF_NOT_IN]), 60, 2)
        assert a.req_classes_append([rc.ONE_TYPE[0], rc.AFF_NOT_IN[0]], [rc.ONE_TYPE[1], rc.AFF_NOT_IN[1]], [rc.ONE_TYPE[2], rc.AFF_NOT_IN[2]]) == 60
        a.set_append_in_place(True)
        assert _append_tail(a, full, tail)["rebuilt"] == 0
        _same(L, oracle_lib, hostsim_lib, a, full, tail)
        a.close()


def test_without_the_flag_classes_and_ids_stay_and_with_it_a_class_only_dead_shapes_name_goes(lib, oracle_lib, hostsim_lib):
    live = list(range(2, 62))
    wl = _class_table(64, live)
    a = _ld(lib, wl)
    _round(a, wl)
    _kill(a, wl, _new_reqs(3), cls=[62, 62, 1])            # classes 62 and 1 are named by dead shapes only
    cmap, st = _compact(a, 3, 3)                           # flag off: the shapes go, every class stays
    assert cmap is None and st["classes_retired"] == 0
    _same(lib, oracle_lib, hostsim_lib, a, wl)
    full, tail = _extend(wl, _new_reqs(1, 7), cls=63)      # (class 63 is still class 63)
    a.set_append_in_place(True)
    _append_tail(a, full, tail)
    _same(lib, oracle_lib, hostsim_lib, a, full, tail)
    a.jobs_delete(tail.astype(np.int32))
    cmap, _ = _compact(a, 1, 1, ncls=4, classes=True, want_map=True)
    _same(lib, oracle_lib, hostsim_lib, a, _reduced(wl, cmap))
    a.close()


# ---------------------------------------------------------------- e. interplay on the compacted handle
def test_the_resident_calls_on_a_compacted_handle(lib, oracle_lib, hostsim_lib):
    """after a compact with class retirement: jobs_append in place (a new shape and a retired one, which is new again), jobs_patch, jobs_reprioritise, nodes_patch of a
    taint a remapped class reads, nodes_append, nodes_delete, jobs_append with the switch off, jobs_delete, a compact of the shape that left and a second compact in a row that retires nothing"""
    live = [2, 3, 5]
    wl = _class_table(6, live, n=130)
    wl.class_tolerations = [[] if c == 3 else list(t) for c, t in enumerate(wl.class_tolerations)]      # class 3 (-> 1) tolerates nothing: the taint on key 9 closes a node to it
    wl.class_selectors[3] = []
    outs, step = [], 0
    for L in _libs(lib, hostsim_lib):
        step = 0
        a = _ld(L, wl)
        _round(a, wl)
        _kill(a, wl, _new_reqs(5), cls=[0, 1, 4, 2, 3])
        cmap, _ = _compact(a, 5, 5, ncls=3, classes=True, want_map=True)
        assert cmap.tolist() == [-1, -1, 0, 1, -1, 2]
        cur = _reduced(wl, cmap)
        tail = None

        def check():
            nonlocal step
            res, _ = _same(L, oracle_lib, hostsim_lib, a, cur, tail, cpu=outs[step] if L is not hostsim_lib else None)
            if L is hostsim_lib:
                outs.append(res)
            step += 1
        check()
        # jobs_append in place: a shape the compact retired (new again: added, not revived) and one never seen
        cur, tail = _extend(cur, np.concatenate([_new_reqs(1, 3), _new_reqs(1, 40)]), cls=[0, 1])
        a.set_append_in_place(True)
        assert _append_tail(a, cur, tail)["rebuilt"] == 0
        sh = a.jobs_append_shape_stats()
        assert sh["added"] == 2 and sh["revived"] == 0 and sh["reason"] == 0, sh
        check()
        # jobs_patch: a new row runs
        cur = copy.copy(cur)
        cur.job_node, cur.job_run_prio, cur.job_run_ts = cur.job_node.copy(), cur.job_run_prio.copy(), cur.job_run_ts.copy()
        j = int(tail[0])
        cur.job_node[j], cur.job_run_prio[j], cur.job_run_ts[j] = 5, 0, 77
        cur.queued = [np.array([x for x in q if int(x) != j], dtype=np.int32) for q in cur.queued]
        a.jobs_patch([j], [5], 0, 77)
        check()
        # jobs_reprioritise: the other new row goes in front of its queue's rows of the same priority class
        cur = copy.copy(cur)
        cur.qprio = np.full(cur.num_jobs, 5, np.uint32)
        a.jobs_reprioritise(np.arange(cur.num_jobs, dtype=np.int32), 5)
        cur.qprio[int(tail[1])] = 1
        a.jobs_reprioritise([int(tail[1])], 1)
        cur.queued = _restated_queued(cur, cur.qprio)
        check()
        # nodes_patch: class 1 (was 3) loses node 1 and gains node 0 by the taint on key 9
        cur = copy.copy(cur)
        cur.node_taints = [list(t) for t in cur.node_taints]
        off = next(i for i in range(1, 130) if not cur.node_taints[i])              # (the running rows are of class 0, which tolerates the taint)
        on = next(i for i in range(0, 130, 4) if cur.node_taints[i] == [(9, 1, 1)])
        cur.node_taints[off] = [(9, 1, 1)]
        cur.node_taints[on] = []
        a.nodes_patch([off, on], taints=[cur.node_taints[off], cur.node_taints[on]])
        assert a.nodes_patch_stats()[2] == 0
        check()
        # nodes_append, nodes_delete
        cur = copy.copy(cur)
        src = [0, 1, 2, 3, 5]
        cur.node_total = np.concatenate([cur.node_total, cur.node_total[src]])
        cur.node_taints = cur.node_taints + [list(cur.node_taints[i]) for i in src]
        cur.node_labels = list(cur.node_labels) + [list(cur.node_labels[i]) for i in src]
        a.nodes_append(cur.node_total[-5:], index=np.arange(131, 136), taints=cur.node_taints[-5:], labels=cur.node_labels[-5:])
        check()
        cur = copy.copy(cur)
        drop = [i for i in range(135) if not (cur.job_node == i).any()][3:40:6]
        keep = np.array([i for i in range(135) if i not in drop])
        new_of = np.full(135, -1, np.int32)
        new_of[keep] = np.arange(len(keep), dtype=np.int32)
        cur.node_total = cur.node_total[keep]
        cur.node_taints = [cur.node_taints[i] for i in keep]
        cur.node_labels = [cur.node_labels[i] for i in keep]
        cur.job_node = np.where(cur.job_node >= 0, new_of[np.maximum(cur.job_node, 0)], -1).astype(np.int32)
        a.nodes_delete(drop)
        check()
        # with the switch off a new shape rebuilds; then it leaves again and a second compact in a row retires nothing
        prev = cur
        cur, tail = _extend(cur, _new_reqs(1, 41), cls=2)
        cur.qprio = np.concatenate([cur.qprio, np.zeros(1, np.uint32)])
        cur.queued = _restated_queued(cur, cur.qprio)
        a.set_append_in_place(False)
        assert _append_tail(a, cur, tail)["rebuilt"] == 1
        check()
        a.jobs_delete(tail.astype(np.int32))                 # jobs_delete on the compacted handle: the row's shape is dead again
        assert a.jobs_delete_stats()["shapes_emptied"] == 1
        cur, tail = prev, None
        check()
        _compact(a, 1, 1, classes=True)
        check()
        _compact(a, 0, 0, classes=True)
        check()
        a.close()


def test_a_compact_before_any_node_table_compacts_the_mirrors_and_nodes_upsert_builds_the_rest(lib, oracle_lib, hostsim_lib):
    base, full, rows, live = _interleaved(65)
    a = _ld(lib, full, nodes=False)
    a.jobs_delete(rows)
    _, st = _compact(a, len(rows), 0, rebuilt=1, reason=1)
    assert st["shapes"] == live and st["fit_shapes"] == 0
    _up_nodes(a, base)
    _same(lib, oracle_lib, hostsim_lib, a, base)
    a.close()


# ---------------------------------------------------------------- f. COUNT_ONLY
def test_count_only_changes_nothing_and_says_what_the_call_retires(lib):
    wl = _class_table(6, [2, 3, 5], n=65)
    a = _ld(lib, wl)
    _kill(a, wl, _new_reqs(3), cls=[0, 4, 2])
    tail = np.arange(wl.num_jobs - 8, wl.num_jobs)
    v0 = _view(a, wl, tail)
    a.shapes_compact(classes=True, count_only=True)
    c = a.shapes_compact_stats()
    assert (c["shapes_retired"], c["fit_retired"], c["classes_retired"], c["rebuilt"], c["reason"]) == (3, 3, 3, 0, 0), c
    assert _view(a, wl, tail) == v0
    a.shapes_compact(count_only=True)
    assert a.shapes_compact_stats()["classes_retired"] == 0
    full, t2 = _extend(wl, _new_reqs(1, 9), cls=4)          # class 4 is still there: nothing was retired
    a.set_append_in_place(True)
    _append_tail(a, full, t2)
    a.jobs_delete(t2.astype(np.int32))
    a.shapes_compact(classes=True)
    st = a.shapes_compact_stats()
    assert (st["shapes_retired"], st["fit_retired"], st["classes_retired"]) == (4, 4, 3), st
    assert st["shapes"] == c["shapes"] - 3 and st["fit_shapes"] == c["fit_shapes"] - 3
    a.close()


# ---------------------------------------------------------------- g. resets and refusals
def test_nothing_dead_performs_the_resets_only(lib, oracle_lib, hostsim_lib):
    wl = _cliff_table()
    a = W.load(lib, wl)
    _round(a, wl)
    _, st = _compact(a, 0, 0)
    assert st["shapes"] > 0 and st["fit_shapes"] == 83
    _, sta = _same(lib, oracle_lib, hostsim_lib, a, wl)
    assert sta["fast_iterations"] > 0
    a.close()


def test_statistics_are_zero_after_jobs_set(lib):
    base, full, rows, _ = _interleaved(65)
    a = W.load(lib, full)
    a.jobs_delete(rows)
    _compact(a, len(rows), len(rows))
    _set_jobs(a, base)
    assert set(a.shapes_compact_stats().values()) == {0}
    a.close()


def test_refusals_leave_the_handle_as_it_was(lib):
    base, full, rows, _ = _interleaved(65)
    s = Scheduler(lib, full.config)
    with pytest.raises(SchedError) as e:          # no job table
        s.shapes_compact()
    assert e.value.code == ERR_INVALID
    s.close()
    a = W.load(lib, full)
    a.jobs_delete(rows)
    tail = np.arange(base.num_jobs - 8, base.num_jobs)
    v0 = _view(a, base, tail)
    assert a.lib.shapes_compact(a.h, 4, None) == ERR_INVALID and a.lib.shapes_compact(a.h, -1, None) == ERR_INVALID      # unknown flag bits
    a.shapes_compact(count_only=True)
    assert a.shapes_compact_stats()["shapes_retired"] == len(rows)
    assert _view(a, base, tail) == v0
    a.close()
    e0 = W.small_random(n_nodes=8, n_jobs=20, n_queues=2, seed=3, occupied=0.0, gangs=0)
    z = W.load(lib, e0)
    z.jobs_set(np.zeros((0, 4), np.int64))        # a table with no rows: every shape is dead
    assert z.lib.shapes_compact(z.h, 0, None) == ERR_UNSUPPORTED
    z.close()
    m = W.load(lib, e0)
    m.jobs_set(e0.job_req, queue=e0.job_queue, pc=e0.job_pc, bid_price=np.ones(e0.num_jobs))       # a market-ordered job set
    assert m.lib.shapes_compact(m.h, 0, None) == ERR_UNSUPPORTED
    m.close()


def test_library_without_the_entry_point_says_so(oracle_lib):
    base = rc._tbl(8, n_jobs=20)
    o = rc._load(oracle_lib, base)
    with pytest.raises(SchedError) as e:
        o.shapes_compact()
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(SchedError):
        o.shapes_compact_stats()
    o.close()


# ---------------------------------------------------------------- h. the simulator drivers
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("classes", [False, True])
def test_retiring_cycles_equal_their_rebuilt_twin_and_the_oracle(lib, oracle_lib, every, classes):
    """eight cycles of 40 arrivals, a new shape (and, with classes, a new class) in every cycle, jobs that finish after a cycle and a half: the deletes empty the shapes
    of the earlier cycles and every `every` cycles the compact retires them"""
    sim = _sim_with_a_shape_per_cycle(40, 1000)
    got = SI.run_cycles_retiring(lib, sim, 40, every=every, classes=classes, max_cycles=8)
    twin = SI.run_cycles_retiring_rebuilt(lib, sim, 40, every=every, classes=classes, max_cycles=8)
    ref = SI.run_cycles_retiring_rebuilt(oracle_lib, sim, 40, every=every, classes=classes, max_cycles=8)
    assert len(got) == 8 and sum(len(c["scheduled"]) for c in got) > 0
    assert _records(got) == _records(twin) == _records(ref)
    last = got[-1]
    assert last["compacts"] == 7 // every and last["shapes_retired"] >= 2 and last["appends_rebuilt"] == 0, last
    assert last["classes_retired"] == (last["shapes_retired"] if classes else 0), last
