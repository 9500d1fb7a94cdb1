"""Who preempted each job of a round, and by which kind of preemption: asched_round_preemption_causes / asched_preemption_join
(PopulatePreemptionDescriptions, scheduling/preemption_description.go:21-81, with the PreemptionDetails of nodedb.go:1034, 514-520 and gang_scheduler.go:268-273).

a. the seven cases of TestPopulatePreemptionDescriptions (tests/golden/preemption_description_cases.json) through preemption_join;
b. preemption_join on synthetic lists against a numpy restatement (a stable sort by node of the URGENCY entries + the reference's order of tests), at the sizes
   where the count / scan / scatter / rank passes take another turn (armada_amd/csrc/kernels_preempt_join.h);
c. the reference's pins that test_z_gang_preemption_marks.py restates without the preemptor, now with it;
d. full rounds: what follows from the oracle's result lists (URGENCY / UNKNOWN / UNKNOWN_GANG records and their candidate slices) is compared record by record; a
   FAIRSHARE / OPTIMISER record, which the oracle does not deliver, is checked for the properties the reference guarantees;
e. a two-word-key round, a market-driven round and an optimiser round (the recording in the other two round kernels);
f. refusals.
Two properties of (d) hold in a narrower form than "a preemptor in the scheduled list has method FAIRSHARE / is in the list when nothing was evicted in phase 3"
(check_round says where): a fair-share preemptor that the oversubscribed evictor evicted again and the second pass put back on its node comes out with method
RESCHEDULED — 11 of the 409 fair-share records of the 24 small rounds, all in rounds with phase-3 evictions, all still on the victim's node — and a queued job the
optimiser placed and later preempted for another one is in neither result list (pqs.go:232-249) although its victims name it.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library — there the records must also equal the CPU build's, byte for byte."""
import copy
import json
import os
import sys

import numpy as np
import pytest

import scenario
from armada_amd import workloads as W
from armada_amd.binding import Config, SchedError, Scheduler

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gofixtures as F  # noqa: E402

UNKNOWN, UNKNOWN_GANG, FAIRSHARE, URGENCY, OPTIMISER = 1, 2, 3, 4, 5
M_RESCHEDULED, M_FAIRSHARE, M_URGENCY, M_OPTIMISER = 1, 3, 4, 6
ERR_INVALID = -1
SIB_OPTIMISER = -2
WG = 256          # workgroup size of the join's kernels
TILE = 4 * WG     # counters per tile of its scan

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preemption_description_cases.json")))


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def libs(request):
    """(library under test, CPU build to compare its records with or None)"""
    hs = request.getfixturevalue("hostsim_lib")
    return (hs, None) if request.param == "hostsim" else (request.getfixturevalue("hip_lib"), hs)


_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for s in _handles.values():
        s.close()
    _handles.clear()


def _handle(lib, n):
    """a handle with n nodes and nothing else: all preemption_join needs"""
    key = (id(lib), n)
    if key not in _handles:
        cfg = Config(num_resources=W.R, indexed_col=[W.CPU, W.MEM, W.GPU], indexed_resolution=[1000, 128 * W.Mi, 1], pc_priority=[0, 1], pc_preemptible=[1, 1],
                     drf_multiplier=[1.0, 1.0, 0.0, 1.0])
        s = Scheduler(lib, cfg)
        total = np.tile(np.array([64 * W.Gi, 16000, 512 * W.Gi, 0], dtype=np.int64), (n, 1))
        s.nodes_upsert(total, total)
        _handles[key] = s
    return _handles[key]


# ---------------------------------------------------------------- a. the reference's table
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_golden_cases(libs, case):
    sch = GOLDEN["scheduled"]
    for lib in libs:
        if lib is None:
            continue
        s = _handle(lib, GOLDEN["num_nodes"])
        rec, cand = s.preemption_join([e["job"] for e in sch], [e["node"] for e in sch], [e["method"] for e in sch], [case["node"]], [case["preempting_job"]],
                                      [case["preempted_sibling"]], [case["in_gang"]])
        t, by, sib, cands = rec[0]
        assert t == case["expected_type"]
        assert list(cands) == case["expected_candidates"]
        assert (by, sib) == ((case["preempting_job"], case["preempted_sibling"]) if t == FAIRSHARE else (-1, -1))
        assert cand.tolist() == [2, 3, 4]          # job-2 on node-1, job-3 and job-4 on node-2: each once, the two job-5 entries and job-6 are not urgency-scheduled


# ---------------------------------------------------------------- b. synthetic lists against numpy
def np_join(n_nodes, sj, sn, sm, pn, pb, ps, pg):
    sj, sn, sm, pn, pb, ps, pg = (np.asarray(x) for x in (sj, sn, sm, pn, pb, ps, pg))
    idx = np.nonzero(sm == M_URGENCY)[0]
    idx = idx[np.argsort(sn[idx], kind="stable")]
    cand = sj[idx]
    off = np.concatenate([[0], np.cumsum(np.bincount(sn[idx], minlength=n_nodes))]) if n_nodes else np.zeros(1, dtype=np.int64)
    rec = []
    for i in range(len(pn)):
        b, e = (int(off[pn[i]]), int(off[pn[i] + 1])) if 0 <= pn[i] < n_nodes else (0, 0)
        if ps[i] == SIB_OPTIMISER:
            rec.append((OPTIMISER, int(pb[i]), -1, ()))
        elif pb[i] >= 0:
            rec.append((FAIRSHARE, int(pb[i]), int(ps[i]) if ps[i] >= 0 else -1, ()))
        elif e > b:
            rec.append((URGENCY, -1, -1, tuple(int(x) for x in cand[b:e])))
        elif pg[i]:
            rec.append((UNKNOWN_GANG, -1, -1, ()))
        else:
            rec.append((UNKNOWN, -1, -1, ()))
    return rec, cand.astype(np.int32)


def _synthetic(n_nodes, ns, npre, seed, heavy=(), ends=False):
    """ns scheduled entries with methods 1..6 on random nodes (`heavy`: (node, count) urgency entries on one node; `ends`: urgency entries and preempted jobs on the first
    and the last node), npre preempted jobs of every kind.  Job ids are NOT ascending: the order within a node is the order of the list"""
    rng = np.random.default_rng(seed)
    sn = rng.integers(0, n_nodes, size=ns).astype(np.int32) if ns else np.zeros(0, np.int32)
    sm = rng.integers(1, 7, size=ns).astype(np.int32) if ns else np.zeros(0, np.int32)
    at = 0
    for node, count in heavy:
        pos = rng.choice(ns, size=count, replace=False) if at == 0 else rng.choice(np.nonzero(sm != M_URGENCY)[0], size=count, replace=False)
        sn[pos] = node; sm[pos] = M_URGENCY; at += 1
    if ends and ns >= 4:
        sn[:2] = [0, n_nodes - 1]; sm[:2] = M_URGENCY; sn[-2:] = [n_nodes - 1, 0]; sm[-2:] = M_URGENCY
    sj = rng.permutation(ns).astype(np.int32) + 1000
    pn = rng.integers(0, n_nodes, size=npre).astype(np.int32) if npre else np.zeros(0, np.int32)
    if ends and npre >= 2:
        pn[0], pn[-1] = n_nodes - 1, 0
    kind = rng.integers(0, 5, size=npre) if npre else np.zeros(0, np.int64)
    if ends and npre >= 2:
        kind[0] = kind[-1] = 0
    pb = np.where(kind >= 2, rng.integers(0, 5000, size=npre), -1).astype(np.int32)      # 0, 1: nothing on record; 2: fair share; 3: fair share through a sibling; 4: optimiser
    ps = np.where(kind == 3, rng.integers(0, 5000, size=npre), np.where(kind == 4, SIB_OPTIMISER, -1)).astype(np.int32)
    pg = ((kind == 3) | (rng.random(npre) < 0.4)).astype(np.uint8)
    return sj, sn, sm, pn, pb, ps, pg


SHAPES = {
    "nothing": dict(n_nodes=4, ns=0, npre=0),
    "no preempted": dict(n_nodes=4, ns=40, npre=0),
    "no scheduled": dict(n_nodes=4, ns=0, npre=9),
    "one node": dict(n_nodes=1, ns=37, npre=11),
    "3 workgroups + 1 nodes": dict(n_nodes=3 * WG + 1, ns=300, npre=200, ends=True),
    "3 scan tiles + 1 nodes": dict(n_nodes=3 * TILE + 1, ns=1500, npre=700, ends=True),
    "more scan tiles than one workgroup": dict(n_nodes=WG * TILE + TILE + 1, ns=2000, npre=700, ends=True),   # the carry of the tile-offset loop
    "65 on a node": dict(n_nodes=20, ns=400, npre=120, heavy=[(7, 65)]),
    "257 on a node": dict(n_nodes=20, ns=900, npre=120, heavy=[(3, 257), (19, 65)]),
    "1025 entries": dict(n_nodes=130, ns=1025, npre=1025, ends=True),
}


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_join_on_synthetic_lists(libs, shape):
    kw = dict(SHAPES[shape])
    n_nodes = kw.pop("n_nodes")
    lists = _synthetic(n_nodes, seed=len(shape), **kw)
    want_rec, want_cand = np_join(n_nodes, *lists)
    if kw["ns"] > 100:
        assert len(set(lists[2].tolist())) == 6 and 0 < len(want_cand) < kw["ns"]      # methods 1..6 are all there, only 4 is picked
    for lib in libs:
        if lib is None:
            continue
        s = _handle(lib, n_nodes)
        for _ in range(2):                                                             # twice: the scatter's order must not show
            rec, cand = s.preemption_join(*lists)
            assert cand.tolist() == want_cand.tolist()
            assert rec == want_rec


# ---------------------------------------------------------------- c. the reference's pins, with the preemptor
def _marks_run(lib, nodes, placed, order, incoming, more=()):
    """tests/test_z_gang_preemption_marks.py _run: placed: [(job, node)] incumbents; order: incumbents in evicted-table index order; incoming: the new job of queue B
    (`more`: further new jobs of queue B behind it)"""
    cfg = F.TestSchedulingConfig()
    jobs = [j for j, _ in placed] + [incoming] + list(more)
    ident = {id(j): i for i, j in enumerate(jobs)}
    c = scenario.Case(lib, cfg, nodes)
    c.set_jobs(jobs, {"A": 0, "B": 1}, {})
    s = c.sched
    npc = len(c.pc_names)
    s.round_prepare([1.0, 1.0], [[], [ident[id(j)] for j in [incoming] + list(more)]], name_rank=[0, 1], demand=np.zeros((2, scenario.R), dtype=np.int64),
                    allocated_by_pc=np.zeros((2, npc, scenario.R), dtype=np.int64), fairshare_preemption_tokens=100.0)
    node_of = {id(j): n for j, n in placed}
    for j, n in placed:
        s.bind(ident[id(j)], n, cfg["priority_classes"][j["pc"]]["priority"])
    for idx, j in enumerate(order):
        s.evict(ident[id(j)], node_of[id(j)])
        s.add_evicted(idx, ident[id(j)], node_of[id(j)])
    res = s.schedule_queues()
    return res, ident, s.preemption_causes()


def test_victim_names_the_incoming_job(libs):
    """gang_scheduler_test.go:812, queue_scheduler_test.go:798: the victim's PreemptingJob is the incoming job"""
    got = []
    for lib in libs:
        if lib is None:
            continue
        node = F.Test32CpuNode(F.TestPriorities)
        incumbents = F.N1Cpu4GiJobs("A", F.PriorityClass0, 32)
        incoming = F.Test1Cpu4GiJob("B", F.PriorityClass1)
        res, ident, causes = _marks_run(lib, [node], [(j, 0) for j in incumbents], incumbents, incoming)
        new = ident[id(incoming)]
        assert res.scheduled == {new: 0} and len(res.preempted) == 1
        assert causes == {next(iter(res.preempted)): (FAIRSHARE, new, -1, ())}
        got.append(causes)
    assert all(g == got[0] for g in got)


def test_sibling_names_the_member_that_pulled_it_in(libs):
    """gang_scheduler_test.go:905-926, nodedb_test.go:1929-1934: g1 is preempted by the incoming job directly, g2 by the same job through its sibling g1"""
    got = []
    for lib in libs:
        if lib is None:
            continue
        nodes = [F.Test32CpuNode(F.TestPriorities), F.Test32CpuNode(F.TestPriorities)]
        g1, g2 = F.WithGangJobDetails(F.N1Cpu4GiJobs("A", F.PriorityClass0, 2), "gang-1", 2, "")
        filler1, filler2 = F.N1Cpu4GiJobs("A", F.PriorityClass0, 31), F.N1Cpu4GiJobs("A", F.PriorityClass0, 31)
        node1_jobs, node2_jobs = [g1] + filler1, [g2] + filler2
        placed = [(j, 0) for j in node1_jobs] + [(j, 1) for j in node2_jobs]
        order = node2_jobs + filler1 + [g1]
        incoming = F.Test1Cpu4GiJob("B", F.PriorityClass1)
        res, ident, causes = _marks_run(lib, nodes, placed, order, incoming)
        new, a, b = ident[id(incoming)], ident[id(g1)], ident[id(g2)]
        assert res.scheduled == {new: 0}
        assert causes == {a: (FAIRSHARE, new, -1, ()), b: (FAIRSHARE, new, a, ())}
        got.append(causes)
    assert all(g == got[0] for g in got)


# ---------------------------------------------------------------- d. full rounds against the oracle's result
def check_round(wl, ref, causes):
    """ref: the oracle's RoundResult of the same round (the product's lists equal it: assert_same_round); causes: Scheduler.preemption_causes()"""
    assert set(causes) == set(ref.preempted)
    by_node = {}
    for j in sorted(ref.scheduled):
        if ref.scheduled_method[j] == M_URGENCY:
            by_node.setdefault(ref.scheduled[j], []).append(j)
    direct = {}                                                         # preemptor -> nodes of the victims it preempted directly
    for v, (t, by, sib, cands) in causes.items():
        node = ref.preempted[v]
        if t in (FAIRSHARE, OPTIMISER):
            assert cands == ()
            assert 0 <= by < wl.num_jobs and by not in ref.preempted, (v, by)
            if by in ref.scheduled:
                # (a preemptor that the oversubscribed evictor evicted again and the second pass put back on its node comes out with the method of that last
                #  selection, ScheduledWithoutPreemption's sibling "rescheduled": only in a round with phase-3 evictions, and still on the victim's node)
                ok = (M_FAIRSHARE, M_RESCHEDULED) if ref.num_evicted_phase3 != 0 else (M_FAIRSHARE,)
                assert ref.scheduled_method[by] in (ok if t == FAIRSHARE else (M_OPTIMISER,)), (v, by, ref.scheduled_method[by])
                if sib == -1:
                    assert ref.scheduled[by] == node, (v, by)
            elif t == FAIRSHARE:
                assert ref.num_evicted_phase3 != 0, (v, by)           # only the oversubscribed evictor takes a job scheduled in this round away again
            else:
                assert wl.job_node[by] < 0, (v, by)                   # ... or the optimiser itself: a queued job it placed and later preempted for another is in neither list (pqs.go:232-249)
            if t == OPTIMISER:
                assert sib == -1
            elif sib != -1:
                assert sib in causes and sib != v
                assert wl.job_gang[sib] >= 0 and wl.job_gang[sib] == wl.job_gang[v] and wl.job_queue[sib] == wl.job_queue[v]
                assert causes[sib][:3] == (FAIRSHARE, by, -1)
            else:
                direct.setdefault(by, set()).add(node)
        else:
            want = by_node.get(node, [])
            assert (t, by, sib, list(cands)) == ((URGENCY if want else UNKNOWN_GANG if wl.job_gang[v] >= 0 else UNKNOWN), -1, -1, want), (v, node)
    for j, m in ref.scheduled_method.items():
        if m == M_FAIRSHARE:
            assert ref.scheduled[j] in direct.get(j, ()), f"job {j} was scheduled by fair-share preemption and no victim on its node names it"
    return causes


def run_round(lib, wl, fp=None, queues_only=False):
    s = W.load(lib, wl); W.prepare(s, wl, fairshare_preemption_tokens=fp)
    res = s.schedule_queues() if queues_only else s.schedule_round()
    causes = s.preemption_causes() if lib.prefix != "oracle_" else None
    s.close()
    return res, causes


_oracle_rounds = {}


def same_round_and_causes(libs, oracle, wl, run=run_round, key=None, **kw):
    """the round on the oracle (once per `key`) and on every library of `libs`; the libraries' causes checked against the oracle's lists and against each other"""
    ref = _oracle_rounds.get(key) if key is not None else None
    if ref is None:
        ref, _ = run(oracle, wl)
        if key is not None:
            _oracle_rounds[key] = ref
    got = []
    for lib in libs:
        if lib is None:
            continue
        res, causes = run(lib, wl)
        scenario.assert_same_round(ref, res)
        got.append(check_round(wl, ref, causes, **kw))
    assert all(g == got[0] for g in got), "the HIP library's records differ from the CPU build's"
    return ref, got[0]


def _small(s, **kw):
    return W.small_random(n_nodes=10 + s % 9 * 7, n_jobs=300 + s % 7 * 60, n_queues=2 + s % 5, seed=7000 + s, occupied=[0.4, 0.8, 0.95, 1.0][s % 4], gangs=s % 4, **kw)


@pytest.mark.parametrize("s", range(24))
def test_small_rounds(libs, oracle_lib, s):
    same_round_and_causes(libs, oracle_lib, _small(s), key=("small", s))


def test_the_small_rounds_preempt_by_both_kinds(hostsim_lib, oracle_lib):
    """the 24 rounds above preempt 2 141 jobs, 2 109 of them on a node with an urgency-scheduled job and 706 on a node with a fair-share-scheduled one"""
    tot = np.zeros(4, dtype=np.int64)
    for s in range(24):
        ref, causes = same_round_and_causes((hostsim_lib, None), oracle_lib, _small(s), key=("small", s))
        urg = {n for j, n in ref.scheduled.items() if ref.scheduled_method[j] == M_URGENCY}
        fs = {n for j, n in ref.scheduled.items() if ref.scheduled_method[j] == M_FAIRSHARE}
        tot += [len(ref.preempted), sum(n in urg for n in ref.preempted.values()), sum(n in fs for n in ref.preempted.values()), sum(c[0] == FAIRSHARE for c in causes.values())]
    assert tot[:3].tolist() == [2141, 2109, 706] and tot[3] > 300, tot


def _paired(seed):
    """running preemptible jobs of one queue and priority class, on different nodes, paired into gangs of two"""
    wl = W.small_random(n_nodes=24, n_jobs=400, n_queues=3, seed=seed, occupied=[0.95, 1.0][seed % 2], gangs=0)
    g = 0
    for q in range(3):
        for pc in (0, 1):
            ids = np.nonzero((wl.job_node >= 0) & (wl.job_queue == q) & (wl.job_pc == pc))[0]
            for a, b in zip(ids[0::2], ids[1::2]):
                if wl.job_node[a] != wl.job_node[b]:
                    wl.job_gang[[a, b]] = g; wl.job_gang_card[[a, b]] = 2; g += 1
    return wl


@pytest.mark.parametrize("seed", range(7100, 7108))
def test_rounds_with_running_gangs(libs, oracle_lib, seed):
    wl = _paired(seed)
    ref, causes = same_round_and_causes(libs, oracle_lib, wl)
    assert sum(wl.job_gang[j] >= 0 for j in ref.preempted) >= 10
    assert any(c[2] >= 0 for c in causes.values())                    # the sibling branch of check_round is taken


def _big_node(protected):
    """one node of 128 cpu holding 128 running 1-cpu priority-0 jobs of queue 0, two 1-cpu nodes with one such job each, 70 queued priority-1 jobs of queue 1"""
    pcs = [(0, True), (1, True)]
    node_total = np.array([[1024 * W.Gi, 128_000, 4096 * W.Gi, 0], [8 * W.Gi, 1000, 32 * W.Gi, 0], [8 * W.Gi, 1000, 32 * W.Gi, 0]], dtype=np.int64)
    one = np.array([1 * W.Gi, 1000, 1 * W.Gi, 0], dtype=np.int64)
    run_node = np.array([0] * 128 + [1, 2], dtype=np.int32)
    nr, nq = len(run_node), 70
    return W._assemble("bignode", W._config(pcs, protected=protected), node_total, np.tile(one, (nr, 1)), run_node, np.zeros(nr, np.int32), np.zeros(nr, np.int32),
                       np.zeros(nr, np.int32), np.tile(one, (nq, 1)), np.ones(nq, np.int32), np.ones(nq, np.int32), np.array([0, 1]), np.array([1.0, 1.0]), {})


def test_one_slice_longer_than_a_wave(libs, oracle_lib):
    """protectedFractionOfFairShare 10: nothing is evicted for fair share, all 70 are placed by urgency preemption, 68 of them on node 0: ONE slice of 68 shared by 68 victims"""
    wl = _big_node(10.0)
    ref, causes = same_round_and_causes(libs, oracle_lib, wl)
    assert len(ref.scheduled) == 70 and set(ref.scheduled_method.values()) == {M_URGENCY}
    on0 = [v for v, n in ref.preempted.items() if n == 0]
    assert len(on0) == 68 and sum(n == 0 for n in ref.scheduled.values()) == 68
    assert all(causes[v][0] == URGENCY and len(causes[v][3]) == 68 for v in on0)


def test_seventy_fair_share_victims_seventy_preemptors(libs, oracle_lib):
    wl = _big_node(1.0)
    ref, causes = same_round_and_causes(libs, oracle_lib, wl)
    assert len(ref.scheduled) == 70 and set(ref.scheduled_method.values()) == {M_FAIRSHARE} and ref.num_evicted_phase3 == 0
    assert len(ref.preempted) == 70 and sum(n == 0 for n in ref.preempted.values()) == 68
    assert all(c[0] == FAIRSHARE and c[2] == -1 for c in causes.values())
    assert len({c[1] for c in causes.values()}) == 70 and {c[1] for c in causes.values()} == set(ref.scheduled)


def test_queue_scheduler_alone_marks_only(libs):
    """after schedule_queues every preempted job is a marked one: every type is FAIRSHARE.  Two full nodes of evicted priority-0 jobs of queue A (the state of
    test_victim_names_the_incoming_job), seven new priority-1 jobs of queue B: seven victims, each naming its own preemptor, on the preemptor's node"""
    got = []
    for lib in libs:
        if lib is None:
            continue
        nodes = [F.Test32CpuNode(F.TestPriorities), F.Test32CpuNode(F.TestPriorities)]
        on0, on1 = F.N1Cpu4GiJobs("A", F.PriorityClass0, 32), F.N1Cpu4GiJobs("A", F.PriorityClass0, 32)
        new = [F.Test1Cpu4GiJob("B", F.PriorityClass1) for _ in range(7)]
        res, ident, causes = _marks_run(lib, nodes, [(j, 0) for j in on0] + [(j, 1) for j in on1], on0 + on1, new[0], new[1:])
        ids = [ident[id(j)] for j in new]
        assert sorted(res.scheduled) == ids and set(res.scheduled_method.values()) == {M_FAIRSHARE}
        assert len(res.preempted) == 7 and set(causes) == set(res.preempted)
        assert all(c[0] == FAIRSHARE and c[2] == -1 and c[3] == () for c in causes.values())
        assert sorted(c[1] for c in causes.values()) == ids
        assert all(res.scheduled[c[1]] == (0 if v < 32 else 1) for v, c in causes.items())   # (incumbents 0..31 sit on node 0, 32..63 on node 1; the queue scheduler alone reports no preempted_node)
        got.append(causes)
    assert all(g == got[0] for g in got)


# ---------------------------------------------------------------- e. the other round kernels
def test_two_word_key_round(libs, oracle_lib, monkeypatch):
    monkeypatch.setenv("ASCHED_KEY_WORDS", "2")                       # tests/test_z_two_word_keys.py: the round kernel of armada_sched_wk.hip
    ref, causes = same_round_and_causes(libs, oracle_lib, _small(3), run=lambda lib, wl: run_round(lib, wl, fp=None))
    assert {c[0] for c in causes.values()} >= {FAIRSHARE, URGENCY}


def _market_round(lib, wl, bids, cutoff):
    """tests/test_z_market_round.py market_round"""
    s = W.load(lib, wl)
    W.set_jobs(s, wl, bid_price=bids)
    pcp = np.asarray(wl.config.pc_priority)
    queued = [sorted(q, key=lambda j: (-int(pcp[wl.job_pc[j]]), -float(bids[j]), int(wl.job_submit[j]), int(j))) for q in wl.queued]   # jobdb.PriceOrder
    nq = wl.num_queues
    s.round_prepare(wl.queue_weight, queued, global_tokens=float(wl.global_burst), global_burst=wl.global_burst, global_rate_inf=wl.rate_inf,
                    queue_tokens=[float(wl.queue_burst)] * nq, queue_burst=[wl.queue_burst] * nq, queue_rate_inf=[wl.rate_inf] * nq)
    s.set_market(True, cutoff)
    res = s.schedule_round()
    causes = s.preemption_causes() if lib.prefix != "oracle_" else None
    s.close()
    return res, causes


def test_market_round(libs, oracle_lib):
    wl = _small(3)
    rng = np.random.default_rng(11)
    bids = rng.integers(0, 4, size=wl.num_jobs).astype(np.float64)
    for g in set(int(x) for x in wl.job_gang if x >= 0):
        m = np.nonzero(wl.job_gang == g)[0]
        bids[m] = bids[m[0]]
    nonpre = np.array([not wl.config.pc_preemptible[p] for p in wl.job_pc])
    bids[(wl.job_node >= 0) & nonpre] = 1_000_000.0                   # pricing.NonPreemptibleRunningPrice
    ref, causes = same_round_and_causes(libs, oracle_lib, wl, run=lambda lib, w: _market_round(lib, w, bids, 0.3))
    assert len(ref.preempted) > 0 and any(c[0] == FAIRSHARE for c in causes.values())


def _optimiser_round(lib, wl, kw):
    s = W.load(lib, wl); W.prepare(s, wl)
    s.set_optimiser(True, **kw)
    res = s.schedule_round()
    causes = s.preemption_causes() if lib.prefix != "oracle_" else None
    s.close()
    return res, causes


@pytest.mark.parametrize("seed", [3, 11])
def test_optimiser_round(libs, oracle_lib, seed):
    """tests/test_z_optimiser_round.py _gang_case: a full cluster, one preemptible class, every queue protected: what is placed is placed by the optimiser"""
    rng = np.random.default_rng(seed)
    wl = W.small_random(n_nodes=int(rng.integers(6, 40)), n_jobs=int(rng.integers(100, 600)), n_queues=int(rng.integers(2, 6)), seed=seed, occupied=1.0, gangs=int(rng.integers(3, 12)))
    wl.config = copy.copy(wl.config); wl.config.protected_fraction_of_fair_share = 1.0
    wl.job_pc[:] = 0
    wl.job_run_ts = (np.arange(wl.num_jobs, dtype=np.int64) * 7919 % 100003) * 1_000_000
    kw = dict(min_improvement_pct=0.0, max_jobs_per_round=60, now_ms=200_000)
    ref, causes = same_round_and_causes(libs, oracle_lib, wl, run=lambda lib, w: _optimiser_round(lib, w, kw))
    placed = [j for j, m in ref.scheduled_method.items() if m == M_OPTIMISER]
    victims = [v for v, c in causes.items() if c[0] == OPTIMISER]
    by = {causes[v][1] for v in victims}
    assert placed and victims and by & set(placed) and all(wl.job_node[j] < 0 for j in by - set(placed))   # (check_round: a preemptor the optimiser preempted again)


# ---------------------------------------------------------------- f. refusals
def test_refusals(libs):
    wl = _small(3)
    got = []
    for lib in libs:
        if lib is None:
            continue
        s = W.load(lib, wl); W.prepare(s, wl)
        with pytest.raises(SchedError) as e:
            s.preemption_causes()
        assert e.value.code == ERR_INVALID and "no round result" in str(e.value)
        res = s.schedule_round()
        npre = len(res.preempted)
        causes = s.preemption_causes()
        need = sum(1 for j, m in res.scheduled_method.items() if m == M_URGENCY)
        assert npre > 0 and need > 0
        from armada_amd.binding import CPreemptionCause
        import ctypes as C
        rec, cand, out = (CPreemptionCause * npre)(), (C.c_int32 * need)(), C.c_int32(-1)
        for cap, ccap in ((npre - 1, need), (npre, need - 1), (0, 0)):
            rc = lib.round_preemption_causes(s.h, rec, cap, cand, ccap, C.byref(out))
            msg = lib.last_error(s.h).decode()
            assert rc == ERR_INVALID and out.value == need and f"{npre} cause records and {need} candidate words" in msg, msg
        assert lib.round_preemption_causes(s.h, rec, npre, cand, need, C.byref(out)) == 0 and out.value == need
        with pytest.raises(SchedError) as e:                               # a scheduled entry on a node the handle does not have
            s.preemption_join([1], [wl.num_nodes], [M_URGENCY], [0], [-1], [-1], [0])
        assert e.value.code == ERR_INVALID
        s.round_exchange()                                                 # the queue-hash mode's resolve (world size 1)
        with pytest.raises(SchedError) as e:
            s.preemption_causes()
        assert e.value.code == ERR_INVALID and "round_exchange" in str(e.value)
        s.close()
        got.append(causes)
    assert all(g == got[0] for g in got)


def test_library_without_the_entry_point_says_so(oracle_lib):
    wl = _small(1)
    s = W.load(oracle_lib, wl); W.prepare(s, wl)
    s.schedule_round()
    with pytest.raises(SchedError) as e:
        s.preemption_causes()
    assert "does not export" in str(e.value)
    with pytest.raises(SchedError):
        s.preemption_join([], [], [], [], [], [], [])
    s.close()
