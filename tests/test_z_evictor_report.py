"""The evictor result of a round: asched_set_evictor_report / asched_round_evictor_report (SchedulingInformation.EvictorResult, scheduling/result.go:81-94;
EvictorResult, eviction.go:27-79) — which running jobs the balancing evictor of phase 1 evicted and from which node, jobs and resources per queue, and per node
whether all of its jobs could be preempted and, if not, why (armada_amd/csrc/kernels_evict_report.h).

The expected report is a numpy restatement (`restate`) of eviction.go:197-238 and the job filter of preempting_queue_scheduler.go:101-136, computed from what was
UPLOADED — the node and job tables, pc_preemptible, the protected fraction, the queues' start-of-round allocation — plus the fair shares of the round result and the
ORACLE's drf_cost for the actual share; it reads no other output of the code under test.  On every round its evicted count must equal the oracle's
num_evicted_phase1 for the same input.  The uploads are recorded by wrapping the Scheduler's upload methods for the duration of a test (`recording`): the same
wrapper turns the switch on, fetches the report after every schedule_round and compares.

a. small rounds with only running jobs, at the sizes where the three passes take another turn; b. the reference's PQS goldens, every round; c. 24 seeded rounds of
the configs[4] shape; d. a two-word-key round and an optimiser round; e. refusals; f. the launches of a round with the switch off.
Every case runs on the CPU build of the device code and, marked gpu, on the HIP library — there every array must also equal the CPU build's, byte for byte."""
import contextlib
import copy

import numpy as np
import pytest

import scenario
from armada_amd import binding as B
from armada_amd import workloads as W
from armada_amd.binding import Config, SchedError, Scheduler
from golden_io import ids, load

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
WG = 256            # workgroup size of the three passes (MG_THREADS)
TILE = 256          # entries of the evicted list per workgroup of the queue pass (EVR_TILE)
REPORT_LAUNCHES = 3  # a constant of the design: the job pass, the node pass, the queue pass
ALL_PRE, BELOW, INVALID_Q, NOT_PRE, EMPTY, UNSCHED = 1, 2, 4, 8, 16, 32
ARRAYS = ("node_preemptible", "node_reasons", "node_evicted_jobs", "queue_evicted_jobs", "queue_evicted_resources", "queue_evicted_off", "evicted_job", "evicted_node")


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def libs(request):
    """(library under test, CPU build to compare its arrays with or None)"""
    hs = request.getfixturevalue("hostsim_lib")
    return (hs, None) if request.param == "hostsim" else (request.getfixturevalue("hip_lib"), hs)


def test_reason_names_are_the_references_sorted_strings():
    assert list(B.EVICTOR_REASONS) == sorted(B.EVICTOR_REASONS) and len(B.EVICTOR_REASONS) == 6
    assert [B.EVR_ALL_JOBS_PREEMPTIBLE, B.EVR_BELOW_PROTECTED_FAIR_SHARE, B.EVR_INVALID_QUEUE, B.EVR_JOB_NOT_PREEMPTIBLE, B.EVR_NODE_EMPTY, B.EVR_NODE_UNSCHEDULABLE] == [1, 2, 4, 8, 16, 32]
    assert B.evictor_reason_string(BELOW | NOT_PRE | UNSCHED) == "below_protected_fair_share,job_not_preemptible,node_unschedulable"   # makeNodePreemptiblityStats: sorted, comma-joined
    assert B.evictor_reason_string(ALL_PRE) == "all_jobs_preemptible" and B.evictor_reason_string(EMPTY | UNSCHED) == "node_empty,node_unschedulable"


# ---------------------------------------------------------------- the restatement
def restate(cfg, nodes, jobs, prep, evicted_on_node, res, drf):
    """cfg: the handle's Config; nodes / jobs / prep: what nodes_upsert / jobs_set / round_prepare were given; evicted_on_node: jobs evicted on their node before the
    round (asched_evict); res: the round result (its fair shares are read); drf(alloc, total) -> the oracle's drf_cost"""
    R = cfg.num_resources
    total = nodes["allocatable"].sum(axis=0).astype(np.int64) if len(nodes["allocatable"]) else np.zeros(R, np.int64)
    floating = np.array([x >= 0 for x in cfg.floating_resource_limit], dtype=bool) if cfg.floating_resource_limit is not None else np.zeros(R, dtype=bool)
    for r in range(R):
        if floating[r]:
            total[r] = cfg.floating_resource_limit[r] if cfg.floating_counts_in_total else 0
    N, Q = len(nodes["total"]), len(prep["weight"])
    req = jobs["req"]
    M = len(req)
    queue = np.asarray(jobs["queue"] if jobs["queue"] is not None else np.zeros(M), dtype=np.int64)
    pc = np.asarray(jobs["pc"] if jobs["pc"] is not None else np.zeros(M), dtype=np.int64)
    node = np.asarray(jobs["node"] if jobs["node"] is not None else np.full(M, -1), dtype=np.int64)
    away = np.asarray(jobs["away"], dtype=bool) if jobs["away"] is not None else np.zeros(M, dtype=bool)
    gang = np.asarray(jobs["gang_id"] if jobs["gang_id"] is not None else np.full(M, -1), dtype=np.int64)
    qprio = np.asarray(jobs["queue_priority"] if jobs["queue_priority"] is not None else np.zeros(M), dtype=np.int64)
    submit = np.asarray(jobs["submit_time"] if jobs["submit_time"] is not None else np.arange(M), dtype=np.int64)
    run_ts = np.asarray(jobs["run_timestamp"] if jobs["run_timestamp"] is not None else np.zeros(M), dtype=np.int64)
    unsched = np.asarray(nodes["unschedulable"], dtype=bool) if nodes["unschedulable"] is not None else np.zeros(N, dtype=bool)
    pre_on = np.zeros(M, dtype=bool)
    pre_on[list(evicted_on_node)] = True
    valid_q = (queue >= 0) & (queue < Q)
    # the queues' allocation at the start of the round: the caller's, or the running jobs'
    if prep.get("allocated_by_pc") is not None:
        alloc = np.asarray(prep["allocated_by_pc"], dtype=np.int64).reshape(Q, -1, R).sum(axis=1)
    else:
        alloc = np.zeros((Q, R), dtype=np.int64)
        on = (node >= 0) & valid_q
        np.add.at(alloc, queue[on], req[on])
    # preempting_queue_scheduler.go:124-134, "as written": !(actual / fair <= protectedFraction)
    evictable = np.zeros(Q, dtype=bool)
    for q in range(Q):
        actual = drf(alloc[q], total)
        fair = max(float(res.demand_capped_adjusted_fair_share[q]), float(res.fair_share[q]))
        if cfg.protect_uncapped_adjusted_fair_share:
            fair = float(res.uncapped_adjusted_fair_share[q])
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.float64(actual) / np.float64(fair)
        evictable[q] = not (frac <= cfg.protected_fraction_of_fair_share)
    preemptible = np.asarray(cfg.pc_preemptible, dtype=bool)
    # reason(j) in the reference's order (:101-136)
    reason = np.zeros(M, dtype=np.int64)
    for j in range(M):
        if away[j]:
            reason[j] = 0
        elif not valid_q[j]:
            reason[j] = INVALID_Q
        elif not preemptible[pc[j]]:
            reason[j] = NOT_PRE
        elif not evictable[queue[j]]:
            reason[j] = BELOW
    considered = (node >= 0) & ~pre_on                              # eviction.go:213-214: on the node and not evicted there
    flag = considered & ~away & valid_q & (reason == 0)
    # evictGangs (preempting_queue_scheduler.go:357-424): a partly evicted gang is evicted entirely
    for key in {(int(queue[j]), int(gang[j])) for j in np.nonzero(flag & (gang >= 0))[0]}:
        mem = (queue == key[0]) & (gang == key[1])
        flag |= mem & considered
    # per node (eviction.go:197-238)
    node_pre, node_reasons, node_ev = np.zeros(N, dtype=bool), np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.int32)
    on_count = np.bincount(node[node >= 0], minlength=N) if N else np.zeros(0, np.int64)
    ors = np.zeros(N, dtype=np.int64)
    for j in np.nonzero(considered)[0]:
        ors[node[j]] |= reason[j]
    for n in range(N):
        if on_count[n] == 0:
            node_reasons[n] = EMPTY | (UNSCHED if unsched[n] else 0)
            node_pre[n] = not unsched[n]
        else:
            r = int(ors[n]) | (UNSCHED if unsched[n] else 0)
            node_reasons[n] = r if r else ALL_PRE
            node_pre[n] = r == 0
    np.add.at(node_ev, node[flag], 1)
    # per queue (eviction.go:60-71); the list: grouped by queue, SchedulingOrderCompare inside (jobdb/comparison.go:49-107, running jobs)
    ev = np.nonzero(flag)[0]
    pcp = np.asarray(cfg.pc_priority, dtype=np.int64)
    order = np.lexsort((ev, submit[ev], run_ts[ev], qprio[ev], -pcp[pc[ev]], queue[ev]))
    ev = ev[order]
    kreq = req.copy()
    kreq[:, floating] = 0                                           # KubernetesResourceRequirements: no floating resources
    q_jobs = np.bincount(queue[ev], minlength=Q).astype(np.int32) if Q else np.zeros(0, np.int32)
    q_res = np.zeros((Q, R), dtype=np.int64)
    np.add.at(q_res, queue[ev], kreq[ev])
    return dict(num_evicted=len(ev), num_affected_nodes=int((node_ev > 0).sum()), node_preemptible=node_pre, node_reasons=node_reasons, node_evicted_jobs=node_ev,
                queue_evicted_jobs=q_jobs, queue_evicted_resources=q_res, queue_evicted_off=np.concatenate([[0], np.cumsum(q_jobs)]).astype(np.int32),
                evicted_job=ev.astype(np.int32), evicted_node=node[ev].astype(np.int32))


def assert_report(got, want, what=""):
    assert got["num_evicted"] == want["num_evicted"] and got["num_affected_nodes"] == want["num_affected_nodes"], (what, got["num_evicted"], want["num_evicted"])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)


# ---------------------------------------------------------------- recording the uploads of every handle while a test runs
class Log:
    def __init__(self):
        self.reports, self.restated, self.oracle_n1, self.results = [], [], [], []


_drf_handles = {}


def _oracle_drf(oracle_lib, cfg):
    key = id(cfg)
    if key not in _drf_handles:
        _drf_handles[key] = (Scheduler.__new__(Scheduler), cfg)
        s = _drf_handles[key][0]
        _ORIG["__init__"](s, oracle_lib, cfg)
    return _drf_handles[key][0].drf_cost


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for s, _ in _drf_handles.values():
        s.close()
    _drf_handles.clear()


_ORIG = {n: getattr(Scheduler, n) for n in ("__init__", "nodes_upsert", "jobs_set", "round_prepare", "schedule_round", "evict")}


@contextlib.contextmanager
def recording(monkeypatch, oracle_lib, switch=True):
    """every Scheduler made inside keeps what it uploads; a library under test gets the switch turned on before each schedule_round, its report fetched and
    compared with the restatement afterwards; the oracle's num_evicted_phase1 is kept per round"""
    log = Log()

    def init(self, lib, cfg):
        _ORIG["__init__"](self, lib, cfg)
        self._up_cfg, self._up_evicted = cfg, set()

    def nodes_upsert(self, total, allocatable=None, **kw):
        t = np.array(total, dtype=np.int64).reshape(-1, self.R)
        self._up_nodes = dict(total=t, allocatable=t if allocatable is None else np.array(allocatable, dtype=np.int64).reshape(-1, self.R), unschedulable=kw.get("unschedulable"))
        return _ORIG["nodes_upsert"](self, total, allocatable, **kw)

    def jobs_set(self, req, **kw):
        names = ("queue", "pc", "node", "away", "gang_id", "queue_priority", "submit_time", "run_timestamp")
        self._up_jobs = dict(req=np.array(req, dtype=np.int64).reshape(-1, self.R), **{n: (None if kw.get(n) is None else np.array(kw[n])) for n in names})
        self._up_evicted = set()
        return _ORIG["jobs_set"](self, req, **kw)

    def round_prepare(self, weight, queued, **kw):
        self._up_prep = dict(weight=list(weight), allocated_by_pc=None if kw.get("allocated_by_pc") is None else np.array(kw["allocated_by_pc"]))
        return _ORIG["round_prepare"](self, weight, queued, **kw)

    def evict(self, job, node):
        self._up_evicted.add(int(job))
        return _ORIG["evict"](self, job, node)

    def schedule_round(self, *a, **kw):
        oracle = self.lib.prefix == "oracle_"
        if not oracle and switch:
            self.set_evictor_report(True)
        res = _ORIG["schedule_round"](self, *a, **kw)
        log.results.append(res)
        if oracle:
            log.oracle_n1.append(res.num_evicted_phase1)
        elif switch:
            rep = self.round_evictor_report()
            want = restate(self._up_cfg, self._up_nodes, self._up_jobs, self._up_prep, self._up_evicted, res, _oracle_drf(oracle_lib, self._up_cfg))
            assert_report(rep, want, f"round {len(log.reports)}")
            assert rep["queue_evicted_jobs"].sum() == rep["num_evicted"] and rep["num_affected_nodes"] == (rep["node_evicted_jobs"] != 0).sum()
            log.reports.append(rep); log.restated.append(want)
        return res

    for name, fn in (("__init__", init), ("nodes_upsert", nodes_upsert), ("jobs_set", jobs_set), ("round_prepare", round_prepare), ("evict", evict), ("schedule_round", schedule_round)):
        monkeypatch.setattr(Scheduler, name, fn)
    try:
        yield log
    finally:
        for name in _ORIG:
            monkeypatch.setattr(Scheduler, name, _ORIG[name])


def run_everywhere(monkeypatch, libs, oracle_lib, run):
    """`run(lib)` on the oracle and on every library of `libs`, recorded: every report equals the restatement, the restatement's evicted count the oracle's, and the
    HIP library's arrays the CPU build's.  -> (oracle's results, reports of the library under test, results of the library under test)"""
    with recording(monkeypatch, oracle_lib) as ref:
        run(oracle_lib)
    out = []
    for lib in libs:
        if lib is None:
            continue
        with recording(monkeypatch, oracle_lib) as log:
            run(lib)
        assert len(log.reports) == len(ref.oracle_n1) > 0
        assert [r["num_evicted"] for r in log.restated] == ref.oracle_n1, "the restatement's evicted count is not the oracle's num_evicted_phase1"
        out.append(log)
    for a, b in zip(out[0].reports, out[-1].reports):
        assert_report(b, a, "HIP library against the CPU build")
    return ref.results, out[0].reports, out[0].results


# ---------------------------------------------------------------- a. small rounds with only running jobs
def _running(n_nodes, run_node, run_queue, run_pc, n_queues, protected, *, pcs=((0, True), (1, True), (3, False)), unschedulable=None, away=None, gang=None, floating=False,
             evict_first=(), seed=0, node_cpu=6_000_000):
    """a pool of n_nodes big nodes with the given running jobs (1 cpu each, memory by the job index) and nothing queued"""
    rng = np.random.default_rng(seed)
    nr = len(run_node)
    cfg = W._config(list(pcs), protected=protected)
    if floating:
        cfg = copy.copy(cfg)
        cfg.floating_resource_limit = [-1, -1, 1 << 50, -1]         # column 2 is a floating resource of the pool (not an indexed column: those are node resources)
    node_total = np.tile(np.array([1 << 46, node_cpu, 1 << 46, 0], dtype=np.int64), (n_nodes, 1))      # (room for 5 000 of the jobs below on one node)
    req = np.stack([(1 + rng.integers(0, 8, size=nr)) * W.Gi, np.full(nr, 1000), (rng.integers(1, 4, size=nr) if floating else rng.integers(0, 4, size=nr)) * W.Gi, np.zeros(nr, np.int64)], axis=1).astype(np.int64)
    pc_prio = np.array([p for p, _ in pcs])
    wl = W._assemble("evr", cfg, node_total, req, np.asarray(run_node, np.int32), np.asarray(run_queue, np.int32), np.asarray(run_pc, np.int32), pc_prio[np.asarray(run_pc)].astype(np.int32),
                     np.zeros((0, W.R), np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), pc_prio, np.ones(n_queues), {})
    if gang is not None:
        wl.job_gang = np.asarray(gang, np.int32)
        wl.job_gang_card = np.array([max(1, int((wl.job_gang == g).sum())) if g >= 0 else 1 for g in wl.job_gang], np.int32)
    if away is not None:
        wl.job_away = np.asarray(away, np.uint8)
    wl.meta = dict(unschedulable=unschedulable, evict_first=list(evict_first))
    return wl


def _run_running(lib, wl):
    s = Scheduler(lib, wl.config)
    s.nodes_upsert(wl.node_total, wl.node_allocatable, unschedulable=wl.meta["unschedulable"])
    W.set_jobs(s, wl)
    W.prepare(s, wl)
    for j in wl.meta["evict_first"]:
        s.evict(int(j), int(wl.job_node[j]))
    s.schedule_round()
    s.close()


def _mixed(n_nodes, n_jobs, n_queues, protected, seed, **kw):
    rng = np.random.default_rng(seed)
    return _running(n_nodes, rng.integers(0, n_nodes, size=n_jobs), rng.integers(0, n_queues, size=n_jobs), rng.choice(3, size=n_jobs, p=[0.5, 0.3, 0.2]), n_queues, protected, seed=seed, **kw)


def _sizes_case(name):
    if name.startswith("N="):       # node counts around the workgroup size; M with a last partial workgroup
        n = int(name[2:])
        return _mixed(n, 3 * WG + 17, 3, 0.0, seed=n)
    if name == "one node carries 5000 jobs":
        return _running(40, np.full(5000, 7), np.arange(5000) % 3, np.arange(5000) % 2, 3, 0.0)
    if name == "Q=1":
        return _mixed(33, 700, 1, 0.0, seed=1)
    if name == "Q=70 many runs in a tile":
        return _mixed(64, 2 * TILE + 40, 70, 0.0, seed=70, pcs=((0, True), (1, True), (2, True)))
    if name == "a run starts mid-tile and covers more than two tiles":
        # queue 0: 100 evicted jobs, queue 1: 3 tiles + 9, queue 2 and 3: none (two adjacent empty queues), queue 4: 30
        q = np.concatenate([np.zeros(100), np.ones(3 * TILE + 9), np.full(30, 4)]).astype(int)
        return _running(50, np.arange(len(q)) % 50, q, np.zeros(len(q), int), 6, 0.0)      # (queue 5 has no running job either)
    if name == "nothing evicted":
        return _mixed(40, 600, 4, 1e9, seed=5)
    if name == "everything preemptible evicted":
        return _mixed(300, 2000, 5, 0.0, seed=6)
    if name == "node reasons":
        # node 0: preemptible and non-preemptible classes mixed; node 1: unschedulable, empty; node 2: unschedulable with jobs; node 3: only away jobs; node 4: empty;
        # node 5: a job of queue -1; node 6: only preemptible jobs
        node = [0, 0, 0, 2, 2, 3, 3, 5, 5, 6, 6]
        pc = [0, 2, 1, 0, 0, 2, 0, 0, 0, 0, 1]
        queue = [0, 0, 1, 1, 1, 0, 1, -1, 0, 1, 0]
        away = [0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
        return _running(7, node, queue, pc, 2, 0.0, unschedulable=[0, 1, 1, 0, 0, 0, 0], away=away)
    if name == "below protected fair share":
        # six nodes of 10 cpu, full: queue 0 holds a tenth of the pool (a fifth of its fair share of one half: protected), queue 1 the rest (1.8 times its fair share)
        node = np.arange(60) % 6
        return _running(6, node, [0] * 6 + [1] * 54, np.zeros(60, int), 2, 0.5, node_cpu=10_000)
    if name == "floating column":
        return _mixed(20, 500, 3, 0.0, seed=9, floating=True)
    if name == "gang closure":
        # gang 0: a preemptible and a non-preemptible member: the filter takes one, the closure the other; gang 1: one member evicted on its node beforehand
        node = [0, 1, 2, 3, 4, 5]
        return _running(6, node, [0] * 6, [0, 2, 0, 0, 2, 2], 1, 0.0, gang=[0, 0, 1, 1, -1, -1], evict_first=[2])
    raise KeyError(name)


SIZES = ["N=1", "N=255", "N=256", "N=257", "N=1025", "one node carries 5000 jobs", "Q=1", "Q=70 many runs in a tile", "a run starts mid-tile and covers more than two tiles",
         "nothing evicted", "everything preemptible evicted", "node reasons", "below protected fair share", "floating column", "gang closure"]


@pytest.mark.parametrize("name", SIZES)
def test_running_jobs_only(libs, oracle_lib, monkeypatch, name):
    wl = _sizes_case(name)
    _, reps, _ = run_everywhere(monkeypatch, libs, oracle_lib, lambda lib: _run_running(lib, wl))
    r = reps[0]
    pre = np.asarray(wl.config.pc_preemptible, dtype=bool)[wl.job_pc]
    if name == "nothing evicted":
        assert r["num_evicted"] == 0 and r["num_affected_nodes"] == 0 and len(r["evicted_job"]) == 0 and not r["queue_evicted_off"].any()
        assert set(r["node_reasons"].tolist()) <= {BELOW, BELOW | NOT_PRE, EMPTY}
    if name in ("everything preemptible evicted", "one node carries 5000 jobs") or name.startswith("N="):
        assert r["num_evicted"] == int(pre.sum()) and sorted(r["evicted_job"].tolist()) == np.nonzero(pre)[0].tolist()
    if name == "one node carries 5000 jobs":
        assert r["node_evicted_jobs"][7] == 5000 and r["num_affected_nodes"] == 1 and (np.delete(r["node_reasons"], 7) == EMPTY).all() and r["node_reasons"][7] == ALL_PRE
    if name == "Q=70 many runs in a tile":
        assert (r["queue_evicted_jobs"] > 0).sum() > 60 and r["num_evicted"] > 2 * TILE
    if name == "a run starts mid-tile and covers more than two tiles":
        assert r["queue_evicted_jobs"].tolist() == [100, 3 * TILE + 9, 0, 0, 30, 0] and r["queue_evicted_off"][1] % TILE != 0
    if name == "node reasons":
        assert r["node_reasons"].tolist() == [NOT_PRE, EMPTY | UNSCHED, UNSCHED, ALL_PRE, EMPTY, INVALID_Q, ALL_PRE]
        assert r["node_preemptible"].tolist() == [False, False, False, True, True, False, True]
        assert sorted(r["evicted_job"].tolist()) == [0, 2, 3, 4, 8, 9, 10]             # the away jobs, the non-preemptible one and the job of no queue stay
    if name == "below protected fair share":
        assert r["queue_evicted_jobs"].tolist() == [0, 54] and (r["node_reasons"] == BELOW).all() and not r["node_preemptible"].any()
    if name == "floating column":
        assert wl.job_req[:, 2].min() > 0 and (r["queue_evicted_resources"][:, 2] == 0).all() and (r["queue_evicted_resources"][:, 1] > 0).all()
    if name == "gang closure":
        # job 1 (not preemptible) is taken with its sibling 0; job 2 was evicted on its node before the round: not evicted again, its sibling 3 is (by the filter)
        assert sorted(r["evicted_job"].tolist()) == [0, 1, 3] and r["node_reasons"].tolist() == [ALL_PRE, NOT_PRE, ALL_PRE, ALL_PRE, NOT_PRE, NOT_PRE]


# ---------------------------------------------------------------- b. the reference's PQS goldens, every round
PQS = load("pqs")


@pytest.mark.parametrize("case", PQS, ids=ids(PQS))
def test_pqs_goldens(libs, oracle_lib, monkeypatch, case):
    def run(lib):
        assert scenario.run_pqs_case(lib, case) == "ok"
    ref, reps, _ = run_everywhere(monkeypatch, libs, oracle_lib, run)
    assert len(reps) == len(case["Rounds"])


# ---------------------------------------------------------------- c. seeded rounds of the configs[4] shape
def _config4(s):
    """BASELINE configs[4] (config3 with gangs, 95 % occupied, protected fraction 0.5) reduced to a few hundred nodes, and around it: other occupancies and protected
    fractions (queues below their protected share), and — every fourth — a full pool with few queued jobs, all of the lowest class: no urgency preemption, so nothing
    is oversubscribed and the oversubscribed evictor takes nothing (num_evicted_phase3 == 0)"""
    calm = s % 4 == 3
    wl = W.config3(n_nodes=150 + s % 5 * 40, n_jobs=150 if calm else 2500 + s % 7 * 300, n_queues=4 + s % 6 * 3, seed=9000 + s, gangs=4 + s % 5,
                   occupied=1.0 if calm else [0.95, 0.6, 1.0][s % 3])
    wl.config = copy.copy(wl.config)
    wl.config.protected_fraction_of_fair_share = [0.5, 0.0, 1.5, 0.5, 1.0, 0.5][s % 6]
    if calm:
        wl.job_pc[wl.job_node < 0] = 0
    if s % 2:                                                   # running gangs: pairs of one queue and class on different nodes (the closure reaches across nodes)
        g = int(wl.job_gang.max()) + 1
        for q in range(wl.num_queues):
            ids_ = np.nonzero((wl.job_node >= 0) & (wl.job_queue == q) & (wl.job_pc == s % 3))[0][:12]
            for a, b in zip(ids_[0::2], ids_[1::2]):
                if wl.job_node[a] != wl.job_node[b]:
                    wl.job_gang[[a, b]] = g; wl.job_gang_card[[a, b]] = 2; g += 1
    return wl


def _run_wl(lib, wl, before=None, then_off=None):
    """then_off: a list that receives the result of a second round on the SAME handle after set_evictor_report(False) and a fresh round_prepare"""
    s = W.load(lib, wl); W.prepare(s, wl)
    if before:
        before(s)
    s.schedule_round()
    if then_off is not None and lib.prefix != "oracle_":
        s.set_evictor_report(False)
        W.prepare(s, wl)
        then_off.append(_ORIG["schedule_round"](s))            # (not through the recording wrapper, which would turn the switch on again)
        _refused(s, ERR_INVALID, "switched off")
    s.close()


@pytest.mark.parametrize("s", range(24))
def test_config4_shaped_rounds(libs, oracle_lib, monkeypatch, s):
    wl = _config4(s)
    off = []
    ref, reps, res = run_everywhere(monkeypatch, libs, oracle_lib, lambda lib: _run_wl(lib, wl, then_off=off))
    o, r, rep = ref[0], res[0], reps[0]
    scenario.assert_same_round(o, r)                            # the round with the switch on is the oracle's ...
    assert len(off) == sum(lib is not None for lib in libs)
    for r_off in off:
        scenario.assert_same_round(r_off, r)                    # ... and the SAME handle's next round of the same input with the switch off (its buffers recycled)
    assert rep["queue_evicted_jobs"].sum() == rep["num_evicted"] == o.num_evicted_phase1
    assert rep["num_affected_nodes"] == np.count_nonzero(rep["node_evicted_jobs"])
    if o.num_evicted_phase3 == 0:                               # every preempted job was evicted by the balancing evictor, from the node it is reported preempted on
        where = dict(zip(rep["evicted_job"].tolist(), rep["evicted_node"].tolist()))
        assert all(where.get(j) == n for j, n in o.preempted.items())


def test_the_config4_shaped_rounds_cover_both_outcomes(hostsim_lib, oracle_lib, monkeypatch):
    """the 24 rounds above: some with phase-3 evictions, some with preemptions and none of phase 3; queues below their protected share, non-preemptible jobs"""
    bits, p3, n1 = 0, 0, 0
    for s in range(24):
        wl = _config4(s)
        ref, reps, _ = run_everywhere(monkeypatch, (hostsim_lib, None), oracle_lib, lambda lib: _run_wl(lib, wl))
        bits |= int(np.bitwise_or.reduce(reps[0]["node_reasons"])); p3 += ref[0].num_evicted_phase3 == 0 and len(ref[0].preempted) > 0; n1 += reps[0]["num_evicted"]
    assert bits & (ALL_PRE | BELOW | NOT_PRE) == ALL_PRE | BELOW | NOT_PRE and p3 > 0 and n1 > 1000, (bits, p3, n1)


# ---------------------------------------------------------------- d. the other split rounds
def test_two_word_key_round(libs, oracle_lib, monkeypatch):
    monkeypatch.setenv("ASCHED_KEY_WORDS", "2")                 # tests/test_z_two_word_keys.py: the round kernel of armada_sched_wk.hip
    wl = _config4(1)
    _, reps, _ = run_everywhere(monkeypatch, libs, oracle_lib, lambda lib: _run_wl(lib, wl))
    assert reps[0]["num_evicted"] > 0


def test_optimiser_round(libs, oracle_lib, monkeypatch):
    """tests/test_z_optimiser_round.py _gang_case: a full cluster, one preemptible class, every queue protected: nothing is evicted for balancing"""
    rng = np.random.default_rng(3)
    wl = W.small_random(n_nodes=int(rng.integers(6, 40)), n_jobs=int(rng.integers(100, 600)), n_queues=int(rng.integers(2, 6)), seed=3, occupied=1.0, gangs=int(rng.integers(3, 12)))
    wl.config = copy.copy(wl.config); wl.config.protected_fraction_of_fair_share = 1.0
    wl.job_pc[:] = 0
    wl.job_run_ts = (np.arange(wl.num_jobs, dtype=np.int64) * 7919 % 100003) * 1_000_000
    kw = dict(min_improvement_pct=0.0, max_jobs_per_round=60, now_ms=200_000)
    ref, reps, res = run_everywhere(monkeypatch, libs, oracle_lib, lambda lib: _run_wl(lib, wl, before=lambda s: s.set_optimiser(True, **kw)))
    scenario.assert_same_round(ref[0], res[0])
    assert 6 in set(ref[0].scheduled_method.values())          # ASCHED_METHOD_OPTIMISER: the optimiser's phase ran


# ---------------------------------------------------------------- e. refusals
def _refused(s, code, *words):
    with pytest.raises(SchedError) as e:
        s.round_evictor_report()
    assert e.value.code == code and str(e.value) and all(w in str(e.value) for w in words), (e.value.code, str(e.value))


def test_refusals(libs):
    wl = _config4(0)
    for lib in libs:
        if lib is None:
            continue
        s = W.load(lib, wl); W.prepare(s, wl)
        _refused(s, ERR_INVALID, "switched off")                        # the default
        s.schedule_round()
        _refused(s, ERR_INVALID, "switched off")
        s.set_evictor_report(True)
        _refused(s, ERR_INVALID, "no completed")                        # no round since the switch was turned on
        W.prepare(s, wl)
        _refused(s, ERR_INVALID, "no completed")                        # before any round
        s.schedule_round()
        assert s.round_evictor_report()["num_evicted"] > 0
        W.prepare(s, wl)
        _refused(s, ERR_INVALID, "no completed")                        # the buffers belong to the handle until the next round_prepare
        s.set_deadline(1e-9)                                            # maxSchedulingDuration already expired when the round starts
        with pytest.raises(SchedError) as e:
            s.schedule_round()
        assert e.value.code == B.ERR_TIMEOUT
        _refused(s, ERR_INVALID, "timed out")
        s.set_deadline(0)
        W.prepare(s, wl)
        s.schedule_round()
        assert s.round_evictor_report()["num_evicted"] > 0
        s.round_exchange()                                              # the queue-hash mode's resolve (world size 1)
        _refused(s, ERR_UNSUPPORTED, "round_exchange")
        s.set_evictor_report(False)
        _refused(s, ERR_INVALID, "switched off")
        s.close()


def test_market_driven_handle_is_refused(libs):
    wl = W.small_random(n_nodes=31, n_jobs=480, n_queues=5, seed=7003, occupied=1.0, gangs=3)
    bids = np.random.default_rng(11).integers(0, 4, size=wl.num_jobs).astype(np.float64)
    for g in set(int(x) for x in wl.job_gang if x >= 0):
        m = np.nonzero(wl.job_gang == g)[0]
        bids[m] = bids[m[0]]
    bids[(wl.job_node >= 0) & np.array([not wl.config.pc_preemptible[p] for p in wl.job_pc])] = 1_000_000.0
    for lib in libs:
        if lib is None:
            continue
        s = W.load(lib, wl)
        W.set_jobs(s, wl, bid_price=bids)
        pcp = np.asarray(wl.config.pc_priority)
        queued = [sorted(q, key=lambda j: (-int(pcp[wl.job_pc[j]]), -float(bids[j]), int(wl.job_submit[j]), int(j))) for q in wl.queued]
        nq = wl.num_queues
        s.round_prepare(wl.queue_weight, queued, global_tokens=float(wl.global_burst), global_burst=wl.global_burst, global_rate_inf=wl.rate_inf,
                        queue_tokens=[float(wl.queue_burst)] * nq, queue_burst=[wl.queue_burst] * nq, queue_rate_inf=[wl.rate_inf] * nq)
        s.set_market(True, 0.3)
        s.set_evictor_report(True)
        _refused(s, ERR_UNSUPPORTED, "market-driven")
        s.schedule_round()
        _refused(s, ERR_UNSUPPORTED, "market-driven")
        s.close()


def test_library_without_the_entry_points_says_so(oracle_lib):
    wl = _config4(2)
    s = W.load(oracle_lib, wl)
    for call in (s.set_evictor_report, s.round_evictor_report):
        with pytest.raises(SchedError) as e:
            call()
        assert "does not export" in str(e.value)
    s.close()


# ---------------------------------------------------------------- f. the switch off changes nothing
def test_switch_off_launches(libs):
    wl = _config4(0)
    for lib in libs:
        if lib is None:
            continue
        n, rounds = [], []
        for on in (False, True, False):
            s = W.load(lib, wl); W.prepare(s, wl)
            if on:
                s.set_evictor_report(True)
            rounds.append(s.schedule_round())
            n.append(s.round_timing()["launches"])
            s.close()
        assert n[0] == n[2] == n[1] - REPORT_LAUNCHES and n[0] > 10, n
        scenario.assert_same_round(rounds[0], rounds[1])
