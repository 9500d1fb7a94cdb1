"""Bulk-merged stream runs that go on across a queue whose stream ends at the queue's own rate-limit tokens (armada_amd/csrc/round_merge.h MG_F_LIMIT, DESIGN.md 3.1
round 7).  The element behind the last token is the queue's *limit element*: it gets QueueRateLimitExceeded, the job behind it is peeked and stashed, the queue is
restricted to evicted jobs and leaves the heap (constraints.go:25-58, queue_scheduler.go:213-220, 338-350, 546-566) — the run carries it through the ring as an entry with
nothing to select or bind and settles the queue when it ends, instead of ending at it.

Every round is compared with the oracle bit for bit (scenario.assert_same_round), with the feature on and off (HS_NO_STREAM_LIMIT / ASCHED_STREAM_LIMIT=0), the bulk
merge taking runs of 64 entries and more (HS_MG_MIN / ASCHED_MERGE_MIN), and on the CPU build again with a node engine that lags behind the merge (HS_RING_LAG).  The
shapes are the smallest at which each part can go wrong; the oracle's rounds are computed once per case.
"""
import numpy as np
import pytest

from armada_amd import workloads as W
from scenario import assert_same_round

QUEUE_RATE_LIMIT = 4     # include/armada_sched.h ASCHED_REASON_QUEUE_RATE_LIMIT
GLOBAL_RATE_LIMIT = 3    # ASCHED_REASON_GLOBAL_RATE_LIMIT
SKIPPED_UNFEASIBLE_KEY = 17
N_JOBS, N_QUEUES = 16000, 24


class Case:
    """a workload and its per-queue limiters (W.prepare gives every queue the same)"""
    def __init__(self, wl, tokens=None, inf=None):
        q = wl.num_queues
        self.wl = wl
        self.tokens = [float(wl.queue_burst)] * q if tokens is None else [float(t) for t in tokens]
        self.inf = [wl.rate_inf] * q if inf is None else list(inf)

    def run(self, lib):
        wl = self.wl
        s = W.load(lib, wl)
        s.round_prepare(wl.queue_weight, wl.queued, global_tokens=float(wl.global_burst), global_burst=wl.global_burst, global_rate_inf=wl.rate_inf,
                        queue_tokens=self.tokens, queue_burst=[wl.queue_burst] * wl.num_queues, queue_rate_inf=self.inf)
        r = s.schedule_round()
        st = s.round_stats()
        s.close()
        return r, st

    def limit_job(self, want, q):
        """the job of queue q that the oracle's round `want` gave QueueRateLimitExceeded: the queue's limit element"""
        ids = self.wl.queued[q]
        hit = ids[np.asarray(want.job_unschedulable_reason)[ids] == QUEUE_RATE_LIMIT]
        assert len(hit) == 1
        return int(hit[0])


def base(seed=1200, gangs=0, occupied=0.5, queue_burst=200, global_burst=N_JOBS // 3, lookback=0):
    wl = W.config3(seed=seed, n_nodes=1200, n_jobs=N_JOBS, n_queues=N_QUEUES, gangs=gangs, occupied=occupied)
    wl.global_burst, wl.queue_burst, wl.rate_inf = global_burst, queue_burst, False
    if lookback:
        wl.config.max_queue_lookback = lookback
    return wl


def _many_limits():        # many queues reach their limit inside one run
    return Case(base())


def _tokens_equal_list():  # tokens == the queue's remaining list length, exactly: no limit element, the list just ends
    wl = base()
    return Case(wl, tokens=[len(wl.queued[q]) if 1 <= len(wl.queued[q]) <= 600 else 200 for q in range(N_QUEUES)])


def gang_behind(wl, q, p, gid):
    """the two jobs behind list position p' >= p of queue q become gang gid (members of a gang share shape and priority class: the first p' at which they share the class
    already, so that the list stays in scheduling order); returns p'.  With p' tokens the queue's limit element is position p' and the job peeked behind it a gang member."""
    ids = wl.queued[q]
    while wl.job_pc[ids[p + 1]] != wl.job_pc[ids[p + 2]]:
        p += 1
    a, b = int(ids[p + 1]), int(ids[p + 2])
    wl.job_gang[[a, b]] = gid
    wl.job_gang_card[[a, b]] = 2
    wl.job_req[b] = wl.job_req[a]
    return p


def _gang_behind_cut():    # the job behind EVERY queue's limit element is a gang member: every stream stays open, as without the feature
    wl = base()
    tokens, gid = [], 0
    for q in range(N_QUEUES):
        n = len(wl.queued[q])
        if n < 300:
            tokens.append(n if n >= 1 else 200)      # the list ends with the tokens: no limit element
        else:
            tokens.append(gang_behind(wl, q, 150 + q, gid))
            gid += 1
    assert gid >= 10
    return Case(wl, tokens=tokens)


def _zero_tokens():        # queues that have no token when the run starts
    wl = base()
    return Case(wl, tokens=[0 if q % 5 == 1 else (0.5 if q % 5 == 2 else 200) for q in range(N_QUEUES)])


def _lookback_at_limit():  # the lookback limit is reached at the limit element / at the job the branch peeks behind it
    return Case(base(lookback=201))


def _lookback_before_limit():
    return Case(base(lookback=200))


def _lookback_behind_limit():
    return Case(base(lookback=202))


def crowded(global_burst=N_JOBS // 3):   # a crowded cluster: scheduling keys are registered as unfeasible while queues reach their limits
    return base(occupied=0.93, queue_burst=120, global_burst=global_burst)


def _unfeasible_keys():
    return Case(crowded())


def gang_q0(global_burst=N_JOBS // 3):   # queue 0 has 150 tokens (or a few more) and a gang directly behind its limit element; the other queues carry theirs
    wl = base(global_burst=global_burst)
    tokens = [200.0] * N_QUEUES
    tokens[0] = gang_behind(wl, 0, 150, 0)
    return Case(wl, tokens=tokens)


def _inf_mix():            # queues without a rate limit next to limited ones
    wl = base()
    return Case(wl, inf=[q % 3 == 0 for q in range(N_QUEUES)])


def _burst_one():
    return Case(base(queue_burst=1))


CASES = {f.__name__[1:]: f for f in (_many_limits, _tokens_equal_list, _gang_behind_cut, _zero_tokens, _lookback_at_limit, _lookback_before_limit, _lookback_behind_limit,
                                     _unfeasible_keys, _inf_mix, _burst_one)}


_EDGE = {}
EDGE_MAKERS = {"plain": lambda g: Case(base(global_burst=g)), "gang": gang_q0}


def _global_edge(oracle, kind):
    """(n, limit job).  n = the number of new jobs the oracle schedules before queue 0's limit element has its turn: with n global
    tokens the last one goes to the entry just in front of the limit element (which then meets the global limiter first and must NOT get its queue's reason), with n + 1 the
    limit element passes the global check and every further token goes to an entry BEHIND it in the same run.  Found with the oracle alone: the reason of that job is
    monotone in the global burst."""
    if kind in _EDGE:
        return _EDGE[kind]
    make = EDGE_MAKERS[kind]
    c = make(N_JOBS // 3)
    lim_job = c.limit_job(c.run(oracle)[0], 0)

    def queue_reason(g):
        r, _ = make(g).run(oracle)
        return int(r.job_unschedulable_reason[lim_job]) == QUEUE_RATE_LIMIT
    lo, hi = 1, N_JOBS // 3
    assert not queue_reason(lo)
    while lo + 1 < hi:           # lo: not the queue's reason, hi: the queue's reason
        mid = (lo + hi) // 2
        if queue_reason(mid):
            hi = mid
        else:
            lo = mid
    _EDGE[kind] = (lo, lim_job)
    return _EDGE[kind]


# the global tokens run out on the entry just in front of queue 0's limit element (0), on the limit element (1), and on entries behind it in the same run (2, 40): the
# limit job's reason and the round's end as the oracle's — also where the element is not carried because a gang member stands behind it (the per-job iteration must
# then meet it with the global tokens of ITS turn, not of the end of the run)
EDGE_CASES = {}
for _kind, _ds in (("plain", (0, 1, 2)), ("gang", (0, 1, 2, 40))):
    for _d in _ds:
        _name = ("global_tokens_end_%d" % _d) if _kind == "plain" else "%s_global_tokens_end_%d" % (_kind, _d)
        EDGE_CASES[_name] = (_kind, _d)
        CASES[_name] = (lambda kind, d: lambda oracle: EDGE_MAKERS[kind](_global_edge(oracle, kind)[0] + d))(_kind, _d)


_ORACLE_ROUNDS = {}


def case_and_oracle(name, oracle):
    """the case and the oracle's round of it: computed once, shared by every test of the case, never changed"""
    if name not in _ORACLE_ROUNDS:
        c = CASES[name](oracle) if name in EDGE_CASES else CASES[name]()
        _ORACLE_ROUNDS[name] = (c, c.run(oracle)[0])
    return _ORACLE_ROUNDS[name]


def on_off(lib, oracle, name, monkeypatch, min_var, off_var, off_val):
    c, want = case_and_oracle(name, oracle)
    monkeypatch.setenv(min_var, "64")
    monkeypatch.delenv(off_var, raising=False)
    r_on, st_on = c.run(lib)
    assert_same_round(r_on, want)
    monkeypatch.setenv(off_var, off_val)
    r_off, st_off = c.run(lib)
    assert_same_round(r_off, want)
    return oracle, c, want, st_on, st_off


def check_case(name, oracle, c, want, st_on, st_off):
    print(f"{name}: stream_runs on {st_on['stream_runs']} off {st_off['stream_runs']}, stream_jobs on {st_on['stream_jobs']} off {st_off['stream_jobs']}")
    assert st_off["stream_runs"] > 0
    if name == "many_limits":
        assert st_on["stream_runs"] < st_off["stream_runs"]
        assert (np.asarray(want.job_unschedulable_reason) == QUEUE_RATE_LIMIT).sum() >= 10      # the case is what it says: many queues hit their limit
    reasons = np.asarray(want.job_unschedulable_reason)
    if name in EDGE_CASES:
        kind, _ = EDGE_CASES[name]
        n, lim_job = _global_edge(oracle, kind)
        assert int(reasons[lim_job]) == (QUEUE_RATE_LIMIT if c.wl.global_burst > n else GLOBAL_RATE_LIMIT)
        assert (reasons == GLOBAL_RATE_LIMIT).any()                 # the global tokens run out in this round
        ids = c.wl.queued[0]
        behind = int(ids[list(ids).index(lim_job) + 1])
        assert (c.wl.job_gang[behind] >= 0) == (kind == "gang")     # the job that the rate-limit branch peeks is a gang member
    if name == "gang_behind_cut":
        for q in range(N_QUEUES):                                   # every queue that is cut at its tokens has a gang member behind its limit element ...
            ids = c.wl.queued[q]
            if len(ids) > c.tokens[q]:                              # (a job that found no node in front of it moves the limit element on to the gang itself)
                i = int(np.nonzero(reasons[ids] == QUEUE_RATE_LIMIT)[0][0])
                assert i >= c.tokens[q] and (c.wl.job_gang[ids[i]] >= 0 or c.wl.job_gang[ids[i + 1]] >= 0)
        assert (reasons == QUEUE_RATE_LIMIT).sum() >= 10
        assert st_on["stream_runs"] == st_off["stream_runs"] and st_on["stream_jobs"] == st_off["stream_jobs"]   # ... so no run goes on across one
    if name == "unfeasible_keys":
        assert (reasons == SKIPPED_UNFEASIBLE_KEY).any() and (reasons == QUEUE_RATE_LIMIT).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_limit_element_rounds_equal_oracle(hostsim_lib, oracle_lib, name, monkeypatch):
    check_case(name, *on_off(hostsim_lib, oracle_lib, name, monkeypatch, "HS_MG_MIN", "HS_NO_STREAM_LIMIT", "1"))


@pytest.mark.parametrize("lag", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_limit_element_rounds_with_a_lagging_engine(hostsim_lib, oracle_lib, name, lag, monkeypatch):
    monkeypatch.setenv("HS_RING_LAG", str(lag))
    on_off(hostsim_lib, oracle_lib, name, monkeypatch, "HS_MG_MIN", "HS_NO_STREAM_LIMIT", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_limit_element_rounds_gpu(hip_lib, oracle_lib, name, monkeypatch):
    check_case(name, *on_off(hip_lib, oracle_lib, name, monkeypatch, "ASCHED_MERGE_MIN", "ASCHED_STREAM_LIMIT", "0"))
