"""A gang placed NESTED in a running stream run (armada_amd/csrc/round_fast.h streamNestSettle / streamNestGang -> fastGangRun -> fastStreamPrepareOne; DESIGN.md 3.1
rounds 5 and 12), with and without a lookback limit, at 64 queues or fewer.

The regression: the `streams` soak's seed 100933.  A stream run's ring lies over the queues' prefetch windows of job records (4 records per queue: ring entry i is
record i % 4 of queue i / 4's window).  A queue whose head was an assembled gang when a run began is never settled inside that run, so its record went on calling valid
the window a per-job iteration had filled before the run; a gang of two or three members leaves the list position behind it inside that window; and when the gang was
placed nested, the queue's next head was read out of the window — by then ring entry 4 q + w, a job of another queue that had been placed already.  The job really there
was passed over: never scheduled, no reason, nothing downstream reports it.  Every round here is compared with the oracle bit for bit (scenario.assert_same_round) and
checked against the invariant that needs no oracle (scenario.assert_no_job_passed_over), which the oracle's own round is asserted to satisfy in the same test.

The lookback limit is not part of the cause; it is what makes the regression round's runs end early (a queue's stream ends at the limit, the run with it), so that per-job
iterations fill windows between runs.  The hand-made cases are one-priority-class pools (a queue's list is its jobs in submit order, so list positions can be written
down) with gangs placed by position.  `nested_gangs` (round_stats word 22, filled by the CPU build alone) is how a CPU test knows that a round placed a gang nested: each
case asserts it, and one test turns the nested path off (HS_NO_GANG_NEST) and asserts the same round with a count of 0.  The GPU tests run the same cases through the HIP
library against the same oracle rounds; that the inputs reach the nested path is what the CPU tests pin.  The oracle's round of a case is computed once and shared.
"""
import numpy as np
import pytest

from armada_amd import workloads as W
from scenario import assert_no_job_passed_over, assert_same_round, jobs_passed_over


# ---------------------------------------------------------------------------------------------------------------- the regression round
def _seed_100933(lookback):
    wl = W.config3(seed=100933, n_nodes=1011, n_jobs=5123, n_queues=22, gangs=50, occupied=0.2)
    wl.global_burst, wl.queue_burst, wl.rate_inf = 500, 5123, True
    wl.config.max_queue_lookback = lookback
    return wl


# ---------------------------------------------------------------------------------------------------------------- hand-made pools
def _pool(seed=5, n_nodes=120, n_jobs=900, n_queues=8, lookback=0):
    """An empty pool, queues of equal weight, ONE priority class and ONE request: queue q's list is its queued jobs in id order, and the queues advance in lockstep —
    every queue is served once per cycle (ties go by queue index) until something sets one apart: a gang costs its whole request at once and waits about a cycle longer.
    So what a run has done when a queue reaches its gang can be written down from list positions."""
    wl = W.config3(seed=seed, n_nodes=n_nodes, n_jobs=n_jobs, n_queues=n_queues, gangs=0, occupied=0.0)
    assert (wl.job_node < 0).all()
    wl.job_pc[:] = 0
    wl.job_req[:] = SMALL
    wl.queue_weight[:] = 1.0
    wl.queued = [np.sort(ids) for ids in wl.queued]
    wl.global_burst, wl.queue_burst, wl.rate_inf = n_jobs, n_jobs, True
    wl.config.max_queue_lookback = lookback
    return wl


def _gang(wl, q, pos, card, positions=None, req=None):
    """the jobs at list positions pos .. pos + card - 1 of queue q become one gang (positions: the members' own list positions, for a gang with members apart)"""
    members = wl.queued[q][list(positions) if positions is not None else list(range(pos, pos + card))]
    assert len(members) == card and (wl.job_gang[members] < 0).all(), "gang members overlap or run off the end of the queue's list"
    wl.job_gang[members] = int(wl.job_gang.max()) + 1
    wl.job_gang_card[members] = card
    wl.job_req[members] = wl.job_req[members[0]] if req is None else np.asarray(req, dtype=np.int64)
    return wl


SMALL = [4 * W.Gi, 1000, 10 * W.Gi, 0]      # a request on the index grid that fits everywhere in a roomy pool
TOO_BIG = [256 * W.Gi, 64000, 1024 * W.Gi, 0]      # twice a node's cpu: a member finds no node


def _single_behind(card=2, lookback=0, q=3, pos=3):
    return _gang(_pool(lookback=lookback), q, pos, card, req=SMALL)


def _last_job_behind():
    wl = _pool()
    q = len(wl.queued) - 1           # the shortest list: the run gets to its end
    n = len(wl.queued[q])
    return _gang(wl, q, n - 3, 2, req=SMALL)


def _gang_behind():
    wl = _pool()
    return _gang(_gang(wl, 3, 3, 2, req=SMALL), 3, 5, 3, req=SMALL)


def _refused_gang_behind():
    wl = _pool()
    return _gang(_gang(wl, 3, 3, 2, req=SMALL), 3, 0, 2, positions=(5, 7), req=SMALL)   # members apart: fastPeekGang leaves it to the generic iterator


def _member_without_node():
    wl = _pool()
    return _gang(_gang(wl, 3, 3, 2, req=TOO_BIG), 5, 2, 2, req=SMALL)   # (queue 5's gang is the one that is placed nested)


def _two_queues():
    wl = _pool()
    return _gang(_gang(wl, 3, 3, 2, req=SMALL), 4, 3, 2, req=SMALL)


def _tokens_run_out_behind():
    # every queue has 5 rate-limit tokens: queue 3 spends them on three single jobs and the gang's two members, the first job behind the gang meets none.  The run is
    # merged by the control wave: mgPrepare (round_merge.h) refuses every run that would nest a gang — a gang member behind a queued stream, an assembled gang at a
    # queue's head — so the limit element of the bulk-merged runs is never carried in front of a gang member; that refusal is what protects this round
    wl = _gang(_pool(), 3, 3, 2, req=SMALL)
    wl.queue_burst, wl.rate_inf = 5, False
    return wl


CASES = {
    "single_behind_card2": lambda: _single_behind(2),
    "single_behind_card3": lambda: _single_behind(3),
    "single_behind_card64": lambda: _single_behind(64, q=0),
    "last_job_behind": _last_job_behind,
    "gang_behind": _gang_behind,
    "refused_gang_behind": _refused_gang_behind,
    "member_without_node": _member_without_node,
    "two_queues": _two_queues,
    "tokens_run_out_behind": _tokens_run_out_behind,
}
# the lookback limit L lets a queue's iterator peek list positions 0 .. L - 1; the gang of three stands at positions 6, 7, 8 of queue 3 (queue 5's gang at 1, 2 is within
# every limit): the limit on the job in front of the gang (L = 6: position 5 is the last one peeked), inside it (7, 8), on its last member (9), on the first (10) and on
# the second job behind it (11), and one beyond
def _lookback_pair(L):
    return _gang(_single_behind(3, lookback=L, q=3, pos=6), 5, 1, 2, req=SMALL)


for _L in (5, 6, 7, 8, 9, 10, 11, 12):
    CASES[f"lookback_{_L}"] = (lambda L: lambda: _lookback_pair(L))(_L)
CASES["no_lookback"] = lambda: _lookback_pair(0)   # the control: the same pair of gangs, no limit at all



# ---- the trigger itself.  When queue t's gang is placed nested, (1) t's record calls valid a prefetch window that holds the list position behind the gang's last member
# at slot w, and (2) the session's ring has reached that slot: more than 4 t + w entries emitted.  For (1) the queue must have got its gang as head OUTSIDE a run (a queue
# settled inside a run has its window struck): a gang with members apart at position x of another queue ends the first run (the generic iterator takes it), the per-job
# iterations of the back-off serve queue t's last single jobs in front of its gang and peek the gang, and the next run starts with the gang as queue t's head.  The gang
# costs its whole request at once, so the other queues are served once more before it.  What the CPU build had at the nested gang before round 12, printed from
# streamNestGangBody:
#     card2           queue 1  window at the gang, position behind it in slot 2: ring entry  6, 11 emitted   LOST the job at list position 5
#     card3           queue 1  window at the gang,                       slot 3: ring entry  7, 11 emitted   LOST (position 6)
#     queue0_card2    queue 0                                            slot 2: ring entry  2, 12 emitted   LOST (position 5)
#     members_apart   queue 1  (its gang, members at 1 and 3, assembled by the GENERIC iterator) slot 1: ring entry 5, 6 emitted   LOST (position 4)
#     card4           queue 1  window at the gang: the position behind a gang of four is outside the window of four           same round
#     queue2          queue 2  window one in front of the gang,          slot 3: ring entry 11, 10 emitted: not reached      same round
#     gang_two_later  queue 1  the second run begins before the gang is the head: the queue is settled inside it, no window   same round
def _trigger(t=1, k=3, c=2, x=1, n_queues=16):
    wl = _pool(n_queues=n_queues, n_jobs=60 * n_queues)
    _gang(wl, t, k, c, req=SMALL)
    return _gang(wl, (t + 3) % n_queues, 0, 2, positions=(x, x + 2), req=SMALL)


TRIGGER = {
    "trigger_card2": lambda: _trigger(c=2),
    "trigger_card3": lambda: _trigger(c=3),
    "trigger_queue0_card2": lambda: _trigger(t=0, c=2),
    "trigger_members_apart": lambda: _trigger(t=6, k=6, c=4, n_queues=8),
    "trigger_card4_outside_window": lambda: _trigger(c=4),
    "trigger_queue2_ring_not_there": lambda: _trigger(t=2, c=2),
    "trigger_gang_two_later": lambda: _trigger(k=5, c=2),
}
CASES.update(TRIGGER)

REGRESSION = {f"seed_100933_lookback_{L}": (lambda L: lambda: _seed_100933(L))(L) for L in (10, 20, 30, 50, 80)}   # 20, 30, 50 lost job 6067; 10 and 80 are the neighbours that passed
BUILDERS = {**CASES, **REGRESSION}
_ORACLE_ROUNDS = {}


def run(lib, wl):
    s = W.load(lib, wl)
    W.prepare(s, wl)
    r = s.schedule_round()
    st = s.round_stats()
    s.close()
    return r, st


def case_and_oracle(name, oracle):
    """the workload and the oracle's round of it: computed once, shared, never changed.  The invariant holds for the oracle's round (asserted once, here)."""
    if name not in _ORACLE_ROUNDS:
        wl = BUILDERS[name]()
        want = run(oracle, wl)[0]
        assert_no_job_passed_over(wl, want)
        _ORACLE_ROUNDS[name] = (wl, want)
    return _ORACLE_ROUNDS[name]


def check(lib, oracle, name):
    wl, want = case_and_oracle(name, oracle)
    r, st = run(lib, wl)
    print(f"{name}: scheduled {len(want.scheduled)} / {len(r.scheduled)}, passed over {jobs_passed_over(wl, r)[:8]}, stream_runs {st['stream_runs']}, stream_jobs {st['stream_jobs']}, nested_gangs {st['nested_gangs']}")
    assert_no_job_passed_over(wl, r)
    assert_same_round(r, want)
    return wl, want, r, st


def _env(monkeypatch, name):
    """the default configuration: none of the switches that change how a round runs"""
    for v in ("HS_NO_GANG_NEST", "HS_MG_MIN", "ASCHED_MERGE_MIN"):
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------------------------------------------------------- CPU build
@pytest.mark.parametrize("name", sorted(REGRESSION))
def test_seed_100933_rounds_equal_oracle(hostsim_lib, oracle_lib, name, monkeypatch):
    """default configuration, no HS_* variable set.  Before round 12 the CPU build scheduled 321 / 443 / 883 jobs at lookback 20 / 30 / 50 where the oracle schedules
    322 / 444 / 884: job 6067 (queue 8, list position 5, directly behind the two-member gang at positions 3 and 4) was passed over"""
    _env(monkeypatch, name)
    _, _, _, st = check(hostsim_lib, oracle_lib, name)
    assert st["stream_runs"] > 0
    if name != "seed_100933_lookback_10":   # (at 10 every queue is at its limit before a gang is reached inside a run: the neighbour below the three that failed)
        assert st["nested_gangs"] > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_nested_gang_rounds_equal_oracle(hostsim_lib, oracle_lib, name, monkeypatch):
    _env(monkeypatch, name)
    _, want, _, st = check(hostsim_lib, oracle_lib, name)
    assert st["stream_runs"] > 0 and st["nested_gangs"] > 0, "the round placed no gang nested in a run: the case does not test what it names"
    if name == "two_queues":
        assert st["nested_gangs"] >= 2


def test_nested_path_off_is_the_same_round(hostsim_lib, oracle_lib, monkeypatch):
    """HS_NO_GANG_NEST (read per call): a run ends where a queue's stream ends at a gang, as before round 5 — the same round, no gang placed nested"""
    name = "single_behind_card2"
    _env(monkeypatch, name)
    _, _, _, st_on = check(hostsim_lib, oracle_lib, name)
    monkeypatch.setenv("HS_NO_GANG_NEST", "1")
    _, _, _, st_off = check(hostsim_lib, oracle_lib, name)
    assert st_on["nested_gangs"] > 0 and st_off["nested_gangs"] == 0 and st_off["stream_runs"] > 0


# ---------------------------------------------------------------------------------------------------------------- HIP library
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_nested_gang_rounds_equal_oracle_gpu(hip_lib, oracle_lib, name, monkeypatch):
    _env(monkeypatch, name)
    _, _, _, st = check(hip_lib, oracle_lib, name)
    assert st["stream_runs"] > 0
