"""The short path of the split node engine (armada_amd/csrc/engine_hc.h): a placement the hot set wins outright — its candidate lies below the
shape's clean-side bound and the cold set's lower bound does not lie below it — skips the general body of the per-job loop.  It must choose exactly what the general body
chooses, so every round is compared with the oracle bit for bit (scenario.assert_same_round), with the path on and off (ASCHED_HC_SHORT=0), the bulk merge taking runs of
64 entries and more (ASCHED_MERGE_MIN) so that small rounds reach the split engine at all.

The split engine is device code only: the CPU build runs the serial engine, so the path itself is exercised by the GPU tests alone.  What the CPU build can and does pin
(test_inputs_reach_stream_runs) is that every input yields bulk-merged stream runs with a few hundred placements — the GPU assertion `hc_short_picks > 0` is not vacuous.
The shapes are the smallest that still reach the states that can go wrong; the oracle's rounds are computed once per case.
"""
import numpy as np
import pytest

from armada_amd import workloads as W
from scenario import assert_same_round


def _bursts(wl, n_jobs):
    """the rate-limit bursts of BASELINE configs[2], scaled with the number of queued jobs as bench.py scales them"""
    scale = n_jobs / 1_000_000.0
    wl.global_burst, wl.queue_burst, wl.rate_inf = max(1, int(200_000 * scale)), max(1, int(20_000 * scale)), False
    return wl


def _both_shape_sets():
    # 64 shapes x the 5 % GPU requests: more than 64 fit shapes (both register sets of HcShapes); 4 000 placements leave more than 48 dirty nodes alive, so the hot set
    # hands entries over and lanes are in flight while later jobs are decided; cold-set questions and base picks are interleaved with short picks
    return _bursts(W.config3(seed=811, n_nodes=2_000, n_jobs=20_000, n_queues=8), 20_000)


def _one_shape_set():
    # 16 shapes, no non-indexed request: the smallest pool
    wl = W.config2(seed=812, n_nodes=300, n_jobs=3_000, n_queues=4)
    wl.global_burst, wl.queue_burst, wl.rate_inf = 1_500, 600, False
    return wl


def _entries_die():
    # a crowded pool and bursts that cover every queued job: the nodes fill up, lanes die in the in-place update, and the run ends on a job that fits nowhere (the
    # generic code finishes the round).  70 % occupied: at 90 % nearly every job needs preemption from the start and the round's stream runs bind 44 jobs in all (CPU
    # build) — none of them long enough for the bulk merge; at 70 % one run places some 450 jobs before the nodes are full
    wl = W.config3(seed=813, n_nodes=200, n_jobs=4_000, n_queues=4, occupied=0.7)
    wl.global_burst, wl.queue_burst, wl.rate_inf = 4_000, 4_000, False
    return wl


def _cold_set_wins():
    # every queue's requests alternate between the largest and the smallest shape: the large ones open new nodes, the small ones go back to old fragments, of which
    # far more than 48 stay alive — the cold set's bound lies below the hot candidate (and is unknown, 0, for a shape's first job)
    wl = _bursts(W.config3(seed=814, n_nodes=1_000, n_jobs=10_000, n_queues=8), 10_000)
    big = np.array([32 * W.Gi, 8000, 200 * W.Gi, 0], dtype=np.int64)
    small = np.array([4 * W.Gi, 1000, 10 * W.Gi, 0], dtype=np.int64)
    for ids in wl.queued:
        wl.job_req[ids[0::2]] = big
        wl.job_req[ids[1::2]] = small
    return wl


def _gangs_through_the_ring():
    # the workload of smoke() on a pool 30 % occupied: sessions opened by fastGangRun (the serial engine) next to bulk-merged runs (at smoke()'s 80 % the round's
    # stream runs bind 18 jobs in all: no run reaches the bulk merge)
    return W.small_random(n_nodes=200, n_jobs=3000, n_queues=6, seed=7, occupied=0.3, gangs=6, burst=(1500, 600))


CASES = {f.__name__[1:]: f for f in (_both_shape_sets, _one_shape_set, _entries_die, _cold_set_wins, _gangs_through_the_ring)}
_ORACLE_ROUNDS = {}


def run(lib, wl):
    s = W.load(lib, wl)
    W.prepare(s, wl)
    r = s.schedule_round()
    st = s.round_stats()
    s.close()
    return r, st


def case_and_oracle(name, oracle):
    """the workload and the oracle's round of it: computed once, shared, never changed"""
    if name not in _ORACLE_ROUNDS:
        wl = CASES[name]()
        _ORACLE_ROUNDS[name] = (wl, run(oracle, wl)[0])
    return _ORACLE_ROUNDS[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_reach_stream_runs(hostsim_lib, oracle_lib, name, monkeypatch):
    """CPU build: the input yields bulk-merged stream runs with a few hundred placements (what the split engine serves on the device) and the oracle's round"""
    wl, want = case_and_oracle(name, oracle_lib)
    monkeypatch.setenv("HS_MG_MIN", "64")
    r, st = run(hostsim_lib, wl)
    assert_same_round(r, want)
    print(f"{name}: scheduled {len(want.scheduled)}, stream_runs {st['stream_runs']}, stream_jobs {st['stream_jobs']}")
    assert st["stream_runs"] > 0 and st["stream_jobs"] >= 300 and len(want.scheduled) >= 300
    assert st["hc_short_picks"] == 0      # the CPU build has no split engine
    if name == "entries_die":
        assert len(want.scheduled) < sum(len(q) for q in wl.queued)      # jobs that fit nowhere


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_short_path_rounds_equal_oracle_gpu(hip_lib, oracle_lib, name, monkeypatch):
    wl, want = case_and_oracle(name, oracle_lib)
    monkeypatch.setenv("ASCHED_MERGE_MIN", "64")
    monkeypatch.delenv("ASCHED_HC_SHORT", raising=False)
    r_on, st_on = run(hip_lib, wl)
    assert_same_round(r_on, want)
    monkeypatch.setenv("ASCHED_HC_SHORT", "0")
    r_off, st_off = run(hip_lib, wl)
    assert_same_round(r_off, want)
    print(f"{name}: stream_runs {st_on['stream_runs']}, stream_jobs {st_on['stream_jobs']}, hc_short_picks on {st_on['hc_short_picks']} off {st_off['hc_short_picks']}")
    assert st_on["stream_runs"] == st_off["stream_runs"] > 0 and st_on["stream_jobs"] == st_off["stream_jobs"]
    assert st_on["hc_short_picks"] > 0
    assert st_off["hc_short_picks"] == 0
