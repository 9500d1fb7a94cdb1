"""The key order of the hot set (armada_amd/csrc/hc_order.h, engine_hc.h): every lane of the engine wave keeps the set of lanes whose entry has a
smaller key, patched where a lane's key changes (the in-place bind, an entry dying, the insert into a free lane, the release of lanes handed to the cold set) and asked by
two ballots per job.  A wrong or stale bit makes first fit name another node than the 64-lane minimum did, so every round is compared with the oracle bit for bit.

The split engine is device code only, so the file follows tests/test_z_hc_engine_edges.py (whose pool builders it imports): on the CPU build the round equals the oracle's, the
input reaches bulk-merged stream runs of a few hundred placements (HS_MG_MIN=64), and the states the case is about are COUNTED from the oracle's round; on the GPU the
product library computes the round three times (default, ASCHED_HC_SHORT=0, ASCHED_ENGINE_HC=0), each with a deadline and each bit-identical to the oracle's.

Every pool has ONE queue and bursts that cover it, so jobs are placed in index order and the oracle's job -> node map can be replayed (`_replay`): free resources per node,
the dirty nodes alive (touched in this round and still able to host the smallest request: what H and C hold between them), and their order by key — the indexed columns'
quotients in the configured order, then the node index.  Counted per case:
  jumps     placements on a live dirty node after which that node stands at least two places further down in key order: the lane's bit changes in several words at once,
            and its own word loses several bits
  passed    placements on a live dirty node that is NOT the smallest in key order: the job fits only some lanes, the answer is not the lane with an empty word
  deaths    placements that leave the node unable to host anything: the lane's key becomes ~0 and the next job is served by what was second
  no_fit    placements of a small job on a clean node while dirty nodes are alive: the job fits no lane of H (nor of C) and falls through to the clean side
  max_alive the most dirty nodes alive at once: beyond 48 (HC_H_MAX) entries are handed to C, released, and come back into freed lanes (HC_D) whose old bits are stale
The recipe is the edges file's: n jobs of 20 or more cores open 32-core nodes and leave fragments, small jobs go back to the fragments; here the openers differ in size
(fragments of 7 to 12 cores and ten of five: distinct key fields, so the order is not the node index's) and jobs of one core alternate with jobs of six, which fit only
some fragments and leave the one they take below the five-core ones.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from armada_amd import workloads as W
from scenario import assert_same_round
from test_z_hc_engine_edges import ARMS, BIG, DEADLINE_S, FILL, NEVER, ONE, _all_indexed, _pool, _two_extras, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = [4 * W.Gi, 6_000, 1 * W.Gi, 0]


def _opener(cores):
    return [32 * W.Gi, cores * 1000, 10 * W.Gi, 0]      # more than half a node: no two share one


def _openers(n):
    # fragments of 12, 11, ... 7 cores in turn, then TEN of five cores: too small for a six-core job, and the last to be touched — the ten are in H whatever n is
    return [_opener(20 + i % 6) for i in range(n - 10)] + [_opener(27)] * 10


def _mixed(n_big, tail, n_nodes=None):
    return _pool(n_nodes if n_nodes is not None else n_big + 60, _openers(n_big) + list(tail), 1)


def _with_gpus(wl):
    # nodes with 2 GPUs; every third small job asks for one and every fifth for 200 GiB of ephemeral storage: with _two_extras both are non-indexed (hcFits<2>), a
    # fragment runs out of GPUs with cores to spare — it stays in key order where it was and fits fewer jobs
    wl.node_total[:, W.GPU] = 2
    small = np.nonzero(wl.job_req[:, W.CPU] <= 6_000)[0]
    wl.job_req[small[::3], W.GPU] = 1
    wl.job_req[small[1::5], W.EPH] = 200 * W.Gi
    return wl


ALT = [ONE, SIX] * 150
# name -> (builder, the least each count must reach on the oracle's round).  The bounds come from the construction, not from a run:
CASES = {
    # 24 fragments of 7 ... 12 cores and ten of five (278 cores), then 150 x (1 + 6) cores.  A one-core job takes the fragment with the fewest cores; a six-core job the
    # smallest with six left, passing the smaller ones (passed), and leaves it with one to five cores (or six, from twelve).  During the first 24 pairs the one-core jobs
    # use at most 24 of the 50 cores of the five-core fragments and the remnants below them, so at least five of the ten stand untouched and every six-core job finds a
    # fragment of 7 ... 12 that no one-core job has touched: the 16 fragments of 7 ... 10 end below five cores, under all the untouched five-core ones (jumps >= 16, passed
    # >= 24), and the one-core job behind each must find it at the front — and uses it up sooner or later (deaths).  Once no fragment has six cores a six-core job opens a
    # clean node with fragments alive (no_fit): 1 050 cores asked for, 278 in fragments, 26 to a new node
    "inversions-e1": (lambda: _mixed(34, ALT), dict(jumps=16, passed=24, deaths=10, no_fit=10)),
    "inversions-e0": (lambda: _all_indexed(_mixed(34, ALT)), dict(jumps=16, passed=24, deaths=10, no_fit=10)),
    # (the argument holds with the extras: an untouched fragment has both GPUs and all its storage, whatever the job asks; later on fragments run out of GPUs first)
    "inversions-e2-gpus": (lambda: _two_extras(_with_gpus(_mixed(34, ALT))), dict(jumps=16, passed=24, deaths=5, no_fit=10)),
    # 20 equal fragments of 12 cores, one-core jobs: each fragment dies at its twelfth job and the thirteenth goes to the next node in index order; five FILLs use up a
    # fragment in one bind.  240 cores in fragments, 355 asked for: every fragment dies
    "lane_dies": (lambda: _pool(40, [BIG] * 20 + [ONE] * 100 + [FILL] * 5 + [ONE] * 195, 1), dict(deaths=20)),
    # fragments of five cores only (openers of 27): every six-core job fits no lane of H while H holds 20 entries, and opens a clean node — which serves the next four
    "no_fitting_lane": (lambda: _pool(80, [_opener(27)] * 20 + [SIX, ONE] * 150, 1), dict(no_fit=5, max_alive=20)),
    # two bulk-merged runs in one round: a job larger than any node ends the first session with H full of entries; the second starts from an empty H (every word 0) after
    # the fold-back, on the same fragments
    "two_runs": (lambda: _mixed(34, ALT[:160] + [NEVER] + ALT[:160]), dict(jumps=16, passed=24, stream_runs=2, unscheduled=[34 + 160])),
}
for n in (47, 48, 49, 112):
    # H at 47 / 48 live entries (never over its size), 49 (the first hand-over and release) and 112 (most entries live in C; the round-robin hand-over wraps): the small
    # jobs go back to the fragments with the fewest cores, wherever they live, so entries of C are picked (HC_D) and return into the lanes the releases freed; the FILL /
    # opener pairs use up 12-core fragments and open nodes, as the edges file's `_returns` does.  n fragments alive before the first small job: max_alive >= n.  The
    # five-core fragments are opened last, so they are in H; at 112 the fragments of seven cores are the oldest and live in C: a six-core job brings one back (HC_D), and it
    # is inserted with one core left, below every five-core lane.  jumps / passed: the argument of "inversions" (n - 10 >= 37 fragments of 7 ... 12, at least 24 of 7 ... 10)
    CASES[f"full_hot_set-{n}"] = (lambda n=n: _mixed(n, [ONE, SIX] * 100 + [FILL, _opener(20)] * 30 + [ONE] * 60, n_nodes=n + 90), dict(jumps=16, passed=24, deaths=10, max_alive=n))
_ORACLE_ROUNDS = {}


def case_and_oracle(name, oracle):
    """the workload and the oracle's round of it: computed once, shared, never changed"""
    if name not in _ORACLE_ROUNDS:
        wl = CASES[name][0]()
        _ORACLE_ROUNDS[name] = (wl, run(oracle, wl)[0])
    return _ORACLE_ROUNDS[name]


def _replay(wl, scheduled):
    """the counts of the module's text, from the oracle's job -> node map (one queue: jobs are placed in index order)"""
    cols, res = list(wl.config.indexed_col), list(wl.config.indexed_resolution)
    free = wl.node_total.astype(np.int64).copy()
    least = wl.job_req.min(axis=0)      # the smallest request per column: a node that cannot host it hosts nothing
    alive = {}      # node -> key, the dirty nodes that can still host something

    def key(n):
        return tuple(int(free[n, c] // r) for c, r in zip(cols, res)) + (n,)

    out = dict(jumps=0, passed=0, deaths=0, no_fit=0, max_alive=0)
    for j in sorted(scheduled):
        n = scheduled[j]
        if n in alive:
            order = sorted(alive.values())
            before = order.index(alive[n])
            out["passed"] += before > 0
        elif alive:
            out["no_fit"] += int(wl.job_req[j, W.CPU] <= 6_000)      # (an opener never fits a fragment: not counted)
        free[n] -= wl.job_req[j]
        assert (free[n] >= 0).all()
        if (free[n] >= least).all():
            was = n in alive
            alive[n] = key(n)
            if was:
                out["jumps"] += before - sorted(alive.values()).index(alive[n]) >= 2
        else:
            alive.pop(n, None)
            out["deaths"] += 1
        out["max_alive"] = max(out["max_alive"], len(alive))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_reach_their_state(hostsim_lib, oracle_lib, name, monkeypatch):
    """CPU build (the serial engine on the same stream runs): the oracle's round, bulk-merged stream runs of a few hundred placements, and the states the case is about"""
    wl, want = case_and_oracle(name, oracle_lib)
    pins = dict(CASES[name][1])
    monkeypatch.setenv("HS_MG_MIN", "64")
    r, st = run(hostsim_lib, wl)
    n_all = sum(len(q) for q in wl.queued)
    got = _replay(wl, want.scheduled)
    print(f"{name}: queued {n_all}, scheduled {len(want.scheduled)}, stream_runs {st['stream_runs']}, stream_jobs {st['stream_jobs']}, l0_max {st['l0_max']}, " + ", ".join(f"{k} {v}" for k, v in got.items()))
    assert_same_round(r, want)
    assert st["stream_runs"] >= pins.pop("stream_runs", 1) and st["stream_jobs"] >= 300 and st["l0_overflows"] == 0
    assert st["hc_short_picks"] == 0      # (the CPU build has no split engine)
    miss = pins.pop("unscheduled", [])
    assert sorted(set(range(n_all)) - set(want.scheduled)) == miss
    for k, least in pins.items():
        assert got[k] >= least, (k, least, got[k])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_order_rounds_equal_oracle_gpu(hip_lib, oracle_lib, name, monkeypatch):
    """product library: the three arms' rounds equal the oracle's, and the split engine served the default arm's runs (hc_short_picks)"""
    wl, want = case_and_oracle(name, oracle_lib)
    monkeypatch.setenv("ASCHED_MERGE_MIN", "64")
    st = {}
    for arm, env in ARMS:
        for v in ("ASCHED_HC_SHORT", "ASCHED_ENGINE_HC"):
            monkeypatch.delenv(v, raising=False)
        for v, x in env.items():
            monkeypatch.setenv(v, x)
        r, st[arm] = run(hip_lib, wl, deadline=DEADLINE_S)
        print(f"{name} [{arm}]: " + ", ".join(f"{k} {st[arm][k]}" for k in ("l0_max", "l0_overflows", "stream_runs", "stream_jobs", "hc_short_picks")))
        assert_same_round(r, want)
    assert st["default"]["hc_short_picks"] > 0
    assert st["short_off"]["hc_short_picks"] == 0 and st["serial"]["hc_short_picks"] == 0
    assert st["default"]["stream_runs"] == st["short_off"]["stream_runs"] == st["serial"]["stream_runs"] > 0
    assert st["default"]["stream_jobs"] == st["short_off"]["stream_jobs"] == st["serial"]["stream_jobs"]
    assert all(s["l0_overflows"] == 0 for s in st.values())


def test_order_model_program(tmp_path):
    """tools/hc_order_model.cpp — 64 simulated lanes over the functions of hc_order.h, every query against the linear scan — built with the host compiler and run"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hc_order_model")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "hc_order_model.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "every query equal to the linear scan" in out.stdout
