"""The edges of the split node engine (armada_amd/csrc/engine_hc.h): the size of the hot set H around HC_H_MAX = 48, the hand-overs to the cold set C and their
back-pressure, the round-robin victim passing lane 63, slots of C given up and reused, the two places where the split engine's list overflows (L0CAP = 1024), the three
instantiations E = 0 / 1 / 2 non-indexed columns, the number of fit shapes at the two register sets (64 / 65) and at the engine's switch (128 / 129), the bitmap words of the
clean side at node counts next to a multiple of 64, and a session that ends on a job that fits nowhere while H is full.

The split engine is device code only: the CPU build runs the serial engine.  So every case is checked twice.  On the CPU build (test_inputs_reach_their_state) the round
equals the oracle's and round_stats pins the state the input reaches — the number of live dirty nodes (l0_max), whether the list overflowed (l0_overflows), the bulk-merged
stream runs and the jobs they bind — so that the GPU test is not vacuous.  On the GPU (test_engine_edges_equal_oracle_gpu) the product library computes each round three times,
every one bit-identical to the oracle's (scenario.assert_same_round): by default, with the short path off (ASCHED_HC_SHORT=0), and on the serial device engine
(ASCHED_ENGINE_HC=0) — the arm that tells "the split engine is wrong" from "the stream run is wrong".  The bulk merge takes runs of 64 entries and more throughout
(HS_MG_MIN / ASCHED_MERGE_MIN).  Every GPU round has a deadline: a protocol defect between the two waves ends as ASCHED_ERR_TIMEOUT, a failed test, not a stuck one.

The recipe for an exact number of live dirty nodes (`_recipe`): an empty pool of 32-core nodes; n_big jobs of 20 cores first, no two of which share a node — each opens a
clean node and leaves a 12-core fragment —, then jobs of one core, which keep the fragments alive.  All fragments carry the same key fields, so first fit goes by node index:
the one-core jobs return to the OLDEST fragment, which lives in C once more than 48 are alive.

Overflow.  The serial engine gives up at the 1025th live dirty node.  The split engine gives up elsewhere: when wave 3's list is full (more than 1024 COLD entries: H's 48 and
the hand-overs in flight are not in it) or at the fold-back of H when the session ends.  Between 1025 and about 1072 live dirty nodes the two overflow at different moments,
or only one of them does; past that, still at different jobs.  Whichever way, the generic scan finishes the round and the round is the oracle's.  So above 1024 the split
arms assert the round (and, at 1200, that the overflow is counted and that short picks were made); their l0_overflows / stream_jobs are printed, not compared: where the
engine learns of wave 3's overflow is a matter of timing between the waves.  The serial arm is deterministic and must count what the CPU build counts.
Measured on the MI355X (split engine; the serial arm: 1 overflow and 1025 jobs in the run from 1025 on, like the CPU build): at 1025 and 1040 NO overflow and every job in
the run — the one-core jobs use up 25 of the oldest fragments before the fold-back, which then fits; at 1072 the run binds every job and the fold-back overflows (1024 cold
entries + 48 in H); at 1073 the 1025th hand-over finds wave 3's list full and the run ends at its 1073rd job, before the first one-core job (hc_short_picks 0).
"""
import numpy as np
import pytest

from armada_amd import workloads as W
from scenario import assert_same_round

BIG = [32 * W.Gi, 20_000, 10 * W.Gi, 0]      # two of them do not fit on one 32-core node
ONE = [4 * W.Gi, 1_000, 1 * W.Gi, 0]
FILL = [4 * W.Gi, 12_000, 1 * W.Gi, 0]       # exactly the fragment a BIG leaves: the node is full afterwards and leaves the list
NEVER = [32 * W.Gi, 40_000, 10 * W.Gi, 0]    # larger than any node
DEADLINE_S = 5.0


def _pool(n_nodes, reqs, n_queues, node=(256 * W.Gi, 32_000, 1024 * W.Gi, 0)):
    """an empty pool (W.config1's shape); job i of `reqs` is the (i // n_queues)-th job of queue i % n_queues; bursts that cover every job"""
    reqs = np.asarray(reqs, dtype=np.int64)
    wl = W.config1(n_nodes=n_nodes, n_jobs=len(reqs), seed=1)
    wl.node_total = np.tile(np.array(node, dtype=np.int64), (n_nodes, 1))
    wl.job_req = reqs
    wl.job_queue = (np.arange(len(reqs)) % n_queues).astype(np.int32)
    wl.queue_weight = np.ones(n_queues)
    wl.queued = [np.arange(q, len(reqs), n_queues, dtype=np.int32) for q in range(n_queues)]
    wl.global_burst, wl.queue_burst, wl.rate_inf = len(reqs), len(reqs), False
    return wl


def _recipe(n_big, n_nodes=None, n_small=300, n_queues=2, tail=()):
    return _pool(n_nodes if n_nodes is not None else n_big + 20, [BIG] * n_big + [ONE] * n_small + list(tail), n_queues)


def _returns(n_big):
    # after the n_big fragments: pairs of a FILL and a BIG.  The FILL takes the oldest fragment — an entry of C, or one still on its way there — and uses it up (HC_D, or
    # HC_C: the slot goes on the free stack); the BIG opens a node, H is over its size again and the hand-over (HC_I) pops that slot.  Never more than n_big alive: each
    # of the two queues gets FILL, BIG, FILL, BIG ... (measured on the CPU build: with [FILL, BIG] dealt out, one queue holds every FILL, the other every BIG, and l0_max
    # is n_big + 1 or + 2).  At n_big = 50 C holds two entries: the two FILLs behind two BIGs want the very entries those BIGs have just handed over — HC_C if wave 3 has
    # not taken them in yet, which is timing: not asserted (on the MI355X it had: profiles/r13_hc_engine_edges.txt).
    pairs = [FILL, FILL, BIG, BIG] * 75
    return _pool(n_big + 170, [BIG] * n_big + pairs + [ONE] * 100, 2)


def _all_indexed(wl):
    # E = 0: four indexed columns in W.default_indexed's order; its resolutions (100m, 100Mi) would put these pools' GiB requests off the index grid (literal iteration, no
    # fast structure), so the columns keep resolutions the requests are multiples of
    wl.config.indexed_col = [W.GPU, W.CPU, W.MEM, W.EPH]
    wl.config.indexed_resolution = [1, 1000, 128 * W.Mi, W.Gi]
    return wl


def _two_extras(wl):
    # E = 2: ephemeral storage and GPUs are checked beside the key (hcFits<2>: ex0, ex1; the base's second extra column at baseExtra[Npad + q])
    wl.config.indexed_col = [W.CPU, W.MEM]
    wl.config.indexed_resolution = [1000, 128 * W.Mi]
    return wl


def _recipe_gpus(n_big):
    # the recipe on nodes with 2 GPUs; every third one-core job asks for one: a fragment runs out of GPUs (the second extra) with cores to spare, and stays alive
    wl = _recipe(n_big)
    wl.node_total[:, W.GPU] = 2
    small = np.nonzero(wl.job_req[:, W.CPU] == 1_000)[0]
    wl.job_req[small[::3], W.GPU] = 1
    wl.job_req[small[1::3], W.EPH] = 200 * W.Gi
    return wl


def _alternating(seed, gpus):
    # test_z_hc_short_path's _cold_set_wins on a smaller pool: every queue's requests alternate between the largest and the smallest shape, the small ones go back to old
    # fragments.  gpus: a third of the nodes has 2 GPUs and a fifth of the jobs asks for one — GPU nodes run out of the second extra first
    wl = W.config3(seed=seed, n_nodes=300, n_jobs=3_000, n_queues=4)
    wl.global_burst, wl.queue_burst, wl.rate_inf = 1_500, 600, False
    big = np.array([32 * W.Gi, 8000, 200 * W.Gi, 0], dtype=np.int64)
    small = np.array([4 * W.Gi, 1000, 10 * W.Gi, 0], dtype=np.int64)
    for ids in wl.queued:
        wl.job_req[ids[0::2]] = big
        wl.job_req[ids[1::2]] = small
        if gpus:
            wl.job_req[ids[2::5], W.GPU] = 1
    if gpus:
        wl.node_total[:, W.GPU] = 0
        wl.node_total[::3, W.GPU] = 2
        running = wl.job_node >= 0
        wl.job_req[running, W.GPU] = 0
    return wl


def _fit_shapes(F):
    # exactly F distinct request rows = F fit shapes (one requirement class, every row fits an empty node, no running job adds a shape): cores 1 ... 8 x memory 1 ... 17 GiB
    palette = np.array([[m * W.Gi, c * 1000, 0, 0] for m in range(1, 18) for c in range(1, 9)], dtype=np.int64)[:F]
    assert len(np.unique(palette, axis=0)) == F
    wl = _pool(400, palette[np.arange(4_000) % F], 4)
    wl.global_burst, wl.queue_burst = 2_000, 800
    return wl


def _node_words(n):
    wl = W.config2(seed=816, n_nodes=n, n_jobs=1_200, n_queues=4)
    wl.global_burst, wl.queue_burst, wl.rate_inf = 1_200, 1_200, False
    return wl


# name -> (builder, pins of the CPU build).  Pins: l0_max, l0_overflows, stream_runs, stream_jobs ("all": every queued job; an int: exactly; ("min", n): at least n)
CASES = {}
for n in (47, 48, 49, 50, 56, 57, 58, 64, 65, 112):
    # 47 / 48: H never over its size, no hand-over; 49: the first; 56 / 57 / 58: eight, nine, ten hand-overs posted back to back, around the back-pressure bound (HC_INS / 2
    # in flight — whether wave 3 ever lags that far is timing); 64 / 65: as many live entries as lanes, and one more; 112: 65 hand-overs — the round-robin victim passes the
    # top occupied lane and wraps (H holds 48 entries and the few in flight: lane 63 itself is never occupied, the wrap is the `hiPart == 0` branch, after 49 hand-overs).
    # (profiling build on the MI355X: hand-overs 0, 0, 2, 3, 9, 10, 11, 17, 18, 65 — the one-core jobs that return to a fragment of C bring it back into H)
    CASES[f"h_size-{n}"] = (lambda n=n: _recipe(n), dict(l0_max=n, l0_overflows=0, stream_runs=1, stream_jobs="all"))
for n in (50, 57, 112):
    CASES[f"h_size_returns-{n}"] = (lambda n=n: _returns(n), dict(l0_max=n, l0_overflows=0, stream_runs=1, stream_jobs="all"))
for n in (1024, 1025, 1040, 1072, 1073):
    # the CPU build (serial engine): the 1025th live dirty node overflows the list, the stream run ends there and the generic code finishes the round
    CASES[f"overflow-{n}"] = (lambda n=n: _recipe(n, n_nodes=n + 50), dict(l0_max=1024, l0_overflows=int(n > 1024), stream_runs=1, stream_jobs="all" if n <= 1024 else 1025))
# 1200 with six one-core jobs behind the 100th BIG.  Measured on the MI355X with the plain recipe: from 1073 on wave 3's list is full while the BIGs are still being placed, the
# session ends before the first one-core job and the split engine has no short pick to show (hc_short_picks 0) although it ran.  The six go to the oldest fragment, which is
# C's by then: one question, then short picks from H — and the fragment stays alive, so the 1025th live dirty node is still the 1025th BIG (the CPU build binds 1031 in the run)
CASES["overflow-1200"] = (lambda: _pool(1250, [BIG] * 100 + [ONE] * 6 + [BIG] * 1100 + [ONE] * 300, 2), dict(l0_max=1024, l0_overflows=1, stream_runs=1, stream_jobs=1031))
CASES["extras-e0-h57"] = (lambda: _all_indexed(_recipe(57)), dict(stream_jobs=("min", 300)))
CASES["extras-e0-alternating"] = (lambda: _all_indexed(_alternating(814, gpus=False)), dict(stream_jobs=("min", 300)))
CASES["extras-e2-h57"] = (lambda: _two_extras(_recipe_gpus(57)), dict(stream_jobs=("min", 300)))
CASES["extras-e2-alternating"] = (lambda: _two_extras(_alternating(815, gpus=True)), dict(stream_jobs=("min", 300)))
for F in (64, 65, 128, 129):
    # 64 / 65: the second register set of HcShapes (lane + 64) empty or not; 128 / 129: the split engine on or off (HCB.clb[128], d.f.F <= 128)
    CASES[f"fit_shapes-{F}"] = (lambda F=F: _fit_shapes(F), dict(stream_jobs=2_000))
for n in (40, 63, 64, 65, 127, 129):
    # fitBits has (N + 63) / 64 words per shape: the clean side's scan ends at `wi >= fitW`, the spare is the next set bit of the SAME word
    CASES[f"node_words-{n}"] = (lambda n=n: _node_words(n), dict(stream_jobs=("min", 300)))
# a session that ends on a job fitting nowhere while H is full, and a second bulk-merged run behind it that reloads cursors and list from what the first folded back.
# "never": a job larger than any node (the ring entry says so: the session ends before any test).  "full": a 58th BIG on 57 nodes, each with a 12-core fragment — the
# general body finds neither a dirty nor a clean candidate.  60 one-core jobs in front use up five fragments: 52 are alive, 48 of them in H, when the session ends
CASES["ends_without_node-never"] = (lambda: _recipe(57, n_small=60, tail=[NEVER] + [ONE] * 240), dict(l0_max=57, l0_overflows=0, stream_runs=("min", 2), unscheduled=[57 + 60]))
CASES["ends_without_node-full"] = (lambda: _recipe(57, n_nodes=57, n_small=60, tail=[BIG] + [ONE] * 240), dict(l0_max=57, l0_overflows=0, stream_runs=("min", 2), unscheduled=[57 + 60]))
_ORACLE_ROUNDS = {}


def run(lib, wl, deadline=0.0):
    s = W.load(lib, wl)
    W.prepare(s, wl)
    if deadline:
        s.set_deadline(deadline)
    r = s.schedule_round()
    st = s.round_stats()
    s.close()
    return r, st


def case_and_oracle(name, oracle):
    """the workload and the oracle's round of it: computed once, shared, never changed"""
    if name not in _ORACLE_ROUNDS:
        wl = CASES[name][0]()
        _ORACLE_ROUNDS[name] = (wl, run(oracle, wl)[0])
    return _ORACLE_ROUNDS[name]


def _holds(pin, got, n_all):
    if pin == "all":
        return got == n_all
    if isinstance(pin, tuple):
        return got >= pin[1]
    return got == pin


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_reach_their_state(hostsim_lib, oracle_lib, name, monkeypatch):
    """CPU build (the serial engine on the same stream runs): the oracle's round, and the state the case is about — read from round_stats"""
    wl, want = case_and_oracle(name, oracle_lib)
    pins = CASES[name][1]
    monkeypatch.setenv("HS_MG_MIN", "64")
    r, st = run(hostsim_lib, wl)
    n_all = sum(len(q) for q in wl.queued)
    print(f"{name}: queued {n_all}, scheduled {len(want.scheduled)}, " + ", ".join(f"{k} {st[k]}" for k in ("l0_max", "l0_overflows", "stream_runs", "stream_jobs")))
    assert_same_round(r, want)
    for k in ("l0_max", "l0_overflows", "stream_runs", "stream_jobs"):
        if k in pins:
            assert _holds(pins[k], st[k], n_all), (k, pins[k], st[k])
    assert st["stream_runs"] > 0 and st["hc_short_picks"] == 0      # (the CPU build has no split engine)
    if "unscheduled" in pins:
        miss = pins["unscheduled"]
        assert all(j not in want.scheduled for j in miss)
        assert sorted(set(range(n_all)) - set(want.scheduled)) == miss      # ... and every job behind it is scheduled
    elif name.startswith(("h_size", "overflow")):
        assert len(want.scheduled) == n_all


ARMS = (("default", {}), ("short_off", {"ASCHED_HC_SHORT": "0"}), ("serial", {"ASCHED_ENGINE_HC": "0"}))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_engine_edges_equal_oracle_gpu(hip_lib, oracle_lib, name, monkeypatch):
    """product library: the three arms' rounds equal the oracle's; the split engine ran where it must (hc_short_picks) and only there.  overflow-1025 ... 1073: the default
    arm's counters are printed and only its round is asserted — the serial engine overflows at the 1025th live dirty node, the split engine when wave 3's list of COLD entries
    is full or when H does not fit behind it at the fold-back, so the two count different overflows and bind different numbers of jobs in the run (the module's text)"""
    wl, want = case_and_oracle(name, oracle_lib)
    pins = CASES[name][1]
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
    split_off = name == "fit_shapes-129"      # more than 128 fit shapes: the serial engine serves the round
    round_only = name.startswith("overflow-") and name not in ("overflow-1024", "overflow-1200")      # 1025 ... 1073: the default arm's round, nothing else
    if split_off:
        assert st["default"]["hc_short_picks"] == 0
    elif not round_only:
        assert st["default"]["hc_short_picks"] > 0
    assert st["short_off"]["hc_short_picks"] == 0 and st["serial"]["hc_short_picks"] == 0
    overflows = pins.get("l0_overflows", 0) > 0
    if overflows:
        n_all = sum(len(q) for q in wl.queued)
        assert st["serial"]["l0_overflows"] == pins["l0_overflows"] and st["serial"]["stream_runs"] == pins["stream_runs"] and _holds(pins["stream_jobs"], st["serial"]["stream_jobs"], n_all)
        if name == "overflow-1200":
            assert st["default"]["l0_overflows"] >= 1 and st["short_off"]["l0_overflows"] >= 1
    else:
        assert st["default"]["stream_runs"] == st["short_off"]["stream_runs"] == st["serial"]["stream_runs"] > 0
        assert st["default"]["stream_jobs"] == st["short_off"]["stream_jobs"] == st["serial"]["stream_jobs"]
        if "l0_overflows" in pins:
            assert st["serial"]["l0_overflows"] == 0
