"""The capacities of the stream runs and of their bulk merge (armada_amd/csrc/round_run.h fastStreamPrepare / fastStreamPrepareOne, round_merge.h, round_wide.h; DESIGN.md
3.1 "stream capacity"), at their edges:

    QS_CMAX = 32768     entries per queue and preparation; the merge passes' grids and arrays (MG_CPQ chunks, MG_SPQ samples per queue) are sized from it
    QS_GANG_CMAX = 4096 the same in a pool with gangs
    QS_ONE_MAX = 1024   fastStreamPrepareOne (ASCHED_PREP_ONE=1)
    MG_SAMPLE = 256     W_MG_CUT: every 256th key of a queue is a sample
    MG_CHUNK = 64       W_MG_PACK / W_MG_FIX: the running maximum within and across chunks
    WIDE_L = 1024       wide runs (more than 64 queues): a queue's cap is 32 in the first run and grows fourfold per run up to this

Every case is a whole round compared with the oracle's (scenario.assert_same_round) and runs three times: on the CPU build with a capacity of 64 (tests/hostsim
libhostsim_cap64.so: -DQS_CMAX=64 -DMG_SAMPLE=64 — C = 64, S = 64), on the default CPU build and, marked gpu, on the HIP library (C = 32768, S = 256).  The sizes of a case
are functions of C and S, so each build meets ITS capacity.  On the CPU builds round_stats pins that the case reached its state (stream_runs, stream_jobs,
stream_prepared); without that the GPU test would be vacuous.  The GPU test computes each round in three arms — the default, ASCHED_MERGE=0 (the control wave merges every
run) and ASCHED_STREAM=0 (no stream runs) — which tell "the bulk merge is wrong" from "the stream is wrong"; every GPU round has a deadline, so that a protocol defect ends
as ASCHED_ERR_TIMEOUT, not as a hang.  The bulk merge takes runs of 64 entries and more (HS_MG_MIN / ASCHED_MERGE_MIN).  The oracle's round of a case is computed once.

The two-queue pool (`_pool`): one long queue of L one-core jobs, one queue of 100, (jobs // 32) + 5 empty 32-core nodes, bursts that cover everything.

test_evicted_stream_over_capacity is the one case of a stream OVER the capacity that reaches the merge: an evicted stream is the rest of its queue's eviction list, which
nothing bounds.  mgWorth / mgPrepare turn it away (round_stats streams_over_cap, CPU build only) and the control wave merges the run; before that guard the passes were
given the 74 entries and the CPU build's bounds checks (round_merge.h MG_BOUND) abort in W_MG_PACK.  CPU only: no input is known that brings more than 32 768 evicted jobs
of one queue into a stream, and none is to be constructed for the device — the guard is the same source line there.
"""
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

from armada_amd import workloads as W
from armada_amd.binding import Library
from scenario import assert_same_round

GLOBAL_RATE_LIMIT = 3    # include/armada_sched.h ASCHED_REASON_GLOBAL_RATE_LIMIT
QUEUE_RATE_LIMIT = 4     # ASCHED_REASON_QUEUE_RATE_LIMIT
ONE = [4 * W.Gi, 1_000, 1 * W.Gi, 0]
BIG = [16 * W.Gi, 8_000, 4 * W.Gi, 0]
DEADLINE_S = 10.0
HERE = os.path.dirname(os.path.abspath(__file__))
BUILDS = {"cap64": (64, 64), "default": (32768, 256)}      # build -> (C, S)


@pytest.fixture(scope="module")
def cap64_lib():
    """the CPU build with a stream capacity of 64 (built under the same lock as conftest's hostsim_lib)"""
    here = os.path.join(HERE, "hostsim")
    with open(os.path.join(here, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", here, "libhostsim_cap64.so"])
    return Library(os.path.join(here, "libhostsim_cap64.so"), "asched_")


def _pool(lens, reqs=None, n_nodes=None, queue_burst=None, global_burst=None, lookback=0):
    """an empty pool of 32-core nodes; queue q holds lens[q] jobs (one core each unless `reqs` gives a row per job, queue after queue), in list order"""
    n = int(sum(lens))
    reqs = np.tile(np.array(ONE, dtype=np.int64), (n, 1)) if reqs is None else np.asarray(reqs, dtype=np.int64)
    assert len(reqs) == n
    if n_nodes is None:
        n_nodes = int(reqs[:, W.CPU].sum()) // 32_000 + 5
    wl = W.config1(n_nodes=n_nodes, n_jobs=n, seed=1)
    wl.node_total = np.tile(np.array((256 * W.Gi, 32_000, 1024 * W.Gi, 0), dtype=np.int64), (n_nodes, 1))
    wl.job_req = reqs
    q = np.repeat(np.arange(len(lens)), lens).astype(np.int32)
    wl.job_queue = q
    wl.queue_weight = np.ones(len(lens))
    wl.queued = [np.nonzero(q == i)[0].astype(np.int32) for i in range(len(lens))]
    wl.global_burst, wl.queue_burst, wl.rate_inf = global_burst or n, queue_burst or n, False
    wl.config.max_queue_lookback = lookback
    return wl


def _gang(wl, members, gid):
    members = np.asarray(members)
    wl.job_gang[members] = gid
    wl.job_gang_card[members] = len(members)
    return wl


class Case:
    def __init__(self, wl, env=(), pins=None, check=None):
        self.wl, self.env, self.pins, self.check = wl, dict(env), pins or {}, check


def _alternating(L, prefer_large, mixed):
    # two queues of L jobs of two priority classes, requests alternating between one and eight cores.  Sorted (SchedulingOrderCompare: the higher class first) a queued
    # stream's keys never decrease: the class falls once, the costs grow with the allocation.  mixed: of every eight jobs of the LIST the first three are of the higher class (the order the
    # queue's iterator yields is the list's, whatever the keys: queue_scheduler.go:701-798 serves a queue's jobs in that order) — from the ninth job on each of them orders
    # before the running maximum in front of it, within a chunk (W_MG_PACK) and, jobs 64 ... 66 and 128, as the first ones of a chunk (W_MG_FIX)
    # A third queue of 64 one-core jobs of the lower class: the bulk merge takes a run when one stream has 64 entries, also where L is 63.
    reqs = [ONE if i % 2 == 0 else BIG for i in range(L)] * 2 + [ONE] * 64
    wl = _pool([L, L, 64], reqs=reqs)
    wl.config.pc_priority, wl.config.pc_preemptible = [0, 1], [1, 1]
    pc = np.zeros(2 * L + 64, dtype=np.int32)
    for ids in wl.queued[:2]:
        if mixed:
            pc[ids] = np.arange(L) % 8 < 3
        else:
            pc[ids[:L // 2]] = 1
    wl.job_pc = pc
    wl.config.prefer_large_job_ordering = prefer_large
    return wl


def cases(C, S):
    """name -> Case, for a build with stream capacity C and cut sample S"""
    out = {}
    # a. stream length at the capacity
    for tag, L in (("C-1", C - 1), ("C", C), ("C+1", C + 1), ("2C", 2 * C), ("2C+1", 2 * C + 1)):
        out[f"a-length-{tag}"] = Case(_pool([L, 100]))
    # b. room for the limit element (fastStreamPrepare and mgPrepare: len < QS_CMAX): C + 10 jobs, C - 2 ... C + 1 tokens per queue; with and without the element carried
    for tag, t in (("C-2", C - 2), ("C-1", C - 1), ("C", C), ("C+1", C + 1)):
        for carried in (True, False):
            def check(wl, want, t=t):
                hit = np.nonzero(np.asarray(want.job_unschedulable_reason)[wl.queued[0]] == QUEUE_RATE_LIMIT)[0].tolist()
                assert hit == [t], hit
            out[f"b-limit-tokens-{tag}" + ("" if carried else "-not-carried")] = Case(
                _pool([C + 10, 100], queue_burst=t), env={} if carried else {"HS_NO_STREAM_LIMIT": "1", "ASCHED_STREAM_LIMIT": "0"}, check=check)
    # c. the lookback limit at the capacity
    for tag, lb in (("C-1", C - 1), ("C", C), ("C+1", C + 1)):
        out[f"c-lookback-{tag}"] = Case(_pool([2 * C, 100], lookback=lb))
    # d. the cut (W_MG_CUT): queue lengths next to multiples of the sample distance (k S - 1, k S, k S + 1: the sample count is a sum over queues) and next to the capacity
    # (C / S samples); the global burst on either side of the cut's switch-on condition needAll + 2 S < total (needAll = the global tokens here).  A stream is also cut at
    # the global tokens, so the condition can only hold where the tokens cover the longest stream: three queues where k >= 2, five (two more of k S) at k = 1
    for ltag, n in (("S", S), ("2S", 2 * S), ("C", C)):
        lens = (n - 1, n, n + 1) if min(n, C) >= 2 * S else (n - 1, n, n + 1, n, n)
        total = sum(min(x, C) for x in lens)      # what the first run's merge is given
        for d in (-1, 0, 1):
            burst = total - 2 * S - 1 - d
            assert burst >= min(max(lens), C)
            def check(wl, want):
                assert (np.asarray(want.job_unschedulable_reason) == GLOBAL_RATE_LIMIT).any()
            out[f"d-cut-{ltag}-burst{-d:+d}"] = Case(_pool(lens, global_burst=burst), check=check, pins={"cut": int(d >= 0)})
    # e. chunk boundaries of the key passes
    for L in (63, 64, 65, 127, 128, 129):
        for pl in (True, False):
            for mixed in (False, True):
                out[f"e-chunks-{L}-" + ("prefer-large" if pl else "plain") + ("-mixed-classes" if mixed else "")] = Case(_alternating(L, pl, mixed), pins={"decreases": mixed})
    # f. a pool with gangs (G > 0): QS_GANG_CMAX = 4096 is the capacity where it is below C
    for n in (4095, 4096, 4097):
        wl = _pool([n, 100])
        out[f"f-gangs-{n}"] = Case(_gang(wl, wl.queued[1][40:42], 0))
    # g. fastStreamPrepareOne (QS_ONE_MAX = 1024): [gang of 2][n singles][gang of 2][100 singles]
    for n in (1023, 1024, 1025, 1026):      # (1026: where the CPU build's run count steps)
        wl = _pool([n + 104, 100])
        ids = wl.queued[0]
        _gang(wl, ids[0:2], 0)
        _gang(wl, ids[n + 2:n + 4], 1)
        out[f"g-prepare-one-{n}"] = Case(wl, env={"ASCHED_PREP_ONE": "1"})
    # i. wide runs: 65 queues, one long one and 64 of three jobs; a queue's cap is 32, 128, 512, then WIDE_L = 1024 per run
    for L in WIDE_LENGTHS:
        out[f"i-wide-{L}"] = Case(_pool([L] + [3] * 64))
    # ... and the long queue's jobs running, on a pool they fill: all of them are evicted (the queue is far over its share of 1 / 65) and return as an evicted stream,
    # cut at the cap of the queue's first run where there are more (W_SEG flag 4).  (The later, larger caps are not reached this way: DESIGN.md 3.1)
    for L in (31, 32, 33, 161):
        out[f"i-wide-evicted-{L}"] = Case(_wide_evicted(L), pins={"evicted_cut": L > 32})
    return out


def _wide_evicted(L):
    wl = _pool([L] + [3] * 64, n_nodes=(L + 31) // 32)
    ids = wl.queued[0]
    wl.job_node[ids] = (np.arange(L) // 32).astype(np.int32)
    wl.job_run_ts[ids] = np.arange(L)
    wl.queued[0] = np.zeros(0, np.int32)
    return wl


# the lengths at which the CPU build's stream_runs steps (cumulative caps 32, 160, 672, 1696, 2720), each with its neighbours, and 128 / 512 / 1024 / 2049
WIDE_LENGTHS = (31, 32, 33, 128, 129, 159, 160, 161, 512, 513, 671, 672, 673, 1023, 1024, 1025, 1695, 1696, 1697, 2049)

NAMES = list(cases(64, 64))
# (stream_runs, stream_jobs, stream_prepared) of the CPU build with capacity 64 and of the default CPU build.  The default build's a-length and b-limit rows are the table of
# the issue this file answers (runs 1, 1, 2, 2, 3; the limit element at position `tokens`); the rest is what the builds counted when the cases were written: they pin
# that a case still reaches the state it names, the rounds themselves are compared with the oracle's
PINS = {
    "a-length-C-1": ((2, 163, 163), (1, 32867, 32867)),
    "a-length-C": ((2, 164, 164), (1, 32868, 32868)),
    "a-length-C+1": ((3, 157, 158), (2, 32869, 32869)),
    "a-length-2C": ((3, 220, 284), (2, 65636, 65636)),
    "a-length-2C+1": ((3, 221, 285), (3, 65637, 65637)),
    "b-limit-tokens-C-2": ((2, 124, 124), (1, 32866, 32866)),
    "b-limit-tokens-C-2-not-carried": ((2, 124, 124), (1, 32866, 32866)),
    "b-limit-tokens-C-1": ((2, 126, 126), (1, 32867, 32867)),
    "b-limit-tokens-C-1-not-carried": ((2, 126, 126), (1, 32867, 32867)),
    "b-limit-tokens-C": ((2, 128, 128), (1, 32868, 32868)),
    "b-limit-tokens-C-not-carried": ((2, 128, 128), (1, 32868, 32868)),
    "b-limit-tokens-C+1": ((2, 128, 129), (2, 32869, 32869)),
    "b-limit-tokens-C+1-not-carried": ((2, 128, 129), (2, 32869, 32869)),
    "c-lookback-C-1": ((2, 126, 126), (1, 32867, 32867)),
    "c-lookback-C": ((2, 128, 128), (1, 32868, 32868)),
    "c-lookback-C+1": ((2, 128, 129), (2, 32869, 32869)),
    "d-cut-S-burst+1": ((2, 191, 319), (2, 768, 1280)),
    "d-cut-S-burst+0": ((2, 190, 319), (2, 767, 1280)),
    "d-cut-S-burst-1": ((2, 189, 319), (2, 766, 1280)),
    "d-cut-2S-burst+1": ((2, 192, 320), (2, 1024, 1536)),
    "d-cut-2S-burst+0": ((2, 191, 320), (2, 1023, 1536)),
    "d-cut-2S-burst-1": ((2, 190, 320), (2, 1022, 1536)),
    "d-cut-C-burst+1": ((2, 191, 319), (2, 97791, 98303)),
    "d-cut-C-burst+0": ((2, 190, 319), (2, 97790, 98303)),
    "d-cut-C-burst-1": ((2, 189, 319), (2, 97789, 98303)),
    "e-chunks-63-prefer-large": ((1, 190, 190), (1, 190, 190)),
    "e-chunks-63-prefer-large-mixed-classes": ((1, 190, 190), (1, 190, 190)),
    "e-chunks-63-plain": ((1, 190, 190), (1, 190, 190)),
    "e-chunks-63-plain-mixed-classes": ((1, 190, 190), (1, 190, 190)),
    "e-chunks-64-prefer-large": ((1, 192, 192), (1, 192, 192)),
    "e-chunks-64-prefer-large-mixed-classes": ((1, 192, 192), (1, 192, 192)),
    "e-chunks-64-plain": ((1, 192, 192), (1, 192, 192)),
    "e-chunks-64-plain-mixed-classes": ((1, 192, 192), (1, 192, 192)),
    "e-chunks-65-prefer-large": ((2, 192, 193), (1, 194, 194)),
    "e-chunks-65-prefer-large-mixed-classes": ((2, 193, 193), (1, 194, 194)),
    "e-chunks-65-plain": ((2, 192, 193), (1, 194, 194)),
    "e-chunks-65-plain-mixed-classes": ((2, 193, 193), (1, 194, 194)),
    "e-chunks-127-prefer-large": ((3, 310, 373), (1, 318, 318)),
    "e-chunks-127-prefer-large-mixed-classes": ((3, 310, 370), (1, 318, 318)),
    "e-chunks-127-plain": ((3, 310, 373), (1, 318, 318)),
    "e-chunks-127-plain-mixed-classes": ((3, 310, 370), (1, 318, 318)),
    "e-chunks-128-prefer-large": ((3, 312, 376), (1, 320, 320)),
    "e-chunks-128-prefer-large-mixed-classes": ((3, 312, 373), (1, 320, 320)),
    "e-chunks-128-plain": ((3, 312, 376), (1, 320, 320)),
    "e-chunks-128-plain-mixed-classes": ((3, 312, 373), (1, 320, 320)),
    "e-chunks-129-prefer-large": ((4, 312, 377), (1, 322, 322)),
    "e-chunks-129-prefer-large-mixed-classes": ((3, 314, 375), (1, 322, 322)),
    "e-chunks-129-plain": ((4, 312, 377), (1, 322, 322)),
    "e-chunks-129-plain-mixed-classes": ((3, 314, 375), (1, 322, 322)),
    "f-gangs-4095": ((64, 4193, 4193), (1, 4193, 4193)),
    "f-gangs-4096": ((64, 4194, 4194), (1, 4194, 4194)),
    "f-gangs-4097": ((65, 4195, 4195), (2, 4195, 4195)),
    "g-prepare-one-1023": ((20, 1219, 1283), (2, 1219, 2242)),
    "g-prepare-one-1024": ((20, 1220, 1284), (2, 1220, 2244)),
    "g-prepare-one-1025": ((20, 1221, 1285), (2, 1221, 2245)),
    "g-prepare-one-1026": ((21, 1222, 1286), (3, 1222, 2246)),
    "i-wide-31": ((1, 223, 223), (1, 223, 223)),
    "i-wide-32": ((1, 224, 224), (1, 224, 224)),
    "i-wide-33": ((2, 225, 225), (2, 225, 225)),
    "i-wide-128": ((2, 320, 320), (2, 320, 320)),
    "i-wide-129": ((2, 321, 321), (2, 321, 321)),
    "i-wide-159": ((2, 351, 351), (2, 351, 351)),
    "i-wide-160": ((2, 352, 352), (2, 352, 352)),
    "i-wide-161": ((3, 353, 353), (3, 353, 353)),
    "i-wide-512": ((3, 704, 704), (3, 704, 704)),
    "i-wide-513": ((3, 705, 705), (3, 705, 705)),
    "i-wide-671": ((3, 863, 863), (3, 863, 863)),
    "i-wide-672": ((3, 864, 864), (3, 864, 864)),
    "i-wide-673": ((4, 865, 865), (4, 865, 865)),
    "i-wide-1023": ((4, 1215, 1215), (4, 1215, 1215)),
    "i-wide-1024": ((4, 1216, 1216), (4, 1216, 1216)),
    "i-wide-1025": ((4, 1217, 1217), (4, 1217, 1217)),
    "i-wide-1695": ((4, 1887, 1887), (4, 1887, 1887)),
    "i-wide-1696": ((4, 1888, 1888), (4, 1888, 1888)),
    "i-wide-1697": ((5, 1889, 1889), (5, 1889, 1889)),
    "i-wide-2049": ((5, 2241, 2241), (5, 2241, 2241)),
    "i-wide-evicted-31": ((1, 2, 223), (1, 2, 223)),
    "i-wide-evicted-32": ((1, 1, 224), (1, 1, 224)),
    "i-wide-evicted-33": ((1, 32, 224), (1, 32, 224)),
    "i-wide-evicted-161": ((1, 32, 224), (1, 32, 224)),
}
_CASES, _ORACLE_ROUNDS = {}, {}


def case_and_oracle(build, name, oracle):
    """the case at the build's capacity and the oracle's round of it: computed once, shared, never changed"""
    C, S = BUILDS[build]
    if C not in _CASES:
        _CASES[C] = cases(C, S)
    c = _CASES[C][name]
    if (C, name) not in _ORACLE_ROUNDS:
        _ORACLE_ROUNDS[C, name] = run(oracle, c.wl)[0]
    return c, _ORACLE_ROUNDS[C, name]


def run(lib, wl, deadline=0.0):
    s = W.load(lib, wl)
    W.prepare(s, wl)
    if deadline:
        s.set_deadline(deadline)
    r = s.schedule_round()
    st = s.round_stats()
    s.close()
    return r, st


ENV_VARS = ("HS_NO_STREAM_LIMIT", "ASCHED_STREAM_LIMIT", "ASCHED_PREP_ONE", "ASCHED_MERGE", "ASCHED_STREAM")
STATS = ("stream_runs", "stream_jobs", "stream_prepared", "streams_over_cap")


def _set_env(monkeypatch, env):
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, x in env.items():
        monkeypatch.setenv(v, x)


def _cpu(build, lib, oracle, name, monkeypatch, capfd):
    """a CPU build: the oracle's round; the counters that show the state the case is about (PINS: what this build counted when the case was written — the issue's table
    for the lengths and the limit element at the real capacity); for the cut and the chunk cases the build's own trace of its bulk merges"""
    c, want = case_and_oracle(build, name, oracle)
    monkeypatch.setenv("HS_MG_MIN", "64")
    monkeypatch.setenv("HS_MG_TRACE", "1")
    monkeypatch.setenv("HS_WIDE_TRACE", "1")
    _set_env(monkeypatch, c.env)
    capfd.readouterr()
    r, st = run(lib, c.wl)
    trace = capfd.readouterr().err
    print(f"{build} {name}: queued {sum(len(q) for q in c.wl.queued)}, scheduled {len(want.scheduled)}, " + ", ".join(f"{k} {st[k]}" for k in STATS))
    assert_same_round(r, want)
    if c.check:
        c.check(c.wl, want)
    assert st["streams_over_cap"] == 0 and st["stream_runs"] > 0
    assert (st["stream_runs"], st["stream_jobs"], st["stream_prepared"]) == PINS[name][build == "default"]
    merges = re.findall(r"bulk merge: (\d+) entries of (\d+) queues, valid (\d+), skip \d+, cut (\d) .*?decreases (\d+) \((\d+) across", trace)
    if "cut" in c.pins:        # the first run's merge: the cut is on and finds its key on one side of the condition, off on the other
        assert merges and int(merges[0][3]) == c.pins["cut"], trace[:400]
    if "decreases" in c.pins:
        L = len(c.wl.queued[0])
        assert merges and (sum(int(m[4]) for m in merges) > 0) == c.pins["decreases"]
        assert sum(int(m[5]) for m in merges) == (2 * ((min(L, BUILDS[build][0]) - 1) // 64) if c.pins["decreases"] else 0)      # per queue: the first entry of every chunk but the first
    if "evicted_cut" in c.pins:
        assert ("open q0 evCnt 32" in trace) == c.pins["evicted_cut"], trace[:400]


@pytest.mark.parametrize("name", NAMES)
def test_capacity_edges_cap64(cap64_lib, oracle_lib, name, monkeypatch, capfd):
    _cpu("cap64", cap64_lib, oracle_lib, name, monkeypatch, capfd)


@pytest.mark.parametrize("name", NAMES)
def test_capacity_edges_default_build(hostsim_lib, oracle_lib, name, monkeypatch, capfd):
    _cpu("default", hostsim_lib, oracle_lib, name, monkeypatch, capfd)


def test_evicted_stream_over_capacity(cap64_lib, oracle_lib, monkeypatch, capfd):
    """tests/soak.py rounds, seed 100137, on the build with capacity 64: queue 3's evicted stream has 74 entries when a run long enough for the bulk merge starts.  The
    guard turns it away (streams_over_cap), the control wave merges the run, the round is the oracle's, and no bounds check of the passes fires (it would abort the process:
    without the guard W_MG_PACK does, "queue 3: 74 entries, the pass packs 1 chunks of 64")"""
    wl = W.small_random(n_nodes=128, n_jobs=222, n_queues=5, seed=100137, occupied=1.0, gangs=6, burst=(1729, 453), away=True, ragged=False)
    monkeypatch.setenv("HS_MG_MIN", "64")
    _set_env(monkeypatch, {})
    want, _ = run(oracle_lib, wl)
    r, st = run(cap64_lib, wl)
    print("seed 100137: " + ", ".join(f"{k} {st[k]}" for k in STATS))
    assert_same_round(r, want)
    assert st["streams_over_cap"] >= 1 and st["stream_runs"] > 0
    assert "out of bounds" not in capfd.readouterr().err


ARMS = (("default", {}), ("merge_off", {"ASCHED_MERGE": "0"}), ("stream_off", {"ASCHED_STREAM": "0"}))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_capacity_edges_gpu(hip_lib, oracle_lib, name, monkeypatch):
    """product library, the real constants: the three arms' rounds equal the oracle's; the default arm and the arm without the bulk merge make stream runs, the third none"""
    c, want = case_and_oracle("default", name, oracle_lib)
    monkeypatch.setenv("ASCHED_MERGE_MIN", "64")
    st = {}
    for arm, env in ARMS:
        _set_env(monkeypatch, {**c.env, **env})
        r, st[arm] = run(hip_lib, c.wl, deadline=DEADLINE_S)
        print(f"{name} [{arm}]: " + ", ".join(f"{k} {st[arm][k]}" for k in STATS))
        assert_same_round(r, want)
    if c.check:
        c.check(c.wl, want)
    assert st["default"]["stream_runs"] > 0 and st["merge_off"]["stream_runs"] > 0 and st["stream_off"]["stream_runs"] == 0
    if name.startswith(("a-", "b-", "c-", "f-")):      # how many runs a list takes is the capacity itself (these runs end where a stream ends, not where the engine is): the CPU build's count
        assert st["default"]["stream_runs"] == st["merge_off"]["stream_runs"] == PINS[name][1][0]
