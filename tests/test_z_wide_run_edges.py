"""Wide runs (armada_amd/csrc/round_wide.h; more than 64 queues) at their edges: the rank pass, the chunked key passes and the rules where a run must stop.

    W_PER = 16      queues one item of the rank pass (W_RANK) walks: the last slice of Q queues holds Q % 16 of them
    W_RG = 8        binary searches of a slice that run side by side; the own queue is skipped, equal keys are ordered by the queue's NAME RANK
    WQ_CHUNK = 8    entries one item of W_QSUM / W_PACK covers; W_STITCH and W_FIX carry sums and the running maximum across the chunks
    32              a queue's cap in its first run (P.cap); the control wave stages the merged order in batches of 64

tests/test_z_wide_runs.py and `tests/soak.py wide` run seeded workloads whose queue name rank is the queue index and whose queues all get the same tokens; the i-wide rows
of tests/test_z_stream_capacity.py pin the cap on one long queue.  Here every case is a whole round on a HAND-BUILT pool, compared bit for bit with the oracle's round
(scenario.assert_same_round), which is computed once per case.  Every case runs on the CPU build and, marked gpu, on the HIP library, where the same source runs with another
item-to-thread mapping, the compact arrays in whatever order the fetch-add served and the integer atomics in any order.  The GPU test computes each round twice, by default
and with ASCHED_WIDE=0: the second arm tells "the wide run is wrong" from "the generic path at more than 64 queues is wrong".  Every GPU round has a deadline, so that a
protocol defect ends as ASCHED_ERR_TIMEOUT, not as a hang.  This file has a `prepare` of its own: W.prepare passes neither a name rank nor per-queue tokens.

A round result holds job -> node, not the order in which the jobs were served.  Two devices make the merged ORDER observable (families A and B use one or both):
  * a global burst smaller than the number of jobs: the scheduled set is the first `burst` new jobs of the merged order;
  * nodes that hold four of the case's one-core jobs: a job's node follows its merged position.

Every case asserts its own coverage condition — from the oracle's result, from the inputs, and on the CPU build from round_stats (PINS) and the build's own trace of its
wide runs; without one the GPU test would be vacuous.  The families:

  A  the rank pass: queue counts around the slices of 16 and the groups of 8 with all queues identical (every key ties: the order IS the name rank; identity, reversed and a
     seeded permutation); ties inside a group only; no ties; searches over 0, 1 and 2 entries next to long ones; a barrier entry (a gang at a queue's head) that ties.
  B  the chunked key passes: queued-part lengths around multiples of 8; a gang and a known-unfeasible key as the barrier at the chunk edges, with the exemption of the peeked
     head and without it (an evicted part in front); an evicted part of 1 ... 13 entries in front of a queued part (the stream's chunk grid and the queued part's are
     misaligned); the evicted part cut at the cap; keys that fall along a queue at the first entry of a chunk (W_FIX) and inside one (W_PACK).
  C  where a run must stop: per-queue tokens, the global tokens on both sides of the first batch of 64 staged entries (with and without returning evicted jobs, which take
     no token), the lookback limit, a pool too small for the run.
  D  a wide round, a round of 12 queues and a wide round again on one handle, with B's evicted-then-queued pool.
  E  one round of 70 queues under a forced two-word key layout (k_control_wk at more than 64 queues): the round is the oracle's and no stream run is made there.

profiles/r28_wide_run_edges.txt has the table of the one-line variants of round_wide.h that these cases were checked against (CPU build, nothing of it committed).
"""
import numpy as np
import pytest

import test_z_stream_capacity as SC
from armada_amd import workloads as W
from scenario import assert_same_round

GLOBAL_RATE_LIMIT, QUEUE_RATE_LIMIT, JOB_DOES_NOT_FIT, SKIPPED_UNFEASIBLE_KEY = 3, 4, 11, 17      # include/armada_sched.h ASCHED_REASON_*
ONE, BIG = SC.ONE, SC.BIG
HALF = [2 * W.Gi, 500, W.Gi // 2, 0]        # two of them cost what ONE costs
HUGE = [4 * W.Gi, 64_000, 1 * W.Gi, 0]      # fits no node of any pool here
DEADLINE_S = 10.0
QUEUE_COUNTS = (65, 72, 73, 79, 80, 81, 96, 97, 130, 257)      # the last slice of 16: 1 queue, one group of 8, 8 + 1, 15, a full 16, 81 opens a sixth slice ...
POSITIONS = (0, 1, 7, 8, 9, 15, 16, 17)                        # of a barrier in the queued part: around the edges of two chunks of 8


class Case:
    """a pool, the name rank and the tokens of its queues; check(case, want, others): the coverage condition on the oracle's round (`others`: name -> oracle round of
    another case); cpu(case, stats, trace): the one on the CPU build's counters and trace"""
    def __init__(self, wl, name_rank=None, tokens=None, check=None, cpu=None, env=(), needs=()):
        self.wl, self.name_rank, self.tokens, self.check, self.cpu, self.env, self.needs = wl, name_rank, tokens, check, cpu, dict(env), tuple(needs)


def prepare(s, wl, name_rank=None, tokens=None):
    """round_prepare with the workload's queues, a name rank per queue and the tokens each queue's limiter holds (None: every limiter full, as W.prepare)"""
    q = wl.num_queues
    s.round_prepare(wl.queue_weight, wl.queued, name_rank=None if name_rank is None else np.asarray(name_rank, np.int32),
                    global_tokens=float(wl.global_burst), global_burst=wl.global_burst, global_rate_inf=wl.rate_inf,
                    queue_tokens=[float(wl.queue_burst)] * q if tokens is None else [float(t) for t in tokens], queue_burst=[wl.queue_burst] * q, queue_rate_inf=[wl.rate_inf] * q)


def run(lib, c, deadline=0.0):
    s = W.load(lib, c.wl)
    prepare(s, c.wl, c.name_rank, c.tokens)
    if deadline:
        s.set_deadline(deadline)
    r = s.schedule_round()
    st = s.round_stats()
    s.close()
    return r, st


def _four_core_nodes(wl, n_jobs):
    """nodes that hold four one-core jobs, enough of them for n_jobs"""
    wl.node_total = np.tile(np.array((16 * W.Gi, 4_000, 4 * W.Gi, 0), dtype=np.int64), (n_jobs // 4 + 5, 1))
    return wl


def _new_scheduled(wl, r):
    """the jobs of the round's result that were queued"""
    return sorted(j for j in r.scheduled if wl.job_node[j] < 0)


def _positions(wl):
    """job -> (queue, position in the queue's list)"""
    return {int(j): (q, e) for q, ids in enumerate(wl.queued) for e, j in enumerate(ids)}


def _all_return(wl, want):
    """every running job is evicted in phase 1 and is back on its node when the round ends (a rescheduled job is neither in the result's scheduled nor in its preempted
    jobs).  -> their number"""
    running = np.nonzero(wl.job_node >= 0)[0]
    assert want.num_evicted_phase1 == len(running) > 0 and not any(int(j) in want.preempted or int(j) in want.scheduled for j in running)
    return len(running)


def _reasons(want, ids):
    return np.asarray(want.job_unschedulable_reason)[np.asarray(ids, dtype=np.int64)]


def _ranks(Q):
    return {"identity": np.arange(Q), "reversed": np.arange(Q)[::-1].copy(), "permuted": np.random.default_rng(Q).permutation(Q)}


def _distinct_weights(Q):
    return 1.0 + np.sqrt(np.arange(Q) + 1.0) / 37.0      # no two queues' costs tie (k / w_a = m / w_b has no solution in small integers)


# ---------------------------------------------------------------------------------------------------------------- A. the rank pass
def _identical(Q, rank):
    wl = _four_core_nodes(SC._pool([40] * Q, global_burst=Q * 40 // 3 + 5), Q * 40 // 3 + 5)

    def check(c, want, others):
        burst, pos = c.wl.global_burst, _positions(c.wl)
        full, rest = burst // Q, burst % Q
        assert 0 < rest < Q
        expect = sorted(j for j, (q, e) in pos.items() if e < full or (e == full and c.name_rank[q] < rest))
        assert _new_scheduled(c.wl, want) == expect
        if "identity" in others:      # the tie-break is observable: under the identity another set of queues serves position `full`
            assert set(want.scheduled) != set(others["identity"].scheduled)
    return Case(wl, name_rank=rank, check=check)


def _pairs(Q, swapped):
    """pairs of neighbouring queues identical, the pairs differ by weight; swapped: within a pair the higher queue index has the lower name rank"""
    wl = _four_core_nodes(SC._pool([40] * Q, global_burst=Q * 40 // 3 + 5), Q * 40 // 3 + 5)
    wl.queue_weight = 1.0 + (np.arange(Q) // 2) / 1000.0
    rank = np.arange(Q)
    if swapped:
        rank = rank ^ 1
        if Q % 2:
            rank[Q - 1] = Q - 1

    def check(c, want, others):
        assert len(_new_scheduled(c.wl, want)) == c.wl.global_burst
        if "identity" in others:
            assert want.scheduled != others["identity"].scheduled      # job -> node: the order within the pairs is observable
    return Case(wl, name_rank=rank, check=check)


def _no_ties(Q, reversed_rank):
    wl = _four_core_nodes(SC._pool([40] * Q, global_burst=Q * 40 // 3 + 5), Q * 40 // 3 + 5)
    wl.queue_weight = _distinct_weights(Q)

    def check(c, want, others):
        assert len(_new_scheduled(c.wl, want)) == c.wl.global_burst
        if "identity" in others:
            assert want.scheduled == others["identity"].scheduled      # no comparison ends in the name rank
    return Case(wl, name_rank=np.arange(Q)[::-1].copy() if reversed_rank else np.arange(Q), check=check)


def _ranges(lens, rank):
    n = int(sum(lens))
    wl = _four_core_nodes(SC._pool(lens, global_burst=2 * n // 3), n)

    def check(c, want, others):
        assert len(_new_scheduled(c.wl, want)) == c.wl.global_burst and (np.asarray(want.job_unschedulable_reason) == GLOBAL_RATE_LIMIT).any()
    return Case(wl, name_rank=rank, check=check)


def _barrier_tie(gang_rank):
    """64 identical queues of 10 one-core jobs and queue 30, which holds nothing but a gang of two half-core jobs: the gang costs what a single job costs, so the barrier
    entry (the gang queue's current key) ties with the first entry of every other queue, and its place among them is the gang queue's name rank — the only thing the
    rank of queue 60 decides.  Rank 0: the gang is the first thing the round serves, and no wide run starts on a gang; rank 4: four entries, one node's worth, order before the barrier
    (a tie-break by queue index would let 60 pass); rank 64: all 64 first entries do"""
    Q, g = 65, 60
    lens = [10] * Q
    lens[g] = 2
    reqs = np.tile(np.array(ONE, dtype=np.int64), (sum(lens), 1))
    wl = SC._pool(lens, reqs=reqs, global_burst=Q * 10 // 3 + 5)
    head = wl.queued[g][:2]
    wl.job_req[head] = HALF
    SC._gang(wl, head, 0)
    _four_core_nodes(wl, Q * 10)
    rank = np.zeros(Q, dtype=np.int64)      # the other queues keep their order among themselves
    rank[[q for q in range(Q) if q != g]] = [r for r in range(Q) if r != gang_rank]
    rank[g] = gang_rank

    def check(c, want, others):
        assert all(int(j) in want.scheduled for j in head)
        if "lowest" in others:
            assert want.scheduled != others["lowest"].scheduled      # the keys tie: the gang queue's name rank decides where the gang is served
    return Case(wl, name_rank=rank, check=check)


# ---------------------------------------------------------------------------------------------------------------- B. the chunked key passes
def _alternating_reqs(lens):
    return [ONE if e % 2 == 0 else BIG for L in lens for e in range(L)]


def _queued_lengths():
    lens = [(7, 8, 9, 15, 16, 17, 31, 32, 33)[q % 9] for q in range(72)]
    n = sum(lens)
    wl = SC._pool(lens, reqs=_alternating_reqs(lens), global_burst=2 * n // 3)
    wl.queue_weight = _distinct_weights(72)

    def check(c, want, others):
        assert len(_new_scheduled(c.wl, want)) == c.wl.global_burst
    return Case(wl, name_rank=np.arange(72)[::-1].copy(), check=check)


def _gang_barrier(p):
    """70 queues of 40 one-core jobs; in every third queue elements p and p + 1 of the list are a gang of two"""
    Q = 70
    wl = _four_core_nodes(SC._pool([40] * Q), Q * 40)
    gangs = 0
    for q in range(0, Q, 3):
        SC._gang(wl, wl.queued[q][p:p + 2], gangs)
        gangs += 1

    def check(c, want, others):
        assert len(want.scheduled) == c.wl.num_jobs

    def cpu(c, st, trace):
        assert st["generic_iterations"] >= gangs, st["generic_iterations"]
    return Case(wl, name_rank=np.random.default_rng(p).permutation(Q), check=check, cpu=cpu)


def _packed_runs(wl, queues, counts, n_nodes_before=0):
    """the first counts[i] jobs of queue queues[i] run, packed on 32-core nodes in queue order; they leave the queued list.  -> the number of nodes used"""
    node, used = n_nodes_before, 0
    ts = 0
    for q, k in zip(queues, counts):
        ids = wl.queued[q][:k]
        for j in ids:
            cpu = int(wl.job_req[j, W.CPU])
            if used + cpu > 32_000:
                node, used = node + 1, 0
            wl.job_node[j], wl.job_run_ts[j] = node, ts
            used += cpu
            ts += 1
        wl.queued[q] = wl.queued[q][k:]
    return node + 1


def _unfeasible_barrier(p, evicted_front):
    """70 queues of 24 one-core jobs.  The head of queue 0 (a weight of 1000: the first job of the round) asks for 64 cores and fits no node: its scheduling key is known to be
    unfeasible from then on.  Every third queue from queue 3 on has a job of that shape at element p of its queued part.  Element 0 is exempt where it is the peeked head (it
    was peeked before the key was known: it fails like queue 0's head); evicted_front: three running jobs of these queues return first, so that element 0 is peeked later
    and skipped like every other one"""
    Q, L = 70, 24
    lens = [L + 3 if (evicted_front and q % 3 == 0 and q) else L for q in range(Q)]
    wl = SC._pool(lens, n_nodes=Q * L // 32 + 12)
    marked = list(range(3, Q, 3))
    if evicted_front:
        _packed_runs(wl, marked, [3] * len(marked))
    wl.job_req[wl.queued[0][0]] = HUGE
    wl.queue_weight[0] = 1000.0      # (its cost: the 64 cores order before every other queue's one core)
    barrier = [int(wl.queued[q][p]) for q in marked]
    wl.job_req[barrier] = HUGE
    running = int((wl.job_node >= 0).sum())

    def check(c, want, others):
        got = _reasons(want, barrier)
        if p == 0 and not evicted_front:
            assert (got == _reasons(want, [c.wl.queued[0][0]])[0]).all() and (got != SKIPPED_UNFEASIBLE_KEY).all(), got      # the peeked heads: the exemption
        else:
            assert (got == SKIPPED_UNFEASIBLE_KEY).all(), got
        assert running == 0 or _all_return(c.wl, want) == running
        assert len(_new_scheduled(c.wl, want)) == c.wl.num_jobs - running - len(barrier) - 1
    return Case(wl, check=check)


def _evicted_then_queued(prefer_large, Q=70):
    """evCnt in 1 ... 13 running jobs per queue, all evicted (protected fraction 0) and on their way back, 20 queued jobs behind; requests alternate"""
    ev = [(1, 3, 7, 8, 9, 13)[q % 6] for q in range(Q)]
    lens = [k + 20 for k in ev]
    wl = SC._pool(lens, reqs=_alternating_reqs(lens))
    used = _packed_runs(wl, range(Q), ev)
    queued_cpu = int(sum(wl.job_req[j, W.CPU] for ids in wl.queued for j in ids))
    wl.node_total = np.tile(wl.node_total[0], (used + queued_cpu // 32_000 + 5, 1))
    wl.queue_weight = _distinct_weights(Q)
    wl.global_burst = 2 * Q * 20 // 3
    wl.config.prefer_large_job_ordering = prefer_large

    def check(c, want, others):
        assert _all_return(c.wl, want) == sum(ev)
        assert len(_new_scheduled(c.wl, want)) == c.wl.global_burst
    return Case(wl, name_rank=np.arange(Q)[::-1].copy(), check=check)


def _evicted_cut():
    """queue 0: 40 running jobs, evicted, returning: its stream is cut at the cap of 32 (W_SEG flag 4); 69 queues of 10 queued jobs beside it"""
    Q = 70
    wl = SC._pool([40] + [10] * (Q - 1), n_nodes=2 + (Q - 1) * 10 // 32 + 5)
    _packed_runs(wl, [0], [40])

    def check(c, want, others):
        assert _all_return(c.wl, want) == 40

    def cpu(c, st, trace):
        assert "open q0 evCnt 32" in trace, trace[:400]
    return Case(wl, check=check, cpu=cpu)


def _falling_keys(L, prefer_large, shift):
    """66 queues of L jobs of two classes, requests alternating: of every eight list entries three are of the higher class, from element `shift` on (SC._alternating's mixed
    construction; the iterator serves a queue in LIST order whatever the keys).  The class rises — the key falls below the running maximum in front of it — at elements
    8 + shift and 16 + shift: shift 0 the first entry of a chunk (W_FIX), shift 1 and 2 inside one (W_PACK)"""
    Q = 66
    lens = [L] * Q
    wl = SC._pool(lens, reqs=_alternating_reqs(lens), global_burst=2 * Q * L // 3)
    wl.config.pc_priority, wl.config.pc_preemptible = [0, 1], [1, 1]
    pc = np.zeros(Q * L, dtype=np.int32)
    for ids in wl.queued:
        pc[ids] = (np.arange(L) - shift) % 8 < 3
    wl.job_pc = pc
    wl.queue_weight = _distinct_weights(Q)
    wl.config.prefer_large_job_ordering = prefer_large

    def check(c, want, others):
        rises = [e for e in (8 + shift, 16 + shift) if e < L]
        assert rises or L <= 8      # (7 and 8: one chunk, the class falls once)
        for ids in c.wl.queued:
            for e in rises:
                assert pc[ids[e]] > pc[ids[e - 1]] and pc[ids[e]] > pc[ids[7 + 8 * ((e - 8) // 8)]]      # above its predecessor's and above the last entry's of the chunk in front
        assert len(_new_scheduled(c.wl, want)) == c.wl.global_burst
    return Case(wl, check=check)


# ---------------------------------------------------------------------------------------------------------------- C. where a run must stop
def _queue_tokens(evicted_front):
    Q = 72
    tokens = [(0, 1, 7, 8, 9, 31, 32, 33)[q % 8] for q in range(Q)]
    lens = [43 if evicted_front and q % 3 == 0 else 40 for q in range(Q)]
    wl = SC._pool(lens, queue_burst=64, n_nodes=Q * 43 // 32 + 8)
    if evicted_front:
        marked = list(range(0, Q, 3))
        _packed_runs(wl, marked, [3] * len(marked))

    def check(c, want, others):
        for q, ids in enumerate(c.wl.queued):      # the returning evicted jobs take no token
            hit = np.nonzero(_reasons(want, ids) == QUEUE_RATE_LIMIT)[0].tolist()
            assert hit == [tokens[q]], (q, hit)
            assert all(int(j) in want.scheduled for j in ids[:tokens[q]])
    return Case(wl, tokens=tokens, name_rank=np.random.default_rng(72).permutation(Q), check=check)


def _global_tokens(burst, evicted_front):
    """70 queues of 5 one-core jobs; evicted_front: queues 0 ... 9 have one running job each, evicted and returning ahead of the new jobs: they take no global token"""
    Q = 70
    lens = [6 if evicted_front and q < 10 else 5 for q in range(Q)]
    wl = _four_core_nodes(SC._pool(lens, global_burst=max(burst, 1)), Q * 6)
    wl.global_burst = burst
    if evicted_front:
        for q in range(10):
            j = wl.queued[q][0]
            wl.job_node[j], wl.job_run_ts[j] = q, q
            wl.queued[q] = wl.queued[q][1:]

    def check(c, want, others):
        assert (np.asarray(want.job_unschedulable_reason) == GLOBAL_RATE_LIMIT).any()
        assert len(_new_scheduled(c.wl, want)) == burst
        if evicted_front:
            assert _all_return(c.wl, want) == 10
    return Case(wl, check=check)


def _lookback(lb):
    """70 queues of 40, longer than the limit; every third queue has three running jobs, evicted and returning, in front of its queued part"""
    Q = 70
    lens = [43 if q % 3 == 0 else 40 for q in range(Q)]
    wl = SC._pool(lens, lookback=lb, n_nodes=Q * 43 // 32 + 8)
    marked = list(range(0, Q, 3))
    _packed_runs(wl, marked, [3] * len(marked))

    def check(c, want, others):
        new = _new_scheduled(c.wl, want)
        pos = _positions(c.wl)
        assert len(new) == Q * lb and all(pos[j][1] < lb for j in new)      # the first lb jobs of every queue, whether its head was queued or evicted
    return Case(wl, check=check)


def _pool_too_small(capacity):
    """65 queues of 40 identical jobs and room for `capacity` of them: the first entry without a node lies in the second batch of 64 staged entries"""
    Q = 65
    wl = SC._pool([40] * Q)
    rows = [(16 * W.Gi, 4_000, 4 * W.Gi, 0)] * (capacity // 4) + ([(16 * W.Gi, 1_000 * (capacity % 4), 4 * W.Gi, 0)] if capacity % 4 else [])
    wl.node_total = np.array(rows, dtype=np.int64)

    def check(c, want, others):
        assert 64 < len(want.scheduled) == capacity < 128 + 64
        assert (np.asarray(want.job_unschedulable_reason) == JOB_DOES_NOT_FIT).any()
    return Case(wl, name_rank=np.arange(Q)[::-1].copy(), check=check)


# ---------------------------------------------------------------------------------------------------------------- the table
def cases():
    out = {}
    for Q in QUEUE_COUNTS:
        for tag, rank in _ranks(Q).items():
            out[f"a-identical-{Q}-{tag}"] = _identical(Q, rank)
            if tag != "identity":
                out[f"a-identical-{Q}-{tag}"].needs = (("identity", f"a-identical-{Q}-identity"),)
    for Q in (65, 73, 79, 80, 81, 97, 129, 257):
        out[f"a-pairs-{Q}-identity"] = _pairs(Q, False)
        out[f"a-pairs-{Q}-swapped"] = _pairs(Q, True)
        out[f"a-pairs-{Q}-swapped"].needs = (("identity", f"a-pairs-{Q}-identity"),)
    for Q in (65, 72, 79, 81, 96, 130, 257):
        out[f"a-no-ties-{Q}-identity"] = _no_ties(Q, False)
        out[f"a-no-ties-{Q}-reversed"] = _no_ties(Q, True)
        out[f"a-no-ties-{Q}-reversed"].needs = (("identity", f"a-no-ties-{Q}-identity"),)
    for Q in (70, 97):
        for tag, rank in _ranks(Q).items():
            if tag != "permuted":
                out[f"a-ranges-0-1-2-40-{Q}-{tag}"] = _ranges([(0, 1, 2, 40)[q % 4] for q in range(Q)], rank)
    for tag, rank in _ranks(65).items():
        if tag != "permuted":
            out[f"a-ranges-300-and-ones-{tag}"] = _ranges([300] + [1] * 64, rank)
    out["a-barrier-tie-lowest"] = _barrier_tie(0)
    for tag, r in (("fifth", 4), ("highest", 64)):
        out[f"a-barrier-tie-{tag}"] = _barrier_tie(r)
        out[f"a-barrier-tie-{tag}"].needs = (("lowest", "a-barrier-tie-lowest"),)
    out["b-queued-lengths"] = _queued_lengths()
    for p in POSITIONS:
        out[f"b-gang-barrier-{p}"] = _gang_barrier(p)
    for p in POSITIONS:
        out[f"b-unfeasible-barrier-{p}"] = _unfeasible_barrier(p, False)
    for p in (0, 1, 8):
        out[f"b-unfeasible-barrier-{p}-evicted-in-front"] = _unfeasible_barrier(p, True)
    for pl in (True, False):
        out["b-evicted-then-queued-" + ("prefer-large" if pl else "plain")] = _evicted_then_queued(pl)
    out["b-evicted-cut"] = _evicted_cut()
    for L in (7, 8, 9, 15, 16, 17, 24, 25):
        for pl in (True, False):
            for shift in (0, 1, 2) if L in (16, 25) else (0,):
                if shift == 0 or 8 + shift < L:
                    out[f"b-falling-keys-{L}-" + ("prefer-large" if pl else "plain") + (f"-shift{shift}" if shift else "")] = _falling_keys(L, pl, shift)
    out["c-queue-tokens"] = _queue_tokens(False)
    out["c-queue-tokens-evicted-in-front"] = _queue_tokens(True)
    for burst in (1, 63, 64, 65):
        out[f"c-global-tokens-{burst}"] = _global_tokens(burst, False)
    for burst in (0, 1, 63, 64, 65):      # (burst 0 without an evicted head starts no wide run: wideHeadOk asks for a global token; with one the run has P.noNew)
        out[f"c-global-tokens-{burst}-evicted-in-front"] = _global_tokens(burst, True)
    for lb in (1, 7, 8, 9, 32, 33):
        out[f"c-lookback-{lb}"] = _lookback(lb)
    for capacity in (100, 130):
        out[f"c-pool-too-small-{capacity}"] = _pool_too_small(capacity)
    return out


CASES = cases()
NAMES = list(CASES)
# (stream_runs, stream_jobs, stream_prepared) of the CPU build: what it counted when the cases were written.  They pin that a case still reaches the wide runs the way it
# did; the rounds themselves are compared with the oracle's.  A row may only be re-pinned with the reason written here.
PINS = {
    "a-identical-65-identity": (1, 871, 2080),
    "a-identical-65-reversed": (1, 871, 2080),
    "a-identical-65-permuted": (1, 871, 2080),
    "a-identical-72-identity": (1, 965, 2304),
    "a-identical-72-reversed": (1, 965, 2304),
    "a-identical-72-permuted": (1, 965, 2304),
    "a-identical-73-identity": (1, 978, 2336),
    "a-identical-73-reversed": (1, 978, 2336),
    "a-identical-73-permuted": (1, 978, 2336),
    "a-identical-79-identity": (1, 1058, 2528),
    "a-identical-79-reversed": (1, 1058, 2528),
    "a-identical-79-permuted": (1, 1058, 2528),
    "a-identical-80-identity": (1, 1071, 2560),
    "a-identical-80-reversed": (1, 1071, 2560),
    "a-identical-80-permuted": (1, 1071, 2560),
    "a-identical-81-identity": (1, 1085, 2592),
    "a-identical-81-reversed": (1, 1085, 2592),
    "a-identical-81-permuted": (1, 1085, 2592),
    "a-identical-96-identity": (1, 1285, 3072),
    "a-identical-96-reversed": (1, 1285, 3072),
    "a-identical-96-permuted": (1, 1285, 3072),
    "a-identical-97-identity": (1, 1298, 3104),
    "a-identical-97-reversed": (1, 1298, 3104),
    "a-identical-97-permuted": (1, 1298, 3104),
    "a-identical-130-identity": (1, 1738, 4160),
    "a-identical-130-reversed": (1, 1738, 4160),
    "a-identical-130-permuted": (1, 1738, 4160),
    "a-identical-257-identity": (1, 3431, 8224),
    "a-identical-257-reversed": (1, 3431, 8224),
    "a-identical-257-permuted": (1, 3431, 8224),
    "a-pairs-65-identity": (1, 871, 2080),
    "a-pairs-65-swapped": (1, 871, 2080),
    "a-pairs-73-identity": (1, 978, 2336),
    "a-pairs-73-swapped": (1, 978, 2336),
    "a-pairs-79-identity": (1, 1058, 2528),
    "a-pairs-79-swapped": (1, 1058, 2528),
    "a-pairs-80-identity": (1, 1071, 2560),
    "a-pairs-80-swapped": (1, 1071, 2560),
    "a-pairs-81-identity": (1, 1085, 2592),
    "a-pairs-81-swapped": (1, 1085, 2592),
    "a-pairs-97-identity": (1, 1298, 3104),
    "a-pairs-97-swapped": (1, 1298, 3104),
    "a-pairs-129-identity": (1, 1725, 4128),
    "a-pairs-129-swapped": (1, 1725, 4128),
    "a-pairs-257-identity": (1, 3431, 8224),
    "a-pairs-257-swapped": (1, 3431, 8224),
    "a-no-ties-65-identity": (1, 871, 2080),
    "a-no-ties-65-reversed": (1, 871, 2080),
    "a-no-ties-72-identity": (1, 965, 2304),
    "a-no-ties-72-reversed": (1, 965, 2304),
    "a-no-ties-79-identity": (1, 1058, 2528),
    "a-no-ties-79-reversed": (1, 1058, 2528),
    "a-no-ties-81-identity": (1, 1085, 2592),
    "a-no-ties-81-reversed": (1, 1085, 2592),
    "a-no-ties-96-identity": (1, 1285, 3072),
    "a-no-ties-96-reversed": (1, 1285, 3072),
    "a-no-ties-130-identity": (1, 1738, 4160),
    "a-no-ties-130-reversed": (1, 1738, 4160),
    "a-no-ties-257-identity": (1, 3431, 8224),
    "a-no-ties-257-reversed": (1, 3431, 8224),
    "a-ranges-0-1-2-40-70-identity": (1, 488, 596),
    "a-ranges-0-1-2-40-70-reversed": (1, 488, 596),
    "a-ranges-0-1-2-40-97-identity": (1, 688, 840),
    "a-ranges-0-1-2-40-97-reversed": (1, 688, 840),
    "a-ranges-300-and-ones-identity": (3, 242, 364),
    "a-ranges-300-and-ones-reversed": (3, 242, 364),
    "a-barrier-tie-lowest": (1, 219, 640),
    "a-barrier-tie-fifth": (2, 219, 1277),
    "a-barrier-tie-highest": (2, 219, 1217),
    "b-queued-lengths": (1, 896, 1336),
    "b-gang-barrier-0": (2, 2752, 2869),
    "b-gang-barrier-1": (7, 2695, 10304),
    "b-gang-barrier-7": (9, 2656, 12908),
    "b-gang-barrier-8": (7, 2702, 11336),
    "b-gang-barrier-9": (7, 2700, 11235),
    "b-gang-barrier-15": (8, 2656, 10748),
    "b-gang-barrier-16": (7, 2703, 9311),
    "b-gang-barrier-17": (8, 2656, 10083),
    "b-unfeasible-barrier-0": (24, 1632, 8256),
    "b-unfeasible-barrier-1": (6, 1536, 8026),
    "b-unfeasible-barrier-7": (7, 1598, 7037),
    "b-unfeasible-barrier-8": (7, 1598, 6734),
    "b-unfeasible-barrier-9": (7, 1598, 6431),
    "b-unfeasible-barrier-15": (7, 1598, 4613),
    "b-unfeasible-barrier-16": (7, 1598, 4310),
    "b-unfeasible-barrier-17": (7, 1598, 4007),
    "b-unfeasible-barrier-0-evicted-in-front": (7, 1667, 8399),
    "b-unfeasible-barrier-1-evicted-in-front": (7, 1667, 8096),
    "b-unfeasible-barrier-8-evicted-in-front": (7, 1667, 5975),
    "b-evicted-then-queued-prefer-large": (1, 1403, 1859),
    "b-evicted-then-queued-plain": (1, 1403, 1859),
    "b-evicted-cut": (2, 730, 730),
    "b-falling-keys-7-prefer-large": (1, 308, 462),
    "b-falling-keys-7-plain": (1, 308, 462),
    "b-falling-keys-8-prefer-large": (1, 352, 528),
    "b-falling-keys-8-plain": (1, 352, 528),
    "b-falling-keys-9-prefer-large": (1, 396, 594),
    "b-falling-keys-9-plain": (1, 396, 594),
    "b-falling-keys-15-prefer-large": (1, 660, 990),
    "b-falling-keys-15-plain": (1, 660, 990),
    "b-falling-keys-16-prefer-large": (1, 704, 1056),
    "b-falling-keys-16-prefer-large-shift1": (1, 704, 1056),
    "b-falling-keys-16-prefer-large-shift2": (1, 704, 1056),
    "b-falling-keys-16-plain": (1, 704, 1056),
    "b-falling-keys-16-plain-shift1": (1, 704, 1056),
    "b-falling-keys-16-plain-shift2": (1, 704, 1056),
    "b-falling-keys-17-prefer-large": (1, 748, 1122),
    "b-falling-keys-17-plain": (1, 748, 1122),
    "b-falling-keys-24-prefer-large": (1, 1056, 1584),
    "b-falling-keys-24-plain": (1, 1056, 1584),
    "b-falling-keys-25-prefer-large": (1, 1100, 1650),
    "b-falling-keys-25-prefer-large-shift1": (1, 1100, 1650),
    "b-falling-keys-25-prefer-large-shift2": (1, 1100, 1650),
    "b-falling-keys-25-plain": (1, 1100, 1650),
    "b-falling-keys-25-plain-shift1": (1, 1100, 1650),
    "b-falling-keys-25-plain-shift2": (1, 1100, 1650),
    "c-queue-tokens": (24, 829, 17197),
    "c-queue-tokens-evicted-in-front": (35, 739, 26833),
    "c-global-tokens-1": (1, 1, 350),
    "c-global-tokens-63": (1, 63, 350),
    "c-global-tokens-64": (1, 64, 350),
    "c-global-tokens-65": (1, 65, 350),
    "c-global-tokens-0-evicted-in-front": (3, 3, 210),
    "c-global-tokens-1-evicted-in-front": (1, 11, 360),
    "c-global-tokens-63-evicted-in-front": (1, 73, 360),
    "c-global-tokens-64-evicted-in-front": (1, 74, 360),
    "c-global-tokens-65-evicted-in-front": (1, 75, 360),
    "c-lookback-1": (7, 9, 743),
    "c-lookback-7": (8, 429, 1302),
    "c-lookback-8": (8, 499, 1372),
    "c-lookback-9": (8, 569, 1442),
    "c-lookback-32": (8, 2179, 2982),
    "c-lookback-33": (9, 2249, 3191),
    "c-pool-too-small-100": (1, 100, 2080),
    "c-pool-too-small-130": (1, 130, 2080),
}
_ORACLE_ROUNDS = {}


def oracle_round(name, oracle):
    """the oracle's round of a case: computed once, shared, never changed"""
    if name not in _ORACLE_ROUNDS:
        _ORACLE_ROUNDS[name] = run(oracle, CASES[name])[0]
    return _ORACLE_ROUNDS[name]


def _checked_oracle_round(name, oracle):
    c = CASES[name]
    want = oracle_round(name, oracle)
    if c.check:
        c.check(c, want, {k: oracle_round(other, oracle) for k, other in c.needs})
    return c, want


ENV_VARS = ("ASCHED_WIDE", "ASCHED_KEY_WORDS", "ASCHED_STREAM", "ASCHED_MERGE")
STATS = ("stream_runs", "stream_jobs", "stream_prepared", "fast_iterations", "generic_iterations")


def _set_env(monkeypatch, env):
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, x in env.items():
        monkeypatch.setenv(v, x)


@pytest.mark.parametrize("name", NAMES)
def test_wide_run_edges_cpu_build(hostsim_lib, oracle_lib, name, monkeypatch, capfd):
    c, want = _checked_oracle_round(name, oracle_lib)
    _set_env(monkeypatch, c.env)
    monkeypatch.setenv("HS_WIDE_TRACE", "1")
    capfd.readouterr()
    r, st = run(hostsim_lib, c)
    trace = capfd.readouterr().err
    print(f"{name}: queued {sum(len(q) for q in c.wl.queued)}, scheduled {len(want.scheduled)}, " + ", ".join(f"{k} {st[k]}" for k in STATS))
    assert_same_round(r, want)
    assert st["stream_runs"] > 0 and st["stream_jobs"] > 0, "no wide run"
    assert (st["stream_runs"], st["stream_jobs"], st["stream_prepared"]) == PINS[name]
    if c.cpu:
        c.cpu(c, st, trace)


ARMS = (("default", {}), ("wide_off", {"ASCHED_WIDE": "0"}))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_wide_run_edges_gpu(hip_lib, oracle_lib, name, monkeypatch):
    """product library: both arms' rounds equal the oracle's; the default arm makes wide runs, the other none"""
    c, want = _checked_oracle_round(name, oracle_lib)
    st = {}
    for arm, env in ARMS:
        _set_env(monkeypatch, {**c.env, **env})
        r, st[arm] = run(hip_lib, c, deadline=DEADLINE_S)
        print(f"{name} [{arm}]: " + ", ".join(f"{k} {st[arm][k]}" for k in STATS))
        assert_same_round(r, want)
    assert st["default"]["stream_runs"] > 0 and st["default"]["stream_jobs"] > 0 and st["wide_off"]["stream_runs"] == 0


# ---------------------------------------------------------------------------------------------------------------- D. one handle: wide, 12 queues, wide
def _reuse_rounds(lib, cs, deadline=0.0):
    """ONE handle through several rounds, nodes and jobs uploaded again before each (tests/test_z_wide_runs.py _reuse_rounds, with this file's prepare)"""
    s = W.load(lib, cs[0].wl)
    out = []
    for i, c in enumerate(cs):
        wl = c.wl
        if i:
            s.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=wl.node_labels, id_rank=wl.node_id_rank)
            W.set_jobs(s, wl)
        prepare(s, wl, c.name_rank, c.tokens)
        if deadline:
            s.set_deadline(deadline)
        out.append((s.schedule_round(), s.round_stats()))
    s.close()
    return out


_REUSE = {}


def _reuse_cases(oracle):
    """B's evicted-then-queued pool at 70, 12 and 70 queues (the third under the identity name rank, the others reversed) and the oracle's rounds on one handle"""
    if not _REUSE:
        cs = [_evicted_then_queued(True, 70), _evicted_then_queued(True, 12), _evicted_then_queued(True, 70)]
        cs[2].name_rank = np.arange(70)
        _REUSE["cases"], _REUSE["want"] = cs, [r for r, _ in _reuse_rounds(oracle, cs)]
        for c, want in zip(cs, _REUSE["want"]):
            c.check(c, want, {})
    return _REUSE["cases"], _REUSE["want"]


def test_a_handle_goes_wide_few_wide_with_evicted_parts(hostsim_lib, oracle_lib, monkeypatch):
    cs, want = _reuse_cases(oracle_lib)
    _set_env(monkeypatch, {})
    got = _reuse_rounds(hostsim_lib, cs)
    for (r, st), b in zip(got, want):
        assert_same_round(r, b)
    assert got[0][1]["stream_runs"] > 0 and got[2][1]["stream_runs"] > 0


@pytest.mark.gpu
def test_a_handle_goes_wide_few_wide_with_evicted_parts_gpu(hip_lib, oracle_lib, monkeypatch):
    cs, want = _reuse_cases(oracle_lib)
    for arm, env in ARMS:
        _set_env(monkeypatch, env)
        got = _reuse_rounds(hip_lib, cs, deadline=DEADLINE_S)
        for (r, st), b in zip(got, want):
            assert_same_round(r, b)
        assert (got[0][1]["stream_runs"] > 0 and got[2][1]["stream_runs"] > 0) == (arm == "default")


# ---------------------------------------------------------------------------------------------------------------- E. two-word keys
TWO_WORD_STREAM_RUNS_ZERO = True      # whether a handle under the forced two-word key layout makes NO stream run at 70 queues


def _two_word_case():
    c = _evicted_then_queued(True, 70)
    c.env = {"ASCHED_KEY_WORDS": "2"}
    return c


def test_two_word_keys_at_70_queues(hostsim_lib, oracle_lib, monkeypatch):
    """k_control_wk at more than 64 queues: the round under ASCHED_KEY_WORDS=2 (read at nodes_upsert / jobs_set) is the oracle's"""
    c = _two_word_case()
    _set_env(monkeypatch, {})
    want = run(oracle_lib, c)[0]
    c.check(c, want, {})
    _set_env(monkeypatch, c.env)
    r, st = run(hostsim_lib, c)
    print("two-word keys, 70 queues: " + ", ".join(f"{k} {st[k]}" for k in STATS))
    assert_same_round(r, want)
    assert (st["stream_runs"] == 0) == TWO_WORD_STREAM_RUNS_ZERO


@pytest.mark.gpu
def test_two_word_keys_at_70_queues_gpu(hip_lib, oracle_lib, monkeypatch):
    c = _two_word_case()
    _set_env(monkeypatch, {})
    want = run(oracle_lib, c)[0]
    for arm, env in ARMS:
        _set_env(monkeypatch, {**c.env, **env})
        r, st = run(hip_lib, c, deadline=DEADLINE_S)
        print(f"two-word keys, 70 queues [{arm}]: " + ", ".join(f"{k} {st[k]}" for k in STATS))
        assert_same_round(r, want)
        assert (st["stream_runs"] == 0) == (TWO_WORD_STREAM_RUNS_ZERO or arm == "wide_off")
