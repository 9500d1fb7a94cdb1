"""The fairness optimiser's GPU-only code at its edges: the one-wave-per-node kernel (kernels_opt.h optScoreNodeWave: k_opt_score_wave, k_opt_detail_wave,
k_opt_detail_sel), the candidate selection on the device (k_opt_select, k_opt_select_final, optSelLess) and the node -> jobs index (k_opt_count, k_opt_scan,
k_opt_scatter).  The CPU build scores with the serial optScoreNodeE and never selects on the device, so only the `gpu` tests below reach that code; what they
compare it with is the oracle, the whole result with ==, floats included (the serial routine's doubles depend on the order of its operations).

Every case is hand-built from build() of test_z_optimiser.py: two resources, four queues, a few hundred jobs at the most.  Each case runs twice:
  * test_case_cpu_build: oracle == CPU build on the whole result, then the case's own assertions — computed from the ORACLE's result and the input as constructed —
    that the case is in the state it is named after (job count of the node, candidates, victims, the winner, a real tie ...);
  * test_case_gpu: oracle == HIP library, in both forms.  per_node=True: every node's score comes back and the host selects; the short form: the device selects
    (k_opt_select .. k_opt_detail_sel), unless a node holds more than 64 jobs — then the wave kernel reports overflow and the call falls back to the long way
    (k_opt_score_big, host selection, k_opt_detail_wave / k_opt_detail_big).  The short result equals the matching keys of the long one (both()).

"Position" below is a job's place among its node's jobs in id order.  k_opt_scatter fills the index with atomics and promises no order, so the lane a job lands in is the
hardware's choice (in practice the id order while one wave scatters the node); no result may depend on it.

Which path a case takes follows from the job counts per node (the PATH column):
  A. lanes of one wave — one scored node, plus a one-cpu node held by a non-preemptible job
     lanes-N      N one-cpu jobs, all candidates, the job needs all: N = 1, 2, 47, 48, 49, 63 wave; 64 wave, used == 64 (full ballot, m2 == ~0, optDest at lane 63);
                  65 k_opt_score_big + fall-back
     sums-N       N = 47, 63, 64 victims of unequal cost, all counted: the cost and impact sums differ in their last bits when added in another order                wave
     stop-K       64 candidates, the first fitting prefix is K = 1, 32, 33, 63, 64 victims; stop-none: all 64 do not suffice (the node allocates less than its total)   wave
     holes-R      64 jobs, non-candidates interleaved (non-preemptible class / gang member / scheduled above the job / larger than max_job_size_to_preempt), each
                  reason once in positions 0, 31, 32, 63 over R = 0..3; holes-all: m == 0 on 64 jobs                                                          wave
     over-70-30   70 jobs, 30 candidates: the wave kernel overflows on the job count, the serial routine never on the candidates                                big + fall-back
     order-id / order-mirror / order-mix / order-two-resources / lease-permuted: the orderings (see each)                                                       wave
  B. grid-N       N = 1 .. 2049 nodes, occupied ones (2 .. 64 jobs) at 0, N-1, either side of the multiples of 256 and 1024, around a scan chunk's end          wave
  C. sel-*        the selection: ties across wave / block boundaries, id ranks, impact, ideal nodes, the strict threshold, cost 0, no candidate                 wave;
     sel-fallback-*: one node of 70 jobs among smaller ones                                                                                                   big + fall-back
  D. state-*      the index across bind / unbind, jobs_patch, and a larger pool after a smaller one in the same process                                         wave
"""
import math

import numpy as np
import pytest

from test_z_optimiser import GI, PC_NAMES, PCS, QA, QB, QC, QD, build

QS = [QA, QB, QC, QD]
NOW = 5000
BLOCKED = ("D", 1, 0, "pc3", 1, 900)   # what holds the one-cpu node 1 of the single-node cases: not preemptible


def both(s, job, **kw):
    """the call in both forms; the short one (the device selects) equals the matching keys of the long one"""
    kw.setdefault("min_improvement_pct", -1e9)
    kw.setdefault("now_ms", NOW)
    long = s.optimiser_schedule_job(job, per_node=True, **kw)
    short = s.optimiser_schedule_job(job, **kw)
    assert short == {k: long[k] for k in short}, (short, {k: long[k] for k in short})
    return long


def one_node(lib, on_node, want, want_mem=0, job_pc="pc2", spare=(0, 0), **kw):
    """node 0 holds on_node = [(queue, cpu, mem, pc, lease ms)] as jobs 0 .. and is full but for `spare` (cpu, mem); node 1 is the blocked one-cpu node; the last job is
    the queued one of queue A -> (scheduler, its id)"""
    jobs = [(q, c, m, pc, 0, lease) for q, c, m, pc, lease in on_node] + [BLOCKED, ("A", want, want_mem, job_pc, -1, 0)]
    nodes = [(sum(j[1] for j in on_node) + spare[0], sum(j[2] for j in on_node) + spare[1], False), (1, 0, False)]
    return build(lib, nodes, jobs, QS, **kw), len(jobs) - 1


def unit_jobs(cnt):
    """cnt one-cpu jobs of four queues, every fifth scheduled below the job's priority, distinct lease times in no order"""
    return [("ABCD"[i % 4], 1, 0, "pc2" if i % 5 else "pc1", 1000 + (i * 37) % 997) for i in range(cnt)]


NOT_SCHEDULED = (False, 0, 0.0, 0.0)
CASES = {}


def case(name):
    def reg(fn):
        CASES[name] = fn
        return fn
    return reg


# ---------------------------------------------------------------- A. lanes of one wave
def _lanes(cnt):
    def run(lib, oracle):
        s, j = one_node(lib, unit_jobs(cnt), cnt)
        r = both(s, j)
        s.close()

        def check(w):
            assert w["node"] == 0 and w["scores"][0][:2] == (True, cnt) and sorted(w["preempted"]) == list(range(cnt))   # the node's job count = candidates = victims
            assert w["scores"][1] == NOT_SCHEDULED and (w["cost"] > 0 or cnt == 1) and 0.99 < w["impact"] < 1.01   # (job 0 alone is a priority preemption: no cost)
        return [r], check
    return run


for _n in (1, 2, 47, 48, 49, 63, 64, 65):
    CASES[f"lanes-{_n}"] = _lanes(_n)


def _sums(cnt):
    """victims of unequal cost, every one of them counted (a large tainted node keeps every queue below its fair share): schedulingCost and the queues' cost changes are
    sums whose double depends on the order of the addends — restated here along the oracle's preemption order, and shown to differ when summed backwards"""
    def run(lib, oracle):
        on = [("ABCD"[i % 4], 1 + (i * 7) % 5, 0, "pc2", 1000 + (i * 37) % 997) for i in range(cnt)]
        s, j = one_node(lib, on, sum(x[1] for x in on), extra_total=(937, 0))
        r = both(s, j)
        s.close()

        def check(w):
            pre = w["preempted"]
            total = (sum(x[1] for x in on) + 1 + 937) * 1000

            def cost(order):
                t = 0.0
                for v in order:
                    t += on[v][1] * 1000 / total
                return t

            def impact(order):
                best = 0.0
                for q in "ABCD":
                    held = sum(x[1] for x in on if x[0] == q) + (q == "D")
                    best = max(best, abs(0.0 - cost([v for v in order if on[v][0] == q])) / (held * 1000 / total))
                return best
            assert w["node"] == 0 and sorted(pre) == list(range(cnt))
            assert cost(pre) == w["cost"] != cost(pre[::-1])
            assert impact(pre) == w["impact"] != impact(pre[::-1])
        return [r], check
    return run


for _n in (47, 63, 64):
    CASES[f"sums-{_n}"] = _sums(_n)


def _stop(k):
    """64 candidates on a node of 66 cpus that allocates 64: the job passes the static check (the node's total) up to 66 cpus, the victims free 64 at the most"""
    def run(lib, oracle):
        want = 65 if k is None else k
        s, j = one_node(lib, unit_jobs(64), want, spare=(2, 0), allocatable=[(64, 0), (1, 0)])
        r = both(s, j)
        s.close()

        def check(w):
            if k is None:
                assert w["node"] == -1 and w["scores"][0] == NOT_SCHEDULED and w["preempted"] == []
            else:
                assert w["node"] == 0 and w["scores"][0][:2] == (True, k) and len(set(w["preempted"])) == k
        return [r], check
    return run


for _k in (1, 32, 33, 63, 64, None):
    CASES[f"stop-{'none' if _k is None else _k}"] = _stop(_k)

REASONS = ("np", "gang", "above", "big")
EDGE_LANES = (0, 31, 32, 63)
HOLE_DENSITY = (5, 6, 9, 16)


def hole_kind(r, p):
    """what sits in position p of the node's 64 jobs in case holes-r: a reason it is no candidate, or None"""
    if r == "all":
        return REASONS[(p * 3 + p // 7) % 4]
    if p in EDGE_LANES:
        return REASONS[(EDGE_LANES.index(p) + r) % 4]
    h = (p * 7 + r * 3) % HOLE_DENSITY[r]
    return REASONS[h] if h < 4 and (p + r) % 3 else None


def _holes(r):
    def run(lib, oracle):
        kinds = [hole_kind(r, p) for p in range(64)]
        cand = [p for p in range(64) if kinds[p] is None]
        m = len(cand)
        want = 1 if m == 0 else m - 3 * r
        on = [("ABCD"[p % 4], 2 if kinds[p] == "big" else 1, 0, "pc2np" if kinds[p] == "np" else ("pc2", "pc1", "pc0")[p % 3], 1000 + (p * 41) % 499) for p in range(64)]
        s, j = one_node(lib, on, want, gang_id=[p if p < 64 and kinds[p] == "gang" else -1 for p in range(66)])
        for p in range(64):
            if kinds[p] == "above":   # a run scheduled at a priority above its class's (and the job's)
                s.unbind(p, 0)
                s.bind(p, 0, 3)
        r_ = both(s, j, max_job_size_to_preempt=[0, 1000])
        s.close()

        def check(w):
            if m == 0:
                assert w["node"] == -1 and w["scores"][0] == NOT_SCHEDULED
            else:
                assert 0 < want <= m < 64 and w["node"] == 0 and w["scores"][0][:2] == (True, want)
                assert len(set(w["preempted"])) == want and set(w["preempted"]) <= set(cand)
        return [r_], check
    return run


for _r in (0, 1, 2, 3, "all"):
    CASES[f"holes-{_r}"] = _holes(_r)


def test_every_reason_sits_in_every_edge_lane_once():
    for reason in REASONS:
        assert sorted(p for r in range(4) for p in EDGE_LANES if hole_kind(r, p) == reason) == list(EDGE_LANES)
    assert len({sum(hole_kind(r, p) is None for p in range(64)) for r in range(4)}) == 4   # the candidate count varies
    assert all(hole_kind("all", p) for p in range(64))


@case("over-70-30")
def _over(lib, oracle):
    on = [("ABCD"[i % 4], 1, 0, "pc2" if i % 7 < 3 else "pc3", 1000 + (i * 37) % 997) for i in range(70)]
    s, j = one_node(lib, on, 20)
    r = both(s, j)
    s.close()

    def check(w):
        assert sum(1 for x in on if x[3] == "pc2") == 30 and w["node"] == 0 and w["scores"][0][:2] == (True, 20)
        assert all(on[v][3] == "pc2" for v in w["preempted"])
    return [r], check


@case("order-id")
def _order_id(lib, oracle):
    """64 jobs of one queue, bound after round_prepare: equal priority, cost and age (0) — the job id alone orders them"""
    jobs = [("B", 1, 0, "pc2", -1, 1000) for _ in range(64)] + [BLOCKED, ("A", 40, 0, "pc2", -1, 0)]
    s = build(lib, [(64, 0, False), (1, 0, False)], jobs, QS, extra_alloc=[("B", "pc2", [0, 64000])])
    for i in range(64):
        s.bind(i, 0, 2)
    r = both(s, 65)
    s.close()

    def check(w):
        assert w["node"] == 0 and w["preempted"] == list(range(40))
    return [r], check


@case("order-mirror")
def _order_mirror(lib, oracle):
    """queues B and C of equal weight hold mirrored jobs: the weighted cost after each preemption ties across the queues at every step, and the tie-break
    (priority, cost, AGE, JOB ID) decides: in every pair of victims the younger one goes first, the lower id where the ages are equal"""
    on = []
    for k in range(32):
        pair = [("B", 1 + k % 2, 0, "pc2", 1000 + 10 * k), ("C", 1 + k % 2, 0, "pc2", 1000 + 10 * k + (0, 3, -3)[k % 3])]
        on += pair[::-1] if k % 4 == 3 else pair
    s, j = one_node(lib, on, 60)
    r = both(s, j)
    s.close()

    def check(w):
        pre = w["preempted"]
        assert w["node"] == 0 and len(pre) >= 40
        by_id = by_age = 0
        for t in range(0, len(pre) - 1, 2):
            a, b = on[pre[t]], on[pre[t + 1]]
            assert {a[0], b[0]} == {"B", "C"} and a[1] == b[1], (t, a, b)
            assert (-a[4], pre[t]) < (-b[4], pre[t + 1]), (t, a, b)
            by_id += a[4] == b[4]
            by_age += a[4] != b[4] and pre[t] > pre[t + 1]
        assert by_id >= 5 and by_age >= 5   # both tie-breaks decided, the age also against the id order
    return [r], check


@case("order-mix")
def _order_mix(lib, oracle):
    """three queues of different weights, victims scheduled below the job's priority and at it; queue B starts below its fair share (12 of 65 cpus against 0.2):
    its victims cost, the cost is summed in preemption order"""
    on = [("B" if i % 16 < 3 else "C" if i % 16 < 8 else "D", 1, 0, "pc1" if i % 3 == 0 else "pc2", 1000 + (i * 29) % 499) for i in range(64)]
    s, j = one_node(lib, on, 50)
    r = both(s, j)
    s.close()

    def check(w):
        pre = w["preempted"]
        assert [sum(1 for x in on if x[0] == q) for q in "BCD"] == [12, 20, 32]
        assert w["node"] == 0 and len(pre) == 50 and {on[v][0] for v in pre} == {"B", "C", "D"} and {on[v][3] for v in pre} == {"pc1", "pc2"}
        assert 0 < w["cost"] < 0.99 * 50 / 65      # some victims cost, some (priority preemptions, queues above their share) do not
        assert any(on[v][3] == "pc2" and on[v][0] == "B" for v in pre)
        assert [on[v][3] for v in pre[:5]] == ["pc1"] * 5   # priority preemptions first
    return [r], check


@case("order-two-resources")
def _order_two_resources(lib, oracle):
    """requests that differ in both resources: along the preemption order the cpus suffice earlier than the memory, and the memory decides the prefix"""
    on = [("ABCD"[i % 4], 1 + i % 3, ((i * 5) % 4) * GI, "pc2", 1000 + (i * 31) % 499) for i in range(64)]
    cpu, mem = sum(x[1] for x in on) // 4, sum(x[2] for x in on) * 3 // 4 // GI * GI
    s, j = one_node(lib, on, cpu, want_mem=mem)
    r = both(s, j)
    s.close()

    def check(w):
        pre = w["preempted"]
        first_cpu = next(k + 1 for k in range(len(pre)) if sum(on[v][1] for v in pre[:k + 1]) >= cpu)
        first_mem = next(k + 1 for k in range(len(pre)) if sum(on[v][2] for v in pre[:k + 1]) >= mem)
        assert w["node"] == 0 and first_cpu < first_mem == len(pre) < 64
    return [r], check


@case("lease-permuted")
def _lease_permuted(lib, oracle):
    """one queue, equal costs: the age alone orders.  The lease times are a permutation of the job ids, and the node's jobs are every id that is no multiple of 4 (the
    others sit on node 1), so the position in the index, the job id and the age all order differently"""
    jobs, mine = [], []
    for i in range(84):
        if i % 4 == 0 and len(jobs) - len(mine) < 20:
            jobs.append(("D", 1, 0, "pc3", 1, 900))
        else:
            mine.append(len(jobs))
            jobs.append(("B", 1, 0, "pc2", 0, 1000 + 5 * ((len(mine) * 37 + 11) % 64)))
    assert len(mine) == 64
    jobs.append(("A", 30, 0, "pc2", -1, 0))
    s = build(lib, [(64, 0, False), (20, 0, False)], jobs, QS)
    r = both(s, len(jobs) - 1)
    s.close()

    def check(w):
        youngest_first = sorted(mine, key=lambda v: -jobs[v][5])
        assert len({jobs[v][5] for v in mine}) == 64 and w["node"] == 0 and w["preempted"] == youngest_first[:30]
        assert w["preempted"] != sorted(w["preempted"]) and w["preempted"] != sorted(w["preempted"], reverse=True)
    return [r], check


# ---------------------------------------------------------------- B. grid and index edges
GRID_COUNTS = (2, 64, 21, 5, 33, 3, 48, 7, 63, 4)


def grid_occupied(N):
    """0, N-1, either side of every multiple of 256 (and so of 1024) below N, and — where k_opt_scan gives a thread more than one node — either side of a chunk's end
    in the middle and the first node of the last chunk that holds any"""
    occ = {0, N - 1} | {x for k in range(256, N, 256) for x in (k - 1, k)}
    C = (N + 1023) // 1024
    if C > 1:
        occ |= {C * 341 - 1, C * 341, (N - 1) // C * C}
    return sorted(occ)


def _grid(N):
    def run(lib, oracle):
        occ = grid_occupied(N)
        nodes, jobs = [(1, 0, False)] * N, []
        for t, n in enumerate(occ):
            cnt = GRID_COUNTS[t % len(GRID_COUNTS)]
            nodes[n] = (cnt, 0, False)
            jobs += [("ABCD"[(i + t) % 4], 1, 0, "pc2" if (i + t) % 5 else "pc1", n, 1000 + (i * 37 + t * 11) % 997) for i in range(cnt)]
        jobs.append(("A", 2, 0, "pc2", -1, 0))
        s = build(lib, nodes, jobs, QS)
        r = both(s, len(jobs) - 1)
        s.close()

        def check(w):
            assert len(w["scores"]) == N and len(jobs) < 700
            for n in range(N):   # the empty one-cpu nodes cannot take the two-cpu job, every occupied node can with two victims
                assert w["scores"][n][:2] == ((True, 2) if n in occ else (False, 0)), n
            assert w["scores"][N - 1][1] > 0 and w["node"] in occ and len(w["preempted"]) == 2
            assert N < 256 or 64 in [GRID_COUNTS[t % 10] for t in range(len(occ))]
        return [r], check
    return run


for _n in (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049):
    CASES[f"grid-{_n}"] = _grid(_n)


# ---------------------------------------------------------------- C. selection
def pool(lib, N, spec, want, id_rank=None, queues=QS, filler=(1, 0, False), more_jobs=()):
    """N nodes, `filler` but for spec = {node: (cpu, taint, [(queue, cpu, pc, lease ms)])}; the queued jobs come last: `more_jobs` [(queue, cpu)], then the one of queue A
    that wants `want` cpus -> (scheduler, its id)"""
    nodes, jobs = [filler] * N, []
    for n in sorted(spec):
        cpu, taint, on = spec[n]
        nodes[n] = (cpu, 0, taint)
        jobs += [(q, c, 0, pc, n, lease) for q, c, pc, lease in on]
    jobs += [(q, c, 0, "pc2", -1, 0) for q, c in more_jobs] + [("A", want, 0, "pc2", -1, 0)]
    return build(lib, nodes, jobs, queues, id_rank=id_rank), len(jobs) - 1


TWIN = (4, False, [("B", 1, "pc2", 1000), ("B", 1, "pc2", 1001), ("C", 1, "pc2", 1002), ("C", 1, "pc2", 1003)])   # identical content = bit-identical (cost, impact)


def ranks(kind, N, first=0):
    return {"index": None, "reversed": [N - 1 - n for n in range(N)], "rotated": [(n - first) % N for n in range(N)]}[kind]


def _tie(a, b, kind):
    def run(lib, oracle):
        N = 300
        rk = ranks(kind, N, b)
        s, j = pool(lib, N, {a: TWIN, b: TWIN}, 3, id_rank=rk)
        r = both(s, j)
        s.close()

        def check(w):
            assert w["scores"][a] == w["scores"][b] and w["scores"][a][0] and w["scores"][a][1] == 3 and w["scores"][a][2] > 0   # a real tie on (cost, impact)
            assert sum(1 for sc in w["scores"] if sc[0]) == 2
            assert w["node"] == (a if rk is None else min((a, b), key=lambda n: rk[n])) == (a if kind == "index" else b)   # the lower id rank wins
        return [r], check
    return run


for _a, _b in ((63, 64), (255, 256), (0, 299)):
    for _kind in ("index", "reversed", "rotated"):
        CASES[f"sel-tie-{_a}-{_b}-{_kind}"] = _tie(_a, _b, _kind)


@case("sel-impact")
def _sel_impact(lib, oracle):
    """equal cost (three victims of equal cost, all below their queues' fair shares), different impact: node 10 empties queue C's and D's whole allocation (impact 1),
    node 290 — in the second block — takes three of queue B's five jobs"""
    spec = {10: (3, False, [("B", 1, "pc2", 1000), ("C", 1, "pc2", 1001), ("D", 1, "pc2", 1002)]),
            290: (3, False, [("B", 1, "pc2", 1000), ("B", 1, "pc2", 1001), ("B", 1, "pc2", 1002)]),
            291: (1, False, [("B", 1, "pc2", 1003)])}
    s, j = pool(lib, 300, spec, 3)
    r = both(s, j)
    s.close()

    def check(w):
        x, y = w["scores"][10], w["scores"][290]
        assert x[:2] == y[:2] == (True, 3) and x[2] == y[2] > 0 and y[3] < x[3] == 1.0 and w["node"] == 290
    return [r], check


def _ideal(kind):
    def run(lib, oracle):
        N = 600
        spec = {5: TWIN, 300: TWIN, 599: (4, False, [])}
        if kind != "one":
            spec[520] = (4, False, [])
        s, j = pool(lib, N, spec, 3, id_rank=ranks("reversed" if kind == "two-reversed" else "index", N))
        r = both(s, j)
        s.close()

        def check(w):
            assert w["scores"][5] == w["scores"][300] and w["scores"][5][:2] == (True, 3)   # candidates before it, cheaper than nothing is
            assert w["scores"][599] == (True, 0, 0.0, 0.0) and (kind == "one" or w["scores"][520] == (True, 0, 0.0, 0.0))
            assert w["node"] == {"one": 599, "two": 520, "two-reversed": 599}[kind] and w["preempted"] == [] and w["cost"] == 0
        return [r], check
    return run


for _kind in ("one", "two", "two-reversed"):
    CASES[f"sel-ideal-{_kind}"] = _ideal(_kind)


@case("sel-threshold")
def _sel_threshold(lib, oracle):
    """improvement > minPct is strict: not selected at exactly (jobCost / cost) * 100 - 100, selected at the next smaller double"""
    N = 257
    s, j = pool(lib, N, {256: TWIN}, 3)
    free = both(s, j)
    job_cost = 3000 / (N - 1 + 4) / 1000     # the job's DRF share: its cpus over the pool's
    pct = (job_cost / free["cost"]) * 100 - 100
    at, below = both(s, j, min_improvement_pct=pct), both(s, j, min_improvement_pct=math.nextafter(pct, -math.inf))
    s.close()

    def check(w):
        assert w[0]["node"] == 256 and w[0]["cost"] > 0 and math.isfinite(pct)
        assert w[1]["node"] == -1 and w[1]["preempted"] == [] and w[1]["scores"] == w[0]["scores"]
        assert w[2] == w[0]
    return [free, at, below], check


def _cost0(shape, kind):
    def run(lib, oracle):
        """PREEMPT_CASES' "above fairshare" and "lower priority" shapes a hundredfold (the filler nodes must not move the fair shares), on three nodes"""
        on = {"above": [("B", 200, "pc2", 1000), ("B", 200, "pc2", 1001), ("B", 400, "pc2", 1002)], "lower": [("B", 200, "pc0", 1000), ("B", 200, "pc0", 1001)]}[shape]
        N = 300
        s, j = pool(lib, N, {n: (1000, False, on) for n in (5, 70, 260)}, {"above": 300, "lower": 800}[shape], id_rank=ranks(kind, N), queues=[QA, QB, QC])
        r = both(s, j, min_improvement_pct=1e300)
        s.close()

        def check(w):
            assert w["scores"][5] == w["scores"][70] == w["scores"][260] and w["scores"][5][:3] == (True, 1, 0.0) and w["scores"][5][3] > 0   # victims, cost 0: +Inf
            assert w["node"] == (5 if kind == "index" else 260) and len(w["preempted"]) == 1
        return [r], check
    return run


for _shape in ("above", "lower"):
    for _kind in ("index", "reversed"):
        CASES[f"sel-cost0-{_shape}-{_kind}"] = _cost0(_shape, _kind)


def _nothing(kind):
    def run(lib, oracle):
        spec = {"one-node": {}, "tainted": {1: (8, True, [])}, "tainted-late": {299: (8, True, [])}}[kind]
        s, j = pool(lib, {"one-node": 1, "tainted": 2, "tainted-late": 300}[kind], spec, 3)
        r = both(s, j)
        s.close()

        def check(w):
            assert w["node"] == -1 and w["cost"] == 0 and w["impact"] == 0 and w["preempted"] == [] and all(sc == NOT_SCHEDULED for sc in w["scores"])
        return [r], check
    return run


for _kind in ("one-node", "tainted", "tainted-late"):
    CASES[f"sel-nothing-{_kind}"] = _nothing(_kind)


def _fallback(big_wins):
    def run(lib, oracle):
        """node 2 holds 70 jobs, the others 64 and fewer; victims of pc0 cost nothing (priority preemptions), those of pc2 do.  Two queued jobs, the short form for
        both before anything else: the second call reuses the index the first built before it fell back"""
        cheap, dear = "pc0", "pc2"
        spec = {0: (64, False, [("BCD"[i % 3], 1, dear if big_wins else cheap, 1000 + i) for i in range(64)]),
                2: (70, False, [("BCD"[i % 3], 1, cheap if big_wins else dear, 1000 + (i * 37) % 499) for i in range(70)]),
                4: (5, False, [("B", 1, dear, 1000 + i) for i in range(5)])}
        s, j = pool(lib, 6, spec, 4, more_jobs=[("C", 3)], filler=(500, 0, True))   # (large tainted nodes nobody can use: every queue is below its fair share)
        kw = dict(min_improvement_pct=-1e9, now_ms=NOW)
        short = [s.optimiser_schedule_job(j, **kw), s.optimiser_schedule_job(j - 1, **kw)]
        long = [both(s, j), both(s, j - 1)]
        s.close()
        for a, b in zip(short, long):
            assert a == {k: b[k] for k in a}

        def check(w):
            for r, want in zip(w, (4, 3)):
                assert [sc[:2] for sc in r["scores"]] == [(True, want), (False, 0), (True, want), (False, 0), (True, want), (False, 0)]
                assert r["node"] == (2 if big_wins else 0) and r["cost"] == 0 and r["scores"][4][2] > 0 and r["scores"][0 if big_wins else 2][2] > 0
        return long, check
    return run


CASES["sel-fallback-big-wins"] = _fallback(True)
CASES["sel-fallback-big-loses"] = _fallback(False)


# ---------------------------------------------------------------- D. the index across state changes on one handle
def _two_nodes():
    jobs = [("BC"[i % 2], 1, 0, "pc2", 0, 1000 + i * 7 % 5) for i in range(6)] + [("CD"[i % 2], 1, 0, "pc2", 1, 1010 + i) for i in range(3)] + [("A", 6, 0, "pc2", -1, 0)]
    return [(8, 0, False), (8, 0, False)], jobs


@case("state-bind-unbind")
def _state_bind(lib, oracle):
    nodes, jobs = _two_nodes()
    s = build(lib, nodes, jobs, QS)
    first = s.optimiser_schedule_job(9, min_improvement_pct=-1e9, now_ms=NOW)
    v = first["preempted"][0]
    s.unbind(v, jobs[v][4])
    s.bind(v, 1 - jobs[v][4], 2)
    after = both(s, 9)
    s.close()

    def check(w):
        assert w[0]["node"] == 1 and len(w[0]["preempted"]) == 1 and jobs[v][4] == 1      # node 1 has 5 cpus free, the job wants 6
        assert w[1]["scores"] == [(True, 5) + w[1]["scores"][0][2:], (True, 0, 0.0, 0.0)] and w[1]["node"] == 1 and w[1]["preempted"] == []   # the victim moved: node 1 fits the job as it is
    return [first, after], check


def _prepare(s, jobs, queues):
    """round_prepare as build() calls it"""
    qn = [q for q, _ in queues]
    alloc = np.zeros((len(qn), len(PC_NAMES), 2), dtype=np.int64)
    for j in jobs:
        if j[4] >= 0:
            alloc[qn.index(j[0]), PC_NAMES.index(j[3])] += np.array([j[2], j[1] * 1000], dtype=np.int64)
    demand = np.tile(np.array([100000 * GI, 10000 * 1000], dtype=np.int64), (len(qn), 1))
    s.round_prepare([1.0 / pf for _, pf in queues], [[] for _ in qn], allocated_by_pc=alloc, demand=demand)


@case("state-jobs-patch")
def _state_patch(lib, oracle):
    """running jobs move between the nodes through jobs_patch; the oracle has no such entry and loads the patched table into a fresh handle"""
    nodes, jobs = _two_nodes()
    moved = {0: 1, 2: 1, 6: 0}     # job -> its new node
    patched = [j[:4] + (moved[i], 2000 + i) if i in moved else j for i, j in enumerate(jobs)]
    s = build(lib, nodes, jobs, QS)
    first = s.optimiser_schedule_job(9, min_improvement_pct=-1e9, now_ms=NOW)
    if oracle:
        s.close()
        s = build(lib, nodes, patched, QS)
    else:
        s.jobs_patch(list(moved), [moved[i] for i in moved], scheduled_at_priority=2, run_timestamp=[(2000 + i) * 1_000_000 for i in moved])
        _prepare(s, patched, QS)
    after = both(s, 9)
    s.close()

    def check(w):
        assert w[0]["node"] == 1 and w[0]["preempted"] != []
        assert [sc[:2] for sc in w[1]["scores"]] == [(True, 3), (True, 2)] and w[1]["node"] == 1    # 5 / 4 jobs on 8 cpus now
        assert any(v in moved and moved[v] == 1 for v in w[1]["preempted"])                        # a job the patch brought to the node is among its victims
    return [first, after], check


@case("state-scratch-growth")
def _state_growth(lib, oracle):
    """a small pool, then one with more nodes and jobs in the same process, then the small one again"""
    small, js = pool(lib, 3, {1: TWIN}, 3)
    a = both(small, js)
    large, jl = pool(lib, 700, {n: TWIN for n in (0, 255, 256, 699)}, 3, id_rank=ranks("rotated", 700, 256))
    b = both(large, jl)
    c = both(small, js)
    small.close()
    large.close()

    def check(w):
        assert w[0] == w[2] and w[0]["node"] == 1 and len(w[0]["scores"]) == 3
        assert w[1]["node"] == 256 and len({w[1]["scores"][n] for n in (0, 255, 256, 699)}) == 1 and sum(1 for sc in w[1]["scores"] if sc[0]) == 4
    return [a, b, c], check


# ---------------------------------------------------------------- the two tests of every case
_WANT = {}


def oracle_result(oracle_lib, name):
    """the oracle's result of a case, computed once and shared by the case's two tests"""
    if name not in _WANT:
        _WANT[name] = CASES[name](oracle_lib, True)
    return _WANT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_case_cpu_build(oracle_lib, hostsim_lib, name):
    want, check = oracle_result(oracle_lib, name)
    got, _ = CASES[name](hostsim_lib, False)
    assert got == want
    check(want[0] if len(want) == 1 else want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_case_gpu(oracle_lib, hip_lib, name):
    want, _ = oracle_result(oracle_lib, name)
    got, _ = CASES[name](hip_lib, False)
    assert got == want
