"""The literal batched first fit (armada_amd/csrc/kernels_fit_lit.h) at the edges of what only the device build does: the 64-wide classification window of flAdvance,
(events on lanes other than 0 and whole windows of "go on" need a one-type row whose yielded entries fail the fit: sections 1b and 3's storage pool), the 65-ary
flLowerBound, the bitonic network past one LDS tile (k_fit_lit_step), flFinish's segment ends at sizes with and without padding records, exactly LIT_TMAX node
types for a row, more queries than k_fit_lit's grid, and the refusal at LIT_TMAX + 1 types.  Every comparison is exact: against a closed form where the pool has one
(staircase pools) and against the CPU oracle always.  CPU tests run the CPU build of the device code (one lane); their `gpu` twins run the HIP library (one wave per query).

All pools of sections 1-3, 5 and 7 are built here: indexed cpu @1000, memory @128Mi, gpu @1, one priority class, nothing running, every request a distinct vector (so every
job is its own mask row) with cpu off the grid, which puts every row on the literal iteration path.

What the pools cannot reach: an entry below the request is a "go on" only if its new lower bound is not above the current one, and an entry that a search for the current
bound has reached never has such a bound (its key is at or above the bound's, so are its rounded quantities, and where they are equal the entry is not below the request).
With several node types every event of flAdvance is therefore on lane 0 of its window; only one-type rows, where a yielded entry that fails the fit is a "go on", have events
on other lanes."""
import numpy as np
import pytest

from armada_amd import workloads as W
from armada_amd.binding import SchedError

Mi = 1024 ** 2
UNIT = 128 * Mi
LIT_TMAX = 64   # armada_amd/csrc/dev.h


# ------------------------------------------------------------------------------------------------ pools
def _jobs_pool(name, node_total, q_req, T, rng, allocatable=None):
    n, m = len(node_total), len(q_req)
    none = np.zeros(0, np.int32)
    wl = W._assemble(name, W._config([(0, True)]), node_total, np.zeros((0, W.R), np.int64), none, none, none, none,
                     q_req, np.zeros(m, np.int32), np.zeros(m, np.int32), np.array([0]), np.ones(1), {})
    wl.node_allocatable = allocatable
    if T > 1:   # T node types through an indexed label, every one of them populated; node ids in another order than node indexes
        wl.config.indexed_label_keys = [3]
        lab = rng.permutation(np.arange(n) % T)
        assert len(np.unique(lab)) == T
        wl.node_labels = [[(3, int(v))] for v in lab]
        wl.node_id_rank = rng.permutation(n).astype(np.int32)
        wl.meta["labels"] = lab
    assert len(np.unique(wl.job_req, axis=0)) == m   # every job is its own mask row
    return wl


def _rank(order, n, rng):
    if order == "asc":
        return np.arange(n)
    if order == "desc":
        return np.arange(n)[::-1].copy()
    return rng.permutation(n)


def staircase(N, T=1, order="random", requests=None, behind=0):
    """node i: cpu 32000, memory (1 + rank[i]) * 128Mi.  Job k asks cpu 500 and memory k * 128Mi + 1: its answer is the node of rank k, none for k >= N — at every
    level (nothing runs) and for any number of node types (the merge pops by raw quantities, memory is distinct).  requests: memory asked per job, instead of N + 2 steps.
    behind = d > 0 (one node type): node i also has (1 + rank[i]) Mi of ephemeral storage, which is not indexed, and job k asks (k + d) Mi + 1 of it.  The iterator yields
    the entries of rank k, k + 1, ... and the d in front of rank k + d fail the fit: d "go on" classifications, then the answer, the node of rank k + d — none for k + d >= N."""
    rng = np.random.Generator(np.random.PCG64(9100 + 7 * N + T))
    rank = _rank(order, N, rng)
    node_total = np.zeros((N, W.R), np.int64)
    node_total[:, W.CPU] = 32000
    node_total[:, W.MEM] = (1 + rank) * UNIT
    mem = np.arange(N + 2, dtype=np.int64) * UNIT + 1 if requests is None else requests
    q_req = np.zeros((len(mem), W.R), np.int64)
    q_req[:, W.CPU] = 500
    q_req[:, W.MEM] = mem
    if behind:
        assert T == 1 and requests is None
        node_total[:, W.EPH] = (1 + rank) * Mi
        q_req[:, W.EPH] = (np.arange(N + 2) + behind) * Mi + 1
    wl = _jobs_pool(f"staircase{N}x{T}{order}{behind}", node_total, q_req, T, rng)
    by_rank = np.full(N + 1, -1, np.int32)
    by_rank[rank] = np.arange(N, dtype=np.int32)
    step = np.minimum((mem + UNIT - 1) // UNIT - 1 + behind, N)   # least rank whose memory (and ephemeral storage) holds the request
    wl.meta["closed_form"] = by_rank[step]
    return wl


ALIGNED, RAGGED, JAGGED, TIED, STORAGE = 0, 1, 2, 3, 4


def two_level(N, T, ragged=ALIGNED):
    """cpu (1 + rank % 8) * 4000, memory (1 + rank // 8) * 128Mi; requests cpu c * 4000 + 500, memory m * 128Mi + 1: the nodes of the cpu steps in front of the answer's have
    enough cpu and, up to some entry, too little memory — every such step is a seek.  RAGGED: allocatable below total by one odd amount of cpu and one of memory for the whole
    pool — off the grid, so the packed-key order is not the iteration order, and the answers stay spread over the pool like the aligned ones.  JAGGED: an odd amount per node,
    as workloads.small_random(ragged=True) draws them: the order by rounded quantities, the merge's order by raw ones and the order of the totals all differ; a cpu step then
    splits into five key values and the answers gather on the few nodes of each step that no node of a lower key value beats on memory, so these pools ask for a smaller spread (JAGGED_SPREAD).  TIED: aligned, and four nodes
    share every (cpu, memory) pair — with several node types the merge's heads then tie on the raw quantities and the node id decides, which is not the node index here.
    STORAGE (one node type): aligned; a node of cpu step s has (1 + s) Mi of ephemeral storage, which is not indexed, and a request also asks e Mi + 1 of it, e drawn like
    c.  In the cpu steps c .. e - 1 every entry with enough memory is yielded and fails the fit — runs of up to N / 8 "go on" classifications, whole windows of them — and
    the run ends on the first entry of the next step, which has too little memory: a seek from whichever lane that entry falls on."""
    rng = np.random.Generator(np.random.PCG64(9200 + 7 * N + T + 3 * ragged))
    rank = rng.permutation(N) // (4 if ragged == TIED else 1)
    node_total = np.zeros((N, W.R), np.int64)
    node_total[:, W.CPU] = (1 + rank % 8) * 4000
    node_total[:, W.MEM] = (1 + rank // 8) * UNIT
    pairs = np.unique(np.stack([rng.integers(0, 9, size=3000), rng.integers(0, N // 8 + 2, size=3000)], axis=1), axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    q_req = np.zeros((len(pairs), W.R), np.int64)
    q_req[:, W.CPU] = pairs[:, 0] * 4000 + 500
    q_req[:, W.MEM] = pairs[:, 1] * UNIT + 1
    if ragged == STORAGE:
        assert T == 1
        node_total[:, W.EPH] = (1 + rank % 8) * Mi
        q_req[:, W.EPH] = rng.integers(0, 9, size=len(pairs)) * Mi + 1
    alloc = None
    if ragged in (RAGGED, JAGGED):
        size = N if ragged == JAGGED else None
        below_cpu, below_mem = rng.integers(0, 24, size=size) * 137, rng.integers(0, 100, size=size) * 1000003
        assert np.all(below_cpu % 1000 != 0) or ragged == JAGGED   # (one amount for the pool: it must be off the grid)
        assert np.any(below_cpu % 1000 != 0) and np.any(below_mem % UNIT != 0)
        alloc = node_total.copy()
        alloc[:, W.CPU] -= below_cpu
        alloc[:, W.MEM] -= below_mem
        assert (alloc >= 0).all()
    return _jobs_pool(f"twolevel{N}x{T}{'arjts'[ragged]}", node_total, q_req, T, rng, allocatable=alloc)


def seeded_ragged(n, away=False):
    """8 node types with segments of roughly 90 to 260 entries, running jobs (the levels differ), selectors and tolerations"""
    return W.small_random(n_nodes=n, n_jobs=1500, n_queues=4, seed=8800 + n, occupied=0.8, gangs=0, ragged=True, away=away)


def many_requests():
    i = np.arange(66_000, dtype=np.int64)
    return staircase(64, requests=(i % 70) * UNIT + 1 + i // 70)


_POOLS = {}


def staircase_behind(N, d):
    return staircase(N, behind=d)


def _pool(key):
    """one pool per key for the whole session: the CPU tests, their GPU twins and the controls share it (nothing changes a workload after it is built)"""
    if key not in _POOLS:
        kind, args = key[0], key[1:]
        _POOLS[key] = {"staircase": staircase, "behind": staircase_behind, "two_level": two_level, "seeded": seeded_ragged, "many": many_requests}[kind](*args)
    return _POOLS[key]


# ------------------------------------------------------------------------------------------------ answers
def _queued(wl):
    return np.nonzero(wl.job_node < 0)[0].astype(np.int32)


def _prepared(lib, wl):
    s = W.load(lib, wl)
    W.prepare(s, wl)
    return s


def _all_priorities(s, jobs):
    return [s.fit_select_batch(jobs, p) for p in s.priorities]


_ORACLE = {}


def _oracle_answers(oracle_lib, key):
    if key not in _ORACLE:
        wl = _pool(key)
        _ORACLE[key] = _all_priorities(_prepared(oracle_lib, wl), _queued(wl))
    return _ORACLE[key]


def _same_as_oracle(lib, oracle_lib, key):
    """every queued job of the pool, at every level, against the oracle; returns (the answers, the oracle's)"""
    wl = _pool(key)
    want = _oracle_answers(oracle_lib, key)
    got = _all_priorities(_prepared(lib, wl), _queued(wl))
    assert len(got) == len(want) >= 2
    for p, (a, b) in enumerate(zip(got, want)):
        assert (a == b).all(), f"{key} level {p}: {int((a != b).sum())} of {len(a)} answers differ from the oracle, first at row {int(np.nonzero(a != b)[0][0])}"
    return got, want


def _outcome_mix(key, want, distinct_nodes, levels=None):
    """both outcomes occur at every level (of `levels`: where jobs run, the upper levels may place every job), and the pool's answers are spread over at least `distinct_nodes` nodes"""
    for p, b in enumerate(want[:levels]):
        assert (b >= 0).any() and (b < 0).any(), f"{key} level {p}: one outcome only"
    spread = len(np.unique(np.concatenate([b[b >= 0] for b in want])))
    assert spread >= distinct_nodes, f"{key}: {spread} distinct answered nodes"


# ------------------------------------------------------------------------------------------------ 1, 2. staircase pools: closed form and oracle
# one type: job k seeks from entry 0 and its lower bound lands on entry k of an N-entry segment — every position of segments of 1 .. 4225 = 65 * 65 entries (three probe
# rounds of the 65-ary search from 4097 on); the window is re-based on the target, so seek and yield are both on lane 0.  2047 / 2048 / 2049: one LDS tile with one, with no padding record, and the first size
# that runs k_fit_lit_step; 4096 / 4097: no padding at two tiles, and two global steps per merge level.  asc / desc / random: the network's direction bits
STAIRS = [(n, 1, "random") for n in (1, 2, 63, 64, 65, 66, 127, 128, 129, 2047, 2048, 2049, 4096, 4097, 4225)] + \
         [(n, 1, o) for n in (2048, 2049, 4097) for o in ("asc", "desc")] + \
         [(300, 3, "random"), (2049, 3, "random")]   # three types: segments of 100 and 683 entries, heads anywhere in them


def _staircase(lib, oracle_lib, N, T, order, behind=0):
    key = ("behind", N, behind) if behind else ("staircase", N, T, order)
    wl = _pool(key)
    got, want = _same_as_oracle(lib, oracle_lib, key)
    closed = wl.meta["closed_form"]
    found = max(N - behind, 0)
    assert len(closed) == N + 2 and (closed[:found] >= 0).all() and (closed[found:] < 0).all() and len(np.unique(closed)) == found + 1
    for p, a in enumerate(got):
        assert (a == closed).all(), f"{key} level {p}: {int((a != closed).sum())} of {len(a)} answers differ from the closed form, first at job {int(np.nonzero(a != closed)[0][0])}"
    for b in want:
        assert (b == closed).all()
    _outcome_mix(key, want, 1)


@pytest.mark.parametrize("N,T,order", STAIRS)
def test_staircase_hostsim(hostsim_lib, oracle_lib, N, T, order):
    _staircase(hostsim_lib, oracle_lib, N, T, order)


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,order", STAIRS)
def test_staircase_gpu(hip_lib, oracle_lib, N, T, order):
    _staircase(hip_lib, oracle_lib, N, T, order)


# ------------------------------------------------------------------------------------------------ 1b. staircase with the answer d entries behind the seek target
# job k's window is based on entry k; the entries k .. k + d - 1 are yielded and fail the fit ("go on"), entry k + d is the answer: the first event is on lane d for d < 64
# (1, 62, 63: ballot, ctz and `it.pos += first + 1` with first != 0), behind one whole "go on" window on lane 0 and lane 1 (64, 65: `it.pos += FL_NL`), behind two on lane 2
# (130); the jobs with k + d >= N run off the segment's end inside a window
BEHIND = [1, 62, 63, 64, 65, 130]


@pytest.mark.parametrize("d", BEHIND)
def test_staircase_answer_behind_hostsim(hostsim_lib, oracle_lib, d):
    _staircase(hostsim_lib, oracle_lib, 200, 1, "random", behind=d)


@pytest.mark.gpu
@pytest.mark.parametrize("d", BEHIND)
def test_staircase_answer_behind_gpu(hip_lib, oracle_lib, d):
    _staircase(hip_lib, oracle_lib, 200, 1, "random", behind=d)


# ------------------------------------------------------------------------------------------------ 3. two-level pools: seeks
# a request (c, m) walks the cpu steps c .. 7: the first entry of a step has enough cpu and too little memory — a seek (from lane 0: header) whose target, found by
# flLowerBound, is any entry of the step or the first of the next one.  (300, 3), (2049, 5): several types with segments longer than a wave; (4097, 64): every row matches
# exactly LIT_TMAX types, with segments of 64 and 65 entries; (1000, 1) storage: runs of 1 to 125 "go on" that end in a seek from the lane the run ends on
TWO_LEVEL = [(300, 3), (1000, 1), (2049, 5), (4097, 64)]
# distinct answered nodes asked of the jagged pools (two_level's docstring: no 100): three quarters of what the oracle's answers give — 52, 278, 196 and 190
JAGGED_SPREAD = {300: 39, 1000: 208, 2049: 147, 4097: 142}


def _two_level(lib, oracle_lib, N, T, ragged):
    key = ("two_level", N, T, ragged)
    wl = _pool(key)
    if T > 1:
        assert len(np.unique(wl.meta["labels"])) == T   # all T labels occur: T populated node types, and no selector keeps a row from any of them
        s = W.load(lib, wl)
        for job in (0, wl.num_jobs // 2, wl.num_jobs - 1):
            assert s.node_types_matching_job(job)[0] == T   # (exactly LIT_TMAX for the last pools)
    want = _same_as_oracle(lib, oracle_lib, key)[1]
    _outcome_mix(key, want, JAGGED_SPREAD[N] if ragged == JAGGED else 100)


TWO_LEVEL_CASES = [(n, t, r) for r in (ALIGNED, RAGGED, JAGGED) for n, t in TWO_LEVEL] + [(2049, 5, TIED), (4097, 64, TIED), (1000, 1, STORAGE)]
TWO_LEVEL_IDS = [f"{n}-{t}-{['aligned', 'ragged', 'jagged', 'tied', 'storage'][r]}" for n, t, r in TWO_LEVEL_CASES]


@pytest.mark.parametrize("N,T,ragged", TWO_LEVEL_CASES, ids=TWO_LEVEL_IDS)
def test_two_level_hostsim(hostsim_lib, oracle_lib, N, T, ragged):
    _two_level(hostsim_lib, oracle_lib, N, T, ragged)


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,ragged", TWO_LEVEL_CASES, ids=TWO_LEVEL_IDS)
def test_two_level_gpu(hip_lib, oracle_lib, N, T, ragged):
    _two_level(hip_lib, oracle_lib, N, T, ragged)


# ------------------------------------------------------------------------------------------------ 4. seeded ragged pools at size
def _seeded(lib, oracle_lib, n):
    key = ("seeded", n)
    want = _same_as_oracle(lib, oracle_lib, key)[1]
    assert len(want) == 5 and len(want[0]) == 1500
    assert any((a != b).any() for a, b in zip(want[:-1], want[1:]))   # jobs are running: the levels differ
    _outcome_mix(key, want, 100, levels=1)


@pytest.mark.parametrize("n", [700, 2100])
def test_seeded_ragged_hostsim(hostsim_lib, oracle_lib, n):
    _seeded(hostsim_lib, oracle_lib, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [700, 2100])
def test_seeded_ragged_gpu(hip_lib, oracle_lib, n):
    _seeded(hip_lib, oracle_lib, n)


# ------------------------------------------------------------------------------------------------ 5. more queries than k_fit_lit's grid of 65 536 waves
def _many_requests(lib, oracle_lib):
    key = ("many",)
    wl = _pool(key)
    got, want = _same_as_oracle(lib, oracle_lib, key)
    closed = wl.meta["closed_form"]
    assert len(closed) == 66_000 > 65_536 and len(np.unique(closed)) == 64 + 1
    i = np.arange(66_000)
    assert ((closed >= 0) == (i % 70 < 64)).all()
    for p, a in enumerate(got):
        assert (a == closed).all(), f"level {p}: {int((a != closed).sum())} answers differ from the closed form, first at job {int(np.nonzero(a != closed)[0][0])}"
    _outcome_mix(key, want, 64)


def test_more_queries_than_the_grid_hostsim(hostsim_lib, oracle_lib):
    _many_requests(hostsim_lib, oracle_lib)


@pytest.mark.gpu
def test_more_queries_than_the_grid_gpu(hip_lib, oracle_lib):
    _many_requests(hip_lib, oracle_lib)


# ------------------------------------------------------------------------------------------------ 6. the submit check on the same pools
# (pool, every unit must be counted as answered by the literal kernel)
SUBMIT_POOLS = [(("staircase", 65, 1, "random"), True), (("staircase", 2049, 1, "random"), True), (("two_level", 2049, 5, RAGGED), True), (("seeded", 2100, True), False)]


def _submit_check(lib, oracle_lib, key, all_literal, monkeypatch):
    wl = _pool(key)
    jobs = _queued(wl)[:1000]
    units, strip = [[int(j)] for j in jobs], [True] * len(jobs)
    s, o = W.load(lib, wl), W.load(oracle_lib, wl)   # pristine: nothing bound
    monkeypatch.delenv("ASCHED_SUBMIT_WIDE", raising=False)
    got, st = s.submit_check(units, strip), s.submit_stats()
    monkeypatch.setenv("ASCHED_SUBMIT_WIDE", "0")
    seq, st0 = s.submit_check(units, strip), s.submit_stats()
    monkeypatch.delenv("ASCHED_SUBMIT_WIDE", raising=False)
    want = o.submit_check(units, strip)
    assert got == want
    assert seq == want
    assert st0["sequential_units"] == len(units) and st0["literal_units"] == 0, st0
    assert st["sequential_units"] == 0 and st["wide_units"] == len(units), st
    assert any(r[0] for r in want)
    if all_literal:   # the literal kernel answered them: a change in how mask rows are classified cannot quietly hand this file's rows to the packed-key kernel
        assert st["literal_units"] == len(units), st
    else:
        assert 0 < st["literal_units"] <= len(units), st


@pytest.mark.parametrize("key,all_literal", SUBMIT_POOLS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_submit_check_hostsim(hostsim_lib, oracle_lib, key, all_literal, monkeypatch):
    _submit_check(hostsim_lib, oracle_lib, key, all_literal, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("key,all_literal", SUBMIT_POOLS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_submit_check_gpu(hip_lib, oracle_lib, key, all_literal, monkeypatch):
    _submit_check(hip_lib, oracle_lib, key, all_literal, monkeypatch)


# ------------------------------------------------------------------------------------------------ 7. LIT_TMAX + 1 node types are refused, LIT_TMAX are answered
def _refusal(lib, oracle_lib):
    wl = _pool(("two_level", 700, LIT_TMAX + 1, ALIGNED))
    assert len(np.unique(wl.meta["labels"])) == LIT_TMAX + 1
    with pytest.raises(SchedError) as e:   # (at upload: the masks are built once nodes and jobs are known)
        s = _prepared(lib, wl)
        s.fit_select_batch(_queued(wl), s.priorities[0])
    assert e.value.code == -2 and "LIT_TMAX" in str(e.value), (e.value.code, str(e.value))
    key = ("two_level", 700, LIT_TMAX, ALIGNED)
    assert len(np.unique(_pool(key).meta["labels"])) == LIT_TMAX
    _outcome_mix(key, _same_as_oracle(lib, oracle_lib, key)[1], 100)


def test_more_than_lit_tmax_types_refused_hostsim(hostsim_lib, oracle_lib):
    _refusal(hostsim_lib, oracle_lib)


@pytest.mark.gpu
def test_more_than_lit_tmax_types_refused_gpu(hip_lib, oracle_lib):
    _refusal(hip_lib, oracle_lib)


# ------------------------------------------------------------------------------------------------ negative control (CPU build): the packed-key argmin is NOT the answer on the ragged pools
CONTROL_POOLS = [("two_level", n, t, r) for r in (RAGGED, JAGGED) for n, t in TWO_LEVEL] + [("seeded", 700), ("seeded", 2100)]


@pytest.mark.parametrize("key", CONTROL_POOLS, ids=lambda v: "-".join(map(str, v)))
def test_packed_key_argmin_differs_on_the_ragged_pools(hostsim_lib, oracle_lib, key, monkeypatch):
    want = _oracle_answers(oracle_lib, key)
    monkeypatch.setenv("HOSTSIM_NO_LITERAL", "1")   # (read when the masks are built: every row takes k_fit_batch's question)
    wl = _pool(key)
    got = _all_priorities(_prepared(hostsim_lib, wl), _queued(wl))
    differ = sum(int((a != b).sum()) for a, b in zip(got, want))
    print(f"{key}: the packed-key argmin differs from the oracle in {differ} of {sum(len(b) for b in want)} answers")
    assert differ >= 1
