"""The oldest grid kernels at their edges: the batched first fit (kernels_fit.h k_fit_batch, armada_sched_wk.hip k_fit_batch_wk), the sorted base of the level-0 fast
structure (k_base_fill / k_bitonic_step / k_bitonic_tile / k_base_finish, launched by plat_hip.inc plat_build_base), the round-input builder's sums (k_agg), the
eviction sums (kernels_split.h k_evict_apply) and the grid stride of the bulk passes (k_bulk, k_bulk_wk).  In the CPU build (tests/hostsim) all of these are serial
loops over the per-element functions: none of the tiling, the wave reductions, the grouping by key, the sort network or the grid stride runs there.  So every case
runs twice: on the CPU build, which proves without a GPU that the case is what its name says and that the oracle agrees, and — marked gpu — on the HIP library, which
is the point.  Every comparison is with the ORACLE through the C ABI, bit for bit (scenario.assert_same_round for rounds, == for fit answers); every case asserts its
own coverage condition from the oracle's result and the input as constructed.  Pools are built by hand.

  group  what                                                     aims at
  A1     the only fitting node at 0, N-1, either side of every    k_fit_batch: `valid`, the lane / wave / tile a node falls into, waveMin64Dpp over a wave with one
         multiple of 64 and 256; N = 1 .. 769                      fitting lane, wmin[] with one live wave, tiles with no fitting node (m == ~0: no write)
  A2     2-4 fitting nodes in other waves / tiles, the smallest    the wmin[] loop; "look first, then atomicMin": a tile whose minimum does not improve the word, whichever tile
         key in the later (and, mirrored, the earlier) one         comes first
  A3     nothing fits (by resources; by the static mask)          the word stays ~0 -> -1
  A4     the minimum-key node is tainted, nodes 63 / 64            the shape mask's word boundary: `word = n >> 6, bit = n & 63`
  A5     full at the evicted priority, free above; all levels      the `level` plane of keys and alloc
  A6     ns = ysplit - 1, ysplit, ysplit + 1 distinct shapes       `per = ceil(ns / gridDim.y)`: y-blocks with an empty range (s0 >= s1)
  A7     A1-A5 under ASCHED_KEY_WORDS=2 (their [..-2] legs); equal high words in       k_fit_batch_wk: pass 0 (high word), pass 1 among `hi == out[i][0]` (the low word of ANOTHER high word
         two tiles; a lower low word under a larger high word      must not win)
  A8     fit_select_batch_global, nq = 255, 256, 257               the same kernel, then k_mgpu_pack: the `slot` indirection, MGPU_NO_NODE, host and device output buffers
  B      the base sort, N = 1 .. 16385; key order ascending,       k_bitonic_step alone (nb2 <= 4096, and the launch of 64 / 128 threads for nb2 = 64 / 128); 4096-key tiles
         descending, random by node id at 4097 and 8193            with padding (4097); one global step between tiles (8193); two (16385); the direction bit `(i & k) == 0`
  C      round_prepare without demand / allocated_by_pc            k_agg: the binary search of the queued walk, __ballot / __shfl grouping, waveSumSel, one atomic per key
  D      the evictor of phase 1 and of phase 3                     k_evict_apply: the same grouping for five sums and two counters; `if (!todo) continue`; gangOff
  E      M = 8 x CUs x 256 + 257 resident jobs                     the second trip of k_bulk / k_bulk_wk, k_agg, k_evict_apply (`rounds = 2`), work on both sides of the seam
"""
import copy
import math
import time

import numpy as np
import pytest

import scenario
from armada_amd import workloads as W
from armada_amd.binding import Config, SchedError
from armada_amd.workloads import CPU, GPU, MEM, Gi, Mi

FIT_TILE = 256       # kernels_fit.h:26 — nodes per workgroup of k_fit_batch
FIT_TILE_WK = 256    # armada_sched_wk.hip:60 — the same of k_fit_batch_wk
FIT_BLOCKS = 2048    # plat_hip.inc:700 — ysplit = min(ns, ceil(2048 / tiles))
SORT_TILE = 4096     # kernels_fit.h:73-74 — keys per workgroup of k_bitonic_tile; plat_hip.inc:654: step kernels alone up to this size
WG = 256             # plat_hip.inc:406-427 — threads per workgroup of k_bulk, k_agg, k_evict_apply; bulkGrid caps a launch at 8 x CUs of them
WAVE = 64
FIT_SHAPES = 200     # distinct request vectors of a sort case: below SMAX = 256 (dev.h:19)
NO_NODE = np.int64(2 ** 63 - 1)   # mgpu.h:23 MGPU_NO_NODE
PCS = ((0, True), (1, True), (3, False))
PC_PRIO = np.array([p for p, _ in PCS])


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def libs(request):
    """the library under test: the CPU build of the device code, or the HIP library"""
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


_ORACLE = {}


def _once(key, fn):
    """the oracle's answer for a case: computed once, shared by the CPU and the GPU leg, never changed"""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _workload(cfg, node_total, req, queue, pc, node, n_queues, *, run_ts=None, gang=None, weight=None):
    """a Workload from per-row arrays in any row order (W._assemble puts the running rows first): submit time = row, run timestamp = row unless given"""
    m = len(req)
    queue, pc, node = (np.asarray(x, np.int32).reshape(m) for x in (queue, pc, node))
    pcp = np.asarray(cfg.pc_priority)
    submit = np.arange(m, dtype=np.int64)
    rts = np.where(node >= 0, submit, 0) if run_ts is None else np.asarray(run_ts, np.int64)
    queued = W._sort_queued(queue, pcp[pc], submit, np.nonzero(node < 0)[0]) if m else []
    queued = [q for q in queued[:n_queues]] + [np.zeros(0, np.int32)] * max(0, n_queues - len(queued))
    g = np.full(m, -1, np.int32) if gang is None else np.asarray(gang, np.int32)
    card = np.array([max(1, int((g == x).sum())) if x >= 0 else 1 for x in g], np.int32).reshape(m)
    return W.Workload(name="edges", config=cfg, node_total=np.asarray(node_total, np.int64), job_req=np.asarray(req, np.int64).reshape(m, cfg.num_resources), job_queue=queue, job_pc=pc,
                      job_submit=submit, job_node=node, job_run_prio=np.where(node >= 0, pcp[pc], 0).astype(np.int32), job_run_ts=rts, job_gang=g, job_gang_card=card,
                      queue_weight=np.ones(n_queues) if weight is None else np.asarray(weight, np.float64), queued=queued)


def _run_order(wl):
    """dev.ordAll restated (asched_host.inc jobs_set, "pre-sorted job order"): by queue; running rows first; priority-class priority descending; run timestamp
    (running) or submit time; submit time; row"""
    active = wl.job_node >= 0
    pcp = np.asarray(wl.config.pc_priority)[wl.job_pc]
    rows = np.arange(wl.num_jobs)
    return np.lexsort((rows, wl.job_submit, np.where(active, wl.job_run_ts, wl.job_submit), -pcp, ~active, wl.job_queue))


def _waves(keys, active):
    """per wave of a walk: (active lanes, distinct keys among them)"""
    return [(int(active[i:i + WAVE].sum()), len(set(keys[i:i + WAVE][active[i:i + WAVE]].tolist()))) for i in range(0, len(keys), WAVE)]


# ================================================================================================ A. k_fit_batch / k_fit_batch_wk through fit_select_batch
NODE_TOTAL = np.array([256 * Gi, 32000, 1024 * Gi, 8], dtype=np.int64)   # memory, cpu, ephemeral storage, gpu


def _fit_pool(n, free, queries, *, run_pc=0, tainted=(), tolerant=()):
    """n nodes of NODE_TOTAL.  free: {node: (cpu cores, memory GiB, gpus)} left free by the node's one running job; every other node's job takes all of its cpu and
    nothing else — such a node carries the SMALLEST keys of the pool (cpu is the first key field) and fails on the resource test alone, not on the static mask.
    queries: [(cpu cores, memory GiB, gpus)], one queued job each, multiples of the index resolutions (1 core, 128Mi, 1): no shape is on the literal path.
    tainted: nodes with a NoSchedule taint; tolerant: indexes into queries whose jobs tolerate it.  -> (workload, job ids of the queries)"""
    fr = np.tile(np.array([256 * Gi, 0, 1024 * Gi, 8], dtype=np.int64), (n, 1))
    for node, (c, m, g) in free.items():
        fr[node] = [m * Gi, c * 1000, 1024 * Gi, g]
    run_req = NODE_TOTAL[None, :] - fr
    assert (run_req >= 0).all()
    keep = run_req.any(axis=1)
    nr = int(keep.sum())
    rpc = np.broadcast_to(np.asarray(run_pc, np.int32), (n,))[keep]
    q_req = np.array([[m * Gi, c * 1000, 0, g] for c, m, g in queries], dtype=np.int64).reshape(len(queries), W.R)
    none = np.zeros(len(queries), np.int32)
    wl = W._assemble("fit-edges", W._config(list(PCS)), np.tile(NODE_TOTAL, (n, 1)), run_req[keep], np.nonzero(keep)[0].astype(np.int32), np.zeros(nr, np.int32), rpc,
                     PC_PRIO[rpc].astype(np.int32), q_req, none, none, PC_PRIO, np.ones(1), {})
    if len(tainted):
        wl.node_taints = [[(9, 1, 1)] if i in set(tainted) else [] for i in range(n)]       # (key, value, NoSchedule)
        wl.class_tolerations, wl.class_selectors = [[], [(9, 1, 0, 0)]], [[], []]             # class 1: Exists on key 9
        wl.job_req_class = np.zeros(wl.num_jobs, np.int32)
        wl.job_req_class[nr + np.asarray(sorted(tolerant), int)] = 1
    return wl, np.arange(nr, nr + len(queries), dtype=np.int32)


def _prepared(lib, wl):
    s = W.load(lib, wl)
    W.prepare(s, wl)   # the running jobs are bound
    return s


def _on_the_packed_key_path(lib, wl, jobs):
    """which path answers these jobs, the way test_z_fit_literal.py asserts it: every request on the index grid, and the submit check — which takes the same decision
    per mask row — counts no unit with a literal row and leaves none to the sequential path"""
    cfg = wl.config
    for col, res in zip(cfg.indexed_col, cfg.indexed_resolution):
        assert (wl.job_req[:, col] % res == 0).all()
    s = W.load(lib, wl)
    s.submit_check([[int(j)] for j in jobs], [True] * len(jobs))
    st = s.submit_stats()
    s.close()
    assert st["literal_units"] == 0 and st["sequential_units"] == 0 and st["wide_units"] == len(jobs), st


def _two_word_fields(n):
    """layoutKeys restated for NODE_TOTAL under ASCHED_KEY_WORDS=2: [(first bit, width)] of the cpu, memory and gpu field of the 128-bit key; the rank is below"""
    cfg = W._config(list(PCS))
    widths = [(int(NODE_TOTAL[c]) // r + 2).bit_length() for c, r in zip(cfg.indexed_col, cfg.indexed_resolution)]   # bitsFor(maxq + 1 - (-1))
    idx = max(1, (max(n - 1, 1)).bit_length())
    shift = max(idx, 64 - sum(widths) // 2)   # the fields are moved up so that they lie across the word boundary
    out = []
    for w in reversed(widths):
        out.append((shift, w)); shift += w
    return out[::-1]


def _fit_answers(lib, wl, jobs, prios=None, single=False, words=None):
    """fit_select_batch at every priority of the config (or `prios`): one call for all jobs, or (single) one call per job.  words == 2: the handle must be on a
    two-word key (it says so when asked for the one-word exchange of fit_select_batch_global)"""
    s = _prepared(lib, wl)
    if words == 2:
        buf = np.empty(len(jobs), dtype=np.int64)
        with pytest.raises(SchedError) as e:
            s.fit_select_batch_global(jobs, 0, [1] * s.K, 1, buf.ctypes.data)
        assert e.value.code == -2 and "two words" in str(e.value)
    out = []
    for p in (s.priorities if prios is None else prios):
        out.append(np.concatenate([s.fit_select_batch(jobs[i:i + 1], p) for i in range(len(jobs))]) if single else s.fit_select_batch(jobs, p))
    s.close()
    return out


def _positions(n):
    """0, N-1 and either side of every multiple of 64 (so of 256 too) below N"""
    pos = {0, n - 1}
    for m in range(WAVE, n, WAVE):
        pos |= {m - 1, m}
    return sorted(pos)


def _only_node_pool(n):
    """every position of _positions(n) holds the ONLY node that fits one query: the free (cpu, memory) pairs form an antichain — cpu rising while memory falls — handed
    to the positions in a scrambled order, so that the key order (cpu first) is not the node order"""
    pos = _positions(n)
    k = len(pos)
    assert k <= 30
    perm = [(i * 7 + 3) % k for i in range(k)] if k > 1 else [0]
    assert sorted(perm) == list(range(k))
    free = {p: (perm[i] + 1, k - perm[i], 0) for i, p in enumerate(pos)}
    queries = [free[p] for p in pos]
    wl, jobs = _fit_pool(n, free, queries)
    return wl, jobs, np.array(pos, np.int32)


FIT_N = [1, 63, 64, 65, 255, 256, 257, 511, 513, 769]
WORDS = [1, 2]


def _set_words(monkeypatch, words):
    if words == 2:
        monkeypatch.setenv("ASCHED_KEY_WORDS", "2")   # read by layoutKeys at nodes_upsert / jobs_set: the handle is served by k_fit_batch_wk
    else:
        monkeypatch.delenv("ASCHED_KEY_WORDS", raising=False)


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("n", FIT_N)
def test_a1_the_only_fitting_node(libs, oracle_lib, monkeypatch, n, words):
    wl, jobs, pos = _only_node_pool(n)
    want = _once(("a1", n), lambda: _fit_answers(oracle_lib, wl, jobs))
    # the case is what it says: at the two lowest levels (evicted, priority 0) every query has exactly one fitting node, the intended one
    al = NODE_TOTAL[None, :] - np.array([wl.job_req[wl.job_node == i].sum(axis=0) for i in range(n)]).reshape(n, W.R)
    for j, p in zip(jobs, pos):
        assert np.nonzero((al >= wl.job_req[j]).all(axis=1))[0].tolist() == [int(p)]
    assert all((w == pos).all() for w in want[:3])                    # levels: evicted (-2), -1, 0
    _set_words(monkeypatch, words)
    _on_the_packed_key_path(libs, wl, jobs)
    got = _fit_answers(libs, wl, jobs, words=words)                                  # all positions' shapes at once, every level
    for a, b in zip(got, want):
        assert (a == b).all(), (n, a, b)
    one = _fit_answers(libs, wl, jobs, prios=[0], single=True)[0]      # one shape per call
    assert (one == want[2]).all(), (n, one, want[2])


def _chain(n, free):
    """queries of 1 .. 31 cores against nodes with `free` = {node: cores} (same memory, no gpu): the answer to c cores is the node with the fewest free cores >= c,
    the lowest node among equals"""
    wl, jobs = _fit_pool(n, {k: (c, 64, 0) for k, c in free.items()}, [(c, 1, 0) for c in range(1, 32)])
    intended = []
    for c in range(1, 32):
        fit = sorted((v, k) for k, v in free.items() if v >= c)
        intended.append(fit[0][1] if fit else -1)
    return wl, jobs, np.array(intended, np.int32)


MINIMA = {
    # the smallest key in the LATER wave of one tile (waves 0, 1, 3, 3)
    "later-wave": (600, {10: 8, 70: 6, 200: 4, 250: 3}),
    # ... in the later tile (tiles 0, 1, 2, 2)
    "later-tile": (600, {10: 8, 300: 6, 520: 4, 599: 3}),
    # mirrored: the first wave / tile holds the minimum, every later tile's minimum does not improve the word
    "earlier-wave": (600, {10: 3, 70: 4, 200: 6, 250: 8}),
    "earlier-tile": (600, {10: 3, 300: 4, 520: 6, 599: 8}),
    # equal fields in three tiles: the rank in the low bits decides; and a fuller node behind them
    "equal-fields": (600, {100: 5, 400: 5, 580: 5, 590: 2}),
    # wave and tile edges on both sides
    "edges": (769, {63: 9, 64: 7, 255: 5, 256: 4, 767: 3, 768: 2}),
}


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("name", list(MINIMA))
def test_a2_minimum_across_waves_and_tiles(libs, oracle_lib, monkeypatch, name, words):
    n, free = MINIMA[name]
    wl, jobs, intended = _chain(n, free)
    want = _once(("a2", name), lambda: _fit_answers(oracle_lib, wl, jobs))
    assert all((w == intended).all() for w in want[:3])
    assert len({k // WAVE for k in free}) >= 3 and len(set(intended.tolist()) - {-1}) >= 2 and -1 in intended   # A3 too: more cores than any node has free
    _set_words(monkeypatch, words)
    _on_the_packed_key_path(libs, wl, jobs)
    for a, b in zip(_fit_answers(libs, wl, jobs, words=words), want):
        assert (a == b).all(), (name, a, b)
    one = _fit_answers(libs, wl, jobs, prios=[0], single=True)[0]
    assert (one == want[2]).all()


@pytest.mark.parametrize("words", WORDS)
def test_a3_nothing_fits(libs, oracle_lib, monkeypatch, words):
    """31 cores: no node has them free (the resource test); 33 cores, 300 GiB: no node has them at all (the static mask); on a pool of 3 tiles"""
    wl, jobs = _fit_pool(700, {5: (30, 64, 0), 300: (30, 64, 0), 699: (30, 64, 0)}, [(31, 1, 0), (33, 1, 0), (1, 300, 0), (30, 64, 0)])
    want = _once("a3", lambda: _fit_answers(oracle_lib, wl, jobs))
    assert all(w.tolist() == [-1, -1, -1, 5] for w in want[:3])
    assert want[-1].tolist() == [0, -1, -1, 0]                          # (above the running jobs' priority every node is empty: 31 cores fit, on node 0)
    _set_words(monkeypatch, words)
    for a, b in zip(_fit_answers(libs, wl, jobs, words=words), want):
        assert (a == b).all(), (a, b)


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("masked", [63, 64])
def test_a4_minimum_key_node_is_masked_out(libs, oracle_lib, monkeypatch, masked, words):
    """nodes 63 and 64 are the last bit of one word of the shape mask and the first of the next: the tainted one has the smaller key and fits by resources"""
    other = 127 - masked
    wl, jobs = _fit_pool(130, {masked: (2, 64, 0), other: (3, 64, 0), 5: (8, 64, 0), 100: (6, 64, 0)}, [(1, 1, 0), (1, 1, 0), (3, 1, 0), (3, 1, 0)], tainted=[masked], tolerant=[1, 3])
    want = _once(("a4", masked), lambda: _fit_answers(oracle_lib, wl, jobs))
    assert all(w.tolist() == [other, masked, other, other] for w in want[:3])
    _set_words(monkeypatch, words)
    _on_the_packed_key_path(libs, wl, jobs)
    for a, b in zip(_fit_answers(libs, wl, jobs, words=words), want):
        assert (a == b).all(), (a, b)


@pytest.mark.parametrize("words", WORDS)
def test_a5_levels(libs, oracle_lib, monkeypatch, words):
    """the running job of node n has class n % 3 (priorities 0, 1, 3): a node is full at every level up to its job's priority and empty above.  Nodes 71 and 299
    (class 2: not preemptible, priority 3) have 4 / 2 cores free at every level"""
    n = 520
    run_pc = np.arange(n) % 3
    wl, jobs = _fit_pool(n, {71: (4, 64, 0), 299: (2, 64, 0)}, [(1, 1, 0), (3, 1, 0), (5, 1, 0), (32, 1, 0)], run_pc=run_pc)
    assert run_pc[71] == run_pc[299] == 2
    want = _once("a5", lambda: _fit_answers(oracle_lib, wl, jobs))
    s = _prepared(oracle_lib, wl)
    assert s.priorities == [-2, -1, 0, 1, 3], s.priorities         # the evicted priority, the one below every class, the classes'
    s.close()
    first = {1: int(np.nonzero(run_pc == 0)[0][0]), 3: int(np.nonzero(run_pc <= 1)[0][0])}
    assert all(w.tolist() == [299, 71, -1, -1] for w in want[:3])
    # at priority 1 the nodes of class-0 jobs are empty: 32 cores fit there, on the first of them; fewer cores still take the fullest node they fit on
    assert want[3].tolist() == [299, 71, first[1], first[1]] and want[4].tolist() == [299, 71, first[3], first[3]]
    _set_words(monkeypatch, words)
    for a, b in zip(_fit_answers(libs, wl, jobs, words=words), want):
        assert (a == b).all(), (a, b)


def _ysplit_pool(n, ns):
    """node i has (i % 32 + 1) cores and (i // 32 % 8 + 1) * 8 GiB free (beyond 256 nodes the pairs repeat: the lowest node wins); ns distinct shapes of 1 .. 32 cores
    and 1 .. 79 GiB, drawn evenly from all 2 528.  A shape's expected node is the lowest one with exactly its cores and the least memory that holds it; above 64 GiB
    nothing fits"""
    free = {i: (i % 32 + 1, (i // 32 % 8 + 1) * 8, 0) for i in range(n)}
    every = [(c, m) for m in range(1, 80) for c in range(1, 33)]
    shapes = [every[i * len(every) // ns] for i in range(ns)]
    wl, jobs = _fit_pool(n, free, [(c, 1, 0) for c, _ in shapes])
    wl.job_req[jobs, MEM] = np.array([m for _, m in shapes], np.int64) * Gi     # 1 .. 79 GiB: above 64 GiB nothing fits
    return wl, jobs


@pytest.mark.parametrize("n,ns", [(256, 2047), (256, 2048), (256, 2049), (200, 2049), (1000, 511), (1000, 512), (1000, 513), (769, 513)])
def test_a6_y_split(libs, oracle_lib, n, ns):
    tiles = (n + FIT_TILE - 1) // FIT_TILE
    ysplit = min(ns, (FIT_BLOCKS + tiles - 1) // tiles)
    per = (ns + ysplit - 1) // ysplit
    assert ysplit in (ns - 1, ns, ns + 1) or ns < ysplit
    wl, jobs = _ysplit_pool(n, ns)
    assert len(np.unique(wl.job_req[jobs], axis=0)) == ns               # the call dedups by shape: this many reach the kernel
    if ns == ysplit + 1:
        assert per == 2 and (ysplit - 1) * per >= ns                    # the upper y-blocks start behind the list
    want = _once(("a6", n, ns), lambda: _fit_answers(oracle_lib, wl, jobs, prios=[-2, 0]))
    for w in want:
        assert len(set(w.tolist())) >= 100 and (w == -1).any(), len(set(w.tolist()))   # the answers are spread over a hundred nodes and more, and some shapes fit nowhere
    for a, b in zip(_fit_answers(libs, wl, jobs, prios=[-2, 0]), want):
        assert (a == b).all(), (n, ns, int((a != b).sum()))


TWO_WORD = {
    # equal cpu and memory in two tiles — equal high words —, the later node has fewer gpus free: the low word decides
    "equal-high-words": ({50: (4, 64, 4), 300: (4, 64, 1)}, [(1, 1, 1), (1, 1, 2)], [300, 50]),
    # the later tile's node has the lower low word (no gpu left but the one asked for) under a larger high word (more cores free): it must not win
    "lower-low-word-under-larger-high-word": ({50: (2, 64, 4), 300: (8, 64, 1)}, [(1, 1, 1), (3, 1, 1)], [50, 300]),
    "lower-low-word-in-the-earlier-tile": ({50: (8, 64, 1), 300: (2, 64, 4), 599: (2, 64, 5)}, [(1, 1, 1), (3, 1, 1), (1, 1, 5)], [300, 50, 599]),
}


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("name", list(TWO_WORD))
def test_a7_two_word_minimum(libs, oracle_lib, monkeypatch, name, words):
    free, queries, intended = TWO_WORD[name]
    n = 600
    wl, jobs = _fit_pool(n, free, queries)
    (cpu0, cpuw), (mem0, memw), (gpu0, gpuw) = _two_word_fields(n)
    assert gpu0 + gpuw <= 64 <= cpu0 and mem0 < 64 < mem0 + memw          # cpu lies in the high word, gpu in the low word, memory (equal in every node) across both
    want = _once(("a7", name), lambda: _fit_answers(oracle_lib, wl, jobs))
    assert all(w.tolist() == intended for w in want[:3])
    _set_words(monkeypatch, words)
    _on_the_packed_key_path(libs, wl, jobs)
    for a, b in zip(_fit_answers(libs, wl, jobs, words=words), want):
        assert (a == b).all(), (name, a, b)


def _layout(wl):
    cfg = wl.config
    width = [max(1, int(int(wl.node_total[:, c].max(initial=0)) // int(r) + 1).bit_length()) for c, r in zip(cfg.indexed_col, cfg.indexed_resolution)]
    return width, max(1, int(wl.num_nodes - 1).bit_length())


def _global_words(lib, wl, jobs, use_cuda):
    s = _prepared(lib, wl)
    width, bits = _layout(wl)
    out = []
    for prio in (-2, 3):
        if use_cuda:
            import torch
            t = torch.empty(len(jobs), dtype=torch.int64, device="cuda")
            s.fit_select_batch_global(jobs, prio, width, bits + 4, t.data_ptr(), rank_offset=4321 % (1 << 3))
            words = t.cpu().numpy()
        else:
            words = np.empty(len(jobs), dtype=np.int64)
            s.fit_select_batch_global(jobs, prio, width, bits + 4, words.ctypes.data, rank_offset=4321 % (1 << 3))
        out.append((words, s.fit_select_batch(jobs, prio)))
    s.close()
    return out, bits + 4


@pytest.mark.parametrize("nq", [255, 256, 257])
def test_a8_global_words(libs, oracle_lib, request, nq):
    """nq queries that repeat 5 shapes (k_mgpu_pack reads the kernel's word through `slot`), one of which fits nowhere below the running jobs' priority"""
    n, free = MINIMA["later-tile"]
    shapes = [(1, 1, 0), (4, 1, 0), (31, 1, 0), (5, 1, 0), (7, 1, 0)]
    wl, jobs = _fit_pool(n, {k: (c, 64, 0) for k, c in free.items()}, [shapes[(i * 3) % 5] for i in range(nq)])
    assert len(np.unique(wl.job_req[jobs], axis=0)) == 5
    want, rb = _once(("a8", nq), lambda: _global_words(oracle_lib, wl, jobs, False))
    assert (want[0][0] == NO_NODE).sum() == sum(1 for i in range(nq) if (i * 3) % 5 == 2) > 0 and not (want[1][0] == NO_NODE).any()
    on_gpu = request.node.callspec.params["libs"] == "hip"
    for use_cuda in ([False, True] if on_gpu else [False]):              # host memory (staged) and a tensor on the handle's GPU (written in place)
        got, _ = _global_words(libs, wl, jobs, use_cuda)
        for (gw, gp), (ww, wp) in zip(got, want):
            assert (gw == ww).all() and (gp == wp).all()
            node = np.where(gw == NO_NODE, -1, (gw & ((1 << rb) - 1)) - 4321 % (1 << 3)).astype(np.int32)
            assert (node == gp).all()


# ================================================================================================ B. the base sort through round_prepare + one round
SORT_N = [(1, "random"), (2, "random"), (63, "random"), (64, "random"), (65, "random"), (127, "random"), (128, "random"), (129, "random"), (2049, "random"),
          (4095, "random"), (4096, "random"), (4097, "ascending"), (4097, "descending"), (4097, "random"), (8191, "random"), (8193, "ascending"), (8193, "descending"),
          (8193, "random"), (16385, "random")]


def _sort_pool(n, order, swap=None):
    """n empty nodes of 32 cores whose memory is (rank + 1) x 128Mi for a permutation `rank` of 0 .. n-1: every node has a free amount of its own and `rank` IS its
    place in the sorted base (cpu equal, memory the next key field).  Up to 1400 queued jobs of 32 cores — a whole node each — ask for the memory of at most 200 ranks spread
    evenly over 0 .. n-1, up to 7 jobs each (more than SMAX = 256 fit shapes and the handle builds no fast structure, dev.h:19): best fit puts each on the smallest
    unused node that holds it, all over the sorted order.
    swap: two nodes whose ranks are exchanged (the negative control)"""
    rng = np.random.default_rng(n)
    rank = {"ascending": np.arange(n), "descending": np.arange(n)[::-1].copy(), "random": rng.permutation(n)}[order]
    if swap:
        rank = rank.copy(); rank[list(swap)] = rank[list(swap)[::-1]]
    total = np.tile(np.array([0, 32000, 1024 * Gi, 0], dtype=np.int64), (n, 1))
    total[:, MEM] = (rank + 1) * 128 * Mi
    target = np.unique(np.linspace(0, n - 1, min(n, FIT_SHAPES)).astype(np.int64))
    target = rng.permutation(np.repeat(target, min(7, -(-n // len(target)))))
    j = len(target)
    req = np.zeros((j, W.R), np.int64)
    req[:, CPU], req[:, MEM] = 32000, (target + 1) * 128 * Mi
    wl = _workload(W._config(list(PCS)), total, req, np.arange(j) % 3, np.zeros(j, int), np.full(j, -1), 3)
    return wl, rank


def _sort_round(lib, wl):
    s = _prepared(lib, wl)
    res = s.schedule_round()
    st = s.round_stats()
    s.close()
    return res, st


@pytest.mark.parametrize("n,order", SORT_N)
def test_b_base_sort(libs, oracle_lib, n, order):
    wl, rank = _sort_pool(n, order)
    assert len(np.unique(wl.node_total[:, MEM])) == n
    want, _ = _once(("b", n, order), lambda: _sort_round(oracle_lib, wl))
    # coverage: the picks fall into every 4096-block of the sorted order, the first and the last included
    picked = rank[sorted(set(want.scheduled.values()))]
    assert set((picked // SORT_TILE).tolist()) == set(range((n - 1) // SORT_TILE + 1)), sorted(set((picked // SORT_TILE).tolist()))
    assert len(want.scheduled) >= max(1, min(n, wl.num_jobs) * 9 // 10)
    got, st = _sort_round(libs, wl)
    scenario.assert_same_round(want, got)
    # the handle built the fast structure (the sorted base) and the round ran on it
    assert st["fast_iterations"] >= len(want.scheduled) and st["generic_iterations"] <= 8 and st["l0_overflows"] == 0, st


def test_b_the_comparison_sees_the_order(oracle_lib):
    """negative control: the same round with the order ranks of two nodes exchanged is a different round"""
    n = 129
    wl, rank = _sort_pool(n, "random")
    want, _ = _once(("b", n, "random"), lambda: _sort_round(oracle_lib, wl))
    a, b = [int(x) for x in sorted(set(want.scheduled.values()))[:2]]
    other, _ = _sort_round(oracle_lib, _sort_pool(n, "random", swap=(a, b))[0])
    with pytest.raises(AssertionError):
        scenario.assert_same_round(want, other)
    assert sorted(other.scheduled.values()) == sorted(want.scheduled.values()) and other.scheduled != want.scheduled   # the same nodes, taken by other jobs


# ================================================================================================ C. k_agg through round_prepare without demand / allocated_by_pc
def _agg_config(r):
    """r = 1: the smallest job table the config allows (one column, indexed); 4: W's; 8 = MAXR (dev.h:12): five columns that are not indexed"""
    if r == W.R:
        return W._config(list(PCS))
    idx = [0] if r == 1 else [CPU, MEM, GPU]
    res = [1000] if r == 1 else [1000, 128 * Mi, 1]
    return Config(num_resources=r, indexed_col=idx, indexed_resolution=res, pc_priority=[p for p, _ in PCS], pc_preemptible=[int(x) for _, x in PCS],
                  drf_multiplier=[1.0] * r, prefer_large_job_ordering=True, protected_fraction_of_fair_share=0.0)


def _agg_pool(segments, n_queues, r=W.R, n_nodes=8):
    """segments: [(queue, class, running rows, queued rows)], rows in this order.  Every column holds a permutation of 1 .. M times the column's unit — distinct
    values in every resource column — and every other row asks for 1 TiB of memory more (a 32-bit sum or a 32-bit request shows; column 2 is in units of 3e9).  The
    pool is twice what all rows ask for: every queue's demand-capped share is its own demand"""
    queue, pc, run = [], [], []
    for q, p, nr, nq in segments:
        queue += [q] * (nr + nq); pc += [p] * (nr + nq); run += [True] * nr + [False] * nq
    m = len(queue)
    rng = np.random.default_rng(m * 31 + n_queues)
    cfg = _agg_config(r)
    unit = np.ones(r, np.int64)
    for c, res in zip(cfg.indexed_col, cfg.indexed_resolution):
        unit[c] = res
    for c in range(r):
        if c not in cfg.indexed_col:
            unit[c] = 3_000_000_017 + c
    req = np.stack([(rng.permutation(m) + 1) * unit[c] for c in range(r)], axis=1).astype(np.int64).reshape(m, r)
    req[::2, MEM if r > 1 else 0] += 8192 * 128 * Mi if r > 1 else (2 ** 41 // 1000 + 1) * 1000
    run = np.array(run, bool)
    node = np.where(run, np.arange(m) % n_nodes, -1)
    res_of = np.array([dict(zip(cfg.indexed_col, cfg.indexed_resolution)).get(c, 1) for c in range(r)], np.int64)
    per_node = ((2 * req.sum(axis=0) // n_nodes + (req.max(axis=0) if m else 0)) // res_of + 1) * res_of if m else res_of * 8
    wl = _workload(cfg, np.tile(per_node, (n_nodes, 1)), req, queue, pc, node, n_queues, weight=1.0 + np.arange(n_queues) % 3)
    return wl


def _agg_fractions(wl, cordoned):
    """per-queue, per-class limit fractions that make a sum booked under the wrong class of the right queue show in the capped demand: class 0 unlimited, class 1
    capped at about half of what the queue asks for in it, class 2 just above what it asks for (anything added there is cut off, anything taken away is missed)"""
    by_pc, _ = _aggregates(wl, cordoned, None)
    total = wl.node_total.sum(axis=0).astype(np.float64)
    q, npc, r = by_pc.shape
    frac = np.full((q, npc, r), math.inf)
    frac[:, 1, :] = np.maximum(by_pc[:, 1, :], 1) * 0.5 / total
    frac[:, 2, :] = (by_pc[:, 2, :] + 1) * 1.001 / total
    return frac


def _aggregates(wl, cordoned, frac):
    """calculateJobSchedulingInfo / constructSchedulingContext in numpy (the scheme of test_z_round_input_builder.py): frac None -> (requests by queue and class,
    allocation by queue and class); else -> (capped demand by queue, allocation by queue and class)"""
    q, npc, r = wl.num_queues, len(wl.config.pc_priority), wl.config.num_resources
    by_pc, alloc = np.zeros((q, npc, r), np.int64), np.zeros((q, npc, r), np.int64)
    running = wl.job_node >= 0
    counted = running | ~np.asarray(cordoned, bool)[wl.job_queue] if wl.num_jobs else running
    np.add.at(by_pc, (wl.job_queue[counted], wl.job_pc[counted]), wl.job_req[counted])
    np.add.at(alloc, (wl.job_queue[running], wl.job_pc[running]), wl.job_req[running])
    if frac is None:
        return by_pc, alloc
    total = wl.node_total.sum(axis=0)
    limit = np.zeros_like(by_pc)
    for i in np.ndindex(*by_pc.shape):
        f = frac[i]
        limit[i] = 2 ** 63 - 1 if math.isinf(f) else (int(total[i[2]]) if f == 1.0 else int(float(total[i[2]]) * f))   # multiplyResource
    return np.minimum(by_pc, limit).sum(axis=1), alloc


def _agg_round(lib, wl, cordoned, frac, explicit, demand=None):
    s = W.load(lib, wl)
    kw = {}
    if explicit:
        dm, al = _aggregates(wl, cordoned, frac)
        kw = dict(demand=dm if demand is None else demand, allocated_by_pc=al)
    s.round_prepare(wl.queue_weight, wl.queued, cordoned=cordoned, pc_resource_limit_fraction=frac, **kw)
    res = s.schedule_round()
    s.close()
    return res


def _three(n, run):
    """n rows over 3 queues x 3 classes in uneven runs"""
    seg, left, i = [], n, 0
    while left:
        k = min(left, 1 + (i * 7) % 23)
        seg.append((min(2, i * 3 // max(1, -(-n // 12))), i % 3, k if run else 0, 0 if run else k))
        left -= k; i += 1
    seg.sort(key=lambda x: x[0])
    return seg


AGG = {}
for _n in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
    AGG[f"running-{_n}"] = dict(segments=_three(_n, True), q=3)       # the run-order walk has this length and every lane of it is active; the queued walk is empty
    AGG[f"queued-{_n}"] = dict(segments=_three(_n, False), q=3)       # the queued walk has this length; the run-order walk too, with no active lane
AGG.update({
    "one-key-per-wave": dict(segments=[(0, 1, 130, 130)], q=1),
    "64-queues-in-a-wave": dict(segments=[(q, q % 3, 1, 1) for q in range(64)], q=64),
    "22-queues-x-3-classes": dict(segments=[(q, p, 1, 1) for q in range(22) for p in range(3)], q=22),
    "64-queues-running": dict(segments=[(q, q % 3, 1, 0) for q in range(64)], q=64),
    "22-queues-x-3-classes-running": dict(segments=[(q, p, 1, 0) for q in range(22) for p in range(3)], q=22),
    # queue 1's run starts at lane 30 of wave 0 and ends in wave 2, in both walks
    "run-from-mid-wave-over-three-waves": dict(segments=[(0, 0, 30, 30), (1, 1, 150, 150), (2, 2, 20, 20)], q=3),
    # inactive lanes between active ones: the queued rows of a queue lie between its running rows and the next queue's (run-order walk); queue 1 and 3 are
    # cordoned (queued walk); both walks end in a partial wave
    "inactive-lanes-between": dict(segments=[(0, 0, 20, 50), (0, 2, 7, 9), (1, 1, 40, 70), (2, 0, 3, 40), (2, 1, 33, 2), (3, 2, 10, 90), (4, 1, 25, 30)], q=5, cordoned=[0, 1, 0, 1, 0]),
    "one-column": dict(segments=[(0, 0, 20, 50), (1, 1, 40, 70), (1, 2, 9, 9), (2, 0, 33, 40)], q=3, r=1, cordoned=[0, 0, 1]),
    "eight-columns": dict(segments=[(0, 0, 20, 50), (1, 1, 40, 70), (1, 2, 9, 9), (2, 0, 33, 40)], q=3, r=8, cordoned=[0, 0, 1]),
})


def _agg_case(name):
    c = AGG[name]
    wl = _agg_pool(c["segments"], c["q"], r=c.get("r", W.R))
    cordoned = c.get("cordoned", [0] * c["q"])
    return wl, cordoned, _agg_fractions(wl, cordoned)


@pytest.mark.parametrize("name", list(AGG))
def test_c_derived_aggregates(libs, oracle_lib, name):
    wl, cordoned, frac = _agg_case(name)
    m, npc = wl.num_jobs, len(PCS)
    # the two walks as the kernel sees them
    order = _run_order(wl)
    run_waves = _waves((wl.job_queue * npc + wl.job_pc)[order], (wl.job_node >= 0)[order])
    ql = np.concatenate(wl.queued).astype(int) if m else np.zeros(0, int)
    q_of = np.concatenate([np.full(len(x), q) for q, x in enumerate(wl.queued)]).astype(int) if m else np.zeros(0, int)
    queued_waves = _waves(q_of * npc + wl.job_pc[ql], ~np.asarray(cordoned, bool)[q_of])
    if name.startswith("running-"):
        n = int(name[8:])
        assert len(order) == n and sum(a for a, _ in run_waves) == n and len(ql) == 0
    if name.startswith("queued-"):
        n = int(name[7:])
        assert len(ql) == n and sum(a for a, _ in queued_waves) == n and sum(a for a, _ in run_waves) == 0 and len(order) == n
    if name == "one-key-per-wave":
        assert run_waves[0] == (64, 1) and run_waves[1] == (64, 1) and queued_waves[:2] == [(64, 1), (64, 1)]
    if name in ("64-queues-in-a-wave", "22-queues-x-3-classes"):
        assert queued_waves[0] == (64, 64)                              # 64 different keys in one wave of the queued walk ...
        assert run_waves[0][0] == run_waves[0][1] >= 32                 # ... and 32 in one of the run-order walk (a queue's queued rows follow its running rows)
    if name in ("64-queues-running", "22-queues-x-3-classes-running"):
        assert run_waves[0] == (64, 64)
    if name == "run-from-mid-wave-over-three-waves":
        assert queued_waves[0] == (64, 2) and queued_waves[1] == (64, 1) and queued_waves[2][1] == 2
    if name == "inactive-lanes-between":
        assert any(0 < a < 64 for a, _ in run_waves[:-1]) and any(0 < a < 64 for a, _ in queued_waves[:-1]) and len(order) % WAVE and len(ql) % WAVE
    if m:
        assert len(np.unique(wl.job_req[:, 0])) == m and wl.job_req.max() > 2 ** 40 or m < 2
        by_pc, _ = _aggregates(wl, cordoned, None)
        assert (2 * by_pc.sum(axis=(0, 1)) <= wl.node_total.sum(axis=0)).all()      # total demand is at most half the pool
    want = _once(("c", name), lambda: _agg_round(oracle_lib, wl, cordoned, frac, True))
    got = _agg_round(libs, wl, cordoned, frac, False)
    scenario.assert_same_round(want, got)


def test_c_the_cap_the_class_and_the_cordon_rule_matter(oracle_lib):
    """negative control (as test_the_cap_and_the_cordon_rule_matter): the aggregates without the per-class cap, with a cordoned queue's queued rows counted, or with one
    row's request booked under another class of its queue are different numbers and give a different round"""
    wl, cordoned, frac = _agg_case("inactive-lanes-between")
    good = _once(("c", "inactive-lanes-between"), lambda: _agg_round(oracle_lib, wl, cordoned, frac, True))
    scenario.assert_same_round(good, _agg_round(oracle_lib, wl, cordoned, frac, False))      # the oracle derives what the numpy restatement hands over
    demand, _ = _aggregates(wl, cordoned, frac)
    uncapped, _ = _aggregates(wl, cordoned, np.full_like(frac, math.inf))
    uncordoned, _ = _aggregates(wl, [0] * wl.num_queues, frac)
    moved = copy.copy(wl)
    moved.job_pc = wl.job_pc.copy()
    j = int(np.nonzero((wl.job_queue == 2) & (wl.job_pc == 0) & (wl.job_node < 0))[0][0])
    moved.job_pc[j] = 2                                                 # a queued row of queue 2, class 0 booked under class 2 (capped just above its own sum)
    misbooked, _ = _aggregates(moved, cordoned, frac)
    for other in (uncapped, uncordoned, misbooked):
        assert (other != demand).any()
        bad = _agg_round(oracle_lib, wl, cordoned, frac, True, demand=other)
        assert (bad.demand_capped_adjusted_fair_share != good.demand_capped_adjusted_fair_share).any()


# ================================================================================================ D. k_evict_apply, phase 1 and phase 3
# three classes of ONE priority: within a queue the pre-sorted order of the running rows is then the run timestamp alone, and the evict flag of a lane is the test's choice
EV_PCS = ((0, True), (0, False), (0, True))
P, N_, P2 = 0, 1, 2   # preemptible, not preemptible, preemptible (a second key of the same queue)


def _evict_pool(rows, gang=None, queued=6):
    """rows: [(queue, class)] of the running jobs in run order (queues ascending; one cpu each, memory and ephemeral storage by the row), 16 to a node, every node
    exactly full; `queued` one-cpu jobs of a further queue that runs nothing: with a protected fraction of 0 the evictor of phase 1 flags every running row of a
    preemptible class, the starved queue takes the place of some of them, the others return"""
    nr = len(rows)
    queue = np.array([q for q, _ in rows] + [max(q for q, _ in rows) + 1] * queued)
    assert (np.diff(queue) >= 0).all()
    pc = np.array([p for _, p in rows] + [P] * queued)
    n_nodes = max(1, nr // 16)
    node = np.concatenate([np.arange(nr) % n_nodes, np.full(queued, -1)])
    m = nr + queued
    req = np.stack([(1 + np.arange(m) % 8) * Gi, np.full(m, 1000), (np.arange(m) % 4) * Gi, np.zeros(m, np.int64)], axis=1).astype(np.int64)
    total = np.tile(np.array([1 << 44, 0, 1 << 44, 0], dtype=np.int64), (n_nodes, 1))
    total[:, CPU] = np.bincount(node[:nr], minlength=n_nodes) * 1000
    g = None if gang is None else np.concatenate([np.asarray(gang), np.full(queued, -1)])
    return _workload(W._config(list(EV_PCS)), total, req, queue, pc, node, int(queue.max()) + 1, gang=g)


def _evict_round(lib, wl):
    s = _prepared(lib, wl)
    res = s.schedule_round()
    alloc = s.get_nodes_alloc()
    s.close()
    return res, alloc


def _pattern(flags, queue=0):
    return [(queue, P if f else N_) for f in flags]


def _total(t):
    """t flagged rows of three queues, an unflagged row after every third"""
    rows = []
    for i in range(t):
        rows.append((i * 3 // max(t, 1), P if i % 5 else P2))
        if i % 3 == 2:
            rows.append((i * 3 // max(t, 1), N_))
    return rows


EVICT = {
    # wave 0: every lane; wave 1: none (`if (!todo) continue`); wave 2: every lane
    "every-lane-none-every-lane": _pattern([1] * 64 + [0] * 64 + [1] * 64),
    "alternating-lanes": _pattern([i % 2 for i in range(130)]),
    "lane-0-only": _pattern([i % 64 == 0 for i in range(200)]),
    "lane-63-only": _pattern([i % 64 == 63 for i in range(200)]),
    "64-keys-in-a-wave": [(q, (P, P2)[k]) for q in range(32) for k in range(2)] + [(32, N_)] * 8,
    # one key from lane 8 of wave 3 to behind the second workgroup boundary
    "run-across-waves-and-workgroups": _pattern([0] * 200, 0) + _pattern([1] * 330, 1) + _pattern([1, 0] * 10, 2),
}
for _t in (1, 63, 64, 65, 255, 256, 257):
    EVICT[f"total-{_t}"] = _total(_t)


@pytest.mark.parametrize("name", list(EVICT) + ["gangs"])
def test_d_evict_phase1(libs, oracle_lib, name):
    gang = None
    if name == "gangs":
        # pairs and a gang of 70 (more than a wave), members in one queue; every third member is of the class that is not preemptible: the closure flags it with its gang
        rows = [(i // 60, N_ if i % 3 == 0 else P) for i in range(180)]
        gang = np.full(180, -1)
        for k in range(20):
            gang[[3 * k, 3 * k + 1]] = k
        gang[100:120] = 20; gang[120:180] = 21
    else:
        rows = EVICT[name]
    wl = _evict_pool(rows, gang)
    nr = len(rows)
    want, want_alloc = _once(("d", name), lambda: _evict_round(oracle_lib, wl))
    order = _run_order(wl)
    assert (order[:nr] == np.arange(nr)).all()                                   # the run order is the row order
    flagged = np.array([p != N_ for _, p in rows])
    if gang is not None:
        flagged |= np.isin(gang, np.unique(gang[flagged & (gang >= 0)])) & (gang >= 0)   # evictGangs: a partly evicted gang is evicted entirely
        assert flagged.sum() > np.array([p != N_ for _, p in rows]).sum()
    assert want.num_evicted_phase1 == int(flagged.sum()) and want.num_evicted_phase3 == 0
    # the starved queue's jobs took the place of some of the evicted (a gang leaves whole), the others returned
    assert (len(want.preempted) > 0 and len(want.scheduled) > 0) or int(flagged.sum()) == 1
    assert len(want.preempted) <= 6 or gang is not None
    keys = np.array([q * 3 + p for q, p in rows])
    waves = _waves(keys, flagged)
    if name == "every-lane-none-every-lane":
        assert [a for a, _ in waves] == [64, 0, 64]
    if name == "alternating-lanes":
        assert waves[0] == (32, 1) and not flagged[0] and flagged[1]
    if name == "lane-0-only":
        assert np.nonzero(flagged)[0].tolist() == [0, 64, 128, 192]
    if name == "lane-63-only":
        assert np.nonzero(flagged)[0].tolist() == [63, 127, 191]
    if name == "64-keys-in-a-wave":
        assert waves[0] == (64, 64)
    if name == "run-across-waves-and-workgroups":
        run = np.nonzero(keys == 1 * 3 + P)[0]
        assert run[0] % WAVE not in (0, 63) and run[0] // WG == 0 and run[-1] // WG == 2 and flagged[run].all()
    if name.startswith("total-"):
        assert int(flagged.sum()) == int(name[6:])
    got, got_alloc = _evict_round(libs, wl)
    scenario.assert_same_round(want, got)
    assert (got_alloc == want_alloc).all()


def _phase3_pool():
    """10 nodes of 16 cores hold 14 one-core jobs of queue 0 each (class 0, priority 0) and are 2 cores short of full; an eleventh node is full of queue 2's (class 0).
    Queue 1 has 20 queued one-core jobs of class 0, queue 2 six queued jobs of 12 cores of class 2 (priority 3) and a weight of 0.001.  Phase 1 evicts every running
    job.  Pass 1 goes by the priority of the queues' next jobs, then by cost: queue 0's jobs return (F_RESCHEDULED), queue 1's take the free cores (F_SUCCESSFUL), queue
    2's own evicted jobs return last — only then are its urgent jobs the queue's next, every node is full at priority 0, and each of them lands on a node of its own
    by urgency preemption.  The oversubscribed evictor of phase 3 then takes all 16 preemptible jobs of each of those nodes"""
    nn = 10
    queue = [0] * (14 * nn) + [2] * 16 + [1] * (2 * nn) + [2] * 6
    pc = [0] * (14 * nn + 16 + 2 * nn) + [2] * 6
    node = [n for n in range(nn) for _ in range(14)] + [nn] * 16 + [-1] * (2 * nn + 6)
    m = len(queue)
    cpu = np.array([1000] * (m - 6) + [12000] * 6)
    req = np.stack([(1 + np.arange(m) % 8) * Gi, cpu, (np.arange(m) % 4) * Gi, np.zeros(m, np.int64)], axis=1).astype(np.int64)
    total = np.tile(np.array([1 << 44, 16000, 1 << 44, 0], dtype=np.int64), (nn + 1, 1))
    return _workload(W._config(list(PCS)), total, req, queue, pc, node, 3, weight=[1.0, 1.0, 0.001])


def test_d_evict_phase3(libs, oracle_lib):
    wl = _phase3_pool()
    want, want_alloc = _once(("d", "phase3"), lambda: _evict_round(oracle_lib, wl))
    urgent = [j for j in want.scheduled if wl.job_pc[j] == 2]
    over = {want.scheduled[j] for j in urgent}
    assert len(urgent) == len(over) == 6 and max(over) < 10                      # six oversubscribed nodes, each held 14 jobs of queue 0 before the round
    assert want.num_evicted_phase1 == int((wl.job_node >= 0).sum())               # every running job was evicted by phase 1: what is bound later was rescheduled or is new
    assert want.num_evicted_phase3 == 16 * len(over) >= 65                        # more than a wave; all 16 preemptible jobs of each of those nodes:
    assert want.num_evicted_phase3 > 14 * len(over)                               #   more than the jobs that had run there: jobs pass 1 newly scheduled among them
    assert want.num_evicted_phase3 > 2 * len(over)                                #   more than the free cores held: jobs pass 1 had rescheduled among them
    assert len(want.preempted) > 0 and set(want.preempted.values()) <= over
    got, got_alloc = _evict_round(libs, wl)
    scenario.assert_same_round(want, got)
    assert (got_alloc == want_alloc).all()


# ================================================================================================ E. the second stride of the grid
def _stride_pool(m, seam):
    """m resident jobs, nearly all running and not preemptible (queues 1 and 3, class 2); `seam` = 8 x CUs x 256 is the first run-order position of the grid's second
    stride.  Twelve preemptible running jobs each sit at run-order positions 0 .., astride the seam (six on either side), behind it and up to m - 1 (queues 0, 2, 4, 5, class
    0), and four queued jobs of class 1 stand behind each of the first three groups: with a protected fraction of 0 phase 1 evicts the 48, the queued ones — a higher
    priority, the same queues, behind their queue's returning jobs — take the place of some of them by urgency preemption, and the evictor of phase 3 follows.  Every node is exactly full"""
    e, k = 12, 4
    assert m >= seam + 2 * (e + k) + e and seam >= 2 * (e + k) + e
    b1 = seam - e // 2 - (e + k)
    b2 = m - (seam + e // 2 + k) - (e + k) - e
    seg = [(0, 0, e, True), (0, 1, k, False), (1, 2, b1, True), (2, 0, e, True), (2, 1, k, False), (3, 2, b2, True), (4, 0, e, True), (4, 1, k, False), (5, 0, e, True)]
    queue = np.concatenate([np.full(n, q) for q, _, n, _ in seg])
    pc = np.concatenate([np.full(n, p) for _, p, n, _ in seg])
    run = np.concatenate([np.full(n, r) for _, _, n, r in seg])
    assert len(queue) == m
    n_nodes = max(1, m // 5000)
    node = np.where(run, np.arange(m) % n_nodes, -1)
    req = np.stack([(1 + np.arange(m) % 8) * Gi, np.full(m, 1000), (np.arange(m) % 4) * Gi, np.zeros(m, np.int64)], axis=1).astype(np.int64)
    total = np.tile(np.array([1 << 46, 0, 1 << 46, 0], dtype=np.int64), (n_nodes, 1))
    total[:, CPU] = np.bincount(node[run], minlength=n_nodes) * 1000
    return _workload(W._config(list(PCS)), total, req, queue, pc, node, 6)


def _stride_round(lib, wl):
    t0 = time.perf_counter()
    res, alloc = _evict_round(lib, wl)
    return res, alloc, time.perf_counter() - t0


@pytest.mark.parametrize("words", WORDS)
def test_e_second_stride(libs, oracle_lib, request, monkeypatch, words):
    """words == 2: the handle's bulk passes are k_bulk_wk's (armada_sched_wk.hip), the sums still k_agg's and k_evict_apply's"""
    if request.node.callspec.params["libs"] == "hip":
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        seam = 8 * cus * WG                                                       # bulkGrid: at most 8 workgroups of 256 threads per CU
        m = seam + 257
        print(f"compute units {cus}: the grid's cap is {seam} elements, M = {m}")
    else:
        m = 4099                                                                  # the CPU build has no grid: this leg only proves the generator
        seam = m - 257
    wl = _stride_pool(m, seam)
    order = _run_order(wl)
    evictable = (wl.job_node >= 0) & (wl.job_pc == 0)
    at = np.nonzero(evictable[order])[0]
    assert {0, seam - 1, seam, m - 1} <= set(at.tolist()) and len(at) == 48
    assert (np.nonzero((wl.job_node < 0)[order])[0] < seam).any() and (np.nonzero((wl.job_node < 0)[order])[0] > seam).any()
    want, want_alloc, secs = _once(("e", m), lambda: _stride_round(oracle_lib, wl))
    print(f"the oracle's round of M = {m}: {secs:.1f} s")
    assert want.num_evicted_phase1 == 48 and want.num_evicted_phase3 > 0        # (the queued jobs' urgency preemption oversubscribes nodes: phase 3 walks the long order too)
    pre = set(order.tolist().index(j) for j in want.preempted)
    assert len(want.scheduled) == 12 and len(pre) == 12 and min(pre) < seam < max(pre)   # work on both sides of the seam
    _set_words(monkeypatch, words)
    got, got_alloc, _ = _stride_round(libs, wl)
    scenario.assert_same_round(want, got)
    assert (got_alloc == want_alloc).all()
