"""The submit check's two gang-unit paths at their edges (armada_amd/csrc/submit_gang.h): `k_submit_gangs` — one workgroup per unit, a 256-thread stride over
the nodes, a node bitmap in LDS, the unit's binds in SgShared, min(units, 4096) workgroups striding over the units, at most SG_TMAX = 256 members — and `k_fit_capacity` —
uniform units as one pass over the nodes, 256 nodes per tile, min(shapes, ceil(2048 / tiles)) rows of blocks striding over the shapes, blocks combined by atomic min / add.

The reference of every case is the ORACLE's submit_check of the same units: one transaction per unit, members one after the other (ScheduleManyWithTxn restated literally; it
reads nothing of the code under test).  All four result words of every unit are compared — integers, tolerance zero — and on top of that the library's own sequential
path (ASCHED_SUBMIT_GANGS=0) must answer the same, and on the GPU the list must equal the CPU build's.  Where a case can be worked out by hand the oracle's answer is
pinned to that too (`want`), so a pool that does not build the situation it is named after fails.

Every case says which path it ran: `submit_stats` counts a unit on the capacity path and a unit on the workgroup path alike in gang_units, but node_passes is +1 per
capacity launch and + the member count of every unit sent to k_submit_gangs, so the expected gang_units / sequential_units / node_passes are computed from how the
input was built and asserted — never read off the library first.

A. the workgroup kernel over the nodes; B. a workgroup reused across units (> 4096 units); C. the capacity kernel; D. one batch through every path; E. the state of the
handle (after a round, after nodes_append / nodes_delete / nodes_patch, used nodes, a two-word key); F. a small seeded sweep.

A.6, the "key field left the layout" exit of sgKey (result -1, the host hands the unit to the sequential path): with non-negative requests it cannot be reached through
the ABI.  sgKey is only asked about a node an earlier member of the unit was bound to, with that unit's binds taken off level 0.  Every bound member fitted, so every
column stays >= 0 and the quotient q stays in [0, allocatable / resolution]: the narrow layout (keyClamp 1, keyLo -1) holds q + 1 <= maxq + 1 by construction of its
width, and the wide layout (keyClamp 0: a negative request, a literal row, ASCHED_KEY_LAYOUT=w) has keyLo <= 0 and a width for maxq + 1 - keyLo, so 0 <= q - keyLo fits as
well (asched_host.inc layoutKeys).  Only a NEGATIVE request on an indexed column — which the reference's jobs never carry — lets a bind RAISE a column past the layout;
then the sequential path raises the same condition (round_ctl.h packKey: ASCHED_ERR_UNSUPPORTED) and the whole call is refused, so there is no answer to compare:
test_negative_request_leaves_the_layout pins exactly that (the refusal, with and without the gang path, and the handle's next call) and nothing more.  B.2's "unit u
ends in -1" has no observable either, for the same reason."""
import numpy as np
import pytest

from armada_amd import workloads as W
from armada_amd.binding import Config, SchedError, Scheduler

SG_NT = 256          # threads of a k_submit_gangs workgroup: the stride of its node loop
SG_UNITS = 4096      # workgroups of one k_submit_gangs launch at the most: the stride over the units
SG_TMAX = 256        # members of a unit on the workgroup path
TILE = 256           # nodes per k_fit_capacity block
CAP_BLOCKS = 2048    # k_fit_capacity: tiles x rows of blocks stays about this
ERR_UNSUPPORTED = -2
T, F = True, False


@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def libs(request):
    """(library under test, CPU build to compare its answers with or None)"""
    hs = request.getfixturevalue("hostsim_lib")
    return (hs, None) if request.param == "hostsim" else (request.getfixturevalue("hip_lib"), hs)


# ---------------------------------------------------------------- pools and the comparison
def config(R=2, res=1, pcs=(0,)):
    """column 0 is the one indexed resource: the key order of the nodes is (allocatable[0] / res, rank of node.index)"""
    return Config(num_resources=R, indexed_col=[0], indexed_resolution=[res], pc_priority=list(pcs), pc_preemptible=[1] * len(pcs), drf_multiplier=[1.0] * R)


class Pool:
    """a node table and a job table built row by row; `handle` uploads them to a library"""

    def __init__(self, alloc, *, cfg=None, index=None, labels=None, taints=None, unschedulable=None, used=None, clear=True):
        self.alloc = np.array(alloc, dtype=np.int64)
        self.cfg = cfg or config(self.alloc.shape[1])
        self.index, self.labels, self.taints, self.unschedulable = index, labels, taints, unschedulable
        self.used = used          # [N][R] taken at priority <= 0 (testfixtures.WithUsedResourcesNodes): alloc_by_prio of the upsert, no clear_allocated
        self.clear = clear and used is None
        self.req, self.pc, self.cls = [], [], []
        self.tolerations, self.selectors = [[]], [[]]

    def rows(self, req, n=1, pc=0, cls=0):
        """n job rows of this request -> their ids"""
        first = len(self.req)
        self.req += [tuple(req)] * n; self.pc += [pc] * n; self.cls += [cls] * n
        return list(range(first, first + n))

    def upsert(self, s):
        abp = None
        if self.used is not None:
            abp = np.repeat(self.alloc[:, None, :], s.P, axis=1).copy()
            for l, pr in enumerate(s.priorities):
                if pr <= 0:
                    abp[:, l, :] -= np.asarray(self.used, dtype=np.int64)
        s.nodes_upsert(self.alloc, index=self.index, labels=self.labels, taints=self.taints, unschedulable=self.unschedulable, alloc_by_prio=abp)

    def set_jobs(self, s):
        s.jobs_set(np.array(self.req, dtype=np.int64).reshape(-1, self.alloc.shape[1]), pc=self.pc, req_class=self.cls, class_tolerations=self.tolerations, class_selectors=self.selectors)

    def handle(self, lib):
        s = Scheduler(lib, self.cfg)
        self.upsert(s)
        if self.clear:
            s.clear_allocated()
        self.set_jobs(s)
        return s


def stats(gang=0, seq=0, passes=0, wide=0, wide_passes=0, literal=0):
    return dict(wide_units=wide, wide_passes=wide_passes, sequential_units=seq, gang_units=gang, node_passes=passes, literal_units=literal)


def ask(s, units, strip, mp, csr=None):
    """the answers and counters of the handle: as it is, and with the gang paths switched off"""
    mp.delenv("ASCHED_SUBMIT_GANGS", raising=False)
    a, st = s.submit_check(units, strip, csr=csr), s.submit_stats()
    mp.setenv("ASCHED_SUBMIT_GANGS", "0")
    try:
        b, st0 = s.submit_check(units, strip, csr=csr), s.submit_stats()
    finally:
        mp.delenv("ASCHED_SUBMIT_GANGS", raising=False)
    return a, st, b, st0


def diff(units, got, ref):
    bad = [i for i in range(len(ref)) if got[i] != ref[i]]
    return [(i, len(units[i]) if units is not None else None, got[i], ref[i]) for i in bad[:5]], len(bad)


def pin(libs, oracle, mp, pool, units, want_stats, *, strip=None, csr=None, want=None):
    """the library's answers == the oracle's == its own sequential path's (== the CPU build's); its counters == want_stats; the oracle's answers == want where given"""
    lib, cpu = libs
    nu = len(units) if csr is None else len(csr[0]) - 1
    strip = [False] * nu if strip is None else strip
    o = pool.handle(oracle)
    ref = o.submit_check(units, strip, csr=csr)
    o.close()
    for u, w in (want or {}).items():
        assert ref[u] == w, ("the pool does not build the situation", u, ref[u], w)
    s = pool.handle(lib)
    got, st, seq, st0 = ask(s, units, strip, mp, csr)
    s.close()
    assert got == ref, diff(units, got, ref)
    assert st == want_stats, (st, want_stats)
    assert seq == ref, diff(units, seq, ref)
    assert st0["gang_units"] == 0 and st0["sequential_units"] == want_stats["sequential_units"] + want_stats["gang_units"], st0
    assert (st0["wide_units"], st0["wide_passes"], st0["literal_units"]) == (st["wide_units"], st["wide_passes"], st["literal_units"])
    if cpu is not None:
        c = pool.handle(cpu)
        assert c.submit_check(units, strip, csr=csr) == got
        c.close()
    return ref


def capacity(alloc, req, nodes=None):
    """members of one request the nodes take together, from the table alone (nodedb.go first fit on an empty NodeDb: each node is filled before the next)"""
    alloc, req = np.asarray(alloc, dtype=np.int64), np.asarray(req, dtype=np.int64)
    total = 0
    for n in (range(len(alloc)) if nodes is None else nodes):
        if (alloc[n] >= req).all():
            total += min(int(alloc[n][r] // req[r]) for r in range(len(req)) if req[r] > 0)
    return total


# ---------------------------------------------------------------- A. the workgroup kernel over the nodes
def stride_pool(N, p, kind):
    """N nodes of (100 cpu, 8 mem); p is the ONLY node that takes the first member (40 mem), q the only other one that takes the second (30 mem).
    kind "last": p is last in key order (105 cpu) and the bind makes it first among what is left (95); "tie": p shares 100 cpu with everyone and wins by rank (p == 0);
    "first": p is first in key order (99) wherever it lies.  q: half the table away ("first": node 5, in the first turn of the stride)."""
    alloc = np.tile(np.array([100, 8], dtype=np.int64), (N, 1))
    alloc[p] = {"last": (105, 64), "tie": (100, 64), "first": (99, 64)}[kind]
    if N >= 2:
        q = 5 if kind == "first" else (p + max(1, N // 2)) % N
        assert q != p
        alloc[q] = (100, 32)
    pool = Pool(alloc)
    # m0 -> p (only node with 40 mem; 24 left).  m1 no longer fits on p -> q (2 mem left there; cpu 90).  "last": m2 (1, 2) -> q (key 90, recomputed), m3 (1, 2): q is
    # full -> p (key 95 recomputed, below the others' 100), leaving 22 mem.  "tie" / "first": m2 and m3 both return to p (90 with the lower rank / 89), leaving 20 mem.
    left = 22 if kind == "last" else 20
    m = [pool.rows(r)[0] for r in ((10, 40), (10, 30), (1, 2), (1, 2), (1, left), (1, left + 1))]
    units = [m[:4] + [m[4]], m[:4] + [m[5]]]
    want = {0: (T, F, 5, p), 1: (F, F, 4, p)} if N >= 2 else {0: (F, F, 1, 0), 1: (F, F, 1, 0)}
    return pool, units, want


@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 600])
def test_a1_node_stride_and_bitmap_words(libs, oracle_lib, monkeypatch, N):
    """the node loop's first and further turns (N around 256 and 512), the bitmap's last word full and partial (N around 32 and 64) with the bound node in it, the only
    fitting node first / last / in the second turn, a member that leaves the node of an earlier one and small members that return to it (tn / td, the key from sgKey)"""
    cases = [(N - 1, "last"), (0, "tie")] if N > 1 else [(0, "tie")]
    if N > SG_NT:
        cases.append((max(SG_NT, N - 3), "first"))
    for p, kind in cases:
        pool, units, want = stride_pool(N, p, kind)
        pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=2, passes=10), want=want)


@pytest.mark.parametrize("N", [255, 300])
def test_a2_every_member_on_a_node_of_its_own(libs, oracle_lib, monkeypatch, N):
    """node-sized members of two alternating shapes: nT reaches 255 and 256 (the last tn / td slot); with 255 nodes the 256th member finds none"""
    pool = Pool(np.tile(np.array([100, 8], dtype=np.int64), (N, 1)))
    a, b = pool.rows((100, 1), 128), pool.rows((100, 2), 128)
    mem = [x for pair in zip(a, b) for x in pair]
    units = [mem[:255], mem[:256]]
    want = {0: (T, F, 255, 0), 1: (T, F, 256, 0) if N >= 256 else (F, F, 255, 0)}
    pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=2, passes=511), want=want)


def test_a3_every_member_on_one_node(libs, oracle_lib, monkeypatch):
    """node 0 (first in key order) takes 100 members of two alternating shapes in ONE tn entry whose td accumulates; the 101st moves on to node 1 — or, where node 1
    has no memory, fails; a member nobody takes at position k fails the unit with num_schedulable == k"""
    for next_takes in (True, False):
        alloc = np.tile(np.array([2000, 0], dtype=np.int64), (40, 1))
        alloc[0] = (1000, 1000)
        if next_takes:
            alloc[1] = (2000, 1000)
        pool = Pool(alloc)
        a, b = pool.rows((10, 1), 60), pool.rows((10, 2), 60)
        mem = [x for pair in zip(a, b) for x in pair]
        huge = pool.rows((5000, 1))[0]
        units = [mem] + [mem[:k] + [huge] + mem[k + 1:] for k in (1, 60, 119)]
        want = {0: (T, F, 120, 0) if next_takes else (F, F, 100, 0), 1: (F, F, 1, 0), 2: (F, F, 60, 0), 3: (F, F, 119, 0) if next_takes else (F, F, 100, 0)}
        pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=4, passes=480), want=want)


def test_a4_member_count_around_sg_tmax(libs, oracle_lib, monkeypatch):
    """255 and 256 members of two shapes: the workgroup path; 257 of two shapes: the sequential path; 257 of one shape: the capacity path"""
    pool = Pool(np.tile(np.array([100, 8], dtype=np.int64), (300, 1)))
    a, b = pool.rows((1, 0), 129), pool.rows((2, 0), 128)
    mem = [a[0]] + [x for pair in zip(b, a[1:]) for x in pair]          # 257 members, two shapes in every prefix of two or more
    uni = pool.rows((1, 0), 257)
    units = [mem[:255], mem[:256], mem, uni]
    want = {0: (T, F, 255, 0), 1: (T, F, 256, 0), 2: (T, F, 257, 0), 3: (T, F, 257, 0)}
    pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=3, seq=1, passes=255 + 256 + 1), want=want)


@pytest.mark.parametrize("kind", ["label", "taint"])
def test_a5_mask_row_excludes_the_node_of_an_earlier_member(libs, oracle_lib, monkeypatch, kind):
    """node 0 is the only one with room for the second member, the first member sits there, and the second member's mask row (a selector on a label node 0 lacks / a
    taint on node 0 it does not tolerate) excludes it: the tn loop must apply the mask too"""
    N = 70
    alloc = np.tile(np.array([100, 8], dtype=np.int64), (N, 1))
    alloc[0] = (50, 64)
    if kind == "label":
        pool = Pool(alloc, labels=[[] if n == 0 else [(7, 1)] for n in range(N)])
        pool.tolerations, pool.selectors = [[], []], [[], [(7, 1)]]
    else:
        pool = Pool(alloc, taints=[[(9, 1, 1)] if n == 0 else [] for n in range(N)])
        pool.tolerations, pool.selectors = [[(9, 1, 0, 0)], []], [[], []]                 # class 0 tolerates key 9, class 1 does not
    m0, m1, m2 = pool.rows((10, 40), cls=0)[0], pool.rows((10, 20), cls=1)[0], pool.rows((10, 8), cls=1)[0]
    units = [[m0, m1], [m0, m2]]
    pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=2, passes=4), want={0: (F, F, 1, 0), 1: (T, F, 2, 0)})


def test_a5_literal_rows_go_sequential(libs, oracle_lib, monkeypatch):
    """a member whose request is off the index grid iterates literally (rowLiteral): the unit is not sent to either kernel"""
    alloc = np.tile(np.array([100000, 8], dtype=np.int64), (70, 1))
    alloc[3] = (50000, 8)
    pool = Pool(alloc, cfg=config(2, res=1000))
    a, b, c = pool.rows((1500, 1))[0], pool.rows((2000, 1))[0], pool.rows((3000, 1))[0]
    units = [[a, b], [b, c], pool.rows((1500, 1), 3)]
    pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=1, seq=2, passes=2), want={0: (T, F, 2, 3), 1: (T, F, 2, 3), 2: (T, F, 3, 3)})


def test_negative_request_leaves_the_layout(libs, oracle_lib, monkeypatch):
    """(A.6, see the module docstring) a negative request on the indexed column raises node 0's quotient past the key layout: sgKey flags it, the host hands the unit to
    the sequential path, which refuses the call for the same reason — with the gang path and without it — and the handle answers the next call"""
    lib, _ = libs
    pool = Pool(np.tile(np.array([100, 8], dtype=np.int64), (40, 1)))
    neg, small = pool.rows((-30000, 1))[0], pool.rows((1, 1))[0]
    ok = [pool.rows((1, 1))[0], pool.rows((2, 1))[0]]
    s = pool.handle(lib)
    for env in (None, "0"):
        monkeypatch.delenv("ASCHED_SUBMIT_GANGS", raising=False)
        if env:
            monkeypatch.setenv("ASCHED_SUBMIT_GANGS", env)
        with pytest.raises(SchedError) as e:
            s.submit_check([ok, [neg, small]], [False, False])
        assert e.value.code == ERR_UNSUPPORTED
        assert s.submit_stats()["sequential_units"] == (1 if env is None else 2)          # the gang path kept the unit it could answer
    monkeypatch.delenv("ASCHED_SUBMIT_GANGS", raising=False)
    assert s.submit_check([ok], [False]) == [(T, F, 2, 0)]
    s.close()


# ---------------------------------------------------------------- B. a workgroup reused across units
def reuse_pool():
    """40 nodes of (100, 8); node 7 is first in key order (95 cpu); X = nodes 3 and 35 — two bitmap words — are the only ones with 64 mem"""
    alloc = np.tile(np.array([100, 8], dtype=np.int64), (40, 1))
    alloc[7] = (95, 8)
    alloc[3] = alloc[35] = (100, 64)
    pool = Pool(alloc)
    r = lambda *req: pool.rows(req)[0]   # noqa: E731
    u = {}
    u["fill"] = ([r(100, 64), r(100, 63)], (T, F, 2, 3))                       # takes all of X
    u["half"] = ([r(100, 64), r(100, 63), r(100, 60)], (F, F, 2, 3))           # binds all of X, then fails
    u["needx"] = ([r(50, 60), r(50, 59)], (T, F, 2, 3))                        # fits on X only, one member on each node
    g = [r(10, 8) if i % 2 == 0 else r(10, 7) for i in range(9)]
    u["nine"] = (g, (T, F, 9, 7))                                             # nodes 7, 0, 1, 2, then 3: five tn entries, node 0 left at (90, 1)
    a, b = r(1, 1), r(2, 1)
    u["f0"] = ([a, b], (T, F, 2, 7))                                           # a stale tn entry of node 0 keyed 90 < 95 would answer node 0
    u["f1"] = ([r(96, 1), b], (T, F, 2, 0))
    u["f2"] = ([r(10, 9), b], (T, F, 2, 3))
    u["f3"] = ([a, r(200, 1)], (F, F, 1, 7))
    return pool, u


def reuse_units(nu):
    pool, u = reuse_pool()
    names = [("f0", "f1", "f2", "f3")[(i * 7 + i // 13) % 4] for i in range(nu)]
    # (workgroup w takes units w, w + 4096, w + 8192)
    special = {0: "fill", SG_UNITS: "half", 2 * SG_UNITS: "needx",                       # X filled / X bound by a unit that fails / X needed
               5: "fill", 5 + SG_UNITS: "needx", 100: "half", 100 + SG_UNITS: "needx",
               4000: "nine", 4000 + SG_UNITS: "f0",                                       # nine members, then two
               4001: "half", 4001 + SG_UNITS: "f2"}
    for i, name in special.items():
        if i < nu:
            names[i] = name
    return pool, [u[n][0] for n in names], {i: u[n][1] for i, n in enumerate(names)}


@pytest.mark.parametrize("nu", [SG_UNITS + 1, 2 * SG_UNITS + 1])
def test_b_workgroup_reused_across_units(libs, oracle_lib, monkeypatch, nu):
    """more than 4096 units of two shapes each in one call: workgroup 0 takes two (4097) or three (8193) of them.  The later unit of a workgroup is built so that a bit
    left in the bitmap, a tn / td entry or an nT left by the earlier one changes its answer; the units in another order give the answers in that order."""
    pool, units, want = reuse_units(nu)
    members = sum(len(x) for x in units)
    assert nu > SG_UNITS and all(len({pool.req[j] for j in x}) > 1 for x in units)         # every unit is sent to k_submit_gangs
    ref = pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=nu, passes=members), want=want)
    perm = np.random.default_rng(nu).permutation(nu)
    s = pool.handle(libs[0])
    got = s.submit_check([units[i] for i in perm], [False] * nu)
    assert s.submit_stats() == stats(gang=nu, passes=members)
    s.close()
    assert got == [ref[i] for i in perm]


# ---------------------------------------------------------------- C. the capacity kernel
def tile_pool(N):
    """resources (cpu, mem, gpu, fpga).  Node 5 (tile 0; 70 cpu: first in key order) has 1 gpu, nodes 7 and 9 (tile 0) 4 fpga each, node N - 1 (the last tile; 80 cpu:
    second in key order) 128 mem, 4 gpu and 1 fpga.  Label (7, 1) on the nodes of the last tile, (7, 2) on those of tile 0 where that is another one."""
    tiles = (N + TILE - 1) // TILE
    alloc = np.tile(np.array([100, 8, 0, 0], dtype=np.int64), (N, 1))
    alloc[5] = (70, 8, 1, 0)
    alloc[7] = alloc[9] = (100, 8, 0, 4)
    alloc[N - 1] = (80, 128, 4, 1)
    last = range(TILE * (tiles - 1), N)
    first = range(0, TILE) if tiles > 1 else range(0)
    labels = [[(7, 1)] if n in last else [(7, 2)] if n in first else [] for n in range(N)]
    pool = Pool(alloc, labels=labels)
    pool.tolerations, pool.selectors = [[], [], []], [[], [(7, 1)], [(7, 2)]]
    units, want = [], {}

    def shape(req, sizes, cls, cap, first_node, nodes=None):
        rows = pool.rows(req, max(max(sizes), 2), cls=cls)
        takes = [n for n in (range(N) if nodes is None else nodes) if (alloc[n] >= np.array(req)).all()]
        assert capacity(alloc, req, nodes) == cap and (min(takes, key=lambda n: (alloc[n, 0], n)) if takes else -1) == first_node
        for n in sizes:
            want[len(units)] = (n <= cap, F, min(n, cap), first_node)
            units.append(rows[:n])
    shape((10, 40, 0, 0), (2, 3, 4), 0, 3, N - 1)                     # only the last node: 128 / 40 = 3 members
    shape((10, 1, 1, 0), (4, 5, 6), 0, 5, 5)                          # first node in tile 0 (1 member), the rest of the capacity on the last node of the last tile (4)
    shape((10, 1, 0, 1), (8, 9, 10), 0, 9, N - 1)                     # the reverse: first in key order is the last node (1), the capacity in tile 0 (4 + 4)
    shape((10, 500, 0, 0), (2,), 0, 0, -1)                            # nobody
    c1 = capacity(alloc, (10, 1, 0, 0), last)                         # the mask row leaves only the last tile ...
    shape((10, 1, 0, 0), (c1 - 1, c1, c1 + 1), 1, c1, N - 1 if tiles > 1 else 5, last)
    c2 = capacity(alloc, (10, 1, 0, 0), first)                        # ... only tile 0 (one tile: nobody)
    shape((10, 1, 0, 0), (c2 - 1, c2, c2 + 1) if c2 else (2,), 2, c2, 5 if c2 else -1, first)
    shape((10, 1, 1, 0), tuple(range(2, 9)), 0, 5, 5)                 # many units of one shape: one slot, one answer, scaled per unit
    return pool, units, want


@pytest.mark.parametrize("N", [255, 256, 257, 512, 513, 2100])
def test_c1_capacity_tiles(libs, oracle_lib, monkeypatch, N):
    """one, two, three and nine tiles, the last one full, one node and partial: the first fitting node and the capacity in different tiles (the blocks' atomic min and
    add), a shape only the last node takes, a shape nobody takes, mask rows that exclude whole tiles, unit sizes one below / at / one above the capacity sum"""
    pool, units, want = tile_pool(N)
    pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=len(units), passes=1), want=want)


def test_c2_more_shapes_than_rows_of_blocks(libs, oracle_lib, monkeypatch):
    """8200 nodes are 33 tiles, so the launch has min(ns, ceil(2048 / 33)) = 63 rows of blocks and 70 uniform shapes make rows 0..6 take a second shape (i and i + 63).
    Even slots fit nowhere, odd slots on the 82 gpu nodes (one member each, spread over the tiles, the last one included): the two shapes of a row of blocks never share an answer"""
    N, ns = 8200, 70
    tiles = (N + TILE - 1) // TILE
    ysplit = min(ns, (CAP_BLOCKS + tiles - 1) // tiles)
    assert (tiles, ysplit) == (33, 63) and ns > ysplit
    alloc = np.tile(np.array([100, 8, 0], dtype=np.int64), (N, 1))
    gpus = list(range(37, N - 100, 100)) + [N - 5]                     # (the last one in the last tile, among its 8 nodes)
    alloc[gpus, 2] = 1
    assert len(gpus) == 82 and len({g // TILE for g in gpus}) >= tiles - 2 and gpus[-1] // TILE == tiles - 1
    pool = Pool(alloc)
    units, want = [], {}
    for i in range(ns):                                               # the i-th unit brings the i-th uniform shape: slot i
        if i % 2 == 0:
            units.append(pool.rows((10 + i, 500, 0), 2)); want[i] = (F, F, 0, -1)
        else:
            n = 82 if i % 4 == 1 else 83
            units.append(pool.rows((10 + i, 1, 1), n)); want[i] = (n <= 82, F, 82, 37)
    pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=ns, passes=1), want=want)


def test_c3_zero_request_and_negative_column(libs, oracle_lib, monkeypatch):
    """a shape with a zero in every column: every node's capacity is SG_CAP_CLAMP and num_schedulable the unit's size; a node whose free gpu column is negative (used
    above total at a low priority) under a zero gpu request counts 0 (nodematching.go:194-197) although it is first in key order, like a node with too little cpu left"""
    N = 260
    alloc = np.tile(np.array([100, 8, 0], dtype=np.int64), (N, 1))
    alloc[20] = (60, 8, 0)                                            # first in key order
    used = np.zeros((N, 3), dtype=np.int64)
    used[20, 2] = 1                                                   # gpu: 0 - 1
    used[258, 0] = 95                                                 # second tile: 5 cpu left
    for u in (None, used):
        pool = Pool(alloc, used=u)
        zero, one = pool.rows((0, 0, 0), 300), pool.rows((10, 1, 0), 8 * N + 1)
        two = [pool.rows((10, 1, 0))[0], pool.rows((20, 1, 0))[0]]
        cap = 8 * (N - 2) if u is not None else 8 * (N - 1) + 6
        first = 0 if u is not None else 20
        units = [zero[:2], zero, one[:cap - 1], one[:cap], one[:cap + 1], two]
        zfirst = 258 if u is not None else 20                         # (a zero request fits the node with 5 cpu left, and that one is first in key order)
        want = {0: (T, F, 2, zfirst), 1: (T, F, 300, zfirst), 2: (T, F, cap - 1, first), 3: (T, F, cap, first), 4: (F, F, cap, first), 5: (T, F, 2, first)}
        pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=6, passes=1 + 2), want=want)


@pytest.mark.parametrize("N", [1999, 2001])
def test_c3_the_references_schedule_many_benchmark_unit(libs, oracle_lib, monkeypatch, N):
    """BenchmarkScheduleMany* (nodedb_test.go:1590-1712): ONE unit of 64 000 one-cpu members on 32-cpu nodes, in the ABI's CSR form — 1999 nodes take 32 fewer, 2001 nodes 32 more"""
    J = 64000
    pool = Pool(np.tile(np.array([32, 256], dtype=np.int64), (N, 1)))
    pool.rows((1, 4), J)
    csr = (np.array([0, J], dtype=np.int32), np.arange(J, dtype=np.int32))
    pin(libs, oracle_lib, monkeypatch, pool, None, stats(gang=1, passes=1), csr=csr, want={0: (32 * N >= J, F, min(J, 32 * N), 0)})


# ---------------------------------------------------------------- D. one batch, every path
def test_d_one_batch_every_path(libs, oracle_lib, monkeypatch):
    """single jobs on the index grid (k_fit_batch) and off it (the literal first fit), uniform gangs (k_fit_capacity), gangs of two shapes (k_submit_gangs), gangs with a
    literal member and gangs of two priority classes (sequential), interleaved in one call: the unit <-> result mapping of every path and their shared scratch"""
    alloc = np.tile(np.array([100000, 8], dtype=np.int64), (300, 1))
    alloc[4] = (50000, 8)                                             # first in key order
    pool = Pool(alloc, cfg=config(2, res=1000, pcs=(0, 1)))
    units, strip, want = [], [], {}
    kinds = ("wide", "uniform", "literal", "gang", "gang_literal", "gang_two_pcs")
    for r in range(5):
        k = 1000 * r
        batch = {
            "wide": (pool.rows((2000 + k, 1 if r != 2 else 9)), (r != 2, F, int(r != 2), 4 if r != 2 else -1)),
            "literal": (pool.rows((1500 + k, 1)), (T, F, 1, 4)),
            "uniform": (pool.rows((60000, 1) if r == 3 else (3000 + k, 1), 3 + r), (T, F, 3 + r, 0 if r == 3 else 4)),
            "gang": ([pool.rows((2000 + k, 1))[0], pool.rows((3000 + k, 9 if r == 3 else 1))[0]], (r != 3, F, 1 if r == 3 else 2, 4)),
            "gang_literal": ([pool.rows((1500 + k, 1))[0], pool.rows((2000 + k, 1))[0]], (T, F, 2, 4)),
            "gang_two_pcs": ([pool.rows((2000 + k, 1), pc=0)[0], pool.rows((2000 + k, 1), pc=1)[0]], (T, F, 2, 4)),
        }
        for i in range(len(kinds)):
            kind = kinds[(i + r) % len(kinds)]
            want[len(units)] = batch[kind][1]
            units.append(batch[kind][0]); strip.append(kind in ("wide", "literal"))
    # node passes: one k_fit_batch launch, one literal index build, one capacity launch, the members of the five two-shape gangs
    expect = stats(wide=10, wide_passes=1, literal=5, gang=10, seq=10, passes=1 + 1 + 1 + 10)
    pin(libs, oracle_lib, monkeypatch, pool, units, expect, strip=strip, want=want)


# ---------------------------------------------------------------- E. the state of the handle
def resident_table(N):
    """cpu 100 + (37 i mod 11) — the key order is nothing like the row order —, 8 mem, every 50th node (from row 3) 64 mem; node.index 10, 20, ... leaves room in between"""
    alloc = np.stack([100 + (37 * np.arange(N)) % 11, np.full(N, 8)], axis=1).astype(np.int64)
    alloc[3::50, 1] = 64
    return alloc, 10 * (np.arange(N, dtype=np.int64) + 1)


def resident_jobs(pool):
    """rows for the probe units of `resident_units`"""
    j = {}
    j["g1"] = [pool.rows(r)[0] for r in ((10, 40), (10, 30), (1, 2), (1, 2), (1, 22))]
    a, b = pool.rows((60, 1), 20), pool.rows((50, 1), 20)
    j["g2"] = [x for pair in zip(a, b) for x in pair]
    a, b = pool.rows((110, 1), 20), pool.rows((110, 2), 20)
    j["g3"] = [x for pair in zip(a, b) for x in pair]
    j["u1"] = pool.rows((10, 40), 64)
    j["u2"] = pool.rows((110, 1), 64)
    j["u3"] = pool.rows((55, 1), 800)
    return j


def resident_units(j, alloc, schedulable=None):
    """units whose answers move with the table: the first-fit node, the nodes with 64 mem, the number of 110-cpu nodes (g3 fails at that member), the capacity sums"""
    nodes = [n for n in range(len(alloc)) if schedulable is None or schedulable[n]]
    c1, c2, c3 = capacity(alloc, (10, 40), nodes), capacity(alloc, (110, 1), nodes), capacity(alloc, (55, 1), nodes)
    assert 2 <= c1 < 63 and 2 <= c2 < 40 and c3 < 799
    units = [j["g1"], j["g2"], j["g3"], j["u1"][:c1], j["u1"][:c1 + 1], j["u2"][:c2 + 1], j["u3"][:c3], j["u3"][:c3 + 1], j["g3"][:c2], j["g3"][:c2 + 1]]
    want = {2: c2, 3: c1, 4: c1, 5: c2, 6: c3, 7: c3, 8: c2, 9: c2}                       # num_schedulable
    members = len(j["g1"]) + len(j["g2"]) + len(j["g3"]) + 2 * c2 + 1
    return units, want, stats(gang=10, passes=1 + members)


def resident_compare(libs, oracle, mp, before, op, after, schedulable=None):
    """a handle that held `before` (jobs set, cleared) and went through `op` against a FRESH handle of `after` and the oracle: answers and counters"""
    lib, cpu = libs
    j = resident_jobs(after)
    before.req, before.pc, before.cls = after.req, after.pc, after.cls
    units, want, expect = resident_units(j, after.alloc, schedulable)
    strip = [False] * len(units)
    o = after.handle(oracle)
    ref = o.submit_check(units, strip)
    o.close()
    for u, n in want.items():
        assert ref[u][2] == n, (u, ref[u], n)
    fresh = after.handle(lib)
    f_got, f_st, _, _ = ask(fresh, units, strip, mp)
    fresh.close()
    s = before.handle(lib)
    old = s.submit_check(units, strip)
    op(s)
    got, st, seq, st0 = ask(s, units, strip, mp)
    s.close()
    assert f_got == ref and f_st == expect, (diff(units, f_got, ref), f_st, expect)
    assert got == ref, diff(units, got, ref)
    assert st == f_st and seq == ref and st0["gang_units"] == 0 and st0["sequential_units"] == len(units)
    if cpu is not None:
        c = before.handle(cpu)
        op(c)
        assert c.submit_check(units, strip) == got
        c.close()
    return old, ref


def test_e_after_nodes_append(libs, oracle_lib, monkeypatch):
    """250 -> 262 nodes: N crosses a tile, the 256-thread stride and a 64-node mask word; the new rows' node.index lies BETWEEN resident ones (nodeByRank changes on both
    sides) and they bring a new first-fit node, a node with 64 mem in front of the old ones and two 110-cpu nodes"""
    alloc, index = resident_table(250)
    new = np.array([[99, 8], [100, 64], [110, 8], [110, 8]] + [[104, 8]] * 8, dtype=np.int64)
    new_index = np.array([15, 25, 1205, 1215] + [2005 + 10 * i for i in range(8)], dtype=np.int64)
    before = Pool(alloc, index=index)
    after = Pool(np.concatenate([alloc, new]), index=np.concatenate([index, new_index]))
    old, ref = resident_compare(libs, oracle_lib, monkeypatch, before, lambda s: s.nodes_append(new, index=new_index), after)
    assert (ref[1][3], ref[0][3]) == (250, 251) and old[1][3] != 250 and old[0][3] != 251 and ref[2][2] == old[2][2] + 2


def test_e_after_nodes_delete(libs, oracle_lib, monkeypatch):
    """262 -> 250 nodes: N drops below a tile and a mask word edge; the deleted rows include the first-fit node of every probe unit and one with 64 mem"""
    alloc, index = resident_table(262)
    first = int(np.lexsort((index, alloc[:, 0]))[0])
    rows = sorted({first, 3, 10, 63, 64, 128, 200, 255, 256, 257, 260, 261})
    assert len(rows) == 12
    before = Pool(alloc, index=index)
    after = Pool(np.delete(alloc, rows, axis=0), index=np.delete(index, rows))
    old, ref = resident_compare(libs, oracle_lib, monkeypatch, before, lambda s: s.nodes_delete(rows), after)
    assert old[1][3] == first and old != ref


def test_e_after_nodes_patch(libs, oracle_lib, monkeypatch):
    """a cordon of the first-fit node and of a node with 64 mem, and three 110-cpu nodes cut to 100 cpu: g3 fails at an earlier member"""
    alloc, index = resident_table(300)
    first = int(np.lexsort((index, alloc[:, 0]))[0])
    big = [int(n) for n in np.nonzero(alloc[:, 0] == 110)[0][:3]]
    patched = alloc.copy()
    patched[big, 0] = 100
    uns = np.zeros(300, dtype=np.uint8)
    uns[[first, 53]] = 1
    before = Pool(alloc, index=index)
    after = Pool(patched, index=index, unschedulable=uns)

    def op(s):
        s.nodes_patch([first, 53], unschedulable=1)
        s.nodes_patch(big, allocatable=patched[big])
    old, ref = resident_compare(libs, oracle_lib, monkeypatch, before, op, after, schedulable=1 - uns)
    assert old[1][3] == first and ref[1][3] != first and old[2][2] == ref[2][2] + 3


def test_e_after_a_round_and_clear_allocated(libs, oracle_lib, monkeypatch):
    """a handle that has scheduled a round (jobs bound, evicted, preempted) and was cleared answers as a fresh, cleared handle of the same tables.  The units' jobs are
    held back from the round's queues: binding a job that already holds resources is an error in the reference (node.go:416-442), not an answer."""
    lib, cpu = libs
    wl = W.small_random(n_nodes=300, n_jobs=500, n_queues=3, seed=41, occupied=0.5, gangs=0)
    queued = np.nonzero(wl.job_node < 0)[0]
    shape = {}
    for i in queued:
        shape.setdefault((tuple(wl.job_req[i]), int(wl.job_pc[i])), []).append(int(i))
    uniform = [v[:n] for v, n in zip([v for v in shape.values() if len(v) >= 6], (2, 3, 6, 6, 5, 4))]
    rng = np.random.default_rng(5)
    mixed = []
    for n in (2, 3, 9, 40):
        pc = int(rng.integers(0, 2))
        cand = [int(i) for i in queued if wl.job_pc[i] == pc]
        u = [int(x) for x in rng.choice(cand, size=n, replace=False)]
        if len({tuple(wl.job_req[i]) for i in u}) > 1:
            mixed.append(u)
    units = [x for pair in zip(uniform, mixed) for x in pair] + uniform[len(mixed):]
    assert len(uniform) >= 4 and len(mixed) >= 3
    strip = [False] * len(units)
    expect = stats(gang=len(units), passes=1 + sum(len(u) for u in mixed))
    held = np.array(sorted({j for u in units for j in u}))
    wl.queued = [q[~np.isin(q, held)] for q in wl.queued]
    out = []
    for l in (oracle_lib, lib) + ((cpu,) if cpu is not None else ()):
        f = W.load(l, wl)
        f.clear_allocated()
        ref, f_st, _, _ = ask(f, units, strip, monkeypatch)
        f.close()
        s = W.load(l, wl)
        W.prepare(s, wl)
        res = s.schedule_round()
        assert len(res.scheduled) > 0
        s.clear_allocated()
        got, st, seq, st0 = ask(s, units, strip, monkeypatch)
        s.close()
        assert got == ref == seq
        if l is not oracle_lib:
            assert st == f_st == expect, (st, f_st, expect)
            assert st0["gang_units"] == 0 and st0["sequential_units"] == len(units)
        out.append(got)
    assert all(o == out[0] for o in out)
    assert any(o[0] for o in out[0])


def test_e_used_nodes_at_a_low_priority(libs, oracle_lib, monkeypatch):
    """resources used at priority 0 lower the planes of every level up to the units' own alike (pristineUpTo): units of priority class 0 take both kernels and see the
    lowered planes; the same units of priority class 1 (whose own level is untouched, but whose first attempt is at the lowest one) are answered sequentially.  Every answer of the
    first kind differs from the empty pool's."""
    N = 300
    alloc, index = resident_table(N)
    first = int(np.lexsort((index, alloc[:, 0]))[0])
    used = np.zeros((N, 2), dtype=np.int64)
    used[first] = (95, 0)                                             # the first-fit node: 5 cpu left
    used[3::50, 1] = 30                                               # the nodes with 64 mem: 34 left
    used[np.nonzero(alloc[:, 0] == 110)[0][:5], 0] = 1                # five of the 110-cpu nodes: 109
    res = {}
    for u in (None, used):
        pool = Pool(alloc, index=index, cfg=config(2, pcs=(0, 1)), used=u, clear=False)
        units = []
        for pc in (0, 1):
            g = [pool.rows(r, pc=pc)[0] for r in ((10, 40), (10, 30), (1, 2), (1, 2))]
            a, b = pool.rows((110, 1), 20, pc=pc), pool.rows((110, 2), 20, pc=pc)
            units += [g, [x for pair in zip(a, b) for x in pair], pool.rows((10, 40), 8, pc=pc), pool.rows((110, 1), 30, pc=pc)]
        if u is None:
            expect = stats(gang=8, passes=2 * (1 + 4 + 40) - 1)        # (one capacity launch for both priority classes' shapes)
        else:
            expect = stats(gang=4, seq=4, passes=1 + 4 + 40)
        res[u is None] = pin(libs, oracle_lib, monkeypatch, pool, units, expect)
    assert all(a != b for a, b in zip(res[False][:4], res[True][:4]))


def test_e_two_word_key(libs, oracle_lib, monkeypatch):
    """a handle whose order key takes two words (forced: ASCHED_KEY_WORDS=2) serves no gang unit on either kernel, and answers the same"""
    pool, units, want = stride_pool(300, 299, "last")
    rows = pool.rows((10, 1), 5)
    units = units + [rows]
    one = pin(libs, oracle_lib, monkeypatch, pool, units, stats(gang=3, passes=11), want=want)
    monkeypatch.setenv("ASCHED_KEY_WORDS", "2")
    two = pin(libs, oracle_lib, monkeypatch, pool, units, stats(seq=3), want=want)
    assert one == two


# ---------------------------------------------------------------- F. a small seeded sweep
SWEEP_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
SIZES = (1, 2, 3, 5, 8, 17, 40, 120, 255, 256, 257, 300)


def sweep_case(seed):
    rng = np.random.default_rng(7000 + seed)
    N = int(rng.integers(200, 701))
    alloc = np.stack([rng.choice([16, 32, 64, 96], size=N), rng.choice([32, 64, 128], size=N)], axis=1).astype(np.int64)
    pool = Pool(alloc)
    shapes = [(1, 1), (2, 8), (4, 4), (8, 32), (16, 16), (32, 64), (48, 8), (96, 200), (128, 128), (24, 100)]
    per = [pool.rows(s, 300) for s in shapes]
    units, strip = [], []
    for _ in range(36):
        n = int(rng.choice(SIZES))
        if n > 1 and rng.random() < 0.45:
            u = per[int(rng.integers(0, len(shapes)))][:n]
        else:
            small = rng.random() < 0.35                               # big members: gangs run out of nodes half way
            cand = np.concatenate([per[i] for i in (range(0, 5) if small else range(3, 10))])
            u = [int(x) for x in rng.choice(cand, size=n, replace=False)]
        units.append(u); strip.append(n == 1)
    return pool, units, strip


def sweep_expect(pool, units):
    """the path of every unit, from the requests alone"""
    wide = uniform = gangs = members = seq = 0
    single_shapes = set()
    for u in units:
        kinds = {pool.req[j] for j in u}
        if len(u) == 1:
            wide += 1; single_shapes |= kinds
        elif len(kinds) == 1:
            uniform += 1
        elif len(u) <= SG_TMAX:
            gangs += 1; members += len(u)
        else:
            seq += 1
    return stats(wide=wide, wide_passes=int(wide > 0), gang=uniform + gangs, seq=seq, passes=int(wide > 0) + int(uniform > 0) + members), uniform, gangs


def test_f_seeded_sweep(libs, oracle_lib, monkeypatch):
    multi = ok = partial = uni = wg = 0
    for seed in SWEEP_SEEDS:
        pool, units, strip = sweep_case(seed)
        expect, uniform, gangs = sweep_expect(pool, units)
        ref = pin(libs, oracle_lib, monkeypatch, pool, units, expect, strip=strip)
        m = [(u, r) for u, r in zip(units, ref) if len(u) > 1]
        multi += len(m); ok += sum(1 for u, r in m if r[0]); partial += sum(1 for u, r in m if not r[0] and 0 < r[2] < len(u))
        uni += uniform; wg += gangs
    assert 3 * ok >= multi and 10 * partial >= multi and uni > 20 and wg > 20, (multi, ok, partial, uni, wg)
