"""Seeded interleavings of the resident table calls (test infrastructure: tests/test_z_resident_sequences.py and `tests/soak.py resident`).

The model is a workloads.Workload, `cur`: what a caller would hand to nodes_upsert plus jobs_set to reach the state the handle under test is in.  It carries, beside
the Workload's fields, qprio (the queue priority of every row), held (rows in a terminal state that were not deleted yet: no run, in no queued list), unsched (the
cordon flag of every node) and class_affinities.  Every operation edits `cur` in plain numpy and issues the matching call on the handle; after every operation the
handle is compared with a fresh handle of `cur` on the same library and with the oracle's round (tests/test_z_shapes_compact.py _same's comparison: scheduling order,
every row's first fit at every priority level, the node types matching the last rows, a submit check, the round, the unfeasible keys, fair shares bit for bit, the
number of fast iterations), and every call's statistics are recorded, so that a replay on another library has to take the same path.
(_same itself prepares every round from explicit lists and builds its fresh handle on the spot; here the preparation varies per check and a replay compares with
recordings, so the comparison is restated in _answers / _compare from the same parts: _view, _round, _set_jobs, scenario.assert_same_round.)

The operations are drawn with numpy.random.default_rng(seed) among those applicable to the current state; a drawn one is never skipped.  A job whose run ended — it
finished or was preempted — is in a terminal state: it stays as a held row until a jobs_delete names it, as INTEGRATION.md describes the cycle.

The view (the NodeDb-level queries and the submit check) is only ever taken when the last successful call on the handle was a resident call or jobs_set, never
directly after a round: a round leaves its placements bound, and round_prepare binds the running jobs, until the next resident call ("Queries after a
round").  A refusal is
therefore drawn as a rider of a check: the view, the refused call, the view again, and only then the round."""
import copy

import numpy as np

import scenario
import test_z_jobs_delete as JD
import test_z_req_classes_append as rc
import test_z_shapes_compact as SC
from armada_amd import workloads as W
from armada_amd.binding import SchedError, Scheduler
from test_z_jobs_append import _append_tail, _round, _shape_keys
from test_z_jobs_append_shapes import _extend, _view
from test_z_jobs_reprioritise import _limits, _restated_queued

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
Gi, CPU, MEM = W.Gi, W.CPU, W.MEM
START_NODES = (3, 40, 63, 64, 65, 100, 128, 130)
OPS = ("jobs_append", "jobs_delete", "apply_round", "jobs_reprioritise", "req_classes_append", "shapes_compact", "nodes_patch", "nodes_delete", "nodes_append")
REFUSALS = ("nodes_delete of a node with a run", "jobs_delete of every row", "row out of range")
REFUSAL_RATE = 0.08
TAINT9 = (9, 1, 1)
# (tolerations, selector, affinity): classes some nodes satisfy and some do not (tests/test_z_req_classes_append.py)
NEW_CLASSES = (rc.ONE_TYPE, rc.OPENS, rc.PLAIN, rc.NON_INDEXED, rc.AFF_IN, rc.AFF_NOT_IN, rc.AFF_GT, rc.AFF_LT_OR)
MAX_CLASSES = 12


class SequenceFailure(AssertionError):
    pass


class Step:
    """one operation of a sequence: what was called, its statistics, the table's size after it, and what the handle answered"""
    def __init__(self, op, detail, stats, cur):
        self.op, self.detail, self.stats, self.M, self.N = op, detail, stats, cur.num_jobs, cur.num_nodes
        self.refusal = None          # (kind, error code) of the refusal that rode on this step's check
        self.answers = None          # (view, round, unfeasible keys of the last rows)
        self.fast_iterations = None
        self.resident = None         # the round of the check was prepared with round_prepare_resident

    def line(self):
        ref = f" refused[{self.refusal[0]}: {self.refusal[1]}]" if self.refusal else ""
        return f"{self.op}({self.detail}) {self.stats} -> M={self.M} N={self.N}{ref}"


# ---------------------------------------------------------------- the model
def start_table(seed, rng):
    """tests/test_z_req_classes_append.py _tbl's node types and classes on a table of a seeded size: 5 ... 200 rows, the node count from START_NODES"""
    n = int(rng.choice(START_NODES))
    m = int(rng.integers(5, 201))
    wl = W.small_random(n_nodes=n, n_jobs=max(m * 2 // 3, 5), n_queues=int(rng.integers(1, 5)), seed=seed, occupied=float(rng.choice([0.0, 0.3, 0.6, 0.9])), gangs=int(rng.integers(0, 3)))
    if wl.num_jobs > m:              # (the running rows of a crowded table alone are more than that)
        wl, _ = JD._reduced_wl(wl, rng.permutation(wl.num_jobs)[: wl.num_jobs - m])
    wl.config.indexed_label_keys = [3]
    wl.node_labels = [[(3, i % 3), (5, i % 2), (6, 100 + i % 4)] for i in range(n)]
    wl.node_taints = [[TAINT9] if i % 4 == 0 else [] for i in range(n)]
    cls = rng.choice(2, size=wl.num_jobs, p=[0.7, 0.3]).astype(np.int32)
    cls[np.asarray(wl.job_node) >= 0] = 0
    cls[np.asarray(wl.job_gang) >= 0] = 0
    wl.job_req_class = cls
    wl.class_tolerations = [[rc.EXISTS9], [rc.EXISTS9]]
    wl.class_selectors = [[], [(3, 1)]]
    wl.class_affinities = None
    wl.type_override = None
    wl.qprio = np.zeros(wl.num_jobs, np.uint32)
    wl.held = np.zeros(wl.num_jobs, bool)
    wl.unsched = np.zeros(n, np.uint8)
    return _requeued(wl)


def _requeued(cur):
    """the queued lists of the model: every row without a run that is not held, in the restated order (priority class, queue priority, submit time, id)"""
    ids = np.nonzero((np.asarray(cur.job_node) < 0) & ~cur.held)[0]
    pcp = np.asarray(cur.config.pc_priority)[cur.job_pc]
    cur.queued = W._sort_queued(cur.job_queue, pcp, cur.job_submit, ids) if len(ids) else []
    cur.queued = [np.asarray(q, np.int32) for q in cur.queued][: cur.num_queues]
    while len(cur.queued) < cur.num_queues:
        cur.queued.append(np.zeros(0, np.int32))
    cur.queued = _restated_queued(cur, cur.qprio)
    return cur


def fresh(L, cur):
    """what a caller would do to reach `cur` from nothing (tests/test_z_shapes_compact.py _ld, with the cordon flags)"""
    s = Scheduler(L, cur.config)
    s.set_label_value_ints(rc.INTS)
    s.nodes_upsert(cur.node_total, cur.node_allocatable, taints=cur.node_taints, labels=cur.node_labels, unschedulable=cur.unsched)
    SC._set_jobs(s, cur)
    return s


def _gang_rows(cur):
    return JD._gangs_of(cur)


# ---------------------------------------------------------------- the operations: each edits a copy of `cur`, issues the call and returns (cur, detail, statistics)
def _op_jobs_append(a, cur, rng, st):
    m0, k = cur.num_jobs, int(rng.integers(1, 41))
    ncls = len(cur.class_tolerations)
    req, fresh_left = [], 3
    for _ in range(k):
        x = rng.random()
        if x < 0.4:
            req.append(cur.job_req[int(rng.integers(0, m0))])
        elif x < 0.8 and st["new_reqs"] > 0 or fresh_left == 0:      # a vector an earlier append brought: its shape may be alive, dead or retired by now
            req.append(SC._new_reqs(1, int(rng.integers(0, max(st["new_reqs"], 1))))[0])
        else:                                                        # a vector the table has never had
            req.append(SC._new_reqs(1, st["new_reqs"])[0])
            st["new_reqs"] += 1
            fresh_left -= 1
    req = np.array(req, dtype=np.int64)
    pc = rng.integers(0, len(cur.config.pc_priority), size=k).astype(np.int32)
    queue = rng.integers(0, cur.num_queues, size=k).astype(np.int32)
    cls = rng.integers(0, ncls, size=k).astype(np.int32)
    gang, card = np.full(k, -1, np.int32), np.ones(k, np.int32)
    i, n_gangs = 0, 0
    while i + 1 < k:                                                 # some appends bring whole new gangs: consecutive rows of one queue, shape and priority class
        if rng.random() < 0.12:
            c = int(rng.integers(2, min(6, k - i) + 1))
            sl = slice(i, i + c)
            req[sl], pc[sl], queue[sl], cls[sl], gang[sl], card[sl] = req[i], pc[i], queue[i], cls[i], st["next_gang"], c
            st["next_gang"] += 1
            n_gangs += 1
            i += c
        else:
            i += 1
    full, tail = _extend(cur, req, pc=pc, cls=cls, queue=queue, gang=gang, card=card)
    full.job_submit = full.job_submit.copy()
    full.job_submit[tail] = st["next_submit"] + np.arange(k)         # behind every row the table ever had
    st["next_submit"] += k
    full.qprio = np.concatenate([cur.qprio, np.zeros(k, np.uint32)])
    full.held = np.concatenate([cur.held, np.zeros(k, bool)])
    _requeued(full)
    in_place = bool(rng.random() < 0.6)
    a.set_append_in_place(in_place)
    js = _append_tail(a, full, tail)
    sh = a.jobs_append_shape_stats()
    assert js["rows"] == k and js["new_gangs"] == n_gangs, js
    grew = js["capacity"] > st["job_cap"]
    stats = dict(rebuilt=js["rebuilt"], in_place=js["in_place"], reason=sh["reason"], added=sh["added"], revived=sh["revived"], new_shapes=js["new_shapes"],
                 reallocated=js["reallocated"], capacity=js["capacity"], grew=int(grew), after_halving=int(grew and st["halved"]))
    if grew:
        st["job_cap"], st["halved"] = js["capacity"], False
    return full, f"{k} rows, {n_gangs} gangs, switch {int(in_place)}", stats


def _op_jobs_delete(a, cur, rng, st):
    m = cur.num_jobs
    most = max(1, m // 2)
    how = str(rng.choice(["random", "first and last", "a shape", "a gang", "part of a gang", "held"]))
    must = []
    if how == "first and last":
        must = [0, m - 1]
    elif how == "a shape":                                           # every row of one shape: the shape dies
        keys = _shape_keys(cur, range(m))
        k0 = keys[int(rng.integers(0, m))]
        must = [j for j, k in enumerate(keys) if k == k0]
    elif how in ("a gang", "part of a gang"):
        gangs = sorted(_gang_rows(cur).items())
        if gangs:
            rows = gangs[int(rng.integers(0, len(gangs)))][1]
            must = rows if how == "a gang" else rows[: max(1, len(rows) // 2)]
    elif how == "held":
        must = [int(j) for j in np.nonzero(cur.held)[0]]
    must = sorted(set(must))[:most]
    rest = np.setdiff1d(np.arange(m), must)
    room = most - len(must)
    extra = room if rng.random() < 0.3 else int(rng.integers(0, room + 1))      # (three deletes in ten take half the table)
    if not must and extra == 0:
        extra = 1
    rows = np.sort(np.concatenate([np.asarray(must, np.int64), rng.permutation(rest)[:extra]])).astype(np.int32)
    assert 1 <= len(rows) <= most and len(rows) < m
    w, _ = JD._reduced_wl(cur, rows)
    keep = np.ones(m, bool)
    keep[rows] = False
    w.qprio, w.held = cur.qprio[keep], cur.held[keep]
    _requeued(w)
    a.jobs_delete(rows)
    ds = a.jobs_delete_stats()
    assert ds["rows"] == len(rows) and ds["num_jobs"] == w.num_jobs, ds
    st["job_cap"] = max(st["job_cap"], ds["capacity"])
    if 2 * w.num_jobs <= st["job_cap"]:
        st["halved"] = True
    return w, f"{len(rows)} rows, {how}", dict(gangs_emptied=ds["gangs_emptied"], shapes_emptied=ds["shapes_emptied"], capacity=ds["capacity"], halved=int(st["halved"]))


def _can_apply(cur, last):
    return last is not None and (len(last.scheduled) + len(last.preempted) + int((np.asarray(cur.job_node) >= 0).sum()) // 5) > 0


def _op_apply_round(a, cur, rng, st):
    """the last round's result becomes the table's state: scheduled rows run, preempted rows lose their run, a seeded fifth of the running rows finishes"""
    r = st["last_round"]
    w = copy.copy(cur)
    w.job_node, w.job_run_prio, w.job_run_ts, w.held = cur.job_node.copy(), cur.job_run_prio.copy(), cur.job_run_ts.copy(), cur.held.copy()
    st["ts"] += 1_000_000_000
    rows = set()
    for j, n in r.scheduled.items():
        w.job_node[j], w.job_run_prio[j], w.job_run_ts[j] = n, r.scheduled_priority[j], st["ts"]
        rows.add(int(j))
    for j in r.preempted:
        w.job_node[j], w.job_run_prio[j], w.job_run_ts[j], w.held[j] = -1, 0, 0, True
        rows.add(int(j))
    run = np.nonzero(w.job_node >= 0)[0]
    fin = rng.permutation(run)[: len(run) // 5]
    w.job_node[fin], w.job_run_prio[fin], w.job_run_ts[fin], w.held[fin] = -1, 0, 0, True
    rows |= set(int(j) for j in fin)
    rows = np.array(sorted(rows), dtype=np.int32)
    assert len(rows)
    _requeued(w)
    a.jobs_patch(rows, w.job_node[rows], w.job_run_prio[rows], w.job_run_ts[rows])
    return w, f"{len(r.scheduled)} scheduled, {len(r.preempted)} preempted, {len(fin)} finished", {}


def _op_jobs_reprioritise(a, cur, rng, st):
    m = cur.num_jobs
    k = int(rng.integers(1, max(2, m // 3)))
    named = set(int(j) for j in rng.permutation(m)[:k])
    w = copy.copy(cur)
    w.qprio = cur.qprio.copy()
    prio = rng.integers(0, 5, size=m).astype(np.uint32)
    gangs = _gang_rows(cur)
    for rows in gangs.values():                                      # a gang moves as a whole and to one priority: its members stay adjacent in their queue
        if named & set(rows):
            named |= set(rows)
            prio[rows] = prio[rows[0]]
    named = np.array(sorted(named), dtype=np.int32)
    w.qprio[named] = prio[named]
    _requeued(w)
    a.jobs_reprioritise(named, w.qprio[named])
    rs = a.jobs_reprioritise_stats()
    assert rs["entries"] == len(named), rs
    running = int((np.asarray(cur.job_node)[named] >= 0).sum())
    return w, f"{len(named)} rows, {running} running", dict(in_order=rs["in_order"], unchanged=rs["unchanged"], made_resident=rs["made_resident"])


def _op_req_classes_append(a, cur, rng, st):
    cl = NEW_CLASSES[int(rng.integers(0, len(NEW_CLASSES)))]
    first = len(cur.class_tolerations)
    w = rc._with_classes(cur, [cl])
    got = a.req_classes_append([cl[0]], [cl[1]], [cl[2]])
    cs = a.req_classes_append_stats()
    assert got == first and cs["added"] == 1 and cs["classes"] == first + 1, (got, cs)
    return w, f"class {first}", dict(by_type=cs["by_type"], on_host=cs["on_host"], moved=cs["moved"], rebuilt=cs["rebuilt"], reason=cs["reason"])


def _op_shapes_compact(a, cur, rng, st):
    classes = bool(rng.random() < 0.5)
    cmap = a.shapes_compact(classes=classes, want_map=classes)
    cs = a.shapes_compact_stats()
    w = cur
    if classes:                                                      # the class map is applied to the model, as simulator_input.run_cycles_retiring applies it
        assert cmap is not None and int((cmap < 0).sum()) == cs["classes_retired"], (cmap, cs)
        w = SC._reduced(cur, cmap)
    return w, f"classes {int(classes)}", dict(shapes_retired=cs["shapes_retired"], fit_retired=cs["fit_retired"], classes_retired=cs["classes_retired"], rebuilt=cs["rebuilt"],
                                             reason=cs["reason"], shapes=cs["shapes"], fit_shapes=cs["fit_shapes"])


def _tolerates9(cur, c):
    return len(cur.class_tolerations[c]) > 0                         # (every toleration of this module's classes is one of key 9)


def _op_nodes_patch(a, cur, rng, st):
    n = cur.num_nodes
    k = int(rng.integers(1, min(n, 12) + 1))
    rows = np.sort(rng.permutation(n)[:k]).astype(np.int32)
    how = str(rng.choice(["cordon", "capacity", "taint"]))
    w = copy.copy(cur)
    if how == "cordon":                                              # cordon or uncordon
        w.unsched = cur.unsched.copy()
        w.unsched[rows] = rng.integers(0, 2, size=k).astype(np.uint8)
        a.nodes_patch(rows, unschedulable=w.unsched[rows])
    elif how == "capacity":                                          # allocatable below total by whole index units, or back at total
        w.node_allocatable = (cur.node_total if cur.node_allocatable is None else cur.node_allocatable).copy()
        cut = np.zeros_like(w.node_total[rows])
        cut[:, CPU] = rng.integers(0, 9, size=k) * 1000
        cut[:, MEM] = rng.integers(0, 33, size=k) * Gi
        w.node_allocatable[rows] = np.maximum(w.node_total[rows] - cut, 0)
        a.nodes_patch(rows, allocatable=w.node_allocatable[rows])
    else:                                                            # the taint the classes read; a node keeps it open where a run of a class without the toleration sits
        w.node_taints = [list(t) for t in cur.node_taints]
        for i in rows:
            closed = [j for j in np.nonzero(np.asarray(cur.job_node) == i)[0] if not _tolerates9(cur, int(cur.job_req_class[j]))]
            w.node_taints[i] = [] if (cur.node_taints[i] or closed) else [TAINT9]
        a.nodes_patch(rows, taints=[w.node_taints[i] for i in rows])
    ps = a.nodes_patch_stats()
    assert ps[0] == k, ps
    return w, f"{how}, {k} rows", dict(type_changed=ps[1], rebuilt=ps[2], reason=ps[3])


def _free_nodes(cur):
    used = np.zeros(cur.num_nodes, bool)
    used[np.asarray(cur.job_node)[np.asarray(cur.job_node) >= 0]] = True
    return np.nonzero(~used)[0]


def _op_nodes_delete(a, cur, rng, st):
    n = cur.num_nodes
    free = _free_nodes(cur)
    most = min(len(free), n - 1)
    k = most if rng.random() < 0.25 else int(rng.integers(1, most + 1))          # (a delete in four drops every node it may drop)
    rows = np.sort(rng.permutation(free)[:k]).astype(np.int32)
    keep = np.ones(n, bool)
    keep[rows] = False
    new_of = np.cumsum(keep).astype(np.int32) - 1
    w = copy.copy(cur)
    w.node_total = cur.node_total[keep]
    w.node_allocatable = None if cur.node_allocatable is None else cur.node_allocatable[keep]
    w.node_taints = [t for t, x in zip(cur.node_taints, keep) if x]
    w.node_labels = [t for t, x in zip(cur.node_labels, keep) if x]
    w.unsched = cur.unsched[keep]
    w.job_node = np.where(cur.job_node >= 0, new_of[np.maximum(cur.job_node, 0)], -1).astype(np.int32)
    a.nodes_delete(rows)
    ds = a.nodes_delete_stats()
    assert ds[0] == k and ds[4] == n - k, ds
    return w, f"{k} rows", dict(renumbered=ds[1], rebuilt=ds[2], reason=ds[3], n_before=n)


def _op_nodes_append(a, cur, rng, st):
    n, k = cur.num_nodes, int(rng.integers(1, 71))
    src = rng.integers(0, n, size=k)
    w = copy.copy(cur)
    w.node_total = np.concatenate([cur.node_total, cur.node_total[src]])
    if cur.node_allocatable is not None:
        w.node_allocatable = np.concatenate([cur.node_allocatable, cur.node_total[src]])
    w.node_taints = list(cur.node_taints) + [list(cur.node_taints[i]) for i in src]
    w.node_labels = list(cur.node_labels) + [list(cur.node_labels[i]) for i in src]
    w.unsched = np.concatenate([cur.unsched, np.zeros(k, np.uint8)])
    a.nodes_append(w.node_total[n:], index=st["next_index"] + np.arange(k), taints=w.node_taints[n:], labels=w.node_labels[n:])
    st["next_index"] += k
    ns = a.nodes_append_stats()
    assert ns[0] == k and ns[4] == n + k, ns
    return w, f"{k} rows", dict(restrided=ns[1], rebuilt=ns[2], reason=ns[3], n_before=n)


_RUN = dict(jobs_append=_op_jobs_append, jobs_delete=_op_jobs_delete, apply_round=_op_apply_round, jobs_reprioritise=_op_jobs_reprioritise,
            req_classes_append=_op_req_classes_append, shapes_compact=_op_shapes_compact, nodes_patch=_op_nodes_patch, nodes_delete=_op_nodes_delete,
            nodes_append=_op_nodes_append)


def _draw(cur, rng, st, step, max_steps):
    """an operation among those applicable to the current state.  The tide of a seed — first out, then in, or the other way round — takes the tables below half their
    size and then past every capacity they had, and the node count across the word edges in both directions"""
    out = (step < st["turn"]) == st["out_first"]
    wt = dict(jobs_append=1.5 if out else 3.0, jobs_delete=3.0 if out else 1.0, apply_round=1.5, jobs_reprioritise=1.2, req_classes_append=1.0, shapes_compact=1.5,
              nodes_patch=1.5, nodes_delete=3.0 if out else 0.7, nodes_append=0.7 if out else 2.5)
    if cur.num_jobs < 2:
        del wt["jobs_delete"]
    if not _can_apply(cur, st["last_round"]):
        del wt["apply_round"]
    if len(cur.class_tolerations) >= MAX_CLASSES:
        del wt["req_classes_append"]
    if cur.num_nodes < 2 or len(_free_nodes(cur)) == 0:
        del wt["nodes_delete"]
    if cur.num_nodes > 400:
        del wt["nodes_append"]
    names = [o for o in OPS if o in wt]
    p = np.array([wt[o] for o in names])
    return names[int(rng.choice(len(names), p=p / p.sum()))]


# ---------------------------------------------------------------- refusals
def _refuse(a, cur, rng):
    """a call the library must refuse, drawn among those the state allows -> (kind, the error code it gave, the code its documentation names)"""
    kinds = [k for k in REFUSALS if k != REFUSALS[0] or (cur.num_nodes > 1 and (np.asarray(cur.job_node) >= 0).any())]      # (the only node named is "every row": another refusal)
    kind = kinds[int(rng.integers(0, len(kinds)))]
    m, n = cur.num_jobs, cur.num_nodes
    try:
        if kind == REFUSALS[0]:
            run = np.asarray(cur.job_node)[np.asarray(cur.job_node) >= 0]
            want = ERR_INVALID
            a.nodes_delete([int(run[int(rng.integers(0, len(run)))])])
        elif kind == REFUSALS[1]:
            want = ERR_UNSUPPORTED
            a.jobs_delete(np.arange(m, dtype=np.int32))
        else:
            want = ERR_INVALID
            bad = int(rng.choice([m, -1]))
            which = int(rng.integers(0, 4))
            if which == 0:
                a.jobs_delete([0, bad] if m > 1 and bad > 0 else [bad])
            elif which == 1:
                a.jobs_patch([bad], [-1], 0, 0)
            elif which == 2:
                a.jobs_reprioritise([bad], 1)
            else:
                a.nodes_delete([n])
    except SchedError as e:
        return kind, e.code, want
    return kind, 0, want


# ---------------------------------------------------------------- what a handle answers
def _answers(s, cur, tail, resident, rider=None):
    """the view first (the last call was a resident call or jobs_set), then the round: prepared from the resident order with the held rows, or from explicit lists"""
    v = _view(s, cur, tail)
    if rider is not None:
        rider(v)
    if resident:
        s.round_prepare_resident(cur.queue_weight, held=np.nonzero(cur.held)[0].astype(np.int32), **_limits(cur))
        got = s.round_queued()
        assert [x.tolist() for x in got] == [np.asarray(x).tolist() for x in cur.queued], "round_queued after round_prepare_resident is not the model's queued order"
        r, st = s.schedule_round(), s.round_stats()
    else:
        r, st = _round(s, cur)
    return v, r, st, [s.job_key_unfeasible(int(j)) for j in tail]


def _compare(got, want, what):
    (v, r, u), (v0, r0, u0) = got, want
    assert v == v0, f"the view differs from {what}"
    scenario.assert_same_round(r0, r)
    assert u == u0, f"the unfeasible keys differ from {what}"
    assert r.fair_share.tobytes() == r0.fair_share.tobytes(), f"fair shares differ from {what}"


def _against_fresh(L, cur, tail, resident, got, fast):
    f = fresh(L, cur)
    vf, rf, stf, uf = _answers(f, cur, tail, resident)
    f.close()
    _compare(got, (vf, rf, uf), "the fresh handle's")
    assert fast == stf["fast_iterations"], "the handle did not run the fresh handle's fast iterations"


def _against_oracle(oracle, cur, r):
    o = fresh(oracle, cur)
    ro, _ = _round(o, cur)
    o.close()
    scenario.assert_same_round(ro, r)
    assert r.fair_share.tobytes() == ro.fair_share.tobytes(), "fair shares differ from the oracle's"


def _rebuilt(step):
    return bool(step.stats.get("rebuilt"))


# ---------------------------------------------------------------- the runner
def run_sequence(L, oracle, seed, max_steps=40, recorded=None):
    """one seeded sequence of at most max_steps operations on library L -> the list of Steps (the first is the load).

    recorded None: after every operation the handle is compared with a fresh handle of the model on L and with the oracle's round.
    recorded (the Steps of the same seed on another library, at least as long): after every operation the handle's answers and its call's statistics must equal the
    recorded ones, and the handle is compared with a fresh handle on L at three points only — after the first rebuild, at the middle and at the end.
    A failure raises SequenceFailure with the seed, the step, the operations so far with their statistics, M and N; max_steps cuts a failing seed to a prefix."""
    rng = np.random.default_rng(seed)
    cur = start_table(seed, rng)
    st = dict(new_reqs=0, next_gang=10_000, next_submit=int(cur.job_submit.max()) + 1 if cur.num_jobs else 0, next_index=100_000, ts=int(cur.job_run_ts.max()) if cur.num_jobs else 0,
              job_cap=cur.num_jobs, halved=False, last_round=None, turn=int(rng.integers(8, 22)), out_first=bool(rng.random() < 0.6))
    steps, a, i = [], None, 0
    first_rebuild_done = False
    try:
        a = fresh(L, cur)
        while True:
            if i == 0:
                step = Step("load", f"seed {seed}", {}, cur)
            else:
                op = _draw(cur, rng, st, i, max_steps)
                cur, detail, stats = _RUN[op](a, cur, rng, st)
                step = Step(op, detail, stats, cur)
            steps.append(step)
            assert a.num_jobs == cur.num_jobs and a.num_nodes == cur.num_nodes
            tail = np.arange(max(cur.num_jobs - 8, 0), cur.num_jobs)
            step.resident = bool(rng.random() < 0.5)
            refusal = bool(rng.random() < REFUSAL_RATE)

            def rider(v0, step=step, cur=cur, tail=tail):
                kind, code, want = _refuse(a, cur, rng)
                step.refusal = (kind, code)
                assert code == want, f"{kind}: error code {code}, documented {want}"
                assert a.num_jobs == cur.num_jobs and a.num_nodes == cur.num_nodes
                assert _view(a, cur, tail) == v0, f"{kind}: the refused call changed what the handle answers"
            v, r, rst, u = _answers(a, cur, tail, step.resident, rider if refusal else None)
            step.answers, step.fast_iterations = (v, r, u), rst["fast_iterations"]
            st["last_round"] = r
            if recorded is None:
                _against_fresh(L, cur, tail, step.resident, step.answers, step.fast_iterations)
                _against_oracle(oracle, cur, r)
            else:
                want = recorded[i]
                assert (step.op, step.detail, step.M, step.N) == (want.op, want.detail, want.M, want.N), f"the replay drew {step.line()}, recorded {want.line()}"
                assert step.stats == want.stats, f"call statistics {step.stats}, recorded {want.stats}: another path was taken"
                assert step.refusal == want.refusal, (step.refusal, want.refusal)
                _compare(step.answers, want.answers, "the recorded ones")
                last = i == min(max_steps, len(recorded) - 1)
                if (_rebuilt(step) and not first_rebuild_done) or i == min(max_steps, len(recorded) - 1) // 2 or last:
                    _against_fresh(L, cur, tail, step.resident, step.answers, step.fast_iterations)
                first_rebuild_done = first_rebuild_done or _rebuilt(step)
            if i >= max_steps:
                break
            i += 1
    except Exception as e:   # noqa: BLE001  (a SchedError of a legal call is a finding like any other)
        trace = "\n".join(f"  {k:2d} {s.line()}" for k, s in enumerate(steps))
        raise SequenceFailure(f"seed {seed}, step {i}, M={cur.num_jobs} N={cur.num_nodes}: {type(e).__name__}: {str(e)[:600]}\n{trace}\n"
                              f"(run_sequence(L, oracle, {seed}, max_steps=k) cuts the sequence to a prefix)") from e
    finally:
        if a is not None:
            a.close()
    return steps


# ---------------------------------------------------------------- what a set of recorded sequences covers
def coverage(recordings):
    """counts over the Steps of many sequences: what tests/test_z_resident_sequences.py's non-triviality test asks of the pinned seeds"""
    c = {f"op {o}": 0 for o in OPS}
    c.update({k: 0 for k in ("append in place", "append rebuilt", "append grew jobCap", "append grew jobCap after a halving delete", "one node", "compact retired a shape",
                             "compact retired a class", "checks", "rounds that placed a job", "resident prepares", "steps")})
    c.update({f"refusal {k}": 0 for k in REFUSALS})
    for edge in (64, 128):
        for op in ("nodes_delete", "nodes_append"):
            c[f"{op} across {edge}"] = 0
    for steps in recordings:
        for s in steps:
            c["checks"] += 1
            c["rounds that placed a job"] += int(len(s.answers[1].scheduled) > 0)
            c["resident prepares"] += int(s.resident)
            c["one node"] += int(s.N == 1)
            if s.refusal:
                c[f"refusal {s.refusal[0]}"] += 1
            if s.op == "load":
                continue
            c["steps"] += 1
            c[f"op {s.op}"] += 1
            if s.op == "jobs_append":
                c["append in place"] += int(s.stats["in_place"] > 0 and s.stats["rebuilt"] == 0)
                c["append rebuilt"] += int(s.stats["rebuilt"] == 1)
                c["append grew jobCap"] += s.stats["grew"]
                c["append grew jobCap after a halving delete"] += s.stats["after_halving"]
            elif s.op == "shapes_compact":
                c["compact retired a shape"] += int(s.stats["shapes_retired"] > 0)
                c["compact retired a class"] += int(s.stats["classes_retired"] > 0)
            elif s.op in ("nodes_delete", "nodes_append"):
                for edge in (64, 128):
                    lo, hi = sorted((s.stats["n_before"], s.N))
                    c[f"{s.op} across {edge}"] += int(lo <= edge < hi)
    return c
