"""What a retried job costs on the headline input (BASELINE configs[2]: 100 000 nodes, 1.56 M rows) on the GPU box: asched_jobs_respec against the only way a build
without it has, asched_jobs_set of the same table with the new classes and requests.

  probe_jobs_respec.py [--reps 10] [--scale 1.0] [--hostsim]

ONE process.  A query that waits for the device stands in front of every timed call.  Each of --reps repetitions after one warm-up pass; every case starts from
jobs_set of the base table (not timed), so its shapes and classes are new every time:
  jobs_set        the parent's way: jobs_set of the table edited as in `five_shapes` -> jobs_set_ms
  one_shape       100 queued rows onto ONE new shape of a resident class (a memory bump)
  five_shapes     1 000 queued rows onto 5 new shapes
  own_class       1 000 queued rows, each with a new class of its own (node anti-affinity against one node: label HOST NotIn [node]) and a new request;
                  req_classes_append of the 1 000 classes is inside the timed region.  1 000 classes are more than the 64 the fast structure serves: the class
                  append rebuilds (its statistics say so), the respec itself does not
  fifty_classes   1 000 queued rows onto 50 new (class, request) pairs, req_classes_append of the 50 classes included: the anti-affinity case while the
                  classes stay under 64 and the fit shapes under SMAX, so that the fast structure stays
                  For the three cases with a class append the two calls are also timed apart -> parts_ms
  own_class_off   the same as own_class with asched_set_append_in_place off: the respec rebuilds masks and fast structure
After the last repetition the first fit of the named rows and of 10 000 others, and the order of the largest queue, must equal what jobs_set of the edited table
leaves.  One JSON line.  --hostsim: a rehearsal of the script on the CPU build of the device code; its times say nothing about the GPU.

  timeout -k 10 900 python tools/probe_jobs_respec.py"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--hostsim", action="store_true")
args = ap.parse_args()
if not args.hostsim:
    import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W
from armada_amd.binding import AFFINITY_OPS, Library, Scheduler

lib = Library(os.path.join(ROOT, "tests", "hostsim", "libhostsim.so"), "asched_") if args.hostsim else armada_amd.load_library()
sc = args.scale
HOST = 9001                                           # a label key that is not indexed: every node carries its number under it


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    s.fit_select_batch(np.zeros(1, np.int32))         # (a query: it changes nothing and returns when the device has caught up)
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
M, N = wl.num_jobs, wl.num_nodes
labels = [list(l) + [(HOST, n)] for n, l in enumerate(wl.node_labels)] if wl.node_labels is not None else [[(HOST, n)] for n in range(N)]
cls0 = np.zeros(M, np.int32) if wl.job_req_class is None else np.asarray(wl.job_req_class, dtype=np.int32)
tol0 = [[]] if wl.class_tolerations is None else wl.class_tolerations
sel0 = wl.class_selectors
C0 = len(tol0)


def set_jobs(req, cls, tol=tol0, sel=sel0, aff=None):
    s.jobs_set(req, queue=wl.job_queue, pc=wl.job_pc, submit_time=wl.job_submit, node=wl.job_node, scheduled_at_priority=wl.job_run_prio, run_timestamp=wl.job_run_ts,
               gang_id=wl.job_gang, gang_cardinality=wl.job_gang_card, req_class=cls, class_tolerations=tol, class_selectors=sel, class_affinities=aff, away=wl.job_away)


rng = np.random.default_rng(26)
free = np.nonzero((np.asarray(wl.job_node) < 0) & (np.asarray(wl.job_gang) < 0) & (np.asarray(wl.job_queue) >= 0))[0]
pc_most = int(np.argmax(np.bincount(np.asarray(wl.job_pc)[free])))
free = rng.permutation(free[(np.asarray(wl.job_pc)[free] == pc_most) & (cls0[free] == cls0[free[0]])])      # one priority class and one class: a request is a shape
assert len(free) >= int(1_100 * sc), len(free)
n100, n1000 = max(1, int(100 * sc)), max(5, int(1_000 * sc))
rows_a, rows_b = np.sort(free[:n100]).astype(np.int32), np.sort(free[n100:n100 + n1000]).astype(np.int32)
MEM = W.MEM
req_a = np.tile(np.asarray(wl.job_req)[rows_a[0]] + np.eye(W.R, dtype=np.int64)[MEM] * (5 * (W.Gi // 8)), (len(rows_a), 1))
cls_a = np.full(len(rows_a), cls0[rows_a[0]], np.int32)
req_b = np.tile(np.asarray(wl.job_req)[rows_b[0]], (len(rows_b), 1)) + np.eye(W.R, dtype=np.int64)[MEM] * ((1 + np.arange(len(rows_b)) % 5)[:, None] * 3 * (W.Gi // 8))
cls_b = np.full(len(rows_b), cls0[rows_b[0]], np.int32)
req_c = np.tile(np.asarray(wl.job_req)[rows_b[0]], (len(rows_b), 1)) + np.eye(W.R, dtype=np.int64)[MEM] * ((1 + np.arange(len(rows_b)) % 8)[:, None] * (W.Gi // 8)) \
    + np.eye(W.R, dtype=np.int64)[W.EPH] * ((1 + np.arange(len(rows_b)) // 8)[:, None] * (W.Gi // 4))      # (every row its own request, on the index grid)
nodes_c = rng.integers(0, N, size=len(rows_b))
aff_c = [[[(HOST, AFFINITY_OPS["NotIn"], [int(n)])]] for n in nodes_c]


def edited(rows, req, cls):
    r, c = np.asarray(wl.job_req).copy(), cls0.copy()
    r[rows], c[rows] = req, cls
    return r, c


s = Scheduler(lib, wl.config)
s.nodes_upsert(wl.node_total, wl.node_allocatable, taints=wl.node_taints, labels=labels, id_rank=wl.node_id_rank)
set_jobs(np.asarray(wl.job_req), cls0)
t = {k: [] for k in ("jobs_set", "one_shape", "five_shapes", "own_class", "fifty_classes", "own_class_off")}
t_parts = {k: dict(class_append=[], respec=[]) for k in ("own_class", "fifty_classes", "own_class_off")}
stats = {}


parts = {}                                            # of the last class-and-respec call: ms of req_classes_append and of jobs_respec


def own_class():
    t0 = time.perf_counter()
    first = s.req_classes_append([[] for _ in aff_c], affinities=aff_c)
    t1 = time.perf_counter()
    s.jobs_respec(rows_b, first + np.arange(len(rows_b), dtype=np.int32), req_c)
    parts.update(class_append=(t1 - t0) * 1e3, respec=(time.perf_counter() - t1) * 1e3)


def fifty_classes():
    k = min(50, len(rows_b))
    t0 = time.perf_counter()
    first = s.req_classes_append([[] for _ in range(k)], affinities=aff_c[:k])
    t1 = time.perf_counter()
    s.jobs_respec(rows_b, first + np.arange(len(rows_b), dtype=np.int32) % k, req_c[np.arange(len(rows_b)) % k])
    parts.update(class_append=(t1 - t0) * 1e3, respec=(time.perf_counter() - t1) * 1e3)


for i in range(args.reps + 1):
    print(f"repetition {i} of {args.reps}", file=sys.stderr, flush=True)
    c = {}
    rb, cb = edited(rows_b, req_b, cls_b)
    c["jobs_set"] = timed(lambda: set_jobs(rb, cb))
    for case, on, call in (("one_shape", True, lambda: s.jobs_respec(rows_a, cls_a, req_a)), ("five_shapes", True, lambda: s.jobs_respec(rows_b, cls_b, req_b)),
                           ("own_class", True, own_class), ("fifty_classes", True, fifty_classes), ("own_class_off", False, own_class)):
        set_jobs(np.asarray(wl.job_req), cls0)
        s.set_append_in_place(on)
        c[case] = timed(call)
        st = s.jobs_respec_stats()
        stats[case] = dict(st, class_append=s.req_classes_append_stats()) if case.startswith("own") else st
        assert st["rebuilt"] == (0 if on else 1) and st["reason"] == 0 and st["entries"] == (len(rows_a) if case == "one_shape" else len(rows_b)), (case, st)
        assert st["new_shapes"] == {"one_shape": 1, "five_shapes": 5, "fifty_classes": min(50, len(rows_b))}.get(case, len(rows_b)), (case, st)
        if case in t_parts and i > 0:
            for k, v in parts.items():
                t_parts[case][k].append(v)
    if i > 0:                                         # (the first pass loads code objects and sizes buffers)
        for k, v in c.items():
            t[k].append(v)
# the handle holds own_class_off; then five_shapes on a fresh table, compared with jobs_set of the edited table
set_jobs(np.asarray(wl.job_req), cls0)
s.set_append_in_place(True)
s.jobs_respec(rows_b, cls_b, req_b)
others = rng.permutation(M)[:max(1, int(10_000 * sc))].astype(np.int32)
big = int(np.argmax(np.bincount(wl.job_queue[wl.job_queue >= 0], minlength=wl.num_queues)))
got = (s.fit_select_batch(rows_b).tolist(), s.fit_select_batch(others).tolist(), s.scheduling_order(big))
rb, cb = edited(rows_b, req_b, cls_b)
set_jobs(rb, cb)
assert got == (s.fit_select_batch(rows_b).tolist(), s.fit_select_batch(others).tolist(), s.scheduling_order(big)), "the respec'd handle does not answer as jobs_set of the edited table"
res = {k: spread(v) for k, v in t.items()}
in_place = ("one_shape", "five_shapes", "own_class", "fifty_classes")
print(json.dumps(dict(input="headline configs[2]", hostsim=args.hostsim, nodes=N, jobs=M, reps=args.reps, rows=dict(one_shape=len(rows_a), others=len(rows_b)), ms=res, parts_ms={c: {k: spread(v) for k, v in p.items()} for c, p in t_parts.items()}, stats=stats,
                      respec_alone_max_below_jobs_set_min={c: spread(p["respec"])["max"] < res["jobs_set"]["min"] for c, p in t_parts.items() if c != "own_class_off"},
                      in_place_max_below_jobs_set_min={k: res[k]["max"] < res["jobs_set"]["min"] for k in in_place})), flush=True)
s.close()
