"""What a NEW requirement class costs on the headline input (BASELINE configs[2]: 100 000 nodes, 1.56 M rows) on the GPU box: asched_req_classes_append against the
only way a build without it has, asched_jobs_set of the same table with the grown class list.

  probe_req_classes_append.py [--reps 10] [--scale 1.0] [--new 20000] [--sync]

The probe gives the nodes an indexed label (key 3, three values), a label that is not indexed (key 5) and an indexed taint (key 9, on every fourth node without a
running job; its key is the one indexed taint key, so the call scans the node taints), so that six node types exist.  ONE process per library: a build without the entry point (the parent commit's, through
ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1) runs jobs_set of the grown class list instead; run the two libraries in turn in one GPU session.  Each of --reps
repetitions after one warm-up pass, per case — t1: one class decided by node type; t2: one class matched on the host; mixed: four classes, two of each:
  jobs_set of the table (timed for reference: jobs_set_ms);
  (with the entry point)    req_classes_append of the case, asserted in place with the expected rows per tier  -> classes_append_ms, with the device ms of the new
                            rows and of the row copies and the host ms of the taint scan and of the host rows (ASCHED_CA_TIMES=1, set here; read back from stderr);
  (without the entry point) jobs_set of the table with the grown class list                                  -> jobs_set_grown_ms.
Then the whole sequence, per repetition: jobs_set, jobs_append of batch A (re-allocates; not timed), then class append (mixed) plus jobs_append of --new rows with
5 new shapes of the new classes, in place -> sequence_ms; without the entry point jobs_set of table + A + the rows with the grown class list -> jobs_set_sequence_ms.
After the last repetition the per-queue scheduling order and the first fit of the new rows must equal what jobs_set of that table leaves.  One JSON line."""
import argparse, copy, json, os, re, statistics, sys, tempfile, time
os.environ["ASCHED_CA_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--new", type=int, default=20_000)
ap.add_argument("--sync", action="store_true", help="a query that waits for the device in front of every timed call: the call alone, without what the jobs_set before it left queued")
args = ap.parse_args()
lib = armada_amd.load_library()
sc = args.scale
have = hasattr(lib.lib, lib.prefix + "req_classes_append")

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    if args.sync:
        s.fit_select_batch(np.zeros(1, np.int32))     # (a query: it changes nothing and returns when the device has caught up)
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
rng = np.random.default_rng(9)
n = wl.num_nodes
busy = np.zeros(n, bool)
busy[np.unique(wl.job_node[wl.job_node >= 0])] = True                  # (the running jobs stay where they are: class 0 tolerates nothing)
wl.config.indexed_label_keys = [3]
wl.config.indexed_taint_keys = [9]                                    # every taint a node carries is indexed, which the call finds out by a scan
wl.node_labels = [[(3, i % 3), (5, i % 2)] for i in range(n)]
wl.node_taints = [[(9, 1, 1)] if (i % 4 == 0 and not busy[i]) else [] for i in range(n)]
wl.job_req_class = np.zeros(wl.num_jobs, np.int32)
wl.class_tolerations, wl.class_selectors = [[]], [[]]
T1 = [([], [(3, 2)]), ([(9, 1, 0, 0)], [(3, 0)])]                     # (tolerations, selector): decided by node type
T2 = [([], [(5, 1)]), ([(9, 1, 0, 0)], [(5, 0), (3, 1)])]             # a selector key that is not indexed: matched on the host
CASES = dict(t1=(T1[:1], 1, 0), t2=(T2[:1], 0, 1), mixed=([T1[0], T2[0], T1[1], T2[1]], 2, 2))


def with_classes(w, classes):
    g = copy.copy(w)
    g.class_tolerations = list(w.class_tolerations) + [t for t, _ in classes]
    g.class_selectors = list(w.class_selectors) + [s for _, s in classes]
    return g


queued = np.nonzero((wl.job_node < 0) & (wl.job_gang < 0))[0]
m = max(8, int(args.new * sc))
t_sub = int(wl.job_submit.max()) + 1
NEW = 5


def batch(k, new_classes=False):
    src = rng.choice(queued, size=m)
    b = dict(req=wl.job_req[src].copy(), queue=wl.job_queue[src].copy(), pc=wl.job_pc[src].copy(), submit_time=t_sub + k * m + np.arange(m, dtype=np.int64),
             req_class=np.zeros(m, np.int32))
    if new_classes:                                   # 5 rows of the four new classes (ids 1 .. 4): 5 new shapes
        for i in range(NEW):
            b["req_class"][i * (m // NEW)] = 1 + i % 4
            b["req"][i * (m // NEW), W.CPU] += 1000 * (i + 1)
    return b


def grown(w, b):
    g = copy.copy(w)
    k = len(b["queue"])
    g.job_req, g.job_queue, g.job_pc, g.job_submit = np.concatenate([w.job_req, b["req"]]), np.concatenate([w.job_queue, b["queue"]]), np.concatenate([w.job_pc, b["pc"]]), np.concatenate([w.job_submit, b["submit_time"]])
    g.job_node, g.job_run_prio, g.job_run_ts = np.concatenate([w.job_node, np.full(k, -1, np.int32)]), np.concatenate([w.job_run_prio, np.zeros(k, np.int32)]), np.concatenate([w.job_run_ts, np.zeros(k, np.int64)])
    g.job_gang, g.job_gang_card = np.concatenate([w.job_gang, np.full(k, -1, np.int32)]), np.concatenate([w.job_gang_card, np.ones(k, np.int32)])
    g.job_req_class = np.concatenate([w.job_req_class, b["req_class"]])
    return g


A, Cb = batch(0), batch(1, new_classes=True)
mixed = CASES["mixed"][0]
final = with_classes(grown(grown(wl, A), Cb), mixed)
s = W.load(lib, wl)
if have and hasattr(lib.lib, lib.prefix + "set_append_in_place"):
    s.set_append_in_place(True)
t_set, t_case, t_seq, stats = [], {k: [] for k in CASES}, [], {}
new_rows = wl.num_jobs + m + np.arange(0, m, max(1, m // 64), dtype=np.int32)
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.reps + 1):
        for name, (classes, by_type, on_host) in CASES.items():
            a = timed(lambda: W.set_jobs(s, wl))
            if have:
                c = timed(lambda: s.req_classes_append([t for t, _ in classes], [x for _, x in classes]))
                st = stats[name] = s.req_classes_append_stats()
                assert st["rebuilt"] == 0 and st["reason"] == 0 and st["by_type"] == by_type and st["on_host"] == on_host and st["added"] == len(classes), st
            else:
                g = with_classes(wl, classes)
                c = timed(lambda: W.set_jobs(s, g))
            if i > 0:                                 # (the first pass loads code objects and sizes buffers)
                t_set.append(a); t_case[name].append(c)
        if have:
            W.set_jobs(s, wl)
            s.jobs_append(**A)

            def seq():
                s.req_classes_append([t for t, _ in mixed], [x for _, x in mixed])
                s.jobs_append(**Cb)
            d = timed(seq)
            stats["sequence_append"], stats["sequence_shapes"] = s.jobs_append_stats(), s.jobs_append_shape_stats()
            assert stats["sequence_append"]["rebuilt"] == 0 and stats["sequence_append"]["in_place"] == NEW and stats["sequence_shapes"]["reason"] == 0, stats
        else:
            d = timed(lambda: W.set_jobs(s, final))
        if i == args.reps:
            got = [s.scheduling_order(q) for q in range(wl.num_queues)], s.fit_select_batch(new_rows).tolist()
        if i > 0:
            t_seq.append(d)
    W.set_jobs(s, final)
    assert ([s.scheduling_order(q) for q in range(wl.num_queues)], s.fit_select_batch(new_rows).tolist()) == got, "the grown handle is not the handle of jobs_set"
finally:
    os.dup2(saved_err, 2)
errlog.seek(0)
lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched req_classes_append]")]
keys = ("new rows", "row copies", "taint scan", "host rows")
dev = {name: {k: [] for k in keys} for name in CASES}
for k, l in enumerate(lines[4:]):                    # (without the warm-up pass: three cases and the sequence per repetition)
    if k % 4 == 3:
        continue
    name = list(CASES)[k % 4]
    for key in keys:
        dev[name][key].append(float(re.search(key + r" ([0-9.]+) ms", l).group(1)))
out = dict(input="headline configs[2] with six node types", sync=args.sync, nodes=wl.num_nodes, jobs=wl.num_jobs, new_rows=m, reps=args.reps, has_req_classes_append=have,
           jobs_set_ms=spread(t_set), stats=stats)
out["classes_append_ms" if have else "jobs_set_grown_ms"] = {k: spread(v) for k, v in t_case.items()}
out["sequence_ms" if have else "jobs_set_sequence_ms"] = spread(t_seq)
if have:
    out.update(pass_ms={name: {k.replace(" ", "_"): spread(v) for k, v in d.items()} for name, d in dev.items()})
print(json.dumps(out), flush=True)
s.close()
