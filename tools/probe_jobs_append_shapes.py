"""What asched_jobs_append costs when the batch brings NEW scheduling-key shapes, with and without asched_set_append_in_place, on the headline input (BASELINE
configs[2]) plus 20 000 newly submitted rows, 5 of them new shapes (tools/probe_jobs_append.py's batch C), on the GPU box.

  probe_jobs_append_shapes.py [--reps 10] [--scale 1.0] [--new 20000] [--away]

ONE process per library: a build without the switch (the parent commit's, through ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1) runs the same calls and takes the rebuild;
run the two libraries in turn in one GPU session and compare append_new_shapes_ms.  Each of --reps repetitions after one warm-up pass:
  jobs_set of the table; jobs_append of batch A (re-allocates: jobs_set allocates exactly M; not reported);
  (known) jobs_append of batch B: the same draw without new shapes;
  (new)   jobs_append of batch C: 5 new shapes — in place where the library has the switch (asserted: rebuilt == 0, in_place == 5), the rebuild otherwise — with the
          device ms of the mask rows and of the row copies (ASCHED_JA_TIMES=1, set here; the library prints them on stderr, which this script reads back).
--away: the table gets away node types and a second requirement class whose rows are all of priority class 0, and batch C's new shapes are of that class in a
priority class with away entries: the append that adds derived away classes and away rows (reported apart: it is another table, with twice the mask rows).
After the last repetition the per-queue scheduling order and every new row's first fit must equal what jobs_set of table + A + B + C leaves.  One JSON line."""
import argparse, copy, json, os, re, statistics, sys, tempfile, time
os.environ["ASCHED_JA_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--new", type=int, default=20_000)
ap.add_argument("--away", action="store_true")
args = ap.parse_args()
lib = armada_amd.load_library()
sc = args.scale
have = hasattr(lib.lib, lib.prefix + "set_append_in_place")

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
rng = np.random.default_rng(9)
if args.away:
    tainted = rng.random(wl.num_nodes) < 0.25
    tainted[np.unique(wl.job_node[wl.job_node >= 0])] = False          # (the running jobs stay where they are)
    wl.node_taints = [[(7, 1, 1)] if t else [] for t in tainted]
    wl.config.wkt_taints = [[(7, 1, 1)], [(7, -1, 1)]]
    wl.config.pc_away = [[], [(0, 0)], [(2, 1), (1, 0)]][:len(wl.config.pc_priority)] + [[]] * max(0, len(wl.config.pc_priority) - 3)
    cls = np.zeros(wl.num_jobs, np.int32)
    small = wl.job_req[:, W.CPU] == wl.job_req[:, W.CPU].min()          # (few distinct requests: the fit shapes, one per (request, class), stay below SMAX)
    cls[(wl.job_pc == 0) & (wl.job_node < 0) & (wl.job_gang < 0) & small & (rng.random(wl.num_jobs) < 0.05)] = 1
    wl.job_req_class, wl.class_tolerations, wl.class_selectors = cls, [[], []], [[], []]
queued = np.nonzero((wl.job_node < 0) & (wl.job_gang < 0))[0]
m = max(8, int(args.new * sc))
t_sub = int(wl.job_submit.max()) + 1
NEW = 5


def batch(k, new_shapes=0):
    src = rng.choice(queued, size=m)
    b = dict(req=wl.job_req[src].copy(), queue=wl.job_queue[src].copy(), pc=wl.job_pc[src].copy(), submit_time=t_sub + k * m + np.arange(m, dtype=np.int64))
    if wl.job_req_class is not None:
        b["req_class"] = wl.job_req_class[src].copy()
    for i in range(new_shapes):                      # request vectors off the table's grid of shapes: one more milli-cpu
        r = i * (m // max(new_shapes, 1))
        b["req"][r, W.CPU] += 1000 * (i + 1) + 1000 * 977
        if args.away:
            b["req_class"][r], b["pc"][r] = 1, 1     # a requirement class that had no away rows, in a priority class with an away entry
    return b


A, B, C = batch(0), batch(1), batch(2, new_shapes=NEW)


def grown(w, b):
    g = copy.copy(w)
    k = len(b["queue"])
    g.job_req, g.job_queue, g.job_pc, g.job_submit = np.concatenate([w.job_req, b["req"]]), np.concatenate([w.job_queue, b["queue"]]), np.concatenate([w.job_pc, b["pc"]]), np.concatenate([w.job_submit, b["submit_time"]])
    g.job_node, g.job_run_prio, g.job_run_ts = np.concatenate([w.job_node, np.full(k, -1, np.int32)]), np.concatenate([w.job_run_prio, np.zeros(k, np.int32)]), np.concatenate([w.job_run_ts, np.zeros(k, np.int64)])
    g.job_gang, g.job_gang_card = np.concatenate([w.job_gang, np.full(k, -1, np.int32)]), np.concatenate([w.job_gang_card, np.ones(k, np.int32)])
    if w.job_req_class is not None:
        g.job_req_class = np.concatenate([w.job_req_class, b["req_class"]])
    return g


s = W.load(lib, wl)
if have:
    s.set_append_in_place(True)
t_known, t_shapes, stats = [], [], {}
new_rows = wl.num_jobs + 2 * m + np.arange(0, m, max(1, m // 64), dtype=np.int32)
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.reps + 1):
        W.set_jobs(s, wl)
        s.jobs_append(**A)
        c = timed(lambda: s.jobs_append(**B)); stats["known"] = s.jobs_append_stats()
        d = timed(lambda: s.jobs_append(**C)); stats["new_shapes"] = s.jobs_append_stats()
        if have:
            stats["shape_stats"] = s.jobs_append_shape_stats()
        if i == args.reps:
            got = [s.scheduling_order(q) for q in range(wl.num_queues)], s.fit_select_batch(new_rows).tolist()
        if i > 0:                                    # (the first pass loads code objects and sizes buffers)
            t_known.append(c); t_shapes.append(d)
    W.set_jobs(s, grown(grown(grown(wl, A), B), C))
    assert ([s.scheduling_order(q) for q in range(wl.num_queues)], s.fit_select_batch(new_rows).tolist()) == got, "the appended table is not the table of jobs_set"
    assert stats["known"]["rebuilt"] == 0 and stats["new_shapes"]["new_shapes"] == NEW, stats
    if have:
        assert stats["new_shapes"]["rebuilt"] == 0 and stats["new_shapes"]["in_place"] == NEW and stats["shape_stats"]["reason"] == 0, stats
        assert stats["shape_stats"]["derived_classes"] == (1 if args.away else 0), stats      # (class 1, the one away entry of priority class 1)
    else:
        assert stats["new_shapes"]["rebuilt"] == 1, stats
finally:
    os.dup2(saved_err, 2)
errlog.seek(0)
lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched jobs_append]") and "shapes in place" in l]
dev = {"mask rows": [], "row copies": []}
for k, l in enumerate(lines[3:]):                    # (without the warm-up pass)
    if k % 3 != 2:
        continue                                     # (the append with new shapes: the third of each repetition)
    for key in dev:
        dev[key].append(float(re.search(key + r" ([0-9.]+) ms", l).group(1)))
out = dict(input="headline configs[2]" + (" with away node types" if args.away else ""), nodes=wl.num_nodes, jobs=wl.num_jobs, new_rows=m, new_shapes=NEW, reps=args.reps,
           has_append_in_place=have, append_known_shapes_ms=spread(t_known), append_new_shapes_ms=spread(t_shapes), samples_new_shapes_ms=[round(x, 3) for x in t_shapes], stats=stats)
if have:
    out.update(device_ms={k.replace(" ", "_"): spread(v) for k, v in dev.items()})
print(json.dumps(out), flush=True)
s.close()
