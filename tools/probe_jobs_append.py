"""What a scheduling cycle pays to tell the handle which jobs were submitted since the last one: asched_jobs_set of the grown table against asched_jobs_append of the new
rows, on the headline input (BASELINE configs[2]) plus 20 000 newly submitted rows, on the GPU box.

  probe_jobs_append.py [--reps 10] [--scale 1.0] [--new 20000]

In ONE process: the table is generated once; the new rows are drawn from the table's own queued rows (their shapes, queues and classes, later submit times) — batch A and
batch B — and batch C is the same draw with a handful of request vectors the table does not hold.  Two phases, each --reps times after one warm-up pass.
Phase 1, the same calls whatever the library (so that two libraries can be compared), alternating:
  (vi)  jobs_set of the UNGROWN table (wall time);
  (i)   jobs_set of the table grown by A (wall time).
Phase 2, a library with the entry point only:
  jobs_set of the ungrown table (reported apart: it releases the larger blocks the appends before it left), then
  (iii) jobs_append of batch A onto it: the append that re-allocates (jobs_set allocates exactly M);
  (ii)  jobs_append of batch B: the append that fits the capacity, wall time and the device time of its three passes from stream events around them (ASCHED_JA_TIMES=1,
        set here; the library prints them on stderr, which this script reads back);
  (iv)  jobs_append of batch C: the append that brings new shapes (masks and fast structure are rebuilt).
After the last repetition the per-queue scheduling order must equal the one jobs_set of table + A + B + C left.  A library without the entry point (an older build, through
ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1: tools/ab_call.sh) gets (i) and (vi) only.  One JSON line."""
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
args = ap.parse_args()
lib = armada_amd.load_library()
sc = args.scale
have = hasattr(lib.lib, lib.prefix + "jobs_append")

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
rng = np.random.default_rng(9)
queued = np.nonzero((wl.job_node < 0) & (wl.job_gang < 0))[0]
m = max(8, int(args.new * sc))
t_sub = int(wl.job_submit.max()) + 1


def batch(k, new_shapes=0):
    src = rng.choice(queued, size=m)
    b = dict(req=wl.job_req[src].copy(), queue=wl.job_queue[src].copy(), pc=wl.job_pc[src].copy(), submit_time=t_sub + k * m + np.arange(m, dtype=np.int64))
    for i in range(new_shapes):                      # request vectors off the table's grid of shapes: one more milli-cpu
        b["req"][i * (m // max(new_shapes, 1)), W.CPU] += 1000 * (i + 1) + 1000 * 977
    return b


A, B, C = batch(0), batch(1), batch(2, new_shapes=5)


def grown(w, b):
    g = copy.copy(w)
    k = len(b["queue"])
    g.job_req, g.job_queue, g.job_pc, g.job_submit = np.concatenate([w.job_req, b["req"]]), np.concatenate([w.job_queue, b["queue"]]), np.concatenate([w.job_pc, b["pc"]]), np.concatenate([w.job_submit, b["submit_time"]])
    g.job_node, g.job_run_prio, g.job_run_ts = np.concatenate([w.job_node, np.full(k, -1, np.int32)]), np.concatenate([w.job_run_prio, np.zeros(k, np.int32)]), np.concatenate([w.job_run_ts, np.zeros(k, np.int64)])
    g.job_gang, g.job_gang_card = np.concatenate([w.job_gang, np.full(k, -1, np.int32)]), np.concatenate([w.job_gang_card, np.ones(k, np.int32)])
    return g


wA = grown(wl, A)
s = W.load(lib, wl)
t_set, t_set_grown, t_set_after, t_realloc, t_fit, t_shapes, stats = [], [], [], [], [], [], {}
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.reps + 1):                   # phase 1
        a = timed(lambda: W.set_jobs(s, wl))
        e = timed(lambda: W.set_jobs(s, wA))
        if i > 0:                                    # (the first pass of each loads code objects and sizes buffers)
            t_set.append(a); t_set_grown.append(e)
    for i in range(args.reps + 1 if have else 0):    # phase 2
        a = timed(lambda: W.set_jobs(s, wl))
        b = timed(lambda: s.jobs_append(**A)); stats["realloc"] = s.jobs_append_stats()
        c = timed(lambda: s.jobs_append(**B)); stats["fits"] = s.jobs_append_stats()
        d = timed(lambda: s.jobs_append(**C)); stats["new_shapes"] = s.jobs_append_stats()
        if i == args.reps:
            got = [s.scheduling_order(q) for q in range(wl.num_queues)]
        if i > 0:
            t_set_after.append(a); t_realloc.append(b); t_fit.append(c); t_shapes.append(d)
    if have:
        W.set_jobs(s, grown(grown(wA, B), C))
        assert [s.scheduling_order(q) for q in range(wl.num_queues)] == got, "the appended order is not the order of jobs_set"
        assert stats["realloc"]["reallocated"] == 1 and stats["fits"]["reallocated"] == 0 and stats["fits"]["rebuilt"] == 0 and stats["new_shapes"]["rebuilt"] == 1, stats
finally:
    os.dup2(saved_err, 2)
errlog.seek(0)
lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched jobs_append]")]
dev = {k: [] for k in ("fill", "sort", "merge")}
for k, l in enumerate(lines[3:]):                    # (without the warm-up pass)
    if k % 3 != 1:
        continue                                     # (the append that fits: the second of each repetition)
    for key in dev:
        dev[key].append(float(re.search(key + r" ([0-9.]+) ms", l).group(1)))
out = dict(input="headline configs[2]", nodes=wl.num_nodes, jobs=wl.num_jobs, new_rows=m, reps=args.reps, has_jobs_append=have,
           jobs_set_ungrown_ms=spread(t_set), jobs_set_grown_ms=spread(t_set_grown))
if have:
    out.update(jobs_set_ungrown_after_appends_ms=spread(t_set_after), append_fits_ms=spread(t_fit), append_reallocates_ms=spread(t_realloc), append_new_shapes_ms=spread(t_shapes),
               append_fits_device_ms={k: spread(v) for k, v in dev.items()}, stats=stats)
print(json.dumps(out), flush=True)
s.close()
