"""What retiring dead shapes costs on the headline input (BASELINE configs[2]: 100 000 nodes, 1.56 M rows) on the GPU box: asched_shapes_compact against the only remedy
a build without it has, asched_jobs_set of the same table.

  probe_shapes_compact.py [--reps 10] [--scale 1.0] [--dead 100] [--rounds]

ONE process per library: a build without the entry point (the parent commit's, through ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1) times jobs_set only; run the two
libraries in turn in one GPU session.  In front of every timed call a query waits for the device.  Each of --reps repetitions after one warm-up pass:
  jobs_set of the table (eleven requirement classes, ten of them without rows)                                        -> jobs_set_ms;
  (with the entry point) --dead rows of --dead new shapes appended in place and deleted again, then shapes_compact()   -> compact_ms, asserted in place;
                         the same with the dead shapes naming the ten classes, then shapes_compact(classes=True)      -> compact_classes_ms, ten classes retired;
                         device ms of the row pass / the gathers / the class bits and host ms of the mirror remap (ASCHED_SC_TIMES=1, set here; read from stderr).
After the last repetition the per-queue scheduling order and a first fit must equal what jobs_set of the table (with the reduced class list) leaves.
--rounds (with the entry point): the headline round on a fresh handle, and on a resident handle with --dead and with 2 x --dead + 60 dead fit shapes (the second is
above SMAX where the first is not), before and after the compact: round ms, fast and generic iterations, fit shapes.  One JSON line."""
import argparse, copy, json, os, re, statistics, sys, tempfile, time
os.environ["ASCHED_SC_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--dead", type=int, default=100)
ap.add_argument("--rounds", action="store_true")
args = ap.parse_args()
lib = armada_amd.load_library()
sc = args.scale
have = hasattr(lib.lib, lib.prefix + "shapes_compact")
NCLS = 10                                            # classes only dead shapes name

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    s.fit_select_batch(np.zeros(1, np.int32))         # (a query: it changes nothing and returns when the device has caught up)
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
wl.job_req_class = np.zeros(wl.num_jobs, np.int32)
wl.class_tolerations, wl.class_selectors = [[] for _ in range(1 + NCLS)], [[] for _ in range(1 + NCLS)]
one = copy.copy(wl)
one.class_tolerations, one.class_selectors = [[]], [[]]
queued = np.nonzero((wl.job_node < 0) & (wl.job_gang < 0))[0]
t_sub = int(wl.job_submit.max()) + 1
M = wl.num_jobs


def kill(k, classes=False, salt=0):
    """k rows of k new fit shapes (the non-indexed request moves) appended in place and deleted again"""
    src = queued[np.arange(k) % len(queued)]
    req = wl.job_req[src].copy()
    req[:, W.EPH] = (3000 + salt + np.arange(k)) * W.Gi
    s.jobs_append(req, queue=wl.job_queue[src], pc=np.zeros(k, np.int32), submit_time=t_sub + np.arange(k, dtype=np.int64),
                  req_class=(1 + np.arange(k) % NCLS).astype(np.int32) if classes else np.zeros(k, np.int32))
    assert s.jobs_append_stats()["rows"] == k
    s.jobs_delete(np.arange(M, M + k, dtype=np.int32))
    assert s.jobs_delete_stats()["shapes_emptied"] == k, s.jobs_delete_stats()


def round_of():
    W.prepare(s, wl)
    t0 = time.perf_counter(); s.schedule_round(); ms = (time.perf_counter() - t0) * 1e3
    st = s.round_stats()
    return dict(round_ms=round(ms, 1), fast_iterations=st["fast_iterations"], generic_iterations=st.get("generic_iterations"))


s = W.load(lib, wl)
if have:
    s.set_append_in_place(True)
t_set, t_c, t_cc, stats, rounds = [], [], [], {}, {}
probe_rows = np.arange(0, M, max(1, M // 64), dtype=np.int32)
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.reps + 1):
        a = timed(lambda: W.set_jobs(s, wl))
        if have:
            kill(args.dead)
            c = timed(lambda: s.shapes_compact())
            st = stats["compact"] = s.shapes_compact_stats()
            assert st["shapes_retired"] == args.dead and st["fit_retired"] == args.dead and st["rebuilt"] == 0 and st["classes_retired"] == 0, st
            kill(args.dead, classes=True)
            cc = timed(lambda: s.shapes_compact(classes=True))
            st = stats["compact_classes"] = s.shapes_compact_stats()
            assert st["shapes_retired"] == args.dead and st["classes_retired"] == NCLS and st["rebuilt"] == 0, st
            if i == args.reps:
                got = [s.scheduling_order(q) for q in range(wl.num_queues)], s.fit_select_batch(probe_rows).tolist()
        if i > 0:                                     # (the first pass loads code objects and sizes buffers)
            t_set.append(a)
            if have:
                t_c.append(c); t_cc.append(cc)
    if have:
        W.set_jobs(s, one)
        assert ([s.scheduling_order(q) for q in range(wl.num_queues)], s.fit_select_batch(probe_rows).tolist()) == got, "the compacted handle is not the handle of jobs_set"
    if have and args.rounds:
        W.set_jobs(s, wl)
        rounds["fresh"] = round_of()
        for name, k in (("dead", args.dead), ("dead_over_smax", 2 * args.dead + 60)):
            W.set_jobs(s, wl)
            for lo in range(0, k, 50):
                kill(min(50, k - lo), salt=lo)
            s.shapes_compact(count_only=True)
            f0 = s.shapes_compact_stats()["fit_shapes"]
            before = round_of()
            s.shapes_compact()
            st = s.shapes_compact_stats()
            rounds[name] = dict(fit_shapes_before=f0, before=before, compact=st, after=round_of())
finally:
    os.dup2(saved_err, 2)
errlog.seek(0)
lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched shapes_compact]")]
keys = ("rows", "gathers", "class bits", "host mirrors")
dev = {name: {k: [] for k in keys} for name in ("compact", "compact_classes")}
for k, l in enumerate(lines[2:2 * (args.reps + 1)]):  # (without the warm-up pass: the two cases per repetition)
    for key in keys:
        dev[("compact", "compact_classes")[k % 2]][key].append(float(re.search(key + r" ([0-9.]+) ms", l).group(1)))
out = dict(input="headline configs[2], eleven requirement classes", nodes=wl.num_nodes, jobs=M, dead=args.dead, reps=args.reps, has_shapes_compact=have, jobs_set_ms=spread(t_set))
if have:
    out.update(compact_ms=spread(t_c), compact_classes_ms=spread(t_cc), stats=stats, pass_ms={n: {k.replace(" ", "_"): spread(v) for k, v in d.items()} for n, d in dev.items()})
    if args.rounds:
        out["rounds"] = rounds
print(json.dumps(out), flush=True)
s.close()
