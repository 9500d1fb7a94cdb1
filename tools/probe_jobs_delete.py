"""What a scheduling cycle pays to drop the finished jobs from the handle: asched_jobs_set of the reduced table against asched_jobs_delete of the rows, on the headline
input (BASELINE configs[2]) with 200 000 rows without a run deleted, and on the configs[4] checker input with 1 000, on the GPU box.

  probe_jobs_delete.py [--reps 10] [--scale 1.0] [--gone 200000] [--only headline|checker]

In ONE process per library: the table is generated once; the rows to delete are a seeded draw from the table's rows without a run.  Two phases, each --reps times after one
warm-up pass.  Phase 1, the same calls whatever the library (so that two libraries can be compared), alternating:
  (i)   jobs_set of the UNTOUCHED table (wall time);
  (ii)  jobs_set of the reduced table (wall time): what a caller without the entry point does instead of a delete.
Phase 2, a library with the entry point only:
  jobs_set of the untouched table, then
  (iii) jobs_delete of the rows, wall time, with the device time of its five passes from stream events around them and the host's compaction of its mirrors (ASCHED_JD_TIMES=1,
        set here; the library prints them on stderr, which this script reads back), and the gather's traffic in GB/s: the bytes of every static per-job array of the surviving
        rows, read and written once, over the device time of the three gather launches;
  (iv)  the same delete with the id map downloaded into a fresh array (what Scheduler.jobs_delete(want_map=True) does);
  (v)   the same through the C entry point into a buffer of the caller's that every repetition uses again.
After the last repetition the per-queue scheduling order and the id map must equal those of jobs_set of the reduced table.  The transient peak of device memory is what the
driver reports as used while the call's fresh blocks and the old ones both exist — read before, and computed from the block sizes (the call is synchronous: nothing can
sample it from outside).  A library without the entry point (an older build, through ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1) gets (i) and (ii) only.  One JSON line per input."""
import argparse, copy, json, os, re, statistics, sys, tempfile, time
os.environ["ASCHED_JD_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--gone", type=int, default=200_000)
ap.add_argument("--only", default="")
args = ap.parse_args()
lib = armada_amd.load_library()
sc = args.scale
have = hasattr(lib.lib, lib.prefix + "jobs_delete")
HBM_PEAK_GBS = 8000.0                                # MI355X: 8 TB/s

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)
F_JOB = ("job_req", "job_queue", "job_pc", "job_submit", "job_node", "job_run_prio", "job_run_ts", "job_gang", "job_gang_card", "job_req_class", "job_away")


def inputs():
    if args.only in ("", "headline"):
        yield "headline configs[2]", W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64), max(8, int(args.gone * sc))
    if args.only in ("", "checker"):
        wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(300_000 * sc)), n_queues=64, occupied=0.95)
        wl.global_burst, wl.queue_burst = 1_000, 1_000; wl.config.max_queue_lookback = 100_000
        yield "configs[4] checker", wl, max(8, int(1_000 * sc))


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def reduced(wl, rows):
    keep = np.ones(wl.num_jobs, bool); keep[rows] = False
    w = copy.copy(wl)
    for f in F_JOB:
        v = getattr(wl, f)
        if v is not None:
            setattr(w, f, np.asarray(v)[keep].copy())
    return w, np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


for name, wl, gone_n in inputs():
    rng = np.random.default_rng(9)
    idle = np.nonzero(wl.job_node < 0)[0]
    gone = np.sort(rng.permutation(idle)[:gone_n]).astype(np.int32)
    w1, want_map = reduced(wl, gone)
    s = W.load(lib, wl)
    t_set, t_set_red, t_set_before, t_del, t_del_map, t_del_reused, stats, got_map = [], [], [], [], [], [], {}, None
    import ctypes
    i32p = ctypes.POINTER(ctypes.c_int32)
    reused = np.zeros(wl.num_jobs, np.int32)         # (v): the id map into a buffer of the caller's that every repetition uses again
    os.dup2(errlog.fileno(), 2)
    errlog.seek(0); errlog.truncate()
    try:
        for i in range(args.reps + 1):               # phase 1
            a = timed(lambda: W.set_jobs(s, wl))
            b = timed(lambda: W.set_jobs(s, w1))
            if i > 0:                                # (the first pass of each loads code objects and sizes buffers)
                t_set.append(a); t_set_red.append(b)
        free0 = torch.cuda.mem_get_info()[0]
        for i in range(args.reps + 1 if have else 0):   # phase 2
            a = timed(lambda: W.set_jobs(s, wl))
            b = timed(lambda: s.jobs_delete(gone)); stats = s.jobs_delete_stats()
            W.set_jobs(s, wl)
            box = []
            c = timed(lambda: box.append(s.jobs_delete(gone, want_map=True)))
            if i == args.reps:
                got = [s.scheduling_order(q) for q in range(wl.num_queues)]
                got_map = box[0]
            W.set_jobs(s, wl)
            d = timed(lambda: lib.jobs_delete(s.h, len(gone), gone.ctypes.data_as(i32p), reused.ctypes.data_as(i32p)))
            s.num_jobs = w1.num_jobs
            if i > 0:
                t_set_before.append(a); t_del.append(b); t_del_map.append(c); t_del_reused.append(d)
        if have:
            W.set_jobs(s, w1)
            assert [s.scheduling_order(q) for q in range(wl.num_queues)] == got, "the order after the delete is not the order of jobs_set"
            assert (got_map == want_map).all(), "the id map is not cumsum(keep) - 1"
            assert stats["rows"] == len(gone) and stats["num_jobs"] == w1.num_jobs, stats
    finally:
        os.dup2(saved_err, 2)
    errlog.seek(0)
    lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched jobs_delete]")]
    keys = ("mark", "scan", "gather", "order", "gang lists", "host mirrors")
    dev = {k: [] for k in keys}
    for l in lines[3:]:                              # (without the warm-up pass: three deletes a repetition)
        for key in keys:
            dev[key].append(float(re.search(key + r" ([0-9.]+) ms", l).group(1)))
    R = wl.job_req.shape[1]
    has_rec = 128                                    # (the JobRec table, where the handle has the fast structure: the headline and the checker input do)
    row_bytes = 8 * 4 + 4 + 1 + 8 + 8 + 8 + 8 * R + has_rec + (1 if wl.job_away is not None else 0)   # eight 4-byte arrays, queue priority, aligned, lease, submit, run timestamp, requests, JobRec
    moved = 2 * row_bytes * w1.num_jobs + 4 * w1.num_jobs          # read + written, and the survivors' list
    out = dict(input=name, nodes=wl.num_nodes, jobs=wl.num_jobs, deleted=len(gone), reps=args.reps, has_jobs_delete=have,
               jobs_set_untouched_ms=spread(t_set), jobs_set_reduced_ms=spread(t_set_red))
    if have:
        g = spread(dev["gather"])
        out.update(jobs_set_untouched_before_delete_ms=spread(t_set_before), delete_ms=spread(t_del), delete_with_map_ms=spread(t_del_map), delete_with_map_reused_buffer_ms=spread(t_del_reused),
                   delete_device_ms={k: spread(v) for k, v in dev.items() if k != "host mirrors"}, delete_host_mirrors_ms=spread(dev["host mirrors"]),
                   gather_bytes=moved, gather_gbs_at_median=round(moved / 1e6 / g["median"], 1) if g and g["median"] > 0 else None,
                   gather_share_of_hbm_peak=round(moved / 1e6 / g["median"] / HBM_PEAK_GBS, 3) if g and g["median"] > 0 else None,
                   transient_peak_bytes=row_bytes * stats["capacity"], device_free_before_bytes=int(free0),
                   gate_delete_max_below_jobs_set_reduced_min=bool(max(t_del) < min(t_set_red)), stats=stats)
    print(json.dumps(out), flush=True)
    s.close()
