"""What a reprioritised job costs on the headline input (BASELINE configs[2]: 100 000 nodes, 1.56 M rows) on the GPU box: asched_jobs_reprioritise against the only way
a build without it has, asched_jobs_set of the same table with the new queue priorities.

  probe_jobs_reprioritise.py [--reps 10] [--scale 1.0] [--scattered 1000] [--jobset 50000] [--hostsim]

ONE process per library: a build without the entry point (the parent commit's, through ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1) runs jobs_set of the edited table
instead; run the two libraries in turn in one GPU session.  A query that waits for the device stands in front of every timed call.  Each of --reps repetitions after
one warm-up pass, per case — scattered: --scattered random rows to random priorities 0..3; jobset: --jobset rows of the largest queue (all of it where it has fewer)
to one priority; first: the scattered rows as the first incremental call after a jobs_set (it uploads the order-key inputs and allocates the second order buffer):
  (with the entry point)    jobs_set of the table, not timed, then the first call -> first_ms; then scattered and jobset on the handle that has the inputs resident
                            -> scattered_ms, jobset_ms, each with the device ms of scatter / remove / sort / merge (ASCHED_JP_TIMES=1, set here; read from
                            jobs_reprioritise_stats); and a scattered call followed by a jobs_patch of 1 000 other rows, timed as one -> with_patch_ms (two calls pay
                            the reset passes twice);
  (both)                    jobs_set of the table with the case's priorities -> jobs_set_ms per case.
After the last repetition the per-queue scheduling order must equal the one jobs_set of the edited table leaves.  One JSON line.
--hostsim: a rehearsal of the script on the CPU build of the device code; its times say nothing about the GPU.

  ASCHED_AB_OLD_LIB=1 ASCHED_LIB_PATH=<parent's library> timeout -k 10 500 python tools/probe_jobs_reprioritise.py && timeout -k 10 500 python tools/probe_jobs_reprioritise.py"""
import argparse, json, os, statistics, sys, tempfile, time
os.environ["ASCHED_JP_TIMES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--scattered", type=int, default=1_000)
ap.add_argument("--jobset", type=int, default=50_000)
ap.add_argument("--hostsim", action="store_true")
args = ap.parse_args()
if not args.hostsim:
    import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W
from armada_amd.binding import Library

lib = Library(os.path.join(ROOT, "tests", "hostsim", "libhostsim.so"), "asched_") if args.hostsim else armada_amd.load_library()
have = hasattr(lib.lib, lib.prefix + "jobs_reprioritise")
sc = args.scale

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines (one per call with ASCHED_JP_TIMES=1) go into a file of our own
saved_err = os.dup(2)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    s.fit_select_batch(np.zeros(1, np.int32))         # (a query: it changes nothing and returns when the device has caught up)
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def set_jobs(qprio):
    s.jobs_set(wl.job_req, queue=wl.job_queue, pc=wl.job_pc, queue_priority=qprio, submit_time=wl.job_submit, node=wl.job_node, scheduled_at_priority=wl.job_run_prio,
               run_timestamp=wl.job_run_ts, gang_id=wl.job_gang, gang_cardinality=wl.job_gang_card)


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
M = wl.num_jobs
rng = np.random.default_rng(22)
q0 = np.zeros(M, np.uint32)
sizes = np.bincount(wl.job_queue[wl.job_queue >= 0], minlength=wl.num_queues)
big = int(np.argmax(sizes))
rows_q = np.nonzero(wl.job_queue == big)[0]
CASES = {}
rows = rng.permutation(M)[:max(1, int(args.scattered * sc))].astype(np.int32)
CASES["scattered"] = (rows, rng.integers(0, 4, size=len(rows)).astype(np.uint32))
rows = rng.permutation(rows_q)[:max(1, int(args.jobset * sc))].astype(np.int32)
CASES["jobset"] = (rows, np.full(len(rows), 3, np.uint32))
patch_rows = np.setdiff1d(np.nonzero(wl.job_node >= 0)[0], CASES["scattered"][0])[:max(1, int(1_000 * sc))].astype(np.int32)


def edited(base, case):
    q = base.copy()
    q[CASES[case][0]] = CASES[case][1]
    return q


s = W.load(lib, wl)
t_set = {k: [] for k in CASES}
t_call = {k: [] for k in ("first", "scattered", "jobset", "with_patch")}
dev = {k: [] for k in ("first", "scattered", "jobset")}
stats = {}
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.reps + 1):
        for case in CASES:
            a = timed(lambda: set_jobs(edited(q0, case)))
            if i > 0:                                 # (the first pass loads code objects and sizes buffers)
                t_set[case].append(a)
        if have:
            set_jobs(q0)
            r, p = CASES["scattered"]
            c = {"first": timed(lambda: s.jobs_reprioritise(r, p))}
            st = {"first": s.jobs_reprioritise_stats()}
            assert st["first"]["made_resident"] == 1 and st["first"]["entries"] == len(r), st
            c["scattered"] = timed(lambda: s.jobs_reprioritise(r, (p + 1) % 4))      # every row moves again
            st["scattered"] = s.jobs_reprioritise_stats()
            r2, p2 = CASES["jobset"]
            c["jobset"] = timed(lambda: s.jobs_reprioritise(r2, p2))
            st["jobset"] = s.jobs_reprioritise_stats()
            assert st["scattered"]["made_resident"] == 0 and st["scattered"]["unchanged"] == 0 and st["jobset"]["in_order"] == len(r2), st

            def both():
                s.jobs_reprioritise(r, p)
                s.jobs_patch(patch_rows, wl.job_node[patch_rows], wl.job_run_prio[patch_rows], wl.job_run_ts[patch_rows] + 1)
            c["with_patch"] = timed(both)
            if i > 0:
                for k, v in c.items():
                    t_call[k].append(v)
                for k in dev:
                    dev[k].append(st[k]["device_ms"])
            stats = {k: {x: v[x] for x in ("entries", "in_order", "unchanged", "made_resident")} for k, v in st.items()}
    if have:                                          # the handle now holds: scattered, jobset, scattered again, and the patch's run timestamps (+1 ns)
        got = [s.scheduling_order(q) for q in range(wl.num_queues)]
        final = edited(edited(q0, "scattered"), "jobset")
        final[CASES["scattered"][0]] = CASES["scattered"][1]
        wl.job_run_ts = wl.job_run_ts.copy(); wl.job_run_ts[patch_rows] += 1
        set_jobs(final)
        assert [s.scheduling_order(q) for q in range(wl.num_queues)] == got, "the reprioritised order is not the order of jobs_set"
finally:
    os.dup2(saved_err, 2)
out = dict(input="headline configs[2]", hostsim=args.hostsim, nodes=wl.num_nodes, jobs=M, reps=args.reps, has_jobs_reprioritise=have,
           rows={k: int(len(v[0])) for k, v in CASES.items()}, largest_queue_rows=int(len(rows_q)), jobs_set_ms={k: spread(v) for k, v in t_set.items()})
if have:
    names = ("scatter", "remove", "sort", "merge")
    out.update(reprioritise_ms={k: spread(v) for k, v in t_call.items()}, stats=stats,
               pass_ms={k: {n: spread([x[j] for x in v]) for j, n in enumerate(names)} for k, v in dev.items()},
               # NOT measured: read off the code.  The first incremental call on a job table uploads queue priority (4 B), submit time and run timestamp (8 B each) per row
               from_the_code_not_measured=dict(first_call_upload_bytes=20 * M))
print(json.dumps(out), flush=True)
s.close()
