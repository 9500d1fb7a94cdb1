"""What applying a round's result to the resident job table costs on the headline input (BASELINE configs[2]: 100 000 nodes, 1.56 M rows) on the GPU box:
asched_round_commit against the path a build without it has — the entries built from the downloaded result (numpy, vectorised) and handed to asched_jobs_patch.

  probe_round_commit.py [--runs 3] [--scale 1.0] [--hostsim]

ONE process, one library, one handle.  After the same headline round each time, the two legs alternate, --runs of each after one warm-up of each (the first
incremental call on the table uploads the order-key inputs, which is neither leg's business):
  parent leg   scheduled_job / scheduled_node / scheduled_priority / preempted_job of the result -> four entry arrays -> jobs_patch      -> parent_ms
  tree leg     round_commit(run_timestamp, 0)                                                                                              -> tree_ms
each with the device ms of scatter / remove / sort / merge (ASCHED_JP_TIMES=1, set here; read from the library's stderr line of the call).  A query that waits for
the device stands in front of every timed leg.  Between two legs the table is put back with a jobs_patch of the same rows to what they held (not timed), so every leg
sees the same table and the same round; the per-queue order after either leg must be the same.  One JSON line.
--hostsim: a rehearsal of the script on the CPU build of the device code; its times say nothing about the GPU.

  timeout -k 10 900 python tools/probe_round_commit.py"""
import argparse, json, os, re, sys, tempfile, time
os.environ["ASCHED_JP_TIMES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--hostsim", action="store_true")
args = ap.parse_args()
if not args.hostsim:
    import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W
from armada_amd.binding import Library

lib = Library(os.path.join(ROOT, "tests", "hostsim", "libhostsim.so"), "asched_") if args.hostsim else armada_amd.load_library()
sc = args.scale
TS = 5_000_000_000
errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines (one per call with ASCHED_JP_TIMES=1) go into a file of our own
saved_err = os.dup(2)
LINE = re.compile(rb"\[asched (jobs_patch|round_commit)\] jobs \d+ entries (\d+) in the order (\d+): scatter ([\d.]+) ms, remove ([\d.]+) ms, sort ([\d.]+) ms, merge ([\d.]+) ms")


def last_line(which):
    text = os.pread(errlog.fileno(), os.fstat(errlog.fileno()).st_size, 0)      # (descriptor 2 shares the file's offset: read beside it)
    hits = [m for m in LINE.finditer(text) if m.group(1) == which.encode()]
    return [float(x) for x in hits[-1].groups()[3:]] if hits else None


def timed(fn):
    s.fit_select_batch(np.zeros(1, np.int32))         # (a query: it changes nothing and returns when the device has caught up)
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def headline_round():
    W.prepare(s, wl)
    return s.schedule_round()


def parent_leg(r):
    """the path of a build without round_commit: the entries from the result, then jobs_patch"""
    ns, npre = len(r.scheduled_job), len(r.preempted_job)
    rows = np.concatenate([r.scheduled_job, r.preempted_job])
    node = np.concatenate([r.scheduled_node, np.full(npre, -1, np.int32)])
    prio = np.concatenate([r.scheduled_priority_arr, np.zeros(npre, np.int32)])
    ts = np.concatenate([np.full(ns, TS, np.int64), np.zeros(npre, np.int64)])
    s.jobs_patch(rows, node, prio, ts)


def put_back(r):
    rows = np.concatenate([r.scheduled_job, r.preempted_job])
    s.jobs_patch(rows, wl.job_node[rows], wl.job_run_prio[rows], wl.job_run_ts[rows])


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
s = W.load(lib, wl)
t = {"parent": [], "tree": []}
dev = {"parent": [], "tree": []}
order = {}
shape = None
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.runs + 1):
        for leg in ("parent", "tree"):
            r = headline_round()
            if shape is None:
                shape = (len(r.scheduled_job), len(r.preempted_job))
            assert shape == (len(r.scheduled_job), len(r.preempted_job)), "the legs do not see the same round"
            ms = timed((lambda: parent_leg(r)) if leg == "parent" else (lambda: s.round_commit(TS, 0)))
            if leg == "tree":
                st = s.round_commit_stats()
                assert (st["scheduled"], st["preempted"], st["extra"]) == (shape[0], shape[1], 0), st
            if i > 0:                                 # (the first pass of either leg loads code objects, sizes the scratch and makes the order-key inputs resident)
                t[leg].append(round(ms, 3))
                dev[leg].append(last_line("jobs_patch" if leg == "parent" else "round_commit"))
            if i == args.runs:
                order[leg] = [s.scheduling_order(q) for q in range(wl.num_queues)]
            put_back(r)
    assert order["parent"] == order["tree"], "the committed order is not the patched order"
finally:
    os.dup2(saved_err, 2)
names = ("scatter", "remove", "sort", "merge")
out = dict(input="headline configs[2]", hostsim=args.hostsim, nodes=wl.num_nodes, jobs=wl.num_jobs, runs=args.runs, scheduled=shape[0], preempted=shape[1],
           parent_ms=dict(min=min(t["parent"]), max=max(t["parent"]), runs=t["parent"]), tree_ms=dict(min=min(t["tree"]), max=max(t["tree"]), runs=t["tree"]),
           pass_ms={leg: {n: [x[j] for x in v if x] for j, n in enumerate(names)} for leg, v in dev.items()},
           tree_max_below_parent_min=bool(max(t["tree"]) < min(t["parent"])))
print(json.dumps(out), flush=True)
s.close()
