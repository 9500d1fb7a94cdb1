"""What a scheduling cycle pays to tell the handle which nodes left the pool since the last one: asched_nodes_upsert of the reduced table (plus the renumbering of the
running jobs) against asched_nodes_delete of the rows, on the headline input (BASELINE configs[2]: 100 000 nodes, 1 560 757 jobs) with 1 000 idle rows deleted, on the
GPU box.

  probe_nodes_delete.py [--reps 10] [--scale 1.0] [--rows 1000]

In ONE process: the table is generated and loaded once (nodes and jobs; the runs on the rows that will leave are ended in the input, and the last of those rows gets a
taint of its own so that it is the only node of its type), then each phase runs --reps times after one warm-up pass.
Phase 1, the same calls whatever the library (so that two libraries can be compared), alternating:
  (iv) nodes_upsert of the untouched table (wall time);
  (i)  nodes_upsert of the reduced table alone (wall time): a LOWER bound on what a library without the entry point needs, which must also renumber the running jobs;
  (v)  that renumbering: jobs_patch of every running row above the first deleted row (wall time); (i) + (v) is the full alternative.
Phase 2, a library with the entry point only; every repetition starts from nodes_upsert of the untouched table and the job table's old numbering, untimed:
  (ii)  nodes_delete of the rows, none of them the last of its type: the device path, wall time and the device time of its passes from stream events around them
        (ASCHED_ND_TIMES=1, set here; the library prints them on stderr, which this script reads back);
  (iii) nodes_delete of the one node that is the last of its type: the rebuild path (reason 2).
After the last repetition of (ii) the first fits of a sample of jobs and the totals must equal those after (i) + (v).  A library without the entry point (an older
build, through ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1) gets phase 1 only.  One JSON line."""
import argparse, json, os, re, statistics, sys, tempfile, time
os.environ["ASCHED_ND_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rows", type=int, default=1000)
args = ap.parse_args()
lib = armada_amd.load_library()
sc = args.scale
have = hasattr(lib.lib, lib.prefix + "nodes_delete")

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
n = wl.num_nodes
rng = np.random.default_rng(9)
k = max(2, min(int(args.rows * sc), n // 2))
rows = np.sort(rng.choice(n, size=k + 1, replace=False)).astype(np.int32)
lone, rows = int(rows[-1]), rows[:-1]                # `lone`: the node that is the last of its type; `rows`: the k rows of the device path
on_rows = np.isin(wl.job_node, np.append(rows, lone))
wl.job_node[on_rows], wl.job_run_prio[on_rows], wl.job_run_ts[on_rows] = -1, 0, 0      # the drained rows are idle: their runs have ended
wl.config.indexed_taint_keys = None
wl.node_taints = [[] for _ in range(n)]
wl.node_taints[lone] = [(9, 1, 1)]
keep = np.ones(n, bool); keep[rows] = False
new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
total1, taints1 = wl.node_total[keep], [t for t, kp in zip(wl.node_taints, keep) if kp]
jrows = np.nonzero(wl.job_node > int(rows[0]))[0].astype(np.int32)                      # the running rows whose node is renumbered
node_old, node_new = wl.job_node[jrows].astype(np.int32), new_id[wl.job_node[jrows]]
prio, ts = wl.job_run_prio[jrows], wl.job_run_ts[jrows]
sample = np.arange(0, wl.num_jobs, max(1, wl.num_jobs // 4096), dtype=np.int32)

s = W.load(lib, wl)
t_same, t_reduced, t_renumber, t_dev, t_rebuild, stats = [], [], [], [], [], {}
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.reps + 1):                   # phase 1
        s.nodes_upsert(wl.node_total, taints=wl.node_taints)
        s.jobs_patch(jrows, node_old, prio, ts)      # (untimed: the whole table and the job table's old numbering)
        a = timed(lambda: s.nodes_upsert(wl.node_total, taints=wl.node_taints))
        b = timed(lambda: s.nodes_upsert(total1, taints=taints1))
        c = timed(lambda: s.jobs_patch(jrows, node_new, prio, ts))
        if i > 0:                                    # (the first pass of each loads code objects and sizes buffers)
            t_same.append(a); t_reduced.append(b); t_renumber.append(c)
    want = (s.fit_select_batch(sample).tolist(), s.total_resources().tolist(), s.lib.num_nodes(s.h))
    for i in range(args.reps + 1 if have else 0):    # phase 2
        s.nodes_upsert(wl.node_total, taints=wl.node_taints)
        s.jobs_patch(jrows, node_old, prio, ts)
        a = timed(lambda: s.nodes_delete(rows)); stats["device"] = s.nodes_delete_stats()
        if i == args.reps:
            got = (s.fit_select_batch(sample).tolist(), s.total_resources().tolist(), s.lib.num_nodes(s.h))
        c = timed(lambda: s.nodes_delete([int(new_id[lone])])); stats["rebuild"] = s.nodes_delete_stats()
        if i > 0:
            t_dev.append(a); t_rebuild.append(c)
    if have:
        assert got == want, "the handle's first fits and totals after the delete are not those of nodes_upsert of the reduced table"
        assert stats["device"][:5] == [k, len(jrows), 0, 0, n - k] and stats["rebuild"][:5] == [1, stats["rebuild"][1], 1, 2, n - k - 1], stats
finally:
    os.dup2(saved_err, 2)
errlog.seek(0)
lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched nodes_delete]") and "path device" in l]
passes = ["mark \\+ check", "scan", "gather", "index order", "mask rows", "job remap", "unmark"]
dev = {p.replace("\\", ""): [] for p in passes}
mask_rows = None
for l in lines[1:]:                                  # (without the warm-up pass)
    for p in passes:
        dev[p.replace("\\", "")].append(float(re.search(p + r" ([0-9.]+) ms", l).group(1)))
    mask_rows = int(re.search(r"mask rows (\d+) path", l).group(1))
out = dict(input="headline configs[2]", nodes=n, jobs=wl.num_jobs, rows_deleted=int(k), running_rows_renumbered=int(len(jrows)), reps=args.reps, has_nodes_delete=have,
           nodes_upsert_untouched_ms=spread(t_same), nodes_upsert_reduced_ms=spread(t_reduced), jobs_patch_renumber_ms=spread(t_renumber),
           full_alternative_ms=spread([x + y for x, y in zip(t_reduced, t_renumber)]))
if have:
    R = wl.node_total.shape[1]
    npad, npad1 = (n + 63) // 64 * 64, (n - k + 63) // 64 * 64
    out.update(delete_device_ms=spread(t_dev), delete_rebuild_ms=spread(t_rebuild), delete_device_passes_ms={key: spread(v) for key, v in dev.items()}, stats=stats, mask_rows=mask_rows,
               gather_bytes=int(2 * 2 * R * (n - k) * 8 + (n - k) * (4 + 1 + 4 + 4 + 8 + 8)), mask_bytes=None if mask_rows is None else int(mask_rows * (npad + npad1) // 8 + 4 * (n - k)),
               gate_max_device_below_min_reduced_upsert=bool(max(t_dev) < min(t_reduced)))
print(json.dumps(out), flush=True)
s.close()
