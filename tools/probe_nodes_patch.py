"""What a scheduling cycle pays to tell the handle which nodes were cordoned or lost capacity since the last one: asched_nodes_upsert of the whole table against
asched_nodes_patch of the changed rows, on the headline input (BASELINE configs[2]: 100 000 nodes, 1 560 757 jobs) with 1 000 rows changed (500 cordoned, 500 with
allocatable cut), on the GPU box.

  probe_nodes_patch.py [--reps 10] [--scale 1.0] [--rows 1000]

In ONE process: the table is generated and loaded once (nodes and jobs), then each phase runs --reps times after one warm-up pass.
Phase 1, the same calls whatever the library (so that two libraries can be compared), alternating:
  (iv) nodes_upsert of the unchanged table (wall time);
  (i)  nodes_upsert of the table with the rows changed (wall time).
Phase 2, a library with the entry point only, alternating:
  (ii)  nodes_patch of the changed rows, then of their old values: the device path, wall time of both and the device time of its two passes from stream events around
        them (ASCHED_NP_TIMES=1, set here; the library prints them on stderr, which this script reads back);
  (iii) nodes_patch that takes 137 milli-cpu off one node of a table whose allocatable is all on the index grid: the rebuild path (reason 3).  The aggregates a
        patch keeps are conservative, so the same patch would take the device path the second time: every repetition starts from nodes_upsert of the unchanged
        table, untimed.
After the last repetition the first fits of a sample of jobs must equal those after nodes_upsert of the same table.  A library without the entry point (an older build,
through ASCHED_LIB_PATH with ASCHED_AB_OLD_LIB=1: tools/ab_call.sh) gets (i) and (iv) only.  One JSON line."""
import argparse, json, os, re, statistics, sys, tempfile, time
os.environ["ASCHED_NP_TIMES"] = "1"
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
have = hasattr(lib.lib, lib.prefix + "nodes_patch")

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None


def timed(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
n = wl.num_nodes
rng = np.random.default_rng(9)
k = max(2, min(int(args.rows * sc), n) // 2 * 2)
rows = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
cordon, cut = rows[: k // 2], rows[k // 2:]
alloc0, uns0 = wl.node_total.copy(), np.zeros(n, np.uint8)
alloc1, uns1 = alloc0.copy(), uns0.copy()
uns1[cordon] = 1
alloc1[cut, W.CPU] -= 8000
alloc1[cut, W.MEM] -= 64 * W.Gi                      # (on the index grid, inside [0, total])
sample = np.arange(0, wl.num_jobs, max(1, wl.num_jobs // 4096), dtype=np.int32)

s = W.load(lib, wl)
t_same, t_changed, t_fwd, t_back, t_rebuild, stats = [], [], [], [], [], {}
off_grid = alloc0[rows[:1]].copy()
off_grid[:, W.CPU] -= 137
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.reps + 1):                   # phase 1
        a = timed(lambda: s.nodes_upsert(wl.node_total, alloc0, unschedulable=uns0))
        b = timed(lambda: s.nodes_upsert(wl.node_total, alloc1, unschedulable=uns1))
        if i > 0:                                    # (the first pass of each loads code objects and sizes buffers)
            t_same.append(a); t_changed.append(b)
    want = s.fit_select_batch(sample).tolist()
    for i in range(args.reps + 1 if have else 0):    # phase 2
        s.nodes_upsert(wl.node_total, alloc0, unschedulable=uns0)
        a = timed(lambda: s.nodes_patch(rows, allocatable=alloc1[rows], unschedulable=uns1[rows])); stats["device"] = s.nodes_patch_stats()
        if i == args.reps:
            got = s.fit_select_batch(sample).tolist()
        b = timed(lambda: s.nodes_patch(rows, allocatable=alloc0[rows], unschedulable=uns0[rows]))
        c = timed(lambda: s.nodes_patch(rows[:1], allocatable=off_grid)); stats["rebuild"] = s.nodes_patch_stats()
        if i > 0:
            t_fwd.append(a); t_back.append(b); t_rebuild.append(c)
    if have:
        assert got == want, "the patched handle's first fits are not those of nodes_upsert"
        assert stats["device"][:4] == [k, 0, 0, 0] and stats["rebuild"][:4] == [1, 0, 1, 3], stats
finally:
    os.dup2(saved_err, 2)
errlog.seek(0)
lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched nodes_patch]")]
dev = {"scatter": [], "mask words": []}
for l in lines[2:]:                                  # (without the warm-up pass; the rebuild path prints nothing)
    for key in dev:
        dev[key].append(float(re.search(key + r" ([0-9.]+) ms", l).group(1)))
out = dict(input="headline configs[2]", nodes=n, jobs=wl.num_jobs, rows_changed=int(k), cordoned=int(k // 2), allocatable_cut=int(k // 2), reps=args.reps, has_nodes_patch=have,
           nodes_upsert_unchanged_ms=spread(t_same), nodes_upsert_changed_ms=spread(t_changed))
if have:
    out.update(patch_device_ms=spread(t_fwd), patch_device_back_ms=spread(t_back), patch_rebuild_ms=spread(t_rebuild),
               patch_device_passes_ms={key: spread(v) for key, v in dev.items()}, stats=stats)
print(json.dumps(out), flush=True)
s.close()
