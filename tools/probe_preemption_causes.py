"""asched_round_preemption_causes on the GPU box after a preemption-heavy round (BASELINE configs[4]: config3 at 95 % occupancy), against the same join done on the
host with numpy over the downloaded result lists (which cannot know the fair-share preemptors: it is given them, so it times the grouping and the record build only).

  probe_preemption_causes.py [--nodes 20000 --jobs 200000 --queues 32] [--reps 5]

Prints one JSON line: sizes, device ms of the join's kernels (kernel_times()['fit_batch_ms'] after the call: the events around its launches), wall ms of the whole
call (scratch, launches, download, the Python dict), wall ms of the numpy join, and the ratio.  ASCHED_PJOIN_TIMES=1 makes the library print the device time itself."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=20_000)
ap.add_argument("--jobs", type=int, default=200_000)
ap.add_argument("--queues", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
lib = armada_amd.load_library()
wl = W.config3(seed=W.SEED, n_nodes=args.nodes, n_jobs=args.jobs, n_queues=args.queues, occupied=0.95)
s = W.load(lib, wl); W.prepare(s, wl)
r = s.schedule_round()


def numpy_join(r, by, sib, in_gang):
    """the join on the host: a stable sort by node of the urgency entries, offsets, the reference's order of tests"""
    n = wl.num_nodes
    idx = np.nonzero(r.scheduled_method_arr == 4)[0]
    idx = idx[np.argsort(r.scheduled_node[idx], kind="stable")]
    cand = r.scheduled_job[idx]
    off = np.concatenate([[0], np.cumsum(np.bincount(r.scheduled_node[idx], minlength=n))])
    beg, end = off[r.preempted_node], off[r.preempted_node + 1]
    t = np.where(sib == -2, 5, np.where(by >= 0, 3, np.where(end > beg, 4, np.where(in_gang, 2, 1))))
    return t, cand, beg, end - beg


dev, wall, host = [], [], []
for i in range(args.reps + 1):
    t0 = time.perf_counter(); causes = s.preemption_causes(); t1 = time.perf_counter()
    if i:   # (the first call loads the code object and sizes the scratch)
        dev.append(s.kernel_times()["fit_batch_ms"]); wall.append((t1 - t0) * 1e3)
by = np.array([causes[int(j)][1] for j in r.preempted_job], dtype=np.int32)
sib = np.array([causes[int(j)][2] for j in r.preempted_job], dtype=np.int32)
in_gang = wl.job_gang[r.preempted_job] >= 0
for i in range(args.reps):
    t0 = time.perf_counter(); t, cand, beg, cnt = numpy_join(r, by, sib, in_gang); t1 = time.perf_counter()
    host.append((t1 - t0) * 1e3)
got_t = np.array([causes[int(j)][0] for j in r.preempted_job])
assert (got_t == t).all() and all(causes[int(j)][3] == tuple(cand[b:b + c].tolist()) for j, b, c, tt in zip(r.preempted_job, beg, cnt, t) if tt == 4)
types, counts = np.unique(got_t, return_counts=True)
print(json.dumps(dict(nodes=args.nodes, jobs=wl.num_jobs, scheduled=len(r.scheduled_job), preempted=len(r.preempted_job), candidates=int(len(cand)),
                      by_type={int(a): int(b) for a, b in zip(types, counts)}, device_ms=dev, device_ms_median=statistics.median(dev),
                      call_wall_ms_median=statistics.median(wall), numpy_join_ms_median=statistics.median(host),
                      numpy_over_device=statistics.median(host) / max(statistics.median(dev), 1e-9))))
