"""The literal batched first fit on the GPU box, one shape per call:

  probe_fit_literal.py batch     [--nodes 100000]            fit_select_batch of off-grid requests (>= 2 000 distinct literal shapes): device ms of index build + query
  probe_fit_literal.py yardstick [--nodes 100000]            fit_select_batch of ONE shape on the aligned twin: device ms of one plane pass (x distinct shapes = "a pass per query")
  probe_fit_literal.py submit    [--nodes 20000 --units N]   submit check of N individual off-grid units on the pristine pool: kernel_times()['submit_check_ms']

--lib PATH loads another build of the library (the parent commit's, for the yardstick and the sequential submit check) instead of the tree's.
ASCHED_FIT_LIT_TIMES=1 is set for `batch`: the library prints the index build and the query kernel separately on stderr."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W
from armada_amd.binding import Library

Gi = 1024 ** 3
ap = argparse.ArgumentParser()
ap.add_argument("what", choices=("batch", "yardstick", "submit"))
ap.add_argument("--nodes", type=int, default=0)
ap.add_argument("--units", type=int, default=10_000)
ap.add_argument("--shapes", type=int, default=2500)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lib", default=None)
args = ap.parse_args()
if args.what == "batch":
    os.environ["ASCHED_FIT_LIT_TIMES"] = "1"
lib = Library(args.lib, "asched_") if args.lib else armada_amd.load_library()
nodes = args.nodes or (20_000 if args.what == "submit" else 100_000)


def offgrid_pool(n_nodes):
    """default_indexed off the grid with the queued requests redrawn from a palette: memory 1-64 GiB, cpu in 250m steps, ephemeral 1-200 GiB"""
    wl = W.default_indexed(n_nodes=n_nodes, n_jobs=200_000, n_queues=64, occupied=0.95, aligned=False)
    rng = np.random.Generator(np.random.PCG64(424242))
    q = np.nonzero(wl.job_node < 0)[0]
    pal = np.zeros((args.shapes, wl.job_req.shape[1]), np.int64)
    pal[:, W.MEM] = rng.integers(1, 65, size=len(pal)) * Gi
    pal[:, W.CPU] = rng.integers(1, 33, size=len(pal)) * 250
    pal[:, W.EPH] = rng.integers(1, 201, size=len(pal)) * Gi
    gpu = wl.job_req[q, W.GPU].copy()
    wl.job_req[q] = pal[rng.integers(0, len(pal), size=len(q))]
    wl.job_req[q, W.GPU] = gpu
    return wl, q.astype(np.int32)


def offgrid(wl, jobs):
    off = np.zeros(len(jobs), bool)
    for col, res in zip(wl.config.indexed_col, wl.config.indexed_resolution):
        off |= wl.job_req[jobs, col] % res != 0
    return off


rec = {"what": args.what, "nodes": nodes, "lib": args.lib or "tree"}
if args.what == "batch":
    wl, q = offgrid_pool(nodes)
    s = W.load(lib, wl); W.prepare(s, wl)
    lit = q[offgrid(wl, q)]
    keys = np.concatenate([wl.job_req[lit], wl.job_pc[lit][:, None]], axis=1)
    rec["queries"] = int(len(lit)); rec["distinct_literal_shapes"] = int(len(np.unique(keys, axis=0)))   # a scheduling-key shape is (request, priority class) here: no selectors, no tolerations
    prio = s.priorities[0]
    ms, host = [], []
    for i in range(args.reps + 1):
        t0 = time.perf_counter(); out = s.fit_select_batch(lit, prio); t1 = time.perf_counter()
        if i:   # (the first call loads the code object and sizes the scratch)
            ms.append(s.kernel_times()["fit_batch_ms"]); host.append((t1 - t0) * 1e3)
    rec.update(device_ms_build_plus_query=ms, device_ms_median=statistics.median(ms), host_ms_median=statistics.median(host), found=int((out >= 0).sum()))
elif args.what == "yardstick":
    wl = W.default_indexed(n_nodes=nodes, n_jobs=200_000, n_queues=64, occupied=0.95, aligned=True)
    s = W.load(lib, wl); W.prepare(s, wl)
    q = np.nonzero(wl.job_node < 0)[0].astype(np.int32)
    one = q[(wl.job_req[q] == wl.job_req[q[0]]).all(axis=1) & (wl.job_pc[q] == wl.job_pc[q[0]])]   # every job of ONE shape
    prio = s.priorities[0]
    ms = []
    for i in range(args.reps + 1):
        s.fit_select_batch(one, prio)
        if i:
            ms.append(s.kernel_times()["fit_batch_ms"])
    rec.update(queries=int(len(one)), device_ms_one_shape=ms, device_ms_median=statistics.median(ms))
else:
    wl, q = offgrid_pool(nodes)
    s = W.load(lib, wl)   # pristine: nothing bound
    lit = q[offgrid(wl, q)][:args.units]
    units = (np.arange(len(lit) + 1, dtype=np.int32), lit)
    ms, host = [], []
    for i in range(2):   # the sequential path of the parent takes seconds: one warm-up, one timed call
        t0 = time.perf_counter(); res = s.submit_check(csr=units, strip_gang=[True] * len(lit)); t1 = time.perf_counter()
        ms.append(s.kernel_times()["submit_check_ms"]); host.append((t1 - t0) * 1e3)
    rec.update(units=int(len(lit)), stats=s.submit_stats(), device_ms=ms, host_ms=host, ok=int(sum(r[0] for r in res)))
print(json.dumps(rec))
