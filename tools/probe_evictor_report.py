"""What the evictor report (asched_set_evictor_report) adds to a round on the GPU box, on the headline input (BASELINE configs[2]) and on the configs[4] checker input
(100 000 nodes 95 % occupied, the reference's default limits: bench.py config4_checker_record).

  probe_evictor_report.py [--reps 10] [--scale 1.0] [--only headline|checker]

In ONE process, after a warm-up round of each setting, rounds alternate between switch off and switch on, --reps of each.  Per input one JSON line: median and
min..max of the round's phase-1 host time (asched_round_timing: evict1_host_ms) and of its total device time, for both settings, and the device time of the three new
launches from stream events around them (ASCHED_EVR_TIMES=1, set here: job pass + node pass, queue pass; the library prints the three separately on stderr).  The
events are recorded only in rounds with the switch on: six hipEventRecord calls are part of what those rounds pay here and not in production."""
import argparse, json, os, statistics, sys, time
os.environ["ASCHED_EVR_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--only", default="")
args = ap.parse_args()
lib = armada_amd.load_library()
sc = args.scale


def inputs():
    if args.only in ("", "headline"):
        yield "headline configs[2]", W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
    if args.only in ("", "checker"):
        wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(300_000 * sc)), n_queues=64, occupied=0.95)
        wl.global_burst, wl.queue_burst = 1_000, 1_000; wl.config.max_queue_lookback = 100_000
        yield "configs[4] checker", wl


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


for name, wl in inputs():
    s = W.load(lib, wl)
    rec = {False: dict(evict1=[], total=[], wall=[]), True: dict(evict1=[], total=[], wall=[], job_node=[], queue=[], fetch=[])}
    n1 = launches = None
    for i in range(2 * (args.reps + 1)):
        on = bool(i & 1)
        s.set_evictor_report(on)
        W.prepare(s, wl)
        t0 = time.perf_counter(); r = s.schedule_round(); t1 = time.perf_counter()
        t = s.round_timing()
        if on:
            t2 = time.perf_counter(); rep = s.round_evictor_report(); t3 = time.perf_counter()
            assert rep["num_evicted"] == r.num_evicted_phase1 == int(rep["queue_evicted_jobs"].sum())
        if i < 2:          # (the first round of each setting loads code objects and sizes buffers)
            continue
        d = rec[on]
        d["evict1"].append(t["evict1_host_ms"]); d["total"].append(t["total_ms"]); d["wall"].append((t1 - t0) * 1e3)
        if on:
            d["job_node"].append(t["evr_job_node_ms"]); d["queue"].append(t["evr_queue_ms"]); d["fetch"].append((t3 - t2) * 1e3)
            n1, launches = rep["num_evicted"], t["launches"]
    print(json.dumps(dict(input=name, nodes=wl.num_nodes, jobs=wl.num_jobs, evicted_phase1=n1, launches_on=launches, reps=args.reps,
                          off={k: spread(v) for k, v in rec[False].items()}, on={k: spread(v) for k, v in rec[True].items()},
                          phase1_host_ms_added=round(statistics.median(rec[True]["evict1"]) - statistics.median(rec[False]["evict1"]), 4),
                          device_ms_added=round(statistics.median(rec[True]["total"]) - statistics.median(rec[False]["total"]), 4))), flush=True)
    s.close()
