"""What a scheduling cycle pays for the queued lists of its round: built on the host and handed to asched_round_prepare, against asched_round_prepare_resident, which
derives them on the device from the resident job order — on the headline input (BASELINE configs[2]: 100 000 nodes, 1 560 757 jobs, 64 queues), on the GPU box.

  probe_round_prepare_resident.py [--reps 20] [--warmup 3] [--scale 1.0] [--held 0]

In ONE process: the table is generated and loaded once (nodes and jobs).  One shape at a time; every figure is the median of --reps repetitions after --warmup passes,
with min and max.
  (a) the host-side construction of the explicit lists, the way the simulator drivers build them every cycle: per queue, the rows of the workload's queue order that
      have no run, as an int32 array (a Python comprehension; a Go host walks its jobDb iterator instead — reported, not judged);
  (b) round_prepare with the explicit lists: wall time of the C call (the library's copy, upload and prepare passes) and of the binding call around it (which also
      concatenates the lists);
  (c) round_prepare_resident: the same two wall times, and the device time of mark / hold / compact from stream events around them (ASCHED_QL_TIMES=1, set here; the
      library prints them on stderr, which this script reads back).  --held names that many queued rows in `held` (they are then left out of the explicit lists too).
round_queued() after (b) and after (c) must be equal, offsets and jobs.  A library without the entry point (an older build, through ASCHED_LIB_PATH with
ASCHED_AB_OLD_LIB=1) gets (a) and (b) only.  One JSON line.
Two libraries in one GPU session: one process per library, every step under its own time limit, chained —
  ASCHED_AB_OLD_LIB=1 ASCHED_LIB_PATH=<parent's library> timeout -k 10 300 python tools/probe_round_prepare_resident.py && timeout -k 10 300 python tools/probe_round_prepare_resident.py"""
import argparse, json, os, re, statistics, sys, tempfile, time
os.environ["ASCHED_QL_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch; torch.cuda.init()
import armada_amd
from armada_amd import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--held", type=int, default=0)
args = ap.parse_args()
lib = armada_amd.load_library()
have = hasattr(lib.lib, lib.prefix + "round_prepare_resident")
sc = args.scale


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), max_minus_median=round(max(v) - statistics.median(v), 3)) if v else None


wl = W.config3(seed=W.SEED, n_nodes=max(64, int(100_000 * sc)), n_jobs=max(640, int(1_000_000 * sc)), n_queues=64)
s = W.load(lib, wl)
q = wl.num_queues
kw = dict(global_tokens=float(wl.global_burst), global_burst=wl.global_burst, global_rate_inf=wl.rate_inf,
          queue_tokens=[float(wl.queue_burst)] * q, queue_burst=[wl.queue_burst] * q, queue_rate_inf=[wl.rate_inf] * q)
node = wl.job_node
rng = np.random.default_rng(5)
all_queued = np.nonzero(node < 0)[0]
held = np.sort(rng.choice(all_queued, size=min(args.held, len(all_queued)), replace=False)).astype(np.int32) if args.held else None
is_held = np.zeros(wl.num_jobs, bool)
if held is not None:
    is_held[held] = True

c_ms = {}                                            # wall time of the C calls alone: the ctypes functions wrapped


def wrap(name):
    fn = getattr(lib, name)

    def timed(*a):
        t0 = time.perf_counter(); rc = fn(*a); c_ms.setdefault(name, []).append((time.perf_counter() - t0) * 1e3); return rc
    setattr(lib, name, timed)


wrap("round_prepare")
if have:
    wrap("round_prepare_resident")

errlog = tempfile.TemporaryFile(mode="w+b")          # the library's stderr lines go through a file of our own
saved_err = os.dup(2)
t_build, t_explicit, t_resident = [], [], []
lists_explicit = lists_resident = None
os.dup2(errlog.fileno(), 2)
try:
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        queued = [np.array([j for j in ql if node[j] < 0 and not is_held[j]], dtype=np.int32) for ql in wl.queued]
        t1 = time.perf_counter()
        s.round_prepare(wl.queue_weight, queued, **kw)
        t2 = time.perf_counter()
        if i >= args.warmup:
            t_build.append((t1 - t0) * 1e3); t_explicit.append((t2 - t1) * 1e3)
    if have:
        lists_explicit = s.round_queued()
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            s.round_prepare_resident(wl.queue_weight, held=held, **kw)
            if i >= args.warmup:
                t_resident.append((time.perf_counter() - t0) * 1e3)
        lists_resident = s.round_queued()
finally:
    os.dup2(saved_err, 2)
if have:
    assert len(lists_explicit) == len(lists_resident) == q and all(a.tolist() == b.tolist() for a, b in zip(lists_explicit, lists_resident)), \
        "round_queued after round_prepare_resident is not round_queued after round_prepare with the explicit lists"
errlog.seek(0)
lines = [l for l in errlog.read().decode(errors="replace").splitlines() if l.startswith("[asched round_prepare_resident]")][args.warmup:]
passes = {p: [float(re.search(p + r" ([0-9.]+) ms", l).group(1)) for l in lines] for p in ("mark", "hold", "compact")}
out = dict(input="headline configs[2]", nodes=wl.num_nodes, jobs=wl.num_jobs, queues=q, queued=int(sum(len(x) for x in queued)), held=0 if held is None else len(held),
           reps=args.reps, warmup=args.warmup, has_round_prepare_resident=have,
           a_host_list_build_ms=spread(t_build),
           b_round_prepare_explicit_c_call_ms=spread(c_ms["round_prepare"][args.warmup:]), b_round_prepare_explicit_binding_ms=spread(t_explicit))
if have:
    out.update(c_round_prepare_resident_c_call_ms=spread(c_ms["round_prepare_resident"][args.warmup:]), c_round_prepare_resident_binding_ms=spread(t_resident),
               device_passes_ms={p: spread(v) for p, v in passes.items()},
               device_mark_hold_compact_ms=spread([a + b + c for a, b, c in zip(passes["mark"], passes["hold"], passes["compact"])]),
               round_queued_equal=True)
print(json.dumps(out), flush=True)
s.close()
