"""The platform layer's measurement hooks (plat.h: the per-pass device times of the resident table calls, of round_prepare_resident's queued lists and of the evictor
report), pinned from outside: the ASCHED_*_TIMES variables are read once per process, so every case is a fresh child process that loads one library.

The child runs one pinned seed of resident_sequences.run_sequence (every operation in resident_sequences.OPS, an in-place append of new shapes and resident prepares:
asserted below from the CPU build's recording, so a change of the runner cannot quiet it), then, on a second handle of the seed's start table, the calls that run no
pass (an empty jobs_reprioritise and jobs_delete, a nodes_delete refused because a node has a run) behind timed ones, and one round with the evictor report on.  It
prints the Step.line() of every step and a fingerprint of the round on stdout, leaves stderr to the library, and logs every call of a timed family on any handle into
a side file: its wall time, the bytes of stderr it wrote (stderr is a file: its size before and after the call), its arguments' sizes and its statistics.

With every ASCHED_*_TIMES=1: each call that ran passes wrote exactly one line of its family, in today's format, with the counts its statistics give; the device
times are 0.0000 on the CPU build; on the GPU they are finite, >= 0, sum to more than zero (every such call launches at least one kernel between its first and last
event) and to no more than the wall time measured around the call (every call waits for its stream; for the evictor report the round's wall time): conditions, not
tolerances.  The timing words of asched_jobs_reprioritise_stats are the printed times in microseconds: the word is (int32)(ms * 1000 + 0.5) of the unrounded time and
the line shows the time to 0.0001 ms, so the two are at most 0.5 + 0.05 us apart.  Words 6 and 7 of asched_round_timing are job pass + node pass and queue pass:
sums of the unrounded times, so within 1e-4 ms (two printed roundings) of the printed ones.
With no variable set: no line that begins with "[asched ", and those words are zero.  The stdout of both children is the same, line for line.

The line of jobs_append carries the two times of the in-place shape append, which has no line of its own: eleven line kinds for the eleven event sets, jobs_patch
and jobs_reprioritise sharing one."""
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 13
STEPS = 40
VARS = ("EVR", "JP", "JA", "CA", "SC", "JD", "NP", "ND", "NA", "QL")
F = r"(\d+\.\d{4})"
# written from the format strings of asched_host.inc: the named groups are the counts compared with the statistics, the unnamed ones the device times (in pass order)
LINES = {
    "jobs_patch": rf"jobs (?P<jobs>\d+) entries (?P<entries>\d+) in the order (?P<in_order>\d+): scatter {F} ms, remove {F} ms, sort {F} ms, merge {F} ms",
    "jobs_reprioritise": rf"jobs (?P<jobs>\d+) entries (?P<entries>\d+) in the order (?P<in_order>\d+): scatter {F} ms, remove {F} ms, sort {F} ms, merge {F} ms",
    "jobs_append": rf"jobs (?P<jobs>\d+) rows (?P<rows>\d+) in the order (?P<in_order>\d+): fill {F} ms, sort {F} ms, merge {F} ms; shapes in place (?P<in_place>\d+): mask rows {F} ms, row copies {F} ms",
    "req_classes_append": rf"nodes (?P<nodes>\d+) classes (?P<added>\d+) \(by node type (?P<by_type>\d+), on the host (?P<on_host>\d+)\), derived rows moved (?P<moved>\d+): "
                          rf"new rows {F} ms, row copies {F} ms; host: taint scan \d+\.\d{{4}} ms, host rows \d+\.\d{{4}} ms",
    "shapes_compact": rf"jobs (?P<jobs>\d+) shapes (?P<s0>\d+) -> (?P<s1>\d+) fit (?P<f0>\d+) -> (?P<f1>\d+) classes (?P<c0>\d+) -> (?P<c1>\d+) \(ext \d+ -> \d+\) (?P<path>rebuild|in place): "
                      rf"rows {F} ms, gathers {F} ms, class bits {F} ms; host mirrors \d+\.\d{{4}} ms",
    "jobs_delete": rf"jobs (?P<jobs>\d+) entries (?P<entries>\d+) in the order (?P<in_order>\d+): mark {F} ms, scan {F} ms, gather {F} ms, order {F} ms, gang lists {F} ms, host mirrors \d+\.\d{{4}} ms",
    "nodes_patch": rf"nodes (?P<nodes>\d+) entries (?P<entries>\d+) words (?P<words>\d+) mask rows \d+: scatter {F} ms, mask words {F} ms",
    "nodes_delete": rf"nodes (?P<nodes>\d+) entries (?P<entries>\d+) jobs (?P<jobs>\d+) mask rows \d+ path (?P<path>rebuild|device): "
                    rf"mark \+ check {F} ms, scan {F} ms, gather {F} ms, index order {F} ms, mask rows {F} ms, job remap {F} ms, unmark {F} ms",
    "nodes_append": rf"nodes (?P<nodes>\d+) entries (?P<entries>\d+) mask rows \d+ fresh blocks \d+: planes {F} ms, narrow arrays {F} ms, index order {F} ms, mask rows {F} ms",
    "round_prepare_resident": rf"rows (?P<jobs>\d+) order entries \d+ queues (?P<queues>\d+) held (?P<held>\d+) queued (?P<queued>\d+): mark {F} ms, hold {F} ms, compact {F} ms",
    "evict_report": rf"nodes (?P<nodes>\d+) jobs (?P<jobs>\d+) evicted (?P<evicted>\d+): job pass {F} ms, node pass {F} ms, queue pass {F} ms",
}
PASSES = dict(jobs_patch=4, jobs_reprioritise=4, jobs_append=5, req_classes_append=2, shapes_compact=3, jobs_delete=5, nodes_patch=2, nodes_delete=7, nodes_append=4,
              round_prepare_resident=3, evict_report=3)
TAG_OF = dict(round_evictor_report="evict_report")      # the call whose line has another tag than its name


def _parse(line):
    m = re.fullmatch(r"\[asched (\w+)\] (.*)", line)
    assert m and m.group(1) in LINES, line
    g = re.fullmatch(LINES[m.group(1)], m.group(2))
    assert g, f"not today's format: {line}"
    named = {k: (v if k == "path" else int(v)) for k, v in g.groupdict().items()}
    times = [float(x) for i, x in enumerate(g.groups(), 1) if i not in g.re.groupindex.values()]
    assert len(times) == PASSES[m.group(1)], line
    return m.group(1), named, times


def _expected(c):
    """-> None when the call ran no pass, else the counts its line must show: from the call's arguments and its statistics"""
    s, call = c["stats"], c["call"]
    if c["refused"]:
        return None
    if call == "jobs_patch":
        return dict(jobs=c["M"], entries=c["n"]) if c["n"] else None
    if call == "jobs_reprioritise":
        return dict(jobs=c["M"], entries=s["entries"], in_order=s["in_order"]) if c["n"] else None
    if call == "jobs_append":
        return dict(jobs=c["M"], rows=s["rows"], in_order=s["in_order"], in_place=s["in_place"]) if c["n"] else None
    if call == "req_classes_append":
        return dict(nodes=c["N"], added=s["added"], by_type=s["by_type"], on_host=s["on_host"], moved=s["moved"]) if s["added"] and not s["rebuilt"] else None
    if call == "shapes_compact":
        if not (s["shapes_retired"] or s["classes_retired"]):
            return None
        return dict(jobs=c["M"], s0=s["shapes"] + s["shapes_retired"], s1=s["shapes"], path="rebuild" if s["rebuilt"] else "in place", classes_retired=s["classes_retired"],
                    fit_retired=s["fit_retired"])
    if call == "jobs_delete":
        return dict(jobs=c["M"], entries=s["rows"], in_order=s["in_order"]) if c["n"] else None
    if call == "nodes_patch":
        return dict(nodes=c["N"], entries=s[0], words=c["words"]) if c["n"] and not s[2] else None
    if call == "nodes_delete":
        return dict(nodes=c["N"], entries=s[0], jobs=c["M"], path="rebuild" if s[2] else "device") if c["n"] else None
    if call == "nodes_append":
        return dict(nodes=c["N"], entries=s[0]) if c["n"] and not s[2] else None
    if call == "round_prepare_resident":
        return dict(jobs=c["M"], queues=c["queues"], held=c["n"], queued=c["queued"])
    if call == "round_evictor_report":
        return dict(nodes=c["N"], jobs=c["M"], evicted=s["evicted"])
    return None


def _run_child(lib, timed):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE]))
    for v in VARS:
        env.pop(f"ASCHED_{v}_TIMES", None)
        if timed:
            env[f"ASCHED_{v}_TIMES"] = "1"
    with tempfile.TemporaryDirectory() as tmp:
        log, errp = os.path.join(tmp, "calls.json"), os.path.join(tmp, "stderr.txt")
        with open(errp, "wb") as err:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), lib.path, str(SEED), log], env=env, stdout=subprocess.PIPE, stderr=err, text=True, timeout=600)
        with open(errp, "rb") as f:
            stderr = f.read()
        assert out.returncode == 0, stderr[-3000:].decode(errors="replace")
        with open(log) as f:
            calls = json.load(f)
    return out.stdout.splitlines(), stderr, calls


def _check(lib, gpu):
    out1, err1, calls1 = _run_child(lib, True)
    out0, err0, calls0 = _run_child(lib, False)
    # ---- timing changes nothing else
    assert out1 == out0
    assert len(out1) == STEPS + 2 and out1[-1].startswith("round ")
    assert [(c["call"], c["refused"], c["stats"]) for c in calls0 if c["call"] != "jobs_reprioritise"] == [(c["call"], c["refused"], c["stats"]) for c in calls1 if c["call"] != "jobs_reprioritise"]
    # ---- no variable set
    assert not [l for l in err0.decode(errors="replace").splitlines() if l.startswith("[asched ")]
    assert all(c["err"][0] == c["err"][1] for c in calls0), "an untimed call wrote to stderr"
    rep0 = [c for c in calls0 if c["call"] == "jobs_reprioritise" and not c["refused"]]
    assert rep0 and all(c["stats"]["device_ms"] == [0.0] * 4 for c in rep0)
    ev0 = [c for c in calls0 if c["call"] == "round_evictor_report"]
    assert len(ev0) == 1 and ev0[0]["timing"][6] == 0 and ev0[0]["timing"][7] == 0
    # ---- all variables set: one line of its family per call that ran passes, and nothing else
    all_lines = [l for l in err1.decode(errors="replace").splitlines() if l.startswith("[asched ")]
    seen, kinds, launched = 0, {k: 0 for k in LINES}, 0
    last_round_wall = None
    for c in calls1:
        if c["call"] == "schedule_round":
            last_round_wall = (c["handle"], c["wall_ms"])
            continue
        lines = [l for l in err1[c["err"][0]:c["err"][1]].decode(errors="replace").splitlines() if l.startswith("[asched ")]
        want = _expected(c)
        assert len(lines) == (0 if want is None else 1), (c, lines)
        seen += len(lines)
        if want is None:
            continue
        tag, named, times = _parse(lines[0])
        assert tag == TAG_OF.get(c["call"], c["call"]), (c, lines)
        kinds[tag] += 1
        if tag == "shapes_compact":
            assert named["c0"] - named["c1"] == want.pop("classes_retired") and named["f0"] - named["f1"] == want.pop("fit_retired"), (c, lines)
        for k, v in want.items():
            assert named[k] == v, (k, c, lines)
        # ---- the times
        if not gpu:
            assert times == [0.0] * len(times), lines
        else:
            wall = c["wall_ms"]
            if tag == "evict_report":
                assert last_round_wall and last_round_wall[0] == c["handle"]
                wall = last_round_wall[1]
            assert all(math.isfinite(t) and t >= 0 for t in times), lines
            assert 0 < sum(times) <= wall, (lines, wall)
            launched += 1
        if tag == "jobs_reprioritise":
            for word_ms, t in zip(c["stats"]["device_ms"], times):
                assert abs(word_ms * 1000.0 - t * 1000.0) <= 0.55 + 1e-6, (c, lines)
        if tag == "evict_report":
            assert abs(c["timing"][6] - (times[0] + times[1])) <= 1e-4 + 1e-9 and abs(c["timing"][7] - times[2]) <= 1e-4 + 1e-9, (c, lines)
    assert seen == len(all_lines), "a line outside the calls of the timed families"
    assert all(kinds[k] >= 1 for k in LINES), kinds
    assert not gpu or launched == seen
    # ---- a call that ran no pass, behind a timed one of its family
    tail = [c for c in calls1 if c["phase"] == "no pass"]
    assert [(c["call"], c["n"], c["refused"]) for c in tail] == [("jobs_reprioritise", 1, False), ("jobs_reprioritise", 0, False), ("jobs_delete", 1, False), ("jobs_delete", 0, False),
                                                                 ("nodes_delete", 1, False), ("nodes_delete", 1, True)]
    assert tail[1]["stats"]["device_ms"] == [0.0] * 4 and tail[1]["stats"]["entries"] == 0
    assert tail[3]["stats"]["rows"] == 0 and tail[3]["stats"]["num_jobs"] == tail[2]["stats"]["num_jobs"]
    assert tail[5]["stats"] == tail[4]["stats"]            # (the refusal came before anything changed)
    assert not gpu or sum(tail[0]["stats"]["device_ms"]) > 0


def test_the_pinned_seed_covers_every_family(hostsim_lib, oracle_lib):
    """from the CPU build's recording: every operation, an in-place append that brought new shapes, resident prepares"""
    import resident_sequences as RS
    import test_z_resident_sequences as TS
    assert SEED in TS.SEEDS and STEPS == TS.STEPS
    steps = TS._cpu(hostsim_lib, oracle_lib, SEED)
    ops = {s.op for s in steps}
    assert all(o in ops for o in RS.OPS), ops
    assert any(s.op == "jobs_append" and s.stats["in_place"] > 0 and s.stats["added"] > 0 and not s.stats["rebuilt"] for s in steps)
    assert any(s.resident for s in steps)


def test_pass_times_on_the_cpu_build(hostsim_lib):
    _check(hostsim_lib, gpu=False)


@pytest.mark.gpu
def test_pass_times_on_the_gpu(hip_lib):
    _check(hip_lib, gpu=True)


# ---------------------------------------------------------------- the child: argv = the library file, the seed, the file of the call log
def _child(path, seed, log_path):
    sys.path.insert(0, os.path.dirname(HERE))
    if not path.endswith("libhostsim.so"):
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
    import resident_sequences as RS
    from armada_amd.binding import Library, SchedError, Scheduler
    from test_z_jobs_reprioritise import _limits
    calls, phase = [], ["sequence"]
    first, none = (lambda a, k: len(a[0])), (lambda a, k: 0)     # the entries of a call: the length of its first argument
    size_of = dict(jobs_patch=first, jobs_reprioritise=first, jobs_append=first, req_classes_append=first, shapes_compact=none, jobs_delete=first, nodes_patch=first, nodes_delete=first,
                   nodes_append=first, round_prepare_resident=lambda a, k: 0 if k.get("held") is None else len(k["held"]), round_evictor_report=none, schedule_round=none)

    def wrap(name):
        inner = getattr(Scheduler, name)

        def outer(self, *a, **k):
            rec = dict(call=name, phase=phase[0], handle=id(self), M=int(self.num_jobs), N=int(self.num_nodes), n=int(size_of[name](a, k)), refused=False, stats=None)
            if name == "nodes_patch":
                rec["words"] = len({int(v) >> 6 for v in np.atleast_1d(a[0])})
            if name == "round_prepare_resident":
                rec["queues"] = len(a[0])
            e0 = os.fstat(2).st_size
            t0 = time.perf_counter()
            try:
                return_value = inner(self, *a, **k)
            except SchedError:
                rec["refused"] = True
                raise
            finally:
                rec["wall_ms"] = (time.perf_counter() - t0) * 1000.0
                rec["err"] = [e0, os.fstat(2).st_size]
                calls.append(rec)
                if name == "round_prepare_resident" and not rec["refused"]:
                    rec["queued"] = int(sum(len(x) for x in self.round_queued()))
                elif name == "round_evictor_report" and not rec["refused"]:
                    t = self.round_timing()
                    rec["timing"] = [t["total_ms"], t["control_ms"], t["launches"], t["evict1_host_ms"], t["evict3_host_ms"], t["final_host_ms"], t["evr_job_node_ms"], t["evr_queue_ms"]]
                elif name not in ("jobs_patch", "schedule_round", "round_prepare_resident", "round_evictor_report") and not (rec["refused"] and name != "nodes_delete"):
                    rec["stats"] = getattr(self, name + "_stats")()
            if name == "round_evictor_report":
                rec["stats"] = dict(evicted=int(return_value["num_evicted"]))
            return return_value
        setattr(Scheduler, name, outer)

    for name in size_of:
        wrap(name)
    L = Library(path, "asched_")
    for s in RS.run_sequence(L, L, seed, max_steps=STEPS):
        print(s.line())
    # ---- a second handle of the seed's start table: the calls that run no pass behind timed ones, then a round with the evictor report on
    cur = RS.start_table(seed, np.random.default_rng(seed))
    a = RS.fresh(L, cur)
    phase[0] = "no pass"
    a.jobs_reprioritise([0], int(cur.qprio[0]) + 1)
    a.jobs_reprioritise([], 0)
    queued = np.nonzero(np.asarray(cur.job_node) < 0)[0]
    a.jobs_delete([int(queued[-1])])
    a.jobs_delete([])
    run = np.asarray(cur.job_node)[np.asarray(cur.job_node) >= 0]
    free = RS._free_nodes(cur)
    assert len(run) and len(free), "the start table of the seed has no run or no free node: the case pins nothing"
    a.nodes_delete([int(free[-1])])
    node_with_a_run = int(run[0]) - int(free[-1] < run[0])
    try:
        a.nodes_delete([node_with_a_run])
        raise AssertionError("nodes_delete of a node with a run was not refused")
    except SchedError:
        pass
    phase[0] = "round"
    a.close()
    b = RS.fresh(L, cur)
    b.set_evictor_report(True)
    b.round_prepare_resident(cur.queue_weight, held=np.nonzero(cur.held)[0].astype(np.int32), **_limits(cur))
    r = b.schedule_round()
    rep = b.round_evictor_report()
    print("round", json.dumps(dict(scheduled=sorted((int(j), int(n)) for j, n in r.scheduled.items()), preempted=sorted(int(j) for j in r.preempted), evicted=int(rep["num_evicted"]),
                                   evicted_job=rep["evicted_job"].tolist(), node_evicted=rep["node_evicted_jobs"].tolist(), fair=r.fair_share.tolist())))
    b.close()
    with open(log_path, "w") as f:
        json.dump(calls, f)


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]), sys.argv[3])
