"""bench.py's output contract, checked without a GPU: torch.cuda and armada_amd.load_library are monkeypatched so that the CPU build of the
device code stands in for the HIP library (test-only; bench.py itself refuses to run without the MI355X).  Guards the JSON line — the keys
the driver and the judge read — for the round bench and for `--submit-check`, at toy sizes."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"}
ROOFLINE_KEYS = {"bound", "achieved", "peak", "unit", "frac", "traffic"}
CPU_KEYS = {"value", "unit", "cores", "kind", "sample"}


@pytest.fixture
def fake_gpu(monkeypatch, hostsim_lib):
    import torch
    import armada_amd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    real_zeros = torch.zeros
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: real_zeros(*a, **{x: y for x, y in k.items() if x != "device"}))
    monkeypatch.setattr(armada_amd, "load_library", lambda: hostsim_lib)
    sys.path.insert(0, ROOT)
    for v in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(v, raising=False)
    import bench
    return bench


def check_line(out, metric_word):
    """the LAST stdout line is the compact record the driver parses (round 4's 28 kB line did not fit its 8 kB capture: `parsed: null`); the line before it — and
    bench_full.json — is the full record.  Returns the full record after checking that both carry the contract's keys and agree."""
    lines = out.strip().splitlines()
    last = lines[-1]
    assert len(last) <= 4000, len(last)
    assert json.loads(out[-8000:].strip().splitlines()[-1]) == json.loads(last)   # what a capture of the final 8 000 characters yields
    compact, line = json.loads(last), json.loads(lines[-2])
    assert ROUND_KEYS <= set(compact), ROUND_KEYS - set(compact)
    assert ROOFLINE_KEYS <= set(compact["roofline"]) and CPU_KEYS <= set(compact["cpu_baseline"])
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert compact[k] == line[k], k
    assert abs(compact["value"] - line["value"]) <= 1e-3 * abs(line["value"]) and abs(compact["roofline"]["frac"] - line["roofline"]["frac"]) <= 1e-3 * abs(line["roofline"]["frac"]) + 1e-12
    timed0 = line.get("device_s", 0) > 0 or (line.get("round") or {}).get("device_ms", 0) > 0   # (the CPU build has no HIP events: no launch duration to price)
    assert not timed0 or compact["roofline"]["frac"] <= 1.0, compact["roofline"]   # a fraction above 1 says the kernel did not do the work it is priced on
    assert compact["parity"]["identical"] == line["parity"]["identical"]
    if "other_configs" in line:
        assert [r[0] for r in compact["other_configs"]] == [r["config"][:40] for r in line["other_configs"]] and "other_configs_truncated" not in compact
        for row, full in zip(compact["other_configs"], line["other_configs"]):
            assert row[5] == (full.get("parity") or {}).get("identical"), row
            timed = full.get("device_ms", 0) > 0 or full.get("device_s", 0) > 0   # (the CPU build has no HIP events: no launch duration to price)
            assert row[4] is None or not timed or row[4] <= 1.0, row
    with open(os.path.join(ROOT, "bench_full.json")) as f:
        assert json.loads(f.read()) == line
    assert ROUND_KEYS <= set(line), ROUND_KEYS - set(line)
    assert metric_word in line["metric"] and line["n_gpus"] == 1 and line["higher_is_better"] is True and line["scaling"] == "weak"
    assert line["vs_baseline"] is None and line["dtype"] == "int64" and line["data"] == "synthetic" and "workload" in line["config"]
    assert ROOFLINE_KEYS <= set(line["roofline"]) and line["roofline"]["bound"] == "hbm" and line["roofline"]["peak"] == 8000.0
    assert CPU_KEYS <= set(line["cpu_baseline"]) and line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] == 1
    assert line["value"] > 0
    return line


def test_round_bench_line(fake_gpu, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--nodes", "500", "--jobs", "5000", "--queues", "8", "--steps", "2", "--warmup", "1", "--cpu-budget", "5", "--other-scale", "0.01", "--full"])
    fake_gpu.main()
    line = check_line(capsys.readouterr().out, "rounds/sec")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "rounds/s" and line["round"]["scheduled"] > 0
    # the headline is self-verifying: the timed round is compared with the oracle round of the cpu_baseline leg
    assert line["parity"] == dict(line["parity"], checked=True, identical=True) and line["parity"]["jobs"] > 5000
    ex = line["parity"]["excluded_nodes"]   # why a job found no node: the records of the timed round against the oracle's walk, for a sample of the failed jobs
    assert ex["checked"] and ex["identical"] and ex["jobs"] > 0 and ex["with_a_failed_selection_on_record"] >= 0, ex   # (the toy round's failures are rate limits: none may have a record)
    assert 1 <= line["cpu_baseline"]["rounds"] <= 3 and line["cpu_baseline"]["upper_bound_extrapolation"] is False   # (up to three oracle rounds when a round is short)
    # every other BASELINE config + the submit check sits in the same record, each with roofline and cpu_baseline
    oc = {r["config"]: r for r in line["other_configs"]}
    assert set(oc) == {"BASELINE configs[1]", "BASELINE configs[3]", "BASELINE configs[4]", "submit check (SURVEY 8f-2)", "fairness optimiser node scoring (SURVEY 8f-3)",
                       "market-driven round + indicative gang pricer (SURVEY 8f-4)", "two-word order keys (SURVEY a4)", "fine resolutions, round requests: coarser exact key divisor (SURVEY a4)", "one pool on two replicas, wide passes split (SURVEY 8e)", "256 queues (beyond the 64-lane fast iteration)", "1024 queues", "256 queues on a crowded pool (95 % occupied: most new jobs need preemption)", "BenchmarkScheduleMany shapes (nodedb_test.go:1590-1712)",
                       "nodedb fit kernel at 100 000 nodes x 1 000 000 queries", "configs[4] shape at 100 000 nodes with the reference's default limits (checker)",
                       "BenchmarkPreemptingQueueScheduler shapes (preempting_queue_scheduler_test.go:2561-2799)"}, set(oc)
    ref = oc.pop("BenchmarkPreemptingQueueScheduler shapes (preempting_queue_scheduler_test.go:2561-2799)")   # a table of eight small shapes: rows instead of one roofline
    assert "error" not in ref and len(ref["rows"]) == 8 and ref["parity"]["identical"] and all(r["steady_state"]["scheduled"] == 0 and r["steady_state"]["preempted"] == 0 for r in ref["rows"])
    sm = oc.pop("BenchmarkScheduleMany shapes (nodedb_test.go:1590-1712)")   # the reference's nodedb benchmark: a table of nine shapes
    assert "error" not in sm and len(sm["rows"]) == 9 and sm["parity"]["identical"] and any(r["how"] == "capacity pass" for r in sm["rows"]), sm
    assert "skipped" in oc.pop("one pool on two replicas, wide passes split (SURVEY 8e)")   # (two round kernels side by side: the HIP library only)
    tw = oc["two-word order keys (SURVEY a4)"]
    assert tw["parity"]["identical"] and tw["round"]["fast_iterations"] == 0 and tw["round"]["scheduled"] > 0, tw
    cd = oc["fine resolutions, round requests: coarser exact key divisor (SURVEY a4)"]
    assert cd["parity"]["identical"] and cd["round"]["fast_iterations"] > 0, cd
    chk = oc["configs[4] shape at 100 000 nodes with the reference's default limits (checker)"]
    assert chk["steps"] == 3 and chk["p99_ms"] >= chk["p50_ms"] > 0 and "kclk_plane_scans_plus_fair_selects" in chk["round"]
    assert "passes_executed" in line["round"]
    for name, r in oc.items():
        assert "error" not in r and "skipped" not in r, r
        assert ROOFLINE_KEYS <= set(r["roofline"]) and CPU_KEYS <= set(r["cpu_baseline"]), name
        if "parity" in r:
            assert r["parity"]["checked"] and r["parity"]["identical"], (name, r["parity"])
    assert oc["BASELINE configs[1]"]["roofline"]["kernel"] == "k_fit_batch" and oc["BASELINE configs[1]"]["parity"]["identical"]
    # configs[3] is checked against the oracle at the size its value is quoted on (no `reduced` leg any more); configs[4] keeps the reduced leg; the submit check carries a verdict too
    assert oc["BASELINE configs[3]"]["parity"]["identical"] and "reduced" not in oc["BASELINE configs[3]"] and oc["BASELINE configs[3]"]["round"]["generic_iterations"] > 0
    assert oc["BASELINE configs[4]"]["reduced"]["parity"]["identical"]
    assert oc["submit check (SURVEY 8f-2)"]["parity"]["identical"] and oc["submit check (SURVEY 8f-2)"]["parity"]["jobs"] > 0
    assert line["cpu_baseline"]["pinned_core"] is not None
    mk = oc["market-driven round + indicative gang pricer (SURVEY 8f-4)"]
    assert mk["parity"]["identical"] and mk["round"]["scheduled"] > 0 and mk["pricer"]["gangs_priced"] >= 0


def test_round_bench_detects_a_mismatch(fake_gpu, monkeypatch, capsys):
    """a GPU round that differs from the oracle's makes bench.py say so in the line and exit non-zero"""
    real = fake_gpu.round_diff
    monkeypatch.setattr(fake_gpu, "round_diff", lambda a, b: real(a, b) + ["scheduled (injected)"])
    monkeypatch.setattr(sys, "argv", ["bench.py", "--nodes", "300", "--jobs", "3000", "--queues", "4", "--steps", "1", "--warmup", "0", "--cpu-budget", "5", "--no-other", "--full"])
    rc = fake_gpu.main()
    lines = capsys.readouterr().out.strip().splitlines()
    line, compact = json.loads(lines[-2]), json.loads(lines[-1])
    assert rc == 3 and line["parity"]["checked"] and not line["parity"]["identical"] and "other_configs" not in line
    assert compact["parity"]["checked"] and compact["parity"]["identical"] is False


PLAIN = ["bench.py", "--gpus", "1", "--nodes", "500", "--jobs", "5000", "--queues", "8", "--steps", "3", "--warmup", "2"]


def _forbid_extras(bench, monkeypatch):
    """a plain run does only what the headline needs: none of the --full legs may start"""
    def refuse(*a, **k):
        raise AssertionError("a plain bench run started a --full leg")
    for name in ("cpu_baseline", "other_configs", "kernel_isa_hash", "emit"):
        monkeypatch.setattr(bench, name, refuse)


def test_plain_round_bench_line(fake_gpu, monkeypatch, capsys):
    """without --full: exactly --warmup + --steps rounds, one stdout line with the headline keys, no oracle leg, roofline or sub-records"""
    from armada_amd import workloads as W
    _forbid_extras(fake_gpu, monkeypatch)
    prepared = []
    real_prepare = W.prepare
    monkeypatch.setattr(W, "prepare", lambda *a, **k: (prepared.append(1), real_prepare(*a, **k))[1])
    monkeypatch.setattr(sys, "argv", PLAIN)
    assert (fake_gpu.main() or 0) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and len(prepared) == 2 + 3
    line = json.loads(lines[0])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "round"} <= set(line), line
    assert not {"roofline", "cpu_baseline", "parity", "other_configs"} & set(line), line
    assert "rounds/sec" in line["metric"] and line["unit"] == "rounds/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["round"]["scheduled"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]   # one pool: rounds/s and ms per timed round say the same


def test_dump_outputs(fake_gpu, monkeypatch, capsys, oracle_lib, tmp_path):
    """--dump-outputs: the last timed round's results as float64 .npy, one entry per job where the round returns lists (no file empty, every shape set by the
    input), the same on every run with the same arguments, and the oracle's round on that input"""
    import numpy as np
    from armada_amd import workloads as W
    from armada_amd.multipool import pool_seed
    _forbid_extras(fake_gpu, monkeypatch)
    dumps = []
    for run in ("a", "b"):
        monkeypatch.setattr(sys, "argv", PLAIN + ["--dump-outputs", str(tmp_path / run)])
        fake_gpu.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        dumps.append({f[:-4]: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    a, b = dumps
    wl = W.config3(n_nodes=500, n_jobs=5000, n_queues=8, seed=pool_seed(W.SEED, 0), gangs=0, occupied=0.5)   # bench.py main()'s input
    wl.global_burst, wl.queue_burst = max(1, int(200_000 * 0.005)), max(1, int(20_000 * 0.005))
    m, q = wl.num_jobs, wl.num_queues
    shapes = {"job_scheduled_node": (m,), "job_scheduled_priority": (m,), "job_scheduled_method": (m,), "job_preempted_node": (m,), "job_unschedulable_reason": (m,),
              "queue_allocated_by_pc": (q, len(wl.config.pc_priority), W.R), "fair_share": (q,), "demand_capped_adjusted_fair_share": (q,), "uncapped_adjusted_fair_share": (q,),
              "queue_tokens_after": (q,), "termination_reason": (1,), "num_evicted_phase1": (1,), "num_evicted_phase3": (1,), "global_tokens_after": (1,)}
    assert {k: x.shape for k, x in a.items()} == shapes and all(x.dtype == np.float64 and x.size > 0 for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64_000_000
    assert a.keys() == b.keys() and all(np.array_equal(a[f], b[f]) for f in a)
    assert int((a["job_scheduled_node"] >= 0).sum()) == line["round"]["scheduled"] > 0
    s = W.load(oracle_lib, wl)
    W.prepare(s, wl)
    want = s.schedule_round()
    node, prio, meth, pre = np.full(m, -1), np.zeros(m), np.zeros(m), np.full(m, -1)
    node[want.scheduled_job], prio[want.scheduled_job], meth[want.scheduled_job] = want.scheduled_node, want.scheduled_priority_arr, want.scheduled_method_arr
    pre[want.preempted_job] = want.preempted_node
    assert np.array_equal(a["job_scheduled_node"], node) and np.array_equal(a["job_scheduled_priority"], prio) and np.array_equal(a["job_scheduled_method"], meth)
    assert np.array_equal(a["job_preempted_node"], pre) and np.array_equal(a["job_unschedulable_reason"], want.job_unschedulable_reason)
    assert np.array_equal(a["queue_allocated_by_pc"], want.queue_allocated_by_pc) and np.array_equal(a["fair_share"], want.fair_share)
    assert a["termination_reason"].tolist() == [want.termination_reason] and a["global_tokens_after"].tolist() == [want.global_tokens_after]


def test_dump_outputs_samples_over_the_limit(fake_gpu, monkeypatch, tmp_path):
    """over the size limit the per-job arrays keep a fixed sample of the jobs, the same jobs in every array, with the jobs named"""
    import numpy as np
    monkeypatch.setattr(fake_gpu, "DUMP_LIMIT", 64 * 1024)
    m = 100_000
    rng = np.random.default_rng(1)
    jobs = np.sort(rng.choice(m, 4000, replace=False)).astype(np.int32)
    res = type("R", (), dict(scheduled_job=jobs, scheduled_node=jobs % 97, scheduled_priority_arr=jobs % 3, scheduled_method_arr=np.ones(4000, np.int32),
                             preempted_job=np.zeros(0, np.int32), preempted_node=np.zeros(0, np.int32), queue_allocated_by_pc=np.arange(96, dtype=np.int64).reshape(2, 3, 16),
                             job_unschedulable_reason=np.arange(m, dtype=np.int32) % 5, fair_share=np.ones(2), demand_capped_adjusted_fair_share=np.ones(2),
                             uncapped_adjusted_fair_share=np.ones(2), queue_tokens_after=np.zeros(2), termination_reason=3, num_evicted_phase1=0, num_evicted_phase3=0,
                             global_tokens_after=1.5))
    for run in ("a", "b"):
        fake_gpu.dump_outputs(res, str(tmp_path / run))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sum(x.nbytes for x in got.values()) <= 64 * 1024 and all(x.dtype == np.float64 and x.size > 0 for x in got.values())
    idx = got["job_sample_index"].astype(np.int64)
    assert len(idx) > 100 and np.all(np.diff(idx) > 0) and all(len(got[k]) == len(idx) for k in got if k.startswith("job_"))
    node = np.full(m, -1); node[jobs] = jobs % 97
    prio = np.zeros(m); prio[jobs] = jobs % 3
    assert np.array_equal(got["job_scheduled_node"], node[idx]) and np.array_equal(got["job_scheduled_priority"], prio[idx])
    assert np.array_equal(got["job_unschedulable_reason"], idx % 5) and np.all(got["job_preempted_node"] == -1)
    assert got["queue_allocated_by_pc"].shape == (2, 3, 16) and got["global_tokens_after"].tolist() == [1.5]
    assert all(np.array_equal(got[f], np.load(tmp_path / "b" / (f + ".npy"))) for f in got)   # the same sample every time


def test_submit_check_bench_line(fake_gpu, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--submit-check", "--nodes", "500", "--submit-jobs", "1500", "--submit-keys", "120", "--steps", "1", "--cpu-budget", "5"])
    fake_gpu.main()
    line = check_line(capsys.readouterr().out, "submit checks")
    assert line["parity"]["checked"] and line["parity"]["identical"]
    assert line["unit"] == "jobs/s" and line["how"][0]["wide_units"] == 120 and line["how"][0]["sequential_units"] == 0 and line["how"][1]["gang_units"] > 0 and line["how"][1]["sequential_units"] == 0   # gang units: one workgroup each (csrc/submit_gang.h)


def test_smoke_entry_point(fake_gpu, capsys):
    """__graft_entry__.smoke(): one small round through the library, checked against the oracle (here: the CPU build stands in)"""
    import __graft_entry__ as g
    g.smoke()
    assert "smoke ok" in capsys.readouterr().out


def test_watchdog_prints_the_record_as_it_stands(fake_gpu, monkeypatch, capsys):
    """a sub-record that never returns (a hung kernel) must not take the headline down: after --watchdog seconds the record is printed with what has finished"""
    import time
    bench = fake_gpu
    exits = []
    monkeypatch.setattr(os, "_exit", lambda code: exits.append(code))
    out = {"metric": "scheduling rounds/sec", "value": 2.0, "unit": "rounds/s", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": 500.0, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "int64", "data": "synthetic", "config": {"workload": "toy"},
           "roofline": {"bound": "hbm", "achieved": 1.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.000125, "traffic": None}, "cpu_baseline": {"value": 0.01, "unit": "rounds/s", "cores": 1, "kind": "port", "sample": "x"},
           "other_configs": [{"config": "BASELINE configs[1]", "value": 1.0, "unit": "ms"}]}
    bench.watchdog_arm(out, 0.05)
    time.sleep(0.5)
    bench.watchdog_disarm()
    assert exits == [5]
    lines = capsys.readouterr().out.strip().splitlines()
    compact, full = json.loads(lines[-1]), json.loads(lines[-2])
    assert "did not return" in compact["watchdog"] and compact["value"] == 2.0 and compact["other_configs"][0][0] == "BASELINE configs[1]"
    assert full["other_configs"] == out["other_configs"] and "watchdog" in full
