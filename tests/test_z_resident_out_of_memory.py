"""The nine resident table calls refused for device memory, on the CPU build: asched_jobs_patch, asched_jobs_reprioritise, asched_jobs_append, asched_req_classes_append,
asched_shapes_compact, asched_jobs_delete, asched_nodes_patch, asched_nodes_delete and asched_nodes_append each promise that a call which cannot get a device block is
refused with ASCHED_ERR_DEVICE and "the handle is as it was".  On a GPU nobody exhausts the memory of a shared machine; the CPU build can refuse any single allocation
a resident call may be refused for (tests/hostsim/hostsim.cpp: hostsim_try_malloc_fail_at(k) makes the k-th plat_try_malloc from now return nullptr once,
hostsim_try_malloc_seen() counts them since arming).

Per call: a small table of tests/resident_sequences.py (start_table) with the operations that bring the handle into the state the case needs, then the call's argument
as the module's drawer draws it from a pinned seed — chosen so that the call needs every kind of block it has, which the unarmed run on a second handle asserts from
the call's statistics and from the number of allocations it made.  Then the sweep k = 0, 1, 2, ...: the hook is armed at k and the same call is made on ONE handle.
While the hook fires the call must be refused as documented, and the handle must answer what it answered before (view, round, unfeasible keys, fair shares, fast
iterations) and what a fresh handle of the unchanged model answers.  The first k the hook does not fire at ends the sweep: that call succeeds, makes exactly as many
allocations as the unarmed run did — a refused attempt neither consumed nor kept the call's scratch — and the handle is compared with a fresh handle of the changed
model and with the oracle, as resident_sequences.run_sequence does.  Every k below the unarmed count is refused, so a block-staging call is refused at its first staged
block, at its last and at every one in between.

(The view is only defined while the last successful call was a resident call or jobs_set, and every check ends with a round: an empty nodes_patch, which allocates
nothing, stands in front of every armed call.)"""
import ctypes

import numpy as np
import pytest

import resident_sequences as RS
from armada_amd.binding import SchedError

ERR_DEVICE = -3
AS_IT_WAS = "the handle is as it was"
# the calls that stage a block per array of the table: refused at the first staged block, the last and one in between needs at least three behind the scratch
# (nodes_delete: the scratch and the keep flags)
STAGING = {"jobs_append": 1, "jobs_delete": 1, "nodes_delete": 2, "nodes_append": 1}


class Case:
    def __init__(self, call, table, draw, setup=(), want=None, single=False, blocks=None):
        self.call, self.table, self.draw, self.setup, self.want, self.single, self.blocks = call, table, draw, setup, want or {}, single, blocks

    @property
    def op(self):
        return "apply_round" if self.call == "jobs_patch" else self.call


# table: the seed of start_table; setup: operations drawn from the table's generator first; draw: the seed the call's argument is drawn from; want: the statistics of
# the unarmed call that say every kind of block was needed; single: the call has one allocation, its scratch (the direct form); blocks: the allocations of a call that
# stages them by hand (shapes_compact: the scratch, the shape mask and, where a class is retired, the class mask).
# Table 36 has 40 rows on 64 nodes.  nodes_append starts from 130 nodes and goes past 192: from 64 or 128 nodes the rank field of the node keys is full and the call
# takes nodes_upsert's path (reason 5), which stages nothing
CASES = {
    "jobs_patch": Case("jobs_patch", table=36, draw=0, single=True),
    "jobs_reprioritise": Case("jobs_reprioritise", table=36, draw=0, single=True, want=dict(made_resident=1)),
    "jobs_append in place": Case("jobs_append", table=36, draw=0, want=dict(in_place=True, rebuilt=0, reallocated=1, new_gangs=True, new_shapes=True)),
    "jobs_append rebuilt": Case("jobs_append", table=36, draw=2, want=dict(in_place=False, rebuilt=1, reallocated=1, new_gangs=True, new_shapes=True)),
    "req_classes_append": Case("req_classes_append", table=36, draw=0, want=dict(rebuilt=0)),
    "shapes_compact": Case("shapes_compact", table=36, draw=2, setup=("jobs_delete",), want=dict(shapes_retired=True, classes_retired=True, rebuilt=0), blocks=3),
    "jobs_delete": Case("jobs_delete", table=36, draw=0),
    "nodes_patch": Case("nodes_patch", table=36, draw=0, single=True, want=dict(rebuilt=0)),
    "nodes_delete": Case("nodes_delete", table=36, draw=0, want=dict(rebuilt=0)),
    "nodes_append": Case("nodes_append", table=29, draw=7, want=dict(rebuilt=0, restrided=1)),
}
REFUSED = {}


def _hook(lib):
    arm, seen = lib.lib.hostsim_try_malloc_fail_at, lib.lib.hostsim_try_malloc_seen
    arm.argtypes, arm.restype, seen.argtypes, seen.restype = [ctypes.c_int], None, [], ctypes.c_int
    return arm, seen


def _tail(cur):
    return np.arange(max(cur.num_jobs - 8, 0), cur.num_jobs)


def _prepared(L, case):
    """a handle in the state the case starts from -> (handle, model, generator state, what the handle answers)"""
    rng = np.random.default_rng(case.table)
    cur = RS.start_table(case.table, rng)
    st = dict(new_reqs=0, next_gang=10_000, next_submit=int(cur.job_submit.max()) + 1, next_index=100_000, ts=int(cur.job_run_ts.max()), job_cap=cur.num_jobs, halved=False,
              last_round=None)
    a = RS.fresh(L, cur)
    for op in case.setup:
        cur, _, _ = RS._RUN[op](a, cur, rng, st)
    v, r, rst, u = RS._answers(a, cur, _tail(cur), True)
    st["last_round"] = r
    return a, cur, st, ((v, r, u), rst["fast_iterations"])


def _call(a, case, cur, st):
    """the case's call with the argument its seed draws: the same one every time (the drawers edit copies of the model; a refused call raises before they return)"""
    a.nodes_patch([])
    after, detail, stats = RS._RUN[case.op](a, cur, np.random.default_rng(case.draw), dict(st))
    if case.call == "jobs_append":
        stats = dict(stats, new_gangs=a.jobs_append_stats()["new_gangs"])
    return after, detail, stats


def _unarmed(L, case):
    """the call on a second handle with the hook counting only -> (its statistics, the allocations it made)"""
    arm, seen = _hook(L)
    b, cur, st, _ = _prepared(L, case)
    try:
        arm(1 << 30)
        _, _, stats = _call(b, case, cur, st)
        return stats, seen()
    finally:
        arm(-1)
        b.close()


def _needs_every_block(case, stats, total):
    for k, v in case.want.items():
        assert (stats[k] > 0) if v is True else (stats[k] == 0) if v is False else (stats[k] == v), (k, stats)
    if case.single or case.blocks:
        assert total == (case.blocks or 1), total
    else:
        assert total > 1, total
    if case.call in STAGING:
        assert total - STAGING[case.call] >= 3, f"{total} allocations: no first, last and in-between staged block to refuse"


@pytest.mark.parametrize("name", list(CASES))
def test_refused_for_memory_the_handle_is_as_it_was(hostsim_lib, oracle_lib, name):
    L, case = hostsim_lib, CASES[name]
    arm, seen = _hook(L)
    stats, total = _unarmed(L, case)
    _needs_every_block(case, stats, total)
    a, cur, st, (want, fast) = _prepared(L, case)
    refused = 0
    try:
        RS._against_fresh(L, cur, _tail(cur), True, want, fast)
        for k in range(total + 1):
            arm(k)
            try:
                after, _, got_stats = _call(a, case, cur, st)
                made, err = seen(), None
            except SchedError as e:
                made, err = seen(), e
            finally:
                arm(-1)
            if made <= k:            # the hook did not fire: the sweep ends with the call that goes through
                assert err is None, f"k={k}: the call failed although every allocation succeeded: {err}"
                assert made == total, f"after {refused} refusals the call made {made} allocations, the unarmed run {total}: a refused attempt consumed or kept a block"
                assert got_stats == stats, (got_stats, stats)
                break
            assert err is not None and err.code == ERR_DEVICE and AS_IT_WAS in str(err), f"k={k}: refused allocation {k} of {total}, the call gave {err}"
            refused += 1
            assert a.num_jobs == cur.num_jobs and a.num_nodes == cur.num_nodes
            v, r, rst, u = RS._answers(a, cur, _tail(cur), True)
            RS._compare((v, r, u), want, f"what the handle answered before refusal {k}")
            assert rst["fast_iterations"] == fast, f"k={k}: fast iterations {rst['fast_iterations']}, before the refusal {fast}"
            RS._against_fresh(L, cur, _tail(cur), True, (v, r, u), rst["fast_iterations"])
        else:
            raise AssertionError(f"the hook still fired at k={total}, past the {total} allocations of the unarmed run")
        assert refused == total and refused >= 1
        REFUSED[name] = refused
        print(f"{name}: {refused} refusals")
        assert a.num_jobs == after.num_jobs and a.num_nodes == after.num_nodes
        v, r, rst, u = RS._answers(a, after, _tail(after), True)
        RS._against_fresh(L, after, _tail(after), True, (v, r, u), rst["fast_iterations"])
        RS._against_oracle(oracle_lib, after, r)
    finally:
        a.close()
