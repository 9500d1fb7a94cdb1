"""The resident table calls under seeded interleavings (tests/resident_sequences.py): jobs_append (also in place, also whole gangs), jobs_delete (first and last row,
whole shapes, whole and partial gangs), the last round applied with jobs_patch, jobs_reprioritise, req_classes_append, shapes_compact (with and without classes),
nodes_patch (cordon, capacity, taint), nodes_delete and nodes_append, in one sequence on one handle, with a round prepared from explicit lists or with
round_prepare_resident after every operation and, at a low rate, a call the library must refuse.  What the per-call test files do not vary is what the calls share:
capacities that only grow, the two order buffers that swap, keep flags sized by an older M or N, scratch kept across calls, blocks whose stride a delete changes, the
host mirrors and the choice between the in-place and the rebuild path, which each call makes from the state an earlier call left.

CPU build: 60 pinned seeds of 40 operations, the full comparison with a fresh handle of the model and with the oracle's round after every operation.
GPU: 24 of those seeds replayed on the HIP library; after every operation its answers and its call's statistics must equal the CPU build's recorded ones (the same
path, so a silent rebuild does not pass), and a fresh HIP handle is compared after the first rebuild, at the middle and at the end.
test_the_pinned_seeds_are_not_trivial keeps the seed list from going quiet (computed from the CPU build's recordings only).

`python tests/soak.py resident N` runs the same runner on seeds 100000 and up.  Outcome on the CPU build: 3000 seeds (120 000 operations), 0 divergences, 323 s; 300 more with
HS_RING_LAG=7 (the serial node engine lags behind the merge in every round), 0 divergences (profiles/r24_resident_sequences.txt).
Mutations of the library tried in a scratch copy against the pinned seeds (CPU build): a job delete that leaves one keep flag at 0 fails 16 of the 60 seeds, a node
delete whose gather is strided by Npad instead of Npad1 fails 49; jobs_patch without the swap of ordCap and ordSpareCap fails none, here and under the sanitizer
program: every path that allocates one of the two order buffers sizes it like the other, so in every state these seeds and 400 more reached the two capacities were
equal when they swapped — the mutant computes the same thing.

A failing seed prints its operations with their statistics; resident_sequences.run_sequence(lib, oracle, seed, max_steps=k) cuts it to a prefix."""
import numpy as np
import pytest

import resident_sequences as RS
from armada_amd import workloads as W
from test_z_jobs_append_shapes import _view

SEEDS = [1, 2, 3, 5, 10, 11, 12, 13, 14, 21, 22, 23, 25, 26, 27, 28, 30, 31, 33, 34, 35, 40, 42, 45, 46, 49, 52, 55, 56, 57, 61, 62, 66, 68, 69, 73, 78, 79, 81, 82, 85, 90, 91, 92,
         93, 99, 101, 103, 105, 108, 112, 113, 114, 117, 120, 130, 131, 136, 142, 163]
GPU_SEEDS = SEEDS[::5] + SEEDS[2::5]
STEPS = 40
assert len(SEEDS) == 60 and len(set(GPU_SEEDS)) == 24

_RECORDED = {}


def _cpu(hostsim_lib, oracle_lib, seed):
    """the CPU build's run of a pinned seed, once per session: the Steps, or the failure it raised"""
    if seed not in _RECORDED:
        try:
            _RECORDED[seed] = RS.run_sequence(hostsim_lib, oracle_lib, seed, max_steps=STEPS)
        except RS.SequenceFailure as e:
            _RECORDED[seed] = e
    if isinstance(_RECORDED[seed], Exception):
        raise _RECORDED[seed]
    return _RECORDED[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_on_the_cpu_build(hostsim_lib, oracle_lib, seed):
    steps = _cpu(hostsim_lib, oracle_lib, seed)
    assert len(steps) == STEPS + 1


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_sequence_replayed_on_the_gpu(hip_lib, hostsim_lib, oracle_lib, seed):
    recorded = _cpu(hostsim_lib, oracle_lib, seed)
    steps = RS.run_sequence(hip_lib, oracle_lib, seed, max_steps=STEPS, recorded=recorded)
    assert [s.line() for s in steps] == [s.line() for s in recorded]


def test_the_pinned_seeds_are_not_trivial(hostsim_lib, oracle_lib):
    """conditions that keep the suite from going quiet, not measurements: from the CPU build's recordings of the pinned seeds"""
    c = RS.coverage([_cpu(hostsim_lib, oracle_lib, seed) for seed in SEEDS])
    for op in RS.OPS:
        assert c[f"op {op}"] >= 20, (op, c)
    assert c["append in place"] >= 10 and c["append rebuilt"] >= 10, c
    assert c["append grew jobCap"] >= 5 and c["append grew jobCap after a halving delete"] >= 2, c
    for edge in (64, 128):
        assert c[f"nodes_delete across {edge}"] >= 3 and c[f"nodes_append across {edge}"] >= 3, c
    assert c["one node"] >= 1, c
    assert c["compact retired a shape"] >= 10 and c["compact retired a class"] >= 3, c
    for kind in RS.REFUSALS:
        assert c[f"refusal {kind}"] >= 2, (kind, c)
    assert c["rounds that placed a job"] >= 0.8 * c["checks"], c
    assert 0.3 * c["checks"] <= c["resident prepares"] <= 0.7 * c["checks"], c


# ---------------------------------------------------------------- queries after a round
@pytest.fixture(params=["hostsim", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "hip_lib")


RESIDENT_CALLS = {
    "jobs_patch": lambda a, cur: a.jobs_patch([], []),
    "jobs_append": lambda a, cur: a.jobs_append(np.zeros((0, 4), np.int64)),
    "jobs_delete": lambda a, cur: a.jobs_delete([]),
    "jobs_reprioritise": lambda a, cur: a.jobs_reprioritise([0], int(cur.qprio[0])),
    "req_classes_append": lambda a, cur: a.req_classes_append([]),
    "shapes_compact": lambda a, cur: a.shapes_compact(),
    "nodes_patch": lambda a, cur: a.nodes_patch([]),
    "nodes_delete": lambda a, cur: a.nodes_delete([]),
    "nodes_append": lambda a, cur: a.nodes_append(np.zeros((0, 4), np.int64), index=[]),
}


def test_after_a_round_any_resident_call_brings_the_view_back(lib):
    """the NodeDb-level queries and the submit check read the NodeDb as the last call left it: a round leaves its placements bound, a resident call — here each with
    nothing to change — leaves what jobs_set leaves, no job bound.  (round_prepare is no such call: it binds the running jobs, as populateNodeDb does)"""
    cur = RS.start_table(5, np.random.default_rng(5))
    tail = np.arange(cur.num_jobs - 8, cur.num_jobs)
    f = RS.fresh(lib, cur)
    want = _view(f, cur, tail)
    f.close()
    a = RS.fresh(lib, cur)
    for name, call in RESIDENT_CALLS.items():
        W.prepare(a, cur)
        r = a.schedule_round()
        assert len(r.scheduled) > 0, "the round placed nothing: the case pins nothing"
        call(a, cur)
        assert _view(a, cur, tail) == want, name
    a.close()
