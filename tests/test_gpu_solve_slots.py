"""Solve slots: pipelined cold solves of one wave-per-problem handle share the device, two at a time, each on its own
set of state arrays and its own stream.  Nothing a caller can read may change: every sequence of tests/solve_slots_cases.py is run
here pipelined, under the default, and compared BITWISE (np.array_equal) with the same sequence run with blocking solves on a
handle created under MI_ILQR_SOLVE_SLOTS=1 - in a fresh child process, since the switch is read once per process.

Pendulum, N = 20, B = 64 (more than four problems: the inputs go through device copies; a few seconds in all); one case at N = 200,
B = 8, where the time-parallel rollout and the Riccati scan run.  No test asserts a speed or that two kernels overlapped: that is
profiles/c2_solve_overlap_ab.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def _child(tmp, tag, slots, mode, *names):
    """Cases in a fresh child process with MI_ILQR_SOLVE_SLOTS set to `slots`, or unset (None: the default)."""
    out = str(tmp / (tag + ".npz"))
    env = {k: v for k, v in os.environ.items() if k != "MI_ILQR_SOLVE_SLOTS"}
    if slots is not None:
        env["MI_ILQR_SOLVE_SLOTS"] = slots
    r = subprocess.run([sys.executable, os.path.join(HERE, "_solve_slots_child.py"), out, mode, *names], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """The blocking, single-slot run of every case: one child process for the module."""
    return _child(tmp_path_factory.mktemp("solve_slots"), "reference", "1", "blocking")


def _compare(name, reference, skip=()):
    import solve_slots_cases as cases
    got = cases.run_all(pipelined=True, names=[name])
    keys = [k for k in reference if k.startswith(name + "/")]
    assert keys and set(keys) <= set(got)
    for k in keys:
        if k.split("/", 1)[1] in skip:
            continue
        assert got[k].shape == reference[k].shape and got[k].dtype == reference[k].dtype, k
        assert np.array_equal(got[k], reference[k], equal_nan=True), k
    return got


def test_sequences_differ_between_the_input_sets(reference):
    """The yardstick itself: the two input sets give different solves, so a solve that read the wrong copy would show."""
    c, it = reference["alternating/ring_cost"], reference["alternating/ring_iters"]
    assert np.array_equal(c[0], c[2]) and np.array_equal(c[1], c[3]) and not np.array_equal(c[0], c[1])
    assert not np.array_equal(it[0], it[1])


def test_alternating_inputs(reference):
    _compare("alternating", reference)


def test_alternating_inputs_time_parallel_horizon(reference):
    _compare("alternating_long", reference)


def test_repeated_inputs(reference):
    _compare("repeated", reference)


def test_partial_inputs(reference):
    _compare("partial_inputs", reference)


def test_warm_solve_continues_from_the_last_cold_one(reference):
    _compare("warm", reference)


def test_other_consumers_read_the_last_solve(reference):
    _compare("consumers", reference)


def test_returned_stream_is_ordered_behind_every_solve(reference):
    got = _compare("stream_order", reference)
    assert np.array_equal(got["stream_order/stream_cost"], reference["alternating/ring_cost"][3])


def test_handle_with_a_result_sink(reference):
    _compare("sink", reference)


def test_tiny_batch(reference):
    _compare("tiny", reference)


def test_control_limited_handle(reference):
    _compare("limited", reference)


def test_second_slot_is_lazy(tmp_path):
    """A handle that only ever solves blocking takes the device memory it takes with one slot; pipelined cold solves add the second.
    Device memory in use before and after create plus blocking solves (hipMemGetInfo), in two fresh processes that differ in the
    switch alone - what the runtime keeps of earlier handles would otherwise show in the difference."""
    one = _child(tmp_path, "one", "1", "blocking", "lazy")
    two = _child(tmp_path, "two", None, "pipelined", "lazy")
    print("bytes, one slot:", one["lazy/blocking_bytes"], " default:", two["lazy/blocking_bytes"], two["lazy/pipelined_bytes"])
    assert np.array_equal(one["lazy/blocking_bytes"], two["lazy/blocking_bytes"])
    assert two["lazy/pipelined_bytes"][0] > two["lazy/blocking_bytes"][0]
