"""The step's enqueue sequence, pinned (tests/_trace.py).

The numeric tests cannot see a reordered capture: hipGraph keeps the first-captured dependant of a node on that node's stream, so a step
that enqueues the same launches in another order gives the same numbers and replays slower.  Every configuration of
tests/golden/step_traces.json — the switch combinations of the schedule tests at the three stages, folded and unfolded, the arm, the
building-block path, frozen maps, disabled terms, the data-parallel path on one rank, the perceptual term — must enqueue exactly the
recorded C-ABI calls (name, stream, every argument), stream waits, event records and clears, in the recorded order.  A change that moves
a launch on purpose regenerates the file (tests/golden/make_step_traces.py)."""
import json

import pytest

from tests import _trace

CONFIGS = _trace.configurations()


def test_golden_file_holds_every_configuration():
    with open(_trace.GOLDEN) as f:
        gold = json.load(f)
    assert set(gold["configs"]) == set(CONFIGS), sorted(set(gold["configs"]) ^ set(CONFIGS))
    assert set(gold["configs"].values()) == set(gold["traces"])


@pytest.fixture(scope="module")
def gold():
    with open(_trace.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    return {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_step_enqueues_the_recorded_sequence(gold, cases, name):
    spec = CONFIGS[name]
    if spec["kind"] not in cases:
        cases[spec["kind"]] = _trace.fit_case(spec["kind"])
    got = _trace.trace_configuration(cases[spec["kind"]]["eng"], spec)
    ref = gold["traces"][gold["configs"][name]]
    diff = _trace.first_difference(got, ref)
    if diff:
        print(f"{name}: {diff}")
    assert diff is None, f"{name}: {diff}"
