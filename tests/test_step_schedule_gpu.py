"""-m gpu: the step schedule, pinned as a trace.  Every scenario of tests/golden/make_step_traces.py (host-fed train / eval step,
three device steps, train_steps_device(7, 4) = graphs of 4 and 2 steps and a single step, an epoch reset, train_steps_device(4, 4);
supervised and unsupervised models, the aggregators, dropout, pipeline off, identity features, the split tail, sampler placement, a
change of batch size, eager and capturable gradient hooks, Node2Vec) is run again under the recorder and its sequence of library
entry points, graph launches, hook calls and gather-share splits must equal tests/golden/step_schedule_traces.json, recorded
before the supervised and unsupervised step machinery were merged into one schedule (SampleAndAggregate, section "the step
schedule (both models)" of models.py).
`use_graphs` stays at its default, so the eager pass, the capture pass and the replays of every graph key are all in the trace."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_step_traces", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_step_traces.py"))
traces = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(traces)


@pytest.fixture(scope="module")
def golden():
    with open(traces.TRACE_FILE) as f:
        return traces.unpack(json.load(f))


def test_every_scenario_is_recorded(golden):
    assert sorted(golden) == sorted(traces.SCENARIOS)


def test_run_length_coding_round_trips():
    seq = [0, 1, 2, 1, 2, 1, 2, 3, 3, 3, 3, 0, 1, 2, 1, 2, 1, 2, 3, 3, 3, 3, 4]
    assert traces.decode(traces.encode(seq)) == seq


@pytest.mark.parametrize("name", sorted(traces.SCENARIOS))
def test_schedule_trace(dev, golden, name):
    got, losses, params = traces.record(name)
    want = golden[name]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, "trace of %s differs at event %d of %d / %d: got %r, recorded %r" % (
        name, first, len(got), len(want), got[max(0, first - 3): first + 3], want[max(0, first - 3): first + 3])
    assert all(x == x and abs(x) < 1e30 for x in losses), losses
