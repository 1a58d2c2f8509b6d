"""-m gpu: the five 128 x 128 fp32-MFMA score sweeps (gs_rank_count, gs_topk_select, gs_ivf_search, gs_kmeans_assign,
gs_linkpred_infonce_fwd_bwd) against outputs recorded with the library of an earlier commit (tests/golden/sweep_parent_outputs.npz,
tests/golden/make_sweep_parent_outputs.py: the kernels that each carried their own copy of the K loop).  They share one tile
pipeline now (csrc/gs_rank_dev.h).  The kernels' own suites use small-integer inputs, exact under any order of additions, and so
cannot see a changed k order; the inputs here are real-valued.  Every output must compare equal to the recorded one -- no
tolerance (float values by `==`: -0 equals +0); outputs above 8 KB are compared through the SHA-256 of their bytes with -0 folded
to +0."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_sweep_parent_outputs", os.path.join(_golden, "make_sweep_parent_outputs.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    return rec.load()


def test_golden_file_covers_every_case(golden):
    assert {k.split(".", 1)[0] for k in golden} == set(rec.CASES) and len(set(rec.CASES)) == 5 + 5 + 5 + 5 + 4
    assert os.path.getsize(rec.GOLDEN_FILE) <= os.path.getsize(os.path.join(_golden, "tail_parent_outputs.npz"))


@pytest.mark.parametrize("name", rec.CASES)
def test_sweep_equals_the_recorded_outputs(dev, golden, name):
    got = rec.run(name, dev)
    assert {"%s.%s" % (name, k) for k in got} == {k for k in golden if k.split(".", 1)[0] == name}
    for key, a in got.items():
        a = np.ascontiguousarray(a)
        want = golden["%s.%s" % (name, key)]
        assert not np.isnan(a).any(), "%s.%s holds a NaN" % (name, key)
        if want[0] == "whole":
            assert a.shape == want[1].shape and a.dtype == want[1].dtype
            diff = int((a != want[1]).sum())
            assert diff == 0, "%s.%s: %d of %d values differ from the recorded ones (first at %s)" % (
                name, key, diff, a.size, np.argwhere(a != want[1])[0].tolist())
        else:
            assert a.nbytes > rec.WHOLE_BYTES
            assert np.array_equal(rec.digest(a), want[1]), "%s.%s: the SHA-256 of its values differs from the recorded one" % (name, key)
