"""-m gpu: the exact-inference passes (embed_full / predict_full, embed_nodes / predict_nodes, rank_full, topk_full) against outputs
recorded while the HOST code of an earlier commit drove the same library (tests/golden/infer_parent_outputs.npz,
tests/golden/make_infer_parent_outputs.py: every aggregator stated its full-neighborhood layer twice then, as infer_full and as
infer_rows, and rank_full / topk_full each carried their own query prelude).  Each aggregator has ONE recipe now, run by a
whole-graph scope and a row-subset scope, so the tests that hold the two passes to each other and to the float64 oracles at 1e-4
would pass a slip in the shared recipe -- another operand, row count or leading dimension that still gives nearly the same
numbers; it fails here.  Every float output compares equal AS A FLOAT VALUE to the recorded one -- no tolerance; outputs above
8 KB are compared through the SHA-256 of their bytes with -0 folded to +0; integer outputs compare with array_equal.

Shapes (tests/infer_cases.py): N = 300, F = 20, a hub cut in three partials, an isolated node; the whole-graph pass also in 19
windows of 16 rows (the last of 13)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_infer_parent_outputs", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_infer_parent_outputs.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
CASES = rec.case_names()


@pytest.fixture(scope="module")
def golden():
    return rec.load()


def test_golden_file_covers_every_case(golden):
    assert {k.split(".", 1)[0] for k in golden} == set(CASES) and len(CASES) == 10 + 1
    assert os.path.getsize(rec.GOLDEN_FILE) <= 113 * 1024
    per_case = {c: {k.split(".", 1)[1].rsplit(".", 1)[0] for k in golden if k.split(".", 1)[0] == c} for c in CASES}
    for c in CASES:
        want = set() if c == rec.BILINEAR else {"full"} | set(rec.REQUESTS)
        want |= {"win16"} if c in rec.WINDOWED else set()
        want |= {"padded"} if c in rec.PADDED else set()
        want |= {"rank_filt", "rank_raw", "topk_filt", "topk_raw"} if c in rec.RANKED else set()
        assert per_case[c] == want, c


@pytest.mark.parametrize("name", CASES)
def test_inference_equals_the_recorded_outputs(dev, golden, name):
    got = rec.run(name)
    assert {"%s.%s" % (name, k) for k in got} == {k for k in golden if k.split(".", 1)[0] == name}
    for key, a in got.items():
        a = np.ascontiguousarray(a)
        want = golden["%s.%s" % (name, key)]
        if rec.is_int(a):
            assert want[0] == "whole" and np.array_equal(a, want[1]), "%s.%s differs from the recorded ids / counts" % (name, key)
            continue
        assert a.dtype == np.float32 and np.isfinite(a[a != -np.inf]).all(), "%s.%s is not finite" % (name, key)
        if want[0] == "whole":
            assert a.shape == want[1].shape
            diff = int((a != want[1]).sum())
            assert diff == 0, "%s.%s: %d of %d values differ from the recorded ones (max |diff| %g)" % (
                name, key, diff, a.size, float(np.abs(a.astype(np.float64)[a != want[1]] - want[1][a != want[1]]).max()))
        else:
            assert a.nbytes > rec.WHOLE_BYTES
            assert np.array_equal(rec.digest(a), want[1]), "%s.%s: the SHA-256 of its values differs from the recorded one" % (name, key)
