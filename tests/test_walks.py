"""Host side of the second-order (p, q) random walks (no GPU): the C ABI of gs_walk_paths / gs_walk_pairs, the thresholds, the
NumPy restatement held to the walk law itself, the walk flags of the unsupervised driver."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import walk_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAW_WALKS, LAW_SEED, LAW_PQ = 1 << 18, 123, (0.5, 2.0)


def test_descriptor_size_and_symbols():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    source = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_walk.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(gs_walk_desc\) == (\d+)", source)
    assert asserted and ctypes.sizeof(_lib.WalkDesc) == int(asserted.group(1)) == 152
    assert re.search(r"typedef struct gs_walk_desc \{", header)
    assert re.search(r"#define GS_WALK_TAG 0x%Xull" % _lib.WALK_TAG, header) and int(wo.TAG) == _lib.WALK_TAG
    assert re.search(r"#define GS_WALK_ATTEMPTS %d\b" % _lib.WALK_ATTEMPTS, header) and wo.ATTEMPTS == _lib.WALK_ATTEMPTS == 256
    lib = _lib.load()
    for name in ("gs_walk_paths", "gs_walk_pairs"):
        assert re.search(r"\bint %s\s*\(const gs_walk_desc\*" % name, header)
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_the_walk_tag_is_a_domain_of_its_own():
    from graphsage_amd import _lib
    in_use = [h << 56 for h in range(64)] + [0xFF << 56, 0xD0 << 56, 0x7AB1E5EED, 0xC0115]      # hop ids and the other tags
    assert _lib.WALK_TAG not in in_use


def test_abi_version_and_struct_count_are_unchanged():
    from graphsage_amd import _lib
    lib = _lib.load()
    assert lib.gs_abi_version() == _lib.GS_ABI_VERSION == 12
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == 8


def test_thresholds():
    from graphsage_amd import ops
    assert sorted(ops.walk_thresholds(0.5, 2)) == [1 << 30, 1 << 31, 1 << 32]
    assert ops.walk_thresholds(0.5, 2) == (1 << 32, 1 << 31, 1 << 30)          # (return, common, far)
    assert ops.walk_thresholds(1, 1) == (1 << 32,) * 3
    assert ops.walk_thresholds(4, 0.25) == (1 << 28, 1 << 30, 1 << 32)         # min / max = 1/16 exactly: still allowed
    assert ops.walk_thresholds(4, 4) == (1 << 30, 1 << 32, 1 << 30)
    assert ops.walk_thresholds(3, 0.7) == tuple(int(Fraction(w) / (1 / Fraction(0.7)) * (1 << 32))
                                                 for w in (1 / Fraction(3.0), 1, 1 / Fraction(0.7)))
    for p, q in ((0.5, 2), (1, 1), (4, 0.25), (4, 4), (3, 0.7), (0.3, 1.9)):
        thr = ops.walk_thresholds(p, q)
        assert thr == wo.thresholds(p, q) and max(thr) == 1 << 32 and min(thr) >= 1 << 28
    for p, q in ((0.25, 8), (8, 0.25), (0.05, 1), (1, 17), (0, 1), (1, -2), (float("nan"), 1), (float("inf"), 1)):
        with pytest.raises(ValueError):
            ops.walk_thresholds(p, q)
    with pytest.raises(ValueError, match="1/16"):
        ops.walk_thresholds(0.25, 8)


def test_entry_points_refuse_before_they_launch():
    from graphsage_amd import _lib
    lib = _lib.load()
    for name in ("gs_walk_paths", "gs_walk_pairs"):
        assert getattr(lib, name)(None, None) == -1 and name.encode() in lib.gs_last_error()
    d = _lib.WalkDesc()                      # every pointer null
    d.n_nodes, d.nnz, d.n_starts, d.num_walks, d.walk_len, d.ld_paths, d.n_walks = 6, 12, 3, 2, 5, 5, 6
    d.thr_return, d.thr_common, d.thr_far = 1 << 32, 1 << 31, 1 << 30
    assert lib.gs_walk_paths(ctypes.addressof(d), None) == -1 and b"non-null" in lib.gs_last_error()
    for thr in ((1 << 32, 1 << 32, (1 << 28) - 1), (1 << 31, 1 << 31, 1 << 31), ((1 << 32) + 1, 1 << 32, 1 << 32), (1 << 32, 0, 1 << 32)):
        d.thr_return, d.thr_common, d.thr_far = thr
        assert lib.gs_walk_paths(ctypes.addressof(d), None) == -1 and b"1/16" in lib.gs_last_error()
    d.thr_return, d.thr_common, d.thr_far = 1 << 32, 1 << 31, 1 << 30
    d.n_walks = 7                            # more walks than 3 starts x 2
    assert lib.gs_walk_paths(ctypes.addressof(d), None) == -1 and b"outside the job" in lib.gs_last_error()
    d.n_walks, d.walk0 = 6, 1
    assert lib.gs_walk_paths(ctypes.addressof(d), None) == -1 and b"outside the job" in lib.gs_last_error()
    d.walk0 = 0
    for bad_len in (0, -1, 4097):
        d.walk_len = bad_len
        assert lib.gs_walk_paths(ctypes.addressof(d), None) == -1 and b"walk_len" in lib.gs_last_error()
        assert lib.gs_walk_pairs(ctypes.addressof(d), None) == -1 and b"walk_len" in lib.gs_last_error()
    d.walk_len, d.ld_paths = 5, 4
    assert lib.gs_walk_paths(ctypes.addressof(d), None) == -1 and b"ld_paths" in lib.gs_last_error()
    d.ld_paths = 5
    assert lib.gs_walk_pairs(ctypes.addressof(d), None) == -1 and b"non-null" in lib.gs_last_error()
    d.n_walks = 0                            # nothing to do: returns at once
    assert lib.gs_walk_paths(ctypes.addressof(d), None) == 0 and lib.gs_walk_pairs(ctypes.addressof(d), None) == 0


def test_transition_probs_of_the_hand_graph():
    rowptr, col = wo.hand_graph()
    F = Fraction
    assert wo.transition_probs(rowptr, col, 0, 1, 0.5, 2) == {0: F(1, 2), 2: F(1, 4), 3: F(1, 8), 5: F(1, 8)}
    assert wo.transition_probs(rowptr, col, 0, 2, 0.5, 2) == {0: F(2, 3), 1: F(1, 3)}
    assert wo.transition_probs(rowptr, col, None, 0, 0.5, 2) == {1: F(1, 2), 2: F(1, 2)}
    assert wo.transition_probs(rowptr, col, 3, 4, 4, 0.25) == {3: F(1)}
    rp2, col2 = wo.csr_from_rows([[1, 1, 2], [0, 0], [0]])                     # an edge stored twice is taken twice as often
    assert wo.transition_probs(rp2, col2, None, 0, 1, 1) == {1: F(2, 3), 2: F(1, 3)}


@pytest.fixture(scope="module")
def law_run():
    rowptr, col = wo.hand_graph()
    stats = {}
    paths, counts = wo.walk_paths(rowptr, col, [0], LAW_WALKS, 3, wo.thresholds(*LAW_PQ), LAW_SEED, stats=stats)
    return rowptr, col, paths, counts, stats


def check_law(rowptr, col, paths, p, q):
    """Walks of length 3 from node 0 of the hand graph: every outcome of the second step, given the first, within 5 binomial
    standard deviations of (0.5, 0.25, 0.125, 0.125) over (0, 2, 3, 5) after 1 and of (2/3, 1/3) over (0, 1) after 2; the
    first step within 5 of (1/2, 1/2)."""
    devs = wo.law_deviations(rowptr, col, paths, p, q)
    want = {"0 -> 1": 0.5, "0 -> 2": 0.5,
            "0 -> 1 -> 0": 0.5, "0 -> 1 -> 2": 0.25, "0 -> 1 -> 3": 0.125, "0 -> 1 -> 5": 0.125,
            "0 -> 2 -> 0": 2.0 / 3.0, "0 -> 2 -> 1": 1.0 / 3.0}
    assert {d[0]: d[1] for d in devs} == pytest.approx(want, abs=1e-15)
    for desc, pr, cnt, n, dev in devs:
        print("%-12s P = %.6f: %d of %d, %.2f sd" % (desc, pr, cnt, n, dev))
    for desc, pr, cnt, n, dev in devs:
        assert dev <= 5.0, (desc, pr, cnt, n, dev)


def test_the_oracle_obeys_the_law(law_run):
    rowptr, col, paths, counts, stats = law_run
    assert paths.shape == (LAW_WALKS, 3)
    check_law(rowptr, col, paths, *LAW_PQ)


def test_no_step_of_the_law_run_reaches_the_attempt_cap(law_run):
    stats = law_run[4]
    assert stats["capped"] == 0
    # 2^18 first steps take one draw each; a second step takes 1 / mean acceptance draws on average: between 1 and 16
    assert LAW_WALKS * 2 <= stats["attempts"] <= LAW_WALKS * 17


def test_oracle_counts_pairs_and_chunks():
    rowptr, col = wo.hand_graph()
    thr = wo.thresholds(4, 0.25)
    starts = [0, 4, -1, 6, 3, 3]
    paths, counts = wo.walk_paths(rowptr, col, starts, 7, 6, thr, 5)
    assert paths.shape == (42, 6) and np.all(paths[14:28] == -1) and np.all(counts[14:28] == 0)
    assert np.array_equal(counts, ((paths[:, 1:] != paths[:, :1]) & (paths[:, :1] >= 0)).sum(axis=1))
    pairs = wo.walk_pairs(paths, counts)
    assert pairs.shape == (counts.sum(), 2) and np.all(pairs[:, 0] != pairs[:, 1]) and pairs.min() >= 0
    parts = [wo.walk_paths(rowptr, col, starts, 7, 6, thr, 5, walk0=w0, n_walks=min(16, 42 - w0)) for w0 in range(0, 42, 16)]
    assert np.array_equal(np.concatenate([a for a, _ in parts]), paths)
    assert np.array_equal(np.concatenate([c for _, c in parts]), counts)
    # every step follows a stored edge
    keys = set(zip(np.repeat(np.arange(6), np.diff(rowptr)).tolist(), col.tolist()))
    for row in paths[paths[:, 0] >= 0]:
        assert all((int(a), int(b)) in keys for a, b in zip(row[:-1], row[1:]))
    # a node without entries keeps the walk where it is; an entry that is no node is walked to and never from
    rp, c = wo.csr_from_rows([[1], [], [3], [2, 4]])                           # 4 = n_nodes: the pad id
    paths, counts = wo.walk_paths(rp, c, [0, 1, 2], 8, 5, thr, 9)
    assert np.all(paths[:8] == [0, 1, 1, 1, 1]) and np.all(paths[8:16] == 1) and np.all(counts[8:16] == 0)
    stuck = paths[16:]
    assert np.all(stuck[:, 1] == 3) and np.any(stuck == 4)
    for row in stuck:
        k = np.nonzero(row == 4)[0]
        assert k.size == 0 or np.all(row[k[0]:] == 4)


def test_driver_flags_and_refusals():
    from graphsage_amd import unsupervised_train as ut
    f = ut.build_flags([])
    assert (f.walk_p, f.walk_q, f.walk_len, f.num_walks, f.device_walks) == (1.0, 1.0, 5, 50, False)
    assert not ut.use_device_walks(f)
    ut.refuse_walk_flags(f)
    assert ut.use_device_walks(ut.build_flags(["--device_walks"]))
    assert ut.use_device_walks(ut.build_flags(["--device_walks", "true"]))
    assert not ut.use_device_walks(ut.build_flags(["--device_walks", "false"]))
    assert ut.use_device_walks(ut.build_flags(["--walk_q", "2"])) and ut.use_device_walks(ut.build_flags(["--walk_p", "0.5"]))
    f = ut.build_flags(["--walk_p", "0.5", "--walk_q", "2", "--walk_len", "7", "--num_walks", "3"])
    assert (f.walk_p, f.walk_q, f.walk_len, f.num_walks) == (0.5, 2.0, 7, 3)
    ut.refuse_walk_flags(f)
    for argv in (["--walk_p", "0.25", "--walk_q", "8"], ["--walk_q", "0.01"], ["--walk_p", "-1"], ["--walk_p", "0"]):
        with pytest.raises(SystemExit, match="1/16|positive"):
            ut.refuse_walk_flags(ut.build_flags(argv))
    for argv in (["--walk_len", "0"], ["--num_walks", "0", "--device_walks"]):
        with pytest.raises(SystemExit, match="at least 1"):
            ut.refuse_walk_flags(ut.build_flags(argv))
    old = ut.FLAGS
    try:                                     # refused before any data is loaded or anything is trained
        with pytest.raises(SystemExit, match="min\\(1/p, 1, 1/q\\)"):
            ut.main(["--synthetic", "small", "--model", "n2v", "--walk_p", "0.25", "--walk_q", "8"])
    finally:
        ut.FLAGS = old
