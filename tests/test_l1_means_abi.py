"""The four entry points of the fused layer-1 means (gs_sage_dense_fwd_tiled3_means and the three *_means tail launches) are ADDED:
declared in the header, bound by _lib, exported by the built library -- with GS_ABI_VERSION and every descriptor struct as they were."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_sage_dense_fwd_tiled3_means", "gs_sage_tail_fwd_bwd_means", "gs_sage_tail_z_means", "gs_linkpred_tail_means")
# sizeof() of gs_gather_desc, gs_wgrad_desc, gs_var_desc, gs_fanout_desc, gs_tail_desc, gs_dropout, gs_pull_desc, gs_lp_tail_desc at ABI 12
STRUCT_SIZES = [80, 88, 40, 288, 344, 48, 312, 216]


def test_new_entry_points_are_declared_bound_and_exported():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
    # same argument lists as the entries they extend (+ n_roots, s, l1_means, ld_means in front of the stream)
    assert _lib._PROTOS["gs_sage_dense_fwd_tiled3_means"][:-5] == _lib._PROTOS["gs_sage_dense_fwd_tiled3"][:-1]
    assert len(_lib._PROTOS["gs_sage_dense_fwd_tiled3_means"]) == len(_lib._PROTOS["gs_sage_dense_fwd_tiled3"]) + 4
    for new, old in (("gs_sage_tail_fwd_bwd_means", "gs_sage_tail_fwd_bwd"), ("gs_sage_tail_z_means", "gs_sage_tail_z"),
                     ("gs_linkpred_tail_means", "gs_linkpred_tail")):
        assert _lib._PROTOS[new] == _lib._PROTOS[old]
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name) is not None


def test_abi_version_and_struct_layouts_did_not_move():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    assert _lib.GS_ABI_VERSION == 12 and re.search(r"#define GS_ABI_VERSION 12\b", header)
    lib = _lib.load()
    assert lib.gs_abi_version() == 12
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == len(STRUCT_SIZES)
    assert list(sizes)[:len(STRUCT_SIZES)] == STRUCT_SIZES
    mirrors = [_lib.GatherDesc, _lib.WgradDesc, _lib.VarDesc, _lib.FanoutDesc, _lib.TailDesc, _lib.Dropout, _lib.PullDesc,
               _lib.LpTailDesc]
    assert [ctypes.sizeof(m) for m in mirrors] == STRUCT_SIZES


def test_null_descriptors_are_refused_not_dereferenced():
    from graphsage_amd import _lib
    lib = _lib.load()
    for name in NEW[1:]:
        assert getattr(lib, name)(None, None, 0, None) == -1 and lib.gs_last_error()
