"""The attention-pooling aggregator (graphsage_attn) without a GPU: the oracle of tests/attn_oracle.py is right (its hand-written
backward equals central finite differences in float64 and torch.autograd on a CPU restatement, every parameter and both inputs),
and the new entry points, op constant, class and model name are in place with GS_ABI_VERSION and every struct as they were."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attn_oracle as ao
from oracle import graphsage_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_segment_attn_fwd", "gs_segment_attn_bwd", "gs_attn_scores")
STRUCT_SIZES = [80, 88, 40, 288, 344, 48, 312, 216]      # tests/test_l1_means_abi.py: the descriptors at ABI 12
KEYS = ("self_weights", "neigh_weights", "mlp_weights", "mlp_bias", "attn_a", "bias")


def layer_case(s, concat, act, seed=0, n=4, d=5, hid=8, o=3):
    rng = np.random.RandomState(seed)
    p = ao.make_params([d, o], concat, rng, hidden=hid, bias=True)[0]
    p["attn_a"] = rng.randn(hid)                        # a wide spread of scores: the softmax is far from uniform
    return p, rng.randn(n, d), rng.randn(n, s, d), rng.randn(n, (2 if concat else 1) * o)


def loss_of(p, self_vecs, neigh, concat, act, R):
    with ao.installed():
        y, _ = orc._agg_fwd("attn", p, self_vecs, neigh, concat, act)
    return float((y * R).sum())


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("act", ["relu", "id"])
def test_oracle_backward_equals_central_differences(s, concat, act):
    p, self_vecs, neigh, R = layer_case(s, concat, act)
    with ao.installed():
        y, cache = orc._agg_fwd("attn", p, self_vecs, neigh, concat, act)
        d_self, d_neigh, g = orc._agg_bwd("attn", p, R, cache, concat, act)
    assert y.dtype == np.float64 and set(g) == set(KEYS)
    eps = 1e-6
    wants = dict(g, self_in=d_self, neigh_in=d_neigh)
    arrays = dict(p, self_in=self_vecs, neigh_in=neigh)
    rng = np.random.RandomState(1)
    for k, want in wants.items():
        a = arrays[k]
        flat = a.reshape(-1)
        for idx in rng.choice(flat.size, size=min(flat.size, 12), replace=False):
            keep = flat[idx]
            flat[idx] = keep + eps
            up = loss_of(p, self_vecs, neigh, concat, act, R)
            flat[idx] = keep - eps
            dn = loss_of(p, self_vecs, neigh, concat, act, R)
            flat[idx] = keep
            fd = (up - dn) / (2 * eps)
            assert abs(fd - want.reshape(-1)[idx]) <= 1e-6 * max(1.0, abs(fd)), (k, idx, fd, want.reshape(-1)[idx])


def torch_layer(p, self_vecs, neigh, concat, act):
    n, s, d = neigh.shape
    V = torch.relu(neigh.reshape(n * s, d) @ p["mlp_weights"] + p["mlp_bias"]).reshape(n, s, -1)
    alpha = torch.softmax(V @ p["attn_a"], dim=1)
    pooled = (alpha[:, :, None] * V).sum(dim=1)
    fs, fn = self_vecs @ p["self_weights"], pooled @ p["neigh_weights"]
    z = (torch.cat([fs, fn], dim=1) if concat else fs + fn) + p["bias"]
    return torch.relu(z) if act == "relu" else z


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("concat", [True, False])
def test_oracle_backward_equals_autograd(s, concat):
    act = "relu"
    p, self_vecs, neigh, R = layer_case(s, concat, act, seed=2)
    with ao.installed():
        y, cache = orc._agg_fwd("attn", p, self_vecs, neigh, concat, act)
        d_self, d_neigh, g = orc._agg_bwd("attn", p, R, cache, concat, act)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    ts = torch.tensor(self_vecs, requires_grad=True)
    tn = torch.tensor(neigh, requires_grad=True)
    ty = torch_layer(tp, ts, tn, concat, act)
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-12, atol=1e-12)
    (ty * torch.tensor(R)).sum().backward()
    for k in KEYS:
        np.testing.assert_allclose(g[k], tp[k].grad.numpy(), rtol=1e-10, atol=1e-12, err_msg=k)
    np.testing.assert_allclose(d_self, ts.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(d_neigh, tn.grad.numpy(), rtol=1e-10, atol=1e-12)
    if s == 1:
        assert np.array_equal(cache[3], np.ones((neigh.shape[0], 1))) and np.all(g["attn_a"] == 0)      # alpha == 1, dt == 0


def test_oracle_follows_the_input_dtype_and_the_whole_list_form_agrees():
    """A node whose whole neighbor list IS its sample gets the sampled layer's value; float32 in, float32 out."""
    p, self_vecs, neigh, _ = layer_case(3, True, "relu", seed=3)
    p.pop("bias")
    n, s, d = neigh.shape
    H = np.concatenate([self_vecs, neigh.reshape(n * s, d)])
    lists = [n + i * s + np.arange(s) for i in range(n)] + [np.zeros(0, np.int64)] * (n * s)
    full = ao.full_layer(lists, H, p, True, last=False)
    with ao.installed():
        y, _ = orc._agg_fwd("attn", p, self_vecs, neigh, True, "relu")
    np.testing.assert_allclose(full[:n], y, rtol=1e-12, atol=1e-12)
    dup = ao.softmax_reduce_rows([np.asarray([1, 1, 2])], H, H[:, 0])            # a duplicate entry counts twice
    w = np.exp(H[[1, 1, 2], 0] - H[[1, 2], 0].max())
    np.testing.assert_allclose(dup[0], (w[:, None] * H[[1, 1, 2]]).sum(axis=0) / w.sum(), rtol=1e-12)
    p32 = {k: v.astype(np.float32) for k, v in p.items()}
    with ao.installed():
        y32, _ = orc._agg_fwd("attn", p32, self_vecs.astype(np.float32), neigh.astype(np.float32), True, "relu")
    assert y32.dtype == np.float32


def test_new_entry_points_are_declared_bound_and_exported():
    from graphsage_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r"#define GS_CSR_SOFTMAX 3\b", header) and _lib.CSR_SOFTMAX == 3
    assert (_lib.CSR_MEAN, _lib.CSR_MEAN_SELF, _lib.CSR_MAX) == (0, 1, 2)
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name) is not None
    for fn in ("segment_attn_fwd", "segment_attn_bwd", "attn_scores", "segment_attn_supported"):
        assert callable(getattr(ops, fn))
    assert ops.segment_attn_supported(128, 1024) and ops.segment_attn_supported(1, 4)
    assert not ops.segment_attn_supported(129, 512) and not ops.segment_attn_supported(0, 512)
    assert not ops.segment_attn_supported(10, 1028) and not ops.segment_attn_supported(10, 510)


def test_abi_version_and_struct_layouts_did_not_move():
    from graphsage_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphsage_amd.h")).read()
    assert _lib.GS_ABI_VERSION == 12 and re.search(r"#define GS_ABI_VERSION 12\b", header)
    lib = _lib.load()
    assert lib.gs_abi_version() == 12
    sizes = (ctypes.c_int32 * 16)()
    assert lib.gs_abi_struct_sizes(sizes, 16) == len(STRUCT_SIZES)
    assert list(sizes)[:len(STRUCT_SIZES)] == STRUCT_SIZES
    assert ctypes.sizeof(_lib.CsrReduceDesc) == 200 and ctypes.sizeof(_lib.CsrRowsDesc) == 168


def test_out_of_range_shapes_are_refused_on_the_host_before_any_launch():
    """GS_ENOTSUP (-3) is decided from s and hidden alone, before a pointer is looked at."""
    from graphsage_amd import _lib
    lib = _lib.load()
    for s, hidden in ((0, 512), (129, 512), (10, 1028), (10, 510), (10, 0)):
        assert lib.gs_segment_attn_fwd(None, 0, None, None, 1, s, hidden, None, 0, None, None) == -3, (s, hidden)
        assert lib.gs_segment_attn_bwd(None, 0, None, 0, None, None, None, 1, s, hidden, None, 0, None, 1, None) == -3, (s, hidden)
        assert lib.gs_last_error()
    assert lib.gs_attn_scores(None, 0, 1, 1028, None, None) == -3


def test_model_name_resolves_and_the_drivers_accept_it():
    from graphsage_amd import models, supervised_train, unsupervised_train
    from graphsage_amd._lib import GraphsageAmdError
    from graphsage_amd.aggregators import AttentionPoolingAggregator, _PoolBase
    cls = models._aggregator_cls("attn")
    assert cls is AttentionPoolingAggregator and issubclass(cls, _PoolBase)
    assert cls._WIDTHS == {"small": (512,), "big": (1024,)}
    for mod in (supervised_train, unsupervised_train):
        flags = mod.build_flags(["--model", "graphsage_attn", "--synthetic", "small", "--samples_1", "128", "--samples_2", "1"])
        assert flags.model == "graphsage_attn" and flags.model.split('_')[1] == "attn"
        supervised_train.refuse_samples(flags)                           # inside the kernels' range
        flags.samples_1 = 129
        with pytest.raises(GraphsageAmdError, match="1 <= samples <= 128"):
            supervised_train.refuse_samples(flags)
        flags.model = "graphsage_maxpool"
        supervised_train.refuse_samples(flags)                           # only the attention model has the limit
