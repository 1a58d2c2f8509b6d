"""-m gpu: whole training steps with Engine.fused_l1_means on and off (the tiled layer-0 forward writes the layer-1 neighbor means
and the fused tail loads them | the tail forms them itself): two models from the same seed, 17 device-epoch steps through 8-step
hipGraphs (1 priming step + 8 + 8), parameters / loss / predictions bit-equal after the last step -- and the `on` model really
went through the new entry points (MeanAggregator.last_fwd_entry, model.last_tail_entry).
Supervised: B = 256, fan-out 5 x 10 = 2,816 layer-0 rows, above the 2,048-row threshold of the tiled forward.  Unsupervised: B = 64
with 20 negatives is 148 roots = 1,628 rows, UNDER that threshold (both models take the plain entries there; checked, with the
bits); B = 128 (276 roots, 3,036 rows) is the size at which the new entries run.  (Unsupervised
steps take the fusion only with Engine.fused_l1_means_unsup -- it measured slower there -- so the test sets it.)"""
import numpy as np
import pytest

from graphsage_amd import engine as eng
from graphsage_amd import inits
from graphsage_amd.minibatch import EdgeMinibatchIterator, NodeMinibatchIterator
from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
from graphsage_amd.neigh_samplers import AdjInfo, CSRAdjacency, UniformNeighborSampler
from graphsage_amd.supervised_models import SupervisedGraphsage
from graphsage_amd.utils import synthetic_graph

pytestmark = pytest.mark.gpu

NS = [5, 10]          # layer-0 gather fan-out 5, hop-1 fan-out s = 10
DIM = 128
STEPS = 17


def _sup_model(fused):
    eng.reset_engine()
    inits.set_seed(7)
    G = synthetic_graph(n_nodes=3000, feat_dim=50, num_classes=7, avg_degree=6, seed=5, multilabel=False)
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    it = NodeMinibatchIterator(G, None, ph, None, G.num_classes, batch_size=256, max_degree=10)
    e = eng.get_engine()
    e.fused_l1_means = fused
    adj_info = AdjInfo(CSRAdjacency(it.train_csr[0], it.train_csr[1], G.n_nodes, e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, NS[i], DIM) for i in range(2)]
    model = SupervisedGraphsage(G.num_classes, ph, G.padded_features(), adj_info, it.deg, layer_infos, concat=True,
                                aggregator_type="mean", sigmoid_loss=False, learning_rate=0.01, weight_decay=0.0)
    return it, model


def _unsup_model(fused):
    eng.reset_engine()
    inits.set_seed(11)
    np.random.seed(7)            # EdgeMinibatchIterator permutes edges with the global NumPy RNG
    G = synthetic_graph(n_nodes=3000, feat_dim=50, num_classes=5, avg_degree=6, seed=5)
    ph = {'batch1': Placeholder('batch1'), 'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'),
          'dropout': Placeholder('dropout', 0.), 'batch_size': Placeholder('batch_size')}
    it = EdgeMinibatchIterator(G, None, ph, context_pairs=None, batch_size=64, max_degree=10)
    e = eng.get_engine()
    e.fused_l1_means = fused
    e.fused_l1_means_unsup = True         # (opt-in for unsupervised steps: Engine.fused_l1_means_unsup)
    adj_info = AdjInfo(CSRAdjacency(it.train_csr[0], it.train_csr[1], G.n_nodes, e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, NS[i], DIM) for i in range(2)]
    model = SampleAndAggregate(ph, G.padded_features(), adj_info, it.deg, layer_infos, concat=True, aggregator_type="mean",
                               learning_rate=0.01, weight_decay=0.0, neg_sample_size=20)
    return it, model


def test_supervised_steps_bit_equal(dev):
    B = 256
    res = []
    for fused in (True, False):
        it, model = _sup_model(fused)
        model.attach_device_epoch(it.train_nodes, it.label_matrix)
        model.train_steps_device(B, STEPS, steps_per_launch=8)
        e = eng.get_engine()
        e.sync()
        assert model._tail_used
        agg0 = model.aggregators[0]
        assert agg0.last_fwd_entry == ("gs_sage_dense_fwd_tiled3_means" if fused else "gs_sage_dense_fwd_tiled3")
        assert model.last_tail_entry == ("gs_sage_tail_fwd_bwd_means" if fused else "gs_sage_tail_fwd_bwd")
        assert ops_error(model) == 0
        res.append((e.params.cpu().numpy().copy(), model.loss_dev.cpu().numpy().copy(), model.preds.numpy().copy()))
    (p1, l1, y1), (p0, l0, y0) = res
    assert np.isfinite(l1).all() and np.array_equal(l1, l0)
    assert np.array_equal(y1, y0) and np.abs(y1).max() > 0
    assert np.array_equal(p1, p0)


def ops_error(model):
    from graphsage_amd import ops
    return ops.tail_sync_error(model._tail_sync, model._tail_sync_n)


@pytest.mark.parametrize("B,taken", [(64, False), (128, True)])
def test_unsupervised_steps_bit_equal(dev, B, taken):
    from graphsage_amd import ops
    res = []
    for fused in (True, False):
        it, model = _unsup_model(fused)
        model.attach_device_pairs(it.train_edges)
        model.train_steps_device(B, STEPS, steps_per_launch=8)
        e = eng.get_engine()
        e.sync()
        assert model._lp_tail_used
        on = fused and taken
        agg0 = model.aggregators[0]
        if taken:
            assert agg0.last_fwd_entry == ("gs_sage_dense_fwd_tiled3_means" if on else "gs_sage_dense_fwd_tiled3")
        else:
            assert agg0.last_fwd_entry != "gs_sage_dense_fwd_tiled3_means"
        assert model.last_tail_entry == ("gs_linkpred_tail_means" if on else "gs_linkpred_tail")
        assert ops.lp_tail_sync_error(model._lp_sync, *model._lp_sync_shape) == 0
        res.append((e.params.cpu().numpy().copy(), model.loss_dev.cpu().numpy().copy(), model.outputs_all.numpy().copy(),
                    model.aff_all.numpy().copy()))
    for a, b in zip(*res):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert np.abs(res[0][2]).max() > 0
