"""The world and the ten models of the exact-inference tests (tests/test_embed_nodes_gpu.py, tests/test_infer_golden_gpu.py) and
of the recorder tests/golden/make_infer_parent_outputs.py, which must not import a test file.

The graph: 300 nodes + the pad row, sparse (mean degree about 3), one hub of 2 L + 77 edges (a cut row: three partials), one
isolated node (from_csr points it at the pad node); built with FullGraph.from_csr, and as a padded table (every row re-sampled
to width 6, no cut row) with FullGraph.from_padded."""
import numpy as np

from graphsage_amd import engine as eng
from graphsage_amd import inits
from graphsage_amd.inference import SPLIT_LEN, FullGraph

N, F, C, L = 300, 20, 5, SPLIT_LEN
HUB, ISOLATED = 40, 77
_cache = {}


def world():
    """rowptr / col of the true graph, its padded twin, features (pad row zero), and both FullGraphs with their lists."""
    if "w" in _cache:
        return _cache["w"]
    rng = np.random.RandomState(2)
    degs = rng.poisson(3.0, size=N)
    degs[HUB], degs[ISOLATED] = 2 * L + 77, 0
    lists = [rng.randint(0, N, size=d) for d in degs]
    lists[HUB] = rng.randint(100, 120, size=degs[HUB])          # the hub lists 20 ids over and over: its field stays small
    for v in range(N):                                          # nobody but node 41 lists the hub or the isolated node
        lists[v][np.isin(lists[v], [HUB, ISOLATED])] = (v + 1) % 30
    lists[41] = np.asarray([HUB, 41, 7])                        # ... with a self-loop
    degs = np.asarray([len(x) for x in lists])
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    col = np.concatenate(lists).astype(np.int32)
    adj = np.full((N + 1, 6), N, np.int64)
    for v in range(N):
        if degs[v]:
            adj[v] = lists[v][rng.randint(0, degs[v], size=6)]
    feats = np.concatenate([rng.randn(N, F).astype(np.float32), np.zeros((1, F), np.float32)])
    g_csr = FullGraph.from_csr(rowptr, col, N)
    g_pad = FullGraph.from_padded(adj)
    assert g_csr.splits.shape[0] == 1 and g_csr.splits[0, 0] == HUB and g_csr.splits[0, 2] == 3 and g_pad.splits.shape[0] == 0
    assert np.array_equal(g_csr.lists()[ISOLATED], [N])
    _cache["w"] = dict(adj=adj, feats=feats, deg=degs, graphs={"csr": (g_csr, g_csr.lists()), "padded": (g_pad, g_pad.lists())})
    return _cache["w"]


MODELS = {
    # name: (aggregator, dim, layers, identity_dim, supervised, sigmoid); concat everywhere but gcn, as the reference runs them
    "mean_narrow": ("mean", 8, 2, 0, True, False),              # dim < F: the reduce runs over H . W_neigh
    "mean_plain": ("mean", 24, 2, 0, True, True),               # dim >= F at layer 0: the plain form; sigmoid head
    "gcn_narrow": ("gcn", 8, 2, 0, True, False),
    "gcn_plain": ("gcn", 24, 2, 0, True, False),
    "maxpool": ("maxpool", 8, 2, 0, True, False),
    "meanpool": ("meanpool", 8, 2, 0, True, True),
    "twomaxpool": ("twomaxpool", 8, 2, 0, True, False),
    "mean_3layer": ("mean", 8, 3, 0, True, False),
    "mean_identity": ("mean", 8, 2, 4, True, False),
    "unsup_mean": ("mean", 8, 2, 0, False, False),
}


# not one of the ten: the link-prediction head with bilinear weights takes embeddings of 64, 128, 256 or 512 columns (rank_full and
# topk_full with the Xq . A product; tests/golden/make_infer_parent_outputs.py)
BILINEAR = {"unsup_bilinear": ("mean", 32, 2, 0, False, False)}


def many_request():
    """17 unsorted ids, one of them twice."""
    many = np.random.RandomState(9).permutation(N)[:16].tolist()
    many.insert(5, many[11])
    assert len(many) == 17 and len(set(many)) == 16 and many != sorted(many)
    return many


def build(name):
    """(model, oracle params in float64, feature table as the device holds it): random weights in EVERY variable, the Dense biases
    included, so that the pad row's hidden state is not zero."""
    from graphsage_amd.models import Placeholder, SAGEInfo, SampleAndAggregate
    from graphsage_amd.neigh_samplers import AdjInfo, PaddedAdjacency, UniformNeighborSampler
    from graphsage_amd.supervised_models import SupervisedGraphsage
    agg, dim, K, idim, sup, sigmoid = MODELS.get(name) or BILINEAR[name]
    model_kw = dict(bilinear_weights=True) if name in BILINEAR else {}
    w = world()
    eng.reset_engine()
    inits.set_seed(1)
    e = eng.get_engine()
    ph = {'labels': Placeholder('labels'), 'batch': Placeholder('batch1'), 'batch1': Placeholder('batch1'),
          'batch2': Placeholder('batch2'), 'neg_samples': Placeholder('neg'), 'dropout': Placeholder('dropout', 0.),
          'batch_size': Placeholder('batch_size')}
    adj_info = AdjInfo(PaddedAdjacency(w["adj"], e.device))
    sampler = UniformNeighborSampler(adj_info)
    layer_infos = [SAGEInfo("node", sampler, 3, dim) for _ in range(K)]
    if sup:
        model = SupervisedGraphsage(C, ph, w["feats"], adj_info, w["deg"], layer_infos, concat=(agg != "gcn"),
                                    aggregator_type=agg, sigmoid_loss=sigmoid, identity_dim=idim, **model_kw)
    else:
        model = SampleAndAggregate(ph, w["feats"], adj_info, w["deg"], layer_infos, concat=(agg != "gcn"), aggregator_type=agg,
                                   identity_dim=idim, **model_kw)
    rng = np.random.RandomState(len(name))

    def fill(v, scale):
        a = (rng.randn(*v.numpy().shape) * scale).astype(np.float32)
        v.assign(a)
        return a.astype(np.float64)

    params = {"agg": []}
    for a in model.aggregators:
        p = {k: fill(v, 0.3) for k, v in sorted(a.vars.items())}
        mlp = [(fill(l.vars['weights'], 0.2), fill(l.vars['bias'], 0.2).reshape(-1)) for l in getattr(a, "mlp_layers", [])]
        if len(mlp) == 1:
            p["mlp_weights"], p["mlp_bias"] = mlp[0]                # fullnbr_oracle's names for the one-Dense aggregators
        elif mlp:
            p["mlp"] = mlp
        if "bias" in p:
            p["bias"] = p["bias"].reshape(-1)
        params["agg"].append(p)
    if sup:
        params["node_pred"] = {"weights": fill(model.node_pred.vars['weights'], 0.5),
                               "bias": fill(model.node_pred.vars['bias'], 0.5).reshape(-1)}
    if model.embeds is not None:
        fill(model.embeds, 0.5)
        model._refresh_embeds()
    e.sync()
    feats = model.features.numpy().astype(np.float64)
    assert feats.shape == (N + 1, F + idim) and len(model.aggregators) == K
    return model, params, feats
