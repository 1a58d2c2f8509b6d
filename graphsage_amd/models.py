"""SampleAndAggregate: the sample -> gather -> aggregate schedule of graphsage/models.py:187-330 on
the gfx950 engine, keeping the reference's method names and argument meaning:

    samples, support_sizes = model.sample(inputs, layer_infos, batch_size)
    out, aggregators       = model.aggregate(samples, [features], dims, num_samples, support_sizes,
                                             batch_size, aggregators, name, concat, model_size)

TF built a static graph once and ran it with sess.run; here the same Python runs eagerly on the
engine's HIP stream, is captured into a hipGraph on its second execution for a given batch size,
and replayed afterwards.  `aggregate_backward` is the hand-written reverse schedule (TF:
optimizer.compute_gradients, models.py:379).
"""
import os
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .aggregators import (AttentionPoolingAggregator, GCNAggregator, MaxPoolingAggregator, MeanAggregator, MeanPoolingAggregator,
                          SeqAggregator, TwoMaxLayerPoolingAggregator, contiguous_rows)
from .engine import get_engine
from .inits import glorot
from .layers import Rows, identity
from .ops import Mat
from .utils import unigram_cdf

# SAGEInfo is a namedtuple that specifies the parameters of the recursive GraphSAGE layers
# (graphsage/models.py:180-185)
SAGEInfo = namedtuple("SAGEInfo",
                      ['layer_name',     # name of the layer (to get feature embedding etc.)
                       'neigh_sampler',  # callable neigh_sampler constructor
                       'num_samples',
                       'output_dim'])    # the output (i.e., hidden) dimension

_AGGREGATORS = {
    "mean": MeanAggregator,
    "maxpool": MaxPoolingAggregator,
    "meanpool": MeanPoolingAggregator,
    "gcn": GCNAggregator,
    "seq": SeqAggregator,
    "twomaxpool": TwoMaxLayerPoolingAggregator,
    "attn": AttentionPoolingAggregator,
}


def _aggregator_cls(aggregator_type):
    """Dispatch of models.py:211-222 / supervised_models.py:34-45."""
    if aggregator_type not in _AGGREGATORS:
        raise Exception("Unknown aggregator: ", aggregator_type)
    return _AGGREGATORS[aggregator_type]


class Placeholder(object):
    """Host-side feed slot standing in for tf.placeholder (supervised_train.py:112-120)."""

    def __init__(self, name, default=None):
        self.name = name
        self.value = default

    def __repr__(self):
        return "<Placeholder %s>" % self.name


def device_features(features, engine=None):
    """Upload the [N+1, F] feature table (row N = zero pad row, supervised_train.py:133-135) with a
    leading dimension of whole 128-byte lines (F=602 -> ld=608)."""
    e = engine or get_engine()
    if isinstance(features, Mat):
        return features
    return Mat.from_numpy(np.asarray(features, dtype=np.float32), e.device, ld_multiple=32)


def _run_captured(graphs, warm, key, fn, stream, may_capture):
    """fn() eagerly on the first use of `key`, captured into a hipGraph (kept in `graphs`) and launched on the second, the
    graph replayed afterwards.  may_capture() is asked only when a capture is about to start; while it says no, fn() stays
    eager.  True when this call captured the graph."""
    g = graphs.get(key)
    if g is not None:
        g.launch()
        return False
    if key not in warm or not may_capture():
        fn()
        warm.add(key)
        return False
    g = ops.Graph(stream)
    g.begin()
    try:
        fn()
    except Exception:
        try:                      # leave the stream out of capture mode, or every later launch on it fails too
            g.end()
        except Exception:
            pass
        raise
    g.end()
    graphs[key] = g
    g.launch()
    return True


class SampleAndAggregate(object):
    """Base implementation of unsupervised GraphSAGE (graphsage/models.py:187-405): three sample+aggregate passes
    (batch1, batch2, 20 degree^0.75 negatives) sharing the aggregators, l2-normalise, skip-gram cross-entropy
    (prediction.py:102-110), loss/batch_size, clip +-5, Adam, MRR.  Here the three passes are ONE pass over the
    concatenated roots [batch1 | batch2 | negatives] (rows are independent and the aggregators are shared, so it is
    the same computation).  `FLAGS.learning_rate / weight_decay / neg_sample_size` are explicit keyword arguments.

        loss, ranks, aff_all, mrr, outputs1 = model.train_step(feed_dict)   # unsupervised_train.py:273-274
        loss, ranks, mrr = model.eval_step(feed_dict)                        # :69-71
    The supervised subclass is in supervised_models.py."""

    def __init__(self, placeholders, features, adj, degrees, layer_infos, concat=True, aggregator_type="mean",
                 model_size="small", identity_dim=0, learning_rate=0.00001, weight_decay=0.0, neg_sample_size=20,
                 world_size=1, rank=0, _defer_build=False, loss_fn='xent', bilinear_weights=False, pred_bias=False,
                 loss_temperature=0.1, **kwargs):
        allowed_kwargs = {'name', 'logging', 'model_size'}
        for kwarg in kwargs.keys():
            assert kwarg in allowed_kwargs, 'Invalid keyword argument: ' + kwarg
        self.name = kwargs.get('name') or self.__class__.__name__.lower()
        self.engine = get_engine()
        # arguments of the link-prediction layer (prediction.py:12-15; the reference hard-codes the defaults, models.py:363-366)
        self.loss_fn, self.bilinear_weights, self.pred_bias = loss_fn, bool(bilinear_weights), bool(pred_bias)
        self.loss_temperature = float(loss_temperature)       # loss_fn='infonce' only (not in the reference)
        self.aggregator_cls = _aggregator_cls(aggregator_type)
        self.aggregator_type = aggregator_type
        self.model_size = model_size
        self.adj_info = adj
        self.identity_dim = int(identity_dim)
        if aggregator_type == "seq" and self.identity_dim > 0:
            # the LSTM's input gradients would have to reach the trainable table columns through every step: not built
            raise ops._lib.GraphsageAmdError("identity_dim > 0 is not supported with the LSTM aggregator (graphsage_seq)")
        self._init_features(features, adj, self.identity_dim)
        self.degrees = degrees
        self.concat = concat
        self.dims = [self.features.d]        # == (0 if features is None else F) + identity_dim  (:244)
        self.dims.extend([layer_infos[i].output_dim for i in range(len(layer_infos))])
        self.placeholders = placeholders
        self.batch_size = placeholders.get("batch_size") if placeholders else None
        self.layer_infos = layer_infos
        self.aggregators = None
        self._tape = None
        self.learning_rate = float(learning_rate)
        self.weight_decay = float(weight_decay)
        self.neg_sample_size = int(neg_sample_size)
        self.world_size, self.rank = int(world_size), int(rank)
        self.engine.dropout_seed = 123 + 1000003 * self.rank      # every data-parallel rank draws its own masks
        self.row_offset = 0
        # shares of the prefetch gather carried by the step's launches (sweeps in DESIGN.md).  Two-launch form (layer-0
        # forward | weight gradients): 0.7 | 0.3 with the LDS-tiled kernels, 0.5 | 0.5 with the stream kernels.
        # Three-launch form of the supervised mean model (layer-0 forward | fused tail | weight gradients): 0.25 | 0.40 |
        # 0.35 since round 6 -- the four-wave tiled forward and weight-gradient workgroups leave room for two rider workgroups on
        # their own CUs (profiles/r06_tiled3_wgrad_ab.txt: headline 97.7 us/step; 0.15 | 0.5 | 0.35 with the stream kernels, where
        # the tail -- 32 busy CUs -- was the best host).
        # Round 6, two main workgroups per group in the fused tail (training launches over 256 input columns, gs_tail.hip): the
        # tail's own chain is 19 us instead of 26, and what it hosts for free is a fixed AMOUNT of gather (~64 MB: 64 + 128 idle
        # CUs for 19 / 11 us), not a fixed share -- rider_shares() sets (forward | tail | weight gradients) from the step's gather
        # bytes: 0.40 | 0.20 | 0.40 for the Reddit step (321 MB: 98.3 -> 94.0 us/step), 0.125 | 0.75 | 0.125 for RMAT
        # (79 MB: 67.4 -> 59.9); profiles/r06_tail_halves_ab.txt.  GS_COGATHER_TAIL / GS_COGATHER_SPLIT3 pin fixed shares.
        # OPT-IN (GS_SAMPLER_IN_WGRAD=1): the sampler of the step after the next rides in the weight-gradient launch instead of
        # the optimizer launch (supervised fused-tail models on the tiled kernels; one root per WAVE of a rider workgroup; the tail
        # launch makes the private id copy the weight gradients then read).  The optimizer launch waits 8 us for the sampler's
        # chain against 5.5 us of its own; same-call A/B: Reddit 95.0 -> 92.0 us/step, GCN 96.1 -> 95.8, RMAT 59.4 -> 57.8.  Every
        # test passes with it (bit-identical ids, steps and parameters against the optimizer-launch form) -- and in graphs of
        # >= 8 steps ONE training run in ~10^5 steps differs from the others (benchmarks/determinism.sh: 2 of 220 200-step runs;
        # benchmarks/race_hunt.py: a z-helper workgroup of the tail read a stale 128-byte line of h0; never in 1.9 M steps with the
        # sampler in the optimizer launch, never in 2-step or 4-step graphs): until that is understood the default stays off
        # (profiles/r06_determinism.txt).
        self.sampler_in_wgrad = os.environ.get("GS_SAMPLER_IN_WGRAD", "0") == "1"
        self.sampler_in_wgrad_max_bytes = 1e15
        self._wgrad_sampler_seen = None
        self.tail_halves = os.environ.get("GS_TAIL_HALVES", "1") != "0"
        self.cogather_auto = ("GS_COGATHER_TAIL" not in os.environ and "GS_COGATHER_SPLIT3" not in os.environ)
        self.tail_free_bytes = float(os.environ.get("GS_TAIL_FREE_MB", 64)) * 1e6     # (sweeps: profiles/r06_tail_halves_ab.txt, fused_l1_means_ab.txt)
        self.cogather_split = float(os.environ.get("GS_COGATHER_SPLIT", 0.5 if self.engine.stream_gemm else 0.7))
        tiled = self.engine.stream_gemm and self.engine.tiled3_fwd and self.engine.tiled3_wgrad
        self.cogather_split3 = float(os.environ.get("GS_COGATHER_SPLIT3", 0.25 if tiled else 0.15))
        self.cogather_tail = float(os.environ.get("GS_COGATHER_TAIL", (0.40 if tiled else 0.5) if self.engine.stream_gemm else 0.0))
        # unsupervised three-launch form (forward | fused link-prediction tail | weight gradients)
        self.cogather_lp_fwd = float(os.environ.get("GS_COGATHER_LP_FWD", 0.20))      # 0.30 with the stream forward (round 5); the tiled forward holds a CU per workgroup: 176.2 vs 179.5 us/step
        self.cogather_lp_tail = float(os.environ.get("GS_COGATHER_LP_TAIL", 0.25))
        self.cogather_lp_neg = float(os.environ.get("GS_COGATHER_LP_NEG", 0.10))
        self.cogather_z = 0.04            # measured: 0 | 0.04 | 0.08 | 0.12 -> 201.5 | 199.1 | 202.9 | 209.4 us
        # DIAGNOSTIC (one test pins it bit-identical): the fused tail as two launches (z helpers | row-group workgroups) --
        # no dependency between workgroups of a launch, the safe form under tools that serialise workgroups; +11 us per step
        self.tail_split = os.environ.get("GS_TAIL_SPLIT", "0") == "1"
        self.cogather_tail_z = 0.35           # part of the tail's gather share the z launch carries in that form
        # (Removed in round 4 after losing their measurements -- sources and numbers in benchmarks/variants/README.md: a gather
        #  share in the optimizer launch, one in the last layer's backward launch, a forked gather branch beside the in-graph
        #  all-reduce, the second-stream pipeline, the weight-stationary form of the layer-0 forward.)
        # inside a multi-step graph the sampler of step t+2 rides in step t's optimizer launch (see _pipelined_steps)
        self.sampler_rides = True         # (diagnostic: False = every sampler launch stands alone; one test)
        # the fused tail launches (supervised: gs_sage_tail_fwd_bwd; unsupervised: gs_linkpred_tail); 0 = per-operator schedule
        self.fuse_tail = os.environ.get("GS_FUSE_TAIL", "1") != "0"
        self._graphs, self._graph_outputs, self._warm = {}, {}, set()
        self.use_graphs = True
        self.grad_hook = None
        if self.identity_dim == 0:
            # next-step gather co-scheduled inside this step's launches (one stream); False = sequential schedule
            self.pipeline = os.environ.get("GS_PIPELINE", "1") != "0"
        self._primed = None
        self._prefetched = {}
        self._pending_stage = None
        if not _defer_build:
            self.inputs1 = placeholders["batch1"]
            self.inputs2 = placeholders["batch2"]
            self.build()

    # ------------------------------------------------------------------------------ identity features (:229-240)
    def _init_features(self, features, adj, identity_dim):
        """self.features = concat([node_embeddings, features], axis=1) (models.py:229-240).  The trainable
        `node_embeddings` [N+1, identity_dim] (tf.get_variable default initializer = glorot_uniform) lives in the flat
        parameter buffer; the concatenation is kept materialised as ONE table so that a sampled id still costs one
        row fetch, and its leading columns are refreshed after every optimizer step (Engine.post_update_hooks)."""
        e = self.engine
        self.embeds = None
        if identity_dim > 0:
            n_rows = adj.n_nodes + 1                                   # adj.get_shape()[0]
            self.embeds = e.add_variable("node_embeddings", glorot((n_rows, identity_dim)), decay=False, scatter=True)
        if features is None:
            if identity_dim == 0:
                raise Exception("Must have a positive value for identity feature dimension if no input features given.")
            self.features = Mat.zeros(n_rows, identity_dim, e.device, ld_multiple=32)
        elif self.embeds is None:
            self.features = device_features(features, e)
        else:
            fixed = np.asarray(features.numpy() if isinstance(features, Mat) else features, dtype=np.float32)
            if fixed.shape[0] != n_rows:
                raise ops._lib.GraphsageAmdError("features must have N+1 = %d rows (got %d)" % (n_rows, fixed.shape[0]))
            self.features = Mat.zeros(n_rows, identity_dim + fixed.shape[1], e.device, ld_multiple=32)
            self.features.buf[:, identity_dim: identity_dim + fixed.shape[1]].copy_(torch.from_numpy(fixed))
            torch.cuda.synchronize()
        if self.embeds is not None:
            e.post_update_hooks.append(self._refresh_embeds)
            # the table's leading columns are rewritten behind every optimizer launch: no cut-once copies of it (Engine.table16_of)
            e.mutable_tables.add(self.features.buf.data_ptr())
            # the prefetch pipeline gathers step t+1's rows before step t's update: not valid for a trainable table
            self.pipeline = False

    def _refresh_embeds(self):
        ops.copy_cols(self.embeds.value, self.features, self.embeds.rows, self.identity_dim, stream=self.engine.stream)

    def _embed_sink(self):
        return (self.embeds, self.identity_dim) if self.embeds is not None else None

    # ------------------------------------------------------------------------------ unsupervised build (:332-391)
    def build(self):
        e = self.engine
        self.num_samples = [layer_info.num_samples for layer_info in self.layer_infos]
        self.aggregators = self.make_aggregators(self.dims, self.num_samples, self.concat, self.model_size)
        from .prediction import BipartiteEdgePredLayer
        dim_mult = 2 if self.concat else 1
        self.link_pred_layer = BipartiteEdgePredLayer(dim_mult * self.dims[-1], dim_mult * self.dims[-1], self.placeholders,
                                                      act="sigmoid", loss_fn=self.loss_fn, bias=self.pred_bias,
                                                      bilinear_weights=self.bilinear_weights,
                                                      temperature=self.loss_temperature, name='edge_predict')
        e.finalize()
        if self.embeds is not None:
            self._refresh_embeds()
        self.loss_dev = torch.zeros(1, dtype=torch.float32, device=e.device)
        self.mrr_dev = torch.zeros(1, dtype=torch.float32, device=e.device)
        # fixed unigram distribution ~ degree^0.75 of tf.nn.fixed_unigram_candidate_sampler (:336-343); uniform if no node
        # has a neighbor
        deg = np.asarray(self.degrees, dtype=np.float64)
        self._guide_bits = 18
        cdf, guide = unigram_cdf(deg if np.power(deg, 0.75).sum() > 0 else np.ones_like(deg), self._guide_bits)
        self._neg_cdf = torch.from_numpy(cdf.view(np.int32).copy()).to(e.device)   # raw bits; the kernel reads uint32
        self._n_cdf = int(cdf.shape[0])
        self._neg_guide = torch.from_numpy(guide).to(e.device)
        self.neg_seed = 123
        torch.cuda.synchronize()

    _OUT_ATTRS = ("samples1", "outputs_all", "outputs1", "agg_out", "_loss_rows", "_rr_rows", "aff_all", "_d_agg_out",
                  "_loss_accumulate", "_tape", "_lp_tail_used", "_tail_h0", "_tail_means", "_tail_dh0", "_lp_sync",
                  "_lp_sync_shape", "_epilogue_folded")

    def rider_shares(self, jobs, tail_d_in):
        """(forward share, tail share) of the next step's gather for the three-launch form (the weight gradients carry the
        rest).  Fixed shares unless the fused tail runs two main workgroups per group (tail_d_in == 256); then the tail takes
        what it hosts for free (tail_free_bytes) and the two contraction launches halve the rest."""
        tiled = self.engine.stream_gemm and self.engine.tiled3_fwd and self.engine.tiled3_wgrad
        if not (self.cogather_auto and self.tail_halves and tiled and tail_d_in == 256 and not self.tail_split):
            return self.cogather_split3, self.cogather_tail
        total = float(sum(j.n * j.s * j.d * 4 for j in jobs))
        f_tail = min(0.75, max(0.10, self.tail_free_bytes / max(total, 1.0)))
        return 0.5 * (1.0 - f_tail), f_tail

    def _roots(self, B, parity=None):
        """[batch1 (B) | batch2 (B) | negatives] = the head of the contiguous id buffer."""
        n_roots = 2 * B + self.neg_sample_size
        return self.ids_buffer(n_roots, parity=parity)[0][:n_roots], n_roots

    def _stage_negatives(self, roots, B, pairs=None, cursor=None):
        e = self.engine
        ops.call("gs_unsup_stage", ops.ptr(pairs), pairs.shape[0] if pairs is not None else 0, ops.ptr(cursor), B,
                 ops.ptr(self._neg_cdf), self._n_cdf, self.neg_sample_size, self.neg_seed, ops.ptr(e.sample_clock_dev),
                 int(getattr(self, "row_offset", 0)), ops.ptr(roots), e.stream)

    def inject_negatives(self, neg):
        """Parity tests: the negatives of the next host-fed step (the reference draws them from TF's candidate sampler,
        models.py:336-343; like the sampler's permutations they are injected so both sides see the same ids)."""
        self._injected_neg = None if neg is None else np.ascontiguousarray(neg, dtype=np.int32)
        self.use_graphs = False if neg is not None else self.use_graphs

    def _stage_negatives_or_injected(self, roots, B):
        neg = getattr(self, "_injected_neg", None)
        if neg is None:
            return self._stage_negatives(roots, B)
        assert neg.shape[0] == self.neg_sample_size
        self._injected_neg = None
        self.engine.sync()
        roots[2 * B: 2 * B + self.neg_sample_size].copy_(torch.from_numpy(neg))
        torch.cuda.current_stream().synchronize()

    def _forward_layers(self, roots, n, prefetched, tail_ok, means_ok, side_jobs, z_jobs=None):
        """The head of either model's forward pass: the data phase (unless prefetched) and the aggregator layers over the n
        roots -- layer 0 alone when the model's fused tail launch takes the rest.  Returns (output of the layers run, tail used?).
        tail_ok(): does the fused tail apply to this step?  It also needs the hops of layer 0 in ONE contiguous buffer
        (model.sample on the model's id buffer); anything else takes the per-operator schedule.  means_ok: let the tiled
        layer-0 launch write the tail's layer-1 neighbor means (Engine.fused_l1_means)."""
        e = self.engine
        self.reset_tapes()
        if prefetched is None:
            prefetched = self._data_phase(roots, n, getattr(self, "_parity", 0), stage=getattr(self, "_pending_stage", None))
        samples1, support_sizes1, means0 = prefetched
        contiguous = all(b.data_ptr() == a.data_ptr() + 4 * a.numel() for a, b in zip(samples1[:-1], samples1[1:]))
        tail_used = bool(contiguous and tail_ok())
        agg0 = self.aggregators[0]
        agg0.l1_means_out = None
        if tail_used and e.fused_l1_means and means_ok:
            # `tail_means` exists before the layer-0 launch: where that is the tiled concat form it writes the layer-1 neighbor
            # means from its finished tiles (agg0.l1_means_written) and the tail's helpers load them
            agg0.l1_means_out = e.ws_mat("tail_means", n, 2 * self.dims[1])
        out, _ = self.aggregate(samples1, [self.features], self.dims, self.num_samples, support_sizes1, batch_size=n,
                                aggregators=self.aggregators, concat=self.concat, model_size=self.model_size,
                                layer0_means=means0, layer0_side_jobs=side_jobs, last_layer_side_jobs=z_jobs,
                                _stop_after_layer=0 if tail_used else None)
        self.samples1 = samples1
        if tail_used and self._tape[0][0] != "batched":
            raise ops._lib.GraphsageAmdError("fused tail needs the contiguous id buffer (model.sample on ids_buffer)")
        return out, tail_used

    def _forward_unsup(self, roots, B, n_roots, train, prefetched=None, side_jobs=None, epilogue=None, z_jobs=None, tail_jobs=None):
        """_build (:347-370) + _loss (:385-391) + _accuracy (:393-405) and, when training, the gradient of the
        link-prediction head w.r.t. the normalised embeddings."""
        e = self.engine
        out, self._lp_tail_used = self._forward_layers(
            roots, n_roots, prefetched, lambda: self._lp_tail_ok() and n_roots == 2 * B + self.neg_sample_size,
            e.fused_l1_means_unsup, side_jobs, z_jobs)
        self._loss_rows = e.ws_f32("loss_rows", B)
        self._rr_rows = e.ws_f32("rr_rows", B)
        self.aff_all = e.ws_mat("aff_all", B, self.neg_sample_size + 1)
        if self._lp_tail_used:
            tj, nj = tail_jobs, None
            if tail_jobs and self.cogather_lp_neg > 0 and self.cogather_lp_tail > 0:
                # the second launch (nine workgroups) carries its own share of the gather
                tj, nj = ops.split_gather_jobs(tail_jobs, self.cogather_lp_tail / (self.cogather_lp_tail + self.cogather_lp_neg))
            self._forward_lp_tail(B, n_roots, train, epilogue, tj, nj)
        else:
            self.agg_out = out
            d = out.d
            self.outputs_all = e.ws_mat("outputs_all", n_roots, d)
            self.outputs1 = self.outputs_all.rows_slice(0, B)
            # l2_normalize (:368-370) + link-prediction loss / MRR ranks (:385-405) + their gradient carried back through the
            # normalisation: ONE launch (+ a 20-workgroup one for the negatives' rows); d_agg_out = dLoss/d(aggregator output)
            self._d_agg_out = e.ws_mat("d_agg_out", n_roots, d)
            # `epilogue` (the step's device-counter increments): without dropout the loss / mrr means and the counters ride in
            # the head's second launch (with dropout the clock must not move before the backward pass: separate launch later)
            fold = epilogue is not None and self._dropout_rate() == 0.0
            self._epilogue_folded = fold
            epi = (self.loss_dev, False, self.mrr_dev, self._epilogue_counters(epilogue)) if fold else None
            if self.loss_fn == 'infonce':
                # the in-batch softmax masks its false negatives by the pairs' node ids (the head of the id buffer, on the
                # device already for the sampler); validation takes its forward-only form
                self.link_pred_layer.loss_and_grads_fused(out, self.outputs_all, B, self.neg_sample_size, 1.0 / B,
                                                          self._loss_rows, self._rr_rows, self.aff_all,
                                                          self._d_agg_out if train else None, epilogue=epi,
                                                          ids=(roots[:B], roots[B:2 * B]))
            else:
                self.link_pred_layer.loss_and_grads_fused(out, self.outputs_all, B, self.neg_sample_size, 1.0 / B,
                                                          self._loss_rows, self._rr_rows, self.aff_all, self._d_agg_out,
                                                          epilogue=epi)
        # loss = (sum_vars wd*l2_loss + xent) / batch_size  (:386-390, :378); the xent mean (and the mrr, :404) are formed
        # by the epilogue (folded: the weight-decay terms are added behind it; separate launch: it adds to them)
        self._weight_decay_loss([v for a in self.aggregators for v in a.vars.values()], 0.5 * self.weight_decay / B,
                                self._epilogue_folded)

    def _epilogue_counters(self, epilogue):
        """The step epilogue's [(device counter, increment)] * 3: optimizer step, sampler clock, pair cursor."""
        e = self.engine
        return [(e.step_dev, epilogue.get("step", 0)), (e.sample_clock_dev, epilogue.get("clock", 0)),
                (epilogue.get("cursor"), epilogue.get("cursor_delta", 0))]

    def _weight_decay_loss(self, variables, scale, fold=False):
        """loss_dev (+)= scale * sum_variables sum(v^2): the weight-decay terms of the loss (unsupervised: the aggregators'
        variables, / batch_size, :386-388, :378; supervised: every decayed variable, supervised_models.py:104-108).  fold: the
        epilogue has written the head's mean already and the terms are added behind it; otherwise they start the sum and the
        later epilogue adds to them (_loss_accumulate)."""
        first = not fold
        if self.weight_decay != 0.0:
            for v in variables:
                ops.call("gs_sumsq_scaled", v.value.ptr, v.size, scale, self.loss_dev.data_ptr(), 0 if first else 1,
                         self.engine.stream)
                first = False
        self._loss_accumulate = not first and not fold

    def _lp_tail_ok(self):
        """The fused layer-1 + link-prediction launches (gs_linkpred_tail / gs_linkpred_tail_neg) apply to the two-layer mean
        model with concat, no aggregator bias, no dropout, no trainable identity features, at shapes the kernel supports."""
        if not getattr(self, "fuse_tail", True) or len(self.layer_infos) != 2 or self.aggregator_type != "mean":
            return False
        if self.loss_fn != 'xent' or self.bilinear_weights:
            return False          # gs_unsup_tail.hip is the xent head; the other losses take the per-operator schedule
        a1 = self.aggregators[1]
        return (self.concat and not a1.bias and self._dropout_rate() == 0 and self.embeds is None
                and self.num_samples[-1] <= 11
                and ops.linkpred_tail_supported(2 * self.dims[1], self.dims[2], self.neg_sample_size))

    def _forward_lp_tail(self, B, n_roots, train, epilogue, tail_jobs, neg_jobs=None):
        """Layer 1 + l2_normalize + link-prediction loss / MRR (+ every input gradient down to layer 0's pre-activations when
        training) as the two launches of gs_unsup_tail.hip; gather jobs of the next step ride in the first one."""
        e = self.engine
        h0 = self._tape[0][4]                       # [n + n*s, 2*dim_1]: layer-0 outputs of both hops
        a1 = self.aggregators[1]
        O = self.dims[2]
        Z = 2 * O
        s = self.num_samples[len(self.num_samples) - 1]
        nn = self.neg_sample_size
        self._tail_h0 = h0
        self._tail_means = e.ws_mat("tail_means", n_roots, h0.d)
        self.agg_out = e.ws_mat("tail_z", n_roots, Z)
        self.outputs_all = e.ws_mat("outputs_all", n_roots, Z)
        self.outputs1 = self.outputs_all.rows_slice(0, B)
        self._d_agg_out = e.ws_mat("d_agg_out", n_roots, Z)
        self._tail_dh0 = e.ws_mat((self.name, "d_hidden", 0), h0.rows, h0.d)
        slabs = e.ws_f32(("lp_neg_slabs", B, nn, Z), ((B + 7) // 8) * nn * Z)
        self._lp_sync = e.ws_i32(("lp_tail_sync", self.name, B, nn), ops.lp_tail_sync_words(B, nn))
        self._lp_sync_shape = (B, nn)
        desc = ops.linkpred_tail_desc(h0, B, nn, s, a1.vars['self_weights'].value, a1.vars['neigh_weights'].value, O,
                                      self._tail_means, self.agg_out, self.outputs_all, self._loss_rows, self._rr_rows,
                                      self.aff_all, self.link_pred_layer.neg_sample_weights, 1.0 / B, self._lp_sync,
                                      dz=self._d_agg_out if train else None, d_h0=self._tail_dh0 if train else None,
                                      neg_slabs=slabs if train else None)
        means_ready = bool(getattr(self.aggregators[0], "l1_means_written", False))
        self.last_tail_entry = "gs_linkpred_tail_means" if means_ready else "gs_linkpred_tail"
        ops.linkpred_tail(desc, jobs=tail_jobs, stream=e.stream, means_ready=means_ready)
        # launch 2 always follows (it commits the hand-over state); the step epilogue rides in it unless dropout needs the
        # clock untouched until the backward pass has run (this path runs without dropout: always folded when given)
        fold = epilogue is not None
        self._epilogue_folded = fold
        counters = self._epilogue_counters(epilogue) if fold else []
        ops.linkpred_tail_neg(desc, loss_out=self.loss_dev if fold else None, accumulate=False,
                              mrr_out=self.mrr_dev if fold else None, counters=counters, jobs=neg_jobs, stream=e.stream)

    def _backward_unsup(self, B, n_roots, fuse_adam, wgrad_jobs=None, epilogue=None):
        """Reverse schedule.  The epilogue (loss / mrr means + device counters) runs FIRST: the fan-out sampler of a later
        step may ride in this pass's optimizer launch and must see the advanced sampler clock and pair cursor; the
        optimizer then uses step_offset = 0 if the step counter has been advanced already."""
        e = self.engine
        # dropout masks are a function of the device clock and the backward pass regenerates them: with dropout on, the
        # clock must not move before the backward pass has run (no sampler rides there: the prefetch pipeline is off)
        folded = epilogue is not None and getattr(self, "_epilogue_folded", False)     # already done by the forward pass
        early = epilogue is not None and not folded and self._dropout_rate() == 0.0
        if early:
            self._epilogue_unsup(B, **epilogue)
        advanced = (early or folded) and bool(epilogue.get("step"))
        e.begin_backward()
        if getattr(self, "_lp_tail_used", False):
            self._queue_tail_wgrads(n_roots, self._d_agg_out)
        else:
            self.link_pred_layer.bilinear_wgrad()          # dW of the bilinear affinity, queued with the other weight gradients
            self.aggregate_backward(self._d_agg_out)
        # every term of the loss is divided by batch_size (:378) -> so is the weight-decay gradient
        e.finish_backward(self.weight_decay / B, fuse_adam=fuse_adam, lr=self.learning_rate, clip=5.0, side_jobs=wgrad_jobs,
                          step_offset=0 if advanced else 1)
        if epilogue is not None and not early and not folded:
            self._epilogue_unsup(B, **epilogue)

    def _epilogue_unsup(self, B, **counters):
        self.engine.advance(loss_rows=self._loss_rows, n=B, loss_out=self.loss_dev, accumulate=self._loss_accumulate,
                            aux_rows=self._rr_rows, aux_out=self.mrr_dev, **counters)

    def _queue_tail_wgrads(self, n, dz):
        """The fused tail launch (either model's) already produced every input gradient; queue the weight gradients it feeds:
        layer 1's from dz = dLoss/dz [n, 2 O] (mean: z = [h0 W_self | means W_neigh]; GCN: its one matrix against the means over
        {neighbors} U {self}), then layer 0's from the tail's d_h0."""
        e = self.engine
        a1 = self.aggregators[1]
        if self.aggregator_type == "gcn":
            e.wgrad(a1.vars['weights'], self._tail_means, None, dz, 0, n)
        else:
            e.wgrad(a1.vars['self_weights'], self._tail_h0.rows_slice(0, n), None, dz, 0, n)
            e.wgrad(a1.vars['neigh_weights'], self._tail_means, None, dz, self.dims[2], n)
        self._tape[0][1].backward_hops(self._tail_dh0, True, embed_sink=None)

    def _optimize(self, advanced=False):
        """Data-parallel path: clip_by_value(+-5) + Adam after the all-reduce.  The local gradient is that of the local batch
        mean; the hook sums over ranks and grad_scale divides by world_size.  advanced: the step counter was already incremented
        by an earlier launch of this step."""
        e = self.engine
        e.adam(self.learning_rate, clip=5.0, grad_scale=1.0 / self.world_size, step_offset=0 if advanced else 1)
        if not advanced:
            e.advance(step=1)

    def _stage_feed_unsup(self, feed_dict):
        e = self.engine
        ph = self.placeholders
        self._parity = "h"         # host-fed batches own their buffers (see SupervisedGraphsage._stage_feed)
        self._pending_stage = None
        e.sync()
        b1 = np.ascontiguousarray(np.asarray(feed_dict[ph['batch1']]), dtype=np.int32)
        b2 = np.ascontiguousarray(np.asarray(feed_dict[ph['batch2']]), dtype=np.int32)
        B = int(b1.shape[0])
        assert b2.shape[0] == B and int(feed_dict.get(ph['batch_size'], B)) == B
        self._feed_dropout(feed_dict)
        roots, n_roots = self._roots(B, parity="h")
        roots[:B].copy_(torch.from_numpy(b1))
        roots[B:2 * B].copy_(torch.from_numpy(b2))
        torch.cuda.current_stream().synchronize()
        return roots, B, n_roots

    def _handover_error(self):
        """(error word of the fused tail's hand-over buffer, the launch's name, its waiting workgroups' name)."""
        err = ops.lp_tail_sync_error(self._lp_sync, *self._lp_sync_shape) if getattr(self, "_lp_sync", None) is not None else 0
        return err, "fused link-prediction tail", "main"

    def _sync_checked(self):
        """What every fetch does first: wait for the stream, then raise if the fused tail's in-kernel hand-over or the
        gradient exchange (peer-store exchange: a bounded device-side wait that tripped) reported an error."""
        self.engine.sync()
        err, launch, waiting = self._handover_error()
        if err:
            raise ops._lib.GraphsageAmdError(
                "%s: hand-over between its workgroups failed (flags %d: 1 = a %s workgroup gave up waiting for its helpers, "
                "2 = unexpected arrival count); results since the last fetch are invalid -- set model.fuse_tail = False to use "
                "the per-operator schedule" % (launch, err, waiting))
        if hasattr(self.grad_hook, "check"):
            self.grad_hook.check()

    def _fetch(self, B):
        return self._fetch_unsup(B)

    def _fetch_unsup(self, B, with_outputs=True):
        self._sync_checked()
        loss = float(self.loss_dev.item())
        mrr = float(self.mrr_dev.item())
        aff = self.aff_all.numpy()
        ranks = (aff[:, :-1] >= aff[:, -1:]).sum(axis=1)
        outs = self.outputs1.numpy() if with_outputs else None
        return loss, ranks, aff, mrr, outs

    def train_step(self, feed_dict, fetch=True):
        """sess.run([merged, opt_op, loss, ranks, aff_all, mrr, outputs1], feed_dict)  (unsupervised_train.py:273-274)."""
        roots, B, n_roots = self._stage_feed_unsup(feed_dict)

        def body(step, local_adam, tail):
            self._stage_negatives_or_injected(roots, B)
            self._step_fwd_bwd(B, (roots, n_roots), None, self._NO_SHARES, dict(step=step, clock=1), local_adam)
            tail()                # (_dispatch: a body calls tail() behind every step it issues)

        self._dispatch("utrain", (B,), body)
        return self._fetch_unsup(B) if fetch else None

    def eval_step(self, feed_dict):
        """sess.run([loss, ranks, mrr], feed_dict)  (unsupervised_train.py:69-71); also used for the (n, n) embedding
        pairs of save_val_embeddings (:94-117) -- `.outputs1` holds the embeddings of batch1."""
        roots, B, n_roots = self._stage_feed_unsup(feed_dict)

        def fwd():
            self._stage_negatives_or_injected(roots, B)
            self._forward_unsup(roots, B, n_roots, False, epilogue=dict(clock=1))
            if not self._epilogue_folded:
                self._epilogue_unsup(B, clock=1)

        self._run(("ueval", B, self._adj_version()), fwd)
        loss, ranks, aff, mrr, outs = self._fetch_unsup(B)
        return loss, ranks, mrr, outs

    # ---- device-resident epoch: edge pairs live in HBM; steady state is one hipGraph replay per step with the next
    #      step's sampling + gather co-scheduled with this step's launches ("the step schedule" below)
    def attach_device_pairs(self, pairs):
        e = self.engine
        if self.embeds is not None:
            raise NotImplementedError("the prefetching device-epoch path reads next-step rows before this step's update; "
                                      "with identity_dim > 0 use train_step(feed_dict)")
        self._pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)).to(e.device)
        self._cursor = torch.zeros(1, dtype=torch.int64, device=e.device)
        self._primed = None
        torch.cuda.synchronize()

    def set_epoch_pairs(self, pairs):
        self._reset_epoch(self._pairs, np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2))

    def _check_exchange(self):
        """A gradient exchange with bounded device-side waits (PeerPushAllReduce) reports a tripped wait through an error
        word: read it once per train_steps_device call, BEFORE further optimizer steps are issued on un-reduced gradients
        (costs one stream synchronisation per call; hooks without check() skip it)."""
        if hasattr(self.grad_hook, "check"):
            self.engine.sync()
            self.grad_hook.check()

    def _dp_in_graph(self):
        """Data-parallel AND the all-reduce hook can be recorded inside the step's hipGraph (NativeAllReduce)."""
        return self.grad_hook is not None and getattr(self.grad_hook, "capturable", False)

    def measure_dp_allreduce(self, log=None):
        """Duration of the gradient all-reduce as a stand-alone call (HIP events around eager calls of the hook on the
        gradient buffer -- every rank calls this, it is a collective): what the in-graph data-parallel step exposes per
        step, echoed by bench.py (dp_schedule)."""
        e = self.engine
        if not self._dp_in_graph():
            return None
        evs = [(ops.Event(), ops.Event()) for _ in range(12)]
        for a, b in evs:
            a.record(e.stream)
            self.grad_hook(self)
            b.record(e.stream)
        e.sync()
        ar_us = float(np.median([a.elapsed_ms(b) for a, b in evs[2:]])) * 1e3
        e.grads.zero_()
        torch.cuda.synchronize()
        if log:
            log("data-parallel schedule: all-reduce %.1f us stand-alone, recorded in the step graph behind the backward pass" % ar_us)
        return {"allreduce_us_standalone": ar_us}

    # ------------------------------------------------------------------------------ the step schedule (both models)
    # ONE schedule: which launch carries which share of the next step's gather, where the sampler rides, the form of the
    # optimizer (fused | in the graph behind a capturable hook | eager hook between two graphs) and the lengths / buffer
    # parities of the captured graphs.  What differs between the models is in these hooks, which SupervisedGraphsage overrides:
    #   _pipe_key              graph-key prefix of the pipelined steps
    #   _sample_roots          staging + sampling of the roots of one buffer parity
    #   _gather_shares         the next step's gather jobs divided over (layer-0 forward | tail | weight gradients | z launch)
    #   _step_fwd_bwd          the forward / backward pair of one step
    #   _sampler_to_wgrad_ok   may the riding sampler leave with the weight-gradient launch?  (supervised only)
    #   _multi_step_ok, _drop_prefetched, _dp_step_early     (see below)
    # The models also DIFFER in these points.  They are behaviour, kept as they were; do not "unify" them in passing:
    #   * Priming.  Both prime through _prime(), but the supervised model's _drop_prefetched() hands the staged ids back to the
    #     epoch cursor and the tick back to the sampler clock when the batch size changes; the unsupervised model hands nothing
    #     back (its _drop_prefetched is empty): after a change of B the pairs of the dropped batch are skipped.
    #   * In-graph data parallel (_dp_step_early).  Supervised: the tail launch / early epilogue advances the step counter
    #     (epilogue step = 1) and the optimizer behind the hook runs with advanced=True.  Unsupervised: the epilogue leaves the
    #     step counter alone (step = 1 only with the local optimizer) and _optimize() advances it in a launch of its own.
    #   * Eligibility.  The supervised model pipelines (and takes multi-step graphs) only with `pipeline` on and no dropout, and
    #     has the non-pipelined "dtrain" form for the rest; the unsupervised model always pipelines and has no such form.
    #   * Sampler segments.  _root_segments: three segments (batch1 | batch2 | negatives) here, None for the supervised model.
    _pipe_key = "updtrain"
    _dp_step_early = False
    _NO_SHARES = (None, None, None, None)

    def _sample_roots(self, B, parity):
        """Stage and sample the roots of buffer `parity`: (what _step_fwd_bwd needs of them, root rows, samples, support)."""
        roots, n_roots = self._roots(B, parity=parity)
        stage = None
        if self._fanout_fusable():
            # the edge-pair batch and the negatives are staged by the fan-out sampler launch itself (one launch, and
            # one that can ride in the optimizer launch)
            stage = ("unsup", self._pairs, self._cursor, B, self._neg_cdf, self._neg_guide, self._guide_bits,
                     self.neg_sample_size, self.neg_seed)
        else:
            self._stage_negatives(roots, B, pairs=self._pairs, cursor=self._cursor)
        samples, support = self._sample_phase(roots, n_roots, parity, stage=stage)
        return (roots, n_roots), n_roots, samples, support

    def _gather_shares(self, jobs):
        tail_jobs = []
        if self._lp_tail_ok() and self.cogather_lp_tail > 0:
            # three-launch form (layer-0 forward | fused link-prediction tail | weight gradients): the tail is long and
            # thin (66 main workgroups), the rest of the chip streams its share of the gather at the full rate
            f_fwd, f_tail = self.cogather_lp_fwd, self.cogather_lp_tail + self.cogather_lp_neg
            fwd_jobs, rest = ops.split_gather_jobs(jobs, f_fwd)
            tail_jobs, wgrad_jobs = ops.split_gather_jobs(rest, min(1.0, f_tail / max(1e-6, 1.0 - f_fwd)))
        else:
            fwd_jobs, wgrad_jobs = ops.split_gather_jobs(jobs, self.cogather_split)
        z_jobs = []
        if not tail_jobs and self.cogather_z > 0 and len(self.num_samples) > 1 and not self._lp_tail_ok():
            # the last layer's lean launch (gs_sage_tail_z) leaves most of the chip idle: a share rides there at
            # the full HBM rate
            wgrad_jobs, z_jobs = ops.split_gather_jobs(wgrad_jobs, max(0.0, 1.0 - self.cogather_z / max(1e-6, 1.0 - self.cogather_split)))
        return fwd_jobs, tail_jobs, wgrad_jobs, z_jobs

    def _step_fwd_bwd(self, B, roots, prefetched, shares, epilogue, local_adam):
        roots, n_roots = roots
        fwd_jobs, tail_jobs, wgrad_jobs, z_jobs = shares
        self._forward_unsup(roots, B, n_roots, True, prefetched=prefetched, side_jobs=fwd_jobs, epilogue=epilogue, z_jobs=z_jobs,
                            tail_jobs=tail_jobs)
        self._backward_unsup(B, n_roots, fuse_adam=local_adam, wgrad_jobs=wgrad_jobs, epilogue=epilogue)

    def _sampler_to_wgrad_ok(self, jobs):
        return False

    def _multi_step_ok(self):
        """May train_steps_device replay several steps per graph launch?  (One GPU, or the exchange recorded in the graph.)"""
        return self.grad_hook is None or self._dp_in_graph()

    def _drop_prefetched(self):
        """The batch size changes under a primed pipeline: nothing is handed back here (see the list above)."""

    def _reset_epoch(self, table, values):
        """New epoch: `values` into the device-resident order / pair list, the cursor back to 0."""
        self.engine.sync()  # steps still queued on the engine stream read the old order / cursor
        table.copy_(torch.from_numpy(values))
        self._cursor.zero_()
        if self._primed is not None:
            # a prefetched-but-unused batch of the old order is dropped: give its sampler-clock tick back so the
            # pipelined schedule draws exactly the samples of the sequential one
            self.engine.sample_clock_dev -= 1
        self._primed = None
        torch.cuda.synchronize()

    def _dispatch(self, prefix, key, body):
        """One launch unit -- a single step, or k pipelined ones -- in the form the gradient exchange allows: the whole unit one
        hipGraph (no hook: key `prefix`) | data parallel with a capturable hook: exchange and optimizer inside the graph too, once
        per step (`prefix`_dp) | forward + backward graph (`prefix`_fb), eager hook, ("opt",) graph.
        body(step, local_adam, tail) issues the steps: `step` is the epilogue's increment of the optimizer step counter,
        local_adam says whether the backward pass applies clip + Adam itself, and tail() is called behind every step."""
        local_adam, in_graph = self.grad_hook is None, self._dp_in_graph()
        step = 1 if local_adam or (in_graph and self._dp_step_early) else 0

        def tail():
            if in_graph:
                self.grad_hook(self)          # ncclAllReduce on the engine stream, recorded in the graph
                self._optimize(advanced=bool(step))

        self._run((prefix + ("" if local_adam else "_dp" if in_graph else "_fb"),) + key + (self._adj_version(),),
                  lambda: body(step, local_adam, tail))
        if not (local_adam or in_graph):
            self.grad_hook(self)              # all-reduce of engine.grads (ordered by stream events)
            self._run(("opt",), self._optimize)

    def _prime(self, n):
        """Fill the pipeline: the data chain (staging, sampling, layer-0 gather + mean) of the first step, into parity 0."""
        if self._primed == n:
            return
        e = self.engine
        self._drop_prefetched()
        self._pipe_parity = 0
        roots, rows, samples, support = self._sample_roots(n, 0)
        self_all, neighs = self._layer0_inputs(samples, support, rows)
        means0 = self.aggregators[0].prefetch(self_all, neighs, tag=0) if self_all is not None else None
        e.advance(clock=1, cursor=self._cursor, cursor_delta=n)
        self._prefetched[(n, 0)] = (roots, (samples, support, means0))   # static views of persistent buffers
        e.sync()
        self._primed = n

    def _pipelined_steps(self, n, k):
        """k consecutive pipelined steps as ONE hipGraph launch (k even, or 1); the pipeline is primed.

        Single stream: step t first samples step t+1 (one small launch, or riding in an optimizer launch), then its
        launches carry step t+1's gather+mean waves along (horizontal fusion): no cross-stream dependency.  Buffers alternate by
        parity; the batches, samples and updates are exactly those of the sequential schedule.  (A second-stream fork/join
        pipeline and a forked gather branch beside the all-reduce were built and measured in rounds 2-3 -- 152-162 us against
        118, 149.9 against 147.9 -- and removed in round 4: benchmarks/variants/README.md.)"""
        e = self.engine
        p0 = self._pipe_parity
        fused = self.grad_hook is None or self._dp_in_graph()
        assert fused or k == 1
        per_root = 1
        for f in self.num_samples[:0:-1]:
            per_root *= f
        # sampler-in-optimizer-launch: inside a multi-step graph the sampler of the step after next rides in this step's
        # optimizer launch.  The device counters are advanced BEFORE that launch -- by the fused tail launch, the folded
        # epilogue or the early epilogue of the backward pass
        ride = self.sampler_rides and fused and k > 1 and self._fanout_fusable() and per_root <= 512

        def body(step, local_adam, tail):
            p, staged = p0, None
            for j in range(k):
                q = 1 - p
                if staged is None:
                    staged = self._sample_roots(n, q)               # standalone sampler launch (first step of a graph)
                roots_q, rows_q, samples, support = staged
                self_all, neighs = self._layer0_inputs(samples, support, rows_q)
                means_q, jobs = self.aggregators[0].prefetch_jobs(self_all, neighs, tag=q)
                staged = None
                if ride and j + 1 < k:
                    # by the time the optimizer launch runs, this step's own id / label buffers (parity p) are free and the
                    # sampler clock and the epoch cursor have been advanced: the draws are those of the standalone launch
                    with e.deferring_sampler():
                        staged = self._sample_roots(n, p)
                    if e._deferred_sampler is None:
                        raise ops._lib.GraphsageAmdError("sampler did not take the one-launch fan-out path")
                self._prefetched[(n, q)] = (roots_q, (samples, support, means_q))
                roots, pre = self._prefetched[(n, p)]
                self._parity = p
                # the next step's gather is split between this step's big launches: they are latency-bound, so the HBM-bound
                # gather waves back-fill their idle slots
                shares = self._gather_shares(jobs)
                # (fused-tail supervised models, opt-in: the riding sampler leaves with the weight-gradient launch instead --
                #  Engine.launch_wgrads -- and the tail launch copies this step's ids for the weight gradients, whose id buffer
                #  the sampler refills)
                e._sampler_to_wgrad = self._sampler_to_wgrad_ok(jobs)
                try:
                    self._step_fwd_bwd(n, roots, pre, shares, dict(step=step, clock=1, cursor=self._cursor, cursor_delta=n),
                                       local_adam)
                finally:
                    if e._sampler_to_wgrad:
                        self._wgrad_sampler_seen = bool(e.last_wgrad_sampler)   # (tests: did the sampler leave with that launch?)
                    e._sampler_to_wgrad = False
                if e._deferred_sampler is not None:
                    raise ops._lib.GraphsageAmdError("deferred sampler was not consumed by the optimizer launch")
                tail()
                p = q

        self._dispatch(self._pipe_key, (n, k, p0), body)
        if k % 2 == 1:
            self._pipe_parity = 1 - p0

    def train_step_device(self, n, fetch=False):
        """One training step on the next n ids / pairs of the device-resident epoch: the step's launches carry the data chain
        of the step after it (batch staging + fan-out sampling + layer-0 gather-means; HBM-bound, needs no weights)."""
        self._prime(n)
        self._pipelined_steps(n, 1)
        return self._fetch(n) if fetch else None

    def train_steps_device(self, n, steps, steps_per_launch=8):
        """`steps` training steps on the device-resident epoch; on a single GPU (or with the exchange in the graph)
        `steps_per_launch` consecutive steps are replayed per hipGraph launch (amortises the launch gap and keeps the GPU fed
        when the host is slow or shared; the schedule and results are unchanged)."""
        k = steps_per_launch - (steps_per_launch % 2)
        if not (self._multi_step_ok() and self.use_graphs and k >= 2):
            for _ in range(steps):
                self.train_step_device(n)
            return
        done = 0
        while done < steps:
            # multi-step graphs always start at buffer parity 0 (one captured graph per length); single steps realign the
            # parity.  A shorter tail (the drivers replay print_every - 1 steps between two printed iterations) takes the
            # largest even length that fits, so it still is one launch with the sampler riding in the optimizer launches.
            rem = steps - done
            kk = min(k, rem - (rem % 2))
            if self._primed == n and self._pipe_parity == 0 and kk >= 2:
                self._pipelined_steps(n, kk)
                done += kk
            else:
                self.train_step_device(n)
                done += 1
        self._check_exchange()

    # ------------------------------------------------------------------------------ sample (S2)
    def ids_buffer(self, batch_size, layer_infos=None, parity=None):
        """One contiguous int32 buffer [batch | hop-1 samples | hop-2 samples | ...] so that the rows of all hops
        of a layer are adjacent (lets `aggregate` run every hop of a layer in one launch).  Returns
        (buffer, offsets) with offsets[k] = start of samples[k]."""
        layer_infos = layer_infos or self.layer_infos
        sizes = [batch_size]
        support = 1
        for k in range(len(layer_infos)):
            support *= layer_infos[len(layer_infos) - k - 1].num_samples
            sizes.append(batch_size * support)
        offsets = [0]
        for sz in sizes:
            offsets.append(offsets[-1] + sz)
        if parity is None:
            parity = getattr(self, "_parity", 0)
        buf = self.engine.ws_i32(("ids_all", tuple(sizes), parity), offsets[-1])
        return buf, offsets

    def _fanout_fusable(self, layer_infos=None):
        """Will model.sample() on the contiguous id buffer take the one-launch fan-out path?"""
        from .neigh_samplers import CSRAdjacency
        layer_infos = layer_infos or self.layer_infos
        sampler0 = layer_infos[0].neigh_sampler
        return (len(layer_infos) <= 3 and all(li.neigh_sampler is sampler0 for li in layer_infos)
                and isinstance(sampler0.adj_info.current, CSRAdjacency) and getattr(self, "fuse_sampler", True))

    def sample(self, inputs, layer_infos, batch_size=None):
        """Sample neighbors to be the supportive fields for multi-layer convolutions
        (models.py:254-275).  `inputs`: int32 device vector of batch node ids.  When `inputs` is the head of
        the model's contiguous id buffer, the sampled hops are written right behind it."""
        if batch_size is None:
            batch_size = inputs.numel()
        samples = [inputs]
        support_size = 1
        support_sizes = [support_size]
        buf, offsets = self.ids_buffer(batch_size, layer_infos)
        contiguous = inputs.data_ptr() == buf.data_ptr() and inputs.numel() == batch_size
        K = len(layer_infos)
        sampler0 = layer_infos[0].neigh_sampler
        fused = contiguous and self._fanout_fusable(layer_infos)
        stage = getattr(self, "_pending_stage", None)
        self._pending_stage = None
        if fused:
            # every hop (and, on the device-epoch path, batch + label staging) in ONE launch with an LDS fan-out buffer
            fans = [layer_infos[K - k - 1].num_samples for k in range(K)]
            per_root = 1
            for f in fans[:-1]:
                per_root *= f
            if per_root <= 8192:
                sampler0.fanout(buf, offsets, fans, batch_size, root_offset=getattr(self, "row_offset", 0), stage=stage)
                for k in range(K):
                    support_size *= fans[k]
                    samples.append(buf[offsets[k + 1]: offsets[k + 2]])
                    support_sizes.append(support_size)
                return samples, support_sizes
        if stage is not None:
            order, cursor, table, labels_out = stage
            ops.stage_batch(order, cursor, batch_size, inputs, table, labels_out, stream=self.engine.stream)
        for k in range(len(layer_infos)):
            t = len(layer_infos) - k - 1
            sampler = layer_infos[t].neigh_sampler
            # this rank's first global row at this hop (keeps draws independent of the DP sharding)
            sampler.global_row_offset = getattr(self, "row_offset", 0) * support_size
            support_size *= layer_infos[t].num_samples
            if contiguous:
                sampler.next_out = buf[offsets[k + 1]: offsets[k + 2]]
            if sampler.root_segments is not None:
                rows_per_root = samples[k].numel() // batch_size
                sampler.call_segments = tuple(b * rows_per_root for b in sampler.root_segments)
            node = sampler((samples[k], layer_infos[t].num_samples))
            samples.append(node.reshape(support_size * batch_size))
            support_sizes.append(support_size)
        return samples, support_sizes

    # ------------------------------------------------------------------------------ aggregate (A0/A1)
    def make_aggregators(self, dims, num_samples, concat, model_size, name=None):
        """Aggregator construction of models.py:303-315 (one per layer, last layer identity act)."""
        aggregators = []
        for layer in range(len(num_samples)):
            dim_mult = 2 if concat and (layer != 0) else 1
            if layer == len(num_samples) - 1:
                aggregator = self.aggregator_cls(dim_mult * dims[layer], dims[layer + 1], act=identity,
                                                 dropout=self.placeholders['dropout'], name=name, concat=concat,
                                                 model_size=model_size)
            else:
                aggregator = self.aggregator_cls(dim_mult * dims[layer], dims[layer + 1],
                                                 dropout=self.placeholders['dropout'], name=name, concat=concat,
                                                 model_size=model_size)
            aggregators.append(aggregator)
        return aggregators

    def layer_inputs(self, hidden, layer, batch_size, num_samples, support_sizes, dims, concat):
        """(self_all, neighs, rows, offsets) of one layer: the contiguous self rows of all hops and the per-hop
        neighbor views reshaped as models.py:323-327."""
        K = len(num_samples)
        n_hops = K - layer
        dim_mult = 2 if concat and (layer != 0) else 1
        neighs = []
        for hop in range(n_hops):
            neigh_dims = [batch_size * support_sizes[hop], num_samples[K - hop - 1], dim_mult * dims[layer]]
            neighs.append(hidden[hop + 1].reshape(neigh_dims))
        self_all = contiguous_rows(hidden[:n_hops])
        rows = [hidden[h].n for h in range(n_hops + 1)]
        offsets = [0]
        for r in rows:
            offsets.append(offsets[-1] + r)
        return self_all, neighs, rows, offsets

    def aggregate(self, samples, input_features, dims, num_samples, support_sizes, batch_size=None,
                  aggregators=None, name=None, concat=False, model_size="small", layer0_means=None,
                  layer0_side_jobs=None, _stop_after_layer=None, last_layer_side_jobs=None):
        if batch_size is None:
            batch_size = samples[0].numel()
        features = input_features[0] if isinstance(input_features, (list, tuple)) else input_features
        # hidden[h] = embedding_lookup(features, samples[h]) -- kept LAZY (models.py:299)
        hidden = [Rows(features, node_samples, requires_grad=False) for node_samples in samples]
        new_agg = aggregators is None
        if new_agg:
            aggregators = self.make_aggregators(dims, num_samples, concat, model_size, name)
            self.engine.finalize()
        tape = []
        K = len(num_samples)
        for layer in range(K):
            aggregator = aggregators[layer]
            n_hops = K - layer
            self_all, neighs, rows, offsets = self.layer_inputs(hidden, layer, batch_size, num_samples, support_sizes,
                                                               dims, concat)
            if self_all is not None:
                means = layer0_means if layer == 0 else None
                jobs = layer0_side_jobs if layer == 0 else (last_layer_side_jobs if layer == K - 1 else None)
                h_all = aggregator.call_hops(self_all, neighs, means=means, side_jobs=jobs)   # all hops, one launch
                outs = [h_all.rows_slice(offsets[h], offsets[h + 1]) for h in range(n_hops)]
                tape.append(("batched", aggregator, rows, offsets, h_all))
            else:                                                           # non-adjacent inputs: hop by hop (:326)
                outs = [aggregator((hidden[hop], neighs[hop])) for hop in range(n_hops)]
                tape.append(("per_hop", aggregator, rows, offsets, outs))
            hidden = [Rows(o, None, requires_grad=True) for o in outs]
            if _stop_after_layer is not None and layer == _stop_after_layer:
                break          # the remaining layers run inside a fused launch (SupervisedGraphsage._forward)
        self._tape = tape
        return hidden[0].src, aggregators

    def aggregate_backward(self, d_out):
        """Reverse schedule of `aggregate`.  d_out: Mat = dLoss/d(hidden[0] of the last layer).
        No gradient flows into the fixed feature columns (models.py:238: trainable=False)."""
        e = self.engine
        tape = self._tape
        d_cur, pre_masked = d_out, False
        for layer in range(len(tape) - 1, -1, -1):
            mode, agg, rows, offsets, outs = tape[layer]
            if mode != "batched":
                raise NotImplementedError("backward through non-contiguous hop inputs (use the model's id buffer)")
            if layer == 0:
                # the fixed features need no gradient; trainable identity columns get theirs scattered per id
                agg.backward_hops(d_cur, pre_masked, embed_sink=self._embed_sink())
                break
            prev_mode, prev_agg, prev_rows, prev_offsets, prev_out = tape[layer - 1]
            d_prev = e.ws_mat((self.name, "d_hidden", layer - 1), prev_out.rows, prev_out.d)
            # the previous layer is never the last one, so its activation is relu (models.py:307-314): its
            # relu gradient is fused into the scatter of this layer's input gradients
            mask = prev_out if prev_agg.act_code == ops.ACT_RELU else None
            agg.backward_hops(d_cur, pre_masked, d_prev=d_prev, prev_mask=mask, prev_offsets=prev_offsets)
            d_cur, pre_masked = d_prev, mask is not None

    # ------------------------------------------------------------------------------ full-neighborhood inference
    def embed_full(self, graph, nodes=None):
        """l2-normalised embeddings (models.py:368-370) [n, d] (NumPy) of `nodes` (default: all N real nodes in id order) from
        the exact layer-wise pass over `graph` (inference.FullGraph): every layer for every node from ALL its neighbors."""
        from . import inference as inf
        return self._l2_numpy(*inf.select_rows(self, inf.layers_full(self, graph), nodes))

    def _l2_numpy(self, rows, n):
        from . import inference as inf
        y = inf.l2_rows(self.engine, rows, n)
        self.engine.sync()
        return y.numpy()[:n]

    def embed_nodes(self, graph, nodes):
        """(embeddings [n, d] (NumPy), stats): embed_full(graph, nodes) computed from the receptive field of `nodes` alone
        (inference.layers_nodes): layer l only for the rows layer l + 1 of the request reads, found on the device.  Rows in
        REQUEST order, a duplicate request answered twice.  stats = {"rows": [|S_K|, ..., |S_0|], "edges": [...], "n_rows":
        N + 1}.  The values agree with embed_full to the float tolerance, not bitwise: the contractions may take another tile
        form at another row count."""
        from . import inference as inf
        H, S, _, stats = inf.layers_nodes(self, graph, nodes)
        return self._l2_numpy(*inf.request_rows(self, H, S, nodes)), stats

    def _exact_table(self, graph):
        """The l2-normalised exact table of `graph` [N + 1, d], pad row included, kept on the device (Mat)."""
        from . import inference as inf
        H = inf.layers_full(self, graph)
        return inf.l2_rows(self.engine, H, H.rows)

    def rank_full(self, graph, edges, filtered=True, hits=(1, 10, 50, 100)):
        """Rank the true partner of every edge (src, dst) among ALL N nodes with the exact embeddings of `graph` (the table of
        embed_full, kept on the device): inference.rank_full with n_cand = N (the pad row is never a candidate), the query
        node left out, the edges of `graph` filtered (filtered=True) and the head's bilinear weights if it has them."""
        from . import inference as inf
        W = self.link_pred_layer.vars['weights'].value if self.bilinear_weights else None
        return inf.rank_full(self.engine, self._exact_table(graph), edges, n_cand=graph.n_nodes,
                             filt=graph.rank_filter() if filtered else None, weights=W, hits=hits)

    def topk_full(self, graph, nodes=None, k=10, filtered=True):
        """The k best-scoring partners of `nodes` (default: all N real nodes in id order) among ALL N nodes with the exact
        embeddings of `graph` (the table of embed_full, kept on the device): inference.topk_full with n_cand = N (the pad row is
        never a candidate), the query node left out, the edges of `graph` filtered (filtered=True) and the head's bilinear weights
        if it has them.  Returns {"ids": int32 [n, k], "scores": float32 [n, k], "count": int32 [n]}."""
        from . import inference as inf
        W = self.link_pred_layer.vars['weights'].value if self.bilinear_weights else None
        return inf.topk_full(self.engine, self._exact_table(graph), np.arange(graph.n_nodes) if nodes is None else nodes, k,
                             n_cand=graph.n_nodes, filt=graph.rank_filter() if filtered else None, weights=W)

    def topk_ivf(self, graph, nodes=None, k=10, nprobe=8, n_clusters=0, filtered=True, seed=123, index=None):
        """topk_full through an inverted file (retrieval.IVFIndex): the same table, candidates (n_cand = N), filter and bilinear
        weights, but every query sees only the members of the nprobe lists it probes.  index: a retrieval.IVFIndex built by an
        earlier call on this graph and these weights (None: retrieval.build_ivf with n_clusters lists, 0 = 4 sqrt(N), seeded
        by `seed`).  Returns topk_full's dict plus "scanned" (int64 [n]) and "index"."""
        from . import retrieval
        W = self.link_pred_layer.vars['weights'].value if self.bilinear_weights else None
        if index is None:
            index = retrieval.build_ivf(self.engine, self._exact_table(graph), n_clusters, n_cand=graph.n_nodes, seed=seed)
        res = index.search(np.arange(graph.n_nodes) if nodes is None else nodes, k, nprobe,
                           filt=graph.rank_filter() if filtered else None, weights=W)
        res["index"] = index
        return res

    # ------------------------------------------------------------------------------ step machinery (shared)
    def _samplers(self):
        seen = []
        for li in self.layer_infos:
            if li.neigh_sampler not in seen:
                seen.append(li.neigh_sampler)
        return seen

    def _sample_phase(self, batch, n, parity, stage=None):
        """Batch/label staging + neighbor sampling into the parity-keyed id buffer (weight-free)."""
        self._parity = parity
        self.reset_tapes()      # a forward-only step (eval) leaves saved activations behind: buffer keys count them
        for s in self._samplers():
            s.new_step()
            # the unsupervised model's one pass over [batch1 | batch2 | negatives] stands for three sample() calls of the
            # reference (:347-357), each with its own column permutations
            s.root_segments = self._root_segments(n)
            s.calls_per_sample = len(self.layer_infos)
        self._pending_stage = stage
        try:
            return self.sample(batch, self.layer_infos, n)
        finally:
            for s in self._samplers():
                s.root_segments = None

    def _root_segments(self, n_roots):
        """(start of batch2, start of the negatives) inside the roots [batch1 | batch2 | negatives] of the unsupervised
        pass (this class); the supervised subclass has one sample() call per step and returns None."""
        B = (n_roots - self.neg_sample_size) // 2
        return (B, 2 * B)

    def _layer0_inputs(self, samples, support_sizes, n):
        hidden = [Rows(self.features, sm, requires_grad=False) for sm in samples]
        self_all, neighs, _, _ = self.layer_inputs(hidden, 0, n, self.num_samples, support_sizes, self.dims, self.concat)
        return self_all, neighs

    def _data_phase(self, batch, n, parity, stage=None):
        """The weight-free half of a step: batch/label staging, neighbor sampling and the layer-0 gather+mean.
        Writes only parity-keyed buffers, so it can run ahead of (or concurrently with) the previous step's compute."""
        samples, support_sizes = self._sample_phase(batch, n, parity, stage)
        self_all, neighs = self._layer0_inputs(samples, support_sizes, n)
        means0 = self.aggregators[0].prefetch(self_all, neighs, tag=parity) if self_all is not None else None
        return samples, support_sizes, means0

    def _schedule_signature(self):
        """Everything that shapes the launches a captured step graph contains: changing one of these on a live model
        (tests and A/B runs do) selects / captures another graph instead of silently replaying the old one."""
        e = self.engine
        law = tuple((s.law, s.max_degree, s.seed) for s in self._samplers())
        return (getattr(self, "fuse_tail", True), getattr(self, "fuse_head", True), getattr(self, "fuse_sampler", True),
                self.sampler_rides, self.cogather_split, self.cogather_split3, self.cogather_tail, self.tail_split,
                self.cogather_auto, self.tail_halves, self.tail_free_bytes, self.sampler_in_wgrad, self.sampler_in_wgrad_max_bytes,
                self.cogather_z, self.cogather_lp_fwd, self.cogather_lp_tail, self.cogather_lp_neg, e.stream_gemm, e.tiled3_fwd, e.fused_l1_means, e.fused_l1_means_unsup, e.tiled3_wgrad, e.tiled3_wgrad_acut, e.split_pool, e.pool_f16, str(getattr(self, "pipeline", None)),
                type(self.grad_hook).__name__,
                id(self.grad_hook), law)

    def _run(self, key, fn):
        """Eager on first use, captured into a hipGraph on the second, replayed afterwards.  The Python attributes
        that name a step's output buffers are snapshotted per key and restored on replay (the Python of `fn` does
        not run again, and other step shapes -- e.g. a validation batch -- may have re-pointed them meanwhile)."""
        e = self.engine
        # the dropout rate and the schedule choices are baked into the captured launches
        key = tuple(key) + (self._dropout_rate(), self._schedule_signature())
        outs = self._graph_outputs.get(key)
        if outs is not None:
            for name, val in outs.items():
                setattr(self, name, val)
        if _run_captured(self._graphs, self._warm, key, fn, e.stream, lambda: self.use_graphs and not self._needs_host_rng()):
            self._graph_outputs[key] = {name: getattr(self, name) for name in self._OUT_ATTRS if hasattr(self, name)}

    def _feed_dropout(self, feed_dict):
        """feed_dict[placeholders['dropout']] (supervised_train.py:117; validation feeds omit it = 0): every layer
        holds the placeholder and reads the rate when it runs."""
        ph = self.placeholders['dropout']
        ph.value = float(feed_dict.get(ph, 0.0))
        return self._dropout_rate()

    def _dropout_rate(self):
        from .layers import _rate
        return _rate(self.placeholders['dropout']) if self.placeholders and 'dropout' in self.placeholders else 0.0

    def _needs_host_rng(self):
        from .neigh_samplers import PaddedAdjacency
        return any(isinstance(s.adj_info.current, PaddedAdjacency) for s in self._samplers())

    def _adj_version(self):
        return tuple(id(s.adj_info.current) for s in self._samplers())

    def reset_tapes(self):
        if self.aggregators:
            for a in self.aggregators:
                a.reset()
        self._tape = None


class Node2VecModel(object):
    """Simple version of the Node2Vec / DeepWalk algorithm (graphsage/models.py:408-504) on the gfx950 engine: trainable
    target / context embedding tables [dict_size, nodevec_dim] and a context bias [dict_size], trained by plain SGD on the
    skip-gram cross-entropy against `neg_sample_size` DISTINCT degree^0.75 negatives shared by the batch.

        loss, ranks, aff_all, mrr, outputs1 = model.train_step(feed_dict)   # unsupervised_train.py:273-274
        loss, ranks, mrr, outputs1 = model.eval_step(feed_dict)             # no update (evaluate, save_val_embeddings)

    dict_size: rows of the tables (the driver passes N + 1, the pad row included); degrees: the N TRAIN degrees (the
    unigrams of the negative sampler); nodevec_dim in {64, 128, 256, 512}; lr: the SGD learning rate.  The reference reads
    FLAGS.neg_sample_size; here it is the keyword neg_sample_size.  A step is three launches (csrc/gs_n2v.hip): staging |
    forward + gradient rows | sparse apply; the tables are updated in place and never copied.  identity_dim, dropout and
    weight_decay have no meaning for this model, as in the reference.  Data-parallel training needs a sparse exchange and
    is refused.  Initial values come from a seeded host stream; device_init=True draws the same distributions with torch's
    generator on the device instead (tables of 10^7 rows would take minutes to draw and upload from the host)."""

    def __init__(self, placeholders, dict_size, degrees, name=None, nodevec_dim=50, lr=0.001, neg_sample_size=20, seed=123,
                 grad_hook=None, world_size=1, device_init=False, **kwargs):
        if grad_hook is not None or int(world_size) > 1:
            raise NotImplementedError("Node2VecModel is single-GPU: its sparse row updates have no gradient exchange")
        self.engine = e = get_engine()
        self.name = name or "node2vecmodel"
        self.placeholders = placeholders
        self.degrees = np.asarray(degrees)
        self.dict_size = int(dict_size)
        self.hidden_dim = d = int(nodevec_dim)
        self.lr = float(lr)
        self.neg_sample_size = n_neg = int(neg_sample_size)
        lib = ops._lib.load()
        if not lib.gs_n2v_supported(d, n_neg):
            raise ops._lib.GraphsageAmdError(
                "Node2VecModel: nodevec_dim = 2 * dim_1 must be one of 64 / 128 / 256 / 512 and neg_sample_size must fit "
                "LDS beside the workgroup's rows (got nodevec_dim=%d, neg_sample_size=%d)" % (d, n_neg))
        if len(self.degrees) > self.dict_size:
            raise ValueError("Node2VecModel: %d degrees for a table of %d rows" % (len(self.degrees), self.dict_size))
        # following the tensorflow word2vec tutorial (models.py:434-445): uniform [-1, 1), truncated normal (draws beyond two
        # standard deviations are re-drawn) with stddev 1 / sqrt(d), zeros -- from a seeded host stream
        if device_init:
            gen = torch.Generator(device=e.device)
            gen.manual_seed(seed)
            self.target_embeds = torch.rand((self.dict_size, d), device=e.device, generator=gen) * 2.0 - 1.0
            self.context_embeds = torch.empty((self.dict_size, d), dtype=torch.float32, device=e.device)
            torch.nn.init.trunc_normal_(self.context_embeds, mean=0.0, std=1.0 / np.sqrt(d), a=-2.0 / np.sqrt(d),
                                        b=2.0 / np.sqrt(d), generator=gen)
        else:
            rng = np.random.RandomState(seed)
            target = rng.uniform(-1.0, 1.0, size=(self.dict_size, d)).astype(np.float32)
            ctx = rng.standard_normal((self.dict_size, d))
            far = np.abs(ctx) > 2.0
            while far.any():
                ctx[far] = rng.standard_normal(int(far.sum()))
                far = np.abs(ctx) > 2.0
            ctx = (ctx / np.sqrt(d)).astype(np.float32)
            self.target_embeds = torch.from_numpy(target).to(e.device)
            self.context_embeds = torch.from_numpy(ctx).to(e.device)
        self.context_bias = torch.zeros(self.dict_size, dtype=torch.float32, device=e.device)
        # fixed unigram distribution ~ degree^0.75, as SampleAndAggregate.build; unique=True (:449-456)
        if np.power(self.degrees.astype(np.float64), 0.75).sum() <= 0:
            raise ValueError("Node2VecModel: every degree is zero, there is nothing to draw negatives from")
        self._guide_bits = 18
        cdf, guide = unigram_cdf(self.degrees, self._guide_bits)
        steps_up = np.concatenate([[0], cdf.astype(np.uint64)])
        reachable = int((steps_up[1:] > steps_up[:-1]).sum())
        if reachable < n_neg:
            # tf.nn.fixed_unigram_candidate_sampler(unique=True) would spin for ever
            raise ValueError("Node2VecModel: neg_sample_size = %d distinct negatives, but only %d nodes have a non-zero "
                             "sampling weight" % (n_neg, reachable))
        self._neg_cdf = torch.from_numpy(cdf.view(np.int32).copy()).to(e.device)
        self._n_cdf = int(cdf.shape[0])
        self._neg_guide = torch.from_numpy(guide).to(e.device)
        self.neg_seed = 123
        self.clock_dev = torch.zeros(1, dtype=torch.int64, device=e.device)
        self.loss_dev = torch.zeros(1, dtype=torch.float32, device=e.device)
        self.mrr_dev = torch.zeros(1, dtype=torch.float32, device=e.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=e.device)
        self.use_graphs = True
        self._bufs, self._graphs, self._warm = {}, {}, set()
        self._injected_neg = None
        self._pairs = self._cursor = None
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------------ buffers / launches
    def _buffers(self, B, tag):
        key = (int(B), tag)
        b = self._bufs.get(key)
        if b is None:
            e, d, n_neg = self.engine, self.hidden_dim, self.neg_sample_size
            n_slabs = int(ops._lib.load().gs_n2v_slabs(B, d, n_neg))
            f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=e.device)
            b = dict(B=int(B), n_slabs=n_slabs, ids=torch.zeros(2 * B + n_neg, dtype=torch.int32, device=e.device),
                     loss_rows=f(B), rr_rows=f(B), aff_all=f(B, n_neg + 1), outputs1=f(B, d), g_target=f(B, d), g_ctx=f(B, d),
                     g_bias=f(B), neg_slabs=f(n_slabs, n_neg, d), bias_slabs=f(n_slabs, n_neg))
            torch.cuda.synchronize()
            self._bufs[key] = b
        return b

    def _stage(self, b, pairs=None, cursor=None):
        ops.call("gs_n2v_stage", ops.ptr(pairs), pairs.shape[0] if pairs is not None else 0, ops.ptr(cursor), b["B"],
                 ops.ptr(self._neg_cdf), self._n_cdf, self.neg_sample_size, self.neg_seed, ops.ptr(self.clock_dev), 0,
                 ops.ptr(self._neg_guide), self._guide_bits, ops.ptr(b["ids"]), ops.ptr(self._status), self.engine.stream)

    def _fwd_bwd(self, b, train):
        P = ops.ptr
        d = self.hidden_dim
        ops.call("gs_n2v_fwd_bwd", P(self.target_embeds), d, P(self.context_embeds), d, P(self.context_bias), self.dict_size,
                 P(b["ids"]), b["B"], d, self.neg_sample_size, 1 if train else 0, P(b["loss_rows"]), P(b["rr_rows"]),
                 P(b["aff_all"]), self.neg_sample_size + 1, P(b["outputs1"]), d, P(b["g_target"]), P(b["g_ctx"]),
                 P(b["g_bias"]), P(b["neg_slabs"]), P(b["bias_slabs"]), self.engine.stream)

    def _apply(self, b, cursor=None):
        """GradientDescentOptimizer(lr).minimize(loss) (models.py:447, 474-475) on the rows of this step, with the step
        epilogue (mean loss / mrr, sampler clock + 1, epoch cursor + B) as an extra workgroup."""
        P = ops.ptr
        d = self.hidden_dim
        ops.call("gs_n2v_apply", P(self.target_embeds), d, P(self.context_embeds), d, P(self.context_bias), self.dict_size,
                 P(b["ids"]), b["B"], d, self.neg_sample_size, self.lr, P(b["g_target"]), P(b["g_ctx"]), P(b["g_bias"]),
                 P(b["neg_slabs"]), P(b["bias_slabs"]), b["n_slabs"], P(b["loss_rows"]), P(b["rr_rows"]), P(self.loss_dev),
                 P(self.mrr_dev), P(self.clock_dev), 1, P(cursor), b["B"] if cursor is not None else 0, self.engine.stream)

    # ------------------------------------------------------------------------------------------------ host-fed steps
    def inject_negatives(self, neg):
        """Parity tests: the negatives of the next host-fed step (the reference draws them from TF's candidate sampler)."""
        self._injected_neg = None if neg is None else np.ascontiguousarray(neg, dtype=np.int32)

    def _check_ids(self, a, what):
        if a.size and (int(a.min()) < 0 or int(a.max()) >= self.dict_size):
            raise ValueError("Node2VecModel: %s holds ids outside [0, %d)" % (what, self.dict_size))

    def _stage_feed(self, feed_dict):
        e, ph = self.engine, self.placeholders
        b1 = np.ascontiguousarray(np.asarray(feed_dict[ph['batch1']]), dtype=np.int32)
        b2 = np.ascontiguousarray(np.asarray(feed_dict[ph['batch2']]), dtype=np.int32)
        B = int(b1.shape[0])
        assert B > 0 and b2.shape[0] == B and int(feed_dict.get(ph['batch_size'], B)) == B
        self._check_ids(b1, "batch1")
        self._check_ids(b2, "batch2")
        b = self._buffers(B, "h")
        e.sync()
        b["ids"][:B].copy_(torch.from_numpy(b1))
        b["ids"][B:2 * B].copy_(torch.from_numpy(b2))
        neg, self._injected_neg = self._injected_neg, None
        if neg is not None:
            assert neg.shape[0] == self.neg_sample_size and len(np.unique(neg)) == len(neg), "negatives must be distinct"
            self._check_ids(neg, "the injected negatives")
            b["ids"][2 * B:].copy_(torch.from_numpy(neg))
        torch.cuda.current_stream().synchronize()
        if neg is None:
            self._stage(b)
        return b

    def _fetch(self, b, with_outputs=True):
        self.engine.sync()
        if int(self._status.item()):
            raise ops._lib.GraphsageAmdError("Node2VecModel: the negative sampler gave up before it saw %d distinct nodes"
                                             % self.neg_sample_size)
        self.outputs1, self.aff_all = b["outputs1"], b["aff_all"]
        self.neg_samples = b["ids"][2 * b["B"]:]
        loss, mrr = float(self.loss_dev.item()), float(self.mrr_dev.item())
        aff = b["aff_all"].cpu().numpy()
        ranks = (aff[:, :-1] >= aff[:, -1:]).sum(axis=1)
        outs = b["outputs1"].cpu().numpy() if with_outputs else None
        return loss, ranks, aff, mrr, outs

    def train_step(self, feed_dict, fetch=True):
        """sess.run([opt_op, loss, ranks, aff_all, mrr, outputs1], feed_dict)  (unsupervised_train.py:273-274, :356-357)."""
        b = self._stage_feed(feed_dict)
        self._fwd_bwd(b, True)
        self._apply(b)
        return self._fetch(b) if fetch else None

    def eval_step(self, feed_dict):
        """sess.run([loss, ranks, mrr(, outputs1)], feed_dict): the evaluation form of the forward launch, no gradients
        and no update; new negatives every call (the sampler clock advances)."""
        b = self._stage_feed(feed_dict)
        self._fwd_bwd(b, False)
        inv = 1.0 / b["B"]
        ops.call("gs_finalize_step2", ops.ptr(b["loss_rows"]), b["B"], inv, ops.ptr(self.loss_dev), 0, ops.ptr(b["rr_rows"]), inv,
                 ops.ptr(self.mrr_dev), None, 0, ops.ptr(self.clock_dev), 1, None, 0, self.engine.stream)
        loss, ranks, aff, mrr, outs = self._fetch(b)
        return loss, ranks, mrr, outs

    # ---- device-resident epoch: the pairs live in HBM and are consumed through a device cursor; `steps_per_launch`
    #      steps are one captured graph.  Step t + 1 reads the rows step t wrote, so the steps of a graph are serial:
    #      nothing of the next step is prefetched here (unlike SampleAndAggregate's device epoch).
    def attach_device_pairs(self, pairs):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if len(pairs) == 0:
            raise ValueError("Node2VecModel: empty pair list")
        self._check_ids(pairs, "the pair list")
        self.engine.sync()
        self._pairs = torch.from_numpy(pairs).to(self.engine.device)
        self._cursor = torch.zeros(1, dtype=torch.int64, device=self.engine.device)
        self._graphs, self._warm = {}, set()          # captured graphs hold the old list's address
        torch.cuda.synchronize()

    def set_epoch_pairs(self, pairs):
        """A re-shuffled list of the same length, in place (captured graphs stay valid); the cursor returns to 0."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        assert pairs.shape == tuple(self._pairs.shape), "set_epoch_pairs: same length as the attached list"
        self._check_ids(pairs, "the pair list")
        self.engine.sync()
        self._pairs.copy_(torch.from_numpy(pairs))
        self._cursor.zero_()
        torch.cuda.synchronize()

    def _device_steps(self, b, k):
        for _ in range(k):
            self._stage(b, self._pairs, self._cursor)
            self._fwd_bwd(b, True)
            self._apply(b, self._cursor)

    def train_step_device(self, B, fetch=False):
        return self.train_steps_device(B, 1, steps_per_launch=1, fetch=fetch)

    def train_steps_device(self, B, steps, steps_per_launch=8, fetch=False):
        """`steps` steps on the attached pairs, `steps_per_launch` per graph launch (eager on first use of a length,
        captured on the second, replayed afterwards)."""
        assert self._pairs is not None, "attach_device_pairs first"
        b = self._buffers(B, "d")
        done = 0
        while done < steps:
            k = max(1, min(int(steps_per_launch), steps - done))
            _run_captured(self._graphs, self._warm, (int(B), k), lambda: self._device_steps(b, k), self.engine.stream,
                          lambda: self.use_graphs)
            done += k
        return self._fetch(b) if fetch else None

    def tables(self):
        """(target_embeds, context_embeds, context_bias) as NumPy arrays (synchronises)."""
        self.engine.sync()
        return self.target_embeds.cpu().numpy(), self.context_embeds.cpu().numpy(), self.context_bias.cpu().numpy()

    def assign_tables(self, target=None, context=None, bias=None):
        """Overwrite variables in place (tests load the reference's values)."""
        self.engine.sync()
        for t, a in ((self.target_embeds, target), (self.context_embeds, context), (self.context_bias, bias)):
            if a is not None:
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(tuple(t.shape))))
        torch.cuda.synchronize()
