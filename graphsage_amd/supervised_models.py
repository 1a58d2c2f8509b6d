"""SupervisedGraphsage on the gfx950 engine -- constructor/attribute surface of
graphsage/supervised_models.py:10-126.

    model = SupervisedGraphsage(num_classes, placeholders, features, adj_info, degrees, layer_infos,
                                concat=True, aggregator_type="mean", model_size="small",
                                sigmoid_loss=False, identity_dim=0)
    loss, preds = model.train_step(feed_dict)      # sess.run([opt_op, loss, preds], feed_dict)   (supervised_train.py:275)
    loss, preds = model.eval_step(feed_dict)       # sess.run([preds, loss], feed_dict)           (:76-77, :101-102)

`FLAGS.learning_rate` / `FLAGS.weight_decay` (read from module-level flags in the reference,
supervised_models.py:73,106-108) are explicit keyword arguments here.
"""
import numpy as np
import torch

from . import ops
from .layers import Dense, Rows, identity
from .models import SampleAndAggregate
from .ops import Mat


class SupervisedGraphsage(SampleAndAggregate):
    """Implementation of supervised GraphSAGE."""

    def __init__(self, num_classes, placeholders, features, adj, degrees, layer_infos, concat=True,
                 aggregator_type="mean", model_size="small", sigmoid_loss=False, identity_dim=0,
                 learning_rate=0.01, weight_decay=0.0, world_size=1, rank=0, **kwargs):
        super(SupervisedGraphsage, self).__init__(placeholders, features, adj, degrees, layer_infos, concat=concat,
                                                  aggregator_type=aggregator_type, model_size=model_size,
                                                  identity_dim=identity_dim, learning_rate=learning_rate,
                                                  weight_decay=weight_decay, world_size=world_size, rank=rank,
                                                  _defer_build=True, **kwargs)
        self.inputs1 = placeholders["batch"]
        self.num_classes = num_classes
        self.sigmoid_loss = sigmoid_loss
        self.label_table = None   # optional device-resident [N+1, C] label matrix (device fast path)
        self.build()

    _OUT_ATTRS = ("preds", "samples1", "outputs1", "node_preds", "agg_out", "_loss_rows", "_dlogits", "_loss_accumulate",
                  "_tail_sync", "_tail_sync_n",
                  "_head_fused", "_d_agg_out", "_tape", "_tail_used", "_tail_means", "_tail_dz", "_tail_dh0", "_tail_h0",
                  "_tail_step_advanced")

    # ------------------------------------------------------------------------------ build (:78-100)
    def _root_segments(self, n_roots):
        return None           # one sample() call per step (supervised_models.py:79)

    def build(self):
        e = self.engine
        self.num_samples = [layer_info.num_samples for layer_info in self.layer_infos]
        self.aggregators = self.make_aggregators(self.dims, self.num_samples, self.concat, self.model_size)
        dim_mult = 2 if self.concat else 1
        self.node_pred = Dense(dim_mult * self.dims[-1], self.num_classes, dropout=self.placeholders['dropout'],
                               act=identity)
        e.finalize()
        if self.embeds is not None:
            self._refresh_embeds()
        self.loss_dev = torch.zeros(1, dtype=torch.float32, device=e.device)

    # ------------------------------------------------------------------------------ one step
    def _fused_head_ok(self, d):
        C = self.num_classes
        return (getattr(self, "fuse_head", True) and self._dropout_rate() == 0 and d in (64, 128, 256, 512) and C <= 128
                and (d * (((C + 3) & ~3) | 1) + 4 + 4 * d) * 4 <= 160 * 1024)

    def _tail_ok(self):
        """The fused layer-1 + head launch (gs_sage_tail_fwd_bwd) applies to the supervised two-layer mean model with
        concat -- and, since round 5, to the two-layer GCN model (one weight matrix, the mean over {neighbors} U {self},
        aggregators.py:101-116) --, no dropout, no trainable identity features and shapes the kernel supports."""
        if not getattr(self, "fuse_tail", True) or len(self.layer_infos) != 2 or self.aggregator_type not in ("mean", "gcn"):
            return False
        a1 = self.aggregators[1]
        if a1.bias or self._dropout_rate() != 0 or self.embeds is not None or self.num_samples[-1] > 11:
            return False                                 # (s <= 11: the neighbor rows of a batch node are held in registers)
        if self.aggregator_type == "gcn":
            # layer-1 input = layer-0 output width (GCN ignores concat, the drivers pass 2 * dim: supervised_train.py:175-185)
            return self.dims[2] % 2 == 0 and ops.sage_tail_supported(self.dims[1], self.dims[2] // 2, self.num_classes)
        return self.concat and ops.sage_tail_supported(2 * self.dims[1], self.dims[2], self.num_classes)

    def _tail_weights(self):
        """(W_self, W_neigh, out_dim O, is_gcn) of the fused tail's layer-1 contraction z = [. W_self | . W_neigh] (z has 2 O
        columns): the mean aggregator's two matrices, or the two column halves of the GCN aggregator's one."""
        a1 = self.aggregators[1]
        if self.aggregator_type == "gcn":
            O = self.dims[2] // 2
            W = a1.vars['weights'].value
            return W.cols_slice(0, O), W.cols_slice(O, 2 * O), O, True
        return a1.vars['self_weights'].value, a1.vars['neigh_weights'].value, self.dims[2], False

    def _forward(self, batch, labels, n, train=False, prefetched=None, side_jobs=None, epilogue=None, tail_jobs=None):
        """sample -> aggregate -> l2_normalize -> node_pred -> loss/preds  (supervised_models.py:79-92,102-126).
        `epilogue`: the step's device-counter increments; when the fused tail launch runs it advances them itself
        (and `_backward` then skips the separate epilogue launch)."""
        e = self.engine
        del self.node_pred._saved[:]
        C = self.num_classes
        agg0 = self.aggregators[0]
        out, self._tail_used = self._forward_layers(batch, n, prefetched, lambda: train and self._tail_ok(),
                                                    self.aggregator_type == "mean", side_jobs)
        self._loss_rows = e.ws_f32("loss_rows", n)
        self.preds = e.ws_mat("preds", n, C)
        self._dlogits = e.ws_mat("dlogits", n, C)
        if self._tail_used:
            # layer 1 + l2_normalize + head + loss + every input gradient down to layer 0's pre-activations: ONE launch
            h0 = self._tape[0][4]                       # [n + n*s, 2*dim_1]: layer-0 outputs of both hops
            W_self1, W_neigh1, O1, gcn1 = self._tail_weights()
            Z = 2 * O1
            s = self.num_samples[len(self.num_samples) - 1]
            self._tail_means = e.ws_mat("tail_means", n, h0.d)
            means_ready = bool(getattr(agg0, "l1_means_written", False))
            self.last_tail_entry = "gs_sage_tail_fwd_bwd_means" if means_ready else "gs_sage_tail_fwd_bwd"
            self.agg_out = e.ws_mat("tail_z", n, Z)
            self.outputs1 = e.ws_mat("outputs1", n, Z)
            self.node_preds = e.ws_mat("node_preds", n, C)
            self._tail_dz = e.ws_mat("tail_dz", n, Z)
            self._tail_dh0 = e.ws_mat((self.name, "d_hidden", 0), h0.rows, h0.d)
            self._tail_h0 = h0
            self._head_fused = True
            counters = self._epilogue_counters(epilogue) if epilogue else []
            self._tail_step_advanced = bool(epilogue and epilogue.get("step"))
            # hand-over state of the launch's helper workgroups: private to this model (its engine stream)
            # (one buffer per batch size: its layout depends on n, and stale granules of another layout must never be met)
            self._tail_sync = e.ws_i32(("tail_sync", self.name, n, O1), ops.tail_sync_words(n, O1))
            self._tail_sync_n = n
            # split form: the z helpers as their own lean launch (its riders stream at the full HBM rate), then the
            # row-group workgroups; the tail's gather share is divided between the two launches
            jobs_z, jobs_m = [], tail_jobs
            if self.tail_split and tail_jobs:
                jobs_z, jobs_m = ops.split_gather_jobs(tail_jobs, self.cogather_tail_z)
            ids_copy = None
            agg0.wgrad_ids = None
            if getattr(e, "_sampler_to_wgrad", False) and self.aggregator_type == "mean" and agg0._saved \
                    and agg0._saved[-1].self_in is not None and agg0._saved[-1].self_in.ids is not None:
                src = agg0._saved[-1].self_in.ids                # the rows layer 0's self term gathered: [roots | hop-1 ids]
                dst = e.ws_i32(("wgrad_ids", self.name, n), src.numel())
                ids_copy = (src, dst, src.numel())
                agg0.wgrad_ids = dst[:src.numel()]
            ops.sage_tail_fwd_bwd(h0, n, s, W_self1, W_neigh1, O1,
                                  self.node_pred.vars['weights'].value, self.node_pred.vars['bias'].value.buf, labels, C,
                                  self.sigmoid_loss, self._tail_means, self.agg_out, self.outputs1, self.node_preds,
                                  self.preds, self._dlogits, self._loss_rows, dz=self._tail_dz, d_h0=self._tail_dh0,
                                  counters=counters, jobs=jobs_m, stream=e.stream, sync=self._tail_sync,
                                  split=self.tail_split, jobs_z=jobs_z, gcn=gcn1, ids_copy=ids_copy, means_ready=means_ready)
        else:
            self.agg_out = out
            self.outputs1 = e.ws_mat("outputs1", n, out.d)
            self._head_fused = self._fused_head_ok(out.d)
            if self._head_fused:
                # l2_normalize (:85) + Dense head (:88-92) + loss/preds (:111-126) + their gradients: ONE launch
                self.node_preds = e.ws_mat("node_preds", n, C)
                self._d_agg_out = e.ws_mat("d_agg_out", n, out.d) if train else None
                ops.head_fwd_bwd(out, n, self.node_pred.vars['weights'].value, self.node_pred.vars['bias'].value.buf, labels,
                                 C, self.sigmoid_loss, self.outputs1, self.node_preds, self.preds, self._dlogits,
                                 self._loss_rows, self._d_agg_out, stream=e.stream)
            else:
                self._inv_norm = e.ws_f32("inv_norm", n)
                ops.l2norm_fwd(out, n, self.outputs1, self._inv_norm, stream=e.stream)                      # :85
                self.node_preds = self.node_pred(Rows(self.outputs1, None, requires_grad=True))             # :88-92
                ops.class_loss(self.node_preds, labels, n, C, self.sigmoid_loss, self._loss_rows, self.preds,
                               self._dlogits, stream=e.stream)                                               # :111-126
        # loss = weight decay terms (:104-108) + mean classification loss (the mean is added by the step epilogue)
        self._weight_decay_loss([v for v in e.variables if v.decay], 0.5 * self.weight_decay)

    def _backward(self, n, fuse_adam, wgrad_jobs=None, epilogue=None):
        """Reverse of _forward.  Every weight gradient of the pass is ONE grouped launch; the slab reduction
        (+ weight decay, :104-108) and -- on a single GPU -- clip + Adam (:96-99) are ONE more launch."""
        e = self.engine
        e.begin_backward()
        if getattr(self, "_tail_used", False):
            # the fused tail launch already produced every input gradient; queue the weight gradients it feeds
            e.wgrad(self.node_pred.vars['weights'], self.outputs1, None, self._dlogits, 0, n)
            e.bgrad(self.node_pred.vars['bias'], self._dlogits, n, self.num_classes)
            self._queue_tail_wgrads(n, self._tail_dz)
            e.finish_backward(self.weight_decay, fuse_adam=fuse_adam, lr=self.learning_rate, clip=5.0, side_jobs=wgrad_jobs,
                              loss=(self._loss_rows, n, 1.0 / n, self.loss_dev, self._loss_accumulate) if epilogue is not None else None,
                              step_offset=0 if self._tail_step_advanced else 1)
            return
        if self._head_fused:
            e.wgrad(self.node_pred.vars['weights'], self.outputs1, None, self._dlogits, 0, n)
            e.bgrad(self.node_pred.vars['bias'], self._dlogits, n, self.num_classes)
            d_out = self._d_agg_out
        else:
            d_outputs1 = self.node_pred.backward(self._dlogits, need_input_grad=True)
            d_out = e.ws_mat("d_agg_out", n, self.agg_out.d)
            ops.l2norm_bwd(d_outputs1, self.outputs1, self._inv_norm, n, d_out, stream=e.stream)
        # The epilogue (loss mean + device counters) runs BEFORE the backward pass when there is no dropout (its masks are a
        # function of the device clock and the backward pass regenerates them): a later mini-batch's fan-out sampler can
        # then ride in this pass's optimizer launch -- it must see the advanced sampler clock and epoch cursor -- as it does
        # behind the fused tail launch.  (Folding the epilogue into the optimizer launch's last workgroup measured 9 us SLOWER.)
        early = epilogue is not None and self._dropout_rate() == 0
        if early:
            self._epilogue(n, **epilogue)
        self._early_epilogue = early
        advanced = early and bool(epilogue.get("step"))
        self.aggregate_backward(d_out)
        e.finish_backward(self.weight_decay, fuse_adam=fuse_adam, lr=self.learning_rate, clip=5.0, side_jobs=wgrad_jobs,
                          step_offset=0 if advanced else 1)
        if epilogue is not None and not early:
            self._epilogue(n, **epilogue)

    def _epilogue(self, n, **counters):
        self.engine.advance(loss_rows=self._loss_rows, n=n, loss_out=self.loss_dev, accumulate=self._loss_accumulate,
                            **counters)

    # ------------------------------------------------------------------------------ feeds
    def _stage_feed(self, feed_dict):
        """Copy the host feed (batch ids + label matrix) into persistent device buffers."""
        e = self.engine
        ph = self.placeholders
        # host-fed batches own their buffers (key "h"): a device-epoch batch prefetched into the parity-0/1 buffers
        # must survive an interleaved eval_step / train_step(feed) of the same size
        self._parity = "h"
        self._pending_stage = None
        e.sync()          # earlier steps still queued on the engine stream read these persistent buffers
        batch = np.ascontiguousarray(np.asarray(feed_dict[ph['batch']]), dtype=np.int32)
        n = int(batch.shape[0])
        bs = feed_dict.get(ph['batch_size'], n)
        assert int(bs) == n, "batch_size feed (%s) != len(batch) (%d)" % (bs, n)
        self._feed_dropout(feed_dict)
        batch_dev = self.ids_buffer(n)[0][:n]     # head of the contiguous id buffer (see models.sample)
        batch_dev.copy_(torch.from_numpy(batch))
        labels = np.ascontiguousarray(np.asarray(feed_dict[ph['labels']]), dtype=np.float32)
        labels_dev = e.ws_mat(("labels", "h"), n, self.num_classes)
        labels_dev.buf[:, : self.num_classes].copy_(torch.from_numpy(labels.reshape(n, self.num_classes)))
        torch.cuda.current_stream().synchronize()
        return batch_dev, labels_dev, n

    # ------------------------------------------------------------------------------ public steps
    def train_step(self, feed_dict, fetch=True):
        batch_dev, labels_dev, n = self._stage_feed(feed_dict)
        return self._train_on_device(batch_dev, labels_dev, n, fetch)

    def eval_step(self, feed_dict, fetch=True):
        batch_dev, labels_dev, n = self._stage_feed(feed_dict)
        e = self.engine
        self._run(("eval", n, self._adj_version()), lambda: (self._forward(batch_dev, labels_dev, n), self._epilogue(n, clock=1)))
        return self._fetch(n) if fetch else None

    def _train_on_device(self, batch_dev, labels_dev, n, fetch=True, prologue=None, cursor=None, key="train"):
        """One non-pipelined step on a staged batch; `cursor`: the epoch cursor the step epilogue advances by n."""
        def body(step, local_adam, tail):
            if prologue is not None:
                prologue()
            ep = dict(step=step, clock=1, cursor=cursor, cursor_delta=n if cursor is not None else 0)
            self._step_fwd_bwd(n, (batch_dev, labels_dev), None, self._NO_SHARES, ep, local_adam)
            tail()                # (_dispatch: a body calls tail() behind every step it issues)

        self._dispatch(key, (n,), body)
        return self._fetch(n) if fetch else None

    def _handover_error(self):
        err = ops.tail_sync_error(self._tail_sync, self._tail_sync_n) if getattr(self, "_tail_sync", None) is not None else 0
        return err, "fused tail launch", "row-group"

    def _fetch(self, n):
        self._sync_checked()
        loss = float(self.loss_dev.item())
        preds = self.preds.view()[:n].detach().cpu().numpy()
        return loss, preds

    # ------------------------------------------------------------------------------ device-resident epoch
    def attach_device_epoch(self, order, label_table):
        """Device fast path: epoch order + label table live in HBM; a step is one hipGraph replay with
        no host->device traffic.  `order`: int32 node ids (this rank's shard); `label_table`: [N+1, C]."""
        e = self.engine
        self._order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(e.device)
        self._cursor = torch.zeros(1, dtype=torch.int64, device=e.device)
        if not isinstance(label_table, Mat):
            label_table = Mat.from_numpy(np.asarray(label_table, dtype=np.float32), e.device)
        self.label_table = label_table
        self._primed = None
        torch.cuda.synchronize()

    def set_epoch_order(self, order):
        self._reset_epoch(self._order, np.ascontiguousarray(order, dtype=np.int32))

    def _drop_prefetched(self):
        """Forget the batch the pipeline has already staged (a different batch size follows, e.g. the short last batch
        of an epoch): hand its ids back to the epoch cursor and its tick back to the sampler clock, so the schedule
        draws exactly what the sequential one would."""
        if self._primed is not None:
            self.engine.sync()
            self._cursor -= int(self._primed)
            self.engine.sample_clock_dev -= 1
            self._primed = None
            torch.cuda.synchronize()

    # ---- the hooks of the step schedule (SampleAndAggregate, "the step schedule": the differences are listed there)
    _pipe_key = "ptrain"
    _dp_step_early = True

    def _pipelined(self):
        return getattr(self, "pipeline", True) and self._dropout_rate() == 0

    def _multi_step_ok(self):
        return self._pipelined() and super(SupervisedGraphsage, self)._multi_step_ok()

    def train_step_device(self, n, fetch=False):
        """One training step on the next n ids of the device-resident epoch order: pipelined (the shared schedule), or -- with
        `pipeline` off or dropout on -- the sequential form below (graph key "dtrain")."""
        if self._pipelined():
            return super(SupervisedGraphsage, self).train_step_device(n, fetch)
        # sequential form: batch selection + label gather ride along with the step's own fused sampler launch
        e = self.engine
        self._parity = 0
        batch_dev = self.ids_buffer(n)[0][:n]
        labels_dev = e.ws_mat(("labels", 0), n, self.num_classes)

        def stage():
            self._pending_stage = (self._order, self._cursor, self.label_table, labels_dev)

        return self._train_on_device(batch_dev, labels_dev, n, fetch, prologue=stage, cursor=self._cursor, key="dtrain")

    def _sample_roots(self, n, parity):
        batch = self.ids_buffer(n, parity=parity)[0][:n]
        labels = self.engine.ws_mat(("labels", parity), n, self.num_classes)
        samples, support = self._sample_phase(batch, n, parity, stage=(self._order, self._cursor, self.label_table, labels))
        return (batch, labels), n, samples, support

    def _gather_shares(self, jobs):
        if jobs and self.cogather_tail > 0 and self._tail_ok():
            # the fused tail launch keeps only n/16 CUs busy: the rest of the chip streams a share of the gather
            f_fwd, f_tail = self.rider_shares(jobs, self.dims[1] if self.aggregator_type == "gcn" else 2 * self.dims[1])
            fwd_jobs, rest = ops.split_gather_jobs(jobs, f_fwd)
            tail_jobs, wgrad_jobs = ops.split_gather_jobs(rest, min(1.0, f_tail / max(1e-6, 1.0 - f_fwd)))
            return fwd_jobs, tail_jobs, wgrad_jobs, []
        fwd_jobs, wgrad_jobs = ops.split_gather_jobs(jobs, self.cogather_split)
        return fwd_jobs, [], wgrad_jobs, []

    def _step_fwd_bwd(self, n, roots, prefetched, shares, epilogue, local_adam):
        batch, labels = roots
        fwd_jobs, tail_jobs, wgrad_jobs, _ = shares
        self._forward(batch, labels, n, train=True, prefetched=prefetched, side_jobs=fwd_jobs, epilogue=epilogue,
                      tail_jobs=tail_jobs)
        self._backward(n, fuse_adam=local_adam, wgrad_jobs=wgrad_jobs, epilogue=epilogue)

    def _sampler_to_wgrad_ok(self, jobs):
        e = self.engine
        return bool(self.sampler_in_wgrad and e._deferred_sampler is not None and self._tail_ok()
                    and sum(jb.n * jb.s * jb.d * 4 for jb in jobs) <= self.sampler_in_wgrad_max_bytes)

    def predict(self):
        """sigmoid / softmax of the logits (supervised_models.py:122-126); filled by the last step."""
        return self.preds

    def predict_full(self, graph, nodes=None):
        """(embeddings [n, d], preds [n, C]) (NumPy) of `nodes` (default: all N real nodes) from the exact layer-wise pass over
        `graph` (inference.FullGraph): l2_normalize, the prediction Dense and its softmax / sigmoid
        (supervised_models.py:85-93, :122-126)."""
        from . import inference as inf
        rows, n = inf.select_rows(self, inf.layers_full(self, graph), nodes)
        return self._head_rows(rows, n)

    def predict_nodes(self, graph, nodes):
        """(embeddings [n, d], preds [n, C], stats): predict_full(graph, nodes) computed from the receptive field of `nodes`
        alone (SampleAndAggregate.embed_nodes): rows in REQUEST order, a duplicate request answered twice."""
        from . import inference as inf
        H, S, _, stats = inf.layers_nodes(self, graph, nodes)
        rows, n = inf.request_rows(self, H, S, nodes)
        return self._head_rows(rows, n) + (stats,)

    def correct_and_smooth(self, graph, labels, known, nodes=None, **kw):
        """propagation.correct_and_smooth over `graph` from this model's exact predictions predict_full(graph) of every node, the
        `labels` ([N, C]) and the rows `known`; kw: correct_alpha, smooth_alpha, iters.  nodes: the rows of "preds" and
        "corrected" to return (default: all N, in id order)."""
        from . import propagation
        ids = None if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1)
        if ids is not None and ids.size and (ids.min() < 0 or ids.max() >= graph.n_nodes):
            raise ops._lib.GraphsageAmdError("correct_and_smooth: node ids must lie in [0, %d)" % graph.n_nodes)
        _, preds = self.predict_full(graph)
        res = propagation.correct_and_smooth(self.engine, graph, preds, labels, known, **kw)
        if ids is not None:
            res["preds"], res["corrected"] = res["preds"][ids], res["corrected"][ids]
        return res

    def _head_rows(self, rows, n):
        """l2_normalize, the prediction Dense and its softmax / sigmoid over the first n rows of `rows`."""
        from . import inference as inf
        e = self.engine
        C = self.num_classes
        preds = inf._table(e, max(n, 1), C)
        y = inf.l2_rows(e, rows, n)
        w = min(inf.WINDOW_ROWS, max(n, 1))
        logits = e.ws_mat((self.name, "full_logits"), w, C)
        no_labels = e.ws_mat((self.name, "full_no_labels"), w, C)          # gs_class_loss also forms the loss: unused here
        loss_rows = e.ws_f32((self.name, "full_loss_rows"), w)
        for r0 in range(0, n, w):
            m = min(w, n - r0)
            ops.gemm(False, False, m, C, y.d, y.rows_slice(r0, r0 + m), self.node_pred.vars['weights'].value, logits,
                     bias=self.node_pred.vars['bias'].value.buf, stream=e.stream)
            ops.class_loss(logits, no_labels, m, C, self.sigmoid_loss, loss_rows, preds=preds.rows_slice(r0, r0 + m),
                           stream=e.stream)
        e.sync()
        return y.numpy()[:n], preds.numpy()[:n]
