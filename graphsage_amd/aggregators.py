"""Mean / GCN / MaxPooling / MeanPooling / Seq (LSTM) aggregators with the constructor and call signatures of
graphsage/aggregators.py, executing on the gfx950 kernels; AttentionPoolingAggregator, which the reference does not have, shares them.

    agg = MeanAggregator(input_dim, output_dim, act=..., dropout=..., name=..., concat=..., model_size=...)
    out = agg((self_vecs, neigh_vecs))        # models.py:326-327

`self_vecs` is a `Rows` [n, d]; `neigh_vecs` is a `Rows` reshaped to [n, s, d] (both may be lazy row gathers of
the feature table, so the [n*s, d] tensor of models.py:299 is never materialised).  `.vars` holds exactly the
variables the reference's weight-decay loop sees (supervised_models.py:104-106).

MI355X-first addition: the reference calls the SAME aggregator once per hop of a layer (models.py:321-328);
`call_hops(self_all, [neigh_0, neigh_1, ...])` runs all hops of a layer in one dense launch (the rows of all
hops are contiguous), and `backward_hops` is its hand-written reverse.  `_call` is `call_hops` with one hop.
"""
import os
from collections import namedtuple

import torch

from . import ops
from .engine import MAX_SLABS
from .inits import glorot, zeros
from .layers import SITE_MLP, SITE_NEIGH, SITE_SELF, Dense, Layer, Rows, _act_code, _rate, relu
from .ops import ACT_IDENTITY, ACT_RELU, Mat

# What one call_hops leaves for its backward_hops, one record type per aggregator family.
_MeanSaved = namedtuple("_MeanSaved", "self_all neighs means out rate self_in h0", defaults=(None, None))   # Mean and GCN
_PoolSaved = namedtuple("_PoolSaved", "self_all neighs pieces rows_total H pooled argmax out rate")
_Pool2Saved = namedtuple("_Pool2Saved", "self_all neighs pieces rows_total H1 inv pooled argmax out")
_AttnSaved = namedtuple("_AttnSaved", "self_all neighs pieces rows_total H inv alpha pooled out rate")
_SeqSaved = namedtuple("_SeqSaved", "self_all neighs pieces rows_total segs lengths gates C Hp h_last out")


def _scope(self_name, name):
    # variable scope naming of aggregators.py:24-29
    return self_name + ('/' + name if name is not None else '') + '_vars'


def contiguous_rows(rows_list):
    """If the Rows views are adjacent slices of one buffer, return the single Rows covering all of them."""
    first = rows_list[0]
    total = first.n
    for prev, cur in zip(rows_list[:-1], rows_list[1:]):
        if (prev.ids is None) != (cur.ids is None):
            return None
        if cur.ids is not None:
            if cur.src is not prev.src or cur.ids.data_ptr() != prev.ids.data_ptr() + 4 * prev.n:
                return None
        else:
            if cur.src.ld != prev.src.ld or cur.src.d != prev.src.d or \
                    cur.src.buf.data_ptr() != prev.src.buf.data_ptr() + 4 * prev.n * prev.src.ld:
                return None
        total += cur.n
    if len(rows_list) == 1:
        return Rows(first.src, first.ids, first.n, first.requires_grad)
    if first.ids is not None:
        ids = torch.as_strided(first.ids, (total,), (1,))
        return Rows(first.src, ids, total, first.requires_grad)
    buf = torch.as_strided(first.src.buf, (total, first.src.buf.shape[1]), first.src.buf.stride())
    return Rows(Mat(buf, first.src.d), None, total, first.requires_grad)


def _hops(neighs):
    """(h, nv, n, s, r, hr) per hop: r is the offset of the hop's n group rows among all hops', hr that of its n * s
    sampled rows."""
    r = hr = 0
    for h, nv in enumerate(neighs):
        n, s, _ = nv.shape3
        yield h, nv, n, s, r, hr
        r += n
        hr += n * s


def _flatten(neighs):
    """Every hop's neighbors as [n * s, d] rows: (flat, x_all, pieces, rows_total).  x_all is the one view over all hops when
    they are adjacent (else None); pieces is what a contraction over every neighbor row runs on, [x_all] or flat."""
    flat = [Rows(nv.src, nv.ids, nv.shape3[0] * nv.shape3[1], nv.requires_grad) for nv in neighs]
    x_all = contiguous_rows(flat)
    return flat, x_all, ([x_all] if x_all is not None else flat), sum(x.n for x in flat)


def _run_jobs(e, jobs):
    """Issue gather+mean job descriptors as standalone launches (aggregators without a fused variant)."""
    for j in jobs or ():
        ops.call("gs_gather_mean_fwd", j.X, j.ldx, j.idx, j.n, j.s, j.d, j.self_src, j.ld_self, j.self_idx, j.out, j.ldo,
                 e.stream)


def _pieces_fwd(e, pieces, W, bias, width, act, out):
    """out = act(X . W + bias) over every neighbor row, one contraction per contiguous piece of the rows (_flatten)."""
    r = 0
    for x in pieces:
        ops.sage_dense_fwd(None, None, x.src, x.ids, x.n, None, W, width, False, act, bias, out.rows_slice(r, r + x.n),
                           stream=e.stream)
        r += x.n


def _pieces_wgrad(e, var, pieces, d_rows):
    """Queue the weight gradient of _pieces_fwd's W from d_rows, one operand per piece."""
    r = 0
    for x in pieces:
        e.wgrad(var, x.src, x.ids, d_rows.rows_slice(r, r + x.n), 0, x.n)
        r += x.n


class _SageBase(Layer):
    """Shared plumbing: construction, saved-activation stack, the SAGE output layer and its backward, masked scatter of
    input gradients."""

    # Switches (set on an instance by models, tests and A/B scripts) and records of what the last call took (read by tests and
    # bench.py) are class attributes of the class whose code reads or writes them, each declared once with its default.

    def _init_sage(self, input_dim, output_dim, neigh_input_dim, dropout, bias, act, concat, name, neigh_rows, bias_cols,
                   self_weights=True):
        """The attributes every aggregator has and the SAGE variables, in the reference's creation order: neighbor weights
        [neigh_rows, output_dim], self weights [input_dim, output_dim] (GCN has none), bias [bias_cols]."""
        self.dropout = dropout
        self.bias = bias
        self.act = act
        self.act_code = _act_code(act)
        self.concat = concat
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.neigh_input_dim = neigh_input_dim
        scope = _scope(self.name, name)
        e = self.engine
        self.vars['neigh_weights'] = e.add_variable(scope + '/neigh_weights', glorot((neigh_rows, output_dim)), decay=True)
        if self_weights:
            self.vars['self_weights'] = e.add_variable(scope + '/self_weights', glorot((input_dim, output_dim)), decay=True)
        if self.bias:
            self.vars['bias'] = e.add_variable(scope + '/bias', zeros((bias_cols,)), decay=True)
        self._saved = []

    def _push(self, rec):
        self._saved.append(rec)

    def _dz(self, d_out, out, n, n_cols, pre_masked):
        e = self.engine
        if self.act_code == ACT_RELU and not pre_masked:
            dz = e.ws_mat((self.name, "dz", len(self._saved)), n, n_cols)
            ops.act_bwd(d_out, out, n, n_cols, ACT_RELU, dz, stream=e.stream)
            return dz
        return d_out

    def reset(self):
        del self._saved[:]

    def prefetch(self, self_all, neighs, tag=0):
        return None   # the neighborhood vector needs the weights (pooling MLP, recurrence): nothing can run ahead

    def prefetch_jobs(self, self_all, neighs, tag=0):
        return None, []

    def _mean_jobs(self, self_all, neighs, tag, self_term):
        """prefetch() of the mean aggregators, but only DESCRIBED: the gather+mean launches (one per hop) as jobs that can be
        issued inside another kernel's launch (horizontal fusion).  self_term: the GCN mean over {neighbors} U {self}.
        Returns (means, jobs)."""
        self._no_dropout_here("the prefetch pipeline")
        e = self.engine
        means = e.ws_mat((self.name, "mean", len(self._saved), tag), self_all.n, neighs[0].shape3[2], ld_multiple=32)
        jobs = []
        for h, nv, n, s, r, hr in _hops(neighs):
            sv = self_all.slice(r, r + n) if self_term else None
            jobs.append(ops.gather_job(nv.src, nv.ids, n, s, means.rows_slice(r, r + n),
                                       self_src=sv.src if self_term else None, self_idx=sv.ids if self_term else None))
        return means, jobs

    # ---- dropout (tf.nn.dropout on the aggregator inputs, aggregators.py:46-47,104-105; layers.py:107) ----
    def _drop(self, rate, role, k, row0=0):
        return self.engine.dropout(rate, self.site + role + 4 * k, row0)

    def _no_dropout_here(self, what):
        if _rate(self.dropout) > 0:
            raise NotImplementedError("dropout > 0 with %s: use the sequential schedule (model.pipeline = False)" % what)

    def _drop_self(self, self_all, rate, k):
        """dropout(self_vecs), materialised once ([n_total, d]; small) so that the GEMMs read it as a dense operand."""
        e = self.engine
        sd = e.ws_mat((self.name, "self_drop", k), self_all.n, self_all.src.d)
        ops.dropout_rows(self_all.src, self_all.ids, self_all.n, self._drop(rate, SITE_SELF, k), sd, stream=e.stream)
        return Rows(sd, None, self_all.n, self_all.requires_grad)

    def _sink(self, var, d_rows, ids, n, s, scale, rate, role, k, row0, tag):
        """Scatter scale * d_rows[i] to the s sampled ids of row i of a trainable table (identity features); with
        dropout the per-sampled-row mask is applied first (the table rows went through `dropout` before the mean)."""
        e = self.engine
        if rate == 0 or role is None:
            e.scatter_grad(var, d_rows, ids, n, s, scale)
            return
        tmp = e.ws_mat((self.name, "d_sink", k, tag), n * s, var.cols)
        ops.mean_bwd(d_rows, n, s, scale, tmp, stream=e.stream)
        ops.dropout_rows(tmp, None, n * s, self._drop(rate, role, k, row0), tmp, stream=e.stream)
        e.scatter_grad(var, tmp, ids, n * s, 1, 1.0)

    def _bwd_dropped(self, d_rows, n, s, scale, rate, role, k, row0, dst, relu_mask, accumulate, tag):
        """dst (+)= relu'(relu_mask) * dropout_mask * broadcast_s(scale * d_rows): the reverse of `dropout` followed by
        a (segmented) mean, with the mask regenerated from the counter hash."""
        e = self.engine
        tmp = e.ws_mat((self.name, "d_bcast", k, tag), n * s, d_rows.d)
        ops.mean_bwd(d_rows, n, s, scale, tmp, stream=e.stream)
        ops.dropout_rows(tmp, None, n * s, self._drop(rate, role, k, row0), tmp, stream=e.stream)
        ops.mean_bwd(tmp, n * s, 1, 1.0, dst, mask_y=relu_mask, accumulate=accumulate, stream=e.stream)

    def _call(self, inputs):
        self_vecs, neigh_vecs = inputs
        return self.call_hops(self_vecs, [neigh_vecs])

    def backward(self, d_out, pre_masked=False):
        """Single-hop reverse of `_call`: returns raw (d_self [n, d], d_neigh [n*s, d]) when the inputs
        require gradients, else (None, None)."""
        self_all, neighs = self._saved[-1].self_all, self._saved[-1].neighs
        need = self_all.requires_grad or neighs[0].requires_grad
        if not need:
            self.backward_hops(d_out, pre_masked)
            return None, None
        n, s, d = neighs[0].shape3
        d_prev = self.engine.ws_mat((self.name, "d_prev1"), n + n * s, self.input_dim)
        self.backward_hops(d_out, pre_masked, d_prev=d_prev, prev_mask=None, prev_offsets=[0, n, n + n * s])
        return d_prev.rows_slice(0, n), d_prev.rows_slice(n, n + n * s)

    def _scatter_self(self, d_self_all, n_total, d_prev, prev_mask):
        """d_prev[0:n_total] = mask * d_self_all  (self rows of hop h are rows h of the previous layer)."""
        e = self.engine
        act = ACT_RELU if prev_mask is not None else ACT_IDENTITY
        ops.act_bwd(d_self_all, prev_mask.rows_slice(0, n_total) if prev_mask is not None else None, n_total,
                    d_self_all.d, act, d_prev.rows_slice(0, n_total), stream=e.stream)

    def _sage_out(self, self_all, pooled, n_total, k):
        """from_self / from_neighs matmuls + concat|add + bias + act over the pooled neighborhood vectors (all hops, one launch)."""
        e = self.engine
        n_out = self.output_dim * (2 if self.concat else 1)
        out = e.ws_mat((self.name, "out", k), n_total, n_out)
        b = self.vars['bias'].value.buf if self.bias else None
        if e.stream_gemm and self.concat and n_total > 2048 and self.output_dim % 2 == 0:
            # the stream form of the two contractions (split-K workgroups, no LDS staging, the self rows gathered in the A loads),
            # with each term's own reduction length: 23 instead of 33 us for the Reddit step's layer 0
            (ops.sage_dense_fwd_tiled3 if (e.tiled3_fwd and self.output_dim % 4 == 0) else ops.sage_dense_fwd_stream2)(
                self_all.src, self_all.ids, pooled, n_total, self.vars['self_weights'].value, self.vars['neigh_weights'].value,
                self.output_dim, self.act_code, b, out, stream=e.stream)
        else:
            ops.sage_dense_fwd(self_all.src, self_all.ids, pooled, None, n_total, self.vars['self_weights'].value,
                               self.vars['neigh_weights'].value, self.output_dim, self.concat, self.act_code, b, out,
                               stream=e.stream)
        return out

    def _sage_bwd(self, d_out, out, n_total, pre_masked, self_src, self_ids, neigh_vecs):
        """Reverse of the SAGE output layer up to its weights: dz = act'(out) * d_out, then the self-weight, neighbor-weight and
        bias gradients QUEUED in that order (the slab order inside the grouped weight-gradient launch follows it).  The self
        operand is rows `self_ids` of `self_src`, the neighbor operand the dense `neigh_vecs`.  Returns (dz, col_n), col_n the
        first column of dz that belongs to the neighbor term."""
        e = self.engine
        o = self.output_dim
        n_out = o * (2 if self.concat else 1)
        dz = self._dz(d_out, out, n_total, n_out, pre_masked)
        col_n = o if self.concat else 0
        e.wgrad(self.vars['self_weights'], self_src, self_ids, dz, 0, n_total)
        e.wgrad(self.vars['neigh_weights'], neigh_vecs, None, dz, col_n, n_total)
        if self.bias:
            e.bgrad(self.vars['bias'], dz, n_total, n_out)
        return dz, col_n

    def _row_input_grads(self, saved, k, dz, d_rows, width, W1, embed_sink, d_prev, prev_mask, prev_offsets, drop=None):
        """Input gradients of an aggregator whose every neighbor row went through a first layer `W1` [neigh_in, width] of its
        own, so that each has its own gradient row in d_rows [rows_total, width]; the self rows only through W_self.  `drop`
        makes the dropout descriptor of those neighbor rows (None: they were not dropped; these aggregators never drop self).
        With embed_sink the leading columns go to the identity-feature table; with d_prev everything, in ONE pull launch."""
        e = self.engine
        self_all, neighs, rows_total = saved.self_all, saved.neighs, saved.rows_total
        n_total, o = self_all.n, self.output_dim
        W_self = self.vars['self_weights'].value
        if embed_sink is not None:
            var, c = embed_sink                    # see MeanAggregator.backward_hops
            d_self_e = e.ws_mat((self.name, "d_self_e", k), n_total, c)
            ops.dense_dgrad(dz, 0, o, n_total, W_self.rows_slice(0, c), d_self_e, stream=e.stream)
            e.scatter_grad(var, d_self_e, self_all.ids, n_total, 1, 1.0)
            d_neigh_e = e.ws_mat((self.name, "d_neigh_e", k), rows_total, c)
            ops.dense_dgrad(d_rows, 0, width, rows_total, W1.rows_slice(0, c), d_neigh_e, stream=e.stream)
            if drop is not None:
                ops.dropout_rows(d_neigh_e, None, rows_total, drop(), d_neigh_e, stream=e.stream)
            for h, nv, n, s, r, hr in _hops(neighs):
                e.scatter_grad(var, d_neigh_e.rows_slice(hr, hr + n * s), nv.ids, n * s, 1, 1.0)
        if d_prev is None:
            return
        d_self_all = e.ws_mat((self.name, "d_self", k), n_total, self.input_dim)
        ops.dense_dgrad(dz, 0, o, n_total, W_self, d_self_all, stream=e.stream)
        d_neigh = e.ws_mat((self.name, "d_neigh", k), rows_total, self.neigh_input_dim)
        ops.dense_dgrad(d_rows, 0, width, rows_total, W1, d_neigh, stream=e.stream)
        if drop is not None:
            ops.dropout_rows(d_neigh, None, rows_total, drop(), d_neigh, stream=e.stream)
        # every neighbor row has its own gradient row (s = 1)
        segs = [(d_neigh.rows_slice(hr, hr + n * s), prev_offsets[h + 1], n * s, 1, 1.0) for h, nv, n, s, r, hr in _hops(neighs)]
        ops.input_grad_pull(d_prev, d_prev.rows, d_prev.d, d_self=d_self_all, n_self=n_total, segments=segs,
                            mask_y=prev_mask, stream=e.stream)

    # ---- exact full-neighborhood inference (inference.py): ONE recipe per aggregator, written on a scope's primitives ----
    def infer(self, scope, H):
        """The layer for the rows `scope` computes, every row from ALL its neighbors, no dropout: H is the table of the layer
        below, the result a table over the computed rows.  scope: inference.GraphLayer (every row of the graph, the pad row
        computed like any other, in row windows) or inference.RowsLayer (a row subset, compact tables)."""
        raise NotImplementedError

    def infer_full(self, graph, H):
        """infer for EVERY row of `graph` (inference.FullGraph): H [N + 1, d_in] -> [N + 1, n_out], once the stream has drained."""
        from . import inference as inf
        return self._drained(self.infer(inf.GraphLayer(graph), H))

    def infer_rows(self, L, H):
        """infer for the rows of L (inference.RowsLayer) only, into a compact [L.n, n_out] table: H is the feature table by node
        id, or the compact table over the rows this layer may read."""
        return self._drained(self.infer(L, H))

    def _drained(self, out):
        self.engine.sync()
        return out

    def _infer_sage(self, scope, csr_op, X, of_src, H):
        """Tail of the wide forms: X reduced over the whole neighbor lists, then the SAGE matmuls over [self rows of H | reduced]."""
        return scope.reduce_sage(self, csr_op, X, of_src, H, self.vars['self_weights'].value, self.vars['neigh_weights'].value,
                                 self.output_dim, self.concat, self.act_code, self.vars['bias'].value.buf if self.bias else None)


class MeanAggregator(_SageBase):
    """Aggregates via mean followed by matmul and non-linearity (aggregators.py:6-64)."""
    layer1_z = True            # switch: the last layer as ONE gs_sage_tail_z launch where _last_layer_z allows it
    wgrad_ids = None           # the step's private copy of the self ids for the next weight gradient (set by the model)
    last_fused_launch = None   # record: (re-issuable launch, description) of the last horizontally fused forward
    l1_means_out = None        # set by the model before a layer-0 call: the fused tail's `means` workspace [n_roots, 2 output_dim]
    l1_means_written = False   # ... and whether that call's launch wrote it (the tail then takes its *_means entry)
    last_fwd_entry = None      # record: library entry point of the last all-hops forward launch (tests)

    def __init__(self, input_dim, output_dim, neigh_input_dim=None, dropout=0., bias=False, act=relu,
                 name=None, concat=False, **kwargs):
        super(MeanAggregator, self).__init__(**kwargs)
        if neigh_input_dim is None:
            neigh_input_dim = input_dim
        self._init_sage(input_dim, output_dim, neigh_input_dim, dropout, bias, act, concat, name,
                        neigh_rows=neigh_input_dim, bias_cols=(2 if concat else 1) * output_dim)

    def prefetch(self, self_all, neighs, tag=0):
        """The weight-free half of the call: reduce_mean(neigh_vecs, axis=1) (aggregators.py:48) fused with the row
        gather, one launch per hop.  Because it needs no weights it can run ahead of time (next step's data chain)."""
        e = self.engine
        n_total = self_all.n
        d = neighs[0].shape3[2]
        k = len(self._saved)
        rate = _rate(self.dropout)
        means = e.ws_mat((self.name, "mean", k, tag), n_total, d, ld_multiple=32)      # whole 128-byte lines per row
        for h, nv, n, s, r, hr in _hops(neighs):
            ops.gather_mean_fwd(nv.src, nv.ids, n, s, out=means.rows_slice(r, r + n),
                                drop=self._drop(rate, SITE_NEIGH, k, hr), stream=e.stream)     # dropout(neigh_vecs) (:46)
        assert sum(nv.shape3[0] for nv in neighs) == n_total
        return means

    def prefetch_jobs(self, self_all, neighs, tag=0):
        return self._mean_jobs(self_all, neighs, tag, self_term=False)

    def _last_layer_z(self, self_all, neighs, rate, means):
        """Can this call be ONE gs_sage_tail_z launch?  A last layer (identity act, concat, no bias, no dropout) over ONE hop
        whose inputs are the dense rows [self (n) | neighbors (n s)] of one buffer -- the layer-1 call of every two-layer
        mean model (models.py:321-328).  Returns that buffer as a Mat, or None."""
        if (means is not None or rate > 0 or len(neighs) != 1 or not self.concat or self.bias or self.act_code != ACT_IDENTITY
                or self_all.ids is not None or neighs[0].ids is not None or not self.layer1_z):
            return None
        n, s, d = neighs[0].shape3
        a, b = self_all.src, neighs[0].src
        if (n != self_all.n or s > 11 or a.ld != b.ld or a.d != d or b.d != d or (n + n * s) * a.ld >= (1 << 31)
                or b.buf.data_ptr() != a.buf.data_ptr() + 4 * n * a.ld or not ops.sage_tail_supported(d, self.output_dim, 1)):
            return None
        return Mat(torch.as_strided(a.buf, (n + n * s, a.buf.shape[1]), a.buf.stride()), d)

    def call_hops(self, self_all, neighs, means=None, side_jobs=None):
        e = self.engine
        n_total = self_all.n
        k = len(self._saved)
        rate = _rate(self.dropout)
        l1_means, self.l1_means_out, self.l1_means_written = self.l1_means_out, None, False
        h0 = self._last_layer_z(self_all, neighs, rate, means)
        if h0 is not None:
            # reduce_mean + both matmuls + concat (aggregators.py:48-58) of the last layer: ONE lean launch instead of a
            # gather-mean launch and a small GEMM (13 -> 8 us at 1044 rows), and one in which gather jobs ride at the full rate
            s = neighs[0].shape3[1]
            means = e.ws_mat((self.name, "mean", k, 0), n_total, h0.d, ld_multiple=32)
            out = e.ws_mat((self.name, "out", k), n_total, 2 * self.output_dim)
            ops.sage_tail_z(h0, n_total, s, self.vars['self_weights'].value, self.vars['neigh_weights'].value, self.output_dim,
                            means, out, jobs=side_jobs, stream=e.stream)
            self._push(_MeanSaved(self_all, neighs, means, out, rate, self_all, h0))
            return out
        if means is None:
            means = self.prefetch(self_all, neighs)
        self_in = self._drop_self(self_all, rate, k) if rate > 0 else self_all           # dropout(self_vecs) (:47)
        # from_neighs / from_self matmuls + concat|add + bias + act   (:51-64): ONE launch for all hops
        n_out = self.output_dim * (2 if self.concat else 1)
        out = e.ws_mat((self.name, "out", k), n_total, n_out)
        b = self.vars['bias'].value.buf if self.bias else None
        stream_fwd = e.stream_gemm and self.concat and rate == 0 and n_total > 2048 and self.output_dim % 2 == 0
        if side_jobs or stream_fwd:
            # horizontally fused launch: the contraction workgroups + the NEXT step's gather-mean waves share the CUs.
            # Stream form (gs_stream.hip): split-K workgroups without LDS staging, the self rows gathered in the A loads.
            tiled3 = stream_fwd and e.tiled3_fwd and self.output_dim % 4 == 0
            # the rows are [roots | hop 1 (s consecutive rows per root)]: the launch can form the next layer's neighbor means
            n_roots = neighs[0].shape3[0]
            s1 = neighs[1].shape3[0] // max(n_roots, 1) if len(neighs) == 2 else 0
            with_means = (tiled3 and l1_means is not None and 1 <= s1 <= 64 and n_total == n_roots * (1 + s1)
                          and l1_means.rows >= n_roots and l1_means.d == n_out)
            self.l1_means_written = with_means
            self.last_fwd_entry = ("gs_sage_dense_fwd_tiled3_means" if with_means else "gs_sage_dense_fwd_tiled3" if tiled3 else
                                   "gs_sage_dense_fwd_stream" if stream_fwd else "gs_sage_dense_fwd_cogather")

            def launch(jobs=list(side_jobs or ())):
                if with_means:
                    ops.sage_dense_fwd_tiled3_means(self_all.src, self_all.ids, means, n_total, self.vars['self_weights'].value,
                                                    self.vars['neigh_weights'].value, self.output_dim, self.act_code, b, out,
                                                    n_roots, s1, l1_means, jobs, stream=e.stream)
                elif tiled3:
                    # LDS-tiled, on the bf16 matrix pipe in the three-piece arithmetic (fp32 in and out, cut inside the kernel)
                    ops.sage_dense_fwd_tiled3(self_all.src, self_all.ids, means, n_total, self.vars['self_weights'].value,
                                              self.vars['neigh_weights'].value, self.output_dim, self.act_code, b, out, jobs,
                                              stream=e.stream)
                elif stream_fwd:
                    ops.sage_dense_fwd_stream(self_all.src, self_all.ids, means, n_total, self.vars['self_weights'].value,
                                              self.vars['neigh_weights'].value, self.output_dim, self.act_code, b, out, jobs,
                                              stream=e.stream)
                else:
                    ops.sage_dense_fwd_cogather(self_all.src, self_all.ids, means, None, n_total,
                                                self.vars['self_weights'].value, self.vars['neigh_weights'].value,
                                                self.output_dim, self.concat, self.act_code, b, out, jobs, stream=e.stream)
            launch()
            # bench.py re-issues exactly this launch between HIP events (roofline of the step's dominant kernel)
            d_in = self_all.src.d
            jobs_ = list(side_jobs or ())
            self.last_fused_launch = (launch, {
                "kernel": "%s: [%d x %d|%d] . [%d x %d] x2 (%s) + %d co-scheduled "
                          "gather+mean jobs of the next step" % ("sage_tiled3_fwd_kernel" if tiled3 else
                                                                 "sage_stream_fwd_kernel" if stream_fwd else "sage_dense_cogather_kernel",
                                                                 n_total, d_in, means.d, d_in, self.output_dim,
                                                                 "fp32 as 3 bf16 pieces, 6 bf16 MFMAs per product" if tiled3 else "fp32 MFMA",
                                                                 len(jobs_)),
                "gather_bytes": sum(j.n * j.s * j.d * 4 + j.n * j.s * 4 + j.n * j.d * 4 for j in jobs_),
                "gemm_bytes": n_total * (d_in + means.d) * 4 + (d_in + means.d) * self.output_dim * 4 + n_total * n_out * 4,
                "flops": 2.0 * n_total * (d_in + means.d) * self.output_dim,
                "piece_products": 6 if tiled3 else 1,       # MFMAs issued per fp32 product tile (bf16 pipe) | fp32 pipe
                "gather_share": sum(j.n * j.s for j in jobs_) / float(max(1, sum(nv.shape3[0] * nv.shape3[1] for nv in neighs)))})
        else:
            ops.sage_dense_fwd(self_in.src, self_in.ids, means, None, n_total, self.vars['self_weights'].value,
                               self.vars['neigh_weights'].value, self.output_dim, self.concat, self.act_code, b, out,
                               stream=e.stream)
        self._push(_MeanSaved(self_all, neighs, means, out, rate, self_in, None))
        return out

    def backward_hops(self, d_out, pre_masked=False, d_prev=None, prev_mask=None, prev_offsets=None, embed_sink=None):
        e = self.engine
        self_all, neighs, means, out, rate, self_in, h0 = self._saved.pop()
        n_total = self_all.n
        k = len(self._saved)
        o = self.output_dim
        # (wgrad_ids: the step's private copy of these ids, made by the fused tail launch when a later step's sampler rides in
        #  the weight-gradient launch and refills the id buffer meanwhile -- SupervisedGraphsage._forward)
        wg_ids = self.wgrad_ids
        self.wgrad_ids = None
        dz, col_n = self._sage_bwd(d_out, out, n_total, pre_masked, self_in.src,
                                   wg_ids if (wg_ids is not None and self_in.ids is not None) else self_in.ids, means)
        if embed_sink is not None:
            # layer 0 over a table whose leading c columns are trainable (identity features): only those columns of
            # the input gradients are formed ([n, c] = dz . W[:c]^T) and scattered per sampled id, 1/s per neighbor
            var, c = embed_sink
            d_self_e = e.ws_mat((self.name, "d_self_e", k), n_total, c)
            ops.dense_dgrad(dz, 0, o, n_total, self.vars['self_weights'].value.rows_slice(0, c), d_self_e, stream=e.stream)
            d_means_e = e.ws_mat((self.name, "d_means_e", k), n_total, c)
            ops.dense_dgrad(dz, col_n, o, n_total, self.vars['neigh_weights'].value.rows_slice(0, c), d_means_e,
                            stream=e.stream)
            self._sink(var, d_self_e, self_all.ids, n_total, 1, 1.0, rate, SITE_SELF, k, 0, "s")
            for h, nv, n, s, r, hr in _hops(neighs):
                self._sink(var, d_means_e.rows_slice(r, r + n), nv.ids, n, s, 1.0 / s, rate, SITE_NEIGH, k, hr, ("n", h))
        if d_prev is None:
            return
        d_in = self.input_dim
        if (h0 is not None and rate == 0 and embed_sink is None and prev_mask is not None and prev_mask.ptr == h0.ptr
                and prev_mask.ld == h0.ld and d_prev.rows == h0.rows and d_prev.d == h0.d
                and list(prev_offsets[:3]) == [0, n_total, h0.rows]):
            # the forward went through gs_sage_tail_z: the input gradients are its backward twin, ONE launch
            # (dz . W^T for both terms + relu mask + 1/s broadcast) instead of a small GEMM and the pull
            ops.sage_tail_dh0(h0, n_total, neighs[0].shape3[1], self.vars['self_weights'].value,
                              self.vars['neigh_weights'].value, o, dz, d_prev, jobs=None, stream=e.stream)
            return
        if self.neigh_input_dim == d_in and d_in % 4 == 0 and (not self.concat or o % 4 == 0):
            t2 = e.ws_mat((self.name, "dgrad2", k), n_total, 2 * d_in)       # [d_self | d_means] in one launch
            ops.sage_dense_dgrad(dz, n_total, o, self.concat, self.vars['self_weights'].value,
                                 self.vars['neigh_weights'].value, d_in, t2, stream=e.stream)
            d_self_all, d_means_all = t2.cols_slice(0, d_in), t2.cols_slice(d_in, 2 * d_in)
        else:
            d_self_all = e.ws_mat((self.name, "d_self", k), n_total, d_in)
            ops.dense_dgrad(dz, 0, o, n_total, self.vars['self_weights'].value, d_self_all, stream=e.stream)
            d_means_all = e.ws_mat((self.name, "d_means", k), n_total, self.neigh_input_dim)
            ops.dense_dgrad(dz, col_n, o, n_total, self.vars['neigh_weights'].value, d_means_all, stream=e.stream)
        if rate == 0:
            # ONE launch: d_prev = relu'(prev) * (d_self on the self rows + d_means / s broadcast over each hop's samples)
            segs = [(d_means_all.rows_slice(r, r + n), prev_offsets[h + 1], n, s, 1.0 / s) for h, nv, n, s, r, hr in _hops(neighs)]
            ops.input_grad_pull(d_prev, d_prev.rows, d_prev.d, d_self=d_self_all, n_self=n_total, segments=segs,
                                mask_y=prev_mask, stream=e.stream)
            return
        ops.dropout_rows(d_self_all, None, n_total, self._drop(rate, SITE_SELF, k), d_self_all, stream=e.stream)
        self._scatter_self(d_self_all, n_total, d_prev, prev_mask)
        for h, nv, n, s, r, hr in _hops(neighs):
            r0 = prev_offsets[h + 1]
            dst = d_prev.rows_slice(r0, r0 + n * s)
            mask = prev_mask.rows_slice(r0, r0 + n * s) if prev_mask is not None else None
            self._bwd_dropped(d_means_all.rows_slice(r, r + n), n, s, 1.0 / s, rate, SITE_NEIGH, k, hr, dst, mask,
                              (h + 1 < len(neighs)), ("n", h))

    def infer(self, scope, H):
        """The mean is linear, so the narrower side is reduced: with concat and output_dim < d_in the rows of H . W_neigh are
        averaged (602 -> 128 at Reddit's layer 0: 4.7 x fewer gathered bytes)."""
        from .inference import CSR_MEAN
        o, d_in = self.output_dim, H.d
        if not (self.concat and not self.bias and o % 4 == 0 and o < d_in):
            return self._infer_sage(scope, CSR_MEAN, H, True, H)
        P = scope.dense(self, H, [(self.vars['neigh_weights'].value, None, o, ACT_IDENTITY)])
        out = scope.table(self, 2 * o)
        scope.self_gemm(self, H, self.vars['self_weights'].value, o, out.cols_slice(0, o), self.act_code)
        scope.reduce(self, CSR_MEAN, P, False, out.cols_slice(o, 2 * o), self.act_code)
        return out


class GCNAggregator(_SageBase):
    """Same matmul parameters for self and neighbor vectors (aggregators.py:66-116).
    `concat` is stored but ignored, as in the reference (:79)."""

    def __init__(self, input_dim, output_dim, neigh_input_dim=None, dropout=0., bias=False, act=relu, name=None,
                 concat=False, **kwargs):
        super(GCNAggregator, self).__init__(**kwargs)
        if neigh_input_dim is None:
            neigh_input_dim = input_dim
        self._init_sage(input_dim, output_dim, neigh_input_dim, dropout, bias, act, concat, name,
                        neigh_rows=neigh_input_dim, bias_cols=output_dim, self_weights=False)
        # ONE matrix, named as the reference names it (scope + '/neigh_weights') but held under the key 'weights'
        self.vars = {('weights' if key == 'neigh_weights' else key): v for key, v in self.vars.items()}

    def prefetch_jobs(self, self_all, neighs, tag=0):
        return self._mean_jobs(self_all, neighs, tag, self_term=True)

    def prefetch(self, self_all, neighs, tag=0):
        """mean over {neighbors} U {self}  (aggregators.py:106-107); weight-free, so it can run ahead of time."""
        e = self.engine
        n_total = self_all.n
        d = neighs[0].shape3[2]
        k = len(self._saved)
        rate = _rate(self.dropout)
        means = e.ws_mat((self.name, "mean", k, tag), n_total, d, ld_multiple=32)      # whole 128-byte lines per row
        self_in = self._drop_self(self_all, rate, k) if rate > 0 else self_all            # dropout(self_vecs) (:105)
        for h, nv, n, s, r, hr in _hops(neighs):
            sv = self_in.slice(r, r + n)
            ops.gather_mean_fwd(nv.src, nv.ids, n, s, out=means.rows_slice(r, r + n), self_src=sv.src,
                                self_idx=sv.ids, drop=self._drop(rate, SITE_NEIGH, k, hr), stream=e.stream)
        return means

    def call_hops(self, self_all, neighs, means=None, side_jobs=None):
        e = self.engine
        n_total = self_all.n
        k = len(self._saved)
        rate = _rate(self.dropout)
        if means is None:
            means = self.prefetch(self_all, neighs)
        out = e.ws_mat((self.name, "out", k), n_total, self.output_dim)
        b = self.vars['bias'].value.buf if self.bias else None
        if e.stream_gemm and e.tiled3_fwd and n_total > 2048 and rate == 0 and self.output_dim % 4 == 0:
            ops.sage_dense_fwd_tiled3(None, None, means, n_total, None, self.vars['weights'].value, self.output_dim, self.act_code,
                                      b, out, side_jobs, stream=e.stream)
        elif e.stream_gemm and n_total > 2048 and rate == 0 and self.output_dim % 2 == 0:
            # stream form: LDS-free contraction waves (+ the next step's gather jobs) in one launch
            ops.sage_dense_fwd_stream(None, None, means, n_total, None, self.vars['weights'].value, self.output_dim, self.act_code,
                                      b, out, side_jobs, stream=e.stream)
        elif side_jobs:
            # horizontally fused launch: these GEMM tiles + the NEXT step's gather-mean waves share the CUs
            ops.sage_dense_fwd_cogather(None, None, means, None, n_total, None, self.vars['weights'].value, self.output_dim,
                                        False, self.act_code, b, out, side_jobs, stream=e.stream)
        else:
            ops.sage_dense_fwd(None, None, means, None, n_total, None, self.vars['weights'].value, self.output_dim, False,
                               self.act_code, b, out, stream=e.stream)
        self._push(_MeanSaved(self_all, neighs, means, out, rate))
        return out

    def backward_hops(self, d_out, pre_masked=False, d_prev=None, prev_mask=None, prev_offsets=None, embed_sink=None):
        e = self.engine
        self_all, neighs, means, out, rate, _, _ = self._saved.pop()
        n_total = self_all.n
        k = len(self._saved)
        dz = self._dz(d_out, out, n_total, self.output_dim, pre_masked)
        e.wgrad(self.vars['weights'], means, None, dz, 0, n_total)
        if self.bias:
            e.bgrad(self.vars['bias'], dz, n_total, self.output_dim)
        if embed_sink is not None:
            var, c = embed_sink                    # see MeanAggregator.backward_hops; self counts as one more neighbor
            d_means_e = e.ws_mat((self.name, "d_means_e", k), n_total, c)
            ops.dense_dgrad(dz, 0, self.output_dim, n_total, self.vars['weights'].value.rows_slice(0, c), d_means_e,
                            stream=e.stream)
            for h, nv, n, s, r, hr in _hops(neighs):
                dm = d_means_e.rows_slice(r, r + n)
                self._sink(var, dm, self_all.slice(r, r + n).ids, n, 1, 1.0 / (s + 1), rate, SITE_SELF, k, r, ("s", h))
                self._sink(var, dm, nv.ids, n, s, 1.0 / (s + 1), rate, SITE_NEIGH, k, hr, ("n", h))
        if d_prev is None:
            return
        d = means.d
        d_means = e.ws_mat((self.name, "d_means", k), n_total, d)
        ops.dense_dgrad(dz, 0, self.output_dim, n_total, self.vars['weights'].value, d_means, stream=e.stream)
        if rate == 0:
            # ONE launch; the self term of hop h is one more "neighbor" of weight 1/(s+1)
            segs = []
            for h, nv, n, s, r, hr in _hops(neighs):
                dm = d_means.rows_slice(r, r + n)
                segs.append((dm, r, n, 1, 1.0 / (s + 1)))
                segs.append((dm, prev_offsets[h + 1], n, s, 1.0 / (s + 1)))
            ops.input_grad_pull(d_prev, d_prev.rows, d_prev.d, segments=segs, mask_y=prev_mask, stream=e.stream)
            return
        for h, nv, n, s, r, hr in _hops(neighs):           # self parts first: d_self = d_means / (s + 1)
            mask = prev_mask.rows_slice(r, r + n) if prev_mask is not None else None
            self._bwd_dropped(d_means.rows_slice(r, r + n), n, 1, 1.0 / (s + 1), rate, SITE_SELF, k, r,
                              d_prev.rows_slice(r, r + n), mask, False, ("s", h))
        for h, nv, n, s, r, hr in _hops(neighs):
            r0 = prev_offsets[h + 1]
            dst = d_prev.rows_slice(r0, r0 + n * s)
            mask = prev_mask.rows_slice(r0, r0 + n * s) if prev_mask is not None else None
            self._bwd_dropped(d_means.rows_slice(r, r + n), n, s, 1.0 / (s + 1), rate, SITE_NEIGH, k, hr, dst, mask,
                              (h + 1 < len(neighs)), ("n", h))

    def infer(self, scope, H):
        """act(mean over {all neighbors} U {self} . W [+ b]) (aggregators.py:96-116).  The mean's weights sum to one, so when
        output_dim <= d_in the rows of H . W + b are averaged instead."""
        from .inference import CSR_MEAN_SELF
        o, d_in = self.output_dim, H.d
        W = self.vars['weights'].value
        b = self.vars['bias'].value.buf if self.bias else None
        if not (o % 4 == 0 and o <= d_in):
            return scope.reduce_sage(self, CSR_MEAN_SELF, H, True, None, None, W, o, False, self.act_code, b)   # one matrix, no self
        P = scope.dense(self, H, [(W, b, o, ACT_IDENTITY)])
        return scope.reduce(self, CSR_MEAN_SELF, P, False, scope.table(self, o), self.act_code)


class _PoolBase(_SageBase):
    """What the one- and two-layer pooling aggregators share: the relu-Dense stack over every neighbor row (widths by
    model_size, _WIDTHS) created BEFORE the SAGE variables, as the reference creates them."""
    _WIDTHS = {}
    fuse_pool = True           # switch: Dense + reduce_max in one launch per hop (False: the [n*s, hidden] rows go to HBM)
    dedup_pool = True          # switch: the first Dense once per DISTINCT sampled id where _dedup_wanted says it pays
    dedup_min_rows = None      # ... sampled rows above which it pays; None = read GS_POOL_DEDUP_MIN_ROWS (2048) at call time
    last_pool_kernel = None    # record: "split16" | "split_bf16x3" | "fp32_mfma", the distinct-id kernel taken (_mlp_distinct)
    last_unique = None         # record: (device count of distinct ids, sampled rows) of the last distinct-id forward

    def __init__(self, input_dim, output_dim, model_size="small", neigh_input_dim=None, dropout=0., bias=False,
                 act=relu, name=None, concat=False, **kwargs):
        super(_PoolBase, self).__init__(**kwargs)
        if neigh_input_dim is None:
            neigh_input_dim = input_dim
        if model_size not in self._WIDTHS:
            raise ops._lib.GraphsageAmdError("model_size must be 'small' or 'big'")
        self._widths = self._WIDTHS[model_size]
        self.mlp_layers = []
        for d_from, d_to in zip((neigh_input_dim,) + self._widths, self._widths):
            self.mlp_layers.append(Dense(input_dim=d_from, output_dim=d_to, act=relu, dropout=dropout,
                                         sparse_inputs=False, logging=self.logging))
        # the MLP weights are NOT part of aggregator.vars (aggregators.py:144-159, :303-325) -> no weight decay
        for layer in self.mlp_layers:
            for v in layer.vars.values():
                v.decay = False
        self._init_sage(input_dim, output_dim, neigh_input_dim, dropout, bias, act, concat, name,
                        neigh_rows=self._widths[-1], bias_cols=(2 if concat else 1) * output_dim)

    def _dedup_wanted(self, x_all, rows_total):
        """Run the pooling MLP once per DISTINCT sampled id of the step?  (the call_hops of both pooling classes)"""
        dedup_min = self.dedup_min_rows
        if dedup_min is None:
            dedup_min = int(os.environ.get("GS_POOL_DEDUP_MIN_ROWS", "2048"))
        return (x_all is not None and x_all.ids is not None and rows_total > dedup_min
                and x_all.src.rows < (1 << 31)
                and x_all.src.rows <= int(os.environ.get("GS_POOL_DEDUP_MAX_RATIO", "16")) * rows_total
                and self.dedup_pool)

    def _mlp_distinct(self, mlp, hidden, x_all, rows_total, k):
        """relu(X[uniq] . W + b) over the step's distinct ids: (H [rows_total, hidden] with the device count's leading rows
        filled, inv [rows_total], count).  Records the kernel taken in last_pool_kernel."""
        e = self.engine
        X, ids, nv_rows = x_all.src, x_all.ids, x_all.src.rows
        rank_ws = e.ws_i32((self.name, "dd_rank", k), 2 * nv_rows)       # [flags | ranks]: zero-initialised, self-cleaning
        sums_ws = e.ws_i32((self.name, "dd_sums", k), 256)
        uniq = e.ws_i32((self.name, "dd_uniq", k), rows_total)
        inv = e.ws_i32((self.name, "dd_inv", k), rows_total)
        cnt = e.ws_i32((self.name, "dd_count", k), 1)
        ops.call("gs_unique_ids", ops.ptr(ids), rows_total, nv_rows, ops.ptr(rank_ws), ops.ptr(sums_ws), ops.ptr(uniq),
                 ops.ptr(inv), ops.ptr(cnt), e.stream)
        Hu = e.ws_mat((self.name, "H_unique", k), rows_total, hidden)
        W, bmlp = mlp.vars['weights'].value, mlp.vars['bias'].value.buf
        self.last_pool_kernel = None
        if (e.split_pool and e.pool_f16 and not x_all.requires_grad and e.is_constant_table(X) and e.table16_fits(X)):
            # ... on the fp16 matrix pipe, operands as two fp16 pieces each (fp32 accuracy class, half the matrix-pipe work of
            # the three-piece form below, which is bound by the chip's POWER cap): the constant feature table is cut once.
            # A table with trainable leading columns (identity features, rewritten behind every optimizer launch) is NOT
            # constant -- its cut-once copy would be stale from the second step on -- and takes the three-piece kernel below,
            # which cuts the rows it reads in registers.
            self.last_pool_kernel = "split16"
            X2, rexp = e.table16_of(X)
            ws = e.ws_f32((self.name, "split_ws"), ops.split_tiled_ws_words())
            ops.call("gs_dense_fwd_rows_split16", ops.ptr(X2), ops.ptr(rexp), ops.ptr(uniq), X.d, rows_total, ops.ptr(cnt),
                     ops.ptr(e.split_of(mlp.vars['weights'], form="f16x2")), hidden, ACT_RELU, ops.ptr(bmlp),
                     Hu.ptr, Hu.ld, ops.ptr(ws), 4 * ws.numel(), e.stream)
        elif e.split_pool:
            # the 51 GF of the pooling MLP on the bf16 matrix pipe, operands as three bf16 pieces (fp32 accuracy)
            # (+ a workspace: the last, nearly empty round of its one-per-CU workgroups is cut along K, gs_split.hip)
            self.last_pool_kernel = "split_bf16x3"
            ws = e.ws_f32((self.name, "split_ws"), ops.split_tiled_ws_words())
            ops.call("gs_dense_fwd_rows_split_ws", X.ptr, X.ld, ops.ptr(uniq), X.d, rows_total, ops.ptr(cnt),
                     ops.ptr(e.split_of(mlp.vars['weights'])), hidden, ACT_RELU, ops.ptr(bmlp), Hu.ptr, Hu.ld,
                     ops.ptr(ws), 4 * ws.numel(), e.stream)
        else:
            self.last_pool_kernel = "fp32_mfma"
            ops.call("gs_dense_fwd_rows_dev", X.ptr, X.ld, ops.ptr(uniq), X.d, rows_total, ops.ptr(cnt), W.ptr, W.ld,
                     hidden, ACT_RELU, ops.ptr(bmlp), Hu.ptr, Hu.ld, e.stream)
        return Hu, inv, cnt

    def _max_gather(self, Hu, inv, neighs, width, pooled, argmax):
        """reduce_max over each hop's s samples of the per-distinct-id rows Hu, picked through the index `inv`."""
        e = self.engine
        for h, nv, n, s, r, hr in _hops(neighs):
            pr, ar = pooled.rows_slice(r, r + n), argmax[r:r + n]
            ops.call("gs_segment_max_gather_fwd", Hu.ptr, Hu.ld, inv.data_ptr() + 4 * hr, n, s, width, pr.ptr, pr.ld,
                     ar.data_ptr(), argmax.stride(0), e.stream)


class _PoolingAggregator(_PoolBase):
    """relu-MLP over every neighbor row, pooled over the s samples, then the SAGE matmuls
    (aggregators.py:119-195 for max, :197-273 for mean)."""
    POOL = "max"
    _WIDTHS = {"small": (512,), "big": (1024,)}
    hidden_dim = property(lambda self: self._widths[0])
    sparse_wgrad = True        # switch: layer 0's MLP weight gradient from the arg-max rows alone (gs_maxpool_sparse_wgrad)

    def call_hops(self, self_all, neighs, means=None, side_jobs=None):
        e = self.engine
        _run_jobs(e, side_jobs)
        n_total = self_all.n
        k = len(self._saved)
        rate = _rate(self.dropout)
        mlp = self.mlp_layers[0]
        flat, x_all, pieces, rows_total = _flatten(neighs)
        pooled = e.ws_mat((self.name, "pooled", k), n_total, self.hidden_dim)
        argmax = None
        if self.POOL == "max":
            argmax = e.ws_i32((self.name, "argmax", k), n_total * self.hidden_dim).view(n_total, self.hidden_dim)
        fused_pool = self.POOL == "max" and rate == 0 and self.fuse_pool and all(nv.shape3[1] <= 64 for nv in neighs)
        # layer 0 (rows gathered from the feature table through the model's contiguous id buffer): the MLP of a node does
        # not depend on who sampled it -- run it once per DISTINCT id of the step and let the reduce_max pick rows
        # through an index (37 % fewer GEMM rows at Reddit's degree)
        # gs_unique_ids makes three passes over a flag word per TABLE row (independent of the batch): worth it while the table
        # is within a small multiple of the step's sampled rows (Reddit: 233 k rows for 133 k ids), not for 10^7-node graphs
        dedup = fused_pool and self._dedup_wanted(x_all, rows_total)
        H = None
        if dedup:
            Hu, inv, cnt = self._mlp_distinct(mlp, self.hidden_dim, x_all, rows_total, k)
            self._max_gather(Hu, inv, neighs, self.hidden_dim, pooled, argmax)
            self.last_unique = (cnt, rows_total)
        elif fused_pool:
            # Dense (:176-179) + reduce_max (:181) in ONE launch per hop: the GEMM tiles hold whole neighbor groups and
            # reduce them in the epilogue, so the [n*s, hidden] activations never exist in HBM
            for (h, nv, n, s, r, hr), x in zip(_hops(neighs), flat):
                ops.dense_pool_max_fwd(x.src, x.ids, n, s, mlp.vars['weights'].value, mlp.vars['bias'].value.buf,
                                       pooled.rows_slice(r, r + n), argmax[r:r + n], stream=e.stream)
        else:
            # h_reshaped = Dense(reshape(neigh, [n*s, d]))   (aggregators.py:176-179): one GEMM over every neighbor row
            H = e.ws_mat((self.name, "H", k), rows_total, self.hidden_dim)
            if rate > 0:
                # the Dense's x = tf.nn.dropout(x, 1 - dropout) (layers.py:107) over every gathered neighbor row: the
                # dropped rows are materialised ([n*s, d]) and feed the MLP GEMM and its weight gradient as a dense operand
                dropped, r = [], 0
                for i, x in enumerate(pieces):
                    xd = e.ws_mat((self.name, "x_drop", k, i), x.n, x.src.d)
                    ops.dropout_rows(x.src, x.ids, x.n, self._drop(rate, SITE_MLP, k, r), xd, stream=e.stream)
                    dropped.append(Rows(xd, None, x.n, x.requires_grad))
                    r += x.n
                pieces = dropped
            _pieces_fwd(e, pieces, mlp.vars['weights'].value, mlp.vars['bias'].value.buf, self.hidden_dim, ACT_RELU, H)
            for h, nv, n, s, r, hr in _hops(neighs):
                if self.POOL == "max":
                    ops.segment_max_fwd(H.rows_slice(hr, hr + n * s), n, s, pooled.rows_slice(r, r + n), argmax[r:r + n],
                                        stream=e.stream)                                             # reduce_max (:181)
                else:
                    ops.gather_mean_fwd(H.rows_slice(hr, hr + n * s), None, n, s, out=pooled.rows_slice(r, r + n),
                                        stream=e.stream)                                             # reduce_mean (:259)
        out = self._sage_out(self_all, pooled, n_total, k)
        self._push(_PoolSaved(self_all, neighs, pieces, rows_total, H, pooled, argmax, out, rate))
        return out

    def backward_hops(self, d_out, pre_masked=False, d_prev=None, prev_mask=None, prev_offsets=None, embed_sink=None):
        e = self.engine
        saved = self._saved.pop()
        self_all, neighs, pieces, rows_total, H, pooled, argmax, out, rate = saved
        n_total = self_all.n
        k = len(self._saved)
        o = self.output_dim
        mlp = self.mlp_layers[0]
        dz, col_n = self._sage_bwd(d_out, out, n_total, pre_masked, self_all.src, self_all.ids, pooled)
        d_pooled = e.ws_mat((self.name, "d_pooled", k), n_total, self.hidden_dim)
        ops.dense_dgrad(dz, col_n, o, n_total, self.vars['neigh_weights'].value, d_pooled, stream=e.stream)
        dpm = None
        if self.POOL == "max":
            # reduce_max grad then the Dense's relu grad: only the arg-max row of each (group, column) receives
            # gradient, and only where the pooled activation is > 0.
            dpm = e.ws_mat((self.name, "d_pooled_masked", k), n_total, self.hidden_dim)
            ops.act_bwd(d_pooled, pooled, n_total, self.hidden_dim, ACT_RELU, dpm, stream=e.stream)
            e.bgrad(mlp.vars['bias'], dpm, n_total, self.hidden_dim)   # column sums of dH == column sums of dpm
        threads = min(512, (self.hidden_dim + 63) // 64 * 64)
        sparse = (self.POOL == "max" and d_prev is None and embed_sink is None and rate == 0
                  and all(nv.ids is not None for nv in neighs)
                  and self.sparse_wgrad
                  and 16 * max(nv.shape3[1] for nv in neighs) <= 4 * threads)
        if sparse:
            # layer 0: the gathered feature rows need no gradient, so dH = [n*s, hidden] is never materialised; the
            # MLP weight gradient is accumulated straight from the arg-max rows (gs_maxpool_sparse_wgrad)
            for h, nv, n, s, r, hr in _hops(neighs):
                e.sparse_pool_wgrad(mlp.vars['weights'], nv.src, nv.ids, n, s, argmax[r:r + n], dpm.rows_slice(r, r + n))
            return
        dH = e.ws_mat((self.name, "dH", k), rows_total, self.hidden_dim)
        for h, nv, n, s, r, hr in _hops(neighs):
            if self.POOL == "max":
                ops.segment_max_bwd(dpm.rows_slice(r, r + n), pooled.rows_slice(r, r + n), argmax[r:r + n], n, s,
                                    dH.rows_slice(hr, hr + n * s), stream=e.stream)
            else:
                ops.mean_bwd(d_pooled.rows_slice(r, r + n), n, s, 1.0 / s, dH.rows_slice(hr, hr + n * s),
                             mask_y=H.rows_slice(hr, hr + n * s), stream=e.stream)
        if self.POOL != "max":
            e.bgrad(mlp.vars['bias'], dH, rows_total, self.hidden_dim)
        _pieces_wgrad(e, mlp.vars['weights'], pieces, dH)
        self._row_input_grads(saved, k, dz, dH, self.hidden_dim, mlp.vars['weights'].value, embed_sink, d_prev, prev_mask,
                              prev_offsets, drop=(lambda: self._drop(rate, SITE_MLP, k)) if rate > 0 else None)

    def infer(self, scope, H):
        """The MLP (aggregators.py:176-179) runs once per row the layer may read, then the hidden table is max- / mean-reduced
        over every computed row's whole neighbor list, then the SAGE matmuls."""
        from . import inference as inf
        mlp = self.mlp_layers[0]
        Hh = scope.dense(self, H, [(mlp.vars['weights'].value, mlp.vars['bias'].value.buf, self.hidden_dim, ACT_RELU)])
        return self._infer_sage(scope, inf.CSR_MAX if self.POOL == "max" else inf.CSR_MEAN, Hh, False, H)


class MaxPoolingAggregator(_PoolingAggregator):
    """Aggregates via max-pooling over MLP functions (aggregators.py:119-195)."""
    POOL = "max"


class MeanPoolingAggregator(_PoolingAggregator):
    """Aggregates via mean-pooling over MLP functions (aggregators.py:197-273)."""
    POOL = "mean"


class AttentionPoolingAggregator(_PoolBase):
    """Aggregates via attention pooling over an MLP function: the pooling aggregators' relu-Dense over every neighbor row, then a
    LEARNED weighting of the s rows instead of their max or mean, then the SAGE matmuls (DESIGN "Attention pooling"):

        V_j = relu(x_j . W_mlp + b_mlp);  t_j = <V_j, a>;  alpha = softmax_j(t_j);  pooled = sum_j alpha_j V_j

    hidden = 512 ("small") or 1024 ("big").  The gate `a` [hidden] (glorot as a [hidden, 1] matrix), like the Dense, is not in
    aggregator.vars (no weight decay; still clipped and updated by Adam).  The gate does not depend on the node that asks, so the
    Dense runs once per DISTINCT sampled id where _dedup_wanted says so and the attention reads through the index
    (gs_segment_attn_fwd / _bwd, csrc/gs_attn.hip).  Dropout applies to the Dense's input rows, as in _PoolingAggregator."""
    _WIDTHS = {"small": (512,), "big": (1024,)}
    hidden_dim = property(lambda self: self._widths[0])

    def __init__(self, input_dim, output_dim, model_size="small", **kwargs):
        super(AttentionPoolingAggregator, self).__init__(input_dim, output_dim, model_size=model_size, **kwargs)
        if not ops.segment_attn_supported(1, self.hidden_dim):
            raise ops._lib.GraphsageAmdError("AttentionPoolingAggregator: hidden width %d outside the kernels' range" % self.hidden_dim)
        self.attn_a = self.engine.add_variable(self.name + '/attn_vars/a', glorot((self.hidden_dim, 1)).reshape(-1), decay=False)

    @staticmethod
    def check_samples(num_samples):
        """Refuse a fan-out outside the range of gs_segment_attn_fwd / _bwd (the drivers call this before training)."""
        for s in num_samples:
            if not 1 <= int(s) <= ops.ATTN_MAX_S:
                raise ops._lib.GraphsageAmdError("graphsage_attn takes 1 <= samples <= %d per layer (got %d)" % (ops.ATTN_MAX_S, s))

    def call_hops(self, self_all, neighs, means=None, side_jobs=None):
        e = self.engine
        _run_jobs(e, side_jobs)
        self.check_samples([nv.shape3[1] for nv in neighs])
        n_total = self_all.n
        k = len(self._saved)
        rate = _rate(self.dropout)
        mlp = self.mlp_layers[0]
        hid = self.hidden_dim
        a = self.attn_a.value.buf
        _, x_all, pieces, rows_total = _flatten(neighs)
        pooled = e.ws_mat((self.name, "pooled", k), n_total, hid)
        alpha = e.ws_f32((self.name, "alpha", k), rows_total)
        self.last_pool_kernel = self.last_unique = None
        inv = None
        if rate == 0 and self._dedup_wanted(x_all, rows_total):
            # the Dense once per DISTINCT id of the step; the attention picks its rows through `inv`
            H, inv, cnt = self._mlp_distinct(mlp, hid, x_all, rows_total, k)
            self.last_unique = (cnt, rows_total)
        else:
            H = e.ws_mat((self.name, "H", k), rows_total, hid)
            if rate > 0:
                # the Dense's x = tf.nn.dropout(x, 1 - dropout) over every gathered neighbor row (as _PoolingAggregator)
                dropped, r = [], 0
                for i, x in enumerate(pieces):
                    xd = e.ws_mat((self.name, "x_drop", k, i), x.n, x.src.d)
                    ops.dropout_rows(x.src, x.ids, x.n, self._drop(rate, SITE_MLP, k, r), xd, stream=e.stream)
                    dropped.append(Rows(xd, None, x.n, x.requires_grad))
                    r += x.n
                pieces = dropped
            _pieces_fwd(e, pieces, mlp.vars['weights'].value, mlp.vars['bias'].value.buf, hid, ACT_RELU, H)
        for h, nv, n, s, r, hr in _hops(neighs):
            ops.segment_attn_fwd(H if inv is not None else H.rows_slice(hr, hr + n * s), inv[hr:hr + n * s] if inv is not None else None,
                                 a, n, s, pooled.rows_slice(r, r + n), alpha[hr:hr + n * s], stream=e.stream)
        out = self._sage_out(self_all, pooled, n_total, k)
        self._push(_AttnSaved(self_all, neighs, pieces, rows_total, H, inv, alpha, pooled, out, rate))
        return out

    def backward_hops(self, d_out, pre_masked=False, d_prev=None, prev_mask=None, prev_offsets=None, embed_sink=None):
        e = self.engine
        saved = self._saved.pop()
        self_all, neighs, pieces, rows_total, H, inv, alpha, pooled, out, rate = saved
        n_total = self_all.n
        k = len(self._saved)
        hid = self.hidden_dim
        mlp = self.mlp_layers[0]
        var_a = self.attn_a
        dz, col_n = self._sage_bwd(d_out, out, n_total, pre_masked, self_all.src, self_all.ids, pooled)
        d_pooled = e.ws_mat((self.name, "d_pooled", k), n_total, hid)
        ops.dense_dgrad(dz, col_n, self.output_dim, n_total, self.vars['neigh_weights'].value, d_pooled, stream=e.stream)
        # softmax and gate gradients, then the Dense's relu: dV per SAMPLED row; da as slabs of the gate's arena, one per workgroup
        dV = e.ws_mat((self.name, "dV", k), rows_total, hid)
        # a slab is a workgroup, and the hops' launches follow each other: the sum of rows_h / slabs_h is least where the gate's
        # free slabs go to the hops by the SQUARE ROOT of their sampled rows (Reddit's layer 0: 11 for the 512 groups of 10, 52
        # for the 5120 groups of 25); at least one each and no more than a hop has groups of 16
        free = MAX_SLABS - var_a.n_slabs - len(neighs)
        roots = [(nv.shape3[0] * nv.shape3[1]) ** 0.5 for nv in neighs]
        for h, nv, n, s, r, hr in _hops(neighs):
            n_slabs = int(max(1, min(1 + int(max(free, 0) * roots[h] / sum(roots)), (n + 15) // 16)))
            if var_a.n_slabs + n_slabs > MAX_SLABS:
                raise ops._lib.GraphsageAmdError("slab arena of %s exhausted" % var_a.name)
            ops.segment_attn_bwd(d_pooled.rows_slice(r, r + n), H if inv is not None else H.rows_slice(hr, hr + n * s),
                                 inv[hr:hr + n * s] if inv is not None else None, var_a.value.buf, alpha[hr:hr + n * s], n, s,
                                 dV.rows_slice(hr, hr + n * s), n_slabs, var_a.slab_ptr(var_a.n_slabs), stream=e.stream)
            var_a.n_slabs += n_slabs
        e.bgrad(mlp.vars['bias'], dV, rows_total, hid)
        _pieces_wgrad(e, mlp.vars['weights'], pieces, dV)
        self._row_input_grads(saved, k, dz, dV, hid, mlp.vars['weights'].value, embed_sink, d_prev, prev_mask, prev_offsets,
                              drop=(lambda: self._drop(rate, SITE_MLP, k)) if rate > 0 else None)

    def infer(self, scope, H):
        """The Dense once per row the layer may read, into a table with one spare column; the gate's score of every such row into
        that column (gs_attn_scores); then the softmax-weighted sum over every computed row's WHOLE neighbor list (a duplicate
        entry counts as often as it occurs) and the SAGE matmuls."""
        from .inference import CSR_SOFTMAX
        mlp = self.mlp_layers[0]
        Hh = scope.dense(self, H, [(mlp.vars['weights'].value, mlp.vars['bias'].value.buf, self.hidden_dim, ACT_RELU)], spare=4)
        ops.attn_scores(Hh, self.attn_a.value.buf, stream=self.engine.stream)
        return self._infer_sage(scope, CSR_SOFTMAX, Hh, False, H)


class SeqAggregator(_SageBase):
    """Aggregates via a standard LSTM (aggregators.py:363-449): TF 1.x BasicLSTMCell(H) run by dynamic_rnn over the s sampled
    neighbors of each node, for the first L = max(1, #non-zero neighbor rows) steps (aggregators.py:411-414); the hidden state
    after step L - 1 is the neighborhood vector, then the SAGE matmuls.  H = 128 ("small") or 256 ("big").  SeqAggregator._call
    applies no dropout.

    The cell's kernel [neigh_in + H, 4H] and bias [4H] are NOT in aggregator.vars (no weight decay; still clipped and
    updated by Adam).  The kernel is held as two variables, its x_t rows (`lstm_wx`) and its h_{t-1} rows (`lstm_wh`): a
    weight gradient's operand has the variable's row count, and clip + Adam are elementwise, so the split changes no result.
    Every hop of a layer shares one cell, as the reference's reused variable scope does.

    Per layer: G = X . W_x + b over every neighbor row (one contraction per contiguous piece), the lengths, ONE recurrence launch
    over all hops (gs_lstm_fwd; the activated gates overwrite G), then [self . W_self | h_last . W_neigh].  The backward runs
    the recurrence in reverse (gs_lstm_bwd; dG overwrites the gates) and sends dG through the ordinary weight-gradient and
    input-gradient contractions."""

    def __init__(self, input_dim, output_dim, model_size="small", neigh_input_dim=None, dropout=0., bias=False,
                 act=relu, name=None, concat=False, **kwargs):
        super(SeqAggregator, self).__init__(**kwargs)
        if neigh_input_dim is None:
            neigh_input_dim = input_dim
        if model_size not in ("small", "big"):
            raise ops._lib.GraphsageAmdError("model_size must be 'small' or 'big'")
        hidden_dim = self.hidden_dim = 128 if model_size == "small" else 256
        if bias and concat:
            # the reference adds a [output_dim] bias to the [n, 2 * output_dim] concatenation, which TF refuses
            raise ops._lib.GraphsageAmdError("SeqAggregator: bias needs concat=False (the bias has output_dim entries)")
        self._init_sage(input_dim, output_dim, neigh_input_dim, dropout, bias, act, concat, name,
                        neigh_rows=hidden_dim, bias_cols=output_dim)
        e = self.engine
        kernel = glorot((neigh_input_dim + hidden_dim, 4 * hidden_dim))       # BasicLSTMCell kernel (glorot over the whole)
        cell = self.name + '/rnn/basic_lstm_cell'
        self.lstm_wx = e.add_variable(cell + '/kernel_x', kernel[:neigh_input_dim], decay=False)
        self.lstm_wh = e.add_variable(cell + '/kernel_h', kernel[neigh_input_dim:], decay=False)
        self.lstm_b = e.add_variable(cell + '/bias', zeros((4 * hidden_dim,)), decay=False)

    def call_hops(self, self_all, neighs, means=None, side_jobs=None):
        e = self.engine
        _run_jobs(e, side_jobs)
        n_total = self_all.n
        k = len(self._saved)
        H = self.hidden_dim
        _, _, pieces, rows_total = _flatten(neighs)
        # one recurrence segment per hop: n sequences of s steps, step rows in the hop's order of the flattened neighbors
        segs = [(nv.src, nv.ids, n, s, hr) for h, nv, n, s, r, hr in _hops(neighs)]
        G = e.ws_mat((self.name, "lstm_gates", k), rows_total, 4 * H)
        # [x_t, h_{t-1}] . kernel + bias, the x_t half for every step at once
        _pieces_fwd(e, pieces, self.lstm_wx.value, self.lstm_b.value.buf, 4 * H, ACT_IDENTITY, G)
        lengths = e.ws_i32((self.name, "lstm_len", k), n_total)
        ops.lstm_lengths(segs, neighs[0].shape3[2], lengths, stream=e.stream)
        C = e.ws_mat((self.name, "lstm_c", k), rows_total, H)
        Hp = e.ws_mat((self.name, "lstm_h_prev", k), rows_total, H)
        h_last = e.ws_mat((self.name, "lstm_h_last", k), n_total, H)
        ops.lstm_fwd(segs, H, self.lstm_wh.value, lengths, G, G, C, Hp, h_last, stream=e.stream)
        # from_self / from_neighs + concat|add + bias + act (aggregators.py:437-449): one launch for all hops
        n_out = self.output_dim * (2 if self.concat else 1)
        out = e.ws_mat((self.name, "out", k), n_total, n_out)
        b = self.vars['bias'].value.buf if self.bias else None
        ops.sage_dense_fwd(self_all.src, self_all.ids, h_last, None, n_total, self.vars['self_weights'].value,
                           self.vars['neigh_weights'].value, self.output_dim, self.concat, self.act_code, b, out,
                           stream=e.stream)
        self._push(_SeqSaved(self_all, neighs, pieces, rows_total, segs, lengths, G, C, Hp, h_last, out))
        return out

    def backward_hops(self, d_out, pre_masked=False, d_prev=None, prev_mask=None, prev_offsets=None, embed_sink=None):
        e = self.engine
        saved = self._saved.pop()
        if embed_sink is not None:
            raise ops._lib.GraphsageAmdError("SeqAggregator: trainable identity features are not supported")
        self_all, neighs, pieces, rows_total, segs, lengths, A, C, Hp, h_last, out = saved
        n_total = self_all.n
        k = len(self._saved)
        H = self.hidden_dim
        dz, col_n = self._sage_bwd(d_out, out, n_total, pre_masked, self_all.src, self_all.ids, h_last)
        dh_last = e.ws_mat((self.name, "d_lstm_h_last", k), n_total, H)
        ops.dense_dgrad(dz, col_n, self.output_dim, n_total, self.vars['neigh_weights'].value, dh_last, stream=e.stream)
        wt = e.ws_f32((self.name, "lstm_wh_t"), 4 * H * H)
        dG = ops.lstm_bwd(segs, H, self.lstm_wh.value, wt, lengths, A, C, dh_last, A, stream=e.stream)   # dG over the gates
        e.wgrad(self.lstm_wh, Hp, None, dG, 0, rows_total)
        e.bgrad(self.lstm_b, dG, rows_total, 4 * H)
        _pieces_wgrad(e, self.lstm_wx, pieces, dG)
        self._row_input_grads(saved, k, dz, dG, 4 * H, self.lstm_wx.value, None, d_prev, prev_mask, prev_offsets)

    def infer(self, scope, H):
        raise ops._lib.GraphsageAmdError("SeqAggregator has no full-neighborhood form: an LSTM over a random permutation of a "
                                         "SAMPLE of the neighbors has no meaning over the whole list (use eval_step)")


class TwoMaxLayerPoolingAggregator(_PoolBase):
    """Aggregates via pooling over two MLP functions (aggregators.py:276-361): Dense(in -> hid1, relu), Dense(hid1 -> hid2,
    relu) over every neighbor row, reduce_max over the s samples, then the SAGE matmuls.  hid1 / hid2 = 512 / 256 ("small")
    or 1024 / 512 ("big").  Neither Dense is in aggregator.vars (no weight decay; still clipped and updated by Adam).

    Layer 1 runs as _PoolingAggregator's MLP does (once per distinct id of the step where that pays) and is kept as H1; layer 2
    and the reduce_max are one launch per hop (gs_dense_pool_max_fwd over H1), or layer 2 per distinct row and
    gs_segment_max_gather_fwd.  Backward: the W2 gradient comes from the arg-max rows of H1 alone (gs_maxpool_sparse_wgrad),
    and dH1 -- the pooled gradient taken back through W2 and the first relu to EVERY neighbor row -- from gs_pool2_dgrad
    (`fuse_dgrad`; False, or a shape outside the kernel's range: gs_segment_max_bwd + gs_dense_dgrad + gs_act_bwd).

    Dropout is refused: the reference drops the input of both Dense layers, and the second has no mask site here."""
    _WIDTHS = {"small": (512, 256), "big": (1024, 512)}
    hidden_dim_1 = property(lambda self: self._widths[0])
    hidden_dim_2 = property(lambda self: self._widths[1])
    fuse_dgrad = True          # switch: dH1 by gs_pool2_dgrad; False = the three-launch composition
    last_dgrad_kernel = None   # record: "pool2_dgrad" | "composed", what the last backward pass took
    last_dgrad_indexed = None  # ... and whether it read H1 through the distinct-id index

    def call_hops(self, self_all, neighs, means=None, side_jobs=None):
        e = self.engine
        if _rate(self.dropout) > 0:
            raise ops._lib.GraphsageAmdError("dropout > 0 is not supported with the two-layer max-pooling aggregator "
                                             "(graphsage_twomaxpool)")
        _run_jobs(e, side_jobs)
        n_total = self_all.n
        k = len(self._saved)
        mlp1, mlp2 = self.mlp_layers
        hid1, hid2 = self.hidden_dim_1, self.hidden_dim_2
        W2, b2 = mlp2.vars['weights'].value, mlp2.vars['bias'].value.buf
        _, x_all, pieces, rows_total = _flatten(neighs)
        pooled = e.ws_mat((self.name, "pooled2", k), n_total, hid2)
        argmax = e.ws_i32((self.name, "argmax2", k), n_total * hid2).view(n_total, hid2)
        fused_pool = self.fuse_pool and all(nv.shape3[1] <= 64 for nv in neighs)
        self.last_pool_kernel = self.last_unique = None
        inv = None
        if fused_pool and self._dedup_wanted(x_all, rows_total):
            # layer 1, then layer 2, once per DISTINCT id of the step; the reduce_max picks rows through `inv`
            H1, inv, cnt = self._mlp_distinct(mlp1, hid1, x_all, rows_total, k)
            H2 = e.ws_mat((self.name, "H2_unique", k), rows_total, hid2)
            ops.sage_dense_fwd(None, None, H1, None, rows_total, None, W2, hid2, False, ACT_RELU, b2, H2, stream=e.stream)
            self._max_gather(H2, inv, neighs, hid2, pooled, argmax)
            self.last_unique = (cnt, rows_total)
        else:
            # h = Dense(reshape(neigh, [n*s, d]))   (aggregators.py:338-341, first layer): one GEMM over every neighbor row
            H1 = e.ws_mat((self.name, "H1", k), rows_total, hid1)
            _pieces_fwd(e, pieces, mlp1.vars['weights'].value, mlp1.vars['bias'].value.buf, hid1, ACT_RELU, H1)
            H2 = None
            if not fused_pool:
                H2 = e.ws_mat((self.name, "H2", k), rows_total, hid2)
                ops.sage_dense_fwd(None, None, H1, None, rows_total, None, W2, hid2, False, ACT_RELU, b2, H2, stream=e.stream)
            for h, nv, n, s, r, hr in _hops(neighs):
                if fused_pool:         # second Dense + reduce_max (:341) in ONE launch: [n*s, hid2] never exists
                    ops.dense_pool_max_fwd(H1.rows_slice(hr, hr + n * s), None, n, s, W2, b2, pooled.rows_slice(r, r + n),
                                           argmax[r:r + n], stream=e.stream)
                else:
                    ops.segment_max_fwd(H2.rows_slice(hr, hr + n * s), n, s, pooled.rows_slice(r, r + n), argmax[r:r + n],
                                        stream=e.stream)
        out = self._sage_out(self_all, pooled, n_total, k)
        self._push(_Pool2Saved(self_all, neighs, pieces, rows_total, H1, inv, pooled, argmax, out))
        return out

    def backward_hops(self, d_out, pre_masked=False, d_prev=None, prev_mask=None, prev_offsets=None, embed_sink=None):
        e = self.engine
        saved = self._saved.pop()
        self_all, neighs, pieces, rows_total, H1, inv, pooled, argmax, out = saved
        n_total = self_all.n
        k = len(self._saved)
        o = self.output_dim
        mlp1, mlp2 = self.mlp_layers
        hid1, hid2 = self.hidden_dim_1, self.hidden_dim_2
        W1, W2 = mlp1.vars['weights'], mlp2.vars['weights']
        dz, col_n = self._sage_bwd(d_out, out, n_total, pre_masked, self_all.src, self_all.ids, pooled)
        d_pooled = e.ws_mat((self.name, "d_pooled2", k), n_total, hid2)
        ops.dense_dgrad(dz, col_n, o, n_total, self.vars['neigh_weights'].value, d_pooled, stream=e.stream)
        # reduce_max grad then the second Dense's relu grad: only the arg-max row of each (group, column), where pooled > 0
        dpm = e.ws_mat((self.name, "d_pooled2_masked", k), n_total, hid2)
        ops.act_bwd(d_pooled, pooled, n_total, hid2, ACT_RELU, dpm, stream=e.stream)
        e.bgrad(mlp2.vars['bias'], dpm, n_total, hid2)           # column sums of dH2 == column sums of dpm
        # the range of gs_pool2_dgrad, and of gs_maxpool_sparse_wgrad (16 s <= 4 min(512, round_up(hid2, 64))): at both model sizes
        # that is s <= 64
        s_max = max(nv.shape3[1] for nv in neighs)
        fits = ops.pool2_dgrad_supported(s_max, hid1, hid2) and 16 * s_max <= 4 * min(512, (hid2 + 63) // 64 * 64)
        fused = self.fuse_dgrad and fits
        self.last_dgrad_kernel = "pool2_dgrad" if fused else "composed"
        self.last_dgrad_indexed = inv is not None                # H1 held one row per distinct id, read through h_idx
        dH1 = e.ws_mat((self.name, "dH1", k), rows_total, hid1)
        H1x = H1                                                 # H1 per sampled row, for the dense forms
        if fused:
            W2T = e.ws_mat((self.name, "W2T"), hid2, hid1)       # this step's W2^T: re-made in every backward pass
            ops.pool2_transpose(W2.value, W2T, stream=e.stream)
        else:
            dH2 = e.ws_mat((self.name, "dH2", k), rows_total, hid2)
            if inv is not None:
                H1x = e.ws_mat((self.name, "H1_rows", k), rows_total, hid1)
                ops.gather_rows(H1, inv, out=H1x, stream=e.stream)
        iota = None
        if fits and inv is None:
            # H1 holds one row per sampled row: gs_maxpool_sparse_wgrad reads each hop's slice of it through 0 .. n s - 1
            n_iota = max(nv.shape3[0] * nv.shape3[1] for nv in neighs)
            iota = ops.pool2_iota(e.ws_i32((self.name, "iota", k), n_iota), n_iota, stream=e.stream)
        for h, nv, n, s, r, hr in _hops(neighs):
            dp, am = dpm.rows_slice(r, r + n), argmax[r:r + n]
            dH = dH1.rows_slice(hr, hr + n * s)
            if fused:
                # the pooled gradient back through W2 and the first relu to every neighbor row, dH2 never formed
                if inv is not None:
                    ops.pool2_dgrad(dp, am, H1, inv[hr:hr + n * s], n, s, dH, W2T=W2T, stream=e.stream)
                else:
                    ops.pool2_dgrad(dp, am, H1.rows_slice(hr, hr + n * s), None, n, s, dH, W2T=W2T, stream=e.stream)
            else:
                d2, hx = dH2.rows_slice(hr, hr + n * s), H1x.rows_slice(hr, hr + n * s)
                ops.segment_max_bwd(dp, pooled.rows_slice(r, r + n), am, n, s, d2, stream=e.stream)
                ops.dense_dgrad(d2, 0, hid2, n * s, W2.value, dH, stream=e.stream)
                ops.act_bwd(dH, hx, n * s, hid1, ACT_RELU, dH, stream=e.stream)
            if fits:
                # dW2 from the arg-max rows of H1 alone (dH2 = [n*s, hid2] has one non-zero per (group, column))
                if inv is not None:
                    e.sparse_pool_wgrad(W2, H1, inv[hr:hr + n * s], n, s, am, dp)
                else:
                    e.sparse_pool_wgrad(W2, H1.rows_slice(hr, hr + n * s), iota[:n * s], n, s, am, dp)
            else:
                e.wgrad(W2, H1x.rows_slice(hr, hr + n * s), None, dH2.rows_slice(hr, hr + n * s), 0, n * s)
        e.bgrad(mlp1.vars['bias'], dH1, rows_total, hid1)
        _pieces_wgrad(e, W1, pieces, dH1)
        self._row_input_grads(saved, k, dz, dH1, hid1, W1.value, embed_sink, d_prev, prev_mask, prev_offsets)

    def infer(self, scope, H):
        """_PoolingAggregator.infer with both Dense layers run once per row the layer may read, then the hid2-wide table is
        max-reduced."""
        from .inference import CSR_MAX
        stack = [(m.vars['weights'].value, m.vars['bias'].value.buf, width, ACT_RELU)
                 for m, width in zip(self.mlp_layers, (self.hidden_dim_1, self.hidden_dim_2))]
        return self._infer_sage(scope, CSR_MAX, scope.dense(self, H, stack), False, H)
