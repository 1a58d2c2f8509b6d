"""BipartiteEdgePredLayer -- graphsage/prediction.py:12-125: the three losses (xent :102-110, skipgram :112-117, hinge
:119-125), the affinities with or without bilinear weights (:68-92) and the MRR ranks of models.py:393-405 as fused
gfx950 kernels that also produce the gradients w.r.t. the three groups of normalised embeddings.

Every configuration runs the one head kernel, gs_linkpred_loss_fwd_bwd (csrc/gs_linkpred_loss.hip); the default one
(loss_fn='xent', bilinear_weights=False: what models.py:363-366 instantiates) may run the model's fused tail instead.

The skipgram loss keeps the reference's sign exactly: it is written `aff - log sum_j exp(neg_aff_j)` (:115-116), so
MINIMISING it pushes the pairs apart.  That is the reference's own source and is not "fixed" here.  neg_sample_weights
enters the xent loss only, as in the reference.  `bias=True` creates vars['bias'] ([1] zeros, :55-56); the reference never
reads it, so it gets no gradient and is never updated.

loss_fn='infonce' is not in the reference: the in-batch softmax, gs_linkpred_infonce_fwd_bwd (csrc/gs_infonce.hip).  Every
normalised outputs2 row of the batch and every sampled negative is a candidate for every left-operand row,
    L_ij = <u_i, [y2 ; neg]_j> / temperature,   loss_i = logsumexp_{j not masked} L_ij - L_ii,
where candidate j < B, j != i is masked for row i when ids2[j] == ids2[i] or ids2[j] == ids1[i] (the same context node in
another pair, or the query node itself).  One direction only (query -> context); aff_all and the MRR stay defined over the
sampled negatives, as for the other losses."""
from . import ops
from .inits import glorot, zeros
from .layers import Layer

LOSS_FNS = ('xent', 'skipgram', 'hinge', 'infonce')


class BipartiteEdgePredLayer(Layer):
    def __init__(self, input_dim1, input_dim2, placeholders, dropout=False, act="sigmoid", loss_fn='xent',
                 neg_sample_weights=1.0, bias=False, bilinear_weights=False, temperature=0.1, **kwargs):
        super(BipartiteEdgePredLayer, self).__init__(**kwargs)
        if loss_fn not in LOSS_FNS:
            raise ValueError("loss_fn must be one of %s (got %r)" % (", ".join(LOSS_FNS), loss_fn))
        lo, hi = ops.INFONCE_TAU_RANGE
        if loss_fn == 'infonce' and not lo <= float(temperature) <= hi:
            raise ValueError("temperature must lie in [%g, %g] (got %r)" % (lo, hi, temperature))
        self.input_dim1 = input_dim1
        self.input_dim2 = input_dim2
        self.act = act
        self.bias = bias
        self.eps = 1e-7
        self.margin = 0.1
        self.temperature = float(temperature)          # the infonce loss only
        self.neg_sample_weights = neg_sample_weights
        self.bilinear_weights = bilinear_weights
        self.loss_fn = loss_fn
        self.dropout = 0.
        self.output_dim = 1
        e = self.engine
        if loss_fn == 'infonce' and (input_dim1 != input_dim2 or input_dim1 not in ops.LP_WIDTHS):
            raise ops._lib.GraphsageAmdError("loss_fn='infonce' needs input_dim1 == input_dim2 in %s (got %d, %d)"
                                             % (list(ops.LP_WIDTHS), input_dim1, input_dim2))
        if bilinear_weights:
            if input_dim1 != input_dim2 or input_dim1 not in ops.LP_WIDTHS:
                raise ops._lib.GraphsageAmdError("bilinear_weights needs input_dim1 == input_dim2 in %s (got %d, %d)"
                                                 % (list(ops.LP_WIDTHS), input_dim1, input_dim2))
            # xavier_initializer (:49-53); no weight decay: _loss decays aggregator variables only (models.py:386-388)
            self.vars['weights'] = e.add_variable(self.name + "/weights", glorot((input_dim1, input_dim2)), decay=False)
        if bias:
            self.vars['bias'] = e.add_variable(self.name + "/bias", zeros((self.output_dim,)), decay=False)

    @property
    def default_head(self):
        """The configuration of models.py:363-366: the xent kernels (and the model's fused tail) apply."""
        return self.loss_fn == 'xent' and not self.bilinear_weights

    def loss_and_grads_fused(self, z_all, outputs_all, batch_size, n_neg, scale, loss_rows, rr_rows, aff_all, d_z_all,
                             epilogue=None, ids=None):
        """z_all: Mat [2B + n_neg, d] RAW aggregator outputs.  One launch (+ a small one for the negatives' rows):
        outputs_all = l2_normalize(z_all) (models.py:368-370), loss_rows (the per-pair loss), rr_rows (1/(rank+1),
        models.py:399-404), aff_all ([neg_aff | aff], models.py:395-400) and d_z_all = scale * dLoss/d(z_all) (the gradient
        carried back through the normalisation).
        With bilinear weights the schedule is normalise | U = Y1 . W | the loss kernel on (U, Y2, Yneg) | dY1 = dU . W^T |
        normalisation backward; `bilinear_wgrad()` then queues dW = Y1^T . dU with the step's other weight gradients.
        loss_fn='infonce' runs that schedule with its own head (without bilinear weights U is Y1 itself and the two
        contractions with W drop out); ids = (ids1, ids2), the pairs' int32 node ids on the device, is its false-negative mask
        (None: nothing masked; the other losses ignore it) and d_z_all=None asks for the forward only."""
        e = self.engine
        d = z_all.d
        B = batch_size
        n_rows = 2 * B + n_neg
        if self.loss_fn == 'infonce':
            return self._infonce(z_all, outputs_all, B, n_neg, n_rows, scale, loss_rows, rr_rows, aff_all, d_z_all, epilogue, ids)
        slabs = e.ws_f32((self.name, "neg_slabs", B, n_neg, d), ((B + 3) // 4) * n_neg * d)
        # `epilogue`: (loss_out, accumulate, mrr_out, [(counter, delta)] * 3) -- the step's loss / mrr means and device
        # counters ride in the second launch
        common = dict(B=B, n_neg=n_neg, neg_weight=self.neg_sample_weights, margin=self.margin, scale=scale,
                      loss_rows=loss_rows, rr_rows=rr_rows, aff_all=aff_all, neg_slabs=slabs, epilogue=epilogue, stream=e.stream)
        if not self.bilinear_weights:
            ops.linkpred_loss_fwd_bwd(self.loss_fn, z_all, dX=d_z_all, Y=outputs_all, **common)
            return
        W = self.vars['weights']
        inv = e.ws_f32((self.name, "inv_norm", n_rows), n_rows)
        U = e.ws_mat((self.name, "bilinear_u"), B, d)
        dU = e.ws_mat((self.name, "bilinear_du"), B, d)
        dY = e.ws_mat((self.name, "d_outputs_all"), n_rows, d)
        y1 = outputs_all.rows_slice(0, B)
        ops.l2norm_fwd(z_all.rows_slice(0, n_rows), n_rows, outputs_all, inv, stream=e.stream)
        ops.gemm(False, False, B, d, d, y1, W.value, U, stream=e.stream)                      # neg_cost's inputs1 . W (:90)
        ops.linkpred_loss_fwd_bwd(self.loss_fn, outputs_all, U=U, dU=dU, dX=dY, **common)
        ops.dense_dgrad(dU, 0, d, B, W.value, dY.rows_slice(0, B), stream=e.stream)          # dY1 = dU . W^T
        ops.l2norm_bwd(dY, outputs_all, inv, n_rows, d_z_all, stream=e.stream)
        self._bilinear_saved = (y1, dU, B)

    def _infonce(self, z_all, outputs_all, B, n_neg, n_rows, scale, loss_rows, rr_rows, aff_all, d_z_all, epilogue, ids):
        """l2norm_fwd | U = Y1 . W (bilinear) | gs_linkpred_infonce_fwd_bwd | dY1 = dU . W^T (bilinear) | l2norm_bwd."""
        e = self.engine
        d = z_all.d
        train = d_z_all is not None
        inv = e.ws_f32((self.name, "inv_norm", n_rows), n_rows)
        stats = e.ws_f32((self.name, "infonce_ws", B, n_neg, d), ops.linkpred_infonce_ws_floats(B, d, n_neg))
        y1 = outputs_all.rows_slice(0, B)
        ops.l2norm_fwd(z_all.rows_slice(0, n_rows), n_rows, outputs_all, inv, stream=e.stream)
        U = y1
        if self.bilinear_weights:
            W = self.vars['weights']
            U = e.ws_mat((self.name, "bilinear_u"), B, d)
            ops.gemm(False, False, B, d, d, y1, W.value, U, stream=e.stream)
        dY = dU = None
        if train:
            dY = e.ws_mat((self.name, "d_outputs_all"), n_rows, d)
            # without W the left operand IS Y1: its gradient goes straight to the first B rows of dY
            dU = e.ws_mat((self.name, "bilinear_du"), B, d) if self.bilinear_weights else dY.rows_slice(0, B)
        ops.linkpred_infonce_fwd_bwd(outputs_all, U, B, n_neg, self.temperature, scale, loss_rows, rr_rows, aff_all, stats,
                                     dX=dY, dU=dU, ids=ids, epilogue=epilogue, stream=e.stream)
        if not train:
            return
        if self.bilinear_weights:
            ops.dense_dgrad(dU, 0, d, B, self.vars['weights'].value, dY.rows_slice(0, B), stream=e.stream)
            self._bilinear_saved = (y1, dU, B)
        ops.l2norm_bwd(dY, outputs_all, inv, n_rows, d_z_all, stream=e.stream)

    def bilinear_wgrad(self):
        """Queue dW = Y1^T . dU of the last loss_and_grads_fused call (between Engine.begin_backward and finish_backward)."""
        if not self.bilinear_weights:
            return
        y1, dU, B = self._bilinear_saved
        self.engine.wgrad(self.vars['weights'], y1, None, dU, 0, B)
