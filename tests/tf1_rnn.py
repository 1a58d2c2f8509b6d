"""`tf.contrib.rnn.BasicLSTMCell` and `tf.nn.dynamic_rnn` for the TF1 stand-in of tests/tf1_shim -- TEST INFRASTRUCTURE ONLY.

`install(tf)` puts them on the stand-in at run time (tests/golden/make_ref_seq_fixtures.py calls it before the reference's
SeqAggregator, aggregators.py:363-449, is built); the stand-in's own module is not changed.  Semantics follow TF 1.x's
published documentation of the two (tensorflow 1.8, which the reference pins):

  BasicLSTMCell(H): variables created on the cell's first call, once per cell object -- `kernel` [input_depth + H, 4H] with
      get_variable's default initializer (glorot_uniform) and `bias` [4H] of zeros, under `<scope>/rnn/basic_lstm_cell/`.
      [i, j, f, o] = split([x_t, h_{t-1}] . kernel + bias, 4);  c_t = c_{t-1} sigmoid(f + forget_bias) + sigmoid(i) tanh(j);
      h_t = tanh(c_t) sigmoid(o); forget_bias = 1.0 is added at call time, not stored in the bias.
  dynamic_rnn(cell, x [B, T, D], sequence_length=L, initial_state): for t >= L_b the state is copied through and the output
      is zero; returns (outputs [B, T, H], (c, h)).

The recurrence is a masked torch loop, so torch.autograd gives the BPTT that tf.gradients would; it computes in the
stand-in's current precision (tf.shim.real: float32, or float64 for the twin run).  TF learns the input depth from static
shapes; the stand-in's reshape carries none, so it is read from the reshape's target shape, whose last entry the reference
always gives as a Python int (models.py:323-325).
"""
import numpy as np
import torch


def _static_depth(tf, t):
    if t.static_shape is not None and isinstance(t.static_shape[-1], int):
        return t.static_shape[-1]
    if len(t.args) == 2 and isinstance(t.args[1], (list, tuple)) and isinstance(t.args[1][-1], (int, np.integer)):
        return int(t.args[1][-1])
    raise ValueError("tf1_rnn: the input depth of dynamic_rnn is not known statically")


def install(tf):
    shim = tf.shim

    class BasicLSTMCell(object):
        def __init__(self, num_units, forget_bias=1.0, state_is_tuple=True, activation=None, reuse=None, name=None):
            assert state_is_tuple and activation is None
            self._num_units = int(num_units)
            self._forget_bias = float(forget_bias)
            self.kernel = self.bias = None

        @property
        def output_size(self):
            return self._num_units

        def zero_state(self, batch_size, dtype):
            H = self._num_units
            z = tf.Tensor(lambda b: torch.zeros(int(b), H, dtype=shim.real), (batch_size,), static_shape=[None, H])
            return (z, z)                                   # LSTMStateTuple(c, h)

        def build(self, input_depth):
            if self.kernel is None:                         # once per cell: every later call reuses the variables
                H = self._num_units
                with tf.variable_scope("rnn"), tf.variable_scope("basic_lstm_cell"):
                    self.kernel = tf.get_variable("kernel", shape=[input_depth + H, 4 * H])
                    self.bias = tf.Variable(np.zeros(4 * H, np.float32), name="bias")

    def dynamic_rnn(cell, inputs, sequence_length=None, initial_state=None, dtype=None, time_major=False, scope=None,
                    **kw):
        assert not time_major
        cell.build(_static_depth(tf, inputs))
        H, fb = cell._num_units, cell._forget_bias

        def run(x, length, state, kernel, bias):
            x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(shim.real)
            B, T = x.shape[0], x.shape[1]
            if state is None:
                c = h = torch.zeros(B, H, dtype=x.dtype)
            else:
                c, h = state
            L = torch.full((B,), T, dtype=torch.int64) if length is None else torch.as_tensor(length).to(torch.int64)
            outs = []
            for t in range(T):
                z = torch.cat([x[:, t], h], dim=1) @ kernel + bias
                i, j, f, o = torch.split(z, H, dim=1)
                new_c = c * torch.sigmoid(f + fb) + torch.sigmoid(i) * torch.tanh(j)
                new_h = torch.tanh(new_c) * torch.sigmoid(o)
                m = (t < L).unsqueeze(1)
                c = torch.where(m, new_c, c)
                h = torch.where(m, new_h, h)
                outs.append(torch.where(m, new_h, torch.zeros_like(new_h)))
            return torch.stack(outs, dim=1), (c, h)

        node = tf.Tensor(run, (inputs, sequence_length, initial_state, cell.kernel, cell.bias))
        outputs = tf.Tensor(lambda r: r[0], (node,), static_shape=[None, None, H])
        state = (tf.Tensor(lambda r: r[1][0], (node,), static_shape=[None, H]),
                 tf.Tensor(lambda r: r[1][1], (node,), static_shape=[None, H]))
        return outputs, state

    tf.contrib.rnn.BasicLSTMCell = BasicLSTMCell
    tf.nn.dynamic_rnn = dynamic_rnn
    return tf
