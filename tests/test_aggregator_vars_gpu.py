"""-m gpu pin of the variables every aggregator class creates: name, shape and weight-decay flag IN CREATION ORDER.

The order fixes two things no other test sees directly: which initialiser draw each variable receives (inits draws from one
seeded stream) and where the variable lies in the engine's flat parameter buffer (Engine.finalize lays them out in list order;
checkpoints and the grouped optimizer launch follow it).  The table was written down from the classes as they stood before their
constructors were merged into _SageBase._init_sage.  No kernel is launched: the engines are never finalized.
"""
import re

import pytest

from graphsage_amd import aggregators as agg
from graphsage_amd import engine as eng
from graphsage_amd import inits

pytestmark = pytest.mark.gpu

# (class, concat, bias) -> [(name without the layer's serial number, rows, cols, decay)], input_dim 8, output_dim 4, "small"
EXPECTED = \
{('GCNAggregator', False, False): [('gcnaggregator_vars/neigh_weights', 8, 4, True)],
 ('GCNAggregator', False, True): [('gcnaggregator_vars/neigh_weights', 8, 4, True),
                                  ('gcnaggregator_vars/bias', 1, 4, True)],
 ('GCNAggregator', True, False): [('gcnaggregator_vars/neigh_weights', 8, 4, True)],
 ('GCNAggregator', True, True): [('gcnaggregator_vars/neigh_weights', 8, 4, True), ('gcnaggregator_vars/bias', 1, 4, True)],
 ('MaxPoolingAggregator', False, False): [('dense_vars/weights', 8, 512, False),
                                          ('dense_vars/bias', 1, 512, False),
                                          ('maxpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                          ('maxpoolingaggregator_vars/self_weights', 8, 4, True)],
 ('MaxPoolingAggregator', False, True): [('dense_vars/weights', 8, 512, False),
                                         ('dense_vars/bias', 1, 512, False),
                                         ('maxpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                         ('maxpoolingaggregator_vars/self_weights', 8, 4, True),
                                         ('maxpoolingaggregator_vars/bias', 1, 4, True)],
 ('MaxPoolingAggregator', True, False): [('dense_vars/weights', 8, 512, False),
                                         ('dense_vars/bias', 1, 512, False),
                                         ('maxpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                         ('maxpoolingaggregator_vars/self_weights', 8, 4, True)],
 ('MaxPoolingAggregator', True, True): [('dense_vars/weights', 8, 512, False),
                                        ('dense_vars/bias', 1, 512, False),
                                        ('maxpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                        ('maxpoolingaggregator_vars/self_weights', 8, 4, True),
                                        ('maxpoolingaggregator_vars/bias', 1, 8, True)],
 ('MeanAggregator', False, False): [('meanaggregator_vars/neigh_weights', 8, 4, True),
                                    ('meanaggregator_vars/self_weights', 8, 4, True)],
 ('MeanAggregator', False, True): [('meanaggregator_vars/neigh_weights', 8, 4, True),
                                   ('meanaggregator_vars/self_weights', 8, 4, True),
                                   ('meanaggregator_vars/bias', 1, 4, True)],
 ('MeanAggregator', True, False): [('meanaggregator_vars/neigh_weights', 8, 4, True),
                                   ('meanaggregator_vars/self_weights', 8, 4, True)],
 ('MeanAggregator', True, True): [('meanaggregator_vars/neigh_weights', 8, 4, True),
                                  ('meanaggregator_vars/self_weights', 8, 4, True),
                                  ('meanaggregator_vars/bias', 1, 8, True)],
 ('MeanPoolingAggregator', False, False): [('dense_vars/weights', 8, 512, False),
                                           ('dense_vars/bias', 1, 512, False),
                                           ('meanpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                           ('meanpoolingaggregator_vars/self_weights', 8, 4, True)],
 ('MeanPoolingAggregator', False, True): [('dense_vars/weights', 8, 512, False),
                                          ('dense_vars/bias', 1, 512, False),
                                          ('meanpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                          ('meanpoolingaggregator_vars/self_weights', 8, 4, True),
                                          ('meanpoolingaggregator_vars/bias', 1, 4, True)],
 ('MeanPoolingAggregator', True, False): [('dense_vars/weights', 8, 512, False),
                                          ('dense_vars/bias', 1, 512, False),
                                          ('meanpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                          ('meanpoolingaggregator_vars/self_weights', 8, 4, True)],
 ('MeanPoolingAggregator', True, True): [('dense_vars/weights', 8, 512, False),
                                         ('dense_vars/bias', 1, 512, False),
                                         ('meanpoolingaggregator_vars/neigh_weights', 512, 4, True),
                                         ('meanpoolingaggregator_vars/self_weights', 8, 4, True),
                                         ('meanpoolingaggregator_vars/bias', 1, 8, True)],
 ('SeqAggregator', False, False): [('seqaggregator_vars/neigh_weights', 128, 4, True),
                                   ('seqaggregator_vars/self_weights', 8, 4, True),
                                   ('seqaggregator/rnn/basic_lstm_cell/kernel_x', 8, 512, False),
                                   ('seqaggregator/rnn/basic_lstm_cell/kernel_h', 128, 512, False),
                                   ('seqaggregator/rnn/basic_lstm_cell/bias', 1, 512, False)],
 ('SeqAggregator', False, True): [('seqaggregator_vars/neigh_weights', 128, 4, True),
                                  ('seqaggregator_vars/self_weights', 8, 4, True),
                                  ('seqaggregator_vars/bias', 1, 4, True),
                                  ('seqaggregator/rnn/basic_lstm_cell/kernel_x', 8, 512, False),
                                  ('seqaggregator/rnn/basic_lstm_cell/kernel_h', 128, 512, False),
                                  ('seqaggregator/rnn/basic_lstm_cell/bias', 1, 512, False)],
 ('SeqAggregator', True, False): [('seqaggregator_vars/neigh_weights', 128, 4, True),
                                  ('seqaggregator_vars/self_weights', 8, 4, True),
                                  ('seqaggregator/rnn/basic_lstm_cell/kernel_x', 8, 512, False),
                                  ('seqaggregator/rnn/basic_lstm_cell/kernel_h', 128, 512, False),
                                  ('seqaggregator/rnn/basic_lstm_cell/bias', 1, 512, False)],
 ('TwoMaxLayerPoolingAggregator', False, False): [('dense_vars/weights', 8, 512, False),
                                                  ('dense_vars/bias', 1, 512, False),
                                                  ('dense_vars/weights', 512, 256, False),
                                                  ('dense_vars/bias', 1, 256, False),
                                                  ('twomaxlayerpoolingaggregator_vars/neigh_weights', 256, 4, True),
                                                  ('twomaxlayerpoolingaggregator_vars/self_weights', 8, 4, True)],
 ('TwoMaxLayerPoolingAggregator', False, True): [('dense_vars/weights', 8, 512, False),
                                                 ('dense_vars/bias', 1, 512, False),
                                                 ('dense_vars/weights', 512, 256, False),
                                                 ('dense_vars/bias', 1, 256, False),
                                                 ('twomaxlayerpoolingaggregator_vars/neigh_weights', 256, 4, True),
                                                 ('twomaxlayerpoolingaggregator_vars/self_weights', 8, 4, True),
                                                 ('twomaxlayerpoolingaggregator_vars/bias', 1, 4, True)],
 ('TwoMaxLayerPoolingAggregator', True, False): [('dense_vars/weights', 8, 512, False),
                                                 ('dense_vars/bias', 1, 512, False),
                                                 ('dense_vars/weights', 512, 256, False),
                                                 ('dense_vars/bias', 1, 256, False),
                                                 ('twomaxlayerpoolingaggregator_vars/neigh_weights', 256, 4, True),
                                                 ('twomaxlayerpoolingaggregator_vars/self_weights', 8, 4, True)],
 ('TwoMaxLayerPoolingAggregator', True, True): [('dense_vars/weights', 8, 512, False),
                                                ('dense_vars/bias', 1, 512, False),
                                                ('dense_vars/weights', 512, 256, False),
                                                ('dense_vars/bias', 1, 256, False),
                                                ('twomaxlayerpoolingaggregator_vars/neigh_weights', 256, 4, True),
                                                ('twomaxlayerpoolingaggregator_vars/self_weights', 8, 4, True),
                                                ('twomaxlayerpoolingaggregator_vars/bias', 1, 8, True)]}


@pytest.mark.parametrize("cls_name,concat,bias", sorted(EXPECTED))
def test_variable_creation_order(dev, cls_name, concat, bias):
    eng.reset_engine()
    inits.set_seed(7)
    e = eng.get_engine()
    kwargs = {} if cls_name in ("MeanAggregator", "GCNAggregator") else {"model_size": "small"}
    getattr(agg, cls_name)(8, 4, concat=concat, bias=bias, **kwargs)
    got = [(re.sub(r"_\d+", "", v.name, count=1), v.rows, v.cols, v.decay) for v in e.variables]
    assert got == EXPECTED[(cls_name, concat, bias)]


def test_every_class_and_flag_combination_is_pinned():
    classes = ["MeanAggregator", "GCNAggregator", "MaxPoolingAggregator", "MeanPoolingAggregator", "SeqAggregator",
               "TwoMaxLayerPoolingAggregator"]
    want = {(c, concat, bias) for c in classes for concat in (False, True) for bias in (False, True)}
    want.discard(("SeqAggregator", True, True))      # refused by the constructor: the bias has output_dim entries
    assert set(EXPECTED) == want
