from .gated_gn import GatedGraphNetwork, edge_plan
from .rnn import RNN
from .diff_conv import DiffConv, DiffusionPlan, diffusion_plan
from .dcrnn import DCRNN, DCRNNCell
from .grin import GRIL, SpatialDecoder
from .gwnet import GatedTemporalConv, Norm, SpatialConvOrderK, TemporalConvNet
from .attention import (LayerNorm, MultiHeadAttention, PositionalEncoding, SpatioTemporalTransformerLayer, Transformer,
                        TransformerLayer)

__all__ = ["GatedGraphNetwork", "edge_plan", "RNN", "DiffConv", "DiffusionPlan", "diffusion_plan", "DCRNN", "DCRNNCell",
           "GatedTemporalConv", "TemporalConvNet", "SpatialConvOrderK", "Norm", "GRIL", "SpatialDecoder",
           "PositionalEncoding", "LayerNorm", "MultiHeadAttention", "TransformerLayer", "SpatioTemporalTransformerLayer",
           "Transformer"]
