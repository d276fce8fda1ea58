from .gated_gn import GatedGraphNetwork, edge_plan
from .rnn import RNN
from .diff_conv import DiffConv, DiffusionPlan, diffusion_plan
from .dcrnn import DCRNN, DCRNNCell

__all__ = ["GatedGraphNetwork", "edge_plan", "RNN", "DiffConv", "DiffusionPlan", "diffusion_plan", "DCRNN", "DCRNNCell"]
