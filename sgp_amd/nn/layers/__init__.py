from .gated_gn import GatedGraphNetwork, edge_plan
from .rnn import RNN

__all__ = ["GatedGraphNetwork", "edge_plan", "RNN"]
