from .esn_model import ESNModel
from .sgp_model import OnlineSGPModel, SGPInputEncoder, SGPModel, masked_mae
from .gated_gn_model import GatedGraphNetwork, GatedGraphNetworkMLPModel, GatedGraphNetworkModel

__all__ = ["SGPInputEncoder", "SGPModel", "OnlineSGPModel", "ESNModel", "masked_mae", "GatedGraphNetwork",
           "GatedGraphNetworkModel", "GatedGraphNetworkMLPModel"]
