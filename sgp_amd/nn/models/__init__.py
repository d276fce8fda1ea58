from .esn_model import ESNModel
from .sgp_model import OnlineSGPModel, SGPInputEncoder, SGPModel, masked_mae

__all__ = ["SGPInputEncoder", "SGPModel", "OnlineSGPModel", "ESNModel", "masked_mae"]
