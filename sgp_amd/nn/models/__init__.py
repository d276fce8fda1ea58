from .sgp_model import OnlineSGPModel, SGPInputEncoder, SGPModel, masked_mae

__all__ = ["SGPInputEncoder", "SGPModel", "OnlineSGPModel", "masked_mae"]
