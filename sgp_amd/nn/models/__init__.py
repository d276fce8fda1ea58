from .esn_model import ESNModel
from .sgp_model import OnlineSGPModel, SGPInputEncoder, SGPModel
from .gated_gn_model import GatedGraphNetwork, GatedGraphNetworkMLPModel, GatedGraphNetworkModel
from .rnn_model import FCRNNModel, RNNModel
from .rnn_imputer import BiRNNImputerModel, RNNImputerModel
from .dcrnn_model import DCRNNModel
from .grin_model import GRINModel
from .gwnet_model import GraphWaveNetModel
from .sgp_online import SGPOnlineModel
from .transformer_model import TransformerModel
from ...metrics import masked_mae        # the loss every model trains with lives with the other losses

__all__ = ["SGPInputEncoder", "SGPModel", "OnlineSGPModel", "ESNModel", "masked_mae", "GatedGraphNetwork",
           "GatedGraphNetworkModel", "GatedGraphNetworkMLPModel", "RNNModel", "FCRNNModel", "DCRNNModel",
           "GraphWaveNetModel", "SGPOnlineModel", "RNNImputerModel", "BiRNNImputerModel", "GRINModel",
           "TransformerModel"]
