from .predictor import Predictor
from .imputer import Imputer
from .subgraph_predictor import SubgraphPredictor

__all__ = ["Predictor", "SubgraphPredictor", "Imputer"]
