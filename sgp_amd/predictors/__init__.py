from .predictor import Predictor
from .subgraph_predictor import SubgraphPredictor

__all__ = ["Predictor", "SubgraphPredictor"]
