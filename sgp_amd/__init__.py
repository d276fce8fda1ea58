"""sgp_amd -- MI355X-native implementation of SGP's training-free spatiotemporal encoder
(reservoir over time + K-hop graph-shift propagation over nodes) behind the reference's own
Python surface.  Compute lives in ``csrc/libsgp_amd.so`` (hand-written HIP for gfx950); there
is no CPU fallback."""
from . import dataloader, datasets, hip
from .connectivity import (correntropy_connectivity, correntropy_similarity, dense_connectivity,
                           geographic_connectivity)
from .datamodule import AtStepSplitter, FixedIndicesSplitter, TemporalSplitter, WindowDataModule
from .datasets import WindowSampler
from .devgraph import DeviceShiftOperator
from .edgetables import EdgeTables, csr_tables, sort_plan, stable_sort_by_key
from .graph import ShiftOperator
from .nn.encoders import GESNEncoder, SGPEncoder, SGPSpatialEncoder, SGPTemporalEncoder
from .nn.reservoir import GESNLayer, GraphESN, Reservoir, ReservoirLayer
from .readout import RidgeReadout, RidgePath, closed_form_readout, ridge_solve_path
from .scalers import MinMaxScaler, RobustScaler, Scaler, StandardScaler
from .metrics import (MaskedMAE, MaskedMAPE, MaskedMRE, MaskedMSE, MetricSet, masked_loss, masked_mae, masked_mape,
                      masked_mse)
from .nn.layers import GRIL
from .nn.models import GRINModel, SGPOnlineModel
from .optim import FusedAdam
from .predictors import Imputer, Predictor, SubgraphPredictor
from .sgp_preprocessing import (preprocess_adj, preprocess_dataset, reservoir_preprocessing_,
                                sgp_spatial_embedding, sgp_spatial_support, window_spatial_embedding)
from .series import Series, aggregate, asfreq, datetime_encoded, resample
from .utils import encode_dataset, self_normalizing_activation
from .whiteness import AZWhiteness, AZWhitenessMultiTestResult, AZWhitenessTestResult, az_whiteness_test

__version__ = "0.1.0"
