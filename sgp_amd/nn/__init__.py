from . import encoders, layers, models, reservoir
