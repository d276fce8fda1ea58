from .iid_dataset import IIDSampler
from .sharded import ShardedEmbedding, ShardedIIDSampler
from .subgraph import SubgraphSampler, k_hop_subgraph
from .windows import WindowSampler

__all__ = ["IIDSampler", "ShardedEmbedding", "ShardedIIDSampler", "SubgraphSampler", "WindowSampler", "k_hop_subgraph"]
