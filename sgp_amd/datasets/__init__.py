from .iid_dataset import IIDSampler
from .sharded import ShardedEmbedding, ShardedIIDSampler
from .subgraph import SubgraphSampler, k_hop_subgraph

__all__ = ["IIDSampler", "ShardedEmbedding", "ShardedIIDSampler", "SubgraphSampler", "k_hop_subgraph"]
