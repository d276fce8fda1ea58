from .gated_gn import GatedGraphNetwork, edge_plan

__all__ = ["GatedGraphNetwork", "edge_plan"]
