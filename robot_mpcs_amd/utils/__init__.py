from .corridor import MapCorridors

__all__ = ["MapCorridors"]
