from .boundary_metrics import BoundaryMetrics
from .sequence_metrics import FrontTrackingMetrics, RegionMetrics, TemporalMetrics
from .stream_metrics import StreamMetrics

__all__ = ["StreamMetrics", "TemporalMetrics", "RegionMetrics", "FrontTrackingMetrics", "BoundaryMetrics"]
