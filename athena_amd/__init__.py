"""athena_amd -- MI355X-native message-passing engine behind athena's layer API.

Only the hot path lives here: the forward/backward of athena's
kipf / duvenaud / graph_nop message-passing layers as hand-written gfx950 HIP kernels behind a
C ABI (include/athena_mp.h), plus the host-side mirrors of the reference interface.
"""
from . import _capi  # noqa: F401
from .graph import DeviceGraph, duvenaud_plan_stats, graph_type  # noqa: F401
from . import geometry  # noqa: F401
from .geometry import points_grad, structures_grad, structures_grad_host  # noqa: F401
from . import batching  # noqa: F401
from .batching import Batch, Block, DeviceDataset, NeighborSampler  # noqa: F401

__all__ = ["_capi", "DeviceGraph", "duvenaud_plan_stats", "graph_type", "geometry", "points_grad", "structures_grad", "structures_grad_host", "batching", "Batch", "DeviceDataset", "Block", "NeighborSampler"]
