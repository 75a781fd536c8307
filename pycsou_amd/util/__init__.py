from .misc import is_range_broadcastable, range_broadcast_shape, peaks  # noqa: F401
from .stats import P2Algorithm  # noqa: F401
