from .warmup import WarmupLR  # noqa: F401
from .decay import LinearDecayLR  # noqa: F401
