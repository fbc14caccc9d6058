from . import ddpm, iddpm, cond  # noqa: F401
from .cond import ConditionalUNet  # noqa: F401
