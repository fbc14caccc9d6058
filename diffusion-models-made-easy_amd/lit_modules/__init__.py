from .ddpm import LitDDPM  # noqa: F401
from .ddim import LitDDIM  # noqa: F401
from .iddpm import LitIDDPM  # noqa: F401
from .cfg import LitClassifierFreeDDPM  # noqa: F401
from .distill import LitDistill  # noqa: F401
from .consistency import LitConsistency  # noqa: F401
