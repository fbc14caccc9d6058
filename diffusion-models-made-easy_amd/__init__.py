"""dmme_amd: MI355X-native DDPM/DDIM/IDDPM denoiser path behind the reference's `dmme` surface.

Importable as `dmme_amd` (the directory name `diffusion-models-made-easy_amd` is not a
valid Python identifier; `dmme_amd/__init__.py` at the repository root aliases it)."""

__version__ = "0.1.0"

from . import _lib  # noqa: F401
from .common.noise import gaussian, gaussian_like, uniform_int, pad  # noqa: F401
from .common.norm import denorm, norm  # noqa: F401
from .common.vis import make_history, save_png  # noqa: F401
from . import models, diffusion_models, equations, lit_modules, lr_scheduler, data_modules, callbacks  # noqa: F401
from .diffusion_models import HistoryRecorder, history_ordinals  # noqa: F401
from .callbacks import GenerateImage  # noqa: F401
from .data_modules import CIFAR10  # noqa: F401
from .diffusion_models import DDPM, DDIM, IDDPM, GeneralizedDDIM, DPMSolverPP  # noqa: F401
from .diffusion_models import RePaint, PaintChainRunner, repaint_levels, repaint_rows  # noqa: F401
from .diffusion_models import ILVR, LikeChainRunner, ilvr_rows, lowpass_matrix  # noqa: F401
from .diffusion_models import DDNM, RestoreChainRunner, ddnm_rows  # noqa: F401
from .diffusion_models import DPS, PosteriorChainRunner, SeparableOperator, dps_rows  # noqa: F401
from .diffusion_models import ProbabilityFlow, FlowChainRunner, LikelihoodChainRunner, LogLikelihood, pf_rows, pf_grid  # noqa: F401
from .diffusion_models import ProgressiveDistillation, distill_rows, distill_grid  # noqa: F401
from .diffusion_models import ConsistencyDistillation, ConsistencySampler, consistency_rows, consistency_sampler_rows, consistency_grid  # noqa: F401
from .diffusion_models import AnalyticDPM, analytic_rows, moment_schedule  # noqa: F401
from .lit_modules import LitDDPM, LitDDIM, LitIDDPM, LitClassifierFreeDDPM, LitDistill, LitConsistency  # noqa: F401
from .lr_scheduler import LinearDecayLR  # noqa: F401
from .models.ddpm import UNet  # noqa: F401
from .models.cond import ConditionalUNet  # noqa: F401
from . import guidance  # noqa: F401
from .guidance import EncoderClassifier, ClassifierGuidedDDPM, ClassifierGuidedDDIM, classifier_loss  # noqa: F401
from .guidance import ClassifierFreeDDPM, ClassifierFreeDDIM, ClassifierFreeDPMSolver  # noqa: F401

__all__ = ["gaussian", "gaussian_like", "uniform_int", "pad", "denorm", "norm", "UNet", "DDPM", "DDIM", "LitDDPM", "LitDDIM", "IDDPM", "LitIDDPM", "CIFAR10", "GeneralizedDDIM",
           "ConditionalUNet", "ClassifierFreeDDPM", "ClassifierFreeDDIM", "LitClassifierFreeDDPM", "DPMSolverPP", "ClassifierFreeDPMSolver",
           "RePaint", "PaintChainRunner", "repaint_levels", "repaint_rows", "ILVR", "LikeChainRunner", "ilvr_rows", "lowpass_matrix", "make_history", "save_png", "HistoryRecorder", "history_ordinals", "GenerateImage",
           "ProgressiveDistillation", "distill_rows", "distill_grid", "LitDistill", "LinearDecayLR", "DDNM", "RestoreChainRunner", "ddnm_rows", "DPS", "PosteriorChainRunner", "SeparableOperator", "dps_rows",
           "ConsistencyDistillation", "ConsistencySampler", "consistency_rows", "consistency_sampler_rows", "consistency_grid", "LitConsistency",
           "ProbabilityFlow", "FlowChainRunner", "LikelihoodChainRunner", "LogLikelihood", "pf_rows", "pf_grid",
           "AnalyticDPM", "analytic_rows", "moment_schedule"]
