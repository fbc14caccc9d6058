from .ddpm import DDPM, HistoryRecorder, history_ordinals  # noqa: F401
from .ddim import DDIM, GeneralizedDDIM  # noqa: F401
from .iddpm import IDDPM  # noqa: F401
from .dpm_solver import DPMSolverPP  # noqa: F401
from .repaint import RePaint, PaintChainRunner, repaint_levels, repaint_rows  # noqa: F401
from .ilvr import ILVR, LikeChainRunner, ilvr_rows, lowpass_matrix  # noqa: F401
from .ddnm import DDNM, RestoreChainRunner, ddnm_rows  # noqa: F401
from .dps import DPS, PosteriorChainRunner, SeparableOperator, dps_rows  # noqa: F401
from .pfode import ProbabilityFlow, FlowChainRunner, LikelihoodChainRunner, LogLikelihood, pf_rows, pf_grid  # noqa: F401
from .distill import ProgressiveDistillation, distill_rows, distill_grid  # noqa: F401
from .consistency import ConsistencyDistillation, ConsistencySampler, consistency_rows, consistency_sampler_rows, consistency_grid  # noqa: F401
from .analytic import AnalyticDPM, analytic_rows, moment_schedule  # noqa: F401
