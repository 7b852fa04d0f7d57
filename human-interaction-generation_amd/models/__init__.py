"""Mirror of codes/models/__init__.py (single- and two-person denoiser, diffusion, evaluation classifiers)."""
from .evaluation_models import MotionConsistencyEvalModel, MotionEncoder
from .gaussian_diffusion import GaussianDiffusion
from .guidance import ClassifierFreeGuidedModel
from .interaction_transformer import MotionInteractionTransformer
from .spaced_diffusion import SpacedDiffusion, space_timesteps, space_timesteps_logsnr
from .transformer import MotionTransformer

__all__ = ["MotionTransformer", "MotionInteractionTransformer", "MotionEncoder", "MotionConsistencyEvalModel",
           "GaussianDiffusion", "SpacedDiffusion", "space_timesteps", "space_timesteps_logsnr", "ClassifierFreeGuidedModel"]
