"""prediff_amd: MI355X-native (gfx950 / CDNA4) sampling engine for PreDiff latent diffusion.

Drop-in for the reference's sampling hot path behind its own Python call conventions
(SURVEY.md §8(b)): ``CuboidTransformerUNet`` / ``AutoencoderKL`` / ``LatentDiffusion`` keep the
reference constructor kwargs, forward signatures and ``state_dict`` schema; their forward passes
run hand-written HIP kernels from ``libprediff_hip.so`` (C ABI in include/prediff_hip.h).
There is no non-HIP execution path in this package.
"""
__version__ = "0.1.0"

from .autoencoder_kl import AutoencoderKL  # noqa: E402,F401
from .cuboid_transformer_unet import CuboidTransformerUNet  # noqa: E402,F401
from .latent_diffusion import LatentDiffusion  # noqa: E402,F401
from .tiled import TileGeometry, TiledLatentDiffusion  # noqa: E402,F401
from .rollout import RolloutPlan, rollout_ensemble, rollout_sample  # noqa: E402,F401
from .sevir_io import SEVIRFrontEnd  # noqa: E402,F401
from .i3d import InceptionI3d  # noqa: E402,F401
from .fvd import FrechetVideoDistance  # noqa: E402,F401
from .spectrum import SEVIRSpectralScore  # noqa: E402,F401
from .object_score import SEVIRObjectScore, label_objects  # noqa: E402,F401
from .distance_score import SEVIRDistanceScore, distance_map  # noqa: E402,F401
from .scale_score import SEVIRScaleScore, scale_energy  # noqa: E402,F401
from .extrapolation import LagrangianPersistence # noqa: E402,F401
from .steps import StochasticExtrapolation, steps_bands  # noqa: E402,F401
from .anvil import AutoregressiveExtrapolation  # noqa: E402,F401
from .probability_matching import match_cdf, probability_matched_mean, rank_frames  # noqa: E402,F401
