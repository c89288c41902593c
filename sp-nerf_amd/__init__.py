"""spnerf_amd — MI355X (gfx950) volumetric render path for SP-NeRF.

Drop-in for the reference's render surface:

* ``render_rays``, ``sample_pdf``, ``sample_3sigma``, ``compute_samples_around_depth``,
  ``GenerateGuidedSamples``  (modules/rendering.py)
* ``SPNeRF``, ``inference``, ``Mapping``, ``Siren``, ``sine_init``, ``first_layer_sine_init``
  (models/spnerf.py) and ``load_model`` (models/__init__.py)

all backed by the hand-written HIP kernels of ``libspnerf_amd.so`` (C ABI:
include/spnerf_amd.h).  Importing the package does not touch the GPU; the first compute
call loads the library and raises if it is missing or if tensors are on the CPU.
"""
from .rendering import (GenerateGuidedSamples, compute_samples_around_depth, render_rays, sample_3sigma,  # noqa: F401
                        sample_pdf, stratified)
from . import optim  # noqa: F401  (optim.Adam: the library's one-launch Adam step)
from . import dsm  # noqa: F401  (DSM extraction: satellite_scene.py:475-568 on the GPU)
from .rng import PhiloxRandom, ReplayRandom, TorchRandom, current_random_source, random_source, set_random_source  # noqa: F401
from .spnerf import (SPNeRF, Mapping, Siren, first_layer_sine_init, inference, inference_rays, run_mlp,  # noqa: F401
                     sine_init)
from . import view  # noqa: F401  (whole views: image products and the validation scores on the GPU)
from .view import render_image, view_loss, view_metrics  # noqa: F401
from . import relight  # noqa: F401  (a view under K sun directions from one pass over its geometry)
from .relight import relight_image  # noqa: F401
from . import ortho  # noqa: F401  (a DSM and true-ortho products on a UTM ground grid)
from .ortho import GroundGrid, ortho_rays, relight_ortho, render_ortho  # noqa: F401
from . import shadow  # noqa: F401  (geometric shadows of a ground-grid DSM under K sun directions)
from .shadow import cast_shadows, shadow_agreement  # noqa: F401
from . import rectify  # noqa: F401  (camera images on the ground grid over a DSM: projection, sampling, occlusion, mosaic)
from .rectify import orthorectify  # noqa: F401
from . import sweep  # noqa: F401  (a photo-consistency DSM from the camera images alone: grey planes, window ZNCC, the pick)
from .sweep import plane_sweep  # noqa: F401
from . import sgm  # noqa: F401  (the sweep's score volume regularised across cells: semi-global aggregation, then the pick)
from .sgm import smooth_sweep  # noqa: F401
from . import occlusion  # noqa: F401  (the sweep's views gated by a visibility floor from a prior DSM, and the two-pass chain)
from .occlusion import gate_plane, refine_sweep, visibility_floor, visible_sweep  # noqa: F401
from . import surface  # noqa: F401  (the sweep around a base surface instead of horizontal planes, and the coarse-to-fine chain)
from .surface import coarsen, pyramid_sweep, surface_grey, surface_lift, surface_sweep, upsample_dsm  # noqa: F401
from . import dsm_view  # noqa: F401  (a ground-grid DSM seen from a camera: the cast, rasters read at the hits, depth priors)
from .dsm_view import dsm_depth_priors, hit_ecef, normalised_depth, sample_at, view_dsm  # noqa: F401
from . import clean  # noqa: F401  (a swept DSM cleaned: the speckle filter, the median, the hole fill, and the two-pass sweep over a cleaned prior)
from .clean import bootstrap_sweep, clean_dsm, fill_holes, median_dsm, speckle_filter  # noqa: F401
from . import confidence  # noqa: F401  (how unambiguous a pick is, from the score volume: margins, peak counts, curvature, the maximum-likelihood measure)
from .confidence import sparsification, volume_confidence  # noqa: F401
from . import image  # noqa: F401  (image scores: the reference's metrics.ssim in fp64 on the GPU)
from .image import ssim  # noqa: F401
from . import perceptual  # noqa: F401  (LPIPS with AlexNet features: eval.py:128-135 on the GPU)
from .perceptual import LpipsWeights, lpips  # noqa: F401
from . import losses  # noqa: F401  (modules/metrics.py, and the fused training losses)
from .losses import FusedRenderLoss, FusedTrainLoss  # noqa: F401
from . import dataset  # noqa: F401  (depth priors, semantic labels and scene.loc: satellite_scene.py on the GPU)
from . import train  # noqa: F401  (main.py's training step and schedule: one HIP-graph replay per step)
from .train import EpochPlan, Trainer, make_plan  # noqa: F401

__version__ = "0.1.0"


def load_model(args):
    """models/__init__.py:4-16."""
    if args.model == "sp-nerf":
        return SPNeRF(num_sem_classes=args.num_sem_classes, s_embedding_factor=args.s_embedding_factor,
                      layers=args.fc_layers, feat=args.fc_units, mapping=args.mapping,
                      t_embedding_dims=args.t_embbeding_tau, beta=args.beta, sem=args.sem,
                      precision=getattr(args, "mlp_precision", "fp32"))
    raise ValueError(f'model {args.model} is not valid')
