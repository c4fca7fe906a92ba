"""MI355X-native (gfx950) implementation of the Metadata-Augmented U-Net hot path.

Importable as ``mau_amd`` through the alias module at the repository root (the directory name
contains hyphens).  Importing loads ``libmau_hip.so`` and fails loudly when it is missing.
"""
from . import _lib                      # noqa: F401  (raises if the HIP library is absent)
from .model import (MetadataEncoder, TemporalEncoder, UrbanPredictor, UrbanPredictor_unet,  # noqa: F401
                    UrbanPredictor_unetpp, VGGBlock)
from .losses import (compute_all_loss, compute_loss_l1_grad_ssim, compute_loss_l1_grad_ssim_trained, compute_loss_mse,   # noqa: F401
                     compute_loss_mse_gradient, gradient_loss)
from .inference import GraphedInference  # noqa: F401
from .train_graph import GraphedTrainStep  # noqa: F401
from .optim import SGD, Adam, AdamW  # noqa: F401
from .functional import mark_params_updated  # noqa: F401
from . import data                      # noqa: F401  (input pipeline: compact tiles, device-side one-hot + RandomFlip)


# The tools are also command lines (``python -m mau_amd.evaluate`` ...): they are imported on first use, so that running one as a
# script does not find it in sys.modules already.
_LAZY_MODULES = ("sensitivity", "ground_truth", "evaluate", "scenario", "dataset_metrics", "compare", "dataset_build", "region", "statistics", "climate", "rank_tests", "placement", "screening")
_LAZY_CLASSES = {"ScenarioSession": "scenario", "ScenarioResult": "scenario", "ComparisonSession": "compare", "ComparisonResult": "compare",
                 "RegionSession": "region", "RegionResult": "region", "ClimateQuery": "climate",
                 "PlacementSession": "placement", "PlacementResult": "placement",
                 "ScreeningSession": "screening", "ScreeningResult": "screening"}


def __getattr__(name):
    import importlib
    if name in _LAZY_MODULES:
        return importlib.import_module("." + name, __name__)
    if name in _LAZY_CLASSES:
        return getattr(importlib.import_module("." + _LAZY_CLASSES[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["UrbanPredictor", "UrbanPredictor_unet", "UrbanPredictor_unetpp", "VGGBlock", "MetadataEncoder",
           "TemporalEncoder", "compute_loss_mse", "compute_loss_mse_gradient", "compute_loss_l1_grad_ssim", "compute_loss_l1_grad_ssim_trained", "compute_all_loss", "gradient_loss",
           "GraphedInference", "GraphedTrainStep", "AdamW", "Adam", "SGD", "mark_params_updated", *_LAZY_MODULES, *_LAZY_CLASSES]
