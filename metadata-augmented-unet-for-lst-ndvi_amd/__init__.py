"""MI355X-native (gfx950) implementation of the Metadata-Augmented U-Net hot path.

Importable as ``mau_amd`` through the alias module at the repository root (the directory name
contains hyphens).  Importing loads ``libmau_hip.so`` and fails loudly when it is missing.
"""
from . import _lib                      # noqa: F401  (raises if the HIP library is absent)
from .model import (MetadataEncoder, TemporalEncoder, UrbanPredictor, UrbanPredictor_unet,  # noqa: F401
                    UrbanPredictor_unetpp, VGGBlock)
from .losses import (compute_all_loss, compute_loss_l1_grad_ssim, compute_loss_mse, compute_loss_mse_gradient,   # noqa: F401
                     gradient_loss)
from .inference import GraphedInference  # noqa: F401
from .train_graph import GraphedTrainStep  # noqa: F401
from .optim import SGD, Adam, AdamW  # noqa: F401
from .functional import mark_params_updated  # noqa: F401
from . import data                      # noqa: F401  (input pipeline: compact tiles, device-side one-hot + RandomFlip)


def __getattr__(name):
    # ``mau_amd.sensitivity`` (metadata sensitivity sweeps), ``mau_amd.ground_truth`` (their dataset counterpart), ``mau_amd.evaluate``
    # (test-split evaluation), ``mau_amd.scenario`` (scenario sessions of the app) and ``mau_amd.dataset_metrics`` (the dataset
    # survey) and ``mau_amd.compare`` (model comparison sessions) are also command lines, ``python -m mau_amd.sensitivity`` /
    # ``.ground_truth`` / ``.evaluate`` / ``.scenario`` / ``.dataset_metrics`` / ``.compare``, and so are ``mau_amd.dataset_build`` (raw
    # tiles -> the processed dataset) and ``mau_amd.region`` (region forecasts: windows gathered and blended on the device) and
    # ``mau_amd.statistics`` (paired tests of several checkpoints in one pass over the test split): they are imported on first use,
    # so that running one as a script does not find it in sys.modules already
    import importlib
    if name in ("sensitivity", "ground_truth", "evaluate", "scenario", "dataset_metrics", "compare", "dataset_build", "region", "statistics"):
        return importlib.import_module("." + name, __name__)
    if name in ("ScenarioSession", "ScenarioResult"):
        return getattr(importlib.import_module(".scenario", __name__), name)
    if name in ("ComparisonSession", "ComparisonResult"):
        return getattr(importlib.import_module(".compare", __name__), name)
    if name in ("RegionSession", "RegionResult"):
        return getattr(importlib.import_module(".region", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["UrbanPredictor", "UrbanPredictor_unet", "UrbanPredictor_unetpp", "VGGBlock", "MetadataEncoder",
           "TemporalEncoder", "compute_loss_mse", "compute_loss_mse_gradient", "compute_loss_l1_grad_ssim", "compute_all_loss", "gradient_loss",
           "GraphedInference", "GraphedTrainStep", "AdamW", "Adam", "SGD", "mark_params_updated", "sensitivity", "ground_truth", "evaluate", "scenario",
           "dataset_metrics", "ScenarioSession", "ScenarioResult", "compare", "ComparisonSession", "ComparisonResult", "dataset_build",
           "region", "RegionSession", "RegionResult", "statistics"]
