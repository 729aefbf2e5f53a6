"""xfmr_rec_amd -- MI355X-native training path of yxtay/transformer-recommenders.

Host-side mirror of the reference's ``xfmr_rec.models`` / ``xfmr_rec.losses`` / ``xfmr_rec.trainer``
interfaces over hand-written gfx950 HIP kernels (``libxfmr_hip.so``, C ABI in ``include/xfmr_hip.h``).
"""

from .checkpoint import parse_max_time, read_checkpoint, reference_checkpoint_options, write_checkpoint  # noqa: F401
from .evalset import DeviceEvalSet, EvalPlan, SampledEvalSet, plan_eval_rows, shard_eval_plan  # noqa: F401
from .losses import LOSS_CLASSES, EmbedLoss, LossConfig, LossType  # noqa: F401
from .models import ModelConfig, RecommenderModel  # noqa: F401
from .trainer import EarlyStopping, FusedAdamW, GraphedStep, LightningConfig, RecommenderLightningModule, Trainer  # noqa: F401

__all__ = [
    "LOSS_CLASSES", "EmbedLoss", "LossConfig", "LossType", "ModelConfig", "RecommenderModel",
    "DeviceEvalSet", "SampledEvalSet", "EarlyStopping", "EvalPlan", "plan_eval_rows", "shard_eval_plan", "FusedAdamW", "GraphedStep", "LightningConfig", "RecommenderLightningModule", "Trainer",
    "parse_max_time", "read_checkpoint", "reference_checkpoint_options", "write_checkpoint",
]
