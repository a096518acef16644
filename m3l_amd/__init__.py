"""m3l_amd — MI355X-native (gfx950, hand-written HIP) masked multimodal auto-encoder training step: a drop-in for the
VTT / VTMAE representation path of Leonhard111/M3L (models/pretrain_models.py, models/VTT.py) and nothing else."""
from ._lib import LIB_PATH, M3LError  # noqa: F401
from .pretrain_models import VTMAE, VTT, Transformer  # noqa: F401
from .dino_vtt import VTT as DinoVTT  # noqa: F401  (reference: models/VTT.py — a second class that is also called VTT)
from .dino import DINOHead, DINOLoss, KoLeoLoss, iBOTPatchLoss, update_moving_average  # noqa: F401  (reference: tactile_ssl dino_head.py, dino_loss.py, koleo_loss.py, utils/ema.py)
from .vtdino import VTDINO  # noqa: F401  (reference: models/vtdino.py)
from .optim import CosineWDSchedule, DinoAdamW, WarmupCosineScheduler  # noqa: F401  (reference: trainer.py:305-342, tactile_ssl/model/custom_scheduler.py)
from .pretrain_utils import vt_load  # noqa: F401
from .dinov2 import DinoV2Frozen  # noqa: F401  (reference: torch.hub dinov2_vits14_reg, train_dino_cat_mae.py:29)
from .fusion import DinoCatMAEExtractor, MAEExtractor  # noqa: F401  (reference: MAEExtractor, models/pretrain_models.py:788-841 and models/pretrain_models_dino_cat_mae.py:793-904)
from .sac_ensemble import SACEnsembleHead, SACEnsembleParams  # noqa: F401  (SB3's SACPolicy(n_critics=N), sac_mae_policy.py:62; REDQ's subset-min target and mean-Q actor loss)
from .tqc import TQCHead, TQCParams  # noqa: F401  (sb3_contrib.TQC's policy behind the extractor: quantile critics, truncated pooled targets, the quantile-Huber loss)
from .td3 import TD3Head, TD3Params  # noqa: F401  (SB3's TD3Policy behind the extractor: the deterministic actor of DDPG, TD3 and DrQ-v2 over the ensemble's critics)
from .sac import SACHead  # noqa: F401  (reference: the head's part of models/sac_mae.py:303-366; SB3's SACPolicy behind the extractor)
from .policy import ActorCriticHead  # noqa: F401  (reference: the policy head and loss of models/ppo_mae.py:280-340; SB3's ActorCriticPolicy behind the extractor)
from .rollout import DeviceRolloutBuffer, LoadedObs, RolloutBatch  # noqa: F401  (reference: the rollout's way to the device, models/ppo_dino_cat_mae.py:25-71,268-332; SB3's DictRolloutBuffer)
from .replay import DeviceReplayBuffer, NStepReplayBatch, PrioritizedReplayBatch, ReplayBatch, per_refresh, per_sample, per_update  # noqa: F401  (reference: `self.replay_buffer.sample` and what follows it, models/sac_mae.py:240,253-260; SB3's DictReplayBuffer)

__all__ = ["VTT", "VTMAE", "Transformer", "DinoVTT", "VTDINO", "DINOHead", "DINOLoss", "KoLeoLoss", "iBOTPatchLoss", "update_moving_average", "DinoAdamW", "WarmupCosineScheduler", "CosineWDSchedule", "DinoV2Frozen", "DinoCatMAEExtractor", "MAEExtractor", "ActorCriticHead", "SACHead", "SACEnsembleHead", "SACEnsembleParams", "TQCHead", "TQCParams", "TD3Head", "TD3Params", "DeviceRolloutBuffer", "LoadedObs", "RolloutBatch", "DeviceReplayBuffer", "ReplayBatch", "NStepReplayBatch", "PrioritizedReplayBatch", "per_refresh", "per_sample", "per_update", "vt_load", "M3LError", "LIB_PATH"]
