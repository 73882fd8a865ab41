"""Rollout-collection side of PPO on the GPU: `NativeActorCritic`, `NativeActorCriticRecurrent`
(LSTM / GRU memory in front of each MLP), `compute_returns`, `collect_rollout`; teacher-student distillation: `NativeStudentTeacher`, `NativeStudentTeacherRecurrent`,
`collect_distillation`, `obs_history_step`; the terrain estimator (depth image -> ray distances): `NativeTerrainEstimator`, `NativeConvEncoder`, `collect_estimation`;
the training side: `NativePPO` (`PPO.update` on the device, include/lgtrain.h), `NativeRecurrentPPO` (the same through the LSTM / GRU memories,
include/lgtrain_recurrent.h), `NativeSymmetricPPO` (`NativePPO` with `symmetry_cfg`: symmetric data augmentation and the mirror loss,
include/lgtrain_symmetry.h; `signed_permutation_tables` turns a `data_augmentation_func` into its tables), `NativeDistillation` (`Distillation.update`, include/lgdistill.h), `NativeRecurrentDistillation` (the same for the
recurrent student: truncated BPTT through its memory, include/lgdistill_recurrent.h) and `NativeEstimatorDistillation`
(`EstimatorDistillation.update`: the terrain estimator's conv backward, truncated BPTT and Adam, include/lgestimator_train.h); the runner:
`NativeOnPolicyRunner` (rsl_rl's `OnPolicyRunner` surface over these pieces), `NativeEmpiricalNormalization` (`empirical_normalization` on the device) and
`collect_rollout_tracked` / `EpisodeTracker` (the collection with the normaliser and the episode bookkeeping between its launches, include/lgrunner.h;
with privileged critic observations -- two observation streams, two normalisers, `NativeEmpiricalNormalization.step_pair` --
include/lgrunner_privileged.h); `NativeDistillationRunner` (the same surface for `Distillation`: the teacher from the PPO runner's checkpoint, two
normalisers) over `collect_distillation_tracked` (include/lgrunner_distill.h); `NativeTerrainEstimatorRunner` (rsl_rl's `TerrainEstimatorRunner` surface:
`learn`, `play`, the reference's checkpoints) over `collect_estimation_driven` -- the estimation collection with the pretrained policy as its driver --
and `estimation_errors` (include/lgrunner_estimator.h); `TerrainEstimatorTorch`, the torch restatement that seeds it."""
from .policy import (NativeActorCritic, NativeActorCriticRecurrent, NativeMemory, NativeMLP,          # noqa: F401
                     NativeStudentTeacher, NativeStudentTeacherRecurrent)
from .storage import compute_returns                      # noqa: F401
from .collector import (EpisodeTracker, collect_distillation, collect_distillation_tracked, collect_estimation, collect_rollout,          # noqa: F401
                        collect_rollout_tracked, obs_history_step)
from .estimator import NativeConvEncoder, NativeTerrainEstimator, parse_estimator_state          # noqa: F401
from .ppo import NativePPO          # noqa: F401
from .ppo_recurrent import NativeRecurrentPPO          # noqa: F401
from .ppo_symmetry import NativeSymmetricPPO          # noqa: F401
from .symmetry import signed_permutation_tables          # noqa: F401
from .distillation import NativeDistillation          # noqa: F401
from .distillation_recurrent import NativeRecurrentDistillation          # noqa: F401
from .estimator_distillation import NativeEstimatorDistillation          # noqa: F401
from .normalizer import NativeEmpiricalNormalization          # noqa: F401
from .runner import NativeOnPolicyRunner          # noqa: F401
from .distillation_runner import NativeDistillationRunner          # noqa: F401
from .sensors import SensorRig          # noqa: F401
from .estimator_torch import TerrainEstimatorTorch          # noqa: F401
from .estimator_runner import NativeTerrainEstimatorRunner, collect_estimation_driven, estimation_errors          # noqa: F401
