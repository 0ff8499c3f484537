"""rl-aerial-manipulator_amd -- MI355X-native batched replacement for the one hot path of
LahiruCooray/rl-aerial-manipulator: `WaypointQuadEnv.step()/reset()` + the `simul_files`
rigid-body integrator.  HIP kernels behind a C ABI (include/amenv.h);
this package is the thin host-side mirror of the reference's Python interface.

The directory name carries a hyphen (project convention), so import it through the alias
module at the repo root:  `import rl_aerial_manipulator_amd as amd`.
"""
from . import _lib, sharding
from ._lib import AmenvError
from . import vec_env
from .gpu_env import GpuWaypointEnv
from .randomization import DynamicsRandomization
from .rotor_lag import RotorLag
from .rate_control import RateControl
from .rotor_failure import RotorFailure
from .sensor_noise import SensorNoise
from .action_delay import ActionDelay
from .action_history import ActionHistory
from .vec_env import GpuVecEnv
from .obs_norm import GpuVecNormalize, ObsNormalizer
from .reward_norm import RewardNormalizer
from . import baselines, ppo
from .baselines import MinSnapTrajectory, PidController, PidWaypointPolicy
from .ppo import PPO, ActorCritic, KlAdaptiveLr, evaluate_policy, reduce_evaluation, clone_pid_policy

__all__ = ["GpuWaypointEnv", "DynamicsRandomization", "RotorLag", "SensorNoise", "ActionDelay", "ActionHistory", "RateControl", "RotorFailure", "GpuVecEnv", "GpuVecNormalize", "ObsNormalizer", "RewardNormalizer", "PPO", "ActorCritic", "KlAdaptiveLr", "evaluate_policy", "reduce_evaluation", "clone_pid_policy", "ppo", "baselines", "PidController", "MinSnapTrajectory", "PidWaypointPolicy", "vec_env", "AmenvError", "_lib", "sharding"]
