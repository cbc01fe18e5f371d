"""MI355X-native batched convex-MPC locomotion stepper (hot path of silvery107/rl-mpc-locomotion).

Only what the path needs lives here: ``csrc/`` (HIP kernels + the C-ABI library), the host-side
mirror of the reference's plugin interface (``mpc_osqp`` shim, batched stepper), the constant tables
and the synthetic workload generator.  See DESIGN.md.
"""
from .rl_task import BatchedRLTask, TaskConfig, TaskPostPhysics  # noqa: E402,F401

_PPO = ("ActorCritic", "RolloutStorage", "PPO", "PPOConfig", "PPOTrainer")
_EPISODE = ("EpisodeStats",)
_OBS_NORM = ("ObsNormalizer", "fold_normalizer")
_CURRICULUM = ("TerrainCurriculum",)
_HEIGHT_SCAN = ("HeightScan",)
_DOMAIN_RAND = ("DomainRand", "NoiseSpec", "PushSpec")
_EPISODE_TERMS = ("EpisodeTerms", "CommandCurriculumSpec")
_PRIVILEGED_OBS = ("PrivilegedObs",)
_PLANT_RAND = ("PlantRand", "PlantSpec")
_RECURRENT = ("ActorCriticRecurrent", "Memory", "RecurrentConfig")
_REWARD_SHAPING = ("RewardShaping", "ShapingSpec")
_FRICTION = ("Friction", "FrictionSpec")
_CONTACT_TERMS = ("ContactTerms", "ContactSpec")

__all__ = ["layout", "quadruped", "gait", "synthetic", "toy_sim", "rl_task", "BatchedRLTask", "TaskConfig", "TaskPostPhysics", "ppo", *_PPO, "episode", *_EPISODE, "obs_norm", *_OBS_NORM, "curriculum", *_CURRICULUM, "height_scan", *_HEIGHT_SCAN, "domain_rand", *_DOMAIN_RAND, "episode_terms", *_EPISODE_TERMS, "privileged_obs", *_PRIVILEGED_OBS, "plant_rand", *_PLANT_RAND, "recurrent", *_RECURRENT, "reward_shaping", *_REWARD_SHAPING, "friction", *_FRICTION, "contact_terms", *_CONTACT_TERMS]


def __getattr__(name):
    # the PPO classes subclass torch.nn.Module: ppo.py imports torch, which this package otherwise leaves to the first call that needs it
    if name in _PPO:
        from . import ppo
        return getattr(ppo, name)
    if name in _EPISODE:
        from . import episode
        return getattr(episode, name)
    if name in _OBS_NORM:
        from . import obs_norm
        return getattr(obs_norm, name)
    if name in _CURRICULUM:
        from . import curriculum
        return getattr(curriculum, name)
    if name in _HEIGHT_SCAN:
        from . import height_scan
        return getattr(height_scan, name)
    if name in _DOMAIN_RAND:
        from . import domain_rand
        return getattr(domain_rand, name)
    if name in _EPISODE_TERMS:
        from . import episode_terms
        return getattr(episode_terms, name)
    if name in _PRIVILEGED_OBS:
        from . import privileged_obs
        return getattr(privileged_obs, name)
    if name in _PLANT_RAND:
        from . import plant_rand
        return getattr(plant_rand, name)
    if name in _RECURRENT:
        from . import recurrent
        return getattr(recurrent, name)
    if name in _REWARD_SHAPING:
        from . import reward_shaping
        return getattr(reward_shaping, name)
    if name in _FRICTION:
        from . import friction
        return getattr(friction, name)
    if name in _CONTACT_TERMS:
        from . import contact_terms
        return getattr(contact_terms, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
