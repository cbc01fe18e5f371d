"""rsl_rl v1.0.2's act, storage and returns restated in plain torch by their published formulas (rsl_rl's source is not in the reference tree):
what tests/test_ppo.py and tests/test_ppo_gpu.py compare the package's arithmetic with.  Every function works in the dtype of its inputs, so the same
text gives the float32 loop (the bar for bit-identity) and its float64 evaluation (for the float32-vs-float64 gap that bounds the rest)."""
import torch


def log_prob(mean, std, actions):
    """ActorCritic.get_actions_log_prob: Normal(mean, mean * 0. + std).log_prob(actions).sum(dim=-1)"""
    return torch.distributions.Normal(mean, mean * 0. + std).log_prob(actions).sum(dim=-1)


def act(actor, critic, std, obs, eps):
    """ActorCritic.act + evaluate with the noise given: Normal.sample() is mean + std * eps.  Returns actions, log-prob, values, mean, sigma."""
    with torch.no_grad():
        mean = actor(obs)
        sigma = mean * 0. + std
        actions = mean + sigma * eps
        return actions, log_prob(mean, std, actions), critic(obs), mean, sigma


def bootstrap(rew, values, time_outs, gamma):
    """PPO.process_env_step: rewards += gamma * squeeze(values * time_outs.unsqueeze(1), 1).  rew [N], values [N,1], time_outs [N]."""
    rewards = rew.clone()
    rewards += gamma * torch.squeeze(values * time_outs.to(values.dtype).unsqueeze(1), 1)
    return rewards


def compute_returns(rewards, dones, values, last_values, gamma, lam):
    """RolloutStorage.compute_returns on [T,N,1] tensors (last_values [N,1]).  Returns (returns, advantages before the normalisation, advantages)."""
    T = rewards.shape[0]
    returns = torch.zeros_like(rewards)
    advantage = 0
    for step in reversed(range(T)):
        next_values = last_values if step == T - 1 else values[step + 1]
        next_is_not_terminal = 1.0 - dones[step]
        delta = rewards[step] + next_is_not_terminal * gamma * next_values - values[step]
        advantage = delta + next_is_not_terminal * gamma * lam * advantage
        returns[step] = advantage + values[step]
    raw = returns - values
    return returns, raw, normalise(raw)


def normalise(advantages):
    return (advantages - advantages.mean()) / (advantages.std() + 1e-8)


def rollout(T, n, seed, done_rate=0.10, timeout_rate=0.05):
    """Random float32 storage contents [T,N,1] with the cases the tests name: a done on the last step, a time-out on the first.  Time-outs are
    dones too (the task resets an environment whose episode has run out).  Returns rew [T,N], reset, time_outs [T,N] int64, values [T,N,1], last [N,1]."""
    g = torch.Generator().manual_seed(seed)
    rew = torch.rand((T, n), generator=g) * 0.02
    values = torch.randn((T, n, 1), generator=g) * 0.5 + 1.0
    last = torch.randn((n, 1), generator=g) * 0.5 + 1.0
    time_outs = (torch.rand((T, n), generator=g) < timeout_rate).long()
    reset = ((torch.rand((T, n), generator=g) < done_rate).long() | time_outs)
    reset[T - 1, 0] = 1
    time_outs[0, n - 1] = 1
    reset[0, n - 1] = 1
    return rew, reset, time_outs, values, last
