"""A deployed recurrent weight policy restated in torch float64: one tick and a roll with resets -- the memory's LSTM step (tests/recurrent_ref.py's
``cell`` / ``roll``), the actor's Linear / ELU stack on h' (its ``mlp``), clamp to [-1, 1] and the affine map to MPC weights with oracle/policy_ref.py's
constants.  What tests/test_recurrent_policy.py and tests/test_recurrent_policy_gpu.py compare ``RecurrentWeightPolicy`` and its kernel against.

    h', c' = cell(x, h, c);   a = actor(h');   weights = clamp(a, -1, 1) * scale + const
"""
import torch

from oracle import policy_ref
from tests import recurrent_ref as ref

SCALE = torch.from_numpy(policy_ref.MPC_PARAM_SCALE).double()
CONST = torch.from_numpy(policy_ref.MPC_PARAM_CONST).double()
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def params(state_dict):
    """(lstm, layers) of a recurrent ``model_state_dict`` as torch tensors in the dict's dtype: memory_a's four arrays and the actor's Linear layers."""
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.startswith("actor.") and k.endswith(".weight")})
    return tuple(state_dict[f"memory_a.rnn.{k}"] for k in LSTM_KEYS), [(state_dict[f"actor.{i}.weight"], state_dict[f"actor.{i}.bias"]) for i in idx]


def head(h1, layers, scale=SCALE, const=CONST):
    """The actor on h' and the map to weights -> (raw actions, weights), float64."""
    a = ref.mlp(h1, layers)
    k = a.shape[-1]
    return a, torch.clamp(a, -1.0, 1.0) * scale[:k] + const[:k]


def tick(x, h, c, lstm, layers, reset=None, scale=SCALE, const=CONST):
    """One tick: reset [n] (non-zero: that row's state is zero before the step) or None -> (h', c', raw actions, weights), float64."""
    h, c = h.detach().double(), c.detach().double()
    if reset is not None:
        keep = (reset == 0).double().unsqueeze(1)
        h, c = h * keep, c * keep
    h1, c1 = ref.cell(x, h, c, *lstm)
    return (h1, c1) + head(h1, layers, scale, const)


def roll(xs, resets, h0, c0, lstm, layers, scale=SCALE, const=CONST):
    """T ticks: xs [T][n][I], resets [T][n] or None -> (h' [T][n][H], c' [T][n][H], raw actions [T][n][A], weights [T][n][A]), float64."""
    hs, cs, _, _ = ref.roll(xs, resets, h0, c0, lstm)
    a, w = head(hs, layers, scale, const)
    return hs, cs, a, w
