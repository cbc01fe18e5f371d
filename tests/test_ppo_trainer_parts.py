"""PPOTrainer's tables as host logic (rl_mpc_locomotion_amd.ppo: _riders / _read_riders, _checkpoint_parts / _save_parts / _load_parts) and the one call
form of both actor-critics, without a GPU: the record assembled from stand-in riders of the real lengths against one written out by hand from the
options' own ``record`` functions and the ``S_*`` indices, with ``float(i)`` at flat position i so that a slice shifted by one shows; the checkpoint
table over every presence combination of its four parts on either side, against the rules and the error texts of the trainer before the tables."""
import itertools
from types import SimpleNamespace

import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import episode as EP, episode_terms as ET, ppo as P
from rl_mpc_locomotion_amd.curriculum import TerrainCurriculum
from rl_mpc_locomotion_amd.recurrent import ActorCriticRecurrent

EPISODES_LEN = EP.S_TOTALS + EP.S_STRIDE * 2             # EpisodeStats(num_groups=1).summary: the overall block and one group
HOST_LR = 0.125                                          # what the torch backend's record carries: the host's value, not read from the device


class _Alg:
    def __init__(self, lr_device):
        self.lr_device, self.learning_rate, self.synced = lr_device, HOST_LR, []

    def sync_learning_rate(self, lr):
        self.synced.append(lr)
        self.learning_rate = float(lr)


class _Summarised:
    """A curriculum or the episode terms: ``summary()`` counts its calls, ``record`` is the real class's."""

    def __init__(self, values, log, **members):
        self.values, self.log, self.reads = values, log, 0
        self.__dict__.update(members)

    def summary(self):
        self.reads += 1
        self.log.append("summary")
        return self.values

    def new_window(self):
        self.log.append("new_window")


def _trainer(lr, num_types, terms):
    """A stand-in with the riders' members whose summaries, laid end to end, hold float(i) at position i; and the flat list."""
    lengths = [5] + [1] * lr + [EPISODES_LEN] + ([2 + 2 * num_types] if num_types else []) + ([ET.SUMMARY_LEN] if terms else [])
    flat = torch.arange(sum(lengths), dtype=torch.float64)
    parts = iter(flat.split(lengths))
    log = []
    t = SimpleNamespace(_scalars=next(parts), alg=_Alg(next(parts) if lr else None), episode_stats=SimpleNamespace(summary=next(parts)), log=log)
    t.curriculum = _Summarised(next(parts), log, record=TerrainCurriculum.record, num_types=num_types) if num_types else None
    t.episode_terms = _Summarised(next(parts), log, record=ET.EpisodeTerms.record) if terms else None
    return t, flat.tolist()


@pytest.mark.parametrize("lr,num_types,terms", [(lr, k, terms) for lr in (0, 1) for k in (0, 1, 3) for terms in (False, True)])
def test_the_record_is_each_riders_own_slice_of_one_read(lr, num_types, terms, monkeypatch):
    t, flat = _trainer(lr, num_types, terms)
    riders = P._riders(t)
    if terms:                                            # replaced on the instance after the riders were built: called through the object
        zero = t.episode_terms.new_window
        t.episode_terms.new_window = lambda: (t.log.append("hook"), zero())
    cats, cat = [], torch.cat
    monkeypatch.setattr(P.torch, "cat", lambda tensors: (cats.append(len(tensors)), t.log.append("read"), cat(tensors))[2])
    record = P._read_riders(riders)
    # by hand
    want = dict(mean_reward=0.0, done_rate=1.0, value_loss=2.0, surrogate_loss=3.0, mean_noise_std=4.0, learning_rate=5.0 if lr else HOST_LR)
    ep = flat[5 + lr:5 + lr + EPISODES_LEN]
    want.update(mean_episode_return=ep[EP.S_MEAN_RETURN], mean_episode_length=ep[EP.S_MEAN_LENGTH], episodes_in_window=int(ep[EP.S_WINDOW_COUNT]),
                episodes_finished=int(ep[EP.S_EPISODES]), timeouts_in_window=int(ep[EP.S_WINDOW_TIMEOUTS]))
    after = 5 + lr + EPISODES_LEN
    if num_types:
        want.update(TerrainCurriculum.record(flat[after:after + 2 + 2 * num_types], num_types))
        assert want["mean_terrain_level"] == after + 1 and want["terrain_level_by_type"] == [float(after + 2 + num_types + k) for k in range(num_types)]
        after += 2 + 2 * num_types
    if terms:
        want["episode_terms"] = ET.EpisodeTerms.record(flat[after:after + ET.SUMMARY_LEN])
        assert want["episode_terms"]["min_command_x"] == after + ET.S_LO and want["episode_terms"]["command_widenings"] == after + ET.S_WIDENINGS
        after += ET.SUMMARY_LEN
    assert after == len(flat)
    assert record == want and list(record) == list(want)                   # the entries and their order
    assert all(type(record[k]) is type(want[k]) for k in want)
    # one read of everything that rides, after every summary and before the new window; the learning rate follows the device's value only
    assert cats == [2 + lr + bool(num_types) + terms]
    assert t.alg.synced == ([5.0] if lr else []) and t.alg.learning_rate == (5.0 if lr else HOST_LR)
    assert t.log == ["summary"] * (bool(num_types) + terms) + ["read"] + ["hook", "new_window"] * terms
    assert all(o.reads == 1 for o in (t.curriculum, t.episode_terms) if o is not None)


class _Holder:
    """Anything with ``state_dict`` / ``load_state_dict``; ``tick`` is what the episode terms restore."""

    def __init__(self, name, loads):
        self.name, self.loads, self.tick = name, loads, 0

    def state_dict(self):
        return {"of": self.name, "tick": 7}

    def load_state_dict(self, sd):
        self.loads.append((self.name, sd["of"]))
        self.tick = sd["tick"]


NAMES = ("obs_norm", "critic_obs_norm", "episode_terms", "plant_rand")
KEYS = tuple(n + "_state_dict" for n in NAMES)
# the texts of PPOTrainer.load before the table
UNEXPECTED_OBS_NORM = "the checkpoint was written with observation normalisation and this trainer has none"
MISSING_OBS_NORM = "this trainer normalises observations and the checkpoint carries no obs_norm_state_dict"
MISSING_CRITIC_NORM = "this trainer normalises the critic's rows and the checkpoint carries no critic_obs_norm_state_dict"


def _owner(have, clock):
    loads = []
    env = SimpleNamespace(common_step_counter=3) if clock else SimpleNamespace()
    t = SimpleNamespace(env=env, obs="held", loads=loads, **{n: _Holder(n, loads) if h else None for n, h in zip(NAMES, have)})
    return t


def test_the_checkpoint_table_saves_what_the_trainer_has():
    for have in itertools.product((False, True), repeat=4):
        t, ck = _owner(have, True), {"model_state_dict": 0}
        P._save_parts(P._checkpoint_parts(t), ck)
        assert list(ck) == ["model_state_dict"] + [k for k, h in zip(KEYS, have) if h]
        assert all(ck[k] == {"of": n, "tick": 7} for n, k, h in zip(NAMES, KEYS, have) if h) and t.loads == [] and t.obs == "held"


def test_the_checkpoint_table_loads_by_the_three_rules():
    seen = set()
    for have, held, clock in itertools.product(itertools.product((False, True), repeat=4), itertools.product((False, True), repeat=4), (False, True)):
        t = _owner(have, clock)
        ck = {k: {"of": "checkpoint's " + n, "tick": 11} for n, k, h in zip(NAMES, KEYS, held) if h}
        before = dict(ck)
        load = lambda: P._load_parts(P._checkpoint_parts(t), ck)
        loaded = lambda names: [(n, "checkpoint's " + n) for n in names]
        if have[0] != held[0]:                           # obs_norm: the two sides must match; nothing has been loaded
            with pytest.raises(ValueError) as e:
                load()
            assert str(e.value) == (MISSING_OBS_NORM if have[0] else UNEXPECTED_OBS_NORM) and t.loads == [] and t.obs == "held"
            seen.add(str(e.value))
        elif have[1] and not held[1]:                    # critic_obs_norm: required when the trainer has it; the observations' statistics came first
            with pytest.raises(ValueError) as e:
                load()
            assert str(e.value) == MISSING_CRITIC_NORM and t.loads == loaded(NAMES[:1] if have[0] else ()) and t.obs == (None if have[0] else "held")
            seen.add(str(e.value))
        else:                                            # episode_terms, plant_rand: restored when both sides have them; a key nobody takes is ignored
            load()
            assert t.loads == loaded(n for n, a, b in zip(NAMES, have, held) if a and b)
            assert t.obs == (None if have[0] else "held")                  # (normalised with the statistics before the load)
            terms_loaded = have[2] and held[2]
            assert getattr(t.env, "common_step_counter", None) == ((11 if terms_loaded else 3) if clock else None)
            assert not terms_loaded or t.episode_terms.tick == 11
        assert ck == before
    assert seen == {MISSING_OBS_NORM, UNEXPECTED_OBS_NORM, MISSING_CRITIC_NORM}


def test_both_actor_critics_take_one_call_form():
    ff, rec = P.ActorCritic(48, 12, (32,), (32,)), ActorCriticRecurrent(48, 12, (32,), (32,), rnn_hidden_size=16)
    assert ff.hidden_sizes is None and rec.hidden_sizes == (16, 16) and ff.reset_memory() is None
    assert P.RolloutStorage(4, 2, "cpu").hidden_slot(1) is None and set(P.RolloutStorage(4, 2, "cpu", hidden=rec.hidden_sizes).hidden_slot(1)) == {"h_a", "c_a", "h_c", "c_c"}
    obs, flag = torch.zeros((4, 48)), torch.zeros(4, dtype=torch.long)
    for call in (lambda: ff.act(obs, 1, 0, reset=flag), lambda: ff.act(obs, 1, 0, saved={}), lambda: ff.evaluate(obs, reset=flag),
                 lambda: ff.act_inference(obs, reset=flag)):
        with pytest.raises(ValueError, match="feed-forward actor-critic, which has no memory"):      # (before anything asks for the device)
            call()
