"""The per-term episode sums and the command curriculum on the MI355X (csrc/mpc_episode_terms.h, rl_mpc_locomotion_amd.episode_terms): the kernels
against the restatement of tests/episode_terms_ref.py on the crafted batch (sums, ticks, counts, ranges, window accumulators and commands EQUAL,
sentinels untouched, reruns identical), and the hooks in BatchedRLTask.step and PPOTrainer: a task with the unit is bit for bit the task without it,
the terms add up to the reward, the sums are the running float32 sums, the curriculum widens and saturates and its commands reach the observations of
the same tick, nothing reaches the host, forced resets are closed like any other, the records carry the terms."""

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, episode_terms as E, rl_task as R
from tests import episode_terms_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
SIZES = (1, 63, 64, 65, 130)           # one lane, a wave less one, a full wave, one lane into the second workgroup, a third partial one
JOIN_WRAPS = 64 * 257 + 1              # 258 block partials: the join's 256-row staging loop runs a second, partial pass
RANGES = ((-2.5, 2.5), (-1.0, 1.0), (-0.75, 0.25))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _robots(n):
    return [i % 3 for i in range(n)]


def _spec_dict(cfg, spec):
    """the restatement's view of a CommandCurriculumSpec under cfg"""
    if spec is None:
        return None
    return dict(update_every=spec.resolved(cfg)[2], max_episode_length=cfg.max_episode_length, threshold=spec.threshold,
                scale=float(np.float32(cfg.reward_scales()[0])), step=spec.step, max_curriculum=spec.max_curriculum)


def _state(et):
    return [x.cpu().numpy().copy() for x in (et.sums, et.ticks, et.counts, et.state)]


@pytest.mark.parametrize("n", SIZES + (JOIN_WRAPS,))
def test_kernels_equal_the_restatement_on_the_crafted_batch(n):
    import torch
    cfg = R.TaskConfig(command_x_range=RANGES[0], command_y_range=RANGES[1], command_yaw_range=RANGES[2], episode_length_s=1.0, seed=777)
    big = n == JOIN_WRAPS
    for with_spec in ((True,) if big else (True, False)):
        spec = E.CommandCurriculumSpec(2.0, x_range0=(-0.5, 1.0), update_every=1) if with_spec else None
        et = E.EpisodeTerms(n, cfg, command_curriculum=spec, device=DEV)
        assert et.sums.dtype == torch.float32 and et.sums.shape == (n, 6) and et.ticks.dtype == torch.int32 and et.ticks.shape == (n,)
        assert et.counts.dtype == torch.int32 and et.counts.shape == (n,) and et.ranges.dtype == torch.float64 and et.ranges.shape == (3, 2)
        assert not et.sums.any().item() and not et.ticks.any().item() and not et.counts.any().item()
        state0 = ref.state0(RANGES, (-0.5, 1.0) if with_spec else None)
        assert np.array_equal(et.state.cpu().numpy(), state0)
        state0[ref.G_WINDOW:ref.G_WINDOW + 7] = np.arange(7) * 0.125 + 3.0     # a window that already holds something
        sd = _spec_dict(cfg, spec)
        for pattern in (("everybody", "mix") if big else ref.PATTERNS):
            case = ref.crafted(n, pattern)
            ids, marked = _dev(case["ids"]), case["marked"]
            runs = []
            for _ in range(2):                                             # the same start twice: bit-identical
                et.sums.copy_(_dev(case["sums"])); et.ticks.copy_(_dev(case["ticks"])); et.counts.copy_(_dev(case["counts"])); et.state.copy_(_dev(state0))
                commands = _dev(case["commands"])
                et.close_and_resample(ids, commands, 5)
                runs.append(_state(et) + [commands.cpu().numpy()])
            assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), pattern
            want = ref.close_and_resample(case["ids"], case["sums"], case["ticks"], case["counts"], state0, case["commands"], 5, sd, cfg.seed)
            for got, w, name in zip(runs[0], want, ("sums", "ticks", "counts", "state", "commands")):
                assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), (n, pattern, with_spec, name)
            sums, ticks, counts, state, cmd = runs[0]
            assert (sums[~marked] == ref.SENTINEL_SUM).all() and (ticks[~marked] == ref.SENTINEL_TICKS).all() and (counts[~marked] == ref.SENTINEL_COUNT).all()
            assert (cmd[~marked] == ref.SENTINEL_COMMAND).all()
            assert not sums[marked].any() and not ticks[marked].any() and np.array_equal(counts[marked], case["counts"][marked] + 1)
            assert state[ref.G_WINDOW] - state0[ref.G_WINDOW] == (marked & (case["ticks"] > 0) & np.isfinite(case["sums"]).all(1)).sum()
            assert np.isfinite(state).all()
            if not with_spec:
                assert (cmd == ref.SENTINEL_COMMAND).all() and np.array_equal(state[:6], state0[:6])
            elif marked.any():
                rg = state[:6].reshape(3, 2).astype(np.float32)
                assert (cmd[marked] >= rg[:, 0]).all() and (cmd[marked] <= rg[:, 1]).all()
            if with_spec and pattern == "everybody" and n >= 63:
                assert state[:2].tolist() == [-1.0, 1.5] and state[ref.G_WIDENINGS] == 1      # the crafted tracking sums are far above the bar
        # summary and new_window on what the last pattern left
        s = et.summary()
        assert s.dtype == torch.float64 and s.shape == (E.SUMMARY_LEN,) and s.data_ptr() == et.summary().data_ptr()
        assert np.array_equal(s.cpu().numpy(), ref.summary(runs[0][3], cfg.episode_length_s))
        et.new_window()
        after = et.state.cpu().numpy()
        assert not after[ref.G_WINDOW:ref.G_WINDOW + 7].any() and np.array_equal(after[:6], runs[0][3][:6]) and after[ref.G_WIDENINGS] == runs[0][3][ref.G_WIDENINGS]


def test_accumulate_kernel_adds_the_terms_it_writes():
    import torch
    n = 130
    cfg = R.TaskConfig(rew_collision=-0.25)
    et = E.EpisodeTerms(n, cfg, device=DEV)
    rng = np.random.default_rng(4)
    root = rng.standard_normal((n, 13)).astype(np.float32)
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    root[:, 7:] *= np.float32(0.3)                                         # (velocity errors small enough for exp(-err / 0.25) to stay a normal float32)
    commands, torques = rng.uniform(-1, 1, (n, 3)).astype(np.float32), (rng.standard_normal((n, 12)) * 20).astype(np.float32)
    fell = torch.zeros(n, dtype=torch.bool, device=DEV)
    terms = torch.full((n, 6), 7.0, dtype=torch.float32, device=DEV)
    et.sums.fill_(1.5)
    et.ticks.fill_(3)
    et.accumulate(_dev(root), _dev(commands), _dev(torques), fell, terms=terms)
    t = terms.cpu().numpy()
    assert np.array_equal(et.sums.cpu().numpy(), (np.float32(1.5) + t).astype(np.float32)) and (et.ticks == 4).all().item()
    assert (t[:, 0] > 0).all() and (t[:, 1] <= 0).all() and (t[:, 4] < 0).all() and not t[:, 5].any() and not (et.counts != 0).any().item()
    et.accumulate(_dev(root), _dev(commands), _dev(torques), None)         # no contacts, no terms buffer
    assert np.array_equal(et.sums.cpu().numpy(), ((np.float32(1.5) + t).astype(np.float32) + t).astype(np.float32)) and (et.ticks == 5).all().item()


def _cfg(**kw):
    return R.TaskConfig(command_x_range=(0.2, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), **kw)


def _task(n, cfg, et=None):
    yaw = np.random.default_rng(6).uniform(-np.pi, np.pi, n)
    return R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=yaw, episode_terms=et)


def _left_to_right(terms):
    total = terms[..., 0]
    for i in range(1, 6):
        total = (total + terms[..., i]).astype(np.float32)
    return np.maximum(total, np.float32(0))


@pytest.fixture(scope="module")
def hundred_ticks():
    """A task with the unit (no curriculum spec) and one without, 130 environments, thirty ticks an episode, the same hundred actions: everything each
    returned, and of the unit per tick the terms, the ids, the sums, the ticks and the counts."""
    import torch
    n, ticks = 130, 100
    cfg = _cfg(episode_length_s=0.3, seed=4)
    et = E.EpisodeTerms(n, cfg, device=DEV)
    plain, hooked = _task(n, cfg), _task(n, cfg, et)
    assert plain.episode_terms is None and hooked.episode_terms is et
    actions = _dev(np.random.default_rng(7).uniform(-1, 1, (ticks, n, 12)).astype(np.float32))
    et.terms_buf = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    out = []
    unit = [torch.zeros((ticks, n, k), dtype=dt, device=DEV) for k, dt in ((6, torch.float32), (1, torch.int32), (6, torch.float32), (1, torch.int32), (1, torch.int32))]
    for task in (plain, hooked):
        rec = [torch.zeros((ticks, n, k), dtype=torch.float32, device=DEV) for k in (48, 1, 1, 12, 3)]
        task.reset()
        if task is hooked:
            after_reset = _state(et)
        for k in range(ticks):
            o, r, d, _ = task.step(actions[k])
            rec[0][k].copy_(o); rec[1][k, :, 0].copy_(r); rec[2][k, :, 0].copy_(d); rec[3][k].copy_(task.torques); rec[4][k].copy_(task.commands)
            if task is hooked:
                unit[0][k].copy_(et.terms_buf); unit[1][k, :, 0].copy_(task.task.reset_ids); unit[2][k].copy_(et.sums)
                unit[3][k, :, 0].copy_(et.ticks); unit[4][k, :, 0].copy_(et.counts)
        st = task.sim.get_state()
        out.append([x.cpu().numpy() for x in rec] + [st["f64"], st["i32"], task.bridge.ctl.solver_record(), task.commands.cpu().numpy()])
    terms, ids, sums, tk, counts = (x.cpu().numpy() for x in unit)
    return dict(plain=out[0], hooked=out[1], terms=terms, ids=ids[..., 0], sums=sums, ticks=tk[..., 0], counts=counts[..., 0], after_reset=after_reset,
                window=et.state.cpu().numpy(), summary=et.summary().cpu().numpy(), cfg=cfg, steps=hooked.common_step_counter, n=n)


def test_a_task_with_the_unit_is_bit_for_bit_the_task_without(hundred_ticks):
    h = hundred_ticks
    for x, y in zip(h["plain"], h["hooked"]):                              # observations, rewards, flags, torques, commands, plant state, solver record
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
    assert h["plain"][2].sum(0).min() >= 2                                 # every environment was reset at least twice
    assert h["steps"] == 101                                               # (reset() is a step)


def test_the_terms_add_up_to_the_reward_on_every_tick(hundred_ticks):
    h = hundred_ticks
    rew = h["hooked"][1][..., 0]
    assert _left_to_right(h["terms"]).tobytes() == rew.tobytes()
    assert (h["terms"][..., 0] >= 0).all() and (h["terms"][..., 0] > 0).any() and (h["terms"][..., 4] < 0).any() and (rew > 0).any()


def test_the_sums_are_the_running_float32_sums_and_the_window_their_blocked_sum(hundred_ticks):
    h = hundred_ticks
    terms, ids, n = h["terms"], h["ids"], h["n"]
    running, held, counts0, state0 = h["after_reset"]                      # reset() was tick 1: everybody marked, nothing to close, one accumulate
    assert (held == 1).all() and (counts0 == 1).all() and not state0[ref.G_WINDOW:].any()
    window, resets = np.zeros(7), np.zeros(n, np.int64)
    for k in range(terms.shape[0]):
        marked = ids[k] >= 0
        assert set(ids[k][marked].tolist()) == set(np.flatnonzero(marked).tolist())
        window = window + ref.reduce_closed(ids[k], running, held)         # what this tick's close saw: the sums as the previous tick left them
        running = np.where(marked[:, None], terms[k], (running + terms[k]).astype(np.float32))
        held = np.where(marked, 1, held + 1).astype(np.int32)
        resets += marked
        assert np.array_equal(h["sums"][k], running), k                    # environments reset this tick hold this tick's terms alone
        assert np.array_equal(h["ticks"][k], held) and np.array_equal(h["counts"][k], 1 + resets), k
    assert resets.min() >= 2
    total = h["window"][ref.G_WINDOW:ref.G_WINDOW + 7]
    assert total[0] == resets.sum() and total.tobytes() == window.tobytes()
    assert np.array_equal(h["summary"], ref.summary(h["window"], h["cfg"].episode_length_s))
    assert np.array_equal(h["window"][:6], np.array([0.2, 0.5, -0.1, 0.1, -0.3, 0.3])) and h["window"][ref.G_WIDENINGS] == 0


def _curriculum_task(n, episode_length_s=0.05, seed=11, **spec_kw):
    cfg = _cfg(episode_length_s=episode_length_s, seed=seed)
    spec = E.CommandCurriculumSpec(1.5, x_range0=(-0.5, 0.5), step=0.5, threshold=0.0, update_every=1, **spec_kw)
    et = E.EpisodeTerms(n, cfg, command_curriculum=spec, device=DEV)
    return cfg, spec, et, _task(n, cfg, et)


def test_the_curriculum_widens_saturates_and_its_commands_reach_the_same_ticks_observations():
    import torch
    n, ticks = 130, 30
    cfg, spec, et, task = _curriculum_task(n)
    sd = _spec_dict(cfg, spec)
    actions = _dev(np.random.default_rng(3).uniform(-1, 1, (ticks, n, 12)).astype(np.float32))
    et.terms_buf = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    task.reset()
    assert np.array_equal(et.ranges.cpu().numpy(), np.array([[-0.5, 0.5], [-0.1, 0.1], [-0.3, 0.3]])) and (et.counts == 1).all().item()
    c0 = task.commands.cpu().numpy()
    assert np.array_equal(c0, np.array([ref.resample(cfg.seed, r, 1, et.ranges.cpu().numpy()) for r in range(n)]))       # the first tick draws too
    prev = _state(et) + [c0]
    ranges_seen, closed_ticks = [tuple(prev[3][:2])], []
    for k in range(ticks):
        obs = task.step(actions[k])[0]
        ids, cmd, terms = task.task.reset_ids.cpu().numpy(), task.commands.cpu().numpy(), et.terms_buf.cpu().numpy()
        want = ref.close_and_resample(ids, *prev, k + 2, sd, cfg.seed)
        now = _state(et)
        marked = ids >= 0
        assert np.array_equal(now[0], (want[0] + terms).astype(np.float32)) and np.array_equal(now[1], want[1] + 1), k
        assert np.array_equal(now[2], want[2]) and now[3].tobytes() == want[3].tobytes(), k
        assert cmd.tobytes() == want[4].tobytes(), k                       # reset environments: the restatement's draws; the others: untouched
        assert np.array_equal(cmd[~marked], prev[4][~marked])
        rg = now[3][:6].reshape(3, 2).astype(np.float32)
        assert (cmd[marked] >= rg[:, 0]).all() and (cmd[marked] <= rg[:, 1]).all()
        assert np.array_equal(obs[:, 9:12].cpu().numpy(), cmd)              # unit scales, |command| < the clip: finish read the new commands
        if want[5][0] > 0:
            closed_ticks.append(k)
            assert want[5][1] > 0                                          # a positive tracking sum: threshold 0.0 fires
        if tuple(now[3][:2]) != ranges_seen[-1]:
            assert closed_ticks and closed_ticks[-1] == k
            ranges_seen.append(tuple(now[3][:2]))
        prev = now + [cmd]
    assert ranges_seen == [(-0.5, 0.5), (-1.0, 1.0), (-1.5, 1.5)] and len(closed_ticks) >= 3
    assert prev[3][ref.G_WIDENINGS] == len(closed_ticks) and task.common_step_counter == ticks + 1 == et.tick
    assert np.abs(prev[4][:, 0]).max() > 1.0                               # commands beyond the first two ranges were drawn


def test_fifty_ticks_without_a_host_synchronisation():
    import torch
    n = 130
    cfg, spec, et, task = _curriculum_task(n, episode_length_s=0.2, seed=2)
    actions = _dev(np.random.default_rng(5).uniform(-1, 1, (50, n, 12)).astype(np.float32))
    summaries = torch.zeros((50, E.SUMMARY_LEN), dtype=torch.float64, device=DEV)
    task.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")            # a torch call that waits for the device or copies to the host raises from here on
    try:
        for k in range(50):
            task.step(actions[k])
            summaries[k].copy_(et.summary())
            if k == 30:
                et.new_window()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s = summaries.cpu().numpy()
    assert (et.counts.cpu().numpy() >= 3).all() and s[30, E.S_CLOSED] >= n and s[31, E.S_CLOSED] < s[30, E.S_CLOSED]
    assert s[-1, E.S_HI] == 1.5 and s[-1, E.S_LO] == -1.5 and s[-1, E.S_WIDENINGS] >= 2 and (s[:, E.S_EPISODE_S] == 0.2).all()
    assert np.array_equal(s[-1], ref.summary(et.state.cpu().numpy(), 0.2))


def test_caller_forced_resets_are_closed_and_resampled_like_any_other():
    import torch
    n = 130
    cfg, spec, et, task = _curriculum_task(n, episode_length_s=20.0, seed=9)
    chosen = [0, 62, 64, 129]
    others = [i for i in range(n) if i not in chosen]
    actions = _dev(np.random.default_rng(3).uniform(-1, 1, (5, n, 12)).astype(np.float32))
    et.terms_buf = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    mask = torch.zeros(n, dtype=torch.long, device=DEV)
    mask[chosen] = 1
    task.reset()
    for k in range(3):
        task.step(actions[k])
    prev = _state(et) + [task.commands.cpu().numpy()]
    assert (prev[1] == 4).all() and (prev[2] == 1).all() and prev[3][ref.G_WINDOW] == 0       # nobody has reset on its own
    task.reset_buf.bitwise_or_(mask)
    task.step(actions[3])
    ids = task.task.reset_ids.cpu().numpy()
    assert np.array_equal(np.flatnonzero(ids >= 0), chosen)
    want = ref.close_and_resample(ids, *prev, 5, _spec_dict(cfg, spec), cfg.seed)
    now, cmd, terms = _state(et), task.commands.cpu().numpy(), et.terms_buf.cpu().numpy()
    assert now[3].tobytes() == want[3].tobytes() and cmd.tobytes() == want[4].tobytes() and np.array_equal(now[2], want[2])
    assert now[3][ref.G_WINDOW] == len(chosen) and now[3][:2].tolist() == [-1.0, 1.0] and now[3][ref.G_WIDENINGS] == 1
    assert np.array_equal(now[3][ref.G_WINDOW + 1:ref.G_WINDOW + 7], ref.reduce_closed(ids, prev[0], prev[1])[1:])
    assert (now[1][chosen] == 1).all() and (now[2][chosen] == 2).all() and np.array_equal(now[0][chosen], terms[chosen])
    assert (now[1][others] == 5).all() and (now[2][others] == 1).all() and np.array_equal(cmd[others], prev[4][others])
    assert np.array_equal(now[0][others], (prev[0][others] + terms[others]).astype(np.float32))
    assert not np.array_equal(cmd[chosen], prev[4][chosen])
    assert np.array_equal(cmd[chosen], np.array([ref.resample(cfg.seed, r, 2, now[3][:6].reshape(3, 2)) for r in chosen]))


KEYS = {"iter", "mean_reward", "done_rate", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate", "mean_episode_return", "mean_episode_length",
        "episodes_in_window", "episodes_finished", "timeouts_in_window"}
TERM_KEYS = {"rew_" + t for t in R.REWARD_TERMS} | {"max_command_x", "min_command_x", "command_widenings"}


@pytest.mark.parametrize("update", ["torch", "hip"])
def test_trainer_records_carry_the_terms(update, tmp_path):
    from rl_mpc_locomotion_amd import ppo as P
    n = 64
    pcfg = P.PPOConfig(num_steps_per_env=16, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    cfg, spec, et, task = _curriculum_task(n, seed=4)
    trainer = P.PPOTrainer(task, pcfg, seed=3, update=update)
    read, zero = [], et.new_window

    def new_window():                                                      # what the window held when the trainer read it
        read.append(et.summary().tolist())
        zero()
    et.new_window = new_window
    infos = trainer.learn(1)
    assert len(infos) == 1 and set(infos[0]) == KEYS | {"episode_terms"} and set(infos[0]["episode_terms"]) == TERM_KEYS
    assert len(read) == 1 and infos[0]["episode_terms"] == E.EpisodeTerms.record(read[0])
    rec, closed = infos[0]["episode_terms"], read[0][E.S_CLOSED]
    assert closed >= 2 * n and rec["rew_lin_vel_xy"] == read[0][E.S_TERMS] / closed / cfg.episode_length_s > 0 and rec["rew_torque"] < 0
    state = et.state.cpu().numpy()
    assert rec["max_command_x"] == state[1] == 1.5 and rec["min_command_x"] == state[0] == -1.5 and rec["command_widenings"] == state[ref.G_WIDENINGS] >= 2
    assert not state[ref.G_WINDOW:ref.G_WINDOW + 7].any()                  # new_window followed the read
    assert task.common_step_counter == 17 == et.tick
    # a save / load round trip restores the range, the widenings and the tick
    path = str(tmp_path / "ck.pt")
    trainer.save(path)
    cfg2, _, et2, task2 = _curriculum_task(n, seed=4)
    other = P.PPOTrainer(task2, pcfg, seed=3, update=update)
    assert et2.state_dict() == {"command_x_range": (-0.5, 0.5), "command_widenings": 0, "tick": 0}
    other.load(path)
    assert et2.state_dict() == et.state_dict() == {"command_x_range": (-1.5, 1.5), "command_widenings": int(state[ref.G_WIDENINGS]), "tick": 17}
    assert task2.common_step_counter == 17
    # the range does not move during evaluate, which still closes episodes and draws commands
    et.load_state_dict({"command_x_range": (-0.5, 0.5), "command_widenings": 0, "tick": 17})
    counts = et.counts.clone()
    trainer.evaluate(12)
    after = et.state.cpu().numpy()
    assert after[:2].tolist() == [-0.5, 0.5] and after[ref.G_WIDENINGS] == 0 and after[ref.G_WINDOW] >= n and et.curriculum_enabled is True
    assert (et.counts > counts).all().item() and task.common_step_counter == 29
    task.step(_dev(np.zeros((n, 12), np.float32)))
    for _ in range(8):                                                     # and moves again afterwards
        task.step(_dev(np.zeros((n, 12), np.float32)))
    assert et.state.cpu().numpy()[1] > 0.5
    # a plain task's record keys are unchanged
    infos = P.PPOTrainer(_task(n, cfg), pcfg, seed=3, update=update).learn(1)
    assert set(infos[0]) == KEYS


def test_argument_errors_come_back_before_any_launch():
    import torch
    n = 8
    cfg = _cfg()
    et = E.EpisodeTerms(n, cfg, command_curriculum=E.CommandCurriculumSpec(1.5, x_range0=(-0.5, 0.5)), device=DEV)
    ids, cmd = _dev(np.full(n, -1, np.int32)), _dev(np.zeros((n, 3), np.float32))
    root, tq, fell = _dev(np.zeros((n, 13), np.float32)), _dev(np.zeros((n, 12), np.float32)), torch.zeros(n, dtype=torch.bool, device=DEV)
    before = _state(et)
    for bad in (dict(reset_ids=_dev(np.full(n, -1, np.int64))), dict(reset_ids=_dev(np.full(n + 1, -1, np.int32))), dict(commands=_dev(np.zeros((n, 3), np.float64))),
                dict(commands=_dev(np.zeros((n + 1, 3), np.float32))), dict(commands=cmd.cpu())):
        with pytest.raises(ValueError):
            et.close_and_resample(**{**dict(reset_ids=ids, commands=cmd, tick=1), **bad})
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*tick"):
        et.close_and_resample(ids, cmd, -1)
    for bad in (dict(root_states=_dev(np.zeros((n, 12), np.float32))), dict(commands=_dev(np.zeros((n, 3), np.float16))), dict(torques=_dev(np.zeros((n + 1, 12), np.float32))),
                dict(fell=torch.zeros(n, dtype=torch.int32, device=DEV)), dict(fell=torch.zeros(n + 1, dtype=torch.bool, device=DEV)),
                dict(terms=torch.zeros((n, 5), dtype=torch.float32, device=DEV)), dict(terms=torch.zeros((n, 6), dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            et.accumulate(**{**dict(root_states=root, commands=cmd, torques=tq, fell=fell), **bad})
    # an object that is not bound to a handle, and null device pointers, at the C ABI
    L = E.lib()
    p, s = ids.data_ptr(), _lib.stream(et.device)
    assert L.mpc_episode_terms_close_and_resample(None, p, cmd.data_ptr(), 1, 1, s) == -1 and b"null" in L.mpc_episode_terms_last_error()
    assert L.mpc_episode_terms_close_and_resample(et._handle, None, cmd.data_ptr(), 1, 1, s) == -1
    assert L.mpc_episode_terms_close_and_resample(et._handle, p, None, 1, 1, s) == -1 and b"d_commands" in L.mpc_episode_terms_last_error()
    assert L.mpc_episode_terms_accumulate(None, root.data_ptr(), cmd.data_ptr(), tq.data_ptr(), None, None, s) == -1
    assert L.mpc_episode_terms_accumulate(et._handle, root.data_ptr(), None, tq.data_ptr(), None, None, s) == -1
    assert L.mpc_episode_terms_summary(et._handle, None, s) == -1 and L.mpc_episode_terms_summary(None, p, s) == -1
    assert L.mpc_episode_terms_new_window(None, s) == -1
    torch.cuda.synchronize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, _state(et)))       # nothing ran
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*min > max"):
        E.EpisodeTerms(n, R.TaskConfig(command_y_range=(1.0, -1.0)), device=DEV)
    with pytest.raises(ValueError, match="max_curriculum"):
        E.EpisodeTerms(n, cfg, command_curriculum=E.CommandCurriculumSpec(0.1, x_range0=(-0.5, 0.5)), device=DEV)
    with pytest.raises(ValueError, match="episode terms hold 8"):
        R.BatchedRLTask(_robots(n + 1), [TROT] * (n + 1), cfg=cfg, device=DEV, episode_terms=et)
