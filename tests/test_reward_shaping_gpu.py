"""The reward shaping terms on the MI355X (csrc/mpc_reward_shaping.h, rl_mpc_locomotion_amd.reward_shaping): the kernels through the C ABI against
the restatement of tests/reward_shaping_ref.py on chained crafted and random ticks (terms, reward, every state array and the window EQUAL, a rerun
identical), a plant state that blew up with the affected terms off and on and the close that follows it, feet that land above and below the air-time
target, and the hooks in BatchedRLTask.step and PPOTrainer: forty ticks on the stairs fed to the restatement tick by tick, no effect on anything
but the reward, the same stage marks, the trainer's record, the refusals.

The task's own six terms hold an expf and are taken from the device (EpisodeTerms.accumulate's ``terms``, the same rltask::reward_terms on the same
tensors); everything the unit adds is compared bit for bit (NaN for NaN)."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import episode_terms as E, reward_shaping as RS, rl_task as R
from tests import reward_shaping_ref as ref
from tests.reward_shaping_ref import F, same
from tests.test_reward_shaping import CFG, TARGET_AIR, TARGET_H, chain, restatement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
STATE = ("last_actions", "last_dof_vel", "air_time", "last_contact", "sums", "ticks", "window")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _robots(n):
    return [i % 3 for i in range(n)]


def _spec(per_second, target_h=TARGET_H):
    return RS.ShapingSpec(**dict(zip(RS.SHAPING_TERMS, per_second)), base_height_target=target_h, air_time_target=TARGET_AIR)


def _state(unit):
    return {name: getattr(unit, name).cpu().numpy().copy() for name in STATE}


def _assert_state(unit, want, what):
    got = _state(unit)
    for name, w in want.state().items():
        assert same(got[name], w), (what, name)


@pytest.mark.parametrize("n", ref.SIZES)
def test_kernels_equal_the_restatement_through_the_c_abi(n):
    import torch
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    sim = BatchedToySim(_robots(n), device=DEV)
    six = E.EpisodeTerms(n, CFG, device=DEV)                                # the device's own six task terms
    plant = sim.get_state()
    for P in (0, 1, 187):
        unit = RS.RewardShaping(n, _spec(ref.ALL_ON), device=DEV, cfg=CFG)
        assert unit.sums.shape == (n, 8) and unit.sums.dtype == torch.float32 and unit.last_contact.dtype == torch.int32 and unit.window.shape == (9,)
        assert not any(getattr(unit, name).any().item() for name in STATE)
        unit.bind(sim)
        want = restatement(n, ref.ALL_ON)
        ticks = chain(n, P, 100 * n + P)
        for t, (ids, b) in enumerate(ticks):
            plant["i32"][:, :4] = b["contact"]
            sim.set_state(plant)                                               # the contact flags the unit reads from the sim's record
            d = {k: _dev(np.ascontiguousarray(b[k], F)) for k in ("root", "dof", "actions", "commands", "torques")}
            d["dof"] = d["dof"].reshape(n * 12, 2)
            fell, reset, progress, d_ids = _dev(b["fell"]), _dev(b["reset"]), _dev(b["progress"]), _dev(ids)
            heights = None if P == 0 else _dev(b["heights"])
            task6 = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
            six.accumulate(d["root"], d["commands"], d["torques"], fell, terms=task6)
            unit.close(d_ids)
            before = {name: getattr(unit, name).clone() for name in STATE}
            out = []
            for rerun in range(2 if t == len(ticks) - 1 else 1):               # the last tick twice from the same state
                if rerun:
                    for name in STATE:
                        getattr(unit, name).copy_(before[name])
                rew, terms = torch.full((n,), 7.0, dtype=torch.float32, device=DEV), torch.full((n, 8), 7.0, dtype=torch.float32, device=DEV)
                unit.run(d["root"], d["dof"], d["actions"], d["commands"], d["torques"], fell, d_ids, reset, progress, rew, heights=heights, terms=terms)
                out.append([rew.cpu().numpy(), terms.cpu().numpy()] + list(_state(unit).values()))
            if len(out) == 2:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(*out)), (n, P, "rerun")
            S = want.close(ids)
            e_want, rew_want = want.run(b["root"], b["dof"], b["actions"], b["commands"], ids, b["reset"], b["progress"], b["contact"], b["heights"],
                                        task6.cpu().numpy())
            assert same(out[0][1], e_want), (n, P, t, "terms", np.argwhere(~(out[0][1] == e_want)))
            assert same(out[0][0], rew_want), (n, P, t, "rew")
            _assert_state(unit, want, (n, P, t))
        assert want.window[0] == 2 * (ref.marks(n, "some") >= 0).sum() and np.isfinite(want.window).all()
        summary = unit.summary().cpu().numpy()
        assert summary.tobytes() == ref.summary(want.window, CFG.episode_length_s).tobytes()
        unit.new_window()
        assert not unit.window.any().item() and unit.sums.any().item()


def _device_tick(unit, six, sim, plant, b, ids, P):
    """One close and one run on the batch b through the C ABI: (rew, terms, the device's six task terms) as numpy."""
    import torch
    n = unit.n
    plant["i32"][:, :4] = b["contact"]
    sim.set_state(plant)                                                   # the contact flags the unit reads from the sim's record
    d = {k: _dev(np.ascontiguousarray(b[k], F)) for k in ("root", "dof", "actions", "commands", "torques")}
    fell = _dev(b["fell"])
    task6 = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    six.accumulate(d["root"], d["commands"], d["torques"], fell, terms=task6)
    d_ids = _dev(ids)
    unit.close(d_ids)
    rew, terms = torch.full((n,), 7.0, dtype=torch.float32, device=DEV), torch.full((n, 8), 7.0, dtype=torch.float32, device=DEV)
    unit.run(d["root"], d["dof"].reshape(n * 12, 2), d["actions"], d["commands"], d["torques"], fell, d_ids, _dev(b["reset"]), _dev(b["progress"]), rew,
             heights=None if P == 0 else _dev(b["heights"]), terms=terms)
    return rew.cpu().numpy(), terms.cpu().numpy(), task6.cpu().numpy()


def _both(unit, want, six, sim, plant, b, ids, P, what):
    """The device and the restatement through one tick, everything EQUAL afterwards: (e, rew, task6) of the device."""
    rew, e, task6 = _device_tick(unit, six, sim, plant, b, ids, P)
    want.close(ids)
    e_want, rew_want = want.run(b["root"], b["dof"], b["actions"], b["commands"], ids, b["reset"], b["progress"], b["contact"], b["heights"], task6)
    assert same(e, e_want), (what, "terms", np.argwhere(~(e == e_want)))
    assert same(rew, rew_want), (what, "rew")
    _assert_state(unit, want, what)
    return e, rew, task6


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_state_that_blew_up_reaches_the_kernels(bad):
    """The rows of the host test, on the device: with the affected terms off nothing of them reaches the reward; with them on the reward is what fmaxf
    gives, and the close of everybody leaves out the episodes whose sums are not finite."""
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    n, P = 70, 65
    sim = BatchedToySim(_robots(n), device=DEV)
    six, plant = E.EpisodeTerms(n, CFG, device=DEV), sim.get_state()
    first, second = ref.blown_up_ticks(n, P, bad)
    none, everybody, rows = ref.marks(n, "none"), ref.marks(n, "all"), sorted(ref.BLOWN)
    for scales, live in ((ref.BLOWN_OFF, False), (ref.ALL_ON, True)):
        unit, want = RS.RewardShaping(n, _spec(scales), device=DEV, cfg=CFG), restatement(n, scales)
        unit.bind(sim)
        _both(unit, want, six, sim, plant, first, everybody, P, (live, "first"))
        e, rew, task6 = _both(unit, want, six, sim, plant, second, none, P, (live, "second"))
        sums = unit.sums.cpu().numpy()
        if not live:
            assert np.isfinite(e).all() and np.isfinite(rew[[5, 7, 9]]).all() and np.isfinite(sums).all()
            assert (e[:, [ref.ORIENTATION, ref.BASE_HEIGHT, ref.DOF_VEL, ref.DOF_ACC]] == 0).all()
        else:
            for r, i in ref.BLOWN.items():
                assert not np.isfinite(e[r, i]), (r, i)
            assert (rew[[5, 7, 9]] == (F(0) + e[:, ref.TERMINATION])[[5, 7, 9]]).all() and np.isfinite(task6[[5, 7, 9]]).all()
            assert not np.isfinite(sums[rows]).all(1).any()
        unit.close(_dev(everybody))                                            # finite_sums_n inside shaping_close_kernel
        S = want.close(everybody)
        _assert_state(unit, want, (live, "close"))
        assert S[0] == (n - len(rows) if live else n) and np.isfinite(unit.window.cpu().numpy()).all() and not unit.sums.any().item()


def test_feet_that_land_above_and_below_the_target_on_the_device():
    """air_time seeded through the tensor view: one foot lands after 0.6 s in the air and is paid, one after 0.2 s and is charged."""
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    n = 2
    sim = BatchedToySim(_robots(n), device=DEV)
    six, plant = E.EpisodeTerms(n, CFG, device=DEV), sim.get_state()
    unit, want = RS.RewardShaping(n, _spec(ref.ALL_ON), device=DEV, cfg=CFG), restatement(n, ref.ALL_ON)
    unit.bind(sim)
    rng = np.random.default_rng(3)
    _both(unit, want, six, sim, plant, dict(ref.random_tick(n, 0, rng), contact=np.zeros((n, 4), np.int32)), ref.marks(n, "all"), 0, "reset")
    b, air = ref.landing_tick(rng)
    unit.air_time.copy_(_dev(air))
    want.air_time = air.copy()
    e, _, _ = _both(unit, want, six, sim, plant, b, ref.marks(n, "none"), 0, "landing")
    dt, scale = F(ref.DT), ref.scales_of(ref.ALL_ON, ref.DT)[ref.FEET_AIR_TIME]
    assert e[0, ref.FEET_AIR_TIME] == ((F(0.6) + dt) - F(TARGET_AIR)) * scale > 0 > e[1, ref.FEET_AIR_TIME] == ((F(0.2) + dt) - F(TARGET_AIR)) * scale
    assert np.array_equal(unit.air_time.cpu().numpy(), np.array([[0, F(0.3) + dt, 0, F(0.25) + dt], [F(0.3) + dt, 0, 0, F(0.25) + dt]], F))


TICKS, FALL_TICK, FALLERS = 41, 10, (3, 40)      # the reset tick (zero actions, what reset() steps with) and forty more


@pytest.fixture(scope="module")
def stairs():
    """Three tasks of 65 robots on the stairs with the default scan, fifteen ticks an episode, the same seed, the reset tick and the same forty random actions: one with
    every shaping scale non-zero, one with all eight 0, one without the option; each with an EpisodeTerms of its own, whose terms_buf gives the device's
    six task terms.  Two robots are tipped over before the tenth of them in all three (a roll of 80 degrees in the plant's state: its next step flags the fall)."""
    import torch
    from rl_mpc_locomotion_amd.height_scan import HeightScan
    from rl_mpc_locomotion_amd.terrain import Terrain
    n = 65
    cfg = R.TaskConfig(command_x_range=(0.0, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), episode_length_s=0.15, seed=5)
    terrain = Terrain.reference_stairs()
    origin = np.stack([np.linspace(2.1, 3.8, n), np.linspace(-0.6, 1.4, n)], 1)                 # on the field: x 2 .. 3.95, y -1 .. 1.75
    yaw = np.random.default_rng(6).uniform(-0.4, 0.4, n)
    actions = _dev(np.concatenate([np.zeros((1, n, 12), F), np.random.default_rng(7).uniform(-1, 1, (TICKS - 1, n, 12)).astype(F)]))
    runs = {}
    for name, per_second in (("shaped", ref.ALL_ON), ("zero", [0.0] * 8), ("plain", None)):
        shaping = None if per_second is None else RS.RewardShaping(n, _spec(per_second), device=DEV, cfg=cfg)
        et = E.EpisodeTerms(n, cfg, device=DEV)
        et.terms_buf = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
        task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, yaw0=yaw, terrain=terrain, origin=origin, height_scan=HeightScan(n, device=DEV),
                               episode_terms=et, reward_shaping=shaping)
        assert task.reward_shaping is shaping
        shapes = dict(obs=(task.num_obs, torch.float32), rew=(1, torch.float32), reset=(1, torch.long), progress=(1, torch.long), root=(13, torch.float32),
                      dof=(24, torch.float32), actions=(12, torch.float32), commands=(3, torch.float32), torques=(12, torch.float32), ids=(1, torch.int32),
                      heights=(task.height_scan.num_points, torch.float32), contact=(4, torch.uint8), six=(6, torch.float32), fell=(1, torch.uint8))
        rec = {k: torch.zeros((TICKS, n, w), dtype=dt, device=DEV) for k, (w, dt) in shapes.items()}
        windows = []
        for k in range(TICKS):
            if k == FALL_TICK:
                st = task.sim.get_state()
                st["f64"][list(FALLERS), 3:7] = (np.sin(np.radians(40.0)), 0.0, 0.0, np.cos(np.radians(40.0)))
                task.sim.set_state(st)
            task.step(actions[k])
            contact, fell = task.sim.flags()
            for key, src in (("obs", task.obs_buf), ("rew", task.rew_buf), ("reset", task.reset_buf), ("progress", task.progress_buf), ("root", task.sim.root_states),
                             ("dof", task.sim.dof_state), ("actions", task.actions), ("commands", task.commands), ("torques", task.torques), ("ids", task.task.reset_ids),
                             ("heights", task.measured_heights), ("contact", contact), ("six", et.terms_buf), ("fell", fell)):
                rec[key][k].copy_(src.reshape(n, -1))
            if shaping is not None:
                windows.append(shaping.window.clone())
        state = None if shaping is None else _state(shaping)
        marks = []
        task.step(actions[0], mark=marks.append)                               # one more tick, for the marks
        runs[name] = dict({k: v.cpu().numpy() for k, v in rec.items()}, marks=marks, windows=[w.cpu().numpy() for w in windows],
                          state=state, points=task.height_scan.num_points)
    runs["cfg"], runs["n"] = cfg, n
    return runs


def test_forty_ticks_on_the_stairs_equal_the_restatement(stairs):
    cfg, n, h = stairs["cfg"], stairs["n"], stairs["shaped"]
    assert h["points"] == 187 and cfg.max_episode_length == 15
    want = restatement(n, ref.ALL_ON, cfg=cfg)                                # from zeros, as the unit is made: the reset tick, which marks everybody, is fed too
    assert (h["ids"][0, :, 0] == np.arange(n)).all() and not h["actions"][0].any()
    falls = timeouts = 0
    for k in range(TICKS):
        ids, reset, progress = h["ids"][k, :, 0], h["reset"][k, :, 0], h["progress"][k, :, 0]
        want.close(ids)
        assert want.window.tobytes() == h["windows"][k].tobytes(), k
        e, rew = want.run(h["root"][k], h["dof"][k], h["actions"][k], h["commands"][k], ids, reset, progress, h["contact"][k], h["heights"][k], h["six"][k])
        assert same(h["rew"][k, :, 0], rew), (k, np.argwhere(~(h["rew"][k, :, 0] == rew)))
        falls += int(((reset != 0) & ~(progress > cfg.max_episode_length)).sum())
        timeouts += int((progress > cfg.max_episode_length).sum())
        assert ((reset != 0) == ((h["fell"][k, :, 0] != 0) | (progress > cfg.max_episode_length))).all()
        if k == 0:                                                             # the reset tick: nothing closed, one tick summed, none of the history's terms paid
            assert (want.ticks == 1).all() and not want.window.any() and not want.air_time.any() and not e[:, [ref.DOF_ACC, ref.ACTION_RATE, ref.FEET_AIR_TIME]].any()
    assert falls >= 1 and timeouts >= 1                                        # falls and time-outs both occurred,
    assert all(h["fell"][FALL_TICK, r, 0] for r in FALLERS)                    # the two robots that were tipped over among them
    for name, w in want.state().items():                                       # the unit's whole state after the last tick
        assert same(h["state"][name], w), name
    assert want.window[0] >= n and (want.window[1:] != 0).all()
    assert (h["rew"] > 0).any() and (h["rew"] < 0).any()


def test_the_option_changes_the_reward_and_nothing_else(stairs):
    shaped, zero, plain = stairs["shaped"], stairs["zero"], stairs["plain"]
    for k in range(TICKS):
        for key in ("obs", "reset", "progress", "root", "dof", "torques", "commands", "ids", "heights", "contact", "six"):
            assert shaped[key][k].tobytes() == plain[key][k].tobytes() == zero[key][k].tobytes(), (k, key)
        assert (zero["rew"][k] == plain["rew"][k]).all() and zero["rew"][k].tobytes() == plain["rew"][k].tobytes(), k
    assert not np.array_equal(shaped["rew"], plain["rew"])
    assert not zero["state"]["sums"].any() and (zero["state"]["ticks"] > 0).all() and zero["state"]["window"][0] >= 2 * stairs["n"]


def test_the_stage_marks_are_the_same_list(stairs):
    assert stairs["shaped"]["marks"] == stairs["plain"]["marks"] == stairs["zero"]["marks"]
    assert len(R.STAGES) == 13 and [m for m in R.STAGES if m in stairs["shaped"]["marks"]] == stairs["shaped"]["marks"]
    assert "height_scan" in stairs["shaped"]["marks"] and "resets" in stairs["shaped"]["marks"] and len(R.REWARD_TERMS) == 6


def test_run_follows_finish_without_a_scan():
    """On the plane there is no scan: the one launch follows `finish`, base_height reads root_z, and the marks are still those of a plain task."""
    import torch
    n = 65
    cfg = R.TaskConfig(command_x_range=(0.2, 0.5), episode_length_s=0.1, seed=2)
    shaping = RS.RewardShaping(n, _spec(ref.ALL_ON), device=DEV, cfg=cfg)
    shaping.terms_buf = torch.zeros((n, 8), dtype=torch.float32, device=DEV)
    et = E.EpisodeTerms(n, cfg, device=DEV)
    et.terms_buf = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, episode_terms=et, reward_shaping=shaping)
    plain = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, episode_terms=E.EpisodeTerms(n, cfg, device=DEV))
    task.reset(), plain.reset()
    want = restatement(n, ref.ALL_ON, cfg=cfg)
    for name, value in _state(shaping).items():
        setattr(want, name, value)
    actions = _dev(np.random.default_rng(1).uniform(-1, 1, (12, n, 12)).astype(F))
    for k in range(12):
        a, b = [], []
        task.step(actions[k], mark=a.append), plain.step(actions[k], mark=b.append)
        assert a == b
        contact, _ = task.sim.flags()
        want.close(task.task.reset_ids.cpu().numpy())
        e, rew = want.run(*(x.cpu().numpy() for x in (task.sim.root_states, task.sim.dof_state, task.actions, task.commands, task.task.reset_ids, task.reset_buf,
                                                      task.progress_buf, contact)), None, et.terms_buf.cpu().numpy())
        assert same(task.rew_buf.cpu().numpy(), rew) and same(shaping.terms_buf.cpu().numpy(), e), k
        assert torch.equal(task.obs_buf, plain.obs_buf) and torch.equal(task.reset_buf, plain.reset_buf)
    d = task.sim.root_states[:, 2].cpu().numpy() - F(TARGET_H)
    assert same(shaping.terms_buf[:, ref.BASE_HEIGHT].cpu().numpy(), (d * d) * ref.scales_of(ref.ALL_ON, cfg.dt)[ref.BASE_HEIGHT])
    assert same(shaping.window.cpu().numpy(), want.window) and want.window[0] >= n


KEYS = {"iter", "mean_reward", "done_rate", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate", "mean_episode_return", "mean_episode_length",
        "episodes_in_window", "episodes_finished", "timeouts_in_window"}


@pytest.mark.parametrize("update", ["torch", "hip"])
def test_trainer_records_carry_the_shaping_terms(update):
    from rl_mpc_locomotion_amd import ppo as P
    n = 64
    pcfg = P.PPOConfig(num_steps_per_env=8, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    cfg = R.TaskConfig(command_x_range=(0.2, 0.5), episode_length_s=0.03, seed=4)
    shaping = RS.RewardShaping(n, _spec(ref.ALL_ON), device=DEV, cfg=cfg)
    task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, episode_terms=E.EpisodeTerms(n, cfg, device=DEV), reward_shaping=shaping)
    trainer = P.PPOTrainer(task, pcfg, seed=3, update=update)
    assert trainer.reward_shaping is shaping
    read, zero = [], shaping.new_window

    def new_window():                                                      # what the window held when the trainer read it
        read.append(shaping.summary().tolist())
        zero()
    shaping.new_window = new_window
    infos = trainer.learn(1)
    assert len(infos) == 1 and set(infos[0]) == KEYS | {"episode_terms", "reward_shaping"}
    rec = infos[0]["reward_shaping"]
    assert list(rec) == ["rew_" + t for t in RS.SHAPING_TERMS] and len(read) == 1 and rec == RS.RewardShaping.record(read[0])
    assert read[0][RS.S_CLOSED] >= n and read[0][RS.S_EPISODE_S] == cfg.episode_length_s and rec["rew_dof_vel"] < 0 and rec["rew_action_rate"] < 0
    assert not shaping.window.any().item()                                     # new_window followed the read


def test_argument_errors_come_back_before_any_launch():
    import ctypes as C
    import torch
    from rl_mpc_locomotion_amd import _lib
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    n = 8
    unit = RS.RewardShaping(n, _spec(ref.ALL_ON), device=DEV, cfg=CFG)
    L, h, E_ARG = RS.lib(), unit._handle, -1
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)
    root, dof, act, cmd, tq, ids, flags, rew, hts = z(n, 13), z(n * 12, 2), z(n, 12), z(n, 3), z(n, 12), z(n, dt=torch.int32), z(n, dt=torch.long), z(n), z(n, 5)
    ptr = lambda t: t.data_ptr()

    def run(P=0, heights=None, reset=flags, handle=h, rew_=rew):
        return L.mpc_shaping_run(handle, ptr(root), ptr(dof), ptr(act), ptr(cmd), ptr(tq), None, ptr(ids), None if reset is None else ptr(reset) if hasattr(reset, "data_ptr") else reset,
                                 ptr(flags), None if heights is None else ptr(heights), P, None if rew_ is None else ptr(rew_), None, None)
    for kw, text in ((dict(), b"no sim bound"), (dict(P=-1), b"P must lie"), (dict(P=209, heights=hts), b"P must lie"), (dict(P=5), b"d_heights goes with"),
                     (dict(heights=hts), b"d_heights goes with"), (dict(reset=None), b"null"), (dict(rew_=None), b"null"), (dict(reset=ptr(flags) + 4), b"8-byte")):
        assert run(**kw) == E_ARG and text in L.mpc_shaping_last_error(), kw
    assert not rew.any().item() and not unit.ticks.any().item()                # nothing ran
    with pytest.raises(_lib.MpcLibraryError, match="8 environments"):
        unit.bind(BatchedToySim(_robots(n + 1), device=DEV))
    assert L.mpc_shaping_bind(h, None) == E_ARG and b"null sim" in L.mpc_shaping_last_error()
    assert L.mpc_shaping_close(h, None, None) == E_ARG and L.mpc_shaping_summary(h, None, None) == E_ARG
    assert L.mpc_shaping_arrays(h, *([C.byref(C.c_void_p())] * 6), None) == E_ARG
    unit.bind(BatchedToySim(_robots(n), device=DEV))
    good = dict(root_states=root, dof_state=dof, actions=act, commands=cmd, torques=tq, fell=None, reset_ids=ids, reset_buf=flags, progress_buf=flags, rew_buf=rew)
    for bad in (dict(root_states=root[:, :12].contiguous()), dict(reset_buf=flags.int()), dict(reset_ids=ids.long()), dict(heights=z(n + 1, 5)), dict(heights=z(n, 209)),
                dict(terms=z(n, 6)), dict(fell=z(n, dt=torch.int32)), dict(rew_buf=z(n, dt=torch.float64))):
        with pytest.raises(ValueError):
            unit.run(**{**good, **bad})
    with pytest.raises(ValueError):
        unit.close(ids.long())
    unit.run(**good)
    assert (unit.ticks == 1).all().item()


def test_the_task_refuses_before_the_device_is_touched(monkeypatch):
    from tests.test_reward_shaping import test_the_task_refuses_before_the_device_is_touched as refusals
    refusals(monkeypatch)
