"""The contact terms on the MI355X (csrc/mpc_contact_terms.h, rl_mpc_locomotion_amd.contact_terms): the kernels through the C ABI against the
restatement of tests/contact_terms_ref.py on chained hand-made ticks (terms, reward, sums, ticks, window and summary EQUAL, unlisted environments
untouched, a rerun identical), the row widening with a sentinel behind the output, and the hooks in BatchedRLTask.step and PPOTrainer: thirty ticks on
a slippery plane fed to the restatement tick by tick without a host synchronisation, the privileged rows of a task with every neighbouring option,
the trainer's records and a checkpoint round trip.

The task's own six terms hold an expf and are taken from the device (EpisodeTerms.accumulate's ``terms``, the same rltask::reward_terms on the same
tensors); everything the unit adds is compared bit for bit (NaN for NaN)."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import contact_terms as CT, episode_terms as E, friction as FR, reward_shaping as RS, rl_task as R
from tests import contact_terms_ref as ref, reward_shaping_ref as sref
from tests.contact_terms_ref import F, same
from tests.test_contact_terms import CFG, CLIP_OBS, FORCE_SCALE, MU_CLIP, restatement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
STATE = ("sums", "ticks", "window")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _robots(n):
    return [i % 3 for i in range(n)]


def _spec(per_second, max_force=ref.MAX_FORCE):
    return CT.ContactSpec(**dict(zip(CT.CONTACT_TERMS, per_second)), max_contact_force=max_force, force_scale=FORCE_SCALE, mu_clip=MU_CLIP)


def _state(unit):
    return {name: getattr(unit, name).cpu().numpy().copy() for name in STATE}


def _bound(n, per_second, mu=0.4):
    """(sim, friction, unit): a plant of n robots with a friction record, whose force and slip rows the tests write by hand, and the unit bound to it."""
    from rl_mpc_locomotion_amd.toy_sim import BatchedToySim
    sim = BatchedToySim(_robots(n), device=DEV)
    fr = FR.Friction(n, mu=mu, device=DEV)
    fr.bind(sim)
    unit = CT.ContactTerms(n, _spec(per_second), cfg=CFG, device=DEV)
    assert unit.sums is None
    unit.bind(sim)
    return sim, fr, unit


@pytest.mark.parametrize("n", ref.SIZES)
def test_kernels_equal_the_restatement_through_the_c_abi(n):
    """Six ticks with resets of everybody at tick 0, of some on two consecutive ticks and of nobody: every term live without and with shaping terms,
    and all three off, where the reward that comes out is the reward that went in."""
    import torch
    six = E.EpisodeTerms(n, CFG, device=DEV)                                # the device's own six task terms
    for per_second, shaping in ((ref.ALL_ON, None), (ref.ALL_ON, ref.SHAPING_ON), (ref.SUBSETS[0], ref.SHAPING_ON), (ref.SUBSETS[0], None), (ref.SUBSETS[5], None)):
        sim, fr, unit = _bound(n, per_second)
        assert unit.sums.shape == (n, 3) and unit.sums.dtype == torch.float32 and unit.ticks.dtype == torch.int32 and unit.window.shape == (4,)
        assert not any(getattr(unit, name).any().item() for name in STATE)
        want = restatement(n, per_second)
        g = None if shaping is None else ref.scales_of(shaping, ref.DT)
        rng, srng = np.random.default_rng(7 * n), np.random.default_rng(9 * n)
        ticks = ref.chain(n, 100 * n)
        for t, (ids, b) in enumerate(ticks):
            s = sref.random_tick(n, 0, rng)                                    # what `finish` read: root states, commands, torques, the fall flag
            d = {k: _dev(np.ascontiguousarray(s[k], F)) for k in ("root", "commands", "torques")}
            fell, d_ids = _dev(s["fell"]), _dev(ids)
            fr.contact_forces.copy_(_dev(b["force"]))
            fr.foot_slip.copy_(_dev(b["slip"]))
            task6 = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
            six.accumulate(d["root"], d["commands"], d["torques"], fell, terms=task6)
            t6 = task6.cpu().numpy()
            se = None if shaping is None else ref.shaping_tick(n, srng)
            rew_in = ref.reward(ref.SUBSETS[0], t6, np.zeros((n, 3), F), g, se)   # what the step without the unit leaves in rew_buf
            before = _state(unit)
            unit.close(d_ids)
            closed_state = _state(unit)
            S = want.close(ids)
            keep = ids < 0
            assert closed_state["sums"][keep].tobytes() == before["sums"][keep].tobytes() and (closed_state["ticks"][keep] == before["ticks"][keep]).all()
            saved = {name: getattr(unit, name).clone() for name in STATE}
            out = []
            for rerun in range(2 if t == len(ticks) - 1 else 1):               # the last tick twice from the same state
                if rerun:
                    for name in STATE:
                        getattr(unit, name).copy_(saved[name])
                rew, terms = _dev(rew_in), torch.full((n, 3), 7.0, dtype=torch.float32, device=DEV)
                unit.run(d["root"], d["commands"], d["torques"], fell, d_ids, rew, shaping_terms=None if se is None else _dev(se),
                         shaping_scales=None if shaping is None else [float(v) * ref.DT for v in shaping], terms=terms)
                out.append([rew.cpu().numpy(), terms.cpu().numpy()] + list(_state(unit).values()))
            if len(out) == 2:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(*out)), (n, "rerun")
            e_want, rew_want = want.run(b["force"], b["slip"], ids, t6, g, se)
            assert same(out[0][1], e_want), (n, t, "terms", np.argwhere(~(out[0][1] == e_want)))
            assert same(out[0][0], rew_want), (n, t, "rew")
            if not any(per_second):
                assert out[0][0].tobytes() == rew_in.tobytes(), (n, t)          # all scales 0: the reward that went in
            for name, w in want.state().items():
                assert same(_state(unit)[name], w), (n, t, name)
            assert np.isfinite(S).all()
        assert want.window[0] == (ref.marks(n, "some", 2) >= 0).sum() + (ref.marks(n, "some", 3) >= 0).sum()
        summary = unit.summary().cpu().numpy()
        assert summary.tobytes() == ref.summary(want.window, CFG.episode_length_s).tobytes()
        assert CT.ContactTerms.record(summary.tolist()) == CT.ContactTerms.record(ref.summary(want.window, CFG.episode_length_s).tolist())
        unit.new_window()
        assert not unit.window.any().item() and (unit.ticks > 0).all().item()


@pytest.mark.parametrize("n,wp", [(1, 64), (65, 240), (130, 256)])
def test_the_row_widening_equals_the_restatement_and_stays_inside_its_rows(n, wp):
    import torch
    rng = np.random.default_rng(n + wp)
    mu = np.resize(np.array([0.0, 0.4, MU_CLIP, np.inf, 1.25, 2.5]), n)
    sim, fr, unit = _bound(n, ref.ALL_ON, mu=mu)
    priv = rng.standard_normal((n, wp)).astype(F)
    priv[0, :4] = (np.nan, -0.0, np.inf, 1e-42)
    force = (rng.standard_normal((n, 4, 3)) * [60, 60, 300]).astype(F)
    force[0, 0] = (500.0, -500.0, np.nextafter(F(500), F(np.inf)))
    fr.contact_forces.copy_(_dev(force))
    width, tail = wp + CT.COLUMNS, 64
    assert unit.width(wp) == width
    flat = torch.full((n * width + tail,), float("nan"), dtype=torch.float32, device=DEV)
    out = flat[:n * width].view(n, width)
    d_priv = _dev(priv)
    assert unit.extend(d_priv, out) is out
    got = flat.cpu().numpy()
    assert np.isnan(got[n * width:]).all()                                     # the sentinel behind the last row
    assert same(got[:n * width].reshape(n, width), ref.extend(priv, mu, force, FORCE_SCALE, MU_CLIP, CLIP_OBS))
    assert d_priv.cpu().numpy().tobytes() == priv.tobytes()
    for bad in (dict(priv_row=d_priv[:, :wp - 8].contiguous()), dict(out=out[:, :wp].contiguous()), dict(priv_row=d_priv.double()), dict(priv_row=d_priv[:max(n - 1, 0)])):
        with pytest.raises(ValueError):
            unit.extend(**{**dict(priv_row=d_priv, out=out), **bad})


TICKS = 30


@pytest.fixture(scope="module")
def slippery():
    """64 robots of the three types on a plane with mu = 0.2, below the controller's fixed 0.4; zero actions for thirty ticks of episodes of twenty;
    every tick's tensors recorded on the device, from the second tick on under torch's sync debug mode."""
    import torch
    n = 64
    cfg = R.TaskConfig(episode_length_s=0.2, seed=5)
    runs = {}
    actions = torch.zeros((n, 12), dtype=torch.float32, device=DEV)
    for name, per_second in (("on", ref.ALL_ON), ("zero", ref.SUBSETS[0]), ("plain", None)):
        unit = None if per_second is None else CT.ContactTerms(n, _spec(per_second), cfg=cfg, device=DEV)
        if unit is not None:
            unit.terms_buf = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
        et = E.EpisodeTerms(n, cfg, device=DEV)
        et.terms_buf = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
        fr = FR.Friction(n, mu=0.2, device=DEV)
        task = R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, episode_terms=et, friction=fr, contact_terms=unit)
        assert task.contact_terms is unit
        shapes = dict(rew=(1, torch.float32), ids=(1, torch.int32), force=(12, torch.float32), slip=(4, torch.float32), six=(6, torch.float32),
                      terms=(3, torch.float32), obs=(task.num_obs, torch.float32), reset=(1, torch.long), root=(13, torch.float32))
        rec = {k: torch.zeros((TICKS, n, w), dtype=dt, device=DEV) for k, (w, dt) in shapes.items()}
        windows = torch.zeros((TICKS, 4), dtype=torch.float64, device=DEV)

        def tick(k):
            task.step(actions)
            for key, src in (("rew", task.rew_buf), ("ids", task.task.reset_ids), ("force", fr.contact_forces), ("slip", fr.foot_slip), ("six", et.terms_buf),
                             ("obs", task.obs_buf), ("reset", task.reset_buf), ("root", task.sim.root_states)):
                rec[key][k].copy_(src.reshape(n, -1))
            if unit is not None:
                rec["terms"][k].copy_(unit.terms_buf)
                windows[k].copy_(unit.window)
        tick(0)                                        # (the reset tick, which also loads the code objects, before the no-wait section)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")        # a torch call that waits for the device or copies to the host raises from here on
        try:
            for k in range(1, TICKS):
                tick(k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        marks = []
        task.step(actions, mark=marks.append)
        runs[name] = dict({k: v.cpu().numpy() for k, v in rec.items()}, windows=windows.cpu().numpy(), marks=marks,
                          state=None if unit is None else _state(unit))
    runs["cfg"], runs["n"] = cfg, n
    return runs


def test_thirty_ticks_on_a_slippery_plane_equal_the_restatement(slippery):
    cfg, n, h = slippery["cfg"], slippery["n"], slippery["on"]
    assert cfg.max_episode_length == 20
    want = restatement(n, ref.ALL_ON, dt=cfg.dt)
    assert (h["ids"][0, :, 0] == np.arange(n)).all()
    resets = 0
    for k in range(TICKS):
        ids = h["ids"][k, :, 0]
        want.close(ids)
        assert want.window.tobytes() == h["windows"][k].tobytes(), k
        e, rew = want.run(h["force"][k], h["slip"][k], ids, h["six"][k])
        assert same(h["terms"][k], e), (k, np.argwhere(~(h["terms"][k] == e)))
        assert same(h["rew"][k, :, 0], rew), (k, np.argwhere(~(h["rew"][k, :, 0] == rew)))
        assert not h["force"][k][ids >= 0].any() and not h["slip"][k][ids >= 0].any()      # friction.draw has zeroed the reset environments' rows
        resets += int((ids >= 0).sum())
    # the condition the test stands on: at mu = 0.2 feet slide, and the term sees it
    assert (h["slip"] != 0).any() and (h["terms"][:, :, ref.FEET_SLIP] != 0).any()
    assert (h["terms"][:, :, ref.FEET_SLIP] <= 0).all() and (h["terms"][:, :, ref.FEET_CONTACT_FORCES] <= 0).all()
    assert resets > n and want.window[0] >= n                                  # the time-out after twenty ticks closed an episode of everybody
    assert (h["state"]["ticks"] > 0).all()


def test_the_option_changes_the_reward_and_nothing_else(slippery):
    on, zero, plain = slippery["on"], slippery["zero"], slippery["plain"]
    for k in range(TICKS):
        for key in ("obs", "reset", "root", "ids", "force", "slip", "six"):
            assert on[key][k].tobytes() == plain[key][k].tobytes() == zero[key][k].tobytes(), (k, key)
        assert zero["rew"][k].tobytes() == plain["rew"][k].tobytes(), k          # all three scales 0: bit for bit the step without the unit
    assert not np.array_equal(on["rew"], plain["rew"])
    assert not zero["state"]["sums"].any() and (zero["state"]["ticks"] > 0).all() and zero["windows"][-1][0] >= slippery["n"]
    assert on["marks"] == plain["marks"] == zero["marks"] == [s for s in R.STAGES if s in ("actions", "controller", "plant", "begin", "episode_close", "resets", "finish",
                                                                                         "episode_accumulate")]
    assert len(R.STAGES) == 13


FULL_MAX_FORCE = 20.0                  # newtons: well below a stance foot's share of the weight, so that feet_contact_forces pays on the stairs
SHAPING = (-0.7, -3.0, -1e-3, -2.5e-7, -0.01, 1.5, -0.3, -200.0)


def _full_task(n=64, seed=3):
    """Every neighbouring option at once on the stairs: reward shaping, the height scan, plant randomisation shown to the critic, friction drawn at
    resets from a range that crosses mu_clip, and the contact terms with the critic's columns."""
    import torch
    from rl_mpc_locomotion_amd import height_scan as HS, plant_rand as PR, privileged_obs as V
    from rl_mpc_locomotion_amd.terrain import Terrain
    cfg = R.TaskConfig(command_x_range=(0.0, 0.5), command_y_range=(-0.1, 0.1), command_yaw_range=(-0.3, 0.3), episode_length_s=0.05, seed=5)
    origin = np.stack([np.linspace(2.1, 3.8, n), np.linspace(-0.6, 1.4, n)], 1)
    shaping = RS.RewardShaping(n, RS.ShapingSpec(**dict(zip(RS.SHAPING_TERMS, SHAPING)), base_height_target=0.31), device=DEV, cfg=cfg)
    et = E.EpisodeTerms(n, cfg, device=DEV)
    et.terms_buf = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    return R.BatchedRLTask(_robots(n), [TROT] * n, cfg=cfg, device=DEV, terrain=Terrain.reference_stairs(), origin=origin, height_scan=HS.HeightScan(n, device=DEV),
                           episode_terms=et, reward_shaping=shaping,
                           plant_rand=PR.PlantRand(n, PR.PlantSpec(payload=(-1.0, 3.0), strength=(0.9, 1.1), gravity=(-1.0, 1.0), resample="reset"), seed=21, device=DEV),
                           friction=FR.Friction(n, FR.FrictionSpec(range=(0.1, 3.0), buckets=0, resample="reset"), seed=seed, device=DEV),
                           privileged_obs=V.PrivilegedObs(n, device=DEV, plant=True),
                           contact_terms=CT.ContactTerms(n, _spec(ref.ALL_ON, max_force=FULL_MAX_FORCE), cfg=cfg, device=DEV, privileged=True))


def test_privileged_rows_carry_the_coefficient_and_the_reactions():
    import torch
    from rl_mpc_locomotion_amd.privileged_obs import privileged_width
    n = 64
    task = _full_task(n)
    fr, unit, cfg = task.friction, task.contact_terms, task.cfg
    wp = privileged_width(task.height_scan.num_points, True)
    assert task.num_privileged_obs == wp + 16 and task.privileged_obs_buf.shape == (n, wp + 16) and task.get_privileged_observations() is task.privileged_obs_buf
    shaping_terms = task._shaping_terms
    want = restatement(n, ref.ALL_ON, max_force=FULL_MAX_FORCE, dt=cfg.dt)
    g = ref.scales_of(SHAPING, cfg.dt)
    actions = _dev(np.random.default_rng(7).uniform(-1, 1, (12, n, 12)).astype(F))
    seen_reset = seen_force = clipped = 0
    for k in range(12):
        marks = []
        task.step(actions[k] if k else torch.zeros_like(actions[0]), mark=marks.append)
        assert marks == [s for s in R.STAGES if s not in ("push", "terrain_curriculum", "observation_noise")]
        ids, force, mu = task.task.reset_ids.cpu().numpy(), fr.contact_forces.cpu().numpy(), fr.get_mu()
        row = task.privileged_obs_buf.cpu().numpy()
        assert same(row, ref.extend(task._narrow_privileged.cpu().numpy(), mu, force, FORCE_SCALE, MU_CLIP, cfg.clip_observations)), k
        assert row[:, wp].tobytes() == np.minimum(mu, MU_CLIP).astype(F).tobytes()          # the mu column: min(get_mu(), mu_clip)
        assert not row[ids >= 0, wp + 1:wp + 13].any()                         # a reset environment's force columns are zero
        assert not row[:, wp + 13:].any()
        seen_reset += int((ids >= 0).sum())
        seen_force += int((row[ids < 0, wp + 1:wp + 13] != 0).sum())
        clipped += int((mu > MU_CLIP).sum())
        # the reward: shaping's terms of the tick and the contact terms inside one clip, termination on top
        want.close(ids)
        e, rew = want.run(force, fr.foot_slip.cpu().numpy(), ids, task.episode_terms.terms_buf.cpu().numpy(), g, shaping_terms.cpu().numpy())
        assert same(task.rew_buf.cpu().numpy(), rew), k
    assert seen_reset > n and seen_force > 0 and clipped > 0
    for name, w in want.state().items():
        assert same(_state(unit)[name], w), name


@pytest.mark.parametrize("kind", ["torch", "hip", "recurrent"])
def test_trainer_records_carry_the_contact_terms_and_checkpoints_round_trip(kind, tmp_path):
    import torch
    from rl_mpc_locomotion_amd import ppo as P
    from rl_mpc_locomotion_amd.recurrent import RecurrentConfig
    pcfg = P.PPOConfig(num_steps_per_env=8, num_learning_epochs=1, num_mini_batches=2, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    how = dict(update="torch", recurrent=RecurrentConfig(hidden_size=32, update_through_time="hip")) if kind == "recurrent" else dict(update=kind)
    task = _full_task()
    trainer = P.PPOTrainer(task, pcfg, seed=3, **how)
    assert trainer.contact_terms is task.contact_terms and trainer.num_privileged_obs == task.num_privileged_obs
    infos = trainer.learn(2)
    assert len(infos) == 2 and all(list(i)[-2:] == ["reward_shaping", "contact_terms"] for i in infos)

    def numbers(v):
        return [x for w in v.values() for x in numbers(w)] if isinstance(v, dict) else list(v) if isinstance(v, (list, tuple)) else [v]
    assert all(np.isfinite(np.asarray(numbers(i), dtype=np.float64)).all() for i in infos)
    rec = infos[1]["contact_terms"]
    assert list(rec) == ["rew_" + t for t in CT.CONTACT_TERMS] and all(v <= 0 for v in rec.values()) and rec["rew_feet_contact_forces"] < 0
    assert not task.contact_terms.window.any().item()                          # new_window followed the read
    path = str(tmp_path / "ck.pt")
    trainer.save(path)
    assert not [k for k in torch.load(path) if "contact" in k]                 # the unit adds no checkpoint part
    fresh = P.PPOTrainer(_full_task(), pcfg, seed=4, **how)
    fresh.load(path)
    assert fresh.iteration == 2 and all(torch.equal(a, b) for a, b in zip(trainer.actor_critic.parameters(), fresh.actor_critic.parameters()))
    assert np.array_equal(fresh.env.friction.get_mu(), task.friction.get_mu())
