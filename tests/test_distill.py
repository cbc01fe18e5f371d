"""Teacher-student policy distillation (rl_mpc_locomotion_amd.distill, include/mpc_ppo.h's mpc_ac_act_distill, include/mpc_ppo_update.h's distillation
entry points, csrc/ppo_update.h's bc_element) on the CPU: the torch backend of Distillation.update and the header's arithmetic against the float64
restatement (tests/distill_ref.py), the view and the runner's refusals, the refusals program under the host sanitizers, the kernels' resource usage,
and which GEMM kernels the single-slot launches of tests/test_distill_gpu.py reach.

The tolerance is the project's rule (tests/test_ppo_update.py): a quantity may differ from the float64 reference by at most 4 x the distance of
torch's own float32 evaluation from it, the distance pooled over the cases (both loss types) because a single one is one draw of a rounding error."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, distill as D, ppo as P
from tests import distill_ref as ref
from tests.helpers import ROOT
from tests.test_ppo_gemm_plan import BACKWARD_DATA, BACKWARD_WEIGHT, FORWARD, NARROW, WIDE, plan  # noqa: F401  (plan: the g++ shim over ppo_gemm_plan.h)

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LOSS_TYPES = ("mse", "huber")
NETS = ((32, 16), (64,))


def _cfg(loss_type, **kw):
    return D.DistillConfig(num_learning_epochs=2, num_mini_batches=4, loss_type=loss_type, actor_hidden_dims=NETS[0], critic_hidden_dims=NETS[1], **kw)


@pytest.fixture(scope="module")
def runs():
    """The fixture (65 environments x 6 slots, 4 mini-batches of 97 rows, 2 rows left out) and per loss type the float64 and the float32 restatement of
    two epochs, computed once."""
    ac, st = ref.fixture(NETS, n=65, T=6)
    perm = torch.randperm(65 * 6, generator=torch.Generator().manual_seed(7))[:4 * 97].contiguous()
    return ac, st, perm, {lt: (ref.update(ac, _cfg(lt), st, perm, torch.float64), ref.update(ac, _cfg(lt), st, perm, torch.float32)) for lt in LOSS_TYPES}


def test_the_huber_fixture_has_elements_on_both_sides_of_delta(runs):
    ac, st, perm, _ = runs
    _, _, share = ref.grads_of(ac, "huber", st, perm, torch.float64)
    print(f"share of elements with |mu - target| > 1: {share:.3f}")
    assert 0.05 < share < 0.95


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_the_torch_backend_matches_the_float64_restatement(runs, loss_type):
    ac, st, perm, both = runs
    names, n_actor = ref.actor_names(ac), len(ref.actor_params(ac))
    p0 = [p.detach().double() for p in ac.bind_order()]
    gaps = {}                                                                     # parameter change, exp_avg, exp_avg_sq: pooled over tensors and loss types
    for r64, r32 in both.values():
        for kind, (a64, a32) in enumerate(((r64[0][:n_actor], r32[0][:n_actor]), (r64[2], r32[2]), (r64[3], r32[3]))):
            for k in range(n_actor):
                off = p0[k] if kind == 0 else 0.0
                gaps[kind] = max(gaps.get(kind, 0.0), ref.rel_l2(a32[k].double() - off, a64[k] - off))
    student = ref.clone(ac, torch.float32)
    rest0 = [p.detach().clone() for p in student.bind_order()[n_actor:]]
    alg = D.Distillation(student, _cfg(loss_type), backend="torch")
    loss, gap = alg.update(st, indices=perm)
    r64 = both[loss_type][0]
    params = student.bind_order()
    state = [params[:n_actor], [alg.optimizer.state[p]["exp_avg"] for p in params[:n_actor]], [alg.optimizer.state[p]["exp_avg_sq"] for p in params[:n_actor]]]
    for kind, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
        want = (r64[0][:n_actor], r64[2], r64[3])[kind]
        errs = []
        for k in range(n_actor):
            off = p0[k] if kind == 0 else 0.0
            errs.append((names[k], ref.rel_l2(state[kind][k].detach().double() - off, want[k] - off), gaps[kind]))
        ref.pooled(errs, f"{loss_type}: {what}")
    assert all(float((p.detach().double() - q).abs().max()) > 0 for p, q in zip(params[:n_actor], p0))       # every actor tensor moved
    # the critic and std: bit for bit where they were, with no gradient and no optimiser state
    for p, q in zip(params[n_actor:], rest0):
        assert torch.equal(p, q) and p.grad is None and p not in alg.optimizer.state
    assert len(alg.optimizer.state) == n_actor and all(int(alg.optimizer.state[p]["step"]) == 8 for p in params[:n_actor])
    # the returned means over the eight mini-batches, the two scalars pooled over both loss types
    means = lambda run: [np.mean([t[q] for t in run[1]]) for q in range(2)]
    pool = max(abs(a - b) / abs(b) for x64, x32 in both.values() for a, b in zip(means(x32), means(x64)))
    for name, got, want in zip(("behaviour loss", "action gap"), (float(loss), float(gap)), means(r64)):
        print(f"{loss_type}: returned mean {name} {got:.9g} float64 {want:.9g} (bound {4 * pool:.3e})")
        assert pool > 0 and abs(got - want) <= 4 * pool * abs(want)


def test_the_losses_differ_and_the_storage_draws_rsl_rls_permutation(runs):
    ac, st, perm, both = runs
    assert abs(both["mse"][0][1][0][0] - both["huber"][0][1][0][0]) > 0.1          # (the first mini-batch's loss: mse is about twice huber's and more)
    torch.manual_seed(3)
    want = torch.randperm(4 * 97)
    torch.manual_seed(3)
    got = list(st.mini_batch_generator(4, 2))
    assert len(got) == 8 and all(torch.equal(got[e * 4 + i], want[i * 97:(i + 1) * 97]) for e in range(2) for i in range(4))
    with pytest.raises(ValueError, match="fewer rows than mini-batches"):
        D.DistillStorage(1, 2, "cpu", 48).indices(3)


# ---- csrc/ppo_update.h's bc_element, compiled with g++, as the device's head runs it
SHIM = r"""
#include "ppo_update.h"
using namespace ppo;
extern "C" void shim_bc(int rows, int loss_type, const float *mu, const float *target, float *terms, float *dmu) {
  const float norm = bc_norm(loss_type, rows);
  double loss = 0, gap = 0;
  for (int e = 0; e < 12 * rows; ++e) {
    float value, d;
    bc_element(loss_type, norm, mu[e], target[e], value, dmu[e], d);
    loss += value; gap += d;
  }
  terms[0] = (float)(loss / (12.0 * rows)); terms[1] = (float)(gap / (12.0 * rows));
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("distill_shim")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    L.shim_bc.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4; L.shim_bc.restype = None
    return L


def _head_torch(mu, target, loss_type, dtype):
    mu = mu.to(dtype).clone().requires_grad_()
    f = torch.nn.functional.mse_loss if loss_type == "mse" else torch.nn.functional.huber_loss
    loss = f(mu, target.to(dtype))
    loss.backward()
    return [float(loss.detach()), float((mu.detach() - target.to(dtype)).abs().mean())], mu.grad


def test_the_header_head_matches_float64_autograd(shim):
    g = torch.Generator().manual_seed(11)
    cases, gaps, term_gap = {}, 0.0, 0.0
    for rows in (1, 97, 390):
        mu = torch.randn((rows, 12), generator=g)
        target = mu + torch.randn((rows, 12), generator=g)
        target[0, 0] = mu[0, 0] + 1.0                                             # |d| on the edge, where both branches of huber agree
        for lt in LOSS_TYPES:
            t64, g64 = _head_torch(mu, target, lt, torch.float64)
            t32, g32 = _head_torch(mu, target, lt, torch.float32)
            cases[(rows, lt)] = (mu, target, t64, g64)
            gaps = max(gaps, ref.rel_l2(g32, g64))
            term_gap = max(term_gap, max(abs(a - b) / abs(b) for a, b in zip(t32, t64)))
    a = lambda t: np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)
    for (rows, lt), (mu, target, t64, g64) in cases.items():
        m, t = a(mu), a(target)
        terms, dmu = np.zeros(2, np.float32), np.zeros((rows, 12), np.float32)
        shim.shim_bc(rows, D.LOSS_TYPES[lt], m.ctypes.data, t.ctypes.data, terms.ctypes.data, dmu.ctypes.data)
        ref.pooled([("d loss / d mu", ref.rel_l2(torch.from_numpy(dmu), g64), gaps)], f"{lt} {rows} rows")
        for name, got, want in zip(("loss", "mean |d|"), terms, t64):
            print(f"{lt} {rows} rows: {name} {got:.9g} float64 {want:.9g} (bound {4 * term_gap:.3e})")
            assert term_gap > 0 and abs(float(got) - want) <= 4 * term_gap * abs(want)


# ---- the view and the runner, without a device
class _Task:
    """What TeacherEnv and Distiller's refusal pass read of a task."""
    num_envs, num_obs, num_actions, device = 4, 48, 12, None

    def __init__(self, privileged=64):
        self.num_privileged_obs = privileged
        self.obs_buf, self.privileged_obs_buf = torch.zeros(4, 48), None if privileged is None else torch.ones(4, privileged)
        self.stepped = None

    def reset(self):
        return self.obs_buf

    def step(self, actions):
        self.stepped = actions
        return self.obs_buf, torch.zeros(4), torch.zeros(4, dtype=torch.long), {"time_outs": torch.zeros(4, dtype=torch.long)}


def test_the_teacher_env_is_a_view_of_the_task():
    with pytest.raises(ValueError, match="no privileged observations"):
        D.TeacherEnv(_Task(privileged=None))
    task = _Task()
    env = D.TeacherEnv(task)
    assert env.num_obs == 64 and env.num_privileged_obs == 64 and env.num_envs == 4 and env.num_actions == 12
    assert env.reset() is task.privileged_obs_buf                               # the task's own buffer: nothing is copied
    actions = torch.zeros(4, 12)
    obs, rew, reset, extras = env.step(actions)
    assert obs is task.privileged_obs_buf and task.stepped is actions and "time_outs" in extras and rew.shape == (4,) and reset.dtype == torch.long
    env.common_step_counter = 7                                                  # written through, as the trainer's checkpoint parts write it
    assert task.common_step_counter == 7 and env.common_step_counter == 7
    with pytest.raises(AttributeError):
        env.no_such_member


def test_the_runner_refuses_before_the_device_is_asked_for(monkeypatch, tmp_path):
    monkeypatch.setattr(D, "need_gpu", lambda *a, **k: (_ for _ in ()).throw(_lib.MpcLibraryError("device asked for")))
    torch.manual_seed(1)
    teacher = P.ActorCritic(64, 12, (64,), (32,))
    ck = {"model_state_dict": teacher.state_dict(), "iter": 1, "infos": []}
    with pytest.raises(ValueError, match="the task has no privileged observations"):
        D.Distiller(_Task(privileged=None), ck)
    with pytest.raises(ValueError, match="the teacher's actor reads rows of 64 columns, the task's privileged rows have 80"):
        D.Distiller(_Task(privileged=80), ck)
    with pytest.raises(ValueError, match="the teacher's actor reads rows of 48 columns"):
        D.Distiller(_Task(), P.ActorCritic(48, 12, (64,), (32,), num_critic_obs=64))
    recurrent = dict(ck, model_state_dict=dict(teacher.state_dict(), **{"memory_a.rnn.weight_ih_l0": torch.zeros(4, 64)}))
    with pytest.raises(ValueError, match="a recurrent teacher is not built"):
        D.Distiller(_Task(), recurrent)
    with pytest.raises(ValueError, match="loss_type is 'mse' or 'huber', not 'l1'"):
        D.Distiller(_Task(), ck, D.DistillConfig(loss_type="l1"))
    with pytest.raises(ValueError, match="update is 'torch' or 'hip'"):
        D.Distiller(_Task(), ck, update="cuda")
    with pytest.raises(ValueError, match="backend is 'torch' or 'hip'"):
        D.Distillation(teacher, backend="cuda")
    with pytest.raises(ValueError, match="loss_type is 'mse' or 'huber'"):
        D.Distillation(teacher, D.DistillConfig(loss_type="l1"))
    # what passes the refusals asks for the device: a checkpoint dict, a bare state dict, a path and a module
    path = str(tmp_path / "teacher.pt")
    torch.save(ck, path)
    for given in (ck, teacher.state_dict(), path, teacher):
        with pytest.raises(_lib.MpcLibraryError, match="device asked for"):
            D.Distiller(_Task(), given)
    with pytest.raises(_lib.MpcLibraryError, match="device asked for"):
        D.Distillation(teacher, backend="hip")


def test_a_normalised_teacher_is_folded_and_frozen():
    from rl_mpc_locomotion_amd.obs_norm import fold_normalizer
    torch.manual_seed(2)
    teacher = P.ActorCritic(64, 12, (32, 16), (32,))
    g = torch.Generator().manual_seed(3)
    mean, std = torch.randn((1, 64), generator=g), torch.rand((1, 64), generator=g) + 0.5
    norm = {"_mean": mean, "_var": std * std, "_std": std, "count": torch.tensor(100)}
    ck = {"model_state_dict": teacher.state_dict(), "obs_norm_state_dict": norm}
    net = D.load_teacher(ck, 64)
    want = fold_normalizer(teacher.state_dict(), norm)
    assert all(torch.equal(v, want[k]) for k, v in net.state_dict().items()) and not torch.equal(net.state_dict()["actor.0.weight"], teacher.state_dict()["actor.0.weight"])
    assert all(not p.requires_grad for p in net.parameters())
    rows = torch.randn((5, 64), generator=g) * std + mean                        # raw rows give what the teacher gave on normalised ones
    np.testing.assert_allclose(net.actor(rows).detach().numpy(), teacher.actor((rows - mean) / (std + 1e-2)).detach().numpy(), rtol=1e-4, atol=1e-5)
    plain = D.load_teacher({"model_state_dict": teacher.state_dict()}, 64)
    assert all(torch.equal(v, teacher.state_dict()[k]) for k, v in plain.state_dict().items())
    assert plain.num_critic_obs is None and D.load_teacher(P.ActorCritic(64, 12, (16,), (16,), num_critic_obs=80).state_dict(), 64).num_critic_obs == 80


def test_the_bindings_name_the_headers_entry_points():
    names = ("mpc_ac_act_distill", "mpc_ppo_update_set_distill_targets", "mpc_ppo_update_grads_distill", "mpc_ppo_update_apply_actor")
    assert names[0] in P.DECLS and all(n in P.UPDATE_DECLS for n in names[1:])
    text = open(os.path.join(ROOT, "include", "mpc_ppo.h")).read() + open(os.path.join(ROOT, "include", "mpc_ppo_update.h")).read()
    for n in names:
        (args,) = re.findall(r"\bint " + n + r"\(([^;]*)\);", text)
        assert len(args.split(",")) == len({**P.DECLS, **P.UPDATE_DECLS}[n][1]), n
    L = P.update_lib()                                                           # the library exports them
    assert all(hasattr(L, n) for n in names)
    assert L.mpc_ppo_update_grads_distill(None, 4, None, 0, None, None) == -1 and b"mpc_ppo_update_grads_distill: bad argument" in L.mpc_ppo_last_error()


def test_refusals_program_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/distill_refusals_main.cpp, a stand-alone program over the new entry points' host paths, built with AddressSanitizer and UBSan on the host
    code and run directly: two valid creates and every refusal that needs no device."""
    exe = tmp_path / "distill_refusals"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-x", "hip",
                    os.path.join(ROOT, "tools", "distill_refusals_main.cpp"), os.path.join(CSRC, "mpc_ppo.hip"), os.path.join(CSRC, "mpc_ppo_update.hip"),
                    os.path.join(CSRC, "mpc_ppo_gemm.hip"), "-o", str(exe)], check=True, cwd=CSRC)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


@pytest.mark.parametrize("unit, kernels", (("mpc_ppo.hip", {"ac_kernel": None}),
                                           ("mpc_ppo_update.hip", {"bc_head_kernel": 2 * 256 * 8 + 2 * 16 * 8, "bc_reduce_kernel": 2 * 16 * 8})))
def test_kernels_compile_for_gfx950_without_scratch(tmp_path, capsys, unit, kernels):
    """The changed kernel (ac_kernel: the second net's row) and the new ones: no scratch, and the static LDS of the new ones' fixed-order sums
    (ac_kernel's LDS is dynamic)."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, unit), "-o", str(tmp_path / "unit.o")], check=True, capture_output=True, text=True)
    found = {}
    for name, sgpr, vgpr, scratch, lds in re.findall(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                                                     r.stderr, re.S):
        found[name] = dict(sgprs=int(sgpr), vgprs=int(vgpr), scratch=int(scratch), lds=int(lds))
    with capsys.disabled():
        for name, v in found.items():
            print(f"\n  {name}: {v}", end="")
    for kernel, lds in kernels.items():
        hit = [v for k, v in found.items() if kernel in k]
        assert len(hit) == 1 and hit[0]["scratch"] == 0 and (lds is None or hit[0]["lds"] == lds), (kernel, found)
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, unit)).read())
    assert "atomic" not in text


# ---- which GEMM kernels the single-slot launches of tests/test_distill_gpu.py reach
def launches(hidden, rows, num_obs=48):
    """mpc_ppo_update_grads_distill's GEMM launches for an actor with `hidden` layers at `rows` rows of `num_obs` columns, in its order, each (kind,
    (M, N, K)) with the critic's slot empty: mpc_ppo_update_grads' sequence (csrc/mpc_ppo_update.hip's forward_pass and backward_pass) for one net."""
    d = [num_obs, *hidden, 12]
    n = len(d) - 1
    out = [(FORWARD, (rows, d[l + 1], d[l])) for l in range(n)]
    for l in range(n - 1, -1, -1):
        out.append((BACKWARD_WEIGHT, (d[l + 1], d[l], rows)))
        if l > 0:
            out.append((BACKWARD_DATA, (rows, d[l], d[l + 1])))
    return out


def planned(plan, hidden, rows, num_obs=48):
    out = []
    for kind, shape in launches(hidden, rows, num_obs):
        p = plan(kind, shape, None)
        assert p["problems"][1] == (0, 0, 1)                                      # the critic's slot: nothing to do
        out.append((kind, p["tile"], p["chunk_rows"], p["problems"][0][2]))
    return out


def test_the_gpu_cases_single_slot_launches_reach_the_kernels_they_name(plan):  # noqa: F811
    from tests import test_distill_gpu as G
    assert G.NETS == {"uneven": ((32, 16), (64,)), "odd": ((80, 48), (144,))} and sorted(G.ROWS.values()) == [1, 97, 257, 1040]
    for hidden, _ in G.NETS.values():
        for rows in G.ROWS.values():
            got = planned(plan, hidden, rows)
            chunks = -(-rows // 256)
            assert got == [(FORWARD, NARROW, 0, 1)] * 3 + [(BACKWARD_WEIGHT, NARROW, 256, chunks), (BACKWARD_DATA, NARROW, 0, 1)] * 2 + [(BACKWARD_WEIGHT, NARROW, 256, chunks)]
    assert -(-1040 // 256) == 5 and 257 - 256 == 1                                # several backward-weight chunks; a second head workgroup with one live row
    # the reference student at 8192 rows: layer 0's forward GEMM, layer 1's weight gradient and the backward-data GEMM into layer 0 take the 128 x 128
    # tile with a single slot
    hidden, rows = G.BIG_NETS[0], G.BIG_ROWS
    assert hidden == P.PPOConfig().actor_hidden_dims == (512, 256, 128) and rows == 8192 and G.BIG_WIDTH == 48
    assert planned(plan, hidden, rows) == [
        (FORWARD, WIDE, 0, 1), (FORWARD, NARROW, 0, 1), (FORWARD, NARROW, 0, 1), (FORWARD, NARROW, 0, 1),
        (BACKWARD_WEIGHT, NARROW, 256, 32), (BACKWARD_DATA, NARROW, 0, 1),
        (BACKWARD_WEIGHT, NARROW, 256, 32), (BACKWARD_DATA, NARROW, 0, 1),
        (BACKWARD_WEIGHT, WIDE, 256, 32), (BACKWARD_DATA, WIDE, 0, 1),
        (BACKWARD_WEIGHT, NARROW, 256, 32)]
    # 8192 is the smallest: one 128-row tile fewer and layer 0's forward GEMM has 63 x 4 < kMinWideTiles tiles
    assert planned(plan, hidden, 8192 - 128)[0] == (FORWARD, NARROW, 0, 1) and planned(plan, hidden, 8192 - 127)[0] == (FORWARD, WIDE, 0, 1)
