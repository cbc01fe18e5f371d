// abi_refusals_main.cpp -- a stand-alone program over the host-only paths of the asymmetric actor-critic's C ABI (include/mpc_ppo.h,
// include/mpc_ppo_update.h, csrc/mpc_privileged_obs.h) and of the two units that read an mpc_task_config (include/mpc_task.h,
// csrc/mpc_episode_terms.h): create and destroy, and every refusal that comes back before the device is touched.  It needs no GPU; on a box
// without one a valid create answers MPC_E_NODEVICE, and that answer is checked too.  Built with the sanitizers on the HOST code of the units, it
// is how those paths are checked for out-of-bounds reads of the dims arrays, leaks of a refused or device-less handle and undefined behaviour
// (DESIGN.md section 8.3.3), and it holds the text of every refusal the two config readers share (csrc/mpc_task_config.h):
//
//   cd rl-mpc-locomotion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//         ../../tools/abi_refusals_main.cpp mpc_ppo.hip mpc_ppo_update.hip mpc_ppo_gemm.hip mpc_privileged_obs.hip mpc_task.hip mpc_episode_terms.hip \
//         -o /tmp/abi_refusals && /tmp/abi_refusals
// (mpc_ppo_gemm.hip: the GEMMs mpc_ppo_update.hip launches live in that unit.)
//
// Exit status 0 and "ok" on the last line when every call answered as expected and the sanitizers stayed silent.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../include/mpc_ppo_update.h"
#include "../include/mpc_task.h"
#include "../rl-mpc-locomotion_amd/csrc/mpc_episode_terms.h"
#include "../rl-mpc-locomotion_amd/csrc/mpc_privileged_obs.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("line %d: %s\n", __LINE__, #cond);                    \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool says(const char *text, const char *part) { return text && std::strstr(text, part) != nullptr; }
static bool is(const char *text, const std::string &whole) { return text && whole == text; }

// a config both units accept (the reference's aliengo numbers)
static mpc_task_config good_config() {
  mpc_task_config c{};
  c.lin_vel_scale = 2.0; c.ang_vel_scale = 0.25; c.dof_pos_scale = 1.0; c.dof_vel_scale = 0.05;
  const double rew[MPC_TASK_REW_TERMS] = {0.02, -0.08, -0.001, 0.01, -5e-7, -0.02};
  for (int i = 0; i < MPC_TASK_REW_TERMS; ++i) c.rew_scale[i] = rew[i];
  const double range[3][2] = {{-2.0, 2.0}, {-1.0, 1.0}, {-3.14, 3.14}};
  for (int a = 0; a < 3; ++a) { c.command_range[a][0] = range[a][0]; c.command_range[a][1] = range[a][1]; }
  c.clip_observations = 5.0;
  for (int i = 0; i < 12; ++i) c.default_dof_pos[i] = 0.1 * (i % 3);
  c.max_episode_length = 1000;
  c.seed = 7;
  return c;
}

// mpc_task_create and mpc_episode_terms_create (no curriculum) on one config: MPC_E_ARG with `<unit>: <text>` (null text: the unit accepts the
// config as far as the device, which this box may not have), and no handle either way unless there is a device
static void expect_config(const mpc_task_config &c, const char *task_text, const char *terms_text, int line) {
  int ndev = 0;
  const bool device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  mpc_task *t = nullptr;
  mpc_episode_terms *h = nullptr;
  const int rt = mpc_task_create(&t, 8, &c), rh = mpc_episode_terms_create(&h, 8, &c, 20.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0);
  bool ok = task_text ? rt == MPC_E_ARG && !t && is(mpc_task_last_error(), std::string("mpc_task_create: ") + task_text)
                      : device ? rt == MPC_OK && t : rt == MPC_E_NODEVICE && !t && is(mpc_task_last_error(), "mpc_task_create: no HIP device");
  ok = ok && (terms_text ? rh == MPC_E_ARG && !h && is(mpc_episode_terms_last_error(), std::string("mpc_episode_terms_create: ") + terms_text)
                         : device ? rh == MPC_OK && h
                                  : rh == MPC_E_NODEVICE && !h && is(mpc_episode_terms_last_error(), "mpc_episode_terms_create: no HIP device"));
  if (!ok) {
    std::printf("line %d: task %d \"%s\", terms %d \"%s\"\n", line, rt, mpc_task_last_error(), rh, mpc_episode_terms_last_error());
    ++failures;
  }
  mpc_task_destroy(t);
  mpc_episode_terms_destroy(h);
}

int main() {
  float *const p = reinterpret_cast<float *>(uintptr_t(0x10000)), *const q = reinterpret_cast<float *>(uintptr_t(0x20000));      // never dereferenced
  // exactly as many widths as the call may read: a read past n_layers + 1 entries is a heap overflow here
  std::vector<int> actor{48, 32, 12}, critic{64, 16, 1}, odd{60, 16, 1}, wide{4096, 16, 12}, wide_c{4096, 16, 1}, eq{48, 16, 1};
  std::vector<int> nine(10, 16);
  nine[0] = 48; nine[9] = 12;
  mpc_ac *ac = nullptr;
  EXPECT(mpc_ac_create_asymmetric(nullptr, 2, actor.data(), 2, critic.data()) == MPC_E_ARG);
  EXPECT(mpc_ac_create_asymmetric(&ac, 2, actor.data(), 2, odd.data()) == MPC_E_ARG && says(mpc_ppo_last_error(), "multiples of 16"));
  EXPECT(mpc_ac_create_asymmetric(&ac, 9, nine.data(), 2, critic.data()) == MPC_E_ARG && says(mpc_ppo_last_error(), "layers"));
  EXPECT(mpc_ac_create_asymmetric(&ac, 0, actor.data(), 2, critic.data()) == MPC_E_ARG);
  EXPECT(mpc_ac_create_asymmetric(&ac, 2, nullptr, 2, critic.data()) == MPC_E_ARG);
  EXPECT(mpc_ac_create_asymmetric(&ac, 2, wide.data(), 2, critic.data()) == MPC_E_ARG && says(mpc_ppo_last_error(), "LDS"));
  EXPECT(mpc_ac_create_asymmetric(&ac, 2, actor.data(), 2, wide_c.data()) == MPC_E_ARG && says(mpc_ppo_last_error(), "LDS"));
  EXPECT(ac == nullptr);
  EXPECT(mpc_ac_create(&ac, 2, actor.data(), 2, critic.data()) == MPC_E_ARG && says(mpc_ppo_last_error(), "same observations"));
  for (const std::vector<int> *c : {&critic, &eq}) {
    EXPECT(mpc_ac_create_asymmetric(&ac, 2, actor.data(), 2, c->data()) == MPC_OK && ac != nullptr);
    const int rc = mpc_ac_act(ac, 4, p, 1, 0, p, p, p, p, p, nullptr, nullptr);
    EXPECT(rc == MPC_E_ARG && says(mpc_ppo_last_error(), c == &critic ? "mpc_ac_act_asymmetric" : "bound"));
    EXPECT(mpc_ac_act_asymmetric(ac, 4, p, nullptr, 1, 0, p, p, p, p, p, nullptr, nullptr) == MPC_E_ARG && says(mpc_ppo_last_error(), "d_critic_obs"));
    EXPECT(mpc_ac_act_asymmetric(ac, 4, p, q, 1, 0, p + 1, p, p, p, p, nullptr, nullptr) == MPC_E_ARG && says(mpc_ppo_last_error(), "8-byte"));
    EXPECT(mpc_ac_act_asymmetric(ac, 4, p, q, 1, 0, p, p, p, p, p, nullptr, nullptr) == MPC_E_ARG && says(mpc_ppo_last_error(), "bound"));
    EXPECT(mpc_ac_evaluate(ac, 4, q, p, nullptr) == MPC_E_ARG && mpc_ac_act_inference(ac, 4, p, p, nullptr) == MPC_E_ARG);
    mpc_ppo_update *u = nullptr;
    EXPECT(mpc_ppo_update_create(&u, ac, 64) == MPC_E_ARG && u == nullptr);      // nothing bound: binding is what needs the device
    mpc_ac_destroy(ac);
    ac = nullptr;
  }
  mpc_ac_destroy(nullptr);
  EXPECT(mpc_ppo_update_set_critic_storage(nullptr, p + 1) == MPC_E_ARG && says(mpc_ppo_last_error(), "16-byte"));
  EXPECT(mpc_ppo_update_set_critic_storage(nullptr, p) == MPC_E_ARG && mpc_ppo_update_set_critic_storage(nullptr, nullptr) == MPC_E_ARG);

  EXPECT(mpc_privobs_width(0) == 64 && mpc_privobs_width(15) == 80 && mpc_privobs_width(187) == 240);
  EXPECT(mpc_privobs_width(-1) == MPC_E_ARG && mpc_privobs_width(209) == MPC_E_ARG);
  mpc_privobs *h = nullptr;
  EXPECT(mpc_privobs_create(nullptr, 4) == MPC_E_ARG && mpc_privobs_create(&h, 0) == MPC_E_ARG && h == nullptr);
  EXPECT(mpc_privobs_create(&h, 4) == MPC_OK && h != nullptr);
  EXPECT(mpc_privobs_bind(h, nullptr) == MPC_E_ARG && mpc_privobs_bind(nullptr, nullptr) == MPC_E_ARG);
  const long long *prog = reinterpret_cast<const long long *>(uintptr_t(0x30000));
  EXPECT(mpc_privobs_run(nullptr, p, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG);
  EXPECT(mpc_privobs_run(h, nullptr, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG);
  EXPECT(mpc_privobs_run(h, p, 48, 209, prog, 0.001, q, nullptr) == MPC_E_ARG);
  EXPECT(mpc_privobs_run(h, p, 62, 15, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "obs_width"));
  EXPECT(mpc_privobs_run(h, p + 1, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "16-byte"));
  EXPECT(mpc_privobs_run(h, p, 64, 0, prog, 0.001, p, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "must not be"));
  EXPECT(mpc_privobs_run(h, p, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "no sim bound"));
  mpc_privobs_destroy(h);
  mpc_privobs_destroy(nullptr);

  // the two readers of an mpc_task_config: what they share they refuse in the same order, each in its own words
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const mpc_task_config good = good_config();
  const char *const nf_task = "a scale, a command range or a default joint angle is not finite", *const nf_terms = "a scale or a command range is not finite";
  const char *const order = "command range with min > max", *const length = "max_episode_length must be at least 1";
  expect_config(good, nullptr, nullptr, __LINE__);
  mpc_task_config c = good;
  c.dof_vel_scale = nan; expect_config(c, nf_task, nf_terms, __LINE__);
  c = good; c.rew_scale[MPC_TASK_REW_TERMS - 1] = inf; expect_config(c, nf_task, nf_terms, __LINE__);
  c = good; c.command_range[2][1] = nan; expect_config(c, nf_task, nf_terms, __LINE__);
  for (int a = 0; a < 3; ++a) {
    c = good; c.command_range[a][0] = 1.0; c.command_range[a][1] = 0.5; expect_config(c, order, order, __LINE__);
  }
  c = good; c.max_episode_length = 0; expect_config(c, length, length, __LINE__);
  // ... what only the task reads only the task refuses
  c = good; c.default_dof_pos[11] = inf; expect_config(c, nf_task, nullptr, __LINE__);
  c = good; c.clip_observations = 0.0; expect_config(c, "clip_observations must be positive", nullptr, __LINE__);
  c = good; c.clip_observations = nan; expect_config(c, "clip_observations must be positive", nullptr, __LINE__);
  // ... and the order of the answers where more than one check fails
  c = good; c.default_dof_pos[0] = nan; c.command_range[0][0] = 3.0; expect_config(c, nf_task, order, __LINE__);
  c = good; c.command_range[1][0] = 3.0; c.clip_observations = -1.0; c.max_episode_length = 0; expect_config(c, order, order, __LINE__);
  c = good; c.clip_observations = -1.0; c.max_episode_length = 0; expect_config(c, "clip_observations must be positive", length, __LINE__);
  // the arguments beside the config
  mpc_task *t = nullptr;
  EXPECT(mpc_task_create(nullptr, 8, &good) == MPC_E_ARG && mpc_task_create(&t, 0, &good) == MPC_E_ARG && mpc_task_create(&t, 8, nullptr) == MPC_E_ARG);
  EXPECT(t == nullptr && is(mpc_task_last_error(), "mpc_task_create: bad argument"));
  mpc_episode_terms *et = nullptr;
  EXPECT(mpc_episode_terms_create(nullptr, 8, &good, 20.0, 0, 0, 0, 0, 0, 0, 0) == MPC_E_ARG && is(mpc_episode_terms_last_error(), "mpc_episode_terms_create: null argument"));
  EXPECT(mpc_episode_terms_create(&et, 0, &good, 20.0, 0, 0, 0, 0, 0, 0, 0) == MPC_E_ARG && is(mpc_episode_terms_last_error(), "mpc_episode_terms_create: n must be at least 1"));
  EXPECT(mpc_episode_terms_create(&et, 8, &good, 0.0, 0, 0, 0, 0, 0, 0, 0) == MPC_E_ARG && says(mpc_episode_terms_last_error(), "episode_length_s"));
  EXPECT(mpc_episode_terms_create(&et, 8, &good, 20.0, 1, 0.5, 1.0, 0.5, 0.8, 2.0, 1) == MPC_E_ARG && says(mpc_episode_terms_last_error(), "lo <= 0 <= hi"));
  EXPECT(mpc_episode_terms_create(&et, 8, &good, 20.0, 1, -1.0, 1.0, 0.5, 0.8, 0.5, 1) == MPC_E_ARG && says(mpc_episode_terms_last_error(), "max_curriculum"));
  EXPECT(mpc_episode_terms_create(&et, 8, &good, 20.0, 1, -1.0, 1.0, 0.0, 0.8, 2.0, 1) == MPC_E_ARG && says(mpc_episode_terms_last_error(), "step"));
  EXPECT(mpc_episode_terms_create(&et, 8, &good, 20.0, 1, -1.0, 1.0, 0.5, nan, 2.0, 1) == MPC_E_ARG && says(mpc_episode_terms_last_error(), "threshold"));
  EXPECT(mpc_episode_terms_create(&et, 8, &good, 20.0, 1, -1.0, 1.0, 0.5, 0.8, 2.0, 0) == MPC_E_ARG && says(mpc_episode_terms_last_error(), "update_every"));
  EXPECT(et == nullptr);
  mpc_task_destroy(nullptr);
  mpc_episode_terms_destroy(nullptr);
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
