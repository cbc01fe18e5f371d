// abi_refusals_main.cpp -- a stand-alone program over the host-only paths of the asymmetric actor-critic's C ABI (include/mpc_ppo.h,
// include/mpc_ppo_update.h, csrc/mpc_privileged_obs.h): create and destroy, and every refusal that comes back before the device is touched.  It
// needs no GPU.  Built with the sanitizers on the HOST code of the three units, it is how those paths are checked for out-of-bounds reads of the
// dims arrays, leaks of a refused handle and undefined behaviour:
//
//   cd rl-mpc-locomotion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//         ../../tools/abi_refusals_main.cpp mpc_ppo.hip mpc_ppo_update.hip mpc_privileged_obs.hip -o /tmp/abi_refusals && /tmp/abi_refusals
//
// Exit status 0 and "ok" on the last line when every call answered as expected and the sanitizers stayed silent.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../include/mpc_ppo_update.h"
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
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
