// distill_refusals_main.cpp -- a stand-alone program over the host-only paths of policy distillation's entry points (include/mpc_ppo.h:
// mpc_ac_act_distill; include/mpc_ppo_update.h: mpc_ppo_update_set_distill_targets, mpc_ppo_update_grads_distill, mpc_ppo_update_apply_actor),
// tools/contact_terms_refusals_main.cpp's sibling: two valid creates (a student and a teacher of another depth and width, host memory until they are
// bound) and every refusal that comes back before the device is touched.  It needs no GPU.  The refusals of an update handle that exists (rows,
// loss_type, nothing bound, no targets) need a bound mpc_ac, so a device, and are tests/test_distill_gpu.py's.  Built with the sanitizers on the
// HOST code of the units, it is how these paths are checked for reads past the width arrays, leaks and undefined behaviour:
//
//   cd rl-mpc-locomotion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//         ../../tools/distill_refusals_main.cpp mpc_ppo.hip mpc_ppo_update.hip mpc_ppo_gemm.hip -o /tmp/distill_refusals && /tmp/distill_refusals
//
// Exit status 0 and "ok" on the last line when every call answered as expected and the sanitizers stayed silent.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mpc_ppo_update.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("line %d: %s\n", __LINE__, #cond);                    \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool says(const char *part) {
  const char *text = mpc_ppo_last_error();
  return text && std::strstr(text, part) != nullptr;
}

// an address of device memory that is never dereferenced
template <typename T>
static T *at(uintptr_t address) { return reinterpret_cast<T *>(address); }

int main() {
  float *const obs = at<float>(0x10000), *const wide = at<float>(0x20000), *const a = at<float>(0x30000), *const m = at<float>(0x40000);
  float *const s = at<float>(0x50000), *const label = at<float>(0x60000), *const eps = at<float>(0x70000);
  float *const odd8 = at<float>(0x30004), *const odd4 = at<float>(0x60002), *const odd16 = at<float>(0x60008);
  const long long *const idx = at<const long long>(0x80000);
  const double *const lr = at<const double>(0x90000);

  // ---- two valid creates: exactly as many widths as a create may read (a read past them is a heap overflow here)
  std::vector<int> student_actor{48, 32, 16, 12}, student_critic{64, 64, 1}, teacher_actor{64, 64, 12}, teacher_critic{64, 32, 1};
  mpc_ac *student = nullptr, *teacher = nullptr;
  EXPECT(mpc_ac_create_asymmetric(&student, 3, student_actor.data(), 2, student_critic.data()) == MPC_OK && student != nullptr);
  EXPECT(mpc_ac_create(&teacher, 2, teacher_actor.data(), 2, teacher_critic.data()) == MPC_OK && teacher != nullptr);

  // ---- mpc_ac_act_distill: the arguments first, then the handles' state
  EXPECT(mpc_ac_act_distill(nullptr, teacher, 4, obs, wide, 1, 0, a, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("mpc_ac_act_distill: bad argument"));
  EXPECT(mpc_ac_act_distill(student, nullptr, 4, obs, wide, 1, 0, a, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ac_act_distill(student, teacher, 0, obs, wide, 1, 0, a, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ac_act_distill(student, teacher, -4, obs, wide, 1, 0, a, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, nullptr, wide, 1, 0, a, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, nullptr, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, nullptr, s, label, nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, m, nullptr, label, nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, nullptr, 1, 0, a, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("d_teacher_obs or d_teacher_actions is null"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, m, s, nullptr, nullptr, nullptr) == MPC_E_ARG && says("d_teacher_obs or d_teacher_actions is null"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, odd8, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("8-byte aligned"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, odd8, s, label, nullptr, nullptr) == MPC_E_ARG && says("8-byte aligned"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, m, odd8, label, nullptr, nullptr) == MPC_E_ARG && says("8-byte aligned"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, m, s, label, odd8, nullptr) == MPC_E_ARG && says("8-byte aligned"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, m, s, odd4, nullptr, nullptr) == MPC_E_ARG && says("4-byte aligned"));
  EXPECT(mpc_ac_act_distill(student, teacher, 4, obs, wide, 1, 0, a, m, s, label, eps, nullptr) == MPC_E_ARG && says("the student has no parameters bound"));
  EXPECT(mpc_ac_act_distill(student, student, 4, obs, obs, 1, 0, a, m, s, label, nullptr, nullptr) == MPC_E_ARG && says("the student has no parameters bound"));

  // ---- the update's entry points without a handle
  EXPECT(mpc_ppo_update_set_distill_targets(nullptr, label) == MPC_E_ARG && says("mpc_ppo_update_set_distill_targets: bad argument"));
  EXPECT(mpc_ppo_update_set_distill_targets(nullptr, nullptr) == MPC_E_ARG && says("bad argument"));
  EXPECT(mpc_ppo_update_set_distill_targets(nullptr, odd16) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_ppo_update_grads_distill(nullptr, 4, idx, 0, m, nullptr) == MPC_E_ARG && says("mpc_ppo_update_grads_distill: bad argument"));
  EXPECT(mpc_ppo_update_apply_actor(nullptr, 1.0, 0.9, 0.999, 1e-8, 1, lr, nullptr) == MPC_E_ARG && says("mpc_ppo_update_apply_actor: bad argument"));
  // an update handle is made over a BOUND mpc_ac: these two are host memory only, and the create says so before it looks for a device
  mpc_ppo_update *u = nullptr;
  EXPECT(mpc_ppo_update_create(&u, student, 64) == MPC_E_ARG && says("no parameters bound") && u == nullptr);
  EXPECT(mpc_ppo_update_create(&u, nullptr, 64) == MPC_E_ARG && u == nullptr);

  mpc_ac_destroy(student);
  mpc_ac_destroy(teacher);
  mpc_ac_destroy(nullptr);
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
