// contact_terms_refusals_main.cpp -- a stand-alone program over the host-only paths of the contact terms' C ABI (csrc/mpc_contact_terms.h),
// tools/friction_refusals_main.cpp's sibling: create and destroy, and every refusal that comes back before the device is touched.  It needs no
// GPU: the handle is host memory until it is bound, and the sims it hands to bind are host structs (csrc/mpc_sim_internal.h) that hold a size and no
// device memory -- every call on them is refused before it would look for any.  Built with the sanitizers on the HOST code of the unit, it is how
// those paths are checked for reads past the scale arrays, leaks of a refused handle and undefined behaviour:
//
//   cd rl-mpc-locomotion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//         ../../tools/contact_terms_refusals_main.cpp mpc_contact_terms.hip -o /tmp/contact_terms_refusals && /tmp/contact_terms_refusals
//
// Exit status 0 and "ok" on the last line when every call answered as expected and the sanitizers stayed silent.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/mpc_batch.h"
#include "../rl-mpc-locomotion_amd/csrc/mpc_contact_terms.h"
#include "../rl-mpc-locomotion_amd/csrc/mpc_sim_internal.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("line %d: %s\n", __LINE__, #cond);                    \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool says(const char *part) {
  const char *text = mpc_contact_last_error();
  return text && std::strstr(text, part) != nullptr;
}

// an address of device floats that is never dereferenced
static float *at(uintptr_t address) { return reinterpret_cast<float *>(address); }

static mpc_task_config config() {
  mpc_task_config c{};
  c.lin_vel_scale = c.ang_vel_scale = c.dof_pos_scale = c.dof_vel_scale = 1.0;
  const double rew[6] = {0.01, -0.04, -0.0005, 0.005, -2.5e-7, 0.0};
  for (int i = 0; i < 6; ++i) c.rew_scale[i] = rew[i];
  const double range[3][2] = {{-2.5, 2.5}, {-1.0, 1.0}, {-2.5, 2.5}};
  for (int a = 0; a < 3; ++a) { c.command_range[a][0] = range[a][0]; c.command_range[a][1] = range[a][1]; }
  c.clip_observations = 5.0;
  c.max_episode_length = 2000;
  return c;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // never dereferenced: 16-byte aligned addresses of device rows, and one that is not
  float *const rows = at(0x10000), *const wide = at(0x80000), *const odd = at(0x10004);
  const int *const ids = reinterpret_cast<const int *>(uintptr_t(0x20000));
  // exactly as many entries as a call may read: a read past them is a heap overflow here
  std::vector<double> scales{-0.004, -0.0002, -0.015}, bad_scales{-0.004, nan, -0.015}, shaping(8, -0.001), bad_shaping(8, -0.001);
  bad_shaping[7] = inf;
  const mpc_task_config good = config();

  // ---- create, destroy
  mpc_contact *h = nullptr;
  EXPECT(mpc_contact_create(nullptr, 4, &good, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_create(&h, 4, nullptr, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_create(&h, 4, &good, nullptr, 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_create(&h, 0, &good, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("n must be at least 1"));
  EXPECT(mpc_contact_create(&h, -3, &good, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && h == nullptr);
  mpc_task_config c = good;
  c.rew_scale[2] = nan;
  EXPECT(mpc_contact_create(&h, 4, &c, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("not finite"));
  c = good;
  c.command_range[1][0] = 1.0, c.command_range[1][1] = -1.0;
  EXPECT(mpc_contact_create(&h, 4, &c, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("min > max"));
  c = good;
  c.max_episode_length = 0;
  EXPECT(mpc_contact_create(&h, 4, &c, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("max_episode_length"));
  c = good;
  c.clip_observations = -1.0;
  EXPECT(mpc_contact_create(&h, 4, &c, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("clip_observations"));
  EXPECT(mpc_contact_create(&h, 4, &good, bad_scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("contact scale"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), -1.0, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("max_contact_force"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), inf, 0.01, 2.0, 0.01, 20.0) == MPC_E_ARG && says("max_contact_force"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 100.0, 0.0, 2.0, 0.01, 20.0) == MPC_E_ARG && says("force_scale"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 100.0, nan, 2.0, 0.01, 20.0) == MPC_E_ARG && says("force_scale"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 100.0, 0.01, 0.0, 0.01, 20.0) == MPC_E_ARG && says("mu_clip"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 100.0, 0.01, inf, 0.01, 20.0) == MPC_E_ARG && says("mu_clip"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 100.0, 0.01, 2.0, 0.0, 20.0) == MPC_E_ARG && says("dt must"));
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 100.0, 0.01, 2.0, 0.01, nan) == MPC_E_ARG && says("episode_length_s"));
  EXPECT(h == nullptr);
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 0.0, 0.01, 2.0, 0.01, 20.0) == MPC_OK && h != nullptr);      // a limit of 0 N is allowed
  mpc_contact_destroy(h);
  h = nullptr;
  EXPECT(mpc_contact_create(&h, 4, &good, scales.data(), 100.0, 0.01, 2.0, 0.01, 20.0) == MPC_OK && h != nullptr);
  mpc_contact_destroy(nullptr);

  // ---- every call before a sim is bound: the arguments first, then "no sim bound"
  float *p = nullptr;
  int *q = nullptr;
  double *w = nullptr;
  double *const out5 = reinterpret_cast<double *>(uintptr_t(0x30000));
  EXPECT(mpc_contact_close(nullptr, ids, nullptr) == MPC_E_ARG && mpc_contact_close(h, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_close(h, ids, nullptr) == MPC_E_ARG && says("no sim bound"));
  EXPECT(mpc_contact_run(nullptr, rows, rows, rows, nullptr, ids, nullptr, nullptr, rows, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_run(h, nullptr, rows, rows, nullptr, ids, nullptr, nullptr, rows, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, nullptr, nullptr, nullptr, rows, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, ids, nullptr, nullptr, nullptr, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, ids, wide, nullptr, rows, nullptr, nullptr) == MPC_E_ARG && says("goes with shaping_scales"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, ids, nullptr, shaping.data(), rows, nullptr, nullptr) == MPC_E_ARG && says("goes with shaping_scales"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, ids, wide, bad_shaping.data(), rows, nullptr, nullptr) == MPC_E_ARG && says("shaping scale is not finite"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, ids, wide, shaping.data(), rows, wide, nullptr) == MPC_E_ARG && says("must not be d_shaping_terms"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, ids, wide, shaping.data(), rows, nullptr, nullptr) == MPC_E_ARG && says("no sim bound"));
  EXPECT(mpc_contact_run(h, rows, rows, rows, nullptr, ids, nullptr, nullptr, rows, nullptr, nullptr) == MPC_E_ARG && says("no sim bound"));
  EXPECT(mpc_contact_extend(nullptr, rows, 64, wide, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_extend(h, nullptr, 64, wide, nullptr) == MPC_E_ARG && mpc_contact_extend(h, rows, 64, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
  for (int Wp : {0, 8, 63, 65, 72, -16, 65552})
    EXPECT(mpc_contact_extend(h, rows, Wp, wide, nullptr) == MPC_E_ARG && says("multiple of 16"));
  EXPECT(mpc_contact_extend(h, odd, 64, wide, nullptr) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_contact_extend(h, rows, 64, at(0x14004), nullptr) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_contact_extend(h, rows, 64, rows, nullptr) == MPC_E_ARG && says("distinct"));
  EXPECT(mpc_contact_extend(h, rows, 64, at(0x10000 + 4 * (4 * 64 - 4)), nullptr) == MPC_E_ARG && says("distinct"));      // the last 16 bytes of the input
  EXPECT(mpc_contact_extend(h, at(0x10000 + 4 * (4 * 80 - 4)), 64, rows, nullptr) == MPC_E_ARG && says("distinct"));      // the last 16 bytes of the output
  EXPECT(mpc_contact_extend(h, rows, 64, at(0x10000 + 4 * (4 * 64)), nullptr) == MPC_E_ARG && says("no sim bound"));      // back to back is distinct
  EXPECT(mpc_contact_summary(nullptr, out5, nullptr) == MPC_E_ARG && mpc_contact_summary(h, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_summary(h, out5, nullptr) == MPC_E_ARG && says("no sim bound"));
  EXPECT(mpc_contact_new_window(nullptr, nullptr) == MPC_E_ARG && says("null handle"));
  EXPECT(mpc_contact_new_window(h, nullptr) == MPC_E_ARG && says("no sim bound"));
  EXPECT(mpc_contact_arrays(nullptr, &p, &q, &w) == MPC_E_ARG && mpc_contact_arrays(h, &p, &q, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_contact_arrays(h, &p, &q, &w) == MPC_E_ARG && says("no sim bound") && !p && !q && !w);

  // ---- bind: host structs that hold no device memory
  mpc_sim plain;                        // no friction record
  plain.n = 4;
  mpc_sim five;
  five.n = 5;
  five.friction = true;
  mpc_sim rowless;                      // as mpc_friction_attach leaves a sim that was given no output rows, short of the device array
  rowless.n = 4;
  rowless.friction = true;
  EXPECT(mpc_contact_bind(nullptr, &plain) == MPC_E_ARG && says("null handle"));
  EXPECT(mpc_contact_bind(h, nullptr) == MPC_E_ARG && says("null sim handle"));
  EXPECT(mpc_contact_bind(h, &five) == MPC_E_ARG && says("the sim has 5 robots, the contact terms 4 environments"));
  EXPECT(mpc_contact_bind(h, &plain) == MPC_E_ARG && says("no friction record"));
  EXPECT(mpc_contact_bind(h, &rowless) == MPC_E_ARG && says("no friction record"));
  EXPECT(mpc_contact_close(h, ids, nullptr) == MPC_E_ARG && says("no sim bound"));      // a refused bind leaves the handle unbound
  mpc_contact_destroy(h);

  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
