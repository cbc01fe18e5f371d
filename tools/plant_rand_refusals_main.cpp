// plant_rand_refusals_main.cpp -- a stand-alone program over the host-only paths of the per-robot plant randomisation's C ABI
// (csrc/mpc_plant_rand.h) and of the plant entry points of the critic's row (csrc/mpc_privileged_obs.h), tools/abi_refusals_main.cpp's sibling:
// create and destroy, and every refusal that comes back before the device is touched.  It needs no GPU; on a box without one a valid create
// answers MPC_E_NODEVICE, and that answer is checked too.  Built with the sanitizers on the HOST code of the units, it is how those paths are
// checked for reads past the present / ranges arrays, leaks of a refused handle and undefined behaviour:
//
//   cd rl-mpc-locomotion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//         ../../tools/plant_rand_refusals_main.cpp mpc_plant_rand.hip mpc_privileged_obs.hip -o /tmp/plant_rand_refusals && /tmp/plant_rand_refusals
//
// Exit status 0 and "ok" on the last line when every call answered as expected and the sanitizers stayed silent.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../include/mpc_batch.h"
#include "../rl-mpc-locomotion_amd/csrc/mpc_plant_rand.h"
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
  int ndev = 0;
  const bool device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int *const ids = reinterpret_cast<const int *>(uintptr_t(0x10000));      // never dereferenced
  mpc_sim *const no_sim = nullptr;
  // exactly as many entries as a call may read: a read past them is a heap overflow here
  std::vector<int> all{1, 1, 1}, none{0, 0, 0}, only_strength{0, 1, 0};
  std::vector<double> good{-1.0, 3.0, 0.9, 1.1, -1.0, 1.0};

  mpc_plant_rand *h = nullptr;
  EXPECT(mpc_plant_rand_create(nullptr, 4, 7) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "null argument"));
  EXPECT(mpc_plant_rand_create(&h, 0, 7) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "n must be at least 1") && h == nullptr);
  EXPECT(mpc_plant_rand_create(&h, -3, 7) == MPC_E_ARG && h == nullptr);
  const int rc = mpc_plant_rand_create(&h, 4, 7);
  EXPECT(device ? rc == MPC_OK && h != nullptr : rc == MPC_E_NODEVICE && h == nullptr && says(mpc_plant_rand_last_error(), "no HIP device"));

  // the calls that need no handle to refuse; draw checks its ranges before it looks at its handle
  EXPECT(mpc_plant_rand_attach(nullptr, no_sim) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "null handle"));
  EXPECT(mpc_plant_rand_draw(h, ids, 4, nullptr, good.data(), nullptr) == MPC_E_ARG && mpc_plant_rand_draw(h, ids, 4, all.data(), nullptr, nullptr) == MPC_E_ARG);
  EXPECT(says(mpc_plant_rand_last_error(), "null argument"));
  EXPECT(mpc_plant_rand_draw(h, ids, -1, all.data(), good.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "negative"));
  std::vector<double> r = good;
  r[1] = inf;
  EXPECT(mpc_plant_rand_draw(h, ids, 4, all.data(), r.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "payload range must be finite"));
  r = good; r[4] = nan;
  EXPECT(mpc_plant_rand_draw(h, ids, 4, all.data(), r.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "gravity range must be finite"));
  r = good; r[5] = 1e39;                    // finite as a double, not as the float32 the kernel draws with
  EXPECT(mpc_plant_rand_draw(h, ids, 4, all.data(), r.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "gravity range must be finite"));
  r = good; r[0] = 4.0;
  EXPECT(mpc_plant_rand_draw(h, ids, 4, all.data(), r.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "payload range with lo > hi"));
  r = good; r[2] = -0.5;
  EXPECT(mpc_plant_rand_draw(h, ids, 4, all.data(), r.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "strength lo must be >= 0"));
  // an absent axis is not read: its (bad) bounds do not matter, and the call gets as far as the handle
  const char *const next = h ? "no sim attached" : "null handle";
  r = good; r[0] = nan; r[5] = -inf;
  EXPECT(mpc_plant_rand_draw(h, ids, 4, only_strength.data(), r.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), next));
  EXPECT(mpc_plant_rand_draw(h, ids, 4, none.data(), good.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), next));
  EXPECT(mpc_plant_rand_draw(h, ids, 4, all.data(), good.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), next));
  std::vector<double> rec(12, 0.0);
  std::vector<unsigned> cnt(4, 0u);
  EXPECT(mpc_plant_rand_get_params(nullptr, rec.data()) == MPC_E_ARG && mpc_plant_rand_set_params(nullptr, rec.data(), nullptr) == MPC_E_ARG);
  EXPECT(mpc_plant_rand_get_counters(nullptr, cnt.data()) == MPC_E_ARG && mpc_plant_rand_set_counters(nullptr, cnt.data()) == MPC_E_ARG);
  mpc_plant_rand_destroy(nullptr);

  if (h) {      // with a device: what a handle refuses before it touches it (nothing is attached, so nothing ever launches)
    EXPECT(mpc_plant_rand_attach(h, no_sim) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "null sim handle"));
    EXPECT(mpc_plant_rand_draw(h, nullptr, 3, all.data(), good.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "k must be n"));
    EXPECT(mpc_plant_rand_get_params(h, nullptr) == MPC_E_ARG && mpc_plant_rand_get_params(h, rec.data()) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "no sim attached"));
    for (int r4 = 0; r4 < 4; ++r4) { rec[3 * r4] = 0.5; rec[3 * r4 + 1] = 1.0; rec[3 * r4 + 2] = -9.81; }
    std::vector<double> mass(4, 10.0);
    EXPECT(mpc_plant_rand_set_params(h, rec.data(), mass.data()) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "no sim attached"));
    rec[3 * 3 + 2] = nan;
    EXPECT(mpc_plant_rand_set_params(h, rec.data(), mass.data()) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "robot 3 is not finite"));
    rec[3 * 3 + 2] = -9.81; rec[3 * 2 + 1] = -0.1;
    EXPECT(mpc_plant_rand_set_params(h, rec.data(), mass.data()) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "strength of robot 2"));
    rec[3 * 2 + 1] = 1.0; rec[3 * 1] = -10.0;
    EXPECT(mpc_plant_rand_set_params(h, rec.data(), mass.data()) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "payload of robot 1"));
    EXPECT(mpc_plant_rand_set_params(h, rec.data(), nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "no sim attached"));      // unchecked without masses
    EXPECT(mpc_plant_rand_get_counters(h, cnt.data()) == MPC_E_ARG && mpc_plant_rand_set_counters(h, cnt.data()) == MPC_E_ARG);
    EXPECT(mpc_plant_rand_set_counters(h, nullptr) == MPC_E_ARG && says(mpc_plant_rand_last_error(), "null argument"));
    mpc_plant_rand_destroy(h);
  }

  // the plant entry points of the critic's row: host-only handles
  EXPECT(mpc_privobs_width_plant(0) == 64 && mpc_privobs_width_plant(8) == 64 && mpc_privobs_width_plant(9) == 80 && mpc_privobs_width_plant(187) == 256);
  EXPECT(mpc_privobs_width_plant(-1) == MPC_E_ARG && mpc_privobs_width_plant(209) == MPC_E_ARG && says(mpc_privobs_last_error(), "mpc_privobs_width_plant"));
  mpc_privobs *v = nullptr;
  EXPECT(mpc_privobs_create(&v, 4) == MPC_OK && v != nullptr);
  EXPECT(mpc_privobs_bind_plant(nullptr, no_sim) == MPC_E_ARG && says(mpc_privobs_last_error(), "null handle"));
  EXPECT(mpc_privobs_bind_plant(v, no_sim) == MPC_E_ARG && says(mpc_privobs_last_error(), "null sim handle"));
  float *const p = reinterpret_cast<float *>(uintptr_t(0x10000)), *const q = reinterpret_cast<float *>(uintptr_t(0x20000));
  const long long *prog = reinterpret_cast<const long long *>(uintptr_t(0x30000));
  EXPECT(mpc_privobs_run_plant(nullptr, p, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "mpc_privobs_run_plant: null"));
  EXPECT(mpc_privobs_run_plant(v, p, 48, 209, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "P must"));
  EXPECT(mpc_privobs_run_plant(v, p, 62, 15, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "obs_width"));
  EXPECT(mpc_privobs_run_plant(v, p + 1, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "16-byte"));
  EXPECT(mpc_privobs_run_plant(v, p, 64, 0, prog, 0.001, p, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "must not be"));
  EXPECT(mpc_privobs_run_plant(v, p, 48, 0, prog, inf, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "inv_len"));
  EXPECT(mpc_privobs_run_plant(v, p, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "mpc_privobs_run_plant: no sim bound"));
  EXPECT(mpc_privobs_run(v, p, 48, 0, prog, 0.001, q, nullptr) == MPC_E_ARG && says(mpc_privobs_last_error(), "mpc_privobs_run: no sim bound"));
  mpc_privobs_destroy(v);
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
