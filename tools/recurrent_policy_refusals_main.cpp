// recurrent_policy_refusals_main.cpp -- a stand-alone program over the host-only paths of the deployed recurrent weight policy's C ABI
// (csrc/mpc_recurrent_policy.h), tools/plant_rand_refusals_main.cpp's sibling: every refusal of create and step that comes back before the device is
// touched, and a valid create.  It needs no GPU; on a box without one the valid create answers MPC_E_NODEVICE, and that answer is checked too.  Built with
// the sanitizers on the HOST code of the unit, it is how those paths are checked for reads past the dims / weights / biases arrays, leaks of a refused
// handle and undefined behaviour:
//
//   cd rl-mpc-locomotion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//         ../../tools/recurrent_policy_refusals_main.cpp mpc_recurrent_policy.hip -o /tmp/recurrent_policy_refusals && /tmp/recurrent_policy_refusals
//
// Exit status 0 and "ok" on the last line when every call answered as expected and the sanitizers stayed silent.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../include/mpc_batch.h"
#include "../rl-mpc-locomotion_amd/csrc/mpc_recurrent_policy.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("line %d: %s\n", __LINE__, #cond);                    \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool says(const char *part) {
  const char *text = mpc_recurrent_policy_last_error();
  return text && std::strstr(text, part) != nullptr;
}

int main() {
  int ndev = 0;
  const bool device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  // exactly as many entries as a call may read: a read past them is a heap overflow here
  const int I = 48, H = 32;
  std::vector<float> w_ih(4 * H * I, 0.01f), w_hh(4 * H * H, 0.01f), b_ih(4 * H, 0.f), b_hh(4 * H, 0.f);
  std::vector<int> dims{H, 64, 12};
  std::vector<float> w0(64 * H, 0.01f), b0(64, 0.f), w1(12 * 64, 0.01f), b1(12, 0.f), scale(12, 1.f), shift(12, 0.f);
  std::vector<const float *> ws{w0.data(), w1.data()}, bs{b0.data(), b1.data()};
  mpc_recurrent_policy *p = nullptr;
  const auto create = [&](mpc_recurrent_policy **out, int i, int h, const float *a, const float *b, const float *c, const float *d, int layers, const int *dm,
                          const float *const *w, const float *const *bb, const float *sc, const float *sh) {
    const int rc = mpc_recurrent_policy_create(out, i, h, a, b, c, d, layers, dm, w, bb, sc, sh);
    if (rc != MPC_OK) EXPECT(p == nullptr);
    return rc;
  };
#define GOOD_LSTM w_ih.data(), w_hh.data(), b_ih.data(), b_hh.data()
#define GOOD_NET 2, dims.data(), ws.data(), bs.data(), scale.data(), shift.data()

  // create: null pointers
  EXPECT(create(nullptr, I, H, GOOD_LSTM, GOOD_NET) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, nullptr, w_hh.data(), b_ih.data(), b_hh.data(), GOOD_NET) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, w_ih.data(), nullptr, b_ih.data(), b_hh.data(), GOOD_NET) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, w_ih.data(), w_hh.data(), nullptr, b_hh.data(), GOOD_NET) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, w_ih.data(), w_hh.data(), b_ih.data(), nullptr, GOOD_NET) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, nullptr, ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, dims.data(), nullptr, bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, dims.data(), ws.data(), nullptr, scale.data(), shift.data()) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, dims.data(), ws.data(), bs.data(), nullptr, shift.data()) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, dims.data(), ws.data(), bs.data(), scale.data(), nullptr) == MPC_E_ARG && says("null argument"));
  // I, H
  for (int bad : {0, -16, 40}) {
    EXPECT(create(&p, bad, H, GOOD_LSTM, GOOD_NET) == MPC_E_ARG && says("input size") && says("not a positive multiple of 16"));
    EXPECT(create(&p, I, bad, GOOD_LSTM, GOOD_NET) == MPC_E_ARG && says("hidden size") && says("not a positive multiple of 16"));
  }
  // n_layers: refused before dims is read (dims has three entries)
  for (int bad : {0, -1, 9, 1000}) EXPECT(create(&p, I, H, GOOD_LSTM, bad, dims.data(), ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("layers: 1 .. 8"));
  // dims
  std::vector<int> d = dims;
  d[0] = 48;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, d.data(), ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("dims[0] = 48 inputs, the memory gives 32"));
  d = dims; d[2] = 17;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, d.data(), ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("17 outputs"));
  d = dims; d[2] = 0;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, d.data(), ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("0 outputs"));
  d = dims; d[1] = 40;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, d.data(), ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("dims[1] = 40 is not a positive multiple of 16"));
  d = dims; d[1] = -16;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, d.data(), ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("dims[1] = -16"));
  // a layer's pointers
  std::vector<const float *> holed = ws;
  holed[1] = nullptr;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, dims.data(), holed.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("layer 1: null"));
  holed = bs; holed[0] = nullptr;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, dims.data(), ws.data(), holed.data(), scale.data(), shift.data()) == MPC_E_ARG && says("layer 0: null"));
  // LDS: 16 (52 + 36 + 36 + W + 4) floats; W = 2448 is the first width over 160 KB.  Refused before a weight is read (the arrays are the small ones).
  d = dims; d[1] = 2448;
  EXPECT(create(&p, I, H, GOOD_LSTM, 2, d.data(), ws.data(), bs.data(), scale.data(), shift.data()) == MPC_E_ARG && says("164864 bytes of LDS"));
  // a valid create
  const int rc = create(&p, I, H, GOOD_LSTM, GOOD_NET);
  EXPECT(device ? rc == MPC_OK && p != nullptr : rc == MPC_E_NODEVICE && p == nullptr && says("no HIP device"));

  // step: every refusal comes before the handle is looked at, and the handle's own last (so they are reachable without a device)
  float *const obs = reinterpret_cast<float *>(uintptr_t(0x10000)), *const h = reinterpret_cast<float *>(uintptr_t(0x20000));      // never dereferenced
  float *const c = reinterpret_cast<float *>(uintptr_t(0x30000)), *const act = reinterpret_cast<float *>(uintptr_t(0x50000));
  float *const wts = reinterpret_cast<float *>(uintptr_t(0x60000));
  const long long *const reset = reinterpret_cast<const long long *>(uintptr_t(0x40000));
  const long long *const odd_reset = reinterpret_cast<const long long *>(uintptr_t(0x40004));
  EXPECT(mpc_recurrent_policy_step(p, 4, nullptr, h, c, reset, act, wts, nullptr) == MPC_E_ARG && says("is null"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, nullptr, c, reset, act, wts, nullptr) == MPC_E_ARG && says("is null"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h, nullptr, reset, act, wts, nullptr) == MPC_E_ARG && says("is null"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h, c, reset, act, nullptr, nullptr) == MPC_E_ARG && says("is null"));
  EXPECT(mpc_recurrent_policy_step(p, 0, obs, h, c, reset, act, wts, nullptr) == MPC_E_ARG && says("n must be at least 1"));
  EXPECT(mpc_recurrent_policy_step(p, -5, obs, h, c, reset, act, wts, nullptr) == MPC_E_ARG && says("n must be at least 1"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs + 1, h, c, reset, act, wts, nullptr) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h + 2, c, reset, act, wts, nullptr) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h, c + 3, reset, act, wts, nullptr) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h, c, reset, act + 1, wts, nullptr) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h, c, reset, act, wts + 2, nullptr) == MPC_E_ARG && says("16-byte aligned"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h, c, odd_reset, act, wts, nullptr) == MPC_E_ARG && says("d_reset must be 8-byte aligned"));
  EXPECT(mpc_recurrent_policy_step(p, 4, obs, h, h, reset, act, wts, nullptr) == MPC_E_ARG && says("d_h and d_c"));
  EXPECT(mpc_recurrent_policy_step(nullptr, 4, obs, h, c, reset, act, wts, nullptr) == MPC_E_ARG && says("null handle"));
  EXPECT(mpc_recurrent_policy_step(nullptr, 4, obs, h, c, nullptr, nullptr, wts, nullptr) == MPC_E_ARG && says("null handle"));      // both are optional
  mpc_recurrent_policy_destroy(nullptr);
  mpc_recurrent_policy_destroy(p);
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
