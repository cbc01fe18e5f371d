// recurrent_bptt_refusals_main.cpp -- a stand-alone program over the host-only paths of the update through time's C ABI (csrc/mpc_recurrent_bptt.h),
// tools/recurrent_policy_refusals_main.cpp's sibling: every refusal of create, bind, forward, backward, weight_gradients and dgates that comes back
// before the device is touched, and a valid create (host only: it succeeds without a GPU).  On a box without a GPU the bind of real host arrays answers
// MPC_E_NODEVICE, and that answer is checked too.  Built with the sanitizers on the HOST code of the unit, it is how those paths are checked for reads
// past the size arrays and the io / grads records, leaks of a handle and undefined behaviour:
//
//   cd rl-mpc-locomotion_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//         ../../tools/recurrent_bptt_refusals_main.cpp mpc_recurrent_bptt.hip mpc_ppo_gemm.hip -o /tmp/recurrent_bptt_refusals && /tmp/recurrent_bptt_refusals
// (mpc_ppo_gemm.hip: the weight-gradient GEMMs mpc_recurrent_bptt.hip launches live in that unit.)
//
// Exit status 0 and "ok" on the last line when every call answered as expected and the sanitizers stayed silent.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../include/mpc_batch.h"
#include "../rl-mpc-locomotion_amd/csrc/mpc_recurrent_bptt.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("line %d: %s\n", __LINE__, #cond);                    \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static bool says(const char *part) {
  const char *text = mpc_recurrent_bptt_last_error();
  return text && std::strstr(text, part) != nullptr;
}

template <typename T>
static T *at(uintptr_t address) { return reinterpret_cast<T *>(address); }      // never dereferenced

int main() {
  int ndev = 0;
  const bool device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  // exactly as many entries as a call may read: a read past them is a heap overflow here
  std::vector<int> I2{48, 64}, H2{32, 32}, I1{16}, H1{624};
  mpc_recurrent_bptt *h = nullptr;
  const auto create = [&](mpc_recurrent_bptt **out, int memories, const int *I, const int *H, int steps, int rows) {
    const int rc = mpc_recurrent_bptt_create(out, memories, I, H, steps, rows);
    if (rc != MPC_OK) EXPECT(h == nullptr);
    return rc;
  };
  // create
  EXPECT(create(nullptr, 2, I2.data(), H2.data(), 6, 40) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&h, 2, nullptr, H2.data(), 6, 40) == MPC_E_ARG && says("null argument"));
  EXPECT(create(&h, 2, I2.data(), nullptr, 6, 40) == MPC_E_ARG && says("null argument"));
  for (int bad : {0, -1, 3, 1000}) EXPECT(create(&h, bad, I2.data(), H2.data(), 6, 40) == MPC_E_ARG && says("one or two memories"));      // before a size is read
  for (int bad : {0, -16, 40}) {
    std::vector<int> v{48, bad};
    EXPECT(create(&h, 2, v.data(), H2.data(), 6, 40) == MPC_E_ARG && says("memory 1: the input size") && says("not a positive multiple of 16"));
    v = {bad, 32};
    EXPECT(create(&h, 2, I2.data(), v.data(), 6, 40) == MPC_E_ARG && says("memory 0: the hidden size") && says("not a positive multiple of 16"));
  }
  for (int bad : {0, -1}) {
    EXPECT(create(&h, 2, I2.data(), H2.data(), bad, 40) == MPC_E_ARG && says("max_steps must be at least 1"));
    EXPECT(create(&h, 2, I2.data(), H2.data(), 6, bad) == MPC_E_ARG && says("max_rows must be at least 1"));
  }
  std::vector<int> wide{1024}, h256{256}, h640{640};
  EXPECT(create(&h, 1, wide.data(), h256.data(), 6, 40) == MPC_E_ARG && says("forward pass") && says("164864 bytes of LDS"));
  EXPECT(create(&h, 1, I1.data(), h640.data(), 6, 40) == MPC_E_ARG && says("backward pass") && says("164096 bytes of LDS"));
  EXPECT(create(&h, 1, I1.data(), h256.data(), 1 << 12, 1 << 12) == MPC_E_ARG && says("2^31"));
  EXPECT(mpc_recurrent_bptt_workspace_bytes(nullptr) == -1);
  EXPECT(create(&h, 1, I1.data(), H1.data(), 6, 40) == MPC_OK && h != nullptr);      // the widest state: 160 000 bytes of LDS
  mpc_recurrent_bptt_destroy(h);
  h = nullptr;
  // a valid create: host memory only, with or without a device
  EXPECT(create(&h, 2, I2.data(), H2.data(), 6, 40) == MPC_OK && h != nullptr);
  const long long R = 6 * 40;
  const auto per_memory = [&](long long I, long long H) { return 4 * (11 * H * R + 4 * H * 64 + (4 * H * I + 4 * H * H + 4 * H)) + 8 * R; };
  EXPECT(mpc_recurrent_bptt_workspace_bytes(h) == per_memory(48, 32) + per_memory(64, 32) + 4 * R);

  // bind
  std::vector<const float *> good{at<const float>(0x10000), at<const float>(0x20000)}, holed{at<const float>(0x10000), nullptr},
      odd{at<const float>(0x10004), at<const float>(0x20000)};
  EXPECT(mpc_recurrent_bptt_bind(nullptr, good.data(), good.data(), good.data(), good.data()) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_recurrent_bptt_bind(h, good.data(), nullptr, good.data(), good.data()) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_recurrent_bptt_bind(h, good.data(), holed.data(), good.data(), good.data()) == MPC_E_ARG && says("memory 1: null parameter"));
  EXPECT(mpc_recurrent_bptt_bind(h, good.data(), good.data(), odd.data(), good.data()) == MPC_E_ARG && says("memory 0") && says("16-byte aligned"));

  // forward: every refusal comes before the parameters are asked for, and "no parameters bound" last (so they are reachable without a device)
  const mpc_recurrent_bptt_io ok_a{at<const float>(0x100000), 40 * 48, at<const float>(0x200000), at<const float>(0x300000), at<float>(0x400000), at<float>(0x500000)};
  const mpc_recurrent_bptt_io ok_c{at<const float>(0x600000), 40 * 64, at<const float>(0x700000), at<const float>(0x800000), at<float>(0x900000), at<float>(0xa00000)};
  std::vector<mpc_recurrent_bptt_io> io{ok_a, ok_c};
  const long long *const reset = at<const long long>(0x70008);
  EXPECT(mpc_recurrent_bptt_forward(nullptr, 6, 40, 0, 2, io.data(), reset, nullptr) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, nullptr, reset, nullptr) == MPC_E_ARG && says("null argument"));
  for (int bad : {0, -2, 7}) EXPECT(mpc_recurrent_bptt_forward(h, bad, 40, 0, 2, io.data(), reset, nullptr) == MPC_E_ARG && says("is outside 1 .. 6 (max_steps)"));
  for (int bad : {0, -2, 41}) EXPECT(mpc_recurrent_bptt_forward(h, 6, bad, 0, 2, io.data(), reset, nullptr) == MPC_E_ARG && says("is outside 1 .. 40 (max_rows)"));
  EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 1, 2, io.data(), reset, nullptr) == MPC_E_ARG && says("memories 1 .. 2"));      // before io[1] would be memory 2's
  EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 0, io.data(), reset, nullptr) == MPC_E_ARG && says("memories"));
  EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, -1, 1, io.data(), reset, nullptr) == MPC_E_ARG && says("memories"));
  EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, io.data(), at<const long long>(0x70004), nullptr) == MPC_E_ARG && says("d_reset must be 8-byte aligned"));
  {
    auto v = io; v[1].d_x = nullptr;
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("memory 1") && says("is null"));
    v = io; v[0].d_h0 = nullptr;
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("memory 0") && says("is null"));
    v = io; v[0].d_c0 = nullptr;
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("is null"));
    v = io; v[1].d_y = nullptr;
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("is null"));
    v = io; v[0].d_x = at<const float>(0x100008);
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("16-byte aligned"));
    v = io; v[1].d_c_last = at<float>(0xa00004);
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("memory 1") && says("16-byte aligned"));
    v = io; v[0].x_stride = 32;
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("the x stride 32 must be a multiple of 4 floats and at least 48"));
    v = io; v[0].x_stride = 50;
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("the x stride 50"));
    v = io; v[1].x_stride = 48;
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("memory 1: the x stride 48"));
    v = io; v[0].d_c_last = at<float>(0x400000 + 4 * 7680 - 16);      // inside y
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("must not overlap"));
    v = io; v[1].d_y = at<float>(0x400010);                           // the critic's y inside the actor's
    EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, v.data(), reset, nullptr) == MPC_E_ARG && says("must not overlap"));
  }
  EXPECT(mpc_recurrent_bptt_forward(h, 6, 40, 0, 2, io.data(), reset, nullptr) == MPC_E_ARG && says("no parameters bound"));
  {
    std::vector<mpc_recurrent_bptt_io> one{ok_c};                       // exactly one record for count = 1; c_last and d_reset are optional
    one[0].d_c_last = nullptr;
    EXPECT(mpc_recurrent_bptt_forward(h, 1, 1, 1, 1, one.data(), nullptr, nullptr) == MPC_E_ARG && says("no parameters bound"));
  }

  // backward and weight_gradients
  const mpc_recurrent_bptt_grads g_a{at<const float>(0x100000), at<float>(0x200000), at<float>(0x300000), at<float>(0x400000), at<float>(0x500000)};
  const mpc_recurrent_bptt_grads g_c{at<const float>(0x600000), at<float>(0x700000), at<float>(0x800000), at<float>(0x900000), at<float>(0xa00000)};
  std::vector<mpc_recurrent_bptt_grads> gr{g_a, g_c};
  for (auto *entry : {mpc_recurrent_bptt_backward, mpc_recurrent_bptt_weight_gradients}) {
    EXPECT(entry(nullptr, 6, 40, 0, 2, gr.data(), nullptr) == MPC_E_ARG && says("null argument"));
    EXPECT(entry(h, 6, 40, 0, 2, nullptr, nullptr) == MPC_E_ARG && says("null argument"));
    EXPECT(entry(h, 7, 40, 0, 2, gr.data(), nullptr) == MPC_E_ARG && says("T = 7 is outside"));
    EXPECT(entry(h, 6, 41, 0, 2, gr.data(), nullptr) == MPC_E_ARG && says("B = 41 is outside"));
    EXPECT(entry(h, 6, 40, 0, 3, gr.data(), nullptr) == MPC_E_ARG && says("memories 0 .. 2"));
    auto v = gr; v[0].d_dy = nullptr;
    EXPECT(entry(h, 6, 40, 0, 2, v.data(), nullptr) == MPC_E_ARG && says("memory 0") && says("is null"));
    v = gr; v[1].d_b_hh = nullptr;
    EXPECT(entry(h, 6, 40, 0, 2, v.data(), nullptr) == MPC_E_ARG && says("memory 1") && says("is null"));
    v = gr; v[1].d_w_hh = at<float>(0x800004);
    EXPECT(entry(h, 6, 40, 0, 2, v.data(), nullptr) == MPC_E_ARG && says("memory 1") && says("16-byte aligned"));
    v = gr; v[0].d_b_hh = at<float>(0x400000 + 4 * 128 - 16);          // inside db_ih
    EXPECT(entry(h, 6, 40, 0, 2, v.data(), nullptr) == MPC_E_ARG && says("must not overlap"));
    v = gr; v[1].d_w_ih = at<float>(0x300000);                         // the actor's dW_hh
    EXPECT(entry(h, 6, 40, 0, 2, v.data(), nullptr) == MPC_E_ARG && says("must not overlap"));
    EXPECT(entry(h, 6, 40, 0, 2, gr.data(), nullptr) == MPC_E_ARG && says("no forward call to go back through"));
  }

  // dgates
  const float *where = nullptr;
  EXPECT(mpc_recurrent_bptt_dgates(nullptr, 0, &where) == MPC_E_ARG && says("null argument"));
  EXPECT(mpc_recurrent_bptt_dgates(h, 0, nullptr) == MPC_E_ARG && says("null argument"));
  for (int bad : {-1, 2}) EXPECT(mpc_recurrent_bptt_dgates(h, bad, &where) == MPC_E_ARG && says("of a handle with 2"));
  EXPECT(mpc_recurrent_bptt_dgates(h, 1, &where) == MPC_E_ARG && says("no workspace before mpc_recurrent_bptt_bind") && where == nullptr);

  // a bind of (never dereferenced) aligned pointers: the workspace is allocated where there is a device, MPC_E_NODEVICE where there is none
  const int rc = mpc_recurrent_bptt_bind(h, good.data(), good.data(), good.data(), good.data());
  EXPECT(device ? rc == MPC_OK : rc == MPC_E_NODEVICE && says("no HIP device"));
  mpc_recurrent_bptt_destroy(nullptr);
  mpc_recurrent_bptt_destroy(h);
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
