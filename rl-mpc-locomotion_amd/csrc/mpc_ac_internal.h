// mpc_ac_internal.h -- what the library's other units may know of an mpc_ac (include/mpc_ppo.h): its two stacks and the parameter addresses that
// mpc_ac_bind keeps.  mpc_ppo.hip owns the handle and fills this view; mpc_ppo_update.hip reads the same addresses, so the update writes the weights
// where mpc_ac_act reads them.  Not part of the C ABI.
#pragma once

struct mpc_ac;

struct mpc_ac_view {
  static constexpr int kMaxLayers = 8;   // MPC_AC_MAX_LAYERS
  int n_layers[2];                       // actor, critic
  int dims[2][kMaxLayers + 1];
  const float *w[2][kMaxLayers];         // [dims[l+1]][dims[l]] row-major
  const float *b[2][kMaxLayers];
  const float *std;                      // [12]
  int device;
  bool bound;
  bool asymmetric;                       // made by mpc_ac_create_asymmetric: the critic's rows are not the actor's (dims[1][0] may differ from dims[0][0])
};

// false for a null handle
bool mpc_ac_get_view(const mpc_ac *ac, mpc_ac_view *out);
// the error text of mpc_ppo_last_error (thread-local, owned by mpc_ppo.hip); returns code
int mpc_ppo_set_error(int code, const char *message);
