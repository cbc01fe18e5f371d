// recurrent_host.h -- what mpc_recurrent and mpc_recurrent_bptt (and, for the sizes, mpc_recurrent_policy) ask of a memory on the host, beside
// recurrent_cell.h's device code.  Each returns the refusal's text, to follow the entry point's own name, or "" where there is nothing to
// refuse.  Host only.
#pragma once
#include <string>

#include "mpc_host.h"
#include "recurrent_cell.h"

namespace recurrent {

inline std::string size_refusal(int I, int H) {
  if (I <= 0 || I % 16 != 0) return "the input size " + std::to_string(I) + " is not a positive multiple of 16";
  if (H <= 0 || H % 16 != 0) return "the hidden size " + std::to_string(H) + " is not a positive multiple of 16";
  return "";
}

// nn.LSTM's four parameter arrays of every memory, as the bind entry points take them: one array of `memories` pointers each
struct Parameters { const float *const *w_ih, *const *w_hh, *const *b_ih, *const *b_hh; };
inline std::string bind_refusal(const Parameters &p, int memories) {
  if (!p.w_ih || !p.w_hh || !p.b_ih || !p.b_hh) return "null argument";
  for (int k = 0; k < memories; ++k) {
    if (!p.w_ih[k] || !p.w_hh[k] || !p.b_ih[k] || !p.b_hh[k]) return "memory " + std::to_string(k) + ": null parameter pointer";
    if (!mpchost::aligned16(p.w_ih[k]) || !mpchost::aligned16(p.w_hh[k]) || !mpchost::aligned16(p.b_ih[k]) || !mpchost::aligned16(p.b_hh[k]))
      return "memory " + std::to_string(k) + ": every parameter pointer must be 16-byte aligned";
  }
  return "";
}
inline void bind(Cell *cell, const Parameters &p, int memories) {
  for (int k = 0; k < memories; ++k) cell[k] = Cell{cell[k].I, cell[k].H, p.w_ih[k], p.w_hh[k], p.b_ih[k], p.b_hh[k]};
}

}  // namespace recurrent
