// Host emulation (TEST ONLY) + one more entry: the QP record of a robot as the assembler writes it (tests/test_kform_structure.py).
// That test compiles it with -DMPC_STRUCT_THETA_MAXT=0: the solver with the dense c Theta_ij, beside the structured one of tests/emu/Makefile's build.
#include "emu.cpp"

extern "C" {
int kform_qp_len(int h) {
#define EMU_CASE(HH) if (h == HH) return Cfg<HH>::QP_LEN;
  EMU_HORIZONS(EMU_CASE)
#undef EMU_CASE
  return -1;
}
int kform_qp_th1(int h) {
#define EMU_CASE(HH) if (h == HH) return Cfg<HH>::QP_TH1;
  EMU_HORIZONS(EMU_CASE)
#undef EMU_CASE
  return -1;
}
int kform_struct_theta(int h) {
#define EMU_CASE(HH) if (h == HH) return Solver<HH, HostExec<WThread<HH>, Cfg<HH>::TW>>::kStructTheta;
  EMU_HORIZONS(EMU_CASE)
#undef EMU_CASE
  return -1;
}
// model: {mass, inertia9[9]}; in: [56 + 4 h] floats; qp: [kform_qp_len(h)] out (a cold robot: the state record is all zeros)
int kform_qp_record(int h, const double *model, double dt, double alpha, const float *in, double *qp) {
  RobotModel mdl = make_model(model[0], model + 1, dt, alpha);
  std::vector<double> state(emu_state_len(h), 0.0), sc(emu_sc_len(h) > 0 ? emu_sc_len(h) : 1, 0.0);
  switch (h) {
#define EMU_CASE(HH) case HH: prep_one<HH>(mdl, in, state.data(), qp, sc.data(), false); return 0;
    EMU_HORIZONS(EMU_CASE)
#undef EMU_CASE
  }
  return -1;
}
}
