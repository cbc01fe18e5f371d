// toy_sim.h -- the toy plant of the closed-loop tests as one robot's float64 state and two functions, shared by the device kernel
// (mpc_sim.hip, one lane per robot) and host C++ (the CPU tests compile this header with g++ and compare it with the numpy model).
//
// A TOY, not a physics engine: one rigid body under gravity; a leg in contact holds its foot at a world anchor (no slip) and pushes the
// body with F = -R J^-T tau, its joint angles following from the anchor by inverse kinematics; a leg that would pull on the ground by more
// than RELEASE_N lets go; a leg in the air is three independent damped joints of inertia I_J (massless for the body) and touches down where
// its foot path crosses the ground.  No articulated dynamics, no joint limits; no friction cone either unless the step is given one (below).
//
// The ground is a template parameter of toy_init / toy_step: Plane (z = gx x + gy y, the numpy ToyRobot's) or HeightField (an int16 grid
// meshed into triangles as Isaac Gym's convert_heightfield_to_trimesh splits its cells; tests/toy_terrain.py's ToyTerrainRobot).  It appears
// in two roles: its height (initial stance, touch-down test and crossing, the anchor's z, the fall test under the base) and its normal for the
// lift-off test f . n, taken under the leg's anchor.  The (..., gx, gy) signatures are wrappers over Plane.
//
// A robot may carry a plant record of its own (kPlant doubles: payload [kg], motor strength [factor], gravity z [m/s^2, absolute]; neutral
// (0, 1, kGravZ)): toy_step_plant steps with mass + payload, every torque times the strength (stance force and swing-joint acceleration both see
// the scaled torque) and that gravity.  The inertia is NOT changed by the payload: Isaac Gym's added base mass (legged_gym's randomize_base_mass)
// changes the body's mass property and leaves its inertia alone as well.  With the neutral record mass + 0.0, tau * 1.0 and kGravZ are exact, so
// toy_step_plant reproduces toy_step bit for bit.
//
// The contact is a template parameter of the step as well: NoFriction (the anchor holds whatever the leg asks of it; what every function named
// toy_step* steps with) or Coulomb (toy_step_friction): a stance leg's force f, after the lift-off tests, is split along the normal n under its
// anchor, ft = f - fn n, and where |ft| > mu fn the ground supplies only fn n + mu fn t (t = ft / |ft|) and the massless foot slides: its anchor
// moves against t by h (|ft| - mu fn) / kSlipDamp, a viscous regularisation, and is put back on the ground.  The lever arm is the foot's position
// before the slide, the normal the one under the anchor before it; the substep's closing inverse kinematics follows the moved anchor.  No new
// state.  Coulomb also reports force[4][3], the world-frame ground reaction of the tick's last substep (zero for a leg in the air, a leg that let
// go or one with fn < 0), and slip[4], the distance slid over the tick.  mu >= 0; with mu = +inf nothing ever exceeds the limit (inf * 0 is NaN
// and compares false) and the step reproduces the NoFriction one bit for bit; mu = 0 leaves the normal force alone.
//
// toy_init / toy_step restate ToyRobot.__init__ / ToyRobot.step of the numpy model operation for operation in float64 (same order of the
// sums, legs 0..3, +0.0 start; 4 IK iterations per substep, 20 at initialisation; 3 x 3 systems solved as LAPACK's dgesv does: partial
// pivoting, multipliers a * (1 / pivot), forward then backward substitution).  Compile with -ffp-contract=off: no fused multiply-adds.
#pragma once

#include <math.h>

#ifndef MPC_HD
#if defined(__HIPCC__)
#define MPC_HD __host__ __device__ __forceinline__
#else
#define MPC_HD inline
#endif
#endif

namespace toysim {

constexpr int kSubsteps = 4;
constexpr double kIJ = 0.005;          // joint inertia of a leg in the air [kg m^2]
constexpr double kBJ = 0.05;           // and its viscous damping [N m s]
constexpr int kLiftTicks = 3;          // ticks after lift-off during which a foot cannot touch down again
constexpr double kReleaseN = 5.0;      // pull [N] at which a foot in contact lets go
constexpr double kReg = 1e-9;          // added to the diagonal of the leg Jacobian systems
constexpr double kGravZ = -9.81;
constexpr double kSlipDamp = 200.0;    // viscous coefficient of a sliding foot [N s/m] (Coulomb)

// columns of quadruped.ROBOT_TABLE64 (COL_ABAD ... COL_HEIGHT) and its row length
constexpr int kColAbad = 0, kColHip = 1, kColKnee = 2, kColHiploc = 3, kColMass = 6, kColInertia = 7, kColHeight = 10, kRobotCols = 25;

// per-robot state record of mpc_sim_get_state / mpc_sim_set_state (include/mpc_sim.h)
constexpr int kF64 = 49;               // pos3 quat4 (xyzw) v3 w3 q12 qd12 anchor12
constexpr int kI32 = 9;                // contact4 lift4 fell
// per-robot plant record (mpc_sim's d_plant, csrc/mpc_plant_rand.h): payload, strength, grav_z
constexpr int kPlant = 3;
constexpr int kPlantPayload = 0, kPlantStrength = 1, kPlantGravZ = 2;
constexpr int kOffPos = 0, kOffQuat = 3, kOffV = 7, kOffW = 10, kOffQ = 13, kOffQd = 25, kOffAnchor = 37;

struct Params {
  double abad, hip, knee, mass, height;
  double hiploc[4][3];
  double inertia[3];
};

struct State {
  double pos[3], quat[4], v[3], w[3];
  double q[4][3], qd[4][3], anchor[4][3];
  int contact[4], lift[4], fell;
};

MPC_HD double side_of(int l) { return (l & 1) ? -1.0 : 1.0; }            // FL FR RL RR
MPC_HD double hip_sx(int l) { return l < 2 ? 1.0 : -1.0; }
MPC_HD double hip_sy(int l) { return (l & 1) ? -1.0 : 1.0; }

MPC_HD void params_from_row(Params &p, const double *r) {
  p.abad = r[kColAbad]; p.hip = r[kColHip]; p.knee = r[kColKnee];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    p.hiploc[l][0] = r[kColHiploc] * hip_sx(l);
    p.hiploc[l][1] = r[kColHiploc + 1] * hip_sy(l);
    p.hiploc[l][2] = r[kColHiploc + 2];
  }
  p.mass = r[kColMass];
  p.inertia[0] = r[kColInertia]; p.inertia[1] = r[kColInertia + 1]; p.inertia[2] = r[kColInertia + 2];
  p.height = r[kColHeight];
}

MPC_HD void sin_cos(double x, double &s, double &c) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincos(x, &s, &c);
#else
  s = sin(x); c = cos(x);
#endif
}

// xyzw, body -> world
MPC_HD void quat_to_rot(const double *q, double R[3][3]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0][0] = 1 - 2 * (y * y + z * z); R[0][1] = 2 * (x * y - z * w); R[0][2] = 2 * (x * z + y * w);
  R[1][0] = 2 * (x * y + z * w); R[1][1] = 1 - 2 * (x * x + z * z); R[1][2] = 2 * (y * z - x * w);
  R[2][0] = 2 * (x * z - y * w); R[2][1] = 2 * (y * z + x * w); R[2][2] = 1 - 2 * (x * x + y * y);
}

MPC_HD void mat_vec(const double R[3][3], const double *v, double *o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2];
}

MPC_HD void mat_t_vec(const double R[3][3], const double *v, double *o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = R[0][i] * v[0] + R[1][i] * v[1] + R[2][i] * v[2];
}

MPC_HD void cross(const double *a, const double *b, double *o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

MPC_HD double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
MPC_HD double norm3(const double *a) { return sqrt(dot3(a, a)); }

// x = A^-1 b as LAPACK dgesv (dgetrf: partial pivoting on the first largest |a|, column scaled by 1 / pivot, rank-1 update; dgetrs: the row
// interchanges on b, unit-lower forward and upper backward substitution).  A and b are overwritten.
MPC_HD void solve3(double A[3][3], double *b) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int p = k;
    double best = fabs(A[k][k]);
#pragma unroll
    for (int i = k + 1; i < 3; ++i) {
      const double a = fabs(A[i][k]);
      if (a > best) { best = a; p = i; }
    }
    // the interchange as selects (static register indices on the device)
#pragma unroll
    for (int i = k + 1; i < 3; ++i) {
      const bool sw = p == i;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double t = A[k][j];
        A[k][j] = sw ? A[i][j] : t;
        A[i][j] = sw ? t : A[i][j];
      }
      const double t = b[k];
      b[k] = sw ? b[i] : t;
      b[i] = sw ? t : b[i];
    }
    const double inv = 1.0 / A[k][k];
#pragma unroll
    for (int i = k + 1; i < 3; ++i) A[i][k] = A[i][k] * inv;
#pragma unroll
    for (int i = k + 1; i < 3; ++i)
#pragma unroll
      for (int j = k + 1; j < 3; ++j) A[i][j] = A[i][j] - A[i][k] * A[k][j];
  }
  // (b's interchanges were applied above in the order of dgetrs' ipiv; the substitutions follow them as there)
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = k + 1; i < 3; ++i) b[i] = b[i] - b[k] * A[i][k];
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    b[k] = b[k] / A[k][k];
#pragma unroll
    for (int i = 0; i < k; ++i) b[i] = b[i] - b[k] * A[i][k];
  }
}

// foot position in the hip frame and its Jacobian (leg_fk_jac of the numpy model)
MPC_HD void leg_fk_jac(const double *q, double side, const Params &P, double *p, double J[3][3]) {
  const double dy = P.abad * side, dz1 = -P.hip, dz2 = -P.knee;
  double s1, s2, s3, c1, c2, c3;
  sin_cos(q[0], s1, c1); sin_cos(q[1], s2, c2); sin_cos(q[2], s3, c3);
  const double c23 = c2 * c3 - s2 * s3, s23 = s2 * c3 + c2 * s3;
  p[0] = dz2 * s23 + dz1 * s2;
  p[1] = dy * c1 - dz1 * c2 * s1 - dz2 * s1 * c23;
  p[2] = dy * s1 + dz1 * c1 * c2 + dz2 * c1 * c23;
  J[0][0] = 0.0; J[0][1] = dz2 * c23 + dz1 * c2; J[0][2] = dz2 * c23;
  J[1][0] = -dy * s1 - dz2 * c1 * c23 - dz1 * c1 * c2; J[1][1] = dz2 * s1 * s23 + dz1 * s1 * s2; J[1][2] = dz2 * s1 * s23;
  J[2][0] = -dz2 * s1 * c23 + dy * c1 - dz1 * c2 * s1; J[2][1] = -dz2 * c1 * s23 - dz1 * c1 * s2; J[2][2] = -dz2 * c1 * s23;
}

MPC_HD void leg_fk(const double *q, double side, const Params &P, double *p) {
  double J[3][3];
  leg_fk_jac(q, side, P, p, J);
}

MPC_HD double ground(double gx, double gy, const double *p) { return gx * p[0] + gy * p[1]; }

// one plane per robot, z = gx x + gy y
struct Plane {
  static constexpr bool kUniformNormal = true;      // toy_step takes the normal once per tick
  double gx, gy;
  MPC_HD double height(const double *p) const { return ground(gx, gy, p); }
  MPC_HD void normal(const double *, double *n) const {
    n[0] = -gx; n[1] = -gy; n[2] = 1.0;
    const double nn = norm3(n);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = n[i] / nn;
  }
};

// the cell index and the fraction inside it of coordinate x (+ the robot's origin o) along one axis of a height field with `count` nodes, the
// first at x0, hscale apart.  The clamp is in floating point BEFORE the integer conversion: NaN and -inf land on 0, +inf and 1e300 on the last
// node, so 0 <= i <= count - 2 and 0 <= f <= 1 for every input and no lookup leaves the field; outside it the border's heights continue.
MPC_HD void terrain_index(double x, double o, double x0, double hscale, int count, int &i, double &f) {
  double u = ((x + o) - x0) / hscale;
  if (!(u > 0)) u = 0;
  if (u > count - 1) u = count - 1;
  i = (int)u;
  if (i > count - 2) i = count - 2;
  f = u - i;
}

// H[rows][cols] int16 (row index along x), hscale m per cell, vscale m per unit, node (0, 0) at (x0, y0); the robot's own coordinates are local
// and the field is sampled at local + (ox, oy).  A cell is split along the diagonal (i, j) - (i + 1, j + 1), as Isaac Gym's
// convert_heightfield_to_trimesh does (its slope_threshold correction is not modelled).  rows, cols >= 2.
struct HeightField {
  static constexpr bool kUniformNormal = false;     // the normal of the triangle under each anchor, in the substep that uses it
  const short *h;
  int rows, cols;
  double hscale, vscale, x0, y0, ox, oy;
  // height z and gradient (gx, gy) at p
  MPC_HD void surface(const double *p, double &z, double &gx, double &gy) const {
    int i, j;
    double fu, fv;
    terrain_index(p[0], ox, x0, hscale, rows, i, fu);
    terrain_index(p[1], oy, y0, hscale, cols, j, fv);
    const short *c = h + (long)i * cols + j;
    const double z00 = vscale * c[0], z10 = vscale * c[cols], z01 = vscale * c[1], z11 = vscale * c[cols + 1];
    if (fu >= fv) {
      z = z00 + fu * (z10 - z00) + fv * (z11 - z10);
      gx = (z10 - z00) / hscale; gy = (z11 - z10) / hscale;
    } else {
      z = z00 + fv * (z01 - z00) + fu * (z11 - z01);
      gx = (z11 - z01) / hscale; gy = (z01 - z00) / hscale;
    }
  }
  MPC_HD double height(const double *p) const {
    double z, gx, gy;
    surface(p, z, gx, gy);
    return z;
  }
  MPC_HD void normal(const double *p, double *n) const {
    double z, gx, gy;
    surface(p, z, gx, gy);
    n[0] = -gx; n[1] = -gy; n[2] = 1.0;
    const double nn = norm3(n);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = n[i] / nn;
  }
};

// ToyRobot._ik: q <- q + solve(J + 1e-9 I, target - p), `iters` times
MPC_HD void leg_ik(int l, const Params &P, const double *target, double *q, int iters) {
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    double p[3], J[3][3];
    leg_fk_jac(q, side_of(l), P, p, J);
#pragma unroll
    for (int i = 0; i < 3; ++i) J[i][i] = J[i][i] + kReg;
    double d[3] = {target[0] - p[0], target[1] - p[1], target[2] - p[2]};
    solve3(J, d);
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = q[i] + d[i];
  }
}

// ToyRobot.__init__(row, yaw0, slope) on ground g
template <class Ground>
MPC_HD void toy_init(State &s, const Params &P, double yaw0, const Ground &g) {
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    s.q[l][0] = 0.0; s.q[l][1] = 0.8; s.q[l][2] = -1.6;
    s.qd[l][0] = s.qd[l][1] = s.qd[l][2] = 0.0;
  }
  double sy, cy;
  sin_cos(yaw0 / 2, sy, cy);
  s.quat[0] = 0.0; s.quat[1] = 0.0; s.quat[2] = sy; s.quat[3] = cy;
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.v[i] = 0.0; s.w[i] = 0.0; s.pos[i] = 0.0; }
  double R[3][3];
  quat_to_rot(s.quat, R);
  double feet[4][3];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    double p[3], hp[3];
    leg_fk(s.q[l], side_of(l), P, p);
#pragma unroll
    for (int i = 0; i < 3; ++i) hp[i] = P.hiploc[l][i] + p[i];
    mat_vec(R, hp, feet[l]);
  }
  // Python's max() over a generator: the first of the largest
  double z = g.height(feet[0]) - feet[0][2];
#pragma unroll
  for (int l = 1; l < 4; ++l) {
    const double c = g.height(feet[l]) - feet[l][2];
    z = c > z ? c : z;
  }
  s.pos[2] = z;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    double a[3], d[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = s.pos[i] + feet[l][i];
    a[2] = g.height(a);
#pragma unroll
    for (int i = 0; i < 3; ++i) { s.anchor[l][i] = a[i]; d[i] = a[i] - s.pos[i]; }
    mat_t_vec(R, d, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = t[i] - P.hiploc[l][i];
    leg_ik(l, P, t, s.q[l], 20);
    s.contact[l] = 1;
    s.lift[l] = 0;
  }
  s.fell = 0;
}

MPC_HD void toy_init(State &s, const Params &P, double yaw0, double gx, double gy) { toy_init(s, P, yaw0, Plane{gx, gy}); }

// the contact policies of the step (see the head of this file)
struct NoFriction {
  static constexpr bool kFriction = false;
};

struct Coulomb {
  static constexpr bool kFriction = true;
  double mu;
  double force[4][3];                  // out: the ground reaction of the tick's last substep, world frame [N]
  double slip[4];                      // out: the distance slid over the tick [m]
};

// ToyRobot.step(tau, dt) on ground g under gravity (0, 0, grav_z) with contact policy c: one tick of kSubsteps substeps
template <class Ground, class Contact>
MPC_HD void toy_step_contact(State &s, const Params &P, const double *tau, double dt, const Ground &g, double grav_z, Contact &c) {
  const double h = dt / kSubsteps;
  double n[3];
  if constexpr (Ground::kUniformNormal) g.normal(s.pos, n);
  if constexpr (Contact::kFriction) {
#pragma unroll
    for (int l = 0; l < 4; ++l) c.slip[l] = 0.0;
  }
#pragma unroll 1
  for (int sub = 0; sub < kSubsteps; ++sub) {
    if constexpr (Contact::kFriction) {
#pragma unroll
      for (int l = 0; l < 4; ++l) c.force[l][0] = c.force[l][1] = c.force[l][2] = 0.0;
    }
    double R[3][3];
    quat_to_rot(s.quat, R);
    double F[3] = {0.0, 0.0, 0.0}, T[3] = {0.0, 0.0, 0.0};
    double pj[4][3];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      double J[3][3];
      leg_fk_jac(s.q[l], side_of(l), P, pj[l], J);
      if (!s.contact[l]) continue;
      double Jt[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Jt[i][j] = J[j][i];
#pragma unroll
      for (int i = 0; i < 3; ++i) Jt[i][i] = Jt[i][i] + kReg;
      double x[3] = {tau[3 * l], tau[3 * l + 1], tau[3 * l + 2]};
      solve3(Jt, x);
      double f[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) f[i] = (-R[i][0]) * x[0] + (-R[i][1]) * x[1] + (-R[i][2]) * x[2];
      if constexpr (!Ground::kUniformNormal) g.normal(s.anchor[l], n);
      const double fn = dot3(f, n);
      if (fn < -kReleaseN) {             // the leg pulls on the ground (a swing command): it lets go
        s.contact[l] = 0;
        s.lift[l] = kLiftTicks * kSubsteps;
        continue;
      }
      if (fn < 0.0) continue;            // (unilateral contact: no pull, but not yet a lift-off either)
      if constexpr (Contact::kFriction) {
        double ft[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) ft[i] = f[i] - fn * n[i];
        const double ftn = norm3(ft), lim = c.mu * fn;
        if (ftn > lim) {                 // beyond the cone: the ground supplies the limit and the foot slides (NaN, mu = inf and fn = 0: it sticks)
          double t[3], a[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) t[i] = ft[i] / ftn;
#pragma unroll
          for (int i = 0; i < 3; ++i) f[i] = fn * n[i] + lim * t[i];
          const double d = h * ((ftn - lim) / kSlipDamp);
#pragma unroll
          for (int i = 0; i < 3; ++i) a[i] = s.anchor[l][i] - d * t[i];
          a[2] = g.height(a);
#pragma unroll
          for (int i = 0; i < 3; ++i) s.anchor[l][i] = a[i];
          c.slip[l] = c.slip[l] + d;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) c.force[l][i] = f[i];
      }
      double hp[3], r[3], cr[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { F[i] = F[i] + f[i]; hp[i] = P.hiploc[l][i] + pj[l][i]; }
      mat_vec(R, hp, r);
      cross(r, f, cr);
#pragma unroll
      for (int i = 0; i < 3; ++i) T[i] = T[i] + cr[i];
    }
    // Iw = (R diag(I)) R^T
    double RD[3][3], Iw[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) RD[i][j] = R[i][j] * P.inertia[j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Iw[i][j] = RD[i][0] * R[j][0] + RD[i][1] * R[j][1] + RD[i][2] * R[j][2];
    s.v[0] = s.v[0] + h * (0.0 + F[0] / P.mass);
    s.v[1] = s.v[1] + h * (0.0 + F[1] / P.mass);
    s.v[2] = s.v[2] + h * (grav_z + F[2] / P.mass);
    double Iww[3], gyro[3], rhs[3];
    mat_vec(Iw, s.w, Iww);
    cross(s.w, Iww, gyro);
#pragma unroll
    for (int i = 0; i < 3; ++i) rhs[i] = T[i] - gyro[i];
    solve3(Iw, rhs);
#pragma unroll
    for (int i = 0; i < 3; ++i) s.w[i] = s.w[i] + h * rhs[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) s.pos[i] = s.pos[i] + h * s.v[i];
    const double wn = norm3(s.w);
    const double ang = wn * h;
    const double wd = wn > 1e-12 ? wn : 1e-12;
    double sa, ca;
    sin_cos(ang / 2, sa, ca);
    const double dq[4] = {s.w[0] / wd * sa, s.w[1] / wd * sa, s.w[2] / wd * sa, ca};
    const double ax = s.quat[0], ay = s.quat[1], az = s.quat[2], aw = s.quat[3];
    const double bx = dq[0], by = dq[1], bz = dq[2], bw = dq[3];
    // quat_mul(dq, quat)
    double qn[4] = {bw * ax + bx * aw + by * az - bz * ay, bw * ay - bx * az + by * aw + bz * ax,
                    bw * az + bx * ay - by * ax + bz * aw, bw * aw - bx * ax - by * ay - bz * az};
    const double qnorm = sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) s.quat[i] = qn[i] / qnorm;
    double R2[3][3];
    quat_to_rot(s.quat, R2);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      if (s.contact[l]) {
        double d[3], t[3], qk[3] = {s.q[l][0], s.q[l][1], s.q[l][2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = s.anchor[l][i] - s.pos[i];
        mat_t_vec(R2, d, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = t[i] - P.hiploc[l][i];
        leg_ik(l, P, t, qk, 4);
#pragma unroll
        for (int i = 0; i < 3; ++i) { s.qd[l][i] = (qk[i] - s.q[l][i]) / h; s.q[l][i] = qk[i]; }
        continue;
      }
      double hp[3], p_old[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) hp[i] = P.hiploc[l][i] + pj[l][i];
      mat_vec(R, hp, p_old);
#pragma unroll
      for (int i = 0; i < 3; ++i) p_old[i] = p_old[i] + (s.pos[i] - h * s.v[i]);      // (world foot position before the substep)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        s.qd[l][i] = s.qd[l][i] + h * (tau[3 * l + i] - kBJ * s.qd[l][i]) / kIJ;
        s.q[l][i] = s.q[l][i] + h * s.qd[l][i];
      }
      if (s.lift[l] > 0) {
        s.lift[l] -= 1;
        continue;
      }
      double pf[3], hp2[3], rp[3], p_new[3];
      leg_fk(s.q[l], side_of(l), P, pf);
#pragma unroll
      for (int i = 0; i < 3; ++i) hp2[i] = P.hiploc[l][i] + pf[i];
      mat_vec(R2, hp2, rp);
#pragma unroll
      for (int i = 0; i < 3; ++i) p_new[i] = s.pos[i] + rp[i];
      const double d_old = p_old[2] - g.height(p_old), d_new = p_new[2] - g.height(p_new);
      if (d_new <= 0.0) {                // touch-down: the anchor is where the foot path crosses the ground
        const double sc = d_old <= 0.0 ? 1.0 : d_old / (d_old - d_new);
        double a[3], d[3], t[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) a[i] = p_old[i] + sc * (p_new[i] - p_old[i]);
        a[2] = g.height(a);
#pragma unroll
        for (int i = 0; i < 3; ++i) { s.anchor[l][i] = a[i]; d[i] = a[i] - s.pos[i]; }
        s.contact[l] = 1;
        mat_t_vec(R2, d, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = t[i] - P.hiploc[l][i];
        leg_ik(l, P, t, s.q[l], 4);
#pragma unroll
        for (int i = 0; i < 3; ++i) s.qd[l][i] = 0.0;
      }
    }
  }
  double R[3][3];
  quat_to_rot(s.quat, R);
  const bool finite = isfinite(s.pos[0]) && isfinite(s.pos[1]) && isfinite(s.pos[2]);
  if (!finite || R[2][2] < 0.3 || fabs(s.pos[2] - g.height(s.pos)) > 3 * P.height) s.fell = 1;
}

// ... with the anchor that holds (no friction cone): what every plant stepped with before Coulomb, and every toy_step* below still does
template <class Ground>
MPC_HD void toy_step_gravity(State &s, const Params &P, const double *tau, double dt, const Ground &g, double grav_z) {
  NoFriction c;
  toy_step_contact(s, P, tau, dt, g, grav_z, c);
}

// ... under the constant kGravZ: the plant every robot of a type shares
template <class Ground>
MPC_HD void toy_step(State &s, const Params &P, const double *tau, double dt, const Ground &g) { toy_step_gravity(s, P, tau, dt, g, kGravZ); }

MPC_HD void toy_step(State &s, const Params &P, const double *tau, double dt, double gx, double gy) { toy_step(s, P, tau, dt, Plane{gx, gy}); }

// ... with the robot's own plant record: mass + payload, tau * strength, its own gravity (see the head of this file)
template <class Ground>
MPC_HD void toy_step_plant(State &s, const Params &P, const double *tau, double dt, const Ground &g, double payload, double strength, double grav_z) {
  Params Q = P;
  Q.mass = P.mass + payload;
  double t[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) t[i] = tau[i] * strength;
  toy_step_gravity(s, Q, t, dt, g, grav_z);
}

// ... with the robot's own plant record and the Coulomb contact c (c.mu in; c.force, c.slip out).  The neutral record and mu = +inf: toy_step.
template <class Ground>
MPC_HD void toy_step_friction(State &s, const Params &P, const double *tau, double dt, const Ground &g, double payload, double strength, double grav_z, Coulomb &c) {
  Params Q = P;
  Q.mass = P.mass + payload;
  double t[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) t[i] = tau[i] * strength;
  toy_step_contact(s, Q, t, dt, g, grav_z, c);
}

// the state record of include/mpc_sim.h: f64[kF64], i32[kI32]; `stride` = distance between two consecutive entries of ONE robot
// (1 on the host; the batch size on the device, whose state is structure-of-arrays)
MPC_HD void pack(const State &s, double *f, int *k, long stride) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { f[(kOffPos + i) * stride] = s.pos[i]; f[(kOffV + i) * stride] = s.v[i]; f[(kOffW + i) * stride] = s.w[i]; }
#pragma unroll
  for (int i = 0; i < 4; ++i) f[(kOffQuat + i) * stride] = s.quat[i];
#pragma unroll
  for (int l = 0; l < 4; ++l)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      f[(kOffQ + 3 * l + i) * stride] = s.q[l][i];
      f[(kOffQd + 3 * l + i) * stride] = s.qd[l][i];
      f[(kOffAnchor + 3 * l + i) * stride] = s.anchor[l][i];
    }
#pragma unroll
  for (int l = 0; l < 4; ++l) { k[l * stride] = s.contact[l]; k[(4 + l) * stride] = s.lift[l]; }
  k[8 * stride] = s.fell;
}

MPC_HD void unpack(State &s, const double *f, const int *k, long stride) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.pos[i] = f[(kOffPos + i) * stride]; s.v[i] = f[(kOffV + i) * stride]; s.w[i] = f[(kOffW + i) * stride]; }
#pragma unroll
  for (int i = 0; i < 4; ++i) s.quat[i] = f[(kOffQuat + i) * stride];
#pragma unroll
  for (int l = 0; l < 4; ++l)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      s.q[l][i] = f[(kOffQ + 3 * l + i) * stride];
      s.qd[l][i] = f[(kOffQd + 3 * l + i) * stride];
      s.anchor[l][i] = f[(kOffAnchor + 3 * l + i) * stride];
    }
#pragma unroll
  for (int l = 0; l < 4; ++l) { s.contact[l] = k[l * stride]; s.lift[l] = k[(4 + l) * stride]; }
  s.fell = k[8 * stride];
}

// ToyRobot.observe: dof_state [12][2] (pos, vel) and root_state [13] (pos3, quat xyzw, lin vel3, ang vel3), float32
MPC_HD void observe(const State &s, float *dof, float *root) {
#pragma unroll
  for (int l = 0; l < 4; ++l)
#pragma unroll
    for (int i = 0; i < 3; ++i) { dof[2 * (3 * l + i)] = (float)s.q[l][i]; dof[2 * (3 * l + i) + 1] = (float)s.qd[l][i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { root[i] = (float)s.pos[i]; root[7 + i] = (float)s.v[i]; root[10 + i] = (float)s.w[i]; }
#pragma unroll
  for (int i = 0; i < 4; ++i) root[3 + i] = (float)s.quat[i];
}

}  // namespace toysim
