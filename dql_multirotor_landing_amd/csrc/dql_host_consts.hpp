// dql_host_consts.hpp — host-side builders of the step kernel's launch constants (dql_config -> SimK / MdpK, the Kalman fixed point, the literal-table
// checks, the eps threshold, the per-period tick schedule).  Shared by the library (dql_hip.hip) and the host emulation of the step kernel
// (tests/host_emu/step_emu.cpp), so that both hand agent_period the same constants.  Host code only; include after dql_device.hpp.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>

#include "dql_device.hpp"

#define DQL_MAX_PERIODS 32  // agent periods one launch may run back to back per env (option "periods_per_launch"; round 5: 32, the schedule arrays' size)

namespace dql {

// ---------------------------------------------------------------------------------------------
// host -> device constants
// ---------------------------------------------------------------------------------------------
template <typename T> static MdpK<T> make_mdpk(const dql_config& c) {
  MdpK<T> d;
  memset(&d, 0, sizeof(d));
  d.p_max = (T)c.p_max; d.v_max = (T)c.v_max; d.a_max = (T)c.a_max; d.theta_max = (T)c.theta_max; d.delta_theta = (T)c.delta_theta;
  d.beta = (T)c.beta; d.sigma_a = (T)c.sigma_a; d.min_alt = (T)c.minimum_altitude;
  d.w_p = (T)c.w_p; d.w_v = (T)c.w_v; d.w_theta = (T)c.w_theta; d.w_dur = (T)c.w_dur; d.w_fail = (T)c.w_fail; d.w_succ = (T)c.w_succ;
  d.delta_t = (T)(1.0 / c.f_ag); d.f_ag = (T)c.f_ag; d.timeout_steps = (T)(c.t_max * c.f_ag);
  for (int i = 0; i < 5; ++i) { d.lim_p[i] = (T)c.lim_p[i]; d.lim_v[i] = (T)c.lim_v[i]; d.lim_a[i] = (T)c.lim_a[i]; }
  const double step = (c.theta_max - (-c.theta_max)) / 6.0;  // np.linspace(-theta_max, theta_max, 7), pkg/mdp.py:145
  for (int i = 0; i < 6; ++i) d.angles[i] = (T)((double)i * step + (-c.theta_max));
  d.angles[6] = (T)c.theta_max;
  d.inv_p_max = (T)(1.0 / c.p_max); d.inv_v_max = (T)(1.0 / c.v_max); d.inv_a_max = (T)(1.0 / c.a_max);
  d.inv_theta_max = (T)(1.0 / c.theta_max); d.dtheta_ratio = (T)(c.delta_theta / c.theta_max);
  for (int j = 0; j < 3; ++j) { const double t = std::tan(((double)j + 0.5) * step); d.tan2_mid[j] = (T)(t * t); }  // bin boundaries of the angle grid (angle_bin_from_tangent)
  d.gamma = c.gamma; d.working = c.working_curriculum_step; d.goal_logic = c.goal_logic; d.quirks = c.quirks;
  return d;
}
// is this SimK the table k_step<float, ., TICK_LIT> was compiled with?  (bit for bit; -0.0 != +0.0 on purpose)
static bool refk_matches(const SimK<float>& s) {
  bool ok = true;
#define DQL_X(n, v) { const float r = v; ok = ok && memcmp(&s.n, &r, sizeof(float)) == 0; }
  DQL_REFK_SCALARS(DQL_X)
#undef DQL_X
#define DQL_A(n, a, b, c) { const float r[3] = {a, b, c}; ok = ok && memcmp(s.n, r, sizeof(r)) == 0; }
  DQL_REFK_VECTORS(DQL_A)
#undef DQL_A
  return ok;
}
// ... and is this MdpK the table LitM was compiled with?  (the run-time members — working, goal_logic, quirks, timeout_steps, gamma — are not part of it)
static bool refm_matches(const MdpK<float>& m) {
  bool ok = true;
#define DQL_X(n, v) { const float r = v; ok = ok && memcmp(&m.n, &r, sizeof(float)) == 0; }
  DQL_REFM_SCALARS(DQL_X)
#undef DQL_X
  for (int k = 0; k < 4; ++k) {  // the quotient tables are what discretise() would divide at run time
    volatile float qp = m.lim_p[k + 1] / m.lim_p[k], qv = m.lim_v[k + 1] / m.lim_v[k];
    const float rp = LitM::ratio_p[k], rv = LitM::ratio_v[k];
    ok = ok && memcmp((const void*)&qp, &rp, sizeof(float)) == 0 && memcmp((const void*)&qv, &rv, sizeof(float)) == 0;
  }
#define DQL_L(n, a, b, c, d, e) { const float r[5] = {a, b, c, d, e}; ok = ok && memcmp(m.n, r, sizeof(r)) == 0; }
  DQL_REFM_LIMITS(DQL_L)
#undef DQL_L
#define DQL_G(n, a, b, c, d, e, f, g) { const float r[7] = {a, b, c, d, e, f, g}; ok = ok && memcmp(m.n, r, sizeof(r)) == 0; }
  DQL_REFM_GRID(DQL_G)
#undef DQL_G
#define DQL_T(n, a, b, c) { const float r[3] = {a, b, c}; ok = ok && memcmp(m.n, r, sizeof(r)) == 0; }
  DQL_REFM_TAN2(DQL_T)
#undef DQL_T
  return ok;
}
// P's fixed point under kalman1d's update in T arithmetic (P += Q; K = P / (P + R); P *= 1 - K), reached from the creation value P = 1; pss = NaN when
// the iteration does not settle on one value (then the kernel's shortcut never fires).  R = 0: kalman1d's own shortcut applies, no fixed point needed.
// A context computes it ONCE (dql_create; the noise constants of a context never change) and hands it to make_simk with every launch: a (Q, R) that
// settles on a 2-cycle costs its 200 000 iterations once, not per launch, and contexts with different noise settings do not evict each other.
template <typename T> static void kalman_fixed_point(T Q, T R, T& pss, T& kss) {
  pss = std::numeric_limits<T>::quiet_NaN(); kss = T(0);
  if (!(R > T(0)) || !(Q >= T(0))) return;
  volatile T P = T(1);
  for (int i = 0; i < 200000; ++i) {
    volatile T P1 = P + Q;
    volatile T den = P1 + R;
    volatile T K = P1 / den;
    volatile T om = T(1) - K;
    volatile T P2 = P1 * om;
    if (P2 == P) { pss = P; kss = K; return; }
    P = P2;
  }
}
struct KalFix { double pss, kss; bool valid; };  // the fixed point in the context's dtype, widened (exact)
template <typename T> static SimK<T> make_simk(const dql_config& c, const KalFix* kf = nullptr) {
  SimK<T> d;
  memset(&d, 0, sizeof(d));
  d.dt = (T)c.dt; d.g = (T)c.gravity; d.inv_m = (T)(1.0 / c.mass);
  d.dtm = (T)(c.dt / c.mass); d.dtg = (T)(c.dt * c.gravity);
  for (int i = 0; i < 3; ++i) d.dtI[i] = (T)(c.dt / c.inertia[i]);
  d.nlcd = (T)(-(c.arm_length * c.c_drag)); d.hdt = (T)(0.5 * c.dt); d.low_z = (T)(c.mp_top_z + c.drone_bottom);
  d.oup = (T)(1.0 - c.rotor_alpha_up); d.odn = (T)(1.0 - c.rotor_alpha_down); d.inv_mgr_dt = (T)(1.0 / (c.dt * c.manager_div));
  for (int i = 0; i < 3; ++i) { d.I[i] = (T)c.inertia[i]; d.inv_I[i] = (T)(1.0 / c.inertia[i]); d.kR[i] = (T)c.k_R[i]; d.kW[i] = (T)c.k_W[i]; }
  d.l = (T)c.arm_length; d.h = (T)c.rotor_z; d.kf = (T)c.k_f; d.km = (T)c.k_m; d.lkf = (T)(c.arm_length * c.k_f); d.kmkf = (T)(c.k_m * c.k_f);
  d.aup = (T)c.rotor_alpha_up; d.adn = (T)c.rotor_alpha_down; d.omax = (T)c.rotor_max; d.cd = (T)c.c_drag; d.crd = (T)(c.c_roll / c.c_drag);
  d.ia = (T)(1.0 / (4.0 * c.k_f)); d.ib = (T)(1.0 / (2.0 * c.arm_length * c.k_f)); d.ic = (T)(1.0 / (4.0 * c.k_f * c.k_m));
  d.vz_kp = (T)c.pid_vz[0]; d.vz_ki = (T)c.pid_vz[1]; d.vz_lo = (T)c.pid_vz[3]; d.vz_hi = (T)c.pid_vz[4]; d.vz_wind = (T)c.pid_vz[5]; d.vz_sp = (T)c.vz_setpoint;
  d.yw_kp = (T)c.pid_yaw[0]; d.yw_ki = (T)c.pid_yaw[1]; d.yw_lo = (T)c.pid_yaw[3]; d.yw_hi = (T)c.pid_yaw[4]; d.yw_wind = (T)c.pid_yaw[5]; d.yw_sp = (T)c.yaw_setpoint;
  const double bc = c.bw_c, denom = 1 + bc * bc + 1.414 * bc;  // pkg/filters.py:94-106
  d.bw_inv = (T)(1.0 / denom); d.bw_k1 = (T)(bc * bc - 1.414 * bc + 1); d.bw_k2 = (T)(-2 * bc * bc + 2);
  d.bw_b2 = (T)(2.0 / denom); d.bw_a2 = (T)((-2 * bc * bc + 2) / denom); d.bw_a3 = (T)((bc * bc - 1.414 * bc + 1) / denom);
  d.mp_dt = (T)c.mp_dt; d.mp_top = (T)c.mp_top_z; d.mp_hx = (T)c.mp_half_x; d.mp_hy = (T)c.mp_half_y; d.bottom = (T)c.drone_bottom;
  d.noise_p = (T)c.noise_pos_sd; d.noise_v = (T)c.noise_vel_sd; d.kal_q = (T)c.kalman_q; d.kal_r = (T)(c.noise_vel_sd * c.noise_vel_sd);
  d.mgr_dt = (T)(c.dt * c.manager_div);
  if (kf && kf->valid) { d.kal_pss = (T)kf->pss; d.kal_kss = (T)kf->kss; }
  else kalman_fixed_point<T>(d.kal_q, d.kal_r, d.kal_pss, d.kal_kss);
  d.mp_r = (T)c.mp_r_x; d.mp_w = (T)(c.mp_t_x / c.mp_r_x);
  if (c.trajectory == DQL_TRAJ_EIGHT) { d.mp_r = (T)3.0; d.mp_w = (T)(0.8 / 3.0); }
  d.p_max = (T)c.p_max; d.theta_max = (T)c.theta_max; d.delta_theta = (T)c.delta_theta; d.z_init = (T)c.z_init; d.init_sigma = (T)c.init_sigma;
  d.div = c.manager_div; d.traj = c.trajectory; d.init_uniform = c.init_uniform; d.working = c.working_curriculum_step;
  d.per_env_platform = c.per_env_platform; d.two_axis = c.two_axis; d.quirks = c.quirks;
  d.noisy = (d.noise_p > T(0) || d.noise_v > T(0)) ? 1 : 0; d.kal_r_zero = (d.kal_r == T(0)) ? 1 : 0;
  return d;
}

// number of k in [0, 2^24) with k 2^-24 < eps (the values u24() takes): eps 2^24 is exact in double, so this is the SAME predicate as the
// reference-shaped `uniform < eps` (pkg/double_q_learning.py:113), evaluated among integers
static unsigned int eps_threshold(double eps) {
  if (!(eps > 0.0)) return 0u;
  const double t = std::ceil(eps * 16777216.0);
  return t >= 16777216.0 ? 16777216u : (unsigned int)t;
}
static long long ticks_before(const dql_config& c, long long j) { return (long long)std::floor((double)j * (1.0 / (c.f_ag * c.dt))); }

// the per-period tick schedule of `count` agent periods from period j on (a step launch's kernel arguments hold DQL_MAX_PERIODS entries; a roll-out
// uploads one per period of the episode)
static void fill_schedule(const dql_config& c, long long j, long long* mgr0, int* sched, int count = DQL_MAX_PERIODS) {
  for (int p = 0; p < count; ++p) {
    const long long g0 = ticks_before(c, j + p);
    const int n_ticks = (int)(ticks_before(c, j + p + 1) - g0), div = c.manager_div;
    const int phase = (int)(g0 % div);                                   // physics ticks since the last 100 Hz manager tick
    mgr0[p] = g0 / div + (phase ? 1 : 0);                                // index of the next manager tick
    const int first_mgr = phase ? div - phase : 0;
    const int last_mgr = first_mgr < n_ticks ? (n_ticks - 1 - first_mgr) / div : 0;
    sched[p] = n_ticks | (phase << 8) | (last_mgr << 16);                // check_config: n_ticks, manager_div <= 255
  }
}

}  // namespace dql
