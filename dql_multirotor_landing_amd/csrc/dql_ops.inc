// dql_ops.inc: the stateless drop-in operators (include/dql.h dql_discretise .. dql_place; include/dql_diag.h dql_diag_selftest_sqrt[_ieee], dql_diag_det_math_run,
// dql_diag_box_muller_run, dql_diag_philox_run): their kernels and their C calls.
// A fragment of dql_hip.hip's translation unit, not a header.  Needs from it: fail / HIP_TRY, by_dtype, DevBuf / OP_PROLOGUE / UP / OUT / DOWN, check_config; and
// dql_device.hpp, dql_host_consts.hpp.  Every call: argument checks (before the device is touched), uploads, one launch, downloads.
template <typename T> __global__ void k_discretise(MdpK<T> c, const double* p, const double* v, const double* acc, const double* ang, long long n, int* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = discretise(c, (T)p[i], (T)v[i], (T)acc[i], (T)ang[i]);
}
template <typename T>
__global__ void k_mdp_transition(MdpK<T> c, long long n, uint32_t stages, const uint8_t* action, const double* obs, double* ms, const int* prev_idx,
                                 int* idx_io, double* reward_out, uint8_t* done_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T sp = (T)ms[0 * n + i], shp_p = (T)ms[1 * n + i], shp_v = (T)ms[2 * n + i], shp_a = (T)ms[3 * n + i], cum = (T)ms[4 * n + i];
  int step_count = (int)ms[5 * n + i], cur_check = (int)ms[6 * n + i], code = (int)ms[7 * n + i];
  const T px = (T)obs[0 * n + i], py = (T)obs[1 * n + i], vx = (T)obs[2 * n + i], ax = (T)obs[3 * n + i], pitch = (T)obs[4 * n + i], z = (T)obs[5 * n + i];
  const bool contact = obs[6 * n + i] != 0.0;
  if (stages & DQL_MDP_ACTION) sp = continuous_action(c, sp, (int)action[i]);
  int idx = idx_io[i];
  if (stages & DQL_MDP_DISCRETISE) { idx = discretise(c, px, vx, ax, pitch); idx_io[i] = idx; }
  const int sidx = idx < 0 ? 0 : idx;
  if (stages & DQL_MDP_CHECK) {
    // SimulationMdp.check has no goal logic: feeding prev = -1 disables that branch (pkg/mdp.py:784-845)
    code = mdp_check(c, step_count, cur_check, code, (stages & DQL_MDP_SIMULATION) ? -1 : prev_idx[i], sidx, contact, px, py, z);
    done_out[i] = code <= DQL_TERMINAL_TIMEOUT;
  }
  if (stages & DQL_MDP_REWARD) reward_out[i] = (double)mdp_reward(c, shp_p, shp_v, shp_a, cum, code, sidx, px, vx, sp);
  ms[0 * n + i] = sp; ms[1 * n + i] = shp_p; ms[2 * n + i] = shp_v; ms[3 * n + i] = shp_a; ms[4 * n + i] = cum;
  ms[5 * n + i] = step_count; ms[6 * n + i] = cur_check; ms[7 * n + i] = code;
}
// the 100 Hz manager tick of the fused kernel (manager_states + manager_obs) replayed over scripted series, one lane per series
template <typename T>
__global__ void k_manager_run(SimK<T> c, long long n_series, long long n_ticks, const double* in, const uint8_t* contact, unsigned long long seed, double* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_series) return;
  Env<T> e;
  memset(&e, 0, sizeof(e));
  e.kal_x_P = T(1.0); e.kal_y_P = T(1.0); e.mp_r = c.mp_r; e.mp_w = c.mp_w;
  for (long long t = 0; t < n_ticks; ++t) {
    const double* r = in + (i * n_ticks + t) * 14;
    for (int k = 0; k < 3; ++k) { e.p[k] = (T)r[k]; e.v[k] = (T)r[3 + k]; }
    for (int k = 0; k < 4; ++k) e.q[k] = (T)r[6 + k];
    e.mp_x = (T)r[10]; e.mp_y = (T)r[11]; e.mp_u = (T)r[12]; e.mp_v = (T)r[13];
    if (contact[i * n_ticks + t]) e.flags |= FL_CONTACT;
    T R[9], cy, sy;
    quat_to_R(e.q, R); yaw_cs(R, cy, sy);
    manager_states(R, cy, sy, e.v[2], e.vz_state, e.yw_state);
    manager_obs(c, e, cy, sy, t, (uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0u, (uint32_t)i, (uint32_t)t);
    double* o = out + (i * n_ticks + t) * 12;
    o[0] = e.obs_px; o[1] = e.obs_py; o[2] = e.obs_vx; o[3] = e.obs_vy; o[4] = e.obs_ax; o[5] = e.obs_ay;
    o[6] = e.vz_state; o[7] = e.yw_state; o[8] = e.mp_x; o[9] = e.mp_y; o[10] = e.mp_u; o[11] = e.mp_v;
  }
}
// the plant of the fused kernel (plant_step + rotor_filter + platform_contact) replayed open loop, one lane per series (dql_plant_run)
template <typename T>
__global__ void k_plant_run(SimK<T> c, long long n_series, long long n_ticks, const double* init, const double* rotor_cmd, double* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_series) return;
  Env<T> e;
  memset(&e, 0, sizeof(e));
  const double* s0 = init + i * 21;
  for (int k = 0; k < 3; ++k) { e.p[k] = (T)s0[k]; e.v[k] = (T)s0[3 + k]; e.w[k] = (T)s0[10 + k]; }
  for (int k = 0; k < 4; ++k) { e.q[k] = (T)s0[6 + k]; e.om[k] = (T)s0[13 + k]; }
  e.mp_x = (T)s0[17]; e.mp_y = (T)s0[18]; e.mp_u = (T)s0[19]; e.mp_v = (T)s0[20];
  for (long long t = 0; t < n_ticks; ++t) {
    const double* r = rotor_cmd + (i * n_ticks + t) * 4;
    const T cmd[4] = {(T)r[0], (T)r[1], (T)r[2], (T)r[3]};
    T R[9];
    quat_to_R(e.q, R);
    plant_step(c, e, R);
    rotor_filter(c, e, cmd);
    platform_contact(c, e);
    double* o = out + (i * n_ticks + t) * 20;
    for (int k = 0; k < 3; ++k) { o[k] = e.p[k]; o[3 + k] = e.v[k]; o[10 + k] = e.w[k]; }
    for (int k = 0; k < 4; ++k) { o[6 + k] = e.q[k]; o[13 + k] = e.om[k]; }
    o[17] = e.mp_x; o[18] = e.mp_y; o[19] = (e.flags & FL_CONTACT) ? 1.0 : 0.0;
  }
}
// ---- the control-side functions of the tick replayed alone (dql_butterworth_run, dql_kalman_run, dql_pid_run, dql_attitude_run,
// dql_platform_run): the SAME device functions the fused step calls, one lane, so that each can be held against the reference's own
// outputs (golden vectors G8, G9, G11) in float64 AND in the float32 forms every throughput figure runs on ----
template <typename T> struct FiltK { T dt, bw_k1, bw_k2, bw_inv, bw_b2, bw_a2, bw_a3; };
template <typename T> static FiltK<T> make_filtk(double bc) {  // pkg/filters.py:94-106, as make_simk has it
  const double denom = 1 + bc * bc + 1.414 * bc;
  FiltK<T> d;
  d.dt = T(0); d.bw_inv = (T)(1.0 / denom); d.bw_k1 = (T)(bc * bc - 1.414 * bc + 1); d.bw_k2 = (T)(-2 * bc * bc + 2);
  d.bw_b2 = (T)(2.0 / denom); d.bw_a2 = (T)((-2 * bc * bc + 2) / denom); d.bw_a3 = (T)((bc * bc - 1.414 * bc + 1) / denom);
  return d;
}
template <typename T> __global__ void k_butterworth_run(FiltK<T> c, const double* x, long long n, double* y) {  // pkg/filters.py:98-109 from zero histories
  if (blockIdx.x || threadIdx.x) return;
  T x1 = T(0), x2 = T(0), y1 = T(0), y2 = T(0), y3 = T(0);
  for (long long i = 0; i < n; ++i) y[i] = (double)butterworth(c, (T)x[i], x1, x2, y1, y2, y3);
}
// KalmanFilter3D.filter over a velocity series (pkg/filters.py:53-80): z = dv / dt with the timestamps 0.01 i, dt <= 0 -> 0.01 (dt_le0[i] forces that branch)
template <typename T> __global__ void k_kalman_run(T Q, T Rm, const double* vel, const uint8_t* dt_le0, long long n, double* acc) {
  if (blockIdx.x || threadIdx.x) return;
  T x[3] = {T(0), T(0), T(0)}, P[3] = {T(1), T(1), T(1)};
  for (long long i = 1; i < n; ++i) {
    T dt_ = dt_le0[i] ? T(0.0) : (T)(0.01 * (double)i) - (T)(0.01 * (double)(i - 1));
    if (dt_ <= T(0.0)) dt_ = T(0.01);
    for (int k = 0; k < 3; ++k) acc[(i - 1) * 3 + k] = (double)kalman1d(x[k], P[k], Q, Rm, ((T)vel[i * 3 + k] - (T)vel[(i - 1) * 3 + k]) / dt_);
  }
}
// PID.output replay (pkg/pid.py:62-104, Kd = 0): the plant state is sampled every 5th tick, tick times are 0.002 (i + 1)
template <typename T> struct PidP { T kp, ki, lo, hi, wind, sp; };
template <typename T> __global__ void k_pid_run(FiltK<T> c, PidP<T> p, const double* state, long long n, double* effort, double* integral) {
  if (blockIdx.x || threadIdx.x) return;
  T integ = T(0), x1 = T(0), x2 = T(0), y1 = T(0), y2 = T(0), y3 = T(0), st = T(0), prev_t = T(0);
  for (long long i = 0; i < n; ++i) {
    const T t = (T)(0.002 * (double)(i + 1));
    if (i % 5 == 0) st = (T)state[i];
    c.dt = t - prev_t;
    effort[i] = (double)pid_output(c, p.kp, p.ki, p.lo, p.hi, p.wind, p.sp, st, integ, x1, x2, y1, y2, y3);
    integral[i] = (double)integ;
    prev_t = t;
  }
}
// AttitudeController.compute_rotor_velocities (pkg/attitude_controller.py:107-156) for n samples: quaternion (x, y, z, w) as ROS has it, body rates,
// cmd = roll, pitch, yaw rate, thrust -> commanded rotor speeds.  xonly: the x-axis closed form the x-axis kernels compile in (roll command exactly 0)
template <typename T> __global__ void k_attitude_run(SimK<T> s, const double* quat_xyzw, const double* omega, const double* cmd, long long n, int xonly, double* rotor) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T q[4] = {(T)quat_xyzw[i * 4 + 3], (T)quat_xyzw[i * 4 + 0], (T)quat_xyzw[i * 4 + 1], (T)quat_xyzw[i * 4 + 2]};
  const T w[3] = {(T)omega[i * 3], (T)omega[i * 3 + 1], (T)omega[i * 3 + 2]};
  T R[9], cy, sy, ct, rn, B[9], out[4];
  quat_to_R(q, R); yaw_cs(R, cy, sy, ct, rn);
  make_B((T)cmd[i * 4 + 1], (T)cmd[i * 4 + 0], B);
  attitude(s, R, w, B, cy, sy, ct, rn, (T)cmd[i * 4 + 2], (T)cmd[i * 4 + 3], out, xonly != 0);
  for (int k = 0; k < 4; ++k) rotor[i * 4 + k] = (double)out[k];
}
// MovingPlatform.compute_trajectory (pkg/moving_platform.py:87-127) from phase 0: x, y, u, v at successive 100 Hz ticks.  carry > 0: sine and cosine
// are evaluated at every carry-th tick only and rotated through the constant phase step in between — what the fused float32 step does inside an
// agent period (platform_update with a PlatRec; four or five manager ticks per period)
template <typename T> __global__ void k_platform_run(SimK<T> s, long long n, int carry, double* out) {
  if (blockIdx.x || threadIdx.x) return;
  Env<T> e;
  memset(&e, 0, sizeof(e));
  e.mp_r = s.mp_r; e.mp_w = s.mp_w;
  PlatRec<T> rec = PlatRec<T>{};
  for (long long i = 0; i < n; ++i) {
    if (carry > 0) platform_update(s, e, &rec, i % carry == 0);
    else platform_update(s, e);
    out[i * 4] = (double)e.mp_x; out[i * 4 + 1] = (double)e.mp_y; out[i * 4 + 2] = (double)e.mp_u; out[i * 4 + 3] = (double)e.mp_v;
  }
}
// exhaustive self-test of sqrt_pos (dql_diag_selftest_sqrt) or, IEEE, of sqrt_(float) (dql_diag_selftest_sqrt_ieee): inputs with bit patterns lo .. hi
// against (float)sqrt((double)x)
template <bool IEEE> __global__ void k_selftest_sqrt(unsigned lo, unsigned hi, unsigned long long* bad) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long n = 0;
  for (unsigned long long b = lo + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b <= hi; b += stride) {
    const float x = __uint_as_float((unsigned)b);
    const float y = IEEE ? sqrt_(x) : sqrt_pos(x);
    if (__float_as_uint(y) != __float_as_uint((float)__builtin_sqrt((double)x))) ++n;
  }
  if (n) atomicAdd(bad, n);
}
// ---- the elementary functions and random draws of dql_device.hpp on the caller's inputs (dql_diag_det_math_run, dql_diag_box_muller_run, dql_diag_philox_run):
// thread i computes element i in blocks of DIAG_BLOCK (a multiple of 64), so elements 64 w .. 64 w + 63 share a wave — the float32 det_atan2 branches on a
// ballot over it.  Lanes past n leave before the first call ----
constexpr int DIAG_BLOCK = 256;
template <typename T> __global__ void k_det_math(const double* x, const double* y, long long n, double* s, double* c, double* at2, double* lg) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T xv = (T)x[i], yv = (T)y[i];
  T ss, cc;
  det_sincos(xv, ss, cc);
  s[i] = (double)ss; c[i] = (double)cc;
  at2[i] = (double)det_atan2(yv, xv);
  const T ax = abs_(xv);
  lg[i] = (double)det_log(ax > T(1e-30) ? ax : T(1.0));
}
template <typename T> __global__ void k_box_muller(const uint32_t* ra, const uint32_t* rb, long long n, double* n0, double* n1) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T a, b;
  box_muller<T>(ra[i], rb[i], a, b);
  n0[i] = (double)a; n1[i] = (double)b;
}
// KEYS: the 20 round keys in VGPRs, filled as k_step fills them from its seed
template <bool KEYS> __global__ void k_philox(const uint4* ctr, uint32_t k0, uint32_t k1, long long n, uint4* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t kv_[20];
  const uint32_t* kv = nullptr;
  if constexpr (KEYS) {
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr(k0 + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr(k1 + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  if (i >= n) return;
  const uint4 c = ctr[i];
  uint32_t r[4];
  philox4x32(c.x, c.y, c.z, c.w, k0, k1, r, kv);
  out[i] = make_uint4(r[0], r[1], r[2], r[3]);
}
template <typename T> __global__ void k_place(int init_mode, T p_max, const double* x0, const double* mp, long long n, double* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (double)place_axis(init_mode, (T)x0[i], (T)mp[i], p_max);
}

// shared by the C calls below (templates cannot live inside extern "C")
template <bool IEEE> static int selftest_sqrt(int device, uint32_t lo_bits, uint32_t hi_bits, int64_t* not_correctly_rounded) {
  if (!not_correctly_rounded) return fail(DQL_EINVAL, "null pointer");
  if (lo_bits > hi_bits || hi_bits > 0x7f7fffffu) return fail(DQL_EINVAL, "bit patterns must satisfy lo <= hi <= 0x7f7fffff (largest finite float32)");
  OP_PROLOGUE(device)
  DevBuf b;
  OUT(b, sizeof(unsigned long long));
  HIP_TRY(hipMemset(b.p, 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(k_selftest_sqrt<IEEE>, dim3(256 * 32), dim3(256), 0, 0, (unsigned)lo_bits, (unsigned)hi_bits, (unsigned long long*)b.p);
  HIP_TRY(hipGetLastError());
  unsigned long long n = 0;
  DOWN(&n, b, sizeof(n));
  *not_correctly_rounded = (int64_t)n;
  return DQL_OK;
}
static int diag_check_n(int32_t dtype, int64_t n, bool any_null) {
  if (dtype != DQL_F32 && dtype != DQL_F64) return fail(DQL_EINVAL, "dtype must be DQL_F32 or DQL_F64");
  if (n < 0 || n > DQL_DIAG_MAX_N) return fail(DQL_EINVAL, "n must be in 0 .. DQL_DIAG_MAX_N (2^24) per call");
  if (n > 0 && any_null) return fail(DQL_EINVAL, "null array");
  return DQL_OK;
}

extern "C" {
int dql_discretise(const dql_config* cfg, int device, const double* rel_p, const double* rel_v, const double* rel_a, const double* angle, int64_t n, int32_t* idx_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!rel_p || !rel_v || !rel_a || !angle || !idx_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf p, v, a, t, o;
  const size_t B = (size_t)n * sizeof(double);
  UP(p, rel_p, B); UP(v, rel_v, B); UP(a, rel_a, B); UP(t, angle, B);
  OUT(o, (size_t)n * sizeof(int));
  const unsigned grid = (unsigned)((n + 255) / 256);
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_discretise<T>, dim3(grid), dim3(256), 0, 0, make_mdpk<T>(*cfg), (const double*)p.p, (const double*)v.p, (const double*)a.p, (const double*)t.p, (long long)n, (int*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(idx_out, o, (size_t)n * sizeof(int));
  return DQL_OK;
}

int dql_mdp_transition(const dql_config* cfg, int device, int64_t n, uint32_t stages, const uint8_t* action, const double* obs, double* mdp_state,
                       const int32_t* prev_idx, int32_t* idx_io, double* reward_out, uint8_t* done_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!action || !obs || !mdp_state || !prev_idx || !idx_io || !reward_out || !done_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  if ((stages & DQL_MDP_ALL) == 0) return fail(DQL_EINVAL, "no stage selected");
  for (int64_t i = 0; i < n; ++i) if (action[i] > 2) return fail(DQL_EINVAL, "action must be 0, 1 or 2");
  if ((stages & (DQL_MDP_CHECK | DQL_MDP_REWARD)) && !(stages & DQL_MDP_DISCRETISE))
    for (int64_t i = 0; i < n; ++i) if (idx_io[i] < 0 || idx_io[i] >= DQL_N_STATES) return fail(DQL_ESTATE, "Cannot check an empty state: call discrete_state first");
  OP_PROLOGUE(device)
  DevBuf a, o, ms, pi, io, ro, dn;
  UP(a, action, (size_t)n); UP(o, obs, (size_t)n * 7 * sizeof(double)); UP(ms, mdp_state, (size_t)n * 8 * sizeof(double)); UP(pi, prev_idx, (size_t)n * sizeof(int));
  UP(io, idx_io, (size_t)n * sizeof(int)); UP(ro, reward_out, (size_t)n * sizeof(double)); UP(dn, done_out, (size_t)n);
  const unsigned grid = (unsigned)((n + 255) / 256);
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_mdp_transition<T>, dim3(grid), dim3(256), 0, 0, make_mdpk<T>(*cfg), (long long)n, stages, (const uint8_t*)a.p, (const double*)o.p, (double*)ms.p, (const int*)pi.p, (int*)io.p, (double*)ro.p, (uint8_t*)dn.p); });
  HIP_TRY(hipGetLastError());
  DOWN(mdp_state, ms, (size_t)n * 8 * sizeof(double));
  DOWN(idx_io, io, (size_t)n * sizeof(int));
  DOWN(reward_out, ro, (size_t)n * sizeof(double));
  DOWN(done_out, dn, (size_t)n);
  return DQL_OK;
}

int dql_manager_run(const dql_config* cfg, int device, int64_t n_series, int64_t n_ticks, const double* in, const uint8_t* contact, uint64_t seed, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n_series < 0 || n_ticks < 0 || ((n_series > 0 && n_ticks > 0) && (!in || !contact || !out))) return fail(DQL_EINVAL, "null array");
  if (n_series == 0 || n_ticks == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  const size_t cells = (size_t)n_series * (size_t)n_ticks;
  UP(a, in, cells * 14 * sizeof(double)); UP(b, contact, cells);
  OUT(o, cells * 12 * sizeof(double));
  dql_config c2 = *cfg;
  c2.two_axis = 1;  // the reference's estimator always runs on every axis; x-axis training configs simply never read y
  const unsigned grid = (unsigned)((n_series + 63) / 64);
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_manager_run<T>, dim3(grid), dim3(64), 0, 0, make_simk<T>(c2), (long long)n_series, (long long)n_ticks, (const double*)a.p, (const uint8_t*)b.p, (unsigned long long)seed, (double*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(out, o, cells * 12 * sizeof(double));
  return DQL_OK;
}

int dql_plant_run(const dql_config* cfg, int device, int64_t n_series, int64_t n_ticks, const double* init, const double* rotor_cmd, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n_series < 0 || n_ticks < 0 || ((n_series > 0 && n_ticks > 0) && (!init || !rotor_cmd || !out))) return fail(DQL_EINVAL, "null array");
  if (n_series == 0 || n_ticks == 0) return DQL_OK;
  const size_t cells = (size_t)n_series * (size_t)n_ticks;
  for (size_t k = 0; k < cells * 4; ++k) if (!(rotor_cmd[k] >= 0.0)) return fail(DQL_EINVAL, "rotor commands must be >= 0 (the attitude law commands sqrt(max(w^2, 0)))");
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  UP(a, init, (size_t)n_series * 21 * sizeof(double)); UP(b, rotor_cmd, cells * 4 * sizeof(double));
  OUT(o, cells * 20 * sizeof(double));
  const unsigned grid = (unsigned)((n_series + 63) / 64);
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_plant_run<T>, dim3(grid), dim3(64), 0, 0, make_simk<T>(*cfg), (long long)n_series, (long long)n_ticks, (const double*)a.p, (const double*)b.p, (double*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(out, o, cells * 20 * sizeof(double));
  return DQL_OK;
}

int dql_butterworth_run(const dql_config* cfg, int device, const double* x, int64_t n, double* y_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!x || !y_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, o;
  UP(a, x, (size_t)n * sizeof(double));
  OUT(o, (size_t)n * sizeof(double));
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_butterworth_run<T>, dim3(1), dim3(64), 0, 0, make_filtk<T>(cfg->bw_c), (const double*)a.p, (long long)n, (double*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(y_out, o, (size_t)n * sizeof(double));
  return DQL_OK;
}

int dql_kalman_run(const dql_config* cfg, int device, const double* vel, const uint8_t* dt_le0, int64_t n, double* acc_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 1 && (!vel || !dt_le0 || !acc_out))) return fail(DQL_EINVAL, "null array");
  if (n <= 1) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  UP(a, vel, (size_t)n * 3 * sizeof(double)); UP(b, dt_le0, (size_t)n);
  OUT(o, (size_t)(n - 1) * 3 * sizeof(double));
  const double r = cfg->noise_vel_sd * cfg->noise_vel_sd;  // pkg/filters.py:49
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_kalman_run<T>, dim3(1), dim3(64), 0, 0, (T)cfg->kalman_q, (T)r, (const double*)a.p, (const uint8_t*)b.p, (long long)n, (double*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(acc_out, o, (size_t)(n - 1) * 3 * sizeof(double));
  return DQL_OK;
}

int dql_pid_run(const dql_config* cfg, int device, const double* params, const double* state, int64_t n, double* effort_out, double* integral_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (!params || n < 0 || (n > 0 && (!state || !effort_out || !integral_out))) return fail(DQL_EINVAL, "null array");
  if (params[2] != 0.0) return fail(DQL_EINVAL, "Kd != 0 is not supported (the reference launches both controllers with Kd = 0, launch/drone.launch:37,51)");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, o, g;
  UP(a, state, (size_t)n * sizeof(double));
  OUT(o, (size_t)n * sizeof(double)); OUT(g, (size_t)n * sizeof(double));
  by_dtype(cfg->dtype, [&](auto ty) {
    using T = decltype(ty);
    const PidP<T> p{(T)params[0], (T)params[1], (T)params[3], (T)params[4], (T)params[5], (T)params[6]};
    hipLaunchKernelGGL(k_pid_run<T>, dim3(1), dim3(64), 0, 0, make_filtk<T>(cfg->bw_c), p, (const double*)a.p, (long long)n, (double*)o.p, (double*)g.p);
  });
  HIP_TRY(hipGetLastError());
  DOWN(effort_out, o, (size_t)n * sizeof(double));
  DOWN(integral_out, g, (size_t)n * sizeof(double));
  return DQL_OK;
}

int dql_attitude_run(const dql_config* cfg, int device, const double* quat_xyzw, const double* omega, const double* cmd, int64_t n, int32_t xonly, double* rotor_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!quat_xyzw || !omega || !cmd || !rotor_out))) return fail(DQL_EINVAL, "null array");
  if (xonly && cfg->dtype != DQL_F32) return fail(DQL_EINVAL, "the x-axis closed form of the attitude law exists in float32 only");
  if (xonly) for (int64_t i = 0; i < n; ++i) if (cmd[i * 4] != 0.0) return fail(DQL_EINVAL, "the x-axis closed form needs a roll command of exactly 0");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, c, o;
  UP(a, quat_xyzw, (size_t)n * 4 * sizeof(double)); UP(b, omega, (size_t)n * 3 * sizeof(double)); UP(c, cmd, (size_t)n * 4 * sizeof(double));
  OUT(o, (size_t)n * 4 * sizeof(double));
  const unsigned grid = (unsigned)((n + 63) / 64);
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_attitude_run<T>, dim3(grid), dim3(64), 0, 0, make_simk<T>(*cfg), (const double*)a.p, (const double*)b.p, (const double*)c.p, (long long)n, (int)xonly, (double*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(rotor_out, o, (size_t)n * 4 * sizeof(double));
  return DQL_OK;
}

int dql_platform_run(const dql_config* cfg, int device, int64_t n, int32_t carry, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || carry < 0 || (n > 0 && !out)) return fail(DQL_EINVAL, "bad argument");
  if (carry && cfg->dtype != DQL_F32) return fail(DQL_EINVAL, "the carried sine / cosine exists in the float32 step only");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf o;
  OUT(o, (size_t)n * 4 * sizeof(double));
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_platform_run<T>, dim3(1), dim3(64), 0, 0, make_simk<T>(*cfg), (long long)n, (int)carry, (double*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(out, o, (size_t)n * 4 * sizeof(double));
  return DQL_OK;
}

int dql_diag_selftest_sqrt(int device, uint32_t lo_bits, uint32_t hi_bits, int64_t* not_correctly_rounded) {
  return selftest_sqrt<false>(device, lo_bits, hi_bits, not_correctly_rounded);
}
int dql_diag_selftest_sqrt_ieee(int device, uint32_t lo_bits, uint32_t hi_bits, int64_t* not_correctly_rounded) {
  return selftest_sqrt<true>(device, lo_bits, hi_bits, not_correctly_rounded);
}

int dql_diag_det_math_run(int device, int32_t dtype, const double* x, const double* y, int64_t n, double* sin_out, double* cos_out, double* atan2_out, double* log_out) {
  int rc = diag_check_n(dtype, n, !x || !y || !sin_out || !cos_out || !atan2_out || !log_out); if (rc) return rc;
  OP_PROLOGUE(device)
  if (n == 0) return DQL_OK;
  DevBuf a, b, s, c, t, l;
  const size_t B = (size_t)n * sizeof(double);
  UP(a, x, B); UP(b, y, B);
  OUT(s, B); OUT(c, B); OUT(t, B); OUT(l, B);
  const unsigned grid = (unsigned)((n + DIAG_BLOCK - 1) / DIAG_BLOCK);
  by_dtype(dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_det_math<T>, dim3(grid), dim3(DIAG_BLOCK), 0, 0, (const double*)a.p, (const double*)b.p, (long long)n, (double*)s.p, (double*)c.p, (double*)t.p, (double*)l.p); });
  HIP_TRY(hipGetLastError());
  DOWN(sin_out, s, B); DOWN(cos_out, c, B); DOWN(atan2_out, t, B); DOWN(log_out, l, B);
  return DQL_OK;
}
int dql_diag_box_muller_run(int device, int32_t dtype, const uint32_t* ra, const uint32_t* rb, int64_t n, double* n0_out, double* n1_out) {
  int rc = diag_check_n(dtype, n, !ra || !rb || !n0_out || !n1_out); if (rc) return rc;
  OP_PROLOGUE(device)
  if (n == 0) return DQL_OK;
  DevBuf a, b, o0, o1;
  UP(a, ra, (size_t)n * sizeof(uint32_t)); UP(b, rb, (size_t)n * sizeof(uint32_t));
  OUT(o0, (size_t)n * sizeof(double)); OUT(o1, (size_t)n * sizeof(double));
  const unsigned grid = (unsigned)((n + DIAG_BLOCK - 1) / DIAG_BLOCK);
  by_dtype(dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_box_muller<T>, dim3(grid), dim3(DIAG_BLOCK), 0, 0, (const uint32_t*)a.p, (const uint32_t*)b.p, (long long)n, (double*)o0.p, (double*)o1.p); });
  HIP_TRY(hipGetLastError());
  DOWN(n0_out, o0, (size_t)n * sizeof(double)); DOWN(n1_out, o1, (size_t)n * sizeof(double));
  return DQL_OK;
}
int dql_diag_philox_run(int device, const uint32_t* counters, uint32_t k0, uint32_t k1, int32_t round_keys, int64_t n, uint32_t* out) {
  int rc = diag_check_n(DQL_F32, n, !counters || !out); if (rc) return rc;
  if (round_keys != 0 && round_keys != 1) return fail(DQL_EINVAL, "round_keys must be 0 (inline key schedule) or 1 (round keys in registers)");
  OP_PROLOGUE(device)
  if (n == 0) return DQL_OK;
  DevBuf a, o;
  UP(a, counters, (size_t)n * 4 * sizeof(uint32_t));
  OUT(o, (size_t)n * 4 * sizeof(uint32_t));
  const unsigned grid = (unsigned)((n + DIAG_BLOCK - 1) / DIAG_BLOCK);
  if (round_keys) hipLaunchKernelGGL(k_philox<true>, dim3(grid), dim3(DIAG_BLOCK), 0, 0, (const uint4*)a.p, k0, k1, (long long)n, (uint4*)o.p);
  else hipLaunchKernelGGL(k_philox<false>, dim3(grid), dim3(DIAG_BLOCK), 0, 0, (const uint4*)a.p, k0, k1, (long long)n, (uint4*)o.p);
  HIP_TRY(hipGetLastError());
  DOWN(out, o, (size_t)n * 4 * sizeof(uint32_t));
  return DQL_OK;
}

int dql_place(const dql_config* cfg, int device, const double* x0, const double* mp, int64_t n, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!x0 || !mp || !out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  UP(a, x0, (size_t)n * sizeof(double)); UP(b, mp, (size_t)n * sizeof(double));
  OUT(o, (size_t)n * sizeof(double));
  const unsigned grid = (unsigned)((n + 255) / 256);
  by_dtype(cfg->dtype, [&](auto ty) { using T = decltype(ty); hipLaunchKernelGGL(k_place<T>, dim3(grid), dim3(256), 0, 0, (int)cfg->init_uniform, (T)cfg->p_max, (const double*)a.p, (const double*)b.p, (long long)n, (double*)o.p); });
  HIP_TRY(hipGetLastError());
  DOWN(out, o, (size_t)n * sizeof(double));
  return DQL_OK;
}
}  // extern "C"
