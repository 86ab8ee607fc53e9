// dql_rollout.hpp — one env's first greedy episode, from reset to termination, in one lane.
//
// rollout_episode is the per-lane body of k_rollout (dql_greedy.inc) and of its host emulation (tests/host_emu/rollout_emu.cpp): the env is
// built in registers as k_init builds it, flown with agent_period<TICK, XMODE> in MODE_EVAL for agent periods 0 .. max_steps (period 0 is the
// reset period of a fresh context) and left at the first period that reports `done`.  What it writes is what a context driven one period at a
// time shows through dql_get_sim_state / dql_get_sim_ints after that period, bit for bit.
//
// The loop runs max_steps + 1 times at most on every path: the data can only shorten it (a wave leaves when none of its lanes flies).
// Include after dql_device.hpp.
#pragma once
#include <cmath>

#include "dql_device.hpp"

namespace dql {

// Fields of a record (the first RO_N_RECORD) and of a trace row (all RO_N_TRACE), in output order; the names travel through the ABI
// (dql_rollout_field_name).  Real fields are widened to double (exact), the three int fields of the trace are small integers.
#define DQL_ROLLOUT_RECORD_FIELDS(X) \
  X(cum_x) X(cum_y) X(reward) X(px) X(py) X(pz) X(vx) X(vy) X(vz) X(mp_x) X(mp_u) X(mp_y) X(mp_v) X(qw) X(qx) X(qy) X(qz) X(pitch_sp) X(roll_sp)
#define DQL_ROLLOUT_TRACE_ONLY_FIELDS(X) X(action) X(idx_x) X(idx_y)
constexpr int RO_N_RECORD = 19, RO_N_TRACE = 22;
static const char* const k_rollout_field_names[RO_N_TRACE] = {
#define DQL_X(n) #n,
    DQL_ROLLOUT_RECORD_FIELDS(DQL_X) DQL_ROLLOUT_TRACE_ONLY_FIELDS(DQL_X)
#undef DQL_X
};

// what k_init's host side derives from the config (launch_init)
template <typename T> struct RolloutInit { T hover, vz_integ, r_lo, r_hi, t_lo, t_hi; };
template <typename T> static RolloutInit<T> make_rollout_init(const dql_config& c) {
  RolloutInit<T> a;
  a.hover = std::sqrt((T)(c.mass * c.gravity / (4.0 * c.k_f)));
  a.vz_integ = (T)(c.mass * c.gravity / c.pid_vz[1]);
  a.r_lo = (T)c.mp_r_lo; a.r_hi = (T)c.mp_r_hi; a.t_lo = (T)c.mp_t_lo; a.t_hi = (T)c.mp_t_hi;
  return a;
}

// the float32 Philox round keys of `seed` in VGPRs (float64 reads them from SGPRs: null), for every kernel that flies agent_period one env per lane: the
// greedy-flight family and the learners
template <typename T> DQL_DEV const uint32_t* lane_round_keys(uint64_t seed, uint32_t (&kv_)[20]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    return kv_;
  } else {
    return nullptr;
  }
}

// [n_total] codes and step counts, [RO_N_RECORD][n_total] record fields, [max_steps + 1][RO_N_TRACE][trace_envs] trace rows (or null)
struct RolloutOut { int* code; int* steps; double* rec; double* trace; long long n_total; int trace_envs; };

// A fresh env as the step kernel finds it in its first launch: k_init's draws (Philox STREAM_INIT, key (env id, seed)), then what store_env / load_env
// make of them for the config `c` the kernel loads with (an x-axis kernel's `c` has two_axis = 0).  mp_v_hbm: the platform's y velocity as k_init leaves
// it in the state array — what dql_get_sim_state keeps showing where the step kernel never stores that quad (x-axis configs on the circular trajectory).
template <typename T> DQL_DEV void rollout_init_env(const SimK<T>& c, const RolloutInit<T>& a, Env<T>& e, uint32_t env_id, uint64_t seed, T& mp_v_hbm) {
  uint32_t r[4];
  philox4x32(0u, 0u, env_id, STREAM_INIT, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  e = Env<T>{};
  e.q[0] = T(1.0); e.p[2] = c.z_init;
  for (int k = 0; k < 4; ++k) e.om[k] = a.hover;
  e.vz_i = a.vz_integ;
  e.kal_x_P = T(1.0); e.kal_y_P = T(1.0);
  e.mp_r = c.mp_r; e.mp_w = c.mp_w;
  if (c.per_env_platform && c.traj == DQL_TRAJ_RPM) {
    e.mp_r = fma_(u24<T>(r[1]), a.r_hi - a.r_lo, a.r_lo);
    const T tx = fma_(u24<T>(r[2]), a.t_hi - a.t_lo, a.t_lo);
    e.mp_w = tx / e.mp_r;
  }
  e.mp_phase = T(6.28318530717958623200e+00) * u24<T>(r[0]);
  platform_eval(c, e);
  mp_v_hbm = e.mp_v;
  e.code = DQL_NON_TERMINAL; e.idx_x = -1; e.idx_y = -1; e.flags = FL_DONE; e.action = 2;
  // load_env: the quads an x-axis kernel does not read, and the unpacked bins of the (absent) previous state
  if (!(c.two_axis || c.traj == DQL_TRAJ_EIGHT)) { e.mp_v = T(0.0); e.vf_y = T(0.0); e.kal_y_x = T(0.0); e.kal_y_P = T(1.0); }
  if (!c.per_env_platform) { e.mp_r = c.mp_r; e.mp_w = c.mp_w; }
  e.bin_k = idx_level(e.idx_x); e.bin_p = idx_pos(e.idx_x); e.bin_ky = idx_level(e.idx_y); e.bin_py = idx_pos(e.idx_y);
}

// the fields of a record / trace row as the state array shows them after the period (store_env: quads 11 and 12 are written for some configs only)
template <typename T> DQL_DEV void rollout_fields(const SimK<T>& c, const Env<T>& e, T mp_v_hbm, double (&f)[RO_N_TRACE]) {
  const T mp_v = (c.two_axis || c.traj == DQL_TRAJ_EIGHT) ? e.mp_v : mp_v_hbm;
  const T cum_y = c.two_axis ? e.cum_y : T(0.0);
  f[0] = (double)e.cum_x; f[1] = (double)cum_y; f[2] = (double)e.reward;
  f[3] = (double)e.p[0]; f[4] = (double)e.p[1]; f[5] = (double)e.p[2]; f[6] = (double)e.v[0]; f[7] = (double)e.v[1]; f[8] = (double)e.v[2];
  f[9] = (double)e.mp_x; f[10] = (double)e.mp_u; f[11] = (double)e.mp_y; f[12] = (double)mp_v;
  f[13] = (double)e.q[0]; f[14] = (double)e.q[1]; f[15] = (double)e.q[2]; f[16] = (double)e.q[3];
  f[17] = (double)e.pitch_sp; f[18] = (double)e.roll_sp;
  f[19] = (double)(e.action & 0xff); f[20] = (double)e.idx_x; f[21] = (double)e.idx_y;
}
template <typename T> DQL_DEV void rollout_write_record(const SimK<T>& c, const Env<T>& e, T mp_v_hbm, const RolloutOut& out, long long g, int code) {
  double f[RO_N_TRACE];
  rollout_fields(c, e, mp_v_hbm, f);
  out.code[g] = code; out.steps[g] = e.step_count & 0xffff;
#pragma unroll
  for (int k = 0; k < RO_N_RECORD; ++k) out.rec[(long long)k * out.n_total + g] = f[k];
}

// c: the config the kernel loads and stores with (x_only(c) in an x-axis kernel); cfgk / tc: the period's and the tick's constants in the layout's form,
// as k_step makes them once per launch.  qa / qb: this lane's table set.  mgr0 / sched: the tick schedule of periods 0 .. max_steps (fill_schedule).
// g: the lane's output column; trace_lane: this lane writes trace rows (column = g, a lane of table set 0's first wave); trace_wave: some lane of this wave does.
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr>
DQL_DEV void rollout_episode(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                             const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, MgrPtr mgr0, SchedPtr sched,
                             const uint32_t* kv, const RolloutOut& out, long long g, bool trace_wave, bool trace_lane) {
  Env<T> e;
  T mp_v_hbm;
  rollout_init_env(c, init, e, env_id, seed, mp_v_hbm);
  QRow qx = load_qrow(qa, qb, 0);  // a fresh env has no previous state: its row is never used (k_step loads row 0 for it as well)
  bool flying = true;
  for (int j = 0; j <= max_steps; ++j) {
    if (flying) {
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, qa, qb, MODE_EVAL, 0u, 2, seed, env_id, (long long)j, mgr0[j], sched[j], kv);
      qx = o.next;
      if (trace_wave) {  // wave-uniform: one wave of the launch at most
        if (trace_lane) {
          double f[RO_N_TRACE];
          rollout_fields(c, e, mp_v_hbm, f);
          double* row = out.trace + (long long)j * RO_N_TRACE * out.trace_envs + g;
#pragma unroll
          for (int k = 0; k < RO_N_TRACE; ++k) row[(long long)k * out.trace_envs] = f[k];
        }
      }
      if (o.done) { rollout_write_record(c, e, mp_v_hbm, out, g, e.code); flying = false; }
    }
    if (__ballot(flying) == 0ull) break;
  }
  if (flying) rollout_write_record(c, e, mp_v_hbm, out, g, -1);  // still in its first episode after max_steps: the state after the last period
}

}  // namespace dql
