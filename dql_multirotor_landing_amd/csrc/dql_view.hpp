// dql_view.hpp — what TrainingLandingEnv.step returns, plus the continuous observation, per env, into caller-owned buffers (dql_view_dev).
//
// One per-lane body, shared by k_env_view (dql_view.inc) and its host emulation (tests/host_emu/view_emu.cpp):
//   env_view   lane i of the grid: nothing beyond the batch (i >= n).  It reads env i's packed ints and, as the outputs asked for need them, quads 7, 10, 14 and 15 of its real state; writes
//                obs[i][0..7]        obs_p_x, obs_v_x, obs_a_x, pitch_sp, obs_p_y, obs_v_y, obs_a_y, roll_sp  (q14.b, q14.c, q14.d, q7.d, q15.a, q15.b, q15.c, q10.c)
//                reward[i]           q14.a          cumulative_reward[i]  q10.b (cum_x)
//                idx_x[i], idx_y[i]  the packed states               step_count[i]  word z & 0xffff
//                code[i]             the low byte of word w          done[i], was_reset[i]  FL_DONE, FL_WAS_RESET of its second byte, as 0 / 1
//              exactly what dql_step_outputs decodes from the same words.  Env 0 also copies the bad-action counter (one word, not cleared).
//   view_cast  the one conversion contract: context element T -> output element R is (R)v.  T == R: the bits (a copy, no arithmetic); float -> double: exact;
//              double -> float: ONE cast, round to nearest even (the default rounding mode of the device and of the host), never a truncation and never two steps.
// An observation row is VIEW_OBS elements = 32 B (float) or 64 B (double), written as 16-byte vectors (ViewVec<R>: 4 floats or 2 doubles), so `obs` needs 16-byte
// alignment only — Quad<double> would ask for 32.
// How state and outputs are reached is a template argument: raw pointers in the kernel, bounds-checked references on the host.  An output that is not asked for
// tests false and is neither read nor written.  Include after dql_device.hpp.
#pragma once
#include "dql_device.hpp"

namespace dql {

constexpr int VIEW_OBS = DQL_VIEW_OBS;

template <typename R> struct ViewVec;
template <> struct alignas(16) ViewVec<float> { float v[4]; };
template <> struct alignas(16) ViewVec<double> { double v[2]; };

template <typename R, typename T> DQL_DEV R view_cast(T v) { return (R)v; }

// the outputs of a view as the kernel reaches them; the host emulation has the same members as checked references
template <typename R> struct ViewOut {
  ViewVec<R>* obs;  // [n][VIEW_OBS] as 16-byte vectors
  R* reward; R* cum;
  int32_t* idx_x; int32_t* idx_y; int32_t* step_count;
  uint8_t* done; uint8_t* was_reset; int8_t* code;
  unsigned long long* bad_actions;
};

template <typename T, typename R, typename QuadPtr, typename IntPtr, typename WordPtr, typename Out>
DQL_DEV void env_view(const QuadPtr& sr, const IntPtr& si, const WordPtr& bad_src, long long n, long long i, const Out& o) {
  if (i >= n) return;  // the tail workgroup's lanes beyond the batch
  const int4 iv = si[i];
  const bool want_obs = (bool)o.obs;
  if (want_obs || o.reward || o.cum) {
    const T zero = T(0.0);
    Quad<T> q7{zero, zero, zero, zero}, q10 = q7, q14 = q7, q15 = q7;
    if (want_obs || o.reward) q14 = sr[14 * n + i];
    if (want_obs || o.cum) q10 = sr[10 * n + i];
    if (want_obs) {
      q7 = sr[7 * n + i]; q15 = sr[15 * n + i];
      const R row[VIEW_OBS] = {view_cast<R>(q14.b), view_cast<R>(q14.c), view_cast<R>(q14.d), view_cast<R>(q7.d),
                               view_cast<R>(q15.a), view_cast<R>(q15.b), view_cast<R>(q15.c), view_cast<R>(q10.c)};
      constexpr int W = 16 / (int)sizeof(R), NV = VIEW_OBS / W;  // elements per 16-byte vector, vectors per row
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        ViewVec<R> v;
#pragma unroll
        for (int j = 0; j < W; ++j) v.v[j] = row[k * W + j];
        o.obs[(size_t)i * NV + k] = v;
      }
    }
    if (o.reward) o.reward[i] = view_cast<R>(q14.a);
    if (o.cum) o.cum[i] = view_cast<R>(q10.b);
  }
  const int fl = (iv.w >> 8) & 0xff;
  if (o.idx_x) o.idx_x[i] = iv.x;
  if (o.idx_y) o.idx_y[i] = iv.y;
  if (o.step_count) o.step_count[i] = iv.z & 0xffff;
  if (o.done) o.done[i] = (fl & FL_DONE) ? (uint8_t)1 : (uint8_t)0;
  if (o.was_reset) o.was_reset[i] = (fl & FL_WAS_RESET) ? (uint8_t)1 : (uint8_t)0;
  if (o.code) o.code[i] = (int8_t)(iv.w & 0xff);
  if (i == 0 && o.bad_actions) o.bad_actions[0] = bad_src[0];
}

}  // namespace dql
