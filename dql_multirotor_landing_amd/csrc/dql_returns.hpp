// dql_returns.hpp — realised discounted returns per (state, action) cell under an eps-greedy policy on fixed tables.
//
// Two per-lane bodies, shared by the kernels of dql_returns.inc and their host emulation (tests/host_emu/returns_emu.cpp):
//   ReturnsLogSink   a Sink of model_episodes (dql_model.hpp, instantiated unchanged).  It keeps the reward_fx of reward(cell, fx) and, on the terminal(cell,
//                    code) or pair(cell, next) that follows it, appends ONE 64-bit word to the lane's column of the decision log:
//                    traj[n_dec * n_columns + column].  Row = the lane's decision number, column = the lane: the lanes of a wave write neighbouring addresses
//                    of almost the same row.  Nothing else is written in the period loop; the log is not zeroed, n_dec says how much of a column is valid.
//   returns_sweep    walks a column backwards, t = t_top - 1 .. 0, taking part where t < n_dec (t_top: the largest n_dec of the lane's wave, so that the
//                    lanes of a wave walk together; a lane alone passes its own n_dec).  A lane is dead until it meets its first end flag: the decisions of an
//                    episode that max_steps cut off are counted in `cut` and contribute nothing.  At an end flag g restarts from 0; then
//                    g = (double)r_t + (gamma * g), two IEEE double operations, each rounded to nearest, never fused; the accumulator sink receives
//                    add(cell, llrint(g)).
// The log word: bits 0-47 the period's reward_fx in two's complement, bits 48-59 the cell, bit 63 "this period ended the episode" (bits 60-62 are zero).
// Range checks (a violation is counted in `faults` and its contribution dropped): a lane's decision count <= capacity = max_steps + 1 and the reward fits its
// 48-bit field (sink); n_dec <= capacity, cell < DQL_N_CELLS and |g| <= g_bound (sweep).  Include after dql_model.hpp.
#pragma once
#include "dql_model.hpp"

namespace dql {

constexpr unsigned long long RETURNS_END = 1ull << 63;
constexpr long long RETURNS_R_MAX = (1ll << 47) - 1;  // the reward field holds [-2^47, 2^47)

DQL_DEV bool returns_reward_fits(long long fx) { return fx >= -RETURNS_R_MAX - 1 && fx <= RETURNS_R_MAX; }
DQL_DEV unsigned long long returns_pack(int cell, long long fx, bool end) {
  return ((unsigned long long)fx & 0xffffffffffffull) | ((unsigned long long)(cell & 0xfff) << 48) | (end ? RETURNS_END : 0ull);
}
DQL_DEV long long returns_reward(unsigned long long w) { return (long long)(w << 16) >> 16; }  // sign-extends bit 47
DQL_DEV int returns_cell(unsigned long long w) { return (int)((w >> 48) & 0xfffull); }
DQL_DEV bool returns_end(unsigned long long w) { return (w & RETURNS_END) != 0ull; }

// WordPtr: unsigned long long* in the kernel, a bounds-checked reference on the host
template <typename WordPtr> struct ReturnsLogSink {
  WordPtr traj;
  size_t n_columns, column;
  unsigned capacity;  // max_steps + 1: the rows of the log
  unsigned n_dec = 0u, faults = 0u;
  long long fx = 0;
  DQL_DEV void reward(int, long long fx_) { fx = fx_; }
  DQL_DEV void terminal(int cell, int) { append(cell, true); }
  DQL_DEV void pair(int cell, int) { append(cell, false); }
  DQL_DEV void append(int cell, bool end) {
    if (n_dec >= capacity || (unsigned)cell >= (unsigned)DQL_N_CELLS || !returns_reward_fits(fx)) { ++faults; return; }
    traj[(size_t)n_dec * n_columns + column] = returns_pack(cell, fx, end);
    ++n_dec;
  }
};

// one step of the backward recursion in units of 2^-26: two roundings, whatever the translation unit's contraction setting
DQL_DEV double returns_step(double r, double gamma, double g) {
#pragma clang fp contract(off)
  const double m = gamma * g;
  return r + m;
}

struct ReturnsSweepTally { unsigned long long cut; unsigned faults; };

constexpr int RETURNS_SWEEP_BATCH = 4;  // log words read ahead of the recursion that consumes them (the loads do not depend on g)

// acc.add(cell, g_fx): cell < DQL_N_CELLS is checked here.  g_bound: ceil(B 2^26) of the host's overflow guard, as a double
template <typename WordPtr, typename Acc>
DQL_DEV ReturnsSweepTally returns_sweep(WordPtr traj, size_t n_columns, size_t column, unsigned n_dec, unsigned capacity, int t_top, double gamma, double g_bound, Acc& acc) {
  ReturnsSweepTally r{0ull, 0u};
  if (n_dec > capacity) { ++r.faults; n_dec = 0u; }  // never taken unless a bug: nothing of this column is read
  bool alive = false;
  double g = 0.0;
  for (int t0 = t_top - 1; t0 >= 0; t0 -= RETURNS_SWEEP_BATCH) {
    unsigned long long w[RETURNS_SWEEP_BATCH];
#pragma unroll
    for (int u = 0; u < RETURNS_SWEEP_BATCH; ++u) {
      const int t = t0 - u;
      w[u] = (t >= 0 && (unsigned)t < n_dec) ? traj[(size_t)t * n_columns + column] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < RETURNS_SWEEP_BATCH; ++u) {
      const int t = t0 - u;
      if (t >= 0 && (unsigned)t < n_dec) {
        if (returns_end(w[u])) { alive = true; g = 0.0; }
        if (alive) {
          g = returns_step((double)returns_reward(w[u]), gamma, g);
          const int cell = returns_cell(w[u]);
          if (cell < DQL_N_CELLS && __builtin_fabs(g) <= g_bound) acc.add(cell, (long long)rint_(g));
          else ++r.faults;
        } else ++r.cut;
      }
    }
  }
  return r;
}

}  // namespace dql
