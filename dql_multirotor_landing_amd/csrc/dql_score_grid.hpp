// dql_score_grid.hpp — greedy scoring of K table sets over S scenarios in one launch, with the landing precision of the touchdowns (DESIGN.md sections 20 and 28).
//
// Three things in plain C++, shared by k_score_grid (dql_score_grid.inc) and its host emulation (tests/host_emu/grid_emu.cpp):
//   grid_coords          which scenario, table set and envs a block of the launch serves (scenario-major)
//   touch_bin            the bin of a touchdown's horizontal offset from the platform centre
//   score_grid_episodes  the per-lane body: fly_episodes (dql_score.hpp) with score's log — one env flies episode after episode under ITS scenario's constants —
//                        and one hook more: in the wave-uniform bookkeeping branch, eight ballots for the touch bins beside the nine for the terminal codes
// Nothing here knows where the scenario's constants come from: the caller hands them over as score_episodes' caller does.  Every output of a (scenario, set)
// is what score_episodes gives for that scenario's config alone; the touch bins are the only output it has no counterpart for.
//
// Include after dql_device.hpp, dql_rollout.hpp and dql_score.hpp.
#pragma once
#include "dql_device.hpp"
#include "dql_rollout.hpp"
#include "dql_score.hpp"

namespace dql {

constexpr int GRID_MAX_SCENARIOS = DQL_GRID_MAX_SCENARIOS, GRID_TOUCH_BINS = DQL_GRID_TOUCH_BINS, GRID_N_EDGES = DQL_GRID_TOUCH_BINS - 1;

// what differs between the scenarios of a launch besides MdpK<T>: one record per scenario in device memory, written by hipMemcpy before the launch only
template <typename T> struct GridScenario { SimK<T> c; MdpRun<T> mr; RolloutInit<T> init; T touch_edges[GRID_N_EDGES]; };

// edge_j = (T)(j * mp_half_x / 4), j = 1 .. 7: four bins inside the platform's half extent, four beyond it
template <typename T> static void make_touch_edges(const dql_config& c, T (&edges)[GRID_N_EDGES]) {
  for (int j = 1; j <= GRID_N_EDGES; ++j) edges[j - 1] = (T)((double)j * c.mp_half_x * 0.25);
}

// block b of S * K * B blocks (B = blocks_per_table = envs_per_table / 64): scenario b / (K B), table set (b / B) mod K, envs (b mod B) * 64 + lane.
// S * K * envs_per_table <= 2^30 (the host refuses more), so b and K B stay below 2^24: 32-bit divisions
struct GridCoords { int s, k, env0; };
DQL_DEV GridCoords grid_coords(unsigned block, unsigned blocks_per_table, unsigned n_tables) {
  const unsigned per_scenario = n_tables * blocks_per_table;
  const unsigned s = block / per_scenario, r = block - s * per_scenario;
  const unsigned k = r / blocks_per_table;
  return GridCoords{(int)s, (int)k, (int)((r - k * blocks_per_table) * 64u)};
}

// the number of edges d reaches; a NaN reaches none
template <typename T> DQL_DEV int touch_bin(T d, const T (&edges)[GRID_N_EDGES]) {
  int b = 0;
#pragma unroll
  for (int j = 0; j < GRID_N_EDGES; ++j) b += d >= edges[j] ? 1 : 0;
  return b;
}

// the drone's horizontal offset from the platform centre as the state shows it after the period (rollout_fields' px, mp_x, py, mp_y); the platform is a square
template <int XMODE, typename T> DQL_DEV T touch_offset(const Env<T>& e) {
  T d = e.p[0] - e.mp_x;
  d = d < T(0.0) ? -d : d;
  if constexpr (XMODE == X_TWO) {
    T dy = e.p[1] - e.mp_y;
    dy = dy < T(0.0) ? -dy : dy;
    if (dy > d || dy != dy) d = dy;  // the larger one; a NaN on either axis stays a NaN
  }
  return d;
}

struct GridTally { ScoreTally t; unsigned touch[GRID_TOUCH_BINS]; };

template <int XMODE, typename T> struct GridHooks : ScoreLogHooks {
  const T (&edges)[GRID_N_EDGES]; unsigned (&touch_hist)[GRID_TOUCH_BINS];
  DQL_DEV GridHooks(const ScoreLog& log_, long long g_, const T (&edges_)[GRID_N_EDGES], unsigned (&touch_)[GRID_TOUCH_BINS]) : ScoreLogHooks(log_, g_), edges(edges_), touch_hist(touch_) {}
  DQL_DEV void wave_end(bool done, int code, const Env<T>& e) {
    // a lane that is `done` here is within its first n_eps episodes (it stops flying after them): its touchdown counts, by the offset after this period
    const bool touch = done && code == DQL_TERMINAL_CONTACT;
    const int bin = touch_bin(touch_offset<XMODE>(e), edges);
#pragma unroll
    for (int b = 0; b < GRID_TOUCH_BINS; ++b) touch_hist[b] += (unsigned)__builtin_popcountll(__ballot(touch && bin == b));
  }
};

// score_episodes' arguments, plus the scenario's touch edges.  g: the lane's column of ITS SCENARIO's log (log.code / log.steps point at that scenario's slice).
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr>
DQL_DEV GridTally score_grid_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                      const RolloutInit<T>& init, const T (&edges)[GRID_N_EDGES], TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps,
                                      int episodes, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, const ScoreLog& log, long long g) {
  GridTally r{};
  GridHooks<XMODE, T> h(log, g, edges, r.touch);
  fly_episodes<TICK, XMODE>(r.t, c, cfgk, tc, mdp, mr, init, qa, qb, seed, env_id, max_steps, episodes, MODE_EVAL, 0u, mgr0, sched, kv, h);
  return r;
}

}  // namespace dql
