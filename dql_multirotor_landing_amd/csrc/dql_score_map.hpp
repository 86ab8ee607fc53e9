// dql_score_map.hpp — greedy scoring that also counts every greedy decision by the cell it was made at.
//
// score_map_episodes is the per-lane body of k_score_map (dql_score_map.inc) and of its host emulation (tests/host_emu/score_map_emu.cpp).  It flies exactly what
// score_episodes (dql_score.hpp) flies — same env, same periods, same tally, same log — and is kept as a second body so that k_score's code does not move.  On top
// of scoring it does three things:
//   - it keeps the env's state indices from before agent_period (the state the period's action was decided from);
//   - after a period with o.decision it adds 1 to the wave's histogram at cell idx_before * 3 + action, for x and, with two axes, for y (the tables are
//     shared between the axes, so both land in the same map);
//   - on `done` it writes the cells of that last decision to the log.
// The histogram is the caller's: `hist.add(cell)` with 0 <= cell < DQL_N_CELLS (LDS atomics in the kernel, a plain array on the host).  Both the cell and the log
// index are range-checked here before anything is written; a violation is counted in the result's `faults` and dropped.
//
// The loop runs max_steps + 1 <= SCORE_MAX_STEPS + 1 times at most on every path, as score_episodes' does.  Include after dql_score.hpp.
#pragma once
#include "dql_score.hpp"

namespace dql {

constexpr uint16_t SCORE_MAP_NO_CELL = 0xffff;
constexpr int SCORE_MAP_SWEEPS = (DQL_N_CELLS + 63) / 64;  // the flush: lanes sweep contiguous cells, c = it * 64 + lane

// the optional log: ScoreLog's two arrays and last_cell [2][episodes][n_total] (plane 0: x, plane 1: y; 0xffff = not finished, or no y axis); all null or all
// given, filled before the launch
struct ScoreMapLog { uint8_t* code; uint16_t* steps; uint16_t* last_cell; long long n_total; int episodes; };

struct ScoreMapTally { ScoreTally t; unsigned faults; };  // faults: this lane's range violations (0 unless a bug)

// arguments as score_episodes'; hist: the wave's histogram (see above)
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename Hist>
DQL_DEV ScoreMapTally score_map_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                         const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes, MgrPtr mgr0,
                                         SchedPtr sched, const uint32_t* kv, const ScoreMapLog& log, long long g, Hist& hist) {
  Env<T> e;
  T mp_v_hbm;
  rollout_init_env(c, init, e, env_id, seed, mp_v_hbm);
  QRow qx = load_qrow(qa, qb, 0);  // a fresh env has no previous state: its row is never used
  ScoreMapTally r{};
  ScoreTally& t = r.t;
  const int n_eps = episodes < SCORE_MAX_EPISODES ? episodes : SCORE_MAX_EPISODES;
  const int last = max_steps < SCORE_MAX_STEPS ? max_steps : SCORE_MAX_STEPS;
  const bool two = XMODE == X_TWO && c.two_axis != 0;
  int finished = 0;
  unsigned lane_steps = 0u;  // at most SCORE_MAX_STEPS + 1 periods: fits
  bool flying = n_eps > 0;
  for (int j = 0; j <= last; ++j) {
    bool done = false;
    int cell_x = -1, cell_y = -1;  // where this period's decision was made (-1: none, or dropped)
    if (flying) {
      const int before_x = e.idx_x, before_y = e.idx_y;
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, qa, qb, MODE_EVAL, 0u, 2, seed, env_id, (long long)j, mgr0[j], sched[j], kv);
      qx = o.next;
      done = o.done != 0;
      if (o.decision) {  // not a reset period
        cell_x = before_x * 3 + (e.action & 3);
        if ((unsigned)cell_x < (unsigned)DQL_N_CELLS && (e.action & 3) < 3) hist.add(cell_x);
        else { ++r.faults; cell_x = -1; }
        if (two) {
          cell_y = before_y * 3 + ((e.action >> 2) & 3);
          if ((unsigned)cell_y < (unsigned)DQL_N_CELLS && ((e.action >> 2) & 3) < 3) hist.add(cell_y);
          else { ++r.faults; cell_y = -1; }
        }
      }
    }
    if (__ballot(done) != 0ull) {  // wave-uniform: the bookkeeping runs in the few periods in which an episode of this wave ends
      const int code = e.code;
#pragma unroll
      for (int k = 0; k < DQL_N_CHECK_CODES; ++k) t.by_code[k] += (unsigned)__builtin_popcountll(__ballot(done && code == k));
      if (done) {
        const int len = e.step_count & 0xffff;
        lane_steps += (unsigned)len;
        if (log.code) {
          if (finished < log.episodes && g >= 0 && g < log.n_total) {
            const long long at = (long long)finished * log.n_total + g;
            log.code[at] = (uint8_t)code;
            log.steps[at] = (uint16_t)len;
            log.last_cell[at] = cell_x < 0 ? SCORE_MAP_NO_CELL : (uint16_t)cell_x;
            log.last_cell[(long long)log.episodes * log.n_total + at] = cell_y < 0 ? SCORE_MAP_NO_CELL : (uint16_t)cell_y;
          } else ++r.faults;
        }
        ++finished;
        flying = finished < n_eps;
      }
    }
    if (__ballot(flying) == 0ull) break;
  }
  // the lanes' sums as sums over bit planes: ballots and scalar counts only, once per launch
  unsigned unfinished = 0u;
#pragma unroll
  for (int b = 0; b < 7; ++b) unfinished += (unsigned)__builtin_popcountll(__ballot((((unsigned)(n_eps - finished) >> b) & 1u) != 0u)) << b;
  t.by_code[DQL_N_CHECK_CODES] = unfinished;
#pragma unroll
  for (int b = 0; b < 13; ++b) t.steps += (unsigned long long)__builtin_popcountll(__ballot(((lane_steps >> b) & 1u) != 0u)) << b;
  return r;
}

}  // namespace dql
