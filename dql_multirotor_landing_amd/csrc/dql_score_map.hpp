// dql_score_map.hpp — greedy scoring that also counts every greedy decision by the cell it was made at (DESIGN.md sections 18 and 28).
//
// score_map_episodes is the per-lane body of k_score_map (dql_score_map.inc) and of its host emulation (tests/host_emu/score_map_emu.cpp).  It flies exactly what
// score_episodes flies — fly_episodes (dql_score.hpp) in MODE_EVAL: same env, same periods, same tally, same log — and its hooks add three things:
//   - after a period with o.decision they add 1 to the wave's histogram at cell idx_before * 3 + action (the state the period's action was decided from), for x
//     and, with two axes, for y (the tables are shared between the axes, so both land in the same map);
//   - they keep the cells of the period's decision;
//   - on `done` they write them to the log beside score's two entries.
// The histogram is the caller's: `hist.add(cell)` with 0 <= cell < DQL_N_CELLS (LDS atomics in the kernel, a plain array on the host).  Both the cell and the log
// index are range-checked here before anything is written; a violation is counted in the result's `faults` and dropped.
//
// Include after dql_score.hpp.
#pragma once
#include "dql_score.hpp"

namespace dql {

constexpr uint16_t SCORE_MAP_NO_CELL = 0xffff;
// the optional log: ScoreLog's two arrays and last_cell [2][episodes][n_total] (plane 0: x, plane 1: y; 0xffff = not finished, or no y axis); all null or all
// given, filled before the launch
struct ScoreMapLog { uint8_t* code; uint16_t* steps; uint16_t* last_cell; long long n_total; int episodes; };

struct ScoreMapTally { ScoreTally t; unsigned faults; };  // faults: this lane's range violations (0 unless a bug)

template <typename Hist> struct ScoreMapHooks : FlyHooks {
  const ScoreMapLog& log; long long g; Hist& hist; unsigned& faults; bool two;
  int cell_x = -1, cell_y = -1;  // where this period's decision was made (-1: none, or dropped)
  DQL_DEV ScoreMapHooks(const ScoreMapLog& log_, long long g_, Hist& hist_, unsigned& faults_, bool two_) : log(log_), g(g_), hist(hist_), faults(faults_), two(two_) {}
  DQL_DEV void period() { cell_x = -1; cell_y = -1; }
  template <typename E> DQL_DEV void decision(int before_x, int before_y, const E& e, const StepOut&, bool) {
    cell_x = before_x * 3 + (e.action & 3);
    if ((unsigned)cell_x < (unsigned)DQL_N_CELLS && (e.action & 3) < 3) hist.add(cell_x);
    else { ++faults; cell_x = -1; }
    if (two) {
      cell_y = before_y * 3 + ((e.action >> 2) & 3);
      if ((unsigned)cell_y < (unsigned)DQL_N_CELLS && ((e.action >> 2) & 3) < 3) hist.add(cell_y);
      else { ++faults; cell_y = -1; }
    }
  }
  DQL_DEV void episode_end(int finished, int code, int len) {
    if (log.code) {
      if (finished < log.episodes && g >= 0 && g < log.n_total) {
        const long long at = (long long)finished * log.n_total + g;
        log.code[at] = (uint8_t)code;
        log.steps[at] = (uint16_t)len;
        log.last_cell[at] = cell_x < 0 ? SCORE_MAP_NO_CELL : (uint16_t)cell_x;
        log.last_cell[(long long)log.episodes * log.n_total + at] = cell_y < 0 ? SCORE_MAP_NO_CELL : (uint16_t)cell_y;
      } else ++faults;
    }
  }
};

// arguments as score_episodes'; hist: the wave's histogram (see above)
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename Hist>
DQL_DEV ScoreMapTally score_map_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                         const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes, MgrPtr mgr0,
                                         SchedPtr sched, const uint32_t* kv, const ScoreMapLog& log, long long g, Hist& hist) {
  ScoreMapTally r{};
  ScoreMapHooks<Hist> h(log, g, hist, r.faults, XMODE == X_TWO && c.two_axis != 0);
  fly_episodes<TICK, XMODE>(r.t, c, cfgk, tc, mdp, mr, init, qa, qb, seed, env_id, max_steps, episodes, MODE_EVAL, 0u, mgr0, sched, kv, h);
  return r;
}

}  // namespace dql
