// dql_score.hpp — greedy scoring of a table set: one env per lane flies episode after episode, the wave counts how they end.
//
// score_episodes is the per-lane body of k_score (dql_greedy.inc) and of its host emulation (tests/host_emu/score_emu.cpp).  The env is built in registers by
// rollout_init_env and flown with agent_period<TICK, XMODE> in MODE_EVAL for agent periods 0 .. max_steps, as rollout_episode does; but a lane does not leave
// at its first `done`: it notes the episode (terminal code, step_count & 0xffff), agent_period sends it through reset in the next period — exactly as a
// context driven one period at a time does — and it stops after `episodes` finished episodes.  There are no records of state and no trace: what comes out
// is the wave's tally (every lane returns the same one) and, optionally, a compact per-episode log.
//
// The loop runs max_steps + 1 <= SCORE_MAX_STEPS + 1 times at most on every path: the data can only shorten it (a wave leaves when none of its lanes flies).
// Include after dql_device.hpp and dql_rollout.hpp.
#pragma once
#include "dql_device.hpp"
#include "dql_rollout.hpp"

namespace dql {

constexpr int SCORE_MAX_STEPS = 4096, SCORE_MAX_EPISODES = 64, SCORE_N_COLS = DQL_N_CHECK_CODES + 1;

// what one wave adds to its table set's row: finished episodes by terminal code, then the episodes its lanes did not finish; the finished episodes' total length
struct ScoreTally { unsigned by_code[SCORE_N_COLS]; unsigned long long steps; };

// the optional log: [episodes][n_total] terminal code (0xff = not finished) and length (0 = not finished); both null or both given, filled before the launch
struct ScoreLog { uint8_t* code; uint16_t* steps; long long n_total; };

// c / cfgk / tc / mdp / mr / init / qa / qb / seed / env_id / mgr0 / sched / kv: as in rollout_episode.  g: the lane's column of the log.
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr>
DQL_DEV ScoreTally score_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                  const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes, MgrPtr mgr0,
                                  SchedPtr sched, const uint32_t* kv, const ScoreLog& log, long long g) {
  Env<T> e;
  T mp_v_hbm;
  rollout_init_env(c, init, e, env_id, seed, mp_v_hbm);
  QRow qx = load_qrow(qa, qb, 0);  // a fresh env has no previous state: its row is never used
  ScoreTally t{};
  const int n_eps = episodes < SCORE_MAX_EPISODES ? episodes : SCORE_MAX_EPISODES;
  const int last = max_steps < SCORE_MAX_STEPS ? max_steps : SCORE_MAX_STEPS;
  int finished = 0;
  unsigned lane_steps = 0u;  // at most SCORE_MAX_STEPS + 1 periods: fits
  bool flying = n_eps > 0;
  for (int j = 0; j <= last; ++j) {
    bool done = false;
    if (flying) {
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, qa, qb, MODE_EVAL, 0u, 2, seed, env_id, (long long)j, mgr0[j], sched[j], kv);
      qx = o.next;
      done = o.done != 0;
    }
    if (__ballot(done) != 0ull) {  // wave-uniform: the bookkeeping runs in the few periods in which an episode of this wave ends
      const int code = e.code;
#pragma unroll
      for (int k = 0; k < DQL_N_CHECK_CODES; ++k) t.by_code[k] += (unsigned)__builtin_popcountll(__ballot(done && code == k));
      if (done) {
        const int len = e.step_count & 0xffff;
        lane_steps += (unsigned)len;
        if (log.code) {
          log.code[(long long)finished * log.n_total + g] = (uint8_t)code;
          log.steps[(long long)finished * log.n_total + g] = (uint16_t)len;
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
  return t;
}

}  // namespace dql
