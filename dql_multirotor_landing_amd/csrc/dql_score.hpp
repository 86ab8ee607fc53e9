// dql_score.hpp — greedy scoring of a table set: one env per lane flies episode after episode, the wave counts how they end (DESIGN.md sections 13 and 28).
//
// fly_episodes is THE episode loop of the greedy-flight family: k_score, k_score_map, k_model, k_returns_fly and k_score_grid and their host emulations all fly
// through it.  The env is built in registers by rollout_init_env and flown with agent_period<TICK, XMODE> (MODE_EVAL, or MODE_TRAIN with one wave-uniform
// threshold) for agent periods 0 .. max_steps, as rollout_episode does; but a lane does not leave at its first `done`: it notes the episode (terminal code,
// step_count & 0xffff), agent_period sends it through reset in the next period — exactly as a context driven one period at a time does — and it stops after
// `episodes` finished episodes.  There are no records of state and no trace: what comes out is the wave's tally (every lane gets the same one), filled in the
// caller's ScoreTally, and whatever the caller's hooks add at four points (FlyHooks).  Every accumulator is the caller's object, updated in place: an aggregate
// copied out of the loop moves the wave-uniform counters from SGPRs to VGPRs (section 28).
//
// score_episodes is the per-lane body of k_score (dql_greedy.inc) and of its host emulation (tests/host_emu/score_emu.cpp): the loop plus a compact per-episode log.
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

// what a body adds to the loop: it derives from this and states only the hooks it has (the others cost nothing)
//   period()                                      every lane, before every period
//   decision(before_x, before_y, e, o, done)      a lane that flies, after a period with o.decision: idx_x / idx_y from before the period, env and output after it
//   wave_end(done, code, e)                       every lane, after the nine code ballots of a period in which an episode of the wave ends
//   episode_end(finished, code, len)              the lane whose episode ended, after wave_end: the episode's number (from 0), terminal code and length
struct FlyHooks {
  DQL_DEV void period() {}
  template <typename E> DQL_DEV void decision(int, int, const E&, const StepOut&, bool) {}
  template <typename E> DQL_DEV void wave_end(bool, int, const E&) {}
  DQL_DEV void episode_end(int, int, int) {}
};

// c / cfgk / tc / mdp / mr / init / qa / qb / seed / env_id / mgr0 / sched / kv: as in rollout_episode.  mode / eps_thr: MODE_EVAL, 0 or MODE_TRAIN, the host's
// eps_threshold(eps), the same for every lane.  t: the caller's zeroed tally.
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename Hooks>
DQL_DEV void fly_episodes(ScoreTally& t, const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                          const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes, int mode, uint32_t eps_thr,
                          MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, Hooks& h) {
  Env<T> e;
  T mp_v_hbm;
  rollout_init_env(c, init, e, env_id, seed, mp_v_hbm);
  QRow qx = load_qrow(qa, qb, 0);  // a fresh env has no previous state: its row is never used
  const int n_eps = episodes < SCORE_MAX_EPISODES ? episodes : SCORE_MAX_EPISODES;
  const int last = max_steps < SCORE_MAX_STEPS ? max_steps : SCORE_MAX_STEPS;
  int finished = 0;
  unsigned lane_steps = 0u;  // at most SCORE_MAX_STEPS + 1 periods: fits
  bool flying = n_eps > 0;
  for (int j = 0; j <= last; ++j) {
    bool done = false;
    h.period();
    if (flying) {
      const int before_x = e.idx_x, before_y = e.idx_y;
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, qa, qb, mode, eps_thr, 2, seed, env_id, (long long)j, mgr0[j], sched[j], kv);
      qx = o.next;
      done = o.done != 0;
      if (o.decision) h.decision(before_x, before_y, e, o, done);  // not a reset period
    }
    if (__ballot(done) != 0ull) {  // wave-uniform: the bookkeeping runs in the few periods in which an episode of this wave ends
      const int code = e.code;
#pragma unroll
      for (int k = 0; k < DQL_N_CHECK_CODES; ++k) t.by_code[k] += (unsigned)__builtin_popcountll(__ballot(done && code == k));
      h.wave_end(done, code, e);
      if (done) {
        const int len = e.step_count & 0xffff;
        lane_steps += (unsigned)len;
        h.episode_end(finished, code, len);
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
}

// score's one addition, shared with the grid: the lane's finished episode goes into column g of the log
struct ScoreLogHooks : FlyHooks {
  const ScoreLog& log; long long g;
  DQL_DEV ScoreLogHooks(const ScoreLog& log_, long long g_) : log(log_), g(g_) {}
  DQL_DEV void episode_end(int finished, int code, int len) {
    if (log.code) {
      log.code[(long long)finished * log.n_total + g] = (uint8_t)code;
      log.steps[(long long)finished * log.n_total + g] = (uint16_t)len;
    }
  }
};

// fly_episodes' arguments in MODE_EVAL.  g: the lane's column of the log.
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr>
DQL_DEV ScoreTally score_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                  const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes, MgrPtr mgr0,
                                  SchedPtr sched, const uint32_t* kv, const ScoreLog& log, long long g) {
  ScoreTally t{};
  ScoreLogHooks h(log, g);
  fly_episodes<TICK, XMODE>(t, c, cfgk, tc, mdp, mr, init, qa, qb, seed, env_id, max_steps, episodes, MODE_EVAL, 0u, mgr0, sched, kv, h);
  return t;
}

}  // namespace dql
