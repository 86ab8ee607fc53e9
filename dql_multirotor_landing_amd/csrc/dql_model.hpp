// dql_model.hpp — the empirical transition model of the discretised x MDP under an eps-greedy policy on fixed tables.
//
// model_episodes is the per-lane body of k_model (dql_model.inc) and of its host emulation (tests/host_emu/model_emu.cpp).  It flies what score_map_episodes
// (dql_score_map.hpp) flies — same env, same periods, same tally — with one difference: agent_period runs in MODE_TRAIN with one wave-uniform threshold, so
// period_begin's own rule picks the action (explore iff (w[0] >> 8) < eps_thr, then (w[1] * 3) >> 32; else the greedy action of the carried row).  Nothing is
// learnt: the TD target agent_period makes in that mode is not used and no table is written.  After every period with o.decision (not a reset period) of a
// lane that still flies, with cell = idx_x before the period * 3 + action, the sink receives
//   - reward(cell, o.reward_fx), terminal periods included;
//   - terminal(cell, code) when the period ended the episode, pair(cell, idx_x after the period) when it did not.
// The sink is the caller's (in the kernel: global atomics for pairs and terminals, an LDS table for the rewards; plain arrays on the host).  Cell, next state and code are range-checked here before the sink sees
// them: 0 <= cell < DQL_N_CELLS, 0 <= s' < DQL_N_STATES, 0 <= code < DQL_N_CHECK_CODES; a violation is counted in the result's `faults` and the whole
// period's contribution is dropped.
//
// The loop runs max_steps + 1 <= SCORE_MAX_STEPS + 1 times at most on every path, as score_episodes' does.  An x-axis body: the caller passes XMODE == X_ONLY
// and a SimK whose two_axis is 0 (the reward is not kept per axis).  Include after dql_score.hpp.
#pragma once
#include "dql_score.hpp"

namespace dql {

struct ModelTally { ScoreTally t; unsigned faults; };  // faults: this lane's range violations (0 unless a bug)

// arguments as score_episodes'; eps_thr: host eps_threshold(eps), the same for every lane; sink: see above
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename Sink>
DQL_DEV ModelTally model_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                  const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes, uint32_t eps_thr,
                                  MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, Sink& sink) {
  static_assert(XMODE == X_ONLY, "the model is the x MDP's");
  Env<T> e;
  T mp_v_hbm;
  rollout_init_env(c, init, e, env_id, seed, mp_v_hbm);
  QRow qx = load_qrow(qa, qb, 0);  // a fresh env has no previous state: its row is never used
  ModelTally r{};
  ScoreTally& t = r.t;
  const int n_eps = episodes < SCORE_MAX_EPISODES ? episodes : SCORE_MAX_EPISODES;
  const int last = max_steps < SCORE_MAX_STEPS ? max_steps : SCORE_MAX_STEPS;
  int finished = 0;
  unsigned lane_steps = 0u;  // at most SCORE_MAX_STEPS + 1 periods: fits
  bool flying = n_eps > 0;
  for (int j = 0; j <= last; ++j) {
    bool done = false;
    if (flying) {
      const int before_x = e.idx_x;
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, qa, qb, MODE_TRAIN, eps_thr, 2, seed, env_id, (long long)j, mgr0[j], sched[j], kv);
      qx = o.next;
      done = o.done != 0;
      if (o.decision) {  // not a reset period
        const int action = e.action & 3, next = e.idx_x, code = e.code;
        const int cell = before_x * 3 + action;
        const bool ok = (unsigned)before_x < (unsigned)DQL_N_STATES && action < 3 && (done ? (unsigned)code < (unsigned)DQL_N_CHECK_CODES : (unsigned)next < (unsigned)DQL_N_STATES);
        if (ok) {
          sink.reward(cell, o.reward_fx);
          if (done) sink.terminal(cell, code);
          else sink.pair(cell, next);
        } else ++r.faults;
      }
    }
    if (__ballot(done) != 0ull) {  // wave-uniform: the bookkeeping runs in the few periods in which an episode of this wave ends
      const int code = e.code;
#pragma unroll
      for (int k = 0; k < DQL_N_CHECK_CODES; ++k) t.by_code[k] += (unsigned)__builtin_popcountll(__ballot(done && code == k));
      if (done) {
        lane_steps += (unsigned)(e.step_count & 0xffff);
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
