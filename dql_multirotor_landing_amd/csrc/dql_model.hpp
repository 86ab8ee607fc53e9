// dql_model.hpp — the empirical transition model of the discretised x MDP under an eps-greedy policy on fixed tables (DESIGN.md sections 19 and 28).
//
// model_episodes is the per-lane body of k_model (dql_model.inc) and of its host emulation (tests/host_emu/model_emu.cpp).  It flies what score_episodes
// flies — fly_episodes (dql_score.hpp): same env, same periods, same tally — with one difference: agent_period runs in MODE_TRAIN with one wave-uniform threshold, so
// period_begin's own rule picks the action (explore iff (w[0] >> 8) < eps_thr, then (w[1] * 3) >> 32; else the greedy action of the carried row).  Nothing is
// learnt: the TD target agent_period makes in that mode is not used and no table is written.  After every period with o.decision (not a reset period) of a
// lane that still flies, with cell = idx_x before the period * 3 + action, the sink receives
//   - reward(cell, o.reward_fx), terminal periods included;
//   - terminal(cell, code) when the period ended the episode, pair(cell, idx_x after the period) when it did not.
// The sink is the caller's (in the kernel: global atomics for pairs and terminals, an LDS table for the rewards; plain arrays on the host).  Cell, next state and code are range-checked here before the sink sees
// them: 0 <= cell < DQL_N_CELLS, 0 <= s' < DQL_N_STATES, 0 <= code < DQL_N_CHECK_CODES; a violation is counted in the result's `faults` and the whole
// period's contribution is dropped.
//
// An x-axis body: the caller passes XMODE == X_ONLY
// and a SimK whose two_axis is 0 (the reward is not kept per axis).  Include after dql_score.hpp.
#pragma once
#include "dql_score.hpp"

namespace dql {

struct ModelTally { ScoreTally t; unsigned faults; };  // faults: this lane's range violations (0 unless a bug)

template <typename Sink> struct ModelHooks : FlyHooks {
  Sink& sink; unsigned& faults;
  DQL_DEV ModelHooks(Sink& sink_, unsigned& faults_) : sink(sink_), faults(faults_) {}
  template <typename E> DQL_DEV void decision(int before_x, int, const E& e, const StepOut& o, bool done) {
    const int action = e.action & 3, next = e.idx_x, code = e.code;
    const int cell = before_x * 3 + action;
    const bool ok = (unsigned)before_x < (unsigned)DQL_N_STATES && action < 3 && (done ? (unsigned)code < (unsigned)DQL_N_CHECK_CODES : (unsigned)next < (unsigned)DQL_N_STATES);
    if (ok) {
      sink.reward(cell, o.reward_fx);
      if (done) sink.terminal(cell, code);
      else sink.pair(cell, next);
    } else ++faults;
  }
};

// arguments as score_episodes'; eps_thr: host eps_threshold(eps), the same for every lane; sink: see above
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename Sink>
DQL_DEV ModelTally model_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                  const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes, uint32_t eps_thr,
                                  MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, Sink& sink) {
  static_assert(XMODE == X_ONLY, "the model is the x MDP's");
  ModelTally r{};
  ModelHooks<Sink> h(sink, r.faults);
  fly_episodes<TICK, XMODE>(r.t, c, cfgk, tc, mdp, mr, init, qa, qb, seed, env_id, max_steps, episodes, MODE_TRAIN, eps_thr, mgr0, sched, kv, h);
  return r;
}

}  // namespace dql
