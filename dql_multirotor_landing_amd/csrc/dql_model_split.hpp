// dql_model_split.hpp — the transition model split by one bit of hidden state.
//
// model_split_episodes is the per-lane body of k_model_split (dql_model_split.inc) and of its host emulation (tests/host_emu/split_model_emu.cpp).  It flies what
// model_episodes flies (dql_model.hpp: the family's episode loop in MODE_TRAIN with one wave-uniform threshold, here in fly_episodes_before; feature and cut touch no flight) and counts what it counts, but
// every counted decision goes to one of two halves: before(j, e) — the env as it stands before the period, the state the decision is taken in — keeps ONE value,
// the selected feature widened to double (not a copy of the env), and decision() compares it in double with the cut of the state before the period:
//   half = value >= cut[idx_x before] ? 1 : 0
// The sink then receives reward(half, cell, fx), terminal(half, cell, code) or pair(half, cell, next), and feature(state before, rint(value * 2^20)).  Checked here
// before the sink sees anything: the indices as in model_episodes, and the value finite with |value| < 8192 (so that value * 2^20 is exact and below 2^33), the half
// in {0, 1}; a violation is counted in `faults` and the whole period's contribution is dropped.  The feature is a wave-uniform switch; the coin reads nothing of
// the env.  Include after dql_score.hpp.
#pragma once
#include "dql_score.hpp"

namespace dql {

struct ModelSplitTally { ScoreTally t; unsigned faults; };  // faults: this lane's range violations (0 unless a bug)

// the coin of period j (include/dql.h): a hash of (env id, period, seed) that reads nothing of the env
DQL_DEV uint32_t split_coin(uint32_t env_id, int j, uint32_t seed32) {
  uint32_t x = env_id * 0x9E3779B1u + (uint32_t)j * 0x85EBCA77u + seed32;
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x >> 31;
}

// the selected feature of the env as it stands, widened to double (DQL_SPLIT_* of include/dql.h); an unknown code gives NaN, which the range check refuses
template <typename E> DQL_DEV double split_feature(int feature, const E& e, int j, uint32_t env_id, uint32_t seed32) {
  switch (feature) {  // wave-uniform
    case DQL_SPLIT_COIN: return (double)split_coin(env_id, j, seed32);
    case DQL_SPLIT_OBS_P_X: return (double)e.obs_px;
    case DQL_SPLIT_OBS_V_X: return (double)e.obs_vx;
    case DQL_SPLIT_OBS_A_X: return (double)e.obs_ax;
    case DQL_SPLIT_PITCH_SP: return (double)e.pitch_sp;
    case DQL_SPLIT_MP_PHASE: return (double)e.mp_phase;
    case DQL_SPLIT_MP_U: return (double)e.mp_u;
    case DQL_SPLIT_ALTITUDE: return (double)e.p[2];
    case DQL_SPLIT_V_Z: return (double)e.v[2];
    case DQL_SPLIT_STEP: return (double)(e.step_count & 0xffff);
    case DQL_SPLIT_PREV_ACTION: return (double)(e.action & 3);
    default: return __builtin_nan("");
  }
}

// fly_episodes' loop (dql_score.hpp) with a fifth point, h.before(j, e): a lane that flies, before period j runs — the env as the period's decision will be
// taken in it, reset periods included (the first decision of every episode follows a reset period, which calls no other hook with the env).  Its own text, not
// a change to the shared loop: with the empty member added there, eleven earlier kernels of the family were compiled to different code.
// Everything else is fly_episodes', line by line: same env, same periods, same tally.
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename Hooks>
DQL_DEV void fly_episodes_before(ScoreTally& t, const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
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
      h.before(j, e);
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

template <typename Sink, typename CutPtr> struct ModelSplitHooks : FlyHooks {
  Sink& sink; unsigned& faults; CutPtr cut; int feature; uint32_t env_id, seed32;
  double value = 0.0;  // the one thing carried across the period
  DQL_DEV ModelSplitHooks(Sink& sink_, unsigned& faults_, CutPtr cut_, int feature_, uint32_t env_id_, uint32_t seed32_)
      : sink(sink_), faults(faults_), cut(cut_), feature(feature_), env_id(env_id_), seed32(seed32_) {}
  template <typename E> DQL_DEV void before(int j, const E& e) { value = split_feature(feature, e, j, env_id, seed32); }
  template <typename E> DQL_DEV void decision(int before_x, int, const E& e, const StepOut& o, bool done) {
    const int action = e.action & 3, next = e.idx_x, code = e.code;
    const int cell = before_x * 3 + action;
    const bool state_ok = (unsigned)before_x < (unsigned)DQL_N_STATES;
    const double at = cut[state_ok ? before_x : 0];  // the cut of the state the decision was taken in
    const int half = value >= at ? 1 : 0;
    const bool value_ok = __builtin_fabs(value) < 8192.0;  // false for NaN and the infinities
    const bool ok = state_ok && action < 3 && (done ? (unsigned)code < (unsigned)DQL_N_CHECK_CODES : (unsigned)next < (unsigned)DQL_N_STATES) && value_ok && (unsigned)half < 2u;
    if (ok) {
      sink.feature(before_x, (long long)__builtin_rint(value * (double)(1 << DQL_SPLIT_FRAC_BITS)));
      sink.reward(half, cell, o.reward_fx);
      if (done) sink.terminal(half, cell, code);
      else sink.pair(half, cell, next);
    } else ++faults;
  }
};

// arguments as model_episodes'; feature: DQL_SPLIT_*; cut: [DQL_N_STATES] doubles, no NaN; sink: see above
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename CutPtr, typename Sink>
DQL_DEV ModelSplitTally model_split_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                             const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes,
                                             uint32_t eps_thr, int feature, CutPtr cut, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, Sink& sink) {
  static_assert(XMODE == X_ONLY, "the model is the x MDP's");
  ModelSplitTally r{};
  ModelSplitHooks<Sink, CutPtr> h(sink, r.faults, cut, feature, env_id, (uint32_t)seed);
  fly_episodes_before<TICK, XMODE>(r.t, c, cfgk, tc, mdp, mr, init, qa, qb, seed, env_id, max_steps, episodes, MODE_TRAIN, eps_thr, mgr0, sched, kv, h);
  return r;
}

}  // namespace dql
