// dql_refined.hpp — sequential learners and greedy scoring on a state split by one bit of hidden state.
//
// The refined state is r = half * DQL_N_STATES + idx_x, its cell r * 3 + action; a table set is double [2][DQL_N_CELLS], the half the slow index.  The half of
// the decision taken in period j is dql_model_split.hpp's, decision for decision:
//   value = split_feature(feature, env as it stands BEFORE period j, j, env_id, (uint32)seed)      half = value >= cut[idx_x before period j] ? 1 : 0
// so a body computes, after period j ends (reset periods included), the half of the state the env is NOW in from the env as it stands, with j + 1, and carries it
// into the next period (refined_half: the value, the range check, the comparison).  A value that is not finite or has |value| >= 8192 gives half 0 and a carried
// flag: the decision taken in that state is a fault (the learner drops its update and counts it, the scorer counts it and the host refuses the result).
//
// refined_learner_periods is the per-lane body of k_learn_refined (dql_refined.inc) and of its host emulation (tests/host_emu/refined_emu.cpp): learner_periods'
// loop (dql_learner.hpp) on refined indices.  agent_period gets the carried refined row as qx; its own o.next (the row of the UNREFINED next state, read from
// half 0's slice, which is all its table pointers have to reach) is ignored: the row of r' is loaded here, before the write.
// score_refined_episodes is the per-lane body of k_score_refined and of the same emulation: fly_episodes' loop text (dql_score.hpp) with the refined row in place of
// qx = o.next — its own text, as fly_episodes_before is, because a member added to the shared loop changes the code of the earlier kernels (section 32).
//
// The launch boundary: load_env zeroes obs_px / obs_vx / obs_ax, so the half of the state a learner stands in cannot be recomputed from the loaded env.  It is
// carried in a per-learner byte (RefinedMem::half: bit 0 the half, bit 1 "the value was out of range"), stored next to books_store and zero until the first reset
// period rewrites it (a reset period reads neither).
// Include after dql_learner.hpp, dql_score.hpp and dql_model_split.hpp.
#pragma once
#include "dql_learner.hpp"
#include "dql_model_split.hpp"
#include "dql_score.hpp"

namespace dql {

constexpr int REFINED_CELLS = 2 * DQL_N_CELLS;

// what dql_ensemble_set_refinement installs, next to LearnMem (whose qa / qb / count are then the refined arrays [L][2][DQL_N_CELLS])
struct RefinedMem {
  const double* cut;  // [DQL_N_STATES], no NaN
  uint8_t* half;      // [L] the half of the state each learner stands in, between launches
  int feature;        // DQL_SPLIT_* (wave-uniform)
};

// The half of the state the env is in, for the decision that period j will take: bit 0 the half, bit 1 set when the value is out of range (then the half is 0).
// at: the cut of that state.
template <typename E> DQL_DEV int refined_half(int feature, const E& e, int j, uint32_t env_id, uint32_t seed32, double at) {
  const double value = split_feature(feature, e, j, env_id, seed32);
  const bool value_ok = __builtin_fabs(value) < 8192.0;  // false for NaN and the infinities
  return value_ok ? (value >= at ? 1 : 0) : 2;
}
// the state index a table or the cut may be read at (0 for an index out of range: the decision is then dropped by the bounds guard)
DQL_DEV int refined_state(int idx_x) { return (unsigned)idx_x < (unsigned)DQL_N_STATES ? idx_x : 0; }

// learner_update (dql_learner.hpp) on a refined table set: cell half * DQL_N_CELLS + sa, sa the unrefined cell; the count and the learning rate are the refined
// cell's.  next: both tables' row of r', read BEFORE the write.  Returns false (and writes nothing) when the cell is out of range; cell_out: the refined cell.
DQL_DEV bool refined_update(double* qa, double* qb, double* count, const LearnSched& sc, uint32_t quirks, double gamma, int half, int sa, bool coin, const QRow& next,
                            double reward, int mask, double& q_new, bool& sel_b_out, int& cell_out) {
  const int cell = half * DQL_N_CELLS + sa;
  cell_out = cell;
  if ((unsigned)sa >= (unsigned)DQL_N_CELLS || (unsigned)half > 1u || (unsigned)cell >= (unsigned)REFINED_CELLS) return false;
  const double cnt = count[cell];
  const double alpha = learner_alpha(sc, cnt);
  count[cell] = cnt + 1.0;
  const bool dbl = !(quirks & DQL_Q_UPDATE_TABLE_A_ONLY);
  const bool sel_b = dbl && coin;
  const double best = learner_best(next, dbl, sel_b);
  double* qsel = sel_b ? qb : qa;
  const double q = qsel[cell];
  const double loss = alpha * (reward + (gamma * best) * (double)mask - q);
  q_new = q + loss;
  qsel[cell] = q_new;
  sel_b_out = sel_b;
  return true;
}

// Arguments as learner_periods'; mem.qa / mem.qb / mem.count: [L][2][DQL_N_CELLS]; rf: feature, cut and the carried byte.
template <int TICK, int XMODE, typename T, typename MgrPtr, typename SchedPtr>
DQL_DEV void refined_learner_periods(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                     const LearnSched& sc, const LearnMem& mem, const RefinedMem& rf, Quad<T>* sr, int4* si, uint64_t seed, long long l, bool active,
                                     long long j0, int n_periods, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv) {
  static_assert(XMODE == X_ONLY, "the refinement is the x MDP's");
  const long long lz = active ? l : 0;
  double* qa = mem.qa + lz * REFINED_CELLS;
  double* qb = mem.qb + lz * REFINED_CELLS;
  double* count = mem.count + lz * REFINED_CELLS;
  Env<T> e = Env<T>{};
  QRow qx{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  LearnerBooks t = LearnerBooks{};
  t.live = active && mem.frozen[lz] == 0;
  const bool loaded = t.live;
  int hb = 0;  // of the state the env is in: bit 0 the half, bit 1 the value was out of range
  if (loaded) {
    load_env(e, sr, si[l], mem.n, l, c);
    hb = rf.half[l] & 3;
    // the row of the refined state the env is in, from the tables as they stand (a reset period does not use it)
    qx = load_qrow((const double*)qa, (const double*)qb, (hb & 1) * DQL_N_STATES + refined_state(e.idx_x));
    t = books_load(sc, mem, l);
  }
  const int np = n_periods < LEARN_MAX_PERIODS ? n_periods : LEARN_MAX_PERIODS;
  for (int p = 0; p < np; ++p) {
    if (t.live) {
      const int prev_p = e.bin_p, hb_before = hb;
      // (agent_period also loads o.next, the row of the UNREFINED next state in half 0, and this body discards it: a load known to be dead, left there so
      //  that the shared period code stays the one every other kernel compiles; the measured cost of the refined lane includes it)
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, (const double*)qa, (const double*)qb, MODE_TRAIN, t.eps_thr, 2, seed, (uint32_t)l,
                                                  j0 + p, mgr0[p], sched[p], kv);
      // the half of the state just entered, for the decision of period j0 + p + 1: one load of the cut, by that state
      const int sx = refined_state(e.idx_x);
      hb = refined_half(rf.feature, e, (int)(uint32_t)(j0 + p + 1), (uint32_t)l, (uint32_t)seed, rf.cut[sx]);
      const int rx = (hb & 1) * DQL_N_STATES + sx;
      const QRow next = load_qrow((const double*)qa, (const double*)qb, rx);  // the row of r', before the write
      qx = next;
      if (o.decision) {
        ++t.decisions;
        const bool coin = o.cell >= DQL_N_CELLS;  // the table the kernel's TD target picked: the coin under Double Q-learning, never set under B1/B2
        const int sa = coin ? o.cell - DQL_N_CELLS : o.cell;
        const int mask = (c.quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) ? (prev_p != e.bin_p) : !o.done;
        double q_new; bool sel_b; int cell;
        if (!(hb_before & 2) && refined_update(qa, qb, count, sc, c.quirks, mr.gamma, hb_before & 1, sa, coin, next, (double)e.reward, mask, q_new, sel_b, cell)) {
          qrow_patch(qx, rx, cell, sel_b, q_new);  // when r' == r the write above changed the carried row (the same state in the other half: no patch)
        } else {
          mem.faults[0] += 1ull;  // never taken unless a bug: a plain (racy) count is enough to make the tests fail
        }
        if (o.done) {
          const int ok = books_episode(t, mem, l, e.code, e.step_count);
          if (books_ring_push(t, sc, ok)) t.live = false;
          t.eps_thr = eps_of_episode(sc, t.lvl_eps);
        }
      }
    }
    if (__ballot(t.live) == 0ull) break;
  }
  if (loaded) {
    store_env(e, sr, si, mem.n, l, c);
    books_store(t, mem, l);
    rf.half[l] = (uint8_t)hb;
  }
}

// fly_episodes' loop (dql_score.hpp) in MODE_EVAL on a refined table set qa / qb [2][DQL_N_CELLS]: the greedy row is that of r.  faults: this lane's decisions
// taken in a state whose value was out of range (0 unless a bug).  Everything else is fly_episodes', line by line: same env, same periods, same tally.
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename CutPtr, typename Hooks>
DQL_DEV void fly_refined_episodes(ScoreTally& t, unsigned& faults, const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp,
                                  const MdpRun<T>& mr, const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes,
                                  int feature, CutPtr cut, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, Hooks& h) {
  Env<T> e;
  T mp_v_hbm;
  rollout_init_env(c, init, e, env_id, seed, mp_v_hbm);
  QRow qx = load_qrow(qa, qb, 0);  // a fresh env has no previous state: its row is never used
  int hb = 0;                      // ... and no half: period 0 is a reset period
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
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, qa, qb, MODE_EVAL, 0u, 2, seed, env_id, (long long)j, mgr0[j], sched[j], kv);
      if (o.decision && (hb & 2)) ++faults;  // the decision just taken stood on a value out of range
      const int sx = refined_state(e.idx_x);
      hb = refined_half(feature, e, j + 1, env_id, (uint32_t)seed, cut[sx]);
      qx = load_qrow(qa, qb, (hb & 1) * DQL_N_STATES + sx);
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

struct ScoreRefinedTally { ScoreTally t; unsigned faults; };

// score_episodes' arguments plus feature and cut; qa / qb: the table set's [2][DQL_N_CELLS].  g: the lane's column of the log.
template <int TICK, int XMODE, typename T, typename TabPtr, typename MgrPtr, typename SchedPtr, typename CutPtr>
DQL_DEV ScoreRefinedTally score_refined_episodes(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                                 const RolloutInit<T>& init, TabPtr qa, TabPtr qb, uint64_t seed, uint32_t env_id, int max_steps, int episodes,
                                                 int feature, CutPtr cut, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, const ScoreLog& log, long long g) {
  static_assert(XMODE == X_ONLY, "the refinement is the x MDP's");
  ScoreRefinedTally r{};
  ScoreLogHooks h(log, g);
  fly_refined_episodes<TICK, XMODE>(r.t, r.faults, c, cfgk, tc, mdp, mr, init, qa, qb, seed, env_id, max_steps, episodes, feature, cut, mgr0, sched, kv, h);
  return r;
}

}  // namespace dql
