// dql_learner.hpp — one sequential Double-Q learner per lane: one env, its own three tables, the reference's update after every agent period
//  — and what every kernel of the learner family shares:
//   the books    LearnerBooks, a learner's counters while a launch holds them in registers, with books_load / books_store; eps_of_episode, the threshold of the
//                episode to come; books_episode (totals, by_code, log) and books_ring_push (the promotion ring and the promote / exhaust decision), the two
//                halves of an episode's end.  The solo bodies call both halves, the team bodies (dql_team.hpp) the second only while the level is undecided.
//   the update   learner_best and learner_alpha, of which learner_update is written and which the n-step update (dql_nstep.hpp) shares; qrow_patch, the
//                carried row after a write to the row of the state the env is in.
// The float32 Philox round keys the seven learner kernels put in VGPRs are lane_round_keys (dql_rollout.hpp), shared with the greedy-flight family.
// The pending windows of the n-step learners are dql_nstep.hpp's.
//
// learner_periods is the per-lane body of k_learn (dql_ensemble.inc) and of its host emulation (tests/host_emu/learner_emu.cpp).  Learner l owns env l of a
// context made with dql_create(cfg, device, L, seed, 0) — the state arrays have that context's layout and are initialised by the same k_init — and the
// slices [l][DQL_N_CELLS] of Q_table_a, Q_table_b and state_action_counter.  A launch loads the env once, flies n_periods agent periods with
// agent_period<TICK, XMODE> in MODE_TRAIN (per-lane eps threshold) and applies DoubleQLearningAgent.update (pkg/double_q_learning.py:91-146) to the
// lane's own cells right after each of them, so the next period's greedy choice reads the updated tables: no accumulators, no fold, no delay.
//
// The loop runs n_periods <= DQL_ENSEMBLE_MAX_PERIODS times at most on every path: the data can only shorten it (a wave leaves when all its lanes are frozen).
// Include after dql_device.hpp.
#pragma once
#include "dql_device.hpp"

namespace dql {

constexpr int LEARN_MAX_PERIODS = 4096, LEARN_MAX_WINDOW = 128;

// what dql_ensemble_set_schedules installs (wave-uniform)
struct LearnSched {
  const double* alpha_tab; int n_alpha; double alpha_min;  // alpha(count) at the PRE-increment count (B5), alpha_min beyond the table
  const uint32_t* eps_tab; int n_eps;                      // eps threshold of the episode index within the level: eps_tab[min(e, n_eps - 1)]
  int window, min_successes, max_episodes;                 // freeze rules
};

// per-learner memory, all indexed by the learner l in [0, L)
struct LearnMem {
  double *qa, *qb, *count;                 // [L][DQL_N_CELLS]
  unsigned long long* decisions;           // [L]
  unsigned long long* by_code;             // [DQL_N_CHECK_CODES][L]
  int *episodes, *successes;               // [L] since creation
  int *level_episodes, *win_count;         // [L] at this level
  unsigned long long* win_bits;            // [2][L] ring of the last `window` episodes' outcomes
  int *promoted, *frozen;                  // [L] episode (count at this level) at which the window filled, or -1; 1 = frozen
  uint8_t* log_code; uint16_t* log_len;    // [L][log_cap] terminal code and length of episode k since the log was enabled
  int* log_n;                              // [L] episodes since the log was enabled (counts on beyond log_cap)
  unsigned long long* faults;              // [1] updates dropped by the bounds guard (0 unless a bug)
  long long n; int log_cap;
};

// ---- the books ----
// a learner's counters while a launch holds them in registers (a team's: in its applying lane's)
struct LearnerBooks {
  unsigned long long decisions, w0, w1;
  int episodes, successes, lvl_eps, win_count, promoted, log_n;
  uint32_t eps_thr;  // of the period to come: eps_of_episode(lvl_eps), the same for all envs of a team
  bool live;
};
// the eps threshold of episode e of a level
DQL_DEV uint32_t eps_of_episode(const LearnSched& sc, int e) { return sc.eps_tab[e < sc.n_eps ? e : sc.n_eps - 1]; }
DQL_DEV LearnerBooks books_load(const LearnSched& sc, const LearnMem& mem, long long l) {
  LearnerBooks t;
  t.decisions = mem.decisions[l]; t.episodes = mem.episodes[l]; t.successes = mem.successes[l]; t.lvl_eps = mem.level_episodes[l]; t.win_count = mem.win_count[l];
  t.w0 = mem.win_bits[l]; t.w1 = mem.win_bits[mem.n + l]; t.promoted = mem.promoted[l]; t.log_n = mem.log_n[l];
  t.eps_thr = eps_of_episode(sc, t.lvl_eps);
  t.live = mem.frozen[l] == 0;
  return t;
}
DQL_DEV void books_store(const LearnerBooks& t, const LearnMem& mem, long long l) {
  mem.decisions[l] = t.decisions; mem.episodes[l] = t.episodes; mem.successes[l] = t.successes; mem.level_episodes[l] = t.lvl_eps; mem.win_count[l] = t.win_count;
  mem.win_bits[l] = t.w0; mem.win_bits[mem.n + l] = t.w1; mem.promoted[l] = t.promoted; mem.log_n[l] = t.log_n;
  mem.frozen[l] = t.live ? 0 : 1;
}
// An episode of learner l that ended with terminal `code` after `steps` steps, into the totals, by_code and the log.  Returns its outcome: 1 for a success.
DQL_DEV int books_episode(LearnerBooks& t, const LearnMem& mem, long long l, int code, int steps) {
  const int ok = code == DQL_TERMINAL_SUCCESS ? 1 : 0;
  ++t.episodes; t.successes += ok;
  if ((unsigned)code < (unsigned)DQL_N_CHECK_CODES) mem.by_code[(long long)code * mem.n + l] += 1ull;
  if (t.log_n < mem.log_cap) { mem.log_code[l * mem.log_cap + t.log_n] = (uint8_t)code; mem.log_len[l * mem.log_cap + t.log_n] = (uint16_t)steps; }
  ++t.log_n;
  return ok;
}
// An outcome into the ring.  Returns whether the level is now decided: promoted (t.promoted is set) or out of episodes.
DQL_DEV bool books_ring_push(LearnerBooks& t, const LearnSched& sc, int ok) {
  // the reference's deque (pkg/trainer.py:219-236): the last `window` outcomes at this level, as a ring of bits
  const int pos = t.lvl_eps % sc.window;
  const unsigned long long bit = 1ull << (pos & 63);
  unsigned long long w = pos >= 64 ? t.w1 : t.w0;
  t.win_count += ok - ((w & bit) ? 1 : 0);
  w = ok ? (w | bit) : (w & ~bit);
  if (pos >= 64) t.w1 = w; else t.w0 = w;
  ++t.lvl_eps;
  if (t.win_count >= sc.min_successes) { t.promoted = t.lvl_eps; return true; }
  return t.lvl_eps >= sc.max_episodes;
}

// ---- the update ----
// the table assignment: the selecting table's arg-max, valued by the other table under Double Q-learning, by table a itself otherwise
DQL_DEV double learner_best(const QRow& next, bool dbl, bool sel_b) {
  double s0 = next.a0, s1 = next.a1, s2 = next.a2, v0 = next.a0, v1 = next.a1, v2 = next.a2;
  if (dbl) {
    s0 = sel_b ? next.b0 : next.a0; s1 = sel_b ? next.b1 : next.a1; s2 = sel_b ? next.b2 : next.a2;
    v0 = sel_b ? next.a0 : next.b0; v1 = sel_b ? next.a1 : next.b1; v2 = sel_b ? next.a2 : next.b2;
  }
  const int b = argmax3(s0, s1, s2);
  return b == 0 ? v0 : (b == 1 ? v1 : v2);
}
// the learning rate: alpha(count) at the pre-increment count (B5), alpha_min beyond the table
DQL_DEV double learner_alpha(const LearnSched& sc, double cnt) { return (cnt < (double)sc.n_alpha) ? sc.alpha_tab[(int)cnt] : sc.alpha_min; }
// DoubleQLearningAgent.update for one transition on the lane's own tables, operation for operation as oracle/dql_oracle.c orc_agent_update (double,
// no contraction).  next: both tables' row of s', read BEFORE the write.  Returns false (and writes nothing) when the cell is out of range.
DQL_DEV bool learner_update(double* qa, double* qb, double* count, const LearnSched& sc, uint32_t quirks, double gamma, int sa, bool coin, const QRow& next,
                            double reward, int mask, double& q_new, bool& sel_b_out) {
  if ((unsigned)sa >= (unsigned)DQL_N_CELLS) return false;
  const double cnt = count[sa];
  const double alpha = learner_alpha(sc, cnt);
  count[sa] = cnt + 1.0;
  const bool dbl = !(quirks & DQL_Q_UPDATE_TABLE_A_ONLY);
  const bool sel_b = dbl && coin;
  const double best = learner_best(next, dbl, sel_b);
  double* qsel = sel_b ? qb : qa;
  const double q = qsel[sa];
  const double loss = alpha * (reward + (gamma * best) * (double)mask - q);
  q_new = q + loss;
  qsel[sa] = q_new;
  sel_b_out = sel_b;
  return true;
}
// the carried row qx (of state idx_x) is the next period's greedy operand: a write of q_new to cell sa of table b (sel_b) or a changed it when sa lies in that row
DQL_DEV void qrow_patch(QRow& qx, int idx_x, int sa, bool sel_b, double q_new) {
  const int k = sa - idx_x * 3;
  if (k == 0) { if (sel_b) qx.b0 = q_new; else qx.a0 = q_new; }
  if (k == 1) { if (sel_b) qx.b1 = q_new; else qx.a1 = q_new; }
  if (k == 2) { if (sel_b) qx.b2 = q_new; else qx.a2 = q_new; }
}

// c: the config the kernel loads and stores with (x_only(c)); cfgk / tc: the period's and the tick's constants in the layout's form.  sr / si: the env state
// arrays (stride mem.n).  l: this lane's learner; active: l < mem.n.  j0: the ensemble's period index at the launch's first period; mgr0 / sched: the tick
// schedule of periods j0 .. j0 + n_periods - 1 (fill_schedule).
template <int TICK, int XMODE, typename T, typename MgrPtr, typename SchedPtr>
DQL_DEV void learner_periods(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                             const LearnSched& sc, const LearnMem& mem, Quad<T>* sr, int4* si, uint64_t seed, long long l, bool active, long long j0,
                             int n_periods, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv) {
  const long long lz = active ? l : 0;
  double* qa = mem.qa + lz * DQL_N_CELLS;
  double* qb = mem.qb + lz * DQL_N_CELLS;
  double* count = mem.count + lz * DQL_N_CELLS;
  Env<T> e = Env<T>{};
  QRow qx{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  LearnerBooks t = LearnerBooks{};
  t.live = active && mem.frozen[lz] == 0;
  const bool loaded = t.live;
  if (loaded) {
    load_env(e, sr, si[l], mem.n, l, c);
    // the row of the state the env is in, from the tables as they stand (a reset period does not use it)
    qx = load_qrow((const double*)qa, (const double*)qb, e.idx_x < 0 ? 0 : e.idx_x);
    t = books_load(sc, mem, l);
  }
  const int np = n_periods < LEARN_MAX_PERIODS ? n_periods : LEARN_MAX_PERIODS;
  for (int p = 0; p < np; ++p) {
    if (t.live) {
      const int prev_p = e.bin_p;
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, (const double*)qa, (const double*)qb, MODE_TRAIN, t.eps_thr, 2, seed, (uint32_t)l,
                                                  j0 + p, mgr0[p], sched[p], kv);
      qx = o.next;
      if (o.decision) {
        ++t.decisions;
        const bool coin = o.cell >= DQL_N_CELLS;  // the table the kernel's TD target picked: the coin under Double Q-learning, never set under B1/B2
        const int sa = coin ? o.cell - DQL_N_CELLS : o.cell;
        const int mask = (c.quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) ? (prev_p != e.bin_p) : !o.done;
        double q_new; bool sel_b;
        if (learner_update(qa, qb, count, sc, c.quirks, mr.gamma, sa, coin, o.next, (double)e.reward, mask, q_new, sel_b)) {
          qrow_patch(qx, e.idx_x, sa, sel_b, q_new);  // when s' == s the write above changed the carried row
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
  }
}

}  // namespace dql
