// dql_learner.hpp — one sequential Double-Q learner per lane: one env, its own three tables, the reference's update after every agent period
// (DESIGN.md section 12).
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

// DoubleQLearningAgent.update for one transition on the lane's own tables, operation for operation as oracle/dql_oracle.c orc_agent_update (double,
// no contraction).  next: both tables' row of s', read BEFORE the write.  Returns false (and writes nothing) when the cell is out of range.
DQL_DEV bool learner_update(double* qa, double* qb, double* count, const LearnSched& sc, uint32_t quirks, double gamma, int sa, bool coin, const QRow& next,
                            double reward, int mask, double& q_new, bool& sel_b_out) {
  if ((unsigned)sa >= (unsigned)DQL_N_CELLS) return false;
  const double cnt = count[sa];
  const double alpha = (cnt < (double)sc.n_alpha) ? sc.alpha_tab[(int)cnt] : sc.alpha_min;
  count[sa] = cnt + 1.0;
  const bool dbl = !(quirks & DQL_Q_UPDATE_TABLE_A_ONLY);
  const bool sel_b = dbl && coin;
  double s0 = next.a0, s1 = next.a1, s2 = next.a2, v0 = next.a0, v1 = next.a1, v2 = next.a2;
  if (dbl) {
    s0 = sel_b ? next.b0 : next.a0; s1 = sel_b ? next.b1 : next.a1; s2 = sel_b ? next.b2 : next.a2;
    v0 = sel_b ? next.a0 : next.b0; v1 = sel_b ? next.a1 : next.b1; v2 = sel_b ? next.a2 : next.b2;
  }
  const int b = argmax3(s0, s1, s2);
  const double best = b == 0 ? v0 : (b == 1 ? v1 : v2);
  double* qsel = sel_b ? qb : qa;
  const double q = qsel[sa];
  const double loss = alpha * (reward + (gamma * best) * (double)mask - q);
  q_new = q + loss;
  qsel[sa] = q_new;
  sel_b_out = sel_b;
  return true;
}

// c: the config the kernel loads and stores with (x_only(c)); cfgk / tc: the period's and the tick's constants in the layout's form.  sr / si: the env state
// arrays (stride mem.n).  l: this lane's learner; active: l < mem.n.  j0: the ensemble's period index at the launch's first period; mgr0 / sched: the tick
// schedule of periods j0 .. j0 + n_periods - 1 (fill_schedule).
template <int TICK, int XMODE, typename T, typename MgrPtr, typename SchedPtr>
DQL_DEV void learner_periods(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                             const LearnSched& sc, const LearnMem& mem, Quad<T>* sr, int4* si, uint64_t seed, long long l, bool active, long long j0,
                             int n_periods, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv) {
  bool live = active && mem.frozen[active ? l : 0] == 0;
  const long long lz = active ? l : 0;
  double* qa = mem.qa + lz * DQL_N_CELLS;
  double* qb = mem.qb + lz * DQL_N_CELLS;
  double* count = mem.count + lz * DQL_N_CELLS;
  Env<T> e = Env<T>{};
  QRow qx{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned long long decisions = 0ull, w0 = 0ull, w1 = 0ull;
  int episodes = 0, successes = 0, lvl_eps = 0, win_count = 0, promoted = -1, log_n = 0;
  uint32_t eps_thr = 0u;
  const bool loaded = live;
  if (live) {
    load_env(e, sr, si[l], mem.n, l, c);
    // the row of the state the env is in, from the tables as they stand (a reset period does not use it)
    qx = load_qrow((const double*)qa, (const double*)qb, e.idx_x < 0 ? 0 : e.idx_x);
    decisions = mem.decisions[l]; episodes = mem.episodes[l]; successes = mem.successes[l]; lvl_eps = mem.level_episodes[l]; win_count = mem.win_count[l];
    w0 = mem.win_bits[l]; w1 = mem.win_bits[mem.n + l]; promoted = mem.promoted[l]; log_n = mem.log_n[l];
    eps_thr = sc.eps_tab[lvl_eps < sc.n_eps ? lvl_eps : sc.n_eps - 1];
  }
  const int np = n_periods < LEARN_MAX_PERIODS ? n_periods : LEARN_MAX_PERIODS;
  for (int p = 0; p < np; ++p) {
    if (live) {
      const int prev_p = e.bin_p;
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, (const double*)qa, (const double*)qb, MODE_TRAIN, eps_thr, 2, seed, (uint32_t)l,
                                                  j0 + p, mgr0[p], sched[p], kv);
      qx = o.next;
      if (o.decision) {
        ++decisions;
        const bool coin = o.cell >= DQL_N_CELLS;  // the table the kernel's TD target picked: the coin under Double Q-learning, never set under B1/B2
        const int sa = coin ? o.cell - DQL_N_CELLS : o.cell;
        const int mask = (c.quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) ? (prev_p != e.bin_p) : !o.done;
        double q_new; bool sel_b;
        if (learner_update(qa, qb, count, sc, c.quirks, mr.gamma, sa, coin, o.next, (double)e.reward, mask, q_new, sel_b)) {
          // the carried row is the next period's greedy operand: when s' == s the write above changed it
          const int k = sa - e.idx_x * 3;
          if (k == 0) { if (sel_b) qx.b0 = q_new; else qx.a0 = q_new; }
          if (k == 1) { if (sel_b) qx.b1 = q_new; else qx.a1 = q_new; }
          if (k == 2) { if (sel_b) qx.b2 = q_new; else qx.a2 = q_new; }
        } else {
          mem.faults[0] += 1ull;  // never taken unless a bug: a plain (racy) count is enough to make the tests fail
        }
        if (o.done) {
          const int code = e.code;
          const int ok = code == DQL_TERMINAL_SUCCESS ? 1 : 0;
          ++episodes; successes += ok;
          if ((unsigned)code < (unsigned)DQL_N_CHECK_CODES) mem.by_code[(long long)code * mem.n + l] += 1ull;
          if (log_n < mem.log_cap) { mem.log_code[l * mem.log_cap + log_n] = (uint8_t)code; mem.log_len[l * mem.log_cap + log_n] = (uint16_t)e.step_count; }
          ++log_n;
          // the reference's deque (pkg/trainer.py:219-236): the last `window` outcomes at this level, as a ring of bits
          const int pos = lvl_eps % sc.window;
          const unsigned long long bit = 1ull << (pos & 63);
          unsigned long long w = pos >= 64 ? w1 : w0;
          win_count += ok - ((w & bit) ? 1 : 0);
          w = ok ? (w | bit) : (w & ~bit);
          if (pos >= 64) w1 = w; else w0 = w;
          ++lvl_eps;
          if (win_count >= sc.min_successes) { promoted = lvl_eps; live = false; }
          else if (lvl_eps >= sc.max_episodes) live = false;
          eps_thr = sc.eps_tab[lvl_eps < sc.n_eps ? lvl_eps : sc.n_eps - 1];
        }
      }
    }
    if (__ballot(live) == 0ull) break;
  }
  if (loaded) {
    store_env(e, sr, si, mem.n, l, c);
    mem.decisions[l] = decisions; mem.episodes[l] = episodes; mem.successes[l] = successes; mem.level_episodes[l] = lvl_eps; mem.win_count[l] = win_count;
    mem.win_bits[l] = w0; mem.win_bits[mem.n + l] = w1; mem.promoted[l] = promoted; mem.log_n[l] = log_n;
    mem.frozen[l] = live ? 0 : 1;
  }
}

}  // namespace dql
