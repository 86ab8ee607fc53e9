// dql_team_nstep.hpp — the team learner of dql_team.hpp with the uncorrected n-step Double-Q return of dql_nstep.hpp as its target, 1 <= n <= DQL_NSTEP_MAX
// (DESIGN.md section 24): one PENDING WINDOW PER ENV, the E records of a period still applied one after the other in env order.
//
// team_env_period and TeamRecord are dql_team.hpp's, unchanged.  team_apply_nstep stands beside team_apply: everything but the update is team_apply's — the
// decisions, the episode bookkeeping, the ring, "a level once decided takes no further outcome into its ring in that period", the freeze at the period's end.
// For the record of env k (k = 0 .. E - 1, in that order) that made a decision:
//   1. the decision's entry (cell, coin, reward as a double) is appended to env k's window;
//   2. both tables' row of s' is read ONCE, at this env's turn: after every write envs < k made in this period, before this env's own writes;
//   3. mask is the record's (team_env_period: the position-bin test under DQL_Q_BOOTSTRAP_ON_POS_CHANGE, !done otherwise);
//   4. if the period ended the env's episode every entry is updated, oldest first, and the window emptied; else if the window holds n entries the oldest is
//      updated and removed; else nothing is updated.
// One update is dql_nstep.hpp's, operation for operation: sel_b = Double Q-learning and the ENTRY's own coin; best = nstep_best on the row of step 2;
// g = best * mask, then for i = m - 1 down to k: g = r_i + (gamma * g) (returns_step); alpha at the cell's count AS IT STANDS AT THAT MOMENT, pre-increment;
// q_new = q + alpha * (g - q) on the value that stands at that moment — team-mates may have written the entry's cell since it was appended.
// With E = 1 this is learner_periods_nstep operation for operation; with n = 1 it is team_apply bit for bit (dql_nstep.hpp's argument about
// gamma * (best * mask)).  A cell outside the tables, or an s' outside them, is counted in `faults`; nothing is updated for it and the window keeps its shape:
// at most n - 1 entries after the record, none after a `done`.
//
// A team freezes at the end of the deciding period, when its envs are mostly in the middle of an episode: A FROZEN TEAM'S WINDOWS ARE GENERALLY NOT EMPTY
// (unlike dql_nstep.hpp's, whose learner freezes on the flush of its one env).  They persist per env and fly on after a rearm.
//
// How the team's windows are reached is a template parameter, TWin: key(k, slot) / val(k, slot) with slot in [0, n), head(k) and len(k) of env k of the team
// (the kernel's are LDS, [slot][lane] and [lane]).  key / val are dql_nstep.hpp's; the window is its ring: position i sits in slot (head + i) mod n.  All
// window work of a team is done by the lane that applies; never a per-lane array indexed at run time.
//
// On the device the windows travel under the two workgroup barriers of k_learn_team's period (dql_team.hpp): a lane writes its env's window into LDS before
// the launch's first barrier, only the applying lane touches the team's windows between the barriers, and every lane reads its own column back after the
// last one.  LDS of one workgroup under __syncthreads() needs no more than that.
//
// Every loop is bounded by E or by n on every path.  Include after dql_team.hpp and dql_nstep.hpp.
#pragma once
#include "dql_team.hpp"
#include "dql_nstep.hpp"

namespace dql {

template <typename RecPtr, typename TWin>
DQL_DEV void team_apply_nstep(const LearnSched& sc, const LearnMem& mem, uint32_t quirks, double gamma, long long l, RecPtr rec, int n_envs, int nstep, TWin tw,
                              TeamState& t) {
  double* qa = mem.qa + l * DQL_N_CELLS;
  double* qb = mem.qb + l * DQL_N_CELLS;
  double* count = mem.count + l * DQL_N_CELLS;
  const int ne = n_envs < TEAM_MAX_ENVS ? n_envs : TEAM_MAX_ENVS;
  const int ns = nstep < 1 ? 1 : (nstep > NSTEP_MAX ? NSTEP_MAX : nstep);
  const bool dbl = !(quirks & DQL_Q_UPDATE_TABLE_A_ONLY);
  bool decided = false;
  for (int k = 0; k < ne; ++k) {
    const TeamRecord r = rec[k];
    if (!(r.what & TEAM_DECISION)) continue;
    ++t.decisions;
    const bool coin = r.cell >= DQL_N_CELLS;
    const int sa_new = coin ? r.cell - DQL_N_CELLS : r.cell;
    // 1. the decision's entry (m < ns here: a full window gave up its oldest entry in the period that filled it)
    int head = tw.head(k), m = tw.len(k);
    head = (unsigned)head < (unsigned)ns ? head : 0;
    m = m < 0 ? 0 : (m > ns - 1 ? ns - 1 : m);
    const int tail = nstep_slot(head, m, ns);
    tw.key(k, tail) = nstep_pack(sa_new, coin); tw.val(k, tail) = r.reward;
    ++m;
    const bool flush = (r.what & TEAM_DONE) != 0;
    const int n_upd = flush ? m : (m == ns ? 1 : 0);
    const bool ok = (unsigned)r.next_idx < (unsigned)(DQL_N_CELLS / 3);
    if (!ok) mem.faults[0] += 1ull;  // never taken unless a bug: a plain (racy) count is enough to make the tests fail
    if (ok && n_upd > 0) {
      // 2. the row of s' as the tables stand now: after envs < k of this period, before this env's own writes; 3. both coins' bootstrap under the mask
      const QRow next = load_qrow((const double*)qa, (const double*)qb, r.next_idx);
      const double mask = (r.what & TEAM_MASK) ? 1.0 : 0.0;
      double ga = nstep_best(next, dbl, false) * mask, gb = nstep_best(next, dbl, true) * mask;
      // backward: both coins' chains through the rewards, newest first.  A flush leaves each entry's return (by its own coin) in the reward's place.
      for (int i = m - 1; i >= 0; --i) {
        const int s = nstep_slot(head, i, ns);
        const double ri = tw.val(k, s);
        ga = returns_step(ri, gamma, ga); gb = returns_step(ri, gamma, gb);
        if (flush) tw.val(k, s) = (tw.key(k, s) & NSTEP_COIN) ? gb : ga;
      }
      // forward: the updates, oldest first, each on the count and the value that stand at its moment
      for (int i = 0; i < n_upd; ++i) {
        const int s = nstep_slot(head, i, ns);
        const uint16_t key = tw.key(k, s);
        const bool sel_b = (key & NSTEP_COIN) != 0;  // (never set under B1/B2: StepOut::cell carries the coin under Double Q-learning only)
        const int sa = key & (NSTEP_COIN - 1);
        const double g = flush ? tw.val(k, s) : (sel_b ? gb : ga);
        if (sa < DQL_N_CELLS) {
          const double cnt = count[sa];
          const double alpha = nstep_alpha(sc, cnt);
          count[sa] = cnt + 1.0;
          double* qsel = sel_b ? qb : qa;
          const double q = qsel[sa];
          const double loss = alpha * (g - q);
          qsel[sa] = q + loss;
        } else {
          mem.faults[0] += 1ull;  // never taken unless a bug
        }
      }
    }
    // 4. what was updated (or dropped with its fault counted) leaves the window
    if (flush) { head = 0; m = 0; }
    else if (n_upd > 0) { head = nstep_slot(head, 1, ns); --m; }
    tw.head(k) = head; tw.len(k) = m;
    if (r.what & TEAM_DONE) {  // team_apply's bookkeeping, unchanged
      const int code = (r.what >> 8) & 0xff;
      const int won = code == DQL_TERMINAL_SUCCESS ? 1 : 0;
      ++t.episodes; t.successes += won;
      if ((unsigned)code < (unsigned)DQL_N_CHECK_CODES) mem.by_code[(long long)code * mem.n + l] += 1ull;
      if (t.log_n < mem.log_cap) { mem.log_code[l * mem.log_cap + t.log_n] = (uint8_t)code; mem.log_len[l * mem.log_cap + t.log_n] = (uint16_t)r.step_count; }
      ++t.log_n;
      if (!decided) {
        const int pos = t.lvl_eps % sc.window;
        const unsigned long long bit = 1ull << (pos & 63);
        unsigned long long w = pos >= 64 ? t.w1 : t.w0;
        t.win_count += won - ((w & bit) ? 1 : 0);
        w = won ? (w | bit) : (w & ~bit);
        if (pos >= 64) t.w1 = w; else t.w0 = w;
        ++t.lvl_eps;
        if (t.win_count >= sc.min_successes) { t.promoted = t.lvl_eps; decided = true; }
        else if (t.lvl_eps >= sc.max_episodes) decided = true;
      }
    }
  }
  if (decided) t.live = false;
  t.eps_thr = sc.eps_tab[t.lvl_eps < sc.n_eps ? t.lvl_eps : sc.n_eps - 1];
}

// The persistent windows of env g (TMem: an NstepMem over n_envs columns) into the launch's working copy, and back.  slot(i) / head / len: the env's own
// column of the working copy.  A window that persists is never full: the period that fills it takes its oldest entry out.
template <typename TMem, typename TWin>
DQL_DEV void team_window_load(const TMem& tm, long long n_envs, long long g, int k, int nstep, TWin tw) {
  const int ns = nstep < 1 ? 1 : (nstep > NSTEP_MAX ? NSTEP_MAX : nstep);
  int m = tm.len[g];
  m = m < 0 ? 0 : (m > ns - 1 ? ns - 1 : m);
  for (int i = 0; i < ns; ++i)
    if (i < m) { tw.key(k, i) = tm.key[(long long)i * n_envs + g]; tw.val(k, i) = tm.val[(long long)i * n_envs + g]; }
  tw.head(k) = 0; tw.len(k) = m;
}
template <typename TMem, typename TWin>
DQL_DEV void team_window_store(const TMem& tm, long long n_envs, long long g, int k, int nstep, TWin tw) {
  const int ns = nstep < 1 ? 1 : (nstep > NSTEP_MAX ? NSTEP_MAX : nstep);
  int head = tw.head(k), m = tw.len(k);
  head = (unsigned)head < (unsigned)ns ? head : 0;
  m = m < 0 ? 0 : (m > ns - 1 ? ns - 1 : m);
  tm.len[g] = m;
  for (int i = 0; i < ns; ++i)
    if (i < m) {
      const int s = nstep_slot(head, i, ns);
      tm.key[(long long)i * n_envs + g] = tw.key(k, s); tm.val[(long long)i * n_envs + g] = tw.val(k, s);
    }
}

}  // namespace dql
