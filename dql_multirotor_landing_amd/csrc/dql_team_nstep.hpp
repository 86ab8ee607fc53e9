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
// One update is dql_nstep.hpp's nstep_update itself: sel_b = Double Q-learning and the ENTRY's own coin; best = learner_best on the row of step 2;
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
// On the device the windows travel under the two workgroup barriers of a team's period (dql_team.hpp): a lane writes its env's window into LDS before
// the launch's first barrier, only the applying lane touches the team's windows between the barriers, and every lane reads its own column back after the
// last one.  LDS of one workgroup under __syncthreads() needs no more than that.
//
// This file also owns team_wave, the one wave body of BOTH team kernels (it needs both apply functions): the lane's role, the state load, the period loop with
// its two barriers, the store; the windows are a template parameter, an empty type for the one-step kernel, so that its three window statements drop out.
//
// Every loop is bounded by E or by n on every path.  Include after dql_team.hpp and dql_nstep.hpp.
#pragma once
#include <type_traits>

#include "dql_team.hpp"
#include "dql_nstep.hpp"

namespace dql {

template <typename RecPtr, typename TWin>
DQL_DEV void team_apply_nstep(const LearnSched& sc, const LearnMem& mem, uint32_t quirks, double gamma, long long l, RecPtr rec, int n_envs, int nstep, TWin tw,
                              LearnerBooks& t) {
  double* qa = mem.qa + l * DQL_N_CELLS;
  double* qb = mem.qb + l * DQL_N_CELLS;
  double* count = mem.count + l * DQL_N_CELLS;
  const int ne = n_envs < TEAM_MAX_ENVS ? n_envs : TEAM_MAX_ENVS;
  const int ns = nstep_clamp(nstep);
  const bool dbl = !(quirks & DQL_Q_UPDATE_TABLE_A_ONLY);
  bool decided = false;
  for (int k = 0; k < ne; ++k) {
    const TeamRecord r = rec[k];
    if (!(r.what & TEAM_DECISION)) continue;
    ++t.decisions;
    const bool coin = r.cell >= DQL_N_CELLS;
    const int sa_new = coin ? r.cell - DQL_N_CELLS : r.cell;
    // 1. the decision's entry (m < ns here: a full window gave up its oldest entry in the period that filled it)
    int head = nstep_head(tw.head(k), ns), m = nstep_len(tw.len(k), ns);
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
      double ga = learner_best(next, dbl, false) * mask, gb = learner_best(next, dbl, true) * mask;
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
        const double g = flush ? tw.val(k, s) : (nstep_coin(key) ? gb : ga);
        double q_new; bool sel_b;  // (no carried row to patch: team_env_period reads the row from the tables)
        if (!nstep_update(qa, qb, count, sc, key, g, q_new, sel_b)) mem.faults[0] += 1ull;  // never taken unless a bug
      }
    }
    // 4. what was updated (or dropped with its fault counted) leaves the window
    if (flush) { head = 0; m = 0; }
    else if (n_upd > 0) { head = nstep_slot(head, 1, ns); --m; }
    tw.head(k) = head; tw.len(k) = m;
    if (r.what & TEAM_DONE) team_episode(sc, mem, l, r, t, decided);  // team_apply's
  }
  if (decided) t.live = false;
  t.eps_thr = eps_of_episode(sc, t.lvl_eps);
}

// The persistent windows of env g (TMem: an NstepMem over n_envs columns) into the launch's working copy, and back: dql_nstep.hpp's window_load /
// window_store on env k's column of the team's windows, whose head and length live in the working copy too.
template <typename TWin> struct TeamColumn {
  TWin tw; int k;
  DQL_DEV uint16_t& key(int slot) const { return tw.key(k, slot); }
  DQL_DEV double& val(int slot) const { return tw.val(k, slot); }
};
template <typename TMem, typename TWin>
DQL_DEV void team_window_load(const TMem& tm, long long n_envs, long long g, int k, int nstep, TWin tw) {
  const int ns = nstep_clamp(nstep), m = nstep_len(tm.len[g], ns);
  window_load(tm, n_envs, g, ns, m, TeamColumn<TWin>{tw, k});
  tw.head(k) = 0; tw.len(k) = m;
}
template <typename TMem, typename TWin>
DQL_DEV void team_window_store(const TMem& tm, long long n_envs, long long g, int k, int nstep, TWin tw) {
  const int ns = nstep_clamp(nstep), m = nstep_len(tw.len(k), ns);
  tm.len[g] = m;
  window_store(tm, n_envs, g, ns, TeamColumn<TWin>{tw, k}, nstep_head(tw.head(k), ns), m);
}

// ---- one team wave: what k_learn_team (dql_teams.inc) and k_learn_team_nstep (dql_team_nstep.inc) run below their declarations ----
// The kernel's view of the team windows in LDS: key / val [slot][lane], head / len [lane]; the pointers name column 0 of the view (a team's first lane, or a
// lane's own column), env e of it is column e.
struct LdsTeamWindow {
  uint16_t* k; double* v; int* h; int* n;
  DQL_DEV uint16_t& key(int e, int slot) const { return k[slot * 64 + e]; }
  DQL_DEV double& val(int e, int slot) const { return v[slot * 64 + e]; }
  DQL_DEV int& head(int e) const { return h[e]; }
  DQL_DEV int& len(int e) const { return n[e]; }
};
// team_wave's windows: none (k_learn_team), or this lane's own column of the wave's LDS windows, where they persist, and n
struct NoTeamWindows {};
template <typename TMem> struct TeamWindows { LdsTeamWindow mine; TMem tm; int nstep; };

// which env and which team a lane of a team wave flies (active: one at all), as the kernel's lane map says
struct TeamLane { long long g, l; bool active; };

#ifdef __HIPCC__  // the barriers have no host restatement: the emulations call the two parts for one lane after the other (dql_team.hpp)
// Workgroups of one wave; a team is E consecutive lanes, so no team straddles waves.  Which env g and team l a lane flies, and whether it flies one at all
// (active), is the caller's: the identity map g = 64 blockIdx.x + tid of k_learn_team and k_learn_team_nstep, whose last wave may hold fewer teams, or the
// worklist's of k_learn_team_levels and k_learn_team_levels_nstep (dql_team_levels.inc), in whose waves a slot of E lanes may be empty.  So are the schedules sc
// and the MdpK the wave flies by (the ensemble's, or its level's).  Lane tid is env tid & (E - 1) of its team under every map.  Per period: every
// live lane flies its env and leaves its record in LDS; barrier; the first lane of every live team applies the team's E records in order and publishes the next
// period's threshold and whether the team flies on; barrier.  All teams of a wave run side by side.  The wave leaves when every team in it is frozen.
// With windows a lane loads its env's window before the first barrier of the launch and stores it beside store_env, after the last; in between only the team's
// applying lane touches the team's columns, between the two barriers of a period.  The windows of a team frozen at the launch's start are neither loaded nor stored.
// t: the kernel's TeamArgs; cl / cfgk / tc / kv: its wave prologue's; sRec / sCtl: [64] in LDS; lane / sc / mdp: the kernel's lane map, schedules and MdpK.
template <int XMODE, int TICK, typename T, typename TArgs, typename Wins>
DQL_DEV void team_wave(const TArgs& t, const SimK<T>& cl, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const uint32_t* kv, int tid, TeamRecord* sRec,
                       TeamCtl* sCtl, const Wins& w, const TeamLane& lane, const LearnSched& sc, const MdpK<T> DQL_CONST_AS* mdp) {
  constexpr bool windows = !std::is_same_v<Wins, NoTeamWindows>;
  const auto& a = t.a;
  const bool active = lane.active;
  const long long g = active ? lane.g : 0;  // < t.n_envs
  const long long l = active ? lane.l : 0;  // < a.mem.n
  const int lead = tid & ~(t.envs_per_learner - 1);      // the team's first lane: the one that applies
  const double* qa = a.mem.qa + l * DQL_N_CELLS;
  const double* qb = a.mem.qb + l * DQL_N_CELLS;
  const bool applies = active && tid == lead;
  TeamState ts = TeamState{};
  if (applies) ts = team_load(sc, a.mem, l);
  bool live = active && a.mem.frozen[l] == 0;
  uint32_t eps_thr = live ? eps_of_episode(sc, a.mem.level_episodes[l]) : 0u;
  const bool loaded = live;
  Env<T> e = Env<T>{};
  if constexpr (windows) { w.mine.head(0) = 0; w.mine.len(0) = 0; }
  if (live) {
    load_env(e, a.sr, a.si[g], t.n_envs, g, cl);
    if constexpr (windows) team_window_load(w.tm, t.n_envs, g, 0, w.nstep, w.mine);  // read by the applying lane behind the period's first barrier
  }
  const int np = a.n_periods < LEARN_MAX_PERIODS ? a.n_periods : LEARN_MAX_PERIODS;
  for (int p = 0; p < np; ++p) {
    TeamRecord r{0.0, -1, 0, 0, 0};
    if (live) r = team_env_period<TICK, XMODE>(cl, cfgk, tc, mdp, a.mdp_run, e, qa, qb, eps_thr, a.seed, g, a.j0 + p, a.mgr0[p], a.tick_sched[p], kv);
    sRec[tid] = r;
    __syncthreads();  // the records (and, in the first period, the windows) are in LDS; every row load of this period lies before the first table write of it
    if (applies && live) {
      if constexpr (windows) team_apply_nstep(sc, a.mem, cl.quirks, a.mdp_run.gamma, l, &sRec[tid], t.envs_per_learner, w.nstep, w.mine, ts);  // `mine` of the first lane: the team's columns
      else team_apply(sc, a.mem, cl.quirks, a.mdp_run.gamma, l, &sRec[tid], t.envs_per_learner, ts);
      sCtl[tid] = TeamCtl{ts.eps_thr, ts.live ? 1 : 0};
    }
    __syncthreads();  // workgroup-scope release of the applying lanes' table stores and window writes, acquire in front of the next period's row loads (dql_team.hpp)
    if (live) { const TeamCtl ctl = sCtl[lead]; eps_thr = ctl.eps_thr; live = ctl.live != 0; }
    if (__ballot(live) == 0ull) break;
  }
  if (loaded) {
    store_env(e, a.sr, a.si, t.n_envs, g, cl);
    if constexpr (windows) team_window_store(w.tm, t.n_envs, g, 0, w.nstep, w.mine);  // behind the last period's second barrier
  }
  if (applies && loaded) team_store(ts, a.mem, l);
}
#endif

}  // namespace dql
