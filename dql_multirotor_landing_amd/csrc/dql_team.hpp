// dql_team.hpp — a sequential Double-Q learner that owns a TEAM of E envs (E in {1, 2, 4, 8, 16, 32, 64}): its own three tables as in dql_learner.hpp, and
// the reference's update applied to the E transitions of every agent period one after the other, in env order.
//
// Learner l owns envs g = l E .. l E + E - 1 of a context made with dql_create(cfg, device, L E, seed, 0) (the state arrays have that context's layout, the
// Philox key of env g is (g, seed)) and the slices [l][DQL_N_CELLS] of Q_table_a, Q_table_b and state_action_counter.  One agent period is two parts:
//
//   team_env_period   per env (one lane each): the greedy row of the env's state is READ FROM THE TABLES, which hold every update of the period before —
//                     a row carried in registers would miss what a team-mate wrote —, then agent_period<TICK, XMODE> in MODE_TRAIN, then the transition
//                     as a TeamRecord.  The tables are only read here.
//   team_apply        per team (one lane): the E records in env order through learner_update (dql_learner.hpp, unchanged).  The row of s' is read from the
//                     tables as they stand at that moment, so after the updates of envs < e of this period; then the episode's end in the learner's books
//                     (LearnerBooks of dql_learner.hpp, which this file only uses: team_episode), except that a level once decided in a period takes no
//                     further outcome into its ring in that period (totals and log only).
//
// With E = 1 the two parts are learner_periods operation for operation: its carried row patched with q_new is the row of the updated tables.
//
// Between the two parts the records cross lanes, and the tables written by the applying lane are read by its team-mates in the next period.  That exchange
// and the ordering live in team_wave (dql_team_nstep.hpp: what k_learn_team and k_learn_team_nstep run below their declarations), not here: the host
// emulation (tests/host_emu/team_emu.cpp) calls the two parts for one lane after the other, where program order does both.  On the device a team is E
// consecutive lanes of a one-wave workgroup, and team_wave puts a __syncthreads() between the parts and another after team_apply.  __syncthreads() is a workgroup-scope release fence, the barrier, and a workgroup-scope
// acquire fence.  The release makes the applying lane's wave wait for its stores (s_waitcnt vmcnt(0): they have reached the CU's write-through vector L1 and
// the L2 behind it), the acquire keeps every later load behind it; writer and readers are lanes of ONE wave, hence of one CU and one vector L1, which is the
// situation workgroup scope is defined for.  No other workgroup ever touches a learner's slices during a launch, so no wider scope is needed.  The records
// travel through LDS under the same two barriers.
//
// The loop of team_wave runs n_periods <= LEARN_MAX_PERIODS times at most on every path.  Include after dql_learner.hpp.
#pragma once
#include "dql_learner.hpp"

namespace dql {

constexpr int TEAM_MAX_ENVS = 64;
constexpr bool team_size_ok(long long e) { return e == 1 || e == 2 || e == 4 || e == 8 || e == 16 || e == 32 || e == 64; }

// what one env hands to its team's applying lane after a period
enum { TEAM_DECISION = 1, TEAM_DONE = 2, TEAM_MASK = 4 };
struct TeamRecord {
  double reward;    // e.reward as a double
  int cell;         // StepOut::cell: coin * DQL_N_CELLS + s * 3 + action
  int next_idx;     // the state the period ended in
  int what;         // TEAM_DECISION | TEAM_DONE | TEAM_MASK | terminal code << 8
  int step_count;   // the episode's length so far (logged when it ended)
};

// A team's name for its learner's books (dql_learner.hpp) while the applying lane holds them in registers: the wave body and the host emulations of the team
// kernels load and store them under these names.  Nothing of the books is stated here.
using TeamState = LearnerBooks;
DQL_DEV TeamState team_load(const LearnSched& sc, const LearnMem& mem, long long l) { return books_load(sc, mem, l); }
DQL_DEV void team_store(const TeamState& t, const LearnMem& mem, long long l) { books_store(t, mem, l); }
// what the applying lane of a team tells its team-mates about the period to come
struct TeamCtl { uint32_t eps_thr; int live; };

// One agent period of env g (the arguments are learner_periods').  qa / qb: the learner's slices, read only.  j: the period's index; mgr0 / sched: its tick schedule.
template <int TICK, int XMODE, typename T>
DQL_DEV TeamRecord team_env_period(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr, Env<T>& e,
                                   const double* qa, const double* qb, uint32_t eps_thr, uint64_t seed, long long g, long long j, long long mgr0, int sched,
                                   const uint32_t* kv) {
  // the row of the state the env is in, from the tables as they stand after every update of the period before (a reset period does not use it)
  const QRow qx = load_qrow(qa, qb, e.idx_x < 0 ? 0 : e.idx_x);
  const int prev_p = e.bin_p;
  const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, qa, qb, MODE_TRAIN, eps_thr, 2, seed, (uint32_t)g, j, mgr0, sched, kv);
  // (o.next was read before this period's updates: team_apply reads the row again when the record's turn comes)
  const int mask = (c.quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) ? (prev_p != e.bin_p) : !o.done;
  TeamRecord r;
  r.reward = (double)e.reward; r.cell = o.cell; r.next_idx = e.idx_x; r.step_count = e.step_count;
  r.what = (o.decision ? TEAM_DECISION : 0) | (o.done ? TEAM_DONE : 0) | (mask ? TEAM_MASK : 0) | ((e.code & 0xff) << 8);
  return r;
}

// The end of the episode record r reports, in the learner's books (dql_learner.hpp): the totals and the log always, the outcome into the ring only while the
// level is undecided in this period — an episode a team-mate finishes after the decision counts in the totals and the log only.
DQL_DEV void team_episode(const LearnSched& sc, const LearnMem& mem, long long l, const TeamRecord& r, LearnerBooks& t, bool& decided) {
  const int won = books_episode(t, mem, l, (r.what >> 8) & 0xff, r.step_count);
  if (!decided) decided = books_ring_push(t, sc, won);
}

// The serial section: the E records of learner l's period in env order, on the learner's own pointers (one thread's program order).  t.eps_thr leaves as the
// next period's threshold; t.live leaves false when the level was decided in this period — after ALL E updates.
template <typename RecPtr>
DQL_DEV void team_apply(const LearnSched& sc, const LearnMem& mem, uint32_t quirks, double gamma, long long l, RecPtr rec, int n_envs, LearnerBooks& t) {
  double* qa = mem.qa + l * DQL_N_CELLS;
  double* qb = mem.qb + l * DQL_N_CELLS;
  double* count = mem.count + l * DQL_N_CELLS;
  const int ne = n_envs < TEAM_MAX_ENVS ? n_envs : TEAM_MAX_ENVS;
  bool decided = false;
  for (int k = 0; k < ne; ++k) {
    const TeamRecord r = rec[k];
    if (!(r.what & TEAM_DECISION)) continue;
    ++t.decisions;
    const bool coin = r.cell >= DQL_N_CELLS;
    const int sa = coin ? r.cell - DQL_N_CELLS : r.cell;
    bool ok = (unsigned)r.next_idx < (unsigned)(DQL_N_CELLS / 3);
    if (ok) {
      const QRow next = load_qrow((const double*)qa, (const double*)qb, r.next_idx);  // as the tables stand now: after envs < k of this period
      double q_new; bool sel_b;
      ok = learner_update(qa, qb, count, sc, quirks, gamma, sa, coin, next, r.reward, (r.what & TEAM_MASK) ? 1 : 0, q_new, sel_b);
    }
    if (!ok) mem.faults[0] += 1ull;  // never taken unless a bug: a plain (racy) count is enough to make the tests fail
    if (r.what & TEAM_DONE) team_episode(sc, mem, l, r, t, decided);
  }
  if (decided) t.live = false;
  t.eps_thr = eps_of_episode(sc, t.lvl_eps);
}

}  // namespace dql
