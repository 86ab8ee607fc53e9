// dql_team_levels.hpp — per-team curriculum levels for the team learners: dql_advance.hpp's two pieces for learners that own E envs.
// The worklist regroups the live TEAMS by level between launches, a wave holding 64 / E team slots, and advance_team is the step a frozen team takes from
// its finished level to the next.
//
// A team is E consecutive lanes of a one-wave workgroup (dql_team.hpp), so a slot of the worklist names a team, not a lane: wave w of k_learn_team_levels
// (dql_team_levels.inc) holds the teams worklist[w tpw .. w tpw + tpw - 1], tpw = 64 / E, all on level wave_level[w].  The level stays a wave's property,
// never a lane's (dql_advance.hpp).  team_wave (dql_team_nstep.hpp) is what flies them, with its lane map handed in.
//
// Both are plain functions that also compile as host C++ (tests/host_emu/team_levels_emu.cpp).  Every loop is bounded by an argument on every path, every
// index is range-checked, and a violation is counted into the ensemble's `faults` word and otherwise skipped, as in dql_advance.hpp.
// Include after dql_advance.hpp, dql_recipes.hpp (the two transfer orders' names) and dql_team.hpp.
#pragma once
#include "dql_advance.hpp"
#include "dql_recipes.hpp"
#include "dql_team.hpp"

namespace dql {

// Team slots a worklist of n teams needs at most: at most five segments, each padded to whole waves of teams_per_wave slots, and
// sum ceil(c_k / tpw) <= ceil(n / tpw) + 5 when the c_k sum to at most n (dql_advance.hpp's argument, a wave being tpw slots).
inline long long team_worklist_capacity(long long n, int teams_per_wave) {
  return ((n + teams_per_wave - 1) / teams_per_wave + ADV_MAX_LEVELS) * teams_per_wave;
}

// The live teams (frozen[l] == 0) grouped by level, levels ascending, teams ascending within a level; each level's segment is padded with -1 to a multiple
// of teams_per_wave (64 / E: one of 64, 32, 16, 8, 4, 2, 1), so wave w = worklist[w tpw .. w tpw + tpw - 1] holds teams of wave_level[w] only.  -> the number of
// waves (0: nobody to fly).  A team whose level is out of range is counted in *faults and left out; so is one the capacity (whole waves of it) has no room for.
// With teams_per_wave = 64 this is build_worklist, slot for slot.
inline int build_team_worklist(const int* frozen, const int* level, long long n_teams, int teams_per_wave, int* worklist, int* wave_level, long long cap_slots,
                               unsigned long long* faults) {
  if (!team_size_ok(teams_per_wave)) { *faults += 1ull; return 0; }
  const long long tpw = teams_per_wave, cap = cap_slots - cap_slots % tpw;
  long long at = 0;
  for (long long l = 0; l < n_teams; ++l)
    if (!frozen[l] && (unsigned)level[l] >= (unsigned)ADV_MAX_LEVELS) *faults += 1ull;
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) {
    for (long long l = 0; l < n_teams; ++l) {
      if (frozen[l] || level[l] != k) continue;
      if (at >= cap) { *faults += 1ull; continue; }
      if (at % tpw == 0) wave_level[at / tpw] = k;
      worklist[at++] = (int)l;
    }
    while (at % tpw != 0 && at < cap) worklist[at++] = -1;
  }
  return (int)(at / tpw);
}

// Team l at an advance point (period index j, before period j is flown): advance_learner's step (dql_advance.hpp) for a learner that owns the envs
// l E .. l E + E - 1.  The decision and the history entry are advance_learner's.  transfer_order RCP_ORDER_REFERENCE is its transfer, Q[k] = Q[k-1] * ratios[k]
// with the k = 0 wrap; RCP_ORDER_PAPER is advance_learner_recipe's paper branch (dql_recipes.hpp), Q[k+1] = Q[k] * ratios[k+1], the level-k block kept, no
// wrap.  Then ALL E envs are marked for reset; where the ensemble has team windows (pending_len: [n E], else null) every one of those envs' pending lengths
// is set to 0 — a frozen team's windows are generally not empty (dql_team_nstep.hpp) and their entries belong to the episodes the reset abandons, which is
// what dql_ensemble_set_level does ensemble-wide —; then the per-level books, ring, promotion record and frozen flag are cleared.  si: [n E].
// n_cells <= DQL_CELLS_PER_LEVEL bounds the transfer loop, n_envs <= TEAM_MAX_ENVS the env loop.  -> true when the team advanced.
DQL_DEV bool advance_team(const LearnMem& mem, const AdvanceMem& adv, const AdvanceRule& rule, int transfer_order, int4* si, int* pending_len, int n_envs, long long l,
                          long long j, int n_cells) {
  if (l < 0 || l >= mem.n || !team_size_ok(n_envs) || (transfer_order != RCP_ORDER_REFERENCE && transfer_order != RCP_ORDER_PAPER)) { mem.faults[0] += 1ull; return false; }
  if (!mem.frozen[l]) return false;
  const int k = adv.level[l];
  if ((unsigned)k >= (unsigned)ADV_MAX_LEVELS || (unsigned)rule.last_level >= (unsigned)ADV_MAX_LEVELS) { mem.faults[0] += 1ull; return false; }
  if (k >= rule.last_level) return false;  // (so k + 1 <= last_level <= 4)
  const int promoted = mem.promoted[l];
  if (promoted < 0 && !rule.advance_exhausted) return false;
  adv.promoted_at[(long long)k * mem.n + l] = promoted;
  adv.episodes_at[(long long)k * mem.n + l] = mem.level_episodes[l];
  const bool paper = transfer_order == RCP_ORDER_PAPER;
  const int dst = paper ? k + 1 : k, src = paper ? k : (k + ADV_MAX_LEVELS - 1) % ADV_MAX_LEVELS;
  const double ratio = rule.ratios[dst];
  double* qa = mem.qa + l * DQL_N_CELLS;
  double* qb = mem.qb + l * DQL_N_CELLS;
  const int nc = n_cells < DQL_CELLS_PER_LEVEL ? n_cells : DQL_CELLS_PER_LEVEL;
  for (int i = 0; i < nc; ++i) {
    qa[dst * DQL_CELLS_PER_LEVEL + i] = qa[src * DQL_CELLS_PER_LEVEL + i] * ratio;
    qb[dst * DQL_CELLS_PER_LEVEL + i] = qb[src * DQL_CELLS_PER_LEVEL + i] * ratio;
  }
  adv.level[l] = k + 1;
  adv.entered_period[(long long)(k + 1) * mem.n + l] = j;
  for (int e = 0; e < n_envs; ++e) {
    const long long g = l * n_envs + e;
    int4 v = si[g];
    v.w |= (FL_DONE << 8);
    si[g] = v;
    if (pending_len) pending_len[g] = 0;
  }
  mem.level_episodes[l] = 0; mem.win_count[l] = 0; mem.win_bits[l] = 0ull; mem.win_bits[mem.n + l] = 0ull; mem.promoted[l] = -1; mem.frozen[l] = 0;
  return true;
}

}  // namespace dql
