// dql_advance.hpp — per-learner curriculum levels for the sequential learners: the worklist that regroups the live learners by
// level between launches, and the step a frozen learner takes from its finished level to the next.
//
// Everything level-dependent in agent_period is wave-uniform (SimK::working is pinned to an SGPR, MdpK is read with scalar loads), so a learner's level is
// never a lane's property: build_worklist lays the live learners out so that every wave of k_learn_levels (dql_ensemble.inc) holds learners of ONE level, and
// advance_learner moves a learner to the next level between launches.  learner_periods (dql_learner.hpp) is what flies them, unchanged.
//
// Both are plain functions that also compile as host C++ (tests/host_emu/advance_emu.cpp).  Every loop is bounded by an argument on every path, every
// index is range-checked, and a violation is counted into the ensemble's `faults` word and otherwise skipped (a plain, racy add on the device, as in
// dql_learner.hpp: whether the word is zero is what counts, not the count).
// Include after dql_learner.hpp.
#pragma once
#include "dql_learner.hpp"

namespace dql {

constexpr int ADV_MAX_LEVELS = 5, ADV_MAX_EVERY = 4096, ADV_WAVE = 64;

// what dql_ensemble_set_level_schedules installs for one level (wave-uniform; the learning-rate table stays the ensemble's)
struct LevelSched {
  const uint32_t* eps_tab; int n_eps;
  int window, min_successes, max_episodes;
};
// what a wave on one level flies by: the learning rates (the ensemble's, or a recipe's) with the level's exploration table and freeze rules
DQL_DEV LearnSched learn_sched(const double* alpha_tab, int n_alpha, double alpha_min, const LevelSched DQL_CONST_AS* lv) {
  return LearnSched{alpha_tab, n_alpha, alpha_min, lv->eps_tab, lv->n_eps, lv->window, lv->min_successes, lv->max_episodes};
}

// per-learner curriculum state, indexed by the learner l in [0, n); the history by [level][l]
struct AdvanceMem {
  int* level;                  // [n] the learner's working level
  int* promoted_at;            // [5][n] episode (count at that level) at which the learner promoted at level k, or -1
  int* episodes_at;            // [5][n] episodes spent at level k
  long long* entered_period;   // [5][n] the ensemble's period index at which the learner entered level k, or -1
};
struct AdvanceRule {
  double ratios[ADV_MAX_LEVELS];  // transfer ratio of the finished level k
  int last_level, advance_exhausted;
};

// Slots a worklist of n learners needs at most: every level's segment is padded to whole waves.
inline long long worklist_capacity(long long n) { return ((n + ADV_WAVE - 1) / ADV_WAVE + ADV_MAX_LEVELS) * ADV_WAVE; }

// The live learners (frozen[l] == 0) grouped by level, levels ascending, learners ascending within a level; each level's segment is padded to a multiple of
// 64 with -1, so wave w = worklist[64 w .. 64 w + 63] holds learners of wave_level[w] only.  -> the number of waves (0: nobody to fly).  A learner whose
// level is out of range is counted in *faults and left out; so is one the capacity has no room for.
inline int build_worklist(const int* frozen, const int* level, long long n, int* worklist, int* wave_level, long long cap_slots, unsigned long long* faults) {
  long long at = 0;
  for (long long l = 0; l < n; ++l)
    if (!frozen[l] && (unsigned)level[l] >= (unsigned)ADV_MAX_LEVELS) *faults += 1ull;
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) {
    for (long long l = 0; l < n; ++l) {
      if (frozen[l] || level[l] != k) continue;
      if (at >= cap_slots) { *faults += 1ull; continue; }
      if (at % ADV_WAVE == 0) wave_level[at / ADV_WAVE] = k;
      worklist[at++] = (int)l;
    }
    while (at % ADV_WAVE != 0 && at < cap_slots) worklist[at++] = -1;
  }
  return (int)(at / ADV_WAVE);
}

// finished for good: frozen at the last level, or out of episodes where those do not advance
inline bool learner_finished(int frozen, int level, int promoted, const AdvanceRule& r) {
  return frozen && (level >= r.last_level || (promoted < 0 && !r.advance_exhausted));
}

// Learner l at an advance point (period index j, before period j is flown).  A frozen learner below the last level that promoted — or ran out of episodes,
// where the rule lets those advance — records its history entry, applies transfer_learning of its finished level k to ITS OWN two tables (Q[k] = Q[k-1] *
// ratios[k]; k = 0 wraps to the last level, B6: k_ens_transfer's arithmetic), moves to level k + 1, marks its env for reset (k_mark_reset) and clears its
// per-level counters, window ring, promotion record and frozen flag (ens_rearm).  n_cells <= DQL_CELLS_PER_LEVEL bounds the transfer loop.
// -> true when the learner advanced.
DQL_DEV bool advance_learner(const LearnMem& mem, const AdvanceMem& adv, const AdvanceRule& rule, int4* si, long long l, long long j, int n_cells) {
  if (l < 0 || l >= mem.n) { mem.faults[0] += 1ull; return false; }
  if (!mem.frozen[l]) return false;
  const int k = adv.level[l];
  if ((unsigned)k >= (unsigned)ADV_MAX_LEVELS || (unsigned)rule.last_level >= (unsigned)ADV_MAX_LEVELS) { mem.faults[0] += 1ull; return false; }
  if (k >= rule.last_level) return false;
  const int promoted = mem.promoted[l];
  if (promoted < 0 && !rule.advance_exhausted) return false;
  adv.promoted_at[(long long)k * mem.n + l] = promoted;
  adv.episodes_at[(long long)k * mem.n + l] = mem.level_episodes[l];
  const int src = (k + ADV_MAX_LEVELS - 1) % ADV_MAX_LEVELS;
  const double ratio = rule.ratios[k];
  double* qa = mem.qa + l * DQL_N_CELLS;
  double* qb = mem.qb + l * DQL_N_CELLS;
  const int nc = n_cells < DQL_CELLS_PER_LEVEL ? n_cells : DQL_CELLS_PER_LEVEL;
  for (int i = 0; i < nc; ++i) {
    qa[k * DQL_CELLS_PER_LEVEL + i] = qa[src * DQL_CELLS_PER_LEVEL + i] * ratio;
    qb[k * DQL_CELLS_PER_LEVEL + i] = qb[src * DQL_CELLS_PER_LEVEL + i] * ratio;
  }
  adv.level[l] = k + 1;
  adv.entered_period[(long long)(k + 1) * mem.n + l] = j;
  int4 v = si[l];
  v.w |= (FL_DONE << 8);
  si[l] = v;
  mem.level_episodes[l] = 0; mem.win_count[l] = 0; mem.win_bits[l] = 0ull; mem.win_bits[mem.n + l] = 0ull; mem.promoted[l] = -1; mem.frozen[l] = 0;
  return true;
}

}  // namespace dql
