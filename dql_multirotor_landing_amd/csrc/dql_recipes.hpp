// dql_recipes.hpp — per-learner recipes for the sequential learners: every learner of an ensemble in curriculum mode belongs to one
// of up to 64 recipes (quirk word, learning rates, per-level exploration table and promotion rule, transfer ratios, last level, transfer order), the worklist
// that regroups the live learners by (recipe, level) between launches, and the step a frozen learner takes to its next level under its own recipe's rule.
//
// Everything recipe-dependent in agent_period and learner_periods is wave-uniform, as everything level-dependent is (dql_advance.hpp): a learner's recipe is
// never a lane's property.  build_worklist_recipes lays the live learners out so that every wave of k_learn_recipes (dql_recipes.inc) holds learners of ONE
// recipe on ONE level; learner_periods (dql_learner.hpp) flies them, unchanged, and advance_learner (dql_advance.hpp) stays the reference's transfer order.
//
// Plain functions that also compile as host C++ (tests/host_emu/recipes_emu.cpp).  Every loop is bounded by an argument on every path, every index is
// range-checked, and a violation is counted into the ensemble's `faults` word and otherwise skipped, as in dql_advance.hpp.
// Include after dql_advance.hpp.
#pragma once
#include "dql_advance.hpp"

namespace dql {

constexpr int RCP_MAX = 64;
constexpr int RCP_ORDER_REFERENCE = 0, RCP_ORDER_PAPER = 1;

// what dql_ensemble_set_recipe installs for one recipe's advance points: AdvanceRule as it stands, and the order of transfer and level change.
//   order 0 (the reference's): leaving level k, Q[k] = Q[k-1] * ratios[k] with the k = 0 wrap (B6) — advance_learner itself;
//   order 1 (the paper's): the level-k block stays as learnt, Q[k+1] = Q[k] * ratios[k+1] on entering level k + 1, no wrap, ratios[0] unused.
struct RecipeRule {
  AdvanceRule rule;
  int transfer_order, pad_;
};
// what a wave of k_learn_recipes reads for its recipe (wave-uniform): the quirk word that replaces the config's in SimK, the learning rates, and LevelSched
// per level.  (The recipe's MdpK per level is a device array of its own, [R][5].)
struct RecipeSched {
  const double* alpha_tab; int n_alpha; uint32_t quirks; double alpha_min;
  LevelSched lv[ADV_MAX_LEVELS];
};

// Slots a worklist of n learners in n_recipes recipes needs at most: there are at most 5 R segments, each padded to whole waves, and
// sum ceil(c_i / 64) <= floor(n / 64) + (number of segments) when the c_i sum to at most n.
inline long long worklist_capacity_recipes(long long n, int n_recipes) { return (n / ADV_WAVE + (long long)ADV_MAX_LEVELS * n_recipes) * ADV_WAVE; }

// The live learners (frozen[l] == 0) grouped by (recipe, level): recipes ascending, then levels, then learners; every segment is padded to a multiple of 64
// with -1, so wave w = worklist[64 w .. 64 w + 63] holds learners of recipe wave_recipe[w] on level wave_level[w] only.  -> the number of waves (0: nobody
// to fly).  A live learner whose recipe or level is out of range is counted in *faults and left out; so is one the capacity has no room for.
// (A counting sort: one pass to count, one over the 5 R segments to place them, one to fill.)
inline int build_worklist_recipes(const int* frozen, const int* level, const int* recipe_of, long long n, int n_recipes, int* worklist, int* wave_recipe,
                                  int* wave_level, long long cap_slots, unsigned long long* faults) {
  if (n_recipes < 1 || n_recipes > RCP_MAX) { *faults += 1ull; return 0; }
  long long at_seg[RCP_MAX * ADV_MAX_LEVELS];
  const int n_seg = n_recipes * ADV_MAX_LEVELS;
  for (int s = 0; s < n_seg; ++s) at_seg[s] = 0;
  for (long long l = 0; l < n; ++l) {
    if (frozen[l]) continue;
    if ((unsigned)recipe_of[l] >= (unsigned)n_recipes || (unsigned)level[l] >= (unsigned)ADV_MAX_LEVELS) { *faults += 1ull; continue; }
    at_seg[recipe_of[l] * ADV_MAX_LEVELS + level[l]] += 1;
  }
  const long long cap = cap_slots - cap_slots % ADV_WAVE;  // whole waves only
  long long at = 0;
  for (int s = 0; s < n_seg; ++s) {  // the segment's count becomes its first slot; its slots start as padding, its waves get their recipe and level
    const long long slots = (at_seg[s] + ADV_WAVE - 1) / ADV_WAVE * ADV_WAVE;
    at_seg[s] = at;
    for (long long i = at; i < at + slots && i < cap; ++i) {
      worklist[i] = -1;
      if (i % ADV_WAVE == 0) { wave_recipe[i / ADV_WAVE] = s / ADV_MAX_LEVELS; wave_level[i / ADV_WAVE] = s % ADV_MAX_LEVELS; }
    }
    at += slots;
  }
  for (long long l = 0; l < n; ++l) {
    if (frozen[l] || (unsigned)recipe_of[l] >= (unsigned)n_recipes || (unsigned)level[l] >= (unsigned)ADV_MAX_LEVELS) continue;
    const long long i = at_seg[recipe_of[l] * ADV_MAX_LEVELS + level[l]]++;
    if (i >= cap) { *faults += 1ull; continue; }
    worklist[i] = (int)l;
  }
  return (int)((at < cap ? at : cap) / ADV_WAVE);
}

// Learner l at an advance point (period index j, before period j is flown) under the rule of ITS recipe.  Order 0 is advance_learner, called as it stands.
// Order 1: a frozen learner below its recipe's last level that promoted — or ran out of episodes, where the rule lets those advance — records its history
// entry, keeps its level-k block as learnt, gets Q[k+1] = Q[k] * ratios[k+1] in ITS OWN two tables, moves to level k + 1, marks its env for reset and clears
// its per-level counters, window ring, promotion record and frozen flag (DESIGN.md section 14's five steps).  n_cells <= DQL_CELLS_PER_LEVEL bounds the
// transfer loop.  -> true when the learner advanced.
DQL_DEV bool advance_learner_recipe(const LearnMem& mem, const AdvanceMem& adv, const RecipeRule* rules, int n_recipes, const int* recipe_of, int4* si, long long l,
                                    long long j, int n_cells) {
  if (l < 0 || l >= mem.n) { mem.faults[0] += 1ull; return false; }
  const int r = recipe_of[l];
  if ((unsigned)r >= (unsigned)n_recipes || n_recipes > RCP_MAX) { mem.faults[0] += 1ull; return false; }
  const RecipeRule& rr = rules[r];
  if (rr.transfer_order == RCP_ORDER_REFERENCE) return advance_learner(mem, adv, rr.rule, si, l, j, n_cells);
  if (rr.transfer_order != RCP_ORDER_PAPER) { mem.faults[0] += 1ull; return false; }
  const AdvanceRule& rule = rr.rule;
  if (!mem.frozen[l]) return false;
  const int k = adv.level[l];
  if ((unsigned)k >= (unsigned)ADV_MAX_LEVELS || (unsigned)rule.last_level >= (unsigned)ADV_MAX_LEVELS) { mem.faults[0] += 1ull; return false; }
  if (k >= rule.last_level) return false;  // (so k + 1 <= last_level <= 4)
  const int promoted = mem.promoted[l];
  if (promoted < 0 && !rule.advance_exhausted) return false;
  adv.promoted_at[(long long)k * mem.n + l] = promoted;
  adv.episodes_at[(long long)k * mem.n + l] = mem.level_episodes[l];
  const double ratio = rule.ratios[k + 1];
  double* qa = mem.qa + l * DQL_N_CELLS;
  double* qb = mem.qb + l * DQL_N_CELLS;
  const int nc = n_cells < DQL_CELLS_PER_LEVEL ? n_cells : DQL_CELLS_PER_LEVEL;
  for (int i = 0; i < nc; ++i) {
    qa[(k + 1) * DQL_CELLS_PER_LEVEL + i] = qa[k * DQL_CELLS_PER_LEVEL + i] * ratio;
    qb[(k + 1) * DQL_CELLS_PER_LEVEL + i] = qb[k * DQL_CELLS_PER_LEVEL + i] * ratio;
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
