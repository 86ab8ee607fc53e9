// recipes_emu.cpp — dql_ensemble_run with recipes installed, emulated on the CPU from the real device source: dql_recipes.hpp's
// build_worklist_recipes and advance_learner_recipe on top of dql_learner.hpp's learner_periods.
//
// The driver does what ens_run_advancing (dql_ensemble.inc) does for ens_run_recipes (dql_recipes.inc), through emu_learners.h's RecipeRun: at an advance point
// every learner takes advance_learner_recipe's step (k_ens_advance_recipes: one thread per learner); then the live learners are regrouped by (recipe, level)
// and flown wave by wave, lane by lane, as k_learn_recipes flies them — the wave's recipe and level from wave_recipe[w] and wave_level[w], the lane's learner
// from the worklist (-1: an inactive lane), SimK::working and SimK::quirks, the MdpK of (recipe, level), the recipe's learning rates and the level's schedules
// from those.  A lane runs alone: __ballot(p) is p (host_shim.h).  Every array is exactly as long as the library allocates it, so the sanitized build sees any
// access beyond them.  What stands here is the wave, and mode 1.
//
//   recipes_emu JOB OUT   run the job (emu::RecipeJob; tests/test_recipes_host_emulation.py writes it), write OUT.  A job is either a run of the ensemble or one
//                         call of build_worklist_recipes on given arrays (mode 1), whose outputs are written as they are.
#include "host_shim.h"

#include "emu_learners.h"

using namespace dql;

namespace {

// one call of build_worklist_recipes: the arrays as long as the capacity says, written whole (slots beyond the returned waves stay at the fill value -2)
int worklist_only(emu::RecipeJob& j, const char* out_path) {
  const size_t slots = (size_t)j.cap_slots, waves = slots / ADV_WAVE;
  std::vector<int> worklist(slots, -2), wave_recipe(waves, -2), wave_level(waves, -2);
  unsigned long long faults = 0ull;
  const long long n_waves = build_worklist_recipes(j.frozen.data(), j.level.data(), j.recipe_of.data(), j.n, j.n_recipes, worklist.data(), wave_recipe.data(), wave_level.data(),
                                                   j.cap_slots, &faults);
  const long long fl = (long long)faults, want = (j.n_recipes >= 1 && j.n_recipes <= RCP_MAX) ? worklist_capacity_recipes(j.n, j.n_recipes) : 0;
  emu::ResultFile f(out_path);
  f.put(&n_waves, 1); f.put(&fl, 1); f.put(&want, 1); f.put(worklist); f.put(wave_recipe); f.put(wave_level);
  return f.close();
}

template <typename T> int launch(emu::RecipeJob& j, const char* out_path) {
  emu::RecipeRun<T> run(j);
  emu::LearnerState<T>& st = run.st;
  run.fly([&](int w, long long j0, int np, const long long* mgr0, const int* sched) {
    const int r = run.wave_recipe[(size_t)w], lvl = run.wave_level[(size_t)w];
    if ((unsigned)r >= (unsigned)j.n_recipes || (unsigned)lvl >= (unsigned)ADV_MAX_LEVELS) { st.faults[0] += 1ull; return; }
    const RecipeSched& rs = run.tab.rs[(size_t)r];
    const SimK<T> cl = run.k.simk(lvl, rs.quirks);
    const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
    const LearnSched sc = learn_sched(rs.alpha_tab, rs.n_alpha, rs.alpha_min, (const LevelSched DQL_CONST_AS*)&rs.lv[lvl]);
    const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&run.tab.mdpk[(size_t)r * ADV_MAX_LEVELS + (size_t)lvl];
    for (int lane = 0; lane < ADV_WAVE; ++lane) {
      const long long l = run.worklist[(size_t)w * ADV_WAVE + (size_t)lane];
      learner_periods<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, run.k.mdp_run, sc, run.mem, st.sr.data(), st.si.data(), j.seed, l, l >= 0 && l < j.n, j0, np, mgr0, sched, lc.kv);
    }
  });
  return run.write(out_path);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: recipes_emu JOB OUT\n"); return 2; }
  emu::RecipeJob j(argv[1], true);
  if (j.mode == 1) return worklist_only(j, argv[2]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
