// nstep_recipes_emu.cpp — dql_ensemble_run with recipes installed of which some have n-step targets, emulated on the CPU from the real
// device source: dql_recipes.hpp's build_worklist_recipes and advance_learner_recipe on top of dql_nstep.hpp's learner_periods_nstep and dql_learner.hpp's
// learner_periods.
//
// It does what ens_run_advancing (dql_ensemble.inc) does for ens_run_recipes (dql_recipes.inc), through emu_learners.h's RecipeRun: at an advance point every
// learner takes advance_learner_recipe's step; then the live learners are regrouped by (recipe, level) and flown wave by wave, lane by lane, as
// k_learn_recipes_nstep (dql_nstep_recipes.inc) flies them — the wave's recipe and level from wave_recipe[w] and wave_level[w], its n from
// recipe_nstep[recipe], the lane's learner from the worklist (-1: an inactive lane); a wave with n = 0 flies learner_periods, the others
// learner_periods_nstep.  A lane runs alone: __ballot(p) is p (host_shim.h).  The windows are reached through checked references (emu_learners.h): the wave's
// working copy stands for the kernel's LDS ([NSTEP_MAX][64], the lane's column) and is poisoned before every wave (keys 0xffff, rewards NaN), as LDS carries
// nothing from launch to launch; the persistent copy is [NSTEP_MAX][n] plus len[n], exactly as long as the library's, entries poisoned, lengths zeroed.  An
// index outside them ends the run with status 3.  Every other array is exactly as long as the library allocates it, so the sanitized build sees any access
// beyond them.  What stands here is the wave.
//
//   nstep_recipes_emu JOB OUT   run the job (emu::RecipeJob; tests/test_nstep_recipes_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include "emu_learners.h"

using namespace dql;

namespace {

template <typename T> int launch(emu::RecipeJob& j, const char* out_path) {
  emu::RecipeRun<T> run(j);
  emu::LearnerState<T>& st = run.st;
  emu::PersistentWindows pw(st.n);  // (ens_alloc_windows)
  const auto nm = pw.mem();
  emu::WaveWindows lds;
  run.fly([&](int w, long long j0, int np, const long long* mgr0, const int* sched) {
    const int r = run.wave_recipe[(size_t)w], lvl = run.wave_level[(size_t)w];
    if ((unsigned)r >= (unsigned)j.n_recipes || (unsigned)lvl >= (unsigned)ADV_MAX_LEVELS) { st.faults[0] += 1ull; return; }
    const int nstep = run.tab.nstep[(size_t)r];
    if ((unsigned)nstep > (unsigned)NSTEP_MAX) { st.faults[0] += 1ull; return; }
    const RecipeSched& rs = run.tab.rs[(size_t)r];
    const SimK<T> cl = run.k.simk(lvl, rs.quirks);
    const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
    const LearnSched sc = learn_sched(rs.alpha_tab, rs.n_alpha, rs.alpha_min, (const LevelSched DQL_CONST_AS*)&rs.lv[lvl]);
    const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&run.tab.mdpk[(size_t)r * ADV_MAX_LEVELS + (size_t)lvl];
    lds.poison();
    for (int lane = 0; lane < ADV_WAVE; ++lane) {
      const long long l = run.worklist[(size_t)w * ADV_WAVE + (size_t)lane];
      const bool active = l >= 0 && l < j.n;
      if (nstep == 0)
        learner_periods<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, run.k.mdp_run, sc, run.mem, st.sr.data(), st.si.data(), j.seed, l, active, j0, np, mgr0, sched, lc.kv);
      else
        learner_periods_nstep<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, run.k.mdp_run, sc, run.mem, st.sr.data(), st.si.data(), j.seed, l, active, j0, np, mgr0, sched, lc.kv, nstep,
                                                  lds.view(lane), nm);
    }
  });
  return run.write(out_path, &pw);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: nstep_recipes_emu JOB OUT\n"); return 2; }
  emu::RecipeJob j(argv[1], false);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
