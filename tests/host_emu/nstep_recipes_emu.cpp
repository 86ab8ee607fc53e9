// nstep_recipes_emu.cpp — dql_ensemble_run with recipes installed of which some have n-step targets, emulated on the CPU from the real
// device source: dql_recipes.hpp's build_worklist_recipes and advance_learner_recipe on top of dql_nstep.hpp's learner_periods_nstep and dql_learner.hpp's
// learner_periods.
//
// recipes_emu.cpp's driver with nstep_emu.cpp's windows.  It does what ens_run_advancing (dql_ensemble.inc) does for ens_run_recipes (dql_recipes.inc): launches cut at the multiples of
// advance_every; at such a period index every learner takes advance_learner_recipe's step; then the live learners are regrouped by (recipe, level) and flown
// wave by wave, lane by lane, as k_learn_recipes_nstep (dql_nstep_recipes.inc) flies them — the wave's recipe and level from wave_recipe[w] and wave_level[w],
// its n from recipe_nstep[recipe], the lane's learner from the worklist (-1: an inactive lane); a wave with n = 0 flies learner_periods, the others
// learner_periods_nstep.  A lane runs alone: __ballot(p) is p (host_shim.h).  The windows are reached through checked references: the wave's working copy
// stands for the kernel's LDS ([NSTEP_MAX][64], the lane's column) and is poisoned before every wave (keys 0xffff, rewards NaN), as LDS carries nothing from
// launch to launch; the persistent copy is [NSTEP_MAX][n] plus len[n], exactly as long as the library's, entries poisoned, lengths zeroed.  An index outside
// them ends the run with status 3.  Every other array is exactly as long as the library allocates it, so the sanitized build sees any access beyond them.
//
//   nstep_recipes_emu JOB OUT   run the job (see read_job; tests/test_nstep_recipes_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_returns.hpp"
#include "dql_nstep.hpp"
#include "dql_advance.hpp"
#include "dql_recipes.hpp"
#define DQL_EMU_LEARNERS
#include "emu_common.h"

using namespace dql;

namespace {

struct JobRecipe {
  uint32_t quirks;
  int n_alpha, last_level, advance_exhausted, transfer_order, nstep;
  int n_eps[ADV_MAX_LEVELS], window[ADV_MAX_LEVELS], min_successes[ADV_MAX_LEVELS], max_episodes[ADV_MAX_LEVELS];
  double alpha_min, ratios[ADV_MAX_LEVELS];
  std::vector<double> alpha, eps[ADV_MAX_LEVELS];
};
struct Job {
  int dtype, n_runs, runs[8], every, log_cap, n_recipes, has_tables;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<int> recipe_of;
  std::vector<JobRecipe> recipes;
  std::vector<double> qa, qb, count;  // the tables: zeros, or the job's initial ones ([L][DQL_N_CELLS] each, at the end of the job)
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[24];  // cfg size, dtype, L, n_runs, runs[8], every, log_cap, n_recipes, has_tables, 0 ...
  int64_t seed;
  f.read(hdr, 24); f.read(&seed, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n = hdr[2]; j.n_runs = hdr[3];
  for (int k = 0; k < 8; ++k) j.runs[k] = hdr[4 + k];
  j.seed = (unsigned long long)seed;
  j.every = hdr[12]; j.log_cap = hdr[13]; j.n_recipes = hdr[14]; j.has_tables = hdr[15];
  if (j.n < 1) emu::bad_job();
  j.recipe_of.resize((size_t)j.n);
  f.read(j.recipe_of);
  bool ok = j.n_runs >= 1 && j.n_runs <= 8 && j.every >= 1 && j.every <= ADV_MAX_EVERY && j.log_cap >= 1 && j.n_recipes >= 1 && j.n_recipes <= RCP_MAX && !j.cfg.two_axis &&
            j.cfg.trajectory != DQL_TRAJ_EIGHT;
  for (int k = 0; ok && k < j.n_runs; ++k) ok = j.runs[k] >= 1;
  for (size_t l = 0; ok && l < (size_t)j.n; ++l) ok = j.recipe_of[l] >= 0 && j.recipe_of[l] < j.n_recipes;
  if (!ok) emu::bad_job();
  j.recipes.resize((size_t)j.n_recipes);
  for (JobRecipe& r : j.recipes) {
    int32_t h[28];  // quirks, n_alpha, last_level, advance_exhausted, transfer_order, nstep, 0, 0, then per level {n_eps, window, min_successes, max_episodes}
    f.read(h, 28);
    r.quirks = (uint32_t)h[0]; r.n_alpha = h[1]; r.last_level = h[2]; r.advance_exhausted = h[3]; r.transfer_order = h[4]; r.nstep = h[5];
    ok = r.n_alpha >= 1 && r.last_level >= j.cfg.working_curriculum_step && r.last_level < ADV_MAX_LEVELS && (r.transfer_order == 0 || r.transfer_order == 1) && r.nstep >= 0 &&
         r.nstep <= NSTEP_MAX;
    for (int k = 0; k < ADV_MAX_LEVELS; ++k) {
      r.n_eps[k] = h[8 + 4 * k]; r.window[k] = h[9 + 4 * k]; r.min_successes[k] = h[10 + 4 * k]; r.max_episodes[k] = h[11 + 4 * k];
      ok = ok && r.n_eps[k] >= 1 && r.window[k] >= 1 && r.window[k] <= LEARN_MAX_WINDOW && r.min_successes[k] >= 1 && r.max_episodes[k] >= 1;
    }
    if (!ok) emu::bad_job();
    f.read(&r.alpha_min, 1); f.read(r.ratios, ADV_MAX_LEVELS);
    r.alpha.resize((size_t)r.n_alpha);
    f.read(r.alpha);
    for (int k = 0; k < ADV_MAX_LEVELS; ++k) { r.eps[k].resize((size_t)r.n_eps[k]); f.read(r.eps[k]); }
  }
  const size_t TB = (size_t)j.n * DQL_N_CELLS;
  j.qa.assign(TB, 0.0); j.qb.assign(TB, 0.0); j.count.assign(TB, 0.0);
  if (j.has_tables) { f.read(j.qa); f.read(j.qb); f.read(j.count); }
  return j;
}

// an array of the window's storage as the device code indexes it: every element reached is bounds-checked
template <typename V> struct Checked {
  V* p; long long size; const char* what;
  V& operator[](long long k) const {
    if (k < 0 || k >= size) { std::fprintf(stderr, "INDEX VIOLATION: element %lld of %s outside [0, %lld)\n", k, what, size); std::exit(3); }
    return p[k];
  }
};
struct EmuWindow {  // dql_nstep.inc's LdsWindow
  Checked<uint16_t> k; Checked<double> v; int lane;
  uint16_t& key(int slot) const { if (slot < 0 || slot >= NSTEP_MAX) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d\n", slot); std::exit(3); } return k[(long long)slot * 64 + lane]; }
  double& val(int slot) const { if (slot < 0 || slot >= NSTEP_MAX) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d\n", slot); std::exit(3); } return v[(long long)slot * 64 + lane]; }
};

template <typename T> int launch(Job& j, const char* out_path) {
  const dql_config& cfg = j.cfg;
  const size_t n = (size_t)j.n, R = (size_t)j.n_recipes;
  const SimK<T> c = make_simk<T>(cfg);
  std::vector<MdpK<T>> mdpk(R * ADV_MAX_LEVELS);  // [R][5]: the config with the recipe's quirks and working = k (dql_ensemble_set_recipe)
  std::vector<std::vector<uint32_t>> thr(R * ADV_MAX_LEVELS);
  std::vector<RecipeSched> rs(R);
  std::vector<RecipeRule> rules(R);
  std::vector<int> recipe_nstep(R);  // EnsRecipes::d_nstep
  for (size_t r = 0; r < R; ++r) {
    const JobRecipe& q = j.recipes[r];
    rs[r].alpha_tab = q.alpha.data(); rs[r].n_alpha = q.n_alpha; rs[r].quirks = q.quirks; rs[r].alpha_min = q.alpha_min;
    recipe_nstep[r] = q.nstep;
    for (int k = 0; k < ADV_MAX_LEVELS; ++k) {
      dql_config ck = cfg; ck.quirks = q.quirks; ck.working_curriculum_step = k;
      mdpk[r * ADV_MAX_LEVELS + (size_t)k] = make_mdpk<T>(ck);
      std::vector<uint32_t>& t = thr[r * ADV_MAX_LEVELS + (size_t)k];
      t.resize((size_t)q.n_eps[k]);
      for (int i = 0; i < q.n_eps[k]; ++i) t[(size_t)i] = eps_threshold(q.eps[k][(size_t)i]);
      rs[r].lv[k] = LevelSched{t.data(), q.n_eps[k], q.window[k], q.min_successes[k], q.max_episodes[k]};
      rules[r].rule.ratios[k] = q.ratios[k];
    }
    rules[r].rule.last_level = q.last_level; rules[r].rule.advance_exhausted = q.advance_exhausted; rules[r].transfer_order = q.transfer_order; rules[r].pad_ = 0;
  }
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  emu::LearnerState<T> st(c, init, n, j.seed, j.log_cap);  // (at the config's level, with the config's quirks: k_init reads neither a recipe nor a level)
  const LearnMem mem = st.mem(j.qa, j.qb, j.count);
  std::vector<int> level(n, cfg.working_curriculum_step), promoted_at((size_t)ADV_MAX_LEVELS * n, -1), episodes_at((size_t)ADV_MAX_LEVELS * n, 0);
  std::vector<long long> entered((size_t)ADV_MAX_LEVELS * n, -1);
  for (size_t l = 0; l < n; ++l) entered[(size_t)cfg.working_curriculum_step * n + l] = 0;
  const AdvanceMem adv{level.data(), promoted_at.data(), episodes_at.data(), entered.data()};
  const long long slots = worklist_capacity_recipes((long long)n, j.n_recipes);
  std::vector<int> worklist((size_t)slots), wave_recipe((size_t)(slots / ADV_WAVE)), wave_level((size_t)(slots / ADV_WAVE));
  // the persistent windows: as long as ens_alloc_windows allocates them; the lengths zeroed, the entries poisoned
  std::vector<uint16_t> g_key((size_t)NSTEP_MAX * n, (uint16_t)0xffffu);
  std::vector<double> g_val((size_t)NSTEP_MAX * n, std::nan(""));
  std::vector<int> g_len(n, 0);
  const NstepMem<Checked<uint16_t>, Checked<double>, Checked<int>> nm{{g_key.data(), (long long)g_key.size(), "the persistent keys"},
                                                                      {g_val.data(), (long long)g_val.size(), "the persistent rewards"},
                                                                      {g_len.data(), (long long)g_len.size(), "the persistent lengths"}};
  std::vector<uint16_t> lds_key((size_t)NSTEP_MAX * 64);
  std::vector<double> lds_val((size_t)NSTEP_MAX * 64);

  long long j0 = 0;
  for (int run = 0; run < j.n_runs; ++run) {
    long long left = j.runs[run];
    while (left > 0) {
      if (j0 % j.every == 0)
        for (size_t l = 0; l < n; ++l) (void)advance_learner_recipe(mem, adv, rules.data(), j.n_recipes, j.recipe_of.data(), st.si.data(), (long long)l, j0, DQL_CELLS_PER_LEVEL);
      long long unfinished = 0;
      for (size_t l = 0; l < n; ++l) unfinished += learner_finished(st.frozen[l], level[l], st.promoted[l], rules[(size_t)j.recipe_of[l]].rule) ? 0 : 1;
      if (unfinished == 0) { j0 += left; break; }
      const long long to_point = j.every - j0 % j.every;
      const int np = (int)(left < to_point ? left : to_point);
      const int n_waves = build_worklist_recipes(st.frozen.data(), level.data(), j.recipe_of.data(), (long long)n, j.n_recipes, worklist.data(), wave_recipe.data(), wave_level.data(),
                                                 slots, st.faults.data());
      std::vector<long long> mgr0((size_t)np);
      std::vector<int> sched((size_t)np);
      fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
      for (int w = 0; w < n_waves; ++w) {
        const int r = wave_recipe[(size_t)w], k = wave_level[(size_t)w];
        if ((unsigned)r >= (unsigned)j.n_recipes || (unsigned)k >= (unsigned)ADV_MAX_LEVELS) { st.faults[0] += 1ull; continue; }
        const int nstep = recipe_nstep[(size_t)r];
        if ((unsigned)nstep > (unsigned)NSTEP_MAX) { st.faults[0] += 1ull; continue; }
        SimK<T> cl = c;
        cl.working = k;
        cl.quirks = rs[(size_t)r].quirks;
        cl.two_axis = 0;
        const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
        const LearnSched sc = learn_sched(rs[(size_t)r].alpha_tab, rs[(size_t)r].n_alpha, rs[(size_t)r].alpha_min, (const LevelSched DQL_CONST_AS*)&rs[(size_t)r].lv[k]);
        const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk[(size_t)r * ADV_MAX_LEVELS + (size_t)k];
        lds_key.assign(lds_key.size(), (uint16_t)0xffffu); lds_val.assign(lds_val.size(), std::nan(""));
        for (int lane = 0; lane < ADV_WAVE; ++lane) {
          const long long l = worklist[(size_t)w * ADV_WAVE + (size_t)lane];
          const bool active = l >= 0 && l < (long long)n;
          if (nstep == 0) {
            learner_periods<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, sc, mem, st.sr.data(), st.si.data(), j.seed, l, active, j0, np, mgr0.data(), sched.data(), lc.kv);
          } else {
            const EmuWindow win{{lds_key.data(), (long long)lds_key.size(), "the working keys"}, {lds_val.data(), (long long)lds_val.size(), "the working rewards"}, lane};
            learner_periods_nstep<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, sc, mem, st.sr.data(), st.si.data(), j.seed, l, active, j0, np, mgr0.data(), sched.data(), lc.kv, nstep,
                                                      win, nm);
          }
        }
      }
      j0 += np; left -= np;
    }
  }
  // dql_ensemble_get_levels: the row of a learner's current level shows its counters as they stand
  for (size_t l = 0; l < n; ++l) { promoted_at[(size_t)level[l] * n + l] = st.promoted[l]; episodes_at[(size_t)level[l] * n + l] = st.lvl[l]; }
  emu::ResultFile f(out_path);
  st.put(f, j.qa, j.qb, j.count);
  f.put(level); f.put(promoted_at); f.put(episodes_at); f.put(entered); f.put(&j0, 1);
  f.put(g_len);
  return f.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: nstep_recipes_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
