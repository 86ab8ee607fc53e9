// dql_recipes.inc: per-learner recipes for the ensembles of sequential learners (include/dql.h dql_ensemble_set_recipes ..., DESIGN.md section 16): the two
// kernels, struct EnsRecipes (what an ensemble holds while recipes are installed), what dql_ensemble_run passes to the advancing run loop for it, and the C calls.
// A fragment of dql_hip.hip's translation unit, included after dql_ensemble.inc, whose struct dql_ensemble, EnsWorklist, make_learn_args, ens_run_advancing and
// shared host helpers (ens_alloc_zeroed, ens_windows_empty, ens_check_upload_rule ...) it uses; csrc/dql_recipes.hpp holds the recipe structs, the worklist and the advance step.

// k_learn_levels with one more scalar load: wave w flies the learners worklist[64 w .. 64 w + 63] (-1: an inactive lane), all of them of recipe
// wave_recipe[w] on level wave_level[w].  From the recipe follow SimK::quirks, the learning rates and the level's exploration table and freeze rules; from
// (recipe, level) the MdpK (a.a.mdp is the array [R][5]).  After that the call to learner_periods is k_learn's.
template <typename T> struct LearnRecipesArgs {
  LearnArgs<T> a;                          // a.mdp: [n_recipes][DQL_MAX_LEVELS]; a.sched is not read (the recipe's RecipeSched replaces it)
  const RecipeSched DQL_CONST_AS* rs;      // [n_recipes]
  const int* worklist;                     // [64 n_waves]
  const int DQL_CONST_AS* wave_recipe;     // [n_waves]
  const int DQL_CONST_AS* wave_level;      // [n_waves]
  int n_waves, n_recipes;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_recipes(LearnRecipesArgs<T> g) {
  const LearnArgs<T>& a = g.a;
  const int tid = threadIdx.x;
  const int w = (int)blockIdx.x;
  if (w >= g.n_waves) return;
  const int r = g.wave_recipe[w];
  const int level = g.wave_level[w];
  // never taken unless a bug (the host builds the worklist)
  if ((unsigned)r >= (unsigned)g.n_recipes || (unsigned)level >= (unsigned)DQL_MAX_LEVELS) { if (tid == 0) a.mem.faults[0] += 1ull; return; }
  const long long l = (long long)g.worklist[(long long)w * 64 + tid];
  const RecipeSched DQL_CONST_AS* rs = g.rs + r;
  SimK<T> cl = a.c;
  cl.working = level;
  cl.quirks = rs->quirks;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // as in k_learn
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  const LearnSched sc = learn_sched(rs->alpha_tab, rs->n_alpha, rs->alpha_min, rs->lv + level);
  learner_periods<TICK, XMODE>(cl, cfgk, tc, a.mdp + (r * DQL_MAX_LEVELS + level), a.mdp_run, sc, a.mem, a.sr, a.si, a.seed, l, l >= 0 && l < a.mem.n, a.j0, a.n_periods, a.mgr0,
                               a.tick_sched, kv);
}
// an advance point: every learner takes advance_learner_recipe's step by itself, under its own recipe's rule (its own thread moves its own 2 x 567 cells;
// ordinary vector stores, nothing shared but the `faults` word: see k_ens_advance)
__global__ void k_ens_advance_recipes(LearnMem mem, AdvanceMem adv, const RecipeRule* rules, int n_recipes, const int* recipe_of, int4* si, long long j, int n_cells) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= mem.n) return;
  (void)advance_learner_recipe(mem, adv, rules, n_recipes, recipe_of, si, l, j, n_cells);
}

// ---- what an ensemble holds while recipes are installed (dql_ensemble::rcp; null: none are) ----
struct EnsRecipes {
  int n = 0;
  std::vector<int> recipe_of;                       // [L]
  RecipeRule rule[RCP_MAX]{}; bool have_rule[RCP_MAX]{};
  RecipeSched sched[RCP_MAX]{}; bool have_lv[RCP_MAX][DQL_MAX_LEVELS]{};   // (the tables its pointers name are the ensemble's device allocations)
  int* d_recipe_of = nullptr; RecipeRule* d_rule = nullptr; RecipeSched* d_sched = nullptr; void* d_mdpk = nullptr;  // [L], [n], [n], [n][DQL_MAX_LEVELS] MdpK<T>
  EnsWorklist wl;                                   // by (recipe, level) (capacity: worklist_capacity_recipes)
  // per-recipe n-step targets (DESIGN.md section 23, dql_nstep_recipes.inc): the capacity of the members' pending windows, 0: the one-step update; the device
  // copy [n] is made by the first dql_ensemble_set_recipe_nstep that changes an n and read by k_learn_recipes_nstep alone
  int nstep[RCP_MAX]{}; int* d_nstep = nullptr;
};
static void ens_recipes_release(dql_ensemble* x) {
  EnsRecipes* q = x->rcp;
  if (!q) return;
  for (int r = 0; r < q->n; ++r) {
    (void)x->dev.release((void*)q->sched[r].alpha_tab);
    for (int k = 0; k < DQL_MAX_LEVELS; ++k) (void)x->dev.release((void*)q->sched[r].lv[k].eps_tab);
  }
  void* own[] = {q->d_recipe_of, q->d_rule, q->d_sched, q->d_mdpk, q->wl.d_list, q->wl.d_wave_recipe, q->wl.d_wave_level, q->d_nstep};
  for (void* p : own) (void)x->dev.release(p);
  delete q;
  x->rcp = nullptr;
}
static const AdvanceRule& ens_rule_of(const dql_ensemble* x, size_t l) {
  return x->rcp ? x->rcp->rule[x->rcp->recipe_of[l]].rule : x->rule;
}
static int ens_recipes_min_last_level(const dql_ensemble* x) {  // over the recipes that have a member and a rule; 4 where there is none
  int lo = DQL_MAX_LEVELS - 1;
  for (int r : x->rcp->recipe_of) if (x->rcp->have_rule[r] && x->rcp->rule[r].rule.last_level < lo) lo = x->rcp->rule[r].rule.last_level;
  return lo;
}
// what k_learn_recipes and k_learn_recipes_nstep (dql_nstep_recipes.inc) share
template <typename T> static LearnRecipesArgs<T> make_learn_recipes_args(dql_ensemble* x, int k, int n_waves) {
  EnsRecipes* q = x->rcp;
  LearnRecipesArgs<T> g;
  g.a = make_learn_args<T>(x, q->d_mdpk, k);
  g.rs = (const RecipeSched DQL_CONST_AS*)q->d_sched; g.worklist = q->wl.d_list;
  g.wave_recipe = (const int DQL_CONST_AS*)q->wl.d_wave_recipe; g.wave_level = (const int DQL_CONST_AS*)q->wl.d_wave_level;
  g.n_waves = n_waves; g.n_recipes = q->n;
  return g;
}
template <typename T> static void launch_learn_recipes(dql_ensemble* x, int k, int n_waves) {
  hipLaunchKernelGGL((k_learn_recipes<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, make_learn_recipes_args<T>(x, k, n_waves));
}
static bool ens_recipes_any_nstep(const dql_ensemble* x) {  // a recipe that has a member has n >= 1
  for (int r : x->rcp->recipe_of) if (x->rcp->nstep[r] >= 1) return true;
  return false;
}
static const int* ens_recipes_nstep_table(const dql_ensemble* x) { return x->rcp->d_nstep; }
// the advancing run loop with the recipe-aware learner_finished (ens_fetch_levels reads each learner's own rule), worklist and kernels.  Complete: every recipe
// with a member has its rule, and schedules for the level each member stands on and every level on its way up to last_level
static int ens_run_recipes(dql_ensemble* x, int64_t periods, EnsKernel kern) {
  EnsRecipes* q = x->rcp;
  return ens_run_advancing(x, periods, kern, q->wl,
                           [&](size_t l, int level) { const int r = q->recipe_of[l]; return q->have_rule[r] && ens_way_up_scheduled(q->have_lv[r], level, q->rule[r].rule.last_level); },
                           "dql_ensemble_run: with recipes installed every recipe that has a member needs dql_ensemble_set_recipe and dql_ensemble_set_recipe_level_schedules for every "
                           "level from its members' up to its last_level; nothing was launched", [&] {
                             hipLaunchKernelGGL(k_ens_advance_recipes, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, 0, x->mem, x->adv, (const RecipeRule*)q->d_rule, q->n,
                                                (const int*)q->d_recipe_of, x->si, (long long)x->j, (int)DQL_CELLS_PER_LEVEL);
                           });
}
// an install or an uninstall would orphan pending entries of the recipes' n-step targets (only an ensemble that called dql_ensemble_set_recipe_nstep with
// n >= 1 has window arrays while recipes can be installed); DQL_OK: every window is empty
static int ens_recipes_windows_empty(dql_ensemble* x) {
  return ens_windows_empty(x, [](size_t) { return true; }, "dql_ensemble_set_recipes: recipes cannot be installed or uninstalled while a learner's pending window holds entries (after dql_ensemble_set_level, or when every learner is frozen); nothing was changed");
}

extern "C" {
int dql_ensemble_set_recipes(dql_ensemble* x, int32_t n_recipes, const int32_t* recipe_of) {
  CHECK_ENS(x);
  ENS_REFINED_REFUSED(x, "dql_ensemble_set_recipes", ENS_REFINED_MODES);
  if (x->envs_per_learner > 1) return fail(DQL_EINVAL, ENS_TEAMS_REFUSED("dql_ensemble_set_recipes"));
  if (x->team_every) return fail(DQL_EINVAL, ENS_TEAM_LEVELS_REFUSED("dql_ensemble_set_recipes"));
  if (n_recipes < 0 || n_recipes > RCP_MAX) return fail(DQL_EINVAL, "dql_ensemble_set_recipes: n_recipes must be in 0..64 (0 uninstalls); nothing was changed");
  if (n_recipes == 0) {
    HIP_TRY(hipSetDevice(x->device));
    HIP_TRY(hipDeviceSynchronize());
    if (x->rcp) { int rc = ens_recipes_windows_empty(x); if (rc) return rc; }
    ens_recipes_release(x);
    return DQL_OK;
  }
  if (x->nstep) return fail(DQL_EINVAL, ENS_NSTEP_REFUSED("dql_ensemble_set_recipes"));
  if (x->team_nstep) return fail(DQL_EINVAL, ENS_TEAM_NSTEP_REFUSED("dql_ensemble_set_recipes"));
  if (!x->advance_every) return fail(DQL_EINVAL, "dql_ensemble_set_recipes: recipes need curriculum mode (dql_ensemble_set_curriculum with advance_every > 0 first); nothing was changed");
  if (!recipe_of) return fail(DQL_EINVAL, "dql_ensemble_set_recipes: null recipe_of; nothing was changed");
  for (long long l = 0; l < x->n; ++l)
    if (recipe_of[l] < 0 || recipe_of[l] >= n_recipes) return fail(DQL_EINVAL, "dql_ensemble_set_recipes: every recipe_of[l] must be in 0..n_recipes - 1; nothing was changed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  { int rc = ens_recipes_windows_empty(x); if (rc) return rc; }
  // the new set is allocated in full before the installed one is let go
  EnsRecipes* q = new EnsRecipes;
  q->n = n_recipes;
  q->recipe_of.assign(recipe_of, recipe_of + x->n);
  q->wl.resize(worklist_capacity_recipes(x->n, n_recipes), q->recipe_of.data(), n_recipes);
  const size_t n = (size_t)x->n, R = (size_t)n_recipes, waves = (size_t)(q->wl.slots / ADV_WAVE);
  bool ok = ens_alloc_zeroed(x->dev, {{(void**)&q->d_recipe_of, n * sizeof(int)}, {(void**)&q->d_rule, R * sizeof(RecipeRule)}, {(void**)&q->d_sched, R * sizeof(RecipeSched)},
                                      {&q->d_mdpk, R * DQL_MAX_LEVELS * mdpk_bytes(x->cfg.dtype)}, {(void**)&q->wl.d_list, (size_t)q->wl.slots * sizeof(int)},
                                      {(void**)&q->wl.d_wave_recipe, waves * sizeof(int)}, {(void**)&q->wl.d_wave_level, waves * sizeof(int)}}) == DQL_OK;
  ok = ok && hipMemcpy(q->d_recipe_of, q->recipe_of.data(), n * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    void* own[] = {q->d_recipe_of, q->d_rule, q->d_sched, q->d_mdpk, q->wl.d_list, q->wl.d_wave_recipe, q->wl.d_wave_level};
    for (void* p : own) (void)x->dev.release(p);
    delete q;
    return fail(DQL_ENOMEM, "dql_ensemble_set_recipes: device memory for the recipes could not be set up; nothing was changed");
  }
  ens_recipes_release(x);
  x->rcp = q;
  return DQL_OK;
}
#define CHECK_RECIPE(who, x, r) do { CHECK_ENS(x); ENS_REFINED_REFUSED(x, who, ENS_REFINED_MODES); \
    if (!(x)->rcp) return fail(DQL_EINVAL, std::string(who) + ": no recipes are installed (dql_ensemble_set_recipes first); nothing was changed"); \
    if ((r) < 0 || (r) >= (x)->rcp->n) return fail(DQL_EINVAL, std::string(who) + ": the recipe must be in 0..n_recipes - 1; nothing was changed"); } while (0)
int dql_ensemble_set_recipe(dql_ensemble* x, int32_t r, uint32_t quirks, const double* alpha, int32_t n_alpha, double alpha_min, const double* ratios, int32_t last_level,
                            int32_t advance_exhausted, int32_t transfer_order) {
  CHECK_RECIPE("dql_ensemble_set_recipe", x, r);
  EnsRecipes* q = x->rcp;
  dql_config c = x->cfg;
  c.quirks = quirks;
  int rc = check_config(&c); if (rc) return rc;
  if (!alpha) return fail(DQL_EINVAL, "dql_ensemble_set_recipe: null table; nothing was changed");
  if (n_alpha < 1 || n_alpha > (1 << 22)) return fail(DQL_EINVAL, "dql_ensemble_set_recipe: table lengths must be in 1..2^22; nothing was changed");
  rc = ens_check_rates(alpha, n_alpha, "dql_ensemble_set_recipe: learning rates must be in [0, 1]; nothing was changed"); if (rc) return rc;
  if (!(alpha_min >= 0.0 && alpha_min <= 1.0)) return fail(DQL_EINVAL, "dql_ensemble_set_recipe: learning rates must be in [0, 1] (alpha_min); nothing was changed");
  if (!ratios) return fail(DQL_EINVAL, "dql_ensemble_set_recipe: null ratios; nothing was changed");
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) if (!std::isfinite(ratios[k])) return fail(DQL_EINVAL, "dql_ensemble_set_recipe: the five transfer ratios must be finite; nothing was changed");
  if (advance_exhausted != 0 && advance_exhausted != 1) return fail(DQL_EINVAL, "dql_ensemble_set_recipe: advance_exhausted must be 0 or 1; nothing was changed");
  if (transfer_order != RCP_ORDER_REFERENCE && transfer_order != RCP_ORDER_PAPER)
    return fail(DQL_EINVAL, "dql_ensemble_set_recipe: transfer_order must be 0 (the reference's) or 1 (the paper's); nothing was changed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int> level;
  rc = ens_fetch(x->adv.level, (size_t)x->n, level); if (rc) return rc;
  int top = 0;
  for (size_t l = 0; l < level.size(); ++l) if (q->recipe_of[l] == r && level[l] > top) top = level[l];
  if (last_level < top || last_level >= DQL_MAX_LEVELS)
    return fail(DQL_EINVAL, "dql_ensemble_set_recipe: last_level must lie between the current level of the recipe's learners and 4; nothing was changed");
  // the device side is staged in full, then swapped in
  const size_t mb = mdpk_bytes(x->cfg.dtype);
  std::vector<char> staged(DQL_MAX_LEVELS * mb);
  double* d_a = nullptr;
  if (x->dev.alloc((void**)&d_a, (size_t)n_alpha * sizeof(double)) != hipSuccess) return fail(DQL_ENOMEM, "dql_ensemble_set_recipe: hipMalloc failed; nothing was changed");
  RecipeRule rule{};
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) rule.rule.ratios[k] = ratios[k];
  rule.rule.last_level = last_level; rule.rule.advance_exhausted = advance_exhausted; rule.transfer_order = transfer_order;
  RecipeSched s = q->sched[r];
  s.alpha_tab = d_a; s.n_alpha = n_alpha; s.alpha_min = alpha_min; s.quirks = quirks;
  bool ok = hipMemcpy(d_a, alpha, (size_t)n_alpha * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  for (int k = 0; ok && k < DQL_MAX_LEVELS; ++k) {  // the recipe's MdpK per level: the config with the recipe's quirks and working = k
    c.working_curriculum_step = k;
    ok = upload_mdpk(c, (char*)q->d_mdpk + ((size_t)r * DQL_MAX_LEVELS + (size_t)k) * mb) == DQL_OK;
  }
  ok = ok && hipMemcpy(q->d_rule + r, &rule, sizeof(rule), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(q->d_sched + r, &s, sizeof(s), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {  // (the recipe is left without a rule: dql_ensemble_run refuses it until the call succeeds)
    (void)x->dev.release(d_a);
    q->have_rule[r] = false;
    return fail(DQL_EHIP, "dql_ensemble_set_recipe: a copy to the device failed; the recipe has no rule now");
  }
  (void)x->dev.release((void*)q->sched[r].alpha_tab);  // the table it replaces
  q->sched[r] = s; q->rule[r] = rule; q->have_rule[r] = true;
  return DQL_OK;
}
int dql_ensemble_set_recipe_level_schedules(dql_ensemble* x, int32_t r, int32_t level, const double* eps, int32_t n_eps, int32_t window, int32_t min_successes, int32_t max_episodes) {
  CHECK_RECIPE("dql_ensemble_set_recipe_level_schedules", x, r);
  EnsRecipes* q = x->rcp;
  if (level < 0 || level >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_recipe_level_schedules: the level must be in 0..4; nothing was changed");
  if (!eps) return fail(DQL_EINVAL, "dql_ensemble_set_recipe_level_schedules: null table; nothing was changed");
  if (n_eps < 1 || n_eps > (1 << 22)) return fail(DQL_EINVAL, "dql_ensemble_set_recipe_level_schedules: the table length must be in 1..2^22; nothing was changed");
  uint32_t* d_e = nullptr;
  const int rc = ens_check_upload_rule(x, "dql_ensemble_set_recipe_level_schedules", "; nothing was changed", nullptr, 0, eps, n_eps, window, min_successes, max_episodes, &d_e); if (rc) return rc;
  RecipeSched s = q->sched[r];
  s.lv[level] = LevelSched{d_e, n_eps, window, min_successes, max_episodes};
  if (hipMemcpy(q->d_sched + r, &s, sizeof(s), hipMemcpyHostToDevice) != hipSuccess) { (void)x->dev.release(d_e); return fail(DQL_EHIP, "hipMemcpy failed"); }
  (void)x->dev.release((void*)q->sched[r].lv[level].eps_tab);  // the table it replaces
  q->sched[r] = s; q->have_lv[r][level] = true;
  return DQL_OK;
}
int dql_ensemble_get_recipes(dql_ensemble* x, int32_t* recipe_of) {
  CHECK_ENS(x);
  if (!recipe_of) return fail(DQL_EINVAL, "dql_ensemble_get_recipes: null array");
  for (long long l = 0; l < x->n; ++l) recipe_of[l] = x->rcp ? x->rcp->recipe_of[(size_t)l] : -1;
  return DQL_OK;
}
}  // extern "C"
