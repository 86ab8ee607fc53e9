// dql_nstep_recipes.inc: n-step Double-Q targets as a property of a recipe (include/dql.h dql_ensemble_set_recipe_nstep / _get_recipe_nstep, DESIGN.md
// section 23): the kernel that flies a (recipe, level) worklist with either lane body, its argument filler, and the two C calls.  A fragment of dql_hip.hip's
// translation unit, included after dql_recipes.inc (EnsRecipes, LearnRecipesArgs, CHECK_RECIPE) and dql_nstep.inc (LdsWindow, NstepDev, ens_alloc_windows).

// k_learn_recipes' shape and prologue with k_learn_nstep's LDS windows: wave w flies worklist[64 w .. 64 w + 63] of recipe wave_recipe[w] on level
// wave_level[w]; the capacity of its pending windows is recipe_nstep[recipe], one scalar load, so it is wave-uniform like everything else the recipe gives.
// A wave whose recipe has n = 0 branches (wave-uniformly) into learner_periods, exactly what k_learn_recipes calls; the others fly learner_periods_nstep.
// The windows: [slot][lane], 10 KB per wave, a lane touches its own column only, no barrier (dql_nstep.inc).
template <typename T> struct LearnRecipesNstepArgs {
  LearnRecipesArgs<T> g;
  NstepDev nm;
  const int DQL_CONST_AS* recipe_nstep;  // [n_recipes]
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_recipes_nstep(LearnRecipesNstepArgs<T> h) {
  const LearnRecipesArgs<T>& g = h.g;
  const LearnArgs<T>& a = g.a;
  const int tid = threadIdx.x;
  const int w = (int)blockIdx.x;
  if (w >= g.n_waves) return;
  const int r = g.wave_recipe[w];
  const int level = g.wave_level[w];
  // never taken unless a bug (the host builds the worklist)
  if ((unsigned)r >= (unsigned)g.n_recipes || (unsigned)level >= (unsigned)DQL_MAX_LEVELS) { if (tid == 0) a.mem.faults[0] += 1ull; return; }
  const int nstep = h.recipe_nstep[r];
  if ((unsigned)nstep > (unsigned)NSTEP_MAX) { if (tid == 0) a.mem.faults[0] += 1ull; return; }  // (the host checks every n it stores)
  const long long l = (long long)g.worklist[(long long)w * 64 + tid];
  const RecipeSched DQL_CONST_AS* rs = g.rs + r;
  SimK<T> cl = a.c;
  cl.working = level;
  cl.quirks = rs->quirks;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // as in k_learn
  __shared__ uint16_t sKey[NSTEP_MAX * 64];
  __shared__ double sVal[NSTEP_MAX * 64];
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  const LearnSched sc = learn_sched(rs->alpha_tab, rs->n_alpha, rs->alpha_min, rs->lv + level);
  const bool active = l >= 0 && l < a.mem.n;
  // the Philox key schedule (float32: in VGPRs, as in k_learn) is made once per body: one array read by both bodies stays in private memory
  if (nstep == 0) {
    uint32_t kv_[20];
    const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
    learner_periods<TICK, XMODE>(cl, cfgk, tc, a.mdp + (r * DQL_MAX_LEVELS + level), a.mdp_run, sc, a.mem, a.sr, a.si, a.seed, l, active, a.j0, a.n_periods, a.mgr0, a.tick_sched, kv);
  } else {
    uint32_t kv_[20];
    const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
    learner_periods_nstep<TICK, XMODE>(cl, cfgk, tc, a.mdp + (r * DQL_MAX_LEVELS + level), a.mdp_run, sc, a.mem, a.sr, a.si, a.seed, l, active, a.j0, a.n_periods, a.mgr0,
                                       a.tick_sched, kv, nstep, LdsWindow{sKey + tid, sVal + tid}, h.nm);
  }
}

// launch_learn_recipes' sibling: the same arguments with the windows and the recipes' n
template <typename T> static void launch_learn_recipes_nstep(dql_ensemble* x, int k, int n_waves) {
  LearnRecipesNstepArgs<T> h;
  h.g = make_learn_recipes_args<T>(x, k, n_waves);
  h.nm = NstepDev{x->ns_key, x->ns_val, x->ns_len};
  h.recipe_nstep = (const int DQL_CONST_AS*)x->rcp->d_nstep;
  hipLaunchKernelGGL((k_learn_recipes_nstep<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, h);
}

extern "C" {
int dql_ensemble_set_recipe_nstep(dql_ensemble* x, int32_t r, int32_t n) {
  CHECK_RECIPE("dql_ensemble_set_recipe_nstep", x, r);
  EnsRecipes* q = x->rcp;
  if (n < 0 || n > DQL_NSTEP_MAX) return fail(DQL_EINVAL, "dql_ensemble_set_recipe_nstep: n must be in 0..16 (DQL_NSTEP_MAX; 0: the one-step update); nothing was changed");
  if (n == q->nstep[r]) return DQL_OK;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  int rc = ens_windows_empty(x, [&](size_t l) { return q->recipe_of[l] == r; }, "dql_ensemble_set_recipe_nstep: a recipe's n cannot change while a member's pending window holds entries (change it after dql_ensemble_set_recipes, after dql_ensemble_set_level, or when every member is frozen); nothing was changed");
  if (rc) return rc;
  if (n >= 1) { rc = ens_alloc_windows(x); if (rc) return rc; }
  int* d = q->d_nstep;
  if (!d) {  // [n_recipes], zeros until set
    if (x->dev.alloc((void**)&d, (size_t)q->n * sizeof(int)) != hipSuccess) return fail(DQL_ENOMEM, "dql_ensemble_set_recipe_nstep: hipMalloc failed; nothing was changed");
    if (hipMemcpy(d, q->nstep, (size_t)q->n * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { (void)x->dev.release(d); return fail(DQL_EHIP, "dql_ensemble_set_recipe_nstep: a copy to the device failed; nothing was changed"); }
  }
  const int v = n;
  if (hipMemcpy(d + r, &v, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    if (!q->d_nstep) (void)x->dev.release(d);
    return fail(DQL_EHIP, "dql_ensemble_set_recipe_nstep: a copy to the device failed; nothing was changed");
  }
  q->d_nstep = d;
  q->nstep[r] = n;
  return DQL_OK;
}
int dql_ensemble_get_recipe_nstep(dql_ensemble* x, int32_t r, int32_t* n) {
  CHECK_RECIPE("dql_ensemble_get_recipe_nstep", x, r);
  if (!n) return fail(DQL_EINVAL, "dql_ensemble_get_recipe_nstep: null pointer");
  *n = x->rcp->nstep[r];
  return DQL_OK;
}
}  // extern "C"
