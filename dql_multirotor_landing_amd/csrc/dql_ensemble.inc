// dql_ensemble.inc: ensembles of sequential Double-Q learners (include/dql.h dql_ensemble_*, DESIGN.md sections 12 and 14): the lane kernels, struct dql_ensemble
// and its C calls.  A fragment of dql_hip.hip's translation unit, not a header.  Needs from it: fail / HIP_TRY, by_dtype, OP_PROLOGUE, DevOwned, upload_mdpk,
// upload_schedule, EvTimer, quads_to_fields / unpack_ints, check_config, InitArgs / k_init, k_mark_reset, TickLds; dql_learner.hpp, dql_advance.hpp, dql_team_levels.hpp; and
// score_check / score_run / TableSets of dql_greedy.inc (dql_ensemble_score, tables_of_slice).  dql_recipes.inc, included after this file, holds the per-learner recipes (DESIGN.md section 16).
// ---- sequential learners (dql_ensemble, DESIGN.md section 12) ----
// One learner per lane (csrc/dql_learner.hpp: learner_periods), workgroups of one wave as in k_rollout; the env stays in registers for all periods of the launch,
// the tables are the lane's own [DQL_N_CELLS] slices (per-lane global pointers, ordinary vector loads and stores, no atomics).
template <typename T> struct LearnArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  LearnSched sched;
  LearnMem mem;
  Quad<T>* sr; int4* si;
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* tick_sched;  // [n_periods] (fill_schedule from period j0)
  unsigned long long seed;
  long long j0;
  int n_periods;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn(LearnArgs<T> a) {
  const int tid = threadIdx.x;
  const long long l = (long long)blockIdx.x * 64 + tid;
  SimK<T> cl = a.c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // float64: the tick's constants are read from LDS (k_step); float32: an unused byte
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  learner_periods<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.sched, a.mem, a.sr, a.si, a.seed, l, l < a.mem.n, a.j0, a.n_periods, a.mgr0, a.tick_sched, kv);
}
// transfer_learning on every learner's tables: Q[l][k] = Q[l][src] * ratio (k_transfer's arithmetic)
__global__ void k_ens_transfer(double* qa, double* qb, long long n, int k, int src, double ratio) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * DQL_CELLS_PER_LEVEL) return;
  const long long l = t / DQL_CELLS_PER_LEVEL; const int i = (int)(t - l * DQL_CELLS_PER_LEVEL);
  double* a = qa + l * DQL_N_CELLS; double* b = qb + l * DQL_N_CELLS;
  a[k * DQL_CELLS_PER_LEVEL + i] = a[src * DQL_CELLS_PER_LEVEL + i] * ratio;
  b[k * DQL_CELLS_PER_LEVEL + i] = b[src * DQL_CELLS_PER_LEVEL + i] * ratio;
}

// ---- per-learner curriculum levels (DESIGN.md section 14) ----
// k_learn over a worklist (csrc/dql_advance.hpp: build_worklist): wave w flies the learners worklist[64 w .. 64 w + 63] (-1: an inactive lane), all of
// them at level wave_level[w] — a scalar load — from which follow SimK::working, the level's MdpK (a.a.mdp is the array of all five) and the level's
// exploration table and freeze rules.  After that the call to learner_periods is k_learn's.
template <typename T> struct LearnLevelsArgs {
  LearnArgs<T> a;                          // a.mdp: [DQL_MAX_LEVELS]; a.sched: the learning rates (its per-level members are replaced by lv[level])
  const LevelSched DQL_CONST_AS* lv;       // [DQL_MAX_LEVELS]
  const int* worklist;                     // [64 n_waves]
  const int DQL_CONST_AS* wave_level;      // [n_waves]
  int n_waves;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_levels(LearnLevelsArgs<T> g) {
  const LearnArgs<T>& a = g.a;
  const int tid = threadIdx.x;
  const int w = (int)blockIdx.x;
  if (w >= g.n_waves) return;
  const int level = g.wave_level[w];
  if ((unsigned)level >= (unsigned)DQL_MAX_LEVELS) { if (tid == 0) a.mem.faults[0] += 1ull; return; }  // never taken unless a bug (the host builds the worklist)
  const long long l = (long long)g.worklist[(long long)w * 64 + tid];
  SimK<T> cl = a.c;
  cl.working = level;
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
  const LearnSched sc = learn_sched(a.sched.alpha_tab, a.sched.n_alpha, a.sched.alpha_min, g.lv + level);
  learner_periods<TICK, XMODE>(cl, cfgk, tc, a.mdp + level, a.mdp_run, sc, a.mem, a.sr, a.si, a.seed, l, l >= 0 && l < a.mem.n, a.j0, a.n_periods, a.mgr0, a.tick_sched, kv);
}
// an advance point: every learner takes advance_learner's step by itself (its own thread moves its own 2 x 567 cells; ordinary vector stores, nothing shared)
// -- but for the `faults` word: advance_learner's `faults[0] += 1` is a plain add that threads of all waves may make at once, as learner_periods' is.  Counts
// can be lost, a nonzero word cannot become zero, and nonzero is all that index_faults() is read for.
__global__ void k_ens_advance(LearnMem mem, AdvanceMem adv, AdvanceRule rule, int4* si, long long j, int n_cells) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= mem.n) return;
  (void)advance_learner(mem, adv, rule, si, l, j, n_cells);
}

// a launch's worklist on the host and on the device: build() regroups the live learners by level (build_worklist) or, where recipe_of is set, by (recipe,
// level) (build_worklist_recipes: then the wave_recipe column exists), or, where a slot is a team (team_slots: per_wave = 64 / E slots make a wave), the live
// teams by level (build_team_worklist); upload() copies the waves build() made.  dql_ensemble holds two (learners, and teams once team curriculum mode was
// switched on) and EnsRecipes (dql_recipes.inc) one: the capacities differ.
struct EnsWorklist {
  long long slots = 0;                                   // per_wave per wave
  int per_wave = ADV_WAVE; bool team_slots = false;
  const int* recipe_of = nullptr; int n_recipes = 0;     // host [L]; null: by level alone
  std::vector<int> list, wave_recipe, wave_level;        // host [slots], [slots / per_wave], [slots / per_wave]
  int* d_list = nullptr; int* d_wave_recipe = nullptr; int* d_wave_level = nullptr;
  void resize(long long n_slots, const int* of = nullptr, int n_of = 0, int teams_per_wave = 0) {
    slots = n_slots; recipe_of = of; n_recipes = n_of; team_slots = teams_per_wave > 0; per_wave = team_slots ? teams_per_wave : ADV_WAVE;
    list.assign((size_t)slots, 0); wave_level.assign((size_t)(slots / per_wave), 0); wave_recipe.assign(of ? (size_t)(slots / per_wave) : 0, 0);
  }
  int build(const int* frozen, const int* level, long long n, unsigned long long* faults) {  // -> the waves to fly
    if (team_slots) return build_team_worklist(frozen, level, n, per_wave, list.data(), wave_level.data(), slots, faults);
    return recipe_of ? build_worklist_recipes(frozen, level, recipe_of, n, n_recipes, list.data(), wave_recipe.data(), wave_level.data(), slots, faults)
                     : build_worklist(frozen, level, n, list.data(), wave_level.data(), slots, faults);
  }
  int upload(int n_waves) const {
    HIP_TRY(hipMemcpy(d_list, list.data(), (size_t)n_waves * per_wave * sizeof(int), hipMemcpyHostToDevice));
    if (recipe_of) HIP_TRY(hipMemcpy(d_wave_recipe, wave_recipe.data(), (size_t)n_waves * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_wave_level, wave_level.data(), (size_t)n_waves * sizeof(int), hipMemcpyHostToDevice));
    return DQL_OK;
  }
};

// ---- ensembles of sequential learners (DESIGN.md section 12) ----
struct dql_ensemble {
  dql_config cfg;
  int device = 0;
  long long n = 0;
  unsigned long long seed = 0;
  long long j = 0;  // the ensemble's period index (period 0 is the reset period)
  DevOwned dev;     // every device allocation below, the replaceable schedule tables included
  void* sr = nullptr; int4* si = nullptr; void* mdpk = nullptr;
  LearnMem mem{};
  LearnSched sched{};
  double* alpha_tab = nullptr; uint32_t* eps_tab = nullptr;
  long long* d_mgr0 = nullptr; int* d_sched = nullptr;  // [LEARN_MAX_PERIODS]
  double last_ms = -1.0;
  // per-learner curriculum levels (DESIGN.md section 14); advance_every = 0: the mode is off
  AdvanceMem adv{};
  AdvanceRule rule{};
  int advance_every = 0;
  void* mdpk5 = nullptr;                                      // [DQL_MAX_LEVELS] MdpK<T>, entry k with working = k
  LevelSched* d_lv = nullptr; LevelSched h_lv[DQL_MAX_LEVELS]{}; bool have_lv[DQL_MAX_LEVELS]{};
  EnsWorklist wl;                                             // by level (capacity: worklist_capacity)
  long long n_launches = 0, launched_periods = 0, launched_wave_periods = 0;  // since creation (dql_diag_ensemble_launches)
  struct EnsRecipes* rcp = nullptr;  // per-learner recipes (DESIGN.md section 16, dql_recipes.inc); null: none are installed and every call is as it was
  // teams (DESIGN.md section 17, dql_teams.inc): learner l owns envs l E .. l E + E - 1 of the n_envs = n E the state arrays hold; teams: dql_ensemble_run flies k_learn_team
  int envs_per_learner = 1; long long n_envs = 0; bool teams = false;
  // n-step targets (DESIGN.md section 22, dql_nstep.inc); nstep = 0: dql_ensemble_run flies k_learn and the arrays below are never read.  The learners' pending
  // windows between launches: key / val [DQL_NSTEP_MAX][n], len [n], allocated by the first dql_ensemble_set_nstep with n >= 1 — or, with recipes installed, by the
  // first dql_ensemble_set_recipe_nstep with n >= 1 (section 23, dql_nstep_recipes.inc: n is then a recipe's, EnsRecipes::nstep, and `nstep` here stays 0)
  int nstep = 0;
  uint16_t* ns_key = nullptr; double* ns_val = nullptr; int* ns_len = nullptr;
  // a team ensemble's n-step targets (DESIGN.md section 24, dql_team_nstep.inc); team_nstep = 0: dql_ensemble_run flies k_learn_team and the arrays below are never
  // read.  One pending window PER ENV between launches: key / val [DQL_NSTEP_MAX][n_envs], len [n_envs], allocated by the first dql_ensemble_set_team_nstep with
  // n >= 1.  Members of their own: nstep and ns_* above stay 0 / null on a team ensemble, so dql_ensemble_get_nstep answers as it always did
  int team_nstep = 0;
  uint16_t* tn_key = nullptr; double* tn_val = nullptr; int* tn_len = nullptr;
  // team curriculum mode (DESIGN.md section 29, dql_team_levels.inc); team_every = 0: the mode is off.  A member of its own: advance_every above stays 0 on an
  // ensemble in this mode, so every condition on it answers as it always did.  The rule is `rule` above (the two modes refuse each other), the order of
  // transfer and level change is RecipeRule's; the worklist of teams is allocated by the first dql_ensemble_set_team_curriculum that switches the mode on
  int team_every = 0, team_order = RCP_ORDER_REFERENCE;
  EnsWorklist twl;                                            // by level, 64 / E team slots per wave (capacity: team_worklist_capacity)
  // the refinement (DESIGN.md section 34, dql_refined.inc); refine_feature = -1: none, and every call is as it was.  Installed once by dql_ensemble_set_refinement:
  // the learners' tables are then rq_a / rq_b / rq_count [n][2][DQL_N_CELLS] (mem.qa / qb / count stay allocated and are never read again), d_cut [DQL_N_STATES]
  // is the cut on the device and h_cut its host copy, d_half [n] the byte a learner carries across launches (RefinedMem::half)
  int refine_feature = -1;
  double *rq_a = nullptr, *rq_b = nullptr, *rq_count = nullptr, *d_cut = nullptr;
  uint8_t* d_half = nullptr;
  double h_cut[DQL_N_STATES]{};
};
// which of the ten learner kernels a launch flies (ens_kernel_of decides, ens_fly switches)
enum EnsKernel { ENS_K_LEARN, ENS_K_TEAM, ENS_K_TEAM_NSTEP, ENS_K_NSTEP, ENS_K_LEVELS, ENS_K_RECIPES, ENS_K_RECIPES_NSTEP, ENS_K_TEAM_LEVELS, ENS_K_TEAM_LEVELS_NSTEP,
                 ENS_K_LEARN_REFINED };
// of dql_recipes.inc: the installed recipes let go, the rule learner l advances by, the smallest last_level of the populated recipes, whether a recipe that has
// a member has n >= 1, the device copy of the recipes' n (null until one was set), dql_ensemble_run's part with recipes installed
static void ens_recipes_release(dql_ensemble* x);
static const AdvanceRule& ens_rule_of(const dql_ensemble* x, size_t l);
static int ens_recipes_min_last_level(const dql_ensemble* x);
static bool ens_recipes_any_nstep(const dql_ensemble* x);
static const int* ens_recipes_nstep_table(const dql_ensemble* x);
static int ens_run_recipes(dql_ensemble* x, int64_t periods, EnsKernel kern);
static int ens_run_team_levels(dql_ensemble* x, int64_t periods, EnsKernel kern);  // of dql_team_levels.inc: dql_ensemble_run's part in team curriculum mode
// each later fragment's argument filler, next to its kernel: the kernel's arguments from the ensemble, and the launch of k periods on n_waves waves
template <typename T> static void launch_learn_recipes(dql_ensemble* x, int k, int n_waves);        // dql_recipes.inc
template <typename T> static void launch_learn_team(dql_ensemble* x, int k, int n_waves);           // dql_teams.inc
template <typename T> static void launch_learn_nstep(dql_ensemble* x, int k, int n_waves);          // dql_nstep.inc
template <typename T> static void launch_learn_team_nstep(dql_ensemble* x, int k, int n_waves);     // dql_team_nstep.inc
template <typename T> static void launch_learn_recipes_nstep(dql_ensemble* x, int k, int n_waves);  // dql_nstep_recipes.inc
template <typename T> static void launch_learn_team_levels(dql_ensemble* x, int k, int n_waves);        // dql_team_levels.inc
template <typename T> static void launch_learn_team_levels_nstep(dql_ensemble* x, int k, int n_waves);  // dql_team_levels.inc
template <typename T> static void launch_learn_refined(dql_ensemble* x, int k, int n_waves);            // dql_refined.inc
#define ENS_NSTEP_REFUSED(who) "" who ": n-step targets (dql_ensemble_set_nstep with n >= 1) are for the plain mode, where every learner flies the config's level; set n = 0 first; nothing was changed and nothing was launched"
#define ENS_TEAM_NSTEP_REFUSED(who) "" who ": team n-step targets (dql_ensemble_set_team_nstep with n >= 1) are for the barrier mode, where every learner flies the config's level: a team ensemble of one env per learner has no per-learner curriculum and no recipes while they are on; set n = 0 first; nothing was changed and nothing was launched"
#define ENS_TEAMS_REFUSED(who) "" who ": an ensemble with more than one env per learner flies the barrier mode only (teams have no per-learner curriculum and no recipes); nothing was changed and nothing was launched"
#define ENS_TEAM_LEVELS_REFUSED(who) "" who ": team curriculum mode (dql_ensemble_set_team_curriculum) is on: a team ensemble of one env per learner flies one of the two curriculum modes at a time; switch it off first (advance_every = 0); nothing was changed and nothing was launched"
// a refined ensemble (dql_ensemble_set_refinement) refuses every call that reads or writes the plain tables or installs another mode; `instead`: what to call
#define ENS_REFINED_REFUSED(x, who, instead) do { if ((x)->refine_feature >= 0) return fail(DQL_EINVAL, "" who ": the ensemble has a refinement (dql_ensemble_set_refinement), its tables are [n][2][DQL_N_CELLS] and its learners fly the plain mode only; " instead "; nothing was changed and nothing was launched"); } while (0)
#define ENS_REFINED_GREEDY "use dql_ensemble_score_refined, or fetch the tables with dql_ensemble_get_refined_tables and hand one half to the plain call"
#define ENS_REFINED_MODES "use dql_ensemble_set_schedules, dql_ensemble_set_level, dql_ensemble_run and dql_ensemble_transfer level by level"
#define CHECK_ENS(e) do { if (!(e)) return fail(DQL_EINVAL, "null ensemble"); } while (0)
// the tables of learners [first, first + count) where they live, for the dql_ensemble_* twins of the greedy family (TableSets of dql_greedy.inc; count >= 1 is the
// twin's own check): the ensemble's device becomes the current one, nothing is copied
static int tables_of_slice(const char* who, dql_ensemble* x, int64_t first, int64_t count, TableSets& q) {
  if (x->refine_feature >= 0)
    return fail(DQL_EINVAL, std::string(who) + ": the ensemble has a refinement (dql_ensemble_set_refinement), its tables are [n][2][DQL_N_CELLS] and its learners fly the plain mode only; " ENS_REFINED_GREEDY "; nothing was changed and nothing was launched");
  if (first < 0 || first > x->n || count > x->n - first)
    return fail(DQL_EINVAL, std::string(who) + ": the slice [first, first + count) must lie inside [0, n_learners); nothing was launched");
  HIP_TRY(hipSetDevice(x->device));
  q.qa = x->mem.qa + (size_t)first * DQL_N_CELLS; q.qb = x->mem.qb + (size_t)first * DQL_N_CELLS;
  return DQL_OK;
}
static void ens_free(dql_ensemble* x) {
  ens_recipes_release(x);
  x->dev.free_all();
  delete x;
}
// ---- shared host helpers of the learner family (DESIGN.md section 15) ----
// `count` elements of one device array -> host
template <typename T> static int ens_fetch(const T* d, size_t count, std::vector<T>& h) {
  h.resize(count);
  HIP_TRY(hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost));
  return DQL_OK;
}
// all of these device arrays, zeroed, or none of them: DQL_OK; DQL_ENOMEM (a hipMalloc failed) or DQL_EHIP (a hipMemset did) with every pointer null again.
// The caller says the sentence.
struct DevWant { void** p; size_t bytes; };
static int ens_alloc_zeroed(DevOwned& dev, std::initializer_list<DevWant> want) {
  int rc = DQL_OK;
  for (const DevWant& w : want) {
    if (rc) break;
    if (dev.alloc(w.p, w.bytes) != hipSuccess) rc = DQL_ENOMEM;
    else if (hipMemset(*w.p, 0, w.bytes) != hipSuccess) rc = DQL_EHIP;
  }
  if (rc) for (const DevWant& w : want) { (void)dev.release(*w.p); *w.p = nullptr; }
  return rc;
}
// DQL_ESTATE with the sentence while a learner l with member(l) has entries in its pending window (no window arrays: nobody has)
template <typename F> static int ens_windows_empty(dql_ensemble* x, F member, const char* sentence) {
  if (!x->ns_len) return DQL_OK;
  std::vector<int> len;
  const int rc = ens_fetch(x->ns_len, (size_t)x->n, len); if (rc) return rc;
  for (size_t l = 0; l < len.size(); ++l) if (len[l] != 0 && member(l)) return fail(DQL_ESTATE, sentence);
  return DQL_OK;
}
// what the host found wrong while it built a worklist, added to the device's `faults` word
static int ens_add_faults(dql_ensemble* x, unsigned long long more) {
  if (!more) return DQL_OK;
  unsigned long long v = 0;
  HIP_TRY(hipMemcpy(&v, x->mem.faults, sizeof(v), hipMemcpyDeviceToHost));
  v += more;
  HIP_TRY(hipMemcpy(x->mem.faults, &v, sizeof(v), hipMemcpyHostToDevice));
  return DQL_OK;
}

// every learner to level k: the per-level history from level k on is cleared, level k is entered at the present period index
static int ens_set_levels(dql_ensemble* x, int k) {
  const size_t n = (size_t)x->n;
  if (x->j == 0) HIP_TRY(hipMemset(x->adv.entered_period, 0xff, (size_t)DQL_MAX_LEVELS * n * sizeof(long long)));  // nothing was flown: no level below k was ever entered
  std::vector<int> lv(n, k);
  HIP_TRY(hipMemcpy(x->adv.level, lv.data(), n * sizeof(int), hipMemcpyHostToDevice));
  const size_t from = (size_t)k * n, rest = (size_t)(DQL_MAX_LEVELS - k) * n;
  HIP_TRY(hipMemset(x->adv.promoted_at + from, 0xff, rest * sizeof(int)));
  HIP_TRY(hipMemset(x->adv.episodes_at + from, 0, rest * sizeof(int)));
  HIP_TRY(hipMemset(x->adv.entered_period + from, 0xff, rest * sizeof(long long)));
  std::vector<long long> at(n, x->j);
  HIP_TRY(hipMemcpy(x->adv.entered_period + from, at.data(), n * sizeof(long long), hipMemcpyHostToDevice));
  return DQL_OK;
}
// the five levels' MdpK (they differ in `working` only), read by k_learn_levels at the wave's level
static int ens_upload_mdpk5(dql_ensemble* x) {
  dql_config c = x->cfg;
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) {
    c.working_curriculum_step = k;
    const int rc = upload_mdpk(c, (char*)x->mdpk5 + (size_t)k * mdpk_bytes(c.dtype)); if (rc) return rc;
  }
  return DQL_OK;
}
// per-level episode counts, windows, promotion records and frozen flags back to "just started"
static int ens_rearm(dql_ensemble* x) {
  const size_t n = (size_t)x->n;
  HIP_TRY(hipMemset(x->mem.level_episodes, 0, n * sizeof(int)));
  HIP_TRY(hipMemset(x->mem.win_count, 0, n * sizeof(int)));
  HIP_TRY(hipMemset(x->mem.win_bits, 0, 2 * n * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(x->mem.promoted, 0xff, n * sizeof(int)));
  HIP_TRY(hipMemset(x->mem.frozen, 0, n * sizeof(int)));
  return DQL_OK;
}
// what k_learn and k_learn_levels share: mdp = the config's MdpK or the five levels'
template <typename T> static LearnArgs<T> make_learn_args(dql_ensemble* x, const void* mdp, int n_periods) {
  LearnArgs<T> a;
  a.c = make_simk<T>(x->cfg);
  a.mdp = (const MdpK<T> DQL_CONST_AS*)mdp;
  a.mdp_run = MdpRun<T>{x->cfg.gamma, (T)(x->cfg.t_max * x->cfg.f_ag), x->cfg.goal_logic};
  a.sched = x->sched; a.mem = x->mem;
  a.sr = (Quad<T>*)x->sr; a.si = x->si;
  a.mgr0 = (const long long DQL_CONST_AS*)x->d_mgr0; a.tick_sched = (const int DQL_CONST_AS*)x->d_sched;
  a.seed = x->seed; a.j0 = x->j; a.n_periods = n_periods;
  return a;
}
template <typename T> static void launch_learn(dql_ensemble* x, int k, int n_waves) {
  hipLaunchKernelGGL((k_learn<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, make_learn_args<T>(x, x->mdpk, k));
}
template <typename T> static void launch_learn_levels(dql_ensemble* x, int k, int n_waves) {
  LearnLevelsArgs<T> g;
  g.a = make_learn_args<T>(x, x->mdpk5, k);
  g.lv = (const LevelSched DQL_CONST_AS*)x->d_lv; g.worklist = x->wl.d_list; g.wave_level = (const int DQL_CONST_AS*)x->wl.d_wave_level; g.n_waves = n_waves;
  hipLaunchKernelGGL((k_learn_levels<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, g);
}
// The one place that says which kernel flies.  by_level: the launch goes through a worklist (curriculum mode, with or without recipes); with one env per learner
// a team ensemble in curriculum mode flies k_learn_levels, the same learner; n >= 1 is refused on team ensembles and in curriculum mode, and with recipes
// installed n is a recipe's: one recipe that has a member and n >= 1 makes every launch k_learn_recipes_nstep's.  A team ensemble with team_nstep >= 1 flies
// k_learn_team_nstep in the barrier mode; team_nstep >= 1 and curriculum mode (possible with one env per learner only) refuse each other, so by_level never
// meets it.  Team curriculum mode (team_every, which refuses that curriculum mode and recipes) flies the two team kernels over the worklist of teams.
static EnsKernel ens_kernel_of(const dql_ensemble* x, bool by_level) {
  if (x->team_every) return x->team_nstep ? ENS_K_TEAM_LEVELS_NSTEP : ENS_K_TEAM_LEVELS;
  if (by_level) return !x->rcp ? ENS_K_LEVELS : ens_recipes_any_nstep(x) ? ENS_K_RECIPES_NSTEP : ENS_K_RECIPES;
  if (x->refine_feature >= 0) return ENS_K_LEARN_REFINED;  // (a refinement refuses teams, n-step targets and both curriculum modes, and they refuse it)
  return x->teams ? (x->team_nstep ? ENS_K_TEAM_NSTEP : ENS_K_TEAM) : x->nstep ? ENS_K_NSTEP : ENS_K_LEARN;
}
// The one launch path of the learners: k periods from period x->j on n_waves waves.  The tick schedule, the kernel, its completion, the launch accounting
// (dql_diag_ensemble_launches).
static int ens_fly(dql_ensemble* x, EnsKernel kern, int k, int n_waves) {
  const bool windows = kern == ENS_K_NSTEP || kern == ENS_K_RECIPES_NSTEP;
  if (windows && (!x->ns_key || !x->ns_val || !x->ns_len || (kern == ENS_K_RECIPES_NSTEP && !ens_recipes_nstep_table(x))))  // (never taken unless a bug)
    return fail(DQL_ESTATE, kern == ENS_K_NSTEP ? "dql_ensemble_run: n-step targets are on but the pending windows were never allocated; nothing was launched"
                                                : "dql_ensemble_run: a recipe has n-step targets but the pending windows were never allocated; nothing was launched");
  if ((kern == ENS_K_TEAM_NSTEP || kern == ENS_K_TEAM_LEVELS_NSTEP) && (!x->tn_key || !x->tn_val || !x->tn_len))  // (never taken unless a bug)
    return fail(DQL_ESTATE, "dql_ensemble_run: team n-step targets are on but the envs' pending windows were never allocated; nothing was launched");
  const int rc = upload_schedule(x->cfg, x->j, k, x->d_mgr0, x->d_sched); if (rc) return rc;  // (synchronous: the previous launch has read its schedule)
  by_dtype(x->cfg.dtype, [&](auto t) {
    using T = decltype(t);
    switch (kern) {
      case ENS_K_LEARN: launch_learn<T>(x, k, n_waves); break;
      case ENS_K_TEAM: launch_learn_team<T>(x, k, n_waves); break;
      case ENS_K_TEAM_NSTEP: launch_learn_team_nstep<T>(x, k, n_waves); break;
      case ENS_K_NSTEP: launch_learn_nstep<T>(x, k, n_waves); break;
      case ENS_K_LEVELS: launch_learn_levels<T>(x, k, n_waves); break;
      case ENS_K_RECIPES: launch_learn_recipes<T>(x, k, n_waves); break;
      case ENS_K_RECIPES_NSTEP: launch_learn_recipes_nstep<T>(x, k, n_waves); break;
      case ENS_K_TEAM_LEVELS: launch_learn_team_levels<T>(x, k, n_waves); break;
      case ENS_K_TEAM_LEVELS_NSTEP: launch_learn_team_levels_nstep<T>(x, k, n_waves); break;
      case ENS_K_LEARN_REFINED: launch_learn_refined<T>(x, k, n_waves); break;
    }
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  x->n_launches += 1; x->launched_periods += k; x->launched_wave_periods += (long long)n_waves * k;
  return DQL_OK;
}
// every rate of a table in [0, 1], or the sentence
static int ens_check_rates(const double* tab, int32_t n, const std::string& sentence) {
  for (int i = 0; i < n; ++i) if (!(tab[i] >= 0.0 && tab[i] <= 1.0)) return fail(DQL_EINVAL, sentence);
  return DQL_OK;
}
// host words in a new device table the ensemble owns
template <typename D> static int ens_upload_table(dql_ensemble* x, const D* h, size_t n, D** d_out) {
  if (x->dev.alloc((void**)d_out, n * sizeof(D)) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc failed");
  if (hipMemcpy(*d_out, h, n * sizeof(D), hipMemcpyHostToDevice) != hipSuccess) { (void)x->dev.release(*d_out); *d_out = nullptr; return fail(DQL_EHIP, "hipMemcpy failed"); }
  return DQL_OK;
}
// What the three schedule calls share: the promotion rule and the rate tables checked in the order dql_ensemble_set_schedules always had (it alone passes
// learning rates), then (the device idle) the exploration rates as eps_threshold words in a new device table.  who: the call's name, the prefix of its
// sentences; tail: their ending ("" or "; nothing was changed").
static int ens_check_upload_rule(dql_ensemble* x, const std::string& who, const char* tail, const double* alpha, int32_t n_alpha, const double* eps, int32_t n_eps, int32_t window,
                                 int32_t min_successes, int32_t max_episodes, uint32_t** d_eps) {
  if (window < 1 || window > DQL_ENSEMBLE_MAX_WINDOW) return fail(DQL_EINVAL, who + ": the promotion window must be in 1..128 (DQL_ENSEMBLE_MAX_WINDOW)" + tail);
  if (min_successes < 1 || max_episodes < 1) return fail(DQL_EINVAL, who + ": min_successes and max_episodes must be positive" + tail);
  int rc = ens_check_rates(alpha, n_alpha, who + ": learning rates must be in [0, 1]" + tail); if (rc) return rc;
  rc = ens_check_rates(eps, n_eps, who + ": exploration rates must be in [0, 1]" + tail); if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> thr((size_t)n_eps);
  for (int i = 0; i < n_eps; ++i) thr[(size_t)i] = eps_threshold(eps[i]);
  return ens_upload_table(x, thr.data(), thr.size(), d_eps);
}
// frozen, level and promoted of every learner -> host; the learners that are not finished for good
static int ens_fetch_levels(dql_ensemble* x, std::vector<int>& frozen, std::vector<int>& level, std::vector<int>& promoted, int64_t* unfinished) {
  const size_t n = (size_t)x->n;
  int rc = ens_fetch(x->mem.frozen, n, frozen);
  if (!rc) rc = ens_fetch(x->adv.level, n, level);
  if (!rc) rc = ens_fetch(x->mem.promoted, n, promoted);
  if (rc) return rc;
  int64_t u = 0;
  for (size_t l = 0; l < n; ++l) u += learner_finished(frozen[l], level[l], promoted[l], ens_rule_of(x, l)) ? 0 : 1;
  *unfinished = u;
  return DQL_OK;
}
// a learner on `level` has the schedules it will fly by: the level it stands on is flown whatever last_level says, then every level on its way up to last_level
static bool ens_way_up_scheduled(const bool* have_lv, int level, int last_level) {
  bool ok = level >= 0 && level < DQL_MAX_LEVELS && have_lv[level];
  for (int k = level + 1; ok && k <= last_level && k < DQL_MAX_LEVELS; ++k) ok = have_lv[k];
  return ok;
}
// The one advancing run loop: dql_ensemble_run in curriculum mode, with and without recipes, and in team curriculum mode.  The launches are cut at the multiples of advance_every; at such a
// period index j, before period j is flown, every learner takes its advance step; each launch flies the live learners regrouped by the worklist.  What the
// modes differ in is passed in: complete(l, level) with the sentence that refuses the call where it fails, the advance kernel's launch, the worklist, the kernel.
template <typename Complete, typename Advance>
static int ens_run_advancing(dql_ensemble* x, int64_t periods, EnsKernel kern, EnsWorklist& wl, Complete complete, const char* incomplete, Advance launch_advance) {
  std::vector<int> frozen, level, promoted;
  int64_t unfinished = 0;
  int rc = ens_fetch_levels(x, frozen, level, promoted, &unfinished); if (rc) return rc;
  for (size_t l = 0; l < (size_t)x->n; ++l) if (!complete(l, level[l])) return fail(DQL_EINVAL, incomplete);
  EvTimer timer;
  rc = timer.start(); if (rc) return rc;
  const long long E = x->team_every ? x->team_every : x->advance_every;
  long long left = periods;
  while (left > 0) {
    if (x->j % E == 0) {  // an advance point
      launch_advance();
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
    }
    rc = ens_fetch_levels(x, frozen, level, promoted, &unfinished); if (rc) return rc;
    if (unfinished == 0) { x->j += left; break; }  // nothing left to fly or to advance, now or later (the period index still advances by `periods`)
    const long long to_point = E - x->j % E;
    const int k = (int)(left < to_point ? left : to_point);  // <= advance_every <= LEARN_MAX_PERIODS
    unsigned long long wl_faults = 0ull;
    const int n_waves = wl.build(frozen.data(), level.data(), x->n, &wl_faults);
    rc = ens_add_faults(x, wl_faults); if (rc) return rc;
    if (n_waves > 0) {  // (nobody live: everyone unfinished waits for the next advance point)
      rc = wl.upload(n_waves); if (rc) return rc;
      rc = ens_fly(x, kern, k, n_waves); if (rc) return rc;
    }
    x->j += k; left -= k;
  }
  return timer.stop_ms(&x->last_ms);
}
static int ens_run_levels(dql_ensemble* x, int64_t periods, EnsKernel kern) {
  return ens_run_advancing(x, periods, kern, x->wl, [&](size_t, int level) { return ens_way_up_scheduled(x->have_lv, level, x->rule.last_level); },
                           "dql_ensemble_run: curriculum mode needs dql_ensemble_set_level_schedules for every level from the learners' up to last_level; nothing was launched", [&] {
                             hipLaunchKernelGGL(k_ens_advance, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, 0, x->mem, x->adv, x->rule, x->si, (long long)x->j, (int)DQL_CELLS_PER_LEVEL);
                           });
}
extern "C" {
// what dql_ensemble_create and dql_ensemble_create_teams (dql_teams.inc) share once their arguments are checked: n_learners learners with envs_per_learner envs each
static int ens_create(const dql_config* cfg, int device, int64_t n_learners, int envs_per_learner, bool teams, uint64_t seed, int32_t log_capacity, dql_ensemble** out) {
  int rc = DQL_OK;
  OP_PROLOGUE(device)
  dql_ensemble* x = new dql_ensemble;
  x->cfg = *cfg; x->device = device; x->n = n_learners; x->seed = seed;
  x->envs_per_learner = envs_per_learner; x->n_envs = n_learners * envs_per_learner; x->teams = teams;
  const size_t n = (size_t)n_learners, n_envs = (size_t)x->n_envs, mdpk_size = mdpk_bytes(cfg->dtype), real = by_dtype(cfg->dtype, [](auto t) { return sizeof(t); });
  const size_t TB = n * DQL_N_CELLS * sizeof(double), I = n * sizeof(int), U = n * sizeof(unsigned long long), LOG = n * (size_t)(log_capacity ? log_capacity : 1);
  const size_t H = (size_t)DQL_MAX_LEVELS * n;  // the per-level history
  LearnMem& m = x->mem; AdvanceMem& a = x->adv;
  x->wl.resize(worklist_capacity(n_learners));
  const size_t waves = (size_t)(x->wl.slots / ADV_WAVE);
  rc = ens_alloc_zeroed(x->dev, {
      {&x->sr, (size_t)NQ_REAL * n_envs * 4 * real}, {(void**)&x->si, n_envs * sizeof(int4)}, {&x->mdpk, mdpk_size},
      {(void**)&m.qa, TB}, {(void**)&m.qb, TB}, {(void**)&m.count, TB}, {(void**)&m.decisions, U}, {(void**)&m.by_code, (size_t)DQL_N_CHECK_CODES * U},
      {(void**)&m.episodes, I}, {(void**)&m.successes, I}, {(void**)&m.level_episodes, I}, {(void**)&m.win_count, I}, {(void**)&m.win_bits, 2 * U},
      {(void**)&m.promoted, I}, {(void**)&m.frozen, I}, {(void**)&m.log_code, LOG}, {(void**)&m.log_len, LOG * sizeof(uint16_t)}, {(void**)&m.log_n, I},
      {(void**)&m.faults, sizeof(unsigned long long)},
      {(void**)&x->d_mgr0, (size_t)LEARN_MAX_PERIODS * sizeof(long long)}, {(void**)&x->d_sched, (size_t)LEARN_MAX_PERIODS * sizeof(int)},
      {(void**)&a.level, I}, {(void**)&a.promoted_at, H * sizeof(int)}, {(void**)&a.episodes_at, H * sizeof(int)}, {(void**)&a.entered_period, H * sizeof(long long)},
      {&x->mdpk5, (size_t)DQL_MAX_LEVELS * mdpk_size}, {(void**)&x->d_lv, (size_t)DQL_MAX_LEVELS * sizeof(LevelSched)},
      {(void**)&x->wl.d_list, (size_t)x->wl.slots * sizeof(int)}, {(void**)&x->wl.d_wave_level, waves * sizeof(int)}});
  if (rc) { ens_free(x); return fail(rc, rc == DQL_ENOMEM ? "hipMalloc failed" : "hipMemset failed"); }
  x->mem.n = n_learners; x->mem.log_cap = log_capacity;
  rc = upload_mdpk(x->cfg, x->mdpk);
  if (!rc) rc = ens_upload_mdpk5(x);
  if (!rc) rc = ens_set_levels(x, 0);  // the whole history cleared ...
  if (!rc) rc = ens_set_levels(x, cfg->working_curriculum_step);  // ... and the config's level entered at period 0
  if (!rc) rc = ens_rearm(x);
  if (!rc) rc = by_dtype(cfg->dtype, [&](auto t) { return launch_init<decltype(t)>(x->cfg, x->sr, x->si, x->n_envs, x->n_envs, x->seed, 0, nullptr); });
  // default schedules: the plateau learning rate, no exploration, the reference's window (100 episodes, 97 successes) and no episode budget
  const double a0 = cfg->alpha_min; const double e0 = 0.0;
  if (!rc) rc = dql_ensemble_set_schedules(x, &a0, 1, &e0, 1, 100, 97, INT32_MAX);
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(DQL_EHIP, "hipDeviceSynchronize failed");
  if (rc) { ens_free(x); return rc; }
  *out = x;
  return DQL_OK;
}
int dql_ensemble_create(const dql_config* cfg, int device, int64_t n_learners, uint64_t seed, int32_t log_capacity, dql_ensemble** out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (!out) return fail(DQL_EINVAL, "dql_ensemble_create: null pointer; nothing was launched");
  if (cfg->two_axis) return fail(DQL_EINVAL, "dql_ensemble_create: two-axis configs are refused (the reference's learner is x-only); nothing was launched");
  if (cfg->trajectory == DQL_TRAJ_EIGHT) return fail(DQL_EINVAL, "dql_ensemble_create: the figure-eight trajectory is refused (the reference's learner is x-only); nothing was launched");
  if (n_learners < 1 || n_learners > DQL_ENSEMBLE_MAX_LEARNERS) return fail(DQL_EINVAL, "dql_ensemble_create: n_learners must be in 1..2^20 (DQL_ENSEMBLE_MAX_LEARNERS); nothing was launched");
  if (log_capacity < 0 || log_capacity > DQL_ENSEMBLE_MAX_LOG) return fail(DQL_EINVAL, "dql_ensemble_create: log_capacity must be in 0..2^20 (DQL_ENSEMBLE_MAX_LOG); nothing was launched");
  return ens_create(cfg, device, n_learners, 1, false, seed, log_capacity, out);
}
int dql_ensemble_destroy(dql_ensemble* x) {
  if (!x) return DQL_OK;
  (void)hipSetDevice(x->device);
  (void)hipDeviceSynchronize();
  ens_free(x);
  return DQL_OK;
}
int dql_ensemble_n_learners(dql_ensemble* x, int64_t* n) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "null pointer");
  *n = x->n;
  return DQL_OK;
}
int dql_ensemble_set_schedules(dql_ensemble* x, const double* alpha, int32_t n_alpha, const double* eps, int32_t n_eps, int32_t window, int32_t min_successes,
                               int32_t max_episodes) {
  CHECK_ENS(x);
  if (!alpha || !eps) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: null table");
  if (n_alpha < 1 || n_alpha > (1 << 22) || n_eps < 1 || n_eps > (1 << 22)) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: table lengths must be in 1..2^22");
  double* d_a = nullptr; uint32_t* d_e = nullptr;
  int rc = ens_check_upload_rule(x, "dql_ensemble_set_schedules", "", alpha, n_alpha, eps, n_eps, window, min_successes, max_episodes, &d_e); if (rc) return rc;
  rc = ens_upload_table(x, alpha, (size_t)n_alpha, &d_a); if (rc) { (void)x->dev.release(d_e); return rc; }
  (void)x->dev.release(x->alpha_tab); (void)x->dev.release(x->eps_tab);  // the tables they replace
  x->alpha_tab = d_a; x->eps_tab = d_e;
  x->sched = LearnSched{d_a, n_alpha, x->cfg.alpha_min, d_e, n_eps, window, min_successes, max_episodes};
  return DQL_OK;
}
int dql_ensemble_rearm(dql_ensemble* x) {
  CHECK_ENS(x);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  return ens_rearm(x);
}
int dql_ensemble_set_level(dql_ensemble* x, int32_t k) {
  CHECK_ENS(x);
  if (k < 0 || k >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_level: curriculum step must be in 0..4");
  if (x->rcp && k > ens_recipes_min_last_level(x))
    return fail(DQL_EINVAL, "dql_ensemble_set_level: with recipes installed the level must not exceed the smallest last_level of the recipes that have a member; nothing was changed");
  if (!x->rcp && x->advance_every && k > x->rule.last_level)
    return fail(DQL_EINVAL, "dql_ensemble_set_level: in curriculum mode the level must not exceed last_level (raise it with dql_ensemble_set_curriculum first); nothing was changed");
  if (x->team_every && k > x->rule.last_level)
    return fail(DQL_EINVAL, "dql_ensemble_set_level: in team curriculum mode the level must not exceed last_level (raise it with dql_ensemble_set_team_curriculum first); nothing was changed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  x->cfg.working_curriculum_step = k;
  int rc = upload_mdpk(x->cfg, x->mdpk); if (rc) return rc;
  hipLaunchKernelGGL(k_mark_reset, dim3((unsigned)((x->n_envs + 255) / 256)), dim3(256), 0, 0, x->si, (const uint8_t*)nullptr, (long long)x->n_envs);  // every env re-enters through reset
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  rc = ens_set_levels(x, k); if (rc) return rc;
  if (x->ns_len) HIP_TRY(hipMemset(x->ns_len, 0, (size_t)x->n * sizeof(int)));  // every env re-enters through reset: the pending windows belong to episodes that are gone
  if (x->tn_len) HIP_TRY(hipMemset(x->tn_len, 0, (size_t)x->n_envs * sizeof(int)));  // ... and so do the team envs' (section 24)
  return ens_rearm(x);
}
int dql_ensemble_n_live(dql_ensemble* x, int64_t* n_live) {
  CHECK_ENS(x);
  if (!n_live) return fail(DQL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(x->device));
  std::vector<int> h;
  const int rc = ens_fetch(x->mem.frozen, (size_t)x->n, h); if (rc) return rc;
  int64_t live = 0;
  for (int v : h) live += v ? 0 : 1;
  *n_live = live;
  return DQL_OK;
}
int dql_ensemble_run(dql_ensemble* x, int64_t periods) {
  CHECK_ENS(x);
  if (periods < 1 || periods > (1ll << 40)) return fail(DQL_EINVAL, "dql_ensemble_run: periods must be in 1..2^40; nothing was launched");
  HIP_TRY(hipSetDevice(x->device));
  const EnsKernel kern = ens_kernel_of(x, x->rcp || x->advance_every);
  if (x->team_every) return ens_run_team_levels(x, periods, kern);
  if (x->rcp) return ens_run_recipes(x, periods, kern);
  if (x->advance_every) return ens_run_levels(x, periods, kern);
  int rc = DQL_OK;
  EvTimer timer;
  rc = timer.start(); if (rc) return rc;
  long long left = periods;
  while (left > 0) {
    const int k = (int)(left < LEARN_MAX_PERIODS ? left : LEARN_MAX_PERIODS);
    if (left != periods) {  // between the launches of a long run: nothing left to fly ends it (the period index still advances by `periods`)
      int64_t live = 0;
      rc = dql_ensemble_n_live(x, &live); if (rc) return rc;
      if (live == 0) { x->j += left; break; }
    }
    rc = ens_fly(x, kern, k, (int)((x->n_envs + 63) / 64)); if (rc) return rc;
    x->j += k; left -= k;
  }
  return timer.stop_ms(&x->last_ms);
}
// ---- per-learner curriculum levels (DESIGN.md section 14) ----
int dql_ensemble_set_curriculum(dql_ensemble* x, int32_t last_level, int32_t advance_every, const double* ratios, int32_t advance_exhausted) {
  CHECK_ENS(x);
  ENS_REFINED_REFUSED(x, "dql_ensemble_set_curriculum", ENS_REFINED_MODES);
  if (x->envs_per_learner > 1) return fail(DQL_EINVAL, ENS_TEAMS_REFUSED("dql_ensemble_set_curriculum"));
  if (x->team_every) return fail(DQL_EINVAL, ENS_TEAM_LEVELS_REFUSED("dql_ensemble_set_curriculum"));
  if (advance_every < 0 || advance_every > ADV_MAX_EVERY) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: advance_every must be in 0..4096 (0 turns the mode off); nothing was changed");
  if (advance_every == 0 && x->rcp)
    return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: the mode cannot be switched off (advance_every = 0) while recipes are installed; uninstall them first (dql_ensemble_set_recipes with n_recipes = 0); nothing was changed");
  if (advance_every == 0) {
    // the plain launch flies everyone at the config's level: switching off is refused while a learner stands on another one (dql_ensemble_set_level first)
    if (x->advance_every) {
      HIP_TRY(hipSetDevice(x->device));
      HIP_TRY(hipDeviceSynchronize());
      std::vector<int> lv;
      const int rc = ens_fetch(x->adv.level, (size_t)x->n, lv); if (rc) return rc;
      for (int v : lv)
        if (v != x->cfg.working_curriculum_step)
          return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: the mode cannot be switched off (advance_every = 0) while learners stand on different levels; call dql_ensemble_set_level first; nothing was changed");
    }
    x->advance_every = 0;
    return DQL_OK;
  }
  if (x->nstep) return fail(DQL_EINVAL, ENS_NSTEP_REFUSED("dql_ensemble_set_curriculum"));
  if (x->team_nstep) return fail(DQL_EINVAL, ENS_TEAM_NSTEP_REFUSED("dql_ensemble_set_curriculum"));
  if (!ratios) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: null ratios; nothing was changed");
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) if (!std::isfinite(ratios[k])) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: the five transfer ratios must be finite; nothing was changed");
  if (advance_exhausted != 0 && advance_exhausted != 1) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: advance_exhausted must be 0 or 1; nothing was changed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int> level;
  int rc = ens_fetch(x->adv.level, (size_t)x->n, level); if (rc) return rc;
  int top = 0;
  for (int v : level) top = v > top ? v : top;
  if (last_level < top || last_level >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: last_level must lie between the learners' current level and 4; nothing was changed");
  rc = ens_upload_mdpk5(x); if (rc) return rc;
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) x->rule.ratios[k] = ratios[k];
  x->rule.last_level = last_level; x->rule.advance_exhausted = advance_exhausted;
  x->advance_every = advance_every;
  return DQL_OK;
}
int dql_ensemble_set_level_schedules(dql_ensemble* x, int32_t level, const double* eps, int32_t n_eps, int32_t window, int32_t min_successes, int32_t max_episodes) {
  CHECK_ENS(x);
  if (level < 0 || level >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: the level must be in 0..4");
  if (!eps) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: null table");
  if (n_eps < 1 || n_eps > (1 << 22)) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: the table length must be in 1..2^22");
  uint32_t* d_e = nullptr;
  const int rc = ens_check_upload_rule(x, "dql_ensemble_set_level_schedules", "", nullptr, 0, eps, n_eps, window, min_successes, max_episodes, &d_e); if (rc) return rc;
  LevelSched lv[DQL_MAX_LEVELS];
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) lv[k] = x->h_lv[k];
  lv[level] = LevelSched{d_e, n_eps, window, min_successes, max_episodes};
  if (hipMemcpy(x->d_lv, lv, sizeof(lv), hipMemcpyHostToDevice) != hipSuccess) { (void)x->dev.release(d_e); return fail(DQL_EHIP, "hipMemcpy failed"); }
  (void)x->dev.release((void*)x->h_lv[level].eps_tab);  // the table it replaces
  x->h_lv[level] = lv[level]; x->have_lv[level] = true;
  return DQL_OK;
}
int dql_ensemble_get_levels(dql_ensemble* x, int32_t* level, int32_t* promoted_at, int32_t* episodes_at, int64_t* entered_period) {
  CHECK_ENS(x);
  if (!level || !promoted_at || !episodes_at || !entered_period) return fail(DQL_EINVAL, "dql_ensemble_get_levels: null array");
  HIP_TRY(hipSetDevice(x->device));
  const size_t n = (size_t)x->n;
  HIP_TRY(hipMemcpy(level, x->adv.level, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(promoted_at, x->adv.promoted_at, (size_t)DQL_MAX_LEVELS * n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(episodes_at, x->adv.episodes_at, (size_t)DQL_MAX_LEVELS * n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(entered_period, x->adv.entered_period, (size_t)DQL_MAX_LEVELS * n * sizeof(long long), hipMemcpyDeviceToHost));
  // the level a learner stands on has no history entry yet: its row shows the counters as they are
  std::vector<int> promoted, lvl_eps;
  int rc = ens_fetch(x->mem.promoted, n, promoted);
  if (!rc) rc = ens_fetch(x->mem.level_episodes, n, lvl_eps);
  if (rc) return rc;
  for (size_t l = 0; l < n; ++l) {
    const int k = level[l];
    if (k < 0 || k >= DQL_MAX_LEVELS) continue;
    promoted_at[(size_t)k * n + l] = promoted[l]; episodes_at[(size_t)k * n + l] = lvl_eps[l];
  }
  return DQL_OK;
}
int dql_ensemble_n_unfinished(dql_ensemble* x, int64_t* n) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "null pointer");
  if (!x->advance_every && !x->team_every) return dql_ensemble_n_live(x, n);
  HIP_TRY(hipSetDevice(x->device));
  std::vector<int> frozen, level, promoted;
  return ens_fetch_levels(x, frozen, level, promoted, n);
}
int dql_ensemble_get_period_index(dql_ensemble* x, int64_t* j) {
  CHECK_ENS(x);
  if (!j) return fail(DQL_EINVAL, "null pointer");
  *j = x->j;
  return DQL_OK;
}
int dql_ensemble_transfer(dql_ensemble* x, int32_t k, double ratio) {
  CHECK_ENS(x);
  if (k < 0 || k >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_transfer: curriculum step must be in 0..4");
  HIP_TRY(hipSetDevice(x->device));
  // a refined ensemble: both halves of every learner, as 2 n table sets of the same kernel
  const bool refined = x->refine_feature >= 0;
  const long long sets = refined ? 2 * x->n : x->n, total = sets * DQL_CELLS_PER_LEVEL;
  hipLaunchKernelGGL(k_ens_transfer, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, refined ? x->rq_a : x->mem.qa, refined ? x->rq_b : x->mem.qb, sets, (int)k,
                     (int)((k - 1 + DQL_MAX_LEVELS) % DQL_MAX_LEVELS), ratio);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return DQL_OK;
}
static int ens_slice(dql_ensemble* x, int64_t first, int64_t count, const char* who) {
  if (first < 0 || count < 1 || first > x->n || count > x->n - first) return fail(DQL_EINVAL, std::string(who) + ": the slice [first, first + count) must lie inside [0, n_learners) and hold at least one learner");
  return DQL_OK;
}
int dql_ensemble_get_tables(dql_ensemble* x, int64_t first, int64_t count, double* qa_or_null, double* qb_or_null, double* count_or_null) {
  CHECK_ENS(x);
  ENS_REFINED_REFUSED(x, "dql_ensemble_get_tables", "use dql_ensemble_get_refined_tables");
  int rc = ens_slice(x, first, count, "dql_ensemble_get_tables"); if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  const size_t off = (size_t)first * DQL_N_CELLS, bytes = (size_t)count * DQL_N_CELLS * sizeof(double);
  if (qa_or_null) HIP_TRY(hipMemcpy(qa_or_null, x->mem.qa + off, bytes, hipMemcpyDeviceToHost));
  if (qb_or_null) HIP_TRY(hipMemcpy(qb_or_null, x->mem.qb + off, bytes, hipMemcpyDeviceToHost));
  if (count_or_null) HIP_TRY(hipMemcpy(count_or_null, x->mem.count + off, bytes, hipMemcpyDeviceToHost));
  return DQL_OK;
}
int dql_ensemble_set_tables(dql_ensemble* x, int64_t first, int64_t count, const double* qa_or_null, const double* qb_or_null, const double* count_or_null) {
  CHECK_ENS(x);
  ENS_REFINED_REFUSED(x, "dql_ensemble_set_tables", "use dql_ensemble_set_refined_tables");
  int rc = ens_slice(x, first, count, "dql_ensemble_set_tables"); if (rc) return rc;
  if (count_or_null)  // the counters index the learning-rate table on the device
    for (size_t i = 0; i < (size_t)count * DQL_N_CELLS; ++i)
      if (!(count_or_null[i] >= 0.0 && count_or_null[i] < 9007199254740992.0)) return fail(DQL_EINVAL, "dql_ensemble_set_tables: visit counters must be in [0, 2^53)");
  HIP_TRY(hipSetDevice(x->device));
  const size_t off = (size_t)first * DQL_N_CELLS, bytes = (size_t)count * DQL_N_CELLS * sizeof(double);
  if (qa_or_null) HIP_TRY(hipMemcpy(x->mem.qa + off, qa_or_null, bytes, hipMemcpyHostToDevice));
  if (qb_or_null) HIP_TRY(hipMemcpy(x->mem.qb + off, qb_or_null, bytes, hipMemcpyHostToDevice));
  if (count_or_null) HIP_TRY(hipMemcpy(x->mem.count + off, count_or_null, bytes, hipMemcpyHostToDevice));
  return DQL_OK;
}
int dql_ensemble_get_counters(dql_ensemble* x, int64_t* decisions, int64_t* episodes, int64_t* successes, int64_t* by_code, int32_t* promoted, int32_t* level_episodes,
                              uint8_t* frozen) {
  CHECK_ENS(x);
  if (!decisions || !episodes || !successes || !by_code || !promoted || !level_episodes || !frozen) return fail(DQL_EINVAL, "dql_ensemble_get_counters: null array");
  HIP_TRY(hipSetDevice(x->device));
  const size_t n = (size_t)x->n;
  std::vector<int> h(n);
  HIP_TRY(hipMemcpy(decisions, x->mem.decisions, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(by_code, x->mem.by_code, (size_t)DQL_N_CHECK_CODES * n * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h.data(), x->mem.episodes, n * sizeof(int), hipMemcpyDeviceToHost)); for (size_t i = 0; i < n; ++i) episodes[i] = h[i];
  HIP_TRY(hipMemcpy(h.data(), x->mem.successes, n * sizeof(int), hipMemcpyDeviceToHost)); for (size_t i = 0; i < n; ++i) successes[i] = h[i];
  HIP_TRY(hipMemcpy(promoted, x->mem.promoted, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(level_episodes, x->mem.level_episodes, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h.data(), x->mem.frozen, n * sizeof(int), hipMemcpyDeviceToHost)); for (size_t i = 0; i < n; ++i) frozen[i] = h[i] ? 1 : 0;
  return DQL_OK;
}
int dql_ensemble_get_episode_log(dql_ensemble* x, uint8_t* code, uint16_t* length, int32_t capacity, int32_t* n_episodes) {
  CHECK_ENS(x);
  if (!code || !length || !n_episodes) return fail(DQL_EINVAL, "dql_ensemble_get_episode_log: null array");
  if (capacity != x->mem.log_cap || capacity < 1) return fail(DQL_EINVAL, "dql_ensemble_get_episode_log: capacity must be the (positive) log capacity the ensemble was created with");
  HIP_TRY(hipSetDevice(x->device));
  const size_t n = (size_t)x->n * (size_t)capacity;
  HIP_TRY(hipMemcpy(code, x->mem.log_code, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(length, x->mem.log_len, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_episodes, x->mem.log_n, (size_t)x->n * sizeof(int), hipMemcpyDeviceToHost));
  return DQL_OK;
}
int dql_ensemble_get_state(dql_ensemble* x, double* reals, int32_t* ints) {
  CHECK_ENS(x);
  if (!reals || !ints) return fail(DQL_EINVAL, "dql_ensemble_get_state: null array");
  HIP_TRY(hipSetDevice(x->device));
  const long long n = x->n_envs;
  int rc = by_dtype(x->cfg.dtype, [&](auto t) -> int {
    std::vector<decltype(t)> h((size_t)NQ_REAL * n * 4);
    HIP_TRY(hipMemcpy(h.data(), x->sr, h.size() * sizeof(t), hipMemcpyDeviceToHost));
    quads_to_fields(h.data(), n, reals);
    return DQL_OK;
  });
  if (rc) return rc;
  std::vector<int4> h((size_t)n);
  HIP_TRY(hipMemcpy(h.data(), x->si, (size_t)n * sizeof(int4), hipMemcpyDeviceToHost));
  unpack_ints(h.data(), n, ints);
  return DQL_OK;
}
int dql_ensemble_index_faults(dql_ensemble* x, int64_t* n) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(x->device));
  unsigned long long v = 0;
  HIP_TRY(hipMemcpy(&v, x->mem.faults, sizeof(v), hipMemcpyDeviceToHost));
  *n = (int64_t)v;
  return DQL_OK;
}
// the learners' tables are read where they live (the ensemble's device arrays are [L][DQL_N_CELLS] double already): k_score only reads them and touches nothing else of the ensemble
int dql_ensemble_score(dql_ensemble* x, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed,
                       int32_t max_steps, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null) {
  CHECK_ENS(x);
  int rc = check_config(eval_cfg); if (rc) return rc;
  rc = score_check("dql_ensemble_score", count, envs_per_learner, episodes_per_env, max_steps, by_code, steps_sum, ep_code_or_null, ep_steps_or_null); if (rc) return rc;
  TableSets q;
  rc = tables_of_slice("dql_ensemble_score", x, first, count, q); if (rc) return rc;
  return score_run(eval_cfg, count, envs_per_learner, episodes_per_env, seed, max_steps, q, by_code, steps_sum, ep_code_or_null, ep_steps_or_null);
}
int dql_diag_ensemble_launches(dql_ensemble* x, int64_t* launches, int64_t* periods, int64_t* wave_periods) {
  CHECK_ENS(x);
  if (!launches || !periods || !wave_periods) return fail(DQL_EINVAL, "null pointer");
  *launches = x->n_launches; *periods = x->launched_periods; *wave_periods = x->launched_wave_periods;
  return DQL_OK;
}
int dql_diag_ensemble_last(dql_ensemble* x, double* run_ms) {
  CHECK_ENS(x);
  if (!run_ms) return fail(DQL_EINVAL, "null pointer");
  if (x->last_ms < 0.0) return fail(DQL_ESTATE, "no dql_ensemble_run call has completed on this ensemble");
  *run_ms = x->last_ms;
  return DQL_OK;
}
}  // extern "C"
