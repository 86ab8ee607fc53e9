// dql_teams.inc: sequential learners with teams of envs (include/dql.h dql_ensemble_create_teams, DESIGN.md section 17): k_learn_team and the C calls a team
// ensemble adds.  A fragment of dql_hip.hip's translation unit, not a header; included after dql_ensemble.inc (struct dql_ensemble, LearnArgs, make_learn_args,
// ens_create) and dql_recipes.inc.  The per-env and per-team bodies, and why two workgroup barriers per period order them, are csrc/dql_team.hpp's.
template <typename T> struct TeamArgs {
  LearnArgs<T> a;      // a.mem.n: the learners; a.sr / a.si: the n_envs envs
  long long n_envs;    // a.mem.n * envs_per_learner: the stride of the state arrays
  int envs_per_learner, team_shift;  // E = 1 << team_shift, a divisor of 64
};
// the identity lane map of k_learn_team and k_learn_team_nstep: lane = env g = 64 blockIdx.x + tid, team g >> team_shift; the last wave may hold fewer teams
template <typename T> DQL_DEV TeamLane team_lane_identity(const TeamArgs<T>& t, int tid) {
  const long long g = (long long)blockIdx.x * 64 + tid;
  return TeamLane{g, g >> t.team_shift, g < t.n_envs};
}
// The wave prologue and the LDS of a team wave; what the wave does is team_wave's (csrc/dql_team_nstep.hpp), here without windows.
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_team(TeamArgs<T> t) {
  const LearnArgs<T>& a = t.a;
  const int tid = threadIdx.x;
  SimK<T> cl = a.c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // as in k_learn
  __shared__ TeamRecord sRec[64];
  __shared__ TeamCtl sCtl[64];
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  team_wave<XMODE>(t, cl, cfgk, tc, kv, tid, sRec, sCtl, NoTeamWindows{}, team_lane_identity(t, tid), a.sched, a.mdp);
}
template <typename T> static void launch_learn_team(dql_ensemble* x, int k, int n_waves) {
  TeamArgs<T> g;
  g.a = make_learn_args<T>(x, x->mdpk, k);
  g.n_envs = x->n_envs; g.envs_per_learner = x->envs_per_learner; g.team_shift = 0;
  while ((1 << g.team_shift) < x->envs_per_learner) ++g.team_shift;
  hipLaunchKernelGGL((k_learn_team<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, g);
}
extern "C" {
int dql_ensemble_create_teams(const dql_config* cfg, int device, int64_t n_learners, int32_t envs_per_learner, uint64_t seed, int32_t log_capacity, dql_ensemble** out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (!out) return fail(DQL_EINVAL, "dql_ensemble_create_teams: null pointer; nothing was launched");
  if (cfg->two_axis) return fail(DQL_EINVAL, "dql_ensemble_create_teams: two-axis configs are refused (the reference's learner is x-only); nothing was launched");
  if (cfg->trajectory == DQL_TRAJ_EIGHT) return fail(DQL_EINVAL, "dql_ensemble_create_teams: the figure-eight trajectory is refused (the reference's learner is x-only); nothing was launched");
  if (!team_size_ok(envs_per_learner)) return fail(DQL_EINVAL, "dql_ensemble_create_teams: envs_per_learner must be one of 1, 2, 4, 8, 16, 32, 64 (a team is consecutive lanes of one wave); nothing was launched");
  if (n_learners < 1 || n_learners > DQL_ENSEMBLE_MAX_LEARNERS / envs_per_learner)
    return fail(DQL_EINVAL, "dql_ensemble_create_teams: n_learners must be positive and n_learners * envs_per_learner at most 2^20 (DQL_ENSEMBLE_MAX_LEARNERS); nothing was launched");
  if (log_capacity < 0 || log_capacity > DQL_ENSEMBLE_MAX_LOG) return fail(DQL_EINVAL, "dql_ensemble_create_teams: log_capacity must be in 0..2^20 (DQL_ENSEMBLE_MAX_LOG); nothing was launched");
  return ens_create(cfg, device, n_learners, envs_per_learner, true, seed, log_capacity, out);
}
int dql_ensemble_envs_per_learner(dql_ensemble* x, int32_t* envs_per_learner) {
  CHECK_ENS(x);
  if (!envs_per_learner) return fail(DQL_EINVAL, "null pointer");
  *envs_per_learner = x->envs_per_learner;
  return DQL_OK;
}
}  // extern "C"
