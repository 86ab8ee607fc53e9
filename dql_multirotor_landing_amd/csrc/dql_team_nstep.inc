// dql_team_nstep.inc: team learners with n-step Double-Q targets, one pending window per env (include/dql.h dql_ensemble_set_team_nstep / _get_team_nstep,
// DESIGN.md section 24): the kernel and the two C calls.  A fragment of dql_hip.hip's translation unit, not a header, included after dql_teams.inc (TeamArgs)
// and dql_nstep.inc (NstepDev).  The per-team body is csrc/dql_team_nstep.hpp's team_apply_nstep; the per-env body is dql_team.hpp's, unchanged.
// k_learn_team's shape: workgroups of one wave, lane = env g, a team is E consecutive lanes, two __syncthreads() per period.  Added: the windows of the wave's
// 64 envs in LDS for the launch, [slot][lane] as in k_learn_nstep (16 x 64 x 10 B), and their heads and lengths [lane] — the applying lane cannot hold those of
// 64 envs in registers.  A lane loads its env's window before the first barrier of the launch and stores it beside store_env, after the last; in between only
// the team's applying lane touches the team's columns, between the two barriers of a period.  The windows of a team frozen at the launch's start are neither
// loaded nor stored.  All of that is team_wave's (csrc/dql_team_nstep.hpp, with its LdsTeamWindow); the kernel is the wave prologue and the LDS.
template <typename T> struct TeamNstepArgs {
  TeamArgs<T> t;
  NstepDev tm;  // the persistent windows: key / val [DQL_NSTEP_MAX][n_envs], len [n_envs]
  int nstep;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_team_nstep(TeamNstepArgs<T> ga) {
  const TeamArgs<T>& t = ga.t;
  const LearnArgs<T>& a = t.a;
  const int tid = threadIdx.x;
  SimK<T> cl = a.c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // as in k_learn
  __shared__ TeamRecord sRec[64];
  __shared__ TeamCtl sCtl[64];
  __shared__ uint16_t sKey[NSTEP_MAX * 64];
  __shared__ double sVal[NSTEP_MAX * 64];
  __shared__ int sHead[64];
  __shared__ int sLen[64];
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  const LdsTeamWindow mine{sKey + tid, sVal + tid, sHead + tid, sLen + tid};  // this lane's own column: env 0 of it
  team_wave<XMODE>(t, cl, cfgk, tc, kv, tid, sRec, sCtl, TeamWindows<NstepDev>{mine, ga.tm, ga.nstep}, team_lane_identity(t, tid), a.sched, a.mdp);
}
template <typename T> static void launch_learn_team_nstep(dql_ensemble* x, int k, int n_waves) {
  TeamNstepArgs<T> g;
  g.t.a = make_learn_args<T>(x, x->mdpk, k);
  g.t.n_envs = x->n_envs; g.t.envs_per_learner = x->envs_per_learner; g.t.team_shift = 0;
  while ((1 << g.t.team_shift) < x->envs_per_learner) ++g.t.team_shift;
  g.tm = NstepDev{x->tn_key, x->tn_val, x->tn_len};
  g.nstep = x->team_nstep;
  hipLaunchKernelGGL((k_learn_team_nstep<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, g);
}

extern "C" {
int dql_ensemble_set_team_nstep(dql_ensemble* x, int32_t n) {
  if (!x) return fail(DQL_EINVAL, "dql_ensemble_set_team_nstep: null ensemble; nothing was changed");
  ENS_REFINED_REFUSED(x, "dql_ensemble_set_team_nstep", ENS_REFINED_MODES);
  if (n < 0 || n > DQL_NSTEP_MAX) return fail(DQL_EINVAL, "dql_ensemble_set_team_nstep: n must be in 0..16 (DQL_NSTEP_MAX; 0: the one-step team kernel); nothing was changed");
  if (!x->teams) return fail(DQL_EINVAL, "dql_ensemble_set_team_nstep: the ensemble was not made by dql_ensemble_create_teams (a plain ensemble takes dql_ensemble_set_nstep); nothing was changed");
  if (n >= 1 && (x->advance_every || x->rcp))
    return fail(DQL_EINVAL, "dql_ensemble_set_team_nstep: team n-step targets are refused in per-learner curriculum mode and with recipes installed (switch them off first); nothing was changed");
  if (n == x->team_nstep) return DQL_OK;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t G = (size_t)x->n_envs;
  if (x->tn_len) {
    std::vector<int> len;
    const int rc = ens_fetch(x->tn_len, G, len); if (rc) return rc;
    for (int v : len)
      if (v != 0)
        return fail(DQL_ESTATE, "dql_ensemble_set_team_nstep: n cannot change while an env's pending window holds entries (change it after creation or after dql_ensemble_set_level; that every team is frozen is not enough, a frozen team's windows stay open); nothing was changed");
  }
  if (n >= 1 && !x->tn_len) {  // the persistent windows, zeroed, on the first call with n >= 1: 160 B per env
    uint16_t* key = nullptr; double* val = nullptr; int* len = nullptr;
    const int rc = ens_alloc_zeroed(x->dev, {{(void**)&key, (size_t)DQL_NSTEP_MAX * G * sizeof(uint16_t)}, {(void**)&val, (size_t)DQL_NSTEP_MAX * G * sizeof(double)}, {(void**)&len, G * sizeof(int)}});
    if (rc) return fail(rc, rc == DQL_ENOMEM ? "hipMalloc failed" : "hipMemset failed");
    x->tn_key = key; x->tn_val = val; x->tn_len = len;
  }
  x->team_nstep = n;
  return DQL_OK;
}
int dql_ensemble_get_team_nstep(dql_ensemble* x, int32_t* n, int32_t* pending_len_or_null) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "dql_ensemble_get_team_nstep: null pointer");
  *n = x->team_nstep;
  if (!pending_len_or_null) return DQL_OK;
  const size_t G = (size_t)x->n_envs;
  if (!x->tn_len) { std::memset(pending_len_or_null, 0, G * sizeof(int32_t)); return DQL_OK; }  // no window was ever made
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemcpy(pending_len_or_null, x->tn_len, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DQL_OK;
}
}  // extern "C"
