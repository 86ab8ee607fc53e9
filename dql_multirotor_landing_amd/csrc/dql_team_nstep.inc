// dql_team_nstep.inc: team learners with n-step Double-Q targets, one pending window per env (include/dql.h dql_ensemble_set_team_nstep / _get_team_nstep,
// DESIGN.md section 24): the kernel and the two C calls.  A fragment of dql_hip.hip's translation unit, not a header, included after dql_teams.inc (TeamArgs,
// TeamCtl) and dql_nstep.inc (NstepDev).  The per-team body is csrc/dql_team_nstep.hpp's team_apply_nstep; the per-env body is dql_team.hpp's, unchanged.
// k_learn_team's shape: workgroups of one wave, lane = env g, a team is E consecutive lanes, two __syncthreads() per period.  Added: the windows of the wave's
// 64 envs in LDS for the launch, [slot][lane] as in k_learn_nstep (16 x 64 x 10 B), and their heads and lengths [lane] — the applying lane cannot hold those of
// 64 envs in registers.  A lane loads its env's window before the first barrier of the launch and stores it beside store_env, after the last; in between only
// the team's applying lane touches the team's columns, between the two barriers of a period.  The windows of a team frozen at the launch's start are neither
// loaded nor stored.
struct LdsTeamWindow {
  uint16_t* k; double* v; int* h; int* n;  // column 0 of the team (its first lane): env e of the team is column e
  DQL_DEV uint16_t& key(int e, int slot) const { return k[slot * 64 + e]; }
  DQL_DEV double& val(int e, int slot) const { return v[slot * 64 + e]; }
  DQL_DEV int& head(int e) const { return h[e]; }
  DQL_DEV int& len(int e) const { return n[e]; }
};
template <typename T> struct TeamNstepArgs {
  TeamArgs<T> t;
  NstepDev tm;  // the persistent windows: key / val [DQL_NSTEP_MAX][n_envs], len [n_envs]
  int nstep;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_team_nstep(TeamNstepArgs<T> ga) {
  const TeamArgs<T>& t = ga.t;
  const LearnArgs<T>& a = t.a;
  const int tid = threadIdx.x;
  const long long g = (long long)blockIdx.x * 64 + tid;
  const bool active = g < t.n_envs;
  const long long l = active ? (g >> t.team_shift) : 0;  // < a.mem.n
  const int lead = tid & ~(t.envs_per_learner - 1);      // the team's first lane: the one that applies
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
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)a.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(a.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  const double* qa = a.mem.qa + l * DQL_N_CELLS;
  const double* qb = a.mem.qb + l * DQL_N_CELLS;
  const bool applies = active && tid == lead;
  TeamState ts = TeamState{};
  if (applies) ts = team_load(a.sched, a.mem, l);
  bool live = active && a.mem.frozen[l] == 0;
  uint32_t eps_thr = live ? a.sched.eps_tab[a.mem.level_episodes[l] < a.sched.n_eps ? a.mem.level_episodes[l] : a.sched.n_eps - 1] : 0u;
  const bool loaded = live;
  Env<T> e = Env<T>{};
  const LdsTeamWindow mine{sKey + tid, sVal + tid, sHead + tid, sLen + tid};  // this lane's own column: env 0 of it
  sHead[tid] = 0; sLen[tid] = 0;
  if (live) {
    load_env(e, a.sr, a.si[g], t.n_envs, g, cl);
    team_window_load(ga.tm, t.n_envs, g, 0, ga.nstep, mine);  // read by the applying lane behind the period's first barrier
  }
  const int np = a.n_periods < LEARN_MAX_PERIODS ? a.n_periods : LEARN_MAX_PERIODS;
  for (int p = 0; p < np; ++p) {
    TeamRecord r{0.0, -1, 0, 0, 0};
    if (live) r = team_env_period<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, e, qa, qb, eps_thr, a.seed, g, a.j0 + p, a.mgr0[p], a.tick_sched[p], kv);
    sRec[tid] = r;
    __syncthreads();  // the records (and, in the first period, the windows) are in LDS; every row load of this period lies before the first table write of it
    if (applies && live) {
      team_apply_nstep(a.sched, a.mem, cl.quirks, a.mdp_run.gamma, l, &sRec[tid], t.envs_per_learner, ga.nstep, mine, ts);  // `mine` of the first lane: the team's columns
      sCtl[tid] = TeamCtl{ts.eps_thr, ts.live ? 1 : 0};
    }
    __syncthreads();  // workgroup-scope release of the applying lanes' table stores and window writes, acquire in front of the next period's row loads (dql_team.hpp)
    if (live) { const TeamCtl ctl = sCtl[lead]; eps_thr = ctl.eps_thr; live = ctl.live != 0; }
    if (__ballot(live) == 0ull) break;
  }
  if (loaded) {
    store_env(e, a.sr, a.si, t.n_envs, g, cl);
    team_window_store(ga.tm, t.n_envs, g, 0, ga.nstep, mine);  // behind the last period's second barrier
  }
  if (applies && loaded) team_store(ts, a.mem, l);
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
