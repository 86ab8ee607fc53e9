// dql_team_levels.inc: team curriculum mode — every team of a team ensemble walks the levels by itself, n-step targets included (include/dql.h
// dql_ensemble_set_team_curriculum, DESIGN.md section 29): the two team kernels over a worklist of teams, the advance kernel, the C call.  A fragment of
// dql_hip.hip's translation unit, not a header, included after dql_teams.inc (TeamArgs) and dql_team_nstep.inc (TeamNstepArgs' NstepDev).  The worklist and
// the advance step are csrc/dql_team_levels.hpp's; the wave body stays team_wave (csrc/dql_team_nstep.hpp).
//
// k_learn_team / k_learn_team_nstep over a worklist, as k_learn_levels is k_learn over one: wave w flies the teams worklist[w tpw .. w tpw + tpw - 1],
// tpw = 64 >> team_shift (-1: a slot of E inactive lanes), all of them at level wave_level[w] — a scalar load — from which follow SimK::working, the level's
// MdpK (t.a.mdp is the array of all five) and the level's exploration table and freeze rules.  Nothing level-dependent is a lane's property.
template <typename T> struct TeamLevelsArgs {
  TeamArgs<T> t;                           // t.a.mdp: [DQL_MAX_LEVELS]; t.a.sched: the learning rates (its per-level members are replaced by lv[level])
  const LevelSched DQL_CONST_AS* lv;       // [DQL_MAX_LEVELS]
  const int* worklist;                     // [(64 >> team_shift) n_waves] teams
  const int DQL_CONST_AS* wave_level;      // [n_waves]
  int n_waves;
};
template <typename T> struct TeamLevelsNstepArgs {
  TeamLevelsArgs<T> q;
  NstepDev tm;  // the persistent windows, as in TeamNstepArgs
  int nstep;
};
// the wave's level, or -1 where the wave has nothing to fly: past the worklist's end, or (never, unless a bug: the host builds the worklist) a level out of range
template <typename T> DQL_DEV int team_levels_wave_level(const TeamLevelsArgs<T>& q, int tid) {
  const int w = (int)blockIdx.x;
  if (w >= q.n_waves) return -1;
  const int level = q.wave_level[w];
  if ((unsigned)level < (unsigned)DQL_MAX_LEVELS) return level;
  if (tid == 0) q.t.a.mem.faults[0] += 1ull;
  return -1;
}
// the worklist's lane map: slot = tid >> team_shift names the team, the lane is env tid & (E - 1) of it
template <typename T> DQL_DEV TeamLane team_lane_worklist(const TeamLevelsArgs<T>& q, int tid) {
  const int shift = q.t.team_shift;
  const long long l = (long long)q.worklist[(long long)blockIdx.x * (64 >> shift) + (tid >> shift)];
  return TeamLane{l * q.t.envs_per_learner + (tid & (q.t.envs_per_learner - 1)), l, l >= 0 && l < q.t.a.mem.n};
}
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_team_levels(TeamLevelsArgs<T> q) {
  const TeamArgs<T>& t = q.t;
  const LearnArgs<T>& a = t.a;
  const int tid = threadIdx.x;
  const int level = team_levels_wave_level(q, tid);
  if (level < 0) return;
  SimK<T> cl = a.c;
  cl.working = level;
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
  const LearnSched sc = learn_sched(a.sched.alpha_tab, a.sched.n_alpha, a.sched.alpha_min, q.lv + level);
  team_wave<XMODE>(t, cl, cfgk, tc, kv, tid, sRec, sCtl, NoTeamWindows{}, team_lane_worklist(q, tid), sc, a.mdp + level);
}
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_team_levels_nstep(TeamLevelsNstepArgs<T> ga) {
  const TeamLevelsArgs<T>& q = ga.q;
  const TeamArgs<T>& t = q.t;
  const LearnArgs<T>& a = t.a;
  const int tid = threadIdx.x;
  const int level = team_levels_wave_level(q, tid);
  if (level < 0) return;
  SimK<T> cl = a.c;
  cl.working = level;
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
  const LearnSched sc = learn_sched(a.sched.alpha_tab, a.sched.n_alpha, a.sched.alpha_min, q.lv + level);
  const LdsTeamWindow mine{sKey + tid, sVal + tid, sHead + tid, sLen + tid};  // this lane's own column: env 0 of it
  team_wave<XMODE>(t, cl, cfgk, tc, kv, tid, sRec, sCtl, TeamWindows<NstepDev>{mine, ga.tm, ga.nstep}, team_lane_worklist(q, tid), sc, a.mdp + level);
}
// an advance point: every team takes advance_team's step by itself, one thread per team (its own 2 x 567 cells, its own E envs and their window lengths;
// ordinary vector stores, nothing shared but the `faults` word, whose plain add is k_ens_advance's)
__global__ void k_ens_advance_teams(LearnMem mem, AdvanceMem adv, AdvanceRule rule, int transfer_order, int4* si, int* pending_len, int envs_per_learner, long long j, int n_cells) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= mem.n) return;
  (void)advance_team(mem, adv, rule, transfer_order, si, pending_len, envs_per_learner, l, j, n_cells);
}

template <typename T> static TeamLevelsArgs<T> make_team_levels_args(dql_ensemble* x, int k, int n_waves) {
  TeamLevelsArgs<T> q;
  q.t.a = make_learn_args<T>(x, x->mdpk5, k);
  q.t.n_envs = x->n_envs; q.t.envs_per_learner = x->envs_per_learner; q.t.team_shift = 0;
  while ((1 << q.t.team_shift) < x->envs_per_learner) ++q.t.team_shift;
  q.lv = (const LevelSched DQL_CONST_AS*)x->d_lv; q.worklist = x->twl.d_list; q.wave_level = (const int DQL_CONST_AS*)x->twl.d_wave_level; q.n_waves = n_waves;
  return q;
}
template <typename T> static void launch_learn_team_levels(dql_ensemble* x, int k, int n_waves) {
  hipLaunchKernelGGL((k_learn_team_levels<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, make_team_levels_args<T>(x, k, n_waves));
}
template <typename T> static void launch_learn_team_levels_nstep(dql_ensemble* x, int k, int n_waves) {
  TeamLevelsNstepArgs<T> g;
  g.q = make_team_levels_args<T>(x, k, n_waves);
  g.tm = NstepDev{x->tn_key, x->tn_val, x->tn_len};
  g.nstep = x->team_nstep;
  hipLaunchKernelGGL((k_learn_team_levels_nstep<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, g);
}
// dql_ensemble_run in team curriculum mode: the one advancing run loop over the worklist of teams.  The windows' lengths are handed to the advance step
// whenever the ensemble has them (a team that flew with n >= 1 earlier may still hold entries at n = 0)
static int ens_run_team_levels(dql_ensemble* x, int64_t periods, EnsKernel kern) {
  return ens_run_advancing(x, periods, kern, x->twl, [&](size_t, int level) { return ens_way_up_scheduled(x->have_lv, level, x->rule.last_level); },
                           "dql_ensemble_run: team curriculum mode needs dql_ensemble_set_level_schedules for every level from the teams' up to last_level; nothing was launched", [&] {
                             hipLaunchKernelGGL(k_ens_advance_teams, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, 0, x->mem, x->adv, x->rule, x->team_order, x->si, x->tn_len,
                                                x->envs_per_learner, (long long)x->j, (int)DQL_CELLS_PER_LEVEL);
                           });
}

extern "C" {
int dql_ensemble_set_team_curriculum(dql_ensemble* x, int32_t last_level, int32_t advance_every, const double* ratios, int32_t advance_exhausted, int32_t transfer_order) {
  if (!x) return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: null ensemble; nothing was changed");
  ENS_REFINED_REFUSED(x, "dql_ensemble_set_team_curriculum", ENS_REFINED_MODES);
  if (!x->teams) return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: the ensemble was not made by dql_ensemble_create_teams (a plain ensemble takes dql_ensemble_set_curriculum); nothing was changed");
  if (advance_every < 0 || advance_every > ADV_MAX_EVERY) return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: advance_every must be in 0..4096 (0 turns the mode off); nothing was changed");
  if (x->advance_every || x->rcp)
    return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: per-learner curriculum mode (dql_ensemble_set_curriculum) is on or recipes are installed; a team ensemble of one env per learner flies one of the two modes at a time, switch them off first; nothing was changed");
  if (advance_every == 0) {
    // the barrier launch flies every team at the config's level: switching off is refused while a team stands on another one (dql_ensemble_set_level first)
    if (x->team_every) {
      HIP_TRY(hipSetDevice(x->device));
      HIP_TRY(hipDeviceSynchronize());
      std::vector<int> lv;
      const int rc = ens_fetch(x->adv.level, (size_t)x->n, lv); if (rc) return rc;
      for (int v : lv)
        if (v != x->cfg.working_curriculum_step)
          return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: the mode cannot be switched off (advance_every = 0) while teams stand on different levels; call dql_ensemble_set_level first; nothing was changed");
    }
    x->team_every = 0;
    return DQL_OK;
  }
  if (!ratios) return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: null ratios; nothing was changed");
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) if (!std::isfinite(ratios[k])) return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: the five transfer ratios must be finite; nothing was changed");
  if (advance_exhausted != 0 && advance_exhausted != 1) return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: advance_exhausted must be 0 or 1; nothing was changed");
  if (transfer_order != RCP_ORDER_REFERENCE && transfer_order != RCP_ORDER_PAPER)
    return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: transfer_order must be 0 (the reference's) or 1 (the paper's); nothing was changed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int> level;
  int rc = ens_fetch(x->adv.level, (size_t)x->n, level); if (rc) return rc;
  int top = 0;
  for (int v : level) top = v > top ? v : top;
  if (last_level < top || last_level >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_team_curriculum: last_level must lie between the teams' current level and 4; nothing was changed");
  if (!x->twl.d_list) {  // the worklist of teams, on the first call that turns the mode on: 64 / E team slots per wave
    const int per_wave = ADV_WAVE / x->envs_per_learner;
    x->twl.resize(team_worklist_capacity(x->n, per_wave), nullptr, 0, per_wave);
    rc = ens_alloc_zeroed(x->dev, {{(void**)&x->twl.d_list, (size_t)x->twl.slots * sizeof(int)}, {(void**)&x->twl.d_wave_level, (size_t)(x->twl.slots / per_wave) * sizeof(int)}});
    if (rc) return fail(rc, rc == DQL_ENOMEM ? "hipMalloc failed" : "hipMemset failed");
  }
  rc = ens_upload_mdpk5(x); if (rc) return rc;
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) x->rule.ratios[k] = ratios[k];
  x->rule.last_level = last_level; x->rule.advance_exhausted = advance_exhausted;
  x->team_order = transfer_order;
  x->team_every = advance_every;
  return DQL_OK;
}
}  // extern "C"
