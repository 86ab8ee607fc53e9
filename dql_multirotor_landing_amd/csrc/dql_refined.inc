// dql_refined.inc: sequential learners and greedy scoring on a state split by one bit of hidden state (dql_ensemble_set_refinement, dql_score_refined and their
// kin, DESIGN.md section 34).  A fragment of dql_hip.hip's translation unit, not a header.  Needs dql_greedy.inc (score_check, TableSets, Flight, Sums, EpisodeLog,
// RangeFaults, LastCall, timed_launch, fill_greedy_args, set_coords, flush_tally), dql_ensemble.inc (struct dql_ensemble, LearnArgs, make_learn_args, ens_slice,
// ens_alloc_zeroed, the forward declaration of launch_learn_refined that ens_fly switches to) and dql_refined.hpp.
// k_learn_refined has k_learn's shape and k_score_refined k_score's: one learner or env per lane, workgroups of one wave, no LDS beyond TickLds, no atomics in the
// learner (the scorer's are flush_tally's and one add of the lane's range faults), the feature a wave-uniform switch, the cut one global load per period.
template <typename T> struct LearnRefinedArgs {
  LearnArgs<T> a;  // a.mem.qa / qb / count: the refined arrays [n][2][DQL_N_CELLS]
  RefinedMem rf;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_refined(LearnRefinedArgs<T> g) {
  const LearnArgs<T>& a = g.a;
  const int tid = threadIdx.x;
  const long long l = (long long)blockIdx.x * 64 + tid;
  SimK<T> cl = a.c;
  cl.two_axis = 0;  // XMODE == X_ONLY (refined_learner_periods asserts it)
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
  refined_learner_periods<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.sched, a.mem, g.rf, a.sr, a.si, a.seed, l, l < a.mem.n, a.j0, a.n_periods, a.mgr0, a.tick_sched, kv);
}
template <typename T> static void launch_learn_refined(dql_ensemble* x, int k, int n_waves) {
  LearnRefinedArgs<T> g;
  g.a = make_learn_args<T>(x, x->mdpk, k);
  g.a.mem.qa = x->rq_a; g.a.mem.qb = x->rq_b; g.a.mem.count = x->rq_count;
  g.rf = RefinedMem{x->d_cut, x->d_half, x->refine_feature};
  hipLaunchKernelGGL((k_learn_refined<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, g);
}

template <typename T> struct ScoreRefinedArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  RolloutInit<T> init;
  const double* qa; const double* qb;                                  // [n_tables][2][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule)
  const double* cut;                                                   // [DQL_N_STATES]
  unsigned long long* by_code;                                         // [n_tables][SCORE_N_COLS]
  unsigned long long* steps_sum;                                       // [n_tables]
  unsigned long long* faults;                                          // [1] decisions taken on a value out of range (0 unless a bug)
  ScoreLog log;
  unsigned long long seed;
  int blocks_per_table, max_steps, episodes, n_tables, feature;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_score_refined(ScoreRefinedArgs<T> a) {
  const int tid = threadIdx.x;
  const auto [k, i, g] = set_coords(a.blocks_per_table);
  if (k >= a.n_tables) {  // never taken unless a bug (the host sizes the grid): nothing is read or written for a table set that is not there
    if (tid == 0) atomicAdd(a.faults, 1ull);
    return;
  }
  SimK<T> cl = a.c;
  cl.two_axis = 0;  // XMODE == X_ONLY (score_refined_episodes asserts it)
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // as in k_score
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  const double* qa = a.qa + (size_t)k * REFINED_CELLS;
  const double* qb = a.qb + (size_t)k * REFINED_CELLS;
  const ScoreRefinedTally r = score_refined_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes, a.feature, a.cut,
                                                                  a.mgr0, a.sched, kv, a.log, g);
  if (r.faults) atomicAdd(a.faults, (unsigned long long)r.faults);
  flush_tally(r.t, a.by_code, a.steps_sum, (size_t)k);
}

extern "C" {
static thread_local LastCall g_score_refined_last;
// feature and cut as dql_model_split takes them
static int refined_check_feature_cut(const std::string& w, int32_t feature, const double* cut, const char* tail) {
  if (feature < 0 || feature >= DQL_SPLIT_N_FEATURES) return fail(DQL_EINVAL, w + ": feature must be one of DQL_SPLIT_* (0..10)" + tail);
  if (!cut) return fail(DQL_EINVAL, w + ": null cut" + tail);
  for (int s = 0; s < DQL_N_STATES; ++s)
    if (cut[s] != cut[s]) return fail(DQL_EINVAL, w + ": cut holds a NaN at state " + std::to_string(s) + " (+-inf are allowed)" + tail);
  return DQL_OK;
}
// everything both scoring entry points share, checked before the device is touched: a refused call starts no kernel
static int score_refined_check(const char* who, const dql_config* cfg, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, int32_t max_steps, int32_t feature,
                               const double* cut, const int64_t* by_code, const int64_t* steps_sum, const uint8_t* ep_code, const uint16_t* ep_steps) {
  const std::string w(who);
  int rc = score_check(who, n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, ep_code, ep_steps); if (rc) return rc;
  if (cfg->two_axis) return fail(DQL_EINVAL, w + ": two-axis configs are refused (the refinement is the x MDP's); nothing was launched");
  if (cfg->trajectory == DQL_TRAJ_EIGHT) return fail(DQL_EINVAL, w + ": the figure-eight trajectory is refused (the refinement is the x MDP's, as the learners are); nothing was launched");
  return refined_check_feature_cut(w, feature, cut, "; nothing was launched");
}
// cut: a DEVICE array [DQL_N_STATES]
static int score_refined_run(const char* who, const dql_config* cfg, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, int feature,
                             const double* d_cut, const TableSets& q, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code, uint16_t* ep_steps) {
  const long long n_total = n_tables * envs_per_table;
  Flight fl;
  int rc = fl.setup(*cfg, max_steps); if (rc) return rc;
  Sums sums;
  const Sums::Slice s_by_code = sums.add((size_t)n_tables * SCORE_N_COLS), s_steps = sums.add((size_t)n_tables), s_faults = sums.add(1);
  rc = sums.alloc_zeroed(); if (rc) return rc;
  EpisodeLog elog;
  rc = elog.setup(ep_code != nullptr, (size_t)episodes * (size_t)n_total); if (rc) return rc;
  const ScoreLog log{(uint8_t*)elog.code.p, (uint16_t*)elog.steps.p, n_total};
  LastCall call;
  rc = timed_launch([&] {
    by_dtype(cfg->dtype, [&](auto t) {
      using T = decltype(t);
      ScoreRefinedArgs<T> a;
      fill_greedy_args<T>(a, *cfg, q, fl, seed, envs_per_table, max_steps);
      a.cut = d_cut; a.by_code = sums.dev(s_by_code); a.steps_sum = sums.dev(s_steps); a.faults = sums.dev(s_faults); a.log = log; a.episodes = episodes;
      a.n_tables = (int)n_tables; a.feature = feature;
      call.instance<T>(TICK_PLAIN, X_ONLY);
      hipLaunchKernelGGL((k_score_refined<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)(n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
    });
  }, &call.ms, RangeFaults{sums.dev(s_faults), who, "kernel's", "decisions"});
  if (rc) return rc;
  rc = sums.down({{by_code, s_by_code}, {steps_sum, s_steps}}); if (rc) return rc;
  rc = elog.down(ep_code, ep_steps); if (rc) return rc;
  g_score_refined_last = call;
  return DQL_OK;
}
int dql_score_refined(const dql_config* cfg, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, int32_t feature,
                      const double* cut, const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n_tables > DQL_SCORE_REFINED_MAX_TABLES)
    return fail(DQL_EINVAL, "dql_score_refined: the number of table sets must be in 1..4096 (DQL_SCORE_REFINED_MAX_TABLES: 90 720 B of tables are uploaded per set); nothing was launched");
  rc = score_refined_check("dql_score_refined", cfg, n_tables, envs_per_table, episodes_per_env, max_steps, feature, cut, by_code, steps_sum, ep_code_or_null, ep_steps_or_null);
  if (rc) return rc;
  TableSets q;
  rc = q.from_host("dql_score_refined", device, 2 * n_tables, qa, qb); if (rc) return rc;  // a refined set is two plain sets' bytes
  DevBuf d_cut;
  UP(d_cut, cut, (size_t)DQL_N_STATES * sizeof(double));
  return score_refined_run("dql_score_refined", cfg, n_tables, envs_per_table, episodes_per_env, seed, max_steps, feature, (const double*)d_cut.p, q, by_code, steps_sum,
                           ep_code_or_null, ep_steps_or_null);
}
int dql_diag_score_refined_last(double* kernel_ms, int32_t* inst3) {
  return diag_last(g_score_refined_last, kernel_ms, inst3, "no dql_score_refined or dql_ensemble_score_refined call has completed on this thread");
}

// ---- the refinement of an ensemble ----
#define ENS_NOT_REFINED(x, who) do { if ((x)->refine_feature < 0) return fail(DQL_EINVAL, who ": the ensemble has no refinement: install one with dql_ensemble_set_refinement first, or use the plain call (" \
                                                                                   "dql_ensemble_score, dql_ensemble_get_tables, dql_ensemble_set_tables); nothing was changed and nothing was launched"); } while (0)
int dql_ensemble_set_refinement(dql_ensemble* x, int32_t feature, const double* cut) {
  CHECK_ENS(x);
  const char* tail = "; nothing was changed";
  if (x->teams || x->envs_per_learner > 1)
    return fail(DQL_EINVAL, "dql_ensemble_set_refinement: a refinement is for an ensemble made by dql_ensemble_create (one env per learner, no teams); nothing was changed");
  if (x->refine_feature >= 0) return fail(DQL_EINVAL, "dql_ensemble_set_refinement: the ensemble already has a refinement (it is installed once, at period index 0); nothing was changed");
  if (x->j != 0) return fail(DQL_EINVAL, "dql_ensemble_set_refinement: a refinement is installed at period index 0, before the first dql_ensemble_run; nothing was changed");
  if (x->rcp || x->advance_every || x->team_every || x->nstep || x->team_nstep)
    return fail(DQL_EINVAL, "dql_ensemble_set_refinement: refined learners fly the plain mode only: no recipes, no curriculum mode, no n-step targets may be installed; nothing was changed");
  int rc = refined_check_feature_cut("dql_ensemble_set_refinement", feature, cut, tail); if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t TB = (size_t)x->n * REFINED_CELLS * sizeof(double);
  rc = ens_alloc_zeroed(x->dev, {{(void**)&x->rq_a, TB}, {(void**)&x->rq_b, TB}, {(void**)&x->rq_count, TB}, {(void**)&x->d_cut, (size_t)DQL_N_STATES * sizeof(double)},
                                 {(void**)&x->d_half, (size_t)x->n}});
  if (rc) return fail(rc, rc == DQL_ENOMEM ? "dql_ensemble_set_refinement: hipMalloc failed; nothing was changed" : "dql_ensemble_set_refinement: hipMemset failed; nothing was changed");
  if (hipMemcpy(x->d_cut, cut, (size_t)DQL_N_STATES * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    for (void** p : {(void**)&x->rq_a, (void**)&x->rq_b, (void**)&x->rq_count, (void**)&x->d_cut, (void**)&x->d_half}) { (void)x->dev.release(*p); *p = nullptr; }
    return fail(DQL_EHIP, "dql_ensemble_set_refinement: hipMemcpy failed; nothing was changed");
  }
  for (int s = 0; s < DQL_N_STATES; ++s) x->h_cut[s] = cut[s];
  x->refine_feature = feature;
  return DQL_OK;
}
int dql_ensemble_get_refinement(dql_ensemble* x, int32_t* feature_or_minus1, double* cut_or_null) {
  CHECK_ENS(x);
  if (!feature_or_minus1) return fail(DQL_EINVAL, "dql_ensemble_get_refinement: null pointer");
  *feature_or_minus1 = x->refine_feature;
  if (cut_or_null && x->refine_feature >= 0) for (int s = 0; s < DQL_N_STATES; ++s) cut_or_null[s] = x->h_cut[s];
  return DQL_OK;
}
int dql_ensemble_get_refined_tables(dql_ensemble* x, int64_t first, int64_t count, double* qa_or_null, double* qb_or_null, double* count_or_null) {
  CHECK_ENS(x);
  ENS_NOT_REFINED(x, "dql_ensemble_get_refined_tables");
  int rc = ens_slice(x, first, count, "dql_ensemble_get_refined_tables"); if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  const size_t off = (size_t)first * REFINED_CELLS, bytes = (size_t)count * REFINED_CELLS * sizeof(double);
  if (qa_or_null) HIP_TRY(hipMemcpy(qa_or_null, x->rq_a + off, bytes, hipMemcpyDeviceToHost));
  if (qb_or_null) HIP_TRY(hipMemcpy(qb_or_null, x->rq_b + off, bytes, hipMemcpyDeviceToHost));
  if (count_or_null) HIP_TRY(hipMemcpy(count_or_null, x->rq_count + off, bytes, hipMemcpyDeviceToHost));
  return DQL_OK;
}
int dql_ensemble_set_refined_tables(dql_ensemble* x, int64_t first, int64_t count, const double* qa_or_null, const double* qb_or_null, const double* count_or_null) {
  CHECK_ENS(x);
  ENS_NOT_REFINED(x, "dql_ensemble_set_refined_tables");
  int rc = ens_slice(x, first, count, "dql_ensemble_set_refined_tables"); if (rc) return rc;
  if (count_or_null)  // the counters index the learning-rate table on the device
    for (size_t i = 0; i < (size_t)count * REFINED_CELLS; ++i)
      if (!(count_or_null[i] >= 0.0 && count_or_null[i] < 9007199254740992.0)) return fail(DQL_EINVAL, "dql_ensemble_set_refined_tables: visit counters must be in [0, 2^53)");
  HIP_TRY(hipSetDevice(x->device));
  const size_t off = (size_t)first * REFINED_CELLS, bytes = (size_t)count * REFINED_CELLS * sizeof(double);
  if (qa_or_null) HIP_TRY(hipMemcpy(x->rq_a + off, qa_or_null, bytes, hipMemcpyHostToDevice));
  if (qb_or_null) HIP_TRY(hipMemcpy(x->rq_b + off, qb_or_null, bytes, hipMemcpyHostToDevice));
  if (count_or_null) HIP_TRY(hipMemcpy(x->rq_count + off, count_or_null, bytes, hipMemcpyHostToDevice));
  return DQL_OK;
}
// the learners' refined tables are read where they live, with the ensemble's own feature and cut: k_score_refined touches nothing else of the ensemble
int dql_ensemble_score_refined(dql_ensemble* x, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed,
                               int32_t max_steps, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null) {
  CHECK_ENS(x);
  ENS_NOT_REFINED(x, "dql_ensemble_score_refined");
  int rc = check_config(eval_cfg); if (rc) return rc;
  rc = score_refined_check("dql_ensemble_score_refined", eval_cfg, count, envs_per_learner, episodes_per_env, max_steps, x->refine_feature, x->h_cut, by_code, steps_sum,
                           ep_code_or_null, ep_steps_or_null); if (rc) return rc;
  if (first < 0 || first > x->n || count > x->n - first)
    return fail(DQL_EINVAL, "dql_ensemble_score_refined: the slice [first, first + count) must lie inside [0, n_learners); nothing was launched");
  HIP_TRY(hipSetDevice(x->device));
  TableSets q;
  q.qa = x->rq_a + (size_t)first * REFINED_CELLS; q.qb = x->rq_b + (size_t)first * REFINED_CELLS;
  return score_refined_run("dql_ensemble_score_refined", eval_cfg, count, envs_per_learner, episodes_per_env, seed, max_steps, x->refine_feature, x->d_cut, q, by_code, steps_sum,
                           ep_code_or_null, ep_steps_or_null);
}
}  // extern "C"
