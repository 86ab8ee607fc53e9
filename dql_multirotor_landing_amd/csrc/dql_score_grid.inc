// dql_score_grid.inc: greedy scoring of K table sets over S scenarios in one launch, with the touchdowns binned by their offset from the platform centre
// (dql_score_grid / dql_ensemble_score_grid, DESIGN.md section 20).  A fragment of dql_hip.hip's translation unit, not a header.  Needs from it: fail / HIP_TRY,
// by_dtype / by_dtype_axes, DevBuf / UP, check_config, TickLds; score_check and the family's host helpers of dql_greedy.inc (TableSets, Flight for the schedule, Sums,
// EpisodeLog, LastCall / diag_last, timed_launch, fill_flight_args); struct dql_ensemble / CHECK_ENS / tables_of_slice of dql_ensemble.inc; and dql_score_grid.hpp.
// k_score's shape — one env per lane, workgroups of one wave, env i of every (scenario, set) has RNG key (i, seed), the same waves_per_eu — with one more
// coordinate: the blocks are scenario-major (grid_coords), so that the scenario s and the table set k of a wave are both wave-uniform.  What k_score receives
// by value in its kernel argument (SimK, MdpRun, RolloutInit) a wave of k_score_grid reads from record s of a device array, and its MdpK from element s of
// another, both through the constant address space: the arrays are written by hipMemcpy before the launch and never by a kernel, the index is wave-uniform, so
// these are scalar loads, as MdpK's already are.  The kernel argument itself holds pointers and the launch's few integers.
// What leaves the wave is its tally: one 64-bit atomicAdd per non-zero column into row (s, k) of buffers zeroed before the launch.  Integer sums: the result
// does not depend on the order the waves arrive in.
template <typename T> struct ScoreGridArgs {
  const GridScenario<T> DQL_CONST_AS* sc;                              // [n_scenarios]
  const MdpK<T> DQL_CONST_AS* mdp;                                     // [n_scenarios]
  const double* qa; const double* qb;                                  // [n_tables][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule): the scenarios share f_ag, dt and manager_div
  unsigned long long* by_code;                                         // [n_scenarios][n_tables][SCORE_N_COLS]
  unsigned long long* steps_sum;                                       // [n_scenarios][n_tables]
  unsigned long long* touch;                                           // [n_scenarios][n_tables][GRID_TOUCH_BINS]
  uint8_t* ep_code; uint16_t* ep_steps;                                // [n_scenarios][episodes][n_tables * envs_per_table], or both null
  unsigned long long seed;
  int n_tables, blocks_per_table, max_steps, episodes, n_scenarios;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_score_grid(ScoreGridArgs<T> a) {
  const int tid = threadIdx.x;
  const GridCoords gc = grid_coords(blockIdx.x, (unsigned)a.blocks_per_table, (unsigned)a.n_tables);  // wave-uniform
  if (gc.s >= a.n_scenarios) return;  // never taken unless a bug (the host sizes the grid): nothing is read or written for a scenario that is not there
  const int i = gc.env0 + tid;                                         // env within its (scenario, table set) = its RNG key
  const long long n_total = (long long)a.n_tables * a.blocks_per_table * 64;  // the lanes of one scenario = the columns of its log
  const long long g = ((long long)gc.k * a.blocks_per_table) * 64 + i;
  GridScenario<T> rec;
  __builtin_memcpy(&rec, a.sc + gc.s, sizeof(rec));
  SimK<T> cl = rec.c;
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
  const double* qa = a.qa + (size_t)gc.k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)gc.k * DQL_N_CELLS;
  const size_t log_off = (size_t)gc.s * (size_t)a.episodes * (size_t)n_total;
  const ScoreLog log{a.ep_code ? a.ep_code + log_off : nullptr, a.ep_code ? a.ep_steps + log_off : nullptr, n_total};
  const GridTally r = score_grid_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp + gc.s, rec.mr, rec.init, rec.touch_edges, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes,
                                                       a.mgr0, a.sched, kv, log, g);
  const size_t row_i = (size_t)gc.s * (size_t)a.n_tables + (size_t)gc.k;
  flush_tally(r.t, a.by_code, a.steps_sum, row_i);
  if (tid == 0) {
    unsigned long long* trow = a.touch + row_i * GRID_TOUCH_BINS;
#pragma unroll
    for (int b = 0; b < GRID_TOUCH_BINS; ++b) if (r.touch[b]) atomicAdd(&trow[b], (unsigned long long)r.touch[b]);
  }
}

extern "C" {
static thread_local LastCall g_grid_last;
// everything both entry points share, checked before the device is touched: a refused call starts no kernel
static int score_grid_check(const char* who, const dql_config* cfgs, int32_t n_scenarios, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, int32_t max_steps,
                            const int64_t* by_code, const int64_t* steps_sum, const uint8_t* ep_code, const uint16_t* ep_steps) {
  const std::string w(who);
  if (!cfgs) return fail(DQL_EINVAL, w + ": the scenario array is null; nothing was launched");
  if (n_scenarios < 1 || n_scenarios > DQL_GRID_MAX_SCENARIOS) return fail(DQL_EINVAL, w + ": n_scenarios must be in 1..1024 (DQL_GRID_MAX_SCENARIOS); nothing was launched");
  for (int s = 0; s < n_scenarios; ++s) {
    const int rc = check_config(&cfgs[s]);
    if (rc) return fail(rc, w + ": scenario " + std::to_string(s) + " is not a valid config: " + g_err + "; nothing was launched");
  }
  const dql_config& c0 = cfgs[0];
  for (int s = 1; s < n_scenarios; ++s) {
    const dql_config& c = cfgs[s];
    const char* field = c.dtype != c0.dtype ? "dtype" : c.two_axis != c0.two_axis ? "two_axis" : c.f_ag != c0.f_ag ? "f_ag" : c.dt != c0.dt ? "dt" : c.manager_div != c0.manager_div ? "manager_div" : nullptr;
    if (field)
      return fail(DQL_EINVAL, w + ": scenario " + std::to_string(s) + " differs from scenario 0 in " + field + ", which one launch must share (dtype and two_axis fix the kernel instance, f_ag, dt and manager_div the tick schedule); nothing was launched");
  }
  int rc = score_check(who, n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, ep_code, ep_steps); if (rc) return rc;
  if ((int64_t)n_scenarios * n_tables * envs_per_table > (1ll << 30)) return fail(DQL_EINVAL, w + ": scenarios x table sets x envs must be at most 2^30; nothing was launched");
  return DQL_OK;
}
static int score_grid_run(const dql_config* cfgs, int S, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, const TableSets& q,
                          int64_t* by_code, int64_t* steps_sum, int64_t* touch_hist, uint8_t* ep_code, uint16_t* ep_steps) {
  const long long n_total = n_tables * envs_per_table;  // per scenario
  const size_t rows = (size_t)S * (size_t)n_tables;
  Flight fl;  // the schedule the scenarios share; fl.mdp: one MdpK per scenario, uploaded below
  int rc = fl.setup(cfgs[0], max_steps, false); if (rc) return rc;
  DevBuf d_sc;
  // the per-scenario constants: make_simk per scenario, the Kalman fixed point (up to 200 000 iterations) once per distinct (kal_q, kal_r) in T
  rc = by_dtype(cfgs[0].dtype, [&](auto t) -> int {
    using T = decltype(t);
    std::vector<GridScenario<T>> sc((size_t)S);
    std::vector<MdpK<T>> mk((size_t)S);
    memset((void*)sc.data(), 0, sc.size() * sizeof(GridScenario<T>));
    struct Fix { T q, r; KalFix f; };
    std::vector<Fix> fixes;
    for (int s = 0; s < S; ++s) {
      const dql_config& c = cfgs[s];
      const T q = (T)c.kalman_q, r = (T)(c.noise_vel_sd * c.noise_vel_sd);
      const KalFix* kf = nullptr;
      for (const Fix& f : fixes) if (memcmp(&f.q, &q, sizeof(T)) == 0 && memcmp(&f.r, &r, sizeof(T)) == 0) { kf = &f.f; break; }
      if (!kf) {
        T pss, kss;
        kalman_fixed_point<T>(q, r, pss, kss);
        fixes.push_back(Fix{q, r, KalFix{(double)pss, (double)kss, true}});
        kf = &fixes.back().f;
      }
      sc[(size_t)s].c = make_simk<T>(c, kf);
      sc[(size_t)s].mr = MdpRun<T>{c.gamma, (T)(c.t_max * c.f_ag), c.goal_logic};
      sc[(size_t)s].init = make_rollout_init<T>(c);
      make_touch_edges<T>(c, sc[(size_t)s].touch_edges);
      mk[(size_t)s] = make_mdpk<T>(c);
    }
    UP(d_sc, sc.data(), sc.size() * sizeof(GridScenario<T>));
    UP(fl.mdp, mk.data(), mk.size() * sizeof(MdpK<T>));
    return DQL_OK;
  });
  if (rc) return rc;
  Sums sums;  // rows are (scenario, table set)
  const Sums::Slice s_by_code = sums.add(rows * SCORE_N_COLS), s_steps = sums.add(rows), s_touch = sums.add(rows * GRID_TOUCH_BINS);
  rc = sums.alloc_zeroed(); if (rc) return rc;
  EpisodeLog elog;
  rc = elog.setup(ep_code != nullptr, (size_t)S * (size_t)episodes * (size_t)n_total); if (rc) return rc;
  LastCall call;
  rc = timed_launch([&] {
    by_dtype_axes(cfgs[0].dtype, cfgs[0].two_axis, [&](auto t, auto xmode) {
      using T = decltype(t);
      constexpr int XMODE = decltype(xmode)::value;
      ScoreGridArgs<T> a;
      fill_flight_args(a, q, fl, seed, envs_per_table, max_steps);
      a.sc = (const GridScenario<T> DQL_CONST_AS*)d_sc.p; a.mdp = (const MdpK<T> DQL_CONST_AS*)fl.mdp.p;
      a.by_code = sums.dev(s_by_code); a.steps_sum = sums.dev(s_steps); a.touch = sums.dev(s_touch);
      a.ep_code = (uint8_t*)elog.code.p; a.ep_steps = (uint16_t*)elog.steps.p;
      a.n_tables = (int)n_tables; a.episodes = episodes; a.n_scenarios = S;
      call.instance<T>(TICK_PLAIN, XMODE);
      hipLaunchKernelGGL((k_score_grid<T, TICK_PLAIN, XMODE>), dim3((unsigned)((long long)S * n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
    });
  }, &call.ms);
  if (rc) return rc;
  rc = sums.down({{by_code, s_by_code}, {steps_sum, s_steps}, {touch_hist, s_touch}}); if (rc) return rc;  // touch_hist: optional
  rc = elog.down(ep_code, ep_steps); if (rc) return rc;
  g_grid_last = call;
  return DQL_OK;
}
int dql_score_grid(const dql_config* cfgs, int32_t n_scenarios, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps,
                   const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, int64_t* touch_hist_or_null, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null) {
  int rc = score_grid_check("dql_score_grid", cfgs, n_scenarios, n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, ep_code_or_null, ep_steps_or_null);
  if (rc) return rc;
  TableSets q;
  rc = q.from_host("dql_score_grid", device, n_tables, qa, qb); if (rc) return rc;
  return score_grid_run(cfgs, n_scenarios, n_tables, envs_per_table, episodes_per_env, seed, max_steps, q, by_code, steps_sum, touch_hist_or_null, ep_code_or_null, ep_steps_or_null);
}
// the learners' tables are read where they live, as dql_ensemble_score reads them: k_score_grid touches nothing else of the ensemble
int dql_ensemble_score_grid(dql_ensemble* x, const dql_config* eval_cfgs, int32_t n_scenarios, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env,
                            uint64_t seed, int32_t max_steps, int64_t* by_code, int64_t* steps_sum, int64_t* touch_hist_or_null, uint8_t* ep_code_or_null,
                            uint16_t* ep_steps_or_null) {
  CHECK_ENS(x);
  int rc = score_grid_check("dql_ensemble_score_grid", eval_cfgs, n_scenarios, count, envs_per_learner, episodes_per_env, max_steps, by_code, steps_sum, ep_code_or_null,
                            ep_steps_or_null);
  if (rc) return rc;
  TableSets q;
  rc = tables_of_slice("dql_ensemble_score_grid", x, first, count, q); if (rc) return rc;
  return score_grid_run(eval_cfgs, n_scenarios, count, envs_per_learner, episodes_per_env, seed, max_steps, q, by_code, steps_sum, touch_hist_or_null, ep_code_or_null,
                        ep_steps_or_null);
}
int dql_diag_score_grid_last(double* kernel_ms, int32_t* inst3) {
  return diag_last(g_grid_last, kernel_ms, inst3, "no dql_score_grid or dql_ensemble_score_grid call has completed on this thread");
}
}  // extern "C"
