// dql_score_map.inc: greedy scoring with a map of where the greedy decisions were made (dql_score_map / dql_ensemble_score_map, DESIGN.md section 18).  A fragment
// of dql_hip.hip's translation unit, not a header.  Needs from it: fail / HIP_TRY, by_dtype_axes, DevBuf / OUT / DOWN, check_config, TickLds; score_check and the
// family's host helpers of dql_greedy.inc (TableSets, Flight, Sums, EpisodeLog, RangeFaults, LastCall / diag_last, timed_launch, fill_greedy_args); struct
// dql_ensemble / CHECK_ENS / tables_of_slice of dql_ensemble.inc; and dql_score_map.hpp.
// k_score's shape — one env per lane, workgroups of one wave, table set k serves blocks [k B, (k + 1) B), env i of every set has RNG key (i, seed), the same
// waves_per_eu — and on top of it the wave's histogram in LDS: unsigned [DQL_N_CELLS], 11 340 B per workgroup.  The wave clears it before the first period,
// every lane adds its decisions with LDS atomics (many lanes hit one cell in the same period), and at the end the wave flushes the non-zero cells into the table
// set's row of the global map — zeroed before the launch — with atomicAdd on unsigned long long: lanes sweep contiguous cells, c = it * 64 + lane, CELL_SWEEPS
// = 45 sweeps, the last one partial (cells 2 816 .. 2 834).  Integer sums: the result does not depend on the order the waves arrive in.
// What orders clear, adds and flush: the workgroup is one wave, the LDS serves a wave's operations in the order they were issued, and the two __syncthreads()
// keep the compiler from moving an LDS access across them (and make the order hold by the language's rules as well, whatever the workgroup size).
template <typename T> struct ScoreMapArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  RolloutInit<T> init;
  const double* qa; const double* qb;                                  // [n_tables][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule)
  unsigned long long* by_code;                                         // [n_tables][SCORE_N_COLS]
  unsigned long long* steps_sum;                                       // [n_tables]
  unsigned long long* visits;                                          // [n_tables][DQL_N_CELLS]
  unsigned long long* faults;                                          // [1] writes the range checks dropped (0 unless a bug)
  ScoreMapLog log;
  unsigned long long seed;
  int blocks_per_table, max_steps, episodes, n_tables;
};
struct LdsHist {  // the wave's histogram as score_map_episodes sees it; cell is range-checked by the caller
  unsigned* h;
  __device__ __forceinline__ void add(int cell) { atomicAdd(&h[cell], 1u); }
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_score_map(ScoreMapArgs<T> a) {
  const int tid = threadIdx.x;
  const auto [k, i, g] = set_coords(a.blocks_per_table);
  if (k >= a.n_tables) {  // never taken unless a bug (the host sizes the grid): nothing is read or written for a table set that is not there
    if (tid == 0) atomicAdd(a.faults, 1ull);
    return;
  }
  SimK<T> cl = a.c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // float64: the tick's constants are read from LDS (k_step); float32: an unused byte
  __shared__ unsigned sHist[DQL_N_CELLS];
  cells_clear(sHist);
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
  }
  __syncthreads();  // the clear (and the tick constants) before the first period
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  const double* qa = a.qa + (size_t)k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)k * DQL_N_CELLS;
  LdsHist hist{sHist};
  const ScoreMapTally r = score_map_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes, a.mgr0, a.sched, kv,
                                                          a.log, g, hist);
  __syncthreads();  // the adds of every lane before the flush
  cells_flush(sHist, a.visits + (size_t)k * DQL_N_CELLS);
  if (r.faults) atomicAdd(a.faults, (unsigned long long)r.faults);
  flush_tally(r.t, a.by_code, a.steps_sum, (size_t)k);
}

extern "C" {
static thread_local LastCall g_score_map_last;
// score_check, and what the map adds to it: checked before the device is touched
static int score_map_check(const char* who, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, int32_t max_steps, const int64_t* by_code, const int64_t* steps_sum,
                           const int64_t* visits, const uint8_t* ep_code, const uint16_t* ep_steps, const uint16_t* ep_last_cell) {
  const std::string w(who);
  if (n_tables > DQL_SCORE_MAP_MAX_TABLES) return fail(DQL_EINVAL, w + ": the number of table sets must be in 1..2^14 (DQL_SCORE_MAP_MAX_TABLES: the map is 22 680 B per set); nothing was launched");
  if ((ep_code == nullptr) != (ep_last_cell == nullptr) || (ep_steps == nullptr) != (ep_last_cell == nullptr))
    return fail(DQL_EINVAL, w + ": the episode log needs all three arrays or none; nothing was launched");
  int rc = score_check(who, n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, ep_code, ep_steps); if (rc) return rc;
  if (!visits) return fail(DQL_EINVAL, w + ": null array; nothing was launched");
  return DQL_OK;
}
static int score_map_run(const char* who, const dql_config* cfg, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, const TableSets& q,
                         int64_t* by_code, int64_t* steps_sum, int64_t* visits, uint8_t* ep_code, uint16_t* ep_steps, uint16_t* ep_last_cell) {
  const long long n_total = n_tables * envs_per_table;
  Flight fl;
  int rc = fl.setup(*cfg, max_steps); if (rc) return rc;
  Sums sums;
  const Sums::Slice s_by_code = sums.add((size_t)n_tables * SCORE_N_COLS), s_steps = sums.add((size_t)n_tables), s_visits = sums.add((size_t)n_tables * DQL_N_CELLS),
                    s_faults = sums.add(1);
  rc = sums.alloc_zeroed(); if (rc) return rc;
  EpisodeLog elog;
  rc = elog.setup(ep_code != nullptr, (size_t)episodes * (size_t)n_total); if (rc) return rc;
  DevBuf d_cells;  // ep_last_cell beside the log: [2] planes of its entries
  const size_t cells_bytes = 2 * elog.entries * sizeof(uint16_t);
  if (elog.on) {
    OUT(d_cells, cells_bytes);
    HIP_TRY(hipMemset(d_cells.p, 0xff, cells_bytes));
  }
  const ScoreMapLog log{(uint8_t*)elog.code.p, (uint16_t*)elog.steps.p, (uint16_t*)d_cells.p, n_total, episodes};
  LastCall call;
  rc = timed_launch([&] {
    by_dtype_axes(cfg->dtype, cfg->two_axis, [&](auto t, auto xmode) {
      using T = decltype(t);
      constexpr int XMODE = decltype(xmode)::value;
      ScoreMapArgs<T> a;
      fill_greedy_args<T>(a, *cfg, q, fl, seed, envs_per_table, max_steps);
      a.by_code = sums.dev(s_by_code); a.steps_sum = sums.dev(s_steps); a.visits = sums.dev(s_visits); a.faults = sums.dev(s_faults);
      a.log = log; a.episodes = episodes; a.n_tables = (int)n_tables;
      call.instance<T>(TICK_PLAIN, XMODE);
      hipLaunchKernelGGL((k_score_map<T, TICK_PLAIN, XMODE>), dim3((unsigned)(n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
    });
  }, &call.ms, RangeFaults{sums.dev(s_faults), who, "kernel's", "writes"});
  if (rc) return rc;
  rc = sums.down({{by_code, s_by_code}, {steps_sum, s_steps}, {visits, s_visits}}); if (rc) return rc;
  rc = elog.down(ep_code, ep_steps); if (rc) return rc;
  if (elog.on) DOWN(ep_last_cell, d_cells, cells_bytes);
  g_score_map_last = call;
  return DQL_OK;
}
int dql_score_map(const dql_config* cfg, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps,
                  const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, int64_t* visits, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null,
                  uint16_t* ep_last_cell_or_null) {
  int rc = check_config(cfg); if (rc) return rc;
  rc = score_map_check("dql_score_map", n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, visits, ep_code_or_null, ep_steps_or_null, ep_last_cell_or_null);
  if (rc) return rc;
  TableSets q;
  rc = q.from_host("dql_score_map", device, n_tables, qa, qb); if (rc) return rc;
  return score_map_run("dql_score_map", cfg, n_tables, envs_per_table, episodes_per_env, seed, max_steps, q, by_code, steps_sum, visits, ep_code_or_null, ep_steps_or_null,
                       ep_last_cell_or_null);
}
// the learners' tables are read where they live, as dql_ensemble_score reads them: k_score_map touches nothing else of the ensemble
int dql_ensemble_score_map(dql_ensemble* x, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed,
                           int32_t max_steps, int64_t* by_code, int64_t* steps_sum, int64_t* visits, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null,
                           uint16_t* ep_last_cell_or_null) {
  CHECK_ENS(x);
  int rc = check_config(eval_cfg); if (rc) return rc;
  rc = score_map_check("dql_ensemble_score_map", count, envs_per_learner, episodes_per_env, max_steps, by_code, steps_sum, visits, ep_code_or_null, ep_steps_or_null,
                       ep_last_cell_or_null);
  if (rc) return rc;
  TableSets q;
  rc = tables_of_slice("dql_ensemble_score_map", x, first, count, q); if (rc) return rc;
  return score_map_run("dql_ensemble_score_map", eval_cfg, count, envs_per_learner, episodes_per_env, seed, max_steps, q, by_code, steps_sum, visits, ep_code_or_null,
                       ep_steps_or_null, ep_last_cell_or_null);
}
int dql_diag_score_map_last(double* kernel_ms, int32_t* inst3) {
  return diag_last(g_score_map_last, kernel_ms, inst3, "no dql_score_map or dql_ensemble_score_map call has completed on this thread");
}
}  // extern "C"
