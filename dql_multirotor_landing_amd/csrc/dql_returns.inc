// dql_returns.inc: realised discounted returns per (state, action) cell under an eps-greedy policy on fixed tables (dql_returns / dql_ensemble_returns, DESIGN.md
// section 21).  A fragment of dql_hip.hip's translation unit, not a header.  Needs from it: fail / HIP_TRY, by_dtype, DevBuf / OUT, EvTimer, check_config, TickLds,
// eps_threshold; score_check and the family's host helpers of dql_greedy.inc (TableSets, Flight, Sums, RangeFaults, LastCall / diag_last, fill_greedy_args); struct
// dql_ensemble / CHECK_ENS / tables_of_slice of dql_ensemble.inc; and dql_returns.hpp.
// A decision's return is known only when its episode ends, so it cannot be summed forward.  Two kernels, launched back to back by one call:
//   k_returns_fly    k_model's shape (one env per lane, workgroups of one wave, table set k serves blocks [k B, (k + 1) B), env i of every set has RNG key
//                    (i, seed), the same waves_per_eu) and k_model's flights (model_episodes, unchanged), with ReturnsLogSink: one 64-bit store per lane and
//                    decision into the log, column = k * envs_per_table + i.  No LDS table and no atomic in the period loop; at the end the lane writes its
//                    decision count, the wave its tally.
//   k_returns_sweep  one lane per column, the lanes of a wave walking their columns backwards together (returns_sweep).  A workgroup's lanes belong to one table
//                    set: its visits (uint32) and returns (int64) are staged in LDS, 11 340 + 22 680 = 34 020 B, cleared before the sweep and flushed at the
//                    end in sweeps of contiguous cells with zeros skipped, as k_model flushes its rewards (same-address global atomics from every wave of a
//                    set cost 3.85 x there).  RETURNS_BLOCK lanes where that divides envs_per_table (four waves share one LDS table: 4 workgroups = 16 waves
//                    per CU fit 160 KB of LDS), else 64 (4 waves per CU).
// All sums are zeroed before the launch; the log is not (n_dec says what is valid).  Integer sums of per-lane deterministic values: the result does not depend
// on the order the lanes or waves arrive in.
template <typename T> struct ReturnsFlyArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  RolloutInit<T> init;
  const double* qa; const double* qb;                                  // [n_tables][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule)
  unsigned long long* traj;                                            // [max_steps + 1][n_columns] the decision log
  unsigned* n_dec;                                                     // [n_columns]
  unsigned long long* by_code;                                         // [n_tables][SCORE_N_COLS]
  unsigned long long* steps_sum;                                       // [n_tables]
  unsigned long long* faults;                                          // [1] contributions the range checks dropped (0 unless a bug)
  unsigned long long seed;
  long long n_columns;
  unsigned eps_thr;
  int blocks_per_table, max_steps, episodes, n_tables;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_returns_fly(ReturnsFlyArgs<T> a) {
  const int tid = threadIdx.x;
  const auto [k, i, g] = set_coords(a.blocks_per_table);
  const size_t column = (size_t)g;                                     // = k * envs_per_table + i
  if (k >= a.n_tables || (size_t)blockIdx.x * 64 + 64 > (size_t)a.n_columns) {  // never taken unless a bug (the host sizes the grid): nothing is read or written
    if (tid == 0) atomicAdd(a.faults, 1ull);
    return;
  }
  SimK<T> cl = a.c;
  cl.two_axis = 0;  // XMODE == X_ONLY (model_episodes asserts it)
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
  const double* qa = a.qa + (size_t)k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)k * DQL_N_CELLS;
  ReturnsLogSink<unsigned long long*> sink{a.traj, (size_t)a.n_columns, column, (unsigned)(a.max_steps + 1)};
  const ModelTally r = model_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes, a.eps_thr, a.mgr0, a.sched, kv, sink);
  a.n_dec[column] = sink.n_dec;
  if (r.faults + sink.faults) atomicAdd(a.faults, (unsigned long long)(r.faults + sink.faults));
  flush_tally(r.t, a.by_code, a.steps_sum, (size_t)k);
}

struct ReturnsSweepArgs {
  const unsigned long long* traj;                                      // [max_steps + 1][n_columns]
  const unsigned* n_dec;                                               // [n_columns]
  unsigned long long* visits;                                          // [n_tables][DQL_N_CELLS]
  unsigned long long* return_fx;                                       // [n_tables][DQL_N_CELLS]
  unsigned long long* cut;                                             // [n_tables]
  unsigned long long* faults;                                          // [1]
  double gamma, g_bound;
  long long n_columns, envs_per_table;
  int max_steps, n_tables;
};
constexpr int RETURNS_BLOCK = 256;
struct LdsReturnsAcc {  // the workgroup's two tables; cell is range-checked by the caller
  unsigned* v; unsigned long long* g;
  __device__ __forceinline__ void add(int cell, long long g_fx) {
    atomicAdd(&v[cell], 1u);
    if (g_fx) atomicAdd(&g[cell], (unsigned long long)g_fx);
  }
};
template <int BLOCK> __global__ __launch_bounds__(BLOCK) void k_returns_sweep(ReturnsSweepArgs a) {
  static_assert(BLOCK % 64 == 0, "whole waves");
  const int tid = threadIdx.x;
  const size_t column = (size_t)blockIdx.x * BLOCK + (size_t)tid;
  const long long k = (long long)((size_t)blockIdx.x * BLOCK / (size_t)a.envs_per_table);  // table set (uniform: BLOCK divides envs_per_table)
  if (k >= a.n_tables || (size_t)blockIdx.x * BLOCK + BLOCK > (size_t)a.n_columns) {  // never taken unless a bug (the host sizes the grid)
    if (tid == 0) atomicAdd(a.faults, 1ull);
    return;
  }
  __shared__ unsigned sVisits[DQL_N_CELLS];
  __shared__ unsigned long long sReturn[DQL_N_CELLS];
  __shared__ unsigned long long sCut;
  __shared__ unsigned sFaults;
  for (int c = tid; c < DQL_N_CELLS; c += BLOCK) { sVisits[c] = 0u; sReturn[c] = 0ull; }
  if (tid == 0) { sCut = 0ull; sFaults = 0u; }
  __syncthreads();  // the clear before the first add
  const unsigned n_dec = a.n_dec[column];
  const unsigned capacity = (unsigned)(a.max_steps + 1);
  unsigned top = n_dec <= capacity ? n_dec : 0u;  // the wave's largest decision count: its lanes walk backwards together
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)top, off, 64);
    top = other > top ? other : top;
  }
  LdsReturnsAcc acc{sVisits, sReturn};
  const ReturnsSweepTally r = returns_sweep(a.traj, (size_t)a.n_columns, column, n_dec, capacity, (int)top, a.gamma, a.g_bound, acc);
  if (r.cut) atomicAdd(&sCut, r.cut);
  if (r.faults) atomicAdd(&sFaults, r.faults);
  __syncthreads();  // the adds of every lane before the flush
  unsigned long long* row_v = a.visits + (size_t)k * DQL_N_CELLS;
  unsigned long long* row_g = a.return_fx + (size_t)k * DQL_N_CELLS;
  for (int c = tid; c < DQL_N_CELLS; c += BLOCK) {
    const unsigned v = sVisits[c];
    const unsigned long long g = sReturn[c];
    if (v) atomicAdd(&row_v[c], (unsigned long long)v);
    if (g) atomicAdd(&row_g[c], g);
  }
  if (tid == 0) {
    if (sCut) atomicAdd(&a.cut[k], sCut);
    if (sFaults) atomicAdd(a.faults, (unsigned long long)sFaults);
  }
}

// R of the overflow guard: the per-step reward bound DqlConfig.max_abs_td_target is built on, term for term (config.py max_abs_reward)
static double returns_reward_bound(const dql_config& c) {
  const double dt = 1.0 / c.f_ag;
  double r = 0.0;
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) {
    const double rp = std::fabs(c.w_p) * c.lim_v[k] * dt, rv = std::fabs(c.w_v) * c.lim_a[k] * dt;
    const double rth_max = std::fabs(c.w_theta) * (c.delta_theta / c.theta_max) * c.lim_v[k];
    const double rd = std::fabs(c.w_dur) * c.lim_v[k] * dt;
    const double rth = std::fabs(c.w_theta) * std::fabs(c.w_theta) / c.theta_max * c.lim_v[k];
    r = std::fmax(r, rp + rv + rth + rd + std::fmax(std::fabs(c.w_succ), std::fabs(c.w_fail)) * (rp + rv + rth_max + rd));
  }
  return r;
}
// ceil(B 2^26), B = R min(1 / (1 - gamma), max_steps + 1) (1 + 2^-10): no |return-to-go| in fixed point exceeds it while |reward| <= R
static double returns_g_bound(const dql_config& c, double gamma, int max_steps) {
  const double horizon = gamma >= 1.0 ? (double)(max_steps + 1) : std::fmin(1.0 / (1.0 - gamma), (double)(max_steps + 1));
  return std::ceil(returns_reward_bound(c) * horizon * (1.0 + 0x1p-10) * (double)(1ll << DQL_TARGET_FRAC_BITS));
}

extern "C" {
static thread_local LastCall g_returns_last;  // ms: fly, ms2: sweep
// everything both entry points share, checked before the device is touched: a refused call starts no kernel
static int returns_check(const char* who, const dql_config* cfg, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, int32_t max_steps, double eps, double gamma,
                         const int64_t* visits, const int64_t* return_fx, const int64_t* cut_decisions, const int64_t* by_code, const int64_t* steps_sum) {
  const std::string w(who);
  if (cfg->two_axis) return fail(DQL_EINVAL, w + ": a two-axis config is refused: the returns are the x MDP's, and the reward is not kept per axis; nothing was launched");
  if (n_tables < 1 || n_tables > DQL_SCORE_MAP_MAX_TABLES)
    return fail(DQL_EINVAL, w + ": the number of table sets must be in 1..2^14 (DQL_SCORE_MAP_MAX_TABLES); nothing was launched");
  if (!visits || !return_fx || !cut_decisions) return fail(DQL_EINVAL, w + ": null array; nothing was launched");
  int rc = score_check(who, n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, nullptr, nullptr); if (rc) return rc;
  if (n_tables * envs_per_table * ((int64_t)max_steps + 1) > (1ll << 29))
    return fail(DQL_EINVAL, w + ": table sets x envs x (max_steps + 1) must be at most 2^29: the decision log is one 64-bit word per possible decision, 4 GiB there; nothing was launched");
  if (!(eps >= 0.0 && eps <= 1.0)) return fail(DQL_EINVAL, w + ": eps must be in [0, 1]; nothing was launched");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(DQL_EINVAL, w + ": gamma must be in [0, 1]; nothing was launched");
  const double bound = returns_g_bound(*cfg, gamma, max_steps);
  const unsigned __int128 most = (unsigned __int128)envs_per_table * (unsigned __int128)(max_steps + 1);
  if (!(bound < 0x1p62) || ((unsigned __int128)bound + 1) * most > (unsigned __int128)INT64_MAX)
    return fail(DQL_EINVAL, w + ": envs_per_table * (max_steps + 1) returns of up to R min(1 / (1 - gamma), max_steps + 1) could overflow one int64 cell of return_fx: fly "
                            "fewer envs per call and add the results of several seeds; nothing was launched");
  return DQL_OK;
}
static int returns_run(const char* who, const dql_config* cfg, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, double eps, double gamma,
                       const TableSets& q, int64_t* visits, int64_t* return_fx, int64_t* cut_decisions, int64_t* by_code, int64_t* steps_sum) {
  const long long n_columns = n_tables * envs_per_table;
  Flight fl;
  int rc = fl.setup(*cfg, max_steps); if (rc) return rc;
  Sums sums;
  const Sums::Slice s_by_code = sums.add((size_t)n_tables * SCORE_N_COLS), s_steps = sums.add((size_t)n_tables), s_cut = sums.add((size_t)n_tables),
                    s_visits = sums.add((size_t)n_tables * DQL_N_CELLS), s_return = sums.add((size_t)n_tables * DQL_N_CELLS), s_faults = sums.add(1);
  rc = sums.alloc_zeroed(); if (rc) return rc;
  DevBuf d_traj, d_ndec;  // the decision log (not zeroed: n_dec says what is valid) in a buffer of its own, the decision counts beside it
  OUT(d_traj, (size_t)(max_steps + 1) * (size_t)n_columns * sizeof(unsigned long long));
  OUT(d_ndec, (size_t)n_columns * sizeof(unsigned));
  HIP_TRY(hipMemset(d_ndec.p, 0, (size_t)n_columns * sizeof(unsigned)));
  // two stretches: the flight from t_fly's first event to t_sweep's first, the sweep between t_sweep's two
  EvTimer t_fly, t_sweep;
  rc = t_fly.start(); if (rc) return rc;
  LastCall call;
  by_dtype(cfg->dtype, [&](auto t) {
    using T = decltype(t);
    ReturnsFlyArgs<T> a;
    fill_greedy_args<T>(a, *cfg, q, fl, seed, envs_per_table, max_steps);
    a.traj = (unsigned long long*)d_traj.p; a.n_dec = (unsigned*)d_ndec.p; a.by_code = sums.dev(s_by_code); a.steps_sum = sums.dev(s_steps); a.faults = sums.dev(s_faults);
    a.n_columns = n_columns; a.eps_thr = eps_threshold(eps); a.episodes = episodes; a.n_tables = (int)n_tables;
    call.instance<T>(TICK_PLAIN, X_ONLY);
    hipLaunchKernelGGL((k_returns_fly<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)(n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
  });
  HIP_TRY(hipGetLastError());
  rc = t_sweep.start(); if (rc) return rc;  // its first event closes the flight's stretch
  const ReturnsSweepArgs s{(const unsigned long long*)d_traj.p, (const unsigned*)d_ndec.p, sums.dev(s_visits), sums.dev(s_return), sums.dev(s_cut), sums.dev(s_faults), gamma,
                           returns_g_bound(*cfg, gamma, max_steps), n_columns, envs_per_table, max_steps, (int)n_tables};
  if (envs_per_table % RETURNS_BLOCK == 0) hipLaunchKernelGGL((k_returns_sweep<RETURNS_BLOCK>), dim3((unsigned)(n_columns / RETURNS_BLOCK)), dim3(RETURNS_BLOCK), 0, 0, s);
  else hipLaunchKernelGGL((k_returns_sweep<64>), dim3((unsigned)(n_columns / 64)), dim3(64), 0, 0, s);
  HIP_TRY(hipGetLastError());
  rc = t_sweep.stop_ms(&call.ms2); if (rc) return rc;
  float fly_ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&fly_ms, t_fly.e0, t_sweep.e0));
  call.ms = (double)fly_ms;
  rc = RangeFaults{sums.dev(s_faults), who, "kernels'", "contributions"}.refuse_if_any(); if (rc) return rc;
  rc = sums.down({{by_code, s_by_code}, {steps_sum, s_steps}, {cut_decisions, s_cut}, {visits, s_visits}, {return_fx, s_return}}); if (rc) return rc;
  g_returns_last = call;
  return DQL_OK;
}
int dql_returns(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, double eps, double gamma,
                const double* qa, const double* qb, int64_t* visits, int64_t* return_fx, int64_t* cut_decisions, int64_t* by_code, int64_t* steps_sum) {
  int rc = check_config(cfg); if (rc) return rc;
  rc = returns_check("dql_returns", cfg, n_tables, envs_per_table, episodes_per_env, max_steps, eps, gamma, visits, return_fx, cut_decisions, by_code, steps_sum); if (rc) return rc;
  TableSets q;
  rc = q.from_host("dql_returns", device, n_tables, qa, qb); if (rc) return rc;
  return returns_run("dql_returns", cfg, n_tables, envs_per_table, episodes_per_env, seed, max_steps, eps, gamma, q, visits, return_fx, cut_decisions, by_code, steps_sum);
}
// the learners' tables are read where they live, as dql_ensemble_model reads them: the kernels touch nothing else of the ensemble
int dql_ensemble_returns(dql_ensemble* x, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed,
                         int32_t max_steps, double eps, double gamma, int64_t* visits, int64_t* return_fx, int64_t* cut_decisions, int64_t* by_code, int64_t* steps_sum) {
  CHECK_ENS(x);
  int rc = check_config(eval_cfg); if (rc) return rc;
  rc = returns_check("dql_ensemble_returns", eval_cfg, count, envs_per_learner, episodes_per_env, max_steps, eps, gamma, visits, return_fx, cut_decisions, by_code, steps_sum);
  if (rc) return rc;
  TableSets q;
  rc = tables_of_slice("dql_ensemble_returns", x, first, count, q); if (rc) return rc;
  return returns_run("dql_ensemble_returns", eval_cfg, count, envs_per_learner, episodes_per_env, seed, max_steps, eps, gamma, q, visits, return_fx, cut_decisions, by_code, steps_sum);
}
int dql_diag_returns_last(double* fly_ms, double* sweep_ms, int32_t* inst3) {
  return diag_last(g_returns_last, fly_ms, sweep_ms, inst3, "no dql_returns or dql_ensemble_returns call has completed on this thread");
}
}  // extern "C"
