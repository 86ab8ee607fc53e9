// dql_model.inc: the empirical transition model of the discretised x MDP under an eps-greedy policy on fixed tables (dql_model / dql_ensemble_model, DESIGN.md
// section 19).  A fragment of dql_hip.hip's translation unit, not a header.  Needs from it: fail / HIP_TRY, by_dtype, DevBuf / OUT / DOWN, check_config, TickLds,
// eps_threshold; score_check and the family's host helpers of dql_greedy.inc (TableSets, Flight, Sums, RangeFaults, LastCall / diag_last, timed_launch,
// fill_greedy_args); struct dql_ensemble / CHECK_ENS / tables_of_slice of dql_ensemble.inc; and dql_model.hpp.
// k_score_map's shape — one env per lane, workgroups of one wave, table set k serves blocks [k B, (k + 1) B), env i of every set has RNG key (i, seed), the same
// waves_per_eu.  Where the counts go:
//   pairs     the pair table of a set (uint32 [DQL_N_CELLS][DQL_N_STATES], 10.7 MB) does not fit LDS: returnless 32-bit atomic adds into global memory.  Lanes
//             of a wave that count the same (cell, s') in the same period — the rule at level 4, not the exception — leave as ONE add of their number: a loop
//             over the wave's distinct keys (the first lane still waiting broadcasts its key, the lanes that hold it are counted with a ballot and leave),
//             64 trips at most.  A sum of ones or their count: not a bit of the result changes.
//   reward    staged in the wave's LDS table, unsigned long long [DQL_N_CELLS] (22 680 B per workgroup), with LDS atomics, as k_score_map stages its
//             histogram: cleared before the first period, flushed at the end into the set's row with one 64-bit global atomic per non-zero cell (lanes sweep
//             contiguous cells, c = it * 64 + lane).  Two's-complement sums: the order does not matter.
//   terminal  once per episode and lane: 64-bit global atomics.
// All tables are zeroed before the launch.  Integer sums: the result does not depend on the order the lanes or waves arrive in.  No count can overflow: a pair
// count is at most envs_per_table * (max_steps + 1) < 2^32 (model_check).  What orders clear, adds and flush of the LDS table: as in dql_score_map.inc.
template <typename T> struct ModelArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  RolloutInit<T> init;
  const double* qa; const double* qb;                                  // [n_tables][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule)
  unsigned* pairs;                                                     // [n_tables][DQL_N_CELLS][DQL_N_STATES]
  unsigned long long* reward_fx;                                       // [n_tables][DQL_N_CELLS]
  unsigned long long* terminal;                                        // [n_tables][DQL_N_CELLS][DQL_N_CHECK_CODES]
  unsigned long long* by_code;                                         // [n_tables][SCORE_N_COLS]
  unsigned long long* steps_sum;                                       // [n_tables]
  unsigned long long* faults;                                          // [1] contributions the range checks dropped (0 unless a bug)
  unsigned long long seed;
  unsigned eps_thr;
  int blocks_per_table, max_steps, episodes, n_tables;
};
struct WaveModelSink {  // the table set's tables as model_episodes sees them; cell, next and code are range-checked by the caller
  unsigned* p; unsigned long long* t; unsigned long long* r_lds; int lane;
  __device__ __forceinline__ void pair(int cell, int next) {
    const unsigned key = (unsigned)cell * (unsigned)DQL_N_STATES + (unsigned)next;  // < 2 679 075
    bool sent = false;
    for (int trip = 0; trip < 64; ++trip) {  // one distinct key of the wave per trip
      const unsigned k = __builtin_amdgcn_readfirstlane(key);
      if (key == k) {
        const unsigned long long same = __ballot(1);  // the lanes still here that hold this key
        if (lane == __builtin_ctzll(same)) atomicAdd(&p[k], (unsigned)__builtin_popcountll(same));
        sent = true;
        break;
      }
    }
    if (!sent) atomicAdd(&p[key], 1u);  // never reached (the first lane waiting always holds its own key): no count is lost if it were
  }
  __device__ __forceinline__ void terminal(int cell, int code) { atomicAdd(&t[(size_t)cell * DQL_N_CHECK_CODES + (size_t)code], 1ull); }
  __device__ __forceinline__ void reward(int cell, long long fx) { if (fx) atomicAdd(&r_lds[cell], (unsigned long long)fx); }
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_model(ModelArgs<T> a) {
  const int tid = threadIdx.x;
  const auto [k, i, g] = set_coords(a.blocks_per_table);  // g: not used, the model has no per-lane output
  if (k >= a.n_tables) {  // never taken unless a bug (the host sizes the grid): nothing is read or written for a table set that is not there
    if (tid == 0) atomicAdd(a.faults, 1ull);
    return;
  }
  SimK<T> cl = a.c;
  cl.two_axis = 0;  // XMODE == X_ONLY (model_episodes asserts it)
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // float64: the tick's constants are read from LDS (k_step); float32: an unused byte
  __shared__ unsigned long long sReward[DQL_N_CELLS];
  cells_clear(sReward);
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
  }
  __syncthreads();  // the clear (and the tick constants) before the first period
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  const double* qa = a.qa + (size_t)k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)k * DQL_N_CELLS;
  WaveModelSink sink{a.pairs + (size_t)k * DQL_N_CELLS * DQL_N_STATES, a.terminal + (size_t)k * DQL_N_CELLS * DQL_N_CHECK_CODES, sReward, tid};
  const ModelTally r = model_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes, a.eps_thr, a.mgr0, a.sched, kv, sink);
  __syncthreads();  // the adds of every lane before the flush
  cells_flush(sReward, a.reward_fx + (size_t)k * DQL_N_CELLS);
  if (r.faults) atomicAdd(a.faults, (unsigned long long)r.faults);
  flush_tally(r.t, a.by_code, a.steps_sum, (size_t)k);
}

extern "C" {
static thread_local LastCall g_model_last;
// everything both entry points share, checked before the device is touched: a refused call starts no kernel
static int model_check(const char* who, const dql_config* cfg, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, int32_t max_steps, double eps,
                       const uint32_t* pairs, const int64_t* reward_fx, const int64_t* terminal, const int64_t* by_code, const int64_t* steps_sum) {
  const std::string w(who);
  if (cfg->two_axis) return fail(DQL_EINVAL, w + ": a two-axis config is refused: the model is the x MDP's, and the reward is not kept per axis; nothing was launched");
  if (n_tables < 1 || n_tables > DQL_MODEL_MAX_TABLES)
    return fail(DQL_EINVAL, w + ": the number of table sets must be in 1..16 (DQL_MODEL_MAX_TABLES: the pair table is 10.7 MB per set); nothing was launched");
  if (!pairs || !reward_fx || !terminal) return fail(DQL_EINVAL, w + ": null array; nothing was launched");
  int rc = score_check(who, n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, nullptr, nullptr); if (rc) return rc;
  if (envs_per_table * ((int64_t)max_steps + 1) >= (1ll << 32))
    return fail(DQL_EINVAL, w + ": envs_per_table * (max_steps + 1) must be below 2^32, so that no 32-bit pair count can overflow; nothing was launched");
  if (!(eps >= 0.0 && eps <= 1.0)) return fail(DQL_EINVAL, w + ": eps must be in [0, 1]; nothing was launched");
  return DQL_OK;
}
static int model_run(const char* who, const dql_config* cfg, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, double eps,
                     const TableSets& q, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal, int64_t* by_code, int64_t* steps_sum) {
  Flight fl;
  int rc = fl.setup(*cfg, max_steps); if (rc) return rc;
  Sums sums;
  const Sums::Slice s_by_code = sums.add((size_t)n_tables * SCORE_N_COLS), s_steps = sums.add((size_t)n_tables), s_reward = sums.add((size_t)n_tables * DQL_N_CELLS),
                    s_terminal = sums.add((size_t)n_tables * DQL_N_CELLS * DQL_N_CHECK_CODES), s_faults = sums.add(1);
  rc = sums.alloc_zeroed(); if (rc) return rc;
  DevBuf d_pairs;  // the 32-bit pair tables in a buffer of their own
  const size_t pairs_bytes = (size_t)n_tables * DQL_N_CELLS * DQL_N_STATES * sizeof(uint32_t);
  OUT(d_pairs, pairs_bytes);
  HIP_TRY(hipMemset(d_pairs.p, 0, pairs_bytes));
  LastCall call;
  rc = timed_launch([&] {
    by_dtype(cfg->dtype, [&](auto t) {
      using T = decltype(t);
      ModelArgs<T> a;
      fill_greedy_args<T>(a, *cfg, q, fl, seed, envs_per_table, max_steps);
      a.pairs = (unsigned*)d_pairs.p; a.reward_fx = sums.dev(s_reward); a.terminal = sums.dev(s_terminal); a.by_code = sums.dev(s_by_code); a.steps_sum = sums.dev(s_steps);
      a.faults = sums.dev(s_faults); a.eps_thr = eps_threshold(eps); a.episodes = episodes; a.n_tables = (int)n_tables;
      call.instance<T>(TICK_PLAIN, X_ONLY);
      hipLaunchKernelGGL((k_model<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)(n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
    });
  }, &call.ms, RangeFaults{sums.dev(s_faults), who, "kernel's", "contributions"});
  if (rc) return rc;
  rc = sums.down({{by_code, s_by_code}, {steps_sum, s_steps}, {reward_fx, s_reward}, {terminal, s_terminal}}); if (rc) return rc;
  DOWN(pairs, d_pairs, pairs_bytes);
  g_model_last = call;
  return DQL_OK;
}
int dql_model(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, double eps,
              const double* qa, const double* qb, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal, int64_t* by_code, int64_t* steps_sum) {
  int rc = check_config(cfg); if (rc) return rc;
  rc = model_check("dql_model", cfg, n_tables, envs_per_table, episodes_per_env, max_steps, eps, pairs, reward_fx, terminal, by_code, steps_sum); if (rc) return rc;
  TableSets q;
  rc = q.from_host("dql_model", device, n_tables, qa, qb); if (rc) return rc;
  return model_run("dql_model", cfg, n_tables, envs_per_table, episodes_per_env, seed, max_steps, eps, q, pairs, reward_fx, terminal, by_code, steps_sum);
}
// the learners' tables are read where they live, as dql_ensemble_score_map reads them: k_model touches nothing else of the ensemble
int dql_ensemble_model(dql_ensemble* x, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed,
                       int32_t max_steps, double eps, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal, int64_t* by_code, int64_t* steps_sum) {
  CHECK_ENS(x);
  int rc = check_config(eval_cfg); if (rc) return rc;
  rc = model_check("dql_ensemble_model", eval_cfg, count, envs_per_learner, episodes_per_env, max_steps, eps, pairs, reward_fx, terminal, by_code, steps_sum); if (rc) return rc;
  TableSets q;
  rc = tables_of_slice("dql_ensemble_model", x, first, count, q); if (rc) return rc;
  return model_run("dql_ensemble_model", eval_cfg, count, envs_per_learner, episodes_per_env, seed, max_steps, eps, q, pairs, reward_fx, terminal, by_code, steps_sum);
}
int dql_diag_model_last(double* kernel_ms, int32_t* inst3) {
  return diag_last(g_model_last, kernel_ms, inst3, "no dql_model or dql_ensemble_model call has completed on this thread");
}
}  // extern "C"
