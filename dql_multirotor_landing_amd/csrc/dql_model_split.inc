// dql_model_split.inc: the transition model split by one bit of hidden state (dql_model_split / dql_ensemble_model_split, DESIGN.md section 32).  A fragment of
// dql_hip.hip's translation unit, not a header.  Needs what dql_model.inc needs and dql_model.inc itself (ModelArgs' layout is repeated, model_check and
// WaveModelSink's merge are used), and dql_model_split.hpp.
// k_model's shape — one env per lane, workgroups of one wave, table set k serves blocks [k B, (k + 1) B), env i of every set has RNG key (i, seed), the same
// waves_per_eu.  Where the counts go:
//   pairs        returnless 32-bit global atomics with k_model's in-wave merge of equal keys; the key is (half * DQL_N_CELLS + cell) * DQL_N_STATES + s' < 5 358 150:
//                the half is part of the key (WaveModelSink::pair with the row half * DQL_N_CELLS + cell of a table of 2 * DQL_N_CELLS rows)
//   reward       staged in LDS, unsigned long long [2][DQL_N_CELLS] (45 360 B), flushed with one 64-bit global atomic per non-zero cell
//   feature sums staged in LDS too, unsigned long long [DQL_N_STATES] (7 560 B): at level 4 most lanes of a wave sit in a handful of states, so a global
//                atomic per decision would queue on a few addresses in every period; 52 920 B a workgroup still lets three one-wave workgroups share a CU's
//                160 KB, as 45 360 B would (DESIGN.md section 32)
//   terminal     once per episode and lane: 64-bit global atomics
// cut is read from global memory by the state before the period, one load per counted decision.  All tables are zeroed before the launch.  Integer sums:
// the result does not depend on the order the lanes or waves arrive in.  feat_sum_fx cannot overflow: |value| 2^20 < 2^33, and a state is visited fewer than
// envs_per_table * (max_steps + 1) < 2^30 times (model_split_check).
template <typename T> struct ModelSplitArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  RolloutInit<T> init;
  const double* qa; const double* qb;                                  // [n_tables][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule)
  const double* cut;                                                   // [DQL_N_STATES]
  unsigned* pairs;                                                     // [n_tables][2][DQL_N_CELLS][DQL_N_STATES]
  unsigned long long* reward_fx;                                       // [n_tables][2][DQL_N_CELLS]
  unsigned long long* terminal;                                        // [n_tables][2][DQL_N_CELLS][DQL_N_CHECK_CODES]
  unsigned long long* feat_sum_fx;                                     // [n_tables][DQL_N_STATES]
  unsigned long long* by_code;                                         // [n_tables][SCORE_N_COLS]
  unsigned long long* steps_sum;                                       // [n_tables]
  unsigned long long* faults;                                          // [1] contributions the range checks dropped (0 unless a bug)
  unsigned long long seed;
  unsigned eps_thr;
  int blocks_per_table, max_steps, episodes, n_tables, feature;
};
constexpr int SPLIT_ROWS = 2 * DQL_N_CELLS;
// a one-wave workgroup's LDS table of n 64-bit cells, swept as cells_clear / cells_flush sweep theirs (c = it * 64 + lane)
__device__ __forceinline__ void split_clear(unsigned long long* cells, int n) {
#pragma unroll 1
  for (int c = (int)threadIdx.x; c < n; c += 64) cells[c] = 0ull;
}
__device__ __forceinline__ void split_flush(const unsigned long long* cells, unsigned long long* row, int n) {
#pragma unroll 1
  for (int c = (int)threadIdx.x; c < n; c += 64) {
    const unsigned long long v = cells[c];
    if (v) atomicAdd(&row[c], v);
  }
}
struct WaveSplitSink {  // the table set's tables as model_split_episodes sees them; half, cell, next, code and state are range-checked by the caller
  WaveModelSink rows;   // p / t / r_lds over 2 * DQL_N_CELLS rows: row = half * DQL_N_CELLS + cell
  unsigned long long* f_lds;
  __device__ __forceinline__ void pair(int half, int cell, int next) { rows.pair(half * DQL_N_CELLS + cell, next); }
  __device__ __forceinline__ void terminal(int half, int cell, int code) { rows.terminal(half * DQL_N_CELLS + cell, code); }
  __device__ __forceinline__ void reward(int half, int cell, long long fx) { rows.reward(half * DQL_N_CELLS + cell, fx); }
  __device__ __forceinline__ void feature(int state, long long fx) { if (fx) atomicAdd(&f_lds[state], (unsigned long long)fx); }
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_model_split(ModelSplitArgs<T> a) {
  const int tid = threadIdx.x;
  const auto [k, i, g] = set_coords(a.blocks_per_table);  // g: not used, the model has no per-lane output
  if (k >= a.n_tables) {  // never taken unless a bug (the host sizes the grid): nothing is read or written for a table set that is not there
    if (tid == 0) atomicAdd(a.faults, 1ull);
    return;
  }
  SimK<T> cl = a.c;
  cl.two_axis = 0;  // XMODE == X_ONLY (model_split_episodes asserts it)
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // float64: the tick's constants are read from LDS (k_step); float32: an unused byte
  __shared__ unsigned long long sReward[SPLIT_ROWS];
  __shared__ unsigned long long sFeature[DQL_N_STATES];
  split_clear(sReward, SPLIT_ROWS);
  split_clear(sFeature, DQL_N_STATES);
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
  }
  __syncthreads();  // the clears (and the tick constants) before the first period
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  const double* qa = a.qa + (size_t)k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)k * DQL_N_CELLS;
  WaveSplitSink sink{WaveModelSink{a.pairs + (size_t)k * SPLIT_ROWS * DQL_N_STATES, a.terminal + (size_t)k * SPLIT_ROWS * DQL_N_CHECK_CODES, sReward, tid}, sFeature};
  const ModelSplitTally r = model_split_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes, a.eps_thr, a.feature,
                                                              a.cut, a.mgr0, a.sched, kv, sink);
  __syncthreads();  // the adds of every lane before the flushes
  split_flush(sReward, a.reward_fx + (size_t)k * SPLIT_ROWS, SPLIT_ROWS);
  split_flush(sFeature, a.feat_sum_fx + (size_t)k * DQL_N_STATES, DQL_N_STATES);
  if (r.faults) atomicAdd(a.faults, (unsigned long long)r.faults);
  flush_tally(r.t, a.by_code, a.steps_sum, (size_t)k);
}

extern "C" {
static thread_local LastCall g_model_split_last;
// everything both entry points share, checked before the device is touched: a refused call starts no kernel
static int model_split_check(const char* who, const dql_config* cfg, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, int32_t max_steps, double eps,
                             int32_t feature, const double* cut, const uint32_t* pairs, const int64_t* reward_fx, const int64_t* terminal, const int64_t* feat_sum_fx,
                             const int64_t* by_code, const int64_t* steps_sum) {
  const std::string w(who);
  if (n_tables < 1 || n_tables > DQL_MODEL_SPLIT_MAX_TABLES)
    return fail(DQL_EINVAL, w + ": the number of table sets must be in 1..8 (DQL_MODEL_SPLIT_MAX_TABLES: the pair table is 21.4 MB per set); nothing was launched");
  if (!cut || !feat_sum_fx) return fail(DQL_EINVAL, w + ": null array; nothing was launched");
  int rc = model_check(who, cfg, n_tables, envs_per_table, episodes_per_env, max_steps, eps, pairs, reward_fx, terminal, by_code, steps_sum); if (rc) return rc;
  if (envs_per_table * ((int64_t)max_steps + 1) >= (1ll << 30))
    return fail(DQL_EINVAL, w + ": envs_per_table * (max_steps + 1) must be below 2^30, so that no 64-bit feature sum can overflow; nothing was launched");
  if (feature < 0 || feature >= DQL_SPLIT_N_FEATURES) return fail(DQL_EINVAL, w + ": feature must be one of DQL_SPLIT_* (0..10); nothing was launched");
  for (int s = 0; s < DQL_N_STATES; ++s)
    if (cut[s] != cut[s]) return fail(DQL_EINVAL, w + ": cut holds a NaN at state " + std::to_string(s) + " (+-inf are allowed); nothing was launched");
  return DQL_OK;
}
static int model_split_run(const char* who, const dql_config* cfg, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, double eps,
                           int feature, const double* cut, const TableSets& q, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal, int64_t* feat_sum_fx,
                           int64_t* by_code, int64_t* steps_sum) {
  Flight fl;
  int rc = fl.setup(*cfg, max_steps); if (rc) return rc;
  Sums sums;
  const Sums::Slice s_by_code = sums.add((size_t)n_tables * SCORE_N_COLS), s_steps = sums.add((size_t)n_tables), s_reward = sums.add((size_t)n_tables * SPLIT_ROWS),
                    s_terminal = sums.add((size_t)n_tables * SPLIT_ROWS * DQL_N_CHECK_CODES), s_feature = sums.add((size_t)n_tables * DQL_N_STATES), s_faults = sums.add(1);
  rc = sums.alloc_zeroed(); if (rc) return rc;
  DevBuf d_pairs, d_cut;  // the 32-bit pair tables in a buffer of their own; the cut, uploaded once per call
  const size_t pairs_bytes = (size_t)n_tables * SPLIT_ROWS * DQL_N_STATES * sizeof(uint32_t);
  OUT(d_pairs, pairs_bytes);
  HIP_TRY(hipMemset(d_pairs.p, 0, pairs_bytes));
  UP(d_cut, cut, (size_t)DQL_N_STATES * sizeof(double));
  LastCall call;
  rc = timed_launch([&] {
    by_dtype(cfg->dtype, [&](auto t) {
      using T = decltype(t);
      ModelSplitArgs<T> a;
      fill_greedy_args<T>(a, *cfg, q, fl, seed, envs_per_table, max_steps);
      a.cut = (const double*)d_cut.p; a.pairs = (unsigned*)d_pairs.p; a.reward_fx = sums.dev(s_reward); a.terminal = sums.dev(s_terminal); a.feat_sum_fx = sums.dev(s_feature);
      a.by_code = sums.dev(s_by_code); a.steps_sum = sums.dev(s_steps); a.faults = sums.dev(s_faults); a.eps_thr = eps_threshold(eps); a.episodes = episodes;
      a.n_tables = (int)n_tables; a.feature = feature;
      call.instance<T>(TICK_PLAIN, X_ONLY);
      hipLaunchKernelGGL((k_model_split<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)(n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
    });
  }, &call.ms, RangeFaults{sums.dev(s_faults), who, "kernel's", "contributions"});
  if (rc) return rc;
  rc = sums.down({{by_code, s_by_code}, {steps_sum, s_steps}, {reward_fx, s_reward}, {terminal, s_terminal}, {feat_sum_fx, s_feature}}); if (rc) return rc;
  DOWN(pairs, d_pairs, pairs_bytes);
  g_model_split_last = call;
  return DQL_OK;
}
int dql_model_split(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, double eps,
                    int32_t feature, const double* cut, const double* qa, const double* qb, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal, int64_t* feat_sum_fx,
                    int64_t* by_code, int64_t* steps_sum) {
  int rc = check_config(cfg); if (rc) return rc;
  rc = model_split_check("dql_model_split", cfg, n_tables, envs_per_table, episodes_per_env, max_steps, eps, feature, cut, pairs, reward_fx, terminal, feat_sum_fx, by_code,
                         steps_sum); if (rc) return rc;
  TableSets q;
  rc = q.from_host("dql_model_split", device, n_tables, qa, qb); if (rc) return rc;
  return model_split_run("dql_model_split", cfg, n_tables, envs_per_table, episodes_per_env, seed, max_steps, eps, feature, cut, q, pairs, reward_fx, terminal, feat_sum_fx,
                         by_code, steps_sum);
}
// the learners' tables are read where they live, as dql_ensemble_model reads them: k_model_split touches nothing else of the ensemble
int dql_ensemble_model_split(dql_ensemble* x, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed,
                             int32_t max_steps, double eps, int32_t feature, const double* cut, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal,
                             int64_t* feat_sum_fx, int64_t* by_code, int64_t* steps_sum) {
  CHECK_ENS(x);
  int rc = check_config(eval_cfg); if (rc) return rc;
  rc = model_split_check("dql_ensemble_model_split", eval_cfg, count, envs_per_learner, episodes_per_env, max_steps, eps, feature, cut, pairs, reward_fx, terminal,
                         feat_sum_fx, by_code, steps_sum); if (rc) return rc;
  TableSets q;
  rc = tables_of_slice("dql_ensemble_model_split", x, first, count, q); if (rc) return rc;
  return model_split_run("dql_ensemble_model_split", eval_cfg, count, envs_per_learner, episodes_per_env, seed, max_steps, eps, feature, cut, q, pairs, reward_fx,
                         terminal, feat_sum_fx, by_code, steps_sum);
}
int dql_diag_model_split_last(double* kernel_ms, int32_t* inst3) {
  return diag_last(g_model_split_last, kernel_ms, inst3, "no dql_model_split or dql_ensemble_model_split call has completed on this thread");
}
}  // extern "C"
