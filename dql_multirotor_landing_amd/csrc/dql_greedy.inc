// dql_greedy.inc: greedy flight of given tables in one launch: the roll-outs with flight records (dql_rollout, DESIGN.md section 11) and the scorer (dql_score,
// DESIGN.md section 13; score_check / score_run also serve dql_ensemble_score), and the host helpers every greedy-flight operator shares (DESIGN.md section 15:
// TableSets, Flight, Sums, EpisodeLog, RangeFaults, LastCall / diag_last, timed_launch, fill_flight_args / fill_greedy_args) and what its kernels share on the
// device (DESIGN.md section 28: set_coords, flush_tally, cells_clear / cells_flush).  A fragment of dql_hip.hip's translation
// unit, not a header.  Needs from it: fail / HIP_TRY, by_dtype_axes, DevBuf / OP_PROLOGUE / UP / OUT / DOWN, mdpk_bytes, upload_mdpk, upload_schedule, EvTimer,
// check_config, TickLds; and dql_rollout.hpp, dql_score.hpp.
// ---- what the family's kernels share on the device (DESIGN.md section 28) ----
// A launch of n_tables * B one-wave workgroups, B = blocks_per_table = envs_per_table / 64: table set k serves blocks [k B, (k + 1) B), so that the set's tables
// are a wave-uniform pointer; env i of every set has env id i = its RNG key (paired episodes); g: the lane's column of the outputs (every lane of the grid is an
// env: envs_per_table is a multiple of 64)
struct SetCoords { int k, i; long long g; };
__device__ __forceinline__ SetCoords set_coords(int blocks_per_table) {
  const int k = (int)blockIdx.x / blocks_per_table;
  return SetCoords{k, ((int)blockIdx.x - k * blocks_per_table) * 64 + (int)threadIdx.x, (long long)blockIdx.x * 64 + (int)threadIdx.x};
}
// what leaves a wave that flew fly_episodes: one atomicAdd per non-zero column of its tally into row `row_i` of buffers zeroed before the launch
__device__ __forceinline__ void flush_tally(const ScoreTally& t, unsigned long long* by_code, unsigned long long* steps_sum, size_t row_i) {
  if (threadIdx.x == 0) {
    unsigned long long* row = by_code + row_i * SCORE_N_COLS;
#pragma unroll
    for (int col = 0; col < SCORE_N_COLS; ++col) if (t.by_code[col]) atomicAdd(&row[col], (unsigned long long)t.by_code[col]);
    if (t.steps) atomicAdd(&steps_sum[row_i], t.steps);
  }
}
// a one-wave workgroup's LDS table of DQL_N_CELLS cells (k_score_map's histogram, k_model's rewards): the lanes sweep contiguous cells, c = it * 64 + lane,
// CELL_SWEEPS = 45 sweeps, the last one partial (cells 2 816 .. 2 834); the flush adds the non-zero cells to a row of 64-bit sums.  The caller's two
// __syncthreads() order clear, adds and flush (dql_score_map.inc)
constexpr int CELL_SWEEPS = (DQL_N_CELLS + 63) / 64;
template <typename Cell> __device__ __forceinline__ void cells_clear(Cell* cells) {
#pragma unroll 1
  for (int it = 0; it < CELL_SWEEPS; ++it) {
    const int c = it * 64 + (int)threadIdx.x;
    if (c < DQL_N_CELLS) cells[c] = Cell(0);
  }
}
template <typename Cell> __device__ __forceinline__ void cells_flush(const Cell* cells, unsigned long long* row) {
#pragma unroll 1
  for (int it = 0; it < CELL_SWEEPS; ++it) {
    const int c = it * 64 + (int)threadIdx.x;
    const Cell v = c < DQL_N_CELLS ? cells[c] : Cell(0);
    if (v) atomicAdd(&row[c], (unsigned long long)v);
  }
}

// ---- greedy roll-outs (dql_rollout, DESIGN.md section 11) ----
// One env per lane flies its FIRST episode from reset to termination (csrc/dql_rollout.hpp: rollout_episode); workgroups of one wave: evaluation batches are
// small, a lone wave per SIMD needs no LDS staging, no barrier, and there are no accumulators, table-writer blocks or statistics here.  Table set k serves
// blocks [k B, (k + 1) B), B = envs_per_table / 64, so that the set's tables are a wave-uniform pointer; env i of every set has env id i (paired episodes).
// The tick schedule of periods 0 .. max_steps sits in a device buffer read as constant memory (scalar loads by the wave-uniform period counter).
template <typename T> struct RolloutArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  RolloutInit<T> init;
  const double* qa; const double* qb;                                  // [n_tables][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule)
  RolloutOut out;
  unsigned long long seed;
  int blocks_per_table, max_steps;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_rollout(RolloutArgs<T> a) {
  const int tid = threadIdx.x;
  const int k = (int)blockIdx.x / a.blocks_per_table;                  // table set (wave-uniform)
  const int i = ((int)blockIdx.x - k * a.blocks_per_table) * 64 + tid;  // env within its table set = its RNG key
  const long long g = (long long)blockIdx.x * 64 + tid;                // output column: every lane of the grid is an env (envs_per_table is a multiple of 64)
  // the launch's constants in the layout's form, as k_step makes them for a 64-thread workgroup
  SimK<T> cl = a.c;
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
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4) {  // lane_round_keys' text, kept here: through the function this kernel's float32 code is allocated differently (DESIGN.md section 28)
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)a.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(a.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  const double* qa = a.qa + (size_t)k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)k * DQL_N_CELLS;
  const bool trace_wave = a.out.trace != nullptr && blockIdx.x == 0;   // the first trace_envs <= 64 envs of table set 0: wave 0 of the grid, nobody else
  rollout_episode<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.mgr0, a.sched, kv, a.out, g, trace_wave,
                               trace_wave && tid < a.out.trace_envs);
}

// ---- greedy scoring (dql_score / dql_ensemble_score, DESIGN.md section 13) ----
// k_rollout's shape — one env per lane, workgroups of one wave, table set k serves blocks [k B, (k + 1) B), env i of every set has RNG key (i, seed) — but a
// lane flies episode after episode (csrc/dql_score.hpp: score_episodes) and what leaves the wave is its tally: one atomicAdd per non-zero column into the
// table set's row of a buffer zeroed before the launch.  Integer sums: the result does not depend on the order the waves arrive in.
template <typename T> struct ScoreArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  RolloutInit<T> init;
  const double* qa; const double* qb;                                  // [n_tables][DQL_N_CELLS]
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* sched;   // [max_steps + 1] (fill_schedule)
  unsigned long long* by_code;                                         // [n_tables][SCORE_N_COLS]
  unsigned long long* steps_sum;                                       // [n_tables]
  ScoreLog log;
  unsigned long long seed;
  int blocks_per_table, max_steps, episodes;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_score(ScoreArgs<T> a) {
  const int tid = threadIdx.x;
  const auto [k, i, g] = set_coords(a.blocks_per_table);
  SimK<T> cl = a.c;
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
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4) {  // lane_round_keys' text, kept here: through the function this kernel's float32 code is allocated differently (DESIGN.md section 28)
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)a.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(a.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  const double* qa = a.qa + (size_t)k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)k * DQL_N_CELLS;
  const ScoreTally t = score_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes, a.mgr0, a.sched, kv, a.log, g);
  flush_tally(t, a.by_code, a.steps_sum, (size_t)k);
}

// ---- shared host helpers of the greedy family (DESIGN.md section 15): what the host side of dql_rollout, dql_score, dql_score_map, dql_model, dql_returns and
// dql_score_grid, and of their dql_ensemble_* twins, does in the same way ----
// the tables a call flies, [n_tables][DQL_N_CELLS] on the current device: uploaded from the host (from_host owns the copies), or a slice of an ensemble's own
// arrays (tables_of_slice, next to struct dql_ensemble)
struct TableSets {
  DevBuf a, b;
  const double* qa = nullptr; const double* qb = nullptr;
  int from_host(const char* who, int device, long long n_tables, const double* h_qa, const double* h_qb) {
    if (!h_qa || !h_qb) return fail(DQL_EINVAL, std::string(who) + ": null array; nothing was launched");
    OP_PROLOGUE(device)
    const size_t TB = (size_t)n_tables * DQL_N_CELLS * sizeof(double);
    UP(a, h_qa, TB); UP(b, h_qb, TB);
    qa = (const double*)a.p; qb = (const double*)b.p;
    return DQL_OK;
  }
};
// the tick schedule of periods 0 .. max_steps and the config's MdpK (score_grid: the schedule only, it uploads one MdpK per scenario into `mdp` itself)
struct Flight {
  DevBuf mgr0, sched, mdp;
  int setup(const dql_config& cfg, int max_steps, bool with_mdp = true) {
    const int n_per = max_steps + 1;
    OUT(mgr0, (size_t)n_per * sizeof(long long)); OUT(sched, (size_t)n_per * sizeof(int));
    if (with_mdp) OUT(mdp, mdpk_bytes(cfg.dtype));
    const int rc = upload_schedule(cfg, 0, n_per, mgr0.p, sched.p); if (rc) return rc;
    return with_mdp ? upload_mdpk(cfg, mdp.p) : DQL_OK;
  }
};
// one zeroed buffer of 64-bit sums, declared slice by slice; a slice is handed to the kernel and downloaded with the size it was declared with
struct Sums {
  struct Slice { size_t at, n; };
  DevBuf buf;
  size_t n_words = 0;
  Slice add(size_t n) { const Slice s{n_words, n}; n_words += n; return s; }
  int alloc_zeroed() {
    OUT(buf, n_words * sizeof(unsigned long long));
    HIP_TRY(hipMemset(buf.p, 0, n_words * sizeof(unsigned long long)));
    return DQL_OK;
  }
  unsigned long long* dev(Slice s) const { return (unsigned long long*)buf.p + s.at; }
  struct To { int64_t* host; Slice s; };
  int down(std::initializer_list<To> parts) const {  // a null host array (an optional output) is skipped
    for (const To& t : parts) if (t.host) HIP_TRY(hipMemcpy(t.host, dev(t.s), t.s.n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return DQL_OK;
  }
};
// the optional episode log, `entries` each of ep_code (0xff: not finished) and ep_steps (0); without one the device pointers are null
struct EpisodeLog {
  DevBuf code, steps;
  size_t entries = 0;
  bool on = false;
  int setup(bool wanted, size_t n) {
    on = wanted; entries = n;
    if (!on) return DQL_OK;
    OUT(code, entries); OUT(steps, entries * sizeof(uint16_t));
    HIP_TRY(hipMemset(code.p, 0xff, entries));  // not finished
    HIP_TRY(hipMemset(steps.p, 0, entries * sizeof(uint16_t)));
    return DQL_OK;
  }
  int down(uint8_t* ep_code, uint16_t* ep_steps) const {
    if (!on) return DQL_OK;
    DOWN(ep_code, code, entries);
    DOWN(ep_steps, steps, entries * sizeof(uint16_t));
    return DQL_OK;
  }
};
// the word a kernel counts in what its range checks dropped (0 unless a bug): read back after the launch, non-zero refuses the result
struct RangeFaults {
  const unsigned long long* d = nullptr; const char* who = ""; const char* whose = "kernel's"; const char* what = "contributions";
  int refuse_if_any() const {
    if (!d) return DQL_OK;
    unsigned long long faults = 0ull;
    HIP_TRY(hipMemcpy(&faults, d, sizeof(faults), hipMemcpyDeviceToHost));
    if (faults) return fail(DQL_ESTATE, std::string(who) + ": the " + whose + " range checks dropped " + std::to_string(faults) + " " + what + " (a bug); no result was returned");
    return DQL_OK;
  }
};
// kernel time(s) and instance (sizeof(T), TICK, XMODE) of a thread's latest completed call of one operator: a *_run fills a local one and stores it on DQL_OK only
struct LastCall {
  double ms = -1.0, ms2 = 0.0;  // ms2: the second stretch of the returns
  int inst[3] = {0, 0, 0};
  template <typename T> void instance(int tick, int xmode) { inst[0] = (int)sizeof(T); inst[1] = tick; inst[2] = xmode; }
};
static int diag_last(const LastCall& c, double* ms, double* ms2, int32_t* out3, const char* none_yet) {
  if (!ms || !ms2 || !out3) return fail(DQL_EINVAL, "null pointer");
  if (c.ms < 0.0) return fail(DQL_ESTATE, none_yet);
  *ms = c.ms; *ms2 = c.ms2;
  for (int k = 0; k < 3; ++k) out3[k] = c.inst[k];
  return DQL_OK;
}
static int diag_last(const LastCall& c, double* kernel_ms, int32_t* out3, const char* none_yet) { double unused = 0.0; return diag_last(c, kernel_ms, &unused, out3, none_yet); }
// the launch bracket: timer start, launch() (the typed hipLaunchKernelGGL and nothing else), hipGetLastError, timer stop, then the range-check word if there is one
template <typename L> static int timed_launch(L&& launch, double* ms, const RangeFaults& faults = RangeFaults{}) {
  EvTimer timer;
  int rc = timer.start(); if (rc) return rc;
  launch();
  HIP_TRY(hipGetLastError());
  rc = timer.stop_ms(ms); if (rc) return rc;
  return faults.refuse_if_any();
}
// the kernel arguments every greedy-flight kernel has, and (fill_greedy_args) the ones made from the call's one config
template <typename A> static void fill_flight_args(A& a, const TableSets& q, const Flight& fl, unsigned long long seed, long long envs_per_table, int max_steps) {
  a.qa = q.qa; a.qb = q.qb;
  a.mgr0 = (const long long DQL_CONST_AS*)fl.mgr0.p; a.sched = (const int DQL_CONST_AS*)fl.sched.p;
  a.seed = seed; a.blocks_per_table = (int)(envs_per_table / 64); a.max_steps = max_steps;
}
template <typename T, typename A> static void fill_greedy_args(A& a, const dql_config& cfg, const TableSets& q, const Flight& fl, unsigned long long seed, long long envs_per_table,
                                                               int max_steps) {
  a.c = make_simk<T>(cfg);
  a.mdp = (const MdpK<T> DQL_CONST_AS*)fl.mdp.p;
  a.mdp_run = MdpRun<T>{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  a.init = make_rollout_init<T>(cfg);
  fill_flight_args(a, q, fl, seed, envs_per_table, max_steps);
}

extern "C" {
// ---- greedy roll-outs ----
static thread_local LastCall g_rollout_last;
int dql_rollout_n_fields(int32_t* n_record, int32_t* n_trace) { if (n_record) *n_record = RO_N_RECORD; if (n_trace) *n_trace = RO_N_TRACE; return DQL_OK; }
const char* dql_rollout_field_name(int32_t i, int32_t is_trace) { return (i >= 0 && i < (is_trace ? RO_N_TRACE : RO_N_RECORD)) ? k_rollout_field_names[i] : nullptr; }
int dql_rollout(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, uint64_t seed, int32_t max_steps, const double* qa, const double* qb,
                int32_t* code, int32_t* steps, double* rec, int32_t trace_envs, double* trace_or_null) {
  int rc = check_config(cfg); if (rc) return rc;
  // every argument is checked before the device is touched: a refused call starts no kernel
  if (n_tables < 1 || n_tables > DQL_ROLLOUT_MAX_TABLES) return fail(DQL_EINVAL, "dql_rollout: n_tables must be in 1..16 (DQL_ROLLOUT_MAX_TABLES); nothing was launched");
  if (envs_per_table < 64 || envs_per_table % 64 != 0) return fail(DQL_EINVAL, "dql_rollout: envs_per_table must be a positive multiple of 64 (one wave per workgroup, whole waves per table set); nothing was launched");
  if ((long long)n_tables * envs_per_table > (1ll << 30)) return fail(DQL_EINVAL, "dql_rollout: n_tables * envs_per_table must be at most 2^30; nothing was launched");
  if (max_steps < 1 || max_steps > DQL_ROLLOUT_MAX_STEPS) return fail(DQL_EINVAL, "dql_rollout: max_steps must be in 1..4096 (DQL_ROLLOUT_MAX_STEPS); nothing was launched");
  if (trace_envs < 0 || trace_envs > 64) return fail(DQL_EINVAL, "dql_rollout: trace_envs must be in 0..64 (the trace stays inside one wave); nothing was launched");
  if (trace_envs > 0 && !trace_or_null) return fail(DQL_EINVAL, "dql_rollout: trace_envs > 0 needs a trace buffer; nothing was launched");
  if (!code || !steps || !rec) return fail(DQL_EINVAL, "dql_rollout: null array; nothing was launched");
  TableSets q;
  rc = q.from_host("dql_rollout", device, n_tables, qa, qb); if (rc) return rc;
  const long long n_total = (long long)n_tables * envs_per_table;
  Flight fl;
  rc = fl.setup(*cfg, max_steps); if (rc) return rc;
  DevBuf d_code, d_steps, d_rec, d_trace;
  OUT(d_code, (size_t)n_total * sizeof(int)); OUT(d_steps, (size_t)n_total * sizeof(int)); OUT(d_rec, (size_t)RO_N_RECORD * n_total * sizeof(double));
  const size_t trace_bytes = (size_t)(max_steps + 1) * RO_N_TRACE * (size_t)trace_envs * sizeof(double);
  if (trace_envs > 0) {
    OUT(d_trace, trace_bytes);
    HIP_TRY(hipMemset(d_trace.p, 0xff, trace_bytes));  // all ones = NaN: what a row keeps after its env's last period
  }
  const RolloutOut out{(int*)d_code.p, (int*)d_steps.p, (double*)d_rec.p, trace_envs > 0 ? (double*)d_trace.p : nullptr, n_total, trace_envs};
  LastCall call;
  rc = timed_launch([&] {
    by_dtype_axes(cfg->dtype, cfg->two_axis, [&](auto t, auto xmode) {
      using T = decltype(t);
      constexpr int XMODE = decltype(xmode)::value;
      RolloutArgs<T> a;
      fill_greedy_args<T>(a, *cfg, q, fl, seed, envs_per_table, max_steps);
      a.out = out;
      call.instance<T>(TICK_PLAIN, XMODE);
      hipLaunchKernelGGL((k_rollout<T, TICK_PLAIN, XMODE>), dim3((unsigned)((long long)n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
    });
  }, &call.ms);
  if (rc) return rc;
  DOWN(code, d_code, (size_t)n_total * sizeof(int));
  DOWN(steps, d_steps, (size_t)n_total * sizeof(int));
  DOWN(rec, d_rec, (size_t)RO_N_RECORD * n_total * sizeof(double));
  if (trace_envs > 0) DOWN(trace_or_null, d_trace, trace_bytes);
  g_rollout_last = call;
  return DQL_OK;
}
int dql_diag_rollout_last(double* kernel_ms, int32_t* out3) { return diag_last(g_rollout_last, kernel_ms, out3, "no dql_rollout call has completed on this thread"); }

// ---- greedy scoring ----
static thread_local LastCall g_score_last;
// every argument both entry points share, checked before the device is touched: a refused call starts no kernel
static int score_check(const char* who, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, int32_t max_steps, const int64_t* by_code, const int64_t* steps_sum,
                       const uint8_t* ep_code, const uint16_t* ep_steps) {
  const std::string w(who);
  if (n_tables < 1 || n_tables > DQL_SCORE_MAX_TABLES) return fail(DQL_EINVAL, w + ": the number of table sets must be in 1..2^20 (DQL_SCORE_MAX_TABLES); nothing was launched");
  if (envs_per_table < 64 || envs_per_table % 64 != 0) return fail(DQL_EINVAL, w + ": the envs per table set must be a positive multiple of 64 (one wave per workgroup, whole waves per table set); nothing was launched");
  if (envs_per_table > (1ll << 30) || n_tables * envs_per_table > (1ll << 30)) return fail(DQL_EINVAL, w + ": table sets x envs must be at most 2^30; nothing was launched");
  if (episodes_per_env < 1 || episodes_per_env > DQL_SCORE_MAX_EPISODES) return fail(DQL_EINVAL, w + ": episodes_per_env must be in 1..64 (DQL_SCORE_MAX_EPISODES); nothing was launched");
  if (max_steps < 1 || max_steps > DQL_SCORE_MAX_STEPS) return fail(DQL_EINVAL, w + ": max_steps must be in 1..4096 (DQL_SCORE_MAX_STEPS); nothing was launched");
  if ((ep_code == nullptr) != (ep_steps == nullptr)) return fail(DQL_EINVAL, w + ": the episode log needs both arrays or neither; nothing was launched");
  if (!by_code || !steps_sum) return fail(DQL_EINVAL, w + ": null array; nothing was launched");
  return DQL_OK;
}
static int score_run(const dql_config* cfg, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, const TableSets& q, int64_t* by_code,
                     int64_t* steps_sum, uint8_t* ep_code, uint16_t* ep_steps) {
  const long long n_total = n_tables * envs_per_table;
  Flight fl;
  int rc = fl.setup(*cfg, max_steps); if (rc) return rc;
  Sums sums;
  const Sums::Slice s_by_code = sums.add((size_t)n_tables * SCORE_N_COLS), s_steps = sums.add((size_t)n_tables);
  rc = sums.alloc_zeroed(); if (rc) return rc;
  EpisodeLog elog;
  rc = elog.setup(ep_code != nullptr, (size_t)episodes * (size_t)n_total); if (rc) return rc;
  const ScoreLog log{(uint8_t*)elog.code.p, (uint16_t*)elog.steps.p, n_total};
  LastCall call;
  rc = timed_launch([&] {
    by_dtype_axes(cfg->dtype, cfg->two_axis, [&](auto t, auto xmode) {
      using T = decltype(t);
      constexpr int XMODE = decltype(xmode)::value;
      ScoreArgs<T> a;
      fill_greedy_args<T>(a, *cfg, q, fl, seed, envs_per_table, max_steps);
      a.by_code = sums.dev(s_by_code); a.steps_sum = sums.dev(s_steps); a.log = log; a.episodes = episodes;
      call.instance<T>(TICK_PLAIN, XMODE);
      hipLaunchKernelGGL((k_score<T, TICK_PLAIN, XMODE>), dim3((unsigned)(n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
    });
  }, &call.ms);
  if (rc) return rc;
  rc = sums.down({{by_code, s_by_code}, {steps_sum, s_steps}}); if (rc) return rc;
  rc = elog.down(ep_code, ep_steps); if (rc) return rc;
  g_score_last = call;
  return DQL_OK;
}
int dql_score(const dql_config* cfg, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps,
              const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null) {
  int rc = check_config(cfg); if (rc) return rc;
  rc = score_check("dql_score", n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, ep_code_or_null, ep_steps_or_null); if (rc) return rc;
  TableSets q;
  rc = q.from_host("dql_score", device, n_tables, qa, qb); if (rc) return rc;
  return score_run(cfg, n_tables, envs_per_table, episodes_per_env, seed, max_steps, q, by_code, steps_sum, ep_code_or_null, ep_steps_or_null);
}
int dql_diag_score_last(double* kernel_ms, int32_t* inst3) { return diag_last(g_score_last, kernel_ms, inst3, "no dql_score or dql_ensemble_score call has completed on this thread"); }
}  // extern "C"
