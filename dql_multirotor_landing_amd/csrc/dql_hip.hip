// dql_hip.hip — kernels + C ABI (include/dql.h) of the MI355X UAV-landing / tabular Double-Q hot path.
//
// Kernels (all wave64, gfx950):
//   k_step<T,BLOCK,TICK>     fused agent period: eps-greedy guess, 21/22 physics ticks (PID, SO(3) attitude law, rotor
//                            model, rigid body, platform, 100 Hz observation pipeline), discretise/check/reward, TD target.
//                            One lane per env, state in VGPRs, 16-byte coalesced quad loads/stores, per-workgroup LDS
//                            accumulators (int64 fixed-point target sums + visit counts), wave64 shuffle reductions of the
//                            counters, one global atomic per touched cell per workgroup.
//                            Extra "table-writer" workgroups of the same launch fold the PREVIOUS launch's accumulators into
//                            the master tables (mean-target contraction) and publish the acting tables of the NEXT launch, so
//                            the table update has no kernel and no time of its own (tables act with one period of delay).
//   k_flush                  same fold outside a launch (host table access, level switch, rank sync).
//   k_apply_window           multi-GPU: folds the all-reduced window accumulators into the base tables.
//   small stateless kernels  drop-in single-call operators (discretise, mdp transition, predict, ordered update).
#include <hip/hip_runtime.h>
#include <limits>
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is dlopen'ed on first use (dql_comm_*)

#include <dlfcn.h>
#include <unistd.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_advance.hpp"
#include "dql_score.hpp"
#include "../../include/dql_diag.h"

using namespace dql;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                                        \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess) return fail(DQL_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)
#define CHECK_CTX(ctx) do { if (!(ctx)) return fail(DQL_EINVAL, "null context"); } while (0)

struct StatsDev { unsigned long long decisions, episodes, by_code[DQL_N_CHECK_CODES]; long long reward_fx; unsigned long long agent_steps, bad_actions; };

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
template <typename T> struct InitArgs {
  SimK<T> c; Quad<T>* sr; int4* si; long long n; unsigned long long seed; long long env_id_offset;
  T hover, vz_integ, r_lo, r_hi, t_lo, t_hi;
};
template <typename T> __global__ void k_init(InitArgs<T> a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const SimK<T>& s = a.c;
  uint32_t r[4];
  philox4x32(0u, 0u, (uint32_t)(a.env_id_offset + i), STREAM_INIT, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
  Env<T> e;
  memset(&e, 0, sizeof(e));
  e.q[0] = T(1.0); e.p[2] = s.z_init;
  for (int k = 0; k < 4; ++k) e.om[k] = a.hover;
  e.vz_i = a.vz_integ;
  e.kal_x_P = T(1.0); e.kal_y_P = T(1.0);
  e.mp_r = s.mp_r; e.mp_w = s.mp_w;
  if (s.per_env_platform && s.traj == DQL_TRAJ_RPM) {
    e.mp_r = fma_(u24<T>(r[1]), a.r_hi - a.r_lo, a.r_lo);
    const T tx = fma_(u24<T>(r[2]), a.t_hi - a.t_lo, a.t_lo);
    e.mp_w = tx / e.mp_r;
  }
  e.mp_phase = T(6.28318530717958623200e+00) * u24<T>(r[0]);
  platform_eval(s, e);
  e.code = DQL_NON_TERMINAL; e.idx_x = -1; e.idx_y = -1; e.flags = FL_DONE; e.action = 2;
  const long long n = a.n;
  // every quad is written once here (also those the step kernel never touches in x-axis configs)
  a.sr[11 * n + i] = Quad<T>{e.mp_v, e.vf_y, e.kal_y_x, e.kal_y_P};
  a.sr[12 * n + i] = Quad<T>{T(0.0), T(0.0), T(0.0), T(0.0)};
  a.sr[13 * n + i] = Quad<T>{e.mp_r, e.mp_w, T(0.0), T(0.0)};
  store_env(e, a.sr, a.si, n, i, s);
}

// mean-target contraction of one cell: Q <- tbar + (Q - tbar) * prod_{j<m} (1 - alpha(count + j))
struct FoldK { const double* alpha_tab; int n_tab; double alpha_min; int per_step; long long n_launch; };
DQL_DEV double fold_q(const FoldK& f, double q, double cnt, long long Tsum, long long m) {
  const double tbar = ((double)Tsum * (1.0 / (double)(1ll << DQL_TARGET_FRAC_BITS))) / (double)m;
  const long long c0 = (long long)cnt;
  double shrink = 1.0;
  long long j = 0;
  // per_step: one learning-rate step per launch the accumulators cover (1 for a launch's own fold, the window length for
  // the multi-GPU window), never more steps than visits
  const long long m_eff = f.per_step ? (m < f.n_launch ? m : f.n_launch) : m;
  // the learning rates of visits c0, c0+1, ... up to the table's plateau: loads in batches of 8 (independent, one memory round trip per
  // batch), products in visit order — the same sequence of multiplications as a plain loop, 8x fewer round trips (a fresh table
  // folds hundreds of visits per cell: 160 us per fold kernel before, profiles/r2_exchange_kernels.csv)
  const long long jn = (m_eff < f.n_tab - c0) ? m_eff : (f.n_tab - c0 > 0 ? f.n_tab - c0 : 0);
  for (; j + 8 <= jn; j += 8) {
    double a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = f.alpha_tab[c0 + j + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) shrink *= (1.0 - a[k]);
  }
  for (; j < jn; ++j) shrink *= (1.0 - f.alpha_tab[c0 + j]);
  long long rem = m_eff - j;
  if (rem > 0) {
    double base = 1.0 - f.alpha_min, pw = 1.0;
    while (rem) { if (rem & 1) pw *= base; base *= base; rem >>= 1; }
    shrink *= pw;
  }
  return tbar + (q - tbar) * shrink;
}
// Accumulators are [4][N_CELLS]: Q_table_a's {target sums, visits}, then Q_table_b's (the second pair stays empty under the
// reference's table-a-only quirk); the visit counter is shared, so table a's fold goes first and table b's visits take the
// learning rates after it (same order in the oracle).
#define DQL_ACC_LEN (4 * DQL_N_CELLS)
#define DQL_ACC_B (2 * DQL_N_CELLS)
// fold one cell of ONE table's accumulator pair into that master table (and the multi-GPU window), clear the accumulator
DQL_DEV double fold_cell(const FoldK& f, double* qa_m, double* cnt_m, long long* acc, long long* window, int windowed, int c) {
  const long long Tsum = acc[c], m = acc[DQL_N_CELLS + c];
  double q = qa_m[c];
  if (m > 0) {
    const double cnt = cnt_m[c];
    if (windowed) { window[c] += Tsum; window[DQL_N_CELLS + c] += m; }
    q = fold_q(f, q, cnt, Tsum, m);
    qa_m[c] = q; cnt_m[c] = cnt + (double)m;
    acc[c] = 0; acc[DQL_N_CELLS + c] = 0;
  }
  return q;
}

#define DQL_ZERO_COPY_ENVS 16384  // up to here dql_step's kernel reads the host actions from pinned memory itself (no copy command)
template <typename T> struct StepArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;  // device buffer, read as constant memory (scalar loads)
  MdpRun<T> mdp_run;                // what the literal-constant layout still needs at run time (dql_device.hpp LitM)
  Quad<T>* sr; int4* si;
  const double* qa; const double* qb;  // ACTING tables of this launch: every accumulator up to launch j-2 folded in
  unsigned long long* acc_cur;         // [2][DQL_N_CELLS] of this launch: target sums (fixed point), visits
  // table-writer blocks (blockIdx >= env_blocks): fold launch j-1's accumulators into the master tables while the env blocks
  // run, publish the result as the acting tables of launch j+1 -> the table update costs no kernel and no time of its own
  double* qa_m; double* qb_m; double* cnt_m; double* qa_pub; double* qb_pub; long long* acc_prev; long long* window;
  FoldK fold;
  StatsDev* stats;
  const uint8_t* actions;
  unsigned long long* elog;            // episode log rows of this launch or null: per period [n_waves] done masks, [n_waves] success masks
  long long n, env_id_offset, step_index;  // step_index: the first agent period of this launch
  // per period of the launch, from the host (round 5: the kernel used to derive them from the tick count g0 with a 64-bit division and a modulo per
  // wave and period): index of the period's first manager tick, and in sched[p] its physics ticks | ticks since the last manager tick << 8 |
  // index of the period's LAST manager tick (the one whose noise is read) << 16
  long long mgr0[DQL_MAX_PERIODS];
  unsigned long long seed;
  unsigned int eps_thr, pad_;  // explore <=> (r >> 8) < eps_thr: ceil(eps 2^24), the integer form of u24(r) < eps (host: eps_threshold)
  int sched[DQL_MAX_PERIODS];
  int mode, n_periods, env_blocks, have_prev, windowed;
  int fair_prio;  // more env waves than SIMDs: the waves of a SIMD take turns at the issue priority (k_step)
};

// wave64 sum on the DPP path (no LDS permutes, no waits): row_shr 1, 2, 4, 8 build the prefix sums of each row of 16 lanes,
// row_bcast15 / row_bcast31 carry the row totals across (CDNA keeps the GFX9 broadcasts); lane 63 holds the total
template <int CTRL, int ROW_MASK> DQL_DEV long long dpp_add64(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROW_MASK, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)v >> 32), CTRL, ROW_MASK, 0xf, false);
  return v + (long long)(((unsigned long long)hi << 32) | lo);
}
DQL_DEV long long wave_sum(long long v) {
  v = dpp_add64<0x111, 0xf>(v); v = dpp_add64<0x112, 0xf>(v); v = dpp_add64<0x114, 0xf>(v); v = dpp_add64<0x118, 0xf>(v);
  v = dpp_add64<0x142, 0xa>(v); v = dpp_add64<0x143, 0xc>(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), 63);
  return (long long)(((unsigned long long)hi << 32) | lo);  // wave-uniform
}

// The step kernel's arguments (constants by value: ~0.5 KB = 8 cache lines) are fetched by the compiler piecemeal, one scalar
// load + wait per line as registers allow: a chain of scalar-cache misses at the head of every wave.  Touch all lines at once
// first; the later loads then hit the scalar cache.
template <int BYTES> DQL_DEV void warm_kernarg() {
  const auto* p = __builtin_amdgcn_kernarg_segment_ptr();
  constexpr int L = (BYTES + 63) / 64;  // 64-byte lines the arguments reach (9 .. 17); offsets beyond the last line fold back onto it (a 17th line — float64 — is left to its first use)
  static_assert(L > 8 && L <= 24, "adjust the touch list to the argument size");  // (sixteen lines are touched: what lies beyond — the tail of the per-period schedule arrays — is left to its first use)
#define DQL_LINE(i) ((i) < L ? (i) * 64 : (L - 1) * 64)
  unsigned t0, t1, t2, t3, t4, t5, t6, t7, u0, u1, u2, u3, u4, u5, u6, u7;
  // sixteen loads in flight, one wait.  The first statement's destinations are inputs of the second, so the compiler keeps them allocated
  // until the wait (a register handed to another value while a load into it is still in flight would be overwritten when it lands)
  asm volatile("s_load_dword %0, %8, %9\n\ts_load_dword %1, %8, %10\n\ts_load_dword %2, %8, %11\n\ts_load_dword %3, %8, %12\n\t"
               "s_load_dword %4, %8, %13\n\ts_load_dword %5, %8, %14\n\ts_load_dword %6, %8, %15\n\ts_load_dword %7, %8, %16"
               : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3), "=&s"(t4), "=&s"(t5), "=&s"(t6), "=&s"(t7)
               : "s"(p), "n"(DQL_LINE(0)), "n"(DQL_LINE(1)), "n"(DQL_LINE(2)), "n"(DQL_LINE(3)), "n"(DQL_LINE(4)), "n"(DQL_LINE(5)), "n"(DQL_LINE(6)), "n"(DQL_LINE(7)));
  asm volatile("s_load_dword %0, %8, %9\n\ts_load_dword %1, %8, %10\n\ts_load_dword %2, %8, %11\n\ts_load_dword %3, %8, %12\n\t"
               "s_load_dword %4, %8, %13\n\ts_load_dword %5, %8, %14\n\ts_load_dword %6, %8, %15\n\ts_load_dword %7, %8, %16\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&s"(u0), "=&s"(u1), "=&s"(u2), "=&s"(u3), "=&s"(u4), "=&s"(u5), "=&s"(u6), "=&s"(u7)
               : "s"(p), "n"(DQL_LINE(8)), "n"(DQL_LINE(9)), "n"(DQL_LINE(10)), "n"(DQL_LINE(11)), "n"(DQL_LINE(12)), "n"(DQL_LINE(13)), "n"(DQL_LINE(14)), "n"(DQL_LINE(15)),
                 "s"(t0), "s"(t1), "s"(t2), "s"(t3), "s"(t4), "s"(t5), "s"(t6), "s"(t7));
#undef DQL_LINE
}
// Population launch (dql_pop_*): K agents' envs in one launch, agent-major (agent k owns envs [k E, (k+1) E), E a multiple of
// 512, so that a workgroup of any size holds one agent).  What differs between agents comes from a descriptor per active agent the host builds for
// the launch (launch_pop) from THAT agent's history; the kernel reads it with scalar loads (constant address space).
struct PopAgentDesc {
  const double* qa; const double* qb; unsigned long long* acc_cur;  // the agent's acting tables and accumulators of this launch (its own launch parity)
  double* qa_m; double* qb_m; double* cnt_m; double* qa_pub; double* qb_pub; long long* acc_prev; long long* window;
  StatsDev* stats;
  const char DQL_CONST_AS* mdp;     // the agent's MdpK<T> (level dependent)
  unsigned long long* elog;          // the episode-log row of the agent's next period (rows span all K E envs) or null
  unsigned long long* faults;        // targets the bounds guard dropped (dql_pop_index_faults)
  FoldK fold;                        // n_launch: the agent's pending periods
  long long step_index;
  unsigned long long seed;
  long long mgr0[DQL_MAX_PERIODS];
  int sched[DQL_MAX_PERIODS];
  unsigned int eps_thr; int have_prev, working, pad_;
};
template <typename T> struct PopArgs {
  StepArgs<T> s;  // what the agents share: c (its level replaced per agent), mdp_run, sr, si, n = K E, mode, n_periods, env_blocks = K E / BLOCK, fair_prio
  const PopAgentDesc DQL_CONST_AS* desc;  // [n_active], in slot order
  int blocks_per_agent, writer_blocks, n_active, pad_;
  int agent[DQL_MAX_AGENTS];  // slot -> agent: the compact list of the launch's active agents
};

// TICK: layout of the 500 Hz loop (dql_device.hpp, agent_period: TICK_PLAIN / TICK_PACKED / TICK_LIT / TICK_PACKED_LITM; launch_step_b
// chooses).  Resident waves per SIMD by workgroup size:
// 64 .. 256 threads: at most 2 waves per SIMD (68 KB of LDS accumulators per workgroup, or the register-hungry layouts); 512 threads:
// two workgroups per CU = 4 waves per SIMD, so the compiler must stay within 128 VGPRs (it parks ~35 cold values in scratch)
constexpr int step_waves_per_simd(int block) { return block == 512 ? 4 : 2; }
// the register budget the compiler is HELD to (the minimum occupancy it must allow): 512-thread workgroups need their 4 waves per SIMD to fit a CU at all;
// the float64 256-thread instance — the one big float64 batches run on — is held to 2 (256 VGPRs: 73 values go to scratch, none of them in the tick loop's
// float64 chain): the float64 pipe issues every 8 cycles, one wave alone leaves it idle a quarter of the time (131 072 envs: 66.0 -> 57.7 us per period,
// profiles/r5_f64_two_waves.jsonl; batches of one wave per SIMD pay 1 % for the spills).  Everything else may take up to 512 registers when it runs alone.
constexpr int step_min_waves_per_simd(int block, int real_size) { return block >= 512 ? step_waves_per_simd(block) : (real_size == 8 && block == 256 ? 2 : 1); }
template <typename T> DQL_DEV SimK<T> x_only(SimK<T> c) { c.two_axis = 0; return c; }
template <typename T> struct TickLds { char unused; };
template <> struct TickLds<double> { SimK<double> k; };
template <typename T, int BLOCK, int TICK, int XMODE> __global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(step_min_waves_per_simd(BLOCK, (int)sizeof(T)), step_waves_per_simd(BLOCK)))) void k_step(StepArgs<T> a) {
  // several waves per workgroup: TD targets meet in LDS first (4x fewer global atomics on the hot cells of a big batch);
  // one wave per workgroup (small batches, latency-bound): 64 envs rarely share a cell, so each lane adds straight into the
  // global accumulators and the wave needs no LDS clear, no barrier and no flush scan (measured: -1.5 us of 26 at 4096 envs)
  constexpr bool STAGED = BLOCK > 64;
  __shared__ unsigned long long sT[STAGED ? 2 * DQL_N_CELLS : 1];  // staged index = table * N_CELLS + cell (StepOut::cell)
  __shared__ unsigned int sM[STAGED ? 2 * DQL_N_CELLS : 1];
  __shared__ unsigned long long sStat[4 + 7];  // decisions, episodes, reward sum, (spare), then the terminal histogram (codes 0 .. TERMINAL_TIMEOUT)
  DQL_PHASE_BEGIN(clk_start);
  warm_kernarg<(int)sizeof(StepArgs<T>)>();
  const int tid = threadIdx.x;
  DQL_WAVE_BEGIN(clk0);
  if ((int)blockIdx.x >= a.env_blocks) {  // table-writer block (whole block takes this path: no barrier is skipped)
    const int c = ((int)blockIdx.x - a.env_blocks) * BLOCK + tid;
    if (c < DQL_N_CELLS) {
      double qa = a.qa_m[c], qb = a.qb_m[c];
      if (a.have_prev) {
        qa = fold_cell(a.fold, a.qa_m, a.cnt_m, a.acc_prev, a.window, a.windowed, c);
        qb = fold_cell(a.fold, a.qb_m, a.cnt_m, a.acc_prev + DQL_ACC_B, a.window + DQL_ACC_B, a.windowed, c);
      }
      a.qa_pub[c] = qa; a.qb_pub[c] = qb;
    }
    return;
  }
  const int ncell = (a.c.working + 1) * DQL_CELLS_PER_LEVEL;
  const int n_tab = (a.c.quirks & DQL_Q_UPDATE_TABLE_A_ONLY) ? 1 : 2;  // tables that can receive targets (wave-uniform)
  const long long i = (long long)blockIdx.x * BLOCK + tid;
  long long dec = 0, don = 0, rfx = 0;
  bool goal = false;
  // P agent periods per launch (option "periods_per_launch", default 1): the env stays in registers between them, so the state
  // round trip through HBM, the launch boundary and the table-writer work are paid once per P periods; the acting tables are
  // those of the launch for all P periods, every period's TD targets go to the launch's accumulators
  Env<T> e;
  QRow qx = QRow{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // The launch's head in the order of its latencies: the state's loads are ISSUED first, and what does not depend on them — the constants' moves to
  // VGPRs, the LDS clear and its barrier — runs while they travel (the clear and the barrier used to come first, with nothing in flight behind them)
  if (i < a.n) {
    // the packed ints go first: their state index addresses the acting-table row, whose request then rides along with the
    // state quads instead of waiting for them (one memory round trip less at the head of the wave).  A fresh or reset env has
    // no previous state (idx -1): its row is never used, but the address must stay inside the table
    const int4 iv = a.si[i];
    qx = load_qrow(a.qa, a.qb, (unsigned)iv.x < (unsigned)(DQL_N_CELLS / DQL_N_ACTIONS) ? iv.x : 0);
    load_env(e, a.sr, iv, a.n, i, XMODE == X_ONLY ? x_only(a.c) : a.c);
  }
  // XMODE (dql_device.hpp agent_period): in an x-axis kernel the config's two_axis is the constant 0 — every y-axis branch of the step folds away
  SimK<T> cfgk = a.c;
  if constexpr (XMODE == X_ONLY) cfgk.two_axis = 0;
  // register headroom (<= 2 waves per SIMD: 256 VGPRs): the manager tick's and the period's run-time constants move to VGPRs once per launch
  if constexpr (sizeof(T) == 4 && BLOCK < 512) cfgk = period_consts_in_vgprs(cfgk);
  // the Philox round keys (a launch constant) in VGPRs, where there are registers to spare (philox4x32)
  uint32_t kv_[20];
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4 && BLOCK < 512 && (TICK == TICK_LIT || TICK == TICK_PLAIN)) {  // (the VGPR-constant layouts have their registers spoken for: 112 SGPR spills with the keys against 47)
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)a.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(a.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  if (STAGED) {
    for (int t = 0; t < n_tab; ++t)
      for (int c = tid; c < ncell; c += BLOCK) { sT[t * DQL_N_CELLS + c] = 0ull; sM[t * DQL_N_CELLS + c] = 0u; }
    if (tid < 4 + 7) sStat[tid] = 0ull;
    __syncthreads();
  }
  DQL_WAVE_END_VAR(clk1);
  if (i < a.n) {
    DQL_MARK_T(e, 2);
    DQL_PHASE_LOADED(e, clk_start);
  }
  long long dec_w = 0, don_w = 0, rfx_w = 0;  // per-wave totals over the periods of this launch (wave-uniform after the reductions)
  // the reward total is an integer (fixed point): every lane keeps its own sum over the launch's periods (< 32 x 2^50) and the wave adds them up ONCE, behind the
  // period loop — the 64-bit DPP reduction used to run in every period (45 instructions of each env wave's period)
  long long rfx_lane = 0;
  // terminal histogram of the wave over the launch: one ballot per CheckResult code and period instead of one global atomic per finished
  // episode (thousands per period on a handful of addresses at large batches)
  unsigned code_w[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  // float64: the tick's constants are read from LDS.  As kernel arguments they are SGPR PAIRS — some 150 of them against 100 scalar registers — and the
  // compiler parked the overflow in VGPR lanes: ~850 v_readlane_b32 per physics tick, three quarters of the tick's instructions, around 264 float64 operations.
  // One copy per workgroup, read back where used (agent_period's plain loop keeps the compiler from hoisting the reads out of the tick loop again).
  __shared__ TickLds<T> sTickK;  // (float32: an unused byte)
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  // ROUND 5: the two waves of a SIMD take turns at the issue priority.  The arbiter serves priority first, then AGE: of two waves running the same
  // program the older one is nearly unimpeded and the younger gets the leftover slots — at exactly two waves per SIMD the older half of the env
  // waves finished a 16-period launch after 272 us and the younger half then ran ALONE, at a lone wave's issue rate, for another 55 us
  // (profiles/r5_wave_tail.jsonl).  Alternating s_setprio by (period + hardware wave slot) parity gives each wave the head of the queue in every
  // other period: both finish together and the SIMD never runs half empty.  (A wave that shares its SIMD with nobody is unaffected.)
  // compiled into the layouts that serve several waves per SIMD only (the packed / VGPR-constant layouts fly batches of at most one env wave per SIMD:
  // nobody to take turns with, and the extra code cost them 0.8 %), and switched on by the host when the batch has more env waves than the device SIMDs
  constexpr bool FAIR = (TICK == TICK_PLAIN || TICK == TICK_LIT) && BLOCK >= 128;
  unsigned prio_role = 0u;
  bool fair_prio = false;
  if constexpr (FAIR) {
    fair_prio = a.fair_prio != 0;
    if (fair_prio) {
      unsigned hw_id;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
      prio_role = hw_id & 1u;  // wave slot parity: the two waves of a SIMD sit in slots 0 and 1
    }
  }
  for (int p = 0; p < a.n_periods; ++p) {
    // (giving the older wave the even periods instead, or the launch's last period to the younger one: 19.46 / 19.38 against 19.18 us per period)
    // (other patterns — the younger wave ahead in 12 of 16 periods, in all, in none — change nothing or bring the tail back: 19.19 / 20.25 / 20.29 us)
    if (fair_prio) { if ((((unsigned)p) ^ prio_role) & 1u) asm volatile("s_setprio 1"); else asm volatile("s_setprio 0"); }
    dec = 0; don = 0; rfx = 0; goal = false;
    int done_code = -1;
    if (i < a.n) {
      const int ext = (a.mode == MODE_EXTERNAL) ? (int)a.actions[i] : 2;
      if (a.mode == MODE_EXTERNAL) {  // the caller's actions are checked here, not by a host loop (dql_step): ax | ay << 2, both in 0..2
        const int ax = ext & 3, ay = (ext >> 2) & 3;
        if (ax > 2 || ay > 2 || (ext >> 4) || (!a.c.two_axis && ay != 0 && ay != 2)) atomicAdd(&a.stats->bad_actions, 1ull);
      }
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, a.mdp, a.mdp_run, e, qx, a.qa, a.qb, a.mode, a.eps_thr, ext, a.seed, (uint32_t)(a.env_id_offset + i), a.step_index + p, a.mgr0[p], a.sched[p], kv);
      DQL_SECTION("accumulate");
      if (STAGED) {
        if (o.cell >= 0) { atomicAdd(&sT[o.cell], (unsigned long long)o.target_fx); atomicAdd(&sM[o.cell], 1u); }
        if (o.cell_y >= 0) { atomicAdd(&sT[o.cell_y], (unsigned long long)o.target_y_fx); atomicAdd(&sM[o.cell_y], 1u); }
      } else {
        // global layout [4][N_CELLS]: a staged index in table b's half sits another N_CELLS further on
        if (o.cell >= 0) { const int g = o.cell + (o.cell >= DQL_N_CELLS ? DQL_N_CELLS : 0); atomicAdd(&a.acc_cur[g], (unsigned long long)o.target_fx); atomicAdd(&a.acc_cur[DQL_N_CELLS + g], 1ull); }
        if (o.cell_y >= 0) { const int g = o.cell_y + (o.cell_y >= DQL_N_CELLS ? DQL_N_CELLS : 0); atomicAdd(&a.acc_cur[g], (unsigned long long)o.target_y_fx); atomicAdd(&a.acc_cur[DQL_N_CELLS + g], 1ull); }
      }
      qx = o.next;  // the row of the state this period ended in = the next period's greedy row (the launch's tables act for all P)
      dec = o.decision; don = o.done; rfx = o.reward_fx;
      if (o.done) { done_code = e.code; goal = e.code == DQL_TERMINAL_SUCCESS; }
    }
    if (ELOG_MASKS && a.elog) {  // finished episodes of this period in env order: one ballot pair per wave (pkg/trainer.py:218-224 needs the order)
      const unsigned long long dm = __ballot(don != 0), sm = __ballot(goal);
      const long long w = i >> 6, nw = (a.n + 63) >> 6;
      unsigned long long* row = a.elog + (size_t)p * 2 * (size_t)nw;
      if ((tid & 63) == 0 && w < nw) { row[w] = dm; row[nw + w] = sm; }
    }
    // wave64 shuffle reductions -> per-wave totals
    dec_w += __popcll(__ballot(dec != 0)); don_w += __popcll(__ballot(don != 0)); rfx_lane += rfx;
    if (i < a.n) DQL_PHASE(e, 5);
    if (__ballot(done_code >= 0)) {  // wave-uniform: most periods of most waves finish no episode
#pragma unroll
      for (int k = 0; k <= DQL_TERMINAL_TIMEOUT; ++k) code_w[k] += (unsigned)__popcll(__ballot(done_code == k));
    }
  }
  DQL_SECTION("store");
  if (i < a.n) {
    store_env(e, a.sr, a.si, a.n, i, XMODE == X_ONLY ? x_only(a.c) : a.c);  // the atomics went out first: their round trip hides behind the state stores
    DQL_MARK_T(e, 6);
    DQL_WAVE_STORED(e, clk1);
  }
  rfx_w = wave_sum(rfx_lane);
  dec = dec_w; don = don_w; rfx = rfx_w;
  if (STAGED) {
    // the wave's statistics (wave-uniform) go out from lanes 0 .. 10, one value per lane: one LDS atomic per wave and, behind the barrier, one global
    // atomic per workgroup — not eleven of each from a single lane, one after the other
    const int lane = tid & 63;
    unsigned long long sv = lane == 0 ? (unsigned long long)dec : lane == 1 ? (unsigned long long)don : lane == 2 ? (unsigned long long)rfx : 0ull;
#pragma unroll
    for (int k = 0; k <= DQL_TERMINAL_TIMEOUT; ++k) if (lane == 4 + k) sv = (unsigned long long)code_w[k];
    if (lane < 4 + 7 && sv) atomicAdd(&sStat[lane], sv);
    __syncthreads();
    if (tid < 4 + 7) {
      const unsigned long long v = sStat[tid];
      unsigned long long* g = tid == 0 ? &a.stats->decisions : tid == 1 ? &a.stats->episodes : tid == 2 ? (unsigned long long*)&a.stats->reward_fx : &a.stats->by_code[tid < 4 ? 0 : tid - 4];
      if (v) atomicAdd(g, v);  // (slot 3 is spare and stays 0)
    }
    for (int t = 0; t < n_tab; ++t)
      for (int c = tid; c < ncell; c += BLOCK) {
        const unsigned int m = sM[t * DQL_N_CELLS + c];
        const unsigned long long s = sT[t * DQL_N_CELLS + c];
        if (s) atomicAdd(&a.acc_cur[t * DQL_ACC_B + c], s);
        if (m) atomicAdd(&a.acc_cur[t * DQL_ACC_B + DQL_N_CELLS + c], (unsigned long long)m);
      }
  } else if (tid == 0) {
    if (dec) atomicAdd(&a.stats->decisions, (unsigned long long)dec);
    if (don) atomicAdd(&a.stats->episodes, (unsigned long long)don);
    if (rfx) atomicAdd((unsigned long long*)&a.stats->reward_fx, (unsigned long long)rfx);
#pragma unroll
    for (int k = 0; k <= DQL_TERMINAL_TIMEOUT; ++k) if (code_w[k]) atomicAdd(&a.stats->by_code[k], (unsigned long long)code_w[k]);
  }
  DQL_PHASE_END(e, i < a.n, a.elog, a.n, i, tid);
  DQL_WAVE_END(clk0, clk1, a.elog, a.n, i, tid);
}

// The population kernel's body: k_step's body with the launch's per-agent arguments from the agent's descriptor (mgr0 / sched per period) and the
// bounds guard on the staged indices.  It is a copy on purpose: moving k_step's body into a shared force-inlined function — even without any change
// to it — changes the register allocation and schedule of all 19 k_step instances (the body is then simplified as a function of its own before it
// is inlined), and every measurement of this repository was taken on those instances.  A change to one of the two bodies belongs in the other.
template <typename T, int BLOCK, int TICK, int XMODE>
DQL_DEV void pop_step_body(const StepArgs<T>& a, const unsigned bid, const PopAgentDesc DQL_CONST_AS* d) {
  // several waves per workgroup: TD targets meet in LDS first (4x fewer global atomics on the hot cells of a big batch);
  // one wave per workgroup (small batches, latency-bound): 64 envs rarely share a cell, so each lane adds straight into the
  // global accumulators and the wave needs no LDS clear, no barrier and no flush scan (measured: -1.5 us of 26 at 4096 envs)
  constexpr bool STAGED = BLOCK > 64;
  __shared__ unsigned long long sT[STAGED ? 2 * DQL_N_CELLS : 1];  // staged index = table * N_CELLS + cell (StepOut::cell)
  __shared__ unsigned int sM[STAGED ? 2 * DQL_N_CELLS : 1];
  __shared__ unsigned long long sStat[4 + 7];  // decisions, episodes, reward sum, (spare), then the terminal histogram (codes 0 .. TERMINAL_TIMEOUT)
  DQL_PHASE_BEGIN(clk_start);
  warm_kernarg<(int)sizeof(PopArgs<T>)>();
  const int tid = threadIdx.x;
  DQL_WAVE_BEGIN(clk0);
  if ((int)bid >= a.env_blocks) {  // table-writer block (whole block takes this path: no barrier is skipped)
    const int c = ((int)bid - a.env_blocks) * BLOCK + tid;
    if (c < DQL_N_CELLS) {
      double qa = a.qa_m[c], qb = a.qb_m[c];
      if (a.have_prev) {
        qa = fold_cell(a.fold, a.qa_m, a.cnt_m, a.acc_prev, a.window, a.windowed, c);
        qb = fold_cell(a.fold, a.qb_m, a.cnt_m, a.acc_prev + DQL_ACC_B, a.window + DQL_ACC_B, a.windowed, c);
      }
      a.qa_pub[c] = qa; a.qb_pub[c] = qb;
    }
    return;
  }
  const int ncell = (a.c.working + 1) * DQL_CELLS_PER_LEVEL;
  const int n_tab = (a.c.quirks & DQL_Q_UPDATE_TABLE_A_ONLY) ? 1 : 2;  // tables that can receive targets (wave-uniform)
  if (STAGED) {
    for (int t = 0; t < n_tab; ++t)
      for (int c = tid; c < ncell; c += BLOCK) { sT[t * DQL_N_CELLS + c] = 0ull; sM[t * DQL_N_CELLS + c] = 0u; }
    if (tid < 4 + 7) sStat[tid] = 0ull;
    __syncthreads();
  }
  const long long i = (long long)bid * BLOCK + tid;
  long long dec = 0, don = 0, rfx = 0;
  bool goal = false;
  DQL_WAVE_END_VAR(clk1);
  // P agent periods per launch (option "periods_per_launch", default 1): the env stays in registers between them, so the state
  // round trip through HBM, the launch boundary and the table-writer work are paid once per P periods; the acting tables are
  // those of the launch for all P periods, every period's TD targets go to the launch's accumulators
  Env<T> e;
  QRow qx = QRow{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < a.n) {
    // the packed ints go first: their state index addresses the acting-table row, whose request then rides along with the
    // state quads instead of waiting for them (one memory round trip less at the head of the wave).  A fresh or reset env has
    // no previous state (idx -1): its row is never used, but the address must stay inside the table
    const int4 iv = a.si[i];
    qx = load_qrow(a.qa, a.qb, (unsigned)iv.x < (unsigned)(DQL_N_CELLS / DQL_N_ACTIONS) ? iv.x : 0);
    load_env(e, a.sr, iv, a.n, i, XMODE == X_ONLY ? x_only(a.c) : a.c);
    DQL_MARK_T(e, 2);
    DQL_PHASE_LOADED(e, clk_start);
  }
  long long dec_w = 0, don_w = 0, rfx_w = 0;  // per-wave totals over the periods of this launch (wave-uniform after the reductions)
  // the reward total is an integer (fixed point): every lane keeps its own sum over the launch's periods (< 32 x 2^50) and the wave adds them up ONCE, behind the
  // period loop — the 64-bit DPP reduction used to run in every period (45 instructions of each env wave's period)
  long long rfx_lane = 0;
  // terminal histogram of the wave over the launch: one ballot per CheckResult code and period instead of one global atomic per finished
  // episode (thousands per period on a handful of addresses at large batches)
  unsigned code_w[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  // XMODE (dql_device.hpp agent_period): in an x-axis kernel the config's two_axis is the constant 0 — every y-axis branch of the step folds away
  SimK<T> cfgk = a.c;
  if constexpr (XMODE == X_ONLY) cfgk.two_axis = 0;
  // register headroom (<= 2 waves per SIMD: 256 VGPRs): the manager tick's and the period's run-time constants move to VGPRs once per launch
  if constexpr (sizeof(T) == 4 && BLOCK < 512) cfgk = period_consts_in_vgprs(cfgk);
  // float64: the tick's constants are read from LDS.  As kernel arguments they are SGPR PAIRS — some 150 of them against 100 scalar registers — and the
  // compiler parked the overflow in VGPR lanes: ~850 v_readlane_b32 per physics tick, three quarters of the tick's instructions, around 264 float64 operations.
  // One copy per workgroup, read back where used (agent_period's plain loop keeps the compiler from hoisting the reads out of the tick loop again).
  __shared__ TickLds<T> sTickK;  // (float32: an unused byte)
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  // the Philox round keys (a launch constant) in VGPRs, where there are registers to spare (philox4x32)
  uint32_t kv_[20];
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4 && BLOCK < 512 && (TICK == TICK_LIT || TICK == TICK_PLAIN)) {  // (the VGPR-constant layouts have their registers spoken for: 112 SGPR spills with the keys against 47)
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)a.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(a.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  // ROUND 5: the two waves of a SIMD take turns at the issue priority.  The arbiter serves priority first, then AGE: of two waves running the same
  // program the older one is nearly unimpeded and the younger gets the leftover slots — at exactly two waves per SIMD the older half of the env
  // waves finished a 16-period launch after 272 us and the younger half then ran ALONE, at a lone wave's issue rate, for another 55 us
  // (profiles/r5_wave_tail.jsonl).  Alternating s_setprio by (period + hardware wave slot) parity gives each wave the head of the queue in every
  // other period: both finish together and the SIMD never runs half empty.  (A wave that shares its SIMD with nobody is unaffected.)
  // compiled into the layouts that serve several waves per SIMD only (the packed / VGPR-constant layouts fly batches of at most one env wave per SIMD:
  // nobody to take turns with, and the extra code cost them 0.8 %), and switched on by the host when the batch has more env waves than the device SIMDs
  constexpr bool FAIR = (TICK == TICK_PLAIN || TICK == TICK_LIT) && BLOCK >= 128;
  unsigned prio_role = 0u;
  bool fair_prio = false;
  if constexpr (FAIR) {
    fair_prio = a.fair_prio != 0;
    if (fair_prio) {
      unsigned hw_id;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
      prio_role = hw_id & 1u;  // wave slot parity: the two waves of a SIMD sit in slots 0 and 1
    }
  }
  for (int p = 0; p < a.n_periods; ++p) {
    // (giving the older wave the even periods instead, or the launch's last period to the younger one: 19.46 / 19.38 against 19.18 us per period)
    // (other patterns — the younger wave ahead in 12 of 16 periods, in all, in none — change nothing or bring the tail back: 19.19 / 20.25 / 20.29 us)
    if (fair_prio) { if ((((unsigned)p) ^ prio_role) & 1u) asm volatile("s_setprio 1"); else asm volatile("s_setprio 0"); }
    dec = 0; don = 0; rfx = 0; goal = false;
    int done_code = -1;
    if (i < a.n) {
      const int ext = (a.mode == MODE_EXTERNAL) ? (int)a.actions[i] : 2;
      if (a.mode == MODE_EXTERNAL) {  // the caller's actions are checked here, not by a host loop (dql_step): ax | ay << 2, both in 0..2
        const int ax = ext & 3, ay = (ext >> 2) & 3;
        if (ax > 2 || ay > 2 || (ext >> 4) || (!a.c.two_axis && ay != 0 && ay != 2)) atomicAdd(&a.stats->bad_actions, 1ull);
      }
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, a.mdp, a.mdp_run, e, qx, a.qa, a.qb, a.mode, a.eps_thr, ext, a.seed, (uint32_t)(a.env_id_offset + i), a.step_index + p, d->mgr0[p], d->sched[p], kv);
      DQL_SECTION("accumulate");
      // bounds guard (population only): a staged index outside [0, 2 N_CELLS) would land in another agent's accumulators when the
      // workgroup adds straight into global memory; drop it and count it (dql_pop_index_faults; the tests hold it at zero)
      const bool okx = (unsigned)o.cell < 2u * DQL_N_CELLS, oky = (unsigned)o.cell_y < 2u * DQL_N_CELLS;
      if ((o.cell >= 0 && !okx) || (o.cell_y >= 0 && !oky)) atomicAdd(d->faults, (unsigned long long)((o.cell >= 0 && !okx) + (o.cell_y >= 0 && !oky)));
      if (STAGED) {
        if (okx) { atomicAdd(&sT[o.cell], (unsigned long long)o.target_fx); atomicAdd(&sM[o.cell], 1u); }
        if (oky) { atomicAdd(&sT[o.cell_y], (unsigned long long)o.target_y_fx); atomicAdd(&sM[o.cell_y], 1u); }
      } else {
        if (okx) { const int g = o.cell + (o.cell >= DQL_N_CELLS ? DQL_N_CELLS : 0); atomicAdd(&a.acc_cur[g], (unsigned long long)o.target_fx); atomicAdd(&a.acc_cur[DQL_N_CELLS + g], 1ull); }
        if (oky) { const int g = o.cell_y + (o.cell_y >= DQL_N_CELLS ? DQL_N_CELLS : 0); atomicAdd(&a.acc_cur[g], (unsigned long long)o.target_y_fx); atomicAdd(&a.acc_cur[DQL_N_CELLS + g], 1ull); }
      }
      qx = o.next;  // the row of the state this period ended in = the next period's greedy row (the launch's tables act for all P)
      dec = o.decision; don = o.done; rfx = o.reward_fx;
      if (o.done) { done_code = e.code; goal = e.code == DQL_TERMINAL_SUCCESS; }
    }
    if (ELOG_MASKS && a.elog) {  // finished episodes of this period in env order: one ballot pair per wave (pkg/trainer.py:218-224 needs the order)
      const unsigned long long dm = __ballot(don != 0), sm = __ballot(goal);
      const long long w = i >> 6, nw = (a.n + 63) >> 6;
      unsigned long long* row = a.elog + (size_t)p * 2 * (size_t)nw;
      if ((tid & 63) == 0 && w < nw) { row[w] = dm; row[nw + w] = sm; }
    }
    // wave64 shuffle reductions -> per-wave totals
    dec_w += __popcll(__ballot(dec != 0)); don_w += __popcll(__ballot(don != 0)); rfx_lane += rfx;
    if (i < a.n) DQL_PHASE(e, 5);
    if (__ballot(done_code >= 0)) {  // wave-uniform: most periods of most waves finish no episode
#pragma unroll
      for (int k = 0; k <= DQL_TERMINAL_TIMEOUT; ++k) code_w[k] += (unsigned)__popcll(__ballot(done_code == k));
    }
  }
  DQL_SECTION("store");
  if (i < a.n) {
    store_env(e, a.sr, a.si, a.n, i, XMODE == X_ONLY ? x_only(a.c) : a.c);  // the atomics went out first: their round trip hides behind the state stores
    DQL_MARK_T(e, 6);
    DQL_WAVE_STORED(e, clk1);
  }
  rfx_w = wave_sum(rfx_lane);
  dec = dec_w; don = don_w; rfx = rfx_w;
  if (STAGED) {
    if ((tid & 63) == 0) {
      if (dec) atomicAdd(&sStat[0], (unsigned long long)dec);
      if (don) atomicAdd(&sStat[1], (unsigned long long)don);
      if (rfx) atomicAdd(&sStat[2], (unsigned long long)rfx);
#pragma unroll
      for (int k = 0; k <= DQL_TERMINAL_TIMEOUT; ++k) if (code_w[k]) atomicAdd(&sStat[4 + k], (unsigned long long)code_w[k]);
    }
    __syncthreads();
    for (int t = 0; t < n_tab; ++t)
      for (int c = tid; c < ncell; c += BLOCK) {
        const unsigned int m = sM[t * DQL_N_CELLS + c];
        if (m) { atomicAdd(&a.acc_cur[t * DQL_ACC_B + c], sT[t * DQL_N_CELLS + c]); atomicAdd(&a.acc_cur[t * DQL_ACC_B + DQL_N_CELLS + c], (unsigned long long)m); }
      }
    if (tid == 0) {
      dec = (long long)sStat[0]; don = (long long)sStat[1]; rfx = (long long)sStat[2];
#pragma unroll
      for (int k = 0; k <= DQL_TERMINAL_TIMEOUT; ++k) code_w[k] = (unsigned)sStat[4 + k];
    }
  }
  if (tid == 0) {
    if (dec) atomicAdd(&a.stats->decisions, (unsigned long long)dec);
    if (don) atomicAdd(&a.stats->episodes, (unsigned long long)don);
    if (rfx) atomicAdd((unsigned long long*)&a.stats->reward_fx, (unsigned long long)rfx);
#pragma unroll
    for (int k = 0; k <= DQL_TERMINAL_TIMEOUT; ++k) if (code_w[k]) atomicAdd(&a.stats->by_code[k], (unsigned long long)code_w[k]);
  }
  DQL_PHASE_END(e, i < a.n, a.elog, a.n, i, tid);
  DQL_WAVE_END(clk0, clk1, a.elog, a.n, i, tid);
}
// grid: n_active x blocks_per_agent env blocks (slot-major), then n_active x writer_blocks table-writer blocks; a block serves one agent
template <typename T, int BLOCK, int TICK, int XMODE> __global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(step_min_waves_per_simd(BLOCK, (int)sizeof(T)), step_waves_per_simd(BLOCK)))) void k_step_pop(PopArgs<T> pa) {
  const int b = (int)blockIdx.x, env_total = pa.n_active * pa.blocks_per_agent;
  const int slot = b < env_total ? b / pa.blocks_per_agent : (b - env_total) / pa.writer_blocks;  // wave-uniform
  const PopAgentDesc DQL_CONST_AS* d = pa.desc + slot;
  const int k = pa.agent[slot];
  const unsigned bid = b < env_total ? (unsigned)(k * pa.blocks_per_agent + (b - slot * pa.blocks_per_agent)) : (unsigned)(pa.s.env_blocks + (b - env_total - slot * pa.writer_blocks));
  StepArgs<T> a = pa.s;
  a.c.working = d->working;
  a.mdp = (const MdpK<T> DQL_CONST_AS*)d->mdp;
  a.qa = d->qa; a.qb = d->qb; a.acc_cur = d->acc_cur;
  a.qa_m = d->qa_m; a.qb_m = d->qb_m; a.cnt_m = d->cnt_m; a.qa_pub = d->qa_pub; a.qb_pub = d->qb_pub; a.acc_prev = d->acc_prev; a.window = d->window;
  a.fold = FoldK{d->fold.alpha_tab, d->fold.n_tab, d->fold.alpha_min, d->fold.per_step, d->fold.n_launch}; a.stats = d->stats; a.elog = d->elog;
  a.env_id_offset = -(long long)k * pa.blocks_per_agent * BLOCK;  // the env's id within its agent keys the RNG, with the agent's seed
  a.step_index = d->step_index; a.seed = d->seed; a.eps_thr = d->eps_thr; a.have_prev = d->have_prev; a.windowed = 0;
  pop_step_body<T, BLOCK, TICK, XMODE>(a, bid, d);
}


// fold the last launch's accumulators into the master tables outside a launch (host table access, level switch, rank sync)
struct FlushArgs { double* qa_m; double* qb_m; double* cnt_m; long long* acc; long long* window; FoldK fold; int windowed; };
__global__ void k_flush(FlushArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < DQL_N_CELLS) {
    fold_cell(a.fold, a.qa_m, a.cnt_m, a.acc, a.window, a.windowed, c);
    fold_cell(a.fold, a.qb_m, a.cnt_m, a.acc + DQL_ACC_B, a.window + DQL_ACC_B, a.windowed, c);
  }
}
// multi-GPU: fold the all-reduced window into the base tables; master and both acting buffers restart from the base
struct WindowArgs { double* qa_base; double* qb_base; double* count_base; double* qa_m; double* qb_m; double* cnt_m; double* tb0; double* tb1; double* tbb0; double* tbb1; long long* window; FoldK fold; };
__global__ void k_apply_window(WindowArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= DQL_N_CELLS) return;
  for (int t = 0; t < 2; ++t) {  // table a first: the shared counter orders the learning rates
    long long* w = a.window + t * DQL_ACC_B;
    double* base = t ? a.qb_base : a.qa_base;
    const long long Tsum = w[c], m = w[DQL_N_CELLS + c];
    if (m > 0) {
      base[c] = fold_q(a.fold, base[c], a.count_base[c], Tsum, m);
      a.count_base[c] += (double)m;
      w[c] = 0; w[DQL_N_CELLS + c] = 0;
    }
  }
  const double qa = a.qa_base[c], qb = a.qb_base[c];
  a.qa_m[c] = qa; a.qb_m[c] = qb; a.cnt_m[c] = a.count_base[c]; a.tb0[c] = qa; a.tb1[c] = qa; a.tbb0[c] = qb; a.tbb1[c] = qb;
}
__global__ void k_mark_reset(int4* si, const uint8_t* mask, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mask && !mask[i]) return;
  int4 v = si[i];
  v.w |= (FL_DONE << 8);
  si[i] = v;
}
// holds a stream for `ticks` of the 100 MHz wall clock (cohort phase offset, dql_diag_delay): one wave, exits on time or on the iteration bound
__global__ void k_delay(unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  for (int i = 0; i < (1 << 22) && wall_clock64() - t0 < ticks; ++i) __builtin_amdgcn_s_sleep(8);
}
__global__ void k_transfer(double* qa, double* qb, int k, int src, double ratio) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= DQL_CELLS_PER_LEVEL) return;
  qa[k * DQL_CELLS_PER_LEVEL + i] = qa[src * DQL_CELLS_PER_LEVEL + i] * ratio;
  qb[k * DQL_CELLS_PER_LEVEL + i] = qb[src * DQL_CELLS_PER_LEVEL + i] * ratio;
}

// ---- stateless operators ----
template <typename T> __global__ void k_discretise(MdpK<T> c, const double* p, const double* v, const double* acc, const double* ang, long long n, int* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = discretise(c, (T)p[i], (T)v[i], (T)acc[i], (T)ang[i]);
}
template <typename T>
__global__ void k_mdp_transition(MdpK<T> c, long long n, uint32_t stages, const uint8_t* action, const double* obs, double* ms, const int* prev_idx,
                                 int* idx_io, double* reward_out, uint8_t* done_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T sp = (T)ms[0 * n + i], shp_p = (T)ms[1 * n + i], shp_v = (T)ms[2 * n + i], shp_a = (T)ms[3 * n + i], cum = (T)ms[4 * n + i];
  int step_count = (int)ms[5 * n + i], cur_check = (int)ms[6 * n + i], code = (int)ms[7 * n + i];
  const T px = (T)obs[0 * n + i], py = (T)obs[1 * n + i], vx = (T)obs[2 * n + i], ax = (T)obs[3 * n + i], pitch = (T)obs[4 * n + i], z = (T)obs[5 * n + i];
  const bool contact = obs[6 * n + i] != 0.0;
  if (stages & DQL_MDP_ACTION) sp = continuous_action(c, sp, (int)action[i]);
  int idx = idx_io[i];
  if (stages & DQL_MDP_DISCRETISE) { idx = discretise(c, px, vx, ax, pitch); idx_io[i] = idx; }
  const int sidx = idx < 0 ? 0 : idx;
  if (stages & DQL_MDP_CHECK) {
    // SimulationMdp.check has no goal logic: feeding prev = -1 disables that branch (pkg/mdp.py:784-845)
    code = mdp_check(c, step_count, cur_check, code, (stages & DQL_MDP_SIMULATION) ? -1 : prev_idx[i], sidx, contact, px, py, z);
    done_out[i] = code <= DQL_TERMINAL_TIMEOUT;
  }
  if (stages & DQL_MDP_REWARD) reward_out[i] = (double)mdp_reward(c, shp_p, shp_v, shp_a, cum, code, sidx, px, vx, sp);
  ms[0 * n + i] = sp; ms[1 * n + i] = shp_p; ms[2 * n + i] = shp_v; ms[3 * n + i] = shp_a; ms[4 * n + i] = cum;
  ms[5 * n + i] = step_count; ms[6 * n + i] = cur_check; ms[7 * n + i] = code;
}
// the 100 Hz manager tick of the fused kernel (manager_states + manager_obs) replayed over scripted series, one lane per series
template <typename T>
__global__ void k_manager_run(SimK<T> c, long long n_series, long long n_ticks, const double* in, const uint8_t* contact, unsigned long long seed, double* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_series) return;
  Env<T> e;
  memset(&e, 0, sizeof(e));
  e.kal_x_P = T(1.0); e.kal_y_P = T(1.0); e.mp_r = c.mp_r; e.mp_w = c.mp_w;
  for (long long t = 0; t < n_ticks; ++t) {
    const double* r = in + (i * n_ticks + t) * 14;
    for (int k = 0; k < 3; ++k) { e.p[k] = (T)r[k]; e.v[k] = (T)r[3 + k]; }
    for (int k = 0; k < 4; ++k) e.q[k] = (T)r[6 + k];
    e.mp_x = (T)r[10]; e.mp_y = (T)r[11]; e.mp_u = (T)r[12]; e.mp_v = (T)r[13];
    if (contact[i * n_ticks + t]) e.flags |= FL_CONTACT;
    T R[9], cy, sy;
    quat_to_R(e.q, R); yaw_cs(R, cy, sy);
    manager_states(R, cy, sy, e.v[2], e.vz_state, e.yw_state);
    manager_obs(c, e, cy, sy, t, (uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0u, (uint32_t)i, (uint32_t)t);
    double* o = out + (i * n_ticks + t) * 12;
    o[0] = e.obs_px; o[1] = e.obs_py; o[2] = e.obs_vx; o[3] = e.obs_vy; o[4] = e.obs_ax; o[5] = e.obs_ay;
    o[6] = e.vz_state; o[7] = e.yw_state; o[8] = e.mp_x; o[9] = e.mp_y; o[10] = e.mp_u; o[11] = e.mp_v;
  }
}
// the plant of the fused kernel (plant_step + rotor_filter + platform_contact) replayed open loop, one lane per series (dql_plant_run)
template <typename T>
__global__ void k_plant_run(SimK<T> c, long long n_series, long long n_ticks, const double* init, const double* rotor_cmd, double* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_series) return;
  Env<T> e;
  memset(&e, 0, sizeof(e));
  const double* s0 = init + i * 21;
  for (int k = 0; k < 3; ++k) { e.p[k] = (T)s0[k]; e.v[k] = (T)s0[3 + k]; e.w[k] = (T)s0[10 + k]; }
  for (int k = 0; k < 4; ++k) { e.q[k] = (T)s0[6 + k]; e.om[k] = (T)s0[13 + k]; }
  e.mp_x = (T)s0[17]; e.mp_y = (T)s0[18]; e.mp_u = (T)s0[19]; e.mp_v = (T)s0[20];
  for (long long t = 0; t < n_ticks; ++t) {
    const double* r = rotor_cmd + (i * n_ticks + t) * 4;
    const T cmd[4] = {(T)r[0], (T)r[1], (T)r[2], (T)r[3]};
    T R[9];
    quat_to_R(e.q, R);
    plant_step(c, e, R);
    rotor_filter(c, e, cmd);
    platform_contact(c, e);
    double* o = out + (i * n_ticks + t) * 20;
    for (int k = 0; k < 3; ++k) { o[k] = e.p[k]; o[3 + k] = e.v[k]; o[10 + k] = e.w[k]; }
    for (int k = 0; k < 4; ++k) { o[6 + k] = e.q[k]; o[13 + k] = e.om[k]; }
    o[17] = e.mp_x; o[18] = e.mp_y; o[19] = (e.flags & FL_CONTACT) ? 1.0 : 0.0;
  }
}
// ---- the control-side functions of the tick replayed alone (dql_butterworth_run, dql_kalman_run, dql_pid_run, dql_attitude_run,
// dql_platform_run): the SAME device functions the fused step calls, one lane, so that each can be held against the reference's own
// outputs (golden vectors G8, G9, G11) in float64 AND in the float32 forms every throughput figure runs on ----
template <typename T> struct FiltK { T dt, bw_k1, bw_k2, bw_inv, bw_b2, bw_a2, bw_a3; };
template <typename T> static FiltK<T> make_filtk(double bc) {  // pkg/filters.py:94-106, as make_simk has it
  const double denom = 1 + bc * bc + 1.414 * bc;
  FiltK<T> d;
  d.dt = T(0); d.bw_inv = (T)(1.0 / denom); d.bw_k1 = (T)(bc * bc - 1.414 * bc + 1); d.bw_k2 = (T)(-2 * bc * bc + 2);
  d.bw_b2 = (T)(2.0 / denom); d.bw_a2 = (T)((-2 * bc * bc + 2) / denom); d.bw_a3 = (T)((bc * bc - 1.414 * bc + 1) / denom);
  return d;
}
template <typename T> __global__ void k_butterworth_run(FiltK<T> c, const double* x, long long n, double* y) {  // pkg/filters.py:98-109 from zero histories
  if (blockIdx.x || threadIdx.x) return;
  T x1 = T(0), x2 = T(0), y1 = T(0), y2 = T(0), y3 = T(0);
  for (long long i = 0; i < n; ++i) y[i] = (double)butterworth(c, (T)x[i], x1, x2, y1, y2, y3);
}
// KalmanFilter3D.filter over a velocity series (pkg/filters.py:53-80): z = dv / dt with the timestamps 0.01 i, dt <= 0 -> 0.01 (dt_le0[i] forces that branch)
template <typename T> __global__ void k_kalman_run(T Q, T Rm, const double* vel, const uint8_t* dt_le0, long long n, double* acc) {
  if (blockIdx.x || threadIdx.x) return;
  T x[3] = {T(0), T(0), T(0)}, P[3] = {T(1), T(1), T(1)};
  for (long long i = 1; i < n; ++i) {
    T dt_ = dt_le0[i] ? T(0.0) : (T)(0.01 * (double)i) - (T)(0.01 * (double)(i - 1));
    if (dt_ <= T(0.0)) dt_ = T(0.01);
    for (int k = 0; k < 3; ++k) acc[(i - 1) * 3 + k] = (double)kalman1d(x[k], P[k], Q, Rm, ((T)vel[i * 3 + k] - (T)vel[(i - 1) * 3 + k]) / dt_);
  }
}
// PID.output replay (pkg/pid.py:62-104, Kd = 0): the plant state is sampled every 5th tick, tick times are 0.002 (i + 1)
template <typename T> struct PidP { T kp, ki, lo, hi, wind, sp; };
template <typename T> __global__ void k_pid_run(FiltK<T> c, PidP<T> p, const double* state, long long n, double* effort, double* integral) {
  if (blockIdx.x || threadIdx.x) return;
  T integ = T(0), x1 = T(0), x2 = T(0), y1 = T(0), y2 = T(0), y3 = T(0), st = T(0), prev_t = T(0);
  for (long long i = 0; i < n; ++i) {
    const T t = (T)(0.002 * (double)(i + 1));
    if (i % 5 == 0) st = (T)state[i];
    c.dt = t - prev_t;
    effort[i] = (double)pid_output(c, p.kp, p.ki, p.lo, p.hi, p.wind, p.sp, st, integ, x1, x2, y1, y2, y3);
    integral[i] = (double)integ;
    prev_t = t;
  }
}
// AttitudeController.compute_rotor_velocities (pkg/attitude_controller.py:107-156) for n samples: quaternion (x, y, z, w) as ROS has it, body rates,
// cmd = roll, pitch, yaw rate, thrust -> commanded rotor speeds.  xonly: the x-axis closed form the x-axis kernels compile in (roll command exactly 0)
template <typename T> __global__ void k_attitude_run(SimK<T> s, const double* quat_xyzw, const double* omega, const double* cmd, long long n, int xonly, double* rotor) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T q[4] = {(T)quat_xyzw[i * 4 + 3], (T)quat_xyzw[i * 4 + 0], (T)quat_xyzw[i * 4 + 1], (T)quat_xyzw[i * 4 + 2]};
  const T w[3] = {(T)omega[i * 3], (T)omega[i * 3 + 1], (T)omega[i * 3 + 2]};
  T R[9], cy, sy, ct, rn, B[9], out[4];
  quat_to_R(q, R); yaw_cs(R, cy, sy, ct, rn);
  make_B((T)cmd[i * 4 + 1], (T)cmd[i * 4 + 0], B);
  attitude(s, R, w, B, cy, sy, ct, rn, (T)cmd[i * 4 + 2], (T)cmd[i * 4 + 3], out, xonly != 0);
  for (int k = 0; k < 4; ++k) rotor[i * 4 + k] = (double)out[k];
}
// MovingPlatform.compute_trajectory (pkg/moving_platform.py:87-127) from phase 0: x, y, u, v at successive 100 Hz ticks.  carry > 0: sine and cosine
// are evaluated at every carry-th tick only and rotated through the constant phase step in between — what the fused float32 step does inside an
// agent period (platform_update with a PlatRec; four or five manager ticks per period)
template <typename T> __global__ void k_platform_run(SimK<T> s, long long n, int carry, double* out) {
  if (blockIdx.x || threadIdx.x) return;
  Env<T> e;
  memset(&e, 0, sizeof(e));
  e.mp_r = s.mp_r; e.mp_w = s.mp_w;
  PlatRec<T> rec = PlatRec<T>{};
  for (long long i = 0; i < n; ++i) {
    if (carry > 0) platform_update(s, e, &rec, i % carry == 0);
    else platform_update(s, e);
    out[i * 4] = (double)e.mp_x; out[i * 4 + 1] = (double)e.mp_y; out[i * 4 + 2] = (double)e.mp_u; out[i * 4 + 3] = (double)e.mp_v;
  }
}
// exhaustive self-test of sqrt_pos (dql_diag_selftest_sqrt): inputs with bit patterns lo .. hi against (float)sqrt((double)x)
__global__ void k_selftest_sqrt(unsigned lo, unsigned hi, unsigned long long* bad) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long n = 0;
  for (unsigned long long b = lo + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b <= hi; b += stride) {
    const float x = __uint_as_float((unsigned)b);
    if (__float_as_uint(sqrt_pos(x)) != __float_as_uint((float)__builtin_sqrt((double)x))) ++n;
  }
  if (n) atomicAdd(bad, n);
}
template <typename T> __global__ void k_place(int init_mode, T p_max, const double* x0, const double* mp, long long n, double* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (double)place_axis(init_mode, (T)x0[i], (T)mp[i], p_max);
}
__global__ void k_predict(const double* qa, const double* qb, const int* idx, long long n, uint8_t* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint8_t)agent_predict(qa, qb, idx[i]);
}
// ordered replay of DoubleQLearningAgent.update (pkg/double_q_learning.py:91-146): inherently sequential -> one lane
// one DoubleQLearningAgent.update (pkg/double_q_learning.py:91-146); returns the updated cell's new value
DQL_DEV double agent_update_one(double* qa, double* qb, double* count, int sa, int ns, double alpha, double gamma, double reward, uint32_t quirks, bool coin, bool done) {
  const bool dbl = !(quirks & DQL_Q_UPDATE_TABLE_A_ONLY);  // Double Q-learning: coin picks the table, the other one values (B1/B2 off)
  count[sa] += 1;
  const bool sel_b = dbl && coin;
  double* qsel = sel_b ? qb : qa;
  const double* qval = dbl ? (sel_b ? qa : qb) : qa;
  const double q0 = qsel[ns * 3], q1 = qsel[ns * 3 + 1], q2 = qsel[ns * 3 + 2];
  const int b = argmax3(q0, q1, q2);
  const double best = qval[ns * 3 + b];
  const int mask = (quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) ? (idx_pos(sa / 3) != idx_pos(ns)) : !done;
  const double loss = alpha * (reward + (gamma * best) * (double)mask - qsel[sa]);
  qsel[sa] += loss;
  return qsel[sa];
}
__global__ void k_update_seq(double* qa, double* qb, double* count, const int* sa, const int* ns, const double* alpha, double gamma,
                             const double* reward, long long n, uint32_t quirks, const uint8_t* coin, const uint8_t* done) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (long long i = 0; i < n; ++i) agent_update_one(qa, qb, count, sa[i], ns[i], alpha[i], gamma, reward[i], quirks, coin && coin[i] != 0, done && done[i] != 0);
}
// resident agent (dql_agent_*): arguments and results in pinned host memory, read and written by the kernel itself
struct AgentUpdIn { int sa, ns; double alpha, reward; int coin, done; };
struct AgentUpdOut { double q_new, count_new; };
struct AgentUpdTail { int next_action; int pad; };  // predict(next state of the LAST transition) on the updated tables: the reference's loop asks for it next
__global__ void k_update_resident(double* qa, double* qb, double* count, const AgentUpdIn* in, AgentUpdOut* out, long long n, double gamma, uint32_t quirks) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (long long i = 0; i < n; ++i) {
    const AgentUpdIn u = in[i];
    out[i].q_new = agent_update_one(qa, qb, count, u.sa, u.ns, u.alpha, gamma, u.reward, quirks, u.coin != 0, u.done != 0);
    out[i].count_new = count[u.sa];
  }
  AgentUpdTail* tail = (AgentUpdTail*)(out + n);
  tail->next_action = agent_predict((const double*)qa, (const double*)qb, in[n - 1].ns);
  __threadfence_system();
}
// one transition, arguments by value (dql_agent_mirror_update): nothing to read over PCIe, one record to write.  The arithmetic of
// agent_update_one + agent_predict, spelled so that all eight table reads (both tables' row of the next state, the cell, its counter) are
// independent and issue together: on an otherwise idle GPU each dependent read is a full trip to HBM, and five of them were the kernel.
// `seq`: the call's sequence number, stored LAST (system-scope release): the host reads the record as soon as it sees the number, without
// waiting for the stream to report the kernel complete (wait_posted)
struct AgentOneOut { double q_new, count_new; int next_action; unsigned seq; };
__global__ void k_update_one(double* qa, double* qb, double* count, int sa, int ns, double alpha, double gamma, double reward, uint32_t quirks, int coin, int done, AgentOneOut* out, unsigned seq) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const bool dbl = !(quirks & DQL_Q_UPDATE_TABLE_A_ONLY);
  const bool sel_b = dbl && coin != 0;
  double ra[3], rb[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ra[k] = qa[ns * 3 + k]; rb[k] = qb[ns * 3 + k]; }
  double* qsel = sel_b ? qb : qa;
  const double cur = qsel[sa], cnt = count[sa] + 1;
  const bool val_b = dbl && !sel_b;  // the table that values the greedy action: the other one (Double Q-learning) or Q_table_a itself (B2)
  const int b = sel_b ? argmax3(rb[0], rb[1], rb[2]) : argmax3(ra[0], ra[1], ra[2]);
  const double va = b == 0 ? ra[0] : (b == 1 ? ra[1] : ra[2]), vb = b == 0 ? rb[0] : (b == 1 ? rb[1] : rb[2]);
  const double best = val_b ? vb : va;
  const int mask = (quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) ? (idx_pos(sa / 3) != idx_pos(ns)) : !done;
  const double loss = alpha * (reward + (gamma * best) * (double)mask - cur);
  const double q_new = cur + loss;
  qsel[sa] = q_new; count[sa] = cnt;
  if (sa / 3 == ns) {  // the next state's row contains the updated cell
    const int k = sa % 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) if (j == k) { if (sel_b) rb[j] = q_new; else ra[j] = q_new; }
  }
  out->q_new = q_new; out->count_new = cnt;
  out->next_action = argmax3((ra[0] + rb[0]) / 2, (ra[1] + rb[1]) / 2, (ra[2] + rb[2]) / 2);
  __threadfence_system();
  __hip_atomic_store(&out->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_predict_resident(const double* qa, const double* qb, const int* idx, long long n, uint8_t* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint8_t)agent_predict(qa, qb, idx[i]);
  __threadfence_system();
}
// what TrainingLandingEnv.step returns, gathered per env into pinned host memory (dql_step_outputs)
struct StepOutRec { int idx_x, idx_y, step_count, code_flags; double reward, cum; };
template <typename T> __global__ void k_step_outputs(const Quad<T>* __restrict__ sr, const int4* __restrict__ si, long long n, StepOutRec* out,
                                                      const unsigned long long* bad_src, unsigned long long* bad_dst, unsigned* posted, unsigned seq) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int4 iv = si[i];
    StepOutRec r;
    r.idx_x = iv.x; r.idx_y = iv.y; r.step_count = iv.z & 0xffff; r.code_flags = iv.w & 0xffff;
    r.reward = (double)sr[14 * n + i].a; r.cum = (double)sr[10 * n + i].b;
    out[i] = r;
  }
  if (i == 0) *bad_dst = *bad_src;  // StatsDev::bad_actions rides along: no copy-engine command between the kernel and the wait
  __threadfence_system();
  if (posted) {  // single-workgroup grids only (wave-uniform): every record of the workgroup is out before the number is
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(posted, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// ---- one-shot peer-to-peer exchange of the window accumulators (second step) ----
// Exchange buffer of a rank: slots[2 parities][world][DQL_ACC_LEN] int64, then flags[2 parities][DQL_P2P_MAX_RANKS] (the sequence
// number of the last exchange a peer has pushed for that parity).  Every rank writes its window into slot [parity][its rank] of
// EVERY rank's buffer (its own included) — world concurrent writes over the direct links, 90 KB each — then raises its flag in every
// buffer (system-scope release); the receiver waits for all flags of the parity (system-scope acquire, bounded spin) and sums the slots
// in rank order into its window: one hop, no ring.  Two parities suffice: a rank can only be one exchange ahead of a peer (its next
// wait needs that peer's next flag).  Buffers are uncached device memory, so a peer's writes are never shadowed by a stale L2 line.
struct P2PPushArgs { const long long* window; unsigned long long* peer[DQL_P2P_MAX_RANKS]; int rank, world, parity; };
DQL_DEV unsigned long long* p2p_slot(unsigned long long* buf, int world, int parity, int r) { return buf + ((size_t)parity * world + r) * DQL_ACC_LEN; }
DQL_DEV unsigned long long* p2p_flags(unsigned long long* buf, int world, int parity) { return buf + (size_t)2 * world * DQL_ACC_LEN + (size_t)parity * DQL_P2P_MAX_RANKS; }
__global__ void k_p2p_push(P2PPushArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= DQL_ACC_LEN) return;
  const unsigned long long v = (unsigned long long)a.window[c];
  for (int r = 0; r < a.world; ++r) __builtin_nontemporal_store(v, &p2p_slot(a.peer[r], a.world, a.parity, a.rank)[c]);
}
// after the push kernel has completed (stream order: its writes are released at the kernel boundary)
__global__ void k_p2p_signal(P2PPushArgs a, unsigned long long seq) {
  const int r = threadIdx.x;
  if (r < a.world) __hip_atomic_store(&p2p_flags(a.peer[r], a.world, a.parity)[a.rank], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ONE waiter per exchange (a single wave; lane r polls peer r's flag): the verdict it leaves — verdict[0] = the last exchange every
// peer showed up for, verdict[1] = the first exchange that was given up on (0 = none) — is what the sum kernel obeys, so a window is
// either the full sum or untouched, never summed by some workgroups and not by others
__global__ void k_p2p_wait(const unsigned long long* mine, int world, int parity, unsigned long long seq, unsigned long long* verdict, long long spin_limit) {
  const int r = threadIdx.x;
  bool good = true;
  if (r < world) {
    const unsigned long long* f = p2p_flags(const_cast<unsigned long long*>(mine), world, parity);
    long long spins = 0;  // every lane reaches an exit: spin_limit polls, then the exchange is reported as failed
    while (__hip_atomic_load(&f[r], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
      if (++spins > spin_limit) { good = false; break; }
      __builtin_amdgcn_s_sleep(8);
    }
  }
  const bool all_good = __ballot(!good) == 0ull;
  if (r == 0) {
    if (all_good) verdict[0] = seq;
    else if (verdict[1] == 0ull) verdict[1] = seq;
  }
}
__global__ void k_p2p_sum(unsigned long long* mine, long long* window, int world, int parity, unsigned long long seq, const unsigned long long* verdict) {
  if (verdict[0] != seq) return;  // given up on: the window stays this rank's own (wave-uniform, whole grid)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= DQL_ACC_LEN) return;
  unsigned long long sum = 0;
  for (int r = 0; r < world; ++r) sum += __builtin_nontemporal_load(&p2p_slot(mine, world, parity, r)[c]);
  window[c] = (long long)sum;
}

// ---- greedy roll-outs (dql_rollout) ----
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
  if constexpr (sizeof(T) == 4) {
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

// ---- sequential learners (dql_ensemble) ----
// One learner per lane (csrc/dql_learner.hpp: learner_periods), workgroups of one wave as in k_rollout; the env stays in registers for all periods of the launch,
// the tables are the lane's own [DQL_N_CELLS] slices (per-lane global pointers, ordinary vector loads and stores, no atomics).
template <typename T> struct LearnArgs {
  SimK<T> c;
  const MdpK<T> DQL_CONST_AS* mdp;
  MdpRun<T> mdp_run;
  LearnSched sched;
  LearnMem mem;
  Quad<T>* sr; int4* si;
  const long long DQL_CONST_AS* mgr0; const int DQL_CONST_AS* tick_sched;  // [n_periods] (fill_schedule from period j0)
  unsigned long long seed;
  long long j0;
  int n_periods;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn(LearnArgs<T> a) {
  const int tid = threadIdx.x;
  const long long l = (long long)blockIdx.x * 64 + tid;
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
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)a.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(a.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  learner_periods<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.sched, a.mem, a.sr, a.si, a.seed, l, l < a.mem.n, a.j0, a.n_periods, a.mgr0, a.tick_sched, kv);
}
// transfer_learning on every learner's tables: Q[l][k] = Q[l][src] * ratio (k_transfer's arithmetic)
__global__ void k_ens_transfer(double* qa, double* qb, long long n, int k, int src, double ratio) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * DQL_CELLS_PER_LEVEL) return;
  const long long l = t / DQL_CELLS_PER_LEVEL; const int i = (int)(t - l * DQL_CELLS_PER_LEVEL);
  double* a = qa + l * DQL_N_CELLS; double* b = qb + l * DQL_N_CELLS;
  a[k * DQL_CELLS_PER_LEVEL + i] = a[src * DQL_CELLS_PER_LEVEL + i] * ratio;
  b[k * DQL_CELLS_PER_LEVEL + i] = b[src * DQL_CELLS_PER_LEVEL + i] * ratio;
}

// ---- per-learner curriculum levels ----
// k_learn over a worklist (csrc/dql_advance.hpp: build_worklist): wave w flies the learners worklist[64 w .. 64 w + 63] (-1: an inactive lane), all of
// them at level wave_level[w] — a scalar load — from which follow SimK::working, the level's MdpK (a.a.mdp is the array of all five) and the level's
// exploration table and freeze rules.  After that the call to learner_periods is k_learn's.
template <typename T> struct LearnLevelsArgs {
  LearnArgs<T> a;                          // a.mdp: [DQL_MAX_LEVELS]; a.sched: the learning rates (its per-level members are replaced by lv[level])
  const LevelSched DQL_CONST_AS* lv;       // [DQL_MAX_LEVELS]
  const int* worklist;                     // [64 n_waves]
  const int DQL_CONST_AS* wave_level;      // [n_waves]
  int n_waves;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_levels(LearnLevelsArgs<T> g) {
  const LearnArgs<T>& a = g.a;
  const int tid = threadIdx.x;
  const int w = (int)blockIdx.x;
  if (w >= g.n_waves) return;
  const int level = g.wave_level[w];
  if ((unsigned)level >= (unsigned)DQL_MAX_LEVELS) { if (tid == 0) a.mem.faults[0] += 1ull; return; }  // never taken unless a bug (the host builds the worklist)
  const long long l = (long long)g.worklist[(long long)w * 64 + tid];
  SimK<T> cl = a.c;
  cl.working = level;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // as in k_learn
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
  const LevelSched DQL_CONST_AS* lv = g.lv + level;
  const LearnSched sc{a.sched.alpha_tab, a.sched.n_alpha, a.sched.alpha_min, lv->eps_tab, lv->n_eps, lv->window, lv->min_successes, lv->max_episodes};
  learner_periods<TICK, XMODE>(cl, cfgk, tc, a.mdp + level, a.mdp_run, sc, a.mem, a.sr, a.si, a.seed, l, l >= 0 && l < a.mem.n, a.j0, a.n_periods, a.mgr0, a.tick_sched, kv);
}
// an advance point: every learner takes advance_learner's step by itself (its own thread moves its own 2 x 567 cells; ordinary vector stores, nothing shared)
// -- but for the `faults` word: advance_learner's `faults[0] += 1` is a plain add that threads of all waves may make at once, as learner_periods' is.  Counts
// can be lost, a nonzero word cannot become zero, and nonzero is all that index_faults() is read for.
__global__ void k_ens_advance(LearnMem mem, AdvanceMem adv, AdvanceRule rule, int4* si, long long j, int n_cells) {
  const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= mem.n) return;
  (void)advance_learner(mem, adv, rule, si, l, j, n_cells);
}

// ---- greedy scoring (dql_score / dql_ensemble_score) ----
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
  const int k = (int)blockIdx.x / a.blocks_per_table;                  // table set (wave-uniform)
  const int i = ((int)blockIdx.x - k * a.blocks_per_table) * 64 + tid;  // env within its table set = its RNG key
  const long long g = (long long)blockIdx.x * 64 + tid;                // log column: every lane of the grid is an env (envs_per_table is a multiple of 64)
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
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)a.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(a.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  const double* qa = a.qa + (size_t)k * DQL_N_CELLS;
  const double* qb = a.qb + (size_t)k * DQL_N_CELLS;
  const ScoreTally t = score_episodes<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.init, qa, qb, a.seed, (uint32_t)i, a.max_steps, a.episodes, a.mgr0, a.sched, kv, a.log, g);
  if (tid == 0) {
    unsigned long long* row = a.by_code + (size_t)k * SCORE_N_COLS;
#pragma unroll
    for (int col = 0; col < SCORE_N_COLS; ++col) if (t.by_code[col]) atomicAdd(&row[col], (unsigned long long)t.by_code[col]);
    if (t.steps) atomicAdd(&a.steps_sum[k], t.steps);
  }
}

struct dql_ctx {
  dql_config cfg;
  int device = 0;
  long long n = 0;
  unsigned long long seed = 0;
  long long env_id_offset = 0;
  int dtype = DQL_F32;
  size_t real_size = 4;
  void* sr = nullptr;  // Quad<T>[NQ_REAL][n]
  int4* si = nullptr;
  double *qa = nullptr, *qb = nullptr, *count = nullptr;          // MASTER tables: every accumulator folded except the last launch's (`pending`)
  double* tbb[2] = {nullptr, nullptr};                            // ... and of Q_table_b (it learns too unless the table-a-only quirk is set)
  double* tb[2] = {nullptr, nullptr};                             // ACTING copies of Q_table_a: launch j reads tb[j & 1], its writer blocks fill tb[(j + 1) & 1]
  double *qa_base = nullptr, *qb_base = nullptr, *count_base = nullptr;               // multi-GPU base tables
  long long* acc[2] = {nullptr, nullptr};                         // accumulators: launch j adds into acc[j & 1]; its writer blocks fold and clear acc[(j + 1) & 1]
  long long *window = nullptr, *window_own = nullptr;
  double* alpha_tab = nullptr; int n_tab = 0;
  StatsDev* stats = nullptr;
  long long step_index = 0;      // agent periods launched so far (the tick schedule is a pure function of it)
  long long launch_index = 0;    // launches so far: its parity selects the ping-pong buffers (a launch may cover several periods)
  int periods_per_launch = 1;    // option "periods_per_launch"
  int pending_periods = 1;       // agent periods the pending accumulators cover (learning-rate steps of a per-step fold)
  long long stats_step_base = 0;
  bool pending = false;          // acc[(launch_index + 1) & 1] holds the last launch's accumulators, not yet folded into the master tables
  uint8_t* d_actions = nullptr;
  void* mdpk = nullptr;  // MdpK<T> in device memory
  long long n_simds = 1024;         // SIMDs of the device (4 per compute unit): create_impl
  int fair_prio = -1;               // option "fair_prio": -1 = when the context has more env waves than the device SIMDs, 0 / 1 = never / always (contexts that share a GPU)
  KalFix kal_fix{0.0, 0.0, false};  // fixed point of the Kalman covariance in this context's dtype (create_impl)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> kev;  // per-launch event pairs while the kernel timer is armed
  bool kernel_timer = false;
  long long timer_launches = 0;
  int sync_period = 1;
  bool windowed = false;
  int block = 0;  // 0 = auto
  int tick = 0;   // 0 = auto, 1 plain loop, 2 VGPR constants + grouped loop, 3 packed float32 tick, 4 literal constants (reference vehicle)
  bool lit_ok = false;  // float32 and the tick AND MDP constants are bit-identical to dql_refk.inc
  bool litm_ok = false;  // float32 and the MDP constants alone are: the packed layout then ends its periods on the literal table (TICK_PACKED_LITM)
  unsigned long long* elog = nullptr;  // episode log: [elog_cap][2][n_waves] ballots of finished / goal-reached episodes
  int elog_cap = 0, elog_n = 0;
  uint8_t* h_actions = nullptr; void* h_actions_dev = nullptr;  // pinned, device-visible staging of dql_step's host actions
  hipEvent_t ev_actions = nullptr; bool actions_in_flight = false, actions_zero_copy = false;
  void* h_out = nullptr; void* h_out_dev = nullptr;  // pinned, device-visible: StepOutRec[n] of dql_step_outputs, bad-action count, posted number
  unsigned out_seq = 0;
  uint8_t* d_mask = nullptr;     // reset mask staging (dql_reset), allocated on first use
  const uint8_t* ext_actions = nullptr;  // caller-owned device actions of the next external step (dql_step_dev), else d_actions
  long long window_launches = 0; // training launches whose accumulators the window holds (windowed mode)
  struct dql_comm* comm = nullptr;  // attached RCCL communicator (not owned)
  // one-shot peer-to-peer exchange (dql_p2p_*): this rank's exchange buffer (uncached, exported over HIP IPC), the peers' mapped
  // buffers, and the exchange counter every rank advances in lock-step
  int p2p_rank = -1, p2p_world = 0;
  unsigned long long* p2p_buf = nullptr;
  unsigned long long* p2p_peer[DQL_P2P_MAX_RANKS] = {nullptr};
  bool p2p_opened[DQL_P2P_MAX_RANKS] = {false};
  unsigned long long* p2p_status = nullptr;  // device verdict[2]: the last exchange every peer showed up for, the first exchange given up on (0 = none)
  unsigned long long p2p_seq = 0;
  bool p2p_pushed = false;  // a push is enqueued whose wait is not (dql_p2p_push_window / dql_p2p_wait_window)
  long long p2p_spin_limit = 60000000ll;  // option "p2p_spin_limit": a peer may be busy with a checkpoint or an evaluation for a while
  std::vector<hipEvent_t> sev;   // event pairs around the exchanges while the kernel timer is armed
  // population (dql_pop_*): n_agents > 0.  The context holds the K E envs (agent-major); each agent's tables, accumulators, statistics, level, seed
  // and launch history live in a context of its own (`agents`: no envs, the population's stream), so that every per-agent call is the
  // single-agent call on that agent's context
  int n_agents = 0;
  long long pop_E = 0;
  std::vector<dql_ctx*> agents;
  bool owns_stream = true;
  unsigned long long* pop_faults = nullptr;            // device [n_agents]: targets the step kernel's bounds guard dropped
  struct PopAgentDesc* pop_h = nullptr;                 // pinned staging ring of launch descriptors: [DQL_POP_RING][DQL_MAX_AGENTS]
  struct PopAgentDesc* pop_d = nullptr;                 // its device copy, read by k_step_pop
  hipEvent_t pop_ev[8] = {nullptr};                     // per ring slot: recorded behind the slot's copy (the staging slot is free again once it fired)
  bool pop_busy[8] = {false};
  int pop_slot = 0;
  int last_step[5] = {0, 0, 0, 0, 0};  // the step kernel the latest launch ran (dql_diag_step_instance): sizeof(T), BLOCK, TICK, XMODE, population
};
#define DQL_POP_RING 8

// first exchange of the peer-to-peer path that gave up on a missing peer (0 = none); synchronises the stream
static int p2p_failed_seq(dql_ctx* x, unsigned long long* seq_out) {
  *seq_out = 0;
  if (!x->p2p_status) return DQL_OK;
  unsigned long long v[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(v, x->p2p_status, sizeof(v), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  *seq_out = v[1];
  return DQL_OK;
}
static int check_config(const dql_config* c) {
  if (!c) return fail(DQL_EINVAL, "null config");
  if (c->working_curriculum_step < 0 || c->working_curriculum_step >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "working_curriculum_step must be in 0..4");
  if (c->dtype != DQL_F32 && c->dtype != DQL_F64) return fail(DQL_EINVAL, "dtype must be DQL_F32 or DQL_F64");
  if (c->pid_vz[2] != 0.0 || c->pid_yaw[2] != 0.0) return fail(DQL_EINVAL, "Kd != 0 is not supported by the fused kernel (reference launch files use Kd = 0)");
  if (c->manager_div < 1 || c->dt <= 0 || c->f_ag <= 0) return fail(DQL_EINVAL, "dt, f_ag, manager_div must be positive");
  // the per-period tick schedule travels packed in one kernel-argument word (StepArgs::sched): 8 bits each for the period's physics ticks and the manager divider
  if (c->manager_div > 255 || !(1.0 / (c->f_ag * c->dt) + 1.0 < 256.0)) return fail(DQL_EINVAL, "an agent period must hold fewer than 255 physics ticks (1 / (f_ag dt)) and manager_div must be <= 255");
  if (c->mass <= 0 || c->k_f <= 0 || c->k_m <= 0 || c->arm_length <= 0) return fail(DQL_EINVAL, "vehicle constants must be positive");
  if (c->init_uniform < 0 || c->init_uniform > 2) return fail(DQL_EINVAL, "init_uniform must be 0 (normal at level 0, else uniform), 1 (uniform) or 2 (SimulationLandingEnv placement)");
  if (c->dtype == DQL_F32) {
    // the float32 tick clamps the allocated w^2 at rotor_max^2 BEFORE the root (rotor_cmd: one med3 instead of a max before and a min after):
    // min(sqrt(x), omax) == sqrt(min(x, omax^2)) bit for bit only when omax^2 is a float32 (the reference's 838^2 = 702 244 is)
    const float om = (float)c->rotor_max; const double p2 = (double)om * (double)om;
    if (!(c->rotor_max > 0) || (double)(float)p2 != p2) return fail(DQL_EINVAL, "float32 contexts need a rotor_max whose square is exactly representable in float32 (the reference's 838 is); use dtype float64 for this vehicle");
  }
  // step_count and curriculum_check are packed into 16 bits each (store_env): an episode must time out before they wrap
  if (!(c->t_max > 0) || c->t_max * c->f_ag >= 65535.0) return fail(DQL_EINVAL, "t_max * f_ag must be in (0, 65535): the per-env step counters are 16 bits wide");
  return DQL_OK;
}

static int upload_mdpk(dql_ctx* x) {
  if (x->dtype == DQL_F32) { const MdpK<float> m = make_mdpk<float>(x->cfg); HIP_TRY(hipMemcpyAsync(x->mdpk, &m, sizeof(m), hipMemcpyHostToDevice, x->stream)); }
  else { const MdpK<double> m = make_mdpk<double>(x->cfg); HIP_TRY(hipMemcpyAsync(x->mdpk, &m, sizeof(m), hipMemcpyHostToDevice, x->stream)); }
  HIP_TRY(hipStreamSynchronize(x->stream));  // the source is a stack temporary
  return DQL_OK;
}
template <typename T> static int launch_init(dql_ctx* x) {
  InitArgs<T> a;
  a.c = make_simk<T>(x->cfg);
  a.sr = (Quad<T>*)x->sr; a.si = x->si; a.n = x->n; a.seed = x->seed; a.env_id_offset = x->env_id_offset;
  const dql_config& c = x->cfg;
  a.hover = std::sqrt((T)(c.mass * c.gravity / (4.0 * c.k_f)));
  a.vz_integ = (T)(c.mass * c.gravity / c.pid_vz[1]);
  a.r_lo = (T)c.mp_r_lo; a.r_hi = (T)c.mp_r_hi; a.t_lo = (T)c.mp_t_lo; a.t_hi = (T)c.mp_t_hi;
  const int B = 256;
  hipLaunchKernelGGL(k_init<T>, dim3((unsigned)((x->n + B - 1) / B)), dim3(B), 0, x->stream, a);
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}

static FoldK make_foldk(const dql_ctx* x, long long n_launch = 1) { return FoldK{x->alpha_tab, x->n_tab, x->cfg.alpha_min, x->cfg.fold_per_step, n_launch}; }
// the template arguments of the step kernel a launch runs, for dql_diag_step_instance (tests assert which instance the host picked)
static void note_step(dql_ctx* x, int bytes, int block, int tick, int xmode, int pop) {
  x->last_step[0] = bytes; x->last_step[1] = block; x->last_step[2] = tick; x->last_step[3] = xmode; x->last_step[4] = pop;
}
// a population launch: the active agents in slot order and their descriptors (already staged on the device)
struct PopLaunch { int n_active; int agent[DQL_MAX_AGENTS]; const PopAgentDesc* desc; };
template <typename T> static StepArgs<T> make_step_args(dql_ctx* x, int mode, double eps, int envs_per_block, int n_periods) {
  const long long j = x->step_index, l = x->launch_index;
  StepArgs<T> a;
  a.c = make_simk<T>(x->cfg, &x->kal_fix);
  a.mdp = (const MdpK<T> DQL_CONST_AS*)x->mdpk;
  a.mdp_run = MdpRun<T>{x->cfg.gamma, (T)(x->cfg.t_max * x->cfg.f_ag), x->cfg.goal_logic};
  a.sr = (Quad<T>*)x->sr; a.si = x->si;
  a.qa = x->tb[l & 1]; a.qb = x->tbb[l & 1]; a.acc_cur = (unsigned long long*)x->acc[l & 1];
  a.qa_m = x->qa; a.qb_m = x->qb; a.cnt_m = x->count; a.qa_pub = x->tb[(l + 1) & 1]; a.qb_pub = x->tbb[(l + 1) & 1];
  a.acc_prev = x->acc[(l + 1) & 1]; a.window = x->window;
  a.fold = make_foldk(x, x->pending_periods); a.stats = x->stats; a.actions = x->ext_actions ? x->ext_actions : x->d_actions;
  a.elog = x->elog ? x->elog + (size_t)x->elog_n * 2 * (size_t)((x->n + 63) >> 6) : nullptr;
  a.n = x->n; a.env_id_offset = x->env_id_offset; a.step_index = j;
  fill_schedule(x->cfg, j, a.mgr0, a.sched);
  a.seed = x->seed; a.eps_thr = eps_threshold(eps); a.pad_ = 0; a.mode = mode; a.n_periods = n_periods;
  a.env_blocks = (int)((x->n + envs_per_block - 1) / envs_per_block); a.have_prev = x->pending ? 1 : 0; a.windowed = x->windowed ? 1 : 0;
  a.fair_prio = x->fair_prio >= 0 ? x->fair_prio : (((x->n + 63) / 64 > x->n_simds) ? 1 : 0);
  return a;
}
template <typename T, int BLOCK, int TICK> static void launch_pop_t(dql_ctx* x, int mode, int n_periods, const PopLaunch& pl) {
  PopArgs<T> pa;
  pa.s = make_step_args<T>(x, mode, 0.0, BLOCK, n_periods);  // the shared part; per-agent members come from the descriptors
  const long long active_envs = (long long)pl.n_active * x->pop_E;
  pa.s.fair_prio = x->fair_prio >= 0 ? x->fair_prio : (((active_envs + 63) / 64 > x->n_simds) ? 1 : 0);
  pa.desc = (const PopAgentDesc DQL_CONST_AS*)pl.desc;
  pa.blocks_per_agent = (int)(x->pop_E / BLOCK);  // exact: E is a multiple of 512
  pa.writer_blocks = (DQL_N_CELLS + BLOCK - 1) / BLOCK;
  pa.n_active = pl.n_active; pa.pad_ = 0;
  for (int s = 0; s < DQL_MAX_AGENTS; ++s) pa.agent[s] = s < pl.n_active ? pl.agent[s] : 0;
  const dim3 grid((unsigned)(pl.n_active * (pa.blocks_per_agent + pa.writer_blocks))), block(BLOCK);
  if constexpr (sizeof(T) == 4 && TICK == TICK_PACKED_LITM) {
    note_step(x, sizeof(T), BLOCK, TICK, X_ONLY, 1); hipLaunchKernelGGL((k_step_pop<T, BLOCK, TICK, X_ONLY>), grid, block, 0, x->stream, pa);
  } else if constexpr (sizeof(T) == 4 && (TICK == TICK_LIT || tick_is_packed(TICK))) {
    if (x->cfg.two_axis) { note_step(x, sizeof(T), BLOCK, TICK, X_TWO, 1); hipLaunchKernelGGL((k_step_pop<T, BLOCK, TICK, X_TWO>), grid, block, 0, x->stream, pa); }
    else { note_step(x, sizeof(T), BLOCK, TICK, X_ONLY, 1); hipLaunchKernelGGL((k_step_pop<T, BLOCK, TICK, X_ONLY>), grid, block, 0, x->stream, pa); }
  } else { note_step(x, sizeof(T), BLOCK, TICK, X_RUNTIME, 1); hipLaunchKernelGGL((k_step_pop<T, BLOCK, TICK, X_RUNTIME>), grid, block, 0, x->stream, pa); }
}
template <typename T, int BLOCK, int TICK> static void launch_step_t(dql_ctx* x, int mode, double eps, int n_periods, const PopLaunch* pl) {
  if (pl) { launch_pop_t<T, BLOCK, TICK>(x, mode, n_periods, *pl); return; }
  const StepArgs<T> a = make_step_args<T>(x, mode, eps, BLOCK, n_periods);
  const int writer_blocks = (DQL_N_CELLS + BLOCK - 1) / BLOCK;
  const dim3 grid((unsigned)(a.env_blocks + writer_blocks)), block(BLOCK);
  // the layouts launch_step_b picks by itself come in an x-axis and a two-axis instance (agent_period's XMODE); the others decide at run time
  if constexpr (sizeof(T) == 4 && TICK == TICK_PACKED_LITM) {  // x-axis configs only (create_impl: litm_ok)
    note_step(x, sizeof(T), BLOCK, TICK, X_ONLY, 0); hipLaunchKernelGGL((k_step<T, BLOCK, TICK, X_ONLY>), grid, block, 0, x->stream, a);
  } else if constexpr (sizeof(T) == 4 && (TICK == TICK_LIT || tick_is_packed(TICK))) {
    if (x->cfg.two_axis) { note_step(x, sizeof(T), BLOCK, TICK, X_TWO, 0); hipLaunchKernelGGL((k_step<T, BLOCK, TICK, X_TWO>), grid, block, 0, x->stream, a); }
    else { note_step(x, sizeof(T), BLOCK, TICK, X_ONLY, 0); hipLaunchKernelGGL((k_step<T, BLOCK, TICK, X_ONLY>), grid, block, 0, x->stream, a); }
  } else { note_step(x, sizeof(T), BLOCK, TICK, X_RUNTIME, 0); hipLaunchKernelGGL((k_step<T, BLOCK, TICK, X_RUNTIME>), grid, block, 0, x->stream, a); }
}
// Which k_step variant serves a launch (options "block" and "tick"; 0 = auto).  Measured on MI355X, periods_per_launch 4
// (profiles/r2_sweep_tick.jsonl, r2_sweep_occupancy.jsonl):
//   block  64 (no LDS staging, one wave per workgroup) up to 8 192 envs; 256 (2 waves per SIMD) up to 196 608; 512 with the register
//          budget of 4 waves per SIMD beyond (float32: -3 % plain, -6 % with literal constants at 1 M envs; 229 376 envs: 59.6 vs
//          63.3 us, 196 608: 57.0 vs 52.8)
//   tick   packed float32 tick while a SIMD hosts at most one env wave (<= 65 536 envs: 18.7 vs 20.2 us at 4 096, 20.8 vs 22.3 at
//          32 768; beside a second wave a packed instruction costs two issue slots and the layout LOSES: 45 vs 36 us at 131 072);
//          literal constants beyond 65 536 envs when the vehicle is the reference's (round 2 took them with the 512-thread block only; with 16
//          periods per launch and the round-3 fixes they also win at 256: 98 304 envs 26.2 us, 131 072 28.4 vs 30.6 plain, 262 144 / 512: 51.6
//          vs 58.8); the plain loop otherwise.
//          (2, round 1's small-batch layout — VGPR constants + grouped loop without the packing — is gone: the packed tick replaced it)
// float64 has one layout (no packed f64 pipe to use, no 64-bit literals): plain.
// (a population launch chooses by the population's whole batch, K E envs: the layout a context of that size would fly)
template <typename T> static void launch_step_b(dql_ctx* x, int mode, double eps, int np, const PopLaunch* pl = nullptr) {
  int block = x->block, tick = x->tick;
  if constexpr (sizeof(T) == 8) {
    if (block == 0) block = (x->n <= 8192) ? 64 : 256;
    if (block == 64) launch_step_t<T, 64, TICK_PLAIN>(x, mode, eps, np, pl);
    else if (block == 128) launch_step_t<T, 128, TICK_PLAIN>(x, mode, eps, np, pl);
    else launch_step_t<T, 256, TICK_PLAIN>(x, mode, eps, np, pl);
  } else {
    if (block == 0) block = (x->n <= 8192) ? 64 : (x->n <= 196608 || tick == 3 ? 256 : 512);
    if (tick == 0) tick = x->n <= 65536 ? 3 : (x->lit_ok ? 4 : 1);  // round 3: literals win from two waves per SIMD on (131 072 envs, P = 16: 28.4 vs 30.6 us)
    if (tick == 4 && !x->lit_ok) tick = 1;
    if (block == 128 || (block == 512 && tick != 4)) tick = 1;
    if (tick == 4) {
      if (block == 64) launch_step_t<T, 64, TICK_LIT>(x, mode, eps, np, pl); else if (block == 512) launch_step_t<T, 512, TICK_LIT>(x, mode, eps, np, pl);
      else launch_step_t<T, 256, TICK_LIT>(x, mode, eps, np, pl);
    } else if (block == 512) launch_step_t<T, 512, TICK_PLAIN>(x, mode, eps, np, pl);
    else if (block == 128) launch_step_t<T, 128, TICK_PLAIN>(x, mode, eps, np, pl);
    else if (block == 64) {
      if (tick == 3 && x->litm_ok) launch_step_t<T, 64, TICK_PACKED_LITM>(x, mode, eps, np, pl); else if (tick == 3) launch_step_t<T, 64, TICK_PACKED>(x, mode, eps, np, pl); else launch_step_t<T, 64, TICK_PLAIN>(x, mode, eps, np, pl);
    } else {
      if (tick == 3 && x->litm_ok) launch_step_t<T, 256, TICK_PACKED_LITM>(x, mode, eps, np, pl); else if (tick == 3) launch_step_t<T, 256, TICK_PACKED>(x, mode, eps, np, pl); else launch_step_t<T, 256, TICK_PLAIN>(x, mode, eps, np, pl);
    }
  }
}
// ONE kernel per launch of n_periods (1 .. periods_per_launch) agent periods
static int launch_period(dql_ctx* x, int mode, double eps, int n_periods = 1) {
  if (x->elog && x->elog_n + n_periods > x->elog_cap) return fail(DQL_ESTATE, "episode log full: read it with dql_episode_log_read before stepping on");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (x->kernel_timer) {  // the pair belongs to the context from its creation on (dql_diag_kernel_timer / dql_destroy free it), whatever fails below
    HIP_TRY(hipEventCreate(&e0)); x->kev.push_back(e0);
    if (hipEventCreate(&e1) != hipSuccess) { x->kev.pop_back(); (void)hipEventDestroy(e0); return fail(DQL_EHIP, "hipEventCreate failed"); }
    x->kev.push_back(e1);
    HIP_TRY(hipEventRecord(e0, x->stream));
  }
  if (x->dtype == DQL_F32) launch_step_b<float>(x, mode, eps, n_periods); else launch_step_b<double>(x, mode, eps, n_periods);
  if (x->kernel_timer) HIP_TRY(hipEventRecord(e1, x->stream));
  HIP_TRY(hipGetLastError());
  if (x->elog) x->elog_n += n_periods;
  x->pending = (mode == MODE_TRAIN);  // this launch's accumulators wait for the next launch's writer blocks (or a flush)
  x->pending_periods = n_periods;
  if (x->windowed && mode == MODE_TRAIN) x->window_launches += n_periods;  // counted in agent periods
  x->step_index += n_periods;
  x->launch_index += 1;
  x->timer_launches += 1;
  return DQL_OK;
}
// ONE population launch of n_periods agent periods for the active agents (active null = all): every active agent's launch arguments come from
// ITS history (step index, launch parity, pending fold, level, seed, eps, episode-log row), exactly as launch_period builds them for a context of its own
static int launch_pop(dql_ctx* x, int mode, const double* eps, const uint8_t* active, int n_periods) {
  PopLaunch pl;
  pl.n_active = 0;
  for (int k = 0; k < x->n_agents; ++k) if (!active || active[k]) pl.agent[pl.n_active++] = k;
  if (!pl.n_active) return DQL_OK;
  for (int s = 0; s < pl.n_active; ++s)
    if (x->elog && x->agents[pl.agent[s]]->elog_n + n_periods > x->elog_cap) return fail(DQL_ESTATE, "episode log full: read it with dql_episode_log_read before stepping on");
  // staging: a pinned ring slot is rewritten only after the copy that last read it has run
  const int slot = x->pop_slot;
  x->pop_slot = (slot + 1) % DQL_POP_RING;
  if (x->pop_busy[slot]) { HIP_TRY(hipEventSynchronize(x->pop_ev[slot])); x->pop_busy[slot] = false; }
  PopAgentDesc* h = x->pop_h + (size_t)slot * DQL_MAX_AGENTS;
  const size_t nw = (size_t)((x->n + 63) >> 6);
  for (int s = 0; s < pl.n_active; ++s) {
    const int k = pl.agent[s];
    const dql_ctx* g = x->agents[k];
    const long long j = g->step_index, l = g->launch_index;
    PopAgentDesc& d = h[s];
    memset(&d, 0, sizeof(d));
    d.qa = g->tb[l & 1]; d.qb = g->tbb[l & 1]; d.acc_cur = (unsigned long long*)g->acc[l & 1];
    d.qa_m = g->qa; d.qb_m = g->qb; d.cnt_m = g->count; d.qa_pub = g->tb[(l + 1) & 1]; d.qb_pub = g->tbb[(l + 1) & 1];
    d.acc_prev = g->acc[(l + 1) & 1]; d.window = g->window;
    d.stats = g->stats; d.mdp = (const char DQL_CONST_AS*)g->mdpk;
    d.elog = x->elog ? x->elog + (size_t)g->elog_n * 2 * nw : nullptr;
    d.faults = x->pop_faults + k;
    d.fold = make_foldk(g, g->pending_periods);
    d.step_index = j; d.seed = g->seed;
    fill_schedule(g->cfg, j, d.mgr0, d.sched);
    d.eps_thr = mode == MODE_TRAIN ? eps_threshold(eps[k]) : 0u;
    d.have_prev = g->pending ? 1 : 0; d.working = g->cfg.working_curriculum_step;
  }
  PopAgentDesc* dd = x->pop_d + (size_t)slot * DQL_MAX_AGENTS;
  HIP_TRY(hipMemcpyAsync(dd, h, (size_t)pl.n_active * sizeof(PopAgentDesc), hipMemcpyHostToDevice, x->stream));
  HIP_TRY(hipEventRecord(x->pop_ev[slot], x->stream));
  x->pop_busy[slot] = true;
  pl.desc = dd;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (x->kernel_timer) {
    HIP_TRY(hipEventCreate(&e0)); x->kev.push_back(e0);
    if (hipEventCreate(&e1) != hipSuccess) { x->kev.pop_back(); (void)hipEventDestroy(e0); return fail(DQL_EHIP, "hipEventCreate failed"); }
    x->kev.push_back(e1);
    HIP_TRY(hipEventRecord(e0, x->stream));
  }
  if (x->dtype == DQL_F32) launch_step_b<float>(x, mode, 0.0, n_periods, &pl); else launch_step_b<double>(x, mode, 0.0, n_periods, &pl);
  if (x->kernel_timer) HIP_TRY(hipEventRecord(e1, x->stream));
  HIP_TRY(hipGetLastError());
  int elog_n = 0;
  for (int s = 0; s < pl.n_active; ++s) {  // what launch_period does to a context of its own
    dql_ctx* g = x->agents[pl.agent[s]];
    if (x->elog) g->elog_n += n_periods;
    g->pending = (mode == MODE_TRAIN);
    g->pending_periods = n_periods;
    g->step_index += n_periods;
    g->launch_index += 1;
  }
  for (dql_ctx* g : x->agents) elog_n = g->elog_n > elog_n ? g->elog_n : elog_n;
  x->elog_n = elog_n;
  x->timer_launches += 1;
  return DQL_OK;
}
// fold the last launch's accumulators into the master tables now
static int flush_pending(dql_ctx* x) {
  if (!x->pending) return DQL_OK;
  FlushArgs f{x->qa, x->qb, x->count, x->acc[(x->launch_index + 1) & 1], x->window, make_foldk(x, x->pending_periods), x->windowed ? 1 : 0};
  hipLaunchKernelGGL(k_flush, dim3((DQL_N_CELLS + 255) / 256), dim3(256), 0, x->stream, f);
  HIP_TRY(hipGetLastError());
  x->pending = false;
  return DQL_OK;
}
// master -> both acting buffers (after the host or a transfer rewrote the master tables)
static int publish_master(dql_ctx* x) {
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(hipMemcpyAsync(x->tb[k], x->qa, DQL_N_CELLS * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
    HIP_TRY(hipMemcpyAsync(x->tbb[k], x->qb, DQL_N_CELLS * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
  }
  return DQL_OK;
}

// ---- typed host<->device copies (templates: C++ linkage) ----
template <typename T> static int fetch_quads(dql_ctx* x, int q0, int nq, std::vector<T>& h) {
  h.resize((size_t)nq * (size_t)x->n * 4);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemcpyAsync(h.data(), (const char*)x->sr + (size_t)q0 * (size_t)x->n * 4 * sizeof(T), h.size() * sizeof(T), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
template <typename T> static int get_sim_state_t(dql_ctx* x, double* out) {
  std::vector<T> h; int rc = fetch_quads<T>(x, 0, NQ_REAL, h); if (rc) return rc;
  const long long n = x->n;
  for (int f = 0; f < NF_REAL; ++f) { const int q = f / 4, k = f % 4; for (long long i = 0; i < n; ++i) out[(long long)f * n + i] = (double)h[((size_t)q * n + i) * 4 + k]; }
  return DQL_OK;
}
template <typename T> static int set_sim_state_t(dql_ctx* x, const double* in) {
  const long long n = x->n;
  std::vector<T> h((size_t)NQ_REAL * n * 4);
  for (int f = 0; f < NF_REAL; ++f) { const int q = f / 4, k = f % 4; for (long long i = 0; i < n; ++i) h[((size_t)q * n + i) * 4 + k] = (T)in[(long long)f * n + i]; }
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemcpyAsync(x->sr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
template <typename T> static int get_rewards_t(dql_ctx* x, double* out) {
  std::vector<T> h; int rc = fetch_quads<T>(x, 14, 1, h); if (rc) return rc;
  for (long long i = 0; i < x->n; ++i) out[i] = (double)h[(size_t)i * 4];
  return DQL_OK;
}
template <typename T> static int get_obs_t(dql_ctx* x, double* out) {
  std::vector<T> h; int rc = fetch_quads<T>(x, 14, 2, h); if (rc) return rc;
  const long long n = x->n;
  for (long long i = 0; i < n; ++i) {
    const T* a = &h[(size_t)i * 4]; const T* b = &h[((size_t)n + i) * 4];
    out[0 * n + i] = a[1]; out[1 * n + i] = b[0]; out[2 * n + i] = a[2]; out[3 * n + i] = b[1]; out[4 * n + i] = a[3]; out[5 * n + i] = b[2];
  }
  return DQL_OK;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// on a population context (dql_pop_create) the single-agent calls act on agent 0 when it is the only one and are refused otherwise; external actions
// and the multi-GPU exchanges are refused on every population
static int pop_refused(const char* call, const char* instead) {
  return fail(DQL_EINVAL, std::string(call) + " acts on one agent: on a population context with several agents use " + instead);
}
#define POP_SINGLE(x, call, instead, fwd) do { if ((x) && (x)->n_agents > 1) return pop_refused(call, instead); if ((x) && (x)->n_agents == 1) return (fwd); } while (0)
#define POP_NEVER(x, call) do { if ((x) && (x)->n_agents) return fail(DQL_EINVAL, std::string(call) + " is not available on a population context (external actions and the multi-GPU exchanges are single-agent only)"); } while (0)
extern "C" {

int dql_abi_version(void) { return DQL_ABI_VERSION; }
const char* dql_last_error(void) { return g_err.c_str(); }
int dql_device_count(int* count) {
  if (!count) return fail(DQL_EINVAL, "null pointer");
  HIP_TRY(hipGetDeviceCount(count));
  return DQL_OK;
}

int dql_config_default(dql_config* c) {
  if (!c) return fail(DQL_EINVAL, "null config");
  memset(c, 0, sizeof(*c));
  c->working_curriculum_step = 0; c->two_axis = 0; c->quirks = DQL_Q_REFERENCE; c->dtype = DQL_F32;
  c->f_ag = 22.92; c->t_max = 20.0; c->p_max = 4.5; c->v_max = 3.39411; c->a_max = 1.28;
  c->theta_max = 21.37723 * (M_PI / 180.0); c->delta_theta = 7.12574 * (M_PI / 180.0); c->beta = 1.0 / 3; c->sigma_a = 0.416; c->minimum_altitude = 0.2;
  c->w_p = -100.0; c->w_v = -10.0; c->w_theta = -1.55; c->w_dur = -6.0; c->w_fail = -2.6; c->w_succ = 2.6;
  const double lp[5] = {1.0, 0.64, 0.4096, 0.262144, 0.16777216}, lv[5] = {1.0, 0.8, 0.64, 0.512, 0.4096};
  for (int i = 0; i < 5; ++i) { c->lim_p[i] = lp[i]; c->lim_v[i] = lv[i]; c->lim_a[i] = 1.0; }
  c->vz_setpoint = -0.1; c->yaw_setpoint = 0.0;
  c->gamma = 0.99; c->alpha_min = 0.02949; c->alpha_omega = 0.51;
  c->dt = 0.002; c->manager_div = 5; c->trajectory = DQL_TRAJ_RPM; c->gravity = 9.8; c->mass = 0.68 + 4 * 0.009 + 1e-5;
  {
    const double m_r = 0.009, l = 0.17, h = 0.01, mb = m_r * 10.0;
    const double ixx_r = 0.0833333 * mb * (0.015 * 0.015 + 0.003 * 0.003), iyy_r = 0.0833333 * mb * (0.1 * 0.1 + 0.003 * 0.003);
    const double izz_r = 0.0833333 * mb * (0.1 * 0.1 + 0.015 * 0.015), inplane = 0.5 * (ixx_r + iyy_r);
    c->inertia[0] = c->inertia[1] = 0.007 + 2 * m_r * (l * l + h * h) + 2 * m_r * h * h + 4 * inplane;
    c->inertia[2] = 0.012 + 4 * m_r * l * l + 4 * izz_r;
  }
  c->arm_length = 0.17; c->rotor_z = 0.01; c->k_f = 8.54858e-06; c->k_m = 0.016;
  c->rotor_alpha_up = std::exp(-0.002 / 0.0125); c->rotor_alpha_down = std::exp(-0.002 / 0.025); c->rotor_max = 838.0;
  c->c_drag = 8.06428e-05; c->c_roll = 1e-06;
  c->k_R[0] = 0.7; c->k_R[1] = 0.7; c->k_R[2] = 0.035; c->k_W[0] = 0.1; c->k_W[1] = 0.1; c->k_W[2] = 0.025;
  const double pv[6] = {5.0, 10.0, 0.0, 0.0, 10.0, 10.0}, py[6] = {8.0, 1.0, 0.0, -3.141592, 3.141592, 5.0};
  for (int i = 0; i < 6; ++i) { c->pid_vz[i] = pv[i]; c->pid_yaw[i] = py[i]; }
  c->bw_c = 1.0; c->mp_r_x = 2.0; c->mp_t_x = 1.6; c->mp_dt = 0.01; c->mp_top_z = 0.455; c->mp_half_x = 0.55; c->mp_half_y = 0.55; c->drone_bottom = 0.06;
  c->z_init = 4.0; c->init_sigma = 4.5 / 3; c->init_uniform = 0; c->per_env_platform = 0; c->goal_logic = 1; c->fold_per_step = 0;
  c->mp_r_lo = 1.0; c->mp_r_hi = 3.0; c->mp_t_lo = 0.8; c->mp_t_hi = 1.6;
  c->noise_pos_sd = 0.0; c->noise_vel_sd = 0.0; c->kalman_q = 1e-4;
  return DQL_OK;
}

static int create_tables(dql_ctx* x);
// allocation + initialisation of a fresh context; any failure leaves a partly built context for the caller to destroy
static int create_impl(dql_ctx* x, const dql_config* cfg) {
#define ALLOC(ptr, bytes) do { hipError_t _e = hipMalloc((void**)&(ptr), (bytes)); if (_e != hipSuccess) return fail(DQL_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(_e)); } while (0)
  HIP_TRY(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&x->ev0)); HIP_TRY(hipEventCreate(&x->ev1));
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, x->device) == hipSuccess && cus > 0) x->n_simds = 4ll * cus; }
  if (cfg->dtype == DQL_F32) { const SimK<float> k = make_simk<float>(*cfg); x->kal_fix = KalFix{(double)k.kal_pss, (double)k.kal_kss, true}; }
  else { const SimK<double> k = make_simk<double>(*cfg); x->kal_fix = KalFix{k.kal_pss, k.kal_kss, true}; }
  const bool refm = cfg->dtype == DQL_F32 && refm_matches(make_mdpk<float>(*cfg));
  x->lit_ok = refm && refk_matches(make_simk<float>(*cfg, &x->kal_fix));
  // x-axis configs only: the two-axis instance of this layout (k_step<float, *, TICK_PACKED_LITM, X_TWO>) faults on its first launch (a memory access the
  // source does not explain — same source as the two instances it combines, both of which are parity-green); it is never selected
  x->litm_ok = refm && !cfg->two_axis;
  ALLOC(x->sr, (size_t)NQ_REAL * (size_t)x->n * 4 * x->real_size);
  ALLOC(x->si, (size_t)x->n * sizeof(int4));
  ALLOC(x->d_actions, (size_t)x->n);
  HIP_TRY(hipMemsetAsync(x->sr, 0, (size_t)NQ_REAL * (size_t)x->n * 4 * x->real_size, x->stream));
  HIP_TRY(hipMemsetAsync(x->d_actions, 2, (size_t)x->n, x->stream));
  int rc = create_tables(x);
  if (rc) return rc;
  rc = (x->dtype == DQL_F32) ? launch_init<float>(x) : launch_init<double>(x);
  if (rc) return rc;
  // default alpha table (plateau only): callers install the reference schedule with dql_set_alpha_table
  const double a0 = cfg->alpha_min;
  return dql_set_alpha_table(x, &a0, 1);
#undef ALLOC
}
// what a context needs besides its envs: tables, ping-pong copies, accumulators, window, statistics, MdpK (also the agents of a population)
static int create_tables(dql_ctx* x) {
#define ALLOC(ptr, bytes) do { hipError_t _e = hipMalloc((void**)&(ptr), (bytes)); if (_e != hipSuccess) return fail(DQL_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(_e)); } while (0)
  ALLOC(x->qa, DQL_N_CELLS * sizeof(double)); ALLOC(x->qb, DQL_N_CELLS * sizeof(double)); ALLOC(x->count, DQL_N_CELLS * sizeof(double));
  ALLOC(x->qa_base, DQL_N_CELLS * sizeof(double)); ALLOC(x->count_base, DQL_N_CELLS * sizeof(double));
  ALLOC(x->qb_base, DQL_N_CELLS * sizeof(double));
  for (int k = 0; k < 2; ++k) { ALLOC(x->tb[k], DQL_N_CELLS * sizeof(double)); ALLOC(x->tbb[k], DQL_N_CELLS * sizeof(double)); ALLOC(x->acc[k], DQL_ACC_LEN * sizeof(long long)); }
  ALLOC(x->window_own, DQL_ACC_LEN * sizeof(long long)); x->window = x->window_own;
  ALLOC(x->stats, sizeof(StatsDev)); ALLOC(x->mdpk, sizeof(MdpK<double>));
#undef ALLOC
  HIP_TRY(hipMemsetAsync(x->qa, 0, DQL_N_CELLS * sizeof(double), x->stream)); HIP_TRY(hipMemsetAsync(x->qb, 0, DQL_N_CELLS * sizeof(double), x->stream));
  HIP_TRY(hipMemsetAsync(x->count, 0, DQL_N_CELLS * sizeof(double), x->stream));
  HIP_TRY(hipMemsetAsync(x->qa_base, 0, DQL_N_CELLS * sizeof(double), x->stream)); HIP_TRY(hipMemsetAsync(x->count_base, 0, DQL_N_CELLS * sizeof(double), x->stream));
  HIP_TRY(hipMemsetAsync(x->qb_base, 0, DQL_N_CELLS * sizeof(double), x->stream));
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(hipMemsetAsync(x->tb[k], 0, DQL_N_CELLS * sizeof(double), x->stream)); HIP_TRY(hipMemsetAsync(x->tbb[k], 0, DQL_N_CELLS * sizeof(double), x->stream));
    HIP_TRY(hipMemsetAsync(x->acc[k], 0, DQL_ACC_LEN * sizeof(long long), x->stream));
  }
  HIP_TRY(hipMemsetAsync(x->window, 0, DQL_ACC_LEN * sizeof(long long), x->stream));
  HIP_TRY(hipMemsetAsync(x->stats, 0, sizeof(StatsDev), x->stream));
  return upload_mdpk(x);
}

int dql_create(const dql_config* cfg, int device, int64_t n_envs, uint64_t seed, int64_t env_id_offset, dql_ctx** out) {
  if (!out) return fail(DQL_EINVAL, "null out pointer");
  *out = nullptr;
  int rc = check_config(cfg);
  if (rc) return rc;
  if (n_envs < 1 || n_envs > (1ll << 31)) return fail(DQL_EINVAL, "n_envs must be in 1..2^31");
  if (env_id_offset < 0 || env_id_offset + n_envs > (1ll << 32)) return fail(DQL_EINVAL, "global env ids (env_id_offset .. env_id_offset + n_envs) must fit 32 bits: they key the per-env RNG");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(DQL_EHIP, "no HIP device visible: libdql_hip needs an MI355X (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(DQL_EINVAL, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  dql_ctx* x = new dql_ctx();
  x->cfg = *cfg; x->device = device; x->n = n_envs; x->seed = seed; x->env_id_offset = env_id_offset; x->dtype = cfg->dtype;
  x->real_size = cfg->dtype == DQL_F32 ? 4 : 8;
  rc = create_impl(x, cfg);
  if (rc) {
    const std::string why = g_err;  // dql_destroy must not lose the reason
    dql_destroy(x);
    return fail(rc, why);
  }
  *out = x;
  return DQL_OK;
}

int dql_destroy(dql_ctx* x) {
  if (!x) return DQL_OK;
  (void)hipSetDevice(x->device);
  if (x->stream) (void)hipStreamSynchronize(x->stream);
  for (dql_ctx* g : x->agents) (void)dql_destroy(g);
  for (int s = 0; s < DQL_POP_RING; ++s) if (x->pop_ev[s]) (void)hipEventDestroy(x->pop_ev[s]);
  if (x->pop_h) (void)hipHostFree(x->pop_h);
  if (x->pop_d) (void)hipFree(x->pop_d);
  if (x->pop_faults) (void)hipFree(x->pop_faults);
  for (hipEvent_t e : x->kev) (void)hipEventDestroy(e);
  for (hipEvent_t e : x->sev) (void)hipEventDestroy(e);
  for (int r = 0; r < DQL_P2P_MAX_RANKS; ++r) if (x->p2p_opened[r] && x->p2p_peer[r]) (void)hipIpcCloseMemHandle(x->p2p_peer[r]);
  void* ptrs[] = {x->sr, x->si, x->qa, x->qb, x->count, x->tb[0], x->tb[1], x->tbb[0], x->tbb[1], x->qa_base, x->qb_base, x->count_base, x->acc[0], x->acc[1], x->window_own, x->alpha_tab, x->stats, x->d_actions, x->mdpk, x->elog, x->d_mask, x->p2p_buf, x->p2p_status};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (x->h_actions) (void)hipHostFree(x->h_actions);
  if (x->h_out) (void)hipHostFree(x->h_out);
  if (x->ev_actions) (void)hipEventDestroy(x->ev_actions);
  if (x->ev0) (void)hipEventDestroy(x->ev0);
  if (x->ev1) (void)hipEventDestroy(x->ev1);
  if (x->stream && x->owns_stream) (void)hipStreamDestroy(x->stream);
  delete x;
  return DQL_OK;
}

// Host wait for the context's stream: poll first (a blocking hipStreamSynchronize parks the thread and wakes it 20-40 us after the
// GPU is done, which is most of a short run), block only when the work is long
static hipError_t wait_stream(hipStream_t st) {
  for (int i = 0; i < 20000; ++i) {  // ~ a few ms of polling at most
    const hipError_t e = hipStreamQuery(st);
    if (e != hipErrorNotReady) return e;
  }
  return hipStreamSynchronize(st);
}
// Completion of a single-workgroup kernel as seen through coherent pinned memory: its last act is a system-scope release store of the
// call's sequence number next to its results.  Seeing the number is enough to read them — several microseconds before the stream reports
// the kernel complete (end-of-kernel cache maintenance, completion signal, the runtime's bookkeeping), which is what a caller stepping ONE
// env pays per call.  Bounded: false -> the caller falls back to the stream.
static bool wait_posted(const unsigned* flag, unsigned seq) {
  for (int i = 0; i < 400000; ++i) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return true;
    __builtin_ia32_pause();
  }
  return false;
}
int dql_sync(dql_ctx* x) { CHECK_CTX(x); HIP_TRY(hipSetDevice(x->device)); HIP_TRY(wait_stream(x->stream)); return DQL_OK; }
int dql_n_envs(dql_ctx* x, int64_t* n) { CHECK_CTX(x); if (!n) return fail(DQL_EINVAL, "null pointer"); *n = x->n; return DQL_OK; }
int dql_state_bytes_per_env(dql_ctx* x, int64_t* bytes) {
  CHECK_CTX(x);
  if (!bytes) return fail(DQL_EINVAL, "null pointer");
  // x-axis: quads 0-10 read + written, quads 14-15 written, int4 read + written; two-axis: + quads 11-12
  const int rw = x->cfg.two_axis ? 13 : 11;
  *bytes = (int64_t)((rw + rw + 2) * 4 * x->real_size + 2 * sizeof(int4));
  return DQL_OK;
}

int dql_set_alpha_table(dql_ctx* x, const double* alpha, int32_t n) {
  CHECK_CTX(x);
  if (!alpha || n < 1) return fail(DQL_EINVAL, "alpha table must have at least one entry");
  if (alpha[n - 1] != x->cfg.alpha_min) return fail(DQL_EINVAL, "alpha table must end on the alpha_min plateau");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(x->stream));
  if (x->alpha_tab) HIP_TRY(hipFree(x->alpha_tab));
  x->alpha_tab = nullptr;
  HIP_TRY(hipMalloc((void**)&x->alpha_tab, (size_t)n * sizeof(double)));
  HIP_TRY(hipMemcpy(x->alpha_tab, alpha, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  x->n_tab = n;
  for (dql_ctx* g : x->agents) { int rc = dql_set_alpha_table(g, alpha, n); if (rc) return rc; }  // population: every agent
  return DQL_OK;
}

int dql_set_curriculum(dql_ctx* x, int32_t k) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_set_curriculum", "dql_pop_set_curriculum", dql_pop_set_curriculum(x, 0, k));
  if (k < 0 || k >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "curriculum step must be in 0..4");
  HIP_TRY(hipSetDevice(x->device));
  int rc = flush_pending(x);
  if (rc) return rc;
  rc = publish_master(x);  // the new level starts acting on everything learnt so far
  if (rc) return rc;
  x->cfg.working_curriculum_step = k;
  rc = upload_mdpk(x);
  if (rc) return rc;
  return dql_reset(x, nullptr);
}

int dql_reset(dql_ctx* x, const uint8_t* mask) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  const uint8_t* dmask = nullptr;
  if (mask) {
    if (!x->d_mask && hipMalloc((void**)&x->d_mask, (size_t)x->n) != hipSuccess) { x->d_mask = nullptr; return fail(DQL_ENOMEM, "hipMalloc(reset mask) failed"); }
    HIP_TRY(hipMemcpyAsync(x->d_mask, mask, (size_t)x->n, hipMemcpyHostToDevice, x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));  // the caller's buffer may be reused right after return
    dmask = x->d_mask;
  }
  hipLaunchKernelGGL(k_mark_reset, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, x->stream, x->si, dmask, (long long)x->n);
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}

int dql_step(dql_ctx* x, const uint8_t* actions) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_step");
  if (!actions) return fail(DQL_EINVAL, "actions must not be null (use dql_train_steps / dql_eval_steps for on-device action selection)");
  HIP_TRY(hipSetDevice(x->device));
  // staged through pinned memory: the caller's buffer is free on return and nobody waits — except for the PREVIOUS step's read of the
  // same staging buffer, which has long happened by the time a caller comes back with new actions.  Up to DQL_ZERO_COPY_ENVS envs the
  // step kernel reads the staging buffer itself (one byte per lane over PCIe: no copy-engine command in front of the kernel — at one env
  // that command costs more than the kernel); larger batches are copied to the device asynchronously first.
  if (!x->h_actions) {
    if (hipHostMalloc((void**)&x->h_actions, (size_t)x->n, hipHostMallocMapped) != hipSuccess) { x->h_actions = nullptr; return fail(DQL_ENOMEM, "hipHostMalloc(action staging) failed"); }
    HIP_TRY(hipHostGetDevicePointer(&x->h_actions_dev, x->h_actions, 0));
    HIP_TRY(hipEventCreateWithFlags(&x->ev_actions, hipEventDisableTiming));
  }
  if (x->actions_in_flight) {
    if (x->actions_zero_copy) HIP_TRY(wait_stream(x->stream));  // the kernel that reads the buffer (dql_step_outputs has normally waited for it already)
    else HIP_TRY(hipEventSynchronize(x->ev_actions));
    x->actions_in_flight = false;
  }
  x->actions_zero_copy = x->n <= DQL_ZERO_COPY_ENVS;
  if (x->actions_zero_copy) {
    // small batches (the single-env drop-in path among them): the bytes are being touched anyway, so the action codes are checked HERE and a bad
    // one is refused before anything is flown — the reject-before-mutation contract of the old host loop.  Larger batches are checked by the
    // step kernel (per env, StatsDev::bad_actions) and reported by the next dql_step_outputs / dql_stats_get: see include/dql.h.
    const bool two = x->cfg.two_axis != 0;
    for (long long i = 0; i < x->n; ++i) {
      const unsigned a = actions[i], ax = a & 3u, ay = (a >> 2) & 3u;
      if (ax > 2u || ay > 2u || (a >> 4) || (!two && ay != 0u && ay != 2u))
        return fail(DQL_EINVAL, "action " + std::to_string(a) + " of env " + std::to_string(i) + " is out of range: ax | ay << 2 with ax, ay in 0 (increase), 1 (decrease), 2 (hold); ay only in two_axis configs");
      x->h_actions[i] = (uint8_t)a;
    }
  } else memcpy(x->h_actions, actions, (size_t)x->n);
  if (x->actions_zero_copy) {
    x->ext_actions = (const uint8_t*)x->h_actions_dev;
  } else {
    HIP_TRY(hipMemcpyAsync(x->d_actions, x->h_actions, (size_t)x->n, hipMemcpyHostToDevice, x->stream));
    HIP_TRY(hipEventRecord(x->ev_actions, x->stream));
    x->ext_actions = nullptr;
  }
  x->actions_in_flight = true;
  const int rc = launch_period(x, MODE_EXTERNAL, 0.0);  // the kernel checks the action codes (StatsDev::bad_actions)
  x->ext_actions = nullptr;
  return rc;
}
// out-of-range external actions seen by the step kernel since the last report: reported ONCE (the counter is cleared)
static int report_bad_actions(dql_ctx* x, unsigned long long bad) {
  if (!bad) return DQL_OK;
  HIP_TRY(hipMemsetAsync((char*)x->stats + offsetof(StatsDev, bad_actions), 0, sizeof(unsigned long long), x->stream));
  return fail(DQL_EINVAL, std::to_string(bad) + " action(s) out of range were flown as 'hold': ax | ay << 2 with ax, ay in 0..2 (ay only in two_axis configs)");
}
int dql_step_outputs(dql_ctx* x, int32_t* idx_x, int32_t* idx_y, double* reward, uint8_t* done, int8_t* code, int32_t* step_count, double* cum, uint8_t* was_reset) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  const size_t n = (size_t)x->n;
  if (!x->h_out) {
    if (hipHostMalloc(&x->h_out, n * sizeof(StepOutRec) + 2 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { x->h_out = nullptr; return fail(DQL_ENOMEM, "hipHostMalloc(step outputs) failed"); }
    HIP_TRY(hipHostGetDevicePointer(&x->h_out_dev, x->h_out, 0));
    memset((char*)x->h_out + n * sizeof(StepOutRec), 0, 2 * sizeof(unsigned long long));
  }
  const unsigned grid = (unsigned)((n + 255) / 256);
  unsigned long long* bad_h = (unsigned long long*)((char*)x->h_out + n * sizeof(StepOutRec));
  unsigned long long* bad_d = (unsigned long long*)((char*)x->h_out_dev + n * sizeof(StepOutRec));
  const unsigned long long* bad_src = (const unsigned long long*)((const char*)x->stats + offsetof(StatsDev, bad_actions));
  const unsigned seq = ++x->out_seq;
  unsigned* posted_d = grid == 1 ? (unsigned*)(bad_d + 1) : nullptr;
  if (x->dtype == DQL_F32) hipLaunchKernelGGL(k_step_outputs<float>, dim3(grid), dim3(256), 0, x->stream, (const Quad<float>*)x->sr, (const int4*)x->si, (long long)n, (StepOutRec*)x->h_out_dev, bad_src, bad_d, posted_d, seq);
  else hipLaunchKernelGGL(k_step_outputs<double>, dim3(grid), dim3(256), 0, x->stream, (const Quad<double>*)x->sr, (const int4*)x->si, (long long)n, (StepOutRec*)x->h_out_dev, bad_src, bad_d, posted_d, seq);
  HIP_TRY(hipGetLastError());
  if (!(posted_d && wait_posted((const unsigned*)(bad_h + 1), seq))) HIP_TRY(wait_stream(x->stream));
  if (x->actions_zero_copy) x->actions_in_flight = false;  // the kernel that read the staged actions has run
  const StepOutRec* r = (const StepOutRec*)x->h_out;
  for (size_t i = 0; i < n; ++i) {
    const int fl = (r[i].code_flags >> 8) & 0xff;
    if (idx_x) idx_x[i] = r[i].idx_x;
    if (idx_y) idx_y[i] = r[i].idx_y;
    if (reward) reward[i] = r[i].reward;
    if (done) done[i] = (fl & FL_DONE) ? 1 : 0;
    if (code) code[i] = (int8_t)(r[i].code_flags & 0xff);
    if (step_count) step_count[i] = r[i].step_count;
    if (cum) cum[i] = r[i].cum;
    if (was_reset) was_reset[i] = (fl & FL_WAS_RESET) ? 1 : 0;
  }
  return report_bad_actions(x, *bad_h);
}
int dql_step_dev(dql_ctx* x, const uint8_t* dev_actions) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_step_dev");
  if (!dev_actions) return fail(DQL_EINVAL, "dev_actions must not be null");
  HIP_TRY(hipSetDevice(x->device));
  x->ext_actions = dev_actions;
  const int rc = launch_period(x, MODE_EXTERNAL, 0.0);
  x->ext_actions = nullptr;
  return rc;
}
int dql_train_steps(dql_ctx* x, int32_t n_steps, double eps) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_train_steps", "dql_pop_train_steps", dql_pop_train_steps(x, n_steps, &eps, nullptr));
  if (n_steps < 0) return fail(DQL_EINVAL, "n_steps must be >= 0");
  HIP_TRY(hipSetDevice(x->device));
  for (int i = 0; i < n_steps;) {
    const int np = n_steps - i < x->periods_per_launch ? n_steps - i : x->periods_per_launch;
    int rc = launch_period(x, MODE_TRAIN, eps, np); if (rc) return rc;
    i += np;
  }
  return DQL_OK;
}
int dql_eval_steps(dql_ctx* x, int32_t n_steps) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_eval_steps", "dql_pop_eval_steps", dql_pop_eval_steps(x, n_steps, nullptr));
  if (n_steps < 0) return fail(DQL_EINVAL, "n_steps must be >= 0");
  HIP_TRY(hipSetDevice(x->device));
  for (int i = 0; i < n_steps;) {
    const int np = n_steps - i < x->periods_per_launch ? n_steps - i : x->periods_per_launch;
    int rc = launch_period(x, MODE_EVAL, 0.0, np); if (rc) return rc;
    i += np;
  }
  return DQL_OK;
}

// ---- getters ----
static int fetch_ints(dql_ctx* x, std::vector<int4>& h) {
  h.resize((size_t)x->n);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemcpyAsync(h.data(), x->si, (size_t)x->n * sizeof(int4), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
int dql_get_states(dql_ctx* x, int32_t* idx_x, int32_t* idx_y) {
  CHECK_CTX(x);
  std::vector<int4> h; int rc = fetch_ints(x, h); if (rc) return rc;
  for (long long i = 0; i < x->n; ++i) { if (idx_x) idx_x[i] = h[i].x; if (idx_y) idx_y[i] = h[i].y; }
  return DQL_OK;
}
int dql_get_dones(dql_ctx* x, uint8_t* dones, int8_t* codes) {
  CHECK_CTX(x);
  std::vector<int4> h; int rc = fetch_ints(x, h); if (rc) return rc;
  for (long long i = 0; i < x->n; ++i) { if (dones) dones[i] = ((h[i].w >> 8) & FL_DONE) ? 1 : 0; if (codes) codes[i] = (int8_t)(h[i].w & 0xff); }
  return DQL_OK;
}
int dql_get_actions(dql_ctx* x, uint8_t* actions) {
  CHECK_CTX(x);
  std::vector<int4> h; int rc = fetch_ints(x, h); if (rc) return rc;
  for (long long i = 0; i < x->n; ++i) actions[i] = (uint8_t)((h[i].w >> 16) & 0xff);
  return DQL_OK;
}
int dql_get_sim_state(dql_ctx* x, double* out, int32_t cap) {
  CHECK_CTX(x);
  if (!out || cap < NF_REAL) return fail(DQL_EINVAL, "out buffer must hold 64 fields x n_envs doubles");
  return x->dtype == DQL_F32 ? get_sim_state_t<float>(x, out) : get_sim_state_t<double>(x, out);
}
static int real_field_index(const char* name);  // (the name table sits further down, with dql_field_name)
int dql_set_sim_state(dql_ctx* x, const double* in, int32_t nf) {
  CHECK_CTX(x);
  if (!in || nf != NF_REAL) return fail(DQL_EINVAL, "in buffer must hold exactly 64 fields x n_envs doubles");
  if (x->dtype == DQL_F32 && !x->cfg.two_axis) {  // the x-axis float32 kernels fly attitude()'s closed form for roll_sp == 0 and never read the field
    const int f_roll = real_field_index("roll_sp");
    for (long long i = 0; f_roll >= 0 && i < x->n; ++i)
      if (in[(long long)f_roll * x->n + i] != 0.0) return fail(DQL_EINVAL, "roll_sp must be 0 in an x-axis float32 context (its attitude law is the closed form for a zero roll set-point); use two_axis = 1 or dtype float64");
  }
  return x->dtype == DQL_F32 ? set_sim_state_t<float>(x, in) : set_sim_state_t<double>(x, in);
}
int dql_get_sim_ints(dql_ctx* x, int32_t* out, int32_t cap) {
  CHECK_CTX(x);
  if (!out || cap < NF_INT) return fail(DQL_EINVAL, "out buffer must hold 7 fields x n_envs int32");
  std::vector<int4> h; int rc = fetch_ints(x, h); if (rc) return rc;
  const long long n = x->n;
  for (long long i = 0; i < n; ++i) {
    out[0 * n + i] = h[i].x; out[1 * n + i] = h[i].y; out[2 * n + i] = h[i].z & 0xffff; out[3 * n + i] = (h[i].z >> 16) & 0xffff;
    out[4 * n + i] = h[i].w & 0xff; out[5 * n + i] = (h[i].w >> 8) & 0xff; out[6 * n + i] = (h[i].w >> 16) & 0xff;
  }
  return DQL_OK;
}
int dql_set_sim_ints(dql_ctx* x, const int32_t* in, int32_t nf) {
  CHECK_CTX(x);
  if (!in || nf != NF_INT) return fail(DQL_EINVAL, "in buffer must hold exactly 7 fields x n_envs int32");
  const long long n = x->n;
  const int n_states = DQL_N_CELLS / DQL_N_ACTIONS;
  for (long long i = 0; i < n; ++i)  // the state indices address the tables on the device: -1 (no state yet) .. 944
    if (in[i] < -1 || in[i] >= n_states || in[n + i] < -1 || in[n + i] >= n_states) return fail(DQL_EINVAL, "idx_x / idx_y out of range (-1 .. 944)");
  for (long long i = 0; i < n; ++i) {  // code indexes the terminal histogram; the packed counters are 16 bits, the action two 2-bit fields
    const int32_t sc = in[2 * n + i], cc = in[3 * n + i], code = in[4 * n + i], fl = in[5 * n + i], act = in[6 * n + i];
    if (code < 0 || code >= DQL_N_CHECK_CODES) return fail(DQL_EINVAL, "code out of range (0 .. 8)");
    if (sc < 0 || sc > 0xffff || cc < 0 || cc > 0xffff || fl < 0 || fl > 0xff) return fail(DQL_EINVAL, "step_count / cur_check / flags out of range");
    if (act < 0 || (act & 3) > 2 || ((act >> 2) & 3) > 2 || (act >> 4)) return fail(DQL_EINVAL, "action out of range (ax | ay << 2, ax, ay in 0..2)");
  }
  std::vector<int4> h((size_t)n);
  for (long long i = 0; i < n; ++i)
    h[i] = make_int4(in[0 * n + i], in[1 * n + i], (in[2 * n + i] & 0xffff) | (in[3 * n + i] << 16),
                     (in[4 * n + i] & 0xff) | ((in[5 * n + i] & 0xff) << 8) | ((in[6 * n + i] & 0xff) << 16));
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemcpyAsync(x->si, h.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
static const char* const k_real_names[NF_REAL] = {
    "px", "py", "pz", "vx", "vy", "vz", "qw", "qx", "qy", "qz", "wx", "wy", "wz", "om0", "om1", "om2",
    "om3", "vz_i", "vz_x1", "vz_x2", "vz_y1", "vz_y2", "vz_y3", "vz_state",
    "yw_i", "yw_x1", "yw_x2", "yw_y1", "yw_y2", "yw_y3", "yw_state", "pitch_sp",
    "mp_phase", "mp_x", "mp_u", "vf_x", "kal_x_x", "kal_x_P", "shp_x_p", "shp_x_v",
    "shp_x_a", "cum_x", "roll_sp", "mp_y", "mp_v", "vf_y", "kal_y_x", "kal_y_P",
    "shp_y_p", "shp_y_v", "shp_y_a", "cum_y", "mp_r", "mp_w", "pad0", "pad1",
    "reward", "obs_p_x", "obs_v_x", "obs_a_x", "obs_p_y", "obs_v_y", "obs_a_y", "pad2"};
static const char* const k_int_names[NF_INT] = {"idx_x", "idx_y", "step_count", "cur_check", "code", "flags", "action"};
static int real_field_index(const char* name) {
  for (int f = 0; f < NF_REAL; ++f) if (!strcmp(k_real_names[f], name)) return f;
  return -1;
}
int dql_n_fields(int32_t* n_real, int32_t* n_int) { if (n_real) *n_real = NF_REAL; if (n_int) *n_int = NF_INT; return DQL_OK; }
const char* dql_field_name(int32_t i, int32_t is_int) {
  if (is_int) return (i >= 0 && i < NF_INT) ? k_int_names[i] : nullptr;
  return (i >= 0 && i < NF_REAL) ? k_real_names[i] : nullptr;
}
int dql_get_rewards(dql_ctx* x, double* rewards) {
  CHECK_CTX(x);
  if (!rewards) return fail(DQL_EINVAL, "null pointer");
  return x->dtype == DQL_F32 ? get_rewards_t<float>(x, rewards) : get_rewards_t<double>(x, rewards);
}
int dql_get_obs(dql_ctx* x, double* out) {
  CHECK_CTX(x);
  if (!out) return fail(DQL_EINVAL, "null pointer");
  return x->dtype == DQL_F32 ? get_obs_t<float>(x, out) : get_obs_t<double>(x, out);
}

// ---- tables ----
int dql_flush(dql_ctx* x) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  for (dql_ctx* g : x->agents) { int rc = flush_pending(g); if (rc) return rc; }  // population: every agent
  return flush_pending(x);
}
int dql_get_tables(dql_ctx* x, double* qa, double* qb, double* count) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_get_tables", "dql_pop_get_tables", dql_pop_get_tables(x, 0, qa, qb, count));
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  const size_t B = DQL_N_CELLS * sizeof(double);
  if (qa) HIP_TRY(hipMemcpyAsync(qa, x->qa, B, hipMemcpyDeviceToHost, x->stream));
  if (qb) HIP_TRY(hipMemcpyAsync(qb, x->qb, B, hipMemcpyDeviceToHost, x->stream));
  if (count) HIP_TRY(hipMemcpyAsync(count, x->count, B, hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
int dql_set_tables(dql_ctx* x, const double* qa, const double* qb, const double* count) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_set_tables", "dql_pop_set_tables", dql_pop_set_tables(x, 0, qa, qb, count));
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  const size_t B = DQL_N_CELLS * sizeof(double);
  if (qa) { HIP_TRY(hipMemcpyAsync(x->qa, qa, B, hipMemcpyHostToDevice, x->stream)); HIP_TRY(hipMemcpyAsync(x->qa_base, qa, B, hipMemcpyHostToDevice, x->stream)); }
  if (qb) { HIP_TRY(hipMemcpyAsync(x->qb, qb, B, hipMemcpyHostToDevice, x->stream)); HIP_TRY(hipMemcpyAsync(x->qb_base, qb, B, hipMemcpyHostToDevice, x->stream)); }
  if (count) { HIP_TRY(hipMemcpyAsync(x->count, count, B, hipMemcpyHostToDevice, x->stream)); HIP_TRY(hipMemcpyAsync(x->count_base, count, B, hipMemcpyHostToDevice, x->stream)); }
  if (qa || qb) { int rc = publish_master(x); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
int dql_transfer(dql_ctx* x, int32_t k, double ratio) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_transfer", "dql_pop_transfer", dql_pop_transfer(x, 0, k, ratio));
  if (k < 0 || k >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "curriculum step must be in 0..4");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  const int src = (k - 1 + DQL_MAX_LEVELS) % DQL_MAX_LEVELS;  // k = 0 wraps to the last level (B6)
  hipLaunchKernelGGL(k_transfer, dim3((DQL_CELLS_PER_LEVEL + 255) / 256), dim3(256), 0, x->stream, x->qa, x->qb, k, src, ratio);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(x->qa_base, x->qa, DQL_N_CELLS * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
  HIP_TRY(hipMemcpyAsync(x->qb_base, x->qb, DQL_N_CELLS * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
  return publish_master(x);
}

// ---- multi-GPU exchange ----
int dql_set_sync_period(dql_ctx* x, int32_t k) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_set_sync_period");
  if (k < 1) return fail(DQL_EINVAL, "sync period must be >= 1");
  x->sync_period = k;
  return DQL_OK;
}
int dql_set_windowed(dql_ctx* x, int32_t on) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_set_windowed");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  if (on && !x->windowed) {
    HIP_TRY(hipMemcpyAsync(x->qa_base, x->qa, DQL_N_CELLS * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
    HIP_TRY(hipMemcpyAsync(x->qb_base, x->qb, DQL_N_CELLS * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
    HIP_TRY(hipMemcpyAsync(x->count_base, x->count, DQL_N_CELLS * sizeof(double), hipMemcpyDeviceToDevice, x->stream));
    HIP_TRY(hipMemsetAsync(x->window, 0, DQL_ACC_LEN * sizeof(long long), x->stream));
    x->window_launches = 0;
  }
  x->windowed = on != 0;
  return DQL_OK;
}
int dql_diag_accum_dev_ptr(dql_ctx* x, void** dev_ptr, int64_t* n_int64) {
  CHECK_CTX(x);
  if (dev_ptr) *dev_ptr = x->window;
  if (n_int64) *n_int64 = DQL_ACC_LEN;
  return DQL_OK;
}
int dql_set_window_buffer(dql_ctx* x, void* dev_ptr) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_set_window_buffer");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(x->stream));
  x->window = dev_ptr ? (long long*)dev_ptr : x->window_own;
  HIP_TRY(hipMemsetAsync(x->window, 0, DQL_ACC_LEN * sizeof(long long), x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
int dql_stream_handle(dql_ctx* x, void** s) { CHECK_CTX(x); if (s) *s = (void*)x->stream; return DQL_OK; }
int dql_apply_accum(dql_ctx* x) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_apply_accum");
  if (!x->windowed) return fail(DQL_ESTATE, "dql_apply_accum needs windowed accumulation (dql_set_windowed)");
  if (x->pending) return fail(DQL_ESTATE, "dql_apply_accum: call dql_flush before reducing the window (the last launch is not in it yet)");
  HIP_TRY(hipSetDevice(x->device));
  WindowArgs a{x->qa_base, x->qb_base, x->count_base, x->qa, x->qb, x->count, x->tb[0], x->tb[1], x->tbb[0], x->tbb[1], x->window,
               make_foldk(x, x->window_launches > 0 ? x->window_launches : 1)};
  hipLaunchKernelGGL(k_apply_window, dim3((DQL_N_CELLS + 255) / 256), dim3(256), 0, x->stream, a);
  HIP_TRY(hipGetLastError());
  x->window_launches = 0;
  if (x->kernel_timer && (x->sev.size() & 1)) {  // closes the pair dql_allreduce_window opened
    hipEvent_t e1 = nullptr;
    HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e1, x->stream)); x->sev.push_back(e1);
  }
  return DQL_OK;
}
int dql_get_accum(dql_ctx* x, int64_t* out) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_get_accum");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  HIP_TRY(hipMemcpyAsync(out, x->window, DQL_ACC_LEN * sizeof(long long), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}
int dql_set_accum(dql_ctx* x, const int64_t* in) {
  CHECK_CTX(x);
  POP_NEVER(x, "dql_set_accum");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemcpyAsync(x->window, in, DQL_ACC_LEN * sizeof(long long), hipMemcpyHostToDevice, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}

int dql_get_step_index(dql_ctx* x, int64_t* step_index) { CHECK_CTX(x); POP_SINGLE(x, "dql_get_step_index", "dql_pop_get_step_index", dql_pop_get_step_index(x, 0, step_index)); if (!step_index) return fail(DQL_EINVAL, "null pointer"); *step_index = x->step_index; return DQL_OK; }
int dql_set_step_index(dql_ctx* x, int64_t step_index) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_set_step_index", "dql_pop_set_step_index", dql_pop_set_step_index(x, 0, step_index));
  if (step_index < 0) return fail(DQL_EINVAL, "step_index must be >= 0");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  // the ping-pong buffers follow the parity of launch_index (a launch may cover several periods): republish, so that whichever buffer
  // the next launch reads holds the same (master) tables
  { int rc = publish_master(x); if (rc) return rc; }
  x->stats_step_base += step_index - x->step_index;  // agent_steps since the last stats reset stays what it was
  x->step_index = step_index;
  return DQL_OK;
}
int dql_publish_tables(dql_ctx* x) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_publish_tables", "dql_pop_publish_tables", dql_pop_publish_tables(x, 0));
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }
  return publish_master(x);
}

// ---- stats / timing / knobs ----
int dql_stats_get(dql_ctx* x, dql_stats* out) {
  CHECK_CTX(x);
  POP_SINGLE(x, "dql_stats_get", "dql_pop_stats_get", dql_pop_stats_get(x, 0, out));
  if (!out) return fail(DQL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(x->device));
  StatsDev s;
  HIP_TRY(hipMemcpyAsync(&s, x->stats, sizeof(s), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  out->agent_steps = (int64_t)(x->step_index - x->stats_step_base); out->decisions = (int64_t)s.decisions; out->episodes = (int64_t)s.episodes;
  for (int k = 0; k < DQL_N_CHECK_CODES; ++k) out->by_code[k] = (int64_t)s.by_code[k];
  out->reward_sum = (double)s.reward_fx / (double)(1ll << DQL_TARGET_FRAC_BITS);
  out->physics_ticks = ticks_before(x->cfg, x->step_index);
  { int rc = report_bad_actions(x, s.bad_actions); if (rc) return rc; }
  if (x->p2p_status) {  // the training loop's per-chunk synchronisation point: a table exchange that gave up on a peer ends the run here
    unsigned long long bad = 0;
    { int rc = p2p_failed_seq(x, &bad); if (rc) return rc; }
    if (bad) return fail(DQL_EPEER, "peer-to-peer table exchange " + std::to_string(bad) + " of rank " + std::to_string(x->p2p_rank) + " gave up waiting for a peer (option p2p_spin_limit): its window was not summed, the table replicas differ from here on");
  }
  return DQL_OK;
}
int dql_stats_reset(dql_ctx* x) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemsetAsync(x->stats, 0, sizeof(StatsDev), x->stream));
  x->stats_step_base = x->step_index;
  for (dql_ctx* g : x->agents) { int rc = dql_stats_reset(g); if (rc) return rc; }  // population: every agent
  return DQL_OK;
}
int dql_diag_timer_start(dql_ctx* x) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  x->timer_launches = 0;
  HIP_TRY(hipEventRecord(x->ev0, x->stream));
  return DQL_OK;
}
int dql_diag_timer_stop(dql_ctx* x, double* ms) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipEventRecord(x->ev1, x->stream));
  HIP_TRY(wait_stream(x->stream));
  float f = 0;
  HIP_TRY(hipEventElapsedTime(&f, x->ev0, x->ev1));
  if (ms) *ms = (double)f;
  return DQL_OK;
}
int dql_diag_kernel_timer(dql_ctx* x, int32_t on) {
  CHECK_CTX(x);
  for (hipEvent_t e : x->kev) (void)hipEventDestroy(e);
  x->kev.clear();
  for (hipEvent_t e : x->sev) (void)hipEventDestroy(e);
  x->sev.clear();
  x->kernel_timer = on != 0;
  return DQL_OK;
}
int dql_diag_kernel_time_ms(dql_ctx* x, double* avg_ms, int64_t* launches) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->stream));
  double tot = 0; int64_t n = 0;
  for (size_t i = 0; i + 1 < x->kev.size(); i += 2) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, x->kev[i], x->kev[i + 1])); tot += f; ++n; }
  if (avg_ms) *avg_ms = n ? tot / (double)n : 0.0;
  if (launches) *launches = n;
  return DQL_OK;
}
int dql_diag_step_instance(dql_ctx* x, int32_t* out5) {
  CHECK_CTX(x);
  if (!out5) return fail(DQL_EINVAL, "null pointer");
  for (int k = 0; k < 5; ++k) out5[k] = x->last_step[k];
  return DQL_OK;
}
int dql_diag_delay(dql_ctx* x, double microseconds) {
  CHECK_CTX(x);
  if (!(microseconds >= 0.0) || microseconds > 1e5) return fail(DQL_EINVAL, "delay must be in 0 .. 100 000 us");
  HIP_TRY(hipSetDevice(x->device));
  hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, x->stream, (unsigned long long)(microseconds * 100.0));
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}
int dql_diag_sync_time_ms(dql_ctx* x, double* avg_ms, int64_t* syncs) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->stream));
  double tot = 0; int64_t n = 0;
  for (size_t i = 0; i + 1 < x->sev.size(); i += 2) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, x->sev[i], x->sev[i + 1])); tot += f; ++n; }
  if (avg_ms) *avg_ms = n ? tot / (double)n : 0.0;
  if (syncs) *syncs = n;
  return DQL_OK;
}
int dql_set_option(dql_ctx* x, const char* name, int32_t value) {
  CHECK_CTX(x);
  if (!name) return fail(DQL_EINVAL, "null option name");
  if (!strcmp(name, "periods_per_launch")) {
    if (value < 1 || value > DQL_MAX_PERIODS) return fail(DQL_EINVAL, "periods_per_launch must be in 1..32");
    x->periods_per_launch = value;
    return DQL_OK;
  }
  if (!strcmp(name, "tick")) {
    if (value < 0 || value > 4 || value == 2) return fail(DQL_EINVAL, "tick must be 0 (auto), 1 (plain), 3 (packed float32) or 4 (literal constants)");
    if (value == 4 && !x->lit_ok) return fail(DQL_EINVAL, "tick 4 serves float32 contexts whose vehicle / controller / MDP constants are the reference's (tools/gen_refk.py); this context's differ");
    x->tick = value;
    return DQL_OK;
  }
  if (!strcmp(name, "fair_prio")) {
    if (value < -1 || value > 1) return fail(DQL_EINVAL, "fair_prio must be -1 (automatic), 0 or 1");
    x->fair_prio = value;
    return DQL_OK;
  }
  if (!strcmp(name, "p2p_spin_limit")) {
    if (value < 1000) return fail(DQL_EINVAL, "p2p_spin_limit must be at least 1000 polls");
    x->p2p_spin_limit = value;
    return DQL_OK;
  }
  if (!strcmp(name, "block")) {
    if (value != 0 && value != 64 && value != 128 && value != 256 && value != 512) return fail(DQL_EINVAL, "block must be 0, 64, 128, 256 or 512");
    if (value == 512 && x->dtype != DQL_F32) return fail(DQL_EINVAL, "block 512 serves float32 contexts");
    x->block = value;
    return DQL_OK;
  }
  return fail(DQL_EINVAL, std::string("unknown option ") + name);
}

// ---- episode log: which envs finished an episode in each agent period, and which of those reached the goal state ----
// population: every agent's rows restart at the top, and the rows read so far are cleared (an agent that runs fewer periods than another leaves its words 0)
static int pop_log_consumed(dql_ctx* x) {
  if (!x->n_agents) return DQL_OK;
  for (dql_ctx* g : x->agents) g->elog_n = 0;
  if (x->elog_n) HIP_TRY(hipMemsetAsync(x->elog, 0, (size_t)x->elog_n * 2 * (size_t)((x->n + 63) >> 6) * sizeof(unsigned long long), x->stream));
  return DQL_OK;
}
int dql_episode_log_enable(dql_ctx* x, int32_t capacity_periods) {
  CHECK_CTX(x);
  if (capacity_periods < 0) return fail(DQL_EINVAL, "capacity_periods must be >= 0");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->stream));
  if (x->elog) { HIP_TRY(hipFree(x->elog)); x->elog = nullptr; }
  x->elog_cap = 0; x->elog_n = 0;
  for (dql_ctx* g : x->agents) g->elog_n = 0;
  if (capacity_periods == 0) return DQL_OK;
  const size_t nw = (size_t)((x->n + 63) >> 6);
  if (hipMalloc((void**)&x->elog, (size_t)capacity_periods * 2 * nw * sizeof(unsigned long long)) != hipSuccess) { x->elog = nullptr; return fail(DQL_ENOMEM, "hipMalloc(episode log) failed"); }
  x->elog_cap = capacity_periods;
  if (x->n_agents) HIP_TRY(hipMemsetAsync(x->elog, 0, (size_t)capacity_periods * 2 * nw * sizeof(unsigned long long), x->stream));  // words of agents that ran fewer periods read 0
  return DQL_OK;
}
int dql_episode_log_read(dql_ctx* x, uint64_t* done_masks, uint64_t* goal_masks, int32_t max_periods, int32_t* n_periods) {
  CHECK_CTX(x);
  if (!x->elog) return fail(DQL_ESTATE, "episode log is not enabled (dql_episode_log_enable)");
  if (!n_periods) return fail(DQL_EINVAL, "n_periods must not be null");
  if (x->elog_n > max_periods || (x->elog_n && (!done_masks || !goal_masks))) return fail(DQL_EINVAL, "output buffers hold fewer periods than were logged");
  const size_t nw = (size_t)((x->n + 63) >> 6);
  HIP_TRY(hipSetDevice(x->device));
  if (x->elog_n) {
    std::vector<unsigned long long> h((size_t)x->elog_n * 2 * nw);
    HIP_TRY(hipMemcpyAsync(h.data(), x->elog, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));
    for (int p = 0; p < x->elog_n; ++p) {
      memcpy(done_masks + (size_t)p * nw, &h[(size_t)p * 2 * nw], nw * sizeof(uint64_t));
      memcpy(goal_masks + (size_t)p * nw, &h[(size_t)p * 2 * nw + nw], nw * sizeof(uint64_t));
    }
  }
  *n_periods = x->elog_n;
  { int rc = pop_log_consumed(x); if (rc) return rc; }
  x->elog_n = 0;
  return DQL_OK;
}

// the same for the first n_words 64-env words of every period only (the promotion rule judges the first few global env ids: 1 KB per chunk
// instead of 16 B per env)
int dql_episode_log_read_words(dql_ctx* x, uint64_t* done_masks, uint64_t* goal_masks, int32_t max_periods, int32_t n_words, int32_t* n_periods) {
  CHECK_CTX(x);
  if (!x->elog) return fail(DQL_ESTATE, "episode log is not enabled (dql_episode_log_enable)");
  if (!n_periods) return fail(DQL_EINVAL, "n_periods must not be null");
  const size_t nw = (size_t)((x->n + 63) >> 6);
  if (n_words < 0 || (size_t)n_words > nw) return fail(DQL_EINVAL, "n_words must be in 0 .. ceil(n_envs / 64)");
  if (x->elog_n > max_periods || (x->elog_n && n_words && (!done_masks || !goal_masks))) return fail(DQL_EINVAL, "output buffers hold fewer periods than were logged");
  HIP_TRY(hipSetDevice(x->device));
  if (x->elog_n && n_words) {
    const size_t k = (size_t)n_words, rows = (size_t)x->elog_n * 2;  // device rows: [period][done | goal][nw]
    std::vector<unsigned long long> h(rows * k);
    HIP_TRY(hipMemcpy2DAsync(h.data(), k * sizeof(unsigned long long), x->elog, nw * sizeof(unsigned long long), k * sizeof(unsigned long long), rows, hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(hipStreamSynchronize(x->stream));
    for (int p = 0; p < x->elog_n; ++p) {
      memcpy(done_masks + (size_t)p * k, &h[(size_t)p * 2 * k], k * sizeof(uint64_t));
      memcpy(goal_masks + (size_t)p * k, &h[(size_t)p * 2 * k + k], k * sizeof(uint64_t));
    }
  }
  *n_periods = x->elog_n;
  { int rc = pop_log_consumed(x); if (rc) return rc; }
  x->elog_n = 0;
  return DQL_OK;
}

// ---- stateless operators ----
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t b) { hipError_t e = hipMalloc(&p, b ? b : 1); return e == hipSuccess ? 0 : -1; }
};
#define OP_PROLOGUE(device)                                                                \
  int _ndev = 0;                                                                           \
  HIP_TRY(hipGetDeviceCount(&_ndev));                                                      \
  if (_ndev < 1) return fail(DQL_EHIP, "no HIP device visible (there is no CPU fallback)"); \
  if ((device) < 0 || (device) >= _ndev) return fail(DQL_EINVAL, "device index out of range"); \
  HIP_TRY(hipSetDevice(device));
#define UP(buf, host, bytes) do { if ((buf).alloc(bytes)) return fail(DQL_ENOMEM, "hipMalloc failed"); HIP_TRY(hipMemcpy((buf).p, (host), (bytes), hipMemcpyHostToDevice)); } while (0)

int dql_discretise(const dql_config* cfg, int device, const double* rel_p, const double* rel_v, const double* rel_a, const double* angle, int64_t n, int32_t* idx_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!rel_p || !rel_v || !rel_a || !angle || !idx_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf p, v, a, t, o;
  const size_t B = (size_t)n * sizeof(double);
  UP(p, rel_p, B); UP(v, rel_v, B); UP(a, rel_a, B); UP(t, angle, B);
  if (o.alloc((size_t)n * sizeof(int))) return fail(DQL_ENOMEM, "hipMalloc failed");
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_discretise<float>, dim3(grid), dim3(256), 0, 0, make_mdpk<float>(*cfg), (const double*)p.p, (const double*)v.p, (const double*)a.p, (const double*)t.p, (long long)n, (int*)o.p);
  else hipLaunchKernelGGL(k_discretise<double>, dim3(grid), dim3(256), 0, 0, make_mdpk<double>(*cfg), (const double*)p.p, (const double*)v.p, (const double*)a.p, (const double*)t.p, (long long)n, (int*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(idx_out, o.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_mdp_transition(const dql_config* cfg, int device, int64_t n, uint32_t stages, const uint8_t* action, const double* obs, double* mdp_state,
                       const int32_t* prev_idx, int32_t* idx_io, double* reward_out, uint8_t* done_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!action || !obs || !mdp_state || !prev_idx || !idx_io || !reward_out || !done_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  if ((stages & DQL_MDP_ALL) == 0) return fail(DQL_EINVAL, "no stage selected");
  for (int64_t i = 0; i < n; ++i) if (action[i] > 2) return fail(DQL_EINVAL, "action must be 0, 1 or 2");
  if ((stages & (DQL_MDP_CHECK | DQL_MDP_REWARD)) && !(stages & DQL_MDP_DISCRETISE))
    for (int64_t i = 0; i < n; ++i) if (idx_io[i] < 0 || idx_io[i] >= DQL_N_STATES) return fail(DQL_ESTATE, "Cannot check an empty state: call discrete_state first");
  OP_PROLOGUE(device)
  DevBuf a, o, ms, pi, io, ro, dn;
  UP(a, action, (size_t)n); UP(o, obs, (size_t)n * 7 * sizeof(double)); UP(ms, mdp_state, (size_t)n * 8 * sizeof(double)); UP(pi, prev_idx, (size_t)n * sizeof(int));
  UP(io, idx_io, (size_t)n * sizeof(int)); UP(ro, reward_out, (size_t)n * sizeof(double)); UP(dn, done_out, (size_t)n);
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_mdp_transition<float>, dim3(grid), dim3(256), 0, 0, make_mdpk<float>(*cfg), (long long)n, stages, (const uint8_t*)a.p, (const double*)o.p, (double*)ms.p, (const int*)pi.p, (int*)io.p, (double*)ro.p, (uint8_t*)dn.p);
  else hipLaunchKernelGGL(k_mdp_transition<double>, dim3(grid), dim3(256), 0, 0, make_mdpk<double>(*cfg), (long long)n, stages, (const uint8_t*)a.p, (const double*)o.p, (double*)ms.p, (const int*)pi.p, (int*)io.p, (double*)ro.p, (uint8_t*)dn.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(mdp_state, ms.p, (size_t)n * 8 * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(idx_io, io.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(reward_out, ro.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(done_out, dn.p, (size_t)n, hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_manager_run(const dql_config* cfg, int device, int64_t n_series, int64_t n_ticks, const double* in, const uint8_t* contact, uint64_t seed, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n_series < 0 || n_ticks < 0 || ((n_series > 0 && n_ticks > 0) && (!in || !contact || !out))) return fail(DQL_EINVAL, "null array");
  if (n_series == 0 || n_ticks == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  const size_t cells = (size_t)n_series * (size_t)n_ticks;
  UP(a, in, cells * 14 * sizeof(double)); UP(b, contact, cells);
  if (o.alloc(cells * 12 * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  dql_config c2 = *cfg;
  c2.two_axis = 1;  // the reference's estimator always runs on every axis; x-axis training configs simply never read y
  const unsigned grid = (unsigned)((n_series + 63) / 64);
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_manager_run<float>, dim3(grid), dim3(64), 0, 0, make_simk<float>(c2), (long long)n_series, (long long)n_ticks, (const double*)a.p, (const uint8_t*)b.p, (unsigned long long)seed, (double*)o.p);
  else hipLaunchKernelGGL(k_manager_run<double>, dim3(grid), dim3(64), 0, 0, make_simk<double>(c2), (long long)n_series, (long long)n_ticks, (const double*)a.p, (const uint8_t*)b.p, (unsigned long long)seed, (double*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, o.p, cells * 12 * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_plant_run(const dql_config* cfg, int device, int64_t n_series, int64_t n_ticks, const double* init, const double* rotor_cmd, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n_series < 0 || n_ticks < 0 || ((n_series > 0 && n_ticks > 0) && (!init || !rotor_cmd || !out))) return fail(DQL_EINVAL, "null array");
  if (n_series == 0 || n_ticks == 0) return DQL_OK;
  const size_t cells = (size_t)n_series * (size_t)n_ticks;
  for (size_t k = 0; k < cells * 4; ++k) if (!(rotor_cmd[k] >= 0.0)) return fail(DQL_EINVAL, "rotor commands must be >= 0 (the attitude law commands sqrt(max(w^2, 0)))");
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  UP(a, init, (size_t)n_series * 21 * sizeof(double)); UP(b, rotor_cmd, cells * 4 * sizeof(double));
  if (o.alloc(cells * 20 * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  const unsigned grid = (unsigned)((n_series + 63) / 64);
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_plant_run<float>, dim3(grid), dim3(64), 0, 0, make_simk<float>(*cfg), (long long)n_series, (long long)n_ticks, (const double*)a.p, (const double*)b.p, (double*)o.p);
  else hipLaunchKernelGGL(k_plant_run<double>, dim3(grid), dim3(64), 0, 0, make_simk<double>(*cfg), (long long)n_series, (long long)n_ticks, (const double*)a.p, (const double*)b.p, (double*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, o.p, cells * 20 * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_butterworth_run(const dql_config* cfg, int device, const double* x, int64_t n, double* y_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!x || !y_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, o;
  UP(a, x, (size_t)n * sizeof(double));
  if (o.alloc((size_t)n * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_butterworth_run<float>, dim3(1), dim3(64), 0, 0, make_filtk<float>(cfg->bw_c), (const double*)a.p, (long long)n, (double*)o.p);
  else hipLaunchKernelGGL(k_butterworth_run<double>, dim3(1), dim3(64), 0, 0, make_filtk<double>(cfg->bw_c), (const double*)a.p, (long long)n, (double*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(y_out, o.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_kalman_run(const dql_config* cfg, int device, const double* vel, const uint8_t* dt_le0, int64_t n, double* acc_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 1 && (!vel || !dt_le0 || !acc_out))) return fail(DQL_EINVAL, "null array");
  if (n <= 1) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  UP(a, vel, (size_t)n * 3 * sizeof(double)); UP(b, dt_le0, (size_t)n);
  if (o.alloc((size_t)(n - 1) * 3 * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  const double r = cfg->noise_vel_sd * cfg->noise_vel_sd;  // pkg/filters.py:49
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_kalman_run<float>, dim3(1), dim3(64), 0, 0, (float)cfg->kalman_q, (float)r, (const double*)a.p, (const uint8_t*)b.p, (long long)n, (double*)o.p);
  else hipLaunchKernelGGL(k_kalman_run<double>, dim3(1), dim3(64), 0, 0, (double)cfg->kalman_q, r, (const double*)a.p, (const uint8_t*)b.p, (long long)n, (double*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(acc_out, o.p, (size_t)(n - 1) * 3 * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_pid_run(const dql_config* cfg, int device, const double* params, const double* state, int64_t n, double* effort_out, double* integral_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (!params || n < 0 || (n > 0 && (!state || !effort_out || !integral_out))) return fail(DQL_EINVAL, "null array");
  if (params[2] != 0.0) return fail(DQL_EINVAL, "Kd != 0 is not supported (the reference launches both controllers with Kd = 0, launch/drone.launch:37,51)");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, o, g;
  UP(a, state, (size_t)n * sizeof(double));
  if (o.alloc((size_t)n * sizeof(double)) || g.alloc((size_t)n * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  if (cfg->dtype == DQL_F32) {
    const PidP<float> p{(float)params[0], (float)params[1], (float)params[3], (float)params[4], (float)params[5], (float)params[6]};
    hipLaunchKernelGGL(k_pid_run<float>, dim3(1), dim3(64), 0, 0, make_filtk<float>(cfg->bw_c), p, (const double*)a.p, (long long)n, (double*)o.p, (double*)g.p);
  } else {
    const PidP<double> p{params[0], params[1], params[3], params[4], params[5], params[6]};
    hipLaunchKernelGGL(k_pid_run<double>, dim3(1), dim3(64), 0, 0, make_filtk<double>(cfg->bw_c), p, (const double*)a.p, (long long)n, (double*)o.p, (double*)g.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(effort_out, o.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(integral_out, g.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_attitude_run(const dql_config* cfg, int device, const double* quat_xyzw, const double* omega, const double* cmd, int64_t n, int32_t xonly, double* rotor_out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!quat_xyzw || !omega || !cmd || !rotor_out))) return fail(DQL_EINVAL, "null array");
  if (xonly && cfg->dtype != DQL_F32) return fail(DQL_EINVAL, "the x-axis closed form of the attitude law exists in float32 only");
  if (xonly) for (int64_t i = 0; i < n; ++i) if (cmd[i * 4] != 0.0) return fail(DQL_EINVAL, "the x-axis closed form needs a roll command of exactly 0");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, c, o;
  UP(a, quat_xyzw, (size_t)n * 4 * sizeof(double)); UP(b, omega, (size_t)n * 3 * sizeof(double)); UP(c, cmd, (size_t)n * 4 * sizeof(double));
  if (o.alloc((size_t)n * 4 * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  const unsigned grid = (unsigned)((n + 63) / 64);
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_attitude_run<float>, dim3(grid), dim3(64), 0, 0, make_simk<float>(*cfg), (const double*)a.p, (const double*)b.p, (const double*)c.p, (long long)n, (int)xonly, (double*)o.p);
  else hipLaunchKernelGGL(k_attitude_run<double>, dim3(grid), dim3(64), 0, 0, make_simk<double>(*cfg), (const double*)a.p, (const double*)b.p, (const double*)c.p, (long long)n, (int)xonly, (double*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(rotor_out, o.p, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_platform_run(const dql_config* cfg, int device, int64_t n, int32_t carry, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || carry < 0 || (n > 0 && !out)) return fail(DQL_EINVAL, "bad argument");
  if (carry && cfg->dtype != DQL_F32) return fail(DQL_EINVAL, "the carried sine / cosine exists in the float32 step only");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf o;
  if (o.alloc((size_t)n * 4 * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_platform_run<float>, dim3(1), dim3(64), 0, 0, make_simk<float>(*cfg), (long long)n, (int)carry, (double*)o.p);
  else hipLaunchKernelGGL(k_platform_run<double>, dim3(1), dim3(64), 0, 0, make_simk<double>(*cfg), (long long)n, (int)carry, (double*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, o.p, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_diag_selftest_sqrt(int device, uint32_t lo_bits, uint32_t hi_bits, int64_t* not_correctly_rounded) {
  if (!not_correctly_rounded) return fail(DQL_EINVAL, "null pointer");
  if (lo_bits > hi_bits || hi_bits > 0x7f7fffffu) return fail(DQL_EINVAL, "bit patterns must satisfy lo <= hi <= 0x7f7fffff (largest finite float32)");
  OP_PROLOGUE(device)
  DevBuf b;
  if (b.alloc(sizeof(unsigned long long))) return fail(DQL_ENOMEM, "hipMalloc failed");
  HIP_TRY(hipMemset(b.p, 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(k_selftest_sqrt, dim3(256 * 32), dim3(256), 0, 0, (unsigned)lo_bits, (unsigned)hi_bits, (unsigned long long*)b.p);
  HIP_TRY(hipGetLastError());
  unsigned long long n = 0;
  HIP_TRY(hipMemcpy(&n, b.p, sizeof(n), hipMemcpyDeviceToHost));
  *not_correctly_rounded = (int64_t)n;
  return DQL_OK;
}

int dql_place(const dql_config* cfg, int device, const double* x0, const double* mp, int64_t n, double* out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (n < 0 || (n > 0 && (!x0 || !mp || !out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  OP_PROLOGUE(device)
  DevBuf a, b, o;
  UP(a, x0, (size_t)n * sizeof(double)); UP(b, mp, (size_t)n * sizeof(double));
  if (o.alloc((size_t)n * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (cfg->dtype == DQL_F32) hipLaunchKernelGGL(k_place<float>, dim3(grid), dim3(256), 0, 0, (int)cfg->init_uniform, (float)cfg->p_max, (const double*)a.p, (const double*)b.p, (long long)n, (double*)o.p);
  else hipLaunchKernelGGL(k_place<double>, dim3(grid), dim3(256), 0, 0, (int)cfg->init_uniform, (double)cfg->p_max, (const double*)a.p, (const double*)b.p, (long long)n, (double*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, o.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return DQL_OK;
}

// ---- greedy roll-outs ----
static thread_local double g_rollout_ms = -1.0;
static thread_local int g_rollout_inst[3] = {0, 0, 0};
extern "C++" {
template <typename T, int XMODE> static void launch_rollout(const dql_config& cfg, const void* mdpk, const double* qa, const double* qb, const long long* mgr0, const int* sched,
                                                           const RolloutOut& out, unsigned long long seed, int n_tables, long long envs_per_table, int max_steps) {
  RolloutArgs<T> a;
  a.c = make_simk<T>(cfg);
  a.mdp = (const MdpK<T> DQL_CONST_AS*)mdpk;
  a.mdp_run = MdpRun<T>{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  a.init = make_rollout_init<T>(cfg);
  a.qa = qa; a.qb = qb;
  a.mgr0 = (const long long DQL_CONST_AS*)mgr0; a.sched = (const int DQL_CONST_AS*)sched;
  a.out = out; a.seed = seed; a.blocks_per_table = (int)(envs_per_table / 64); a.max_steps = max_steps;
  g_rollout_inst[0] = (int)sizeof(T); g_rollout_inst[1] = TICK_PLAIN; g_rollout_inst[2] = XMODE;
  hipLaunchKernelGGL((k_rollout<T, TICK_PLAIN, XMODE>), dim3((unsigned)((long long)n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
}
}  // extern "C++"
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
  if (!qa || !qb || !code || !steps || !rec) return fail(DQL_EINVAL, "dql_rollout: null array; nothing was launched");
  OP_PROLOGUE(device)
  const long long n_total = (long long)n_tables * envs_per_table;
  const int n_per = max_steps + 1;
  std::vector<long long> h_mgr0((size_t)n_per);
  std::vector<int> h_sched((size_t)n_per);
  fill_schedule(*cfg, 0, h_mgr0.data(), h_sched.data(), n_per);
  DevBuf d_qa, d_qb, d_mgr0, d_sched, d_mdp, d_code, d_steps, d_rec, d_trace;
  const size_t TB = (size_t)n_tables * DQL_N_CELLS * sizeof(double);
  UP(d_qa, qa, TB); UP(d_qb, qb, TB);
  UP(d_mgr0, h_mgr0.data(), (size_t)n_per * sizeof(long long)); UP(d_sched, h_sched.data(), (size_t)n_per * sizeof(int));
  if (cfg->dtype == DQL_F32) { const MdpK<float> m = make_mdpk<float>(*cfg); UP(d_mdp, &m, sizeof(m)); }
  else { const MdpK<double> m = make_mdpk<double>(*cfg); UP(d_mdp, &m, sizeof(m)); }
  if (d_code.alloc((size_t)n_total * sizeof(int)) || d_steps.alloc((size_t)n_total * sizeof(int)) || d_rec.alloc((size_t)RO_N_RECORD * n_total * sizeof(double))) return fail(DQL_ENOMEM, "hipMalloc failed");
  const size_t trace_bytes = (size_t)n_per * RO_N_TRACE * (size_t)trace_envs * sizeof(double);
  if (trace_envs > 0) {
    if (d_trace.alloc(trace_bytes)) return fail(DQL_ENOMEM, "hipMalloc failed");
    HIP_TRY(hipMemset(d_trace.p, 0xff, trace_bytes));  // all ones = NaN: what a row keeps after its env's last period
  }
  const RolloutOut out{(int*)d_code.p, (int*)d_steps.p, (double*)d_rec.p, trace_envs > 0 ? (double*)d_trace.p : nullptr, n_total, trace_envs};
  struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } e0, e1;
  HIP_TRY(hipEventCreate(&e0.e)); HIP_TRY(hipEventCreate(&e1.e));
  HIP_TRY(hipEventRecord(e0.e, 0));
  const bool two = cfg->two_axis != 0;
  if (cfg->dtype == DQL_F32) {
    if (two) launch_rollout<float, X_TWO>(*cfg, d_mdp.p, (const double*)d_qa.p, (const double*)d_qb.p, (const long long*)d_mgr0.p, (const int*)d_sched.p, out, seed, n_tables, envs_per_table, max_steps);
    else launch_rollout<float, X_ONLY>(*cfg, d_mdp.p, (const double*)d_qa.p, (const double*)d_qb.p, (const long long*)d_mgr0.p, (const int*)d_sched.p, out, seed, n_tables, envs_per_table, max_steps);
  } else {
    if (two) launch_rollout<double, X_TWO>(*cfg, d_mdp.p, (const double*)d_qa.p, (const double*)d_qb.p, (const long long*)d_mgr0.p, (const int*)d_sched.p, out, seed, n_tables, envs_per_table, max_steps);
    else launch_rollout<double, X_ONLY>(*cfg, d_mdp.p, (const double*)d_qa.p, (const double*)d_qb.p, (const long long*)d_mgr0.p, (const int*)d_sched.p, out, seed, n_tables, envs_per_table, max_steps);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1.e, 0));
  HIP_TRY(hipMemcpy(code, d_code.p, (size_t)n_total * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(steps, d_steps.p, (size_t)n_total * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rec, d_rec.p, (size_t)RO_N_RECORD * n_total * sizeof(double), hipMemcpyDeviceToHost));
  if (trace_envs > 0) HIP_TRY(hipMemcpy(trace_or_null, d_trace.p, trace_bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipEventSynchronize(e1.e));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
  g_rollout_ms = (double)ms;
  return DQL_OK;
}
int dql_diag_rollout_last(double* kernel_ms, int32_t* out3) {
  if (!kernel_ms || !out3) return fail(DQL_EINVAL, "null pointer");
  if (g_rollout_ms < 0.0) return fail(DQL_ESTATE, "no dql_rollout call has completed on this thread");
  *kernel_ms = g_rollout_ms;
  for (int k = 0; k < 3; ++k) out3[k] = g_rollout_inst[k];
  return DQL_OK;
}

// ---- greedy scoring ----
static thread_local double g_score_ms = -1.0;
static thread_local int g_score_inst[3] = {0, 0, 0};
extern "C++" {
template <typename T, int XMODE> static void launch_score(const dql_config& cfg, const void* mdpk, const double* qa, const double* qb, const long long* mgr0, const int* sched,
                                                         unsigned long long* by_code, unsigned long long* steps_sum, const ScoreLog& log, unsigned long long seed,
                                                         long long n_tables, long long envs_per_table, int episodes, int max_steps) {
  ScoreArgs<T> a;
  a.c = make_simk<T>(cfg);
  a.mdp = (const MdpK<T> DQL_CONST_AS*)mdpk;
  a.mdp_run = MdpRun<T>{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  a.init = make_rollout_init<T>(cfg);
  a.qa = qa; a.qb = qb;
  a.mgr0 = (const long long DQL_CONST_AS*)mgr0; a.sched = (const int DQL_CONST_AS*)sched;
  a.by_code = by_code; a.steps_sum = steps_sum; a.log = log;
  a.seed = seed; a.blocks_per_table = (int)(envs_per_table / 64); a.max_steps = max_steps; a.episodes = episodes;
  g_score_inst[0] = (int)sizeof(T); g_score_inst[1] = TICK_PLAIN; g_score_inst[2] = XMODE;
  hipLaunchKernelGGL((k_score<T, TICK_PLAIN, XMODE>), dim3((unsigned)(n_tables * a.blocks_per_table)), dim3(64), 0, 0, a);
}
}  // extern "C++"
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
// d_qa / d_qb: [n_tables][DQL_N_CELLS] on the current device
static int score_run(const dql_config* cfg, long long n_tables, long long envs_per_table, int episodes, uint64_t seed, int max_steps, const double* d_qa, const double* d_qb,
                     int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code, uint16_t* ep_steps) {
  const long long n_total = n_tables * envs_per_table;
  const int n_per = max_steps + 1;
  std::vector<long long> h_mgr0((size_t)n_per);
  std::vector<int> h_sched((size_t)n_per);
  fill_schedule(*cfg, 0, h_mgr0.data(), h_sched.data(), n_per);
  DevBuf d_mgr0, d_sched, d_mdp, d_sums, d_code, d_steps;
  UP(d_mgr0, h_mgr0.data(), (size_t)n_per * sizeof(long long)); UP(d_sched, h_sched.data(), (size_t)n_per * sizeof(int));
  if (cfg->dtype == DQL_F32) { const MdpK<float> m = make_mdpk<float>(*cfg); UP(d_mdp, &m, sizeof(m)); }
  else { const MdpK<double> m = make_mdpk<double>(*cfg); UP(d_mdp, &m, sizeof(m)); }
  // one buffer for both sums: [n_tables][SCORE_N_COLS] counts, then [n_tables] step totals
  const size_t sums_bytes = (size_t)n_tables * (SCORE_N_COLS + 1) * sizeof(unsigned long long);
  if (d_sums.alloc(sums_bytes)) return fail(DQL_ENOMEM, "hipMalloc failed");
  HIP_TRY(hipMemset(d_sums.p, 0, sums_bytes));
  const size_t log_n = (size_t)episodes * (size_t)n_total;
  if (ep_code) {
    if (d_code.alloc(log_n) || d_steps.alloc(log_n * sizeof(uint16_t))) return fail(DQL_ENOMEM, "hipMalloc failed");
    HIP_TRY(hipMemset(d_code.p, 0xff, log_n));  // not finished
    HIP_TRY(hipMemset(d_steps.p, 0, log_n * sizeof(uint16_t)));
  }
  unsigned long long* d_by_code = (unsigned long long*)d_sums.p;
  unsigned long long* d_steps_sum = d_by_code + (size_t)n_tables * SCORE_N_COLS;
  const ScoreLog log{(uint8_t*)d_code.p, (uint16_t*)d_steps.p, n_total};
  struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } e0, e1;
  HIP_TRY(hipEventCreate(&e0.e)); HIP_TRY(hipEventCreate(&e1.e));
  HIP_TRY(hipEventRecord(e0.e, 0));
  const bool two = cfg->two_axis != 0;
  const long long* mg = (const long long*)d_mgr0.p; const int* sc = (const int*)d_sched.p;
  if (cfg->dtype == DQL_F32) {
    if (two) launch_score<float, X_TWO>(*cfg, d_mdp.p, d_qa, d_qb, mg, sc, d_by_code, d_steps_sum, log, seed, n_tables, envs_per_table, episodes, max_steps);
    else launch_score<float, X_ONLY>(*cfg, d_mdp.p, d_qa, d_qb, mg, sc, d_by_code, d_steps_sum, log, seed, n_tables, envs_per_table, episodes, max_steps);
  } else {
    if (two) launch_score<double, X_TWO>(*cfg, d_mdp.p, d_qa, d_qb, mg, sc, d_by_code, d_steps_sum, log, seed, n_tables, envs_per_table, episodes, max_steps);
    else launch_score<double, X_ONLY>(*cfg, d_mdp.p, d_qa, d_qb, mg, sc, d_by_code, d_steps_sum, log, seed, n_tables, envs_per_table, episodes, max_steps);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1.e, 0));
  HIP_TRY(hipMemcpy(by_code, d_by_code, (size_t)n_tables * SCORE_N_COLS * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(steps_sum, d_steps_sum, (size_t)n_tables * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (ep_code) {
    HIP_TRY(hipMemcpy(ep_code, d_code.p, log_n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ep_steps, d_steps.p, log_n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipEventSynchronize(e1.e));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
  g_score_ms = (double)ms;
  return DQL_OK;
}
int dql_score(const dql_config* cfg, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps,
              const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null) {
  int rc = check_config(cfg); if (rc) return rc;
  rc = score_check("dql_score", n_tables, envs_per_table, episodes_per_env, max_steps, by_code, steps_sum, ep_code_or_null, ep_steps_or_null); if (rc) return rc;
  if (!qa || !qb) return fail(DQL_EINVAL, "dql_score: null array; nothing was launched");
  OP_PROLOGUE(device)
  DevBuf d_qa, d_qb;
  const size_t TB = (size_t)n_tables * DQL_N_CELLS * sizeof(double);
  UP(d_qa, qa, TB); UP(d_qb, qb, TB);
  return score_run(cfg, n_tables, envs_per_table, episodes_per_env, seed, max_steps, (const double*)d_qa.p, (const double*)d_qb.p, by_code, steps_sum, ep_code_or_null, ep_steps_or_null);
}
int dql_diag_score_last(double* kernel_ms, int32_t* inst3) {
  if (!kernel_ms || !inst3) return fail(DQL_EINVAL, "null pointer");
  if (g_score_ms < 0.0) return fail(DQL_ESTATE, "no dql_score or dql_ensemble_score call has completed on this thread");
  *kernel_ms = g_score_ms;
  for (int k = 0; k < 3; ++k) inst3[k] = g_score_inst[k];
  return DQL_OK;
}

// ---- ensembles of sequential learners ----
struct dql_ensemble {
  dql_config cfg;
  int device = 0;
  long long n = 0;
  unsigned long long seed = 0;
  long long j = 0;  // the ensemble's period index (period 0 is the reset period)
  void* sr = nullptr; int4* si = nullptr; void* mdpk = nullptr;
  LearnMem mem{};
  LearnSched sched{};
  double* alpha_tab = nullptr; uint32_t* eps_tab = nullptr;
  long long* d_mgr0 = nullptr; int* d_sched = nullptr;  // [LEARN_MAX_PERIODS]
  double last_ms = -1.0;
  // per-learner curriculum levels; advance_every = 0: the mode is off
  AdvanceMem adv{};
  AdvanceRule rule{};
  int advance_every = 0;
  void* mdpk5 = nullptr;                                      // [DQL_MAX_LEVELS] MdpK<T>, entry k with working = k
  LevelSched* d_lv = nullptr; LevelSched h_lv[DQL_MAX_LEVELS]{}; bool have_lv[DQL_MAX_LEVELS]{};
  int* d_worklist = nullptr; int* d_wave_level = nullptr; long long wl_slots = 0;
  long long n_launches = 0, launched_periods = 0, launched_wave_periods = 0;  // since creation (dql_diag_ensemble_launches)
};
#define CHECK_ENS(e) do { if (!(e)) return fail(DQL_EINVAL, "null ensemble"); } while (0)
static void ens_free(dql_ensemble* x) {
  void* ptrs[] = {x->sr, x->si, x->mdpk, x->mem.qa, x->mem.qb, x->mem.count, x->mem.decisions, x->mem.by_code, x->mem.episodes, x->mem.successes, x->mem.level_episodes,
                  x->mem.win_count, x->mem.win_bits, x->mem.promoted, x->mem.frozen, x->mem.log_code, x->mem.log_len, x->mem.log_n, x->mem.faults, x->alpha_tab, x->eps_tab,
                  x->d_mgr0, x->d_sched, x->adv.level, x->adv.promoted_at, x->adv.episodes_at, x->adv.entered_period, x->mdpk5, x->d_lv, x->d_worklist, x->d_wave_level,
                  (void*)x->h_lv[0].eps_tab, (void*)x->h_lv[1].eps_tab, (void*)x->h_lv[2].eps_tab, (void*)x->h_lv[3].eps_tab, (void*)x->h_lv[4].eps_tab};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  delete x;
}
static int ens_upload_mdpk(dql_ensemble* x) {
  if (x->cfg.dtype == DQL_F32) { const MdpK<float> m = make_mdpk<float>(x->cfg); HIP_TRY(hipMemcpy(x->mdpk, &m, sizeof(m), hipMemcpyHostToDevice)); }
  else { const MdpK<double> m = make_mdpk<double>(x->cfg); HIP_TRY(hipMemcpy(x->mdpk, &m, sizeof(m), hipMemcpyHostToDevice)); }
  return DQL_OK;
}
// every learner to level k: the per-level history from level k on is cleared, level k is entered at the present period index
static int ens_set_levels(dql_ensemble* x, int k) {
  const size_t n = (size_t)x->n;
  if (x->j == 0) HIP_TRY(hipMemset(x->adv.entered_period, 0xff, (size_t)DQL_MAX_LEVELS * n * sizeof(long long)));  // nothing was flown: no level below k was ever entered
  std::vector<int> lv(n, k);
  HIP_TRY(hipMemcpy(x->adv.level, lv.data(), n * sizeof(int), hipMemcpyHostToDevice));
  const size_t from = (size_t)k * n, rest = (size_t)(DQL_MAX_LEVELS - k) * n;
  HIP_TRY(hipMemset(x->adv.promoted_at + from, 0xff, rest * sizeof(int)));
  HIP_TRY(hipMemset(x->adv.episodes_at + from, 0, rest * sizeof(int)));
  HIP_TRY(hipMemset(x->adv.entered_period + from, 0xff, rest * sizeof(long long)));
  std::vector<long long> at(n, x->j);
  HIP_TRY(hipMemcpy(x->adv.entered_period + from, at.data(), n * sizeof(long long), hipMemcpyHostToDevice));
  return DQL_OK;
}
// the five levels' MdpK (they differ in `working` only), read by k_learn_levels at the wave's level
static int ens_upload_mdpk5(dql_ensemble* x) {
  dql_config c = x->cfg;
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) {
    c.working_curriculum_step = k;
    if (x->cfg.dtype == DQL_F32) { const MdpK<float> m = make_mdpk<float>(c); HIP_TRY(hipMemcpy((MdpK<float>*)x->mdpk5 + k, &m, sizeof(m), hipMemcpyHostToDevice)); }
    else { const MdpK<double> m = make_mdpk<double>(c); HIP_TRY(hipMemcpy((MdpK<double>*)x->mdpk5 + k, &m, sizeof(m), hipMemcpyHostToDevice)); }
  }
  return DQL_OK;
}
// per-level episode counts, windows, promotion records and frozen flags back to "just started"
static int ens_rearm(dql_ensemble* x) {
  const size_t n = (size_t)x->n;
  HIP_TRY(hipMemset(x->mem.level_episodes, 0, n * sizeof(int)));
  HIP_TRY(hipMemset(x->mem.win_count, 0, n * sizeof(int)));
  HIP_TRY(hipMemset(x->mem.win_bits, 0, 2 * n * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(x->mem.promoted, 0xff, n * sizeof(int)));
  HIP_TRY(hipMemset(x->mem.frozen, 0, n * sizeof(int)));
  return DQL_OK;
}
extern "C++" {
template <typename T> static int ens_init(dql_ensemble* x) {
  InitArgs<T> a;
  a.c = make_simk<T>(x->cfg);
  a.sr = (Quad<T>*)x->sr; a.si = x->si; a.n = x->n; a.seed = x->seed; a.env_id_offset = 0;
  const RolloutInit<T> r = make_rollout_init<T>(x->cfg);
  a.hover = r.hover; a.vz_integ = r.vz_integ; a.r_lo = r.r_lo; a.r_hi = r.r_hi; a.t_lo = r.t_lo; a.t_hi = r.t_hi;
  hipLaunchKernelGGL(k_init<T>, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}
template <typename T> static void ens_launch(dql_ensemble* x, int n_periods) {
  LearnArgs<T> a;
  a.c = make_simk<T>(x->cfg);
  a.mdp = (const MdpK<T> DQL_CONST_AS*)x->mdpk;
  a.mdp_run = MdpRun<T>{x->cfg.gamma, (T)(x->cfg.t_max * x->cfg.f_ag), x->cfg.goal_logic};
  a.sched = x->sched; a.mem = x->mem;
  a.sr = (Quad<T>*)x->sr; a.si = x->si;
  a.mgr0 = (const long long DQL_CONST_AS*)x->d_mgr0; a.tick_sched = (const int DQL_CONST_AS*)x->d_sched;
  a.seed = x->seed; a.j0 = x->j; a.n_periods = n_periods;
  hipLaunchKernelGGL((k_learn<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)((x->n + 63) / 64)), dim3(64), 0, 0, a);
}
template <typename T> static void ens_launch_levels(dql_ensemble* x, int n_periods, int n_waves) {
  LearnLevelsArgs<T> g;
  LearnArgs<T>& a = g.a;
  a.c = make_simk<T>(x->cfg);
  a.mdp = (const MdpK<T> DQL_CONST_AS*)x->mdpk5;
  a.mdp_run = MdpRun<T>{x->cfg.gamma, (T)(x->cfg.t_max * x->cfg.f_ag), x->cfg.goal_logic};
  a.sched = x->sched; a.mem = x->mem;
  a.sr = (Quad<T>*)x->sr; a.si = x->si;
  a.mgr0 = (const long long DQL_CONST_AS*)x->d_mgr0; a.tick_sched = (const int DQL_CONST_AS*)x->d_sched;
  a.seed = x->seed; a.j0 = x->j; a.n_periods = n_periods;
  g.lv = (const LevelSched DQL_CONST_AS*)x->d_lv; g.worklist = x->d_worklist; g.wave_level = (const int DQL_CONST_AS*)x->d_wave_level; g.n_waves = n_waves;
  hipLaunchKernelGGL((k_learn_levels<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, g);
}
template <typename T> static int ens_get_state_t(dql_ensemble* x, double* out) {
  const long long n = x->n;
  std::vector<T> h((size_t)NQ_REAL * n * 4);
  HIP_TRY(hipMemcpy(h.data(), x->sr, h.size() * sizeof(T), hipMemcpyDeviceToHost));
  for (int f = 0; f < NF_REAL; ++f) { const int q = f / 4, k = f % 4; for (long long i = 0; i < n; ++i) out[(long long)f * n + i] = (double)h[((size_t)q * n + i) * 4 + k]; }
  return DQL_OK;
}
}  // extern "C++"
#define ENS_ALLOC(ptr, bytes) do { if (hipMalloc((void**)&(ptr), (bytes)) != hipSuccess) { (ptr) = nullptr; ens_free(x); return fail(DQL_ENOMEM, "hipMalloc failed"); } \
                                   if (hipMemset((ptr), 0, (bytes)) != hipSuccess) { ens_free(x); return fail(DQL_EHIP, "hipMemset failed"); } } while (0)
int dql_ensemble_create(const dql_config* cfg, int device, int64_t n_learners, uint64_t seed, int32_t log_capacity, dql_ensemble** out) {
  int rc = check_config(cfg); if (rc) return rc;
  if (!out) return fail(DQL_EINVAL, "dql_ensemble_create: null pointer; nothing was launched");
  if (cfg->two_axis) return fail(DQL_EINVAL, "dql_ensemble_create: two-axis configs are refused (the reference's learner is x-only); nothing was launched");
  if (cfg->trajectory == DQL_TRAJ_EIGHT) return fail(DQL_EINVAL, "dql_ensemble_create: the figure-eight trajectory is refused (the reference's learner is x-only); nothing was launched");
  if (n_learners < 1 || n_learners > DQL_ENSEMBLE_MAX_LEARNERS) return fail(DQL_EINVAL, "dql_ensemble_create: n_learners must be in 1..2^20 (DQL_ENSEMBLE_MAX_LEARNERS); nothing was launched");
  if (log_capacity < 0 || log_capacity > DQL_ENSEMBLE_MAX_LOG) return fail(DQL_EINVAL, "dql_ensemble_create: log_capacity must be in 0..2^20 (DQL_ENSEMBLE_MAX_LOG); nothing was launched");
  OP_PROLOGUE(device)
  dql_ensemble* x = new dql_ensemble;
  x->cfg = *cfg; x->device = device; x->n = n_learners; x->seed = seed;
  const size_t n = (size_t)n_learners, real = cfg->dtype == DQL_F32 ? 4 : 8;
  const size_t TB = n * DQL_N_CELLS * sizeof(double);
  ENS_ALLOC(x->sr, (size_t)NQ_REAL * n * 4 * real);
  ENS_ALLOC(x->si, n * sizeof(int4));
  ENS_ALLOC(x->mdpk, cfg->dtype == DQL_F32 ? sizeof(MdpK<float>) : sizeof(MdpK<double>));
  ENS_ALLOC(x->mem.qa, TB); ENS_ALLOC(x->mem.qb, TB); ENS_ALLOC(x->mem.count, TB);
  ENS_ALLOC(x->mem.decisions, n * sizeof(unsigned long long));
  ENS_ALLOC(x->mem.by_code, (size_t)DQL_N_CHECK_CODES * n * sizeof(unsigned long long));
  ENS_ALLOC(x->mem.episodes, n * sizeof(int)); ENS_ALLOC(x->mem.successes, n * sizeof(int));
  ENS_ALLOC(x->mem.level_episodes, n * sizeof(int)); ENS_ALLOC(x->mem.win_count, n * sizeof(int));
  ENS_ALLOC(x->mem.win_bits, 2 * n * sizeof(unsigned long long));
  ENS_ALLOC(x->mem.promoted, n * sizeof(int)); ENS_ALLOC(x->mem.frozen, n * sizeof(int));
  ENS_ALLOC(x->mem.log_code, n * (size_t)(log_capacity ? log_capacity : 1)); ENS_ALLOC(x->mem.log_len, n * (size_t)(log_capacity ? log_capacity : 1) * sizeof(uint16_t));
  ENS_ALLOC(x->mem.log_n, n * sizeof(int));
  ENS_ALLOC(x->mem.faults, sizeof(unsigned long long));
  ENS_ALLOC(x->d_mgr0, (size_t)LEARN_MAX_PERIODS * sizeof(long long)); ENS_ALLOC(x->d_sched, (size_t)LEARN_MAX_PERIODS * sizeof(int));
  ENS_ALLOC(x->adv.level, n * sizeof(int));
  ENS_ALLOC(x->adv.promoted_at, (size_t)DQL_MAX_LEVELS * n * sizeof(int)); ENS_ALLOC(x->adv.episodes_at, (size_t)DQL_MAX_LEVELS * n * sizeof(int));
  ENS_ALLOC(x->adv.entered_period, (size_t)DQL_MAX_LEVELS * n * sizeof(long long));
  ENS_ALLOC(x->mdpk5, (size_t)DQL_MAX_LEVELS * (cfg->dtype == DQL_F32 ? sizeof(MdpK<float>) : sizeof(MdpK<double>)));
  ENS_ALLOC(x->d_lv, (size_t)DQL_MAX_LEVELS * sizeof(LevelSched));
  x->wl_slots = worklist_capacity(n_learners);
  ENS_ALLOC(x->d_worklist, (size_t)x->wl_slots * sizeof(int)); ENS_ALLOC(x->d_wave_level, (size_t)(x->wl_slots / ADV_WAVE) * sizeof(int));
  x->mem.n = n_learners; x->mem.log_cap = log_capacity;
  rc = ens_upload_mdpk(x);
  if (!rc) rc = ens_upload_mdpk5(x);
  if (!rc) rc = ens_set_levels(x, 0);  // the whole history cleared ...
  if (!rc) rc = ens_set_levels(x, cfg->working_curriculum_step);  // ... and the config's level entered at period 0
  if (!rc) rc = ens_rearm(x);
  if (!rc) rc = cfg->dtype == DQL_F32 ? ens_init<float>(x) : ens_init<double>(x);
  // default schedules: the plateau learning rate, no exploration, the reference's window (100 episodes, 97 successes) and no episode budget
  const double a0 = cfg->alpha_min; const double e0 = 0.0;
  if (!rc) rc = dql_ensemble_set_schedules(x, &a0, 1, &e0, 1, 100, 97, INT32_MAX);
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(DQL_EHIP, "hipDeviceSynchronize failed");
  if (rc) { ens_free(x); return rc; }
  *out = x;
  return DQL_OK;
}
int dql_ensemble_destroy(dql_ensemble* x) {
  if (!x) return DQL_OK;
  (void)hipSetDevice(x->device);
  (void)hipDeviceSynchronize();
  ens_free(x);
  return DQL_OK;
}
int dql_ensemble_n_learners(dql_ensemble* x, int64_t* n) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "null pointer");
  *n = x->n;
  return DQL_OK;
}
int dql_ensemble_set_schedules(dql_ensemble* x, const double* alpha, int32_t n_alpha, const double* eps, int32_t n_eps, int32_t window, int32_t min_successes,
                               int32_t max_episodes) {
  CHECK_ENS(x);
  if (!alpha || !eps) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: null table");
  if (n_alpha < 1 || n_alpha > (1 << 22) || n_eps < 1 || n_eps > (1 << 22)) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: table lengths must be in 1..2^22");
  if (window < 1 || window > DQL_ENSEMBLE_MAX_WINDOW) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: the promotion window must be in 1..128 (DQL_ENSEMBLE_MAX_WINDOW)");
  if (min_successes < 1 || max_episodes < 1) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: min_successes and max_episodes must be positive");
  for (int i = 0; i < n_alpha; ++i) if (!(alpha[i] >= 0.0 && alpha[i] <= 1.0)) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: learning rates must be in [0, 1]");
  for (int i = 0; i < n_eps; ++i) if (!(eps[i] >= 0.0 && eps[i] <= 1.0)) return fail(DQL_EINVAL, "dql_ensemble_set_schedules: exploration rates must be in [0, 1]");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> thr((size_t)n_eps);
  for (int i = 0; i < n_eps; ++i) thr[(size_t)i] = eps_threshold(eps[i]);
  double* d_a = nullptr; uint32_t* d_e = nullptr;
  if (hipMalloc((void**)&d_a, (size_t)n_alpha * sizeof(double)) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc failed");
  if (hipMalloc((void**)&d_e, (size_t)n_eps * sizeof(uint32_t)) != hipSuccess) { (void)hipFree(d_a); return fail(DQL_ENOMEM, "hipMalloc failed"); }
  if (hipMemcpy(d_a, alpha, (size_t)n_alpha * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_e, thr.data(), (size_t)n_eps * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d_a); (void)hipFree(d_e);
    return fail(DQL_EHIP, "hipMemcpy failed");
  }
  if (x->alpha_tab) (void)hipFree(x->alpha_tab);
  if (x->eps_tab) (void)hipFree(x->eps_tab);
  x->alpha_tab = d_a; x->eps_tab = d_e;
  x->sched = LearnSched{d_a, n_alpha, x->cfg.alpha_min, d_e, n_eps, window, min_successes, max_episodes};
  return DQL_OK;
}
int dql_ensemble_rearm(dql_ensemble* x) {
  CHECK_ENS(x);
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  return ens_rearm(x);
}
int dql_ensemble_set_level(dql_ensemble* x, int32_t k) {
  CHECK_ENS(x);
  if (k < 0 || k >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_level: curriculum step must be in 0..4");
  if (x->advance_every && k > x->rule.last_level)
    return fail(DQL_EINVAL, "dql_ensemble_set_level: in curriculum mode the level must not exceed last_level (raise it with dql_ensemble_set_curriculum first); nothing was changed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  x->cfg.working_curriculum_step = k;
  int rc = ens_upload_mdpk(x); if (rc) return rc;
  hipLaunchKernelGGL(k_mark_reset, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, 0, x->si, (const uint8_t*)nullptr, (long long)x->n);  // every env re-enters through reset
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  rc = ens_set_levels(x, k); if (rc) return rc;
  return ens_rearm(x);
}
int dql_ensemble_n_live(dql_ensemble* x, int64_t* n_live) {
  CHECK_ENS(x);
  if (!n_live) return fail(DQL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(x->device));
  std::vector<int> h((size_t)x->n);
  HIP_TRY(hipMemcpy(h.data(), x->mem.frozen, h.size() * sizeof(int), hipMemcpyDeviceToHost));
  int64_t live = 0;
  for (int v : h) live += v ? 0 : 1;
  *n_live = live;
  return DQL_OK;
}
// frozen, level and promoted of every learner -> host; the learners that are not finished for good
static int ens_fetch_levels(dql_ensemble* x, std::vector<int>& frozen, std::vector<int>& level, std::vector<int>& promoted, int64_t* unfinished) {
  const size_t n = (size_t)x->n;
  frozen.resize(n); level.resize(n); promoted.resize(n);
  HIP_TRY(hipMemcpy(frozen.data(), x->mem.frozen, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(level.data(), x->adv.level, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(promoted.data(), x->mem.promoted, n * sizeof(int), hipMemcpyDeviceToHost));
  int64_t u = 0;
  for (size_t l = 0; l < n; ++l) u += learner_finished(frozen[l], level[l], promoted[l], x->rule) ? 0 : 1;
  *unfinished = u;
  return DQL_OK;
}
// dql_ensemble_run in curriculum mode: the launches are cut at the multiples of advance_every; at such a period index j, before period j is flown, every
// learner takes advance_learner's step; each launch flies the live learners regrouped by level (build_worklist)
static int ens_run_levels(dql_ensemble* x, int64_t periods) {
  std::vector<int> frozen, level, promoted;
  int64_t unfinished = 0;
  int rc = ens_fetch_levels(x, frozen, level, promoted, &unfinished); if (rc) return rc;
  // the level a learner stands on is flown whatever last_level says, so its schedule is asked for first; then every level on its way up to last_level
  for (size_t l = 0; l < (size_t)x->n; ++l) {
    bool ok = level[l] >= 0 && level[l] < DQL_MAX_LEVELS && x->have_lv[level[l]];
    for (int k = level[l] + 1; ok && k <= x->rule.last_level && k < DQL_MAX_LEVELS; ++k) ok = x->have_lv[k];
    if (!ok) return fail(DQL_EINVAL, "dql_ensemble_run: curriculum mode needs dql_ensemble_set_level_schedules for every level from the learners' up to last_level; nothing was launched");
  }
  struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } e0, e1;
  HIP_TRY(hipEventCreate(&e0.e)); HIP_TRY(hipEventCreate(&e1.e));
  HIP_TRY(hipEventRecord(e0.e, 0));
  std::vector<long long> h_mgr0((size_t)LEARN_MAX_PERIODS);
  std::vector<int> h_sched((size_t)LEARN_MAX_PERIODS);
  std::vector<int> worklist((size_t)x->wl_slots), wave_level((size_t)(x->wl_slots / ADV_WAVE));
  const long long E = x->advance_every;
  long long left = periods;
  while (left > 0) {
    if (x->j % E == 0) {  // an advance point
      hipLaunchKernelGGL(k_ens_advance, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, 0, x->mem, x->adv, x->rule, x->si, (long long)x->j, (int)DQL_CELLS_PER_LEVEL);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
    }
    rc = ens_fetch_levels(x, frozen, level, promoted, &unfinished); if (rc) return rc;
    if (unfinished == 0) { x->j += left; break; }  // nothing left to fly or to advance, now or later (the period index still advances by `periods`)
    const long long to_point = E - x->j % E;
    const int k = (int)(left < to_point ? left : to_point);  // <= advance_every <= LEARN_MAX_PERIODS
    unsigned long long wl_faults = 0ull;
    const int n_waves = build_worklist(frozen.data(), level.data(), x->n, worklist.data(), wave_level.data(), x->wl_slots, &wl_faults);
    if (wl_faults) {
      unsigned long long v = 0;
      HIP_TRY(hipMemcpy(&v, x->mem.faults, sizeof(v), hipMemcpyDeviceToHost));
      v += wl_faults;
      HIP_TRY(hipMemcpy(x->mem.faults, &v, sizeof(v), hipMemcpyHostToDevice));
    }
    if (n_waves > 0) {  // (nobody live: everyone unfinished waits for the next advance point)
      fill_schedule(x->cfg, x->j, h_mgr0.data(), h_sched.data(), k);
      HIP_TRY(hipMemcpy(x->d_mgr0, h_mgr0.data(), (size_t)k * sizeof(long long), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(x->d_sched, h_sched.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(x->d_worklist, worklist.data(), (size_t)n_waves * ADV_WAVE * sizeof(int), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(x->d_wave_level, wave_level.data(), (size_t)n_waves * sizeof(int), hipMemcpyHostToDevice));
      if (x->cfg.dtype == DQL_F32) ens_launch_levels<float>(x, k, n_waves); else ens_launch_levels<double>(x, k, n_waves);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
      x->n_launches += 1; x->launched_periods += k; x->launched_wave_periods += (long long)n_waves * k;
    }
    x->j += k; left -= k;
  }
  HIP_TRY(hipEventRecord(e1.e, 0));
  HIP_TRY(hipEventSynchronize(e1.e));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
  x->last_ms = (double)ms;
  return DQL_OK;
}
int dql_ensemble_run(dql_ensemble* x, int64_t periods) {
  CHECK_ENS(x);
  if (periods < 1 || periods > (1ll << 40)) return fail(DQL_EINVAL, "dql_ensemble_run: periods must be in 1..2^40; nothing was launched");
  HIP_TRY(hipSetDevice(x->device));
  if (x->advance_every) return ens_run_levels(x, periods);
  struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } e0, e1;
  HIP_TRY(hipEventCreate(&e0.e)); HIP_TRY(hipEventCreate(&e1.e));
  HIP_TRY(hipEventRecord(e0.e, 0));
  std::vector<long long> h_mgr0((size_t)LEARN_MAX_PERIODS);
  std::vector<int> h_sched((size_t)LEARN_MAX_PERIODS);
  long long left = periods;
  while (left > 0) {
    const int k = (int)(left < LEARN_MAX_PERIODS ? left : LEARN_MAX_PERIODS);
    if (left != periods) {  // between the launches of a long run: nothing left to fly ends it (the period index still advances by `periods`)
      int64_t live = 0;
      int rc = dql_ensemble_n_live(x, &live); if (rc) return rc;
      if (live == 0) { x->j += left; break; }
    }
    fill_schedule(x->cfg, x->j, h_mgr0.data(), h_sched.data(), k);
    HIP_TRY(hipMemcpy(x->d_mgr0, h_mgr0.data(), (size_t)k * sizeof(long long), hipMemcpyHostToDevice));  // (synchronous: the previous launch has read its schedule)
    HIP_TRY(hipMemcpy(x->d_sched, h_sched.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice));
    if (x->cfg.dtype == DQL_F32) ens_launch<float>(x, k); else ens_launch<double>(x, k);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    x->n_launches += 1; x->launched_periods += k; x->launched_wave_periods += ((x->n + 63) / 64) * k;
    x->j += k; left -= k;
  }
  HIP_TRY(hipEventRecord(e1.e, 0));
  HIP_TRY(hipEventSynchronize(e1.e));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
  x->last_ms = (double)ms;
  return DQL_OK;
}
// ---- per-learner curriculum levels ----
int dql_ensemble_set_curriculum(dql_ensemble* x, int32_t last_level, int32_t advance_every, const double* ratios, int32_t advance_exhausted) {
  CHECK_ENS(x);
  if (advance_every < 0 || advance_every > ADV_MAX_EVERY) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: advance_every must be in 0..4096 (0 turns the mode off); nothing was changed");
  if (advance_every == 0) {
    // the plain launch flies everyone at the config's level: switching off is refused while a learner stands on another one (dql_ensemble_set_level first)
    if (x->advance_every) {
      HIP_TRY(hipSetDevice(x->device));
      HIP_TRY(hipDeviceSynchronize());
      std::vector<int> lv((size_t)x->n);
      HIP_TRY(hipMemcpy(lv.data(), x->adv.level, lv.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (int v : lv)
        if (v != x->cfg.working_curriculum_step)
          return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: the mode cannot be switched off (advance_every = 0) while learners stand on different levels; call dql_ensemble_set_level first; nothing was changed");
    }
    x->advance_every = 0;
    return DQL_OK;
  }
  if (!ratios) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: null ratios; nothing was changed");
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) if (!std::isfinite(ratios[k])) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: the five transfer ratios must be finite; nothing was changed");
  if (advance_exhausted != 0 && advance_exhausted != 1) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: advance_exhausted must be 0 or 1; nothing was changed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int> level((size_t)x->n);
  HIP_TRY(hipMemcpy(level.data(), x->adv.level, level.size() * sizeof(int), hipMemcpyDeviceToHost));
  int top = 0;
  for (int v : level) top = v > top ? v : top;
  if (last_level < top || last_level >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_curriculum: last_level must lie between the learners' current level and 4; nothing was changed");
  int rc = ens_upload_mdpk5(x); if (rc) return rc;
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) x->rule.ratios[k] = ratios[k];
  x->rule.last_level = last_level; x->rule.advance_exhausted = advance_exhausted;
  x->advance_every = advance_every;
  return DQL_OK;
}
int dql_ensemble_set_level_schedules(dql_ensemble* x, int32_t level, const double* eps, int32_t n_eps, int32_t window, int32_t min_successes, int32_t max_episodes) {
  CHECK_ENS(x);
  if (level < 0 || level >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: the level must be in 0..4");
  if (!eps) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: null table");
  if (n_eps < 1 || n_eps > (1 << 22)) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: the table length must be in 1..2^22");
  if (window < 1 || window > DQL_ENSEMBLE_MAX_WINDOW) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: the promotion window must be in 1..128 (DQL_ENSEMBLE_MAX_WINDOW)");
  if (min_successes < 1 || max_episodes < 1) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: min_successes and max_episodes must be positive");
  for (int i = 0; i < n_eps; ++i) if (!(eps[i] >= 0.0 && eps[i] <= 1.0)) return fail(DQL_EINVAL, "dql_ensemble_set_level_schedules: exploration rates must be in [0, 1]");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> thr((size_t)n_eps);
  for (int i = 0; i < n_eps; ++i) thr[(size_t)i] = eps_threshold(eps[i]);
  uint32_t* d_e = nullptr;
  if (hipMalloc((void**)&d_e, (size_t)n_eps * sizeof(uint32_t)) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc failed");
  LevelSched lv[DQL_MAX_LEVELS];
  for (int k = 0; k < DQL_MAX_LEVELS; ++k) lv[k] = x->h_lv[k];
  lv[level] = LevelSched{d_e, n_eps, window, min_successes, max_episodes};
  if (hipMemcpy(d_e, thr.data(), (size_t)n_eps * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(x->d_lv, lv, sizeof(lv), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d_e);
    return fail(DQL_EHIP, "hipMemcpy failed");
  }
  if (x->h_lv[level].eps_tab) (void)hipFree((void*)x->h_lv[level].eps_tab);
  x->h_lv[level] = lv[level]; x->have_lv[level] = true;
  return DQL_OK;
}
int dql_ensemble_get_levels(dql_ensemble* x, int32_t* level, int32_t* promoted_at, int32_t* episodes_at, int64_t* entered_period) {
  CHECK_ENS(x);
  if (!level || !promoted_at || !episodes_at || !entered_period) return fail(DQL_EINVAL, "dql_ensemble_get_levels: null array");
  HIP_TRY(hipSetDevice(x->device));
  const size_t n = (size_t)x->n;
  HIP_TRY(hipMemcpy(level, x->adv.level, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(promoted_at, x->adv.promoted_at, (size_t)DQL_MAX_LEVELS * n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(episodes_at, x->adv.episodes_at, (size_t)DQL_MAX_LEVELS * n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(entered_period, x->adv.entered_period, (size_t)DQL_MAX_LEVELS * n * sizeof(long long), hipMemcpyDeviceToHost));
  // the level a learner stands on has no history entry yet: its row shows the counters as they are
  std::vector<int> promoted(n), lvl_eps(n);
  HIP_TRY(hipMemcpy(promoted.data(), x->mem.promoted, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(lvl_eps.data(), x->mem.level_episodes, n * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t l = 0; l < n; ++l) {
    const int k = level[l];
    if (k < 0 || k >= DQL_MAX_LEVELS) continue;
    promoted_at[(size_t)k * n + l] = promoted[l]; episodes_at[(size_t)k * n + l] = lvl_eps[l];
  }
  return DQL_OK;
}
int dql_ensemble_n_unfinished(dql_ensemble* x, int64_t* n) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "null pointer");
  if (!x->advance_every) return dql_ensemble_n_live(x, n);
  HIP_TRY(hipSetDevice(x->device));
  std::vector<int> frozen, level, promoted;
  return ens_fetch_levels(x, frozen, level, promoted, n);
}
int dql_ensemble_get_period_index(dql_ensemble* x, int64_t* j) {
  CHECK_ENS(x);
  if (!j) return fail(DQL_EINVAL, "null pointer");
  *j = x->j;
  return DQL_OK;
}
int dql_ensemble_transfer(dql_ensemble* x, int32_t k, double ratio) {
  CHECK_ENS(x);
  if (k < 0 || k >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "dql_ensemble_transfer: curriculum step must be in 0..4");
  HIP_TRY(hipSetDevice(x->device));
  const long long total = x->n * DQL_CELLS_PER_LEVEL;
  hipLaunchKernelGGL(k_ens_transfer, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, x->mem.qa, x->mem.qb, (long long)x->n, (int)k,
                     (int)((k - 1 + DQL_MAX_LEVELS) % DQL_MAX_LEVELS), ratio);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return DQL_OK;
}
static int ens_slice(dql_ensemble* x, int64_t first, int64_t count, const char* who) {
  if (first < 0 || count < 1 || first > x->n || count > x->n - first) return fail(DQL_EINVAL, std::string(who) + ": the slice [first, first + count) must lie inside [0, n_learners) and hold at least one learner");
  return DQL_OK;
}
int dql_ensemble_get_tables(dql_ensemble* x, int64_t first, int64_t count, double* qa_or_null, double* qb_or_null, double* count_or_null) {
  CHECK_ENS(x);
  int rc = ens_slice(x, first, count, "dql_ensemble_get_tables"); if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  const size_t off = (size_t)first * DQL_N_CELLS, bytes = (size_t)count * DQL_N_CELLS * sizeof(double);
  if (qa_or_null) HIP_TRY(hipMemcpy(qa_or_null, x->mem.qa + off, bytes, hipMemcpyDeviceToHost));
  if (qb_or_null) HIP_TRY(hipMemcpy(qb_or_null, x->mem.qb + off, bytes, hipMemcpyDeviceToHost));
  if (count_or_null) HIP_TRY(hipMemcpy(count_or_null, x->mem.count + off, bytes, hipMemcpyDeviceToHost));
  return DQL_OK;
}
int dql_ensemble_set_tables(dql_ensemble* x, int64_t first, int64_t count, const double* qa_or_null, const double* qb_or_null, const double* count_or_null) {
  CHECK_ENS(x);
  int rc = ens_slice(x, first, count, "dql_ensemble_set_tables"); if (rc) return rc;
  if (count_or_null)  // the counters index the learning-rate table on the device
    for (size_t i = 0; i < (size_t)count * DQL_N_CELLS; ++i)
      if (!(count_or_null[i] >= 0.0 && count_or_null[i] < 9007199254740992.0)) return fail(DQL_EINVAL, "dql_ensemble_set_tables: visit counters must be in [0, 2^53)");
  HIP_TRY(hipSetDevice(x->device));
  const size_t off = (size_t)first * DQL_N_CELLS, bytes = (size_t)count * DQL_N_CELLS * sizeof(double);
  if (qa_or_null) HIP_TRY(hipMemcpy(x->mem.qa + off, qa_or_null, bytes, hipMemcpyHostToDevice));
  if (qb_or_null) HIP_TRY(hipMemcpy(x->mem.qb + off, qb_or_null, bytes, hipMemcpyHostToDevice));
  if (count_or_null) HIP_TRY(hipMemcpy(x->mem.count + off, count_or_null, bytes, hipMemcpyHostToDevice));
  return DQL_OK;
}
int dql_ensemble_get_counters(dql_ensemble* x, int64_t* decisions, int64_t* episodes, int64_t* successes, int64_t* by_code, int32_t* promoted, int32_t* level_episodes,
                              uint8_t* frozen) {
  CHECK_ENS(x);
  if (!decisions || !episodes || !successes || !by_code || !promoted || !level_episodes || !frozen) return fail(DQL_EINVAL, "dql_ensemble_get_counters: null array");
  HIP_TRY(hipSetDevice(x->device));
  const size_t n = (size_t)x->n;
  std::vector<int> h(n);
  HIP_TRY(hipMemcpy(decisions, x->mem.decisions, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(by_code, x->mem.by_code, (size_t)DQL_N_CHECK_CODES * n * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h.data(), x->mem.episodes, n * sizeof(int), hipMemcpyDeviceToHost)); for (size_t i = 0; i < n; ++i) episodes[i] = h[i];
  HIP_TRY(hipMemcpy(h.data(), x->mem.successes, n * sizeof(int), hipMemcpyDeviceToHost)); for (size_t i = 0; i < n; ++i) successes[i] = h[i];
  HIP_TRY(hipMemcpy(promoted, x->mem.promoted, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(level_episodes, x->mem.level_episodes, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h.data(), x->mem.frozen, n * sizeof(int), hipMemcpyDeviceToHost)); for (size_t i = 0; i < n; ++i) frozen[i] = h[i] ? 1 : 0;
  return DQL_OK;
}
int dql_ensemble_get_episode_log(dql_ensemble* x, uint8_t* code, uint16_t* length, int32_t capacity, int32_t* n_episodes) {
  CHECK_ENS(x);
  if (!code || !length || !n_episodes) return fail(DQL_EINVAL, "dql_ensemble_get_episode_log: null array");
  if (capacity != x->mem.log_cap || capacity < 1) return fail(DQL_EINVAL, "dql_ensemble_get_episode_log: capacity must be the (positive) log capacity the ensemble was created with");
  HIP_TRY(hipSetDevice(x->device));
  const size_t n = (size_t)x->n * (size_t)capacity;
  HIP_TRY(hipMemcpy(code, x->mem.log_code, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(length, x->mem.log_len, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_episodes, x->mem.log_n, (size_t)x->n * sizeof(int), hipMemcpyDeviceToHost));
  return DQL_OK;
}
int dql_ensemble_get_state(dql_ensemble* x, double* reals, int32_t* ints) {
  CHECK_ENS(x);
  if (!reals || !ints) return fail(DQL_EINVAL, "dql_ensemble_get_state: null array");
  HIP_TRY(hipSetDevice(x->device));
  int rc = x->cfg.dtype == DQL_F32 ? ens_get_state_t<float>(x, reals) : ens_get_state_t<double>(x, reals);
  if (rc) return rc;
  const long long n = x->n;
  std::vector<int4> h((size_t)n);
  HIP_TRY(hipMemcpy(h.data(), x->si, (size_t)n * sizeof(int4), hipMemcpyDeviceToHost));
  for (long long i = 0; i < n; ++i) {
    ints[0 * n + i] = h[i].x; ints[1 * n + i] = h[i].y; ints[2 * n + i] = h[i].z & 0xffff; ints[3 * n + i] = (h[i].z >> 16) & 0xffff;
    ints[4 * n + i] = h[i].w & 0xff; ints[5 * n + i] = (h[i].w >> 8) & 0xff; ints[6 * n + i] = (h[i].w >> 16) & 0xff;
  }
  return DQL_OK;
}
int dql_ensemble_index_faults(dql_ensemble* x, int64_t* n) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(x->device));
  unsigned long long v = 0;
  HIP_TRY(hipMemcpy(&v, x->mem.faults, sizeof(v), hipMemcpyDeviceToHost));
  *n = (int64_t)v;
  return DQL_OK;
}
// the learners' tables are read where they live (the ensemble's device arrays are [L][DQL_N_CELLS] double already): k_score only reads them and touches nothing else of the ensemble
int dql_ensemble_score(dql_ensemble* x, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed,
                       int32_t max_steps, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null) {
  CHECK_ENS(x);
  int rc = check_config(eval_cfg); if (rc) return rc;
  rc = score_check("dql_ensemble_score", count, envs_per_learner, episodes_per_env, max_steps, by_code, steps_sum, ep_code_or_null, ep_steps_or_null); if (rc) return rc;
  if (first < 0 || first > x->n || count > x->n - first) return fail(DQL_EINVAL, "dql_ensemble_score: the slice [first, first + count) must lie inside [0, n_learners); nothing was launched");
  HIP_TRY(hipSetDevice(x->device));
  const size_t off = (size_t)first * DQL_N_CELLS;
  return score_run(eval_cfg, count, envs_per_learner, episodes_per_env, seed, max_steps, x->mem.qa + off, x->mem.qb + off, by_code, steps_sum, ep_code_or_null, ep_steps_or_null);
}
int dql_diag_ensemble_launches(dql_ensemble* x, int64_t* launches, int64_t* periods, int64_t* wave_periods) {
  CHECK_ENS(x);
  if (!launches || !periods || !wave_periods) return fail(DQL_EINVAL, "null pointer");
  *launches = x->n_launches; *periods = x->launched_periods; *wave_periods = x->launched_wave_periods;
  return DQL_OK;
}
int dql_diag_ensemble_last(dql_ensemble* x, double* run_ms) {
  CHECK_ENS(x);
  if (!run_ms) return fail(DQL_EINVAL, "null pointer");
  if (x->last_ms < 0.0) return fail(DQL_ESTATE, "no dql_ensemble_run call has completed on this ensemble");
  *run_ms = x->last_ms;
  return DQL_OK;
}

// ---- resident agent ----
struct dql_agent {
  int device = 0;
  double *qa = nullptr, *qb = nullptr, *count = nullptr;
  hipStream_t stream = nullptr;
  void* pin = nullptr; void* pin_dev = nullptr; size_t pin_bytes = 0;  // pinned + device-visible: arguments in, results out
  // dql_agent_mirror_*: what the device tables hold, as the caller's arrays would have to look ([3][DQL_N_CELLS], pinned), and the answer
  // the last update left for the next predict
  double* shadow = nullptr; bool shadow_valid = false; int shadow_levels = 0;
  int next_idx = -1, next_action = 0;
  unsigned seq = 0;
  void* post = nullptr; void* post_dev = nullptr;  // the mirror calls' own pinned page: [0] AgentOneOut, [64] predict's index, [128] its answer
  // dql_agent_mirror_update_deferred: an update whose kernel is in flight and whose cell has not been patched into the caller's arrays yet
  bool pending = false; double* p_q = nullptr; double* p_count = nullptr; int p_sa = 0, p_t = 0, p_ns = -1; unsigned p_seq = 0;
};
static int mirror_complete(dql_agent* a);
static int agent_pin(dql_agent* a, size_t bytes) {
  if (bytes <= a->pin_bytes) return DQL_OK;
  if (a->pin) { HIP_TRY(hipStreamSynchronize(a->stream)); HIP_TRY(hipHostFree(a->pin)); a->pin = nullptr; a->pin_bytes = 0; }
  bytes = (bytes + 4095) & ~(size_t)4095;
  if (hipHostMalloc(&a->pin, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { a->pin = nullptr; return fail(DQL_ENOMEM, "hipHostMalloc(agent staging) failed"); }
  memset(a->pin, 0, bytes);
  HIP_TRY(hipHostGetDevicePointer(&a->pin_dev, a->pin, 0));
  a->pin_bytes = bytes;
  return DQL_OK;
}
#define CHECK_AGENT(a) do { if (!(a)) return fail(DQL_EINVAL, "null agent"); } while (0)
int dql_agent_create(int device, dql_agent** out) {
  if (!out) return fail(DQL_EINVAL, "null out pointer");
  *out = nullptr;
  OP_PROLOGUE(device)
  dql_agent* a = new dql_agent();
  a->device = device;
  const size_t B = DQL_N_CELLS * sizeof(double);
  int rc = DQL_OK;
  do {
    if (hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(DQL_EHIP, "hipStreamCreate failed"); break; }
    if (hipMalloc((void**)&a->qa, B) != hipSuccess || hipMalloc((void**)&a->qb, B) != hipSuccess || hipMalloc((void**)&a->count, B) != hipSuccess) { rc = fail(DQL_ENOMEM, "hipMalloc failed"); break; }
    if (hipMemsetAsync(a->qa, 0, B, a->stream) != hipSuccess || hipMemsetAsync(a->qb, 0, B, a->stream) != hipSuccess || hipMemsetAsync(a->count, 0, B, a->stream) != hipSuccess) { rc = fail(DQL_EHIP, "hipMemset failed"); break; }
    rc = agent_pin(a, 4096);
    if (rc) break;
    if (hipHostMalloc(&a->post, 4096, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { a->post = nullptr; rc = fail(DQL_ENOMEM, "hipHostMalloc(agent results) failed"); break; }
    memset(a->post, 0, 4096);
    if (hipHostGetDevicePointer(&a->post_dev, a->post, 0) != hipSuccess) { rc = fail(DQL_EHIP, "hipHostGetDevicePointer failed"); break; }
  } while (0);
  if (rc) { const std::string why = g_err; dql_agent_destroy(a); return fail(rc, why); }
  *out = a;
  return DQL_OK;
}
int dql_agent_destroy(dql_agent* a) {
  if (!a) return DQL_OK;
  (void)hipSetDevice(a->device);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  if (a->qa) (void)hipFree(a->qa);
  if (a->qb) (void)hipFree(a->qb);
  if (a->count) (void)hipFree(a->count);
  if (a->pin) (void)hipHostFree(a->pin);
  if (a->shadow) (void)hipHostFree(a->shadow);
  if (a->post) (void)hipHostFree(a->post);
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
  return DQL_OK;
}
int dql_agent_set_tables(dql_agent* a, const double* qa, const double* qb, const double* count) {
  CHECK_AGENT(a);
  { int rc = mirror_complete(a); if (rc) return rc; }
  HIP_TRY(hipSetDevice(a->device));
  const size_t B = DQL_N_CELLS * sizeof(double);
  if (qa) HIP_TRY(hipMemcpyAsync(a->qa, qa, B, hipMemcpyHostToDevice, a->stream));
  if (qb) HIP_TRY(hipMemcpyAsync(a->qb, qb, B, hipMemcpyHostToDevice, a->stream));
  if (count) HIP_TRY(hipMemcpyAsync(a->count, count, B, hipMemcpyHostToDevice, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));  // the caller's arrays may change right after return
  a->shadow_valid = false; a->next_idx = -1;
  return DQL_OK;
}
int dql_agent_get_tables(dql_agent* a, double* qa, double* qb, double* count) {
  CHECK_AGENT(a);
  { int rc = mirror_complete(a); if (rc) return rc; }
  HIP_TRY(hipSetDevice(a->device));
  const size_t B = DQL_N_CELLS * sizeof(double);
  if (qa) HIP_TRY(hipMemcpyAsync(qa, a->qa, B, hipMemcpyDeviceToHost, a->stream));
  if (qb) HIP_TRY(hipMemcpyAsync(qb, a->qb, B, hipMemcpyDeviceToHost, a->stream));
  if (count) HIP_TRY(hipMemcpyAsync(count, a->count, B, hipMemcpyDeviceToHost, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  return DQL_OK;
}
int dql_agent_predict_resident(dql_agent* a, const int32_t* idx, int64_t n, uint8_t* action_out) {
  CHECK_AGENT(a);
  { int rc = mirror_complete(a); if (rc) return rc; }
  if (n < 0 || (n > 0 && (!idx || !action_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  for (int64_t i = 0; i < n; ++i) if (idx[i] < 0 || idx[i] >= DQL_N_STATES) return fail(DQL_EINVAL, "state index out of range");
  HIP_TRY(hipSetDevice(a->device));
  const size_t in_b = ((size_t)n * sizeof(int32_t) + 63) & ~(size_t)63;
  { int rc = agent_pin(a, in_b + (size_t)n); if (rc) return rc; }
  memcpy(a->pin, idx, (size_t)n * sizeof(int32_t));
  hipLaunchKernelGGL(k_predict_resident, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a->stream, (const double*)a->qa, (const double*)a->qb, (const int*)a->pin_dev, (long long)n,
                     (uint8_t*)a->pin_dev + in_b);
  HIP_TRY(hipGetLastError());
  HIP_TRY(wait_stream(a->stream));
  memcpy(action_out, (const char*)a->pin + in_b, (size_t)n);
  return DQL_OK;
}
int dql_agent_update_resident(dql_agent* a, const int32_t* sa, const int32_t* ns, const double* alpha, double gamma, const double* reward, int64_t n,
                              uint32_t quirks, const uint8_t* coin, const uint8_t* done, double* q_new, double* count_new, uint8_t* next_action) {
  CHECK_AGENT(a);
  { int rc = mirror_complete(a); if (rc) return rc; }
  if (n < 0 || (n > 0 && (!sa || !ns || !alpha || !reward))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  if (!(quirks & DQL_Q_UPDATE_TABLE_A_ONLY) && !coin) return fail(DQL_EINVAL, "Double Q-learning (DQL_Q_UPDATE_TABLE_A_ONLY cleared) needs the caller's coin per transition");
  if (!(quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) && !done) return fail(DQL_EINVAL, "bootstrapping on non-terminal transitions (DQL_Q_BOOTSTRAP_ON_POS_CHANGE cleared) needs the done flags");
  for (int64_t i = 0; i < n; ++i) if (sa[i] < 0 || sa[i] >= DQL_N_CELLS || ns[i] < 0 || ns[i] >= DQL_N_STATES) return fail(DQL_EINVAL, "index out of range");
  HIP_TRY(hipSetDevice(a->device));
  const size_t in_b = (size_t)n * sizeof(AgentUpdIn);
  { int rc = agent_pin(a, in_b + (size_t)n * sizeof(AgentUpdOut) + sizeof(AgentUpdTail)); if (rc) return rc; }
  AgentUpdIn* in = (AgentUpdIn*)a->pin;
  for (int64_t i = 0; i < n; ++i) in[i] = AgentUpdIn{sa[i], ns[i], alpha[i], reward[i], coin ? (int)coin[i] : 0, done ? (int)done[i] : 0};
  hipLaunchKernelGGL(k_update_resident, dim3(1), dim3(64), 0, a->stream, a->qa, a->qb, a->count, (const AgentUpdIn*)a->pin_dev, (AgentUpdOut*)((char*)a->pin_dev + in_b), (long long)n, gamma, quirks);
  HIP_TRY(hipGetLastError());
  HIP_TRY(wait_stream(a->stream));
  const AgentUpdOut* o = (const AgentUpdOut*)((const char*)a->pin + in_b);
  for (int64_t i = 0; i < n; ++i) { if (q_new) q_new[i] = o[i].q_new; if (count_new) count_new[i] = o[i].count_new; }
  if (next_action) *next_action = (uint8_t)((const AgentUpdTail*)(o + n))->next_action;
  a->shadow_valid = false; a->next_idx = -1;
  return DQL_OK;
}
// ---- host-mirrored single transitions ----
// brings the device tables up to the caller's arrays; what changed is found by comparing with the shadow of the last upload
// a deferred update's second half: wait for its kernel (it has usually finished while the caller was busy), patch the one cell and its visit counter into
// the caller's arrays and into the shadow, keep the kernel's answer for the next predict
static int mirror_complete(dql_agent* a) {
  if (!a->pending) return DQL_OK;
  a->pending = false;
  HIP_TRY(hipSetDevice(a->device));
  AgentOneOut* o = (AgentOneOut*)a->post;
  if (!wait_posted(&o->seq, a->p_seq)) HIP_TRY(wait_stream(a->stream));
  a->p_q[a->p_sa] = o->q_new; a->p_count[a->p_sa] = o->count_new;
  a->shadow[(size_t)a->p_t * DQL_N_CELLS + a->p_sa] = o->q_new; a->shadow[(size_t)2 * DQL_N_CELLS + a->p_sa] = o->count_new;
  a->next_idx = a->p_ns; a->next_action = o->next_action;
  return DQL_OK;
}
static int mirror_refresh(dql_agent* a, const double* qa, const double* qb, const double* count, int32_t n_levels) {
  if (!qa || !qb || !count) return fail(DQL_EINVAL, "null table");
  { int rc = mirror_complete(a); if (rc) return rc; }
  if (n_levels < 1 || n_levels > DQL_MAX_LEVELS) return fail(DQL_EINVAL, "n_levels must be in 1..5");
  HIP_TRY(hipSetDevice(a->device));
  const size_t B = DQL_N_CELLS * sizeof(double), used = (size_t)n_levels * DQL_STATES_PER_LEVEL * 3 * sizeof(double);
  if (!a->shadow) {
    if (hipHostMalloc((void**)&a->shadow, 3 * B, hipHostMallocDefault) != hipSuccess) { a->shadow = nullptr; return fail(DQL_ENOMEM, "hipHostMalloc(table shadow) failed"); }
    a->shadow_valid = false;
  }
  const double* host[3] = {qa, qb, count};
  double* dev[3] = {a->qa, a->qb, a->count};
  bool sent = false;
  for (int t = 0; t < 3; ++t) {
    double* sh = a->shadow + (size_t)t * DQL_N_CELLS;
    if (a->shadow_valid && a->shadow_levels == n_levels && memcmp(sh, host[t], used) == 0) continue;
    memcpy(sh, host[t], used);
    memset((char*)sh + used, 0, B - used);
    HIP_TRY(hipMemcpyAsync(dev[t], sh, B, hipMemcpyHostToDevice, a->stream));
    sent = true;
  }
  if (sent) { HIP_TRY(hipStreamSynchronize(a->stream)); a->next_idx = -1; }  // the shadow may be patched right after return
  a->shadow_valid = true; a->shadow_levels = n_levels;
  return DQL_OK;
}
int dql_agent_mirror_predict(dql_agent* a, const double* qa, const double* qb, const double* count, int32_t n_levels, int32_t idx, uint8_t* action_out) {
  CHECK_AGENT(a);
  if (!action_out) return fail(DQL_EINVAL, "null action_out");
  { int rc = mirror_refresh(a, qa, qb, count, n_levels); if (rc) return rc; }
  if (idx < 0 || idx >= n_levels * DQL_STATES_PER_LEVEL) return fail(DQL_EINVAL, "state index outside the table's levels");
  if (idx == a->next_idx) { *action_out = (uint8_t)a->next_action; return DQL_OK; }  // the last update's kernel answered this on the tables as they are
  *(int*)((char*)a->post + 64) = idx;
  hipLaunchKernelGGL(k_predict_resident, dim3(1), dim3(64), 0, a->stream, (const double*)a->qa, (const double*)a->qb, (const int*)((char*)a->post_dev + 64), 1ll, (uint8_t*)a->post_dev + 128);
  HIP_TRY(hipGetLastError());
  HIP_TRY(wait_stream(a->stream));
  *action_out = *((const uint8_t*)a->post + 128);
  return DQL_OK;
}
int dql_agent_mirror_update_deferred(dql_agent* a, double* qa, double* qb, double* count, int32_t n_levels, int32_t sa, int32_t ns, double alpha, double gamma,
                                     double reward, uint32_t quirks, int32_t coin, int32_t done) {
  CHECK_AGENT(a);
  { int rc = mirror_refresh(a, qa, qb, count, n_levels); if (rc) return rc; }
  if (sa < 0 || sa >= n_levels * DQL_STATES_PER_LEVEL * 3 || ns < 0 || ns >= n_levels * DQL_STATES_PER_LEVEL) return fail(DQL_EINVAL, "index outside the table's levels");
  const unsigned seq = ++a->seq;
  hipLaunchKernelGGL(k_update_one, dim3(1), dim3(64), 0, a->stream, a->qa, a->qb, a->count, (int)sa, (int)ns, alpha, gamma, reward, quirks, (int)coin, (int)done, (AgentOneOut*)a->post_dev, seq);
  HIP_TRY(hipGetLastError());
  const int t = (!(quirks & DQL_Q_UPDATE_TABLE_A_ONLY) && coin) ? 1 : 0;  // the table agent_update_one writes
  a->pending = true; a->p_q = t ? qb : qa; a->p_count = count; a->p_sa = sa; a->p_t = t; a->p_ns = ns; a->p_seq = seq;
  a->next_idx = -1;  // (the device tables are ahead of the caller's arrays until mirror_complete)
  return DQL_OK;
}
int dql_agent_mirror_complete(dql_agent* a) {
  CHECK_AGENT(a);
  return mirror_complete(a);
}
int dql_agent_mirror_update(dql_agent* a, double* qa, double* qb, double* count, int32_t n_levels, int32_t sa, int32_t ns, double alpha, double gamma,
                            double reward, uint32_t quirks, int32_t coin, int32_t done) {
  const int rc = dql_agent_mirror_update_deferred(a, qa, qb, count, n_levels, sa, ns, alpha, gamma, reward, quirks, coin, done);
  return rc ? rc : mirror_complete(a);
}

int dql_agent_transfer(int device, double* qa, double* qb, int32_t k, double ratio) {
  if (!qa || !qb) return fail(DQL_EINVAL, "null array");
  if (k < 0 || k >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "curriculum step must be in 0..4");
  OP_PROLOGUE(device)
  DevBuf a, b;
  const size_t B = DQL_N_CELLS * sizeof(double);
  UP(a, qa, B); UP(b, qb, B);
  hipLaunchKernelGGL(k_transfer, dim3((DQL_CELLS_PER_LEVEL + 255) / 256), dim3(256), 0, 0, (double*)a.p, (double*)b.p, (int)k, (int)((k - 1 + DQL_MAX_LEVELS) % DQL_MAX_LEVELS), ratio);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(qa, a.p, B, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(qb, b.p, B, hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_agent_predict(int device, const double* qa, const double* qb, const int32_t* idx, int64_t n, uint8_t* action_out) {
  if (n < 0 || !qa || !qb || (n > 0 && (!idx || !action_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  for (int64_t i = 0; i < n; ++i) if (idx[i] < 0 || idx[i] >= DQL_N_STATES) return fail(DQL_EINVAL, "state index out of range");
  OP_PROLOGUE(device)
  DevBuf a, b, ix, o;
  UP(a, qa, DQL_N_CELLS * sizeof(double)); UP(b, qb, DQL_N_CELLS * sizeof(double)); UP(ix, idx, (size_t)n * sizeof(int));
  if (o.alloc((size_t)n)) return fail(DQL_ENOMEM, "hipMalloc failed");
  hipLaunchKernelGGL(k_predict, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double*)a.p, (const double*)b.p, (const int*)ix.p, (long long)n, (uint8_t*)o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(action_out, o.p, (size_t)n, hipMemcpyDeviceToHost));
  return DQL_OK;
}

int dql_agent_update(int device, double* qa, double* qb, double* count, const int32_t* sa, const int32_t* ns, const double* alpha, double gamma,
                     const double* reward, int64_t n, uint32_t quirks, const uint8_t* coin, const uint8_t* done) {
  if (n < 0 || !qa || !qb || !count || (n > 0 && (!sa || !ns || !alpha || !reward))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  if (!(quirks & DQL_Q_UPDATE_TABLE_A_ONLY) && !coin) return fail(DQL_EINVAL, "Double Q-learning (DQL_Q_UPDATE_TABLE_A_ONLY cleared) needs the caller's coin per transition");
  if (!(quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) && !done) return fail(DQL_EINVAL, "bootstrapping on non-terminal transitions (DQL_Q_BOOTSTRAP_ON_POS_CHANGE cleared) needs the done flags");
  for (int64_t i = 0; i < n; ++i) if (sa[i] < 0 || sa[i] >= DQL_N_CELLS || ns[i] < 0 || ns[i] >= DQL_N_STATES) return fail(DQL_EINVAL, "index out of range");
  OP_PROLOGUE(device)
  DevBuf a, b, c, s, t, al, rw, cn, dn;
  const size_t B = DQL_N_CELLS * sizeof(double);
  UP(a, qa, B); UP(b, qb, B); UP(c, count, B); UP(s, sa, (size_t)n * sizeof(int)); UP(t, ns, (size_t)n * sizeof(int)); UP(al, alpha, (size_t)n * sizeof(double)); UP(rw, reward, (size_t)n * sizeof(double));
  if (coin) UP(cn, coin, (size_t)n);
  if (done) UP(dn, done, (size_t)n);
  hipLaunchKernelGGL(k_update_seq, dim3(1), dim3(64), 0, 0, (double*)a.p, (double*)b.p, (double*)c.p, (const int*)s.p, (const int*)t.p, (const double*)al.p, gamma, (const double*)rw.p, (long long)n, quirks,
                     (const uint8_t*)cn.p, (const uint8_t*)dn.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(qa, a.p, B, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(qb, b.p, B, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(count, c.p, B, hipMemcpyDeviceToHost));
  return DQL_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// RCCL communicator.  librccl.so is half a gigabyte: it is loaded with dlopen the first time a
// communicator is asked for, so a single-GPU process never maps it.
// ---------------------------------------------------------------------------------------------
struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;
static int load_rccl() {
  if (g_rccl.handle) return DQL_OK;
  const char* env = getenv("DQL_RCCL_PATH");
  const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  std::string tried;
  for (const char* nm : names) {
    if (!nm || !*nm) continue;
    h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
    if (h) break;
    tried += std::string(" ") + nm + " (" + dlerror() + ")";
  }
  if (!h) return fail(DQL_ERCCL, "cannot load librccl:" + tried);
#define DQL_SYM(field, name) do { *(void**)(&g_rccl.field) = dlsym(h, name); if (!g_rccl.field) { dlclose(h); return fail(DQL_ERCCL, std::string("librccl lacks ") + name); } } while (0)
  DQL_SYM(GetUniqueId, "ncclGetUniqueId"); DQL_SYM(CommInitRank, "ncclCommInitRank"); DQL_SYM(CommDestroy, "ncclCommDestroy");
  DQL_SYM(AllReduce, "ncclAllReduce"); DQL_SYM(AllGather, "ncclAllGather"); DQL_SYM(GetErrorString, "ncclGetErrorString");
#undef DQL_SYM
  g_rccl.handle = h;
  return DQL_OK;
}
#define NCCL_TRY(expr)                                                                                         \
  do {                                                                                                         \
    ncclResult_t _r = (expr);                                                                                  \
    if (_r != ncclSuccess) return fail(DQL_ERCCL, std::string(#expr) + ": " + g_rccl.GetErrorString(_r));      \
  } while (0)

struct dql_comm {
  int device = 0, rank = 0, world = 1;
  ncclComm_t nccl = nullptr;
  hipStream_t stream = nullptr;
  void* stage = nullptr;  // device staging of the host-buffer collectives
  size_t stage_bytes = 0;
};
static int comm_stage(dql_comm* c, size_t bytes) {
  if (bytes <= c->stage_bytes) return DQL_OK;
  if (c->stage) { HIP_TRY(hipFree(c->stage)); c->stage = nullptr; c->stage_bytes = 0; }
  bytes = (bytes + 4095) & ~(size_t)4095;
  if (hipMalloc(&c->stage, bytes) != hipSuccess) { c->stage = nullptr; return fail(DQL_ENOMEM, "hipMalloc(comm staging) failed"); }
  c->stage_bytes = bytes;
  return DQL_OK;
}
#define CHECK_COMM(c) do { if (!(c)) return fail(DQL_EINVAL, "null communicator"); } while (0)

extern "C" {

int dql_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(DQL_EINVAL, "null pointer");
  static_assert(sizeof(ncclUniqueId) == DQL_COMM_ID_BYTES, "DQL_COMM_ID_BYTES must be the size of ncclUniqueId");
  { int rc = load_rccl(); if (rc) return rc; }
  ncclUniqueId id;
  NCCL_TRY(g_rccl.GetUniqueId(&id));
  memcpy(id_out, &id, sizeof(id));
  return DQL_OK;
}
int dql_comm_create(int device, int32_t rank, int32_t world, const uint8_t* id, dql_comm** out) {
  if (!out) return fail(DQL_EINVAL, "null out pointer");
  *out = nullptr;
  if (!id) return fail(DQL_EINVAL, "null unique id");
  if (world < 1 || rank < 0 || rank >= world) return fail(DQL_EINVAL, "rank must be in 0 .. world-1");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(DQL_EHIP, "no HIP device visible (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(DQL_EINVAL, "device index out of range");
  { int rc = load_rccl(); if (rc) return rc; }
  HIP_TRY(hipSetDevice(device));
  dql_comm* c = new dql_comm();
  c->device = device; c->rank = rank; c->world = world;
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  int rc = DQL_OK;
  do {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(DQL_EHIP, "hipStreamCreate failed"); break; }
    // RCCL 2.27 prints a version banner on STDOUT from ncclCommInitRank (no switch for it): a launcher that reads one result line
    // from rank 0's stdout must not find it there.  Park fd 1 on stderr for the duration of the call (one host thread per
    // process talks to this library while a communicator is created).
    fflush(stdout);
    const int saved_out = dup(1);
    if (saved_out >= 0) (void)dup2(2, 1);
    const ncclResult_t r = g_rccl.CommInitRank(&c->nccl, world, uid, rank);
    fflush(stdout);
    if (saved_out >= 0) { (void)dup2(saved_out, 1); (void)close(saved_out); }
    if (r != ncclSuccess) { c->nccl = nullptr; rc = fail(DQL_ERCCL, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); break; }
  } while (0);
  if (rc) { const std::string why = g_err; dql_comm_destroy(c); return fail(rc, why); }
  *out = c;
  return DQL_OK;
}
int dql_comm_destroy(dql_comm* c) {
  if (!c) return DQL_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->nccl) (void)g_rccl.CommDestroy(c->nccl);
  if (c->stage) (void)hipFree(c->stage);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return DQL_OK;
}
int dql_comm_info(dql_comm* c, int32_t* rank, int32_t* world, int32_t* device) {
  CHECK_COMM(c);
  if (rank) *rank = c->rank;
  if (world) *world = c->world;
  if (device) *device = c->device;
  return DQL_OK;
}
static int comm_allreduce(dql_comm* c, void* inout, int64_t n, ncclDataType_t dt, int32_t op) {
  CHECK_COMM(c);
  if (n < 0 || (n > 0 && !inout)) return fail(DQL_EINVAL, "null array");
  if (op != DQL_OP_SUM && op != DQL_OP_MAX) return fail(DQL_EINVAL, "op must be DQL_OP_SUM or DQL_OP_MAX");
  if (n == 0) return DQL_OK;
  const size_t bytes = (size_t)n * 8;
  HIP_TRY(hipSetDevice(c->device));
  { int rc = comm_stage(c, bytes); if (rc) return rc; }
  HIP_TRY(hipMemcpyAsync(c->stage, inout, bytes, hipMemcpyHostToDevice, c->stream));
  NCCL_TRY(g_rccl.AllReduce(c->stage, c->stage, (size_t)n, dt, op == DQL_OP_SUM ? ncclSum : ncclMax, c->nccl, c->stream));
  HIP_TRY(hipMemcpyAsync(inout, c->stage, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DQL_OK;
}
int dql_comm_allreduce_f64(dql_comm* c, double* inout, int64_t n, int32_t op) { return comm_allreduce(c, inout, n, ncclDouble, op); }
int dql_comm_allreduce_i64(dql_comm* c, int64_t* inout, int64_t n, int32_t op) { return comm_allreduce(c, inout, n, ncclInt64, op); }
int dql_comm_allgather_u64(dql_comm* c, const uint64_t* in, int64_t n, uint64_t* out) {
  CHECK_COMM(c);
  if (n < 0 || (n > 0 && (!in || !out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  const size_t bytes = (size_t)n * 8;
  HIP_TRY(hipSetDevice(c->device));
  { int rc = comm_stage(c, bytes * (size_t)(c->world + 1)); if (rc) return rc; }
  char* send = (char*)c->stage;
  char* recv = send + bytes;
  HIP_TRY(hipMemcpyAsync(send, in, bytes, hipMemcpyHostToDevice, c->stream));
  NCCL_TRY(g_rccl.AllGather(send, recv, (size_t)n, ncclUint64, c->nccl, c->stream));
  HIP_TRY(hipMemcpyAsync(out, recv, bytes * (size_t)c->world, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DQL_OK;
}
int dql_comm_barrier(dql_comm* c) {
  int64_t one = 1;
  return dql_comm_allreduce_i64(c, &one, 1, DQL_OP_SUM);
}

int dql_attach_comm(dql_ctx* x, dql_comm* c) {
  POP_NEVER(x, "dql_attach_comm");
  CHECK_CTX(x);
  if (c && c->device != x->device) return fail(DQL_EINVAL, "communicator and context live on different devices");
  x->comm = c;
  return DQL_OK;
}
int dql_allreduce_window(dql_ctx* x) {
  POP_NEVER(x, "dql_allreduce_window");
  CHECK_CTX(x);
  if (!x->comm) return fail(DQL_ESTATE, "dql_allreduce_window: no communicator attached (dql_attach_comm)");
  if (!x->windowed) return fail(DQL_ESTATE, "dql_allreduce_window needs windowed accumulation (dql_set_windowed)");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }  // the last launch's accumulators enter the window here
  if (x->kernel_timer) {
    if (x->sev.size() & 1) { (void)hipEventDestroy(x->sev.back()); x->sev.pop_back(); }  // an exchange that was never folded
    hipEvent_t e0 = nullptr;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventRecord(e0, x->stream)); x->sev.push_back(e0);
  }
  NCCL_TRY(g_rccl.AllReduce(x->window, x->window, (size_t)DQL_ACC_LEN, ncclInt64, ncclSum, x->comm->nccl, x->stream));
  return DQL_OK;
}

// ---- one-shot peer-to-peer exchange ----
int dql_p2p_create(dql_ctx* x, int32_t rank, int32_t world, uint8_t* handle_out) {
  POP_NEVER(x, "dql_p2p_create");
  CHECK_CTX(x);
  if (!handle_out) return fail(DQL_EINVAL, "null pointer");
  static_assert(sizeof(hipIpcMemHandle_t) == DQL_P2P_HANDLE_BYTES, "DQL_P2P_HANDLE_BYTES must be the size of hipIpcMemHandle_t");
  if (world < 1 || world > DQL_P2P_MAX_RANKS || rank < 0 || rank >= world) return fail(DQL_EINVAL, "rank must be in 0 .. world-1, world at most DQL_P2P_MAX_RANKS");
  if (x->p2p_buf) return fail(DQL_ESTATE, "dql_p2p_create: this context already has an exchange buffer");
  HIP_TRY(hipSetDevice(x->device));
  const size_t words = (size_t)2 * world * DQL_ACC_LEN + (size_t)2 * DQL_P2P_MAX_RANKS;
  if (hipExtMallocWithFlags((void**)&x->p2p_buf, words * sizeof(unsigned long long), hipDeviceMallocUncached) != hipSuccess) { x->p2p_buf = nullptr; return fail(DQL_ENOMEM, "hipExtMallocWithFlags(exchange buffer) failed"); }
  if (hipMalloc((void**)&x->p2p_status, 2 * sizeof(unsigned long long)) != hipSuccess) { x->p2p_status = nullptr; return fail(DQL_ENOMEM, "hipMalloc failed"); }
  HIP_TRY(hipMemsetAsync(x->p2p_buf, 0, words * sizeof(unsigned long long), x->stream));
  HIP_TRY(hipMemsetAsync(x->p2p_status, 0, 2 * sizeof(unsigned long long), x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  hipIpcMemHandle_t h;
  {
    const hipError_t e = hipIpcGetMemHandle(&h, x->p2p_buf);
    if (e != hipSuccess) return fail(DQL_EHIP, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e) + " (ranks sharing one GPU need HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment before the first HIP call)");
  }
  memcpy(handle_out, &h, sizeof(h));
  x->p2p_rank = rank; x->p2p_world = world; x->p2p_seq = 0;
  x->p2p_peer[rank] = x->p2p_buf;
  return DQL_OK;
}
int dql_p2p_connect(dql_ctx* x, const uint8_t* all_handles) {
  POP_NEVER(x, "dql_p2p_connect");
  CHECK_CTX(x);
  if (!all_handles) return fail(DQL_EINVAL, "null pointer");
  if (!x->p2p_buf) return fail(DQL_ESTATE, "dql_p2p_connect: call dql_p2p_create first");
  HIP_TRY(hipSetDevice(x->device));
  for (int r = 0; r < x->p2p_world; ++r) {
    if (r == x->p2p_rank || x->p2p_opened[r] || x->p2p_peer[r]) continue;  // itself, mapped already, or connected by pointer (same process)
    hipIpcMemHandle_t h;
    memcpy(&h, all_handles + (size_t)r * DQL_P2P_HANDLE_BYTES, sizeof(h));
    void* ptr = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(DQL_EHIP, std::string("hipIpcOpenMemHandle(rank ") + std::to_string(r) + "): " + hipGetErrorString(e));
    x->p2p_peer[r] = (unsigned long long*)ptr; x->p2p_opened[r] = true;
  }
  return DQL_OK;
}
int dql_p2p_connect_local(dql_ctx* x, dql_ctx* const* peers) {
  POP_NEVER(x, "dql_p2p_connect_local");
  CHECK_CTX(x);
  if (!peers) return fail(DQL_EINVAL, "null pointer");
  if (!x->p2p_buf) return fail(DQL_ESTATE, "dql_p2p_connect_local: call dql_p2p_create first");
  HIP_TRY(hipSetDevice(x->device));
  for (int r = 0; r < x->p2p_world; ++r) {
    dql_ctx* pr = peers[r];
    if (!pr || r == x->p2p_rank) continue;
    if (!pr->p2p_buf || pr->p2p_rank != r || pr->p2p_world != x->p2p_world) return fail(DQL_EINVAL, "dql_p2p_connect_local: peers[r] must be the context that called dql_p2p_create(rank r, same world)");
    if (pr->device != x->device) {
      const hipError_t e = hipDeviceEnablePeerAccess(pr->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(DQL_EHIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
      (void)hipGetLastError();
    }
    x->p2p_peer[r] = pr->p2p_buf;
  }
  return DQL_OK;
}
static int p2p_ready(dql_ctx* x, const char* who) {
  if (!x->p2p_buf) return fail(DQL_ESTATE, std::string(who) + ": no exchange buffer (dql_p2p_create / dql_p2p_connect)");
  if (!x->windowed) return fail(DQL_ESTATE, std::string(who) + " needs windowed accumulation (dql_set_windowed)");
  for (int r = 0; r < x->p2p_world; ++r) if (!x->p2p_peer[r]) return fail(DQL_ESTATE, std::string(who) + ": not connected to every peer (dql_p2p_connect / dql_p2p_connect_local)");
  return DQL_OK;
}
static P2PPushArgs p2p_args(dql_ctx* x, unsigned long long seq) {
  P2PPushArgs a;
  a.window = x->window; a.rank = x->p2p_rank; a.world = x->p2p_world; a.parity = (int)(seq & 1);
  for (int r = 0; r < DQL_P2P_MAX_RANKS; ++r) a.peer[r] = r < x->p2p_world ? x->p2p_peer[r] : nullptr;
  return a;
}
int dql_p2p_push_window(dql_ctx* x) {
  POP_NEVER(x, "dql_p2p_push_window");
  CHECK_CTX(x);
  { int rc = p2p_ready(x, "dql_p2p_push_window"); if (rc) return rc; }
  if (x->p2p_pushed) return fail(DQL_ESTATE, "dql_p2p_push_window: the previous push has not been waited for (dql_p2p_wait_window)");
  HIP_TRY(hipSetDevice(x->device));
  { int rc = flush_pending(x); if (rc) return rc; }  // the last launch's accumulators enter the window here
  if (x->kernel_timer) {
    if (x->sev.size() & 1) { (void)hipEventDestroy(x->sev.back()); x->sev.pop_back(); }
    hipEvent_t e0 = nullptr;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventRecord(e0, x->stream)); x->sev.push_back(e0);
  }
  const unsigned long long seq = ++x->p2p_seq;
  const P2PPushArgs a = p2p_args(x, seq);
  const int B = 256, G = (DQL_ACC_LEN + B - 1) / B;
  hipLaunchKernelGGL(k_p2p_push, dim3(G), dim3(B), 0, x->stream, a);
  hipLaunchKernelGGL(k_p2p_signal, dim3(1), dim3(64), 0, x->stream, a, seq);
  HIP_TRY(hipGetLastError());
  x->p2p_pushed = true;
  return DQL_OK;
}
int dql_p2p_wait_window(dql_ctx* x) {
  POP_NEVER(x, "dql_p2p_wait_window");
  CHECK_CTX(x);
  { int rc = p2p_ready(x, "dql_p2p_wait_window"); if (rc) return rc; }
  if (!x->p2p_pushed) return fail(DQL_ESTATE, "dql_p2p_wait_window: nothing pushed (dql_p2p_push_window)");
  HIP_TRY(hipSetDevice(x->device));
  const unsigned long long seq = x->p2p_seq;
  const int parity = (int)(seq & 1);
  const int B = 256, G = (DQL_ACC_LEN + B - 1) / B;
  hipLaunchKernelGGL(k_p2p_wait, dim3(1), dim3(64), 0, x->stream, (const unsigned long long*)x->p2p_buf, x->p2p_world, parity, seq, x->p2p_status, x->p2p_spin_limit);
  hipLaunchKernelGGL(k_p2p_sum, dim3(G), dim3(B), 0, x->stream, x->p2p_buf, x->window, x->p2p_world, parity, seq, (const unsigned long long*)x->p2p_status);
  HIP_TRY(hipGetLastError());
  x->p2p_pushed = false;
  return DQL_OK;
}
int dql_p2p_exchange_window(dql_ctx* x) {
  POP_NEVER(x, "dql_p2p_exchange_window");
  const int rc = dql_p2p_push_window(x);
  return rc ? rc : dql_p2p_wait_window(x);
}
int dql_p2p_status(dql_ctx* x, int32_t* failed_seq) {
  CHECK_CTX(x);
  if (!failed_seq) return fail(DQL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(x->device));
  unsigned long long v = 0;
  { int rc = p2p_failed_seq(x, &v); if (rc) return rc; }
  *failed_seq = (int32_t)(v > 0x7fffffffull ? 0x7fffffffull : v);
  return DQL_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// populations (include/dql.h dql_pop_*)
// ---------------------------------------------------------------------------------------------
static int pop_agent(dql_ctx* x, int32_t k, dql_ctx** g) {
  CHECK_CTX(x);
  if (!x->n_agents) return fail(DQL_EINVAL, "not a population context (dql_pop_create)");
  if (k < 0 || k >= x->n_agents) return fail(DQL_EINVAL, "agent index out of range");
  HIP_TRY(hipSetDevice(x->device));
  *g = x->agents[k];
  return DQL_OK;
}
template <typename T> static int launch_init_agent(dql_ctx* x, int k) {
  // k_init over agent k's E envs alone: the state arrays keep the population's stride (n = K E), the base moves to the agent's first env, and the grid
  // is exactly E threads (E is a multiple of 512), so that no thread reaches past the agent's slice
  const dql_ctx* g = x->agents[k];
  InitArgs<T> a;
  a.c = make_simk<T>(x->cfg);
  a.sr = (Quad<T>*)x->sr + k * x->pop_E; a.si = x->si + k * x->pop_E; a.n = x->n; a.seed = g->seed; a.env_id_offset = 0;
  const dql_config& c = x->cfg;
  a.hover = std::sqrt((T)(c.mass * c.gravity / (4.0 * c.k_f)));
  a.vz_integ = (T)(c.mass * c.gravity / c.pid_vz[1]);
  a.r_lo = (T)c.mp_r_lo; a.r_hi = (T)c.mp_r_hi; a.t_lo = (T)c.mp_t_lo; a.t_hi = (T)c.mp_t_hi;
  const int B = 256;
  hipLaunchKernelGGL(k_init<T>, dim3((unsigned)(x->pop_E / B)), dim3(B), 0, x->stream, a);
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}
static int pop_create_impl(dql_ctx* x, const uint64_t* seeds) {
  int rc = create_impl(x, &x->cfg);
  if (rc) return rc;
  for (int k = 0; k < x->n_agents; ++k) {
    dql_ctx* g = new dql_ctx();
    x->agents.push_back(g);
    g->cfg = x->cfg; g->device = x->device; g->n = x->pop_E; g->seed = seeds[k]; g->env_id_offset = 0; g->dtype = x->dtype; g->real_size = x->real_size;
    g->stream = x->stream; g->owns_stream = false; g->n_simds = x->n_simds; g->kal_fix = x->kal_fix; g->lit_ok = x->lit_ok; g->litm_ok = x->litm_ok;
    rc = create_tables(g);
    if (rc) return rc;
    const double a0 = x->cfg.alpha_min;
    rc = dql_set_alpha_table(g, &a0, 1);
    if (rc) return rc;
    rc = x->dtype == DQL_F32 ? launch_init_agent<float>(x, k) : launch_init_agent<double>(x, k);
    if (rc) return rc;
  }
  const size_t ring = (size_t)DQL_POP_RING * DQL_MAX_AGENTS * sizeof(PopAgentDesc);
  if (hipHostMalloc((void**)&x->pop_h, ring, hipHostMallocDefault) != hipSuccess) { x->pop_h = nullptr; return fail(DQL_ENOMEM, "hipHostMalloc(launch descriptors) failed"); }
  if (hipMalloc((void**)&x->pop_d, ring) != hipSuccess) { x->pop_d = nullptr; return fail(DQL_ENOMEM, "hipMalloc(launch descriptors) failed"); }
  if (hipMalloc((void**)&x->pop_faults, (size_t)x->n_agents * sizeof(unsigned long long)) != hipSuccess) { x->pop_faults = nullptr; return fail(DQL_ENOMEM, "hipMalloc(fault counters) failed"); }
  HIP_TRY(hipMemsetAsync(x->pop_faults, 0, (size_t)x->n_agents * sizeof(unsigned long long), x->stream));
  for (int s = 0; s < DQL_POP_RING; ++s) HIP_TRY(hipEventCreateWithFlags(&x->pop_ev[s], hipEventDisableTiming));
  HIP_TRY(hipStreamSynchronize(x->stream));
  return DQL_OK;
}

extern "C" {

int dql_pop_create(const dql_config* cfg, int device, int32_t n_agents, int64_t envs_per_agent, const uint64_t* seeds, dql_ctx** out) {
  if (!out) return fail(DQL_EINVAL, "null out pointer");
  *out = nullptr;
  int rc = check_config(cfg);
  if (rc) return rc;
  if (n_agents < 1 || n_agents > DQL_MAX_AGENTS) return fail(DQL_EINVAL, "n_agents must be in 1..16 (DQL_MAX_AGENTS)");
  if (envs_per_agent < 512 || envs_per_agent % 512) return fail(DQL_EINVAL, "envs_per_agent must be a positive multiple of 512 (a workgroup of any size then holds one agent)");
  if ((long long)n_agents * envs_per_agent > (1ll << 31)) return fail(DQL_EINVAL, "n_agents * envs_per_agent must be at most 2^31");
  if (!seeds) return fail(DQL_EINVAL, "seeds must not be null (one per agent)");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(DQL_EHIP, "no HIP device visible: libdql_hip needs an MI355X (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(DQL_EINVAL, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  dql_ctx* x = new dql_ctx();
  x->cfg = *cfg; x->device = device; x->n = (long long)n_agents * envs_per_agent; x->seed = seeds[0]; x->env_id_offset = 0; x->dtype = cfg->dtype;
  x->real_size = cfg->dtype == DQL_F32 ? 4 : 8;
  x->n_agents = n_agents; x->pop_E = envs_per_agent;
  rc = pop_create_impl(x, seeds);
  if (rc) {
    const std::string why = g_err;
    dql_destroy(x);
    return fail(rc, why);
  }
  *out = x;
  return DQL_OK;
}
int dql_pop_n_agents(dql_ctx* x, int32_t* n) { CHECK_CTX(x); if (!n) return fail(DQL_EINVAL, "null pointer"); *n = x->n_agents; return DQL_OK; }
static int pop_steps(dql_ctx* x, int mode, int32_t n_steps, const double* eps, const uint8_t* active) {
  CHECK_CTX(x);
  if (!x->n_agents) return fail(DQL_EINVAL, "not a population context (dql_pop_create)");
  if (n_steps < 0) return fail(DQL_EINVAL, "n_steps must be >= 0");
  if (mode == MODE_TRAIN && !eps) return fail(DQL_EINVAL, "eps must not be null (one per agent)");
  HIP_TRY(hipSetDevice(x->device));
  for (int i = 0; i < n_steps;) {
    const int np = n_steps - i < x->periods_per_launch ? n_steps - i : x->periods_per_launch;
    int rc = launch_pop(x, mode, eps, active, np); if (rc) return rc;
    i += np;
  }
  return DQL_OK;
}
int dql_pop_train_steps(dql_ctx* x, int32_t n_steps, const double* eps, const uint8_t* active_or_null) { return pop_steps(x, MODE_TRAIN, n_steps, eps, active_or_null); }
int dql_pop_eval_steps(dql_ctx* x, int32_t n_steps, const uint8_t* active_or_null) { return pop_steps(x, MODE_EVAL, n_steps, nullptr, active_or_null); }
int dql_pop_set_curriculum(dql_ctx* x, int32_t agent, int32_t level) {
  dql_ctx* g = nullptr;
  int rc = pop_agent(x, agent, &g); if (rc) return rc;
  if (level < 0 || level >= DQL_MAX_LEVELS) return fail(DQL_EINVAL, "curriculum step must be in 0..4");
  rc = flush_pending(g); if (rc) return rc;
  rc = publish_master(g); if (rc) return rc;
  g->cfg.working_curriculum_step = level;
  rc = upload_mdpk(g); if (rc) return rc;
  hipLaunchKernelGGL(k_mark_reset, dim3((unsigned)((x->pop_E + 255) / 256)), dim3(256), 0, x->stream, x->si + agent * x->pop_E, (const uint8_t*)nullptr, (long long)x->pop_E);
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}
int dql_pop_get_tables(dql_ctx* x, int32_t agent, double* qa, double* qb, double* count) { dql_ctx* g = nullptr; int rc = pop_agent(x, agent, &g); return rc ? rc : dql_get_tables(g, qa, qb, count); }
int dql_pop_set_tables(dql_ctx* x, int32_t agent, const double* qa, const double* qb, const double* count) { dql_ctx* g = nullptr; int rc = pop_agent(x, agent, &g); return rc ? rc : dql_set_tables(g, qa, qb, count); }
int dql_pop_transfer(dql_ctx* x, int32_t agent, int32_t k, double ratio) { dql_ctx* g = nullptr; int rc = pop_agent(x, agent, &g); return rc ? rc : dql_transfer(g, k, ratio); }
int dql_pop_publish_tables(dql_ctx* x, int32_t agent) { dql_ctx* g = nullptr; int rc = pop_agent(x, agent, &g); return rc ? rc : dql_publish_tables(g); }
int dql_pop_stats_get(dql_ctx* x, int32_t agent, dql_stats* out) { dql_ctx* g = nullptr; int rc = pop_agent(x, agent, &g); return rc ? rc : dql_stats_get(g, out); }
int dql_pop_get_step_index(dql_ctx* x, int32_t agent, int64_t* j) { dql_ctx* g = nullptr; int rc = pop_agent(x, agent, &g); return rc ? rc : dql_get_step_index(g, j); }
int dql_pop_set_step_index(dql_ctx* x, int32_t agent, int64_t j) { dql_ctx* g = nullptr; int rc = pop_agent(x, agent, &g); return rc ? rc : dql_set_step_index(g, j); }
int dql_pop_index_faults(dql_ctx* x, int32_t agent, int64_t* n) {
  dql_ctx* g = nullptr;
  int rc = pop_agent(x, agent, &g); if (rc) return rc;
  if (!n) return fail(DQL_EINVAL, "null pointer");
  unsigned long long v = 0;
  HIP_TRY(hipMemcpyAsync(&v, x->pop_faults + agent, sizeof(v), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipStreamSynchronize(x->stream));
  *n = (int64_t)v;
  return DQL_OK;
}

}  // extern "C"
