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
//
// This file is the root of the library's one translation unit.  It holds the error plumbing and the shared host helpers, the step engine (the kernels above,
// dql_ctx, the step launch path, the dql_ctx calls, the dql_pop_* calls), and at its end includes one fragment per other subsystem, kernels and host code and
// C calls together: dql_ops.inc (stateless operators), dql_greedy.inc (roll-outs, scorer), dql_ensemble.inc (sequential learners),
// dql_agent.inc (drop-in agent), dql_comm.inc (RCCL, peer-to-peer exchange).
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
#include <type_traits>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_team.hpp"
#include "dql_advance.hpp"
#include "dql_recipes.hpp"
#include "dql_score.hpp"
#include "dql_score_map.hpp"
#include "dql_model.hpp"
#include "dql_model_split.hpp"
#include "dql_refined.hpp"
#include "dql_returns.hpp"
#include "dql_score_grid.hpp"
#include "dql_nstep.hpp"
#include "dql_team_nstep.hpp"
#include "dql_team_levels.hpp"
#include "dql_view.hpp"
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

// ---------------------------------------------------------------------------------------------
// shared host helpers (this file and every subsystem file it includes)
// ---------------------------------------------------------------------------------------------
// the typed code for a run-time dtype: f(float{}) or f(double{}); by_dtype_axes adds the config's X_TWO / X_ONLY instance as a compile-time second argument
template <typename F> static auto by_dtype(int dtype, F&& f) { return dtype == DQL_F32 ? f(float{}) : f(double{}); }
template <typename F> static auto by_dtype_axes(int dtype, int two_axis, F&& f) {
  return by_dtype(dtype, [&](auto t) { return two_axis ? f(t, std::integral_constant<int, X_TWO>{}) : f(t, std::integral_constant<int, X_ONLY>{}); });
}
static size_t mdpk_bytes(int dtype) { return by_dtype(dtype, [](auto t) { return sizeof(MdpK<decltype(t)>); }); }

// device memory of one call (the stateless operators, the roll-outs, the scorer)
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
#define OUT(buf, bytes) do { if ((buf).alloc(bytes)) return fail(DQL_ENOMEM, "hipMalloc failed"); } while (0)
#define UP(buf, host, bytes) do { OUT(buf, bytes); HIP_TRY(hipMemcpy((buf).p, (host), (bytes), hipMemcpyHostToDevice)); } while (0)
#define DOWN(host, buf, bytes) HIP_TRY(hipMemcpy((host), (buf).p, (bytes), hipMemcpyDeviceToHost))

namespace {  // (internal linkage: the library exports its C calls, not these)
// the device memory an object owns for life: alloc() records what it hands out, so no member can be missing from a free list; release() frees one pointer early
// (a table that is being replaced)
struct DevOwned {
  std::vector<void*> ptrs;
  hipError_t alloc(void** p, size_t bytes) { const hipError_t e = hipMalloc(p, bytes); if (e == hipSuccess) adopt(*p); else *p = nullptr; return e; }
  void adopt(void* p) { ptrs.push_back(p); }
  hipError_t release(void* p) {
    for (void*& q : ptrs) if (p && q == p) { q = ptrs.back(); ptrs.pop_back(); return hipFree(p); }
    return hipSuccess;
  }
  void free_all() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); }
};
// device time of a stretch of null-stream work: start(), the work, stop_ms() (which waits for the work)
struct EvTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EvTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  int start() { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e0, 0)); return DQL_OK; }
  int stop_ms(double* ms) {
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float f = 0.0f;
    HIP_TRY(hipEventElapsedTime(&f, e0, e1));
    *ms = (double)f;
    return DQL_OK;
  }
};
}  // namespace

// make_mdpk<T>(cfg) -> device memory at dst: a synchronous copy, or on stream st followed by its synchronisation (the source is a stack temporary)
static int upload_mdpk(const dql_config& cfg, void* dst, hipStream_t st = nullptr) {
  return by_dtype(cfg.dtype, [&](auto t) -> int {
    const MdpK<decltype(t)> m = make_mdpk<decltype(t)>(cfg);
    if (!st) { HIP_TRY(hipMemcpy(dst, &m, sizeof(m), hipMemcpyHostToDevice)); return DQL_OK; }
    HIP_TRY(hipMemcpyAsync(dst, &m, sizeof(m), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DQL_OK;
  });
}
// the tick schedule of periods j0 .. j0 + n - 1 (fill_schedule) -> device arrays of at least n entries (synchronous copies)
static int upload_schedule(const dql_config& cfg, long long j0, int n, void* d_mgr0, void* d_sched) {
  std::vector<long long> h_mgr0((size_t)n);
  std::vector<int> h_sched((size_t)n);
  fill_schedule(cfg, j0, h_mgr0.data(), h_sched.data(), n);
  HIP_TRY(hipMemcpy(d_mgr0, h_mgr0.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_sched, h_sched.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  return DQL_OK;
}
// the real state as the device holds it, Quad<T>[NQ_REAL][n], <-> field-major doubles [NF_REAL][n]; the packed discrete state int4[n] -> field-major ints [NF_INT][n]
template <typename T> static void quads_to_fields(const T* h, long long n, double* out) {
  for (int f = 0; f < NF_REAL; ++f) { const int q = f / 4, k = f % 4; for (long long i = 0; i < n; ++i) out[(long long)f * n + i] = (double)h[((size_t)q * n + i) * 4 + k]; }
}
template <typename T> static void fields_to_quads(const double* in, long long n, T* h) {
  for (int f = 0; f < NF_REAL; ++f) { const int q = f / 4, k = f % 4; for (long long i = 0; i < n; ++i) h[((size_t)q * n + i) * 4 + k] = (T)in[(long long)f * n + i]; }
}
static void unpack_ints(const int4* h, long long n, int32_t* out) {
  for (long long i = 0; i < n; ++i) {
    out[0 * n + i] = h[i].x; out[1 * n + i] = h[i].y; out[2 * n + i] = h[i].z & 0xffff; out[3 * n + i] = (h[i].z >> 16) & 0xffff;
    out[4 * n + i] = h[i].w & 0xff; out[5 * n + i] = (h[i].w >> 8) & 0xff; out[6 * n + i] = (h[i].w >> 16) & 0xff;
  }
}

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
// LEVEL: nothing, or the tag AnyLevel.  k_step<T, BLOCK, TICK, X_ONLY> without the tag is the LEVEL-0 instance of a layout that ends its periods on the literal
// MDP table (TICK_LIT, TICK_PACKED_LITM; x-axis configs, see launch_step_t): agent_period's LEVEL0 form, in which the working level is the compile-time
// constant 0 and the period end's level searches and per-level select chains fold away.  launch_step_t picks it per launch, from the level the launch runs at, and never at
// another level; k_step<..., AnyLevel> is the generic body every other launch runs, and the only form of the layouts without the literal table.  The level-0
// THE ENCODING IS INVERTED ON PURPOSE, and a plain `bool LEVEL0` fifth argument is what it should become: the bench's headline kernel has to keep the name
// `k_step<float, 256, 3, 1>`, because tests/test_profiles_consistency.py looks the kernel up under exactly that name in the newest committed kernel summary
// (profiles/r*_bench_kernel_stats_config4.csv), the bench runs at level 0, and an existing test may not change together with the kernel it checks.  So the
// level-0 instance keeps the four-argument name — the kernel every committed profile measured, all of them at level 0 — and the ordinary one carries the tag.
// A maintainer who writes k_step<T, B, TICK, X> for a layout without a level-0 form meets the static_assert below: add AnyLevel.  The rename (bool argument,
// the test's name pattern and the profiles' kernel names in one change of their own) is listed in DESIGN.md section 10 item 2.
struct AnyLevel {};
template <typename T, int BLOCK, int TICK, int XMODE, typename... LEVEL> __global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(step_min_waves_per_simd(BLOCK, (int)sizeof(T)), step_waves_per_simd(BLOCK)))) void k_step(StepArgs<T> a) {
  constexpr bool LEVEL0 = sizeof...(LEVEL) == 0;
  static_assert(!LEVEL0 || (sizeof(T) == 4 && (TICK == TICK_LIT || TICK == TICK_PACKED_LITM) && XMODE == X_ONLY), "level-0 instances exist for the x-axis literal-MDP layouts only");
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
      const StepOut o = agent_period<TICK, XMODE, LEVEL0>(cfgk, tc, a.mdp, a.mdp_run, e, qx, a.qa, a.qb, a.mode, a.eps_thr, ext, a.seed, (uint32_t)(a.env_id_offset + i), a.step_index + p, a.mgr0[p], a.sched[p], kv);
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
#define DQL_POP_RING 8  // staging slots of population launch descriptors
struct dql_ctx {
  dql_config cfg;
  int device = 0;
  long long n = 0;
  unsigned long long seed = 0;
  long long env_id_offset = 0;
  int dtype = DQL_F32;
  size_t real_size = 4;
  DevOwned dev;         // every plain device allocation below (freed by dql_destroy)
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
  hipEvent_t pop_ev[DQL_POP_RING] = {nullptr};                     // per ring slot: recorded behind the slot's copy (the staging slot is free again once it fired)
  bool pop_busy[DQL_POP_RING] = {false};
  int pop_slot = 0;
  int last_step[5] = {0, 0, 0, 0, 0};  // the step kernel the latest launch ran (dql_diag_step_instance): sizeof(T), BLOCK, TICK, XMODE, population
  bool last_step_level0 = false;      // ... and whether it was the layout's level-0 instance (dql_diag_step_level0)
};

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

// k_init over `count` envs from sr / si on, arrays of stride n: a context's envs, one agent's slice of a population, an ensemble's learners
template <typename T> static int launch_init(const dql_config& c, void* sr, int4* si, long long n, long long count, unsigned long long seed, long long env_id_offset, hipStream_t st) {
  InitArgs<T> a;
  a.c = make_simk<T>(c);
  a.sr = (Quad<T>*)sr; a.si = si; a.n = n; a.seed = seed; a.env_id_offset = env_id_offset;
  const RolloutInit<T> r = make_rollout_init<T>(c);
  a.hover = r.hover; a.vz_integ = r.vz_integ; a.r_lo = r.r_lo; a.r_hi = r.r_hi; a.t_lo = r.t_lo; a.t_hi = r.t_hi;
  const int B = 256;
  hipLaunchKernelGGL(k_init<T>, dim3((unsigned)((count + B - 1) / B)), dim3(B), 0, st, a);
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}

static FoldK make_foldk(const dql_ctx* x, long long n_launch = 1) { return FoldK{x->alpha_tab, x->n_tab, x->cfg.alpha_min, x->cfg.fold_per_step, n_launch}; }
// the template arguments of the step kernel a launch runs, for dql_diag_step_instance (tests assert which instance the host picked)
static void note_step(dql_ctx* x, int bytes, int block, int tick, int xmode, int pop, bool level0 = false) {
  x->last_step[0] = bytes; x->last_step[1] = block; x->last_step[2] = tick; x->last_step[3] = xmode; x->last_step[4] = pop;
  x->last_step_level0 = level0;
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
  // The level-0 instance (k_step without the AnyLevel tag) serves a launch of a literal-MDP layout whose working level is 0, and no other: decided here, at every
  // launch, from the level this launch's constants carry — the trainer promotes levels between launches of the same context.
  auto fly = [&](auto xmode) {
    constexpr int X = decltype(xmode)::value;
    // x-axis instances only.  The two-axis level-0 instance of the 512-thread literal layout (k_step<float, 512, TICK_LIT, X_TWO> without the tag) flies every env
    // exactly as the oracle does and sends wrong targets to table a and the visit counters from its first launch on (1 100 and 262 144 envs, with and without
    // noise and per-env platforms); its 64- and 256-thread siblings and the CPU emulation of the same source (tests/test_level0_host_emulation.py) match bit for
    // bit.  Unexplained, as the two-axis packed + literal-MDP instance is (create_impl): two-axis configs keep the generic body at every level.
    constexpr bool HAS_LEVEL0 = sizeof(T) == 4 && (TICK == TICK_LIT || TICK == TICK_PACKED_LITM) && X == X_ONLY;
    const bool level0 = HAS_LEVEL0 && a.c.working == 0;
    note_step(x, sizeof(T), BLOCK, TICK, X, 0, level0);
    if constexpr (HAS_LEVEL0) {
      if (level0) { hipLaunchKernelGGL((k_step<T, BLOCK, TICK, X>), grid, block, 0, x->stream, a); return; }
    }
    hipLaunchKernelGGL((k_step<T, BLOCK, TICK, X, AnyLevel>), grid, block, 0, x->stream, a);
  };
  // the layouts launch_step_b picks by itself come in an x-axis and a two-axis instance (agent_period's XMODE); the others decide at run time
  if constexpr (sizeof(T) == 4 && TICK == TICK_PACKED_LITM) fly(std::integral_constant<int, X_ONLY>{});  // x-axis configs only (create_impl: litm_ok)
  else if constexpr (sizeof(T) == 4 && (TICK == TICK_LIT || tick_is_packed(TICK))) {
    if (x->cfg.two_axis) fly(std::integral_constant<int, X_TWO>{}); else fly(std::integral_constant<int, X_ONLY>{});
  } else fly(std::integral_constant<int, X_RUNTIME>{});
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
  quads_to_fields(h.data(), x->n, out);
  return DQL_OK;
}
template <typename T> static int set_sim_state_t(dql_ctx* x, const double* in) {
  const long long n = x->n;
  std::vector<T> h((size_t)NQ_REAL * n * 4);
  fields_to_quads(in, n, h.data());
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
#define ALLOC(ptr, bytes) do { hipError_t _e = x->dev.alloc((void**)&(ptr), (bytes)); if (_e != hipSuccess) return fail(DQL_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(_e)); } while (0)
#define ZALLOC(ptr, bytes) do { ALLOC(ptr, bytes); HIP_TRY(hipMemsetAsync((ptr), 0, (bytes), x->stream)); } while (0)
// allocation + initialisation of a fresh context; any failure leaves a partly built context for the caller to destroy
static int create_impl(dql_ctx* x, const dql_config* cfg) {
  HIP_TRY(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&x->ev0)); HIP_TRY(hipEventCreate(&x->ev1));
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, x->device) == hipSuccess && cus > 0) x->n_simds = 4ll * cus; }
  by_dtype(cfg->dtype, [&](auto t) { const SimK<decltype(t)> k = make_simk<decltype(t)>(*cfg); x->kal_fix = KalFix{(double)k.kal_pss, (double)k.kal_kss, true}; });
  const bool refm = cfg->dtype == DQL_F32 && refm_matches(make_mdpk<float>(*cfg));
  x->lit_ok = refm && refk_matches(make_simk<float>(*cfg, &x->kal_fix));
  // x-axis configs only: the two-axis instance of this layout (k_step<float, *, TICK_PACKED_LITM, X_TWO>) faults on its first launch (a memory access the
  // source does not explain — same source as the two instances it combines, both of which are parity-green); it is never selected
  x->litm_ok = refm && !cfg->two_axis;
  ZALLOC(x->sr, (size_t)NQ_REAL * (size_t)x->n * 4 * x->real_size);
  ALLOC(x->si, (size_t)x->n * sizeof(int4));
  ALLOC(x->d_actions, (size_t)x->n);
  HIP_TRY(hipMemsetAsync(x->d_actions, 2, (size_t)x->n, x->stream));
  int rc = create_tables(x);
  if (rc) return rc;
  rc = by_dtype(x->dtype, [&](auto t) { return launch_init<decltype(t)>(x->cfg, x->sr, x->si, x->n, x->n, x->seed, x->env_id_offset, x->stream); });
  if (rc) return rc;
  // default alpha table (plateau only): callers install the reference schedule with dql_set_alpha_table
  const double a0 = cfg->alpha_min;
  return dql_set_alpha_table(x, &a0, 1);
}
// what a context needs besides its envs: tables, ping-pong copies, accumulators, window, statistics, MdpK (also the agents of a population)
static int create_tables(dql_ctx* x) {
  const size_t TB = DQL_N_CELLS * sizeof(double), AB = DQL_ACC_LEN * sizeof(long long);
  ZALLOC(x->qa, TB); ZALLOC(x->qb, TB); ZALLOC(x->count, TB);
  ZALLOC(x->qa_base, TB); ZALLOC(x->count_base, TB); ZALLOC(x->qb_base, TB);
  for (int k = 0; k < 2; ++k) { ZALLOC(x->tb[k], TB); ZALLOC(x->tbb[k], TB); ZALLOC(x->acc[k], AB); }
  ZALLOC(x->window_own, AB); x->window = x->window_own;
  ZALLOC(x->stats, sizeof(StatsDev)); ALLOC(x->mdpk, sizeof(MdpK<double>));
  return upload_mdpk(x->cfg, x->mdpk, x->stream);
}
#undef ZALLOC
#undef ALLOC

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
  for (hipEvent_t e : x->kev) (void)hipEventDestroy(e);
  for (hipEvent_t e : x->sev) (void)hipEventDestroy(e);
  for (int r = 0; r < DQL_P2P_MAX_RANKS; ++r) if (x->p2p_opened[r] && x->p2p_peer[r]) (void)hipIpcCloseMemHandle(x->p2p_peer[r]);
  x->dev.free_all();
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
  HIP_TRY(x->dev.release(x->alpha_tab));
  x->alpha_tab = nullptr;
  HIP_TRY(x->dev.alloc((void**)&x->alpha_tab, (size_t)n * sizeof(double)));
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
  rc = upload_mdpk(x->cfg, x->mdpk, x->stream);
  if (rc) return rc;
  return dql_reset(x, nullptr);
}

int dql_reset(dql_ctx* x, const uint8_t* mask) {
  CHECK_CTX(x);
  HIP_TRY(hipSetDevice(x->device));
  const uint8_t* dmask = nullptr;
  if (mask) {
    if (!x->d_mask && x->dev.alloc((void**)&x->d_mask, (size_t)x->n) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc(reset mask) failed");
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
  return by_dtype(x->dtype, [&](auto t) { return get_sim_state_t<decltype(t)>(x, out); });
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
  return by_dtype(x->dtype, [&](auto t) { return set_sim_state_t<decltype(t)>(x, in); });
}
int dql_get_sim_ints(dql_ctx* x, int32_t* out, int32_t cap) {
  CHECK_CTX(x);
  if (!out || cap < NF_INT) return fail(DQL_EINVAL, "out buffer must hold 7 fields x n_envs int32");
  std::vector<int4> h; int rc = fetch_ints(x, h); if (rc) return rc;
  unpack_ints(h.data(), x->n, out);
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
  return by_dtype(x->dtype, [&](auto t) { return get_rewards_t<decltype(t)>(x, rewards); });
}
int dql_get_obs(dql_ctx* x, double* out) {
  CHECK_CTX(x);
  if (!out) return fail(DQL_EINVAL, "null pointer");
  return by_dtype(x->dtype, [&](auto t) { return get_obs_t<decltype(t)>(x, out); });
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
int dql_diag_step_level0(dql_ctx* x, int32_t* level0) {
  CHECK_CTX(x);
  if (!level0) return fail(DQL_EINVAL, "null pointer");
  *level0 = x->last_step_level0 ? 1 : 0;
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
  if (x->elog) { HIP_TRY(x->dev.release(x->elog)); x->elog = nullptr; }
  x->elog_cap = 0; x->elog_n = 0;
  for (dql_ctx* g : x->agents) g->elog_n = 0;
  if (capacity_periods == 0) return DQL_OK;
  const size_t nw = (size_t)((x->n + 63) >> 6);
  if (x->dev.alloc((void**)&x->elog, (size_t)capacity_periods * 2 * nw * sizeof(unsigned long long)) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc(episode log) failed");
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
    // k_init over agent k's E envs alone: the state arrays keep the population's stride (n = K E), the base moves to the agent's first env, and the grid
    // is exactly E threads (E is a multiple of 512), so that no thread reaches past the agent's slice
    void* sr_k = (char*)x->sr + (size_t)k * (size_t)x->pop_E * 4 * x->real_size;
    rc = by_dtype(x->dtype, [&](auto t) { return launch_init<decltype(t)>(x->cfg, sr_k, x->si + k * x->pop_E, x->n, x->pop_E, g->seed, 0, x->stream); });
    if (rc) return rc;
  }
  const size_t ring = (size_t)DQL_POP_RING * DQL_MAX_AGENTS * sizeof(PopAgentDesc);
  if (hipHostMalloc((void**)&x->pop_h, ring, hipHostMallocDefault) != hipSuccess) { x->pop_h = nullptr; return fail(DQL_ENOMEM, "hipHostMalloc(launch descriptors) failed"); }
  if (x->dev.alloc((void**)&x->pop_d, ring) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc(launch descriptors) failed");
  if (x->dev.alloc((void**)&x->pop_faults, (size_t)x->n_agents * sizeof(unsigned long long)) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc(fault counters) failed");
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
  rc = upload_mdpk(g->cfg, g->mdpk, g->stream); if (rc) return rc;
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

#include "dql_ops.inc"
#include "dql_greedy.inc"
#include "dql_ensemble.inc"
#include "dql_recipes.inc"
#include "dql_teams.inc"
#include "dql_nstep.inc"
#include "dql_nstep_recipes.inc"
#include "dql_team_nstep.inc"
#include "dql_team_levels.inc"
#include "dql_score_map.inc"
#include "dql_model.inc"
#include "dql_model_split.inc"
#include "dql_refined.inc"
#include "dql_returns.inc"
#include "dql_score_grid.inc"
#include "dql_view.inc"
#include "dql_agent.inc"
#include "dql_comm.inc"
