/*
 * dql_diag.h — measurement and self-test entry points of libdql_hip.so.  NOT part of the drop-in boundary: nothing in the reference maps onto
 * these, the host classes (TrainingMdp, DoubleQLearningAgent, TrainingLandingEnv, Trainer) never call them, and a maintainer who swaps the
 * library in behind the reference's classes needs none of them (INTEGRATION.md section 3 lists what IS needed).  They exist for bench.py, the
 * profiling tools under tools/ and the self-tests in tests/; same conventions as dql.h (0 / negative dql_status, dql_last_error()).
 */
#ifndef DQL_DIAG_H
#define DQL_DIAG_H

#include "dql.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- stream timers (HIP events on the context's stream; torch.cuda.Event would only see torch's stream) ---- */
int dql_diag_timer_start(dql_ctx* ctx);                    /* hipEventRecord on the ctx stream */
int dql_diag_timer_stop(dql_ctx* ctx, double* elapsed_ms); /* records, synchronises, returns elapsed */
/* arm / disarm per-launch event pairs around the fused step kernel and around every table exchange */
int dql_diag_kernel_timer(dql_ctx* ctx, int32_t on);
/* average device duration of the fused step kernel over the launches made while the kernel timer was armed */
int dql_diag_kernel_time_ms(dql_ctx* ctx, double* avg_ms, int64_t* launches);
/* average device time of the exchanges (all-reduce or peer-to-peer push / wait / sum, + fold) made while the kernel timer was armed */
int dql_diag_sync_time_ms(dql_ctx* ctx, double* avg_ms, int64_t* syncs);
/* the step kernel the context's latest launch ran: out5 = {sizeof(real) in bytes, BLOCK, TICK (csrc/dql_device.hpp TICK_*), XMODE (X_TWO 0, X_ONLY 1,
 * X_RUNTIME 2), 1 for the population kernel k_step_pop}: the template arguments of its name; all 0 before the first launch */
int dql_diag_step_instance(dql_ctx* ctx, int32_t* out5);
/* 1 when that launch ran the layout's level-0 instance (working level 0 compiled in: TICK_LIT and TICK_PACKED_LITM launches of x-axis configs at level 0, chosen per launch),
 * 0 for the generic instance; the five numbers above are the same for both */
int dql_diag_step_level0(dql_ctx* ctx, int32_t* level0);
/* holds the context's stream for this long (a one-wave timer kernel): phase offset between contexts that share a GPU (tools/exp_cohorts.py) */
int dql_diag_delay(dql_ctx* ctx, double microseconds);
/* the window accumulators' device buffer (4 * 2835 int64), for a caller that wants to reduce it with a collective of its own; the product path
 * never needs the pointer (dql_allreduce_window / dql_p2p_exchange_window reduce it in place) */
int dql_diag_accum_dev_ptr(dql_ctx* ctx, void** dev_ptr, int64_t* n_int64);

/* device duration (HIP events around the kernel) of the calling thread's latest completed dql_rollout, and the kernel it ran: out3 = {sizeof(real) in
 * bytes, TICK, XMODE}, the template arguments of k_rollout's name */
int dql_diag_rollout_last(double* kernel_ms, int32_t* out3);

/* the same for the calling thread's latest completed dql_score or dql_ensemble_score: inst3 = {sizeof(real) in bytes, TICK, XMODE}, the template arguments
 * of k_score's name */
int dql_diag_score_last(double* kernel_ms, int32_t* inst3);
/* the same for the calling thread's latest completed dql_score_map or dql_ensemble_score_map: the template arguments of k_score_map's name.
 * dql_diag_score_last keeps its meaning: a map call does not change what it reports */
int dql_diag_score_map_last(double* kernel_ms, int32_t* inst3);
/* the same for the calling thread's latest completed dql_model or dql_ensemble_model: the template arguments of k_model's name */
int dql_diag_model_last(double* kernel_ms, int32_t* inst3);
/* the same for the calling thread's latest completed dql_model_split or dql_ensemble_model_split: the template arguments of k_model_split's name.  A refused
 * call leaves the record as it was */
int dql_diag_model_split_last(double* kernel_ms, int32_t* inst3);
/* the calling thread's latest completed dql_returns or dql_ensemble_returns: the device durations of its two kernels (k_returns_fly, then k_returns_sweep) and
 * the template arguments of k_returns_fly's name.  A refused call leaves the record as it was */
int dql_diag_returns_last(double* fly_ms, double* sweep_ms, int32_t* inst3);
/* the same for the calling thread's latest completed dql_score_grid or dql_ensemble_score_grid: the template arguments of k_score_grid's name.  A refused
 * call leaves the record as it was */
int dql_diag_score_grid_last(double* kernel_ms, int32_t* inst3);
/* the same for the calling thread's latest completed dql_score_refined or dql_ensemble_score_refined: the template arguments of k_score_refined's name.  A
 * refused call leaves the record as it was, and dql_diag_score_last keeps its meaning */
int dql_diag_score_refined_last(double* kernel_ms, int32_t* inst3);

/* wall duration on the device (HIP events around all launches) of the ensemble's latest completed dql_ensemble_run */
int dql_diag_ensemble_last(dql_ensemble* ens, double* run_ms);
/* since the ensemble's creation: k_learn / k_learn_levels launches, their agent periods summed, and waves x periods summed (what a launch may fly at most:
 * a wave leaves its loop once none of its lanes is live) */
int dql_diag_ensemble_launches(dql_ensemble* ens, int64_t* launches, int64_t* periods, int64_t* wave_periods);

/* ---- self-test ---- */
/* The float32 tick's square root (csrc/dql_device.hpp sqrt_pos: v_rsq_f32 + one residual correction; until the end of round 5 with a Goldschmidt step in between): counts the inputs with bit
 * patterns lo_bits .. hi_bits whose result is NOT the correctly rounded sqrt.  The CPU oracle computes sqrtf(); parity is bit for bit only while
 * this count is 0 on the tick's domain [1e-30, FLT_MAX] — all 2.1e9 inputs take under a second. */
int dql_diag_selftest_sqrt(int device, uint32_t lo_bits, uint32_t hi_bits, int64_t* not_correctly_rounded);
/* The same count for sqrt_(float) (v_sqrt_f32 + a neighbour test: Box-Muller's radius, the float64-form attitude law), against (float)sqrt((double)x).
 * The CPU oracle's sqrtf() is the definition: the count is 0 at x = 0 and on sqrt_'s domain [2^-102, FLT_MAX]; the normal inputs below 2^-104 are outside it
 * (3 954 656 of them misround) and Box-Muller never produces one. */
int dql_diag_selftest_sqrt_ieee(int device, uint32_t lo_bits, uint32_t hi_bits, int64_t* not_correctly_rounded);

/* ---- the elementary functions and random draws at the top of csrc/dql_device.hpp, evaluated on inputs of the caller's choosing ----
 * The kernels call det_sincos / det_atan2 / det_log / box_muller / philox4x32 themselves and restate nothing.  dtype: DQL_F32 (0) or DQL_F64 (1), the
 * arithmetic the function runs in; values travel as float64 (every float32 is one) and 32-bit words.  1 <= n <= DQL_DIAG_MAX_N per call (n = 0: nothing to do).
 *
 * WAVE LAYOUT: element i is computed by thread i of a one-dimensional grid of 256-thread blocks, so elements 64 w .. 64 w + 63 share wave w and the caller
 * decides which inputs meet in a wave (lanes past n have left before the first function is called).  The float32 det_atan2 branches on a ballot over the wave;
 * the tests construct waves in which some lanes pass its fast-path predicate and others do not. */
#define DQL_DIAG_MAX_N (1ll << 24)
/* element i: sin and cos of x[i], atan2(y[i], x[i]), and log of |x[i]| where |x[i]| > 1e-30, else of 1 */
int dql_diag_det_math_run(int device, int32_t dtype, const double* x, const double* y, int64_t n, double* sin_out, double* cos_out, double* atan2_out, double* log_out);
/* element i: the two normal deviates box_muller makes of the raw words ra[i], rb[i] (radius from ra's upper 24 bits, angle from rb's) */
int dql_diag_box_muller_run(int device, int32_t dtype, const uint32_t* ra, const uint32_t* rb, int64_t n, double* n0_out, double* n1_out);
/* philox4x32-10 of counters [n][4] under the key (k0, k1) -> out [n][4].  round_keys = 0: the key schedule computed inline; 1: the 20 round keys preloaded
 * into registers and passed as philox4x32's kv, filled the way the step kernel fills them */
int dql_diag_philox_run(int device, const uint32_t* counters, uint32_t k0, uint32_t k1, int32_t round_keys, int64_t n, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* DQL_DIAG_H */
