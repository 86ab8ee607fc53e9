/*
 * dql.h — C ABI of libdql_hip.so: the MI355X (gfx950) vectorised UAV-landing environment +
 * tabular Double-Q trainer hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI: the path sits behind
 * Python classes.  Each entry point below names the reference interface it replaces; the Python
 * host package `dql_multirotor_landing_amd` binds these with ctypes and re-exposes the reference's
 * class/method names (INTEGRATION.md shows the stub).
 *
 * Conventions: every function returns 0 (DQL_OK) or a negative dql_status; dql_last_error() gives
 * the thread-local message of the last failure.  All pointers are plain host pointers unless the
 * name says "dev".  A dql_ctx owns its device memory and stream; it is not thread-safe; calls on
 * one ctx are stream-ordered and asynchronous until a dql_get_* / dql_stats / dql_sync call.
 * No torch types, no C++ types.
 */
#ifndef DQL_H
#define DQL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQL_ABI_VERSION 6 /* 6: dql_agent_mirror_update_deferred / _complete (added since, without a new number: dql_ensemble_set_curriculum, _set_level_schedules, _get_levels, _n_unfinished; dql_ensemble_set_recipes, _set_recipe, _set_recipe_level_schedules, _get_recipes; dql_ensemble_create_teams, _envs_per_learner; dql_ensemble_set_nstep, _get_nstep; dql_ensemble_set_recipe_nstep, _get_recipe_nstep); 5: tick replay operators (dql_*_run), measurement symbols moved to dql_diag.h as dql_diag_* */

typedef enum dql_status {
  DQL_OK = 0,
  DQL_EINVAL = -1, /* bad argument / unsupported configuration (Python: ValueError) */
  DQL_EHIP = -2,   /* HIP runtime error (Python: RuntimeError) */
  DQL_ESTATE = -3, /* call order violation, e.g. step before reset (Python: ValueError) */
  DQL_ENOMEM = -4,
  DQL_ERCCL = -5,  /* RCCL error, or librccl could not be loaded (Python: RuntimeError) */
  DQL_EPEER = -6   /* a peer-to-peer table exchange gave up on a missing peer: the replicas may differ from here on (Python: RuntimeError) */
} dql_status;

/* CheckResult codes, declaration order of pkg/mdp.py:68-77 */
enum {
  DQL_TERMINAL_CONTACT = 0,
  DQL_TERMINAL_SUCCESS = 1,
  DQL_TERMINAL_FLYZONE_X = 2,
  DQL_TERMINAL_FLYZONE_Y = 3,
  DQL_TERMINAL_FLYZONE_Z = 4,
  DQL_TERMINAL_MINIMUM_ALTITUDE = 5,
  DQL_TERMINAL_TIMEOUT = 6,
  DQL_NON_TERMINAL_SUCCESS = 7,
  DQL_NON_TERMINAL = 8,
  DQL_N_CHECK_CODES = 9
};

/* Quirk switches.  mode="reference" = all set; mode="paper" = DQL_Q_GOAL_COUNT_KEPT only. */
enum {
  DQL_Q_FAIL_TERM_EVERY_STEP = 1 << 0,  /* B7  pkg/mdp.py:528-536 */
  DQL_Q_STICKY_CHECK = 1 << 1,          /* B8  pkg/mdp.py:363-425: _check_result is only ever set inside an episode, so after the first
                                         * NON_TERMINAL_SUCCESS every later step keeps the success code (and its reward term) */
  DQL_Q_SHAPING_SURVIVES_RESET = 1 << 2,/* B9  pkg/mdp.py:196-197,469-474 */
  DQL_Q_FROZEN_ACC_REFERENCE = 1 << 3,  /* B19 pkg/observation_utils.py:137-150: last_velocity never updated */
  DQL_Q_BOOTSTRAP_ON_POS_CHANGE = 1 << 4,/* B3  pkg/double_q_learning.py:139-145 */
  DQL_Q_UPDATE_TABLE_A_ONLY = 1 << 5,   /* B1/B2 pkg/double_q_learning.py:101-108,136-146: both arms of the coin pick Q_table_a and
                                         * it values its own greedy action.  Cleared (mode="paper"): Double Q-learning as the paper
                                         * has it: a fair coin picks the table to update, the OTHER table values the picked
                                         * table's greedy action at s'; Q_table_b learns too. */
  DQL_Q_GOAL_COUNT_KEPT = 1 << 6,       /* second half of B8, pkg/mdp.py:402-425: _curriculum_check counts the steps spent in the goal bins at
                                         * the working level and is reset only by a goal-bin step at another level — leaving the bins keeps
                                         * it, so "Goal state reached" needs f_ag such steps in TOTAL, not in a row.  This is the success
                                         * criterion the reference's trainer promotes on (B17), kept in paper mode.  Cleared: the counter
                                         * restarts whenever the goal bins are left (one second WITHOUT interruption inside the innermost
                                         * bins: stricter than the code and than the paper's "in that curriculum step's discrete states") */
  DQL_Q_REFERENCE = 0x7f
};

enum { DQL_F32 = 0, DQL_F64 = 1 };
enum { DQL_TRAJ_RPM = 0, DQL_TRAJ_EIGHT = 1 };

#define DQL_MAX_LEVELS 5
#define DQL_N_ACTIONS 3
#define DQL_N_ANGLES 7
#define DQL_STATES_PER_LEVEL (3 * 3 * 3 * DQL_N_ANGLES)            /* 189 */
#define DQL_CELLS_PER_LEVEL (DQL_STATES_PER_LEVEL * DQL_N_ACTIONS) /* 567 */
#define DQL_N_STATES (DQL_MAX_LEVELS * DQL_STATES_PER_LEVEL)       /* 945 */
#define DQL_N_CELLS (DQL_MAX_LEVELS * DQL_CELLS_PER_LEVEL)         /* 2835 = (5,3,3,3,7,3) C-order */
#define DQL_TARGET_FRAC_BITS 26 /* fixed-point scale of the int64 TD-target accumulators */

/* One POD configuration block; the Python dataclass `DqlConfig` mirrors it field for field with the
 * reference's defaults (constants harvested in SURVEY.md appendix A, cited per field). */
typedef struct dql_config {
  /* ---- MDP: pkg/mdp.py:87-147, 214-255 ---- */
  int32_t working_curriculum_step; /* 0..4 */
  int32_t two_axis;                /* 0: TrainingMdp (x / pitch), 1: x+y (SimulationMdp layout) */
  uint32_t quirks;                 /* DQL_Q_* */
  int32_t dtype;                   /* DQL_F32 | DQL_F64: arithmetic of the fused simulator kernel */
  double f_ag, t_max, p_max, v_max, a_max;
  double theta_max, delta_theta, beta, sigma_a, minimum_altitude;
  double w_p, w_v, w_theta, w_dur, w_fail, w_succ;
  double lim_p[DQL_MAX_LEVELS], lim_v[DQL_MAX_LEVELS], lim_a[DQL_MAX_LEVELS]; /* pkg/mdp.py:45-53 */
  double vz_setpoint, yaw_setpoint; /* pkg/mdp.py:212 (-0.1 training), :580 (-0.4 simulation) */
  /* ---- agent / trainer: pkg/trainer.py:31-33 ---- */
  double gamma, alpha_min, alpha_omega;
  /* ---- simulator (replaces Gazebo + RotorS + 5 ROS nodes) ---- */
  double dt;           /* worlds/basic.world:64-70  0.002 */
  int32_t manager_div; /* physics ticks per manager tick: 100 Hz -> 5 (launch/environment.launch:55) */
  int32_t trajectory;  /* DQL_TRAJ_* (pkg/moving_platform.py:87-127) */
  double gravity;      /* 9.8 (worlds/basic.world:36) */
  double mass;         /* 0.68 + 4*0.009 + 1e-5 (hummingbird.xacro:29,32) */
  double inertia[3];   /* composite diagonal about the base origin */
  double arm_length, rotor_z;   /* 0.17, 0.01 */
  double k_f, k_m;              /* 8.54858e-06, 0.016 */
  double rotor_alpha_up, rotor_alpha_down; /* exp(-dt/0.0125), exp(-dt/0.025) (common.h:147-183) */
  double rotor_max;             /* 838 */
  double c_drag, c_roll;        /* 8.06428e-05, 1e-06 */
  double k_R[3], k_W[3];        /* pkg/attitude_controller.py:86-87 */
  double pid_vz[6];             /* Kp Ki Kd lower upper windup: launch/drone.launch:35-40 */
  double pid_yaw[6];            /* launch/drone.launch:49-54 */
  double bw_c;                  /* Butterworth c = 1 (pkg/filters.py:93) */
  double mp_r_x, mp_t_x;        /* platform amplitude and speed, omega = t_x / r_x (environment.launch:60-72) */
  double mp_dt;                 /* 1 / frequency = 0.01 */
  double mp_top_z, mp_half_x, mp_half_y; /* landing surface 0.455, half extents 0.5 (+ drone half width) */
  double drone_bottom;          /* base box half height 0.06 */
  double z_init, init_sigma;    /* pkg/trainer.py:41 (4.0), p_max/3 (landing_simulation_env.py:189) */
  int32_t init_uniform;         /* start offset x0 and placement: 0: x0 ~ N(0,sigma) at level 0 else U(-p_max, p_max), drone at clip(x0 + mp, mp +- p_max)
                                   (TrainingLandingEnv.reset, pkg/landing_simulation_env.py:181-209); 1: always U, same placement; 2: always U,
                                   drone at clip(mp - x0, +-p_max) as SimulationLandingEnv.reset has it (:331-343: offset subtracted, absolute clip) */
  int32_t per_env_platform;     /* 1: r_x, t_x drawn per env from the ranges below (BASELINE config 5) */
  int32_t goal_logic;           /* 1: TrainingMdp.check goal / success branch (pkg/mdp.py:402-425); 0: SimulationMdp.check (:784-845) */
  int32_t fold_per_step;        /* 0: per-visit fold (prod of (1-alpha) over the m visits of a launch); 1: ONE alpha step per launch towards the
                                   launch's mean target (count still advances by m): smoother at large N */
  double mp_r_lo, mp_r_hi, mp_t_lo, mp_t_hi;
  double noise_pos_sd, noise_vel_sd, kalman_q; /* scripts/manager_node.py:83-98 */
} dql_config;

/* Aggregated counters since the last dql_stats_reset (device-side reductions). */
typedef struct dql_stats {
  int64_t agent_steps;   /* launches of the fused step kernel */
  int64_t decisions;     /* env-steps: (env, step) pairs in which an action was taken (reset periods excluded) */
  int64_t episodes;      /* finished episodes */
  int64_t by_code[DQL_N_CHECK_CODES]; /* terminal histogram by CheckResult code */
  double reward_sum;     /* sum of step rewards over all decisions */
  int64_t physics_ticks; /* global physics tick index */
} dql_stats;

typedef struct dql_ctx dql_ctx;

/* ---- library ---- */
int dql_abi_version(void);
const char* dql_last_error(void);
int dql_device_count(int* count);
/* fill cfg with the reference defaults; training flavour */
int dql_config_default(dql_config* cfg);

/* ---- context: replaces gym.make("Landing-Training-v0") + DoubleQLearningAgent() (pkg/trainer.py:176-183,46-48) ---- */
int dql_create(const dql_config* cfg, int device, int64_t n_envs, uint64_t seed, int64_t env_id_offset, dql_ctx** out);
int dql_destroy(dql_ctx* ctx);
int dql_sync(dql_ctx* ctx);
int dql_n_envs(dql_ctx* ctx, int64_t* n);
int dql_state_bytes_per_env(dql_ctx* ctx, int64_t* bytes);

/* alpha(count) table: alpha[c] for c < n, alpha_min beyond (pkg/trainer.py:88-110, computed by the host exactly
 * as the reference does so that device and oracle share bit-identical values) */
int dql_set_alpha_table(dql_ctx* ctx, const double* alpha, int32_t n);
/* Trainer creates a new env per curriculum level (pkg/trainer.py:172-183): new limits, every env re-enters via reset */
int dql_set_curriculum(dql_ctx* ctx, int32_t working_curriculum_step);

/* ---- env: TrainingLandingEnv.reset / .step (pkg/landing_simulation_env.py:167-282) ---- */
/* mark envs for reset (mask NULL = all); the reset (placement + one agent period + first discrete state)
 * is executed by the next step/train call, as the reference's reset() runs one agent period of simulation */
int dql_reset(dql_ctx* ctx, const uint8_t* mask_or_null);
/* one agent step with caller-supplied actions (uint8 per env: ax | ay << 2, ax, ay in 0 / 1 / 2, ay only in two_axis configs); no table
 * update.  The actions are staged through pinned host memory.  Up to 16 384 envs (the single-env drop-in path among them) the codes are
 * checked while they are staged and a bad one is REFUSED before anything is flown: DQL_EINVAL, no env has moved (the reference raises before
 * publishing the action, pkg/mdp.py:544-545).  Beyond that the step kernel checks them per env (no host loop over n_envs, no wait): an
 * out-of-range action is flown as "hold" and makes the next dql_step_outputs / dql_stats_get return DQL_EINVAL once — a caller that reads
 * results with dql_get_states / dql_get_sim_state only must ask dql_stats_get for the verdict. */
int dql_step(dql_ctx* ctx, const uint8_t* actions);
/* what `TrainingLandingEnv.step` returns (pkg/landing_simulation_env.py:245-282), for every env, in ONE device round trip: packed
 * states, reward, done ("Termination condition" in info), CheckResult code, "Number of steps", cumulative reward (after this step's
 * reward), and whether the env spent the period in reset().  Any output may be NULL.  The step kernel's results are gathered into
 * pinned host memory by a small kernel on the context's stream; the call returns when it has run. */
int dql_step_outputs(dql_ctx* ctx, int32_t* idx_x, int32_t* idx_y, double* reward, uint8_t* done, int8_t* code, int32_t* step_count,
                     double* cumulative_reward, uint8_t* was_reset);
/* same with the actions already in device memory (n_envs bytes, readable on the context's device): no copy, no host-side
 * validation, fully asynchronous (the buffer must stay valid until the step has run); values other than 0 / 1 act as "hold" */
int dql_step_dev(dql_ctx* ctx, const uint8_t* dev_actions);
/* Device-resident step outputs: what dql_step_outputs returns, plus the continuous observation, written into CALLER-OWNED DEVICE buffers by one kernel
 * on the context's stream.  The call returns without waiting; the buffers must stay valid until the kernel has run.  Every pointer is a device address
 * readable and writable on the context's device, and every pointer may be NULL: that output is skipped.  The view reports the state as it stands after
 * the stream's earlier work (dql_step_dev, dql_step, dql_train_steps, dql_eval_steps).
 * An obs row holds the state fields obs_p_x, obs_v_x, obs_a_x, pitch_sp, obs_p_y, obs_v_y, obs_a_y, roll_sp; reward is the field reward,
 * cumulative_reward is cum_x; the integer and byte outputs are what dql_step_outputs decodes from the same words.
 * Conversion of a context element to real_dtype: the same type keeps the bits, float -> double is exact, double -> float is one round-to-nearest-even
 * cast.  DQL_EINVAL (nothing launched, no buffer touched): a null ctx or view, real_dtype neither DQL_F32 nor DQL_F64, reserved != 0, obs not 16-byte
 * aligned, a population context.  A view whose pointers are all NULL returns DQL_OK and launches nothing. */
#define DQL_VIEW_OBS 8
typedef struct dql_view {
  int32_t real_dtype;          /* DQL_F32 or DQL_F64: element type of obs, reward, cumulative_reward — independent of the context's dtype */
  int32_t reserved;            /* must be 0 */
  void*    obs;                /* [n_envs][DQL_VIEW_OBS] row-major, 16-byte aligned */
  void*    reward;             /* [n_envs] */
  void*    cumulative_reward;  /* [n_envs] */
  int32_t* idx_x; int32_t* idx_y; int32_t* step_count;   /* [n_envs] each */
  uint8_t* done; uint8_t* was_reset; int8_t* code;       /* [n_envs] each */
  uint64_t* bad_actions;       /* one word: the count of out-of-range external actions as it stands, NOT cleared (dql_step_outputs / dql_stats_get report and clear it) */
} dql_view;
int dql_view_dev(dql_ctx* ctx, const dql_view* view);
/* dql_reset with a mask that already lives in device memory (n_envs bytes, non-zero = reset): read by the marking kernel itself, no copy and no
 * wait; the buffer must stay valid until the kernel has run.  NULL is refused (dql_reset with NULL marks every env). */
int dql_reset_dev(dql_ctx* ctx, const uint8_t* dev_mask);
/* n fused agent steps: on-device eps-greedy guess + step + TD-target accumulation + table apply
 * (pkg/trainer.py:191-212 loop body for all envs at once) */
int dql_train_steps(dql_ctx* ctx, int32_t n_steps, double eps);
/* n greedy steps without learning (scripts/simulation.py:49-56) */
int dql_eval_steps(dql_ctx* ctx, int32_t n_steps);

/* per-env results of the last step (host out buffers of n_envs elements) */
int dql_get_states(dql_ctx* ctx, int32_t* idx_x, int32_t* idx_y_or_null); /* packed ((((k*3+p)*3+v)*3+a)*7+theta) */
int dql_get_rewards(dql_ctx* ctx, double* rewards);
int dql_get_dones(dql_ctx* ctx, uint8_t* dones, int8_t* codes_or_null);
int dql_get_actions(dql_ctx* ctx, uint8_t* actions);
/* raw continuous state, field-major [n_fields][n_envs] as doubles (see dql_field_names).
 * All 64 real fields mean the same in float32 and float64 contexts EXCEPT the two PIDs' Butterworth filter fields vz_x1 vz_x2 vz_y1 vz_y2 vz_y3 and
 * yw_*: a float64 context keeps the reference's histories there (x1, x2 = the last two inputs, y1..y3 = the last three outputs, pkg/filters.py:98-109),
 * a float32 context the three states of the same recurrence in transposed form in (x1, x2, y1) with y2 = y3 = 0:
 *   t1 = 2b x1 + b x2 - a2 y2 - a3 y3,  t2 = b x1 - a2 y1 - a3 y2,  t3 = -a3 y1   (b, a2, a3: csrc/dql_device.hpp butterworth).
 * State written by one dtype must be mapped before it is handed to the other (host: dql_multirotor_landing_amd/state_layout.py; float64 -> float32
 * only: three numbers do not determine five).  The library cannot tell the two apart: dql_set_sim_state trusts the caller.  The Trainer's
 * checkpoints carry dtype + layout version and map or refuse a shard by themselves.
 * A float32 x-axis context (two_axis = 0) flies the attitude law's closed form for a roll set-point of exactly 0: dql_set_sim_state refuses
 * (DQL_EINVAL) a non-zero roll_sp field there instead of ignoring it. */
int dql_get_sim_state(dql_ctx* ctx, double* out, int32_t n_fields_capacity);
int dql_set_sim_state(dql_ctx* ctx, const double* in, int32_t n_fields);
int dql_get_sim_ints(dql_ctx* ctx, int32_t* out, int32_t n_fields_capacity);
int dql_set_sim_ints(dql_ctx* ctx, const int32_t* in, int32_t n_fields);
int dql_n_fields(int32_t* n_real, int32_t* n_int);
const char* dql_field_name(int32_t i, int32_t is_int);
/* last latched observation per env: [6][n] = rel_p_x, rel_p_y, rel_v_x, rel_v_y, rel_a_x, rel_a_y */
int dql_get_obs(dql_ctx* ctx, double* out);

/* ---- tables: DoubleQLearningAgent.Q_table_a/_b/state_action_counter (pkg/double_q_learning.py:35-40) ---- */
int dql_get_tables(dql_ctx* ctx, double* qa, double* qb, double* count); /* 2835 doubles each, C order (5,3,3,3,7,3) */
int dql_set_tables(dql_ctx* ctx, const double* qa, const double* qb, const double* count);
int dql_transfer(dql_ctx* ctx, int32_t k, double ratio); /* transfer_learning (pkg/double_q_learning.py:77-89) */

/* ---- multi-GPU exchange: int64 accumulators [4][2835] = Q_table_a's {sum of targets (fixed point), visits},
 * then Q_table_b's (all zero under DQL_Q_UPDATE_TABLE_A_ONLY) ---- */
int dql_set_sync_period(dql_ctx* ctx, int32_t k_steps); /* 1 = apply every step (single-GPU semantics) */
/* windowed accumulation: every step also adds its accumulators into the window buffer and updates only the local
 * work tables; dql_apply_accum folds the (all-reduced) window into the base tables and re-bases the work tables */
int dql_set_windowed(dql_ctx* ctx, int32_t on);
/* use a caller-owned device buffer of 4*2835 int64 as the window (e.g. a torch tensor handed to torch.distributed);
 * NULL restores the context's own buffer.  The buffer is zeroed; the context never frees it. */
int dql_set_window_buffer(dql_ctx* ctx, void* dev_ptr);
int dql_stream_handle(dql_ctx* ctx, void** hip_stream);
/* The table update of launch j rides in the writer workgroups of launch j+1 (tables act with one period of delay);
 * dql_flush folds what is still pending (master tables and window) now.  Table getters / setters flush by themselves;
 * call it before all-reducing the window buffer directly. */
int dql_flush(dql_ctx* ctx);
/* fold the (all-reduced) window into the base tables; master and acting tables restart from them.  With fold_per_step a
 * cell visited m times (all ranks together) in a window of L launches takes min(m, L) learning-rate steps towards the
 * window's mean target (L = 1: the single-launch rule), so the step size per env-step does not depend on the sync period */
int dql_apply_accum(dql_ctx* ctx);
int dql_get_accum(dql_ctx* ctx, int64_t* out); /* host copy of the 4*2835 window words, for tests */
int dql_set_accum(dql_ctx* ctx, const int64_t* in);
/* agent periods launched so far: the physics tick schedule and the per-period RNG counters are functions of it, so a
 * checkpointed run resumes by restoring the env fields (dql_set_sim_state / _ints), the tables and this index */
int dql_get_step_index(dql_ctx* ctx, int64_t* step_index);
int dql_set_step_index(dql_ctx* ctx, int64_t step_index);
/* checkpoint barrier: fold what is pending and make the acting tables equal to the master tables (what a resumed run starts from) */
int dql_publish_tables(dql_ctx* ctx);

/* ---- RCCL communicator (ncclAllReduce(ncclInt64, ncclSum) of the window over xGMI; no PyTorch) ----
 * librccl.so is loaded on first use (dlopen), so single-GPU users never pay for it.  One process per GPU: rank 0 calls
 * dql_comm_unique_id and hands the 128 bytes to the other ranks out of band (the Python host uses a file, comm.py), then
 * every rank calls dql_comm_create.  The host-buffer collectives below are the Trainer's control plane (chunk counters,
 * judged envs' episode logs, the bench's max-over-ranks timing); they stage through a device buffer on the communicator's
 * own stream and return when the result is in `inout` / `out`. */
#define DQL_COMM_ID_BYTES 128
typedef struct dql_comm dql_comm;
enum { DQL_OP_SUM = 0, DQL_OP_MAX = 1 };
int dql_comm_unique_id(uint8_t* id_out /* [DQL_COMM_ID_BYTES] */);
int dql_comm_create(int device, int32_t rank, int32_t world, const uint8_t* id /* [DQL_COMM_ID_BYTES] */, dql_comm** out);
int dql_comm_destroy(dql_comm* comm);
int dql_comm_info(dql_comm* comm, int32_t* rank, int32_t* world, int32_t* device);
int dql_comm_allreduce_f64(dql_comm* comm, double* inout, int64_t n, int32_t op);
int dql_comm_allreduce_i64(dql_comm* comm, int64_t* inout, int64_t n, int32_t op);
int dql_comm_allgather_u64(dql_comm* comm, const uint64_t* in, int64_t n, uint64_t* out /* [world][n], rank order */);
int dql_comm_barrier(dql_comm* comm);
/* data path: the context's window is summed over the ranks in place, on the context's stream (asynchronous; the fold
 * that follows, dql_apply_accum, is stream-ordered behind it).  Flushes first.  NULL detaches. */
int dql_attach_comm(dql_ctx* ctx, dql_comm* comm_or_null);
int dql_allreduce_window(dql_ctx* ctx);

/* ---- one-shot peer-to-peer exchange (second step; no counterpart in the reference) ----
 * The same sum of the window accumulators without a collective: every rank pushes its 90 KB window into a slot of EVERY rank's
 * exchange buffer (HIP IPC mappings of uncached device memory: world concurrent one-hop writes over the direct xGMI links), raises
 * a flag there, waits for its peers' flags and adds the slots up in rank order.  Call order on every rank:
 *   dql_p2p_create(ctx, rank, world, handle)  -> 64-byte IPC handle of this rank's buffer; gather all ranks' handles (any way:
 *   dql_comm_allgather_u64, files, ...), dql_p2p_connect(ctx, handles in rank order), then per exchange
 *   dql_p2p_exchange_window(ctx) (asynchronous, on the context's stream; includes the flush) followed by dql_apply_accum(ctx) —
 *   the drop-in for dql_allreduce_window.  A peer that never shows up makes the wait give up after option "p2p_spin_limit" polls
 *   (default 60 M, a minute or two) instead of hanging the GPU.  ONE waiter decides per exchange: the window is then either the full
 *   sum or untouched (this rank's own accumulators), never half-summed; the sequence number of the first failed exchange is kept
 *   (dql_p2p_status: failed_seq, 0 = none) and from then on dql_stats_get — the per-chunk synchronisation point of the training
 *   loop — returns DQL_EPEER, so a training run cannot carry on with diverging replicas.  world <= DQL_P2P_MAX_RANKS.
 *   Ranks that share ONE GPU (tests, rehearsals) need HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment before the first HIP call:
 *   the host driver only supports dmabuf IPC, and hipIpcGetMemHandle fails with "invalid argument" without it. */
#define DQL_P2P_HANDLE_BYTES 64
#define DQL_P2P_MAX_RANKS 8
int dql_p2p_create(dql_ctx* ctx, int32_t rank, int32_t world, uint8_t* handle_out);
int dql_p2p_connect(dql_ctx* ctx, const uint8_t* all_handles);
/* peers that live in THIS process (one host thread driving several contexts, SURVEY.md section 8b "threading"): their exchange buffers
 * are connected by pointer instead of through an IPC handle (which cannot be opened by the process that exported it).  peers[world] in
 * rank order, NULL for ranks of other processes (those come through dql_p2p_connect).  Peer access between devices is enabled here. */
int dql_p2p_connect_local(dql_ctx* ctx, dql_ctx* const* peers);
int dql_p2p_exchange_window(dql_ctx* ctx);
/* the two halves of dql_p2p_exchange_window, for a host thread that drives several ranks: enqueue EVERY local rank's push (flush +
 * push + signal) before any local rank's wait (wait + sum) — streams of one process may share a hardware queue, and a wait kernel
 * queued ahead of the push it waits for would only end at its poll bound */
int dql_p2p_push_window(dql_ctx* ctx);
int dql_p2p_wait_window(dql_ctx* ctx);
int dql_p2p_status(dql_ctx* ctx, int32_t* failed_seq);

/* ---- stats ----  (timers, the kernel's self-test and other measurement equipment: include/dql_diag.h) */
int dql_stats_get(dql_ctx* ctx, dql_stats* out);
int dql_stats_reset(dql_ctx* ctx);
/* knobs: "block" (0 = auto, 64, 128, 256 threads per workgroup; 512 = float32 at 4 waves per SIMD); "tick" (0 = auto; layout of the
 * 500 Hz loop: 1 plain loop on scalar-register constants, 3 the packed float32 tick, 4 constants as instruction literals — float32
 * contexts whose vehicle / controller constants are the reference's, DQL_EINVAL otherwise: same arithmetic, bit for bit, in all;
 * 2, a retired layout, is DQL_EINVAL);
 * "periods_per_launch" P in 1..32 (default 1): dql_train_steps / dql_eval_steps run P agent periods per kernel launch — every env
 * stays in registers between them, so the state round trip through HBM and the launch boundary are paid once per P periods.
 * Table timing in units of launches is unchanged (a launch acts on every accumulator up to the launch before the previous one,
 * all P periods of a launch act on the same tables and add to the same accumulators; a per-step fold takes min(visits, P)
 * learning-rate steps per launch); P = 1 is the period-by-period schedule.  n_steps need not be a multiple of P.
 * "fair_prio" (-1 automatic, 0, 1): the waves that share a SIMD take turns at the issue priority (s_setprio by period + wave-slot parity) so that they finish a
 * launch together instead of the older one first; automatic = when the context has more env waves than the device has SIMDs; 1 for contexts that share one GPU. */
int dql_set_option(dql_ctx* ctx, const char* name, int32_t value);

/* ---- episode log (Trainer promotion rule, pkg/trainer.py:218-232) ----
 * The reference appends one 0/1 ("Goal state reached" in info["Termination condition"]) per finished episode to a
 * deque(maxlen=100) and promotes when its sum / 100 exceeds 0.96: the rule needs the ORDER in which episodes finish.  With
 * the log enabled every launch records, per wave of 64 envs, a 64-bit mask of the envs whose episode ended in that agent
 * period and a mask of those that ended in TERMINAL_SUCCESS; periods in launch order x envs in index order is the global
 * completion order.  n_waves = (n_envs + 63) / 64.  A launch with a full log fails with DQL_ESTATE. */
int dql_episode_log_enable(dql_ctx* ctx, int32_t capacity_periods); /* 0 disables and frees */
/* copies the periods logged since the last read into done_masks / goal_masks [n_periods][n_waves] and empties the log */
int dql_episode_log_read(dql_ctx* ctx, uint64_t* done_masks, uint64_t* goal_masks, int32_t max_periods, int32_t* n_periods);
/* the same, restricted to the first n_words words (64 envs each) of every period: done_masks / goal_masks [n_periods][n_words].  The
 * promotion rule (pkg/trainer.py:218-232) judges a fixed few envs — the first global env ids —, the population's totals come from dql_stats_get. */
int dql_episode_log_read_words(dql_ctx* ctx, uint64_t* done_masks, uint64_t* goal_masks, int32_t max_periods, int32_t n_words, int32_t* n_periods);

/* ---- stateless batch operators (host arrays in/out, computed on the device; drop-in class methods) ---- */
/* TrainingMdp.discrete_state (pkg/mdp.py:257-333): 4 x double[n] -> packed idx int32[n]; -1 where the reference raises */
int dql_discretise(const dql_config* cfg, int device, const double* rel_p, const double* rel_v, const double* rel_a,
                   const double* angle, int64_t n, int32_t* idx_out);
/* TrainingMdp / SimulationMdp methods for n independent MDPs (pkg/mdp.py:257-560, 625-877).  `stages` selects which
 * of the reference's methods run in this call, in the reference's call order:
 *   DQL_MDP_ACTION (continuous_action) | DQL_MDP_DISCRETISE (discrete_state) | DQL_MDP_CHECK (check) | DQL_MDP_REWARD (reward)
 *   DQL_MDP_SIMULATION: SimulationMdp.check flavour (no goal / success logic, pkg/mdp.py:784-845)
 * mdp_state: double[8][n] in/out = angle set-point, shaping_p, shaping_v, shaping_a, cumulative, step_count,
 * curriculum_check, check_code; prev_idx int32[n] in (-1 = none); idx_io int32[n]: current packed state, written by
 * DISCRETISE and read by CHECK / REWARD; obs double[7][n] = rel_p (axis), rel_p (other axis), rel_v, rel_a, angle,
 * abs_p_z, contact */
enum { DQL_MDP_ACTION = 1, DQL_MDP_DISCRETISE = 2, DQL_MDP_CHECK = 4, DQL_MDP_REWARD = 8, DQL_MDP_SIMULATION = 16, DQL_MDP_ALL = 15 };
int dql_mdp_transition(const dql_config* cfg, int device, int64_t n, uint32_t stages, const uint8_t* action, const double* obs,
                       double* mdp_state, const int32_t* prev_idx, int32_t* idx_io, double* reward_out, uint8_t* done_out);
/* ManagerNode.publish_obs (scripts/manager_node.py:192-214, 292-310) + ObservationUtils.get_relative_state / get_observation
 * (pkg/observation_utils.py:77-158) replayed for n_series independent scripted series of n_ticks 100 Hz ticks, with the
 * device functions the fused step kernel runs.  in double[n_series][n_ticks][14] = drone p(3), v(3), quaternion w x y z (world
 * frame), platform x y u v as reported at that tick; contact uint8[n_series][n_ticks]; out double[n_series][n_ticks][12] =
 * observation p_x p_y v_x v_y a_x a_y, the v_z and yaw PID plant states, the platform set-point x y u v published by the tick.
 * Noise (cfg noise_*_sd > 0) comes from the Philox stream of (seed, series). */
int dql_manager_run(const dql_config* cfg, int device, int64_t n_series, int64_t n_ticks, const double* in, const uint8_t* contact,
                    uint64_t seed, double* out);
/* The plant of the fused step — what replaces Gazebo's motor-model plugin + ODE — replayed OPEN LOOP for n_series independent
 * series of n_ticks 500 Hz physics ticks, with the device functions the step kernel runs, in the kernel's order: rotation matrix of
 * the attitude quaternion; forces and moments of the CURRENT rotor speeds (thrust, rotor drag, rolling moment, drag torque:
 * rotors_gazebo_plugins/src/gazebo_motor_model.cpp:434-482) and one semi-implicit Euler step of the rigid body (dt, g:
 * worlds/basic.world:36-73); first-order rotor filter towards min(command, max_rot_velocity) (common.h:147-183,
 * gazebo_motor_model.cpp:358-364); platform extrapolation and the bumper-contact latch.  No controller, no MDP.
 * init double[n_series][21] = drone p(3), v(3), quaternion w x y z, body rates(3), rotor speeds(4), platform x y u v;
 * rotor_cmd double[n_series][n_ticks][4] commanded rotor speeds (rad/s, >= 0); out double[n_series][n_ticks][20] = p(3), v(3),
 * quaternion(4), body rates(3), rotor speeds(4), platform x y, contact latch (0 / 1) AFTER each tick.  Exists so that tests can hold
 * the plant against closed forms (tests/test_plant_closed_forms.py); Gazebo itself cannot run here (parity vs Gazebo: unpinned). */
int dql_plant_run(const dql_config* cfg, int device, int64_t n_series, int64_t n_ticks, const double* init, const double* rotor_cmd, double* out);
/* ---- the control-side functions of the 500 Hz / 100 Hz ticks replayed ALONE, one call per reference class method, with the device functions
 * the fused step kernel runs (float64: the reference's expressions operation by operation; float32: the forms every throughput figure runs on).
 * They exist so that each function can be held against the reference's own outputs (tests/golden G8, G9, G11) in BOTH dtypes ---- */
/* ButterworthFilter.update (pkg/filters.py:98-109) over x[n] from zero histories, c = cfg->bw_c */
int dql_butterworth_run(const dql_config* cfg, int device, const double* x, int64_t n, double* y_out);
/* KalmanFilter3D.filter (pkg/filters.py:53-80) over a velocity series vel[n][3] sampled at t = 0.01 i: z = dv / dt, dt <= 0 -> 0.01 (dt_le0[i] != 0
 * forces that branch), Q = cfg->kalman_q, R = cfg->noise_vel_sd^2 -> acc_out[n - 1][3] */
int dql_kalman_run(const dql_config* cfg, int device, const double* vel, const uint8_t* dt_le0, int64_t n, double* acc_out);
/* PID.output (pkg/pid.py:62-104) replayed over n 500 Hz ticks at t = 0.002 (i + 1); params[7] = Kp Ki Kd lower upper windup setpoint (Kd must be 0:
 * launch/drone.launch:37,51), state[n] sampled every 5th tick as the 100 Hz manager publishes it -> control effort and integral per tick */
int dql_pid_run(const dql_config* cfg, int device, const double* params, const double* state, int64_t n, double* effort_out, double* integral_out);
/* AttitudeController.compute_rotor_velocities (pkg/attitude_controller.py:107-156) for n samples: quat_xyzw[n][4] (ROS order), omega[n][3] body rates,
 * cmd[n][4] = roll, pitch, yaw rate, thrust -> rotor_out[n][4] commanded rotor speeds (rad/s).  xonly = 1 (float32 only, every roll command
 * exactly 0): the closed form the x-axis kernels compile in */
int dql_attitude_run(const dql_config* cfg, int device, const double* quat_xyzw, const double* omega, const double* cmd, int64_t n, int32_t xonly,
                     double* rotor_out);
/* MovingPlatform.compute_trajectory (pkg/moving_platform.py:87-127) from phase 0 -> out[n][4] = x, y, u, v at successive 100 Hz ticks.  carry > 0
 * (float32 only): sine / cosine evaluated at every carry-th tick and rotated through the constant phase step in between, as the fused float32
 * step carries them through the four or five manager ticks of an agent period */
int dql_platform_run(const dql_config* cfg, int device, int64_t n, int32_t carry, double* out);
/* start coordinate of the drone along one axis for n (random offset x0, platform coordinate) pairs: the placement arithmetic of
 * TrainingLandingEnv.reset / SimulationLandingEnv.reset selected by cfg->init_uniform (see dql_config) */
int dql_place(const dql_config* cfg, int device, const double* x0, const double* mp, int64_t n, double* out);
/* ---- greedy roll-outs: every env's FIRST episode from reset to termination in one launch, for up to 16 table sets at once ----
 * Table set k (qa / qb [n_tables][DQL_N_CELLS]) flies envs_per_table envs; env i of every set has the RNG key (i, seed) and the initial state of env i
 * of a context made with dql_create(cfg, device, envs_per_table, seed, 0), so the sets are compared on paired episodes.  Row (k, i) — output column
 * k * envs_per_table + i — is what that context, its tables set to set k and driven by dql_eval_steps(ctx, 1) once for the reset period and then max_steps
 * more times, shows at the first period after which env i is done: its terminal code, its step_count and the record fields of its state (the names:
 * dql_rollout_field_name), bit for bit in float32 and float64.  An env still in its first episode after max_steps periods has code -1 and the fields
 * of its state after the last period.
 *   code, steps  int32 [n_tables * envs_per_table];  rec  double [n_record][n_tables * envs_per_table]
 *   trace (trace_envs > 0): double [max_steps + 1][n_trace][trace_envs], the trace fields (the record's, then action, idx_x, idx_y) of the first
 *   trace_envs envs of table set 0 after every period they fly; rows after an env's last period are NaN.
 * DQL_EINVAL (and no launch) unless 1 <= n_tables <= DQL_ROLLOUT_MAX_TABLES, envs_per_table is a positive multiple of 64, 1 <= max_steps <=
 * DQL_ROLLOUT_MAX_STEPS, 0 <= trace_envs <= 64, a trace buffer comes with trace_envs > 0 and no other pointer is null. */
#define DQL_ROLLOUT_MAX_STEPS 4096
#define DQL_ROLLOUT_MAX_TABLES 16
int dql_rollout_n_fields(int32_t* n_record, int32_t* n_trace);
const char* dql_rollout_field_name(int32_t i, int32_t is_trace);
int dql_rollout(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, uint64_t seed, int32_t max_steps, const double* qa,
                const double* qb, int32_t* code, int32_t* steps, double* rec, int32_t trace_envs, double* trace_or_null);
/* ---- greedy scoring: how the episodes of up to 2^20 table sets end, counted on the device in one launch ----
 * Table set k (qa / qb [n_tables][DQL_N_CELLS]) flies envs_per_table envs as in dql_rollout (env i of every set has the RNG key (i, seed)), but an env does
 * not stop at its first episode: it flies on, through reset, until it has finished episodes_per_env episodes or max_steps periods are over.
 * The equality contract: take a context from dql_create(cfg, device, envs_per_table, seed, 0) with the tables of set k and drive it with
 * dql_eval_steps(ctx, 1) once for the reset period and then max_steps more times.  The m-th time (m = 0, 1, ... < episodes_per_env) env i shows FL_DONE after
 * a period, its code and its step_count are ep_code[m][k * envs_per_table + i] and ep_steps[m][k * envs_per_table + i] — whichever block or tick layout
 * that context picked —, and by_code[k] / steps_sum[k] are the sums of exactly those entries:
 *   by_code    int64 [n_tables][DQL_N_CHECK_CODES + 1]: finished episodes by terminal code; the last column, "unfinished", is envs_per_table *
 *              episodes_per_env minus the finished episodes
 *   steps_sum  int64 [n_tables]: the total length (step_count) of the finished episodes
 *   ep_code    uint8 [episodes_per_env][n_tables * envs_per_table], 0xff = not finished;  ep_steps uint16, same shape, 0 = not finished (both or neither)
 * The counts are integer sums: bit-reproducible.  With episodes_per_env = 1, code and steps are those of dql_rollout.  Episodes beyond the first are NOT
 * paired across table sets: when episode m starts depends on when episode m - 1 ended, and the Philox counter is the period index.
 * dql_ensemble_score (below, with the ensembles) scores the tables of an ensemble's learners where they live.
 * DQL_EINVAL (and no launch) unless 1 <= n_tables <= DQL_SCORE_MAX_TABLES, envs_per_table is a positive multiple of 64, n_tables * envs_per_table <= 2^30,
 * 1 <= episodes_per_env <= DQL_SCORE_MAX_EPISODES, 1 <= max_steps <= DQL_SCORE_MAX_STEPS, both log pointers are given or neither, and no other pointer is null. */
#define DQL_SCORE_MAX_TABLES (1 << 20)
#define DQL_SCORE_MAX_EPISODES 64
#define DQL_SCORE_MAX_STEPS 4096
int dql_score(const dql_config* cfg, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps,
              const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null);
/* ---- greedy scoring with a map: where the greedy policy of each table set flies, counted on the device in the same launch ----
 * dql_score_map flies exactly what dql_score flies: the table sets, the envs, the key (i, seed), max_steps, episodes_per_env and the schedules are the same, and
 * for equal arguments by_code, steps_sum, ep_code and ep_steps are equal to dql_score's.  It returns two more things.
 *   visits  int64 [n_tables][DQL_N_CELLS].  Take the stepwise context of dql_score's contract: dql_create(cfg, device, envs_per_table, seed, 0) with the tables
 *           of set k, then dql_eval_steps(ctx, 1) for periods 0 .. max_steps.  An env counts in a period if it has finished fewer than episodes_per_env
 *           episodes before that period and the period is not a reset period of that env (FL_WAS_RESET clear).  Each such period adds 1 at cell
 *           idx_x_before * 3 + (action & 3), where idx_x_before is the env's idx_x as it stood after the previous period; with two_axis it also adds 1 at
 *           idx_y_before * 3 + ((action >> 2) & 3) — the tables are shared between the axes, so the y decision lands in the same map.  A lane that has
 *           finished its episodes counts nothing more; decisions of episodes that max_steps cuts off are counted.  Integer sums: bit-reproducible.
 *   ep_last_cell  uint16 [2][episodes_per_env][n_tables * envs_per_table], optional (all three log arrays are given, or none).  Plane 0 holds the x cell of the
 *           decision made in the period in which the episode ended, plane 1 the y cell.  0xffff marks an episode that did not finish; plane 1 holds 0xffff
 *           everywhere under an x-only config.
 * dql_ensemble_score_map (below, with the ensembles) does the same on the tables of an ensemble's learners where they live.
 * DQL_EINVAL (and no launch) for whatever dql_score refuses, for a null visits, for a log of which only some arrays are given, and for n_tables >
 * DQL_SCORE_MAP_MAX_TABLES: the map is 22 680 B per set, so 2^14 sets are 372 MB on the device and on the host; the caller slices beyond that. */
#define DQL_SCORE_MAP_MAX_TABLES (1 << 14)
int dql_score_map(const dql_config* cfg, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps,
                  const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, int64_t* visits, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null,
                  uint16_t* ep_last_cell_or_null);
/* ---- the empirical transition model of the discretised x MDP, counted on the device in one launch ----
 * dql_model flies what dql_score flies — table set k, envs i with the RNG key (i, seed), periods 0 .. max_steps, every env until it has finished
 * episodes_per_env episodes — but the behaviour policy is eps-greedy on the fixed tables, and nothing is learnt.
 * The equality contract: take a context from dql_create(cfg, device, envs_per_table, seed, 0) and drive it with EXTERNAL actions through dql_step.  For env i
 * in period j, not a reset period of that env: w = philox((j_lo, j_hi, i, 0), (seed_lo, seed_hi)) (the action stream); the env explores iff (w[0] >> 8) <
 * ceil(eps 2^24), and its action is then (w[1] * 3) >> 32; otherwise its action is dql_agent_predict on the tables of set k at the env's idx_x.  An env counts
 * in a period exactly as in dql_score_map: it has finished fewer than episodes_per_env episodes before that period, and FL_WAS_RESET is clear after it.  With
 * cell = idx_x before the period * 3 + action, each counted period adds
 *   pairs      uint32 [n_tables][DQL_N_CELLS][DQL_N_STATES]: 1 at (cell, idx_x after the period) when the period did not end the episode
 *   terminal   int64 [n_tables][DQL_N_CELLS][DQL_N_CHECK_CODES]: 1 at (cell, code) when it did
 *   reward_fx  int64 [n_tables][DQL_N_CELLS]: the period's reward times 2^DQL_TARGET_FRAC_BITS, rounded to nearest even, at the cell (terminal periods included)
 *   by_code / steps_sum: as dql_score's
 * Everything is an integer sum: bit-reproducible, whatever order the lanes arrive in.  dql_ensemble_model (below, with the ensembles) does the same on the
 * tables of an ensemble's learners where they live.
 * DQL_EINVAL (and no launch) for a two_axis config (the model is the x MDP's; the reward is not kept per axis), n_tables outside 1..DQL_MODEL_MAX_TABLES (the
 * pair table is 10.7 MB per set), envs_per_table not a positive multiple of 64, envs_per_table * (max_steps + 1) >= 2^32 (below that no pair count can
 * overflow), episodes_per_env or max_steps outside dql_score's ranges, eps outside [0, 1], or a null pointer. */
#define DQL_MODEL_MAX_TABLES 16
int dql_model(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, double eps,
              const double* qa, const double* qb, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal, int64_t* by_code, int64_t* steps_sum);
/* ---- the transition model split by one bit of hidden state ----
 * dql_model_split flies exactly what dql_model flies with the same arguments — the envs and their RNG keys, period_begin's own eps-greedy rule, which periods
 * count — and `feature` and `cut` have no influence on any flight.  For every counted decision of an env, `value` is the selected feature read from the env AS
 * IT STANDS BEFORE THE PERIOD (the state the decision was taken in), widened to double (a float32 value widens exactly), and half = (value >= cut[idx_x before
 * the period]) ? 1 : 0, compared in double.  The outputs, all integer sums, bit-reproducible whatever order the lanes arrive in:
 *   pairs        uint32 [n_tables][2][DQL_N_CELLS][DQL_N_STATES]      as dql_model's, the half as the second index
 *   terminal     int64 [n_tables][2][DQL_N_CELLS][DQL_N_CHECK_CODES]  as dql_model's, the half as the second index
 *   reward_fx    int64 [n_tables][2][DQL_N_CELLS]                     as dql_model's, the half as the second index
 *   feat_sum_fx  int64 [n_tables][DQL_N_STATES]                       per state before the period and per counted decision, rint(value * 2^DQL_SPLIT_FRAC_BITS):
 *                the product is exact in double, the rounding is to nearest even; the per-state mean is feat_sum_fx / 2^20 / visits of the state
 *   by_code / steps_sum: as dql_model's
 * The two halves of pairs, terminal and reward_fx sum to dql_model's.  The features (the names in parentheses are dql_field_name's):
 *   DQL_SPLIT_COIN 0         0.0 or 1.0, a coin that reads nothing of the env (use cut = 0.5 everywhere): with j the period's index, x = env_id * 0x9E3779B1 +
 *                            (uint32)j * 0x85EBCA77 + (uint32)seed in 32-bit unsigned arithmetic, then x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13;
 *                            x *= 0xC2B2AE35; x ^= x >> 16; the value is x >> 31.  It gives the sampling floor for exactly the same sample sizes
 *   DQL_SPLIT_OBS_P_X 1 (obs_p_x)   DQL_SPLIT_OBS_V_X 2 (obs_v_x)   DQL_SPLIT_OBS_A_X 3 (obs_a_x)   DQL_SPLIT_PITCH_SP 4 (pitch_sp: the continuous set-point)
 *   DQL_SPLIT_MP_PHASE 5 (mp_phase) DQL_SPLIT_MP_U 6 (mp_u)         DQL_SPLIT_ALTITUDE 7 (pz)       DQL_SPLIT_V_Z 8 (vz)
 *   DQL_SPLIT_STEP 9         step_count & 0xffff
 *   DQL_SPLIT_PREV_ACTION 10 action & 3 as it stands: the previous decision's action, or whatever reset left
 * A value that is not finite or has |value| >= 8192, or a half outside {0, 1}, is a fault like an index out of range: the period's whole contribution is
 * dropped and counted, and the call returns DQL_ESTATE and no result.
 * DQL_EINVAL (and no launch, no buffer touched): everything dql_model refuses, with n_tables outside 1..DQL_MODEL_SPLIT_MAX_TABLES (21.4 MB of pair table per
 * set) and envs_per_table * (max_steps + 1) >= 2^30 (below that feat_sum_fx cannot overflow: 2^33 * 2^30) in place of dql_model's bounds; feature outside
 * 0..10; a null cut or feat_sum_fx; a NaN in cut (+-inf are allowed and meaningful: with +inf everything is in half 0). */
#define DQL_MODEL_SPLIT_MAX_TABLES 8
#define DQL_SPLIT_FRAC_BITS 20
#define DQL_SPLIT_N_FEATURES 11
enum { DQL_SPLIT_COIN = 0, DQL_SPLIT_OBS_P_X = 1, DQL_SPLIT_OBS_V_X = 2, DQL_SPLIT_OBS_A_X = 3, DQL_SPLIT_PITCH_SP = 4, DQL_SPLIT_MP_PHASE = 5, DQL_SPLIT_MP_U = 6,
       DQL_SPLIT_ALTITUDE = 7, DQL_SPLIT_V_Z = 8, DQL_SPLIT_STEP = 9, DQL_SPLIT_PREV_ACTION = 10 };
int dql_model_split(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, double eps,
                    int32_t feature, const double* cut /* [DQL_N_STATES] */, const double* qa, const double* qb, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal,
                    int64_t* feat_sum_fx, int64_t* by_code, int64_t* steps_sum);
/* ---- realised discounted returns per (state, action) cell, to be held against the Q tables ----
 * dql_returns flies exactly what dql_model flies, counted the same way: table set k, env i with the RNG key (i, seed), periods 0 .. max_steps, the eps-greedy
 * rule of dql_model's contract on the fixed tables (eps = 0: the greedy policy), and an env counts in a period as in dql_score_map.  Take the counted decisions
 * of env i in period order; each carries a cell c_t = idx_x before the period * 3 + action, the period's reward_fx r_t (int64: reward * 2^26 rounded to nearest
 * even, as dql_model has it) and the flag "this period ended the episode".  For every episode of the env that FINISHED, with decisions t = 0 .. L - 1, the
 * return-to-go in units of 2^-26 is defined backwards in IEEE double: g_L = 0.0, g_t = (double)r_t + (gamma * g_{t+1}) — two operations, each rounded to
 * nearest, never fused.  Decision t then adds
 *   visits         int64 [n_tables][DQL_N_CELLS]: 1 at c_t
 *   return_fx      int64 [n_tables][DQL_N_CELLS]: llrint(g_t) at c_t (round to nearest even)
 * Decisions of an episode that max_steps cuts off contribute to neither (their return is not known); they are counted in
 *   cut_decisions  int64 [n_tables]
 * by_code / steps_sum are dql_score's and, for equal arguments, dql_model's; visits.sum() + cut_decisions equals dql_model's visits.sum().  Integer sums of
 * per-lane deterministic values: bit-reproducible in any arrival order.  gamma is an argument, not cfg->gamma.
 * DQL_EINVAL (and no launch) for a two_axis config, n_tables outside 1..DQL_SCORE_MAP_MAX_TABLES, envs_per_table not a positive multiple of 64,
 * episodes_per_env or max_steps outside dql_score's ranges, eps or gamma outside [0, 1] (NaN included), a null pointer, n_tables * envs_per_table *
 * (max_steps + 1) > 2^29 (the decision log is one 64-bit word per possible decision: 4 GiB there), and when one int64 cell of return_fx could overflow: with R
 * the per-step reward bound of the config (26.0 by default) and B = R min(1 / (1 - gamma), max_steps + 1) (1 + 2^-10), when (ceil(B 2^26) + 1) *
 * envs_per_table * (max_steps + 1) > 2^63 - 1.  Sums of several calls with different seeds add: the caller slices.  DQL_ESTATE (no result) if a range check
 * in the kernels dropped a contribution. */
int dql_returns(const dql_config* cfg, int device, int32_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, double eps,
                double gamma, const double* qa, const double* qb, int64_t* visits, int64_t* return_fx, int64_t* cut_decisions, int64_t* by_code, int64_t* steps_sum);
/* ---- greedy scoring over a grid of scenarios: S configs x K table sets in one launch, with the landing precision of the touchdowns ----
 * The equality contract: slice s of every output is what dql_score(&cfgs[s], ...) returns for the same remaining arguments — in turn the stepwise context of
 * dql_score's own contract: dql_create(&cfgs[s], device, envs_per_table, seed, 0) with the tables of set k, then dql_eval_steps(ctx, 1) for periods 0 ..
 * max_steps.  Env i of every (scenario, set) has the key (i, seed): first episodes are paired across table sets and across scenarios.
 *   by_code    int64 [n_scenarios][n_tables][DQL_N_CHECK_CODES + 1];  steps_sum  int64 [n_scenarios][n_tables]
 *   ep_code    uint8 [n_scenarios][episodes_per_env][n_tables * envs_per_table];  ep_steps uint16, same shape (both or neither)
 *   touch_hist int64 [n_scenarios][n_tables][DQL_GRID_TOUCH_BINS], optional, the only output dql_score has no counterpart for.  It counts, among the first
 *              episodes_per_env episodes of an env, those that end with DQL_TERMINAL_CONTACT, binned by d, the drone's horizontal offset from the platform
 *              centre after the terminal period: d = |px - mp_x| in the config's real type T, on the values dql_rollout's record shows as px and mp_x at that
 *              period; with two_axis d = max(|px - mp_x|, |py - mp_y|) (the platform is a square).  bin = the number of j in 1..7 with d >= edge_j, edge_j =
 *              (T)((double)j * cfgs[s].mp_half_x * 0.25): bins 0 - 3 lie inside the half extent, bins 4 - 7 beyond it (they do occur: the contact latch is set
 *              at a physics tick, the offset is read at the period's end).  A NaN offset falls into bin 0.  Integer sums: bit-reproducible.
 * The scenarios may differ in anything except what one launch must share: dtype and two_axis (they fix the kernel instance) and f_ag, dt and manager_div (they
 * fix the tick schedule, which is uploaded once).  dql_ensemble_score_grid (below, with the ensembles) does the same on an ensemble's resident tables.
 * DQL_EINVAL (and no launch, outputs untouched), in a sentence that names the scenario where there is one: n_scenarios outside 1..DQL_GRID_MAX_SCENARIOS, a
 * scenario that is not a valid config, a scenario that differs from scenario 0 in one of the five shared fields, n_scenarios * n_tables * envs_per_table >
 * 2^30, whatever dql_score refuses, a log of which only one array is given, a null cfgs, qa, qb, by_code or steps_sum. */
#define DQL_GRID_MAX_SCENARIOS 1024
#define DQL_GRID_TOUCH_BINS 8
int dql_score_grid(const dql_config* cfgs /* [n_scenarios] */, int32_t n_scenarios, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env,
                   uint64_t seed, int32_t max_steps, const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum, int64_t* touch_hist_or_null,
                   uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null);
/* ---- a DoubleQLearningAgent's tables RESIDENT on the device (pkg/double_q_learning.py:32-146) ----
 * The stateless dql_agent_predict / dql_agent_update below ship all three tables (3 x 22 680 B) both ways per call — fine for a batch,
 * 6x slower than the reference's own Python for a caller that steps ONE env (BASELINE configs[0]).  A dql_agent keeps them in device
 * memory between calls; arguments and results travel through pinned host memory the kernels read and write directly (one launch
 * and one wait per call, no allocation, no copy engine).  dql_agent_update_resident returns, per transition, the new value of the
 * updated cell and of its visit counter, so the caller can patch its host copy of the tables instead of fetching them. */
typedef struct dql_agent dql_agent;
int dql_agent_create(int device, dql_agent** out);
int dql_agent_destroy(dql_agent* agent);
int dql_agent_set_tables(dql_agent* agent, const double* qa_or_null, const double* qb_or_null, const double* count_or_null);
int dql_agent_get_tables(dql_agent* agent, double* qa_or_null, double* qb_or_null, double* count_or_null);
int dql_agent_predict_resident(dql_agent* agent, const int32_t* idx, int64_t n, uint8_t* action_out);
int dql_agent_update_resident(dql_agent* agent, const int32_t* sa, const int32_t* ns, const double* alpha, double gamma, const double* reward,
                              int64_t n, uint32_t quirks, const uint8_t* coin_or_null, const uint8_t* done_or_null, double* q_new_out,
                              double* count_new_out, uint8_t* next_action_out_or_null /* predict(ns[n-1]) on the updated tables: the
                              reference's loop (pkg/trainer.py:191-212) asks for exactly that next, and gets it without a second round trip */);
/* The resident agent driven the way the reference's loop drives it (pkg/trainer.py:191-212) — ONE transition per call — against tables
 * that live in the CALLER's arrays (DoubleQLearningAgent.Q_table_a / Q_table_b / state_action_counter: float64, C order,
 * [n_levels][3][3][3][7][3], public and writable at any time).  Every call first compares the caller's three arrays with what the device
 * holds (memcmp against a pinned host shadow, ~1 us per table) and uploads what differs: writes between calls are honoured without a
 * dirty flag.  dql_agent_mirror_update applies pkg/double_q_learning.py:91-146 to the one transition (sa = cell index idx * 3 + action,
 * ns = packed next state; quirks / coin / done as in dql_agent_update) and patches the ONE changed cell and its visit counter into the
 * caller's arrays itself; it also keeps predict(ns) on the updated tables, which dql_agent_mirror_predict hands out without a device round
 * trip when asked for exactly that state next (as the reference's loop does) and the tables were not written in between.
 * Levels n_levels..4 of the device tables are zero.  DQL_EINVAL: null array, n_levels outside 1..5, index outside the n_levels levels. */
int dql_agent_mirror_predict(dql_agent* agent, const double* qa, const double* qb, const double* count, int32_t n_levels, int32_t idx, uint8_t* action_out);
int dql_agent_mirror_update(dql_agent* agent, double* qa, double* qb, double* count, int32_t n_levels, int32_t sa, int32_t ns, double alpha,
                            double gamma, double reward, uint32_t quirks, int32_t coin, int32_t done);
/* The same update in two halves (ABI v6): _deferred launches the kernel and returns — the caller's arrays still hold the OLD cell; dql_agent_mirror_complete, or the next
 * call of any kind on this agent, waits for the kernel and patches the cell and its visit counter in (into the arrays that were passed to _deferred: they must stay alive
 * until then).  For a host loop that has other work between update() and the next guess() (the reference's has: pkg/trainer.py:204-212) the kernel's round trip hides
 * behind that work.  dql_agent_mirror_update == _deferred + _complete. */
int dql_agent_mirror_update_deferred(dql_agent* agent, double* qa, double* qb, double* count, int32_t n_levels, int32_t sa, int32_t ns, double alpha,
                                     double gamma, double reward, uint32_t quirks, int32_t coin, int32_t done);
int dql_agent_mirror_complete(dql_agent* agent);
/* DoubleQLearningAgent.predict (pkg/double_q_learning.py:119-124) for n packed states */
int dql_agent_predict(int device, const double* qa, const double* qb, const int32_t* idx, int64_t n, uint8_t* action_out);
/* DoubleQLearningAgent.update (pkg/double_q_learning.py:91-146) replayed strictly in order for n transitions:
 * sa int32[n] = cell index (idx*3+action), ns int32[n] = packed next state; tables updated in place.
 * quirks: DQL_Q_UPDATE_TABLE_A_ONLY (B1/B2) = the reference: always Q_table_a, valued by itself; cleared = Double Q-learning:
 * coin[i] (required then: 0 -> Q_table_a, 1 -> Q_table_b; the caller draws it where the reference draws its unused uniform)
 * picks the table to update and the OTHER table values the picked table's greedy action at s'.
 * DQL_Q_BOOTSTRAP_ON_POS_CHANGE (B3) = bootstrap only when the position bin changed; cleared = bootstrap unless done[i]
 * (required then).  Other quirk bits do not concern the agent and are ignored. */
int dql_agent_update(int device, double* qa, double* qb, double* count, const int32_t* sa, const int32_t* ns,
                     const double* alpha, double gamma, const double* reward, int64_t n, uint32_t quirks,
                     const uint8_t* coin_or_null, const uint8_t* done_or_null);

/* DoubleQLearningAgent.transfer_learning (pkg/double_q_learning.py:77-89) on host tables: Q[k] = Q[k-1] * ratio (k = 0 wraps, B6) */
int dql_agent_transfer(int device, double* qa, double* qb, int32_t k, double ratio);

/* ---- populations: K independent agents in one context, stepped by one launch ----
 * Agent k owns envs [k E, (k+1) E) (E = envs_per_agent, a multiple of 512) and has its own Q tables, visit counters, accumulators,
 * curriculum level, seed, step index, statistics and exploration rate.  Agent k is bit-identical to a context made with
 * dql_create(cfg, device, E, seeds[k], env_id_offset = 0) and driven through the same per-agent calls; launches in which it is inactive
 * do not touch it (the stand-alone context skips them).
 * Whole-context calls act on all K E envs in agent-major order: dql_reset, dql_get_states / rewards / dones / actions / obs,
 * dql_step_outputs, dql_get/set_sim_state, dql_get/set_sim_ints, dql_episode_log_* (a period row spans all K E envs; agent k's rows
 * are its own periods since the last read, words of agents that ran fewer periods are 0), dql_set_option (periods_per_launch, block,
 * tick), dql_set_alpha_table (every agent), dql_flush (every agent), dql_stats_reset (every agent), dql_sync, dql_n_envs, dql_destroy.
 * With n_agents > 1 the single-agent calls (dql_train_steps, dql_eval_steps, dql_get/set_tables, dql_transfer, dql_set_curriculum,
 * dql_publish_tables, dql_stats_get, dql_get/set_step_index) return DQL_EINVAL naming their dql_pop_* form; with n_agents == 1 they act
 * on agent 0.  External actions (dql_step, dql_step_dev) and everything windowed, RCCL or peer-to-peer are refused on every population.
 * active_or_null: uint8[n_agents], non-zero = step this agent (null = all).  eps: double[n_agents]. */
#define DQL_MAX_AGENTS 16
int dql_pop_create(const dql_config* cfg, int device, int32_t n_agents, int64_t envs_per_agent, const uint64_t* seeds, dql_ctx** out);
int dql_pop_n_agents(dql_ctx* ctx, int32_t* n);
int dql_pop_train_steps(dql_ctx* ctx, int32_t n_steps, const double* eps, const uint8_t* active_or_null);
int dql_pop_eval_steps(dql_ctx* ctx, int32_t n_steps, const uint8_t* active_or_null);
int dql_pop_set_curriculum(dql_ctx* ctx, int32_t agent, int32_t level); /* flush, publish, level, reset of that agent's envs only */
int dql_pop_get_tables(dql_ctx* ctx, int32_t agent, double* qa, double* qb, double* count);
int dql_pop_set_tables(dql_ctx* ctx, int32_t agent, const double* qa, const double* qb, const double* count);
int dql_pop_transfer(dql_ctx* ctx, int32_t agent, int32_t k, double ratio);
int dql_pop_publish_tables(dql_ctx* ctx, int32_t agent);
int dql_pop_stats_get(dql_ctx* ctx, int32_t agent, dql_stats* out);
int dql_pop_get_step_index(dql_ctx* ctx, int32_t agent, int64_t* j);
int dql_pop_set_step_index(dql_ctx* ctx, int32_t agent, int64_t j);
int dql_pop_index_faults(dql_ctx* ctx, int32_t agent, int64_t* n); /* targets dropped by the step kernel's bounds guard (0 unless a bug) */

/* ---- ensembles of sequential learners: L independent Double-Q learners with ONE env each, stepped by one launch ----
 * Learner l owns env l of a context made with dql_create(cfg, device, n_learners, seed, 0) and its own Q_table_a, Q_table_b and
 * state_action_counter.  All learners share the period index j (period 0 is the reset period; a learner whose episode ended in period j
 * resets in period j + 1).  In a non-reset period a learner explores iff its action word says so against ITS eps threshold (the eps table
 * at min(e, n_eps - 1), e = episodes it has finished at the current level), else acts greedily on its CURRENT tables; right after the
 * period it applies DoubleQLearningAgent.update (pkg/double_q_learning.py:91-146: learning rate from the alpha table at the pre-increment
 * count, alpha_min of the config beyond it; quirks as in dql_agent_update) to its own cells.  No accumulators, no fold, no delay: the
 * reference's loop (pkg/trainer.py:187-236), bit for bit in float32 and float64.
 * A learner FREEZES (env, tables and counters untouched until re-armed) when the successes among its last `window` episodes at this level
 * reach min_successes (promotion: the reference's window = 100, min_successes = 97) or when it has finished max_episodes at this level.
 * Tables: double [n_learners][DQL_N_CELLS] each, whole or the slice [first, first + count) of the learners.
 * Two-axis configs and the figure-eight trajectory are refused.  Every refused call returns DQL_EINVAL with a message and launches nothing. */
#define DQL_ENSEMBLE_MAX_PERIODS 4096   /* agent periods per kernel launch; the run call loops launches for longer runs */
#define DQL_ENSEMBLE_MAX_WINDOW 128
#define DQL_ENSEMBLE_MAX_LEARNERS (1 << 20)
#define DQL_ENSEMBLE_MAX_LOG (1 << 20)
typedef struct dql_ensemble dql_ensemble;
/* log_capacity > 0: keep terminal code and length of every learner's first log_capacity episodes (later ones are counted, not logged) */
int dql_ensemble_create(const dql_config* cfg, int device, int64_t n_learners, uint64_t seed, int32_t log_capacity, dql_ensemble** out);
int dql_ensemble_destroy(dql_ensemble* ens);
int dql_ensemble_n_learners(dql_ensemble* ens, int64_t* n);
/* alpha double[n_alpha], eps double[n_eps] (turned into thresholds as the step kernel's eps is); window in 1..DQL_ENSEMBLE_MAX_WINDOW */
int dql_ensemble_set_schedules(dql_ensemble* ens, const double* alpha, int32_t n_alpha, const double* eps, int32_t n_eps, int32_t window,
                               int32_t min_successes, int32_t max_episodes);
/* new working level for all learners: every env re-enters through reset, then dql_ensemble_rearm */
int dql_ensemble_set_level(dql_ensemble* ens, int32_t level);
/* clears the per-level episode counts, windows, promotion records and frozen flags of all learners */
int dql_ensemble_rearm(dql_ensemble* ens);
/* `periods` agent periods for every learner that is not frozen; two runs of a and b periods equal one run of a + b, bit for bit */
int dql_ensemble_run(dql_ensemble* ens, int64_t periods);
int dql_ensemble_get_period_index(dql_ensemble* ens, int64_t* j);
int dql_ensemble_n_live(dql_ensemble* ens, int64_t* n_live); /* learners not frozen */
/* dql_agent_transfer's arithmetic on every learner's tables: Q[k] = Q[k-1] * ratio, k = 0 wraps (B6) */
int dql_ensemble_transfer(dql_ensemble* ens, int32_t k, double ratio);
int dql_ensemble_get_tables(dql_ensemble* ens, int64_t first, int64_t count, double* qa_or_null, double* qb_or_null, double* count_or_null);
int dql_ensemble_set_tables(dql_ensemble* ens, int64_t first, int64_t count, const double* qa_or_null, const double* qb_or_null,
                            const double* count_or_null);
/* per learner: decisions, episodes, successes int64[n]; by_code int64[DQL_N_CHECK_CODES][n] (all since creation); promoted int32[n] = number of
 * episodes at this level when the window filled, or -1; level_episodes int32[n]; frozen uint8[n] */
int dql_ensemble_get_counters(dql_ensemble* ens, int64_t* decisions, int64_t* episodes, int64_t* successes, int64_t* by_code, int32_t* promoted,
                              int32_t* level_episodes, uint8_t* frozen);
/* code uint8[n][capacity], length uint16[n][capacity], n_episodes int32[n] (counts on beyond capacity); capacity = the creation's log_capacity */
int dql_ensemble_get_episode_log(dql_ensemble* ens, uint8_t* code, uint16_t* length, int32_t capacity, int32_t* n_episodes);
/* env state after the last period in the layout of dql_get_sim_state / dql_get_sim_ints (names: dql_field_name): reals double[64][n], ints int32[7][n];
 * the x-axis fields are live, those of the y axis keep their initial values */
int dql_ensemble_get_state(dql_ensemble* ens, double* reals, int32_t* ints);
int dql_ensemble_index_faults(dql_ensemble* ens, int64_t* n); /* updates dropped by the kernel's bounds guard (0 unless a bug) */
/* dql_score on the tables of learners [first, first + count), read in the ensemble's device memory (no host copy): table set k is learner first + k, outputs
 * and refusals as for dql_score (count in place of n_tables; the slice must lie inside the ensemble).  eval_cfg is any valid config and need not be the
 * ensemble's own (another level, the simulation flavour, two axes, the other dtype).  The ensemble is left exactly as it was: env state, tables, counters,
 * windows and period index. */
int dql_ensemble_score(dql_ensemble* ens, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env,
                       uint64_t seed, int32_t max_steps, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null);
/* dql_score_map on the tables of learners [first, first + count), as dql_ensemble_score is dql_score on them: outputs and refusals as for dql_score_map (count
 * in place of n_tables; the slice must lie inside the ensemble).  The ensemble is left exactly as it was. */
int dql_ensemble_score_map(dql_ensemble* ens, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env,
                           uint64_t seed, int32_t max_steps, int64_t* by_code, int64_t* steps_sum, int64_t* visits, uint8_t* ep_code_or_null,
                           uint16_t* ep_steps_or_null, uint16_t* ep_last_cell_or_null);
/* dql_model on the tables of learners [first, first + count), as dql_ensemble_score_map is dql_score_map on them: outputs and refusals as for dql_model (count
 * in place of n_tables, so count <= DQL_MODEL_MAX_TABLES; the slice must lie inside the ensemble).  The ensemble is left exactly as it was. */
int dql_ensemble_model(dql_ensemble* ens, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env,
                       uint64_t seed, int32_t max_steps, double eps, uint32_t* pairs, int64_t* reward_fx, int64_t* terminal, int64_t* by_code,
                       int64_t* steps_sum);
/* dql_model_split on the tables of learners [first, first + count): outputs and refusals as for dql_model_split (count in place of n_tables, so count <=
 * DQL_MODEL_SPLIT_MAX_TABLES; the slice must lie inside the ensemble).  The ensemble is left exactly as it was. */
int dql_ensemble_model_split(dql_ensemble* ens, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env,
                             uint64_t seed, int32_t max_steps, double eps, int32_t feature, const double* cut, uint32_t* pairs, int64_t* reward_fx,
                             int64_t* terminal, int64_t* feat_sum_fx, int64_t* by_code, int64_t* steps_sum);
/* dql_returns on the tables of learners [first, first + count): outputs and refusals as for dql_returns (count in place of n_tables; the slice must lie
 * inside the ensemble).  The ensemble is left exactly as it was. */
int dql_ensemble_returns(dql_ensemble* ens, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env,
                         uint64_t seed, int32_t max_steps, double eps, double gamma, int64_t* visits, int64_t* return_fx, int64_t* cut_decisions,
                         int64_t* by_code, int64_t* steps_sum);
/* dql_score_grid on the tables of learners [first, first + count): outputs and refusals as for dql_score_grid (count in place of n_tables; the slice must lie
 * inside the ensemble).  The ensemble is left exactly as it was. */
int dql_ensemble_score_grid(dql_ensemble* ens, const dql_config* eval_cfgs /* [n_scenarios] */, int32_t n_scenarios, int64_t first, int64_t count,
                            int64_t envs_per_learner, int32_t episodes_per_env, uint64_t seed, int32_t max_steps, int64_t* by_code, int64_t* steps_sum,
                            int64_t* touch_hist_or_null, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null);

/* ---- a state split by one bit of hidden state: refined learners and their greedy scoring ----
 * The refined state is r = half * DQL_N_STATES + idx_x and its cell r * 3 + action: a refined table set is double [2][DQL_N_CELLS], the half the slow index
 * (DQL_N_STATES is a multiple of 189 and of 63, so (r / 63) % 3 is still the position bin, and dql_agent_update / dql_agent_predict on tables of
 * 2 * DQL_N_CELLS entries are the yardstick).  The half of the decision taken in period j is dql_model_split's, decision for decision:
 *   value = the feature (DQL_SPLIT_*) read from the env as it stands BEFORE period j, widened to double; the coin's j is the period index truncated to 32
 *           bits, its env id the learner's or env's index, its seed the low 32 bits of the seed
 *   half  = value >= cut[idx_x before period j] ? 1 : 0, compared in double
 * so after period j ends (reset periods included) the half of the state the env is now in follows from the env as it stands, with j + 1.  A value that is not
 * finite or has |value| >= 8192 is a fault: a learner takes the half as 0, drops the update of the decision taken in that state and counts it in
 * dql_ensemble_index_faults; a scoring call returns DQL_ESTATE and no result.
 *
 * dql_ensemble_set_refinement: accepted only on an ensemble made by dql_ensemble_create (no teams), at period index 0, with no recipes, curriculum mode or n-step
 * targets installed, and once; feature in 0..10, cut double[DQL_N_STATES] without NaN (+-inf are meaningful: +inf puts everything in half 0, -inf in half 1).
 * It allocates zeroed refined tables and counts, [n_learners][2][DQL_N_CELLS] each; the plain arrays stay allocated and are never read again.  From then on
 * dql_ensemble_run flies the refined learner: the eps-greedy choice reads the row of r, the update is DoubleQLearningAgent.update on cell r * 3 + action with
 * the row of r' read before the write and the learning rate at the refined cell's pre-increment count; coin, quirks, mask, books, ring, freeze and log are the
 * plain learner's, and two runs of a and b periods still equal one run of a + b.  dql_ensemble_set_schedules, _set_level, _rearm, _run, _get_counters,
 * _get_episode_log, _get_state, _n_live and _get_period_index work unchanged; dql_ensemble_transfer applies its arithmetic to both halves.
 * Refused on a refined ensemble with DQL_EINVAL and a sentence that names the call to use (nothing launched, no buffer touched): dql_ensemble_get_tables /
 * _set_tables, _score, _score_map, _model, _model_split, _returns, _score_grid, _set_curriculum, _set_recipes and the per-recipe calls, _set_nstep, _set_team_nstep
 * and _set_team_curriculum.  dql_ensemble_score_refined, _get_refined_tables and _set_refined_tables are refused on an ensemble without a refinement.
 * dql_ensemble_get_refinement: the feature, or -1 without a refinement; cut_or_null receives the cut when there is one. */
#define DQL_SCORE_REFINED_MAX_TABLES 4096 /* dql_score_refined uploads 2 x 2 x 22 680 B per table set: 372 MB at the bound */
int dql_ensemble_set_refinement(dql_ensemble* ens, int32_t feature, const double* cut /* [DQL_N_STATES] */);
int dql_ensemble_get_refinement(dql_ensemble* ens, int32_t* feature_or_minus1, double* cut_or_null /* [DQL_N_STATES] */);
/* the refined tables of learners [first, first + count), double [count][2][DQL_N_CELLS] each, sliced like dql_ensemble_get_tables / _set_tables; each array optional */
int dql_ensemble_get_refined_tables(dql_ensemble* ens, int64_t first, int64_t count, double* qa_or_null, double* qb_or_null, double* count_or_null);
int dql_ensemble_set_refined_tables(dql_ensemble* ens, int64_t first, int64_t count, const double* qa_or_null, const double* qb_or_null,
                                    const double* count_or_null);
/* dql_score on refined table sets qa / qb double [n_tables][2][DQL_N_CELLS]: the same envs (key (i, seed), periods 0..max_steps, episodes through reset), the
 * greedy row that of r by the half rule above.  Outputs and refusals are dql_score's, plus DQL_EINVAL for a two-axis config, the figure-eight trajectory (the
 * ensembles refuse both: the refinement is the x MDP's), a feature outside 0..10, a null cut or a NaN in it, and n_tables above DQL_SCORE_REFINED_MAX_TABLES. */
int dql_score_refined(const dql_config* cfg, int device, int64_t n_tables, int64_t envs_per_table, int32_t episodes_per_env, uint64_t seed, int32_t max_steps,
                      int32_t feature, const double* cut /* [DQL_N_STATES] */, const double* qa, const double* qb, int64_t* by_code, int64_t* steps_sum,
                      uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null);
/* dql_score_refined on the refined tables of learners [first, first + count) where they live, with the ensemble's own feature and cut (count in place of
 * n_tables, up to DQL_SCORE_MAX_TABLES: nothing is uploaded; the slice must lie inside the ensemble).  The ensemble is left byte for byte as it was. */
int dql_ensemble_score_refined(dql_ensemble* ens, const dql_config* eval_cfg, int64_t first, int64_t count, int64_t envs_per_learner, int32_t episodes_per_env,
                               uint64_t seed, int32_t max_steps, int64_t* by_code, int64_t* steps_sum, uint8_t* ep_code_or_null, uint16_t* ep_steps_or_null);

/* ---- per-learner curriculum levels ----
 * Every learner has its own working level (it starts at the config's working_curriculum_step; dql_ensemble_set_level sets everybody's and clears the history
 * from that level on).  CURRICULUM MODE — off by default, and while it is off every call above behaves as described there — lets a learner walk the levels by
 * itself.  At a period index j that is a multiple of advance_every, before period j is flown and nowhere else (dql_ensemble_run cuts its launches there),
 * every frozen learner below last_level that promoted, or that ran out of episodes while advance_exhausted is 1, records its history entry, applies
 * dql_ensemble_transfer's arithmetic for k = its finished level with ratios[k] to ITS OWN two tables (the k = 0 wrap included), moves up one level,
 * re-enters through reset and has its per-level counters, window, promotion record and frozen flag cleared.  A learner frozen at last_level — or out of
 * episodes with advance_exhausted 0 — is finished and never touched again.  Between advance points a learner flies as described above with ITS level's
 * limits, exploration table, window, min_successes and max_episodes (dql_ensemble_set_level_schedules; the learning rates stay those of
 * dql_ensemble_set_schedules); the RNG key stays (learner, seed).  Advance points depend on j only: two runs of a and b periods equal one run of a + b bit
 * for bit, and a learner's whole history is independent of which other learners exist.  promoted / level_episodes of dql_ensemble_get_counters refer to
 * each learner's current level.
 * Refused with DQL_EINVAL, a message and no launch: advance_every outside 0..4096, last_level below a learner's current level or above 4, a ratio that is
 * not finite, advance_exhausted other than 0 / 1, a level outside 0..4, schedule arguments dql_ensemble_set_schedules refuses, and dql_ensemble_run in
 * curriculum mode before every level from the learners' up to last_level has its schedules (a learner's own level first, whatever last_level is); also
 * dql_ensemble_set_level above last_level while the mode is on, and advance_every = 0 while learners stand on different levels (the plain launch flies
 * everyone at the config's level: dql_ensemble_set_level first). */
/* ratios double[5]: ratios[k] is applied when level k is finished; advance_every = 0 turns the mode off (the other arguments are then ignored) */
int dql_ensemble_set_curriculum(dql_ensemble* ens, int32_t last_level, int32_t advance_every, const double* ratios, int32_t advance_exhausted);
/* eps double[n_eps] per episode index within the level, window / min_successes / max_episodes as in dql_ensemble_set_schedules, for one level */
int dql_ensemble_set_level_schedules(dql_ensemble* ens, int32_t level, const double* eps, int32_t n_eps, int32_t window, int32_t min_successes,
                                     int32_t max_episodes);
/* level int32[n]; per level k and learner: promoted_at int32[5][n] (episode at level k at which the window filled, or -1), episodes_at int32[5][n] (episodes
 * spent at level k), entered_period int64[5][n] (period index at which level k was entered, or -1).  The row of a learner's current level shows its counters
 * as they stand. */
int dql_ensemble_get_levels(dql_ensemble* ens, int32_t* level, int32_t* promoted_at, int32_t* episodes_at, int64_t* entered_period);
/* learners that still have something to fly or a level to advance to; with the mode off: dql_ensemble_n_live */
int dql_ensemble_n_unfinished(dql_ensemble* ens, int64_t* n);

/* ---- per-learner recipes ----
 * In curriculum mode an ensemble can hold up to DQL_ENSEMBLE_MAX_RECIPES recipes, and every learner belongs to one of them (recipe_of[l]).  A recipe holds
 * what every learner of an ensemble otherwise shares: the quirk word (it replaces the config's for the recipe's learners, env side and update), the
 * learning-rate table and alpha_min, per level 0..4 the exploration table, window, min_successes and max_episodes, and the rule of its advance points:
 * ratios[5], last_level, advance_exhausted and transfer_order.  transfer_order 0 is the reference's order, exactly as described above.  transfer_order 1 is
 * the paper's: a learner that leaves level k keeps its level-k block as learnt, and on entering level k + 1 gets Q[k+1] = Q[k] * ratios[k+1] in both tables;
 * there is no wrap and ratios[0] is unused; everything else at an advance point is as above.  advance_every, the env-side config, gamma and dtype stay the
 * ensemble's.  The RNG key stays (learner, seed) and advance points depend on the period index only, so learner l of a recipe ensemble equals, bit for bit
 * in every output, learner l of an ensemble of the same size and seed in which EVERY learner has l's recipe; two runs of a and b periods equal one of a + b.
 * While no recipes are installed every call behaves as described above.
 * dql_ensemble_set_recipes installs n_recipes empty recipes and the assignment (replacing whatever was installed); n_recipes = 0 uninstalls.  Each recipe is
 * then filled with dql_ensemble_set_recipe and, per level, dql_ensemble_set_recipe_level_schedules.  While recipes are installed the rule of
 * dql_ensemble_set_curriculum and the schedules of dql_ensemble_set_schedules / _set_level_schedules are kept but not read; dql_ensemble_n_unfinished,
 * dql_ensemble_get_levels and dql_ensemble_run go by each learner's own recipe.
 * Refused with DQL_EINVAL, a message, nothing changed and nothing launched: dql_ensemble_set_recipes while curriculum mode is off, with n_recipes outside
 * 0..64, with an index outside 0..n_recipes - 1, or with a null array and n_recipes > 0; dql_ensemble_set_recipe / _set_recipe_level_schedules for a recipe
 * that is not installed, with what dql_ensemble_set_curriculum and dql_ensemble_set_schedules / _set_level_schedules refuse (last_level is held against the
 * recipe's own learners; alpha_min is a learning rate), or with a transfer_order other than 0 or 1; dql_ensemble_run unless every recipe that has a member
 * has its rule and its schedules for every level from each member's level up to its last_level; dql_ensemble_set_curriculum with advance_every = 0; and
 * dql_ensemble_set_level above the smallest last_level of the recipes that have a member. */
#define DQL_ENSEMBLE_MAX_RECIPES 64
int dql_ensemble_set_recipes(dql_ensemble* ens, int32_t n_recipes, const int32_t* recipe_of); /* recipe_of int32[n_learners] */
/* alpha double[n_alpha], ratios double[5] (transfer_order 0: ratios[k] when level k is finished; 1: ratios[k + 1] when level k + 1 is entered) */
int dql_ensemble_set_recipe(dql_ensemble* ens, int32_t recipe, uint32_t quirks, const double* alpha, int32_t n_alpha, double alpha_min, const double* ratios,
                            int32_t last_level, int32_t advance_exhausted, int32_t transfer_order);
int dql_ensemble_set_recipe_level_schedules(dql_ensemble* ens, int32_t recipe, int32_t level, const double* eps, int32_t n_eps, int32_t window,
                                            int32_t min_successes, int32_t max_episodes);
/* recipe_of int32[n_learners]: every learner's recipe, or -1 everywhere while none are installed */
int dql_ensemble_get_recipes(dql_ensemble* ens, int32_t* recipe_of);

/* ---- learners with teams of envs ----
 * dql_ensemble_create_teams makes an ensemble whose learner l owns, besides its three tables, the envs g = l E .. l E + E - 1 (E = envs_per_learner, one of
 * 1, 2, 4, 8, 16, 32, 64) of a context made with dql_create(cfg, device, n_learners * E, seed, 0): the Philox key of env g is (g, seed).  All envs share
 * the period index.  In a period every env of a live learner that is not resetting acts on ONE exploration threshold (the eps table at the episodes the
 * learner had finished at the level when the period began) and, where it does not explore, greedily on the learner's tables as they stood after all of the
 * previous period's updates.  Then the learner applies DoubleQLearningAgent.update to the E transitions one after the other in env order — learning rate at
 * the pre-increment count as it stands at that moment, the row of s' read from the tables as they stand at that moment, so after the updates of the envs
 * before it in the same period — and books finished episodes in the same order (totals, by_code, episode log, the promotion ring).  Once the level is
 * decided in a period (promotion or max_episodes), episodes that later envs finish in the SAME period count in the totals and the log only, so
 * level_episodes and promoted never exceed max_episodes.  The learner freezes at the end of that period: all E updates applied, all E envs left as they
 * are after it.  No fold, no delay: a literal sequence of update calls.  With E = 1 every output equals dql_ensemble_create's, bit for bit.
 * Every dql_ensemble_* call works on such an ensemble; dql_ensemble_get_state returns n_learners * E envs in env order ([64][n_learners * E] and
 * [7][n_learners * E]), dql_ensemble_set_level sends all of them through reset; tables, counters, log and score stay per learner.  With E > 1 the ensemble
 * flies the barrier mode or team curriculum mode (dql_ensemble_set_team_curriculum, below); it has no per-learner curriculum and no recipes:
 * dql_ensemble_set_curriculum and dql_ensemble_set_recipes return DQL_EINVAL with nothing changed and nothing launched.
 * Refused like dql_ensemble_create, and for an envs_per_learner outside the seven values or n_learners * envs_per_learner > DQL_ENSEMBLE_MAX_LEARNERS. */
int dql_ensemble_create_teams(const dql_config* cfg, int device, int64_t n_learners, int32_t envs_per_learner, uint64_t seed, int32_t log_capacity,
                              dql_ensemble** out);
int dql_ensemble_envs_per_learner(dql_ensemble* ens, int32_t* envs_per_learner); /* 1 for dql_ensemble_create's */

/* ---- n-step Double-Q targets for the plain sequential ensemble ----
 * dql_ensemble_set_nstep(ens, n): n = 0, the state at creation, lets dql_ensemble_run fly the one-step kernel exactly as before; 1 <= n <= DQL_NSTEP_MAX
 * makes it fly the n-step kernel (n = 1 included, which equals n = 0 bit for bit).  The period schedule, the action rule (STREAM_ACTION word, per-learner
 * eps threshold, greedy choice on the learner's current tables), reset periods, counters, the episode log, the promotion ring and the freeze rules do not
 * change; only the update does.
 * Each learner keeps a PENDING WINDOW of at most n entries (cell, reward, coin), one per decision of the current episode, oldest first: cell = idx_x before
 * the period * 3 + action, reward = the env's reward field as a double, coin = bit 31 of the third word of that decision's action draw.  After a decision
 * that ended in state s': (1) its entry is appended; (2) both tables' row of s' is read once, before this period's first write; (3) mask = "the position
 * bin of the newest entry's state differs from that of s'" under DQL_Q_BOOTSTRAP_ON_POS_CHANGE, !done otherwise; (4) if the period ended the episode every
 * entry is updated, oldest first, and the window emptied; else if the window holds n entries the oldest is updated and removed; else nothing is updated.
 * The update of the entry at position k of a window of m entries (0 = oldest): sel_b = Double Q-learning and the ENTRY's coin (never under
 * DQL_Q_UPDATE_TABLE_A_ONLY); best = the valuing table's element of the row of s' at the arg-max of the selecting table's row, tables assigned as in the
 * one-step update; g = best * mask, then for i = m - 1 down to k: g = r_i + (gamma * g), IEEE double, two roundings per step, never contracted; alpha at
 * the cell's pre-increment count, which is then incremented; q_new = q + alpha * (g - q) on the selected table.  A cell outside [0, 2835) is counted in
 * dql_ensemble_index_faults and dropped.  A write to the row of the state the env is in now also reaches the next period's greedy choice, whichever entry
 * made it.
 * A learner freezes only at an episode's end, after the flush: a frozen learner's window is empty.  A window that is open at a launch's end persists, so
 * runs of a and b periods equal one run of a + b.  dql_ensemble_set_level discards every window (every env re-enters through reset); dql_ensemble_rearm,
 * _transfer and _set_tables leave them alone.
 * Refused with a message, nothing launched and nothing changed: DQL_EINVAL for n outside 0..DQL_NSTEP_MAX, for n >= 1 on a team ensemble
 * (dql_ensemble_create_teams), and for n >= 1 in per-learner curriculum mode or with recipes installed (and dql_ensemble_set_curriculum with
 * advance_every > 0 and dql_ensemble_set_recipes with n_recipes > 0 while n >= 1); DQL_ESTATE for any change of n while some learner's window holds
 * entries (allowed after creation, after dql_ensemble_set_level, or when every learner is frozen); a null pointer.
 * dql_ensemble_get_nstep returns the setting and, where asked for, the windows' lengths (int32 [n_learners]). */
#define DQL_NSTEP_MAX 16
int dql_ensemble_set_nstep(dql_ensemble* ens, int32_t n);
int dql_ensemble_get_nstep(dql_ensemble* ens, int32_t* n, int32_t* pending_len_or_null);

/* ---- n-step targets per recipe ----
 * With recipes installed (curriculum mode), n is a property of a recipe: dql_ensemble_set_recipe_nstep(ens, recipe, n) with 0 <= n <= DQL_NSTEP_MAX.  The
 * learners of a recipe with n = 0, the state after dql_ensemble_set_recipes, fly the one-step update exactly as before; those of a recipe with n >= 1 walk
 * the levels under their recipe's rule and update with the n-step return described above (append, one early read of the row of s', mask, flush at an
 * episode's end, oldest-entry update from a full window, the entry's own coin), with the recipe's quirks, learning rates and per-level schedules.  Launches
 * are cut at the multiples of advance_every as before; a window that is open at a cut persists, so runs of a and b periods equal one run of a + b.  A
 * learner freezes only after its flush, so a learner that advances has an empty window.  Learner l of a mixed ensemble equals, bit for bit in every output,
 * learner l of an ensemble of the same size and seed in which every learner has l's recipe, n included.  dql_ensemble_set_level empties every window;
 * dql_ensemble_transfer, _set_tables and _rearm leave them alone.  The ensemble-wide dql_ensemble_set_nstep stays the plain mode's switch with its refusals
 * unchanged, and dql_ensemble_get_nstep keeps returning it (0 in a recipe ensemble) and the windows' lengths.
 * Refused with a message and nothing changed: DQL_EINVAL while no recipes are installed, for a recipe outside 0..n_recipes - 1 and for n outside
 * 0..DQL_NSTEP_MAX; DQL_ESTATE for a change of n while a member of that recipe has a pending window with entries (the value the recipe already has is
 * accepted).  dql_ensemble_set_recipes, install or uninstall, returns DQL_ESTATE with nothing changed while any window holds entries. */
int dql_ensemble_set_recipe_nstep(dql_ensemble* ens, int32_t recipe, int32_t n);
int dql_ensemble_get_recipe_nstep(dql_ensemble* ens, int32_t recipe, int32_t* n);

/* ---- n-step targets for team ensembles: one pending window per env ----
 * A team ensemble (dql_ensemble_create_teams, any E, E = 1 included) has an ensemble-wide team_nstep.  At 0, the state at creation, dql_ensemble_run flies
 * the one-step team kernel exactly as before.  At 1 <= n <= DQL_NSTEP_MAX every ENV g keeps a pending window of its own: at most n entries (cell, reward as
 * a double, coin), one per decision of env g's running episode, oldest first.  A period of a live learner is the team period described above — one
 * threshold per team, the greedy row read from the tables as they stand after all of the previous period's updates, the flight, the bookkeeping, the
 * decision rule, the freeze at the period's end — with the update replaced.  For e = 0 .. E - 1 in env order, for an env that made a decision: (1) the
 * decision's entry is appended to env g's window; (2) both tables' row of s' is read ONCE, AT THIS ENV'S TURN: after every write that envs < e made in this
 * period and before this env's own; (3) mask as in the team period; (4) if the period ended the env's episode every entry is updated, oldest first, and the
 * window emptied; else if the window holds n entries the oldest is updated and removed; else nothing is updated.  One update is dql_ensemble_set_nstep's,
 * operation for operation: the ENTRY's own coin, best on the row of step 2, g = best * mask, g = r_i + (gamma * g) for i = m - 1 down to k, alpha at the
 * cell's count as it stands at that moment (pre-increment), q_new = q + alpha * (g - q) on the value that stands at that moment: team-mates may have
 * written the entry's cell since it was appended.  A cell outside [0, 2835), or an s' outside the tables, is counted in dql_ensemble_index_faults; nothing
 * is updated for it and the window keeps its shape (at most n - 1 entries after the record, none after a done).
 * With E = 1 every output equals a plain ensemble's under dql_ensemble_set_nstep(n); with n = 1 every output equals team_nstep = 0, bit for bit.
 * A team freezes at the end of the deciding period, when its envs are mostly in the middle of an episode: A FROZEN TEAM'S WINDOWS ARE GENERALLY NOT EMPTY,
 * unlike a plain n-step learner's.  The windows persist in device memory per env across launches and across a freeze: runs of a and b periods equal one
 * run of a + b; dql_ensemble_rearm, _transfer and _set_tables leave them alone, and after a rearm the envs fly on with the windows they had;
 * dql_ensemble_set_level empties all of them.  The first call with n >= 1 allocates them (160 B per env); creation is untouched.  They are not the plain
 * mode's: dql_ensemble_get_nstep keeps answering 0 and zeros [n_learners] on a team ensemble, and dql_ensemble_set_nstep, _set_curriculum and
 * _set_recipes keep their refusals.
 * dql_ensemble_set_team_nstep: DQL_EINVAL with nothing changed for n outside 0..DQL_NSTEP_MAX, for an ensemble not made by dql_ensemble_create_teams and
 * for a null pointer; DQL_ESTATE for a change of n while any env's window holds entries — allowed after creation and after dql_ensemble_set_level; that
 * every team is frozen is NOT enough.  The value it already has is accepted.  (At n = 0 and n = 1 every window is empty after every period, so a change
 * from those values is accepted at any time, in the middle of episodes included: the first windows then begin with the next decision.)
 * A team ensemble of one env per learner may enter per-learner curriculum mode and take recipes; those modes fly the one-step learners, so they and
 * team_nstep >= 1 refuse each other with DQL_EINVAL and nothing changed: dql_ensemble_set_curriculum with advance_every > 0 and dql_ensemble_set_recipes with
 * n_recipes > 0 while team_nstep >= 1, and dql_ensemble_set_team_nstep with n >= 1 while curriculum mode is on or recipes are installed.
 * dql_ensemble_get_team_nstep returns n and, where asked for, the windows' lengths, int32 [n_learners * E] in env order. */
int dql_ensemble_set_team_nstep(dql_ensemble* ens, int32_t n);
int dql_ensemble_get_team_nstep(dql_ensemble* ens, int32_t* n, int32_t* pending_len_or_null);

/* ---- team curriculum mode: every team walks the levels by itself, n-step targets included ----
 * A team ensemble (dql_ensemble_create_teams, any E, E = 1 included) with advance_every >= 1: every team stands on a level of its own, starting at the
 * config's, and dql_ensemble_run is per-learner curriculum mode's for teams.  Its launches are cut at the period indices that are multiples of
 * advance_every.  At such an index j, before period j is flown, a frozen team below last_level that promoted — or ran out of episodes, with
 * advance_exhausted = 1 — takes the step a learner takes there: its history entry (promoted_at, episodes_at of the level it leaves) is recorded; the
 * transfer is applied to ITS OWN two tables, with transfer_order 0 the reference's Q[k] = Q[k-1] * ratios[k] for the finished level k (k = 0 wraps to level
 * 4), with transfer_order 1 the paper's Q[k+1] = Q[k] * ratios[k+1] (the level-k block kept, no wrap, ratios[0] unused); it moves to level k + 1, entered
 * at period j; ALL E of its envs re-enter through reset; where the ensemble has team n-step windows, every one of those envs' windows is emptied (a frozen
 * team's windows are generally not empty, and their entries belong to the episodes the reset abandons: what dql_ensemble_set_level does for everyone); its
 * per-level episode count, promotion ring, promotion record and frozen flag are cleared.  Each launch flies the live teams regrouped by level, 64 / E teams
 * to a wave and one level to a wave, so a frozen team costs nothing after the launch it froze in.  A team's period is the team period of the barrier mode,
 * with the one-step update (team_nstep = 0) or the per-env windows (1 <= team_nstep <= DQL_NSTEP_MAX), at the team's level: that level's MDP constants and
 * the schedules dql_ensemble_set_level_schedules installed for it; the learning rates stay dql_ensemble_set_schedules'.  A team's results do not depend on
 * the other teams of the ensemble, nor on how a run is split into calls.  With E = 1 and transfer_order 0 every output equals the same ensemble's under
 * dql_ensemble_set_curriculum.  dql_ensemble_n_unfinished, dql_ensemble_get_levels and dql_diag_ensemble_launches answer as they do in that mode.
 * Teams have no recipes: dql_ensemble_set_recipes stays refused for E > 1.
 * DQL_EINVAL, nothing changed, nothing launched, each with its own sentence: an ensemble not made by dql_ensemble_create_teams; advance_every outside
 * 0..4096; per-learner curriculum mode on or recipes installed (E = 1 only); with advance_every = 0 (the mode off, the barrier launch again) while teams
 * stand on different levels; null or non-finite ratios; advance_exhausted or transfer_order outside {0, 1}; last_level below a team's level or above 4.
 * While the mode is on, dql_ensemble_set_curriculum and dql_ensemble_set_recipes are refused on that ensemble, dql_ensemble_set_level holds k <= last_level,
 * and dql_ensemble_run refuses while a level on a team's way up to last_level has no schedules.  dql_ensemble_set_team_nstep is accepted before and after
 * the mode is switched on, under its own rule (no env's window holds entries). */
int dql_ensemble_set_team_curriculum(dql_ensemble* ens, int32_t last_level, int32_t advance_every, const double* ratios, int32_t advance_exhausted, int32_t transfer_order);

#ifdef __cplusplus
}
#endif
#endif /* DQL_H */
