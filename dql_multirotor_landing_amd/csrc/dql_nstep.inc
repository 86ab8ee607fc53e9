// dql_nstep.inc: sequential learners with n-step Double-Q targets (include/dql.h dql_ensemble_set_nstep / _get_nstep, DESIGN.md section 22): the lane kernel
// and the two C calls.  A fragment of dql_hip.hip's translation unit, not a header, included after dql_ensemble.inc, whose struct dql_ensemble, LearnArgs,
// make_learn_args and shared host helpers it works with (ens_fly launches the kernel through launch_learn_nstep below); dql_nstep.hpp holds the per-lane body.
// k_learn's shape: one learner per lane, workgroups of one wave, the env in registers for all periods of the launch, the tables the lane's own slices.  The
// pending windows live in LDS for the launch, [slot][lane]: 16 x 64 x (2 + 8) B = 10 KB per wave whatever n is; a lane reads and writes its own column only,
// so no barrier is needed.  learner_periods_nstep loads them from the ensemble's arrays at its start and stores them back beside store_env.
struct LdsWindow {
  uint16_t* k; double* v;  // the lane's column: element [slot] at slot * 64
  DQL_DEV uint16_t& key(int slot) const { return k[slot * 64]; }
  DQL_DEV double& val(int slot) const { return v[slot * 64]; }
};
using NstepDev = NstepMem<uint16_t*, double*, int*>;
template <typename T> struct NstepArgs {
  LearnArgs<T> a;
  NstepDev nm;
  int nstep;
};
template <typename T, int TICK, int XMODE> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_learn_nstep(NstepArgs<T> g) {
  const LearnArgs<T>& a = g.a;
  const int tid = threadIdx.x;
  const long long l = (long long)blockIdx.x * 64 + tid;
  SimK<T> cl = a.c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  __shared__ TickLds<T> sTickK;  // as in k_learn
  __shared__ uint16_t sKey[NSTEP_MAX * 64];
  __shared__ double sVal[NSTEP_MAX * 64];
  if constexpr (sizeof(T) == 8) {
    if (tid == 0) sTickK.k = cfgk;
    __syncthreads();
  }
  const TickConsts<TICK, T> tc([&]() -> const SimK<T>& { if constexpr (sizeof(T) == 8) return sTickK.k; else return cfgk; }());
  uint32_t kv_[20];
  const uint32_t* kv = lane_round_keys<T>(a.seed, kv_);
  learner_periods_nstep<TICK, XMODE>(cl, cfgk, tc, a.mdp, a.mdp_run, a.sched, a.mem, a.sr, a.si, a.seed, l, l < a.mem.n, a.j0, a.n_periods, a.mgr0, a.tick_sched, kv,
                                     g.nstep, LdsWindow{sKey + tid, sVal + tid}, g.nm);
}

template <typename T> static void launch_learn_nstep(dql_ensemble* x, int k, int n_waves) {
  NstepArgs<T> g;
  g.a = make_learn_args<T>(x, x->mdpk, k);
  g.nm = NstepDev{x->ns_key, x->ns_val, x->ns_len};
  g.nstep = x->nstep;
  hipLaunchKernelGGL((k_learn_nstep<T, TICK_PLAIN, X_ONLY>), dim3((unsigned)n_waves), dim3(64), 0, 0, g);
}

// the persistent windows, zeroed, on the first call (dql_ensemble_set_nstep and dql_ensemble_set_recipe_nstep with n >= 1); later calls change nothing
static int ens_alloc_windows(dql_ensemble* x) {
  if (x->ns_len) return DQL_OK;
  const size_t L = (size_t)x->n;
  uint16_t* key = nullptr; double* val = nullptr; int* len = nullptr;
  const int rc = ens_alloc_zeroed(x->dev, {{(void**)&key, (size_t)DQL_NSTEP_MAX * L * sizeof(uint16_t)}, {(void**)&val, (size_t)DQL_NSTEP_MAX * L * sizeof(double)}, {(void**)&len, L * sizeof(int)}});
  if (rc) return fail(rc, rc == DQL_ENOMEM ? "hipMalloc failed" : "hipMemset failed");
  x->ns_key = key; x->ns_val = val; x->ns_len = len;
  return DQL_OK;
}

extern "C" {
int dql_ensemble_set_nstep(dql_ensemble* x, int32_t n) {
  CHECK_ENS(x);
  ENS_REFINED_REFUSED(x, "dql_ensemble_set_nstep", ENS_REFINED_MODES);
  if (n < 0 || n > DQL_NSTEP_MAX) return fail(DQL_EINVAL, "dql_ensemble_set_nstep: n must be in 0..16 (DQL_NSTEP_MAX; 0: the one-step kernel); nothing was changed");
  if (n >= 1 && (x->teams || x->envs_per_learner > 1))
    return fail(DQL_EINVAL, "dql_ensemble_set_nstep: a team ensemble (dql_ensemble_create_teams) has the one-step update only; nothing was changed");
  if (n >= 1 && (x->advance_every || x->rcp))
    return fail(DQL_EINVAL, "dql_ensemble_set_nstep: n-step targets are refused in per-learner curriculum mode and with recipes installed (switch them off first); nothing was changed");
  if (n == x->nstep) return DQL_OK;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipDeviceSynchronize());
  int rc = ens_windows_empty(x, [](size_t) { return true; }, "dql_ensemble_set_nstep: n cannot change while a learner's pending window holds entries (change it after creation, after dql_ensemble_set_level, or when every learner is frozen); nothing was changed");
  if (rc) return rc;
  if (n >= 1) { rc = ens_alloc_windows(x); if (rc) return rc; }
  x->nstep = n;
  return DQL_OK;
}
int dql_ensemble_get_nstep(dql_ensemble* x, int32_t* n, int32_t* pending_len_or_null) {
  CHECK_ENS(x);
  if (!n) return fail(DQL_EINVAL, "dql_ensemble_get_nstep: null pointer");
  *n = x->nstep;
  if (!pending_len_or_null) return DQL_OK;
  const size_t L = (size_t)x->n;
  if (!x->ns_len) { std::memset(pending_len_or_null, 0, L * sizeof(int32_t)); return DQL_OK; }  // no window was ever made
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipMemcpy(pending_len_or_null, x->ns_len, L * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DQL_OK;
}
}  // extern "C"
