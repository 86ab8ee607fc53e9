// dql_view.inc: device-resident step outputs (dql_view_dev) and the device-mask reset (dql_reset_dev), DESIGN.md section 31.  A fragment of dql_hip.hip's
// translation unit, not a header.  Needs from it: fail / HIP_TRY / CHECK_CTX, POP_NEVER, struct dql_ctx, StatsDev, k_mark_reset; and dql_view.hpp.
//   k_env_view<T, R>   context element T, output element R: four instances.  One env per lane, workgroups of 256, the tail workgroup bounded by i < n (in the body).  Per env
//                      it reads the int4 word and quads 14, 10, 7, 15 as the outputs asked for need them (float32, everything: 80 B) and writes the row of 8 as
//                      16-byte vectors — a wave covers 2 KiB (float32) or 4 KiB (float64) of `obs` contiguously — and the per-env scalars at consecutive addresses
//                      (about 55 B with every output in float32).  No atomics, no LDS, no barrier; lane 0 of block 0 copies StatsDev::bad_actions with an ordinary
//                      store.  The body is env_view (dql_view.hpp), the text the host emulation runs.
// Both calls enqueue on the context's stream and return without waiting; dql_step_outputs, dql_reset and dql_step_dev keep their own code.
template <typename T, typename R> struct ViewArgs {
  const Quad<T>* sr; const int4* si;
  const unsigned long long* bad_src;
  long long n;
  ViewOut<R> o;
};
constexpr int VIEW_BLOCK = 256;
template <typename T, typename R> __global__ __launch_bounds__(VIEW_BLOCK) void k_env_view(ViewArgs<T, R> a) {
  const long long i = (long long)blockIdx.x * VIEW_BLOCK + threadIdx.x;
  env_view<T, R>(a.sr, a.si, a.bad_src, a.n, i, a.o);  // bounded by i < n in the body
}

template <typename T, typename R> static void launch_view(dql_ctx* x, const dql_view* v) {
  ViewArgs<T, R> a;
  a.sr = (const Quad<T>*)x->sr; a.si = x->si;
  a.bad_src = (const unsigned long long*)((const char*)x->stats + offsetof(StatsDev, bad_actions));
  a.n = x->n;
  a.o = ViewOut<R>{(ViewVec<R>*)v->obs, (R*)v->reward, (R*)v->cumulative_reward, v->idx_x, v->idx_y, v->step_count, v->done, v->was_reset, v->code,
                   (unsigned long long*)v->bad_actions};
  hipLaunchKernelGGL((k_env_view<T, R>), dim3((unsigned)((x->n + VIEW_BLOCK - 1) / VIEW_BLOCK)), dim3(VIEW_BLOCK), 0, x->stream, a);
}

extern "C" {
int dql_view_dev(dql_ctx* x, const dql_view* v) {
  CHECK_CTX(x);
  if (!v) return fail(DQL_EINVAL, "dql_view_dev: the view must not be null; nothing was launched");
  if (v->real_dtype != DQL_F32 && v->real_dtype != DQL_F64)
    return fail(DQL_EINVAL, "dql_view_dev: real_dtype must be DQL_F32 (0) or DQL_F64 (1), the element type of obs, reward and cumulative_reward; nothing was launched");
  if (v->reserved != 0) return fail(DQL_EINVAL, "dql_view_dev: the reserved word must be 0; nothing was launched");
  if ((uintptr_t)v->obs % 16u) return fail(DQL_EINVAL, "dql_view_dev: obs must be 16-byte aligned (its rows are written as 16-byte vectors); nothing was launched");
  POP_NEVER(x, "dql_view_dev");
  if (!v->obs && !v->reward && !v->cumulative_reward && !v->idx_x && !v->idx_y && !v->step_count && !v->done && !v->was_reset && !v->code && !v->bad_actions) return DQL_OK;
  HIP_TRY(hipSetDevice(x->device));
  if (x->dtype == DQL_F32) { if (v->real_dtype == DQL_F32) launch_view<float, float>(x, v); else launch_view<float, double>(x, v); }
  else { if (v->real_dtype == DQL_F32) launch_view<double, float>(x, v); else launch_view<double, double>(x, v); }
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}
// dql_reset with the mask where it already lives: k_mark_reset reads the caller's buffer, no staging copy and no wait
int dql_reset_dev(dql_ctx* x, const uint8_t* dev_mask) {
  CHECK_CTX(x);
  if (!dev_mask) return fail(DQL_EINVAL, "dql_reset_dev: dev_mask must not be null: dql_reset(ctx, NULL) marks every env; nothing was launched");
  HIP_TRY(hipSetDevice(x->device));
  hipLaunchKernelGGL(k_mark_reset, dim3((unsigned)((x->n + 255) / 256)), dim3(256), 0, x->stream, x->si, dev_mask, (long long)x->n);
  HIP_TRY(hipGetLastError());
  return DQL_OK;
}
}  // extern "C"
