// dql_agent.inc: the drop-in DoubleQLearningAgent (include/dql.h dql_agent_*): predict / ordered update kernels, the resident agent (struct dql_agent) and its
// host-mirrored single transitions.  A fragment of dql_hip.hip's translation unit, not a header.  Needs from it: fail / HIP_TRY, DevBuf / OP_PROLOGUE / UP,
// wait_stream / wait_posted, k_transfer; and dql_device.hpp (agent_predict, argmax3).
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

extern "C" {
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
  DOWN(qa, a, B); DOWN(qb, b, B);
  return DQL_OK;
}

int dql_agent_predict(int device, const double* qa, const double* qb, const int32_t* idx, int64_t n, uint8_t* action_out) {
  if (n < 0 || !qa || !qb || (n > 0 && (!idx || !action_out))) return fail(DQL_EINVAL, "null array");
  if (n == 0) return DQL_OK;
  for (int64_t i = 0; i < n; ++i) if (idx[i] < 0 || idx[i] >= DQL_N_STATES) return fail(DQL_EINVAL, "state index out of range");
  OP_PROLOGUE(device)
  DevBuf a, b, ix, o;
  UP(a, qa, DQL_N_CELLS * sizeof(double)); UP(b, qb, DQL_N_CELLS * sizeof(double)); UP(ix, idx, (size_t)n * sizeof(int));
  OUT(o, (size_t)n);
  hipLaunchKernelGGL(k_predict, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double*)a.p, (const double*)b.p, (const int*)ix.p, (long long)n, (uint8_t*)o.p);
  HIP_TRY(hipGetLastError());
  DOWN(action_out, o, (size_t)n);
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
  DOWN(qa, a, B); DOWN(qb, b, B); DOWN(count, c, B);
  return DQL_OK;
}

}  // extern "C"
