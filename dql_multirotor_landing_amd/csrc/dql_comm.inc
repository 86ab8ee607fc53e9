// dql_comm.inc: the multi-GPU exchanges of a context's window accumulators: RCCL loaded on first use (include/dql.h dql_comm_*, dql_attach_comm,
// dql_allreduce_window) and the one-shot peer-to-peer exchange over HIP IPC (dql_p2p_*) with its kernels.  A fragment of dql_hip.hip's translation unit, not a
// header.  Needs from it: fail / HIP_TRY, dql_ctx (its DevOwned owns the exchange buffers), CHECK_CTX / POP_NEVER, flush_pending, p2p_failed_seq, DQL_ACC_LEN.
// ---- one-shot peer-to-peer exchange of the window accumulators (SURVEY.md 8e, second step) ----
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

// ---------------------------------------------------------------------------------------------
// RCCL communicator (SURVEY.md section 8e).  librccl.so is half a gigabyte: it is loaded with dlopen the first time a
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
  x->dev.adopt(x->p2p_buf);
  if (x->dev.alloc((void**)&x->p2p_status, 2 * sizeof(unsigned long long)) != hipSuccess) return fail(DQL_ENOMEM, "hipMalloc failed");
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
