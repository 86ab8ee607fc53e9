// emu_common.h — what every driver under tests/host_emu/ shares, included after host_shim.h and the device headers: the job and result files, the per-launch
// prologue every kernel begins with, the packed state arrays and the checked acting table.  What only the drivers of the sequential-learner family share
// (their jobs, state, windows and run loops) is emu_learners.h, which includes this file.  A driver keeps the part that restates one kernel.
// The Python side of the same plumbing is tests/host_emu_harness.py.  Exit status 2 is a bad job or a file that cannot be written, 3 an index violation.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace emu {

// ---- the job file (read) and the result file (written): raw arrays one after the other, in the order the test module packs / takes them
struct JobFile {
  FILE* f;
  explicit JobFile(const char* path) : f(std::fopen(path, "rb")) { if (!f) { std::perror(path); std::exit(2); } }
  JobFile(const JobFile&) = delete;
  ~JobFile() { std::fclose(f); }
  template <typename V> void read(V* p, size_t n) {
    if (n && std::fread(p, sizeof(V), n, f) != n) { std::fprintf(stderr, "short job file\n"); std::exit(2); }
  }
  template <typename V> void read(std::vector<V>& v) { read(v.data(), v.size()); }
  // the config, after the header whose first word states the size the writer believes it has
  void read_config(dql_config& cfg, int32_t stated_size) {
    if (stated_size != (int32_t)sizeof(dql_config)) { std::fprintf(stderr, "dql_config size %d != %d\n", stated_size, (int)sizeof(dql_config)); std::exit(2); }
    read(&cfg, 1);
  }
};
[[noreturn]] inline void bad_job() { std::fprintf(stderr, "bad job\n"); std::exit(2); }

struct ResultFile {
  FILE* f;
  bool ok = true;
  explicit ResultFile(const char* path) : f(std::fopen(path, "wb")) { if (!f) { std::perror(path); std::exit(2); } }
  ResultFile(const ResultFile&) = delete;
  template <typename V> void put(const V* p, size_t n) { ok = std::fwrite(p, sizeof(V), n, f) == n && ok; }
  template <typename V> void put(const std::vector<V>& v) { put(v.data(), v.size()); }
  int close() { return (std::fclose(f) == 0 && ok) ? 0 : 2; }  // main's return value
};

// ---- the launch prologue of k_step, k_rollout, k_score, k_learn and k_learn_levels: from the launch's SimK (the caller has set two_axis / working as the
// kernel sees them), the run-time constants in VGPRs, the tick constants in the layout's form, and the 20 Philox round keys in VGPRs where the kernel keeps
// them (float32; k_step only for TICK_LIT / TICK_PLAIN), a null pointer where it does not.  tc may refer to cfgk (TickK<TICK_PLAIN>): not copyable.
template <typename T, int TICK> struct Launch {
  const dql::SimK<T> cfgk;
  const dql::TickConsts<TICK, T> tc;
  uint32_t keys[20];
  const uint32_t* kv = nullptr;
  Launch(const dql::SimK<T>& cl, unsigned long long seed, bool round_keys = sizeof(T) == 4) : cfgk(dql::period_consts_in_vgprs(cl)), tc(cfgk) {
    if (!round_keys) return;
    for (int r = 0; r < 10; ++r) {
      keys[r] = dql::to_vgpr((uint32_t)seed + (uint32_t)r * 0x9E3779B9u);
      keys[10 + r] = dql::to_vgpr((uint32_t)(seed >> 32) + (uint32_t)r * 0xBB67AE85u);
    }
    kv = keys;
  }
  Launch(const Launch&) = delete;
  Launch& operator=(const Launch&) = delete;
};

// ---- the state arrays <-> the oracle's fields ([NF_REAL][n] doubles, [NF_INT][n] ints: dql_get_sim_state / dql_get_sim_ints).  The emulators' own statement of
// the packing, independent of the library's quads_to_fields / unpack_ints
template <typename T> void unpack_state(const dql::Quad<T>* sr, const int4* si, size_t n, std::vector<double>& reals, std::vector<int32_t>& ints) {
  reals.resize((size_t)dql::NF_REAL * n); ints.resize((size_t)dql::NF_INT * n);
  for (int f = 0; f < dql::NF_REAL; ++f)
    for (size_t i = 0; i < n; ++i) reals[(size_t)f * n + i] = (double)(&sr[(size_t)(f / 4) * n + i].a)[f % 4];
  for (size_t i = 0; i < n; ++i) {
    const int4 h = si[i];
    ints[0 * n + i] = h.x; ints[1 * n + i] = h.y; ints[2 * n + i] = h.z & 0xffff; ints[3 * n + i] = (h.z >> 16) & 0xffff;
    ints[4 * n + i] = h.w & 0xff; ints[5 * n + i] = (h.w >> 8) & 0xff; ints[6 * n + i] = (h.w >> 16) & 0xff;
  }
}
template <typename T> void pack_state(const std::vector<double>& reals, const std::vector<int32_t>& ints, size_t n, std::vector<dql::Quad<T>>& sr, std::vector<int4>& si) {
  sr.resize((size_t)dql::NQ_REAL * n); si.resize(n);
  for (int f = 0; f < dql::NF_REAL; ++f)
    for (size_t i = 0; i < n; ++i) (&sr[(size_t)(f / 4) * n + i].a)[f % 4] = (T)reals[(size_t)f * n + i];
  const int32_t* g = ints.data();
  for (size_t i = 0; i < n; ++i)
    si[i] = make_int4(g[0 * n + i], g[1 * n + i], (g[2 * n + i] & 0xffff) | (g[3 * n + i] << 16), (g[4 * n + i] & 0xff) | ((g[5 * n + i] & 0xff) << 8) | ((g[6 * n + i] & 0xff) << 16));
}

// ---- an acting table as the device code's TabPtr: every element read is bounds-checked; the driver's report names where it was and ends the run
[[noreturn]] inline void index_violation(long long k, const char* where, long long at) {
  std::fprintf(stderr, "INDEX VIOLATION: acting-table element %lld outside [0, N_CELLS) at %s %lld\n", k, where, at);
  std::exit(3);
}
struct TabRef {
  const double* p;
  void (*violation)(long long k);
  double operator[](long long k) const {
    if (k < 0 || k >= DQL_N_CELLS) { violation(k); std::exit(3); }
    return p[k];
  }
};

}  // namespace emu
