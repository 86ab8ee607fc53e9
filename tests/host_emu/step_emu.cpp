// step_emu.cpp — one launch of the step kernel k_step, emulated on the CPU from the real device source (dql_device.hpp).
//
// For every env the driver does what one lane of k_step (dql_hip.hip) does in one launch: the packed ints and the clamped acting-table
// row first, load_env, P x agent_period<TICK, XMODE> with the launch's schedule, eps threshold, seed, env id and step index, the
// un-staged accumulation into the int64 [4][N_CELLS] accumulators (the one-wave-per-workgroup path), store_env.  The acting tables stay
// constant over the launch, as they do on the device.  A lane runs alone: __ballot(p) is p (host_shim.h).
//
// Index checks: every table read the device code makes goes through TabRef, which stops on an element outside [0, N_CELLS); every
// accumulator target is checked to lie in [0, 2 N_CELLS) AND to be the cell of the row the env left with the action it took, in the
// table its coin picked.  A violation stops the run with exit status 3 and names the env, the period and the state.
//
//   step_emu JOB OUT     run the launch described by JOB (see read_job; tests/test_step_host_emulation.py writes it), write OUT
//   step_emu --admits JOB      print refm and lit_ok of JOB's config: may TICK_PACKED_LITM / TICK_LIT serve it (create_impl)
//   step_emu --asan-selftest   read one element past a heap array (the sanitized build must report it)
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"

using namespace dql;

namespace {

constexpr int N_STATES = DQL_N_CELLS / DQL_N_ACTIONS;
template <typename T> SimK<T> x_only_(SimK<T> c) { c.two_axis = 0; return c; }  // k_step's x_only (dql_hip.hip)

struct Where { long long env = -1; int period = -1; int idx_x = 0, idx_y = 0, flags = 0, step_count = 0; };
Where g_where;

[[noreturn]] void violation(const char* what, long long a, long long b = 0) {
  std::fprintf(stderr, "INDEX VIOLATION: %s (%lld, %lld) at env %lld, period %d of the launch; state before the period: idx_x %d idx_y %d flags %d step_count %d\n",
               what, a, b, g_where.env, g_where.period, g_where.idx_x, g_where.idx_y, g_where.flags, g_where.step_count);
  std::exit(3);
}

// an acting table as agent_period's TabPtr: every element read is bounds-checked
struct TabRef {
  const double* p;
  double operator[](long long k) const {
    if (k < 0 || k >= DQL_N_CELLS) violation("acting-table element outside [0, N_CELLS)", k);
    return p[k];
  }
};

struct Job {
  int dtype, tick, xmode, mode, n_periods;
  long long n, env_id_offset, step_index;
  double eps;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> reals;  // [NF_REAL][n], dql_get_sim_state's layout
  std::vector<int32_t> ints;  // [NF_INT][n], dql_get_sim_ints'
  std::vector<double> qa, qb; // acting tables [N_CELLS]
  std::vector<uint8_t> actions;
};

template <typename V> void read_into(FILE* f, V* p, size_t n) {
  if (n && std::fread(p, sizeof(V), n, f) != n) { std::fprintf(stderr, "short job file\n"); std::exit(2); }
}

Job read_job(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  Job j;
  int32_t hdr[8];   // cfg size, dtype, tick, xmode, mode, n_periods, have_actions, 0
  int64_t ll[4];    // n, env_id_offset, step_index, seed
  read_into(f, hdr, 8); read_into(f, ll, 4); read_into(f, &j.eps, 1);
  if (hdr[0] != (int32_t)sizeof(dql_config)) { std::fprintf(stderr, "dql_config size %d != %d\n", hdr[0], (int)sizeof(dql_config)); std::exit(2); }
  read_into(f, &j.cfg, 1);
  j.dtype = hdr[1]; j.tick = hdr[2]; j.xmode = hdr[3]; j.mode = hdr[4]; j.n_periods = hdr[5];
  j.n = ll[0]; j.env_id_offset = ll[1]; j.step_index = ll[2]; j.seed = (unsigned long long)ll[3];
  if (j.n < 1 || j.n_periods < 1 || j.n_periods > DQL_MAX_PERIODS) { std::fprintf(stderr, "bad job\n"); std::exit(2); }
  j.reals.resize((size_t)NF_REAL * j.n); j.ints.resize((size_t)NF_INT * j.n); j.qa.resize(DQL_N_CELLS); j.qb.resize(DQL_N_CELLS);
  read_into(f, j.reals.data(), j.reals.size()); read_into(f, j.ints.data(), j.ints.size());
  read_into(f, j.qa.data(), j.qa.size()); read_into(f, j.qb.data(), j.qb.size());
  if (hdr[6]) { j.actions.resize((size_t)j.n); read_into(f, j.actions.data(), j.actions.size()); }
  std::fclose(f);
  return j;
}

// what the launch leaves behind, in the oracle's formats
struct Result {
  std::vector<double> reals; std::vector<int32_t> ints;
  std::vector<unsigned long long> acc;  // [4][N_CELLS]: table a's {target sums, visits}, then table b's (k_step's global layout)
  unsigned long long stats[12] = {};    // decisions, episodes, by_code[9], reward_fx (Oracle.stats)
  unsigned long long bad_actions = 0;
};

template <typename T, int TICK, int XMODE> void launch(const Job& j, Result& out) {
  const dql_config& cfg = j.cfg;
  const long long n = j.n;
  // create_impl: the Kalman fixed point once per context; make_step_args: the launch's constants
  KalFix kal_fix;
  { const SimK<T> k = make_simk<T>(cfg); kal_fix = KalFix{(double)k.kal_pss, (double)k.kal_kss, true}; }
  const SimK<T> c = make_simk<T>(cfg, &kal_fix);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  long long mgr0[DQL_MAX_PERIODS]; int sched[DQL_MAX_PERIODS];
  fill_schedule(cfg, j.step_index, mgr0, sched);
  const unsigned eps_thr = eps_threshold(j.eps);
  // HBM images of the state (dql_set_sim_state / dql_set_sim_ints)
  std::vector<Quad<T>> sr((size_t)NQ_REAL * n);
  std::vector<int4> si((size_t)n);
  for (int f = 0; f < NF_REAL; ++f) {
    const int q = f / 4, k = f % 4;
    for (long long i = 0; i < n; ++i) (&sr[(size_t)q * n + i].a)[k] = (T)j.reals[(size_t)f * n + i];
  }
  for (long long i = 0; i < n; ++i) {
    const int32_t* g = j.ints.data();
    si[i] = make_int4(g[0 * n + i], g[1 * n + i], (g[2 * n + i] & 0xffff) | (g[3 * n + i] << 16), (g[4 * n + i] & 0xff) | ((g[5 * n + i] & 0xff) << 8) | ((g[6 * n + i] & 0xff) << 16));
  }
  const TabRef qa{j.qa.data()}, qb{j.qb.data()};
  out.acc.assign(4 * (size_t)DQL_N_CELLS, 0ull);
  // k_step, per launch: the x-axis kernels see two_axis as the constant 0; the run-time constants move to VGPRs; the tick constants in the layout's form
  SimK<T> cfgk = c;
  if constexpr (XMODE == X_ONLY) cfgk.two_axis = 0;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);  // (BLOCK < 512: the instances this driver stands for)
  const TickConsts<TICK, T> tc(cfgk);
  uint32_t kv_[20];
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4 && (TICK == TICK_LIT || TICK == TICK_PLAIN)) {
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)j.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(j.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  for (long long i = 0; i < n; ++i) {
    g_where = Where{i, -1, 0, 0, 0, 0};
    const int4 iv = si[i];
    QRow qx = load_qrow(qa, qb, (unsigned)iv.x < (unsigned)(DQL_N_CELLS / DQL_N_ACTIONS) ? iv.x : 0);
    Env<T> e;
    load_env(e, sr.data(), iv, n, i, XMODE == X_ONLY ? x_only_(c) : c);
    for (int p = 0; p < j.n_periods; ++p) {
      g_where = Where{i, p, e.idx_x, e.idx_y, e.flags, e.step_count};
      const int ext = (j.mode == MODE_EXTERNAL) ? (int)j.actions[i] : 2;
      if (j.mode == MODE_EXTERNAL) {
        const int ax = ext & 3, ay = (ext >> 2) & 3;
        if (ax > 2 || ay > 2 || (ext >> 4) || (!c.two_axis && ay != 0 && ay != 2)) out.bad_actions += 1;
      }
      const int prev_idx = e.idx_x, prev_idy = e.idx_y;
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mdp_run, e, qx, qa, qb, j.mode, eps_thr, ext, j.seed, (uint32_t)(j.env_id_offset + i),
                                                  j.step_index + p, mgr0[p], sched[p], kv);
      // the accumulator targets: inside [0, 2 N_CELLS), and the cell of the row the env left with the action it took
      const int ax = e.action & 3, ay = (e.action >> 2) & 3;
      const struct { int cell; long long target; int prev, act; const char* what; } tgt[2] = {
          {o.cell, o.target_fx, prev_idx, ax, "cell"}, {o.cell_y, o.target_y_fx, prev_idy, ay, "cell_y"}};
      for (const auto& t : tgt) {
        if (t.cell < 0) continue;
        if (t.cell >= 2 * DQL_N_CELLS) violation(t.what, t.cell, 2 * DQL_N_CELLS);
        if (t.prev < 0 || t.prev >= N_STATES) violation(t.what, t.cell, t.prev);
        if (t.cell % DQL_N_CELLS != t.prev * 3 + t.act) violation(t.what, t.cell, (long long)t.prev * 3 + t.act);
        const int g = t.cell + (t.cell >= DQL_N_CELLS ? DQL_N_CELLS : 0);  // k_step's global layout [4][N_CELLS]
        out.acc[g] += (unsigned long long)t.target;
        out.acc[DQL_N_CELLS + g] += 1ull;
      }
      if (o.cell_y >= 0 && o.cell < 0) violation("cell_y without cell", o.cell_y, o.cell);
      qx = o.next;
      out.stats[0] += (unsigned long long)o.decision;
      out.stats[11] += (unsigned long long)o.reward_fx;
      if (o.done) { out.stats[1] += 1; if (e.code >= 0 && e.code <= DQL_TERMINAL_TIMEOUT) out.stats[2 + e.code] += 1; else violation("terminal code", e.code); }
    }
    store_env(e, sr.data(), si.data(), n, i, XMODE == X_ONLY ? x_only_(c) : c);
  }
  out.reals.resize((size_t)NF_REAL * n); out.ints.resize((size_t)NF_INT * n);
  for (int f = 0; f < NF_REAL; ++f) {
    const int q = f / 4, k = f % 4;
    for (long long i = 0; i < n; ++i) out.reals[(size_t)f * n + i] = (double)(&sr[(size_t)q * n + i].a)[k];
  }
  for (long long i = 0; i < n; ++i) {
    const int4 h = si[i];
    out.ints[0 * n + i] = h.x; out.ints[1 * n + i] = h.y; out.ints[2 * n + i] = h.z & 0xffff; out.ints[3 * n + i] = (h.z >> 16) & 0xffff;
    out.ints[4 * n + i] = h.w & 0xff; out.ints[5 * n + i] = (h.w >> 8) & 0xff; out.ints[6 * n + i] = (h.w >> 16) & 0xff;
  }
}

template <typename T, int TICK> bool dispatch_x(const Job& j, Result& r) {
  switch (j.xmode) {
    case X_TWO: launch<T, TICK, X_TWO>(j, r); return true;
    case X_ONLY: launch<T, TICK, X_ONLY>(j, r); return true;
    case X_RUNTIME: launch<T, TICK, X_RUNTIME>(j, r); return true;
  }
  return false;
}

bool dispatch(const Job& j, Result& r) {
  if (j.dtype == DQL_F64) return j.tick == TICK_PLAIN && dispatch_x<double, TICK_PLAIN>(j, r);
  switch (j.tick) {
    case TICK_PLAIN: return dispatch_x<float, TICK_PLAIN>(j, r);
    case TICK_PACKED: return dispatch_x<float, TICK_PACKED>(j, r);
    case TICK_LIT: return dispatch_x<float, TICK_LIT>(j, r);
    case TICK_PACKED_LITM: return dispatch_x<float, TICK_PACKED_LITM>(j, r);
  }
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string_view(argv[1]) == "--asan-selftest") {
    std::vector<int>* v = new std::vector<int>(8, 1);
    volatile const int* p = v->data();
    const int past = p[8];  // one past the end of a heap array
    std::printf("read %d\n", past);
    delete v;
    return 0;
  }
  if (argc == 3 && std::string_view(argv[1]) == "--admits") {  // may the literal-table instances serve this config?  (create_impl: refm, lit_ok)
    const Job j = read_job(argv[2]);
    const bool refm = refm_matches(make_mdpk<float>(j.cfg));
    KalFix kf;
    { const SimK<float> k = make_simk<float>(j.cfg); kf = KalFix{(double)k.kal_pss, (double)k.kal_kss, true}; }
    std::printf("%d %d\n", refm ? 1 : 0, (refm && refk_matches(make_simk<float>(j.cfg, &kf))) ? 1 : 0);
    return 0;
  }
  if (argc != 3) { std::fprintf(stderr, "usage: step_emu JOB OUT | --admits JOB | --asan-selftest\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (!dispatch(j, r)) { std::fprintf(stderr, "no such instance: dtype %d tick %d xmode %d\n", j.dtype, j.tick, j.xmode); return 2; }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  std::fwrite(r.reals.data(), sizeof(double), r.reals.size(), f);
  std::fwrite(r.ints.data(), sizeof(int32_t), r.ints.size(), f);
  std::fwrite(r.acc.data(), sizeof(unsigned long long), r.acc.size(), f);
  std::fwrite(r.stats, sizeof(unsigned long long), 12, f);
  std::fwrite(&r.bad_actions, sizeof(unsigned long long), 1, f);
  return std::fclose(f) == 0 ? 0 : 2;
}
