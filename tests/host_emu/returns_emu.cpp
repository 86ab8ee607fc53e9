// returns_emu.cpp — one call of the realised-returns kernels k_returns_fly + k_returns_sweep, emulated on the CPU from the real device source (dql_returns.hpp's
// ReturnsLogSink and returns_sweep on top of dql_model.hpp's model_episodes, dql_score.hpp, dql_rollout.hpp and dql_device.hpp).
//
// For every env of every table set the driver does what one lane of k_returns_fly (dql_returns.inc) does — the launch's constants as the host side makes them,
// the lane's table set, its env id within the set, its column of the log, model_episodes<TICK_PLAIN, X_ONLY> with the log sink — and then, column by column, what
// one lane of k_returns_sweep does: returns_sweep with the column's decision count, the accumulator adding to the table set's two tables.  A lane runs alone:
// __ballot(p) is p (host_shim.h), a "wave" is one lane, so t_top is the lane's own decision count — 64 lanes of different lengths sweeping together and the LDS
// staging show on the GPU only.  The log is exactly (max_steps + 1) x n_columns words long and every access to it goes through a checked reference (exit status
// 3 outside it); it is filled with a poison pattern (end flag set, cell 4095) before the flight, so a word read that was never written trips a range check or
// changes a result.  Every table read goes through TabRef; the schedule arrays are exactly max_steps + 1 long.
//
//   returns_emu JOB OUT   run the call described by JOB (see read_job; tests/test_returns_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_score.hpp"
#include "dql_model.hpp"
#include "dql_returns.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

long long g_env = -1;

void table_violation(long long k) { emu::index_violation(k, "env", g_env); }

struct Job {
  int dtype, n_tables, max_steps, episodes;
  long long n;  // envs per table set
  unsigned long long seed;
  double eps, gamma, g_bound;
  dql_config cfg;
  std::vector<double> qa, qb;  // [n_tables][N_CELLS]
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[6];  // cfg size, dtype, n_tables, max_steps, episodes, 0
  int64_t ll[2];   // envs per table set, seed
  double d[3];     // eps, gamma, g_bound (ceil(B 2^26) of the overflow guard)
  f.read(hdr, 6); f.read(ll, 2); f.read(d, 3);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n_tables = hdr[2]; j.max_steps = hdr[3]; j.episodes = hdr[4];
  j.n = ll[0]; j.seed = (unsigned long long)ll[1]; j.eps = d[0]; j.gamma = d[1]; j.g_bound = d[2];
  if (j.n < 1 || j.n_tables < 1 || j.n_tables > 16 || j.max_steps < 1 || j.max_steps > DQL_SCORE_MAX_STEPS || j.episodes < 1 || j.episodes > DQL_SCORE_MAX_EPISODES ||
      !(j.eps >= 0.0 && j.eps <= 1.0) || !(j.gamma >= 0.0 && j.gamma <= 1.0) || !(j.g_bound >= 0.0) || j.cfg.two_axis) emu::bad_job();
  j.qa.resize((size_t)j.n_tables * DQL_N_CELLS); j.qb.resize(j.qa.size());
  f.read(j.qa); f.read(j.qb);
  return j;
}

struct Result {
  std::vector<int64_t> visits, return_fx, cut, by_code, steps_sum, faults;
};

// the decision log as the device code's WordPtr: every element touched is bounds-checked
struct LogRef {
  unsigned long long* p;
  size_t n;
  unsigned long long& operator[](size_t k) const {
    if (k >= n) { std::fprintf(stderr, "INDEX VIOLATION: log word %zu outside [0, %zu) at env %lld\n", k, n, g_env); std::exit(3); }
    return p[k];
  }
};

// a table set's two tables: k_returns_sweep's LDS atomics and their flush as ordinary additions (one lane)
struct HostAcc {
  int64_t* v; int64_t* g;
  void add(int cell, long long g_fx) {
    if (cell < 0 || cell >= DQL_N_CELLS) { std::fprintf(stderr, "INDEX VIOLATION: cell %d outside its table at env %lld\n", cell, g_env); std::exit(3); }
    ++v[cell];
    g[cell] += g_fx;
  }
};

template <typename T> void launch(const Job& j, Result& out) {
  const dql_config& cfg = j.cfg;
  const SimK<T> c = make_simk<T>(cfg);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  std::vector<long long> mgr0((size_t)j.max_steps + 1);
  std::vector<int> sched((size_t)j.max_steps + 1);
  fill_schedule(cfg, 0, mgr0.data(), sched.data(), j.max_steps + 1);
  const size_t n_columns = (size_t)j.n_tables * (size_t)j.n;
  const unsigned capacity = (unsigned)(j.max_steps + 1);
  // as dql_returns prepares its buffers: the sums zeroed, the log NOT (here: poisoned)
  std::vector<unsigned long long> traj((size_t)capacity * n_columns, ~0ull);
  std::vector<unsigned> n_dec(n_columns, 0u);
  out.visits.assign((size_t)j.n_tables * DQL_N_CELLS, 0); out.return_fx.assign((size_t)j.n_tables * DQL_N_CELLS, 0); out.cut.assign((size_t)j.n_tables, 0);
  out.by_code.assign((size_t)j.n_tables * SCORE_N_COLS, 0); out.steps_sum.assign((size_t)j.n_tables, 0); out.faults.assign(1, 0);
  SimK<T> cl = c;
  cl.two_axis = 0;
  const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  const uint32_t eps_thr = eps_threshold(j.eps);
  const LogRef log{traj.data(), traj.size()};
  // k_returns_fly
  for (int k = 0; k < j.n_tables; ++k) {
    const emu::TabRef qa{j.qa.data() + (size_t)k * DQL_N_CELLS, table_violation}, qb{j.qb.data() + (size_t)k * DQL_N_CELLS, table_violation};
    for (long long i = 0; i < j.n; ++i) {
      const size_t column = (size_t)k * (size_t)j.n + (size_t)i;
      g_env = (long long)column;
      ReturnsLogSink<LogRef> sink{log, n_columns, column, capacity};
      const ModelTally r = model_episodes<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, init, qa, qb, j.seed, (uint32_t)i, j.max_steps, j.episodes, eps_thr, mgr0.data(),
                                                              sched.data(), lc.kv, sink);
      n_dec[column] = sink.n_dec;
      out.faults[0] += r.faults + sink.faults;
      for (int col = 0; col < SCORE_N_COLS; ++col) out.by_code[(size_t)k * SCORE_N_COLS + col] += r.t.by_code[col];
      out.steps_sum[(size_t)k] += (int64_t)r.t.steps;
    }
  }
  // k_returns_sweep
  for (size_t column = 0; column < n_columns; ++column) {
    const size_t k = column / (size_t)j.n;
    g_env = (long long)column;
    HostAcc acc{out.visits.data() + k * DQL_N_CELLS, out.return_fx.data() + k * DQL_N_CELLS};
    const unsigned top = n_dec[column] <= capacity ? n_dec[column] : 0u;
    const ReturnsSweepTally r = returns_sweep(log, n_columns, column, n_dec[column], capacity, (int)top, j.gamma, j.g_bound, acc);
    out.cut[k] += (int64_t)r.cut;
    out.faults[0] += r.faults;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: returns_emu JOB OUT\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (j.dtype == DQL_F64) launch<double>(j, r); else launch<float>(j, r);
  emu::ResultFile f(argv[2]);
  f.put(r.visits); f.put(r.return_fx); f.put(r.cut); f.put(r.by_code); f.put(r.steps_sum); f.put(r.faults);
  return f.close();
}
