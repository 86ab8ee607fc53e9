// split_model_emu.cpp — one launch of the split transition-model kernel k_model_split, emulated on the CPU from the real device source (dql_model_split.hpp's
// model_split_episodes on top of dql_score.hpp, dql_rollout.hpp and dql_device.hpp).
//
// For every env of every table set the driver does what one lane of k_model_split (dql_model_split.inc) does: the launch's constants as the host side makes
// them, the lane's table set, its env id within the set, model_split_episodes<TICK_PLAIN, X_ONLY> with the one threshold eps_threshold(eps), the feature and the
// cut; the sink adds to the table set's four tables, and the wave's tally is added to the set's rows.  A lane runs alone: __ballot(p) is p (host_shim.h), so a
// "wave" is one lane — that two lanes of a wave hold the same (cell, s') in different halves shows on the GPU only.  The tables here are exactly as long as the
// ABI says, and the sink stops on an index outside them with exit status 3; every table read goes through TabRef and every cut read through CutRef; the schedule
// arrays are exactly max_steps + 1 long, so the sanitized build sees any access beyond them.
//
//   split_model_emu JOB OUT   run the launch described by JOB (see read_job; tests/test_split_model_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_score.hpp"
#include "dql_model_split.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

long long g_env = -1;

void table_violation(long long k) { emu::index_violation(k, "env", g_env); }

struct Job {
  int dtype, n_tables, max_steps, episodes, feature;
  long long n;  // envs per table set
  unsigned long long seed;
  double eps;
  dql_config cfg;
  std::vector<double> cut;     // [N_STATES]
  std::vector<double> qa, qb;  // [n_tables][N_CELLS]
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[8];  // cfg size, dtype, n_tables, max_steps, episodes, feature, 0, 0
  int64_t ll[2];   // envs per table set, seed
  double eps[1];
  f.read(hdr, 8); f.read(ll, 2); f.read(eps, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n_tables = hdr[2]; j.max_steps = hdr[3]; j.episodes = hdr[4]; j.feature = hdr[5];
  j.n = ll[0]; j.seed = (unsigned long long)ll[1]; j.eps = eps[0];
  if (j.n < 1 || j.n_tables < 1 || j.n_tables > DQL_MODEL_SPLIT_MAX_TABLES || j.max_steps < 1 || j.max_steps > DQL_SCORE_MAX_STEPS || j.episodes < 1 ||
      j.episodes > DQL_SCORE_MAX_EPISODES || !(j.eps >= 0.0 && j.eps <= 1.0) || j.cfg.two_axis || j.feature < 0 || j.feature >= DQL_SPLIT_N_FEATURES) emu::bad_job();
  j.cut.resize(DQL_N_STATES);
  f.read(j.cut);
  for (double c : j.cut) if (c != c) emu::bad_job();
  j.qa.resize((size_t)j.n_tables * DQL_N_CELLS); j.qb.resize(j.qa.size());
  f.read(j.qa); f.read(j.qb);
  return j;
}

struct Result {
  std::vector<uint32_t> pairs;
  std::vector<int64_t> reward_fx, terminal, feat_sum_fx, by_code, steps_sum, faults;
};

[[noreturn]] void violation(const char* what, long long a, long long b, long long c) {
  std::fprintf(stderr, "INDEX VIOLATION: %s (%lld, %lld, %lld) outside its table at env %lld\n", what, a, b, c, g_env);
  std::exit(3);
}

// the cut as the device code's CutPtr: every element read is bounds-checked
struct CutRef {
  const double* p;
  double operator[](long long s) const {
    if (s < 0 || s >= DQL_N_STATES) violation("cut", s, 0, 0);
    return p[s];
  }
};

// a table set's four tables: k_model_split's atomics as ordinary additions (one lane)
struct HostSink {
  uint32_t* p; int64_t* r; int64_t* t; int64_t* f;
  static bool row_ok(int half, int cell) { return half >= 0 && half < 2 && cell >= 0 && cell < DQL_N_CELLS; }
  void pair(int half, int cell, int next) {
    if (!row_ok(half, cell) || next < 0 || next >= DQL_N_STATES) violation("pair", half, cell, next);
    ++p[((size_t)half * DQL_N_CELLS + (size_t)cell) * DQL_N_STATES + (size_t)next];
  }
  void terminal(int half, int cell, int code) {
    if (!row_ok(half, cell) || code < 0 || code >= DQL_N_CHECK_CODES) violation("terminal", half, cell, code);
    ++t[((size_t)half * DQL_N_CELLS + (size_t)cell) * DQL_N_CHECK_CODES + (size_t)code];
  }
  void reward(int half, int cell, long long fx) {
    if (!row_ok(half, cell)) violation("reward", half, cell, 0);
    r[(size_t)half * DQL_N_CELLS + (size_t)cell] += fx;
  }
  void feature(int state, long long fx) {
    if (state < 0 || state >= DQL_N_STATES) violation("feature", state, 0, 0);
    f[state] += fx;
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
  // as dql_model_split prepares its buffers: everything zeroed
  const size_t rows = (size_t)j.n_tables * 2 * DQL_N_CELLS;
  out.pairs.assign(rows * DQL_N_STATES, 0u);
  out.reward_fx.assign(rows, 0); out.terminal.assign(rows * DQL_N_CHECK_CODES, 0); out.feat_sum_fx.assign((size_t)j.n_tables * DQL_N_STATES, 0);
  out.by_code.assign((size_t)j.n_tables * SCORE_N_COLS, 0); out.steps_sum.assign((size_t)j.n_tables, 0); out.faults.assign(1, 0);
  SimK<T> cl = c;
  cl.two_axis = 0;
  const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  const uint32_t eps_thr = eps_threshold(j.eps);
  const CutRef cut{j.cut.data()};
  for (int k = 0; k < j.n_tables; ++k) {
    const emu::TabRef qa{j.qa.data() + (size_t)k * DQL_N_CELLS, table_violation}, qb{j.qb.data() + (size_t)k * DQL_N_CELLS, table_violation};
    HostSink sink{out.pairs.data() + (size_t)k * 2 * DQL_N_CELLS * DQL_N_STATES, out.reward_fx.data() + (size_t)k * 2 * DQL_N_CELLS,
                  out.terminal.data() + (size_t)k * 2 * DQL_N_CELLS * DQL_N_CHECK_CODES, out.feat_sum_fx.data() + (size_t)k * DQL_N_STATES};
    for (long long i = 0; i < j.n; ++i) {
      g_env = (long long)k * j.n + i;
      const ModelSplitTally r = model_split_episodes<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, init, qa, qb, j.seed, (uint32_t)i, j.max_steps, j.episodes, eps_thr,
                                                                         j.feature, cut, mgr0.data(), sched.data(), lc.kv, sink);
      out.faults[0] += r.faults;
      for (int col = 0; col < SCORE_N_COLS; ++col) out.by_code[(size_t)k * SCORE_N_COLS + col] += r.t.by_code[col];
      out.steps_sum[(size_t)k] += (int64_t)r.t.steps;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: split_model_emu JOB OUT\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (j.dtype == DQL_F64) launch<double>(j, r); else launch<float>(j, r);
  emu::ResultFile f(argv[2]);
  f.put(r.pairs); f.put(r.reward_fx); f.put(r.terminal); f.put(r.feat_sum_fx); f.put(r.by_code); f.put(r.steps_sum); f.put(r.faults);
  return f.close();
}
