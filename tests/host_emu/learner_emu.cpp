// learner_emu.cpp — launches of the sequential-learner kernel k_learn, emulated on the CPU from the real device source (dql_learner.hpp's
// learner_periods on top of dql_device.hpp).
//
// For every learner the driver does what one lane of k_learn (dql_ensemble.inc) does: the launch's constants as the host side makes them (make_simk /
// make_mdpk / fill_schedule from the ensemble's period index), the env state arrays initialised as k_init initialises them, the learner's own table
// slices, learner_periods<TICK_PLAIN, X_ONLY>.  A lane runs alone: __ballot(p) is p (host_shim.h).  The job lists the lengths of the consecutive runs
// (launches); state, tables and counters live in arrays exactly as long as the ABI says, so the sanitized build sees any access beyond them.  Those arrays
// and the head of the result file (emu::LearnerState), the launch prologue (emu::Launch) and the job and result files are emu_common.h's; advance_emu.cpp
// uses the same.
//
//   learner_emu JOB OUT   run the launches described by JOB (see read_job; tests/test_learner_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#define DQL_EMU_LEARNERS
#include "emu_common.h"

using namespace dql;

namespace {

struct Job {
  int dtype, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> alpha, eps, qa, qb, count;
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[16];  // cfg size, dtype, L, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, 0
  int64_t seed;
  f.read(hdr, 16); f.read(&seed, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n = hdr[2]; j.n_runs = hdr[3];
  for (int k = 0; k < 4; ++k) j.runs[k] = hdr[4 + k];
  j.n_alpha = hdr[8]; j.n_eps = hdr[9]; j.window = hdr[10]; j.min_successes = hdr[11]; j.max_episodes = hdr[12]; j.log_cap = hdr[13]; j.has_tables = hdr[14];
  j.seed = (unsigned long long)seed;
  bool ok = j.n >= 1 && j.n_runs >= 1 && j.n_runs <= 4 && j.n_alpha >= 1 && j.n_eps >= 1 && j.window >= 1 && j.window <= LEARN_MAX_WINDOW && j.min_successes >= 1 &&
            j.max_episodes >= 1 && j.log_cap >= 1 && !j.cfg.two_axis && j.cfg.trajectory != DQL_TRAJ_EIGHT;
  for (int k = 0; ok && k < j.n_runs; ++k) ok = j.runs[k] >= 1 && j.runs[k] <= LEARN_MAX_PERIODS;
  if (!ok) emu::bad_job();
  j.alpha.resize((size_t)j.n_alpha); j.eps.resize((size_t)j.n_eps);
  f.read(j.alpha); f.read(j.eps);
  const size_t TB = (size_t)j.n * DQL_N_CELLS;
  j.qa.assign(TB, 0.0); j.qb.assign(TB, 0.0); j.count.assign(TB, 0.0);
  if (j.has_tables) { f.read(j.qa); f.read(j.qb); f.read(j.count); }
  return j;
}

template <typename T> int launch(Job& j, const char* out_path) {
  const dql_config& cfg = j.cfg;
  const size_t n = (size_t)j.n;
  const SimK<T> c = make_simk<T>(cfg);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  SimK<T> cl = c;
  cl.two_axis = 0;
  const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  emu::LearnerState<T> st(c, init, n, j.seed, j.log_cap);
  std::vector<uint32_t> thr((size_t)j.n_eps);
  for (int i = 0; i < j.n_eps; ++i) thr[(size_t)i] = eps_threshold(j.eps[(size_t)i]);
  const LearnSched sc{j.alpha.data(), j.n_alpha, cfg.alpha_min, thr.data(), j.n_eps, j.window, j.min_successes, j.max_episodes};
  const LearnMem mem = st.mem(j.qa, j.qb, j.count);
  long long j0 = 0;
  for (int r = 0; r < j.n_runs; ++r) {
    const int np = j.runs[r];
    std::vector<long long> mgr0((size_t)np);
    std::vector<int> sched((size_t)np);
    fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
    for (size_t l = 0; l < n; ++l)
      learner_periods<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, sc, mem, st.sr.data(), st.si.data(), j.seed, (long long)l, true, j0, np, mgr0.data(), sched.data(), lc.kv);
    j0 += np;
  }
  emu::ResultFile f(out_path);
  st.put(f, j.qa, j.qb, j.count);
  return f.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: learner_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
