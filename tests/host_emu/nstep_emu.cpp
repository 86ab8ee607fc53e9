// nstep_emu.cpp — launches of the n-step learner kernel k_learn_nstep, emulated on the CPU from the real device source (dql_nstep.hpp's
// learner_periods_nstep on top of dql_learner.hpp and dql_device.hpp).
//
// learner_emu.cpp's driver with the pending windows added.  For every learner it does what one lane of k_learn_nstep (dql_nstep.inc) does: the launch's
// constants as the host side makes them, the env state arrays as k_init leaves them, the learner's own table slices, learner_periods_nstep<TICK_PLAIN,
// X_ONLY>.  A lane runs alone: __ballot(p) is p (host_shim.h).  The windows are reached through checked references: the launch's working copy stands for the
// kernel's LDS ([NSTEP_MAX][64], the learner in column l mod 64), the persistent copy is [NSTEP_MAX][n] plus len[n], exactly as long as the library's; both
// are poisoned (keys 0xffff, rewards NaN) — the working copy before every launch of every lane, as LDS carries nothing from launch to launch — so an entry
// read before it was written, or kept in the working copy only, changes the result.  An index outside them ends the run with status 3.
//
//   nstep_emu JOB OUT   run the launches described by JOB (see read_job; tests/test_nstep_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_returns.hpp"
#include "dql_nstep.hpp"
#define DQL_EMU_LEARNERS
#include "emu_common.h"

using namespace dql;

namespace {

struct Job {
  int dtype, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, nstep;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> alpha, eps, qa, qb, count;
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[16];  // cfg size, dtype, L, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, nstep
  int64_t seed;
  f.read(hdr, 16); f.read(&seed, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n = hdr[2]; j.n_runs = hdr[3];
  for (int k = 0; k < 4; ++k) j.runs[k] = hdr[4 + k];
  j.n_alpha = hdr[8]; j.n_eps = hdr[9]; j.window = hdr[10]; j.min_successes = hdr[11]; j.max_episodes = hdr[12]; j.log_cap = hdr[13]; j.has_tables = hdr[14]; j.nstep = hdr[15];
  j.seed = (unsigned long long)seed;
  bool ok = j.n >= 1 && j.n_runs >= 1 && j.n_runs <= 4 && j.n_alpha >= 1 && j.n_eps >= 1 && j.window >= 1 && j.window <= LEARN_MAX_WINDOW && j.min_successes >= 1 &&
            j.max_episodes >= 1 && j.log_cap >= 1 && !j.cfg.two_axis && j.cfg.trajectory != DQL_TRAJ_EIGHT && j.nstep >= 1 && j.nstep <= NSTEP_MAX;
  for (int k = 0; ok && k < j.n_runs; ++k) ok = j.runs[k] >= 1 && j.runs[k] <= LEARN_MAX_PERIODS;
  if (!ok) emu::bad_job();
  j.alpha.resize((size_t)j.n_alpha); j.eps.resize((size_t)j.n_eps);
  f.read(j.alpha); f.read(j.eps);
  const size_t TB = (size_t)j.n * DQL_N_CELLS;
  j.qa.assign(TB, 0.0); j.qb.assign(TB, 0.0); j.count.assign(TB, 0.0);
  if (j.has_tables) { f.read(j.qa); f.read(j.qb); f.read(j.count); }
  return j;
}

// an array of the window's storage as the device code indexes it: every element reached is bounds-checked
template <typename V> struct Checked {
  V* p; long long size; const char* what;
  V& operator[](long long k) const {
    if (k < 0 || k >= size) { std::fprintf(stderr, "INDEX VIOLATION: element %lld of %s outside [0, %lld)\n", k, what, size); std::exit(3); }
    return p[k];
  }
};
struct EmuWindow {  // dql_nstep.inc's LdsWindow
  Checked<uint16_t> k; Checked<double> v; int lane;
  uint16_t& key(int slot) const { if (slot < 0 || slot >= NSTEP_MAX) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d\n", slot); std::exit(3); } return k[(long long)slot * 64 + lane]; }
  double& val(int slot) const { if (slot < 0 || slot >= NSTEP_MAX) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d\n", slot); std::exit(3); } return v[(long long)slot * 64 + lane]; }
};

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
  // the persistent windows: as long as dql_ensemble_set_nstep allocates them; the lengths zeroed, the entries poisoned
  std::vector<uint16_t> g_key((size_t)NSTEP_MAX * n, (uint16_t)0xffffu);
  std::vector<double> g_val((size_t)NSTEP_MAX * n, std::nan(""));
  std::vector<int> g_len(n, 0);
  const NstepMem<Checked<uint16_t>, Checked<double>, Checked<int>> nm{{g_key.data(), (long long)g_key.size(), "the persistent keys"},
                                                                      {g_val.data(), (long long)g_val.size(), "the persistent rewards"},
                                                                      {g_len.data(), (long long)g_len.size(), "the persistent lengths"}};
  std::vector<uint16_t> lds_key((size_t)NSTEP_MAX * 64);
  std::vector<double> lds_val((size_t)NSTEP_MAX * 64);
  long long j0 = 0;
  for (int r = 0; r < j.n_runs; ++r) {
    const int np = j.runs[r];
    std::vector<long long> mgr0((size_t)np);
    std::vector<int> sched((size_t)np);
    fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
    for (size_t l = 0; l < n; ++l) {
      lds_key.assign(lds_key.size(), (uint16_t)0xffffu); lds_val.assign(lds_val.size(), std::nan(""));
      const EmuWindow win{{lds_key.data(), (long long)lds_key.size(), "the working keys"}, {lds_val.data(), (long long)lds_val.size(), "the working rewards"}, (int)(l % 64)};
      learner_periods_nstep<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, sc, mem, st.sr.data(), st.si.data(), j.seed, (long long)l, true, j0, np, mgr0.data(), sched.data(), lc.kv,
                                                j.nstep, win, nm);
    }
    j0 += np;
  }
  emu::ResultFile f(out_path);
  st.put(f, j.qa, j.qb, j.count);
  f.put(g_len);
  return f.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: nstep_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
