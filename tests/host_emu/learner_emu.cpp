// learner_emu.cpp — launches of the sequential-learner kernel k_learn, emulated on the CPU from the real device source (dql_learner.hpp's
// learner_periods on top of dql_device.hpp).
//
// For every learner the driver does what one lane of k_learn (dql_ensemble.inc) does: the launch's constants as the host side makes them (make_simk /
// make_mdpk / fill_schedule from the ensemble's period index), the env state arrays initialised as k_init initialises them, the learner's own table
// slices, learner_periods<TICK_PLAIN, X_ONLY>.  A lane runs alone: __ballot(p) is p (host_shim.h).  The job lists the lengths of the consecutive runs
// (launches); state, tables and counters live in arrays exactly as long as the ABI says, so the sanitized build sees any access beyond them.
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

using namespace dql;

namespace {

struct Job {
  int dtype, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> alpha, eps, qa, qb, count;
};

template <typename V> void read_into(FILE* f, V* p, size_t n) {
  if (n && std::fread(p, sizeof(V), n, f) != n) { std::fprintf(stderr, "short job file\n"); std::exit(2); }
}

Job read_job(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  Job j;
  int32_t hdr[16];  // cfg size, dtype, L, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, 0
  int64_t seed;
  read_into(f, hdr, 16); read_into(f, &seed, 1);
  if (hdr[0] != (int32_t)sizeof(dql_config)) { std::fprintf(stderr, "dql_config size %d != %d\n", hdr[0], (int)sizeof(dql_config)); std::exit(2); }
  read_into(f, &j.cfg, 1);
  j.dtype = hdr[1]; j.n = hdr[2]; j.n_runs = hdr[3];
  for (int k = 0; k < 4; ++k) j.runs[k] = hdr[4 + k];
  j.n_alpha = hdr[8]; j.n_eps = hdr[9]; j.window = hdr[10]; j.min_successes = hdr[11]; j.max_episodes = hdr[12]; j.log_cap = hdr[13]; j.has_tables = hdr[14];
  j.seed = (unsigned long long)seed;
  bool ok = j.n >= 1 && j.n_runs >= 1 && j.n_runs <= 4 && j.n_alpha >= 1 && j.n_eps >= 1 && j.window >= 1 && j.window <= LEARN_MAX_WINDOW && j.min_successes >= 1 &&
            j.max_episodes >= 1 && j.log_cap >= 1 && !j.cfg.two_axis && j.cfg.trajectory != DQL_TRAJ_EIGHT;
  for (int k = 0; ok && k < j.n_runs; ++k) ok = j.runs[k] >= 1 && j.runs[k] <= LEARN_MAX_PERIODS;
  if (!ok) { std::fprintf(stderr, "bad job\n"); std::exit(2); }
  j.alpha.resize((size_t)j.n_alpha); j.eps.resize((size_t)j.n_eps);
  read_into(f, j.alpha.data(), j.alpha.size()); read_into(f, j.eps.data(), j.eps.size());
  const size_t TB = (size_t)j.n * DQL_N_CELLS;
  j.qa.assign(TB, 0.0); j.qb.assign(TB, 0.0); j.count.assign(TB, 0.0);
  if (j.has_tables) { read_into(f, j.qa.data(), TB); read_into(f, j.qb.data(), TB); read_into(f, j.count.data(), TB); }
  std::fclose(f);
  return j;
}

template <typename V> void put(FILE* f, const std::vector<V>& v) { std::fwrite(v.data(), sizeof(V), v.size(), f); }

template <typename T> int launch(Job& j, const char* out_path) {
  const dql_config& cfg = j.cfg;
  const size_t n = (size_t)j.n;
  const SimK<T> c = make_simk<T>(cfg);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  SimK<T> cl = c;
  cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  const TickConsts<TICK_PLAIN, T> tc(cfgk);
  uint32_t kv_[20];
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4) {
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)j.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(j.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  // the state arrays as k_init leaves them
  std::vector<Quad<T>> sr((size_t)NQ_REAL * n, Quad<T>{T(0.0), T(0.0), T(0.0), T(0.0)});
  std::vector<int4> si(n);
  for (size_t l = 0; l < n; ++l) {
    Env<T> e; T mp_v_hbm;
    rollout_init_env(cl, init, e, (uint32_t)l, j.seed, mp_v_hbm);
    sr[11 * n + l] = Quad<T>{mp_v_hbm, T(0.0), T(0.0), T(1.0)};
    sr[13 * n + l] = Quad<T>{e.mp_r, e.mp_w, T(0.0), T(0.0)};
    store_env(e, sr.data(), si.data(), (long long)n, (long long)l, c);
  }
  std::vector<uint32_t> thr((size_t)j.n_eps);
  for (int i = 0; i < j.n_eps; ++i) thr[(size_t)i] = eps_threshold(j.eps[(size_t)i]);
  const LearnSched sc{j.alpha.data(), j.n_alpha, cfg.alpha_min, thr.data(), j.n_eps, j.window, j.min_successes, j.max_episodes};
  std::vector<unsigned long long> decisions(n, 0ull), by_code((size_t)DQL_N_CHECK_CODES * n, 0ull), win_bits(2 * n, 0ull), faults(1, 0ull);
  std::vector<int> episodes(n, 0), successes(n, 0), lvl(n, 0), win_count(n, 0), promoted(n, -1), frozen(n, 0), log_n(n, 0);
  std::vector<uint8_t> log_code(n * (size_t)j.log_cap, 0);
  std::vector<uint16_t> log_len(n * (size_t)j.log_cap, 0);
  const LearnMem mem{j.qa.data(), j.qb.data(), j.count.data(), decisions.data(), by_code.data(), episodes.data(), successes.data(), lvl.data(), win_count.data(),
                     win_bits.data(), promoted.data(), frozen.data(), log_code.data(), log_len.data(), log_n.data(), faults.data(), (long long)n, j.log_cap};
  long long j0 = 0;
  for (int r = 0; r < j.n_runs; ++r) {
    const int np = j.runs[r];
    std::vector<long long> mgr0((size_t)np);
    std::vector<int> sched((size_t)np);
    fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
    for (size_t l = 0; l < n; ++l)
      learner_periods<TICK_PLAIN, X_ONLY>(cl, cfgk, tc, mdp, mdp_run, sc, mem, sr.data(), si.data(), j.seed, (long long)l, true, j0, np, mgr0.data(), sched.data(), kv);
    j0 += np;
  }
  std::vector<double> reals((size_t)NF_REAL * n);
  std::vector<int32_t> ints((size_t)NF_INT * n);
  for (int f = 0; f < NF_REAL; ++f)
    for (size_t l = 0; l < n; ++l) { const Quad<T>& q = sr[(size_t)(f / 4) * n + l]; const T v = (f % 4 == 0) ? q.a : (f % 4 == 1) ? q.b : (f % 4 == 2) ? q.c : q.d; reals[(size_t)f * n + l] = (double)v; }
  for (size_t l = 0; l < n; ++l) {
    const int4 h = si[l];
    ints[0 * n + l] = h.x; ints[1 * n + l] = h.y; ints[2 * n + l] = h.z & 0xffff; ints[3 * n + l] = (h.z >> 16) & 0xffff;
    ints[4 * n + l] = h.w & 0xff; ints[5 * n + l] = (h.w >> 8) & 0xff; ints[6 * n + l] = (h.w >> 16) & 0xff;
  }
  FILE* f = std::fopen(out_path, "wb");
  if (!f) { std::perror(out_path); return 2; }
  put(f, j.qa); put(f, j.qb); put(f, j.count); put(f, decisions); put(f, by_code);
  put(f, episodes); put(f, successes); put(f, lvl); put(f, promoted); put(f, frozen); put(f, log_n);
  put(f, log_code); put(f, log_len); put(f, reals); put(f, ints); put(f, faults);
  return std::fclose(f) == 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: learner_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
