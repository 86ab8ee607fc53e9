// team_emu.cpp — launches of the team-learner kernel k_learn_team, emulated on the CPU from the real device source (dql_team.hpp's team_env_period and
// team_apply on top of dql_learner.hpp and dql_device.hpp).
//
// For every live team the driver does what the team's lanes do in k_learn_team (dql_teams.inc): the launch's constants as the host side makes them, the env
// state arrays of the L * E envs initialised as k_init initialises them, the envs and the learner's counters loaded once per launch, and per period
// team_env_period<TICK_PLAIN, X_ONLY> for the E envs one after the other into an array of E records, then the real team_apply on that array.  What the
// kernel adds to these two bodies — the records' way through LDS and the two workgroup barriers per period — is program order here.  Teams share nothing,
// so they are flown one after the other.  The job lists the lengths of the consecutive launches; state, tables and counters live in arrays exactly as
// long as the ABI says (per-learner arrays [L], per-env arrays [L * E]), so the sanitized build sees any access beyond them.
//
//   team_emu JOB OUT   run the launches described by JOB (see read_job; tests/test_team_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_team.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

struct Job {
  int dtype, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, envs_per_learner;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> alpha, eps, qa, qb, count;
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[16];  // cfg size, dtype, L, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, E
  int64_t seed;
  f.read(hdr, 16); f.read(&seed, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n = hdr[2]; j.n_runs = hdr[3];
  for (int k = 0; k < 4; ++k) j.runs[k] = hdr[4 + k];
  j.n_alpha = hdr[8]; j.n_eps = hdr[9]; j.window = hdr[10]; j.min_successes = hdr[11]; j.max_episodes = hdr[12]; j.log_cap = hdr[13]; j.has_tables = hdr[14];
  j.envs_per_learner = hdr[15];
  j.seed = (unsigned long long)seed;
  bool ok = j.n >= 1 && j.n_runs >= 1 && j.n_runs <= 4 && j.n_alpha >= 1 && j.n_eps >= 1 && j.window >= 1 && j.window <= LEARN_MAX_WINDOW && j.min_successes >= 1 &&
            j.max_episodes >= 1 && j.log_cap >= 1 && !j.cfg.two_axis && j.cfg.trajectory != DQL_TRAJ_EIGHT && team_size_ok(j.envs_per_learner);
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
  const size_t n = (size_t)j.n, E = (size_t)j.envs_per_learner, n_envs = n * E, cap = (size_t)j.log_cap;
  const SimK<T> c = make_simk<T>(cfg);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  SimK<T> cl = c;
  cl.two_axis = 0;
  const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  // the envs as k_init leaves them in a context of L * E envs (emu_common.h's LearnerState does the same for L)
  std::vector<Quad<T>> sr((size_t)NQ_REAL * n_envs, Quad<T>{T(0.0), T(0.0), T(0.0), T(0.0)});
  std::vector<int4> si(n_envs);
  for (size_t g = 0; g < n_envs; ++g) {
    Env<T> e; T mp_v_hbm;
    rollout_init_env(cl, init, e, (uint32_t)g, j.seed, mp_v_hbm);
    sr[11 * n_envs + g] = Quad<T>{mp_v_hbm, T(0.0), T(0.0), T(1.0)};
    sr[13 * n_envs + g] = Quad<T>{e.mp_r, e.mp_w, T(0.0), T(0.0)};
    store_env(e, sr.data(), si.data(), (long long)n_envs, (long long)g, c);
  }
  // the learners' counters, zeroed as dql_ensemble_create_teams leaves them
  std::vector<unsigned long long> decisions(n, 0ull), by_code((size_t)DQL_N_CHECK_CODES * n, 0ull), win_bits(2 * n, 0ull), faults(1, 0ull);
  std::vector<int> episodes(n, 0), successes(n, 0), lvl(n, 0), win_count(n, 0), promoted(n, -1), frozen(n, 0), log_n(n, 0);
  std::vector<uint8_t> log_code(n * cap, 0);
  std::vector<uint16_t> log_len(n * cap, 0);
  const LearnMem mem{j.qa.data(), j.qb.data(), j.count.data(), decisions.data(), by_code.data(), episodes.data(), successes.data(), lvl.data(), win_count.data(),
                     win_bits.data(), promoted.data(), frozen.data(), log_code.data(), log_len.data(), log_n.data(), faults.data(), (long long)n, j.log_cap};
  std::vector<uint32_t> thr((size_t)j.n_eps);
  for (int i = 0; i < j.n_eps; ++i) thr[(size_t)i] = eps_threshold(j.eps[(size_t)i]);
  const LearnSched sc{j.alpha.data(), j.n_alpha, cfg.alpha_min, thr.data(), j.n_eps, j.window, j.min_successes, j.max_episodes};
  std::vector<Env<T>> envs(E);
  std::vector<TeamRecord> rec(E);  // exactly E records: team_apply reading a team-mate's beyond them is an ASan report
  long long j0 = 0;
  for (int r = 0; r < j.n_runs; ++r) {
    const int np = j.runs[r];
    std::vector<long long> mgr0((size_t)np);
    std::vector<int> sched((size_t)np);
    fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
    for (size_t l = 0; l < n; ++l) {
      if (frozen[l]) continue;  // a frozen team's lanes load nothing and store nothing
      TeamState ts = team_load(sc, mem, (long long)l);
      for (size_t k = 0; k < E; ++k) load_env(envs[k], sr.data(), si[l * E + k], (long long)n_envs, (long long)(l * E + k), cl);
      const double* qa = j.qa.data() + l * DQL_N_CELLS;
      const double* qb = j.qb.data() + l * DQL_N_CELLS;
      for (int p = 0; p < np && ts.live; ++p) {
        const uint32_t eps_thr = ts.eps_thr;  // one threshold for the period, whatever team_apply makes of it meanwhile
        for (size_t k = 0; k < E; ++k)
          rec[k] = team_env_period<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, envs[k], qa, qb, eps_thr, j.seed, (long long)(l * E + k), j0 + p, mgr0[(size_t)p],
                                                       sched[(size_t)p], lc.kv);
        team_apply(sc, mem, cl.quirks, mdp_run.gamma, (long long)l, (const TeamRecord*)rec.data(), (int)E, ts);
      }
      for (size_t k = 0; k < E; ++k) store_env(envs[k], sr.data(), si.data(), (long long)n_envs, (long long)(l * E + k), cl);
      team_store(ts, mem, (long long)l);
    }
    j0 += np;
  }
  std::vector<double> reals;
  std::vector<int32_t> ints;
  emu::unpack_state(sr.data(), si.data(), n_envs, reals, ints);
  emu::ResultFile f(out_path);
  f.put(j.qa); f.put(j.qb); f.put(j.count); f.put(decisions); f.put(by_code);
  f.put(episodes); f.put(successes); f.put(lvl); f.put(promoted); f.put(frozen); f.put(log_n);
  f.put(log_code); f.put(log_len); f.put(reals); f.put(ints); f.put(faults);
  return f.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: team_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
