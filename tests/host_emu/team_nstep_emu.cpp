// team_nstep_emu.cpp — launches of the team n-step kernel k_learn_team_nstep, emulated on the CPU from the real device source (dql_team.hpp's
// team_env_period, dql_team_nstep.hpp's team_apply_nstep, team_window_load and team_window_store on top of dql_nstep.hpp, dql_learner.hpp and dql_device.hpp).
//
// team_emu.cpp's driver with the envs' pending windows added.  For every live team it does what the team's lanes do in k_learn_team_nstep
// (dql_team_nstep.inc): the envs, their windows and the learner's counters loaded once per launch, per period team_env_period<TICK_PLAIN, X_ONLY> for the E
// envs one after the other into an array of E records, then the real team_apply_nstep on that array and on the team's windows; envs and windows stored at the
// launch's end.  What the kernel adds — the way through LDS and the two workgroup barriers per period — is program order here.  The windows are reached
// through checked references: the team's working copy is exactly [NSTEP_MAX][E] plus head and len [E], poisoned (keys 0xffff, rewards NaN, head and len
// far out of range) before every launch of every team, as LDS carries nothing from launch to launch; the persistent copy is exactly [NSTEP_MAX][L * E] plus
// len [L * E], its entries poisoned at the start.  An entry read before it was written, kept in the working copy only, or reached by lane instead of by env
// changes the result; an index outside an array ends the run with status 3.  A team frozen at a launch's start loads nothing and stores nothing.
//
// The job may rearm the learners after a run (team_checks' rearm: per-level counters, ring, promotion record and frozen flag cleared; envs and windows stay).
//
//   team_nstep_emu JOB OUT   run the launches described by JOB (see read_job; tests/test_team_nstep_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_team.hpp"
#include "dql_returns.hpp"
#include "dql_nstep.hpp"
#include "dql_team_nstep.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

struct Job {
  int dtype, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, envs_per_learner, nstep, rearm_after;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> alpha, eps, qa, qb, count;
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[18];  // cfg size, dtype, L, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, E, nstep, rearm_after (run index or -1)
  int64_t seed;
  f.read(hdr, 18); f.read(&seed, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n = hdr[2]; j.n_runs = hdr[3];
  for (int k = 0; k < 4; ++k) j.runs[k] = hdr[4 + k];
  j.n_alpha = hdr[8]; j.n_eps = hdr[9]; j.window = hdr[10]; j.min_successes = hdr[11]; j.max_episodes = hdr[12]; j.log_cap = hdr[13]; j.has_tables = hdr[14];
  j.envs_per_learner = hdr[15]; j.nstep = hdr[16]; j.rearm_after = hdr[17];
  j.seed = (unsigned long long)seed;
  bool ok = j.n >= 1 && j.n_runs >= 1 && j.n_runs <= 4 && j.n_alpha >= 1 && j.n_eps >= 1 && j.window >= 1 && j.window <= LEARN_MAX_WINDOW && j.min_successes >= 1 &&
            j.max_episodes >= 1 && j.log_cap >= 1 && !j.cfg.two_axis && j.cfg.trajectory != DQL_TRAJ_EIGHT && team_size_ok(j.envs_per_learner) && j.nstep >= 1 &&
            j.nstep <= NSTEP_MAX && j.rearm_after >= -1 && j.rearm_after < j.n_runs;
  for (int k = 0; ok && k < j.n_runs; ++k) ok = j.runs[k] >= 1 && j.runs[k] <= LEARN_MAX_PERIODS;
  if (!ok) emu::bad_job();
  j.alpha.resize((size_t)j.n_alpha); j.eps.resize((size_t)j.n_eps);
  f.read(j.alpha); f.read(j.eps);
  const size_t TB = (size_t)j.n * DQL_N_CELLS;
  j.qa.assign(TB, 0.0); j.qb.assign(TB, 0.0); j.count.assign(TB, 0.0);
  if (j.has_tables) { f.read(j.qa); f.read(j.qb); f.read(j.count); }
  return j;
}

// an array of the windows' storage as the device code indexes it: every element reached is bounds-checked
template <typename V> struct Checked {
  V* p; long long size; const char* what;
  V& operator[](long long k) const {
    if (k < 0 || k >= size) { std::fprintf(stderr, "INDEX VIOLATION: element %lld of %s outside [0, %lld)\n", k, what, size); std::exit(3); }
    return p[k];
  }
};
// dql_team_nstep.inc's LdsTeamWindow on a working copy of exactly E columns: [slot][e], head [e], len [e]; `first`: the column that env 0 of the view is
struct EmuTeamWindow {
  Checked<uint16_t> k; Checked<double> v; Checked<int> h, n; int E, first;
  long long at(int e, int slot) const {
    if (slot < 0 || slot >= NSTEP_MAX || e < 0 || first + e >= E) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d of env %d + %d of a team of %d\n", slot, first, e, E); std::exit(3); }
    return (long long)slot * E + first + e;
  }
  uint16_t& key(int e, int slot) const { return k[at(e, slot)]; }
  double& val(int e, int slot) const { return v[at(e, slot)]; }
  int& head(int e) const { return h[(long long)first + e]; }
  int& len(int e) const { return n[(long long)first + e]; }
};

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
  // the envs as k_init leaves them in a context of L * E envs
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
  // the persistent windows: as long as dql_ensemble_set_team_nstep allocates them; the lengths zeroed, the entries poisoned
  std::vector<uint16_t> g_key((size_t)NSTEP_MAX * n_envs, (uint16_t)0xffffu);
  std::vector<double> g_val((size_t)NSTEP_MAX * n_envs, std::nan(""));
  std::vector<int> g_len(n_envs, 0);
  const NstepMem<Checked<uint16_t>, Checked<double>, Checked<int>> tm{{g_key.data(), (long long)g_key.size(), "the persistent keys"},
                                                                      {g_val.data(), (long long)g_val.size(), "the persistent rewards"},
                                                                      {g_len.data(), (long long)g_len.size(), "the persistent lengths"}};
  // the team's working copy: exactly [NSTEP_MAX][E] and [E]
  std::vector<uint16_t> w_key((size_t)NSTEP_MAX * E);
  std::vector<double> w_val((size_t)NSTEP_MAX * E);
  std::vector<int> w_head(E), w_len(E);
  std::vector<Env<T>> envs(E);
  std::vector<TeamRecord> rec(E);  // exactly E records
  long long j0 = 0;
  for (int r = 0; r < j.n_runs; ++r) {
    const int np = j.runs[r];
    std::vector<long long> mgr0((size_t)np);
    std::vector<int> sched((size_t)np);
    fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
    for (size_t l = 0; l < n; ++l) {
      if (frozen[l]) continue;  // a frozen team's lanes load nothing and store nothing: its windows stay as they are
      w_key.assign(w_key.size(), (uint16_t)0xffffu); w_val.assign(w_val.size(), std::nan(""));
      w_head.assign(E, 1 << 20); w_len.assign(E, 1 << 20);
      const EmuTeamWindow team{{w_key.data(), (long long)w_key.size(), "the working keys"}, {w_val.data(), (long long)w_val.size(), "the working rewards"},
                               {w_head.data(), (long long)E, "the working heads"}, {w_len.data(), (long long)E, "the working lengths"}, (int)E, 0};
      TeamState ts = team_load(sc, mem, (long long)l);
      for (size_t k = 0; k < E; ++k) {
        load_env(envs[k], sr.data(), si[l * E + k], (long long)n_envs, (long long)(l * E + k), cl);
        EmuTeamWindow mine = team; mine.first = (int)k;  // the lane's own column
        team_window_load(tm, (long long)n_envs, (long long)(l * E + k), 0, j.nstep, mine);
      }
      const double* qa = j.qa.data() + l * DQL_N_CELLS;
      const double* qb = j.qb.data() + l * DQL_N_CELLS;
      for (int p = 0; p < np && ts.live; ++p) {
        const uint32_t eps_thr = ts.eps_thr;  // one threshold for the period, whatever team_apply_nstep makes of it meanwhile
        for (size_t k = 0; k < E; ++k)
          rec[k] = team_env_period<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, envs[k], qa, qb, eps_thr, j.seed, (long long)(l * E + k), j0 + p, mgr0[(size_t)p],
                                                       sched[(size_t)p], lc.kv);
        team_apply_nstep(sc, mem, cl.quirks, mdp_run.gamma, (long long)l, (const TeamRecord*)rec.data(), (int)E, j.nstep, team, ts);
      }
      for (size_t k = 0; k < E; ++k) {
        store_env(envs[k], sr.data(), si.data(), (long long)n_envs, (long long)(l * E + k), cl);
        EmuTeamWindow mine = team; mine.first = (int)k;
        team_window_store(tm, (long long)n_envs, (long long)(l * E + k), 0, j.nstep, mine);
      }
      team_store(ts, mem, (long long)l);
    }
    j0 += np;
    if (r == j.rearm_after)  // dql_ensemble_rearm: the windows are left alone
      for (size_t l = 0; l < n; ++l) { lvl[l] = 0; win_count[l] = 0; win_bits[l] = 0ull; win_bits[n + l] = 0ull; promoted[l] = -1; frozen[l] = 0; }
  }
  std::vector<double> reals;
  std::vector<int32_t> ints;
  emu::unpack_state(sr.data(), si.data(), n_envs, reals, ints);
  emu::ResultFile f(out_path);
  f.put(j.qa); f.put(j.qb); f.put(j.count); f.put(decisions); f.put(by_code);
  f.put(episodes); f.put(successes); f.put(lvl); f.put(promoted); f.put(frozen); f.put(log_n);
  f.put(log_code); f.put(log_len); f.put(reals); f.put(ints); f.put(faults);
  f.put(g_len);
  return f.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: team_nstep_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
