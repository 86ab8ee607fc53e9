// team_emu.cpp — launches of the team-learner kernel k_learn_team, emulated on the CPU from the real device source (dql_team.hpp's team_env_period and
// team_apply on top of dql_learner.hpp and dql_device.hpp).
//
// For every live team the driver does what the team's lanes do in k_learn_team (dql_teams.inc): the launch's constants as the host side makes them, the env
// state arrays of the L * E envs initialised as k_init initialises them, the envs and the learner's counters loaded once per launch, and per period
// team_env_period<TICK_PLAIN, X_ONLY> for the E envs one after the other into an array of E records, then the real team_apply on that array.  What the
// kernel adds to these two bodies — the records' way through LDS and the two workgroup barriers per period — is program order here.  Teams share nothing,
// so they are flown one after the other.  The job lists the lengths of the consecutive launches; state, tables and counters live in arrays exactly as
// long as the ABI says (per-learner arrays [L], per-env arrays [L * E]: emu_learners.h's LearnerState), so the sanitized build sees any access beyond them.
//
//   team_emu JOB OUT   run the launches described by JOB (emu::LearnerJob, word 15: E; tests/test_team_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include "emu_learners.h"
#include "dql_team.hpp"

using namespace dql;

namespace {

template <typename T> int launch(emu::LearnerJob& j, const char* out_path) {
  const size_t E = (size_t)j.word15;
  emu::PlainRun<T> p(j, E);
  emu::LearnerState<T>& st = p.st;
  const long long n_envs = (long long)st.n_envs;
  std::vector<Env<T>> envs(E);
  std::vector<TeamRecord> rec(E);  // exactly E records: team_apply reading a team-mate's beyond them is an ASan report
  emu::for_each_launch(j.cfg, j.runs, j.n_runs, [&](long long j0, int np, const long long* mgr0, const int* sched) {
    for (size_t l = 0; l < st.n; ++l) {
      if (st.frozen[l]) continue;  // a frozen team's lanes load nothing and store nothing
      TeamState ts = team_load(p.sc, p.mem, (long long)l);
      for (size_t k = 0; k < E; ++k) load_env(envs[k], st.sr.data(), st.si[l * E + k], n_envs, (long long)(l * E + k), p.cl);
      const double* qa = j.qa.data() + l * DQL_N_CELLS;
      const double* qb = j.qb.data() + l * DQL_N_CELLS;
      for (int q = 0; q < np && ts.live; ++q) {
        const uint32_t eps_thr = ts.eps_thr;  // one threshold for the period, whatever team_apply makes of it meanwhile
        for (size_t k = 0; k < E; ++k)
          rec[k] = team_env_period<TICK_PLAIN, X_ONLY>(p.cl, p.lc.cfgk, p.lc.tc, p.mdp, p.k.mdp_run, envs[k], qa, qb, eps_thr, j.seed, (long long)(l * E + k), j0 + q, mgr0[q], sched[q], p.lc.kv);
        team_apply(p.sc, p.mem, p.cl.quirks, p.k.mdp_run.gamma, (long long)l, (const TeamRecord*)rec.data(), (int)E, ts);
      }
      for (size_t k = 0; k < E; ++k) store_env(envs[k], st.sr.data(), st.si.data(), n_envs, (long long)(l * E + k), p.cl);
      team_store(ts, p.mem, (long long)l);
    }
  });
  return emu::write_result(out_path, st, j);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: team_emu JOB OUT\n"); return 2; }
  emu::LearnerJob j(argv[1], 0, [](const emu::LearnerJob& q) { return team_size_ok(q.word15); });
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
