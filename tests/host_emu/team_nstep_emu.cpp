// team_nstep_emu.cpp — launches of the team n-step kernel k_learn_team_nstep, emulated on the CPU from the real device source (dql_team.hpp's
// team_env_period, dql_team_nstep.hpp's team_apply_nstep, team_window_load and team_window_store on top of dql_nstep.hpp, dql_learner.hpp and dql_device.hpp).
//
// For every live team it does what the team's lanes do in k_learn_team_nstep (dql_team_nstep.inc): the envs, their windows and the learner's counters loaded
// once per launch, per period team_env_period<TICK_PLAIN, X_ONLY> for the E envs one after the other into an array of E records, then the real
// team_apply_nstep on that array and on the team's windows; envs and windows stored at the launch's end.  What the kernel adds — the way through LDS and the
// two workgroup barriers per period — is program order here.  The windows are reached through checked references (emu_learners.h's Checked): the team's
// working copy is exactly [NSTEP_MAX][E] plus head and len [E], poisoned (keys 0xffff, rewards NaN, head and len far out of range) before every launch of
// every team, as LDS carries nothing from launch to launch; the persistent copy is exactly [NSTEP_MAX][L * E] plus len [L * E], its entries poisoned at the
// start.  An entry read before it was written, kept in the working copy only, or reached by lane instead of by env changes the result; an index outside an
// array ends the run with status 3.  A team frozen at a launch's start loads nothing and stores nothing.
//
// The job may rearm the learners after a run (team_checks' rearm: per-level counters, ring, promotion record and frozen flag cleared; envs and windows stay).
//
//   team_nstep_emu JOB OUT   run the launches described by JOB (emu::LearnerJob, word 15: E, two extra words: n, rearm_after (run index or -1);
//                            tests/test_team_nstep_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include "emu_learners.h"
#include "dql_team.hpp"
#include "dql_team_nstep.hpp"

using namespace dql;

namespace {

// dql_team_nstep.inc's LdsTeamWindow on a working copy of exactly E columns: [slot][e], head [e], len [e]
struct EmuTeamWindow {
  const int E;
  std::vector<uint16_t> key;
  std::vector<double> val;
  std::vector<int> head, len;
  explicit EmuTeamWindow(size_t E_) : E((int)E_), key((size_t)NSTEP_MAX * E_), val((size_t)NSTEP_MAX * E_), head(E_), len(E_) {}
  void poison() { emu::poison(key, val); emu::poison(head); emu::poison(len); }
  struct View {  // `first`: the column that env 0 of the view is
    emu::Checked<uint16_t> k; emu::Checked<double> v; emu::Checked<int> h, n; int E, first;
    long long at(int e, int slot) const {
      if (slot < 0 || slot >= NSTEP_MAX || e < 0 || first + e >= E) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d of env %d + %d of a team of %d\n", slot, first, e, E); std::exit(3); }
      return (long long)slot * E + first + e;
    }
    uint16_t& key(int e, int slot) const { return k[at(e, slot)]; }
    double& val(int e, int slot) const { return v[at(e, slot)]; }
    int& head(int e) const { return h[(long long)first + e]; }
    int& len(int e) const { return n[(long long)first + e]; }
  };
  View view(size_t first) {
    return View{emu::checked(key, "the working keys"), emu::checked(val, "the working rewards"), emu::checked(head, "the working heads"), emu::checked(len, "the working lengths"), E, (int)first};
  }
};

template <typename T> int launch(emu::LearnerJob& j, const char* out_path) {
  const size_t E = (size_t)j.word15;
  const int nstep = j.extra[0], rearm_after = j.extra[1];
  emu::PlainRun<T> p(j, E);
  emu::LearnerState<T>& st = p.st;
  const long long n_envs = (long long)st.n_envs;
  emu::PersistentWindows pw(st.n_envs);  // (dql_ensemble_set_team_nstep)
  const auto tm = pw.mem();
  EmuTeamWindow work(E);
  std::vector<Env<T>> envs(E);
  std::vector<TeamRecord> rec(E);  // exactly E records
  emu::for_each_launch(
      j.cfg, j.runs, j.n_runs,
      [&](long long j0, int np, const long long* mgr0, const int* sched) {
        for (size_t l = 0; l < st.n; ++l) {
          if (st.frozen[l]) continue;  // a frozen team's lanes load nothing and store nothing: its windows stay as they are
          work.poison();
          const EmuTeamWindow::View team = work.view(0);
          TeamState ts = team_load(p.sc, p.mem, (long long)l);
          for (size_t k = 0; k < E; ++k) {
            load_env(envs[k], st.sr.data(), st.si[l * E + k], n_envs, (long long)(l * E + k), p.cl);
            team_window_load(tm, n_envs, (long long)(l * E + k), 0, nstep, work.view(k));  // the lane's own column
          }
          const double* qa = j.qa.data() + l * DQL_N_CELLS;
          const double* qb = j.qb.data() + l * DQL_N_CELLS;
          for (int q = 0; q < np && ts.live; ++q) {
            const uint32_t eps_thr = ts.eps_thr;  // one threshold for the period, whatever team_apply_nstep makes of it meanwhile
            for (size_t k = 0; k < E; ++k)
              rec[k] = team_env_period<TICK_PLAIN, X_ONLY>(p.cl, p.lc.cfgk, p.lc.tc, p.mdp, p.k.mdp_run, envs[k], qa, qb, eps_thr, j.seed, (long long)(l * E + k), j0 + q, mgr0[q], sched[q],
                                                           p.lc.kv);
            team_apply_nstep(p.sc, p.mem, p.cl.quirks, p.k.mdp_run.gamma, (long long)l, (const TeamRecord*)rec.data(), (int)E, nstep, team, ts);
          }
          for (size_t k = 0; k < E; ++k) {
            store_env(envs[k], st.sr.data(), st.si.data(), n_envs, (long long)(l * E + k), p.cl);
            team_window_store(tm, n_envs, (long long)(l * E + k), 0, nstep, work.view(k));
          }
          team_store(ts, p.mem, (long long)l);
        }
      },
      [&](int r) { if (r == rearm_after) st.rearm(); });  // dql_ensemble_rearm: the windows are left alone
  return emu::write_result(out_path, st, j, &pw);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: team_nstep_emu JOB OUT\n"); return 2; }
  emu::LearnerJob j(argv[1], 2, [](const emu::LearnerJob& q) {
    return team_size_ok(q.word15) && q.extra[0] >= 1 && q.extra[0] <= NSTEP_MAX && q.extra[1] >= -1 && q.extra[1] < q.n_runs;
  });
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
