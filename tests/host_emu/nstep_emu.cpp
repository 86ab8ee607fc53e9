// nstep_emu.cpp — launches of the n-step learner kernel k_learn_nstep, emulated on the CPU from the real device source (dql_nstep.hpp's
// learner_periods_nstep on top of dql_learner.hpp and dql_device.hpp).
//
// For every learner it does what one lane of k_learn_nstep (dql_nstep.inc) does: the launch's constants as the host side makes them, the env state arrays as
// k_init leaves them, the learner's own table slices, learner_periods_nstep<TICK_PLAIN, X_ONLY>.  A lane runs alone: __ballot(p) is p (host_shim.h).  The
// windows are reached through checked references (emu_learners.h): the launch's working copy stands for the kernel's LDS ([NSTEP_MAX][64], the learner in
// column l mod 64), the persistent copy is [NSTEP_MAX][n] plus len[n], exactly as long as the library's; both are poisoned (keys 0xffff, rewards NaN) — the
// working copy before every launch of every lane, as LDS carries nothing from launch to launch — so an entry read before it was written, or kept in the
// working copy only, changes the result.  An index outside them ends the run with status 3.
//
//   nstep_emu JOB OUT   run the launches described by JOB (emu::LearnerJob, word 15: n; tests/test_nstep_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include "emu_learners.h"

using namespace dql;

namespace {

template <typename T> int launch(emu::LearnerJob& j, const char* out_path) {
  const int nstep = j.word15;
  emu::PlainRun<T> p(j);
  emu::PersistentWindows pw((size_t)j.n);  // (dql_ensemble_set_nstep)
  const auto nm = pw.mem();
  emu::WaveWindows lds;
  emu::for_each_launch(j.cfg, j.runs, j.n_runs, [&](long long j0, int np, const long long* mgr0, const int* sched) {
    for (long long l = 0; l < j.n; ++l) {
      lds.poison();
      learner_periods_nstep<TICK_PLAIN, X_ONLY>(p.cl, p.lc.cfgk, p.lc.tc, p.mdp, p.k.mdp_run, p.sc, p.mem, p.st.sr.data(), p.st.si.data(), j.seed, l, true, j0, np, mgr0, sched, p.lc.kv,
                                                nstep, lds.view((int)(l % 64)), nm);
    }
  });
  return emu::write_result(out_path, p.st, j, &pw);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: nstep_emu JOB OUT\n"); return 2; }
  emu::LearnerJob j(argv[1], 0, [](const emu::LearnerJob& q) { return q.word15 >= 1 && q.word15 <= NSTEP_MAX; });
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
