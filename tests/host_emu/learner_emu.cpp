// learner_emu.cpp — launches of the sequential-learner kernel k_learn, emulated on the CPU from the real device source (dql_learner.hpp's
// learner_periods on top of dql_device.hpp).
//
// For every learner the driver does what one lane of k_learn (dql_ensemble.inc) does: the launch's constants as the host side makes them (make_simk /
// make_mdpk / fill_schedule from the ensemble's period index), the env state arrays initialised as k_init initialises them, the learner's own table
// slices, learner_periods<TICK_PLAIN, X_ONLY>.  A lane runs alone: __ballot(p) is p (host_shim.h).  The job lists the lengths of the consecutive runs
// (launches); state, tables and counters live in arrays exactly as long as the ABI says, so the sanitized build sees any access beyond them.  The job, those
// arrays, the constants and the loop over the launches are emu_learners.h's; what stands here is the lane.
//
//   learner_emu JOB OUT   run the launches described by JOB (emu::LearnerJob; tests/test_learner_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include "emu_learners.h"

using namespace dql;

namespace {

template <typename T> int launch(emu::LearnerJob& j, const char* out_path) {
  emu::PlainRun<T> p(j);
  emu::for_each_launch(j.cfg, j.runs, j.n_runs, [&](long long j0, int np, const long long* mgr0, const int* sched) {
    for (long long l = 0; l < j.n; ++l)
      learner_periods<TICK_PLAIN, X_ONLY>(p.cl, p.lc.cfgk, p.lc.tc, p.mdp, p.k.mdp_run, p.sc, p.mem, p.st.sr.data(), p.st.si.data(), j.seed, l, true, j0, np, mgr0, sched, p.lc.kv);
  });
  return emu::write_result(out_path, p.st, j);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: learner_emu JOB OUT\n"); return 2; }
  emu::LearnerJob j(argv[1], 0, [](const emu::LearnerJob&) { return true; });  // (word 15 is 0)
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
