// rollout_emu.cpp — one launch of the roll-out kernel k_rollout, emulated on the CPU from the real device source (dql_rollout.hpp's
// rollout_episode on top of dql_device.hpp).
//
// For every env of every table set the driver does what one lane of k_rollout (dql_greedy.inc) does: the launch's constants as the host side
// makes them (make_simk / make_mdpk / make_rollout_init / fill_schedule over max_steps + 1 periods), the lane's table set, its env id within
// the set, rollout_episode<TICK_PLAIN, X_ONLY | X_TWO>.  A lane runs alone: __ballot(p) is p (host_shim.h).  Every table read goes through
// TabRef, which stops on an element outside [0, N_CELLS) with exit status 3; the schedule arrays are exactly max_steps + 1 long and the
// output arrays exactly as long as the ABI says, so the sanitized build sees any access beyond them.  The job and result files, the launch prologue
// (emu::Launch) and TabRef are emu_common.h's, shared with the other four drivers.
//
//   rollout_emu JOB OUT   run the launch described by JOB (see read_job; tests/test_rollout_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

long long g_env = -1;

void table_violation(long long k) { emu::index_violation(k, "output column", g_env); }

struct Job {
  int dtype, xmode, n_tables, max_steps, trace_envs;
  long long n;  // envs per table set
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> qa, qb;  // [n_tables][N_CELLS]
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[8];  // cfg size, dtype, xmode, n_tables, max_steps, trace_envs, 0, 0
  int64_t ll[2];   // envs per table set, seed
  f.read(hdr, 8); f.read(ll, 2);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.xmode = hdr[2]; j.n_tables = hdr[3]; j.max_steps = hdr[4]; j.trace_envs = hdr[5];
  j.n = ll[0]; j.seed = (unsigned long long)ll[1];
  if (j.n < 1 || j.n_tables < 1 || j.n_tables > DQL_ROLLOUT_MAX_TABLES || j.max_steps < 1 || j.max_steps > DQL_ROLLOUT_MAX_STEPS || j.trace_envs < 0 || j.trace_envs > 64 ||
      j.trace_envs > j.n) emu::bad_job();
  j.qa.resize((size_t)j.n_tables * DQL_N_CELLS); j.qb.resize(j.qa.size());
  f.read(j.qa); f.read(j.qb);
  return j;
}

struct Result { std::vector<int32_t> code, steps; std::vector<double> rec, trace; };

template <typename T, int XMODE> void launch(const Job& j, Result& out) {
  const dql_config& cfg = j.cfg;
  const SimK<T> c = make_simk<T>(cfg);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  std::vector<long long> mgr0((size_t)j.max_steps + 1);
  std::vector<int> sched((size_t)j.max_steps + 1);
  fill_schedule(cfg, 0, mgr0.data(), sched.data(), j.max_steps + 1);
  const long long n_total = (long long)j.n_tables * j.n;
  out.code.assign((size_t)n_total, -2); out.steps.assign((size_t)n_total, -2);
  out.rec.assign((size_t)RO_N_RECORD * n_total, std::numeric_limits<double>::quiet_NaN());
  out.trace.assign((size_t)(j.max_steps + 1) * RO_N_TRACE * j.trace_envs, std::numeric_limits<double>::quiet_NaN());
  const RolloutOut ro{out.code.data(), out.steps.data(), out.rec.data(), j.trace_envs ? out.trace.data() : nullptr, n_total, j.trace_envs};
  // k_rollout, per launch: the x-axis kernels see two_axis as the constant 0; the run-time constants move to VGPRs; the Philox round keys in VGPRs
  SimK<T> cl = c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  for (int k = 0; k < j.n_tables; ++k) {
    const emu::TabRef qa{j.qa.data() + (size_t)k * DQL_N_CELLS, table_violation}, qb{j.qb.data() + (size_t)k * DQL_N_CELLS, table_violation};
    for (long long i = 0; i < j.n; ++i) {
      const long long g = (long long)k * j.n + i;
      g_env = g;
      const bool first_wave = k == 0 && i < 64;
      rollout_episode<TICK_PLAIN, XMODE>(cl, lc.cfgk, lc.tc, mdp, mdp_run, init, qa, qb, j.seed, (uint32_t)i, j.max_steps, mgr0.data(), sched.data(), lc.kv, ro, g,
                                         first_wave && j.trace_envs > 0, first_wave && i < j.trace_envs);
    }
  }
}

bool dispatch(const Job& j, Result& r) {
  if (j.xmode != (j.cfg.two_axis ? X_TWO : X_ONLY)) return false;  // dql_rollout picks the instance by the config's axes
  if (j.dtype == DQL_F64) { if (j.xmode == X_TWO) launch<double, X_TWO>(j, r); else launch<double, X_ONLY>(j, r); return true; }
  if (j.xmode == X_TWO) launch<float, X_TWO>(j, r); else launch<float, X_ONLY>(j, r);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: rollout_emu JOB OUT\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (!dispatch(j, r)) { std::fprintf(stderr, "no such instance: dtype %d xmode %d for two_axis %d\n", j.dtype, j.xmode, j.cfg.two_axis); return 2; }
  emu::ResultFile f(argv[2]);
  f.put(r.code); f.put(r.steps); f.put(r.rec); f.put(r.trace);
  return f.close();
}
