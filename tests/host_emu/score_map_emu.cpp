// score_map_emu.cpp — one launch of the mapping scorer k_score_map, emulated on the CPU from the real device source (dql_score_map.hpp's score_map_episodes
// on top of dql_score.hpp, dql_rollout.hpp and dql_device.hpp).
//
// For every env of every table set the driver does what one lane of k_score_map (dql_score_map.inc) does: the launch's constants as the host side makes them,
// the lane's table set, its env id within the set, the wave's histogram cleared, score_map_episodes<TICK_PLAIN, X_ONLY | X_TWO>; then what the kernel does at
// the end: the non-zero cells of the histogram and the wave's tally are added to the table set's rows.  A lane runs alone: __ballot(p) is p (host_shim.h), so
// a "wave" is one lane, its histogram that lane's own, and the flush's sweeps are a plain loop over the cells — what depends on 64 lanes sharing one
// histogram (the LDS atomics, the partial last sweep) shows on the GPU only.  The histogram here is exactly DQL_N_CELLS long and its add() stops on a cell
// outside it with exit status 3; every table read goes through TabRef; the schedule arrays are exactly max_steps + 1 long and the log arrays exactly as long
// as the ABI says, so the sanitized build sees any access beyond them.
//
//   score_map_emu JOB OUT   run the launch described by JOB (see read_job; tests/test_score_map_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_score.hpp"
#include "dql_score_map.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

long long g_env = -1;

void table_violation(long long k) { emu::index_violation(k, "log column", g_env); }

struct Job {
  int dtype, xmode, n_tables, max_steps, episodes, log;
  long long n;  // envs per table set
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> qa, qb;  // [n_tables][N_CELLS]
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[8];  // cfg size, dtype, xmode, n_tables, max_steps, episodes, log (0 / 1), 0
  int64_t ll[2];   // envs per table set, seed
  f.read(hdr, 8); f.read(ll, 2);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.xmode = hdr[2]; j.n_tables = hdr[3]; j.max_steps = hdr[4]; j.episodes = hdr[5]; j.log = hdr[6];
  j.n = ll[0]; j.seed = (unsigned long long)ll[1];
  if (j.n < 1 || j.n_tables < 1 || j.n_tables > DQL_SCORE_MAP_MAX_TABLES || j.max_steps < 1 || j.max_steps > DQL_SCORE_MAX_STEPS || j.episodes < 1 ||
      j.episodes > DQL_SCORE_MAX_EPISODES) emu::bad_job();
  j.qa.resize((size_t)j.n_tables * DQL_N_CELLS); j.qb.resize(j.qa.size());
  f.read(j.qa); f.read(j.qb);
  return j;
}

struct Result {
  std::vector<int64_t> by_code, steps_sum, visits, faults;
  std::vector<uint8_t> ep_code;
  std::vector<uint16_t> ep_steps, ep_last_cell;
};

// the wave's histogram: k_score_map's LDS array, its add an ordinary increment (one lane)
struct HostHist {
  std::vector<unsigned> h;
  HostHist() : h((size_t)DQL_N_CELLS, 0u) {}
  void clear() { h.assign((size_t)DQL_N_CELLS, 0u); }
  void add(int cell) {
    if (cell < 0 || cell >= DQL_N_CELLS) { std::fprintf(stderr, "INDEX VIOLATION: histogram cell %d outside [0, N_CELLS) at env %lld\n", cell, g_env); std::exit(3); }
    ++h[(size_t)cell];
  }
};

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
  // as dql_score_map prepares its buffers: sums and map zeroed, the log "not finished"
  out.by_code.assign((size_t)j.n_tables * SCORE_N_COLS, 0); out.steps_sum.assign((size_t)j.n_tables, 0);
  out.visits.assign((size_t)j.n_tables * DQL_N_CELLS, 0); out.faults.assign(1, 0);
  if (j.log) {
    out.ep_code.assign((size_t)j.episodes * n_total, 0xff); out.ep_steps.assign((size_t)j.episodes * n_total, 0);
    out.ep_last_cell.assign((size_t)2 * j.episodes * n_total, SCORE_MAP_NO_CELL);
  }
  const ScoreMapLog log{j.log ? out.ep_code.data() : nullptr, j.log ? out.ep_steps.data() : nullptr, j.log ? out.ep_last_cell.data() : nullptr, n_total, j.episodes};
  SimK<T> cl = c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  HostHist hist;
  for (int k = 0; k < j.n_tables; ++k) {
    const emu::TabRef qa{j.qa.data() + (size_t)k * DQL_N_CELLS, table_violation}, qb{j.qb.data() + (size_t)k * DQL_N_CELLS, table_violation};
    for (long long i = 0; i < j.n; ++i) {
      const long long g = (long long)k * j.n + i;
      g_env = g;
      hist.clear();
      const ScoreMapTally r = score_map_episodes<TICK_PLAIN, XMODE>(cl, lc.cfgk, lc.tc, mdp, mdp_run, init, qa, qb, j.seed, (uint32_t)i, j.max_steps, j.episodes, mgr0.data(),
                                                                    sched.data(), lc.kv, log, g, hist);
      for (int cell = 0; cell < DQL_N_CELLS; ++cell)
        if (hist.h[(size_t)cell]) out.visits[(size_t)k * DQL_N_CELLS + cell] += hist.h[(size_t)cell];
      out.faults[0] += r.faults;
      for (int col = 0; col < SCORE_N_COLS; ++col) out.by_code[(size_t)k * SCORE_N_COLS + col] += r.t.by_code[col];
      out.steps_sum[(size_t)k] += (int64_t)r.t.steps;
    }
  }
}

bool dispatch(const Job& j, Result& r) {
  if (j.xmode != (j.cfg.two_axis ? X_TWO : X_ONLY)) return false;  // dql_score_map picks the instance by the config's axes
  if (j.dtype == DQL_F64) { if (j.xmode == X_TWO) launch<double, X_TWO>(j, r); else launch<double, X_ONLY>(j, r); return true; }
  if (j.xmode == X_TWO) launch<float, X_TWO>(j, r); else launch<float, X_ONLY>(j, r);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: score_map_emu JOB OUT\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (!dispatch(j, r)) { std::fprintf(stderr, "no such instance: dtype %d xmode %d for two_axis %d\n", j.dtype, j.xmode, j.cfg.two_axis); return 2; }
  emu::ResultFile f(argv[2]);
  f.put(r.by_code); f.put(r.steps_sum); f.put(r.visits); f.put(r.faults); f.put(r.ep_code); f.put(r.ep_steps); f.put(r.ep_last_cell);
  return f.close();
}
