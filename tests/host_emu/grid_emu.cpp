// grid_emu.cpp — one launch of the scenario-grid scoring kernel k_score_grid, emulated on the CPU from the real device source (dql_score_grid.hpp's
// grid_coords, touch_bin and score_grid_episodes on top of dql_score.hpp, dql_rollout.hpp and dql_device.hpp).
//
// The driver walks every BLOCK of the launch, as the hardware does: grid_coords tells it which scenario, table set and envs the block serves, and for each of
// the block's 64 lanes it does what one lane of k_score_grid (dql_score_grid.inc) does — the scenario's record of constants (make_simk / make_mdpk /
// make_rollout_init / make_touch_edges, as dql_score_grid's host side fills it) picked by the block's scenario index, the lane's table set, its env id,
// score_grid_episodes<TICK_PLAIN, X_ONLY | X_TWO> — then what the kernel does with the wave's tally: it is added to row (scenario, set).  A lane runs alone:
// __ballot(p) is p (host_shim.h), so a "wave" is one lane and its tally that lane's own.  Every table read goes through TabRef; the schedule arrays, the
// records, the rows and the log are exactly as long as the ABI says, so the sanitized build sees any access beyond them.
//
//   grid_emu JOB OUT   run the launch described by JOB (see read_job; tests/test_score_grid_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_score.hpp"
#include "dql_score_grid.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

long long g_env = -1;

void table_violation(long long k) { emu::index_violation(k, "lane", g_env); }

struct Job {
  int dtype, xmode, n_tables, max_steps, episodes, log, touch, n_scenarios;
  long long n;  // envs per table set
  unsigned long long seed;
  std::vector<dql_config> cfgs;
  std::vector<double> qa, qb;  // [n_tables][N_CELLS]
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[8];  // cfg size, dtype, xmode, n_tables, max_steps, episodes, flags (1: log, 2: touch_hist), n_scenarios
  int64_t ll[2];   // envs per table set, seed
  f.read(hdr, 8); f.read(ll, 2);
  j.dtype = hdr[1]; j.xmode = hdr[2]; j.n_tables = hdr[3]; j.max_steps = hdr[4]; j.episodes = hdr[5]; j.log = hdr[6] & 1; j.touch = (hdr[6] >> 1) & 1; j.n_scenarios = hdr[7];
  j.n = ll[0]; j.seed = (unsigned long long)ll[1];
  if (j.n < 64 || j.n % 64 || j.n_tables < 1 || j.n_tables > DQL_SCORE_MAX_TABLES || j.max_steps < 1 || j.max_steps > DQL_SCORE_MAX_STEPS || j.episodes < 1 ||
      j.episodes > DQL_SCORE_MAX_EPISODES || j.n_scenarios < 1 || j.n_scenarios > DQL_GRID_MAX_SCENARIOS || (long long)j.n_scenarios * j.n_tables * j.n > (1ll << 30))
    emu::bad_job();
  j.cfgs.resize((size_t)j.n_scenarios);
  for (dql_config& c : j.cfgs) f.read_config(c, hdr[0]);
  j.qa.resize((size_t)j.n_tables * DQL_N_CELLS); j.qb.resize(j.qa.size());
  f.read(j.qa); f.read(j.qb);
  return j;
}

struct Result { std::vector<int64_t> by_code, steps_sum, touch; std::vector<uint8_t> ep_code; std::vector<uint16_t> ep_steps; };

template <typename T, int XMODE> void launch(const Job& j, Result& out) {
  const int S = j.n_scenarios, K = j.n_tables, B = (int)(j.n / 64);
  // as dql_score_grid's host side: one record and one MdpK per scenario, the schedule of scenario 0 (the scenarios share what fixes it)
  std::vector<GridScenario<T>> sc((size_t)S);
  std::vector<MdpK<T>> mk((size_t)S);
  for (int s = 0; s < S; ++s) {
    const dql_config& c = j.cfgs[(size_t)s];
    sc[(size_t)s].c = make_simk<T>(c);
    sc[(size_t)s].mr = MdpRun<T>{c.gamma, (T)(c.t_max * c.f_ag), c.goal_logic};
    sc[(size_t)s].init = make_rollout_init<T>(c);
    make_touch_edges<T>(c, sc[(size_t)s].touch_edges);
    mk[(size_t)s] = make_mdpk<T>(c);
  }
  std::vector<long long> mgr0((size_t)j.max_steps + 1);
  std::vector<int> sched((size_t)j.max_steps + 1);
  fill_schedule(j.cfgs[0], 0, mgr0.data(), sched.data(), j.max_steps + 1);
  const long long n_total = (long long)K * j.n;  // per scenario
  const size_t rows = (size_t)S * (size_t)K;
  // as dql_score_grid prepares its buffers: sums zeroed, the log "not finished"
  out.by_code.assign(rows * SCORE_N_COLS, 0); out.steps_sum.assign(rows, 0); out.touch.assign(rows * GRID_TOUCH_BINS, 0);
  const size_t log_n = (size_t)S * (size_t)j.episodes * (size_t)n_total;
  if (j.log) { out.ep_code.assign(log_n, 0xff); out.ep_steps.assign(log_n, 0); }
  const unsigned n_blocks = (unsigned)S * (unsigned)K * (unsigned)B;
  for (unsigned b = 0; b < n_blocks; ++b) {
    // k_score_grid, per wave
    const GridCoords gc = grid_coords(b, (unsigned)B, (unsigned)K);
    if (gc.s >= S) continue;
    if (gc.s < 0 || gc.k < 0 || gc.k >= K || gc.env0 < 0 || gc.env0 + 64 > j.n) { std::fprintf(stderr, "INDEX VIOLATION: block %u -> scenario %d set %d env0 %d\n", b, gc.s, gc.k, gc.env0); std::exit(3); }
    const GridScenario<T> rec = sc[(size_t)gc.s];
    SimK<T> cl = rec.c;
    if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
    const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
    const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mk[(size_t)gc.s];
    const emu::TabRef qa{j.qa.data() + (size_t)gc.k * DQL_N_CELLS, table_violation}, qb{j.qb.data() + (size_t)gc.k * DQL_N_CELLS, table_violation};
    const size_t log_off = (size_t)gc.s * (size_t)j.episodes * (size_t)n_total;
    const ScoreLog log{j.log ? out.ep_code.data() + log_off : nullptr, j.log ? out.ep_steps.data() + log_off : nullptr, n_total};
    const size_t row_i = (size_t)gc.s * (size_t)K + (size_t)gc.k;
    for (int lane = 0; lane < 64; ++lane) {
      const int i = gc.env0 + lane;
      const long long g = ((long long)gc.k * B) * 64 + i;
      g_env = (long long)b * 64 + lane;
      const GridTally r = score_grid_episodes<TICK_PLAIN, XMODE>(cl, lc.cfgk, lc.tc, mdp, rec.mr, rec.init, rec.touch_edges, qa, qb, j.seed, (uint32_t)i, j.max_steps, j.episodes,
                                                                 mgr0.data(), sched.data(), lc.kv, log, g);
      for (int col = 0; col < SCORE_N_COLS; ++col) out.by_code[row_i * SCORE_N_COLS + col] += r.t.by_code[col];
      out.steps_sum[row_i] += (int64_t)r.t.steps;
      for (int q = 0; q < GRID_TOUCH_BINS; ++q) out.touch[row_i * GRID_TOUCH_BINS + q] += r.touch[q];
    }
  }
  if (!j.touch) out.touch.clear();  // a caller without touch_hist receives none
}

bool dispatch(const Job& j, Result& r) {
  for (const dql_config& c : j.cfgs)  // dql_score_grid picks the instance by scenario 0 and refuses a scenario that differs in dtype or axes
    if (j.xmode != (c.two_axis ? X_TWO : X_ONLY) || j.dtype != c.dtype) return false;
  if (j.dtype == DQL_F64) { if (j.xmode == X_TWO) launch<double, X_TWO>(j, r); else launch<double, X_ONLY>(j, r); return true; }
  if (j.xmode == X_TWO) launch<float, X_TWO>(j, r); else launch<float, X_ONLY>(j, r);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: grid_emu JOB OUT\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (!dispatch(j, r)) { std::fprintf(stderr, "no such instance: dtype %d xmode %d for these scenarios\n", j.dtype, j.xmode); return 2; }
  emu::ResultFile f(argv[2]);
  f.put(r.by_code); f.put(r.steps_sum); f.put(r.touch); f.put(r.ep_code); f.put(r.ep_steps);
  return f.close();
}
