// level0_emu.cpp — the step kernel's level-0 instance and its generic twin, emulated on the CPU from the real device source (dql_device.hpp).
//
// k_step (dql_hip.hip) comes in two forms for the layouts that end their periods on the literal MDP table (TICK_LIT, TICK_PACKED_LITM): the generic body, and
// a level-0 instance that calls agent_period<TICK, XMODE, true>, in which the working level is the compile-time constant 0.  The host picks the level-0
// instance for an x-axis launch at level 0 and never otherwise.  This driver runs ONE launch the way step_emu.cpp does — per env: the clamped acting-table row,
// load_env, P x agent_period, the un-staged accumulation, store_env, every table read and accumulator target index-checked — through either form, chosen
// by the job (header word 7), so that the test can hold the two result files of the same level-0 job against each other byte for byte.  A job whose level
// is not 0 is refused for the level-0 form, as launch_step_t never makes that choice.
//
//   level0_emu JOB OUT          run the launch described by JOB (tests/test_level0_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

constexpr int N_STATES = DQL_N_CELLS / DQL_N_ACTIONS;
template <typename T> SimK<T> x_only_(SimK<T> c) { c.two_axis = 0; return c; }  // k_step's x_only (dql_hip.hip)

struct Where { long long env = -1; int period = -1; };
Where g_where;

[[noreturn]] void violation(const char* what, long long a, long long b = 0) {
  std::fprintf(stderr, "INDEX VIOLATION: %s (%lld, %lld) at env %lld, period %d of the launch\n", what, a, b, g_where.env, g_where.period);
  std::exit(3);
}
void table_violation(long long k) { violation("acting-table element outside [0, N_CELLS)", k); }

struct Job {
  int tick, xmode, mode, n_periods, level0;
  long long n, env_id_offset, step_index;
  double eps;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> reals;  // [NF_REAL][n]
  std::vector<int32_t> ints;  // [NF_INT][n]
  std::vector<double> qa, qb; // acting tables [N_CELLS]
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[8];   // cfg size, dtype (float32 only), tick, xmode, mode, n_periods, 0, level0
  int64_t ll[4];    // n, env_id_offset, step_index, seed
  f.read(hdr, 8); f.read(ll, 4); f.read(&j.eps, 1);
  f.read_config(j.cfg, hdr[0]);
  if (hdr[1] != DQL_F32 || hdr[6] != 0) emu::bad_job();
  j.tick = hdr[2]; j.xmode = hdr[3]; j.mode = hdr[4]; j.n_periods = hdr[5]; j.level0 = hdr[7];
  j.n = ll[0]; j.env_id_offset = ll[1]; j.step_index = ll[2]; j.seed = (unsigned long long)ll[3];
  if (j.n < 1 || j.n_periods < 1 || j.n_periods > DQL_MAX_PERIODS || j.mode == MODE_EXTERNAL) emu::bad_job();
  j.reals.resize((size_t)NF_REAL * j.n); j.ints.resize((size_t)NF_INT * j.n); j.qa.resize(DQL_N_CELLS); j.qb.resize(DQL_N_CELLS);
  f.read(j.reals); f.read(j.ints); f.read(j.qa); f.read(j.qb);
  return j;
}

struct Result {
  std::vector<double> reals; std::vector<int32_t> ints;
  std::vector<unsigned long long> acc;  // [4][N_CELLS]: k_step's global layout
  unsigned long long stats[12] = {};    // decisions, episodes, by_code[9], reward_fx
};

template <int TICK, int XMODE, bool LEVEL0> void launch(const Job& j, Result& out) {
  using T = float;
  const dql_config& cfg = j.cfg;
  const long long n = j.n;
  KalFix kal_fix;
  { const SimK<T> k = make_simk<T>(cfg); kal_fix = KalFix{(double)k.kal_pss, (double)k.kal_kss, true}; }
  const SimK<T> c = make_simk<T>(cfg, &kal_fix);
  if (LEVEL0 && c.working != 0) { std::fprintf(stderr, "the level-0 instance never serves level %d\n", c.working); std::exit(2); }
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  long long mgr0[DQL_MAX_PERIODS]; int sched[DQL_MAX_PERIODS];
  fill_schedule(cfg, j.step_index, mgr0, sched);
  const unsigned eps_thr = eps_threshold(j.eps);
  std::vector<Quad<T>> sr;
  std::vector<int4> si;
  emu::pack_state(j.reals, j.ints, (size_t)n, sr, si);
  const emu::TabRef qa{j.qa.data(), table_violation}, qb{j.qb.data(), table_violation};
  out.acc.assign(4 * (size_t)DQL_N_CELLS, 0ull);
  const emu::Launch<T, TICK> lc(XMODE == X_ONLY ? x_only_(c) : c, j.seed, TICK == TICK_LIT);
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  for (long long i = 0; i < n; ++i) {
    g_where = Where{i, -1};
    const int4 iv = si[i];
    QRow qx = load_qrow(qa, qb, (unsigned)iv.x < (unsigned)N_STATES ? iv.x : 0);
    Env<T> e;
    load_env(e, sr.data(), iv, n, i, XMODE == X_ONLY ? x_only_(c) : c);
    for (int p = 0; p < j.n_periods; ++p) {
      g_where = Where{i, p};
      const int prev_idx = e.idx_x, prev_idy = e.idx_y;
      const StepOut o = agent_period<TICK, XMODE, LEVEL0>(lc.cfgk, lc.tc, mdp, mdp_run, e, qx, qa, qb, j.mode, eps_thr, 2, j.seed, (uint32_t)(j.env_id_offset + i),
                                                          j.step_index + p, mgr0[p], sched[p], lc.kv);
      const int ax = e.action & 3, ay = (e.action >> 2) & 3;
      const struct { int cell; long long target; int prev, act; const char* what; } tgt[2] = {
          {o.cell, o.target_fx, prev_idx, ax, "cell"}, {o.cell_y, o.target_y_fx, prev_idy, ay, "cell_y"}};
      for (const auto& t : tgt) {
        if (t.cell < 0) continue;
        if (t.cell >= 2 * DQL_N_CELLS) violation(t.what, t.cell, 2 * DQL_N_CELLS);
        if (t.prev < 0 || t.prev >= N_STATES) violation(t.what, t.cell, t.prev);
        if (t.cell % DQL_N_CELLS != t.prev * 3 + t.act) violation(t.what, t.cell, (long long)t.prev * 3 + t.act);
        const int g = t.cell + (t.cell >= DQL_N_CELLS ? DQL_N_CELLS : 0);
        out.acc[g] += (unsigned long long)t.target;
        out.acc[DQL_N_CELLS + g] += 1ull;
      }
      qx = o.next;
      out.stats[0] += (unsigned long long)o.decision;
      out.stats[11] += (unsigned long long)o.reward_fx;
      if (o.done) { out.stats[1] += 1; if (e.code >= 0 && e.code <= DQL_TERMINAL_TIMEOUT) out.stats[2 + e.code] += 1; else violation("terminal code", e.code); }
    }
    store_env(e, sr.data(), si.data(), n, i, XMODE == X_ONLY ? x_only_(c) : c);
  }
  emu::unpack_state(sr.data(), si.data(), (size_t)n, out.reals, out.ints);
}

template <int TICK, int XMODE> void by_level(const Job& j, Result& r) {
  if (j.level0) launch<TICK, XMODE, true>(j, r); else launch<TICK, XMODE, false>(j, r);
}
// the level-0 forms: TICK_LIT and TICK_PACKED_LITM for x-axis configs — the ones launch_step_t selects — and TICK_LIT / X_TWO, which the library does not
// compile (its 512-thread instance sent wrong targets to the tables on the GPU): here its source is held to the generic form and the oracle all the same
bool dispatch(const Job& j, Result& r) {
  if (j.tick == TICK_LIT && j.xmode == X_ONLY) { by_level<TICK_LIT, X_ONLY>(j, r); return true; }
  if (j.tick == TICK_LIT && j.xmode == X_TWO) { by_level<TICK_LIT, X_TWO>(j, r); return true; }
  if (j.tick == TICK_PACKED_LITM && j.xmode == X_ONLY) { by_level<TICK_PACKED_LITM, X_ONLY>(j, r); return true; }
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: level0_emu JOB OUT\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (!dispatch(j, r)) { std::fprintf(stderr, "no level-0 form of this instance: tick %d xmode %d\n", j.tick, j.xmode); return 2; }
  emu::ResultFile f(argv[2]);
  f.put(r.reals); f.put(r.ints); f.put(r.acc); f.put(r.stats, 12);
  return f.close();
}
