// step_emu.cpp — one launch of the step kernel k_step, emulated on the CPU from the real device source (dql_device.hpp).
//
// For every env the driver does what one lane of k_step (dql_hip.hip) does in one launch: the packed ints and the clamped acting-table
// row first, load_env, P x agent_period<TICK, XMODE> with the launch's schedule, eps threshold, seed, env id and step index, the
// un-staged accumulation into the int64 [4][N_CELLS] accumulators (the one-wave-per-workgroup path), store_env.  The acting tables stay
// constant over the launch, as they do on the device.  A lane runs alone: __ballot(p) is p (host_shim.h).
//
// Index checks: every table read the device code makes goes through TabRef, which stops on an element outside [0, N_CELLS); every
// accumulator target is checked to lie in [0, 2 N_CELLS) AND to be the cell of the row the env left with the action it took, in the
// table its coin picked.  A violation stops the run with exit status 3 and names the env, the period and the state.
//
// The job and result files, the launch prologue, the state packing and the checked table are emu_common.h's, shared with the other four drivers.
//
//   step_emu JOB OUT     run the launch described by JOB (see read_job; tests/test_step_host_emulation.py writes it), write OUT
//   step_emu --admits JOB      print refm and lit_ok of JOB's config: may TICK_PACKED_LITM / TICK_LIT serve it (create_impl)
//   step_emu --asan-selftest   read one element past a heap array (the sanitized build must report it)
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

constexpr int N_STATES = DQL_N_CELLS / DQL_N_ACTIONS;
template <typename T> SimK<T> x_only_(SimK<T> c) { c.two_axis = 0; return c; }  // k_step's x_only (dql_hip.hip)

struct Where { long long env = -1; int period = -1; int idx_x = 0, idx_y = 0, flags = 0, step_count = 0; };
Where g_where;

[[noreturn]] void violation(const char* what, long long a, long long b = 0) {
  std::fprintf(stderr, "INDEX VIOLATION: %s (%lld, %lld) at env %lld, period %d of the launch; state before the period: idx_x %d idx_y %d flags %d step_count %d\n",
               what, a, b, g_where.env, g_where.period, g_where.idx_x, g_where.idx_y, g_where.flags, g_where.step_count);
  std::exit(3);
}

void table_violation(long long k) { violation("acting-table element outside [0, N_CELLS)", k); }

struct Job {
  int dtype, tick, xmode, mode, n_periods;
  long long n, env_id_offset, step_index;
  double eps;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> reals;  // [NF_REAL][n], dql_get_sim_state's layout
  std::vector<int32_t> ints;  // [NF_INT][n], dql_get_sim_ints'
  std::vector<double> qa, qb; // acting tables [N_CELLS]
  std::vector<uint8_t> actions;
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[8];   // cfg size, dtype, tick, xmode, mode, n_periods, have_actions, 0
  int64_t ll[4];    // n, env_id_offset, step_index, seed
  f.read(hdr, 8); f.read(ll, 4); f.read(&j.eps, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.tick = hdr[2]; j.xmode = hdr[3]; j.mode = hdr[4]; j.n_periods = hdr[5];
  j.n = ll[0]; j.env_id_offset = ll[1]; j.step_index = ll[2]; j.seed = (unsigned long long)ll[3];
  if (j.n < 1 || j.n_periods < 1 || j.n_periods > DQL_MAX_PERIODS) emu::bad_job();
  j.reals.resize((size_t)NF_REAL * j.n); j.ints.resize((size_t)NF_INT * j.n); j.qa.resize(DQL_N_CELLS); j.qb.resize(DQL_N_CELLS);
  f.read(j.reals); f.read(j.ints); f.read(j.qa); f.read(j.qb);
  if (hdr[6]) { j.actions.resize((size_t)j.n); f.read(j.actions); }
  return j;
}

// what the launch leaves behind, in the oracle's formats
struct Result {
  std::vector<double> reals; std::vector<int32_t> ints;
  std::vector<unsigned long long> acc;  // [4][N_CELLS]: table a's {target sums, visits}, then table b's (k_step's global layout)
  unsigned long long stats[12] = {};    // decisions, episodes, by_code[9], reward_fx (Oracle.stats)
  unsigned long long bad_actions = 0;
};

template <typename T, int TICK, int XMODE> void launch(const Job& j, Result& out) {
  const dql_config& cfg = j.cfg;
  const long long n = j.n;
  // create_impl: the Kalman fixed point once per context; make_step_args: the launch's constants
  KalFix kal_fix;
  { const SimK<T> k = make_simk<T>(cfg); kal_fix = KalFix{(double)k.kal_pss, (double)k.kal_kss, true}; }
  const SimK<T> c = make_simk<T>(cfg, &kal_fix);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  long long mgr0[DQL_MAX_PERIODS]; int sched[DQL_MAX_PERIODS];
  fill_schedule(cfg, j.step_index, mgr0, sched);
  const unsigned eps_thr = eps_threshold(j.eps);
  // HBM images of the state (dql_set_sim_state / dql_set_sim_ints)
  std::vector<Quad<T>> sr;
  std::vector<int4> si;
  emu::pack_state(j.reals, j.ints, (size_t)n, sr, si);
  const emu::TabRef qa{j.qa.data(), table_violation}, qb{j.qb.data(), table_violation};
  out.acc.assign(4 * (size_t)DQL_N_CELLS, 0ull);
  // k_step, per launch (emu::Launch): the x-axis kernels see two_axis as the constant 0; the run-time constants move to VGPRs (BLOCK < 512: the
  // instances this driver stands for); the tick constants in the layout's form; the Philox round keys in VGPRs only for TICK_LIT / TICK_PLAIN
  const emu::Launch<T, TICK> lc(XMODE == X_ONLY ? x_only_(c) : c, j.seed, sizeof(T) == 4 && (TICK == TICK_LIT || TICK == TICK_PLAIN));
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  for (long long i = 0; i < n; ++i) {
    g_where = Where{i, -1, 0, 0, 0, 0};
    const int4 iv = si[i];
    QRow qx = load_qrow(qa, qb, (unsigned)iv.x < (unsigned)(DQL_N_CELLS / DQL_N_ACTIONS) ? iv.x : 0);
    Env<T> e;
    load_env(e, sr.data(), iv, n, i, XMODE == X_ONLY ? x_only_(c) : c);
    for (int p = 0; p < j.n_periods; ++p) {
      g_where = Where{i, p, e.idx_x, e.idx_y, e.flags, e.step_count};
      const int ext = (j.mode == MODE_EXTERNAL) ? (int)j.actions[i] : 2;
      if (j.mode == MODE_EXTERNAL) {
        const int ax = ext & 3, ay = (ext >> 2) & 3;
        if (ax > 2 || ay > 2 || (ext >> 4) || (!c.two_axis && ay != 0 && ay != 2)) out.bad_actions += 1;
      }
      const int prev_idx = e.idx_x, prev_idy = e.idx_y;
      const StepOut o = agent_period<TICK, XMODE>(lc.cfgk, lc.tc, mdp, mdp_run, e, qx, qa, qb, j.mode, eps_thr, ext, j.seed, (uint32_t)(j.env_id_offset + i),
                                                  j.step_index + p, mgr0[p], sched[p], lc.kv);
      // the accumulator targets: inside [0, 2 N_CELLS), and the cell of the row the env left with the action it took
      const int ax = e.action & 3, ay = (e.action >> 2) & 3;
      const struct { int cell; long long target; int prev, act; const char* what; } tgt[2] = {
          {o.cell, o.target_fx, prev_idx, ax, "cell"}, {o.cell_y, o.target_y_fx, prev_idy, ay, "cell_y"}};
      for (const auto& t : tgt) {
        if (t.cell < 0) continue;
        if (t.cell >= 2 * DQL_N_CELLS) violation(t.what, t.cell, 2 * DQL_N_CELLS);
        if (t.prev < 0 || t.prev >= N_STATES) violation(t.what, t.cell, t.prev);
        if (t.cell % DQL_N_CELLS != t.prev * 3 + t.act) violation(t.what, t.cell, (long long)t.prev * 3 + t.act);
        const int g = t.cell + (t.cell >= DQL_N_CELLS ? DQL_N_CELLS : 0);  // k_step's global layout [4][N_CELLS]
        out.acc[g] += (unsigned long long)t.target;
        out.acc[DQL_N_CELLS + g] += 1ull;
      }
      if (o.cell_y >= 0 && o.cell < 0) violation("cell_y without cell", o.cell_y, o.cell);
      qx = o.next;
      out.stats[0] += (unsigned long long)o.decision;
      out.stats[11] += (unsigned long long)o.reward_fx;
      if (o.done) { out.stats[1] += 1; if (e.code >= 0 && e.code <= DQL_TERMINAL_TIMEOUT) out.stats[2 + e.code] += 1; else violation("terminal code", e.code); }
    }
    store_env(e, sr.data(), si.data(), n, i, XMODE == X_ONLY ? x_only_(c) : c);
  }
  emu::unpack_state(sr.data(), si.data(), (size_t)n, out.reals, out.ints);
}

template <typename T, int TICK> bool dispatch_x(const Job& j, Result& r) {
  switch (j.xmode) {
    case X_TWO: launch<T, TICK, X_TWO>(j, r); return true;
    case X_ONLY: launch<T, TICK, X_ONLY>(j, r); return true;
    case X_RUNTIME: launch<T, TICK, X_RUNTIME>(j, r); return true;
  }
  return false;
}

bool dispatch(const Job& j, Result& r) {
  if (j.dtype == DQL_F64) return j.tick == TICK_PLAIN && dispatch_x<double, TICK_PLAIN>(j, r);
  switch (j.tick) {
    case TICK_PLAIN: return dispatch_x<float, TICK_PLAIN>(j, r);
    case TICK_PACKED: return dispatch_x<float, TICK_PACKED>(j, r);
    case TICK_LIT: return dispatch_x<float, TICK_LIT>(j, r);
    case TICK_PACKED_LITM: return dispatch_x<float, TICK_PACKED_LITM>(j, r);
  }
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string_view(argv[1]) == "--asan-selftest") {
    std::vector<int>* v = new std::vector<int>(8, 1);
    volatile const int* p = v->data();
    const int past = p[8];  // one past the end of a heap array
    std::printf("read %d\n", past);
    delete v;
    return 0;
  }
  if (argc == 3 && std::string_view(argv[1]) == "--admits") {  // may the literal-table instances serve this config?  (create_impl: refm, lit_ok)
    const Job j = read_job(argv[2]);
    const bool refm = refm_matches(make_mdpk<float>(j.cfg));
    KalFix kf;
    { const SimK<float> k = make_simk<float>(j.cfg); kf = KalFix{(double)k.kal_pss, (double)k.kal_kss, true}; }
    std::printf("%d %d\n", refm ? 1 : 0, (refm && refk_matches(make_simk<float>(j.cfg, &kf))) ? 1 : 0);
    return 0;
  }
  if (argc != 3) { std::fprintf(stderr, "usage: step_emu JOB OUT | --admits JOB | --asan-selftest\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (!dispatch(j, r)) { std::fprintf(stderr, "no such instance: dtype %d tick %d xmode %d\n", j.dtype, j.tick, j.xmode); return 2; }
  emu::ResultFile f(argv[2]);
  f.put(r.reals); f.put(r.ints); f.put(r.acc); f.put(r.stats, 12); f.put(&r.bad_actions, 1);
  return f.close();
}
