// score_emu.cpp — one launch of the scoring kernel k_score, emulated on the CPU from the real device source (dql_score.hpp's score_episodes on
// top of dql_rollout.hpp and dql_device.hpp).
//
// For every env of every table set the driver does what one lane of k_score (dql_greedy.inc) does: the launch's constants as the host side makes
// them (make_simk / make_mdpk / make_rollout_init / fill_schedule over max_steps + 1 periods), the lane's table set, its env id within the set,
// score_episodes<TICK_PLAIN, X_ONLY | X_TWO>; then what the kernel does with the wave's tally: it is added to the table set's row.  A lane runs
// alone: __ballot(p) is p (host_shim.h), so a "wave" is one lane and its tally that lane's own.  Every table read goes through TabRef, which stops
// on an element outside [0, N_CELLS) with exit status 3; the schedule arrays are exactly max_steps + 1 long and the log arrays exactly as long as
// the ABI says, so the sanitized build sees any access beyond them.
//
//   score_emu JOB OUT   run the launch described by JOB (see read_job; tests/test_score_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_score.hpp"

using namespace dql;

namespace {

long long g_env = -1;

struct TabRef {
  const double* p;
  double operator[](long long k) const {
    if (k < 0 || k >= DQL_N_CELLS) { std::fprintf(stderr, "INDEX VIOLATION: acting-table element %lld outside [0, N_CELLS) at log column %lld\n", k, g_env); std::exit(3); }
    return p[k];
  }
};

struct Job {
  int dtype, xmode, n_tables, max_steps, episodes, log;
  long long n;  // envs per table set
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> qa, qb;  // [n_tables][N_CELLS]
};

template <typename V> void read_into(FILE* f, V* p, size_t n) {
  if (n && std::fread(p, sizeof(V), n, f) != n) { std::fprintf(stderr, "short job file\n"); std::exit(2); }
}

Job read_job(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  Job j;
  int32_t hdr[8];  // cfg size, dtype, xmode, n_tables, max_steps, episodes, log (0 / 1), 0
  int64_t ll[2];   // envs per table set, seed
  read_into(f, hdr, 8); read_into(f, ll, 2);
  if (hdr[0] != (int32_t)sizeof(dql_config)) { std::fprintf(stderr, "dql_config size %d != %d\n", hdr[0], (int)sizeof(dql_config)); std::exit(2); }
  read_into(f, &j.cfg, 1);
  j.dtype = hdr[1]; j.xmode = hdr[2]; j.n_tables = hdr[3]; j.max_steps = hdr[4]; j.episodes = hdr[5]; j.log = hdr[6];
  j.n = ll[0]; j.seed = (unsigned long long)ll[1];
  if (j.n < 1 || j.n_tables < 1 || j.n_tables > DQL_SCORE_MAX_TABLES || j.max_steps < 1 || j.max_steps > DQL_SCORE_MAX_STEPS || j.episodes < 1 ||
      j.episodes > DQL_SCORE_MAX_EPISODES) { std::fprintf(stderr, "bad job\n"); std::exit(2); }
  j.qa.resize((size_t)j.n_tables * DQL_N_CELLS); j.qb.resize(j.qa.size());
  read_into(f, j.qa.data(), j.qa.size()); read_into(f, j.qb.data(), j.qb.size());
  std::fclose(f);
  return j;
}

struct Result { std::vector<int64_t> by_code, steps_sum; std::vector<uint8_t> ep_code; std::vector<uint16_t> ep_steps; };

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
  // as dql_score prepares its buffers: sums zeroed, the log "not finished"
  out.by_code.assign((size_t)j.n_tables * SCORE_N_COLS, 0); out.steps_sum.assign((size_t)j.n_tables, 0);
  if (j.log) { out.ep_code.assign((size_t)j.episodes * n_total, 0xff); out.ep_steps.assign((size_t)j.episodes * n_total, 0); }
  const ScoreLog log{j.log ? out.ep_code.data() : nullptr, j.log ? out.ep_steps.data() : nullptr, n_total};
  // k_score, per launch: the x-axis kernels see two_axis as the constant 0; the run-time constants move to VGPRs; the Philox round keys in VGPRs
  SimK<T> cl = c;
  if constexpr (XMODE == X_ONLY) cl.two_axis = 0;
  SimK<T> cfgk = cl;
  if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
  const TickConsts<TICK_PLAIN, T> tc(cfgk);
  uint32_t kv_[20];
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4) {
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)j.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(j.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk;
  for (int k = 0; k < j.n_tables; ++k) {
    const TabRef qa{j.qa.data() + (size_t)k * DQL_N_CELLS}, qb{j.qb.data() + (size_t)k * DQL_N_CELLS};
    for (long long i = 0; i < j.n; ++i) {
      const long long g = (long long)k * j.n + i;
      g_env = g;
      const ScoreTally t = score_episodes<TICK_PLAIN, XMODE>(cl, cfgk, tc, mdp, mdp_run, init, qa, qb, j.seed, (uint32_t)i, j.max_steps, j.episodes, mgr0.data(),
                                                             sched.data(), kv, log, g);
      for (int col = 0; col < SCORE_N_COLS; ++col) out.by_code[(size_t)k * SCORE_N_COLS + col] += t.by_code[col];
      out.steps_sum[(size_t)k] += (int64_t)t.steps;
    }
  }
}

bool dispatch(const Job& j, Result& r) {
  if (j.xmode != (j.cfg.two_axis ? X_TWO : X_ONLY)) return false;  // dql_score picks the instance by the config's axes
  if (j.dtype == DQL_F64) { if (j.xmode == X_TWO) launch<double, X_TWO>(j, r); else launch<double, X_ONLY>(j, r); return true; }
  if (j.xmode == X_TWO) launch<float, X_TWO>(j, r); else launch<float, X_ONLY>(j, r);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: score_emu JOB OUT\n"); return 2; }
  const Job j = read_job(argv[1]);
  Result r;
  if (!dispatch(j, r)) { std::fprintf(stderr, "no such instance: dtype %d xmode %d for two_axis %d\n", j.dtype, j.xmode, j.cfg.two_axis); return 2; }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  std::fwrite(r.by_code.data(), sizeof(int64_t), r.by_code.size(), f);
  std::fwrite(r.steps_sum.data(), sizeof(int64_t), r.steps_sum.size(), f);
  std::fwrite(r.ep_code.data(), sizeof(uint8_t), r.ep_code.size(), f);
  std::fwrite(r.ep_steps.data(), sizeof(uint16_t), r.ep_steps.size(), f);
  return std::fclose(f) == 0 ? 0 : 2;
}
