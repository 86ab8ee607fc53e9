// refined_emu.cpp — launches of the refined-state kernels k_learn_refined and k_score_refined, emulated on the CPU from the real device source
// (dql_refined.hpp's refined_learner_periods and score_refined_episodes on top of dql_learner.hpp, dql_score.hpp, dql_model_split.hpp and dql_device.hpp).
//
// Mode 0, the learners: for every learner the driver does what one lane of k_learn_refined (dql_refined.inc) does — the launch's constants as the host side
// makes them, the env state arrays as k_init leaves them, the learner's own refined table slices [2][DQL_N_CELLS], the cut, the carried byte — through a list
// of STAGES: a stage flies its runs (launches) at its level with its schedules and may end with dql_ensemble_transfer's arithmetic on both halves; from the
// second stage on it begins with what dql_ensemble_set_level does (every env re-enters through reset, the per-level books are cleared).  The period index runs
// on across the stages.  Mode 1, the scorer: for every env of every refined table set what one lane of k_score_refined does, then the wave's tally into the
// set's row and the lane's range faults into the call's word.  A lane runs alone: __ballot(p) is p (host_shim.h).  Arrays are exactly as long as the ABI says,
// and every table read of the scorer goes through RefinedTab, which stops on an element outside [0, 2 * DQL_N_CELLS) with exit status 3.
//
//   refined_emu JOB OUT   run what JOB describes (tests/test_refined_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include "emu_learners.h"
#include "dql_score.hpp"
#include "dql_model_split.hpp"
#include "dql_refined.hpp"

using namespace dql;

namespace {

long long g_env = -1;
struct RefinedTab {
  const double* p;
  double operator[](long long k) const {
    if (k < 0 || k >= REFINED_CELLS) { std::fprintf(stderr, "INDEX VIOLATION: refined-table element %lld outside [0, 2 N_CELLS) at env %lld\n", k, g_env); std::exit(3); }
    return p[k];
  }
};

// the job's head: 8 words {cfg size, dtype, mode, feature, n_stages | n_tables, log_cap | log, has_tables | max_steps, episodes}, then n (learners, or envs per
// table set) and the seed, the config, the cut [DQL_N_STATES]
struct Head {
  int dtype, mode, feature, w4, w5, w6, w7;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> cut;
  explicit Head(emu::JobFile& f) : cut((size_t)DQL_N_STATES) {
    int32_t hdr[8]; int64_t ll[2];
    f.read(hdr, 8); f.read(ll, 2);
    f.read_config(cfg, hdr[0]);
    dtype = hdr[1]; mode = hdr[2]; feature = hdr[3]; w4 = hdr[4]; w5 = hdr[5]; w6 = hdr[6]; w7 = hdr[7];
    n = ll[0]; seed = (unsigned long long)ll[1];
    f.read(cut);
    bool ok = n >= 1 && (mode == 0 || mode == 1) && feature >= 0 && feature < DQL_SPLIT_N_FEATURES && emu::config_ok(cfg);
    for (double c : cut) ok = ok && c == c;
    if (!ok) emu::bad_job();
  }
};

// a stage: 12 words {level, n_runs, runs[4], n_eps, window, min_successes, max_episodes, transfer_after, 0}, the ratio, the eps table
struct Stage {
  int level, n_runs, runs[4], n_eps, window, min_successes, max_episodes, transfer_after;
  double ratio;
  std::vector<double> eps;
  explicit Stage(emu::JobFile& f) {
    int32_t h[12];
    f.read(h, 12); f.read(&ratio, 1);
    level = h[0]; n_runs = h[1];
    for (int k = 0; k < 4; ++k) runs[k] = h[2 + k];
    n_eps = h[6]; window = h[7]; min_successes = h[8]; max_episodes = h[9]; transfer_after = h[10];
    if (!(level >= 0 && level < DQL_MAX_LEVELS && emu::runs_ok(runs, n_runs, 4, LEARN_MAX_PERIODS) && emu::sched_ok(n_eps, window, min_successes, max_episodes))) emu::bad_job();
    eps.resize((size_t)n_eps);
    f.read(eps);
  }
};

template <typename T> int learners(const Head& h, emu::JobFile& f, const char* out_path) {
  const int n_stages = h.w4, log_cap = h.w5, has_tables = h.w6, n_alpha = h.w7;
  if (n_stages < 1 || n_stages > 8 || log_cap < 1 || n_alpha < 1) emu::bad_job();
  std::vector<double> alpha((size_t)n_alpha);
  f.read(alpha);
  std::vector<Stage> stages;
  for (int s = 0; s < n_stages; ++s) stages.emplace_back(f);
  emu::Tables tab;  // refined: [n][2][DQL_N_CELLS] each
  const size_t TB = (size_t)h.n * REFINED_CELLS;
  tab.qa.assign(TB, 0.0); tab.qb.assign(TB, 0.0); tab.count.assign(TB, 0.0);
  if (has_tables) { f.read(tab.qa); f.read(tab.qb); f.read(tab.count); }
  dql_config cfg = h.cfg;
  cfg.working_curriculum_step = stages[0].level;  // dql_ensemble_create at the first stage's level
  const emu::Consts<T> k0(cfg);
  emu::LearnerState<T> st(k0, (size_t)h.n, h.seed, log_cap);
  const LearnMem mem = st.mem(tab);
  std::vector<uint8_t> half((size_t)h.n, 0);  // dql_ensemble_set_refinement: zeroed
  const RefinedMem rf{h.cut.data(), half.data(), h.feature};
  long long j0 = 0;
  for (int s = 0; s < n_stages; ++s) {
    const Stage& g = stages[(size_t)s];
    if (s > 0) {  // dql_ensemble_set_level: k_mark_reset on every env, the books re-armed
      for (size_t i = 0; i < st.n_envs; ++i) st.si[i].w |= (FL_DONE << 8);
      st.rearm();
    }
    cfg.working_curriculum_step = g.level;
    const emu::Consts<T> k(cfg);
    const MdpK<T> mdpk = make_mdpk<T>(cfg);
    const SimK<T> cl = k.simk();
    const emu::Launch<T, TICK_PLAIN> lc(cl, h.seed);
    const std::vector<uint32_t> thr = emu::thresholds(g.eps);
    const LearnSched sc{alpha.data(), n_alpha, cfg.alpha_min, thr.data(), g.n_eps, g.window, g.min_successes, g.max_episodes};
    for (int r = 0; r < g.n_runs; ++r) {
      const int np = g.runs[r];
      std::vector<long long> mgr0((size_t)np);
      std::vector<int> sched((size_t)np);
      fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
      for (long long l = 0; l < h.n; ++l)
        refined_learner_periods<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, (const MdpK<T> DQL_CONST_AS*)&mdpk, k.mdp_run, sc, mem, rf, st.sr.data(), st.si.data(), h.seed, l, true, j0,
                                                    np, (const long long*)mgr0.data(), (const int*)sched.data(), lc.kv);
      j0 += np;
    }
    if (g.transfer_after) {  // dql_ensemble_transfer on a refined ensemble: k_ens_transfer's arithmetic over 2 n table sets
      const int kk = g.level, src = (kk - 1 + DQL_MAX_LEVELS) % DQL_MAX_LEVELS;
      for (long long set = 0; set < 2 * h.n; ++set) {
        double* a = tab.qa.data() + (size_t)set * DQL_N_CELLS; double* b = tab.qb.data() + (size_t)set * DQL_N_CELLS;
        for (int i = 0; i < DQL_CELLS_PER_LEVEL; ++i) {
          a[kk * DQL_CELLS_PER_LEVEL + i] = a[src * DQL_CELLS_PER_LEVEL + i] * g.ratio;
          b[kk * DQL_CELLS_PER_LEVEL + i] = b[src * DQL_CELLS_PER_LEVEL + i] * g.ratio;
        }
      }
    }
  }
  emu::ResultFile out(out_path);
  st.put(out, tab);
  out.put(half);
  out.put(&j0, 1);
  return out.close();
}

template <typename T> int scorer(const Head& h, emu::JobFile& f, const char* out_path) {
  const int n_tables = h.w4, want_log = h.w5, max_steps = h.w6, episodes = h.w7;
  if (n_tables < 1 || n_tables > DQL_SCORE_REFINED_MAX_TABLES || max_steps < 1 || max_steps > DQL_SCORE_MAX_STEPS || episodes < 1 || episodes > DQL_SCORE_MAX_EPISODES) emu::bad_job();
  std::vector<double> qa((size_t)n_tables * REFINED_CELLS), qb(qa.size());
  f.read(qa); f.read(qb);
  const dql_config& cfg = h.cfg;
  const emu::Consts<T> k(cfg);
  const MdpK<T> mdpk = make_mdpk<T>(cfg);
  std::vector<long long> mgr0((size_t)max_steps + 1);
  std::vector<int> sched((size_t)max_steps + 1);
  fill_schedule(cfg, 0, mgr0.data(), sched.data(), max_steps + 1);
  const long long n_total = (long long)n_tables * h.n;
  std::vector<int64_t> by_code((size_t)n_tables * SCORE_N_COLS, 0), steps_sum((size_t)n_tables, 0), faults(1, 0);
  std::vector<uint8_t> ep_code; std::vector<uint16_t> ep_steps;
  if (want_log) { ep_code.assign((size_t)episodes * n_total, 0xff); ep_steps.assign((size_t)episodes * n_total, 0); }
  const ScoreLog log{want_log ? ep_code.data() : nullptr, want_log ? ep_steps.data() : nullptr, n_total};
  const SimK<T> cl = k.simk();
  const emu::Launch<T, TICK_PLAIN> lc(cl, h.seed);
  for (int t = 0; t < n_tables; ++t) {
    const RefinedTab ta{qa.data() + (size_t)t * REFINED_CELLS}, tb{qb.data() + (size_t)t * REFINED_CELLS};
    for (long long i = 0; i < h.n; ++i) {
      const long long g = (long long)t * h.n + i;
      g_env = g;
      const ScoreRefinedTally r = score_refined_episodes<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, (const MdpK<T> DQL_CONST_AS*)&mdpk, k.mdp_run, k.init, ta, tb, h.seed, (uint32_t)i,
                                                                             max_steps, episodes, h.feature, h.cut.data(), mgr0.data(), sched.data(), lc.kv, log, g);
      for (int col = 0; col < SCORE_N_COLS; ++col) by_code[(size_t)t * SCORE_N_COLS + col] += r.t.by_code[col];
      steps_sum[(size_t)t] += (int64_t)r.t.steps;
      faults[0] += r.faults;
    }
  }
  emu::ResultFile out(out_path);
  out.put(by_code); out.put(steps_sum); out.put(ep_code); out.put(ep_steps); out.put(faults);
  return out.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: refined_emu JOB OUT\n"); return 2; }
  emu::JobFile f(argv[1]);
  const Head h(f);
  if (h.mode == 0) return h.dtype == DQL_F64 ? learners<double>(h, f, argv[2]) : learners<float>(h, f, argv[2]);
  return h.dtype == DQL_F64 ? scorer<double>(h, f, argv[2]) : scorer<float>(h, f, argv[2]);
}
