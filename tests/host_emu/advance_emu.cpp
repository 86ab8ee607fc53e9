// advance_emu.cpp — dql_ensemble_run in curriculum mode, emulated on the CPU from the real device source: dql_advance.hpp's
// build_worklist and advance_learner on top of dql_learner.hpp's learner_periods.
//
// The driver does what ens_run_advancing does for ens_run_levels (dql_ensemble.inc): launches cut at the multiples of advance_every; at such a period index every learner takes
// advance_learner's step (k_ens_advance: one thread per learner); then the live learners are regrouped by level (build_worklist) and flown wave by wave, lane
// by lane, as k_learn_levels flies them — the wave's level from wave_level[w], the lane's learner from the worklist (-1: an inactive lane), SimK::working, the
// level's MdpK and the level's schedules from that level.  A lane runs alone: __ballot(p) is p (host_shim.h).  Every array is exactly as long as the library
// allocates it, so the sanitized build sees any access beyond them.  The learners' arrays and the head of the result file (emu::LearnerState), the per-wave
// prologue (emu::Launch) and the job and result files are emu_common.h's; learner_emu.cpp uses the same.
//
//   advance_emu JOB OUT   run the calls described by JOB (see read_job; tests/test_advance_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_advance.hpp"
#define DQL_EMU_LEARNERS
#include "emu_common.h"

using namespace dql;

namespace {

struct Job {
  int dtype, n_runs, runs[8], n_alpha, every, last_level, advance_exhausted, log_cap, has_tables;
  int n_eps[ADV_MAX_LEVELS], window[ADV_MAX_LEVELS], min_successes[ADV_MAX_LEVELS], max_episodes[ADV_MAX_LEVELS];
  long long n;
  unsigned long long seed;
  dql_config cfg;
  double ratios[ADV_MAX_LEVELS];
  std::vector<double> alpha, eps[ADV_MAX_LEVELS], qa, qb, count;  // the tables: zeros, or the job's initial ones ([L][DQL_N_CELLS] each, after the eps tables)
};

Job read_job(const char* path) {
  emu::JobFile f(path);
  Job j;
  int32_t hdr[40];  // cfg size, dtype, L, n_runs, runs[8], n_alpha, every, last_level, advance_exhausted, log_cap, then per level {n_eps, window, min_successes, max_episodes}, has_tables, 0 ...
  int64_t seed;
  f.read(hdr, 40); f.read(&seed, 1);
  f.read_config(j.cfg, hdr[0]);
  j.dtype = hdr[1]; j.n = hdr[2]; j.n_runs = hdr[3];
  for (int k = 0; k < 8; ++k) j.runs[k] = hdr[4 + k];
  j.seed = (unsigned long long)seed;
  j.n_alpha = hdr[12]; j.every = hdr[13]; j.last_level = hdr[14]; j.advance_exhausted = hdr[15]; j.log_cap = hdr[16]; j.has_tables = hdr[37];
  bool ok = j.n >= 1 && j.n_runs >= 1 && j.n_runs <= 8 && j.n_alpha >= 1 && j.every >= 1 && j.every <= ADV_MAX_EVERY && j.last_level >= j.cfg.working_curriculum_step &&
            j.last_level < ADV_MAX_LEVELS && j.log_cap >= 1 && !j.cfg.two_axis && j.cfg.trajectory != DQL_TRAJ_EIGHT;
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) {
    j.n_eps[k] = hdr[17 + 4 * k]; j.window[k] = hdr[18 + 4 * k]; j.min_successes[k] = hdr[19 + 4 * k]; j.max_episodes[k] = hdr[20 + 4 * k];
    ok = ok && j.n_eps[k] >= 1 && j.window[k] >= 1 && j.window[k] <= LEARN_MAX_WINDOW && j.min_successes[k] >= 1 && j.max_episodes[k] >= 1;
  }
  for (int k = 0; ok && k < j.n_runs; ++k) ok = j.runs[k] >= 1;
  if (!ok) emu::bad_job();
  f.read(j.ratios, ADV_MAX_LEVELS);
  j.alpha.resize((size_t)j.n_alpha);
  f.read(j.alpha);
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) { j.eps[k].resize((size_t)j.n_eps[k]); f.read(j.eps[k]); }
  const size_t TB = (size_t)j.n * DQL_N_CELLS;
  j.qa.assign(TB, 0.0); j.qb.assign(TB, 0.0); j.count.assign(TB, 0.0);
  if (j.has_tables) { f.read(j.qa); f.read(j.qb); f.read(j.count); }
  return j;
}

template <typename T> int launch(Job& j, const char* out_path) {
  const dql_config& cfg = j.cfg;
  const size_t n = (size_t)j.n;
  const SimK<T> c = make_simk<T>(cfg);
  MdpK<T> mdpk5[ADV_MAX_LEVELS];
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) { dql_config ck = cfg; ck.working_curriculum_step = k; mdpk5[k] = make_mdpk<T>(ck); }
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  emu::LearnerState<T> st(c, init, n, j.seed, j.log_cap);  // (at the config's level)
  std::vector<uint32_t> thr[ADV_MAX_LEVELS];
  LevelSched lv[ADV_MAX_LEVELS];
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) {
    thr[k].resize((size_t)j.n_eps[k]);
    for (int i = 0; i < j.n_eps[k]; ++i) thr[k][(size_t)i] = eps_threshold(j.eps[k][(size_t)i]);
    lv[k] = LevelSched{thr[k].data(), j.n_eps[k], j.window[k], j.min_successes[k], j.max_episodes[k]};
  }
  const LearnMem mem = st.mem(j.qa, j.qb, j.count);
  std::vector<int> level(n, cfg.working_curriculum_step), promoted_at((size_t)ADV_MAX_LEVELS * n, -1), episodes_at((size_t)ADV_MAX_LEVELS * n, 0);
  std::vector<long long> entered((size_t)ADV_MAX_LEVELS * n, -1);
  for (size_t l = 0; l < n; ++l) entered[(size_t)cfg.working_curriculum_step * n + l] = 0;
  const AdvanceMem adv{level.data(), promoted_at.data(), episodes_at.data(), entered.data()};
  AdvanceRule rule;
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) rule.ratios[k] = j.ratios[k];
  rule.last_level = j.last_level; rule.advance_exhausted = j.advance_exhausted;
  const long long slots = worklist_capacity((long long)n);
  std::vector<int> worklist((size_t)slots), wave_level((size_t)(slots / ADV_WAVE));

  long long j0 = 0;
  for (int r = 0; r < j.n_runs; ++r) {
    long long left = j.runs[r];
    while (left > 0) {
      if (j0 % j.every == 0)
        for (size_t l = 0; l < n; ++l) (void)advance_learner(mem, adv, rule, st.si.data(), (long long)l, j0, DQL_CELLS_PER_LEVEL);
      long long unfinished = 0;
      for (size_t l = 0; l < n; ++l) unfinished += learner_finished(st.frozen[l], level[l], st.promoted[l], rule) ? 0 : 1;
      if (unfinished == 0) { j0 += left; break; }
      const long long to_point = j.every - j0 % j.every;
      const int np = (int)(left < to_point ? left : to_point);
      const int n_waves = build_worklist(st.frozen.data(), level.data(), (long long)n, worklist.data(), wave_level.data(), slots, st.faults.data());
      std::vector<long long> mgr0((size_t)np);
      std::vector<int> sched((size_t)np);
      fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
      for (int w = 0; w < n_waves; ++w) {
        const int k = wave_level[(size_t)w];
        if ((unsigned)k >= (unsigned)ADV_MAX_LEVELS) { st.faults[0] += 1ull; continue; }
        SimK<T> cl = c;
        cl.working = k;
        cl.two_axis = 0;
        const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
        const LearnSched sc = learn_sched(j.alpha.data(), j.n_alpha, cfg.alpha_min, (const LevelSched DQL_CONST_AS*)&lv[k]);
        const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk5[k];
        for (int lane = 0; lane < ADV_WAVE; ++lane) {
          const long long l = worklist[(size_t)w * ADV_WAVE + (size_t)lane];
          learner_periods<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, mdp_run, sc, mem, st.sr.data(), st.si.data(), j.seed, l, l >= 0 && l < (long long)n, j0, np, mgr0.data(), sched.data(), lc.kv);
        }
      }
      j0 += np; left -= np;
    }
  }
  // dql_ensemble_get_levels: the row of a learner's current level shows its counters as they stand
  for (size_t l = 0; l < n; ++l) { promoted_at[(size_t)level[l] * n + l] = st.promoted[l]; episodes_at[(size_t)level[l] * n + l] = st.lvl[l]; }
  emu::ResultFile f(out_path);
  st.put(f, j.qa, j.qb, j.count);
  f.put(level); f.put(promoted_at); f.put(episodes_at); f.put(entered); f.put(&j0, 1);
  return f.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: advance_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
