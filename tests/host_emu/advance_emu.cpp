// advance_emu.cpp — dql_ensemble_run in curriculum mode, emulated on the CPU from the real device source: dql_advance.hpp's
// build_worklist and advance_learner on top of dql_learner.hpp's learner_periods.
//
// The driver does what ens_run_levels (dql_ensemble.inc) does: launches cut at the multiples of advance_every; at such a period index every learner takes
// advance_learner's step (k_ens_advance: one thread per learner); then the live learners are regrouped by level (build_worklist) and flown wave by wave, lane
// by lane, as k_learn_levels flies them — the wave's level from wave_level[w], the lane's learner from the worklist (-1: an inactive lane), SimK::working, the
// level's MdpK and the level's schedules from that level.  A lane runs alone: __ballot(p) is p (host_shim.h).  Every array is exactly as long as the library
// allocates it, so the sanitized build sees any access beyond them.
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

template <typename V> void read_into(FILE* f, V* p, size_t n) {
  if (n && std::fread(p, sizeof(V), n, f) != n) { std::fprintf(stderr, "short job file\n"); std::exit(2); }
}

Job read_job(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  Job j;
  int32_t hdr[40];  // cfg size, dtype, L, n_runs, runs[8], n_alpha, every, last_level, advance_exhausted, log_cap, then per level {n_eps, window, min_successes, max_episodes}, has_tables, 0 ...
  int64_t seed;
  read_into(f, hdr, 40); read_into(f, &seed, 1);
  if (hdr[0] != (int32_t)sizeof(dql_config)) { std::fprintf(stderr, "dql_config size %d != %d\n", hdr[0], (int)sizeof(dql_config)); std::exit(2); }
  read_into(f, &j.cfg, 1);
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
  if (!ok) { std::fprintf(stderr, "bad job\n"); std::exit(2); }
  read_into(f, j.ratios, ADV_MAX_LEVELS);
  j.alpha.resize((size_t)j.n_alpha);
  read_into(f, j.alpha.data(), j.alpha.size());
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) { j.eps[k].resize((size_t)j.n_eps[k]); read_into(f, j.eps[k].data(), j.eps[k].size()); }
  const size_t TB = (size_t)j.n * DQL_N_CELLS;
  j.qa.assign(TB, 0.0); j.qb.assign(TB, 0.0); j.count.assign(TB, 0.0);
  if (j.has_tables) { read_into(f, j.qa.data(), TB); read_into(f, j.qb.data(), TB); read_into(f, j.count.data(), TB); }
  std::fclose(f);
  return j;
}

template <typename V> void put(FILE* f, const std::vector<V>& v) { std::fwrite(v.data(), sizeof(V), v.size(), f); }

template <typename T> int launch(Job& j, const char* out_path) {
  const dql_config& cfg = j.cfg;
  const size_t n = (size_t)j.n;
  const SimK<T> c = make_simk<T>(cfg);
  MdpK<T> mdpk5[ADV_MAX_LEVELS];
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) { dql_config ck = cfg; ck.working_curriculum_step = k; mdpk5[k] = make_mdpk<T>(ck); }
  const MdpRun<T> mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic};
  const RolloutInit<T> init = make_rollout_init<T>(cfg);
  uint32_t kv_[20];
  const uint32_t* kv = nullptr;
  if constexpr (sizeof(T) == 4) {
    for (int r = 0; r < 10; ++r) { kv_[r] = to_vgpr((uint32_t)j.seed + (uint32_t)r * 0x9E3779B9u); kv_[10 + r] = to_vgpr((uint32_t)(j.seed >> 32) + (uint32_t)r * 0xBB67AE85u); }
    kv = kv_;
  }
  // the state arrays as k_init leaves them (at the config's level)
  std::vector<Quad<T>> sr((size_t)NQ_REAL * n, Quad<T>{T(0.0), T(0.0), T(0.0), T(0.0)});
  std::vector<int4> si(n);
  {
    SimK<T> cl = c;
    cl.two_axis = 0;
    for (size_t l = 0; l < n; ++l) {
      Env<T> e; T mp_v_hbm;
      rollout_init_env(cl, init, e, (uint32_t)l, j.seed, mp_v_hbm);
      sr[11 * n + l] = Quad<T>{mp_v_hbm, T(0.0), T(0.0), T(1.0)};
      sr[13 * n + l] = Quad<T>{e.mp_r, e.mp_w, T(0.0), T(0.0)};
      store_env(e, sr.data(), si.data(), (long long)n, (long long)l, c);
    }
  }
  std::vector<uint32_t> thr[ADV_MAX_LEVELS];
  LevelSched lv[ADV_MAX_LEVELS];
  for (int k = 0; k < ADV_MAX_LEVELS; ++k) {
    thr[k].resize((size_t)j.n_eps[k]);
    for (int i = 0; i < j.n_eps[k]; ++i) thr[k][(size_t)i] = eps_threshold(j.eps[k][(size_t)i]);
    lv[k] = LevelSched{thr[k].data(), j.n_eps[k], j.window[k], j.min_successes[k], j.max_episodes[k]};
  }
  std::vector<double>& qa = j.qa;
  std::vector<double>& qb = j.qb;
  std::vector<double>& count = j.count;
  std::vector<unsigned long long> decisions(n, 0ull), by_code((size_t)DQL_N_CHECK_CODES * n, 0ull), win_bits(2 * n, 0ull), faults(1, 0ull);
  std::vector<int> episodes(n, 0), successes(n, 0), lvl(n, 0), win_count(n, 0), promoted(n, -1), frozen(n, 0), log_n(n, 0);
  std::vector<uint8_t> log_code(n * (size_t)j.log_cap, 0);
  std::vector<uint16_t> log_len(n * (size_t)j.log_cap, 0);
  const LearnMem mem{qa.data(), qb.data(), count.data(), decisions.data(), by_code.data(), episodes.data(), successes.data(), lvl.data(), win_count.data(),
                     win_bits.data(), promoted.data(), frozen.data(), log_code.data(), log_len.data(), log_n.data(), faults.data(), (long long)n, j.log_cap};
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
        for (size_t l = 0; l < n; ++l) (void)advance_learner(mem, adv, rule, si.data(), (long long)l, j0, DQL_CELLS_PER_LEVEL);
      long long unfinished = 0;
      for (size_t l = 0; l < n; ++l) unfinished += learner_finished(frozen[l], level[l], promoted[l], rule) ? 0 : 1;
      if (unfinished == 0) { j0 += left; break; }
      const long long to_point = j.every - j0 % j.every;
      const int np = (int)(left < to_point ? left : to_point);
      const int n_waves = build_worklist(frozen.data(), level.data(), (long long)n, worklist.data(), wave_level.data(), slots, faults.data());
      std::vector<long long> mgr0((size_t)np);
      std::vector<int> sched((size_t)np);
      fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
      for (int w = 0; w < n_waves; ++w) {
        const int k = wave_level[(size_t)w];
        if ((unsigned)k >= (unsigned)ADV_MAX_LEVELS) { faults[0] += 1ull; continue; }
        SimK<T> cl = c;
        cl.working = k;
        cl.two_axis = 0;
        SimK<T> cfgk = cl;
        if constexpr (sizeof(T) == 4) cfgk = period_consts_in_vgprs(cfgk);
        const TickConsts<TICK_PLAIN, T> tc(cfgk);
        const LearnSched sc{j.alpha.data(), j.n_alpha, cfg.alpha_min, lv[k].eps_tab, lv[k].n_eps, lv[k].window, lv[k].min_successes, lv[k].max_episodes};
        const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk5[k];
        for (int lane = 0; lane < ADV_WAVE; ++lane) {
          const long long l = worklist[(size_t)w * ADV_WAVE + (size_t)lane];
          learner_periods<TICK_PLAIN, X_ONLY>(cl, cfgk, tc, mdp, mdp_run, sc, mem, sr.data(), si.data(), j.seed, l, l >= 0 && l < (long long)n, j0, np, mgr0.data(), sched.data(), kv);
        }
      }
      j0 += np; left -= np;
    }
  }
  // dql_ensemble_get_levels: the row of a learner's current level shows its counters as they stand
  for (size_t l = 0; l < n; ++l) { promoted_at[(size_t)level[l] * n + l] = promoted[l]; episodes_at[(size_t)level[l] * n + l] = lvl[l]; }
  std::vector<double> reals((size_t)NF_REAL * n);
  std::vector<int32_t> ints((size_t)NF_INT * n);
  for (int f = 0; f < NF_REAL; ++f)
    for (size_t l = 0; l < n; ++l) { const Quad<T>& q = sr[(size_t)(f / 4) * n + l]; const T v = (f % 4 == 0) ? q.a : (f % 4 == 1) ? q.b : (f % 4 == 2) ? q.c : q.d; reals[(size_t)f * n + l] = (double)v; }
  for (size_t l = 0; l < n; ++l) {
    const int4 h = si[l];
    ints[0 * n + l] = h.x; ints[1 * n + l] = h.y; ints[2 * n + l] = h.z & 0xffff; ints[3 * n + l] = (h.z >> 16) & 0xffff;
    ints[4 * n + l] = h.w & 0xff; ints[5 * n + l] = (h.w >> 8) & 0xff; ints[6 * n + l] = (h.w >> 16) & 0xff;
  }
  std::vector<long long> tail{j0};
  FILE* f = std::fopen(out_path, "wb");
  if (!f) { std::perror(out_path); return 2; }
  put(f, qa); put(f, qb); put(f, count); put(f, decisions); put(f, by_code);
  put(f, episodes); put(f, successes); put(f, lvl); put(f, promoted); put(f, frozen); put(f, log_n);
  put(f, log_code); put(f, log_len); put(f, reals); put(f, ints); put(f, faults);
  put(f, level); put(f, promoted_at); put(f, episodes_at); put(f, entered); put(f, tail);
  return std::fclose(f) == 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: advance_emu JOB OUT\n"); return 2; }
  Job j = read_job(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
