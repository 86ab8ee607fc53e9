// emu_learners.h — what the drivers of the sequential-learner family share beyond emu_common.h: learner_emu, nstep_emu, team_emu, team_nstep_emu (plain
// jobs: every learner on the config's level) and advance_emu, recipes_emu, nstep_recipes_emu (advancing jobs: levels, recipes).  Included after host_shim.h;
// it pulls in the learner family's device headers itself.  It owns the job files' layouts and their validity clauses, the learners' state and the head of every
// result file, the checked and poisoned storage of the pending windows, the launch constants, and the two run loops (for_each_launch: dql_ensemble_run in
// the plain modes; run_advancing: ens_run_advancing).  A driver keeps what restates one kernel: what a lane, a team or a wave does in one launch.
// The Python side of the same layouts is tests/host_emu_harness.py (learner_job, recipes_job, learner_result).
#pragma once
#include <climits>
#include <cmath>

#include "dql_device.hpp"
#include "dql_host_consts.hpp"
#include "dql_rollout.hpp"
#include "dql_learner.hpp"
#include "dql_returns.hpp"
#include "dql_nstep.hpp"
#include "dql_advance.hpp"
#include "dql_recipes.hpp"
#include "emu_common.h"

namespace emu {

// ---- the jobs: the validity clauses every layout shares, the initial tables every layout ends with
inline bool config_ok(const dql_config& cfg) { return !cfg.two_axis && cfg.trajectory != DQL_TRAJ_EIGHT; }
inline bool runs_ok(const int* runs, int n_runs, int max_runs, int max_periods) {
  bool ok = n_runs >= 1 && n_runs <= max_runs;
  for (int k = 0; ok && k < n_runs; ++k) ok = runs[k] >= 1 && runs[k] <= max_periods;
  return ok;
}
inline bool sched_ok(int n_eps, int window, int min_successes, int max_episodes) {
  return n_eps >= 1 && window >= 1 && window <= dql::LEARN_MAX_WINDOW && min_successes >= 1 && max_episodes >= 1;
}
struct Tables {  // zeros, or the job's initial ones ([L][DQL_N_CELLS] each, at the end of the job)
  std::vector<double> qa, qb, count;
  void read(JobFile& f, long long n, int has_tables) {
    const size_t TB = (size_t)n * DQL_N_CELLS;
    qa.assign(TB, 0.0); qb.assign(TB, 0.0); count.assign(TB, 0.0);
    if (has_tables) { f.read(qa); f.read(qb); f.read(count); }
  }
};

// the plain layout: 16 words {cfg size, dtype, L, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, has_tables, word15} and
// n_extra (0..2) more, the seed, the config, alpha, eps, the tables.  word15 and the extra words are the driver's, and so are the clauses on them (extra_ok)
struct LearnerJob : Tables {
  int dtype, n_runs, runs[4], n_alpha, n_eps, window, min_successes, max_episodes, log_cap, word15, extra[2];
  long long n;
  unsigned long long seed;
  dql_config cfg;
  std::vector<double> alpha, eps;
  template <typename ExtraOk> LearnerJob(const char* path, int n_extra, ExtraOk extra_ok) {
    JobFile f(path);
    int32_t hdr[18] = {};
    int64_t s;
    f.read(hdr, 16 + (size_t)n_extra); f.read(&s, 1);
    f.read_config(cfg, hdr[0]);
    dtype = hdr[1]; n = hdr[2]; n_runs = hdr[3];
    for (int k = 0; k < 4; ++k) runs[k] = hdr[4 + k];
    n_alpha = hdr[8]; n_eps = hdr[9]; window = hdr[10]; min_successes = hdr[11]; max_episodes = hdr[12]; log_cap = hdr[13];
    word15 = hdr[15]; extra[0] = hdr[16]; extra[1] = hdr[17];
    seed = (unsigned long long)s;
    if (!(n >= 1 && runs_ok(runs, n_runs, 4, dql::LEARN_MAX_PERIODS) && n_alpha >= 1 && sched_ok(n_eps, window, min_successes, max_episodes) && log_cap >= 1 &&
          config_ok(cfg) && extra_ok(*this)))
      bad_job();
    alpha.resize((size_t)n_alpha); eps.resize((size_t)n_eps);
    f.read(alpha); f.read(eps);
    Tables::read(f, n, hdr[14]);
  }
};

// the schedules of the five levels as an advancing job carries them: four words per level in its header, the eps tables among its arrays
struct JobLevels {
  int n_eps[dql::ADV_MAX_LEVELS], window[dql::ADV_MAX_LEVELS], min_successes[dql::ADV_MAX_LEVELS], max_episodes[dql::ADV_MAX_LEVELS];
  std::vector<double> eps[dql::ADV_MAX_LEVELS];
  bool take(const int32_t* h) {  // h: per level {n_eps, window, min_successes, max_episodes}
    bool ok = true;
    for (int k = 0; k < dql::ADV_MAX_LEVELS; ++k) {
      n_eps[k] = h[4 * k]; window[k] = h[4 * k + 1]; min_successes[k] = h[4 * k + 2]; max_episodes[k] = h[4 * k + 3];
      ok = ok && sched_ok(n_eps[k], window[k], min_successes[k], max_episodes[k]);
    }
    return ok;
  }
  void read_eps(JobFile& f) { for (int k = 0; k < dql::ADV_MAX_LEVELS; ++k) { eps[k].resize((size_t)n_eps[k]); f.read(eps[k]); } }
};
inline bool advancing_ok(const dql_config& cfg, const int* runs, int n_runs, int every, int log_cap) {
  return runs_ok(runs, n_runs, 8, INT_MAX) && every >= 1 && every <= dql::ADV_MAX_EVERY && log_cap >= 1 && config_ok(cfg);
}
inline bool rule_ok(const dql_config& cfg, int n_alpha, int last_level) { return n_alpha >= 1 && last_level >= cfg.working_curriculum_step && last_level < dql::ADV_MAX_LEVELS; }

// the recipe layout: 24 words {cfg size, dtype, L, n_runs, runs[8], every, log_cap, n_recipes, has_tables, mode, worklist capacity (mode 1), 0 ...}, the seed, the
// config, recipe_of[L]; then (mode 0) per recipe 28 words {quirks, n_alpha, last_level, advance_exhausted, transfer_order, nstep, 0, 0, then JobLevels' words},
// alpha_min, ratios[5], alpha, the eps tables; the tables at the end.  Mode 1 (recipes_emu's worklist_only) carries frozen[L] and level[L] instead
struct JobRecipe : JobLevels {
  uint32_t quirks;
  int n_alpha, last_level, advance_exhausted, transfer_order, nstep;
  double alpha_min, ratios[dql::ADV_MAX_LEVELS];
  std::vector<double> alpha;
};
struct RecipeJob : Tables {
  int mode, dtype, n_runs, runs[8], every, log_cap, n_recipes;
  long long n, cap_slots;
  unsigned long long seed;
  dql_config cfg;
  std::vector<int> recipe_of, frozen, level;  // frozen, level: mode 1 only
  std::vector<JobRecipe> recipes;
  RecipeJob(const char* path, bool one_step) {  // one_step (recipes_emu): mode 1 exists, and nstep is carried as 0 and never looked at
    JobFile f(path);
    int32_t hdr[24];
    int64_t s;
    f.read(hdr, 24); f.read(&s, 1);
    f.read_config(cfg, hdr[0]);
    dtype = hdr[1]; n = hdr[2]; n_runs = hdr[3];
    for (int k = 0; k < 8; ++k) runs[k] = hdr[4 + k];
    seed = (unsigned long long)s;
    every = hdr[12]; log_cap = hdr[13]; n_recipes = hdr[14]; mode = one_step ? hdr[16] : 0; cap_slots = hdr[17];
    if (n < 1 || (mode != 0 && mode != 1)) bad_job();
    recipe_of.resize((size_t)n);
    f.read(recipe_of);
    if (mode == 1) {  // (any n_recipes and any indices: the faults are what is looked at)
      if (cap_slots < 0) bad_job();
      frozen.resize((size_t)n); level.resize((size_t)n);
      f.read(frozen); f.read(level);
      return;
    }
    bool ok = advancing_ok(cfg, runs, n_runs, every, log_cap) && n_recipes >= 1 && n_recipes <= dql::RCP_MAX;
    for (size_t l = 0; ok && l < (size_t)n; ++l) ok = recipe_of[l] >= 0 && recipe_of[l] < n_recipes;
    if (!ok) bad_job();
    recipes.resize((size_t)n_recipes);
    for (JobRecipe& r : recipes) {
      int32_t h[28];
      f.read(h, 28);
      r.quirks = (uint32_t)h[0]; r.n_alpha = h[1]; r.last_level = h[2]; r.advance_exhausted = h[3]; r.transfer_order = h[4]; r.nstep = h[5];
      ok = rule_ok(cfg, r.n_alpha, r.last_level) && (r.transfer_order == 0 || r.transfer_order == 1) &&
           (one_step || (r.nstep >= 0 && r.nstep <= dql::NSTEP_MAX));
      if (!(r.take(h + 8) && ok)) bad_job();
      f.read(&r.alpha_min, 1); f.read(r.ratios, dql::ADV_MAX_LEVELS);
      r.alpha.resize((size_t)r.n_alpha);
      f.read(r.alpha);
      r.read_eps(f);
    }
    Tables::read(f, n, hdr[15]);
  }
};

// ---- the launch constants as the host side makes them from the config: the context's SimK, MdpRun, what k_init reads; simk(): SimK as a launch sees it
template <typename T> struct Consts {
  const dql::SimK<T> c;
  const dql::MdpRun<T> mdp_run;
  const dql::RolloutInit<T> init;
  explicit Consts(const dql_config& cfg) : c(dql::make_simk<T>(cfg)), mdp_run{cfg.gamma, (T)(cfg.t_max * cfg.f_ag), cfg.goal_logic}, init(dql::make_rollout_init<T>(cfg)) {}
  dql::SimK<T> simk() const { dql::SimK<T> cl = c; cl.two_axis = 0; return cl; }
  dql::SimK<T> simk(int working, uint32_t quirks) const { dql::SimK<T> cl = simk(); cl.working = working; cl.quirks = quirks; return cl; }
};
inline std::vector<uint32_t> thresholds(const std::vector<double>& eps) {
  std::vector<uint32_t> thr(eps.size());
  for (size_t i = 0; i < eps.size(); ++i) thr[i] = dql::eps_threshold(eps[i]);
  return thr;
}
struct LevelTables {  // LevelSched of the five levels over their thresholds
  std::vector<uint32_t> thr[dql::ADV_MAX_LEVELS];
  dql::LevelSched lv[dql::ADV_MAX_LEVELS];
  explicit LevelTables(const JobLevels& q) {
    for (int k = 0; k < dql::ADV_MAX_LEVELS; ++k) {
      thr[k] = thresholds(q.eps[k]);
      lv[k] = dql::LevelSched{thr[k].data(), q.n_eps[k], q.window[k], q.min_successes[k], q.max_episodes[k]};
    }
  }
  LevelTables(const LevelTables&) = delete;
};
template <typename T> void mdpk_per_level(dql_config cfg, dql::MdpK<T>* out) {  // [5]: the config with working = k
  for (int k = 0; k < dql::ADV_MAX_LEVELS; ++k) { cfg.working_curriculum_step = k; out[k] = dql::make_mdpk<T>(cfg); }
}
// what dql_ensemble_set_recipe installs: MdpK [R][5] with the recipe's quirks, RecipeSched, RecipeRule and the recipe's n (EnsRecipes::d_nstep)
template <typename T> struct RecipeTables {
  std::vector<dql::MdpK<T>> mdpk;
  std::vector<LevelTables> lt;
  std::vector<dql::RecipeSched> rs;
  std::vector<dql::RecipeRule> rules;
  std::vector<int> nstep;
  RecipeTables(const dql_config& cfg, const std::vector<JobRecipe>& recipes)
      : mdpk(recipes.size() * dql::ADV_MAX_LEVELS), lt(recipes.begin(), recipes.end()), rs(recipes.size()), rules(recipes.size()), nstep(recipes.size()) {
    for (size_t r = 0; r < recipes.size(); ++r) {
      const JobRecipe& q = recipes[r];
      dql_config cq = cfg;
      cq.quirks = q.quirks;
      mdpk_per_level(cq, &mdpk[r * dql::ADV_MAX_LEVELS]);
      rs[r].alpha_tab = q.alpha.data(); rs[r].n_alpha = q.n_alpha; rs[r].quirks = q.quirks; rs[r].alpha_min = q.alpha_min;
      for (int k = 0; k < dql::ADV_MAX_LEVELS; ++k) { rs[r].lv[k] = lt[r].lv[k]; rules[r].rule.ratios[k] = q.ratios[k]; }
      rules[r].rule.last_level = q.last_level; rules[r].rule.advance_exhausted = q.advance_exhausted; rules[r].transfer_order = q.transfer_order; rules[r].pad_ = 0;
      nstep[r] = q.nstep;
    }
  }
};

// ---- the learners of an ensemble, in arrays exactly as long as the library allocates them (per-learner arrays [n], per-env arrays [n_envs] = [n * E] for
// teams): the env state as k_init leaves it in a context of n_envs envs (c: the context's SimK, whose level is the config's), the counters zeroed; mem() is
// the kernels' view of them with the job's tables, put() the head of every result file, rearm() what dql_ensemble_rearm clears
template <typename T> struct LearnerState {
  const size_t n, n_envs;
  const int log_cap;
  std::vector<dql::Quad<T>> sr;
  std::vector<int4> si;
  std::vector<unsigned long long> decisions, by_code, win_bits, faults;
  std::vector<int> episodes, successes, lvl, win_count, promoted, frozen, log_n;
  std::vector<uint8_t> log_code;
  std::vector<uint16_t> log_len;

  LearnerState(const Consts<T>& k, size_t n_, unsigned long long seed, int log_cap_, size_t envs_per_learner = 1)
      : n(n_), n_envs(n_ * envs_per_learner), log_cap(log_cap_), sr((size_t)dql::NQ_REAL * n_envs, dql::Quad<T>{T(0.0), T(0.0), T(0.0), T(0.0)}), si(n_envs),
        decisions(n, 0ull), by_code((size_t)DQL_N_CHECK_CODES * n, 0ull), win_bits(2 * n, 0ull), faults(1, 0ull), episodes(n, 0), successes(n, 0), lvl(n, 0),
        win_count(n, 0), promoted(n, -1), frozen(n, 0), log_n(n, 0), log_code(n * (size_t)log_cap, 0), log_len(n * (size_t)log_cap, 0) {
    const dql::SimK<T> cl = k.simk();
    for (size_t g = 0; g < n_envs; ++g) {
      dql::Env<T> e; T mp_v_hbm;
      dql::rollout_init_env(cl, k.init, e, (uint32_t)g, seed, mp_v_hbm);
      sr[11 * n_envs + g] = dql::Quad<T>{mp_v_hbm, T(0.0), T(0.0), T(1.0)};
      sr[13 * n_envs + g] = dql::Quad<T>{e.mp_r, e.mp_w, T(0.0), T(0.0)};
      dql::store_env(e, sr.data(), si.data(), (long long)n_envs, (long long)g, k.c);
    }
  }
  dql::LearnMem mem(Tables& t) {
    return dql::LearnMem{t.qa.data(), t.qb.data(), t.count.data(), decisions.data(), by_code.data(), episodes.data(), successes.data(), lvl.data(), win_count.data(),
                         win_bits.data(), promoted.data(), frozen.data(), log_code.data(), log_len.data(), log_n.data(), faults.data(), (long long)n, log_cap};
  }
  void rearm() {  // per-level counters, ring, promotion record and frozen flag; envs and windows stay
    for (size_t l = 0; l < n; ++l) { lvl[l] = 0; win_count[l] = 0; win_bits[l] = 0ull; win_bits[n + l] = 0ull; promoted[l] = -1; frozen[l] = 0; }
  }
  void put(ResultFile& out, const Tables& t) const {
    std::vector<double> reals;
    std::vector<int32_t> ints;
    unpack_state(sr.data(), si.data(), n_envs, reals, ints);
    out.put(t.qa); out.put(t.qb); out.put(t.count); out.put(decisions); out.put(by_code);
    out.put(episodes); out.put(successes); out.put(lvl); out.put(promoted); out.put(frozen); out.put(log_n);
    out.put(log_code); out.put(log_len); out.put(reals); out.put(ints); out.put(faults);
  }
};

// ---- the pending windows: storage as the device code indexes it, every element reached bounds-checked (exit status 3), every entry poisoned until written
template <typename V> struct Checked {
  V* p; long long size; const char* what;
  V& operator[](long long k) const {
    if (k < 0 || k >= size) { std::fprintf(stderr, "INDEX VIOLATION: element %lld of %s outside [0, %lld)\n", k, what, size); std::exit(3); }
    return p[k];
  }
};
template <typename V> Checked<V> checked(std::vector<V>& v, const char* what) { return Checked<V>{v.data(), (long long)v.size(), what}; }
inline void poison(std::vector<uint16_t>& key, std::vector<double>& val) { key.assign(key.size(), (uint16_t)0xffffu); val.assign(val.size(), std::nan("")); }
inline void poison(std::vector<int>& head_or_len) { head_or_len.assign(head_or_len.size(), 1 << 20); }  // (a working copy's: far out of range)

// the persistent windows, as long as the library allocates them: [NSTEP_MAX][columns] plus len[columns] (a column per learner, or per env of a team); the
// lengths zeroed, the entries poisoned.  len is the tail of the n-step drivers' result files
struct PersistentWindows {
  std::vector<uint16_t> key;
  std::vector<double> val;
  std::vector<int> len;
  explicit PersistentWindows(size_t columns) : key((size_t)dql::NSTEP_MAX * columns), val((size_t)dql::NSTEP_MAX * columns), len(columns, 0) { poison(key, val); }
  dql::NstepMem<Checked<uint16_t>, Checked<double>, Checked<int>> mem() {
    return {checked(key, "the persistent keys"), checked(val, "the persistent rewards"), checked(len, "the persistent lengths")};
  }
};
// a wave's working copy, which stands for the kernel's LDS: [NSTEP_MAX][64], a lane's window in its column (dql_nstep.inc's LdsWindow).  LDS carries nothing
// from launch to launch: poison() before every launch, so that an entry read before it was written, or kept here only, changes the result
struct WaveWindows {
  std::vector<uint16_t> key = std::vector<uint16_t>((size_t)dql::NSTEP_MAX * 64);
  std::vector<double> val = std::vector<double>((size_t)dql::NSTEP_MAX * 64);
  void poison() { emu::poison(key, val); }
  struct View {
    Checked<uint16_t> k; Checked<double> v; int lane;
    long long at(int slot) const {
      if (slot < 0 || slot >= dql::NSTEP_MAX) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d\n", slot); std::exit(3); }
      return (long long)slot * 64 + lane;
    }
    uint16_t& key(int slot) const { return k[at(slot)]; }
    double& val(int slot) const { return v[at(slot)]; }
  };
  View view(int lane) { return View{checked(key, "the working keys"), checked(val, "the working rewards"), lane}; }
};

// ---- the plain run loop (dql_ensemble_run without levels): per run the schedule of np periods from period index j0, body(j0, np, mgr0, sched), then
// after_run(r) (team_nstep_emu's rearm)
template <typename Body, typename AfterRun> void for_each_launch(const dql_config& cfg, const int* runs, int n_runs, Body body, AfterRun after_run) {
  long long j0 = 0;
  for (int r = 0; r < n_runs; ++r) {
    const int np = runs[r];
    std::vector<long long> mgr0((size_t)np);
    std::vector<int> sched((size_t)np);
    dql::fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
    body(j0, np, (const long long*)mgr0.data(), (const int*)sched.data());
    j0 += np;
    after_run(r);
  }
}
template <typename Body> void for_each_launch(const dql_config& cfg, const int* runs, int n_runs, Body body) { for_each_launch(cfg, runs, n_runs, body, [](int) {}); }

// what the launches of a plain job read: the constants, the prologue, the learners (with envs_per_learner envs each), the job's schedules
template <typename T> struct PlainRun {
  LearnerJob& j;
  const Consts<T> k;
  const dql::MdpK<T> mdpk;
  const dql::SimK<T> cl;
  const Launch<T, dql::TICK_PLAIN> lc;
  const dql::MdpK<T> DQL_CONST_AS* const mdp;
  LearnerState<T> st;
  const std::vector<uint32_t> thr;
  const dql::LearnSched sc;
  const dql::LearnMem mem;
  explicit PlainRun(LearnerJob& job, size_t envs_per_learner = 1)
      : j(job), k(j.cfg), mdpk(dql::make_mdpk<T>(j.cfg)), cl(k.simk()), lc(cl, j.seed), mdp((const dql::MdpK<T> DQL_CONST_AS*)&mdpk),
        st(k, (size_t)j.n, j.seed, j.log_cap, envs_per_learner), thr(thresholds(j.eps)),
        sc{j.alpha.data(), j.n_alpha, j.cfg.alpha_min, thr.data(), j.n_eps, j.window, j.min_successes, j.max_episodes}, mem(st.mem(j)) {}
};

// ---- the advancing run loop, as ens_run_advancing (dql_ensemble.inc) has it
// a learner's level and its history per level, as dql_ensemble_create leaves them (AdvanceMem); put(): the advancing drivers' part of the result file
struct LevelBooks {
  const size_t n;
  std::vector<int> level, promoted_at, episodes_at;
  std::vector<long long> entered;
  LevelBooks(size_t n_, int start) : n(n_), level(n, start), promoted_at((size_t)dql::ADV_MAX_LEVELS * n, -1), episodes_at((size_t)dql::ADV_MAX_LEVELS * n, 0),
                                     entered((size_t)dql::ADV_MAX_LEVELS * n, -1) {
    for (size_t l = 0; l < n; ++l) entered[(size_t)start * n + l] = 0;
  }
  dql::AdvanceMem mem() { return dql::AdvanceMem{level.data(), promoted_at.data(), episodes_at.data(), entered.data()}; }
  // dql_ensemble_get_levels: the row of a learner's current level shows its counters as they stand
  template <typename T> void put(ResultFile& f, const LearnerState<T>& st, long long j0) {
    for (size_t l = 0; l < n; ++l) { promoted_at[(size_t)level[l] * n + l] = st.promoted[l]; episodes_at[(size_t)level[l] * n + l] = st.lvl[l]; }
    f.put(level); f.put(promoted_at); f.put(episodes_at); f.put(entered); f.put(&j0, 1);
  }
};
// the result file: the learners, then what the advancing drivers add (their books and the period index reached), then the n-step drivers' persistent lengths
template <typename T> int write_result(const char* path, const LearnerState<T>& st, const Tables& t, const PersistentWindows* pw = nullptr, LevelBooks* books = nullptr, long long j0 = 0) {
  ResultFile f(path);
  st.put(f, t);
  if (books) books->put(f, st, j0);
  if (pw) f.put(pw->len);
  return f.close();
}
// Launches cut at the multiples of `every`; at such a period index, before that period is flown, advance() (every learner's step); when finished(l) holds for
// all n learners the period index moves on and nothing is flown; else build() regroups the live learners and returns the number of waves, and
// fly_wave(w, j0, np, mgr0, sched) flies each.  -> the period index reached
template <typename Advance, typename Finished, typename Build, typename FlyWave>
long long run_advancing(const dql_config& cfg, const int* runs, int n_runs, int every, size_t n, Advance advance, Finished finished, Build build, FlyWave fly_wave) {
  long long j0 = 0;
  for (int r = 0; r < n_runs; ++r) {
    long long left = runs[r];
    while (left > 0) {
      if (j0 % every == 0) advance(j0);
      long long unfinished = 0;
      for (size_t l = 0; l < n; ++l) unfinished += finished(l) ? 0 : 1;
      if (unfinished == 0) { j0 += left; break; }
      const long long to_point = every - j0 % every;
      const int np = (int)(left < to_point ? left : to_point);
      const int n_waves = build();
      std::vector<long long> mgr0((size_t)np);
      std::vector<int> sched((size_t)np);
      dql::fill_schedule(cfg, j0, mgr0.data(), sched.data(), np);
      for (int w = 0; w < n_waves; ++w) fly_wave(w, j0, np, (const long long*)mgr0.data(), (const int*)sched.data());
      j0 += np; left -= np;
    }
  }
  return j0;
}

// dql_ensemble_run with recipes installed: everything of a recipe job's run but the wave, which is the driver's.  fly_wave(w, j0, np, mgr0, sched) reads
// wave_recipe[w], wave_level[w] and the lanes' learners worklist[64 w ..] as its kernel does
template <typename T> struct RecipeRun {
  RecipeJob& j;
  const Consts<T> k;
  const RecipeTables<T> tab;
  LearnerState<T> st;  // (at the config's level, with the config's quirks: k_init reads neither a recipe nor a level)
  const dql::LearnMem mem;
  LevelBooks books;
  std::vector<int> worklist, wave_recipe, wave_level;
  long long j0 = 0;
  explicit RecipeRun(RecipeJob& job)
      : j(job), k(j.cfg), tab(j.cfg, j.recipes), st(k, (size_t)j.n, j.seed, j.log_cap), mem(st.mem(j)), books((size_t)j.n, j.cfg.working_curriculum_step),
        worklist((size_t)dql::worklist_capacity_recipes(j.n, j.n_recipes)), wave_recipe(worklist.size() / dql::ADV_WAVE), wave_level(worklist.size() / dql::ADV_WAVE) {}
  template <typename FlyWave> void fly(FlyWave fly_wave) {
    const dql::AdvanceMem adv = books.mem();
    j0 = run_advancing(
        j.cfg, j.runs, j.n_runs, j.every, st.n,
        [&](long long at) {  // k_ens_advance_recipes: one thread per learner
          for (size_t l = 0; l < st.n; ++l) (void)dql::advance_learner_recipe(mem, adv, tab.rules.data(), j.n_recipes, j.recipe_of.data(), st.si.data(), (long long)l, at, DQL_CELLS_PER_LEVEL);
        },
        [&](size_t l) { return dql::learner_finished(st.frozen[l], books.level[l], st.promoted[l], tab.rules[(size_t)j.recipe_of[l]].rule); },
        [&] {
          return dql::build_worklist_recipes(st.frozen.data(), books.level.data(), j.recipe_of.data(), j.n, j.n_recipes, worklist.data(), wave_recipe.data(), wave_level.data(),
                                             (long long)worklist.size(), st.faults.data());
        },
        fly_wave);
  }
  int write(const char* path, const PersistentWindows* pw = nullptr) { return write_result(path, st, j, pw, &books, j0); }
};

}  // namespace emu
