// team_levels_emu.cpp — dql_ensemble_run in team curriculum mode, emulated on the CPU from the real device source: dql_team_levels.hpp's
// build_team_worklist and advance_team on top of dql_team.hpp's team_env_period and team_apply and dql_team_nstep.hpp's team_apply_nstep, team_window_load
// and team_window_store.
//
// The driver does what ens_run_advancing does for ens_run_team_levels (dql_team_levels.inc), through emu_learners.h's run_advancing: at an advance point every
// team takes advance_team's step (k_ens_advance_teams: one thread per team); then the live teams are regrouped by level (build_team_worklist, 64 / E team slots
// to a wave) and flown wave by wave, slot by slot, as k_learn_team_levels and k_learn_team_levels_nstep fly them — the wave's level from wave_level[w], a
// slot's team from the worklist (-1: a slot of inactive lanes), SimK::working, the level's MdpK and the level's schedules from that level, env e of team l
// being env l E + e.  A team's launch is team_emu's (nstep 0) or team_nstep_emu's (nstep >= 1): the two barriers of a period are program order here, the
// team's working windows are exactly [NSTEP_MAX][E] and poisoned before every launch of every team, the persistent ones exactly [NSTEP_MAX][L E], poisoned
// at the start, every element reached through a checked reference (exit status 3).  With nstep 0 the advance step gets no window lengths, as in the library
// before dql_ensemble_set_team_nstep allocated them.  Every array is exactly as long as the library allocates it, so the sanitized build sees any access
// beyond them.
//
//   team_levels_emu JOB OUT   run the calls described by JOB (see Job; tests/test_team_levels_host_emulation.py writes it), write OUT.
//                             Mode 1 is one call of build_team_worklist on the job's frozen[] and level[] with the job's capacity and teams per wave:
//                             OUT is then n_waves, the faults counted, the worklist [capacity] and wave_level [capacity / teams per wave].
#include "host_shim.h"

#include "emu_learners.h"
#include "dql_team.hpp"
#include "dql_team_nstep.hpp"
#include "dql_team_levels.hpp"

using namespace dql;

namespace {

// 48 words {cfg size, dtype, L, n_runs, runs[8], n_alpha, every, last_level, advance_exhausted, log_cap, then emu::JobLevels' words, has_tables, E, nstep,
// transfer_order, mode, worklist capacity and teams per wave (mode 1), 0 ...}, the seed, the config; then (mode 0) ratios[5], alpha, the eps tables, the tables,
// or (mode 1) frozen[L], level[L]
struct Job : emu::Tables {
  int dtype, n_runs, runs[8], n_alpha, every, log_cap, E, nstep, order, mode, per_wave;
  long long n, cap_slots;
  unsigned long long seed;
  dql_config cfg;
  AdvanceRule rule;
  emu::JobLevels levels;
  std::vector<double> alpha;
  std::vector<int> frozen, level;  // mode 1 only
  explicit Job(const char* path) {
    emu::JobFile f(path);
    int32_t hdr[48];
    int64_t s;
    f.read(hdr, 48); f.read(&s, 1);
    f.read_config(cfg, hdr[0]);
    dtype = hdr[1]; n = hdr[2]; n_runs = hdr[3];
    for (int k = 0; k < 8; ++k) runs[k] = hdr[4 + k];
    seed = (unsigned long long)s;
    n_alpha = hdr[12]; every = hdr[13]; rule.last_level = hdr[14]; rule.advance_exhausted = hdr[15]; log_cap = hdr[16];
    E = hdr[38]; nstep = hdr[39]; order = hdr[40]; mode = hdr[41]; cap_slots = hdr[42]; per_wave = hdr[43];
    if (n < 1 || (mode != 0 && mode != 1)) emu::bad_job();
    if (mode == 1) {  // (any capacity, any teams per wave, any levels: the faults are what is looked at)
      if (cap_slots < 0 || per_wave < 1) emu::bad_job();
      frozen.resize((size_t)n); level.resize((size_t)n);
      f.read(frozen); f.read(level);
      return;
    }
    const bool ok = emu::advancing_ok(cfg, runs, n_runs, every, log_cap) && emu::rule_ok(cfg, n_alpha, rule.last_level) && team_size_ok(E) && nstep >= 0 && nstep <= NSTEP_MAX &&
                    (order == RCP_ORDER_REFERENCE || order == RCP_ORDER_PAPER);
    if (!(levels.take(hdr + 17) && ok)) emu::bad_job();
    f.read(rule.ratios, ADV_MAX_LEVELS);
    alpha.resize((size_t)n_alpha);
    f.read(alpha);
    levels.read_eps(f);
    Tables::read(f, n, hdr[37]);
  }
};

int worklist_only(Job& j, const char* out_path) {
  std::vector<int> worklist((size_t)j.cap_slots, 0x7fffffff), wave_level((size_t)(j.cap_slots / j.per_wave), 0x7fffffff);
  unsigned long long faults = 0ull;
  const int32_t n_waves = build_team_worklist(j.frozen.data(), j.level.data(), j.n, j.per_wave, worklist.data(), wave_level.data(), j.cap_slots, &faults);
  emu::ResultFile f(out_path);
  f.put(&n_waves, 1); f.put(&faults, 1); f.put(worklist); f.put(wave_level);
  return f.close();
}

// dql_team_nstep.hpp's LdsTeamWindow on a working copy of exactly E columns: [slot][e], head [e], len [e] (team_nstep_emu.cpp's)
struct EmuTeamWindow {
  const int E;
  std::vector<uint16_t> key;
  std::vector<double> val;
  std::vector<int> head, len;
  explicit EmuTeamWindow(size_t E_) : E((int)E_), key((size_t)NSTEP_MAX * E_), val((size_t)NSTEP_MAX * E_), head(E_), len(E_) {}
  void poison() { emu::poison(key, val); emu::poison(head); emu::poison(len); }
  struct View {  // `first`: the column that env 0 of the view is
    emu::Checked<uint16_t> k; emu::Checked<double> v; emu::Checked<int> h, n; int E, first;
    long long at(int e, int slot) const {
      if (slot < 0 || slot >= NSTEP_MAX || e < 0 || first + e >= E) { std::fprintf(stderr, "INDEX VIOLATION: window slot %d of env %d + %d of a team of %d\n", slot, first, e, E); std::exit(3); }
      return (long long)slot * E + first + e;
    }
    uint16_t& key(int e, int slot) const { return k[at(e, slot)]; }
    double& val(int e, int slot) const { return v[at(e, slot)]; }
    int& head(int e) const { return h[(long long)first + e]; }
    int& len(int e) const { return n[(long long)first + e]; }
  };
  View view(size_t first) {
    return View{emu::checked(key, "the working keys"), emu::checked(val, "the working rewards"), emu::checked(head, "the working heads"), emu::checked(len, "the working lengths"), E, (int)first};
  }
};

template <typename T> int launch(Job& j, const char* out_path) {
  const size_t n = (size_t)j.n, E = (size_t)j.E;
  const int per_wave = ADV_WAVE / j.E;
  const emu::Consts<T> k(j.cfg);
  MdpK<T> mdpk5[ADV_MAX_LEVELS];
  emu::mdpk_per_level(j.cfg, mdpk5);
  const emu::LevelTables lt(j.levels);
  emu::LearnerState<T> st(k, n, j.seed, j.log_cap, E);  // (at the config's level)
  const long long n_envs = (long long)st.n_envs;
  const LearnMem mem = st.mem(j);
  emu::LevelBooks books(n, j.cfg.working_curriculum_step);
  const AdvanceMem adv = books.mem();
  emu::PersistentWindows pw(st.n_envs);  // (dql_ensemble_set_team_nstep; with nstep 0 nobody reads or writes them)
  const auto tm = pw.mem();
  int* pending_len = j.nstep ? pw.len.data() : nullptr;
  EmuTeamWindow work(E);
  std::vector<Env<T>> envs(E);
  std::vector<TeamRecord> rec(E);  // exactly E records
  const long long slots = team_worklist_capacity(j.n, per_wave);
  std::vector<int> worklist((size_t)slots), wave_level((size_t)(slots / per_wave));
  const long long j_end = emu::run_advancing(
      j.cfg, j.runs, j.n_runs, j.every, n,
      [&](long long j0) {
        for (size_t l = 0; l < n; ++l) (void)advance_team(mem, adv, j.rule, j.order, st.si.data(), pending_len, j.E, (long long)l, j0, DQL_CELLS_PER_LEVEL);
      },
      [&](size_t l) { return learner_finished(st.frozen[l], books.level[l], st.promoted[l], j.rule); },
      [&] { return build_team_worklist(st.frozen.data(), books.level.data(), j.n, per_wave, worklist.data(), wave_level.data(), slots, st.faults.data()); },
      [&](int w, long long j0, int np, const long long* mgr0, const int* sched) {
        const int lvl = wave_level[(size_t)w];
        if ((unsigned)lvl >= (unsigned)ADV_MAX_LEVELS) { st.faults[0] += 1ull; return; }
        const SimK<T> cl = k.simk(lvl, k.c.quirks);
        const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
        const LearnSched sc = learn_sched(j.alpha.data(), j.n_alpha, j.cfg.alpha_min, (const LevelSched DQL_CONST_AS*)&lt.lv[lvl]);
        const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk5[lvl];
        for (int slot = 0; slot < per_wave; ++slot) {
          const long long l = worklist[(size_t)w * (size_t)per_wave + (size_t)slot];
          if (l < 0 || l >= j.n || st.frozen[(size_t)l]) continue;  // an empty slot; a frozen team's lanes load nothing and store nothing
          const long long g0 = l * j.E;  // the team's first env
          TeamState ts = team_load(sc, mem, l);
          if (j.nstep) work.poison();
          const EmuTeamWindow::View team = work.view(0);
          for (size_t e = 0; e < E; ++e) {
            load_env(envs[e], st.sr.data(), st.si[(size_t)g0 + e], n_envs, g0 + (long long)e, cl);
            if (j.nstep) team_window_load(tm, n_envs, g0 + (long long)e, 0, j.nstep, work.view(e));  // the lane's own column
          }
          const double* qa = j.qa.data() + l * DQL_N_CELLS;
          const double* qb = j.qb.data() + l * DQL_N_CELLS;
          for (int q = 0; q < np && ts.live; ++q) {
            const uint32_t eps_thr = ts.eps_thr;  // one threshold for the period, whatever the apply makes of it meanwhile
            for (size_t e = 0; e < E; ++e)
              rec[e] = team_env_period<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, k.mdp_run, envs[e], qa, qb, eps_thr, j.seed, g0 + (long long)e, j0 + q, mgr0[q], sched[q], lc.kv);
            if (j.nstep) team_apply_nstep(sc, mem, cl.quirks, k.mdp_run.gamma, l, (const TeamRecord*)rec.data(), j.E, j.nstep, team, ts);
            else team_apply(sc, mem, cl.quirks, k.mdp_run.gamma, l, (const TeamRecord*)rec.data(), j.E, ts);
          }
          for (size_t e = 0; e < E; ++e) {
            store_env(envs[e], st.sr.data(), st.si.data(), n_envs, g0 + (long long)e, cl);
            if (j.nstep) team_window_store(tm, n_envs, g0 + (long long)e, 0, j.nstep, work.view(e));
          }
          team_store(ts, mem, l);
        }
      });
  return emu::write_result(out_path, st, j, &pw, &books, j_end);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: team_levels_emu JOB OUT\n"); return 2; }
  Job j(argv[1]);
  if (j.mode == 1) return worklist_only(j, argv[2]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
