// advance_emu.cpp — dql_ensemble_run in curriculum mode, emulated on the CPU from the real device source: dql_advance.hpp's
// build_worklist and advance_learner on top of dql_learner.hpp's learner_periods.
//
// The driver does what ens_run_advancing does for ens_run_levels (dql_ensemble.inc), through emu_learners.h's run_advancing: at an advance point every learner
// takes advance_learner's step (k_ens_advance: one thread per learner); then the live learners are regrouped by level (build_worklist) and flown wave by wave,
// lane by lane, as k_learn_levels flies them — the wave's level from wave_level[w], the lane's learner from the worklist (-1: an inactive lane), SimK::working,
// the level's MdpK and the level's schedules from that level.  A lane runs alone: __ballot(p) is p (host_shim.h).  Every array is exactly as long as the library
// allocates it, so the sanitized build sees any access beyond them.  The job's layout is this driver's own (one rule and one set of level schedules in the
// header); its clauses, tables and level schedules are read with emu_learners.h's pieces.
//
//   advance_emu JOB OUT   run the calls described by JOB (see Job; tests/test_advance_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include "emu_learners.h"

using namespace dql;

namespace {

// 40 words {cfg size, dtype, L, n_runs, runs[8], n_alpha, every, last_level, advance_exhausted, log_cap, then emu::JobLevels' words, has_tables, 0 ...}, the seed,
// the config, ratios[5], alpha, the eps tables, the tables
struct Job : emu::Tables {
  int dtype, n_runs, runs[8], n_alpha, every, log_cap;
  long long n;
  unsigned long long seed;
  dql_config cfg;
  AdvanceRule rule;
  emu::JobLevels levels;
  std::vector<double> alpha;
  explicit Job(const char* path) {
    emu::JobFile f(path);
    int32_t hdr[40];
    int64_t s;
    f.read(hdr, 40); f.read(&s, 1);
    f.read_config(cfg, hdr[0]);
    dtype = hdr[1]; n = hdr[2]; n_runs = hdr[3];
    for (int k = 0; k < 8; ++k) runs[k] = hdr[4 + k];
    seed = (unsigned long long)s;
    n_alpha = hdr[12]; every = hdr[13]; rule.last_level = hdr[14]; rule.advance_exhausted = hdr[15]; log_cap = hdr[16];
    const bool ok = n >= 1 && emu::advancing_ok(cfg, runs, n_runs, every, log_cap) && emu::rule_ok(cfg, n_alpha, rule.last_level);
    if (!(levels.take(hdr + 17) && ok)) emu::bad_job();
    f.read(rule.ratios, ADV_MAX_LEVELS);
    alpha.resize((size_t)n_alpha);
    f.read(alpha);
    levels.read_eps(f);
    Tables::read(f, n, hdr[37]);
  }
};

template <typename T> int launch(Job& j, const char* out_path) {
  const size_t n = (size_t)j.n;
  const emu::Consts<T> k(j.cfg);
  MdpK<T> mdpk5[ADV_MAX_LEVELS];
  emu::mdpk_per_level(j.cfg, mdpk5);
  const emu::LevelTables lt(j.levels);
  emu::LearnerState<T> st(k, n, j.seed, j.log_cap);  // (at the config's level)
  const LearnMem mem = st.mem(j);
  emu::LevelBooks books(n, j.cfg.working_curriculum_step);
  const AdvanceMem adv = books.mem();
  const long long slots = worklist_capacity(j.n);
  std::vector<int> worklist((size_t)slots), wave_level((size_t)(slots / ADV_WAVE));
  const long long j_end = emu::run_advancing(
      j.cfg, j.runs, j.n_runs, j.every, n,
      [&](long long j0) { for (size_t l = 0; l < n; ++l) (void)advance_learner(mem, adv, j.rule, st.si.data(), (long long)l, j0, DQL_CELLS_PER_LEVEL); },
      [&](size_t l) { return learner_finished(st.frozen[l], books.level[l], st.promoted[l], j.rule); },
      [&] { return build_worklist(st.frozen.data(), books.level.data(), j.n, worklist.data(), wave_level.data(), slots, st.faults.data()); },
      [&](int w, long long j0, int np, const long long* mgr0, const int* sched) {
        const int lvl = wave_level[(size_t)w];
        if ((unsigned)lvl >= (unsigned)ADV_MAX_LEVELS) { st.faults[0] += 1ull; return; }
        const SimK<T> cl = k.simk(lvl, k.c.quirks);
        const emu::Launch<T, TICK_PLAIN> lc(cl, j.seed);
        const LearnSched sc = learn_sched(j.alpha.data(), j.n_alpha, j.cfg.alpha_min, (const LevelSched DQL_CONST_AS*)&lt.lv[lvl]);
        const MdpK<T> DQL_CONST_AS* mdp = (const MdpK<T> DQL_CONST_AS*)&mdpk5[lvl];
        for (int lane = 0; lane < ADV_WAVE; ++lane) {
          const long long l = worklist[(size_t)w * ADV_WAVE + (size_t)lane];
          learner_periods<TICK_PLAIN, X_ONLY>(cl, lc.cfgk, lc.tc, mdp, k.mdp_run, sc, mem, st.sr.data(), st.si.data(), j.seed, l, l >= 0 && l < j.n, j0, np, mgr0, sched, lc.kv);
        }
      });
  return emu::write_result(out_path, st, j, nullptr, &books, j_end);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: advance_emu JOB OUT\n"); return 2; }
  Job j(argv[1]);
  return j.dtype == DQL_F64 ? launch<double>(j, argv[2]) : launch<float>(j, argv[2]);
}
