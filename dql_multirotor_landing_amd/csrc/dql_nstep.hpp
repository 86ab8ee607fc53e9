// dql_nstep.hpp — the sequential learner of dql_learner.hpp with the uncorrected n-step Double-Q return as its target, 1 <= n <= DQL_NSTEP_MAX (DESIGN.md
// section 22).
//
// This file owns the pending windows of the whole learner family: the entry's packing, the ring, nstep_update (the n-step update of
// one cell, shared with dql_team_nstep.hpp) and window_load / window_store (persistent window <-> working copy of one env, whoever's env it is).
//
// learner_periods_nstep is the per-lane body of k_learn_nstep (dql_nstep.inc) and of its host emulation (tests/host_emu/nstep_emu.cpp).  Everything but the
// update is learner_periods' and comes from dql_learner.hpp: the period schedule, the action rule, reset periods, the books (counters, the episode log, the
// promotion ring, the freeze rules), load_env / store_env.  The update works on the lane's PENDING WINDOW: at most n entries (cell, coin, reward), one per
// decision of the current episode, oldest first.
//
// After a decision that ended in state s' (both tables' row of s' read once, before the period's first write: StepOut::next):
//   1. the decision's entry is appended;
//   2. if the period ended the episode, every entry is updated, oldest first, and the window emptied; else if the window holds n entries the oldest is
//      updated and removed; else nothing is updated.
// The update of the entry at position k of a window of m entries: sel_b = Double Q-learning and the ENTRY's coin; best = the valuing table's element of the
// row of s' at the arg-max of the selecting table's row (learner_best, learner_update's table assignment); g = best * mask, then for i = m - 1 down to k:
// g = r_i + (gamma * g) (returns_step: two roundings); alpha at the cell's pre-increment count; q_new = q + alpha * (g - q).  At n = 1 this is learner_update
// bit for bit (mask is 0 or 1, so gamma * (best * mask) == (gamma * best) * mask for finite values).
//
// How the window is reached is a template parameter.  Win: the launch's working copy, win.key(slot) / win.val(slot) with slot in [0, n) (the kernel's is LDS
// laid out [slot][lane]); NMem: where it persists between launches, arrays [DQL_NSTEP_MAX][L] and len[L].  key: the cell in bits 0..14 (NSTEP_BAD_CELL for
// a cell outside the tables, which the update then counts and drops), the coin in bit 15.  val: the reward widened to double — and, during a flush, the
// entry's return, which takes the reward's place once no older entry needs it (the window is emptied right after).  The window is a ring: the entry at
// position i sits in slot (head + i) mod n.  Never a per-lane array indexed at run time: that would be scratch.
//
// Every loop is bounded by LEARN_MAX_PERIODS or by n on every path.  Include after dql_learner.hpp and dql_returns.hpp.
#pragma once
#include "dql_learner.hpp"
#include "dql_returns.hpp"

namespace dql {

constexpr int NSTEP_MAX = 16;  // include/dql.h DQL_NSTEP_MAX
constexpr uint16_t NSTEP_COIN = 0x8000u, NSTEP_BAD_CELL = 0x7fffu;

// where the windows persist between launches (KeyPtr: uint16_t[NSTEP_MAX][n], ValPtr: double[NSTEP_MAX][n], LenPtr: int[n]), position order: entry i of
// learner l at [i * n + l], i < len[l]
template <typename KeyPtr, typename ValPtr, typename LenPtr> struct NstepMem { KeyPtr key; ValPtr val; LenPtr len; };

DQL_DEV uint16_t nstep_pack(int sa, bool coin) {
  const uint16_t cell = (unsigned)sa < (unsigned)DQL_N_CELLS ? (uint16_t)sa : NSTEP_BAD_CELL;
  return (uint16_t)(cell | (coin ? NSTEP_COIN : 0));
}
DQL_DEV bool nstep_coin(uint16_t key) { return (key & NSTEP_COIN) != 0; }  // (never set under B1/B2: StepOut::cell carries the coin under Double Q-learning only)
DQL_DEV int nstep_cell(uint16_t key) { return key & (NSTEP_COIN - 1); }
// the window's capacity a launch works with
DQL_DEV int nstep_clamp(int nstep) { return nstep < 1 ? 1 : (nstep > NSTEP_MAX ? NSTEP_MAX : nstep); }
// the length of a window that persists: never full, the period that fills it takes its oldest entry out
DQL_DEV int nstep_len(int m, int ns) { return m < 0 ? 0 : (m > ns - 1 ? ns - 1 : m); }
// ... and the slot of its oldest entry, read back from memory another lane wrote
DQL_DEV int nstep_head(int head, int ns) { return (unsigned)head < (unsigned)ns ? head : 0; }
// position -> slot of a ring of n slots whose oldest entry sits in slot head (head < n, pos <= n)
DQL_DEV int nstep_slot(int head, int pos, int n) { const int s = head + pos; return s >= n ? s - n : s; }

// The n-step update of the cell of one entry towards its return g, on the table the entry's own coin names (sel_b): alpha at the cell's pre-increment count
// (learner_alpha), q_new = q + alpha * (g - q).  Returns false (and writes nothing) for a cell outside the tables.
DQL_DEV bool nstep_update(double* qa, double* qb, double* count, const LearnSched& sc, uint16_t key, double g, double& q_new, bool& sel_b) {
  sel_b = nstep_coin(key);
  const int sa = nstep_cell(key);
  if (sa >= DQL_N_CELLS) return false;
  const double cnt = count[sa];
  const double alpha = learner_alpha(sc, cnt);
  count[sa] = cnt + 1.0;
  double* qsel = sel_b ? qb : qa;
  const double q = qsel[sa];
  const double loss = alpha * (g - q);
  q_new = q + loss;
  qsel[sa] = q_new;
  return true;
}

// ---- persistent window <-> working copy ----
// nm: the persistent arrays over `stride` columns, of which this is column i; col: the same env's column of the working copy, key(slot) / val(slot).  The load
// leaves the m entries in slots 0 .. m - 1 (head 0); the store takes the ring (head, m) back into position order.  The length itself (nm.len, clamped by
// nstep_len) is read and written by the caller, beside its other loads and stores: with m = 0 both are no-ops and touch no address, so a lane that loaded
// nothing calls them outside its branch, where the compiler keeps the loops out of the divergent code (section 26: inside it k_learn_nstep lost 5 %).
template <typename NMem, typename Col>
DQL_DEV void window_load(const NMem& nm, long long stride, long long i, int ns, int m, Col col) {
  for (int k = 0; k < ns; ++k)
    if (k < m) { col.key(k) = nm.key[(long long)k * stride + i]; col.val(k) = nm.val[(long long)k * stride + i]; }
}
template <typename NMem, typename Col>
DQL_DEV void window_store(const NMem& nm, long long stride, long long i, int ns, Col col, int head, int m) {
  for (int k = 0; k < ns; ++k)
    if (k < m) {
      const int s = nstep_slot(head, k, ns);
      nm.key[(long long)k * stride + i] = col.key(s); nm.val[(long long)k * stride + i] = col.val(s);
    }
}

// the arguments of learner_periods, then nstep: the window's capacity n (wave-uniform); win / nm: see above
template <int TICK, int XMODE, typename T, typename MgrPtr, typename SchedPtr, typename Win, typename NMem>
DQL_DEV void learner_periods_nstep(const SimK<T>& c, const SimK<T>& cfgk, const TickConsts<TICK, T>& tc, const MdpK<T> DQL_CONST_AS* mdp, const MdpRun<T>& mr,
                                   const LearnSched& sc, const LearnMem& mem, Quad<T>* sr, int4* si, uint64_t seed, long long l, bool active, long long j0,
                                   int n_periods, MgrPtr mgr0, SchedPtr sched, const uint32_t* kv, int nstep, Win win, const NMem& nm) {
  const long long lz = active ? l : 0;
  double* qa = mem.qa + lz * DQL_N_CELLS;
  double* qb = mem.qb + lz * DQL_N_CELLS;
  double* count = mem.count + lz * DQL_N_CELLS;
  const int ns = nstep_clamp(nstep);
  const bool dbl = !(c.quirks & DQL_Q_UPDATE_TABLE_A_ONLY);
  Env<T> e = Env<T>{};
  QRow qx{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  LearnerBooks t = LearnerBooks{};
  int head = 0, m = 0;  // the window: the slot of its oldest entry, its length
  t.live = active && mem.frozen[lz] == 0;
  const bool loaded = t.live;
  if (loaded) {
    load_env(e, sr, si[l], mem.n, l, c);
    // the row of the state the env is in, from the tables as they stand (a reset period does not use it)
    qx = load_qrow((const double*)qa, (const double*)qb, e.idx_x < 0 ? 0 : e.idx_x);
    t = books_load(sc, mem, l);
    m = nstep_len(nm.len[l], ns);
  }
  window_load(nm, mem.n, l, ns, m, win);  // (m = 0 on a lane that loaded nothing)
  const int np = n_periods < LEARN_MAX_PERIODS ? n_periods : LEARN_MAX_PERIODS;
  for (int p = 0; p < np; ++p) {
    int n_upd = 0;      // entries this lane updates this period, from position 0 on
    bool flush = false;
    double ga = 0.0, gb = 0.0;  // the return by the coin: the bootstrap first, then the chains through the rewards
    uint16_t key_new = 0;       // the decision's entry, also kept in registers: the update of the newest entry (all of n = 1) reads no LDS
    double val_new = 0.0;
    // the oldest entry's key, asked for before the flight: a full window's update begins with it
    uint16_t key_old = 0;
    if (t.live && ns > 1 && m > 0) key_old = win.key(head);
    if (t.live) {
      const int prev_p = e.bin_p;
      const StepOut o = agent_period<TICK, XMODE>(cfgk, tc, mdp, mr, e, qx, (const double*)qa, (const double*)qb, MODE_TRAIN, t.eps_thr, 2, seed, (uint32_t)l,
                                                  j0 + p, mgr0[p], sched[p], kv);
      qx = o.next;
      if (o.decision) {
        ++t.decisions;
        const bool coin = o.cell >= DQL_N_CELLS;  // the table the kernel's TD target picked: the coin under Double Q-learning, never set under B1/B2
        const int sa = coin ? o.cell - DQL_N_CELLS : o.cell;
        const int tail = nstep_slot(head, m, ns);  // m < ns here: a full window gave up its oldest entry in the period that filled it
        key_new = nstep_pack(sa, coin); val_new = (double)e.reward;
        if (ns > 1) { win.key(tail) = key_new; win.val(tail) = val_new; }
        ++m;
        const int mask = (c.quirks & DQL_Q_BOOTSTRAP_ON_POS_CHANGE) ? (prev_p != e.bin_p) : !o.done;
        // both coins' bootstrap from the row of s' as it was read, before any write of this period
        ga = learner_best(o.next, dbl, false) * (double)mask;
        gb = learner_best(o.next, dbl, true) * (double)mask;
        flush = o.done != 0;
        n_upd = flush ? m : (m == ns ? 1 : 0);
      }
    }
    if (__ballot(n_upd > 0) != 0ull) {
      // backward: both coins' chains through the rewards, newest first.  A flush leaves each entry's return (by its own coin) in the reward's place.
      if (ns == 1) {
        ga = returns_step(val_new, mr.gamma, ga);
        gb = returns_step(val_new, mr.gamma, gb);
      } else {
        const bool any_flush = __ballot(flush) != 0ull;
        // four positions at a time, so that their LDS reads travel together; a position at or beyond m is read (its slot lies inside the NSTEP_MAX slots) and not used
        for (int i0 = (ns - 1) & ~3; i0 >= 0; i0 -= 4) {
          int s[4]; double r[4]; uint16_t kk[4] = {0, 0, 0, 0};
#pragma unroll
          for (int u = 0; u < 4; ++u) { s[u] = nstep_slot(head, i0 + u, ns); r[u] = win.val(s[u]); }
          if (any_flush) {
#pragma unroll
            for (int u = 0; u < 4; ++u) kk[u] = win.key(s[u]);
          }
#pragma unroll
          for (int u = 3; u >= 0; --u) {
            const bool on = n_upd > 0 && i0 + u < m;
            const double na = returns_step(r[u], mr.gamma, ga), nb = returns_step(r[u], mr.gamma, gb);
            ga = on ? na : ga; gb = on ? nb : gb;
            if (any_flush) { if (on && flush) win.val(s[u]) = (kk[u] & NSTEP_COIN) ? gb : ga; }
          }
        }
      }
      // forward: the updates, oldest first
      for (int k = 0; k < ns; ++k) {
        if (__ballot(k < n_upd) == 0ull) break;
        if (k < n_upd) {
          const int s = nstep_slot(head, k, ns);
          const bool newest = k == m - 1;
          uint16_t key = newest ? key_new : key_old;
          if (!newest && k > 0) key = win.key(s);
          double g = nstep_coin(key) ? gb : ga;  // a full window's single update, and a flush of one entry
          if (flush && ns > 1) g = win.val(s);
          double q_new; bool sel_b;
          if (nstep_update(qa, qb, count, sc, key, g, q_new, sel_b)) {
            // a write to the row of the state the env is in now changes the carried row, whichever entry made it
            qrow_patch(qx, e.idx_x, nstep_cell(key), sel_b, q_new);
          } else {
            mem.faults[0] += 1ull;  // never taken unless a bug: a plain (racy) count is enough to make the tests fail
          }
        }
      }
      if (n_upd > 0) {
        if (flush) { head = 0; m = 0; }
        else { head = nstep_slot(head, 1, ns); --m; }
      }
    }
    if (t.live && flush) {
      const int ok = books_episode(t, mem, l, e.code, e.step_count);
      if (books_ring_push(t, sc, ok)) t.live = false;
      t.eps_thr = eps_of_episode(sc, t.lvl_eps);
    }
    if (__ballot(t.live) == 0ull) break;
  }
  if (loaded) {
    store_env(e, sr, si, mem.n, l, c);
    books_store(t, mem, l);
    nm.len[l] = m;
  }
  window_store(nm, mem.n, l, ns, win, head, m);  // (m = 0 on a lane that loaded nothing)
}

}  // namespace dql
