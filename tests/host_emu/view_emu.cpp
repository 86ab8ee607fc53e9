// view_emu.cpp — one launch of k_env_view<T, R> (dql_view.inc), emulated on the CPU from the real device source (dql_view.hpp's env_view on dql_device.hpp).
//
// The driver does what the kernel does: a grid of ceil(n / 256) workgroups of 256 lanes, and for EVERY lane of it — those of the tail workgroup beyond the batch
// included — the real env_view with the lane's global index.  The state is the job's bytes as they are: Quad<T>[16][n] and int4[n], never interpreted here.  State
// and outputs are reached through checked references (exit status 3 outside them) exactly as long as the library's buffers: 16 n quads, n words, 2 n (float) or
// 4 n (double) 16-byte vectors of obs, n elements of every per-env output, one word of bad_actions.  Every output buffer is filled with a poison byte before the
// launch and written to the result file whole, whether it was asked for or not: an output the job's mask leaves out is handed over as a null reference, as the
// library hands over a NULL pointer, and must come back poisoned.
//
//   view_emu JOB OUT   run the launch described by JOB (see main; tests/test_view_host_emulation.py writes it), write OUT
#include "host_shim.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dql_device.hpp"
#include "dql_view.hpp"
#include "emu_common.h"

using namespace dql;

namespace {

constexpr unsigned char POISON = 0xA5;
constexpr int BLOCK = 256;  // VIEW_BLOCK of dql_view.inc

// a buffer as the device code's pointer: every element touched is bounds-checked; a null reference tests false and may not be touched at all
template <typename V> struct Ref {
  V* p; size_t n; const char* what;
  explicit operator bool() const { return p != nullptr; }
  V& operator[](size_t k) const {
    if (!p || k >= n) { std::fprintf(stderr, "INDEX VIOLATION: %s element %zu outside [0, %zu)\n", what, k, p ? n : (size_t)0); std::exit(3); }
    return p[k];
  }
};
template <typename R> struct HostOut {
  Ref<ViewVec<R>> obs;
  Ref<R> reward, cum;
  Ref<int32_t> idx_x, idx_y, step_count;
  Ref<uint8_t> done, was_reset;
  Ref<int8_t> code;
  Ref<unsigned long long> bad_actions;
};
template <typename V> std::vector<V> poisoned(size_t n) {
  std::vector<V> v(n);
  std::memset((void*)v.data(), POISON, n * sizeof(V));
  return v;
}
template <typename V> Ref<V> ref(std::vector<V>& v, bool asked, const char* what) { return Ref<V>{asked ? v.data() : nullptr, v.size(), what}; }

// output bits of the job's mask, in the order of dql_view's pointers
enum { M_OBS = 1, M_REWARD = 2, M_CUM = 4, M_IDX_X = 8, M_IDX_Y = 16, M_STEPS = 32, M_DONE = 64, M_WAS_RESET = 128, M_CODE = 256, M_BAD = 512 };

template <typename T, typename R> int launch(emu::JobFile& f, long long n, int mask, const char* out_path) {
  std::vector<Quad<T>> sr((size_t)NQ_REAL * (size_t)n);
  std::vector<int4> si((size_t)n);
  unsigned long long bad = 0;
  f.read(sr); f.read(si); f.read(&bad, 1);
  constexpr size_t NV = VIEW_OBS * sizeof(R) / 16;
  auto obs = poisoned<ViewVec<R>>(NV * (size_t)n);
  auto reward = poisoned<R>((size_t)n), cum = poisoned<R>((size_t)n);
  auto idx_x = poisoned<int32_t>((size_t)n), idx_y = poisoned<int32_t>((size_t)n), steps = poisoned<int32_t>((size_t)n);
  auto done = poisoned<uint8_t>((size_t)n), was_reset = poisoned<uint8_t>((size_t)n);
  auto code = poisoned<int8_t>((size_t)n);
  auto bad_out = poisoned<unsigned long long>(1);
  const Ref<const Quad<T>> srr{sr.data(), sr.size(), "state quad"};
  const Ref<const int4> sir{si.data(), si.size(), "state word"};
  const Ref<const unsigned long long> badr{&bad, 1, "bad-action counter"};
  const HostOut<R> o{ref(obs, mask & M_OBS, "obs vector"), ref(reward, mask & M_REWARD, "reward"), ref(cum, mask & M_CUM, "cumulative_reward"),
                     ref(idx_x, mask & M_IDX_X, "idx_x"), ref(idx_y, mask & M_IDX_Y, "idx_y"), ref(steps, mask & M_STEPS, "step_count"),
                     ref(done, mask & M_DONE, "done"), ref(was_reset, mask & M_WAS_RESET, "was_reset"), ref(code, mask & M_CODE, "code"),
                     ref(bad_out, mask & M_BAD, "bad_actions")};
  if (mask) {  // a view without outputs launches nothing
    const long long grid = (n + BLOCK - 1) / BLOCK;
    for (long long b = 0; b < grid; ++b)
      for (int t = 0; t < BLOCK; ++t) env_view<T, R>(srr, sir, badr, n, b * BLOCK + t, o);
  }
  emu::ResultFile r(out_path);
  r.put(obs); r.put(reward); r.put(cum); r.put(idx_x); r.put(idx_y); r.put(steps); r.put(done); r.put(was_reset); r.put(code); r.put(bad_out);
  return r.close();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: view_emu JOB OUT\n"); return 2; }
  emu::JobFile f(argv[1]);
  int32_t hdr[4];  // context dtype, real_dtype, output mask, 0
  int64_t n;
  f.read(hdr, 4); f.read(&n, 1);
  if (n < 1 || n > (1 << 20) || (hdr[0] != DQL_F32 && hdr[0] != DQL_F64) || (hdr[1] != DQL_F32 && hdr[1] != DQL_F64) || hdr[2] < 0 || hdr[2] > 1023 || hdr[3]) emu::bad_job();
  if (hdr[0] == DQL_F32) return hdr[1] == DQL_F32 ? launch<float, float>(f, n, hdr[2], argv[2]) : launch<float, double>(f, n, hdr[2], argv[2]);
  return hdr[1] == DQL_F32 ? launch<double, float>(f, n, hdr[2], argv[2]) : launch<double, double>(f, n, hdr[2], argv[2]);
}
