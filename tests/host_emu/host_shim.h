// host_shim.h — the device names dql_device.hpp uses, defined for a plain host C++ build (x86-64, clang++) of that header.
//
// The five emulators (step_emu, rollout_emu, score_emu, learner_emu, advance_emu) run the kernels' device code on the CPU, one lane at a
// time, so that a sanitizer and explicit index checks can watch it; each includes this file first, then the device headers, then
// emu_common.h (what the drivers share: job and result files, the launch prologue, the state packing, the checked table).  Every
// definition here either restates an instruction exactly or is licensed by a check that the device code's own comments name:
//   __ballot(p)                     one lane per wave: p ? 1 : 0.  Each ballot in the header guards a wave-uniform fast path that is
//                                   documented as bit-identical to the per-lane path (det_atan2, kalman1d, the footprint tests), so
//                                   running it for single lanes tests those claims.
//   __builtin_amdgcn_sqrtf          the correctly rounded sqrtf: sqrt_()'s neighbour test then leaves it unchanged, which is the
//                                   result the library's exhaustive check (dql_diag_selftest_sqrt) holds the device to.
//   __builtin_amdgcn_rsqf           1 / sqrt(x) rounded to float: sqrt_pos() built on it equals sqrtf on every float in
//                                   [SQRT_POS_MIN, 838^2] (checked exhaustively on the CPU: 998 846 433 inputs, no difference), the
//                                   domain the rotor command clamps it to.
//   __builtin_amdgcn_fmed3f         v_med3_f32 as the gfx9 ISA pseudo-code defines it: the oracle's own restatement (dql_oracle.c
//                                   amd_max_f32 / clip3), signed-zero ties and NaN operands included.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#define __device__
#define __forceinline__ inline __attribute__((always_inline))

struct int4 { int x, y, z, w; };
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }

inline unsigned long long __ballot(bool p) { return p ? 1ull : 0ull; }

inline unsigned __float_as_uint(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
inline float __uint_as_float(unsigned u) { float x; std::memcpy(&x, &u, 4); return x; }
inline long long __double_as_longlong(double x) { long long u; std::memcpy(&u, &x, 8); return u; }
inline double __longlong_as_double(long long u) { double x; std::memcpy(&x, &u, 8); return x; }

namespace dql_emu {
inline float amd_max_f32(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == 0.0f && b == 0.0f) return (std::signbit(a) && std::signbit(b)) ? a : 0.0f;
  return a >= b ? a : b;
}
inline float amd_min_f32(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == 0.0f && b == 0.0f) return (std::signbit(a) || std::signbit(b)) ? -0.0f : a;
  return a <= b ? a : b;
}
inline float med3_f32(float a, float b, float c) {
  if (a != a || b != b || c != c) return amd_min_f32(amd_min_f32(a, b), c);
  const float mx = amd_max_f32(amd_max_f32(a, b), c);
  if (mx == a) return amd_max_f32(b, c);
  if (mx == b) return amd_max_f32(a, c);
  return amd_max_f32(a, b);
}
inline float sqrt_cr(float x) { return std::sqrt(x); }
inline float rsq(float x) { return (float)(1.0 / std::sqrt((double)x)); }
}  // namespace dql_emu

#define __builtin_amdgcn_sqrtf(x) dql_emu::sqrt_cr(x)
#define __builtin_amdgcn_rsqf(x) dql_emu::rsq(x)
#define __builtin_amdgcn_fmed3f(a, b, c) dql_emu::med3_f32((a), (b), (c))
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
