// Stand-in for the HIP runtime header when dql_device.hpp is compiled for the host (the drivers of this directory).  The device names the header
// uses (__device__, int4, __ballot, the amdgcn builtins) come from host_shim.h, which every driver includes first.  The header's inline-asm
// macros, defined just before it includes this file, are redefined here with their portable meaning: a register pin or a block marker
// is nothing the host needs (a compiler barrier at most), the opaque SGPR -> VGPR copy is a copy, and each three-address fma is the fma
// it spells (v_fmamk_f32 / v_fma_f32: d = x * k + y).
#pragma once
#undef DQL_ASM_PIN
#undef DQL_ASM_BLOCK
#undef DQL_ASM_VMOV
#undef DQL_ASM_FMA_LIT
#undef DQL_ASM_FMA_V
#undef DQL_ASM_FMA_S
#define DQL_ASM_PIN(...) do { } while (0)
#define DQL_ASM_BLOCK(text) asm volatile("" ::: "memory")
#define DQL_ASM_VMOV(dst, src) ((dst) = (src))
#define DQL_ASM_FMA_LIT(d, x, k, y) ((d) = fma_((x), (float)(k), (y)))
#define DQL_ASM_FMA_V(d, x, k, y) ((d) = fma_((x), (float)(k), (y)))
#define DQL_ASM_FMA_S(d, x, k, y) ((d) = fma_((x), (float)(k), (y)))
