// Fused broadcast-FMA tail of a register factor step:
//   BcastFmaTail<FIRST, LAST>::run(a, s, x):  a[m] += bcast_m(s) * x  for m = FIRST..LAST
// (bcast_m: lane m of each 16-lane row, DPP row_newbcast), as v_fmac_f64 with a
// DPP source: one instruction per update instead of a v_mov_b64_dpp + v_fma_f64
// pair -- the compiler does not combine 64-bit DPP moves into VOP2.  One asm
// statement per call, so nothing is scheduled between the updates.  The
// leading s_nop 1 covers the VALU-write -> DPP-read hazard of the broadcast
// source; no register these blocks write is read by a DPP (compiler or asm)
// before compiler code rewrites it.  Bit for bit the products and sums of the
// two-instruction form.  An empty range (FIRST > LAST) is a no-op.
#pragma once

#include <hip/hip_runtime.h>

template <int FIRST, int LAST>
struct BcastFmaTail {
  static_assert(FIRST > LAST, "BcastFmaTail: declare this range below");
  static __device__ __forceinline__ void run(double (&)[LAST + 1], double, double) {}
};

// The asm text and the output operands of a[m], m = FIRST..LAST, as chains
// DPP_FMAC_{I,O}<LAST>_<FIRST> = (m = FIRST) then the chain from FIRST + 1.
#define DPP_FMAC_I(m) \
  "v_fmac_f64_dpp %[v" #m "], %[s], %[x] row_newbcast:" #m " row_mask:0xf bank_mask:0xf\n"
#define DPP_FMAC_O(m) [v##m] "+v"(a[m])

#define DPP_FMAC_I8_8 DPP_FMAC_I(8)
#define DPP_FMAC_I8_7 DPP_FMAC_I(7) DPP_FMAC_I8_8
#define DPP_FMAC_I8_6 DPP_FMAC_I(6) DPP_FMAC_I8_7
#define DPP_FMAC_I8_5 DPP_FMAC_I(5) DPP_FMAC_I8_6
#define DPP_FMAC_I8_4 DPP_FMAC_I(4) DPP_FMAC_I8_5
#define DPP_FMAC_I8_3 DPP_FMAC_I(3) DPP_FMAC_I8_4
#define DPP_FMAC_I8_2 DPP_FMAC_I(2) DPP_FMAC_I8_3
#define DPP_FMAC_O8_8 DPP_FMAC_O(8)
#define DPP_FMAC_O8_7 DPP_FMAC_O(7), DPP_FMAC_O8_8
#define DPP_FMAC_O8_6 DPP_FMAC_O(6), DPP_FMAC_O8_7
#define DPP_FMAC_O8_5 DPP_FMAC_O(5), DPP_FMAC_O8_6
#define DPP_FMAC_O8_4 DPP_FMAC_O(4), DPP_FMAC_O8_5
#define DPP_FMAC_O8_3 DPP_FMAC_O(3), DPP_FMAC_O8_4
#define DPP_FMAC_O8_2 DPP_FMAC_O(2), DPP_FMAC_O8_3

#define DPP_FMAC_I15_15 DPP_FMAC_I(15)
#define DPP_FMAC_I15_14 DPP_FMAC_I(14) DPP_FMAC_I15_15
#define DPP_FMAC_I15_13 DPP_FMAC_I(13) DPP_FMAC_I15_14
#define DPP_FMAC_I15_12 DPP_FMAC_I(12) DPP_FMAC_I15_13
#define DPP_FMAC_I15_11 DPP_FMAC_I(11) DPP_FMAC_I15_12
#define DPP_FMAC_I15_10 DPP_FMAC_I(10) DPP_FMAC_I15_11
#define DPP_FMAC_I15_9 DPP_FMAC_I(9) DPP_FMAC_I15_10
#define DPP_FMAC_I15_8 DPP_FMAC_I(8) DPP_FMAC_I15_9
#define DPP_FMAC_I15_7 DPP_FMAC_I(7) DPP_FMAC_I15_8
#define DPP_FMAC_I15_6 DPP_FMAC_I(6) DPP_FMAC_I15_7
#define DPP_FMAC_I15_5 DPP_FMAC_I(5) DPP_FMAC_I15_6
#define DPP_FMAC_I15_4 DPP_FMAC_I(4) DPP_FMAC_I15_5
#define DPP_FMAC_I15_3 DPP_FMAC_I(3) DPP_FMAC_I15_4
#define DPP_FMAC_I15_2 DPP_FMAC_I(2) DPP_FMAC_I15_3
#define DPP_FMAC_I15_1 DPP_FMAC_I(1) DPP_FMAC_I15_2
#define DPP_FMAC_O15_15 DPP_FMAC_O(15)
#define DPP_FMAC_O15_14 DPP_FMAC_O(14), DPP_FMAC_O15_15
#define DPP_FMAC_O15_13 DPP_FMAC_O(13), DPP_FMAC_O15_14
#define DPP_FMAC_O15_12 DPP_FMAC_O(12), DPP_FMAC_O15_13
#define DPP_FMAC_O15_11 DPP_FMAC_O(11), DPP_FMAC_O15_12
#define DPP_FMAC_O15_10 DPP_FMAC_O(10), DPP_FMAC_O15_11
#define DPP_FMAC_O15_9 DPP_FMAC_O(9), DPP_FMAC_O15_10
#define DPP_FMAC_O15_8 DPP_FMAC_O(8), DPP_FMAC_O15_9
#define DPP_FMAC_O15_7 DPP_FMAC_O(7), DPP_FMAC_O15_8
#define DPP_FMAC_O15_6 DPP_FMAC_O(6), DPP_FMAC_O15_7
#define DPP_FMAC_O15_5 DPP_FMAC_O(5), DPP_FMAC_O15_6
#define DPP_FMAC_O15_4 DPP_FMAC_O(4), DPP_FMAC_O15_5
#define DPP_FMAC_O15_3 DPP_FMAC_O(3), DPP_FMAC_O15_4
#define DPP_FMAC_O15_2 DPP_FMAC_O(2), DPP_FMAC_O15_3
#define DPP_FMAC_O15_1 DPP_FMAC_O(1), DPP_FMAC_O15_2

#define DPP_FMAC_TAIL(FIRST, LAST)                                                         \
  template <>                                                                              \
  struct BcastFmaTail<FIRST, LAST> {                                                       \
    static __device__ __forceinline__ void run(double (&a)[LAST + 1], double s, double x) { \
      asm("s_nop 1\n" DPP_FMAC_I##LAST##_##FIRST                                           \
          : DPP_FMAC_O##LAST##_##FIRST                                                     \
          : [s] "v"(s), [x] "v"(x));                                                       \
    }                                                                                      \
  };
// a 9-wide panel (k_solve_blk): rows FIRST..8
DPP_FMAC_TAIL(2, 8) DPP_FMAC_TAIL(3, 8) DPP_FMAC_TAIL(4, 8) DPP_FMAC_TAIL(5, 8)
DPP_FMAC_TAIL(6, 8) DPP_FMAC_TAIL(7, 8) DPP_FMAC_TAIL(8, 8)
// a 16x16 diagonal block (blk_factor_w0): rows FIRST..15
DPP_FMAC_TAIL(1, 15) DPP_FMAC_TAIL(2, 15) DPP_FMAC_TAIL(3, 15) DPP_FMAC_TAIL(4, 15)
DPP_FMAC_TAIL(5, 15) DPP_FMAC_TAIL(6, 15) DPP_FMAC_TAIL(7, 15) DPP_FMAC_TAIL(8, 15)
DPP_FMAC_TAIL(9, 15) DPP_FMAC_TAIL(10, 15) DPP_FMAC_TAIL(11, 15) DPP_FMAC_TAIL(12, 15)
DPP_FMAC_TAIL(13, 15) DPP_FMAC_TAIL(14, 15) DPP_FMAC_TAIL(15, 15)
#undef DPP_FMAC_TAIL
// The DPP_FMAC_I* / DPP_FMAC_O* chain macros stay defined: the DPP_FMAC_
// prefix belongs to this header, and 46 #undef lines would be half of it.
