// ML-KEM single-shot phase trace (tools only): the array and the marks, for the two path files whose
// kernels stamp them (mlkem_one.cuh, which holds qrk_dbg_ss_trace, and mlkem_kg.cuh; both are part of
// the translation unit mlkem.hip, so this is the array's one definition).
#pragma once
#include "mlkem_layout.cuh"

namespace qrk {
namespace mlkem {

// ------------------------------------------------------------ single-shot phase trace (tools only)
// -DQRK_SS_TRACE=1 (a tools/build_variant.sh build): the single-shot kernels stamp the 100 MHz
// wall clock at phase boundaries into g_ss_trace; qrk_dbg_ss_trace() copies it out.
#ifndef QRK_SS_TRACE
#define QRK_SS_TRACE 0
#endif
#if QRK_SS_TRACE
__device__ unsigned long long g_ss_trace[32];
#define SS_MARK(cond, i)                                      \
  do {                                                        \
    if (cond) g_ss_trace[i] = wall_clock64();                 \
  } while (0)
#define SS_CLK(cond, i)                                       \
  do {                                                        \
    if (cond) g_ss_trace[i] = clock64();                      \
  } while (0)
#else
#define SS_CLK(cond, i) \
  do {                  \
  } while (0)
#define SS_MARK(cond, i) \
  do {                   \
  } while (0)
#endif

}  // namespace mlkem
}  // namespace qrk
