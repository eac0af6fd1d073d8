/*
 * fltx_typed_entry.h -- the __global__ entry points of fltx_decode_batch_typed (fltx_wlane_typed.h): the token beams of
 * fltx_wlane.h from the typed frames, a wave per frame; the float32 rows e for the utterances another engine decodes; the
 * back-trace kernels whose score passes gather the typed element with the frame's lse (the walk is the float32 kernels';
 * the word-piece engine's records are 16 + 16 bits).  FLTX_TYPED_ALL lists every instantiation once: fltx_api.cpp
 * declares them `extern template`, fltx_typed_kinst.cpp defines them -- an object of its own, compiled without packed
 * float32 instructions (the front end's float32 arithmetic decides the bits of a frame's lse), so that fltx_api.o keeps
 * the flags and the kernels it had.
 */
#pragma once
#include "fltx_kernel_entry.h"
#include "fltx_s2s.h"
#include "fltx_wlane_typed.h"

#ifndef FLTX_EMU
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(256) fltx_tokbeam_typed_kernel(WtParams Z) {
  __shared__ __attribute__((aligned(16))) WlFrontLds fltx_wt_front[4];
  wtTokBeamRows<DT, LOGITS>(Z, (char*)fltx_wt_front);
}
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(256) fltx_widen_rows_kernel(WtParams Z) {
  wtWidenRows<DT, LOGITS>(Z, nullptr);
}
template <int EM, bool LOGITS>
__global__ void __launch_bounds__(512) fltx_backtrace_typed_kernel(BacktraceParams P) {
  extern __shared__ __attribute__((aligned(16))) char fltx_btt_smem[];
  backtraceUtterance<EM, LOGITS>(P, fltx_btt_smem);
}
template <bool PW, int EM, bool LOGITS>
__global__ void __launch_bounds__(512, 4) fltx_backtrace_narrow_typed_kernel(BacktraceParams P) {
  extern __shared__ __attribute__((aligned(16))) char fltx_btnt_smem[];
  backtraceNarrow<uint32_t, PW, EM, LOGITS>(P, fltx_btnt_smem);
}
#define FLTX_TYPED_KERNELS(X, DT, LG)                              \
  X(fltx_tokbeam_typed_kernel<DT, LG>(WtParams))                   \
  X(fltx_widen_rows_kernel<DT, LG>(WtParams))                      \
  X(fltx_backtrace_typed_kernel<DT, LG>(BacktraceParams))          \
  X(fltx_backtrace_narrow_typed_kernel<true, DT, LG>(BacktraceParams)) \
  X(fltx_backtrace_narrow_typed_kernel<false, DT, LG>(BacktraceParams))
#define FLTX_TYPED_ALL(X)                                                                                  \
  FLTX_TYPED_KERNELS(X, kS2sDtF32, false) FLTX_TYPED_KERNELS(X, kS2sDtF32, true) FLTX_TYPED_KERNELS(X, kS2sDtF16, false) \
  FLTX_TYPED_KERNELS(X, kS2sDtF16, true) FLTX_TYPED_KERNELS(X, kS2sDtBf16, false) FLTX_TYPED_KERNELS(X, kS2sDtBf16, true)
#else
#define FLTX_TYPED_ALL(X)
#endif /* !FLTX_EMU */
