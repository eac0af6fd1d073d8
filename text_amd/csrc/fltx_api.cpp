/*
 * fltx_api.cpp -- host side of the C ABI declared in include/fltx.h:
 * HBM allocation and layout, table flattening (n-gram LM, trie), kernel
 * launches, result retrieval.  Compiled by hipcc (-x hip) into
 * text_amd/lib/libfltx.so together with the kernels of fltx_kernels.h.
 *
 * There is no CPU decode path in this file: every decode launches the HIP
 * kernels and fails with FLTX_ERR_HIP if that is impossible.  (The FLTX_EMU
 * branches below exist only for tests/emu/libfltx_emu.so, a host-thread
 * emulation used to debug kernel logic; see tests/emu/hip_emu.h.)
 */
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <limits>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <atomic>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "fltx.h"
#include "fltx_kernel_entry.h"
#include "fltx_engines.h"
#include "fltx_s2s.h"
#include "fltx_s2s_lex.h"
#include "fltx_ctc_rows.h"
#include "fltx_ctc_rows_typed.h"
#include "fltx_ctc_rows_lex.h"
#include "fltx_ctc_rows_stream.h"
#include "fltx_transcript.h"
#include "fltx_stream_partials.h"
#include "fltx_stream_finish.h"
#include "fltx_ctc_rows_plan.h"

using namespace fltx;

/* Streams on the optimistic (LDS-sized) geometry: the parked beam of every stream is saved before a chunk
 * and put back for the streams whose chunk has to be decoded again on the general path (dir 1, map). */
struct SnapParams {
  int32_t K, dir;
  const int32_t* map; /* utterances to restore, null = all */
  double *gScore, *gAm, *gLm;
  float* gLexMax;
  uint32_t *gState, *gSPar, *gLex, *gTokPb;
  int32_t* gSEdge;
  int32_t *uttNBeam, *uttFrame, *uttTotal, *uttStatus;
  char* snap;
  int64_t B;
};
template <class T>
FLTX_HD void snapMove(int dir, T* live, char* snap, size_t& off, int64_t B, int32_t K, int b, int i) {
  T* s = (T*)(snap + off) + (size_t)b * K + i;
  T* l = live + (size_t)b * K + i;
  if (dir) {
    *l = *s;
  } else {
    *s = *l;
  }
  off += sizeof(T) * (size_t)B * K;
}
FLTX_HD void snapUtterance(const SnapParams& Q, int b, int i0, int step) {
  for (int i = i0; i < Q.K; i += step) {
    size_t off = 0;
    snapMove(Q.dir, Q.gScore, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gAm, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gLm, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gLexMax, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gState, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gSPar, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gLex, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gTokPb, Q.snap, off, Q.B, Q.K, b, i);
    snapMove(Q.dir, Q.gSEdge, Q.snap, off, Q.B, Q.K, b, i);
  }
  if (i0 == 0) {
    int32_t* u = (int32_t*)(Q.snap + (size_t)Q.B * Q.K * (3 * 8 + 6 * 4)) + (size_t)b * 4;
    int32_t* live[4] = {Q.uttNBeam, Q.uttFrame, Q.uttTotal, Q.uttStatus};
    for (int k = 0; k < 4; ++k) {
      if (Q.dir) {
        live[k][b] = u[k];
      } else {
        u[k] = live[k][b];
      }
    }
  }
}
#ifndef FLTX_EMU
#define FLTX_INST(...) extern template __global__ void __VA_ARGS__(DecodeParams);
#include "fltx_instances.h"
#undef FLTX_INST
/* the front end of fltx_wlane.h: the token beam of every row of the batch, one wave per row */
__global__ void __launch_bounds__(256) fltx_tokbeam_kernel(DecodeParams P) {
  extern __shared__ __attribute__((aligned(16))) char fltx_tb_smem[];
  wlTokBeamRows(P, fltx_tb_smem);
}
/* streams: LM-state ids nothing can meet again go back to the utterance's free list (compactStates) */
__global__ void __launch_bounds__(1024) fltx_compact_states_kernel(CompactParams Q) {
  extern __shared__ __attribute__((aligned(16))) char fltx_cs_smem[];
  compactStates(Q, fltx_cs_smem);
}
/* host LM: the (LM state, index) questions of the next frame, one workgroup per utterance (hostLmQuestions) */
__global__ void __launch_bounds__(256) fltx_hostlm_questions_kernel(DecodeParams P) {
  extern __shared__ __attribute__((aligned(16))) char fltx_hq_smem[];
  hostLmQuestions(P, fltx_hq_smem);
}
__global__ void __launch_bounds__(512) fltx_backtrace_kernel(BacktraceParams P) {
  extern __shared__ __attribute__((aligned(16))) char fltx_bt_smem[];
  backtraceUtterance(P, fltx_bt_smem);
}
/* packed records narrowed into LDS, the token tile resident (backtraceNarrow): 8 + 8 and 16 + 16 bits; PW = every wave
 * walks a stretch of each chunk from every slot and the paths are composed (K <= 64), else one walk per hypothesis */
template <typename RT, bool PW>
__global__ void __launch_bounds__(512, 4) fltx_backtrace_narrow_kernel(BacktraceParams P) {
  extern __shared__ __attribute__((aligned(16))) char fltx_btn_smem[];
  backtraceNarrow<RT, PW>(P, fltx_btn_smem);
}
__global__ void __launch_bounds__(64) fltx_snapshot_kernel(SnapParams Q) {
  const int b = Q.map ? Q.map[blockIdx.x] : (int)blockIdx.x;
  snapUtterance(Q, b, (int)threadIdx.x, 64);
}
/* fltx_result_fetch_batch_compact: the rows that exist, tokens narrowed to bytes, packed back to back */
struct PackParams {
  const int32_t* tokens;
  const int32_t* words; /* null: lexicon-free */
  const int64_t* srcOff;
  const int64_t* dstOff;
  const int32_t* count; /* n_hyp[b] * length[b] */
  uint8_t* tok8;
  int32_t* wordsOut;
};
__global__ void __launch_bounds__(256) fltx_pack_results_kernel(PackParams Q) {
  const int b = (int)blockIdx.x;
  const int n = Q.count[b];
  const int32_t* src = Q.tokens + Q.srcOff[b];
  uint8_t* dst = Q.tok8 + Q.dstOff[b];
  for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
    const int32_t v = src[i];
    dst[i] = v < 0 ? (uint8_t)0xFF : (uint8_t)v;
  }
  if (Q.words) {
    const int32_t* ws = Q.words + Q.srcOff[b];
    int32_t* wd = Q.wordsOut + Q.dstOff[b];
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) {
      wd[i] = ws[i];
    }
  }
}
/* fltx_transcript.h: collapsed transcripts of frame rows -- count per row, offsets, write */
__global__ void __launch_bounds__(kTrThreads) fltx_transcript_count_kernel(TrParams Q) { trCountRows(Q, nullptr); }
__global__ void __launch_bounds__(kTrScanThreads) fltx_transcript_scan_kernel(TrParams Q) {
  __shared__ __attribute__((aligned(16))) TrScanLds fltx_tr_scan_lds;
  trScanRows(Q, (char*)&fltx_tr_scan_lds);
}
__global__ void __launch_bounds__(kTrThreads) fltx_transcript_write_kernel(TrParams Q) { trWriteRows(Q, nullptr); }
/* fltx_ctc_rows_plan.h: the LM rows of a CTC rows step's list -- new states marked and counted, rows assigned and the
 * lists written; the same pair for a release */
__global__ void __launch_bounds__(kCpThreads) fltx_ctc_rows_plan_mark_kernel(CpParams P) {
  __shared__ CpLds lds;
  cpMark(P, (char*)&lds);
}
__global__ void __launch_bounds__(kCpThreads) fltx_ctc_rows_plan_assign_kernel(CpParams P) {
  __shared__ CpLds lds;
  cpAssign(P, (char*)&lds);
}
__global__ void __launch_bounds__(kCpThreads) fltx_ctc_rows_plan_release_count_kernel(CpParams P) {
  __shared__ CpLds lds;
  cpReleaseCount(P, (char*)&lds);
}
__global__ void __launch_bounds__(kCpThreads) fltx_ctc_rows_plan_release_kernel(CpParams P) {
  __shared__ CpLds lds;
  cpRelease(P, (char*)&lds);
}
/* fltx_s2s.h: the seq2seq step (front end, step), its start and its back-trace */
__global__ void __launch_bounds__(256) fltx_s2s_tokbeam_kernel(S2sParams P) {
  __shared__ __attribute__((aligned(16))) S2sFrontLds fltx_s2s_front[4];
  s2sTokBeamRows(P, (char*)fltx_s2s_front);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_s2s_step_kernel(S2sParams P) {
  __shared__ __attribute__((aligned(16))) S2sStepLds fltx_s2s_lds;
  s2sStepUtterance(P, (char*)&fltx_s2s_lds);
}
__global__ void __launch_bounds__(kS2sBeginThreads) fltx_s2s_begin_kernel(S2sParams P) {
  s2sBeginUtterance(P, nullptr);
}
__global__ void __launch_bounds__(kS2sEndThreads) fltx_s2s_end_kernel(S2sParams P) {
  s2sEndUtterance(P, nullptr);
}
/* fltx_s2s_finish: a named slot's back-trace, then its restart or parking; every other slot's rows listed again */
__global__ void __launch_bounds__(kS2sEndThreads) fltx_s2s_finish_kernel(S2sFinishKernelParams Z) {
  __shared__ S2sFinishLds fltx_s2s_finish_lds;
  s2sFinishUtterance(Z, (char*)&fltx_s2s_finish_lds);
}
/* the typed front end (fltx_s2s_step_typed): fp16 / bf16 rows, and logits of any of the three types */
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sTypedThreads) fltx_s2s_typed_kernel(S2sTypedParams Q) {
  __shared__ __attribute__((aligned(16))) S2sTypedLds fltx_s2s_typed_lds;
  s2sTypedRows<DT, LOGITS>(Q, (char*)&fltx_s2s_typed_lds);
}
/* a rows LM (fltx_s2s_step_lm_rows): the LM scores of the records' tokens, then the step that reads them */
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sLmThreads) fltx_s2s_lm_rows_kernel(S2sLmRowsParams Q) {
  __shared__ __attribute__((aligned(16))) S2sLmRowsLds fltx_s2s_lm_rows_lds;
  s2sLmRows<DT, LOGITS>(Q, (char*)&fltx_s2s_lm_rows_lds);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_s2s_step_lm_rows_kernel(S2sLmRowsParams Q) {
  __shared__ __attribute__((aligned(16))) S2sStepLds fltx_s2s_lm_step_lds;
  s2sStepUtteranceLmRows(Q, (char*)&fltx_s2s_lm_step_lds);
}
/* fltx_s2s_lex.h: the lexicon seq2seq step (its front end is fltx_s2s_tokbeam_kernel), start and back-trace */
__global__ void __launch_bounds__(kS2sStepThreads) fltx_s2s_lex_step_kernel(S2lParams Q) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_s2l_lds;
  s2lStepUtterance(Q, (char*)&fltx_s2l_lds);
}
/* ... with a rows LM: after fltx_s2s_lm_rows_kernel, the LM term read from the records */
__global__ void __launch_bounds__(kS2sStepThreads) fltx_s2s_lex_step_lm_rows_kernel(S2lLmRowsParams R) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_s2l_lm_lds;
  s2lStepUtteranceLmRows(R, (char*)&fltx_s2l_lm_lds);
}
/* ... with a word rows LM (fltx_s2s_step_word_lm_rows): the records' word-level LM entries, then the step on them */
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sLmThreads) fltx_s2s_lex_word_lm_rows_kernel(S2lWordLmParams W) {
  __shared__ __attribute__((aligned(16))) S2sLmRowsLds fltx_s2l_word_lm_lds;
  s2lWordLmRows<DT, LOGITS>(W, (char*)&fltx_s2l_word_lm_lds);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_s2s_lex_step_word_lm_rows_kernel(S2lWordLmStepParams R) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_s2l_word_lm_step_lds;
  s2lStepUtteranceWordLmRows(R, (char*)&fltx_s2l_word_lm_step_lds);
}
__global__ void __launch_bounds__(kS2sBeginThreads) fltx_s2s_lex_begin_kernel(S2lParams Q) {
  s2lBeginUtterance(Q, nullptr);
}
__global__ void __launch_bounds__(kS2sEndThreads) fltx_s2s_lex_end_kernel(S2lParams Q) {
  s2lEndUtterance(Q, nullptr);
}
__global__ void __launch_bounds__(kS2sEndThreads) fltx_s2s_lex_finish_kernel(S2lFinishKernelParams Z) {
  __shared__ S2sFinishLds fltx_s2l_finish_lds;
  s2lFinishUtterance(Z, (char*)&fltx_s2l_finish_lds);
}
/* fltx_ctc_rows.h: lexicon-free CTC with a rows LM -- the frames' token beams (once), the LM entries of a frame's kept
 * tokens, the frame step and its finish variant (decodeEnd + back-trace), the start */
__global__ void __launch_bounds__(256) fltx_ctc_rows_tokbeam_kernel(CrParams Q) {
  __shared__ __attribute__((aligned(16))) S2sFrontLds fltx_cr_front[4];
  crTokBeamRows(Q, (char*)fltx_cr_front);
}
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sLmThreads) fltx_ctc_rows_lm_kernel(CrLmParams W) {
  __shared__ __attribute__((aligned(16))) S2sLmRowsLds fltx_cr_lm_lds;
  crLmRows<DT, LOGITS>(W, (char*)&fltx_cr_lm_lds);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_step_kernel(CrParams Q) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_cr_step_lds;
  crStepUtterance<false>(Q, (char*)&fltx_cr_step_lds);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_end_kernel(CrParams Q) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_cr_end_lds;
  crStepUtterance<true>(Q, (char*)&fltx_cr_end_lds);
}
__global__ void __launch_bounds__(kS2sBeginThreads) fltx_ctc_rows_begin_kernel(CrParams Q) {
  crBeginUtterance(Q, nullptr);
}
/* fltx_ctc_rows_lex.h: lexicon CTC with a rows LM -- the word-level gather, the frame step and its finish variant per LM
 * level (SRC), the start; the token beams and the token-level gather are the kernels above */
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sLmThreads) fltx_ctc_rows_lex_word_lm_kernel(CrlWordLmParams W) {
  __shared__ __attribute__((aligned(16))) S2sLmRowsLds fltx_crl_lm_lds;
  crlWordLmRows<DT, LOGITS>(W, (char*)&fltx_crl_lm_lds);
}
template <int SRC>
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_lex_step_kernel(CrlParams R) {
  __shared__ __attribute__((aligned(16))) CrlStepLds fltx_crl_step_lds;
  crlStepUtterance<SRC, false>(R, (char*)&fltx_crl_step_lds);
}
template <int SRC>
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_lex_end_kernel(CrlParams R) {
  __shared__ __attribute__((aligned(16))) CrlStepLds fltx_crl_end_lds;
  crlStepUtterance<SRC, true>(R, (char*)&fltx_crl_end_lds);
}
__global__ void __launch_bounds__(kS2sBeginThreads) fltx_ctc_rows_lex_begin_kernel(CrlParams R) {
  crlBeginUtterance(R, nullptr);
}
/* fltx_ctc_rows_typed.h: the typed frame front end (fp16 / bf16 / float32 frames of any stride, log-probs or logits) --
 * a wave per narrow frame, a workgroup per wide one -- and the lexicon step that reads its blank and same-node emissions
 * from the typed frames */
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(256) fltx_ctc_rows_typed_wave_kernel(CrTypedParams Z) {
  __shared__ __attribute__((aligned(16))) CrTypedWaveLds fltx_crt_wave_lds[4];
  crTypedWaveRows<DT, LOGITS>(Z, (char*)fltx_crt_wave_lds);
}
template <int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sTypedThreads) fltx_ctc_rows_typed_wg_kernel(CrTypedParams Z) {
  __shared__ __attribute__((aligned(16))) S2sTypedLds fltx_crt_wg_lds;
  crTypedWgRows<DT, LOGITS>(Z, (char*)&fltx_crt_wg_lds);
}
template <int SRC, int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_lex_typed_step_kernel(CrlTypedParams Y) {
  __shared__ __attribute__((aligned(16))) CrlStepLds fltx_crlt_step_lds;
  crlStepTyped<SRC, DT, LOGITS>(Y, (char*)&fltx_crlt_step_lds);
}
/* fltx_ctc_rows_stream.h: streams on the two CTC rows kinds -- the start, the frame step and its finish variant on the
 * streams' own counts and history ring; getBestHypothesis and prune */
__global__ void __launch_bounds__(kS2sBeginThreads) fltx_ctc_rows_stream_begin_kernel(CrStreamParams Z) {
  crsBeginStream(Z, nullptr);
}
__global__ void __launch_bounds__(kS2sBeginThreads) fltx_ctc_rows_lex_stream_begin_kernel(CrlStreamParams Z) {
  crlsBeginStream(Z, nullptr);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_stream_step_kernel(CrStreamParams Z) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_crs_step_lds;
  crsStepStream<false>(Z, (char*)&fltx_crs_step_lds);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_stream_end_kernel(CrStreamParams Z) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_crs_end_lds;
  crsStepStream<true>(Z, (char*)&fltx_crs_end_lds);
}
template <int SRC>
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_lex_stream_step_kernel(CrlStreamParams Z) {
  __shared__ __attribute__((aligned(16))) CrlStepLds fltx_crls_step_lds;
  crlsStepStream<SRC, false>(Z, (char*)&fltx_crls_step_lds);
}
template <int SRC>
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_lex_stream_end_kernel(CrlStreamParams Z) {
  __shared__ __attribute__((aligned(16))) CrlStepLds fltx_crls_end_lds;
  crlsStepStream<SRC, true>(Z, (char*)&fltx_crls_end_lds);
}
template <int SRC, int DT, bool LOGITS>
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_lex_typed_stream_step_kernel(CrlTypedStreamParams Y) {
  __shared__ __attribute__((aligned(16))) CrlStepLds fltx_crlts_step_lds;
  crlsStepStreamTyped<SRC, DT, LOGITS>(Y, (char*)&fltx_crlts_step_lds);
}
template <bool LEX>
__global__ void __launch_bounds__(kCrsOpThreads) fltx_ctc_rows_stream_best_kernel(CrsOpParams W) {
  __shared__ __attribute__((aligned(16))) CrsOpLds fltx_crs_best_lds;
  crsBest<LEX>(W, (char*)&fltx_crs_best_lds);
}
template <bool LEX>
__global__ void __launch_bounds__(kCrsOpThreads) fltx_ctc_rows_stream_prune_kernel(CrsOpParams W) {
  __shared__ __attribute__((aligned(16))) CrsOpLds fltx_crs_prune_lds;
  crsPrune<LEX>(W, (char*)&fltx_crs_prune_lds);
}
template <bool LEX>
__global__ void __launch_bounds__(kCrsOpThreads) fltx_ctc_rows_stream_collect_kernel(CrsCollectParams W) {
  __shared__ __attribute__((aligned(16))) CrsCollectLds fltx_crs_collect_lds;
  crsCollect<LEX>(W, (char*)&fltx_crs_collect_lds);
}
/* fltx_ctc_rows_stream_finish: which rows its gather reads; decodeEnd and decodeBegin of the named streams in one launch,
 * a workgroup per stream; the planner's rows of their ids given back (fltx_ctc_rows_plan.h) */
__global__ void __launch_bounds__(kS2sBeginThreads) fltx_ctc_rows_stream_finish_mask_kernel(CrFinishParams Z) {
  crsFinishMask(Z, nullptr);
}
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_stream_finish_kernel(CrFinishParams Z) {
  __shared__ __attribute__((aligned(16))) S2lStepLds fltx_crs_finish_lds;
  crsFinishStream(Z, (char*)&fltx_crs_finish_lds);
}
template <int SRC>
__global__ void __launch_bounds__(kS2sStepThreads) fltx_ctc_rows_lex_stream_finish_kernel(CrlFinishParams Z) {
  __shared__ __attribute__((aligned(16))) CrlStepLds fltx_crls_finish_lds;
  crlsFinishStream<SRC>(Z, (char*)&fltx_crls_finish_lds);
}
__global__ void __launch_bounds__(kCpThreads) fltx_ctc_rows_plan_finish_count_kernel(CpFinishParams F) {
  __shared__ CpLds lds;
  cpFinishCount(F, (char*)&lds);
}
__global__ void __launch_bounds__(kCpThreads) fltx_ctc_rows_plan_finish_release_kernel(CpFinishParams F) {
  __shared__ CpLds lds;
  cpFinishRelease(F, (char*)&lds);
}
/* fltx_stream_partials.h: the partial transcript and the stable prefix of every stream (KIND 0: the classic streams,
 * 1 / 2: the lexicon-free / lexicon rows streams) */
template <int KIND>
__global__ void __launch_bounds__(kSpThreads) fltx_stream_partials_kernel(SpParams Q) {
  __shared__ __attribute__((aligned(16))) SpLds fltx_sp_lds;
  spPartials<KIND>(Q, (char*)&fltx_sp_lds);
}
/* fltx_stream_finish.h: the back-trace of the named classic streams after their decodeEnd (and the counts of all B), and
 * the named streams' LM-state ids and tables started over before their decodeBegin; a workgroup per named stream */
__global__ void __launch_bounds__(kSfThreads) fltx_stream_finish_kernel(SfParams Q) {
  __shared__ __attribute__((aligned(16))) SfLds fltx_sf_lds;
  sfFinishStream(Q, (char*)&fltx_sf_lds);
}
__global__ void __launch_bounds__(kSfThreads) fltx_stream_restart_kernel(SfRestartParams Q) {
  sfRestartStream(Q, nullptr);
}
__global__ void __launch_bounds__(1024) fltx_streamop_kernel(StreamOpParams Q) {
  __shared__ int32_t sh[kStreamOpLds / 4];
  streamOpUtterance(Q, sh);
}
#endif

/* ------------------------------------------------------------------------ */
/* device back-end                                                           */
/* ------------------------------------------------------------------------ */
namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#ifdef FLTX_EMU
typedef void* Stream;
int devCount() { return 1; }
int devMalloc(void** p, size_t n) {
  *p = calloc(1, n ? n : 1);
  return *p ? 0 : 1;
}
void devFree(void* p) { free(p); }
int devMemset(void* p, int v, size_t n, Stream) {
  memset(p, v, n);
  return 0;
}
int devCopyH2D(void* d, const void* h, size_t n, Stream) {
  memcpy(d, h, n);
  return 0;
}
int devCopyD2H(void* h, const void* d, size_t n, Stream) {
  memcpy(h, d, n);
  return 0;
}
int devSync(Stream) { return 0; }
const char* devErr() { return "emu"; }
constexpr size_t kMaxLds = 160 * 1024;
#else
typedef hipStream_t Stream;
#define HIPCHK(x)                                                              \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess)                                                      \
      return fail(FLTX_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_));          \
  } while (0)
int devMalloc(void** p, size_t n) { return hipMalloc(p, n ? n : 1) == hipSuccess ? 0 : 1; }
void devFree(void* p) { (void)hipFree(p); }
int devMemset(void* p, int v, size_t n, Stream s) { return hipMemsetAsync(p, v, n, s) == hipSuccess ? 0 : 1; }
int devCopyH2D(void* d, const void* h, size_t n, Stream s) {
  return hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s) == hipSuccess ? 0 : 1;
}
int devCopyD2H(void* h, const void* d, size_t n, Stream s) {
  if (hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s) != hipSuccess) {
    return 1;
  }
  return hipStreamSynchronize(s) == hipSuccess ? 0 : 1;
}
int devSync(Stream s) { return hipStreamSynchronize(s) == hipSuccess ? 0 : 1; }
const char* devErr() { return hipGetErrorString(hipGetLastError()); }
constexpr size_t kMaxLds = 160 * 1024; /* gfx950: 160 KiB LDS per CU */

#endif

/* growable PINNED host buffer: results cross PCIe in one transfer per array */
struct HBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) {
      return 0;
    }
    release();
#ifdef FLTX_EMU
    p = malloc(n ? n : 1);
    if (!p) {
      return 1;
    }
#else
    if (hipHostMalloc(&p, n ? n : 1, hipHostMallocDefault) != hipSuccess) {
      p = nullptr;
      return 1;
    }
#endif
    cap = n;
    return 0;
  }
  void release() {
    if (p) {
#ifdef FLTX_EMU
      free(p);
#else
      (void)hipHostFree(p);
#endif
    }
    p = nullptr;
    cap = 0;
  }
  ~HBuf() { release(); }
};

/* PINNED staging of a small upload that must not stall its stream: the host writes it, an asynchronous copy reads it,
 * and it is rewritten only when that copy has completed (an event of its own: queried, waited for only if it has not
 * fired -- after a settled batch it always has) */
struct Staging {
  HBuf h;
#ifndef FLTX_EMU
  hipEvent_t done = nullptr;
  bool inFlight = false;
  ~Staging() {
    if (done) {
      (void)hipEventDestroy(done);
    }
  }
#endif
  void* acquire(size_t n) { /* null: failed */
#ifndef FLTX_EMU
    if (inFlight) {
      if (hipEventQuery(done) != hipSuccess) {
        (void)hipGetLastError(); /* ("not ready" is no error of the launch that follows) */
        if (hipEventSynchronize(done) != hipSuccess) {
          return nullptr;
        }
      }
      inFlight = false;
    }
#endif
    return h.ensure(n) ? nullptr : h.p;
  }
  int sent(Stream s) { /* the copy that reads the staging has been queued on s */
#ifndef FLTX_EMU
    if (!done && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) {
      return 1;
    }
    if (hipEventRecord(done, s) != hipSuccess) {
      return 1;
    }
    inFlight = true;
#else
    (void)s;
#endif
    return 0;
  }
};

/* a part of a device buffer */
struct DView {
  void* p = nullptr;
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

/* growable device buffer */
struct DBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~DBuf() {
    if (p) {
      devFree(p);
    }
  }
  /* returns 0 ok; `grew` tells the caller the contents are fresh (zeroed) */
  int ensure(size_t n, Stream s, bool zero, bool* grew = nullptr) {
    if (grew) {
      *grew = false;
    }
    if (n <= cap) {
      return 0;
    }
    if (p) {
      devSync(s);
      devFree(p);
      p = nullptr;
      cap = 0;
    }
    size_t want = n + n / 8;
    if (devMalloc(&p, want)) {
      p = nullptr;
      return 1;
    }
    cap = want;
    if (zero && devMemset(p, 0, want, s)) {
      return 1;
    }
    if (grew) {
      *grew = true;
    }
    return 0;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

/* fltx_collapse_rows / fltx_result_transcripts: one set of growing buffers per owner (context / decoder) */
struct TrBufs {
  DBuf meta;  /* totals[2] i64, tokOff[n + 1] i64, wordOff[n + 1] i64, nTok[n] i32, nWord[n] i32 */
  DBuf desc;  /* rowOff[n] i64, rowLen[n] i32 (the decoder call's rows) */
  DBuf tokens, timesteps, words, wordT, wordEnd;
  HBuf hTotals, hDesc, hOff, hTokens, hTimesteps, hWords, hWordT, hWordEnd;
  DBuf pack;  /* fltx_stream_partials: the five arrays back to back, and their pinned twin -- one copy home */
  HBuf hPack;
  std::vector<int64_t> rowFirst;
  /* "time_transcripts": HIP events around the three kernels (and around fltx_pack_results_kernel) */
  int timed = 0;
  float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f}; /* count, scan, write; pack */
#ifndef FLTX_EMU
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~TrBufs() {
    for (hipEvent_t e : ev) {
      if (e) {
        (void)hipEventDestroy(e);
      }
    }
  }
#endif
};

uint32_t nextPow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) {
    p <<= 1;
  }
  return (uint32_t)p;
}

} // namespace

/* ------------------------------------------------------------------------ */
/* objects                                                                   */
/* ------------------------------------------------------------------------ */
struct fltx_ctx {
  uint64_t uid = 0; /* never reused: per-context tables are keyed by it, not by the object's address */
  int device = 0;
  int numCUs = 256; /* MI355X; read from the device at creation */
  Stream stream = nullptr;
  bool ownStream = false;
  TrBufs tr; /* fltx_collapse_rows */
};

/* every entry point that allocates, copies or launches selects its context's device first:
 * decoders of several devices are driven from several host threads (fltx_group_*) */
/* ... and puts the calling thread's device back when the entry point returns: the host framework's
 * later allocations and launches in that thread must not move to another GPU because of a call here */
struct DeviceScope {
  int prev = -1;
  bool failed = false;
  explicit DeviceScope(const fltx_ctx* ctx) {
#ifndef FLTX_EMU
    if (ctx) {
      if (hipGetDevice(&prev) != hipSuccess) {
        prev = -1;
      }
      if (prev == ctx->device) {
        prev = -1; /* nothing to restore */
      } else {
        failed = hipSetDevice(ctx->device) != hipSuccess;
      }
    }
#else
    (void)ctx;
#endif
  }
  ~DeviceScope() {
#ifndef FLTX_EMU
    if (prev >= 0) {
      (void)hipSetDevice(prev);
    }
#endif
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

struct fltx_lm {
  fltx_ctx* ctx = nullptr;
  int kind = 0; /* 0 zero, 1 ngram, 2 host callbacks (fltx_lm_host_create), 3 rows (fltx_lm_rows_create), 4 word-level
                 * rows (fltx_lm_word_rows_create: hUsr maps word ids, rowsFinish is given) */
  fltx_host_lm host{};
  /* rows LM: entries per LM row (0: the decoder's V), the LM index finish reads (-1: usr_to_lm[eos]), and whether hUsr
   * holds a map (else identity) */
  int32_t rowsWidth = 0, rowsFinish = -1;
  bool rowsMap = false;
  int order = 0;
  int32_t bos = 0, eos = 0, unk = 0, nUsr = 0;
  uint32_t mask = 0;
  /* device copies of the tables, one set per context (= per device) that has a decoder using this LM */
  struct Dev {
    DBuf tab, backoff, usrToLm;
    std::map<int, std::unique_ptr<DBuf>> tokDense; /* key = token count N: this device's copy of TokDense::tab */
  };
  /* The LM as ONE gather for a decoder over a small token set (fltx_slane.h's TL variant: a token-level n-gram LM on
   * the lexicon-free decoder, LexiconFreeDecoder.cpp:69-85 + KenLM.cpp:63-83): row c = a context the model can be
   * in (the vector of suffix node ids ngScore takes), reached from KenLM::start(false) by any token sequence; column
   * n < N = {float bits of lm.score(c, token n), row of the context after it}; column N = lm.finish(c).  Built on first use
   * per N by a breadth-first walk with the host twin of ngScore (lmStepWord): the scores are the ones the generic engine
   * computes, bit for bit.  nCtx < 0: the model has more contexts than the cap -- such decoders stay on the generic engine. */
  struct TokDense {
    int64_t nCtx = 0;
    std::vector<int2> tab; /* [nCtx][N + 1] */
  };
  std::map<int, std::unique_ptr<TokDense>> tokDense; /* guarded by devMu */
  std::mutex devMu;
  std::unordered_map<uint64_t, std::unique_ptr<Dev>> dev; /* key = fltx_ctx::uid */
  /* host copies for fltx_lm_score_sequence */
  std::vector<NgramSlot> hTab;
  std::vector<float> hBackoff;
  std::vector<int32_t> hUsr;
};

/* live LM objects: fltx_ctx_destroy drops the tables they hold for that context */
static std::mutex g_lmRegMu;
static std::unordered_set<fltx_lm*> g_lmReg;
static std::atomic<uint64_t> g_ctxUid{1};

struct fltx_trie {
  fltx_ctx* ctx = nullptr;
  int64_t nNodes = 0;
  int32_t nTokens = 0;
  DBuf edge, labels, mask;
  /* breadth-first re-layout for the lane = (LM state, trie node) engine (fltx_xlane.h): a node's
   * children are contiguous and in token order, so a child's id is the first child's id plus the
   * number of children with a smaller token; one 32-byte XNode per node, root = 0 */
  DBuf xnode, xdelta, xextra;
  bool xMulti = false;  /* some spelling has several words (Trie.h:19: up to 6 labels per node): fltx_ylane.h's LMK bit 2 */
  std::vector<int32_t> xEndHost; /* XNode::endLabel0 per node (host copy: decoders map it to LM word ids) */
  bool xOk = false;     /* the layout exists and the trie has the shape that engine assumes: */
  int32_t xEndTok = -1; /* every node that carries labels is entered by this one token (the word separator) */
  float xDeltaMin = 0.0f, xDeltaMax = 0.0f; /* range of the smearing differences of the layout */
  bool xZeroSmear = true; /* every maxScore is 0 (a lexicon without LM scores) */
};

struct fltx_decoder {
  fltx_ctx* ctx = nullptr;
  fltx_lm::Dev* lmDev = nullptr; /* this context's copy of the LM tables (null for ZeroLM) */
  int kind = 0;
  fltx_options opt{};
  const fltx_trie* trie = nullptr;
  const fltx_lm* lm = nullptr;
  int sil = 0, blank = 0, unk = 0, isLmToken = 0;
  int nTrans = 0;
  double transMax = 0.0; /* largest transition score, at least 0 */
  DBuf transitions;
  /* tunables */
  int threads = 0; /* 0 = pick per configuration (prepare()) */
  int userThreads = 0;
  int forceGlobalWs = 0;
  /* batch state */
  int B = 0, N = 0;
  bool streaming = false, ended = false, haveResults = false;
  int maxFrames = 0;
  std::vector<int32_t> T;       /* frames given in the last step */
  std::vector<int32_t> frames;  /* host mirror of uttFrame after sync */
  bool framesExact = true;       /* false: frames[] is an upper bound (lexicon prunes not yet asked about) */
  /* an optimistic stream chunk is launched and left alone: whether it has to be decoded again is looked at by the next
   * call that needs the beam (settleStream), so the next chunk's upload runs under this chunk's kernel */
  bool chunkPending = false, settling = false;
  const float* pendEmis = nullptr;
  int pendSlot = 0;
  int pendingPrune = -1;         /* prune(lookBack) asked for while the chunk was pending: runs right after the look */
  bool useLmCache = false;
  int noLmCache = 0;             /* tunable lm_cache = 0 */
  int deferRedo = 1;             /* tunable stream_defer: 0 = look at every chunk before fltx_stream_step returns */
  std::vector<int64_t> histOff; /* records */
  int64_t histRecords = 0;
  uint32_t stateCap = 0;
  uint32_t epoch = 0;
  int CAP = 0, HS = 0, NB = 0, SCAP = 0, dense = 0, noDense = 0;
  int lean = 0, noLean = 0; /* lean: GMAX of the lean lexicon-free kernel, 0 = generic engine */
  int lane = 0, noLane = 0; /* lane: tokens per wave of the lane-per-slot kernel (fltx_lane.h), 0 = off */
  int slaneThreads = 0; /* tuning: workgroup size of the lane = LM state kernel (0 = first that fits) */
  int wlane = 0, noWlane = 0; /* wlane: the lane = LM state kernel is fltx_wlane.h's (token sets beyond 64, token beam <= 64); slane = its list positions per wave */
  int slane = 0, noSlane = 0; /* slane: list positions per wave of the lane = LM state kernel (fltx_slane.h), 0 = off */
  /* ... its variant for a token-level n-gram LM (TL): the LM's dense (context, token) table on this device; noTlane:
   * tunable "tlane" = 0 (tests compare with the generic engine) */
  int tlane = 0, noTlane = 0, tlaneFirst = 0;
  int noTokDense = 0; /* tunable "tok_dense" = 0: no dense table at all (the generic engine probes the n-gram tables) */
  const int2* tokLm = nullptr;
  int64_t tokLmCtx = 0;
  int tlEdgeSlots = 4096, tlMaskSlots = 2048;
  bool tokLmTooBig = false; /* the model has more contexts than a dense table holds (why_not_lane: LM) */
  /* ... with several lane groups (fltx_mlane.h, beams beyond 64): lane groups (0 / 1 = fltx_slane.h), groups per token
   * wave, groups per self wave; userLaneGroups: tuning / tests, 0 = as many as the beam needs, -1 = never */
  int mlaneNG = 0, mlaneGPW = 0, mlaneSPW = 0, userLaneGroups = 0, userMlaneGeo = -1;
  int noYlaneAsg = 0;        /* tests: ASG lexicon decodes stay on the generic engine */
  int userYRankAt = 0;       /* tests: DecodeParams::yRankAt */
  int userTune = 0;          /* development: DecodeParams::tune */
  int userYlaneGroups = 0;   /* tests: at least this many lane groups on fltx_ylane.h (0 = what the beam needs) */
  uint32_t ymemoSlots = 8192; /* slots per utterance of the LM-state memo in HBM (fltx_ylane.h: follows the frames) */
  int64_t fallbackReasons = 0; /* bit r: an utterance of the last batch left fltx_ylane.h for reason r (see YL_WHY there) */
  int64_t whyNotLane = 0; /* FLTX_WHY_* bits: the eligibility terms that kept the last call off the lane engines (0 = it ran there) */
  bool preferYlane = false;
  bool genericAsked = false;  /* fltx_decoder_set touched a tunable of the generic engine */
  int engineFirst = 0;
  /* diagnostics of the engine a call STARTED on (a retry's prepare() must not overwrite them) */
  int64_t whyFirst = 0;
  int wlaneFirst = 0, slaneFirst = 0, laneGroupsFirst = 0, xlaneFirst = 0, ylaneFirst = 0;
  int slaneM32First = 0; /* ... on the fltx_slane.h kernel with 32-bit token masks (slaneM32) */
  int noSlaneM32 = 0;    /* tuning: 64-bit token masks whatever the token set (measurements: fltx_decoder_set "slane_m32" 0) */
  int lastRedo = 0;           /* utterances of the last offline call that had to be decoded again on a general path */
  int packedBits = 8;         /* width of the parent-slot field of those records (fltx_mlane.h: 10) */
  bool batchPacked = false;   /* some utterance of the current results has packed history records (ST_PACKED) */
  bool batchTlane = false;    /* ... by fltx_slane.h's token-LM variant (the back-trace re-accumulates the LM score as well) */
  bool batchWlane = false;    /* ... written by fltx_wlane.h (tokens beyond a byte, emissions gathered by the back-trace) */
  DBuf xlmword;               /* fltx_ylane.h: LM word id of XNode::endLabel0 per node (this decoder's trie x LM) */
  const fltx_trie* xlmwordTrie = nullptr;
  const fltx_lm* xlmwordLm = nullptr;
  int ylane = 0, noYlane = 0, ylaneLm = 0, ylaneRounds = 0, ylaneTpw = 0; /* ylane: lane groups of fltx_ylane.h (0 = not used) */
  int btLdsKb = 0;
  int btNarrow = 0, btChunk = 0, btStretch = 0; /* fltx_decoder_get "bt_record_bytes", "bt_chunk_frames", "bt_stretch_frames" */
  int btThreads = 0;    /* "bt_threads": threads of a back-trace workgroup (0: 512; the emulator: one wave; never fewer than the beam's slots) */
  int btWalkAsked = -1; /* "bt_walk_waves" (set): 0 / 1 = the serial walk, else the parallel walk where it applies */
  int btWalkWaves = 0;  /* "bt_walk_waves" (get): waves that walked the chunks of the last back-trace (1 = the serial walk) */
  bool btProfile = false; /* "bt_profile": shader-clock marks of the narrow back-trace (btProf, kBtProfMarks per utterance) */
  DBuf btProf;
  int streamTotalFrames = 0; /* frames a stream will decode in all (sizes its LM-state id tables), 0 = default */
  /* stream chunks of the lexicon-free decoder on the lane = LM state engine (fltx_slane.h, ST): list positions per
   * token wave (0 = not used) and threads; begin / end / prune / best stay the lane-per-slot engine's */
  int sstream = 0, sstreamThreads = 0, noSstream = 0;
  int tstream = 0; /* ... the stream's chunks run on fltx_slane.h's token-LM variant (ids from the generic engine's table) */
  bool sstreamLaunch = false;
  /* streams of the lexicon decoder on the optimistic geometry (LDS workspace, cut-off generation): a chunk that
   * overflows is decoded again from the saved beam on the general path (HBM workspace) */
  int userStreamOpt = 1;
  bool streamOpt = false;
  int streamRedone = 0; /* stream-chunks decoded again since fltx_stream_begin */
  DBuf snap;
  int yshare = 0, userYshare = -1; /* the geometry of fltx_ylane.h that shares a CU (memo in HBM); user: -1 = when the batch exceeds the CUs */
  DBuf ymemo;
  DBuf lmCache;               /* DecodeParams::lmCache */
  int xlane = 0, noXlane = 0; /* xlane: list positions per token wave of the lane = (LM state, trie node) kernel (fltx_xlane.h) */
  bool offlineCall = false;   /* prepare() is sizing an fltx_decode_batch (begin + frames + end in one launch) */
  /* "defer_check": fltx_decode_batch returns with its kernels queued; the look at the utterances' statuses (and the
   * second pass of what a fast path flagged) waits for the first call that reads results */
  int deferCheck = 0; /* 1: an unread batch is settled by the next fltx_decode_batch; 2: dropped there (counted in looksDropped) */
  bool offlinePending = false;
  int64_t looksDropped = 0;  /* batches whose statuses nobody ever looked at ("looks_dropped"; defer_check = 2 only) */
  int64_t unreadRedone = 0;  /* utterances decoded again while settling batches the caller never read ("unread_redone") */
  std::vector<int32_t> offT;
  std::vector<int64_t> offOffsets;
  int offN = 0, offUpSlot = 0;
  const float* offEmis = nullptr;
  const float* lastEmis = nullptr; /* device emissions of the last offline batch (the back-trace re-reads them) */
  size_t hotBytes = 0; /* LDS part of a split (HBM + LDS) workspace */
  int hotLevel = 0;    /* what the LDS part holds (carveWs) */
  size_t ldsBudget = 0; /* tests: smaller LDS than the hardware's */
  int maxHotLevel = 2;
  int itemCap = 0, noItems = 0, itemWide = 0; /* lexicon decoder: list of existing (hypothesis, token) children */
  int CAP2 = 0, cutM = 0, noCut = 0, userCutM = 0;
  int cutRecompute = 0, noSlim = 0; /* cut-off generation without the slim list (beams it does not fit) */ /* lexicon decoder: slim score-pass list + cut-off (runFrame) */
  size_t wsBytes = 0;
  bool wsInLds = true;
  /* device buffers */
  /* what a step uploads, in two slots taking turns: the upload of step k + 1 runs on a copy stream under the kernel of
   * step k (which reads the other slot) */
  DBuf emis[2], emOff[2], stepT[2];
  int upSlot = 0;
  DBuf histOffD, histPT, histW, stateTab, stateCtx;
  std::vector<int64_t> histOffSent; /* what histOffD holds ... */
  const void* histOffSentTo = nullptr; /* ... in this allocation (uploadHistOff) */
  Staging histOffStage, descStage[2]; /* pinned: histOff; the offsets and T of an upload slot */
  const void* ldsRaisedFn[2] = {nullptr, nullptr}; /* decode / back-trace kernel whose LDS limit this decoder last raised ... */
  size_t ldsRaisedTo[2] = {0, 0};                  /* ... and to what (raiseMaxLdsOnce) */
  DBuf tokRowsBuf; /* fltx_wlane.h: the token beams of all rows (fltx_tokbeam_kernel) */
  int wlMaxT = 0;  /* ... longest utterance of the call (the front-end kernel's grid) */
  DBuf gScore, gAm, gLm, gState, gSPar, gSEdge, gLex, gTokPb;
  DBuf uttRes;   /* rows of uttRow int32: beam count, final frame, status per utterance -- one allocation, so that
                    syncResults brings the three home in one copy (ensureUttRes) */
  size_t uttRow = 0;
  DView uttNBeam, uttFrame, uttStatus;
  DBuf uttTotal, outN, outScores, gws;
  DBuf childTab, maskTab, uttNextId, gMask, gLexMax;
  /* streams: recycled LM-state ids (DecodeParams::idPar ...) */
  DBuf idPar, idEdge, idBorn, idKeep, idNew, idList, stateVal;
  bool recycle = false;       /* this stream hands ids out from free lists */
  int idFamily = 0;           /* 0: childTab / maskTab engines, 1: generic engine (stateTab + stateVal) */
  int64_t idsUsedBound = 0;   /* upper bound of the ids any stream has taken since its free list was last rebuilt */
  int64_t idsFreeBound = 0;   /* lower bound of what a rebuilt free list holds (beam x max_frames) */
  int compactions = 0;        /* fltx_compact_states_kernel launches since fltx_stream_begin ("compactions") */
  int userCompactAlways = 0;  /* tests ("compact_always"): rebuild the free lists before every chunk */
  DBuf scored; /* n-gram LM queries per utterance (accounting) */
  /* host LM (lm->kind == 2): question lists and beam states in pinned host memory (written by the kernel), the
   * answer tables staged in pinned memory and uploaded once per frame */
  HBuf hlmQCount, hlmQ, hlmBeamN, hlmBeam, hlmStage;
  DBuf hlmTabD;
  int hlmQCap = 0;
  bool hlmAnnounce = false; /* a frame has been decoded since decodeBegin: the beam is announced through update_cache */
  int64_t hlmAsked = 0, hlmDistinct = 0; /* questions listed / answered by the callbacks since decodeBegin ("hlm_asked", "hlm_distinct") */
  bool keepScored = false;
  int64_t idCap = 0;
  DBuf tokens, words, prof, histS, bestLen, bestScores, bestTok, bestWrd;
  HBuf hTokens, hWords, hScores; /* fltx_result_fetch_batch */
  HBuf hTok8, hWordsC, hPackMeta;  /* fltx_result_fetch_batch_compact */
  TrBufs tr;                       /* fltx_result_transcripts */
  /* fltx_stream_partials: the frames each classic stream has pruned off (int64 [B], zeroed by fltx_stream_begin); what
   * a call reports ({first_frame, rowOff}[B] int64, scores [B][3], {length, stable_frames, stable_tokens, stable_words,
   * status}[B] int32) with its pinned twin; the frame rows [B][cap]; the transcript's buffers, apart from tr's */
  DBuf uttFirst, spOut, spTok, spWrd;
  HBuf hSpOut;
  TrBufs spTr;
  HBuf hSync;                      /* syncResults */
  HBuf hStat;                      /* DecodeParams::statusHost */
  DBuf dTok8, dWordsC, dPackMeta;
  std::vector<int64_t> packOff;
  bool compactFetched = false, scoresFetched = false;
  DBuf uttMap;                   /* utterances of a partial re-run */
  int nLaunch = 0;               /* workgroups of the next decode launch (0: all B) */
  std::vector<int32_t> hLen, hNHyp;
  bool hostFetched = false;
  int keepScores = 0, userKeepScores = 0; /* (streams force the score history on; offline decodes use the caller's choice) */
  int profile = 0, profWave = 0;
  /* host caches of the last results */
  std::vector<int32_t> hN, hFrame, hStatus;
  bool resultsSynced = false;
  bool backtraced = false;
  int64_t statFrames = 0, statBytes = 0, statDecodeBytes = 0, statEpilogueBytes = 0, statLmBytes = 0;
  bool statsDone = false;
#ifndef FLTX_EMU
  /* HIP events on the launch stream bracketing the two kernels of the last
   * fltx_decode_batch (bench.py's roofline leg reads them) */
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipStream_t copyStream = nullptr;
  hipEvent_t evSlotFree[2] = {nullptr, nullptr}; /* recorded on the launch stream once everything that reads a slot is queued */
  bool slotUsed[2] = {false, false};
  hipEvent_t lookEv = nullptr; /* "defer_check": fires when the pending batch's status rows have reached hSync */
#endif
  bool lookQueued = false; /* the copy of the pending batch's status rows is queued behind its back-trace (queueLook) */
  bool timed = false;
  /* seq2seq (kinds FLTX_DECODER_S2S_LEXFREE / _LEXICON, fltx_s2s_*: fltx_s2s.h, fltx_s2s_lex.h) */
  struct {
    fltx_s2s_options opt{};
    int eos = 0, maxOut = 0, t = 0, cap = 0, mSel = 0, eosExtra = 0;
    bool begun = false;
    int32_t ctx0[kS2sCtx] = {0};
    DBuf beam, beamN, hist, rowsInt, done, finalStep, recTok, recAm, recN, cKey; /* (beam, hist: of the kind's types) */
    DBuf scores, valid; /* device copies of host inputs */
    DBuf recLm, lmScores; /* a rows LM: the records' LM scores; the device copy of host LM rows */
    int lmWidth = 0, lmFinish = 0; /* a rows LM: as fltx_s2s_begin resolved them for V */
    DBuf rowNode, lmRowOf; /* a word rows LM: the trie node of each row's hypothesis; the device copy of a host lm_row_of */
    /* with a lexicon (fltx_s2s_lex_decoder_create) */
    double wordScore = 0.0;
    bool isLmToken = false;
    int maxLabels = 0, slots = 1, mSize = 0, sSize = 0, sMax = 0, maxStates = 0;
    int64_t nodes = 0, edges = 0, labels = 0, trieBytes = 0;
    DBuf trieMax, kidOff, kidTok, kidNode, labOff, lab; /* the compact trie */
    DBuf cScore, cMk, cGrp, cList, cNext, mTab, sKey, sVal, sCount, status, merges;
    /* a step count per slot (fltx_s2s_finish): origin[B] and parked[B] live behind finalStep on the device (s2sOrigin);
     * this is what the host knows of them from `which` -- the batch's step count at each slot's last (re)start, the
     * parked slots, and the step count from which no slot can be live any more (the largest origin + max_output_length
     * of a slot not parked) */
    std::vector<int32_t> hOrigin;
    std::vector<uint8_t> hParked;
    int liveUntil = 0;
    /* lexicon-free CTC with a rows LM (kind FLTX_DECODER_CTC_ROWS, fltx_ctc_rows.h; it shares the buffers above): the
     * longest utterance, frames in all, {frameOff[B + 1], emOff[B]} int64 then T[B] int32 on the device and their host
     * copy, the device copy of host emissions */
    int crMaxT = 0;
    int64_t crFrames = 0;
    DBuf crMeta, crEmis;
    std::vector<int64_t> crMetaHost;
    const float* crEmisDev = nullptr;
    /* typed emissions (fltx_ctc_rows_begin_typed / _stream_append_typed, fltx_ctc_rows_typed.h) of the batch or the
     * current chunk: the dtype (kCrEmPlain: the float32 log-probs above), logits, the frame stride in elements, the
     * frames on the device (crEmis holds a host buffer's copy in its own type), each frame record's lse, and the
     * widest frame the wave-per-frame front end takes ("emissions_narrow_max") */
    int crEmDt = kCrEmPlain, crNarrowMax = kCrTypedNarrowMax;
    bool crEmLogits = false;
    int64_t crEmStride = 0;
    const void* crEmX = nullptr;
    DBuf crLse;
    /* lexicon CTC with a rows LM (kind FLTX_DECODER_LEX_CTC_ROWS, fltx_ctc_rows_lex.h; the compact trie, slots = S,
     * isLmToken and rowNode above are its too): the publisher's beam index, which is nobody's output */
    DBuf crOutBeam;
    /* streams on the two CTC rows kinds (fltx_ctc_rows_stream_begin, fltx_ctc_rows_stream.h): the frames a stream may
     * hold, the rows of the rings, {nDec[B], base[B]} and the score ring on the device, the host's upper bound of the
     * frames each stream holds, and the look-back the best* buffers answer (-1: none) */
    bool crStream = false;
    int crCap = 0, crRing = 0, crBestLb = -1;
    std::vector<int32_t> crBestLen;  /* [2][B] of the last best launch: lengths, statuses */
    std::vector<double> crBestScores; /* [B][3] */
    DBuf crCnt, crSHist;
    /* what fltx_ctc_rows_stream_collect recycles LM-state ids with: {sPar, sEdge, sFree}[B][sMax] then sFreeN[B], and
     * the mark bitsets [B][2][(sMax + 31) / 32] of tables too large for the kernel's LDS */
    DBuf crIds, crMarks;
    std::vector<int32_t> crBuf;
    /* fltx_ctc_rows_plan_begin (fltx_ctc_rows_plan.h): rowOf, the free stack, meta and prev (two halves each, the one
     * to read next in plMetaPar / plPrevPar), the counts and ranks between the two launches; and what the host knows of
     * the call sequence -- the last list is unplanned, a list was never planned, collects without their release */
    bool plOn = false, plFresh = false, plSkipped = false;
    int plRowCap = 0, plMetaPar = 0, plPrevPar = 0, plCollects = 0;
    DBuf plRowOf, plFree, plMeta, plPrev, plCnt, plRank;
    /* fltx_ctc_rows_stream_finish: its results, apart from those of fltx_ctc_rows_end -- scores [B*K*3], tokens and
     * words laid out by histOff, {n_hyp, length, status}[B] -- on the device and in pinned host memory; what it uploads
     * per call, {row_off[B] int64, which[B] int32}, through pinned staging; the gather's mask.
     * fltx_s2s_finish shares these buffers (a decoder is of one kind): its results, apart from those of fltx_s2s_end, are
     * scores [B*K*3], tokens and words [B*K][len] and {n_hyp, steps, status, the back-trace's two other counts}[B] in
     * finMeta; which[B] goes up through finStage into finIn */
    DBuf finScores, finTok, finWrd, finMeta, finIn, finSkip;
    HBuf hFinScores, hFinTok, hFinWrd, hFinMeta;
    Staging finStage;
  } s2s;
};

static bool isS2sKind(int kind) { return kind == FLTX_DECODER_S2S_LEXFREE || kind == FLTX_DECODER_S2S_LEXICON; }
static bool isCrKind(int kind) { return kind == FLTX_DECODER_CTC_ROWS || kind == FLTX_DECODER_LEX_CTC_ROWS; }
/* decoders that are stepped by their own entry points (fltx_s2s_*, fltx_ctc_rows_*): no batch call, no streams */
static const char* stepKindCalls(int kind) {
  return isS2sKind(kind) ? "a seq2seq decoder steps with fltx_s2s_step"
                         : isCrKind(kind) ? "a CTC rows decoder steps with fltx_ctc_rows_step" : nullptr;
}
/* decoders whose results carry words */
static bool kindHasWords(int kind) {
  return kind == FLTX_DECODER_LEXICON || kind == FLTX_DECODER_S2S_LEXICON || kind == FLTX_DECODER_LEX_CTC_ROWS;
}

/* how an entry point opens: the device of its context (or of its decoder's) selected for the call -- DeviceScope puts
 * the caller's back on every return path -- and then, for the entry points of the step decoders, the check that comes
 * first (s2sCheck, crCheck, crsCheck) under the call's name.  rc != 0 is what the call returns */
struct EntryScope {
  DeviceScope dev;
  int rc;
  explicit EntryScope(const fltx_ctx* ctx)
      : dev(ctx), rc(dev.failed ? fail(FLTX_ERR_HIP, "hipSetDevice failed") : (int)FLTX_OK) {}
  explicit EntryScope(fltx_decoder* d, const char* what = nullptr, int (*check)(fltx_decoder*, const char*) = nullptr)
      : EntryScope(d ? d->ctx : nullptr) {
    if (!rc && check) {
      rc = check(d, what);
    }
  }
};

/* ------------------------------------------------------------------------ */
extern "C" {

const char* fltx_last_error(void) { return g_err.c_str(); }
/* internal: lets the other translation units record an error message */
__attribute__((visibility("hidden"))) int fltx_set_error_(int code, const char* msg) {
  g_err = msg ? msg : "";
  return code;
}
/* internal (fltx_group.cpp): 0 ZeroLM, 1 n-gram tables, 2 host callbacks, 3 rows */
__attribute__((visibility("hidden"))) int fltx_lm_kind_(const fltx_lm* lm) { return lm ? lm->kind : -1; }
const char* fltx_version(void) {
#ifdef FLTX_EMU
  return "fltx 0.1 (host-thread emulation, tests only)";
#else
  return "fltx 0.1 (HIP gfx950)";
#endif
}

int fltx_ctx_create(int device, void* stream, fltx_ctx** out) {
  if (!out) {
    return fail(FLTX_ERR_INVALID, "fltx_ctx_create: out is null");
  }
  auto* c = new fltx_ctx();
  c->uid = g_ctxUid.fetch_add(1);
#ifndef FLTX_EMU
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    delete c;
    return fail(FLTX_ERR_HIP, "fltx_ctx_create: no HIP device available (this library has no CPU path)");
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) {
      delete c;
      return fail(FLTX_ERR_HIP, "hipGetDevice failed");
    }
  }
  if (device >= n) {
    delete c;
    return fail(FLTX_ERR_INVALID, "fltx_ctx_create: device %d out of range (%d devices)", device, n);
  }
  c->device = device;
  DeviceScope devScope(c);
  if (devScope.failed) {
    delete c;
    return fail(FLTX_ERR_HIP, "hipSetDevice(%d) failed", device);
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) {
      c->numCUs = cus;
    }
  }
  if (stream) {
    c->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return fail(FLTX_ERR_HIP, "hipStreamCreate failed");
    }
    c->ownStream = true;
  }
#else
  (void)device;
  (void)stream;
#endif
  *out = c;
  return FLTX_OK;
}

int fltx_ctx_destroy(fltx_ctx* ctx) {
  if (!ctx) {
    return FLTX_OK;
  }
  DeviceScope devScope(ctx);
  { /* the n-gram tables uploaded for this context die with it (a later context may get this address) */
    std::lock_guard<std::mutex> reg(g_lmRegMu);
    for (fltx_lm* lm : g_lmReg) {
      std::lock_guard<std::mutex> lock(lm->devMu);
      lm->dev.erase(ctx->uid);
    }
  }
#ifndef FLTX_EMU
  if (ctx->ownStream) {
    (void)hipStreamDestroy(ctx->stream);
  }
#endif
  delete ctx;
  return FLTX_OK;
}

int fltx_ctx_synchronize(fltx_ctx* ctx) {
  if (!ctx) {
    return fail(FLTX_ERR_INVALID, "null ctx");
  }
  return devSync(ctx->stream) ? fail(FLTX_ERR_HIP, "stream synchronize failed: %s", devErr()) : FLTX_OK;
}

void* fltx_ctx_stream(fltx_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
uint64_t fltx_ctx_uid(fltx_ctx* ctx) { return ctx ? ctx->uid : 0; }

/* ---- LM ------------------------------------------------------------------ */
int fltx_lm_zero_create(fltx_ctx* ctx, fltx_lm** out) {
  if (!out) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_zero_create: null argument");
  }
  auto* lm = new fltx_lm();
  lm->ctx = ctx;
  lm->kind = 0;
  {
    std::lock_guard<std::mutex> reg(g_lmRegMu);
    g_lmReg.insert(lm);
  }
  *out = lm;
  return FLTX_OK;
}

/* a user subclass of LM behind callbacks (include/fltx.h): nothing to upload */
int fltx_lm_host_create(const fltx_host_lm* cb, fltx_lm** out) {
  if (!cb || !out || !cb->start || !cb->score) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_host_create: null argument (start and score are required)");
  }
  auto* lm = new fltx_lm();
  lm->kind = 2;
  lm->host = *cb;
  {
    std::lock_guard<std::mutex> lock(g_lmRegMu);
    g_lmReg.insert(lm);
  }
  *out = lm;
  return FLTX_OK;
}

/* an LM whose answers arrive per step as rows (fltx_s2s_step_lm_rows): only the map is kept */
int fltx_lm_rows_create(int32_t lmWidth, const int32_t* usrToLm, int32_t nUsr, int32_t finishIndex, fltx_lm** out) {
  if (!out || lmWidth < 0 || finishIndex < -1 || (usrToLm && nUsr < 0)) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_rows_create: bad argument");
  }
  if (lmWidth > kS2sMaxV) {
    return fail(FLTX_ERR_UNSUPPORTED, "fltx_lm_rows_create: lm_width %d > %d", lmWidth, kS2sMaxV);
  }
  if (lmWidth > 0 && finishIndex >= lmWidth) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_rows_create: finish_index %d outside [0, %d)", finishIndex, lmWidth);
  }
  if (usrToLm && lmWidth > 0) {
    for (int32_t u = 0; u < nUsr; ++u) {
      if (usrToLm[u] < 0 || usrToLm[u] >= lmWidth) {
        return fail(FLTX_ERR_INVALID, "fltx_lm_rows_create: usr_to_lm[%d] = %d outside [0, %d)", u, usrToLm[u], lmWidth);
      }
    }
  }
  auto* lm = new fltx_lm();
  lm->kind = 3;
  lm->rowsWidth = lmWidth;
  lm->rowsFinish = finishIndex;
  lm->rowsMap = usrToLm != nullptr;
  if (usrToLm) {
    lm->hUsr.assign(usrToLm, usrToLm + nUsr);
    lm->nUsr = nUsr;
  }
  {
    std::lock_guard<std::mutex> lock(g_lmRegMu);
    g_lmReg.insert(lm);
  }
  *out = lm;
  return FLTX_OK;
}

/* a word-level rows LM (fltx_s2s_step_word_lm_rows): the word map and the finish index; the trie's labels are checked
 * against them where the trie is known, at fltx_s2s_lex_decoder_create */
int fltx_lm_word_rows_create(int32_t lmWidth, const int32_t* wordToLm, int32_t nWords, int32_t finishIndex,
                             fltx_lm** out) {
  if (!out || lmWidth <= 0 || finishIndex < 0 || (wordToLm && nWords < 0)) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_word_rows_create: bad argument (lm_width > 0 and finish_index >= 0 are required)");
  }
  if (lmWidth > kS2lMaxLmWidth) {
    return fail(FLTX_ERR_UNSUPPORTED, "fltx_lm_word_rows_create: lm_width %d > %d", lmWidth, kS2lMaxLmWidth);
  }
  auto* lm = new fltx_lm();
  lm->kind = 4;
  lm->rowsWidth = lmWidth;
  lm->rowsFinish = finishIndex;
  lm->rowsMap = wordToLm != nullptr;
  if (wordToLm) {
    lm->hUsr.assign(wordToLm, wordToLm + nWords);
    lm->nUsr = nWords;
  }
  {
    std::lock_guard<std::mutex> lock(g_lmRegMu);
    g_lmReg.insert(lm);
  }
  *out = lm;
  return FLTX_OK;
}

int fltx_lm_ngram_create(fltx_ctx* ctx, int32_t order, int64_t nNgrams, const int32_t* ngOrder,
                         const int32_t* ngWords, const float* prob, const float* backoff,
                         const int32_t* usrToLm, int32_t nUsr, int32_t bos, int32_t eos,
                         int32_t unk, fltx_lm** out) {
  if (!out || !ngOrder || !ngWords || !prob || !backoff || nNgrams <= 0) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_ngram_create: null argument");
  }
  if (order < 1 || order > kMaxNgramOrder) {
    return fail(FLTX_ERR_UNSUPPORTED, "n-gram order %d outside 1..%d (FL_TEXT_KENLM_MAX_ORDER)", order,
                kMaxNgramOrder);
  }
  if (nUsr < 0 || (nUsr > 0 && !usrToLm)) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_ngram_create: usr_to_lm is null for n_usr = %d", nUsr);
  }
  for (int32_t u = 0; u < nUsr; ++u) {
    if (usrToLm[u] < 0) {
      return fail(FLTX_ERR_INVALID, "fltx_lm_ngram_create: usr_to_lm[%d] = %d is negative", u, usrToLm[u]);
    }
  }
  /* forward trie of n-grams: node id per n-gram, (context node, word) -> node */
  struct HostNode {
    float prob;
    float backoff;
    bool phantom;
  };
  std::vector<HostNode> nodes(1, HostNode{0, 0, true}); /* node 0 = empty context */
  std::unordered_map<uint64_t, uint32_t> kids;
  kids.reserve((size_t)nNgrams * 2);
  std::vector<uint32_t> entCtx, entWord, entNode;
  auto childOf = [&](uint32_t ctxNode, uint32_t word, bool create) -> uint32_t {
    uint64_t k = ((uint64_t)ctxNode << 32) | word;
    auto it = kids.find(k);
    if (it != kids.end()) {
      return it->second;
    }
    if (!create) {
      return 0;
    }
    uint32_t id = (uint32_t)nodes.size();
    nodes.push_back(HostNode{0, 0, true});
    kids.emplace(k, id);
    entCtx.push_back(ctxNode);
    entWord.push_back(word);
    entNode.push_back(id);
    return id;
  };
  for (int64_t i = 0; i < nNgrams; ++i) {
    int k = ngOrder[i];
    if (k < 1 || k > order) {
      return fail(FLTX_ERR_INVALID, "n-gram %lld has order %d", (long long)i, k);
    }
    const int32_t* wds = ngWords + i * order;
    uint32_t node = 0;
    for (int j = 0; j < k; ++j) {
      if (wds[j] < 0) {
        return fail(FLTX_ERR_INVALID, "n-gram %lld has a negative word id", (long long)i);
      }
      node = childOf(node, (uint32_t)wds[j], true); /* missing prefixes become phantoms */
    }
    nodes[node].prob = prob[i];
    nodes[node].backoff = backoff[i];
    nodes[node].phantom = false;
  }
  if (nodes.size() >= 0x7FFFFFFFull) {
    return fail(FLTX_ERR_UNSUPPORTED, "too many n-grams");
  }
  auto* lm = new fltx_lm();
  lm->ctx = ctx;
  lm->kind = 1;
  lm->order = order;
  lm->bos = bos;
  lm->eos = eos;
  lm->unk = unk;
  lm->nUsr = nUsr;
  /* (4x slots: 2^31 slots of 16 B is what the 32-bit slot index reaches; a model beyond 2^29 n-grams takes 2x) */
  const uint64_t wantSlots = (uint64_t)entNode.size() * ((uint64_t)entNode.size() * 4 + 16 <= (1ull << 31) ? 4 : 2) + 16;
  if (wantSlots > (1ull << 31)) {
    return fail(FLTX_ERR_UNSUPPORTED, "too many n-grams for the 32-bit slot index of the look-up table");
  }
  uint32_t cap = nextPow2(wantSlots); /* at most a quarter full: a look-up is a chain of dependent trips to HBM, one more per occupied slot it meets (C4: 2x -> 4x slots = -4 % on the whole kernel) */
  lm->mask = cap - 1;
  lm->hTab.assign(cap, NgramSlot{0, kEmpty, 0, 0.0f});
  for (size_t e = 0; e < entNode.size(); ++e) {
    uint32_t s = hashKey(entCtx[e], entWord[e], 0x5bd1e995u, 0) & lm->mask;
    while (lm->hTab[s].word != kEmpty) {
      s = (s + 1) & lm->mask;
    }
    const HostNode& nd = nodes[entNode[e]];
    lm->hTab[s] = NgramSlot{entCtx[e], entWord[e], entNode[e] | (nd.phantom ? kPhantomNode : 0u), nd.prob};
  }
  lm->hBackoff.resize(nodes.size());
  for (size_t i = 0; i < nodes.size(); ++i) {
    lm->hBackoff[i] = nodes[i].phantom ? 0.0f : nodes[i].backoff;
  }
  lm->hUsr.assign(usrToLm, usrToLm + (usrToLm ? nUsr : 0));
  /* the tables go to HBM when a decoder is created on a context */
  {
    std::lock_guard<std::mutex> reg(g_lmRegMu);
    g_lmReg.insert(lm);
  }
  *out = lm;
  return FLTX_OK;
}

int fltx_lm_destroy(fltx_lm* lm) {
  if (lm) {
    std::lock_guard<std::mutex> reg(g_lmRegMu);
    g_lmReg.erase(lm);
  }
  delete lm;
  return FLTX_OK;
}

/* host walk over the same flat tables the kernels use (known-answer checks of
 * the table builder; decode-time scoring always happens on the device) */
int fltx_lm_score_sequence(fltx_lm* lm, const int32_t* usrWords, int32_t n, int32_t withFinish,
                           float* perWord, float* total) {
  if (!lm || (!usrWords && n > 0)) {
    return fail(FLTX_ERR_INVALID, "fltx_lm_score_sequence: null argument");
  }
  if (lm->kind == 2) {
    return fail(FLTX_ERR_UNSUPPORTED, "a host LM keeps its own states (call the LM object)");
  }
  if (lm->kind == 3 || lm->kind == 4) {
    return fail(FLTX_ERR_UNSUPPORTED, "a rows LM has no states here: its answers arrive with fltx_s2s_step_lm_rows");
  }
  float tot = 0;
  if (lm->kind == 0) {
    for (int i = 0; i < n; ++i) {
      if (perWord) {
        perWord[i] = 0.0f;
      }
    }
    if (total) {
      *total = 0;
    }
    return FLTX_OK;
  }
  const int L = lm->order - 1;
  auto find = [&](uint32_t ctx, uint32_t word, uint32_t& node, float& pr) {
    uint32_t s = hashKey(ctx, word, 0x5bd1e995u, 0) & lm->mask;
    for (;;) {
      const NgramSlot& e = lm->hTab[s];
      if (e.word == kEmpty) {
        return false;
      }
      if (e.ctx == ctx && e.word == word) {
        node = e.node;
        pr = e.prob;
        return true;
      }
      s = (s + 1) & lm->mask;
    }
  };
  std::vector<int32_t> ctx(std::max(L, 1), 0), nxt(std::max(L, 1), 0);
  {
    uint32_t nd;
    float pr;
    if (L > 0 && find(0, (uint32_t)lm->bos, nd, pr)) {
      ctx[0] = (int32_t)(nd & ~kPhantomNode);
    }
  }
  auto score = [&](uint32_t word) {
    std::vector<uint32_t> nodes(L + 1, 0);
    std::vector<char> found(L + 1, 0);
    float prob = 0;
    int longest = -1;
    for (int k = 0; k <= L; ++k) {
      uint32_t c = k == 0 ? 0u : (uint32_t)ctx[k - 1];
      if (k > 0 && c == 0) {
        continue;
      }
      float pr;
      if (find(c, word, nodes[k], pr)) {
        found[k] = 1;
        if (!(nodes[k] & kPhantomNode)) {
          longest = k;
          prob = pr;
        }
        nodes[k] &= ~kPhantomNode;
      }
    }
    if (longest < 0) {
      uint32_t nd = 0;
      if (!find(0, (uint32_t)lm->unk, nd, prob)) {
        prob = -100.0f;
      }
      nodes[0] = nd & ~kPhantomNode;
      found[0] = 1;
      longest = 0;
    }
    for (int j = longest + 1; j <= L; ++j) {
      uint32_t c = (uint32_t)ctx[j - 1];
      if (c != 0) {
        prob += lm->hBackoff[c];
      }
    }
    for (int j = 0; j < L; ++j) {
      nxt[j] = (j <= longest && found[j]) ? (int32_t)nodes[j] : 0;
    }
    ctx = nxt;
    return prob;
  };
  for (int i = 0; i < n; ++i) {
    int u = usrWords[i];
    if (u < 0 || u >= lm->nUsr) {
      return fail(FLTX_ERR_RANGE, "[ngram LM] Invalid user token index: %d", u); /* KenLM.cpp:66-69 */
    }
    float s = score((uint32_t)lm->hUsr[u]);
    if (perWord) {
      perWord[i] = s;
    }
    tot += s;
  }
  if (withFinish) {
    tot += score((uint32_t)lm->eos);
  }
  if (total) {
    *total = tot;
  }
  return FLTX_OK;
}

/* LM::start / LM::score / LM::finish on explicit states (decoder/lm/LM.h:61-78),
 * host walk over the flat tables.  A state is lmOrder-1 context node ids. */
static bool lmFind(const fltx_lm* lm, uint32_t ctx, uint32_t word, uint32_t& node, float& pr) {
  uint32_t s = hashKey(ctx, word, 0x5bd1e995u, 0) & lm->mask;
  for (;;) {
    const NgramSlot& e = lm->hTab[s];
    if (e.word == kEmpty) {
      return false;
    }
    if (e.ctx == ctx && e.word == word) {
      node = e.node;
      pr = e.prob;
      return true;
    }
    s = (s + 1) & lm->mask;
  }
}

int fltx_lm_state_size(fltx_lm* lm, int32_t* n) {
  if (!lm || !n) {
    return fail(FLTX_ERR_INVALID, "null argument");
  }
  if (lm->kind == 2) {
    return fail(FLTX_ERR_UNSUPPORTED, "a host LM keeps its own states (call the LM object)");
  }
  if (lm->kind == 3 || lm->kind == 4) {
    return fail(FLTX_ERR_UNSUPPORTED, "a rows LM has no states here: its answers arrive with fltx_s2s_step_lm_rows");
  }
  *n = lm->kind == 0 ? 0 : std::max(1, lm->order - 1);
  return FLTX_OK;
}

int fltx_lm_start(fltx_lm* lm, int32_t startWithNothing, int32_t* ctxOut) {
  if (!lm) {
    return fail(FLTX_ERR_INVALID, "null lm");
  }
  if (lm->kind == 2) {
    return fail(FLTX_ERR_UNSUPPORTED, "a host LM keeps its own states (call the LM object)");
  }
  if (lm->kind == 3 || lm->kind == 4) {
    return fail(FLTX_ERR_UNSUPPORTED, "a rows LM has no states here: its answers arrive with fltx_s2s_step_lm_rows");
  }
  if (lm->kind == 0) {
    return FLTX_OK;
  }
  const int L = std::max(1, lm->order - 1);
  for (int j = 0; j < L; ++j) {
    ctxOut[j] = 0;
  }
  uint32_t nd;
  float pr;
  if (!startWithNothing && lm->order > 1 && lmFind(lm, 0, (uint32_t)lm->bos, nd, pr)) {
    ctxOut[0] = (int32_t)(nd & ~kPhantomNode); /* BeginSentenceWrite, KenLM.cpp:57 */
  }
  return FLTX_OK;
}

/* log10 p(word | context) and the context after it: the host twin of ngScore (fltx_kernels.h), same tables, same
 * order of the float additions.  ctxOut may alias ctxIn. */
static float lmStepWord(const fltx_lm* lm, const int32_t* ctxIn, uint32_t word, int32_t* ctxOut) {
  const int L = lm->order - 1;
  uint32_t nodes[kMaxNgramOrder] = {0};
  bool found[kMaxNgramOrder] = {false};
  float prob = 0;
  int longest = -1;
  for (int k = 0; k <= L; ++k) {
    const uint32_t c = k == 0 ? 0u : (uint32_t)ctxIn[k - 1];
    if (k > 0 && c == 0) {
      continue;
    }
    float pr;
    if (lmFind(lm, c, word, nodes[k], pr)) {
      found[k] = true;
      if (!(nodes[k] & kPhantomNode)) {
        longest = k;
        prob = pr;
      }
      nodes[k] &= ~kPhantomNode;
    }
  }
  if (longest < 0) {
    uint32_t nd = 0;
    if (!lmFind(lm, 0, (uint32_t)lm->unk, nd, prob)) {
      prob = -100.0f;
    }
    nodes[0] = nd & ~kPhantomNode;
    found[0] = true;
    longest = 0;
  }
  for (int j = longest + 1; j <= L; ++j) {
    const uint32_t c = (uint32_t)ctxIn[j - 1];
    if (c != 0) {
      prob += lm->hBackoff[c];
    }
  }
  if (ctxOut) {
    int32_t tmp[kMaxNgramOrder];
    for (int j = 0; j < L; ++j) {
      tmp[j] = (j <= longest && found[j]) ? (int32_t)nodes[j] : 0;
    }
    for (int j = 0; j < std::max(1, L); ++j) {
      ctxOut[j] = j < L ? tmp[j] : 0;
    }
  }
  return prob;
}

/* usr_idx >= 0: LM::score; usr_idx == -1: LM::finish (scores </s>) */
int fltx_lm_step(fltx_lm* lm, const int32_t* ctxIn, int32_t usrIdx, int32_t* ctxOut, float* score) {
  if (!lm || !score) {
    return fail(FLTX_ERR_INVALID, "null argument");
  }
  if (lm->kind == 2) {
    return fail(FLTX_ERR_UNSUPPORTED, "a host LM keeps its own states (call the LM object)");
  }
  if (lm->kind == 3 || lm->kind == 4) {
    return fail(FLTX_ERR_UNSUPPORTED, "a rows LM has no states here: its answers arrive with fltx_s2s_step_lm_rows");
  }
  if (lm->kind == 0) {
    *score = 0.0f;
    return FLTX_OK;
  }
  uint32_t word;
  if (usrIdx == -1) {
    word = (uint32_t)lm->eos;
  } else {
    if (usrIdx < 0 || usrIdx >= lm->nUsr) {
      return fail(FLTX_ERR_RANGE, "[ngram LM] Invalid user token index: %d", usrIdx); /* KenLM.cpp:66-69 */
    }
    word = (uint32_t)lm->hUsr[usrIdx];
  }
  *score = lmStepWord(lm, ctxIn, word, ctxOut);
  return FLTX_OK;
}

/* ---- trie ---------------------------------------------------------------- */
int fltx_trie_create(fltx_ctx* ctx, int64_t nNodes, int32_t nTokens, const int32_t* child,
                     const float* maxScore, const int32_t* labelOff, const int32_t* labels,
                     fltx_trie** out) {
  if (!ctx || !out || !child || !maxScore || !labelOff || nNodes <= 0 || nTokens <= 0) {
    return fail(FLTX_ERR_INVALID, "fltx_trie_create: null or empty argument");
  }
  if (nNodes >= (1ll << 31)) {
    return fail(FLTX_ERR_UNSUPPORTED, "trie too large");
  }
  EntryScope entry(ctx);
  if (entry.rc) {
    return entry.rc;
  }
  if (nNodes >= (1ll << 28) || (int64_t)labelOff[nNodes] >= (1ll << 28)) {
    return fail(FLTX_ERR_UNSUPPORTED, "trie too large for the packed edge records");
  }
  std::vector<int32_t> nKids((size_t)nNodes, 0);
  for (int64_t i = 0; i < nNodes; ++i) {
    for (int t = 0; t < nTokens; ++t) {
      const int32_t c = child[i * nTokens + t];
      if (c >= nNodes) {
        return fail(FLTX_ERR_RANGE, "trie child index %d out of range", c);
      }
      nKids[i] += c >= 0;
    }
    const int nl = labelOff[i + 1] - labelOff[i];
    if (nl < 0 || nl > 6) {
      return fail(FLTX_ERR_INVALID, "trie node %lld has %d labels (kTrieMaxLabel = 6)", (long long)i, nl);
    }
  }
  std::vector<TrieEdge> edge((size_t)nNodes * nTokens);
  for (int64_t i = 0; i < nNodes; ++i) {
    for (int t = 0; t < nTokens; ++t) {
      const int32_t c = child[i * nTokens + t];
      TrieEdge e{-1, 0.0f, -1, 0u};
      if (c >= 0) {
        const int nl = labelOff[c + 1] - labelOff[c];
        e.child = c;
        e.childMax = maxScore[c];
        e.label0 = nl > 0 ? labels[labelOff[c]] : -1;
        e.meta = (uint32_t)nl | (nKids[c] > 0 ? 8u : 0u) | ((uint32_t)labelOff[c] << 4);
      }
      edge[(size_t)i * nTokens + t] = e;
    }
  }
  /* per node: which tokens have a child (the generic engine lists only those) */
  std::vector<unsigned long long> cmask;
  if (nTokens <= 64) {
    cmask.assign((size_t)nNodes, 0ull);
    for (int64_t i = 0; i < nNodes; ++i) {
      for (int t = 0; t < nTokens; ++t) {
        if (child[i * nTokens + t] >= 0) {
          cmask[(size_t)i] |= 1ull << t;
        }
      }
    }
  }
  auto* t = new fltx_trie();
  t->ctx = ctx;
  t->nNodes = nNodes;
  t->nTokens = nTokens;
  Stream st = ctx->stream;
  size_t nLab = (size_t)labelOff[nNodes];
  /* breadth-first layout (see fltx_trie::xnode) */
  std::vector<XNode> xn;
  std::vector<float> xdHost;
  if (nTokens <= 64 && !cmask.empty()) {
    std::vector<int64_t> order; /* new id -> old id */
    std::vector<int32_t> tokOf((size_t)nNodes, -1);
    std::vector<uint32_t> parentOf((size_t)nNodes + 1, 0u); /* by new id */
    order.reserve((size_t)nNodes);
    order.push_back(0);
    xn.resize((size_t)nNodes);
    bool ok = true, multi = false;
    int endTok = -1;
    bool zero = true;
    std::vector<uint32_t> xextraHost((size_t)nNodes, 0u);
    std::vector<uint8_t> seen((size_t)nNodes, 0);
    seen[0] = 1;
    for (size_t q = 0; q < order.size() && ok; ++q) {
      const int64_t o = order[q];
      XNode x;
      memset(&x, 0, sizeof(x));
      x.childMask = cmask[(size_t)o];
      x.firstChild = (uint32_t)order.size();
      x.maxScore = maxScore[o];
      x.endLabel0 = -1;
      x.parent = parentOf[q];
      zero = zero && maxScore[o] == 0.0f;
      for (int tk = 0; tk < nTokens; ++tk) {
        const int32_t c = child[o * nTokens + tk];
        if (c < 0) {
          continue;
        }
        if (seen[(size_t)c] || order.size() >= (size_t)nNodes) { /* not a tree (shared suffix, back edge): */
          ok = false;                                            /* no breadth-first layout, generic engine only */
          break;
        }
        seen[(size_t)c] = 1;
        parentOf[order.size()] = (uint32_t)q;
        order.push_back(c);
        tokOf[(size_t)c] = tk;
        if (nKids[(size_t)c] > 0) {
          x.kidsMask |= 1ull << tk;
        }
        const int nl = labelOff[c + 1] - labelOff[c];
        if (nl > 0) {
          if (endTok < 0) {
            endTok = tk;
          }
          ok = ok && tk == endTok && nl <= 6 && labelOff[c] < (1 << 28); /* one word-ending token; Trie.h:19: at most 6 words per spelling */
          x.endLabel0 = labels[labelOff[c]];
          xextraHost[q] = ((uint32_t)labelOff[c] << 3) | (uint32_t)nl;
          multi = multi || nl > 1;
        }
      }
      xn[q] = x;
    }
    std::vector<float> xd(xn.size(), 0.0f);
    for (size_t q = 1; ok && q < order.size() && q < xd.size(); ++q) { /* lex->maxScore - lexMaxScore, LexiconDecoder.cpp:47,96 */
      const uint32_t pq = xn[q].parent;
      xd[q] = xn[q].maxScore - (pq == 0u ? 0.0f : xn[pq].maxScore);
    }
    ok = ok && order.size() == (size_t)nNodes && (labelOff[1] - labelOff[0]) == 0; /* a tree; no label on the root */
    t->xOk = ok;
    t->xMulti = ok && multi;
    t->xEndTok = endTok;
    if (ok && multi) {
      if (t->xextra.ensure(sizeof(uint32_t) * xextraHost.size(), st, false) ||
          devCopyH2D(t->xextra.p, xextraHost.data(), sizeof(uint32_t) * xextraHost.size(), st) || devSync(st)) {
        delete t;
        return fail(FLTX_ERR_OOM, "trie upload: labels of the spellings");
      }
    }
    t->xZeroSmear = zero;
    if (!ok) {
      xn.clear();
      xd.clear();
    }
    for (float v : xd) {
      t->xDeltaMin = std::min(t->xDeltaMin, v);
      t->xDeltaMax = std::max(t->xDeltaMax, v);
    }
    t->xEndHost.resize(xn.size());
    for (size_t q = 0; q < xn.size(); ++q) {
      t->xEndHost[q] = xn[q].endLabel0;
    }
    xdHost.swap(xd);
  }
  if (!xn.empty()) {
    if (t->xnode.ensure(sizeof(XNode) * xn.size(), st, false) ||
        devCopyH2D(t->xnode.p, xn.data(), sizeof(XNode) * xn.size(), st)) {
      delete t;
      return fail(FLTX_ERR_OOM, "trie: breadth-first layout upload failed");
    }
    if (t->xdelta.ensure(sizeof(float) * xdHost.size(), st, false) ||
        devCopyH2D(t->xdelta.p, xdHost.data(), sizeof(float) * xdHost.size(), st)) {
      delete t;
      return fail(FLTX_ERR_OOM, "trie: breadth-first layout upload failed");
    }
  }
  if (!cmask.empty()) {
    if (t->mask.ensure(8 * cmask.size(), st, false) ||
        devCopyH2D(t->mask.p, cmask.data(), 8 * cmask.size(), st)) {
      delete t;
      return fail(FLTX_ERR_OOM, "trie: child-mask upload failed");
    }
  }
  if (t->edge.ensure(sizeof(TrieEdge) * edge.size(), st, false) ||
      t->labels.ensure(sizeof(int32_t) * std::max<size_t>(1, nLab), st, false)) {
    delete t;
    return fail(FLTX_ERR_OOM, "trie: device allocation failed");
  }
  if (devCopyH2D(t->edge.p, edge.data(), sizeof(TrieEdge) * edge.size(), st) ||
      (nLab && devCopyH2D(t->labels.p, labels, sizeof(int32_t) * nLab, st)) || devSync(st)) {
    delete t;
    return fail(FLTX_ERR_HIP, "trie: upload failed");
  }
  *out = t;
  return FLTX_OK;
}

int fltx_trie_destroy(fltx_trie* t) {
  delete t;
  return FLTX_OK;
}

/* upload the flat n-gram tables to the context's device (once) */
static int lmEnsureUploaded(fltx_lm* lm, fltx_ctx* ctx, fltx_lm::Dev** out) {
  *out = nullptr;
  if (lm->kind != 1 && !((lm->kind == 3 || lm->kind == 4) && lm->rowsMap)) {
    return FLTX_OK; /* (ZeroLM: nothing to compute; host LM: answered on the host; rows LM without a map: identity) */
  }
  std::lock_guard<std::mutex> lock(lm->devMu);
  auto it = lm->dev.find(ctx->uid);
  if (it != lm->dev.end()) {
    *out = it->second.get();
    return FLTX_OK;
  }
  std::unique_ptr<fltx_lm::Dev> dv(new fltx_lm::Dev());
  Stream st = ctx->stream;
  if (lm->kind == 3 || lm->kind == 4) { /* a rows LM: the map alone */
    const size_t nb = sizeof(int32_t) * std::max<size_t>(1, lm->hUsr.size());
    if (dv->usrToLm.ensure(nb, st, false)) {
      return fail(FLTX_ERR_OOM, "rows LM: device allocation failed");
    }
    if ((!lm->hUsr.empty() && devCopyH2D(dv->usrToLm.p, lm->hUsr.data(), sizeof(int32_t) * lm->hUsr.size(), st)) ||
        devSync(st)) {
      return fail(FLTX_ERR_HIP, "rows LM: upload failed");
    }
    *out = dv.get();
    lm->dev[ctx->uid] = std::move(dv);
    return FLTX_OK;
  }
  const size_t cap = lm->hTab.size(), nn = lm->hBackoff.size();
  if (dv->tab.ensure(sizeof(NgramSlot) * cap, st, false) || dv->backoff.ensure(sizeof(float) * nn, st, false) ||
      dv->usrToLm.ensure(sizeof(int32_t) * std::max<size_t>(1, lm->hUsr.size()), st, false)) {
    return fail(FLTX_ERR_OOM, "n-gram tables: device allocation failed");
  }
  if (devCopyH2D(dv->tab.p, lm->hTab.data(), sizeof(NgramSlot) * cap, st) ||
      devCopyH2D(dv->backoff.p, lm->hBackoff.data(), sizeof(float) * nn, st) ||
      (!lm->hUsr.empty() && devCopyH2D(dv->usrToLm.p, lm->hUsr.data(), sizeof(int32_t) * lm->hUsr.size(), st)) ||
      devSync(st)) {
    return fail(FLTX_ERR_HIP, "n-gram tables: upload failed");
  }
  *out = dv.get();
  lm->dev[ctx->uid] = std::move(dv);
  return FLTX_OK;
}

/* The dense (context, token) table of an n-gram LM over N tokens (fltx_lm::TokDense), built once per (LM, N) and
 * uploaded once per context.  *out = null (and FLTX_OK): the model has too many contexts for a dense table. */
constexpr int64_t kTokDenseMaxCtx = 1ll << 24;      /* contexts */
constexpr int64_t kTokDenseMaxBytes = 1ll << 35;    /* 32 GB of the device's 288 (a character LM: 240 B per context) */
static int lmTokDense(fltx_lm* lm, fltx_ctx* ctx, fltx_lm::Dev* dv, int N, const int2** out, int64_t* nCtxOut) {
  *out = nullptr;
  if (lm->kind != 1 || !dv || N <= 0) {
    return FLTX_OK;
  }
  std::lock_guard<std::mutex> lock(lm->devMu);
  auto it = lm->tokDense.find(N);
  if (it == lm->tokDense.end()) {
    std::unique_ptr<fltx_lm::TokDense> td(new fltx_lm::TokDense());
    const int L = std::max(1, lm->order - 1);
    const int stride = N + 1;
    const int64_t capCtx = std::min<int64_t>(kTokDenseMaxCtx, kTokDenseMaxBytes / (8 * (int64_t)stride));
    /* contexts in the order they are first reached: row 0 = KenLM::start(false) (KenLM.cpp:52-61).  Rows live in one
     * flat array, their ids in an open-addressing table keyed by the L node ids; the frontier is scored a block of
     * rows at a time by the host's threads (the LM tables are read-only), the new contexts are numbered by one thread
     * in row order afterwards -- so the numbering does not depend on the number of threads.  (A 5-gram over 29 tokens
     * with 390 k contexts: 8.1 s with a std::map and one thread before; the caps below are what this has to reach.) */
    std::vector<int32_t> rows((size_t)L, 0); /* row r = rows[r * L .. r * L + L) */
    {
      uint32_t nd;
      float pr;
      if (lm->order > 1 && lmFind(lm, 0, (uint32_t)lm->bos, nd, pr)) {
        rows[0] = (int32_t)(nd & ~kPhantomNode);
      }
    }
    int64_t nRows = 1;
    std::vector<int32_t> slots((size_t)1 << 16, -1);
    auto hashOf = [&](const int32_t* c) {
      uint64_t h = 0x9E3779B97F4A7C15ull;
      for (int k = 0; k < L; ++k) {
        h = (h ^ (uint64_t)(uint32_t)c[k]) * 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
      }
      return h;
    };
    auto place = [&](int32_t id) { /* (table with room: the caller grows it) */
      const uint64_t mask = slots.size() - 1;
      uint64_t h = hashOf(&rows[(size_t)id * L]) & mask;
      while (slots[h] >= 0) {
        h = (h + 1) & mask;
      }
      slots[h] = id;
    };
    place(0);
    auto findOrAdd = [&](const int32_t* c, bool& full) -> int32_t {
      const uint64_t mask = slots.size() - 1;
      uint64_t h = hashOf(c) & mask;
      while (slots[h] >= 0) {
        if (memcmp(&rows[(size_t)slots[h] * L], c, sizeof(int32_t) * (size_t)L) == 0) {
          return slots[h];
        }
        h = (h + 1) & mask;
      }
      if (nRows >= capCtx) {
        full = true;
        return 0;
      }
      const int32_t id = (int32_t)nRows++;
      rows.insert(rows.end(), c, c + L);
      slots[h] = id;
      if ((uint64_t)nRows * 2 > slots.size()) {
        slots.assign(slots.size() * 4, -1);
        for (int32_t r = 0; r < (int32_t)nRows; ++r) {
          place(r);
        }
      }
      return id;
    };
    bool tooMany = false;
    const int nThr = (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    constexpr int64_t kBlock = 1 << 14; /* rows scored between two numbering passes */
    std::vector<int32_t> nxt((size_t)kBlock * (size_t)N * (size_t)L);
    for (int64_t r0 = 0, r1 = 0; r0 < nRows && !tooMany; r0 = r1) {
      r1 = std::min(nRows, r0 + kBlock);
      td->tab.resize((size_t)r1 * (size_t)stride);
      auto scoreRows = [&](int64_t a, int64_t b2) {
        for (int64_t r = a; r < b2; ++r) {
          const int32_t* cur = &rows[(size_t)r * L];
          for (int n = 0; n <= N; ++n) {
            /* KenLM::score: usrToLmIdxMap_, an index beyond the dictionary goes to <unk> as on the device (lmScoreDev);
             * column N: KenLM::finish = the score of </s> */
            const uint32_t word = n == N ? (uint32_t)lm->eos : (n < lm->nUsr ? (uint32_t)lm->hUsr[(size_t)n] : (uint32_t)lm->unk);
            int32_t tmp[kMaxNgramOrder];
            const float sc = lmStepWord(lm, cur, word, tmp);
            if (n < N) {
              memcpy(&nxt[((size_t)(r - r0) * (size_t)N + (size_t)n) * (size_t)L], tmp, sizeof(int32_t) * (size_t)L);
            }
            uint32_t bits;
            memcpy(&bits, &sc, 4);
            td->tab[(size_t)r * (size_t)stride + (size_t)n] = make_int2((int)bits, 0);
          }
        }
      };
      const int64_t per = (r1 - r0 + nThr - 1) / nThr;
      if (nThr == 1 || r1 - r0 < 256) {
        scoreRows(r0, r1);
      } else {
        std::vector<std::thread> pool;
        for (int64_t a = r0; a < r1; a += per) {
          pool.emplace_back(scoreRows, a, std::min(r1, a + per));
        }
        for (auto& th : pool) {
          th.join();
        }
      }
      for (int64_t r = r0; r < r1 && !tooMany; ++r) { /* (rows may move: `rows` grows) */
        for (int n = 0; n < N; ++n) {
          const int32_t to = findOrAdd(&nxt[((size_t)(r - r0) * (size_t)N + (size_t)n) * (size_t)L], tooMany);
          if (tooMany) {
            break;
          }
          td->tab[(size_t)r * (size_t)stride + (size_t)n].y = to;
        }
      }
    }
    if (tooMany) {
      td->nCtx = -1;
      td->tab.clear();
      td->tab.shrink_to_fit();
    } else {
      td->nCtx = nRows;
    }
    it = lm->tokDense.emplace(N, std::move(td)).first;
  }
  const fltx_lm::TokDense& td = *it->second;
  if (td.nCtx <= 0) {
    return FLTX_OK;
  }
  auto dit = dv->tokDense.find(N);
  if (dit == dv->tokDense.end()) {
    std::unique_ptr<DBuf> buf(new DBuf());
    Stream st = ctx->stream;
    if (buf->ensure(sizeof(int2) * td.tab.size(), st, false)) {
      return fail(FLTX_ERR_OOM, "dense token-LM table: device allocation failed");
    }
    if (devCopyH2D(buf->p, td.tab.data(), sizeof(int2) * td.tab.size(), st) || devSync(st)) {
      return fail(FLTX_ERR_HIP, "dense token-LM table: upload failed");
    }
    dit = dv->tokDense.emplace(N, std::move(buf)).first;
  }
  *out = dit->second->as<int2>();
  if (nCtxOut) {
    *nCtxOut = td.nCtx;
  }
  return FLTX_OK;
}

/* ---- decoder ------------------------------------------------------------- */
int fltx_decoder_create(fltx_ctx* ctx, int32_t kind, const fltx_options* opt, const fltx_trie* trie,
                        const fltx_lm* lm, int32_t sil, int32_t blank, int32_t unk,
                        const float* transitions, int32_t nTrans, int32_t isLmToken,
                        fltx_decoder** out) {
  if (!ctx || !opt || !lm || !out) {
    return fail(FLTX_ERR_INVALID, "fltx_decoder_create: null argument");
  }
  if (kind == FLTX_DECODER_CTC_ROWS) { /* (fltx_group_create comes through here too) */
    return fail(FLTX_ERR_UNSUPPORTED, "a CTC rows decoder is made with fltx_ctc_rows_decoder_create (no groups)");
  }
  if (kind == FLTX_DECODER_LEX_CTC_ROWS) {
    return fail(FLTX_ERR_UNSUPPORTED, "a lexicon CTC rows decoder is made with fltx_ctc_rows_lex_decoder_create (no groups)");
  }
  if (kind != FLTX_DECODER_LEXFREE && kind != FLTX_DECODER_LEXICON) {
    return fail(FLTX_ERR_INVALID, "unknown decoder kind %d", kind);
  }
  if (lm->kind == 3 || lm->kind == 4) {
    return fail(FLTX_ERR_UNSUPPORTED, "a rows LM (fltx_lm_rows_create, fltx_lm_word_rows_create) serves the seq2seq "
                                      "decoders, fltx_ctc_rows_decoder_create and fltx_ctc_rows_lex_decoder_create only");
  }
  if (kind == FLTX_DECODER_LEXICON && !trie) {
    return fail(FLTX_ERR_INVALID, "lexicon decoder needs a trie");
  }
  if (opt->beam_size < 1 || opt->beam_size_token < 1) {
    return fail(FLTX_ERR_INVALID, "beam_size and beam_size_token must be >= 1");
  }
  if (opt->beam_size > 0x7FFFFF) {
    return fail(FLTX_ERR_UNSUPPORTED, "beam_size too large");
  }
  if (opt->criterion != FLTX_CRITERION_ASG && opt->criterion != FLTX_CRITERION_CTC) {
    return fail(FLTX_ERR_UNSUPPORTED, "criterion %d not supported (ASG, CTC only)", opt->criterion);
  }
  if (trie && trie->ctx != ctx) {
    return fail(FLTX_ERR_INVALID, "fltx_decoder_create: the trie was uploaded to another context (device)");
  }
  EntryScope entry(ctx);
  if (entry.rc) {
    return entry.rc;
  }
  fltx_lm::Dev* lmDev = nullptr;
  {
    int rcu = lmEnsureUploaded(const_cast<fltx_lm*>(lm), ctx, &lmDev);
    if (rcu) {
      return rcu;
    }
  }
  auto* d = new fltx_decoder();
  d->lmDev = lmDev;
  d->ctx = ctx;
  d->kind = kind;
  d->opt = *opt;
  d->trie = trie;
  d->lm = lm;
  d->sil = sil;
  d->blank = blank;
  d->unk = unk;
  d->isLmToken = isLmToken ? 1 : 0;
  if (transitions && nTrans > 0) {
    d->nTrans = nTrans;
    d->transMax = 0.0;
    for (int i = 0; i < nTrans; ++i) {
      d->transMax = std::max(d->transMax, (double)transitions[i]);
    }
    if (d->transitions.ensure(sizeof(float) * (size_t)nTrans, ctx->stream, false) ||
        devCopyH2D(d->transitions.p, transitions, sizeof(float) * (size_t)nTrans, ctx->stream) ||
        devSync(ctx->stream)) {
      delete d;
      return fail(FLTX_ERR_HIP, "transitions upload failed");
    }
  }
  *out = d;
  return FLTX_OK;
}

int fltx_decoder_destroy(fltx_decoder* d) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (d) {
    devSync(d->ctx->stream);
#ifndef FLTX_EMU
    for (int i = 0; i < 3; ++i) {
      if (d->ev[i]) {
        (void)hipEventDestroy(d->ev[i]);
      }
    }
    if (d->lookEv) {
      (void)hipEventDestroy(d->lookEv);
    }
    if (d->copyStream) {
      (void)hipStreamSynchronize(d->copyStream);
      (void)hipEventDestroy(d->evSlotFree[0]);
      (void)hipEventDestroy(d->evSlotFree[1]);
      (void)hipStreamDestroy(d->copyStream);
    }
#endif
  }
  delete d;
  return FLTX_OK;
}

static int settlePendingLook(fltx_decoder* d); /* (defined after syncResults) */
/* the fltx_decoder_get keys of TrBufs::ms -> its slot, -1: none of them */
static int trTimedSlot(const char* key) {
  static const char* const kKeys[4] = {"transcript_count_ns", "transcript_scan_ns", "transcript_write_ns", "pack_ns"};
  for (int i = 0; i < 4; ++i) {
    if (!strcmp(key, kKeys[i])) {
      return i;
    }
  }
  return -1;
}
/* fltx_decoder_get "bt_prof_<what>" after a batch decoded with "bt_profile" = 1: shader clocks of the last narrow
 * back-trace summed over the utterances that took it -- copy0 (the first chunk into LDS), walk (the marking wave's own
 * share of the walk loop: walking, composing, copying), wait (its barrier waits in that loop), store (the widened token
 * rows), fetch0 (the first stretch of addends staged), score (the score loop), of which add is the first adding wave's own
 * time and addwait its waits at the stretch barriers (for the staging waves), total; utts = utterances counted */
static int btProfileGet(fltx_decoder* d, const char* what, int64_t* value) {
  if (!d->btProfile || !d->btProf.p || !d->backtraced) {
    return fail(FLTX_ERR_STATE, "no back-trace profile: fltx_decoder_set(dec, \"bt_profile\", 1) before the batch");
  }
  DeviceScope devScope(d->ctx);
  std::vector<unsigned long long> h((size_t)kBtProfMarks * d->B);
  if (devCopyD2H(h.data(), d->btProf.p, 8 * h.size(), d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "profile copy failed");
  }
  int64_t sum[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < d->B; ++b) {
    const unsigned long long* m = h.data() + (size_t)b * kBtProfMarks;
    if (!m[1]) {
      continue; /* (not a narrow back-trace: no marks) */
    }
    sum[0] += (int64_t)(m[1] - m[0]);
    unsigned long long prev = m[1];
    for (int c = 0; c < (int)m[6]; ++c) {
      sum[1] += (int64_t)(m[8 + 2 * c] - prev);
      sum[2] += (int64_t)(m[9 + 2 * c] - m[8 + 2 * c]);
      prev = m[9 + 2 * c];
    }
    sum[1] += (int64_t)(m[2] - prev); /* (the word rows of the last chunk; chunks beyond the marked ones) */
    sum[3] += (int64_t)(m[3] - m[2]);
    if (m[5]) {
      sum[4] += (int64_t)(m[4] - m[3]);
      sum[5] += (int64_t)(m[5] - m[4]);
      sum[8] += (int64_t)(m[5] - m[4]) - (int64_t)m[7];
      sum[9] += (int64_t)m[7];
    }
    sum[6] += (int64_t)((m[5] ? m[5] : m[3]) - m[0]);
    sum[7] += 1;
  }
  static const char* const kNames[10] = {"copy0", "walk", "wait", "store", "fetch0", "score", "total", "utts", "add", "addwait"};
  for (int i = 0; i < 10; ++i) {
    if (!strcmp(what, kNames[i])) {
      *value = sum[i];
      return FLTX_OK;
    }
  }
  return fail(FLTX_ERR_INVALID, "fltx_decoder_get: unknown key bt_prof_%s", what);
}

int fltx_decoder_get(fltx_decoder* d, const char* key, int64_t* value) {
  if (!d || !key || !value) {
    return fail(FLTX_ERR_INVALID, "fltx_decoder_get: null argument");
  }
  if (!strcmp(key, "engine")) { /* the engine the last call started on ("redone" counts what it handed on) */
    *value = d->engineFirst;
  } else if (!strcmp(key, "xlane")) {
    *value = d->xlaneFirst;
  } else if (!strcmp(key, "ylane")) {
    *value = d->ylaneFirst;
  } else if (!strcmp(key, "yshare")) {
    *value = (d->ylane || d->xlane) ? d->yshare : 0;
  } else if (!strcmp(key, "redone")) {
    if (d->offlinePending) { /* ("defer_check": the look has not happened yet) */
      DeviceScope devScope(d->ctx);
      int rc = settlePendingLook(d);
      if (rc) {
        return rc;
      }
    }
    *value = d->lastRedo;
  } else if (!strcmp(key, "sstream")) {
    *value = d->sstream;
  } else if (!strcmp(key, "tstream")) { /* 1: the stream's chunks run on the token-LM variant of fltx_slane.h */
    *value = d->tstream;
  } else if (!strcmp(key, "looks_dropped")) { /* defer_check = 2: batches that were overwritten without a look at their statuses */
    *value = d->looksDropped;
  } else if (!strcmp(key, "unread_redone")) { /* defer_check = 1: utterances decoded again while settling batches nobody read */
    *value = d->unreadRedone;
  } else if (!strcmp(key, "compactions")) { /* streams: times the LM-state free lists were rebuilt since fltx_stream_begin */
    *value = d->compactions;
  } else if (!strcmp(key, "staged_emissions")) { /* address of the library's own device copy of the last offline batch's emissions
                                                     (0 when the caller's device buffer was used): valid until the next call */
    *value = (d->haveResults && d->lastEmis && (d->lastEmis == d->emis[0].as<float>() || d->lastEmis == d->emis[1].as<float>()))
                 ? (int64_t)(uintptr_t)d->lastEmis : 0;
  } else if (!strcmp(key, "id_cap")) {     /* streams: LM-state ids per stream (constant however long the stream runs) */
    *value = d->recycle ? d->idCap : 0;
  } else if (!strcmp(key, "hlm_asked")) { /* host LM: questions the frames listed since decodeBegin ... */
    *value = d->hlmAsked;
  } else if (!strcmp(key, "hlm_distinct")) { /* ... and how many the callbacks were asked (distinct per frame) */
    *value = d->hlmDistinct;
  } else if (!strcmp(key, "stream_redone")) {
    *value = d->streamRedone;
  } else if (!strcmp(key, "wlane")) { /* 1: the last call ran on fltx_wlane.h (token sets beyond 64) */
    *value = d->wlaneFirst;
  } else if (!strcmp(key, "slane")) {
    *value = d->slaneFirst;
  } else if (!strcmp(key, "slane_m32")) { /* 1: the last call started on fltx_slane.h's kernel with 32-bit token masks */
    *value = d->slaneM32First;
  } else if (!strcmp(key, "tlane")) { /* 1: the last call started on fltx_slane.h's token-LM variant */
    *value = d->tlaneFirst;
  } else if (!strcmp(key, "toklm_contexts")) { /* rows of the LM's dense (context, token) table (0: none built) */
    *value = d->tokLmCtx;
  } else if (!strcmp(key, "fallback_reasons")) {
    *value = d->fallbackReasons;
  } else if (!strcmp(key, "bt_record_bytes")) { /* the last back-trace: 2 / 4 = packed records narrowed to that width with the
                                                    token tile resident in LDS (backtraceNarrow), 0 = backtraceUtterance */
    *value = d->btNarrow;
  } else if (!strcmp(key, "bt_chunk_frames")) { /* ... frames per chunk of history records in LDS (0: none, walked through HBM) */
    *value = d->btChunk;
  } else if (!strcmp(key, "bt_stretch_frames")) { /* ... frames per stretch of staged addends in LDS while the scores are re-added */
    *value = d->btStretch;
  } else if (!strcmp(key, "bt_walk_waves")) { /* ... waves that walked its chunks: 1 = one walk per hypothesis, more = every wave walked
                                                  a stretch of each chunk from every slot and the paths were composed */
    *value = d->btWalkWaves;
  } else if (!strcmp(key, "bt_threads")) {
    *value = d->btThreads;
  } else if (!strncmp(key, "bt_prof_", 8)) { /* "bt_profile": shader clocks of the last narrow back-trace, summed over the utterances */
    return btProfileGet(d, key + 8, value);
  } else if (!strcmp(key, "why_not_lane")) { /* FLTX_WHY_* (include/fltx.h): why the last call did not start on a lane engine */
    *value = d->whyFirst;
  } else if (!strcmp(key, "lane_groups")) { /* lane groups of the lane = LM state engine: 1 = fltx_slane.h, 2 / 4 / 8 = fltx_mlane.h;
                                                fltx_ylane.h: 1 / 2 / 4 */
    *value = d->laneGroupsFirst;
  } else if (!strcmp(key, "ymemo_slots")) {
    *value = (d->ylane || d->xlane) && d->yshare ? (int64_t)d->ymemoSlots : 0;
  } else if (!strcmp(key, "lane")) {
    *value = d->lane;
  } else if (!strcmp(key, "lean")) {
    *value = d->lean; /* groups per thread kept in registers: 6 / 12, or 255 = streaming */
  } else if (!strcmp(key, "threads")) {
    *value = d->threads;
  } else if (!strcmp(key, "lds")) {
    *value = d->wsInLds ? 1 : 0;
  } else if (!strcmp(key, "cut")) {
    *value = d->cutM;
  } else if (!strcmp(key, "hot_level")) {
    *value = d->wsInLds ? 0 : d->hotLevel;
  } else if (!strcmp(key, "recompute")) {
    *value = d->cutRecompute;
  } else if (!strcmp(key, "cap")) {
    *value = d->CAP;
  } else if (!strcmp(key, "cap2")) {
    *value = d->CAP2;
  } else if (!strcmp(key, "items")) {
    *value = d->itemCap;
  } else if (trTimedSlot(key) >= 0) {
    /* "time_transcripts": device time of the last fltx_result_transcripts' three kernels / of the last
     * fltx_pack_results_kernel (HIP events around each; 0 when not timed or not launched) */
    *value = (int64_t)((double)d->tr.ms[trTimedSlot(key)] * 1e6 + 0.5);
  } else if (!strcmp(key, "emissions_narrow_max")) { /* see fltx_decoder_set */
    *value = d->s2s.crNarrowMax;
  } else if (!strcmp(key, "ws_bytes")) { /* d->wsBytes: the workspace bytes of one utterance that prepare() sized */
    *value = (int64_t)d->wsBytes;
  } else {
    return fail(FLTX_ERR_INVALID, "fltx_decoder_get: unknown key '%s'", key);
  }
  return FLTX_OK;
}

int fltx_decoder_set(fltx_decoder* d, const char* key, int64_t value) {
  if (!d || !key) {
    return fail(FLTX_ERR_INVALID, "null argument");
  }
  if (!strcmp(key, "defer_check")) {
    d->deferCheck = value == 2 ? 2 : (value ? 1 : 0);
    return FLTX_OK;
  }
  if (!strcmp(key, "max_states")) { /* a CTC rows decoder: LM states per utterance from the next fltx_ctc_rows_begin on */
    if (!isCrKind(d->kind) || value < 1 || value > 0x7FFFFFFF) {
      return fail(FLTX_ERR_INVALID, "max_states: a CTC rows decoder (fltx_ctc_rows_decoder_create, "
                                    "fltx_ctc_rows_lex_decoder_create) and a count >= 1");
    }
    d->s2s.maxStates = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "emissions_narrow_max")) { /* a CTC rows decoder: the widest typed frame a wave takes (0: none) */
    if (!isCrKind(d->kind) || value < 0 || value > kCrTypedNarrowCap) {
      return fail(FLTX_ERR_INVALID, "emissions_narrow_max: a CTC rows decoder and a width in [0, %d]", kCrTypedNarrowCap);
    }
    d->s2s.crNarrowMax = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "time_transcripts")) { /* measurement: see fltx_decoder_get "transcript_count_ns" */
    d->tr.timed = value ? 1 : 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "compact_always")) {
    d->userCompactAlways = value ? 1 : 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "threads")) {
    if (value != 64 && value != 128 && value != 256 && value != 512 && value != 1024) {
      return fail(FLTX_ERR_INVALID, "threads must be 64, 128, 256, 512 or 1024");
    }
    d->userThreads = (int)value;
    d->threads = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "keep_scores")) { /* record {score, am, lm} per history slot (getBestHypothesis) */
    d->keepScores = d->userKeepScores = value != 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "profile_wave")) {
    d->profWave = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "profile")) {
    d->profile = value != 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "lean")) { /* 0: lexicon-free + ZeroLM frames use the generic engine */
    d->noLean = value == 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "items")) { /* 0: the lexicon decoder walks the full hypothesis x token grid */
    d->genericAsked = true; /* a knob of the generic lexicon engine: that engine is what the caller wants */
    d->noItems = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "slim")) { /* 0: the cut-off generation recomputes instead of keeping slim records */
    d->genericAsked = true; /* a knob of the generic lexicon engine: that engine is what the caller wants */
    d->noSlim = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "hot_level")) { /* testing: 1 keeps the candidate records of an HBM workspace in HBM */
    d->genericAsked = true; /* a knob of the generic lexicon engine: that engine is what the caller wants */
    d->maxHotLevel = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "lds_budget")) { /* testing: pretend the CU has this many bytes of LDS (<= 160 KiB) */
    d->genericAsked = true; /* a knob of the generic lexicon engine: that engine is what the caller wants */
    d->ldsBudget = value > 0 && (size_t)value < kMaxLds ? (size_t)value : 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "cut_m")) { /* testing: number of best candidates kept by the cut (default 3K + 64) */
    d->genericAsked = true; /* a knob of the generic lexicon engine: that engine is what the caller wants */
    d->userCutM = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "cut")) { /* 0: the lexicon decoder materialises every candidate (no score-pass cut) */
    d->genericAsked = true; /* a knob of the generic lexicon engine: that engine is what the caller wants */
    d->noCut = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "xlane")) { /* 0: do not use the lane = (LM state, trie node) kernel (fltx_xlane.h) */
    d->noXlane = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "stream_total_frames")) { /* before fltx_stream_begin: see prepare() */
    d->streamTotalFrames = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "sstream")) { /* 0: stream chunks stay on the lane-per-slot step (fltx_lane.h) */
    d->noSstream = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "stream_optimistic")) { /* 0: streams of the lexicon decoder start on the worst-case (HBM) workspace */
    d->userStreamOpt = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "lm_cache")) { /* 0: the generic step asks the n-gram tables every time (DecodeParams::lmCache) */
    d->noLmCache = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "stream_defer")) { /* 0: fltx_stream_step waits for its chunk and decodes it again there if it must */
    d->deferRedo = value ? 1 : 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "bt_threads")) { /* threads of a back-trace workgroup: 64 .. 512 in whole waves, 0 = the default */
    if (value != 0 && (value < 64 || value > 512 || value % 64 != 0)) {
      return fail(FLTX_ERR_INVALID, "bt_threads must be 0 or a multiple of 64 up to 512");
    }
    d->btThreads = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "bt_walk_waves")) { /* 0 / 1: the narrow back-trace keeps one walk per hypothesis (A/B runs, tests) */
    d->btWalkAsked = (value == 0 || value == 1) ? 1 : -1;
    return FLTX_OK;
  }
  if (!strcmp(key, "bt_profile")) { /* phase marks of the narrow back-trace: fltx_decoder_get "bt_prof_*" */
    d->btProfile = value != 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "bt_lds_kb")) { /* LDS the back-trace kernel stages history chunks in (0: 144 KB) */
    d->btLdsKb = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "yshare")) { /* fltx_ylane.h geometry that shares a CU: 1 always, 0 never, -1 when the batch exceeds the CUs */
    d->userYshare = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "ylane")) { /* 0: do not use fltx_ylane.h; 2: prefer it where fltx_xlane.h applies too */
    d->noYlane = value ? 0 : 1;
    d->preferYlane = value == 2;
    return FLTX_OK;
  }
  if (!strcmp(key, "slane_threads")) {
    d->slaneThreads = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "wlane")) { /* 0: large token sets stay off the lane = LM state engine (fltx_wlane.h) */
    d->noWlane = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "tok_dense")) { /* 0: a token-level n-gram LM is not flattened to a dense table (tests: the probe chain) */
    d->noTokDense = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "tlane")) { /* 0: a token-level n-gram LM on the lexicon-free decoder stays on the generic engine */
    d->noTlane = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "slane")) { /* 0: do not use the lane = LM state kernel (fltx_slane.h) */
    d->noSlane = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "ylane_asg")) { /* 0: the ASG criterion keeps the lexicon decoder on the generic engine */
    d->noYlaneAsg = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "slane_m32")) { /* 0: fltx_slane.h keeps 64-bit token masks whatever the token set (measurements) */
    d->noSlaneM32 = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "tune")) { /* development: see DecodeParams::tune */
    d->userTune = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "ylane_rank_at")) { /* tests: see DecodeParams::yRankAt */
    d->userYRankAt = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "ylane_groups")) { /* fltx_ylane.h: at least this many lane groups (tests) */
    d->userYlaneGroups = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "lane_groups")) { /* fltx_mlane.h: 0 = as many lane groups as the beam needs, 2 / 4 / 8 = at least that many, -1 = never */
    d->userLaneGroups = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "mlane_geo")) { /* tuning: row of kMlaneGeo to use (-1 = first that fits) */
    d->userMlaneGeo = (int)value;
    return FLTX_OK;
  }
  if (!strcmp(key, "lane")) { /* 0: beams <= 64 use the lean kernel instead of the lane-per-slot kernel */
    d->noLane = value ? 0 : 1;
    return FLTX_OK;
  }
  if (!strcmp(key, "dense")) { /* 0: force the generic hash merge for lexicon-free frames */
    d->noDense = value == 0;
    return FLTX_OK;
  }
  if (!strcmp(key, "force_global_ws")) {
    d->genericAsked = true; /* a knob of the generic lexicon engine: that engine is what the caller wants */
    d->forceGlobalWs = value != 0;
    return FLTX_OK;
  }
  return fail(FLTX_ERR_INVALID, "unknown tunable '%s'", key);
}

} /* extern "C" */

namespace {

/* geometry + buffers for B streams of up to maxFrames frames (plus seed and
 * decodeEnd slots) */
/* the compiled geometries of the lane engines (fltx_engines.h) */
struct LaneGeo {
  int threads, gt;
};
struct MlaneGeo {
  int threads, gt, ng, gpw, spw;
};
#define FLTX_GEO2(WW, GG) {WW, GG},
#define FLTX_GEO5(WW, GG, NG, GPW, SPW) {WW, GG, NG, GPW, SPW},
static const LaneGeo kSlaneGeo[] = {FLTX_SLANE_GEOS(FLTX_GEO2)};
static const LaneGeo kSstreamGeo[] = {FLTX_SSTREAM_GEOS(FLTX_GEO2)};
static const LaneGeo kWlaneGeo[] = {FLTX_WLANE_GEOS(FLTX_GEO2)};
static const LaneGeo kXlaneGeo[] = {FLTX_XLANE_GEOS(FLTX_GEO2)};
static const MlaneGeo kMlaneGeo[] = {FLTX_MLANE_GEOS(FLTX_GEO5)}; /* "mlane_geo" = row */
static const MlaneGeo kTmlaneGeo[] = {FLTX_TMLANE_GEOS(FLTX_GEO5)};
#undef FLTX_GEO2
#undef FLTX_GEO5
constexpr int kMlaneGeoCount = (int)(sizeof(kMlaneGeo) / sizeof(kMlaneGeo[0]));
constexpr int kSlaneGeoCount = (int)(sizeof(kSlaneGeo) / sizeof(kSlaneGeo[0]));
/* kSlaneGeo rows, fastest first (C2: 1.95, 2.11, 2.14 ms ...); more utterances than CUs: 512 threads (104 VGPRs: four
 * waves per SIMD) let two utterances share a CU -- C2 at 512 utterances: 162.7 M frames/s against 119.3 M with nine
 * waves each */
static const int kSlaneOrderOne[kSlaneGeoCount] = {4, 3, 2, 1, 0, 5, 6, 7};
static const int kSlaneOrderTwo[kSlaneGeoCount] = {3, 2, 1, 4, 0, 5, 6, 7};

int engineOf(const fltx_decoder* d) {
  return d->ylane ? 6 : d->xlane ? 5 : (d->slane ? 4 : (d->lane ? 3 : (d->lean ? 2 : (d->dense ? 1 : 0))));
}
/* fltx_slane.h's offline max-merge kernel keeps its token masks in 32 bits when the token set has at most 32 tokens
 * (the M32 instantiations: every geometry of FLTX_SLANE_GEOS has one) */
bool slaneM32(const fltx_decoder* d) {
  return d->slane && !d->tlane && !d->wlane && d->mlaneNG <= 1 && !d->xlane && !d->ylane && !d->opt.log_add && d->N <= 32 &&
         !d->noSlaneM32;
}
/* what fltx_decoder_get reports about the engine a call started on */
void latchFirst(fltx_decoder* d) {
  d->engineFirst = engineOf(d);
  d->whyFirst = d->whyNotLane;
  d->wlaneFirst = d->wlane;
  d->slaneFirst = d->slane;
  d->slaneM32First = slaneM32(d) ? 1 : 0;
  d->tlaneFirst = d->tlane;
  d->xlaneFirst = d->xlane;
  d->ylaneFirst = d->ylane;
  d->laneGroupsFirst = d->slane ? std::max(1, d->mlaneNG) : d->ylane;
}

/* the per-utterance results a look reads (beam count, final frame, status): three rows of one allocation */
int ensureUttRes(fltx_decoder* d, int B, Stream st) {
  if ((size_t)B > d->uttRow || !d->uttRes.p) {
    const size_t row = ((size_t)B + (size_t)B / 8 + 3) & ~(size_t)3;
    bool grew = false;
    if (d->uttRes.ensure(12 * row, st, true, &grew) || (!grew && devMemset(d->uttRes.p, 0, 12 * row, st))) {
      return 1; /* (rows that move start zeroed, as a fresh allocation does) */
    }
    d->uttRow = row;
    d->uttNBeam.p = d->uttRes.p;
    d->uttFrame.p = d->uttRes.as<int32_t>() + row;
    d->uttStatus.p = d->uttRes.as<int32_t>() + 2 * row;
  }
  return 0;
}

/* histOff is a function of (T[], K) alone: it travels only when it differs from what histOffD already holds, and then
 * through pinned staging (no pageable copy on the launch stream) */
int uploadHistOff(fltx_decoder* d, Stream st) {
  if (d->histOffSentTo == d->histOffD.p && d->histOffSent == d->histOff) {
    return 0;
  }
  const size_t n = sizeof(int64_t) * d->histOff.size();
  void* h = d->histOffStage.acquire(n);
  if (!h) {
    return 1;
  }
  memcpy(h, d->histOff.data(), n);
  d->histOffSentTo = nullptr;
  if (devCopyH2D(d->histOffD.p, h, n, st) || d->histOffStage.sent(st)) {
    return 1;
  }
  d->histOffSent = d->histOff;
  d->histOffSentTo = d->histOffD.p;
  return 0;
}

int prepare(fltx_decoder* d, int B, int N, const int32_t* Tmax, bool forceWorstCaseCap) {
  /* host LM: the generic engine, a frame per launch, every candidate's record built in one pass (the cut-off
   * generation rebuilds LM-state keys from (state, label) pairs, which a host LM's states are not) */
  const bool hostLm = d->lm->kind == 2;
  forceWorstCaseCap = forceWorstCaseCap || hostLm;
  const size_t kMaxLdsHw = kMaxLds;
  const size_t kMaxLds = d->ldsBudget ? d->ldsBudget : kMaxLdsHw;
  Stream st = d->ctx->stream;
  const int K = d->opt.beam_size;
  if (d->kind == FLTX_DECODER_LEXICON && d->trie->nTokens != N) {
    return fail(FLTX_ERR_INVALID, "N = %d but the trie was built for %d tokens", N, d->trie->nTokens);
  }
  if (d->nTrans && d->nTrans != N * N) {
    return fail(FLTX_ERR_INVALID, "transitions has %d entries, expected N*N = %d", d->nTrans, N * N);
  }
  if (d->opt.criterion == FLTX_CRITERION_ASG && !d->nTrans) {
    return fail(FLTX_ERR_INVALID, "ASG criterion needs N*N transitions");
  }
  if (d->sil < 0 || d->sil >= N) {
    return fail(FLTX_ERR_RANGE, "sil index %d outside [0, %d)", d->sil, N);
  }
  if (d->opt.criterion == FLTX_CRITERION_CTC && (d->blank < 0 || d->blank >= N)) {
    return fail(FLTX_ERR_RANGE, "blank index %d outside [0, %d)", d->blank, N);
  }
  d->B = B;
  d->N = N;
  d->histOff.resize(B + 1);
  int64_t off = 0;
  int maxT = 0;
  for (int b = 0; b < B; ++b) {
    if (Tmax[b] < 0) {
      return fail(FLTX_ERR_INVALID, "T[%d] = %d is negative", b, Tmax[b]);
    }
    d->histOff[b] = off;
    off += (int64_t)(Tmax[b] + 2) * K;
    maxT = std::max(maxT, Tmax[b]);
  }
  d->histOff[B] = off;
  d->histRecords = off;
  /* LM states are created for as long as a stream runs, not for as long as its frames stay buffered: the id
   * tables of a stream are sized for `stream_total_frames` (default: at least 2 048 frames; a longer stream says
   * so before fltx_stream_begin, or its status reports a full table), the history for max_frames */
  /* A stream's ids are recycled (fltx_compact_states_kernel): its tables are sized for what the buffer can hold --
   * beam x max_frames states made between two rebuilds of the free list, plus the states a rebuild keeps -- however
   * long the stream runs ("stream_total_frames" is accepted and ignored).  A host LM numbers its own states. */
  d->recycle = !d->offlineCall && !hostLm;
  const int idT = maxT;
  const int64_t streamIds = (int64_t)K * (idT + 2) + 8 * (int64_t)K + 64;
  uint64_t wantStates = d->recycle ? 2ull * (uint64_t)streamIds : 2ull * ((uint64_t)K * (uint64_t)(idT + 2) + 2);
  uint32_t cap = nextPow2(std::max<uint64_t>(wantStates, 1024));
  if (d->recycle && cap > (1u << 24)) { /* (a stream's ids are bounded below: 2^23 of them fill half of this) */
    cap = 1u << 24;
  }
  if (cap > (1u << 23) && !d->recycle) {
    return fail(FLTX_ERR_UNSUPPORTED, "K * T = %llu exceeds the 2^23 LM states per utterance this build indexes",
                (unsigned long long)K * (maxT + 2));
  }
  /* candidate capacity */
  const int nTok = std::min(d->opt.beam_size_token, N);
  /* tokens a lane engine lists per frame (CTC with the whole token set: the blank is not listed) */
  const int nList = nTok - ((d->opt.criterion == FLTX_CRITERION_CTC && d->opt.beam_size_token >= N) ? 1 : 0);
  /* (sil and blank are in range: checked above) */
  const bool optionsOk = d->opt.beam_threshold >= 0.0;
  /* lexicon-free frames merge through the dense (hash-free) path: one slot per
   * (LM state, token) group plus one per orphan repeat; the hash is then only
   * used by decodeEnd (<= K candidates) */
  /* (not for a host LM: the dense merge assumes at most two hypotheses per LM state -- true of states that are a trie
   * over their inputs, not of whatever a user's LM::score returns) */
  d->dense = (d->kind == FLTX_DECODER_LEXFREE && !d->noDense && !hostLm) ? 1 : 0;
  /* threads per utterance: the frame step is latency bound, so more waves per
   * utterance win as long as the batch does not fill the CUs on its own
   * (measured on C2: 256 -> 15.3 ms, 512 -> 13.0 ms per 256-utterance batch) */
  if (!d->userThreads) {
    /* one workgroup per CU: give it two waves per SIMD; more utterances than
     * CUs: 256 threads, so that several utterances share a CU (C2 at B=512:
     * 512 threads cannot co-reside (VGPRs), 256 can) */
    d->threads = (d->kind == FLTX_DECODER_LEXICON || B <= d->ctx->numCUs) ? 512 : 256;
    /* (the lexicon decoder's workspace fills a CU's LDS, so one utterance per CU either way:
     * 1024 utterances, 256 -> 512 threads: C3 19.7 -> 27.9 M frames/s, C4 9.8 -> 12.7 M) */
  }
  /* lean frame step (fltx_lean.h): lexicon-free + ZeroLM, groups held in registers */
  d->lean = 0;
  bool leanInHbm = false;
  if (d->dense && !d->noLean && !d->forceGlobalWs && d->lm->kind == 0 && K < 32000 && N <= 64) {
    const int64_t groups = (int64_t)K * (nTok + 1);
    const int64_t per = (groups + d->threads - 1) / d->threads;
    d->lean = per <= 6 ? 6 : (per <= 12 ? 12 : 255); /* 255: streaming lean step (groups evaluated twice) */
  }
  /* lane-per-slot frame step (fltx_lane.h): beam and token set fit one wave's lanes */
  d->lane = 0;
  if (d->lean && !d->noLane && K <= 64 && N <= 64) {
    const int nW = d->threads / 64;
    const int per = (nTok + nW - 1) / nW;
    d->lane = per <= 4 ? 4 : (per <= 8 ? 8 : 0);
  }
  /* lane = LM state decode (fltx_slane.h): offline lexicon-free + ZeroLM max-merge, beam and
   * tokens within one wave's lanes; the history rows are its LM-state memo (23-bit ids) */
  d->slane = 0;
  const int* slaneOrder = B > d->ctx->numCUs ? kSlaneOrderTwo : kSlaneOrderOne;
  if (d->lane && !d->noSlane && d->offlineCall && !d->keepScores && !forceWorstCaseCap &&
      optionsOk && (int64_t)K * (maxT + 2) < (1 << 23) - 1) {
    for (int oi = 0; oi < kSlaneGeoCount; ++oi) {
      const int gi = slaneOrder[oi];
      const LaneGeo& g = kSlaneGeo[gi];
      if ((d->userThreads && d->threads != g.threads) || (d->slaneThreads && d->slaneThreads != g.threads)) {
        continue;
      }
      if (nList <= g.gt * (g.threads / 64 - 2)) {
        d->slane = g.gt;
        d->threads = g.threads;
        break;
      }
    }
  }
  /* ... with a token-level n-gram LM (slaneUtterance<.., TL = true>; LexiconFreeDecoder.cpp:69-85 + KenLM.cpp:63-83):
   * LM states are still the trie of token histories, so the lanes keep their shape; the LM is one gather from a dense
   * (context, token) table built on the host (lmTokDense) -- when the model's contexts fit one */
  d->tlane = 0;
  d->tokLm = nullptr;
  d->tokLmTooBig = false;
  const int2* tab = nullptr;
  int64_t nCtx = 0;
  const bool tokenLm = d->kind == FLTX_DECODER_LEXFREE || (d->kind == FLTX_DECODER_LEXICON && d->isLmToken);
  if (tokenLm && d->lm->kind == 1 && N <= 64 && !d->noTokDense) { /* (every index the LM is asked about is a token) */
    /* the dense table serves every engine this decoder can run on: the lane engine below gathers from it, and the
     * generic engine (beams beyond 64, streams, fallbacks) keeps a state's context as a row number and replaces its
     * chain of n-gram probes by the same gather (lmScoreDev) */
    int rcd = lmTokDense(const_cast<fltx_lm*>(d->lm), d->ctx, d->lmDev, N, &tab, &nCtx);
    if (rcd) {
      return rcd;
    }
    d->tokLmTooBig = tab == nullptr;
    d->tokLm = tab;
    d->tokLmCtx = tab ? nCtx : 0;
  }
  if (tab && d->kind == FLTX_DECODER_LEXFREE && !d->noSlane && !d->noTlane && !d->genericAsked &&
      !d->noDense && d->offlineCall && !d->keepScores && !forceWorstCaseCap && !d->forceGlobalWs && K <= 64 &&
      optionsOk && (int64_t)K * (maxT + 2) < (1 << 23) - 1) {
    for (int oi = 0; oi < kSlaneGeoCount; ++oi) {
      const LaneGeo& g = kSlaneGeo[slaneOrder[oi]];
      if ((d->userThreads && d->threads != g.threads) || (d->slaneThreads && d->slaneThreads != g.threads)) {
        continue;
      }
      if (nList <= g.gt * (g.threads / 64 - 2)) {
        d->slane = g.gt;
        d->tlane = 1;
        /* the re-entry memos in LDS: 4 096 edges + 2 048 child masks (75 KB: two workgroups fit a CU) when the batch
         * has more utterances than CUs, twice as many of both (131 KB) when a workgroup has the CU to itself */
        const bool shareCu = B > d->ctx->numCUs || (d->deferCheck && g.threads == 512); /* (defer_check: the caller keeps two batches in flight) */
        d->tlEdgeSlots = shareCu ? 4096 : 8192;
        d->tlMaskSlots = shareCu ? 2048 : 4096;
        d->threads = g.threads;
        break;
      }
    }
  }
  /* ... for token sets beyond 64 (word pieces) when the token beam keeps at most 64 of them (fltx_wlane.h): masks and
   * lists by position in the frame's token beam, a front-end wave that cuts the row to it */
  d->wlane = 0;
  if (d->kind == FLTX_DECODER_LEXFREE && !d->noSlane && !d->noWlane && !d->genericAsked && d->offlineCall && !d->keepScores &&
      !forceWorstCaseCap && !d->forceGlobalWs && !d->opt.log_add && d->lm->kind == 0 && !d->isLmToken && N > 64 &&
      N <= kWlMaxN && K <= 64 && nTok <= 64 && optionsOk && (int64_t)K * (maxT + 2) < (1 << 23) - 1) {
    for (const LaneGeo& g : kWlaneGeo) {
      if (d->userThreads && d->threads != g.threads) {
        continue;
      }
      if (nTok <= g.gt * (g.threads / 64 - 2)) {
        d->slane = g.gt;
        d->wlane = 1;
        d->wlMaxT = maxT;
        d->threads = g.threads;
        break;
      }
    }
  }
  /* ... with several groups of 64 lanes for beams beyond one wave's lanes (fltx_mlane.h): same candidates, merges and
   * selection; a wave holds the states of whole lane groups, history records carry 10-bit slots */
  d->mlaneNG = 0;
  if ((!d->slane || d->userLaneGroups > 1) && d->lean && !d->noSlane && d->userLaneGroups >= 0 && d->offlineCall && !d->keepScores &&
      !forceWorstCaseCap && K <= 64 * kMlMaxGroups && (K > 64 || d->userLaneGroups > 1) && N <= 64 &&
      optionsOk && (int64_t)K * (maxT + 2) < (1ll << 31) - 1) {
    const int needNG = std::max((K + 63) / 64, d->userLaneGroups);
    /* fastest first per group count (C2 shape, profiles/r04: beam 100 3.17 ms on row 1 against 3.23 on row 0, beam 200
     * 5.79 on row 4 against 6.21 on row 3; the wide rows 2 / 5 spill registers and are for token lists beyond 30) */
    static const int order[kMlaneGeoCount] = {1, 0, 2, 4, 3, 5, 6};
    for (int oi = 0; oi < kMlaneGeoCount; ++oi) {
      const int gi = order[oi];
      const MlaneGeo& g = kMlaneGeo[gi];
      if (d->userMlaneGeo >= 0 ? gi != d->userMlaneGeo : (d->userThreads && d->threads != g.threads)) {
        continue;
      }
      const int nBlk = (g.threads / 64 - g.ng / g.spw - 1) / (g.ng / g.gpw);
      if (g.ng >= needNG && nList <= g.gt * nBlk) {
        d->slane = g.gt;
        d->mlaneNG = g.ng;
        d->mlaneGPW = g.gpw;
        d->mlaneSPW = g.spw;
        d->threads = g.threads;
        break;
      }
    }
  }
  /* ... and both: a token-level n-gram LM at beams beyond 64 (mlaneUtterance<.., TL = true>): the dense table's gather per
   * candidate, state ids from a table in HBM (ymemo: a slot per state an utterance can create); token lists
   * of up to 64 at beams up to 256, of up to 30 beyond (the five geometries compiled for it) */
  if (tab && !d->slane && d->kind == FLTX_DECODER_LEXFREE && !d->noSlane && !d->noTlane && !d->genericAsked && !d->noDense &&
      d->userLaneGroups >= 0 && d->offlineCall && !d->keepScores && !forceWorstCaseCap && !d->forceGlobalWs &&
      K > 64 && K <= 64 * kMlMaxGroups && optionsOk && (int64_t)K * (maxT + 2) < (1ll << 27)) {
    const int needNG = std::max((K + 63) / 64, d->userLaneGroups);
    for (const MlaneGeo& g : kTmlaneGeo) {
      const int nBlk = (g.threads / 64 - g.ng / g.spw - 1) / (g.ng / g.gpw);
      if (g.ng >= needNG && nList <= g.gt * nBlk && (!d->userThreads || d->threads == g.threads)) {
        uint32_t slots = 1024;
        while ((int64_t)slots < (int64_t)K * (maxT + 2) && slots < (1u << 27)) {
          slots <<= 1;
        }
        if ((int64_t)slots * 8 * (int64_t)B > (16ll << 30)) {
          break; /* (very long utterances at a large beam: 16 GB of id tables is where this engine stops) */
        }
        d->slane = g.gt;
        d->tlane = 1;
        d->mlaneNG = g.ng;
        d->mlaneGPW = g.gpw;
        d->mlaneSPW = g.spw;
        d->threads = g.threads;
        d->ymemoSlots = slots; /* every state an utterance can create has a slot: the table cannot fill */
        break;
      }
    }
  }
  /* ... and the frames of a stream's decodeStep chunks on the same engine (the parked beam, the (parent, token) ->
   * id tables and the history rows keep the lane-per-slot engine's format) */
  d->sstream = 0;
  const auto chooseSstream = [&]() {
    for (const LaneGeo& g : kSstreamGeo) {
      if (nList <= g.gt * (g.threads / 64 - 2)) {
        d->sstream = g.gt;
        d->sstreamThreads = g.threads;
        return true;
      }
    }
    return false;
  };
  if (d->lane && !d->noSlane && !d->noSstream && !d->offlineCall && d->keepScores && !d->opt.log_add && optionsOk) {
    chooseSstream();
  }
  /* lane = (LM state, trie node) decode (fltx_xlane.h): offline LexiconDecoder + ZeroLM over a lexicon
   * without LM scores, CTC, max-merge or logAdd (round 5), one word per spelling, every word ending in sil, no <unk> */
  d->xlane = 0;
  d->yshare = 0;
  if (d->kind == FLTX_DECODER_LEXICON && !d->noXlane && !d->genericAsked && d->offlineCall && !d->keepScores &&
      !forceWorstCaseCap && !d->forceGlobalWs && d->lm->kind == 0 && !d->isLmToken && d->trie && d->trie->xOk &&
      !d->trie->xMulti && d->trie->xZeroSmear && d->trie->xEndTok == d->sil && d->sil != d->blank &&
      d->opt.criterion == FLTX_CRITERION_CTC && !(d->opt.unk_score > -std::numeric_limits<double>::infinity()) &&
      K <= 64 && N <= 64 && optionsOk && (int64_t)K * (maxT + 2) < (1 << 23) - 1) {
    for (const LaneGeo& g : kXlaneGeo) {
      if ((d->userThreads && d->threads != g.threads) || (d->slaneThreads && d->slaneThreads != g.threads)) {
        continue;
      }
      if (nTok <= g.gt * (g.threads / 64 - 3)) {
        d->xlane = g.gt;
        d->threads = g.threads;
        /* more utterances than CUs: the LM-state memo moves to HBM, 28 KB of LDS and 81 VGPRs let several
         * workgroups share a CU (see the lane engine with LM terms below) */
        d->yshare = (d->userYshare >= 0 ? d->userYshare != 0 : B > d->ctx->numCUs) ? 1 : 0;
        d->ymemoSlots = kXlMemoH;
        break;
      }
    }
  }
  /* ... with the LM terms and two lane groups (fltx_ylane.h): n-gram word LM and / or smeared trie,
   * beams up to 128 */
  d->ylane = 0;
  if (d->kind == FLTX_DECODER_LEXICON && !d->noYlane && !d->genericAsked && (!d->xlane || d->preferYlane) &&
      d->offlineCall && !d->keepScores && !forceWorstCaseCap && !d->forceGlobalWs &&
      (d->lm->kind == 0 || d->lm->kind == 1) && !d->isLmToken && d->trie && d->trie->xOk &&
      /* (several words per spelling: with an n-gram LM only -- under ZeroLM the words of a spelling tie in one LM state; one
       * and two lane groups only -- with four, the word wave's twelve candidate slots need twice the 128 registers a
       * 1 024-thread workgroup leaves a wave, and the spills made it 2.3 x slower than the generic engine on the
       * reference's test lexicon at beam 256) */
      (!d->trie->xMulti || (d->lm->kind == 1 && K <= 128 && d->userYlaneGroups <= 2)) && d->trie->xEndTok == d->sil &&
      (d->opt.criterion == FLTX_CRITERION_CTC ? d->sil != d->blank : (d->nTrans == N * N && !d->noYlaneAsg)) &&
      !(d->opt.unk_score > -std::numeric_limits<double>::infinity()) && K <= 256 && N <= 64 && optionsOk) {
    const int ng = std::max(K <= 64 ? 1 : (K <= 128 ? 2 : 4), d->userYlaneGroups);
    /* More utterances than CUs: the geometry of which two workgroups fit a CU (512 threads, <= 128
     * VGPRs, 77 KB of LDS: the LM-state memo moves to HBM) -- one utterance's waits are the other's
     * time to run (C5's 1 024 utterances per GPU: 1.6x).  With no more utterances than CUs the second
     * workgroup would not exist and the memo in LDS is the faster one. */
    /* Four lane groups (beams 129 .. 256): sixteen waves, the memo in HBM whatever the batch (the lanes, the merge
     * and orphan tables and ten token waves' pair lists fill the LDS); a long utterance creates more LM states than
     * the memo in LDS numbers (about 2.2 per frame on the C4 shape, 6 144 at most): it takes the HBM memo as well,
     * sized for its frames, instead of leaving the engine half way */
    const bool longUtt = (int64_t)maxT * 5 / 2 + 64 > kYlMemo * 3 / 4;
    /* (several words per spelling: the larger merge table takes the memo's place in LDS -- memo in HBM always) */
    const bool share = (ng == 4 || d->trie->xMulti) ? true : (d->userYshare >= 0 ? d->userYshare != 0 : (B > d->ctx->numCUs || longUtt));
    const bool multi = d->trie->xMulti; /* (one workgroup per CU: two lane groups keep their eight token waves) */
    const int threads = ng == 4 ? 1024 : (ng == 1 ? 512 : ((share && !multi) ? 512 : 768));
    const int nTokWaves = threads / 64 - ng - 2;
    const int tpw = (nTok + nTokWaves - 1) / nTokWaves;
    const int pairCap = ng == 4 ? kYlPairs4 : ((ng == 2 && share && !multi) ? 1024 : 512);
    const int maxTokWaves = ng == 4 ? 10 : 8;
    if ((!d->userThreads || d->threads == threads) && tpw * nTokWaves <= 96 && tpw * 64 * ng <= pairCap &&
        nTokWaves <= maxTokWaves) {
      /* slots of the memo in HBM: four per LM state the utterance can create, a power of two, 16-bit state numbers */
      uint32_t ms = kYlMemo;
      /* (C4 shape: 2.2 new LM states per frame at beam 100, 4 .. 6.5 at beam 256; a memo no bigger than it has to be
       * stays in the L2: 8 192 slots unless the utterance is long or the beam needs four groups) */
      /* (several words per spelling: every further word that stays in the beam is one more LM state -- four times as many) */
      const int perFrame = (ng == 4 ? 8 : 5) * (d->trie->xMulti ? 4 : 1);
      while ((longUtt || ng == 4 || d->trie->xMulti) && ms < 65536u && (int64_t)ms * 3 / 4 < (int64_t)maxT * perFrame + 256) {
        ms *= 2;
      }
      d->ymemoSlots = share ? ms : kYlMemo;
      d->yshare = share ? 1 : 0;
      d->ylane = ng;
      d->ylaneRounds = ng == 1 ? 2 : 4;
      d->ylaneTpw = tpw;
      d->ylaneLm = ((d->lm->kind != 0 || !d->trie->xZeroSmear) ? 1 : 0) | (d->opt.criterion == FLTX_CRITERION_CTC ? 0 : 2) |
                   (d->trie->xMulti ? 4 : 0) | (d->opt.log_add ? 8 : 0);
      d->threads = threads;
      d->xlane = 0;
    }
  }
  /* ... and the chunks of a stream with a token-level n-gram LM (slaneUtterance<.., ST, TL>): begin / end / prune /
   * getBestHypothesis stay the generic engine's kernels -- they know n-gram LMs and keep a state's context row in stateCtx --
   * and the chunk's frames take their state ids from that engine's (parent id, edge) -> id table */
  d->tstream = 0;
  if (d->tokLm && d->kind == FLTX_DECODER_LEXFREE && !d->noSlane && !d->noTlane && !d->noSstream && !d->genericAsked &&
      !d->offlineCall && d->keepScores && !d->opt.log_add && K <= 64 && d->recycle && optionsOk && chooseSstream()) {
    d->tstream = 1;
  }
  { /* which eligibility terms kept this call off the lane engines (fltx_decoder_get "why_not_lane") */
    int64_t why = 0;
    if (!(d->slane || d->xlane || d->ylane || d->sstream)) {
      const bool lexi = d->kind == FLTX_DECODER_LEXICON;
      const bool unkOn = d->opt.unk_score > -std::numeric_limits<double>::infinity();
      why |= (N > 64 && (lexi || N > kWlMaxN || nTok > 64)) ? FLTX_WHY_TOKENS : 0; /* (lexicon-free: the token BEAM has to fit, fltx_wlane.h) */
      why |= (lexi ? K > ((d->trie && d->trie->xMulti) ? 128 : 256) : K > 64 * kMlMaxGroups) ? FLTX_WHY_BEAM : 0;
      why |= (!d->offlineCall && (lexi || d->opt.log_add || d->lm->kind == 1)) ? FLTX_WHY_STREAM : 0;
      /* (lexicon-free + n-gram LM: the TL variants of fltx_slane.h / fltx_mlane.h take it at beams up to 512 when the
       * model's contexts fit a dense table -- what is left of the term there: a host LM, a model too large for the
       * table; a token list no compiled geometry covers shows as GEOMETRY below) */
      why |= (d->lm->kind == 2 || (lexi && d->isLmToken) || (!lexi && d->lm->kind == 1 && d->tokLm == nullptr)) ? FLTX_WHY_LM : 0;
      /* (logAdd on the lexicon lane engines: CTC, one word per spelling) */
      /* (logAdd on the lexicon decoder is no reason any more: every configuration the lexicon lane engines take without
       * it, they take with it) */
      why |= (lexi && d->opt.criterion != FLTX_CRITERION_CTC && d->noYlaneAsg) ? FLTX_WHY_ASG : 0;
      why |= (lexi && unkOn) ? FLTX_WHY_UNK : 0;
      why |= (lexi && d->trie && (!d->trie->xOk || (d->trie->xMulti && d->lm->kind == 0))) ? FLTX_WHY_TRIE_SHAPE : 0;
      why |= (lexi && d->trie && d->trie->xOk && (d->trie->xEndTok != d->sil || d->sil == d->blank)) ? FLTX_WHY_WORD_END : 0;
      why |= !optionsOk ? FLTX_WHY_OPTIONS : 0;
      why |= ((int64_t)K * (maxT + 2) >= (lexi || K <= 64 ? (1ll << 23) - 1 : (1ll << 31) - 1)) ? FLTX_WHY_LENGTH : 0;
      why |= (d->noSlane || d->noXlane || d->noYlane || d->genericAsked || d->forceGlobalWs || d->noLean || d->noDense ||
              d->userLaneGroups < 0 || forceWorstCaseCap || (d->offlineCall && d->keepScores) ||
              (!lexi && N > 64 && d->noWlane) || (!lexi && d->lm->kind == 1 && d->noTlane)) ? FLTX_WHY_SWITCHED_OFF : 0;
      why |= (!lexi && N > 64 && d->opt.log_add) ? FLTX_WHY_LOGADD : 0; /* (fltx_wlane.h has no logAdd variant) */
      why |= (!lexi && nList > 70) ? FLTX_WHY_GEOMETRY : 0;
      if (!why) {
        why = FLTX_WHY_GEOMETRY; /* (no compiled geometry covers this token list / thread count) */
      }
    }
    d->whyNotLane = why;
  }
  if (d->lean && !d->lane && !d->slane) { /* the lean steps keep their (record-free) workspace in LDS or are not used */
    Ws t2;
    const size_t need = carveWs(t2, nullptr, K, 1, 64, 1024, N, K + 256, 2, 0, 0, 0, d->threads / 64);
    if (need > kMaxLds) {
      d->lean = 255; /* too big for LDS: the streaming step over an HBM workspace (leanBarrier) */
      leanInHbm = true;
      if (!d->userThreads) {
        d->threads = 1024; /* (C2 shape, beam 1000: 314 -> 234 ms, beam 2500: 1375 -> 1046) */
      }
    }
  }
  if (d->lean) {
    d->dense = 2; /* lean-only workspace layout (carveWs) */
  }
  int64_t worst = d->kind == FLTX_DECODER_LEXFREE ? (int64_t)K * (nTok + (d->dense ? 1 : 0))
                                                  : (int64_t)K * ((int64_t)nTok * 8 + 2);
  worst = std::max<int64_t>(worst, K);
  if (d->lean) {
    worst = 1; /* no candidate records at all */
  }
  int64_t capC = worst;
  d->NB = 1024;
  d->SCAP = K + 256;
  Ws tmp;
  auto hsFor = [&](int64_t c) {
    if (d->lean) {
      return 64; /* the merge hash is not used */
    }
    int64_t keys = d->dense ? K : c;
    return std::max((int)nextPow2((uint64_t)keys * 2), 64);
  };
  /* lexicon decoder: generate from a list of the (hypothesis, token) pairs that
   * have a child in the trie when the full grid would take several rounds */
  d->itemCap = 0;
  d->itemWide = 0;
  if (d->kind == FLTX_DECODER_LEXICON && !d->noItems && !d->forceGlobalWs && N <= 64 && d->trie &&
      d->trie->mask.p && (int64_t)K * nTok > d->threads && (int64_t)K * nTok < (1 << 29)) {
    /* (an item is hypothesis << 6 | token: 16 bits up to beam 1 024, a 32-bit word -- two of the list's uint16 words --
     * beyond: the reference's own test decodes at beam 2 500, where the full grid is 76 rounds of mostly empty cells) */
    d->itemWide = K > 1024 ? 1 : 0;
    d->itemCap = K * nTok * (d->itemWide ? 2 : 1);
  }
  const int itemCap0 = d->itemCap;
  auto bytesFor = [&](int64_t c) {
    return carveWs(tmp, nullptr, K, (int)c, hsFor(c), d->NB, N, d->SCAP, d->dense, d->lane, 0, d->itemCap,
                   d->threads / 64);
  };
  bool lds = !d->forceGlobalWs && !leanInHbm;
  d->CAP2 = 0;
  d->cutM = 0;
  d->cutRecompute = 0;
  const bool forceCut = d->userCutM > 0 && d->kind == FLTX_DECODER_LEXICON && !forceWorstCaseCap; /* tests */
  if (lds && (bytesFor(capC) > kMaxLds || forceCut)) {
    if (d->kind == FLTX_DECODER_LEXICON && !forceWorstCaseCap) {
      /* trie fan-out is sparse: size for the LDS and retry in HBM on overflow */
      int64_t c = capC;
      while (c > K && bytesFor(c) > kMaxLds) {
        c = c * 3 / 4;
      }
      const bool fits = c >= std::max<int64_t>(K * 4, 64) && bytesFor(c) <= kMaxLds;
      /* About K * (nTok + 2) candidates pass the pre-filter in a frame (measured:
       * C3 mean 280 / max 580 of 600, beam 100 x 29 tokens mean 1300 / max 2900
       * of 3100).  With room for 1.5x that, build every candidate's record in
       * one pass.  Otherwise (max-merge only) score every candidate into a slim
       * {score, order} list first and build records only for the best
       * cutM = 3K + 64 of them (runFrame): the record area then holds a few
       * hundred entries and the slim list takes what is left of the LDS. */
      const int64_t expect = (int64_t)K * (nTok + 2) * 3 / 2;
      bool cut = false;
      if ((!fits || c < expect || forceCut) && !d->noCut && !d->opt.log_add) {
        /* a merge group has up to three members: 3K + 64 of the best candidates hold K groups */
        const int64_t M = d->userCutM > 0 ? std::max<int64_t>(d->userCutM, K) : 3 * (int64_t)K + 64;
        const int64_t capRec = std::max<int64_t>(2 * M, 512);
        auto bytesCut = [&](int64_t c2) {
          return carveWs(tmp, nullptr, K, (int)capRec, hsFor(capRec), d->NB, N, d->SCAP, d->dense, d->lane, (int)c2,
                         d->itemCap, d->threads / 64);
        };
        int64_t c2 = std::min<int64_t>(worst, 16384);
        while (c2 > 4 * M && bytesCut(c2) > kMaxLds) {
          c2 = c2 * 7 / 8;
        }
        /* the slim list should hold what a frame produces (about K * (nTok + 2));
         * otherwise generate twice instead of remembering (runFrame) */
        if (!d->noSlim && bytesCut(c2) <= kMaxLds && c2 >= std::min<int64_t>(std::max<int64_t>(4 * M, expect * 2 / 3), worst)) {
          d->CAP2 = (int)c2;
          d->cutM = (int)M;
          capC = capRec;
          cut = true;
        } else {
          int64_t Mr = M;
          int64_t capRec2 = std::max<int64_t>(Mr * 5 / 4 + 64, 256);
          auto bytesRe = [&]() {
            return carveWs(tmp, nullptr, K, (int)capRec2, hsFor(capRec2), d->NB, N, d->SCAP, d->dense, d->lane, 0,
                           d->itemCap, d->threads / 64);
          };
          if (bytesRe() > kMaxLds && d->itemCap && d->userCutM <= 0) {
            /* The item list is worth more than the third member of every group
             * (groups average ~1.3 members): keep 2K + 64 if that makes it fit.
             * A frame whose merge then yields fewer than K groups although a
             * candidate above the threshold was left out is flagged as always
             * (beam 300 x 29 tokens: 15.6 -> 9.5 ms, none flagged). */
            const int64_t M2 = 2 * (int64_t)K + 64, cap2 = std::max<int64_t>(M2 * 5 / 4 + 64, 256);
            if (carveWs(tmp, nullptr, K, (int)cap2, hsFor(cap2), d->NB, N, d->SCAP, d->dense, d->lane, 0, d->itemCap,
                        d->threads / 64) <= kMaxLds) {
              Mr = M2;
              capRec2 = cap2;
            }
          }
          if (bytesRe() > kMaxLds && d->itemCap) {
            d->itemCap = 0; /* the grid form of the generation needs no list */
          }
          if (bytesRe() <= kMaxLds) {
            d->cutRecompute = 1;
            d->cutM = (int)Mr;
            capC = capRec2;
            cut = true;
          }
        }
      }
      if (!cut) {
        if (fits) {
          capC = c;
        } else {
          lds = false;
        }
      }
    } else {
      lds = false;
    }
  }
  if (!lds) {
    d->lane = 0;
    d->itemCap = 0;
    if (!d->userThreads && d->kind == FLTX_DECODER_LEXICON && !leanInHbm) {
      /* a beam that does not fit the LDS has work for sixteen waves, and the barriers of this path no longer cost
       * per wave (wsNoInv): C4 shape, beam 500 108 -> 86 ms, beam 1000 265 -> 195, beam 2500 961 -> 657 */
      d->threads = 1024;
    }
    /* Lexicon beams too big for the LDS: the recompute form of the cut-off
     * generation still keeps the candidate records few (3K + 64), so those and
     * the merge hash usually fit the LDS while the beam itself, its select
     * lists and the item list live in HBM (carveWs level 2). */
    if (d->kind == FLTX_DECODER_LEXICON && !forceWorstCaseCap && !d->forceGlobalWs && !leanInHbm && !d->noCut &&
        !d->opt.log_add && N <= 64) {
      const int64_t M = d->userCutM > 0 ? std::max<int64_t>(d->userCutM, K) : 3 * (int64_t)K + 64;
      d->cutM = (int)M;
      capC = std::max<int64_t>(M * 5 / 4 + 64, 256);
      d->itemCap = itemCap0;
      if (!d->noSlim) { /* HBM has room for the slim list of everything a frame can produce */
        d->CAP2 = (int)std::min<int64_t>(worst, std::max<int64_t>(4 * M, (int64_t)K * (nTok + 2) * 3));
      } else {
        d->CAP2 = 0;
        d->cutRecompute = 1;
      }
    }
  }
  d->CAP = (int)capC;
  d->HS = hsFor(capC);
  d->hotBytes = 0;
  d->hotLevel = 0;
  if (!lds) {
    d->hotLevel = 1;
    if (!leanInHbm) {
      size_t hb = 0;
      carveWs(tmp, nullptr, K, d->CAP, d->HS, d->NB, N, d->SCAP, d->dense, d->lane, d->CAP2, d->itemCap,
              d->threads / 64, 2, nullptr, &hb);
      if (hb <= kMaxLdsHw && d->maxHotLevel >= 2) {
        d->hotLevel = 2;
      }
    }
    d->wsBytes = carveWs(tmp, nullptr, K, d->CAP, d->HS, d->NB, N, d->SCAP, d->dense, d->lane, d->CAP2, d->itemCap,
                         d->threads / 64, d->hotLevel, nullptr, &d->hotBytes);
  } else {
    d->wsBytes = carveWs(tmp, nullptr, K, d->CAP, d->HS, d->NB, N, d->SCAP, d->dense, d->lane, d->CAP2, d->itemCap,
                         d->threads / 64);
  }
  d->wsInLds = lds;
  if (d->slane) {
    d->wsBytes = d->wlane          ? sizeof(WlaneLds)
                 : d->mlaneNG == 2 ? sizeof(MlaneLds<2>)
                 : d->mlaneNG == 4 ? sizeof(MlaneLds<4>)
                 : d->mlaneNG == 8 ? sizeof(MlaneLds<8>)
                 : d->tlane        ? sizeof(TlaneLds) + 8 * (size_t)d->tlEdgeSlots + 12 * (size_t)d->tlMaskSlots
                                   : offsetof(SlaneLds, amNB); /* (the stream variant's arrays are its last members) */
    d->wsInLds = true;
    lds = true;
  }
  if (d->ylane) {
    /* (shared-CU geometries: the part of YlaneLds::pscore their token waves use -- five waves x 512 floats with one lane
     * group, four with two -- so that two workgroups still fit a CU's 160 KB) */
    const size_t pscorePart = (size_t)(d->ylane == 2 ? 4 : 5) * 512 * sizeof(float);
    if (d->ylaneLm & 4) { /* several words per spelling: a larger merge table and the further words' lists (one workgroup per CU) */
      using YlaneLdsMl = YlaneLdsT<2, true>;
      using YlaneLdsMlLa = YlaneLdsT<2, true, true>;
      static_assert(offsetof(YlaneLdsMl, pscore) + 8 * 512 * sizeof(float) <= 160 * 1024, "one CU's LDS");
      /* (memo in HBM; one and two lane groups only; two groups: 768 threads, eight token waves' kept scores) */
      static_assert(offsetof(YlaneLdsMlLa, pscore) + 8 * 512 * sizeof(float) <= 160 * 1024, "one CU's LDS");
      d->wsBytes = ((d->ylaneLm & 8) ? offsetof(YlaneLdsMlLa, pscore) : offsetof(YlaneLdsMl, pscore)) +
                   (d->ylane == 2 ? (size_t)8 * 512 * sizeof(float) : pscorePart);
    } else if (d->ylaneLm & 8) { /* logAdd: the merge-table slots' sums */
      using YlaneLdsLa = YlaneLdsT<2, false, true>;
      using YlaneLdsLa4 = YlaneLdsT<4, false, true>;
      static_assert(sizeof(YlaneLdsLa) <= 160 * 1024 && offsetof(YlaneLdsLa4, memo) <= 160 * 1024, "one CU's LDS");
      d->wsBytes = d->ylane == 4 ? offsetof(YlaneLdsLa4, memo)
                                 : (d->yshare ? offsetof(YlaneLdsLa, pscore) + pscorePart : sizeof(YlaneLdsLa));
    } else {
      d->wsBytes = d->ylane == 4 ? offsetof(YlaneLdsT<4>, memo)
                                 : (d->yshare ? offsetof(YlaneLds, pscore) + pscorePart : sizeof(YlaneLds));
    }
    d->wsInLds = true;
    lds = true;
    d->itemCap = 0;
    d->CAP2 = 0;
    d->cutM = 0;
    d->cutRecompute = 0;
  }
  if (d->xlane) {
    d->wsBytes = d->yshare ? offsetof(XlaneLds, memo) : sizeof(XlaneLds);
    d->wsInLds = true;
    lds = true;
    d->itemCap = 0;
    d->CAP2 = 0;
    d->cutM = 0;
    d->cutRecompute = 0;
  }
  /* buffers */
  if (d->ylane && d->lm->kind == 1 && (d->xlmwordTrie != d->trie || d->xlmwordLm != d->lm)) { /* LM word ids of the lexicon's words */
    const std::vector<int32_t>& el = d->trie->xEndHost;
    std::vector<int32_t> w(el.size());
    for (size_t i = 0; i < el.size(); ++i) { /* KenLM::score: usrToLmIdxMap_, unknown words -> <unk> */
      w[i] = el[i] < 0 ? -1 : ((size_t)el[i] < d->lm->hUsr.size() ? d->lm->hUsr[(size_t)el[i]] : d->lm->unk);
    }
    if (d->xlmword.ensure(sizeof(int32_t) * std::max<size_t>(1, w.size()), st, false) ||
        devCopyH2D(d->xlmword.p, w.data(), sizeof(int32_t) * w.size(), st)) {
      return fail(FLTX_ERR_OOM, "LM word ids of the lexicon: upload failed");
    }
    devSync(st); /* (w is a local) */
    d->xlmwordTrie = d->trie;
    d->xlmwordLm = d->lm;
  }
  bool grewTab = false;
  int rc = 0;
  rc |= d->histOffD.ensure(sizeof(int64_t) * (B + 1), st, false);
  rc |= d->histPT.ensure(sizeof(int2) * (size_t)off, st, false);
  if (d->wlane) {
    rc |= d->tokRowsBuf.ensure(sizeof(WlTokRow) * ((size_t)off / (size_t)K + 1), st, false);
  }
  if (d->kind == FLTX_DECODER_LEXICON) {
    rc |= d->histW.ensure(sizeof(int32_t) * (size_t)off, st, false);
  }
  if (d->keepScores) {
    rc |= d->histS.ensure(sizeof(double) * 3 * (size_t)off, st, false);
  }
  if (cap != d->stateCap) {
    /* geometry changed: stale keys would hash to other slots; start clean */
    d->stateTab.cap = 0;
    if (d->stateTab.p) {
      devSync(st);
      devFree(d->stateTab.p);
      d->stateTab.p = nullptr;
    }
    d->stateCap = cap;
    d->epoch = 0;
  }
  /* (the lean / lane engines name their states with a counter and childTab: no table) */
  rc |= d->stateTab.ensure(sizeof(unsigned long long) * ((d->lean || d->tlane) ? 1 : (size_t)B * cap), st, true, &grewTab);
  if (grewTab) {
    d->epoch = 0;
  }
  if (d->lm->kind == 1 && !d->tlane) { /* (TL: a state's context is a row number kept with its lane) */
    rc |= d->stateCtx.ensure(sizeof(int32_t) * (size_t)B * cap * std::max(1, d->lm->order - 1), st, false);
  }
  size_t bk = (size_t)B * K;
  rc |= d->gScore.ensure(8 * bk, st, false) | d->gAm.ensure(8 * bk, st, false) | d->gLm.ensure(8 * bk, st, false);
  rc |= d->gState.ensure(4 * bk, st, false) | d->gSPar.ensure(4 * bk, st, false) | d->gSEdge.ensure(4 * bk, st, false);
  rc |= d->gLex.ensure(4 * bk, st, false) | d->gTokPb.ensure(4 * bk, st, false) | d->gLexMax.ensure(4 * bk, st, false);
  rc |= ensureUttRes(d, B, st);
  rc |= d->uttTotal.ensure(4 * (size_t)B, st, true);
  rc |= d->outN.ensure(4 * (size_t)B, st, true) | d->outScores.ensure(8 * bk * 3, st, false);
  for (int u = 0; u < 2; ++u) {
    rc |= d->emOff[u].ensure(sizeof(int64_t) * (size_t)B, st, false) | d->stepT[u].ensure(4 * (size_t)B, st, false);
  }
  if (!lds) {
    rc |= d->gws.ensure(d->wsBytes * (size_t)B, st, false);
  }
  d->idFamily = d->lean ? 0 : 1;
  if (d->lean && !d->slane) {
    d->idCap = std::min<int64_t>(d->recycle ? streamIds : (int64_t)K * (idT + 2) + 2, (1ll << 23) - 2);
    rc |= d->childTab.ensure(4 * (size_t)B * d->idCap * N, st, false);
    rc |= d->maskTab.ensure(8 * (size_t)B * d->idCap, st, false);
    rc |= d->uttNextId.ensure(4 * (size_t)B, st, true);
    rc |= d->gMask.ensure(8 * bk, st, false);
  } else if (d->recycle) {
    d->idCap = std::min<int64_t>(streamIds, (1ll << 23) - 2);
    rc |= d->uttNextId.ensure(4 * (size_t)B, st, true);
    rc |= d->stateVal.ensure(4 * (size_t)B * cap, st, false);
    rc |= d->idEdge.ensure(4 * (size_t)B * d->idCap, st, false);
  }
  if (d->recycle) {
    if (streamIds > (1ll << 23) - 2) {
      return fail(FLTX_ERR_UNSUPPORTED, "beam %d x max_frames %d exceeds the 2^23 LM-state ids a stream indexes", K, idT);
    }
    rc |= d->idPar.ensure(4 * (size_t)B * d->idCap, st, false) | d->idBorn.ensure(4 * (size_t)B * d->idCap, st, false);
    rc |= d->idKeep.ensure((size_t)B * d->idCap, st, false) | d->idNew.ensure(4 * (size_t)B * d->idCap, st, false);
    rc |= d->idList.ensure(4 * (size_t)B * d->idCap, st, false);
    d->idsFreeBound = (int64_t)K * (idT + 2);
  }
  if ((d->ylane || d->xlane) && d->yshare) {
    rc |= d->ymemo.ensure(sizeof(unsigned long long) * (size_t)d->ymemoSlots * (size_t)B, st, false); /* (wiped by the kernel) */
  }
  if (d->tlane && d->mlaneNG > 1) { /* the token-LM variant of fltx_mlane.h: its state-id table */
    rc |= d->ymemo.ensure(sizeof(unsigned long long) * (size_t)d->ymemoSlots * (size_t)B, st, false); /* (wiped by the kernel) */
  }
  d->useLmCache = d->lm->kind == 1 && !d->ylane && !d->xlane && !d->noLmCache;
  if (d->useLmCache) {
    /* (emptied here and at every new epoch: LM-state ids are table slots, a new batch gives them new meanings) */
    rc |= d->lmCache.ensure(8 * (size_t)kLmCache * (size_t)B, st, false);
    if (!rc) {
      devMemset(d->lmCache.p, 0xFF, 8 * (size_t)kLmCache * (size_t)B, st);
    }
  }
  if (d->lm->kind == 1) {
    rc |= d->scored.ensure(4 * (size_t)B, st, false);
    if (!rc && !d->keepScored) { /* (a partial re-run keeps the counts of the utterances it does not touch) */
      devMemset(d->scored.p, 0, 4 * (size_t)B, st);
    }
  }
  if (rc) {
    return fail(FLTX_ERR_OOM, "device allocation failed (B=%d K=%d T<=%d)", B, K, maxT);
  }
  if (uploadHistOff(d, st)) {
    return fail(FLTX_ERR_HIP, "upload failed");
  }
  return FLTX_OK;
}

void fillParams(fltx_decoder* d, DecodeParams& P) {
  memset(&P, 0, sizeof(P));
  P.K = d->opt.beam_size;
  P.Kt = d->opt.beam_size_token;
  P.beamThreshold = d->opt.beam_threshold;
  P.lmWeight = d->opt.lm_weight;
  P.wordScore = d->opt.word_score;
  P.unkScore = d->opt.unk_score;
  P.silScore = d->opt.sil_score;
  P.logAdd = d->opt.log_add;
  P.criterion = d->opt.criterion;
  P.sil = d->sil;
  P.blank = d->blank;
  P.unk = d->unk;
  P.isLmToken = d->isLmToken;
  P.kind = d->kind;
  P.N = d->N;
  P.transitions = d->nTrans ? d->transitions.as<float>() : nullptr;
  if (d->trie) {
    P.trieEdge = d->trie->edge.as<TrieEdge>();
    P.trieMask = d->trie->mask.p ? d->trie->mask.as<unsigned long long>() : nullptr;
    P.itemCap = P.trieMask ? d->itemCap : 0;
    P.itemWide = d->itemWide;
    P.trieLabels = d->trie->labels.as<int32_t>();
  }
  P.lmKind = d->lm->kind;
  P.lmOrder = d->lm->order;
  P.ngTab = d->lmDev ? d->lmDev->tab.as<NgramSlot>() : nullptr;
  P.ngMask = d->lm->mask;
  P.ngBackoff = d->lmDev ? d->lmDev->backoff.as<float>() : nullptr;
  P.usrToLm = d->lmDev ? d->lmDev->usrToLm.as<int32_t>() : nullptr;
  P.nUsr = d->lm->nUsr;
  P.lmBos = d->lm->bos;
  P.lmEos = d->lm->eos;
  P.lmUnk = d->lm->unk;
  P.stateCtx = d->stateCtx.as<int32_t>();
  P.emOff = d->emOff[d->upSlot].as<int64_t>();
  P.stepT = d->stepT[d->upSlot].as<int32_t>();
  P.uttNBeam = d->uttNBeam.as<int32_t>();
  P.uttFrame = d->uttFrame.as<int32_t>();
  P.uttTotal = d->uttTotal.as<int32_t>();
  P.uttStatus = d->uttStatus.as<int32_t>();
  P.gScore = d->gScore.as<double>();
  P.gAm = d->gAm.as<double>();
  P.gLm = d->gLm.as<double>();
  P.gState = d->gState.as<uint32_t>();
  P.gSPar = d->gSPar.as<uint32_t>();
  P.gSEdge = d->gSEdge.as<int32_t>();
  P.gLex = d->gLex.as<uint32_t>();
  P.gTokPb = d->gTokPb.as<uint32_t>();
  P.histPT = d->histPT.as<int2>();
  P.tokRows = d->wlane ? d->tokRowsBuf.p : nullptr;
  P.tokRowBlocks = d->wlane ? std::max(1, (d->wlMaxT + 3) / 4) : 1;
  P.histW = d->histW.as<int32_t>();
  P.histS = d->keepScores ? d->histS.as<double>() : nullptr;
  P.histOff = d->histOffD.as<int64_t>();
  P.stateTab = d->stateTab.as<unsigned long long>();
  P.stateCap = d->stateCap;
  P.epoch = d->epoch;
  P.CAP = d->CAP;
  P.HS = d->HS;
  P.NB = d->NB;
  P.SCAP = d->SCAP;
  P.dense = d->dense;
  P.lane = d->lane;
  P.CAP2 = d->CAP2;
  P.cutM = d->cutM;
  P.cutRecompute = d->cutRecompute;
  P.hotLevel = d->hotLevel;
  P.gLexMax = d->gLexMax.as<float>();
  P.gws = d->wsInLds ? nullptr : d->gws.as<char>();
  P.gwsStride = (int64_t)d->wsBytes;
  P.outN = d->outN.as<int32_t>();
  P.outScores = d->outScores.as<double>();
  P.childTab = d->childTab.as<uint32_t>();
  P.maskTab = d->maskTab.as<unsigned long long>();
  P.idCap = d->idCap;
  P.uttNextId = d->uttNextId.as<int32_t>();
  P.gMask = d->gMask.as<unsigned long long>();
  P.prof = nullptr;
  P.xnode = (d->trie && d->trie->xnode.p) ? d->trie->xnode.as<XNode>() : nullptr;
  P.xEndTok = d->trie ? d->trie->xEndTok : -1;
  P.xdelta = (d->trie && d->trie->xdelta.p) ? d->trie->xdelta.as<float>() : nullptr;
  P.xextra = (d->trie && d->trie->xextra.p) ? d->trie->xextra.as<uint32_t>() : nullptr;
  P.yTpw = d->ylaneTpw;
  P.xlmword = d->xlmword.p ? d->xlmword.as<int32_t>() : nullptr;
  P.ymemo = (((d->ylane || d->xlane) && d->yshare) || (d->tlane && d->mlaneNG > 1)) ? d->ymemo.as<unsigned long long>() : nullptr;
  P.ymemoSlots = d->ymemoSlots;
  P.yRankAt = d->userYRankAt;
  P.tune = d->userTune;
  P.statusHost = (!d->offlineCall && d->streamOpt) ? (int32_t*)d->hStat.p : nullptr;
  /* (the lean step on an HBM workspace reads its atomically ORed addMask words at L2 as well: wsLoadAtomic64) */
  P.wsNoInv = (!d->wsInLds && d->hotLevel >= 1) ? 1 : 0;
  P.lmCache = d->useLmCache ? d->lmCache.as<unsigned long long>() : nullptr;
  P.tokLm = d->tokLm; /* (null unless this is a lexicon-free decoder over an n-gram LM with a dense table) */
  P.tokLmStride = d->N + 1;
  P.tlEdgeSlots = d->tlEdgeSlots;
  P.tlMaskSlots = d->tlMaskSlots;
  P.yBound = d->trie ? std::max(0.0, std::max(d->opt.lm_weight * (double)d->trie->xDeltaMin,
                                              d->opt.lm_weight * (double)d->trie->xDeltaMax))
                     : 0.0;
  P.yTransMax = d->transMax;
  P.scored = (d->lm->kind == 1 && d->scored.p) ? d->scored.as<uint32_t>() : nullptr;
  if (d->recycle) {
    P.idPar = d->idPar.as<uint32_t>();
    P.idBorn = d->idBorn.as<uint32_t>();
    if (d->idFamily == 1) {
      P.idEdge = d->idEdge.as<int32_t>();
      P.stateVal = d->stateVal.as<uint32_t>();
    }
  }
  if (d->lm->kind == 2) {
    P.hlmQCap = d->hlmQCap;
    P.hlmQCount = (int32_t*)d->hlmQCount.p;
    P.hlmQ = (uint2*)d->hlmQ.p;
    P.hlmBeamN = (int32_t*)d->hlmBeamN.p;
    P.hlmBeam = (uint32_t*)d->hlmBeam.p;
  }
  P.profThread = 64 * d->profWave;
  if (d->profile && !d->prof.ensure(8 * 8 * (size_t)d->B, d->ctx->stream, true)) {
    devMemset(d->prof.p, 0, 8 * 8 * (size_t)d->B, d->ctx->stream);
    P.prof = d->prof.as<unsigned long long>();
  }
}

/* The lane-engine kernels, one entry per (family, variant, geometry) of fltx_engines.h.  The emulator build maps the
 * same entries to the host functions the kernels are made of (tests/emu/fltx_emu_launch.inc). */
enum LaneFamily { kGeneric, kSlane, kTlane, kSstream, kTstream, kMlane, kTmlane, kWlane, kXlane, kYlane };
enum { kVarLA = 1, kVarProf = 2, kVarHM = 4, kVarM32 = 8 }; /* logAdd merges, phase clocks, memo in HBM, 32-bit token masks */
struct LaneKey {
  int fam, var, threads, g[4];
};
#ifdef FLTX_EMU
using LaneFn = void (*)(const DecodeParams&, char*);
#define FLTX_LK(FAM, VAR, WW, A, B, C, D, KERNEL, EMU) {{FAM, VAR, WW, {A, B, C, D}}, EMU},
#else
using LaneFn = const void*;
#define FLTX_LK(FAM, VAR, WW, A, B, C, D, KERNEL, EMU) {{FAM, VAR, WW, {A, B, C, D}}, (const void*)KERNEL},
#endif
struct LaneKernel {
  LaneKey key;
  LaneFn fn;
};
#define FLTX_LK_SLANE(WW, GG)                                                                                       \
  FLTX_LK(kSlane, 0, WW, GG, 0, 0, 0, (fltx_decode_kernel_slane<WW, GG, false, false>), (slaneUtterance<GG, false, false, false>)) \
  FLTX_LK(kSlane, kVarProf, WW, GG, 0, 0, 0, (fltx_decode_kernel_slane<WW, GG, false, true>), (slaneUtterance<GG, false, false, true>)) \
  FLTX_LK(kSlane, kVarM32, WW, GG, 0, 0, 0, (fltx_decode_kernel_slane<WW, GG, false, false, true>), (slaneUtterance<GG, false, false, false, false, true>)) \
  FLTX_LK(kSlane, kVarM32 | kVarProf, WW, GG, 0, 0, 0, (fltx_decode_kernel_slane<WW, GG, false, true, true>), (slaneUtterance<GG, false, false, true, false, true>)) \
  FLTX_LK(kSlane, kVarLA, WW, GG, 0, 0, 0, (fltx_decode_kernel_slane<WW, GG, true, false>), (slaneUtterance<GG, true, false, false>)) \
  FLTX_LK(kTlane, 0, WW, GG, 0, 0, 0, (fltx_decode_kernel_tlane<WW, GG, false>), (slaneUtterance<GG, false, false, false, true>)) \
  FLTX_LK(kTlane, kVarLA, WW, GG, 0, 0, 0, (fltx_decode_kernel_tlane<WW, GG, true>), (slaneUtterance<GG, true, false, false, true>))
#define FLTX_LK_TLANE_PROF(WW, GG) \
  FLTX_LK(kTlane, kVarProf, WW, GG, 0, 0, 0, (fltx_decode_kernel_tlane<WW, GG, false, true>), (slaneUtterance<GG, false, false, false, true>))
#define FLTX_LK_SSTREAM(WW, GG)                                                                                     \
  FLTX_LK(kSstream, 0, WW, GG, 0, 0, 0, (fltx_decode_kernel_slane_stream<WW, GG>), (slaneUtterance<GG, false, true, false>)) \
  FLTX_LK(kTstream, 0, WW, GG, 0, 0, 0, (fltx_decode_kernel_tlane_stream<WW, GG>), (slaneUtterance<GG, false, true, false, true>))
#define FLTX_LK_MLANE(WW, GG, NG, GPW, SPW)                                                                        \
  FLTX_LK(kMlane, 0, WW, GG, NG, GPW, SPW, (fltx_decode_kernel_mlane<WW, GG, NG, GPW, SPW, false>), (mlaneUtterance<GG, NG, GPW, SPW, false>)) \
  FLTX_LK(kMlane, kVarLA, WW, GG, NG, GPW, SPW, (fltx_decode_kernel_mlane<WW, GG, NG, GPW, SPW, true>), (mlaneUtterance<GG, NG, GPW, SPW, true>))
#define FLTX_LK_TMLANE(WW, GG, NG, GPW, SPW)                                                                       \
  FLTX_LK(kTmlane, 0, WW, GG, NG, GPW, SPW, (fltx_decode_kernel_tmlane<WW, GG, NG, GPW, SPW, false>), (mlaneUtterance<GG, NG, GPW, SPW, false, true>)) \
  FLTX_LK(kTmlane, kVarLA, WW, GG, NG, GPW, SPW, (fltx_decode_kernel_tmlane<WW, GG, NG, GPW, SPW, true>), (mlaneUtterance<GG, NG, GPW, SPW, true, true>))
#define FLTX_LK_WLANE(WW, GG) FLTX_LK(kWlane, 0, WW, GG, 0, 0, 0, (fltx_decode_kernel_wlane<WW, GG>), (wlaneUtterance<GG>))
#define FLTX_LK_XLANE(WW, GG)                                                                                       \
  FLTX_LK(kXlane, 0, WW, GG, 0, 0, 0, (fltx_decode_kernel_xlane<WW, GG, 0, false>), (xlaneUtterance<GG, 0, false>))  \
  FLTX_LK(kXlane, kVarProf, WW, GG, 0, 0, 0, (fltx_decode_kernel_xlane<WW, GG, 0, true>), (xlaneUtterance<GG, 0, false>)) \
  FLTX_LK(kXlane, kVarHM, WW, GG, 0, 0, 0, (fltx_decode_kernel_xlane<WW, GG, 1, false>), (xlaneUtterance<GG, 1, false>)) \
  FLTX_LK(kXlane, kVarLA, WW, GG, 0, 0, 0, (fltx_decode_kernel_xlane<WW, GG, 0, false, true>), (xlaneUtterance<GG, 0, false, true>)) \
  FLTX_LK(kXlane, kVarLA | kVarHM, WW, GG, 0, 0, 0, (fltx_decode_kernel_xlane<WW, GG, 1, false, true>), (xlaneUtterance<GG, 1, false, true>))
#define FLTX_LK_YLANE(WW, NG, RR, HM, LMK) \
  FLTX_LK(kYlane, HM ? kVarHM : 0, WW, NG, RR, LMK, 0, (fltx_decode_kernel_ylane<WW, NG, RR, LMK, HM, false>), (ylaneUtterance<NG, RR, LMK, HM, false>))
#define FLTX_LK_YLANE_PROF(WW, NG, RR, HM, LMK) \
  FLTX_LK(kYlane, (HM ? kVarHM : 0) | kVarProf, WW, NG, RR, LMK, 0, (fltx_decode_kernel_ylane<WW, NG, RR, LMK, HM, true>), (ylaneUtterance<NG, RR, LMK, HM, false>))
static const LaneKernel kLaneKernels[] = {
    FLTX_SLANE_GEOS(FLTX_LK_SLANE) FLTX_TLANE_PROF_GEOS(FLTX_LK_TLANE_PROF) FLTX_SSTREAM_GEOS(FLTX_LK_SSTREAM)
    FLTX_MLANE_GEOS(FLTX_LK_MLANE) FLTX_TMLANE_GEOS(FLTX_LK_TMLANE) FLTX_WLANE_GEOS(FLTX_LK_WLANE)
    FLTX_XLANE_GEOS(FLTX_LK_XLANE) FLTX_YLANE_KERNELS(FLTX_LK_YLANE) FLTX_YLANE_GEOS(FLTX_YLMK_01, FLTX_LK_YLANE_PROF)};
#undef FLTX_LK
#undef FLTX_LK_SLANE
#undef FLTX_LK_TLANE_PROF
#undef FLTX_LK_SSTREAM
#undef FLTX_LK_MLANE
#undef FLTX_LK_TMLANE
#undef FLTX_LK_WLANE
#undef FLTX_LK_XLANE
#undef FLTX_LK_YLANE
#undef FLTX_LK_YLANE_PROF

/* what launchDecode runs: the lane engine's family, variant and geometry (kGeneric: the per-W kernels) */
LaneKey laneKeyOf(const fltx_decoder* d) {
  const int W = d->sstreamLaunch ? d->sstreamThreads : d->threads;
  const int la = d->opt.log_add ? kVarLA : 0, prof = d->profile ? kVarProf : 0, hm = d->yshare ? kVarHM : 0;
  if (d->sstreamLaunch) {
    return {d->tstream ? kTstream : kSstream, prof, W, {d->sstream, 0, 0, 0}};
  } else if (d->ylane) { /* (logAdd: LMK bit 3) */
    return {kYlane, prof | hm, W, {d->ylane, d->ylaneRounds, d->ylaneLm, 0}};
  } else if (d->xlane) {
    return {kXlane, la | prof | hm, W, {d->xlane, 0, 0, 0}};
  } else if (d->slane && d->mlaneNG > 1) {
    return {d->tlane ? kTmlane : kMlane, la | prof, W, {d->slane, d->mlaneNG, d->mlaneGPW, d->mlaneSPW}};
  } else if (d->slane && d->wlane) {
    return {kWlane, prof, W, {d->slane, 0, 0, 0}};
  } else if (d->slane) {
    return {d->tlane ? kTlane : kSlane, la | prof | (slaneM32(d) ? kVarM32 : 0), W, {d->slane, 0, 0, 0}};
  }
  return {kGeneric, 0, W, {0, 0, 0, 0}};
}

/* the kernel of a lane engine's key; a variant without phase clocks stands in for a missing phase-clock variant */
const LaneKernel* findLaneKernel(LaneKey k) {
  for (int pass = 0; pass < 2; ++pass, k.var &= ~kVarProf) {
    for (const LaneKernel& e : kLaneKernels) {
      if (e.key.fam == k.fam && e.key.var == k.var && e.key.threads == k.threads && e.key.g[0] == k.g[0] &&
          e.key.g[1] == k.g[1] && e.key.g[2] == k.g[2] && e.key.g[3] == k.g[3]) {
        return &e;
      }
    }
  }
  return nullptr;
}

/* dynamic LDS of the launch */
size_t launchLds(const fltx_decoder* d, const LaneKey& k) {
  if (k.fam == kSstream) {
    return sizeof(SlaneLds);
  } else if (k.fam == kTstream) {
    return sizeof(TlaneLds) + (size_t)(k.threads / 64) * kTlGatherBytes;
  }
  return (k.fam == kGeneric && !d->wsInLds) ? d->hotBytes : d->wsBytes;
}

#ifndef FLTX_EMU
/* the generic / lean / lane-per-slot kernels of one workgroup size */
template <int W>
const void* genericKernel(const fltx_decoder* d) {
  const bool la = d->opt.log_add, ft = d->opt.beam_size_token >= d->N;
  if (!d->wsInLds) {
    return d->lean ? (const void*)fltx_decode_kernel_gwslean<W> : (const void*)fltx_decode_kernel_gws<W>;
  } else if (d->lane == 4) {
    return la ? (ft ? (const void*)fltx_decode_kernel_lane<W, 4, true, true> : (const void*)fltx_decode_kernel_lane<W, 4, true, false>)
              : (ft ? (const void*)fltx_decode_kernel_lane<W, 4, false, true> : (const void*)fltx_decode_kernel_lane<W, 4, false, false>);
  } else if (d->lane == 8) {
    return la ? (ft ? (const void*)fltx_decode_kernel_lane<W, 8, true, true> : (const void*)fltx_decode_kernel_lane<W, 8, true, false>)
              : (ft ? (const void*)fltx_decode_kernel_lane<W, 8, false, true> : (const void*)fltx_decode_kernel_lane<W, 8, false, false>);
  } else if (d->lean == 6) {
    return (const void*)fltx_decode_kernel_lds<W, 6>;
  } else if (d->lean == 12) {
    return (const void*)fltx_decode_kernel_lds<W, 12>;
  } else if (d->lean == 255) {
    return (const void*)fltx_decode_kernel_lds<W, 255>;
  } else if (d->kind == FLTX_DECODER_LEXICON && !d->isLmToken && d->lm->kind == 0) {
    return (const void*)fltx_decode_kernel_lds_spec<W, true, true>;
  } else if (d->kind == FLTX_DECODER_LEXICON && !d->isLmToken && d->lm->kind == 1) {
    return (const void*)fltx_decode_kernel_lds_spec<W, true, false>;
  } else if (d->lm->kind == 0 && !d->isLmToken) {
    return (const void*)fltx_decode_kernel_lds_spec<W, false, true>;
  }
  return (const void*)fltx_decode_kernel_lds<W, 0>;
}

/* hipFuncAttributeMaxDynamicSharedMemorySize of a kernel: raised when a launch needs more than it was set to, once per
 * (device, kernel, bytes) -- under defer_check two host threads launch */
int raiseMaxLds(int device, const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> set;
  std::lock_guard<std::mutex> lock(mu);
  auto it = set.find({device, fn});
  if (it == set.end() || it->second < bytes) {
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    set[{device, fn}] = bytes;
  }
  return FLTX_OK;
}
/* ... and per decoder object nothing at all while it launches the same kernel within what it last asked for (which: 0 the
 * decode kernel, 1 the back-trace) */
int raiseMaxLdsOnce(fltx_decoder* d, int which, const void* fn, size_t bytes) {
  if (d->ldsRaisedFn[which] == fn && bytes <= d->ldsRaisedTo[which]) {
    return FLTX_OK;
  }
  int rc = raiseMaxLds(d->ctx->device, fn, bytes);
  if (!rc) {
    d->ldsRaisedFn[which] = fn;
    d->ldsRaisedTo[which] = bytes;
  }
  return rc;
}
#endif

int launchDecode(fltx_decoder* d, const DecodeParams& P) {
  const LaneKey key = laneKeyOf(d);
  const LaneKernel* lane = key.fam == kGeneric ? nullptr : findLaneKernel(key);
  if (key.fam != kGeneric && !lane) {
    return fail(FLTX_ERR_INVALID, "no kernel of lane engine %d (variant %d) for %d threads x (%d, %d, %d, %d)", key.fam,
                key.var, key.threads, key.g[0], key.g[1], key.g[2], key.g[3]);
  }
  const int W = key.threads;
  const int nGrid = d->nLaunch > 0 ? d->nLaunch : d->B;
  const size_t lds = launchLds(d, key);
#ifdef FLTX_EMU
#include "fltx_emu_launch.inc" /* tests/emu/: host-thread dispatch over the kernel variants */
#else
  for (int i = 0; i < 3; ++i) {
    if (!d->ev[i]) {
      HIPCHK(hipEventCreate(&d->ev[i]));
    }
  }
  HIPCHK(hipEventRecord(d->ev[0], d->ctx->stream));
  const void* fn = lane ? lane->fn : nullptr;
  switch (lane ? 0 : W) {
    case 0: break;
    case 64: fn = genericKernel<64>(d); break;
    case 128: fn = genericKernel<128>(d); break;
    case 256: fn = genericKernel<256>(d); break;
    case 512: fn = genericKernel<512>(d); break;
    case 1024: fn = genericKernel<1024>(d); break;
    default: return fail(FLTX_ERR_INVALID, "threads per utterance must be 64, 128, 256, 512 or 1024");
  }
  if (key.fam == kWlane && d->wlMaxT > 0) { /* the token beams of all rows first (same stream) */
    hipLaunchKernelGGL(fltx_tokbeam_kernel, dim3((unsigned)(P.tokRowBlocks * nGrid)), dim3(256), 4 * sizeof(WlFrontLds),
                       d->ctx->stream, P);
  }
  /* (slane, the stream chunks and gwslean launch within the default limit, as they always have) */
  const bool defaultLimit = key.fam == kSlane || key.fam == kSstream || key.fam == kTstream ||
                            (key.fam == kGeneric && !d->wsInLds && d->lean);
  int rc;
  if (!defaultLimit && (rc = raiseMaxLdsOnce(d, 0, fn, lds))) {
    return rc;
  }
  void* args[] = {(void*)&P};
  HIPCHK(hipLaunchKernel(fn, dim3(nGrid), dim3(W), args, lds, d->ctx->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(d->ev[1], d->ctx->stream));
  d->timed = false;
  return FLTX_OK;
#endif
}

int bumpEpoch(fltx_decoder* d) {
  if (d->epoch >= 65535u) {
    /* the whole allocation, not just this batch's part: a larger earlier batch left keys tagged
     * with epochs that are about to be reused */
    if (devMemset(d->stateTab.p, 0, d->stateTab.cap, d->ctx->stream)) {
      return fail(FLTX_ERR_HIP, "state table reset failed");
    }
    d->epoch = 0;
  }
  d->epoch += 1;
  if (d->useLmCache && d->lmCache.p && devMemset(d->lmCache.p, 0xFF, d->lmCache.cap, d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "LM score cache reset failed");
  }
  return FLTX_OK;
}

int uploadStep(fltx_decoder* d, const float* emissions, int onDevice, const int64_t* offsets,
               const int32_t* T, DecodeParams& P) {
  Stream st = d->ctx->stream;
  const int B = d->B, N = d->N;
  int64_t maxEnd = 0;
  for (int b = 0; b < B; ++b) {
    if (offsets && offsets[b] < 0) {
      return fail(FLTX_ERR_INVALID, "offsets[%d] is negative", b);
    }
    maxEnd = std::max<int64_t>(maxEnd, (offsets ? offsets[b] : 0) + (int64_t)T[b] * N);
  }
  if (maxEnd > 0 && !emissions) {
    return fail(FLTX_ERR_INVALID, "emissions is null");
  }
#ifdef FLTX_EMU
  const int slot = d->offlineCall ? d->upSlot : d->upSlot ^ 1; /* (streams take turns on the two slots as on the device:
                                                                   a deferred second pass reads the previous chunk's) */
  Stream cs = st;
#else
  /* Stream chunks go to the other slot on a copy stream: it waits for what read that slot two steps ago, not for
   * the kernel of the step before, which is still running (the chunk's H2D under the previous chunk's kernel).
   * Offline batches upload on the launch stream as before (two decoder objects overlap them: bench.py). */
  int slot = d->upSlot;
  Stream cs = st;
  if (!d->offlineCall) {
    if (!d->copyStream) {
      HIPCHK(hipStreamCreateWithFlags(&d->copyStream, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&d->evSlotFree[0], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&d->evSlotFree[1], hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(d->evSlotFree[d->upSlot], st)); /* everything queued so far may read the current slot */
    d->slotUsed[d->upSlot] = true;
    slot = d->upSlot ^ 1;
    cs = d->copyStream;
    if (d->slotUsed[slot]) {
      HIPCHK(hipStreamWaitEvent(cs, d->evSlotFree[slot], 0));
    }
  }
#endif
  if (onDevice) {
    P.emissions = emissions;
  } else {
    if (d->emis[slot].ensure(sizeof(float) * (size_t)std::max<int64_t>(maxEnd, 1), st, false)) {
      return fail(FLTX_ERR_OOM, "emissions staging allocation failed");
    }
    if (maxEnd > 0 && devCopyH2D(d->emis[slot].p, emissions, sizeof(float) * (size_t)maxEnd, cs)) {
      return fail(FLTX_ERR_HIP, "emissions upload failed");
    }
    P.emissions = d->emis[slot].as<float>();
  }
  d->lastEmis = P.emissions;
  /* the batch descriptors go through the slot's pinned staging: the copies are asynchronous for real, and nothing
   * of this call has to outlive it */
  int64_t* offs = (int64_t*)d->descStage[slot].acquire(12 * (size_t)B);
  if (!offs) {
    return fail(FLTX_ERR_HIP, "batch descriptor staging failed");
  }
  int32_t* stT = (int32_t*)(offs + B);
  for (int b = 0; b < B; ++b) {
    offs[b] = offsets ? offsets[b] : 0;
    stT[b] = T[b];
  }
  if (devCopyH2D(d->emOff[slot].p, offs, sizeof(int64_t) * B, cs) ||
      devCopyH2D(d->stepT[slot].p, stT, sizeof(int32_t) * B, cs) || d->descStage[slot].sent(cs)) {
    return fail(FLTX_ERR_HIP, "batch descriptor upload failed");
  }
  d->upSlot = slot;
  P.emOff = d->emOff[slot].as<int64_t>();
  P.stepT = d->stepT[slot].as<int32_t>();
#ifndef FLTX_EMU
  /* A stream chunk's copies run on the copy stream: when it is drained they are in place for the launch that follows
   * on the other stream.  An offline batch uploads on its launch stream, which orders them before the kernel: it waits
   * only where the caller's own (pageable) emissions have to be consumed before the call returns. */
  if ((!d->offlineCall || (!onDevice && maxEnd > 0)) && devSync(cs)) {
    return fail(FLTX_ERR_HIP, "stream synchronize failed");
  }
#endif
  return FLTX_OK;
}

int settleStream(fltx_decoder* d);
} // namespace
static int offlineAttempts(fltx_decoder* d, const float* emissions, int32_t onDevice, int firstAttempt);
namespace {

int syncResults(fltx_decoder* d) {
  if (!d->settling && (d->chunkPending || d->pendingPrune >= 0)) {
    int rc = settleStream(d);
    if (rc) {
      return rc;
    }
  }
  if (d->offlinePending) { /* "defer_check": the look at the batch's statuses, and the second pass of what the fast path flagged */
    d->offlinePending = false;
    d->upSlot = d->offUpSlot;
    int rc = offlineAttempts(d, d->offEmis, 1, 1);
    if (rc) {
      return rc;
    }
  }
  if (d->resultsSynced) {
    return FLTX_OK;
  }
  Stream st = d->ctx->stream;
  const int B = d->B;
  d->hN.resize(B);
  d->hFrame.resize(B);
  d->hStatus.resize(B);
  /* the three rows share an allocation (ensureUttRes): one copy into pinned staging, one wait */
  const size_t row = d->uttRow;
  if (d->hSync.ensure(4 * (2 * row + (size_t)B))) {
    return fail(FLTX_ERR_OOM, "pinned staging allocation failed");
  }
  const int32_t* h = (const int32_t*)d->hSync.p;
  if (d->lookQueued) { /* the rows were copied right behind the back-trace (queueLook): wait for them, no copy, no stream drained */
    d->lookQueued = false;
#ifndef FLTX_EMU
    if (hipEventSynchronize(d->lookEv) != hipSuccess) {
      return fail(FLTX_ERR_HIP, "result copy failed: %s", devErr());
    }
#endif
  } else if (devCopyD2H(d->hSync.p, d->uttRes.p, 4 * (2 * row + (size_t)B), st)) {
    return fail(FLTX_ERR_HIP, "result copy failed: %s", devErr());
  }
  memcpy(d->hN.data(), h, 4 * (size_t)B);
  memcpy(d->hFrame.data(), h + row, 4 * (size_t)B);
  memcpy(d->hStatus.data(), h + 2 * row, 4 * (size_t)B);
  d->resultsSynced = true;
  return FLTX_OK;
}

int launchBacktrace(fltx_decoder* d) {
  Stream st = d->ctx->stream;
  if (d->tokens.ensure(4 * (size_t)std::max<int64_t>(d->histRecords, 1), st, false)) {
    return fail(FLTX_ERR_OOM, "token buffer allocation failed");
  }
  if (d->kind == FLTX_DECODER_LEXICON &&
      d->words.ensure(4 * (size_t)std::max<int64_t>(d->histRecords, 1), st, false)) {
    return fail(FLTX_ERR_OOM, "word buffer allocation failed");
  }
  BacktraceParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.K = d->opt.beam_size;
  Q.kind = d->kind;
  Q.histPT = d->histPT.as<int2>();
  Q.histW = d->histW.as<int32_t>();
  Q.histOff = d->histOffD.as<int64_t>();
  Q.uttFrame = d->uttFrame.as<int32_t>();
  Q.uttNBeam = d->uttNBeam.as<int32_t>();
  Q.tokOff = d->histOffD.as<int64_t>();
  Q.tokens = d->tokens.as<int32_t>();
  Q.words = d->kind == FLTX_DECODER_LEXICON ? d->words.as<int32_t>() : nullptr;
  Q.nbest = 0;
  /* frames per LDS chunk: two record buffers in ({parent, token} 8 B, word 4 B) + token and word tiles out */
#ifdef FLTX_EMU
  const int btAsked = d->btThreads ? d->btThreads : 64;
#else
  const int btAsked = d->btThreads ? d->btThreads : 512;
#endif
  /* (the score passes are one thread per hypothesis: a workgroup never has fewer threads than the beam has slots,
   * whatever "bt_threads" asks for) */
  const int btThreads = std::min(512, std::max(btAsked, (d->opt.beam_size + 63) / 64 * 64));
  const size_t perFrame = (size_t)Q.K * (2 * (8 + (d->kind == FLTX_DECODER_LEXICON ? 4 : 0)) + 8);
  /* 140 KB: leaves a CU room for a 16 KB decode workgroup of the next batch beside a back-trace workgroup */
  size_t btBudget = 0;
  int F = 0;
  auto chunkFor = [&](size_t budget) {
    btBudget = budget;
    F = (int)std::min<size_t>(btBudget / perFrame, 512);
    if (d->batchPacked) { /* the emission rows, transitions and addends of a chunk share the same LDS (amLds below) */
      /* (fltx_wlane.h's token sets: the tokens of the paths only, emissions and transitions read where needed) */
      const size_t fixed = d->batchWlane ? 16 : 4 * ((d->opt.criterion == FLTX_CRITERION_ASG && d->nTrans) ? (size_t)d->N * d->N : 0) + 16;
      const size_t perAm = 4 * ((d->batchWlane ? 0 : (size_t)d->N) + (size_t)Q.K);
      const size_t room = btBudget > fixed ? btBudget - fixed : 0;
      F = (int)std::min<size_t>((size_t)F, room / perAm);
    }
    if (F < 8 || Q.K > 4 * btThreads) {
      F = 0;
    }
  };
  chunkFor((size_t)(d->btLdsKb > 0 ? std::min(d->btLdsKb, 144) : 140) * 1024);
  if (F == 0 && d->btLdsKb > 0) {
    chunkFor((size_t)144 * 1024); /* (the caller's budget holds no chunk of this beam: the tunable yields, the decode does not fail) */
  }
  if (d->batchPacked && F == 0) {
    return fail(FLTX_ERR_UNSUPPORTED, "back-trace: packed history records need an LDS chunk (K=%d N=%d)", Q.K, d->N);
  }
  Q.F = F;
  size_t btLds = F > 0 ? (size_t)F * perFrame + 16 : 16;
  if (d->batchPacked && F > 0) { /* packed records; emitting-model scores re-accumulated along the paths */
    Q.packed = d->packedBits;
    Q.packedTokMask = d->batchWlane ? 0x7FFFFFFF : 0xFF;
    Q.amGather = d->batchWlane ? 1 : 0;
    Q.uttStatus = d->uttStatus.as<int32_t>();
    Q.amOut = d->outScores.as<double>();
    Q.emissions = d->lastEmis;
    Q.emOff = d->emOff[d->upSlot].as<int64_t>();
    Q.N = d->N;
    Q.transitions = (d->opt.criterion == FLTX_CRITERION_ASG && d->nTrans) ? d->transitions.as<float>() : nullptr;
    Q.tokLm = d->batchTlane ? d->tokLm : nullptr;
    Q.tokLmStride = d->N + 1;
    Q.blank = d->opt.criterion == FLTX_CRITERION_CTC ? d->blank : -1;
    const size_t amLds = Q.amGather ? 4 * (size_t)Q.K * F + 16
                                    : 4 * ((size_t)F * d->N + (Q.transitions ? (size_t)d->N * d->N : 0) + (size_t)Q.K * F) + 16;
    btLds = std::max(btLds, amLds);
  }
  /* Packed records in one residency (backtraceNarrow): the batch's longest token tile at the narrow width, and behind
   * it, within the same budget, double-buffered chunks of narrowed records (walk) and then of emission rows (score).
   * 8 + 8 bits when slots and tokens both fit a byte beside the all-ones "none", 16 + 16 otherwise.  A budget that
   * holds no tile with chunks of 8 frames keeps backtraceUtterance (long utterances, big beams). */
  int narrow = 0; /* bytes of a narrowed record: 2, 4, or 0 = backtraceUtterance */
  int walkWaves = 1; /* waves that walk a chunk: 1 = one walk per hypothesis */
  if (d->batchPacked && F > 0 && Q.K <= btThreads) {
    const bool byteRec = d->packedBits <= 8 && Q.packedTokMask == 0xFF && d->N <= 255;
    const bool wordRec = d->packedBits <= 16 && d->N <= 65535;
    const size_t rec = byteRec ? 2 : 4, tokB = rec / 2;
    size_t row = 0;
    for (int b = 0; b < d->B; ++b) {
      row = std::max<size_t>(row, (size_t)((d->histOff[b + 1] - d->histOff[b]) / Q.K));
    }
    const bool lexRec = d->kind == FLTX_DECODER_LEXICON;
    const size_t tile = ((size_t)Q.K * row * tokB + 15) & ~(size_t)15;
    const size_t room = btBudget > tile + 16 ? btBudget - tile - 16 : 0;
    const size_t perWalk = (size_t)Q.K * (2 * rec + (lexRec ? 2 * 4 + 4 : 0));
    const size_t trBytes = (Q.transitions && !Q.amGather) ? btTransBytes(d->N) : 0;
    const size_t npF = std::min<size_t>(room / perWalk, std::max<size_t>(row, 8));
    /* the score pass: two buffers of addends by hypothesis (floats; f64 sums with transitions), padded rows
     * (btAddStride), and for the parallel walk under a token LM the stretch's tokens by hypothesis -> the longest
     * stretch that `avail` bytes hold */
    const bool withTrans = Q.transitions != nullptr;
    auto stretchFor = [&](size_t avail, bool tokRows) {
      const size_t perFe = (size_t)2 * Q.K * (withTrans ? 8 : 4) + (tokRows ? (size_t)2 * Q.K * tokB : 0);
      size_t fe = std::min<size_t>(avail / perFe, std::max<size_t>(row, 8));
      while (fe > 0 && btScoreBytes(Q.K, (int)fe, withTrans, tokRows, (int)tokB) > avail) {
        --fe;
      }
      return fe;
    };
    const size_t npFe = room > trBytes ? stretchFor(room - trBytes, false) : 0;
    /* The parallel walk (K <= 64: a lane per slot; two waves or more): ONE chunk buffer, the waves' exit maps beside
     * it, and between the tile and all that the entry map [chunk][wave][K], which the score pass still reads.  The
     * chunk keeps the length the double-buffered walk has (short chunks cost the parallel walk a barrier, not a
     * serial stretch), so the buffer it no longer doubles pays for the maps; where they do not fit, and for beams
     * beyond 64 -- their walk is already spread over K / 64 waves, and they are not where the time is -- the walk
     * stays serial. */
    const size_t nW = (size_t)btThreads / 64;
    if ((byteRec || wordRec) && Q.K <= 64 && nW >= 2 && d->btWalkAsked != 1 && row > 0 && row < (1u << 24) && npF >= 8) {
      /* (the records of a chunk, rounded up to 16 bytes so that the int32 words behind them stay aligned) */
      const size_t pwChunk = (((size_t)Q.K * npF * rec + 15) & ~(size_t)15) + (lexRec ? (size_t)Q.K * npF * (4 + 4) : 0);
      const size_t exitB = (nW * Q.K + 15) & ~(size_t)15;
      const size_t ent = ((size_t)Q.K * nW * ((row + npF - 1) / npF) + 15) & ~(size_t)15;
      const size_t roomE = room > ent ? room - ent : 0;
      const bool tokRows = Q.tokLm != nullptr;
      const size_t pwFe = roomE > trBytes ? stretchFor(roomE - trBytes, tokRows) : 0;
      if (ent + exitB + pwChunk <= room && pwFe >= 8) {
        narrow = (int)rec;
        walkWaves = (int)nW;
        Q.npRow = (int32_t)row;
        Q.npF = (int32_t)npF;
        Q.npFe = (int32_t)pwFe;
        Q.npWaves = (int32_t)nW;
        Q.npEntry = (int32_t)tile;
        Q.npScratch = (int32_t)(tile + ent);
        btLds = std::max(btLds, tile + ent + std::max(exitB + pwChunk, trBytes + btScoreBytes(Q.K, (int)pwFe, withTrans, tokRows, (int)tokB)) + 16);
      }
    }
    if (!narrow && (byteRec || wordRec) && row > 0 && row < (1u << 24) && npF >= 8 && npFe >= 8) {
      narrow = (int)rec;
      Q.npRow = (int32_t)row;
      Q.npF = (int32_t)npF;
      Q.npFe = (int32_t)npFe;
      Q.npScratch = (int32_t)tile;
      btLds = std::max(btLds, tile + std::max(npF * perWalk, trBytes + btScoreBytes(Q.K, (int)npFe, withTrans, false, (int)tokB)) + 16);
    }
  }
  if (narrow && d->btProfile) {
    if (d->btProf.ensure(8 * (size_t)kBtProfMarks * d->B, st, true)) {
      return fail(FLTX_ERR_OOM, "back-trace profile allocation failed");
    }
    devMemset(d->btProf.p, 0, 8 * (size_t)kBtProfMarks * d->B, st);
    Q.btProf = d->btProf.as<unsigned long long>();
  }
  d->btWalkWaves = walkWaves;
  d->btNarrow = narrow;
  d->btChunk = narrow ? Q.npF : F;
  d->btStretch = narrow ? Q.npFe : (d->batchPacked && !Q.amGather ? F : 0);
#ifdef FLTX_EMU
  const BacktraceParams* qq = &Q;
  if (narrow == 2 && walkWaves > 1) {
    emuLaunch(d->B, btThreads, btLds, [qq](char* smem) { backtraceNarrow<uint16_t, true>(*qq, smem); });
  } else if (narrow == 4 && walkWaves > 1) {
    emuLaunch(d->B, btThreads, btLds, [qq](char* smem) { backtraceNarrow<uint32_t, true>(*qq, smem); });
  } else if (narrow == 2) {
    emuLaunch(d->B, btThreads, btLds, [qq](char* smem) { backtraceNarrow<uint16_t, false>(*qq, smem); });
  } else if (narrow == 4) {
    emuLaunch(d->B, btThreads, btLds, [qq](char* smem) { backtraceNarrow<uint32_t, false>(*qq, smem); });
  } else {
    emuLaunch(d->B, btThreads, btLds, [qq](char* smem) { backtraceUtterance(*qq, smem); });
  }
#else
  const void* btFn = narrow == 2   ? (walkWaves > 1 ? (const void*)fltx_backtrace_narrow_kernel<uint16_t, true>
                                                   : (const void*)fltx_backtrace_narrow_kernel<uint16_t, false>)
                     : narrow == 4 ? (walkWaves > 1 ? (const void*)fltx_backtrace_narrow_kernel<uint32_t, true>
                                                   : (const void*)fltx_backtrace_narrow_kernel<uint32_t, false>)
                                   : (const void*)fltx_backtrace_kernel;
  int rcLds = raiseMaxLdsOnce(d, 1, btFn, btLds);
  if (rcLds) {
    return rcLds;
  }
  void* btArgs[] = {(void*)&Q};
  HIPCHK(hipLaunchKernel(btFn, dim3(d->B), dim3(btThreads), btArgs, btLds, st));
  HIPCHK(hipGetLastError());
  if (d->ev[2]) {
    HIPCHK(hipEventRecord(d->ev[2], st));
    d->timed = true;
  }
#endif
  d->backtraced = true;
  return FLTX_OK;
}

/* SURVEY.md section 8(d), per utterance: decode phase = T x (4N + 8K (+ 4*K*Kt + 8K + 4K for the
 * lexicon decoder)) + 16 * order per n-gram LM query the kernel issued; epilogue = 16 * H * (T + 2)
 * for the H hypotheses actually returned.  Needs the result counts: evaluated when asked for. */
int accountBytes(fltx_decoder* d) {
  if (d->statsDone) {
    return FLTX_OK;
  }
  const int64_t K = d->opt.beam_size, N = d->N;
  const int64_t Kt = std::min<int64_t>(d->opt.beam_size_token, N);
  int rc = syncResults(d);
  if (rc) {
    return rc;
  }
  std::vector<uint32_t> scored(d->B, 0u);
  if (d->lm->kind == 1 && d->scored.p &&
      devCopyD2H(scored.data(), d->scored.p, 4 * (size_t)d->B, d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "counter copy failed");
  }
  int64_t frames = 0, dec = 0, epi = 0, lm = 0;
  for (int b = 0; b < d->B; ++b) {
    const int64_t T = d->T[b];
    frames += T;
    int64_t per = 4 * N + 8 * K;
    if (d->kind == FLTX_DECODER_LEXICON) {
      per += 4 * K * Kt + 8 * K + 4 * K;
    }
    dec += per * T;
    lm += 16 * (int64_t)d->lm->order * (int64_t)scored[b];
    epi += 16 * (int64_t)d->hN[b] * (T + 2);
  }
  d->statFrames = frames;
  d->statDecodeBytes = dec + lm;
  d->statLmBytes = lm;
  d->statEpilogueBytes = epi;
  d->statBytes = dec + lm + epi;
  d->statsDone = true;
  return FLTX_OK;
}

/* save (dir 0) / put back (dir 1; `map`: device list of n utterances, null = all) the parked beams */
int streamSnapshot(fltx_decoder* d, int dir, const int32_t* map, int n) {
  SnapParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.K = d->opt.beam_size;
  Q.dir = dir;
  Q.map = map;
  Q.gScore = d->gScore.as<double>();
  Q.gAm = d->gAm.as<double>();
  Q.gLm = d->gLm.as<double>();
  Q.gLexMax = d->gLexMax.as<float>();
  Q.gState = d->gState.as<uint32_t>();
  Q.gSPar = d->gSPar.as<uint32_t>();
  Q.gLex = d->gLex.as<uint32_t>();
  Q.gTokPb = d->gTokPb.as<uint32_t>();
  Q.gSEdge = d->gSEdge.as<int32_t>();
  Q.uttNBeam = d->uttNBeam.as<int32_t>();
  Q.uttFrame = d->uttFrame.as<int32_t>();
  Q.uttTotal = d->uttTotal.as<int32_t>();
  Q.uttStatus = d->uttStatus.as<int32_t>();
  Q.snap = d->snap.as<char>();
  Q.B = d->B;
  if (n <= 0) {
    return FLTX_OK;
  }
#ifdef FLTX_EMU
  for (int i = 0; i < n; ++i) {
    snapUtterance(Q, map ? map[i] : i, 0, 1);
  }
#else
  hipLaunchKernelGGL(fltx_snapshot_kernel, dim3(n), dim3(64), 0, d->ctx->stream, Q);
  HIPCHK(hipGetLastError());
#endif
  return FLTX_OK;
}

/* after an optimistic stream chunk: the streams whose chunk overflowed a candidate list (or whose cut left
 * fewer than K groups) get their beam back and decode the chunk again on the general path */
int streamRedoFlagged(fltx_decoder* d) {
  d->resultsSynced = false;
  int rc = FLTX_OK;
  /* the chunk's kernel left every stream's status in pinned host memory: wait for the kernel, nothing to copy */
  if (devSync(d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "stream synchronize failed: %s", devErr());
  }
  const int32_t* status = (const int32_t*)d->hStat.p;
  std::vector<int32_t> again;
  for (int b = 0; b < d->B; ++b) {
    if (status[b] & (ST_CAND_OVERFLOW | ST_CUT_RETRY)) {
      again.push_back(b);
    }
  }
  d->resultsSynced = false;
  if (again.empty()) {
    return FLTX_OK;
  }
  Stream st = d->ctx->stream;
  if (d->uttMap.ensure(4 * again.size(), st, false) ||
      devCopyH2D(d->uttMap.p, again.data(), 4 * again.size(), st) || devSync(st)) {
    return fail(FLTX_ERR_OOM, "re-run list upload failed");
  }
  if ((rc = streamSnapshot(d, 1, d->uttMap.as<int32_t>(), (int)again.size()))) {
    return rc;
  }
  const int savedWs = d->forceGlobalWs, savedCut = d->noCut;
  std::vector<int32_t> Tm(d->B, d->maxFrames);
  d->forceGlobalWs = 1;
  d->noCut = 1;
  d->keepScored = true;
  rc = prepare(d, d->B, d->N, Tm.data(), true);
  if (!rc) {
    DecodeParams P;
    fillParams(d, P);
    P.emissions = d->lastEmis;
    P.doBegin = 0;
    P.doEnd = 0;
    P.uttMap = d->uttMap.as<int32_t>();
    d->nLaunch = (int)again.size();
    rc = launchDecode(d, P);
    d->nLaunch = 0;
  }
  d->forceGlobalWs = savedWs;
  d->noCut = savedCut;
  if (!rc) {
    rc = prepare(d, d->B, d->N, Tm.data(), false); /* back to the optimistic geometry for the next chunk */
  }
  d->keepScored = false;
  d->streamRedone += (int)again.size();
  return rc;
}

int launchStreamOp(fltx_decoder* d, int op, int lookBack, int cap) {
  StreamOpParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.K = d->opt.beam_size;
  Q.kind = d->kind;
  Q.op = op;
  Q.lookBack = lookBack;
  Q.histPT = d->histPT.as<int2>();
  Q.histW = d->histW.as<int32_t>();
  Q.histS = d->keepScores ? d->histS.as<double>() : nullptr;
  Q.histOff = d->histOffD.as<int64_t>();
  Q.uttFrame = d->uttFrame.as<int32_t>();
  Q.uttNBeam = d->uttNBeam.as<int32_t>();
  Q.gScore = d->gScore.as<double>();
  Q.firstFrame = d->streaming ? d->uttFirst.as<int64_t>() : nullptr;
  Q.outLen = d->bestLen.as<int32_t>();
  Q.outScores = d->bestScores.as<double>();
  Q.outTok = d->bestTok.as<int32_t>();
  Q.outWrd = d->bestWrd.as<int32_t>();
  Q.cap = cap;
#ifdef FLTX_EMU
  const StreamOpParams* qq = &Q;
  emuLaunch(d->B, 256, kStreamOpLds, [qq](char* sm) { streamOpUtterance(*qq, (int32_t*)sm); });
#else
  /* (sixteen waves: they stage the rows the ancestor walk visits, and prune moves up to lookBack + 101 history rows
   * -- a thread's loads and stores follow each other, so the fewer rounds the better) */
  hipLaunchKernelGGL(fltx_streamop_kernel, dim3(d->B), dim3(1024), 0, d->ctx->stream, Q);
  HIPCHK(hipGetLastError());
#endif
  return FLTX_OK;
}

/* the look at the chunk left pending by fltx_stream_step (decode it again where a list overflowed), then the prune that
 * was asked for meanwhile */
int settleStream(fltx_decoder* d) {
  int rc = FLTX_OK;
  struct Scope {
    bool& flag;
    ~Scope() { flag = false; }
  } scope{d->settling};
  d->settling = true;
  if (d->chunkPending) {
    d->chunkPending = false;
    const float* curEmis = d->lastEmis;
    const int curSlot = d->upSlot;
    d->lastEmis = d->pendEmis; /* (the next chunk may be uploaded already: the other slot) */
    d->upSlot = d->pendSlot;
    const int before = d->streamRedone;
    rc = streamRedoFlagged(d);
#ifndef FLTX_EMU
    if (!rc && d->streamRedone != before && d->copyStream) {
      HIPCHK(hipEventRecord(d->evSlotFree[d->pendSlot], d->ctx->stream)); /* the second pass read the slot too */
    }
#endif
    d->lastEmis = curEmis;
    d->upSlot = curSlot;
  }
  if (!rc && d->pendingPrune >= 0) {
    const int lb = d->pendingPrune;
    d->pendingPrune = -1;
    rc = launchStreamOp(d, 1, lb, 0);
    d->resultsSynced = false;
  }
  return rc;
}

/* streams: mode 0 = a new stream, mode 1 = renumber the LM-state ids the beam can still meet to the front.  Runs on the launch
 * stream between two decode launches; nothing is waited for. */
int launchCompact(fltx_decoder* d, int mode) {
  if (!d->recycle) {
    return FLTX_OK;
  }
  int rc;
  if (mode == 1 && d->idFamily == 1 && (rc = bumpEpoch(d))) { /* (the rebuilt table's epoch; empties the LM score cache too) */
    return rc;
  }
  CompactParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.K = d->opt.beam_size;
  Q.N = d->N;
  Q.mode = mode;
  Q.family = d->idFamily;
  Q.idCap = d->idCap;
  Q.uttNBeam = d->uttNBeam.as<int32_t>();
  Q.gState = d->gState.as<uint32_t>();
  Q.gSPar = d->gSPar.as<uint32_t>();
  Q.uttNextId = d->uttNextId.as<int32_t>();
  Q.newId = d->idNew.as<uint32_t>();
  Q.list = d->idList.as<uint32_t>();
  if (d->lm->kind == 1 && d->idFamily == 1) {
    Q.stateCtx = d->stateCtx.as<int32_t>();
    Q.ctxL = std::max(1, d->lm->order - 1);
  }
  Q.idPar = d->idPar.as<uint32_t>();
  Q.idEdge = d->idEdge.as<int32_t>();
  Q.idBorn = d->idBorn.as<uint32_t>();
  Q.keep = d->idKeep.as<uint8_t>();
  Q.childTab = d->childTab.as<uint32_t>();
  Q.maskTab = d->maskTab.as<unsigned long long>();
  Q.gMask = d->gMask.as<unsigned long long>();
  Q.stateTab = d->stateTab.as<unsigned long long>();
  Q.stateVal = d->stateVal.as<uint32_t>();
  Q.stateCap = d->stateCap;
  Q.epoch = d->epoch;
#ifdef FLTX_EMU
  const CompactParams* qq = &Q;
  emuLaunch(d->B, 64, kCompactLds, [qq](char* sm) { compactStates(*qq, sm); });
#else
  HIPCHK(hipFuncSetAttribute((const void*)fltx_compact_states_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             kCompactLds));
  hipLaunchKernelGGL(fltx_compact_states_kernel, dim3(d->B), dim3(1024), kCompactLds, d->ctx->stream, Q);
  HIPCHK(hipGetLastError());
#endif
  d->idsUsedBound = mode == 0 ? 1 : 0;
  d->compactions += mode;
  return FLTX_OK;
}

/* ---- host LM (fltx_lm_host_create): one frame per launch, the frame's LM questions answered on the host ------- */
int hostLmEnsure(fltx_decoder* d) {
  const int64_t K = d->opt.beam_size, N = d->N, B = d->B;
  const int64_t nTok = std::min<int64_t>(d->opt.beam_size_token, N);
  /* what a frame can ask: one question per (hypothesis, token); the lexicon decoder with a word LM one per word a
   * child ends (<= 6, Trie.h:19) or the unknown word; decodeEnd one per hypothesis */
  int64_t cap = K * nTok * ((d->kind == FLTX_DECODER_LEXICON && !d->isLmToken) ? 6 : 1);
  cap = std::max<int64_t>(cap, K);
  if (cap * B * 8 > (1ll << 32)) {
    return fail(FLTX_ERR_UNSUPPORTED, "host LM: %lld questions per frame x %lld utterances exceed the question buffer",
                (long long)cap, (long long)B);
  }
  d->hlmQCap = (int)cap;
  if (d->hlmQCount.ensure(4 * (size_t)B) || d->hlmQ.ensure(8 * (size_t)B * (size_t)cap) ||
      d->hlmBeamN.ensure(4 * (size_t)B) || d->hlmBeam.ensure(4 * (size_t)B * (size_t)K)) {
    return fail(FLTX_ERR_OOM, "host LM: pinned buffers");
  }
  return FLTX_OK;
}

int hostLmCall(int rc, const char* what) {
  return rc ? fail(FLTX_ERR_CALLBACK, "host LM: the %s callback reported failure (%d)", what, rc) : FLTX_OK;
}

/* list the questions of frame `frame` of the chunk (or of decodeEnd), have the user's LM answer each distinct one
 * and leave the answers where the frame's launch finds them (P.hlmTab / P.hlmDir) */
int hostLmExchange(fltx_decoder* d, DecodeParams& P, int frame, bool end) {
  Stream st = d->ctx->stream;
  const int B = d->B, K = d->opt.beam_size;
  const fltx_host_lm& cb = d->lm->host;
  P.hlmFrame = frame;
  P.hlmEnd = end ? 1 : 0;
  const size_t qLds = 4 * (size_t)(std::min(d->opt.beam_size_token, d->N) + 4);
#ifdef FLTX_EMU
  {
    const DecodeParams* pp = &P;
    emuLaunch(B, 64, qLds, [pp](char* smem) { hostLmQuestions(*pp, smem); }); /* (one wave: host threads are expensive) */
  }
#else
  HIPCHK(hipFuncSetAttribute((const void*)fltx_hostlm_questions_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)qLds));
  hipLaunchKernelGGL(fltx_hostlm_questions_kernel, dim3(B), dim3(256), qLds, st, P);
  HIPCHK(hipGetLastError());
#endif
  if (devSync(st)) { /* (also: the previous frame's table upload has been consumed, the staging buffer is free) */
    return fail(FLTX_ERR_HIP, "host LM: questions kernel failed: %s", devErr());
  }
  const int32_t* qCount = (const int32_t*)d->hlmQCount.p;
  const uint2* q = (const uint2*)d->hlmQ.p;
  const int32_t* beamN = (const int32_t*)d->hlmBeamN.p;
  const int32_t* beam = (const int32_t*)d->hlmBeam.p;
  int rc;
  if (d->hlmAnnounce && cb.update_cache) { /* updateLMCache(lm_, hyp_[t + 1]) of the frame before (Utils.h:346-354) */
    for (int b = 0; b < B; ++b) {
      if (beamN[b] > 0 && (rc = hostLmCall(cb.update_cache(cb.user, b, beamN[b], beam + (size_t)b * K), "update_cache"))) {
        return rc;
      }
    }
  }
  /* one open-addressing table per utterance, at most half full; the tables double as the set of distinct questions */
  std::vector<uint2> dir((size_t)B);
  size_t slots = 0;
  for (int b = 0; b < B; ++b) {
    if (qCount[b] > d->hlmQCap) {
      return fail(FLTX_ERR_UNSUPPORTED, "host LM: utterance %d asked %d questions in one frame (capacity %d)", b, qCount[b],
                  d->hlmQCap);
    }
    const uint32_t n = nextPow2(std::max<uint64_t>(2ull * (uint64_t)qCount[b], 2));
    dir[(size_t)b] = make_uint2((uint32_t)slots, n - 1u);
    slots += n;
  }
  const size_t dirBytes = alignUp(sizeof(uint2) * (size_t)B, 16);
  const size_t bytes = dirBytes + 16 * slots;
  if (d->hlmStage.ensure(bytes) || d->hlmTabD.ensure(bytes, st, false)) {
    return fail(FLTX_ERR_OOM, "host LM: answer table");
  }
  char* stage = (char*)d->hlmStage.p;
  memcpy(stage, dir.data(), sizeof(uint2) * (size_t)B);
  uint4* tab = (uint4*)(stage + dirBytes);
  memset(tab, 0xFF, 16 * slots);
  std::vector<int32_t> qu, qs, qi, os;
  std::vector<float> of;
  std::vector<size_t> where;
  for (int b = 0; b < B; ++b) {
    const uint2 dd = dir[(size_t)b];
    const uint2* qb = q + (size_t)b * d->hlmQCap;
    d->hlmAsked += qCount[b];
    for (int i = 0; i < qCount[b]; ++i) {
      const uint32_t sid = qb[i].x, idx = qb[i].y;
      uint32_t s = hashKey(sid, idx, 0x7f4a7c15u, 0) & dd.y;
      for (;;) {
        uint4& e = tab[(size_t)dd.x + s];
        if (e.x == sid && e.y == idx) {
          break;
        }
        if (e.x == kEmpty && e.y == kEmpty) {
          e.x = sid;
          e.y = idx;
          qu.push_back(b);
          qs.push_back((int32_t)sid);
          qi.push_back((int32_t)idx);
          where.push_back((size_t)dd.x + s);
          break;
        }
        s = (s + 1) & dd.y;
      }
    }
  }
  const size_t nq = qu.size();
  d->hlmDistinct += (int64_t)nq;
  if (nq > 0) {
    os.assign(nq, 0);
    of.assign(nq, 0.0f);
    if ((rc = hostLmCall(cb.score(cb.user, (int32_t)nq, qu.data(), qs.data(), qi.data(), os.data(), of.data()), "score"))) {
      return rc;
    }
    for (size_t i = 0; i < nq; ++i) {
      uint32_t bits;
      memcpy(&bits, &of[i], 4);
      tab[where[i]].z = (uint32_t)os[i];
      tab[where[i]].w = bits;
    }
  }
  if (devCopyH2D(d->hlmTabD.p, stage, bytes, st)) {
    return fail(FLTX_ERR_HIP, "host LM: answer upload failed");
  }
  P.hlmDir = (const uint2*)d->hlmTabD.p;
  P.hlmTab = (const uint4*)((const char*)d->hlmTabD.p + dirBytes);
  return FLTX_OK;
}

/* the frames of one chunk (T[b] frames of utterance b), a launch each */
int hostLmFrames(fltx_decoder* d, DecodeParams& P, const int32_t* T) {
  int maxT = 0;
  for (int b = 0; b < d->B; ++b) {
    maxT = std::max(maxT, T[b]);
  }
  P.doBegin = 0;
  P.doEnd = 0;
  for (int t = 0; t < maxT; ++t) {
    int rc = hostLmExchange(d, P, t, false);
    if (rc || (rc = launchDecode(d, P))) {
      return rc;
    }
    d->hlmAnnounce = true;
  }
  return FLTX_OK;
}

/* decodeBegin on the device (the seed hypothesis in LM state 0) and LM::start on the host */
int hostLmBegin(fltx_decoder* d, DecodeParams& P) {
  int rc = hostLmEnsure(d);
  if (rc) {
    return rc;
  }
  fillParams(d, P); /* (the question buffers exist now) */
  d->hlmAnnounce = false;
  d->hlmAsked = 0;
  d->hlmDistinct = 0;
  return hostLmCall(d->lm->host.start(d->lm->host.user, d->B), "start");
}

/* Decoder::prune: the LM states the beam still holds (the callee may release the others) */
int hostLmRetain(fltx_decoder* d) {
  const fltx_host_lm& cb = d->lm->host;
  if (!cb.retain) {
    return FLTX_OK;
  }
  const int B = d->B, K = d->opt.beam_size;
  std::vector<int32_t> nb((size_t)B), st((size_t)B * K);
  if (devCopyD2H(nb.data(), d->uttNBeam.p, 4 * (size_t)B, d->ctx->stream) ||
      devCopyD2H(st.data(), d->gState.p, 4 * (size_t)B * K, d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "host LM: beam copy failed");
  }
  for (int b = 0; b < B; ++b) {
    int rc = hostLmCall(cb.retain(cb.user, b, nb[(size_t)b], st.data() + (size_t)b * K), "retain");
    if (rc) {
      return rc;
    }
  }
  return FLTX_OK;
}

/* fltx_decode_batch with a host LM: begin, a launch per frame, end, back-trace */
int hostLmDecodeBatch(fltx_decoder* d, const float* emissions, int32_t onDevice, const int64_t* offsets, const int32_t* T,
                      int32_t B, int32_t N) {
  d->offlineCall = true;
  d->batchPacked = false;
  d->batchWlane = false;
  d->batchTlane = false;
  d->keepScores = d->userKeepScores;
  d->fallbackReasons = 0;
  int rc = prepare(d, B, N, T, true);
  if (rc) {
    return rc;
  }
  latchFirst(d);
  if ((rc = bumpEpoch(d))) {
    return rc;
  }
  DecodeParams P;
  fillParams(d, P);
  if ((rc = hostLmBegin(d, P)) || (rc = uploadStep(d, emissions, onDevice, offsets, T, P))) {
    return rc;
  }
  d->nLaunch = 0;
  P.doBegin = 1;
  P.doEnd = 0;
  P.hlmFrame = 1 << 30; /* (no frame in this launch: decodeBegin only) */
  if ((rc = launchDecode(d, P)) || (rc = hostLmFrames(d, P, T))) {
    return rc;
  }
  if ((rc = hostLmExchange(d, P, 1 << 30, true))) {
    return rc;
  }
  P.doBegin = 0;
  P.doEnd = 1;
  P.hlmFrame = 1 << 30;
  if ((rc = launchDecode(d, P))) {
    return rc;
  }
  d->lastRedo = 0;
  d->resultsSynced = false;
  if ((rc = launchBacktrace(d))) {
    return rc;
  }
  d->T.assign(T, T + B);
  d->statsDone = false;
  d->haveResults = true;
  d->ended = true;
  return FLTX_OK;
}

} // namespace

extern "C" {

int fltx_decode_batch(fltx_decoder* d, const float* emissions, int32_t onDevice, const int64_t* offsets,
                      const int32_t* T, int32_t B, int32_t N) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (d && stepKindCalls(d->kind)) {
    return fail(FLTX_ERR_STATE, "fltx_decode_batch: %s", stepKindCalls(d->kind));
  }
  if (!d || !T || B <= 0 || N <= 0) {
    return fail(FLTX_ERR_INVALID, "fltx_decode_batch: bad argument");
  }
  if (d->offlinePending) {
    /* "defer_check": the batch before this one was never read.  Its statuses are looked at all the same (and what the
     * fast path flagged is decoded again: that is how a decoder learns that a fallback should stick) -- a caller who
     * only wants kernels queued back to back asks for defer_check = 2 and gets the drops counted */
    if (d->deferCheck == 2) {
      d->offlinePending = false;
      d->lookQueued = false;
      ++d->looksDropped;
    } else {
      int rc = syncResults(d);
      if (rc) {
        return rc;
      }
      d->unreadRedone += d->lastRedo;
    }
  }
  d->streaming = false;
  d->chunkPending = false;
  d->pendingPrune = -1;
  d->haveResults = false;
  d->resultsSynced = false;
  d->backtraced = false;
  d->hostFetched = false;
  d->compactFetched = false;
  d->scoresFetched = false;
  if (d->lm->kind == 2) {
    return hostLmDecodeBatch(d, emissions, onDevice, offsets, T, B, N);
  }
  d->offT.assign(T, T + B);
  d->offOffsets.clear();
  if (offsets) {
    d->offOffsets.assign(offsets, offsets + B);
  }
  d->offN = N;
  d->offlinePending = false;
  return offlineAttempts(d, emissions, onDevice, 0);
}

/* The attempts of one offline batch.  firstAttempt 0: the call itself (the fast path); 1: the look at a batch whose
 * status scan was deferred (fltx_decoder_set "defer_check"): the decode kernel and the back-trace were launched and
 * the call returned -- the scan, and the second pass of whatever the fast path flagged, happen when the results are
 * first asked for (syncResults), on the emissions where the first pass left them in HBM. */
} /* extern "C" */
static int settlePendingLook(fltx_decoder* d) { return syncResults(d); }
/* "defer_check" left the batch pending: the copy of its status rows (what syncResults brings home) and an event are
 * queued on the launch stream right behind the back-trace, so that the settle finds them in the pinned rows and waits
 * for that event only.  The rows are the decoder object's own and nothing else writes them before the settle. */
static int queueLook(fltx_decoder* d) {
#ifndef FLTX_EMU
  const size_t bytes = 4 * (2 * d->uttRow + (size_t)d->B);
  if (d->hSync.ensure(bytes)) {
    return fail(FLTX_ERR_OOM, "pinned staging allocation failed");
  }
  if (!d->lookEv) {
    HIPCHK(hipEventCreateWithFlags(&d->lookEv, hipEventDisableTiming));
  }
  HIPCHK(hipMemcpyAsync(d->hSync.p, d->uttRes.p, bytes, hipMemcpyDeviceToHost, d->ctx->stream));
  HIPCHK(hipEventRecord(d->lookEv, d->ctx->stream));
  d->lookQueued = true;
#else
  (void)d; /* (the emulator's kernels have run when the launch returns: the settle copies as before) */
#endif
  return FLTX_OK;
}
static int offlineAttempts(fltx_decoder* d, const float* emissions, int32_t onDevice, int firstAttempt) {
  const int32_t* T = d->offT.data();
  const int64_t* offsets = d->offOffsets.empty() ? nullptr : d->offOffsets.data();
  const int32_t B = (int32_t)d->offT.size(), N = d->offN;
  /* The optimistic fast paths (LDS-sized candidate lists of the lexicon
   * decoder, the score cut, the one-pass histogram select of the lean / lane
   * steps) flag the rare utterance they cannot serve.  Only those utterances
   * are decoded again, on the general path (HBM workspace / no cut / generic
   * engine); the others keep their results.  The fallback sticks to the decoder
   * only when a large part of the batch needed it. */
  std::vector<int32_t> redoList;
  size_t firstRedo = 0;
  if (firstAttempt == 0) {
    d->fallbackReasons = 0;
  }
  bool recomputeRetry = false; /* this attempt is the recompute form of the cut-off generation */
  bool recomputeTried = false;
  const int savedGlobalWs = d->forceGlobalWs, savedNoCut = d->noCut, savedNoLean = d->noLean, savedNoSlim = d->noSlim;
  const int savedNoSlane = d->noSlane, savedNoXlane = d->noXlane, savedNoYlane = d->noYlane, savedNoWlane = d->noWlane;
  d->offlineCall = true;
  if (firstAttempt == 0) {
    d->batchPacked = false;
    d->batchWlane = false;
    d->batchTlane = false;
  }
  d->keepScores = d->userKeepScores; /* a stream on this decoder had switched the score history on */
  for (int attempt = firstAttempt; attempt < 3 + firstAttempt; ++attempt) {
    const bool finalForm = attempt > firstAttempt && !recomputeRetry; /* the general path: nothing left to fall back to */
    const bool look = firstAttempt > 0 && attempt == firstAttempt; /* the deferred look at what is already decoded */
    int rc;
    if (!look) {
      d->keepScored = attempt > 0;
      rc = prepare(d, B, N, T, finalForm);
      d->keepScored = false;
      if (rc) {
        return rc;
      }
    }
    if (!look && attempt > 0 && d->lm->kind == 1 && d->scored.p) {
      for (int32_t b : redoList) { /* only the utterances decoded again start their query count over */
        devMemset(d->scored.as<uint32_t>() + b, 0, 4, d->ctx->stream);
      }
    }
    if (!look) {
    d->batchPacked = d->batchPacked || d->slane || d->xlane || d->ylane;
    d->batchTlane = d->batchTlane || d->tlane != 0;
    if (d->slane || d->xlane || d->ylane) {
      d->packedBits = (d->slane && d->mlaneNG > 1) ? 10 : (d->ylane == 4 ? 13 : 8); /* (a re-run on a general engine leaves plain records) */
      d->batchWlane = d->wlane != 0; /* ... and so is the records' token width (the back-trace reads it, not d->wlane) */
    }
    if (attempt == 0) {
      latchFirst(d);
    }
    if ((rc = bumpEpoch(d))) {
      return rc;
    }
    DecodeParams P;
    fillParams(d, P);
    if ((rc = uploadStep(d, emissions, onDevice, offsets, T, P))) {
      return rc;
    }
    P.doBegin = 1;
    P.doEnd = 1;
    d->nLaunch = 0;
    if (attempt > 0) {
      if (d->uttMap.ensure(4 * redoList.size(), d->ctx->stream, false) ||
          devCopyH2D(d->uttMap.p, redoList.data(), 4 * redoList.size(), d->ctx->stream)) {
        return fail(FLTX_ERR_OOM, "re-run list upload failed");
      }
      P.uttMap = d->uttMap.as<int32_t>();
      d->nLaunch = (int)redoList.size();
    }
    rc = launchDecode(d, P);
    d->nLaunch = 0;
    if (rc) {
      return rc;
    }
    } /* !look */
    const bool cutMode = d->CAP2 > 0 || d->cutRecompute;
    const bool needLook = !finalForm && ((d->kind == FLTX_DECODER_LEXICON && (d->wsInLds || cutMode)) || d->lean || d->wlane || d->xlane || d->ylane || d->tlane);
    if (needLook && attempt == 0 && d->deferCheck) {
      /* the caller keeps the emissions where they are until the results are read: launch the back-trace and return;
       * the look happens in syncResults() */
      d->offlinePending = true;
      d->offEmis = d->lastEmis;
      d->offUpSlot = d->upSlot;
      break;
    }
    if (needLook) {
      d->resultsSynced = false;
      d->offlinePending = false; /* (syncResults below must not come back here) */
      if ((rc = syncResults(d))) {
        return rc;
      }
      bool ws = false, cut = false, lean = false, slaneMiss = false, xlaneMiss = false, wlaneMiss = false;
      const bool slimMode = d->CAP2 > 0;
      std::vector<int32_t> again;
      const bool firstScan = attempt == 0 || look;
      const int nScan = firstScan ? B : (int)redoList.size();
      for (int i = 0; i < nScan; ++i) {
        const int b = firstScan ? i : redoList[i];
        const int st = d->hStatus[b];
        if (firstScan && (st & ST_SELECT_FALLBACK)) {
          d->fallbackReasons |= 1ll << ((st >> 8) & 31); /* (the lexicon lane engine says why: fltx_ylane.h) */
        }
        const bool o = (st & ST_CAND_OVERFLOW) && d->kind == FLTX_DECODER_LEXICON;
        const bool c = (st & ST_CUT_RETRY) && cutMode;
        const bool l = (st & ST_SELECT_FALLBACK) && (d->lean || d->tlane);
        const bool x = (st & ST_SELECT_FALLBACK) && (d->xlane || d->ylane);
        const bool wl = (st & ST_SELECT_FALLBACK) && d->wlane; /* fltx_wlane.h: a row without a defined token beam, a select that did not converge */
        if (o || c || l || x || wl) {
          again.push_back(b);
          ws |= o;
          cut |= c;
          lean |= l;
          slaneMiss |= l && d->slane;
          xlaneMiss |= x;
          wlaneMiss |= wl;
        }
      }
      redoList.swap(again);
      if (firstScan) {
        firstRedo = redoList.size();
      }
      if (!redoList.empty()) {
        recomputeRetry = false;
        if (ws && slimMode && !cut && !recomputeTried) { /* the slim list overflowed: generate twice instead */
          d->noSlim = 1;
          ws = false;
          recomputeRetry = true;
          recomputeTried = true;
        } else if (!d->wsInLds && cutMode) { /* HBM workspace with the cut: the plain HBM path is what is left */
          ws = true;
          cut = true;
        }
        d->forceGlobalWs = ws ? 1 : d->forceGlobalWs;
        d->noCut = cut ? 1 : d->noCut;
        d->noLean = lean ? 1 : d->noLean;
        d->noSlane = slaneMiss ? 1 : d->noSlane; /* (re-run on the generic engine) */
        d->noWlane = wlaneMiss ? 1 : d->noWlane;
        d->noXlane = xlaneMiss ? 1 : d->noXlane;
        d->noYlane = xlaneMiss ? 1 : d->noYlane;
        d->resultsSynced = false;
        continue;
      }
    }
    break;
  }
  if (!d->offlinePending) {
    d->lastRedo = (int)firstRedo;
  }
  if (firstAttempt > 0 && firstRedo == 0) {
    return FLTX_OK; /* the deferred look found nothing to decode again: the back-trace already ran */
  }
  if (firstRedo > 0 && firstRedo * 4 <= (size_t)B) { /* a few outliers: next batch tries the fast path again */
    d->forceGlobalWs = savedGlobalWs;
    d->noCut = savedNoCut;
    d->noLean = savedNoLean;
    d->noSlim = savedNoSlim;
    d->noSlane = savedNoSlane;
    d->noWlane = savedNoWlane;
    d->noXlane = savedNoXlane;
    d->noYlane = savedNoYlane;
  }
  d->resultsSynced = false;
  int rc = launchBacktrace(d);
  if (rc) {
    return rc;
  }
  d->lookQueued = false;
  if (d->offlinePending && (rc = queueLook(d))) {
    return rc;
  }
  d->T.assign(T, T + B);
  d->statsDone = false;
  d->haveResults = true;
  d->ended = true;
  return FLTX_OK;
}
extern "C" {

int fltx_stream_begin(fltx_decoder* d, int32_t B, int32_t N, int32_t maxFrames) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (d && stepKindCalls(d->kind)) {
    return fail(FLTX_ERR_STATE, "fltx_stream_begin: %s", stepKindCalls(d->kind));
  }
  if (!d || B <= 0 || N <= 0 || maxFrames < 0) {
    return fail(FLTX_ERR_INVALID, "fltx_stream_begin: bad argument");
  }
  /* prune(lookBack) of the lexicon decoder walks on from lookBack frames back to the last COMPLETE hypothesis (its parent
   * ended a word), up to kLookBackLimit frames further (Utils.h:28,293-308): that many frames can stay in the buffer
   * whatever the caller prunes.  The reference's buffer grows as needed; here the stream's buffer is sized when it
   * begins, so a lexicon stream gets those kLookBackLimit frames ON TOP of max_frames: a caller whose own count (lookBack
   * frames left after a prune, plus the chunks since) stays within max_frames never fills it (round 5 raised
   * "exceed max_frames" in the middle of such a stream) */
  if (d->kind == FLTX_DECODER_LEXICON) {
    maxFrames += kLookBackLimit;
  }
  std::vector<int32_t> Tm(B, maxFrames);
  d->offlineCall = false;
  d->offlinePending = false; /* (an offline batch whose results were never read) */
  d->lookQueued = false;
  d->batchPacked = false;
  d->keepScores = 1; /* streams serve getBestHypothesis(lookBack) of ancestors */
  /* The lexicon decoder's candidate lists are sized for what a frame usually produces (LDS) when a chunk
   * can be decoded again: the beam a chunk starts from is saved, the state table is idempotent (same
   * (parent, edge) -> same id), history rows are rewritten in place.  (The lexicon-free engines never
   * overflow and number their states with a counter: always one pass.) */
  d->streamOpt = d->kind == FLTX_DECODER_LEXICON && d->userStreamOpt != 0 && !d->forceGlobalWs && d->lm->kind != 2;
  d->streamRedone = 0;
  int rc = prepare(d, B, N, Tm.data(), !d->streamOpt);
  if (rc) {
    return rc;
  }
  if (d->streamOpt && (d->lean || !(d->wsInLds || d->CAP2 > 0 || d->cutRecompute))) {
    d->streamOpt = false; /* nothing optimistic came out of it */
    if ((rc = prepare(d, B, N, Tm.data(), true))) {
      return rc;
    }
  }
  if (d->streamOpt &&
      d->snap.ensure((size_t)B * d->opt.beam_size * (3 * 8 + 6 * 4) + (size_t)B * 16, d->ctx->stream, false)) {
    return fail(FLTX_ERR_OOM, "stream snapshot allocation failed");
  }
  if (d->streamOpt && d->hStat.ensure(4 * (size_t)B)) {
    return fail(FLTX_ERR_OOM, "pinned status allocation failed");
  }
  latchFirst(d);
  if ((rc = bumpEpoch(d))) {
    return rc;
  }
  d->maxFrames = maxFrames;
  d->streaming = true;
  d->ended = false;
  d->haveResults = false;
  d->resultsSynced = false;
  d->backtraced = false;
  d->hostFetched = false;
  d->compactFetched = false;
  d->scoresFetched = false;
  d->frames.assign(B, 0);
  d->framesExact = true;
  d->chunkPending = false;
  d->pendingPrune = -1;
  d->compactions = 0;
  if (d->uttFirst.ensure(8 * (size_t)B, d->ctx->stream, false) || devMemset(d->uttFirst.p, 0, 8 * (size_t)B, d->ctx->stream)) {
    return fail(FLTX_ERR_OOM, "stream counters: allocation failed");
  }
  if ((rc = launchCompact(d, 0))) {
    return rc;
  }
  DecodeParams P;
  fillParams(d, P);
  if (d->lm->kind == 2 && (rc = hostLmBegin(d, P))) {
    return rc;
  }
  std::vector<int32_t> zeroT(B, 0);
  if ((rc = uploadStep(d, nullptr, 1, nullptr, zeroT.data(), P))) {
    return rc;
  }
  P.doBegin = 1;
  P.doEnd = 0;
  P.hlmFrame = 1 << 30;
  if ((rc = launchDecode(d, P))) {
    return rc;
  }
  d->haveResults = true;
  return FLTX_OK;
}

int fltx_stream_step(fltx_decoder* d, const float* emissions, int32_t onDevice, const int64_t* offsets,
                     const int32_t* T) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (d && stepKindCalls(d->kind)) {
    return fail(FLTX_ERR_STATE, "fltx_stream_step: %s", stepKindCalls(d->kind));
  }
  if (!d || !T) {
    return fail(FLTX_ERR_INVALID, "fltx_stream_step: bad argument");
  }
  if (!d->streaming || d->ended) {
    return fail(FLTX_ERR_STATE, "fltx_stream_step: call fltx_stream_begin first");
  }
  for (int pass = 0; pass < 2; ++pass) {
    int bad = -1;
    for (int b = 0; b < d->B && bad < 0; ++b) {
      if (T[b] < 0 || d->frames[b] + T[b] > d->maxFrames) {
        bad = b;
      }
    }
    if (bad < 0) {
      break;
    }
    if (pass == 0 && !d->framesExact && T[bad] >= 0) {
      int rcs = syncResults(d); /* what the prunes since the last look really left in the buffers */
      if (rcs) {
        return rcs;
      }
      for (int b = 0; b < d->B; ++b) {
        d->frames[b] = d->hFrame[b];
      }
      d->framesExact = true;
      continue;
    }
    return fail(FLTX_ERR_RANGE, "stream %d: %d buffered + %d new frames exceed max_frames %d%s", bad, d->frames[bad],
                T[bad], d->maxFrames,
                d->kind == FLTX_DECODER_LEXICON
                    ? " (a lexicon stream's prune keeps the frames back to the last complete word, up to lookBack + 100: "
                      "size the buffer for 100 + lookBack + the largest chunk, Utils.h:28,293-308)"
                    : "");
  }
  /* the chunk's upload first (copy stream: under the kernel of the chunk before, if that one is still pending), then
   * the look at the chunk before, then this chunk's launch */
  DecodeParams up;
  memset(&up, 0, sizeof(up));
  int rc = uploadStep(d, emissions, onDevice, offsets, T, up);
  if (rc) {
    return rc;
  }
  if ((rc = settleStream(d))) {
    return rc;
  }
  if (d->recycle) {
    /* a frame makes at most beam new LM states per stream: when this chunk could run a stream out of ids, the ids
     * nothing can meet again are given back first (beam x max_frames ids are free after that, or the chunk's status
     * says the table is full) */
    int maxT = 0;
    for (int b = 0; b < d->B; ++b) {
      maxT = std::max(maxT, T[b]);
    }
    const int64_t want = (int64_t)d->opt.beam_size * maxT * (d->streamOpt ? 2 : 1); /* (a chunk decoded again may name states twice) */
    const int64_t room = (d->compactions ? d->idsFreeBound : d->idCap) - d->idsUsedBound;
    if ((want > room || d->userCompactAlways) && (rc = launchCompact(d, 1))) {
      return rc;
    }
    d->idsUsedBound += want;
  }
  DecodeParams P;
  fillParams(d, P); /* (emOff / stepT: the slot uploadStep has just filled) */
  P.emissions = up.emissions;
  P.doBegin = 0;
  P.doEnd = 0;
  if (d->streamOpt && (rc = streamSnapshot(d, 0, nullptr, d->B))) {
    return rc;
  }
  d->sstreamLaunch = d->sstream != 0;
  rc = d->lm->kind == 2 ? hostLmFrames(d, P, T) : launchDecode(d, P);
  d->sstreamLaunch = false;
  if (rc) {
    return rc;
  }
  if (d->streamOpt) {
    d->chunkPending = true;
    d->pendEmis = P.emissions;
    d->pendSlot = d->upSlot;
    /* A chunk handed over as a device pointer is the caller's buffer: a second pass deferred to the next call would
     * read whatever the caller has put there since (one buffer reused chunk after chunk is legal).  Such a chunk is
     * settled before the call returns; host chunks live in this decoder's own staging slots and may wait. */
    if ((!d->deferRedo || onDevice) && (rc = settleStream(d))) {
      return rc;
    }
  }
  for (int b = 0; b < d->B; ++b) {
    d->frames[b] += T[b];
  }
  d->resultsSynced = false;
  d->backtraced = false;
  d->hostFetched = false;
  d->compactFetched = false;
  d->scoresFetched = false;
  return FLTX_OK;
}

int fltx_stream_end(fltx_decoder* d) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (d && stepKindCalls(d->kind)) {
    return fail(FLTX_ERR_STATE, "fltx_stream_end: %s", stepKindCalls(d->kind));
  }
  if (!d) {
    return fail(FLTX_ERR_INVALID, "null decoder");
  }
  if (!d->streaming || d->ended) {
    return fail(FLTX_ERR_STATE, "fltx_stream_end: no open stream");
  }
  int rc = settleStream(d);
  if (rc) {
    return rc;
  }
  DecodeParams P;
  fillParams(d, P);
  std::vector<int32_t> zeroT(d->B, 0);
  if ((rc = uploadStep(d, nullptr, 1, nullptr, zeroT.data(), P))) {
    return rc;
  }
  if (d->lm->kind == 2 && (rc = hostLmExchange(d, P, 1 << 30, true))) {
    return rc;
  }
  P.doBegin = 0;
  P.doEnd = 1;
  P.hlmFrame = 1 << 30;
  if ((rc = launchDecode(d, P))) {
    return rc;
  }
  d->ended = true;
  d->resultsSynced = false;
  d->backtraced = false;
  d->hostFetched = false;
  d->compactFetched = false;
  d->scoresFetched = false;
  return FLTX_OK;
}

int fltx_stream_prune(fltx_decoder* d, int32_t lookBack) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (d && stepKindCalls(d->kind)) {
    return fail(FLTX_ERR_STATE, "fltx_stream_prune: %s", stepKindCalls(d->kind));
  }
  if (!d || lookBack < 0) {
    return fail(FLTX_ERR_INVALID, "fltx_stream_prune: bad argument");
  }
  if (!d->streaming) {
    return fail(FLTX_ERR_STATE, "fltx_stream_prune: call fltx_stream_begin first");
  }
  int rc = FLTX_OK;
  if (d->chunkPending && d->pendingPrune < 0) {
    d->pendingPrune = lookBack; /* runs right after the look at the pending chunk (settleStream) */
  } else if ((rc = settleStream(d)) || (rc = launchStreamOp(d, 1, lookBack, 0))) {
    return rc;
  }
  if (d->lm->kind == 2 && (rc = hostLmRetain(d))) {
    return rc;
  }
  d->resultsSynced = false;
  d->backtraced = false;
  d->hostFetched = false;
  d->compactFetched = false;
  d->scoresFetched = false;
  if (d->kind == FLTX_DECODER_LEXFREE) {
    /* every hypothesis of the lexicon-free decoder is complete (LexiconFreeDecoder.h:84-86): findBestAncestor stops
     * exactly lookBack frames back, so what stays buffered is known without asking the device (no wait per chunk;
     * fltx_stream_frames_in_buffer still reads the device's count) */
    for (int b = 0; b < d->B; ++b) {
      if (d->frames[b] - lookBack >= 1) {
        d->frames[b] = lookBack;
      }
    }
    return FLTX_OK;
  }
  /* the lexicon decoder prunes back to a complete hypothesis (LexiconDecoder.h:97-99), or not at all: what stays buffered
   * is the device's to say.  No wait here: frames[] stays the upper bound "nothing pruned" and fltx_stream_step asks
   * the device only when that bound would not fit max_frames */
  d->framesExact = false;
  return FLTX_OK;
}

static int checkStatus(fltx_decoder* d, int b);

int fltx_stream_frames_in_buffer(fltx_decoder* d, int32_t b, int32_t* n) {
  EntryScope entry(d); /* (syncResults may run the deferred second pass of a chunk) */
  if (entry.rc) {
    return entry.rc;
  }
  if (!d || !n || b < 0 || b >= d->B) {
    return fail(FLTX_ERR_INVALID, "bad argument");
  }
  int rc = syncResults(d);
  if (rc) {
    return rc;
  }
  *n = d->hFrame[b] + 1;
  return FLTX_OK;
}

static int checkStatus(fltx_decoder* d, int b) {
  int s = d->hStatus[b];
  if (s & ST_CAND_OVERFLOW) {
    return fail(FLTX_ERR_UNSUPPORTED, "utterance %d: candidate buffer overflow (CAP=%d)", b, d->CAP);
  }
  if (s & ST_TABLE_FULL) {
    return fail(FLTX_ERR_UNSUPPORTED, "utterance %d: LM-state table full (cap=%u)", b, d->stateCap);
  }
  if (s & ST_SELECT_FALLBACK) {
    return fail(FLTX_ERR_UNSUPPORTED, "utterance %d: top-K select did not converge (non-finite scores?)", b);
  }
  if (s & ST_HLM_MISS) {
    return fail(FLTX_ERR_STATE, "utterance %d: host LM: a frame asked a question that had not been listed (internal error)", b);
  }
  return FLTX_OK;
}

int fltx_result_count(fltx_decoder* d, int32_t b, int32_t* nHyp, int32_t* length) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d || b < 0 || b >= d->B) {
    return fail(FLTX_ERR_INVALID, "fltx_result_count: bad argument");
  }
  if (!d->haveResults) {
    return fail(FLTX_ERR_STATE, "no decode has been run");
  }
  int rc = syncResults(d);
  if (rc) {
    return rc;
  }
  if ((rc = checkStatus(d, b))) {
    return rc;
  }
  int ff = d->hFrame[b];
  int n = d->hN[b];
  /* LexiconDecoder.cpp:276-280: nothing before the first frame */
  if (d->kind == FLTX_DECODER_LEXICON && ff < 1) {
    n = 0;
  }
  if (nHyp) {
    *nHyp = n;
  }
  if (length) {
    *length = ff + 1;
  }
  return FLTX_OK;
}

int fltx_result_fetch(fltx_decoder* d, int32_t b, int32_t maxHyp, double* scores, int32_t* tokens,
                      int32_t* words, int32_t* nCopied) {
  int32_t n = 0, len = 0;
  int rc = fltx_result_count(d, b, &n, &len);
  if (rc) {
    return rc;
  }
  n = std::min(n, maxHyp);
  if (nCopied) {
    *nCopied = n;
  }
  if (n <= 0) {
    return FLTX_OK;
  }
  Stream st = d->ctx->stream;
  const int K = d->opt.beam_size;
  if (scores) {
    /* beam slots are score-sorted; after decodeEnd they are the final n-best */
    std::vector<double> sc((size_t)n), am((size_t)n), lm((size_t)n);
    if (d->ended) {
      if (devCopyD2H(scores, d->outScores.as<double>() + (size_t)b * K * 3, 8 * 3 * (size_t)n, st)) {
        return fail(FLTX_ERR_HIP, "score copy failed");
      }
    } else {
      if (devCopyD2H(sc.data(), d->gScore.as<double>() + (size_t)b * K, 8 * (size_t)n, st) ||
          devCopyD2H(am.data(), d->gAm.as<double>() + (size_t)b * K, 8 * (size_t)n, st) ||
          devCopyD2H(lm.data(), d->gLm.as<double>() + (size_t)b * K, 8 * (size_t)n, st)) {
        return fail(FLTX_ERR_HIP, "score copy failed");
      }
      for (int i = 0; i < n; ++i) {
        scores[3 * i] = sc[i];
        scores[3 * i + 1] = am[i];
        scores[3 * i + 2] = lm[i];
      }
    }
  }
  if (tokens || words) {
    if (!d->backtraced && (rc = launchBacktrace(d))) {
      return rc;
    }
    const int64_t base = d->histOff[b];
    if (tokens && devCopyD2H(tokens, d->tokens.as<int32_t>() + base, 4 * (size_t)n * len, st)) {
      return fail(FLTX_ERR_HIP, "token copy failed");
    }
    if (words) {
      if (kindHasWords(d->kind)) {
        if (devCopyD2H(words, d->words.as<int32_t>() + base, 4 * (size_t)n * len, st)) {
          return fail(FLTX_ERR_HIP, "word copy failed");
        }
      } else {
        std::fill(words, words + (size_t)n * len, -1); /* LexiconFreeDecoder.h:80-82 */
      }
    }
  }
  return FLTX_OK;
}

int fltx_result_fetch_batch(fltx_decoder* d, const int32_t** nHyp, const int32_t** length, const double** scores,
                            const int32_t** tokens, const int32_t** words, const int64_t** offsets) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d) {
    return fail(FLTX_ERR_INVALID, "fltx_result_fetch_batch: null decoder");
  }
  if (!d->haveResults || !d->ended) {
    return fail(FLTX_ERR_STATE, "fltx_result_fetch_batch: no finished decode (use fltx_result_fetch on a stream)");
  }
  int rc = syncResults(d);
  if (rc) {
    return rc;
  }
  const int B = d->B, K = d->opt.beam_size;
  for (int b = 0; b < B; ++b) {
    if ((rc = checkStatus(d, b))) {
      return rc;
    }
  }
  if (!d->hostFetched) {
    if (!d->backtraced && (rc = launchBacktrace(d))) {
      return rc;
    }
    Stream st = d->ctx->stream;
    const size_t nRec = (size_t)std::max<int64_t>(d->histRecords, 1);
    if (d->hTokens.ensure(4 * nRec) || d->hScores.ensure(8 * 3 * (size_t)B * K) ||
        (kindHasWords(d->kind) && d->hWords.ensure(4 * nRec))) {
      return fail(FLTX_ERR_OOM, "pinned result buffers: allocation failed");
    }
    if (devCopyD2H(d->hScores.p, d->outScores.p, 8 * 3 * (size_t)B * K, st) ||
        devCopyD2H(d->hTokens.p, d->tokens.p, 4 * nRec, st) ||
        (kindHasWords(d->kind) && devCopyD2H(d->hWords.p, d->words.p, 4 * nRec, st))) {
      return fail(FLTX_ERR_HIP, "result copy failed: %s", devErr());
    }
    d->hLen.resize(B);
    d->hNHyp.resize(B);
    for (int b = 0; b < B; ++b) {
      d->hLen[b] = d->hFrame[b] + 1;
      /* LexiconDecoder.cpp:276-280: nothing before the first frame */
      d->hNHyp[b] = (d->kind == FLTX_DECODER_LEXICON && d->hFrame[b] < 1) ? 0 : d->hN[b];
    }
    d->hostFetched = true;
  }
  if (nHyp) {
    *nHyp = d->hNHyp.data();
  }
  if (length) {
    *length = d->hLen.data();
  }
  if (scores) {
    *scores = (const double*)d->hScores.p;
  }
  if (tokens) {
    *tokens = (const int32_t*)d->hTokens.p;
  }
  if (words) {
    *words = kindHasWords(d->kind) ? (const int32_t*)d->hWords.p : nullptr;
  }
  if (offsets) {
    *offsets = d->histOff.data();
  }
  return FLTX_OK;
}

static int trMark(TrBufs& T, int i, Stream st);
static void trElapsed(TrBufs& T, int from, int to, int slot);

int fltx_result_fetch_batch_compact(fltx_decoder* d, const int32_t** nHyp, const int32_t** length,
                                    const double** scores, const uint8_t** tokensU8, const int32_t** words,
                                    const int64_t** offsets) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d) {
    return fail(FLTX_ERR_INVALID, "fltx_result_fetch_batch_compact: null decoder");
  }
  if (!d->haveResults || !d->ended) {
    return fail(FLTX_ERR_STATE, "fltx_result_fetch_batch_compact: no finished decode");
  }
  if (d->N >= 255) {
    return fail(FLTX_ERR_UNSUPPORTED, "fltx_result_fetch_batch_compact: %d tokens do not fit a byte", d->N);
  }
  int rc = syncResults(d);
  if (rc) {
    return rc;
  }
  const int B = d->B, K = d->opt.beam_size;
  for (int b = 0; b < B; ++b) {
    if ((rc = checkStatus(d, b))) {
      return rc;
    }
  }
  if (!d->compactFetched) {
    if (!d->backtraced && (rc = launchBacktrace(d))) {
      return rc;
    }
    Stream st = d->ctx->stream;
    const bool lex = kindHasWords(d->kind);
    d->hLen.resize(B);
    d->hNHyp.resize(B);
    d->packOff.resize((size_t)B + 1);
    /* meta (one upload): dstOff[B] int64, count[B] int32 */
    if (d->hPackMeta.ensure(12 * (size_t)B) || d->dPackMeta.ensure(12 * (size_t)B, st, false)) {
      return fail(FLTX_ERR_OOM, "compact results: allocation failed");
    }
    int64_t* hOff = (int64_t*)d->hPackMeta.p;
    int32_t* hCnt = (int32_t*)(hOff + B);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
      d->hLen[b] = d->hFrame[b] + 1;
      d->hNHyp[b] = (lex && d->hFrame[b] < 1) ? 0 : d->hN[b]; /* LexiconDecoder.cpp:276-280 */
      d->packOff[b] = total;
      hOff[b] = total;
      hCnt[b] = d->hNHyp[b] * d->hLen[b];
      total += hCnt[b];
    }
    d->packOff[B] = total;
    const size_t tot = (size_t)std::max<int64_t>(total, 1);
    if (d->dTok8.ensure(tot, st, false) || d->hTok8.ensure(tot) || d->hScores.ensure(8 * 3 * (size_t)B * K) ||
        (lex && (d->dWordsC.ensure(4 * tot, st, false) || d->hWordsC.ensure(4 * tot)))) {
      return fail(FLTX_ERR_OOM, "compact results: allocation failed");
    }
    if (devCopyH2D(d->dPackMeta.p, d->hPackMeta.p, 12 * (size_t)B, st)) {
      return fail(FLTX_ERR_HIP, "compact results: upload failed");
    }
#ifdef FLTX_EMU
    for (int b = 0; b < B; ++b) {
      const int32_t* src = d->tokens.as<int32_t>() + d->histOff[b];
      for (int i = 0; i < hCnt[b]; ++i) {
        d->dTok8.as<uint8_t>()[hOff[b] + i] = src[i] < 0 ? (uint8_t)0xFF : (uint8_t)src[i];
        if (lex) {
          d->dWordsC.as<int32_t>()[hOff[b] + i] = d->words.as<int32_t>()[d->histOff[b] + i];
        }
      }
    }
#else
    PackParams Q;
    Q.tokens = d->tokens.as<int32_t>();
    Q.words = lex ? d->words.as<int32_t>() : nullptr;
    Q.srcOff = d->histOffD.as<int64_t>();
    Q.dstOff = d->dPackMeta.as<int64_t>();
    Q.count = (const int32_t*)(d->dPackMeta.as<int64_t>() + B);
    Q.tok8 = d->dTok8.as<uint8_t>();
    Q.wordsOut = lex ? d->dWordsC.as<int32_t>() : nullptr;
    if (trMark(d->tr, 0, st)) {
      return fail(FLTX_ERR_HIP, "compact results: event failed");
    }
    hipLaunchKernelGGL(fltx_pack_results_kernel, dim3(B), dim3(256), 0, st, Q);
    HIPCHK(hipGetLastError());
    if (trMark(d->tr, 1, st)) {
      return fail(FLTX_ERR_HIP, "compact results: event failed");
    }
#endif
    if ((!d->scoresFetched && devCopyD2H(d->hScores.p, d->outScores.p, 8 * 3 * (size_t)B * K, st)) ||
        (total > 0 && devCopyD2H(d->hTok8.p, d->dTok8.p, (size_t)total, st)) ||
        (lex && total > 0 && devCopyD2H(d->hWordsC.p, d->dWordsC.p, 4 * (size_t)total, st))) {
      return fail(FLTX_ERR_HIP, "result copy failed: %s", devErr());
    }
    d->scoresFetched = true;
    d->compactFetched = true;
    if (d->tr.timed) {
      trElapsed(d->tr, 0, 1, 3);
    }
  }
  if (nHyp) {
    *nHyp = d->hNHyp.data();
  }
  if (length) {
    *length = d->hLen.data();
  }
  if (scores) {
    *scores = (const double*)d->hScores.p;
  }
  if (tokensU8) {
    *tokensU8 = (const uint8_t*)d->hTok8.p;
  }
  if (words) {
    *words = kindHasWords(d->kind) ? (const int32_t*)d->hWordsC.p : nullptr;
  }
  if (offsets) {
    *offsets = d->packOff.data();
  }
  return FLTX_OK;
}

static int crsResultBest(fltx_decoder* d, int32_t b, int32_t lookBack, double* scores, int32_t* tokens, int32_t* words,
                  int32_t capacity, int32_t* length);

int fltx_result_best(fltx_decoder* d, int32_t b, int32_t lookBack, double* scores, int32_t* tokens,
                     int32_t* words, int32_t capacity, int32_t* length) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d || b < 0 || b >= d->B || lookBack < 0 || !length) {
    return fail(FLTX_ERR_INVALID, "fltx_result_best: bad argument");
  }
  if (isCrKind(d->kind) && d->s2s.begun && d->s2s.crStream) { /* inside a stream: getBestHypothesis(lookBack) */
    return crsResultBest(d, b, lookBack, scores, tokens, words, capacity, length);
  }
  if (!d->haveResults) {
    return fail(FLTX_ERR_STATE, "no decode has been run");
  }
  if (stepKindCalls(d->kind)) { /* getBestHypothesis ignores lookBack: the final beam's first (:165-169) */
    int32_t n = 0, len = 0;
    int rc = fltx_result_count(d, b, &n, &len);
    if (rc) {
      return rc;
    }
    *length = n > 0 ? len : 0;
    if (n == 0) {
      return FLTX_OK;
    }
    if (len > capacity) {
      return fail(FLTX_ERR_RANGE, "fltx_result_best: capacity %d < length %d", capacity, len);
    }
    return fltx_result_fetch(d, b, 1, scores, tokens, words, &n);
  }
  if (!d->keepScores) {
    return fail(FLTX_ERR_STATE,
                "getBestHypothesis needs the per-frame score history: use the streaming calls or "
                "fltx_decoder_set(dec, \"keep_scores\", 1) before decoding");
  }
  int rc = syncResults(d);
  if (rc) {
    return rc;
  }
  if ((rc = checkStatus(d, b))) {
    return rc;
  }
  int maxLen = 0;
  for (int i = 0; i < d->B; ++i) {
    maxLen = std::max(maxLen, d->hFrame[i] + 1);
  }
  Stream st = d->ctx->stream;
  if (d->bestLen.ensure(4 * (size_t)d->B, st, true) || d->bestScores.ensure(24 * (size_t)d->B, st, true) ||
      d->bestTok.ensure(4 * (size_t)d->B * maxLen, st, false) ||
      d->bestWrd.ensure(4 * (size_t)d->B * maxLen, st, false)) {
    return fail(FLTX_ERR_OOM, "best-hypothesis buffers: allocation failed");
  }
  if ((rc = launchStreamOp(d, 0, lookBack, maxLen))) {
    return rc;
  }
  int32_t len = 0;
  if (devCopyD2H(&len, d->bestLen.as<int32_t>() + b, 4, st)) {
    return fail(FLTX_ERR_HIP, "copy failed");
  }
  *length = len;
  if (len == 0) {
    return FLTX_OK; /* empty DecodeResult */
  }
  if (len > capacity) {
    return fail(FLTX_ERR_RANGE, "fltx_result_best: capacity %d < length %d", capacity, len);
  }
  if (scores && devCopyD2H(scores, d->bestScores.as<double>() + 3 * (size_t)b, 24, st)) {
    return fail(FLTX_ERR_HIP, "copy failed");
  }
  if (tokens && devCopyD2H(tokens, d->bestTok.as<int32_t>() + (size_t)b * maxLen, 4 * (size_t)len, st)) {
    return fail(FLTX_ERR_HIP, "copy failed");
  }
  if (words) {
    if (d->kind == FLTX_DECODER_LEXICON) {
      if (devCopyD2H(words, d->bestWrd.as<int32_t>() + (size_t)b * maxLen, 4 * (size_t)len, st)) {
        return fail(FLTX_ERR_HIP, "copy failed");
      }
    } else {
      std::fill(words, words + len, -1);
    }
  }
  return FLTX_OK;
}

int fltx_result_device(fltx_decoder* d, const int32_t** nHyp, const double** scores,
                       const int32_t** tokens, const int32_t** words, const int64_t** tokOff) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d || !d->haveResults) {
    return fail(FLTX_ERR_STATE, "no decode has been run");
  }
  if (d->offlinePending) { /* "defer_check": the look at the statuses (and the second pass) before anybody reads the results */
    int rc = syncResults(d);
    if (rc) {
      return rc;
    }
  }
  if (!d->backtraced) {
    int rc = launchBacktrace(d);
    if (rc) {
      return rc;
    }
  }
  if (nHyp) {
    *nHyp = d->outN.as<int32_t>();
  }
  if (scores) {
    *scores = d->outScores.as<double>();
  }
  if (tokens) {
    *tokens = d->tokens.as<int32_t>();
  }
  if (words) {
    *words = kindHasWords(d->kind) ? d->words.as<int32_t>() : nullptr;
  }
  if (tokOff) {
    *tokOff = d->histOffD.as<int64_t>();
  }
  return FLTX_OK;
}

/* phase profile of the last launch: out[8] = shader clocks summed over the
 * utterances of the batch (0 prep, 1 generate, 2 fold, 3 select, 4 build,
 * 5 row hand-over) */
int fltx_decoder_profile(fltx_decoder* d, uint64_t* out) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d || !out) {
    return fail(FLTX_ERR_INVALID, "null argument");
  }
  if (!d->profile || !d->prof.p) {
    return fail(FLTX_ERR_STATE, "profiling is off: fltx_decoder_set(dec, \"profile\", 1)");
  }
  std::vector<unsigned long long> h(8 * (size_t)d->B);
  if (devCopyD2H(h.data(), d->prof.p, 8 * h.size(), d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "profile copy failed");
  }
  for (int i = 0; i < 8; ++i) {
    out[i] = 0;
  }
  for (size_t i = 0; i < h.size(); ++i) {
    out[i & 7] += h[i];
  }
  return FLTX_OK;
}

int fltx_decoder_timing(fltx_decoder* d, float* decodeMs, float* backtraceMs) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d) {
    return fail(FLTX_ERR_INVALID, "null decoder");
  }
#ifdef FLTX_EMU
  if (decodeMs) {
    *decodeMs = 0;
  }
  if (backtraceMs) {
    *backtraceMs = 0;
  }
  return FLTX_OK;
#else
  if (!d->timed) {
    return fail(FLTX_ERR_STATE, "no timed decode_batch has been run");
  }
  HIPCHK(hipEventSynchronize(d->ev[2]));
  float a = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&a, d->ev[0], d->ev[1]));
  HIPCHK(hipEventElapsedTime(&b, d->ev[1], d->ev[2]));
  if (decodeMs) {
    *decodeMs = a;
  }
  if (backtraceMs) {
    *backtraceMs = b;
  }
  return FLTX_OK;
#endif
}

int fltx_decoder_stats(fltx_decoder* d, int64_t* frames, int64_t* bytes, int32_t* threads,
                       int32_t* ldsBytes) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d) {
    return fail(FLTX_ERR_INVALID, "null decoder");
  }
  if (d->haveResults && d->ended && !d->streaming) {
    int rc = accountBytes(d);
    if (rc) {
      return rc;
    }
  }
  if (frames) {
    *frames = d->statFrames;
  }
  if (bytes) {
    *bytes = d->statBytes;
  }
  if (threads) {
    *threads = d->threads;
  }
  if (ldsBytes) {
    *ldsBytes = d->wsInLds ? (int32_t)d->wsBytes : 0;
  }
  return FLTX_OK;
}

int fltx_decoder_bytes(fltx_decoder* d, int64_t* decodeBytes, int64_t* epilogueBytes, int64_t* lmBytes) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d) {
    return fail(FLTX_ERR_INVALID, "null decoder");
  }
  if (!d->haveResults || !d->ended || d->streaming) {
    return fail(FLTX_ERR_STATE, "fltx_decoder_bytes: no finished offline decode");
  }
  int rc = accountBytes(d);
  if (rc) {
    return rc;
  }
  if (decodeBytes) {
    *decodeBytes = d->statDecodeBytes;
  }
  if (epilogueBytes) {
    *epilogueBytes = d->statEpilogueBytes;
  }
  if (lmBytes) {
    *lmBytes = d->statLmBytes;
  }
  return FLTX_OK;
}


/* ---- seq2seq (fltx_s2s.h) ------------------------------------------------------------------------------------------ */
static int s2sCheck(fltx_decoder* d, const char* what) {
  if (!d) {
    return fail(FLTX_ERR_INVALID, "%s: null decoder", what);
  }
  if (!isS2sKind(d->kind)) {
    return fail(FLTX_ERR_STATE, "%s: not a seq2seq decoder (fltx_s2s_decoder_create)", what);
  }
  return FLTX_OK;
}

/* a seq2seq launch, written once for both builds: `kernel` over grid x block workgroups on the stream; the emulator runs
 * `body`, the device function that kernel wraps, on host threads with `lds` bytes per workgroup */
#ifdef FLTX_EMU
#define S2S_LAUNCH(kernel, body, grid, block, lds, st, params) \
  emuLaunch((grid), (block), (lds), [&](char* smem) { body((params), smem); })
#else
#define S2S_LAUNCH(kernel, body, grid, block, lds, st, params)              \
  do {                                                                       \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (st), (params)); \
    HIPCHK(hipGetLastError());                                               \
  } while (0)
#endif

/* ---- what the step decoders' host code decides once (seq2seq, the CTC rows kinds, their streams and finishes) ---------- */
/* a fltx_dtype and a kind of the ABI, and the bytes of an element */
static bool s2sDtypeOk(int32_t dtype) {
  return dtype == FLTX_DTYPE_F32 || dtype == FLTX_DTYPE_F16 || dtype == FLTX_DTYPE_BF16;
}
static bool s2sKindOk(int32_t kind) { return kind == FLTX_S2S_LOG_PROBS || kind == FLTX_S2S_LOGITS; }
static size_t s2sDtypeBytes(int32_t dtype) { return dtype == FLTX_DTYPE_F32 ? 4 : 2; }

extern "C++" { /* (templates, inside this file's extern "C" block) */
/* the one map from a checked (dtype, logits) to the <DT, LOGITS> of a kernel: f(dt, lg) gets the pair as compile-time
 * constants -- S2S_DT_LOGITS names them inside a generic lambda, in both builds */
template <class F>
static int s2sTypedDispatch(int32_t dtype, bool logits, F&& f) {
  using F32 = std::integral_constant<int, kS2sDtF32>;
  using F16 = std::integral_constant<int, kS2sDtF16>;
  using Bf16 = std::integral_constant<int, kS2sDtBf16>;
  switch (dtype * 2 + (logits ? 1 : 0)) {
    case 0: return f(F32(), std::false_type());
    case 1: return f(F32(), std::true_type());
    case 2: return f(F16(), std::false_type());
    case 3: return f(F16(), std::true_type());
    case 4: return f(Bf16(), std::false_type());
    default: return f(Bf16(), std::true_type());
  }
}
}
#define S2S_DT_LOGITS(dt, lg)              \
  constexpr int DT = decltype(dt)::value; \
  constexpr bool LOGITS = decltype(lg)::value
/* the gather of a rows LM's scores into recLm by `kernel` / `body`, templates on the LM rows' <DT, LOGITS>: log-probs
 * take a wave per row, four rows per workgroup; logits a workgroup per row */
#define S2S_LM_ROWS_LAUNCH(kernel, body, dtype, logits, nRows, st, params)                                      \
  s2sTypedDispatch((dtype), (logits), [&](auto dt, auto lg) -> int {                                             \
    S2S_DT_LOGITS(dt, lg);                                                                                       \
    S2S_LAUNCH((kernel<DT, LOGITS>), (body<DT, LOGITS>), LOGITS ? (nRows) : ((nRows) + 3) / 4, kS2sLmThreads,    \
               sizeof(S2sLmRowsLds), (st), (params));                                                            \
    return FLTX_OK;                                                                                              \
  })

/* the rows of a rows LM of either level as the gather kernels take them (R.s is the caller's) */
static void s2sLmRowsFill(S2sLmRowsParams& R, fltx_decoder* d, const void* x, int64_t rowStride, bool logits,
                          double* rowLse) {
  R.x = x;
  R.rowStride = rowStride;
  R.width = d->s2s.lmWidth;
  R.finishIdx = d->s2s.lmFinish;
  R.usrToLm = d->lm->rowsMap ? d->lmDev->usrToLm.as<int32_t>() : nullptr;
  R.recLm = d->s2s.recLm.as<float>();
  R.rowLse = logits ? rowLse : nullptr;
}

/* a call's LM rows on the device: the host's nLm rows are copied into the decoder's staging buffer in their own type --
 * the last row ends after the LM's width, not after a stride -- and so are the B*K entries of lm_row_of when it is
 * given; the pointers then name the copies.  `who` starts the message of a failure */
static int s2sStageLmRows(fltx_decoder* d, const char* who, int32_t dtype, int64_t rowStride, size_t nLm, size_t BK,
                          const void** lmScores, const int32_t** lmRowOf, Stream st) {
  const size_t bytes = s2sDtypeBytes(dtype) * ((nLm - 1) * (size_t)rowStride + (size_t)d->s2s.lmWidth);
  if (d->s2s.lmScores.ensure(bytes, st, false) || (*lmRowOf && d->s2s.lmRowOf.ensure(4 * BK, st, false))) {
    return fail(FLTX_ERR_OOM, "%s: staging allocation failed", who);
  }
  if (devCopyH2D(d->s2s.lmScores.p, *lmScores, bytes, st) ||
      (*lmRowOf && devCopyH2D(d->s2s.lmRowOf.p, *lmRowOf, 4 * BK, st))) {
    return fail(FLTX_ERR_HIP, "%s: upload failed", who);
  }
  *lmScores = d->s2s.lmScores.p;
  *lmRowOf = *lmRowOf ? d->s2s.lmRowOf.as<int32_t>() : nullptr;
  return FLTX_OK;
}

/* a call with nothing to score still answers a logits caller: every row's lse a NaN (all-ones) */
static int s2sIdleLse(const char* what, bool logits, double* rowLse, size_t BK, Stream st) {
  if (logits && rowLse && devMemset(rowLse, 0xFF, 8 * BK, st)) {
    return fail(FLTX_ERR_HIP, "%s: memset failed", what);
  }
  return FLTX_OK;
}

/* where a back-trace leaves its results: the decoder's own buffers (an end) or the fin* ones (a finish) */
struct StepResults {
  double* scores;
  int32_t *tokens, *nHyp, *nBeam, *frame, *status;
};
static void s2sSetResults(S2sParams& P, const StepResults& r) {
  P.outScores = r.scores;
  P.tokens = r.tokens;
  P.outNHyp = r.nHyp;
  P.uttNBeam = r.nBeam;
  P.uttFrame = r.frame;
  P.uttStatus = r.status;
}

/* the results of an end (fltx_s2s_end, fltx_ctc_rows_end) as every decoder's results are read: the buffers -- words
 * where the kind has words -- histOff on the device, and P's result pointers.  `who` starts the message of a failure */
static int stepEndResults(fltx_decoder* d, const char* who, S2sParams& P) {
  Stream st = d->ctx->stream;
  const size_t B = (size_t)d->B, nRec = (size_t)std::max<int64_t>(d->histRecords, 1);
  if (d->outScores.ensure(24 * B * d->opt.beam_size, st, false) || d->tokens.ensure(4 * nRec, st, false) ||
      d->outN.ensure(4 * B, st, false) || ensureUttRes(d, d->B, st) || d->histOffD.ensure(8 * (B + 1), st, false) ||
      (kindHasWords(d->kind) && d->words.ensure(4 * nRec, st, false))) {
    return fail(FLTX_ERR_OOM, "%s results: device allocation failed", who);
  }
  if (uploadHistOff(d, st)) {
    return fail(FLTX_ERR_HIP, "%s results: upload failed", who);
  }
  s2sSetResults(P, {d->outScores.as<double>(), d->tokens.as<int32_t>(), d->outN.as<int32_t>(),
                    d->uttNBeam.as<int32_t>(), d->uttFrame.as<int32_t>(), d->uttStatus.as<int32_t>()});
  return FLTX_OK;
}
/* ... and what the decoder knows once the end's kernels are queued */
static void stepEnded(fltx_decoder* d) {
  d->haveResults = true;
  d->ended = true;
  d->backtraced = true;
  d->streaming = false;
  d->resultsSynced = false;
  d->hostFetched = false;
  d->compactFetched = false;
  d->scoresFetched = false;
  d->offlinePending = false;
  d->lookQueued = false;
}

/* a copy home that waits for nothing: the caller synchronises once behind the last one */
static int crsCopyHomeAsync(void* h, const void* dv, size_t n, Stream st) {
#ifdef FLTX_EMU
  (void)st;
  memcpy(h, dv, n);
  return 0;
#else
  return hipMemcpyAsync(h, dv, n, hipMemcpyDeviceToHost, st) == hipSuccess ? 0 : 1;
#endif
}

/* the buffers of a finish (fltx_ctc_rows_stream_finish and fltx_s2s_finish share them by design): scores [B*K*3], nRec
 * tokens and words, the counts in finMeta, the call's input in finIn and, for the streams, finSkip; their pinned twins
 * unless the results stay */
static int stepFinishBuffers(fltx_decoder* d, const char* what, size_t nRec, size_t metaBytes, size_t inBytes,
                             size_t skipBytes, int32_t resultsOnDevice) {
  Stream st = d->ctx->stream;
  const size_t B = (size_t)d->B, K = (size_t)d->opt.beam_size;
  const bool lex = kindHasWords(d->kind);
  if (d->s2s.finScores.ensure(24 * B * K, st, false) || d->s2s.finTok.ensure(4 * nRec, st, false) ||
      (lex && d->s2s.finWrd.ensure(4 * nRec, st, false)) || d->s2s.finMeta.ensure(metaBytes, st, false) ||
      d->s2s.finIn.ensure(inBytes, st, false) || (skipBytes && d->s2s.finSkip.ensure(skipBytes, st, false)) ||
      (!resultsOnDevice && (d->s2s.hFinScores.ensure(24 * B * K) || d->s2s.hFinTok.ensure(4 * nRec) ||
                            (lex && d->s2s.hFinWrd.ensure(4 * nRec)) || d->s2s.hFinMeta.ensure(12 * B)))) {
    return fail(FLTX_ERR_OOM, "%s: allocation failed (B=%d K=%d)", what, d->B, d->opt.beam_size);
  }
  return FLTX_OK;
}

extern "C++" {
/* the results of a finish: *out points at the device's, or at the host's after copying them home -- the counts
 * {n_hyp, counts, status}[B] of finMeta first, then what the named slots really have, n_hyp hypotheses each, and one
 * wait.  Slot b's rows start at rowOff[b] (null: b * K * len) and a hypothesis has len entries (0: the slot's own
 * count).  `counts` is the member of OUT the second count goes by; what else OUT has is the caller's */
template <class OUT>
static int stepFinishResults(fltx_decoder* d, const char* what, int32_t resultsOnDevice, const int64_t* rowOff,
                             int32_t len, const int32_t* OUT::*counts, OUT* out) {
  Stream st = d->ctx->stream;
  const size_t B = (size_t)d->B, K = (size_t)d->opt.beam_size;
  const bool lex = kindHasWords(d->kind);
  const int32_t* meta = d->s2s.finMeta.as<int32_t>();
  if (!resultsOnDevice) {
    int32_t* hMeta = (int32_t*)d->s2s.hFinMeta.p;
    if (devCopyD2H(hMeta, meta, 12 * B, st)) {
      return fail(FLTX_ERR_HIP, "%s: result copy failed: %s", what, devErr());
    }
    int bad = 0;
    for (size_t b = 0; b < B && !bad; ++b) {
      const size_t n = (size_t)hMeta[b], at = rowOff ? (size_t)rowOff[b] : b * K * (size_t)len;
      const size_t cnt = n * (size_t)(len ? len : hMeta[B + b]), sAt = 3 * b * K;
      if (n == 0) {
        continue;
      }
      bad = crsCopyHomeAsync((double*)d->s2s.hFinScores.p + sAt, d->s2s.finScores.as<double>() + sAt, 24 * n, st) ||
            crsCopyHomeAsync((int32_t*)d->s2s.hFinTok.p + at, d->s2s.finTok.as<int32_t>() + at, 4 * cnt, st) ||
            (lex && crsCopyHomeAsync((int32_t*)d->s2s.hFinWrd.p + at, d->s2s.finWrd.as<int32_t>() + at, 4 * cnt, st));
    }
    if (bad || devSync(st)) {
      return fail(FLTX_ERR_HIP, "%s: result copy failed: %s", what, devErr());
    }
    meta = hMeta;
  }
  out->n_hyp = meta;
  out->*counts = meta + B;
  out->status = meta + 2 * B;
  out->scores = resultsOnDevice ? d->s2s.finScores.as<double>() : (const double*)d->s2s.hFinScores.p;
  out->tokens = resultsOnDevice ? d->s2s.finTok.as<int32_t>() : (const int32_t*)d->s2s.hFinTok.p;
  out->words = !lex ? nullptr : resultsOnDevice ? d->s2s.finWrd.as<int32_t>() : (const int32_t*)d->s2s.hFinWrd.p;
  return FLTX_OK;
}
}

static S2sParams s2sParams(fltx_decoder* d) {
  S2sParams P;
  memset(&P, 0, sizeof(P));
  const fltx_lm* lm = d->lm;
  if (lm->kind == 1) {
    P.lmOn = 1;
    P.lmp.lmKind = 1;
    P.lmp.lmOrder = lm->order;
    P.lmp.ngTab = d->lmDev->tab.as<NgramSlot>();
    P.lmp.ngMask = lm->mask;
    P.lmp.ngBackoff = d->lmDev->backoff.as<float>();
    P.lmp.usrToLm = d->lmDev->usrToLm.as<int32_t>();
    P.lmp.nUsr = lm->nUsr;
    P.lmp.lmBos = lm->bos;
    P.lmp.lmEos = lm->eos;
    P.lmp.lmUnk = lm->unk;
  }
  P.B = d->B;
  P.K = d->s2s.opt.beam_size;
  P.Kt = d->s2s.opt.beam_size_token;
  P.V = d->N;
  P.eos = d->s2s.eos;
  P.maxOut = d->s2s.maxOut;
  P.t = d->s2s.t;
  P.cap = d->s2s.cap;
  P.mSel = d->s2s.mSel;
  P.eosExtra = d->s2s.eosExtra;
  P.beamThreshold = d->s2s.opt.beam_threshold;
  P.lmWeight = d->s2s.opt.lm_weight;
  P.eosScore = d->s2s.opt.eos_score;
  P.beam = d->s2s.beam.as<S2sHyp>();
  P.beamN = d->s2s.beamN.as<int32_t>();
  P.hist = d->s2s.hist.as<int2>();
  P.nRowsInt = d->s2s.rowsInt.as<int32_t>();
  P.done = d->s2s.done.as<int32_t>();
  P.finalStep = d->s2s.finalStep.as<int32_t>();
  P.recTok = d->s2s.recTok.as<int32_t>();
  P.recAm = d->s2s.recAm.as<float>();
  P.recN = d->s2s.recN.as<int32_t>();
  P.cKey = d->s2s.cKey.as<unsigned long long>();
  P.nC = (int64_t)P.K * P.cap + P.K;
  for (int j = 0; j < kS2sCtx; ++j) {
    P.ctx0[j] = d->s2s.ctx0[j];
  }
  P.len = d->s2s.maxOut + 3;
  return P;
}

/* (fltx_s2s_lex_decoder_create makes its decoder here too: wordRows = it was given a word-level rows LM) */
static int s2sDecoderCreate(fltx_ctx* ctx, const fltx_s2s_options* opt, const fltx_lm* lm, int32_t eos, int32_t maxOut,
                            bool wordRows, fltx_decoder** out) {
  if (!ctx || !opt || !lm || !out) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_decoder_create: null argument");
  }
  if (lm->kind == 4 && !wordRows) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq: a word-level rows LM (fltx_lm_word_rows_create) serves the lexicon "
                                      "seq2seq decoder with is_lm_token == 0 only");
  }
  if (opt->beam_size < 1 || opt->beam_size_token < 1) {
    return fail(FLTX_ERR_INVALID, "beam_size and beam_size_token must be >= 1");
  }
  if (opt->beam_size > kS2sMaxBeam) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq: beam_size %d > %d", opt->beam_size, kS2sMaxBeam);
  }
  if (maxOut < 0) {
    return fail(FLTX_ERR_INVALID, "seq2seq: max_output_length < 0");
  }
  if (maxOut > kS2sMaxLen) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq: max_output_length %d > %d", maxOut, kS2sMaxLen);
  }
  if (eos < 0) {
    return fail(FLTX_ERR_INVALID, "seq2seq: eos index %d < 0", eos);
  }
  if (lm->kind == 2) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq: a user-defined (host) LM is not supported; ZeroLM or n-gram tables only");
  }
  if (lm->kind == 1 && lm->order - 1 > kS2sCtx) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq: n-gram order %d > %d", lm->order, kS2sCtx + 1);
  }
  EntryScope entry(ctx);
  if (entry.rc) {
    return entry.rc;
  }
  fltx_lm::Dev* lmDev = nullptr;
  int rc = lmEnsureUploaded(const_cast<fltx_lm*>(lm), ctx, &lmDev);
  if (rc) {
    return rc;
  }
  auto* d = new fltx_decoder();
  d->ctx = ctx;
  d->lm = lm;
  d->lmDev = lmDev;
  d->kind = FLTX_DECODER_S2S_LEXFREE;
  d->s2s.opt = *opt;
  d->opt.beam_size = opt->beam_size;
  d->opt.beam_size_token = opt->beam_size_token;
  d->opt.beam_threshold = opt->beam_threshold;
  d->opt.lm_weight = opt->lm_weight;
  d->opt.log_add = opt->log_add;
  d->opt.criterion = FLTX_CRITERION_S2S;
  d->s2s.eos = eos;
  d->s2s.maxOut = maxOut;
  if (lm->kind == 1) {
    int32_t c[kMaxNgramOrder] = {0};
    if ((rc = fltx_lm_start(const_cast<fltx_lm*>(lm), 0, c))) {
      delete d;
      return rc;
    }
    for (int j = 0; j < kS2sCtx; ++j) {
      d->s2s.ctx0[j] = j < lm->order - 1 ? c[j] : 0;
    }
  }
  *out = d;
  return FLTX_OK;
}

int fltx_s2s_decoder_create(fltx_ctx* ctx, const fltx_s2s_options* opt, const fltx_lm* lm, int32_t eos,
                            int32_t maxOut, fltx_decoder** out) {
  return s2sDecoderCreate(ctx, opt, lm, eos, maxOut, false, out);
}

/* ---- lexicon seq2seq (fltx_s2s_lex.h) ---------------------------------------------------------------------------- */
/* the parameters of either kind: .s is the lexicon-free view, the rest stays 0 without a lexicon */
/* a rows LM of either level: the finish index lies inside the LM's rows */
static int s2sRowsLmFinishCheck(int finish, int width) {
  if (finish < 0 || finish >= width) {
    return fail(FLTX_ERR_INVALID, "seq2seq rows LM: finish index %d outside the LM's rows of %d", finish, width);
  }
  return FLTX_OK;
}

static S2lParams s2sStepParams(fltx_decoder* d) {
  S2lParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.s = s2sParams(d);
  if (d->kind != FLTX_DECODER_S2S_LEXICON) {
    return Q;
  }
  Q.s.nC = (int64_t)Q.s.K * Q.s.cap * d->s2s.slots + Q.s.K;
  Q.trie.maxScore = d->s2s.trieMax.as<float>();
  Q.trie.kidOff = d->s2s.kidOff.as<int32_t>();
  Q.trie.kidTok = d->s2s.kidTok.as<int32_t>();
  Q.trie.kidNode = d->s2s.kidNode.as<int32_t>();
  Q.trie.labOff = d->s2s.labOff.as<int32_t>();
  Q.trie.labels = d->s2s.lab.as<int32_t>();
  Q.isLmToken = d->s2s.isLmToken ? 1 : 0;
  Q.S = d->s2s.slots;
  Q.wordScore = d->s2s.wordScore;
  Q.logAdd = d->s2s.opt.log_add ? 1 : 0;
  Q.beam = d->s2s.beam.as<S2lHyp>();
  Q.hist = d->s2s.hist.as<S2lRec>();
  Q.cScore = d->s2s.cScore.as<double>();
  Q.cMk = d->s2s.cMk.as<uint4>();
  Q.cGrp = d->s2s.cGrp.as<int32_t>();
  Q.cList = d->s2s.cList.as<int32_t>();
  Q.cNext = d->s2s.cNext.as<int32_t>();
  Q.mTab = d->s2s.mTab.as<int32_t>();
  Q.mSize = d->s2s.mSize;
  Q.sKey = d->s2s.sKey.as<unsigned long long>();
  Q.sVal = d->s2s.sVal.as<int32_t>();
  Q.sCount = d->s2s.sCount.as<int32_t>();
  Q.sSize = d->s2s.sSize;
  Q.sMax = d->s2s.sMax;
  Q.status = d->s2s.status.as<int32_t>();
  Q.merges = d->s2s.merges.as<int32_t>();
  return Q;
}

static int s2lPow2AtLeast(int64_t n) {
  int64_t p = 1;
  while (p < n) {
    p <<= 1;
  }
  return (int)p;
}

/* the compact trie: per node maxScore, children sorted by token (CSR) and labels; bytes ~ nodes + edges + labels */
static int s2lUploadTrie(fltx_decoder* d, fltx_htrie* t, std::vector<int32_t>* labelsOut = nullptr) {
  int64_t nn = 0;
  int rc = fltx_htrie_num_nodes(t, &nn);
  if (rc) {
    return rc;
  }
  if (nn >= (int64_t)1 << 31) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq lexicon: %lld trie nodes", (long long)nn);
  }
  std::vector<float> mx((size_t)nn);
  std::vector<int32_t> kidOff((size_t)nn + 1, 0), labOff((size_t)nn + 1, 0), kidTok, kidNode, lab;
  std::vector<int32_t> ct;
  std::vector<int64_t> cn;
  std::vector<std::pair<int32_t, int32_t>> kids;
  int maxLabels = 0;
  for (int64_t i = 0; i < nn; ++i) {
    int32_t nl = 0, nc = 0, labels[kS2lMaxLabels];
    float ms = 0.0f;
    if ((rc = fltx_htrie_node(t, i, nullptr, &ms, &nl, labels, nullptr, &nc, nullptr, nullptr, 0))) {
      return rc;
    }
    ct.resize((size_t)std::max(nc, 1));
    cn.resize((size_t)std::max(nc, 1));
    if ((rc = fltx_htrie_node(t, i, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ct.data(), cn.data(), nc))) {
      return rc;
    }
    kids.clear();
    for (int c = 0; c < nc; ++c) {
      kids.emplace_back(ct[c], (int32_t)cn[c]);
    }
    std::sort(kids.begin(), kids.end());
    for (const auto& kv : kids) {
      kidTok.push_back(kv.first);
      kidNode.push_back(kv.second);
    }
    for (int l = 0; l < nl; ++l) {
      lab.push_back(labels[l]);
    }
    maxLabels = std::max(maxLabels, (int)nl);
    mx[(size_t)i] = ms;
    kidOff[(size_t)i + 1] = (int32_t)kidTok.size();
    labOff[(size_t)i + 1] = (int32_t)lab.size();
  }
  Stream st = d->ctx->stream;
  const size_t nE = kidTok.size(), nL = lab.size();
  if (d->s2s.trieMax.ensure(4 * (size_t)nn, st, false) || d->s2s.kidOff.ensure(4 * ((size_t)nn + 1), st, false) ||
      d->s2s.kidTok.ensure(4 * std::max<size_t>(nE, 1), st, false) ||
      d->s2s.kidNode.ensure(4 * std::max<size_t>(nE, 1), st, false) ||
      d->s2s.labOff.ensure(4 * ((size_t)nn + 1), st, false) || d->s2s.lab.ensure(4 * std::max<size_t>(nL, 1), st, false)) {
    return fail(FLTX_ERR_OOM, "seq2seq lexicon: trie allocation failed (%lld nodes)", (long long)nn);
  }
  if (devCopyH2D(d->s2s.trieMax.p, mx.data(), 4 * (size_t)nn, st) ||
      devCopyH2D(d->s2s.kidOff.p, kidOff.data(), 4 * ((size_t)nn + 1), st) ||
      (nE && devCopyH2D(d->s2s.kidTok.p, kidTok.data(), 4 * nE, st)) ||
      (nE && devCopyH2D(d->s2s.kidNode.p, kidNode.data(), 4 * nE, st)) ||
      devCopyH2D(d->s2s.labOff.p, labOff.data(), 4 * ((size_t)nn + 1), st) ||
      (nL && devCopyH2D(d->s2s.lab.p, lab.data(), 4 * nL, st)) || devSync(st)) {
    return fail(FLTX_ERR_HIP, "seq2seq lexicon: trie upload failed");
  }
  d->s2s.nodes = nn;
  d->s2s.edges = (int64_t)nE;
  d->s2s.labels = (int64_t)nL;
  d->s2s.maxLabels = maxLabels;
  d->s2s.trieBytes = 4 * nn + 4 * 2 * (nn + 1) + 8 * (int64_t)nE + 4 * (int64_t)nL;
  if (labelsOut) {
    labelsOut->swap(lab);
  }
  return FLTX_OK;
}

int fltx_s2s_lex_decoder_create(fltx_ctx* ctx, const fltx_s2s_lex_options* opt, const fltx_htrie* trie,
                                const fltx_lm* lm, int32_t eos, int32_t maxOut, int32_t isLmToken, fltx_decoder** out) {
  if (!ctx || !opt || !trie || !lm || !out) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_lex_decoder_create: null argument");
  }
  if (lm->kind == 3 && !isLmToken) {
    /* (its rows are read one per decoder row through the token map: word-level rows come in by their own LM object) */
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq lexicon: a word-level rows LM (fltx_lm_rows_create with is_lm_token == 0) "
                                      "is not supported; make it with fltx_lm_word_rows_create");
  }
  if (lm->kind == 4 && isLmToken) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq lexicon: a word-level rows LM (fltx_lm_word_rows_create) goes with "
                                      "is_lm_token == 0");
  }
  fltx_s2s_options o{};
  o.beam_size = opt->beam_size;
  o.beam_size_token = opt->beam_size_token;
  o.beam_threshold = opt->beam_threshold;
  o.lm_weight = opt->lm_weight;
  o.eos_score = opt->eos_score;
  o.log_add = opt->log_add;
  fltx_decoder* d = nullptr;
  int rc = s2sDecoderCreate(ctx, &o, lm, eos, maxOut, lm->kind == 4, &d);
  if (rc) {
    return rc;
  }
  EntryScope entry(ctx);
  if (entry.rc) {
    delete d;
    return entry.rc;
  }
  d->kind = FLTX_DECODER_S2S_LEXICON;
  d->opt.word_score = opt->word_score;
  d->s2s.wordScore = opt->word_score;
  d->s2s.isLmToken = isLmToken != 0;
  d->s2s.maxStates = kS2lDefaultStates;
  std::vector<int32_t> labels;
  if ((rc = s2lUploadTrie(d, const_cast<fltx_htrie*>(trie), &labels))) {
    delete d;
    return rc;
  }
  if (lm->kind == 4) { /* every index the word gather can form lies inside the LM's rows */
    const int width = lm->rowsWidth;
    rc = s2sRowsLmFinishCheck(lm->rowsFinish, width);
    for (size_t i = 0; i < labels.size() && !rc; ++i) {
      const int32_t w = labels[i];
      if (w < 0 || (lm->rowsMap && w >= lm->nUsr)) {
        rc = fail(FLTX_ERR_INVALID, "seq2seq word rows LM: the trie's label %d outside the %d entries of word_to_lm", w,
                  lm->nUsr);
      } else {
        const int32_t idx = lm->rowsMap ? lm->hUsr[(size_t)w] : w;
        if (idx < 0 || idx >= width) {
          rc = fail(FLTX_ERR_INVALID, "seq2seq word rows LM: word %d has LM index %d outside the LM's rows of %d", w, idx,
                    width);
        }
      }
    }
    if (rc) {
      delete d;
      return rc;
    }
  }
  d->s2s.slots = 1 + (d->s2s.isLmToken ? std::min(d->s2s.maxLabels, 1) : d->s2s.maxLabels);
  *out = d;
  return FLTX_OK;
}

int fltx_s2s_lex_set_max_states(fltx_decoder* d, int32_t maxStates) {
  int rc = s2sCheck(d, "fltx_s2s_lex_set_max_states");
  if (rc) {
    return rc;
  }
  if (d->kind != FLTX_DECODER_S2S_LEXICON || maxStates < 1) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_lex_set_max_states: a lexicon seq2seq decoder and a count >= 1");
  }
  d->s2s.maxStates = maxStates;
  return FLTX_OK;
}

int fltx_s2s_lex_info(fltx_decoder* d, int64_t* trieBytes, int64_t* nNodes, int64_t* nEdges, int32_t* merges) {
  int rc = s2sCheck(d, "fltx_s2s_lex_info");
  if (rc) {
    return rc;
  }
  if (d->kind != FLTX_DECODER_S2S_LEXICON) {
    return fail(FLTX_ERR_STATE, "fltx_s2s_lex_info: not a lexicon seq2seq decoder");
  }
  EntryScope entry(d->ctx);
  if (entry.rc) {
    return entry.rc;
  }
  if (trieBytes) {
    *trieBytes = d->s2s.trieBytes;
  }
  if (nNodes) {
    *nNodes = d->s2s.nodes;
  }
  if (nEdges) {
    *nEdges = d->s2s.edges;
  }
  if (merges && d->s2s.begun) {
    if (devCopyD2H(merges, d->s2s.merges.p, 4 * (size_t)d->B, d->ctx->stream) || devSync(d->ctx->stream)) {
      return fail(FLTX_ERR_HIP, "fltx_s2s_lex_info: copy failed: %s", devErr());
    }
  }
  return FLTX_OK;
}

/* fltx_s2s_begin's parts that depend on the kind: the token beam the front end keeps (mSel / eosExtra / cap) and the
 * candidates per step (*nC); with a lexicon also the sizes of its tables, and then the buffers only it has */
/* a rows LM: every index the gather can form lies inside the LM's rows (either decoder kind) */
static int s2sPlanRowsLm(fltx_decoder* d, int32_t V) {
  const fltx_lm* lm = d->lm;
  const int eos = d->s2s.eos;
  const int width = lm->rowsWidth > 0 ? lm->rowsWidth : V;
  if (lm->rowsMap && V > lm->nUsr) {
    return fail(FLTX_ERR_INVALID, "seq2seq rows LM: V = %d > the %d entries of usr_to_lm", V, lm->nUsr);
  }
  int finish = lm->rowsFinish;
  if (finish < 0 && eos < V) {
    finish = lm->rowsMap ? lm->hUsr[(size_t)eos] : eos;
  }
  if (eos < V && s2sRowsLmFinishCheck(finish, width)) {
    return FLTX_ERR_INVALID;
  }
  if (lm->rowsMap) {
    for (int u = 0; u < V; ++u) {
      if (lm->hUsr[(size_t)u] < 0 || lm->hUsr[(size_t)u] >= width) {
        return fail(FLTX_ERR_INVALID, "seq2seq rows LM: usr_to_lm[%d] = %d outside the LM's rows of %d (lm_width 0: V)",
                    u, lm->hUsr[(size_t)u], width);
      }
    }
  } else if (width < V) {
    return fail(FLTX_ERR_INVALID, "seq2seq rows LM: lm_width %d < V = %d without a map", width, V);
  }
  d->s2s.lmWidth = width;
  d->s2s.lmFinish = eos < V ? finish : 0; /* (eos >= V is never proposed: finish is never read) */
  return FLTX_OK;
}

static int s2sPlanLexFree(fltx_decoder* d, int32_t V, int64_t* nC) {
  const int K = d->s2s.opt.beam_size, Kt = d->s2s.opt.beam_size_token;
  const int ktEff = std::min(Kt, V);
  /* without LM terms in the score a row contributes at most K survivors besides eos: its top min(Kt, K + 1) (one more
   * than K: eos may be among them) and eos when it is in the top Kt are every candidate that can survive */
  const bool lmTerms = (d->lm->kind == 1 || d->lm->kind == 3) && d->s2s.opt.lm_weight != 0.0;
  if (lmTerms && ktEff > kS2sMaxKtLm) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq: a token beam of %d (beam_size_token, V = %d) > %d with LM terms", ktEff, V,
                kS2sMaxKtLm);
  }
  d->s2s.mSel = lmTerms ? ktEff : std::min(ktEff, K + 1);
  d->s2s.eosExtra = d->s2s.mSel < ktEff ? 1 : 0;
  d->s2s.cap = d->s2s.mSel + d->s2s.eosExtra;
  *nC = (int64_t)K * d->s2s.cap + K;
  if (d->lm->kind == 3) {
    return s2sPlanRowsLm(d, V);
  }
  return FLTX_OK;
}

static int s2sPlanLexicon(fltx_decoder* d, int32_t V, int64_t* nC) {
  const int K = d->s2s.opt.beam_size, Kt = d->s2s.opt.beam_size_token;
  const int ktEff = std::min(Kt, V);
  if (ktEff > kS2lMaxKt) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq lexicon: a token beam of %d (beam_size_token, V = %d) > %d", ktEff, V,
                kS2lMaxKt);
  }
  d->s2s.mSel = ktEff; /* the exact token beam: the trie and word scores make the score non-monotone in the model's */
  d->s2s.eosExtra = 0;
  d->s2s.cap = ktEff;
  *nC = (int64_t)K * ktEff * d->s2s.slots + K;
  if (*nC >= (int64_t)1 << 30) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq lexicon: %lld candidates per step", (long long)*nC);
  }
  d->s2s.mSize = s2lPow2AtLeast(2 * *nC);
  d->s2s.sMax = (int)std::min<int64_t>((int64_t)K * d->s2s.maxOut + 1, d->s2s.maxStates);
  d->s2s.sSize = s2lPow2AtLeast(2 * (int64_t)d->s2s.sMax);
  if (d->lm->kind == 3) { /* (the token beam's limit stays kS2lMaxKt: kS2sMaxKtLm is the lexicon-free step's) */
    return s2sPlanRowsLm(d, V);
  }
  if (d->lm->kind == 4) { /* (word ids, not tokens: checked against the trie's labels at create; nothing depends on V) */
    d->s2s.lmWidth = d->lm->rowsWidth;
    d->s2s.lmFinish = d->lm->rowsFinish;
  }
  return FLTX_OK;
}

static int s2sAllocLexicon(fltx_decoder* d, int32_t B, int32_t V, int64_t nC) {
  Stream st = d->ctx->stream;
  const size_t BC = (size_t)B * (size_t)nC;
  if (d->s2s.cScore.ensure(8 * BC, st, false) || d->s2s.cMk.ensure(16 * BC, st, false) ||
      d->s2s.cGrp.ensure(4 * BC, st, false) || d->s2s.cList.ensure(4 * BC, st, false) ||
      d->s2s.cNext.ensure(4 * BC, st, false) || d->s2s.mTab.ensure(4 * (size_t)B * d->s2s.mSize, st, false) ||
      d->s2s.sKey.ensure(8 * (size_t)B * d->s2s.sSize, st, false) ||
      d->s2s.sVal.ensure(4 * (size_t)B * d->s2s.sSize, st, false) || d->s2s.sCount.ensure(4 * (size_t)B, st, false) ||
      d->s2s.status.ensure(4 * (size_t)B, st, false) || d->s2s.merges.ensure(4 * (size_t)B, st, false)) {
    return fail(FLTX_ERR_OOM, "seq2seq lexicon workspace: device allocation failed (B=%d K=%d V=%d)", B,
                d->s2s.opt.beam_size, V);
  }
  if (devMemset(d->s2s.sKey.p, 0xFF, 8 * (size_t)B * d->s2s.sSize, st)) { /* the state tables: empty */
    return fail(FLTX_ERR_HIP, "seq2seq lexicon: memset failed");
  }
  return FLTX_OK;
}

int fltx_s2s_begin(fltx_decoder* d, int32_t B, int32_t V, int32_t* nextTok, int32_t* nextBeam, int32_t* nextSrc,
                   int32_t* nRows) {
  EntryScope entry(d, "fltx_s2s_begin", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (B < 1 || V < 1 || !nextTok || !nextBeam || !nextSrc || !nRows) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_begin: bad argument");
  }
  if (V > kS2sMaxV) {
    return fail(FLTX_ERR_UNSUPPORTED, "seq2seq: row width V = %d > %d", V, kS2sMaxV);
  }
  const bool lex = d->kind == FLTX_DECODER_S2S_LEXICON;
  int64_t nC = 0;
  int rc = lex ? s2sPlanLexicon(d, V, &nC) : s2sPlanLexFree(d, V, &nC);
  if (rc) {
    return rc;
  }
  Stream st = d->ctx->stream;
  const size_t BK = (size_t)B * d->s2s.opt.beam_size;
  const size_t hypBytes = lex ? sizeof(S2lHyp) : sizeof(S2sHyp), recBytes = lex ? sizeof(S2lRec) : sizeof(int2);
  if (d->s2s.beam.ensure(2 * BK * hypBytes, st, false) || d->s2s.beamN.ensure(8 * (size_t)B, st, false) ||
      d->s2s.hist.ensure((size_t)(d->s2s.maxOut + 1) * BK * recBytes, st, false) ||
      d->s2s.rowsInt.ensure(4 * (size_t)B, st, false) || d->s2s.done.ensure(4 * (size_t)B, st, false) ||
      d->s2s.finalStep.ensure(12 * (size_t)B, st, false) || /* (finalStep, origin, parked: s2sOrigin) */
      d->s2s.recTok.ensure(4 * BK * d->s2s.cap, st, false) || d->s2s.recAm.ensure(4 * BK * d->s2s.cap, st, false) ||
      d->s2s.recN.ensure(4 * BK, st, false) || d->s2s.cKey.ensure(8 * (size_t)B * (size_t)nC, st, false) ||
      (d->lm->kind == 3 && d->s2s.recLm.ensure(4 * BK * d->s2s.cap, st, false)) ||
      (d->lm->kind == 4 && (d->s2s.recLm.ensure(4 * BK * d->s2s.cap * d->s2s.slots, st, false) ||
                            d->s2s.rowNode.ensure(4 * BK, st, false)))) {
    return fail(FLTX_ERR_OOM, "seq2seq workspace: device allocation failed (B=%d K=%d V=%d)", B, d->s2s.opt.beam_size,
                V);
  }
  if (lex && (rc = s2sAllocLexicon(d, B, V, nC))) {
    return rc;
  }
  if (d->lm->kind == 4 && devMemset(d->s2s.rowNode.p, 0, 4 * BK, st)) { /* the first call's row: the root */
    return fail(FLTX_ERR_HIP, "seq2seq lexicon: memset failed");
  }
  d->B = B;
  d->N = V;
  d->s2s.t = 0;
  d->s2s.begun = true;
  d->s2s.hOrigin.assign((size_t)B, 0);
  d->s2s.hParked.assign((size_t)B, 0);
  d->s2s.liveUntil = d->s2s.maxOut;
  d->haveResults = false;
  d->ended = false;
  d->backtraced = false;
  d->resultsSynced = false;
  if (lex) {
    d->stateCap = (uint32_t)d->s2s.sMax;
  }
  S2lParams Q = s2sStepParams(d);
  S2sParams& P = Q.s;
  P.outTok = nextTok;
  P.outBeam = nextBeam;
  P.outSrc = nextSrc;
  P.outN = nRows;
  const int nGrid = (B + kS2sBeginThreads - 1) / kS2sBeginThreads;
  if (lex) {
    S2S_LAUNCH(fltx_s2s_lex_begin_kernel, s2lBeginUtterance, nGrid, kS2sBeginThreads, 0, st, Q);
  } else {
    S2S_LAUNCH(fltx_s2s_begin_kernel, s2sBeginUtterance, nGrid, kS2sBeginThreads, 0, st, P);
  }
  return FLTX_OK;
}

/* the LM's rows of fltx_s2s_step_lm_rows */
struct S2sLmIn {
  const void* scores;
  int32_t dtype;
  bool logits;
  int64_t rowStride;
  double* rowLse;
  /* fltx_s2s_step_word_lm_rows: word-level rows, read through lmRowOf (null: identity, nLmRows = B*K) */
  bool wordRows = false;
  const int32_t* lmRowOf = nullptr;
  int32_t nLmRows = 0;
  int32_t* nextWord = nullptr;
};

/* one step of either kind (the entry points have checked the decoder, `what` names the one that was called): the front
 * end the input asks for -- fltx_s2s_tokbeam_kernel for float log-probs, else the typed one (fltx_s2s.h: s2sTypedRows)
 * -- then, with a rows LM, the gather of the records' LM scores, then the kind's step kernel */
static int s2sStep(fltx_decoder* d, const char* what, const void* scores, int32_t dtype, bool logits, int32_t onDevice,
                   int64_t rowStride, const uint8_t* rowValid, double* rowLse, int32_t* nextTok, int32_t* nextBeam,
                   int32_t* nextSrc, int32_t* nRows, const S2sLmIn* lmIn = nullptr) {
  const bool wordRows = lmIn && lmIn->wordRows;
  if ((d->lm->kind == 4) != wordRows) {
    return fail(FLTX_ERR_STATE, wordRows ? "%s: the decoder has no word-level rows LM (fltx_lm_word_rows_create)"
                                         : "%s: a decoder with a word-level rows LM steps with fltx_s2s_step_word_lm_rows",
                what);
  }
  if (!wordRows && (d->lm->kind == 3) != (lmIn != nullptr)) {
    return fail(FLTX_ERR_STATE, lmIn ? "%s: the decoder has no rows LM (fltx_lm_rows_create)"
                                     : "%s: a decoder with a rows LM steps with fltx_s2s_step_lm_rows", what);
  }
  if (!d->s2s.begun) {
    return fail(FLTX_ERR_STATE, "%s: fltx_s2s_begin first", what);
  }
  const bool last = d->s2s.t >= d->s2s.liveUntil; /* no slot can be live: the kernels only list no rows */
  if (lmIn && ((!lmIn->scores && !last) || lmIn->rowStride < d->s2s.lmWidth)) {
    return fail(FLTX_ERR_INVALID, "%s: bad argument (lm_row_stride %lld, lm_width = %d)", what,
                (long long)lmIn->rowStride, d->s2s.lmWidth);
  }
  if (!nextTok || !nextBeam || !nextSrc || !nRows || (!scores && !last) || rowStride < d->N) {
    return fail(FLTX_ERR_INVALID, "%s: bad argument (row_stride %lld, V = %d)", what, (long long)rowStride, d->N);
  }
  const bool typed = dtype != FLTX_DTYPE_F32 || logits;
  if (typed && d->s2s.mSel > kS2sTypedMaxList) { /* (not reachable within the limits of fltx_s2s_begin) */
    return fail(FLTX_ERR_UNSUPPORTED, "%s: a token beam of %d > %d", what, d->s2s.mSel, kS2sTypedMaxList);
  }
  Stream st = d->ctx->stream;
  const size_t BK = (size_t)d->B * d->s2s.opt.beam_size;
  const size_t elem = s2sDtypeBytes(dtype);
  const size_t nLmRows = wordRows && lmIn->lmRowOf ? (size_t)std::max(lmIn->nLmRows, 0) : BK;
  if (wordRows && (!lmIn->nextWord || (lmIn->lmRowOf && lmIn->nLmRows < 1 && !last))) {
    return fail(FLTX_ERR_INVALID, "%s: bad argument (next_word is required; n_lm_rows %d with lm_row_of)", what,
                lmIn->nLmRows);
  }
  if (!onDevice && !last) {
    const size_t nE = (BK - 1) * (size_t)rowStride + (size_t)d->N;
    if (d->s2s.scores.ensure(elem * nE, st, false) || (rowValid && d->s2s.valid.ensure(BK, st, false))) {
      return fail(FLTX_ERR_OOM, "seq2seq: staging allocation failed");
    }
    if (devCopyH2D(d->s2s.scores.p, scores, elem * nE, st) ||
        (rowValid && devCopyH2D(d->s2s.valid.p, rowValid, BK, st))) {
      return fail(FLTX_ERR_HIP, "seq2seq: upload failed");
    }
    scores = d->s2s.scores.p;
    rowValid = rowValid ? d->s2s.valid.as<uint8_t>() : nullptr;
  }
  const void* lmScores = lmIn ? lmIn->scores : nullptr;
  const int32_t* lmRowOf = wordRows ? lmIn->lmRowOf : nullptr;
  int rc;
  if (lmIn && !onDevice && !last &&
      (rc = s2sStageLmRows(d, "seq2seq", lmIn->dtype, lmIn->rowStride, nLmRows, BK, &lmScores, &lmRowOf, st))) {
    return rc;
  }
  if (last && ((rc = s2sIdleLse(what, logits, rowLse, BK, st)) ||
               (lmIn && (rc = s2sIdleLse(what, lmIn->logits, lmIn->rowLse, BK, st))))) {
    return rc;
  }
  S2lParams Q = s2sStepParams(d);
  S2sParams& P = Q.s;
  P.scores = typed ? nullptr : (const float*)scores;
  P.rowStride = rowStride;
  P.rowValid = rowValid;
  P.outTok = nextTok;
  P.outBeam = nextBeam;
  P.outSrc = nextSrc;
  P.outN = nRows;
  if (!last && !typed) {
    S2S_LAUNCH(fltx_s2s_tokbeam_kernel, s2sTokBeamRows, (int)((BK + 3) / 4), 256, 4 * sizeof(S2sFrontLds), st, P);
  } else if (!last) {
    S2sTypedParams T;
    T.s = P;
    T.x = scores;
    T.rowLse = logits ? rowLse : nullptr;
    rc = s2sTypedDispatch(dtype, logits, [&](auto dt, auto lg) -> int {
      S2S_DT_LOGITS(dt, lg);
      if constexpr (DT != kS2sDtF32 || LOGITS) { /* (float32 log-probs are the untyped front end's: no such kernel) */
        S2S_LAUNCH((fltx_s2s_typed_kernel<DT, LOGITS>), (s2sTypedRows<DT, LOGITS>), (int)BK, kS2sTypedThreads,
                   sizeof(S2sTypedLds), st, T);
      }
      return FLTX_OK;
    });
    if (rc) {
      return rc;
    }
  }
  if (wordRows) {
    S2lWordLmParams W;
    memset(&W, 0, sizeof(W));
    W.r.s = P;
    s2sLmRowsFill(W.r, d, lmScores, lmIn->rowStride, lmIn->logits, lmIn->rowLse);
    W.trie = Q.trie;
    W.rowNode = d->s2s.rowNode.as<int32_t>();
    W.lmRowOf = lmRowOf;
    W.nLmRows = (int32_t)nLmRows;
    W.S = Q.S;
    if (!last && (rc = S2S_LM_ROWS_LAUNCH(fltx_s2s_lex_word_lm_rows_kernel, s2lWordLmRows, lmIn->dtype, lmIn->logits,
                                          (int)BK, st, W))) {
      return rc;
    }
    S2lWordLmStepParams RW;
    RW.q = Q;
    RW.recLm = W.r.recLm;
    RW.outWord = lmIn->nextWord;
    RW.rowNode = d->s2s.rowNode.as<int32_t>();
    S2S_LAUNCH(fltx_s2s_lex_step_word_lm_rows_kernel, s2lStepUtteranceWordLmRows, d->B, kS2sStepThreads,
               sizeof(S2lStepLds), st, RW);
  } else if (d->kind == FLTX_DECODER_S2S_LEXICON && !lmIn) {
    S2S_LAUNCH(fltx_s2s_lex_step_kernel, s2lStepUtterance, d->B, kS2sStepThreads, sizeof(S2lStepLds), st, Q);
  } else if (lmIn) {
    S2sLmRowsParams R;
    R.s = P;
    s2sLmRowsFill(R, d, lmScores, lmIn->rowStride, lmIn->logits, lmIn->rowLse);
    if (!last &&
        (rc = S2S_LM_ROWS_LAUNCH(fltx_s2s_lm_rows_kernel, s2sLmRows, lmIn->dtype, lmIn->logits, (int)BK, st, R))) {
      return rc;
    }
    if (d->kind == FLTX_DECODER_S2S_LEXICON) {
      S2lLmRowsParams RL;
      RL.q = Q;
      RL.recLm = R.recLm;
      S2S_LAUNCH(fltx_s2s_lex_step_lm_rows_kernel, s2lStepUtteranceLmRows, d->B, kS2sStepThreads, sizeof(S2lStepLds), st,
                 RL);
    } else {
      S2S_LAUNCH(fltx_s2s_step_lm_rows_kernel, s2sStepUtteranceLmRows, d->B, kS2sStepThreads, sizeof(S2sStepLds), st, R);
    }
  } else {
    S2S_LAUNCH(fltx_s2s_step_kernel, s2sStepUtterance, d->B, kS2sStepThreads, sizeof(S2sStepLds), st, P);
  }
  if (!last) {
    ++d->s2s.t;
  }
  return FLTX_OK;
}

int fltx_s2s_step(fltx_decoder* d, const float* scores, int32_t onDevice, int64_t rowStride, const uint8_t* rowValid,
                  int32_t* nextTok, int32_t* nextBeam, int32_t* nextSrc, int32_t* nRows) {
  EntryScope entry(d, "fltx_s2s_step", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  return s2sStep(d, "fltx_s2s_step", scores, FLTX_DTYPE_F32, false, onDevice, rowStride, rowValid, nullptr, nextTok,
                 nextBeam, nextSrc, nRows);
}

/* the model's rows as it produces them: fp16 / bf16 / f32, log-probs or raw logits */
int fltx_s2s_step_typed(fltx_decoder* d, const void* scores, int32_t dtype, int32_t kind, int32_t onDevice,
                        int64_t rowStride, const uint8_t* rowValid, double* rowLse, int32_t* nextTok,
                        int32_t* nextBeam, int32_t* nextSrc, int32_t* nRows) {
  EntryScope entry(d, "fltx_s2s_step_typed", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!s2sDtypeOk(dtype)) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_step_typed: dtype %d", dtype);
  }
  if (!s2sKindOk(kind)) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_step_typed: kind %d", kind);
  }
  return s2sStep(d, "fltx_s2s_step_typed", scores, dtype, kind == FLTX_S2S_LOGITS, onDevice, rowStride, rowValid,
                 rowLse, nextTok, nextBeam, nextSrc, nRows);
}

/* fltx_s2s_step_typed with the rows of a rows LM (fltx_lm_rows_create) next to the model's */
int fltx_s2s_step_lm_rows(fltx_decoder* d, const void* scores, int32_t dtype, int32_t kind, int64_t rowStride,
                          const void* lmScores, int32_t lmDtype, int32_t lmKind, int64_t lmRowStride, int32_t onDevice,
                          const uint8_t* rowValid, double* rowLse, double* lmRowLse, int32_t* nextTok,
                          int32_t* nextBeam, int32_t* nextSrc, int32_t* nRows) {
  EntryScope entry(d, "fltx_s2s_step_lm_rows", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (d->lm->kind != 3) {
    return fail(FLTX_ERR_STATE, "fltx_s2s_step_lm_rows: the decoder has no rows LM (fltx_lm_rows_create)");
  }
  if (!s2sDtypeOk(dtype) || !s2sDtypeOk(lmDtype)) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_step_lm_rows: dtype %d, lm_dtype %d", dtype, lmDtype);
  }
  if (!s2sKindOk(kind) || !s2sKindOk(lmKind)) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_step_lm_rows: kind %d, lm_kind %d", kind, lmKind);
  }
  const S2sLmIn lmIn{lmScores, lmDtype, lmKind == FLTX_S2S_LOGITS, lmRowStride, lmRowLse};
  return s2sStep(d, "fltx_s2s_step_lm_rows", scores, dtype, kind == FLTX_S2S_LOGITS, onDevice, rowStride, rowValid,
                 rowLse, nextTok, nextBeam, nextSrc, nRows, &lmIn);
}

/* fltx_s2s_step_lm_rows for a word-level rows LM (fltx_lm_word_rows_create): the LM's rows through lm_row_of */
int fltx_s2s_step_word_lm_rows(fltx_decoder* d, const void* scores, int32_t dtype, int32_t kind, int64_t rowStride,
                               const void* lmScores, int32_t lmDtype, int32_t lmKind, int64_t lmRowStride,
                               const int32_t* lmRowOf, int32_t nLmRows, int32_t onDevice, const uint8_t* rowValid,
                               double* rowLse, double* lmRowLse, int32_t* nextTok, int32_t* nextBeam, int32_t* nextSrc,
                               int32_t* nextWord, int32_t* nRows) {
  EntryScope entry(d, "fltx_s2s_step_word_lm_rows", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (d->lm->kind != 4) {
    return fail(FLTX_ERR_STATE, "fltx_s2s_step_word_lm_rows: the decoder has no word-level rows LM "
                                "(fltx_lm_word_rows_create)");
  }
  if (!s2sDtypeOk(dtype) || !s2sDtypeOk(lmDtype)) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_step_word_lm_rows: dtype %d, lm_dtype %d", dtype, lmDtype);
  }
  if (!s2sKindOk(kind) || !s2sKindOk(lmKind)) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_step_word_lm_rows: kind %d, lm_kind %d", kind, lmKind);
  }
  S2sLmIn lmIn{lmScores, lmDtype, lmKind == FLTX_S2S_LOGITS, lmRowStride, lmRowLse};
  lmIn.wordRows = true;
  lmIn.lmRowOf = lmRowOf;
  lmIn.nLmRows = nLmRows;
  lmIn.nextWord = nextWord;
  return s2sStep(d, "fltx_s2s_step_word_lm_rows", scores, dtype, kind == FLTX_S2S_LOGITS, onDevice, rowStride, rowValid,
                 rowLse, nextTok, nextBeam, nextSrc, nRows, &lmIn);
}

int fltx_s2s_done(fltx_decoder* d, int32_t* done) {
  EntryScope entry(d, "fltx_s2s_done", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!done) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_done: null argument");
  }
  if (!d->s2s.begun) {
    return fail(FLTX_ERR_STATE, "fltx_s2s_done: fltx_s2s_begin first");
  }
  if (d->s2s.t >= d->s2s.liveUntil) { /* every slot has had its max_output_length steps, or is parked */
    *done = 1;
    return FLTX_OK;
  }
  std::vector<int32_t> h((size_t)d->B);
  if (devCopyD2H(h.data(), d->s2s.done.p, 4 * (size_t)d->B, d->ctx->stream) || devSync(d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "fltx_s2s_done: copy failed: %s", devErr());
  }
  *done = 1;
  for (int32_t v : h) {
    *done = *done && v != 0;
  }
  return FLTX_OK;
}

int fltx_s2s_end(fltx_decoder* d) {
  EntryScope entry(d, "fltx_s2s_end", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d->s2s.begun) {
    return fail(FLTX_ERR_STATE, "fltx_s2s_end: fltx_s2s_begin first");
  }
  Stream st = d->ctx->stream;
  const int B = d->B, K = d->s2s.opt.beam_size, len = d->s2s.maxOut + 3;
  d->histOff.resize((size_t)B + 1);
  for (int b = 0; b <= B; ++b) {
    d->histOff[b] = (int64_t)b * K * len;
  }
  d->histRecords = (int64_t)B * K * len;
  S2lParams Q = s2sStepParams(d);
  S2sParams& P = Q.s;
  int rc = stepEndResults(d, "seq2seq", P);
  if (rc) {
    return rc;
  }
  const bool lex = d->kind == FLTX_DECODER_S2S_LEXICON;
  Q.words = lex ? d->words.as<int32_t>() : nullptr;
  if (lex) {
    S2S_LAUNCH(fltx_s2s_lex_end_kernel, s2lEndUtterance, B, kS2sEndThreads, 0, st, Q);
  } else {
    S2S_LAUNCH(fltx_s2s_end_kernel, s2sEndUtterance, B, kS2sEndThreads, 0, st, P);
  }
  stepEnded(d);
  return FLTX_OK;
}

/* ---- lexicon-free CTC with a rows LM (fltx_ctc_rows.h) ------------------------------------------------------------- */
static int crCheck(fltx_decoder* d, const char* what) {
  if (!d) {
    return fail(FLTX_ERR_INVALID, "%s: null decoder", what);
  }
  if (!isCrKind(d->kind)) {
    return fail(FLTX_ERR_STATE, "%s: not a CTC rows decoder (fltx_ctc_rows_decoder_create, "
                                "fltx_ctc_rows_lex_decoder_create)", what);
  }
  return FLTX_OK;
}

static CrParams crParams(fltx_decoder* d) {
  CrParams Q;
  memset(&Q, 0, sizeof(Q));
  S2sParams& P = Q.s;
  const int B = d->B;
  P.B = B;
  P.K = d->opt.beam_size;
  P.Kt = d->opt.beam_size_token;
  P.V = d->N;
  P.eos = -1;
  P.maxOut = std::numeric_limits<int32_t>::max();
  P.t = d->s2s.t;
  P.cap = d->s2s.cap;
  P.mSel = d->s2s.cap;
  P.beamThreshold = d->opt.beam_threshold;
  P.lmWeight = d->opt.lm_weight;
  P.beamN = d->s2s.beamN.as<int32_t>();
  P.nRowsInt = d->s2s.rowsInt.as<int32_t>();
  P.done = d->s2s.done.as<int32_t>();
  P.finalStep = d->s2s.finalStep.as<int32_t>();
  P.recTok = d->s2s.recTok.as<int32_t>();
  P.recAm = d->s2s.recAm.as<float>();
  P.recN = d->s2s.recN.as<int32_t>();
  P.cKey = d->s2s.cKey.as<unsigned long long>();
  P.nC = (int64_t)P.K * P.cap;
  P.outBeam = d->s2s.rowNode.as<int32_t>(); /* (the publisher's beam index: src_row - b*K here, nobody's output) */
  if (d->kind == FLTX_DECODER_LEX_CTC_ROWS) { /* (rowNode is the word gather's there) */
    P.nC = (int64_t)P.K * ((int64_t)P.cap * (1 + d->s2s.slots) + 2);
    P.outBeam = d->s2s.crOutBeam.as<int32_t>();
  }
  Q.sil = d->sil;
  Q.blank = d->blank;
  Q.logAdd = d->opt.log_add ? 1 : 0;
  Q.silScore = d->opt.sil_score;
  Q.frameOff = d->s2s.crMeta.as<int64_t>();
  Q.emOff = Q.frameOff + (B + 1);
  Q.T = (const int32_t*)(Q.emOff + B);
  Q.emissions = d->s2s.crEmisDev;
  Q.beam = d->s2s.beam.as<CrHyp>();
  Q.hist = d->s2s.hist.as<int2>();
  Q.cScore = d->s2s.cScore.as<double>();
  Q.cMk = d->s2s.cMk.as<uint4>();
  Q.cGrp = d->s2s.cGrp.as<int32_t>();
  Q.cList = d->s2s.cList.as<int32_t>();
  Q.cNext = d->s2s.cNext.as<int32_t>();
  Q.mTab = d->s2s.mTab.as<int32_t>();
  Q.mSize = d->s2s.mSize;
  Q.sKey = d->s2s.sKey.as<unsigned long long>();
  Q.sVal = d->s2s.sVal.as<int32_t>();
  Q.sCount = d->s2s.sCount.as<int32_t>();
  Q.sSize = d->s2s.sSize;
  Q.sMax = d->s2s.sMax;
  Q.status = d->s2s.status.as<int32_t>();
  Q.merges = d->s2s.merges.as<int32_t>();
  Q.recLm = d->s2s.recLm.as<float>();
  return Q;
}

/* the lexicon kind's parameters around those (fltx_ctc_rows_lex.h) */
static CrlParams crlParams(fltx_decoder* d, const CrParams& Q) {
  CrlParams R;
  memset(&R, 0, sizeof(R));
  R.c = Q;
  R.trie.maxScore = d->s2s.trieMax.as<float>();
  R.trie.kidOff = d->s2s.kidOff.as<int32_t>();
  R.trie.kidTok = d->s2s.kidTok.as<int32_t>();
  R.trie.kidNode = d->s2s.kidNode.as<int32_t>();
  R.trie.labOff = d->s2s.labOff.as<int32_t>();
  R.trie.labels = d->s2s.lab.as<int32_t>();
  R.S = d->s2s.slots;
  R.unk = d->opt.unk_score > -std::numeric_limits<double>::infinity() ? d->unk : -1;
  R.lmStride = d->s2s.isLmToken ? d->s2s.cap : d->s2s.cap * d->s2s.slots;
  R.wordScore = d->opt.word_score;
  R.unkScore = d->opt.unk_score;
  R.beam = d->s2s.beam.as<CrlHyp>();
  R.hist = d->s2s.hist.as<S2lRec>();
  R.rowNode = d->s2s.rowNode.as<int32_t>();
  R.words = d->words.as<int32_t>();
  return R;
}

int fltx_ctc_rows_lex_decoder_create(fltx_ctx* ctx, const fltx_options* opt, const fltx_htrie* trie, const fltx_lm* lm,
                                     int32_t sil, int32_t blank, int32_t unk, int32_t isLmToken, fltx_decoder** out) {
  if (!ctx || !opt || !trie || !lm || !out) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_lex_decoder_create: null argument");
  }
  if (lm->kind != (isLmToken ? 3 : 4)) {
    return fail(FLTX_ERR_UNSUPPORTED, "fltx_ctc_rows_lex_decoder_create: a word-level rows LM (fltx_lm_word_rows_create) "
                                      "with is_lm_token == 0, a token-level one (fltx_lm_rows_create) with is_lm_token "
                                      "!= 0; other LMs decode with fltx_decoder_create");
  }
  if (opt->criterion != FLTX_CRITERION_CTC) {
    return fail(FLTX_ERR_UNSUPPORTED, "fltx_ctc_rows_lex_decoder_create: criterion %d not supported (CTC only)",
                opt->criterion);
  }
  if (opt->beam_size < 1 || opt->beam_size_token < 1 || sil < 0 || blank < 0) {
    return fail(FLTX_ERR_INVALID, "beam_size and beam_size_token must be >= 1, sil and blank >= 0");
  }
  if (opt->beam_size > kS2sMaxBeam) {
    return fail(FLTX_ERR_UNSUPPORTED, "lexicon CTC rows: beam_size %d > %d", opt->beam_size, kS2sMaxBeam);
  }
  if (lm->rowsFinish < 0) { /* (CTC has no eos token whose entry finish could fall back to) */
    return fail(FLTX_ERR_INVALID, "lexicon CTC rows: the LM needs a finish_index >= 0");
  }
  if (opt->unk_score > -std::numeric_limits<double>::infinity() && unk < 0) { /* (the unknown word's id is listed and stored) */
    return fail(FLTX_ERR_INVALID, "lexicon CTC rows: unk_score > -inf needs an unk word id >= 0 (unk = %d)", unk);
  }
  EntryScope entry(ctx);
  if (entry.rc) {
    return entry.rc;
  }
  fltx_lm::Dev* lmDev = nullptr;
  int rc = lmEnsureUploaded(const_cast<fltx_lm*>(lm), ctx, &lmDev);
  if (rc) {
    return rc;
  }
  std::unique_ptr<fltx_decoder> d(new fltx_decoder());
  d->ctx = ctx;
  d->lm = lm;
  d->lmDev = lmDev;
  d->kind = FLTX_DECODER_LEX_CTC_ROWS;
  d->opt = *opt;
  d->sil = sil;
  d->blank = blank;
  d->unk = unk;
  d->isLmToken = isLmToken ? 1 : 0;
  d->s2s.isLmToken = isLmToken != 0;
  d->s2s.maxStates = kS2lDefaultStates;
  std::vector<int32_t> labels;
  if ((rc = s2lUploadTrie(d.get(), const_cast<fltx_htrie*>(trie), &labels))) {
    return rc;
  }
  if (lm->kind == 4) { /* every index the word gather can form lies inside the LM's rows */
    const int width = lm->rowsWidth;
    if (lm->rowsFinish >= width) {
      return fail(FLTX_ERR_INVALID, "lexicon CTC rows: finish index %d outside the LM's rows of %d", lm->rowsFinish, width);
    }
    if (opt->unk_score > -std::numeric_limits<double>::infinity()) {
      labels.push_back(unk);
    }
    for (int32_t w : labels) {
      if (w < 0 || (lm->rowsMap && w >= lm->nUsr)) {
        return fail(FLTX_ERR_INVALID, "lexicon CTC rows: word %d (a label of the trie, or unk) outside the %d entries of "
                                      "word_to_lm", w, lm->nUsr);
      }
      const int32_t idx = lm->rowsMap ? lm->hUsr[(size_t)w] : w;
      if (idx < 0 || idx >= width) {
        return fail(FLTX_ERR_INVALID, "lexicon CTC rows: word %d has LM index %d outside the LM's rows of %d", w, idx, width);
      }
    }
  }
  d->s2s.slots = std::max(1, d->s2s.maxLabels);
  *out = d.release();
  return FLTX_OK;
}

int fltx_ctc_rows_decoder_create(fltx_ctx* ctx, const fltx_options* opt, const fltx_lm* lm, int32_t sil, int32_t blank,
                                 fltx_decoder** out) {
  if (!ctx || !opt || !lm || !out) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_decoder_create: null argument");
  }
  if (lm->kind != 3) {
    return fail(FLTX_ERR_UNSUPPORTED, "fltx_ctc_rows_decoder_create: a token-level rows LM (fltx_lm_rows_create) only; "
                                      "other LMs decode with fltx_decoder_create");
  }
  if (opt->criterion != FLTX_CRITERION_CTC) {
    return fail(FLTX_ERR_UNSUPPORTED, "fltx_ctc_rows_decoder_create: criterion %d not supported (CTC only)",
                opt->criterion);
  }
  if (opt->beam_size < 1 || opt->beam_size_token < 1 || sil < 0 || blank < 0) {
    return fail(FLTX_ERR_INVALID, "beam_size and beam_size_token must be >= 1, sil and blank >= 0");
  }
  if (opt->beam_size > kS2sMaxBeam) {
    return fail(FLTX_ERR_UNSUPPORTED, "CTC rows: beam_size %d > %d", opt->beam_size, kS2sMaxBeam);
  }
  EntryScope entry(ctx);
  if (entry.rc) {
    return entry.rc;
  }
  fltx_lm::Dev* lmDev = nullptr;
  int rc = lmEnsureUploaded(const_cast<fltx_lm*>(lm), ctx, &lmDev);
  if (rc) {
    return rc;
  }
  auto* d = new fltx_decoder();
  d->ctx = ctx;
  d->lm = lm;
  d->lmDev = lmDev;
  d->kind = FLTX_DECODER_CTC_ROWS;
  d->opt = *opt;
  d->sil = sil;
  d->blank = blank;
  d->s2s.maxStates = kS2lDefaultStates;
  *out = d;
  return FLTX_OK;
}

static CrsParams crsParams(fltx_decoder* d) {
  CrsParams X;
  X.nDec = d->s2s.crCnt.as<int32_t>();
  X.base = X.nDec + d->B;
  X.ring = d->s2s.crRing;
  X.sHist = d->s2s.crSHist.as<double>();
  const size_t ids = (size_t)d->B * d->s2s.sMax;
  X.sPar = d->s2s.crIds.as<int32_t>();
  X.sEdge = X.sPar + ids;
  X.sFree = X.sEdge + ids;
  X.sFreeN = X.sFree + ids;
  return X;
}

/* the emissions of a begin or an append: float32 log-probs, frame after frame (dt == kCrEmPlain: fltx_ctc_rows_begin,
 * fltx_ctc_rows_stream_append), or typed frames (fltx_ctc_rows_begin_typed, fltx_ctc_rows_stream_append_typed) */
struct CrEmIn {
  const void* x = nullptr;
  int dt = kCrEmPlain; /* else a fltx_dtype */
  int kind = FLTX_S2S_LOG_PROBS;
  int64_t stride = 0;  /* elements between two frames; 0: N */
  double* frameLse = nullptr;
  size_t elem() const { return dt == kCrEmPlain || dt == FLTX_DTYPE_F32 ? 4 : 2; }
};

static int crEmCheck(const char* what, const CrEmIn& in) {
  if (in.dt != kCrEmPlain && !s2sDtypeOk(in.dt)) {
    return fail(FLTX_ERR_INVALID, "%s: dtype %d", what, in.dt);
  }
  if (!s2sKindOk(in.kind)) {
    return fail(FLTX_ERR_INVALID, "%s: kind %d", what, in.kind);
  }
  return FLTX_OK;
}

/* the frames on the device: a host buffer is copied, in its own type and with its own stride, utterance after utterance
 * (meta: frameOff[B + 1], emOff[B] as the kernels read them); then the decoder reads these emissions until the next
 * begin or append */
static int crEmStage(fltx_decoder* d, const char* what, const CrEmIn& in, int64_t stride, int32_t onDevice, bool packed,
                     const int64_t* offsets, const int32_t* T, int64_t frames, Stream st) {
  const int B = d->B, N = d->N;
  const std::vector<int64_t>& meta = d->s2s.crMetaHost;
  const void* x = in.x;
  if (!onDevice && frames > 0) {
    const size_t es = in.elem();
    char* dst = (char*)d->s2s.crEmis.p;
    const char* src = (const char*)in.x;
    int bad = 0;
    if (packed) { /* (the last frame ends after N elements, not after a stride) */
      bad = devCopyH2D(dst, src + es * (size_t)(offsets ? offsets[0] : 0), es * (size_t)((frames - 1) * stride + N), st);
    } else {
      for (int b = 0; b < B && !bad; ++b) {
        if (T[b] > 0) {
          bad = devCopyH2D(dst + es * (size_t)(meta[(size_t)b] * stride), src + es * (size_t)offsets[b],
                           es * (size_t)((int64_t)(T[b] - 1) * stride + N), st);
        }
      }
    }
    if (bad || devSync(st)) { /* (the caller's buffer is only borrowed for the call) */
      return fail(FLTX_ERR_HIP, "%s: emission upload failed", what);
    }
    x = dst;
  }
  d->s2s.crEmDt = in.dt;
  d->s2s.crEmLogits = in.kind == FLTX_S2S_LOGITS;
  d->s2s.crEmStride = stride;
  d->s2s.crEmX = x;
  d->s2s.crEmisDev = in.dt == kCrEmPlain ? (const float*)x : nullptr;
  return FLTX_OK;
}

static CrTypedEm crTypedEm(fltx_decoder* d) {
  CrTypedEm E;
  E.x = d->s2s.crEmX;
  E.stride = d->s2s.crEmStride;
  E.lse = d->s2s.crLse.as<double>();
  return E;
}

extern "C++" {
template <int DT, bool LOGITS>
static int crTypedFrontLaunch(fltx_decoder* d, int64_t frames, Stream st, const CrTypedParams& Z) {
  if (d->N <= d->s2s.crNarrowMax) {
    S2S_LAUNCH((fltx_ctc_rows_typed_wave_kernel<DT, LOGITS>), (crTypedWaveRows<DT, LOGITS>), (int)((frames + 3) / 4), 256,
               4 * sizeof(CrTypedWaveLds), st, Z);
  } else {
    S2S_LAUNCH((fltx_ctc_rows_typed_wg_kernel<DT, LOGITS>), (crTypedWgRows<DT, LOGITS>), (int)frames, kS2sTypedThreads,
               sizeof(S2sTypedLds), st, Z);
  }
  return FLTX_OK;
}
}

/* the token beams of the call's frames: one launch */
static int crFrontEnd(fltx_decoder* d, int64_t frames, Stream st, const CrParams& Q, double* frameLse) {
  if (d->s2s.crEmDt == kCrEmPlain) {
    S2S_LAUNCH(fltx_ctc_rows_tokbeam_kernel, crTokBeamRows, (int)((frames + 3) / 4), 256, 4 * sizeof(S2sFrontLds), st, Q);
    return FLTX_OK;
  }
  CrTypedParams Z;
  memset(&Z, 0, sizeof(Z));
  Z.c = Q;
  Z.e = crTypedEm(d);
  Z.lseOut = frameLse;
  return s2sTypedDispatch(d->s2s.crEmDt, d->s2s.crEmLogits, [&](auto dt, auto lg) -> int {
    S2S_DT_LOGITS(dt, lg);
    return crTypedFrontLaunch<DT, LOGITS>(d, frames, st, Z);
  });
}

/* the meta of a begin's utterances or of an append's chunk, as the kernels read it (crParams): frameOff[B + 1], emOff[B],
 * then T[B] as int32.  frames: the sum of T; packed: the utterances' emissions follow each other */
struct CrChunk {
  int64_t frames = 0;
  int maxT = 0;
  bool packed = true;
};
static int crChunkMeta(fltx_decoder* d, int B, const int32_t* T, const int64_t* offsets, int64_t stride, int32_t onDevice,
                       CrChunk* c) {
  std::vector<int64_t>& meta = d->s2s.crMetaHost;
  meta.assign((size_t)2 * B + 1 + ((size_t)B + 1) / 2, 0);
  int32_t* hT = (int32_t*)(meta.data() + 2 * (size_t)B + 1);
  for (int b = 0; b < B; ++b) {
    if (T[b] < 0) {
      return fail(FLTX_ERR_INVALID, "T[%d] = %d is negative", b, T[b]);
    }
    meta[(size_t)b] = c->frames;
    c->packed = c->packed && (!offsets || offsets[b] == c->frames * stride);
    meta[(size_t)B + 1 + b] = onDevice && offsets ? offsets[b] : c->frames * stride;
    hT[b] = T[b];
    c->frames += T[b];
    c->maxT = std::max(c->maxT, T[b]);
  }
  meta[(size_t)B] = c->frames;
  return FLTX_OK;
}

/* decodeBegin of a batch (maxFrames < 0: fltx_ctc_rows_begin, fltx_ctc_rows_begin_typed) or of B streams that hold up to
 * maxFrames frames each (fltx_ctc_rows_stream_begin; T: null) */
static int crBegin(fltx_decoder* d, const char* what, const CrEmIn& in, int32_t onDevice, const int64_t* offsets,
                   const int32_t* T, int32_t B, int32_t N, int32_t maxFrames, int32_t* nextTok, int32_t* nextSrc,
                   int32_t* nextState, int32_t* nRows) {
  EntryScope entry(d, what, crCheck);
  if (entry.rc) {
    return entry.rc;
  }
  int rc = crEmCheck(what, in);
  if (rc) {
    return rc;
  }
  const void* emissions = in.x;
  const bool stream = maxFrames >= 0;
  if (B < 1 || N < 1 || (!T && !stream) || (stream && maxFrames < 1) || !nextTok || !nextSrc || !nextState || !nRows) {
    return fail(FLTX_ERR_INVALID, "%s: bad argument", what);
  }
  std::vector<int32_t> noFrames;
  if (stream) { /* no frames yet: a chunk brings them (fltx_ctc_rows_stream_append) */
    noFrames.assign((size_t)B, 0);
    T = noFrames.data();
  }
  if (N > kS2sMaxV) {
    return fail(FLTX_ERR_UNSUPPORTED, "CTC rows: N = %d > %d", N, kS2sMaxV);
  }
  if (in.stride != 0 && in.stride < N) {
    return fail(FLTX_ERR_INVALID, "%s: frame_stride %lld < N = %d", what, (long long)in.stride, N);
  }
  const int64_t stride = in.stride ? in.stride : N;
  const int K = d->opt.beam_size, cap = std::min(d->opt.beam_size_token, N);
  if (cap > kS2lMaxKt) {
    return fail(FLTX_ERR_UNSUPPORTED, "CTC rows: a token beam of %d (beam_size_token, N = %d) > %d", cap, N, kS2lMaxKt);
  }
  if (d->sil >= N || d->blank >= N) {
    return fail(FLTX_ERR_RANGE, "sil index %d or blank index %d outside [0, %d)", d->sil, d->blank, N);
  }
  /* the LM's map and finish index against rows of this width (s2sPlanRowsLm's checks with N for V; CTC has no eos token
   * whose entry finish could fall back to) */
  d->s2s.eos = N;
  const bool lex = d->kind == FLTX_DECODER_LEX_CTC_ROWS;
  /* a stream's rings: the frames it may hold -- for the lexicon kind kLookBackLimit ON TOP of max_frames, as
   * fltx_stream_begin explains -- the root's row and the row the next step writes */
  const int sCap = stream ? maxFrames + (lex ? kLookBackLimit : 0) : 0, ring = sCap + 2;
  if (lex && d->lm->kind == 4) { /* (word ids, not tokens: checked against the trie's labels at create) */
    d->s2s.lmWidth = d->lm->rowsWidth;
  } else if ((rc = s2sPlanRowsLm(d, N)) || (rc = s2sRowsLmFinishCheck(d->lm->rowsFinish, d->s2s.lmWidth))) {
    return rc;
  }
  d->s2s.lmFinish = d->lm->rowsFinish;
  CrChunk chunk;
  if ((rc = crChunkMeta(d, B, T, offsets, stride, onDevice, &chunk))) {
    return rc;
  }
  const std::vector<int64_t>& meta = d->s2s.crMetaHost;
  const int64_t frames = chunk.frames;
  const int maxT = chunk.maxT;
  d->histOff.resize((size_t)B + 1);
  int64_t off = 0;
  for (int b = 0; b < B; ++b) {
    d->histOff[(size_t)b] = off;
    off += (int64_t)(stream ? ring : T[b] + 2) * K; /* (a stream's results: frames in buffer + 1 <= ring entries) */
  }
  d->histOff[(size_t)B] = off;
  d->histRecords = off;
  if (frames > 0 && !emissions) {
    return fail(FLTX_ERR_INVALID, "%s: null emissions", what);
  }
  const int64_t nC = lex ? (int64_t)K * ((int64_t)cap * (1 + d->s2s.slots) + 2) : (int64_t)K * cap;
  if (nC > (int64_t)1 << 29) { /* (the merge table holds the next power of two >= 2 nC slots, an int32 count) */
    return fail(FLTX_ERR_UNSUPPORTED, "%s: %lld candidates per frame", lex ? "lexicon CTC rows" : "CTC rows",
                (long long)nC);
  }
  const size_t hypBytes = lex ? sizeof(CrlHyp) : sizeof(CrHyp), recBytes = lex ? sizeof(S2lRec) : sizeof(int2);
  const size_t lmPerRow = (size_t)cap * (lex && !d->s2s.isLmToken ? d->s2s.slots : 1);
  d->s2s.cap = cap;
  d->s2s.mSize = s2lPow2AtLeast(2 * nC);
  d->s2s.sMax = stream ? d->s2s.maxStates : (int)std::min<int64_t>((int64_t)K * maxT + 2, d->s2s.maxStates);
  d->s2s.sSize = s2lPow2AtLeast(2 * (int64_t)d->s2s.sMax);
  Stream st = d->ctx->stream;
  const size_t BK = (size_t)B * K, BC = (size_t)B * (size_t)nC, nF = (size_t)std::max<int64_t>(frames, 1);
  if (d->s2s.beam.ensure(2 * BK * hypBytes, st, false) || d->s2s.beamN.ensure(8 * (size_t)B, st, false) ||
      d->s2s.hist.ensure((size_t)(stream ? ring : maxT + 2) * BK * recBytes, st, false) ||
      (stream && (d->s2s.crCnt.ensure(8 * (size_t)B, st, false) || d->s2s.crSHist.ensure((size_t)ring * BK * 24, st, false) ||
                  d->s2s.crIds.ensure(4 * (size_t)B * (3 * (size_t)d->s2s.sMax + 1), st, false) ||
                  (d->s2s.sMax > kCrsLdsIds &&
                   d->s2s.crMarks.ensure(8 * (size_t)B * (((size_t)d->s2s.sMax + 31) / 32), st, false)))) ||
      (lex && d->s2s.crOutBeam.ensure(4 * BK, st, false)) ||
      d->s2s.rowsInt.ensure(4 * (size_t)B, st, false) || d->s2s.done.ensure(4 * (size_t)B, st, false) ||
      d->s2s.finalStep.ensure(4 * (size_t)B, st, false) || d->s2s.recTok.ensure(4 * nF * cap, st, false) ||
      d->s2s.recAm.ensure(4 * nF * cap, st, false) || d->s2s.recN.ensure(4 * nF, st, false) ||
      d->s2s.cKey.ensure(8 * BC, st, false) || d->s2s.recLm.ensure(4 * BK * lmPerRow, st, false) ||
      d->s2s.rowNode.ensure(4 * BK, st, false) || d->s2s.cScore.ensure(8 * BC, st, false) ||
      d->s2s.cMk.ensure(16 * BC, st, false) || d->s2s.cGrp.ensure(4 * BC, st, false) ||
      d->s2s.cList.ensure(4 * BC, st, false) || d->s2s.cNext.ensure(4 * BC, st, false) ||
      d->s2s.mTab.ensure(4 * (size_t)B * d->s2s.mSize, st, false) ||
      d->s2s.sKey.ensure(8 * (size_t)B * d->s2s.sSize, st, false) ||
      d->s2s.sVal.ensure(4 * (size_t)B * d->s2s.sSize, st, false) || d->s2s.sCount.ensure(4 * (size_t)B, st, false) ||
      d->s2s.status.ensure(4 * (size_t)B, st, false) || d->s2s.merges.ensure(4 * (size_t)B, st, false) ||
      d->s2s.crMeta.ensure(8 * meta.size(), st, false) ||
      (!onDevice && d->s2s.crEmis.ensure(in.elem() * nF * (size_t)stride, st, false)) ||
      (in.kind == FLTX_S2S_LOGITS && d->s2s.crLse.ensure(8 * nF, st, false))) {
    return fail(FLTX_ERR_OOM, "CTC rows workspace: device allocation failed (B=%d K=%d N=%d, %lld frames)", B, K, N,
                (long long)frames);
  }
  if (devMemset(d->s2s.sKey.p, 0xFF, 8 * (size_t)B * d->s2s.sSize, st) || /* the state tables: empty */
      devCopyH2D(d->s2s.crMeta.p, meta.data(), 8 * meta.size(), st)) {
    return fail(FLTX_ERR_HIP, "CTC rows: upload failed");
  }
  d->B = B;
  d->N = N;
  if ((rc = crEmStage(d, what, in, stride, onDevice, chunk.packed, offsets, T, frames, st))) {
    return rc;
  }
  d->s2s.t = 0;
  d->s2s.crMaxT = maxT;
  d->s2s.crFrames = frames;
  d->s2s.begun = true;
  d->s2s.crStream = stream;
  d->s2s.crCap = sCap;
  d->s2s.crRing = ring;
  d->s2s.crBestLb = -1;
  d->s2s.crBuf.assign(stream ? (size_t)B : 0, 0);
  d->s2s.plOn = false; /* (planning ends with the decode it was begun for: fltx_ctc_rows_plan_begin) */
  d->haveResults = false;
  d->ended = false;
  d->backtraced = false;
  d->resultsSynced = false;
  d->stateCap = (uint32_t)d->s2s.sMax;
  CrParams Q = crParams(d);
  Q.s.outTok = nextTok;
  Q.s.outSrc = nextSrc;
  Q.s.outN = nRows;
  Q.outState = nextState;
  if (stream) {
    const int grid = (B + kS2sBeginThreads - 1) / kS2sBeginThreads;
    if (lex) {
      const CrlStreamParams Z = {crlParams(d, Q), crsParams(d)};
      S2S_LAUNCH(fltx_ctc_rows_lex_stream_begin_kernel, crlsBeginStream, grid, kS2sBeginThreads, 0, st, Z);
    } else {
      const CrStreamParams Z = {Q, crsParams(d)};
      S2S_LAUNCH(fltx_ctc_rows_stream_begin_kernel, crsBeginStream, grid, kS2sBeginThreads, 0, st, Z);
    }
    return FLTX_OK;
  }
  if (frames > 0 && (rc = crFrontEnd(d, frames, st, Q, in.frameLse))) {
    return rc;
  }
  if (lex) {
    const CrlParams R = crlParams(d, Q);
    S2S_LAUNCH(fltx_ctc_rows_lex_begin_kernel, crlBeginUtterance, (B + kS2sBeginThreads - 1) / kS2sBeginThreads,
               kS2sBeginThreads, 0, st, R);
    return FLTX_OK;
  }
  S2S_LAUNCH(fltx_ctc_rows_begin_kernel, crBeginUtterance, (B + kS2sBeginThreads - 1) / kS2sBeginThreads,
             kS2sBeginThreads, 0, st, Q);
  return FLTX_OK;
}

int fltx_ctc_rows_begin(fltx_decoder* d, const float* emissions, int32_t onDevice, const int64_t* offsets,
                        const int32_t* T, int32_t B, int32_t N, int32_t* nextTok, int32_t* nextSrc, int32_t* nextState,
                        int32_t* nRows) {
  CrEmIn in;
  in.x = emissions;
  return crBegin(d, "fltx_ctc_rows_begin", in, onDevice, offsets, T, B, N, -1, nextTok, nextSrc, nextState, nRows);
}

int fltx_ctc_rows_begin_typed(fltx_decoder* d, const void* emissions, int32_t dtype, int32_t kind, int32_t onDevice,
                              const int64_t* offsets, int64_t frameStride, const int32_t* T, int32_t B, int32_t N,
                              double* frameLse, int32_t* nextTok, int32_t* nextSrc, int32_t* nextState, int32_t* nRows) {
  CrEmIn in;
  in.x = emissions;
  in.dt = dtype == kCrEmPlain ? -2 : dtype; /* (no dtype of the ABI means "plain") */
  in.kind = kind;
  in.stride = frameStride;
  in.frameLse = frameLse;
  return crBegin(d, "fltx_ctc_rows_begin_typed", in, onDevice, offsets, T, B, N, -1, nextTok, nextSrc, nextState, nRows);
}

int fltx_ctc_rows_stream_begin(fltx_decoder* d, int32_t B, int32_t N, int32_t maxFrames, int32_t* nextTok,
                               int32_t* nextSrc, int32_t* nextState, int32_t* nRows) {
  if (maxFrames < 1) {
    DeviceScope devScope(d ? d->ctx : nullptr);
    int rc = crCheck(d, "fltx_ctc_rows_stream_begin");
    return rc ? rc : fail(FLTX_ERR_INVALID, "fltx_ctc_rows_stream_begin: max_frames = %d (>= 1)", maxFrames);
  }
  return crBegin(d, "fltx_ctc_rows_stream_begin", CrEmIn(), 1, nullptr, nullptr, B, N, maxFrames, nextTok, nextSrc,
                 nextState, nRows);
}

/* the LM rows of a step or of the end (fin): checked, staged when they are the host's, and gathered into recLm */
static int crLmRowsIn(fltx_decoder* d, const char* what, bool fin, bool idle, const void* lmScores, int32_t lmDtype,
                      int32_t lmKind, int64_t lmRowStride, const int32_t* lmRowOf, int32_t nLmRows, int32_t onDevice,
                      double* lmRowLse, const CrParams& Q) {
  if (!s2sDtypeOk(lmDtype)) {
    return fail(FLTX_ERR_INVALID, "%s: lm_dtype %d", what, lmDtype);
  }
  if (!s2sKindOk(lmKind)) {
    return fail(FLTX_ERR_INVALID, "%s: lm_kind %d", what, lmKind);
  }
  if ((!lmScores && !idle) || lmRowStride < d->s2s.lmWidth || (lmRowOf && nLmRows < 1 && !idle)) {
    return fail(FLTX_ERR_INVALID, "%s: bad argument (lm_row_stride %lld, lm_width = %d, n_lm_rows %d)", what,
                (long long)lmRowStride, d->s2s.lmWidth, nLmRows);
  }
  Stream st = d->ctx->stream;
  const size_t BK = (size_t)d->B * d->opt.beam_size;
  const bool logits = lmKind == FLTX_S2S_LOGITS;
  if (idle) { /* nothing to score */
    return s2sIdleLse(what, logits, lmRowLse, BK, st);
  }
  const size_t nLm = lmRowOf ? (size_t)nLmRows : BK;
  int rc;
  if (!onDevice && (rc = s2sStageLmRows(d, what, lmDtype, lmRowStride, nLm, BK, &lmScores, &lmRowOf, st))) {
    return rc;
  }
  CrLmParams W;
  memset(&W, 0, sizeof(W));
  W.r.s = Q.s;
  s2sLmRowsFill(W.r, d, lmScores, lmRowStride, logits, lmRowLse);
  W.T = Q.T;
  W.frameOff = Q.frameOff;
  W.lmRowOf = lmRowOf;
  W.nLmRows = (int32_t)nLm;
  W.fin = fin ? 1 : 0;
  if (d->kind == FLTX_DECODER_LEX_CTC_ROWS && !d->s2s.isLmToken) { /* a word LM: the entries of the labels (fltx_ctc_rows_lex.h) */
    const CrlParams R = crlParams(d, Q);
    CrlWordLmParams X;
    memset(&X, 0, sizeof(X));
    X.w = W;
    X.trie = R.trie;
    X.rowNode = R.rowNode;
    X.S = R.S;
    X.unk = R.unk;
    return S2S_LM_ROWS_LAUNCH(fltx_ctc_rows_lex_word_lm_kernel, crlWordLmRows, lmDtype, logits, (int)BK, st, X);
  }
  return S2S_LM_ROWS_LAUNCH(fltx_ctc_rows_lm_kernel, crLmRows, lmDtype, logits, (int)BK, st, W);
}

/* a launch of the lexicon kind that is an instantiation per LM level: `launch` names the level SRC */
#define CRL_BY_LM_LEVEL(d, launch)          \
  if ((d)->s2s.isLmToken) {                 \
    constexpr int SRC = kCrlLmTokenRows;    \
    launch;                                 \
  } else {                                  \
    constexpr int SRC = kCrlLmWordRows;     \
    launch;                                 \
  }

/* the lexicon kind's frame step on typed emissions (fltx_ctc_rows_typed.h): an instantiation per (LM level, dtype, kind) */
extern "C++" {
template <int SRC>
static int crlTypedStep(fltx_decoder* d, const CrParams& Q) {
  return s2sTypedDispatch(d->s2s.crEmDt, d->s2s.crEmLogits, [&](auto dt, auto lg) -> int {
    S2S_DT_LOGITS(dt, lg);
    if (d->s2s.crStream) {
      const CrlTypedStreamParams Y = {crlParams(d, Q), crsParams(d), crTypedEm(d)};
      S2S_LAUNCH((fltx_ctc_rows_lex_typed_stream_step_kernel<SRC, DT, LOGITS>), (crlsStepStreamTyped<SRC, DT, LOGITS>),
                 d->B, kS2sStepThreads, sizeof(CrlStepLds), d->ctx->stream, Y);
    } else {
      const CrlTypedParams Y = {crlParams(d, Q), crTypedEm(d)};
      S2S_LAUNCH((fltx_ctc_rows_lex_typed_step_kernel<SRC, DT, LOGITS>), (crlStepTyped<SRC, DT, LOGITS>), d->B,
                 kS2sStepThreads, sizeof(CrlStepLds), d->ctx->stream, Y);
    }
    return FLTX_OK;
  });
}
}

int fltx_ctc_rows_step(fltx_decoder* d, const void* lmScores, int32_t lmDtype, int32_t lmKind, int64_t lmRowStride,
                       const int32_t* lmRowOf, int32_t nLmRows, int32_t onDevice, double* lmRowLse, int32_t* nextTok,
                       int32_t* nextSrc, int32_t* nextState, int32_t* nRows) {
  EntryScope entry(d, "fltx_ctc_rows_step", crCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d->s2s.begun) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_step: fltx_ctc_rows_begin first");
  }
  if (!nextTok || !nextSrc || !nextState || !nRows) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_step: null output");
  }
  const bool last = d->s2s.t >= d->s2s.crMaxT; /* every utterance's frames are used up: the beams are listed again */
  CrParams Q = crParams(d);
  Q.s.outTok = nextTok;
  Q.s.outSrc = nextSrc;
  Q.s.outN = nRows;
  Q.outState = nextState;
  int rc = crLmRowsIn(d, "fltx_ctc_rows_step", false, last, lmScores, lmDtype, lmKind, lmRowStride, lmRowOf, nLmRows,
                      onDevice, lmRowLse, Q);
  if (rc) {
    return rc;
  }
  d->s2s.crBestLb = -1;
  if (d->kind == FLTX_DECODER_LEX_CTC_ROWS && d->s2s.crEmDt != kCrEmPlain) {
    if ((rc = d->s2s.isLmToken ? crlTypedStep<kCrlLmTokenRows>(d, Q) : crlTypedStep<kCrlLmWordRows>(d, Q))) {
      return rc;
    }
  } else if (d->s2s.crStream) { /* the same step on the streams' own counts (fltx_ctc_rows_stream.h) */
    if (d->kind == FLTX_DECODER_LEX_CTC_ROWS) {
      const CrlStreamParams Z = {crlParams(d, Q), crsParams(d)};
      CRL_BY_LM_LEVEL(d, S2S_LAUNCH(fltx_ctc_rows_lex_stream_step_kernel<SRC>, (crlsStepStream<SRC, false>), d->B,
                                    kS2sStepThreads, sizeof(CrlStepLds), d->ctx->stream, Z));
    } else {
      const CrStreamParams Z = {Q, crsParams(d)};
      S2S_LAUNCH(fltx_ctc_rows_stream_step_kernel, crsStepStream<false>, d->B, kS2sStepThreads, sizeof(S2lStepLds),
                 d->ctx->stream, Z);
    }
  } else if (d->kind == FLTX_DECODER_LEX_CTC_ROWS) {
    const CrlParams R = crlParams(d, Q);
    CRL_BY_LM_LEVEL(d, S2S_LAUNCH(fltx_ctc_rows_lex_step_kernel<SRC>, (crlStepUtterance<SRC, false>), d->B, kS2sStepThreads,
                                  sizeof(CrlStepLds), d->ctx->stream, R));
  } else {
    S2S_LAUNCH(fltx_ctc_rows_step_kernel, crStepUtterance<false>, d->B, kS2sStepThreads, sizeof(S2lStepLds),
               d->ctx->stream, Q);
  }
  if (!last) {
    ++d->s2s.t;
  }
  d->s2s.plSkipped = d->s2s.plSkipped || d->s2s.plFresh; /* (the list before this one was never planned) */
  d->s2s.plFresh = true;
  return FLTX_OK;
}

int fltx_ctc_rows_end(fltx_decoder* d, const void* lmScores, int32_t lmDtype, int32_t lmKind, int64_t lmRowStride,
                      const int32_t* lmRowOf, int32_t nLmRows, int32_t onDevice, double* lmRowLse) {
  EntryScope entry(d, "fltx_ctc_rows_end", crCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d->s2s.begun) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_end: fltx_ctc_rows_begin first");
  }
  Stream st = d->ctx->stream;
  const int B = d->B;
  CrParams Q = crParams(d);
  int rc = stepEndResults(d, "CTC rows", Q.s);
  if (rc || (rc = crLmRowsIn(d, "fltx_ctc_rows_end", true, false, lmScores, lmDtype, lmKind, lmRowStride, lmRowOf,
                             nLmRows, onDevice, lmRowLse, Q))) {
    return rc;
  }
  Q.histOff = d->histOffD.as<int64_t>();
  if (d->s2s.crStream) { /* (frames in buffer + 1 entries per hypothesis: what is left of the stream, and decodeEnd's sil) */
    if (d->kind == FLTX_DECODER_LEX_CTC_ROWS) {
      const CrlStreamParams Z = {crlParams(d, Q), crsParams(d)};
      CRL_BY_LM_LEVEL(d, S2S_LAUNCH(fltx_ctc_rows_lex_stream_end_kernel<SRC>, (crlsStepStream<SRC, true>), B,
                                    kS2sStepThreads, sizeof(CrlStepLds), st, Z));
    } else {
      const CrStreamParams Z = {Q, crsParams(d)};
      S2S_LAUNCH(fltx_ctc_rows_stream_end_kernel, crsStepStream<true>, B, kS2sStepThreads, sizeof(S2lStepLds), st, Z);
    }
    d->s2s.crStream = false; /* the stream is over: its results are read as a batch's */
    d->s2s.begun = false;
    d->s2s.crBestLb = -1;
  } else if (d->kind == FLTX_DECODER_LEX_CTC_ROWS) {
    const CrlParams R = crlParams(d, Q);
    CRL_BY_LM_LEVEL(d, S2S_LAUNCH(fltx_ctc_rows_lex_end_kernel<SRC>, (crlStepUtterance<SRC, true>), B, kS2sStepThreads,
                                  sizeof(CrlStepLds), st, R));
  } else {
    S2S_LAUNCH(fltx_ctc_rows_end_kernel, crStepUtterance<true>, B, kS2sStepThreads, sizeof(S2lStepLds), st, Q);
  }
  stepEnded(d);
  return FLTX_OK;
}

/* ---- streams on the CTC rows kinds (fltx_ctc_rows_stream.h) ----------------------------------------------------------- */
static int crsCheck(fltx_decoder* d, const char* what) {
  int rc = crCheck(d, what);
  if (rc) {
    return rc;
  }
  if (!d->s2s.begun || !d->s2s.crStream) {
    return fail(FLTX_ERR_STATE, "%s: no open stream (fltx_ctc_rows_stream_begin first)", what);
  }
  return FLTX_OK;
}

/* {nDec[B], base[B]} as the device has them: the frames each stream really holds */
static int crsReadCounts(fltx_decoder* d, std::vector<int32_t>& cnt) {
  cnt.resize(2 * (size_t)d->B);
  if (devCopyD2H(cnt.data(), d->s2s.crCnt.p, 4 * cnt.size(), d->ctx->stream) || devSync(d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "CTC rows stream: copy failed");
  }
  return FLTX_OK;
}

static int crsAppend(fltx_decoder* d, const char* what, const CrEmIn& in, int32_t onDevice, const int64_t* offsets,
                     const int32_t* T) {
  EntryScope entry(d, what, crsCheck);
  if (entry.rc) {
    return entry.rc;
  }
  int rc = crEmCheck(what, in);
  if (rc) {
    return rc;
  }
  if (!T) {
    return fail(FLTX_ERR_INVALID, "%s: bad argument", what);
  }
  const void* emissions = in.x;
  const int B = d->B, N = d->N, cap = d->s2s.cap;
  if (in.stride != 0 && in.stride < N) {
    return fail(FLTX_ERR_INVALID, "%s: frame_stride %lld < N = %d", what, (long long)in.stride, N);
  }
  const int64_t stride = in.stride ? in.stride : N;
  for (int b = 0; b < B; ++b) {
    if (T[b] < 0) {
      return fail(FLTX_ERR_INVALID, "T[%d] = %d is negative", b, T[b]);
    }
  }
  if (d->s2s.t < d->s2s.crMaxT) {
    return fail(FLTX_ERR_STATE, "%s: %d frames of the previous chunk are unstepped (fltx_ctc_rows_step)", what,
                d->s2s.crMaxT - d->s2s.t);
  }
  std::vector<int32_t>& buf = d->s2s.crBuf;
  for (int pass = 0; pass < 2; ++pass) {
    int bad = -1;
    for (int b = 0; b < B && bad < 0; ++b) {
      if (buf[(size_t)b] + T[b] > d->s2s.crCap) {
        bad = b;
      }
    }
    if (bad < 0) {
      break;
    }
    if (pass == 0) { /* the host's count is an upper bound (a prune of the lexicon kind, a stream that stopped) */
      std::vector<int32_t> cnt;
      if ((rc = crsReadCounts(d, cnt))) {
        return rc;
      }
      for (int b = 0; b < B; ++b) {
        buf[(size_t)b] = cnt[(size_t)b] - cnt[(size_t)B + b];
      }
      continue;
    }
    const bool lex = d->kind == FLTX_DECODER_LEX_CTC_ROWS;
    return fail(FLTX_ERR_RANGE, "stream %d: %d buffered + %d new frames exceed max_frames %d%s", bad, buf[(size_t)bad],
                T[bad], d->s2s.crCap - (lex ? kLookBackLimit : 0),
                lex ? " + 100 (a lexicon stream's prune keeps the frames back to the last complete word, up to lookBack + "
                      "100, Utils.h:28,293-308)"
                    : "");
  }
  CrChunk chunk; /* (the meta is the CHUNK's from here on) */
  if ((rc = crChunkMeta(d, B, T, offsets, stride, onDevice, &chunk))) {
    return rc;
  }
  const std::vector<int64_t>& meta = d->s2s.crMetaHost;
  const int64_t frames = chunk.frames;
  if (frames > 0 && !emissions) {
    return fail(FLTX_ERR_INVALID, "%s: null emissions", what);
  }
  Stream st = d->ctx->stream;
  const size_t nF = (size_t)std::max<int64_t>(frames, 1);
  if (d->s2s.recTok.ensure(4 * nF * cap, st, false) || d->s2s.recAm.ensure(4 * nF * cap, st, false) ||
      d->s2s.recN.ensure(4 * nF, st, false) ||
      (!onDevice && d->s2s.crEmis.ensure(in.elem() * nF * (size_t)stride, st, false)) ||
      (in.kind == FLTX_S2S_LOGITS && d->s2s.crLse.ensure(8 * nF, st, false))) {
    return fail(FLTX_ERR_OOM, "CTC rows stream: device allocation failed (%lld frames)", (long long)frames);
  }
  if (devCopyH2D(d->s2s.crMeta.p, meta.data(), 8 * meta.size(), st)) {
    return fail(FLTX_ERR_HIP, "CTC rows stream: upload failed");
  }
  if ((rc = crEmStage(d, what, in, stride, onDevice, chunk.packed, offsets, T, frames, st))) { /* (a host chunk is copied here) */
    return rc;
  }
  d->s2s.t = 0;
  d->s2s.crMaxT = chunk.maxT;
  d->s2s.crFrames = frames;
  d->s2s.crBestLb = -1;
  for (int b = 0; b < B; ++b) {
    buf[(size_t)b] += T[b];
  }
  if (frames > 0) {
    return crFrontEnd(d, frames, st, crParams(d), in.frameLse);
  }
  return FLTX_OK;
}

int fltx_ctc_rows_stream_append(fltx_decoder* d, const float* emissions, int32_t onDevice, const int64_t* offsets,
                                const int32_t* T) {
  CrEmIn in;
  in.x = emissions;
  return crsAppend(d, "fltx_ctc_rows_stream_append", in, onDevice, offsets, T);
}

int fltx_ctc_rows_stream_append_typed(fltx_decoder* d, const void* emissions, int32_t dtype, int32_t kind,
                                      int32_t onDevice, const int64_t* offsets, int64_t frameStride, const int32_t* T,
                                      double* frameLse) {
  CrEmIn in;
  in.x = emissions;
  in.dt = dtype == kCrEmPlain ? -2 : dtype; /* (no dtype of the ABI means "plain") */
  in.kind = kind;
  in.stride = frameStride;
  in.frameLse = frameLse;
  return crsAppend(d, "fltx_ctc_rows_stream_append_typed", in, onDevice, offsets, T);
}

static CrsOpParams crsOpParams(fltx_decoder* d, int lookBack) {
  CrsOpParams W;
  memset(&W, 0, sizeof(W));
  W.B = d->B;
  W.K = d->opt.beam_size;
  W.lookBack = lookBack;
  W.maxLen = d->s2s.crRing;
  W.beamN = d->s2s.beamN.as<int32_t>();
  W.status = d->s2s.status.as<int32_t>();
  W.x = crsParams(d);
  W.beam = d->s2s.beam.p;
  W.hist = d->s2s.hist.p;
  W.bestLen = d->bestLen.as<int32_t>();
  W.bestScores = d->bestScores.as<double>();
  W.bestTok = d->bestTok.as<int32_t>();
  W.bestWrd = d->bestWrd.as<int32_t>();
  return W;
}

int fltx_ctc_rows_stream_prune(fltx_decoder* d, int32_t lookBack) {
  EntryScope entry(d, "fltx_ctc_rows_stream_prune", crsCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (lookBack < 0) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_stream_prune: look_back = %d", lookBack);
  }
  const CrsOpParams W = crsOpParams(d, lookBack);
  if (d->kind == FLTX_DECODER_LEX_CTC_ROWS) {
    S2S_LAUNCH(fltx_ctc_rows_stream_prune_kernel<true>, crsPrune<true>, d->B, kCrsOpThreads, sizeof(CrsOpLds),
               d->ctx->stream, W);
  } else {
    S2S_LAUNCH(fltx_ctc_rows_stream_prune_kernel<false>, crsPrune<false>, d->B, kCrsOpThreads, sizeof(CrsOpLds),
               d->ctx->stream, W);
  }
  d->s2s.crBestLb = -1;
  /* what stays buffered, without asking the device: look_back frames (every lexicon-free hypothesis is complete), up to
   * kLookBackLimit more for the lexicon kind; a prune that does nothing leaves no more than that either */
  const int keep = lookBack + (d->kind == FLTX_DECODER_LEX_CTC_ROWS ? kLookBackLimit : 0);
  /* (a prune between append and the chunk's last step sees only the frames stepped so far: the chunk's unstepped frames
   * -- T[b] of the chunk's meta less the steps taken -- arrive afterwards and stay on top of the bound) */
  const int32_t* chunkT = (const int32_t*)(d->s2s.crMetaHost.data() + 2 * (size_t)d->B + 1);
  for (int b = 0; b < d->B; ++b) {
    const int pending = std::max(0, chunkT[b] - d->s2s.t);
    const int stepped = d->s2s.crBuf[(size_t)b] - pending;
    d->s2s.crBuf[(size_t)b] = (stepped - lookBack >= 1 ? std::min(stepped, keep) : stepped) + pending;
  }
  return FLTX_OK;
}

int fltx_ctc_rows_stream_collect(fltx_decoder* d, int32_t releaseCap, int32_t* released, int32_t* nReleased,
                                 int32_t* nLive) {
  EntryScope entry(d, "fltx_ctc_rows_stream_collect", crsCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (releaseCap < 1 || !released || !nReleased) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_stream_collect: release_cap = %d (>= 1), null released or n_released",
                releaseCap);
  }
  CrsCollectParams W;
  memset(&W, 0, sizeof(W));
  W.B = d->B;
  W.K = d->opt.beam_size;
  W.sMax = d->s2s.sMax;
  W.sSize = d->s2s.sSize;
  W.releaseCap = releaseCap;
  W.beamN = d->s2s.beamN.as<int32_t>();
  W.done = d->s2s.done.as<int32_t>();
  W.x = crsParams(d);
  W.beam = d->s2s.beam.p;
  W.sKey = d->s2s.sKey.as<unsigned long long>();
  W.sVal = d->s2s.sVal.as<int32_t>();
  W.sCount = d->s2s.sCount.as<int32_t>();
  W.marks = d->s2s.sMax > kCrsLdsIds ? d->s2s.crMarks.as<uint32_t>() : nullptr;
  W.released = released;
  W.nReleased = nReleased;
  W.nLive = nLive;
  if (d->kind == FLTX_DECODER_LEX_CTC_ROWS) {
    S2S_LAUNCH(fltx_ctc_rows_stream_collect_kernel<true>, crsCollect<true>, d->B, kCrsOpThreads, sizeof(CrsCollectLds),
               d->ctx->stream, W);
  } else {
    S2S_LAUNCH(fltx_ctc_rows_stream_collect_kernel<false>, crsCollect<false>, d->B, kCrsOpThreads, sizeof(CrsCollectLds),
               d->ctx->stream, W);
  }
  ++d->s2s.plCollects; /* (a planner must hear of it: fltx_ctc_rows_plan_release) */
  return FLTX_OK;
}

int fltx_ctc_rows_stream_frames_in_buffer(fltx_decoder* d, int32_t b, int32_t* n) {
  EntryScope entry(d, "fltx_ctc_rows_stream_frames_in_buffer", crsCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!n || b < 0 || b >= d->B) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_stream_frames_in_buffer: bad argument");
  }
  std::vector<int32_t> cnt;
  int rc = crsReadCounts(d, cnt);
  if (rc) {
    return rc;
  }
  *n = cnt[(size_t)b] - cnt[(size_t)d->B + b] + 1; /* nDecodedFramesInBuffer: the buffer's first frame counts */
  return FLTX_OK;
}

/* fltx_result_best inside a stream of a CTC rows decoder: getBestHypothesis(lookBack) of all B streams in one launch,
 * kept until the next step, append or prune */
static int crsResultBest(fltx_decoder* d, int32_t b, int32_t lookBack, double* scores, int32_t* tokens, int32_t* words,
                  int32_t capacity, int32_t* length) {
  Stream st = d->ctx->stream;
  const int B = d->B, maxLen = d->s2s.crRing;
  const bool lex = d->kind == FLTX_DECODER_LEX_CTC_ROWS;
  if (d->s2s.crBestLb != lookBack) {
    if (d->bestLen.ensure(8 * (size_t)B, st, false) || d->bestScores.ensure(24 * (size_t)B, st, false) ||
        d->bestTok.ensure(4 * (size_t)B * maxLen, st, false) || d->bestWrd.ensure(4 * (size_t)B * maxLen, st, false)) {
      return fail(FLTX_ERR_OOM, "best-hypothesis buffers: allocation failed");
    }
    const CrsOpParams W = crsOpParams(d, lookBack);
    if (lex) {
      S2S_LAUNCH(fltx_ctc_rows_stream_best_kernel<true>, crsBest<true>, B, 64, sizeof(CrsOpLds), st, W);
    } else {
      S2S_LAUNCH(fltx_ctc_rows_stream_best_kernel<false>, crsBest<false>, B, 64, sizeof(CrsOpLds), st, W);
    }
    /* the lengths, statuses and scores of all B streams cross once per launch; a call then copies its tokens alone */
    d->s2s.crBestLen.resize(2 * (size_t)B);
    d->s2s.crBestScores.resize(3 * (size_t)B);
    if (devCopyD2H(d->s2s.crBestLen.data(), d->bestLen.p, 8 * (size_t)B, st) ||
        devCopyD2H(d->s2s.crBestScores.data(), d->bestScores.p, 24 * (size_t)B, st)) {
      return fail(FLTX_ERR_HIP, "copy failed");
    }
    d->s2s.crBestLb = lookBack;
  }
  const int32_t len = d->s2s.crBestLen[(size_t)b], status = d->s2s.crBestLen[(size_t)B + b];
  if (status & ST_TABLE_FULL) {
    return fail(FLTX_ERR_UNSUPPORTED, "utterance %d: LM-state table full (cap=%u)", b, d->stateCap);
  }
  *length = len;
  if (len == 0) {
    return FLTX_OK; /* an empty DecodeResult */
  }
  if (len > capacity) {
    return fail(FLTX_ERR_RANGE, "fltx_result_best: capacity %d < length %d", capacity, len);
  }
  if (scores) {
    memcpy(scores, d->s2s.crBestScores.data() + 3 * (size_t)b, 24);
  }
  if ((tokens && devCopyD2H(tokens, d->bestTok.as<int32_t>() + (size_t)b * maxLen, 4 * (size_t)len, st)) ||
      (words && lex && devCopyD2H(words, d->bestWrd.as<int32_t>() + (size_t)b * maxLen, 4 * (size_t)len, st))) {
    return fail(FLTX_ERR_HIP, "copy failed");
  }
  if (words && !lex) {
    std::fill(words, words + len, -1); /* LexiconFreeDecoder.h:80-82 */
  }
  return FLTX_OK;
}

/* ---- the LM rows of the CTC rows decoders, planned on the device (fltx_ctc_rows_plan.h) ------------------------------- */
static CpParams cpParams(fltx_decoder* d) {
  CpParams P;
  memset(&P, 0, sizeof(P));
  P.B = d->B;
  P.K = d->opt.beam_size;
  P.sMax = d->s2s.sMax;
  P.rowCap = d->s2s.plRowCap;
  P.metaPar = d->s2s.plMetaPar;
  P.prevPar = d->s2s.plPrevPar;
  P.rowOf = d->s2s.plRowOf.as<int32_t>();
  P.freeRows = d->s2s.plFree.as<int32_t>();
  P.meta = d->s2s.plMeta.as<int32_t>();
  P.prev = d->s2s.plPrev.as<int32_t>();
  P.cnt = d->s2s.plCnt.as<int32_t>();
  P.rank = d->s2s.plRank.as<int32_t>();
  return P;
}

int fltx_ctc_rows_plan_begin(fltx_decoder* d, int32_t rowCapacity) {
  EntryScope entry(d, "fltx_ctc_rows_plan_begin", crCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d->s2s.begun || d->ended) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_plan_begin: fltx_ctc_rows_begin or fltx_ctc_rows_stream_begin first");
  }
  if (rowCapacity < 1) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_plan_begin: row_capacity = %d (>= 1)", rowCapacity);
  }
  Stream st = d->ctx->stream;
  const size_t B = (size_t)d->B, BK = B * (size_t)d->opt.beam_size, nIds = B * (size_t)d->s2s.sMax;
  if (d->s2s.plRowOf.ensure(4 * nIds, st, false) || d->s2s.plFree.ensure(4 * (size_t)rowCapacity, st, false) ||
      d->s2s.plMeta.ensure(32, st, false) || d->s2s.plPrev.ensure(8 * BK, st, false) ||
      d->s2s.plCnt.ensure(4 * B, st, false) || d->s2s.plRank.ensure(4 * BK, st, false)) {
    return fail(FLTX_ERR_OOM, "fltx_ctc_rows_plan_begin: device allocation failed (B=%d, %d states, %d rows)", d->B,
                d->s2s.sMax, rowCapacity);
  }
  if (devMemset(d->s2s.plRowOf.p, 0xFF, 4 * nIds, st) || devMemset(d->s2s.plPrev.p, 0xFF, 8 * BK, st) ||
      devMemset(d->s2s.plMeta.p, 0, 32, st)) {
    return fail(FLTX_ERR_HIP, "fltx_ctc_rows_plan_begin: clearing the tables failed");
  }
  d->s2s.plOn = true;
  d->s2s.plFresh = true; /* the begin's list (or the last step's) */
  d->s2s.plSkipped = false;
  d->s2s.plRowCap = rowCapacity;
  d->s2s.plMetaPar = 0;
  d->s2s.plPrevPar = 0;
  d->s2s.plCollects = 0;
  return FLTX_OK;
}

int fltx_ctc_rows_plan(fltx_decoder* d, const int32_t* nextTok, const int32_t* nextSrc, const int32_t* nextState,
                       const int32_t* nRows, int32_t* lmRowOf, int32_t* newRow, int32_t* newParentRow, int32_t* newEdge,
                       int32_t* newDecRow, int32_t* counts) {
  EntryScope entry(d, "fltx_ctc_rows_plan", crCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d->s2s.plOn) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_plan: fltx_ctc_rows_plan_begin first (after the decode's begin)");
  }
  if (!nextTok || !nextSrc || !nextState || !nRows || !lmRowOf || !newRow || !newParentRow || !newEdge || !newDecRow ||
      !counts) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_plan: null argument");
  }
  if (d->s2s.plSkipped) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_plan: a step was queued whose list was never planned (the parent rows "
                                "of this list are unknown)");
  }
  if (!d->s2s.plFresh) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_plan: this list has been planned already");
  }
  if (d->s2s.plCollects > 0) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_plan: fltx_ctc_rows_plan_release first (%d fltx_ctc_rows_stream_collect "
                                "since the last plan)", d->s2s.plCollects);
  }
  CpParams P = cpParams(d);
  P.tok = nextTok;
  P.src = nextSrc;
  P.state = nextState;
  P.nRows = nRows;
  P.lmRowOf = lmRowOf;
  P.newRow = newRow;
  P.newParent = newParentRow;
  P.newEdge = newEdge;
  P.newDecRow = newDecRow;
  P.counts = counts;
  S2S_LAUNCH(fltx_ctc_rows_plan_mark_kernel, cpMark, d->B, kCpThreads, sizeof(CpLds), d->ctx->stream, P);
  S2S_LAUNCH(fltx_ctc_rows_plan_assign_kernel, cpAssign, d->B, kCpThreads, sizeof(CpLds), d->ctx->stream, P);
  d->s2s.plMetaPar ^= 1;
  d->s2s.plPrevPar ^= 1;
  d->s2s.plFresh = false;
  return FLTX_OK;
}

int fltx_ctc_rows_plan_release(fltx_decoder* d, const int32_t* released, const int32_t* nReleased, int32_t releaseCap) {
  EntryScope entry(d, "fltx_ctc_rows_plan_release", crsCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d->s2s.plOn) {
    return fail(FLTX_ERR_STATE, "fltx_ctc_rows_plan_release: fltx_ctc_rows_plan_begin first");
  }
  if (!released || !nReleased || releaseCap < 1) {
    return fail(FLTX_ERR_INVALID, "fltx_ctc_rows_plan_release: release_cap = %d (>= 1), null released or n_released",
                releaseCap);
  }
  CpParams P = cpParams(d);
  P.released = released;
  P.nReleased = nReleased;
  P.releaseCap = releaseCap;
  S2S_LAUNCH(fltx_ctc_rows_plan_release_count_kernel, cpReleaseCount, d->B, kCpThreads, sizeof(CpLds), d->ctx->stream, P);
  S2S_LAUNCH(fltx_ctc_rows_plan_release_kernel, cpRelease, d->B, kCpThreads, sizeof(CpLds), d->ctx->stream, P);
  d->s2s.plMetaPar ^= 1;
  d->s2s.plCollects = std::max(0, d->s2s.plCollects - 1);
  return FLTX_OK;
}

/* ---- finish and restart single streams (fltx_ctc_rows_stream.h) --------------------------------------------------------- */
int fltx_ctc_rows_stream_finish(fltx_decoder* d, const int32_t* which, const void* lmScores, int32_t lmDtype,
                                int32_t lmKind, int64_t lmRowStride, const int32_t* lmRowOf, int32_t nLmRows,
                                int32_t onDevice, double* lmRowLse, int32_t* nextTok, int32_t* nextSrc,
                                int32_t* nextState, int32_t* nRows, int32_t resultsOnDevice, fltx_finished_out* out) {
  const char* what = "fltx_ctc_rows_stream_finish";
  EntryScope entry(d, what, crsCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!which || !nextTok || !nextSrc || !nextState || !nRows || !out) {
    return fail(FLTX_ERR_INVALID, "%s: null which, list or out", what);
  }
  if (d->s2s.t < d->s2s.crMaxT) {
    return fail(FLTX_ERR_STATE, "%s: %d frames of the last chunk are unstepped (fltx_ctc_rows_step)", what,
                d->s2s.crMaxT - d->s2s.t);
  }
  if (d->s2s.plOn && d->s2s.plCollects > 0) {
    return fail(FLTX_ERR_STATE, "%s: fltx_ctc_rows_plan_release first (%d fltx_ctc_rows_stream_collect since the last "
                                "plan)", what, d->s2s.plCollects);
  }
  Stream st = d->ctx->stream;
  const int B = d->B;
  const bool lex = d->kind == FLTX_DECODER_LEX_CTC_ROWS;
  bool named = false;
  for (int b = 0; b < B; ++b) {
    named = named || which[b] != 0;
  }
  const size_t nRec = (size_t)std::max<int64_t>(d->histRecords, 1), inBytes = 12 * (size_t)B;
  int rc = stepFinishBuffers(d, what, nRec, 12 * (size_t)B, inBytes, 4 * (size_t)B, resultsOnDevice);
  if (rc) {
    return rc;
  }
  char* stage = (char*)d->s2s.finStage.acquire(inBytes);
  if (!stage) {
    return fail(FLTX_ERR_OOM, "%s: staging allocation failed", what);
  }
  memcpy(stage, d->histOff.data(), 8 * (size_t)B);
  int32_t* stWhich = (int32_t*)(stage + 8 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    stWhich[b] = which[b] != 0 ? 1 : 0;
  }
  if (devCopyH2D(d->s2s.finIn.p, stage, inBytes, st) || d->s2s.finStage.sent(st)) {
    return fail(FLTX_ERR_HIP, "%s: upload failed", what);
  }
  int32_t* meta = d->s2s.finMeta.as<int32_t>();
  CrParams Q = crParams(d);
  Q.s.outTok = nextTok;
  Q.s.outSrc = nextSrc;
  Q.s.outN = nRows;
  Q.outState = nextState;
  Q.histOff = d->s2s.finIn.as<int64_t>();
  s2sSetResults(Q.s, {d->s2s.finScores.as<double>(), d->s2s.finTok.as<int32_t>(), meta, meta, meta + B,
                      meta + 2 * (size_t)B});
  CrsFinishParams F;
  memset(&F, 0, sizeof(F));
  F.which = (const int32_t*)(Q.histOff + B);
  F.skip = d->s2s.finSkip.as<int32_t>();
  F.errUnsupported = FLTX_ERR_UNSUPPORTED;
  F.errState = FLTX_ERR_STATE;
  const CrFinishParams Z = {Q, crsParams(d), F};
  if (named) { /* the finish entries of the named streams' rows, of those alone */
    S2S_LAUNCH(fltx_ctc_rows_stream_finish_mask_kernel, crsFinishMask, (B + kS2sBeginThreads - 1) / kS2sBeginThreads,
               kS2sBeginThreads, 0, st, Z);
    CrParams G = Q;
    G.s.done = F.skip;
    if ((rc = crLmRowsIn(d, what, true, false, lmScores, lmDtype, lmKind, lmRowStride, lmRowOf, nLmRows, onDevice,
                         lmRowLse, G))) {
      return rc;
    }
    if (d->s2s.plOn) { /* their LM rows back to the planner, while the ids' count still stands */
      CpFinishParams R;
      memset(&R, 0, sizeof(R));
      R.p = cpParams(d);
      R.which = F.which;
      R.sCount = Q.sCount;
      S2S_LAUNCH(fltx_ctc_rows_plan_finish_count_kernel, cpFinishCount, B, kCpThreads, sizeof(CpLds), st, R);
      S2S_LAUNCH(fltx_ctc_rows_plan_finish_release_kernel, cpFinishRelease, B, kCpThreads, sizeof(CpLds), st, R);
      d->s2s.plMetaPar ^= 1;
    }
  }
  if (lex) {
    CrlFinishParams Y = {crlParams(d, Q), Z.x, F};
    Y.r.words = d->s2s.finWrd.as<int32_t>();
    CRL_BY_LM_LEVEL(d, S2S_LAUNCH(fltx_ctc_rows_lex_stream_finish_kernel<SRC>, crlsFinishStream<SRC>, B, kS2sStepThreads,
                                  sizeof(CrlStepLds), st, Y));
  } else {
    S2S_LAUNCH(fltx_ctc_rows_stream_finish_kernel, crsFinishStream, B, kS2sStepThreads, sizeof(S2lStepLds), st, Z);
  }
  d->s2s.crBestLb = -1;
  for (int b = 0; b < B; ++b) {
    if (which[b] != 0) {
      d->s2s.crBuf[(size_t)b] = 0;
    }
  }
  d->s2s.plSkipped = d->s2s.plSkipped || d->s2s.plFresh; /* (the list before this one was never planned) */
  d->s2s.plFresh = true;
  memset(out, 0, sizeof(*out));
  out->row_off = resultsOnDevice ? Q.histOff : d->histOff.data();
  /* (home: n_hyp * length entries of each named stream) */
  return stepFinishResults(d, what, resultsOnDevice, d->histOff.data(), 0, &fltx_finished_out::length, out);
}

/* ---- finish and restart single streams of a classic stream batch (fltx_stream_finish.h) ------------------------------- */
int fltx_stream_finish(fltx_decoder* d, const int32_t* which, int32_t resultsOnDevice, fltx_finished_out* out) {
  const char* what = "fltx_stream_finish";
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (d && stepKindCalls(d->kind)) {
    return fail(FLTX_ERR_STATE, "%s: %s", what, stepKindCalls(d->kind));
  }
  if (!d || !which || !out) {
    return fail(FLTX_ERR_INVALID, "%s: null decoder, which or out", what);
  }
  if (!d->streaming || d->ended) {
    return fail(FLTX_ERR_STATE, "%s: no open stream (fltx_stream_begin first)", what);
  }
  if (d->lm->kind == 2) {
    /* (a host LM's states are the callee's, and its start / retain protocol is per decoder: left for later) */
    return fail(FLTX_ERR_UNSUPPORTED, "%s: a decoder with a host LM (fltx_lm_host_create) ends and begins all its streams "
                                      "together (fltx_stream_end, fltx_stream_begin)", what);
  }
  /* what fltx_stream_end settles first: the look at a pending chunk, its second pass, the prune deferred behind it */
  int rc = settleStream(d);
  if (rc) {
    return rc;
  }
  Stream st = d->ctx->stream;
  const int B = d->B;
  const bool lex = d->kind == FLTX_DECODER_LEXICON;
  std::vector<int32_t> named;
  for (int b = 0; b < B; ++b) {
    if (which[b] != 0) {
      named.push_back(b);
    }
  }
  const int n = (int)named.size();
  const size_t nRec = (size_t)std::max<int64_t>(d->histRecords, 1), inBytes = 8 * (size_t)B;
  if ((rc = stepFinishBuffers(d, what, nRec, 12 * (size_t)B, inBytes, 4 * (size_t)B, resultsOnDevice))) {
    return rc;
  }
  int32_t* meta = d->s2s.finMeta.as<int32_t>();
  if (n == 0) { /* nobody is named: the counts say so, nothing else happens */
    if (devMemset(meta, 0, 12 * (size_t)B, st)) {
      return fail(FLTX_ERR_HIP, "%s: memset failed", what);
    }
  } else {
    int32_t* stage = (int32_t*)d->s2s.finStage.acquire(inBytes); /* the named streams, then the B flags */
    if (!stage) {
      return fail(FLTX_ERR_OOM, "%s: staging allocation failed", what);
    }
    for (int b = 0; b < B; ++b) {
      stage[b] = b < n ? named[(size_t)b] : 0;
      stage[B + b] = which[b] != 0 ? 1 : 0;
    }
    if (devCopyH2D(d->s2s.finIn.p, stage, inBytes, st) || d->s2s.finStage.sent(st)) {
      return fail(FLTX_ERR_HIP, "%s: upload failed", what);
    }
    const int32_t* dNamed = d->s2s.finIn.as<int32_t>();
    /* decodeEnd of the named streams: fltx_stream_end's launch over the list, the n-best's scores into the finish's own */
    DecodeParams P;
    fillParams(d, P);
    std::vector<int32_t> zeroT((size_t)B, 0);
    if ((rc = uploadStep(d, nullptr, 1, nullptr, zeroT.data(), P))) {
      return rc;
    }
    P.doBegin = 0;
    P.doEnd = 1;
    P.hlmFrame = 1 << 30;
    P.uttMap = dNamed;
    P.outScores = d->s2s.finScores.as<double>();
    P.outN = d->s2s.finSkip.as<int32_t>(); /* (the count is read where fltx_result_count reads it: uttNBeam) */
    d->nLaunch = n;
    rc = launchDecode(d, P);
    d->nLaunch = 0;
    if (rc) {
      return rc;
    }
    SfParams F;
    memset(&F, 0, sizeof(F));
    F.B = B;
    F.K = d->opt.beam_size;
    F.lex = lex ? 1 : 0;
    F.nNamed = n;
    F.errState = FLTX_ERR_STATE;
    F.errUnsupported = FLTX_ERR_UNSUPPORTED;
    F.named = dNamed;
    F.which = dNamed + B;
    F.histPT = d->histPT.as<int2>();
    F.histW = d->histW.as<int32_t>();
    F.histOff = d->histOffD.as<int64_t>();
    F.uttFrame = d->uttFrame.as<int32_t>();
    F.uttNBeam = d->uttNBeam.as<int32_t>();
    F.uttStatus = d->uttStatus.as<int32_t>();
    F.nHyp = meta;
    F.length = meta + B;
    F.status = meta + 2 * (size_t)B;
    F.tokens = d->s2s.finTok.as<int32_t>();
    F.words = lex ? d->s2s.finWrd.as<int32_t>() : nullptr;
    S2S_LAUNCH(fltx_stream_finish_kernel, sfFinishStream, n, kSfThreads, sizeof(SfLds), st, F);
    /* the slots start over: what launchCompact(d, 0) and a new epoch give a new batch of streams, for these alone */
    SfRestartParams R;
    memset(&R, 0, sizeof(R));
    R.nNamed = n;
    R.named = dNamed;
    R.idCap = d->idCap;
    R.stateCap = d->stateCap;
    const bool counted = d->lean && !d->slane; /* (prepare(): which family's buffers exist) */
    R.idPar = d->recycle ? d->idPar.as<uint32_t>() : nullptr;
    R.uttNextId = (counted || d->recycle) ? d->uttNextId.as<int32_t>() : nullptr;
    R.maskTab = counted ? d->maskTab.as<unsigned long long>() : nullptr;
    R.stateTab = (d->lean || d->tlane) ? nullptr : d->stateTab.as<unsigned long long>();
    R.stateVal = (!counted && d->recycle) ? d->stateVal.as<uint32_t>() : nullptr;
    R.lmCache = d->useLmCache ? d->lmCache.as<unsigned long long>() : nullptr;
    R.uttFirst = d->uttFirst.as<int64_t>();
    S2S_LAUNCH(fltx_stream_restart_kernel, sfRestartStream, n, kSfThreads, 0, st, R);
    /* decodeBegin of the named streams: fltx_stream_begin's launch over the list */
    P.doBegin = 1;
    P.doEnd = 0;
    d->nLaunch = n;
    rc = launchDecode(d, P);
    d->nLaunch = 0;
    if (rc) {
      return rc;
    }
    for (int b : named) {
      d->frames[(size_t)b] = 0; /* (exact, whatever the prunes since the last look left of the others' bounds) */
    }
    d->resultsSynced = false;
    d->backtraced = false;
    d->hostFetched = false;
    d->compactFetched = false;
    d->scoresFetched = false;
  }
  memset(out, 0, sizeof(*out));
  out->row_off = resultsOnDevice ? d->histOffD.as<int64_t>() : d->histOff.data();
  /* (home: n_hyp * length entries of each named stream) */
  return stepFinishResults(d, what, resultsOnDevice, d->histOff.data(), 0, &fltx_finished_out::length, out);
}

/* ---- seq2seq: finish and restart single utterances of a running batch (fltx_s2s.h: s2sFinishSlot) ---------------------- */
int fltx_s2s_done_each(fltx_decoder* d, int32_t* done) {
  EntryScope entry(d, "fltx_s2s_done_each", s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!done) {
    return fail(FLTX_ERR_INVALID, "fltx_s2s_done_each: null argument");
  }
  if (!d->s2s.begun) {
    return fail(FLTX_ERR_STATE, "fltx_s2s_done_each: fltx_s2s_begin first");
  }
  if (devCopyD2H(done, d->s2s.done.p, 4 * (size_t)d->B, d->ctx->stream) || devSync(d->ctx->stream)) {
    return fail(FLTX_ERR_HIP, "fltx_s2s_done_each: copy failed: %s", devErr());
  }
  for (int b = 0; b < d->B; ++b) {
    done[b] = done[b] != 0 ? 1 : 0;
  }
  return FLTX_OK;
}

int fltx_s2s_finish(fltx_decoder* d, const int32_t* which, int32_t* nextTok, int32_t* nextBeam, int32_t* nextSrc,
                    int32_t* nRows, int32_t* nextWord, int32_t resultsOnDevice, fltx_s2s_finished_out* out) {
  const char* what = "fltx_s2s_finish";
  EntryScope entry(d, what, s2sCheck);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d->s2s.begun || d->ended) {
    return fail(FLTX_ERR_STATE, "%s: between fltx_s2s_begin and fltx_s2s_end", what);
  }
  if (!which || !nextTok || !nextBeam || !nextSrc || !nRows || !out) {
    return fail(FLTX_ERR_INVALID, "%s: null which, list or out", what);
  }
  const bool wordRows = d->lm->kind == 4;
  if (wordRows && !nextWord) {
    return fail(FLTX_ERR_INVALID, "%s: a decoder with a word-level rows LM lists next_word", what);
  }
  const int B = d->B, K = d->s2s.opt.beam_size, len = d->s2s.maxOut + 3;
  for (int b = 0; b < B; ++b) {
    if (which[b] < 0 || which[b] > 2) {
      return fail(FLTX_ERR_INVALID, "%s: which[%d] = %d (0 leave, 1 finish + restart, 2 finish + park)", what, b, which[b]);
    }
  }
  Stream st = d->ctx->stream;
  const bool lex = d->kind == FLTX_DECODER_S2S_LEXICON;
  int rc = stepFinishBuffers(d, what, (size_t)B * K * len, 20 * (size_t)B, 4 * (size_t)B, 0, resultsOnDevice);
  if (rc) {
    return rc;
  }
  int32_t* stage = (int32_t*)d->s2s.finStage.acquire(4 * (size_t)B);
  if (!stage) {
    return fail(FLTX_ERR_OOM, "%s: staging allocation failed", what);
  }
  memcpy(stage, which, 4 * (size_t)B);
  if (devCopyH2D(d->s2s.finIn.p, stage, 4 * (size_t)B, st) || d->s2s.finStage.sent(st)) {
    return fail(FLTX_ERR_HIP, "%s: upload failed", what);
  }
  int32_t* meta = d->s2s.finMeta.as<int32_t>(); /* n_hyp, steps, status, then the back-trace's beam and frame counts */
  S2lFinishKernelParams Z;
  memset(&Z, 0, sizeof(Z));
  Z.q = s2sStepParams(d);
  Z.q.words = lex ? d->s2s.finWrd.as<int32_t>() : nullptr;
  S2sParams& P = Z.q.s;
  P.outTok = nextTok;
  P.outBeam = nextBeam;
  P.outSrc = nextSrc;
  P.outN = nRows;
  s2sSetResults(P, {d->s2s.finScores.as<double>(), d->s2s.finTok.as<int32_t>(), meta, meta + 3 * (size_t)B,
                    meta + 4 * (size_t)B, meta + 2 * (size_t)B});
  Z.f.which = d->s2s.finIn.as<int32_t>();
  Z.f.steps = meta + B;
  Z.f.errUnsupported = FLTX_ERR_UNSUPPORTED;
  Z.outWord = wordRows ? nextWord : nullptr;
  Z.rowNode = wordRows ? d->s2s.rowNode.as<int32_t>() : nullptr;
  if (lex) {
    S2S_LAUNCH(fltx_s2s_lex_finish_kernel, s2lFinishUtterance, B, kS2sEndThreads, sizeof(S2sFinishLds), st, Z);
  } else {
    const S2sFinishKernelParams Y = {P, Z.f};
    S2S_LAUNCH(fltx_s2s_finish_kernel, s2sFinishUtterance, B, kS2sEndThreads, sizeof(S2sFinishLds), st, Y);
  }
  /* what the host knows of the slots from here on */
  for (int b = 0; b < B; ++b) {
    if (which[b] == 1) {
      d->s2s.hOrigin[(size_t)b] = d->s2s.t;
      d->s2s.hParked[(size_t)b] = 0;
    } else if (which[b] == 2) {
      d->s2s.hParked[(size_t)b] = 1;
    }
  }
  d->s2s.liveUntil = 0;
  for (int b = 0; b < B; ++b) {
    if (!d->s2s.hParked[(size_t)b]) {
      d->s2s.liveUntil = std::max(d->s2s.liveUntil, d->s2s.hOrigin[(size_t)b] + d->s2s.maxOut);
    }
  }
  memset(out, 0, sizeof(*out));
  out->length = len;
  /* (home: n_hyp * length entries of each named slot) */
  return stepFinishResults(d, what, resultsOnDevice, nullptr, len, &fltx_s2s_finished_out::steps, out);
}

/* ---- collapsed transcripts (fltx_transcript.h) -------------------------------------------------------------------------- */
static int trMark(TrBufs& T, int i, Stream st) {
#ifndef FLTX_EMU
  if (T.timed) {
    if (!T.ev[i] && hipEventCreate(&T.ev[i]) != hipSuccess) {
      return 1;
    }
    return hipEventRecord(T.ev[i], st) != hipSuccess;
  }
#else
  (void)T, (void)i, (void)st;
#endif
  return 0;
}
/* ms[slot] = the time between two marks, once `to` has fired */
static void trElapsed(TrBufs& T, int from, int to, int slot) {
  T.ms[slot] = 0.0f;
#ifndef FLTX_EMU
  if (T.timed && T.ev[from] && T.ev[to] && hipEventSynchronize(T.ev[to]) == hipSuccess) {
    (void)hipEventElapsedTime(&T.ms[slot], T.ev[from], T.ev[to]);
  }
#else
  (void)from, (void)to;
#endif
}
/* a copy home that waits for nothing: trRun waits once, behind the last */
static int trCopyHome(void* h, const void* dv, size_t n, Stream st) {
#ifndef FLTX_EMU
  return hipMemcpyAsync(h, dv, n, hipMemcpyDeviceToHost, st) == hipSuccess ? 0 : 1;
#else
  (void)st;
  memcpy(h, dv, n);
  return 0;
#endif
}

/* count, scan, (the host reads the two totals and sizes the output,) write; then the arrays home unless on_device.
 * tok / wrd / rowOff / rowLen: device pointers.  Fills everything of *out but row_first and scores. */
static int trRun(TrBufs& T, Stream st, const int32_t* tok, const int32_t* wrd, const int64_t* rowOff, const int32_t* rowLen,
                 int64_t n, int32_t blank, int32_t onDevice, const char* what, fltx_transcripts* out,
                 const std::function<int(const TrParams&)>* counted = nullptr) {
  const size_t n1 = (size_t)n + 1;
  const int64_t blocks = (n + kTrRowsPerBlock - 1) / kTrRowsPerBlock;
  if (blocks > 0x7FFFFFFF) {
    return fail(FLTX_ERR_RANGE, "%s: %lld rows exceed a launch", what, (long long)n);
  }
  if (T.meta.ensure(16 + 16 * n1 + 8 * (size_t)n, st, false) || T.hTotals.ensure(16)) {
    return fail(FLTX_ERR_OOM, "%s: allocation failed", what);
  }
  TrParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.tok = tok;
  Q.wrd = wrd;
  Q.rowOff = rowOff;
  Q.rowLen = rowLen;
  Q.nRows = n;
  Q.blank = blank;
  Q.totals = T.meta.as<int64_t>();
  Q.tokOff = Q.totals + 2;
  Q.wordOff = Q.tokOff + n1;
  Q.nTok = (int32_t*)(Q.wordOff + n1);
  Q.nWord = Q.nTok + n;
  for (float& m : T.ms) {
    m = 0.0f;
  }
  if (n > 0) {
    if (trMark(T, 0, st)) {
      return fail(FLTX_ERR_HIP, "%s: event failed", what);
    }
    if (counted) { /* (the caller's kernel makes the rows and counts them: fltx_stream_partials) */
      const int rc = (*counted)(Q);
      if (rc) {
        return rc;
      }
    } else {
      S2S_LAUNCH(fltx_transcript_count_kernel, trCountRows, (int)blocks, kTrThreads, 0, st, Q);
    }
  }
  if (trMark(T, 1, st)) {
    return fail(FLTX_ERR_HIP, "%s: event failed", what);
  }
  S2S_LAUNCH(fltx_transcript_scan_kernel, trScanRows, 1, kTrScanThreads, sizeof(TrScanLds), st, Q);
  if (trMark(T, 2, st)) {
    return fail(FLTX_ERR_HIP, "%s: event failed", what);
  }
  /* the one look in between: 16 bytes, one wait */
  const int64_t* tot = (const int64_t*)T.hTotals.p;
  if (devCopyD2H(T.hTotals.p, Q.totals, 16, st)) {
    return fail(FLTX_ERR_HIP, "%s: copy failed: %s", what, devErr());
  }
  if (tot[0] < 0) {
    return fail(FLTX_ERR_INVALID, "%s: a row length is negative", what);
  }
  const size_t nt = (size_t)tot[0], nw = (size_t)tot[1];
  /* counted (fltx_stream_partials): the five arrays lie back to back in one allocation -- tokens, timesteps [ntc], words,
   * wordT, wordEnd [nwc] -- so that host mode brings them home in one copy: per chunk of a stream the copies of a call
   * cost more than its kernels.  (The other callers keep one buffer per array, at addresses that do not move.) */
  const bool packed = counted != nullptr;
  const size_t ntc = std::max<size_t>(nt, 1), nwc = std::max<size_t>(nw, 1);
  const size_t bt = 4 * ntc, bw = 4 * nwc, packBytes = 2 * bt + 3 * bw;
  if (packed) {
    if (T.pack.ensure(packBytes, st, false)) {
      return fail(FLTX_ERR_OOM, "%s: allocation failed", what);
    }
    Q.tokens = T.pack.as<int32_t>();
    Q.timesteps = Q.tokens + ntc;
    Q.words = Q.timesteps + ntc;
    Q.wordT = Q.words + nwc;
    Q.wordEnd = Q.wordT + nwc;
  } else {
    if (T.tokens.ensure(bt, st, false) || T.timesteps.ensure(bt, st, false) || T.words.ensure(bw, st, false) ||
        T.wordT.ensure(bw, st, false) || T.wordEnd.ensure(bw, st, false)) {
      return fail(FLTX_ERR_OOM, "%s: allocation failed", what);
    }
    Q.tokens = T.tokens.as<int32_t>();
    Q.timesteps = T.timesteps.as<int32_t>();
    Q.words = T.words.as<int32_t>();
    Q.wordT = T.wordT.as<int32_t>();
    Q.wordEnd = T.wordEnd.as<int32_t>();
  }
  const bool wrote = n > 0 && nt + nw > 0;
  if (wrote) {
    if (trMark(T, 3, st)) {
      return fail(FLTX_ERR_HIP, "%s: event failed", what);
    }
    S2S_LAUNCH(fltx_transcript_write_kernel, trWriteRows, (int)blocks, kTrThreads, 0, st, Q);
    if (trMark(T, 4, st)) {
      return fail(FLTX_ERR_HIP, "%s: event failed", what);
    }
  }
  out->n_rows = n;
  out->n_tokens = (int64_t)nt;
  out->n_words = (int64_t)nw;
  if (onDevice) {
    out->tok_off = Q.tokOff;
    out->word_off = Q.wordOff;
    out->tokens = Q.tokens;
    out->timesteps = Q.timesteps;
    out->words = Q.words;
    out->word_timesteps = Q.wordT;
    out->word_tok_end = Q.wordEnd;
  } else {
    if (T.hOff.ensure(16 * n1)) {
      return fail(FLTX_ERR_OOM, "%s: pinned buffers: allocation failed", what);
    }
    if (packed) {
      const size_t home = nw ? packBytes : (nt ? 2 * bt : 0); /* (without words: tokens and timesteps alone) */
      if (T.hPack.ensure(packBytes)) {
        return fail(FLTX_ERR_OOM, "%s: pinned buffers: allocation failed", what);
      }
      if (trCopyHome(T.hOff.p, Q.tokOff, 16 * n1, st) || (home && trCopyHome(T.hPack.p, T.pack.p, home, st)) || devSync(st)) {
        return fail(FLTX_ERR_HIP, "%s: copy failed: %s", what, devErr());
      }
      out->tokens = (const int32_t*)T.hPack.p;
      out->timesteps = out->tokens + ntc;
      out->words = out->timesteps + ntc;
      out->word_timesteps = out->words + nwc;
      out->word_tok_end = out->word_timesteps + nwc;
    } else {
      if (T.hTokens.ensure(bt) || T.hTimesteps.ensure(bt) || T.hWords.ensure(bw) || T.hWordT.ensure(bw) ||
          T.hWordEnd.ensure(bw)) {
        return fail(FLTX_ERR_OOM, "%s: pinned buffers: allocation failed", what);
      }
      if (trCopyHome(T.hOff.p, Q.tokOff, 16 * n1, st) || /* (tokOff and wordOff lie back to back) */
          (nt && (trCopyHome(T.hTokens.p, Q.tokens, 4 * nt, st) || trCopyHome(T.hTimesteps.p, Q.timesteps, 4 * nt, st))) ||
          (nw && (trCopyHome(T.hWords.p, Q.words, 4 * nw, st) || trCopyHome(T.hWordT.p, Q.wordT, 4 * nw, st) ||
                  trCopyHome(T.hWordEnd.p, Q.wordEnd, 4 * nw, st))) ||
          devSync(st)) {
        return fail(FLTX_ERR_HIP, "%s: copy failed: %s", what, devErr());
      }
      out->tokens = (const int32_t*)T.hTokens.p;
      out->timesteps = (const int32_t*)T.hTimesteps.p;
      out->words = (const int32_t*)T.hWords.p;
      out->word_timesteps = (const int32_t*)T.hWordT.p;
      out->word_tok_end = (const int32_t*)T.hWordEnd.p;
    }
    out->tok_off = (const int64_t*)T.hOff.p;
    out->word_off = out->tok_off + n1;
  }
  if (T.timed) {
    if (n > 0) {
      trElapsed(T, 0, 1, 0);
    }
    trElapsed(T, 1, 2, 1);
    if (wrote) {
      trElapsed(T, 3, 4, 2);
    }
  }
  return FLTX_OK;
}

int fltx_collapse_rows(fltx_ctx* ctx, const int32_t* tokens, const int32_t* words, const int64_t* rowOff,
                       const int32_t* rowLen, int64_t nRows, int32_t blank, int32_t onDevice, fltx_transcripts* out) {
  EntryScope entry(ctx);
  if (entry.rc) {
    return entry.rc;
  }
  if (!ctx || !out || nRows < 0 || (nRows > 0 && (!tokens || !rowOff || !rowLen))) {
    return fail(FLTX_ERR_INVALID, "fltx_collapse_rows: null ctx, out, tokens, row_off or row_len, or n_rows < 0");
  }
  memset(out, 0, sizeof(*out));
  return trRun(ctx->tr, ctx->stream, tokens, words, rowOff, rowLen, nRows, blank, onDevice, "fltx_collapse_rows", out);
}

int fltx_result_transcripts(fltx_decoder* d, int32_t maxHyp, int32_t onDevice, fltx_transcripts* out) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d || !out || maxHyp < 1) {
    return fail(FLTX_ERR_INVALID, "fltx_result_transcripts: null decoder or out, or max_hyp < 1");
  }
  if (isS2sKind(d->kind)) {
    return fail(FLTX_ERR_STATE, "fltx_result_transcripts: a seq2seq decoder's results are token strings already");
  }
  if (!d->haveResults || !d->ended) {
    return fail(FLTX_ERR_STATE, "fltx_result_transcripts: no finished decode");
  }
  int rc = syncResults(d);
  if (rc) {
    return rc;
  }
  const int B = d->B, K = d->opt.beam_size;
  for (int b = 0; b < B; ++b) {
    if ((rc = checkStatus(d, b))) {
      return rc;
    }
  }
  if (!d->backtraced && (rc = launchBacktrace(d))) {
    return rc;
  }
  Stream st = d->ctx->stream;
  TrBufs& T = d->tr;
  const bool lex = kindHasWords(d->kind);
  /* the rows: the first min(n_hyp[b], max_hyp) hypotheses of every utterance (counts as fltx_result_fetch_batch_compact) */
  T.rowFirst.resize((size_t)B + 1);
  int64_t n = 0;
  for (int b = 0; b < B; ++b) {
    T.rowFirst[b] = n;
    n += std::min((lex && d->hFrame[b] < 1) ? 0 : d->hN[b], maxHyp); /* LexiconDecoder.cpp:276-280 */
  }
  T.rowFirst[B] = n;
  const size_t nd = (size_t)std::max<int64_t>(n, 1);
  if (T.hDesc.ensure(12 * nd) || T.desc.ensure(12 * nd, st, false) || (!onDevice && d->hScores.ensure(8 * 3 * (size_t)B * K))) {
    return fail(FLTX_ERR_OOM, "fltx_result_transcripts: allocation failed");
  }
  int64_t* hOff = (int64_t*)T.hDesc.p;
  int32_t* hLen = (int32_t*)(hOff + n);
  for (int b = 0; b < B; ++b) {
    const int32_t len = d->hFrame[b] + 1;
    for (int64_t r = T.rowFirst[b]; r < T.rowFirst[b + 1]; ++r) {
      hOff[r] = d->histOff[b] + (r - T.rowFirst[b]) * len;
      hLen[r] = len;
    }
  }
  if (n > 0 && devCopyH2D(T.desc.p, T.hDesc.p, 12 * (size_t)n, st)) { /* (pinned; the look at the totals waits behind it) */
    return fail(FLTX_ERR_HIP, "fltx_result_transcripts: upload failed");
  }
  memset(out, 0, sizeof(*out));
  const int32_t blank = d->opt.criterion == FLTX_CRITERION_CTC ? d->blank : -1;
  if ((rc = trRun(T, st, d->tokens.as<int32_t>(), lex ? d->words.as<int32_t>() : nullptr, T.desc.as<int64_t>(),
                  (const int32_t*)(T.desc.as<int64_t>() + n), n, blank, onDevice, "fltx_result_transcripts", out))) {
    return rc;
  }
  out->row_first = T.rowFirst.data();
  if (onDevice) {
    out->scores = d->outScores.as<double>();
  } else {
    if (!d->scoresFetched && devCopyD2H(d->hScores.p, d->outScores.p, 8 * 3 * (size_t)B * K, st)) {
      return fail(FLTX_ERR_HIP, "result copy failed: %s", devErr());
    }
    d->scoresFetched = true;
    out->scores = (const double*)d->hScores.p;
  }
  return FLTX_OK;
}

/* ---- partial transcripts of all streams (fltx_stream_partials.h) -------------------------------------------------------- */
int fltx_stream_partials(fltx_decoder* d, int32_t lookBack, int32_t onDevice, fltx_stream_partials_out* out) {
  EntryScope entry(d);
  if (entry.rc) {
    return entry.rc;
  }
  if (!d || !out || lookBack < 0) {
    return fail(FLTX_ERR_INVALID, "fltx_stream_partials: null decoder or out, or look_back < 0");
  }
  const bool rows = isCrKind(d->kind);
  if (isS2sKind(d->kind)) {
    return fail(FLTX_ERR_STATE, "fltx_stream_partials: a seq2seq decoder has no streams");
  }
  if (rows ? !(d->s2s.begun && d->s2s.crStream) : !(d->streaming && !d->ended && d->haveResults)) {
    return fail(FLTX_ERR_STATE, "fltx_stream_partials: no open stream (%s first)",
                rows ? "fltx_ctc_rows_stream_begin" : "fltx_stream_begin");
  }
  const int B = d->B;
  int cap = 1;
  if (rows) {
    cap = d->s2s.crRing;
  } else {
    /* the waits fltx_result_best makes before its launch: a pending chunk is settled, the counts and statuses looked at */
    int rc = syncResults(d);
    if (rc) {
      return rc;
    }
    for (int b = 0; b < B; ++b) {
      cap = std::max(cap, d->hFrame[b] + 1);
    }
  }
  Stream st = d->ctx->stream;
  const bool lex = kindHasWords(d->kind);
  const size_t outBytes = 60 * (size_t)B;
  if (d->spOut.ensure(outBytes, st, false) || d->spTok.ensure(4 * (size_t)B * cap, st, false) ||
      (lex && d->spWrd.ensure(4 * (size_t)B * cap, st, false)) || (!onDevice && d->hSpOut.ensure(outBytes))) {
    return fail(FLTX_ERR_OOM, "fltx_stream_partials: allocation failed");
  }
  SpParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.B = B;
  Q.K = d->opt.beam_size;
  Q.lex = lex ? 1 : 0;
  Q.lookBack = lookBack;
  Q.cap = cap;
  Q.blank = d->opt.criterion == FLTX_CRITERION_CTC ? d->blank : -1;
  Q.errState = FLTX_ERR_STATE;
  Q.errUnsupported = FLTX_ERR_UNSUPPORTED;
  if (rows) {
    const CrsParams X = crsParams(d);
    Q.hist = d->s2s.hist.p;
    Q.sHist = X.sHist;
    Q.nDec = X.nDec;
    Q.base = X.base;
    Q.ring = X.ring;
    Q.beamN = d->s2s.beamN.as<int32_t>();
    Q.status = d->s2s.status.as<int32_t>();
  } else {
    Q.histPT = d->histPT.as<int2>();
    Q.histW = d->histW.as<int32_t>();
    Q.histS = d->histS.as<double>();
    Q.histOff = d->histOffD.as<int64_t>();
    Q.uttFrame = d->uttFrame.as<int32_t>();
    Q.uttNBeam = d->uttNBeam.as<int32_t>();
    Q.uttStatus = d->uttStatus.as<int32_t>();
    Q.uttFirst = d->uttFirst.as<int64_t>();
  }
  Q.rowTok = d->spTok.as<int32_t>();
  Q.rowWrd = lex ? d->spWrd.as<int32_t>() : nullptr;
  Q.firstFrame = d->spOut.as<int64_t>();
  Q.rowOff = Q.firstFrame + B;
  Q.scores = (double*)(Q.rowOff + B);
  Q.length = (int32_t*)(Q.scores + 3 * (size_t)B);
  Q.stableFrames = Q.length + B;
  Q.stableTokens = Q.stableFrames + B;
  Q.stableWords = Q.stableTokens + B;
  Q.outStatus = Q.stableWords + B;
  const int kind = d->kind;
  void* hHome = onDevice ? nullptr : d->hSpOut.p;
  const void* dHome = d->spOut.p;
  const std::function<int(const TrParams&)> counted = [&Q, B, kind, st, hHome, dHome, outBytes](const TrParams& T) -> int {
    Q.nTok = T.nTok;
    Q.nWord = T.nWord;
    if (kind == FLTX_DECODER_LEX_CTC_ROWS) {
      S2S_LAUNCH(fltx_stream_partials_kernel<2>, spPartials<2>, B, kSpThreads, sizeof(SpLds), st, Q);
    } else if (kind == FLTX_DECODER_CTC_ROWS) {
      S2S_LAUNCH(fltx_stream_partials_kernel<1>, spPartials<1>, B, kSpThreads, sizeof(SpLds), st, Q);
    } else {
      S2S_LAUNCH(fltx_stream_partials_kernel<0>, spPartials<0>, B, kSpThreads, sizeof(SpLds), st, Q);
    }
    /* (the per-stream numbers home in one copy, which the look at the totals waits behind) */
    if (hHome && trCopyHome(hHome, dHome, outBytes, st)) {
      return fail(FLTX_ERR_HIP, "fltx_stream_partials: copy failed: %s", devErr());
    }
    return FLTX_OK;
  };
  memset(out, 0, sizeof(*out));
  int rc = trRun(d->spTr, st, Q.rowTok, Q.rowWrd, Q.rowOff, Q.length, B, Q.blank, onDevice, "fltx_stream_partials", &out->t,
                 &counted);
  if (rc) {
    return rc;
  }
  const char* home = onDevice ? (const char*)d->spOut.p : (const char*)d->hSpOut.p;
  out->first_frame = (const int64_t*)home;
  out->t.scores = (const double*)(home + 16 * (size_t)B);
  out->length = (const int32_t*)(home + 40 * (size_t)B);
  out->stable_frames = out->length + B;
  out->stable_tokens = out->stable_frames + B;
  out->stable_words = out->stable_tokens + B;
  out->status = out->stable_words + B;
  return FLTX_OK;
}

} /* extern "C" */
