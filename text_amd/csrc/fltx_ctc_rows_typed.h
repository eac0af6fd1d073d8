/*
 * fltx_ctc_rows_typed.h -- the emissions of the two CTC rows kinds as the acoustic model produces them: float32, fp16 or
 * bf16, log-probs or raw logits, frames of any stride (fltx_ctc_rows_begin_typed, fltx_ctc_rows_stream_append_typed).
 * Included after fltx_ctc_rows.h and before fltx_ctc_rows_lex.h.
 *
 * The emission of token n in a frame is e[n]: the element widened exactly (s2sElem, bit operations only), for logits
 * (float)((double)x_n - lse) with the frame's lse as fltx_s2s.h defines it (s2sTypedScore).  No float32 copy of the
 * emissions exists in HBM: the front end reads the typed frames once per begin / append and writes the same recTok /
 * recAm / recN records fltx_ctc_rows_tokbeam_kernel writes for the rows e, the lexicon step reads its blank and same-node
 * emissions from the typed buffer through crEmission with the frame's lse, which the decoder keeps per frame record.
 *
 * The front end is one launch of one of two kernels, chosen by the width of a frame:
 *   fltx_ctc_rows_typed_wave_kernel  N <= the switch-over width (kCrTypedNarrowMax; at most kCrTypedNarrowCap): four
 *                                    waves per workgroup, a wave per frame, as the float32 front end.  The wave widens
 *                                    the frame into its slice of LDS, takes max and sum there (lane-strided partial sums
 *                                    in double, then a fixed butterfly: the same bits run to run), turns the slice into e
 *                                    in place and runs s2sTokBeamRow on it -- the float32 front end's selection itself.
 *   fltx_ctc_rows_typed_wg_kernel    wider frames: a workgroup of 256 per frame, s2sTypedRow -- the seq2seq typed front end
 *                                    as it is, with its read-once registers (N <= 16 384) -- on the frame.
 * Both give a token its rank by (e, lower token first), so they write the same records; a frame's lse may differ in the
 * last bits between the two (the partial sums are grouped differently), which is why the choice depends on N alone.
 */
#pragma once

namespace fltx {

constexpr int kCrTypedNarrowCap = 1024; /* the widest frame a wave takes: its slice of LDS */
constexpr int kCrTypedNarrowMax = 1024; /* the switch-over, measured (profiles/ctc_rows_typed_emissions/README.md): the
                                         * wave is the faster one at every width it can take */
constexpr int kCrEmPlain = -1;          /* EM of a step that reads the float32 log-probs of fltx_ctc_rows_begin */

struct CrTypedEm { /* the typed frames of the batch or chunk */
  const void* x;   /* frame f of utterance b at x + (emOff[b] + f * stride) ELEMENTS */
  int64_t stride;
  double* lse;     /* [frame records] the decoder's own: each frame's lse (logits) */
};

struct CrTypedParams {
  CrParams c;     /* (c.emissions is not read) */
  CrTypedEm e;
  double* lseOut; /* the caller's frame_lse: [frame records] or null */
};

/* the emission of token n of the frame at `em`: a float32 log-prob (kCrEmPlain), else the typed element */
template <int EM, bool LOGITS>
FLTX_DEV float crEmission(const void* em, int n, double lse) {
  if constexpr (EM == kCrEmPlain) {
    return ((const float*)em)[n];
  } else {
    return s2sTypedScore<EM, LOGITS>(em, n, lse);
  }
}

template <int DT>
FLTX_DEV const void* crTypedFrame(const CrTypedParams& Z, int b, int64_t fr) {
  return (const char*)Z.e.x + (Z.c.emOff[b] + (fr - Z.c.frameOff[b]) * Z.e.stride) * (DT == kS2sDtF32 ? 4 : 2);
}

struct CrTypedWaveLds { /* per wave */
  S2sFrontLds f;
  float e[kCrTypedNarrowCap];
};

/* workgroup = four waves, wave = frame record fr of the batch (N <= kCrTypedNarrowCap) */
template <int DT, bool LOGITS>
FLTX_DEV void crTypedWaveRows(const CrTypedParams& Z, char* smem) {
  const CrParams& Q = Z.c;
  const S2sParams& P = Q.s;
  const int wave = waveUniform(waveId()), lane = laneId();
  const int64_t fr = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
  if (fr >= Q.frameOff[P.B]) {
    return;
  }
  const int b = crFrameUtterance(Q, fr);
  const void* row = crTypedFrame<DT>(Z, b, fr);
  CrTypedWaveLds& S = ((CrTypedWaveLds*)smem)[wave];
  const int V = P.V;
  uint32_t mk = 0u;
  for (int i = lane; i < V; i += 64) { /* (every lane reads back the slots it wrote, here and in s2sTokBeamRow) */
    const float x = s2sElem<DT>(row, i);
    S.e[i] = x;
    const uint32_t k = s2sRawKey(x);
    mk = k > mk ? k : mk;
  }
  if constexpr (LOGITS) { /* lse = max + log(sum exp(x - max)) over the non-NaN entries; lse = max when that is not finite */
    mk = waveMax32(mk);
    const float mx = mk != 0u ? f32FromKey(mk) : -__builtin_huge_valf();
    double lse = (double)mx;
    if (mx - mx == 0.0f) { /* finite */
      double s = 0.0;
      for (int i = lane; i < V; i += 64) {
        const float x = S.e[i];
        if (x == x) {
          s += (double)expf(x - mx);
        }
      }
      for (int d = 32; d >= 1; d >>= 1) { /* (a fixed butterfly: the same sum in every lane, run to run) */
        s += __longlong_as_double((long long)waveShflXor64((unsigned long long)__double_as_longlong(s), d));
      }
      lse = (double)mx + log(s);
    }
    if (lane == 0) {
      Z.e.lse[fr] = lse;
      if (Z.lseOut) {
        Z.lseOut[fr] = lse;
      }
    }
    for (int i = lane; i < V; i += 64) {
      S.e[i] = (float)((double)S.e[i] - lse);
    }
  }
  waveSync();
  s2sTokBeamRow(P, S.f, S.e, P.recTok + fr * P.cap, P.recAm + fr * P.cap, P.recN + fr);
}

/* workgroup = frame record fr of the batch */
template <int DT, bool LOGITS>
FLTX_DEV void crTypedWgRows(const CrTypedParams& Z, char* smem) {
  const CrParams& Q = Z.c;
  const S2sParams& P = Q.s;
  const int64_t fr = (int64_t)blockIdx.x;
  const int b = crFrameUtterance(Q, fr);
  S2sTypedLds& S = *(S2sTypedLds*)smem;
  /* s2sTypedRow's "row fr": the frame itself (a row stride of 0 from it), record fr, the decoder's lse of record fr */
  S2sTypedParams Y;
  Y.s = P;
  Y.s.rowStride = 0;
  Y.x = crTypedFrame<DT>(Z, b, fr);
  Y.rowLse = LOGITS ? Z.e.lse : nullptr;
  if (P.V <= kS2sTypedReadOnceV) {
    s2sTypedRow<DT, LOGITS, true>(Y, S, fr);
  } else {
    s2sTypedRow<DT, LOGITS, false>(Y, S, fr);
  }
  if (LOGITS && Z.lseOut && threadIdx.x == 0) { /* (thread 0 wrote it) */
    Z.lseOut[fr] = Z.e.lse[fr];
  }
}

} // namespace fltx
