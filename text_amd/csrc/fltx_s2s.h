/*
 * fltx_s2s.h -- the lexicon-free seq2seq beam search (LexiconFreeSeq2SeqDecoder.cpp:20-165) as a batched device step.
 *
 * The emitting model is the caller's: it runs between two steps (a PyTorch attention decoder on the same stream) and
 * leaves one row of V scores per live hypothesis in HBM.  A step is two kernels:
 *   fltx_s2s_tokbeam_kernel  one wave per live row, all rows of the batch: the row's token beam (its largest scores,
 *                            LexiconFreeSeq2SeqDecoder.cpp:87-107), written as a compact record;
 *   fltx_s2s_step_kernel     one workgroup per utterance: the candidates of the step from the records and the carried
 *                            finished hypotheses, their scores with the device LM (ZeroLM / the n-gram tables), the
 *                            threshold and the top K (Utils.h:121-228), the new beam, one history record per
 *                            hypothesis, and the next step's row list (what the model gathers its state with).
 * fltx_s2s_end_kernel writes the n-best in the layout fltx_result_* read.
 *
 * Both selections are a most-significant-digit-first radix select over order keys (f32Key / f64Key, 256 bins per
 * pass, slScan finds the bin that holds the cut): exact, the ties at the cut to the lower index.
 *
 * No merges: the reference compares LM-state OBJECTS (compareNoScoreStates), and ZeroLM / KenLM hand out a new child
 * object per (state, token), so two candidates of one step never share a state and candidatesStore's merge -- logAdd
 * with it -- never fires.  A hypothesis carries its n-gram context (the suffix node ids ngScore takes) in its record.
 */
#pragma once

namespace fltx {

constexpr int kS2sMaxBeam = 256;     /* beamSize */
constexpr int kS2sMaxV = 65536;      /* row width */
constexpr int kS2sMaxKtLm = 64;      /* min(beamSizeToken, V) with a scoring LM (lmWeight != 0, n-gram) */
constexpr int kS2sMaxLen = 4096;     /* maxOutputLength */
constexpr int kS2sCtx = kMaxNgramOrder - 1;
constexpr int kS2sStepThreads = 256; /* the step kernel: one thread per beam slot */
constexpr int kS2sBeginThreads = 64; /* the begin kernel: one thread per utterance */
constexpr int kS2sEndThreads = 256;  /* the end kernel: one workgroup per utterance, thread per hypothesis */

struct S2sHyp { /* one hypothesis of a beam, 56 B */
  double score, am, lm;
  int32_t token;  /* -1: the root */
  int32_t parent; /* index in the previous beam (prevHypIdx) */
  int32_t ctx[kS2sCtx];
  int32_t pad;
};

struct S2sParams {
  DecodeParams lmp; /* the LM fields only (ngScore reads them) */
  int32_t B, K, Kt, V, eos, maxOut;
  int32_t t;        /* steps the batch has taken before this one (beam parity t & 1 is the current beam) */
  int32_t cap;      /* entries per row record */
  int32_t mSel;     /* tokens per row the front end keeps */
  int32_t eosExtra; /* 1: mSel < min(Kt, V) (exact shortcut without LM terms): eos is added when it is in the top Kt */
  int32_t lmOn;     /* n-gram LM: score / finish on the device tables */
  double beamThreshold, lmWeight, eosScore;
  const float* scores;
  int64_t rowStride;
  const uint8_t* rowValid; /* may be null */
  S2sHyp* beam;            /* [2][B*K] */
  int32_t* beamN;          /* [2][B] */
  int2* hist;              /* [maxOut + 1][B*K]: (token, parent) of the hypotheses of step s */
  int32_t* nRowsInt;       /* [B] rows of the current step */
  int32_t* done;           /* [B] */
  int32_t* finalStep;      /* [B] the step whose beam is the final one (valid when done), counted as s2sLocalT counts;
                            * seq2seq: [3][B], see s2sOrigin (no field of its own: the CTC rows kernels share this
                            * struct and keep their argument layout) */
  int32_t* recTok;         /* [B*K][cap] */
  float* recAm;
  int32_t* recN;           /* [B*K] */
  unsigned long long* cKey; /* [B][nC]: order keys of the step's candidates, 0 = none */
  int64_t nC;
  int32_t ctx0[kS2sCtx];   /* LM::start(false) */
  int32_t *outTok, *outBeam, *outSrc, *outN; /* the caller's next-row lists [B*K], [B] */
  /* end */
  double* outScores;
  int32_t* tokens;
  int32_t *outNHyp, *uttNBeam, *uttFrame, *uttStatus;
  int32_t len;
};

/* seq2seq: behind finalStep[B], origin[B] -- the batch's step count when the utterance in slot b was (re)started
 * (fltx_s2s_begin: 0, fltx_s2s_finish: t) -- and parked[B], 1 for a parked slot.
 * The steps the utterance in slot b has taken: what the length limit, the history row, finalStep and the back-trace
 * count in.  The beam parity stays the batch's (t & 1): a restart writes its root into the current half */
FLTX_DEV int32_t* s2sOrigin(const S2sParams& P) { return P.finalStep + P.B; }
FLTX_DEV int s2sLocalT(const S2sParams& P, int b) { return P.t - s2sOrigin(P)[b]; }
/* The length limit needs no test of its own where `done` is read: the step that takes an utterance to max_output_length
 * sets done[b] (s2sPublishStepWith), and so does a (re)start with max_output_length 0 -- a slot that is not done has
 * local steps left.  So the front ends and the steps' entry test read done[b] alone, and the origin is loaded where the
 * step first needs it: the history row. */

/* ---- LM ------------------------------------------------------------------------------------------------------- */
/* LM::score (KenLM.cpp:63-75: child state per token) over the LM's user ids, and LM::finish, of the n-gram tables;
 * ZeroLM: 0.  The question is `usr`, or finish when usr == finishUsr: eos where the ids are the model's tokens,
 * kS2sLmFinish where no id means it.  (The comparison stays in here, behind lmOn: handed in as a flag it cost the
 * lexicon-free step kernel 1.3 us a launch.) */
constexpr int kS2sLmFinish = -2;
FLTX_DEV float s2sLm(const S2sParams& P, const int32_t* ctx, int usr, int finishUsr, int32_t* ctxOut) {
  if (!P.lmOn) {
    return 0.0f;
  }
  const DecodeParams& L = P.lmp;
  uint32_t word;
  if (usr == finishUsr) {
    word = (uint32_t)L.lmEos;
  } else {
    word = (usr >= 0 && usr < L.nUsr) ? (uint32_t)L.usrToLm[usr] : (uint32_t)L.lmUnk;
  }
  return ngScore(L, ctx, word, ctxOut);
}

/* the candidate (hypothesis h, token tok, emitting-model score a): LexiconFreeSeq2SeqDecoder.cpp:113-141, the same
 * double operations in the same order (the library is built with -ffp-contract=off) */
FLTX_DEV double s2sScore(const S2sParams& P, const S2sHyp& h, int tok, float a, float lmS) {
  if (tok == P.eos) {
    return ((h.score + (double)a) + P.eosScore) + P.lmWeight * (double)lmS;
  }
  return (h.score + (double)a) + P.lmWeight * (double)lmS;
}

/* ---- front end: the token beam of every live row ----------------------------------------------------------------- */
struct S2sFrontLds { /* per wave */
  uint32_t hist[kSlNB];
};

/* key of a score: NaN is never a candidate (0) */
FLTX_DEV uint32_t s2sKey32(float x) { return x == x ? f32Key(x + 0.0f) : 0u; }

FLTX_DEV void s2sTokBeamRow(const S2sParams& P, S2sFrontLds& S, const float* row, int32_t* tok, float* am,
                            int32_t* nOut) {
  const int lane = laneId();
  const int V = P.V, m = P.mSel;
  /* passes over the digits, most significant first: pre / msk = the digits decided so far, `need` = how many of the
   * values that share them the token beam still takes */
  uint32_t pre = 0u, msk = 0u;
  int need = m;
  bool all = m >= V, allEq = false;
  for (int shift = 24; shift >= 0 && !all && !allEq; shift -= 8) {
    waveSync();
    ((uint4*)S.hist)[lane] = make_uint4(0u, 0u, 0u, 0u);
    waveSync();
    for (int i = lane; i < V; i += 64) {
      const uint32_t k = s2sKey32(row[i]);
      if (k != 0u && (k & msk) == pre) {
        atomAdd32(&S.hist[255u - ((k >> shift) & 255u)], 1u);
      }
    }
    waveSync();
    const SlScan sc = slScan(S.hist, need, false);
    if (sc.total <= need) { /* (first pass: no more values than the beam takes) */
      all = true;
      break;
    }
    need -= sc.cum;
    pre |= (uint32_t)(255 - sc.bstar) << shift;
    msk |= 255u << shift;
    allEq = sc.cnt == need;
  }
  /* the list, in token order: the values above the decided digits, and the first `need` of those equal to them */
  int nList = 0, eqSeen = 0;
  bool eosIn = false;
  for (int c = 0; c < V; c += 64) {
    const int i = c + lane;
    const float x = i < V ? row[i] : 0.0f;
    const uint32_t k = i < V ? s2sKey32(x) : 0u;
    bool sel = k != 0u && (all || (k & msk) > pre);
    if (!all) {
      const bool eq = k != 0u && (k & msk) == pre;
      const unsigned long long eb = waveBallot(eq);
      sel = sel || (eq && (allEq || eqSeen + wavePrefixCount(eb) < need));
      eqSeen += popc64(eb);
    }
    const unsigned long long sb = waveBallot(sel);
    if (sel) {
      const int pos = nList + wavePrefixCount(sb);
      tok[pos] = i;
      am[pos] = x;
    }
    const bool eosHere = waveBallot(sel && i == P.eos) != 0ull;
    eosIn = eosIn || eosHere;
    nList += popc64(sb);
  }
  /* the shortcut kept fewer than the token beam: eos still is a candidate when it is among the row's Kt best (ties to
   * the lower token, as above) */
  if (P.eosExtra && !eosIn && P.eos >= 0 && P.eos < V) {
    const float xe = row[P.eos];
    const uint32_t ke = s2sKey32(xe);
    if (ke != 0u) {
      int above = 0;
      for (int i = lane; i < V; i += 64) {
        const uint32_t k = s2sKey32(row[i]);
        above += (k > ke || (k == ke && i < P.eos)) ? 1 : 0;
      }
      above = (int)waveReadLane32((uint32_t)waveInclusiveScan(above), 63);
      if (above < P.Kt) {
        if (lane == 0) {
          tok[nList] = P.eos;
          am[nList] = xe;
        }
        ++nList;
      }
    }
  }
  if (lane == 0) {
    *nOut = nList;
  }
}

/* workgroup = four waves, wave = row b*K + k of the step */
FLTX_DEV void s2sTokBeamRows(const S2sParams& P, char* smem) {
  const int wave = waveUniform(waveId());
  const int64_t r = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
  if (r >= (int64_t)P.B * P.K) {
    return;
  }
  const int b = (int)(r / P.K), k = (int)(r % P.K);
  const bool live = !P.done[b] && k < P.nRowsInt[b] && (P.rowValid == nullptr || P.rowValid[r] != 0);
  if (!live) {
    if (laneId() == 0) {
      P.recN[r] = 0;
    }
    return;
  }
  S2sFrontLds& S = ((S2sFrontLds*)smem)[wave];
  s2sTokBeamRow(P, S, P.scores + r * P.rowStride, P.recTok + r * P.cap, P.recAm + r * P.cap, P.recN + r);
}

/* ---- typed front end: the model's rows as it produces them (f32 / fp16 / bf16, log-probs or raw logits) ----------
 * One workgroup of kS2sTypedThreads per live row; it writes the record s2sTokBeamRow writes.  Each element is widened
 * to float with bit operations (no half-precision intrinsics: the emulator runs the same code); logits become
 * a_v = (float)((double)x_v - lse) with lse the row's log-sum-exp (max, then the sum of f32 exp(x - max) in double).
 * The token beam is taken over s2sKey32(a_v) with the ties to the lower token, as in the f32 path: a radix select over
 * the 48-bit composite key32(a_v) << 16 | (0xFFFF - token), whose keys are distinct, so the cut is one element.
 * A row of V <= kS2sTypedRegs * kS2sTypedThreads values is read from HBM once and kept in registers (64 per thread)
 * between the max, sum, radix and listing passes; wider rows (up to kS2sMaxV) are re-read in every pass. */
constexpr int kS2sTypedThreads = 256;
constexpr int kS2sTypedRegs = 64;
constexpr int kS2sTypedReadOnceV = kS2sTypedThreads * kS2sTypedRegs; /* 16 384 */
constexpr int kS2sTypedMaxList = 264; /* >= the largest mSel: min(Kt, V, K + 1) <= 257, kS2lMaxKt = 256 */
enum { kS2sDtF32 = 0, kS2sDtF16 = 1, kS2sDtBf16 = 2 };

struct S2sTypedParams {
  S2sParams s;     /* (s.scores is not read) */
  const void* x;   /* the rows: element (r, i) at x + (r * s.rowStride + i) elements */
  double* rowLse;  /* [B*K] or null: logits mode writes lse (live rows) or NaN */
};

struct S2sTypedLds {
  uint32_t hist[kSlNB];
  int32_t listTok[kS2sTypedMaxList];
  float listAm[kS2sTypedMaxList];
  double wsum[kS2sTypedThreads / 64];
  uint32_t wmax[kS2sTypedThreads / 64];
  int32_t wcnt[kS2sTypedThreads / 64];
  uint32_t nList;
  int32_t eosIn;
  float eosA;
};

/* fp16 -> float, exact: normals and inf / NaN by moving the fields, subnormals as mantissa * 2^-24 (exact in f32) */
FLTX_DEV float s2sWidenF16(uint32_t h) {
  const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
  if (e == 31u) {
    return __uint_as_float(s | 0x7F800000u | (m << 13));
  }
  if (e != 0u) {
    return __uint_as_float(s | ((e + 112u) << 23) | (m << 13));
  }
  return __uint_as_float(s | __float_as_uint((float)m * 5.9604644775390625e-8f));
}

template <int DT>
FLTX_DEV float s2sElem(const void* row, int i) {
  if constexpr (DT == kS2sDtF32) {
    return ((const float*)row)[i];
  } else if constexpr (DT == kS2sDtF16) {
    return s2sWidenF16((uint32_t)((const uint16_t*)row)[i]);
  } else {
    return __uint_as_float((uint32_t)((const uint16_t*)row)[i] << 16);
  }
}

/* the order key of a raw element: f32Key, 0 for NaN (the max and the sum skip those) */
FLTX_DEV uint32_t s2sRawKey(float x) { return x == x ? f32Key(x) : 0u; }

/* the model score of token i: the widened element, minus lse for logits */
template <int DT, bool LOGITS>
FLTX_DEV float s2sTypedScore(const void* row, int i, double lse) {
  const float x = s2sElem<DT>(row, i);
  return LOGITS ? (float)((double)x - lse) : x;
}

/* f(token, key) for every token of the row -- with the registers, also for the padding slots beyond V, whose key is
 * 0.  RAW: the raw element's s2sRawKey (logits before lse is known), else s2sKey32 of the model score */
template <int DT, bool LOGITS, bool CACHED, bool RAW, typename F>
FLTX_DEV void s2sTypedEach(const void* row, int V, double lse, const uint32_t* kr, F&& f) {
  int tid = (int)threadIdx.x;
  if constexpr (CACHED) {
#ifndef FLTX_EMU
    __asm__ volatile("" : "+v"(tid)); /* (a new value per pass: nothing per token is hoisted out of the passes) */
#endif
#pragma unroll
    for (int j = 0; j < kS2sTypedRegs; ++j) {
      if (j * kS2sTypedThreads < V) { /* (uniform: the slots a narrow row does not reach cost a scalar branch) */
        f(tid + j * kS2sTypedThreads, kr[j]);
      }
    }
  } else {
    for (int i = tid; i < V; i += kS2sTypedThreads) {
      f(i, RAW ? s2sRawKey(s2sElem<DT>(row, i)) : s2sKey32(s2sTypedScore<DT, LOGITS>(row, i, lse)));
    }
  }
}

/* sum of v over the workgroup, in every thread (the typed front end's workgroup and the step's: four waves) */
static_assert(kS2sTypedThreads == kS2sStepThreads, "s2sBlockSum: one wcnt slot per wave");
FLTX_DEV int s2sBlockSum(int32_t (&wcnt)[kS2sStepThreads / 64], int v) {
  const int s = (int)waveReadLane32((uint32_t)waveInclusiveScan(v), 63);
  __syncthreads();
  if (laneId() == 0) {
    wcnt[waveId()] = s;
  }
  __syncthreads();
  int all = 0;
  for (int w = 0; w < kS2sStepThreads / 64; ++w) {
    all += wcnt[w];
  }
  return all;
}

template <int DT, bool LOGITS, bool CACHED>
FLTX_DEV void s2sTypedRow(const S2sTypedParams& Q, S2sTypedLds& S, int64_t r) {
  const S2sParams& P = Q.s;
  const int tid = (int)threadIdx.x, lane = laneId(), wave = waveId();
  const int V = P.V, m = P.mSel;
  const void* row = (const char*)Q.x + r * P.rowStride * (DT == kS2sDtF32 ? 4 : 2);
  /* the row's keys, 64 per thread: raw keys for logits (model-score keys once lse is known), model-score keys else */
  uint32_t kr[CACHED ? kS2sTypedRegs : 1];
  if constexpr (CACHED) {
#pragma unroll
    for (int j = 0; j < kS2sTypedRegs; ++j) {
      const int i = tid + j * kS2sTypedThreads;
      kr[j] = 0u;
      if (j * kS2sTypedThreads < V) {
        const float x = i < V ? s2sElem<DT>(row, i) : __uint_as_float(0x7FC00000u);
        kr[j] = LOGITS ? s2sRawKey(x) : s2sKey32(x);
      }
    }
  }
  /* logits: lse = max + log(sum exp(x - max)) over the non-NaN entries; lse = max when that is not finite */
  double lse = 0.0;
  if constexpr (LOGITS) {
    uint32_t mk = 0u;
    s2sTypedEach<DT, LOGITS, CACHED, true>(row, V, 0.0, kr, [&](int, uint32_t k) { mk = k > mk ? k : mk; });
    mk = waveMax32(mk);
    if (lane == 0) {
      S.wmax[wave] = mk;
    }
    __syncthreads();
    for (int w = 0; w < kS2sTypedThreads / 64; ++w) {
      mk = S.wmax[w] > mk ? S.wmax[w] : mk;
    }
    const float mx = mk != 0u ? f32FromKey(mk) : -__builtin_huge_valf();
    lse = (double)mx;
    if (mx - mx == 0.0f) { /* finite */
      double s = 0.0;
      s2sTypedEach<DT, LOGITS, CACHED, true>(row, V, 0.0, kr, [&](int, uint32_t k) {
        if (k != 0u) {
          s += (double)expf(f32FromKey(k) - mx);
        }
      });
      for (int d = 32; d >= 1; d >>= 1) { /* (a fixed butterfly: the same sum in every lane, run to run) */
        s += __longlong_as_double((long long)waveShflXor64((unsigned long long)__double_as_longlong(s), d));
      }
      if (lane == 0) {
        S.wsum[wave] = s;
      }
      __syncthreads();
      s = 0.0;
      for (int w = 0; w < kS2sTypedThreads / 64; ++w) {
        s += S.wsum[w];
      }
      lse = (double)mx + log(s);
    }
    if (Q.rowLse && tid == 0) {
      Q.rowLse[r] = lse;
    }
    if constexpr (CACHED) {
#pragma unroll
      for (int j = 0; j < kS2sTypedRegs; ++j) { /* (slots beyond V hold 0 and stay 0) */
        kr[j] = kr[j] != 0u ? s2sKey32((float)((double)f32FromKey(kr[j]) - lse)) : 0u;
      }
    }
  }
  /* the radix select over the 48-bit composite key << 16 | (0xFFFF - token), most significant digit first: four
   * digits of the key, then (equal keys at the cut) two of the inverted token */
  uint32_t preK = 0u, mskK = 0u, preI = 0u, mskI = 0u;
  int need = m;
  bool all = m >= V, allEq = false;
  for (int shift = 40; shift >= 0 && !all && !allEq; shift -= 8) {
    __syncthreads();
    S.hist[tid] = 0u; /* (kS2sTypedThreads == kSlNB) */
    __syncthreads();
    s2sTypedEach<DT, LOGITS, CACHED, false>(row, V, lse, kr, [&](int i, uint32_t k) {
      const uint32_t ix = 0xFFFFu - (uint32_t)i;
      if (k != 0u && (k & mskK) == preK && (ix & mskI) == preI) {
        const uint32_t dg = shift >= 16 ? (k >> (shift - 16)) & 255u : (ix >> shift) & 255u;
        atomAdd32(&S.hist[255u - dg], 1u);
      }
    });
    __syncthreads();
    const SlScan sc = slScan(S.hist, need, false); /* (every wave scans the same counts) */
    if (sc.total <= need) {
      all = true;
      break;
    }
    need -= sc.cum;
    const uint32_t dg = (uint32_t)(255 - sc.bstar);
    if (shift >= 16) {
      preK |= dg << (shift - 16);
      mskK |= 255u << (shift - 16);
    } else {
      preI |= dg << shift;
      mskI |= 255u << shift;
    }
    allEq = sc.cnt == need;
  }
  /* the list: every candidate at or above the cut (the composite keys are distinct: min(mSel, candidates) of them) */
  if (tid == 0) {
    S.nList = 0u;
    S.eosIn = 0;
    S.eosA = __uint_as_float(0x7FC00000u);
  }
  __syncthreads();
  s2sTypedEach<DT, LOGITS, CACHED, false>(row, V, lse, kr, [&](int i, uint32_t k) {
    const uint32_t ix = 0xFFFFu - (uint32_t)i;
    const bool sel = k != 0u && (all || (k & mskK) > preK || ((k & mskK) == preK && (ix & mskI) >= preI));
    if (sel || (i == P.eos && k != 0u)) {
      const float a = f32FromKey(k); /* (a zero comes back as +0: no score the step forms can tell the sign) */
      if (sel) {
        const uint32_t p = atomAdd32(&S.nList, 1u);
        if (p < (uint32_t)kS2sTypedMaxList) {
          S.listTok[p] = i;
          S.listAm[p] = a;
        }
      }
      if (i == P.eos) {
        S.eosIn = sel ? 1 : 0;
        S.eosA = a;
      }
    }
  });
  __syncthreads();
  const int n = (int)(S.nList < (uint32_t)kS2sTypedMaxList ? S.nList : (uint32_t)kS2sTypedMaxList);
  /* the shortcut kept fewer than the token beam: eos still is a candidate when it is among the row's Kt best */
  bool eosAdd = false;
  const float ae = S.eosA;
  if (P.eosExtra && !S.eosIn && P.eos >= 0 && P.eos < V) {
    const uint32_t ke = s2sKey32(ae);
    if (ke != 0u) {
      int above = 0;
      s2sTypedEach<DT, LOGITS, CACHED, false>(row, V, lse, kr, [&](int i, uint32_t k) {
        above += (k > ke || (k == ke && i < P.eos)) ? 1 : 0;
      });
      eosAdd = s2sBlockSum(S.wcnt, above) < P.Kt;
    }
  }
  /* written in token order (the rank of each token among the listed), eos after them */
  int32_t* tok = P.recTok + r * P.cap;
  float* am = P.recAm + r * P.cap;
  for (int e = tid; e < n; e += kS2sTypedThreads) {
    const int32_t te = S.listTok[e];
    int rank = 0;
    for (int q = 0; q < n; ++q) {
      rank += S.listTok[q] < te ? 1 : 0;
    }
    tok[rank] = te;
    am[rank] = S.listAm[e];
  }
  if (tid == 0) {
    if (eosAdd) {
      tok[n] = P.eos;
      am[n] = ae;
    }
    P.recN[r] = n + (eosAdd ? 1 : 0);
  }
}

/* workgroup = row b*K + k of the step */
template <int DT, bool LOGITS>
FLTX_DEV void s2sTypedRows(const S2sTypedParams& Q, char* smem) {
  const S2sParams& P = Q.s;
  const int64_t r = (int64_t)blockIdx.x;
  const int b = (int)(r / P.K), k = (int)(r % P.K);
  const bool live = !P.done[b] && k < P.nRowsInt[b] && (P.rowValid == nullptr || P.rowValid[r] != 0);
  if (!live) {
    if (threadIdx.x == 0) {
      P.recN[r] = 0;
      if (LOGITS && Q.rowLse) {
        Q.rowLse[r] = __longlong_as_double(0x7FF8000000000000ll);
      }
    }
    return;
  }
  S2sTypedLds& S = *(S2sTypedLds*)smem;
  if (P.V <= kS2sTypedReadOnceV) {
    s2sTypedRow<DT, LOGITS, true>(Q, S, r);
  } else {
    s2sTypedRow<DT, LOGITS, false>(Q, S, r);
  }
}

/* ---- the step: one workgroup of kS2sStepThreads per utterance ---------------------------------------------------- */
struct S2sStepLds {
  uint32_t hist[kSlNB];
  unsigned long long wmax[kS2sStepThreads / 64];
  int32_t wcnt[kS2sStepThreads / 64];
  int32_t rowOfHyp[kS2sMaxBeam]; /* hypothesis of the current beam -> its row in this step's call, -1: finished */
  int32_t hypOfRow[kS2sMaxBeam];
  uint32_t selIdx[kS2sMaxBeam];
  unsigned long long selKey[kS2sMaxBeam];
  int32_t order[kS2sMaxBeam];
  unsigned long long pre, msk;
  int32_t need, allEq, nSel, nSurv;
  int64_t eqCut;
  int32_t scanBstar, scanCum, scanCnt, scanTotal;
};

/* position of this thread's flag among the set flags of threads before it; *total = flags of the workgroup */
FLTX_DEV int s2sBlockRank(S2sStepLds& S, bool flag, int* total) {
  const int wave = waveId(), lane = laneId();
  const unsigned long long bl = waveBallot(flag);
  __syncthreads();
  if (lane == 0) {
    S.wcnt[wave] = popc64(bl);
  }
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < kS2sStepThreads / 64; ++w) {
    base += w < wave ? S.wcnt[w] : 0;
    all += S.wcnt[w];
  }
  *total = all;
  return base + wavePrefixCount(bl);
}

/* ---- the step's skeleton: what the lexicon-free step below and the lexicon step (fltx_s2s_lex.h) share. -------------
 * A decoder differs in its hypothesis / record types (template parameters) and in the values it hands in; every
 * function here is called by all kS2sStepThreads threads of the workgroup under uniform control flow (barriers). */

/* the order key of a score: NaN is never a candidate (0); +0.0: -0 and +0 compare equal, as the reference's doubles */
FLTX_DEV unsigned long long s2sScoreKey(double s) { return s == s ? f64Key(s + 0.0) : 0ull; }

/* a step that scores nothing (after the last one, a stopped utterance): no rows for the model */
FLTX_DEV void s2sIdleStep(const S2sParams& P, int b) {
  const int64_t rb = (int64_t)b * P.K;
  for (int k = (int)threadIdx.x; k < P.K; k += kS2sStepThreads) {
    P.outTok[rb + k] = -1;
    P.outBeam[rb + k] = -1;
    P.outSrc[rb + k] = -1;
  }
  if (threadIdx.x == 0) {
    P.outN[b] = 0;
  }
}

/* rows <-> hypotheses: the live ones (not ended by eos) of the current beam, in beam order */
template <typename Hyp>
FLTX_DEV void s2sMapRows(S2sStepLds& S, const Hyp* prev, int nPrev, int eos) {
  const int tid = (int)threadIdx.x;
  const bool isLive = tid < nPrev && prev[tid].token != eos;
  int tot;
  const int q = s2sBlockRank(S, isLive, &tot);
  if (tid < nPrev) {
    S.rowOfHyp[tid] = isLive ? q : -1;
    if (isLive) {
      S.hypOfRow[q] = tid;
    }
  }
  __syncthreads();
}

/* the largest of the threads' keys, in every thread */
FLTX_DEV unsigned long long s2sBlockMaxKey(S2sStepLds& S, unsigned long long mx) {
  mx = waveMax64(mx);
  if (laneId() == 0) {
    S.wmax[waveId()] = mx;
  }
  __syncthreads();
  for (int w = 0; w < kS2sStepThreads / 64; ++w) {
    mx = S.wmax[w] > mx ? S.wmax[w] : mx;
  }
  return mx;
}

/* threshold (candidatesAdd / candidatesStore: score >= best - beamThreshold, best over the whole step) as a key:
 * a candidate survives when its key is >= this one */
FLTX_DEV unsigned long long s2sThresholdKey(unsigned long long bestKey, double beamThreshold) {
  unsigned long long thrKey = 1ull;
  if (bestKey != 0ull) {
    const double thr = f64FromKey(bestKey) - beamThreshold;
    thrKey = thr == thr ? f64Key(thr + 0.0) : ~0ull;
    thrKey = thrKey == 0ull ? 1ull : thrKey;
  }
  return thrKey;
}

/* the K best of the utterance's keys cKey[0..n) (0: none), nSurv of them not 0: a radix select over the 64-bit keys,
 * then the selected sorted best first (returnSorted: Utils.h:204-216).  Leaves S.selIdx / S.selKey (the selected, in
 * no order) and S.order (rank -> position in those); returns how many */
FLTX_DEV int s2sSelectTopK(S2sStepLds& S, const unsigned long long* cKey, int64_t n, int K, int nSurv) {
  const int tid = (int)threadIdx.x, lane = laneId(), wave = waveId();
  unsigned long long pre = 0ull, msk = 0ull;
  bool all = nSurv <= K, allEq = false;
  int need = K;
  int64_t eqCut = -1;
  for (int shift = 56; shift >= 0 && !all && !allEq; shift -= 8) {
    __syncthreads();
    S.hist[tid] = 0u; /* (kS2sStepThreads == kSlNB) */
    __syncthreads();
    for (int64_t j = tid; j < n; j += kS2sStepThreads) {
      const unsigned long long key = cKey[j];
      if (key != 0ull && (key & msk) == pre) {
        atomAdd32(&S.hist[255u - (uint32_t)((key >> shift) & 255ull)], 1u);
      }
    }
    __syncthreads();
    if (wave == 0) {
      const SlScan sc = slScan(S.hist, need, false);
      if (lane == 0) {
        S.scanBstar = sc.bstar;
        S.scanCum = sc.cum;
        S.scanCnt = sc.cnt;
      }
    }
    __syncthreads();
    need -= S.scanCum;
    pre |= (unsigned long long)(255 - S.scanBstar) << shift;
    msk |= 255ull << shift;
    allEq = S.scanCnt == need;
  }
  if (!all && !allEq) { /* equal keys at the cut (exact ties of the double scores): the lower candidate indices --
                           * the need-th equal key in index order, 256 candidates per round */
    int seen = 0;
    for (int64_t j0 = 0; j0 < n && eqCut < 0; j0 += kS2sStepThreads) {
      const int64_t j = j0 + tid;
      const bool eq = j < n && cKey[j] == pre;
      int tot;
      const int r = s2sBlockRank(S, eq, &tot);
      if (eq && seen + r == need - 1) {
        S.eqCut = j;
      }
      __syncthreads();
      if (seen + tot >= need) {
        eqCut = S.eqCut;
      }
      seen += tot;
    }
  }
  if (tid == 0) {
    S.nSel = 0;
  }
  __syncthreads();
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    const unsigned long long key = cKey[j];
    const bool sel = key != 0ull && (all || (key & msk) > pre || ((key & msk) == pre && (allEq || j <= eqCut)));
    if (sel) {
      const uint32_t p = atomAdd32((uint32_t*)&S.nSel, 1u);
      if (p < (uint32_t)K) { /* (exactly K are selected; the bound only guards the list) */
        S.selIdx[p] = (uint32_t)j;
        S.selKey[p] = key;
      }
    }
  }
  __syncthreads();
  const int nSel = S.nSel < K ? S.nSel : K;
  if (tid < nSel) {
    const unsigned long long mk = S.selKey[tid];
    const uint32_t mi = S.selIdx[tid];
    int rank = 0;
    for (int q = 0; q < nSel; ++q) {
      const unsigned long long ok = S.selKey[q];
      rank += (ok > mk || (ok == mk && S.selIdx[q] < mi)) ? 1 : 0;
    }
    S.order[rank] = tid;
  }
  __syncthreads();
  return nSel;
}

/* the step's outcome: thread tid < nSel made hypothesis tid of the new beam, (token, parent), `isLive` when the model
 * extends it, from row `srcRow` of this call.  Writes the next call's rows and the utterance's bookkeeping */
struct S2sNoRowExtra { /* nothing more per listed row */
  __device__ __forceinline__ void put(int64_t) const {}
  __device__ __forceinline__ void none(int64_t) const {}
};

/* ... `extra` says what else a row of the next call's list gets: put(r) for the listed row r of this thread's
 * hypothesis, none(r) for a padding row (the lexicon step with word-level LM rows: next_word and the row's trie node).
 * lt: the steps the utterance had taken before this one (s2sLocalT; the CTC rows steps: the frame, P.t) */
template <typename Extra>
FLTX_DEV void s2sPublishStepWith(const S2sParams& P, S2sStepLds& S, int b, int lt, int nSel, bool isLive, int token,
                                 int parent, int srcRow, const Extra& extra) {
  const int tid = (int)threadIdx.x, K = P.K, par = P.t & 1;
  const int64_t rb = (int64_t)b * K;
  int nLive;
  const int q = s2sBlockRank(S, isLive, &nLive);
  const bool fin = nSel == 0 || nLive == 0 || lt + 1 >= P.maxOut;
  if (fin) {
    nLive = 0;
  }
  if (isLive && !fin) {
    P.outTok[rb + q] = token;
    P.outBeam[rb + q] = parent;
    P.outSrc[rb + q] = srcRow;
    extra.put(rb + q);
  }
  for (int k = nLive + tid; k < K; k += kS2sStepThreads) {
    P.outTok[rb + k] = -1;
    P.outBeam[rb + k] = -1;
    P.outSrc[rb + k] = -1;
    extra.none(rb + k);
  }
  if (tid == 0) {
    P.outN[b] = nLive;
    P.nRowsInt[b] = nLive;
    if (nSel > 0) {
      P.beamN[(par ^ 1) * P.B + b] = nSel;
    }
    if (fin) {
      P.done[b] = 1;
      P.finalStep[b] = nSel > 0 ? lt + 1 : lt; /* the last non-empty beam (:152-158; lexicon: :204-207) */
    }
  }
}

FLTX_DEV void s2sPublishStep(const S2sParams& P, S2sStepLds& S, int b, int lt, int nSel, bool isLive, int token,
                             int parent, int srcRow) {
  s2sPublishStepWith(P, S, b, lt, nSel, isLive, token, parent, srcRow, S2sNoRowExtra{});
}

/* decodeStep's start (:30-32): the root's fields that every hypothesis type has ... */
template <typename Hyp>
FLTX_DEV void s2sRootHyp(const S2sParams& P, Hyp& h) {
  h.score = 0.0;
  h.am = 0.0;
  h.lm = 0.0;
  h.token = -1;
  h.parent = -1;
  for (int j = 0; j < kS2sCtx; ++j) {
    h.ctx[j] = P.ctx0[j];
  }
}

/* ... and the utterance's state: a beam of one, the first call's single row (token -1, beam index -1, no source row) */
FLTX_DEV void s2sBeginReset(const S2sParams& P, int b) {
  const int64_t rb = (int64_t)b * P.K;
  P.beamN[b] = 1;
  const int live = P.maxOut > 0 ? 1 : 0;
  P.nRowsInt[b] = live;
  P.done[b] = live ? 0 : 1;
  P.finalStep[b] = 0;
  s2sOrigin(P)[b] = 0;
  s2sOrigin(P)[P.B + b] = 0;
  for (int k = 0; k < P.K; ++k) {
    P.outTok[rb + k] = -1;
    P.outBeam[rb + k] = -1;
    P.outSrc[rb + k] = -1;
  }
  P.outN[b] = live;
}

/* getAllFinalHypothesis (:160-163, Utils.h:230-266): the final beam's scores and paths, right-aligned in rows of
 * `len` = maxOutputLength + 3 with -1 in front; workgroup per utterance, thread per hypothesis.  `beams` / `hist` are
 * the decoder's own; `path` says where a record goes: none(at) writes -1 at element `at`, put(at, rec) the record,
 * returning its parent.  put takes the record BY VALUE: by reference, its fields may alias the rows it stores to, and
 * every field is loaded again after each store -- three dependent loads per step of the walk instead of one */
template <typename Hyp, typename Rec, typename Path>
FLTX_DEV void s2sBackTrace(const S2sParams& P, const Hyp* beams, const Rec* hist, const Path& path, int status) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int K = P.K;
  const int64_t rb = (int64_t)b * K;
  const int origin = s2sOrigin(P)[b];
  const int fs = P.done[b] ? P.finalStep[b] : P.t - origin;
  const int par = (origin + fs) & 1; /* (the half the final beam was written under) */
  const int n = P.beamN[par * P.B + b];
  const Hyp* beam = beams + (size_t)par * P.B * K + rb;
  const int len = P.len;
  for (int k = tid; k < n; k += kS2sEndThreads) {
    const Hyp& h = beam[k];
    double* sc = P.outScores + (rb + k) * 3;
    sc[0] = h.score;
    sc[1] = h.am;
    sc[2] = h.lm;
    const int64_t row = (rb + k) * len;
    for (int f = 0; f < len - fs; ++f) {
      path.none(row + f);
    }
    int p = k;
    for (int s = fs; s >= 1; --s) {
      const Rec rec = hist[(size_t)s * P.B * K + rb + p];
      p = path.put(row + len - 1 - (fs - s), rec);
    }
  }
  if (tid == 0) {
    P.outNHyp[b] = n;
    P.uttNBeam[b] = n;
    P.uttFrame[b] = len - 1;
    P.uttStatus[b] = status;
  }
}

/* ---- the lexicon-free step ------------------------------------------------------------------------------------ */
/* Where a candidate's LM score comes from is a template parameter, not a flag (see s2sLm): REC false: ZeroLM / the
 * n-gram tables (s2sLm); REC true: a rows LM, recLm[r * cap + e] as fltx_s2s_lm_rows_kernel gathered it -- no n-gram
 * context, ctx stays ctx0.  The step is instantiated once per source. */
/* candidate j of the utterance: row k = j / cap, entry e = j % cap for j < nRows*cap; then the carried hypotheses */
template <bool REC>
FLTX_DEV void s2sStepUtteranceOn(const S2sParams& P, char* smem, const float* recLm) {
  S2sStepLds& S = *(S2sStepLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int K = P.K;
  const int64_t rb = (int64_t)b * K;
  if (P.done[b]) { /* a step after the last one, a parked slot: nothing to score */
    s2sIdleStep(P, b);
    return;
  }
  const int par = P.t & 1;
  const S2sHyp* prev = P.beam + (size_t)par * P.B * K + rb;
  S2sHyp* next = P.beam + (size_t)(par ^ 1) * P.B * K + rb;
  const int nPrev = P.beamN[par * P.B + b];
  const int nRows = P.nRowsInt[b];
  const int cap = P.cap;
  /* 1. rows <-> hypotheses (the live ones in beam order: LexiconFreeSeq2SeqDecoder.cpp:44-55) */
  s2sMapRows(S, prev, nPrev, P.eos);
  /* 2. the candidates' keys and the best of the step */
  unsigned long long* cKey = P.cKey + (size_t)b * P.nC;
  const int64_t nRowC = (int64_t)nRows * cap, n = nRowC + nPrev;
  unsigned long long mx = 0ull;
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    unsigned long long key = 0ull;
    if (j < nRowC) {
      const int k = (int)(j / cap), e = (int)(j % cap);
      const int64_t r = rb + k;
      if (e < P.recN[r]) {
        const S2sHyp& h = prev[S.hypOfRow[k]];
        const int tok = P.recTok[r * cap + e];
        float lmS;
        if constexpr (REC) {
          lmS = recLm[r * cap + e];
        } else {
          lmS = s2sLm(P, h.ctx, tok, P.eos, nullptr);
        }
        key = s2sScoreKey(s2sScore(P, h, tok, P.recAm[r * cap + e], lmS));
      }
    } else {
      const S2sHyp& h = prev[j - nRowC];
      if (h.token == P.eos) { /* a finished hypothesis is carried unchanged (:68-82) */
        key = s2sScoreKey(h.score);
      }
    }
    cKey[j] = key;
    mx = key > mx ? key : mx;
  }
  /* 3. threshold */
  const unsigned long long thrKey = s2sThresholdKey(s2sBlockMaxKey(S, mx), P.beamThreshold);
  int surv = 0;
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    const unsigned long long key = cKey[j];
    if (key != 0ull && key < thrKey) {
      cKey[j] = 0ull;
    } else if (key != 0ull) {
      ++surv;
    }
  }
  /* 4. the K best survivors, sorted best first */
  const int nSel = s2sSelectTopK(S, cKey, n, K, s2sBlockSum(S.wcnt, surv));
  /* 5. the new beam, its history records and the next call's rows */
  const int lt = s2sLocalT(P, b); /* (loaded here, where the step first needs it: not kept across the search) */
  S2sHyp nh;
  bool isLive = false;
  int srcRow = -1, token = -1, parent = -1;
  if (tid < nSel) {
    const int64_t j = S.selIdx[S.order[tid]];
    if (j < nRowC) {
      const int k = (int)(j / cap), e = (int)(j % cap);
      const int64_t r = rb + k;
      const int i = S.hypOfRow[k];
      const S2sHyp& h = prev[i];
      const int tok = P.recTok[r * cap + e];
      const float a = P.recAm[r * cap + e];
      nh = h;
      float lmS;
      if constexpr (REC) {
        lmS = recLm[r * cap + e];
      } else {
        lmS = s2sLm(P, h.ctx, tok, P.eos, tok == P.eos ? nullptr : nh.ctx);
      }
      nh.score = s2sScore(P, h, tok, a, lmS);
      nh.am = h.am + (double)a;
      nh.lm = h.lm + (double)lmS;
      nh.token = tok;
      nh.parent = i;
      isLive = tok != P.eos;
      srcRow = (int)rb + k;
    } else {
      const int i = (int)(j - nRowC);
      nh = prev[i];
      nh.parent = i;
    }
    next[tid] = nh;
    P.hist[(size_t)(lt + 1) * P.B * K + rb + tid] = make_int2(nh.token, nh.parent);
    token = nh.token;
    parent = nh.parent;
  }
  s2sPublishStep(P, S, b, lt, nSel, isLive, token, parent, srcRow);
}

FLTX_DEV void s2sStepUtterance(const S2sParams& P, char* smem) { s2sStepUtteranceOn<false>(P, smem, nullptr); }

FLTX_DEV void s2sBeginUtterance(const S2sParams& P, char*) {
  const int b = (int)(blockIdx.x * kS2sBeginThreads + threadIdx.x);
  if (b >= P.B) {
    return;
  }
  S2sHyp h;
  s2sRootHyp(P, h);
  h.pad = 0;
  P.beam[(int64_t)b * P.K] = h;
  s2sBeginReset(P, b);
}

struct S2sPath { /* a path's records: the tokens row */
  int32_t* tokens;
  __device__ __forceinline__ void none(int64_t at) const { tokens[at] = -1; }
  __device__ __forceinline__ int put(int64_t at, int2 rec) const {
    tokens[at] = rec.x;
    return rec.y;
  }
};

FLTX_DEV void s2sEndUtterance(const S2sParams& P, char*) {
  s2sBackTrace(P, P.beam, P.hist, S2sPath{P.tokens}, 0);
}

/* ---- fltx_s2s_finish: end the utterances of named slots, restart or park those slots -------------------------------------
 * One workgroup of kS2sEndThreads per slot, by which[b]:
 *   0  the slot is left alone: nothing of it is written.  Its rows are listed again from its current beam -- the live
 *      hypotheses in beam order, which is the order the last step listed them in (s2sMapRows / s2sPublishStepWith), with
 *      their token and parent; next_src_row is the row itself, so the model's index_select is the identity for it;
 *   1  s2sBackTrace for this utterance alone into the finish's own result buffers (P.outScores / tokens / outNHyp /
 *      uttStatus are those), then the slot is what the begin kernel leaves: the root in the CURRENT half of the beam,
 *      origin[b] = t (local step 0), done cleared, one row listed;
 *   2  the same back-trace, then the slot is parked: done, no rows, an empty beam (fltx_s2s_end: n_hyp 0).
 * A parked slot has no utterance: named, it reports n_hyp 0, steps 0, status 0; 1 restarts it, 2 leaves it parked.
 * The back-trace's reads of the beam and the root's store are ordered by the workgroup's barrier.
 * `kind` is the decoder's: root(h) the root hypothesis; restart(b) / park(b) the rest of the utterance's state (the
 * lexicon kind's state table and counters), called by every thread; listed(r, h) / padding(r) what else a listed row
 * gets (next_word). */
struct S2sFinishParams {
  const int32_t* which; /* [B] */
  int32_t* steps;       /* [B] local steps the finished utterance took */
  int32_t errUnsupported; /* the FLTX_ERR_* of a stopped utterance's status */
};

struct S2sFinishLds {
  int32_t wcnt[kS2sEndThreads / 64];
};

static_assert(kS2sMaxBeam <= kS2sEndThreads, "s2sFinishSlot: a thread per hypothesis of the beam");

template <typename Hyp, typename Rec, typename Path, typename Kind>
FLTX_DEV void s2sFinishSlot(const S2sParams& P, const S2sFinishParams& F, S2sFinishLds& S, Hyp* beams, const Rec* hist,
                            const Path& path, int status, const Kind& kind) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int K = P.K, par = P.t & 1;
  const int64_t rb = (int64_t)b * K;
  const int w = F.which[b];
  const bool parked = s2sOrigin(P)[P.B + b] != 0;
  Hyp* cur = beams + (size_t)par * P.B * K + rb;
  if (w == 0) {
    const int nRows = P.done[b] ? 0 : P.nRowsInt[b];
    const int nCur = nRows > 0 ? P.beamN[par * P.B + b] : 0;
    const Hyp h = cur[tid < nCur ? tid : 0];
    const bool isLive = tid < nCur && h.token != P.eos;
    const unsigned long long bl = waveBallot(isLive);
    if (laneId() == 0) {
      S.wcnt[waveId()] = popc64(bl);
    }
    __syncthreads();
    int q = wavePrefixCount(bl);
    for (int v = 0; v < waveId(); ++v) {
      q += S.wcnt[v];
    }
    if (isLive && q < nRows) {
      P.outTok[rb + q] = h.token;
      P.outBeam[rb + q] = h.parent;
      P.outSrc[rb + q] = (int32_t)(rb + q);
      kind.listed(rb + q, h);
    }
    for (int k = nRows + tid; k < K; k += kS2sEndThreads) {
      P.outTok[rb + k] = -1;
      P.outBeam[rb + k] = -1;
      P.outSrc[rb + k] = -1;
      kind.padding(rb + k);
    }
    if (tid == 0) {
      P.outN[b] = nRows;
      P.outNHyp[b] = 0;
      F.steps[b] = 0;
      P.uttStatus[b] = 0;
    }
    return;
  }
  if (!parked) {
    const int fs = P.done[b] ? P.finalStep[b] : s2sLocalT(P, b);
    s2sBackTrace(P, beams, hist, path, status);
    if (tid == 0) {
      F.steps[b] = fs;
    }
  } else if (tid == 0) {
    P.outNHyp[b] = 0;
    F.steps[b] = 0;
    P.uttStatus[b] = 0;
  }
  for (int k = tid; k < K; k += kS2sEndThreads) {
    P.outTok[rb + k] = -1;
    P.outBeam[rb + k] = -1;
    P.outSrc[rb + k] = -1;
    kind.padding(rb + k);
  }
  if (w == 2 && parked) {
    if (tid == 0) {
      P.outN[b] = 0;
    }
    return;
  }
  __syncthreads();
  if (w == 1) {
    const int live = P.maxOut > 0 ? 1 : 0;
    if (tid == 0) {
      Hyp root;
      kind.root(P, root);
      cur[0] = root;
      P.beamN[par * P.B + b] = 1;
      P.nRowsInt[b] = live;
      P.done[b] = live ? 0 : 1;
      P.finalStep[b] = 0;
      s2sOrigin(P)[b] = P.t;
      s2sOrigin(P)[P.B + b] = 0;
      P.outN[b] = live;
    }
    kind.restart(b);
  } else {
    if (tid == 0) {
      P.beamN[par * P.B + b] = 0;
      P.nRowsInt[b] = 0;
      P.done[b] = 1;
      P.finalStep[b] = 0;
      s2sOrigin(P)[b] = P.t;
      s2sOrigin(P)[P.B + b] = 1;
      P.outN[b] = 0;
    }
    kind.park(b);
  }
}

struct S2sFinishKind { /* the lexicon-free decoder: the beam is all there is */
  __device__ __forceinline__ void root(const S2sParams& P, S2sHyp& h) const {
    s2sRootHyp(P, h);
    h.pad = 0;
  }
  __device__ __forceinline__ void restart(int) const {}
  __device__ __forceinline__ void park(int) const {}
  __device__ __forceinline__ void listed(int64_t, const S2sHyp&) const {}
  __device__ __forceinline__ void padding(int64_t) const {}
};

struct S2sFinishKernelParams {
  S2sParams s;
  S2sFinishParams f;
};

FLTX_DEV void s2sFinishUtterance(const S2sFinishKernelParams& Z, char* smem) {
  s2sFinishSlot(Z.s, Z.f, *(S2sFinishLds*)smem, Z.s.beam, Z.s.hist, S2sPath{Z.s.tokens}, 0, S2sFinishKind{});
}

/* ---- a rows LM (fltx_lm_rows_create): the LM's answers arrive as rows next to the model's ------------------------------
 * Shallow fusion with an LM that scores a whole vocabulary per state (ConvLM.cpp:120-141's shape): like the emitting
 * model it runs between two steps and leaves row b*K + k = LM::score(state of that hypothesis, v) for every LM index v;
 * its state is carried by index_select(next_src_row) as the model's is.  Every hypothesis has its own prefix, hence its
 * own LM state, so -- as for KenLM above -- candidatesStore's merge cannot fire: no state table, no merges.
 *
 * fltx_s2s_lm_rows_kernel runs after the front end (either of the two, unchanged) and before the step: for every entry
 * of a live row's record it writes the LM score of that token into recLm, a float: the LM row's element at
 * usrToLm[token] (at finishIdx for eos: LM::finish), widened exactly; with logits, (float)((double)x - lse) with lse
 * the LM row's log-sum-exp as the typed front end defines it.  The step then is s2sStepUtteranceOn<S2sLmRecords>.
 *   log-probs: a pure gather -- one wave per row, four rows per workgroup, <= cap elements of the row are read;
 *   logits:    one workgroup per row: the row is read once with 16-byte loads (element-wise up to the first 16-byte
 *              boundary and after the last) and kept in registers between the max and the sum pass when it has at most
 *              kS2sLmVecs * 256 vectors; wider rows are read once per pass.  The sum is the typed front end's: f32 exp
 *              summed in double per thread in a fixed order, the same butterfly per wave, the waves in order. */
constexpr int kS2sLmThreads = 256;
constexpr int kS2sLmVecs = 16; /* 16-byte vectors per thread kept in registers: 32 768 2-byte / 16 384 4-byte elements */

struct S2sLmRowsParams {
  S2sParams s;            /* (s.scores is not read) */
  const void* x;          /* the LM's rows: element (r, i) at x + (r * rowStride + i) elements */
  int64_t rowStride;
  int32_t width;          /* entries per LM row */
  int32_t finishIdx;      /* the LM index LM::finish reads */
  const int32_t* usrToLm; /* [>= V] or null: identity */
  float* recLm;           /* [B*K][cap] */
  double* rowLse;         /* [B*K] or null: logits mode writes lse (live rows) or NaN */
};

struct S2sLmRowsLds {
  double wsum[kS2sLmThreads / 64];
  uint32_t wmax[kS2sLmThreads / 64];
};

FLTX_DEV bool s2sRowLive(const S2sParams& P, int64_t r) {
  const int b = (int)(r / P.K), k = (int)(r % P.K);
  return !P.done[b] && k < P.nRowsInt[b] && (P.rowValid == nullptr || P.rowValid[r] != 0);
}

/* the LM scores of row r's record: entry e by thread `tid` of `nThreads` */
template <int DT, bool LOGITS>
FLTX_DEV void s2sLmGather(const S2sLmRowsParams& Q, int64_t r, const void* row, double lse, int tid, int nThreads) {
  const S2sParams& P = Q.s;
  const int n = P.recN[r];
  for (int e = tid; e < n; e += nThreads) {
    const int tok = P.recTok[r * P.cap + e];
    const int idx = tok == P.eos ? Q.finishIdx : (Q.usrToLm ? Q.usrToLm[tok] : tok);
    float v = __uint_as_float(0x7FC00000u); /* (an index outside the row -- fltx_s2s_begin refuses those -- is no candidate) */
    if (idx >= 0 && idx < Q.width) {
      v = s2sTypedScore<DT, LOGITS>(row, idx, lse);
    }
    Q.recLm[r * P.cap + e] = v;
  }
}

/* log-probs: workgroup = four waves, wave = row b*K + k of the step */
template <int DT>
FLTX_DEV void s2sLmRowsGather(const S2sLmRowsParams& Q, char*) {
  const S2sParams& P = Q.s;
  const int wave = waveUniform(waveId());
  const int64_t r = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
  if (r >= (int64_t)P.B * P.K || !s2sRowLive(P, r)) {
    return; /* (the record of a row that is not live is empty: the step reads no recLm of it) */
  }
  const void* row = (const char*)Q.x + r * Q.rowStride * (DT == kS2sDtF32 ? 4 : 2);
  s2sLmGather<DT, false>(Q, r, row, 0.0, laneId(), 64);
}

/* f(raw key) for the j-th element of a 16-byte vector */
template <int DT>
FLTX_DEV uint32_t s2sVecKey(const uint4& v, int j) {
  if constexpr (DT == kS2sDtF32) {
    const uint32_t w = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
    return s2sRawKey(__uint_as_float(w));
  } else {
    const uint32_t w = (j >> 1) == 0 ? v.x : (j >> 1) == 1 ? v.y : (j >> 1) == 2 ? v.z : v.w;
    const uint32_t h = (j & 1) ? w >> 16 : w & 0xFFFFu;
    return s2sRawKey(DT == kS2sDtF16 ? s2sWidenF16(h) : __uint_as_float(h << 16));
  }
}

/* f(raw key) for every element of the row this thread holds, in a fixed order: the head and tail elements (one per
 * thread at most), then its vectors -- from the registers (CACHED) or from memory */
template <int DT, bool CACHED, typename F>
FLTX_DEV void s2sLmEach(const void* row, int nEdge, int edgeAt, const uint4* body, int nVec, const uint4* vr, F&& f) {
  constexpr int kPer = DT == kS2sDtF32 ? 4 : 8;
  const int tid = (int)threadIdx.x;
  if (tid < nEdge) {
    f(s2sRawKey(s2sElem<DT>(row, edgeAt)));
  }
  if constexpr (CACHED) {
#pragma unroll
    for (int q = 0; q < kS2sLmVecs; ++q) {
      if (q * kS2sLmThreads < nVec && tid + q * kS2sLmThreads < nVec) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          f(s2sVecKey<DT>(vr[q], j));
        }
      }
    }
  } else {
    for (int i = tid; i < nVec; i += kS2sLmThreads) {
      const uint4 v = body[i];
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        f(s2sVecKey<DT>(v, j));
      }
    }
  }
}

template <int DT, bool CACHED>
FLTX_DEV double s2sLmRowLse(const S2sLmRowsParams& Q, S2sLmRowsLds& S, const void* row) {
  constexpr int kElem = DT == kS2sDtF32 ? 4 : 2, kPer = 16 / kElem;
  const int tid = (int)threadIdx.x, lane = laneId(), wave = waveId();
  const int W = Q.width;
  /* head: the elements before the first 16-byte boundary; body: whole vectors; tail: the rest */
  int nHead = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) / kElem);
  nHead = nHead < W ? nHead : W;
  const int nVec = (W - nHead) / kPer, nTail = W - nHead - nVec * kPer;
  const uint4* body = (const uint4*)((const char*)row + (size_t)nHead * kElem);
  const int nEdge = nHead + nTail; /* < 2 * kPer <= kS2sLmThreads */
  const int edgeAt = tid < nHead ? tid : nHead + nVec * kPer + (tid - nHead);
  uint4 vr[CACHED ? kS2sLmVecs : 1];
  if constexpr (CACHED) {
#pragma unroll
    for (int q = 0; q < kS2sLmVecs; ++q) {
      if (q * kS2sLmThreads < nVec && tid + q * kS2sLmThreads < nVec) {
        vr[q] = body[tid + q * kS2sLmThreads];
      }
    }
  }
  uint32_t mk = 0u;
  s2sLmEach<DT, CACHED>(row, nEdge, edgeAt, body, nVec, vr, [&](uint32_t k) { mk = k > mk ? k : mk; });
  mk = waveMax32(mk);
  if (lane == 0) {
    S.wmax[wave] = mk;
  }
  __syncthreads();
  for (int w = 0; w < kS2sLmThreads / 64; ++w) {
    mk = S.wmax[w] > mk ? S.wmax[w] : mk;
  }
  const float mx = mk != 0u ? f32FromKey(mk) : -__builtin_huge_valf();
  double lse = (double)mx;
  if (mx - mx == 0.0f) { /* finite */
    double s = 0.0;
    s2sLmEach<DT, CACHED>(row, nEdge, edgeAt, body, nVec, vr, [&](uint32_t k) {
      if (k != 0u) {
        s += (double)expf(f32FromKey(k) - mx);
      }
    });
    for (int d = 32; d >= 1; d >>= 1) { /* (the typed front end's butterfly: the same sum in every lane, run to run) */
      s += __longlong_as_double((long long)waveShflXor64((unsigned long long)__double_as_longlong(s), d));
    }
    if (lane == 0) {
      S.wsum[wave] = s;
    }
    __syncthreads();
    s = 0.0;
    for (int w = 0; w < kS2sLmThreads / 64; ++w) {
      s += S.wsum[w];
    }
    lse = (double)mx + log(s);
  }
  return lse;
}

/* logits: workgroup = row b*K + k of the step */
template <int DT>
FLTX_DEV void s2sLmRowsLogits(const S2sLmRowsParams& Q, char* smem) {
  const S2sParams& P = Q.s;
  const int64_t r = (int64_t)blockIdx.x;
  if (!s2sRowLive(P, r)) {
    if (threadIdx.x == 0 && Q.rowLse) {
      Q.rowLse[r] = __longlong_as_double(0x7FF8000000000000ll);
    }
    return;
  }
  S2sLmRowsLds& S = *(S2sLmRowsLds*)smem;
  const void* row = (const char*)Q.x + r * Q.rowStride * (DT == kS2sDtF32 ? 4 : 2);
  constexpr int kPer = DT == kS2sDtF32 ? 4 : 8;
  const double lse = Q.width <= kS2sLmVecs * kS2sLmThreads * kPer ? s2sLmRowLse<DT, true>(Q, S, row)
                                                                   : s2sLmRowLse<DT, false>(Q, S, row);
  if (Q.rowLse && threadIdx.x == 0) {
    Q.rowLse[r] = lse;
  }
  s2sLmGather<DT, true>(Q, r, row, lse, (int)threadIdx.x, kS2sLmThreads);
}

template <int DT, bool LOGITS>
FLTX_DEV void s2sLmRows(const S2sLmRowsParams& Q, char* smem) {
  if constexpr (LOGITS) {
    s2sLmRowsLogits<DT>(Q, smem);
  } else {
    s2sLmRowsGather<DT>(Q, smem);
  }
}

/* the step with the LM term from the records */
FLTX_DEV void s2sStepUtteranceLmRows(const S2sLmRowsParams& Q, char* smem) {
  s2sStepUtteranceOn<true>(Q.s, smem, Q.recLm);
}

} // namespace fltx
