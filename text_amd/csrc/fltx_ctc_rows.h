/*
 * fltx_ctc_rows.h -- the lexicon-free CTC beam search (LexiconFreeDecoder.cpp:20-158) with a token-level rows LM
 * (fltx_lm_rows_create) as a batched device step per frame, beside the seq2seq steps of fltx_s2s.h / fltx_s2s_lex.h
 * whose front end, LM-row passes, merge, selection and publisher it reuses.
 *
 * The emissions of all frames are known at the start, so the token beams do not wait for the LM:
 *   fltx_ctc_rows_tokbeam_kernel  once, at begin: one wave per (utterance, frame), s2sTokBeamRow on the frame's N
 *                                 emissions -- its min(Kt, N) largest, ties to the lower token -- as a record of the frame.
 * A frame step is two kernels:
 *   fltx_ctc_rows_lm_kernel       per row b*K + k of the current beams (every hypothesis is live in CTC) and kept token of
 *                                 the utterance's frame one float into recLm[row][e]: the entry at usrToLm[token] of the LM
 *                                 row lmRowOf names (log-probs: a wave per row; logits: a workgroup per row, s2sLmRowLse);
 *   fltx_ctc_rows_step_kernel     one workgroup per utterance: the nPrev x cap candidates by the three CTC branches
 *                                 (:64-110), the threshold, the merge of candidates equal in (LM state, token, prevBlank)
 *                                 (crMergeCandidates), s2sSelectTopK, the state id of the survivors that entered a new
 *                                 state, the history record, and the next call's rows through s2sPublishStepWith.
 * decodeEnd (:127-158) is the same two kernels' finish variant: the gather reads the finish index of every row, the step
 * makes one candidate per hypothesis in state child(sid, -1), merges, sorts, and walks the history into the result layout
 * fltx_decode_batch writes (T[b] + 2 tokens per hypothesis, the root's sil first and decodeEnd's sil last; frames decoded
 * so far + 2 when the caller ends early).
 *
 * LM states.  LMState::child gives one object per (parent state, token), so the state of a hypothesis is the token string
 * CTC collapses its path to.  As in the lexicon seq2seq step a hypothesis carries a canonical id `sid` and the (parent
 * sid, edge) pair that made it; ids come from the utterance's lookup-or-insert table, which lives for the whole decode: a
 * state left and entered again gets its old id, so the caller can keep one LM row per id.  A full table stops the
 * utterance with ST_TABLE_FULL.
 *
 * An utterance whose frames are used up keeps its beam (parity T[b] & 1) and lists it again at every later step.
 */
#pragma once

namespace fltx {

struct CrHyp { /* one hypothesis of a beam, 48 B */
  double score, am, lm;
  int32_t token;     /* the frame's token (the root: sil) */
  int32_t parent;    /* index in the previous beam */
  int32_t sid;       /* canonical LM state */
  int32_t psid, edge; /* the state is child(psid, edge); (-1, -1): LM::start */
  int32_t prevBlank;
};

struct CrParams {
  S2sParams s; /* B, K, Kt, V = N, cap = mSel = min(Kt, N), eos = -1, maxOut = INT32_MAX (no step is the publisher's last),
                * t = frames stepped; recTok / recAm / recN: the FRAME records [sum T][cap]; cKey, nC = K * cap; beamN,
                * nRowsInt, done (1: the utterance stopped -- no candidate left, or a full table), finalStep; the outputs */
  int32_t sil, blank, logAdd;
  double silScore;
  const int32_t* T;        /* [B] frames */
  const int64_t* frameOff; /* [B + 1] first frame record of the utterance */
  const int64_t* emOff;    /* [B] first emission (in floats) of the utterance */
  const float* emissions;
  CrHyp* beam;             /* [2][B*K] */
  int2* hist;              /* [maxT + 2][B*K]: (token, parent) of the hypotheses after s frames */
  double* cScore;          /* [B][nC] */
  uint4* cMk;              /* [B][nC]: merge key (state pair, token, prevBlank) */
  int32_t *cGrp, *cList, *cNext;
  int32_t* mTab;           /* [B][mSize] */
  int32_t mSize;
  unsigned long long* sKey; /* [B][sSize]: (parent sid, edge) -> sid; ~0: empty */
  int32_t* sVal;
  int32_t* sCount;         /* [B] states handed out */
  int32_t sSize, sMax;
  int32_t* status;         /* [B] ST_* */
  int32_t* merges;         /* [B] */
  const float* recLm;      /* [B*K][cap] */
  int32_t* outState;       /* the caller's next_state [B*K] */
  const int64_t* histOff;  /* end: [B] first result token of the utterance */
};

/* the beam an utterance reads at step t: the one after min(t, T[b]) frames */
FLTX_DEV int crParity(const CrParams& Q, int b) {
  const int tb = Q.T[b];
  return (Q.s.t < tb ? Q.s.t : tb) & 1;
}

/* what a stream (fltx_ctc_rows_stream_begin, fltx_ctc_rows_stream.h) adds: there s.t, T, frameOff and emOff are those of
 * the current CHUNK, every stream counts its own frames, and the history is a ring.  beamN holds a stream's count in
 * both of its slots, so the gathers -- which take the slot from the chunk's t -- run as they are. */
struct CrsParams {
  int32_t* nDec;  /* [B] frames decoded since begin: the beam's parity, the history row (nDec % ring) */
  int32_t* base;  /* [B] frames pruned off: the buffer holds frames base .. nDec */
  int32_t ring;   /* rows of the two rings */
  double* sHist;  /* [ring][B*K][3]: (score, am, lm) of the hypotheses after s frames */
  /* what fltx_ctc_rows_stream_collect recycles ids with (fltx_ctc_rows_stream.h) */
  int32_t* sPar;   /* [B][sMax] the parent id of state id's table entry; -1: allocated without an entry; -2: free */
  int32_t* sEdge;  /* [B][sMax] the entry's edge */
  int32_t* sFree;  /* [B][sMax] the stack of free ids below the high-water mark sCount */
  int32_t* sFreeN; /* [B] ids on the stack */
};

/* a stream's step hands out an id for the state child(psid, edge): one off the free stack (fltx_ctc_rows_stream_collect
 * put it there) while there is one, else the next unused one; >= Q.sMax: the table is full.  The threads of a step pop
 * concurrently, so the count may pass below zero: crsClaimDone puts it right behind the step's barrier. */
FLTX_DEV int32_t crsClaimId(const CrParams& Q, const CrsParams& X, int b, int32_t psid, int32_t edge) {
  int32_t v;
  const int32_t f = (int32_t)atomAdd32((uint32_t*)&X.sFreeN[b], 0xFFFFFFFFu);
  if (f > 0) {
    v = (int32_t)loadCoherent32((const uint32_t*)&X.sFree[(size_t)b * Q.sMax + f - 1]);
  } else {
    v = (int32_t)atomAdd32((uint32_t*)&Q.sCount[b], 1u);
  }
  if (v < Q.sMax) {
    X.sPar[(size_t)b * Q.sMax + v] = psid;
    X.sEdge[(size_t)b * Q.sMax + v] = edge;
  }
  return v;
}

FLTX_DEV void crsClaimDone(const CrsParams& X, int b) {
  if (threadIdx.x == 0 && (int32_t)loadCoherent32((const uint32_t*)&X.sFreeN[b]) < 0) {
    X.sFreeN[b] = 0;
  }
}

/* the frames stream b has decoded, and its beam's parity */
template <bool STREAM>
FLTX_DEV int crStepParity(const CrParams& Q, const CrsParams* X, int b, int& nd) {
  if constexpr (STREAM) {
    nd = X->nDec[b];
    return nd & 1;
  } else {
    nd = 0;
    return crParity(Q, b);
  }
}

/* a stream's step is over: the count in both slots of beamN, the scores into their ring, one frame more */
template <typename Hyp>
FLTX_DEV void crsStepDone(const CrParams& Q, const CrsParams& X, int b, int nd, int nSel, const Hyp& nh) {
  const S2sParams& P = Q.s;
  const int tid = (int)threadIdx.x;
  if (tid < nSel) {
    double* sc = X.sHist + ((size_t)((nd + 1) % X.ring) * P.B * P.K + (size_t)b * P.K + tid) * 3;
    sc[0] = nh.score;
    sc[1] = nh.am;
    sc[2] = nh.lm;
  }
  if (tid == 0) { /* (nSel == 0 -- every candidate NaN: the frame counts and its beam is empty, as in the reference; the
                   * publisher has stopped the stream, best answers with an empty result) */
    P.beamN[b] = nSel;
    P.beamN[P.B + b] = nSel;
    X.nDec[b] = nd + 1;
  }
}

/* ---- front end: the token beam of every frame, once ------------------------------------------------------------------ */
/* the utterance of frame record fr: the last one whose first record is <= fr (utterances without frames share theirs) */
FLTX_DEV int crFrameUtterance(const CrParams& Q, int64_t fr) {
  int lo = 0, hi = Q.s.B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (Q.frameOff[mid] <= fr) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return waveUniform(lo);
}

/* workgroup = four waves, wave = frame record fr of the batch */
FLTX_DEV void crTokBeamRows(const CrParams& Q, char* smem) {
  const S2sParams& P = Q.s;
  const int wave = waveUniform(waveId());
  const int64_t fr = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
  if (fr >= Q.frameOff[P.B]) {
    return;
  }
  const int b = crFrameUtterance(Q, fr);
  const float* row = Q.emissions + Q.emOff[b] + (fr - Q.frameOff[b]) * (int64_t)P.V;
  S2sFrontLds& S = ((S2sFrontLds*)smem)[wave];
  s2sTokBeamRow(P, S, row, P.recTok + fr * P.cap, P.recAm + fr * P.cap, P.recN + fr);
}

/* ---- the gather: the LM entries of the frame's kept tokens, per row ---------------------------------------------------- */
struct CrLmParams {
  S2sLmRowsParams r;      /* r.s: CrParams::s; r.x / rowStride / width / finishIdx / usrToLm / rowLse: the LM's rows;
                           * r.recLm: [B*K][cap] */
  const int32_t* T;
  const int64_t* frameOff;
  const int32_t* lmRowOf; /* [B*K] or null (identity): the LM row of each decoder row */
  int32_t nLmRows;
  int32_t fin;            /* decodeEnd: one entry per row, the finish index */
};

/* row r holds a hypothesis that this call scores */
FLTX_DEV bool crRowLive(const CrLmParams& W, int64_t r) {
  const S2sParams& P = W.r.s;
  const int b = (int)(r / P.K), k = (int)(r % P.K);
  const int tb = W.T[b];
  if (P.done[b] || (!W.fin && P.t >= tb)) {
    return false;
  }
  return k < P.beamN[((P.t < tb ? P.t : tb) & 1) * P.B + b];
}

/* the LM row of decoder row r; null: none */
template <int DT>
FLTX_DEV const void* crLmRow(const CrLmParams& W, int64_t r) {
  const int64_t lr = W.lmRowOf ? (int64_t)W.lmRowOf[r] : r;
  if (lr < 0 || lr >= (int64_t)W.nLmRows) {
    return nullptr;
  }
  return (const char*)W.r.x + lr * W.r.rowStride * (DT == kS2sDtF32 ? 4 : 2);
}

template <int DT, bool LOGITS>
FLTX_DEV void crLmGather(const CrLmParams& W, int64_t r, const void* row, double lse, int tid, int nThreads) {
  const S2sLmRowsParams& Q = W.r;
  const S2sParams& P = Q.s;
  const int b = (int)(r / P.K);
  const int64_t fr = W.frameOff[b] + P.t;
  const int n = W.fin ? 1 : P.recN[fr];
  for (int e = tid; e < n; e += nThreads) {
    int idx = Q.finishIdx;
    if (!W.fin) {
      const int tok = P.recTok[fr * P.cap + e];
      idx = Q.usrToLm ? Q.usrToLm[tok] : tok;
    }
    float v = __uint_as_float(0x7FC00000u);
    if (row != nullptr && idx >= 0 && idx < Q.width) {
      v = s2sTypedScore<DT, LOGITS>(row, idx, lse);
    }
    Q.recLm[r * P.cap + e] = v;
  }
}

template <int DT, bool LOGITS>
FLTX_DEV void crLmRows(const CrLmParams& W, char* smem) {
  const S2sLmRowsParams& Q = W.r;
  const S2sParams& P = Q.s;
  if constexpr (!LOGITS) { /* workgroup = four waves, wave = row b*K + k */
    const int wave = waveUniform(waveId());
    const int64_t r = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
    if (r >= (int64_t)P.B * P.K || !crRowLive(W, r)) {
      return;
    }
    crLmGather<DT, false>(W, r, crLmRow<DT>(W, r), 0.0, laneId(), 64);
  } else { /* workgroup = row b*K + k */
    const int64_t r = (int64_t)blockIdx.x;
    const bool live = crRowLive(W, r);
    const void* row = live ? crLmRow<DT>(W, r) : nullptr;
    if (row == nullptr) {
      if (threadIdx.x == 0 && Q.rowLse) {
        Q.rowLse[r] = __longlong_as_double(0x7FF8000000000000ll);
      }
      if (live) {
        crLmGather<DT, true>(W, r, nullptr, 0.0, (int)threadIdx.x, kS2sLmThreads);
      }
      return;
    }
    S2sLmRowsLds& S = *(S2sLmRowsLds*)smem;
    constexpr int kPer = DT == kS2sDtF32 ? 4 : 8;
    const double lse = Q.width <= kS2sLmVecs * kS2sLmThreads * kPer ? s2sLmRowLse<DT, true>(Q, S, row)
                                                                     : s2sLmRowLse<DT, false>(Q, S, row);
    if (Q.rowLse && threadIdx.x == 0) {
      Q.rowLse[r] = lse;
    }
    crLmGather<DT, true>(W, r, row, lse, (int)threadIdx.x, kS2sLmThreads);
  }
}

/* ---- the step ------------------------------------------------------------------------------------------------------- */
struct CrCand {
  double score;
  float am, lmS;
  int32_t hyp; /* index in the previous beam */
  int32_t token, prevBlank;
  bool isNew;  /* the state is child(prev.sid, edge) */
  int32_t edge;
};

/* candidate j of the utterance: hypothesis k = j / cap and entry e = j % cap of the frame's record (LexiconFreeDecoder.cpp
 * :54-111, the same double operations in the same order); FIN: hypothesis j, decodeEnd's (:129-147).  false: none */
template <bool FIN>
FLTX_DEV bool crCand(const CrParams& Q, const CrHyp* prev, int64_t fr, int nE, int64_t rb, int64_t j, CrCand& c) {
  const S2sParams& P = Q.s;
  const int cap = P.cap;
  if constexpr (FIN) {
    const CrHyp& h = prev[j];
    c.hyp = (int)j;
    c.am = 0.0f;
    c.lmS = Q.recLm[(rb + j) * cap];
    c.score = h.score + P.lmWeight * (double)c.lmS;
    c.token = Q.sil;
    c.prevBlank = 0;
    c.isNew = true;
    c.edge = -1;
    return true;
  } else {
    const int k = (int)(j / cap), e = (int)(j % cap);
    if (e >= nE) {
      return false;
    }
    const CrHyp& h = prev[k];
    const int tok = P.recTok[fr * cap + e];
    const float a = P.recAm[fr * cap + e];
    double score = h.score + (double)a;
    if (tok == Q.sil) {
      score += Q.silScore;
    }
    c.hyp = k;
    c.am = a;
    c.token = tok;
    c.edge = tok;
    if (tok != Q.blank && (tok != h.token || h.prevBlank)) { /* a new token: the LM's entry, the child state */
      c.lmS = Q.recLm[(rb + k) * cap + e];
      c.score = score + P.lmWeight * (double)c.lmS;
      c.isNew = true;
      c.prevBlank = 0;
    } else { /* a blank, or a repeat without a blank in between: the state is the parent's */
      c.lmS = 0.0f;
      c.score = score;
      c.isNew = false;
      c.prevBlank = tok == Q.blank ? 1 : 0;
    }
    return true;
  }
}

/* the merge key: (the state's (parent sid, edge), token, prevBlank) -- compareNoScoreStates (LexiconFreeDecoder.h:55-66) */
FLTX_DEV uint4 crMergeKey(const CrCand& c, const CrHyp& h) {
  const unsigned long long st = c.isNew ? s2lPair(h.sid, c.edge) : s2lPair(h.psid, h.edge);
  return make_uint4((uint32_t)(st >> 32), (uint32_t)st, (uint32_t)c.token, (uint32_t)c.prevBlank);
}

/* candidatesStore's step 2 over the utterance's candidates cKey[0..n) (0: none; below thrKey: dropped here): a group is the
 * candidates of one merge key cMk; its score is folded into the best member, whose key alone stays.  mTab (mSize >= 2 n
 * slots, a power of two) holds -1.  Called by every thread of the workgroup; returns this thread's count of folded
 * candidates.  (The lexicon seq2seq step's merge, fltx_s2s_lex.h step 4, statement for statement: shared there it moved
 * two SGPR spills of fltx_s2s_lex_step_lm_rows_kernel, and no existing kernel may compile differently.) */
FLTX_DEV int crMergeCandidates(int64_t n, unsigned long long thrKey, int logAdd, unsigned long long* cKey,
                                double* cScore, const uint4* cMk, int32_t* cGrp, int32_t* cList, int32_t* cNext,
                                int32_t* mTab, int mSize) {
  /* the first survivor of a key to claim its slot heads the group, the others join its list */
  const int tid = (int)threadIdx.x;
  const uint32_t mMask = (uint32_t)mSize - 1u;
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    const unsigned long long key = cKey[j];
    if (key != 0ull && key < thrKey) {
      cKey[j] = 0ull;
    } else if (key != 0ull) {
      const uint4 mk = cMk[j];
      uint32_t slot = (uint32_t)s2lMix(((unsigned long long)mk.x << 32 | mk.y) ^ s2lMix((unsigned long long)mk.z << 32 | mk.w)) & mMask;
      for (;;) { /* (mSize >= 2 nC: a free slot always exists) */
        const int32_t old = (int32_t)atomCas32((uint32_t*)&mTab[slot], 0xFFFFFFFFu, (uint32_t)j);
        if (old == -1) {
          cGrp[j] = (int32_t)j;
          cList[j] = -1;
          break;
        }
        if (s2lSameKey(cMk[old], mk)) {
          cGrp[j] = old;
          break;
        }
        slot = (slot + 1u) & mMask;
      }
    }
  }
  __syncthreads();
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    if (cKey[j] != 0ull && cGrp[j] != (int32_t)j) {
      cNext[j] = (int32_t)atomExch32((uint32_t*)&cList[cGrp[j]], (uint32_t)j);
    }
  }
  __threadfence();
  __syncthreads();
  int nMerged = 0;
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    if (cKey[j] == 0ull || cGrp[j] != (int32_t)j || cList[j] < 0) {
      continue;
    }
    /* a group of two or more: the best member, then the fold in descending order from it */
    int64_t best = j;
    for (int32_t m = cList[j]; m >= 0; m = cNext[m]) {
      best = s2lBefore(cScore[m], m, cScore[best], best) ? m : best;
    }
    double acc = cScore[best];
    double lastS = acc;
    int64_t lastJ = best;
    for (;;) { /* the next member in the order after (lastS, lastJ) */
      int64_t nx = -1;
      double ns = 0.0;
      for (int64_t m = j; m >= 0; m = (m == j ? cList[j] : cNext[m])) {
        if (s2lBefore(lastS, lastJ, cScore[m], m) && (nx < 0 || s2lBefore(cScore[m], m, ns, nx))) {
          nx = m;
          ns = cScore[m];
        }
      }
      if (nx < 0) {
        break;
      }
      const double hi = acc > ns ? acc : ns, lo = acc < ns ? acc : ns;
      acc = logAdd ? hi + log1p(exp(lo - hi)) : hi;
      lastS = ns;
      lastJ = nx;
      ++nMerged;
    }
    for (int64_t m = j; m >= 0; m = (m == j ? cList[j] : cNext[m])) {
      cKey[m] = 0ull;
    }
    cScore[best] = acc;
    cKey[best] = s2sScoreKey(acc);
  }
  return nMerged;
}

/* what a row of the next call's list gets besides the publisher's three: next_state */
struct CrRowState {
  int32_t* outState;
  int32_t sid;
  __device__ __forceinline__ void put(int64_t r) const { outState[r] = sid; }
  __device__ __forceinline__ void none(int64_t r) const { outState[r] = -1; }
};

/* an utterance that lists no rows (it stopped) */
FLTX_DEV void crIdleStep(const CrParams& Q, int b) {
  s2sIdleStep(Q.s, b);
  for (int k = (int)threadIdx.x; k < Q.s.K; k += kS2sStepThreads) {
    Q.outState[(int64_t)b * Q.s.K + k] = -1;
  }
}

template <bool FIN, bool STREAM = false>
FLTX_DEV void crStepUtterance(const CrParams& Q, char* smem, const CrsParams* X = nullptr) {
  const S2sParams& P = Q.s;
  S2lStepLds& L = *(S2lStepLds*)smem;
  S2sStepLds& S = L.s;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int K = P.K;
  const int64_t rb = (int64_t)b * K;
  const int tb = Q.T[b];
  int nd;
  const int par = crStepParity<STREAM>(Q, X, b, nd);
  const CrHyp* prev = Q.beam + (size_t)par * P.B * K + rb;
  const int nPrev = P.done[b] ? 0 : P.beamN[par * P.B + b];
  if constexpr (!FIN) {
    if (P.done[b]) {
      crIdleStep(Q, b);
      return;
    }
    if (P.t >= tb) { /* no frames left: the beam as it is -- each slot its own source, no token, the same states */
      for (int k = tid; k < K; k += kS2sStepThreads) {
        const bool in = k < nPrev;
        P.outTok[rb + k] = -1;
        P.outBeam[rb + k] = in ? k : -1;
        P.outSrc[rb + k] = in ? (int32_t)(rb + k) : -1;
        Q.outState[rb + k] = in ? prev[k].sid : -1;
      }
      if (tid == 0) {
        P.outN[b] = nPrev;
      }
      return;
    }
  }
  CrHyp* next = Q.beam + (size_t)(par ^ 1) * P.B * K + rb;
  if (tid == 0) {
    L.full = 0;
  }
  /* 1. the candidates: order keys, scores, merge keys; the best of the step */
  const size_t cb = (size_t)b * P.nC;
  unsigned long long* cKey = P.cKey + cb;
  double* cScore = Q.cScore + cb;
  uint4* cMk = Q.cMk + cb;
  int32_t* mTab = Q.mTab + (size_t)b * Q.mSize;
  const int64_t fr = Q.frameOff[b] + (FIN ? 0 : P.t);
  const int nE = FIN ? 1 : P.recN[fr];
  const int64_t n = FIN ? (int64_t)nPrev : (int64_t)nPrev * P.cap;
  for (int j = tid; j < Q.mSize; j += kS2sStepThreads) {
    mTab[j] = -1;
  }
  unsigned long long mx = 0ull;
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    unsigned long long key = 0ull;
    CrCand c;
    if (crCand<FIN>(Q, prev, fr, nE, rb, j, c)) {
      key = s2sScoreKey(c.score);
      cScore[j] = c.score;
      cMk[j] = crMergeKey(c, prev[c.hyp]);
    }
    cKey[j] = key;
    mx = key > mx ? key : mx;
  }
  /* 2. threshold (candidatesStore step 1), 3. merge (step 2) */
  const unsigned long long thrKey = s2sThresholdKey(s2sBlockMaxKey(S, mx), P.beamThreshold);
  int nMerged = crMergeCandidates(n, thrKey, Q.logAdd, cKey, cScore, cMk, Q.cGrp + cb, Q.cList + cb, Q.cNext + cb, mTab,
                                   Q.mSize);
  __threadfence();
  int surv = 0;
  __syncthreads();
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    surv += cKey[j] != 0ull ? 1 : 0;
  }
  const int nSurv = s2sBlockSum(S.wcnt, surv);
  nMerged = s2sBlockSum(S.wcnt, nMerged);
  /* 4. the K best, sorted best first */
  const int nSel = s2sSelectTopK(S, cKey, n, K, nSurv);
  CrHyp nh = {};
  CrCand c = {};
  if (tid < nSel) {
    const int64_t j = S.selIdx[S.order[tid]];
    crCand<FIN>(Q, prev, fr, nE, rb, j, c);
    const CrHyp& h = prev[c.hyp];
    nh = h;
    nh.parent = c.hyp;
    nh.score = cScore[j];
    nh.token = c.token;
    nh.prevBlank = c.prevBlank;
    if (!FIN) {
      nh.am = h.am + (double)c.am;
    }
    if (c.isNew) {
      nh.lm = h.lm + (double)c.lmS;
      nh.psid = h.sid;
      nh.edge = c.edge;
    }
  }
  if constexpr (FIN) {
    /* 5. the n-best: scores, and the paths walked back through the history (getAllHypothesis, Utils.h:230-266) */
    int fb = P.t < tb ? P.t : tb; /* frames decoded (all of them, unless the caller ends early) */
    int first = 0;
    if constexpr (STREAM) { /* the frames in the buffer, walked by count: its first row has parents of a pruned frame */
      first = X->base[b];
      fb = nd - first;
    }
    const int len = fb + 2;
    if (tid < nSel) {
      double* sc = P.outScores + (rb + tid) * 3;
      sc[0] = nh.score;
      sc[1] = nh.am;
      sc[2] = nh.lm;
      int32_t* out = P.tokens + Q.histOff[b] + (int64_t)tid * len;
      out[len - 1] = Q.sil;
      int p = c.hyp;
      for (int s = fb; s >= 0; --s) {
        const int2 rec = Q.hist[(size_t)(STREAM ? (first + s) % X->ring : s) * P.B * K + rb + p];
        out[s] = rec.x;
        p = rec.y;
      }
    }
    if (tid == 0) {
      Q.merges[b] += nMerged;
      P.outNHyp[b] = nSel;
      P.uttNBeam[b] = nSel;
      P.uttFrame[b] = len - 1;
      P.uttStatus[b] = Q.status[b];
    }
  } else {
    /* 5. survivors that entered a new state look it up (or insert it) in the utterance's state table */
    bool claimed = false;
    uint32_t sslot = 0u;
    unsigned long long* sKey = Q.sKey + (size_t)b * Q.sSize;
    int32_t* sVal = Q.sVal + (size_t)b * Q.sSize;
    const bool hasNew = tid < nSel && c.isNew;
    if (hasNew) {
      const unsigned long long skey = s2lPair(nh.psid, nh.edge);
      const uint32_t sMask = (uint32_t)Q.sSize - 1u;
      uint32_t slot = (uint32_t)s2lMix(skey) & sMask;
      int probes = 0;
      for (; probes < Q.sSize; ++probes) {
        const unsigned long long old = atomCas64(&sKey[slot], ~0ull, skey);
        if (old == ~0ull || old == skey) {
          claimed = old == ~0ull;
          break;
        }
        slot = (slot + 1u) & sMask;
      }
      if (probes == Q.sSize) {
        L.full = 1;
      }
      sslot = slot;
    }
    __syncthreads();
    if (claimed) {
      int32_t v;
      if constexpr (STREAM) { /* (ids come back: fltx_ctc_rows_stream_collect) */
        v = crsClaimId(Q, *X, b, nh.psid, nh.edge);
      } else {
        v = (int32_t)atomAdd32((uint32_t*)&Q.sCount[b], 1u);
      }
      if (v >= Q.sMax) {
        L.full = 1;
      }
      sVal[sslot] = v;
    }
    __threadfence();
    __syncthreads();
    if constexpr (STREAM) {
      crsClaimDone(*X, b);
    }
    if (L.full) { /* the state table is full: the utterance stops, its status says so (never a silent wrong merge) */
      crIdleStep(Q, b);
      if (tid == 0) {
        Q.status[b] |= ST_TABLE_FULL;
        P.nRowsInt[b] = 0;
        P.done[b] = 1;
        P.finalStep[b] = P.t;
      }
      return;
    }
    /* 6. the new beam, its history records and the next call's rows */
    if (tid < nSel) {
      if (hasNew) {
        nh.sid = (int32_t)loadCoherent32((const uint32_t*)&sVal[sslot]);
      }
      next[tid] = nh;
      Q.hist[(size_t)(STREAM ? (nd + 1) % X->ring : P.t + 1) * P.B * K + rb + tid] = make_int2(nh.token, nh.parent);
    }
    if (tid == 0) {
      Q.merges[b] += nMerged;
    }
    const bool in = tid < nSel;
    s2sPublishStepWith(P, S, b, P.t, nSel, in, in && c.isNew ? c.token : -1, in ? nh.parent : -1,
                       in ? (int)rb + nh.parent : -1, CrRowState{Q.outState, nh.sid});
    if constexpr (STREAM) {
      crsStepDone(Q, *X, b, nd, nSel, nh);
    }
  }
}

/* decodeBegin (:20-28): the root (token sil) in LM::start's state (sid 0); the first call's single row */
FLTX_DEV void crBeginOne(const CrParams& Q, int b) {
  const S2sParams& P = Q.s;
  const int64_t rb = (int64_t)b * P.K;
  CrHyp h;
  h.score = 0.0;
  h.am = 0.0;
  h.lm = 0.0;
  h.token = Q.sil;
  h.parent = -1;
  h.sid = 0;
  h.psid = -1;
  h.edge = -1;
  h.prevBlank = 0;
  Q.beam[rb] = h;
  Q.hist[rb] = make_int2(Q.sil, -1);
  Q.sCount[b] = 1;
  Q.status[b] = 0;
  Q.merges[b] = 0;
  P.beamN[b] = 1;
  P.nRowsInt[b] = 1;
  P.done[b] = 0;
  P.finalStep[b] = 0;
  for (int k = 0; k < P.K; ++k) {
    P.outTok[rb + k] = k == 0 ? Q.sil : -1;
    P.outBeam[rb + k] = -1;
    P.outSrc[rb + k] = -1;
    Q.outState[rb + k] = k == 0 ? 0 : -1;
  }
  P.outN[b] = 1;
}

FLTX_DEV void crBeginUtterance(const CrParams& Q, char*) {
  const int b = (int)(blockIdx.x * kS2sBeginThreads + threadIdx.x);
  if (b < Q.s.B) {
    crBeginOne(Q, b);
  }
}

} // namespace fltx
