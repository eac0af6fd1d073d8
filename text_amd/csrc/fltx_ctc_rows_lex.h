/*
 * fltx_ctc_rows_lex.h -- the lexicon CTC beam search (LexiconDecoder.cpp:32-274) with a rows LM, word-level
 * (fltx_lm_word_rows_create) or token-level (fltx_lm_rows_create, isLmToken), as a batched device step per frame.  It is
 * included after fltx_s2s_lex.h and fltx_ctc_rows.h: the compact trie and s2lChild are the lexicon seq2seq step's, the
 * per-frame skeleton -- the token beams of all frames once at begin (fltx_ctc_rows_tokbeam_kernel), crMergeCandidates,
 * the utterance's persistent (parent sid, edge) -> sid table, the next_state publisher, the finish variant that writes
 * fltx_decode_batch's layout -- is the lexicon-free CTC rows step's.
 *
 * A frame step is two kernels:
 *   the gather   token LM: fltx_ctc_rows_lm_kernel as it is, one float per (row, kept token) into recLm[row][e];
 *                word LM:  fltx_ctc_rows_lex_word_lm_kernel, per live row b*K + k (trie node rowNode[row]) and kept token
 *                          e of the utterance's FRAME S = max(1, max labels of the trie) floats recLm[row][e][s]: slot s the
 *                          entry of label s of the token's child, slot 0 unk's entry when the child has no labels and unk
 *                          is on, NaN elsewhere.  Rows are read through lmRowOf; log-probs: a wave per row, logits: a
 *                          workgroup per row (s2sLmRowLse).  Its finish variant reads the finish entry of every row.
 *   the step     fltx_ctc_rows_lex_step_kernel<SRC>, one workgroup of 256 threads per utterance.  The candidates of a
 *                hypothesis are per = cap * (1 + S) + 2 slots, enumerated by index: for entry e of the frame's record slot
 *                0 the move to the token's child (:88-110), slots 1.. a word end per label (:113-142) or the unknown
 *                word (:145-164); then the same node (:167-194) and blank (:196-213), whose emission is read from the
 *                frame's emissions directly -- the reference does not restrict them to the token beam.  Then the
 *                threshold, the merge of candidates equal in (LM state, trie node, token, prevBlank)
 *                (LexiconDecoder.h:79-91), the K best, the state ids, the history record (token, word, parent) and the next
 *                call's rows with next_state and, for the word gather, rowNode.
 * decodeEnd (:231-274) is the step's finish variant: if any hypothesis sits at the root only those finish (a block-wide
 * flag), each in state child(sid, -1) with the finish entry of its row; merge, sort, and the walk through the history into
 * the result layout of the lexicon fltx_decode_batch: T[b] + 2 tokens and words per hypothesis, the word where it ended.
 *
 * LM states.  Word LM: the state changes where a word ends (edge: the word id, unk included); a move inside a word keeps
 * the state and takes the smeared maxScore difference from the trie, no row read.  Token LM: every move and every word end
 * over token n enters child(state, n) with the one LM entry of (row, n); nothing is subtracted.  next_token is that edge,
 * -1 where the state is the parent's.
 */
#pragma once

namespace fltx {

struct CrlHyp { /* one hypothesis of a beam, 56 B */
  double score, am, lm;
  int32_t token;      /* the frame's token (the root: sil) */
  int32_t word;       /* the word that ended in this frame, -1: none */
  int32_t parent;     /* index in the previous beam */
  int32_t node;       /* trie node (0: the root) */
  int32_t sid;        /* canonical LM state */
  int32_t psid, edge; /* the state is child(psid, edge); (-1, -1): LM::start */
  int32_t prevBlank;
};

struct CrlParams {
  CrParams c;       /* the lexicon-free fields (beam / hist unused: the types differ); c.s.nC = K * per; c.recLm: word LM
                     * [B*K][cap][S], token LM [B*K][cap] */
  S2lTrie trie;
  int32_t S;        /* word-end slots per record entry: max(1, max labels) */
  int32_t unk;      /* the unknown word, -1: off (unk_score == -inf) */
  int32_t lmStride; /* floats per row of recLm */
  double wordScore, unkScore;
  CrlHyp* beam;     /* [2][B*K] */
  S2lRec* hist;     /* [maxT + 2][B*K]: (token, word, parent) of the hypotheses after s frames */
  int32_t* rowNode; /* [B*K]: the trie node of each listed row's hypothesis (the word gather reads it) */
  int32_t* words;   /* end: the result's words, laid out as the tokens */
};

enum { kCrlLmWordRows = 0, kCrlLmTokenRows = 1 };

/* ---- the word-rows gather ---------------------------------------------------------------------------------------------- */
struct CrlWordLmParams {
  CrLmParams w;           /* w.r.usrToLm: word id -> LM index (null: identity); w.r.recLm: [B*K][cap][S] */
  S2lTrie trie;
  const int32_t* rowNode; /* [B*K] */
  int32_t S;
  int32_t unk;            /* -1: off */
};

template <int DT, bool LOGITS>
FLTX_DEV void crlWordLmGather(const CrlWordLmParams& W, int64_t r, const void* row, double lse, int tid, int nThreads) {
  const S2sLmRowsParams& Q = W.w.r;
  const S2sParams& P = Q.s;
  const int S = W.S;
  const float nan = __uint_as_float(0x7FC00000u);
  if (W.w.fin) { /* decodeEnd: the finish entry alone */
    if (tid == 0) {
      float v = nan;
      if (row != nullptr && Q.finishIdx >= 0 && Q.finishIdx < Q.width) {
        v = s2sTypedScore<DT, LOGITS>(row, Q.finishIdx, lse);
      }
      Q.recLm[r * P.cap * S] = v;
    }
    return;
  }
  const int b = (int)(r / P.K);
  const int64_t fr = W.w.frameOff[b] + P.t;
  const int n = P.recN[fr];
  const int node = W.rowNode[r];
  for (int e = tid; e < n; e += nThreads) { /* (one trie look-up per kept token, then its S slots) */
    const int tok = P.recTok[fr * P.cap + e];
    const int child = s2lChild(W.trie, node, tok);
    int l0 = 0, nl = 0;
    if (child >= 0) {
      l0 = W.trie.labOff[child];
      nl = W.trie.labOff[child + 1] - l0;
    }
    float* out = Q.recLm + (r * P.cap + e) * S;
    for (int s = 0; s < S; ++s) {
      int word = -1;
      if (s < nl) {
        word = W.trie.labels[l0 + s];
      } else if (child >= 0 && nl == 0 && s == 0) {
        word = W.unk;
      }
      float v = nan;
      if (row != nullptr && word >= 0) {
        const int idx = Q.usrToLm ? Q.usrToLm[word] : word;
        if (idx >= 0 && idx < Q.width) {
          v = s2sTypedScore<DT, LOGITS>(row, idx, lse);
        }
      }
      out[s] = v;
    }
  }
}

template <int DT, bool LOGITS>
FLTX_DEV void crlWordLmRows(const CrlWordLmParams& W, char* smem) {
  const S2sLmRowsParams& Q = W.w.r;
  const S2sParams& P = Q.s;
  if constexpr (!LOGITS) { /* workgroup = four waves, wave = row b*K + k */
    const int wave = waveUniform(waveId());
    const int64_t r = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
    if (r >= (int64_t)P.B * P.K || !crRowLive(W.w, r)) {
      return;
    }
    crlWordLmGather<DT, false>(W, r, crLmRow<DT>(W.w, r), 0.0, laneId(), 64);
  } else { /* workgroup = row b*K + k */
    const int64_t r = (int64_t)blockIdx.x;
    const bool live = crRowLive(W.w, r);
    const void* row = live ? crLmRow<DT>(W.w, r) : nullptr;
    if (row == nullptr) {
      if (threadIdx.x == 0 && Q.rowLse) {
        Q.rowLse[r] = __longlong_as_double(0x7FF8000000000000ll);
      }
      if (live) {
        crlWordLmGather<DT, true>(W, r, nullptr, 0.0, (int)threadIdx.x, kS2sLmThreads);
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
    crlWordLmGather<DT, true>(W, r, row, lse, (int)threadIdx.x, kS2sLmThreads);
  }
}

/* ---- the step ------------------------------------------------------------------------------------------------------- */
struct CrlCand {
  double score;
  float am, lmS;
  int32_t hyp; /* index in the previous beam */
  int32_t token, word, node, prevBlank;
  int32_t edge;
  bool isNew;  /* the state is child(prev.sid, edge) */
  bool hasLm;  /* lmS is added to the hypothesis' LM score (a child of the node; decodeEnd) */
};

struct CrlStepLds {
  S2lStepLds l;
  int32_t nice; /* decodeEnd: a hypothesis sits at the root */
};

/* candidate j of the utterance (LexiconDecoder.cpp:55-213, the same double operations in the same order): hypothesis
 * k = j / per, slot q = j % per -- q < cap * (1 + S): entry e = q / (1 + S) of the frame's record, sub-slot 0 the move,
 * 1.. the word ends; then the same node and blank.  FIN: hypothesis j, decodeEnd's (:241-262).  false: none */
template <int SRC, bool FIN, int EM = kCrEmPlain, bool LOGITS = false>
FLTX_DEV bool crlCand(const CrlParams& R, const CrlHyp* prev, const void* em, double lse, int64_t fr, int nE, int64_t rb,
                      int nice, int64_t j, CrlCand& c) {
  const CrParams& Q = R.c;
  const S2sParams& P = Q.s;
  const int cap = P.cap;
  if constexpr (FIN) {
    const CrlHyp& h = prev[j];
    if (nice && h.node != 0) {
      return false;
    }
    c.hyp = (int)j;
    c.am = 0.0f;
    c.lmS = Q.recLm[(rb + j) * R.lmStride];
    c.score = h.score + P.lmWeight * (double)c.lmS;
    c.token = Q.sil;
    c.word = -1;
    c.node = h.node;
    c.prevBlank = 0;
    c.isNew = true;
    c.hasLm = true;
    c.edge = -1;
    return true;
  } else {
    const int S1 = 1 + R.S, per = cap * S1 + 2;
    const int k = (int)(j / per), q = (int)(j % per);
    const CrlHyp& h = prev[k];
    c.hyp = k;
    c.word = -1;
    c.edge = -1;
    c.isNew = false;
    if (q >= cap * S1) { /* (2) the same node, (3) blank: the frame's emission itself; state, node and lm stay */
      int n = Q.blank;
      if (q == cap * S1) {
        if (h.prevBlank && h.node != 0) {
          return false;
        }
        n = h.node == 0 ? Q.sil : h.token;
      }
      const float a = crEmission<EM, LOGITS>(em, n, lse);
      double score = h.score + (double)a;
      if (q == cap * S1 && n == Q.sil) {
        score += Q.silScore;
      }
      c.score = score;
      c.am = a;
      c.lmS = 0.0f;
      c.hasLm = false;
      c.token = n;
      c.node = h.node;
      c.prevBlank = q == cap * S1 ? 0 : 1;
      return true;
    }
    const int e = q / S1, s = q % S1;
    if (e >= nE) {
      return false;
    }
    const int tok = P.recTok[fr * cap + e];
    const int child = s2lChild(R.trie, h.node, tok); /* (1) a child of the hypothesis' node */
    if (child < 0) {
      return false;
    }
    const float a = P.recAm[fr * cap + e];
    double score = h.score + (double)a;
    if (tok == Q.sil) {
      score += Q.silScore;
    }
    c.am = a;
    c.token = tok;
    c.prevBlank = 0;
    c.hasLm = true;
    float lexMax = 0.0f; /* (a token LM subtracts nothing: the trie's scores are not read) */
    if constexpr (SRC == kCrlLmWordRows) {
      lexMax = h.node == 0 ? 0.0f : R.trie.maxScore[h.node];
    }
    if (s == 0) { /* a new token that stays inside a word (:88-110) */
      if (!(h.prevBlank || tok != h.token) || R.trie.kidOff[child + 1] == R.trie.kidOff[child]) {
        return false;
      }
      if constexpr (SRC == kCrlLmWordRows) {
        c.lmS = R.trie.maxScore[child] - lexMax; /* smearing (float) */
      } else {
        c.lmS = Q.recLm[(rb + k) * R.lmStride + e];
        c.isNew = true;
        c.edge = tok;
      }
      c.score = score + P.lmWeight * (double)c.lmS;
      c.node = child;
      return true;
    }
    const int l0 = R.trie.labOff[child], nl = R.trie.labOff[child + 1] - l0;
    double add;
    if (nl > 0) { /* a word per label (:113-142); not the one-token word repeated at the root */
      if (s - 1 >= nl || (h.node == 0 && h.token == tok)) {
        return false;
      }
      c.word = R.trie.labels[l0 + s - 1];
      add = R.wordScore;
    } else { /* the unknown word (:145-164) */
      if (s != 1 || R.unk < 0) {
        return false;
      }
      c.word = R.unk;
      add = R.unkScore;
    }
    if constexpr (SRC == kCrlLmWordRows) {
      c.lmS = Q.recLm[(rb + k) * R.lmStride + e * R.S + (s - 1)] - lexMax;
      c.edge = c.word;
    } else {
      c.lmS = Q.recLm[(rb + k) * R.lmStride + e];
      c.edge = tok;
    }
    c.isNew = true;
    c.score = (score + P.lmWeight * (double)c.lmS) + add;
    c.node = 0;
    return true;
  }
}

/* the merge key: (the state's (parent sid, edge), trie node, token and prevBlank) -- LexiconDecoder.h:79-91 */
FLTX_DEV uint4 crlMergeKey(const CrlCand& c, const CrlHyp& h) {
  const unsigned long long st = c.isNew ? s2lPair(h.sid, c.edge) : s2lPair(h.psid, h.edge);
  return make_uint4((uint32_t)(st >> 32), (uint32_t)st, (uint32_t)c.node, ((uint32_t)c.token << 1) | (uint32_t)c.prevBlank);
}

/* what a row of the next call's list gets besides the publisher's three: next_state, and the row's trie node */
struct CrlRowState {
  int32_t *outState, *rowNode;
  int32_t sid, node;
  __device__ __forceinline__ void put(int64_t r) const {
    outState[r] = sid;
    rowNode[r] = node;
  }
  __device__ __forceinline__ void none(int64_t r) const { outState[r] = -1; }
};

/* EM / LOGITS: what the frame's emissions are read as (kCrEmPlain: the float32 log-probs of fltx_ctc_rows_begin; a
 * dtype: the typed frames E names, fltx_ctc_rows_typed.h) -- compile-time, so that the plain step stays the code it was */
template <int SRC, bool FIN, bool STREAM = false, int EM = kCrEmPlain, bool LOGITS = false>
FLTX_DEV void crlStepUtterance(const CrlParams& R, char* smem, const CrsParams* Z = nullptr,
                               const CrTypedEm* E = nullptr) {
  static_assert(!FIN || EM == kCrEmPlain, "decodeEnd reads no emissions");
  const CrParams& Q = R.c;
  const S2sParams& P = Q.s;
  CrlStepLds& X = *(CrlStepLds*)smem;
  S2lStepLds& L = X.l;
  S2sStepLds& S = L.s;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int K = P.K;
  const int64_t rb = (int64_t)b * K;
  const int tb = Q.T[b];
  int nd;
  const int par = crStepParity<STREAM>(Q, Z, b, nd);
  const CrlHyp* prev = R.beam + (size_t)par * P.B * K + rb;
  const int nPrev = P.done[b] ? 0 : P.beamN[par * P.B + b];
  if constexpr (!FIN) {
    if (P.done[b]) {
      crIdleStep(Q, b);
      return;
    }
    if (P.t >= tb) { /* no frames left: the beam as it is -- each slot its own source, no edge, the same states */
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
  CrlHyp* next = R.beam + (size_t)(par ^ 1) * P.B * K + rb;
  if (tid == 0) {
    L.full = 0;
    X.nice = 0;
  }
  int nice = 0;
  if constexpr (FIN) { /* hasNiceEnding (:233-240) */
    __syncthreads();
    if (tid < nPrev && prev[tid].node == 0) {
      X.nice = 1;
    }
    __syncthreads();
    nice = X.nice;
  }
  /* 1. the candidates: order keys, scores, merge keys; the best of the step */
  const size_t cb = (size_t)b * P.nC;
  unsigned long long* cKey = P.cKey + cb;
  double* cScore = Q.cScore + cb;
  uint4* cMk = Q.cMk + cb;
  int32_t* mTab = Q.mTab + (size_t)b * Q.mSize;
  const int64_t fr = Q.frameOff[b] + (FIN ? 0 : P.t);
  const int nE = FIN ? 1 : P.recN[fr];
  const void* em;
  double lse = 0.0;
  if constexpr (EM == kCrEmPlain) {
    em = Q.emissions + Q.emOff[b] + (FIN ? (int64_t)0 : (int64_t)P.t * P.V);
  } else {
    em = (const char*)E->x + (Q.emOff[b] + (int64_t)P.t * E->stride) * (EM == kS2sDtF32 ? 4 : 2);
    if constexpr (LOGITS) {
      lse = E->lse[fr];
    }
  }
  const int64_t n = FIN ? (int64_t)nPrev : (int64_t)nPrev * (P.cap * (1 + R.S) + 2);
  for (int j = tid; j < Q.mSize; j += kS2sStepThreads) {
    mTab[j] = -1;
  }
  unsigned long long mx = 0ull;
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    unsigned long long key = 0ull;
    CrlCand c;
    if (crlCand<SRC, FIN, EM, LOGITS>(R, prev, em, lse, fr, nE, rb, nice, j, c)) {
      key = s2sScoreKey(c.score);
      cScore[j] = c.score;
      cMk[j] = crlMergeKey(c, prev[c.hyp]);
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
  CrlHyp nh = {};
  CrlCand c = {};
  if (tid < nSel) {
    const int64_t j = S.selIdx[S.order[tid]];
    crlCand<SRC, FIN, EM, LOGITS>(R, prev, em, lse, fr, nE, rb, nice, j, c);
    const CrlHyp& h = prev[c.hyp];
    nh = h;
    nh.parent = c.hyp;
    nh.score = cScore[j];
    nh.token = c.token;
    nh.word = c.word;
    nh.node = c.node;
    nh.prevBlank = c.prevBlank;
    if (!FIN) {
      nh.am = h.am + (double)c.am;
    }
    if (c.hasLm) {
      nh.lm = h.lm + (double)c.lmS;
    }
    if (c.isNew) {
      nh.psid = h.sid;
      nh.edge = c.edge;
    }
  }
  if constexpr (FIN) {
    /* 5. the n-best: scores, and the paths walked back through the history (getAllHypothesis, Utils.h:230-266) */
    int fb = P.t < tb ? P.t : tb; /* frames decoded (all of them, unless the caller ends early) */
    int first = 0;
    if constexpr (STREAM) { /* the frames in the buffer, walked by count */
      first = Z->base[b];
      fb = nd - first;
    }
    const int len = fb + 2;
    if (tid < nSel) {
      double* sc = P.outScores + (rb + tid) * 3;
      sc[0] = nh.score;
      sc[1] = nh.am;
      sc[2] = nh.lm;
      const int64_t at = Q.histOff[b] + (int64_t)tid * len;
      int32_t* out = P.tokens + at;
      int32_t* outW = R.words + at;
      out[len - 1] = Q.sil;
      outW[len - 1] = -1;
      int p = c.hyp;
      for (int s = fb; s >= 0; --s) {
        const S2lRec rec = R.hist[(size_t)(STREAM ? (first + s) % Z->ring : s) * P.B * K + rb + p];
        out[s] = rec.token;
        outW[s] = rec.word;
        p = rec.parent;
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
        v = crsClaimId(Q, *Z, b, nh.psid, nh.edge);
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
      crsClaimDone(*Z, b);
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
      S2lRec rec;
      rec.token = nh.token;
      rec.word = nh.word;
      rec.parent = nh.parent;
      rec.pad = 0;
      R.hist[(size_t)(STREAM ? (nd + 1) % Z->ring : P.t + 1) * P.B * K + rb + tid] = rec;
    }
    if (tid == 0) {
      Q.merges[b] += nMerged;
    }
    const bool in = tid < nSel;
    s2sPublishStepWith(P, S, b, P.t, nSel, in, in && c.isNew ? c.edge : -1, in ? nh.parent : -1,
                       in ? (int)rb + nh.parent : -1, CrlRowState{Q.outState, R.rowNode, nh.sid, nh.node});
    if constexpr (STREAM) {
      crsStepDone(Q, *Z, b, nd, nSel, nh);
    }
  }
}

/* the frame step on typed emissions (fltx_ctc_rows_begin_typed): the same step, its two direct emission reads typed */
struct CrlTypedParams {
  CrlParams r; /* (r.c.emissions is not read; r.c.emOff counts elements of e.x) */
  CrTypedEm e;
};

template <int SRC, int DT, bool LOGITS>
FLTX_DEV void crlStepTyped(const CrlTypedParams& Y, char* smem) {
  crlStepUtterance<SRC, false, false, DT, LOGITS>(Y.r, smem, nullptr, &Y.e);
}

/* decodeBegin (:21-30): the root (token sil) at the trie's root in LM::start's state (sid 0); the first call's single
 * row, made by no edge */
FLTX_DEV void crlBeginOne(const CrlParams& R, int b) {
  const CrParams& Q = R.c;
  const S2sParams& P = Q.s;
  const int64_t rb = (int64_t)b * P.K;
  CrlHyp h;
  h.score = 0.0;
  h.am = 0.0;
  h.lm = 0.0;
  h.token = Q.sil;
  h.word = -1;
  h.parent = -1;
  h.node = 0;
  h.sid = 0;
  h.psid = -1;
  h.edge = -1;
  h.prevBlank = 0;
  R.beam[rb] = h;
  S2lRec rec;
  rec.token = Q.sil;
  rec.word = -1;
  rec.parent = -1;
  rec.pad = 0;
  R.hist[rb] = rec;
  R.rowNode[rb] = 0;
  Q.sCount[b] = 1;
  Q.status[b] = 0;
  Q.merges[b] = 0;
  P.beamN[b] = 1;
  P.nRowsInt[b] = 1;
  P.done[b] = 0;
  P.finalStep[b] = 0;
  for (int k = 0; k < P.K; ++k) {
    P.outTok[rb + k] = -1;
    P.outBeam[rb + k] = -1;
    P.outSrc[rb + k] = -1;
    Q.outState[rb + k] = k == 0 ? 0 : -1;
  }
  P.outN[b] = 1;
}

FLTX_DEV void crlBeginUtterance(const CrlParams& R, char*) {
  const int b = (int)(blockIdx.x * kS2sBeginThreads + threadIdx.x);
  if (b < R.c.s.B) {
    crlBeginOne(R, b);
  }
}

} // namespace fltx
