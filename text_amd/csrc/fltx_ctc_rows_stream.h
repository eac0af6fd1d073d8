/*
 * fltx_ctc_rows_stream.h -- streams on the two CTC rows decoders (fltx_ctc_rows.h, fltx_ctc_rows_lex.h): decodeStep on
 * chunks as they arrive, getBestHypothesis(lookBack) and prune(lookBack) (LexiconFreeDecoder.cpp:188-227,
 * LexiconDecoder.cpp:285-325, Utils.h:268-342).  Included after fltx_ctc_rows_lex.h.
 *
 * Counts.  A chunk is what the offline path calls a batch: s.t, T, frameOff and emOff of CrParams are the chunk's, so the
 * token beams (crTokBeamRows) and the two gathers (crLmRows, crlWordLmRows) run unchanged.  What outlives a chunk is per
 * stream and on the device (CrsParams): nDec, the frames decoded since begin, and base, the frames pruned off.  The
 * buffer holds frames base .. nDec: nDecodedFramesInBuffer is nDec - base + 1.  The beam after nDec frames is the one
 * of parity nDec & 1; beamN carries its size in both slots.
 *
 * Rings.  The history row of frame s is s % ring, ring = max_frames (+ kLookBackLimit for the lexicon kind) + 2 rows of
 * [B*K] records; a second ring of the same shape holds (score, am, lm), which getBestHypothesis(lookBack > 0) returns of
 * the ancestor.  Walks stop by count: the first row of the buffer still names parents, of a frame that is gone.  So
 * prune moves base, subtracts the current beam's largest score from the current beam's scores (beam and score ring;
 * am and lm stay, and so do the scores of older frames: Utils.h:331-341) and copies nothing.
 *
 * Kernels: the begin, step and end variants of the two kinds (the offline bodies with STREAM set), and
 *   fltx_ctc_rows_stream_best_kernel<LEX>   one workgroup per stream: the first best of the beam by strict > is slot 0
 *   fltx_ctc_rows_stream_prune_kernel<LEX>  (the beams are sorted best first); thread 0 alone walks lookBack
 *                                           records up -- a chain of dependent loads, nothing to spread -- and, for
 *                                           the lexicon kind, on to a complete hypothesis (its parent ended a word, or
 *                                           it has none), lookBack + kLookBackLimit steps at most.  best writes the
 *                                           ancestor's scores and its path; prune the new base and the normalised scores.
 *   fltx_ctc_rows_stream_collect_kernel<LEX> the LM-state ids nothing can meet again, back to the stream's free stack
 *   fltx_ctc_rows_stream_finish_kernel,     fltx_ctc_rows_stream_finish: one workgroup per stream.  A stream the call
 *   fltx_ctc_rows_lex_stream_finish_kernel  does not name lists its beam again and returns.  A named one runs the end
 *                                           variant's body against the finish's own result buffers and then, behind a
 *                                           barrier, the begin for this b: the root in the beam and both rings, the
 *                                           counts and the ids started over, and its slice of the state table emptied --
 *                                           the one part whose cost grows with max_states (1 MB of keys at the default).
 */
#pragma once

namespace fltx {

constexpr int kCrsOpThreads = 256;  /* >= kS2sMaxBeam: prune normalises with a thread per hypothesis */

struct CrStreamParams {
  CrParams c;
  CrsParams x;
};

struct CrlStreamParams {
  CrlParams r;
  CrsParams x;
};

/* ---- begin, step, end: the offline bodies on a stream's counts -------------------------------------------------------- */
FLTX_DEV void crsBeginCountsOne(const CrParams& Q, const CrsParams& X, int b) {
  const S2sParams& P = Q.s;
  X.nDec[b] = 0;
  X.base[b] = 0;
  X.sFreeN[b] = 0; /* no id is free; id 0, LM::start, is allocated and has no table entry */
  X.sPar[(size_t)b * Q.sMax] = -1;
  X.sEdge[(size_t)b * Q.sMax] = -1;
  P.beamN[P.B + b] = 1;
  double* sc = X.sHist + (size_t)b * P.K * 3; /* the root's scores */
  sc[0] = 0.0;
  sc[1] = 0.0;
  sc[2] = 0.0;
}

FLTX_DEV void crsBeginCounts(const CrParams& Q, const CrsParams& X) {
  const int b = (int)(blockIdx.x * kS2sBeginThreads + threadIdx.x);
  if (b < Q.s.B) {
    crsBeginCountsOne(Q, X, b);
  }
}

FLTX_DEV void crsBeginStream(const CrStreamParams& Z, char* smem) {
  crBeginUtterance(Z.c, smem);
  crsBeginCounts(Z.c, Z.x);
}

FLTX_DEV void crlsBeginStream(const CrlStreamParams& Z, char* smem) {
  crlBeginUtterance(Z.r, smem);
  crsBeginCounts(Z.r.c, Z.x);
}

template <bool FIN>
FLTX_DEV void crsStepStream(const CrStreamParams& Z, char* smem) {
  crStepUtterance<FIN, true>(Z.c, smem, &Z.x);
}

template <int SRC, bool FIN>
FLTX_DEV void crlsStepStream(const CrlStreamParams& Z, char* smem) {
  crlStepUtterance<SRC, FIN, true>(Z.r, smem, &Z.x);
}

struct CrlTypedStreamParams { /* a chunk of typed emissions (fltx_ctc_rows_stream_append_typed) */
  CrlParams r;
  CrsParams x;
  CrTypedEm e;
};

template <int SRC, int DT, bool LOGITS>
FLTX_DEV void crlsStepStreamTyped(const CrlTypedStreamParams& Y, char* smem) {
  crlStepUtterance<SRC, false, true, DT, LOGITS>(Y.r, smem, &Y.x, &Y.e);
}

/* ---- getBestHypothesis and prune ------------------------------------------------------------------------------------------ */
struct CrsOpParams {
  int32_t B, K, lookBack, maxLen;
  const int32_t* beamN; /* [2][B], both slots the stream's */
  const int32_t* status; /* [B] ST_* */
  CrsParams x;
  void* beam;           /* [2][B*K] CrHyp / CrlHyp */
  const void* hist;     /* [ring][B*K] int2 / S2lRec */
  /* best */
  int32_t* bestLen;     /* [2][B]: the length (0: an empty result), the stream's status */
  double* bestScores;   /* [B][3] */
  int32_t *bestTok, *bestWrd; /* [B][maxLen] */
};

struct CrsOpLds {
  int32_t anc, steps; /* the ancestor's slot in its beam (-1: none) and how far back it is */
  double largest;
};

template <bool LEX>
struct CrsKind {
  using Hyp = CrHyp;
  using Rec = int2;
  static __device__ __forceinline__ int token(const Rec& r) { return r.x; }
  static __device__ __forceinline__ int word(const Rec&) { return -1; }
  static __device__ __forceinline__ int parent(const Rec& r) { return r.y; }
};
template <>
struct CrsKind<true> {
  using Hyp = CrlHyp;
  using Rec = S2lRec;
  static __device__ __forceinline__ int token(const Rec& r) { return r.token; }
  static __device__ __forceinline__ int word(const Rec& r) { return r.word; }
  static __device__ __forceinline__ int parent(const Rec& r) { return r.parent; }
};

/* findBestAncestor (Utils.h:268-310) on stream b, whose buffer holds F + 1 frames.  Every thread gets the same answer:
 * S.anc the ancestor's slot in the beam of buffer frame F - S.steps (-1: the walk left the buffer, or the beam is empty),
 * S.steps the updated lookBack, S.largest the beam's largest score. */
template <bool LEX>
FLTX_DEV void crsFindBestAncestor(const CrsOpParams& W, CrsOpLds& S, int b, int nd, int first, int n) {
  using Kd = CrsKind<LEX>;
  const int tid = (int)threadIdx.x;
  const int64_t BK = (int64_t)W.B * W.K, rb = (int64_t)b * W.K;
  const typename Kd::Hyp* beam = (const typename Kd::Hyp*)W.beam + (size_t)(nd & 1) * BK + rb;
  const typename Kd::Rec* hist = (const typename Kd::Rec*)W.hist;
  if (tid == 0) {
    const int F = nd - first;
    /* The first best by strict > (the largest score, the lower slot among equals) is slot 0: the step leaves every beam
     * sorted best first (s2sSelectTopK), and a prune takes one value off all of its scores.  No reduction over the beam. */
    int p = n > 0 ? 0 : -1;
    int f = F, steps = 0;
    S.largest = n > 0 ? beam[0].score : 0.0;
    while (p >= 0 && steps < W.lookBack) { /* (the parent of the buffer's first frame is null) */
      ++steps;
      p = f > 0 ? Kd::parent(hist[(size_t)((first + f) % W.x.ring) * BK + rb + p]) : -1;
      --f;
    }
    if constexpr (LEX) { /* (one record per step: the parent's record says whether it ended a word, and names its own parent) */
      const int maxLookBack = W.lookBack + kLookBackLimit;
      typename Kd::Rec rec = {};
      if (p >= 0 && f > 0) {
        rec = hist[(size_t)((first + f) % W.x.ring) * BK + rb + p];
      }
      while (p >= 0 && f > 0) { /* isComplete (LexiconDecoder.h:97-99): no parent (f == 0) ... */
        const int pp = Kd::parent(rec);
        rec = hist[(size_t)((first + f - 1) % W.x.ring) * BK + rb + pp];
        if (Kd::word(rec) >= 0) { /* ... or the parent ended a word */
          break;
        }
        ++steps;
        p = pp;
        --f;
        if (steps == maxLookBack) {
          break;
        }
      }
    }
    S.anc = p;
    S.steps = steps;
  }
  __syncthreads();
}

/* getBestHypothesis(lookBack) of every stream: workgroup = stream */
template <bool LEX>
FLTX_DEV void crsBest(const CrsOpParams& W, char* smem) {
  using Kd = CrsKind<LEX>;
  CrsOpLds& S = *(CrsOpLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int64_t BK = (int64_t)W.B * W.K, rb = (int64_t)b * W.K;
  const int nd = W.x.nDec[b], first = W.x.base[b];
  const int F = nd - first;
  const int n = W.beamN[b];
  if (tid == 0) {
    W.bestLen[W.B + b] = W.status[b];
  }
  if (LEX && F - W.lookBack < 1) { /* LexiconDecoder.cpp:286 */
    if (tid == 0) {
      W.bestLen[b] = 0;
    }
    return;
  }
  crsFindBestAncestor<LEX>(W, S, b, nd, first, n);
  if (tid != 0) {
    return;
  }
  int p = S.anc;
  if (p < 0) {
    W.bestLen[b] = 0;
    return;
  }
  const int f0 = F - S.steps; /* the ancestor's frame in the buffer: getHypothesis(node, f0) (Utils.h:229-250) */
  const typename Kd::Rec* hist = (const typename Kd::Rec*)W.hist;
  const double* sc = W.x.sHist + ((size_t)((first + f0) % W.x.ring) * BK + rb + p) * 3;
  W.bestScores[3 * b] = sc[0];
  W.bestScores[3 * b + 1] = sc[1];
  W.bestScores[3 * b + 2] = sc[2];
  W.bestLen[b] = f0 + 1;
  int32_t* tok = W.bestTok + (size_t)b * W.maxLen;
  int32_t* wrd = W.bestWrd + (size_t)b * W.maxLen;
  for (int f = f0; f >= 0; --f) {
    const typename Kd::Rec rec = hist[(size_t)((first + f) % W.x.ring) * BK + rb + p];
    tok[f] = Kd::token(rec);
    wrd[f] = Kd::word(rec);
    p = Kd::parent(rec);
  }
}

/* prune(lookBack) of every stream: workgroup = stream */
template <bool LEX>
FLTX_DEV void crsPrune(const CrsOpParams& W, char* smem) {
  using Kd = CrsKind<LEX>;
  CrsOpLds& S = *(CrsOpLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int64_t BK = (int64_t)W.B * W.K, rb = (int64_t)b * W.K;
  const int nd = W.x.nDec[b], first = W.x.base[b];
  const int F = nd - first;
  const int n = W.beamN[b];
  if (F - W.lookBack < 1) {
    return; /* not enough decoded frames */
  }
  crsFindBestAncestor<LEX>(W, S, b, nd, first, n);
  const int startFrame = F - S.steps;
  if (S.anc < 0 || startFrame < 1) {
    return;
  }
  /* pruneAndNormalize (Utils.h:312-342): the buffer begins at startFrame; the current beam's scores, less their largest */
  if (tid < n) {
    typename Kd::Hyp* beam = (typename Kd::Hyp*)W.beam + (size_t)(nd & 1) * BK + rb;
    double s = beam[tid].score;
    s -= S.largest;
    beam[tid].score = s;
    W.x.sHist[((size_t)(nd % W.x.ring) * BK + rb + tid) * 3] = s;
  }
  if (tid == 0) {
    W.x.base[b] = first + startFrame;
  }
}

/* ---- collect: the LM-state ids nothing can meet again go back to the stream ------------------------------------------- */
constexpr int kCrsLdsIds = 65536; /* ids whose two mark bitsets fit the kernel's LDS (2 x 8 KB); more: the HBM scratch */

struct CrsCollectParams {
  int32_t B, K, sMax, sSize, releaseCap;
  const int32_t* beamN;  /* [2][B], both slots the stream's */
  const int32_t* done;   /* [B] the stream has stopped */
  CrsParams x;
  const void* beam;      /* [2][B*K] CrHyp / CrlHyp */
  unsigned long long* sKey;
  int32_t* sVal;
  const int32_t* sCount;
  uint32_t* marks;       /* [B][2][(sMax + 31) / 32] when sMax > kCrsLdsIds, else null */
  int32_t *released, *nReleased, *nLive;
};

struct CrsCollectLds {
  uint32_t bits[2][kCrsLdsIds / 32];
  int32_t wsum[kCrsOpThreads / 64];
  int32_t changed;
};

FLTX_DEV bool crsMarked(const uint32_t* bits, int id) {
  return (loadCoherent32(&bits[id >> 5]) >> (id & 31)) & 1u;
}
FLTX_DEV void crsMark(uint32_t* bits, int id) { (void)atomOr32(&bits[id >> 5], 1u << (id & 31)); }

/* One workgroup per stream.  With R the ids a later step can still look up or enter -- the sids of the current beam and,
 * transitively, every id whose table entry hangs below one of R -- and the psids of the current beam, which merge keys
 * still compare as numbers, every other allocated id is dead: the lowest releaseCap of them go on the free stack and
 * into released[] (ascending, -1 behind them), the table entries whose id or parent went are dropped, and a pinned id
 * that loses its entry keeps its number. */
template <bool LEX>
FLTX_DEV void crsCollect(const CrsCollectParams& W, char* smem) {
  using Hyp = typename CrsKind<LEX>::Hyp;
  CrsCollectLds& S = *(CrsCollectLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const size_t sb = (size_t)b * W.sMax;
  int32_t* sPar = W.x.sPar + sb;
  int32_t* sEdge = W.x.sEdge + sb;
  int32_t* out = W.released + (size_t)b * W.releaseCap;
  for (int i = tid; i < W.releaseCap; i += kCrsOpThreads) {
    out[i] = -1;
  }
  const int cnt = W.sCount[b];
  const int hw = cnt < W.sMax ? cnt : W.sMax; /* ids below the high-water mark */
  const int nFree = W.x.sFreeN[b];
  if (W.done[b]) { /* a stopped stream is left alone */
    if (tid == 0) {
      W.nReleased[b] = 0;
      if (W.nLive) {
        W.nLive[b] = hw - nFree;
      }
    }
    return;
  }
  const int words = (W.sMax + 31) >> 5;
  uint32_t* inR = W.marks ? W.marks + (size_t)b * 2 * words : S.bits[0];
  uint32_t* pin = W.marks ? inR + words : S.bits[1];
  /* 1. mark: the beam's states and their parents' numbers, then R down the table tree until a pass adds nothing */
  for (int i = tid; i < ((hw + 31) >> 5); i += kCrsOpThreads) {
    inR[i] = 0u;
    pin[i] = 0u;
  }
  __threadfence();
  __syncthreads();
  const int nd = W.x.nDec[b];
  const int n = W.beamN[b];
  const Hyp* beam = (const Hyp*)W.beam + (size_t)(nd & 1) * W.B * W.K + (size_t)b * W.K;
  for (int k = tid; k < n; k += kCrsOpThreads) {
    const int sid = beam[k].sid, psid = beam[k].psid;
    if (sid >= 0 && sid < hw) {
      crsMark(inR, sid);
    }
    if (psid >= 0 && psid < hw) {
      crsMark(pin, psid);
    }
  }
  for (;;) {
    __threadfence();
    __syncthreads();
    if (tid == 0) {
      S.changed = 0;
    }
    __syncthreads();
    bool any = false;
    for (int id = tid; id < hw; id += kCrsOpThreads) {
      const int p = sPar[id];
      if (p >= 0 && !crsMarked(inR, id) && crsMarked(inR, p)) {
        crsMark(inR, id);
        any = true;
      }
    }
    if (any) {
      S.changed = 1;
    }
    __threadfence();
    __syncthreads();
    if (!S.changed) {
      break;
    }
  }
  /* 2. select: the dead ids in ascending order -- thread tid owns ids [tid * per, (tid + 1) * per) */
  const int per = (hw + kCrsOpThreads - 1) / kCrsOpThreads;
  const int lo = tid * per < hw ? tid * per : hw, hi = lo + per < hw ? lo + per : hw;
  int mine = 0;
  for (int id = lo; id < hi; ++id) {
    mine += sPar[id] != -2 && !crsMarked(inR, id) && !crsMarked(pin, id) ? 1 : 0;
  }
  const int incl = waveInclusiveScan(mine);
  if (laneId() == 63) {
    S.wsum[waveId()] = incl;
  }
  __syncthreads();
  int rank = incl - mine, dead = 0;
  for (int w = 0; w < kCrsOpThreads / 64; ++w) {
    rank += w < waveId() ? S.wsum[w] : 0;
    dead += S.wsum[w];
  }
  const int nRel = dead < W.releaseCap ? dead : W.releaseCap;
  /* 3. free: on the stack and into the caller's list */
  int32_t* stack = W.x.sFree + sb + nFree;
  for (int id = lo; id < hi && rank < nRel; ++id) {
    if (sPar[id] != -2 && !crsMarked(inR, id) && !crsMarked(pin, id)) {
      out[rank] = id;
      stack[rank] = id;
      sPar[id] = -2;
      ++rank;
    }
  }
  if (tid == 0) {
    W.x.sFreeN[b] = nFree + nRel;
    W.nReleased[b] = nRel;
    if (W.nLive) {
      W.nLive[b] = hw - nFree - nRel;
    }
  }
  if (nRel == 0) {
    return;
  }
  /* 4. rebuild: linear probing has no single-slot delete, so the table is cleared and the entries that stay -- neither
   * the id nor its parent went -- are inserted again */
  unsigned long long* sKey = W.sKey + (size_t)b * W.sSize;
  int32_t* sVal = W.sVal + (size_t)b * W.sSize;
  for (int i = tid; i < W.sSize; i += kCrsOpThreads) {
    sKey[i] = ~0ull;
  }
  __threadfence();
  __syncthreads();
  const uint32_t sMask = (uint32_t)W.sSize - 1u;
  for (int id = tid; id < hw; id += kCrsOpThreads) {
    const int p = sPar[id];
    if (p < 0) {
      continue;
    }
    if ((int32_t)loadCoherent32((const uint32_t*)&sPar[p]) == -2) { /* (a parent's own entry may go meanwhile: -1, not -2) */
      sPar[id] = -1;
      continue;
    }
    const unsigned long long skey = s2lPair(p, sEdge[id]);
    uint32_t slot = (uint32_t)s2lMix(skey) & sMask;
    for (int probes = 0; probes < W.sSize; ++probes) { /* (sSize >= 2 sMax: a free slot always exists) */
      if (atomCas64(&sKey[slot], ~0ull, skey) == ~0ull) {
        sVal[slot] = id;
        break;
      }
      slot = (slot + 1u) & sMask;
    }
  }
}

/* ---- finish: decodeEnd and decodeBegin of the named streams, the others untouched ------------------------------------- */
struct CrsFinishParams {
  const int32_t* which; /* [B] != 0: the stream is named */
  int32_t* skip;        /* [B] what the finish's gather reads as `done`: the stream stopped, or is not named */
  int32_t errUnsupported, errState; /* the FLTX_ERR_* of a stopped stream's status */
};

struct CrFinishParams {
  CrParams c; /* c.s.outScores / tokens / outNHyp (= uttNBeam) / uttFrame / uttStatus, c.histOff: the finish's results */
  CrsParams x;
  CrsFinishParams f;
};

struct CrlFinishParams {
  CrlParams r; /* likewise, and r.words */
  CrsParams x;
  CrsFinishParams f;
};

/* before the gather: only rows of named streams that have not stopped are read (crRowLive) */
FLTX_DEV void crsFinishMask(const CrFinishParams& Z, char*) {
  const int b = (int)(blockIdx.x * kS2sBeginThreads + threadIdx.x);
  if (b < Z.c.s.B) {
    Z.f.skip[b] = Z.c.s.done[b] || Z.f.which[b] == 0 ? 1 : 0;
  }
}

/* a stream the call does not name: its beam listed again as a step without frames lists it, an empty result */
template <typename Hyp>
FLTX_DEV void crsFinishIdle(const CrParams& Q, const Hyp* beam, int b, int nd) {
  const S2sParams& P = Q.s;
  const int K = P.K;
  const int64_t rb = (int64_t)b * K;
  const Hyp* prev = beam + (size_t)(nd & 1) * P.B * K + rb;
  const int nPrev = P.done[b] ? 0 : P.beamN[b];
  for (int k = (int)threadIdx.x; k < K; k += kS2sStepThreads) {
    const bool in = k < nPrev;
    P.outTok[rb + k] = -1;
    P.outBeam[rb + k] = in ? k : -1;
    P.outSrc[rb + k] = in ? (int32_t)(rb + k) : -1;
    Q.outState[rb + k] = in ? prev[k].sid : -1;
  }
  if (threadIdx.x == 0) {
    P.outN[b] = nPrev;
    P.outNHyp[b] = 0;
    P.uttFrame[b] = 0;
    P.uttStatus[b] = 0;
  }
}

/* behind a named stream's decodeEnd and a barrier: its state table emptied (16 bytes a store), and what the finish body
 * left in uttFrame / uttStatus turned into the entries per hypothesis and the FLTX_ERR_* of the status.  Thread 0 then
 * runs the kind's decodeBegin for this b. */
FLTX_DEV void crsFinishRestart(const CrParams& Q, const CrsFinishParams& F, int b) {
  const S2sParams& P = Q.s;
  uint4* keys = (uint4*)(Q.sKey + (size_t)b * Q.sSize); /* (sSize is a power of two >= 2: whole 16-byte pairs) */
  for (int i = (int)threadIdx.x; i < Q.sSize / 2; i += kS2sStepThreads) {
    keys[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  }
  if (threadIdx.x == 0) {
    const int s = P.uttStatus[b];
    P.uttFrame[b] += 1;
    P.uttStatus[b] = (s & (ST_CAND_OVERFLOW | ST_TABLE_FULL | ST_SELECT_FALLBACK)) ? F.errUnsupported
                                                                                    : (s & ST_HLM_MISS) ? F.errState : 0;
  }
}

FLTX_DEV void crsFinishStream(const CrFinishParams& Z, char* smem) {
  const int b = (int)blockIdx.x;
  if (Z.f.which[b] == 0) {
    crsFinishIdle(Z.c, Z.c.beam, b, Z.x.nDec[b]);
    return;
  }
  crStepUtterance<true, true>(Z.c, smem, &Z.x);
  __syncthreads(); /* (the walks have read the rings and the beam the begin writes to) */
  crsFinishRestart(Z.c, Z.f, b);
  if (threadIdx.x == 0) {
    crBeginOne(Z.c, b);
    crsBeginCountsOne(Z.c, Z.x, b);
  }
}

template <int SRC>
FLTX_DEV void crlsFinishStream(const CrlFinishParams& Z, char* smem) {
  const int b = (int)blockIdx.x;
  if (Z.f.which[b] == 0) {
    crsFinishIdle(Z.r.c, Z.r.beam, b, Z.x.nDec[b]);
    return;
  }
  crlStepUtterance<SRC, true, true>(Z.r, smem, &Z.x);
  __syncthreads();
  crsFinishRestart(Z.r.c, Z.f, b);
  if (threadIdx.x == 0) {
    crlBeginOne(Z.r, b);
    crsBeginCountsOne(Z.r.c, Z.x, b);
  }
}

} // namespace fltx
