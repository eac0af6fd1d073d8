/*
 * fltx_stream_partials.h -- the partial transcript of every stream in one launch, with its stable prefix
 * (fltx_stream_partials).  Included after fltx_ctc_rows_stream.h and fltx_transcript.h.
 *
 * One workgroup per stream, on either history layout behind one accessor (SpClassicHist: histPT / histW / histS at
 * histOff[b] + frame * K + slot; SpRowsHist<LEX>: the ring of int2 / S2lRec records with sHist).  Three things:
 *
 *   1. getBestHypothesis(lookBack): findBestAncestor from slot 0 of the current beam (the beams are sorted best first),
 *      lookBack records up and, with a lexicon, on to a complete hypothesis (streamOpUtterance op 0 and crsBest say the
 *      same; they stay as they are).  The ancestor's path goes to a scratch row [cap] of frame entries.
 *   2. The stable prefix: the set of distinct ancestors of the current beam at frame j is a K-bit set in LDS.  Per frame
 *      the lanes are tiled over the set's 64-bit words (a wave skips a word that is empty), every set slot ORs its
 *      parent's bit into the next set.  The walk ends when one bit is left -- every later frame descends from that one
 *      hypothesis, so entries 0 .. j are final -- or at buffer frame 0.  K walkers would each go all the way down; the
 *      set shrinks wherever two paths join, and with it the work per frame and the number of frames.
 *   3. The collapse's count: wave 0 walks the scratch row with fltx_transcript.h's rule (trWalkSpan) and leaves nTok /
 *      nWord for trScanRows / trWriteRows, and in the same pass the tokens and words below min(stable_frames, length).
 *
 * Every chain of parents is walked in LDS: the rows it is about to visit are fetched R = kStageInts / 2 / K at a time
 * by all threads (parent, token, word columns), as op 0 does.  A beam too wide for two rows reads HBM through the same
 * accessor.  Every loop is bounded by the frames in the buffer; a parent outside [-1, K) ends the stream's walk with
 * status = errState.
 */
#pragma once

namespace fltx {

constexpr int kSpThreads = 256;
constexpr int kSpMaxBeam = 2560;              /* bits of a set: the classic kinds' beams reach 2 500 */
constexpr int kSpSetWords = kSpMaxBeam / 64;
constexpr int kSpStageInts = kStageInts / 2;  /* entries of one staged column */
constexpr int kSpPathRows = 1024;             /* frames a window of the walks spans at most */

struct SpParams {
  int32_t B, K, lex, lookBack, cap, blank;
  int32_t errState, errUnsupported; /* FLTX_ERR_* a status row maps to */
  /* classic streams */
  const int2* histPT;
  const int32_t* histW;
  const double* histS;
  const int64_t* histOff;
  const int32_t *uttFrame, *uttNBeam, *uttStatus;
  const int64_t* uttFirst;
  /* rows streams */
  const void* hist;
  const double* sHist;
  const int32_t *nDec, *base, *beamN, *status;
  int32_t ring;
  /* out */
  int32_t *rowTok, *rowWrd; /* [B][cap] frame rows (rowWrd: the lexicon kinds) */
  int64_t* rowOff;          /* [B] = b * cap */
  int32_t *length, *stableFrames, *stableTokens, *stableWords, *outStatus; /* [B] */
  int64_t* firstFrame;      /* [B] */
  double* scores;           /* [B][3] */
  int32_t *nTok, *nWord;    /* [B] what trScanRows reads */
};

struct SpLds {
  int32_t f, s, steps, done, bad, pad[3];
  unsigned long long set[2][kSpSetWords];
  int32_t path[kSpPathRows];
  int32_t par[kSpStageInts], tok[kSpStageInts], wrd[kSpStageInts];
};

struct SpRec {
  int parent, token, word;
};

FLTX_DEV int spStatusCode(const SpParams& Q, int st) {
  if (st & (ST_CAND_OVERFLOW | ST_TABLE_FULL | ST_SELECT_FALLBACK)) {
    return Q.errUnsupported;
  }
  return (st & ST_HLM_MISS) ? Q.errState : 0;
}

/* the classic streams: records at histOff[b] + frame * K + slot, frame 0 the buffer's first */
struct SpClassicHist {
  const SpParams& Q;
  const int b;
  const int64_t base;
  __device__ __forceinline__ SpClassicHist(const SpParams& q, int bb) : Q(q), b(bb), base(q.histOff[bb]) {}
  __device__ __forceinline__ int lastFrame() const { return Q.uttFrame[b]; }
  __device__ __forceinline__ int beamSize() const { return Q.uttNBeam[b]; }
  __device__ __forceinline__ int status() const { return spStatusCode(Q, Q.uttStatus[b]); }
  __device__ __forceinline__ long long first() const { return Q.uttFirst[b]; }
  __device__ __forceinline__ SpRec rec(int f, int s) const {
    const int64_t i = base + (int64_t)f * Q.K + s;
    const int2 pt = Q.histPT[i];
    return SpRec{pt.x, pt.y, Q.lex ? Q.histW[i] : -1};
  }
  __device__ __forceinline__ const double* scores(int f, int s) const { return Q.histS + 3 * (base + (int64_t)f * Q.K + s); }
};

/* the rows streams: buffer frame f is ring row (base[b] + f) % ring */
template <bool LEX>
struct SpRowsHist {
  using Kd = CrsKind<LEX>;
  const SpParams& Q;
  const int b;
  const int nd, first0;
  const int64_t BK, rb;
  __device__ __forceinline__ SpRowsHist(const SpParams& q, int bb)
      : Q(q), b(bb), nd(q.nDec[bb]), first0(q.base[bb]), BK((int64_t)q.B * q.K), rb((int64_t)bb * q.K) {}
  __device__ __forceinline__ int lastFrame() const { return nd - first0; }
  __device__ __forceinline__ int beamSize() const { return Q.beamN[b]; }
  __device__ __forceinline__ int status() const { return spStatusCode(Q, Q.status[b]); }
  __device__ __forceinline__ long long first() const { return first0; }
  __device__ __forceinline__ int64_t at(int f, int s) const { return (int64_t)((first0 + f) % Q.ring) * BK + rb + s; }
  __device__ __forceinline__ SpRec rec(int f, int s) const {
    const typename Kd::Rec r = ((const typename Kd::Rec*)Q.hist)[at(f, s)];
    return SpRec{Kd::parent(r), Kd::token(r), Kd::word(r)};
  }
  __device__ __forceinline__ const double* scores(int f, int s) const { return Q.sHist + 3 * at(f, s); }
};

/* OR over the wave, the result in every lane (the DPP scan of fltx_rt.h's waveMax64: 0 is the identity here too) */
#ifndef FLTX_EMU
FLTX_DEV unsigned long long spOr64(unsigned long long a, unsigned long long b) { return a | b; }
FLTX_DEV unsigned long long spWaveOr64(unsigned long long v) {
  FLTX_DPP_SCAN(v, spOr64, dppTake64)
  return waveBcastLast64(v);
}
#else
FLTX_DEV unsigned long long spWaveOr64(unsigned long long v) {
  for (int d = 1; d < kWave; d <<= 1) {
    v |= waveShflXor64(v, d);
  }
  return v;
}
#endif

template <class H>
FLTX_DEV void spStream(const SpParams& Q, char* smem) {
  SpLds& L = *(SpLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, W = (int)blockDim.x;
  const H h(Q, b);
  const int K = Q.K;
  const int F = h.lastFrame(); /* the buffer holds frames 0 .. F */
  int n = h.beamSize();
  n = n < 0 ? 0 : (n > K ? K : n);
  int status = h.status();
  if (status == 0 && (F < 0 || F >= Q.cap || K > kSpMaxBeam)) {
    status = Q.errState; /* (counts no stream can have: nothing is walked) */
  }
  const bool live = status == 0;
  int R = kSpStageInts / K; /* rows a window stages */
  R = R > kSpPathRows ? kSpPathRows : R;
  if (R < 2) {
    R = 0; /* a beam too wide for the staging area: the accessor reads HBM */
  }
  const int RW = R ? R : kSpPathRows; /* frames a window spans */

  /* rows [top - RW + 1, top] are the window; staged in LDS when R > 0, unless the rows staged last cover them (the
   * three walks of a short buffer share one fetch).  Every thread keeps the staged range [slo, shi] in registers. */
  int slo = 1, shi = 0;
  auto stage = [&](int top) {
    const int lo = top - RW + 1 > 0 ? top - RW + 1 : 0;
    if (!R || (slo <= lo && top <= shi)) {
      return lo;
    }
    __syncthreads(); /* (whoever read the window before has) */
    slo = lo;
    shi = top;
    const int cnt = (top - lo + 1) * K;
    for (int e0 = tid; e0 < cnt; e0 += 4 * W) { /* (four records in flight per thread) */
      SpRec r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W;
        if (e < cnt) {
          r[u] = h.rec(lo + e / K, e % K);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W;
        if (e < cnt) {
          L.par[e] = r[u].parent;
          L.tok[e] = r[u].token;
          L.wrd[e] = r[u].word;
        }
      }
    }
    __syncthreads();
    return lo;
  };
  auto rec = [&](int f, int s) {
    if (f >= slo && f <= shi) {
      const int e = (f - slo) * K + s;
      return SpRec{L.par[e], L.tok[e], L.wrd[e]};
    }
    return h.rec(f, s);
  };

  /* ---- 1. the best ancestor (findBestAncestor, Utils.h:268-310) ---------------------------------------------------- */
  const bool empty = !live || n == 0 || (Q.lex && F - Q.lookBack < 1); /* LexiconDecoder.cpp:286 */
  if (tid == 0) {
    L.f = F;
    L.s = empty ? -1 : 0;
    L.steps = 0;
    L.done = empty ? 1 : 0;
    L.bad = 0;
  }
  __syncthreads();
  const int maxLookBack = Q.lookBack + kLookBackLimit;
  for (int w = 0; w <= F + 1; ++w) { /* (a window ends at least one frame below the one before) */
    const int top = L.f, over = L.done;
    __syncthreads(); /* (every thread has read the walk's state before thread 0 moves it) */
    if (over) {
      break;
    }
    const int wlo = stage(top);
    if (tid == 0) {
      int f = L.f, s = L.s, m = L.steps;
      bool done = false;
      for (int it = 0; it <= F + 1 && !done; ++it) {
        if (m < Q.lookBack) {
          if (f == 0) { /* the parent of the buffer's first frame is null */
            s = -1;
            done = true;
            break;
          }
          if (f < wlo) {
            break; /* the next rows */
          }
          const int p = rec(f, s).parent;
          if (p < -1 || p >= K) {
            L.bad = 1;
          }
          s = (p < 0 || p >= K) ? -1 : p;
          --f;
          ++m;
          done = s < 0;
          continue;
        }
        if (!Q.lex || f == 0) { /* complete: every lexicon-free hypothesis is; no parent */
          done = true;
          break;
        }
        if (f < wlo || f - 1 < wlo) {
          break; /* the parent's row is not here */
        }
        const int p = rec(f, s).parent;
        if (p < 0 || p >= K) {
          L.bad = p < -1 || p >= K ? 1 : L.bad;
          done = true; /* no parent */
          break;
        }
        if (rec(f - 1, p).word >= 0) { /* the parent ended a word (LexiconDecoder.h:97-99) */
          done = true;
          break;
        }
        ++m;
        s = p;
        --f;
        done = m == maxLookBack;
      }
      L.f = f;
      L.s = s;
      L.steps = m;
      L.done = done ? 1 : 0;
    }
    __syncthreads();
  }
  __syncthreads();
  const int f0 = L.f;
  const int s0 = (L.done && !L.bad) ? L.s : -1;
  const int len = s0 >= 0 ? f0 + 1 : 0;
  __syncthreads();

  /* ---- the ancestor's path -> the scratch row (getHypothesis, Utils.h:229-250) ---------------------------------------- */
  if (tid == 0) {
    L.f = s0 >= 0 ? f0 : -1;
    L.s = s0;
  }
  __syncthreads();
  int32_t* rowTok = Q.rowTok + (int64_t)b * Q.cap;
  int32_t* rowWrd = Q.lex ? Q.rowWrd + (int64_t)b * Q.cap : nullptr;
  for (int w = 0; w <= F + 1; ++w) {
    const int top = L.f;
    __syncthreads();
    if (top < 0) {
      break;
    }
    const int wlo = stage(top);
    if (tid == 0) {
      int s = L.s;
      for (int fr = top; fr >= wlo; --fr) {
        L.path[fr - wlo] = s;
        if (s >= 0 && fr > 0) {
          const int p = rec(fr, s).parent;
          if (p < -1 || p >= K) {
            L.bad = 1;
          }
          s = (p < 0 || p >= K) ? -1 : p;
        }
      }
      L.f = wlo - 1;
      L.s = s;
    }
    __syncthreads();
    for (int i = tid; i <= top - wlo; i += W) {
      const int s = L.path[i];
      SpRec r = SpRec{-1, -1, -1};
      if (s >= 0) {
        r = rec(wlo + i, s);
      }
      rowTok[wlo + i] = r.token;
      if (rowWrd) {
        rowWrd[wlo + i] = r.word;
      }
    }
    __syncthreads();
  }
  __syncthreads();

  /* ---- 2. the stable prefix: the beam's distinct ancestors, frame by frame -------------------------------------------- */
  const int nW = (K + 63) >> 6, lane = laneId(), nWaves = W >> 6;
  int stable = 0;
  bool badParent = false;
  if (nW == 1) {
    /* a beam of up to 64: the set is one word, which every wave keeps in a register and walks with on its own (lane =
     * slot, the next set an OR over the wave) -- all waves get the same answer, and no barrier or LDS atomic lies on
     * the chain of frames, which is the kernel's longest */
    unsigned long long m = !live || n == 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
    int wlo = F + 1; /* (no window yet) */
    for (int j = F; j >= 0 && m != 0ull; --j) {
      if ((m & (m - 1ull)) == 0ull) {
        stable = j + 1;
        break;
      }
      if (j == 0) {
        break; /* several parentless hypotheses */
      }
      if (j < wlo) {
        wlo = stage(j);
      }
      const bool on = (m >> lane) & 1ull;
      const int p = on ? rec(j, lane).parent : 0;
      if (waveBallot(on && (p < 0 || p >= K)) != 0ull) { /* (a frame above the first has a parent) */
        badParent = true;
        break;
      }
      m = spWaveOr64(on ? 1ull << p : 0ull);
    }
  } else {
    for (int i = tid; i < nW; i += W) {
      const int lo = i << 6;
      L.set[0][i] = !live || n <= lo ? 0ull : (n - lo >= 64 ? ~0ull : ((1ull << (n - lo)) - 1ull));
      L.set[1][i] = 0ull;
    }
    __syncthreads();
    int count = live ? n : 0, cur = 0;
    int wlo = F + 1; /* (no window yet) */
    for (int j = F; j >= 0 && count > 0; --j) {
      if (count == 1) {
        stable = j + 1;
        break;
      }
      if (j == 0) {
        break; /* several parentless hypotheses */
      }
      if (j < wlo) {
        wlo = stage(j);
      }
      unsigned long long* from = L.set[cur];
      unsigned long long* to = L.set[cur ^ 1];
      for (int w = waveId(); w < nW; w += nWaves) {
        const unsigned long long m = from[w];
        if (m == 0ull) {
          continue;
        }
        if ((m >> lane) & 1ull) {
          const int p = rec(j, (w << 6) + lane).parent;
          if (p < 0 || p >= K) {
            L.bad = 1; /* (a frame above the first has a parent) */
          } else {
            (void)atomOr64(&to[p >> 6], 1ull << (p & 63));
          }
        }
      }
      __syncthreads();
      int c = 0;
      for (int w = 0; w < nW; ++w) {
        c += popc64(to[w]);
      }
      const int bad = L.bad;
      for (int i = tid; i < nW; i += W) {
        from[i] = 0ull;
      }
      __syncthreads();
      if (bad) {
        count = 0;
        break;
      }
      count = c;
      cur ^= 1;
    }
  }
  __syncthreads();
  if (L.bad || badParent) {
    status = Q.errState;
    stable = 0;
  }
  const int outLen = status == 0 ? len : 0;

  /* ---- 3. what the stream reports; the collapse's count on the row just written ----------------------------------------- */
  if (tid == 0) {
    Q.rowOff[b] = (int64_t)b * Q.cap;
    Q.length[b] = outLen;
    Q.stableFrames[b] = stable;
    Q.outStatus[b] = status;
    Q.firstFrame[b] = h.first();
    double sc[3] = {0.0, 0.0, 0.0};
    if (outLen > 0) {
      const double* p = h.scores(f0, s0);
      sc[0] = p[0];
      sc[1] = p[1];
      sc[2] = p[2];
    }
    Q.scores[3 * b] = sc[0];
    Q.scores[3 * b + 1] = sc[1];
    Q.scores[3 * b + 2] = sc[2];
  }
  __threadfence();
  __syncthreads();
  if (tid < kWave) {
    TrParams T{};
    T.blank = Q.blank;
    int nk = 0, nw = 0, nkb = 0, nwb = 0;
    trWalkSpan<false, true>(T, rowTok, rowWrd, outLen, 0, 0, stable < outLen ? stable : outLen, nk, nw, nkb, nwb);
    if (tid == 0) {
      Q.nTok[b] = nk;
      Q.nWord[b] = nw;
      Q.stableTokens[b] = nkb;
      Q.stableWords[b] = nwb;
    }
  }
}

/* kind: 0 the classic streams, 1 / 2 the lexicon-free / lexicon rows streams */
template <int KIND>
FLTX_DEV void spPartials(const SpParams& Q, char* smem) {
  if constexpr (KIND == 0) {
    spStream<SpClassicHist>(Q, smem);
  } else {
    spStream<SpRowsHist<KIND == 2>>(Q, smem);
  }
}

} // namespace fltx
