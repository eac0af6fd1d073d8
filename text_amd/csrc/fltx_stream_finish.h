/*
 * fltx_stream_finish.h -- finish and restart single streams of a classic stream batch (fltx_stream_finish).
 * Included after fltx_stream_partials.h.
 *
 * The call's launches, over the list of the named streams (one workgroup each):
 *
 *   1. the decode kernel with doEnd = 1 and no frames (uttMap): decodeEnd on the parked beam, the n-best's three scores
 *      straight into the finish's own score buffer;
 *   2. sfFinishStream: the back-trace from decodeEnd's records over the frames in the buffer into the finish's own token
 *      (and word) rows, and n_hyp / length / status of all B streams -- zero for the streams not named;
 *   3. sfRestartStream: what launchCompact(d, 0) does for a new stream, for this one, plus the two things a new BATCH of
 *      streams gets from a new epoch and a single stream must get on its own (see below);
 *   4. the decode kernel with doBegin = 1 and no frames (uttMap): decodeBegin -- the root in the parked beam and at the first
 *      history row, counts and status cleared, maskTab row 0, the id counter, the n-gram start context.
 *
 * The back-trace is backtraceUtterance's plain-record walk: hypothesis k starts at slot k of the last frame and follows
 * the parents, -1 below a pruned cut.  The chain of parents is a chain of dependent loads, so the parent column of the
 * rows it is about to visit is fetched into LDS by all threads, R = kSfStageInts / K rows at a time (as streamOpUtterance
 * stages the rows it visits), and a lane per hypothesis walks there; a lane's slot between two windows waits in LDS.  The
 * token and the word of a visited record are read from HBM at the slot the walk has reached: loads that nothing waits
 * for.  A beam too wide for two rows walks HBM.  A parent outside [-1, K) ends a hypothesis' walk.
 *
 * The two decoder-wide items.  The state table (generic engine) tags a key with the decoder's epoch, and a key whose tag
 * is not the current epoch is a free slot; epochs start at 1.  A restarted stream's slice is therefore ZEROED: free
 * under every epoch, and no other stream's slice or the epoch itself is touched.  The LM score cache is per stream
 * (lmCache + b * kLmCache) and tagged by (state id, word): the restarted stream hands its ids out again, so its slice --
 * and only its slice -- is set to all ones, which no (id, word) tag equals.
 */
#pragma once

namespace fltx {

constexpr int kSfThreads = 256;
constexpr int kSfStageInts = kStageInts; /* entries of the staged parent column (32 KB) */
constexpr int kSfMaxBeam = kSpMaxBeam;   /* hypotheses whose slot waits in LDS between two windows */

struct SfParams {
  int32_t B, K, lex, nNamed;
  int32_t errState, errUnsupported; /* FLTX_ERR_* a status row maps to */
  const int32_t* named;             /* [nNamed] the named streams, ascending */
  const int32_t* which;             /* [B] != 0: named */
  const int2* histPT;
  const int32_t* histW;
  const int64_t* histOff;           /* [B + 1] history rows of stream b, and where its result rows start */
  const int32_t *uttFrame, *uttNBeam, *uttStatus; /* as decodeEnd left them */
  int32_t *nHyp, *length, *status;  /* [B] out */
  int32_t *tokens, *words;          /* out: hypothesis k of stream b at histOff[b] + k * length[b] (words: lexicon kind) */
};

struct SfLds {
  int32_t cur[kSfMaxBeam];
  int32_t par[kSfStageInts];
};

struct SfRestartParams {
  int32_t nNamed;
  const int32_t* named;
  int64_t idCap;
  uint32_t stateCap;
  uint32_t* idPar;              /* recycling streams, else null */
  int32_t* uttNextId;           /* where the engine counts ids, else null */
  unsigned long long* maskTab;  /* childTab / maskTab family, else null */
  unsigned long long* stateTab; /* generic family: [B * stateCap], else null */
  uint32_t* stateVal;           /* generic family with recycling, else null */
  unsigned long long* lmCache;  /* n-gram LM score cache, else null */
  int64_t* uttFirst;            /* [B] frames pruned off */
};

/* what fltx_result_count would report for a status row */
FLTX_DEV int sfStatusCode(const SfParams& Q, int st) {
  if (st & (ST_CAND_OVERFLOW | ST_TABLE_FULL | ST_SELECT_FALLBACK)) {
    return Q.errUnsupported;
  }
  return (st & ST_HLM_MISS) ? Q.errState : 0;
}

FLTX_DEV void sfFinishStream(const SfParams& Q, char* smem) {
  SfLds& L = *(SfLds*)smem;
  const int tid = (int)threadIdx.x, W = (int)blockDim.x;
  /* the counts of the streams not named: zero (the workgroups share them) */
  for (int i = (int)blockIdx.x * W + tid; i < Q.B; i += Q.nNamed * W) {
    if (Q.which[i] == 0) {
      Q.nHyp[i] = 0;
      Q.length[i] = 0;
      Q.status[i] = 0;
    }
  }
  const int b = Q.named[blockIdx.x];
  const int K = Q.K;
  const int ff = Q.uttFrame[b];
  const int len = ff + 1;
  const int64_t hb = Q.histOff[b];
  int status = sfStatusCode(Q, Q.uttStatus[b]);
  if (status == 0 && (ff < 0 || hb + (int64_t)K * len > Q.histOff[b + 1])) {
    status = Q.errState; /* (counts no stream can have: nothing is walked) */
  }
  int nh = Q.uttNBeam[b];
  nh = nh < 0 ? 0 : (nh > K ? K : nh);
  if (status != 0 || (Q.lex && ff < 1)) { /* LexiconDecoder.cpp:276-280: nothing before the first frame */
    nh = 0;
  }
  if (tid == 0) {
    Q.nHyp[b] = nh;
    Q.length[b] = status == Q.errState && ff < 0 ? 0 : len;
    Q.status[b] = status;
  }
  if (nh == 0) {
    return;
  }
  int32_t* tokens = Q.tokens + hb;
  int32_t* words = Q.lex ? Q.words + hb : nullptr;
  /* a record's token and word at the slot the walk has reached; -1 below a pruned cut */
  auto emit = [&](int k, int fr, int s) {
    int tokv = -1, wv = -1;
    if (s >= 0) {
      const int64_t idx = hb + (int64_t)fr * K + s;
      tokv = Q.histPT[idx].y;
      wv = Q.lex ? Q.histW[idx] : -1;
    }
    tokens[(int64_t)k * len + fr] = tokv;
    if (words) {
      words[(int64_t)k * len + fr] = wv;
    }
  };
  int R = kSfStageInts / K; /* rows a window stages */
  if (R < 2 || nh > kSfMaxBeam) { /* a beam too wide for the staging area: a thread per hypothesis through HBM */
    for (int k = tid; k < nh; k += W) {
      int s = k;
      for (int fr = ff; fr >= 0; --fr) {
        emit(k, fr, s);
        if (s >= 0) {
          const int p = Q.histPT[hb + (int64_t)fr * K + s].x;
          s = (p < 0 || p >= K) ? -1 : p;
        }
      }
    }
    return;
  }
  for (int k = tid; k < nh; k += W) {
    L.cur[k] = k;
  }
  for (int hi = ff; hi >= 0; hi -= R) {
    const int lo = hi - R + 1 > 0 ? hi - R + 1 : 0;
    const int cnt = (hi - lo + 1) * K;
    const int64_t src = hb + (int64_t)lo * K;
    __syncthreads(); /* (whoever walked the window before has) */
    for (int e0 = tid; e0 < cnt; e0 += 4 * W) { /* (four records in flight per thread) */
      int32_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W;
        v[u] = e < cnt ? Q.histPT[src + e].x : -1;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W;
        if (e < cnt) {
          L.par[e] = v[u];
        }
      }
    }
    __syncthreads();
    for (int k = tid; k < nh; k += W) { /* (a hypothesis is its thread's alone: cur[k] needs no barrier) */
      int s = L.cur[k];
      for (int fr = hi; fr >= lo; --fr) {
        emit(k, fr, s);
        if (s >= 0) {
          const int p = L.par[(fr - lo) * K + s];
          s = (p < 0 || p >= K) ? -1 : p;
        }
      }
      L.cur[k] = s;
    }
  }
}

FLTX_DEV void sfRestartStream(const SfRestartParams& Q, char*) {
  const int tid = (int)threadIdx.x, W = (int)blockDim.x;
  const int b = Q.named[blockIdx.x];
  if (tid == 0) { /* compactStates mode 0, and the counts decodeBegin does not own */
    if (Q.idPar) {
      Q.idPar[(size_t)b * Q.idCap] = kNoParent32;
    }
    if (Q.uttNextId) {
      Q.uttNextId[b] = 1;
    }
    if (Q.maskTab) {
      Q.maskTab[(size_t)b * Q.idCap] = 0ull;
    }
    Q.uttFirst[b] = 0;
  }
  if (Q.stateTab) { /* keys of no epoch: free slots */
    for (uint32_t s = (uint32_t)tid; s < Q.stateCap; s += (uint32_t)W) {
      Q.stateTab[(size_t)b * Q.stateCap + s] = 0ull;
    }
  }
  if (Q.stateVal) {
    for (uint32_t s = (uint32_t)tid; s < Q.stateCap; s += (uint32_t)W) {
      Q.stateVal[(size_t)b * Q.stateCap + s] = kEmpty;
    }
  }
  if (Q.lmCache) { /* the ids are handed out again: nothing cached under the old ones may answer */
    for (int i = tid; i < kLmCache; i += W) {
      Q.lmCache[(size_t)b * kLmCache + i] = ~0ull;
    }
  }
}

} // namespace fltx
