/*
 * fltx_ctc_rows_plan.h -- the LM rows of the CTC rows decoders, planned on the device (fltx_ctc_rows_plan_begin,
 * fltx_ctc_rows_plan, fltx_ctc_rows_plan_release).
 *
 * A step lists (next_token, next_src_row, next_state, n_rows).  The planner keeps, per decoder,
 *   rowOf[B][sMax]   the LM row of every state id: -1 unplanned, -2 dropped (the store was full when the id came)
 *   freeRows[cap]    a stack of rows whose ids were released, meta = {nFree, highWater, nDropped}
 *   prev[B*K]        the lm_row_of of the call before: a new state's parent row is prev[next_src_row]
 * and turns a list into the next step's lm_row_of plus the compact list of the states that are new.  The result is that of
 * the serial loop "b ascending, k ascending: a state without a row pops the free stack, else takes highWater++, else is
 * dropped": the j-th new state OVERALL takes freeRows[nFree - 1 - j], else highWater + (j - nFree), else -2, and j is a
 * prefix count -- no atomic's arrival order decides a row.  (The sums of the counts are integer atomics on LDS: their
 * order does not matter.)
 *
 * Two launches per plan, a workgroup of kCpThreads >= kS2sMaxBeam threads per utterance, a thread per row:
 *   cpMark     which rows carry a state without a row, which of those is its lowest k (a walk over the lower rows in LDS);
 *              rank[row] = that row's place among the utterance's new states, -(2 + k0) for a later row of the same new
 *              state, -1 else; cnt[b] = the utterance's new states
 *   cpAssign   the sums of cnt below b and over all B (every workgroup adds them up itself: B ints, no scan launch),
 *              then rowOf, the four lists, lm_row_of and its copy.  meta and prev are kept twice and read from one half,
 *              written to the other: a workgroup never reads what another one writes.
 * A release is the same pair: cpReleaseCount counts the listed ids of a stream that hold a row, cpRelease pushes those
 * rows -- stream b ascending, in listed order -- and clears rowOf (for a dropped id too).  fltx_ctc_rows_stream_finish
 * releases every id of the streams it names with the same pair on the ids themselves (cpFinishCount, cpFinishRelease):
 * stream b ascending, ids ascending.
 *
 * The bodies are FLTX_DEV functions on fltx_rt.h's primitives, so tests/emu runs them as it runs the other steps.
 */
#pragma once
#include "fltx_rt.h"

namespace fltx {

constexpr int kCpThreads = 256; /* >= kS2sMaxBeam: a thread per row of the utterance */

struct CpParams {
  int32_t B, K, sMax, rowCap;
  int32_t metaPar, prevPar; /* the half of meta / prev this call reads; it writes the other */
  const int32_t *tok, *src, *state, *nRows; /* the list: [B*K] x 3, [B] */
  int32_t* rowOf;    /* [B][sMax] */
  int32_t* freeRows; /* [rowCap] */
  int32_t* meta;     /* [2][4]: nFree, highWater, nDropped, - */
  int32_t* prev;     /* [2][B*K] */
  int32_t* cnt;      /* [B] */
  int32_t* rank;     /* [B*K] */
  int32_t *lmRowOf, *newRow, *newParent, *newEdge, *newDecRow; /* [B*K] each, the caller's */
  int32_t* counts;   /* [4]: n_new, high_water, n_free, n_dropped */
  const int32_t *released, *nReleased; /* collect's [B][releaseCap], [B] */
  int32_t releaseCap;
};

struct CpLds {
  int32_t v[kCpThreads];
  int32_t wsum[kCpThreads / kWave];
  uint32_t below, all;
};

/* the place of this thread among the workgroup's threads with `flag` (lower threads first); total: how many there are */
FLTX_DEV int cpBlockRank(CpLds& L, bool flag, int& total) {
  const unsigned long long m = waveBallot(flag);
  const int wv = waveId();
  __syncthreads(); /* (the sums of a call before are read) */
  if (laneId() == 0) {
    L.wsum[wv] = popc64(m);
  }
  __syncthreads();
  int at = wavePrefixCount(m);
  total = 0;
  for (int w = 0; w < kCpThreads / kWave; ++w) {
    at += w < wv ? L.wsum[w] : 0;
    total += L.wsum[w];
  }
  return at;
}

/* the sum of cnt[0 .. b) and of cnt[0 .. B), in every thread */
FLTX_DEV void cpSums(const CpParams& P, CpLds& L, int b, int& below, int& all) {
  const int tid = (int)threadIdx.x;
  if (tid == 0) {
    L.below = 0u;
    L.all = 0u;
  }
  __syncthreads();
  uint32_t lo = 0u, sum = 0u;
  for (int i = tid; i < P.B; i += kCpThreads) {
    const uint32_t c = (uint32_t)P.cnt[i];
    sum += c;
    lo += i < b ? c : 0u;
  }
  if (sum) {
    atomAdd32(&L.all, sum);
  }
  if (lo) {
    atomAdd32(&L.below, lo);
  }
  __syncthreads();
  below = (int)L.below;
  all = (int)L.all;
}

FLTX_DEV int cpRowsOf(const CpParams& P, int b) {
  const int n = P.nRows[b];
  return n < 0 ? 0 : n > P.K ? P.K : n;
}

FLTX_DEV void cpMark(const CpParams& P, char* smem) {
  CpLds& L = *(CpLds*)smem;
  const int b = (int)blockIdx.x, k = (int)threadIdx.x;
  const int n = cpRowsOf(P, b);
  const int64_t row = (int64_t)b * P.K + k;
  const int32_t s = k < n ? P.state[row] : -1;
  const bool isNew = k < n && s >= 0 && s < P.sMax && P.rowOf[(int64_t)b * P.sMax + s] == -1;
  L.v[k] = isNew ? s : -1;
  __syncthreads();
  int first = -1; /* the lowest row with this new state */
  if (isNew) {
    first = k;
    for (int j = 0; j < k; ++j) {
      if (L.v[j] == s) {
        first = j;
        break;
      }
    }
  }
  int total;
  const int at = cpBlockRank(L, isNew && first == k, total);
  if (k < P.K) {
    P.rank[row] = !isNew ? -1 : first == k ? at : -(2 + first);
  }
  if (k == 0) {
    P.cnt[b] = total;
  }
}

FLTX_DEV void cpAssign(const CpParams& P, char* smem) {
  CpLds& L = *(CpLds*)smem;
  const int b = (int)blockIdx.x, k = (int)threadIdx.x;
  int off, nNew;
  cpSums(P, L, b, off, nNew);
  const int32_t* cur = P.meta + 4 * P.metaPar;
  int32_t* nxt = P.meta + 4 * (P.metaPar ^ 1);
  const int nFree = cur[0], hw = cur[1], room = P.rowCap - hw;
  const int nListed = nNew < nFree + room ? nNew : nFree + room; /* the dropped ones are the last */
  const int64_t BK = (int64_t)P.B * P.K;
  const int32_t* prevIn = P.prev + BK * P.prevPar;
  int32_t* prevOut = P.prev + BK * (P.prevPar ^ 1);
  const int n = cpRowsOf(P, b);
  const int64_t row = (int64_t)b * P.K + k;
  int32_t out = -1, r = -1, s = -1;
  if (k < n) {
    s = P.state[row];
    if (s >= 0 && s < P.sMax) {
      r = P.rank[row];
      if (r >= 0) { /* a new state at its lowest k: the j-th of the call */
        const int j = off + r;
        out = j < nFree ? P.freeRows[nFree - 1 - j] : j - nFree < room ? hw + (j - nFree) : -2;
        P.rowOf[(int64_t)b * P.sMax + s] = out;
        if (out >= 0) {
          const int32_t sr = P.src[row];
          P.newRow[j] = out;
          P.newParent[j] = sr < 0 || sr >= BK ? -1 : prevIn[sr];
          P.newEdge[j] = sr < 0 ? -1 : P.tok[row];
          P.newDecRow[j] = (int32_t)row;
        }
      } else if (r == -1) {
        out = P.rowOf[(int64_t)b * P.sMax + s];
      }
    }
  }
  L.v[k] = out;
  __syncthreads();
  if (r <= -2) { /* the same new state on a later row: the row its lowest k took */
    out = L.v[-(r + 2)];
  }
  if (k < P.K) {
    out = out < -1 ? -1 : out;
    P.lmRowOf[row] = out;
    prevOut[row] = out;
    if (row >= nListed) {
      P.newRow[row] = -1;
      P.newParent[row] = -1;
      P.newEdge[row] = -1;
      P.newDecRow[row] = -1;
    }
  }
  if (b == 0 && k == 0) {
    const int fromHw = nListed - (nNew < nFree ? nNew : nFree);
    nxt[0] = nFree - (nNew < nFree ? nNew : nFree);
    nxt[1] = hw + fromHw;
    nxt[2] = cur[2] + (nNew - nListed);
    P.counts[0] = nListed;
    P.counts[1] = nxt[1];
    P.counts[2] = nxt[0];
    P.counts[3] = nxt[2];
  }
}

/* the listed id at place i of stream b's released list holds a row */
FLTX_DEV bool cpHoldsRow(const CpParams& P, int b, int i, int n, int32_t& id) {
  id = i < n ? P.released[(int64_t)b * P.releaseCap + i] : -1;
  return id >= 0 && id < P.sMax && P.rowOf[(int64_t)b * P.sMax + id] >= 0;
}

FLTX_DEV int cpReleasedOf(const CpParams& P, int b) {
  const int n = P.nReleased[b];
  return n < 0 ? 0 : n > P.releaseCap ? P.releaseCap : n;
}

FLTX_DEV void cpReleaseCount(const CpParams& P, char* smem) {
  CpLds& L = *(CpLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int n = cpReleasedOf(P, b);
  int sum = 0;
  for (int base = 0; base < n; base += kCpThreads) {
    int32_t id;
    int total;
    cpBlockRank(L, cpHoldsRow(P, b, base + tid, n, id), total);
    sum += total;
  }
  if (tid == 0) {
    P.cnt[b] = sum;
  }
}

FLTX_DEV void cpRelease(const CpParams& P, char* smem) {
  CpLds& L = *(CpLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  int off, all;
  cpSums(P, L, b, off, all);
  const int32_t* cur = P.meta + 4 * P.metaPar;
  int32_t* nxt = P.meta + 4 * (P.metaPar ^ 1);
  const int nFree = cur[0];
  const int n = cpReleasedOf(P, b);
  int at = nFree + off;
  for (int base = 0; base < n; base += kCpThreads) {
    int32_t id;
    int total;
    const bool holds = cpHoldsRow(P, b, base + tid, n, id);
    const int r = cpBlockRank(L, holds, total);
    if (id >= 0 && id < P.sMax) {
      int32_t* at0 = P.rowOf + (int64_t)b * P.sMax + id;
      if (holds && at + r < P.rowCap) { /* (rows pushed <= rows handed out <= rowCap) */
        P.freeRows[at + r] = *at0;
      }
      *at0 = -1;
    }
    at += total;
  }
  if (b == 0 && tid == 0) {
    nxt[0] = nFree + all < P.rowCap ? nFree + all : P.rowCap;
    nxt[1] = cur[1];
    nxt[2] = cur[2];
  }
}

/* fltx_ctc_rows_stream_finish: every id of a named stream below its high-water mark is released, ascending -- the same
 * pair on the ids themselves, queued BEFORE the finish kernel starts the stream's count over */
struct CpFinishParams {
  CpParams p;
  const int32_t* which;  /* [B] != 0: the stream is named */
  const int32_t* sCount; /* [B] ids handed out (may have passed sMax on a full table) */
};

FLTX_DEV int cpFinishIds(const CpFinishParams& F, int b) {
  const int n = F.sCount[b];
  return F.which[b] == 0 || n < 0 ? 0 : n > F.p.sMax ? F.p.sMax : n;
}

FLTX_DEV void cpFinishCount(const CpFinishParams& F, char* smem) {
  const CpParams& P = F.p;
  CpLds& L = *(CpLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int n = cpFinishIds(F, b);
  int sum = 0;
  for (int base = 0; base < n; base += kCpThreads) {
    int total;
    cpBlockRank(L, base + tid < n && P.rowOf[(int64_t)b * P.sMax + base + tid] >= 0, total);
    sum += total;
  }
  if (tid == 0) {
    P.cnt[b] = sum;
  }
}

FLTX_DEV void cpFinishRelease(const CpFinishParams& F, char* smem) {
  const CpParams& P = F.p;
  CpLds& L = *(CpLds*)smem;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  int off, all;
  cpSums(P, L, b, off, all);
  const int32_t* cur = P.meta + 4 * P.metaPar;
  int32_t* nxt = P.meta + 4 * (P.metaPar ^ 1);
  const int nFree = cur[0];
  const int n = cpFinishIds(F, b);
  int at = nFree + off;
  for (int base = 0; base < n; base += kCpThreads) {
    const int id = base + tid;
    int32_t* at0 = P.rowOf + (int64_t)b * P.sMax + id;
    const bool holds = id < n && *at0 >= 0;
    int total;
    const int r = cpBlockRank(L, holds, total);
    if (id < n) {
      if (holds && at + r < P.rowCap) { /* (rows pushed <= rows handed out <= rowCap) */
        P.freeRows[at + r] = *at0;
      }
      *at0 = -1;
    }
    at += total;
  }
  if (b == 0 && tid == 0) {
    nxt[0] = nFree + all < P.rowCap ? nFree + all : P.rowCap;
    nxt[1] = cur[1];
    nxt[2] = cur[2];
  }
}

} // namespace fltx
