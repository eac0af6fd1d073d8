/*
 * fltx_transcript.h -- collapsed transcripts from frame rows in HBM (fltx_collapse_rows, fltx_result_transcripts).
 *
 * A row is `len` int32 tokens (and, optionally, as many word entries) at an arbitrary element offset.  The rule, with
 * `blank < 0` meaning that nothing is a blank:
 *   position i is KEPT iff tok[i] >= 0, tok[i] != blank and (i == 0 or tok[i] != tok[i - 1]) -- the RAW previous entry, so a
 *   blank or a -1 between two equal tokens makes the second one a new token;
 *   a kept position yields (tokens, timesteps) = (tok[i], i);
 *   every position with wrd[i] >= 0 yields (words, word_timesteps, word_tok_end) = (wrd[i], i, kept positions <= i).
 *
 * Three kernels, no atomics:
 *   trCountRows  one wave per row, kTrRowsPerBlock waves per workgroup: tiles of 64 entries, one int32 per lane (coalesced
 *                whatever the row's start), the previous token from the lower lane, lane 0's from the tile before (a
 *                scalar carry); ballot + popcount -> nTok[row], nWord[row]
 *   trScanRows   ONE workgroup: exclusive int64 prefix sums tokOff / wordOff [rows + 1] in chunks of kTrScanChunk rows
 *                (eight per thread) with a running carry; totals[0..1] = the two sums (what the host reads to size the output),
 *                totals[0] = -1 if some row's length is negative
 *   trWriteRows  the walk again: a kept entry goes to off[row] + kept so far + wavePrefixCount(ballot)
 *
 * The bodies are FLTX_DEV functions on fltx_rt.h's primitives, so tests/emu runs them as it runs the other steps.
 */
#pragma once
#include "fltx_rt.h"

namespace fltx {

constexpr int kTrRowsPerBlock = 4;                 /* waves (= rows) per workgroup of the count / write kernels */
constexpr int kTrThreads = kTrRowsPerBlock * kWave;
constexpr int kTrScanThreads = 256;                /* the scan's workgroup */
constexpr int kTrScanRows = 8;                     /* ... rows per thread and step */
constexpr int kTrScanChunk = kTrScanThreads * kTrScanRows;

struct TrParams {
  const int32_t* tok;
  const int32_t* wrd;    /* null: no word row */
  const int64_t* rowOff; /* [nRows] element offset of a row in tok / wrd */
  const int32_t* rowLen; /* [nRows] */
  int64_t nRows;
  int32_t blank;
  int32_t *nTok, *nWord;      /* [nRows] */
  int64_t *tokOff, *wordOff;  /* [nRows + 1] */
  int64_t* totals;            /* [2] */
  int32_t *tokens, *timesteps, *words, *wordT, *wordEnd;
};

struct TrScanLds {
  long long sum[kTrScanThreads / kWave][2];
  int bad[kTrScanThreads / kWave];
};

/* The walk of one row -- len entries at t (and w, which may be null) -- by one wave.  WRITE = false counts, WRITE = true
 * stores at the offsets to / wo.  -> kept tokens in nk, words in nw (the same in every lane); LIMIT: those of them at
 * positions below `limit` in nkBelow / nwBelow as well (fltx_stream_partials.h: the stable part of a partial result). */
template <bool WRITE, bool LIMIT>
FLTX_DEV void trWalkSpan(const TrParams& Q, const int32_t* t, const int32_t* w, int len, int64_t to, int64_t wo, int limit,
                         int& nkOut, int& nwOut, int& nkBelow, int& nwBelow) {
  const int lane = laneId();
  int nk = 0, nw = 0, nkb = 0, nwb = 0;
  int32_t carry = -1; /* the last entry of the tile before (tile 0: position 0 compares with nothing) */
  for (int64_t base = 0; base < (int64_t)len; base += kWave) {
    const int64_t i = base + lane;
    const bool in = i < (int64_t)len;
    const int32_t v = in ? t[i] : -1;
    int32_t prev = (int32_t)waveGather32((uint32_t)v, (lane + kWave - 1) & (kWave - 1));
    if (lane == 0) {
      prev = carry;
    }
    carry = (int32_t)waveReadLane32((uint32_t)v, kWave - 1);
    const bool keep = in && v >= 0 && v != Q.blank && (i == 0 || v != prev);
    const unsigned long long km = waveBallot(keep);
    const int kBelow = wavePrefixCount(km);
    if (LIMIT) {
      nkb += popc64(waveBallot(keep && i < (int64_t)limit));
    }
    if (WRITE && keep) {
      Q.tokens[to + nk + kBelow] = v;
      Q.timesteps[to + nk + kBelow] = (int32_t)i;
    }
    if (w) {
      const int32_t x = in ? w[i] : -1;
      const unsigned long long wm = waveBallot(x >= 0);
      if (WRITE && x >= 0) {
        const int64_t o = wo + nw + wavePrefixCount(wm);
        Q.words[o] = x;
        Q.wordT[o] = (int32_t)i;
        Q.wordEnd[o] = nk + kBelow + (keep ? 1 : 0);
      }
      nw += popc64(wm);
      if (LIMIT) {
        nwb += popc64(waveBallot(x >= 0 && i < (int64_t)limit));
      }
    }
    nk += popc64(km);
  }
  nkOut = nk;
  nwOut = nw;
  nkBelow = nkb;
  nwBelow = nwb;
}

/* ... of row `row` of Q */
template <bool WRITE>
FLTX_DEV void trWalkRow(const TrParams& Q, int64_t row, int& nkOut, int& nwOut) {
  const int64_t at = Q.rowOff[row];
  int below0 = 0, below1 = 0;
  trWalkSpan<WRITE, false>(Q, Q.tok + at, Q.wrd ? Q.wrd + at : nullptr, Q.rowLen[row], WRITE ? Q.tokOff[row] : 0,
                           WRITE ? Q.wordOff[row] : 0, 0, nkOut, nwOut, below0, below1);
}

FLTX_DEV void trCountRows(const TrParams& Q, char*) {
  const int64_t row = (int64_t)blockIdx.x * kTrRowsPerBlock + waveUniform(waveId());
  if (row >= Q.nRows) {
    return; /* (the whole wave) */
  }
  int nk = 0, nw = 0;
  if (Q.rowLen[row] >= 0) {
    trWalkRow<false>(Q, row, nk, nw);
  } else {
    nk = -1; /* the scan reports it */
  }
  if (laneId() == 0) {
    Q.nTok[row] = nk;
    Q.nWord[row] = nw;
  }
}

FLTX_DEV void trWriteRows(const TrParams& Q, char*) {
  const int64_t row = (int64_t)blockIdx.x * kTrRowsPerBlock + waveUniform(waveId());
  if (row >= Q.nRows) {
    return;
  }
  int nk = 0, nw = 0;
  trWalkRow<true>(Q, row, nk, nw);
}

/* inclusive sum over the wave (int64: the offsets of a call are not bounded by 2^31) */
FLTX_DEV long long trWaveScan64(long long x) {
  const int lane = laneId();
  for (int d = 1; d < kWave; d <<= 1) {
    const long long u = (long long)waveShfl64((unsigned long long)x, (lane + kWave - d) & (kWave - 1));
    if (lane >= d) {
      x += u;
    }
  }
  return x;
}

FLTX_DEV void trScanRows(const TrParams& Q, char* smem) {
  TrScanLds& L = *(TrScanLds*)smem;
  const int tid = (int)threadIdx.x, lane = laneId(), wv = waveId();
  constexpr int kWaves = kTrScanThreads / kWave;
  long long carryT = 0, carryW = 0;
  bool bad = false;
  /* a thread takes kTrScanRows consecutive rows (a serial sum in registers), the workgroup kTrScanChunk per step: the
   * steps -- a wave scan, two barriers -- are what the kernel's time is made of */
  for (int64_t base = 0; base < Q.nRows; base += kTrScanChunk) {
    const int64_t r0 = base + (int64_t)tid * kTrScanRows;
    int a[kTrScanRows], b[kTrScanRows];
    long long ta = 0, tb = 0;
#pragma unroll
    for (int k = 0; k < kTrScanRows; ++k) {
      a[k] = 0;
      b[k] = 0;
      if (r0 + k < Q.nRows) {
        a[k] = Q.nTok[r0 + k];
        b[k] = Q.nWord[r0 + k];
        if (a[k] < 0) {
          bad = true;
          a[k] = 0;
        }
      }
      ta += a[k];
      tb += b[k];
    }
    const long long sa = trWaveScan64(ta), sb = trWaveScan64(tb);
    if (lane == kWave - 1) {
      L.sum[wv][0] = sa;
      L.sum[wv][1] = sb;
    }
    __syncthreads();
    long long atT = carryT + sa - ta, atW = carryW + sb - tb;
    for (int k = 0; k < kWaves; ++k) {
      if (k < wv) {
        atT += L.sum[k][0];
        atW += L.sum[k][1];
      }
      carryT += L.sum[k][0];
      carryW += L.sum[k][1];
    }
#pragma unroll
    for (int k = 0; k < kTrScanRows; ++k) {
      if (r0 + k < Q.nRows) {
        Q.tokOff[r0 + k] = atT;
        Q.wordOff[r0 + k] = atW;
      }
      atT += a[k];
      atW += b[k];
    }
    __syncthreads(); /* (the sums are read before the next chunk's are written) */
  }
  const unsigned long long anyBad = waveBallot(bad);
  if (lane == 0) {
    L.bad[wv] = anyBad != 0ull;
  }
  __syncthreads();
  if (tid == 0) {
    int nb = 0;
    for (int k = 0; k < kWaves; ++k) {
      nb |= L.bad[k];
    }
    Q.tokOff[Q.nRows] = carryT;
    Q.wordOff[Q.nRows] = carryW;
    Q.totals[0] = nb ? -1 : carryT;
    Q.totals[1] = carryW;
  }
}

} // namespace fltx
