/*
 * fltx_wlane_typed.h -- the front end of fltx_wlane.h on the emissions as the acoustic model produces them: fp16, bf16 or
 * float32 frames of any stride, log-probs or raw logits (fltx_decode_batch_typed).  Included after fltx_wlane.h (the
 * records, the selection's LDS) and fltx_s2s.h (the typed contract: s2sWidenF16, the lse definition).
 *
 * The emission of token n of a frame is e[n]: the element widened exactly; for logits (float)((double)x_n - lse), lse =
 * max + log(sum of the f32 exp(x - max), added in double) over the frame's non-NaN elements, lse = max when that is not
 * finite.  wtTokBeamRows writes, per frame, the WlTokRow record wlTokBeamRows writes for the float32 row e -- list in
 * token order, e, tok, eBlank, eSil, ek, nList, silPos, flags, the give-up flag included -- and wlaneUtterance runs on
 * those records unchanged.  No float32 copy of the emissions is made.
 *
 * A wave takes a frame, as in wlTokBeamRows; how the frame reaches the registers is this file's own:
 *   * 16-byte loads.  A lane reads whole aligned 16-byte blocks: eight 2-byte elements (four float32) per load, two
 *     loads (four) per chunk of 1 024 places.  A frame of a 2-byte type owes its caller 2-byte alignment only -- odd N,
 *     odd strides and odd offsets are legal -- so the blocks are counted from the block that holds token 0, not from
 *     the frame's first byte: token 0 sits at place `mis` (0 .. 7) of block 0 and place p of the frame holds token
 *     p - mis.  Places before token 0 and past token N - 1 read as -inf (never a candidate, nothing in the sum); a
 *     block without a token is not loaded, so every byte read shares an aligned 16-byte block with a byte of the frame.
 *   * read once.  A lane keeps its sixteen widened values of a chunk (kWlRowRegs) in registers through all passes: a
 *     frame of N + mis <= 1 024 places is read from HBM once -- an aligned frame of 1 024 tokens, any frame up to
 *     1 017 --, wider ones chunk by chunk in every pass.
 *   * passes.  Logits: the maximum over the raw values, then every lane adds the exp of ITS places in place order in
 *     double and a fixed butterfly adds the lanes, so the bits of lse are the same run to run; the registers then turn
 *     into e in place.  The selection is wlTokBeamRow's on e: the maximum, the counting passes over the window of
 *     float bits, the pairwise ranking of the boundary bin (ties to the lower token) into the bitmap over the row.
 *   * list.  A lane's places are consecutive tokens, so the list in token order is lane-major: per load, a lane
 *     counts its winners, one scan over the wave gives it its first position, and it writes its winners in place order
 *     (wlTokBeamRow, whose lane l holds tokens l, l + 64, ..., takes a ballot per register instead).
 * wtWidenRows writes the float32 rows e of the utterances no typed reader serves -- another engine than fltx_wlane.h, or
 * an utterance of it that is decoded again on the general engines -- with the same loads and the same lse.
 */
#pragma once

namespace fltx {

struct WtParams {
  DecodeParams p;          /* geometry, uttMap, stepT, histOff, tokRows as wlTokBeamRows reads them; p.emissions / p.emOff are not read */
  const void* x;           /* frame t of utterance b starts at x + (emOff[b] + t * stride) ELEMENTS */
  const int64_t* emOff;    /* [B] */
  const int64_t* frameOff; /* [B] frames of the call before utterance b: where its lse entries start */
  int64_t stride;
  double* lse;             /* [frames of the call] the decoder's own: each frame's lse (logits) */
  double* lseOut;          /* the caller's frame_lse, or null */
  float* wide;             /* wtWidenRows: utterance b's float32 rows e at wide + wideOff[b], N apart */
  const int64_t* wideOff;  /* [B] */
  int32_t rowBlocks;       /* workgroups per utterance (four frames each) */
  int32_t haveLse;         /* wtWidenRows: `lse` holds these frames' lse already (the front end ran on them) */
};

/* a frame as a wave reads it */
template <int DT>
struct WtRow {
  static constexpr int ES = DT == kS2sDtF32 ? 4 : 2;  /* bytes of an element */
  static constexpr int EPL = 16 / ES;                 /* elements of a 16-byte block */
  static constexpr int LPC = kWlRowRegs / EPL;        /* blocks a lane loads per chunk */
  static constexpr int CH = 64 * kWlRowRegs;          /* places of a chunk */
  const uint4* blk0; /* the aligned block that holds token 0 */
  int mis;           /* ... at this place */
  int N;
};
template <int DT>
FLTX_DEV WtRow<DT> wtRowOf(const void* frame, int N) {
  const uintptr_t a = (uintptr_t)frame;
  WtRow<DT> r;
  r.blk0 = (const uint4*)(a & ~(uintptr_t)15);
  r.mis = (int)((a & 15u) / WtRow<DT>::ES);
  r.N = N;
  return r;
}
template <int DT>
FLTX_DEV int wtChunks(const WtRow<DT>& r) {
  return (r.N + r.mis + WtRow<DT>::CH - 1) / WtRow<DT>::CH;
}
/* the token at register k of chunk c in this lane (< 0 or >= N: no token) */
template <int DT>
FLTX_DEV int wtTokOf(const WtRow<DT>& r, int c, int k) {
  constexpr int EPL = WtRow<DT>::EPL;
  return c * WtRow<DT>::CH + (k / EPL) * (64 * EPL) + laneId() * EPL + (k % EPL) - r.mis;
}
/* this lane's sixteen places of chunk c, widened */
template <int DT>
FLTX_DEV void wtLoad(const WtRow<DT>& r, int c, float (&v)[kWlRowRegs]) {
  constexpr int EPL = WtRow<DT>::EPL;
  const float NEGF = -__builtin_huge_valf();
#pragma unroll
  for (int h = 0; h < WtRow<DT>::LPC; ++h) {
    const int b = c * (WtRow<DT>::CH / EPL) + h * 64 + laneId();
    const int t0 = b * EPL - r.mis;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (t0 + EPL > 0 && t0 < r.N) { /* (a block with a token of the frame in it) */
      w = r.blk0[b];
    }
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      float x;
      if constexpr (DT == kS2sDtF32) {
        x = __uint_as_float(ww[j]);
      } else {
        const uint32_t hbits = (j & 1) ? ww[j >> 1] >> 16 : ww[j >> 1] & 0xFFFFu;
        x = DT == kS2sDtF16 ? s2sWidenF16(hbits) : __uint_as_float(hbits << 16);
      }
      const int tok = t0 + j;
      v[h * EPL + j] = (tok >= 0 && tok < r.N) ? x : NEGF;
    }
  }
}

/* lse of the frame over its raw values (every lane returns it).  chunk(c) leaves the raw places of chunk c in v */
template <typename Chunk>
FLTX_DEV double wtRowLse(int nChunk, float (&v)[kWlRowRegs], Chunk&& chunk) {
  uint32_t mk = 0u;
  for (int c = 0; c < nChunk; ++c) {
    chunk(c);
#pragma unroll
    for (int k = 0; k < kWlRowRegs; ++k) {
      const uint32_t key = s2sRawKey(v[k]);
      mk = key > mk ? key : mk;
    }
  }
  mk = waveMax32(mk);
  const float mx = mk != 0u ? f32FromKey(mk) : -__builtin_huge_valf();
  double lse = (double)mx;
  if (mx - mx == 0.0f) { /* finite */
    double s = 0.0;
    for (int c = 0; c < nChunk; ++c) {
      chunk(c);
#pragma unroll
      for (int k = 0; k < kWlRowRegs; ++k) {
        if (v[k] == v[k]) {
          s += (double)expf(v[k] - mx); /* (a place without a token: exp(-inf) = +0) */
        }
      }
    }
    for (int d = 32; d >= 1; d >>= 1) { /* (a fixed butterfly: the same sum in every lane, run to run) */
      s += __longlong_as_double((long long)waveShflXor64((unsigned long long)__double_as_longlong(s), d));
    }
    lse = (double)mx + log(s);
  }
  return lse;
}

/* where frame t of utterance b starts */
template <int DT>
FLTX_DEV const void* wtFrame(const WtParams& Z, int b, int t) {
  return (const char*)Z.x + (Z.emOff[b] + (int64_t)t * Z.stride) * WtRow<DT>::ES;
}

/* The token beam of one typed frame: wlTokBeamRow on the row e, one wave. */
template <int DT, bool LOGITS>
FLTX_DEV void wtTokBeamRow(const WtParams& Z, WlFrontLds& S, const void* frame, int64_t lseAt, WlTokRow* out, bool ctc) {
  const DecodeParams& P = Z.p;
  const int lane = laneId();
  const int N = P.N, Kt = P.Kt < 64 ? P.Kt : 64;
  typedef WtRow<DT> Row;
  const Row row = wtRowOf<DT>(frame, N);
  const int nChunk = wtChunks(row);
  const float NEGF = -__builtin_huge_valf();
  float v[kWlRowRegs];
  int lastChunk = -1;
  bool toE = false; /* logits: lse is known, the registers hold e */
  double lse = 0.0;
  auto chunk = [&](int c) { /* -> v: this lane's sixteen places of chunk c (a frame of one chunk: read once) */
    if (c != lastChunk) {
      lastChunk = c;
      wtLoad(row, c, v);
      if (LOGITS && toE) {
#pragma unroll
        for (int k = 0; k < kWlRowRegs; ++k) {
          const int tok = wtTokOf(row, c, k);
          v[k] = (tok >= 0 && tok < N) ? (float)((double)v[k] - lse) : NEGF;
        }
      }
    }
  };
  if constexpr (LOGITS) {
    lse = wtRowLse(nChunk, v, chunk);
    if (lane == 0) {
      Z.lse[lseAt] = lse;
      if (Z.lseOut) {
        Z.lseOut[lseAt] = lse;
      }
    }
    toE = true;
    if (nChunk == 1) { /* (the registers hold the raw frame: turned into e in place) */
#pragma unroll
      for (int k = 0; k < kWlRowRegs; ++k) {
        const int tok = wtTokOf(row, 0, k);
        v[k] = (tok >= 0 && tok < N) ? (float)((double)v[k] - lse) : NEGF;
      }
    } else {
      lastChunk = -1;
    }
  }
  /* pass A: the row's largest value */
  bool anyNan = false;
  float mx = NEGF;
  for (int c = 0; c < nChunk; ++c) {
    chunk(c);
#pragma unroll
    for (int k = 0; k < kWlRowRegs; ++k) {
      anyNan = anyNan || !(v[k] == v[k]);
      mx = v[k] > mx ? v[k] : mx;
    }
  }
  const uint32_t mxKey = waveMax32((mx == mx && mx > NEGF) ? f32Key(mx) : 0u);
  const bool rowBad = waveBallot(anyNan) != 0ull || mxKey == 0u;
  const float rowMax = mxKey != 0u ? f32FromKey(mxKey) : 0.0f;
  auto binOf = [&](float x, int shift, int base) -> int { /* -inf (and NaN): not a candidate */
    const float d = rowMax - x;
    if (!(d == d) || !(x > NEGF)) {
      return kSlInvalid;
    }
    int qn = (int)(__float_as_uint(d > 0.0f ? d : 0.0f) >> shift) - base;
    qn = qn < 0 ? 0 : qn;
    return qn > kSlNB - 1 ? kSlNB - 1 : qn;
  };
  /* pass B: counts per bin and the bin of the Kt-th largest (wlTokBeamRow's, on this file's places) */
  int shift = kSlCoarseShift, base = kSlCoarseBase;
  int lim = -1, need = 0, nBnd = 0, bstar = -1;
  unsigned long long bLo = 0ull, bHi = 0x7FFFFFFFull;
  bool giveUp = rowBad;
  SlScan sc = {};
  while (!giveUp) {
    ((uint4*)S.fhist)[lane] = make_uint4(0u, 0u, 0u, 0u);
    waveSync();
    int nNear = 0, nFarV = 0;
    for (int c = 0; c < nChunk; ++c) {
      chunk(c);
#pragma unroll
      for (int k = 0; k < kWlRowRegs; ++k) {
        const int b = binOf(v[k], shift, base);
        nNear += b == 0 ? 1 : 0;
        nFarV += b == kSlNB - 1 ? 1 : 0;
        if (b > 0 && b < kSlNB - 1) {
          atomAdd32(&S.fhist[b], 1u);
        }
      }
    }
    nNear = (int)waveReadLane32((uint32_t)waveInclusiveScan(nNear), 63);
    nFarV = (int)waveReadLane32((uint32_t)waveInclusiveScan(nFarV), 63);
    if (lane == 0) {
      S.fhist[0] = (uint32_t)nNear;
      S.fhist[kSlNB - 1] = (uint32_t)nFarV;
    }
    waveSync();
    sc = slScan(S.fhist, Kt, false);
    if (sc.total <= Kt) { /* fewer values than the token beam takes: all of them */
      lim = kSlNB - 1;
      break;
    }
    need = Kt - sc.cum;
    if (sc.cnt == need) {
      lim = sc.bstar;
      break;
    }
    if (sc.cnt <= kWlPairwise || (bLo >= bHi && sc.cnt <= kSlBCap)) { /* the members of the boundary bin: the larger values, ties to the lower token */
      bstar = sc.bstar;
      lim = sc.bstar - 1;
      nBnd = sc.cnt;
      if (lane == 0) {
        S.fScal[0] = 0u;
      }
      for (int i = lane; i < (N + 63) / 64; i += 64) { /* (the winners' bitmap: a bit per token) */
        S.fSel[i] = 0ull;
      }
      waveSync();
      for (int c = 0; c < nChunk; ++c) {
        chunk(c);
#pragma unroll
        for (int k = 0; k < kWlRowRegs; ++k) {
          if (binOf(v[k], shift, base) == bstar) { /* (a place without a token holds -inf: no bin) */
            const uint32_t tok = (uint32_t)wtTokOf(row, c, k);
            const uint32_t i = atomAdd32(&S.fScal[0], 1u);
            if (i < (uint32_t)kSlBCap) {
              S.fKey[i] = ((unsigned long long)f32Key(v[k] + 0.0f) << 32) | (unsigned long long)(~tok);
            }
          }
        }
      }
      waveSync();
      for (int m0 = 0; m0 < nBnd; m0 += 64) { /* member m0 + lane: its rank among the members */
        const int m = m0 + lane;
        const unsigned long long mine = S.fKey[m < nBnd ? m : 0];
        int rank = 0;
#pragma unroll 4
        for (int i = 0; i < nBnd; ++i) {
          rank += S.fKey[i] > mine ? 1 : 0;
        }
        if (m < nBnd && rank < need) {
          const uint32_t tok = ~(uint32_t)mine;
          atomOr64(&S.fSel[(tok >> 6) & (uint32_t)(kWlMaxN / 64 - 1)], 1ull << (tok & 63u));
        }
      }
      waveSync();
      break;
    }
    { /* too many in one bin: the finest window that spans its bracket */
      const unsigned long long vv = (unsigned long long)(sc.bstar + base);
      if (sc.bstar > 0 || base == 0) {
        const unsigned long long l2 = vv << shift;
        bLo = l2 > bLo ? l2 : bLo;
      }
      if (sc.bstar < kSlNB - 1) {
        const unsigned long long h2 = ((vv + 1ull) << shift) - 1ull;
        bHi = h2 < bHi ? h2 : bHi;
      }
      if (bLo >= bHi && shift == 0) { /* one value of the distance, and many of it: ranked pairwise next, or given up */
        if (sc.cnt > kSlBCap) {
          giveUp = true;
          break;
        }
        continue;
      }
      int ns = 0; /* (the bracket takes bins 1 .. 254, as in wlTokBeamRow) */
      while ((bHi >> ns) > (bLo >> ns) + (unsigned long long)(kSlNB - 3)) {
        ++ns;
      }
      shift = ns;
      base = (int)(bLo >> ns) - 1;
    }
  }
  /* pass C: the list, in token order -- lane-major within a load */
  int nList = 0;
  float eBlankF = __builtin_nanf(""), eSilF = 0.0f;
  int silPos = -4096;
  bool silSel = false; /* sil is in the token beam (listed, unless it is the blank) */
  uint32_t ek = 0u;
  for (int c = 0; c < nChunk && !giveUp; ++c) {
    chunk(c);
#pragma unroll
    for (int h = 0; h < Row::LPC; ++h) {
      uint32_t selBits = 0u, listBits = 0u;
#pragma unroll
      for (int j = 0; j < Row::EPL; ++j) {
        const int k = h * Row::EPL + j;
        const int tok = wtTokOf(row, c, k);
        bool sel = binOf(v[k], shift, base) <= lim;
        if (nBnd > 0 && tok >= 0 && tok < N) {
          sel = sel || ((S.fSel[tok >> 6] >> (tok & 63)) & 1ull) != 0ull;
        }
        selBits |= sel ? 1u << j : 0u;
        listBits |= (sel && !(ctc && tok == P.blank)) ? 1u << j : 0u;
      }
      if (waveBallot(selBits != 0u) == 0ull) {
        continue;
      }
      const int mine = __builtin_popcount(listBits);
      const int upTo = waveInclusiveScan(mine);
      int pos = nList + upTo - mine;
#pragma unroll
      for (int j = 0; j < Row::EPL; ++j) {
        if ((selBits >> j) & 1u) {
          const int k = h * Row::EPL + j;
          const int tok = wtTokOf(row, c, k);
          const float x = v[k];
          if (!((listBits >> j) & 1u)) {
            eBlankF = x;
          }
          if (tok != P.sil) {
            const uint32_t kk = f32Key(x);
            ek = kk > ek ? kk : ek;
          } else {
            eSilF = x;
            silSel = true;
          }
          if (((listBits >> j) & 1u) && pos < 64) {
            out->e[pos] = x;
            out->tok[pos] = (uint16_t)tok;
            if (tok == P.sil) {
              silPos = pos;
            }
            ++pos;
          }
        }
      }
      nList += (int)waveReadLane32((uint32_t)upTo, 63);
    }
  }
  /* what one lane found, to all */
  ek = waveMax32(ek);
  const unsigned long long blankAt = waveBallot(eBlankF == eBlankF);
  const unsigned long long silAt = waveBallot(silSel);
  if (blankAt != 0ull) {
    eBlankF = __uint_as_float(waveReadLane32(__float_as_uint(eBlankF), __builtin_ctzll(blankAt)));
  }
  if (silAt != 0ull) {
    const int sl = __builtin_ctzll(silAt);
    eSilF = __uint_as_float(waveReadLane32(__float_as_uint(eSilF), sl));
    silPos = (int)waveReadLane32((uint32_t)silPos, sl);
  }
  if (lane == 0) {
    out->eBlank = eBlankF;
    out->eSil = eSilF;
    out->ek = ek;
    out->nList = nList;
    out->silPos = silPos;
    out->flags = (silAt != 0ull ? 1u : 0u) | (giveUp ? 2u : 0u);
  }
}

/* which frame a wave of the two kernels takes: workgroup = utterance * rowBlocks + row block, four frames per block */
FLTX_DEV bool wtWaveFrame(const WtParams& Z, int& b, int& t) {
  const DecodeParams& P = Z.p;
  const int wave = waveUniform(waveId());
  const int ub = (int)blockIdx.x / Z.rowBlocks, rb = (int)blockIdx.x % Z.rowBlocks;
  b = P.uttMap ? P.uttMap[ub] : ub;
  t = rb * ((int)blockDim.x >> 6) + wave;
  return t < (P.stepT ? P.stepT[b] : 0);
}

/* the typed front-end kernel */
template <int DT, bool LOGITS>
FLTX_DEV void wtTokBeamRows(const WtParams& Z, char* smem) {
  const DecodeParams& P = Z.p;
  int b, t;
  if (!wtWaveFrame(Z, b, t)) {
    return;
  }
  WlFrontLds& S = ((WlFrontLds*)smem)[waveUniform(waveId())];
  WlTokRow* out = (WlTokRow*)P.tokRows + (P.histOff[b] / P.K + t);
  wtTokBeamRow<DT, LOGITS>(Z, S, wtFrame<DT>(Z, b, t), Z.frameOff[b] + t, out, P.criterion == 1);
}

/* the float32 rows e of the utterances the launch names, for the engines that read float32 */
template <int DT, bool LOGITS>
FLTX_DEV void wtWidenRows(const WtParams& Z, char*) {
  const DecodeParams& P = Z.p;
  int b, t;
  if (!wtWaveFrame(Z, b, t)) {
    return;
  }
  const int N = P.N;
  typedef WtRow<DT> Row;
  const Row row = wtRowOf<DT>(wtFrame<DT>(Z, b, t), N);
  const int nChunk = wtChunks(row);
  const int64_t lseAt = Z.frameOff[b] + t;
  float v[kWlRowRegs];
  int lastChunk = -1;
  auto chunk = [&](int c) {
    if (c != lastChunk) {
      lastChunk = c;
      wtLoad(row, c, v);
    }
  };
  double lse = 0.0;
  if constexpr (LOGITS) {
    if (Z.haveLse) {
      lse = Z.lse[lseAt];
    } else {
      lse = wtRowLse(nChunk, v, chunk);
      if (laneId() == 0) {
        Z.lse[lseAt] = lse;
        if (Z.lseOut) {
          Z.lseOut[lseAt] = lse;
        }
      }
    }
  }
  float* dst = Z.wide + Z.wideOff[b] + (int64_t)t * N;
  for (int c = 0; c < nChunk; ++c) {
    chunk(c);
#pragma unroll
    for (int k = 0; k < kWlRowRegs; ++k) {
      const int tok = wtTokOf(row, c, k);
      if (tok >= 0 && tok < N) {
        dst[tok] = LOGITS ? (float)((double)v[k] - lse) : v[k];
      }
    }
  }
}

} // namespace fltx
