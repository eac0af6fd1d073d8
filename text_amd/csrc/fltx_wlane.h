/*
 * fltx_wlane.h -- "lane = LM state" decode of a whole utterance for LARGE token sets (word pieces: 65 .. 16 384
 * tokens) with a token beam of at most 64: LexiconFreeDecoder + ZeroLM, max-merge, beam <= 64, offline.  Included
 * by fltx_kernels.h after fltx_slane.h, whose lane formulation, selection and history records it keeps (read the
 * head of that file first).  Same candidates, same merge groups, same selection as
 * LexiconFreeDecoder::decodeStep (LexiconFreeDecoder.cpp:30-125) with candidatesStore (Utils.h:146-225):
 * bit-identical n-best.
 *
 * What differs from fltx_slane.h, whose per-lane masks have one bit per TOKEN (<= 64 tokens):
 *   * the token beam (LexiconFreeDecoder.cpp:42-51: the beamSizeToken largest emissions of the row) is what the
 *     frame works with, and everything token-shaped is keyed by the POSITION of a token in the frame's list of
 *     at most 64: a lane's record carries its last token's position in the list of the frame that reads the
 *     record (0xFF: not in that frame's token beam -- the state can be neither repeated nor extended by it) next
 *     to the token itself; cmask[lane] has a bit per list position; the token waves' skip test is a bit test
 *     with their own position numbers.  The staging wave keeps a token -> position table (posOf, one byte per
 *     token) of the newest list, which the build step reads for the records it writes;
 *   * the token beams are found before the decode kernel starts, by a kernel of their own (fltx_tokbeam_kernel: one
 *     wave per row of N emissions, all rows of the batch in parallel): the histogram selection the frames use (a
 *     window over the float bits of the distance to the row's largest, the members of the one boundary bin ranked
 *     pairwise, ties to the lower token), the list written in token order, one 416-byte record per row; the staging
 *     wave of the decode kernel takes a record per frame, a frame ahead;
 *   * "this (LM state, token) edge had a child before" (LMState::child's memo, lm/LM.h:24-34) is a Bloom filter
 *     over (state id, token) in LDS -- two bits per edge in 512 Kbit -- instead of a 64-bit mask per lane: a
 *     hit, true or false, makes the next frame look the edge up -- first in an exact direct-mapped memo of the newest
 *     4 096 edges in LDS, then in the history rows (slReenter's scan, which finds the new record itself when the hit
 *     was false) --, so the filter only has to be free of false negatives.
 *
 * TL (wlaneUtterance<GT, false, true>, opt-in through "wtlane"): the same with a token n-gram LM over the word pieces,
 * see the comment at WtLds below; one more barrier per frame (the frame's best is a reduction).
 * ST + TL (wlaneUtterance<GT, true, true>, opt-in through "wtstream"): a stream's chunks with that LM, see WtStreamLds.
 * LA (wlaneUtterance<GT, false, TL, true>, opt-in through "wlogadd"): the members of a merge group are log-added
 * (DecoderOptions::logAdd), see the comment at WlaLds below; offline only.
 *
 * Roles and barriers as in fltx_slane.h: token waves (GT list positions each), one wave for the lanes' own groups
 * (blank, repeat + the parent state's extension, blank-then-last), the staging wave; three barriers per frame.
 */
#pragma once

constexpr int kWlMaxN = 16384;        /* tokens the position table covers */
constexpr int kWlBloomWords = 16384;  /* 64 KB = 2^19 bits */
constexpr int kWlRowRegs = 16;        /* row values a lane of the front end holds: one chunk of 1 024 tokens */
constexpr uint32_t kWlNoPos = 0xFFu;
constexpr int kWlEdgeSlots = 4096;    /* direct-mapped memo of the newest (state id, token) -> child state id edges, 32 KB */
constexpr uint32_t kWlNoSid = 0xFFFFFFFFu;

struct WlRow { /* what a frame needs to know about its emission row */
  double best;    /* the frame's best candidate (Utils.h:131-137) */
  double thr;     /* best - beamThreshold */
  double eBlank;  /* blank's emission, NaN when blank is not in the token beam (or the criterion has none) */
  int32_t nList;  /* tokens the token waves evaluate (in the token beam, not blank) */
  int32_t silPos; /* list position of sil, or a value no wave matches */
  uint32_t dead;  /* no candidate at all / not finite: the utterance goes to the general engines */
  uint32_t nev;   /* re-entry events recorded by the build of the previous frame */
};

struct WlaneLds {
  SlRec rec[2][64];                /* info: position of the last token in the reading frame's list | (parent lane + 1) << 8 |
                                      history slot of nb << 16 | of b << 24; pad: the last token */
  unsigned long long cmask[2][64]; /* list positions whose child state is in the beam and linked to this lane */
  uint32_t hist[2][kSlNB];
  double eTok[2][64];              /* emission of the listed tokens by list position, NaN past the list */
  uint32_t tokTok[2][64];          /* list position -> token */
  WlRow row[2];
  uint32_t off[32];
  int32_t newLane[64];
  uint32_t scal[16];
  unsigned long long bKey[kSlBCap];
  uint32_t bOrd[kSlBCap];
  uint32_t evLane[64], evSpar[64], evTok[64];
  uint32_t evSid[64];              /* the state's id when the edge memo still had it (no look-up in the history rows), else kWlNoSid */
  uint32_t scanMin, pad0;
  unsigned long long edge[kWlEdgeSlots]; /* bit 63 | parent id:23 << 37 | token:14 << 23 | child id:23 */
  uint32_t bloom[kWlBloomWords];
  uint8_t posOf[kWlMaxN];          /* token -> position in the newest list (the frame after the current one), 0xFF = not listed */
};
/* Stream chunks (wlaneUtterance<GT, true>): LM states are named through the generic engine's (epoch, parent id, token)
 * -> id table in HBM (tlStreamChild), which is exact and says whether an edge had a child before -- no Bloom filter, no
 * edge memo, no look-up in the history rows.  In their place: the emitting-model score of a lane's two hypotheses
 * (getBestHypothesis reports an ancestor's) and the parked slots the restore found them in.  31 KB against 124 KB.
 * The members both kernels use are WlaneLds's, by the same names (a struct of its own, not a shared base: the offline
 * kernel's accesses keep the types, and so the code, they had). */
struct WlStreamLds {
  SlRec rec[2][64];
  unsigned long long cmask[2][64];
  uint32_t hist[2][kSlNB];
  double eTok[2][64];
  uint32_t tokTok[2][64];
  WlRow row[2];
  uint32_t off[32];
  int32_t newLane[64];
  uint32_t scal[16];
  unsigned long long bKey[kSlBCap];
  uint32_t bOrd[kSlBCap];
  uint32_t evLane[64], evSpar[64], evTok[64];
  uint32_t evSid[64];              /* always the state's id */
  alignas(16) double amNB[2][64];  /* emitting-model score of a lane's two hypotheses */
  double amB[2][64];
  uint8_t rsNB[64], rsB[64];       /* restore: the parked slot of a lane's two hypotheses */
  uint8_t posOf[kWlMaxN];          /* (16-byte aligned: the prologue wipes it four words at a time) */
};
/* What only a stream's frame computes: empty offline, and touched under `if constexpr (ST)` alone, so that the offline
 * kernel's frame is the code it was (locals and lambdas both variants declared moved its registers and spills). */
template <bool ST>
struct WlStreamRegs {};
template <>
struct WlStreamRegs<true> {
  int frame0, total0;                  /* rows already in the buffer; frames decoded since decodeBegin */
  double amNB, amB, parAmNB, parAmB;   /* emitting-model score of the lane's two hypotheses, of its parent lane's */
  double amM;                          /* ... of the better of the lane's two */
  double amR;                          /* ... of the repeat group's winning member */
  uint32_t prevR;                      /* ... and that member's token (ASG transition) */
  double amNew;                        /* ... of the state newState() is about to make */
  uint32_t bit, fresh;                 /* ST + TL: the candidate slot newState() is called for; slots whose state's id is new */
};
enum { WL_FRAME0 = 6, WL_TOTAL0 = 7 }; /* scal[], next to fltx_slane.h's SL_* */

/* ---- TL: a token n-gram LM over the word pieces (wlaneUtterance<GT, false, true>) -------------------------------------
 * fltx_slane.h's TL pattern (read the head comment there: an LM term per new-token candidate, the frame's best a
 * reduction behind one more barrier, decodeEnd adds lmWeight x finish, the LM score of every path is returned) without
 * its dense (context, token) table, which N > 64 has no room for.  A look-up is ngScore(context, usrToLm[token]), a
 * chain of dependent probes of ~4 k clocks; what keeps them few:
 *   filter   the candidates without a new LM term (a lane's blank and its own repeat) are priced by every wave from the
 *            records it holds anyway; their maximum bounds the frame's best from below.  A (lane, position) pair whose
 *            score with the LM's extreme term (DecodeParams::wtLmMax / wtLmMin, by lmWeight's sign) stays under that
 *            bound - beamThreshold cannot pass the frame's threshold and asks nothing: rounding is monotone, so the
 *            drop is exact;
 *   memo     lmMemo: (state id, token) -> score, direct-mapped in LDS, slot and tag together hold the whole key (lmCache's
 *            layout, fltx_kernels.h): a hit is exact.  One 64-bit word per entry, written and read whole by waves that
 *            nothing orders: the exactness rests on the compiler emitting one 64-bit LDS operation per access (an
 *            aligned unsigned long long; lmCache and `edge` assume the same of their 64-bit words);
 *   drain    the misses of a wave are asked a lane at a time, every lane's next miss side by side (ngScoreT issues all
 *            context lengths of a query at once);
 *   context  a state's n-gram context (order - 1 suffix node ids) lives with its lane (ctx, double-buffered like rec): a
 *            new state's is the ctxOut of the edge that entered it, asked for the survivors only, in the build;
 *   lmIn     the LM score a state was entered with: the parent state's extension by last(S) joins S's repeat group with
 *            exactly that term;
 *   lmNB/lmB the LM score of a lane's two hypotheses, carried like a stream's emitting-model score (the winner of a
 *            max-merge hands on its own): the back-trace has nothing to re-walk. */
constexpr int kWtMemoSlots = 2048; /* 16 KB: with the members below 145 KB of the CU's 160 */
constexpr int kWtCtx = kMaxNgramOrder - 1;
struct WtLds : WlaneLds {
  unsigned long long fbest[2];     /* order key of the frame's best candidate, 0 = none yet */
  double lmNB[2][64], lmB[2][64];
  float lmIn[2][64];
  int32_t ctx[2][kWtCtx][64];
  uint32_t stat[4];                /* profile: pairs, pairs the filter dropped, look-ups, memo hits */
  unsigned long long lmMemo[kWtMemoSlots]; /* tag (state id << 3 | token >> 11) << 32 | float bits of the score */
};
static_assert(sizeof(WtLds) <= 160 * 1024, "one CU's LDS");
template <bool TL, int GT>
struct WlTokLmRegs {};
template <int GT>
struct WlTokLmRegs<true, GT> {
  int32_t ctx[kWtCtx];   /* the lane's context */
  double thrLB;          /* lower bound of the frame's threshold */
  float lmv[GT];         /* LM score of the lane's candidates (self wave: [2] = blank-then-last) */
  bool pre[GT];          /* ... which are candidates at all */
  float lIn;             /* self wave: the score the state was entered with */
  double lmNB, lmB, parLmNB, parLmB; /* LM score of the lane's two hypotheses, of its parent lane's */
  double lmR;            /* ... of the repeat group's winning member */
  float lmE;             /* the state newState() is about to make: the score it is entered with ... */
  double lmNew;          /* ... and its hypothesis's LM score */
};
/* ... and what the utterance keeps across its frames */
template <bool TL>
struct WlTokLmUtt {};
template <>
struct WlTokLmUtt<true> {
  double lmW;      /* lmWeight */
  double wU;       /* lmWeight x the LM's extreme score on the side its sign makes the upper one (the filter's bound) */
  bool prof;       /* the phase clocks are on: count */
  uint32_t cnt[4]; /* ... this lane's pairs, pairs the filter dropped, look-ups, memo hits */
};
FLTX_DEV uint32_t wtMemoSlot(uint32_t sid, uint32_t tok) { return (tok ^ sid ^ (sid >> 11)) & (uint32_t)(kWtMemoSlots - 1); }
FLTX_DEV uint32_t wtMemoTag(uint32_t sid, uint32_t tok) { return (sid << 3) | (tok >> 11); }
/* ---- ST + TL: a stream's chunks with the token n-gram LM (wlaneUtterance<GT, true, true>, opt-in through "wtstream") ----
 * WlStreamLds's members and the TL members of WtLds by the same names, so the frame's TL code is the offline variant's.
 * The stream layout leaves room the offline one does not have (32 KB against 124 KB), and nine waves of 168 VGPRs keep a
 * second workgroup off the CU whatever the LDS, so the score memo's slot count is a constant of this variant
 * (kWtsMemoBits).  Measured at 2 048 and 8 192 slots: the same 1.2 % of the look-ups answered and rates
 * whose ranges overlap -- on those rows a pair is rarely asked twice, whatever the memo holds -- so it stays at 2 048
 * (16 KB; 54 KB in all, within the default launch limit).  Slot and tag hold the whole (state id, token) key as offline:
 * tag = id << (14 - bits) | token >> bits, the slot gives the token's low bits back.  Ids are the generic table's (below
 * 2^23: prepare() refuses what would not fit kWtsMaxSid); compactions renumber them between chunks, so the memo lives for
 * one launch and starts empty in each.
 * Restore: a lane's LM scores are its two slots' gLm, its context the id's stateCtx row (order - 1 suffix node ids: no dense
 * table at N > 64), the term it was entered with one wtNgram(stateCtx row of its parent id, its last token) -- for every
 * lane that takes arrivals, linked to its parent's lane or not: wlRelink may link it later in the chunk.
 * A state whose id is new gets its context written to stateCtx (the generic engine's begin / end / prune / redo read it). */
constexpr int kWtsMemoBits = 11;
constexpr int kWtsMemoSlots = 1 << kWtsMemoBits;
constexpr uint32_t kWtsMaxSid = (1u << (18 + kWtsMemoBits < 31 ? 18 + kWtsMemoBits : 31)) - 2u; /* (no id reaches the empty slot's tag) */
static_assert(kWtsMemoBits <= 14 && kWlMaxN <= (1 << 14), "tag = id << (14 - bits) | token >> bits");
struct WtStreamLds : WlStreamLds {
  unsigned long long fbest[2];
  double lmNB[2][64], lmB[2][64];
  float lmIn[2][64];
  int32_t ctx[2][kWtCtx][64];
  uint32_t stat[4];
  unsigned long long lmMemo[kWtsMemoSlots]; /* tag (state id << (14 - bits) | token >> bits) << 32 | float bits of the score */
};
static_assert(sizeof(WtStreamLds) <= 64 * 1024, "launched within the default limit, as every kWstream kernel");
template <bool ST>
FLTX_DEV uint32_t wtSlotOf(uint32_t sid, uint32_t tok) {
  if constexpr (ST) {
    return (tok ^ sid ^ (sid >> kWtsMemoBits)) & (uint32_t)(kWtsMemoSlots - 1);
  } else {
    return wtMemoSlot(sid, tok);
  }
}
template <bool ST>
FLTX_DEV uint32_t wtTagOf(uint32_t sid, uint32_t tok) {
  if constexpr (ST) {
    return (sid << (14 - kWtsMemoBits)) | (tok >> kWtsMemoBits);
  } else {
    return wtMemoTag(sid, tok);
  }
}
/* ---- LA: logAdd merges (wlaneUtterance<GT, false, TL, true>, opt-in through "wlogadd") -------------------------------
 * fltx_slane.h's LA pattern, keyed by list position.  The merge groups keep their fixed shape; the members that pass the
 * frame's threshold are log-added in descending order (Utils.h:167-198), the back-pointer -- and with it the
 * emitting-model score, the LM score and the n-gram context -- stays the best member's:
 *   token waves   a new-token candidate's second member is the state's other hypothesis + the same emission (+ silScore,
 *                 + the same LM term): fl(a + e) is monotone, so it is the smaller one;
 *   own groups    blank: nb and b; repeat: the lane's own repeat and the parent state's two extensions by last(S), sorted
 *                 (three members); blank-then-last has one member;
 *   decodeEnd     a state's two hypotheses finish into one.
 * Without a token LM the frame's best candidate is no recurrence any more (a merged hypothesis can score above every
 * candidate of its frame): the build raises mmaxKey to the best surviving score, and every wave prices the row at the head
 * of the next frame as that + the row's largest listed emission, sil apart (silScore) -- eMax / eSil, which the staging
 * wave leaves next to the row; WlRow::best / thr are not read, WlRow::dead says only whether the token beam could be cut.
 * With a token LM the best is the reduction behind barrier 0 as it was (second members are never above first ones), the
 * merges follow that barrier, and WtLds is the layout unchanged.
 * sizeof(WlaLds) = sizeof(WlaneLds) + 48 = 126 536 bytes; TL + LA: WtLds, 148 024 bytes. */
struct WlaLds : WlaneLds {
  unsigned long long mmaxKey[2]; /* order key of the best hypothesis of the beam a frame starts from */
  double eMax[2];                /* the row's largest listed emission other than sil's (blank's included), NaN: none */
  double eSil[2];                /* sil's emission, NaN: sil is not in the token beam */
};
static_assert(sizeof(WlaLds) == 126536 && sizeof(WlaLds) < sizeof(WtLds), "one CU's LDS; the size the comment states");
/* what a logAdd frame keeps of a lane's groups until the frame's threshold is known (TL: across barrier 0); empty
 * otherwise, and touched under `if constexpr (LA)` alone */
template <bool LA, int GT>
struct WlLogAddRegs {};
template <int GT>
struct WlLogAddRegs<true, GT> {
  double c2[GT];     /* second member of the group of slot j */
  uint32_t two;      /* slots that have one */
  double r0, r1, r2; /* own-groups wave: the repeat group's members ... */
  uint32_t has;      /* ... which of them exist (bits 0 .. 2) */
};
/* the repeat group under logAdd: the members that exist and pass the threshold, added best first; false: none passes */
FLTX_DEV bool wlRepeatLogAdd(double r0, double r1, double r2, uint32_t has, double thr, double& sum) {
  const double NEG = slNegInf();
  const bool v0 = (has & 1u) && r0 >= thr, v1 = (has & 2u) && r1 >= thr, v2 = (has & 4u) && r2 >= thr;
  const double a = v0 ? r0 : NEG, bq = v1 ? r1 : NEG, cq = v2 ? r2 : NEG;
  const double t0 = a > bq ? a : bq, t1 = a > bq ? bq : a; /* three-element sort, descending */
  const double hi = t0 > cq ? t0 : cq;
  const double mid = t0 > cq ? (t1 > cq ? t1 : cq) : t0;
  const double lo = t0 > cq ? (t1 > cq ? cq : t1) : t1;
  double acc = hi;
  if (mid > NEG) {
    acc = slLogAdd(acc, mid);
  }
  if (lo > NEG) {
    acc = slLogAdd(acc, lo);
  }
  sum = acc;
  return v0 || v1 || v2;
}
/* what the head of a logAdd frame prices the row with, left next to the row the staging wave has just staged.  One lane. */
FLTX_DEV void wlStageLa(WlaLds& S, int q, uint32_t ek, float eSil, uint32_t flags) {
  S.eMax[q] = ek != 0u ? (double)f32FromKey(ek) : __builtin_nan("");
  S.eSil[q] = (flags & 1u) ? (double)eSil : __builtin_nan("");
  S.row[q].dead = (flags & 2u) ? 1u : 0u;
}

/* lm.score(context, token) (KenLM.cpp:63-75): tokens outside the LM's vocabulary are <unk>, as lmScoreDev */
FLTX_DEV float wtNgram(const DecodeParams& P, const int32_t* ctx, uint32_t tok, int32_t* ctxOut) {
  const uint32_t word = tok < (uint32_t)P.nUsr ? (uint32_t)P.usrToLm[tok] : (uint32_t)P.lmUnk;
  return P.lmOrder <= 3 ? ngScoreT<3>(P, ctx, word, ctxOut) : ngScoreT<kMaxNgramOrder>(P, ctx, word, ctxOut);
}
/* LexiconFreeDecoder.cpp:58-64: the ASG transition enters the emitting-model score only */
FLTX_DEV double wlAmStep(const DecodeParams& P, bool first, double amPrev, double e, uint32_t n, uint32_t prevTok) {
  double x = e;
  if (P.criterion != 1 && P.transitions && !first) {
    x = x + (double)P.transitions[(size_t)n * P.N + prevTok];
  }
  return amPrev + x;
}
/* the generic engine's plain record, and a record's {score, emitting-model score, 0.0} */
FLTX_DEV int2 wlPlainRec(uint32_t hp, uint32_t n) { return make_int2(hp == kSlNoHyp ? -1 : (int)hp, (int)n); }
FLTX_DEV void wlScoreRec(const DecodeParams& P, int64_t at, double c, double am) {
  if (P.histS) {
    double* hs = P.histS + 3 * at;
    hs[0] = c;
    hs[1] = am;
    hs[2] = 0.0;
  }
}
/* ... with a token LM: {score, emitting-model score, LM score} */
FLTX_DEV void wlScoreRecLm(const DecodeParams& P, int64_t at, double c, double am, double lm) {
  if (P.histS) {
    double* hs = P.histS + 3 * at;
    hs[0] = c;
    hs[1] = am;
    hs[2] = lm;
  }
}
/* a lane's `spar` in a stream: bit 31 (no state id has it) = the state takes no arrival -- the start state, or a state
 * whose parent a compaction has cut loose, whose number in gSPar is stale and must not be matched (fltx_xlane.h) */
constexpr uint32_t kWlNoArrival = 0x80000000u;

FLTX_DEV uint32_t wlHash(uint32_t sid, uint32_t tok, uint32_t seed) {
  uint32_t h = (sid * 0x9E3779B1u) ^ (tok * 0x85EBCA77u) ^ seed;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}
/* marks the edge (state id, token) and tells whether it may have been marked before (no false negatives) */
FLTX_DEV bool wlEdgeSeen(WlaneLds& S, uint32_t sid, uint32_t tok) {
  const uint32_t h1 = wlHash(sid, tok, 0x1234567u), h2 = wlHash(tok, sid, 0x89ABCDEu);
  const uint32_t b1 = 1u << (h1 & 31u), b2 = 1u << (h2 & 31u);
  const uint32_t o1 = atomOr32(&S.bloom[(h1 >> 5) & (kWlBloomWords - 1)], b1);
  const uint32_t o2 = atomOr32(&S.bloom[(h2 >> 5) & (kWlBloomWords - 1)], b2);
  return (o1 & b1) != 0u && (o2 & b2) != 0u;
}

FLTX_DEV unsigned long long wlEdgePack(uint32_t psid, uint32_t tok, uint32_t csid) {
  return (1ull << 63) | ((unsigned long long)(psid & 0x7FFFFFu) << 37) | ((unsigned long long)(tok & 0x3FFFu) << 23) |
         (unsigned long long)(csid & 0x7FFFFFu);
}
FLTX_DEV uint32_t wlEdgeSlot(uint32_t psid, uint32_t tok) { return wlHash(psid, tok, 0x5bd1e995u) & (uint32_t)(kWlEdgeSlots - 1); }

/* Re-entry of LM states (see slReenter): the earliest history record {new state, parent id, token} names the
 * state of a lane whose edge the filter had seen; lanes whose parent id it is get their link back.  All waves. */
FLTX_DEV __attribute__((noinline)) void wlReenter(WlaneLds& S, const int2* histPT, int q, int nState, int64_t hbase,
                                                   int64_t nRec) {
  const int tid = (int)threadIdx.x, W = (int)blockDim.x;
  const int nev = (int)S.row[q].nev;
  ldsBarrier(); /* (everybody has read the count before the first one through resets it) */
  bool settled = false; /* the history stores of the last build have reached the L2 (needed by the look-ups only) */
  for (int e = 0; e < nev; ++e) {
    const int X = (int)S.evLane[e];
    const uint32_t ps = S.evSpar[e], n = S.evTok[e];
    const uint32_t known = S.evSid[e]; /* (uniform) */
    if (known != kWlNoSid) { /* the edge memo had the state's id: the record carries it already; its orphans: */
      if (tid < nState && tid != X && S.rec[q][tid].spar == known) {
        const uint32_t info = S.rec[q][tid].info;
        S.rec[q][tid].info = (info & ~0xFF00u) | ((uint32_t)(X + 1) << 8);
        if ((info & 0xFFu) < 64u) {
          atomOr64(&S.cmask[q][X], 1ull << (info & 0xFFu));
        }
      }
      continue;
    }
    if (!settled) { /* (waiting for a wave's stores costs 2 - 4 k clocks: only when the rows are read) */
      settled = true;
#ifndef FLTX_EMU
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
      ldsBarrier();
    }
    if (tid == 0) {
      S.scanMin = 0xFFFFFFFFu;
    }
    ldsBarrier();
    const unsigned long long* h = (const unsigned long long*)(histPT + hbase);
    uint32_t found = 0xFFFFFFFFu;
    for (int64_t i0 = tid; i0 < nRec; i0 += 8 * (int64_t)W) { /* eight loads in flight (one at a time, a scan of the
                                                                   rows of a long utterance is tens of microseconds) */
      unsigned long long rr[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t i = i0 + (int64_t)u * W;
        rr[u] = i < nRec ? loadCoherent64(h + i) : 0ull;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t i = i0 + (int64_t)u * W;
        const uint32_t x = (uint32_t)rr[u], y = (uint32_t)(rr[u] >> 32);
        if (i < nRec && (x & kSlNewFlag) && y == n && (x >> 9) == ps) {
          found = found < (uint32_t)i ? found : (uint32_t)i;
        }
      }
    }
    if (found != 0xFFFFFFFFu) {
      atomMin32(&S.scanMin, found);
    }
    ldsBarrier();
    const uint32_t sid = S.scanMin;
    if (sid != 0xFFFFFFFFu && tid == 0) {
      S.edge[wlEdgeSlot(ps, n)] = wlEdgePack(ps, n, sid); /* (the memo learns the edge, again or for the first time) */
    }
    if (sid != 0xFFFFFFFFu && sid != S.rec[q][X].sid) { /* (its own record: the filter's hit was a false one) */
      ldsBarrier();
      if (tid == 0) {
        S.rec[q][X].sid = sid;
      }
      if (tid < nState && tid != X && S.rec[q][tid].spar == sid) { /* orphans get their parent back */
        const uint32_t info = S.rec[q][tid].info;
        S.rec[q][tid].info = (info & ~0xFF00u) | ((uint32_t)(X + 1) << 8);
        if ((info & 0xFFu) < 64u) {
          atomOr64(&S.cmask[q][X], 1ull << (info & 0xFFu));
        }
      }
    }
    ldsBarrier();
  }
  if (tid == 0) {
    S.row[q].nev = 0u;
  }
  ldsBarrier();
}

/* ... in a stream: every re-entered state knows its id (the table gave it), so what is left is wlReenter's "known"
 * branch -- the lanes whose parent a re-entered state is get their link back.  All waves. */
FLTX_DEV __attribute__((noinline)) void wlRelink(WlStreamLds& S, int q, int nState) {
  const int tid = (int)threadIdx.x;
  const int nev = (int)S.row[q].nev;
  ldsBarrier(); /* (everybody has read the count before it is reset) */
  if (tid < nState) {
    const uint32_t spar = S.rec[q][tid].spar; /* (kWlNoArrival set: equals no id) */
    for (int e = 0; e < nev && e < 64; ++e) {
      const int X = (int)S.evLane[e];
      if (tid != X && spar == S.evSid[e]) {
        const uint32_t info = S.rec[q][tid].info;
        S.rec[q][tid].info = (info & ~0xFF00u) | ((uint32_t)(X + 1) << 8);
        if ((info & 0xFFu) < 64u) {
          atomOr64(&S.cmask[q][X], 1ull << (info & 0xFFu));
        }
      }
    }
  }
  if (tid == 0) {
    S.row[q].nev = 0u;
  }
  ldsBarrier();
}

/* ---- front end: the token beams of all rows, a kernel of its own ------------------------------------------------ */
/* Which tokens a frame works with does not depend on the beam: the beamSizeToken largest emissions of every row of the
 * batch are found by fltx_tokbeam_kernel before the decode kernel starts -- one wave per row, all rows of all
 * utterances in parallel over the chip (inside the decode kernel the same selection was one wave's serial work per
 * frame: 15 k .. 23 k clocks against the 4 k of the frame's own) -- and left in HBM as one 416-byte record per row. */
struct WlTokRow {
  float e[64];       /* emissions of the listed tokens (in the token beam, not blank), in token order */
  uint16_t tok[64];  /* ... the tokens */
  float eBlank;      /* blank's emission, NaN when blank is not in the token beam (or the criterion has none) */
  float eSil;        /* sil's emission when it is in the token beam */
  uint32_t ek;       /* order key of the largest emission in the token beam other than sil's (blank's included), 0 = none */
  int32_t nList;
  int32_t silPos;    /* list position of sil, -4096 = not listed */
  uint32_t flags;    /* bit 0: sil is in the token beam; bit 1: the row cannot be cut (NaN, or more equal values at the
                        cut than the pairwise list holds): the utterance goes to the general engines */
  uint32_t pad[2];
};
static_assert(sizeof(WlTokRow) == 416, "one record per row");
constexpr int kWlShift = 18;    /* the counting pass after the coarse one: 32 bins per octave */
constexpr int kWlPairwise = 16; /* members of the boundary bin ranked against each other; beyond that the bin is looked at again */

struct WlFrontLds { /* per wave of the front-end kernel */
  uint32_t fhist[kSlNB];            /* counts of the row's values per bin */
  unsigned long long fKey[kSlBCap]; /* members of the boundary bin: value key << 32 | ~token */
  unsigned long long fSel[kWlMaxN / 64]; /* those of them the token beam takes: a bit per value of the row */
  uint32_t fScal[4];
};

FLTX_DEV void wlLoadChunk(const float* row, int N, int chunk, float (&v)[kWlRowRegs]) {
  const int lane = laneId();
#pragma unroll
  for (int k = 0; k < kWlRowRegs; ++k) {
    const int idx = chunk * (64 * kWlRowRegs) + k * 64 + lane;
    v[k] = idx < N ? row[idx] : -__builtin_huge_valf();
  }
}

/* The token beam of one row = its Kt largest values (LexiconFreeDecoder.cpp:42-51).  One wave.  A counting pass over
 * a window of the float bits of the distance to the row's largest (16 bins per octave, 2^-7 .. 2^9; the two ends of a
 * window would take hundreds of counts on one LDS address and are counted with ballots instead), one scan; a bin
 * with more than a handful of members is looked at again through the finest window that spans it; the members of
 * the bin that holds the Kt-th largest are then ranked against each other (value, then the lower token) by one lane
 * each, and the winners marked in a bitmap over the row.  The list is written in token order. */
FLTX_DEV void wlTokBeamRow(const DecodeParams& P, WlFrontLds& S, const float* row, WlTokRow* out, bool ctc) {
  const int lane = laneId();
  const int N = P.N, Kt = P.Kt < 64 ? P.Kt : 64;
  constexpr int CH = 64 * kWlRowRegs;
  const int nChunk = (N + CH - 1) / CH;
  const float NEGF = -__builtin_huge_valf();
  float v[kWlRowRegs];
  int lastChunk = -1;
  auto chunk = [&](int c) { /* -> v: this lane's sixteen values of chunk c (rows of up to 1 024 tokens: read once) */
    if (c != lastChunk) {
      lastChunk = c;
      wlLoadChunk(row, N, c, v);
    }
  };
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
  /* pass B: counts per bin and the bin of the Kt-th largest */
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
      for (int i = lane; i < 8 * nChunk; i += 64) { /* (the winners' bitmap: a bit per value of the row) */
        ((uint4*)S.fSel)[i] = make_uint4(0u, 0u, 0u, 0u);
      }
      waveSync();
      for (int c = 0; c < nChunk; ++c) {
        chunk(c);
#pragma unroll
        for (int k = 0; k < kWlRowRegs; ++k) {
          if (binOf(v[k], shift, base) == bstar) {
            const uint32_t tok = (uint32_t)(c * CH + k * 64 + lane);
            const uint32_t i = atomAdd32(&S.fScal[0], 1u);
            S.fKey[i] = ((unsigned long long)f32Key(v[k] + 0.0f) << 32) | (unsigned long long)(~tok);
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
          atomOr64(&S.fSel[tok >> 6], 1ull << (tok & 63u));
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
      if (bLo >= bHi && shift == 0) { /* bin bstar is one value of the distance, and many of it: the next pass ranks
                                         them pairwise, or gives up */
        if (sc.cnt > kSlBCap) {
          giveUp = true;
          break;
        }
        continue;
      }
      /* The bracket takes bins 1 .. 254; bin 0 holds what is nearer, 255 what is farther.  (With the bracket from bin 0
       * on, bin 0 also held every nearer value: a cut on a value at the bracket's lower end counted them with its own
       * ties, and a row with at most kSlBCap values of the distance at the cut was given up.) */
      int ns = 0;
      while ((bHi >> ns) > (bLo >> ns) + (unsigned long long)(kSlNB - 3)) {
        ++ns;
      }
      shift = ns;
      base = (int)(bLo >> ns) - 1;
    }
  }
  /* pass C: the list, in token order */
  int nList = 0;
  float eBlankF = __builtin_nanf(""), eSilF = 0.0f;
  int silPos = -4096;
  bool silSel = false; /* sil is in the token beam (listed, unless it is the blank) */
  uint32_t ek = 0u;
  for (int c = 0; c < nChunk && !giveUp; ++c) {
    chunk(c);
    /* (the winners' words of this chunk: lane k holds word k) */
    const unsigned long long fsMine = nBnd > 0 ? S.fSel[c * kWlRowRegs + (lane & (kWlRowRegs - 1))] : 0ull;
#pragma unroll
    for (int k = 0; k < kWlRowRegs; ++k) {
      const int tok = c * CH + k * 64 + lane;
      const float x = v[k];
      const int b = binOf(x, shift, base);
      bool sel = b <= lim;
      if (nBnd > 0) {
        const unsigned long long w = ((unsigned long long)waveReadLane32((uint32_t)(fsMine >> 32), k) << 32) |
                                     (unsigned long long)waveReadLane32((uint32_t)fsMine, k);
        sel = sel || ((w >> lane) & 1ull) != 0ull;
      }
      const bool isBlank = ctc && tok == P.blank;
      const unsigned long long selAll = waveBallot(sel);
      if (selAll == 0ull) {
        continue;
      }
      const unsigned long long bal = waveBallot(sel && !isBlank);
      if (sel && isBlank) {
        eBlankF = x;
      }
      if (sel && tok != P.sil) {
        const uint32_t kk = f32Key(x);
        ek = kk > ek ? kk : ek;
      }
      if (sel && tok == P.sil) {
        eSilF = x;
        silSel = true;
      }
      if (sel && !isBlank) {
        const int pos = nList + wavePrefixCount(bal);
        out->e[pos] = x;
        out->tok[pos] = (uint16_t)tok;
        if (tok == P.sil) {
          silPos = pos;
        }
      }
      nList += popc64(bal);
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

/* the front-end kernel: workgroup = utterance * tokRowBlocks + row block, (row block) * (waves per workgroup) + wave = row */
FLTX_DEV void wlTokBeamRows(const DecodeParams& P, char* smem) {
  const int wave = waveUniform(waveId());
  const int ub = (int)blockIdx.x / P.tokRowBlocks, rb = (int)blockIdx.x % P.tokRowBlocks;
  const int b = P.uttMap ? P.uttMap[ub] : ub;
  const int t = rb * ((int)blockDim.x >> 6) + wave;
  const int T = P.stepT ? P.stepT[b] : 0;
  if (t >= T) {
    return;
  }
  WlFrontLds& S = ((WlFrontLds*)smem)[wave];
  const float* row = P.emissions + P.emOff[b] + (size_t)t * P.N;
  WlTokRow* out = (WlTokRow*)P.tokRows + (P.histOff[b] / P.K + t);
  wlTokBeamRow(P, S, row, out, P.criterion == 1);
}

/* A stream's chunk: the records are indexed by the CALL's frames -- stream b's start at the number of frames the call
 * gives the streams before it -- so the buffer is as large as the call, not as the streams' history.  One wave. */
FLTX_DEV int64_t wlCallRowBase(const DecodeParams& P, int b) {
  int s = 0;
  for (int i = laneId(); i < b; i += 64) {
    s += P.stepT[i];
  }
  return (int64_t)waveReadLane32((uint32_t)waveInclusiveScan(s), 63);
}
/* ... its front-end kernel: workgroup = stream * tokRowBlocks + row block, as above */
FLTX_DEV void wlTokBeamRowsCall(const DecodeParams& P, char* smem) {
  const int wave = waveUniform(waveId());
  const int ub = (int)blockIdx.x / P.tokRowBlocks, rb = (int)blockIdx.x % P.tokRowBlocks;
  const int b = P.uttMap ? P.uttMap[ub] : ub;
  const int t = rb * ((int)blockDim.x >> 6) + wave;
  const int T = P.stepT ? P.stepT[b] : 0;
  if (t >= T) {
    return;
  }
  WlFrontLds& S = ((WlFrontLds*)smem)[wave];
  const float* row = P.emissions + P.emOff[b] + (size_t)t * P.N;
  WlTokRow* out = (WlTokRow*)P.tokRows + (wlCallRowBase(P, b) + t);
  wlTokBeamRow(P, S, row, out, P.criterion == 1);
}

struct WlFront {
  double bestChain; /* best candidate of the newest staged frame.  With a token LM (TL) it is the chain of the rows' best
                       emissions only, no frame's best candidate: `best` / `thr` staged from it are replaced behind
                       barrier 0, and what it still decides is WlRow::dead -- a row whose best emissions do not add up to
                       a finite number sends the utterance to the general engines, as a non-finite frame's best does */
  /* the record of the row the next call stages, loaded a frame ahead: lane l holds list position l */
  float pe;
  uint32_t ptok;
  float pBlank, pSil;
  uint32_t pEk, pFlags;
  int32_t pNList, pSilPos;
};
FLTX_DEV void wlRowPrefetch(const DecodeParams& P, WlFront& F, int64_t rowIdx, bool any) {
  const int lane = laneId();
  const WlTokRow* rec = (const WlTokRow*)P.tokRows + rowIdx;
  if (any) {
    F.pe = rec->e[lane];
    F.ptok = (uint32_t)rec->tok[lane];
    F.pBlank = rec->eBlank;
    F.pSil = rec->eSil;
    F.pEk = rec->ek;
    F.pFlags = rec->flags;
    F.pNList = rec->nList;
    F.pSilPos = rec->silPos;
  }
}
/* Stages the prefetched row into parity q: list (eTok / tokTok / posOf), blank's emission, the frame's best candidate.
 * One wave.  nListOld: the positions of parity q ^ 1's list are taken out of posOf first. */
template <class LdsT>
FLTX_DEV void wlStageRow(const DecodeParams& P, LdsT& S, WlFront& F, int64_t rowIdxNext, bool anyNext, int q,
                         double silScore, int nListOld) {
  const int lane = laneId();
  if (lane < nListOld) {
    S.posOf[S.tokTok[q ^ 1][lane]] = (uint8_t)kWlNoPos;
  }
  waveSync();
  const int nList = F.pNList;
  const bool listed = lane < nList;
  S.eTok[q][lane] = listed ? (double)F.pe : __builtin_nan("");
  S.tokTok[q][lane] = listed ? F.ptok : 0u;
  if (listed) {
    S.posOf[F.ptok] = (uint8_t)lane;
  }
  /* best candidate of the frame: best hypothesis (= the last frame's best candidate) + best token, sil priced apart */
  const double mmax = F.bestChain;
  double best = 0.0;
  bool any = false;
  if (F.pEk != 0u) {
    best = mmax + (double)f32FromKey(F.pEk);
    any = true;
  }
  if (F.pFlags & 1u) {
    const double sS = (mmax + (double)F.pSil) + silScore;
    if (sS == sS && (!any || sS > best)) {
      best = sS;
      any = true;
    }
  }
  F.bestChain = best;
  if (lane == 0) {
    S.row[q].best = best;
    S.row[q].thr = best - P.beamThreshold;
    S.row[q].eBlank = (double)F.pBlank;
    S.row[q].nList = nList;
    S.row[q].silPos = F.pSilPos;
    S.row[q].dead = ((F.pFlags & 2u) || !any || !(best - best == 0.0)) ? 1u : 0u;
  }
  wlRowPrefetch(P, F, rowIdxNext, anyNext); /* the row after this one on its way into the registers */
}

/* ST: the frames of one decodeStep chunk of a LexiconFreeDecoder stream.  The beam comes from the slots the last launch
 * (or the generic engine's begin / prune) parked and goes back there in that engine's format, so begin, end, prune,
 * getBestHypothesis, finish and the partial transcripts stay the kernels they are; LM states are named through that
 * engine's id table; history rows are its plain records with the token in a word of its own (tokens beyond a byte).
 * The token beams of the chunk's rows come from fltx_tokbeam_stream_kernel, launched ahead on the same stream. */
template <int GT, bool ST = false, bool TL = false, bool LA = false>
FLTX_DEV void wlaneUtterance(const DecodeParams& P, char* smem) {
  static_assert(!(LA && ST), "streams with logAdd stay on the generic engine");
  using LdsT = typename std::conditional<ST, typename std::conditional<TL, WtStreamLds, WlStreamLds>::type,
                                         typename std::conditional<TL, WtLds, typename std::conditional<LA, WlaLds, WlaneLds>::type>::type>::type;
  LdsT& S = *(LdsT*)smem;
  const int b = P.uttMap ? P.uttMap[blockIdx.x] : (int)blockIdx.x;
  const int W = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = laneId(), wave = waveUniform(waveId());
  const int nW = W >> 6;
  const int selfWave = nW - 2;
  const int prepWave = nW - 1;
  const bool isSelfW = wave == selfWave, isSvcW = wave == prepWave;
#ifndef FLTX_EMU
  if (!(P.tune & 1) && (isSelfW || isSvcW)) { /* (see fltx_slane.h) */
    __builtin_amdgcn_s_setprio(3);
  }
#endif
  const int K = P.K, N = P.N;
  const bool ctc = P.criterion == 1;
  const int T = P.stepT ? P.stepT[b] : 0;
  const float* em = P.emissions ? P.emissions + P.emOff[b] : nullptr;
  const int64_t hbase = P.histOff[b];
  const double NEG = slNegInf();
  static_assert(GT >= 3, "the self wave keeps its three groups in the slot arrays");
  double silScore = P.silScore;
#ifndef FLTX_EMU
  __asm__ volatile("" : "+v"(silScore)); /* (see fltx_slane.h) */
#endif

  if constexpr (ST) {
    if (T == 0) { /* no frames for this stream in this chunk: its parked beam, counters and history stay as they are */
      if (tid == 0 && P.statusHost) {
        P.statusHost[b] = P.uttStatus[b];
      }
      return;
    }
  }

  /* ---- decodeBegin (LexiconFreeDecoder.cpp:20-28): the root state ------------------ */
  for (int i = tid; i < 2 * 64; i += W) {
    ((unsigned long long*)S.cmask)[i] = 0ull;
  }
  for (int i = tid; i < 2 * kSlNB; i += W) {
    ((uint32_t*)S.hist)[i] = 0u;
  }
  if constexpr (!ST) {
  for (int i = tid; i < kWlBloomWords / 4; i += W) {
    ((uint4*)S.bloom)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  for (int i = tid; i < kWlEdgeSlots / 2; i += W) {
    ((uint4*)S.edge)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  }
  for (int i = tid; i < kWlMaxN / 16; i += W) {
    ((uint4*)S.posOf)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
  }
  if (tid < 32) {
    S.off[tid] = 0u;
  }
  if (tid < 16) {
    S.scal[tid] = 0u;
  }
  if constexpr (ST) {
    if (tid == 0) {
      S.row[0].nev = 0u;
      S.row[1].nev = 0u;
      S.row[0].dead = 0u;
      S.row[1].dead = 0u;
    }
  } else {
  if (tid == 0) {
    SlRec r;
    r.nb = 0.0;
    r.b = NEG;
    r.info = kWlNoPos | (0u << 8) | (0u << 16) | (kSlNoHyp << 24); /* (the position is filled in below) */
    r.sid = 0u;
    r.spar = 0x7FFFFFu;
    r.pad = (uint32_t)P.sil;
    S.rec[0][0] = r;
    S.row[0].nev = 0u;
    S.row[1].nev = 0u;
    S.row[0].dead = 0u;
    S.row[1].dead = 0u;
    P.histPT[hbase] = make_int2((int)kSlNoHyp, P.sil);
  }
  if (tid > 0 && tid < K) { /* unused slots of a row never look like the record of a new state (wlReenter) */
    P.histPT[hbase + tid] = make_int2((int)kSlNoHyp, -1);
  }
  }
  if constexpr (ST && TL) { /* (ids are renumbered between chunks: the memo starts empty in every launch) */
    for (int i = tid; i < kWtsMemoSlots / 2; i += W) {
      ((uint4*)S.lmMemo)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    if (tid < 4) {
      S.stat[tid] = 0u;
    }
    if (tid < 2) {
      S.fbest[tid] = 0ull;
    }
  }
  if constexpr (TL && !ST) {
    for (int i = tid; i < kWtMemoSlots; i += W) {
      S.lmMemo[i] = ~0ull; /* (no state id reaches this tag) */
    }
    if (tid < 4) {
      S.stat[tid] = 0u;
    }
    if (tid == 0) { /* KenLM::start(false): context = <s> (KenLM.cpp:57), as the generic engine's decodeBegin */
      uint32_t node = 0u;
      float pr;
      const bool ok = ngFind(P, 0u, (uint32_t)P.lmBos, node, pr);
      for (int k = 0; k < kWtCtx; ++k) {
        S.ctx[0][k][0] = (k == 0 && ok) ? (int32_t)node : 0;
      }
      S.lmNB[0][0] = 0.0;
      S.lmB[0][0] = 0.0;
      S.lmIn[0][0] = 0.0f;
      S.fbest[0] = 0ull;
      S.fbest[1] = 0ull;
    }
  }
  if constexpr (LA && !TL) {
    if (tid == 0) {
      S.mmaxKey[0] = f64Key(0.0); /* decodeBegin: the root hypothesis, score 0 */
      S.mmaxKey[1] = 0ull;
    }
  }
  ldsBarrier();
  WlFront F;
  F.bestChain = 0.0; /* decodeBegin: the root hypothesis, score 0 */
  F.pe = 0.0f;
  F.ptok = 0u;
  F.pBlank = 0.0f;
  F.pSil = 0.0f;
  F.pEk = 0u;
  F.pFlags = 0u;
  F.pNList = 0;
  F.pSilPos = -4096;
  int64_t rowBase; /* this utterance's records of the front-end kernel */
  if constexpr (ST) {
    rowBase = wlCallRowBase(P, b);
  } else {
    rowBase = hbase / K;
  }
  if (wave == prepWave) {
    if constexpr (ST) { /* (the parked beam is sorted: slot 0 is the best hypothesis) */
      F.bestChain = P.uttNBeam[b] > 0 ? P.gScore[(size_t)b * K] : 0.0;
    }
    wlRowPrefetch(P, F, rowBase, T > 0);
    if (T > 0) {
      if constexpr (LA && !TL) { /* (the staging moves on to the next record: what the head prices the row with, first) */
        const uint32_t ek = F.pEk, flags = F.pFlags;
        const float es = F.pSil;
        wlStageRow(P, S, F, rowBase + 1, T > 1, 0, silScore, 0);
        if (lane == 0) {
          wlStageLa(S, 0, ek, es, flags);
        }
      } else {
      wlStageRow(P, S, F, rowBase + 1, T > 1, 0, silScore, 0);
      }
    } else if (lane == 0) {
      S.row[0].nList = 0;
    }
    waveSync();
    if (!ST && lane == 0) { /* the root's token (sil) in the first list */
      S.rec[0][0].info = (uint32_t)S.posOf[P.sil] | (0u << 8) | (0u << 16) | (kSlNoHyp << 24);
    }
  }
  if constexpr (ST) {
    if (tid == 0) {
      S.scal[SL_NEXTID] = (uint32_t)P.uttNextId[b];
      S.scal[WL_FRAME0] = (uint32_t)P.uttFrame[b]; /* rows already in the buffer */
      S.scal[WL_TOTAL0] = (uint32_t)P.uttTotal[b]; /* frames decoded since decodeBegin */
    }
  }
  ldsBarrier();
  if constexpr (ST) {
    /* ---- restore: the beam parked by the last launch (sorted slots, one hypothesis each) -> lanes, one per LM state;
     * a slot's number is its hypothesis's slot in the last history row.  After the first row is staged: a lane's record
     * carries the position of its last token in THAT row's list ------------------------------------------------- */
    if (wave == 0) {
      const int nB = P.uttNBeam[b];
      const bool valid = lane < nB;
      const size_t g = (size_t)b * K + (valid ? lane : 0);
      const double sc = P.gScore[g], amv = P.gAm[g];
      const uint32_t sid = valid ? P.gState[g] : 0xFFFFFFFFu, spar = P.gSPar[g], tp = P.gTokPb[g];
      const int32_t edge = P.gSEdge[g];
      const bool isB = (tp & kPrevBlank) != 0u;
      int leader = lane;
      for (int i = 0; i < nB && i < 64; ++i) {
        const uint32_t si = waveReadLane32(sid, i);
        leader = (valid && si == sid && i < leader) ? i : leader;
      }
      const unsigned long long leaders = waveBallot(valid && leader == lane);
      const int L = popc64(leaders & ((1ull << leader) - 1ull));
      if (valid && leader == lane) {
        /* (the start state, and a state whose parent a compaction has cut loose, take no arrival: fltx_xlane.h) */
        const bool noArr = sid == 0u || P.idPar[(size_t)b * P.idCap + sid] == kNoParent32;
        const uint32_t tok = sid == 0u ? (uint32_t)P.sil : (uint32_t)edge;
        SlRec r;
        r.nb = NEG;
        r.b = NEG;
        r.info = tok < (uint32_t)kWlMaxN ? (uint32_t)S.posOf[tok] : kWlNoPos;
        r.sid = sid;
        r.spar = noArr ? (spar | kWlNoArrival) : spar;
        r.pad = tok;
        S.rec[0][L] = r;
        S.amNB[0][L] = 0.0;
        S.amB[0][L] = 0.0;
        S.rsNB[L] = (uint8_t)kSlNoHyp;
        S.rsB[L] = (uint8_t)kSlNoHyp;
        if constexpr (TL) { /* the state's context: its id's stateCtx row (compactions move the rows with the ids) */
          const int Lc = P.lmOrder - 1;
          const int32_t* cx = P.stateCtx + ((size_t)b * P.stateCap + (sid < P.stateCap ? sid : 0u)) * (size_t)Lc;
#pragma unroll
          for (int k = 0; k < kWtCtx; ++k) {
            S.ctx[0][k][L] = k < Lc ? cx[k] : 0;
          }
          S.lmNB[0][L] = 0.0;
          S.lmB[0][L] = 0.0;
        }
      }
      waveSync();
      if (valid) {
        if (isB) {
          S.rec[0][L].b = sc;
          S.amB[0][L] = amv;
          S.rsB[L] = (uint8_t)lane;
          if constexpr (TL) {
            S.lmB[0][L] = P.gLm[g];
          }
        } else {
          S.rec[0][L].nb = sc;
          S.amNB[0][L] = amv;
          S.rsNB[L] = (uint8_t)lane;
          if constexpr (TL) {
            S.lmNB[0][L] = P.gLm[g];
          }
        }
      }
      waveSync();
      const int nSt = popc64(leaders);
      /* lane j: history slots of its hypotheses, the lane of its parent state */
      const bool lv = lane < nSt;
      const SlRec mine = S.rec[0][lv ? lane : 0];
      int plr = -1;
      for (int i = 0; i < nSt; ++i) {
        const uint32_t si = waveReadLane32(mine.sid, i);
        plr = (lv && si == mine.spar && i != lane) ? i : plr;
      }
      if (lv) {
        S.rec[0][lane].info = (mine.info & 0xFFu) | ((uint32_t)(plr + 1) << 8) | ((uint32_t)S.rsNB[lane] << 16) |
                              ((uint32_t)S.rsB[lane] << 24);
        if (plr >= 0 && (mine.info & 0xFFu) < 64u) {
          atomOr64(&S.cmask[0][plr], 1ull << (mine.info & 0xFFu));
        }
      }
      if constexpr (TL) {
        /* the LM score a state was entered with = its parent state's extension by its last token: one look-up per lane
         * that takes arrivals, all lanes side by side, from the parent id's stateCtx row (the row of the parent's lane when
         * it holds one; when it does not, wlRelink may still give the lane its parent back later in this chunk) */
        float lin = 0.0f;
        if (lv && (mine.spar & kWlNoArrival) == 0u && mine.spar < P.stateCap) {
          const int Lc = P.lmOrder - 1;
          const int32_t* px = P.stateCtx + ((size_t)b * P.stateCap + mine.spar) * (size_t)Lc;
          int32_t pc[kWtCtx];
#pragma unroll
          for (int k = 0; k < kWtCtx; ++k) {
            pc[k] = k < Lc ? px[k] : 0;
          }
          lin = wtNgram(P, pc, mine.pad, nullptr);
        }
        if (lv) {
          S.lmIn[0][lane] = lin;
        }
      }
      if (lane == 0) {
        S.scal[SL_NSTATE] = (uint32_t)nSt;
      }
    }
    ldsBarrier();
  }

  int nState = ST ? (int)S.scal[SL_NSTATE] : 1;
  double endBest = 0.0; /* best hypothesis of the final beam (decodeEnd's threshold) */
  int winShift = kSlCoarseShift, winBase = kSlCoarseBase;
  bool dead = false; /* this utterance goes to the general engines */
  const int blank = P.blank;
  int2* const histPT = P.histPT;
  /* per-phase clocks of one thread (bench.py --profile: the marks of fltx_slane.h) */
  unsigned long long acc[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  unsigned long long tPrev = devClock();
  const bool profMe = P.prof != nullptr && tid == P.profThread;
  auto mark = [&](int i) {
    if (profMe) {
      const unsigned long long t_ = devClock();
      acc[i] += t_ - tPrev;
      tPrev = t_;
    }
  };

  /* the first list position of this token wave, kept in a vector register: as a scalar the compiler derives sixteen more
   * scalars per frame from it (position numbers, 64-bit masks), which the frame loop has no scalar registers for --
   * it recomputed and spilled them at the head of every frame */
  int posBase = wave * GT;
#ifndef FLTX_EMU
  __asm__ volatile("" : "+v"(posBase));
#endif
  WlTokLmUtt<TL> U; /* (empty without a token LM, and touched under `if constexpr (TL)` alone) */
  if constexpr (TL) {
    U.lmW = P.lmWeight;
    U.wU = U.lmW >= 0.0 ? U.lmW * (double)P.wtLmMax : U.lmW * (double)P.wtLmMin;
    U.prof = P.prof != nullptr;
    U.cnt[0] = U.cnt[1] = U.cnt[2] = U.cnt[3] = 0u;
  }

  auto frameStep = [&](auto PT, auto RL, const int t) {
    constexpr int p = decltype(PT)::value, q = p ^ 1;
    constexpr bool isSelf = decltype(RL)::value == 1, isSvc = decltype(RL)::value == 2;
    WlStreamRegs<ST> A;
    int frameOut = t + 1;
    if constexpr (ST) {
      A.frame0 = (int)S.scal[WL_FRAME0];
      A.total0 = (int)S.scal[WL_TOTAL0];
      frameOut = A.frame0 + t + 1;
    }
    const int64_t hrow = hbase + (int64_t)frameOut * K;
    /* ---- phase 1: own state, candidates, histogram ------------------------------------- */
    double best = S.row[p].best, thr = S.row[p].thr; /* (TL: the reduction behind barrier 0 replaces both) */
    WlTokLmRegs<TL, GT> L;
    const int nList = S.row[p].nList, silPos = S.row[p].silPos;
    const uint32_t rowDead = S.row[p].dead;
    const uint32_t nev = S.row[p].nev;
    WlLogAddRegs<LA, GT> G; /* (empty without logAdd) */
    if constexpr (LA && !TL) { /* best candidate = best hypothesis of the beam + best listed token, sil priced apart */
      const double mmax = f64FromKey(S.mmaxKey[p]);
      const double eM = S.eMax[p];
      const double sS = (mmax + S.eSil[p]) + silScore;
      bool any = eM == eM;
      best = any ? mmax + eM : 0.0;
      if (sS == sS && (!any || sS > best)) {
        best = sS;
        any = true;
      }
      thr = best - P.beamThreshold;
      if (!any || !(best - best == 0.0)) { /* no candidate at all, or not finite: the general engines (every wave alike) */
        dead = true;
        return;
      }
    }
    SlRec me = {};
    unsigned long long cm = 0ull;
    if (!isSvc) {
      me = S.rec[p][lane];
      cm = S.cmask[p][lane];
    }
    double ev[GT];
    uint32_t tk[GT];
    double eBlank = 0.0;
#pragma unroll
    for (int j = 0; j < GT; ++j) {
      ev[j] = 0.0;
      tk[j] = 0u;
    }
    if (isSelf) {
      eBlank = S.row[p].eBlank;
    } else if (!isSvc) {
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        const int pos = posBase + j;
        ev[j] = pos < 64 ? S.eTok[p][pos < 64 ? pos : 0] : __builtin_nan("");
        tk[j] = S.tokTok[p][pos < 64 ? pos : 0];
      }
    }
    (void)nList;
#ifndef FLTX_EMU
    if (!isSvc) { /* (the loads stay above the rare branches that follow: see fltx_slane.h) */
      __asm__ volatile("" : "+v"(me.nb), "+v"(me.b), "+v"(me.info), "+v"(me.sid), "+v"(me.spar), "+v"(me.pad), "+v"(cm));
    }
#endif
    if (nev != 0u) { /* rare: edges the filter had seen were taken in the previous build */
      if constexpr (ST) {
        wlRelink(S, p, nState);
      } else {
        wlReenter(S, histPT, p, nState, hbase, (int64_t)frameOut * K);
      }
      me = S.rec[p][lane];
      cm = S.cmask[p][lane];
    }
    if (rowDead) { /* nothing to extend with, not finite, or the token beam could not be cut: general path */
      dead = true;
      return;
    }
    const bool live = lane < nState && !isSvc;
    const double nb = live ? me.nb : NEG, bb = live ? me.b : NEG;
    const uint32_t lastPos = me.info & 0xFFu;
    const uint32_t last = me.pad;
    const int pl = live ? (int)((me.info >> 8) & 0xFFu) - 1 : -1;
    const uint32_t hypNB = (me.info >> 16) & 0xFFu, hypB = me.info >> 24;
    const bool whichB = bb > nb;
    const double m = whichB ? bb : nb;
    const uint32_t hypM = whichB ? hypB : hypNB;
    if constexpr (ST) { /* streams carry the emitting-model score of every hypothesis (getBestHypothesis returns an ancestor's) */
      A.amNB = isSvc ? 0.0 : S.amNB[p][lane];
      A.amB = isSvc ? 0.0 : S.amB[p][lane];
      A.amM = whichB ? A.amB : A.amNB;
      A.parAmNB = 0.0;
      A.parAmB = 0.0;
      A.amR = 0.0;
      A.prevR = 0u;
      A.amNew = 0.0;
    }
    if constexpr (ST && TL) {
      A.bit = 0u;
      A.fresh = 0u;
    }
    /* self wave: what its groups need beyond the lane's own record (second LDS round trip) */
    SlRec par = {};
    double eLast = 0.0;
    if (isSelf) {
      par = S.rec[p][pl >= 0 ? pl : 0];
      eLast = S.eTok[p][lastPos < 64u ? lastPos : 0u];
      if constexpr (ST) {
        A.parAmNB = S.amNB[p][pl >= 0 ? pl : 0];
        A.parAmB = S.amB[p][pl >= 0 ? pl : 0];
      }
    }
    if constexpr (TL) {
      L.thrLB = NEG;
      L.lIn = 0.0f;
      L.lmE = 0.0f;
      L.lmNew = 0.0;
      L.lmR = 0.0;
      L.parLmNB = 0.0;
      L.parLmB = 0.0;
      if (!isSvc) {
#pragma unroll
        for (int k = 0; k < kWtCtx; ++k) {
          L.ctx[k] = S.ctx[p][k][lane];
        }
        L.lmNB = S.lmNB[p][lane];
        L.lmB = S.lmB[p][lane];
        /* the filter's bound: the lanes' blank and own-repeat candidates carry no new LM term and are candidates of this
         * frame, so their maximum is at most the frame's best; every wave prices them from the records it holds */
        const double eB = S.row[p].eBlank; /* (NaN: blank is not in the token beam) */
        const double eL0 = S.eTok[p][lastPos < 64u ? lastPos : 0u];
        double cb = m + eB, r0 = nb + eL0;
        if (blank == P.sil) {
          cb = cb + silScore;
        }
        if ((int)lastPos == silPos) {
          r0 = r0 + silScore;
        }
        unsigned long long k = (ctc && live && cb == cb) ? f64Key(cb) : 0ull;
        const unsigned long long k2 = (live && lastPos < 64u && hypNB != kSlNoHyp && r0 == r0) ? f64Key(r0) : 0ull;
        k = k2 > k ? k2 : k;
        k = waveMax64(k);
        L.thrLB = k != 0ull ? f64FromKey(k) - P.beamThreshold : NEG;
      }
      if (isSelf) {
        L.lIn = S.lmIn[p][lane];
        L.parLmNB = S.lmNB[p][pl >= 0 ? pl : 0];
        L.parLmB = S.lmB[p][pl >= 0 ? pl : 0];
      }
    }
    mark(0);
    double cs[GT];
    int cbin[GT];
    uint32_t parR = kSlNoHyp;
    if (isSvc) {
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        cs[j] = NEG;
        cbin[j] = kSlInvalid;
      }
      /* the next frame's list (found by the front-end kernel, on its way since the last frame), position table and
       * best candidate, while the other waves evaluate this frame's candidates (everything written here belongs to
       * the next frame; the position table is read by the build below, after the second barrier, and by nothing
       * before that) */
      if constexpr (LA && !TL) {
        if (t + 1 < T) {
          const uint32_t ek = F.pEk, flags = F.pFlags;
          const float es = F.pSil;
          wlStageRow(P, S, F, rowBase + t + 2, t + 2 < T, q, silScore, nList);
          if (lane == 0) {
            wlStageLa(S, q, ek, es, flags);
          }
        }
        if (lane == 0) {
          S.mmaxKey[q] = 0ull; /* (this frame's build raises it) */
        }
      } else {
      if (t + 1 < T) {
        wlStageRow(P, S, F, rowBase + t + 2, t + 2 < T, q, silScore, nList);
      }
      }
    } else if (!isSelf) {
      /* positions this lane does not extend with here: its own last token's (the repeat and the blank-then-last case
       * belong to the self wave) and those whose child state holds a lane (that lane merges the extension into its
       * repeat).  A lane without a state skips all. */
      const unsigned long long skip = live ? (cm | (lastPos < 64u ? 1ull << lastPos : 0ull)) : ~0ull;
      if constexpr (LA && !TL) {
        /* the state's other hypothesis reaches the same child state: fl(a + e) is monotone, so it is the smaller member */
        const bool hasOther = (whichB ? hypNB : hypB) != kSlNoHyp;
        double c1[GT];
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          c1[j] = m + ev[j]; /* NaN past the end of the list */
          G.c2[j] = (whichB ? nb : bb) + ev[j];
        }
        slSilAdd<GT, true>(c1, G.c2, silScore != 0.0, silPos, wave, silScore);
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          const int pos = posBase + j;
          double c = c1[j];
          const bool ok = pos < 64 && ((skip >> (pos & 63)) & 1ull) == 0ull && c >= thr;
          if (ok && hasOther && G.c2[j] >= thr) {
            c = slLogAdd(c, G.c2[j]);
          }
          cs[j] = c;
          cbin[j] = ok ? slBin<true>(best, c, winShift, winBase) : kSlInvalid;
        }
      } else {
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        const int pos = posBase + j;
        double c = m + ev[j]; /* NaN past the end of the list */
        if (pos == silPos) {
          c = c + silScore;
        }
        if constexpr (TL) { /* (the LM term, the threshold and the bin follow below) */
          L.pre[j] = pos < 64 && ((skip >> (pos & 63)) & 1ull) == 0ull && c == c;
          cs[j] = c;
          cbin[j] = kSlInvalid;
          if constexpr (LA) { /* the second member: the state's other hypothesis, the same emission (and LM term, below) */
            double c2 = (whichB ? nb : bb) + ev[j];
            if (pos == silPos) {
              c2 = c2 + silScore;
            }
            G.c2[j] = c2;
            G.two = (whichB ? hypNB : hypB) != kSlNoHyp ? (1u << GT) - 1u : 0u;
          }
        } else {
        const bool ok = pos < 64 && ((skip >> (pos & 63)) & 1ull) == 0ull && c >= thr;
        cs[j] = c;
        cbin[j] = ok ? slBin<false>(best, c, winShift, winBase) : kSlInvalid;
        }
      }
      }
    } else {
      const bool lastOk = live && lastPos < 64u; /* the last token is in the frame's token beam (never blank) */
      const bool lastSil = (int)lastPos == silPos;
      /* (S, blank, true): LexiconFreeDecoder.cpp:86-97 -- eBlank is NaN when blank is not in the token beam */
      double cB = m + eBlank;
      if (blank == P.sil) {
        cB = cB + silScore;
      }
      const bool okB = ctc && live && cB >= thr;
      if constexpr (LA) { /* the blank group's second member: the state's other hypothesis */
        double cB2 = (whichB ? nb : bb) + eBlank;
        if (blank == P.sil) {
          cB2 = cB2 + silScore;
        }
        G.c2[0] = cB2;
        G.two = (whichB ? hypNB : hypB) != kSlNoHyp ? 1u : 0u;
        if constexpr (!TL) {
          if (okB && G.two != 0u && cB2 >= thr) {
            cB = slLogAdd(cB, cB2);
          }
        }
      }
      /* (S, last, false): the repeat (:98-110) and the parent state's extension by last (:69-85) */
      const uint32_t lastP = par.pad;
      const uint32_t h1 = (par.info >> 16) & 0xFFu, h2 = par.info >> 24;
      const bool has0 = hypNB != kSlNoHyp;
      const bool has1 = pl >= 0 && last != lastP && h1 != kSlNoHyp;
      const bool has2 = pl >= 0 && ctc && h2 != kSlNoHyp;
      const bool hasB = hypB != kSlNoHyp;
      double r0 = nb + eLast;
      double r1 = has1 ? par.nb + eLast : NEG;
      double r2 = has2 ? par.b + eLast : NEG;
      /* (S.last, last, false) from (S, blank, true) when no lane holds S.last */
      double cL = bb + eLast;
      if (silScore != 0.0) {
        r0 = lastSil ? r0 + silScore : r0;
        r1 = lastSil ? r1 + silScore : r1;
        r2 = lastSil ? r2 + silScore : r2;
        cL = lastSil ? cL + silScore : cL;
      }
      if constexpr (TL) { /* the parent state's extension by last(S) is a new-token candidate: the term S was entered with */
        const double wIn = U.lmW * (double)L.lIn;
        r1 = r1 + wIn;
        r2 = r2 + wIn;
      }
      /* max-merge (Utils.h:194-196); a tie goes to the lower history slot */
      double cR = r0;
      parR = hypNB;
      const bool t1 = has1 & ((r1 > cR) | ((r1 == cR) & (h1 < parR)));
      cR = t1 ? r1 : cR;
      parR = t1 ? h1 : parR;
      const bool t2 = has2 & ((r2 > cR) | ((r2 == cR) & (h2 < parR)));
      cR = t2 ? r2 : cR;
      parR = t2 ? h2 : parR;
      if constexpr (ST) {
        A.amR = t2 ? A.parAmB : (t1 ? A.parAmNB : A.amNB);
        A.prevR = t2 ? (uint32_t)blank : (t1 ? lastP : last);
      }
      bool okR = lastOk && (has0 || has1 || has2) && cR >= thr;
      if constexpr (LA) { /* (the best member is cR, its slot parR) */
        G.r0 = r0;
        G.r1 = r1;
        G.r2 = r2;
        G.has = (has0 ? 1u : 0u) | (has1 ? 2u : 0u) | (has2 ? 4u : 0u);
        if constexpr (!TL) {
          double sum;
          okR = wlRepeatLogAdd(r0, r1, r2, G.has, thr, sum) && lastOk;
          cR = okR ? sum : cR;
        }
      }
      const bool okL = ctc && lastOk && hasB && ((cm >> (lastPos & 63u)) & 1ull) == 0ull && cL >= thr;
      cs[0] = cB;
      cs[1] = cR;
      cs[2] = cL;
      cbin[0] = okB ? slBin<LA>(best, cB, winShift, winBase) : kSlInvalid;
      cbin[1] = okR ? slBin<LA>(best, cR, winShift, winBase) : kSlInvalid;
      cbin[2] = okL ? slBin<LA>(best, cL, winShift, winBase) : kSlInvalid;
#pragma unroll
      for (int j = 3; j < GT; ++j) {
        cs[j] = NEG;
        cbin[j] = kSlInvalid;
      }
      if constexpr (TL) { /* (blank-then-last is a new-token candidate of the lane's own: position 2 asks the LM below) */
        L.lmR = t2 ? L.parLmB + (double)L.lIn : (t1 ? L.parLmNB + (double)L.lIn : L.lmNB);
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          L.pre[j] = false;
        }
        L.pre[0] = ctc && live && cB == cB;
        L.pre[1] = lastOk && (has0 || has1 || has2) && cR == cR;
        L.pre[2] = ctc && lastOk && hasB && ((cm >> (lastPos & 63u)) & 1ull) == 0ull && cL == cL;
        tk[2] = last;
      }
    }
    if constexpr (TL) {
      if (!isSvc) {
        /* which of these candidates ask the LM: a token wave's all, the own-groups wave's third */
        constexpr uint32_t lmSlots = isSelf ? 4u : (1u << GT) - 1u;
        uint32_t need = 0u;
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          L.lmv[j] = 0.0f;
          if (((lmSlots >> j) & 1u) != 0u && L.pre[j]) {
            const bool ask = !(cs[j] + U.wU < L.thrLB); /* (below the bound with the LM's best term: cannot reach the threshold) */
            L.pre[j] = ask;
            bool hit = false;
            if (ask) {
              const unsigned long long e = S.lmMemo[wtSlotOf<ST>(me.sid, tk[j])];
              hit = (uint32_t)(e >> 32) == wtTagOf<ST>(me.sid, tk[j]);
              L.lmv[j] = hit ? __uint_as_float((uint32_t)e) : 0.0f;
              need |= hit ? 0u : (1u << j);
            }
            if (U.prof) {
              U.cnt[0] += 1u;
              U.cnt[1] += ask ? 0u : 1u;
              U.cnt[2] += ask ? 1u : 0u;
              U.cnt[3] += hit ? 1u : 0u;
            }
          }
        }
        while (waveBallot(need != 0u) != 0ull) { /* the misses: every lane's next one side by side */
          if (need != 0u) {
            const int jj = __builtin_ctz(need);
            need &= need - 1u;
            uint32_t tok = 0u;
#pragma unroll
            for (int j = 0; j < GT; ++j) {
              tok = j == jj ? tk[j] : tok;
            }
            const float v = wtNgram(P, L.ctx, tok, nullptr);
            S.lmMemo[wtSlotOf<ST>(me.sid, tok)] = ((unsigned long long)wtTagOf<ST>(me.sid, tok) << 32) | (unsigned long long)__float_as_uint(v);
#pragma unroll
            for (int j = 0; j < GT; ++j) {
              L.lmv[j] = j == jj ? v : L.lmv[j];
            }
          }
        }
        /* LexiconFreeDecoder.cpp:79: score + lmWeight * lmScore */
        unsigned long long k = 0ull;
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          if (((lmSlots >> j) & 1u) != 0u) {
            cs[j] = cs[j] + U.lmW * (double)L.lmv[j];
            if constexpr (LA) { /* (the same edge, the same term) */
              if constexpr (!isSelf) {
                G.c2[j] = G.c2[j] + U.lmW * (double)L.lmv[j];
              }
            }
          }
          const unsigned long long kc = (L.pre[j] && cs[j] == cs[j]) ? f64Key(cs[j]) : 0ull;
          k = kc > k ? kc : k;
        }
        /* the frame's best candidate (Utils.h:131-137) is a maximum over the candidates: one LDS max per wave */
        if (waveBallot(k != 0ull) != 0ull) {
          k = waveMax64(k);
          if (lane == 0) {
            atomMax64(&S.fbest[p], k);
          }
        }
      }
      ldsBarrier(); /* 0: the frame's best candidate */
      const unsigned long long bk = S.fbest[p];
      best = f64FromKey(bk);
      thr = best - P.beamThreshold;
      if (bk == 0ull || !(best - best == 0.0)) { /* no candidate at all, or not finite: the general engines */
        dead = true;
        return;
      }
      if constexpr (LA) { /* the merges, now that the threshold is known: the members that pass it, best first */
        if (!isSvc) {
#pragma unroll
          for (int j = 0; j < GT; ++j) {
            bool ok = L.pre[j] && cs[j] >= thr;
            if (isSelf && j == 1) {
              double sum;
              ok = wlRepeatLogAdd(G.r0, G.r1, G.r2, G.has, thr, sum) && L.pre[1];
              cs[1] = ok ? sum : cs[1];
            } else if (ok && ((G.two >> j) & 1u) != 0u && G.c2[j] >= thr) {
              cs[j] = slLogAdd(cs[j], G.c2[j]);
            }
            cbin[j] = ok ? slBin<true>(best, cs[j], winShift, winBase) : kSlInvalid;
          }
        }
      } else {
      if (!isSvc) {
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          cbin[j] = (L.pre[j] && cs[j] >= thr) ? slBin<false>(best, cs[j], winShift, winBase) : kSlInvalid;
        }
      }
      }
    }
    if (wave == 0) { /* housekeeping for everybody: what this frame's build adds to */
      S.cmask[q][lane] = 0ull;
      if (lane < 32) {
        S.off[lane] = 0u;
      }
      if (lane == 0) {
        S.scal[SL_BCNT] = 0u;
        if constexpr (TL) {
          S.fbest[q] = 0ull; /* (the next frame's; last read a frame ago) */
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GT; ++j) {
      if (cbin[j] < kSlFar) {
        atomAdd32(&S.hist[p][cbin[j]], 1u);
      }
    }
    mark(1);
    ldsBarrier(); /* 1 */
    /* ---- phase 2: which candidates survive (Utils.h:200-220; as fltx_slane.h) ------------ */
    unsigned long long selMask[GT];
    SlScan sc = slScan(S.hist[p], K, true);
    int shift = winShift, base = winBase;
    int lim = -1;
    uint32_t take = 0u;
    bool usual = false;
    if (sc.crossed) {
      if (sc.total <= K) {
        lim = kSlFar - 1;
        usual = true;
      } else if (sc.cnt == K - sc.cum) {
        lim = sc.bstar;
        usual = true;
      }
    }
    if (__builtin_expect(usual, 1)) {
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        selMask[j] = waveBallot(cbin[j] <= lim);
      }
    } else {
      unsigned long long bLo = 0ull, bHi = 0x7FFFFFFFull;
      bool full = false;
      for (;;) {
        if (!full && !sc.crossed) {
          int nFar = 0;
#pragma unroll
          for (int j = 0; j < GT; ++j) {
            nFar += popc64(waveBallot(cbin[j] == kSlFar));
          }
          if (lane == 0 && nFar > 0) {
            atomAdd32(&S.hist[p][kSlFar], (uint32_t)nFar);
          }
          full = true;
          ldsBarrier();
          sc = slScan(S.hist[p], K, false);
          continue;
        }
        if (sc.total <= K) {
          lim = full ? kSlFar : kSlFar - 1;
          break;
        }
        const int need = K - sc.cum;
        if (sc.cnt == need) {
          lim = sc.bstar;
          break;
        }
        if (sc.cnt <= kSlBCap) {
          /* (the members loop over the list here, not slRankBin's broadcast + ballot of the other lane engines: with it
           * this kernel -- which spills 460 scalar registers in its frame loop -- returned wrong survivors on the GPU for
           * token beams of 64 while the emulator, compiling the same source, agreed with the oracle; not understood, so
           * the loop that 600 GPU configurations have checked stays) */
#pragma unroll
          for (int j = 0; j < GT; ++j) {
            if (cbin[j] == sc.bstar) {
              const uint32_t i = atomAdd32(&S.scal[SL_BCNT], 1u);
              S.bKey[i] = f64Key(cs[j]);
              S.bOrd[i] = ((uint32_t)wave << 16) | ((uint32_t)j << 8) | (uint32_t)lane;
            }
          }
          ldsBarrier();
#pragma unroll
          for (int j = 0; j < GT; ++j) {
            if (cbin[j] == sc.bstar) {
              const unsigned long long k = f64Key(cs[j]);
              const uint32_t o = ((uint32_t)wave << 16) | ((uint32_t)j << 8) | (uint32_t)lane;
              int rank = 0;
              for (int i = 0; i < sc.cnt; ++i) {
                const unsigned long long k2 = S.bKey[i];
                rank += (k2 > k || (k2 == k && S.bOrd[i] < o)) ? 1 : 0;
              }
              take |= rank < need ? (1u << j) : 0u;
            }
          }
          lim = sc.bstar - 1;
          break;
        }
        {
          const unsigned long long v = (unsigned long long)(sc.bstar + base);
          if (sc.bstar > 0 || base == 0) {
            const unsigned long long l2 = v << shift;
            bLo = l2 > bLo ? l2 : bLo;
          }
          if (sc.bstar < kSlNB - 1) {
            const unsigned long long h2 = ((v + 1ull) << shift) - 1ull;
            bHi = h2 < bHi ? h2 : bHi;
          }
          if (bLo >= bHi) {
            dead = true;
            break;
          }
          int ns = 0;
          while (((bHi >> ns) - (bLo >> ns)) > (unsigned long long)(kSlNB - 1)) {
            ++ns;
          }
          shift = ns;
          base = (int)(bLo >> ns);
        }
        ldsBarrier();
        for (int i = tid; i < kSlNB; i += W) {
          S.hist[p][i] = 0u;
        }
        ldsBarrier();
        full = true;
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          if (cbin[j] != kSlInvalid) {
            cbin[j] = slBin<LA>(best, cs[j], shift, base);
            atomAdd32(&S.hist[p][cbin[j]], 1u);
          }
        }
        ldsBarrier();
        sc = slScan(S.hist[p], K, false);
      }
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        selMask[j] = waveBallot(cbin[j] <= lim || ((take >> j) & 1u) != 0u);
      }
    }
    if (dead) {
      return;
    }
    if (sc.total > K) {
      const int q15 = shift >= kSlFineShift ? (sc.bstar + base) << (shift - kSlFineShift)
                                            : (sc.bstar + base) >> (kSlFineShift - shift);
      winShift = kSlFineShift;
      winBase = q15 > kSlMid ? q15 - kSlMid : 0;
    }
    mark(2);
    /* new lanes: survivors first (self wave), then the new states wave by wave */
    int nNewWave = 0;
    int myNew[GT];
    int surv = -1;
    uint32_t hNB = kSlNoHyp, hB = kSlNoHyp;
    if (isSvc) {
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        myNew[j] = 0;
      }
      ((uint4*)S.hist[q])[lane] = make_uint4(0u, 0u, 0u, 0u); /* the other parity's histogram (last read a frame ago) */
    } else if (!isSelf) {
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        myNew[j] = nNewWave + wavePrefixCount(selMask[j]);
        nNewWave += popc64(selMask[j]);
      }
      if (lane > wave && lane <= selfWave + 1 && nNewWave > 0) {
        atomAdd32(&S.off[lane], (uint32_t)nNewWave);
      }
    } else {
      const unsigned long long balB = selMask[0], balR = selMask[1], balL = selMask[2];
      const unsigned long long balS = balB | balR;
      const bool sR = ((balR >> lane) & 1ull) != 0ull;
      surv = ((balS >> lane) & 1ull) ? wavePrefixCount(balS) : -1;
      hNB = (uint32_t)(wavePrefixCount(balR) + wavePrefixCount(balB));
      hB = hNB + (sR ? 1u : 0u);
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        myNew[j] = 0;
      }
      myNew[2] = wavePrefixCount(balL);
      nNewWave = popc64(balL);
      S.newLane[lane] = surv;
      if (lane == 0) {
        S.scal[SL_NSURV] = (uint32_t)popc64(balS);
        S.scal[SL_NHSURV] = (uint32_t)(popc64(balR) + popc64(balB));
      }
      if (lane == selfWave + 1 && nNewWave > 0) {
        atomAdd32(&S.off[lane], (uint32_t)nNewWave);
      }
    }
    if constexpr (LA && !TL) {
      if (!isSvc) { /* the best hypothesis of the next beam: the best surviving (merged) score */
        unsigned long long k = 0ull;
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          const unsigned long long kj = ((selMask[j] >> lane) & 1ull) ? f64Key(cs[j]) : 0ull;
          k = kj > k ? kj : k;
        }
        if (waveBallot(k != 0ull) != 0ull) {
          k = waveMax64(k);
          if (lane == 0) {
            atomMax64(&S.mmaxKey[q], k);
          }
        }
      }
    }
    mark(3);
    ldsBarrier(); /* 2 */
    /* ---- phase 3: every survivor is written by the lane that evaluated it ---------------- */
    const int nSurv = (int)S.scal[SL_NSURV], nHSurv = (int)S.scal[SL_NHSURV];
    const int offW = (int)S.off[wave], nNew = (int)S.off[selfWave + 1];
    const int myNewLane = S.newLane[lane];
    const int plNew = S.newLane[pl >= 0 ? pl : 0];
    /* a token's position in the NEXT frame's list (the staging wave has just written the table) */
    auto nextPosOf = [&](uint32_t tok) -> uint32_t { return (t + 1 < T && tok < (uint32_t)kWlMaxN) ? (uint32_t)S.posOf[tok] : kWlNoPos; };
    auto newState = [&](int idx, double c, uint32_t n, uint32_t np, uint32_t hp) {
      const int nl = nSurv + idx;
      const uint32_t hyp = (uint32_t)(nHSurv + idx);
      SlRec r;
      r.nb = c;
      r.b = NEG;
      r.info = np | ((uint32_t)(myNewLane + 1) << 8) | (hyp << 16) | (kSlNoHyp << 24);
      r.sid = (uint32_t)frameOut * (uint32_t)K + hyp;
      r.spar = me.sid;
      r.pad = n;
      if constexpr (ST) {
        /* the generic engine's (parent id, token) -> id table names the state and remembers that it did: `fresh` = false
         * is LMState::child's memo.  One candidate per (lane, token) and frame: nobody asks about a pair twice */
        bool fresh = false;
        r.sid = tlStreamChild(P, b, me.sid, (int32_t)n, (uint32_t)(A.total0 + t + 1), &S.scal[SL_NEXTID], &S.scal[SL_STATUS], fresh);
        S.amNB[q][nl] = A.amNew;
        S.rec[q][nl] = r;
        if (myNewLane >= 0 && np < 64u) {
          atomOr64(&S.cmask[q][myNewLane], 1ull << np);
        }
        histPT[hrow + hyp] = wlPlainRec(hp, n);
        if constexpr (TL) {
          S.lmNB[q][nl] = L.lmNew;
          S.lmB[q][nl] = 0.0;
          S.lmIn[q][nl] = L.lmE;
          wlScoreRecLm(P, hrow + hyp, c, A.amNew, L.lmNew);
          A.fresh |= (fresh && r.sid != 0u) ? A.bit : 0u; /* (id 0 under `fresh`: the ids ran out, the chunk is redone) */
        } else {
        wlScoreRec(P, hrow + hyp, c, A.amNew);
        }
        if (!fresh) { /* entered before: it may have descendants in the beam (wlRelink) */
          const uint32_t e = atomAdd32(&S.row[q].nev, 1u);
          S.evLane[e] = (uint32_t)nl;
          S.evSid[e] = r.sid;
        }
      } else {
      const bool again = wlEdgeSeen(S, me.sid, n); /* this edge may have had a child before */
      const uint32_t eslot = wlEdgeSlot(me.sid, n);
      uint32_t known = kWlNoSid;
      if (again) { /* ... and the memo may still know which: the state keeps its id, the history rows are not searched */
        const unsigned long long cur = S.edge[eslot];
        if ((cur >> 23) == (wlEdgePack(me.sid, n, 0u) >> 23)) {
          known = (uint32_t)cur & 0x7FFFFFu;
          r.sid = known;
        }
      } else {
        S.edge[eslot] = wlEdgePack(me.sid, n, r.sid);
      }
      S.rec[q][nl] = r;
      if constexpr (TL) {
        S.lmNB[q][nl] = L.lmNew;
        S.lmB[q][nl] = 0.0;
        S.lmIn[q][nl] = L.lmE;
      }
      if (myNewLane >= 0 && np < 64u) {
        atomOr64(&S.cmask[q][myNewLane], 1ull << np);
      }
      histPT[hrow + hyp] = make_int2((int)(hp | kSlNewFlag | (me.sid << 9)), (int)n);
      if (again) { /* it may have descendants in the beam */
        const uint32_t e = atomAdd32(&S.row[q].nev, 1u);
        S.evLane[e] = (uint32_t)nl;
        S.evSpar[e] = me.sid;
        S.evTok[e] = n;
        S.evSid[e] = known;
      }
      }
    };
    if (isSvc) {
      /* (its part of the build went ahead of the second barrier) */
    } else if (!isSelf) {
      if (!ST && wave == 0 && lane >= nHSurv + nNew && lane < K) { /* unused slots of the history row: see wlReenter (a
                                                                       stream's rows are read up to the parked count) */
        histPT[hrow + lane] = make_int2((int)kSlNoHyp, -1);
      }
#pragma unroll
      for (int j = 0; j < GT; ++j) {
        if (selMask[j] != 0ull) {
          const uint32_t np = nextPosOf(tk[j]);
          if ((selMask[j] >> lane) & 1ull) {
            if constexpr (ST) {
              A.amNew = wlAmStep(P, A.total0 + t == 0, A.amM, ev[j], tk[j], whichB ? (uint32_t)blank : last);
            }
            if constexpr (TL) { /* LexiconFreeDecoder.cpp:85: prevHyp.lmScore + lmScore */
              L.lmE = L.lmv[j];
              L.lmNew = (whichB ? L.lmB : L.lmNB) + (double)L.lmv[j];
            }
            if constexpr (ST && TL) {
              A.bit = 1u << j;
            }
            newState(offW + myNew[j], cs[j], tk[j], np, hypM);
          }
        }
      }
    } else {
      const uint32_t lastNext = nextPosOf(last);
      if (surv >= 0) {
        const bool sB = ((selMask[0] >> lane) & 1ull) != 0ull, sR = ((selMask[1] >> lane) & 1ull) != 0ull;
        const int pln = pl >= 0 ? plNew : -1;
        SlRec r;
        r.nb = sR ? cs[1] : NEG;
        r.b = sB ? cs[0] : NEG;
        r.info = lastNext | ((uint32_t)(pln + 1) << 8) | ((sR ? hNB : kSlNoHyp) << 16) | ((sB ? hB : kSlNoHyp) << 24);
        r.sid = me.sid;
        r.spar = me.spar;
        r.pad = last;
        S.rec[q][surv] = r;
        if (pln >= 0 && lastNext < 64u) {
          atomOr64(&S.cmask[q][pln], 1ull << lastNext);
        }
        if constexpr (ST) {
          if (sR) {
            const double a = wlAmStep(P, A.total0 + t == 0, A.amR, eLast, last, A.prevR);
            S.amNB[q][surv] = a;
            histPT[hrow + hNB] = wlPlainRec(parR, last);
            if constexpr (TL) {
              wlScoreRecLm(P, hrow + hNB, cs[1], a, L.lmR);
            } else {
            wlScoreRec(P, hrow + hNB, cs[1], a);
            }
          }
          if (sB) {
            const double a = A.amM + eBlank;
            S.amB[q][surv] = a;
            histPT[hrow + hB] = wlPlainRec(hypM, (uint32_t)blank);
            if constexpr (TL) {
              wlScoreRecLm(P, hrow + hB, cs[0], a, whichB ? L.lmB : L.lmNB);
            } else {
            wlScoreRec(P, hrow + hB, cs[0], a);
            }
          }
        } else {
        if (sR) {
          histPT[hrow + hNB] = make_int2((int)parR, (int)last);
        }
        if (sB) {
          histPT[hrow + hB] = make_int2((int)hypM, blank);
        }
        }
        if constexpr (TL) { /* the state keeps its context and the term it was entered with; blank adds no LM score */
#pragma unroll
          for (int k = 0; k < kWtCtx; ++k) {
            S.ctx[q][k][surv] = L.ctx[k];
          }
          S.lmIn[q][surv] = L.lIn;
          S.lmNB[q][surv] = sR ? L.lmR : 0.0;
          S.lmB[q][surv] = sB ? (whichB ? L.lmB : L.lmNB) : 0.0;
        }
      }
      if ((selMask[2] >> lane) & 1ull) {
        if constexpr (ST) {
          A.amNew = wlAmStep(P, A.total0 + t == 0, A.amB, eLast, last, (uint32_t)blank);
        }
        if constexpr (TL) {
          L.lmE = L.lmv[2];
          L.lmNew = L.lmB + (double)L.lmv[2];
        }
        if constexpr (ST && TL) {
          A.bit = 4u;
        }
        newState(offW + myNew[2], cs[2], last, lastNext, hypB);
      }
    }
    if constexpr (TL) {
      if (!isSvc) {
        /* the contexts of the new states: ctxOut of the edge that enters them, asked for the survivors only -- every
         * lane's next one side by side */
        constexpr uint32_t lmSlots = isSelf ? 4u : (1u << GT) - 1u;
        uint32_t todo = 0u;
#pragma unroll
        for (int j = 0; j < GT; ++j) {
          todo |= (((lmSlots >> j) & 1u) != 0u && ((selMask[j] >> lane) & 1ull) != 0ull) ? (1u << j) : 0u;
        }
        while (waveBallot(todo != 0u) != 0ull) {
          if (todo != 0u) {
            const int jj = __builtin_ctz(todo);
            todo &= todo - 1u;
            uint32_t tok = 0u;
            int idx = 0;
#pragma unroll
            for (int j = 0; j < GT; ++j) {
              tok = j == jj ? tk[j] : tok;
              idx = j == jj ? myNew[j] : idx;
            }
            int32_t co[kWtCtx];
#pragma unroll
            for (int k = 0; k < kWtCtx; ++k) {
              co[k] = 0;
            }
            wtNgram(P, L.ctx, tok, co);
            const int nl = nSurv + offW + idx;
#pragma unroll
            for (int k = 0; k < kWtCtx; ++k) {
              S.ctx[q][k][nl] = co[k];
            }
            if constexpr (ST) { /* a new id: its context goes where the generic engine's kernels and the next restore look */
              const uint32_t sidNew = S.rec[q][nl].sid; /* (this lane wrote the record) */
              if (((A.fresh >> jj) & 1u) != 0u && sidNew < P.stateCap) {
                const int Lc = P.lmOrder - 1;
                int32_t* dst = P.stateCtx + ((size_t)b * P.stateCap + sidNew) * (size_t)Lc;
#pragma unroll
                for (int k = 0; k < kWtCtx; ++k) {
                  if (k < Lc) {
                    dst[k] = co[k];
                  }
                }
              }
            }
          }
        }
      }
    }
    nState = nSurv + nNew;
    endBest = best;
    mark(4);
    ldsBarrier(); /* 3 */
    mark(5);
  };
  auto frames = [&](auto RL) {
    int t = 0;
    for (; t + 1 < T && !dead; t += 2) {
      frameStep(SlParity<0>(), RL, t);
      if (dead) {
        break;
      }
      frameStep(SlParity<1>(), RL, t + 1);
    }
    if (!dead && t < T) {
      frameStep(SlParity<0>(), RL, t);
    }
  };
  if (isSvcW) {
    frames(SlParity<2>());
  } else if (isSelfW) {
    frames(SlParity<1>());
  } else {
    frames(SlParity<0>());
  }

  /* ---- decodeEnd (LexiconFreeDecoder.cpp:127-158): finish() keeps the state, token = sil; the two
   * hypotheses of a state merge; sorted n-best (candidatesStore returnSorted) ------------------ */
  if constexpr (ST) {
    /* ---- park the beam for the next launch / prune / getBestHypothesis / decodeEnd: one slot per hypothesis, sorted by
     * (score descending, history slot ascending), in the generic engine's format; the last history row rewritten in
     * that order ------------------------------------------------------------------------------------------------ */
#ifndef FLTX_EMU
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* this wave's history records are in L2 */
#endif
    ldsBarrier();
    /* (the id table full or the ids exhausted: the chunk cannot be finished here either) */
    const bool failed = dead || S.scal[SL_STATUS] != 0u;
    const int pe = T & 1;
    const int frame0 = (int)S.scal[WL_FRAME0], total0 = (int)S.scal[WL_TOTAL0];
    if (wave == 0 && !failed) {
      const bool live = lane < nState;
      const int li = live ? lane : 0;
      const SlRec me = S.rec[pe][li];
      const uint32_t sNB = live ? (me.info >> 16) & 0xFFu : kSlNoHyp, sB = live ? me.info >> 24 : kSlNoHyp;
      const bool hasNB = sNB != kSlNoHyp, hasB = sB != kSlNoHyp;
      const unsigned long long kNB = hasNB ? f64Key(me.nb) : 0ull, kB = hasB ? f64Key(me.b) : 0ull;
      int rNB = 0, rB = 0;
      for (int i = 0; i < nState; ++i) {
        const unsigned long long k1 = ((unsigned long long)waveReadLane32((uint32_t)(kNB >> 32), i) << 32) |
                                      waveReadLane32((uint32_t)kNB, i);
        const unsigned long long k2 = ((unsigned long long)waveReadLane32((uint32_t)(kB >> 32), i) << 32) |
                                      waveReadLane32((uint32_t)kB, i);
        const uint32_t s1 = waveReadLane32(sNB, i), s2 = waveReadLane32(sB, i);
        const bool e1 = s1 != kSlNoHyp, e2 = s2 != kSlNoHyp;
        rNB += (e1 && (k1 > kNB || (k1 == kNB && s1 < sNB))) ? 1 : 0;
        rNB += (e2 && (k2 > kNB || (k2 == kNB && s2 < sNB))) ? 1 : 0;
        rB += (e1 && (k1 > kB || (k1 == kB && s1 < sB))) ? 1 : 0;
        rB += (e2 && (k2 > kB || (k2 == kB && s2 < sB))) ? 1 : 0;
      }
      const int nHyp = popc64(waveBallot(hasNB)) + popc64(waveBallot(hasB));
      const int64_t hlast = hbase + (int64_t)(frame0 + T) * K;
      const unsigned long long* hrec = (const unsigned long long*)(histPT + hlast);
      const unsigned long long recNB = hasNB ? loadCoherent64(hrec + sNB) : 0ull;
      const unsigned long long recB = hasB ? loadCoherent64(hrec + sB) : 0ull;
      const double aNB = S.amNB[pe][li], aB = S.amB[pe][li];
      const uint32_t lastTok = me.pad; /* (the start state's: sil) */
      const uint32_t sparOut = me.sid == 0u ? kNoParent : (me.spar & ~kWlNoArrival);
      const int32_t edgeOut = me.sid == 0u ? 0 : (int32_t)lastTok;
#ifndef FLTX_EMU
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* every lane has its old records before any is rewritten */
#endif
      waveSync();
      double lNB = 0.0, lB = 0.0; /* the LM score of the lane's two hypotheses (ZeroLM: 0) */
      if constexpr (TL) {
        lNB = S.lmNB[pe][li];
        lB = S.lmB[pe][li];
      }
      auto put = [&](int r, double sc, double am, double lm, uint32_t tokpb, unsigned long long rec) {
        const size_t g = (size_t)b * K + r;
        P.gScore[g] = sc;
        P.gAm[g] = am;
        P.gLm[g] = lm;
        P.gState[g] = me.sid;
        P.gSPar[g] = sparOut;
        P.gSEdge[g] = edgeOut;
        P.gLex[g] = 0u;
        P.gLexMax[g] = 0.0f;
        P.gTokPb[g] = tokpb;
        ((unsigned long long*)(histPT + hlast))[r] = rec;
        if (P.histS) {
          double* hs = P.histS + 3 * (hlast + r);
          hs[0] = sc;
          hs[1] = am;
          hs[2] = lm;
        }
      };
      if (hasNB) {
        put(rNB, me.nb, aNB, lNB, lastTok, recNB);
      }
      if (hasB) {
        put(rB, me.b, aB, lB, (uint32_t)blank | kPrevBlank, recB);
      }
      if (lane == 0) {
        const int32_t stNow = P.uttStatus[b] | (int32_t)S.scal[SL_STATUS];
        P.uttNBeam[b] = nHyp;
        P.uttFrame[b] = frame0 + T;
        P.uttTotal[b] = total0 + T;
        P.uttNextId[b] = (int32_t)S.scal[SL_NEXTID];
        P.uttStatus[b] = stNow;
        if (P.statusHost) {
          P.statusHost[b] = stNow;
        }
      }
    }
    if (failed && tid == 0) {
      /* a row without a defined token beam or not finite, a select that did not converge, the id table full: this chunk
       * cannot be finished here.  The beam the chunk started from is in the host layer's snapshot; it puts it back and
       * decodes the chunk again on the general path (the ids named so far stay in the table: that pass names them too) */
      const int32_t stNow = P.uttStatus[b] | (int32_t)S.scal[SL_STATUS] | ST_SELECT_FALLBACK;
      P.uttNextId[b] = (int32_t)S.scal[SL_NEXTID];
      P.uttStatus[b] = stNow;
      if (P.statusHost) {
        P.statusHost[b] = stNow;
      }
    }
  } else {
  const int pe = T & 1;
  const int ff = T + 1;
  if (wave == 0 && !dead) {
    const bool live = lane < nState;
    const SlRec me = S.rec[pe][live ? lane : 0];
    const double nb = live ? me.nb : NEG, bb = live ? me.b : NEG;
    const bool whichB = bb > nb;
    double m = whichB ? bb : nb;
    const uint32_t hp = whichB ? (me.info >> 24) : ((me.info >> 16) & 0xFFu);
    float fin = 0.0f;
    if constexpr (TL) {
      /* lm->finish(state) (KenLM.cpp:77-83: </s> in the state's context): both hypotheses of a state add the same term;
       * the best candidate of decodeEnd is a maximum again */
      int32_t cx[kWtCtx];
#pragma unroll
      for (int k = 0; k < kWtCtx; ++k) {
        cx[k] = S.ctx[pe][k][live ? lane : 0];
      }
      fin = P.lmOrder <= 3 ? ngScoreT<3>(P, cx, (uint32_t)P.lmEos, nullptr) : ngScoreT<kMaxNgramOrder>(P, cx, (uint32_t)P.lmEos, nullptr);
      m = m + U.lmW * (double)fin;
      const bool has = live && hp != kSlNoHyp && m == m;
      const unsigned long long k = waveMax64(has ? f64Key(m) : 0ull);
      endBest = k != 0ull ? f64FromKey(k) : 0.0;
    }
    if constexpr (LA && !TL) { /* the best candidate of decodeEnd is the best hypothesis of the final beam */
      endBest = f64FromKey(S.mmaxKey[pe]);
    }
    const double thr = endBest - P.beamThreshold;
    const bool ok = live && m >= thr && (!TL || hp != kSlNoHyp);
    if constexpr (LA) { /* the state's two hypotheses finish into one (LexiconFreeDecoder.cpp:127-158), best first */
      double lo = whichB ? nb : bb;
      if constexpr (TL) {
        lo = lo + U.lmW * (double)fin;
      }
      const uint32_t hl = whichB ? ((me.info >> 16) & 0xFFu) : (me.info >> 24);
      if (ok && hl != kSlNoHyp && lo >= thr) {
        m = slLogAdd(m, lo);
      }
    }
    const unsigned long long key = ok ? f64Key(m) : 0ull;
    int rank = 0;
    for (int i = 0; i < nState; ++i) {
      const uint32_t lo = waveReadLane32((uint32_t)key, i), hi = waveReadLane32((uint32_t)(key >> 32), i);
      const unsigned long long k2 = ((unsigned long long)hi << 32) | lo;
      const uint32_t h2 = waveReadLane32(hp, i);
      rank += (k2 > key || (k2 == key && h2 < hp)) ? 1 : 0;
    }
    const unsigned long long okMask = waveBallot(ok);
    if (ok) { /* at most K states hold a hypothesis, so every candidate above the threshold stays */
      const size_t g = ((size_t)b * K + rank) * 3;
      P.outScores[g + 0] = m;
      P.outScores[g + 1] = 0.0; /* emitting-model score: the back-trace kernel fills it in */
      P.outScores[g + 2] = 0.0; /* ZeroLM */
      if constexpr (TL) { /* LexiconFreeDecoder.cpp:146: prevHyp.lmScore + lmScore */
        P.outScores[g + 2] = (whichB ? S.lmB[pe][lane] : S.lmNB[pe][lane]) + (double)fin;
      }
      P.histPT[hbase + (int64_t)ff * K + rank] = make_int2((int)hp, P.sil);
    }
    if (lane == 0) {
      P.outN[b] = popc64(okMask);
      P.uttNBeam[b] = popc64(okMask);
      P.uttFrame[b] = ff;
      P.uttTotal[b] = ff;
      P.uttStatus[b] = ST_PACKED;
    }
  }
  if (dead && tid == 0) {
    P.outN[b] = 0;
    P.uttNBeam[b] = 0;
    P.uttFrame[b] = ff;
    P.uttTotal[b] = ff;
    P.uttStatus[b] = ST_SELECT_FALLBACK;
  }
  }
  if constexpr (TL) {
    if (U.prof) { /* marks 6 / 7: pairs | pairs the filter dropped << 32, look-ups | memo hits << 32 */
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (U.cnt[i] != 0u) {
          atomAdd32(&S.stat[i], U.cnt[i]);
        }
      }
      ldsBarrier();
      acc[6] = (unsigned long long)S.stat[0] | ((unsigned long long)S.stat[1] << 32);
      acc[7] = (unsigned long long)S.stat[2] | ((unsigned long long)S.stat[3] << 32);
    }
  }
  if (profMe) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      P.prof[(size_t)b * 8 + i] = acc[i];
    }
  }
}
