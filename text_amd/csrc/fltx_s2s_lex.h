/*
 * fltx_s2s_lex.h -- the lexicon-constrained seq2seq beam search (LexiconSeq2SeqDecoder.cpp:20-202) as a batched
 * device step, beside the lexicon-free one of fltx_s2s.h (whose front end, LM helpers and selection it reuses).
 *
 * A step is two kernels, as there:
 *   fltx_s2s_tokbeam_kernel   one wave per live row: the row's exact token beam, its min(Kt, V) largest scores
 *                             (:94-112), taken before the trie filter (tokens that are no children still use slots);
 *   fltx_s2s_lex_step_kernel  one workgroup per utterance: every (row, token) of the records becomes up to 1 + labels
 *                             candidates (stay in the trie, end a word per label: :142-200; eos at the root: :115-141),
 *                             the finished hypotheses are carried (:68-83); then candidatesStore (Utils.h:146-225):
 *                             the threshold, the MERGE of candidates in one LM state, trie node and token, and the
 *                             sorted top K.
 * fltx_s2s_lex_end_kernel writes the n-best with words.
 *
 * Merging.  compareNoScoreStates (LexiconSeq2SeqDecoder.h:85-97) compares LM-state OBJECTS, and LMState::child hands
 * out the existing child (lm/LM.h:24-34), so two hypotheses in one state that end the same word, or two spellings of a
 * token string under a token LM, meet again.  A hypothesis carries a canonical state id `sid` and the (parent sid,
 * edge) pair its state was made by (edge: word / token id, -1 for KenLM's finish; the root is (-1, -1)).  child() is
 * injective, so a candidate's state is named without a lookup: (h.sid, e) when it moves to child(h, e), h's own pair
 * when it keeps h's state (smearing, ZeroLM's finish, a carried hypothesis).  Merge groups are found with a per-step
 * hash table over the survivors of the threshold; a group of two or more is folded by one thread in descending score
 * order (max, or logAdd's max + log1p(exp(min - max)) from the best), the best member's fields survive.  The <= K
 * survivors that enter a new state get a canonical id from the utterance's lookup-or-insert table in HBM, which lives
 * across steps (a state can be born again at a later step); a full table stops the utterance with ST_TABLE_FULL.
 *
 * LM rows.  With a rows LM (fltx_lm_rows_create, a token LM: isLmToken) the step is three kernels: the front end,
 * fltx_s2s_lm_rows_kernel (fltx_s2s.h, unchanged: one float per record entry into recLm -- usrToLm[token], the finish
 * index for eos) and fltx_s2s_lex_step_lm_rows_kernel, this step with its LM term read from recLm.  Where the LM term
 * comes from is a template parameter (REC) as in s2sStepUtteranceOn, so fltx_s2s_lex_step_kernel compiles to what it
 * was.  Under REC the token move, the word end (the first label) and eos of a record entry share its one LM entry and
 * all enter a new state: child(h.sid, token), or child(h.sid, -1) for eos (finish is its own child, as KenLM's) --
 * LexiconSeq2SeqDecoder.cpp:115-198 with isLmToken.  The LM's state is the token prefix, so two segmentations of one
 * token string carry the same (parent sid, edge) and merge by the keys above.  No n-gram walk: ctx stays ctx0.
 *
 * Word-level LM rows.  With a word rows LM (fltx_lm_word_rows_create: an LM over the lexicon's words, !isLmToken) the
 * step is the front end, fltx_s2s_lex_word_lm_rows_kernel and fltx_s2s_lex_step_word_lm_rows_kernel.  An LM row is as
 * wide as the word vocabulary, its state changes only where a word ends, and many hypotheses share one: the rows are
 * read through lmRowOf (decoder row -> LM row), and the gather reads only what the step can use -- per record entry
 * S = 1 + max labels floats recLm[row][e][s]: slot 0 the finish entry (eos at the root), slot s >= 1 the entry of label
 * s - 1 of the token's child, NaN where there is none.  The trie node of a row's hypothesis comes from rowNode, which
 * this step's instantiation leaves for the next call's rows (the root's 0 by fltx_s2s_begin).  The step (kS2lLmWordRows)
 * takes eos from slot 0 and a word end from slot s minus lexMaxScore (a float subtraction, :174-198); the move inside a
 * word reads no LM entry (smearing, the same state); states and merge keys are the tables path's -- child(h.sid, word),
 * child(h.sid, -1).  It also writes next_word: the word each listed row's hypothesis ended in this step, -1 for none.
 */
#pragma once

namespace fltx {

constexpr int kS2lMaxKt = 256;     /* min(beamSizeToken, V): the records' width */
constexpr int kS2lMaxLabels = 6;   /* kTrieMaxLabel (Trie.h:19) */
constexpr int kS2lDefaultStates = 1 << 16; /* LM states per utterance (fltx_s2s_lex_set_max_states) */

struct S2lHyp { /* one hypothesis of a beam, 72 B */
  double score, am, lm;
  int32_t token;  /* -1: the root */
  int32_t word;   /* -1: none */
  int32_t parent; /* index in the previous beam */
  int32_t node;   /* trie node (0: the root) */
  int32_t sid;    /* canonical LM state */
  int32_t psid, edge; /* the state is child(psid, edge); (-1, -1): LM::start */
  int32_t ctx[kS2sCtx];
};

struct S2lRec { /* a hypothesis' history record */
  int32_t token, word, parent, pad;
};

/* the compact trie: children sorted by token per node (CSR), labels per node */
struct S2lTrie {
  const float* maxScore;  /* [nNodes] */
  const int32_t* kidOff;  /* [nNodes + 1] */
  const int32_t* kidTok;  /* [nEdges] */
  const int32_t* kidNode; /* [nEdges] */
  const int32_t* labOff;  /* [nNodes + 1] */
  const int32_t* labels;  /* [nLabels] */
};

struct S2lParams {
  S2sParams s;          /* the lexicon-free fields: rows, records, front end, outputs */
  S2lTrie trie;
  int32_t isLmToken;
  int32_t S;            /* candidate slots per record entry: 1 + labels that can end a word */
  double wordScore;
  int32_t logAdd;
  S2lHyp* beam;         /* [2][B*K] */
  S2lRec* hist;         /* [maxOut + 1][B*K] */
  double* cScore;       /* [B][nC] */
  uint4* cMk;           /* [B][nC]: merge key (state pair, node, token) */
  int32_t *cGrp, *cList, *cNext; /* [B][nC] */
  int32_t* mTab;        /* [B][mSize]: per-step merge table (candidate index, -1 empty) */
  int32_t mSize;
  unsigned long long* sKey; /* [B][sSize]: (parent sid, edge) -> sid; ~0: empty */
  int32_t* sVal;
  int32_t* sCount;      /* [B] states handed out */
  int32_t sSize, sMax;
  int32_t* status;      /* [B] ST_* */
  int32_t* merges;      /* [B] candidates folded into another (all steps) */
  int32_t* words;       /* end: [B*K][len] */
};

FLTX_DEV uint64_t s2lMix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  return x ^ (x >> 33);
}

FLTX_DEV unsigned long long s2lPair(int32_t psid, int32_t edge) {
  return ((unsigned long long)(uint32_t)psid << 32) | (uint32_t)edge;
}

/* TrieNode::children.find (binary search over the sorted tokens); -1: no child */
FLTX_DEV int s2lChild(const S2lTrie& T, int node, int tok) {
  int lo = T.kidOff[node], hi = T.kidOff[node + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int t = T.kidTok[mid];
    if (t == tok) {
      return T.kidNode[mid];
    }
    if (t < tok) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return -1;
}

struct S2lCand {
  double score;
  float am, lmS;
  int32_t hyp;       /* index in the previous beam */
  int32_t token, word, node, src;
  int32_t newEdge;   /* the state is child(prev.sid, newEdge) when isNew */
  bool isNew;
  int32_t usr;       /* the LM question that made the state (kS2sLmFinish: finish) */
};

/* where a candidate's LM term comes from: a template parameter of the step, never a runtime flag */
enum { kS2lLmTables = 0,    /* ZeroLM / the n-gram tables (s2sLm) */
       kS2lLmTokenRows = 1, /* a token rows LM: recLm[r * cap + e] for all three kinds of candidate */
       kS2lLmWordRows = 2 };/* a word rows LM: recLm[(r * cap + e) * S + s] for eos (s = 0) and a word end (s >= 1) */

/* candidate j of the utterance: record slot j < nRowC (row k, entry e, sub-slot s: 0 = stay / eos, 1.. = the labels),
 * then the carried hypotheses; false: no candidate */
template <int SRC>
FLTX_DEV bool s2lCand(const S2lParams& Q, const float* recLm, const S2lHyp* prev, const int32_t* hypOfRow, int64_t rb,
                      int64_t nRowC, int64_t j, S2lCand& c) {
  const S2sParams& P = Q.s;
  if (j >= nRowC) {
    const int i = (int)(j - nRowC);
    const S2lHyp& h = prev[i];
    if (h.token != P.eos) {
      return false;
    }
    c.score = h.score;
    c.am = 0.0f;
    c.lmS = 0.0f;
    c.hyp = i;
    c.token = h.token;
    c.word = -1;
    c.node = h.node;
    c.src = -1;
    c.isNew = false;
    return true;
  }
  const int cap = P.cap, S = Q.S;
  const int k = (int)(j / ((int64_t)cap * S)), e = (int)((j / S) % cap), s = (int)(j % S);
  const int64_t r = rb + k;
  if (e >= P.recN[r]) {
    return false;
  }
  const int i = hypOfRow[k];
  const S2lHyp& h = prev[i];
  const int tok = P.recTok[r * cap + e];
  const float a = P.recAm[r * cap + e];
  c.am = a;
  c.hyp = i;
  c.token = tok;
  c.src = (int)r;
  if (tok == P.eos) { /* (1) eos, at the root only (:115-141): finish(state) -- a new child with n-gram tables, the
                       * same state with ZeroLM (lm/ZeroLM.cpp:24-25) */
    if (s != 0 || h.node != 0) {
      return false;
    }
    if constexpr (SRC == kS2lLmTokenRows) { /* LM::finish: the entry at the finish index, a child of its own */
      c.lmS = recLm[r * cap + e];
      c.isNew = true;
    } else if constexpr (SRC == kS2lLmWordRows) {
      c.lmS = recLm[(r * cap + e) * S] - 0.0f; /* (lexMaxScore is 0 at the root) */
      c.isNew = true;
    } else {
      c.lmS = s2sLm(P, h.ctx, kS2sLmFinish, kS2sLmFinish, nullptr) - 0.0f; /* (lexMaxScore is 0 at the root) */
      c.isNew = P.lmOn != 0;
    }
    c.score = (((h.score + (double)a) + P.eosScore) + P.lmWeight * (double)c.lmS);
    c.word = -1;
    c.node = 0;
    c.newEdge = -1;
    c.usr = kS2sLmFinish;
    return true;
  }
  const int child = s2lChild(Q.trie, h.node, tok); /* (2) a normal token: a child of the hypothesis' node */
  if (child < 0) {
    return false;
  }
  if constexpr (SRC == kS2lLmTokenRows) { /* a token LM: the move and the word end (the first label) share the entry and the new state */
    const int l0 = Q.trie.labOff[child];
    if (s > 1 || (s == 1 && Q.trie.labOff[child + 1] == l0)) {
      return false;
    }
    c.lmS = recLm[r * cap + e];
    c.isNew = true;
    c.newEdge = tok;
    c.usr = tok;
    c.word = s == 0 ? -1 : Q.trie.labels[l0];
    c.node = s == 0 ? child : 0;
    c.score = s == 0 ? (h.score + (double)a) + P.lmWeight * (double)c.lmS
                     : ((h.score + (double)a) + Q.wordScore) + P.lmWeight * (double)c.lmS;
    return true;
  }
  const float lexMax = h.node == 0 ? 0.0f : Q.trie.maxScore[h.node];
  if constexpr (SRC == kS2lLmWordRows) { /* a word LM: the move reads the trie alone, a word end its label's entry */
    if (s == 0) {
      c.lmS = Q.trie.maxScore[child] - lexMax; /* smearing (float) */
      c.isNew = false;
      c.score = (h.score + (double)a) + P.lmWeight * (double)c.lmS;
      c.word = -1;
      c.node = child;
      return true;
    }
    const int l0 = Q.trie.labOff[child];
    if (s - 1 >= Q.trie.labOff[child + 1] - l0) {
      return false;
    }
    const int word = Q.trie.labels[l0 + s - 1];
    c.lmS = recLm[(r * cap + e) * S + s] - lexMax;
    c.newEdge = word;
    c.usr = word;
    c.isNew = true;
    c.score = ((h.score + (double)a) + Q.wordScore) + P.lmWeight * (double)c.lmS;
    c.word = word;
    c.node = 0;
    return true;
  }
  if (s == 0) { /* stay in the trie (:146-171) */
    if (Q.isLmToken) {
      c.lmS = s2sLm(P, h.ctx, tok, kS2sLmFinish, nullptr);
      c.isNew = true;
      c.newEdge = tok;
      c.usr = tok;
    } else {
      c.lmS = Q.trie.maxScore[child] - lexMax; /* smearing (float) */
      c.isNew = false;
    }
    c.score = (h.score + (double)a) + P.lmWeight * (double)c.lmS;
    c.word = -1;
    c.node = child;
    return true;
  }
  /* end a word: label s - 1 (:174-198; a token LM: the first label only, with the token's state and score) */
  const int l0 = Q.trie.labOff[child], nl = Q.trie.labOff[child + 1] - l0;
  if (s - 1 >= nl || (Q.isLmToken && s > 1)) {
    return false;
  }
  const int word = Q.trie.labels[l0 + s - 1];
  if (Q.isLmToken) {
    c.lmS = s2sLm(P, h.ctx, tok, kS2sLmFinish, nullptr);
    c.newEdge = tok;
    c.usr = tok;
  } else {
    c.lmS = s2sLm(P, h.ctx, word, kS2sLmFinish, nullptr) - lexMax;
    c.newEdge = word;
    c.usr = word;
  }
  c.isNew = true;
  c.score = ((h.score + (double)a) + Q.wordScore) + P.lmWeight * (double)c.lmS;
  c.word = word;
  c.node = 0;
  return true;
}

/* the merge key: (the state's (parent sid, edge), trie node, token) */
FLTX_DEV uint4 s2lMergeKey(const S2lCand& c, const S2lHyp& h) {
  const unsigned long long st = c.isNew ? s2lPair(h.sid, c.newEdge) : s2lPair(h.psid, h.edge);
  return make_uint4((uint32_t)(st >> 32), (uint32_t)st, (uint32_t)c.node, (uint32_t)c.token);
}

FLTX_DEV bool s2lSameKey(uint4 a, uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

/* the order of a group's fold: score descending, ties to the lower candidate index */
FLTX_DEV bool s2lBefore(double sa, int64_t ja, double sb, int64_t jb) { return sa > sb || (sa == sb && ja < jb); }

struct S2lStepLds {
  S2sStepLds s;
  int32_t full;
};

/* what the word-rows step leaves per row of the next call: next_word and the row's trie node (the gather's) */
struct S2lRowExtra {
  int32_t *outWord, *rowNode;
  int32_t word, node;
  __device__ __forceinline__ void put(int64_t r) const {
    outWord[r] = word;
    rowNode[r] = node;
  }
  __device__ __forceinline__ void none(int64_t r) const { outWord[r] = -1; }
};

FLTX_DEV void s2lNoWords(const S2sParams& P, int b, int32_t* outWord) {
  for (int k = (int)threadIdx.x; k < P.K; k += kS2sStepThreads) {
    outWord[(int64_t)b * P.K + k] = -1;
  }
}

/* outWord / rowNode: kS2lLmWordRows only */
template <int SRC>
FLTX_DEV void s2lStepUtteranceOn(const S2lParams& Q, char* smem, const float* recLm, int32_t* outWord = nullptr,
                                 int32_t* rowNode = nullptr) {
  const S2sParams& P = Q.s;
  S2lStepLds& L = *(S2lStepLds*)smem;
  S2sStepLds& S = L.s;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int K = P.K;
  const int64_t rb = (int64_t)b * K;
  if (P.done[b]) { /* a step after the last one, a parked slot: nothing to score */
    s2sIdleStep(P, b);
    if constexpr (SRC == kS2lLmWordRows) {
      s2lNoWords(P, b, outWord);
    }
    return;
  }
  const int par = P.t & 1;
  const S2lHyp* prev = Q.beam + (size_t)par * P.B * K + rb;
  S2lHyp* next = Q.beam + (size_t)(par ^ 1) * P.B * K + rb;
  const int nPrev = P.beamN[par * P.B + b];
  const int nRows = P.nRowsInt[b];
  /* 1. rows <-> hypotheses (the live ones in beam order: :42-52) */
  if (tid == 0) {
    L.full = 0;
  }
  s2sMapRows(S, prev, nPrev, P.eos);
  /* 2. the candidates: order keys, scores, merge keys; the best of the step */
  const size_t cb = (size_t)b * P.nC;
  unsigned long long* cKey = P.cKey + cb;
  double* cScore = Q.cScore + cb;
  uint4* cMk = Q.cMk + cb;
  int32_t* cGrp = Q.cGrp + cb;
  int32_t* cList = Q.cList + cb;
  int32_t* cNext = Q.cNext + cb;
  int32_t* mTab = Q.mTab + (size_t)b * Q.mSize;
  const int64_t nRowC = (int64_t)nRows * P.cap * Q.S, n = nRowC + nPrev;
  for (int j = tid; j < Q.mSize; j += kS2sStepThreads) {
    mTab[j] = -1;
  }
  unsigned long long mx = 0ull;
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    unsigned long long key = 0ull;
    S2lCand c;
    if (s2lCand<SRC>(Q, recLm, prev, S.hypOfRow, rb, nRowC, j, c)) {
      key = s2sScoreKey(c.score);
      cScore[j] = c.score;
      cMk[j] = s2lMergeKey(c, prev[c.hyp]);
    }
    cKey[j] = key;
    mx = key > mx ? key : mx;
  }
  /* 3. threshold (candidatesStore step 1: score >= best - beamThreshold) */
  const unsigned long long thrKey = s2sThresholdKey(s2sBlockMaxKey(S, mx), P.beamThreshold);
  /* 4. merge (step 2): the first survivor of a key to claim its slot heads the group, the others join its list */
  const uint32_t mMask = (uint32_t)Q.mSize - 1u;
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
      acc = Q.logAdd ? hi + log1p(exp(lo - hi)) : hi;
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
  __threadfence();
  int surv = 0;
  __syncthreads();
  for (int64_t j = tid; j < n; j += kS2sStepThreads) {
    surv += cKey[j] != 0ull ? 1 : 0;
  }
  const int nSurv = s2sBlockSum(S.wcnt, surv);
  nMerged = s2sBlockSum(S.wcnt, nMerged);
  /* 5. the K best, sorted best first */
  const int nSel = s2sSelectTopK(S, cKey, n, K, nSurv);
  /* 6. the new beam; survivors that enter a new state look it up (or insert it) in the utterance's state table */
  S2lHyp nh;
  S2lCand c;
  bool isLive = false, claimed = false, hasNew = false;
  int token = -1, parent = -1, srcRow = -1;
  uint32_t sslot = 0u;
  unsigned long long skey = 0ull;
  unsigned long long* sKey = Q.sKey + (size_t)b * Q.sSize;
  int32_t* sVal = Q.sVal + (size_t)b * Q.sSize;
  if (tid < nSel) {
    const int64_t j = S.selIdx[S.order[tid]];
    s2lCand<SRC>(Q, recLm, prev, S.hypOfRow, rb, nRowC, j, c);
    const S2lHyp& h = prev[c.hyp];
    nh = h;
    nh.parent = c.hyp;
    nh.score = cScore[j];
    if (j < nRowC) {
      nh.am = h.am + (double)c.am;
      nh.lm = h.lm + (double)c.lmS;
      nh.token = c.token;
      nh.word = c.word;
      nh.node = c.node;
      if (c.isNew) {
        nh.psid = h.sid;
        nh.edge = c.newEdge;
        if constexpr (SRC == kS2lLmTables) {
          if (P.lmOn) {
            (void)s2sLm(P, h.ctx, c.usr, kS2sLmFinish, nh.ctx);
          }
        }
        skey = s2lPair(nh.psid, nh.edge);
        hasNew = true;
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
      isLive = c.token != P.eos;
    } else {
      nh.word = -1;
    }
  }
  __syncthreads();
  if (claimed) {
    const int32_t v = (int32_t)atomAdd32((uint32_t*)&Q.sCount[b], 1u);
    if (v >= Q.sMax) {
      L.full = 1;
    }
    sVal[sslot] = v;
  }
  __threadfence();
  __syncthreads();
  if (L.full) { /* the state table is full: the utterance stops, its status says so (never a silent wrong merge) */
    s2sIdleStep(P, b);
    if constexpr (SRC == kS2lLmWordRows) {
      s2lNoWords(P, b, outWord);
    }
    if (tid == 0) {
      Q.status[b] |= ST_TABLE_FULL;
      P.nRowsInt[b] = 0;
      P.done[b] = 1;
      P.finalStep[b] = s2sLocalT(P, b);
    }
    return;
  }
  const int lt = s2sLocalT(P, b); /* (loaded here, where the step first needs it: not kept across the search) */
  if (tid < nSel) {
    if (hasNew) {
      nh.sid = (int32_t)loadCoherent32((const uint32_t*)&sVal[sslot]);
    }
    next[tid] = nh;
    {
      S2lRec rec;
      rec.token = nh.token;
      rec.word = nh.word;
      rec.parent = nh.parent;
      rec.pad = 0;
      Q.hist[(size_t)(lt + 1) * P.B * K + rb + tid] = rec;
    }
    token = nh.token;
    parent = nh.parent;
    srcRow = c.src;
  }
  if (tid == 0) {
    Q.merges[b] += nMerged;
  }
  if constexpr (SRC == kS2lLmWordRows) {
    s2sPublishStepWith(P, S, b, lt, nSel, isLive, token, parent, srcRow,
                       S2lRowExtra{outWord, rowNode, nh.word, nh.node});
  } else {
    s2sPublishStep(P, S, b, lt, nSel, isLive, token, parent, srcRow);
  }
}

FLTX_DEV void s2lStepUtterance(const S2lParams& Q, char* smem) {
  s2lStepUtteranceOn<kS2lLmTables>(Q, smem, nullptr);
}

/* the step with the LM term from the records (a rows LM) */
struct S2lLmRowsParams {
  S2lParams q;
  const float* recLm; /* [B*K][cap], as fltx_s2s_lm_rows_kernel gathered it */
};

FLTX_DEV void s2lStepUtteranceLmRows(const S2lLmRowsParams& R, char* smem) {
  s2lStepUtteranceOn<kS2lLmTokenRows>(R.q, smem, R.recLm);
}

/* ---- word-level LM rows (fltx_lm_word_rows_create) ------------------------------------------------------------------
 * the gather: for every entry of a live row's record the S floats the step can read (see the head of this file).
 *   log-probs: one wave per row, four rows per workgroup, lanes over the record's entries: <= cap * S elements of the
 *              LM row are read, whatever its width;
 *   logits:    one workgroup per decoder row: s2sLmRowLse (fltx_s2s.h: the same max / sum passes, summation order and
 *              widening; rows wider than the register cache re-read per pass) over the LM row lmRowOf names, then the
 *              same gather.  A shared LM row has its lse computed once per decoder row that names it -- the same bits
 *              every time; the duplicated reads are the price of one launch without a row-level dependency.
 * Every index is formed in 64 bits from a row number and a stride; an element index is an int below the width (at most
 * kS2lMaxLmWidth).  A decoder row whose lmRowOf entry lies outside [0, nLmRows) reads nothing: its slots are NaN. */
constexpr int kS2lMaxLmWidth = 1 << 22;

struct S2lWordLmParams {
  S2sLmRowsParams r;      /* r.s: the step's lexicon-free view; r.x / rowStride / width / finishIdx / rowLse: the LM's
                           * rows; r.usrToLm: word id -> LM index (null: identity); r.recLm: [B*K][cap][S] */
  S2lTrie trie;
  const int32_t* rowNode; /* [B*K]: the trie node of each row's hypothesis */
  const int32_t* lmRowOf; /* [B*K] or null (identity): the LM row of each decoder row */
  int32_t nLmRows;
  int32_t S;
};

/* the LM row of decoder row r; null: none */
template <int DT>
FLTX_DEV const void* s2lWordLmRow(const S2lWordLmParams& W, int64_t r) {
  const int64_t lr = W.lmRowOf ? (int64_t)W.lmRowOf[r] : r;
  if (lr < 0 || lr >= (int64_t)W.nLmRows) {
    return nullptr;
  }
  return (const char*)W.r.x + lr * W.r.rowStride * (DT == kS2sDtF32 ? 4 : 2);
}

template <int DT, bool LOGITS>
FLTX_DEV void s2lWordLmGather(const S2lWordLmParams& W, int64_t r, const void* row, double lse, int tid, int nThreads) {
  const S2sLmRowsParams& Q = W.r;
  const S2sParams& P = Q.s;
  const int n = P.recN[r], S = W.S;
  const int node = W.rowNode[r];
  for (int e = tid; e < n; e += nThreads) {
    const int tok = P.recTok[r * P.cap + e];
    float* out = Q.recLm + (r * P.cap + e) * S;
    int l0 = 0, nl = 0;
    bool fin = false;
    if (tok == P.eos) {
      fin = node == 0;
    } else {
      const int child = s2lChild(W.trie, node, tok);
      if (child >= 0) {
        l0 = W.trie.labOff[child];
        nl = W.trie.labOff[child + 1] - l0;
      }
    }
    for (int s = 0; s < S; ++s) {
      int idx = -1;
      if (s == 0) {
        idx = fin ? Q.finishIdx : -1;
      } else if (s - 1 < nl) {
        const int word = W.trie.labels[l0 + s - 1];
        idx = Q.usrToLm ? Q.usrToLm[word] : word;
      }
      float v = __uint_as_float(0x7FC00000u);
      if (row != nullptr && idx >= 0 && idx < Q.width) {
        v = s2sTypedScore<DT, LOGITS>(row, idx, lse);
      }
      out[s] = v;
    }
  }
}

template <int DT, bool LOGITS>
FLTX_DEV void s2lWordLmRows(const S2lWordLmParams& W, char* smem) {
  const S2sLmRowsParams& Q = W.r;
  const S2sParams& P = Q.s;
  if constexpr (!LOGITS) { /* workgroup = four waves, wave = row b*K + k of the step */
    const int wave = waveUniform(waveId());
    const int64_t r = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
    if (r >= (int64_t)P.B * P.K || !s2sRowLive(P, r)) {
      return; /* (the record of a row that is not live is empty: the step reads no recLm of it) */
    }
    s2lWordLmGather<DT, false>(W, r, s2lWordLmRow<DT>(W, r), 0.0, laneId(), 64);
  } else { /* workgroup = row b*K + k of the step */
    const int64_t r = (int64_t)blockIdx.x;
    const void* row = s2sRowLive(P, r) ? s2lWordLmRow<DT>(W, r) : nullptr;
    if (row == nullptr) {
      if (threadIdx.x == 0 && Q.rowLse) {
        Q.rowLse[r] = __longlong_as_double(0x7FF8000000000000ll);
      }
      if (s2sRowLive(P, r)) {
        s2lWordLmGather<DT, true>(W, r, nullptr, 0.0, (int)threadIdx.x, kS2sLmThreads);
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
    s2lWordLmGather<DT, true>(W, r, row, lse, (int)threadIdx.x, kS2sLmThreads);
  }
}

/* the step with the LM term from the word-level records; it also lists next_word and leaves rowNode */
struct S2lWordLmStepParams {
  S2lParams q;
  const float* recLm; /* [B*K][cap][S], as fltx_s2s_lex_word_lm_rows_kernel gathered it */
  int32_t* outWord;   /* [B*K]: the caller's next_word */
  int32_t* rowNode;   /* [B*K] */
};

FLTX_DEV void s2lStepUtteranceWordLmRows(const S2lWordLmStepParams& R, char* smem) {
  s2lStepUtteranceOn<kS2lLmWordRows>(R.q, smem, R.recLm, R.outWord, R.rowNode);
}

/* decodeStep's start (:29-31): the root in LM::start's state (sid 0) at the trie's root */
FLTX_DEV void s2lBeginUtterance(const S2lParams& Q, char*) {
  const S2sParams& P = Q.s;
  const int b = (int)(blockIdx.x * kS2sBeginThreads + threadIdx.x);
  if (b >= P.B) {
    return;
  }
  S2lHyp h;
  s2sRootHyp(P, h);
  h.word = -1;
  h.node = 0;
  h.sid = 0;
  h.psid = -1;
  h.edge = -1;
  Q.beam[(int64_t)b * P.K] = h;
  Q.sCount[b] = 1;
  Q.status[b] = 0;
  Q.merges[b] = 0;
  s2sBeginReset(P, b);
}

struct S2lPath { /* a path's records: the tokens row and the words row */
  int32_t *tokens, *words;
  __device__ __forceinline__ void none(int64_t at) const {
    tokens[at] = -1;
    words[at] = -1;
  }
  __device__ __forceinline__ int put(int64_t at, S2lRec rec) const {
    tokens[at] = rec.token;
    words[at] = rec.word;
    return rec.parent;
  }
};

/* getAllFinalHypothesis (:209-211, Utils.h:230-266): tokens and words of the final beam's paths */
FLTX_DEV void s2lEndUtterance(const S2lParams& Q, char*) {
  s2sBackTrace(Q.s, Q.beam, Q.hist, S2lPath{Q.s.tokens, Q.words}, Q.status[blockIdx.x]);
}

/* fltx_s2s_finish (s2sFinishSlot) on the lexicon kind: a restarted slot also gets back what s2lBeginUtterance and
 * fltx_s2s_begin's memsets leave -- the utterance's state table empty (cleared only when a state was ever inserted:
 * every insert counts in sCount), the count started over, status and merges cleared, and with a word rows LM the trie
 * node of the listed root row at the root.  Word rows: a row listed again keeps its rowNode, next_word is its
 * hypothesis' word, as the last step listed it */
struct S2lFinishKind {
  S2lParams q;
  int32_t *outWord, *rowNode; /* null unless a word rows LM */
  bool dirty;                 /* the slot's state table holds entries */
  __device__ __forceinline__ void root(const S2sParams& P, S2lHyp& h) const {
    s2sRootHyp(P, h);
    h.word = -1;
    h.node = 0;
    h.sid = 0;
    h.psid = -1;
    h.edge = -1;
  }
  __device__ __forceinline__ void restart(int b) const {
    const int tid = (int)threadIdx.x;
    if (dirty) {
      uint4* tab = (uint4*)(q.sKey + (size_t)b * q.sSize); /* (sSize: a power of two >= 2, 8 bytes an entry) */
      for (int i = tid; i < q.sSize / 2; i += kS2sEndThreads) {
        tab[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
      }
    }
    if (tid == 0) {
      q.sCount[b] = 1;
      q.status[b] = 0;
      q.merges[b] = 0;
      if (rowNode) {
        rowNode[(int64_t)b * q.s.K] = 0;
      }
    }
  }
  __device__ __forceinline__ void park(int b) const {
    if (threadIdx.x == 0) {
      q.status[b] = 0;
      q.merges[b] = 0;
    }
  }
  __device__ __forceinline__ void listed(int64_t r, const S2lHyp& h) const {
    if (outWord) {
      outWord[r] = h.word;
    }
  }
  __device__ __forceinline__ void padding(int64_t r) const {
    if (outWord) {
      outWord[r] = -1;
    }
  }
};

struct S2lFinishKernelParams {
  S2lParams q;
  S2sFinishParams f;
  int32_t *outWord, *rowNode;
};

FLTX_DEV void s2lFinishUtterance(const S2lFinishKernelParams& Z, char* smem) {
  const S2lParams& Q = Z.q;
  const int b = (int)blockIdx.x;
  const int st = Q.status[b]; /* (read, like sCount, before the barrier behind which a restart clears them) */
  const int status = (st & (ST_CAND_OVERFLOW | ST_TABLE_FULL | ST_SELECT_FALLBACK)) ? Z.f.errUnsupported : 0;
  s2sFinishSlot(Q.s, Z.f, *(S2sFinishLds*)smem, Q.beam, Q.hist, S2lPath{Q.s.tokens, Q.words}, status,
                S2lFinishKind{Q, Z.outWord, Z.rowNode, Q.sCount[b] != 1});
}

} // namespace fltx
