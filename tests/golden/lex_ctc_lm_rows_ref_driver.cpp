/*
 * tests/golden/lex_ctc_lm_rows_ref_driver.cpp -- runs the reference's LexiconDecoder (CTC; compiled from the unmodified
 * flashlight/text sources by make_lex_ctc_lm_rows_golden.py into oracle/_ref/, dev container only) with an LM that scores
 * a whole vocabulary per state, as a neural LM does: the fixtures of the lexicon CTC rows decoder.
 *
 * The LM is ctc_lm_rows_ref_driver.cpp's prefix-hash LM: its state is a child<>() per edge that holds the prefix of edges
 * (word ids with is_lm_token = 0, tokens with is_lm_token = 1); its answer for LM index i after a prefix is a splitmix64
 * function of (lm_seed, prefix, i) mapped to -(h >> 40) * 2^-20 (exact in float32).  score(state, u) reads index
 * usr_to_lm[u] -- the identity, or (perm != 0) the first n_map entries of a permutation of [0, W) -- and finish reads
 * finish_index.  The emissions are a splitmix64 function of (seed, frame, token) with the same mapping, times 1/4.  The
 * lexicon comes from a file of lines "label score tok tok ...", inserted in file order into Trie(N, sil) and smeared with
 * MAX when smear != 0.
 *
 * usage: lex_ctc_lm_rows_ref_driver seed T N K Kt thr lmw word_score unk_score sil_score sil blank unk log_add is_lm_token
 *        lexicon lm_seed W perm finish n_map smear junk
 * (junk: bytes allocated and kept per LM call -- a different heap layout for the second run)
 * prints: one line per final hypothesis: score am lm (%.17g), the tokens, " | ", the words.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "flashlight/lib/text/decoder/LexiconDecoder.h"
#include "flashlight/lib/text/decoder/Trie.h"

using namespace fl::lib::text;

static uint64_t sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct PrefixState : LMState {
  std::vector<int> prefix;
};

struct RowsLM : LM {
  uint64_t seed;
  int finishIdx;
  size_t junk;
  std::vector<int> usrToLm;
  std::vector<std::unique_ptr<char[]>> keep;
  float value(const std::vector<int>& prefix, int idx) {
    if (junk) {
      keep.emplace_back(new char[junk + 48 * (keep.size() % 7)]);
    }
    uint64_t h = sm64(seed ^ 0x5DEECE66Dull);
    for (int edge : prefix) {
      h = sm64(h ^ (uint64_t)(edge + 1));
    }
    const uint64_t x = sm64(h ^ ((uint64_t)(idx + 1) * 0xD1B54A32D192ED03ull));
    return -(float)((double)(x >> 40) * (1.0 / 1048576.0));
  }
  LMStatePtr start(bool) override { return std::make_shared<PrefixState>(); }
  std::pair<LMStatePtr, float> score(const LMStatePtr& state, const int usrIdx) override {
    auto in = std::static_pointer_cast<PrefixState>(state);
    auto out = in->child<PrefixState>(usrIdx); /* (the existing child when there is one: lm/LM.h:24-34) */
    out->prefix = in->prefix;
    out->prefix.push_back(usrIdx);
    return {out, value(in->prefix, usrToLm[(size_t)usrIdx])};
  }
  std::pair<LMStatePtr, float> finish(const LMStatePtr& state) override {
    auto in = std::static_pointer_cast<PrefixState>(state);
    auto out = in->child<PrefixState>(-1);
    out->prefix = in->prefix;
    return {out, value(in->prefix, finishIdx)};
  }
};

int main(int argc, char** argv) {
  if (argc != 24) {
    fprintf(stderr, "usage: %s seed T N K Kt thr lmw word_score unk_score sil_score sil blank unk log_add is_lm_token "
                    "lexicon lm_seed W perm finish n_map smear junk\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[1], nullptr, 10);
  const int T = atoi(argv[2]), N = atoi(argv[3]);
  LexiconDecoderOptions opt;
  opt.beamSize = atoi(argv[4]);
  opt.beamSizeToken = atoi(argv[5]);
  opt.beamThreshold = atof(argv[6]);
  opt.lmWeight = atof(argv[7]);
  opt.wordScore = atof(argv[8]);
  opt.unkScore = atof(argv[9]); /* ("-inf": off) */
  opt.silScore = atof(argv[10]);
  const int sil = atoi(argv[11]), blank = atoi(argv[12]), unk = atoi(argv[13]);
  opt.logAdd = atoi(argv[14]) != 0;
  opt.criterionType = CriterionType::CTC;
  const bool isLmToken = atoi(argv[15]) != 0;
  const std::string lexPath = argv[16];
  auto lm = std::make_shared<RowsLM>();
  lm->seed = strtoull(argv[17], nullptr, 10);
  const int W = atoi(argv[18]);
  const uint64_t perm = strtoull(argv[19], nullptr, 10);
  lm->finishIdx = atoi(argv[20]);
  const int nMap = atoi(argv[21]);
  const bool smear = atoi(argv[22]) != 0;
  lm->junk = (size_t)atoll(argv[23]);
  std::vector<int> all((size_t)W);
  std::iota(all.begin(), all.end(), 0);
  if (perm) { /* the indices of [0, W) ordered by a hash: a permutation */
    std::stable_sort(all.begin(), all.end(), [&](int a, int b) {
      return sm64(perm ^ (uint64_t)(a + 1)) < sm64(perm ^ (uint64_t)(b + 1));
    });
  }
  lm->usrToLm.assign(all.begin(), all.begin() + nMap); /* (W >= n_map) */
  auto trie = std::make_shared<Trie>(N, sil);
  {
    std::ifstream f(lexPath);
    std::string line;
    while (std::getline(f, line)) {
      std::istringstream ss(line);
      int label;
      float score;
      ss >> label >> score;
      std::vector<int> toks;
      int t;
      while (ss >> t) {
        toks.push_back(t);
      }
      trie->insert(toks, label, score);
    }
  }
  if (smear) {
    trie->smear(SmearingMode::MAX);
  }
  std::vector<float> em((size_t)T * N);
  for (int t = 0; t < T; ++t) {
    const uint64_t h = sm64(sm64(seed) ^ (uint64_t)(t + 1));
    for (int n = 0; n < N; ++n) {
      const uint64_t x = sm64(h ^ ((uint64_t)(n + 1) * 0xD1B54A32D192ED03ull));
      em[(size_t)t * N + n] = -(float)((double)(x >> 40) * (1.0 / 1048576.0)) * 0.25f;
    }
  }
  LexiconDecoder dec(opt, trie, lm, sil, blank, unk, {}, isLmToken);
  dec.decodeBegin();
  dec.decodeStep(em.data(), T, N);
  dec.decodeEnd();
  for (const auto& r : dec.getAllFinalHypothesis()) {
    printf("%.17g %.17g %.17g", r.score, r.emittingModelScore, r.lmScore);
    for (int tok : r.tokens) {
      printf(" %d", tok);
    }
    printf(" |");
    for (int w : r.words) {
      printf(" %d", w);
    }
    printf("\n");
  }
  return 0;
}
