/*
 * tests/golden/lex_s2s_word_lm_rows_ref_driver.cpp -- runs the reference's LexiconSeq2SeqDecoder with isLmToken = false
 * (compiled from the unmodified flashlight/text sources by make_lex_s2s_word_lm_rows_golden.py, dev container only) and
 * an LM over WORDS that scores its whole vocabulary per state, as a word-level neural LM does: the fixtures of the
 * lexicon decoder's word-level rows LM.
 *
 * The model is s2s_ref_driver.cpp's: a pure function of (seed, token prefix), rows dropped with probability drop.  The
 * lexicon comes from a file of lines "label score tok tok ...", inserted in file order into Trie(V, 0) and smeared with
 * SmearingMode::MAX, so that lexMaxScore and the children's maxScore are not zero and the float subtractions of
 * LexiconSeq2SeqDecoder.cpp:146-198 matter.  The LM's state is the WORD prefix: a child<>(word) per score and a
 * child<>(-1) per finish, so two spellings of one word sequence meet in one state object, which is what candidatesStore
 * merges by.  Its answer for LM index i after a word prefix is lex_s2s_lm_rows_ref_driver.cpp's splitmix64 function of
 * (lm_seed, prefix, i), -(h >> 40) * 2^-20 (exact in float32), or -inf for one index in inf_mod; score(state, w) reads
 * index word_to_lm[w], finish reads finish_index.  make_s2s_lm_rows_golden.SmRowsLM over the word ids computes the
 * same floats.
 *
 * usage: lex_s2s_word_lm_rows_ref_driver seed V K Kt thr lmw word_score eos_score eos maxlen eos_bias drop log_add
 *        lexicon lm_seed W perm finish inf_mod junk n_words
 * (junk: bytes allocated and kept between model calls -- a different heap layout for the second run)
 * prints: one line per final hypothesis: score am lm (%.17g), then the tokens, "|", then the words.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <memory>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "flashlight/lib/text/decoder/LexiconSeq2SeqDecoder.h"
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
  uint64_t infMod;
  std::vector<int> usrToLm;
  float value(const std::vector<int>& prefix, int idx) const {
    uint64_t h = sm64(seed ^ 0x5DEECE66Dull);
    for (int tok : prefix) {
      h = sm64(h ^ (uint64_t)(tok + 1));
    }
    const uint64_t x = sm64(h ^ ((uint64_t)(idx + 1) * 0xD1B54A32D192ED03ull));
    if (infMod && sm64(x ^ 0xC0FFEEull) % infMod == 0) {
      return -std::numeric_limits<float>::infinity();
    }
    return -(float)((double)(x >> 40) * (1.0 / 1048576.0));
  }
  LMStatePtr start(bool) override { return std::make_shared<PrefixState>(); }
  /* (usrTokenIdx: a word id -- the decoder was made with isLmToken = false) */
  std::pair<LMStatePtr, float> score(const LMStatePtr& state, const int usrTokenIdx) override {
    auto in = std::static_pointer_cast<PrefixState>(state);
    auto out = in->child<PrefixState>(usrTokenIdx); /* (the existing child when there is one: lm/LM.h:24-34) */
    out->prefix = in->prefix;
    out->prefix.push_back(usrTokenIdx);
    return {out, value(in->prefix, usrToLm[(size_t)usrTokenIdx])};
  }
  std::pair<LMStatePtr, float> finish(const LMStatePtr& state) override {
    auto in = std::static_pointer_cast<PrefixState>(state);
    auto out = in->child<PrefixState>(-1);
    out->prefix = in->prefix;
    return {out, value(in->prefix, finishIdx)};
  }
};

int main(int argc, char** argv) {
  if (argc != 22) {
    fprintf(stderr, "usage: %s seed V K Kt thr lmw word_score eos_score eos maxlen eos_bias drop log_add lexicon "
                    "lm_seed W perm finish inf_mod junk n_words\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[1], nullptr, 10);
  const int V = atoi(argv[2]);
  LexiconSeq2SeqDecoderOptions opt;
  opt.beamSize = atoi(argv[3]);
  opt.beamSizeToken = atoi(argv[4]);
  opt.beamThreshold = atof(argv[5]);
  opt.lmWeight = atof(argv[6]);
  opt.wordScore = atof(argv[7]);
  opt.eosScore = atof(argv[8]);
  const int eos = atoi(argv[9]);
  const int maxlen = atoi(argv[10]);
  const float eosBias = (float)atof(argv[11]);
  const double drop = atof(argv[12]);
  opt.logAdd = atoi(argv[13]) != 0;
  const std::string lexPath = argv[14];
  auto lm = std::make_shared<RowsLM>();
  lm->seed = strtoull(argv[15], nullptr, 10);
  const int W = atoi(argv[16]);
  const uint64_t perm = strtoull(argv[17], nullptr, 10);
  const int finish = atoi(argv[18]);
  lm->infMod = strtoull(argv[19], nullptr, 10);
  const size_t junk = (size_t)atoll(argv[20]);
  const int nWords = atoi(argv[21]);
  std::vector<int> all((size_t)W);
  std::iota(all.begin(), all.end(), 0);
  if (perm) { /* the indices of [0, W) ordered by a hash: a permutation */
    std::stable_sort(all.begin(), all.end(), [&](int a, int b) {
      return sm64(perm ^ (uint64_t)(a + 1)) < sm64(perm ^ (uint64_t)(b + 1));
    });
  }
  lm->usrToLm.assign(all.begin(), all.begin() + nWords); /* word id -> LM index (W >= n_words) */
  lm->finishIdx = finish;
  auto trie = std::make_shared<Trie>(V, 0);
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
  trie->smear(SmearingMode::MAX);
  std::vector<std::unique_ptr<char[]>> keep;
  auto update = [&](const float*, const int, const int, const std::vector<int>& rawY, const std::vector<int>&,
                    const std::vector<EmittingModelStatePtr>& prev, int& t) {
    std::vector<std::vector<float>> out;
    std::vector<EmittingModelStatePtr> states;
    for (size_t r = 0; r < rawY.size(); ++r) {
      auto pre = std::make_shared<std::vector<int>>();
      if (t > 0) {
        *pre = *std::static_pointer_cast<std::vector<int>>(prev[r]);
        pre->push_back(rawY[r]);
      }
      uint64_t h = sm64(seed);
      for (int tok : *pre) {
        h = sm64(h ^ (uint64_t)(tok + 1));
      }
      std::vector<float> row((size_t)V);
      for (int v = 0; v < V; ++v) {
        const uint64_t x = sm64(h ^ ((uint64_t)(v + 1) * 0xD1B54A32D192ED03ull));
        row[v] = -(float)((double)(x >> 40) * (1.0 / 1048576.0));
        if (v == eos) {
          row[v] = row[v] + eosBias;
        }
      }
      const bool dropped = !pre->empty() && (double)(sm64(h ^ 0xA5A5A5A5ull) % 1000000ull) < drop * 1e6;
      out.push_back(std::move(row));
      states.push_back(dropped ? nullptr : EmittingModelStatePtr(pre));
      if (junk) {
        keep.emplace_back(new char[junk + 48 * (keep.size() % 7)]);
      }
    }
    return std::make_pair(out, states);
  };
  LexiconSeq2SeqDecoder dec(opt, trie, lm, eos, update, maxlen, false);
  std::vector<float> em(1, 0.0f);
  dec.decodeStep(em.data(), 1, V);
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
