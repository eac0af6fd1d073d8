/*
 * tests/golden/lex_s2s_ref_driver.cpp -- runs the reference's LexiconSeq2SeqDecoder (compiled from the unmodified
 * flashlight/text sources by make_lex_s2s_golden.py, dev container only) on the synthetic model of the seq2seq
 * fixtures (s2s_ref_driver.cpp's: a pure function of (seed, token prefix), rows dropped with probability drop).
 *
 * The lexicon comes from a file of lines "label score tok tok ...", inserted in file order into Trie(V, 0) and smeared
 * with the given mode.  An n-gram case scores with an LM subclass over oracle/arpa_lm.h's ArpaModel whose states are
 * LMState::child objects (one per (state, id), as KenLM's are: lm/KenLM.cpp:63-83); user id i is the LM word
 * "<prefix><i>" (w: words, t: tokens with is_lm_token).
 *
 * usage: lex_s2s_ref_driver seed V K Kt thr lmw word_score eos_score eos maxlen eos_bias drop log_add is_lm_token
 *                           lexicon smear arpa|- prefix junk
 * prints: one line per final hypothesis: score am lm (%.17g), then the tokens, "|", then the words.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "flashlight/lib/text/decoder/LexiconSeq2SeqDecoder.h"
#include "flashlight/lib/text/decoder/Trie.h"
#include "flashlight/lib/text/decoder/lm/ZeroLM.h"
#include "arpa_lm.h"

using namespace fl::lib::text;

static uint64_t sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct ArpaState : LMState {
  std::vector<int32_t> ctx;
};

struct ArpaLM : LM {
  orc::ArpaModel m;
  std::string prefix;
  ArpaLM(const std::string& path, const std::string& pre) : prefix(pre) { m.load(path); }
  int32_t word(int usr) const { return m.index(prefix + std::to_string(usr)); }
  LMStatePtr start(bool startWithNothing) override {
    auto s = std::make_shared<ArpaState>();
    if (!startWithNothing) {
      s->ctx.push_back(m.bos);
    }
    return s;
  }
  std::pair<LMStatePtr, float> score(const LMStatePtr& state, const int usrTokenIdx) override {
    auto in = std::static_pointer_cast<ArpaState>(state);
    auto out = in->child<ArpaState>(usrTokenIdx);
    out->ctx.clear();
    const float p = m.score(in->ctx, word(usrTokenIdx), out->ctx);
    return {out, p};
  }
  std::pair<LMStatePtr, float> finish(const LMStatePtr& state) override {
    auto in = std::static_pointer_cast<ArpaState>(state);
    auto out = in->child<ArpaState>(-1);
    out->ctx.clear();
    const float p = m.score(in->ctx, m.eos, out->ctx);
    return {out, p};
  }
};

int main(int argc, char** argv) {
  if (argc != 20) {
    fprintf(stderr, "usage: %s seed V K Kt thr lmw word_score eos_score eos maxlen eos_bias drop log_add is_lm_token "
                    "lexicon smear arpa|- prefix junk\n", argv[0]);
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
  const bool isLmToken = atoi(argv[14]) != 0;
  const std::string lexPath = argv[15];
  const int smear = atoi(argv[16]);
  const std::string arpa = argv[17];
  const std::string prefix = argv[18];
  const size_t junk = (size_t)atoll(argv[19]);
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
  trie->smear(smear == 0 ? SmearingMode::NONE : smear == 1 ? SmearingMode::MAX : SmearingMode::LOGADD);
  LMPtr lm;
  if (arpa == "-") {
    lm = std::make_shared<ZeroLM>();
  } else {
    lm = std::make_shared<ArpaLM>(arpa, prefix);
  }
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
  LexiconSeq2SeqDecoder dec(opt, trie, lm, eos, update, maxlen, isLmToken);
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
