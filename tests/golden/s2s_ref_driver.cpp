/*
 * tests/golden/s2s_ref_driver.cpp -- runs the reference's LexiconFreeSeq2SeqDecoder (compiled from the unmodified
 * flashlight/text sources by make_s2s_golden.py, dev container only) on the synthetic model of the seq2seq fixtures.
 *
 * The model is a pure function of (seed, token prefix): a splitmix64 chain over the seed and the prefix, then one
 * draw per token v mapped to -(h >> 40) * 2^-20 (exact in float32; make_s2s_golden.SmModel computes the same floats),
 * eos_bias added to eos's score, and a row dropped (null state) with probability drop for every non-root prefix.
 * An n-gram case scores with an LM subclass over oracle/arpa_lm.h's ArpaModel whose states are a new child per token,
 * as KenLM's are (lm/KenLM.cpp:63-83); user token i is the LM word "t<i>".
 *
 * usage: s2s_ref_driver seed V K Kt thr lmw eos_score eos maxlen eos_bias drop log_add arpa|- junk
 * (junk: bytes allocated and kept between model calls -- a different heap layout for the second run)
 * prints: one line per final hypothesis: score am lm (%.17g) then the tokens.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "flashlight/lib/text/decoder/LexiconFreeSeq2SeqDecoder.h"
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
  explicit ArpaLM(const std::string& path) { m.load(path); }
  int32_t word(int usr) const { return m.index("t" + std::to_string(usr)); }
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
    const float p = m.score(in->ctx, word(usrTokenIdx), out->ctx);
    return {out, p};
  }
  std::pair<LMStatePtr, float> finish(const LMStatePtr& state) override {
    auto in = std::static_pointer_cast<ArpaState>(state);
    auto out = in->child<ArpaState>(-1);
    const float p = m.score(in->ctx, m.eos, out->ctx);
    return {out, p};
  }
};

int main(int argc, char** argv) {
  if (argc != 15) {
    fprintf(stderr, "usage: %s seed V K Kt thr lmw eos_score eos maxlen eos_bias drop log_add arpa|- junk\n", argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[1], nullptr, 10);
  const int V = atoi(argv[2]);
  LexiconFreeSeq2SeqDecoderOptions opt;
  opt.beamSize = atoi(argv[3]);
  opt.beamSizeToken = atoi(argv[4]);
  opt.beamThreshold = atof(argv[5]);
  opt.lmWeight = atof(argv[6]);
  opt.eosScore = atof(argv[7]);
  const int eos = atoi(argv[8]);
  const int maxlen = atoi(argv[9]);
  const float eosBias = (float)atof(argv[10]);
  const double drop = atof(argv[11]);
  opt.logAdd = atoi(argv[12]) != 0;
  const std::string arpa = argv[13];
  const size_t junk = (size_t)atoll(argv[14]);
  LMPtr lm;
  if (arpa == "-") {
    lm = std::make_shared<ZeroLM>();
  } else {
    lm = std::make_shared<ArpaLM>(arpa);
  }
  std::vector<std::unique_ptr<char[]>> keep;
  auto update = [&](const float*, const int, const int, const std::vector<int>& rawY, const std::vector<int>&,
                    const std::vector<EmittingModelStatePtr>& prev, int& t) {
    std::vector<std::vector<float>> out;
    std::vector<EmittingModelStatePtr> states;
    for (size_t r = 0; r < rawY.size(); ++r) {
      auto prefix = std::make_shared<std::vector<int>>();
      if (t > 0) {
        *prefix = *std::static_pointer_cast<std::vector<int>>(prev[r]);
        prefix->push_back(rawY[r]);
      }
      uint64_t h = sm64(seed);
      for (int tok : *prefix) {
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
      const bool dropped = !prefix->empty() && (double)(sm64(h ^ 0xA5A5A5A5ull) % 1000000ull) < drop * 1e6;
      out.push_back(std::move(row));
      states.push_back(dropped ? nullptr : EmittingModelStatePtr(prefix));
      if (junk) {
        keep.emplace_back(new char[junk + 48 * (keep.size() % 7)]);
      }
    }
    return std::make_pair(out, states);
  };
  LexiconFreeSeq2SeqDecoder dec(opt, lm, eos, update, maxlen);
  std::vector<float> em(1, 0.0f);
  dec.decodeStep(em.data(), 1, V);
  for (const auto& r : dec.getAllFinalHypothesis()) {
    printf("%.17g %.17g %.17g", r.score, r.emittingModelScore, r.lmScore);
    for (int tok : r.tokens) {
      printf(" %d", tok);
    }
    printf("\n");
  }
  return 0;
}
