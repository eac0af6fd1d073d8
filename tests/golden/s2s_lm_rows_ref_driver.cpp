/*
 * tests/golden/s2s_lm_rows_ref_driver.cpp -- runs the reference's LexiconFreeSeq2SeqDecoder (compiled from the
 * unmodified flashlight/text sources by make_s2s_lm_rows_golden.py, dev container only) with an LM that scores a whole
 * vocabulary per state, as a neural token LM does (ConvLM.cpp:120-141's shape): the fixtures of the rows LM.
 *
 * The model is s2s_ref_driver.cpp's: a pure function of (seed, token prefix).  The LM's state is a new child<>() per
 * token that holds the prefix; its answer for LM index i after a prefix is a splitmix64 function of (lm_seed, prefix, i)
 * mapped to -(h >> 40) * 2^-20 (exact in float32), or -inf for one index in inf_mod (inf_mod 0: never).  score(state,
 * u) reads index usr_to_lm[u] -- the identity, or (perm != 0) the first V entries of a permutation of [0, W) -- and
 * finish reads finish_index (-1: usr_to_lm[eos]).  make_s2s_lm_rows_golden.SmRowsLM computes the same floats.
 *
 * usage: s2s_lm_rows_ref_driver seed V K Kt thr lmw eos_score eos maxlen eos_bias drop log_add lm_seed W perm finish
 *        inf_mod junk
 * (junk: bytes allocated and kept between model calls -- a different heap layout for the second run)
 * prints: one line per final hypothesis: score am lm (%.17g) then the tokens.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "flashlight/lib/text/decoder/LexiconFreeSeq2SeqDecoder.h"

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
  std::pair<LMStatePtr, float> score(const LMStatePtr& state, const int usrTokenIdx) override {
    auto in = std::static_pointer_cast<PrefixState>(state);
    auto out = in->child<PrefixState>(usrTokenIdx);
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
  if (argc != 19) {
    fprintf(stderr, "usage: %s seed V K Kt thr lmw eos_score eos maxlen eos_bias drop log_add lm_seed W perm finish "
                    "inf_mod junk\n", argv[0]);
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
  auto lm = std::make_shared<RowsLM>();
  lm->seed = strtoull(argv[13], nullptr, 10);
  const int W = atoi(argv[14]);
  const uint64_t perm = strtoull(argv[15], nullptr, 10);
  lm->infMod = strtoull(argv[17], nullptr, 10);
  const size_t junk = (size_t)atoll(argv[18]);
  std::vector<int> all((size_t)W);
  std::iota(all.begin(), all.end(), 0);
  if (perm) { /* the indices of [0, W) ordered by a hash: a permutation */
    std::stable_sort(all.begin(), all.end(), [&](int a, int b) {
      return sm64(perm ^ (uint64_t)(a + 1)) < sm64(perm ^ (uint64_t)(b + 1));
    });
  }
  lm->usrToLm.assign(all.begin(), all.begin() + V); /* (W >= V) */
  const int finish = atoi(argv[16]);
  lm->finishIdx = finish >= 0 ? finish : (eos < V ? lm->usrToLm[(size_t)eos] : 0); /* (eos >= V: never proposed) */
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
