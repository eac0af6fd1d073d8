/*
 * tests/golden/ctc_lm_rows_stream_ref_driver.cpp -- runs the reference's LexiconFreeDecoder (CTC; compiled from the
 * unmodified flashlight/text sources by make_ctc_lm_rows_stream_golden.py into oracle/_ref/, dev container only) as ONE
 * STREAM: decodeStep on chunks, getBestHypothesis(lookBack), prune(lookBack), then decodeEnd -- the fixtures of the CTC
 * rows decoder's streams.  The LM and the emissions are ctc_lm_rows_ref_driver.cpp's.
 *
 * usage: ctc_lm_rows_stream_ref_driver seed T N K Kt thr lmw sil_score sil blank log_add lm_seed W perm finish junk script
 * script: comma-separated ops -- cN: decodeStep on the next N frames (0 allowed), bL: getBestHypothesis(L), pL: prune(L);
 * the frames of all c ops add up to T.
 * prints: per b op "B score am lm tokens..." (an empty result: "B"), per p op "P nDecodedFramesInBuffer", and after
 * decodeEnd one line "H score am lm tokens..." per final hypothesis; scores as %.17g.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "flashlight/lib/text/decoder/LexiconFreeDecoder.h"

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
    for (int tok : prefix) {
      h = sm64(h ^ (uint64_t)(tok + 1));
    }
    const uint64_t x = sm64(h ^ ((uint64_t)(idx + 1) * 0xD1B54A32D192ED03ull));
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
  if (argc != 18) {
    fprintf(stderr, "usage: %s seed T N K Kt thr lmw sil_score sil blank log_add lm_seed W perm finish junk script\n",
            argv[0]);
    return 2;
  }
  const uint64_t seed = strtoull(argv[1], nullptr, 10);
  const int T = atoi(argv[2]), N = atoi(argv[3]);
  LexiconFreeDecoderOptions opt;
  opt.beamSize = atoi(argv[4]);
  opt.beamSizeToken = atoi(argv[5]);
  opt.beamThreshold = atof(argv[6]);
  opt.lmWeight = atof(argv[7]);
  opt.silScore = atof(argv[8]);
  const int sil = atoi(argv[9]), blank = atoi(argv[10]);
  opt.logAdd = atoi(argv[11]) != 0;
  opt.criterionType = CriterionType::CTC;
  auto lm = std::make_shared<RowsLM>();
  lm->seed = strtoull(argv[12], nullptr, 10);
  const int W = atoi(argv[13]);
  const uint64_t perm = strtoull(argv[14], nullptr, 10);
  lm->finishIdx = atoi(argv[15]);
  lm->junk = (size_t)atoll(argv[16]);
  std::vector<int> all((size_t)W);
  std::iota(all.begin(), all.end(), 0);
  if (perm) { /* the indices of [0, W) ordered by a hash: a permutation */
    std::stable_sort(all.begin(), all.end(), [&](int a, int b) {
      return sm64(perm ^ (uint64_t)(a + 1)) < sm64(perm ^ (uint64_t)(b + 1));
    });
  }
  lm->usrToLm.assign(all.begin(), all.begin() + N); /* (W >= N) */
  std::vector<float> em((size_t)T * N);
  for (int t = 0; t < T; ++t) {
    const uint64_t h = sm64(sm64(seed) ^ (uint64_t)(t + 1));
    for (int n = 0; n < N; ++n) {
      const uint64_t x = sm64(h ^ ((uint64_t)(n + 1) * 0xD1B54A32D192ED03ull));
      em[(size_t)t * N + n] = -(float)((double)(x >> 40) * (1.0 / 1048576.0)) * 0.25f;
    }
  }
  LexiconFreeDecoder dec(opt, lm, sil, blank, {});
  dec.decodeBegin();
  auto print = [](const char* tag, const DecodeResult& r) {
    printf("%s", tag);
    if (!r.tokens.empty()) {
      printf(" %.17g %.17g %.17g", r.score, r.emittingModelScore, r.lmScore);
    }
    for (int tok : r.tokens) {
      printf(" %d", tok);
    }
    printf("\n");
  };
  int at = 0;
  const std::string script = argv[17];
  for (size_t i = 0; i < script.size();) {
    const char op = script[i];
    size_t j = script.find(',', i);
    j = j == std::string::npos ? script.size() : j;
    const int v = atoi(script.substr(i + 1, j - i - 1).c_str());
    if (op == 'c') {
      if (at + v > T) {
        fprintf(stderr, "script: more than T frames\n");
        return 2;
      }
      dec.decodeStep(em.data() + (size_t)at * N, v, N);
      at += v;
    } else if (op == 'b') {
      print("B", dec.getBestHypothesis(v));
    } else if (op == 'p') {
      dec.prune(v);
      printf("P %d\n", dec.nDecodedFramesInBuffer());
    } else {
      fprintf(stderr, "script: op %c\n", op);
      return 2;
    }
    i = j + 1;
  }
  if (at != T) {
    fprintf(stderr, "script: %d of %d frames\n", at, T);
    return 2;
  }
  dec.decodeEnd();
  for (const auto& r : dec.getAllFinalHypothesis()) {
    print("H", r);
  }
  return 0;
}
