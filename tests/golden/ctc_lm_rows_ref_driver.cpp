/*
 * tests/golden/ctc_lm_rows_ref_driver.cpp -- runs the reference's LexiconFreeDecoder (CTC; compiled from the unmodified
 * flashlight/text sources by make_ctc_lm_rows_golden.py into oracle/_ref/, dev container only) with an LM that scores a
 * whole vocabulary per state, as a neural token LM does: the fixtures of the CTC rows decoder.
 *
 * The LM is s2s_lm_rows_ref_driver.cpp's prefix-hash LM: its state is a child<>() per token that holds the prefix; its
 * answer for LM index i after a prefix is a splitmix64 function of (lm_seed, prefix, i) mapped to -(h >> 40) * 2^-20
 * (exact in float32).  score(state, u) reads index usr_to_lm[u] -- the identity, or (perm != 0) the first N entries of a
 * permutation of [0, W) -- and finish reads finish_index.  The emissions are a splitmix64 function of (seed, frame,
 * token) with the same mapping, times 1/4 (exact).  make_ctc_lm_rows_golden.py computes the same floats.
 *
 * usage: ctc_lm_rows_ref_driver seed T N K Kt thr lmw sil_score sil blank log_add lm_seed W perm finish junk
 * (junk: bytes allocated and kept per LM call -- a different heap layout for the second run)
 * prints: one line per final hypothesis: score am lm (%.17g) then the tokens.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
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
  if (argc != 17) {
    fprintf(stderr, "usage: %s seed T N K Kt thr lmw sil_score sil blank log_add lm_seed W perm finish junk\n", argv[0]);
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
  dec.decodeStep(em.data(), T, N);
  dec.decodeEnd();
  for (const auto& r : dec.getAllFinalHypothesis()) {
    printf("%.17g %.17g %.17g", r.score, r.emittingModelScore, r.lmScore);
    for (int tok : r.tokens) {
      printf(" %d", tok);
    }
    printf("\n");
  }
  return 0;
}
