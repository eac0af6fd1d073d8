/*
 * tests/golden/lex_ctc_lm_rows_stream_ref_driver.cpp -- runs the reference's LexiconDecoder (CTC; compiled from the
 * unmodified flashlight/text sources by make_lex_ctc_lm_rows_stream_golden.py into oracle/_ref/, dev container only) as
 * ONE STREAM: decodeStep on chunks, getBestHypothesis(lookBack), prune(lookBack), then decodeEnd -- the fixtures of the
 * lexicon CTC rows decoder's streams.  LM, lexicon file and emissions are lex_ctc_lm_rows_ref_driver.cpp's; `hold` forces
 * stretches of frames onto one token: "t0:t1:tok/..." gives token tok the emission 0 in frames [t0, t1) and every other
 * token its own emission - 8 (float32), "-" holds nothing.
 *
 * usage: lex_ctc_lm_rows_stream_ref_driver seed T N K Kt thr lmw word_score unk_score sil_score sil blank unk log_add
 *        is_lm_token lexicon lm_seed W perm finish n_map smear junk hold script
 * script: comma-separated ops -- cN: decodeStep on the next N frames (0 allowed), bL: getBestHypothesis(L), pL: prune(L);
 * the frames of all c ops add up to T.
 * prints: per b op "B score am lm tokens... | words..." (an empty result: "B"), per p op "P nDecodedFramesInBuffer", and
 * after decodeEnd one line "H score am lm tokens... | words..." per final hypothesis; scores as %.17g.
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
  if (argc != 26) {
    fprintf(stderr, "usage: %s seed T N K Kt thr lmw word_score unk_score sil_score sil blank unk log_add is_lm_token "
                    "lexicon lm_seed W perm finish n_map smear junk hold script\n", argv[0]);
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
  for (std::string hold = argv[24]; hold != "-" && !hold.empty();) {
    const size_t cut = hold.find('/');
    int t0 = 0, t1 = 0, tok = 0;
    if (sscanf(hold.substr(0, cut).c_str(), "%d:%d:%d", &t0, &t1, &tok) != 3 || t0 < 0 || t1 > T || tok < 0 || tok >= N) {
      fprintf(stderr, "hold: %s\n", hold.c_str());
      return 2;
    }
    for (int t = t0; t < t1; ++t) {
      for (int n = 0; n < N; ++n) {
        em[(size_t)t * N + n] = n == tok ? 0.0f : em[(size_t)t * N + n] - 8.0f;
      }
    }
    hold = cut == std::string::npos ? "" : hold.substr(cut + 1);
  }
  LexiconDecoder dec(opt, trie, lm, sil, blank, unk, {}, isLmToken);
  dec.decodeBegin();
  auto print = [](const char* tag, const DecodeResult& r) {
    printf("%s", tag);
    if (!r.tokens.empty()) {
      printf(" %.17g %.17g %.17g", r.score, r.emittingModelScore, r.lmScore);
      for (int tok : r.tokens) {
        printf(" %d", tok);
      }
      printf(" |");
      for (int w : r.words) {
        printf(" %d", w);
      }
    }
    printf("\n");
  };
  int at = 0;
  const std::string script = argv[25];
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
