/*
 * tests/cpp/backtrace_walk_san.cpp -- a stand-alone driver for a sanitizer build of the EMULATION of the narrow
 * back-trace's parallel walk (backtraceNarrow<RT, true>, text_amd/csrc/fltx_kernels.h); no device, nothing loaded into
 * an interpreter.  tests/cpp/backtrace_walk_san.sh compiles it with the emulator's sources under
 * -fsanitize=address,undefined and runs it.
 *
 * Three cases through the C ABI, ZeroLM on seeded emissions, the first two on the lexicon-free decoder, "bt_threads" = 256 (four waves):
 *   reused workspace  one decoder object decodes a dense batch (4 x 40 frames, beam 50), then a shorter one (5 .. 12
 *                     frames): the slots without a record of the second batch hold the first batch's;
 *   seams             beam 10, "bt_lds_kb" = 4: a 170-frame utterance holds the chunk length still while a second one's
 *                     history rows run from one below two chunks to one above the waves past it (last chunks of fewer
 *                     frames than waves, as many, one more; stretches of no frame and of one).
 *   odd lexicon       lexicon decoder over a small seeded trie, beam 15, odd lengths: a chunk of F x 15 two-byte records
 *                     ends on an odd half-word, and the int32 word records behind it must still be aligned.
 * Every batch is decoded again by a fresh decoder with "bt_walk_waves" = 1 (one walk per hypothesis) and the n-best --
 * counts, lengths, tokens, the three scores -- must be bit equal; "bt_walk_waves" must read 4 and 1.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "fltx.h"

#define CHECK(x)                                                                        \
  do {                                                                                  \
    if ((x) != FLTX_OK) {                                                               \
      std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, fltx_last_error()); \
      std::exit(2);                                                                     \
    }                                                                                   \
  } while (0)

static const int N = 29;

struct Batch {
  std::vector<float> e;
  std::vector<int64_t> off;
  std::vector<int32_t> T;
};

/* CTC-like rows: one peaked token per frame (a run of a few frames), the blank often, the rest far below */
static Batch makeBatch(const std::vector<int>& Ts, uint64_t seed) {
  Batch b;
  uint64_t s = seed * 6364136223846793005ull + 1442695040888963407ull;
  auto rnd = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  };
  for (int T : Ts) {
    b.off.push_back((int64_t)b.e.size());
    b.T.push_back(T);
    int peak = (int)(rnd() % (N - 1));
    for (int t = 0; t < T; ++t) {
      if (rnd() % 3 == 0) {
        peak = (int)(rnd() % (N - 1));
      }
      for (int n = 0; n < N; ++n) {
        float v = -6.0f - (float)(rnd() % 4096) / 1024.0f;
        if (n == peak) {
          v = -0.5f - (float)(rnd() % 1024) / 1024.0f;
        }
        if (n == N - 1) {
          v = -1.0f - (float)(rnd() % 2048) / 1024.0f;
        }
        b.e.push_back(v);
      }
    }
  }
  return b;
}

struct Result {
  std::vector<int32_t> nh, len, tokens;
  std::vector<double> scores;
  bool operator==(const Result& o) const {
    return nh == o.nh && len == o.len && tokens == o.tokens && scores.size() == o.scores.size() &&
           (scores.empty() || !std::memcmp(scores.data(), o.scores.data(), 8 * scores.size()));
  }
};

static fltx_decoder* newDecoder(fltx_ctx* ctx, fltx_lm* lm, int K, int ldsKb, int walk, const fltx_trie* trie = nullptr) {
  fltx_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.beam_size = K;
  opt.beam_size_token = N;
  opt.beam_threshold = 25.0;
  opt.unk_score = -1e30;
  opt.criterion = FLTX_CRITERION_CTC;
  fltx_decoder* d = nullptr;
  if (trie) { /* words over the tokens 0 .. N - 3, each ended by the silence N - 2; no <unk> paths */
    opt.unk_score = -std::numeric_limits<double>::infinity();
    CHECK(fltx_decoder_create(ctx, FLTX_DECODER_LEXICON, &opt, trie, lm, N - 2, N - 1, -1, nullptr, 0, 0, &d));
  } else {
    CHECK(fltx_decoder_create(ctx, FLTX_DECODER_LEXFREE, &opt, nullptr, lm, 0, N - 1, 0, nullptr, 0, 0, &d));
  }
  CHECK(fltx_decoder_set(d, "bt_threads", 256));
  CHECK(fltx_decoder_set(d, "bt_lds_kb", ldsKb));
  CHECK(fltx_decoder_set(d, "bt_walk_waves", walk));
  return d;
}

static Result decode(fltx_decoder* d, const Batch& b, int K, int wantWaves, int64_t* chunk = nullptr) {
  const int B = (int)b.T.size();
  CHECK(fltx_decode_batch(d, b.e.data(), 0, b.off.data(), b.T.data(), B, N));
  Result r;
  for (int i = 0; i < B; ++i) {
    int32_t nh = 0, len = 0, got = 0;
    CHECK(fltx_result_count(d, i, &nh, &len));
    std::vector<double> sc(3 * (size_t)nh + 1);
    std::vector<int32_t> tk((size_t)nh * len + 1);
    CHECK(fltx_result_fetch(d, i, nh, sc.data(), tk.data(), nullptr, &got));
    if (got != nh) {
      std::fprintf(stderr, "utterance %d: %d of %d hypotheses\n", i, got, nh);
      std::exit(2);
    }
    r.nh.push_back(nh);
    r.len.push_back(len);
    r.scores.insert(r.scores.end(), sc.begin(), sc.begin() + 3 * (size_t)nh);
    r.tokens.insert(r.tokens.end(), tk.begin(), tk.begin() + (size_t)nh * len);
  }
  int64_t waves = 0, rec = 0, lane = 0;
  CHECK(fltx_decoder_get(d, "bt_walk_waves", &waves));
  CHECK(fltx_decoder_get(d, "bt_record_bytes", &rec));
  CHECK(fltx_decoder_get(d, "engine", &lane));
  if (waves != wantWaves || rec != 2) {
    std::fprintf(stderr, "bt_walk_waves %lld (want %d), bt_record_bytes %lld, engine %lld, beam %d\n", (long long)waves,
                 wantWaves, (long long)rec, (long long)lane, K);
    std::exit(2);
  }
  if (chunk) {
    CHECK(fltx_decoder_get(d, "bt_chunk_frames", chunk));
  }
  return r;
}

static int g_cases = 0;

static void same(fltx_ctx* ctx, fltx_lm* lm, const Result& par, const Batch& b, int K, int ldsKb, const char* what,
                 const fltx_trie* trie = nullptr) {
  fltx_decoder* s = newDecoder(ctx, lm, K, ldsKb, 1, trie);
  const Result ser = decode(s, b, K, 1);
  CHECK(fltx_decoder_destroy(s));
  if (!(par == ser)) {
    std::fprintf(stderr, "FAILED %s: the parallel walk's n-best differs from the serial walk's\n", what);
    std::exit(1);
  }
  ++g_cases;
}

int main() {
  fltx_ctx* ctx = nullptr;
  fltx_lm* lm = nullptr;
  CHECK(fltx_ctx_create(-1, nullptr, &ctx));
  CHECK(fltx_lm_zero_create(ctx, &lm));
  { /* reused workspace */
    fltx_decoder* d = newDecoder(ctx, lm, 50, 0, -1);
    const Batch dense = makeBatch({40, 40, 40, 40}, 1), after = makeBatch({5, 12, 8, 9}, 2);
    const Result r1 = decode(d, dense, 50, 4);
    same(ctx, lm, r1, dense, 50, 0, "dense batch");
    const Result r2 = decode(d, after, 50, 4);
    same(ctx, lm, r2, after, 50, 0, "shorter batch on the same decoder object");
    CHECK(fltx_decoder_destroy(d));
  }
  { /* seams */
    const int anchor = 170, waves = 4;
    fltx_decoder* d = newDecoder(ctx, lm, 10, 4, -1);
    int64_t F = 0;
    decode(d, makeBatch({anchor}, 3), 10, waves, &F);
    if (F < 8 || 2 * F + waves + 1 > anchor + 2) {
      std::fprintf(stderr, "FAILED seams: chunk of %lld frames\n", (long long)F);
      return 1;
    }
    for (int rows = (int)(2 * F - 1); rows <= (int)(2 * F + waves + 1); ++rows) {
      int64_t f = 0;
      const Batch b = makeBatch({anchor, rows - 2}, 100 + (uint64_t)rows);
      const Result r = decode(d, b, 10, waves, &f);
      if (f != F) {
        std::fprintf(stderr, "FAILED seams: chunk %lld, then %lld\n", (long long)F, (long long)f);
        return 1;
      }
      same(ctx, lm, r, b, 10, 4, "seam");
    }
    CHECK(fltx_decoder_destroy(d));
  }
  { /* odd lexicon: F K two-byte records end on an odd half-word, the int32 word records follow them */
    const int K = 15;
    fltx_htrie* ht = nullptr;
    fltx_trie* trie = nullptr;
    CHECK(fltx_htrie_create(N, 0, &ht));
    uint64_t s = 77;
    std::set<std::vector<int32_t>> seen; /* (one word per spelling) */
    for (int w = 0; w < 60; ++w) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const int n = 1 + (int)((s >> 40) % 4);
      std::vector<int32_t> sp;
      for (int i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        sp.push_back((int32_t)((s >> 40) % (N - 2)));
      }
      sp.push_back(N - 2);
      if (seen.insert(sp).second) {
        CHECK(fltx_htrie_insert(ht, sp.data(), (int32_t)sp.size(), w, 0.0f));
      }
    }
    CHECK(fltx_htrie_smear(ht, FLTX_SMEAR_MAX));
    CHECK(fltx_htrie_upload(ht, ctx, &trie));
    fltx_decoder* d = newDecoder(ctx, lm, K, 0, -1, trie);
    int odd = 0;
    for (int T : {39, 37, 21}) {
      int64_t F = 0;
      const Batch b = makeBatch({T, T - 6}, 200 + (uint64_t)T);
      const Result r = decode(d, b, K, 4, &F);
      odd += (int)((F * K) & 1);
      same(ctx, lm, r, b, K, 0, "odd lexicon", trie);
    }
    if (!odd) {
      std::fprintf(stderr, "FAILED odd lexicon: no chunk with an odd number of records\n");
      return 1;
    }
    CHECK(fltx_decoder_destroy(d));
    CHECK(fltx_trie_destroy(trie));
    CHECK(fltx_htrie_destroy(ht));
  }
  CHECK(fltx_lm_destroy(lm));
  CHECK(fltx_ctx_destroy(ctx));
  std::printf("PASSED %d comparisons\n", g_cases);
  return 0;
}
