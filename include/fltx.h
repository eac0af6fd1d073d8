/*
 * include/fltx.h -- C ABI of the MI355X-native batched beam-search decoder.
 *
 * This is the drop-in boundary for the hot path of flashlight/text's
 * LexiconFreeDecoder / LexiconDecoder.  The reference
 * has no FFI for this path (it is a header/C++ library); the functions below
 * are what a cgo/JNI/ctypes/C++ binding of that path binds.  Each entry point
 * cites the reference interface it replaces (paths relative to
 * /root/reference/flashlight/lib/text/).
 *
 * Conventions: plain pointers and sizes only; every function returns an int
 * status (FLTX_OK == 0) and records a message retrievable with
 * fltx_last_error() (thread-local).  The reference reports errors as C++
 * exceptions (decoder/lm/LM.h:40, decoder/Trie.cpp:32,54); the C++ facade in
 * text_amd/csrc/flashlight/ converts non-zero statuses back into the same
 * exception types.
 *
 * There is NO CPU fallback behind this ABI: every decode call runs the HIP
 * kernels in text_amd/csrc/fltx_kernels.h on a gfx950 device and fails with
 * FLTX_ERR_HIP when no device is usable.
 */
#ifndef FLTX_H_
#define FLTX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLTX_API __attribute__((visibility("default")))

enum {
  FLTX_OK = 0,
  FLTX_ERR_INVALID = 1,     /* bad argument (std::invalid_argument) */
  FLTX_ERR_HIP = 2,         /* HIP runtime failure / no device (std::runtime_error) */
  FLTX_ERR_OOM = 3,         /* device allocation failed */
  FLTX_ERR_UNSUPPORTED = 4, /* configuration the device path does not cover */
  FLTX_ERR_RANGE = 5,       /* index out of range (std::out_of_range) */
  FLTX_ERR_STATE = 6,       /* call sequence error (e.g. results before decode) */
  FLTX_ERR_CALLBACK = 7     /* a host-LM callback reported failure (the binding rethrows what the user's LM threw) */
};

/* CriterionType, decoder/Decoder.h:16. */
enum { FLTX_CRITERION_ASG = 0, FLTX_CRITERION_CTC = 1, FLTX_CRITERION_S2S = 2 };
/* SmearingMode, decoder/Trie.h:21-25. */
enum { FLTX_SMEAR_NONE = 0, FLTX_SMEAR_MAX = 1, FLTX_SMEAR_LOGADD = 2 };
enum { FLTX_DECODER_LEXFREE = 0, FLTX_DECODER_LEXICON = 1, FLTX_DECODER_S2S_LEXFREE = 2, FLTX_DECODER_S2S_LEXICON = 3,
       FLTX_DECODER_CTC_ROWS = 4, FLTX_DECODER_LEX_CTC_ROWS = 5 };

/* LexiconDecoderOptions (decoder/LexiconDecoder.h:21-31); the lexicon-free
 * decoder (decoder/LexiconFreeDecoder.h:20-28) ignores word_score/unk_score. */
typedef struct fltx_options {
  int32_t beam_size;
  int32_t beam_size_token;
  double beam_threshold;
  double lm_weight;
  double word_score;
  double unk_score;
  double sil_score;
  int32_t log_add;
  int32_t criterion;
} fltx_options;

typedef struct fltx_ctx fltx_ctx;         /* one HIP device + stream */
typedef struct fltx_lm fltx_lm;           /* LM tables resident in HBM */
typedef struct fltx_trie fltx_trie;       /* flattened lexicon trie in HBM */
typedef struct fltx_decoder fltx_decoder; /* options + per-batch workspace */

FLTX_API const char* fltx_last_error(void);
FLTX_API const char* fltx_version(void);

/* ---- context ------------------------------------------------------------ */
/* device < 0: use the current HIP device.  stream == NULL: library-owned
 * stream.  A caller-owned hipStream_t may be passed as void*. */
FLTX_API int fltx_ctx_create(int device, void* stream, fltx_ctx** out);
FLTX_API int fltx_ctx_destroy(fltx_ctx* ctx);
FLTX_API int fltx_ctx_synchronize(fltx_ctx* ctx);
/* the hipStream_t kernels are launched on (for event timing by the caller) */
FLTX_API void* fltx_ctx_stream(fltx_ctx* ctx);
/* a number that names this context and is never handed out again (an address can be: callers that cache per-context
 * objects -- the facade's Trie keeps one flattened copy per context -- key them by this, not by the pointer) */
FLTX_API uint64_t fltx_ctx_uid(fltx_ctx* ctx);

/* ---- language models ---------------------------------------------------- */
/* ZeroLM (decoder/lm/ZeroLM.h:22-32, ZeroLM.cpp:14-26). */
/* (ctx may be NULL for both LM constructors: tables are built on the host and
 * uploaded when a decoder is created.) */
FLTX_API int fltx_lm_zero_create(fltx_ctx* ctx, fltx_lm** out);
/* Back-off n-gram LM with ARPA semantics, replacing the KenLM adapter
 * (decoder/lm/KenLM.h:52-63, KenLM.cpp:32-83).  The model is passed as flat
 * host arrays, one row per n-gram, all orders concatenated in increasing
 * order: ngram_order[i] in 1..order, ngram_words[i*order .. i*order+order-1]
 * = LM word ids oldest first (unused tail = -1), prob/backoff = log10 values.
 * usr_to_lm[u] maps the decoder's word/token index u to an LM word id
 * (KenLM.cpp:44-49); bos/eos/unk are LM ids of <s>, </s>, <unk>. */
FLTX_API int fltx_lm_ngram_create(fltx_ctx* ctx, int32_t order, int64_t n_ngrams,
                                  const int32_t* ngram_order,
                                  const int32_t* ngram_words,
                                  const float* prob, const float* backoff,
                                  const int32_t* usr_to_lm, int32_t n_usr,
                                  int32_t bos, int32_t eos, int32_t unk,
                                  fltx_lm** out);
/* KenLM(path, usrTknDict) for ARPA text models (decoder/lm/KenLM.cpp:32-50):
 * parse the file on the host, map every '\n'-separated entry of usr_words
 * (index = user dictionary index) to an LM word id, unknown strings to <unk>.
 * No device is needed until a decoder is created with the LM. */
FLTX_API int fltx_lm_arpa_load(const char* path, const char* usr_words, fltx_lm** out);
/* A user-defined LM: any subclass of `LM` (decoder/lm/LM.h:61-85), e.g. through the reference's Python trampoline
 * PyLM (bindings/python/flashlight/lib/text/_decoder.cpp:39-56).  It has no tables to flatten, so LM::start / score /
 * finish stay calls into host code -- but the beam search does not: candidates, merge, prune and history run in the
 * HIP kernels as for every other LM.  Once per frame a kernel lists the (LM state, index) pairs the frame's candidate
 * generation will ask about, for the whole batch; the library asks the callbacks below about each DISTINCT pair
 * once (what LMState::child's memo gives the reference, lm/LM.h:24-34: LM::score must be a function of its arguments)
 * and uploads the answers; the frame's kernel reads them.  The shape is the reference's own for LMs that batch
 * their queries (decoder/lm/ConvLM.cpp:144-240 behind Utils.h:346-354 updateLMCache).
 *
 * LM states cross this boundary as int32 ids, per utterance, handed out by the callee: 0 is what LM::start returned;
 * `score` must return the SAME id whenever the user's LM returns the same LMState object and a new id otherwise --
 * the reference merges hypotheses on the state's address (lm/LM.h:37-49), the kernels merge on this id.
 * Every callback returns 0, or non-zero to abort the decode call with FLTX_ERR_CALLBACK.  Callbacks are made on the
 * thread that called the decoder, never concurrently (decoder/Utils.h:60-62).  Not usable with fltx_group_*. */
typedef struct fltx_host_lm {
  void* user;
  /* decodeBegin: LM::start(false) (LexiconFreeDecoder.cpp:24, LexiconDecoder.cpp:24) for utterances 0 .. n_utt-1;
   * ids of an earlier decode on this decoder are void */
  int32_t (*start)(void* user, int32_t n_utt);
  /* n questions: idx[i] >= 0: LM::score(state[i] of utterance utt[i], idx[i]); idx[i] == -1: LM::finish(state[i]).
   * out_state[i] = id of the returned state, out_score[i] = the returned score */
  int32_t (*score)(void* user, int32_t n, const int32_t* utt, const int32_t* state, const int32_t* idx,
                   int32_t* out_state, float* out_score);
  /* may be NULL.  LM::updateCache(states of utterance utt's beam) after every frame (Utils.h:346-354) */
  int32_t (*update_cache)(void* user, int32_t utt, int32_t n, const int32_t* states);
  /* may be NULL.  After Decoder::prune: only these states of utterance utt are still held by a hypothesis; ids of
   * the others will not be passed again and their LMState objects may be released (what dropping the pruned
   * hypotheses' shared_ptrs does in the reference, Utils.h:312-342) */
  int32_t (*retain)(void* user, int32_t utt, int32_t n, const int32_t* states);
} fltx_host_lm;
FLTX_API int fltx_lm_host_create(const fltx_host_lm* callbacks, fltx_lm** out);
FLTX_API int fltx_lm_destroy(fltx_lm* lm);
/* LM::start + LM::score chain + optional LM::finish on the device tables
 * (decoder/lm/LM.h:61-78); per_word may be NULL.  Used by known-answer tests
 * (test/decoder/DecoderTest.cpp:107-120). */
FLTX_API int fltx_lm_score_sequence(fltx_lm* lm, const int32_t* usr_words,
                                    int32_t n, int32_t with_finish,
                                    float* per_word, float* total);

/* Explicit-state LM::start / LM::score / LM::finish on the host copy of the
 * flat tables (decoder/lm/LM.h:61-78), for the C++ facade's LM objects (trie
 * label scores, known-answer checks).  A state is fltx_lm_state_size() int32
 * context node ids (0 for ZeroLM).  usr_idx == -1 scores </s> (finish). */
FLTX_API int fltx_lm_state_size(fltx_lm* lm, int32_t* n);
FLTX_API int fltx_lm_start(fltx_lm* lm, int32_t start_with_nothing, int32_t* ctx_out);
FLTX_API int fltx_lm_step(fltx_lm* lm, const int32_t* ctx_in, int32_t usr_idx, int32_t* ctx_out,
                          float* score);

/* ---- lexicon trie -------------------------------------------------------- */
/* Upload an already built and smeared trie (decoder/Trie.h:64-92) as flat
 * arrays; node 0 is the root.  child[node*n_tokens + token] = child node or
 * -1; max_score[node] (float, after smearing); labels of node i are
 * labels[label_off[i] .. label_off[i+1]) (at most kTrieMaxLabel = 6 each,
 * Trie.h:19). */
FLTX_API int fltx_trie_create(fltx_ctx* ctx, int64_t n_nodes, int32_t n_tokens,
                              const int32_t* child, const float* max_score,
                              const int32_t* label_off, const int32_t* labels,
                              fltx_trie** out);
FLTX_API int fltx_trie_destroy(fltx_trie* trie);

/* Host-side trie builder with the reference's Trie semantics
 * (decoder/Trie.h:64-92, Trie.cpp:26-101): insert / search / smear on the CPU
 * (setup, runs once), then fltx_htrie_upload flattens it into HBM.  insert
 * returns FLTX_ERR_RANGE for an index outside [0, max_children)
 * (Trie.cpp:31-34 throws std::out_of_range) and silently drops labels beyond
 * kTrieMaxLabel = 6 per node (Trie.cpp:40-46). */
typedef struct fltx_htrie fltx_htrie;
FLTX_API int fltx_htrie_create(int32_t max_children, int32_t root_idx, fltx_htrie** out);
FLTX_API int fltx_htrie_destroy(fltx_htrie* t);
FLTX_API int fltx_htrie_insert(fltx_htrie* t, const int32_t* indices, int32_t n,
                               int32_t label, float score);
/* *found = 0/1; max_score, n_labels, labels[<=6], scores[<=6] may be NULL */
FLTX_API int fltx_htrie_search(fltx_htrie* t, const int32_t* indices, int32_t n,
                               int32_t* found, float* max_score, int32_t* n_labels,
                               int32_t* labels, float* scores);
FLTX_API int fltx_htrie_smear(fltx_htrie* t, int32_t mode);
FLTX_API int fltx_htrie_num_nodes(fltx_htrie* t, int64_t* n);
FLTX_API int fltx_htrie_upload(fltx_htrie* t, fltx_ctx* ctx, fltx_trie** out);
/* One node of the host trie by id (0 = root): TrieNode::idx / maxScore / labels / scores and
 * the (token, node id) pairs of TrieNode::children (decoder/Trie.h:30-55), for bindings that
 * expose the node tree (bindings/python/.../_decoder.cpp:173-186).  Any output may be NULL;
 * labels / scores hold up to 6 entries, the child arrays child_capacity. */
FLTX_API int fltx_htrie_node(fltx_htrie* t, int64_t node, int32_t* token, float* max_score,
                             int32_t* n_labels, int32_t* labels, float* scores, int32_t* n_children,
                             int32_t* child_tokens, int64_t* child_nodes, int32_t child_capacity);

/* ---- decoder ------------------------------------------------------------- */
/* LexiconFreeDecoder(opt, lm, sil, blank, transitions)
 * (decoder/LexiconFreeDecoder.h:102-112) when kind == FLTX_DECODER_LEXFREE
 * (trie NULL, unk/is_lm_token ignored);
 * LexiconDecoder(opt, trie, lm, sil, blank, unk, transitions, isLmToken)
 * (decoder/LexiconDecoder.h:117-133) when kind == FLTX_DECODER_LEXICON.
 * transitions: n_tokens*n_tokens floats or NULL/0 (copied). */
FLTX_API int fltx_decoder_create(fltx_ctx* ctx, int32_t kind,
                                 const fltx_options* opt, const fltx_trie* trie,
                                 const fltx_lm* lm, int32_t sil, int32_t blank,
                                 int32_t unk, const float* transitions,
                                 int32_t n_transitions, int32_t is_lm_token,
                                 fltx_decoder** out);
FLTX_API int fltx_decoder_destroy(fltx_decoder* dec);

/* Batched Decoder::decode (decoder/Decoder.h:51-57) for B independent
 * utterances: decodeBegin + decodeStep(all frames) + decodeEnd + back-trace,
 * all on the device.  Utterance b reads T[b]*N floats (frame-major, token
 * fastest, LexiconDecoder.cpp:69) starting at emissions + offsets[b].
 * emissions_on_device != 0: `emissions` is a device pointer (HBM resident);
 * otherwise it is a host pointer and is copied to the device first (the
 * pointer is only borrowed for the duration of the call).  offsets and T are
 * host arrays.  The call is asynchronous on the context stream; results are
 * read with fltx_result_*, which synchronise. */
FLTX_API int fltx_decode_batch(fltx_decoder* dec, const float* emissions,
                               int32_t emissions_on_device,
                               const int64_t* offsets, const int32_t* T,
                               int32_t B, int32_t N);

/* Streaming interface for B parallel streams (Decoder::decodeBegin /
 * decodeStep / decodeEnd / prune, decoder/Decoder.h:42-61).  max_frames bounds
 * the total frames buffered per stream between prunes.
 * Lifetime of a device buffer (emissions_on_device != 0; the same holds for fltx_decode_batch): every read of it
 * is queued on the context's stream before the call returns -- also the second pass of a lexicon stream's chunk
 * whose candidate list overflowed, which is therefore not deferred to a later call for such a chunk.  The caller
 * may overwrite the buffer in stream order on that stream, or from anywhere after fltx_ctx_synchronize / after
 * any call that returns results of this chunk.  A host buffer is only borrowed for the duration of the call. */
FLTX_API int fltx_stream_begin(fltx_decoder* dec, int32_t B, int32_t N,
                               int32_t max_frames);
FLTX_API int fltx_stream_step(fltx_decoder* dec, const float* emissions,
                              int32_t emissions_on_device,
                              const int64_t* offsets, const int32_t* T);
FLTX_API int fltx_stream_end(fltx_decoder* dec);
/* Decoder::prune(lookBack) for every stream (LexiconFreeDecoder.cpp:205-227). */
FLTX_API int fltx_stream_prune(fltx_decoder* dec, int32_t look_back);
/* nDecodedFramesInBuffer (LexiconFreeDecoder.cpp:201-203). */
FLTX_API int fltx_stream_frames_in_buffer(fltx_decoder* dec, int32_t b,
                                          int32_t* n);

/* ---- seq2seq: LexiconFreeSeq2SeqDecoder as a batched device step ----------- */
/* LexiconFreeSeq2SeqDecoderOptions (decoder/LexiconFreeSeq2SeqDecoder.h:23-30). */
typedef struct fltx_s2s_options {
  int32_t beam_size;
  int32_t beam_size_token;
  double beam_threshold;
  double lm_weight;
  double eos_score;
  int32_t log_add; /* accepted and without effect: no two candidates of a step share an LM state, nothing merges */
} fltx_s2s_options;

/* LexiconFreeSeq2SeqDecoder(opt, lm, eos, emittingModelUpdateFunc, maxOutputLength)
 * (decoder/LexiconFreeSeq2SeqDecoder.h:100-111, .cpp:20-165) for B utterances at once.  The emitting model stays the
 * caller's: between two fltx_s2s_step calls it scores the rows the previous call listed.  The decoder is an
 * fltx_decoder: fltx_result_count / fetch / fetch_batch / fetch_batch_compact / device / best read its n-best after
 * fltx_s2s_end (rows of max_output_length + 3 tokens, right-aligned, -1 in front; words all -1); fltx_decode_batch and
 * fltx_stream_* return FLTX_ERR_STATE on it.
 * Limits (FLTX_ERR_UNSUPPORTED beyond them; there is no CPU fallback): beam_size <= 256, V <= 65 536,
 * max_output_length <= 4 096, min(beam_size_token, V) <= 64 when the LM scores (an n-gram LM with lm_weight != 0; any
 * beam_size_token under ZeroLM or lm_weight == 0), ZeroLM or n-gram LMs only (a host LM, fltx_lm_host_create, may hand
 * out repeated states and would need merges). */
FLTX_API int fltx_s2s_decoder_create(fltx_ctx* ctx, const fltx_s2s_options* opt, const fltx_lm* lm, int32_t eos,
                                     int32_t max_output_length, fltx_decoder** out);
/* decodeStep's start (LexiconFreeSeq2SeqDecoder.cpp:22-32) for B utterances whose model rows are V scores wide.
 * Writes the first call's rows.  Row lists are caller-owned DEVICE buffers of B*K int32 (K = beam_size), n_rows of B:
 * row k of utterance b is entry b*K + k, rows k >= n_rows[b] are padding (-1).  For row k:
 *   next_token   the hypothesis' last token (rawY; -1 for the root);
 *   next_beam_idx  its parent's index in the previous beam (rawBeamIdx: that beam includes finished hypotheses, so it
 *                is not a row number; -1 for the root);
 *   next_src_row the row of the previous step's call that produced the parent (b*K + k'; -1 for the root): the index a
 *                model passes to index_select on its per-row state (rawPrevStates).
 * A decoder may begin again after any step or end: the search restarts from the root. */
FLTX_API int fltx_s2s_begin(fltx_decoder* dec, int32_t B, int32_t V, int32_t* next_token, int32_t* next_beam_idx,
                            int32_t* next_src_row, int32_t* n_rows);
/* One step of every utterance (:34-150): `scores` holds the model's rows, row b*K + k at scores + (b*K + k) *
 * row_stride (row_stride >= V floats); a device pointer when on_device != 0, else a host pointer copied first.
 * row_valid (may be NULL; device / host as scores) holds B*K bytes: 0 marks a row the model dropped (its state came
 * back null, :86-89) -- it proposes nothing.  Padding rows and rows of row_valid 0 are never read.  The four outputs
 * are the next call's rows, as fltx_s2s_begin writes them; an utterance that is done lists none.  Asynchronous on the
 * context's stream.  A step after the last one (max_output_length steps, or every utterance done) changes nothing and
 * lists no rows. */
FLTX_API int fltx_s2s_step(fltx_decoder* dec, const float* scores, int32_t on_device, int64_t row_stride,
                           const uint8_t* row_valid, int32_t* next_token, int32_t* next_beam_idx,
                           int32_t* next_src_row, int32_t* n_rows);
/* Element types and kinds of the rows fltx_s2s_step_typed reads. */
typedef enum fltx_dtype { FLTX_DTYPE_F32 = 0, FLTX_DTYPE_F16 = 1, FLTX_DTYPE_BF16 = 2 } fltx_dtype;
enum { FLTX_S2S_LOG_PROBS = 0, FLTX_S2S_LOGITS = 1 };
/* fltx_s2s_step on the model's output as the model produces it: rows of `dtype` (IEEE binary16 or bfloat16 bits, or
 * float), row b*K + k at scores + (b*K + k) * row_stride ELEMENTS (row_stride >= V; rows of 2-byte types need only be
 * 2-byte aligned).  kind FLTX_S2S_LOG_PROBS: the row holds the model's scores (widened exactly to float).
 * kind FLTX_S2S_LOGITS: raw logits; the model score of token v is (float)((double)x_v - lse), lse = m + log(sum over
 * the non-NaN entries of exp(x_v - m)), m their maximum (lse = m when m is not finite); a NaN score is never a
 * candidate.  row_lse (may be NULL) is a device buffer of B*K doubles: in logits mode it receives each live row's lse
 * and NaN for every other row; in log-probs mode it is left untouched.  Host rows (on_device == 0) are staged in their
 * own type.  Row contract, asynchrony and the no-op step after the last one are those of fltx_s2s_step; works on both
 * seq2seq decoder kinds.  FLTX_ERR_INVALID on a bad dtype or kind or row_stride < V. */
FLTX_API int fltx_s2s_step_typed(fltx_decoder* dec, const void* scores, int32_t dtype, int32_t kind,
                                 int32_t on_device, int64_t row_stride, const uint8_t* row_valid, double* row_lse,
                                 int32_t* next_token, int32_t* next_beam_idx, int32_t* next_src_row, int32_t* n_rows);
/* Shallow fusion with an LM that scores a whole vocabulary per state (a neural token LM: ConvLM, a transformer LM).
 * An LM whose answers arrive per step as rows next to the model's rows: row b*K+k holds LM::score(state of that
 * hypothesis, v) for every LM index v (ConvLM.cpp:120-141's shape).  lm_width: entries per LM row (0: the decoder's V).
 * usr_to_lm (may be NULL: identity, n_usr ignored): the LM index of the model's token u (ConvLM.cpp:40-49); every
 * entry must lie in [0, lm_width) when lm_width > 0, else FLTX_ERR_INVALID.  finish_index: the LM index LM::finish reads
 * (ConvLM.cpp:140-141: the LM's </s>); -1: usr_to_lm[eos] of the decoder.  The LM's per-hypothesis state is the
 * caller's, carried by index_select(next_src_row) as the model's is.
 * Four decoders take such an LM: fltx_s2s_decoder_create (every hypothesis has its own prefix and so its own state: no
 * merges), fltx_s2s_lex_decoder_create with is_lm_token != 0 (a word-piece LM under a lexicon: hypotheses that
 * segment one token string differently share a state and merge, see there), fltx_ctc_rows_decoder_create (CTC
 * emissions, one LM row per LM state; finish_index must be given there) and fltx_ctc_rows_lex_decoder_create with
 * is_lm_token != 0 (CTC emissions under a lexicon; finish_index likewise).  The other decoders (fltx_decoder_create among
 * them), a lexicon seq2seq
 * decoder with is_lm_token == 0 (word-level rows come in by fltx_lm_word_rows_create below), fltx_group_create and the
 * fltx_lm_* state functions return FLTX_ERR_UNSUPPORTED.
 * The caller's obligation: the LM must be a pure function of the token prefix -- the same row for the same tokens since
 * the start, whatever words they were cut into (LMState::child semantics, lm/LM.h:24-34; what a neural token LM fed
 * its own prefix is).  Under the lexicon decoder the state a merged hypothesis carries on is the one
 * index_select(next_src_row) picks, the best member's; that equals any member's only under this condition.
 * At fltx_s2s_begin: FLTX_ERR_INVALID when a map has fewer than V entries, or when a token's LM index or (eos < V) the
 * finish index lies outside the LM's rows. */
FLTX_API int fltx_lm_rows_create(int32_t lm_width, const int32_t* usr_to_lm, int32_t n_usr, int32_t finish_index,
                                 fltx_lm** out);
/* fltx_s2s_step_typed on a decoder of either seq2seq kind made with a rows LM (LexiconFreeSeq2SeqDecoder.cpp:103-143,
 * LexiconSeq2SeqDecoder.cpp:94-198 with isLmToken): the token beam of a
 * row is taken from the model's scores alone; for each kept token n the LM score is a float -- in log-probs mode the LM
 * row's entry at usr_to_lm[n] (at finish_index when n == eos), widened exactly; in logits mode (float)((double)x -
 * lse_lm), lse_lm as fltx_s2s_step_typed defines lse, which lm_row_lse (may be NULL; B*K doubles on the device)
 * receives -- and the candidate's score, emittingModelScore and lmScore are built with the reference's double
 * operations (lmScore accumulates when lm_weight == 0 too).  A candidate whose score is NaN (a NaN LM entry,
 * 0 * -inf) is never a candidate; a -inf LM entry behaves as a -inf model entry.  LM rows of padding rows and of rows
 * with row_valid 0 are never read.  The model's and the LM's rows have independent dtype, kind and stride
 * (lm_row_stride >= lm_width, in elements); both are device pointers, or both host pointers staged in their own types.
 * Lexicon-free decoder: with lm_weight != 0 the exact token beam is kept (min(beam_size_token, V) <= 64); with
 * lm_weight == 0 the shortcut of ZeroLM stays (the row's best min(beam_size_token, beam_size + 1) tokens and eos) and
 * the LM entries of those are gathered for lmScore -- a NaN candidate among them is dropped, not replaced by a token
 * beyond the shortcut.
 * Lexicon decoder (is_lm_token != 0): always the exact token beam, min(beam_size_token, V) <= 256, taken before the trie
 * filter; no shortcut at lm_weight == 0.  A kept token n of a hypothesis makes up to three kinds of candidate, which
 * share the one LM entry of (row, n): eos at the trie root -- the entry at finish_index, new LM state child(state, -1),
 * score ((h.score + am) + eos_score) + lm_weight * lm; the move to n's child in the trie -- the entry at usr_to_lm[n],
 * new state child(state, n), score (h.score + am) + lm_weight * lm (no smearing term); and, when that child carries
 * labels, the end of its first label's word -- the same entry and state, score ((h.score + am) + word_score) +
 * lm_weight * lm, back at the root.  Candidates in one state, trie node and token merge (max or logAdd); the merged
 * hypothesis keeps the best member's fields, next_src_row among them.
 * fltx_s2s_step / fltx_s2s_step_typed on a decoder with a rows LM, and this call on any other, return FLTX_ERR_STATE;
 * FLTX_ERR_INVALID on a bad dtype or kind, a stride below the width, or NULL rows before the last step. */
FLTX_API int fltx_s2s_step_lm_rows(fltx_decoder* dec,
    const void* scores, int32_t dtype, int32_t kind, int64_t row_stride,
    const void* lm_scores, int32_t lm_dtype, int32_t lm_kind, int64_t lm_row_stride,
    int32_t on_device, const uint8_t* row_valid, double* row_lse, double* lm_row_lse,
    int32_t* next_token, int32_t* next_beam_idx, int32_t* next_src_row, int32_t* n_rows);
/* A word-level rows LM: a neural LM over the lexicon's WORDS (a word-level ConvLM / transformer LM) in shallow fusion
 * under fltx_s2s_lex_decoder_create with is_lm_token == 0 -- spellings constrained by the trie, whole words scored by the
 * LM, the smeared trie standing in for the LM inside a word.  lm_width (required, 0 < lm_width <= 4 194 304 = 2^22;
 * FLTX_ERR_UNSUPPORTED beyond): entries per LM row; every row offset is formed in 64 bits.  word_to_lm (may be NULL:
 * identity, n_words ignored): the LM index of the lexicon's word id w (a trie label).  finish_index (required, >= 0:
 * eos is a token and has no word id): the LM index LM::finish reads.  Only fltx_s2s_lex_decoder_create and
 * fltx_ctc_rows_lex_decoder_create (CTC emissions, the same checks at its create; there unk needs a map entry too when
 * unk_score > -inf), both with is_lm_token == 0, take such an LM; those decoders with is_lm_token != 0,
 * fltx_s2s_decoder_create, fltx_ctc_rows_decoder_create, fltx_decoder_create,
 * fltx_group_create and the fltx_lm_* state functions return FLTX_ERR_UNSUPPORTED ("rows LM").  The trie is known at
 * fltx_s2s_lex_decoder_create, which returns FLTX_ERR_INVALID when a label w of the trie has no entry in a given map
 * (w >= n_words) or an LM index outside [0, lm_width), or when finish_index lies outside [0, lm_width).
 * The caller's obligation (the token-level one above, for words): the LM must be a pure function of the WORD prefix --
 * the same row for the same words since the start, however they were spelled.  Hypotheses in one LM state, trie node
 * and token merge; the state that lives on is the one index_select(next_src_row) picks, the best member's, which equals
 * any member's only under this condition. */
FLTX_API int fltx_lm_word_rows_create(int32_t lm_width, const int32_t* word_to_lm, int32_t n_words, int32_t finish_index,
                                      fltx_lm** out);
/* The step of a decoder made with a word-level rows LM (LexiconSeq2SeqDecoder.cpp:91-198 with isLmToken == false).  The
 * model's rows are fltx_s2s_step_lm_rows' in every respect: dtypes, kinds, strides in elements, host staging, row_valid,
 * row_lse, the no-op step after the last one, asynchrony.
 * The LM's state changes only where a word ends, so most hypotheses carry the state they had a step ago and many share
 * one: lm_scores holds n_lm_rows rows of lm_width entries (lm_row_stride >= lm_width), and lm_row_of (B*K int32; a device
 * pointer when on_device, else a host pointer, staged) names the LM row of each decoder row -- one LM row can serve
 * many.  lm_row_of == NULL: identity, n_lm_rows is ignored and taken as B*K.  An entry outside [0, n_lm_rows) on a live
 * row makes that row's LM entries NaN: it keeps its moves inside words and has no word-end and no eos candidate;
 * nothing is read through it.  lm_row_lse (may be NULL; B*K doubles on the device, indexed by DECODER row) receives in
 * logits mode the lse of the LM row each live decoder row names, NaN for the other rows.  A shared LM row has its lse
 * computed once per decoder row that names it -- the same bits every time; the work is duplicated, not deduplicated.
 * The token beam is the exact min(beam_size_token, V) <= 256 largest model scores, before the trie filter.  A kept
 * token n of hypothesis h makes three kinds of candidate: eos at the trie root -- lm = the entry at finish_index (minus
 * lexMaxScore, 0 at the root), new LM state child(state, -1), score ((h.score + am) + eos_score) + lm_weight * lm; the
 * move to n's child -- no LM entry is read, lm = maxScore[child] - lexMaxScore in float (smearing), the state unchanged;
 * and one word end per label w of that child -- lm = (float)entry(word_to_lm[w]) - lexMaxScore (a float subtraction),
 * new state child(state, w), score ((h.score + am) + word_score) + lm_weight * lm, back at the root.  am and lm
 * accumulate separately, also at lm_weight == 0; a NaN score is never a candidate; a -inf entry behaves as a -inf model
 * entry.  Log-probs rows cost about rows * min(beam_size_token, V) * (1 + labels) element reads, whatever lm_width.
 * next_word (required; B*K int32 on the device): for every listed row the word its hypothesis ended in this step, -1
 * when it ended none, -1 on padding rows (fltx_s2s_begin lists the root, which ended none: nothing to write there).
 * With next_src_row it is all the caller's LM needs: next_word[r] < 0 -- the state, and its LM row, are those of
 * next_src_row[r]; else the caller advances that state by the word and makes a new row.
 * fltx_s2s_step / _typed / _lm_rows on such a decoder, and this call on any other, return FLTX_ERR_STATE;
 * FLTX_ERR_INVALID on a bad dtype or kind, a stride below the width, NULL next_word, n_lm_rows < 1 with lm_row_of, or
 * NULL rows before the last step. */
FLTX_API int fltx_s2s_step_word_lm_rows(fltx_decoder* dec,
    const void* scores, int32_t dtype, int32_t kind, int64_t row_stride,
    const void* lm_scores, int32_t lm_dtype, int32_t lm_kind, int64_t lm_row_stride,
    const int32_t* lm_row_of, int32_t n_lm_rows,
    int32_t on_device, const uint8_t* row_valid, double* row_lse, double* lm_row_lse,
    int32_t* next_token, int32_t* next_beam_idx, int32_t* next_src_row, int32_t* next_word, int32_t* n_rows);
/* *done = 1 when every utterance is done (no live hypothesis, or max_output_length steps); synchronises. */
FLTX_API int fltx_s2s_done(fltx_decoder* dec, int32_t* done);
/* The back-trace (:152-163): every utterance's final beam -- the last non-empty one, which may hold unfinished
 * hypotheses -- becomes the decoder's results. */
FLTX_API int fltx_s2s_end(fltx_decoder* dec);

/* ---- seq2seq: finish and restart single utterances of a running batch ------------------------------------------------
 * Autoregressive utterances end after very different numbers of steps, and the model runs on the rows the step lists:
 * fltx_s2s_finish ends the utterances of the slots `which` names (a HOST array of B: 0 leave, 1 finish + restart,
 * 2 finish + park), hands out their n-best and restarts or parks those slots, in one call, and leaves every other
 * utterance alone.  Both seq2seq kinds, every LM (ZeroLM / n-gram, token rows, word rows).  Every slot counts its own
 * steps: max_output_length holds per utterance, from its (re)start, whatever the batch has done before.
 *
 * A named slot b first gets fltx_s2s_end's back-trace for that utterance alone: its last non-empty beam, which may hold
 * unfinished hypotheses -- naming a running utterance aborts it.  Rows and scores are bit for bit what fltx_s2s_end would
 * have written for it; they go into result buffers of the finish's own, and fltx_result_* keep returning what they
 * returned before the call.  An utterance that had stopped (lexicon kind: state table full) is finished as fltx_s2s_end
 * finishes it: status[b] says why it had stopped.
 * A slot named with 1 is then in exactly the state fltx_s2s_begin leaves an utterance in: the root in the current beam,
 * local step 0, `done` cleared; lexicon kind: the slot's state table empty and its count started over (max_states
 * stays), its status and its merge count (fltx_s2s_lex_info) cleared; word rows: the listed root row's trie node is the
 * root.  Nothing later reads a record of the utterance before.
 * A slot named with 2 is parked: it lists no rows, steps skip it, fltx_s2s_done and fltx_s2s_done_each count it as done,
 * fltx_s2s_end returns n_hyp 0 for it.  A later finish that names a parked slot with 1 restarts it and reports n_hyp 0,
 * steps 0, status 0 for it; naming it with 2 again changes nothing.
 * Of every other slot nothing is written; every later call decides for it, bit for bit, what it would have decided
 * without this call.
 *
 * The lists (DEVICE, as fltx_s2s_step's; next_word: required with a word-level rows LM, else NULL): a restarted slot
 * lists the root as fltx_s2s_begin does -- one row, next_token -1, next_beam_idx -1, next_src_row -1, next_word -1; a
 * parked slot lists none; every other slot lists its current rows again with next_src_row the row itself (b*K + k) --
 * the model's index_select is the identity for it -- and next_token, next_beam_idx and next_word what the last step
 * listed (they are read back from the slot's beam, which holds them).  The call after a finish is a step: the model
 * runs on these lists, a restarted slot's root row with fresh state.
 *
 * Results, in `out`: results_on_device != 0 -- the pointers address HBM, written in the order of the context's stream;
 * nothing crosses PCIe and the call does not wait.  results_on_device == 0 -- pinned host buffers, complete when the
 * call returns: the counts of all B slots cross, then n_hyp * length entries and 3 n_hyp scores of each named slot.
 * Both stay valid until the next finish, fltx_s2s_end or fltx_s2s_begin on this decoder; steps do not disturb them.
 *
 * A call that names nothing is legal and changes nothing: it lists every slot's rows again.
 * fltx_s2s_end after finishes still ends all slots: a restarted slot returns what it has decoded since its restart, a
 * parked slot n_hyp 0.
 * FLTX_ERR_STATE before fltx_s2s_begin, after fltx_s2s_end, and on every kind that is not seq2seq.  FLTX_ERR_INVALID on a
 * NULL which, list or out, a which entry outside 0..2, and a NULL next_word on a word-rows decoder. */
typedef struct fltx_s2s_finished_out {
  const int32_t* n_hyp;   /* [B] 0 for a slot not named and for a parked slot */
  const int32_t* steps;   /* [B] local steps the finished utterance took; 0 for a slot not named */
  const int32_t* status;  /* [B] 0, or the FLTX_ERR_* fltx_result_count would report after fltx_s2s_end */
  const double* scores;   /* [B*K*3] score, emitting-model score, LM score */
  const int32_t* tokens;  /* hypothesis k of slot b at (b*K + k) * length, right-aligned, -1 in front, as fltx_s2s_end */
  const int32_t* words;   /* likewise; NULL for the lexicon-free kind */
  int32_t length;         /* max_output_length + 3 */
} fltx_s2s_finished_out;
FLTX_API int fltx_s2s_finish(fltx_decoder* dec, const int32_t* which, int32_t* next_token, int32_t* next_beam_idx,
                             int32_t* next_src_row, int32_t* n_rows, int32_t* next_word, int32_t results_on_device,
                             fltx_s2s_finished_out* out);
/* done[b] (HOST, B entries) = 1 when the utterance in slot b is done or the slot is parked: fltx_s2s_done per slot (one
 * copy; synchronises).  What a server names in fltx_s2s_finish. */
FLTX_API int fltx_s2s_done_each(fltx_decoder* dec, int32_t* done);

/* ---- seq2seq: LexiconSeq2SeqDecoder as a batched device step --------------- */
/* LexiconSeq2SeqDecoderOptions (decoder/LexiconSeq2SeqDecoder.h:23-31). */
typedef struct fltx_s2s_lex_options {
  int32_t beam_size;
  int32_t beam_size_token;
  double beam_threshold;
  double lm_weight;
  double word_score;
  double eos_score;
  int32_t log_add; /* how merged hypotheses combine: logAdd of their scores, else the max */
} fltx_s2s_lex_options;

/* LexiconSeq2SeqDecoder(opt, lexicon, lm, eos, emittingModelUpdateFunc, maxOutputLength, isLmToken)
 * (decoder/LexiconSeq2SeqDecoder.h:116-133, .cpp:20-231) for B utterances at once: an attention model's output
 * constrained to the spellings of `trie` (a host trie, already smeared; copied into a compact device layout -- per node
 * its maxScore, labels and children sorted by token, bytes proportional to nodes + edges -- so the trie may be
 * destroyed afterwards), whole words scored by `lm` over word ids (token ids when is_lm_token != 0).  The decoder runs
 * through fltx_s2s_begin / step / done / end with the lexicon-free decoder's row contract (next_beam_idx: the parent's
 * index in the previous beam), and its results carry words (fltx_result_*: the word a hypothesis ended at a token, -1
 * elsewhere).  Candidates in one LM state, trie node and token merge exactly as candidatesStore does (Utils.h:146-225:
 * max, or logAdd when log_add != 0).
 * Limits (FLTX_ERR_UNSUPPORTED beyond them; there is no CPU fallback): beam_size <= 256, V <= 65 536,
 * max_output_length <= 4 096, min(beam_size_token, V) <= 256 (fltx_s2s_begin, with any LM).  `lm`: ZeroLM, n-gram
 * tables, with is_lm_token != 0 a rows LM (fltx_lm_rows_create: a neural token LM; the decoder then steps with
 * fltx_s2s_step_lm_rows, which describes the candidates; the LM must be a pure function of the token prefix), or with
 * is_lm_token == 0 a word-level rows LM (fltx_lm_word_rows_create: a neural word LM; the decoder steps with
 * fltx_s2s_step_word_lm_rows; a pure function of the word prefix).  A host LM, a fltx_lm_rows_create LM with
 * is_lm_token == 0 and a fltx_lm_word_rows_create LM with is_lm_token != 0 are refused.  Each utterance names its LM
 * states in a table of min(beam_size * max_output_length + 1, max_states) entries (max_states: 65 536, or fltx_s2s_lex_set_max_states); an utterance that needs more stops, and
 * fltx_result_count reports FLTX_ERR_UNSUPPORTED ("LM-state table full") for it. */
FLTX_API int fltx_s2s_lex_decoder_create(fltx_ctx* ctx, const fltx_s2s_lex_options* opt, const fltx_htrie* trie,
                                         const fltx_lm* lm, int32_t eos, int32_t max_output_length,
                                         int32_t is_lm_token, fltx_decoder** out);
/* LM states per utterance from the next fltx_s2s_begin on (>= 1). */
FLTX_API int fltx_s2s_lex_set_max_states(fltx_decoder* dec, int32_t max_states);
/* The device trie's bytes, nodes and edges; merges (may be NULL, else B entries, valid after fltx_s2s_begin): the
 * candidates of each utterance folded into another since fltx_s2s_begin (synchronises). */
FLTX_API int fltx_s2s_lex_info(fltx_decoder* dec, int64_t* trie_bytes, int64_t* n_nodes, int64_t* n_edges,
                               int32_t* merges);

/* ---- lexicon-free CTC with a rows LM: LexiconFreeDecoder as a batched device step per frame ----------------------- */
/* LexiconFreeDecoder(opt, lm, sil, blank, {}) (decoder/LexiconFreeDecoder.h:102-112, .cpp:20-158) for B utterances at once
 * with a neural token LM in shallow fusion: `lm` is a rows LM (fltx_lm_rows_create: lm_width, usr_to_lm, and a
 * finish_index >= 0 -- CTC has no eos token whose entry LM::finish could default to).  The LM stays the caller's: between
 * two frame steps it runs on the device and hands in one row of lm_width scores per LM STATE.  A decoder kind of its own
 * (FLTX_DECODER_CTC_ROWS): fltx_decoder_create keeps refusing rows LMs; fltx_decode_batch, fltx_stream_* and fltx_s2s_* on
 * this decoder, and fltx_ctc_rows_* on any other, return FLTX_ERR_STATE; fltx_group_create refuses the kind.  Any other
 * LM (a word-level rows LM included) and the ASG criterion: FLTX_ERR_UNSUPPORTED.  word_score and unk_score are ignored.
 * The caller's obligation is fltx_lm_rows_create's: the LM is a pure function of the token prefix -- here the token
 * string CTC collapses a path to.
 * Limits (FLTX_ERR_UNSUPPORTED beyond them; there is no CPU fallback): beam_size <= 256, N <= 65 536,
 * min(beam_size_token, N) <= 256.  Each utterance names its LM states in a table of min(beam_size * max T + 2,
 * max_states) entries (max_states: 65 536, or fltx_decoder_set(dec, "max_states", n) before fltx_ctc_rows_begin); an
 * utterance that needs more stops, and fltx_result_count reports FLTX_ERR_UNSUPPORTED ("LM-state table full") for it.
 * (A stream -- fltx_ctc_rows_stream_begin -- holds max_states ids and gets dead ones back through
 * fltx_ctc_rows_stream_collect.) */
FLTX_API int fltx_ctc_rows_decoder_create(fltx_ctx* ctx, const fltx_options* opt, const fltx_lm* lm, int32_t sil,
                                          int32_t blank, fltx_decoder** out);
/* decodeBegin (:20-28) for B utterances.  Emissions as for fltx_decode_batch: float32, utterance b reads T[b]*N floats
 * (frame-major) at emissions + offsets[b] (offsets NULL: one after the other); offsets and T are host arrays.  A host
 * buffer (on_device == 0) is copied before the call returns.  A DEVICE buffer is read by this call alone -- the token
 * beams of all frames are taken here, on the context's stream -- but must stay valid and unchanged until
 * fltx_ctc_rows_end has been queued: a later begin may read it again.  FLTX_ERR_INVALID when the LM's map has fewer than
 * N entries, a token's LM index or the finish index lies outside the LM's rows, or finish_index < 0.
 * Row lists are caller-owned DEVICE buffers of B*K int32 (K = beam_size), n_rows of B: row b*K + k is hypothesis k of
 * utterance b's current beam (every hypothesis is live in CTC); entries k >= n_rows[b] are padding (-1).  For each row:
 *   next_src_row  the parent's row in the call that produced it (-1 for the root);
 *   next_token    the token that advanced the LM state in this frame, -1 when the state is the parent's (a blank, or a
 *                 repeat without a blank in between); the root lists sil;
 *   next_state    the hypothesis' canonical LM-state id within its utterance (the root's: 0), stable for the whole decode
 *                 (in a stream: until fltx_ctc_rows_stream_collect lists it as released):
 *                 two rows with the same id are in the same LM state, and the same id at a later frame is that state again
 *                 -- a caller keeps one LM row per id and runs the LM only for ids it has not seen (the new state is the
 *                 state of row next_src_row advanced by next_token).
 * This call lists one row per utterance: the root. */
FLTX_API int fltx_ctc_rows_begin(fltx_decoder* dec, const float* emissions, int32_t on_device, const int64_t* offsets,
                                 const int32_t* T, int32_t B, int32_t N, int32_t* next_token, int32_t* next_src_row,
                                 int32_t* next_state, int32_t* n_rows);
/* fltx_ctc_rows_begin on the emissions as the acoustic model produces them: elements of `dtype` (a fltx_dtype), `kind`
 * FLTX_S2S_LOG_PROBS or FLTX_S2S_LOGITS.  Frame f of utterance b starts at emissions + (offsets[b] + f * frame_stride)
 * ELEMENTS; frame_stride >= N, 0 means N; offsets NULL: utterance b starts at frame_stride times the total of
 * T[0 .. b-1].  Frames of the 2-byte types need only be 2-byte aligned: an odd N, an odd offset and an odd stride are
 * legal.  The emission of token n in a frame is e[n]: the element widened exactly for log-probs; for logits
 * (float)((double)x_n - lse), lse as fltx_s2s_step_typed defines it over the frame's N elements (an all-NaN frame and a
 * frame whose maximum is -inf have lse = that maximum and no candidates).  Everything fltx_ctc_rows_step and the lexicon
 * kind say about a frame -- the token beam with its ties to the lower token, the three CTC branches, the lexicon kind's
 * blank and same-node candidates, NaN and -inf -- is said about this e; a decode is bit for bit the decode of
 * fltx_ctc_rows_begin on the float32 matrix e.  No float32 copy of the emissions is made, on the device or on the host:
 * a host buffer is staged in its own type (and stride), the token beams are taken from the typed frames in this call
 * (one launch: a wave per frame up to the width fltx_decoder_get(dec, "emissions_narrow_max") reports, a workgroup per
 * frame beyond it; fltx_decoder_set changes the width, 0 .. 1024), and the lexicon step reads its two emissions from the
 * typed buffer with the frame's lse, which the decoder keeps in a buffer of its own.  A DEVICE buffer must stay valid
 * and unchanged as fltx_ctc_rows_begin demands.
 * frame_lse: NULL, or a DEVICE buffer of one double per frame of the call, utterance after utterance (the sum of the
 * T[b]); logits mode writes each frame's lse there, log-probs mode leaves it untouched.
 * FLTX_ERR_INVALID on a bad dtype or kind and on 0 < frame_stride < N; every other refusal is fltx_ctc_rows_begin's.
 * Works on both CTC rows kinds; step, end, plan, the stream calls and the results keep their contracts. */
FLTX_API int fltx_ctc_rows_begin_typed(fltx_decoder* dec, const void* emissions, int32_t dtype, int32_t kind,
                                       int32_t on_device, const int64_t* offsets, int64_t frame_stride,
                                       const int32_t* T, int32_t B, int32_t N, double* frame_lse, int32_t* next_token,
                                       int32_t* next_src_row, int32_t* next_state, int32_t* n_rows);
/* One frame of every utterance that has frames left (:41-123).  lm_scores: n_lm_rows rows of lm_width entries of
 * lm_dtype, row i at lm_scores + i * lm_row_stride ELEMENTS (lm_row_stride >= lm_width); lm_row_of (B*K int32, may be
 * NULL: identity, n_lm_rows taken as B*K) names the LM row of each decoder row -- one LM row can serve many.  An entry
 * outside [0, n_lm_rows) on a live row makes that row's LM entries NaN: it keeps its blank and repeat candidates and has
 * no new-token candidate; nothing is read through it.  Both are device pointers (on_device != 0) or host pointers, staged
 * in their own types.  lm_kind FLTX_S2S_LOG_PROBS: the entry widened exactly; FLTX_S2S_LOGITS: (float)((double)x - lse),
 * lse as fltx_s2s_step_typed defines it; lm_row_lse (may be NULL; B*K doubles on the device, indexed by DECODER row)
 * receives the lse of the LM row each live row names, NaN for the other rows.
 * Per frame and utterance: the token beam is the frame's min(beam_size_token, N) largest emissions (ties to the lower
 * token).  For hypothesis h and kept token n: score = h.score + e[n] (+ sil_score when n == sil); when n != blank and
 * (n != h.token or h.prevBlank) -- a new token -- lm = the entry at usr_to_lm[n] of h's LM row, score += lm_weight * lm
 * (a mul and an add), the state becomes child(state, n); a blank keeps the state and sets prevBlank; a repeat keeps the
 * state.  emittingModelScore and lmScore accumulate separately, also at lm_weight == 0.  Candidates below best -
 * beam_threshold go; candidates equal in (state, token, prevBlank) merge (max, or logAdd when log_add != 0; the best
 * member's fields survive, next_src_row among them); the beam_size best survive, sorted best first.  A NaN score is never
 * a candidate; a -inf LM entry behaves as a -inf emission.
 * An utterance with no frames left keeps its beam and lists it again unchanged (next_src_row the slot itself, next_token
 * -1, the same ids); a step after every utterance's last frame changes nothing (lm_scores may be NULL then).
 * Asynchronous on the context's stream.  FLTX_ERR_INVALID on a bad lm_dtype or lm_kind, lm_row_stride < lm_width, NULL
 * outputs, n_lm_rows < 1 with lm_row_of, or NULL lm_scores while frames are left. */
FLTX_API int fltx_ctc_rows_step(fltx_decoder* dec, const void* lm_scores, int32_t lm_dtype, int32_t lm_kind,
                                int64_t lm_row_stride, const int32_t* lm_row_of, int32_t n_lm_rows, int32_t on_device,
                                double* lm_row_lse, int32_t* next_token, int32_t* next_src_row, int32_t* next_state,
                                int32_t* n_rows);
/* decodeEnd (:127-158) and the back-trace.  The LM rows are given as to fltx_ctc_rows_step, for the rows the last step
 * listed; each hypothesis reads the entry at finish_index of its row: score += lm_weight * lm, the state child(state, -1),
 * the token sil.  Hypotheses in one state merge, the n-best is sorted best first, and fltx_result_* read it in the layout
 * fltx_decode_batch produces: T[b] + 2 tokens per hypothesis (the root's sil, the frames' tokens, decodeEnd's sil), words
 * all -1.  (Ended before an utterance's last frame, its results hold the frames decoded so far.) */
FLTX_API int fltx_ctc_rows_end(fltx_decoder* dec, const void* lm_scores, int32_t lm_dtype, int32_t lm_kind,
                               int64_t lm_row_stride, const int32_t* lm_row_of, int32_t n_lm_rows, int32_t on_device,
                               double* lm_row_lse);

/* ---- lexicon CTC with a rows LM: LexiconDecoder as a batched device step per frame -------------------------------- */
/* LexiconDecoder(opt, lexicon, lm, sil, blank, unk, {}, isLmToken) (decoder/LexiconDecoder.h:117-133, .cpp:21-274) for B
 * utterances at once with a neural LM in shallow fusion: CTC emissions, spellings constrained by `trie` (a host trie,
 * already smeared; copied into the compact device layout of fltx_s2s_lex_decoder_create, so it may be destroyed
 * afterwards), and `lm` a word-level rows LM (fltx_lm_word_rows_create) when is_lm_token == 0 or a token-level one
 * (fltx_lm_rows_create) when is_lm_token != 0; the crossed pairs and every other LM: FLTX_ERR_UNSUPPORTED, as the ASG
 * criterion.  finish_index >= 0 is required for both (FLTX_ERR_INVALID).  unk_score > -inf needs unk >= 0, the unknown
 * word's id (FLTX_ERR_INVALID otherwise, either LM).  Word LM: FLTX_ERR_INVALID when a label of the
 * trie, or unk when opt->unk_score > -inf, has no entry in word_to_lm or an LM index outside [0, lm_width), or when
 * finish_index lies outside; token LM: the map is checked against N at fltx_ctc_rows_begin.  A decoder kind of its own
 * (FLTX_DECODER_LEX_CTC_ROWS), refused where FLTX_DECODER_CTC_ROWS is: fltx_decoder_create, fltx_group_create
 * (FLTX_ERR_UNSUPPORTED), fltx_decode_batch, fltx_stream_*, fltx_s2s_* (FLTX_ERR_STATE).  Limits and the state table
 * (fltx_decoder_set(dec, "max_states", n)) are fltx_ctc_rows_decoder_create's; lm_width <= 2^22 for the word LM.
 *
 * The decoder is stepped with fltx_ctc_rows_begin / step / end; next_state, next_src_row, n_rows, lm_row_of, n_lm_rows,
 * lm_row_lse, typed rows, host staging and the idle steps keep their contract.  next_token is the LM EDGE that made the
 * row's state from the state of row next_src_row: the word id that ended in this frame (word LM, unk included), the token
 * (token LM), -1 where the state is the parent's, -1 for the root at begin.  A DEVICE emissions buffer is read by every
 * step (below): it must stay valid and unchanged until fltx_ctc_rows_end has been queued.
 * Per frame, hypothesis h (trie node, last token, prevBlank) and kept token n with a child c of h's node:
 * s = h.score + e[n] (+ sil_score when n == sil), lexMax = 0 at the root, else maxScore[node];
 *   move      when (h.prevBlank or n != h.token) and c has children: word LM lm = maxScore[c] - lexMax (float; no row is
 *             read; the state stays), token LM lm = the entry at usr_to_lm[n] of h's row (state child(state, n));
 *             score = s + lm_weight * lm; node c;
 *   word end  per label w of c (not when h is at the root and n == h.token): word LM lm = entry(word_to_lm[w]) - lexMax
 *             (float), state child(state, w); token LM the move's entry and state; score = (s + lm_weight * lm) +
 *             word_score; the root, word w;
 *   unknown   when c has no labels and unk_score > -inf: as the word end with unk for w and unk_score.
 * Two more candidates read their emission from the frame itself, not from the token beam: the same node (when not
 * h.prevBlank, or at the root; token sil at the root, else h.token; + sil_score for sil) and blank (prevBlank = 1); state,
 * node and lmScore stay.  Then the threshold, the merge of candidates equal in (LM state, trie node, token, prevBlank)
 * (max / logAdd, the best member's fields survive) and the beam_size best.  NaN and -inf behave as in fltx_ctc_rows_step;
 * an out-of-range lm_row_of entry makes the row's LM entries NaN: it keeps the same-node and blank candidates and, under
 * the word LM, its moves.
 * fltx_ctc_rows_end: if any hypothesis sits at the root only those finish, else all; lm = the entry at finish_index,
 * score = h.score + lm_weight * lm, the state child(state, -1), the token sil.  fltx_result_* return tokens and WORDS in
 * the layout of the lexicon fltx_decode_batch: T[b] + 2 entries per hypothesis, the word where it ended, -1 elsewhere. */
FLTX_API int fltx_ctc_rows_lex_decoder_create(fltx_ctx* ctx, const fltx_options* opt, const fltx_htrie* trie,
                                              const fltx_lm* lm, int32_t sil, int32_t blank, int32_t unk,
                                              int32_t is_lm_token, fltx_decoder** out);

/* ---- streams on the two CTC rows kinds: decodeStep on chunks, getBestHypothesis, prune ------------------------------ */
/* The online half of the Decoder interface (decoder/Decoder.h:40-69) for a decoder of fltx_ctc_rows_decoder_create or
 * fltx_ctc_rows_lex_decoder_create; on any other kind these calls return FLTX_ERR_STATE, and fltx_stream_* keeps
 * returning FLTX_ERR_STATE on these kinds.  All of it runs on the device, asynchronously on the context's stream: every
 * stream counts its own frames there, its history is a ring of max_frames (+ 100, lexicon kind) + 2 rows, and a prune
 * copies nothing.
 *
 * fltx_ctc_rows_stream_begin: decodeBegin for B parallel streams.  No emissions; N, the token beam, sil / blank and the
 * LM's map and finish index are checked as by fltx_ctc_rows_begin, and the root is listed per stream as there.
 * max_frames >= 1 bounds the frames a stream holds between prunes; the lexicon kind gets kLookBackLimit = 100
 * (Utils.h:28) frames on top, which its prune may keep beyond look_back.  The LM-state table of a stream holds max_states
 * entries (fltx_decoder_set(dec, "max_states", n) before this call; 65 536): an id keeps its meaning until
 * fltx_ctc_rows_stream_collect lists it, and a stream that needs more ids than are free stops with the "LM-state table
 * full" status while the others go on.  A stream that never collects hands every id out once.  A begin starts the ids
 * over: nothing is free, the root is id 0. */
FLTX_API int fltx_ctc_rows_stream_begin(fltx_decoder* dec, int32_t B, int32_t N, int32_t max_frames, int32_t* next_token,
                                        int32_t* next_src_row, int32_t* next_state, int32_t* n_rows);
/* The next chunk: T[b] >= 0 frames of stream b (0 is allowed; chunks of unequal lengths are the normal case), laid out
 * as fltx_ctc_rows_begin's emissions.  The token beams of the chunk's frames are taken here.  A host buffer is copied
 * before the call returns; a DEVICE buffer must stay valid and unchanged until the next append, end or begin on this
 * decoder has been queued (the lexicon step reads the blank and same-node emissions from it).  Then fltx_ctc_rows_step,
 * max_b T[b] times, consumes the chunk: each call decodes one frame of every stream that still has frames of it, and a
 * stream without lists its beam again unchanged, exactly as an exhausted utterance of a batch does.
 * FLTX_ERR_RANGE when a stream's buffered frames plus the new ones exceed its bound (the host counts an upper bound --
 * look_back, + 100 for the lexicon kind, after a prune -- and asks the device only when that would not fit);
 * FLTX_ERR_STATE while frames of the previous chunk are unstepped, outside a stream, and on a decoder begun with
 * fltx_ctc_rows_begin; FLTX_ERR_INVALID on a negative T[b]. */
FLTX_API int fltx_ctc_rows_stream_append(fltx_decoder* dec, const float* emissions, int32_t on_device,
                                         const int64_t* offsets, const int32_t* T);
/* fltx_ctc_rows_stream_append on a typed chunk, laid out and read as fltx_ctc_rows_begin_typed's emissions; frame_lse
 * (NULL, or one double per frame of the CHUNK on the device, stream after stream) as there.  Each append names its own
 * dtype, kind and stride: a stream may change them from chunk to chunk and may mix these appends with
 * fltx_ctc_rows_stream_append.  A host chunk is staged in its own type before the call returns; a DEVICE chunk must stay
 * valid and unchanged until the next append, end or begin has been queued.  FLTX_ERR_INVALID on a bad dtype or kind and
 * on 0 < frame_stride < N; every other refusal is fltx_ctc_rows_stream_append's. */
FLTX_API int fltx_ctc_rows_stream_append_typed(fltx_decoder* dec, const void* emissions, int32_t dtype, int32_t kind,
                                               int32_t on_device, const int64_t* offsets, int64_t frame_stride,
                                               const int32_t* T, double* frame_lse);
/* prune(lookBack) of every stream (LexiconFreeDecoder.cpp:205-227, LexiconDecoder.cpp:304-325), no host
 * synchronisation.  findBestAncestor (Utils.h:268-310): from the first best of the current beam (strict >) look_back
 * frames up, for the lexicon kind further while the hypothesis is not complete (its parent ended no word), look_back + 100
 * steps at most; that updated look-back is what stays buffered.  Nothing happens with too few frames.  pruneAndNormalize
 * (Utils.h:312-342): the largest score of the CURRENT beam is subtracted from the current beam's scores only; the
 * emitting-model and LM scores stay, and older frames keep the scores they had -- fltx_result_best(look_back > 0) after a
 * prune shows them, as the reference does.  FLTX_ERR_INVALID on look_back < 0. */
FLTX_API int fltx_ctc_rows_stream_prune(fltx_decoder* dec, int32_t look_back);
/* Give back the LM-state ids of every stream that no later step can meet again, so that a stream of any length runs in
 * a table of max_states ids and the caller keeps a bounded number of LM rows.  With R the next_state ids of the stream's
 * current beam plus, transitively, every id whose (parent id, edge) table entry has its parent in R, an allocated id is
 * kept while it is in R or is the parent id a hypothesis of the current beam was made from (merge keys still compare
 * that number); every other allocated id is dead.  Per stream the lowest release_cap dead ids are released -- the rest
 * at a later call -- and listed ascending in released[b * release_cap ..], -1 behind them; n_released[b] is their count
 * and n_live[b] (may be NULL) the ids still allocated after the call.  All three are DEVICE buffers.  A released id may
 * be handed out again by a later step for a DIFFERENT state: the caller drops the LM row it kept for it, and an id a
 * later row list shows that the caller does not hold is a new state -- that of row next_src_row advanced by next_token,
 * as always.  Ids not listed keep their meaning, and every later step decides what it would have decided without the
 * call.  A stream that has stopped (a full table, an empty beam) is left alone: n_released[b] = 0, its status stays.
 * May be called wherever fltx_ctc_rows_stream_prune may, also between an append and its steps; asynchronous on the
 * context's stream, nothing is copied to the host.  FLTX_ERR_STATE outside a stream, on a decoder begun with
 * fltx_ctc_rows_begin and on any other kind; FLTX_ERR_INVALID on release_cap < 1 or NULL released / n_released. */
FLTX_API int fltx_ctc_rows_stream_collect(fltx_decoder* dec, int32_t release_cap, int32_t* released,
                                          int32_t* n_released, int32_t* n_live);
/* ---- the LM rows of a CTC rows decode, planned on the device ---------------------------------------------------------
 * What connects the row lists to the caller's LM: which states of a list are new, the row of the LM-row store each
 * gets, the row of its parent and the edge that advanced it, and the next step's lm_row_of.  Per decoder the planner
 * keeps the LM row of every state id (-1: none yet, -2: dropped), a stack of free rows, a high-water mark and the
 * lm_row_of of the call before.  Everything runs on the context's stream; nothing is copied to the host.  A decoder that
 * never calls fltx_ctc_rows_plan_begin steps exactly as before.
 *
 * fltx_ctc_rows_plan_begin: after fltx_ctc_rows_begin or fltx_ctc_rows_stream_begin and before the first plan; sizes and
 * clears the tables for that decode's B and state ids, for a store of row_capacity rows.  FLTX_ERR_INVALID on
 * row_capacity < 1; FLTX_ERR_STATE outside a begun decode and on any other decoder kind.  The next begin ends planning
 * until the next fltx_ctc_rows_plan_begin. */
FLTX_API int fltx_ctc_rows_plan_begin(fltx_decoder* dec, int32_t row_capacity);
/* Plan the list the last begin / step wrote (the four device lists, unchanged).  The outputs are caller-owned DEVICE
 * buffers of B*K int32, counts of 4.  The result is that of this loop -- a function of the call sequence alone:
 *   for b ascending, k < n_rows[b] ascending, s = next_state[b*K + k]:
 *     s outside the decode's ids: lm_row_of = -1 (nothing is read through it);
 *     s has no row yet -- a NEW state, listed once, at its lowest k (two rows of a list can carry the same new state):
 *       r = the top of the free stack, else high_water++ while high_water < row_capacity, else the state is DROPPED;
 *       a new state with a row is entry i = n_new++ of the lists:  new_row[i] = r,  new_parent_row[i] = the lm_row_of
 *       the PREVIOUS plan gave row next_src_row (-1 for a root),  new_edge[i] = next_token (-1 for a root),
 *       new_dec_row[i] = b*K + k;
 *     lm_row_of[b*K + k] = the state's row, -1 for a dropped state.
 *   rows k >= n_rows[b] and list entries >= n_new: -1.
 *   counts = {n_new, high_water, rows on the free stack, states dropped since fltx_ctc_rows_plan_begin}.
 * The caller runs its LM for the n_new listed states, writes row new_row[i] of its store and passes lm_row_of and
 * n_lm_rows = row_capacity to the next fltx_ctc_rows_step / _end.  A dropped state stays dropped until its id is
 * released: its rows read -1, so by the step's contract their LM entries are NaN, it keeps its blank / repeat / same-node
 * candidates and makes no child state -- a parent always has a row.
 * FLTX_ERR_INVALID on a NULL pointer.  FLTX_ERR_STATE without fltx_ctc_rows_plan_begin; when a step was queued whose list
 * was never planned (the parent rows would be wrong); when this list has been planned already; and when a
 * fltx_ctc_rows_stream_collect was queued without a fltx_ctc_rows_plan_release after it. */
FLTX_API int fltx_ctc_rows_plan(fltx_decoder* dec, const int32_t* next_token, const int32_t* next_src_row,
                                const int32_t* next_state, const int32_t* n_rows, int32_t* lm_row_of, int32_t* new_row,
                                int32_t* new_parent_row, int32_t* new_edge, int32_t* new_dec_row, int32_t* counts);
/* Tell the planner what a fltx_ctc_rows_stream_collect released: its DEVICE outputs released / n_released and its
 * release_cap, unchanged, once per collect.  For each stream b ascending, each listed id in listed order: the id's row,
 * if it has one, goes on the free stack; the id is unplanned again (a dropped id too).  FLTX_ERR_STATE outside a stream
 * or without fltx_ctc_rows_plan_begin; FLTX_ERR_INVALID on NULL or release_cap < 1. */
FLTX_API int fltx_ctc_rows_plan_release(fltx_decoder* dec, const int32_t* released, const int32_t* n_released,
                                        int32_t release_cap);
/* ---- finish and restart single streams of a stream batch -------------------------------------------------------------
 * Sessions start and stop at different times: fltx_ctc_rows_stream_finish ends the utterances of the streams `which`
 * names (a HOST array of B, != 0: named) and restarts those slots from the root, in one call, and leaves every other
 * stream alone.
 *
 * A named stream b first gets exactly fltx_ctc_rows_end's decodeEnd: the entry at finish_index of each hypothesis' LM row
 * (lexicon kind: only the hypotheses at the root finish, if there are any), merge, sort best first, the walk back over
 * the frames in the buffer by count -- frames in buffer + 1 entries per hypothesis.  The LM rows are passed as to
 * fltx_ctc_rows_end, for the rows the last call listed; only rows of named streams are read (through lm_row_of or not),
 * lm_row_lse is written for those rows only, and lm_scores may be NULL when no stream is named.  A stream that had stopped
 * (table full, empty beam) is finished as fltx_ctc_rows_end finishes it: status[b] says why it had stopped.
 * Then, in the same call, slot b is in exactly the state fltx_ctc_rows_stream_begin leaves a stream in: no frames decoded
 * and none pruned, the root in the beam, its scores in the score ring, the LM-state ids started over (root id 0, nothing
 * free, the stream's table empty), status and the stopped flag cleared, the host's frame bound for append back to zero.
 * max_frames, max_states and the rings' size stay; the rings are not cleared, and nothing reads a row of the utterance
 * before.
 * Of every other stream nothing is written and only the current beam's state ids are read; every later call decides for
 * it, bit for bit, what it would have decided without this call.
 *
 * The four lists (DEVICE, as fltx_ctc_rows_step's): a named stream lists its root as fltx_ctc_rows_stream_begin does --
 * one row, next_src_row -1, next_state 0, next_token sil (-1: lexicon kind); every other stream lists its beam again as
 * a step without frames does -- next_src_row the slot itself, next_token -1, the same ids.
 *
 * With fltx_ctc_rows_plan_begin in force the named streams' LM rows go back to the planner in the same call, on the
 * device: streams ascending, within a stream ids ascending, a row an id has goes on the free stack, and every id of the
 * stream is unplanned (the dropped ones too; the count of dropped states stays).  The finish's list is then planned like
 * any other list before the next step: the root is a new state with new_parent_row -1 and new_edge -1.
 *
 * Results, in `out`: results_on_device != 0 -- the pointers address HBM, written in the order of the context's stream;
 * nothing crosses PCIe, and tokens / words / row_off / length are valid inputs of fltx_collapse_rows.
 * results_on_device == 0 -- pinned host buffers, complete when the call returns (the only case in which it waits): the
 * counts of all B streams cross, then n_hyp * length entries and 3 n_hyp scores of each named stream.  Both stay valid
 * until the next finish, fltx_ctc_rows_end or begin on this decoder; steps, appends, prunes, collects and
 * fltx_result_best do not disturb them, and fltx_result_* keep returning what they returned before the call.
 *
 * A call that names no stream is legal, reads no LM row and changes nothing: it lists every beam again.
 * FLTX_ERR_STATE outside a rows stream, on a decoder begun with fltx_ctc_rows_begin, on every other kind, while frames
 * of the last chunk are unstepped, and -- with planning active -- when a fltx_ctc_rows_stream_collect was queued without
 * its fltx_ctc_rows_plan_release.  FLTX_ERR_INVALID on a NULL which, list or out, and, when a stream is named, on a bad
 * lm_dtype or lm_kind, lm_row_stride < lm_width or NULL lm_scores. */
typedef struct fltx_finished_out {
  const int32_t* n_hyp;   /* [B]  0 for a stream the call did not name */
  const int32_t* length;  /* [B]  entries per hypothesis = frames in buffer + 1; 0 for a stream not named */
  const int32_t* status;  /* [B]  0, or the FLTX_ERR_* fltx_result_count would report for it after fltx_ctc_rows_end */
  const double* scores;   /* [B*K*3] score, emitting-model score, LM score, as fltx_result_fetch_batch */
  const int32_t* tokens;  /* hypothesis k of stream b: row_off[b] + k * length[b] */
  const int32_t* words;   /* likewise; NULL for the lexicon-free kind */
  const int64_t* row_off; /* [B] fixed for the life of the stream batch */
} fltx_finished_out;
FLTX_API int fltx_ctc_rows_stream_finish(fltx_decoder* dec, const int32_t* which, const void* lm_scores,
                                         int32_t lm_dtype, int32_t lm_kind, int64_t lm_row_stride,
                                         const int32_t* lm_row_of, int32_t n_lm_rows, int32_t on_device,
                                         double* lm_row_lse, int32_t* next_token, int32_t* next_src_row,
                                         int32_t* next_state, int32_t* n_rows, int32_t results_on_device,
                                         fltx_finished_out* out);
/* The same for the classic streams (fltx_stream_begin / _step / _prune / _end on FLTX_DECODER_LEXFREE and
 * FLTX_DECODER_LEXICON): fltx_stream_finish ends the utterances of the streams `which` names (a HOST array of B, != 0:
 * named) and restarts those slots, in one call, and leaves every other stream alone.
 *
 * First the call settles what fltx_stream_end settles: the look at a pending optimistic lexicon chunk (its second pass
 * included) and a prune deferred behind it.  A named stream b then gets exactly fltx_stream_end's decodeEnd and the
 * back-trace over the frames in its buffer: n_hyp[b], length[b], the token rows, the word rows and the three scores of
 * each hypothesis are, entry for entry and bit for bit, what fltx_result_count and fltx_result_fetch return for the stream
 * after fltx_stream_end at the same point (length = that call's length); status[b] is 0 or the FLTX_ERR_* that
 * fltx_result_count would report (n_hyp[b] is then 0).
 * Then, in the same call, slot b is in exactly the state fltx_stream_begin leaves a stream in: the root in the beam and
 * at the first history row, no frames decoded and none pruned (fltx_stream_partials: first_frame 0), status cleared, the
 * LM-state ids started over (root id 0; the stream's own part of the state table and of the LM score cache emptied), the
 * host's frame count for max_frames back to zero.  max_frames stays.
 * Of every other stream nothing observable changes: every later fltx_stream_step, _prune, _end, fltx_result_best,
 * fltx_stream_partials and fltx_stream_frames_in_buffer returns for it, bit for bit, what it would have returned without
 * the call, and fltx_result_* serve the live streams as before.
 *
 * Results, in `out` (the struct above; words NULL for the lexicon-free kind; row_off fixed for the life of the stream
 * batch): results_on_device != 0 -- the pointers address HBM, written in the order of the context's stream; no result
 * crosses PCIe and the call does not wait for the device; tokens / words / row_off / length are valid inputs of
 * fltx_collapse_rows.  results_on_device == 0 -- pinned host buffers, complete when the call returns: the counts of all B
 * streams cross, then n_hyp * length entries and 3 n_hyp scores of each named stream.  The buffers are the finish's own
 * and stay valid until the next finish, fltx_stream_end or fltx_stream_begin on this decoder.
 *
 * A call that names no stream is legal and changes nothing; one that names all B equals fltx_stream_end followed by
 * fltx_stream_begin.  FLTX_ERR_STATE outside a stream, after fltx_stream_end and on the step kinds; FLTX_ERR_INVALID on
 * a NULL which or out; FLTX_ERR_UNSUPPORTED on a decoder whose LM is a host LM (fltx_lm_host_create): its states are the
 * callee's and its start / retain protocol is per decoder -- left for later; end and begin all streams together. */
FLTX_API int fltx_stream_finish(fltx_decoder* dec, const int32_t* which, int32_t results_on_device,
                                fltx_finished_out* out);
/* nDecodedFramesInBuffer of stream b (synchronises). */
FLTX_API int fltx_ctc_rows_stream_frames_in_buffer(fltx_decoder* dec, int32_t b, int32_t* n);
/* Inside such a stream fltx_result_best(dec, b, look_back, ...) is getBestHypothesis(lookBack): the ancestor's score,
 * emitting-model score and LM score, its tokens (and words, lexicon kind), length = frames in buffer - look_back'; an
 * empty result (LexiconDecoder.cpp:286 included) has length 0.  One launch answers all B streams, and the answer is kept
 * until the next step, append or prune.  fltx_ctc_rows_end finishes the stream: frames in buffer + 1 entries per
 * hypothesis -- the buffer's first frame first (the root's sil only if nothing was pruned), decodeEnd's sil last -- read
 * with fltx_result_* as a batch's. */

/* ---- results (getAllFinalHypothesis / getBestHypothesis) ------------------ */
/* Number of hypotheses of utterance b and the length (finalFrame + 1) of each
 * tokens/words vector (decoder/Utils.h:236-247). */
FLTX_API int fltx_result_count(fltx_decoder* dec, int32_t b, int32_t* n_hyp,
                               int32_t* length);
/* Copy out the first max_hyp hypotheses of utterance b, best first:
 * scores[3*i + {0,1,2}] = score, emittingModelScore, lmScore
 * (decoder/Utils.h:30-39); tokens/words [i*length + f]; either may be NULL. */
FLTX_API int fltx_result_fetch(fltx_decoder* dec, int32_t b, int32_t max_hyp,
                               double* scores, int32_t* tokens, int32_t* words,
                               int32_t* n_copied);
/* The whole batch's n-best in one PCIe transfer per array (offline decodes):
 * counts, scores and token / word rows are copied into pinned host buffers
 * owned by the decoder and pointers to them are returned; they stay valid
 * until the next decode on this decoder.  Hypothesis k of utterance b:
 * scores[(b * beam_size + k) * 3 + {0,1,2}] = score, emitting-model score, LM
 * score; tokens + offsets[b] + k * length[b] holds its length[b] tokens (words
 * likewise; *words is NULL for the lexicon-free decoder, whose word sequence
 * is all -1, LexiconFreeDecoder.h:80-82).  Replaces a loop of
 * getAllFinalHypothesis() calls (Decoder.h:71-73) over the utterances. */
FLTX_API int fltx_result_fetch_batch(fltx_decoder* dec, const int32_t** n_hyp, const int32_t** length,
                                     const double** scores, const int32_t** tokens, const int32_t** words,
                                     const int64_t** offsets);
/* The same, compacted on the device first so that only what exists crosses PCIe: the rows of the n_hyp[b]
 * hypotheses an utterance really has (a lexicon beam of 100 returns a dozen), tokens as bytes (0xFF = -1;
 * token sets of up to 254 symbols -- FLTX_ERR_UNSUPPORTED beyond: use fltx_result_fetch_batch), words as
 * int32 rows.  Hypothesis k of utterance b: tokens_u8 + offsets[b] + k * length[b] (words likewise, NULL for
 * the lexicon-free decoder); scores as fltx_result_fetch_batch.  C4's batch of 256: 308 MB -> 23 MB.
 * Replaces the same loop of getAllFinalHypothesis() calls (Decoder.h:71-73). */
FLTX_API int fltx_result_fetch_batch_compact(fltx_decoder* dec, const int32_t** n_hyp, const int32_t** length,
                                             const double** scores, const uint8_t** tokens_u8,
                                             const int32_t** words, const int64_t** offsets);
/* ---- collapsed transcripts ------------------------------------------------ */
/* What a caller wants of a CTC / ASG n-best is rarely its frame rows (T[b] + 2 tokens per hypothesis, a word row that is
 * -1 except where a word ended) but the transcript: the tokens after CTC collapse, the frame at which each starts, the
 * words and their frames.  These two calls collapse frame rows on the device (text_amd/csrc/fltx_transcript.h), so
 * that only the transcript -- ten to a hundred times smaller -- crosses PCIe, or nothing at all.
 *
 * The rule, for one row tok[0 .. len) with an optional wrd[0 .. len) and a blank id (blank < 0: nothing is a blank):
 *   position i is kept iff tok[i] >= 0, tok[i] != blank and (i == 0 or tok[i] != tok[i - 1]) -- the RAW previous
 *   entry: a blank or a -1 between two equal tokens makes the second one a new token;
 *   a kept position yields (tokens, timesteps) = (tok[i], i);
 *   every position with wrd[i] >= 0 yields (words, word_timesteps, word_tok_end) = (wrd[i], i, kept positions <= i),
 *   so tokens[word_tok_end[j - 1] .. word_tok_end[j]) of the row is the spelling that ended word j, with its leading
 *   separators.
 * (The host-side groupby / drop-blank / first-index rule.  In a decoder's rows entry 0 is the root's sil: the emission
 * frame of a token is timestep - 1.)
 *
 * Row r's tokens / timesteps are at [tok_off[r], tok_off[r + 1]), its words / word_timesteps / word_tok_end at
 * [word_off[r], word_off[r + 1]).  on_device == 0: the arrays are copied into pinned host buffers, one transfer per
 * array.  on_device != 0: the pointers address HBM (in the order of the context's stream) and only the two totals
 * cross PCIe.  The buffers belong to the context (fltx_collapse_rows) or the decoder (fltx_result_transcripts), grow
 * as needed and stay valid until the next such call on it, or the next decode. */
typedef struct fltx_transcripts {
  int64_t n_rows;
  const int64_t* row_first;      /* [B + 1] rows of utterance b: row_first[b] .. row_first[b+1]  (decoder call; NULL for fltx_collapse_rows) */
  const double*  scores;         /* [B*K*3] as fltx_result_fetch_batch  (decoder call; NULL otherwise) */
  const int64_t* tok_off;        /* [n_rows + 1] */
  const int32_t* tokens;         /* [tok_off[n_rows]] */
  const int32_t* timesteps;
  const int64_t* word_off;       /* [n_rows + 1]; all 0 without a word row */
  const int32_t* words, *word_timesteps, *word_tok_end;
  int64_t n_tokens, n_words;     /* = tok_off[n_rows], word_off[n_rows]: the two totals, on the host either way */
} fltx_transcripts;
/* Any frame rows in HBM: row r = row_len[r] entries at element offset row_off[r] of tokens (and of words, which may be
 * NULL); all four are device pointers.  n_rows == 0 or all lengths 0 give empty arrays; a negative row_len is
 * FLTX_ERR_INVALID. */
FLTX_API int fltx_collapse_rows(fltx_ctx* ctx, const int32_t* tokens, const int32_t* words, const int64_t* row_off,
                                const int32_t* row_len, int64_t n_rows, int32_t blank, int32_t on_device,
                                fltx_transcripts* out);
/* The n-best of the last finished decode (fltx_decode_batch, or fltx_ctc_rows_end -- of a stream too): the first
 * min(n_hyp[b], max_hyp) hypotheses of every utterance, best first, with the decoder's own blank (under the ASG
 * criterion nothing is a blank); n_hyp / length and the errors of an utterance's status as fltx_result_fetch_batch_compact,
 * token sets of any size.  FLTX_ERR_STATE without a finished decode and on the seq2seq kinds (their results are token
 * strings already), FLTX_ERR_INVALID on max_hyp < 1.  The other fetch calls return what they return without it. */
FLTX_API int fltx_result_transcripts(fltx_decoder* dec, int32_t max_hyp, int32_t on_device, fltx_transcripts* out);
/* getBestHypothesis(lookBack) of stream b (LexiconFreeDecoder.cpp:188-194,
 * decoder/Utils.h:268-310): *length = 0 for an empty result. */
FLTX_API int fltx_result_best(fltx_decoder* dec, int32_t b, int32_t look_back,
                              double* scores, int32_t* tokens, int32_t* words,
                              int32_t capacity, int32_t* length);
/* ---- partial transcripts of all streams ----------------------------------- */
/* What a streaming recogniser shows after every chunk, for all B streams in one call: row b of `t` is the frame row
 * fltx_result_best(dec, b, look_back, ...) returns (findBestAncestor, with the lexicon kinds' walk on to a complete
 * hypothesis and their empty result while frames in buffer - 1 - look_back < 1), collapsed on the device by the rule
 * above fltx_transcripts with the decoder's own blank (under the ASG criterion nothing is a blank).  Buffer entry 0 is
 * the root's sil, or the hypothesis the last prune kept: like any other entry it is listed if it is not a blank, so a
 * client that concatenates across prunes counts absolute entry first_frame[b] + i once.
 *
 * stable_frames[b]: with anc(h, j) the ancestor at buffer frame j of a hypothesis h of the current beam, 1 + the largest j
 * at which anc(h, j) is one and the same hypothesis for every h -- every later hypothesis descends from the current
 * beam, so entries [0, stable_frames) of the row can no longer change; 0 if there is no such j (after a prune buffer
 * frame 0 can hold several parentless hypotheses) and for an empty beam, frames in buffer for a beam of one; independent
 * of look_back.  stable_tokens / stable_words count the row's tokens / words at timesteps below
 * min(stable_frames, length).
 *
 * Valid inside a stream: after fltx_stream_begin on the lexicon-free and lexicon decoders, after
 * fltx_ctc_rows_stream_begin on the two CTC rows decoders where fltx_result_best is valid; FLTX_ERR_STATE elsewhere
 * (offline decodes, the seq2seq kinds, a rows decoder begun with fltx_ctc_rows_begin), FLTX_ERR_INVALID on look_back < 0
 * or a NULL out.  A stream that has stopped is no error of the call: its row is empty, length[b] = 0 and status[b] says
 * why.  One launch for all streams, then the transcript's scan and write; the number of launches and copies does not
 * depend on B.  on_device == 0: every array lands in the decoder's pinned buffers.  on_device != 0: the pointers address
 * HBM in the order of the context's stream and only the two totals cross PCIe.  The buffers stay valid until the next
 * call on the decoder that steps, appends, prunes or asks again. */
typedef struct fltx_stream_partials_out {
  fltx_transcripts t;            /* n_rows = B, row b = stream b; t.scores = [B*3] score / emitting-model / LM score of the
                                    ancestor (as fltx_result_best); t.row_first = NULL */
  const int32_t* length;         /* [B] frames of the result = what fltx_result_best would return in *length; 0: empty */
  const int32_t* stable_frames;  /* [B] leading buffer entries that every hypothesis of the current beam shares */
  const int32_t* stable_tokens;  /* [B] tokens of row b that lie inside them (timestep < stable_frames[b]) */
  const int32_t* stable_words;   /* [B] likewise for words (word_timesteps) */
  const int64_t* first_frame;    /* [B] frames pruned away so far: buffer entry i is absolute entry first_frame[b] + i */
  const int32_t* status;         /* [B] 0, or the FLTX_ERR_* that fltx_result_best(dec, b, ...) would return for this stream */
} fltx_stream_partials_out;
FLTX_API int fltx_stream_partials(fltx_decoder* dec, int32_t look_back, int32_t on_device, fltx_stream_partials_out* out);
/* Device-resident results of the last batch (no host copy): pointers into HBM
 * valid until the next decode call.  n_hyp: int32[B]; scores: double[B*K*3];
 * tokens/words: int32 at tok_off[b] + i*(T[b]+2) + f. */
FLTX_API int fltx_result_device(fltx_decoder* dec, const int32_t** n_hyp,
                                const double** scores, const int32_t** tokens,
                                const int32_t** words, const int64_t** tok_off);

/* ---- one batch over several devices -------------------------------------- */
/* Utterances are independent: a group holds one context
 * and one decoder per entry of `devices` (an index may repeat: two contexts on
 * one device), the trie of `htrie` and the tables of `lm` replicated on each.
 * fltx_group_decode_batch cuts the batch into contiguous shards of about equal
 * frame count and runs fltx_decode_batch on every shard from its own host
 * thread; there is no inter-device traffic.  Replaces the loop over
 * Decoder::decode (decoder/Decoder.h:51-57) a multi-GPU caller would write.
 * emissions[i] is the buffer device i reads its shard from (the same host
 * pointer for all, or per-device HBM pointers with on_device[i] != 0); offsets
 * (NULL: utterances packed back to back) index into it with the caller's
 * utterance numbering.  Results are addressed by that numbering too. */
typedef struct fltx_group fltx_group;
FLTX_API int fltx_group_create(const int32_t* devices, int32_t n_devices, int32_t kind,
                               const fltx_options* opt, fltx_htrie* htrie, const fltx_lm* lm,
                               int32_t sil, int32_t blank, int32_t unk, const float* transitions,
                               int32_t n_transitions, int32_t is_lm_token, fltx_group** out);
FLTX_API int fltx_group_destroy(fltx_group* group);
FLTX_API int fltx_group_size(fltx_group* group, int32_t* n_devices);
/* decoder of part i and the utterances [first, first + count) it holds of the last batch */
FLTX_API int fltx_group_decoder(fltx_group* group, int32_t i, fltx_decoder** dec, int32_t* first,
                                int32_t* count);
FLTX_API int fltx_group_decode_batch(fltx_group* group, const float* const* emissions,
                                     const int32_t* on_device, const int64_t* offsets,
                                     const int32_t* T, int32_t B, int32_t N);
FLTX_API int fltx_group_result_count(fltx_group* group, int32_t b, int32_t* n_hyp, int32_t* length);
FLTX_API int fltx_group_result_fetch(fltx_group* group, int32_t b, int32_t max_hyp, double* scores,
                                     int32_t* tokens, int32_t* words, int32_t* n_copied);
FLTX_API int fltx_group_synchronize(fltx_group* group);

/* fltx_decoder_get(dec, "why_not_lane"): 0 when the last call started on a lane engine ("engine" 4 / 5 / 6), else the
 * eligibility terms it failed (the lane engines run the reference's LexiconFreeDecoder.cpp:30-125 /
 * LexiconDecoder.cpp:32-229 under these assumptions; everything else runs on the lean / generic engines) */
enum {
  FLTX_WHY_TOKENS = 1,        /* more than 64 tokens (lexicon-free decoder: a token BEAM of more than 64, or more than 16 384 tokens) */
  FLTX_WHY_BEAM = 2,          /* beam beyond the lane groups (lexicon-free: 512, lexicon: 256; 128 when spellings carry several words) */
  FLTX_WHY_STREAM = 4,        /* a stream the lane engines do not serve (lexicon streams, logAdd streams) */
  FLTX_WHY_LM = 8,            /* LM kind: a token-level LM on the lexicon decoder; a host LM (fltx_lm_host_create); an n-gram LM on the
                               * lexicon-free decoder whose contexts do not fit a dense table (more than 64 tokens, 2^24 contexts or 32 GB:
                               * round 6 -- otherwise the lane-state engine takes it at beams up to 512) */
  FLTX_WHY_LOGADD = 16,       /* lexicon-free decoder with logAdd over more than 64 tokens (round 5: the lexicon lane engines, 5 / 6,
                               * take logAdd wherever they take max-merge) */
  FLTX_WHY_ASG = 32,          /* lexicon decoder with the ASG criterion */
  FLTX_WHY_UNK = 64,          /* lexicon decoder with <unk> enabled (unk_score > -inf) */
  FLTX_WHY_TRIE_SHAPE = 128,  /* trie without a breadth-first layout (not a tree, a word that ends without the separator); several
                               * words per spelling (Trie.h:19) under ZeroLM -- those words tie in one LM state (round 5: with an
                               * n-gram LM such lexicons, the reference's own test lexicon among them, run on fltx_ylane.h) */
  FLTX_WHY_WORD_END = 256,    /* words do not all end in the separator (= sil), or sil == blank */
  FLTX_WHY_OPTIONS = 512,     /* negative beam threshold, sil / blank outside the token set */
  FLTX_WHY_LENGTH = 1024,     /* beam x frames beyond the state-id width of the history records */
  FLTX_WHY_SWITCHED_OFF = 2048, /* a tunable switched the engine off / a fallback is in force */
  FLTX_WHY_GEOMETRY = 4096    /* no compiled (threads, positions) geometry covers the token list */
};

/* ---- introspection for bench.py ------------------------------------------ */
/* Frames decoded and kernel launches issued by the last decode call, plus the
 * algorithmic HBM bytes of SURVEY.md section 8(d) for it. */
FLTX_API int fltx_decoder_stats(fltx_decoder* dec, int64_t* frames,
                                int64_t* algorithmic_bytes, int32_t* threads_per_utt,
                                int32_t* lds_bytes);
/* The same algorithmic bytes split by kernel: the decode kernel's share (emission rows in,
 * one back-pointer record per surviving slot out, trie gathers, plus 16 * order bytes per
 * n-gram LM query the kernel counted: *lm_bytes, included in *decode_bytes) and the
 * back-trace epilogue's (16 bytes per step of each hypothesis actually returned). */
FLTX_API int fltx_decoder_bytes(fltx_decoder* dec, int64_t* decode_bytes, int64_t* epilogue_bytes,
                                int64_t* lm_bytes);
/* Durations (ms) of the decode kernel and of the back-trace kernel of the last
 * fltx_decode_batch, from HIP events recorded on the context stream. */
FLTX_API int fltx_decoder_timing(fltx_decoder* dec, float* decode_ms, float* backtrace_ms);
/* Phase profile of the last launch (after fltx_decoder_set(dec,"profile",1)):
 * out[8] shader clocks summed over the batch. */
FLTX_API int fltx_decoder_profile(fltx_decoder* dec, uint64_t* out);
/* Tunables: "threads" (threads per utterance: 64..1024), "force_global_ws",
 * "dense" (0 = use the generic hash merge for lexicon-free frames too), "lean" /
 * "lane" / "slane" (0 = do not use that specialised lexicon-free + ZeroLM frame
 * step), "slane_threads", "xlane" / "ylane" (0 = do not use that lane engine of the
 * lexicon decoder; "ylane" = 2 prefers fltx_ylane.h where both apply), "keep_scores", "profile", "profile_wave"; lexicon decoder: "cut" (0 = build
 * every candidate's record), "slim" (0 = recompute form of the cut-off
 * generation), "items" (0 = no child-mask item list); test hooks: "cut_m",
 * "lds_budget" (pretend the CU has fewer bytes of LDS), "hot_level".
 * Round 3: "yshare" (-1 = the lexicon lane engines take the geometry of which several workgroups share a CU when the
 * batch exceeds the CUs; 1 / 0 = always / never), "stream_total_frames" (set before fltx_stream_begin: frames the
 * stream will decode in all -- its LM-state id tables grow with the stream, not with max_frames; default: at least
 * 2048), "sstream" (0 = a lexicon-free stream's chunks stay on the lane-per-slot step), "stream_optimistic" (0 = lexicon
 * streams use the worst-case HBM workspace from the start instead of decoding an overflowing chunk again),
 * "stream_defer" (0 = fltx_stream_step of a lexicon stream waits for its chunk; default: the chunk is launched and whether
 * a stream has to decode it again is looked at by the next call that needs the beam -- the next chunk's upload runs
 * under the kernel; a deferred fltx_stream_prune reports its errors there too), "lm_cache" (0 = the generic step asks
 * the n-gram tables for every word-end candidate instead of keeping the last (LM state, word) answers), "bt_lds_kb".  fltx_decoder_get also answers "engine", "redone", "stream_redone", "yshare", "sstream",
 * "bt_record_bytes" (the last back-trace: 2 or 4 = it narrowed the lane engines' packed history records to that many
 * bytes and kept the utterance's token tile in LDS; 0 = the chunked back-trace of plain 8-byte records),
 * "bt_chunk_frames" / "bt_stretch_frames" (frames per LDS chunk of history records / per stretch of the addends
 * staged by hypothesis while the emitting-model scores are re-added),
 * "bt_walk_waves" (waves that walked that back-trace's chunks: 1 = one walk per hypothesis; more = every wave walked
 * its own stretch of each chunk from every slot and the hypotheses were composed through the waves' maps -- narrowed
 * records at beams up to 64).  fltx_decoder_set: "bt_walk_waves" 0 / 1 keeps the walk per hypothesis (A/B runs, tests;
 * any other value: the default choice), "bt_threads" (threads of a back-trace workgroup, 64 .. 512 in whole waves,
 * 0 = the default: 512; the host-thread emulation of the tests: one wave; a workgroup never has fewer threads than the
 * beam rounded up to whole waves, whatever is asked: the score passes are one thread per hypothesis), "bt_profile"
 * (1 = thread 0 of each workgroup of the narrow back-trace stores shader clocks at its phase borders; afterwards
 * fltx_decoder_get "bt_prof_copy0" / "bt_prof_walk" / "bt_prof_wait" / "bt_prof_store" / "bt_prof_fetch0" /
 * "bt_prof_score" / "bt_prof_total" give the clocks summed over the "bt_prof_utts" utterances of the last batch;
 * "bt_prof_add" + "bt_prof_addwait" = "bt_prof_score": the first adding wave's own time in the score loop, and its
 * waits at the stretch barriers for the waves that stage the addends). */
/* Round 5: "defer_check" (1 = fltx_decode_batch returns as soon as its kernels are queued.  By default the call waits
 * for the decode kernel when the batch ran on a fast path that may flag an utterance, decodes the flagged ones again
 * and only then queues the back-trace -- every read of a device buffer is then queued before the call returns.  With
 * defer_check the look at the statuses, and that second pass, wait for the first call that reads results or "redone":
 * the caller keeps a device emissions buffer unchanged until then.  Batches of several decoder objects / streams
 * then run side by side on the CUs), "compact_always" (tests: streams rebuild their LM-state ids before every chunk). */
FLTX_API int fltx_decoder_set(fltx_decoder* dec, const char* key, int64_t value);
/* Geometry chosen for the last batch: "engine" (0 generic hash merge, 1 generic
 * dense merge, 2 lean register-resident step, 3 lane-per-slot step, 4 lane = LM
 * state step, 5 lane = (LM state, trie node) step of the lexicon decoder, 6 the
 * same with the LM terms: n-gram word LM, smeared trie, beams up to 128),
 * "lane" / "slane" / "xlane" (tokens per wave of engine 3 / 4 / 5, else 0),
 * "ylane" (lane groups of engine 6, else 0),
 * "redone" (utterances of the last offline call that the fast path handed to a
 * general one), "threads", "lds" (1 = workspace in LDS),
 * "hot_level" (HBM workspace: 1 = counters in LDS, 2 = candidate records too),
 * "cut" (candidates kept by the cut-off generation, 0 = off), "recompute",
 * "cap", "cap2", "items".
 * Round 5: "staged_emissions" (address of the library's own device copy of the last offline batch's host emissions, 0
 * when the caller passed a device buffer; valid until the decoder's next call -- a binding can decode the same batch
 * again from it with other settings, e.g. with "keep_scores" for Decoder::getBestHypothesis(lookBack) after decode()),
 * "compactions" / "id_cap" (streams: times the LM-state ids were rebuilt, ids per stream), "hlm_asked" / "hlm_distinct"
 * (host LM: questions listed / put to the callbacks), "fallback_reasons" (bit r: fltx_ylane.h's reason r, its header). */
FLTX_API int fltx_decoder_get(fltx_decoder* dec, const char* key, int64_t* value);

#ifdef __cplusplus
}
#endif
#endif /* FLTX_H_ */
