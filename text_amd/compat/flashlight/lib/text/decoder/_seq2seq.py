"""LexiconFreeSeq2SeqDecoder and LexiconSeq2SeqDecoder with the reference's Python surface
(bindings/python/flashlight/lib/text/_decoder.cpp:128-160, 443-535) over the batched device steps (fltx_s2s_*,
text_amd._capi.Seq2SeqBatchDecoder / LexiconSeq2SeqBatchDecoder) at B = 1.

decode_step(emissions, T, N) calls the user's update_func once per step with the live hypotheses of the beam
(rawY / rawBeamIdx / rawPrevStates, LexiconFreeSeq2SeqDecoder.cpp:44-60), uploads the rows it returns and runs one
device step; the per-row states are permuted on the host by the step's src_row.  The path is host-bound by
construction (one model call and one host wait per step): it exists for drop-in correctness.  Batches of utterances
with the model on the GPU use Seq2SeqBatchDecoder directly.
"""
import numpy as np

from text_amd import _capi
from text_amd.flashlight_lib_text_decoder import DecodeResult, ZeroLM


class EmittingModelState:
    """EmittingModelStatePtr (decoder/Utils.h:92): an opaque holder of the model's Python object."""
    __slots__ = ("obj",)

    def __init__(self, obj):
        self.obj = obj


def create_emitting_model_state(obj):
    return EmittingModelState(obj)


def get_obj_from_emitting_model_state(state):
    return state.obj


class LexiconFreeSeq2SeqDecoderOptions:
    """LexiconFreeSeq2SeqDecoderOptions (decoder/LexiconFreeSeq2SeqDecoder.h:23-30)."""
    __slots__ = ("beam_size", "beam_size_token", "beam_threshold", "lm_weight", "eos_score", "log_add")

    def __init__(self, beam_size, beam_size_token, beam_threshold, lm_weight, eos_score, log_add):
        self.beam_size, self.beam_size_token = int(beam_size), int(beam_size_token)
        self.beam_threshold, self.lm_weight = float(beam_threshold), float(lm_weight)
        self.eos_score, self.log_add = float(eos_score), bool(log_add)

    def __reduce__(self):
        return (LexiconFreeSeq2SeqDecoderOptions, (self.beam_size, self.beam_size_token, self.beam_threshold,
                                                   self.lm_weight, self.eos_score, self.log_add))


_ctx = None


def _context():
    """One context per process, on a torch stream of its own (the default stream's handle is NULL)."""
    global _ctx
    if _ctx is None:
        import torch
        torch.cuda.init()
        stream = torch.cuda.Stream()
        _ctx = (_capi.Context(stream=stream.cuda_stream), stream)  # (the stream lives as long as the context)
    return _ctx[0]


def _pad_rows(K, vectors):
    W = max(len(r) for r in vectors)
    rows = np.full((K, W), np.nan, dtype=np.float32)
    for k, r in enumerate(vectors):
        rows[k, :len(r)] = np.asarray(r, dtype=np.float32)
    return rows


def _decode(dec, K, update_func, max_output_length, emissions, T, N, raw_beam_idx, rows_lm=False):
    """decodeStep over a batched decoder at B = 1: one update_func call and one device step per step.  raw_beam_idx:
    update_func sees the parents' beam indices (LexiconFreeSeq2SeqDecoder.cpp:49), else -1 for every row (the
    lexicon decoder's candidates never record prevHypIdx: LexiconSeq2SeqDecoder.cpp:49).  rows_lm: update_func returns
    a third element, the LM's row vectors aligned with the scores (text_amd._capi.RowsLM)."""
    raw_y, raw_beam, prev_states = [-1], [-1], [None]
    dec.raw_words = [-1]  # (a WordRowsLM: the word each row of the coming update_func call ended, see below)
    t = 0
    begun = False
    while t < max_output_length:
        ret = update_func(emissions, N, T, raw_y, raw_beam, prev_states, t)
        if rows_lm:
            if len(ret) != 3:
                raise ValueError("update_func: with a RowsLM it returns (scores, states, lm_scores)")
            scores, out_states, lm_rows = ret
        else:
            scores, out_states = ret
        V = max(len(r) for r in scores)
        if not begun:
            dec.begin(1, V)
            begun = True
        rows = np.full((K, V), np.nan, dtype=np.float32)
        valid = np.zeros(K, dtype=np.uint8)
        for k, (r, s) in enumerate(zip(scores, out_states)):
            rows[k, :len(r)] = np.asarray(r, dtype=np.float32)
            valid[k] = s is not None
        out = dec.step(rows, valid, lm_scores=_pad_rows(K, lm_rows)) if rows_lm else dec.step(rows, valid)
        next_word = out[4] if len(out) == 5 else None  # (a decoder made with a text_amd._capi.WordRowsLM lists it)
        out = out[:4]
        dec.ctx.synchronize()  # (the rows decide the next model call: one host wait per step)
        tok, beam, src, n = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in out)
        t += 1
        n = int(n[0])
        if n == 0:
            break
        raw_y = tok[0, :n].tolist()
        if next_word is not None:
            dec.raw_words = (next_word.cpu().numpy() if hasattr(next_word, "cpu") else next_word)[0, :n].tolist()
        raw_beam = beam[0, :n].tolist() if raw_beam_idx else [-1] * n
        prev_states = [out_states[int(s)] for s in src[0, :n]]
    if not begun:  # maxOutputLength 0: the root alone
        dec.begin(1, 1)
    dec.end()
    hyps = []
    for h in dec.results(0):
        r = DecodeResult(len(h.tokens))
        r.score, r.emittingModelScore, r.lmScore = h.score, h.am, h.lm
        r.tokens, r.words = h.tokens.tolist(), h.words.tolist()
        hyps.append(r)
    return hyps


class LexiconFreeSeq2SeqDecoder:
    """LexiconFreeSeq2SeqDecoder(options, lm, eos_idx, update_func, max_output_length): ZeroLM, or an LM object of
    text_amd._capi (ZeroLM / NgramLM / ArpaLM / RowsLM); any other user-defined LM is refused
    (FLTX_ERR_UNSUPPORTED).

    With a text_amd._capi.RowsLM (a neural token LM in shallow fusion) update_func returns three elements,
    (scores, states, lm_scores): lm_scores is a list of row vectors aligned with scores, row k holding the LM's
    log-probabilities of every LM index after the hypothesis of row k (the LM's own state travels inside the model's
    state object).  The decoder keeps emittingModelScore and lmScore apart, as the reference does."""

    def __init__(self, options, lm, eos_idx, update_func, max_output_length):
        self.options, self.eos = options, int(eos_idx)
        self.update_func, self.max_output_length = update_func, int(max_output_length)
        ctx = _context()
        if isinstance(lm, ZeroLM):
            self._lm = _capi.ZeroLM(ctx)
        elif isinstance(lm, _capi.ZeroLM):  # (and its subclasses: n-gram tables)
            self._lm = lm
        else:
            raise _capi.FltxError(_capi.ERR_UNSUPPORTED, "seq2seq: ZeroLM or n-gram LM tables only (a user-defined LM "
                                  "may return repeated states and would need merges)")
        opts = _capi.make_s2s_options(options.beam_size, options.beam_size_token, options.beam_threshold,
                                      options.lm_weight, options.eos_score, options.log_add)
        self._dec = _capi.Seq2SeqBatchDecoder(ctx, opts, self._lm, self.eos, self.max_output_length)
        self._hyps = []

    def decode_step(self, emissions, T, N):
        self._hyps = _decode(self._dec, self.options.beam_size, self.update_func, self.max_output_length, emissions, T,
                             N, raw_beam_idx=True, rows_lm=isinstance(self._lm, _capi.RowsLM))

    def prune(self, look_back=0):
        return None

    def n_decoded_frames_in_buffer(self):
        return -1

    def get_best_hypothesis(self, look_back=0):
        return self._hyps[0] if self._hyps else DecodeResult(0)

    def get_all_final_hypothesis(self):
        return list(self._hyps)


class LexiconSeq2SeqDecoderOptions:
    """LexiconSeq2SeqDecoderOptions (decoder/LexiconSeq2SeqDecoder.h:23-31)."""
    __slots__ = ("beam_size", "beam_size_token", "beam_threshold", "lm_weight", "word_score", "eos_score", "log_add")

    def __init__(self, beam_size, beam_size_token, beam_threshold, lm_weight, word_score, eos_score, log_add):
        self.beam_size, self.beam_size_token = int(beam_size), int(beam_size_token)
        self.beam_threshold, self.lm_weight = float(beam_threshold), float(lm_weight)
        self.word_score, self.eos_score, self.log_add = float(word_score), float(eos_score), bool(log_add)

    def __reduce__(self):
        return (LexiconSeq2SeqDecoderOptions, (self.beam_size, self.beam_size_token, self.beam_threshold,
                                               self.lm_weight, self.word_score, self.eos_score, self.log_add))


class _Handle:
    """An fltx handle owned by another object (kept alive here)."""

    def __init__(self, h, owner):
        import ctypes
        self.h, self.owner = ctypes.c_void_p(h), owner


def _trie_handle(trie):
    if isinstance(trie, _capi.HostTrie):
        return trie
    if hasattr(trie, "_fltx_host_handle"):  # (the compat package's Trie)
        return _Handle(trie._fltx_host_handle(), trie)
    raise TypeError("LexiconSeq2SeqDecoder: the lexicon must be a Trie")


def _lm_handle(lm, ctx):
    if isinstance(lm, ZeroLM):
        return _capi.ZeroLM(ctx)
    if isinstance(lm, _capi.ZeroLM):  # (and its subclasses: n-gram tables)
        return lm
    h = lm._fltx_device_handle() if hasattr(lm, "_fltx_device_handle") else 0
    if not h:
        raise _capi.FltxError(_capi.ERR_UNSUPPORTED, "seq2seq: ZeroLM or n-gram LM tables only (a user-defined LM is "
                              "not supported)")
    return _Handle(h, lm)


class LexiconSeq2SeqDecoder:
    """LexiconSeq2SeqDecoder with the reference binding's signature (bindings/python/.../_decoder.cpp:497-512):
    (options, lm, trie, eos_idx, update_func, max_output_length, is_token_lm) -- the second parameter is named `lm`
    and takes the Trie, the third is named `trie` and takes the LM, as there.  The trie is the compat package's Trie
    (or a text_amd._capi.HostTrie), already smeared; the LM ZeroLM / KenLM (or a text_amd._capi LM object).
    update_func sees -1 for every beam index, as the reference's does.

    With a text_amd._capi.RowsLM and is_token_lm=True (a neural word-piece LM in shallow fusion) update_func returns
    three elements, (scores, states, lm_scores), as LexiconFreeSeq2SeqDecoder's does: row k of lm_scores holds the LM's
    log-probabilities of every LM index after the hypothesis of row k.  The LM must be a pure function of the token
    prefix (hypotheses that spell one token string differently merge; the best member's state object survives)."""

    @property
    def raw_words(self):
        """With a text_amd._capi.WordRowsLM and is_token_lm=False (a neural word LM in shallow fusion) update_func returns
        the three elements of the token case; row k of lm_scores holds the LM's log-probabilities of every LM index
        after the WORDS of the hypothesis of row k (one row per hypothesis: the decoder reads them with an identity
        lm_row_of).  The reference's update_func signature does not say where a word ended, so the decoder does: during
        a call, raw_words[k] is the word the hypothesis of row k ended at its last token, -1 for none -- the LM state of
        row k is that of prev_states[k], advanced by raw_words[k] when it is >= 0.  The LM must be a pure function of
        the word prefix.  None with any other LM."""
        return getattr(self._dec, "raw_words", None) if self._dec.has_word_rows_lm else None

    def __init__(self, options, lm, trie, eos_idx, update_func, max_output_length, is_token_lm):
        self.options, self.eos = options, int(eos_idx)
        self.update_func, self.max_output_length = update_func, int(max_output_length)
        ctx = _context()
        self._trie = _trie_handle(lm)
        self._lm = _lm_handle(trie, ctx)
        opts = _capi.make_s2s_lex_options(options.beam_size, options.beam_size_token, options.beam_threshold,
                                          options.lm_weight, options.word_score, options.eos_score, options.log_add)
        self._dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, opts, self._trie, self._lm, self.eos,
                                                     self.max_output_length, bool(is_token_lm))
        self._hyps = []

    def decode_step(self, emissions, T, N):
        self._hyps = _decode(self._dec, self.options.beam_size, self.update_func, self.max_output_length, emissions, T,
                             N, raw_beam_idx=False, rows_lm=isinstance(self._lm, _capi.RowsLM))

    def prune(self, look_back=0):
        return None

    def n_decoded_frames_in_buffer(self):
        return -1

    def get_best_hypothesis(self, look_back=0):
        return self._hyps[0] if self._hyps else DecodeResult(0)

    def get_all_final_hypothesis(self):
        return list(self._hyps)
