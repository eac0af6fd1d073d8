"""ctypes binding of the C ABI in include/fltx.h (text_amd/lib/libfltx.so).

This is the only way Python reaches the decoder: every decode call runs the
HIP kernels.  If the shared library is missing or no gfx950 device is usable
the calls raise -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libfltx.so")

FLTX_OK, ERR_INVALID, ERR_HIP, ERR_OOM, ERR_UNSUPPORTED, ERR_RANGE, ERR_STATE = range(7)
CRITERION = {"asg": 0, "ctc": 1, "s2s": 2}
LEXFREE, LEXICON, S2S_LEXFREE, S2S_LEXICON, CTC_ROWS, LEX_CTC_ROWS = 0, 1, 2, 3, 4, 5
# fltx_decoder_get "why_not_lane" (include/fltx.h FLTX_WHY_*)
(FLTX_WHY_TOKENS, FLTX_WHY_BEAM, FLTX_WHY_STREAM, FLTX_WHY_LM, FLTX_WHY_LOGADD, FLTX_WHY_ASG, FLTX_WHY_UNK,
 FLTX_WHY_TRIE_SHAPE, FLTX_WHY_WORD_END, FLTX_WHY_OPTIONS, FLTX_WHY_LENGTH, FLTX_WHY_SWITCHED_OFF,
 FLTX_WHY_GEOMETRY) = (1 << i for i in range(13))


class Options(C.Structure):
    """fltx_options == LexiconDecoderOptions (decoder/LexiconDecoder.h:21-31)."""

    _fields_ = [
        ("beam_size", C.c_int32),
        ("beam_size_token", C.c_int32),
        ("beam_threshold", C.c_double),
        ("lm_weight", C.c_double),
        ("word_score", C.c_double),
        ("unk_score", C.c_double),
        ("sil_score", C.c_double),
        ("log_add", C.c_int32),
        ("criterion", C.c_int32),
    ]


class S2sOptions(C.Structure):
    """fltx_s2s_options == LexiconFreeSeq2SeqDecoderOptions (decoder/LexiconFreeSeq2SeqDecoder.h:23-30)."""

    _fields_ = [
        ("beam_size", C.c_int32),
        ("beam_size_token", C.c_int32),
        ("beam_threshold", C.c_double),
        ("lm_weight", C.c_double),
        ("eos_score", C.c_double),
        ("log_add", C.c_int32),
    ]


class S2sLexOptions(C.Structure):
    """fltx_s2s_lex_options == LexiconSeq2SeqDecoderOptions (decoder/LexiconSeq2SeqDecoder.h:23-31)."""

    _fields_ = [
        ("beam_size", C.c_int32),
        ("beam_size_token", C.c_int32),
        ("beam_threshold", C.c_double),
        ("lm_weight", C.c_double),
        ("word_score", C.c_double),
        ("eos_score", C.c_double),
        ("log_add", C.c_int32),
    ]


class Transcripts(C.Structure):
    """fltx_transcripts (include/fltx.h)"""
    _fields_ = [
        ("n_rows", C.c_int64),
        ("row_first", C.c_void_p),
        ("scores", C.c_void_p),
        ("tok_off", C.c_void_p),
        ("tokens", C.c_void_p),
        ("timesteps", C.c_void_p),
        ("word_off", C.c_void_p),
        ("words", C.c_void_p),
        ("word_timesteps", C.c_void_p),
        ("word_tok_end", C.c_void_p),
        ("n_tokens", C.c_int64),
        ("n_words", C.c_int64),
    ]


class StreamPartialsOut(C.Structure):
    """fltx_stream_partials_out (include/fltx.h)"""
    _fields_ = [
        ("t", Transcripts),
        ("length", C.c_void_p),
        ("stable_frames", C.c_void_p),
        ("stable_tokens", C.c_void_p),
        ("stable_words", C.c_void_p),
        ("first_frame", C.c_void_p),
        ("status", C.c_void_p),
    ]


class FinishedOut(C.Structure):
    """fltx_finished_out (include/fltx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("n_hyp", "length", "status", "scores", "tokens", "words", "row_off")]


class S2sFinishedOut(C.Structure):
    """fltx_s2s_finished_out (include/fltx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("n_hyp", "steps", "status", "scores", "tokens", "words")] + \
        [("length", C.c_int32)]


def _view(ptr, ctype, n):
    """n elements at a host address as a NumPy array (no copy)"""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=np.dtype(ctype))
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))


def _transcript_views(t, device):
    """The arrays of a filled fltx_transcripts.  Host: NumPy views of the library's pinned buffers (valid until the next
    call on the same owner).  device: the integer addresses, and the sizes n_tokens / n_words."""
    n = int(t.n_rows)
    if device:
        return {"n_rows": n, "n_tokens": int(t.n_tokens), "n_words": int(t.n_words), "tok_off": t.tok_off, "tokens": t.tokens, "timesteps": t.timesteps,
                "word_off": t.word_off, "words": t.words, "word_timesteps": t.word_timesteps,
                "word_tok_end": t.word_tok_end}
    tok_off = _view(t.tok_off, C.c_int64, n + 1)
    word_off = _view(t.word_off, C.c_int64, n + 1)
    nt, nw = int(t.n_tokens), int(t.n_words)
    return {"n_rows": n, "n_tokens": nt, "n_words": nw, "tok_off": tok_off, "tokens": _view(t.tokens, C.c_int32, nt),
            "timesteps": _view(t.timesteps, C.c_int32, nt), "word_off": word_off,
            "words": _view(t.words, C.c_int32, nw), "word_timesteps": _view(t.word_timesteps, C.c_int32, nw),
            "word_tok_end": _view(t.word_tok_end, C.c_int32, nw)}


def _finished_host(fo, w, B, K):
    """A filled fltx_finished_out with host results, for the streams the flags w name: n_hyp, length, status ([B] int32
    copies) and hyps = {b: [Hyp]} copied out of the library's pinned buffers."""
    n_hyp, length, status = (_view(p, C.c_int32, B).copy() for p in (fo.n_hyp, fo.length, fo.status))
    row_off = _view(fo.row_off, C.c_int64, B)
    scores = _view(fo.scores, C.c_double, 3 * B * K)
    hyps = {}
    for b in np.flatnonzero(w):
        n, ln, at = int(n_hyp[b]), int(length[b]), int(row_off[b])
        hyps[int(b)] = []
        for i in range(n if status[b] == 0 else 0):
            tk = _view(fo.tokens + 4 * (at + i * ln), C.c_int32, ln).copy()
            wd = _view(fo.words + 4 * (at + i * ln), C.c_int32, ln).copy() if fo.words else np.full(ln, -1, np.int32)
            s = scores[3 * (b * K + i):3 * (b * K + i) + 3]
            hyps[int(b)].append(Hyp(float(s[0]), float(s[1]), float(s[2]), tk, wd))
    return {"n_hyp": n_hyp, "length": length, "status": status, "hyps": hyps}


class FltxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fltx error %d: %s" % (code, msg))
        self.code = code


_EXC = {ERR_INVALID: ValueError, ERR_RANGE: IndexError}


class Lib:
    """A loaded libfltx with typed entry points."""

    SYMBOLS = [
        "fltx_last_error", "fltx_version", "fltx_ctx_create", "fltx_ctx_destroy",
        "fltx_ctx_synchronize", "fltx_ctx_stream", "fltx_ctx_uid", "fltx_lm_zero_create",
        "fltx_lm_ngram_create", "fltx_lm_host_create", "fltx_lm_arpa_load", "fltx_lm_state_size", "fltx_lm_start", "fltx_lm_step", "fltx_lm_destroy", "fltx_lm_score_sequence",
        "fltx_trie_create", "fltx_trie_destroy", "fltx_decoder_create",
        "fltx_decoder_destroy", "fltx_decode_batch", "fltx_stream_begin",
        "fltx_stream_step", "fltx_stream_end", "fltx_stream_prune",
        "fltx_stream_frames_in_buffer", "fltx_result_count", "fltx_result_fetch", "fltx_result_fetch_batch", "fltx_result_fetch_batch_compact",
        "fltx_result_best", "fltx_result_device", "fltx_decoder_stats",
        "fltx_decoder_set", "fltx_decoder_get", "fltx_decoder_timing", "fltx_decoder_profile", "fltx_htrie_create", "fltx_htrie_destroy", "fltx_htrie_insert",
        "fltx_htrie_search", "fltx_htrie_smear", "fltx_htrie_num_nodes", "fltx_htrie_upload",
        "fltx_decoder_bytes", "fltx_htrie_node", "fltx_group_create", "fltx_group_destroy", "fltx_group_size", "fltx_group_decoder",
        "fltx_group_decode_batch", "fltx_group_result_count", "fltx_group_result_fetch", "fltx_group_synchronize",
        "fltx_s2s_decoder_create", "fltx_s2s_begin", "fltx_s2s_step", "fltx_s2s_step_typed", "fltx_s2s_done",
        "fltx_s2s_end", "fltx_s2s_finish", "fltx_s2s_done_each", "fltx_s2s_lex_decoder_create", "fltx_s2s_lex_set_max_states", "fltx_s2s_lex_info",
        "fltx_lm_rows_create", "fltx_s2s_step_lm_rows",
        "fltx_lm_word_rows_create", "fltx_s2s_step_word_lm_rows",
        "fltx_ctc_rows_decoder_create", "fltx_ctc_rows_lex_decoder_create", "fltx_ctc_rows_begin", "fltx_ctc_rows_step", "fltx_ctc_rows_end",
        "fltx_ctc_rows_begin_typed", "fltx_ctc_rows_stream_append_typed",
        "fltx_ctc_rows_stream_begin", "fltx_ctc_rows_stream_append", "fltx_ctc_rows_stream_prune",
        "fltx_ctc_rows_stream_frames_in_buffer", "fltx_ctc_rows_stream_collect", "fltx_ctc_rows_stream_finish",
        "fltx_ctc_rows_plan_begin", "fltx_ctc_rows_plan", "fltx_ctc_rows_plan_release",
        "fltx_collapse_rows", "fltx_result_transcripts", "fltx_stream_partials", "fltx_stream_finish",
    ]

    def __init__(self, path=None):
        path = path or DEFAULT_LIB
        if not os.path.exists(path):
            raise FileNotFoundError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % path)
        self.path = path
        L = self.lib = C.CDLL(path)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        pvp = C.POINTER(C.c_void_p)
        L.fltx_last_error.restype = C.c_char_p
        L.fltx_version.restype = C.c_char_p
        L.fltx_ctx_stream.restype = vp
        L.fltx_ctx_stream.argtypes = [vp]
        L.fltx_ctx_uid.restype = C.c_uint64
        L.fltx_ctx_uid.argtypes = [vp]
        sig = {
            "fltx_ctx_create": [C.c_int, vp, pvp],
            "fltx_ctx_destroy": [vp],
            "fltx_ctx_synchronize": [vp],
            "fltx_lm_zero_create": [vp, pvp],
            "fltx_lm_ngram_create": [vp, i32, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, pvp],
            "fltx_lm_arpa_load": [C.c_char_p, C.c_char_p, pvp],
            "fltx_lm_host_create": [vp, pvp],
            "fltx_lm_state_size": [vp, vp],
            "fltx_lm_start": [vp, i32, vp],
            "fltx_lm_step": [vp, vp, i32, vp, vp],
            "fltx_lm_destroy": [vp],
            "fltx_lm_score_sequence": [vp, vp, i32, i32, vp, vp],
            "fltx_trie_create": [vp, i64, i32, vp, vp, vp, vp, pvp],
            "fltx_trie_destroy": [vp],
            "fltx_decoder_create": [vp, i32, C.POINTER(Options), vp, vp, i32, i32, i32, vp, i32, i32, pvp],
            "fltx_decoder_destroy": [vp],
            "fltx_decode_batch": [vp, vp, i32, vp, vp, i32, i32],
            "fltx_stream_begin": [vp, i32, i32, i32],
            "fltx_stream_step": [vp, vp, i32, vp, vp],
            "fltx_stream_end": [vp],
            "fltx_stream_prune": [vp, i32],
            "fltx_stream_frames_in_buffer": [vp, i32, vp],
            "fltx_result_count": [vp, i32, vp, vp],
            "fltx_result_fetch": [vp, i32, i32, vp, vp, vp, vp],
            "fltx_result_fetch_batch": [vp, pvp, pvp, pvp, pvp, pvp, pvp],
            "fltx_result_fetch_batch_compact": [vp, pvp, pvp, pvp, pvp, pvp, pvp],
            "fltx_result_best": [vp, i32, i32, vp, vp, vp, i32, vp],
            "fltx_result_device": [vp, pvp, pvp, pvp, pvp, pvp],
            "fltx_decoder_stats": [vp, vp, vp, vp, vp],
            "fltx_decoder_set": [vp, C.c_char_p, i64],
            "fltx_decoder_get": [vp, C.c_char_p, vp],
            "fltx_decoder_timing": [vp, vp, vp],
            "fltx_decoder_profile": [vp, vp],
            "fltx_htrie_create": [i32, i32, pvp],
            "fltx_htrie_destroy": [vp],
            "fltx_htrie_insert": [vp, vp, i32, i32, C.c_float],
            "fltx_htrie_search": [vp, vp, i32, vp, vp, vp, vp, vp],
            "fltx_htrie_smear": [vp, i32],
            "fltx_htrie_num_nodes": [vp, vp],
            "fltx_htrie_upload": [vp, vp, pvp],
            "fltx_decoder_bytes": [vp, vp, vp, vp],
            "fltx_htrie_node": [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32],
            "fltx_group_create": [vp, i32, i32, C.POINTER(Options), vp, vp, i32, i32, i32, vp, i32, i32, pvp],
            "fltx_group_destroy": [vp],
            "fltx_group_size": [vp, vp],
            "fltx_group_decoder": [vp, i32, pvp, vp, vp],
            "fltx_group_decode_batch": [vp, vp, vp, vp, vp, i32, i32],
            "fltx_group_result_count": [vp, i32, vp, vp],
            "fltx_group_result_fetch": [vp, i32, i32, vp, vp, vp, vp],
            "fltx_group_synchronize": [vp],
            "fltx_s2s_decoder_create": [vp, C.POINTER(S2sOptions), vp, i32, i32, pvp],
            "fltx_s2s_begin": [vp, i32, i32, vp, vp, vp, vp],
            "fltx_s2s_step": [vp, vp, i32, i64, vp, vp, vp, vp, vp],
            "fltx_s2s_step_typed": [vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp],
            "fltx_lm_rows_create": [i32, vp, i32, i32, pvp],
            "fltx_s2s_step_lm_rows": [vp, vp, i32, i32, i64, vp, i32, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp],
            "fltx_lm_word_rows_create": [i32, vp, i32, i32, pvp],
            "fltx_s2s_step_word_lm_rows": [vp, vp, i32, i32, i64, vp, i32, i32, i64, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                           vp, vp],
            "fltx_s2s_done": [vp, vp],
            "fltx_s2s_end": [vp],
            "fltx_s2s_finish": [vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(S2sFinishedOut)],
            "fltx_s2s_done_each": [vp, vp],
            "fltx_s2s_lex_decoder_create": [vp, C.POINTER(S2sLexOptions), vp, vp, i32, i32, i32, pvp],
            "fltx_s2s_lex_set_max_states": [vp, i32],
            "fltx_s2s_lex_info": [vp, vp, vp, vp, vp],
            "fltx_ctc_rows_decoder_create": [vp, C.POINTER(Options), vp, i32, i32, pvp],
            "fltx_ctc_rows_lex_decoder_create": [vp, C.POINTER(Options), vp, vp, i32, i32, i32, i32, pvp],
            "fltx_ctc_rows_begin": [vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp],
            "fltx_ctc_rows_begin_typed": [vp, vp, i32, i32, i32, vp, i64, vp, i32, i32, vp, vp, vp, vp, vp],
            "fltx_ctc_rows_stream_append_typed": [vp, vp, i32, i32, i32, vp, i64, vp, vp],
            "fltx_ctc_rows_step": [vp, vp, i32, i32, i64, vp, i32, i32, vp, vp, vp, vp, vp],
            "fltx_ctc_rows_end": [vp, vp, i32, i32, i64, vp, i32, i32, vp],
            "fltx_ctc_rows_stream_begin": [vp, i32, i32, i32, vp, vp, vp, vp],
            "fltx_ctc_rows_stream_append": [vp, vp, i32, vp, vp],
            "fltx_ctc_rows_stream_prune": [vp, i32],
            "fltx_ctc_rows_stream_frames_in_buffer": [vp, i32, vp],
            "fltx_ctc_rows_stream_collect": [vp, i32, vp, vp, vp],
            "fltx_ctc_rows_stream_finish": [vp, vp, vp, i32, i32, i64, vp, i32, i32, vp, vp, vp, vp, vp, i32,
                                            C.POINTER(FinishedOut)],
            "fltx_ctc_rows_plan_begin": [vp, i32],
            "fltx_ctc_rows_plan": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
            "fltx_ctc_rows_plan_release": [vp, vp, vp, i32],
            "fltx_collapse_rows": [vp, vp, vp, vp, vp, i64, i32, i32, C.POINTER(Transcripts)],
            "fltx_result_transcripts": [vp, i32, i32, C.POINTER(Transcripts)],
            "fltx_stream_partials": [vp, i32, i32, C.POINTER(StreamPartialsOut)],
            "fltx_stream_finish": [vp, vp, i32, C.POINTER(FinishedOut)],
        }
        for name, args in sig.items():
            fn = getattr(L, name)
            fn.restype = C.c_int
            fn.argtypes = args

    def check(self, rc):
        if rc != FLTX_OK:
            msg = self.lib.fltx_last_error().decode()
            raise _EXC.get(rc, FltxError)(msg) if rc in _EXC else FltxError(rc, msg)

    def version(self):
        return self.lib.fltx_version().decode()


_default = None

# Live handles are destroyed explicitly at interpreter exit, decoders first and
# contexts last, while the HIP runtime is still loaded (garbage-collection order
# at shutdown is arbitrary and the runtime aborts if it is torn down first).
import atexit
import weakref

_live = {"dec": weakref.WeakSet(), "trie": weakref.WeakSet(), "lm": weakref.WeakSet(), "ctx": weakref.WeakSet()}


def _close_all():
    for kind in ("dec", "trie", "lm", "ctx"):
        for obj in list(_live[kind]):
            try:
                obj.close()
            except Exception:
                pass


atexit.register(_close_all)


def default_lib():
    global _default
    if _default is None:
        _default = Lib()
    return _default


def _ptr(a):
    return None if a is None else a.ctypes.data


class Context:
    def __init__(self, device=-1, stream=None, lib=None):
        self.L = lib or default_lib()
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_ctx_create(device, stream, C.byref(h)))
        self.h = h
        _live["ctx"].add(self)

    def synchronize(self):
        self.L.check(self.L.lib.fltx_ctx_synchronize(self.h))

    @property
    def stream(self):
        return self.L.lib.fltx_ctx_stream(self.h)

    def collapse_rows(self, tokens, words, row_off, row_len, blank, device=False, n_rows=None):
        """fltx_collapse_rows: the collapsed transcripts of frame rows in HBM.  tokens (int32) / words (int32; None: no
        word row) / row_off (int64) / row_len (int32) are each a device address (int) or a NumPy array, which is uploaded
        first (a convenience for tests and small uses; it needs torch unless the library is the emulator, whose device
        memory is host memory).  n_rows: the row count -- needed when row_len is an address, else len(row_len).
        -> a dict of NumPy views of the context's pinned buffers (n_rows, n_tokens, n_words, tok_off, tokens, timesteps,
        word_off, words, word_timesteps, word_tok_end), valid until the next call; with device=True the array keys hold
        device addresses, n_tokens / n_words the sizes."""
        if n_rows is None:
            if not isinstance(row_len, np.ndarray):
                raise TypeError("collapse_rows: n_rows is needed when row_len is a device address")
            n_rows = len(row_len)
        keep = []

        def addr(a, dtype):
            if a is None or isinstance(a, int):
                return a
            a = np.ascontiguousarray(a, dtype=dtype)
            if "emulation" not in self.L.version() and a.size:
                import torch
                a = torch.from_numpy(a).to(torch.device("cuda", torch.cuda.current_device()))
            keep.append(a)
            return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        ptrs = (addr(tokens, np.int32), addr(words, np.int32), addr(row_off, np.int64), addr(row_len, np.int32))
        uploaded = any(not isinstance(k, np.ndarray) for k in keep)
        if uploaded:  # (the uploads are done before the context's stream reads them)
            import torch
            torch.cuda.current_stream().synchronize()
        t = Transcripts()
        self.L.check(self.L.lib.fltx_collapse_rows(self.h, *ptrs, int(n_rows), int(blank), 1 if device else 0,
                                                   C.byref(t)))
        if device and uploaded:  # (the write kernel may still be reading the uploads, which go when this returns)
            self.synchronize()
        return _transcript_views(t, device)

    def close(self):
        if self.h:
            self.L.lib.fltx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ZeroLM:
    def __init__(self, ctx=None, lib=None):
        self.ctx, self.L = ctx, (ctx.L if ctx is not None else (lib or default_lib()))
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_lm_zero_create(ctx.h if ctx is not None else None, C.byref(h)))
        self.h = h
        _live["lm"].add(self)

    def score_sequence(self, words, with_finish=True):
        return self._score(words, with_finish)

    # explicit-state LM::start / score / finish on the host copy of the tables (decoder/lm/LM.h:61-78)
    def state_size(self):
        n = C.c_int32(0)
        self.L.check(self.L.lib.fltx_lm_state_size(self.h, C.addressof(n)))
        return n.value

    def start(self, start_with_nothing=False):
        ctx = np.zeros(max(1, self.state_size()), dtype=np.int32)
        self.L.check(self.L.lib.fltx_lm_start(self.h, int(start_with_nothing), _ptr(ctx)))
        return ctx

    def step(self, ctx, usr_idx):
        """-> (context of the next state, score); usr_idx == -1: LM::finish"""
        out = np.zeros_like(ctx)
        sc = C.c_float(0)
        self.L.check(self.L.lib.fltx_lm_step(self.h, _ptr(ctx), int(usr_idx), _ptr(out), C.addressof(sc)))
        return out, sc.value

    def _score(self, words, with_finish):
        w = np.ascontiguousarray(words, dtype=np.int32)
        per = np.zeros(len(w), dtype=np.float32)
        tot = C.c_float(0)
        self.L.check(self.L.lib.fltx_lm_score_sequence(self.h, _ptr(w), len(w), int(with_finish),
                                                       _ptr(per), C.addressof(tot)))
        return per, tot.value

    def close(self):
        if self.h:
            self.L.lib.fltx_lm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NgramLM(ZeroLM):
    """Flat back-off n-gram tables in HBM (replaces lm/KenLM.cpp:32-83)."""

    def __init__(self, ctx, order, ngram_order, ngram_words, prob, backoff, usr_to_lm, bos, eos, unk, lib=None):
        self.ctx, self.L = ctx, (ctx.L if ctx is not None else (lib or default_lib()))
        no = np.ascontiguousarray(ngram_order, dtype=np.int32)
        nw = np.ascontiguousarray(ngram_words, dtype=np.int32).reshape(len(no), order)
        pr = np.ascontiguousarray(prob, dtype=np.float32)
        bo = np.ascontiguousarray(backoff, dtype=np.float32)
        um = np.ascontiguousarray(usr_to_lm, dtype=np.int32)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_lm_ngram_create(ctx.h if ctx is not None else None, order, len(no), _ptr(no), _ptr(nw), _ptr(pr),
                                                     _ptr(bo), _ptr(um), len(um), bos, eos, unk,
                                                     C.byref(h)))
        self.h = h
        _live["lm"].add(self)


class RowsLM(ZeroLM):
    """fltx_lm_rows_create: an LM whose answers arrive per step as rows next to the model's rows (a neural token LM in
    shallow fusion; Seq2SeqBatchDecoder.step(..., lm_scores=), and LexiconSeq2SeqBatchDecoder's with is_lm_token=True).
    lm_width: entries per LM row (0: the decoder's V); usr_to_lm: the LM index of each model token (None: identity);
    finish_index: the LM index LM::finish reads (-1: usr_to_lm[eos])."""

    def __init__(self, lm_width=0, usr_to_lm=None, finish_index=-1, lib=None):
        self.ctx, self.L = None, lib or default_lib()
        um = None if usr_to_lm is None else np.ascontiguousarray(usr_to_lm, dtype=np.int32)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_lm_rows_create(int(lm_width), None if um is None else _ptr(um),
                                                    0 if um is None else len(um), int(finish_index), C.byref(h)))
        self.h = h
        self.lm_width, self.usr_to_lm, self.finish_index = int(lm_width), um, int(finish_index)
        _live["lm"].add(self)


class WordRowsLM(RowsLM):
    """fltx_lm_word_rows_create: a neural LM over the lexicon's WORDS whose answers arrive per step as rows
    (LexiconSeq2SeqBatchDecoder with is_lm_token=False; step(..., lm_scores=, lm_row_of=)).  lm_width: entries per LM
    row (required, at most 2**22); word_to_lm: the LM index of each lexicon word id (None: identity); finish_index: the
    LM index LM::finish reads (required: eos is a token and has no word id).  No other decoder takes it."""

    def __init__(self, lm_width, word_to_lm=None, finish_index=0, lib=None):
        self.ctx, self.L = None, lib or default_lib()
        wm = None if word_to_lm is None else np.ascontiguousarray(word_to_lm, dtype=np.int32)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_lm_word_rows_create(int(lm_width), None if wm is None else _ptr(wm),
                                                         0 if wm is None else len(wm), int(finish_index), C.byref(h)))
        self.h = h
        self.lm_width, self.word_to_lm, self.finish_index = int(lm_width), wm, int(finish_index)
        self.usr_to_lm = wm
        _live["lm"].add(self)


class ArpaLM(ZeroLM):
    """KenLM(path, usr_token_dict) for ARPA text models (lm/KenLM.cpp:32-50)."""

    def __init__(self, path, usr_words, lib=None):
        self.ctx, self.L = None, lib or default_lib()
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_lm_arpa_load(path.encode(), "\n".join(usr_words).encode(), C.byref(h)))
        self.h = h
        _live["lm"].add(self)


_HLM_START = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32)
_HLM_SCORE = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float))
_HLM_STATES = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32))


class _HostLmStruct(C.Structure):
    _fields_ = [("user", C.c_void_p), ("start", _HLM_START), ("score", _HLM_SCORE),
                ("update_cache", _HLM_STATES), ("retain", _HLM_STATES)]


class HostLM(ZeroLM):
    """A user-defined LM behind fltx_lm_host_create (include/fltx.h): `lm` is any object with the reference's LM
    methods (decoder/lm/LM.h:61-85) -- start(start_with_nothing) -> state, score(state, idx) -> (state, score),
    finish(state) -> (state, score), optionally update_cache(states).  States are arbitrary Python objects; as in
    the reference two hypotheses share an LM state iff the LM returned the SAME object (`is`).  The beam search runs
    in the HIP kernels; once per frame the distinct (state, idx) questions of the whole batch are answered here."""

    def __init__(self, lm, lib=None):
        self.ctx, self.L = None, lib or default_lib()
        self.lm = lm
        self.states = []     # per utterance: id -> state object
        self.ids = []        # per utterance: id(state object) -> id
        self.error = None    # the exception a callback raised (re-raised by the decoder call)
        self.calls = 0       # LM.score / LM.finish calls made
        self.released = 0    # states dropped after prune

        def guard(fn):
            def run(*a):
                try:
                    return fn(*a)
                except BaseException as e:  # noqa: BLE001 -- must not unwind through the C frames
                    self.error = e
                    return 1
            return run

        def start(_user, n_utt):
            self.states, self.ids = [], []
            for _ in range(n_utt):
                s0 = self.lm.start(False)
                self.states.append({0: s0})
                self.ids.append({id(s0): 0})
            self.next = [1] * n_utt
            return 0

        def score(_user, n, utt, state, idx, out_state, out_score):
            for i in range(n):
                b = utt[i]
                st = self.states[b][state[i]]
                self.calls += 1
                ns, sc = self.lm.finish(st) if idx[i] < 0 else self.lm.score(st, idx[i])
                k = self.ids[b].get(id(ns))
                if k is None or self.states[b][k] is not ns:
                    k = self.next[b]
                    self.next[b] += 1
                    self.ids[b][id(ns)] = k
                    self.states[b][k] = ns
                out_state[i] = k
                out_score[i] = sc
            return 0

        def update_cache(_user, b, n, states):
            f = getattr(self.lm, "update_cache", None)
            if f is not None:
                f([self.states[b][states[i]] for i in range(n)])
            return 0

        def retain(_user, b, n, states):
            keep = {states[i] for i in range(n)}
            for k in [k for k in self.states[b] if k not in keep]:
                self.ids[b].pop(id(self.states[b][k]), None)
                del self.states[b][k]
                self.released += 1
            return 0

        self._cb = _HostLmStruct(None, _HLM_START(guard(start)), _HLM_SCORE(guard(score)),
                                 _HLM_STATES(guard(update_cache)), _HLM_STATES(guard(retain)))
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_lm_host_create(C.byref(self._cb), C.byref(h)))
        self.h = h
        _live["lm"].add(self)

    def score_sequence(self, words, with_finish=True):
        st = self.lm.start(False)
        per = np.zeros(len(words), dtype=np.float32)
        for i, w in enumerate(words):
            st, per[i] = self.lm.score(st, int(w))
        tot = float(per.sum())
        if with_finish:
            tot += self.lm.finish(st)[1]
        return per, tot


class Trie:
    """Flattened, already smeared lexicon trie in HBM (decoder/Trie.h:64-92)."""

    def __init__(self, ctx, child, max_score, label_off, labels):
        self.ctx, self.L = ctx, ctx.L
        ch = np.ascontiguousarray(child, dtype=np.int32)
        n_nodes, n_tokens = ch.shape
        ms = np.ascontiguousarray(max_score, dtype=np.float32)
        lo = np.ascontiguousarray(label_off, dtype=np.int32)
        lb = np.ascontiguousarray(labels, dtype=np.int32)
        assert len(ms) == n_nodes and len(lo) == n_nodes + 1
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_trie_create(ctx.h, n_nodes, n_tokens, _ptr(ch), _ptr(ms), _ptr(lo),
                                                 _ptr(lb) if len(lb) else None, C.byref(h)))
        self.h = h
        self.n_nodes, self.n_tokens = n_nodes, n_tokens
        _live["trie"].add(self)

    def close(self):
        if self.h:
            self.L.lib.fltx_trie_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostTrie:
    """Host-side Trie(maxChildren, rootIdx) with insert/search/smear
    (decoder/Trie.h:64-92); `upload` flattens it into HBM."""

    def __init__(self, max_children, root_idx, lib=None):
        self.L = lib or default_lib()
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_htrie_create(max_children, root_idx, C.byref(h)))
        self.h = h

    def insert(self, indices, label, score):
        a = np.ascontiguousarray(indices, dtype=np.int32)
        self.L.check(self.L.lib.fltx_htrie_insert(self.h, _ptr(a), len(a), int(label), float(score)))

    def insert_many(self, spell_flat, spell_off, labels, scores):
        sf = np.ascontiguousarray(spell_flat, dtype=np.int32)
        f = self.L.lib.fltx_htrie_insert
        base = sf.ctypes.data
        for w in range(len(spell_off) - 1):
            a, b = int(spell_off[w]), int(spell_off[w + 1])
            self.L.check(f(self.h, base + 4 * a, b - a, int(labels[w]), float(scores[w])))

    def search(self, indices):
        a = np.ascontiguousarray(indices, dtype=np.int32)
        found, nl = C.c_int32(0), C.c_int32(0)
        ms = C.c_float(0)
        labels = np.zeros(6, dtype=np.int32)
        scores = np.zeros(6, dtype=np.float32)
        self.L.check(self.L.lib.fltx_htrie_search(self.h, _ptr(a), len(a), C.addressof(found),
                                                  C.addressof(ms), C.addressof(nl), _ptr(labels),
                                                  _ptr(scores)))
        if not found.value:
            return None
        return {"max_score": ms.value, "labels": labels[:nl.value].tolist(),
                "scores": scores[:nl.value].tolist()}

    def smear(self, mode=1):
        self.L.check(self.L.lib.fltx_htrie_smear(self.h, int(mode)))

    def num_nodes(self):
        n = C.c_int64(0)
        self.L.check(self.L.lib.fltx_htrie_num_nodes(self.h, C.addressof(n)))
        return n.value

    def upload(self, ctx):
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_htrie_upload(self.h, ctx.h, C.byref(h)))
        t = Trie.__new__(Trie)
        t.ctx, t.L, t.h = ctx, ctx.L, h
        t.n_nodes, t.n_tokens = self.num_nodes(), None
        _live["trie"].add(t)
        return t

    def close(self):
        if self.h:
            self.L.lib.fltx_htrie_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Hyp:
    __slots__ = ("score", "am", "lm", "tokens", "words")

    def __init__(self, score, am, lm, tokens, words):
        self.score, self.am, self.lm = score, am, lm
        self.tokens, self.words = tokens, words


_U8_TO_I32 = np.arange(256, dtype=np.int32)
_U8_TO_I32[255] = -1  # (fltx_result_fetch_batch_compact: 0xFF = -1)


class Transcript:
    """One hypothesis after CTC collapse (BatchDecoder.transcripts_batch): tokens and the row index at which each starts
    (the emission frame is timestep - 1), the words with the index at which each ended, and word_tok_end[j] = the tokens
    up to and including word j's end -- tokens[word_tok_end[j - 1]:word_tok_end[j]] spells word j."""
    __slots__ = ("score", "am", "lm", "tokens", "timesteps", "words", "word_timesteps", "word_tok_end")

    def __init__(self, score, am, lm, tokens, timesteps, words, word_timesteps, word_tok_end):
        self.score, self.am, self.lm = score, am, lm
        self.tokens, self.timesteps = tokens, timesteps
        self.words, self.word_timesteps, self.word_tok_end = words, word_timesteps, word_tok_end


class Partial(Transcript):
    """One stream's partial result (BatchDecoder.stream_partials_batch): the Transcript of getBestHypothesis(look_back),
    and what of it can no longer change -- the first stable_frames buffer entries, which hold the first stable_tokens
    tokens and stable_words words; buffer entry i is absolute entry first_frame + i of the stream.  status: 0, or the
    error code fltx_result_best would report for the stream (its transcript is empty then)."""
    __slots__ = ("length", "stable_frames", "stable_tokens", "stable_words", "first_frame", "status")


class _CompactHyp(Hyp):
    """A hypothesis of results_batch(): its token row stays the byte row the device packed until somebody reads it
    (an n-best of 50 x 1 002 frames is read in full by few callers; widening 12.8 M bytes per batch up front cost more
    than everything else on the way to Python objects)."""
    __slots__ = ("_t8", "_tok")

    def __init__(self, score, am, lm, t8, words):
        self.score, self.am, self.lm, self.words = score, am, lm, words
        self._t8, self._tok = t8, None

    @property
    def tokens(self):
        t = self._tok
        if t is None:
            t = self._tok = _U8_TO_I32[self._t8]
        return t


class _CompactHypSmall(_CompactHyp):
    """... over at most 128 tokens: 0xFF read as a signed byte IS -1, so widening is one astype."""
    __slots__ = ()

    @property
    def tokens(self):
        t = self._tok
        if t is None:
            t = self._tok = self._t8.view(np.int8).astype(np.int32)
        return t


class BatchDecoder:
    """fltx_decoder: batched LexiconFreeDecoder / LexiconDecoder on the device."""

    def __init__(self, ctx, kind, options, lm, sil, blank, unk=-1, trie=None, transitions=None,
                 is_lm_token=False):
        self.ctx, self.L = ctx, ctx.L
        self.kind, self.options = kind, options
        self._keep = (lm, trie)
        tr = None if transitions is None or len(transitions) == 0 else \
            np.ascontiguousarray(transitions, dtype=np.float32)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_decoder_create(
            ctx.h, kind, C.byref(options), trie.h if trie is not None else None, lm.h, sil, blank, unk,
            _ptr(tr), 0 if tr is None else tr.size, int(is_lm_token), C.byref(h)))
        self.h = h
        self.B = 0
        self.N = None  # token-set size of the last offline batch
        _live["dec"].add(self)

    def _chk(self, rc):
        """Like Lib.check; a failure reported by a host-LM callback re-raises what the user's LM raised."""
        lm = self._keep[0]
        if rc == 7 and getattr(lm, "error", None) is not None:
            e, lm.error = lm.error, None
            raise e
        self.L.check(rc)

    def set(self, key, value):
        self.L.check(self.L.lib.fltx_decoder_set(self.h, key.encode(), int(value)))

    def decode_batch(self, emissions, T, N, offsets=None, device_ptr=None):
        """emissions: host float32 array (any shape, flat layout) or None when
        device_ptr (int) addresses HBM-resident emissions."""
        T = np.ascontiguousarray(T, dtype=np.int32)
        B = len(T)
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(T.astype(np.int64) * N)[:-1]]).astype(np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if device_ptr is not None:
            self._chk(self.L.lib.fltx_decode_batch(self.h, device_ptr, 1, _ptr(offsets), _ptr(T), B, N))
        else:
            e = np.ascontiguousarray(emissions, dtype=np.float32)
            self._chk(self.L.lib.fltx_decode_batch(self.h, _ptr(e), 0, _ptr(offsets), _ptr(T), B, N))
        self.B = B
        self.N = N

    def stream_begin(self, B, N, max_frames):
        self._chk(self.L.lib.fltx_stream_begin(self.h, B, N, max_frames))
        self.B = B
        self.N = None  # (streams: fltx_result_fetch per utterance)
        self._N = N

    def stream_step(self, emissions, T, offsets=None, device_ptr=None):
        """emissions: host float32 array, or None when device_ptr (int) addresses the chunk in HBM (the buffer
        is the caller's again as soon as the call returns)."""
        T = np.ascontiguousarray(T, dtype=np.int32)
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(T.astype(np.int64) * self._N)[:-1]]).astype(np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if device_ptr is not None:
            self._chk(self.L.lib.fltx_stream_step(self.h, device_ptr, 1, _ptr(offsets), _ptr(T)))
            return
        e = np.ascontiguousarray(emissions, dtype=np.float32)
        self._chk(self.L.lib.fltx_stream_step(self.h, _ptr(e), 0, _ptr(offsets), _ptr(T)))

    def stream_end(self):
        self._chk(self.L.lib.fltx_stream_end(self.h))

    def stream_finish(self, which, device=False):
        """End the utterances of the streams `which` names (B flags) and restart those slots, leaving every other stream
        as it is (fltx_stream_finish).  device=False -> {b: the list of Hyp that results(b) gives after stream_end()} for
        the named streams; a stream whose status is not 0 raises what count(b) would raise after stream_end().
        device=True: nothing is copied; -> a dict of the integer device addresses n_hyp, length, status, scores, tokens,
        words (None: lexicon-free), row_off -- tokens / words / row_off / length are what
        Context.collapse_rows(device=True) takes.  Both stay valid until the next stream_finish(), stream_end() or
        stream_begin()."""
        w = np.ascontiguousarray(np.asarray(which) != 0, dtype=np.int32)
        assert w.size == self.B, "which: one flag per stream"
        fo = FinishedOut()
        self._chk(self.L.lib.fltx_stream_finish(self.h, _ptr(w), 1 if device else 0, C.byref(fo)))
        if device:
            return {f: getattr(fo, f) for f, _ in FinishedOut._fields_}
        fin = _finished_host(fo, w, self.B, int(self.options.beam_size))
        for b in np.flatnonzero(w):
            if fin["status"][b] != 0:
                raise FltxError(int(fin["status"][b]), "stream %d stopped before it was finished (status %d)"
                                % (b, fin["status"][b]))
        return fin["hyps"]

    def stream_prune(self, look_back=0):
        self._chk(self.L.lib.fltx_stream_prune(self.h, look_back))

    def frames_in_buffer(self, b):
        n = C.c_int32(0)
        self.L.check(self.L.lib.fltx_stream_frames_in_buffer(self.h, b, C.addressof(n)))
        return n.value

    def count(self, b):
        n, ln = C.c_int32(0), C.c_int32(0)
        self.L.check(self.L.lib.fltx_result_count(self.h, b, C.addressof(n), C.addressof(ln)))
        return n.value, ln.value

    def results(self, b, max_hyp=None):
        n, ln = self.count(b)
        if max_hyp is not None:
            n = min(n, max_hyp)
        if n == 0:
            return []
        scores = np.zeros(3 * n, dtype=np.float64)
        tokens = np.zeros((n, ln), dtype=np.int32)
        words = np.zeros((n, ln), dtype=np.int32)
        got = C.c_int32(0)
        self.L.check(self.L.lib.fltx_result_fetch(self.h, b, n, _ptr(scores), _ptr(tokens), _ptr(words),
                                                  C.addressof(got)))
        assert got.value == n
        return [Hyp(scores[3 * i], scores[3 * i + 1], scores[3 * i + 2], tokens[i].copy(), words[i].copy())
                for i in range(n)]

    def fetch_batch_raw(self):
        """The six pointers of fltx_result_fetch_batch (n_hyp, length, scores, tokens, words, offsets)."""
        ptrs = [C.c_void_p() for _ in range(6)]
        self.L.check(self.L.lib.fltx_result_fetch_batch(self.h, *[C.byref(p) for p in ptrs]))
        return [p.value for p in ptrs]

    def results_arrays(self):
        """n-best of every utterance of the last decode_batch as NumPy arrays over the
        decoder's pinned host buffers (one transfer per array; valid until the next decode):
        n_hyp [B], length [B], scores [B, K, 3] (score, emitting-model score, LM score),
        tokens / words: flat int32 with offsets [B + 1] -- hypothesis i of utterance b is
        tokens[offsets[b] + i * length[b] : offsets[b] + (i + 1) * length[b]]."""
        pn, pl, ps, pt, pw, po = (C.c_void_p() for _ in range(6))
        self.L.check(self.L.lib.fltx_result_fetch_batch(self.h, C.byref(pn), C.byref(pl), C.byref(ps), C.byref(pt),
                                                        C.byref(pw), C.byref(po)))
        B = self.B

        def view(ptr, ctype, n):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))
        off = view(po, C.c_int64, B + 1)
        total = int(off[B])
        K = int(self.options.beam_size)
        return {"n_hyp": view(pn, C.c_int32, B), "length": view(pl, C.c_int32, B), "offsets": off,
                "scores": view(ps, C.c_double, B * K * 3).reshape(B, K, 3),
                "tokens": view(pt, C.c_int32, max(total, 1)),
                "words": view(pw, C.c_int32, max(total, 1)) if pw.value else None}

    def results_arrays_compact(self):
        """The same through fltx_result_fetch_batch_compact: only the rows of the hypotheses that exist cross
        PCIe, tokens as uint8 (0xFF = -1), words as int32 rows; `offsets` [B + 1] index both flat arrays.
        tokens_of(r, b, i) / words_of(r, b, i) below widen one hypothesis' rows on demand."""
        pn, pl, ps, pt, pw, po = (C.c_void_p() for _ in range(6))
        self.L.check(self.L.lib.fltx_result_fetch_batch_compact(self.h, C.byref(pn), C.byref(pl), C.byref(ps),
                                                                C.byref(pt), C.byref(pw), C.byref(po)))
        B = self.B

        def view(ptr, ctype, n):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))
        off = view(po, C.c_int64, B + 1)
        total = int(off[B])
        K = int(self.options.beam_size)
        return {"n_hyp": view(pn, C.c_int32, B), "length": view(pl, C.c_int32, B), "offsets": off,
                "scores": view(ps, C.c_double, B * K * 3).reshape(B, K, 3),
                "tokens_u8": view(pt, C.c_uint8, max(total, 1)),
                "words": view(pw, C.c_int32, max(total, 1)) if pw.value else None}

    @staticmethod
    def tokens_of(r, b, i):
        L, o = int(r["length"][b]), int(r["offsets"][b])
        t = r["tokens_u8"][o + i * L:o + (i + 1) * L].astype(np.int32)
        t[t == 255] = -1
        return t

    @staticmethod
    def words_of(r, b, i):
        L, o = int(r["length"][b]), int(r["offsets"][b])
        return r["words"][o + i * L:o + (i + 1) * L] if r["words"] is not None else np.full(L, -1, dtype=np.int32)

    def results_batch(self, max_hyp=None):
        """[[Hyp]] for every utterance: Python objects over the arrays of results_arrays_compact()
        (or results_arrays() for token sets that do not fit a byte)."""
        compact = self.N is not None and self.N < 255
        if compact:
            r = self.results_arrays_compact()
            nh, ln, off, sc, wrd = r["n_hyp"], r["length"], r["offsets"], r["scores"], r["words"]
            total = int(off[self.B])
            tok = r["tokens_u8"][:total].copy()  # (the library's buffer is the next batch's too)
            wrd = wrd[:total].copy() if wrd is not None else None
        else:
            r = self.results_arrays()
            nh, ln, off, sc, tok, wrd = r["n_hyp"], r["length"], r["offsets"], r["scores"], r["tokens"], r["words"]
        make = (_CompactHypSmall if self.N <= 128 else _CompactHyp) if compact else Hyp
        no_words = {}
        out = []
        for b in range(self.B):
            n = int(nh[b]) if max_hyp is None else min(int(nh[b]), max_hyp)
            L = int(ln[b])
            o = int(off[b])
            tb = tok[o:o + n * L].reshape(n, L)
            if wrd is not None:
                wb = wrd[o:o + n * L].reshape(n, L)
            else:  # lexicon-free: every word slot is -1 (LexiconFreeDecoder.h:80-82) -- one read-only row per length
                row = no_words.get(L)
                if row is None:
                    row = no_words[L] = np.full(L, -1, dtype=np.int32)
                    row.flags.writeable = False
                wb = None
            s3 = sc[b, :n].tolist()
            out.append([make(s3[i][0], s3[i][1], s3[i][2], tb[i], wb[i] if wb is not None else row) for i in range(n)])
        return out

    def transcripts(self, max_hyp=None, device=False):
        """fltx_result_transcripts: the n-best of the last finished decode after CTC collapse, made on the device -- the
        first min(n_hyp[b], max_hyp) hypotheses of every utterance, best first.  -> a dict: row_first [B + 1] (the rows
        of utterance b are row_first[b] .. row_first[b + 1]), scores [B, K, 3], and per row r tokens / timesteps at
        tok_off[r]:tok_off[r + 1], words / word_timesteps / word_tok_end at word_off[r]:word_off[r + 1] -- NumPy
        views of the decoder's pinned buffers, valid until the next call or decode.  device=True: the arrays stay in
        HBM; their keys hold integer addresses and n_tokens / n_words the sizes (row_first stays a host array)."""
        K = int(self.options.beam_size)
        t = Transcripts()
        self._chk(self.L.lib.fltx_result_transcripts(self.h, K if max_hyp is None else int(max_hyp),
                                                     1 if device else 0, C.byref(t)))
        r = _transcript_views(t, device)
        r["row_first"] = _view(t.row_first, C.c_int64, self.B + 1)
        if device:
            r["scores"] = t.scores
        else:
            r["scores"] = _view(t.scores, C.c_double, self.B * K * 3).reshape(self.B, K, 3)
        return r

    def transcripts_batch(self, max_hyp=None):
        """[[Transcript]] for every utterance: the arrays of transcripts() copied once, sliced per hypothesis"""
        r = self.transcripts(max_hyp)
        first, to, wo = r["row_first"].tolist(), r["tok_off"].tolist(), r["word_off"].tolist()
        tok, ts = r["tokens"].copy(), r["timesteps"].copy()
        wrd, wts, wte = r["words"].copy(), r["word_timesteps"].copy(), r["word_tok_end"].copy()
        out = []
        for b in range(self.B):
            s3 = r["scores"][b].tolist()
            out.append([Transcript(s3[i][0], s3[i][1], s3[i][2], tok[to[q]:to[q + 1]], ts[to[q]:to[q + 1]],
                                   wrd[wo[q]:wo[q + 1]], wts[wo[q]:wo[q + 1]], wte[wo[q]:wo[q + 1]])
                        for i, q in enumerate(range(first[b], first[b + 1]))])
        return out

    def stream_partials(self, look_back=0, device=False):
        """fltx_stream_partials: inside a stream, the partial transcript of every stream in one call -- row b is
        getBestHypothesis(look_back) of stream b after CTC collapse, made on the device -- and how much of it is final.
        -> a dict: the keys of transcripts() without row_first (n_rows = B), scores [B, 3], and per stream length
        (frames of the result), stable_frames / stable_tokens / stable_words (the leading buffer entries every
        hypothesis of the current beam shares, and the row's tokens / words inside them), first_frame (int64: frames
        pruned away so far) and status.  NumPy views of the decoder's pinned buffers, valid until the next call that
        steps, appends, prunes or asks again.  device=True: integer addresses of the arrays in HBM."""
        o = StreamPartialsOut()
        self._chk(self.L.lib.fltx_stream_partials(self.h, int(look_back), 1 if device else 0, C.byref(o)))
        r = _transcript_views(o.t, device)
        B = self.B
        if device:
            r.update(scores=o.t.scores, length=o.length, stable_frames=o.stable_frames, stable_tokens=o.stable_tokens,
                     stable_words=o.stable_words, first_frame=o.first_frame, status=o.status)
            return r
        r["scores"] = _view(o.t.scores, C.c_double, 3 * B).reshape(B, 3)
        for k in ("length", "stable_frames", "stable_tokens", "stable_words", "status"):
            r[k] = _view(getattr(o, k), C.c_int32, B)
        r["first_frame"] = _view(o.first_frame, C.c_int64, B)
        return r

    def stream_partials_batch(self, look_back=0):
        """[Partial] per stream: the arrays of stream_partials() copied once, sliced per stream"""
        r = self.stream_partials(look_back)
        to, wo = r["tok_off"].tolist(), r["word_off"].tolist()
        tok, ts = r["tokens"].copy(), r["timesteps"].copy()
        wrd, wts, wte = r["words"].copy(), r["word_timesteps"].copy(), r["word_tok_end"].copy()
        sc = r["scores"].tolist()
        num = {k: r[k].tolist() for k in Partial.__slots__}
        out = []
        for b in range(self.B):
            p = Partial(sc[b][0], sc[b][1], sc[b][2], tok[to[b]:to[b + 1]], ts[to[b]:to[b + 1]], wrd[wo[b]:wo[b + 1]],
                        wts[wo[b]:wo[b + 1]], wte[wo[b]:wo[b + 1]])
            for k, v in num.items():
                setattr(p, k, v[b])
            out.append(p)
        return out

    def best(self, b, look_back=0, capacity=1 << 16):
        scores = np.zeros(3, dtype=np.float64)
        tokens = np.zeros(capacity, dtype=np.int32)
        words = np.zeros(capacity, dtype=np.int32)
        ln = C.c_int32(0)
        self.L.check(self.L.lib.fltx_result_best(self.h, b, look_back, _ptr(scores), _ptr(tokens),
                                                 _ptr(words), capacity, C.addressof(ln)))
        n = ln.value
        return Hyp(scores[0], scores[1], scores[2], tokens[:n].copy(), words[:n].copy())

    def get(self, key):
        v = C.c_int64(0)
        self.L.check(self.L.lib.fltx_decoder_get(self.h, key.encode(), C.addressof(v)))
        return v.value

    def stats(self):
        fr, by = C.c_int64(0), C.c_int64(0)
        th, lds = C.c_int32(0), C.c_int32(0)
        self.L.check(self.L.lib.fltx_decoder_stats(self.h, C.addressof(fr), C.addressof(by),
                                                   C.addressof(th), C.addressof(lds)))
        return {"frames": fr.value, "algorithmic_bytes": by.value, "threads_per_utt": th.value,
                "lds_bytes": lds.value}

    def bytes(self):
        """Algorithmic bytes of the last offline decode, split by kernel."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.L.check(self.L.lib.fltx_decoder_bytes(self.h, C.addressof(a), C.addressof(b), C.addressof(c)))
        return {"decode": a.value, "epilogue": b.value, "lm": c.value}

    def profile(self):
        out = np.zeros(8, dtype=np.uint64)
        self.L.check(self.L.lib.fltx_decoder_profile(self.h, _ptr(out)))
        return out

    def timing(self):
        a, b = C.c_float(0), C.c_float(0)
        self.L.check(self.L.lib.fltx_decoder_timing(self.h, C.addressof(a), C.addressof(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            self.L.lib.fltx_decoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# fltx_s2s_step_typed: element types (fltx_dtype) and kinds of the rows
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2
S2S_KINDS = {"log_probs": 0, "logits": 1}
_NP_DTYPES = {DTYPE_F32: np.float32, DTYPE_F16: np.float16, DTYPE_BF16: np.uint16}


def _torch_dtypes():
    import torch
    return {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}


class Seq2SeqBatchDecoder(BatchDecoder):
    """fltx_s2s_*: LexiconFreeSeq2SeqDecoder for B utterances at once, one device step per model call.

    begin(B, V) and step(scores) return the next call's rows (token, beam_idx, src_row) as [B, K] int32 and n_rows as
    [B] int32: torch tensors allocated on the context's device (numpy arrays on the emulator library).  Row k of
    utterance b is row b*K + k of the scores the model returns; rows k >= n_rows[b] are padding.  src_row is what the
    model passes to index_select on its per-row state (-1 for the root and padding).  After end(), the results*
    methods of BatchDecoder read the n-best (rows of max_output_length + 3 tokens, -1 in front).  Create the context
    on the torch stream the model runs on so that the model's kernels and the decoder's are ordered without a host
    wait -- a stream of its own (torch.cuda.Stream()): the default stream's handle is NULL, and a context given NULL
    makes a stream of its own."""

    def __init__(self, ctx, options, lm, eos, max_output_length):
        self.ctx, self.L = ctx, ctx.L
        self.kind, self.options = S2S_LEXFREE, options
        self._keep = (lm, None)
        self.eos, self.max_output_length = int(eos), int(max_output_length)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_s2s_decoder_create(ctx.h, C.byref(options), lm.h, self.eos,
                                                        self.max_output_length, C.byref(h)))
        self.h = h
        self.B = 0
        self.N = None
        self.V = None
        self._emu = "emulation" in self.L.version()
        _live["dec"].add(self)

    @property
    def has_rows_lm(self):
        """the decoder (either seq2seq kind) was made with a RowsLM: step() takes lm_scores"""
        return isinstance(self._keep[0], RowsLM)

    def _rows(self):
        B, K = self.B, int(self.options.beam_size)
        if self._emu:  # (the emulator's "device" memory is host memory)
            return [np.empty((B, K), np.int32) for _ in range(3)] + [np.empty(B, np.int32)]
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        return [torch.empty((B, K), dtype=torch.int32, device=dev) for _ in range(3)] + \
            [torch.empty(B, dtype=torch.int32, device=dev)]

    @staticmethod
    def _addr(a):
        return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()

    def begin(self, B, V):
        self.B, self.V, self.N = int(B), int(V), None
        out = self._rows()
        self._chk(self.L.lib.fltx_s2s_begin(self.h, self.B, self.V, *[self._addr(o) for o in out]))
        return tuple(out)

    def _rows_in(self, scores, dtype, BK, what="scores"):
        """-> (the array kept alive, fltx_dtype, row stride, address, on_device, the rows live on the host)"""
        if isinstance(scores, np.ndarray):
            if dtype is not None:
                if dtype not in ("bf16", "bfloat16") or scores.dtype != np.uint16:
                    raise TypeError("dtype=%r: numpy rows of bfloat16 bits are uint16 with dtype='bf16'" % (dtype,))
                dt = DTYPE_BF16
            elif scores.dtype == np.float16:
                dt = DTYPE_F16
            else:
                dt = DTYPE_F32
            sc = np.ascontiguousarray(scores, dtype=_NP_DTYPES[dt]).reshape(BK, -1)
            return sc, dt, sc.shape[1], sc.ctypes.data, 1 if self._emu else 0, True
        import torch
        sc = scores.reshape(-1, scores.shape[-1])
        dts = {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}
        assert sc.dtype in dts and sc.stride(-1) == 1, \
            "%s: float32 / float16 / bfloat16 rows of unit column stride" % what
        cpu = sc.device.type == "cpu"
        return sc, dts[sc.dtype], sc.stride(0), sc.data_ptr(), 0 if cpu else 1, cpu

    def _lse_ptr(self, lse_out, BK):
        if lse_out is None:
            return None
        n_lse = lse_out.size if isinstance(lse_out, np.ndarray) else lse_out.numel()
        assert n_lse >= BK and str(lse_out.dtype).endswith("float64"), "lse_out: B*K float64 on the device"
        return self._addr(lse_out)

    def step(self, scores, row_valid=None, *, kind="log_probs", lse_out=None, dtype=None, lm_scores=None,
             lm_kind="log_probs", lm_lse_out=None, lm_dtype=None):
        """scores: [B*K, >= V] rows b*K + k: a torch tensor of float32, float16 or bfloat16 on the device or the host
        (any row stride, unit column stride), or a numpy float32 / float16 array -- or uint16 holding bfloat16 bits
        with dtype="bf16".  kind: "log_probs" (the model's scores) or "logits" (the step takes each row's
        log-softmax itself, fltx_s2s_step_typed).  lse_out: None or a device float64 tensor of B*K that receives each
        live row's log-sum-exp in logits mode (NaN for the other rows).  row_valid: None or B*K bytes / bools (0: the
        model dropped the row).  float32 log-probs go through fltx_s2s_step exactly as before.
        lm_scores / lm_kind / lm_lse_out / lm_dtype: the rows of a RowsLM ([B*K, >= lm_width], the same forms as
        `scores` and on the same side -- both on the device or both on the host), required when the decoder was made
        with one and refused otherwise (fltx_s2s_step_lm_rows)."""
        if kind not in S2S_KINDS or lm_kind not in S2S_KINDS:
            raise ValueError("kind: one of %s" % sorted(S2S_KINDS))
        if (lm_scores is not None) != self.has_rows_lm:
            raise FltxError(ERR_STATE, "%s.step: lm_scores go with a decoder made with a RowsLM, and such a decoder "
                            "takes them at every step" % type(self).__name__)
        out = self._rows()
        ptrs = [self._addr(o) for o in out]
        BK = self.B * int(self.options.beam_size)
        sc, dt, stride, ptr, on_dev, host = self._rows_in(scores, dtype, BK)
        if isinstance(scores, np.ndarray):
            rv = None if row_valid is None else np.ascontiguousarray(row_valid, dtype=np.uint8)
            rvp = None if rv is None else rv.ctypes.data
        elif host:
            rv = None if row_valid is None else np.ascontiguousarray(
                row_valid.cpu().numpy() if hasattr(row_valid, "cpu") else row_valid, dtype=np.uint8)
            rvp = None if rv is None else rv.ctypes.data
        else:
            import torch
            rv = None if row_valid is None else row_valid.reshape(-1).to(torch.uint8).contiguous()
            rvp = None if rv is None else rv.data_ptr()
        lsc = None
        if lm_scores is not None:
            lsc, ldt, lstride, lptr, l_on_dev, _ = self._rows_in(lm_scores, lm_dtype, BK, "lm_scores")
            assert l_on_dev == on_dev, "scores and lm_scores: both on the device or both on the host"
            self._chk(self.L.lib.fltx_s2s_step_lm_rows(self.h, ptr, dt, S2S_KINDS[kind], stride, lptr, ldt,
                                                        S2S_KINDS[lm_kind], lstride, on_dev, rvp,
                                                        self._lse_ptr(lse_out, BK), self._lse_ptr(lm_lse_out, BK),
                                                        *ptrs))
        elif dt == DTYPE_F32 and kind == "log_probs":
            self._chk(self.L.lib.fltx_s2s_step(self.h, ptr, on_dev, stride, rvp, *ptrs))
        else:
            self._chk(self.L.lib.fltx_s2s_step_typed(self.h, ptr, dt, S2S_KINDS[kind], on_dev, stride, rvp,
                                                      self._lse_ptr(lse_out, BK), *ptrs))
        self._inputs = (sc, rv, lsc)  # (kept until the next step: the kernels read them asynchronously)
        return tuple(out)

    def done(self):
        v = C.c_int32(0)
        self.L.check(self.L.lib.fltx_s2s_done(self.h, C.addressof(v)))
        return bool(v.value)

    def end(self):
        self._chk(self.L.lib.fltx_s2s_end(self.h))
        self.N = self.V

    def done_each(self):
        """-> [B] bool: the utterance in the slot is done, or the slot is parked (fltx_s2s_done_each; a host wait)"""
        v = np.zeros(max(self.B, 1), np.int32)
        self.L.check(self.L.lib.fltx_s2s_done_each(self.h, _ptr(v)))
        return v[:self.B] != 0

    def finish(self, which, results_on_device=False):
        """End the utterances of the slots `which` names (B entries: 0 leave, 1 finish + restart, 2 finish + park),
        leaving every other utterance as it is (fltx_s2s_finish).  -> (lists, finished): the lists are step()'s
        (token, beam_idx, src_row, n_rows[, next_word]) -- the root for a restarted slot, nothing for a parked one,
        every other slot's rows again with src_row the row itself.  finished, results_on_device=False: a dict with
        n_hyp, steps, status ([B] int32 copies; status 0 or the error code count(b) would raise with after end()) and
        hyps = {b: the list of Hyp that results(b) gives after end()} for the named slots.  results_on_device=True:
        nothing is copied and the call does not wait; the dict holds the integer device addresses n_hyp, steps, status,
        scores, tokens, words (None: lexicon-free) and `length`.  Both stay valid until the next finish(), end() or
        begin(); steps do not disturb them."""
        w = np.ascontiguousarray(np.asarray(which), dtype=np.int32).reshape(-1)
        assert w.size == self.B, "which: one entry per slot"
        out = self._rows()
        word = None
        if isinstance(self._keep[0], WordRowsLM):
            word = out[0].copy() if self._emu else out[0].clone()
        fo = S2sFinishedOut()
        self._chk(self.L.lib.fltx_s2s_finish(self.h, _ptr(w), *[self._addr(o) for o in out],
                                             None if word is None else self._addr(word),
                                             1 if results_on_device else 0, C.byref(fo)))
        if word is not None:
            out.append(word)
        if results_on_device:
            return tuple(out), {f: getattr(fo, f) for f, _ in S2sFinishedOut._fields_}
        B, K, ln = self.B, int(self.options.beam_size), int(fo.length)
        n_hyp, steps, status = (_view(p, C.c_int32, B).copy() for p in (fo.n_hyp, fo.steps, fo.status))
        scores = _view(fo.scores, C.c_double, 3 * B * K)
        hyps = {}
        for b in map(int, np.flatnonzero(w)):
            hyps[b] = []
            for i in range(int(n_hyp[b]) if status[b] == 0 else 0):
                at = (b * K + i) * ln
                tk = _view(fo.tokens + 4 * at, C.c_int32, ln).copy()
                wd = _view(fo.words + 4 * at, C.c_int32, ln).copy() if fo.words else np.full(ln, -1, np.int32)
                s = scores[3 * (b * K + i):3 * (b * K + i) + 3]
                hyps[b].append(Hyp(float(s[0]), float(s[1]), float(s[2]), tk, wd))
        return tuple(out), {"n_hyp": n_hyp, "steps": steps, "status": status, "hyps": hyps}

    def _finish_between(self, listed, which):
        """finish(which) between the call that returned `listed` and the step_fn call that consumes it.  step_fn gathers
        its state and advances it in one call and has not seen `listed` yet: the slots that are not named keep the
        src_row `listed` has for them (-1 on a root row; the finish lists the same rows with src_row the row itself),
        the named ones take the finish's.  -> (lists, finished)"""
        lists, fin = self.finish(which)
        named = np.asarray(which) != 0
        if self._emu:
            src = np.where(named[:, None], lists[2], listed[2])
        else:
            import torch
            src = torch.where(torch.as_tensor(named, device=lists[2].device)[:, None], lists[2], listed[2])
        return lists[:2] + (src,) + lists[3:], fin

    def decode_queue(self, step_fn, n_utterances, B, V, check_every=4, *, kind="log_probs"):
        """Continuous batching: n_utterances go through B slots, none waits for another.  The loop steps, asks
        done_each() every `check_every` steps (a host wait), finishes the done slots, admits the next utterances of
        the queue into them and parks slots once the queue is empty.  step_fn(token [B*K], src_row [B*K], row_mask
        [B*K] bool, t, slot_utt, restarted) -> what decode()'s step_fn returns (a decoder made with a RowsLM:
        (scores, row_valid, lm_scores)); slot_utt [B] int64 (host): the queue entry in each slot, -1 for a parked one;
        restarted [B] bool (host): the slots whose single listed row is a new utterance's root -- the model starts
        their state afresh (src_row is -1 there).  A decoder with a WordRowsLM is stepped by hand (lm_row_of is the
        caller's).  -> [[Hyp]] in queue order, each what decode() returns for that utterance."""
        assert not isinstance(self._keep[0], WordRowsLM), "decode_queue: step a WordRowsLM decoder by hand"
        K = int(self.options.beam_size)
        n_utt, B = int(n_utterances), int(B)
        results = [None] * n_utt
        slot_utt = np.full(B, -1, np.int64)
        lists = self.begin(B, V)
        nxt = min(B, n_utt)
        slot_utt[:nxt] = np.arange(nxt)
        restarted = slot_utt >= 0
        if nxt < B:  # fewer utterances than slots: the rest is parked before the first step
            lists, _ = self._finish_between(lists, np.where(slot_utt >= 0, 0, 2).astype(np.int32))
        if self._emu:
            ar = np.arange(K, dtype=np.int32)
        else:
            import torch
            ar = torch.arange(K, device=lists[3].device, dtype=torch.int32)
        t = since = 0
        while (slot_utt >= 0).any():
            tok, beam, src, n = lists[:4]
            mask = (ar[None, :] < n[:, None]).reshape(-1)
            r = step_fn(tok.reshape(-1), src.reshape(-1), mask, t, slot_utt.copy(), restarted.copy())
            r = r if isinstance(r, tuple) else (r, None)
            kw = {"lm_scores": r[2]} if len(r) > 2 else {}
            lists = self.step(r[0], r[1], kind=kind, **kw)
            restarted = np.zeros(B, bool)
            t += 1
            since += 1
            if since < min(check_every, self.max_output_length):
                continue
            since = 0
            done = self.done_each() & (slot_utt >= 0)
            if not done.any():
                continue
            which = np.zeros(B, np.int32)
            for b in np.flatnonzero(done):
                which[b] = 1 if nxt < n_utt else 2
                nxt += which[b] == 1
            lists, fin = self._finish_between(lists, which)
            for b in np.flatnonzero(done):
                if fin["status"][b] != 0:
                    raise FltxError(int(fin["status"][b]), "decode_queue: utterance %d stopped" % slot_utt[b])
                results[slot_utt[b]] = fin["hyps"][int(b)]
            adm = nxt - int((which == 1).sum())
            for b in np.flatnonzero(which == 1):
                slot_utt[b] = adm
                adm += 1
                restarted[b] = True
            slot_utt[which == 2] = -1
        self.end()
        return results

    def decode(self, step_fn, B, V, check_every=8, *, kind="log_probs"):
        """The whole search: step_fn(token [B*K], src_row [B*K], row_mask [B*K] bool, t) -> scores [B*K, V] (or
        (scores, row_valid)) is called until every utterance is done; returns results_batch().  A step after the
        last one is a no-op, so done() -- a host wait -- is asked every `check_every` steps only.  kind="logits":
        step_fn returns the model's raw logits (float32 / float16 / bfloat16), see step()."""
        import torch
        K = int(self.options.beam_size)
        tok, beam, src, n = self.begin(B, V)
        ar = torch.arange(K, device=n.device, dtype=torch.int32)
        for t in range(self.max_output_length):
            if t % check_every == 0 and self.done():
                break
            mask = (ar[None, :] < n[:, None]).reshape(-1)
            r = step_fn(tok.reshape(-1), src.reshape(-1), mask, t)
            scores, valid = r if isinstance(r, tuple) else (r, None)
            tok, beam, src, n = self.step(scores, valid, kind=kind)
        self.end()
        return self.results_batch()


class LexiconSeq2SeqBatchDecoder(Seq2SeqBatchDecoder):
    """fltx_s2s_lex_*: LexiconSeq2SeqDecoder for B utterances at once, with Seq2SeqBatchDecoder's begin / step / done /
    end / decode loop and row contract.  `trie` is a HostTrie (already smeared) or anything with an fltx_htrie handle
    `.h`; `lm` a ZeroLM / n-gram LM of this module (words are its user ids, tokens when is_lm_token), or -- with
    is_lm_token=True only -- a RowsLM: a neural token LM whose rows go to step(..., lm_scores=) next to the model's,
    exactly as on Seq2SeqBatchDecoder (a word-level RowsLM is refused).  A row's token move, its word end and eos read
    the row's one LM entry (usr_to_lm[token]; finish_index for eos); there is no shortcut at lm_weight == 0; the token
    beam min(beam_size_token, V) is at most 256.  The LM must be a pure function of the token prefix: hypotheses that
    spell one token string differently share an LM state and merge, and the merged survivor's next_src_row is the best
    member's -- index_select the LM's state by it as the model's.  The results carry words."""

    def __init__(self, ctx, options, trie, lm, eos, max_output_length, is_lm_token=False):
        self.ctx, self.L = ctx, ctx.L
        self.kind, self.options = S2S_LEXICON, options
        self._keep = (lm, trie)
        self.eos, self.max_output_length = int(eos), int(max_output_length)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_s2s_lex_decoder_create(ctx.h, C.byref(options), trie.h, lm.h, self.eos,
                                                            self.max_output_length, int(bool(is_lm_token)),
                                                            C.byref(h)))
        self.h = h
        self.B = 0
        self.N = None
        self.V = None
        self._emu = "emulation" in self.L.version()
        _live["dec"].add(self)

    def set_max_states(self, n):
        self.L.check(self.L.lib.fltx_s2s_lex_set_max_states(self.h, int(n)))

    @property
    def has_word_rows_lm(self):
        """the decoder was made with a WordRowsLM: step() takes lm_scores / lm_row_of and returns next_word too"""
        return isinstance(self._keep[0], WordRowsLM)

    def step(self, scores, row_valid=None, *, lm_row_of=None, **kw):
        """Seq2SeqBatchDecoder.step.  With a WordRowsLM (is_lm_token=False): lm_scores is [n_lm_rows, >= lm_width], one
        row per LM STATE, and lm_row_of (None: identity, lm_scores then has B*K rows) B*K int32 -- a device tensor, or
        numpy on the host side -- naming the LM row of each decoder row; an entry outside [0, n_lm_rows) takes the
        row's word ends and eos away.  Returns (token, beam_idx, src_row, n_rows, next_word): next_word [B, K] int32
        is the word each listed row's hypothesis ended in this step, -1 for none and on padding rows.  The caller's
        recipe: the LM state of next row r is that of row src_row[r] when next_word[r] < 0 (reuse its LM row), else
        that state advanced by next_word[r] (run the LM for it alone).  The LM must be a pure function of the word
        prefix.  lm_lse_out is indexed by decoder row (fltx_s2s_step_word_lm_rows)."""
        if not self.has_word_rows_lm:
            if lm_row_of is not None:
                raise FltxError(ERR_STATE, "%s.step: lm_row_of goes with a decoder made with a WordRowsLM"
                                % type(self).__name__)
            return super().step(scores, row_valid, **kw)
        kind, lm_kind = kw.pop("kind", "log_probs"), kw.pop("lm_kind", "log_probs")
        lse_out, lm_lse_out = kw.pop("lse_out", None), kw.pop("lm_lse_out", None)
        dtype, lm_dtype, lm_scores = kw.pop("dtype", None), kw.pop("lm_dtype", None), kw.pop("lm_scores", None)
        if kw:
            raise TypeError("step: unexpected arguments %s" % sorted(kw))
        if kind not in S2S_KINDS or lm_kind not in S2S_KINDS:
            raise ValueError("kind: one of %s" % sorted(S2S_KINDS))
        if lm_scores is None:
            raise FltxError(ERR_STATE, "%s.step: a decoder made with a WordRowsLM takes lm_scores at every step"
                            % type(self).__name__)
        out = self._rows()
        out.append(out[0].copy() if self._emu else out[0].clone())  # next_word
        BK = self.B * int(self.options.beam_size)
        sc, dt, stride, ptr, on_dev, host = self._rows_in(scores, dtype, BK)
        if row_valid is None:
            rv = None
        elif host:
            rv = np.ascontiguousarray(row_valid.cpu().numpy() if hasattr(row_valid, "cpu") else row_valid, dtype=np.uint8)
        else:
            import torch
            rv = row_valid.reshape(-1).to(torch.uint8).contiguous()
        # the LM's rows: any number of them (one per LM state), the same forms and side as `scores`
        if isinstance(lm_scores, np.ndarray):
            if lm_dtype is not None:
                if lm_dtype not in ("bf16", "bfloat16") or lm_scores.dtype != np.uint16:
                    raise TypeError("lm_dtype=%r: numpy rows of bfloat16 bits are uint16 with lm_dtype='bf16'" % (lm_dtype,))
                ldt = DTYPE_BF16
            else:
                ldt = DTYPE_F16 if lm_scores.dtype == np.float16 else DTYPE_F32
            l_on_dev = 1 if self._emu else 0
            lsc = np.ascontiguousarray(lm_scores, dtype=_NP_DTYPES[ldt]).reshape(-1, lm_scores.shape[-1])
            lstride, lptr = lsc.shape[1], lsc.ctypes.data
        else:
            lsc, ldt, lstride, lptr, l_on_dev, _ = self._rows_in(lm_scores, lm_dtype, BK, "lm_scores")
        assert l_on_dev == on_dev, "scores and lm_scores: both on the device or both on the host"
        n_lm = int(lsc.shape[0])
        ro = None
        if lm_row_of is not None:
            if isinstance(lm_row_of, np.ndarray) or host:
                ro = np.ascontiguousarray(lm_row_of.cpu().numpy() if hasattr(lm_row_of, "cpu") else lm_row_of,
                                          dtype=np.int32).reshape(-1)
                n_ro = ro.size
            else:
                import torch
                ro = lm_row_of.reshape(-1).to(torch.int32).contiguous()
                n_ro = ro.numel()
            assert n_ro == BK, "lm_row_of: B*K entries"
        else:
            assert n_lm >= BK, "lm_scores: B*K rows without lm_row_of"
        self._chk(self.L.lib.fltx_s2s_step_word_lm_rows(
            self.h, ptr, dt, S2S_KINDS[kind], stride, lptr, ldt, S2S_KINDS[lm_kind], lstride,
            None if ro is None else self._addr(ro), n_lm, on_dev, None if rv is None else self._addr(rv),
            self._lse_ptr(lse_out, BK), self._lse_ptr(lm_lse_out, BK), self._addr(out[0]), self._addr(out[1]),
            self._addr(out[2]), self._addr(out[4]), self._addr(out[3])))
        self._inputs = (sc, rv, lsc, ro)  # (kept until the next step: the kernels read them asynchronously)
        return tuple(out)

    def info(self):
        """-> dict(trie_bytes, nodes, edges, merges: per utterance since begin, or None before it)."""
        tb, nn, ne = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        m = np.zeros(max(self.B, 1), np.int32)
        self.L.check(self.L.lib.fltx_s2s_lex_info(self.h, C.addressof(tb), C.addressof(nn), C.addressof(ne),
                                                  _ptr(m) if self.B else None))
        return dict(trie_bytes=tb.value, nodes=nn.value, edges=ne.value, merges=m.tolist() if self.B else None)


class CtcRowsBatchDecoder(BatchDecoder):
    """fltx_ctc_rows_*: LexiconFreeDecoder (CTC) for B utterances at once with a neural token LM in shallow fusion, one
    device step per frame.  `rows_lm` is a RowsLM with a finish_index >= 0; `options` are make_options(...)'s with the
    CTC criterion (word_score / unk_score ignored).

    begin(emissions, T, N) and step(lm_scores) return the next call's rows (token, src_row, state) as [B, K] int32 and
    n_rows as [B] int32 -- torch tensors on the context's device (numpy arrays on the emulator library).  Row k of
    utterance b is hypothesis k of its current beam; `state` is the hypothesis' LM-state id within the utterance, stable
    for the whole decode; `token` is the token that advanced the state in this frame (-1: the state is that of row
    src_row); rows k >= n_rows[b] are padding (-1).  lm_scores is [n_lm_rows, >= lm_width], ONE ROW PER LM STATE, and
    lm_row_of (B*K int32; None: identity) names the LM row of each decoder row.  end(lm_scores) reads each row's finish
    entry; then the results* methods read the n-best (T[b] + 2 tokens, as decode_batch gives them).  decode() drives it
    all from a callable.  Streams: stream_begin(B, N, max_frames), then append(chunk, T) and as many step() calls as it
    returns, prune(look_back), best(b, look_back) -- getBestHypothesis(lookBack), an empty result has no tokens --
    frames_in_buffer(b), and end(); decode_stream() drives those.  A stream's state ids stay stable until collect()
    lists them as released: a released id may come back for another state.  stream_finish(which, lm_scores) ends the
    utterances of single streams and restarts those slots while the others decode on.  plan_begin(row_capacity), plan(lists) and
    plan_release(released, n_released) keep the LM rows of the state ids on the device (fltx_ctc_rows_plan_*);
    decode_device() and decode_stream_device() are decode() and decode_stream() on those."""

    _rows = Seq2SeqBatchDecoder._rows
    _addr = staticmethod(Seq2SeqBatchDecoder._addr)
    _lse_ptr = Seq2SeqBatchDecoder._lse_ptr

    def __init__(self, ctx, options, rows_lm, sil, blank):
        self._init(ctx, CTC_ROWS, options, rows_lm, None, sil, blank)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_ctc_rows_decoder_create(ctx.h, C.byref(options), rows_lm.h, int(sil), int(blank),
                                                             C.byref(h)))
        self._made(h)

    def _init(self, ctx, kind, options, lm, trie, sil, blank):
        self.ctx, self.L = ctx, ctx.L
        self.kind, self.options = kind, options
        self._keep = (lm, trie)
        self.sil, self.blank = int(sil), int(blank)

    def _made(self, h):
        self.h = h
        self.B = 0
        self.N = None
        self._emu = "emulation" in self.L.version()
        self._max_states = 65536    # what the next begin / stream_begin gives every utterance
        self._stream_states = 65536  # what the open stream got: collect()'s default cap
        _live["dec"].add(self)

    @staticmethod
    def _state_key(b, prefix, parent_id, edge, state_id):
        """what decode() hands lm_rows for a state it has not seen"""
        return (b, prefix)

    def set_max_states(self, n):
        """LM states per utterance from the next begin() on (default 65 536)"""
        self.set("max_states", n)

    def set(self, key, value):
        BatchDecoder.set(self, key, value)
        if key == "max_states":  # (takes effect at the next begin: an open stream keeps its table)
            self._max_states = int(value)

    def _frames_in(self, emissions, dtype, kind, offsets, T, N):
        """The typed forms of begin() / append() -> None for the float32 log-probs numpy route of the existing entry
        points, else (the array kept alive, fltx_dtype, address, on_device, offsets, frame stride in elements)"""
        if kind not in S2S_KINDS:
            raise ValueError("kind: one of %s" % sorted(S2S_KINDS))
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        if hasattr(emissions, "data_ptr"):  # a torch tensor
            dts = _torch_dtypes()
            assert emissions.dtype in dts, "emissions: float32 / float16 / bfloat16"
            e, dt = emissions, dts[emissions.dtype]
            shape, strides = tuple(e.shape), tuple(e.stride())
            ptr, on_dev = e.data_ptr(), 0 if e.device.type == "cpu" else 1
        else:
            if dtype is not None:
                if dtype not in ("bf16", "bfloat16") or getattr(emissions, "dtype", None) != np.uint16:
                    raise TypeError("dtype=%r: numpy emissions of bfloat16 bits are uint16 with dtype='bf16'" % (dtype,))
                dt = DTYPE_BF16
            elif getattr(emissions, "dtype", None) == np.float16:
                dt = DTYPE_F16
            elif kind == "log_probs":
                return None
            else:
                dt = DTYPE_F32
            e = np.asarray(emissions, dtype=_NP_DTYPES[dt])
            if e.ndim < 2 or e.strides[-1] != e.itemsize or any(st % e.itemsize for st in e.strides):
                e = np.ascontiguousarray(e).reshape(-1)  # (flat layout: frame after frame)
            shape, strides = e.shape, tuple(st // e.itemsize for st in e.strides)
            ptr, on_dev = e.ctypes.data, 1 if self._emu else 0
        stride = N
        if len(shape) > 1:
            assert shape[-1] == N and strides[-1] == 1 and len(shape) <= 3, \
                "emissions: [frames * N], [frames, N] or [B, T_max, N], unit column stride"
            if len(shape) == 3:  # one plane per utterance, any plane and frame strides
                assert shape[0] == len(T) and int(max(T, default=0)) <= shape[1] and off is None, \
                    "emissions [B, T_max, N]: one plane per utterance, no offsets"
                off = np.arange(len(T), dtype=np.int64) * strides[0]
            stride = strides[-2] if shape[-2] > 1 else N
        return e, dt, ptr, on_dev, off, stride

    def _frame_lse_ptr(self, lse_out, T):
        if lse_out is None:
            return None
        n = lse_out.size if isinstance(lse_out, np.ndarray) else lse_out.numel()
        assert n >= int(np.sum(T)) and str(lse_out.dtype).endswith("float64"), "lse_out: sum(T) float64 on the device"
        return self._addr(lse_out)

    def begin(self, emissions, T, N, offsets=None, device_ptr=None, *, kind="log_probs", dtype=None, lse_out=None):
        """emissions: a host float32 array (flat layout, copied by the call), or None when device_ptr (int) addresses
        float32 log-probs in HBM -- those must stay valid until end(); both go through fltx_ctc_rows_begin.  Or the
        acoustic model's output as it is (fltx_ctc_rows_begin_typed, no float32 copy is made): a torch tensor of
        float32, float16 or bfloat16 on the device or the host with unit column stride -- [B, T_max, N] with any plane
        and frame strides (utterance b reads its first T[b] frames), or [frames, N] / flat with `offsets` in elements --
        a numpy float16 array, or numpy uint16 holding bfloat16 bits with dtype="bf16" (flat layout).  kind "logits":
        the decoder takes each frame's log-softmax itself; lse_out (device float64, sum(T), utterance after utterance)
        then receives each frame's log-sum-exp.  A device tensor is kept referenced until the next begin().
        -> (token, src_row, state, n_rows): the roots."""
        T = np.ascontiguousarray(T, dtype=np.int32)
        self.B, self.N, self._T = len(T), int(N), T
        out = self._rows()
        ptrs = [self._addr(o) for o in out]
        typed = None if device_ptr is not None else self._frames_in(emissions, dtype, kind, offsets, T, self.N)
        if typed is not None:
            e, dt, ptr, on_dev, off, stride = typed
            self._chk(self.L.lib.fltx_ctc_rows_begin_typed(self.h, ptr, dt, S2S_KINDS[kind], on_dev, _ptr(off), stride,
                                                           _ptr(T), self.B, self.N, self._frame_lse_ptr(lse_out, T),
                                                           *ptrs))
            self._emissions = e
            return tuple(out)
        assert kind == "log_probs" and dtype is None, "device_ptr: float32 log-probs"
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        if device_ptr is not None:
            self._chk(self.L.lib.fltx_ctc_rows_begin(self.h, device_ptr, 1, _ptr(off), _ptr(T), self.B, self.N, *ptrs))
        else:
            e = np.ascontiguousarray(emissions, dtype=np.float32)
            self._chk(self.L.lib.fltx_ctc_rows_begin(self.h, _ptr(e), 0, _ptr(off), _ptr(T), self.B, self.N, *ptrs))
        return tuple(out)

    # ---- streams: chunks as they arrive, partial results, a bounded buffer (fltx_ctc_rows_stream_*) ----
    def stream_begin(self, B, N, max_frames):
        """decodeBegin for B parallel streams that hold up to max_frames frames each between prunes (the lexicon kind:
        100 more, which its prune may keep).  Every stream gets a table of max_states LM-state ids, cleared here: call
        set_max_states(n) first (the default of 65 536 is 1.5 MB per stream).  -> (token, src_row, state, n_rows): the roots.  Then append() a chunk,
        step() as often as append() says, prune() / best() as wanted, ..., end()."""
        self.B, self.N, self._T = int(B), int(N), np.zeros(int(B), np.int32)
        out = self._rows()
        self._chk(self.L.lib.fltx_ctc_rows_stream_begin(self.h, self.B, self.N, int(max_frames),
                                                        *[self._addr(o) for o in out]))
        self._stream_states = self._max_states
        return tuple(out)

    def append(self, emissions, T, offsets=None, device_ptr=None, *, kind="log_probs", dtype=None, lse_out=None):
        """The next chunk: T[b] >= 0 frames of stream b; emissions a host float32 array (flat layout, copied by the
        call), or None when device_ptr (int) addresses the chunk in HBM -- that must stay valid until the next append()
        or end().  Or a typed chunk in the forms begin() takes, with kind / dtype / lse_out as there
        (fltx_ctc_rows_stream_append_typed); every chunk names its own.  A device tensor is kept referenced until the
        next append().  -> the number of step() calls that consume the chunk (max T)."""
        T = np.ascontiguousarray(T, dtype=np.int32)
        assert len(T) == self.B, "T: one entry per stream"
        typed = None if device_ptr is not None else self._frames_in(emissions, dtype, kind, offsets, T, self.N)
        if typed is not None:
            e, dt, ptr, on_dev, off, stride = typed
            self._chk(self.L.lib.fltx_ctc_rows_stream_append_typed(self.h, ptr, dt, S2S_KINDS[kind], on_dev, _ptr(off),
                                                                   stride, _ptr(T), self._frame_lse_ptr(lse_out, T)))
            self._emissions = e
            self._T = T
            return int(T.max()) if len(T) else 0
        assert kind == "log_probs" and dtype is None, "device_ptr: float32 log-probs"
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        if device_ptr is not None:
            self._chk(self.L.lib.fltx_ctc_rows_stream_append(self.h, device_ptr, 1, _ptr(off), _ptr(T)))
        else:
            e = None if emissions is None else np.ascontiguousarray(emissions, dtype=np.float32)
            self._chk(self.L.lib.fltx_ctc_rows_stream_append(self.h, _ptr(e), 0, _ptr(off), _ptr(T)))
        self._T = T
        return int(T.max()) if len(T) else 0

    def prune(self, look_back=0):
        """prune(lookBack) of every stream, on the device"""
        self._chk(self.L.lib.fltx_ctc_rows_stream_prune(self.h, int(look_back)))

    def collect(self, release_cap=None):
        """Give back the state ids of every stream that no later step can meet again (fltx_ctc_rows_stream_collect):
        the ids that are neither in the current beam, nor below one of its states in the table, nor the parent id of
        one of its hypotheses.  -> (released [B, cap], n_released [B], n_live [B]) int32 -- torch tensors on the
        context's device, numpy arrays on the emulator library; nothing is copied to the host.  released[b] lists the
        stream's released ids ascending, -1 behind them, at most release_cap (default: the stream's max_states) per call; n_live
        the ids still allocated.  A released id may be handed out again for another state: drop the LM row kept for
        it.  A stopped stream releases nothing."""
        cap = self._stream_states if release_cap is None else int(release_cap)
        B = self.B
        if self._emu:
            out = [np.empty((B, max(cap, 0)), np.int32), np.empty(B, np.int32), np.empty(B, np.int32)]
        else:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            out = [torch.empty((B, max(cap, 0)), dtype=torch.int32, device=dev),
                   torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)]
        self._chk(self.L.lib.fltx_ctc_rows_stream_collect(self.h, cap, *[self._addr(o) for o in out]))
        return tuple(out)

    def frames_in_buffer(self, b):
        """nDecodedFramesInBuffer of stream b (synchronises)"""
        n = C.c_int32(0)
        self._chk(self.L.lib.fltx_ctc_rows_stream_frames_in_buffer(self.h, int(b), C.addressof(n)))
        return n.value

    # ---- the LM rows planned on the device (fltx_ctc_rows_plan_*) ----
    def plan_begin(self, row_capacity):
        """After begin() / stream_begin(): plan this decode's LM rows on the device, for a store of row_capacity rows."""
        self._chk(self.L.lib.fltx_ctc_rows_plan_begin(self.h, int(row_capacity)))

    def plan(self, tok, src, state, n):
        """The lists of the last begin() / step() -> a CtcRowsPlan: lm_row_of for the next step() / end(), and the
        states that are new in this list -- new_row (their rows of the store), new_parent_row (-1: a root), new_edge,
        new_dec_row -- the first counts[0] entries of each; counts = (n_new, high_water, n_free, n_dropped).  All [B*K]
        int32 ([4] for counts): torch tensors on the context's device, numpy arrays on the emulator library; nothing
        is copied to the host."""
        BK = self.B * int(self.options.beam_size)
        if self._emu:
            out = [np.empty(BK, np.int32) for _ in range(5)] + [np.empty(4, np.int32)]
        else:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            out = [torch.empty(BK, dtype=torch.int32, device=dev) for _ in range(5)] + \
                [torch.empty(4, dtype=torch.int32, device=dev)]
        self._chk(self.L.lib.fltx_ctc_rows_plan(self.h, *[self._addr(a) for a in (tok, src, state, n)],
                                                *[self._addr(o) for o in out]))
        return CtcRowsPlan(*out)

    def plan_release(self, released, n_released):
        """collect()'s `released` and `n_released`, unchanged, once per collect() and before the next plan(): the rows
        of the released ids are free again."""
        self._chk(self.L.lib.fltx_ctc_rows_plan_release(self.h, self._addr(released), self._addr(n_released),
                                                        int(released.shape[1])))

    def _planned(self, lists, lm_store, lm_new):
        """plan the lists and have lm_new fill the new rows -> (the plan, its counts on the host: 16 bytes)"""
        p = self.plan(*lists)
        counts = p.counts if self._emu else p.counts.cpu()  # (waits for the stream: the one read per frame)
        n_new = int(counts[0])
        if n_new:
            lm_new(p, n_new)
        return p, counts

    @staticmethod
    def _store_full(counts):
        if int(counts[3]) > 0:
            raise RuntimeError("LM row store full: %d states got no row (row_capacity = lm_store.shape[0] is too "
                               "small; a stream can collect_every)" % int(counts[3]))

    def decode_device(self, emissions, T, N, lm_store, lm_new, *, offsets=None, device_ptr=None, lm_kind="log_probs",
                      kind="log_probs", dtype=None, lse_out=None):
        """decode() without the host in the loop: lm_store is the caller's [row_capacity, >= lm_width] array of LM rows
        (a torch tensor on the context's device; numpy on the emulator library) and lm_new(p, n_new) writes its rows
        p.new_row[:n_new] -- row i the LM's scores after the state of row p.new_parent_row[i] (-1: the start) advanced
        by p.new_edge[i]; p.new_dec_row[i] // K is the utterance.  Per frame the host reads the plan's four counts and
        nothing else.  kind / dtype / lse_out: begin()'s.  RuntimeError "LM row store full" if a state got no row.
        Returns results_batch()."""
        lists = self.begin(emissions, T, N, offsets=offsets, device_ptr=device_ptr, kind=kind, dtype=dtype,
                           lse_out=lse_out)
        self.plan_begin(lm_store.shape[0])
        for _ in range(int(self._T.max()) if self.B else 0):
            p, _c = self._planned(lists, lm_store, lm_new)
            lists = self.step(lm_store, lm_row_of=p.lm_row_of, lm_kind=lm_kind)
        p, counts = self._planned(lists, lm_store, lm_new)
        self.end(lm_store, lm_row_of=p.lm_row_of, lm_kind=lm_kind)
        self._store_full(counts)
        return self.results_batch()

    def decode_stream_device(self, chunks, lm_store, lm_new, look_back=None, *, N=None, max_frames=None,
                             collect_every=None, lm_kind="log_probs", kind="log_probs", dtype=None):
        """decode_stream() on decode_device()'s terms: chunks, look_back, N, max_frames, collect_every, kind and dtype as there,
        lm_store and lm_new as in decode_device.  A collect's released ids go straight to plan_release() on the
        device: their rows of lm_store are handed out again.  Yields what decode_stream() yields."""
        N = self.N if N is None else int(N)
        chunks = iter(chunks)
        first = next(chunks, None)
        B = self.B if first is None else len(first[1])
        lists = self.stream_begin(B, N, 4096 if max_frames is None else max_frames)
        self.plan_begin(lm_store.shape[0])
        p, counts = self._planned(lists, lm_store, lm_new)
        chunk = first
        n_chunks = 0
        while chunk is not None:
            for _ in range(self.append(chunk[0], chunk[1], **self._chunk_kw(chunk, kind, dtype))):
                lists = self.step(lm_store, lm_row_of=p.lm_row_of, lm_kind=lm_kind)
                p, counts = self._planned(lists, lm_store, lm_new)
            if look_back is not None:
                self.prune(look_back)
            n_chunks += 1
            if collect_every is not None and n_chunks % int(collect_every) == 0:
                rel, n_rel, _ = self.collect(min(self._stream_states, 1024))
                self.plan_release(rel, n_rel)
            yield [self.best(b) for b in range(B)]
            chunk = next(chunks, None)
        self.end(lm_store, lm_row_of=p.lm_row_of, lm_kind=lm_kind)
        self._store_full(counts)
        yield self.results_batch()

    def _lm_in(self, lm_scores, lm_row_of, lm_kind, lm_lse_out, lm_dtype):
        """-> the C arguments of the LM rows (and what must stay alive while the kernels read them)"""
        if lm_kind not in S2S_KINDS:
            raise ValueError("lm_kind: one of %s" % sorted(S2S_KINDS))
        BK = self.B * int(self.options.beam_size)
        if lm_scores is None:  # (a step after the last frame reads no LM rows)
            return (None, DTYPE_F32, S2S_KINDS[lm_kind], 1 << 40, None, 0, 1, self._lse_ptr(lm_lse_out, BK)), ()
        if isinstance(lm_scores, np.ndarray):
            if lm_dtype is not None:
                if lm_dtype not in ("bf16", "bfloat16") or lm_scores.dtype != np.uint16:
                    raise TypeError("lm_dtype=%r: numpy rows of bfloat16 bits are uint16 with lm_dtype='bf16'" % (lm_dtype,))
                ldt = DTYPE_BF16
            else:
                ldt = DTYPE_F16 if lm_scores.dtype == np.float16 else DTYPE_F32
            lsc = np.ascontiguousarray(lm_scores, dtype=_NP_DTYPES[ldt]).reshape(-1, lm_scores.shape[-1])
            lstride, lptr, on_dev, host = lsc.shape[1], lsc.ctypes.data, 1 if self._emu else 0, True
        else:
            lsc, ldt, lstride, lptr, on_dev, host = Seq2SeqBatchDecoder._rows_in(self, lm_scores, lm_dtype, BK, "lm_scores")
        n_lm = int(lsc.shape[0])
        ro = None
        if lm_row_of is not None:
            if isinstance(lm_row_of, np.ndarray) or host:
                ro = np.ascontiguousarray(lm_row_of.cpu().numpy() if hasattr(lm_row_of, "cpu") else lm_row_of,
                                          dtype=np.int32).reshape(-1)
                n_ro = ro.size
            else:
                import torch
                ro = lm_row_of.reshape(-1).to(torch.int32).contiguous()
                n_ro = ro.numel()
            assert n_ro == BK, "lm_row_of: B*K entries"
        else:
            assert n_lm >= BK, "lm_scores: B*K rows without lm_row_of"
        return (lptr, ldt, S2S_KINDS[lm_kind], lstride, None if ro is None else self._addr(ro), n_lm, on_dev,
                self._lse_ptr(lm_lse_out, BK)), (lsc, ro)

    def step(self, lm_scores, *, lm_row_of=None, lm_kind="log_probs", lm_lse_out=None, lm_dtype=None):
        """One frame of every utterance that has frames left (fltx_ctc_rows_step).  lm_scores: a torch tensor of
        float32 / float16 / bfloat16 on the device or the host, or a numpy float32 / float16 array (uint16 holding
        bfloat16 bits with lm_dtype="bf16"); lm_row_of on the same side.  lm_kind "logits": the step takes each LM
        row's log-softmax itself; lm_lse_out (device float64, B*K) then receives each live row's log-sum-exp."""
        out = self._rows()
        args, keep = self._lm_in(lm_scores, lm_row_of, lm_kind, lm_lse_out, lm_dtype)
        self._chk(self.L.lib.fltx_ctc_rows_step(self.h, *args, *[self._addr(o) for o in out]))
        self._inputs = keep  # (kept until the next call: the kernels read them asynchronously)
        return tuple(out)

    def end(self, lm_scores, *, lm_row_of=None, lm_kind="log_probs", lm_lse_out=None, lm_dtype=None):
        """decodeEnd and the back-trace: the LM rows of the rows the last step listed, as step() takes them."""
        args, keep = self._lm_in(lm_scores, lm_row_of, lm_kind, lm_lse_out, lm_dtype)
        self._chk(self.L.lib.fltx_ctc_rows_end(self.h, *args))
        self._inputs = keep

    def stream_finish(self, which, lm_scores, *, lm_row_of=None, lm_kind="log_probs", lm_dtype=None, lm_lse_out=None,
                      device=False):
        """End the utterances of the streams `which` names (B flags) and restart those slots from the root, leaving every
        other stream as it is (fltx_ctc_rows_stream_finish).  lm_scores / lm_row_of / lm_kind / lm_dtype / lm_lse_out as
        end() takes them, for the rows the last call listed; only the named streams' rows are read, and lm_scores may
        be None when no stream is named.  -> ((token, src_row, state, n_rows), finished): the lists name the root of a
        named stream and every other beam again, unchanged.  finished, device=False: a dict with n_hyp, length, status
        ([B] int32 copies; status 0 or the error code count(b) would raise with after end()) and hyps = {b: the list of
        Hyp that results(b) gives after end()} for the named streams.  device=True: nothing is copied; the dict holds
        the integer device addresses n_hyp, length, status, scores, tokens, words (None: lexicon-free), row_off --
        tokens / words / row_off / length are what Context.collapse_rows(device=True) takes.  Both stay valid until
        the next stream_finish(), end() or begin."""
        w = np.ascontiguousarray(np.asarray(which) != 0, dtype=np.int32)
        assert w.size == self.B, "which: one flag per stream"
        out = self._rows()
        args, keep = self._lm_in(lm_scores, lm_row_of, lm_kind, lm_lse_out, lm_dtype)
        fo = FinishedOut()
        self._chk(self.L.lib.fltx_ctc_rows_stream_finish(self.h, _ptr(w), *args, *[self._addr(o) for o in out],
                                                         1 if device else 0, C.byref(fo)))
        self._inputs = keep
        if device:
            return tuple(out), {f: getattr(fo, f) for f, _ in FinishedOut._fields_}
        return tuple(out), _finished_host(fo, w, self.B, int(self.options.beam_size))

    @staticmethod
    def _chunk_kw(chunk, kind, dtype):
        """append()'s keywords for a chunk: the stream's, or those the chunk's own third element names"""
        return dict({"kind": kind, "dtype": dtype}, **(chunk[2] if len(chunk) > 2 else {}))

    def decode(self, emissions, T, N, lm_rows, *, offsets=None, device_ptr=None, lm_kind="log_probs", kind="log_probs",
               dtype=None, lse_out=None):
        """The whole batch from a callable: lm_rows(state_keys) -> rows, where state_keys is a list of (b, prefix) --
        utterance and the tuple of tokens the state stands for -- one per LM state the search has just entered, and
        rows is [len(state_keys), >= lm_width] (a torch tensor on the context's device; numpy on the emulator library),
        row i the LM's scores after state_keys[i].  One row is kept per state id and shared through lm_row_of, so the
        LM runs once per state, however many hypotheses and frames are in it.  kind / dtype / lse_out: begin()'s -- the
        acoustic model's fp16 / bf16 output or raw logits go in as they are.  Returns results_batch().  (The rows are
        read on the host once per frame to name the new states.)"""
        tok, src, state, n = self.begin(emissions, T, N, offsets=offsets, device_ptr=device_ptr, kind=kind, dtype=dtype,
                                        lse_out=lse_out)
        lister = _RowLister(self, self.B, int(self.options.beam_size), lm_rows)
        for _ in range(int(self._T.max()) if self.B else 0):
            rows, ro = lister.rows(tok, src, state, n)
            tok, src, state, n = self.step(rows, lm_row_of=ro, lm_kind=lm_kind)
        rows, ro = lister.rows(tok, src, state, n)
        self.end(rows, lm_row_of=ro, lm_kind=lm_kind)
        return self.results_batch()

    def decode_stream(self, chunks, lm_rows, look_back=None, *, N=None, max_frames=None, lm_kind="log_probs",
                      collect_every=None, on_release=None, kind="log_probs", dtype=None):
        """B streams from an iterable of chunks, each (emissions, T): a host float32 array in flat layout and the B
        frame counts (0 allowed) -- or emissions in any form append() takes, with kind / dtype for all chunks, or
        (emissions, T, {"kind": ..., "dtype": ...}) for a chunk that names its own.  lm_rows is decode()'s callable.  A generator: after every chunk it yields the list
        of best(b) per stream -- after prune(look_back) when look_back is given -- and, when the chunks are used up,
        ends the streams and yields results_batch().  N: the token-set size (default: that of the last begin);
        max_frames: the frames a stream holds between prunes (default: 4096).
        collect_every=n: after every n-th chunk (after the prune) collect() gives the dead state ids back, the LM rows
        kept for them are dropped and their places reused, and on_release(b, ids) -- ids a list, ascending -- tells an
        LM that caches per state_id to drop its states; a stream then runs in max_states ids and a bounded row store
        however long it is.  (The `prefix` handed to lm_rows still grows with the stream.)  None: no collect, ids are
        handed out once, as without the argument."""
        N = self.N if N is None else int(N)
        chunks = iter(chunks)
        first = next(chunks, None)
        B = self.B if first is None else len(first[1])
        tok, src, state, n = self.stream_begin(B, N, 4096 if max_frames is None else max_frames)
        K = int(self.options.beam_size)
        lister = _RowLister(self, B, K, lm_rows)
        args = lister.rows(tok, src, state, n)
        chunk = first
        n_chunks = 0
        while chunk is not None:
            for _ in range(self.append(chunk[0], chunk[1], **self._chunk_kw(chunk, kind, dtype))):
                tok, src, state, n = self.step(args[0], lm_row_of=args[1], lm_kind=lm_kind)
                args = lister.rows(tok, src, state, n)
            if look_back is not None:
                self.prune(look_back)
            n_chunks += 1
            if collect_every is not None and n_chunks % int(collect_every) == 0:
                # (a modest cap: the list is cleared on the device whatever it holds; what does not fit goes at the next
                # collect.  The counts come to the host first, then only the part of the list that is filled.)
                rel, n_rel, _ = self.collect(min(self._stream_states, 1024))
                if not self._emu:
                    self.ctx.synchronize()
                    n_rel = n_rel.cpu().numpy()
                    rel = rel[:, :max(int(n_rel.max()), 1)].cpu().numpy()
                for b in range(B):
                    if n_rel[b]:
                        ids = [int(i) for i in rel[b, :int(n_rel[b])]]
                        lister.release(b, ids)
                        if on_release is not None:
                            on_release(b, ids)
            yield [self.best(b) for b in range(B)]
            chunk = next(chunks, None)
        self.end(args[0], lm_row_of=args[1], lm_kind=lm_kind)
        yield self.results_batch()


class CtcRowsPlan:
    """What CtcRowsBatchDecoder.plan() returns (fltx_ctc_rows_plan's outputs)"""
    __slots__ = ("lm_row_of", "new_row", "new_parent_row", "new_edge", "new_dec_row", "counts")

    def __init__(self, lm_row_of, new_row, new_parent_row, new_edge, new_dec_row, counts):
        self.lm_row_of, self.new_row, self.new_parent_row = lm_row_of, new_row, new_parent_row
        self.new_edge, self.new_dec_row, self.counts = new_edge, new_dec_row, counts


class _RowLister:
    """The bookkeeping of decode() and decode_stream(): one LM row per state id, the LM asked once per id (once per
    time the id is handed out, when release() gives ids back).  `prefix` -- what lm_rows is handed -- is the tuple of
    edges since the start of the stream and grows with it; the rows kept do not."""

    def __init__(self, dec, B, K, lm_rows):
        self.dec, self.B, self.K, self.lm_rows = dec, B, K, lm_rows
        self.row_of, self.prefix = {}, {}
        self.store, self.n_store, self.prev_state = None, 0, None
        self.free = []  # rows of the store whose state ids were released

    def release(self, b, ids):
        """stream b's state ids `ids` were released (collect()): forget them, their rows of the store are free"""
        for i in ids:
            key = (b, int(i))
            self.free.append(self.row_of.pop(key))
            del self.prefix[key]

    def rows(self, tok, src, state, n):
        """the row lists of a call -> (lm_scores, lm_row_of) for the next"""
        dec, B, K = self.dec, self.B, self.K
        if not dec._emu:
            dec.ctx.synchronize()
        tok_h, src_h, st_h, n_h = [a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in (tok, src, state, n)]
        keys, slots = [], []
        ro = np.full(B * K, -1, np.int32)
        for b in range(B):
            for k in range(int(n_h[b])):
                key = (b, int(st_h[b, k]))
                if key not in self.row_of:
                    s = int(src_h[b, k])
                    par = -1 if s < 0 else int(self.prev_state.reshape(-1)[s])
                    self.prefix[key] = () if s < 0 else self.prefix[(b, par)] + (int(tok_h[b, k]),)
                    if self.free:
                        slots.append(self.free.pop())
                    else:
                        slots.append(self.n_store)
                        self.n_store += 1
                    self.row_of[key] = slots[-1]
                    keys.append(dec._state_key(b, self.prefix[key], par, int(tok_h[b, k]) if s >= 0 else -1, key[1]))
                ro[b * K + k] = self.row_of[key]
        if keys:
            rows = self.lm_rows(keys)
            need = self.n_store
            if self.store is None or need > self.store.shape[0]:
                cap = max(need, 2 * (0 if self.store is None else self.store.shape[0]), B * K)
                if isinstance(rows, np.ndarray):
                    grown = np.empty((cap, rows.shape[1]), rows.dtype)
                else:
                    grown = rows.new_empty((cap, rows.shape[1]))
                if self.store is not None:
                    grown[:self.store.shape[0]] = self.store
                self.store = grown
            if slots == list(range(slots[0], slots[0] + len(slots))):
                self.store[slots[0]:slots[0] + len(slots)] = rows
            elif isinstance(self.store, np.ndarray):
                self.store[np.asarray(slots)] = rows
            else:
                self.store[_to_device_i32(np.asarray(slots, np.int64), self.store.device)] = rows
        self.prev_state = st_h.copy()
        ro_in = ro if isinstance(self.store, np.ndarray) else _to_device_i32(ro, self.store.device)
        return self.store[:self.n_store], ro_in


class LexiconCtcRowsBatchDecoder(CtcRowsBatchDecoder):
    """fltx_ctc_rows_lex_decoder_create: LexiconDecoder (CTC) for B utterances at once with a neural LM in shallow
    fusion, stepped by CtcRowsBatchDecoder's begin / step / end / set_max_states and row contract.  `host_trie` is a
    HostTrie (already smeared); `lm` a WordRowsLM (is_lm_token=False: an LM over the lexicon's words) or a RowsLM
    (is_lm_token=True: an LM over the tokens), either with a finish_index >= 0; `options` are make_options(...)'s with
    the CTC criterion, word_score and unk_score included (unk_score > -inf needs `unk`).  The `token` a row lists is the
    LM EDGE that made its state from the state of row src_row: the word that ended in this frame (word LM), the token
    (token LM), -1 where the state is the parent's (and for the root).  The results carry words.

    decode(emissions, T, N, lm_rows, ...): lm_rows(state_keys) gets one (b, prefix, parent_id, edge, state_id) per LM
    state the search has just entered -- prefix the tuple of edges (words or tokens) since the start, parent_id the
    next_state id of the state it was made from (-1: LM::start) and edge what advanced it -- so an LM that caches its
    hidden state per id advances parent_id's by edge; it is asked once per state id."""

    def __init__(self, ctx, options, host_trie, lm, sil, blank, unk=-1, is_lm_token=False):
        self._init(ctx, LEX_CTC_ROWS, options, lm, host_trie, sil, blank)
        self.unk, self.is_lm_token = int(unk), bool(is_lm_token)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_ctc_rows_lex_decoder_create(ctx.h, C.byref(options), host_trie.h, lm.h, int(sil),
                                                                 int(blank), int(unk), int(bool(is_lm_token)),
                                                                 C.byref(h)))
        self._made(h)

    @staticmethod
    def _state_key(b, prefix, parent_id, edge, state_id):
        return (b, prefix, parent_id, edge, state_id)


def _to_device_i32(a, device):
    import torch
    return torch.from_numpy(a).to(device)


class DecoderGroup:
    """fltx_group: one batch sharded over several devices (one context, decoder
    and host thread per entry of `devices`; no inter-device traffic)."""

    def __init__(self, devices, kind, options, lm, sil, blank, unk=-1, host_trie=None, transitions=None,
                 is_lm_token=False, lib=None):
        self.L = lib or lm.L
        self.options = options
        self._keep = (lm, host_trie)
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        tr = None if transitions is None or len(transitions) == 0 else \
            np.ascontiguousarray(transitions, dtype=np.float32)
        h = C.c_void_p()
        self.L.check(self.L.lib.fltx_group_create(
            _ptr(dv), len(dv), kind, C.byref(options), host_trie.h if host_trie is not None else None, lm.h,
            sil, blank, unk, _ptr(tr), 0 if tr is None else tr.size, int(is_lm_token), C.byref(h)))
        self.h = h
        self.n = len(dv)
        self.B = 0

    def decode_batch(self, emissions, T, N, offsets=None, device_ptrs=None):
        """emissions: one host float32 array for the whole batch, or device_ptrs =
        one HBM address per device (the part's shard, addressed by `offsets`)."""
        T = np.ascontiguousarray(T, dtype=np.int32)
        B = len(T)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        ptrs = (C.c_void_p * self.n)()
        ond = np.zeros(self.n, dtype=np.int32)
        if device_ptrs is not None:
            for i, p in enumerate(device_ptrs):
                ptrs[i] = p
            ond[:] = 1
        else:
            self._e = np.ascontiguousarray(emissions, dtype=np.float32)
            for i in range(self.n):
                ptrs[i] = self._e.ctypes.data
        self.L.check(self.L.lib.fltx_group_decode_batch(self.h, ptrs, _ptr(ond), _ptr(off), _ptr(T), B, N))
        self.B = B

    def parts(self):
        """[(BatchDecoder-like handle, first, count)] of the last batch."""
        out = []
        for i in range(self.n):
            d, f, c = C.c_void_p(), C.c_int32(0), C.c_int32(0)
            self.L.check(self.L.lib.fltx_group_decoder(self.h, i, C.byref(d), C.addressof(f), C.addressof(c)))
            out.append((d, f.value, c.value))
        return out

    def results(self, b, max_hyp=None):
        n, ln = C.c_int32(0), C.c_int32(0)
        self.L.check(self.L.lib.fltx_group_result_count(self.h, b, C.addressof(n), C.addressof(ln)))
        n, ln = n.value, ln.value
        if max_hyp is not None:
            n = min(n, max_hyp)
        if n == 0:
            return []
        scores = np.zeros(3 * n, dtype=np.float64)
        tokens = np.zeros((n, ln), dtype=np.int32)
        words = np.zeros((n, ln), dtype=np.int32)
        got = C.c_int32(0)
        self.L.check(self.L.lib.fltx_group_result_fetch(self.h, b, n, _ptr(scores), _ptr(tokens), _ptr(words),
                                                        C.addressof(got)))
        return [Hyp(scores[3 * i], scores[3 * i + 1], scores[3 * i + 2], tokens[i].copy(), words[i].copy())
                for i in range(n)]

    def synchronize(self):
        self.L.check(self.L.lib.fltx_group_synchronize(self.h))

    def close(self):
        if self.h:
            self.L.lib.fltx_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_s2s_options(beam_size, beam_size_token, beam_threshold=25.0, lm_weight=0.0, eos_score=0.0, log_add=False):
    return S2sOptions(beam_size, beam_size_token, beam_threshold, lm_weight, eos_score, int(bool(log_add)))


def make_s2s_lex_options(beam_size, beam_size_token, beam_threshold=25.0, lm_weight=0.0, word_score=0.0,
                        eos_score=0.0, log_add=False):
    return S2sLexOptions(beam_size, beam_size_token, beam_threshold, lm_weight, word_score, eos_score,
                         int(bool(log_add)))


def make_options(beam_size, beam_size_token, beam_threshold=25.0, lm_weight=0.0, word_score=0.0,
                 unk_score=-float("inf"), sil_score=0.0, log_add=False, criterion="ctc"):
    crit = CRITERION[criterion] if isinstance(criterion, str) else int(criterion)
    return Options(beam_size, beam_size_token, beam_threshold, lm_weight, word_score, unk_score, sil_score,
                   int(bool(log_add)), crit)
