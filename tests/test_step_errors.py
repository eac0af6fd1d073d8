"""What the step decoders' entry checks say (seq2seq: fltx_s2s_*; the CTC rows kinds: fltx_ctc_rows_*, their streams and
finish calls): the code and the text of fltx_last_error for calls with exactly ONE thing wrong, through the C ABI handles
of _capi.Lib (the Python wrappers reject some of these inputs themselves).

The host layer writes each of these decisions once ("the step decoders' host layer"); this file pins what a
caller sees of them, so that the checks can be moved without changing it.  The expected texts are literal.  Emulator
only; nothing beyond a begin is launched, except by fltx_ctc_rows_stream_finish, whose LM rows are looked at behind its
mask kernel.

Shapes: B = 2, K = 2, V = N = 5, T = 2, a RowsLM / WordRowsLM of width 5 and a ZeroLM.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi  # noqa: E402

B, K, V, T, W = 2, 2, 5, 2, 5
INVALID, STATE = _capi.ERR_INVALID, _capi.ERR_STATE
NOT_S2S = "%s: not a seq2seq decoder (fltx_s2s_decoder_create)"
NOT_CR = "%s: not a CTC rows decoder (fltx_ctc_rows_decoder_create, fltx_ctc_rows_lex_decoder_create)"
NO_STREAM = "%s: no open stream (fltx_ctc_rows_stream_begin first)"


def p(a):
    return None if a is None else a.ctypes.data


class Env:
    """The decoders of the cases and valid arguments for every call; the emulator's device memory is host memory"""

    def __init__(self, sess):
        self.L, self.f = sess.lib, sess.lib.lib
        ctx = sess.ctx
        self.rows = _capi.RowsLM(W, None, W - 1, lib=self.L)
        self.wrows = _capi.WordRowsLM(W, None, W - 1, lib=self.L)
        self.trie = _capi.HostTrie(V, 0, lib=self.L)
        self.trie.insert([1, 2], 0, 0.0)
        self.trie.insert([3], 1, 0.0)
        self.trie.smear(1)
        so = _capi.make_s2s_options(K, K)
        self.tok, self.beam, self.src, self.state, self.word = (np.zeros((B, K), np.int32) for _ in range(5))
        self.n = np.zeros(B, np.int32)
        self.scores = np.zeros((B * K, V), np.float32)
        self.lm_scores = np.zeros((B * K, W), np.float32)
        self.row_of = np.zeros(B * K, np.int32)
        self.em = np.zeros((B * T, V), np.float32)
        self.Ts = np.full(B, T, np.int32)
        self.which = np.array([1, 0], np.int32)
        self.released, self.n_rel = np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
        self.fin, self.s2s_fin = _capi.FinishedOut(), _capi.S2sFinishedOut()
        # seq2seq: ZeroLM, a rows LM, a word-level rows LM (lexicon kind); one of each begun, one ZeroLM decoder not
        self.s2z_fresh = _capi.Seq2SeqBatchDecoder(ctx, so, sess.zero, V - 1, 3)
        self.s2z = _capi.Seq2SeqBatchDecoder(ctx, so, sess.zero, V - 1, 3)
        self.s2r = _capi.Seq2SeqBatchDecoder(ctx, so, self.rows, V - 1, 3)
        self.s2w = _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(K, K), self.trie, self.wrows, V - 1, 3)
        for d in (self.s2z, self.s2r, self.s2w):
            self.ok(self.f.fltx_s2s_begin(d.h, B, V, *self.s2s_lists()))
        # CTC rows: not begun (two of them), begun as a batch, begun as streams
        co = _capi.make_options(K, K)
        self.cr_fresh, self.cr_typed, self.cr_batch, self.cr_stream = (
            _capi.CtcRowsBatchDecoder(ctx, co, self.rows, 0, 1) for _ in range(4))
        self.ok(self.f.fltx_ctc_rows_begin(self.cr_batch.h, p(self.em), 1, None, p(self.Ts), B, V, *self.cr_lists()))
        self.ok(self.f.fltx_ctc_rows_stream_begin(self.cr_stream.h, B, V, 8, *self.cr_lists()))

    def ok(self, rc):
        assert rc == 0, self.f.fltx_last_error().decode()

    def s2s_lists(self, **kw):
        a = dict(tok=p(self.tok), beam=p(self.beam), src=p(self.src), n=p(self.n))
        a.update(kw)
        return a["tok"], a["beam"], a["src"], a["n"]

    def cr_lists(self, **kw):
        a = dict(tok=p(self.tok), src=p(self.src), state=p(self.state), n=p(self.n))
        a.update(kw)
        return a["tok"], a["src"], a["state"], a["n"]

    # ---- the calls, valid unless a keyword says otherwise --------------------------------------------------------------
    def s2s_step(self, d, **kw):
        a = dict(stride=V)
        a.update(kw)
        lists = self.s2s_lists(**{k: a.pop(k) for k in ("tok", "beam", "src", "n") if k in a})
        return self.f.fltx_s2s_step(d.h, p(self.scores), 1, a["stride"], None, *lists)

    def s2s_step_typed(self, d, dtype=0, kind=0):
        return self.f.fltx_s2s_step_typed(d.h, p(self.scores), dtype, kind, 1, V, None, None, *self.s2s_lists())

    def s2s_step_lm_rows(self, d, dtype=0, kind=0, lm_dtype=0, lm_kind=0, lm_stride=W):
        return self.f.fltx_s2s_step_lm_rows(d.h, p(self.scores), dtype, kind, V, p(self.lm_scores), lm_dtype, lm_kind,
                                            lm_stride, 1, None, None, None, *self.s2s_lists())

    def s2s_step_word_lm_rows(self, d, dtype=0, kind=0, lm_dtype=0, lm_kind=0, lm_stride=W, row_of=None, n_lm_rows=0,
                              word=True):
        tok, beam, src, n = self.s2s_lists()
        return self.f.fltx_s2s_step_word_lm_rows(d.h, p(self.scores), dtype, kind, V, p(self.lm_scores), lm_dtype,
                                                 lm_kind, lm_stride, p(row_of), n_lm_rows, 1, None, None, None, tok,
                                                 beam, src, p(self.word) if word else None, n)

    def s2s_finish(self, d, word=False, **kw):
        return self.f.fltx_s2s_finish(d.h, p(self.which), *self.s2s_lists(**kw), p(self.word) if word else None, 1,
                                      C.byref(self.s2s_fin))

    def cr_begin_typed(self, d, dtype=0, kind=0, stride=V):
        return self.f.fltx_ctc_rows_begin_typed(d.h, p(self.em), dtype, kind, 1, None, stride, p(self.Ts), B, V, None,
                                                *self.cr_lists())

    def crs_append_typed(self, d, dtype=0, kind=0, stride=V):
        return self.f.fltx_ctc_rows_stream_append_typed(d.h, p(self.em), dtype, kind, 1, None, stride, p(self.Ts), None)

    def cr_step(self, d, lm_dtype=0, lm_kind=0, lm_stride=W, row_of=None, n_lm_rows=0, **kw):
        return self.f.fltx_ctc_rows_step(d.h, p(self.lm_scores), lm_dtype, lm_kind, lm_stride, p(row_of), n_lm_rows, 1,
                                         None, *self.cr_lists(**kw))

    def cr_end(self, d, lm_dtype=0, lm_kind=0, lm_stride=W):
        return self.f.fltx_ctc_rows_end(d.h, p(self.lm_scores), lm_dtype, lm_kind, lm_stride, None, 0, 1, None)

    def crs_finish(self, d, lm_dtype=0, lm_kind=0, lm_stride=W, out=True, **kw):
        return self.f.fltx_ctc_rows_stream_finish(d.h, p(self.which), p(self.lm_scores), lm_dtype, lm_kind, lm_stride,
                                                  None, 0, 1, None, *self.cr_lists(**kw), 1,
                                                  C.byref(self.fin) if out else None)

    def crs_collect(self, d):
        return self.f.fltx_ctc_rows_stream_collect(d.h, 4, p(self.released), p(self.n_rel), None)


@pytest.fixture(scope="module")
def env(emu_session):
    return Env(emu_session)


def says(env, rc, code, text):
    """the way Lib.check reads a failed call: its code, and the thread's last error"""
    msg = env.f.fltx_last_error().decode()
    print("rc = %d: %s" % (rc, msg))
    assert (rc, msg) == (code, text)


class _Null:
    h = None


NULL = _Null()


# ---- a null decoder, a decoder of the other family: one call of each check function ----------------------------------------
def test_null_decoder(env):
    says(env, env.f.fltx_s2s_end(None), INVALID, "fltx_s2s_end: null decoder")
    says(env, env.f.fltx_ctc_rows_plan_begin(None, 1), INVALID, "fltx_ctc_rows_plan_begin: null decoder")
    says(env, env.f.fltx_ctc_rows_stream_prune(None, 0), INVALID, "fltx_ctc_rows_stream_prune: null decoder")
    # (and the entry points that name themselves through a helper)
    says(env, env.s2s_step(NULL), INVALID, "fltx_s2s_step: null decoder")
    says(env, env.cr_begin_typed(NULL), INVALID, "fltx_ctc_rows_begin_typed: null decoder")
    says(env, env.crs_append_typed(NULL), INVALID, "fltx_ctc_rows_stream_append_typed: null decoder")
    says(env, env.crs_finish(NULL), INVALID, "fltx_ctc_rows_stream_finish: null decoder")
    says(env, env.s2s_finish(NULL), INVALID, "fltx_s2s_finish: null decoder")


def test_wrong_family(env):
    says(env, env.f.fltx_s2s_end(env.cr_batch.h), STATE, NOT_S2S % "fltx_s2s_end")
    says(env, env.s2s_step(env.cr_batch), STATE, NOT_S2S % "fltx_s2s_step")
    says(env, env.s2s_finish(env.cr_stream), STATE, NOT_S2S % "fltx_s2s_finish")
    says(env, env.f.fltx_ctc_rows_plan_begin(env.s2z.h, 1), STATE, NOT_CR % "fltx_ctc_rows_plan_begin")
    says(env, env.cr_step(env.s2z), STATE, NOT_CR % "fltx_ctc_rows_step")
    says(env, env.cr_end(env.s2r), STATE, NOT_CR % "fltx_ctc_rows_end")
    says(env, env.f.fltx_ctc_rows_stream_prune(env.s2z.h, 0), STATE, NOT_CR % "fltx_ctc_rows_stream_prune")
    says(env, env.crs_finish(env.s2z), STATE, NOT_CR % "fltx_ctc_rows_stream_finish")


# ---- the order of the calls ----------------------------------------------------------------------------------------------------
def test_before_begin(env):
    says(env, env.s2s_step(env.s2z_fresh), STATE, "fltx_s2s_step: fltx_s2s_begin first")
    says(env, env.f.fltx_s2s_end(env.s2z_fresh.h), STATE, "fltx_s2s_end: fltx_s2s_begin first")
    says(env, env.s2s_finish(env.s2z_fresh), STATE, "fltx_s2s_finish: between fltx_s2s_begin and fltx_s2s_end")
    says(env, env.cr_step(env.cr_fresh), STATE, "fltx_ctc_rows_step: fltx_ctc_rows_begin first")
    says(env, env.cr_end(env.cr_fresh), STATE, "fltx_ctc_rows_end: fltx_ctc_rows_begin first")
    says(env, env.crs_finish(env.cr_fresh), STATE, NO_STREAM % "fltx_ctc_rows_stream_finish")


def test_stream_call_on_a_batch(env):
    d = env.cr_batch
    says(env, env.f.fltx_ctc_rows_stream_append(d.h, p(env.em), 1, None, p(env.Ts)), STATE,
         NO_STREAM % "fltx_ctc_rows_stream_append")
    says(env, env.crs_append_typed(d), STATE, NO_STREAM % "fltx_ctc_rows_stream_append_typed")
    says(env, env.f.fltx_ctc_rows_stream_prune(d.h, 0), STATE, NO_STREAM % "fltx_ctc_rows_stream_prune")
    says(env, env.crs_collect(d), STATE, NO_STREAM % "fltx_ctc_rows_stream_collect")
    says(env, env.crs_finish(d), STATE, NO_STREAM % "fltx_ctc_rows_stream_finish")


# ---- a dtype of 7 and a kind of 7, for each argument that carries one ----------------------------------------------------------
def test_dtype_and_kind_seq2seq(env):
    says(env, env.s2s_step_typed(env.s2z, dtype=7), INVALID, "fltx_s2s_step_typed: dtype 7")
    says(env, env.s2s_step_typed(env.s2z, kind=7), INVALID, "fltx_s2s_step_typed: kind 7")
    for name, call, d in (("fltx_s2s_step_lm_rows", env.s2s_step_lm_rows, env.s2r),
                          ("fltx_s2s_step_word_lm_rows", env.s2s_step_word_lm_rows, env.s2w)):
        says(env, call(d, dtype=7), INVALID, "%s: dtype 7, lm_dtype 0" % name)
        says(env, call(d, lm_dtype=7), INVALID, "%s: dtype 0, lm_dtype 7" % name)
        says(env, call(d, kind=7), INVALID, "%s: kind 7, lm_kind 0" % name)
        says(env, call(d, lm_kind=7), INVALID, "%s: kind 0, lm_kind 7" % name)
        says(env, call(d, dtype=-1), INVALID, "%s: dtype -1, lm_dtype 0" % name)
        says(env, call(d, lm_dtype=3), INVALID, "%s: dtype 0, lm_dtype 3" % name)
        says(env, call(d, lm_kind=2), INVALID, "%s: kind 0, lm_kind 2" % name)


def test_dtype_and_kind_ctc_rows(env):
    for name, call, d in (("fltx_ctc_rows_begin_typed", env.cr_begin_typed, env.cr_typed),
                          ("fltx_ctc_rows_stream_append_typed", env.crs_append_typed, env.cr_stream)):
        says(env, call(d, dtype=7), INVALID, "%s: dtype 7" % name)
        says(env, call(d, kind=7), INVALID, "%s: kind 7" % name)
        says(env, call(d, dtype=3), INVALID, "%s: dtype 3" % name)
        says(env, call(d, kind=-1), INVALID, "%s: kind -1" % name)
        # -1 is the host's own mark of the plain float32 entry points, and no dtype of the ABI
        says(env, call(d, dtype=-1), INVALID, "%s: dtype -2" % name)
    for name, call, d in (("fltx_ctc_rows_step", env.cr_step, env.cr_batch), ("fltx_ctc_rows_end", env.cr_end, env.cr_batch),
                          ("fltx_ctc_rows_stream_finish", env.crs_finish, env.cr_stream)):
        says(env, call(d, lm_dtype=7), INVALID, "%s: lm_dtype 7" % name)
        says(env, call(d, lm_kind=7), INVALID, "%s: lm_kind 7" % name)
        says(env, call(d, lm_dtype=-1), INVALID, "%s: lm_dtype -1" % name)


# ---- strides, row maps, output lists -------------------------------------------------------------------------------------------
def test_lm_row_stride_below_the_width(env):
    says(env, env.s2s_step_lm_rows(env.s2r, lm_stride=W - 1), INVALID,
         "fltx_s2s_step_lm_rows: bad argument (lm_row_stride 4, lm_width = 5)")
    says(env, env.s2s_step_word_lm_rows(env.s2w, lm_stride=W - 1), INVALID,
         "fltx_s2s_step_word_lm_rows: bad argument (lm_row_stride 4, lm_width = 5)")
    for name, call, d in (("fltx_ctc_rows_step", env.cr_step, env.cr_batch), ("fltx_ctc_rows_end", env.cr_end, env.cr_batch),
                          ("fltx_ctc_rows_stream_finish", env.crs_finish, env.cr_stream)):
        says(env, call(d, lm_stride=W - 1), INVALID,
             "%s: bad argument (lm_row_stride 4, lm_width = 5, n_lm_rows 0)" % name)


def test_row_stride_and_frame_stride_below_the_width(env):
    says(env, env.s2s_step(env.s2z, stride=V - 1), INVALID, "fltx_s2s_step: bad argument (row_stride 4, V = 5)")
    says(env, env.cr_begin_typed(env.cr_typed, stride=V - 1), INVALID, "fltx_ctc_rows_begin_typed: frame_stride 4 < N = 5")
    says(env, env.crs_append_typed(env.cr_stream, stride=V - 1), INVALID,
         "fltx_ctc_rows_stream_append_typed: frame_stride 4 < N = 5")


def test_lm_row_of_without_rows(env):
    says(env, env.cr_step(env.cr_batch, row_of=env.row_of, n_lm_rows=0), INVALID,
         "fltx_ctc_rows_step: bad argument (lm_row_stride 5, lm_width = 5, n_lm_rows 0)")
    says(env, env.s2s_step_word_lm_rows(env.s2w, row_of=env.row_of, n_lm_rows=0), INVALID,
         "fltx_s2s_step_word_lm_rows: bad argument (next_word is required; n_lm_rows 0 with lm_row_of)")


def test_null_output_lists(env):
    f = env.f
    for k in ("tok", "beam", "src", "n"):
        says(env, f.fltx_s2s_begin(env.s2z_fresh.h, B, V, *env.s2s_lists(**{k: None})), INVALID,
             "fltx_s2s_begin: bad argument")
        says(env, env.s2s_step(env.s2z, **{k: None}), INVALID, "fltx_s2s_step: bad argument (row_stride 5, V = 5)")
        says(env, env.s2s_finish(env.s2z, **{k: None}), INVALID, "fltx_s2s_finish: null which, list or out")
    for k in ("tok", "src", "state", "n"):
        says(env, f.fltx_ctc_rows_begin(env.cr_fresh.h, p(env.em), 1, None, p(env.Ts), B, V, *env.cr_lists(**{k: None})),
             INVALID, "fltx_ctc_rows_begin: bad argument")
        says(env, f.fltx_ctc_rows_stream_begin(env.cr_fresh.h, B, V, 8, *env.cr_lists(**{k: None})), INVALID,
             "fltx_ctc_rows_stream_begin: bad argument")
        says(env, env.cr_step(env.cr_batch, **{k: None}), INVALID, "fltx_ctc_rows_step: null output")
        says(env, env.crs_finish(env.cr_stream, **{k: None}), INVALID,
             "fltx_ctc_rows_stream_finish: null which, list or out")
    says(env, env.crs_finish(env.cr_stream, out=False), INVALID, "fltx_ctc_rows_stream_finish: null which, list or out")
    says(env, env.s2s_step_word_lm_rows(env.s2w, word=False), INVALID,
         "fltx_s2s_step_word_lm_rows: bad argument (next_word is required; n_lm_rows 0 with lm_row_of)")
    says(env, env.s2s_finish(env.s2w, word=False), INVALID,
         "fltx_s2s_finish: a decoder with a word-level rows LM lists next_word")


def test_the_step_call_of_the_decoders_lm(env):
    """(the LM level is a check the three seq2seq steps share too)"""
    says(env, env.s2s_step(env.s2r), STATE, "fltx_s2s_step: a decoder with a rows LM steps with fltx_s2s_step_lm_rows")
    says(env, env.s2s_step(env.s2w), STATE,
         "fltx_s2s_step: a decoder with a word-level rows LM steps with fltx_s2s_step_word_lm_rows")
    says(env, env.s2s_step_lm_rows(env.s2z), STATE,
         "fltx_s2s_step_lm_rows: the decoder has no rows LM (fltx_lm_rows_create)")
    says(env, env.s2s_step_word_lm_rows(env.s2r), STATE,
         "fltx_s2s_step_word_lm_rows: the decoder has no word-level rows LM (fltx_lm_word_rows_create)")
