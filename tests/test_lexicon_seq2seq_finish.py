"""fltx_s2s_finish / fltx_s2s_done_each on the lexicon seq2seq decoder (text_amd/csrc/fltx_s2s_lex.h: S2lFinishKind):
the scripts of tests/test_seq2seq_finish.py -- the queue through few slots, the bystander, the reused slot, the edges,
decode_queue -- with the n-gram tables over the words, a token rows LM and a word rows LM (next_word, lm_row_of), and
what only this kind has: a restarted slot's state table, count, status and merges start over.

The yardstick is the ordinary batch (fltx_s2s_begin / step / fltx_s2s_end, one slot per utterance), which
tests/test_lexicon_seq2seq.py and its rows-LM siblings hold to the reference; `restate_lex()` of that file runs on the
CPU to show that the inputs are tie-free and the schedules the ones meant.

Every test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi, ngram_synth  # noqa: E402

CHILD = os.environ.get("FLTX_LEX_S2S_FINISH_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from golden import make_lex_s2s_lm_rows_golden as GL  # noqa: E402
from golden.make_s2s_lm_rows_golden import SmRowsLM  # noqa: E402
from test_collapse_rows import read_device  # noqa: E402
from test_lexicon_seq2seq import (ObjLM, _GpuSess, host_trie, is_gpu, make_lexicon, restate_lex, sm_model,  # noqa: E402
                                  trie_nodes)
from test_seq2seq_finish import (Batch, Setup, Utt, _dev, _trim, bystander_case, decode_queue_case, edges_case,  # noqa: E402
                                 fin_hyps, queue_case, reuse_case)

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]


@pytest.fixture(scope="module")
def gpu_sess(gpu_session):
    return _GpuSess(gpu_session)


@pytest.fixture(params=BACKENDS)
def sess(request):
    if request.param == "emu":
        return request.getfixturevalue("emu_session")
    import torch
    g = request.getfixturevalue("gpu_sess")
    torch.cuda.set_stream(g.stream)
    return g


# ---- decoder configurations --------------------------------------------------------------------------------------------
class LexSetup(Setup):
    """The lexicon kind with the n-gram tables over the words.  Seeds are moved on to the first whose search the
    restatement finds tie-free (as tests/test_lexicon_seq2seq.py does); the tests assert that it is."""
    V, K, Kt, eos, maxlen, thr, lmw = 14, 4, 14, 0, 6, 20.0, 0.8
    word_score, log_add, is_lm_token = -0.2, False, False
    n_words, lex_seed, smear = 40, 21, 1
    max_states = None
    never, quick, mid = -40.0, 40.0, 20.0  # (the model's scores span 16 a step; the threshold is 20)

    def __init__(self, sess, **kw):
        super().__init__(**kw)
        self.sess = sess
        self._trie = self._nodes = None
        self.lexicon = self.make_lexicon()

    def make_lexicon(self):
        return make_lexicon(self.V, self.eos, self.n_words, self.lex_seed, respell=0.3)

    def trie(self, sess):
        if self._trie is None:
            self._trie = host_trie(sess.lib, self.V, self.lexicon, self.smear)
            self._nodes = trie_nodes(self._trie)
        return self._trie

    def lm(self, sess):
        if self._lm is None:
            import tempfile
            self._tmp = tempfile.TemporaryDirectory()
            path = os.path.join(self._tmp.name, "w%d.arpa" % self.n_words)
            vocab = ngram_synth.words(self.n_words, "w")
            ngram_synth.write_arpa(path, vocab, 3, (0, 300, 150), 5)
            self._lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
        return self._lm

    def obj_lm(self, sess, u):
        return ObjLM(self.lm(sess))

    def _utt(self, seed, eos_bias):
        return Utt(sm_model(seed, self.V, self.eos, eos_bias, self.drop))

    def utt(self, seed, eos_bias):
        for s in range(seed * 1000, seed * 1000 + 60):
            ties = []
            u = self._utt(s, eos_bias)
            n = len(self.restate_utt(self.sess, u, ties)[1])
            if not ties and (eos_bias != self.never or n == self.maxlen):  # (`never`: nor does its beam die out)
                return u
        raise AssertionError("no tie-free seed from %d" % (seed * 1000))

    def make_dec(self, sess):
        opts = _capi.make_s2s_lex_options(self.K, self.Kt, self.thr, self.lmw, self.word_score, self.eos_score,
                                          self.log_add)
        dec = _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, opts, self.trie(sess), self.lm(sess), self.eos, self.maxlen,
                                               self.is_lm_token)
        if self.max_states is not None:
            dec.set_max_states(self.max_states)
        return dec

    def restate_utt(self, sess, u, ties):
        self.trie(sess)
        final, rows = restate_lex(u, self._nodes, self.obj_lm(sess, u), self.K, self.Kt, self.thr, self.lmw,
                                  self.word_score, self.eos_score, self.eos, self.maxlen, self.log_add,
                                  self.is_lm_token, ties=ties)
        assert not any(h[5] for h in final)  # (no logAdd fold: the scores are exact)
        return [h[:5] for h in final], rows

    def close(self):
        if self._lm is not None:
            self._lm.close()
            self._lm = None
            if hasattr(self, "_tmp"):
                self._tmp.cleanup()


class LexTokenRowsSetup(LexSetup):
    """a token rows LM (is_lm_token): the LM's rows next to the model's"""
    V, eos, Kt, lmw, word_score, is_lm_token = 10, 9, 10, 0.6, 0.2, True
    n_words, lex_seed = 30, 31
    W, perm = 12, 77

    def make_lexicon(self):
        return make_lexicon(self.V, self.eos, self.n_words, self.lex_seed, max_len=3, respell=0.3, single=0.4)

    def lm(self, sess):
        if self._lm is None:
            rl = SmRowsLM(1, self.V, self.W, self.perm, self.W - 1, self.eos)
            self._lm = _capi.RowsLM(rl.W, rl.usr_to_lm, rl.finish, lib=sess.lib)
        return self._lm

    def _utt(self, seed, eos_bias):
        return Utt(sm_model(seed, self.V, self.eos, eos_bias, self.drop),
                   SmRowsLM(seed ^ 0xABCDEF, self.V, self.W, self.perm, self.W - 1, self.eos))

    def obj_lm(self, sess, u):
        return GL.PrefixObjLM(u.lm)


class LexWordRowsSetup(LexTokenRowsSetup):
    """a word rows LM: one LM row per decoder row, handed over in reverse order through lm_row_of; the lists carry
    next_word, and a row's LM state is kept from next_src_row and next_word alone"""
    is_lm_token, words = False, True
    W, perm = 33, 78

    def lm(self, sess):
        if self._lm is None:
            rl = SmRowsLM(1, self.n_words, self.W, self.perm, self.W - 1, 0)
            self._lm = _capi.WordRowsLM(rl.W, rl.usr_to_lm, rl.finish, lib=sess.lib)
        return self._lm

    def _utt(self, seed, eos_bias):
        return Utt(sm_model(seed, self.V, self.eos, eos_bias, self.drop),
                   SmRowsLM(seed ^ 0xABCDEF, self.n_words, self.W, self.perm, self.W - 1, 0))

    def step(self, sess, dec, sc, valid, lr):
        n = lr.shape[0]
        ro = np.arange(n - 1, -1, -1, dtype=np.int32)
        return dec.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, np.ascontiguousarray(lr[::-1])),
                        lm_row_of=_dev(sess, ro))


SETUPS = {
    "ngram": LexSetup,
    "token_rows": LexTokenRowsSetup,
    "word_rows": LexWordRowsSetup,
}


@pytest.mark.parametrize("name", sorted(SETUPS))
def test_queue_through_three_slots(sess, name):
    queue_case(sess, SETUPS[name](sess))


@pytest.mark.parametrize("name", sorted(SETUPS))
def test_bystander_is_untouched(sess, name):
    bystander_case(sess, SETUPS[name](sess))


@pytest.mark.parametrize("name", ["ngram", "word_rows"])
def test_third_utterance_of_a_slot_equals_a_fresh_decode(sess, name):
    reuse_case(sess, SETUPS[name](sess))


@pytest.mark.parametrize("name,K", [("token_rows", 1), ("word_rows", 4), ("ngram", 70)])
def test_edges(sess, name, K):
    edges_case(sess, SETUPS[name](sess, K=K))


def test_decode_queue(sess):
    decode_queue_case(sess, SETUPS["token_rows"](sess))


# ---- what only the lexicon kind has ---------------------------------------------------------------------------------------
def _end_counts(sess, dec, B):
    """n_hyp of every slot after fltx_s2s_end, whatever the slots' statuses"""
    p = C.c_void_p()
    assert sess.lib.lib.fltx_result_device(dec.h, C.byref(p), None, None, None, None) == 0
    return read_device(sess, p.value, B, np.int32).tolist()


def test_full_state_table_then_a_clean_utterance(sess):
    """max_states 3.  The first utterance of slot 0 runs its state table full and stops: the finish reports it in
    status[b], with fltx_s2s_end's n_hyp.  The next utterance in that slot needs no more than three states, so it
    decodes clean exactly if the restart emptied the table and started the count, the status and the merges over."""
    setup = LexSetup(sess, max_states=3)
    big, short = setup.utt(41, setup.never), setup.utt(42, setup.quick)
    ties = []
    want_short, rows_short = setup.restate_utt(sess, short, ties)
    assert ties == []
    # the yardstick: the ordinary batch with the same table -- the long utterance stops, the short one fits
    twin = Batch(sess, setup, [(0, big), (1, short)])
    for _ in range(setup.maxlen + 1):
        twin.step()
    twin.dec.end()
    want_n = _end_counts(sess, twin.dec, 2)
    with pytest.raises(_capi.FltxError, match="LM-state table full"):
        twin.dec.results(0)
    assert [(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in twin.dec.results(1)] == want_short
    twin.close()
    # the same utterances one after the other through slot 0
    bt = Batch(sess, setup, [(0, big), None])
    while not bt.done_each()[0]:
        bt.step()
    assert bt.steps < setup.maxlen  # (it stopped: it never proposes eos)
    fin = bt.finish([1, 0], {0: (1, short)})
    assert fin["status"][0] == _capi.ERR_UNSUPPORTED and fin["n_hyp"][0] == want_n[0] and fin["hyps"][0] == []
    while not bt.done_each()[0]:
        bt.step()
    fin = bt.finish([2, 0])
    assert fin_hyps(fin, 0) == want_short
    assert _trim(bt.rows[1]) == _trim([[tuple(r) for r in step] for step in rows_short])
    assert bt.dec.info()["merges"][0] == 0
    bt.close()
    setup.close()


def test_refusals(sess):
    """a word-rows decoder lists next_word: NULL is refused; the other refusals are the lexicon-free kind's"""
    setup = LexWordRowsSetup(sess)
    dec = setup.make_dec(sess)
    dec.begin(2, setup.V)
    lists = dec._rows()
    fo = _capi.S2sFinishedOut()
    w = np.zeros(2, np.int32)
    a = [dec._addr(x) for x in lists]
    L = sess.lib.lib
    assert L.fltx_s2s_finish(dec.h, w.ctypes.data, *a, None, 0, C.byref(fo)) == _capi.ERR_INVALID
    word = lists[0].copy() if isinstance(lists[0], np.ndarray) else lists[0].clone()
    assert L.fltx_s2s_finish(dec.h, w.ctypes.data, *a, dec._addr(word), 0, C.byref(fo)) == _capi.FLTX_OK
    assert fo.words  # (the lexicon kind's results carry words)
    dec.close()
    setup.close()


# ---- the GPU cases, in a fresh process ------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_S2S_FINISH_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
