"""fltx_ctc_rows_stream_finish on the lexicon CTC rows decoder, with a word LM and with a token LM: the checks of
tests/test_ctc_lm_rows_stream_finish.py -- a reused slot against a fresh B = 1 stream and the float64 restatement of
tests/test_lexicon_ctc_lm_rows_stream.py, a bystander against the script without finishes, stale ring rows (the lexicon
ring holds kLookBackLimit rows more), a beam of 70, a stream emptied by a frame without candidates, a typed chunk after a
restart, and the results with their words on the host and on the device.

Every device test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_LEX_CTC_LMROWS_FINISH_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

import test_ctc_lm_rows_stream_finish as F0  # noqa: E402
import test_lexicon_ctc_lm_rows as L0  # noqa: E402
import test_lexicon_ctc_lm_rows_stream as LS  # noqa: E402
from golden import make_lex_ctc_lm_rows_stream_golden as GS  # noqa: E402
from test_ctc_lm_rows import PrefixLM  # noqa: E402
from test_lexicon_ctc_lm_rows import NINF, SMEAR_MAX, Lex, dev_lm, make_dec, opts  # noqa: E402
from test_seq2seq_model_output import _GpuSess  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
LMS = pytest.mark.parametrize("tokl", [False, True], ids=["word_lm", "token_lm"])


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


class LexKind(F0.Kind):
    """The lexicon kind as tests/test_lexicon_ctc_lm_rows_stream.py has it: N = 6, K = 6, W = 8, lexicon "a" under a word
    LM and "b" under a token LM"""
    lexicon = True

    def __init__(self, tokl, log_add=False, K=6, thr=25.0):
        self.tokl, self.log_add, self.K, self.N, self.W, self.thr = tokl, log_add, K, 6, 8, thr
        self.sil, self.blank = 0, 1
        self.o = opts(K, self.N, thr, 0.7, 0.25, NINF, -0.3, 0, 1, -1, log_add, tokl)
        self.rl = GS.GL.SmRowsLM(93, 6, self.W, 43, self.W - 1, 0)
        self.row = lambda p: self.rl.row(list(p))

    def open(self, sess):
        self.sess = sess
        self.lx = Lex(sess.lib, self.N, 0, GS.LEX["b" if self.tokl else "a"], 0 if self.tokl else SMEAR_MAX)
        self.lm = dev_lm(sess, self.rl, self.o)
        return self

    def dec(self, max_states=None):
        d = make_dec(self.sess, self.lx, self.lm, self.o)
        if max_states is not None:
            d.set_max_states(max_states)
        return d

    def close(self):
        self.lm.close()
        self.lx.close()

    def emissions(self, seed, T):
        return GS._emissions(seed, T, self.N)

    def restate(self, em, script, st):
        lm = PrefixLM(self.row, self.rl.usr_to_lm, self.rl.finish)
        return LS.restate_stream(em, self.lx.nodes, lm, self.o, script, st=st)

    assert_final = staticmethod(L0.assert_final)
    assert_rows = staticmethod(L0.assert_rows)


@LMS
@pytest.mark.parametrize("log_add", [False, True], ids=["max", "logadd"])
def test_reused_slot_is_a_fresh_stream_and_a_bystander_sees_nothing(sess, tokl, log_add):
    F0.check_reused_slot(sess, LexKind(tokl, log_add))


@LMS
def test_stale_ring_rows(sess, tokl):
    F0.check_stale_ring_rows(sess, LexKind(tokl))


@LMS
def test_emptied_stream_comes_back(sess, tokl):
    F0.check_empty_beam_comes_back(sess, LexKind(tokl))


@LMS
def test_wide_beam(sess, tokl):
    F0.check_wide_beam(sess, LexKind(tokl, K=70, thr=1e9))


@LMS
def test_typed_chunk_after_a_restart(sess, tokl):
    F0.check_typed_chunk_after_restart(sess, LexKind(tokl))


@LMS
def test_results_on_the_host_and_on_the_device(sess, tokl):
    F0.check_results(sess, LexKind(tokl))


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_CTC_LMROWS_FINISH_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
