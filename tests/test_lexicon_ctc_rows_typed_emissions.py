"""fp16 / bf16 / float32 emissions and raw logits in the lexicon CTC rows decoder (fltx_ctc_rows_begin_typed,
fltx_ctc_rows_stream_append_typed; the step's blank and same-node emissions read through the typed frames,
text_amd/csrc/fltx_ctc_rows_lex.h).

The parity chain of tests/test_ctc_rows_typed_emissions.py on this kind: decoder A on the typed frames, decoder B on the
float32 matrix they stand for through the existing float32 entry points -- row lists, tokens, WORDS and all three scores
bit for bit, word LM and token LM, unk on and off, max-merge and logAdd.  Here the step itself reads emissions: the
cases use a token beam small enough that the float32 decoder B provably takes the blank or the same-node candidate of a
token that is NOT in the frame's token beam (asserted on B's best path), so a wrong typed read shows.  The typed entry
with float32 log-probs reproduces the compiled reference's fixtures.

Every case runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_LEX_CTC_ROWS_TYPED_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from golden import make_lex_ctc_lm_rows_golden as G  # noqa: E402
import test_lexicon_ctc_lm_rows as L0  # noqa: E402
import test_ctc_rows_typed_emissions as T0  # noqa: E402
from test_ctc_rows_typed_emissions import begin_typed, frames, run_pair, stream_script  # noqa: E402
from test_lexicon_ctc_lm_rows import NINF, SMEAR_MAX, Lex, dedup, dev_lm, make_dec, opts  # noqa: E402
from test_seq2seq_model_output import BF16, F16, F32, _GpuSess  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
DT_NAMES = T0.DT_NAMES


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


class Case:
    """lexicon "a" (unk on: word id 6) over N = 6 tokens, sil 0, blank 1"""

    def __init__(self, sess, tokl, K=6, Kt=2, log_add=False, unk=True, thr=25.0):
        self.sess, self.N = sess, 6
        lex = dedup(G.LEX["a"]) if tokl else G.LEX["a"]
        self.o = opts(K, Kt, thr, 0.7, 0.25, -0.5 if unk else NINF, -0.2, unk=6 if unk else -1, log_add=log_add,
                      is_lm_token=tokl)
        self.lx = Lex(sess.lib, self.N, 0, lex, 0 if tokl else SMEAR_MAX)
        n_map = self.N if tokl else 7
        self.W = n_map + 2
        self.rl = G.SmRowsLM(0x5A5A ^ (17 if tokl else 3), n_map, self.W, 0, self.W - 1, 0)
        self.lm = dev_lm(sess, self.rl, self.o, mapped=False)

    def mk(self):
        return make_dec(self.sess, self.lx, self.lm, self.o)

    def lm_row(self, b, p):
        return self.rl.row(list(p))

    def pair(self, raws, dt, kind, **kw):
        return run_pair(self.sess, self.mk, L0.decode, raws, dt, kind, self.N, self.W, self.lm_row, **kw)

    def close(self):
        for d in (self.lm, self.lx):
            d.close()


def outside_the_token_beam(e32, final, Kt):
    """frames of the best path whose token is not among the frame's Kt largest emissions (ties to the lower token): only
    the step's blank and same-node candidates, read from the frame itself, can have put it there"""
    out = []
    if not final:
        return out
    toks = final[0][3]
    for t in range(e32.shape[0]):
        e = e32[t]
        kept = sorted((n for n in range(e.size) if not np.isnan(e[n])), key=lambda n: (-float(e[n]), n))[:Kt]
        if toks[t + 1] not in kept:
            out.append(t)
    return out


CASES = [(dt, kind, tokl) for dt in (F16, BF16, F32) for kind in ("log_probs", "logits") for tokl in (False, True)]


@pytest.mark.parametrize("dt,kind,tokl", CASES,
                         ids=["%s-%s-%s" % (DT_NAMES[c[0]], c[1], "token" if c[2] else "word") for c in CASES])
def test_parity_with_candidates_outside_the_token_beam(sess, dt, kind, tokl):
    """beam_size_token = 2 of N = 6, unk_score > -inf, T = 9, 0 and 5 at odd offsets and an odd stride: a best path of
    B holds a blank / same-node token from outside the frame's token beam"""
    i = CASES.index((dt, kind, tokl))
    c = Case(sess, tokl, Kt=2, log_add=i % 3 == 2)
    raws = [frames(6000 + 10 * i + b, T, 6, dt, kind) for b, T in enumerate((9, 0, 5))]
    a, b, e32, _ = c.pair(raws, dt, kind, layout="odd", host=i % 4 == 1)
    used = [outside_the_token_beam(e32[u], b[0][u], 2) for u in (0, 2)]
    assert used[0] or used[1], used
    assert any(w >= 0 for h in a[0][0] for w in h[4]) or tokl  # (words ended)
    c.close()


@pytest.mark.parametrize("front", ["wave", "wg"])
def test_both_front_ends_and_no_unknown_word(sess, front):
    c = Case(sess, False, Kt=3, unk=False)
    c.pair([frames(6200 + b, T, 6, BF16, "logits") for b, T in enumerate((7, 3))], BF16, "logits", front=front)
    c.close()


def test_special_values_in_the_direct_reads(sess):
    """NaN, -inf and -0 at blank and at the hypothesis' own token: the two direct reads see what the float32 step sees;
    an all-NaN frame leaves no candidate"""
    inf = np.inf
    x = np.asarray([[-1.0, -3.0, -0.25, -0.5, -2.0, -4.0],
                    [-1.0, np.nan, -0.0, -0.5, -inf, -4.0],
                    [-0.5, -inf, np.nan, -0.25, -2.0, -1.0],
                    [-2.0, -0.0, -0.25, -1.5, -1.0, np.nan]])
    for dt in (F16, BF16):
        for kind in ("log_probs", "logits"):
            c = Case(sess, False, Kt=2)
            a, _, _, _ = c.pair([T0.to_dtype(x, dt).reshape(4, 6)], dt, kind, layout="odd")
            assert a[0][0]
            c.close()
    y = x.copy()
    y[2] = np.nan
    c = Case(sess, True, Kt=2)
    a, _, _, ls = c.pair([T0.to_dtype(y, F16).reshape(4, 6)], F16, "logits")
    assert ls[2] == -inf and a[0][0] == []
    c.close()


@pytest.mark.parametrize("c", L0._golden(), ids=lambda c: c["name"])
def test_typed_float32_log_probs_reproduce_reference_fixtures(c, sess):
    o = L0.case_opts(c)
    rl = G.case_lm(c)
    lx = Lex(sess.lib, c["N"], c["sil"], c["lex"], 0 if c["is_lm_token"] else SMEAR_MAX)
    lm = dev_lm(sess, rl, o, mapped=bool(c["perm"]))
    dec = make_dec(sess, lx, lm, o)
    em = G.emissions(c["seed"], c["T"], c["N"])
    dec.begin = lambda flat, Ts, N: begin_typed(sess, dec, em.reshape(-1), F32, "log_probs", False, None, 0, Ts, N, None)
    got, _, _ = L0.decode(sess, dec, [em], c["N"], rl.W, lambda b, p: rl.row(list(p)))
    L0.assert_final(c["hyps"], got[0], c["log_add"], c["name"])
    for d in (dec, lm, lx):
        d.close()


@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
def test_streams_event_by_event(sess, tokl):
    """tests/test_ctc_rows_typed_emissions.py's script on this kind, whose step reads the chunk's buffer: a device chunk
    overwritten after the next append has been queued changes nothing"""
    c = Case(sess, tokl, K=4, Kt=2)
    stream_script(sess, c.mk, c.N, c.W, c.lm_row, lexicon=True)
    c.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_CTC_ROWS_TYPED_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
