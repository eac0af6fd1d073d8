"""Recycled LM-state ids on streams of the lexicon CTC rows decoder (fltx_ctc_rows_stream_collect on a decoder of
fltx_ctc_rows_lex_decoder_create), word and token LM rows: tests/test_ctc_lm_rows_recycle.py's tracker and model on the
lexicon restatement of tests/test_lexicon_ctc_lm_rows_stream.py.  One stream is held inside a word across collects: its
state and the parent id it was made from stay pinned while nothing new is entered.

Every device test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_LEX_CTC_LMROWS_RECYCLE_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
import test_ctc_lm_rows_recycle as R0  # noqa: E402
import test_lexicon_ctc_lm_rows_stream as L1  # noqa: E402
from golden import make_lex_ctc_lm_rows_stream_golden as GS  # noqa: E402
from test_ctc_lm_rows import MIN_GAP, PrefixLM, Stats  # noqa: E402
from test_ctc_lm_rows import _dev  # noqa: E402
from test_lexicon_ctc_lm_rows import NINF, SMEAR_MAX, Lex, assert_final, dev_lm, make_dec, opts  # noqa: E402
from test_seq2seq_model_output import _GpuSess, _np  # noqa: E402

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

MAX_STATES = 32
N, K, W, LB = 6, 6, 8, 2
TS = (200, 120)
HOLD = (30, 75, 4)  # stream 1, frames 30 .. 74: letter 4, the first of the word [4, 5, 2], and little else
SIZES = ([10, 5, 15], [10])

_CASES = {}


def lex_case(sess, tokl, log_add):
    """emissions, restatement and table profile of the two streams; seeds without ties (logAdd: without a small gap)"""
    key = (tokl, log_add)
    if key in _CASES:
        return _CASES[key]
    # (lm_weight 0.3: at the 0.7 of the other stream tests the LM's answers -- down to -16 -- keep the search from
    # entering states: ten in 200 frames under the token LM, which charges every letter, 31 under the word LM)
    o = opts(K, N, 25.0, 0.3, 0.25, NINF, -0.3, 0, 1, -1, log_add, tokl)
    lex = GS.LEX["b" if tokl else "a"]
    rl = GS.GL.SmRowsLM(93, N if tokl else 6, W, 43, W - 1, 0)
    lx = Lex(sess.lib, N, 0, lex, 0 if tokl else SMEAR_MAX)  # (the restatement's trie, through the library's host trie)
    nodes = lx.nodes
    lx.close()
    cuts = R0.stream_cuts(TS, SIZES)
    ems, want, prof = [], [], []
    for b, T in enumerate(TS):
        for seed in range(2300 + 100 * b, 2360 + 100 * b):
            st = Stats()
            em = GS._emissions(seed, T, N)
            if b == 1:
                for t in range(HOLD[0], HOLD[1]):
                    keep = em[t] - np.float32(8.0)
                    keep[HOLD[2]] = np.float32(0.0)
                    em[t] = keep
            res = L1.restate_stream(em, nodes, PrefixLM(R0.last3(rl), rl.usr_to_lm, rl.finish), o,
                                    R0.script_of(cuts, b, LB), st=st)
            if not st.ties and (not log_add or st.gap > MIN_GAP):
                break
        assert not st.ties and (not log_add or st.gap > MIN_GAP), (b, st.ties, st.gap)
        ems.append(em)
        want.append(res)
        prof.append(R0.table_profile(res[3], R0.collect_points(cuts, b)))
    _CASES[key] = dict(o=o, lex=lex, rl=rl, cuts=cuts, ems=ems, want=want, prof=prof, log_add=log_add, tokl=tokl)
    return _CASES[key]


@pytest.mark.parametrize("tokl", [False, True], ids=["word_lm", "token_lm"])
@pytest.mark.parametrize("log_add", [False, True])
def test_lexicon_streams_through_a_small_table(sess, tokl, log_add):
    """200 and 120 frames in tables of 32 ids, prune(2) and collect after every chunk: row lists, bests (words included)
    and the n-best are the restatement's, every collect releases the model's dead set"""
    c = lex_case(sess, tokl, log_add)
    print("states ever / peak table / most released per stream:", c["prof"])
    assert c["prof"][0][0] > MAX_STATES, "the stream would pass without recycling"
    assert all(p[1] <= MAX_STATES for p in c["prof"]), "the table must hold what lives between two collects"
    # stream 1 sits inside a word over a whole chunk and the collects around it: its best hypothesis keeps its state,
    # and no state shows up in those frames that the stream had not entered before the chunk
    at = R0.collect_points(c["cuts"], 1)
    rows1 = c["want"][1][3]
    quiet = [i for i in range(1, len(at)) if at[i] > at[i - 1] and
             all(rows1[t][0][1] == -1 for t in range(at[i - 1], at[i])) and
             {s for t in range(at[i - 1], at[i]) for _, _, s in rows1[t]} <=
             {s for t in range(at[i - 1]) for _, _, s in rows1[t]}]
    assert quiet, "no chunk of the held stream without a new state"
    lx = Lex(sess.lib, N, 0, c["lex"], 0 if tokl else SMEAR_MAX)
    lm = dev_lm(sess, c["rl"], c["o"])
    dec = make_dec(sess, lx, lm, c["o"])
    dec.set_max_states(MAX_STATES)
    bests, final, ds = R0.run_recycling(sess, dec, c["ems"], N, W, lambda b, p: R0.last3(c["rl"])(p), c["cuts"], LB, 32,
                                        lexicon=True)
    R0.assert_against_restatement(c, bests, final, ds, final_check=assert_final)
    assert ds.ever[0] == c["prof"][0][0] and any(w >= 0 for g in bests[0] if g for w in g[4])
    for d in (dec, lm, lx):
        d.close()


def test_without_collect_the_lexicon_stream_stops(sess):
    """the same streams, no collect: "LM-state table full", as before"""
    c = lex_case(sess, False, False)
    lx = Lex(sess.lib, N, 0, c["lex"], SMEAR_MAX)
    lm = dev_lm(sess, c["rl"], c["o"])
    dec = make_dec(sess, lx, lm, c["o"])
    dec.set_max_states(MAX_STATES)
    ds = R0.S0.DeviceStreams(sess, dec, 2, N, W, lambda b, p: R0.last3(c["rl"])(p), 32, lexicon=True)
    at = [0, 0]
    for cut in c["cuts"]:
        ds.chunk([c["ems"][b][at[b]:at[b] + cut[b]] for b in range(2)])
        at = [a + x for a, x in zip(at, cut)]
        dec.prune(LB)
    with pytest.raises(_capi.FltxError) as e:
        dec.best(0)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "LM-state table full" in str(e.value)
    for d in (dec, lm, lx):
        d.close()


def test_refusals_on_the_lexicon_kind(sess):
    """outside a stream and on a lexicon decoder begun with fltx_ctc_rows_begin: FLTX_ERR_STATE; in a stream: the
    arguments, and a collect right after begin releases nothing"""
    S, I = _capi.ERR_STATE, _capi.ERR_INVALID
    o = opts(4, N, 25.0, 0.3, 0.25, NINF, 0.0, 0, 1, -1, False, False)
    lx = Lex(sess.lib, N, 0, GS.LEX["a"], SMEAR_MAX)
    lm = _capi.WordRowsLM(7, None, 6, lib=sess.lib)
    dec = make_dec(sess, lx, lm, o)
    collect = sess.lib.lib.fltx_ctc_rows_stream_collect
    bufs = [_dev(sess, np.zeros(8, np.int32)) for _ in range(3)]
    pr, pn, pl = [dec._addr(x) for x in bufs]
    assert collect(dec.h, 8, pr, pn, pl) == S
    dec.begin(GS._emissions(2500, 3, N), [3], N)
    assert collect(dec.h, 8, pr, pn, pl) == S
    dec.stream_begin(1, N, 8)
    assert collect(dec.h, 0, pr, pn, pl) == I and collect(dec.h, 8, None, pn, pl) == I
    assert collect(dec.h, 8, pr, pn, None) == 0 and collect(dec.h, 8, pr, pn, pl) == 0
    dec.ctx.synchronize()
    assert (_np(bufs[0]) == -1).all() and int(_np(bufs[1])[0]) == 0 and int(_np(bufs[2])[0]) == 1
    for d in (dec, lm, lx):
        d.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_CTC_LMROWS_RECYCLE_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
