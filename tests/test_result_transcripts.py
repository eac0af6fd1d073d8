"""fltx_result_transcripts (text_amd/csrc/fltx_transcript.h) through real decodes: the transcripts of the n-best of every
CTC / ASG decoder kind equal `restate` -- the rule of include/fltx.h written out here, not imported from the package --
applied to results_arrays() of the same decode; exact integer equality, scores bit for bit.

Emissions are peaked along a path that holds a plain repeat and a blank-separated repeat, T is 0, 1, 70 and 130 in one
batch (the longer two cross a tile of the kernels' walk, the last one two).

Every device test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_RESULT_TRANSCRIPTS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
from golden import make_ctc_lm_rows_golden as G  # noqa: E402
from golden import make_lex_ctc_lm_rows_golden as GL  # noqa: E402
import helpers  # noqa: E402
import test_ctc_lm_rows as R0  # noqa: E402
import test_lexicon_ctc_lm_rows as R1  # noqa: E402
from test_seq2seq_model_output import _bits_equal, _GpuSess, is_gpu  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
N, K, SIL, BLANK = 6, 6, 0, 1
TS = (70, 0, 1, 130)
SEED = 4100
LEX = GL.LEX["b"]  # words [2], [2 3], [3 2], [4 5 2], [5]
# one period of the path the emissions are peaked along: words of LEX, with 2 2 (a plain repeat), 2 blank 2 and
# 5 blank 5 (blank-separated repeats), sil between some words
PATH = [0, 2, 2, 1, 2, 2, 0, 5, 5, 1, 5, 0, 4, 4, 5, 5, 2, 2, 0, 3, 2, 1, 1, 2, 3, 0, 0]
KEYS = ("tokens", "timesteps", "words", "word_timesteps", "word_tok_end")


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


# ---- the rule --------------------------------------------------------------------------------------------------------------
def restate(tok, wrd, blank):
    """-> (tokens, timesteps, words, word_timesteps, word_tok_end) of one row"""
    toks, ts, ws, wts, wte = [], [], [], [], []
    for i in range(len(tok)):
        if tok[i] >= 0 and tok[i] != blank and (i == 0 or tok[i] != tok[i - 1]):
            toks.append(int(tok[i]))
            ts.append(i)
        if wrd is not None and wrd[i] >= 0:
            ws.append(int(wrd[i]))
            wts.append(i)
            wte.append(len(toks))
    return toks, ts, ws, wts, wte


def emissions():
    """[T, N] per utterance: G.emissions' values (in [-1, 0]) with 10 added along PATH"""
    ems = []
    for b, T in enumerate(TS):
        e = G.emissions(SEED + b, T, N).copy()
        for t in range(T):
            e[t, PATH[(t + 3 * b) % len(PATH)]] += np.float32(10.0)
        ems.append(e)
    return ems


def has_plain_repeat(row, blank):
    return any(row[i] == row[i - 1] and row[i] >= 0 and row[i] != blank for i in range(1, len(row)))


def has_blank_separated_repeat(row, blank):
    return any(row[i] == row[i - 2] and row[i - 1] == blank and row[i] >= 0 and row[i] != blank
               for i in range(2, len(row)))


def frame_rows(dec):
    """results_arrays() of the decode, copied -> (n_hyp, length, scores, rows per utterance [(tokens, words or None)])"""
    r = dec.results_arrays()
    nh, ln, off = r["n_hyp"].tolist(), r["length"].tolist(), r["offsets"].tolist()
    rows = []
    for b in range(dec.B):
        rows.append([])
        for i in range(nh[b]):
            a = off[b] + i * ln[b]
            rows[b].append((r["tokens"][a:a + ln[b]].tolist(),
                            None if r["words"] is None else r["words"][a:a + ln[b]].tolist()))
    return nh, ln, r["scores"].copy(), rows


def assert_transcripts(dec, blank, lexicon, max_hyps=(1, 2, None)):
    """transcripts(max_hyp) of the finished decode against the restatement on its frame rows -> those rows"""
    nh, ln, scores, rows = frame_rows(dec)
    Kd = int(dec.options.beam_size)
    for mh in max_hyps:
        t = dec.transcripts(mh)
        take = [min(n, Kd if mh is None else mh) for n in nh]
        assert t["row_first"].dtype == np.int64 and t["row_first"].tolist() == [0] + np.cumsum(take).tolist(), mh
        assert t["n_rows"] == sum(take)
        want = {k: [] for k in KEYS}
        tok_off, word_off = [0], [0]
        for b in range(dec.B):
            for i in range(take[b]):
                res = restate(rows[b][i][0], rows[b][i][1], blank)
                for k, v in zip(KEYS, res):
                    want[k] += v
                tok_off.append(len(want["tokens"]))
                word_off.append(len(want["words"]))
                if lexicon:
                    assert res[2] == [w for w in rows[b][i][1] if w >= 0]
            assert _bits_equal(t["scores"][b, :take[b]], scores[b, :take[b]]), (mh, b)
        assert t["tok_off"].tolist() == tok_off and t["word_off"].tolist() == word_off, mh
        for k in KEYS:
            assert t[k].tolist() == want[k], (mh, k)
        if not lexicon:
            assert t["words"].size == 0
    return nh, ln, rows


def assert_path_properties(rows, blank):
    """what makes the fixture worth its name, on the restatement's input: the best path of a long utterance holds a plain
    repeat and (under CTC) a blank-separated repeat, and collapses to fewer tokens than frames"""
    best = rows[0][0][0]
    assert has_plain_repeat(best, blank), best
    if blank >= 0:
        assert has_blank_separated_repeat(best, blank), best
    kept = restate(best, None, blank)[0]
    assert 2 < len(kept) < len(best)


# ---- the kinds ---------------------------------------------------------------------------------------------------------------
def lexfree(sess, crit="ctc"):
    tr = None
    if crit == "asg":
        rng = np.random.default_rng(3)
        tr = (rng.random((N, N)) * 0.1).astype(np.float32)
    opt = _capi.make_options(K, N, 25.0, 0.0, 0.0, -float("inf"), -0.1, False, crit)
    return _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, opt, sess.zero, SIL, BLANK, transitions=tr)


def batch_decode(dec, ems):
    dec.decode_batch(np.concatenate([e.reshape(-1) for e in ems]), [e.shape[0] for e in ems], N)


def test_lexicon_free_ctc_on_the_lane_engine(sess):
    dec = lexfree(sess)
    batch_decode(dec, emissions())
    assert dec.get("why_not_lane") == 0, "the decode left the lane engines"
    nh, ln, rows = assert_transcripts(dec, BLANK, False)
    assert_path_properties(rows, BLANK)
    # T = 0: the root's sil and decodeEnd's sil -- one token at timestep 0
    b = TS.index(0)
    t = dec.transcripts()
    q = int(t["row_first"][b])
    assert nh[b] == 1 and ln[b] == 2 and rows[b][0][0] == [SIL, SIL]
    assert t["tokens"][t["tok_off"][q]:t["tok_off"][q + 1]].tolist() == [SIL]
    assert t["timesteps"][t["tok_off"][q]:t["tok_off"][q + 1]].tolist() == [0]
    dec.close()


def test_lexicon_free_asg_has_no_blank(sess):
    dec = lexfree(sess, "asg")
    batch_decode(dec, emissions())
    nh, ln, rows = assert_transcripts(dec, -1, False)
    assert_path_properties(rows, -1)
    best = rows[0][0][0]
    assert BLANK in best and BLANK in restate(best, None, -1)[0]  # (token 1 is a letter like any other here)
    dec.close()


def lexicon_dec(sess, lx):
    opt = _capi.make_options(K, N, 25.0, 0.0, 0.5, -float("inf"), -0.1, False, "ctc")
    return _capi.BatchDecoder(sess.ctx, _capi.LEXICON, opt, sess.zero, SIL, BLANK, unk=-1, trie=lx.trie.upload(sess.ctx))


def assert_lexicon_fixture(dec, nh, rows):
    assert max(sum(1 for w in r[1] if w >= 0) for r in rows[0] + rows[3]) >= 2, "no utterance ends two words"
    # T = 0.  "Nothing before the first frame" (LexiconDecoder.cpp:276-280) holds before decodeEnd only: decodeEnd counts
    # as a frame (:273), so a FINISHED decode of no frames has the one hypothesis [sil, sil], as results_arrays() says --
    # one row, one token at timestep 0, no word
    t = dec.transcripts()
    b = TS.index(0)
    assert nh[b] == 1 and rows[b][0][0] == [SIL, SIL] and t["row_first"][b + 1] - t["row_first"][b] == 1
    q = int(t["row_first"][b])
    assert t["tokens"][t["tok_off"][q]:t["tok_off"][q + 1]].tolist() == [SIL]
    assert t["timesteps"][t["tok_off"][q]:t["tok_off"][q + 1]].tolist() == [0]
    assert t["word_off"][q] == t["word_off"][q + 1]
    # the spelling that ended each word of the best hypothesis, with its leading separators
    q = 0
    tok = t["tokens"][t["tok_off"][q]:t["tok_off"][q + 1]].tolist()
    ends = [0] + t["word_tok_end"][t["word_off"][q]:t["word_off"][q + 1]].tolist()
    spell = {w: sp for w, _, sp in LEX}
    for j, w in enumerate(t["words"][t["word_off"][q]:t["word_off"][q + 1]].tolist()):
        assert [x for x in tok[ends[j]:ends[j + 1]] if x != SIL] == spell[w], (j, w)


def test_lexicon_decoder(sess):
    lx = R1.Lex(sess.lib, N, SIL, LEX, 1)
    dec = lexicon_dec(sess, lx)
    batch_decode(dec, emissions())
    nh, ln, rows = assert_transcripts(dec, BLANK, True)
    assert_path_properties(rows, BLANK)
    assert_lexicon_fixture(dec, nh, rows)
    dec.close()
    lx.close()


def zero_rows(sess, W):
    def lm_rows(keys):
        return R0._dev(sess, np.zeros((max(len(keys), 1), W), np.float32))
    return lm_rows


def chunks_of(ems, size):
    out = []
    for at in range(0, max(TS), size):
        parts = [e[at:at + size] for e in ems]
        out.append((np.concatenate([p.reshape(-1) for p in parts]), [p.shape[0] for p in parts]))
    return out


@pytest.mark.parametrize("stream", [False, True], ids=["batch", "stream"])
def test_ctc_rows_kind_after_end(sess, stream):
    lm = _capi.RowsLM(N + 1, None, N, lib=sess.lib)
    dec = R0.make_dec(sess, lm, K, N, 25.0, 0.5, -0.1, SIL, BLANK, False)
    ems = emissions()
    if stream:
        list(dec.decode_stream(chunks_of(ems, 32), zero_rows(sess, N + 1), N=N, max_frames=160))
    else:
        dec.decode(np.concatenate([e.reshape(-1) for e in ems]), TS, N, zero_rows(sess, N + 1))
    nh, ln, rows = assert_transcripts(dec, BLANK, False)
    assert_path_properties(rows, BLANK)
    assert ln == [T + 2 for T in TS] and nh[TS.index(0)] == 1
    dec.close()
    lm.close()


@pytest.mark.parametrize("stream", [False, True], ids=["batch", "stream"])
def test_lexicon_ctc_rows_kind_after_end(sess, stream):
    lx = R1.Lex(sess.lib, N, SIL, LEX, 0)
    lm = _capi.RowsLM(N + 1, None, N, lib=sess.lib)
    o = R1.opts(K, N, 25.0, 0.5, 0.5, sil_score=-0.1, sil=SIL, blank=BLANK, is_lm_token=True)
    dec = R1.make_dec(sess, lx, lm, o)
    ems = emissions()
    if stream:
        list(dec.decode_stream(chunks_of(ems, 32), zero_rows(sess, N + 1), N=N, max_frames=160))
    else:
        dec.decode(np.concatenate([e.reshape(-1) for e in ems]), TS, N, zero_rows(sess, N + 1))
    nh, ln, rows = assert_transcripts(dec, BLANK, True)
    assert_path_properties(rows, BLANK)
    assert_lexicon_fixture(dec, nh, rows)
    for d in (dec, lm, lx):
        d.close()


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def test_contract(sess):
    L = sess.lib.lib
    t = _capi.Transcripts()
    dec = lexfree(sess)
    assert L.fltx_result_transcripts(dec.h, 1, 0, C.byref(t)) == _capi.ERR_STATE  # before any decode
    s2s = _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    assert L.fltx_result_transcripts(s2s.h, 1, 0, C.byref(t)) == _capi.ERR_STATE
    assert "seq2seq" in L.fltx_last_error().decode()
    s2s.close()
    ems = emissions()
    batch_decode(dec, ems)
    before = [[(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in hyps] for hyps in dec.results_batch()]
    assert L.fltx_result_transcripts(dec.h, 0, 0, C.byref(t)) == _capi.ERR_INVALID
    assert L.fltx_result_transcripts(dec.h, 1, 0, None) == _capi.ERR_INVALID
    assert L.fltx_result_transcripts(None, 1, 0, C.byref(t)) == _capi.ERR_INVALID
    tr = dec.transcripts()
    flat = {k: tr[k].copy() for k in KEYS + ("tok_off", "word_off", "row_first", "scores")}
    # the other fetch calls return what they returned
    after = [[(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in hyps] for hyps in dec.results_batch()]
    assert after == before
    assert [[(h.score, h.tokens.tolist()) for h in dec.results(b)] for b in range(dec.B)] == \
        [[(h[0], h[3]) for h in hyps] for hyps in before]
    # transcripts_batch() is transcripts(), sliced
    for mh in (None, 2):
        tb = dec.transcripts_batch(mh)
        assert [len(x) for x in tb] == [min(len(h), K if mh is None else mh) for h in before]
        for b, hyps in enumerate(tb):
            for i, h in enumerate(hyps):
                q = int(flat["row_first"][b]) + i if mh is None else None
                assert (h.score, h.am, h.lm) == before[b][i][:3]
                want = restate(before[b][i][3], None, BLANK)
                assert (h.tokens.tolist(), h.timesteps.tolist()) == want[:2] and h.words.size == 0
                assert h.word_timesteps.size == 0 and h.word_tok_end.size == 0
                if q is not None:
                    a, z = int(flat["tok_off"][q]), int(flat["tok_off"][q + 1])
                    assert h.tokens.tolist() == flat["tokens"][a:z].tolist()
    # a second call allocates nothing: the same buffers
    where = [dec.transcripts()[k].ctypes.data for k in KEYS[:2] + ("tok_off",)]
    assert [dec.transcripts()[k].ctypes.data for k in KEYS[:2] + ("tok_off",)] == where
    # device=True: addresses and sizes, the same totals
    d = dec.transcripts(device=True)
    assert d["n_tokens"] == flat["tokens"].size and d["n_words"] == 0 and d["n_rows"] == tr["n_rows"]
    assert all(isinstance(d[k], int) and d[k] for k in ("tokens", "timesteps", "tok_off", "word_off", "scores"))
    dec.close()
    # defer_check: the call settles the batch itself
    dec = lexfree(sess)
    dec.set("defer_check", 1)
    batch_decode(dec, ems)
    got = dec.transcripts()
    for k in KEYS + ("tok_off", "word_off", "row_first"):
        assert got[k].tolist() == flat[k].tolist(), k
    assert _bits_equal(got["scores"][0, :1], flat["scores"][0, :1])
    dec.close()


# ---- the reference's own n-best ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _decodertest_transcripts(gpu_sess, tmp_path):
    """The DecoderTest configuration (tests/test_gpu_parity.py replays it: LexiconDecoder, 3-gram, ASG, beam 2500, T = 235):
    the transcript words are the non-negative entries of each golden hypothesis' words, the transcript tokens the collapse
    of its tokens -- the compiled reference's n-best, not our own fetch path.  On the HIP library only: a beam of 2500 over a
    26 000-word trie for 235 frames takes the emulator minutes (tests/test_gpu_parity.py replays it on the device alone for
    the same reason); the walk itself runs on the emulator in every other case of this module."""
    import gzip
    import json
    from golden.make_golden import parse_lexicon_dump
    d = os.path.join(helpers.GOLDEN_DIR, "decodertest")
    rd = lambda n: gzip.open(os.path.join(d, n + ".gz"), "rb").read()  # noqa: E731
    lex = parse_lexicon_dump(rd("lexicon_dump.txt").decode())
    TN = np.frombuffer(rd("TN.bin"), dtype=np.int32)
    T, Nt = int(TN[0]), int(TN[1])
    em = np.frombuffer(rd("emission.bin"), dtype=np.float32).copy()
    tr = np.frombuffer(rd("transition.bin"), dtype=np.float32).copy()
    arpa = tmp_path / "lm.arpa"
    arpa.write_bytes(rd("lm.arpa"))
    exp = json.load(open(os.path.join(d, "expected.json")))["nbest"]
    lm = _capi.ArpaLM(str(arpa), lex["words"], lib=gpu_sess.lib)
    ht = _capi.HostTrie(lex["ntok"], lex["sil"], lib=gpu_sess.lib)
    cache = {}
    for wi, w, sp in lex["entries"]:
        if wi not in cache:
            cache[wi] = lm.score_sequence([wi], False)[0][0]
        ht.insert(sp, wi, cache[wi])
    ht.smear(1)
    ctx = gpu_sess.ctx
    opt = _capi.make_options(2500, 25000, 100.0, 2.0, 2.0, -float("inf"), -1.0, False, "asg")
    dec = _capi.BatchDecoder(ctx, _capi.LEXICON, opt, lm, lex["sil"], -1, unk=lex["unk"], trie=ht.upload(ctx),
                             transitions=tr, is_lm_token=False)
    dec.decode_batch(em, [T], Nt)
    hyps = dec.transcripts_batch()[0]
    assert len(hyps) == exp["n"] == len(exp["tokens"]) and exp["n"] > 1
    for i, h in enumerate(hyps):
        want = restate(exp["tokens"][i], exp["words"][i], -1)
        assert h.words.tolist() == [w for w in exp["words"][i] if w >= 0] == want[2] and len(want[2]) > 1
        assert h.tokens.tolist() == want[0] and 0 < len(want[0]) < len(exp["tokens"][i])
        assert h.timesteps.tolist() == want[1]
        assert (h.word_timesteps.tolist(), h.word_tok_end.tolist()) == want[3:]
        assert h.score == float.fromhex(exp["scores"][i][0])
    dec.close()
    lm.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_RESULT_TRANSCRIPTS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if CHILD:
    test_decodertest_transcripts = _decodertest_transcripts
else:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
