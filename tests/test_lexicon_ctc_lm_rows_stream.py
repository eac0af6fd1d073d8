"""Streams on the lexicon CTC rows decoder (fltx_ctc_rows_stream_* on a decoder of fltx_ctc_rows_lex_decoder_create,
text_amd/csrc/fltx_ctc_rows_stream.h): decodeStep on chunks, getBestHypothesis(lookBack) and prune(lookBack) with the
lexicon decoder's walk on to a complete hypothesis (its parent ended a word; look_back + 100 steps at most), word and token
LM rows.

The checks: a stream without prunes against the offline begin / step / end, bit for bit, row lists included; the compiled
reference's fixtures (tests/golden/make_lex_ctc_lm_rows_stream_golden.py) -- reproduced by the float64 restatement below
and by the device: tokens and words exact, the three scores bit-identical under max-merge and within 1e-5 under logAdd --
among them a best ancestor inside a word, and a non-final letter held for more than 104 frames, where look_back + 100
steps end the walk and the history ring wraps; the buffer's bound; the Python helper.

The restatement is tests/test_lexicon_ctc_lm_rows.py's frame (restated here on hypotheses that point at their parents)
under the StreamBuffer of tests/test_ctc_lm_rows_stream.py.

Every device test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import gzip
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_LEX_CTC_LMROWS_STREAM_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
import test_ctc_lm_rows as C0  # noqa: E402
import test_ctc_lm_rows_stream as S0  # noqa: E402
import test_lexicon_ctc_lm_rows as L0  # noqa: E402
from golden import make_lex_ctc_lm_rows_stream_golden as GS  # noqa: E402
from test_ctc_lm_rows import MIN_GAP, PrefixLM, Stats, _dev  # noqa: E402,F401
from test_lexicon_ctc_lm_rows import NINF, SMEAR_MAX, Lex, _fsub, assert_final, dev_lm, make_dec, opts  # noqa: E402
from test_seq2seq_model_output import _bits_equal, _GpuSess, is_gpu  # noqa: E402,F401

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


# ---- the restatement --------------------------------------------------------------------------------------------------
def lex_frame(beam, e, nodes, lm, o, st, where):
    """one frame of tests/test_lexicon_ctc_lm_rows.py's restate (LexiconDecoder.cpp:47-226) on a beam of parent-linked
    hypotheses -> the next beam, best first"""
    N = len(e)
    K, Kt, thr, lmw, sil, blank, tokl = o["K"], o["Kt"], o["thr"], o["lmw"], o["sil"], o["blank"], o["is_lm_token"]
    order = sorted((n for n in range(N) if not np.isnan(e[n])), key=lambda n: (-float(e[n]), n))
    kt = min(Kt, N)
    if len(order) > kt and e[order[kt - 1]] == e[order[kt]]:
        st.ties.append((where, "token cut"))
    kept = sorted(order[:kt])
    cands = []

    def add(h, i, score, a, l, state, node, n, word, pb, edge):
        if math.isnan(score):
            return
        cands.append(dict(score=score, am=h["am"] + a, lm=h["lm"] + l if l is not None else h["lm"], state=state,
                          node=node, token=n, word=word, pb=pb, src=i, edge=edge, key=(state, node, n, pb), parent=h))
    for i, h in enumerate(beam):
        kids_h = nodes[h["node"]][0]
        lex_max = 0.0 if h["node"] == 0 else float(nodes[h["node"]][2])
        for n in kept:
            c = kids_h.get(n)
            if c is None:
                continue
            a = float(e[n])
            s = h["score"] + a
            if n == sil:
                s += o["sil_score"]
            if tokl:
                state_n, l_n = lm.score(h["state"], n)
            kids, labels, ms = nodes[c]
            new_tok = h["pb"] or n != h["token"]
            if new_tok and kids:
                if tokl:
                    add(h, i, s + lmw * l_n, a, l_n, state_n, c, n, -1, False, n)
                else:
                    l = _fsub(ms, lex_max)
                    add(h, i, s + lmw * l, a, l, h["state"], c, n, -1, False, -1)
            ends = [(w, o["word_score"]) for w in labels]
            if ends and h["node"] == 0 and h["token"] == n:
                ends = []
            if not labels and o["unk_score"] > NINF:
                ends = [(o["unk"], o["unk_score"])]
            for w, ws in ends:
                if tokl:
                    state, l = state_n, l_n
                else:
                    state, l = lm.score(h["state"], w)
                    l = _fsub(l, lex_max)
                add(h, i, (s + lmw * l) + ws, a, l, state, 0, n, w, False, n if tokl else w)
        if not h["pb"] or h["node"] == 0:
            n = sil if h["node"] == 0 else h["token"]
            a = float(e[n])
            s = h["score"] + a
            if n == sil:
                s += o["sil_score"]
            add(h, i, s, a, None, h["state"], h["node"], n, -1, False, -1)
        a = float(e[blank])
        add(h, i, h["score"] + a, a, None, h["state"], h["node"], blank, -1, True, -1)
    return C0._store(cands, K, thr, o["log_add"], st, where)


def _complete(h):
    """LexiconDecoder.h:97-99"""
    return h["parent"] is None or h["parent"]["word"] >= 0


def restate_stream(em, nodes, lm, o, script, st=None):
    """One stream: em [T, N] float32, script a list of ("c", n) / ("b", look_back) / ("p", look_back).
    -> (bests [(score, am, lm, tokens, words) or None], frames in buffer after each prune, final, rows per frame
        [(src, edge, state)])"""
    st = st if st is not None else Stats()
    sil, lmw = o["sil"], o["lmw"]
    buf = S0.StreamBuffer(dict(score=0.0, am=0.0, lm=0.0, state=lm.start(), node=0, token=sil, word=-1, pb=False,
                               parent=None), _complete, lexicon=True)
    bests, frames, rows, at = [], [], [], 0
    for i, (op, v) in enumerate(script):
        if op == "c":
            for t in range(at, at + v):
                buf.hyp.append(lex_frame(buf.hyp[-1], em[t], nodes, lm, o, st, t))
                rows.append([(c["src"], c["edge"], c["state"]) for c in buf.hyp[-1]])
            at += v
        elif op == "b":
            bests.append(buf.best(v, st, ("best", i)))
        else:
            buf.prune(v, st, ("prune", i))
            frames.append(buf.frames_in_buffer)
    assert at == len(em)
    beam = buf.hyp[-1]
    nice = any(h["node"] == 0 for h in beam)
    cands = []
    for h in beam:
        if nice and h["node"] != 0:
            continue
        state, l = lm.finish(h["state"])
        score = h["score"] + lmw * l
        if not math.isnan(score):
            cands.append(dict(score=score, am=h["am"], lm=h["lm"] + l, key=(state, h["node"], sil, False), token=sil,
                              word=-1, parent=h))
    final = [S0.hypothesis(c, len(buf.hyp)) for c in C0._store(cands, o["K"], o["thr"], o["log_add"], st, "end")]
    if len(buf.hyp) < 1:  # (getAllFinalHypothesis returns nothing before the first frame: never so after decodeEnd)
        final = []
    return bests, frames, final, rows


def shows(need, st):
    """what a fixture's case is there to show, counted by the restatement's findBestAncestor"""
    return all(getattr(st, nd, 0) >= 1 for nd in filter(None, need.split(",")))


# ---- fixtures of the reference itself -----------------------------------------------------------------------------------
def _golden():
    path = os.path.join(ROOT, "tests", "golden", "lex_ctc_lm_rows_stream_expected.json.gz")
    if not os.path.exists(path):  # (the generator imports this module before it has written the file; the coverage test
        return []                 # below fails on an empty list)
    with gzip.open(path, "rt") as f:
        return json.load(f)


def case_opts(c):
    return opts(c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["unk_score"], c["sil_score"], c["sil"],
                c["blank"], c["unk"], c["log_add"], bool(c["is_lm_token"]))


_NODES = {}


def case_nodes(c):
    """the restatement's trie of a case, through the emulator library's host trie (smeared for the word LM)"""
    key = (c["lexname"], c["N"], c["sil"], c["is_lm_token"])
    if key not in _NODES:
        lib = _capi.Lib(os.path.join(ROOT, "tests", "emu", "libfltx_emu.so"))
        lx = Lex(lib, c["N"], c["sil"], c["lex"], 0 if c["is_lm_token"] else SMEAR_MAX)
        _NODES[key] = lx.nodes
        lx.close()
    return _NODES[key]


def case_restate(c, b, st):
    rl = GS.case_lm(c, b)
    lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
    return restate_stream(GS.emissions(c, b), case_nodes(c), lm, case_opts(c), GS.stream_script(c, b), st=st)


def assert_case(c, b, got, what):
    """got = (bests, frames, final) of stream b against the fixture"""
    want = c["streams"][b]
    assert len(got[0]) == len(want["best"]) and got[1] == want["frames"], (what, got[1], want["frames"])
    for i, (w, g) in enumerate(zip(want["best"], got[0])):
        S0.assert_best(None if w is None else tuple(w), g, c["log_add"], (what, "best", i), final=assert_final)
    assert_final([tuple(h) for h in want["final"]], got[2], c["log_add"], what)


def test_fixtures_cover_the_cases():
    cs = {c["name"]: c for c in _golden()}
    assert list(cs) == [c["name"] for c in GS.all_cases()]
    ops = [op for c in cs.values() for op in c["ops"]]
    assert {v for op, v in ops if op == "p"} >= {0, 2} and {v for op, v in ops if op == "b"} >= {0, 1, 99}
    assert any(c["log_add"] for c in cs.values()) and any(c["is_lm_token"] for c in cs.values())
    assert any(0 in v for op, v in ops if op == "c") and any(len(c["Ts"]) == 3 for c in cs.values())
    assert any(w is None for c in cs.values() for s in c["streams"] for w in s["best"])
    assert any(w >= 0 for c in cs.values() for s in c["streams"] for h in s["best"] if h for w in h[4])
    assert cs["word_inside_word"]["need"] == "extended"
    h = cs["word_hold_limit"]
    assert (h["N"], h["K"], h["Ts"], h["max_frames"], h["need"]) == (4, 2, [115], 8, "limited")
    # the walk's limit is what pruned: look_back + 100 frames and the buffer's first stay (the ring has 110 rows)
    assert h["streams"][0]["frames"][:20] == list(range(6, 106, 5)) and h["streams"][0]["frames"][20:] == [103, 103, 103]
    assert all(len(x[3]) == 1 for x in h["streams"][0]["best"][20:])
    for c in cs.values():
        if c["name"] != "word_hold_limit":
            assert all(T <= 40 for T in c["Ts"]) and c["N"] <= 6 and c["K"] <= 8


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c):
    for b in range(len(c["Ts"])):
        st = Stats()
        bests, frames, final, _ = case_restate(c, b, st)
        assert not st.ties and (not c["log_add"] or st.gap > MIN_GAP), (st.ties, st.gap)
        assert shows(c["need"], st), c["need"]
        assert_case(c, b, (bests, frames, final), (c["name"], b))


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess):
    B, o = len(c["Ts"]), case_opts(c)
    rls = [GS.case_lm(c, b) for b in range(B)]
    lx = Lex(sess.lib, c["N"], c["sil"], c["lex"], 0 if c["is_lm_token"] else SMEAR_MAX)
    lm = dev_lm(sess, rls[0], o, mapped=bool(c["perm"]))
    dec = make_dec(sess, lx, lm, o)
    ems = [GS.emissions(c, b) for b in range(B)]
    got, _ = S0.run_script(sess, dec, ems, c["N"], c["W"], lambda b, p: rls[b].row(list(p)),
                           [tuple(x) for x in c["ops"]], c["max_frames"], lexicon=True)
    for b in range(B):
        assert_case(c, b, got[b], (c["name"], b))
    for d in (dec, lm, lx):
        d.close()


# ---- a stream without prunes is the offline decode ----------------------------------------------------------------------
@pytest.mark.parametrize("tokl", [False, True], ids=["word_lm", "token_lm"])
@pytest.mark.parametrize("log_add", [False, True])
def test_stream_equals_offline(sess, tokl, log_add):
    """The same emissions cut into unequal chunks per stream, no prune; stream 1 gets an empty chunk while the others
    advance: the n-best after end and the row lists of every frame are those of fltx_ctc_rows_begin / step / end."""
    N, Ts = 6, (11, 7, 4)
    lex = [(lab, sc, toks) for lab, sc, toks in GS.LEX["b" if tokl else "a"]]
    o = opts(6, N, 25.0, 0.7, 0.25, NINF, -0.3, 0, 1, -1, log_add, tokl)
    W = 8
    ems = [GS._emissions(1500 + b, T, N) for b, T in enumerate(Ts)]
    rl = GS.GL.SmRowsLM(93, N if tokl else 6, W, 43, W - 1, 0)
    lx = Lex(sess.lib, N, 0, lex, 0 if tokl else SMEAR_MAX)
    lm = dev_lm(sess, rl, o)

    def lm_row(b, p):
        return rl.row(list(p))
    off = make_dec(sess, lx, lm, o)
    want, want_rows, want_prefix = L0.decode(sess, off, ems, N, W, lm_row)
    off.close()
    dec = make_dec(sess, lx, lm, o)
    ops = [("c", [3, 0, 4]), ("c", [5, 2, 0]), ("b", 0), ("c", [0, 5, 0]), ("c", [3, 0, 0])]
    got, ds = S0.run_script(sess, dec, ems, N, W, lm_row, ops, 16, lexicon=True)
    for b in range(len(Ts)):
        assert len(got[b][2]) == len(want[b]) and len(want[b]) >= 1
        for w, g in zip(want[b], got[b][2]):
            assert g[3] == w[3] and g[4] == w[4] and _bits_equal(g[:3], w[:3]), (b, g, w)
        assert len(ds.rows[b]) == Ts[b] == len(want_rows[b])
        for t, (wr, gr) in enumerate(zip(want_rows[b], ds.rows[b])):
            assert [x[:2] for x in gr] == [x[:2] for x in wr], (b, t)
            assert [ds.prefix[b][x[2]] for x in gr] == [want_prefix[b][x[2]] for x in wr], (b, t)
    for d in (dec, lm, lx):
        d.close()


# ---- the buffer's bound -------------------------------------------------------------------------------------------------
def test_lexicon_stream_holds_a_hundred_frames_more(sess):
    """max_frames 4 on the lexicon kind: 104 frames fit (kLookBackLimit on top), the 105th does not; after prune(1) the
    host's bound is look_back + 100, and the device's count is asked only when that would not fit"""
    N, K = 6, 2
    o = opts(K, N, 25.0, 0.7, 0.25, NINF, 0.0, 0, 1, -1, False, False)
    lx = Lex(sess.lib, N, 0, GS.LEX["a"], SMEAR_MAX)
    lm = _capi.WordRowsLM(7, None, 6, lib=sess.lib)
    dec = make_dec(sess, lx, lm, o)
    dec.stream_begin(1, N, 4)
    lr = _dev(sess, np.zeros((K, 7), np.float32))
    em = GS._emissions(1600, 104, N)
    for _ in range(dec.append(em, [104])):
        dec.step(lr)
    assert dec.frames_in_buffer(0) == 105
    with pytest.raises(IndexError) as e:  # (FLTX_ERR_RANGE)
        dec.append(em[:1], [1])
    assert "104 buffered + 1 new frames exceed max_frames 4 + 100" in str(e.value)
    dec.prune(1)
    n = dec.frames_in_buffer(0)
    assert 2 <= n <= 102
    with pytest.raises(IndexError):
        dec.append(em[:106 - n], [106 - n])  # (one more than fits: the bound 101 + 5 would, so the device's count decides)
    assert dec.append(em[:105 - n], [105 - n]) == 105 - n
    dec.close()
    lm.close()
    lx.close()


# ---- the Python helper ------------------------------------------------------------------------------------------------
def test_python_helper_on_a_toy_word_lm(sess):
    """decode_stream with a callable word LM: asked once per state id, with (b, prefix, parent id, edge, id); against the
    restatement"""
    N, K, W, lb = 6, 6, 7, 2
    o = opts(K, N, 25.0, 0.7, 0.25, NINF, 0.0, 0, 1, -1, False, False)
    rl = GS.GL.SmRowsLM(23, 6, W, 0, W - 1, 0)
    lx = Lex(sess.lib, N, 0, GS.LEX["a"], SMEAR_MAX)
    Ts, cuts = (9, 5), [(4, 0), (2, 3), (3, 2)]
    ems, want = [], []
    for b, T in enumerate(Ts):
        script = [x for c in cuts for x in (("c", c[b]), ("p", lb), ("b", 0))]
        for seed in range(1700 + 50 * b, 1800 + 50 * b):
            st = Stats()
            em = GS._emissions(seed, T, N)
            res = restate_stream(em, lx.nodes, PrefixLM(lambda p: rl.row(list(p)), np.arange(6), W - 1), o, script, st=st)
            if not st.ties:
                break
        assert not st.ties
        ems.append(em)
        want.append(res)
    lm = _capi.WordRowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lx, lm, o)
    asked = []

    def lm_rows(keys):
        asked.extend(keys)
        return _dev(sess, np.stack([rl.row(list(k[1])) for k in keys]))
    at, chunks = [0, 0], []
    for c in cuts:
        chunks.append((np.concatenate([ems[b][at[b]:at[b] + c[b]].reshape(-1) for b in range(2)]), list(c)))
        at = [a + x for a, x in zip(at, c)]
    outs = list(dec.decode_stream(chunks, lm_rows, look_back=lb, N=N, max_frames=8))
    assert len(outs) == len(cuts) + 1 and len({(k[0], k[4]) for k in asked}) == len(asked)
    for b in range(2):
        for i in range(len(cuts)):
            h = outs[i][b]
            got = None if len(h.tokens) == 0 else (h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist())
            S0.assert_best(want[b][0][i], got, False, (b, i), final=assert_final)
        assert_final(want[b][2], [(h.score, h.am, h.lm, list(h.tokens), list(h.words)) for h in outs[-1][b]], False, b)
    for d in (dec, lm, lx):
        d.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_CTC_LMROWS_STREAM_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
