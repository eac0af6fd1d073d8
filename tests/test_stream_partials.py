"""fltx_stream_partials (text_amd/csrc/fltx_stream_partials.h): the partial transcript of every stream in one call, and
how much of it can no longer change.

The checks: the classic streams (lexicon-free / lexicon decoder) against one oracle decoder per stream -- the rows of
getBestHypothesis(look_back) after the collapse restated below in NumPy, scores, lengths, the frames pruned, the stable
prefix against the common prefix of the oracle's current beam, and over the whole run that nothing reported stable ever
changes; the CTC rows streams against the float64 restatement of tests/test_ctc_lm_rows_stream.py /
tests/test_lexicon_ctc_lm_rows_stream.py, the stable prefix against the convergence frame of the restatement's node
objects; the edges (a beam of one, a set over two 64-bit words, no frames yet, look_back beyond the buffer, a buffer
longer than the kernel's LDS window, device mode); the contract.

Every scenario runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_STREAM_PARTIALS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

import cases  # noqa: E402
import helpers  # noqa: E402
import stream_scenarios as ss  # noqa: E402
from oracle import orclib  # noqa: E402
from text_amd import _capi, synth  # noqa: E402
from golden import make_ctc_lm_rows_golden as G  # noqa: E402
import test_ctc_lm_rows_stream as S0  # noqa: E402
import test_lexicon_ctc_lm_rows_stream as S1  # noqa: E402
from test_ctc_lm_rows import PrefixLM, Stats, _dev, make_dec  # noqa: E402
from test_lexicon_ctc_lm_rows import SMEAR_MAX, Lex, dev_lm  # noqa: E402
from test_lexicon_ctc_lm_rows import make_dec as make_lex_dec  # noqa: E402
from test_seq2seq_model_output import _bits_equal, _GpuSess, is_gpu  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]


@pytest.fixture(scope="module")
def gpu_sess(gpu_session):
    return _GpuSess(gpu_session)


@pytest.fixture(params=BACKENDS)
def sess(request):
    """the rows decoders' session: the emulator's, or a context on a torch stream"""
    if request.param == "emu":
        return request.getfixturevalue("emu_session")
    import torch
    g = request.getfixturevalue("gpu_sess")
    torch.cuda.set_stream(g.stream)
    return g


@pytest.fixture(params=BACKENDS)
def csess(request):
    """the classic decoders' session (helpers.FltxSession)"""
    return request.getfixturevalue("emu_session" if request.param == "emu" else "gpu_session")


@pytest.fixture(params=BACKENDS)
def both(request):
    """(the classic decoders' session, the rows decoders' session) of one backend"""
    if request.param == "emu":
        e = request.getfixturevalue("emu_session")
        return e, e
    import torch
    g = request.getfixturevalue("gpu_sess")
    torch.cuda.set_stream(g.stream)
    return request.getfixturevalue("gpu_session"), g


# ---- the rule of include/fltx.h above fltx_transcripts, restated -----------------------------------------------------------
def collapse(tok, wrd, blank):
    """-> tokens, timesteps, words, word_timesteps, word_tok_end of one frame row"""
    tok, wrd = np.asarray(tok, np.int32), np.asarray(wrd, np.int32)
    keep = (tok >= 0) & (tok != blank) & np.r_[True, tok[1:] != tok[:-1]][:len(tok)]
    wi = np.flatnonzero(wrd >= 0)
    return tok[keep], np.flatnonzero(keep), wrd[wi], wi, np.cumsum(keep)[wi]


KEYS = ("tokens", "timesteps", "words", "word_timesteps", "word_tok_end")


def row_of(p, b):
    to, wo = p["tok_off"], p["word_off"]
    return [p[k][int(to[b]):int(to[b + 1])].tolist() for k in KEYS[:2]] + \
        [p[k][int(wo[b]):int(wo[b + 1])].tolist() for k in KEYS[2:]]


def assert_row(p, b, tok, wrd, blank, what):
    """row b of a stream_partials() dict is the collapse of the frame row (tok, wrd); its stable counts follow"""
    want = collapse(tok, wrd, blank)
    assert row_of(p, b) == [w.tolist() for w in want], what
    assert int(p["length"][b]) == len(tok), what
    lim = min(int(p["stable_frames"][b]), len(tok))
    assert int(p["stable_tokens"][b]) == int((want[1] < lim).sum()), what
    assert int(p["stable_words"][b]) == int((want[3] < lim).sum()), what


def common_prefix(hyps):
    """leading entries on which the (token, word) frame rows of all hypotheses agree"""
    rows = [list(zip(h.tokens.tolist(), h.words.tolist())) for h in hyps]
    n = 0
    while rows and all(len(r) > n for r in rows) and all(r[n] == rows[0][n] for r in rows):
        n += 1
    return n


class Committed:
    """what a stream has reported stable, by absolute entry: nothing that comes later may disagree"""

    def __init__(self):
        self.at = {}

    def check(self, first, tok, wrd, what):
        for i, e in enumerate(zip(tok, wrd)):
            assert self.at.get(first + i, e) == e, (what, first + i, self.at.get(first + i), e)

    def commit(self, first, tok, wrd, n):
        for i in range(min(n, len(tok))):
            self.at[first + i] = (tok[i], wrd[i])


def blank_of(c):
    return c["N"] - 1 if c["crit"] == "ctc" else -1


# ---- 1. + 2. the classic streams against one oracle per stream ---------------------------------------------------------------
CLASSIC = ["lf_ctc_t60_k10", "ng_tok_lexfree_t40", "lx_spell_t60_k12_full", "ng_word_t60_k16_4g", "lf_asg_t40_n29_kt7"]


@pytest.mark.parametrize("name", CLASSIC)
def test_classic_streams_against_the_oracle(csess, oracle_lib, name):
    """The ragged four-stream plan of tests/test_streaming.py (chunks of length 0 among them, prune(1) after the third
    call).  After every call, for look_back 0 and 2: row, scores and length of every stream are the oracle's
    best(look_back) after the collapse, fltx_result_best says the same before and after, first_frame is what the oracle
    pruned; stable_frames is the common prefix of the oracle's current beam (no larger after a prune); and whatever a
    stream reported stable stays in every later row and in the final n-best."""
    c = cases.BY_NAME[name]
    inp = helpers.case_inputs(c)
    N, B, blank = c["N"], 4, blank_of(c)
    Ts = [c["T"], c["T"] // 2, 7, c["T"] - 3]
    lex = inp["lex"] if c["dist"] == "lexspell" else None
    es = [synth.emissions(c["dist"], 900 + b, Ts[b], N, lexicon=lex) for b in range(B)]
    plan = [[5, 0, 3, 9], [7, 11, 0, 1], [0, 4, 4, 20], [30, 30, 30, 30], [100, 100, 100, 100]]
    ods = [ss.checker_decoder(oracle_lib, c, inp)[0] for _ in range(B)]
    for od in ods:
        oracle_lib.decoder_begin(od)
    d = csess.decoder(c, inp)
    d.stream_begin(B, N, max(Ts) + 4)
    done, pruned, cap = [0] * B, False, max(Ts) + 8
    com = [Committed() for _ in range(B)]
    for step, row in enumerate([[0] * B] + plan):  # (the first look: no frames yet)
        take = [min(row[b], Ts[b] - done[b]) for b in range(B)]
        parts = [es[b][done[b]:done[b] + take[b]] for b in range(B)]
        if step:
            flat = np.concatenate([p.reshape(-1) for p in parts]) if sum(take) else np.zeros(1, np.float32)
            d.stream_step(flat.astype(np.float32), take)
        for b in range(B):
            if take[b]:
                oracle_lib.decoder_step(ods[b], orclib._fp(np.ascontiguousarray(parts[b])), take[b], N)
            done[b] += take[b]
        for lb in (0, 2):
            before = [d.best(b, lb, cap) for b in range(B)]
            p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.stream_partials(lb).items()}
            assert p["n_rows"] == B and (p["status"] == 0).all()
            for b in range(B):
                what = (name, "call", step, "look_back", lb, "stream", b)
                want = oracle_lib.best(ods[b], lb, cap)
                assert_row(p, b, want.tokens, want.words, blank, what)
                if len(want.tokens):
                    assert _bits_equal(p["scores"][b], [want.score, want.am, want.lm]), what
                in_buf = oracle_lib.decoder_n_frames_in_buffer(ods[b])
                assert int(p["first_frame"][b]) == done[b] + 1 - in_buf, what
                for h in (before[b], d.best(b, lb, cap)):
                    assert ss._enc_one(h) == ss._enc_one(want), what
                hyps = oracle_lib.collect(ods[b])
                assert sum(oracle_lib.ties(ods[b]).values()) == 0, what
                lcp = common_prefix(hyps) if hyps else None
                stable = int(p["stable_frames"][b])
                assert 0 <= stable <= in_buf, what
                if lcp is not None:  # (a lexicon decoder lists nothing before its first frame)
                    assert stable <= lcp and (pruned or stable == lcp), (what, stable, lcp)
                if len(hyps) == 1:
                    assert stable == in_buf, what
                first = int(p["first_frame"][b])
                com[b].check(first, want.tokens.tolist(), want.words.tolist(), what)
                for h in hyps:
                    com[b].check(first, h.tokens.tolist(), h.words.tolist(), what + ("beam",))
                if lb == 0 and hyps:  # (any hypothesis of the beam spells the stable entries)
                    com[b].commit(first, hyps[0].tokens.tolist(), hyps[0].words.tolist(), stable)
        if step == 3:
            d.stream_prune(1)
            for od in ods:
                oracle_lib.decoder_prune(od, 1)
            pruned = True
    first = [int(x) for x in d.stream_partials(0)["first_frame"]]
    # (a lexicon stream prunes back to a complete hypothesis, or not at all: the oracle's count above is the check)
    assert (any(first) or c["kind"] == "lexicon") and any(len(cm.at) > 1 for cm in com)
    d.stream_end()
    for b in range(B):
        oracle_lib.decoder_end(ods[b])
        final = oracle_lib.collect(ods[b])
        ok, why = helpers.hyps_equal(final, d.results(b))
        assert ok, "stream %d: %s" % (b, why)
        for h in final:
            com[b].check(first[b], h.tokens.tolist(), h.words.tolist(), (name, "final", b))
        oracle_lib.decoder_destroy(ods[b])
    d.close()


# ---- 3. the rows streams against the restatement --------------------------------------------------------------------------
def convergence(buf):
    """stable_frames of a restated stream (S0.StreamBuffer): 1 + the last buffer frame at which the current beam's
    ancestors are one node"""
    nodes = {id(h): h for h in buf.hyp[-1]}
    for j in range(len(buf.hyp) - 1, -1, -1):
        if len(nodes) == 1:
            return j + 1
        if j == 0 or not nodes:
            return 0
        nodes = {id(h["parent"]): h["parent"] for h in nodes.values()}
    return 0


def _golden_case(mod, lexicon):
    """a reference fixture's decoder, emissions and LMs on three streams, and the script (the lexicon-free fixture's own
    prunes nothing; the lexicon fixture whose prune drops frames -- a word ends inside the buffer -- has one stream: here
    three streams take its emissions in chunks of their own)"""
    if not lexicon:
        c = {c["name"]: c for c in mod._golden()}["chunks_best"]
        script = [("c", [3, 2, 0]), ("p", 1), ("c", [4, 0, 3]), ("p", 2), ("c", [2, 5, 2]), ("p", 0)]
    else:
        c = dict({c["name"]: c for c in mod._golden()}["word_inside_word"])
        c["Ts"], c["seeds"] = [14, 14, 14], [c["seeds"][0]] * 3
        script = [("c", [5, 3, 4]), ("p", 1), ("c", [4, 6, 5]), ("p", 2), ("c", [5, 5, 5]), ("p", 0)]
    assert len(c["Ts"]) == 3 and not c["log_add"]
    assert [sum(v[b] for op, v in script if op == "c") for b in range(3)] == c["Ts"]
    return c, script


@pytest.mark.parametrize("lexicon", [False, True], ids=["lexfree", "lexicon"])
def test_rows_streams_against_the_restatement(sess, lexicon):
    """A script of append / step / prune on the three streams of a reference fixture, with unequal chunks; after every
    operation, for look_back 0 and 2: row, scores and length against the restatement's best, stable_frames exactly
    the convergence frame of its node objects, before and after prunes, first_frame the frames it dropped."""
    mod = S1 if lexicon else S0
    c, script = _golden_case(mod, lexicon)
    B, N, W = len(c["Ts"]), c["N"], c["W"]
    if lexicon:
        o = S1.case_opts(c)
        rls = [S1.GS.case_lm(c, b) for b in range(B)]
        lx = Lex(sess.lib, N, c["sil"], c["lex"], 0 if c["is_lm_token"] else SMEAR_MAX)
        lm = dev_lm(sess, rls[0], o, mapped=bool(c["perm"]))
        dec = make_lex_dec(sess, lx, lm, o)
        ems = [S1.GS.emissions(c, b) for b in range(B)]
        nodes = lx.nodes  # (the restatement's trie, through this library's host trie)
        plms = [PrefixLM(lambda p, rl=rl: rl.row(list(p)), rl.usr_to_lm, rl.finish) for rl in rls]
        bufs = [S0.StreamBuffer(dict(score=0.0, am=0.0, lm=0.0, state=plms[b].start(), node=0, token=c["sil"], word=-1,
                                     pb=False, parent=None), S1._complete, lexicon=True) for b in range(B)]

        def frame(b, e, st, t):
            return S1.lex_frame(bufs[b].hyp[-1], e, nodes, plms[b], o, st, t)
    else:
        rls = [S0._case_lm(c, b) for b in range(B)]
        lm = _capi.RowsLM(W, rls[0].usr_to_lm if c["perm"] else None, W - 1, lib=sess.lib)
        dec = make_dec(sess, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"], c["sil"], c["blank"], c["log_add"])
        ems = [G.emissions(c["seeds"][b], c["Ts"][b], N) for b in range(B)]
        plms = [PrefixLM(lambda p, rl=rl: rl.row(list(p)), rl.usr_to_lm, rl.finish) for rl in rls]
        bufs = [S0.StreamBuffer(dict(score=0.0, am=0.0, lm=0.0, state=plms[b].start(), token=c["sil"], pb=False,
                                     parent=None)) for b in range(B)]

        def frame(b, e, st, t):
            return S0.ctc_frame(bufs[b].hyp[-1], e, plms[b], c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"], c["sil"],
                                c["blank"], c["log_add"], st, t)
    ds = S0.DeviceStreams(sess, dec, B, N, W, lambda b, p: rls[b].row(list(p)), c["max_frames"], lexicon)
    st = Stats()
    at, dropped, prunes = [0] * B, [0] * B, 0

    def look(what):
        for lb in (0, 2):
            p = dec.stream_partials(lb)
            assert (p["status"] == 0).all()
            for b in range(B):
                r = bufs[b].best(lb, st, what)
                tok, wrd = ([], []) if r is None else (r[3], r[4] if lexicon else [-1] * len(r[3]))
                assert_row(p, b, tok, wrd, c["blank"], (what, lb, b))
                if r is not None:
                    assert _bits_equal(p["scores"][b], r[:3]), (what, lb, b)
                assert int(p["stable_frames"][b]) == convergence(bufs[b]), (what, lb, b)
                assert int(p["first_frame"][b]) == dropped[b], (what, lb, b)
    look("begin")
    for i, (op, v) in enumerate(script):
        if op == "c":
            ds.chunk([ems[b][at[b]:at[b] + v[b]] for b in range(B)])
            for b in range(B):
                for t in range(at[b], at[b] + v[b]):
                    bufs[b].hyp.append(frame(b, ems[b][t], st, t))
                at[b] += v[b]
        elif op == "p":
            dec.prune(v)
            for b in range(B):
                n = bufs[b].frames_in_buffer
                bufs[b].prune(v, st, ("prune", i))
                dropped[b] += n - bufs[b].frames_in_buffer
            prunes += 1
        else:
            continue
        look((op, i))
    assert not st.ties and prunes and any(dropped)
    ds.end()
    for x in (dec, lm) + ((lx,) if lexicon else ()):
        x.close()


def test_rows_stream_that_stopped(sess):
    """tests/test_ctc_lm_rows_stream.py's stopped stream: stream 0 ran out of LM states, stream 1 goes on"""
    N, K, W, sil, blank = 4, 6, 4, 0, 1
    flat = np.full((1, N), -5.0, np.float32)
    flat[0, blank] = 0.0
    ems = [G.emissions(800, 9, N) * np.float32(0.25), np.repeat(flat, 9, axis=0)]
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 2.0, 0.7, 0.0, sil, blank, False)
    dec.set_max_states(4)
    dec.stream_begin(2, N, 6)
    lr = _dev(sess, np.zeros((2 * K, W), np.float32))
    at = 0
    for T in (3, 3, 3):
        for _ in range(dec.append(np.concatenate([e[at:at + T].reshape(-1) for e in ems]), [T, T])):
            dec.step(lr)
        at += T
        dec.prune(1)
        p = dec.stream_partials(0)
        assert int(p["status"][0]) == _capi.ERR_UNSUPPORTED and int(p["length"][0]) == 0 and not row_of(p, 0)[0]
        assert int(p["status"][1]) == 0 and int(p["length"][1]) == 2 and int(p["first_frame"][1]) == at - 1
        assert row_of(p, 1) == [[], [], [], [], []] and p["scores"][1, 0] == 0.0  # (two blanks)
        assert 0 <= int(p["stable_frames"][1]) <= 2
    dec.close()
    lm.close()


# ---- 4. edges -----------------------------------------------------------------------------------------------------------
def _stream(csess, c, chunks, sets=()):
    inp = helpers.case_inputs(c)
    d = csess.decoder(c, inp)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(1, c["N"], c["T"] + 4)
    t = 0
    for ch in chunks:
        d.stream_step(np.ascontiguousarray(inp["e"][t:t + ch]), [ch])
        t += ch
    return d


def _check_against_best(d, look_backs, blank, cap):
    out = []
    for lb in look_backs:
        p = d.stream_partials(lb)
        h = d.best(0, lb, cap)
        assert_row(p, 0, h.tokens, h.words, blank, lb)
        if len(h.tokens):
            assert _bits_equal(p["scores"][0], [h.score, h.am, h.lm])
        out.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()})
    return out


def test_a_beam_of_one_is_stable_throughout(csess):
    c = cases.BY_NAME["lf_ctc_k1"]
    d = _stream(csess, c, [11, 8])
    for p in _check_against_best(d, (0, 3), blank_of(c), 64):
        assert int(p["stable_frames"][0]) == d.frames_in_buffer(0) == 20
    d.stream_prune(4)
    p = d.stream_partials(0)
    assert int(p["stable_frames"][0]) == d.frames_in_buffer(0) == 5 and int(p["first_frame"][0]) == 15
    d.close()


def test_a_beam_over_two_set_words(csess, oracle_lib):
    """K = 100 at N = 12, T = 40 on the generic engine: the ancestor set spans two 64-bit words"""
    c = cases.case("sp_k100", dist="ctc", T=40, N=12, K=100, u=77)
    inp = helpers.case_inputs(c)
    od = ss.checker_decoder(oracle_lib, c, inp)[0]
    oracle_lib.decoder_begin(od)
    d = _stream(csess, c, [], (("lane", 0), ("slane", 0), ("lean", 0)))
    seen = set()
    for t in range(0, 40, 8):
        d.stream_step(np.ascontiguousarray(inp["e"][t:t + 8]), [8])
        oracle_lib.decoder_step(od, orclib._fp(np.ascontiguousarray(inp["e"][t:t + 8])), 8, 12)
        hyps = oracle_lib.collect(od)
        assert len(hyps) > 64 and sum(oracle_lib.ties(od).values()) == 0
        p = _check_against_best(d, (0,), blank_of(c), 64)[0]
        assert int(p["stable_frames"][0]) == common_prefix(hyps)
        seen.add(len(hyps))
    assert max(seen) == 100  # (a hundred paths that part at the first frame: the walk goes all the way down)
    oracle_lib.decoder_destroy(od)
    d.close()


@pytest.mark.parametrize("name", ["lf_ctc_t20_k4", "lx_spell_t40_k8"])
def test_a_stream_without_frames_and_a_long_look_back(csess, name):
    """no frames yet: the root's sil for the lexicon-free kind, an empty result for the lexicon kind; look_back beyond
    the buffer: what fltx_result_best says (nothing)"""
    c = cases.BY_NAME[name]
    d = _stream(csess, c, [])
    p = d.stream_partials(0)
    lexicon = c["kind"] == "lexicon"
    assert row_of(p, 0)[:2] == ([[], []] if lexicon else [[0], [0]]) and int(p["length"][0]) == (0 if lexicon else 1)
    assert int(p["stable_frames"][0]) == 1 and int(p["first_frame"][0]) == 0 and int(p["status"][0]) == 0
    d.stream_step(np.ascontiguousarray(helpers.case_inputs(c)["e"][:9]), [9])
    for p in _check_against_best(d, (0, 9, 10, 500), blank_of(c), 64)[2:]:
        assert int(p["length"][0]) == 0 and int(p["n_tokens"]) == 0
    d.close()


def test_a_buffer_longer_than_the_staging_window(csess, oracle_lib):
    """K = 50: the kernel stages 81 history rows at a time; 200 frames without a prune take three windows"""
    c = cases.case("sp_t200_k50", T=200, K=50, u=3)
    inp = helpers.case_inputs(c)
    od = ss.checker_decoder(oracle_lib, c, inp)[0]
    oracle_lib.decoder_begin(od)
    oracle_lib.decoder_step(od, orclib._fp(np.ascontiguousarray(inp["e"])), 200, c["N"])
    d = _stream(csess, c, [120, 80])
    ps = _check_against_best(d, (0, 90, 170), blank_of(c), 256)
    assert [int(p["length"][0]) for p in ps] == [201, 111, 31]
    hyps = oracle_lib.collect(od)
    assert sum(oracle_lib.ties(od).values()) == 0
    assert int(ps[0]["stable_frames"][0]) == common_prefix(hyps) and len(hyps) > 1
    want = oracle_lib.best(od, 90, 256)
    assert_row(ps[1], 0, want.tokens, want.words, blank_of(c), "oracle")
    oracle_lib.decoder_destroy(od)
    d.close()


def _read(sess_, addr, ctype, n):
    """n elements at a device address (the emulator's device memory is host memory)"""
    out = np.zeros(n, np.dtype(ctype))
    if n == 0:
        return out
    if "emulation" in sess_.lib.version():
        ctypes.memmove(out.ctypes.data, addr, out.nbytes)
        return out
    hip = ctypes.CDLL("libamdhip64.so.7")  # (the runtime libfltx.so is linked against: already mapped)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    sess_.ctx.synchronize()
    assert hip.hipMemcpy(out.ctypes.data, addr, out.nbytes, 2) == 0
    return out


def test_device_mode_holds_what_host_mode_returns(csess):
    c = cases.BY_NAME["lx_spell_t60_k12_full"]
    d = _stream(csess, c, [25, 20])
    h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.stream_partials(1).items()}
    assert h["n_tokens"] > 0 and h["n_words"] > 0
    g = d.stream_partials(1, device=True)
    assert (g["n_rows"], g["n_tokens"], g["n_words"]) == (1, h["n_tokens"], h["n_words"])
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    sizes = {"tok_off": (i64, 2), "word_off": (i64, 2), "tokens": (i32, h["n_tokens"]), "timesteps": (i32, h["n_tokens"]),
             "words": (i32, h["n_words"]), "word_timesteps": (i32, h["n_words"]), "word_tok_end": (i32, h["n_words"]),
             "scores": (ctypes.c_double, 3), "length": (i32, 1), "stable_frames": (i32, 1), "stable_tokens": (i32, 1),
             "stable_words": (i32, 1), "status": (i32, 1), "first_frame": (i64, 1)}
    for k, (ct, n) in sizes.items():
        assert isinstance(g[k], int) and g[k], k
        got = _read(csess, g[k], ct, n)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(h[k]).reshape(-1).view(np.uint8)), k
    d.close()


# ---- 5. the contract -------------------------------------------------------------------------------------------------------
def test_contract_and_refusals(both):
    csess, sess = both
    L = csess.lib.lib
    I, S = _capi.ERR_INVALID, _capi.ERR_STATE
    out = _capi.StreamPartialsOut()
    c = cases.BY_NAME["lf_ctc_t60_k10"]
    inp = helpers.case_inputs(c)
    d = csess.decoder(c, inp)
    call = L.fltx_stream_partials
    assert call(None, 0, 0, ctypes.byref(out)) == I
    assert call(d.h, 0, 0, ctypes.byref(out)) == S                       # a fresh decoder
    d.decode_batch(inp["e"], [c["T"]], c["N"])
    assert call(d.h, 0, 0, ctypes.byref(out)) == S                       # an offline decode
    d.stream_begin(1, c["N"], 64)
    assert call(d.h, -1, 0, ctypes.byref(out)) == I and call(d.h, 0, 0, None) == I
    d.stream_step(np.ascontiguousarray(inp["e"][:30]), [30])
    # twice the same answer, in the same buffers; the views stay valid until the next step
    p = d.stream_partials(0)
    first = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    q = d.stream_partials(0)
    assert all(np.array_equal(first[k], q[k]) for k in first)
    assert [q[k].ctypes.data for k in KEYS[:2]] == [p[k].ctypes.data for k in KEYS[:2]]
    h = d.best(0, 0, 64)
    assert all(np.array_equal(first[k], p[k]) for k in first) and first["n_tokens"] > 0
    ps = d.stream_partials_batch(2)
    assert len(ps) == 1 and isinstance(ps[0], _capi.Partial) and ps[0].length == 29 and ps[0].status == 0
    want = collapse(d.best(0, 2, 64).tokens, d.best(0, 2, 64).words, blank_of(c))
    assert ps[0].tokens.tolist() == want[0].tolist() and ps[0].timesteps.tolist() == want[1].tolist()
    assert ps[0].first_frame == 0 and 0 <= ps[0].stable_tokens <= len(ps[0].tokens)
    d.stream_end()
    assert call(d.h, 0, 0, ctypes.byref(out)) == S                       # the stream is over
    d.close()
    # the seq2seq kinds; a rows decoder outside a stream and one begun with fltx_ctc_rows_begin
    Lr = sess.lib.lib
    s2s = _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(4, 4), sess.zero, 1, 5)
    assert Lr.fltx_stream_partials(s2s.h, 0, 0, ctypes.byref(out)) == S
    s2s.close()
    N, K = 6, 4
    lm = _capi.RowsLM(N + 1, None, N, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    assert Lr.fltx_stream_partials(dec.h, 0, 0, ctypes.byref(out)) == S
    dec.begin(G.emissions(900, 3, N), [3], N)
    assert Lr.fltx_stream_partials(dec.h, 0, 0, ctypes.byref(out)) == S
    dec.stream_begin(1, N, 4)
    assert Lr.fltx_stream_partials(dec.h, -1, 0, ctypes.byref(out)) == I
    assert Lr.fltx_stream_partials(dec.h, 0, 0, ctypes.byref(out)) == 0 and out.t.n_rows == 1
    dec.close()
    lm.close()


@pytest.mark.parametrize("name", ["lx_spell_t60_k12_full"])
def test_a_stream_that_never_asks_traces_as_before(csess, oracle_lib, name):
    """the prune operation's new counter changes nothing a stream returns: the scenario of tests/test_streaming.py"""
    c = cases.BY_NAME[name]
    inp = helpers.case_inputs(c)
    chunks, lbs = ss.SCENARIOS[name]
    want = ss.trace_checker(oracle_lib, c, inp, chunks, lbs)
    got, _ = ss.trace_device(csess, c, inp, chunks, lbs)
    assert ss.first_difference(want, got) is None


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_STREAM_PARTIALS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
