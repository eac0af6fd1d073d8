"""Streams on the lexicon-free CTC rows decoder (fltx_ctc_rows_stream_*, text_amd/csrc/fltx_ctc_rows_stream.h): decodeStep
on chunks as they arrive, getBestHypothesis(lookBack), prune(lookBack), a bounded history ring.

The checks: a stream without prunes against the offline begin / step / end on the same emissions, bit for bit, row lists
included; the compiled reference's fixtures (tests/golden/make_ctc_lm_rows_stream_golden.py: scripts of chunks, best and
prune calls -- the float64 restatement below reproduces them, the device reproduces them: tokens exact, the three scores
bit-identical under max-merge and within 1e-5 under logAdd); the ring's wrap; a beam wider than a wave; a stream that
stops on a full LM-state table beside one that goes on; the ABI's contract and refusals; the Python helper.

The restatement (`restate_stream`) is tests/test_ctc_lm_rows.py's search (its `_store`, `PrefixLM`, `Stats`) on a buffer of
beams whose hypotheses point at their parents, with the reference's findBestAncestor and pruneAndNormalize (Utils.h:
268-342).  It counts its own ties -- the search's, and equal scores at the first best of a best or prune call.

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

CHILD = os.environ.get("FLTX_CTC_LMROWS_STREAM_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
from golden import make_ctc_lm_rows_golden as G  # noqa: E402
from golden import make_ctc_lm_rows_stream_golden as GS  # noqa: E402
from test_ctc_lm_rows import (LOGADD_TOL, MIN_GAP, PrefixLM, Stats, _dev, _store, assert_final, assert_rows,  # noqa: E402
                              decode, make_dec)
from test_seq2seq_model_output import _bits_equal, _GpuSess, _np, is_gpu  # noqa: E402

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
def find_best_ancestor(beam, look_back, complete, st, where, limit=100):
    """findBestAncestor (Utils.h:268-310) -> (node or None, the updated look_back)"""
    if not beam:
        return None, look_back
    node = beam[0]
    for h in beam[1:]:
        if h["score"] == node["score"]:
            st.ties.append((where, "first best"))
        if h["score"] > node["score"]:
            node = h
    n = 0
    while node is not None and n < look_back:
        n += 1
        node = node["parent"]
    while node is not None:
        if complete(node):
            st.extended = getattr(st, "extended", 0) + (n > look_back)  # (the walk went on to the last word end)
            break
        n += 1
        node = node["parent"]
        if n == look_back + limit:
            st.limited = getattr(st, "limited", 0) + 1  # (look_back + kLookBackLimit steps ended it)
            break
    return node, n


def hypothesis(node, final_frame):
    """getHypothesis (Utils.h:229-250) -> (score, am, lm, tokens, words) or None"""
    if node is None:
        return None
    toks, words = [-1] * (final_frame + 1), [-1] * (final_frame + 1)
    res = (node["score"], node["am"], node["lm"], toks, words)
    i = 0
    while node is not None:
        toks[final_frame - i] = node["token"]
        words[final_frame - i] = node.get("word", -1)
        node = node["parent"]
        i += 1
    return res


class StreamBuffer:
    """hyp_ of a stream: the beams in the buffer, parents by reference; prune and best as the reference has them"""

    def __init__(self, root, complete=lambda h: True, lexicon=False):
        self.hyp, self.complete, self.lexicon = [[root]], complete, lexicon

    @property
    def frames_in_buffer(self):
        return len(self.hyp)

    def best(self, look_back, st, where):
        F = len(self.hyp) - 1
        if self.lexicon and F - look_back < 1:  # LexiconDecoder.cpp:286
            return None
        node, n = find_best_ancestor(self.hyp[F], look_back, self.complete, st, where)
        return hypothesis(node, F - n)

    def prune(self, look_back, st, where):
        F = len(self.hyp) - 1
        if F - look_back < 1:
            return
        node, n = find_best_ancestor(self.hyp[F], look_back, self.complete, st, where)
        if node is None or F - n < 1:
            return
        self.hyp = self.hyp[F - n:]
        for h in self.hyp[0]:
            h["parent"] = None
        largest = max(h["score"] for h in self.hyp[-1])
        for h in self.hyp[-1]:
            h["score"] -= largest


def ctc_frame(beam, e, lm, K, Kt, thr, lmw, sil_score, sil, blank, log_add, st, where):
    """one frame of tests/test_ctc_lm_rows.py's restate on a beam of parent-linked hypotheses -> the next beam"""
    N = len(e)
    order = sorted((n for n in range(N) if not np.isnan(e[n])), key=lambda n: (-float(e[n]), n))
    kt = min(Kt, N)
    if len(order) > kt and e[order[kt - 1]] == e[order[kt]]:
        st.ties.append((where, "token cut"))
    cands = []
    for i, h in enumerate(beam):
        for n in sorted(order[:kt]):
            a = float(e[n])
            score = h["score"] + a
            if n == sil:
                score += sil_score
            if n != blank and (n != h["token"] or h["pb"]):
                state, l = lm.score(h["state"], n)
                c = dict(score=score + lmw * l, am=h["am"] + a, lm=h["lm"] + l, state=state, token=n, pb=False, new=True)
            else:
                c = dict(score=score, am=h["am"] + a, lm=h["lm"], state=h["state"], token=n, pb=n == blank, new=False)
            if math.isnan(c["score"]):
                continue
            c.update(src=i, key=(c["state"], n, c["pb"]), parent=h)
            cands.append(c)
    return _store(cands, K, thr, log_add, st, where)


def restate_stream(em, lm, K, Kt, thr, lmw, sil_score, sil, blank, log_add, script, st=None):
    """One stream: em [T, N] float32, script a list of ("c", n) / ("b", look_back) / ("p", look_back).
    -> (bests [(score, am, lm, tokens) or None], frames in buffer after each prune, final [(score, am, lm, tokens)],
        rows per frame [(src, token, state)])"""
    st = st if st is not None else Stats()
    buf = StreamBuffer(dict(score=0.0, am=0.0, lm=0.0, state=lm.start(), token=sil, pb=False, parent=None))
    bests, frames, rows, at = [], [], [], 0
    for i, (op, v) in enumerate(script):
        if op == "c":
            for t in range(at, at + v):
                buf.hyp.append(ctc_frame(buf.hyp[-1], em[t], lm, K, Kt, thr, lmw, sil_score, sil, blank, log_add, st, t))
                rows.append([(c["src"], c["token"] if c["new"] else -1, c["state"]) for c in buf.hyp[-1]])
            at += v
        elif op == "b":
            r = buf.best(v, st, ("best", i))
            bests.append(None if r is None else r[:4])
        else:
            buf.prune(v, st, ("prune", i))
            frames.append(buf.frames_in_buffer)
    assert at == len(em)
    cands = []
    for h in buf.hyp[-1]:
        state, l = lm.finish(h["state"])
        score = h["score"] + lmw * l
        if not math.isnan(score):
            cands.append(dict(score=score, am=h["am"], lm=h["lm"] + l, key=(state, sil, False), token=sil, parent=h))
    final = []
    for c in _store(cands, K, thr, log_add, st, "end"):
        final.append(hypothesis(c, len(buf.hyp))[:4])
    return bests, frames, final, rows


# ---- the device loop ---------------------------------------------------------------------------------------------------
class DeviceStreams:
    """B streams on the device, one LM row per hypothesis: keeps the prefix of every state id and the row lists"""

    def __init__(self, sess, dec, B, N, W, lm_row, max_frames, lexicon=False):
        self.sess, self.dec, self.B, self.N, self.W, self.lm_row, self.lexicon = sess, dec, B, N, W, lm_row, lexicon
        self.K = int(dec.options.beam_size)
        self.prefix = [dict() for _ in range(B)]
        self.rows = [[] for _ in range(B)]
        self.prev_state = None
        self._take(dec.stream_begin(B, N, max_frames), [False] * B, first=True)

    def _take(self, out, stepped, first=False):
        """the row lists of a call; stepped[b]: stream b decoded a frame in it"""
        if is_gpu(self.sess):
            self.dec.ctx.synchronize()
        tok, src, state, n = [_np(a).copy() for a in out]
        B, K = self.B, self.K
        for b in range(B):
            nb = int(n[b])
            assert (tok[b, nb:] == -1).all() and (src[b, nb:] == -1).all() and (state[b, nb:] == -1).all(), b
            if first:
                assert (int(src[b, 0]), int(tok[b, 0]), int(state[b, 0]), nb) == \
                    (-1, -1 if self.lexicon else self.dec.sil, 0, 1)
                self.prefix[b][0] = ()
            elif stepped[b]:
                for k in range(nb):
                    sid, s = int(state[b, k]), int(src[b, k])
                    assert b * K <= s < b * K + K, (b, k, s)
                    par = int(self.prev_state[b, s - b * K])
                    p = self.prefix[b][par] + (int(tok[b, k]),) if tok[b, k] >= 0 else self.prefix[b][par]
                    assert tok[b, k] >= 0 or sid == par, (b, k)
                    assert self.prefix[b].setdefault(sid, p) == p, (b, k, "one id, two states")
                self.rows[b].append([(int(src[b, k]) - b * K, int(tok[b, k]), int(state[b, k])) for k in range(nb)])
            else:  # no frame of this stream: the beam listed again, unchanged
                assert (src[b, :nb] == b * K + np.arange(nb)).all() and (tok[b, :nb] == -1).all(), b
                assert (state[b, :nb] == self.prev_state[b, :nb]).all() and nb == int(self.prev_n[b]), b
        self.prev_state, self.prev_n = state, n

    def lm_rows(self):
        lr = np.full((self.B * self.K, self.W), np.nan, np.float32)
        for b in range(self.B):
            for k in range(int(self.prev_n[b])):
                lr[b * self.K + k] = self.lm_row(b, self.prefix[b][int(self.prev_state[b, k])])
        return _dev(self.sess, lr)

    def chunk(self, parts, extra_steps=0):
        """parts[b]: [T_b, N] float32 (T_b >= 0).  extra_steps: steps after the chunk is used up (they change nothing)"""
        Ts = [p.shape[0] for p in parts]
        flat = np.concatenate([p.reshape(-1) for p in parts]) if sum(Ts) else np.zeros(0, np.float32)
        steps = self.dec.append(flat, Ts)
        assert steps == max(Ts)
        for t in range(steps + extra_steps):
            self._take(self.dec.step(self.lm_rows()), [t < T for T in Ts])

    def best(self, b, look_back):
        h = self.dec.best(b, look_back)
        if len(h.tokens) == 0:
            return None
        return self._hyp(h)

    def _hyp(self, h):
        if self.lexicon:
            return (h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist())
        assert (h.words == -1).all()
        return (h.score, h.am, h.lm, h.tokens.tolist())

    def end(self):
        self.dec.end(self.lm_rows())
        return [[self._hyp(h) for h in self.dec.results(b)] for b in range(self.B)]


def assert_best(want, got, log_add, what="", final=assert_final):
    assert (want is None) == (got is None), (what, want, got)
    if want is not None:
        final([want], [got], log_add, what)


def run_script(sess, dec, ems, N, W, lm_row, ops, max_frames, lexicon=False):
    """ops: ("c", [T_b]) / ("b", look_back) / ("p", look_back) for all streams at once
    -> per stream (bests, frames after each prune, final), and the DeviceStreams"""
    B = len(ems)
    ds = DeviceStreams(sess, dec, B, N, W, lm_row, max_frames, lexicon)
    at = [0] * B
    out = [([], [], None) for _ in range(B)]
    for op, v in ops:
        if op == "c":
            ds.chunk([ems[b][at[b]:at[b] + v[b]] for b in range(B)])
            at = [a + x for a, x in zip(at, v)]
        elif op == "b":
            for b in range(B):
                out[b][0].append(ds.best(b, v))
        else:
            dec.prune(v)
            for b in range(B):
                out[b][1].append(dec.frames_in_buffer(b))
    assert at == [e.shape[0] for e in ems]
    fib = [dec.frames_in_buffer(b) for b in range(B)]
    final = ds.end()
    for b in range(B):  # frames in buffer + 1 entries: what is left of the stream, and decodeEnd's sil
        assert final[b] and all(len(h[3]) == fib[b] + 1 for h in final[b]), (b, fib[b])
    return [(o[0], o[1], final[b]) for b, o in enumerate(out)], ds


# ---- 1. a stream without prunes is the offline decode -------------------------------------------------------------------
@pytest.mark.parametrize("log_add", [False, True])
def test_stream_equals_offline(sess, log_add):
    """The same emissions cut into unequal chunks per stream, no prune; stream 1 gets an empty chunk while the others
    advance: the n-best after end and the row lists of every frame are those of fltx_ctc_rows_begin / step / end."""
    N, K, W, sil, blank, Ts = 5, 6, 7, 0, 1, (11, 7, 4)
    ems = [G.emissions(1200 + b, T, N) for b, T in enumerate(Ts)]
    rl = G.SmRowsLM(91, N, W, 41, W - 1, 0)
    lm = _capi.RowsLM(W, rl.usr_to_lm, W - 1, lib=sess.lib)

    def lm_row(b, p):
        return rl.row(list(p))
    off = make_dec(sess, lm, K, N, 25.0, 0.7, -0.3, sil, blank, log_add)
    want, want_rows, want_prefix = decode(sess, off, ems, N, W, lm_row)
    off.close()
    dec = make_dec(sess, lm, K, N, 25.0, 0.7, -0.3, sil, blank, log_add)
    ops = [("c", [3, 0, 4]), ("c", [5, 2, 0]), ("b", 0), ("c", [0, 5, 0]), ("c", [3, 0, 0])]
    got, ds = run_script(sess, dec, ems, N, W, lm_row, ops, 16)
    for b in range(len(Ts)):
        assert len(got[b][2]) > 1
        assert len(got[b][2]) == len(want[b])
        for w, g in zip(want[b], got[b][2]):
            assert g[3] == w[3] and _bits_equal(g[:3], w[:3]), (b, g, w)
        assert len(ds.rows[b]) == Ts[b] == len(want_rows[b])
        for t, (wr, gr) in enumerate(zip(want_rows[b], ds.rows[b])):
            assert [x[:2] for x in gr] == [x[:2] for x in wr], (b, t)
            assert [ds.prefix[b][x[2]] for x in gr] == [want_prefix[b][x[2]] for x in wr], (b, t)
        # best(0) mid-stream is the first hypothesis of the beam then: frames so far + the root
        assert len(got[b][0][0][3]) == [9, 3, 5][b]
    dec.close()
    lm.close()


# ---- 2. - 5. fixtures of the reference itself ---------------------------------------------------------------------------
def _golden():
    path = os.path.join(ROOT, "tests", "golden", "ctc_lm_rows_stream_expected.json.gz")
    if not os.path.exists(path):  # (the generator imports this module before it has written the file; the coverage test
        return []                 # below fails on an empty list)
    with gzip.open(path, "rt") as f:
        return json.load(f)


def _case_lm(c, b):
    return G.SmRowsLM((c["seeds"][b] ^ 0xABCDEF), c["N"], c["W"], c["perm"], c["W"] - 1, 0)


def case_restate(c, b, st):
    rl = _case_lm(c, b)
    lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
    return restate_stream(G.emissions(c["seeds"][b], c["Ts"][b], c["N"]), lm, c["K"], c["Kt"], c["thr"], c["lmw"],
                          c["sil_score"], c["sil"], c["blank"], c["log_add"], GS.stream_script(c, b), st=st)


def assert_case(c, b, got, what):
    """got = (bests, frames, final) of stream b against the fixture"""
    want = c["streams"][b]
    assert len(got[0]) == len(want["best"]) and got[1] == want["frames"], (what, got[1], want["frames"])
    for i, (w, g) in enumerate(zip(want["best"], got[0])):
        assert_best(None if w is None else tuple(w), g, c["log_add"], (what, "best", i))
    assert_final([tuple(h) for h in want["final"]], got[2], c["log_add"], what)


def test_fixtures_cover_the_cases():
    cs = {c["name"]: c for c in _golden()}
    assert set(cs) == {n for n, *_ in GS.CASES}
    ops = [op for c in cs.values() for op in c["ops"]]
    assert {v for op, v in ops if op == "p"} >= {0, 2} and {v for op, v in ops if op == "b"} >= {0, 1, 99}
    assert any(c["log_add"] for c in cs.values()) and any(len(c["Ts"]) == 3 for c in cs.values())
    assert any(0 in v for op, v in ops if op == "c")
    # an empty result, a no-op prune, and older frames that keep their scores after a prune
    assert any(w is None for c in cs.values() for s in c["streams"] for w in s["best"])
    w = cs["ring_wrap"]
    assert w["max_frames"] == 8 and w["Ts"] == [40] and len(w["streams"][0]["frames"]) == 10
    assert cs["wide_beam"]["K"] == 70


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c):
    for b in range(len(c["Ts"])):
        st = Stats()
        bests, frames, final, _ = case_restate(c, b, st)
        assert not st.ties and (not c["log_add"] or st.gap > MIN_GAP), (st.ties, st.gap)
        assert_case(c, b, (bests, frames, final), (c["name"], b))


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess):
    B = len(c["Ts"])
    rls = [_case_lm(c, b) for b in range(B)]
    lm = _capi.RowsLM(c["W"], rls[0].usr_to_lm if c["perm"] else None, c["W"] - 1, lib=sess.lib)
    dec = make_dec(sess, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"], c["sil"], c["blank"], c["log_add"])
    ems = [G.emissions(c["seeds"][b], c["Ts"][b], c["N"]) for b in range(B)]
    got, _ = run_script(sess, dec, ems, c["N"], c["W"], lambda b, p: rls[b].row(list(p)), [tuple(o) for o in c["ops"]],
                        c["max_frames"])
    for b in range(B):
        assert_case(c, b, got[b], (c["name"], b))
    dec.close()
    lm.close()


def test_older_frames_keep_their_scores_after_a_prune():
    """pruneAndNormalize subtracts the current beam's largest score from the current beam only: best(1) right after a
    prune returns the un-normalised score of the frame before, best(0) a normalised one (the fixture says so)"""
    c = {c["name"]: c for c in _golden()}["prune_then_best"]
    i = [op for op, _ in c["ops"]].index("p")
    assert [tuple(o) for o in c["ops"][i:i + 3]] == [("p", 2), ("b", 0), ("b", 1)]
    nb = sum(1 for op, _ in c["ops"][:i] if op == "b")
    b0, b1 = c["streams"][0]["best"][nb], c["streams"][0]["best"][nb + 1]
    assert b0[0] == 0.0 and b1[0] < 0.0 and len(b0[3]) == 3 and len(b1[3]) == 2
    first = [op for op, _ in c["ops"]].index("b")
    assert c["streams"][0]["best"][0][0] < 0.0 and first < i  # (before the prune best(0) is not normalised)


def test_wide_beam_calls_see_more_than_a_wave():
    """K = 70: the beams that the case's best and prune calls work on hold more than 64 hypotheses, so prune's
    normalisation crosses a wave.  The step leaves a beam sorted best first and a prune shifts all of its scores alike,
    so the first best by strict > is slot 0 whatever is called: the kernels read slot 0 and reduce nothing, and no
    sequence of calls could put the first best into the second wave."""
    c = {c["name"]: c for c in _golden()}["wide_beam"]
    st = Stats()
    rl = _case_lm(c, 0)
    lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
    em = G.emissions(c["seeds"][0], c["Ts"][0], c["N"])
    beam = [dict(score=0.0, am=0.0, lm=0.0, state=lm.start(), token=c["sil"], pb=False, parent=None)]
    sizes = []
    for t in range(c["Ts"][0]):
        beam = ctc_frame(beam, em[t], lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"], c["sil"], c["blank"],
                         c["log_add"], st, t)
        sizes.append(len(beam))
    assert sizes[4] > 64 and sizes[7] > 64  # (the calls come after 5 and after 8 frames)


# ---- 6. a stream that stops -------------------------------------------------------------------------------------------
def test_stopped_stream(sess):
    """max_states = 4: stream 0 needs more and reports "LM-state table full"; stream 1 streams on, prunes and ends"""
    N, K, W, sil, blank = 4, 6, 4, 0, 1
    flat = np.full((1, N), -5.0, np.float32)
    flat[0, blank] = 0.0  # stream 1: blanks only -- the root's state and little else survives the threshold
    ems = [G.emissions(800, 9, N) * np.float32(0.25), np.repeat(flat, 9, axis=0)]
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 2.0, 0.7, 0.0, sil, blank, False)
    dec.set_max_states(4)
    dec.stream_begin(2, N, 6)
    lr = _dev(sess, np.zeros((2 * K, W), np.float32))
    at = 0
    for T in (3, 3, 3):
        flat_in = np.concatenate([e[at:at + T].reshape(-1) for e in ems])
        for _ in range(dec.append(flat_in, [T, T])):
            tok, src, state, n = dec.step(lr)
        at += T
        dec.prune(1)
        assert dec.frames_in_buffer(1) == 2
        h = dec.best(1)
        assert h.tokens.tolist() == [blank, blank] and h.score == 0.0 and h.am == 0.0
        with pytest.raises(_capi.FltxError) as e:
            dec.best(0)
        assert e.value.code == _capi.ERR_UNSUPPORTED and "LM-state table full" in str(e.value)
    dec.ctx.synchronize()
    assert int(_np(n)[0]) == 0 and int(_np(n)[1]) >= 1
    dec.end(lr)
    with pytest.raises(_capi.FltxError) as e:
        dec.count(0)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "LM-state table full" in str(e.value)
    assert dec.count(1)[1] == 3 and dec.results(1)[0].tokens.tolist() == [blank, blank, sil]
    dec.close()
    lm.close()


def test_prune_between_append_and_the_steps_keeps_the_bound(sess):
    """A prune while frames of the chunk are unstepped sees only the stepped ones; the others arrive afterwards and count
    against max_frames all the same (the host's bound stays an upper bound of the device's count)"""
    N, K, W = 4, 3, 5
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    lr = _dev(sess, np.zeros((K, W), np.float32))
    em = G.emissions(1900, 10, N)
    dec.stream_begin(1, N, 10)
    assert dec.append(em, [10]) == 10
    dec.prune(0)                                   # nothing stepped yet: the device does nothing
    for _ in range(10):
        dec.step(lr)
    assert dec.frames_in_buffer(0) == 11
    with pytest.raises(IndexError):                # (FLTX_ERR_RANGE: 10 buffered + 1)
        dec.append(em[:1], [1])
    dec.prune(0)
    assert dec.frames_in_buffer(0) == 1
    assert dec.append(em[:6], [6]) == 6
    for _ in range(3):
        dec.step(lr)
    dec.prune(0)                                   # three frames stepped and pruned, three to come
    for _ in range(3):
        dec.step(lr)
    assert dec.frames_in_buffer(0) == 4
    with pytest.raises(IndexError):                # 3 buffered + 8
        dec.append(em[:8], [8])
    assert dec.append(em[:7], [7]) == 7
    for _ in range(7):
        dec.step(lr)
    assert dec.frames_in_buffer(0) == 11 and len(dec.best(0).tokens) == 11
    dec.end(lr)
    assert dec.count(0)[1] == 12
    dec.close()
    lm.close()


def test_a_frame_without_candidates_empties_the_beam(sess):
    """A frame whose emissions are all NaN leaves no candidate: the frame counts, the stream's beam is empty and
    getBestHypothesis returns an empty result (findBestAncestor on no hypotheses, Utils.h:272-275); the other stream
    goes on"""
    N, K, W = 4, 3, 5
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    lr = _dev(sess, np.zeros((2 * K, W), np.float32))
    ems = [G.emissions(1910, 4, N), G.emissions(1911, 4, N)]
    ems[0][2, :] = np.nan
    dec.stream_begin(2, N, 8)
    for _ in range(dec.append(np.concatenate([e.reshape(-1) for e in ems]), [4, 4])):
        tok, src, state, n = dec.step(lr)
    dec.ctx.synchronize()
    assert int(_np(n)[0]) == 0 and int(_np(n)[1]) >= 1
    assert dec.frames_in_buffer(0) == 4 and dec.frames_in_buffer(1) == 5
    for lb in (0, 1):
        assert len(dec.best(0, lb).tokens) == 0 and len(dec.best(1, lb).tokens) == 5 - lb
    dec.prune(1)
    assert dec.frames_in_buffer(0) == 4 and dec.frames_in_buffer(1) == 2
    dec.end(lr)
    assert dec.count(0)[0] == 0 and dec.count(1) == (dec.count(1)[0], 3) and dec.count(1)[0] >= 1
    dec.close()
    lm.close()


# ---- 7. contract and refusals -----------------------------------------------------------------------------------------
def test_contract_and_refusals(sess):
    import ctypes as C
    L, ctx = sess.lib, sess.ctx
    I, S, R = _capi.ERR_INVALID, _capi.ERR_STATE, _capi.ERR_RANGE
    N, K = 6, 4
    lm = _capi.RowsLM(N + 1, None, N, lib=L)
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    dec.B = 1
    outs = dec._rows()
    po = [dec._addr(o) for o in outs]
    em = G.emissions(900, 6, N)
    e_ptr = em.ctypes.data

    def tp(*v):
        a = np.asarray(v, np.int32)
        tp.keep = a
        return a.ctypes.data
    lr = _dev(sess, np.zeros((K, N + 1), np.float32))
    pl = dec._addr(lr)
    sbegin, append = L.lib.fltx_ctc_rows_stream_begin, L.lib.fltx_ctc_rows_stream_append
    prune, frames = L.lib.fltx_ctc_rows_stream_prune, L.lib.fltx_ctc_rows_stream_frames_in_buffer
    step, end, best = L.lib.fltx_ctc_rows_step, L.lib.fltx_ctc_rows_end, L.lib.fltx_result_best
    n = C.c_int32(0)
    ln = C.c_int32(0)
    sc = np.zeros(3)
    toks = np.zeros(64, np.int32)
    # outside a stream
    assert append(dec.h, e_ptr, 0, None, tp(1)) == S and prune(dec.h, 0) == S and frames(dec.h, 0, C.addressof(n)) == S
    # on a rows decoder begun with fltx_ctc_rows_begin
    assert L.lib.fltx_ctc_rows_begin(dec.h, e_ptr, 0, None, tp(3), 1, N, *po) == 0
    assert append(dec.h, e_ptr, 0, None, tp(1)) == S and prune(dec.h, 0) == S and frames(dec.h, 0, C.addressof(n)) == S
    assert best(dec.h, 0, 0, sc.ctypes.data, toks.ctypes.data, None, 64, C.addressof(ln)) == S
    # begin: its own arguments, and fltx_ctc_rows_begin's checks
    assert sbegin(dec.h, 1, N, 0, *po) == I and sbegin(dec.h, 0, N, 4, *po) == I
    assert sbegin(dec.h, 1, N, 4, po[0], None, po[2], po[3]) == I
    assert sbegin(dec.h, 1, 65537, 4, *po) == _capi.ERR_UNSUPPORTED
    bad_lm = _capi.RowsLM(N - 1, None, 0, lib=L)
    d4 = make_dec(sess, bad_lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    assert sbegin(d4.h, 1, N, 4, *po) == I
    d4.close()
    bad_lm.close()
    assert sbegin(dec.h, 1, N, 4, *po) == 0
    assert append(dec.h, e_ptr, 0, None, None) == I and append(dec.h, e_ptr, 0, None, tp(-1)) == I
    assert append(dec.h, None, 0, None, tp(2)) == I
    assert prune(dec.h, -1) == I and frames(dec.h, 0, None) == I and frames(dec.h, 1, C.addressof(n)) == I
    assert best(dec.h, 0, -1, sc.ctypes.data, toks.ctypes.data, None, 64, C.addressof(ln)) == I
    assert best(dec.h, 0, 0, sc.ctypes.data, toks.ctypes.data, None, 64, None) == I
    assert append(dec.h, e_ptr, 0, None, tp(5)) == R                                 # past max_frames
    assert "exceed max_frames 4" in L.lib.fltx_last_error().decode()
    assert append(dec.h, e_ptr, 0, None, tp(3)) == 0
    assert append(dec.h, e_ptr, 0, None, tp(1)) == S                                 # unstepped frames
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == 0
    assert append(dec.h, e_ptr, 0, None, tp(1)) == S
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == 0
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == 0
    assert step(dec.h, None, 0, 0, N + 1, None, 0, 1, None, *po) == 0                # a step after the chunk: nothing
    assert frames(dec.h, 0, C.addressof(n)) == 0 and n.value == 4
    assert append(dec.h, e_ptr, 0, None, tp(2)) == R                                 # 3 buffered + 2
    assert best(dec.h, 0, 0, sc.ctypes.data, toks.ctypes.data, None, 2, C.addressof(ln)) == R and ln.value == 4
    assert best(dec.h, 0, 9, sc.ctypes.data, toks.ctypes.data, None, 64, C.addressof(ln)) == 0 and ln.value == 0
    assert prune(dec.h, 1) == 0
    assert append(dec.h, e_ptr, 0, None, tp(3)) == 0                                 # 1 buffered + 3
    assert append(dec.h, e_ptr, 0, None, tp(0)) == S
    # fltx_stream_* on this kind, as before; the new calls on other kinds
    assert L.lib.fltx_stream_begin(dec.h, 1, N, 10) == S and L.lib.fltx_stream_end(dec.h) == S
    t1 = tp(1)
    assert L.lib.fltx_stream_step(dec.h, e_ptr, 0, None, t1) == S and L.lib.fltx_stream_prune(dec.h, 0) == S
    ok = _capi.make_options(K, N, lm_weight=0.5)
    other = _capi.BatchDecoder(ctx, _capi.LEXFREE, ok, sess.zero, 0, 1)
    s2s = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    for o in (other, s2s):
        assert sbegin(o.h, 1, N, 4, *po) == S and append(o.h, e_ptr, 0, None, t1) == S
        assert prune(o.h, 0) == S and frames(o.h, 0, C.addressof(n)) == S
        o.close()
    # an early end: one frame of the chunk decoded; then the stream is over, and fltx_result_best is what it was
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == 0
    assert end(dec.h, pl, 0, 0, N + 1, None, 0, 1, None) == 0
    assert dec.count(0)[1] == 4                                                      # 3 frames in the buffer + the end
    assert best(dec.h, 0, 5, sc.ctypes.data, toks.ctypes.data, None, 64, C.addressof(ln)) == 0 and ln.value == 4
    assert toks[:4].tolist() == dec.results(0)[0].tokens.tolist() and sc[0] == dec.results(0)[0].score
    assert append(dec.h, e_ptr, 0, None, t1) == S and prune(dec.h, 0) == S
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == S
    dec.close()
    lm.close()


# ---- 8. the Python helper ----------------------------------------------------------------------------------------------
def test_python_helper_on_a_toy_lm(sess):
    """decode_stream with a callable: one LM row per state id, asked once per state; against the restatement"""
    N, K, W, sil, blank, lb = 4, 6, 5, 0, 1, 2
    rl = G.SmRowsLM(21, N, W, 0, W - 1, 0)
    Ts, cuts = (9, 5), [(4, 0), (2, 3), (3, 2)]
    ems, want = [], []
    for b, T in enumerate(Ts):
        script = [x for c in cuts for x in (("c", c[b]), ("p", lb), ("b", 0))]
        for seed in range(1300 + 50 * b, 1400 + 50 * b):
            st = Stats()
            em = G.emissions(seed, T, N)
            res = restate_stream(em, PrefixLM(lambda p: rl.row(list(p)), np.arange(N), W - 1), K, N, 25.0, 0.7, 0.0, sil,
                                 blank, False, script, st=st)
            if not st.ties:
                break
        assert not st.ties
        ems.append(em)
        want.append(res)
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.7, 0.0, sil, blank, False)
    asked = []

    def lm_rows(keys):
        asked.extend(keys)
        return _dev(sess, np.stack([rl.row(list(p)) for _, p in keys]))
    at = [0, 0]
    chunks = []
    for c in cuts:
        chunks.append((np.concatenate([ems[b][at[b]:at[b] + c[b]].reshape(-1) for b in range(2)]), list(c)))
        at = [a + x for a, x in zip(at, c)]
    outs = list(dec.decode_stream(chunks, lm_rows, look_back=lb, N=N, max_frames=8))
    assert len(outs) == len(cuts) + 1 and len(set(asked)) == len(asked)
    for b in range(2):
        for i in range(len(cuts)):
            h = outs[i][b]
            assert_best(want[b][0][i], (h.score, h.am, h.lm, h.tokens.tolist()), False, (b, i))
        assert_final(want[b][2], [(h.score, h.am, h.lm, list(h.tokens)) for h in outs[-1][b]], False, b)
    dec.close()
    lm.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_CTC_LMROWS_STREAM_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
