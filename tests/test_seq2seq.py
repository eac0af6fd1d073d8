"""LexiconFreeSeq2SeqDecoder on the device (text_amd/csrc/fltx_s2s.h, fltx_s2s_* in include/fltx.h).

`restate()` below is a float64 restatement of the reference's search (LexiconFreeSeq2SeqDecoder.cpp:20-165,
decoder/Utils.h:121-266): the model is called with the live hypotheses of the beam in beam order, finished ones are
carried unchanged, a null state drops a row, a row's token beam is its beamSizeToken largest scores, a candidate
scores ((prev + am) + eosScore) + lmWeight * finish for eos and (prev + am) + lmWeight * lm(n) otherwise, survivors are
those >= best - beamThreshold, the beam is their top beamSize, best first, and nothing merges.  The search stops when
no row is live or after maxOutputLength steps; the result rows are maxOutputLength + 3 tokens, right-aligned.

Every test runs on the emulator library (host threads, tests/emu) and -- marked `gpu` -- on the HIP library.  The
model is a pure function of (seed, token prefix), so any row order replays it; its rows are tie-free (distinct values
in a row, a random offset per row), so the token beams and the K-cuts are unique and the device must match exactly:
tokens, the three scores bit for bit, and the row lists of every step.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi, ngram_synth  # noqa: E402

# The GPU cases hand torch device buffers to the library.  torch carries its own HIP runtime, which finds no device
# once the library's runtime has opened it first -- as earlier GPU tests of a session do.  So the `gpu` variant of this
# module runs in a fresh child process (test_gpu_cases_in_a_fresh_process below) that initialises torch first.
CHILD = os.environ.get("FLTX_S2S_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]


class _GpuSess:
    """The HIP library with a context on a torch stream made current: the scores torch uploads and the row lists it
    reads back are ordered with the decoder's kernels on that stream."""

    def __init__(self, gpu_session):
        import torch
        self.lib = gpu_session.lib
        self.stream = torch.cuda.Stream()  # (not the default stream: its handle is NULL, which asks for a library stream)
        torch.cuda.set_stream(self.stream)
        self.ctx = _capi.Context(stream=self.stream.cuda_stream, lib=self.lib)
        self.zero = _capi.ZeroLM(self.ctx)


@pytest.fixture(scope="module")
def gpu_sess(gpu_session):
    return _GpuSess(gpu_session)


@pytest.fixture(params=BACKENDS)
def sess(request):
    if request.param == "emu":
        return request.getfixturevalue("emu_session")
    import torch
    g = request.getfixturevalue("gpu_sess")
    torch.cuda.set_stream(g.stream)  # (the context's stream is the one torch reads the row lists on)
    return g


def is_gpu(sess):
    return "emulation" not in sess.lib.version()


# ---- the model: a pure function of (seed, prefix) --------------------------------------------------------------------
class Model:
    """row(prefix) -> V float32 scores, or None when the model drops the row (a null state).  Values of a row are
    distinct (a permutation, exact in float32) plus one random offset per row; eos_bias makes eos likelier."""

    def __init__(self, seed, V, eos, eos_bias=0.0, drop=0.0, width=None):
        self.seed, self.V, self.eos, self.eos_bias, self.drop = seed, V, eos, eos_bias, drop
        self.width = width or V  # the row width the model returns (need not be the emissions' N)
        self.calls = 0

    def _rng(self, prefix):
        h = hashlib.blake2b(np.asarray([self.seed] + list(prefix), dtype=np.int64).tobytes(), digest_size=8).digest()
        return np.random.default_rng(int.from_bytes(h, "little"))

    def row(self, prefix):
        self.calls += 1
        g = self._rng(prefix)
        if self.drop > 0 and len(prefix) > 0 and g.random() < self.drop:
            return None
        V = self.width
        perm = g.permutation(V).astype(np.float64)
        off = np.float32(g.random())
        r = (-(perm * 2.0 ** -6) - float(off)).astype(np.float32)
        if self.eos < V and self.eos_bias:
            r[self.eos] = np.float32(r[self.eos] + np.float32(self.eos_bias))
        return r


class HostLM:
    """LM::start / score / finish of the library's LM objects (the host twins of the device tables)."""

    def __init__(self, lm):
        self.lm = lm

    def start(self):
        return tuple(self.lm.start(False).tolist()) if self.lm is not None else ()

    def score(self, ctx, n):
        if self.lm is None:
            return ctx, 0.0
        out, s = self.lm.step(np.asarray(ctx, np.int32), n)
        return tuple(out.tolist()), float(np.float32(s))

    def finish(self, ctx):
        return self.score(ctx, -1)


# ---- the restatement --------------------------------------------------------------------------------------------------
def restate(model, lm, K, Kt, thr, lmw, eos_score, eos, maxlen, ties=None):
    """One utterance.  -> (final hypotheses [(score, am, lm, tokens)], rows per step [(token, beam_idx, src_row)]).
    ties: a list that receives (step, what) for every tie at a token-beam cut or among the kept K (their order is the
    reference's partial_sort's / the heap's, nothing to reproduce)."""
    root = dict(score=0.0, am=0.0, lm=0.0, token=-1, prev=-1, ctx=lm.start(), path=[])
    beam = [root]
    hyps = [beam]
    rows_per_step = []
    t = 0
    while t < maxlen:
        live = [(i, h) for i, h in enumerate(beam) if h["token"] != eos]
        if not live:
            break
        row_of = {i: q for q, (i, _) in enumerate(live)}
        cands = []
        for i, h in enumerate(beam):
            if h["token"] == eos:
                cands.append(dict(h, prev=i, path=h["path"] + [eos], src=None))
                continue
            r = model.row(h["path"])
            if r is None:
                continue
            V = len(r)
            order = np.argsort(-r.astype(np.float64), kind="stable")
            if ties is not None and V > Kt and r[order[Kt - 1]] == r[order[Kt]]:
                ties.append((t, "token beam"))
            idx = order[:Kt] if V > Kt else np.arange(V)
            for n in idx.tolist():
                a = float(r[n])
                if n == eos:
                    c2, l = lm.finish(h["ctx"])
                    s = ((h["score"] + a) + eos_score) + lmw * l
                else:
                    c2, l = lm.score(h["ctx"], n)
                    s = (h["score"] + a) + lmw * l
                cands.append(dict(score=s, am=h["am"] + a, lm=h["lm"] + l, token=n, prev=i, ctx=c2,
                                  path=h["path"] + [n], src=row_of[i]))
        if not cands:
            beam = []
            hyps.append(beam)
            rows_per_step.append([])
            break
        best = max(c["score"] for c in cands)
        surv = [c for c in cands if c["score"] >= best - thr]
        surv.sort(key=lambda c: -c["score"])
        if ties is not None:
            sc = [c["score"] for c in surv[:K + 1]]
            if any(a == b for a, b in zip(sc, sc[1:])):
                ties.append((t, "beam"))
        beam = surv[:K]
        hyps.append(beam)
        t += 1
        nxt = [(c["token"], c["prev"], c["src"]) for c in beam if c["token"] != eos]
        rows_per_step.append(nxt if t < maxlen else [])
    final = next(b for b in reversed(hyps) if b)
    L = maxlen + 3
    out = []
    for h in final:
        toks = [-1] * L
        p = h["path"]
        for j, tok in enumerate(reversed(p)):
            toks[L - 1 - j] = tok
        out.append((h["score"], h["am"], h["lm"], toks))
    return out, rows_per_step


# ---- the device path -------------------------------------------------------------------------------------------------
def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def run_device(sess, models, lm, K, Kt, thr, lmw, eos_score, eos, maxlen, V, log_add=False, pad="nan",
               host_scores=False, dec=None):
    """All utterances in one batch.  -> (final per utterance as restate's, rows per step per utterance)"""
    B = len(models)
    own = dec is None
    if own:
        opts = _capi.make_s2s_options(K, Kt, thr, lmw, eos_score, log_add)
        dec = _capi.Seq2SeqBatchDecoder(sess.ctx, opts, lm if lm is not None else sess.zero, eos, maxlen)
    tok, beam, src, n = dec.begin(B, V)
    prefix = {(b, 0): [] for b in range(B)}
    rows = [[] for _ in range(B)]
    gpu = is_gpu(sess)
    rng = np.random.default_rng(7)
    for t in range(maxlen + 2):  # (two steps more than it takes: a step after the last one is a no-op)
        if gpu:
            dec.ctx.synchronize()
        tok_h, beam_h, src_h, n_h = _np(tok), _np(beam), _np(src), _np(n)
        if t > 0:
            for b in range(B):
                rows[b].append([(int(tok_h[b, k]), int(beam_h[b, k]), int(src_h[b, k]) - b * K if src_h[b, k] >= 0
                                 else None) for k in range(n_h[b])])
                assert (tok_h[b, n_h[b]:] == -1).all() and (src_h[b, n_h[b]:] == -1).all(), \
                    (t, b, n_h.tolist(), tok_h.tolist(), beam_h.tolist(), src_h.tolist())
        W = max(m.width for m in models)
        sc = np.full((B * K, W), np.nan if pad == "nan" else 0.0, dtype=np.float32)
        if pad == "garbage":
            sc[:] = rng.standard_normal(sc.shape).astype(np.float32) * 100
        valid = np.zeros(B * K, dtype=np.uint8)
        newpre = {}
        for b in range(B):
            for k in range(n_h[b]):
                p = [] if t == 0 else prefix[(b, int(src_h[b, k]) - b * K)] + [int(tok_h[b, k])]
                newpre[(b, k)] = p
                r = models[b].row(p)
                if r is None:
                    if pad == "garbage":
                        sc[b * K + k, :] = 1e30  # (must be ignored: the row is marked dropped)
                    continue
                sc[b * K + k, :len(r)] = r
                valid[b * K + k] = 1
        prefix = newpre
        if gpu and not host_scores:
            import torch
            scd, vd = torch.from_numpy(sc).cuda(), torch.from_numpy(valid).cuda()
            tok, beam, src, n = dec.step(scd, vd)
        else:
            tok, beam, src, n = dec.step(sc, valid)
    assert dec.done()
    dec.end()
    out = []
    for b in range(B):
        hs = dec.results(b)
        out.append([(h.score, h.am, h.lm, h.tokens.tolist()) for h in hs])
        assert all((h.words == -1).all() for h in hs)
    # the row lists: stop at the first empty step (the restatement stops there)
    for b in range(B):
        while rows[b] and rows[b][-1] == [] and (len(rows[b]) < 2 or rows[b][-2] == []):
            rows[b].pop()
    if own:
        dec.close()
    return out, rows


def check_case(sess, seeds, V, K, Kt, thr=1e9, lmw=0.0, eos_score=0.0, eos=None, maxlen=6, eos_bias=0.0, drop=0.0,
               lm=None, log_add=False, pad="nan", width=None, host_scores=False):
    eos = V - 1 if eos is None else eos
    models = [Model(s, V, eos, eos_bias, drop, width) for s in seeds]
    hl = HostLM(lm)
    want = [restate(m, hl, K, Kt, thr, lmw, eos_score, eos, maxlen) for m in models]
    got, rows = run_device(sess, [Model(s, V, eos, eos_bias, drop, width) for s in seeds], lm, K, Kt, thr, lmw,
                           eos_score, eos, maxlen, width or V, log_add, pad, host_scores)
    for b, ((wf, wr), gf, gr) in enumerate(zip(want, got, rows)):
        assert len(gf) == len(wf), (b, len(gf), len(wf))
        for i, (w, g) in enumerate(zip(wf, gf)):
            assert g[3] == w[3], (b, i, g[3], w[3])
            assert g[:3] == w[:3], (b, i, g[:3], w[:3])  # bit-equal doubles
        wr_trim = [r for r in wr]
        while wr_trim and wr_trim[-1] == []:
            wr_trim.pop()
        gr_trim = [r for r in gr]
        while gr_trim and gr_trim[-1] == []:
            gr_trim.pop()
        assert gr_trim == wr_trim, (b, gr_trim, wr_trim)
    return want


# ---- the restatement against the reference's own test (bindings/python/test/test_decoder.py:255-382) ---------------
def test_restatement_reproduces_reference_python_test():
    """The reference's seq2seq test: V = 4, eos = 4 (never proposed), beam 2, token beam 4 (= V: no partial sort),
    maxOutputLength 3, the model's rows fixed per step.  Expected tokens [-1, -1, -1, 2, 0, 1] / [.., 2, 1, 1]."""
    steps = [np.array([0.1, 0.2, 0.5, 0.2], np.float32), np.array([0.4, 0.3, 0.2, 0.1], np.float32),
             np.array([0.2, 0.6, 0.1, 0.1], np.float32)]

    class Fixed:
        width = 4

        def row(self, prefix):
            return steps[len(prefix)]

    out, _ = restate(Fixed(), HostLM(None), 2, 4, 1e9, 0.0, 0.0, 4, 3)
    assert out[0][3] == [-1, -1, -1, 2, 0, 1]
    assert out[1][3] == [-1, -1, -1, 2, 1, 1]


# ---- device against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,Kt", [(4, 2, 4), (29, 1, 5), (29, 8, 29), (29, 8, 40), (1000, 8, 50), (1000, 50, 1000),
                                    (10000, 2, 10000)])
def test_zero_lm_matches_restatement(sess, V, K, Kt):
    """ZeroLM: Kt < V, = V, > V; eos inside the rows, early finishes (eos bias), K from 1 to 50."""
    check_case(sess, [11, 12, 13], V, K, Kt, eos=V // 2, eos_bias=0.3, maxlen=5)


def test_eos_outside_the_rows(sess):
    """eos >= V: never proposed, every hypothesis runs to maxOutputLength (the reference's own tests: eos = V)."""
    check_case(sess, [3, 4], 6, 4, 6, eos=6, maxlen=4)


def test_eos_score_threshold_and_dropped_rows(sess):
    """eosScore != 0, a small beam threshold, rows the model drops (null states), garbage in dropped rows."""
    check_case(sess, [21, 22, 23, 24], 50, 8, 12, thr=0.3, eos_score=-0.75, eos=3, eos_bias=1.0, drop=0.2, maxlen=7,
               pad="garbage")


def test_eos_beyond_the_kept_list(sess):
    """Without LM terms a row keeps min(Kt, K + 1) tokens; eos must still come in when it is among the Kt best."""
    check_case(sess, [31, 32, 33], 200, 2, 150, eos=7, eos_bias=-0.05, eos_score=5.0, maxlen=5)


def test_host_scores(sess):
    """scores from host memory (copied by the library)."""
    check_case(sess, [41], 30, 4, 8, eos=2, eos_bias=0.2, maxlen=4, host_scores=True)


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    def make(V, seed=5):
        path = str(tmp_path_factory.mktemp("s2s_lm") / ("t%d_s%d.arpa" % (V, seed)))
        vocab = ngram_synth.words(V, "t")
        ngram_synth.write_arpa(path, vocab, 3, (0, 400, 200), seed)
        return path, vocab
    return make


@pytest.mark.parametrize("lmw,log_add", [(0.7, False), (0.7, True), (0.0, False)])
def test_ngram_lm(sess, arpa, lmw, log_add):
    """A 3-gram over the tokens, lmWeight != 0 (and 0: the shortcut still fills in the LM score); logAdd has no
    effect (nothing merges)."""
    path, vocab = arpa(29)
    lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
    check_case(sess, [51, 52, 53], 29, 8, 10, lmw=lmw, eos=5, eos_bias=0.3, eos_score=-0.5, maxlen=6, lm=lm,
               log_add=log_add)


def test_log_add_changes_nothing(sess, arpa):
    path, vocab = arpa(40)
    lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
    a = check_case(sess, [61, 62], 40, 6, 12, lmw=0.5, eos=4, eos_bias=0.2, maxlen=5, lm=lm, log_add=False)
    b = check_case(sess, [61, 62], 40, 6, 12, lmw=0.5, eos=4, eos_bias=0.2, maxlen=5, lm=lm, log_add=True)
    assert a == b


def test_random_cases(sess):
    """Seeded random configurations (more and larger on the GPU)."""
    rng = np.random.default_rng(2024)
    n = 30 if is_gpu(sess) else 240
    for _ in range(n):
        V = int(rng.choice([3, 5, 17, 64, 300] + ([2000, 32768] if is_gpu(sess) else [])))
        K = int(rng.integers(1, 33 if not is_gpu(sess) or V > 2000 else 257))
        Kt = int(rng.integers(1, V + 5))
        eos = int(rng.integers(0, V + 2))
        check_case(sess, [int(rng.integers(1 << 30))], V, K, Kt, thr=float(rng.choice([0.5, 3.0, 1e9])),
                   eos_score=float(rng.choice([0.0, -0.3, 0.2])), eos=eos, eos_bias=float(rng.choice([0.0, 0.2, 0.6])),
                   drop=float(rng.choice([0.0, 0.1])), maxlen=int(rng.integers(1, 6)),
                   pad=str(rng.choice(["nan", "garbage"])))


def _large_batch(gpu_sess):
    """B = 64: V = 32 768 (K = 16), K = 256 (V = 600); garbage in dropped rows, NaN padding."""
    check_case(gpu_sess, list(range(100, 164)), 32768, 16, 300, eos=9, eos_bias=1.0, drop=0.05, maxlen=3,
               pad="garbage")
    check_case(gpu_sess, list(range(400, 464)), 600, 256, 40, eos=9, eos_bias=0.3, drop=0.05, maxlen=3, pad="garbage")
    check_case(gpu_sess, list(range(200, 264)), 1000, 64, 64, eos=1, eos_bias=0.3, maxlen=6, pad="nan")


def _large_batch_ngram(gpu_sess, arpa):
    path, vocab = arpa(500, 9)
    lm = _capi.ArpaLM(path, vocab, lib=gpu_sess.lib)
    check_case(gpu_sess, list(range(300, 364)), 500, 32, 64, lmw=0.8, eos=2, eos_bias=0.3, maxlen=5, lm=lm)


# ---- the ABI contract -------------------------------------------------------------------------------------------------
def _rows_arrays(sess, B, K):
    if is_gpu(sess):
        import torch
        return [torch.zeros(B * K, dtype=torch.int32, device="cuda") for _ in range(3)] + \
            [torch.zeros(B, dtype=torch.int32, device="cuda")]
    return [np.zeros(B * K, np.int32) for _ in range(3)] + [np.zeros(B, np.int32)]


def _addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def test_rows_and_finished_ahead_of_live(sess):
    """The rows of a step: padded at b*K + k, beam_idx = parent's index in the previous beam (which includes a
    finished hypothesis ahead of the live ones), src_row = the parent's row of the call that produced it."""
    K, V, eos = 3, 5, 0
    opts = _capi.make_s2s_options(K, V, 1e9)
    dec = _capi.Seq2SeqBatchDecoder(sess.ctx, opts, sess.zero, eos, 5)
    tok, beam, src, n = (_np(x) for x in dec.begin(2, V))
    assert n.tolist() == [1, 1] and tok[:, 0].tolist() == [-1, -1] and (src == -1).all() and (beam == -1).all()
    # step 1: eos best, then tokens 3, 1
    sc = np.full((2 * K, V), np.nan, np.float32)
    sc[0] = [-0.1, -3.0, -4.0, -0.5, -5.0]
    sc[K] = [-9.0, -1.0, -2.0, -3.0, -0.2]
    tok, beam, src, n = (_np(x) for x in dec.step(sc, np.array([1, 0, 0, 1, 0, 0], np.uint8)))
    assert n.tolist() == [2, 3]
    assert tok[0, :2].tolist() == [3, 1] and beam[0, :2].tolist() == [0, 0] and src[0, :2].tolist() == [0, 0]
    assert tok[0, 2] == -1 and src[0, 2] == -1
    assert tok[1].tolist() == [4, 1, 2] and src[1].tolist() == [K, K, K]
    # step 2, utterance 0: beam = [eos(-0.1), 3(-0.5), 1(-3.0)]: rows are hyps 1 and 2 of that beam
    sc = np.full((2 * K, V), np.nan, np.float32)
    sc[0] = [-5.0, -0.01, -6.0, -7.0, -8.0]   # hyp 1 (token 3): child 1 at -0.51
    sc[1] = [-5.0, -6.0, -0.02, -7.0, -8.0]   # hyp 2 (token 1): child 2 at -3.02
    for k in range(3):
        sc[K + k] = -np.arange(V, dtype=np.float32) - k
    tok, beam, src, n = (_np(x) for x in dec.step(sc, None))
    # new beam of utterance 0: eos carried (-0.1) first, then (3,1) at -0.51, (3,0)... by score
    assert tok[0, 0] == 1 and beam[0, 0] == 1 and src[0, 0] == 0
    dec.end()
    h = dec.results(0)
    assert h[0].tokens.tolist()[-3:] == [-1, 0, 0] and h[0].score == np.float64(np.float32(-0.1))
    best = dec.best(0, look_back=5)  # (getBestHypothesis ignores lookBack: the final beam's first)
    assert best.tokens.tolist() == h[0].tokens.tolist() and best.score == h[0].score
    dec.close()


def test_step_after_done_is_a_noop(sess):
    """eos = 0, K = 2.  Step 1: beam [eos (-0.1), 1 (-5.0)], one live row.  Step 2: the carried eos (-0.1) and 1 -> eos
    (-5.1) beat 1 -> 1 (-10.0): no live row, done.  A step after that lists no rows and changes no result."""
    K, V = 2, 4
    dec = _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(K, V, 1e9), sess.zero, 0, 3)
    dec.begin(1, V)
    sc = np.full((K, V), np.nan, np.float32)
    sc[0] = [-0.1, -5.0, -6.0, -7.0]
    tok, beam, src, n = (_np(x) for x in dec.step(sc))
    assert n.tolist() == [1] and tok[0].tolist() == [1, -1] and beam[0].tolist() == [0, -1] and src[0].tolist() == [0, -1]
    assert not dec.done()
    tok, beam, src, n = (_np(x) for x in dec.step(sc))
    assert n.tolist() == [0] and (tok == -1).all() and dec.done()
    dec.end()
    a = [(h.score, h.tokens.tolist()) for h in dec.results(0)]
    assert a == [(float(np.float32(-0.1)), [-1, -1, -1, -1, 0, 0]), (-5.0 + float(np.float32(-0.1)), [-1, -1, -1, -1, 1, 0])]
    tok, beam, src, n = (_np(x) for x in dec.step(sc))
    assert n.tolist() == [0] and (tok == -1).all()
    dec.end()
    assert [(h.score, h.tokens.tolist()) for h in dec.results(0)] == a
    dec.close()


def test_max_length_zero_and_restart(sess):
    """maxOutputLength 0: the root alone (length 3); decodeStep again on the same object restarts from the root."""
    dec = _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(2, 4, 1e9), sess.zero, 9, 0)
    tok, beam, src, n = (_np(x) for x in dec.begin(1, 4))
    assert n.tolist() == [0] and dec.done()
    dec.end()
    h = dec.results(0)
    assert len(h) == 1 and h[0].tokens.tolist() == [-1, -1, -1] and h[0].score == 0.0
    dec.close()
    want, _ = restate(Model(77, 12, 3, 1.0), HostLM(None), 4, 6, 1e9, 0.0, 0.0, 3, 4)
    dec = _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(4, 6, 1e9), sess.zero, 3, 4)
    for _ in range(2):
        got, _ = run_device(sess, [Model(77, 12, 3, 1.0)], None, 4, 6, 1e9, 0.0, 0.0, 3, 4, 12, dec=dec)
        assert got[0] == want
    dec.close()


def test_limits_and_refusals(sess):
    L, ctx = sess.lib, sess.ctx
    h = C.c_void_p()

    def create(opts, lm=None, eos=1, maxlen=5):
        return L.lib.fltx_s2s_decoder_create(ctx.h, C.byref(opts), (lm or sess.zero).h, eos, maxlen, C.byref(h))
    assert create(_capi.make_s2s_options(257, 4)) == _capi.ERR_UNSUPPORTED
    assert create(_capi.make_s2s_options(4, 4), maxlen=4097) == _capi.ERR_UNSUPPORTED
    assert create(_capi.make_s2s_options(0, 4)) == _capi.ERR_INVALID
    assert create(_capi.make_s2s_options(4, 4), eos=-1) == _capi.ERR_INVALID

    class Lm:
        def start(self, start_with_nothing):
            return 0

        def score(self, state, idx):
            return state, 0.0

        def finish(self, state):
            return state, 0.0
    hlm = _capi.HostLM(Lm(), lib=L)
    assert create(_capi.make_s2s_options(4, 4), lm=hlm) == _capi.ERR_UNSUPPORTED
    assert "host" in L.lib.fltx_last_error().decode()
    dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(4, 4), sess.zero, 1, 5)
    out = _rows_arrays(sess, 2, 4)
    assert L.lib.fltx_s2s_begin(dec.h, 2, 65537, *[_addr(o) for o in out]) == _capi.ERR_UNSUPPORTED
    assert L.lib.fltx_s2s_step(dec.h, None, 0, 4, None, *[_addr(o) for o in out]) == _capi.ERR_STATE
    T = np.array([2], np.int32)
    e = np.zeros(8, np.float32)
    assert L.lib.fltx_decode_batch(dec.h, e.ctypes.data, 0, None, T.ctypes.data, 1, 4) == _capi.ERR_STATE
    assert L.lib.fltx_stream_begin(dec.h, 1, 4, 10) == _capi.ERR_STATE
    dec.close()
    # a token beam beyond 64 with LM terms
    vocab = ngram_synth.words(100, "t")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "lm.arpa")
        ngram_synth.write_arpa(p, vocab, 2, (0, 50), 3)
        lm = _capi.ArpaLM(p, vocab, lib=L)
        dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(4, 65, lm_weight=0.5), lm, 1, 5)
        assert L.lib.fltx_s2s_begin(dec.h, 1, 100, *[_addr(o) for o in out]) == _capi.ERR_UNSUPPORTED
        assert L.lib.fltx_s2s_begin(dec.h, 1, 64, *[_addr(o) for o in out]) == _capi.FLTX_OK
        dec.close()
        dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(4, 65, lm_weight=0.0), lm, 1, 5)
        assert L.lib.fltx_s2s_begin(dec.h, 1, 100, *[_addr(o) for o in out]) == _capi.FLTX_OK
        dec.close()
    # a lexicon-free CTC decoder refuses the seq2seq calls
    bd = _capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(4, 4), sess.zero, 0, 1)
    assert L.lib.fltx_s2s_begin(bd.h, 1, 4, *[_addr(o) for o in out]) == _capi.ERR_STATE
    bd.close()


def _torch_model_decode_loop(gpu_session):
    """Seq2SeqBatchDecoder.decode with a tiny torch "model" -- an embedding and a hidden state gathered by src_row
    (elementwise float32 arithmetic, so every row is the same float whatever the batch) -- against the restatement run
    on the same model's outputs."""
    import torch
    B, K, Kt, V, eos, maxlen = 8, 6, 10, 40, 3, 7
    g = np.random.default_rng(5)
    E = g.standard_normal((V + 1, V)).astype(np.float32)  # row V: the root's token (-1)
    E[:, eos] -= np.float32(0.8)
    H0 = g.standard_normal((B, V)).astype(np.float32)
    half = np.float32(0.5)

    class Ref:
        width = V

        def __init__(self, b):
            self.b = b

        def row(self, prefix):
            h = H0[self.b].copy()
            for tok in [-1] + list(prefix):
                h = h * half + E[tok if tok >= 0 else V]
            return h

    want = [restate(Ref(b), HostLM(None), K, Kt, 2.0, 0.0, 0.0, eos, maxlen)[0] for b in range(B)]
    stream = torch.cuda.Stream()
    prev_stream = torch.cuda.current_stream()
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream, lib=gpu_session.lib)
    dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 2.0), _capi.ZeroLM(ctx), eos, maxlen)
    Et = torch.from_numpy(E).cuda()
    state = {"h": torch.from_numpy(np.repeat(H0, K, axis=0)).cuda()}  # [B*K, V]: row b*K + k

    def step_fn(token, src_row, row_mask, t):
        if t > 0:
            state["h"] = state["h"].index_select(0, src_row.clamp(min=0).long())
        tok = torch.where(token >= 0, token, torch.full_like(token, V)).long()
        state["h"] = torch.add(state["h"].mul(0.5), Et.index_select(0, tok))
        return state["h"]

    try:
        got = dec.decode(step_fn, B, V)
    finally:
        torch.cuda.set_stream(prev_stream)
    for b in range(B):
        assert [(h.score, h.am, h.lm, list(h.tokens)) for h in got[b]] == want[b], b
    dec.close()
    ctx.close()


if CHILD:  # (GPU-only cases: defined in the child alone)
    test_large_batch = pytest.mark.gpu(_large_batch)
    test_large_batch_ngram = pytest.mark.gpu(_large_batch_ngram)
    test_torch_model_decode_loop = pytest.mark.gpu(_torch_model_decode_loop)


@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_S2S_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process


# ---- fixtures of the reference itself (tests/golden/make_s2s_golden.py) ---------------------------------------------
def _golden():
    import gzip
    import json
    with gzip.open(os.path.join(ROOT, "tests", "golden", "seq2seq_expected.json.gz"), "rt") as f:
        return json.load(f)


def _golden_lm(c, d, lib):
    from golden import make_s2s_golden as G
    if not c["lm"]:
        return None
    path, vocab = G.arpa_file(str(d), c["lm"])
    return _capi.ArpaLM(path, vocab, lib=lib)


def _golden_model(c):
    from golden import make_s2s_golden as G
    return G.SmModel(c["seed"], c["V"], c["eos"], c["eos_bias"], c["drop"])


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c, emu_session, tmp_path):
    """The restatement against the compiled reference: every fixture, tokens exact and the three scores bit-equal
    (the n-gram cases: the reference over oracle/arpa_lm.h, the restatement over the library's LM tables)."""
    lm = _golden_lm(c, tmp_path, emu_session.lib)
    ties = []
    got, _ = restate(_golden_model(c), HostLM(lm), c["K"], c["Kt"], c["thr"], c["lmw"], c["eos_score"], c["eos"],
                     c["maxlen"], ties=ties)
    assert not ties
    assert [list(h[:3]) + [h[3]] for h in got] == c["hyps"]


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess, tmp_path):
    """The device path against the compiled reference, with logAdd as the fixture has it and flipped (no effect)."""
    lm = _golden_lm(c, tmp_path, sess.lib)
    for log_add in (c["log_add"], not c["log_add"]):
        got, _ = run_device(sess, [_golden_model(c)], lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["eos_score"],
                            c["eos"], c["maxlen"], c["V"], log_add=log_add)
        assert [list(h[:3]) + [h[3]] for h in got[0]] == c["hyps"], (c["name"], log_add)


# ---- the reference's Python surface (text_amd/compat: flashlight.lib.text.decoder) ----------------------------------
COMPAT = os.path.join(ROOT, "text_amd", "compat")


def test_compat_options_pickle_and_emitting_model_state():
    if COMPAT not in sys.path:
        sys.path.insert(0, COMPAT)
    import pickle
    from flashlight.lib.text.decoder import (CriterionType, LexiconFreeSeq2SeqDecoderOptions,
                                             create_emitting_model_state, get_obj_from_emitting_model_state)
    o = LexiconFreeSeq2SeqDecoderOptions(beam_size=2, beam_size_token=4, beam_threshold=1000.0, lm_weight=0.5,
                                         eos_score=-1.5, log_add=True)
    o2 = pickle.loads(pickle.dumps(o))
    assert (o2.beam_size, o2.beam_size_token, o2.beam_threshold, o2.lm_weight, o2.eos_score, o2.log_add) == \
        (2, 4, 1000.0, 0.5, -1.5, True)
    obj = {"h": 1}
    assert get_obj_from_emitting_model_state(create_emitting_model_state(obj)) is obj
    assert CriterionType.S2S != CriterionType.CTC


def _reference_python_flow(gpu_sess):
    """bindings/python/test/test_decoder.py:255-382 (DecoderLexiconFreeSeq2SeqTestCase) against the compat package:
    the callback's asserted token / beam indices and states, the final scores and tokens; decode_step twice."""
    if COMPAT not in sys.path:
        sys.path.insert(0, COMPAT)
    from flashlight.lib.text.decoder import (LexiconFreeSeq2SeqDecoder, LexiconFreeSeq2SeqDecoderOptions, ZeroLM,
                                             create_emitting_model_state, get_obj_from_emitting_model_state)
    T, N = 3, 4
    emissions = np.array([i - (T * N) / 2 for i in range(0, T * N)])
    mapping = {0: [0.1, 0.1, 0.5, 0.1], 1: [0.5, 0.2, 0.1, 0.0], 2: [0.1, 0.5, 0.1, 0.1]}

    class St:
        def __init__(self, timestep, token_idx, score):
            self.timestep, self.token_idx, self.score = timestep, token_idx, score
    calls = []

    def update_func(emissions_ptr, n, t_, tok, beam, states, timestep):
        calls.append(timestep)
        assert (n, t_) == (N, T) and len(tok) == len(states)
        if timestep == 0:
            assert tok == [-1] and beam == [-1] and len(states) == 1
        else:
            for s in states:
                p = get_obj_from_emitting_model_state(s)
                if timestep == 1:
                    assert p.score == -1 and p.token_idx == 0 and beam == [0] * len(tok)
                else:
                    sc = mapping[timestep - 1]
                    assert math.isclose(p.score, max(sc)) and p.token_idx == sc.index(max(sc))
                    assert beam == [0] * len(tok)
        cur = mapping[timestep]
        st = [create_emitting_model_state(St(timestep, i, -1 if timestep == 0 else cur[i])) for i in range(len(tok))]
        return [cur] * len(tok), st

    import math
    opts = LexiconFreeSeq2SeqDecoderOptions(beam_size=2, beam_size_token=4, beam_threshold=1000, lm_weight=0,
                                            eos_score=0, log_add=True)
    dec = LexiconFreeSeq2SeqDecoder(options=opts, lm=ZeroLM(), eos_idx=4, update_func=update_func,
                                    max_output_length=3)
    for _ in range(2):  # (decodeStep restarts from the root)
        calls.clear()
        dec.decode_step(emissions.ctypes.data, T, N)
        assert calls == [0, 1, 2]
        hyps = dec.get_all_final_hypothesis()
        assert len(hyps) == 2
        assert math.isclose(hyps[0].score, 0.5 + 0.5 + 0.5, rel_tol=1e-6)
        assert math.isclose(hyps[1].score, 0.5 + 0.2 + 0.5, rel_tol=1e-6)
        for h in hyps:
            assert h.lmScore == 0 and h.score == h.emittingModelScore and len(h.words) == len(h.tokens)
        assert hyps[0].tokens == [-1, -1, -1, 2, 0, 1]
        assert hyps[1].tokens == [-1, -1, -1, 2, 1, 1]
        assert dec.get_best_hypothesis().tokens == hyps[0].tokens
        assert dec.prune() is None and dec.n_decoded_frames_in_buffer() == -1


if CHILD:
    test_reference_python_flow = pytest.mark.gpu(_reference_python_flow)


@pytest.mark.parametrize("V,K,Kt", [(4, 2, 4), (100, 3, 5), (300, 8, 300), (1000, 50, 64)])
def test_exact_ties_at_the_cuts(sess, V, K, Kt):
    """Rows of equal values: ties at the token-beam cut and at the K-cut (the reference resolves them by partial_sort's
    order; any valid top-k is accepted).  Two steps: distinct tokens per hypothesis, every score exact, rows padded."""
    eos = V + 1
    dec = _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(K, Kt, 1e9), sess.zero, eos, 4)
    tok, beam, src, n = (_np(x) for x in dec.begin(2, V))
    for step in range(2):
        sc = np.full((2 * K, V), -0.5, np.float32)
        sc[K:] = -0.25
        tok, beam, src, n = (_np(x) for x in dec.step(sc))
        want_n = min(K, min(Kt, V) * (1 if step == 0 else int(min(K, min(Kt, V)))))
        assert n.tolist() == [want_n, want_n]
        for b in range(2):
            rows = list(zip(tok[b, :want_n].tolist(), beam[b, :want_n].tolist()))
            assert len(set(rows)) == want_n and all(0 <= t < V for t, _ in rows)
            assert (tok[b, want_n:] == -1).all()
    dec.end()
    for b, v in ((0, -0.5), (1, -0.25)):
        hs = dec.results(b)
        assert len(hs) == K and all(h.score == 2 * v for h in hs)
        assert len({tuple(h.tokens.tolist()) for h in hs}) == K
    dec.close()
