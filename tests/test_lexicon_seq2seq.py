"""LexiconSeq2SeqDecoder on the device (text_amd/csrc/fltx_s2s_lex.h, fltx_s2s_lex_* in include/fltx.h).

`restate_lex()` below is a float64 restatement of the reference's search (LexiconSeq2SeqDecoder.cpp:20-231,
decoder/Utils.h:121-266).  The model is called with the live hypotheses in beam order; finished ones are carried; a null
state drops a row; a row's token beam is its beamSizeToken largest scores, taken before the trie filter.  eos is a
candidate at the root only (LM term finish(state)); a token that is a child of the hypothesis' node stays in the trie
(smearing: child.maxScore - lexMaxScore in float, same LM state; a token LM: score(state, token)) and ends a word per
label (score(state, word) - lexMaxScore, + wordScore; a token LM: the first label with the token's state and score).
Survivors of the threshold MERGE when they share an LM-state object, trie node and token: the group is folded from its
best member in descending score order (max, or max + log1p(exp(min - max))).  The beam is the top beamSize, best first.
LM states are objects here as in the reference: LMState::child hands out the existing child.

Every test runs on the emulator library (host threads, tests/emu) and -- marked `gpu` -- on the HIP library, in a fresh
child process that initialises torch first (as tests/test_seq2seq.py does).
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi, ngram_synth  # noqa: E402

CHILD = os.environ.get("FLTX_LEX_S2S_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
F32 = np.float32


class _GpuSess:
    def __init__(self, gpu_session):
        import torch
        self.lib = gpu_session.lib
        self.stream = torch.cuda.Stream()  # (not the default stream: its handle is NULL)
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
    torch.cuda.set_stream(g.stream)
    return g


def is_gpu(sess):
    return "emulation" not in sess.lib.version()


# ---- the model (tests/golden/make_s2s_golden.SmModel: a pure function of (seed, prefix)) --------------------------
def sm_model(seed, V, eos, eos_bias=0.0, drop=0.0):
    from golden import make_s2s_golden as G
    return G.SmModel(seed, V, eos, eos_bias, drop)


# ---- lexicons ------------------------------------------------------------------------------------------------------
def make_lexicon(V, eos, n_words, seed, max_len=4, homophones=0.0, respell=0.0, single=0.1):
    """[(label, score, tokens)]: random spellings over the tokens other than eos; `homophones`: share of words that
    reuse an earlier word's spelling (several labels on a node -- their words tie under ZeroLM); `respell`: share of
    words that add a second spelling of an earlier word ending in the same token (w: a b c and w: c -- what makes
    hypotheses meet in one LM state); `single`: share of one-token words.  Otherwise no spelling has two labels."""
    g = np.random.default_rng(seed)
    alpha = [t for t in range(V) if t != eos]
    out, owner = [], {}

    def draw(n):
        return [alpha[int(g.integers(len(alpha)))] for _ in range(n)]
    for w in range(n_words):
        u = g.random()
        lab = w
        if out and u < homophones:
            toks = list(out[int(g.integers(len(out)))][2])
        else:
            if out and u < homophones + respell:
                lab, _, t0 = out[int(g.integers(len(out)))]
                toks = draw(int(g.integers(0, max_len))) + [t0[-1]]
            elif g.random() < single:
                toks = draw(1)
            else:
                toks = draw(int(g.integers(2, max_len + 1)))
            if owner.get(tuple(toks), lab) != lab:
                continue
        owner.setdefault(tuple(toks), lab)
        out.append((lab, float(F32(-g.random() * 3)), toks))
    return out


def host_trie(lib, V, lexicon, smear):
    t = _capi.HostTrie(V, 0, lib=lib)
    for lab, sc, toks in lexicon:
        t.insert(toks, lab, sc)
    t.smear(smear)
    return t


def trie_nodes(t):
    """The host trie's nodes: [(children {token: node}, labels, maxScore)]."""
    L = t.L.lib
    n = t.num_nodes()
    out = []
    for i in range(n):
        nl, nc, ms = C.c_int32(0), C.c_int32(0), C.c_float(0)
        labels = np.zeros(6, np.int32)
        L.fltx_htrie_node(t.h, i, None, C.addressof(ms), C.addressof(nl), labels.ctypes.data, None,
                          C.addressof(nc), None, None, 0)
        ct = np.zeros(max(nc.value, 1), np.int32)
        cn = np.zeros(max(nc.value, 1), np.int64)
        L.fltx_htrie_node(t.h, i, None, None, None, None, None, None, ct.ctypes.data, cn.ctypes.data, nc.value)
        out.append(({int(a): int(b) for a, b in zip(ct[:nc.value], cn[:nc.value])}, labels[:nl.value].tolist(),
                    F32(ms.value)))
    return out


# ---- LM states as objects (lm/LM.h:24-34) ---------------------------------------------------------------------------
class St:
    __slots__ = ("ctx", "children")

    def __init__(self, ctx):
        self.ctx, self.children = ctx, {}


class ObjLM:
    """LM::start / score / finish over the library's LM tables (None: ZeroLM), with LMState::child objects."""

    def __init__(self, lm):
        self.lm = lm

    def start(self):
        return St(tuple(self.lm.start(False).tolist()) if self.lm is not None else ())

    def _child(self, st, usr):
        if self.lm is None:
            return st.children.setdefault(usr, St(())), F32(0.0)
        out, s = self.lm.step(np.asarray(st.ctx, np.int32), usr)
        c = st.children.get(usr)
        if c is None:
            c = st.children[usr] = St(tuple(out.tolist()))
        return c, F32(s)

    def score(self, st, usr):
        return self._child(st, usr)

    def finish(self, st):
        if self.lm is None:  # ZeroLM::finish: the same state (lm/ZeroLM.cpp:24-25)
            return st, F32(0.0)
        return self._child(st, -1)


def _fields(c):
    return (c["prev"], c["am"], c["lm"], c["word"], c["path"])


def f32sub(a, b):
    return F32(F32(a) - F32(b))


# ---- the restatement ----------------------------------------------------------------------------------------------
def restate_lex(model, nodes, lm, K, Kt, thr, lmw, word_score, eos_score, eos, maxlen, log_add, is_lm_token,
                ties=None, stats=None):
    """One utterance.  -> (final [(score, am, lm, tokens, words)], rows per step [(token, beam_idx, src_row)]).
    ties: receives (step, what) for a tie at a token-beam cut, inside a merge group, or among the kept K (a near-tie
    under 1e-9 relative where a logAdd merge fed the scores); stats: dict that counts 'merges'."""
    root = dict(score=0.0, am=0.0, lm=0.0, token=-1, word=-1, node=0, st=lm.start(), path=[], words=[], folded=False)
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

        def add(h, i, s, am, l, tok, word, node, st, src):
            cands.append(dict(score=s, am=h["am"] + am, lm=h["lm"] + float(l), token=tok, word=word, node=node, st=st,
                              prev=i, src=src, path=h["path"] + [tok], words=h["words"] + [word], folded=False))

        for i, h in enumerate(beam):
            if h["token"] == eos:
                cands.append(dict(h, prev=i, path=h["path"] + [eos], words=h["words"] + [-1], src=None, folded=False))
                continue
            r = model.row(h["path"])
            if r is None:
                continue
            V = len(r)
            order = np.argsort(-r.astype(np.float64), kind="stable")
            if ties is not None and V > Kt and r[order[Kt - 1]] == r[order[Kt]]:
                ties.append((t, "token beam"))
            idx = order[:Kt] if V > Kt else np.arange(V)
            kids, _, hmax = nodes[h["node"]]
            lex_max = F32(0.0) if h["node"] == 0 else hmax
            for n in idx.tolist():
                a = float(r[n])
                if n == eos:
                    if h["node"] == 0:
                        st, l = lm.finish(h["st"])
                        l = l if is_lm_token else f32sub(l, lex_max)
                        add(h, i, ((h["score"] + a) + eos_score) + lmw * float(l), a, l, n, -1, 0, st, row_of[i])
                    continue
                child = kids.get(n)
                if child is None:
                    continue
                if is_lm_token:
                    st, l = lm.score(h["st"], n)
                else:
                    st, l = h["st"], f32sub(nodes[child][2], lex_max)
                add(h, i, (h["score"] + a) + lmw * float(l), a, l, n, -1, child, st, row_of[i])
                for w in nodes[child][1]:
                    if not is_lm_token:
                        st, l = lm.score(h["st"], w)
                        l = f32sub(l, lex_max)
                    add(h, i, ((h["score"] + a) + word_score) + lmw * float(l), a, l, n, w, 0, st, row_of[i])
                    if is_lm_token:
                        break
        if not cands:
            beam = []
            hyps.append(beam)
            rows_per_step.append([])
            break
        best = max(c["score"] for c in cands)
        surv = [c for c in cands if c["score"] >= best - thr]
        groups = {}
        for c in surv:
            groups.setdefault((id(c["st"]), c["node"], c["token"]), []).append(c)
        merged = []
        for g in groups.values():
            g.sort(key=lambda c: -c["score"])
            if ties is not None and any(x["score"] == y["score"] and _fields(x) != _fields(y) for x, y in zip(g, g[1:])):
                ties.append((t, "merge group"))  # (equal members that differ: which one's fields survive is open)
            acc = g[0]["score"]
            for c in g[1:]:
                hi, lo = max(acc, c["score"]), min(acc, c["score"])
                acc = hi + math.log1p(math.exp(lo - hi)) if log_add else hi
            if stats is not None:
                stats["merges"] = stats.get("merges", 0) + len(g) - 1
            merged.append(dict(g[0], score=acc, folded=g[0]["folded"] or (log_add and len(g) > 1)))
        merged.sort(key=lambda c: -c["score"])
        if ties is not None:
            top = merged[:K + 1]
            for x, y in zip(top, top[1:]):
                near = (x["folded"] or y["folded"]) and abs(x["score"] - y["score"]) <= 1e-9 * abs(x["score"])
                if x["score"] == y["score"] or near:
                    ties.append((t, "beam"))
        beam = merged[:K]
        hyps.append(beam)
        t += 1
        nxt = [(c["token"], c["prev"], c["src"]) for c in beam if c["token"] != eos]
        rows_per_step.append(nxt if t < maxlen else [])
    final = next(b for b in reversed(hyps) if b)
    L = maxlen + 3
    out = []
    for h in final:
        toks, words = [-1] * L, [-1] * L
        for j, (tok, w) in enumerate(zip(reversed(h["path"]), reversed(h["words"]))):
            toks[L - 1 - j] = tok
            words[L - 1 - j] = w
        out.append((h["score"], h["am"], h["lm"], toks, words, h["folded"]))
    return out, rows_per_step


# ---- the device path ----------------------------------------------------------------------------------------------
def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def run_device(sess, models, trie, lm, K, Kt, thr, lmw, word_score, eos_score, eos, maxlen, V, log_add, is_lm_token,
               dec=None, pad="nan", fetch=True):
    """All utterances in one batch.  -> (final per utterance [(score, am, lm, tokens, words)], rows per step, merges)"""
    B = len(models)
    own = dec is None
    if own:
        opts = _capi.make_s2s_lex_options(K, Kt, thr, lmw, word_score, eos_score, log_add)
        dec = _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, opts, trie, lm if lm is not None else sess.zero, eos, maxlen,
                                               is_lm_token)
    tok, beam, src, n = dec.begin(B, V)
    prefix = {(b, 0): [] for b in range(B)}
    rows = [[] for _ in range(B)]
    gpu = is_gpu(sess)
    rng = np.random.default_rng(3)
    for t in range(maxlen + 2):  # (two steps more than it takes: a step after the last one is a no-op)
        if gpu:
            dec.ctx.synchronize()
        tok_h, beam_h, src_h, n_h = _np(tok), _np(beam), _np(src), _np(n)
        if t > 0:
            for b in range(B):
                rows[b].append([(int(tok_h[b, k]), int(beam_h[b, k]), int(src_h[b, k]) - b * K if src_h[b, k] >= 0
                                 else None) for k in range(n_h[b])])
                assert (tok_h[b, n_h[b]:] == -1).all() and (src_h[b, n_h[b]:] == -1).all()
        sc = np.full((B * K, V), np.nan, dtype=np.float32)
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
                    continue
                sc[b * K + k, :len(r)] = r
                valid[b * K + k] = 1
        prefix = newpre
        if gpu:
            import torch
            tok, beam, src, n = dec.step(torch.from_numpy(sc).cuda(), torch.from_numpy(valid).cuda())
        else:
            tok, beam, src, n = dec.step(sc, valid)
    assert dec.done()
    merges = dec.info()["merges"]
    dec.end()
    out = [[(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in dec.results(b)] for b in range(B)] \
        if fetch else None
    for b in range(B):
        while rows[b] and rows[b][-1] == []:
            rows[b].pop()
    if own:
        dec.close()
    return out, rows, merges


def compare(want, got, exact_scores=True):
    """want: restate_lex's final list; got: run_device's of one utterance.  Tokens, words exact; scores bit for bit,
    or within 1e-9 relative for a hypothesis whose score a logAdd merge fed."""
    assert len(got) == len(want), (len(got), len(want))
    for i, (w, g) in enumerate(zip(want, got)):
        assert g[3] == w[3], (i, g[3], w[3])
        assert g[4] == w[4], (i, g[4], w[4])
        if w[5] or not exact_scores:
            for x, y in zip(g[:3], w[:3]):
                assert abs(x - y) <= 1e-9 * max(1.0, abs(y)), (i, g[:3], w[:3])
        else:
            assert g[:3] == w[:3], (i, g[:3], w[:3])


class _Ties(Exception):
    """The restatement saw a tie: the reference's order decides it, nothing to reproduce."""


def check_case(sess, seeds, V, K, Kt, lexicon, smear=1, thr=1e9, lmw=0.0, word_score=0.0, eos_score=0.0, eos=None,
               maxlen=6, eos_bias=0.0, drop=0.0, lm=None, log_add=False, is_lm_token=False, pad="nan"):
    eos = V - 1 if eos is None else eos
    t = host_trie(sess.lib, V, lexicon, smear)
    nodes = trie_nodes(t)
    want, nmerge, used = [], 0, []
    for s in seeds:  # (the first seed from s on whose search the restatement sees no tie)
        for s in range(s, s + 40):
            ties, stats = [], {}
            w = restate_lex(sm_model(s, V, eos, eos_bias, drop), nodes, ObjLM(lm), K, Kt, thr, lmw, word_score,
                            eos_score, eos, maxlen, log_add, is_lm_token, ties=ties, stats=stats)
            if not ties:
                break
        if ties:
            raise _Ties(ties)
        want.append(w)
        used.append(s)
        nmerge += stats.get("merges", 0)
    seeds = used
    got, rows, merges = run_device(sess, [sm_model(s, V, eos, eos_bias, drop) for s in seeds], t, lm, K, Kt, thr, lmw,
                                   word_score, eos_score, eos, maxlen, V, log_add, is_lm_token, pad=pad)
    for b, ((wf, wr), gf, gr) in enumerate(zip(want, got, rows)):
        compare(wf, gf)
        wr = list(wr)
        while wr and wr[-1] == []:
            wr.pop()
        assert gr == wr, (b, gr, wr)
    assert sum(merges) == nmerge, (merges, nmerge)
    return nmerge


# ---- device against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("smear", [0, 1, 2])
def test_zero_lm_smearing(sess, smear):
    lex = make_lexicon(12, 11, 40, 5, respell=0.2)  # (no homophones under ZeroLM: their words tie)
    check_case(sess, [1, 2, 3], 12, 8, 12, lex, smear=smear, lmw=0.5, word_score=0.3, eos_bias=0.8, maxlen=7)


@pytest.mark.parametrize("log_add", [False, True])
def test_merges_fire(sess, log_add):
    """Multi-spelling words over a small alphabet and a wide beam: hypotheses in one LM state end the same word."""
    lex = make_lexicon(8, 7, 30, 11, max_len=3, respell=0.5, single=0.3)
    n = check_case(sess, [4, 5, 6, 7], 8, 32, 8, lex, smear=1, lmw=0.2, word_score=0.5, eos_bias=0.5, maxlen=8,
                   log_add=log_add)
    assert n > 0


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    def make(n, prefix, seed=5):
        path = str(tmp_path_factory.mktemp("lex_s2s_lm") / ("%s%d_s%d.arpa" % (prefix, n, seed)))
        vocab = ngram_synth.words(n, prefix)
        ngram_synth.write_arpa(path, vocab, 3, (0, 300, 150), seed)
        return path, vocab
    return make


@pytest.mark.parametrize("log_add", [False, True])
def test_word_ngram(sess, arpa, log_add):
    lex = make_lexicon(14, 0, 40, 21, homophones=0.15, respell=0.3)
    path, vocab = arpa(40, "w")
    lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
    check_case(sess, [8, 9], 14, 12, 14, lex, smear=1, lmw=0.8, word_score=-0.2, eos_score=-0.3, eos=0, eos_bias=0.6,
               maxlen=7, lm=lm, log_add=log_add, drop=0.05)


def test_token_lm(sess, arpa):
    lex = make_lexicon(10, 9, 30, 31, max_len=3, respell=0.3, single=0.4)
    path, vocab = arpa(10, "t")
    lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
    check_case(sess, [10, 11, 12], 10, 16, 10, lex, smear=0, lmw=0.6, word_score=0.2, eos_bias=0.5, maxlen=7, lm=lm,
               log_add=True, is_lm_token=True)
    check_case(sess, [13], 10, 16, 10, lex, smear=0, word_score=0.25, eos_bias=0.5, maxlen=6, is_lm_token=True)


def test_random_cases(sess):
    """Seeded random configurations; the restatement sees no tie (a seed with ties is skipped over)."""
    rng = np.random.default_rng(77)
    n = 20 if is_gpu(sess) else 40
    done = 0
    while done < n:
        V = int(rng.choice([5, 9, 16, 30]))
        eos = int(rng.integers(0, V))
        K = int(rng.integers(1, 40))
        Kt = int(rng.integers(1, V + 3))
        lex = make_lexicon(V, eos, int(rng.integers(5, 60)), int(rng.integers(1 << 20)), max_len=int(rng.integers(2, 5)),
                           respell=float(rng.choice([0.0, 0.3, 0.6])))
        try:
            check_case(sess, [int(rng.integers(1 << 30))], V, K, Kt, lex, smear=int(rng.integers(0, 3)),
                       thr=float(rng.choice([0.5, 3.0, 1e9])), lmw=float(rng.choice([0.0, 0.5])),
                       word_score=float(rng.choice([0.0, 0.7, -0.4])), eos_score=float(rng.choice([0.0, -0.3])),
                       eos=eos, eos_bias=float(rng.choice([0.0, 0.5])), drop=float(rng.choice([0.0, 0.1])),
                       maxlen=int(rng.integers(1, 8)), log_add=bool(rng.integers(2)), pad=str(rng.choice(["nan", "garbage"])))
        except _Ties:
            continue
        done += 1


def _large_batch(gpu_sess):
    """B = 64 with multi-spelling lexicons: K = 256 (V = 30, three steps) and K = 64 / K = 32 with logAdd merges;
    every utterance's seed tie-free."""
    for V, K, n, maxlen, log_add in ((30, 256, 300, 3, False), (12, 64, 80, 4, True), (16, 32, 120, 6, True)):
        eos = V - 1
        lex = make_lexicon(V, eos, n, 3, max_len=3, respell=0.4, single=0.3)
        seeds = _tie_free(gpu_sess, list(range(1000, 1400)), V, eos, K, V, lex, 64, maxlen=maxlen, lmw=0.3,
                          word_score=0.2, eos_bias=0.5, log_add=log_add)
        assert check_case(gpu_sess, seeds, V, K, V, lex, lmw=0.3, word_score=0.2, eos_bias=0.5, maxlen=maxlen,
                          log_add=log_add) > 0


def _tie_free(sess, cands, V, eos, K, Kt, lex, B, maxlen, lmw, word_score, eos_bias, log_add):
    nodes = trie_nodes(host_trie(sess.lib, V, lex, 1))
    out = []
    for s in cands:
        ties = []
        restate_lex(sm_model(s, V, eos, eos_bias), nodes, ObjLM(None), K, Kt, 1e9, lmw, word_score, 0.0, eos, maxlen,
                    log_add, False, ties=ties)
        if not ties:
            out.append(s)
        if len(out) == B:
            break
    assert len(out) == B
    return out


# ---- fixtures of the reference itself (tests/golden/make_lex_s2s_golden.py) ----------------------------------------
def _golden():
    import gzip
    import json
    with gzip.open(os.path.join(ROOT, "tests", "golden", "lexicon_seq2seq_expected.json.gz"), "rt") as f:
        return json.load(f)


def _golden_setup(c, d, lib):
    from golden import make_lex_s2s_golden as G
    lex = G.lexicon(c)
    t = host_trie(lib, c["V"], lex, c["smear"])
    lm = None
    if c["lm"]:
        path, vocab = G.arpa_file(str(d), c["lm"])
        lm = _capi.ArpaLM(path, vocab, lib=lib)
    return t, lm


def test_golden_covers_the_ground():
    cases = _golden()
    assert len(cases) >= 15
    assert sum(1 for c in cases if c["merges"] > 0) >= 5
    assert {c["smear"] for c in cases} == {0, 1, 2} and any(c["lm"] for c in cases) and any(not c["lm"] for c in cases)
    assert any(c["is_lm_token"] for c in cases) and any(c["word_score"] != 0 for c in cases)
    assert any(c["log_add"] and c["merges"] for c in cases) and any(not c["log_add"] and c["merges"] for c in cases)
    assert any(c["drop"] > 0 for c in cases)
    assert any(any(h[3][-1] != c["eos"] for h in c["hyps"]) for c in cases)  # (max_output_length with live hypotheses)


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c, emu_session, tmp_path):
    """The restatement against the compiled reference: tokens and words exact, the three scores bit for bit; the merge
    count as recorded, no tie."""
    t, lm = _golden_setup(c, tmp_path, emu_session.lib)
    ties, stats = [], {}
    got, _ = restate_lex(sm_model(c["seed"], c["V"], c["eos"], c["eos_bias"], c["drop"]), trie_nodes(t), ObjLM(lm),
                         c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"], c["maxlen"],
                         c["log_add"], c["is_lm_token"], ties=ties, stats=stats)
    assert not ties and stats.get("merges", 0) == c["merges"]
    assert [list(h[:5]) for h in got] == c["hyps"]


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess, tmp_path):
    """The device against the compiled reference: tokens, words and the rows of every step exactly (rows: the
    restatement's); scores bit for bit, within 1e-9 relative where a logAdd merge fed them."""
    t, lm = _golden_setup(c, tmp_path, sess.lib)
    want, wrows = restate_lex(sm_model(c["seed"], c["V"], c["eos"], c["eos_bias"], c["drop"]), trie_nodes(t),
                              ObjLM(lm), c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                              c["maxlen"], c["log_add"], c["is_lm_token"])
    got, rows, merges = run_device(sess, [sm_model(c["seed"], c["V"], c["eos"], c["eos_bias"], c["drop"])], t, lm,
                                   c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                                   c["maxlen"], c["V"], c["log_add"], c["is_lm_token"])
    ref = [tuple(h[:5]) + (w[5],) for h, w in zip(c["hyps"], want)]
    compare(ref, got[0])
    while wrows and wrows[-1] == []:
        wrows.pop()
    assert rows[0] == wrows
    assert merges == [c["merges"]]


# ---- the ABI contract -----------------------------------------------------------------------------------------------
def _rows_arrays(sess, B, K):
    if is_gpu(sess):
        import torch
        return [torch.zeros(B * K, dtype=torch.int32, device="cuda") for _ in range(3)] + \
            [torch.zeros(B, dtype=torch.int32, device="cuda")]
    return [np.zeros(B * K, np.int32) for _ in range(3)] + [np.zeros(B, np.int32)]


def _addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def test_limits_and_refusals(sess):
    L, ctx = sess.lib, sess.ctx
    t = host_trie(L, 10, make_lexicon(10, 9, 20, 1), 1)
    h = C.c_void_p()

    def create(opts, lm=None, eos=9, maxlen=5, trie=t):
        return L.lib.fltx_s2s_lex_decoder_create(ctx.h, C.byref(opts), trie.h if trie else None, (lm or sess.zero).h,
                                                 eos, maxlen, 0, C.byref(h))
    assert create(_capi.make_s2s_lex_options(257, 4)) == _capi.ERR_UNSUPPORTED
    assert create(_capi.make_s2s_lex_options(4, 4), maxlen=4097) == _capi.ERR_UNSUPPORTED
    assert create(_capi.make_s2s_lex_options(0, 4)) == _capi.ERR_INVALID
    assert create(_capi.make_s2s_lex_options(4, 4), trie=None) == _capi.ERR_INVALID

    class Lm:
        def start(self, start_with_nothing):
            return 0

        def score(self, state, idx):
            return state, 0.0

        def finish(self, state):
            return state, 0.0
    assert create(_capi.make_s2s_lex_options(4, 4), lm=_capi.HostLM(Lm(), lib=L)) == _capi.ERR_UNSUPPORTED
    assert "host" in L.lib.fltx_last_error().decode()
    out = _rows_arrays(sess, 2, 4)
    dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(4, 300), t, sess.zero, 9, 5)
    assert L.lib.fltx_s2s_begin(dec.h, 2, 65537, *[_addr(o) for o in out]) == _capi.ERR_UNSUPPORTED
    assert L.lib.fltx_s2s_begin(dec.h, 2, 1000, *[_addr(o) for o in out]) == _capi.ERR_UNSUPPORTED  # (Kt 300 > 256)
    assert L.lib.fltx_s2s_begin(dec.h, 2, 256, *[_addr(o) for o in out]) == _capi.FLTX_OK
    dec.close()
    for V, Kt in ((64, 64), (10000, 50)):  # (Kt = V for V <= 64, Kt = 50 at V = 10 000)
        dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(4, Kt), t, sess.zero, 9, 5)
        assert L.lib.fltx_s2s_begin(dec.h, 2, V, *[_addr(o) for o in out]) == _capi.FLTX_OK
        dec.close()
    T_ = np.array([2], np.int32)
    e = np.zeros(8, np.float32)
    dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(4, 4), t, sess.zero, 9, 5)
    assert L.lib.fltx_decode_batch(dec.h, e.ctypes.data, 0, None, T_.ctypes.data, 1, 4) == _capi.ERR_STATE
    assert L.lib.fltx_stream_begin(dec.h, 1, 4, 10) == _capi.ERR_STATE
    dec.close()


def test_full_state_table_is_reported(sess):
    """A table of 3 LM states: an utterance that needs more stops and says so (never a silent wrong merge); with the
    default table the same decode completes."""
    V, eos = 8, 7
    lex = make_lexicon(V, eos, 30, 11, max_len=3, respell=0.5, single=0.6)
    t = host_trie(sess.lib, V, lex, 1)
    dec = _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_lex_options(8, 8, 1e9, 0.2, 0.5), t, sess.zero,
                                           eos, 6)
    dec.set_max_states(3)
    models = [sm_model(5, V, eos, 0.5)]
    run_device(sess, models, t, None, 8, 8, 1e9, 0.2, 0.5, 0.0, eos, 6, V, False, False, dec=dec, fetch=False)
    with pytest.raises(_capi.FltxError, match="LM-state table full"):
        dec.results(0)
    dec.set_max_states(1 << 16)
    got, _, _ = run_device(sess, models, t, None, 8, 8, 1e9, 0.2, 0.5, 0.0, eos, 6, V, False, False, dec=dec)
    assert len(got[0]) == 8
    dec.close()


def test_restart_and_step_after_done(sess):
    """Beginning again after a step restarts from the root; a step after done lists no rows and changes nothing."""
    V, eos = 12, 11
    lex = make_lexicon(V, eos, 40, 5, respell=0.2)
    t = host_trie(sess.lib, V, lex, 1)
    nodes = trie_nodes(t)
    want, _ = restate_lex(sm_model(1, V, eos, 0.8), nodes, ObjLM(None), 8, 12, 1e9, 0.5, 0.3, 0.0, eos, 7, False,
                          False)
    dec = _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_lex_options(8, 12, 1e9, 0.5, 0.3), t, sess.zero,
                                           eos, 7)
    dec.begin(1, V)
    dec.step(sm_model(1, V, eos, 0.8).row([])[None, :].repeat(8, 0))
    for _ in range(2):
        got, _, _ = run_device(sess, [sm_model(1, V, eos, 0.8)], t, None, 8, 12, 1e9, 0.5, 0.3, 0.0, eos, 7, V, False,
                               False, dec=dec)
        compare(want, got[0])
    tok, beam, src, n = (_np(x) for x in dec.step(np.zeros((8, V), np.float32)))
    assert n.tolist() == [0] and (tok == -1).all()
    dec.end()
    assert [(h.score, h.tokens.tolist(), h.words.tolist()) for h in dec.results(0)] == \
        [(w[0], w[3], w[4]) for w in want]
    dec.close()


def test_word_piece_trie_uploads_compact(sess):
    """A 50k-word word-piece lexicon at V = 10 000: the device trie holds nodes, edges and labels only (the dense
    edge table of fltx_htrie_upload would be nodes x V x 16 B)."""
    rng = np.random.default_rng(1)
    V, eos = 10000, 2
    t = _capi.HostTrie(V, 0, lib=sess.lib)
    n_words = 50000 if is_gpu(sess) else 5000
    spellings = {}
    for w in range(n_words):
        toks = rng.integers(3, V, size=int(rng.integers(1, 4)))
        t.insert(toks, w, float(F32(-rng.random())))
        spellings[tuple(toks.tolist())] = spellings.get(tuple(toks.tolist()), 0) + 1
    n_labels = sum(min(c, 6) for c in spellings.values())  # (Trie.cpp:40-46: at most 6 labels per node)
    t.smear(1)
    dec = _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_lex_options(4, 50), t, sess.zero, eos, 5)
    info = dec.info()
    nodes = t.num_nodes()
    assert info["nodes"] == nodes and info["edges"] == nodes - 1
    assert info["trie_bytes"] == 12 * nodes + 8 + 8 * (nodes - 1) + 4 * n_labels
    assert info["trie_bytes"] < nodes * 64
    dec.close()


# ---- the reference's Python surface (text_amd/compat: flashlight.lib.text.decoder) --------------------------------
COMPAT = os.path.join(ROOT, "text_amd", "compat")


def test_compat_options_pickle():
    if COMPAT not in sys.path:
        sys.path.insert(0, COMPAT)
    import pickle
    from flashlight.lib.text.decoder import LexiconSeq2SeqDecoder, LexiconSeq2SeqDecoderOptions  # noqa: F401
    o = LexiconSeq2SeqDecoderOptions(beam_size=2, beam_size_token=4, beam_threshold=1000.0, lm_weight=0.5,
                                     word_score=0.25, eos_score=-1.5, log_add=True)
    o2 = pickle.loads(pickle.dumps(o))
    assert (o2.beam_size, o2.beam_size_token, o2.beam_threshold, o2.lm_weight, o2.word_score, o2.eos_score,
            o2.log_add) == (2, 4, 1000.0, 0.5, 0.25, -1.5, True)


def _reference_python_flow(gpu_sess):
    """The reference binding's flow through the compat names: keywords (lm takes the Trie, trie the LM, as the binding
    names them), update_func sees -1 beam indices, words in get_all_final_hypothesis; against the restatement."""
    if COMPAT not in sys.path:
        sys.path.insert(0, COMPAT)
    from flashlight.lib.text.decoder import (LexiconSeq2SeqDecoder, LexiconSeq2SeqDecoderOptions, SmearingMode, Trie,
                                             ZeroLM, create_emitting_model_state, get_obj_from_emitting_model_state)
    V, eos, K, maxlen = 12, 11, 8, 7
    lex = make_lexicon(V, eos, 40, 5, respell=0.2)
    trie = Trie(V, 0)
    for lab, sc, toks in lex:
        trie.insert(toks, lab, sc)
    trie.smear(SmearingMode.MAX)
    model = sm_model(1, V, eos, 0.8)
    seen = []

    def update_func(emissions_ptr, n, t_, tok, beam, states, timestep):
        seen.append(list(beam))
        prefixes = [[] if s is None else get_obj_from_emitting_model_state(s) for s in states]
        if timestep > 0:
            prefixes = [p + [y] for p, y in zip(prefixes, tok)]
        rows = [model.row(p) for p in prefixes]
        return [r.tolist() for r in rows], [create_emitting_model_state(p) for p in prefixes]

    opts = LexiconSeq2SeqDecoderOptions(beam_size=K, beam_size_token=12, beam_threshold=1e9, lm_weight=0.5,
                                        word_score=0.3, eos_score=0.0, log_add=False)
    dec = LexiconSeq2SeqDecoder(options=opts, lm=trie, trie=ZeroLM(), eos_idx=eos, update_func=update_func,
                                max_output_length=maxlen, is_token_lm=False)
    em = np.zeros(4, np.float32)
    dec.decode_step(em.ctypes.data, 1, V)
    assert all(b == [-1] * len(b) for b in seen) and len(seen) > 2
    ref = _capi.HostTrie(V, 0, lib=gpu_sess.lib)
    for lab, sc, toks in lex:
        ref.insert(toks, lab, sc)
    ref.smear(1)
    want, _ = restate_lex(sm_model(1, V, eos, 0.8), trie_nodes(ref), ObjLM(None), K, 12, 1e9, 0.5, 0.3, 0.0, eos,
                          maxlen, False, False)
    hyps = dec.get_all_final_hypothesis()
    assert [(h.score, h.tokens, h.words) for h in hyps] == [(w[0], w[3], w[4]) for w in want]
    assert any(w >= 0 for h in hyps for w in h.words)
    assert dec.get_best_hypothesis().tokens == hyps[0].tokens and dec.prune() is None


def _torch_model_decode_loop(gpu_session):
    """LexiconSeq2SeqBatchDecoder.decode with a tiny torch model (an embedding and a hidden state gathered by
    src_row, elementwise float32 arithmetic) against the restatement on the same model's outputs."""
    import torch
    B, K, Kt, V, eos, maxlen = 8, 8, 12, 12, 11, 7
    g = np.random.default_rng(5)
    E = g.standard_normal((V + 1, V)).astype(np.float32)
    E[:, eos] += np.float32(0.3)
    H0 = g.standard_normal((B, V)).astype(np.float32)
    half = np.float32(0.5)
    lex = make_lexicon(V, eos, 40, 5, respell=0.2)

    class Ref:
        def __init__(self, b):
            self.b = b

        def row(self, prefix):
            h = H0[self.b].copy()
            for tok in [-1] + list(prefix):
                h = h * half + E[tok if tok >= 0 else V]
            return h

    stream = torch.cuda.Stream()
    prev_stream = torch.cuda.current_stream()
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream, lib=gpu_session.lib)
    t = host_trie(gpu_session.lib, V, lex, 1)
    want = [restate_lex(Ref(b), trie_nodes(t), ObjLM(None), K, Kt, 1e9, 0.5, 0.3, 0.0, eos, maxlen, True, False)[0]
            for b in range(B)]
    dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(K, Kt, 1e9, 0.5, 0.3, 0.0, True), t,
                                           _capi.ZeroLM(ctx), eos, maxlen)
    Et = torch.from_numpy(E).cuda()
    state = {"h": torch.from_numpy(np.repeat(H0, K, axis=0)).cuda()}

    def step_fn(token, src_row, row_mask, t_):
        if t_ > 0:
            state["h"] = state["h"].index_select(0, src_row.clamp(min=0).long())
        tok = torch.where(token >= 0, token, torch.full_like(token, V)).long()
        state["h"] = torch.add(state["h"].mul(0.5), Et.index_select(0, tok))
        return state["h"]

    try:
        got = dec.decode(step_fn, B, V)
    finally:
        torch.cuda.set_stream(prev_stream)
    for b in range(B):
        compare(want[b], [(h.score, h.am, h.lm, list(h.tokens), list(h.words)) for h in got[b]])
    dec.close()
    ctx.close()


if CHILD:  # (GPU-only cases: defined in the child alone)
    test_large_batch = pytest.mark.gpu(_large_batch)
    test_reference_python_flow = pytest.mark.gpu(_reference_python_flow)
    test_torch_model_decode_loop = pytest.mark.gpu(_torch_model_decode_loop)


@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_S2S_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
