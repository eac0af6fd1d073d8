"""Lexicon CTC shallow fusion with a rows LM (fltx_ctc_rows_lex_decoder_create, text_amd/csrc/fltx_ctc_rows_lex.h): a
word-level rows LM, or a token-level one with is_lm_token.

The decoder is stepped by fltx_ctc_rows_begin / step / end; it lists for every hypothesis its parent's row, the LM edge
(word or token) that made its LM state and a canonical state id.  The checks: the compiled reference's fixtures (tests/
golden/make_lex_ctc_lm_rows_golden.py: the float64 restatement below reproduces them, the device reproduces them --
tokens and words exact, the three scores bit-identical under max-merge and within 1e-5 under logAdd); the n-gram device
decode of fltx_decode_batch on the lexicon decoder as a bit-for-bit cross-check, on a lane engine and on the generic one;
random batches, the row contract, lm_row_of, typed LM rows, the NaN and -inf rules, the state-table limit, the ABI's
contract and refusals, and the Python helper.

The restatement (`restate`) carries the word (or token) prefix as the LM state and counts its own ties -- equal emissions
at the token cut, equal scores at the K cut, among merge members and in the final order -- and the smallest gap at any
decision taken on scores (test_ctc_lm_rows.Stats / _store, shared).  Every seeded case asserts zero ties on the
restatement alone, every logAdd case a smallest gap above 1e-3.

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

from text_amd import _capi, ngram_synth  # noqa: E402

CHILD = os.environ.get("FLTX_LEX_CTC_LMROWS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

import engine_choices  # noqa: E402,F401  (the selection switches of the n-gram cross-check are its "sw/" ones)
import test_ctc_lm_rows as C0  # noqa: E402
from golden import make_lex_ctc_lm_rows_golden as G  # noqa: E402
from test_ctc_lm_rows import MIN_GAP, LOGADD_TOL, PrefixLM, Stats, TypedFeed, _dev  # noqa: E402,F401
from test_lexicon_seq2seq import host_trie, trie_nodes  # noqa: E402
from test_seq2seq import HostLM  # noqa: E402
from test_seq2seq_model_output import BF16, F16, F32, _bits_equal, _GpuSess, _np, is_gpu  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
NINF = -float("inf")
SMEAR_MAX = 1


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


# ---- 1. the restatement -----------------------------------------------------------------------------------------------
def opts(K, Kt, thr=25.0, lmw=0.7, word_score=0.0, unk_score=NINF, sil_score=0.0, sil=0, blank=1, unk=-1, log_add=False,
         is_lm_token=False):
    return dict(K=K, Kt=Kt, thr=thr, lmw=lmw, word_score=word_score, unk_score=unk_score, sil_score=sil_score, sil=sil,
                blank=blank, unk=unk, log_add=log_add, is_lm_token=is_lm_token)


def _fsub(a, b):
    """float32 a - float32 b, as a Python float"""
    with np.errstate(invalid="ignore"):
        return float(np.float32(a) - np.float32(b))


def restate(em, nodes, lm, o, st=None, hole=None):
    """LexiconDecoder.cpp:32-274 on one utterance: em [T, N] float32, nodes as trie_nodes gives them, lm a PrefixLM over
    words (tokens with is_lm_token).  -> (final [(score, am, lm, tokens, words)], rows per frame [(src, edge, state)]:
    the beam after each frame, best first, state = the prefix of edges).  hole = (t, i): hypothesis i of the beam that
    frame t extends reads NaN LM entries (an lm_row_of entry out of range).  st also counts what the fixtures' cases are
    there to show (guard, outside, label_and_kids, unk, smear).  o["mut"] names one rule to BREAK (see MUTATIONS): a
    case shows a rule when breaking it changes the case's final n-best."""
    st = st if st is not None else Stats()
    for f in ("guard", "outside", "label_and_kids", "unk", "smear"):
        setattr(st, f, getattr(st, f, 0))
    T, N = em.shape
    K, Kt, thr, lmw, sil, blank, tokl = o["K"], o["Kt"], o["thr"], o["lmw"], o["sil"], o["blank"], o["is_lm_token"]
    mut = o.get("mut", "")
    beam = [dict(score=0.0, am=0.0, lm=0.0, state=lm.start(), node=0, token=sil, pb=False, path=[sil], words=[-1])]
    seen = {beam[0]["state"]}
    rows = []
    for t in range(T):
        e = em[t]
        order = sorted((n for n in range(N) if not np.isnan(e[n])), key=lambda n: (-float(e[n]), n))
        kt = min(Kt, N)
        if len(order) > kt and e[order[kt - 1]] == e[order[kt]]:
            st.ties.append((t, "token cut"))
        kept = sorted(order[:kt])
        cands = []

        def add(h, i, score, a, l, state, node, n, word, pb, edge):
            if math.isnan(score):
                return
            cands.append(dict(score=score, am=h["am"] + a, lm=h["lm"] + l if l is not None else h["lm"], state=state,
                              node=node, token=n, pb=pb, src=i, edge=edge, key=(state, node, n, pb), path=h["path"] + [n],
                              words=h["words"] + [word]))
        for i, h in enumerate(beam):
            kids_h = nodes[h["node"]][0]
            lex_max = 0.0 if h["node"] == 0 or mut == "smear" else float(nodes[h["node"]][2])
            nan_row = hole == (t, i)
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
                    l_n = math.nan if nan_row else l_n
                kids, labels, ms = nodes[c]
                ms = 0.0 if mut == "smear" else ms
                new_tok = h["pb"] or n != h["token"]
                if new_tok and kids and not (mut == "label_and_kids" and labels):
                    if tokl:
                        add(h, i, s + lmw * l_n, a, l_n, state_n, c, n, -1, False, n)
                    else:
                        l = _fsub(ms, lex_max)
                        st.smear += l != 0.0
                        add(h, i, s + lmw * l, a, l, h["state"], c, n, -1, False, -1)
                    st.label_and_kids += bool(labels)
                ends = [(w, o["word_score"]) for w in labels]
                if ends and h["node"] == 0 and h["token"] == n:
                    st.guard += 1
                    ends = ends if mut == "guard" else []
                if mut == "repeat_end" and not new_tok:
                    ends = []
                if not labels and o["unk_score"] > NINF and mut != "unk":
                    ends = [(o["unk"], o["unk_score"])]
                for w, ws in ends:
                    if tokl:
                        state, l = state_n, l_n
                    else:
                        state, l = lm.score(h["state"], w)
                        l = _fsub(math.nan if nan_row else l, lex_max)
                    add(h, i, (s + lmw * l) + ws, a, l, state, 0, n, w, False, n if tokl else w)
            if not h["pb"] or h["node"] == 0:
                n = sil if h["node"] == 0 else h["token"]
                st.outside += n not in kept
                a = float(e[n])
                s = h["score"] + a
                if n == sil:
                    s += o["sil_score"]
                if mut != "outside" or n in kept:
                    add(h, i, s, a, None, h["state"], h["node"], n, -1, False, -1)
            st.outside += blank not in kept
            a = float(e[blank])
            if mut != "outside" or blank in kept:
                add(h, i, h["score"] + a, a, None, h["state"], h["node"], blank, -1, True, -1)
        beam = C0._store(cands, K, thr, o["log_add"], st, t)
        for c in beam:
            if c["edge"] != -1 and c["state"] in seen:
                st.reentered += 1
        seen.update(c["state"] for c in beam)
        rows.append([(c["src"], c["edge"], c["state"]) for c in beam])
    cands = []
    nice = any(h["node"] == 0 for h in beam)
    for i, h in enumerate(beam):
        if nice and h["node"] != 0:
            continue
        state, l = lm.finish(h["state"])
        score = h["score"] + lmw * l
        if not math.isnan(score):
            cands.append(dict(score=score, am=h["am"], lm=h["lm"] + l, key=(state, h["node"], sil, False),
                              path=h["path"] + [sil], words=h["words"] + [-1]))
    final = C0._store(cands, K, thr, o["log_add"], st, "end")
    st.unk += sum(o["unk"] in c["words"] for c in final) if o["unk_score"] > NINF else 0
    st.no_root_end = not nice
    return [(c["score"], c["am"], c["lm"], c["path"], c["words"]) for c in final], rows


# a rule of the search, broken: the restatement under o["mut"] (or with these options changed) must give another n-best
MUTATIONS = {"guard": dict(mut="guard"),                    # the root guard (:114-122) removed
             "repeat_end": dict(mut="repeat_end"),          # word ends put under the move's condition
             "smear": dict(mut="smear"),                    # every maxScore 0
             "outside": dict(mut="outside"),                # same node and blank only when their token is in the beam
             "label_and_kids": dict(mut="label_and_kids"),  # no move into a node that also ends a word
             "unk": dict(mut="unk"),                        # no unknown word
             "tight_thr": dict(thr=25.0),
             "scores": dict(sil_score=0.0, word_score=0.0)}


def shows(need, st, final, rerun=None):
    """what a fixture's case is there to show, shown in its final n-best on this seed.  need: names joined by commas;
    rerun(changed options) -> the final n-best of the case with them"""
    for nd in filter(None, need.split(",")):
        if nd == "both_labels":  # two hypotheses with the same tokens and different words
            seen = {}
            ok = any(seen.setdefault(tuple(h[3]), tuple(h[4])) != tuple(h[4]) for h in final)
        elif nd == "words":  # a word in the n-best
            ok = any(w >= 0 for h in final for w in h[4])
        elif nd == "merges":
            ok = st.merges >= 1
        elif nd == "no_root_end":
            ok = bool(st.no_root_end)
        else:
            other = rerun(MUTATIONS[nd])
            ok = [(h[0], list(h[3]), list(h[4])) for h in other] != [(h[0], list(h[3]), list(h[4])) for h in final]
            ok = ok and (nd not in ("guard", "outside", "label_and_kids", "unk", "smear") or bool(getattr(st, nd)))
        if not ok:
            return False
    return True


def assert_final(want, got, log_add, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (w, g) in enumerate(zip(want, got)):
        assert list(g[3]) == list(w[3]) and list(g[4]) == list(w[4]), (what, i, g[3:], w[3:])
        if log_add:
            assert all(abs(x - y) <= LOGADD_TOL for x, y in zip(g[:3], w[:3])), (what, i, g[:3], w[:3])
        else:
            assert _bits_equal(g[:3], w[:3]), (what, i, g[:3], w[:3])


def assert_rows(want_rows, got_rows, prefix):
    """per frame and slot: the parent's slot and the edge equal; the state ids name the restatement's states one to one"""
    assert len(got_rows) == len(want_rows)
    fwd, back = {}, {}
    for t, (wr, gr) in enumerate(zip(want_rows, got_rows)):
        assert len(gr) == len(wr), (t, len(gr), len(wr))
        for k, (w, g) in enumerate(zip(wr, gr)):
            assert g[:2] == w[:2], (t, k, g, w)
            assert fwd.setdefault(g[2], w[2]) == w[2] and back.setdefault(w[2], g[2]) == g[2], (t, k, g, w)
            assert prefix[g[2]] == w[2], (t, k)


def clean(case_fn, base, log_add, tries=400, need=""):
    """the first seed from `base` whose restatement has no tie (and, under logAdd, no gap below MIN_GAP)
    -> (seed, inputs, result, stats)"""
    for seed in range(base, base + tries):
        st = Stats()
        inp = case_fn(seed)
        res = restate(*inp, st=st)
        if not st.ties and (not log_add or st.gap > MIN_GAP) and \
                shows(need, st, res[0], lambda ch: restate(inp[0], inp[1], inp[2], dict(inp[3], **ch))[0]):
            return seed, inp, res, st
    raise AssertionError("no clean seed in %d tries from %d" % (tries, base))


# ---- the device loop ---------------------------------------------------------------------------------------------------
class Lex:
    """a lexicon [(label, score, spelling)] as the host trie of a library and as the restatement's nodes"""

    def __init__(self, lib, N, sil, lex, smear=SMEAR_MAX):
        self.trie = _capi.HostTrie(N, sil, lib=lib)
        for lab, sc, toks in lex:
            self.trie.insert(toks, lab, sc)
        if smear:
            self.trie.smear(smear)
        self.nodes = trie_nodes(self.trie)

    def close(self):
        self.trie.close()


def make_dec(sess, lex, lm, o):
    return _capi.LexiconCtcRowsBatchDecoder(
        sess.ctx, _capi.make_options(o["K"], o["Kt"], o["thr"], o["lmw"], o["word_score"], o["unk_score"], o["sil_score"],
                                     o["log_add"]), lex.trie, lm, o["sil"], o["blank"], o["unk"], o["is_lm_token"])


def decode(sess, dec, ems, N, W, lm_row, per_state=False, feed=None, extra_steps=2, bad_rows=()):
    """test_ctc_lm_rows.decode for this decoder: the root row lists no edge, a row's edge is a word or a token, and the
    results carry words.  -> (final per utterance [(score, am, lm, tokens, words)], rows per frame per utterance
    [(src, edge, state id)], the prefix of every state id per utterance -- rebuilt from (src_row, token, state) alone)"""
    B, K = len(ems), int(dec.options.beam_size)
    Ts = [e.shape[0] for e in ems]
    flat = np.concatenate([e.reshape(-1) for e in ems]) if sum(Ts) else np.zeros(0, np.float32)
    tok, src, state, n = dec.begin(flat, Ts, N)
    gpu = is_gpu(sess)
    prefix = [dict() for _ in range(B)]
    rows = [[] for _ in range(B)]
    prev_state = prev_n = None
    max_t = max(Ts)
    for t in range(max_t + extra_steps + 1):
        if gpu:
            dec.ctx.synchronize()
        tok_h, src_h, st_h, n_h = _np(tok).copy(), _np(src).copy(), _np(state).copy(), _np(n).copy()
        for b in range(B):
            nb = int(n_h[b])
            assert (tok_h[b, nb:] == -1).all() and (src_h[b, nb:] == -1).all() and (st_h[b, nb:] == -1).all(), (t, b)
            for k in range(nb):
                sid, s = int(st_h[b, k]), int(src_h[b, k])
                if t == 0:
                    assert (s, int(tok_h[b, k]), sid, nb) == (-1, -1, 0, 1)
                    prefix[b][sid] = ()
                    continue
                assert b * K <= s < b * K + K, (t, b, k, s)
                par = int(prev_state[b, s - b * K])
                p = prefix[b][par] + (int(tok_h[b, k]),) if tok_h[b, k] >= 0 else prefix[b][par]
                if tok_h[b, k] < 0:
                    assert sid == par, (t, b, k)
                assert prefix[b].setdefault(sid, p) == p, (t, b, k, "one id, two states")
            if 0 < t <= Ts[b]:
                rows[b].append([(int(src_h[b, k]) - b * K, int(tok_h[b, k]), int(st_h[b, k])) for k in range(nb)])
            elif t > Ts[b] and t > 0:  # no frames left: the beam listed again, unchanged
                assert (src_h[b, :nb] == b * K + np.arange(nb)).all() and (tok_h[b, :nb] == -1).all(), (t, b)
                assert (st_h[b, :nb] == prev_state[b, :nb]).all() and nb == int(prev_n[b]), (t, b)
        prev_state, prev_n = st_h, n_h
        if per_state:
            keys = sorted({(b, int(st_h[b, k])) for b in range(B) for k in range(int(n_h[b]))})
            at = {key: i for i, key in enumerate(keys)}
            lr = np.stack([lm_row(b, prefix[b][sid]) for b, sid in keys]).astype(np.float32)
            ro = np.full(B * K, -1, np.int32)
            for b in range(B):
                for k in range(int(n_h[b])):
                    ro[b * K + k] = at[(b, int(st_h[b, k]))]
        else:
            lr = np.full((B * K, W), np.nan, np.float32)
            for b in range(B):
                for k in range(int(n_h[b])):
                    lr[b * K + k] = lm_row(b, prefix[b][int(st_h[b, k])])
            ro = None
        for (tf, b, k) in bad_rows:
            if tf == t:
                ro = np.arange(B * K, dtype=np.int32) if ro is None else ro
                ro[b * K + k] = len(lr) + 5
        end = t == max_t + extra_steps
        if feed is not None:
            scored = np.zeros(B * K, bool)
            for b in range(B):
                if end or t < Ts[b]:
                    scored[b * K:b * K + int(n_h[b])] = True
            out = feed(dec, lr, ro, end, scored)
        elif end:
            out = dec.end(_dev(sess, lr), lm_row_of=None if ro is None else _dev(sess, ro))
        else:
            out = dec.step(_dev(sess, lr), lm_row_of=None if ro is None else _dev(sess, ro))
        if not end:
            tok, src, state, n = out
    final = []
    for b in range(B):
        hs = dec.results(b)
        final.append([(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in hs])
        assert all(len(h.tokens) == Ts[b] + 2 and len(h.words) == Ts[b] + 2 for h in hs)
    return final, rows, prefix


def dev_lm(sess, rl, o, mapped=True):
    """the library's LM object for a rows LM of the golden module"""
    cls = _capi.RowsLM if o["is_lm_token"] else _capi.WordRowsLM
    return cls(rl.W, rl.usr_to_lm if mapped else None, rl.finish, lib=sess.lib)


# ---- 2. fixtures of the reference itself ------------------------------------------------------------------------------
def _golden():
    path = os.path.join(ROOT, "tests", "golden", "lex_ctc_lm_rows_expected.json.gz")
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


def case_restate(c, st, seed=None, changed=None):
    seed = c["seed"] if seed is None else seed
    rl = G.case_lm(c, seed)
    lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
    return restate(G.emissions(seed, c["T"], c["N"]), case_nodes(c), lm, dict(case_opts(c), **(changed or {})), st=st)


def test_fixtures_cover_the_cases():
    cs = _golden()
    assert [c["name"] for c in cs] == [c["name"] for c in G.all_cases()] and len(cs) >= 28
    assert all(c["N"] <= 6 and c["T"] <= 12 and c["K"] <= 8 for c in cs)
    for tok in (0, 1):
        ct = [c for c in cs if c["is_lm_token"] == tok]
        assert any(c["T"] == 1 and c["K"] == 1 for c in ct) and any(c["Kt"] < c["N"] for c in ct)
        assert any(c["thr"] < 2 for c in ct) and any(c["sil_score"] != 0 and c["word_score"] != 0 for c in ct)
        assert any(c["lmw"] == 0 for c in ct) and any(c["unk_score"] > NINF for c in ct) and any(c["log_add"] for c in ct)
        assert any(c["perm"] and c["W"] > c["n_map"] for c in ct)
        needs = {nd for c in ct for nd in c["need"].split(",")}
        assert {"guard", "repeat_end", "label_and_kids", "outside", "unk", "no_root_end", "merges", "tight_thr", "scores",
                "words"} <= needs
    assert {"both_labels", "smear"} <= {nd for c in cs if not c["is_lm_token"] for nd in c["need"].split(",")}


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c):
    st = Stats()
    got, _ = case_restate(c, st)
    assert not st.ties and (not c["log_add"] or st.gap > MIN_GAP), (st.ties, st.gap)
    assert shows(c["need"], st, got, lambda ch: case_restate(c, Stats(), changed=ch)[0]), c["need"]
    assert_final(c["hyps"], got, c["log_add"], c["name"])


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess):
    o = case_opts(c)
    rl = G.case_lm(c)
    lx = Lex(sess.lib, c["N"], c["sil"], c["lex"], 0 if c["is_lm_token"] else SMEAR_MAX)
    lm = dev_lm(sess, rl, o, mapped=bool(c["perm"]))
    dec = make_dec(sess, lx, lm, o)
    got, _, _ = decode(sess, dec, [G.emissions(c["seed"], c["T"], c["N"])], c["N"], rl.W, lambda b, p: rl.row(list(p)))
    assert_final(c["hyps"], got[0], c["log_add"], c["name"])
    for d in (dec, lm, lx):
        d.close()


# ---- 3. the n-gram cross-check ----------------------------------------------------------------------------------------
LEX_X = [(0, [2]), (1, [2, 3]), (2, [3, 2]), (3, [3, 2]), (4, [4, 5, 2]), (5, [5])]  # (word, spelling); N = 6
# the shape the lexicon lane engines take (fltx_ylane.h): every word ends in sil, so labels sit behind that one token
LEX_LANE = [(w, sp + [0]) for w, sp in LEX_X]
GENERIC = {"slane": 0, "xlane": 0, "ylane": 0, "lane": 0}
LANE_ENGINES = (4, 5, 6)


@pytest.fixture(scope="module")
def arpas(tmp_path_factory):
    d = tmp_path_factory.mktemp("lex_ctc_lmrows")
    out = {}
    for name, n, seed in (("word", 6, 7), ("tok", 6, 5)):
        path = str(d / ("%s.arpa" % name))
        vocab = ngram_synth.words(n, name[0])
        ngram_synth.write_arpa(path, vocab, 3, (0, 30, 60), seed)
        out[name] = (path, vocab)
    return out


@pytest.mark.parametrize("tokl,engine", [(False, "lane"), (False, "generic"), (True, "generic")],
                         ids=["word-lane", "word-generic", "token-generic"])
def test_equals_the_ngram_device_decode(sess, arpas, tokl, engine):
    """LM rows computed on the host from a 3-gram (fltx_lm_start / fltx_lm_step, finish into finish_index) and the trie
    smeared with it: fltx_decode_batch on the lexicon decoder with that LM gives the same n-best bit for bit.  The word
    LM runs against a lane engine (K = 8, words ending in sil: the decode must report engine 4 - 6 and why_not_lane 0)
    and against the generic engine.  A token n-gram on the lexicon decoder never takes a lane engine
    (FLTX_WHY_LM), so the token LM has the generic leg alone."""
    N, K, sil, blank = 6, 8, 0, 1
    path, vocab = arpas["tok" if tokl else "word"]
    ng = _capi.ArpaLM(path, vocab, lib=sess.lib)
    hl = HostLM(ng)
    nv = 6  # words, or tokens
    lex_words = [(w, sp) for w, sp in (LEX_LANE if engine == "lane" else LEX_X)
                 if not (tokl and w == 3)]  # (a token LM: both labels of a node would tie)
    lex = [(w, 0.0 if tokl else hl.score(hl.start(), w)[1], sp) for w, sp in lex_words]
    lx = Lex(sess.lib, N, sil, lex, SMEAR_MAX)
    o = opts(K, N, 25.0, 0.7, 0.5, NINF, -0.3, sil, blank, -1, False, tokl)
    memo = {}

    def lm_row(b, p):
        if p not in memo:
            c = hl.start()
            for edge in p:
                c = hl.score(c, edge)[0]
            memo[p] = np.asarray([hl.score(c, v)[1] for v in range(nv)] + [hl.finish(c)[1]], np.float32)
        return memo[p]

    for seed in range(4300, 4500):  # a seed whose utterances have no tie in the restatement
        ems = [G.emissions(seed + 7 * b, T, N) for b, T in enumerate((5, 9, 12))]
        ok = True
        for e in ems:
            st = Stats()
            restate(e, lx.nodes, PrefixLM(lambda p: lm_row(0, p), np.arange(nv), nv), o, st=st)
            ok = ok and not st.ties
        if ok:
            break
    assert ok
    ref = _capi.BatchDecoder(sess.ctx, _capi.LEXICON, _capi.make_options(K, N, 25.0, 0.7, 0.5, sil_score=-0.3), ng, sil,
                             blank, -1, trie=lx.trie.upload(sess.ctx), is_lm_token=tokl)
    if engine == "generic":
        for k, v in GENERIC.items():
            ref.set(k, v)
    ref.decode_batch(np.concatenate([e.reshape(-1) for e in ems]), [e.shape[0] for e in ems], N)
    if engine == "lane":
        assert ref.get("why_not_lane") == 0 and ref.get("engine") in LANE_ENGINES, (ref.get("why_not_lane"),
                                                                                    ref.get("engine"))
    else:
        assert ref.get("engine") not in LANE_ENGINES and not ref.get("ylane") and not ref.get("xlane")
    lm = (_capi.RowsLM if tokl else _capi.WordRowsLM)(nv + 1, None, nv, lib=sess.lib)
    dec = make_dec(sess, lx, lm, o)
    got, _, _ = decode(sess, dec, ems, N, nv + 1, lm_row, per_state=True)
    for b in range(len(ems)):
        want = [(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in ref.results(b)]
        assert len(want) > 1
        assert_final(want, got[b], False, b)
    for d in (dec, ref, lm, ng, lx):
        d.close()


# ---- 4. random batches against the restatement; 5. the row contract ----------------------------------------------------
def rand_lex(N, n_words, seed, max_len=3, first=2):
    """n_words spellings over the letters first .. N-1 from a small generator (duplicates make two-label nodes)"""
    r = np.random.RandomState(seed)
    out = []
    for w in range(n_words):
        ln = 1 + int(r.randint(max_len))
        out.append((w, -0.25 * (1 + int(r.randint(8))), [first + int(r.randint(N - first)) for _ in range(ln)]))
    return out


def dedup(lex):
    """one label per spelling (a token LM gives the labels of a node one score: a tie by construction)"""
    seen, out = set(), []
    for w, sc, sp in lex:
        if tuple(sp) not in seen:
            seen.add(tuple(sp))
            out.append((w, sc, sp))
    return out


def batch(sess, base, Ts, N, lex, o, W, perm, per_state=False, scale=1.0, need=""):
    """B utterances of Ts frames, each on the first clean seed from its base -> (results, stats) per utterance"""
    tokl = o["is_lm_token"]
    lx = Lex(sess.lib, N, o["sil"], lex, 0 if tokl else SMEAR_MAX)
    n_map = N if tokl else 1 + max([w for w, _, _ in lex] + [o["unk"]])
    found = []
    for b, T in enumerate(Ts):
        def case_fn(seed, T=T):
            rl = G.SmRowsLM(seed ^ 0x5A5A, n_map, W, perm, W - 1, 0)
            lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
            return (G.emissions(seed, T, N) * np.float32(scale), lx.nodes, lm, o)
        found.append(clean(case_fn, base + 1000 * b, o["log_add"], need=need if b == 0 else ""))
    rls = [G.SmRowsLM(seed ^ 0x5A5A, n_map, W, perm, W - 1, 0) for seed, _, _, _ in found]
    lm = dev_lm(sess, rls[0], o, mapped=bool(perm))
    dec = make_dec(sess, lx, lm, o)
    got, rows, prefix = decode(sess, dec, [inp[0] for _, inp, _, _ in found], N, W,
                               lambda b, p: rls[b].row(list(p)), per_state=per_state)
    for b, (_, _, (want, want_rows), _) in enumerate(found):
        assert_final(want, got[b], o["log_add"], b)
        assert_rows(want_rows, rows[b], prefix[b])
    for d in (dec, lm, lx):
        d.close()
    return [(res, st) for _, _, res, st in found]


@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
def test_unequal_lengths_in_one_batch(sess, tokl):
    """T = 7, 0, 1, 4 in one batch; unk on"""
    lex = dedup(G.LEX["a"]) if tokl else G.LEX["a"]
    batch(sess, 100, (7, 0, 1, 4), 6, lex, opts(6, 5, 25.0, 0.7, 0.25, -0.5, -0.2, unk=6, is_lm_token=tokl), 9, 31,
          per_state=True)


@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
@pytest.mark.parametrize("log_add", [False, True])
def test_small_alphabet_merges_and_reentries(sess, log_add, tokl):
    """two letters (N = 4), K = 8, T = 10: hypotheses merge and states are entered again"""
    lex = [(0, -0.5, [2]), (1, -0.75, [3]), (2, -1.0, [2, 3]), (3, -0.25, [3, 2])]
    out = batch(sess, 200, (10, 3), 4, lex, opts(8, 4, 25.0, 0.7, 0.25, log_add=log_add, is_lm_token=tokl), 6, 0,
                scale=0.25, need="merges")
    assert out[0][1].merges >= 1 and out[0][1].reentered >= 1


@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
def test_more_candidates_than_threads(sess, tokl):
    """N = 20 = Kt, K = 8, S >= 1: at least 8 * (20 * 2 + 2) = 336 candidates, more than one pass of the step's 256
    threads"""
    lex = rand_lex(20, 40, 5)
    lex = dedup(lex) if tokl else lex
    batch(sess, 300, (5, 2), 20, lex, opts(8, 20, 8.0, 0.7, 0.25, NINF, -0.2, is_lm_token=tokl), 41 if not tokl else 21,
          0, per_state=True)


@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
def test_wide_beam(sess, tokl):
    """K = 256, T = 6: more than 128 hypotheses in the last beam"""
    # (a token LM scores "word a, then into b.." and "into ab, word ab" alike; with every candidate kept the two always
    # meet, so its lexicon here has one-letter words only)
    lex = [(i, -0.25 * (i + 1), [2 + i]) for i in range(4)] if tokl else G.LEX["a"]
    out = batch(sess, 400, (6,), 6, lex, opts(256, 6, 1e9, 0.7, 0.25, -0.5, unk=6, is_lm_token=tokl), 8, 0,
                per_state=True)
    assert len(out[0][0][1][-1]) > 128


def test_token_beam_limit(sess):
    """N = 300, Kt = 256 (the limit), K = 4, T = 3; 257 is refused at begin"""
    lex = rand_lex(300, 200, 9, 2)
    o = opts(4, 256, 25.0, 0.7, 0.25)
    batch(sess, 500, (3, 2), 300, lex, o, 201, 0)
    lx = Lex(sess.lib, 300, 0, lex)
    lm = _capi.WordRowsLM(201, None, 200, lib=sess.lib)
    dec = make_dec(sess, lx, lm, dict(o, Kt=257))
    with pytest.raises(_capi.FltxError) as e:
        dec.begin(np.zeros(300, np.float32), [1], 300)
    assert e.value.code == _capi.ERR_UNSUPPORTED
    for d in (dec, lm, lx):
        d.close()


@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
def test_one_row_per_state_equals_one_per_hypothesis(sess, tokl):
    """(decode() rebuilds every prefix from (src_row, token, state) and asserts one prefix per id across frames)"""
    N, W = 6, 9
    lex = dedup(G.LEX["a"]) if tokl else G.LEX["a"]
    o = opts(6, N, 25.0, 0.7, 0.25, -0.5, unk=6, is_lm_token=tokl)
    ems = [G.emissions(510 + b, T, N) for b, T in enumerate((7, 4))]
    rl = G.SmRowsLM(77, N if tokl else 7, W, 35, W - 1, 0)
    lx = Lex(sess.lib, N, 0, lex, 0 if tokl else SMEAR_MAX)
    lm = dev_lm(sess, rl, o)
    res = []
    for per_state in (False, True):
        dec = make_dec(sess, lx, lm, o)
        res.append(decode(sess, dec, ems, N, W, lambda b, p: rl.row(list(p)), per_state=per_state))
        dec.close()
    assert res[0][1] == res[1][1]
    for a, b in zip(res[0][0], res[1][0]):
        assert_final(a, b, False)
    # an out-of-range entry: that row's LM entries are NaN -- the restatement with that hole
    bad = (2, 0, 1)
    dec = make_dec(sess, lx, lm, o)
    got, rows, prefix = decode(sess, dec, ems, N, W, lambda b, p: rl.row(list(p)), per_state=True, bad_rows=[bad])
    dec.close()
    st = Stats()
    want, want_rows = restate(ems[0], lx.nodes, PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish), o, st=st,
                              hole=(bad[0], bad[2]))
    assert not st.ties
    assert_final(want, got[0], False)
    assert_rows(want_rows, rows[0], prefix[0])
    assert_final(res[1][0][1], got[1], False)  # (the other utterance: untouched)
    lm.close()
    lx.close()


# ---- 6. typed LM rows in lockstep ---------------------------------------------------------------------------------------
def _typed(sess, dt, kind, mode, tokl, W, N=6):
    lex = dedup(G.LEX["a"]) if tokl else G.LEX["a"]
    o = opts(4, N, 25.0, 0.7, 0.25, is_lm_token=tokl)
    ems = [G.emissions(610 + b, T, N) for b, T in enumerate((5, 3))]
    n_map = N if tokl else 6
    rl = G.SmRowsLM(99, n_map, W, 37, W - 1, 0)
    lx = Lex(sess.lib, N, 0, lex, 0 if tokl else SMEAR_MAX)
    lm = dev_lm(sess, rl, o)

    def lm_row(b, p):
        return rl.row(list(p)) * np.float32(3.0 if kind else 1.0)
    feed = TypedFeed(sess, dt, kind, mode, W)
    A = make_dec(sess, lx, lm, o)
    a = decode(sess, A, ems, N, W, lm_row, feed=feed)
    R = make_dec(sess, lx, lm, o)
    seq = iter(feed.mats)

    def feed_r(dec, lr, ro, end, scored):
        lf = next(seq)
        return dec.end(_dev(sess, lf)) if end else dec.step(_dev(sess, lf))
    r = decode(sess, R, ems, N, W, lm_row, feed=feed_r)
    assert a[1] == r[1]
    for x, y in zip(a[0], r[0]):
        assert_final(x, y, False)
    assert not kind or feed.n_lse > 10
    for d in (A, R, lm, lx):
        d.close()


@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
@pytest.mark.parametrize("dt", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", [0, 1], ids=["log_probs", "logits"])
@pytest.mark.parametrize("mode", ["dev", "host", "strided"])
def test_typed_lm_rows_lockstep(sess, dt, kind, mode, tokl):
    """A on typed rows of odd width 9, R on the float32 matrix those rows stand for: the row lists of every frame and
    the results are bit-identical; lm_row_lse against ref_lse."""
    _typed(sess, dt, kind, mode, tokl, 9)


@pytest.mark.parametrize("kind", [0, 1], ids=["log_probs", "logits"])
def test_wide_word_lm_rows_of_odd_width(sess, kind):
    """the word LM at lm_width = 70 001, bf16 rows one element into a buffer of odd stride"""
    _typed(sess, BF16, kind, "strided", False, 70001)


# ---- 7. NaN and -inf; the state-table limit ---------------------------------------------------------------------------
@pytest.mark.parametrize("tokl", [False, True], ids=["word", "token"])
@pytest.mark.parametrize("lmw", [0.0, 0.5])
def test_nan_and_inf_entries(sess, lmw, tokl):
    """A NaN LM entry, and 0 * -inf, are no candidates; under lm_weight 0.5 a -inf entry makes a -inf candidate, which
    the threshold removes as it removes a -inf emission; a NaN emission is never a candidate."""
    N, W, T = 6, 8, 6
    lex = dedup(G.LEX["a"]) if tokl else G.LEX["a"]
    o = opts(6, N, 25.0, lmw, 0.25, -0.5, unk=6, is_lm_token=tokl)
    rl = G.SmRowsLM(55, N if tokl else 7, W, 0, W - 1, 0)

    def row(p):
        r = rl.row(list(p)).copy()
        if len(p) % 2 == 1:
            r[2] = -np.inf
        if len(p) == 2:
            r[3] = np.nan
        return r
    lx = Lex(sess.lib, N, 0, lex, 0 if tokl else SMEAR_MAX)

    def case_fn(seed):
        em = G.emissions(seed, T, N)
        em[2, 3] = np.nan
        em[3, 2] = -np.inf
        return em, lx.nodes, PrefixLM(row, rl.usr_to_lm, rl.finish), o
    _, (em, _, _, _), (want, want_rows), _ = clean(case_fn, 700, False)  # (at lm_weight 0 segmentations tie easily)
    lm = dev_lm(sess, rl, o, mapped=False)
    dec = make_dec(sess, lx, lm, o)
    got, rows, prefix = decode(sess, dec, [em], N, W, lambda b, p: row(p))
    assert_final(want, got[0], False)
    assert_rows(want_rows, rows[0], prefix[0])
    assert all(not (np.isnan(g[:3]).any()) for g in got[0])
    for d in (dec, lm, lx):
        d.close()


def test_state_table_limit(sess):
    """max_states = 3: the utterance that needs more states reports "LM-state table full", the other one decodes"""
    N, K, W = 6, 6, 7
    flat = np.full((1, N), -5.0, np.float32)
    flat[0, 1] = 0.0  # utterance 1: blanks only -- the root's state alone survives the threshold
    ems = [G.emissions(800, 6, N), np.repeat(flat, 6, axis=0)]
    lx = Lex(sess.lib, N, 0, G.LEX["a"])
    lm = _capi.WordRowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lx, lm, opts(K, N, 2.0, 0.0, 1.0))
    dec.set_max_states(3)
    dec.begin(np.concatenate([e.reshape(-1) for e in ems]), [6, 6], N)
    lr = np.zeros((2 * K, W), np.float32)
    for _ in range(6):
        tok, src, state, n = dec.step(_dev(sess, lr))
    dec.ctx.synchronize()
    assert int(_np(n)[0]) == 0 and int(_np(n)[1]) >= 1
    dec.end(_dev(sess, lr))
    with pytest.raises(_capi.FltxError) as e:
        dec.count(0)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "LM-state table full" in str(e.value)
    nh, ln = dec.count(1)
    assert nh >= 1 and ln == 8
    h = dec.results(1)[0]
    assert h.tokens.tolist() == [0] + [1] * 6 + [0] and (h.words == -1).all()
    for d in (dec, lm, lx):
        d.close()


# ---- 8. contract and refusals -----------------------------------------------------------------------------------------
def test_contract_and_refusals(sess):
    import ctypes as C
    L, ctx = sess.lib, sess.ctx
    I, U, S = _capi.ERR_INVALID, _capi.ERR_UNSUPPORTED, _capi.ERR_STATE
    N, K = 6, 4
    lx = Lex(L, N, 0, G.LEX["a"])
    wl = _capi.WordRowsLM(8, None, 7, lib=L)
    tl = _capi.RowsLM(N + 1, None, N, lib=L)
    h = C.c_void_p()

    def create(o, lm_, tok, unk=-1, trie=lx.trie):
        return L.lib.fltx_ctc_rows_lex_decoder_create(ctx.h, C.byref(o), trie.h, lm_.h, 0, 1, unk, tok, C.byref(h))
    ok = _capi.make_options(K, N, lm_weight=0.5)
    assert create(ok, wl, 1) == U and create(ok, tl, 0) == U and create(ok, sess.zero, 0) == U  # crossed kinds, other LMs
    assert create(ok, sess.zero, 1) == U
    assert create(_capi.make_options(K, N, criterion="asg"), wl, 0) == U
    assert create(_capi.make_options(257, N), wl, 0) == U and create(_capi.make_options(256, N), wl, 0) == 0
    L.lib.fltx_decoder_destroy(h)
    assert create(ok, tl, 1) == 0
    L.lib.fltx_decoder_destroy(h)
    # the word LM's map against the trie's labels, unk and the finish index; a finish index for both kinds
    for bad, tok, unk, o in ((_capi.WordRowsLM(8, [0, 1, 2, 3, 4], 7, lib=L), 0, -1, ok),          # label 5: no entry
                             (_capi.WordRowsLM(8, [0, 1, 2, 3, 4, 9], 7, lib=L), 0, -1, ok),       # ... outside the rows
                             (_capi.WordRowsLM(5, None, 4, lib=L), 0, -1, ok),                     # identity, narrow rows
                             (_capi.WordRowsLM(8, None, 7, lib=L), 0, 8, _capi.make_options(K, N, unk_score=-1.0)),  # unk
                             (_capi.WordRowsLM(8, [0, 1, 2, 3, 4, 5], 7, lib=L), 0, 6, _capi.make_options(K, N, unk_score=-1.0)),
                             (_capi.WordRowsLM(8, None, 8, lib=L), 0, -1, ok),                     # finish outside
                             (_capi.RowsLM(N + 1, None, -1, lib=L), 1, -1, ok)):                   # no finish index
        assert create(o, bad, tok, unk) == I, L.lib.fltx_last_error()
        bad.close()
    assert create(_capi.make_options(K, N, unk_score=-1.0), wl, 0, -1) == I  # unk_score > -inf needs the unk word's id,
    assert create(_capi.make_options(K, N, unk_score=-1.0), tl, 1, -1) == I  # ... under either LM
    assert create(_capi.make_options(K, N, unk_score=-1.0), wl, 0, 7) == 0  # (unk inside the rows)
    with pytest.raises(_capi.FltxError) as e:  # lm_width <= 2^22 for the word LM
        _capi.WordRowsLM((1 << 22) + 1, None, 0, lib=L)
    assert e.value.code == U
    L.lib.fltx_decoder_destroy(h)
    # fltx_decoder_create and groups refuse the kind and the rows LMs
    assert L.lib.fltx_decoder_create(ctx.h, _capi.LEX_CTC_ROWS, C.byref(ok), None, sess.zero.h, 0, 1, -1, None, 0, 0,
                                     C.byref(h)) == U
    assert L.lib.fltx_decoder_create(ctx.h, _capi.LEXICON, C.byref(ok), None, wl.h, 0, 1, -1, None, 0, 0, C.byref(h)) == U
    g = C.c_void_p()
    dev0 = (C.c_int32 * 1)(-1)
    assert L.lib.fltx_group_create(dev0, 1, _capi.LEX_CTC_ROWS, C.byref(ok), None, sess.zero.h, 0, 1, -1, None, 0, 0,
                                   C.byref(g)) == U
    o = opts(K, N, 25.0, 0.5)
    dec = make_dec(sess, lx, wl, o)
    dec.B = 1
    outs = dec._rows()
    po = [dec._addr(x) for x in outs]
    em = G.emissions(900, 3, N)
    T = np.asarray([3], np.int32)
    e_ptr, t_ptr = em.ctypes.data, T.ctypes.data
    lr = _dev(sess, np.zeros((K, 8), np.float32))
    pl = dec._addr(lr)
    step, end, begin = L.lib.fltx_ctc_rows_step, L.lib.fltx_ctc_rows_end, L.lib.fltx_ctc_rows_begin
    assert step(dec.h, pl, 0, 0, 8, None, 0, 1, None, *po) == S and end(dec.h, pl, 0, 0, 8, None, 0, 1, None) == S
    assert begin(dec.h, e_ptr, 0, None, t_ptr, 1, N, po[0], po[1], None, po[3]) == I
    assert begin(dec.h, e_ptr, 0, None, t_ptr, 1, 65537, *po) == U
    # a token LM's map is checked against N at begin
    short = _capi.RowsLM(N + 1, [0, 1, 2], N, lib=L)
    d2 = make_dec(sess, lx, short, dict(o, is_lm_token=True))
    assert begin(d2.h, e_ptr, 0, None, t_ptr, 1, N, *po) == I
    d2.close()
    short.close()
    assert begin(dec.h, e_ptr, 0, None, t_ptr, 1, N, *po) == 0
    assert step(dec.h, pl, 3, 0, 8, None, 0, 1, None, *po) == I and step(dec.h, pl, 0, 2, 8, None, 0, 1, None, *po) == I
    assert step(dec.h, pl, 0, 0, 7, None, 0, 1, None, *po) == I                       # lm_row_stride < lm_width
    assert step(dec.h, None, 0, 0, 8, None, 0, 1, None, *po) == I
    assert step(dec.h, pl, 0, 0, 8, None, 0, 1, None, *po) == 0
    assert L.lib.fltx_decode_batch(dec.h, e_ptr, 0, None, t_ptr, 1, N) == S
    assert L.lib.fltx_stream_begin(dec.h, 1, N, 10) == S and L.lib.fltx_stream_end(dec.h) == S
    assert L.lib.fltx_stream_step(dec.h, e_ptr, 0, None, t_ptr) == S and L.lib.fltx_stream_prune(dec.h, 0) == S
    assert L.lib.fltx_s2s_begin(dec.h, 1, N, *po) == S and L.lib.fltx_s2s_end(dec.h) == S
    assert L.lib.fltx_s2s_step(dec.h, pl, 1, 8, None, *po) == S
    assert L.lib.fltx_s2s_lex_set_max_states(dec.h, 8) == S
    assert L.lib.fltx_decoder_set(dec.h, b"max_states", 0) == I and L.lib.fltx_decoder_set(dec.h, b"max_states", 9) == 0
    # fltx_ctc_rows_* on the old kinds
    other = _capi.BatchDecoder(ctx, _capi.LEXFREE, ok, sess.zero, 0, 1)
    s2s = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    for x in (other, s2s):
        assert begin(x.h, e_ptr, 0, None, t_ptr, 1, N, *po) == S
        assert step(x.h, pl, 0, 0, 8, None, 0, 1, None, *po) == S and end(x.h, pl, 0, 0, 8, None, 0, 1, None) == S
        x.close()
    assert end(dec.h, pl, 0, 0, 8, None, 0, 1, None) == 0                             # an early end: one frame decoded
    assert dec.count(0)[1] == 3
    for d in (dec, wl, tl, lx):
        d.close()


def test_lexfree_rows_decode_is_untouched_by_this_kind(sess):
    """a FLTX_DECODER_CTC_ROWS decode before and after a decode of the new kind on the same context: identical bits"""
    N, K, W = 6, 6, 7
    em = G.emissions(1200, 8, N)
    rl = G.SmRowsLM(5, N, W, 0, W - 1, 0)
    tl = _capi.RowsLM(W, None, W - 1, lib=sess.lib)

    def lexfree():
        d = C0.make_dec(sess, tl, K, N, 25.0, 0.7, -0.2, 0, 1, False)
        out = C0.decode(sess, d, [em], N, W, lambda b, p: rl.row(list(p)))
        d.close()
        return out
    before = lexfree()
    batch(sess, 1300, (5,), N, G.LEX["a"], opts(6, N, 25.0, 0.7, 0.25), 7, 0)
    after = lexfree()
    assert before[1] == after[1] and len(before[0][0]) == len(after[0][0]) > 1
    for x, y in zip(before[0][0], after[0][0]):
        assert x[3] == y[3] and _bits_equal(x[:3], y[:3])
    tl.close()


# ---- 9. the Python helper ----------------------------------------------------------------------------------------------
def test_python_helper_on_a_toy_word_lm(sess):
    """LexiconCtcRowsBatchDecoder.decode with a callable: one LM row per state id, asked once per state, told the parent
    id and the edge; against the restatement."""
    N, W = 6, 7
    o = opts(6, N, 25.0, 0.7, 0.25)
    lx = Lex(sess.lib, N, 0, G.LEX["a"])
    rl = G.SmRowsLM(21, 6, W, 0, W - 1, 0)
    found = [clean(lambda seed, T=T: (G.emissions(seed, T, N), lx.nodes,
                                      PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish), o), 950 + 50 * b, False)
             for b, T in enumerate((6, 2, 4))]
    lm = _capi.WordRowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lx, lm, o)
    asked, known = [], {}

    def lm_rows(keys):
        for b, p, par, edge, sid in keys:
            assert (par, edge) == (-1, -1) and p == () or known[(b, par)] + (edge,) == p
            known[(b, sid)] = p
        asked.extend((b, sid) for b, _, _, _, sid in keys)
        return _dev(sess, np.stack([rl.row(list(p)) for _, p, _, _, _ in keys]))
    ems = [inp[0] for _, inp, _, _ in found]
    got = dec.decode(np.concatenate([e.reshape(-1) for e in ems]), [e.shape[0] for e in ems], N, lm_rows)
    assert len(set(asked)) == len(asked)  # once per state
    states = set()
    for b, (_, _, (_, want_rows), _) in enumerate(found):
        states |= {(b, ())} | {(b, s) for fr in want_rows[:-1] for _, _, s in fr}
        states |= {(b, s) for _, _, s in want_rows[-1]}
    assert {(b, known[(b, sid)]) for b, sid in asked} == states and len(asked) == len(states)
    for b, (_, _, (want, _), _) in enumerate(found):
        assert_final(want, [(h.score, h.am, h.lm, list(h.tokens), list(h.words)) for h in got[b]], False, b)
    for d in (dec, lm, lx):
        d.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_CTC_LMROWS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
