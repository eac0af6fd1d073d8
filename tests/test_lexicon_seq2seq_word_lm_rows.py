"""Lexicon seq2seq shallow fusion with a WORD-level rows LM (fltx_lm_word_rows_create, fltx_s2s_lex_decoder_create with
is_lm_token == 0, fltx_s2s_step_word_lm_rows; text_amd/csrc/fltx_s2s_lex.h "Word-level LM rows").

The LM scores the lexicon's words; its rows arrive per step, one per LM state, and lm_row_of names the row of each decoder
row.  A record entry's eos (at the root) reads the finish entry, a word end reads its label's entry minus lexMaxScore, the
move inside a word reads the smeared trie alone.  The step also lists next_word, with which (and next_src_row) the caller
keeps the LM's states.  The checks: the compiled reference's fixtures (tests/golden/
make_lex_s2s_word_lm_rows_golden.py: the restatement reproduces them, the device reproduces them); the existing word
n-gram device decode as a cross-check; next_word and the caller's recipe (one row per state) against identity rows;
random batches against the float64 restatement of tests/test_lexicon_seq2seq.py; rows wider than 65 536 and than the
register cache, rows at 2-byte-aligned starts, records longer than a wave; typed LM rows in lockstep with float32 rows;
the ABI's contract; the compat decoder.

Every test makes a decoder with a WordRowsLM, which does not exist before this feature.  Every device test runs on the
emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that initialises torch first (as
tests/test_seq2seq.py explains).
"""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi, ngram_synth  # noqa: E402

CHILD = os.environ.get("FLTX_LEX_S2S_WORDLMROWS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from golden import make_lex_s2s_lm_rows_golden as GT  # noqa: E402
from golden import make_lex_s2s_word_lm_rows_golden as G  # noqa: E402
from golden.make_s2s_lm_rows_golden import SmRowsLM  # noqa: E402
from test_lexicon_seq2seq import (_GpuSess, _np, compare, host_trie, is_gpu, make_lexicon, restate_lex,  # noqa: E402
                                  sm_model, trie_nodes)
from test_lexicon_seq2seq import run_device as run_device_tables  # noqa: E402
from test_seq2seq import HostLM  # noqa: E402
from test_seq2seq_model_output import BF16, F16, F32, _bits_equal, ref_lse, to_dtype, widen  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
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


def _dev(sess, a, dt=F32, shift=False):
    """a numpy array as the step takes it on this backend: itself (emulator) or a device tensor.  shift: the data
    start one 2-byte element after an aligned address (bf16 / fp16 rows)"""
    if shift:
        assert a.dtype.itemsize == 2
        buf = np.zeros(a.size + 8, a.dtype)
        buf[1:1 + a.size] = a.reshape(-1)
        if not is_gpu(sess):
            v = buf[1:1 + a.size].reshape(a.shape)
            assert v.ctypes.data % 16 == 2 or v.ctypes.data % 4 == 2
            return v
        import torch
        t = torch.from_numpy(buf.view(np.int16)).cuda()
        t = t.view(torch.bfloat16) if dt == BF16 else t.view(torch.float16)
        v = t[1:1 + a.size].view(*a.shape)
        assert v.data_ptr() % 16 == 2
        return v
    if not is_gpu(sess):
        return a
    import torch
    t = torch.from_numpy(a.view(np.int16) if dt == BF16 else a).cuda()
    return t.view(torch.bfloat16) if dt == BF16 else t


def word_lm(sess, rl):
    """the library's LM object of a word rows LM of the tests (usr_to_lm: word id -> LM index, W, finish)"""
    ident = np.array_equal(rl.usr_to_lm, np.arange(len(rl.usr_to_lm)))
    return _capi.WordRowsLM(rl.W, None if ident else rl.usr_to_lm, rl.finish, lib=sess.lib)


def make_dec(sess, trie, lm, K, Kt, thr=1e9, lmw=0.0, word_score=0.0, eos_score=0.0, eos=0, maxlen=5, log_add=False,
             is_lm_token=False):
    return _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_lex_options(K, Kt, thr, lmw, word_score, eos_score,
                                                                               log_add), trie, lm, eos, maxlen,
                                            is_lm_token)


def case_dec(sess, c, t, lm):
    return make_dec(sess, t, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                    c["maxlen"], c["log_add"])


def _trim(r):
    r = list(r)
    while r and r[-1] == []:
        r.pop()
    return r


# ---- the device loop ------------------------------------------------------------------------------------------------------
def run_device(sess, dec, models, lms, maxlen, V, W, states=False, feed=None, pad=np.nan, fetch=True, lm_dt=F32):
    """All utterances in one batch: models[b].row(token prefix) -> V float32 (None: the row is dropped),
    lms[b].row(word prefix) -> W float32.  A row's word prefix is kept from next_src_row and next_word alone.
    states False: one LM row per decoder row (identity, lm_row_of None; padding and dropped rows hold `pad`);
    states True: the caller's recipe -- one LM row per LM state in use, lm_row_of naming it (-1 for rows that are not
    live: nothing may be read through those).
    -> (final per utterance, rows per step per utterance, merges per utterance,
        the (token path, per-position words) of every listed row per step per utterance)"""
    B, K = len(models), int(dec.options.beam_size)
    tok, beam, src, n = dec.begin(B, V)
    word = None
    prefix = {(b, 0): ([], [], ()) for b in range(B)}  # row -> (token path, words per position, word prefix)
    rows = [[] for _ in range(B)]
    listed = [[] for _ in range(B)]
    gpu = is_gpu(sess)
    for t in range(maxlen + 2):  # (two steps more than it takes: a step after the last one is a no-op)
        if gpu:
            dec.ctx.synchronize()
        tok_h, beam_h, src_h, n_h = _np(tok), _np(beam), _np(src), _np(n)
        word_h = _np(word) if word is not None else np.full((B, K), -1, np.int32)
        if t > 0:
            for b in range(B):
                rows[b].append([(int(tok_h[b, k]), int(beam_h[b, k]), int(src_h[b, k]) - b * K if src_h[b, k] >= 0
                                 else None) for k in range(n_h[b])])
                assert (tok_h[b, n_h[b]:] == -1).all() and (src_h[b, n_h[b]:] == -1).all(), (t, b)
                assert (word_h[b, n_h[b]:] == -1).all(), (t, b, word_h[b].tolist())
        sc = np.full((B * K, V), pad, dtype=np.float32)
        valid = np.zeros(B * K, dtype=np.uint8)
        newpre = {}
        for b in range(B):
            for k in range(n_h[b]):
                if t == 0:
                    p = ([], [], ())
                else:
                    tp, wl, wp = prefix[(b, int(src_h[b, k]) - b * K)]
                    w = int(word_h[b, k])
                    p = (tp + [int(tok_h[b, k])], wl + [w], wp + ((w,) if w >= 0 else ()))
                newpre[(b, k)] = p
                r = models[b].row(p[0])
                if r is None:
                    continue
                sc[b * K + k] = r
                valid[b * K + k] = 1
            if t > 0:
                listed[b].append({(tuple(newpre[(b, k)][0]), tuple(newpre[(b, k)][1])) for k in range(n_h[b])})
        prefix = newpre
        ro = None
        if states:
            keys = sorted({(b, p[2]) for (b, k), p in prefix.items() if valid[b * K + k]})
            at = {key: i for i, key in enumerate(keys)}
            lr = np.full((max(len(keys), 1), W), pad, dtype=np.float32)
            for key, i in at.items():
                lr[i] = lms[key[0]].row(list(key[1]))
            ro = np.full(B * K, -1, np.int32)
            for (b, k), p in prefix.items():
                if valid[b * K + k]:
                    ro[b * K + k] = at[(b, p[2])]
        else:
            lr = np.full((B * K, W), pad, dtype=np.float32)
            for (b, k), p in prefix.items():
                if valid[b * K + k]:
                    lr[b * K + k] = lms[b].row(list(p[2]))
        if feed is not None:
            tok, beam, src, n, word = feed(dec, sc, lr, valid, ro)
        else:
            lraw = lr if lm_dt == F32 else to_dtype(lr.astype(np.float64), lm_dt)
            tok, beam, src, n, word = dec.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, lraw, lm_dt),
                                               lm_row_of=None if ro is None else _dev(sess, ro))
    assert dec.done()
    merges = dec.info()["merges"]
    dec.end()
    out = [[(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in dec.results(b)] for b in range(B)] \
        if fetch else None
    return out, [_trim(r) for r in rows], merges, listed


# ---- 1. fixtures of the reference itself ------------------------------------------------------------------------------
def _golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "lexicon_seq2seq_word_lm_rows_expected.json.gz"), "rt") as f:
        return json.load(f)


def _case(name):
    return next(c for c in _golden() if c["name"] == name)


def _case_trie(c, lib):
    return host_trie(lib, c["V"], G.lexicon(c), SMEAR_MAX)


def test_fixtures_cover_the_ground(emu_session):
    cs = _golden()
    assert all(9 <= c["V"] <= 14 and 8 <= c["K"] <= 24 and c["Kt"] <= c["V"] and 6 <= c["maxlen"] <= 8 and
               30 <= c["lex"][0] <= 40 for c in cs)
    assert any(c["log_add"] and c["merges"] for c in cs) and any(not c["log_add"] and c["merges"] for c in cs)
    assert any(G.both_labels(c["hyps"]) for c in cs)  # (two labels of one node both survive)
    for c in cs:
        um = G.case_lm(c).usr_to_lm
        c["permuted"] = not np.array_equal(um, np.arange(len(um)))
        nodes = trie_nodes(_case_trie(c, emu_session.lib))
        assert any(n[2] != 0 for n in nodes[1:]) and any(len(n[1]) >= 2 for n in nodes) or c["lex"][3] == 0
    assert any(c["permuted"] and c["W"] > c["lex"][0] + 1 for c in cs)
    assert any(c["drop"] > 0 for c in cs)
    assert any(c["lmw"] == 0 and not c["inf_mod"] and all(h[2] != 0.0 for h in c["hyps"]) for c in cs)  # (lm accumulates)
    assert any(c["lmw"] == 0 and c["inf_mod"] and c["infs"] > 0 for c in cs)
    assert any(any(h[3][-1] != c["eos"] for h in c["hyps"]) for c in cs)  # (max_output_length with live hypotheses)
    lm = _capi.WordRowsLM(4, None, 3, lib=emu_session.lib)  # (the feature under test exists)
    lm.close()


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c, emu_session):
    """The restatement with a word-prefix object LM against the compiled reference: tokens and words exact; scores bit
    for bit, within 1e-5 where a logAdd merge fed them; the merge count as recorded, no tie.  (The trie the restatement
    walks is the library's, smeared by it; the decoder below is made on it.)"""
    t = _case_trie(c, emu_session.lib)
    ties, stats = [], {}
    got, _, _ = G.restate_case(c, trie_nodes(t), ties=ties, stats=stats)
    assert not ties and stats.get("merges", 0) == c["merges"]
    assert GT.same(got, c["hyps"], c["log_add"]), (got[:2], c["hyps"][:2])
    lm = word_lm(emu_session, G.case_lm(c))
    case_dec(emu_session, c, t, lm).close()
    lm.close()


def _same_as_fixture(c, got):
    """tokens, words and n-best order exact; scores bit-identical for max merge, within the stated 1e-5 for logAdd"""
    assert len(got) == len(c["hyps"])
    for g, r in zip(got, c["hyps"]):
        assert g[3] == r[3] and g[4] == r[4], (g, r)
        if c["log_add"]:
            assert all(abs(x - y) <= 1e-5 * max(1.0, abs(y)) for x, y in zip(g[:3], r[:3])), (g[:3], r[:3])
        else:
            assert _bits_equal(g[:3], r[:3]), (g[:3], r[:3])


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess):
    t = _case_trie(c, sess.lib)
    want, wrows, _ = G.restate_case(c, trie_nodes(t))
    rl = G.case_lm(c)
    lm = word_lm(sess, rl)
    dec = case_dec(sess, c, t, lm)
    got, rows, merges, _ = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"])
    dec.close()
    lm.close()
    _same_as_fixture(c, got[0])
    compare(want, got[0])
    assert rows[0] == _trim(wrows)
    assert merges == [c["merges"]]


# ---- 2. the n-gram tables decode as a cross-check ---------------------------------------------------------------------------
class _NgramWordRows:
    """LM rows from a word n-gram's host twin: row(word prefix)[w] = score(context after the prefix, w) for every word,
    and finish in an extra column."""

    def __init__(self, ng, nw):
        self.hl, self.nw, self.W = HostLM(ng), nw, nw + 1
        self.usr_to_lm, self.finish = np.arange(nw, dtype=np.int32), nw
        self.ctx = {(): self.hl.start()}
        self.rows = {}

    def row(self, prefix):
        p = tuple(prefix)
        if p in self.rows:
            return self.rows[p]
        for i in range(1, len(p) + 1):
            if p[:i] not in self.ctx:
                self.ctx[p[:i]] = self.hl.score(self.ctx[p[:i - 1]], p[i - 1])[0]
        c = self.ctx[p]
        r = np.zeros(self.W, np.float32)
        for w in range(self.nw):
            r[w] = self.hl.score(c, w)[1]
        r[self.nw] = self.hl.finish(c)[1]
        self.rows[p] = r
        return r


def _restate(model, rl, nodes, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add, ties=None, stats=None):
    return restate_lex(model, nodes, GT.PrefixObjLM(rl), K, Kt, thr, lmw, ws, es, eos, maxlen, log_add, False, ties=ties,
                       stats=stats)


def tie_free(base, mk, nodes, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add, tries=60):
    """the first seed from `base` on which the restatement sees no tie: -> (seed, result, merges)"""
    for seed in range(base, base + tries):
        ties, stats = [], {}
        m, rl = mk(seed)
        want = _restate(m, rl, nodes, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add, ties, stats)
        if not ties:
            return seed, want, stats.get("merges", 0)
    raise AssertionError("no tie-free seed in %d tries from %d" % (tries, base))


@pytest.mark.parametrize("lmw", [0.6, 0.0])
def test_equals_the_ngram_device_decode(sess, tmp_path_factory, lmw):
    """A word 3-gram over the lexicon's 30 words: the WordRowsLM decode, its rows evaluated at each hypothesis' word
    history, equals the word-level n-gram device decode on the same smeared trie -- n-best, rows of every step and merge
    counts; exact (max merge), on tie-free seeds."""
    V, K, Kt, eos, maxlen, B, nw = 10, 12, 10, 9, 6, 3, 30
    path = str(tmp_path_factory.mktemp("lex_s2s_wordlmrows") / "w30_s6.arpa")
    vocab = ngram_synth.words(nw, "w")
    ngram_synth.write_arpa(path, vocab, 3, (0, 300, 150), 6)
    ng = _capi.ArpaLM(path, vocab, lib=sess.lib)
    lex = make_lexicon(V, eos, nw, 12, max_len=3, respell=0.5, single=0.3)  # (homophones tie at lm_weight 0)
    t = host_trie(sess.lib, V, lex, SMEAR_MAX)
    nodes = trie_nodes(t)
    nr = _NgramWordRows(ng, nw)
    seeds = [tie_free(500 + 100 * b, lambda s: (sm_model(s, V, eos, 0.5), nr), nodes, K, Kt, 1e9, lmw, 0.2, -0.1, eos,
                      maxlen, False)[0] for b in range(B)]
    models = [sm_model(s, V, eos, 0.5) for s in seeds]
    want, wrows, wmerges = run_device_tables(sess, models, t, ng, K, Kt, 1e9, lmw, 0.2, -0.1, eos, maxlen, V, False,
                                             False)
    lm = _capi.WordRowsLM(nw + 1, None, nw, lib=sess.lib)
    dec = make_dec(sess, t, lm, K, Kt, 1e9, lmw, 0.2, -0.1, eos, maxlen, False)
    got, rows, merges, _ = run_device(sess, dec, models, [nr] * B, maxlen, V, nw + 1)
    for b in range(B):
        assert len(got[b]) == len(want[b])
        for g, w in zip(got[b], want[b]):
            assert g[3] == w[3] and g[4] == w[4] and _bits_equal(g[:3], w[:3]), (b, g, w)
        assert rows[b] == _trim(wrows[b])
    assert merges == wmerges and sum(merges) > 0
    dec.close()
    lm.close()
    ng.close()


# ---- 3. next_word and lm_row_of ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["merge_max", "homophones", "dropped_rows_logadd"])
def test_next_word_and_one_row_per_state(sess, name):
    """next_word against the history records: every ancestor of a final hypothesis was a listed row of its step, and
    the words run_device collected for it from next_word alone are the record's.  Then the caller's recipe -- one LM row
    per state, lm_row_of built from next_src_row / next_word only, -1 on rows that are not live -- against identity with
    duplicated rows: bit for bit, rows and next_word of every step included."""
    c = _case(name)
    t = _case_trie(c, sess.lib)
    rl = G.case_lm(c)
    lm = word_lm(sess, rl)
    dec = case_dec(sess, c, t, lm)
    a, arows, am, alist = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"])
    s, srows, sm, slist = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"], states=True)
    dec.close()
    lm.close()
    _same_as_fixture(c, a[0])
    n_checked = n_words = 0
    for h in a[0]:
        toks = [x for x in h[3] if x >= 0]
        words = h[4][len(h[4]) - len(toks):]
        for j in range(1, len(toks) + 1):
            if toks[j - 1] == c["eos"] or j >= c["maxlen"]:
                continue  # (a finished hypothesis is not listed; nor is the beam of the last step)
            assert (tuple(toks[:j]), tuple(words[:j])) in alist[0][j - 1], (j, toks, words)
            n_checked += 1
            n_words += words[j - 1] >= 0
    assert n_checked > 0 and n_words > 0
    assert len(a[0]) == len(s[0]) and arows == srows and am == sm and alist == slist
    for x, y in zip(a[0], s[0]):
        assert x[3] == y[3] and x[4] == y[4] and _bits_equal(x[:3], y[:3]), (x, y)


def test_out_of_range_lm_row_of(sess):
    """An lm_row_of entry outside [0, n_lm_rows) takes the row's word ends and eos away and leaves its moves; nothing
    is read through it (the LM rows are one row long)."""
    V, K, eos, nw = 10, 24, 9, 30
    lex = make_lexicon(V, eos, nw, 31, max_len=3, respell=0.4, single=0.5)
    t = host_trie(sess.lib, V, lex, SMEAR_MAX)
    nodes = trie_nodes(t)
    lm = _capi.WordRowsLM(nw + 1, None, nw, lib=sess.lib)
    sc = np.full((K, V), -1.0, np.float32) - np.arange(V, dtype=np.float32)[None, :] * 0.01
    lr = np.full((1, nw + 1), -0.5, np.float32)
    kids = nodes[0][0]
    n_moves = len(kids)
    n_ends = sum(len(set(nodes[ch][1])) for ch in kids.values())  # (a word listed twice on a node merges with itself)
    assert n_ends > 0 and n_moves + n_ends + 1 <= K
    seen = {}
    for bad in (0, -1, 1, 1 << 30):
        dec = make_dec(sess, t, lm, K, V, 1e9, 0.5, 0.2, 0.0, eos, 4)
        dec.begin(1, V)
        ro = np.full(K, bad, np.int32)
        out = dec.step(_dev(sess, sc), lm_scores=_dev(sess, lr), lm_row_of=_dev(sess, ro))
        if is_gpu(sess):
            sess.ctx.synchronize()
        n = int(_np(out[3])[0])
        words = _np(out[4])[0]
        dec.end()
        res = dec.results(0)
        seen[bad] = (n, int((words[:n] >= 0).sum()), sum(1 for h in res if h.tokens[-1] == eos), len(res))
        assert (words[n:] == -1).all()
        dec.close()
    assert seen[0] == (n_moves + n_ends, n_ends, 1, n_moves + n_ends + 1), seen
    for bad in (-1, 1, 1 << 30):
        assert seen[bad] == (n_moves, 0, 0, n_moves), seen
    lm.close()


# ---- 4. random batches against the restatement ------------------------------------------------------------------------
def batch_case(sess, rng, B, V, K, Kt, nw, W, perm, finish, thr, lmw, ws, es, eos, maxlen, drop, log_add, lex, states,
               pad=np.nan):
    t = host_trie(sess.lib, V, lex, SMEAR_MAX)
    nodes = trie_nodes(t)
    biases = [float(x) for x in rng.choice([0.0, 0.4, 0.9], B)]  # (utterances of one batch end at different steps)

    def mk(b):
        return lambda seed: (sm_model(seed, V, eos, biases[b], drop), SmRowsLM(seed ^ 0x77, nw, W, perm, finish, 0))
    found = [tie_free(int(rng.integers(1 << 30)), mk(b), nodes, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add)
             for b in range(B)]
    pairs = [mk(b)(found[b][0]) for b in range(B)]
    lm = word_lm(sess, pairs[0][1])
    dec = make_dec(sess, t, lm, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add)
    got, rows, merges, _ = run_device(sess, dec, [p[0] for p in pairs], [p[1] for p in pairs], maxlen, V, W,
                                      states=states, pad=pad)
    for b in range(B):  # (no utterance skipped)
        wf, wr = found[b][1]
        compare(wf, got[b])
        assert rows[b] == _trim(wr), (b, rows[b], _trim(wr))
    assert merges == [f[2] for f in found]
    dec.close()
    lm.close()
    return sum(merges)


def test_random_batches(sess):
    """B = 3 utterances with their own seeds and unequal lengths in one decoder; dropped rows and padding (NaN, or
    garbage where nothing may be read); identity rows and one row per state."""
    rng = np.random.default_rng(2025)
    total = 0
    for i in range(4):
        V = int(rng.choice([9, 11, 14]))
        eos = int(rng.integers(0, V))
        K = int(rng.integers(8, 25))
        nw = int(rng.integers(30, 41))
        W = nw + 1 + int(rng.choice([0, 9]))
        lex = make_lexicon(V, eos, nw, int(rng.integers(1 << 20)), max_len=3, homophones=float(rng.choice([0.0, 0.15])),
                           respell=float(rng.choice([0.2, 0.5])), single=0.4)
        total += batch_case(sess, rng, 3, V, K, int(rng.integers(4, V + 1)), nw, W, int(rng.choice([0, 91])), W - 1,
                            float(rng.choice([3.0, 1e9])), float(rng.choice([0.0, 0.5, 1.1])),
                            float(rng.choice([0.6, -0.3])), float(rng.choice([0.0, -0.3])), eos, int(rng.integers(6, 9)),
                            float(rng.choice([0.0, 0.1])), bool(rng.integers(2)), lex, states=bool(i & 1),
                            pad=float(rng.choice([np.nan, 1e30])))
    assert total > 0


# ---- 5. wide rows, unaligned rows, long records -------------------------------------------------------------------------------
WIDE = 70001  # (beyond 65 536, beyond the logits pass's register cache of 32 768 2-byte / 16 384 4-byte elements)


class _WideLM:
    """The case's LM with its entries scattered into rows of WIDE: word w at 70000 - 1750 w (words 0-2 beyond 65 536),
    finish at 65 537; the rest holds a filler the decode never reads (the logits' lse does)."""

    def __init__(self, rl, nw):
        self.rl, self.W, self.finish = rl, WIDE, 65537
        self.usr_to_lm = (70000 - 1750 * np.arange(nw)).astype(np.int32)
        self.fill = (-5.0 - (np.arange(WIDE) % 7)).astype(np.float32)

    def row(self, prefix):
        base = self.rl.row(prefix)
        r = self.fill.copy()
        r[self.usr_to_lm] = base[self.rl.usr_to_lm]
        r[self.finish] = base[self.rl.finish]
        return r


def test_wide_f32_log_probs_rows(sess):
    """lm_width 70 001, K = 4, float32 log-probs: equals the decode on the narrow rows that hold the same entries."""
    c = dict(_case("perm_wide_finish"), K=4)
    t = _case_trie(c, sess.lib)
    rl = G.case_lm(c)
    wl = _WideLM(rl, G.n_words(c))
    out = []
    for r_ in (rl, wl):
        lm = word_lm(sess, r_)
        dec = case_dec(sess, c, t, lm)
        out.append(run_device(sess, dec, [G.case_model(c)], [r_], c["maxlen"], c["V"], r_.W))
        dec.close()
        lm.close()
    (a, arows, am, alist), (w, wrows, wm, wlist) = out
    assert len(a[0]) == len(w[0]) > 0 and arows == wrows and am == wm and alist == wlist
    assert any(x >= 0 for h in a[0] for x in h[4])
    for x, y in zip(a[0], w[0]):
        assert x[3] == y[3] and x[4] == y[4] and _bits_equal(x[:3], y[:3]), (x, y)


def lockstep(sess, c, dtl, kindl, host=False, wide=False, shift=False):
    """A steps on LM rows of type dtl (log-probs, or logits: kindl) that hold round-to-nearest of the case's LM rows; R
    on float32 log-probs rows holding the values A's rows stand for (widened; for logits (float)((double)x - lse) with
    the lse A's step reports, itself checked against a float64 log-sum-exp).  Both read one row per decoder row
    (identity).  Rows and next_word at every step, n-best and the three scores are bit-identical."""
    t = _case_trie(c, sess.lib)
    m, rl = G.case_model(c), G.case_lm(c)
    if wide:
        rl = _WideLM(rl, G.n_words(c))
    lm = word_lm(sess, rl)
    K, V, W, maxlen = c["K"], c["V"], rl.W, c["maxlen"]
    A, R = (case_dec(sess, c, t, lm) for _ in range(2))
    gpu = is_gpu(sess)
    outA, outR = A.begin(1, V) + (None,), R.begin(1, V) + (None,)
    prefix = {0: ([], ())}
    n_lse = 0
    for step in range(maxlen + 2):
        if gpu:
            sess.ctx.synchronize()
        ta, tr = [_np(o).copy() for o in outA[:4]], [_np(o).copy() for o in outR[:4]]
        wa = _np(outA[4]).copy() if outA[4] is not None else np.full((1, K), -1, np.int32)
        wr = _np(outR[4]).copy() if outR[4] is not None else np.full((1, K), -1, np.int32)
        for x, y, name in zip(ta + [wa], tr + [wr], ("token", "beam_idx", "src_row", "n_rows", "word")):
            assert np.array_equal(x, y), (step, name, x.tolist(), y.tolist())
        tok_h, src_h, n_h = ta[0], ta[2], int(ta[3][0])
        sc = np.full((K, V), np.nan, np.float32)
        l64 = np.full((K, W), np.nan)
        valid = np.zeros(K, np.uint8)
        newpre = {}
        for k in range(n_h):
            if step == 0:
                p = ([], ())
            else:
                tp, wp = prefix[int(src_h[0, k])]
                p = (tp + [int(tok_h[0, k])], wp + ((int(wa[0, k]),) if wa[0, k] >= 0 else ()))
            newpre[k] = p
            r = m.row(p[0])
            if r is None:
                continue
            sc[k], valid[k] = r, 1
            l64[k] = rl.row(list(p[1])).astype(np.float64) * (3.0 if kindl else 1.0)
        prefix = newpre
        lraw = to_dtype(l64, dtl)
        lw = widen(lraw, dtl)
        lse = None
        if kindl:
            lse = _dev(sess, np.full(K, 7.0))  # (device memory on the HIP library, also with host-staged rows)
        kw = dict(lm_kind="logits" if kindl else "log_probs", lm_lse_out=lse)
        if host or not gpu:
            lin = _dev(sess, lraw, dtl, shift=True) if (shift and not gpu) else lraw
            outA = A.step(sc, valid, lm_scores=lin, lm_dtype="bf16" if dtl == BF16 else None, **kw)
        else:
            outA = A.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, lraw, dtl, shift=shift), **kw)
        if kindl:
            if gpu:
                sess.ctx.synchronize()
            ls = _np(lse).copy()
            live = np.zeros(K, bool)
            live[:n_h] = True
            live &= valid.astype(bool)
            assert np.isnan(ls[~live]).all(), (step, ls.tolist())
            for r_ in np.nonzero(live)[0]:
                want = ref_lse(lw[r_])
                assert abs(ls[r_] - want) <= 1e-6 * max(1.0, abs(want)), (step, r_, ls[r_], want)
                n_lse += 1
            with np.errstate(invalid="ignore"):
                lf = (lw.astype(np.float64) - np.where(live, ls, 0.0)[:, None]).astype(np.float32)
        else:
            lf = lw
        lf = np.ascontiguousarray(lf)
        outR = R.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, lf))
    assert A.done() and R.done()
    assert A.info()["merges"] == R.info()["merges"]
    A.end()
    R.end()
    ha, hr = A.results(0), R.results(0)
    assert len(ha) == len(hr) > 0
    for x, y in zip(ha, hr):
        assert x.tokens.tolist() == y.tokens.tolist() and x.words.tolist() == y.words.tolist()
        assert _bits_equal([x.score, x.am, x.lm], [y.score, y.am, y.lm]), (x.score, y.score)
    assert any(w >= 0 for x in ha for w in x.words.tolist())
    A.close()
    R.close()
    lm.close()
    return n_lse


def test_wide_bf16_logits_rows(sess):
    """lm_width 70 001, K = 4, bfloat16 logits (the uncached max / sum passes), rows of odd width starting at a
    2-byte-aligned address: every row start has another alignment."""
    assert lockstep(sess, dict(_case("perm_wide_finish"), K=4), BF16, 1, wide=True, shift=True) > 0


def test_unaligned_cached_logits_rows(sess):
    """fp16 logits rows inside the register cache whose first row starts 2 bytes after a 16-byte boundary."""
    assert lockstep(sess, _case("homophones"), F16, 1, shift=True) > 0


def test_record_longer_than_a_wave(sess):
    """V = Kt = 70: a row's record has more entries than a wave has lanes (the log-probs gather strides over them)."""
    V, K, Kt, eos, maxlen, nw = 70, 8, 70, 69, 4, 40
    lex = make_lexicon(V, eos, nw, 3, max_len=2, homophones=0.1, respell=0.3, single=0.6)
    t = host_trie(sess.lib, V, lex, SMEAR_MAX)
    nodes = trie_nodes(t)
    mk = lambda s: (sm_model(s, V, eos, 0.5), SmRowsLM(s ^ 0x77, nw, nw + 1, 0, nw, 0))  # noqa: E731
    seed, want, _ = tie_free(40, mk, nodes, K, Kt, 1e9, 0.5, 0.3, 0.0, eos, maxlen, False)
    m, rl = mk(seed)
    lm = word_lm(sess, rl)
    dec = make_dec(sess, t, lm, K, Kt, 1e9, 0.5, 0.3, 0.0, eos, maxlen)
    got, rows, _, _ = run_device(sess, dec, [m], [rl], maxlen, V, nw + 1)
    compare(want[0], got[0])
    assert rows[0] == _trim(want[1])
    assert any(w >= 0 for h in got[0] for w in h[4])
    dec.close()
    lm.close()


# ---- 6. typed LM rows in lockstep -----------------------------------------------------------------------------------------
def test_bf16_log_probs_lm_rows(sess):
    assert lockstep(sess, _case("perm_wide_finish"), BF16, 0) == 0


def test_fp16_logits_lm_rows(sess):
    assert lockstep(sess, _case("merge_max"), F16, 1) > 0


def test_host_staged_rows(sess):
    """Host rows (numpy on the HIP library: on_device == 0) of both matrices and a host lm_row_of are staged in their
    own types: bf16 logits in lockstep, and a float32 fixture decode with one row per state."""
    assert lockstep(sess, _case("perm_wide_finish"), BF16, 1, host=True) > 0
    c = _case("merge_logadd")
    t = _case_trie(c, sess.lib)
    want, wrows, _ = G.restate_case(c, trie_nodes(t))
    rl = G.case_lm(c)
    lm = word_lm(sess, rl)
    dec = case_dec(sess, c, t, lm)
    got, rows, merges, _ = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"], states=True,
                                      feed=lambda d, sc, lr, valid, ro: d.step(sc, valid, lm_scores=lr, lm_row_of=ro))
    compare(want, got[0])
    assert rows[0] == _trim(wrows) and merges == [c["merges"]]
    dec.close()
    lm.close()


# ---- 7. the contract ----------------------------------------------------------------------------------------------------
def _outs(sess, B, K):
    if is_gpu(sess):
        import torch
        return [torch.zeros(B * K, dtype=torch.int32, device="cuda") for _ in range(4)] + \
            [torch.zeros(B, dtype=torch.int32, device="cuda")]
    return [np.zeros(B * K, np.int32) for _ in range(4)] + [np.zeros(B, np.int32)]


def _addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def test_contract_and_refusals(sess):
    L, ctx = sess.lib, sess.ctx
    U, I, S = _capi.ERR_UNSUPPORTED, _capi.ERR_INVALID, _capi.ERR_STATE
    V, K, eos, nw = 6, 4, 1, 8
    lex = make_lexicon(V, eos, nw, 1)
    n_lab = max(lab for lab, _, _ in lex) + 1
    trie = host_trie(L, V, lex, SMEAR_MAX)
    h = C.c_void_p()

    def err():
        return L.lib.fltx_last_error().decode()
    # fltx_lm_word_rows_create
    create = L.lib.fltx_lm_word_rows_create
    assert create(0, None, 0, 0, C.byref(h)) == I            # lm_width must be given
    assert create(8, None, 0, -1, C.byref(h)) == I           # finish_index is required
    assert create((1 << 22) + 1, None, 0, 0, C.byref(h)) == U
    big = _capi.WordRowsLM(1 << 22, None, 0, lib=L)
    big.close()
    lm = _capi.WordRowsLM(n_lab + 1, None, n_lab, lib=L)
    # the decoders that refuse it
    opts = _capi.make_s2s_lex_options(K, 4, lm_weight=0.5)
    assert L.lib.fltx_s2s_lex_decoder_create(ctx.h, C.byref(opts), trie.h, lm.h, eos, 5, 1, C.byref(h)) == U
    assert "rows LM" in err()
    with pytest.raises(_capi.FltxError) as e:
        _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4), lm, eos, 5)
    assert e.value.code == U and "rows LM" in str(e.value)
    with pytest.raises(_capi.FltxError) as e:
        _capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(4, 4), lm, 0, 1)
    assert e.value.code == U and "rows LM" in str(e.value)
    with pytest.raises(_capi.FltxError) as e:
        _capi.DecoderGroup([0], _capi.LEXFREE, _capi.make_options(4, 4), lm, 0, 1, lib=L)
    assert e.value.code == U and "rows LM" in str(e.value)
    for f in (lm.state_size, lm.start, lambda: lm.step(np.zeros(1, np.int32), 1), lambda: lm.score_sequence([1, 2])):
        with pytest.raises(_capi.FltxError) as e:
            f()
        assert e.value.code == U and "rows LM" in str(e.value)
    # today's rows LM stays refused with is_lm_token == 0
    tl = _capi.RowsLM(lib=L)
    assert L.lib.fltx_s2s_lex_decoder_create(ctx.h, C.byref(opts), trie.h, tl.h, eos, 5, 0, C.byref(h)) == U
    assert "rows LM" in err()
    tl.close()

    # the create-time map checks
    def create_rc(lmx):
        rc = L.lib.fltx_s2s_lex_decoder_create(ctx.h, C.byref(opts), trie.h, lmx.h, eos, 5, 0, C.byref(h))
        if rc == 0:
            L.lib.fltx_decoder_destroy(h)
        lmx.close()
        return rc
    ident = list(range(n_lab))
    assert create_rc(_capi.WordRowsLM(n_lab + 1, ident, n_lab, lib=L)) == 0
    assert create_rc(_capi.WordRowsLM(n_lab + 1, ident[:-1], n_lab, lib=L)) == I       # a label beyond the map
    assert create_rc(_capi.WordRowsLM(n_lab + 1, ident[:-1] + [n_lab + 1], 0, lib=L)) == I  # an index beyond the rows
    assert create_rc(_capi.WordRowsLM(n_lab + 1, [-1] + ident[1:], 0, lib=L)) == I
    assert create_rc(_capi.WordRowsLM(n_lab - 1, None, 0, lib=L)) == I                 # identity into narrower rows
    assert create_rc(_capi.WordRowsLM(n_lab, None, n_lab, lib=L)) == I                 # finish outside the rows
    assert create_rc(_capi.WordRowsLM(n_lab, None, n_lab - 1, lib=L)) == 0
    # the step entry points
    W = n_lab + 1
    dr = make_dec(sess, trie, lm, K, 4, lmw=0.5, eos=eos, maxlen=5)
    dz = make_dec(sess, trie, sess.zero, K, 4, eos=eos, maxlen=5)
    sc, lr = _dev(sess, np.zeros((K, V), np.float32)), _dev(sess, np.zeros((K, W), np.float32))
    ro = _dev(sess, np.zeros(K, np.int32))
    ps, pl, pr = _addr(sc), _addr(lr), _addr(ro)
    o = [_addr(x) for x in _outs(sess, 1, K)]
    po, pw = [o[0], o[1], o[2], o[4]], o[3]
    step = L.lib.fltx_s2s_step_word_lm_rows

    def wstep(d, ps_=ps, dt=0, kind=0, stride=V, pl_=pl, ldt=0, lkind=0, lstride=W, pr_=None, nlm=0, pw_=pw):
        return step(d.h, ps_, dt, kind, stride, pl_, ldt, lkind, lstride, pr_, nlm, 1, None, None, None, po[0], po[1],
                    po[2], pw_, po[3])
    assert wstep(dr) == S                                                           # before fltx_s2s_begin
    dr.begin(1, V)
    dz.begin(1, V)
    assert L.lib.fltx_s2s_step(dr.h, ps, 1, V, None, *po) == S
    assert L.lib.fltx_s2s_step_typed(dr.h, ps, 0, 1, 1, V, None, None, *po) == S
    assert L.lib.fltx_s2s_step_lm_rows(dr.h, ps, 0, 0, V, pl, 0, 0, W, 1, None, None, None, *po) == S
    assert wstep(dz) == S                                                           # a decoder without a word rows LM
    assert wstep(dr, dt=3) == I and wstep(dr, ldt=3) == I                           # dtype, lm_dtype
    assert wstep(dr, kind=2) == I and wstep(dr, lkind=2) == I                       # kind, lm_kind
    assert wstep(dr, lstride=W - 1) == I                                            # lm_row_stride < lm_width
    assert wstep(dr, stride=V - 1) == I                                             # row_stride < V
    assert wstep(dr, pl_=None) == I                                                 # NULL lm_scores before the last step
    assert wstep(dr, pw_=None) == I                                                 # next_word is required
    assert wstep(dr, pr_=pr, nlm=0) == I                                            # lm_row_of and no LM rows
    assert wstep(dr, pr_=pr, nlm=1) == 0
    assert wstep(dr) == 0                                                           # identity: n_lm_rows ignored
    with pytest.raises(_capi.FltxError) as e:
        dz.step(sc, lm_scores=lr)
    assert e.value.code == S
    with pytest.raises(_capi.FltxError) as e:
        dz.step(sc, lm_row_of=ro)
    assert e.value.code == S
    with pytest.raises(_capi.FltxError) as e:
        dr.step(sc)
    assert e.value.code == S and "LexiconSeq2SeqBatchDecoder" in str(e.value)
    assert dr.has_rows_lm and dr.has_word_rows_lm and not dz.has_rows_lm and not dz.has_word_rows_lm
    assert len(dr.step(sc, lm_scores=lr)) == 5
    if is_gpu(sess):
        sess.ctx.synchronize()
    dr.close()
    dz.close()
    lm.close()


def test_step_after_done_and_restart(sess):
    """A step after the last one lists no rows and no words, writes NaN lse and changes no result; NULL rows are
    accepted there; a decoder that begins again restarts from the root."""
    c = _case("perm_wide_finish")
    t = _case_trie(c, sess.lib)
    want, _, _ = G.restate_case(c, trie_nodes(t))
    rl = G.case_lm(c)
    lm = word_lm(sess, rl)
    K, V, W = c["K"], c["V"], c["W"]
    dec = case_dec(sess, c, t, lm)
    dec.begin(1, V)
    dec.step(_dev(sess, np.repeat(G.case_model(c).row([])[None, :], K, 0)),
             lm_scores=_dev(sess, np.repeat(rl.row([])[None, :], K, 0)))
    for _ in range(2):
        got, _, merges, _ = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], V, W)
        compare(want, got[0])
        assert merges == [c["merges"]]
    lse = _dev(sess, np.full(K, 7.0))
    out = dec.step(_dev(sess, np.zeros((K, V), np.float32)), lm_scores=_dev(sess, np.zeros((K, W), np.float32)),
                   lm_kind="logits", lm_lse_out=lse)
    if is_gpu(sess):
        sess.ctx.synchronize()
    assert _np(out[3]).tolist() == [0] and (_np(out[0]) == -1).all() and (_np(out[4]) == -1).all()
    assert np.isnan(_np(lse)).all()
    o = _outs(sess, 1, K)
    assert sess.lib.lib.fltx_s2s_step_word_lm_rows(dec.h, None, 0, 0, V, None, 0, 0, W, None, 0, 1, None, None, None,
                                                   _addr(o[0]), _addr(o[1]), _addr(o[2]), _addr(o[3]), _addr(o[4])) == 0
    dec.end()
    assert [(h.tokens.tolist(), h.words.tolist()) for h in dec.results(0)] == [(w[3], w[4]) for w in want]
    dec.close()
    lm.close()


def test_full_state_table_is_reported(sess):
    """A table of 3 LM states: the utterance stops and says so (never a silent wrong merge); with the default table
    the same decode completes."""
    c = _case("merge_max")
    t = _case_trie(c, sess.lib)
    rl = G.case_lm(c)
    lm = word_lm(sess, rl)
    dec = case_dec(sess, c, t, lm)
    dec.set_max_states(3)
    run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"], fetch=False)
    with pytest.raises(_capi.FltxError, match="LM-state table full"):
        dec.results(0)
    dec.set_max_states(1 << 16)
    got, _, _, _ = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"])
    assert [g[3] for g in got[0]] == [h[3] for h in c["hyps"]]
    dec.close()
    lm.close()


# ---- 8. the reference's Python surface (GPU only: the compat package makes its own context) -----------------------------
def _compat_three_element_update_func(gpu_sess):
    """The compat LexiconSeq2SeqDecoder with a WordRowsLM and is_token_lm=False: update_func returns (scores, states,
    lm_scores), lm_scores[k] the LM row of hypothesis k, whose word prefix update_func keeps with the decoder's
    raw_words; the n-best equals the batched decoder's at B = 1 and the reference fixture.  A two-element return raises."""
    compat = os.path.join(ROOT, "text_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    from flashlight.lib.text.decoder import (LexiconSeq2SeqDecoder, LexiconSeq2SeqDecoderOptions,
                                             create_emitting_model_state, get_obj_from_emitting_model_state)
    c = _case("homophones")
    m, rl = G.case_model(c), G.case_lm(c)
    t = _case_trie(c, gpu_sess.lib)
    lm = word_lm(gpu_sess, rl)
    dec = case_dec(gpu_sess, c, t, lm)
    want, _, _, _ = run_device(gpu_sess, dec, [m], [rl], c["maxlen"], c["V"], c["W"])
    dec.close()
    box = {}

    def update(emissions, N, T, raw_y, raw_beam, prev_states, t_, n_ret=3):
        scores, states, lms = [], [], []
        for k, (y, st) in enumerate(zip(raw_y, prev_states)):
            if t_ == 0:
                p = ([], ())
            else:
                tp, wp = get_obj_from_emitting_model_state(st)
                w = box["dec"].raw_words[k]
                p = (tp + [y], wp + ((w,) if w >= 0 else ()))
            r = m.row(p[0])
            scores.append((r if r is not None else np.zeros(c["V"], np.float32)).tolist())
            states.append(create_emitting_model_state(p) if r is not None else None)
            lms.append(rl.row(list(p[1])).tolist())
        return (scores, states, lms)[:n_ret]
    opts = LexiconSeq2SeqDecoderOptions(c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"],
                                        c["log_add"])
    cd = box["dec"] = LexiconSeq2SeqDecoder(opts, t, lm, c["eos"], update, c["maxlen"], False)
    cd.decode_step(0, 1, c["V"])
    got = cd.get_all_final_hypothesis()
    assert len(got) == len(want[0]) == len(c["hyps"])
    for g, w, f in zip(got, want[0], c["hyps"]):
        assert g.tokens == w[3] == f[3] and g.words == w[4] == f[4]
        assert _bits_equal([g.score, g.emittingModelScore, g.lmScore], w[:3])
    two = box["dec"] = LexiconSeq2SeqDecoder(opts, t, lm, c["eos"], lambda *a: update(*a, n_ret=2), c["maxlen"], False)
    with pytest.raises(ValueError):
        two.decode_step(0, 1, c["V"])
    with pytest.raises(_capi.FltxError) as e:
        LexiconSeq2SeqDecoder(opts, t, lm, c["eos"], update, c["maxlen"], True)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "rows LM" in str(e.value)


if CHILD:  # (GPU-only cases: defined in the child alone)
    test_compat_three_element_update_func = pytest.mark.gpu(_compat_three_element_update_func)


@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_S2S_WORDLMROWS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
