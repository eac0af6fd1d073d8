"""Lexicon seq2seq shallow fusion with a rows LM (fltx_s2s_lex_decoder_create with fltx_lm_rows_create and is_lm_token,
fltx_s2s_step_lm_rows; text_amd/csrc/fltx_s2s_lex.h "LM rows").

The LM's answers arrive per step as rows next to the model's rows; a record entry's token move, its word end (the first
label) and eos read the entry's one LM score; the LM's state is the token prefix, so two segmentations of one token
string meet in one state and merge.  The checks: the compiled reference's fixtures (tests/golden/
make_lex_s2s_lm_rows_golden.py: the restatement reproduces them, the device reproduces them); the row contract after
merges; random batches against the float64 restatement of tests/test_lexicon_seq2seq.py with an LM adapter whose states
are named as the reference driver's; the n-gram device path as a cross-check; typed LM rows in lockstep with float32
rows; the ABI's contract; the compat decoder.

Every decoder created here with a rows LM and is_lm_token=True is refused (FLTX_ERR_UNSUPPORTED) before this feature.
Every device test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
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

CHILD = os.environ.get("FLTX_LEX_S2S_LMROWS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from golden import make_lex_s2s_lm_rows_golden as G  # noqa: E402
from golden.make_s2s_lm_rows_golden import SmRowsLM  # noqa: E402
from test_lexicon_seq2seq import (_GpuSess, _np, compare, host_trie, is_gpu, make_lexicon, restate_lex,  # noqa: E402
                                  sm_model, trie_nodes)
from test_lexicon_seq2seq import run_device as run_device_tables  # noqa: E402
from test_seq2seq import HostLM  # noqa: E402
from test_seq2seq_model_output import BF16, F16, F32, _bits_equal, ref_lse, to_dtype, widen  # noqa: E402

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


def _dev(sess, a, dt=F32):
    """a numpy array as the step takes it on this backend: itself (emulator) or a device tensor"""
    if not is_gpu(sess):
        return a
    import torch
    t = torch.from_numpy(a.view(np.int16) if dt == BF16 else a).cuda()
    return t.view(torch.bfloat16) if dt == BF16 else t


def rows_lm(sess, rl):
    """the library's LM object of a rows LM of the tests (usr_to_lm, W, finish)"""
    ident = np.array_equal(rl.usr_to_lm, np.arange(len(rl.usr_to_lm)))
    return _capi.RowsLM(rl.W, None if ident else rl.usr_to_lm, rl.finish, lib=sess.lib)


def make_dec(sess, trie, lm, K, Kt, thr=1e9, lmw=0.0, word_score=0.0, eos_score=0.0, eos=0, maxlen=5, log_add=False,
             is_lm_token=True):
    return _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_lex_options(K, Kt, thr, lmw, word_score, eos_score,
                                                                               log_add), trie, lm, eos, maxlen,
                                            is_lm_token)


def _trim(r):
    r = list(r)
    while r and r[-1] == []:
        r.pop()
    return r


# ---- the device loop (test_lexicon_seq2seq.run_device with the LM's rows next to the model's) --------------------------
def run_device(sess, dec, models, lms, maxlen, V, W, feed=None, pad=np.nan, fetch=True):
    """All utterances in one batch: models[b].row(prefix) -> V float32 (None: the row is dropped), lms[b].row(prefix)
    -> W float32.  Padding and dropped rows hold `pad` in both matrices (never read).
    -> (final per utterance [(score, am, lm, tokens, words)], rows per step per utterance, merges per utterance)"""
    B, K = len(models), int(dec.options.beam_size)
    tok, beam, src, n = dec.begin(B, V)
    prefix = {(b, 0): [] for b in range(B)}
    rows = [[] for _ in range(B)]
    gpu = is_gpu(sess)
    for t in range(maxlen + 2):  # (two steps more than it takes: a step after the last one is a no-op)
        if gpu:
            dec.ctx.synchronize()
        tok_h, beam_h, src_h, n_h = _np(tok), _np(beam), _np(src), _np(n)
        if t > 0:
            for b in range(B):
                rows[b].append([(int(tok_h[b, k]), int(beam_h[b, k]), int(src_h[b, k]) - b * K if src_h[b, k] >= 0
                                 else None) for k in range(n_h[b])])
                assert (tok_h[b, n_h[b]:] == -1).all() and (src_h[b, n_h[b]:] == -1).all(), (t, b)
        sc = np.full((B * K, V), pad, dtype=np.float32)
        lr = np.full((B * K, W), pad, dtype=np.float32)
        valid = np.zeros(B * K, dtype=np.uint8)
        newpre = {}
        for b in range(B):
            for k in range(n_h[b]):
                p = [] if t == 0 else prefix[(b, int(src_h[b, k]) - b * K)] + [int(tok_h[b, k])]
                newpre[(b, k)] = p
                r = models[b].row(p)
                if r is None:
                    continue
                sc[b * K + k] = r
                lr[b * K + k] = lms[b].row(p)
                valid[b * K + k] = 1
        prefix = newpre
        if feed is not None:
            tok, beam, src, n = feed(dec, sc, lr, valid)
        else:
            tok, beam, src, n = dec.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, lr))
    assert dec.done()
    merges = dec.info()["merges"]
    dec.end()
    out = [[(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in dec.results(b)] for b in range(B)] \
        if fetch else None
    return out, [_trim(r) for r in rows], merges


# ---- 1. fixtures of the reference itself ------------------------------------------------------------------------------
def _golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "lexicon_seq2seq_lm_rows_expected.json.gz"), "rt") as f:
        return json.load(f)


def _case(name):
    return next(c for c in _golden() if c["name"] == name)


def _case_trie(c, lib):
    return host_trie(lib, c["V"], G.lexicon(c), 0)


def test_fixtures_cover_the_ground():
    cs = _golden()
    assert all(8 <= c["V"] <= 16 and 8 <= c["K"] <= 32 and c["Kt"] <= c["V"] and 6 <= c["maxlen"] <= 8
               for c in cs if c["name"] not in ("k1", "v300_kt256"))
    assert sum(1 for c in cs if c["min_merges"] >= 1 and c["merges"] >= 1) >= 2
    assert any(c["log_add"] and c["merges"] for c in cs) and any(not c["log_add"] and c["merges"] for c in cs)
    for c in cs:
        um = G.case_lm(c).usr_to_lm
        c["finish_ne"] = c["finish"] >= 0 and c["finish"] != int(um[c["eos"]])
        c["permuted"] = not np.array_equal(um, np.arange(c["V"]))
    assert any(c["permuted"] and c["W"] > c["V"] and c["finish_ne"] for c in cs)
    assert any(c["drop"] > 0 for c in cs)
    assert any(c["lmw"] == 0 and not c["inf_mod"] and all(h[2] != 0.0 for h in c["hyps"]) for c in cs)  # (lm accumulates)
    assert any(c["lmw"] == 0 and c["inf_mod"] and c["infs"] > 0 and all(np.isfinite(h[2]) for h in c["hyps"])
               for c in cs)  # (a -inf entry was read; no candidate carries it)
    assert any(c["word_score"] != 0 and c["lex"][5] >= 0.8 for c in cs)
    assert any(any(h[3][-1] != c["eos"] for h in c["hyps"]) for c in cs)  # (max_output_length with live hypotheses)
    assert any(c["K"] == 1 for c in cs)
    assert any((c["V"], c["Kt"], c["K"], c["maxlen"]) == (300, 256, 4, 3) for c in cs)


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c, emu_session):
    """The restatement, its LM states named as the driver's (prefix; finish its own child), against the compiled
    reference: tokens and words exact; scores bit for bit, within 1e-5 where a logAdd merge fed them; the merge count
    as recorded, no tie."""
    ties, stats = [], {}
    got, _, _ = G.restate_case(c, trie_nodes(_case_trie(c, emu_session.lib)), ties=ties, stats=stats)
    assert not ties and stats.get("merges", 0) == c["merges"]
    assert G.same(got, c["hyps"], c["log_add"]), (got[:2], c["hyps"][:2])


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess):
    """The device against the compiled reference: tokens, words exact; the three scores bit for bit under max, within
    compare()'s bound where a logAdd merge fed them; the rows of every step and the merge count are the restatement's."""
    t = _case_trie(c, sess.lib)
    want, wrows, _ = G.restate_case(c, trie_nodes(t))
    rl = G.case_lm(c)
    lm = rows_lm(sess, rl)
    dec = make_dec(sess, t, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                   c["maxlen"], c["log_add"])
    got, rows, merges = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"])
    dec.close()
    lm.close()
    ref = [tuple(h[:5]) + (w[5],) for h, w in zip(c["hyps"], want)]
    assert len(ref) == len(c["hyps"]) == len(want)
    compare(ref, got[0])
    assert rows[0] == _trim(wrows)
    assert merges == [c["merges"]]


# ---- 2. the row contract after merges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["merge_max", "merge_logadd", "dropped_rows_logadd"])
def test_rows_after_merges(sess, name):
    """Every step's next_token / next_beam_idx / next_src_row / n_rows against the restatement's rows, whose merged
    survivor is its group's best member (restate_lex keeps g[0] of the group sorted by score): the survivor lists that
    member's src_row, which is what the caller's index_select of the model's and the LM's state needs.  The merge count
    of fltx_s2s_lex_info is the restatement's."""
    c = _case(name)
    t = _case_trie(c, sess.lib)
    stats = {}
    want, wrows, _ = G.restate_case(c, trie_nodes(t), stats=stats)
    assert stats["merges"] >= 1
    rl = G.case_lm(c)
    lm = rows_lm(sess, rl)
    dec = make_dec(sess, t, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                   c["maxlen"], c["log_add"])
    got, rows, merges = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"])
    wrows = _trim(wrows)
    assert len(rows[0]) == len(wrows)
    for step, (g, w) in enumerate(zip(rows[0], wrows)):
        assert g == w, (step, g, w)
    assert merges == [stats["merges"]]
    compare(want, got[0])
    dec.close()
    lm.close()


# ---- 3. random batches against the restatement ------------------------------------------------------------------------
def _restate(model, rl, nodes, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add, ties=None, stats=None):
    return restate_lex(model, nodes, G.PrefixObjLM(rl), K, Kt, thr, lmw, ws, es, eos, maxlen, log_add, True, ties=ties,
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


def batch_case(sess, rng, B, V, K, Kt, W, perm, finish, thr, lmw, ws, es, eos, maxlen, drop, log_add, lex, pad=np.nan):
    t = host_trie(sess.lib, V, lex, 0)
    nodes = trie_nodes(t)
    biases = [float(x) for x in rng.choice([0.0, 0.4, 0.9], B)]  # (utterances of one batch end at different steps)

    def mk(b):
        return lambda seed: (sm_model(seed, V, eos, biases[b], drop), SmRowsLM(seed ^ 0x77, V, W, perm, finish, eos))
    found = [tie_free(int(rng.integers(1 << 30)), mk(b), nodes, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add)
             for b in range(B)]
    pairs = [mk(b)(found[b][0]) for b in range(B)]
    lm = rows_lm(sess, pairs[0][1])
    dec = make_dec(sess, t, lm, K, Kt, thr, lmw, ws, es, eos, maxlen, log_add)
    got, rows, merges = run_device(sess, dec, [p[0] for p in pairs], [p[1] for p in pairs], maxlen, V, W, pad=pad)
    for b in range(B):  # (no utterance skipped)
        wf, wr = found[b][1]
        compare(wf, got[b])
        assert rows[b] == _trim(wr), (b, rows[b], _trim(wr))
    assert merges == [f[2] for f in found]
    dec.close()
    lm.close()
    return sum(merges)


def test_random_batches(sess):
    """B = 3-4 utterances with their own seeds and lengths in one decoder; mixed dropped rows and padding (NaN, or
    garbage where nothing may be read)."""
    rng = np.random.default_rng(2024)
    total = 0
    for _ in range(4 if is_gpu(sess) else 8):
        V = int(rng.choice([8, 11, 16]))
        eos = int(rng.integers(0, V))
        K = int(rng.integers(2, 25))
        W = V + int(rng.choice([0, 5]))
        lex = make_lexicon(V, eos, int(rng.integers(20, 50)), int(rng.integers(1 << 20)), max_len=3,
                           respell=float(rng.choice([0.2, 0.5])), single=0.4)
        total += batch_case(sess, rng, int(rng.integers(3, 5)), V, K, int(rng.integers(2, V + 3)), W,
                            int(rng.choice([0, 91])), int(rng.choice([-1, W - 1])), float(rng.choice([3.0, 1e9])),
                            float(rng.choice([0.0, 0.5, 1.1])), float(rng.choice([0.6, -0.3])),  # (word_score 0: a word end ties with its token move)
                            float(rng.choice([0.0, -0.3])), eos, int(rng.integers(2, 8)),
                            float(rng.choice([0.0, 0.1])), bool(rng.integers(2)), lex,
                            pad=float(rng.choice([np.nan, 1e30])))
    assert total > 0


# ---- 4. the n-gram path as a cross-check --------------------------------------------------------------------------------
class _NgramRows:
    """LM rows from a token n-gram's host twin: row(prefix)[v] = score(context after the prefix, v) for every token,
    and finish into an extra column."""

    def __init__(self, ng, V):
        self.hl, self.V, self.W = HostLM(ng), V, V + 1
        self.usr_to_lm, self.finish = np.arange(V, dtype=np.int32), V
        self.ctx = {(): self.hl.start()}

    def row(self, prefix):
        p = tuple(prefix)
        for i in range(1, len(p) + 1):
            if p[:i] not in self.ctx:
                self.ctx[p[:i]] = self.hl.score(self.ctx[p[:i - 1]], p[i - 1])[0]
        c = self.ctx[p]
        r = np.zeros(self.W, np.float32)
        for v in range(self.V):
            r[v] = self.hl.score(c, v)[1]
        r[self.V] = self.hl.finish(c)[1]
        return r


@pytest.mark.parametrize("lmw", [0.6, 0.0])
def test_equals_the_ngram_device_decode(sess, tmp_path_factory, lmw):
    """A token 3-gram over V = 10: the rows-LM decode with is_lm_token equals the n-gram device decode with
    is_lm_token -- n-best, rows of every step and merge counts; exact (max merge), on tie-free seeds."""
    V, K, Kt, eos, maxlen, B = 10, 16, 10, 9, 6, 3
    path = str(tmp_path_factory.mktemp("lex_s2s_lmrows") / "t10_s6.arpa")
    vocab = ngram_synth.words(V, "t")
    ngram_synth.write_arpa(path, vocab, 3, (0, 300, 150), 6)
    ng = _capi.ArpaLM(path, vocab, lib=sess.lib)
    lex = make_lexicon(V, eos, 30, 31, max_len=3, respell=0.3, single=0.4)
    t = host_trie(sess.lib, V, lex, 0)
    nodes = trie_nodes(t)
    nr = _NgramRows(ng, V)
    seeds = [tie_free(500 + 100 * b, lambda s: (sm_model(s, V, eos, 0.5), nr), nodes, K, Kt, 1e9, lmw, 0.2, -0.1, eos,
                      maxlen, False)[0] for b in range(B)]
    models = [sm_model(s, V, eos, 0.5) for s in seeds]
    want, wrows, wmerges = run_device_tables(sess, models, t, ng, K, Kt, 1e9, lmw, 0.2, -0.1, eos, maxlen, V, False, True)
    lm = _capi.RowsLM(V + 1, None, V, lib=sess.lib)
    dec = make_dec(sess, t, lm, K, Kt, 1e9, lmw, 0.2, -0.1, eos, maxlen, False)
    got, rows, merges = run_device(sess, dec, models, [nr] * B, maxlen, V, V + 1)
    for b in range(B):
        assert len(got[b]) == len(want[b])
        for g, w in zip(got[b], want[b]):
            assert g[3] == w[3] and g[4] == w[4] and _bits_equal(g[:3], w[:3]), (b, g, w)
        assert rows[b] == _trim(wrows[b])
    assert merges == wmerges and sum(merges) > 0
    dec.close()
    lm.close()
    ng.close()


# ---- 5. typed LM rows in lockstep -----------------------------------------------------------------------------------------
def lockstep(sess, c, dtl, kindl, host=False):
    """A steps on LM rows of type dtl (log-probs, or logits: kindl) that hold round-to-nearest of the case's LM rows; R
    on float32 rows holding the values A's rows stand for (widened; for logits (float)((double)x - lse) with the lse A's
    step reports, itself checked against a float64 log-sum-exp).  Rows at every step, n-best and the three scores are
    bit-identical."""
    t = _case_trie(c, sess.lib)
    m, rl = G.case_model(c), G.case_lm(c)
    lm = rows_lm(sess, rl)
    K, V, W, maxlen = c["K"], c["V"], c["W"], c["maxlen"]
    A, R = (make_dec(sess, t, lm, K, c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"], maxlen,
                     c["log_add"]) for _ in range(2))
    gpu = is_gpu(sess)
    outA, outR = A.begin(1, V), R.begin(1, V)
    prefix = {0: []}
    n_lse = 0
    for step in range(maxlen + 2):
        if gpu:
            sess.ctx.synchronize()
        ta, tr = [_np(o).copy() for o in outA], [_np(o).copy() for o in outR]
        for x, y, name in zip(ta, tr, ("token", "beam_idx", "src_row", "n_rows")):
            assert np.array_equal(x, y), (step, name, x.tolist(), y.tolist())
        tok_h, src_h, n_h = ta[0], ta[2], int(ta[3][0])
        sc = np.full((K, V), np.nan, np.float32)
        l64 = np.full((K, W), np.nan)
        valid = np.zeros(K, np.uint8)
        newpre = {}
        for k in range(n_h):
            p = [] if step == 0 else prefix[int(src_h[0, k])] + [int(tok_h[0, k])]
            newpre[k] = p
            r = m.row(p)
            if r is None:
                continue
            sc[k], valid[k] = r, 1
            l64[k] = rl.row(p).astype(np.float64) * (3.0 if kindl else 1.0)
        prefix = newpre
        lraw = to_dtype(l64, dtl)
        lw = widen(lraw, dtl)
        lse = None
        if kindl:
            lse = _dev(sess, np.full(K, 7.0))  # (device memory on the HIP library, also with host-staged rows)
        kw = dict(lm_kind="logits" if kindl else "log_probs", lm_lse_out=lse)
        if host or not gpu:
            outA = A.step(sc, valid, lm_scores=lraw, lm_dtype="bf16" if dtl == BF16 else None, **kw)
        else:
            outA = A.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, lraw, dtl), **kw)
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
    A.close()
    R.close()
    lm.close()
    return n_lse


def test_bf16_log_probs_lm_rows(sess):
    assert lockstep(sess, _case("perm_wide_finish"), BF16, 0) == 0


def test_fp16_logits_lm_rows(sess):
    assert lockstep(sess, _case("merge_max"), F16, 1) > 0


def test_host_staged_rows(sess):
    """Host rows (numpy on the HIP library: on_device == 0) of both matrices are staged in their own type: bf16 logits
    in lockstep, and a float32 fixture decode."""
    assert lockstep(sess, _case("perm_wide_finish"), BF16, 1, host=True) > 0
    c = _case("merge_logadd")
    t = _case_trie(c, sess.lib)
    want, wrows, _ = G.restate_case(c, trie_nodes(t))
    rl = G.case_lm(c)
    lm = rows_lm(sess, rl)
    dec = make_dec(sess, t, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                   c["maxlen"], c["log_add"])
    got, rows, merges = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"],
                                   feed=lambda d, sc, lr, valid: d.step(sc, valid, lm_scores=lr))
    compare(want, got[0])
    assert rows[0] == _trim(wrows) and merges == [c["merges"]]
    dec.close()
    lm.close()


# ---- 6. the contract ----------------------------------------------------------------------------------------------------
def _outs(sess, B, K):
    if is_gpu(sess):
        import torch
        return [torch.zeros(B * K, dtype=torch.int32, device="cuda") for _ in range(3)] + \
            [torch.zeros(B, dtype=torch.int32, device="cuda")]
    return [np.zeros(B * K, np.int32) for _ in range(3)] + [np.zeros(B, np.int32)]


def _addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def test_contract_and_refusals(sess):
    L, ctx = sess.lib, sess.ctx
    U, I, S = _capi.ERR_UNSUPPORTED, _capi.ERR_INVALID, _capi.ERR_STATE
    V, K, eos = 6, 4, 1
    trie = host_trie(L, V, make_lexicon(V, eos, 8, 1), 0)
    lm = _capi.RowsLM(lib=L)
    h = C.c_void_p()
    opts = _capi.make_s2s_lex_options(K, 4, lm_weight=0.5)
    # a word-level rows LM stays refused; a token-level one is accepted
    assert L.lib.fltx_s2s_lex_decoder_create(ctx.h, C.byref(opts), trie.h, lm.h, eos, 5, 0, C.byref(h)) == U
    assert "rows LM" in L.lib.fltx_last_error().decode()
    with pytest.raises(_capi.FltxError) as e:
        make_dec(sess, trie, lm, K, 4, is_lm_token=False)
    assert e.value.code == U and "rows LM" in str(e.value)
    po = [_addr(o) for o in _outs(sess, 1, K)]

    def begin(lmx, V_, eos_=eos, Kt=4, lmw=0.5):
        d = make_dec(sess, trie, lmx, K, Kt, lmw=lmw, eos=eos_, maxlen=5)
        rc = L.lib.fltx_s2s_begin(d.h, 1, V_, *po)
        d.close()
        return rc
    assert begin(_capi.RowsLM(0, [0, 1, 2, 3, 4], -1, lib=L), V) == I        # V > n_usr: a short map
    assert begin(_capi.RowsLM(0, [0, 1, 2, 3, 4, 5], -1, lib=L), V) == 0
    assert begin(_capi.RowsLM(0, [0, 1, 2, 3, 4, 9], -1, lib=L), V) == I     # lm_width 0 (= V) and a map that leaves it
    assert begin(_capi.RowsLM(0, None, 7, lib=L), V) == I                    # ... and a finish index that does
    assert begin(_capi.RowsLM(4, None, -1, lib=L), V) == I                   # identity into narrower rows
    assert begin(_capi.RowsLM(8, None, 7, lib=L), V) == 0
    assert begin(lm, 300, Kt=257) == U and begin(lm, 300, Kt=256) == 0       # the token beam's limit is 256, with LM terms
    # the step entry points
    dr = make_dec(sess, trie, lm, K, 4, lmw=0.5, eos=eos, maxlen=5)
    dz = make_dec(sess, trie, sess.zero, K, 4, eos=eos, maxlen=5)
    sc, lr = _dev(sess, np.zeros((K, V), np.float32)), _dev(sess, np.zeros((K, V), np.float32))
    ps, pl = _addr(sc), _addr(lr)
    step = L.lib.fltx_s2s_step_lm_rows
    assert step(dr.h, ps, 0, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == S      # before fltx_s2s_begin
    dr.begin(1, V)
    dz.begin(1, V)
    assert L.lib.fltx_s2s_step(dr.h, ps, 1, V, None, *po) == S
    assert L.lib.fltx_s2s_step_typed(dr.h, ps, 0, 1, 1, V, None, None, *po) == S
    assert step(dz.h, ps, 0, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == S      # a lexicon decoder without a rows LM
    assert step(dr.h, ps, 0, 0, V, pl, 3, 0, V, 1, None, None, None, *po) == I      # lm_dtype
    assert step(dr.h, ps, 0, 0, V, pl, 0, 2, V, 1, None, None, None, *po) == I      # lm_kind
    assert step(dr.h, ps, 0, 0, V, pl, 0, 0, V - 1, 1, None, None, None, *po) == I  # lm_row_stride < lm_width
    assert step(dr.h, ps, 0, 0, V - 1, pl, 0, 0, V, 1, None, None, None, *po) == I  # row_stride < V
    assert step(dr.h, ps, 0, 0, V, None, 0, 0, V, 1, None, None, None, *po) == I    # NULL lm_scores before the last step
    assert step(dr.h, ps, 0, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == 0
    with pytest.raises(_capi.FltxError) as e:
        dz.step(sc, lm_scores=lr)
    assert e.value.code == S
    with pytest.raises(_capi.FltxError) as e:
        dr.step(sc)
    assert e.value.code == S and "LexiconSeq2SeqBatchDecoder" in str(e.value)
    assert dr.has_rows_lm and not dz.has_rows_lm
    if is_gpu(sess):
        sess.ctx.synchronize()
    dr.close()
    dz.close()
    lm.close()


def test_step_after_done_and_restart(sess):
    """A step after the last one lists no rows, writes NaN lse and changes no result; NULL rows are accepted there; a
    decoder that begins again restarts from the root."""
    c = _case("perm_wide_finish")
    t = _case_trie(c, sess.lib)
    want, _, _ = G.restate_case(c, trie_nodes(t))
    rl = G.case_lm(c)
    lm = rows_lm(sess, rl)
    K, V, W = c["K"], c["V"], c["W"]
    dec = make_dec(sess, t, lm, K, c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"], c["maxlen"],
                   c["log_add"])
    dec.begin(1, V)
    dec.step(_dev(sess, np.repeat(G.case_model(c).row([])[None, :], K, 0)),
             lm_scores=_dev(sess, np.repeat(rl.row([])[None, :], K, 0)))
    for _ in range(2):
        got, _, merges = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], V, W)
        compare(want, got[0])
        assert merges == [c["merges"]]
    lse = _dev(sess, np.full(K, 7.0))
    out = dec.step(_dev(sess, np.zeros((K, V), np.float32)), lm_scores=_dev(sess, np.zeros((K, W), np.float32)),
                   lm_kind="logits", lm_lse_out=lse)
    if is_gpu(sess):
        sess.ctx.synchronize()
    assert _np(out[3]).tolist() == [0] and (_np(out[0]) == -1).all() and np.isnan(_np(lse)).all()
    outs = dec._rows()
    assert sess.lib.lib.fltx_s2s_step_lm_rows(dec.h, None, 0, 0, V, None, 0, 0, W, 1, None, None, None,
                                              *[dec._addr(o) for o in outs]) == 0
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
    lm = rows_lm(sess, rl)
    dec = make_dec(sess, t, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                   c["maxlen"], c["log_add"])
    dec.set_max_states(3)
    run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"], fetch=False)
    with pytest.raises(_capi.FltxError, match="LM-state table full"):
        dec.results(0)
    dec.set_max_states(1 << 16)
    got, _, _ = run_device(sess, dec, [G.case_model(c)], [rl], c["maxlen"], c["V"], c["W"])
    assert [g[3] for g in got[0]] == [h[3] for h in c["hyps"]]
    dec.close()
    lm.close()


# ---- 7. the reference's Python surface (GPU only: the compat package makes its own context) -----------------------------
def _compat_three_element_update_func(gpu_sess):
    """The compat LexiconSeq2SeqDecoder with a RowsLM and is_token_lm: update_func returns (scores, states, lm_scores);
    the n-best equals the batched decoder's at B = 1 (and the reference fixture).  A two-element return raises."""
    compat = os.path.join(ROOT, "text_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    from flashlight.lib.text.decoder import (LexiconSeq2SeqDecoder, LexiconSeq2SeqDecoderOptions,
                                             create_emitting_model_state, get_obj_from_emitting_model_state)
    c = _case("perm_wide_finish")
    m, rl = G.case_model(c), G.case_lm(c)
    t = _case_trie(c, gpu_sess.lib)
    lm = rows_lm(gpu_sess, rl)
    dec = make_dec(gpu_sess, t, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"], c["eos"],
                   c["maxlen"], c["log_add"])
    want, _, _ = run_device(gpu_sess, dec, [m], [rl], c["maxlen"], c["V"], c["W"])
    dec.close()

    def update(emissions, N, T, raw_y, raw_beam, prev_states, t_, n_ret=3):
        scores, states, lms = [], [], []
        for y, st in zip(raw_y, prev_states):
            p = [] if t_ == 0 else get_obj_from_emitting_model_state(st) + [y]
            r = m.row(p)
            scores.append((r if r is not None else np.zeros(c["V"], np.float32)).tolist())
            states.append(create_emitting_model_state(p) if r is not None else None)
            lms.append(rl.row(p).tolist())
        return (scores, states, lms)[:n_ret]
    opts = LexiconSeq2SeqDecoderOptions(c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"], c["eos_score"],
                                        c["log_add"])
    cd = LexiconSeq2SeqDecoder(opts, t, lm, c["eos"], update, c["maxlen"], True)
    cd.decode_step(0, 1, c["V"])
    got = cd.get_all_final_hypothesis()
    assert len(got) == len(want[0]) == len(c["hyps"])
    for g, w, f in zip(got, want[0], c["hyps"]):
        assert g.tokens == w[3] == f[3] and g.words == w[4] == f[4]
        assert _bits_equal([g.score, g.emittingModelScore, g.lmScore], w[:3])
    two = LexiconSeq2SeqDecoder(opts, t, lm, c["eos"], lambda *a: update(*a, n_ret=2), c["maxlen"], True)
    with pytest.raises(ValueError):
        two.decode_step(0, 1, c["V"])
    with pytest.raises(_capi.FltxError) as e:
        LexiconSeq2SeqDecoder(opts, t, lm, c["eos"], update, c["maxlen"], False)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "rows LM" in str(e.value)


if CHILD:  # (GPU-only cases: defined in the child alone)
    test_compat_three_element_update_func = pytest.mark.gpu(_compat_three_element_update_func)


@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_S2S_LMROWS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
