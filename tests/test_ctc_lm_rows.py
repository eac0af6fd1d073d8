"""Lexicon-free CTC shallow fusion with a rows LM (fltx_ctc_rows_*, text_amd/csrc/fltx_ctc_rows.h).

The LM's answers arrive per frame step as rows, one per LM state; the decoder lists for every hypothesis its parent's row,
the token that advanced its LM state and a canonical state id.  The checks: the compiled reference's fixtures (tests/
golden/make_ctc_lm_rows_golden.py: the float64 restatement below reproduces them, the device reproduces them -- tokens
exact, the three scores bit-identical under max-merge and within 1e-5 under logAdd); the n-gram device decode of
fltx_decode_batch as a bit-for-bit cross-check; random batches, the row contract, lm_row_of, typed LM rows, the NaN and
-inf rules, the state-table limit, the ABI's contract and refusals, and the Python helper.

The restatement (`restate`) carries the token prefix as the LM state and counts its own ties -- equal emissions at the
token cut, equal scores at the K cut, among merge members and in the final order -- and the smallest gap at any decision
taken on scores (threshold, K cut, fold order, final order; the token cut compares float32 emissions, which are exact).
Every seeded case asserts zero ties on the restatement alone, every logAdd case a smallest gap above 1e-3.

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

CHILD = os.environ.get("FLTX_CTC_LMROWS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from golden import make_ctc_lm_rows_golden as G  # noqa: E402
from test_seq2seq import HostLM  # noqa: E402
from test_seq2seq_model_output import (BF16, F16, F32, _bits_equal, _GpuSess, _np, is_gpu, ref_lse, to_dtype,  # noqa: E402
                                       widen)

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
LOGADD_TOL = 1e-5  # the project's stated bound for logAdd decodes
MIN_GAP = 1e-3


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


# ---- the restatement --------------------------------------------------------------------------------------------------
class PrefixLM:
    """A host LM whose state is the token prefix: row_fn(prefix) -> the LM's row, read through usr_to_lm / finish."""

    def __init__(self, row_fn, usr_to_lm, finish):
        self.row_fn, self.usr_to_lm, self.fin = row_fn, usr_to_lm, finish
        self.rows = {}

    def start(self):
        return ()

    def _at(self, ctx, idx):
        if ctx not in self.rows:
            self.rows[ctx] = self.row_fn(ctx)
        return float(self.rows[ctx][idx])

    def score(self, ctx, n):
        return ctx + (n,), self._at(ctx, int(self.usr_to_lm[n]))

    def finish(self, ctx):
        return ctx + (-1,), self._at(ctx, self.fin)


class Stats:
    def __init__(self):
        self.ties, self.gap, self.merges, self.reentered = [], math.inf, 0, 0

    def decide(self, a, b):
        """a decision between scores a and b"""
        if not (math.isinf(a) and math.isinf(b)):
            self.gap = min(self.gap, abs(a - b))


def _store(cands, K, thr, log_add, st, where):
    """candidatesStore (Utils.h:146-225) on [dict(score, key, ...)] in candidate order -> the survivors, best first"""
    if not cands:
        return []
    best = max(c["score"] for c in cands)
    kept = []
    for c in cands:
        st.decide(c["score"], best - thr)
        if c["score"] >= best - thr:
            kept.append(c)
    groups = {}
    for c in kept:
        groups.setdefault(c["key"], []).append(c)
    merged = []
    for g in groups.values():
        g.sort(key=lambda c: -c["score"])
        acc = g[0]["score"]
        for prev, c in zip(g, g[1:]):
            if prev["score"] == c["score"]:
                st.ties.append((where, "merge members"))
            st.decide(prev["score"], c["score"])
            hi, lo = max(acc, c["score"]), min(acc, c["score"])
            acc = hi + math.log1p(math.exp(lo - hi)) if log_add and not math.isinf(hi) else hi
            st.merges += 1
        merged.append(dict(g[0], score=acc))
    merged.sort(key=lambda c: -c["score"])
    for i in range(min(len(merged) - 1, K)):
        if merged[i]["score"] == merged[i + 1]["score"]:
            st.ties.append((where, "K cut" if i == K - 1 else "order"))
        st.decide(merged[i]["score"], merged[i + 1]["score"])
    return merged[:K]


def restate(em, lm, K, Kt, thr, lmw, sil_score, sil, blank, log_add=False, st=None, hole=None):
    """One utterance: em [T, N] float32.  -> (final [(score, am, lm, tokens)], rows per frame [(src, token, state)]: the
    beam after each frame, best first, state = the prefix).  hole = (t, i): hypothesis i of the beam that frame t
    extends reads NaN LM entries (an lm_row_of entry out of range)."""
    st = st if st is not None else Stats()
    T, N = em.shape
    beam = [dict(score=0.0, am=0.0, lm=0.0, state=lm.start(), token=sil, pb=False, path=[sil])]
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
        for i, h in enumerate(beam):
            for n in kept:
                a = float(e[n])
                score = h["score"] + a
                if n == sil:
                    score += sil_score
                if n != blank and (n != h["token"] or h["pb"]):
                    state, l = lm.score(h["state"], n)
                    l = math.nan if hole == (t, i) else l
                    score = score + lmw * l
                    c = dict(score=score, am=h["am"] + a, lm=h["lm"] + l, state=state, token=n, pb=False, new=True)
                else:
                    c = dict(score=score, am=h["am"] + a, lm=h["lm"], state=h["state"], token=n, pb=n == blank, new=False)
                if math.isnan(c["score"]):
                    continue
                c.update(src=i, key=(c["state"], n, c["pb"]), path=h["path"] + [n])
                cands.append(c)
        beam = _store(cands, K, thr, log_add, st, t)
        for c in beam:
            if c["new"] and c["state"] in seen:
                st.reentered += 1
        seen.update(c["state"] for c in beam)
        rows.append([(c["src"], c["token"] if c["new"] else -1, c["state"]) for c in beam])
    cands = []
    for i, h in enumerate(beam):
        state, l = lm.finish(h["state"])
        score = h["score"] + lmw * l
        if not math.isnan(score):
            cands.append(dict(score=score, am=h["am"], lm=h["lm"] + l, key=(state, sil, False), path=h["path"] + [sil]))
    final = _store(cands, K, thr, log_add, st, "end")
    return [(c["score"], c["am"], c["lm"], c["path"]) for c in final], rows


# ---- the device loop ---------------------------------------------------------------------------------------------------
def make_dec(sess, lm, K, Kt, thr=1e9, lmw=0.0, sil_score=0.0, sil=0, blank=0, log_add=False):
    return _capi.CtcRowsBatchDecoder(sess.ctx, _capi.make_options(K, Kt, thr, lmw, sil_score=sil_score, log_add=log_add),
                                     lm, sil, blank)


def decode(sess, dec, ems, N, W, lm_row, per_state=False, feed=None, extra_steps=2, bad_rows=()):
    """All utterances in one batch: ems[b] is [T_b, N] float32, lm_row(b, prefix) -> W float32.  per_state: one LM row
    per state id, shared through lm_row_of (else one per hypothesis, identity).  bad_rows: (frame, b, k) whose lm_row_of
    entry is out of range.  Rows that hold no hypothesis are NaN (never read).  extra_steps more steps than frames are
    taken (a step after the last frame is a no-op).  feed(dec, lr, ro, end, scored) replaces the step / end call;
    scored marks the rows whose LM row this call reads: those of utterances with frames left, all of them at the end.
    -> (final per utterance [(score, am, lm, tokens)], rows per frame per utterance [(src, token, state id)], the
    prefix of every state id per utterance)"""
    B, K = len(ems), int(dec.options.beam_size)
    Ts = [e.shape[0] for e in ems]
    flat = np.concatenate([e.reshape(-1) for e in ems]) if sum(Ts) else np.zeros(0, np.float32)
    tok, src, state, n = dec.begin(flat, Ts, N)
    gpu = is_gpu(sess)
    prefix = [dict() for _ in range(B)]
    rows = [[] for _ in range(B)]
    prev_state = None
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
                    assert (s, int(tok_h[b, k]), sid, nb) == (-1, dec.sil, 0, 1)
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
        final.append([(h.score, h.am, h.lm, h.tokens.tolist()) for h in hs])
        assert all((h.words == -1).all() and len(h.tokens) == Ts[b] + 2 for h in hs)
    return final, rows, prefix


def assert_final(want, got, log_add, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (w, g) in enumerate(zip(want, got)):
        assert g[3] == list(w[3]), (what, i, g[3], w[3])
        if log_add:
            assert all(abs(x - y) <= LOGADD_TOL for x, y in zip(g[:3], w[:3])), (what, i, g[:3], w[:3])
        else:
            assert _bits_equal(g[:3], w[:3]), (what, i, g[:3], w[:3])


def assert_rows(want_rows, got_rows, prefix):
    """per frame and slot: the parent's slot and the token equal; the state ids name the restatement's states one to one"""
    assert len(got_rows) == len(want_rows)
    fwd, back = {}, {}
    for t, (wr, gr) in enumerate(zip(want_rows, got_rows)):
        assert len(gr) == len(wr), (t, len(gr), len(wr))
        for k, (w, g) in enumerate(zip(wr, gr)):
            assert g[:2] == w[:2], (t, k, g, w)
            assert fwd.setdefault(g[2], w[2]) == w[2] and back.setdefault(w[2], g[2]) == g[2], (t, k, g, w)
            assert prefix[g[2]] == w[2], (t, k)


def clean(case_fn, base, log_add, tries=400):
    """the first seed from `base` whose restatement has no tie (and, under logAdd, no gap below MIN_GAP)
    -> (seed, inputs, result, stats)"""
    for seed in range(base, base + tries):
        st = Stats()
        inp = case_fn(seed)
        res = restate(*inp, st=st)
        if not st.ties and (not log_add or st.gap > MIN_GAP):
            return seed, inp, res, st
    raise AssertionError("no clean seed in %d tries from %d" % (tries, base))


# ---- 1. fixtures of the reference itself ------------------------------------------------------------------------------
def _golden():
    path = os.path.join(ROOT, "tests", "golden", "ctc_lm_rows_expected.json.gz")
    if not os.path.exists(path):  # (the generator imports this module before it has written the file; the coverage test
        return []                 # below fails on an empty list)
    with gzip.open(path, "rt") as f:
        return json.load(f)


def _case_restate(c, st):
    rl = G.case_lm(c)
    lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
    return restate(G.emissions(c["seed"], c["T"], c["N"]), lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"],
                   c["sil"], c["blank"], c["log_add"], st=st)


def test_fixtures_cover_the_cases():
    cs = _golden()
    assert {c["T"] for c in cs} == {1, 7, 12} and {c["N"] for c in cs} == {3, 6} and {c["K"] for c in cs} == {1, 2, 8}
    assert {c["lmw"] for c in cs} == {0.0, 0.7}
    assert any(c["Kt"] < c["N"] for c in cs) and any(c["Kt"] == c["N"] for c in cs)
    assert any(c["thr"] < 100 for c in cs) and any(c["sil_score"] != 0 for c in cs)
    assert any(c["perm"] and c["W"] > c["N"] for c in cs) and any(c["log_add"] for c in cs)


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c):
    st = Stats()
    got, _ = _case_restate(c, st)
    assert not st.ties and (not c["log_add"] or st.gap > MIN_GAP), (st.ties, st.gap)
    assert_final(c["hyps"], got, c["log_add"], c["name"])


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess):
    st = Stats()
    _case_restate(c, st)
    assert not st.ties and (not c["log_add"] or st.gap > MIN_GAP)
    rl = G.case_lm(c)
    lm = _capi.RowsLM(rl.W, rl.usr_to_lm if c["perm"] else None, rl.finish, lib=sess.lib)
    dec = make_dec(sess, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"], c["sil"], c["blank"], c["log_add"])
    got, _, _ = decode(sess, dec, [G.emissions(c["seed"], c["T"], c["N"])], c["N"], rl.W, lambda b, p: rl.row(list(p)))
    assert_final(c["hyps"], got[0], c["log_add"], c["name"])
    dec.close()
    lm.close()


# ---- 2. the n-gram cross-check ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ctc_lmrows") / "t6_s5.arpa")
    vocab = ngram_synth.words(6, "t")
    ngram_synth.write_arpa(path, vocab, 3, (0, 30, 60), 5)
    return path, vocab


def test_equals_the_ngram_device_decode(sess, arpa):
    """LM rows computed on the host from a 3-gram (fltx_lm_start / fltx_lm_step per token, finish into finish_index):
    fltx_decode_batch on the lexicon-free decoder with that LM gives the same n-best bit for bit."""
    N, K, B, sil, blank = 6, 8, 3, 0, 1
    ng = _capi.ArpaLM(arpa[0], arpa[1], lib=sess.lib)
    hl = HostLM(ng)

    def lm_row(b, p):
        c = hl.start()
        for tok in p:
            c = hl.score(c, tok)[0]
        return np.asarray([hl.score(c, v)[1] for v in range(N)] + [hl.finish(c)[1]], np.float32)

    def case(seed):
        ems = [G.emissions(seed + b, T, N) for b, T in enumerate((5, 9, 12))]
        return ems

    for seed in range(4100, 4200):  # a seed whose three utterances have no tie in the restatement
        ems, ok = case(seed), True
        for e in ems:
            st = Stats()
            restate(e, PrefixLM(lambda p: lm_row(0, p), np.arange(N), N), K, N, 25.0, 0.7, -0.3, sil, blank, st=st)
            ok = ok and not st.ties
        if ok:
            break
    assert ok
    opts = _capi.make_options(K, N, 25.0, 0.7, sil_score=-0.3)
    ref = _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, opts, ng, sil, blank)
    ref.decode_batch(np.concatenate([e.reshape(-1) for e in ems]), [e.shape[0] for e in ems], N)
    lm = _capi.RowsLM(N + 1, None, N, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.7, -0.3, sil, blank, False)
    got, _, _ = decode(sess, dec, ems, N, N + 1, lm_row, per_state=True)
    for b in range(B):
        want = [(h.score, h.am, h.lm, h.tokens.tolist()) for h in ref.results(b)]
        assert len(want) > 1
        assert_final(want, got[b], False, b)
    for d in (dec, ref, lm, ng):
        d.close()


# ---- 3. / 4. random batches against the restatement; the row contract -------------------------------------------------
def batch(sess, base, Ts, N, K, Kt, W, perm, thr, lmw, sil_score, sil, blank, log_add, per_state=False, scale=1.0):
    """B utterances of Ts frames, each on the first clean seed from its base -> (results, stats) per utterance"""
    found = []
    for b, T in enumerate(Ts):
        def case_fn(seed, T=T):
            rl = G.SmRowsLM(seed ^ 0x5A5A, N, W, perm, W - 1, 0)
            lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
            return (G.emissions(seed, T, N) * np.float32(scale), lm, K, Kt, thr, lmw, sil_score, sil, blank, log_add)
        found.append(clean(case_fn, base + 1000 * b, log_add))
    rls = [G.SmRowsLM(seed ^ 0x5A5A, N, W, perm, W - 1, 0) for seed, _, _, _ in found]
    lm = _capi.RowsLM(W, rls[0].usr_to_lm if perm else None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, Kt, thr, lmw, sil_score, sil, blank, log_add)
    got, rows, prefix = decode(sess, dec, [inp[0] for _, inp, _, _ in found], N, W,
                               lambda b, p: rls[b].row(list(p)), per_state=per_state)
    for b, (_, _, (want, want_rows), _) in enumerate(found):
        assert_final(want, got[b], log_add, b)
        assert_rows(want_rows, rows[b], prefix[b])
    dec.close()
    lm.close()
    return [(res, st) for _, _, res, st in found]


@pytest.mark.parametrize("log_add", [False, True])
def test_small_alphabet_merges_and_reentries(sess, log_add):
    """N = 3 (blank, a, b), K = 8, T = 10 and unequal T down to 1: hypotheses merge and states are entered again"""
    out = batch(sess, 100, (10, 1, 6), 3, 8, 3, 5, 31, 25.0, 0.7, 0.0, 1, 0, log_add, scale=0.25)
    assert out[0][1].merges >= 1 and out[0][1].reentered >= 1


def test_more_candidates_than_threads(sess):
    """N = 40 = Kt, K = 8: 320 candidates, more than one pass of the step's 256 threads"""
    batch(sess, 200, (6, 3, 1), 40, 8, 40, 40, 0, 8.0, 0.7, -0.2, 3, 0, False, per_state=True)


def test_token_beam_limit(sess):
    """N = 300, Kt = 256 (the limit), K = 4, T = 3"""
    batch(sess, 300, (3, 2), 300, 4, 256, 310, 33, 25.0, 0.7, 0.0, 5, 0, False)


def test_wide_beam(sess):
    """N = 6, K = 256, T = 6: more than 128 hypotheses in the final beam"""
    out = batch(sess, 400, (6,), 6, 256, 6, 6, 0, 1e9, 0.7, 0.0, 0, 1, False, per_state=True)
    assert len(out[0][0][0]) > 128


# ---- 5. lm_row_of -------------------------------------------------------------------------------------------------------
def test_one_row_per_state_equals_one_per_hypothesis(sess):
    N, K, W, sil, blank = 4, 6, 6, 0, 1
    ems = [G.emissions(510 + b, T, N) * np.float32(0.25) for b, T in enumerate((7, 4))]
    rl = G.SmRowsLM(77, N, W, 35, W - 1, 0)
    lm = _capi.RowsLM(W, rl.usr_to_lm, W - 1, lib=sess.lib)
    res = []
    for per_state in (False, True):
        dec = make_dec(sess, lm, K, N, 25.0, 0.7, 0.0, sil, blank, False)
        res.append(decode(sess, dec, ems, N, W, lambda b, p: rl.row(list(p)), per_state=per_state))
        dec.close()
    assert res[0][1] == res[1][1]
    for a, b in zip(res[0][0], res[1][0]):
        assert_final(a, b, False)
    # an out-of-range entry: that row has no new-token candidate -- the restatement with that row's LM entries NaN
    bad = (2, 0, 1)
    dec = make_dec(sess, lm, K, N, 25.0, 0.7, 0.0, sil, blank, False)
    got, rows, prefix = decode(sess, dec, ems, N, W, lambda b, p: rl.row(list(p)), per_state=True, bad_rows=[bad])
    dec.close()
    st = Stats()
    want, want_rows = restate(ems[0], PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish), K, N, 25.0, 0.7, 0.0,
                              sil, blank, st=st, hole=(bad[0], bad[2]))
    assert not st.ties
    assert_final(want, got[0], False)
    assert_rows(want_rows, rows[0], prefix[0])
    assert want_rows != res[1][1][0] or [w[3] for w in want] != [g[3] for g in res[1][0][0]]  # (the hole changed the search)
    assert_final(res[1][0][1], got[1], False)  # ... of that utterance alone
    lm.close()


# ---- 6. typed LM rows in lockstep ---------------------------------------------------------------------------------------
def _lse_buf(sess, BK):
    if is_gpu(sess):
        import torch
        return torch.full((BK,), 7.0, dtype=torch.float64, device="cuda")
    return np.full(BK, 7.0)


class TypedFeed:
    """The step / end call of a decode on typed LM rows (dt, kind; mode "dev", "host": staged from the host, "strided":
    rows one element into a buffer of odd stride, so 2-byte rows start unaligned).  Records the float32 matrix each
    call's rows stand for -- widened, minus the lse the call reports -- and checks that lse against ref_lse."""

    def __init__(self, sess, dt, kind, mode, W):
        self.sess, self.dt, self.kind, self.mode, self.W = sess, dt, kind, mode, W
        self.mats, self.n_lse = [], 0

    def __call__(self, dec, lr, ro, end, live):
        sess, dt, kind, W = self.sess, self.dt, self.kind, self.W
        gpu, BK = is_gpu(sess), lr.shape[0]
        raw = to_dtype(lr.astype(np.float64), dt)
        w = widen(raw, dt)
        lse = _lse_buf(sess, BK) if kind else None
        kw = dict(lm_kind="logits" if kind else "log_probs", lm_lse_out=lse)
        if self.mode == "strided":
            buf = np.full((BK, W + 4), to_dtype(np.full(1, np.nan), dt)[0], dtype=raw.dtype)
            buf[:, 1:W + 1] = raw
            dbuf = _dev(sess, buf, dt)
            addr = (dbuf.data_ptr() if gpu else dbuf.ctypes.data) + (dbuf.element_size() if gpu else dbuf.itemsize)
            outs = dec._rows()
            args = (addr, dt, kind, W + 4, None, 0, 1, None if lse is None else dec._addr(lse))
            if end:
                rc = sess.lib.lib.fltx_ctc_rows_end(dec.h, *args)
            else:
                rc = sess.lib.lib.fltx_ctc_rows_step(dec.h, *args, *[dec._addr(o) for o in outs])
            assert rc == 0, sess.lib.lib.fltx_last_error()
            dec._inputs = (dbuf,)
            out = None if end else tuple(outs)
        else:
            rows_in = raw if (self.mode == "host" or not gpu) else _dev(sess, raw, dt)
            kw["lm_dtype"] = "bf16" if dt == BF16 and isinstance(rows_in, np.ndarray) else None
            out = dec.end(rows_in, **kw) if end else dec.step(rows_in, **kw)
        if kind:
            if gpu:
                sess.ctx.synchronize()
            got = _np(lse).copy()
            assert np.isnan(got[~live]).all(), got.tolist()  # (also every row of a step after the last frame)
            for i in np.nonzero(live)[0]:
                want = ref_lse(w[i])
                print("lm_row_lse", i, got[i], want)
                assert abs(got[i] - want) <= 1e-6 * max(1.0, abs(want)), (i, got[i], want)
                self.n_lse += 1
            with np.errstate(invalid="ignore"):
                w = (w.astype(np.float64) - np.where(live, got, 0.0)[:, None]).astype(np.float32)
        self.mats.append(np.ascontiguousarray(w))
        return out


@pytest.mark.parametrize("dt", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", [0, 1], ids=["log_probs", "logits"])
@pytest.mark.parametrize("mode", ["dev", "host", "strided"])
def test_typed_lm_rows_lockstep(sess, dt, kind, mode):
    """A on typed rows of odd width 7, R on the float32 matrix those rows stand for: the row lists of every frame and
    the results are bit-identical; lm_row_lse against ref_lse."""
    N, K, W, sil, blank = 5, 4, 7, 0, 1
    ems = [G.emissions(610 + b, T, N) * np.float32(0.25) for b, T in enumerate((5, 3))]
    rl = G.SmRowsLM(99, N, W, 37, W - 1, 0)
    lm = _capi.RowsLM(W, rl.usr_to_lm, W - 1, lib=sess.lib)

    def lm_row(b, p):
        return rl.row(list(p)) * np.float32(3.0 if kind else 1.0)
    feed = TypedFeed(sess, dt, kind, mode, W)
    A = make_dec(sess, lm, K, N, 25.0, 0.7, 0.0, sil, blank, False)
    a = decode(sess, A, ems, N, W, lm_row, feed=feed)
    R = make_dec(sess, lm, K, N, 25.0, 0.7, 0.0, sil, blank, False)
    seq = iter(feed.mats)

    def feed_r(dec, lr, ro, end, scored):
        lf = next(seq)
        return dec.end(_dev(sess, lf)) if end else dec.step(_dev(sess, lf))
    r = decode(sess, R, ems, N, W, lm_row, feed=feed_r)
    assert a[1] == r[1]
    for x, y in zip(a[0], r[0]):
        assert_final(x, y, False)
    assert not kind or feed.n_lse > 10
    for d in (A, R, lm):
        d.close()


# ---- 7. NaN and -inf ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmw", [0.0, 0.5])
def test_nan_and_inf_entries(sess, lmw):
    """A NaN LM entry, and 0 * -inf, are no candidates; under lm_weight 0.5 a -inf entry makes a -inf candidate, which
    the threshold removes as it removes a -inf emission; a NaN emission is never in the token beam."""
    N, K, W, sil, blank, T = 5, 6, 5, 0, 1, 5
    em = G.emissions(700, T, N) * np.float32(0.25)
    em[2, 3] = np.nan
    em[3, 2] = -np.inf
    rl = G.SmRowsLM(55, N, W, 0, W - 1, 0)

    def row(p):
        r = rl.row(list(p)).copy()
        if len(p) % 2 == 1:
            r[2] = -np.inf
        if len(p) == 2:
            r[3] = np.nan
        return r
    st = Stats()
    want, want_rows = restate(em, PrefixLM(row, rl.usr_to_lm, rl.finish), K, N, 25.0, lmw, 0.0, sil, blank, st=st)
    assert not st.ties
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, lmw, 0.0, sil, blank, False)
    got, rows, prefix = decode(sess, dec, [em], N, W, lambda b, p: row(p))
    assert_final(want, got[0], False)
    assert_rows(want_rows, rows[0], prefix[0])
    assert all(not (np.isnan(g[:3]).any()) for g in got[0])
    dec.close()
    lm.close()


# ---- 8. the state-table limit -----------------------------------------------------------------------------------------
def test_state_table_limit(sess):
    """max_states = 4: the utterance that needs more states reports "LM-state table full", the other one decodes"""
    N, K, W, sil, blank = 4, 6, 4, 0, 1
    flat = np.full((1, N), -5.0, np.float32)
    flat[0, blank] = 0.0  # utterance 1: blanks only -- the root's state and little else survives the threshold
    ems = [G.emissions(800, 6, N) * np.float32(0.25), np.repeat(flat, 6, axis=0)]
    rl = G.SmRowsLM(56, N, W, 0, W - 1, 0)
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 2.0, 0.7, 0.0, sil, blank, False)
    dec.set_max_states(4)
    Ts = [6, 6]
    dec.begin(np.concatenate([e.reshape(-1) for e in ems]), Ts, N)
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
    assert dec.results(1)[0].tokens.tolist() == [sil] + [blank] * 6 + [sil]
    dec.close()
    lm.close()


# ---- 9. contract and refusals -----------------------------------------------------------------------------------------
def test_contract_and_refusals(sess):
    import ctypes as C
    L, ctx = sess.lib, sess.ctx
    I, U, S = _capi.ERR_INVALID, _capi.ERR_UNSUPPORTED, _capi.ERR_STATE
    N, K = 6, 4
    lm = _capi.RowsLM(N + 1, None, N, lib=L)
    h = C.c_void_p()

    def create(opts, lm_, sil=0, blank=1):
        return L.lib.fltx_ctc_rows_decoder_create(ctx.h, C.byref(opts), lm_.h, sil, blank, C.byref(h))
    ok = _capi.make_options(K, N, lm_weight=0.5)
    wl = _capi.WordRowsLM(8, None, 7, lib=L)
    assert create(ok, sess.zero) == U and create(ok, wl) == U                        # any other LM, word-level rows too
    assert create(_capi.make_options(K, N, criterion="asg"), lm) == U               # ASG, for now
    assert create(_capi.make_options(257, N), lm) == U and create(_capi.make_options(256, N), lm) == 0
    L.lib.fltx_decoder_destroy(h)
    # fltx_decoder_create still refuses a rows LM; the new kind is not made there, nor by a group
    assert L.lib.fltx_decoder_create(ctx.h, _capi.LEXFREE, C.byref(ok), None, lm.h, 0, 1, -1, None, 0, 0, C.byref(h)) == U
    assert L.lib.fltx_decoder_create(ctx.h, _capi.CTC_ROWS, C.byref(ok), None, sess.zero.h, 0, 1, -1, None, 0, 0,
                                     C.byref(h)) == U
    g = C.c_void_p()
    dev0 = (C.c_int32 * 1)(-1)
    assert L.lib.fltx_group_create(dev0, 1, _capi.CTC_ROWS, C.byref(ok), None, sess.zero.h, 0, 1, -1, None, 0, 0,
                                   C.byref(g)) != 0
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    dec.B = 1  # (the row lists of one utterance)
    outs = dec._rows()
    po = [dec._addr(o) for o in outs]
    em = G.emissions(900, 3, N)
    T = np.asarray([3], np.int32)
    e_ptr, t_ptr = em.ctypes.data, T.ctypes.data
    lr = _dev(sess, np.zeros((K, N + 1), np.float32))
    pl = dec._addr(lr)
    step, end, begin = L.lib.fltx_ctc_rows_step, L.lib.fltx_ctc_rows_end, L.lib.fltx_ctc_rows_begin
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == S                  # before begin
    assert end(dec.h, pl, 0, 0, N + 1, None, 0, 1, None) == S
    assert begin(dec.h, e_ptr, 0, None, t_ptr, 1, N, po[0], po[1], None, po[3]) == I  # NULL output
    assert begin(dec.h, e_ptr, 0, None, t_ptr, 1, 65537, *po) == U                    # N
    # the limits of the token beam, and the LM's map against N
    d2 = make_dec(sess, lm, K, 300, 25.0, 0.5, 0.0, 0, 1, False)
    assert begin(d2.h, e_ptr, 0, None, t_ptr, 1, 300, *po) in (U, I)
    d2.close()
    wide = _capi.RowsLM(400, None, 399, lib=L)
    d3 = make_dec(sess, wide, K, 257, 25.0, 0.5, 0.0, 0, 1, False)
    big = np.zeros(3 * 300, np.float32)
    assert begin(d3.h, big.ctypes.data, 0, None, t_ptr, 1, 300, *po) == U            # min(Kt, N) = 257 > 256
    d3.close()
    wide.close()
    for bad_lm in (_capi.RowsLM(N + 1, None, -1, lib=L),                 # no finish index (CTC has no eos to fall back to)
                   _capi.RowsLM(0, None, N + 1, lib=L),                  # lm_width 0 = N: the finish index outside
                   _capi.RowsLM(N - 1, None, 0, lib=L),                  # identity into narrower rows
                   _capi.RowsLM(N + 1, [0, 1, 2], N, lib=L),             # a map of fewer than N entries
                   _capi.RowsLM(0, [0, 1, 2, 3, 4, 9], 0, lib=L)):       # a token's LM index outside the rows
        d4 = make_dec(sess, bad_lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
        assert begin(d4.h, e_ptr, 0, None, t_ptr, 1, N, *po) == I
        d4.close()
        bad_lm.close()
    assert begin(dec.h, e_ptr, 0, None, t_ptr, 1, N, *po) == 0
    assert step(dec.h, pl, 3, 0, N + 1, None, 0, 1, None, *po) == I                  # lm_dtype
    assert step(dec.h, pl, 0, 2, N + 1, None, 0, 1, None, *po) == I                  # lm_kind
    assert step(dec.h, pl, 0, 0, N, None, 0, 1, None, *po) == I                      # lm_row_stride < lm_width
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, po[0], None, po[2], po[3]) == I  # NULL output
    assert step(dec.h, None, 0, 0, N + 1, None, 0, 1, None, *po) == I                # NULL rows while frames are left
    assert step(dec.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == 0
    # the other entry points on this kind, and these on another kind
    assert L.lib.fltx_decode_batch(dec.h, e_ptr, 0, None, t_ptr, 1, N) == S
    assert L.lib.fltx_stream_begin(dec.h, 1, N, 10) == S and L.lib.fltx_stream_end(dec.h) == S
    assert L.lib.fltx_stream_step(dec.h, e_ptr, 0, None, t_ptr) == S and L.lib.fltx_stream_prune(dec.h, 0) == S
    assert L.lib.fltx_s2s_begin(dec.h, 1, N, *po) == S and L.lib.fltx_s2s_end(dec.h) == S
    assert L.lib.fltx_s2s_step(dec.h, pl, 1, N + 1, None, *po) == S
    assert L.lib.fltx_s2s_lex_set_max_states(dec.h, 8) == S
    other = _capi.BatchDecoder(ctx, _capi.LEXFREE, ok, sess.zero, 0, 1)
    s2s = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    for o in (other, s2s):
        assert begin(o.h, e_ptr, 0, None, t_ptr, 1, N, *po) == S
        assert step(o.h, pl, 0, 0, N + 1, None, 0, 1, None, *po) == S
        assert end(o.h, pl, 0, 0, N + 1, None, 0, 1, None) == S
        o.close()
    other = _capi.BatchDecoder(ctx, _capi.LEXFREE, ok, sess.zero, 0, 1)
    assert L.lib.fltx_decoder_set(other.h, b"max_states", 8) == I                   # the tunable is this kind's
    assert L.lib.fltx_decoder_set(dec.h, b"max_states", 0) == I
    other.close()
    assert end(dec.h, pl, 0, 0, N + 1, None, 0, 1, None) == 0                        # an early end: one frame decoded
    assert dec.count(0)[1] == 3
    dec.close()
    lm.close()
    wl.close()


# ---- 10. the Python helper ----------------------------------------------------------------------------------------------
def test_python_helper_on_a_toy_lm(sess):
    """CtcRowsBatchDecoder.decode with a callable: one LM row per state id, asked once per state; against the
    restatement."""
    N, K, W, sil, blank = 4, 6, 5, 0, 1
    found = [clean(lambda seed, T=T: (G.emissions(seed, T, N) * np.float32(0.25),
                                      PrefixLM(lambda p: G.SmRowsLM(21, N, W, 0, W - 1, 0).row(list(p)), np.arange(N),
                                               W - 1), K, N, 25.0, 0.7, 0.0, sil, blank, False), 950 + 50 * b, False)
             for b, T in enumerate((6, 2, 4))]
    rl = G.SmRowsLM(21, N, W, 0, W - 1, 0)
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.7, 0.0, sil, blank, False)
    asked = []

    def lm_rows(keys):
        asked.extend(keys)
        return _dev(sess, np.stack([rl.row(list(p)) for _, p in keys]))
    ems = [inp[0] for _, inp, _, _ in found]
    got = dec.decode(np.concatenate([e.reshape(-1) for e in ems]), [e.shape[0] for e in ems], N, lm_rows)
    assert len(set(asked)) == len(asked)  # once per state
    for b, (_, _, (want, _), _) in enumerate(found):
        assert_final(want, [(h.score, h.am, h.lm, list(h.tokens)) for h in got[b]], False, b)
    dec.close()
    lm.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_CTC_LMROWS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
