"""Seq2seq shallow fusion with a rows LM (fltx_lm_rows_create / fltx_s2s_step_lm_rows, text_amd/csrc/fltx_s2s.h).

The LM's answers arrive per step as rows next to the model's rows: row b*K + k holds the LM's score of every LM index
after the hypothesis of that row.  The checks: the compiled reference's fixtures (tests/golden/
make_s2s_lm_rows_golden.py: the restatement reproduces them, the device reproduces them -- tokens exact, the three
scores bit-identical); random batches against the float64 restatement of tests/test_seq2seq.py with a host LM whose
state is the prefix; typed LM rows (f16 / bf16 / f32, log-probs and logits) in lockstep with a decoder on the float32
LM matrix those rows stand for; the n-gram device path as a cross-check; the NaN rule; the ABI's contract and refusals.

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

CHILD = os.environ.get("FLTX_S2S_LMROWS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from golden import make_s2s_lm_rows_golden as G  # noqa: E402
from test_seq2seq import HostLM, Model, restate  # noqa: E402
from test_seq2seq_model_output import (BF16, F16, F32, NAN_BITS, Rows, _bits_equal, _GpuSess, _np, is_gpu,  # noqa: E402
                                       ref_lse, to_dtype, widen)

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


def make_dec(sess, lm, K, Kt, thr=1e9, lmw=0.0, eos_score=0.0, eos=0, maxlen=5, log_add=False):
    return _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(K, Kt, thr, lmw, eos_score, log_add), lm, eos,
                                     maxlen)


def rows_lm(sess, rl):
    """the library's LM object of a generator LM (G.SmRowsLM)"""
    ident = np.array_equal(rl.usr_to_lm, np.arange(len(rl.usr_to_lm)))
    return _capi.RowsLM(rl.W, None if ident else rl.usr_to_lm, rl.finish, lib=sess.lib)


# ---- the device loop ---------------------------------------------------------------------------------------------------
def decode(sess, dec, B, V, W, model_row, lm_row, maxlen, feed=None, pad=np.nan):
    """All utterances in one batch: model_row(b, prefix) -> V float32 (None: the model drops the row), lm_row(b, prefix)
    -> W float32.  Padding and dropped rows hold `pad` in both matrices (never read).  -> (final per utterance as
    restate's, rows per step per utterance)"""
    K = int(dec.options.beam_size)
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
                r = model_row(b, p)
                if r is None:
                    continue
                sc[b * K + k] = r
                lr[b * K + k] = lm_row(b, p)
                valid[b * K + k] = 1
        prefix = newpre
        if feed is not None:
            tok, beam, src, n = feed(dec, sc, lr, valid)
        else:
            tok, beam, src, n = dec.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, lr))
    assert dec.done()
    dec.end()
    out = []
    for b in range(B):
        hs = dec.results(b)
        out.append([(h.score, h.am, h.lm, h.tokens.tolist()) for h in hs])
        assert all((h.words == -1).all() for h in hs)
    return out, rows


def _trim(r):
    r = list(r)
    while r and r[-1] == []:
        r.pop()
    return r


def assert_same(want, got, rows):
    for b, ((wf, wr), gf, gr) in enumerate(zip(want, got, rows)):
        assert len(gf) == len(wf), (b, len(gf), len(wf))
        for i, (w, g) in enumerate(zip(wf, gf)):
            assert g[3] == w[3], (b, i, g[3], w[3])
            assert _bits_equal(g[:3], w[:3]), (b, i, g[:3], w[:3])
        assert _trim(gr) == _trim(wr), (b, _trim(gr), _trim(wr))


# ---- 1. fixtures of the reference itself ------------------------------------------------------------------------------
def _golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "seq2seq_lm_rows_expected.json.gz"), "rt") as f:
        return json.load(f)


def test_fixtures_cover_the_cases():
    cs = _golden()
    assert {c["lmw"] for c in cs} >= {0.0, 0.7, 1.2}
    assert any(c["perm"] and c["W"] > c["V"] for c in cs) and any(not c["perm"] for c in cs)
    assert any(c["finish"] >= 0 and c["finish"] != c["eos"] for c in cs)
    assert any(c["eos_score"] != 0 for c in cs) and any(c["drop"] > 0 for c in cs) and any(c["log_add"] for c in cs)
    assert max(c["K"] for c in cs) == 50 and max(c["V"] for c in cs) == 1000
    assert all(min(c["Kt"], c["V"]) <= 64 for c in cs if c["lmw"] != 0)
    assert any(c["eos"] >= c["V"] for c in cs)
    assert any(c["inf_mod"] and c["lmw"] == 0 for c in cs)


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_restatement_reproduces_reference_fixtures(c):
    """The restatement (a host LM whose state is the prefix) against the compiled reference: tokens exact, the three
    scores bit-equal."""
    ties = []
    got, _ = restate(G.case_model(c), G.PrefixLM(G.case_lm(c)), c["K"], c["Kt"], c["thr"], c["lmw"], c["eos_score"],
                     c["eos"], c["maxlen"], ties=ties)
    assert not ties
    assert len(got) == len(c["hyps"])
    for g, w in zip(got, c["hyps"]):
        assert g[3] == w[3] and _bits_equal(g[:3], w[:3]), (g, w)


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_device_reproduces_reference_fixtures(c, sess):
    """The device path against the compiled reference, with logAdd as the fixture has it and flipped (no effect)."""
    m, rl = G.case_model(c), G.case_lm(c)
    lm = rows_lm(sess, rl)
    for log_add in (c["log_add"], not c["log_add"]):
        dec = make_dec(sess, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["eos_score"], c["eos"], c["maxlen"], log_add)
        got, _ = decode(sess, dec, 1, c["V"], c["W"], lambda b, p: m.row(p), lambda b, p: rl.row(p), c["maxlen"])
        dec.close()
        assert len(got[0]) == len(c["hyps"])
        for g, w in zip(got[0], c["hyps"]):
            assert g[3] == w[3] and _bits_equal(g[:3], w[:3]), (c["name"], log_add, g, w)
    lm.close()


# ---- 2. random batches against the restatement ------------------------------------------------------------------------
def tie_free(base, mk, K, Kt, thr, lmw, eos_score, eos, maxlen, tries=50):
    """the first seed from `base` on which the restatement sees no tie: -> (seed, its result); asserts there is one"""
    for seed in range(base, base + tries):
        ties = []
        m, rl = mk(seed)
        want = restate(m, G.PrefixLM(rl), K, Kt, thr, lmw, eos_score, eos, maxlen, ties=ties)
        if not ties:
            return seed, want
    raise AssertionError("no tie-free seed in %d tries from %d" % (tries, base))


def batch_case(sess, rng, B, V, K, Kt, W, perm, finish, thr, lmw, eos_score, eos, maxlen, eos_bias, drop, pad=np.nan):
    def mk(seed):
        return (G.SmModel(seed, V, eos, eos_bias, drop), G.SmRowsLM(seed ^ 0x77, V, W, perm, finish, eos))
    found = [tie_free(int(rng.integers(1 << 30)), mk, K, Kt, thr, lmw, eos_score, eos, maxlen) for _ in range(B)]
    pairs = [mk(seed) for seed, _ in found]
    lm = rows_lm(sess, pairs[0][1])
    dec = make_dec(sess, lm, K, Kt, thr, lmw, eos_score, eos, maxlen)
    got, rows = decode(sess, dec, B, V, W, lambda b, p: pairs[b][0].row(p), lambda b, p: pairs[b][1].row(p), maxlen,
                       pad=pad)
    assert_same([w for _, w in found], got, rows)
    dec.close()
    lm.close()


def test_random_batches(sess):
    """B > 1, mixed dropped rows and padding (NaN or garbage where nothing may be read)."""
    rng = np.random.default_rng(311)
    for _ in range(8 if is_gpu(sess) else 24):
        V = int(rng.choice([5, 17, 64, 300]))
        K = int(rng.integers(1, 17))
        lmw = float(rng.choice([0.0, 0.7, 1.2]))
        Kt = int(rng.integers(1, min(V, 64) + 1)) if lmw else int(rng.integers(1, V + 5))
        W = V + int(rng.choice([0, 0, 7]))
        perm = int(rng.choice([0, 91]))
        eos = int(rng.integers(0, V + 2))
        finish = int(rng.choice([-1, W - 1]))
        batch_case(sess, rng, int(rng.integers(2, 5)), V, K, Kt, W, perm, finish, float(rng.choice([0.5, 3.0, 1e9])),
                   lmw, float(rng.choice([0.0, -0.3, 0.2])), eos, int(rng.integers(1, 6)),
                   float(rng.choice([0.0, 0.2, 0.6])), float(rng.choice([0.0, 0.15])),
                   pad=float(rng.choice([np.nan, 1e30])))


# ---- 3. typed LM rows in lockstep ---------------------------------------------------------------------------------------
def _step_raw(sess, dec, m_buf, m_off, dtm, kindm, l_buf, l_off, dtl, kindl, valid, lse_m, lse_l, W):
    """fltx_s2s_step_lm_rows on rows that start m_off / l_off elements into buffers of odd strides (2-byte types: rows
    only 2-byte aligned).  On the GPU the buffers are device tensors."""
    gpu = is_gpu(sess)
    outs = dec._rows()

    def addr(buf, off):
        base = buf.data_ptr() if gpu else buf.ctypes.data
        return base + off * (buf.element_size() if gpu else buf.itemsize)
    v = _dev(sess, valid)
    rc = sess.lib.lib.fltx_s2s_step_lm_rows(
        dec.h, addr(m_buf, m_off), dtm, kindm, m_buf.shape[1], addr(l_buf, l_off), dtl, kindl, l_buf.shape[1], 1,
        dec._addr(v), None if lse_m is None else dec._addr(lse_m), None if lse_l is None else dec._addr(lse_l),
        *[dec._addr(o) for o in outs])
    assert rc == 0, sess.lib.lib.fltx_last_error()
    dec._inputs = (m_buf, l_buf, v)
    return tuple(outs)


def _lse_buf(sess, BK):
    if is_gpu(sess):
        import torch
        return torch.full((BK,), 7.0, dtype=torch.float64, device="cuda")
    return np.full(BK, 7.0)


def lockstep(sess, lm, K, Kt, lmw, eos, maxlen, B, V, W, mrows, lrows, dtm, kindm, dtl, kindl, mode, thr=1e9):
    """A steps on typed rows (model dtm / kindm, LM dtl / kindl; mode "dev", "host" (both staged from the host) or
    "strided" (odd strides, rows one element into their buffers)); R on the same model rows and the float32 LM matrix
    A's LM rows stand for.  Row lists at every step, final tokens and the three scores are bit-identical."""
    A = make_dec(sess, lm, K, Kt, thr, lmw, 0.0, eos, maxlen)
    R = make_dec(sess, lm, K, Kt, thr, lmw, 0.0, eos, maxlen)
    BK, gpu = B * K, is_gpu(sess)
    outA, outR = A.begin(B, V), R.begin(B, V)
    prefix = {(b, 0): [] for b in range(B)}
    n_lse = 0
    for t in range(maxlen + 2):
        if gpu:
            sess.ctx.synchronize()
        ta, tr = [_np(o).copy() for o in outA], [_np(o).copy() for o in outR]
        for x, y, name in zip(ta, tr, ("token", "beam_idx", "src_row", "n_rows")):
            assert np.array_equal(x, y), (t, name, x.tolist(), y.tolist())
        tok_h, src_h, n_h = ta[0], ta[2], ta[3]
        m64, l64 = np.full((BK, V), np.nan), np.full((BK, W), np.nan)
        valid = np.zeros(BK, np.uint8)
        newpre = {}
        for b in range(B):
            for k in range(int(n_h[b])):
                p = [] if t == 0 else prefix[(b, int(src_h[b, k]) - b * K)] + [int(tok_h[b, k])]
                newpre[(b, k)] = p
                if mrows.dropped(b, p):
                    m64[b * K + k], l64[b * K + k] = 1e4, 1e4  # (never read: the row is marked dropped)
                    continue
                m64[b * K + k], l64[b * K + k] = mrows.row(b, p), lrows.row(b, p)
                valid[b * K + k] = 1
        prefix = newpre
        mraw, lraw = to_dtype(m64, dtm), to_dtype(l64, dtl)
        lw = widen(lraw, dtl)
        lse_m = _lse_buf(sess, BK) if kindm else None
        lse_l = _lse_buf(sess, BK) if kindl else None
        km, kl = ("logits" if kindm else "log_probs"), ("logits" if kindl else "log_probs")
        bf = {BF16: "bf16"}
        if mode == "strided":
            mb = np.full((BK, V + 3), NAN_BITS[dtm] if dtm != F32 else np.nan, dtype=mraw.dtype)
            lb = np.full((BK, W + 5), NAN_BITS[dtl] if dtl != F32 else np.nan, dtype=lraw.dtype)
            mb[:, 1:V + 1], lb[:, 1:W + 1] = mraw, lraw
            outA = _step_raw(sess, A, _dev(sess, mb, dtm), 1, dtm, kindm, _dev(sess, lb, dtl), 1, dtl, kindl, valid,
                             lse_m, lse_l, W)
        elif mode == "host" or not gpu:
            outA = A.step(mraw, valid, kind=km, lse_out=lse_m, dtype=bf.get(dtm), lm_scores=lraw, lm_kind=kl,
                          lm_lse_out=lse_l, lm_dtype=bf.get(dtl))
        else:
            outA = A.step(_dev(sess, mraw, dtm), _dev(sess, valid), kind=km, lse_out=lse_m,
                          lm_scores=_dev(sess, lraw, dtl), lm_kind=kl, lm_lse_out=lse_l)
        if kindl:
            if gpu:
                sess.ctx.synchronize()
            lse = _np(lse_l).copy()
            live = np.zeros(BK, bool)
            for b in range(B):
                live[b * K:b * K + int(n_h[b])] = True
            live &= valid.astype(bool)
            assert np.isnan(lse[~live]).all(), (t, lse.tolist())
            for r in np.nonzero(live)[0]:
                want = ref_lse(lw[r])
                print("lm_row_lse", t, r, lse[r], want)
                if np.isfinite(want):
                    assert abs(lse[r] - want) <= 1e-6 * max(1.0, abs(want)), (t, r, lse[r], want)
                else:
                    assert lse[r] == want, (t, r, lse[r], want)
                n_lse += 1
            with np.errstate(invalid="ignore"):
                lf = (lw.astype(np.float64) - np.where(live, lse, 0.0)[:, None]).astype(np.float32)
        else:
            lf = lw
        lf = np.ascontiguousarray(lf)
        if gpu:
            outR = R.step(_dev(sess, mraw, dtm), _dev(sess, valid), kind=km, lm_scores=_dev(sess, lf))
        else:
            outR = R.step(mraw, valid, kind=km, dtype=bf.get(dtm), lm_scores=lf)
    assert A.done() and R.done()
    A.end()
    R.end()
    res = []
    for b in range(B):
        ha, hr = A.results(b), R.results(b)
        assert len(ha) == len(hr), (b, len(ha), len(hr))
        for i, (x, y) in enumerate(zip(ha, hr)):
            assert x.tokens.tolist() == y.tokens.tolist(), (b, i)
            assert _bits_equal([x.score, x.am, x.lm], [y.score, y.am, y.lm]), (b, i, x.score, y.score)
        res.append([(h.score, h.am, h.lm, h.tokens.tolist()) for h in ha])
    A.close()
    R.close()
    return res, n_lse


MODEL_KINDS = [(F32, 0), (BF16, 1)]  # every LM dtype x kind is crossed with these two model dtype x kind


@pytest.mark.parametrize("dtm,kindm", MODEL_KINDS)
@pytest.mark.parametrize("dtl", [F32, F16, BF16])
@pytest.mark.parametrize("kindl", [0, 1])
def test_typed_lm_rows(sess, dtm, kindm, dtl, kindl):
    """Many exact ties (style "ties"), -inf and NaN entries in the LM rows; a permuted map into wider LM rows; device
    rows, host-staged rows and odd strides with 2-byte-aligned row starts."""
    B, K, Kt, V, W, eos, maxlen = 3, 5, 7, 41, 53, 4, 4
    um = np.random.default_rng(9).permutation(W)[:V].astype(np.int32)
    lm = _capi.RowsLM(W, um, 52, lib=sess.lib)
    n = 0
    for mode, lstyle in (("dev", "ties"), ("strided", "logits" if kindl else "perm"), ("host", "ties")):
        mrows = Rows(5 + kindm, V, eos, style="logits" if kindm else "perm", eos_bias=0.5, drop=0.1)
        lrows = Rows(11 + dtl, W, W + 1, style=lstyle, masked=0.1, nans=0.05)
        res, n_lse = lockstep(sess, lm, K, Kt, 0.7, eos, maxlen, B, V, W, mrows, lrows, dtm, kindm, dtl, kindl, mode)
        n += n_lse
        assert all(len(r) > 0 for r in res)
    assert (n > 0) == bool(kindl)
    lm.close()


@pytest.mark.parametrize("dtl,W", [(BF16, 16384 * 2 + 9), (F32, 16384 + 9), (F16, 16384 * 2)])
def test_typed_lm_logits_wider_than_the_registers(sess, dtl, W):
    """LM rows wider than one workgroup keeps in registers (read once per pass), and the widest that it keeps."""
    B, K, Kt, V, eos, maxlen = 1, 2, 3, 11, 4, 2
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    res, n_lse = lockstep(sess, lm, K, Kt, 1.2, eos, maxlen, B, V, W, Rows(3, V, eos, eos_bias=0.5),
                          Rows(4, W, W + 1, style="logits", nans=0.01), F32, 0, dtl, 1, "strided")
    assert n_lse > 0
    lm.close()


def test_lmw0_gathers_the_lm_field(sess):
    """lm_weight == 0: the shortcut's records (min(Kt, K + 1) tokens and eos) still get their LM entries: lm accumulates."""
    B, K, Kt, V, W, eos, maxlen = 2, 3, 20, 30, 30, 4, 4
    lm = _capi.RowsLM(lib=sess.lib)
    res, _ = lockstep(sess, lm, K, Kt, 0.0, eos, maxlen, B, V, W, Rows(21, V, eos, eos_bias=0.5), Rows(22, W, W + 1),
                      F16, 0, BF16, 1, "dev")
    assert all(h[2] != 0.0 and h[0] == h[1] for r in res for h in r)
    lm.close()


# ---- 4. the n-gram path as a cross-check --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("s2s_lmrows") / "t29_s5.arpa")
    vocab = ngram_synth.words(29, "t")
    ngram_synth.write_arpa(path, vocab, 3, (0, 400, 200), 5)
    return path, vocab


@pytest.mark.parametrize("lmw", [0.7, 0.0])
def test_equals_the_ngram_device_decode(sess, arpa, lmw):
    """V = 29: LM rows filled from the n-gram LM's host twin (HostLM.score for every token, finish into finish_index):
    the rows-LM decode equals the n-gram device decode bit for bit."""
    from test_seq2seq import run_device
    V, K, Kt, eos, maxlen, B = 29, 6, 12, 3, 5, 3
    ng = _capi.ArpaLM(arpa[0], arpa[1], lib=sess.lib)
    hl = HostLM(ng)
    models = [Model(900 + b, V, eos, 0.3) for b in range(B)]
    want, want_rows = run_device(sess, [Model(900 + b, V, eos, 0.3) for b in range(B)], ng, K, Kt, 25.0, lmw, -0.2, eos,
                                 maxlen, V)
    ctx_of = {(): hl.start()}

    def lm_row(b, p):
        c = ctx_of[()]
        for tok in p:  # (the n-gram context after the prefix)
            c = hl.score(c, tok)[0]
        r = np.zeros(V + 1, np.float32)
        for v in range(V):
            r[v] = hl.score(c, v)[1]
        r[V] = hl.finish(c)[1]
        return r
    lm = _capi.RowsLM(V + 1, None, V, lib=sess.lib)
    dec = make_dec(sess, lm, K, Kt, 25.0, lmw, -0.2, eos, maxlen)
    got, rows = decode(sess, dec, B, V, V + 1, lambda b, p: models[b].row(p), lm_row, maxlen)
    for b in range(B):
        assert len(got[b]) == len(want[b])
        for g, w in zip(got[b], want[b]):
            assert g[3] == w[3] and _bits_equal(g[:3], w[:3]), (b, g, w)
        assert _trim(rows[b]) == _trim(want_rows[b])
    dec.close()
    lm.close()
    ng.close()


# ---- 5. the NaN rule ----------------------------------------------------------------------------------------------------
def test_nan_candidates_are_absent(sess):
    """lm_weight == 0 and a -inf LM entry inside the token beam: 0 * -inf is NaN, the candidate is absent (the
    reference's candidatesAdd compares with >=); a NaN LM entry likewise; under lm_weight 0.5 the -inf entry makes a
    -inf candidate, which the threshold removes as it removes a -inf model entry."""
    K, V, eos = 4, 4, 9
    sc = np.full((K, V), np.nan, np.float32)
    sc[0] = [-1.0, -2.0, -3.0, -4.0]
    lr = np.zeros((K, V), np.float32)
    lr[0] = [-0.5, -np.inf, np.nan, -0.25]
    lm = _capi.RowsLM(lib=sess.lib)
    for lmw, want in ((0.0, [(0, -1.0, -0.5), (3, -4.0, -0.25)]),
                      (0.5, [(0, -1.25, -0.5), (3, -4.125, -0.25)])):
        dec = make_dec(sess, lm, K, V, 1e9, lmw, 0.0, eos, 1)
        dec.begin(1, V)
        tok, beam, src, n = dec.step(_dev(sess, sc), lm_scores=_dev(sess, lr))
        dec.end()
        got = [(int(h.tokens[-1]), h.score, h.lm) for h in dec.results(0)]
        assert got == want, (lmw, got)
        assert [h.am for h in dec.results(0)] == [float(sc[0, t]) for t, _, _ in want]
        dec.close()
    lm.close()


# ---- 6. the step's contract -------------------------------------------------------------------------------------------
def test_step_after_done_max_length_and_restart(sess):
    """A step after the last one lists no rows and changes no result (and writes NaN lse); maxOutputLength 0 is the
    root alone; a decoder that begins again restarts from the root."""
    K, V, W, eos, maxlen = 3, 12, 15, 3, 3
    m, rl = G.SmModel(31, V, eos, 0.5), G.SmRowsLM(32, V, W, 93, -1, eos)
    want, _ = restate(m, G.PrefixLM(rl), K, 6, 1e9, 0.7, 0.0, eos, maxlen)
    lm = rows_lm(sess, rl)
    dec = make_dec(sess, lm, K, 6, 1e9, 0.7, 0.0, eos, maxlen)
    for _ in range(2):
        got, _ = decode(sess, dec, 1, V, W, lambda b, p: m.row(p), lambda b, p: rl.row(p), maxlen)
        assert [g[3] for g in got[0]] == [w[3] for w in want]
        assert all(_bits_equal(g[:3], w[:3]) for g, w in zip(got[0], want))
    lse = _lse_buf(sess, K)
    out = dec.step(_dev(sess, np.zeros((K, V), np.float32)), lm_scores=_dev(sess, np.zeros((K, W), np.float32)),
                   lm_kind="logits", lm_lse_out=lse)
    if is_gpu(sess):
        sess.ctx.synchronize()
    assert _np(out[3]).tolist() == [0] and (_np(out[0]) == -1).all() and np.isnan(_np(lse)).all()
    outs = dec._rows()  # (NULL rows after the last step are accepted: nothing is read)
    assert sess.lib.lib.fltx_s2s_step_lm_rows(dec.h, None, 0, 0, V, None, 0, 0, W, 1, None, None, None,
                                              *[dec._addr(o) for o in outs]) == 0
    dec.end()
    assert [h.tokens.tolist() for h in dec.results(0)] == [w[3] for w in want]
    dec.close()
    dec = make_dec(sess, lm, K, 6, 1e9, 0.7, 0.0, eos, 0)
    tok, beam, src, n = dec.begin(1, V)
    assert _np(n).tolist() == [0] and dec.done()
    dec.end()
    h = dec.results(0)
    assert len(h) == 1 and h[0].tokens.tolist() == [-1, -1, -1] and h[0].score == 0.0 and h[0].lm == 0.0
    dec.close()
    lm.close()


def test_host_staged_rows(sess):
    """Host rows (numpy on the HIP library: on_device == 0) of both matrices are staged in their own type."""
    K, V, W, eos, maxlen = 4, 20, 20, 2, 4
    m, rl = G.SmModel(41, V, eos, 0.3), G.SmRowsLM(42, V, W, 0, -1, eos)
    want = restate(m, G.PrefixLM(rl), K, 8, 1e9, 1.2, 0.0, eos, maxlen)
    lm = rows_lm(sess, rl)
    dec = make_dec(sess, lm, K, 8, 1e9, 1.2, 0.0, eos, maxlen)
    got, rows = decode(sess, dec, 1, V, W, lambda b, p: m.row(p), lambda b, p: rl.row(p), maxlen,
                       feed=lambda d, sc, lr, valid: d.step(sc, valid, lm_scores=lr))
    assert_same([want], got, rows)
    dec.close()
    lm.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(sess):
    L, ctx = sess.lib, sess.ctx
    U, I, S = _capi.ERR_UNSUPPORTED, _capi.ERR_INVALID, _capi.ERR_STATE
    h = C.c_void_p()
    i32 = np.int32

    def create(width, um, finish):
        a = None if um is None else np.asarray(um, i32)
        return L.lib.fltx_lm_rows_create(width, None if a is None else a.ctypes.data, 0 if a is None else len(a), finish,
                                         C.byref(h))
    # fltx_lm_rows_create: a map entry outside [0, lm_width), a finish index outside it, null out
    assert create(4, [0, 1, 4], -1) == I and create(4, [0, -1], -1) == I and create(4, None, 4) == I
    assert create(-1, None, -1) == I and L.lib.fltx_lm_rows_create(0, None, 0, -1, None) == I
    assert create(65537, None, -1) == U
    lm = _capi.RowsLM(lib=L)
    # the LM state functions and the other decoders
    with pytest.raises(_capi.FltxError) as e:
        lm.score_sequence([1, 2])
    assert e.value.code == U
    for f in (lm.state_size, lm.start, lambda: lm.step(np.zeros(1, i32), 1)):
        with pytest.raises(_capi.FltxError) as e:
            f()
        assert e.value.code == U
    for kind in (_capi.LEXFREE,):
        with pytest.raises(_capi.FltxError) as e:
            _capi.BatchDecoder(ctx, kind, _capi.make_options(4, 4), lm, 0, 1)
        assert e.value.code == U
        with pytest.raises(_capi.FltxError) as e:
            _capi.DecoderGroup([0], kind, _capi.make_options(4, 4), lm, 0, 1, lib=L)
        assert e.value.code == U
    from test_lexicon_seq2seq import host_trie, make_lexicon
    trie = host_trie(L, 6, make_lexicon(6, 1, 5, 1), 1)
    with pytest.raises(_capi.FltxError) as e:
        _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(4, 4), trie, lm, 1, 5)
    assert e.value.code == U and "rows LM" in str(e.value)
    # fltx_s2s_begin: V beyond the map; a finish index (usr_to_lm[eos] / eos itself) or a token outside the rows
    outs = [np.zeros(8, i32) for _ in range(3)] + [np.zeros(2, i32)]
    if is_gpu(sess):
        import torch
        outs = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in range(3)] + \
            [torch.zeros(2, dtype=torch.int32, device="cuda")]
    po = [o.ctypes.data if isinstance(o, np.ndarray) else o.data_ptr() for o in outs]

    def begin(lmx, V, eos=1, lmw=0.5, Kt=4):
        d = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(4, Kt, lm_weight=lmw), lmx, eos, 5)
        rc = L.lib.fltx_s2s_begin(d.h, 1, V, *po)
        d.close()
        return rc
    assert begin(_capi.RowsLM(0, [0, 1, 2], -1, lib=L), 4) == I          # V > n_usr
    assert begin(_capi.RowsLM(0, [0, 1, 2, 3], -1, lib=L), 4) == 0
    assert begin(_capi.RowsLM(0, [0, 1, 2, 7], -1, lib=L), 4) == I       # lm_width 0 (= V) and a map that leaves it
    assert begin(_capi.RowsLM(0, None, 5, lib=L), 4) == I                # ... and a finish index that does
    assert begin(_capi.RowsLM(3, None, -1, lib=L), 4) == I               # identity into narrower rows
    assert begin(_capi.RowsLM(6, None, 5, lib=L), 4) == 0
    assert begin(_capi.RowsLM(0, None, -1, lib=L), 4, eos=9) == 0        # eos >= V: finish is never read
    assert begin(lm, 100, Kt=65) == U and begin(lm, 100, Kt=64) == 0     # kS2sMaxKtLm with LM terms
    assert begin(lm, 100, Kt=65, lmw=0.0) == 0
    # the step entry points
    K, V = 4, 6
    dr = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4, lm_weight=0.5), lm, 1, 5)
    dz = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    sc, lr = _dev(sess, np.zeros((K, V), np.float32)), _dev(sess, np.zeros((K, V), np.float32))
    ps, pl = dr._addr(sc), dr._addr(lr)
    step = L.lib.fltx_s2s_step_lm_rows
    assert step(dr.h, ps, 0, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == S  # before fltx_s2s_begin
    dr.begin(1, V)
    dz.begin(1, V)
    assert L.lib.fltx_s2s_step(dr.h, ps, 1, V, None, *po) == S
    assert L.lib.fltx_s2s_step_typed(dr.h, ps, 0, 1, 1, V, None, None, *po) == S
    assert step(dz.h, ps, 0, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == S
    bd = _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(4, 4), trie, sess.zero, 1, 5)
    assert step(bd.h, ps, 0, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == S
    bd.close()
    assert step(dr.h, ps, 0, 0, V, pl, 3, 0, V, 1, None, None, None, *po) == I      # lm_dtype
    assert step(dr.h, ps, 0, 0, V, pl, 0, 2, V, 1, None, None, None, *po) == I      # lm_kind
    assert step(dr.h, ps, 3, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == I      # dtype
    assert step(dr.h, ps, 0, 0, V, pl, 0, 0, V - 1, 1, None, None, None, *po) == I  # lm_row_stride < lm_width
    assert step(dr.h, ps, 0, 0, V - 1, pl, 0, 0, V, 1, None, None, None, *po) == I  # row_stride < V
    assert step(dr.h, ps, 0, 0, V, None, 0, 0, V, 1, None, None, None, *po) == I    # NULL lm_scores before the last step
    assert step(dr.h, ps, 0, 0, V, pl, 0, 0, V, 1, None, None, None, *po) == 0
    # Python: lm_scores with a decoder without a RowsLM, and a RowsLM decoder without them
    with pytest.raises(_capi.FltxError) as e:
        dz.step(sc, lm_scores=lr)
    assert e.value.code == S
    with pytest.raises(_capi.FltxError) as e:
        dr.step(sc)
    assert e.value.code == S
    dr.close()
    dz.close()
    lm.close()


# ---- 8. GPU only --------------------------------------------------------------------------------------------------------
def _large_batch(gpu_sess):
    """B = 256, K = 50, V = 1000 (token beam 50, a permuted map into LM rows of 1 100) against the restatement."""
    rng = np.random.default_rng(77)
    batch_case(gpu_sess, rng, 256, 1000, 50, 50, 1100, 95, 1099, 25.0, 0.7, -0.1, 11, 3, 0.05, 0.02, pad=1e30)


def _torch_bf16_loop(gpu_sess):
    """A torch loop whose model and LM both emit bf16 logits on the device, their states gathered by next_src_row, in
    lockstep with a float32 decoder fed the rows they stand for (widened, minus the lse the step reports)."""
    import torch
    B, K, Kt, V, W, eos, maxlen = 16, 8, 12, 500, 640, 3, 8
    g = np.random.default_rng(6)
    E = torch.from_numpy(g.standard_normal((V + 1, V)).astype(np.float32)).cuda()
    F = torch.from_numpy(g.standard_normal((V + 1, W)).astype(np.float32)).cuda()
    E[:, eos] -= 1.5
    um = g.permutation(W)[:V].astype(np.int32)
    lm = _capi.RowsLM(W, um, W - 1, lib=gpu_sess.lib)
    A = make_dec(gpu_sess, lm, K, Kt, 6.0, 0.6, 0.0, eos, maxlen)
    R = make_dec(gpu_sess, lm, K, Kt, 6.0, 0.6, 0.0, eos, maxlen)
    h = torch.from_numpy(np.repeat(g.standard_normal((B, V)).astype(np.float32), K, axis=0)).cuda()
    s = torch.zeros((B * K, W), device="cuda")
    outA, outR = A.begin(B, V), R.begin(B, V)
    for t in range(maxlen + 1):
        gpu_sess.ctx.synchronize()
        for x, y in zip(outA, outR):
            assert torch.equal(x, y), t
        tok, src = outA[0].reshape(-1), outA[2].reshape(-1)
        if t > 0:
            h, s = h.index_select(0, src.clamp(min=0).long()), s.index_select(0, src.clamp(min=0).long())
        ti = torch.where(tok >= 0, tok, torch.full_like(tok, V)).long()
        h = h * 0.5 + E.index_select(0, ti)
        s = s * 0.25 + F.index_select(0, ti)
        mb, lb = h.to(torch.bfloat16), (s * 2.0).to(torch.bfloat16)
        lse_m = torch.zeros(B * K, dtype=torch.float64, device="cuda")
        lse_l = torch.zeros(B * K, dtype=torch.float64, device="cuda")
        outA = A.step(mb, kind="logits", lse_out=lse_m, lm_scores=lb, lm_kind="logits", lm_lse_out=lse_l)
        mf = (mb.double() - lse_m[:, None]).float()
        lf = (lb.double() - lse_l[:, None]).float()
        outR = R.step(mf, lm_scores=lf)
    assert A.done() and R.done()
    A.end()
    R.end()
    n = 0
    for b in range(B):
        for x, y in zip(A.results(b), R.results(b)):
            assert x.tokens.tolist() == y.tokens.tolist() and _bits_equal([x.score, x.am, x.lm], [y.score, y.am, y.lm])
            n += 1
    assert n >= B
    A.close()
    R.close()
    lm.close()


def _compat_three_element_update_func(gpu_sess):
    """The compat LexiconFreeSeq2SeqDecoder (B = 1) with a RowsLM: update_func returns (scores, states, lm_scores);
    against a reference fixture.  Any other user-defined LM is still refused."""
    compat = os.path.join(ROOT, "text_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    from flashlight.lib.text.decoder import (LexiconFreeSeq2SeqDecoder, LexiconFreeSeq2SeqDecoderOptions,
                                             create_emitting_model_state, get_obj_from_emitting_model_state)
    c = next(c for c in _golden() if c["name"] == "perm_wide")
    m, rl = G.case_model(c), G.case_lm(c)

    def update(emissions, N, T, raw_y, raw_beam, prev_states, t):
        scores, states, lms = [], [], []
        for y, st in zip(raw_y, prev_states):
            p = [] if t == 0 else get_obj_from_emitting_model_state(st) + [y]
            r = m.row(p)
            scores.append((r if r is not None else np.zeros(c["V"], np.float32)).tolist())
            states.append(create_emitting_model_state(p) if r is not None else None)
            lms.append(rl.row(p).tolist())
        return scores, states, lms
    opts = LexiconFreeSeq2SeqDecoderOptions(c["K"], c["Kt"], c["thr"], c["lmw"], c["eos_score"], c["log_add"])
    dec = LexiconFreeSeq2SeqDecoder(opts, rows_lm(gpu_sess, rl), c["eos"], update, c["maxlen"])
    dec.decode_step(0, 1, c["V"])
    got = dec.get_all_final_hypothesis()
    assert len(got) == len(c["hyps"])
    for g, w in zip(got, c["hyps"]):
        assert g.tokens == w[3] and _bits_equal([g.score, g.emittingModelScore, g.lmScore], w[:3])

    class UserLM:
        pass
    with pytest.raises(_capi.FltxError) as e:
        LexiconFreeSeq2SeqDecoder(opts, UserLM(), c["eos"], update, c["maxlen"])
    assert e.value.code == _capi.ERR_UNSUPPORTED and "would need merges" in str(e.value)


if CHILD:  # (GPU-only cases: defined in the child alone)
    test_large_batch = pytest.mark.gpu(_large_batch)
    test_torch_bf16_loop = pytest.mark.gpu(_torch_bf16_loop)
    test_compat_three_element_update_func = pytest.mark.gpu(_compat_three_element_update_func)


@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_S2S_LMROWS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
