"""fltx_s2s_step_typed: the seq2seq step on the model's output as the model produces it (text_amd/csrc/fltx_s2s.h,
s2sTypedRows) -- float32 / float16 / bfloat16 rows holding log-probabilities or raw logits.

Every check runs two decoders in lockstep on the same rows: A steps on the typed rows, R steps with fltx_s2s_step on
the float32 matrix those rows stand for -- the exact widening for log-probs, and np.float32(np.float64(x) - lse) built
from the lse A reports for logits.  The row lists of every step, the final tokens (and words) and the three scores
must be identical, bit for bit.  Each reported lse must be within 1e-6 * max(1, |ref|) of a float64 log-sum-exp of the
widened row.

Every test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a child process that
initialises torch first (as tests/test_seq2seq.py does).
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

CHILD = os.environ.get("FLTX_S2S_MO_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from test_lexicon_seq2seq import host_trie, make_lexicon  # noqa: E402
from test_seq2seq import HostLM, Model, restate  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
F32, F16, BF16 = _capi.DTYPE_F32, _capi.DTYPE_F16, _capi.DTYPE_BF16
NAN_BITS = {F32: np.uint32(0x7FC00000), F16: np.uint16(0x7E00), BF16: np.uint16(0x7FC0)}


class _GpuSess:
    def __init__(self, gpu_session):
        import torch
        self.lib = gpu_session.lib
        self.stream = torch.cuda.Stream()
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


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


# ---- element types ----------------------------------------------------------------------------------------------------
def to_dtype(x64, dt):
    """float64 values -> the raw array of type dt (float32 / float16 / uint16 bfloat16 bits, round to nearest even)"""
    if dt == F32:
        return x64.astype(np.float32)
    if dt == F16:
        return x64.astype(np.float16)
    f = x64.astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    b[np.isnan(f)] = NAN_BITS[BF16]
    return b


def widen(raw, dt):
    if dt == BF16:
        return (raw.astype(np.uint32) << 16).view(np.float32)
    return raw.astype(np.float32)


def ref_lse(w):
    """float64 log-sum-exp of a widened row over its non-NaN entries (max when that is not finite)"""
    x = w.astype(np.float64)
    x = x[~np.isnan(x)]
    if x.size == 0:
        return -np.inf
    m = x.max()
    if not np.isfinite(m):
        return m
    return m + np.log(np.exp(x - m).sum())


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---- the lockstep driver ----------------------------------------------------------------------------------------------
class Rows:
    """row(b, prefix) -> V float64 model values; a pure function of (seed, b, prefix).  style: "perm" (distinct
    values), "ties" (a few levels: many exact ties, bf16's normal case), "logits" (wide logits with near-duplicates)."""

    def __init__(self, seed, V, eos, style="perm", eos_bias=0.0, drop=0.0, masked=0.0, nans=0.0):
        self.seed, self.V, self.eos, self.style = seed, V, eos, style
        self.eos_bias, self.drop, self.masked, self.nans = eos_bias, drop, masked, nans

    def _rng(self, b, prefix):
        h = hashlib.blake2b(np.asarray([self.seed, b] + list(prefix), dtype=np.int64).tobytes(),
                            digest_size=8).digest()
        return np.random.default_rng(int.from_bytes(h, "little"))

    def dropped(self, b, prefix):
        return self.drop > 0 and len(prefix) > 0 and self._rng(b, prefix + [-7]).random() < self.drop

    def row(self, b, prefix):
        g = self._rng(b, prefix)
        V = self.V
        if self.style == "perm":
            x = -(g.permutation(V).astype(np.float64) * 2.0 ** -6) - g.random()
        elif self.style == "ties":
            x = -np.floor(g.exponential(2.0, V) * 4) / 4 - 0.25
        else:
            x = g.standard_normal(V) * 3.0
            dup = g.integers(0, V, max(1, V // 4))
            x[dup] = x[(dup + 1) % V] + g.standard_normal(dup.size) * 1e-4
        if self.eos < V and self.eos_bias:
            x[self.eos] += self.eos_bias
        if self.masked:
            x[g.random(V) < self.masked] = -np.inf
        if self.nans:
            x[g.random(V) < self.nans] = np.nan
        return x


def _feed(sess, dec, raw, dt, kind, valid, mode, lse_out):
    """one typed step of A: raw [BK, V] of dt; mode "dev" (device rows), "host" (host rows, staged), "strided"
    (device rows at an odd element stride, starting one element into a buffer: 2-byte types only 2-byte aligned)"""
    BK, V = raw.shape
    kname = "logits" if kind else "log_probs"
    gpu = is_gpu(sess)
    if mode == "strided":
        W = V + 3
        buf = np.full((BK, W), NAN_BITS[dt] if dt != F32 else np.nan, dtype=raw.dtype)
        buf[:, 1:V + 1] = raw
        if gpu:
            import torch
            tb = torch.from_numpy(buf.view(np.int16) if dt == BF16 else buf).cuda()
            if dt == BF16:
                tb = tb.view(torch.bfloat16)
            out = dec.step(tb[:, 1:V + 1], torch.from_numpy(valid).cuda(), kind=kname, lse_out=lse_out)
            dec._inputs = (tb, dec._inputs)
            return out
        outs = dec._rows()
        ptr = buf.ctypes.data + buf.itemsize
        rc = sess.lib.lib.fltx_s2s_step_typed(dec.h, ptr, dt, kind, 1, W, valid.ctypes.data,
                                              None if lse_out is None else lse_out.ctypes.data,
                                              *[o.ctypes.data for o in outs])
        assert rc == 0, sess.lib.last_error() if hasattr(sess.lib, "last_error") else rc
        dec._inputs = (buf, valid)
        return tuple(outs)
    if gpu and mode == "dev":
        import torch
        t = torch.from_numpy(raw.view(np.int16) if dt == BF16 else raw).cuda()
        if dt == BF16:
            t = t.view(torch.bfloat16)
        return dec.step(t, torch.from_numpy(valid).cuda(), kind=kname, lse_out=lse_out)
    return dec.step(raw, valid, kind=kname, lse_out=lse_out, dtype="bf16" if dt == BF16 else None)


def lockstep(sess, make_dec, rows, B, V, maxlen, plan, lex=False):
    """A on the typed rows plan(t) = (dtype, kind, mode), R on the float32 matrix they stand for.  -> A's results."""
    A, R = make_dec(), make_dec()
    K = int(A.options.beam_size)
    BK = B * K
    gpu = is_gpu(sess)
    outA, outR = A.begin(B, V), R.begin(B, V)
    prefix = {(b, 0): [] for b in range(B)}
    n_lse = 0
    for t in range(maxlen + 2):  # (a step after the last one is a no-op: its rows are none)
        if gpu:
            sess.ctx.synchronize()
        ta, tr = [_np(o).copy() for o in outA], [_np(o).copy() for o in outR]
        for x, y, name in zip(ta, tr, ("token", "beam_idx", "src_row", "n_rows")):
            assert np.array_equal(x, y), (t, name, x.tolist(), y.tolist())
        tok_h, src_h, n_h = ta[0], ta[2], ta[3]
        dt, kind, mode = plan(t)
        x64 = np.full((BK, V), np.nan)
        valid = np.zeros(BK, np.uint8)
        newpre = {}
        for b in range(B):
            for k in range(int(n_h[b])):
                p = [] if t == 0 else prefix[(b, int(src_h[b, k]) - b * K)] + [int(tok_h[b, k])]
                newpre[(b, k)] = p
                if rows.dropped(b, p):
                    x64[b * K + k] = 1e4  # (never read: the row is marked dropped)
                    continue
                x64[b * K + k] = rows.row(b, p)
                valid[b * K + k] = 1
        prefix = newpre
        raw = to_dtype(x64, dt)
        w = widen(raw, dt)
        lse = None
        if kind:
            if gpu:
                import torch
                lse_out = torch.full((BK,), 7.0, dtype=torch.float64, device="cuda")
            else:
                lse_out = np.full(BK, 7.0)
        else:
            lse_out = None
        outA = _feed(sess, A, raw, dt, kind, valid, mode, lse_out)
        if kind:
            if gpu:
                sess.ctx.synchronize()
            lse = _np(lse_out).copy()
            live = np.zeros(BK, bool)
            for b in range(B):
                live[b * K:b * K + int(n_h[b])] = True
            live &= valid.astype(bool)
            assert np.isnan(lse[~live]).all(), (t, lse.tolist())
            for r in np.nonzero(live)[0]:
                want = ref_lse(w[r])
                if np.isfinite(want):
                    assert abs(lse[r] - want) <= 1e-6 * max(1.0, abs(want)), (t, r, lse[r], want)
                else:
                    assert lse[r] == want, (t, r, lse[r], want)
                n_lse += 1
            with np.errstate(invalid="ignore"):
                f = (w.astype(np.float64) - np.where(live, lse, 0.0)[:, None]).astype(np.float32)
        else:
            f = w
        if gpu:
            import torch
            outR = R.step(torch.from_numpy(np.ascontiguousarray(f)).cuda(), torch.from_numpy(valid).cuda())
        else:
            outR = R.step(np.ascontiguousarray(f), valid)
    assert A.done() and R.done()
    A.end()
    R.end()
    res = []
    for b in range(B):
        ha, hr = A.results(b), R.results(b)
        assert len(ha) == len(hr), (b, len(ha), len(hr))
        for i, (x, y) in enumerate(zip(ha, hr)):
            assert x.tokens.tolist() == y.tokens.tolist(), (b, i)
            assert x.words.tolist() == y.words.tolist(), (b, i)
            assert _bits_equal([x.score, x.am, x.lm], [y.score, y.am, y.lm]), (b, i, x.score, y.score)
        res.append([(h.score, h.am, h.lm, h.tokens.tolist()) for h in ha])
    A.close()
    R.close()
    return res, n_lse


def lexfree(sess, K, Kt, thr=1e9, lmw=0.0, eos_score=0.0, eos=0, maxlen=5, lm=None):
    opts = _capi.make_s2s_options(K, Kt, thr, lmw, eos_score)
    return lambda: _capi.Seq2SeqBatchDecoder(sess.ctx, opts, lm if lm is not None else sess.zero, eos, maxlen)


def lexicon(sess, trie, K, Kt, thr=1e9, lmw=0.0, word_score=0.0, eos=0, maxlen=5, lm=None):
    opts = _capi.make_s2s_lex_options(K, Kt, thr, lmw, word_score)
    return lambda: _capi.LexiconSeq2SeqBatchDecoder(sess.ctx, opts, trie, lm if lm is not None else sess.zero, eos,
                                                    maxlen)


def const_plan(dt, kind, mode="dev"):
    return lambda t: (dt, kind, mode)


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    def make(V, seed=5):
        path = str(tmp_path_factory.mktemp("s2s_mo_lm") / ("t%d_s%d.arpa" % (V, seed)))
        vocab = ngram_synth.words(V, "t")
        ngram_synth.write_arpa(path, vocab, 3, (0, 400, 200), seed)
        return path, vocab
    return make


# ---- 1. exact widening -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("style,V,K,Kt,mode", [("perm", 37, 4, 6, "dev"),       # the shortcut (min(Kt, K + 1) + eos)
                                               ("perm", 37, 4, 37, "strided"),  # Kt = V
                                               ("ties", 300, 5, 50, "host"),    # many exact ties at the cuts
                                               ("ties", 29, 3, 40, "strided")])
def test_widened_log_probs_lexicon_free(sess, dt, style, V, K, Kt, mode):
    rows = Rows(3 + V, V, eos=2, style=style, eos_bias=0.5, drop=0.15)
    lockstep(sess, lexfree(sess, K, Kt, eos=2), rows, 3, V, 5, const_plan(dt, 0, mode))


@pytest.mark.parametrize("dt", [F16, BF16])
def test_widened_log_probs_ngram(sess, arpa, dt):
    path, vocab = arpa(29)
    lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
    rows = Rows(21, 29, eos=5, style="ties", eos_bias=0.3, drop=0.1)
    lockstep(sess, lexfree(sess, 6, 10, lmw=0.7, eos_score=-0.5, eos=5, maxlen=6, lm=lm), rows, 2, 29, 6,
             const_plan(dt, 0, "strided"))


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("mode", ["dev", "strided"])
def test_widened_log_probs_lexicon(sess, dt, mode):
    V, eos = 24, 0
    trie = host_trie(sess.lib, V, make_lexicon(V, eos, 60, 8), 1)
    rows = Rows(31, V, eos=eos, style="ties", eos_bias=-1.0, drop=0.1)
    lockstep(sess, lexicon(sess, trie, 5, 8, eos=eos, word_score=0.25), rows, 2, V, 5, const_plan(dt, 0, mode))
    trie.close()


def test_widening_special_values(sess):
    """fp16 subnormals, infinities, signed zeros and NaN payloads widen exactly (the f32 step on np.float32 of them)."""
    V = 64
    specials = np.array([0x0001, 0x03FF, 0x0200, 0x8001, 0x83FF, 0x7C00, 0xFC00, 0x0000, 0x8000, 0x7E01, 0xFC01,
                         0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x0400], np.uint16)

    class Special(Rows):
        def row(self, b, prefix):
            g = self._rng(b, prefix)
            bits = specials[g.integers(0, specials.size, V)]
            return bits.view(np.float16).astype(np.float64)

    lockstep(sess, lexfree(sess, 4, 8, eos=3), Special(5, V, 3), 2, V, 4, const_plan(F16, 0, "dev"))


# ---- 2. logits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F16, BF16])
@pytest.mark.parametrize("V,K,Kt,mode", [(53, 4, 7, "dev"), (53, 4, 53, "strided"), (400, 6, 50, "host")])
def test_logits_lexicon_free(sess, dt, V, K, Kt, mode):
    rows = Rows(40 + V, V, eos=7, style="logits", eos_bias=1.0, drop=0.1, masked=0.1, nans=0.02)
    _, n = lockstep(sess, lexfree(sess, K, Kt, eos=7), rows, 3, V, 5, const_plan(dt, 1, mode))
    assert n > 0


@pytest.mark.parametrize("dt", [F32, BF16])
def test_logits_lexicon_and_ngram(sess, arpa, dt):
    V, eos = 24, 0
    trie = host_trie(sess.lib, V, make_lexicon(V, eos, 60, 9), 1)
    rows = Rows(32, V, eos=eos, style="logits", eos_bias=-2.0, masked=0.1)
    lockstep(sess, lexicon(sess, trie, 5, 8, eos=eos), rows, 2, V, 5, const_plan(dt, 1, "strided"))
    trie.close()
    path, vocab = arpa(29)
    lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
    rows = Rows(33, 29, eos=5, style="logits", eos_bias=0.5)
    lockstep(sess, lexfree(sess, 6, 10, lmw=0.7, eos=5, maxlen=6, lm=lm), rows, 2, 29, 6, const_plan(dt, 1, "dev"))


def test_logits_rounding_ties_at_the_cut(sess):
    """Distinct logits that round to one log-prob at the token-beam cut: the lower token wins, as in the f32 path."""
    V, Kt = 40, 5

    class Near(Rows):
        def row(self, b, prefix):
            g = self._rng(b, prefix)
            x = -3.0 - g.random(V) * 4.0
            base = np.float32(-1.0)
            ulp = float(np.spacing(base))
            # tokens 30, 12, 25, 3, 18, 7 all within a fraction of an ulp of -1: one float after subtracting lse
            for j, tk in enumerate([30, 12, 25, 3, 18, 7]):
                x[tk] = float(base) + (j - 2.5) * ulp * 1e-3
            x[1] = 0.5
            return x

    rows = Near(9, V, eos=39)
    res, _ = lockstep(sess, lexfree(sess, 6, Kt, eos=39, maxlen=2), rows, 1, V, 2, const_plan(F32, 1, "dev"))
    first = sorted({h[3][-2] for h in res[0]} | {h[3][-1] for h in res[0]})
    assert 1 in first and 3 in first and 30 not in first


def test_logits_masked_and_degenerate_rows(sess):
    """-inf-masked entries, an all -inf row (proposes nothing), NaN entries, a +inf entry, V = 1."""
    V = 12

    class Odd(Rows):
        def row(self, b, prefix):
            g = self._rng(b, prefix)
            x = g.standard_normal(V)
            x[g.random(V) < 0.4] = -np.inf
            x[g.random(V) < 0.1] = np.nan
            if b == 1:
                x[:] = -np.inf
            if b == 2 and len(prefix) == 1:
                x[4] = np.inf
            return x

    for dt in (F32, F16, BF16):
        lockstep(sess, lexfree(sess, 3, 5, eos=0, maxlen=3), Odd(2, V, 0), 3, V, 3, const_plan(dt, 1, "dev"))
    for dt in (F32, BF16):
        lockstep(sess, lexfree(sess, 2, 3, eos=0, maxlen=3), Rows(3, 1, 0, "logits"), 2, 1, 3,
                 const_plan(dt, 1, "dev"))
        lockstep(sess, lexfree(sess, 2, 3, eos=0, maxlen=3), Rows(3, 1, 0, "logits"), 2, 1, 3,
                 const_plan(dt, 0, "host"))


@pytest.mark.parametrize("V", [16384, 16385])
def test_read_once_boundary(sess, V):
    """The last width kept in registers and the first one re-read, logits and log-probs."""
    rows = Rows(V, V, eos=V - 3, style="logits", masked=0.01)
    lockstep(sess, lexfree(sess, 2, 3, eos=V - 3, maxlen=2), rows, 1, V, 2,
             lambda t: [(BF16, 1, "dev"), (F16, 0, "strided")][t % 2])


def _wide_rows(gpu_sess):
    """V = 65 536 (the widest row) on the device: a batch of rows re-read per pass."""
    V = 65536
    rows = Rows(1, V, eos=17, style="logits", masked=0.01, drop=0.1)
    lockstep(gpu_sess, lexfree(gpu_sess, 8, 50, eos=17, maxlen=3), rows, 4, V, 3,
             lambda t: [(BF16, 1, "dev"), (F16, 0, "strided"), (F32, 1, "host")][t % 3])


# ---- 3. mixing -----------------------------------------------------------------------------------------------------------
def test_mixed_steps(sess):
    """f32, bf16 and logits steps alternate inside one search, on both decoders."""
    V, eos = 24, 0
    plan = [(F32, 0, "dev"), (BF16, 1, "strided"), (BF16, 0, "dev"), (F32, 1, "host"), (F16, 1, "dev"),
            (F16, 0, "host")]
    rows = Rows(71, V, eos=eos, style="logits", eos_bias=-0.5, drop=0.1)
    lockstep(sess, lexfree(sess, 5, 8, eos=eos, maxlen=7), rows, 3, V, 7, lambda t: plan[t % len(plan)])
    trie = host_trie(sess.lib, V, make_lexicon(V, eos, 60, 10), 1)
    lockstep(sess, lexicon(sess, trie, 5, 8, eos=eos, maxlen=6), rows, 2, V, 6, lambda t: plan[(t + 1) % len(plan)])
    trie.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(sess):
    L = sess.lib
    gpu = is_gpu(sess)
    dec = lexfree(sess, 2, 4)()
    out = dec.begin(1, 8)
    ptrs = [o.data_ptr() if gpu else o.ctypes.data for o in out]
    if gpu:
        import torch
        x = torch.zeros((2, 8), dtype=torch.float16, device="cuda")
        xp = x.data_ptr()
    else:
        x = np.zeros((2, 8), np.float16)
        xp = x.ctypes.data
    f = L.lib.fltx_s2s_step_typed
    assert f(dec.h, xp, 3, 0, 1, 8, None, None, *ptrs) == _capi.ERR_INVALID
    assert f(dec.h, xp, -1, 0, 1, 8, None, None, *ptrs) == _capi.ERR_INVALID
    assert f(dec.h, xp, F16, 2, 1, 8, None, None, *ptrs) == _capi.ERR_INVALID
    assert f(dec.h, xp, F16, 0, 1, 7, None, None, *ptrs) == _capi.ERR_INVALID
    assert f(dec.h, xp, F32, 1, 1, 7, None, None, *ptrs) == _capi.ERR_INVALID
    assert f(dec.h, xp, F16, 1, 1, 8, None, None, *ptrs) == 0
    with pytest.raises(ValueError):
        dec.step(x, kind="probs")
    dec.close()
    bd = _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, _capi.make_options(4, 4), sess.zero, 0, 1)
    assert f(bd.h, xp, F16, 0, 1, 8, None, None, *ptrs) == _capi.ERR_STATE
    bd.close()
    if gpu:
        sess.ctx.synchronize()


# ---- 5. Python: decode(kind="logits") with a torch bf16 model ------------------------------------------------------------
def _torch_bf16_decode(gpu_sess):
    """decode(step_fn -> bf16 logits, kind="logits") equals the f32 loop on np.float32(widened - lse), lse as reported
    by a logits step on the same rows (a restatement of the search on those rows)."""
    import torch
    B, K, Kt, V, eos, maxlen = 6, 5, 9, 48, 3, 6
    g = np.random.default_rng(11)
    E = torch.from_numpy(g.standard_normal((V + 1, V)).astype(np.float32) * 2).cuda()
    H0 = torch.from_numpy(g.standard_normal((B, V)).astype(np.float32)).cuda()
    ctx = gpu_sess.ctx

    def model(prefixes):
        """bf16 logits of each prefix: an elementwise recurrence, the same bits whatever the batch"""
        out = []
        for b, p in prefixes:
            h = H0[b].clone()
            for tok in [-1] + list(p):
                h = h * 0.5 + E[tok if tok >= 0 else V]
            out.append(h.to(torch.bfloat16))
        return torch.stack(out)

    state = {"p": [(b, []) for b in range(B) for _ in range(K)]}

    def step_fn(token, src_row, row_mask, t):
        tok, src = token.cpu().tolist(), src_row.cpu().tolist()
        if t > 0:
            state["p"] = [(r // K, state["p"][s][1] + [tk]) if s >= 0 else (r // K, []) for r, (tk, s)
                          in enumerate(zip(tok, src))]
        return model(state["p"])

    dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 1e9), gpu_sess.zero, eos, maxlen)
    got = dec.decode(step_fn, B, V, kind="logits")
    dec.close()

    one = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(1, 1, 1e9), gpu_sess.zero, eos, 1)

    class Ref:
        width = V

        def __init__(self, b):
            self.b = b

        def row(self, prefix):
            x = model([(self.b, prefix)])
            lse = torch.full((1,), 0.0, dtype=torch.float64, device="cuda")
            one.begin(1, V)
            one.step(x, kind="logits", lse_out=lse)
            ctx.synchronize()
            w = x.float().cpu().numpy()[0].astype(np.float64)
            return (w - float(lse.item())).astype(np.float32)

    for b in range(B):
        want, _ = restate(Ref(b), HostLM(None), K, Kt, 1e9, 0.0, 0.0, eos, maxlen)
        assert [(h.score, h.am, h.lm, list(h.tokens)) for h in got[b]] == want, b
    one.close()


if CHILD:  # (GPU-only cases: defined in the child alone)
    test_wide_rows = pytest.mark.gpu(_wide_rows)
    test_torch_bf16_decode = pytest.mark.gpu(_torch_bf16_decode)


@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_S2S_MO_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
