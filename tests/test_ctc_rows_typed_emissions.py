"""fp16 / bf16 / float32 emissions and raw logits in the lexicon-free CTC rows decoder (fltx_ctc_rows_begin_typed,
fltx_ctc_rows_stream_append_typed; text_amd/csrc/fltx_ctc_rows_typed.h).

The parity chain: decoder A gets the typed frames, decoder B the float32 matrix they stand for -- the exact widening for
log-probs, np.float32(np.float64(widened) - lse) with the lse A reports for logits -- through the EXISTING float32 entry
points.  The row lists of every step, the final tokens and all three scores must be identical bit for bit, under
max-merge and under logAdd alike (the steps are the same code on the same records); every reported lse is held to
1e-6 * max(1, |ref|) of a float64 log-sum-exp, the bound tests/test_seq2seq_model_output.py holds the seq2seq lse to.
The float32 path is pinned to the compiled reference's fixtures by tests/test_ctc_lm_rows.py; the typed entry with
float32 log-probs is linked to the same fixtures here.  For seeded cases of distinct representable values the float64
restatement of tests/test_ctc_lm_rows.py agrees on the widened matrix and reports zero ties.

Every case runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_CTC_ROWS_TYPED_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
from golden import make_ctc_lm_rows_golden as G  # noqa: E402
import test_ctc_lm_rows as C0  # noqa: E402
import test_ctc_lm_rows_stream as S0  # noqa: E402
from test_ctc_lm_rows import PrefixLM, Stats, _dev, make_dec  # noqa: E402
from test_seq2seq_model_output import (BF16, F16, F32, NAN_BITS, _bits_equal, _GpuSess, _np, is_gpu, ref_lse,  # noqa: E402
                                       to_dtype, widen)

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
KINDS = {"log_probs": 0, "logits": 1}
DT_NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}
SENTINEL = 7.0


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


# ---- typed frames in a caller's buffer ------------------------------------------------------------------------------------
def place(raws, dt, N, layout):
    """raws[b]: [T_b, N] raw elements -> (buffer, offsets or None, frame stride): "packed" -- frame after frame, no
    offsets, stride 0 (= N) -- or "odd": an odd stride > N, odd offsets, every gap filled with NaN bits so that a read
    outside a frame shows"""
    if layout == "packed":
        flat = [r.reshape(-1) for r in raws]
        return (np.concatenate(flat) if flat else np.zeros(0, raws[0].dtype)), None, 0
    S = (N + 2) | 1
    offs, cur = [], 1
    for r in raws:
        offs.append(cur)
        cur = (cur + r.shape[0] * S + 2) | 1
    buf = np.full(cur + 4, NAN_BITS[dt]).view(raws[0].dtype).copy()
    for r, o in zip(raws, offs):
        for f in range(r.shape[0]):
            buf[o + f * S:o + f * S + N] = r[f]
    return buf, np.asarray(offs, np.int64), S


def lse_buf(sess, n):
    return _dev(sess, np.full(max(n, 1), SENTINEL))


def _args(sess, dec, buf, dt, host, offs, lse):
    """-> (address, on_device, offsets address, frame_lse address, what must stay alive)"""
    keep = buf if host or not is_gpu(sess) else _dev(sess, buf, dt)
    ptr = keep.ctypes.data if isinstance(keep, np.ndarray) else keep.data_ptr()
    return ptr, 0 if host else 1, _capi._ptr(offs), None if lse is None else dec._addr(lse), keep


def begin_typed(sess, dec, buf, dt, kind, host, offs, stride, Ts, N, lse):
    """fltx_ctc_rows_begin_typed itself -> the row lists"""
    T = np.ascontiguousarray(Ts, np.int32)
    dec.B, dec.N, dec._T = len(T), int(N), T
    out = dec._rows()
    ptr, on_dev, offp, lsep, keep = _args(sess, dec, buf, dt, host, offs, lse)
    dec._chk(dec.L.lib.fltx_ctc_rows_begin_typed(dec.h, ptr, dt, KINDS.get(kind, kind), on_dev, offp, stride, _capi._ptr(T),
                                                 dec.B, dec.N, lsep, *[dec._addr(o) for o in out]))
    dec._emissions = keep
    return tuple(out)


def append_typed(sess, dec, buf, dt, kind, host, offs, stride, Ts, lse):
    T = np.ascontiguousarray(Ts, np.int32)
    ptr, on_dev, offp, lsep, keep = _args(sess, dec, buf, dt, host, offs, lse)
    dec._chk(dec.L.lib.fltx_ctc_rows_stream_append_typed(dec.h, ptr, dt, KINDS.get(kind, kind), on_dev, offp, stride,
                                                         _capi._ptr(T), lsep))
    dec._emissions, dec._T = keep, T
    return int(T.max())


def check_lse(got, raws, dt, kind):
    """the reported lse of every frame against the float64 log-sum-exp -> the float32 matrices e the frames stand for"""
    out, at = [], 0
    for r in raws:
        w = widen(r, dt).reshape(r.shape)
        if kind == "log_probs":
            out.append(w)
            continue
        ls = got[at:at + r.shape[0]]
        at += r.shape[0]
        for f in range(r.shape[0]):
            ref = ref_lse(w[f])
            if np.isfinite(ref):
                assert abs(ls[f] - ref) <= 1e-6 * max(1.0, abs(ref)), (f, ls[f], ref)
            else:
                assert ls[f] == ref, (f, ls[f], ref)  # an all-NaN frame, a maximum that is not finite: lse = max
        with np.errstate(invalid="ignore"):
            out.append((w.astype(np.float64) - ls[:, None]).astype(np.float32))
    if kind == "log_probs":
        assert (got == SENTINEL).all(), "log-probs mode leaves frame_lse untouched"
    return out


def same_decodes(a, b, what=""):
    """(final, rows, prefix) of two decodes: the n-best bit for bit, the row lists of every frame"""
    (fa, ra, pa), (fb, rb, pb) = a, b
    assert len(fa) == len(fb)
    for u in range(len(fa)):
        assert len(fa[u]) == len(fb[u]), (what, u, len(fa[u]), len(fb[u]))
        for x, y in zip(fa[u], fb[u]):
            assert x[3:] == y[3:] and _bits_equal(x[:3], y[:3]), (what, u, x, y)
        assert [[(s, t, i, pa[u][i]) for s, t, i in fr] for fr in ra[u]] == \
            [[(s, t, i, pb[u][i]) for s, t, i in fr] for fr in rb[u]], (what, u)


def run_pair(sess, mk_dec, decode, raws, dt, kind, N, W, lm_row, layout="packed", host=False, front=None, lse=True):
    """decoder A on the typed frames, decoder B on the float32 matrix they stand for -> (A's decode, B's, the matrices, lse)"""
    Ts = [r.shape[0] for r in raws]
    dec = mk_dec()
    if front is not None:  # the wave-per-frame front end for every width it can take, or for none
        dec.set("emissions_narrow_max", 1024 if front == "wave" else 0)
    buf, offs, stride = place(raws, dt, N, layout)
    lb = lse_buf(sess, sum(Ts)) if lse else None
    dec.begin = lambda flat, Ts_, N_: begin_typed(sess, dec, buf, dt, kind, host, offs, stride, Ts, N, lb)
    a = decode(sess, dec, [np.zeros((T, N), np.float32) for T in Ts], N, W, lm_row)
    if is_gpu(sess):
        dec.ctx.synchronize()
    assert np.array_equal(buf.view(np.uint8), place(raws, dt, N, layout)[0].view(np.uint8))  # (read only)
    ls = _np(lb).copy()[:sum(Ts)] if lse else None
    dec.close()
    if ls is None:
        return a, None, None, None
    e32 = check_lse(ls, raws, dt, kind)
    ref = mk_dec()
    b = decode(sess, ref, e32, N, W, lm_row)
    ref.close()
    same_decodes(a, b, (DT_NAMES[dt], kind, N, layout, host, front))
    return a, b, e32, ls


def frames(seed, T, N, dt, kind):
    """[T, N] raw elements: the golden module's emissions rounded to dt (log-probs), wide normal logits"""
    if kind == "log_probs":
        return to_dtype(G.emissions(seed, T, N).astype(np.float64), dt).reshape(T, N)
    return to_dtype(np.random.default_rng(seed).standard_normal((T, N)) * 3.0, dt).reshape(T, N)


class Case:
    def __init__(self, sess, N, K, Kt, log_add=False, thr=25.0, lm_seed=77):
        W = N + 1
        self.sess, self.N, self.W = sess, N, W
        self.rl = G.SmRowsLM(lm_seed, N, W, 0, W - 1, 0)
        self.lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
        self.o = (K, Kt, thr, 0.7, -0.2, 0, 1 if N > 1 else 0, log_add)

    def mk(self):
        return make_dec(self.sess, self.lm, *self.o)

    def lm_row(self, b, p):
        return self.rl.row(list(p))

    def pair(self, raws, dt, kind, **kw):
        return run_pair(self.sess, self.mk, C0.decode, raws, dt, kind, self.N, self.W, self.lm_row, **kw)

    def close(self):
        self.lm.close()


def narrow_max(sess):
    c = Case(sess, 2, 1, 1)
    dec = c.mk()
    n = int(dec.get("emissions_narrow_max"))
    dec.close()
    c.close()
    return n


# ---- 1. shapes: the smallest at which the front ends can go wrong ----------------------------------------------------------
# (N, Kt, dtype, kind, layout, host, front): N = 2, 29, 63 / 64 / 65 on both front ends, beam_size_token below, equal to
# and above N, odd N with 2-byte types at odd offsets and an odd stride > N, host and device buffers, T = 0 in the batch
SHAPES = [(2, 1, BF16, "logits", "odd", False, None), (2, 2, F16, "log_probs", "packed", True, "wg"),
          (29, 8, BF16, "logits", "odd", False, None), (29, 29, F16, "logits", "packed", True, "wg"),
          (29, 40, F32, "logits", "odd", True, None), (29, 5, F32, "log_probs", "odd", False, "wg"),
          (63, 7, F16, "logits", "odd", False, "wave"), (63, 7, BF16, "log_probs", "odd", True, "wg"),
          (64, 64, BF16, "logits", "packed", False, "wave"), (64, 9, F16, "logits", "odd", False, "wg"),
          (65, 66, F16, "log_probs", "odd", False, "wave"), (65, 6, BF16, "logits", "odd", True, "wg"),
          (65, 6, F32, "logits", "packed", False, "wave")]


@pytest.mark.parametrize("N,Kt,dt,kind,layout,host,front", SHAPES,
                         ids=["N%d-Kt%d-%s-%s-%s-%s-%s" % (s[0], s[1], DT_NAMES[s[2]], s[3], s[4], "host" if s[5] else "dev", s[6])
                              for s in SHAPES])
def test_parity_over_shapes(sess, N, Kt, dt, kind, layout, host, front):
    c = Case(sess, N, 4, Kt)
    raws = [frames(1000 + 10 * N + b, T, N, dt, kind) for b, T in enumerate((5, 0, 3))]
    a, _, _, _ = c.pair(raws, dt, kind, layout=layout, host=host, front=front)
    assert [len(h[3]) for u in a[0] for h in u[:1]] == [7, 2, 5]  # (T = 0: the root's sil and decodeEnd's)
    c.close()


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("side", [0, 1])
def test_parity_on_both_sides_of_the_switch_over(sess, side, log_add):
    """N = the widest frame a wave takes and one more, the default choice of the front end; max-merge and logAdd"""
    N = narrow_max(sess) + side
    c = Case(sess, N, 4, 6, log_add=log_add)
    c.pair([frames(2000 + b, T, N, BF16, "logits") for b, T in enumerate((3, 2))], BF16, "logits", layout="odd")
    c.close()


@pytest.mark.parametrize("N", [16384, 16385])
def test_read_once_boundary(sess, N):
    """the workgroup front end keeps a frame of up to 16 384 values in registers and re-reads a wider one: two frames"""
    c = Case(sess, N, 2, 3)
    c.pair([frames(2100, 2, N, BF16, "logits")], BF16, "logits")
    c.close()


def test_small_alphabet_merges(sess):
    """N = 3, K = 8: hypotheses merge and states are entered again, under logAdd -- still bit for bit"""
    for log_add in (False, True):
        c = Case(sess, 3, 8, 3, log_add=log_add)
        c.pair([frames(2200 + b, T, 3, F16, "logits") * np.float16(0.25) for b, T in enumerate((10, 1, 6))], F16, "logits")
        c.close()


# ---- 2. the reference's fixtures through the typed entry ------------------------------------------------------------------
@pytest.mark.parametrize("c", C0._golden(), ids=lambda c: c["name"])
def test_typed_float32_log_probs_reproduce_reference_fixtures(c, sess):
    rl = G.case_lm(c)
    lm = _capi.RowsLM(rl.W, rl.usr_to_lm if c["perm"] else None, rl.finish, lib=sess.lib)
    dec = make_dec(sess, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"], c["sil"], c["blank"], c["log_add"])
    em = G.emissions(c["seed"], c["T"], c["N"])
    dec.begin = lambda flat, Ts, N: begin_typed(sess, dec, em.reshape(-1), F32, "log_probs", False, None, 0, Ts, N, None)
    got, _, _ = C0.decode(sess, dec, [em], c["N"], rl.W, lambda b, p: rl.row(list(p)))
    C0.assert_final(c["hyps"], got[0], c["log_add"], c["name"])
    dec.close()
    lm.close()


# ---- 3. an independent oracle: the float64 restatement on the widened matrix, no ties ---------------------------------------
def distinct_frames(seed, T, N, dt, kind):
    """frames of distinct values representable in dt (the "perm" style of the seq2seq tests): a permutation of a grid of
    7-bit multiples of 2^-4, exact in fp16 and bf16 alike, per frame"""
    g = np.random.default_rng(seed)
    x = np.stack([-(g.permutation(127)[:N] + 1.0) * 2.0 ** -4 for _ in range(T)])
    if kind == "logits":
        x = x + 3.0
    raw = to_dtype(x, dt).reshape(T, N)
    assert np.array_equal(widen(raw, dt).reshape(T, N).astype(np.float64), x)
    return raw


@pytest.mark.parametrize("kind", ["log_probs", "logits"])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=["f16", "bf16", "f32"])
def test_restatement_agrees_on_distinct_values(sess, dt, kind):
    """(for logits the restatement reads the matrix built from the lse the device reports, itself held to the float64
    log-sum-exp: a float64 lse of its own could round an emission the other way)"""
    N, K, Kt, T = 12, 4, 5, 8
    c = Case(sess, N, K, Kt)
    lm = PrefixLM(lambda p: c.rl.row(list(p)), c.rl.usr_to_lm, c.rl.finish)
    done = 0
    for seed in range(3000, 3040):
        raw = distinct_frames(seed, T, N, dt, kind)
        if kind == "log_probs":  # the zero-tie condition is the restatement's alone: found before the device runs
            st = Stats()
            C0.restate(widen(raw, dt).reshape(T, N), lm, *c.o, st=st)
            if st.ties:
                continue
        a, _, e32, _ = c.pair([raw], dt, kind)
        st = Stats()
        want, want_rows = C0.restate(e32[0], lm, *c.o, st=st)
        if st.ties:
            continue
        C0.assert_final(want, a[0][0], False, seed)
        C0.assert_rows(want_rows, a[1][0], a[2][0])
        done += 1
        if done == 2:
            break
    assert done == 2, "no tie-free seeds"
    c.close()


# ---- 4. values --------------------------------------------------------------------------------------------------------------
def test_special_values(sess):
    """fp16 subnormals, +-inf, NaN and -0; a frame that is all NaN and one whose maximum is -inf: there lse equals the
    maximum and the frame has no candidates"""
    N = 6
    inf = np.inf
    x = np.asarray([[-0.0, -2.0 ** -24, -2.0 ** -15, -1.0, np.nan, -inf],
                    [-2.0 ** -14, 5.96e-8, -0.5, np.nan, -3.0, -0.25],
                    [-1.0, -0.0, 0.0, -2.0, -inf, 2.0 ** -24]])
    for dt in (F16, BF16):
        for kind in ("log_probs", "logits"):
            c = Case(sess, N, 4, 4)
            a, _, _, ls = c.pair([to_dtype(x, dt).reshape(3, N)], dt, kind, layout="odd")
            assert len(a[0][0]) >= 1
            c.close()
    dead = [np.full(N, np.nan), np.asarray([-inf, np.nan, -inf, -inf, np.nan, -inf])]
    for bad in dead:
        y = np.stack([x[2], bad, x[0]])
        c = Case(sess, N, 4, 4)
        a, _, _, ls = c.pair([to_dtype(y, F16).reshape(3, N), to_dtype(x, F16).reshape(3, N)], F16, "logits")
        assert ls[1] == -inf and a[0][0] == [] and a[1][0][1] == [] and len(a[0][1]) >= 1
        c.close()
    c = Case(sess, N, 4, 4)  # +inf: lse = +inf, every finite logit is -inf, the +inf one NaN
    y = x.copy()
    y[1, 2] = inf
    a, _, _, ls = c.pair([to_dtype(y, BF16).reshape(3, N)], BF16, "logits")
    assert ls[1] == inf
    c.close()


def test_logits_rounding_ties_at_the_cut(sess):
    """Logits 2^-30 apart beside one of 20: after the lse is subtracted they round to ONE float, and the token cut falls
    among them -- the ties go to the lower tokens, as on the float32 matrix"""
    N, Kt = 8, 4
    x = np.zeros((3, N))
    for t in range(3):
        x[t] = np.arange(N)[::-1] * 2.0 ** -30  # (the higher token has the smaller logit, and still wins no tie)
        x[t, (3 * t) % N] = 20.0
    c = Case(sess, N, 6, Kt, thr=1e9)
    a, b, e32, _ = c.pair([to_dtype(x, F32).reshape(3, N)], F32, "logits", layout="odd")
    for t in range(3):
        assert len(set(e32[0][t].tolist())) == 2  # one float for the seven
    st = Stats()
    C0.restate(e32[0], PrefixLM(lambda p: c.rl.row(list(p)), c.rl.usr_to_lm, c.rl.finish), *c.o, st=st)
    assert any(w == "token cut" for _, w in st.ties)
    toks = {tok for fr in a[1][0][:1] for _, tok, _ in fr if tok >= 0}
    assert toks == {2, 3}, toks  # frame 0 keeps token 0 (the 20: sil again) and the lowest three of the equal ones: 1 is blank
    c.close()


# ---- 5. streams --------------------------------------------------------------------------------------------------------------
class Streams(S0.DeviceStreams):
    """DeviceStreams with typed chunks, the planner on every list and collect: every event is kept for the comparison"""

    def __init__(self, *a, cap=64, **kw):
        self.events, self.cap, self.planned = [], cap, False
        S0.DeviceStreams.__init__(self, *a, **kw)

    def _take(self, out, stepped, first=False):
        S0.DeviceStreams._take(self, out, stepped, first)
        self.events.append(("rows", [[(s, t, self.prefix[b][i]) for s, t, i in self.rows[b][-1]] if stepped[b] else None
                                     for b in range(self.B)]))
        if first:
            self.dec.plan_begin(self.cap)
        p = self.dec.plan(*out)
        if is_gpu(self.sess):
            self.dec.ctx.synchronize()
        self.events.append(("plan", [_np(getattr(p, n)).tolist() for n in
                                     ("lm_row_of", "new_row", "new_parent_row", "new_edge", "new_dec_row", "counts")]))

    def typed_chunk(self, raws, dt, kind, layout, host, lse):
        Ts = [r.shape[0] for r in raws]
        buf, offs, stride = place(raws, dt, self.N, layout)
        steps = append_typed(self.sess, self.dec, buf, dt, kind, host, offs, stride, Ts, lse)
        held = self.dec._emissions
        for t in range(steps):
            self._take(self.dec.step(self.lm_rows()), [t < T for T in Ts])
        return held

    def collect(self):
        rel, n_rel, live = self.dec.collect(16)
        self.dec.plan_release(rel, n_rel)
        if is_gpu(self.sess):
            self.dec.ctx.synchronize()
        n = _np(n_rel)
        for b in range(self.B):  # (a released id may come back for another state)
            for i in _np(rel)[b, :int(n[b])].tolist():
                self.prefix[b].pop(i)
        self.events.append(("collect", [sorted(_np(rel)[b, :int(n[b])].tolist()) for b in range(self.B)], _np(live).tolist()))


def overwrite(sess, held, dt):
    """a chunk's buffer, once the next append has been queued, is the caller's again"""
    if isinstance(held, np.ndarray):
        held[...] = np.asarray(NAN_BITS[dt]).view(held.dtype)
    else:
        held.fill_(float("nan"))


def stream_script(sess, mk_dec, N, W, lm_row, lexicon=False, T=(14, 9)):
    """Chunks of unequal lengths whose dtype and kind change from chunk to chunk, typed appends alternating with float32
    ones; best(look_back), prune, collect + plan_release and end -- event by event against decoder B fed the equivalent
    float32 chunks.  The buffer of a device chunk is overwritten after the next append has been queued."""
    B = len(T)
    plan = [((3, 2), BF16, "logits", "odd", False), ((4, 0), None, None, None, None), ((2, 3), F16, "log_probs", "odd", True),
            ((0, 2), F32, "logits", "packed", False), ((5, 2), BF16, "log_probs", "packed", False)]
    assert tuple(sum(p[0][b] for p in plan) for b in range(B)) == tuple(T)
    dA, dB = mk_dec(), mk_dec()
    for d in (dA, dB):
        d.set_max_states(64)
    A = Streams(sess, dA, B, N, W, lm_row, 12, lexicon=lexicon)
    Bs = Streams(sess, dB, B, N, W, lm_row, 12, lexicon=lexicon)
    held = None
    for i, (Ts, dt, kind, layout, host) in enumerate(plan):
        if dt is None:
            parts = [G.emissions(4000 + 10 * i + b, Ts[b], N) for b in range(B)]
            A.chunk(parts)
            now = None
        else:
            raws = [frames(4000 + 10 * i + b, Ts[b], N, dt, kind) for b in range(B)]
            lb = lse_buf(sess, sum(Ts))
            now = (A.typed_chunk(raws, dt, kind, layout, host, lb), dt)
            if is_gpu(sess):
                dA.ctx.synchronize()
            parts = check_lse(_np(lb).copy()[:sum(Ts)], raws, dt, kind)
        if held is not None and not held[2]:
            overwrite(sess, held[0], held[1])
        held = None if now is None else (now[0], now[1], host)
        Bs.chunk(parts)
        for S in (A, Bs):
            S.events.append(("best", [S.best(b, lb_) for b in range(B) for lb_ in (0, 2)]))
            if i in (1, 3):
                S.dec.prune(3)
                S.events.append(("frames", [S.dec.frames_in_buffer(b) for b in range(B)]))
                S.collect()
    fa, fb = A.end(), Bs.end()
    assert len(A.events) == len(Bs.events)
    for ea, eb in zip(A.events, Bs.events):
        assert ea[0] == eb[0]
        if ea[0] == "best":
            for x, y in zip(ea[1], eb[1]):
                assert (x is None) == (y is None) and (x is None or (x[3:] == y[3:] and _bits_equal(x[:3], y[:3]))), (x, y)
        else:
            assert ea == eb, (ea, eb)
    same_decodes((fa, [[]] * B, None), (fb, [[]] * B, None), "stream")
    assert all(fa[b] for b in range(B)) and any(e[0] == "collect" and any(e[1]) for e in A.events)
    dA.close()
    dB.close()


def test_streams_event_by_event(sess):
    c = Case(sess, 7, 4, 3)
    stream_script(sess, c.mk, c.N, c.W, c.lm_row)
    c.close()


# ---- 6. refusals, and the Python forms ---------------------------------------------------------------------------------------
def test_refusals(sess):
    N = 5
    c = Case(sess, N, 3, 3)
    raw = frames(5000, 2, N, F16, "logits")
    dec = c.mk()

    def code(fn):
        try:
            fn()
        except ValueError:  # (what the binding raises for FLTX_ERR_INVALID)
            return _capi.ERR_INVALID
        except _capi.FltxError as e:
            return e.code
        return _capi.FLTX_OK
    for dt, kind, stride in ((3, 0, 0), (-1, 0, 0), (F16, 2, 0), (F16, -1, 0), (F16, 1, N - 1), (F16, 1, 1)):
        assert code(lambda: begin_typed(sess, dec, raw.reshape(-1), dt, kind, False, None, stride, [2], N, None)) == \
            _capi.ERR_INVALID, (dt, kind, stride)
    assert code(lambda: begin_typed(sess, dec, raw.reshape(-1), F16, 1, False, None, 0, [-1], N, None)) == _capi.ERR_INVALID
    assert code(lambda: append_typed(sess, dec, raw.reshape(-1), F16, 1, False, None, 0, [2], None)) == _capi.ERR_STATE
    dec.stream_begin(1, N, 8)
    for dt, kind, stride in ((3, 0, 0), (F16, 2, 0), (F16, 1, N - 1)):
        assert code(lambda: append_typed(sess, dec, raw.reshape(-1), dt, kind, False, None, stride, [2], None)) == \
            _capi.ERR_INVALID
    assert append_typed(sess, dec, raw.reshape(-1), F16, 1, False, None, 0, [2], None) == 2  # frame_lse NULL
    assert code(lambda: append_typed(sess, dec, raw.reshape(-1), F16, 1, False, None, 0, [1], None)) == _capi.ERR_STATE
    dec.close()
    # frame_lse NULL in a batch: the decode is the one with it
    a, _, _, _ = c.pair([raw], F16, "logits")
    a0, _, _, _ = c.pair([raw], F16, "logits", lse=False)
    same_decodes(a, a0)
    # the calls on other decoder kinds
    other = _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, _capi.make_options(3, 3, 25.0, 0.0), sess.zero, 0, 1)
    out = [np.zeros(3, np.int32) for _ in range(4)]
    L = sess.lib.lib
    T = np.asarray([2], np.int32)
    rc = L.fltx_ctc_rows_begin_typed(other.h, raw.ctypes.data, F16, 1, 0, None, 0, _capi._ptr(T), 1, N, None,
                                     *[o.ctypes.data for o in out])
    assert rc == _capi.ERR_STATE
    assert L.fltx_ctc_rows_stream_append_typed(other.h, raw.ctypes.data, F16, 1, 0, None, 0, _capi._ptr(T), None) == \
        _capi.ERR_STATE
    other.close()
    c.close()


def test_python_forms(sess):
    """numpy float16, numpy uint16 + dtype="bf16", a strided [B, T_max, N] view (a torch bfloat16 tensor on the GPU), the
    keywords through decode() -- and the float32 numpy route, which still reaches fltx_ctc_rows_begin"""
    N, B, Tm = 9, 2, 6
    Ts = [6, 4]
    c = Case(sess, N, 4, 4)
    calls = []
    lib = sess.lib.lib

    class Spy:  # counts the entry points begin() reaches
        def __getattr__(self, name):
            if name in ("fltx_ctc_rows_begin", "fltx_ctc_rows_begin_typed"):
                calls.append(name)
            return getattr(lib, name)
    x = np.random.default_rng(5100).standard_normal((B, Tm, N + 3)) * 3.0
    x[1, Ts[1]:] = np.nan  # (the padding frames are never read)
    def lm_rows(keys):
        return _dev(sess, np.stack([c.lm_row(b, p) for b, p in keys]).astype(np.float32))

    def hyps(dec, *a, **kw):
        dec.L = type("L", (), {"lib": Spy(), "check": dec.L.check, "version": dec.L.version})()
        out = dec.decode(*a, **kw)
        if is_gpu(sess):
            dec.ctx.synchronize()
        return [[(h.score, h.am, h.lm, h.tokens.tolist()) for h in u] for u in out]
    for dt in (BF16, F16):
        raw = to_dtype(x, dt).reshape(B, Tm, N + 3)
        if dt == BF16 and is_gpu(sess):
            em, kw = _dev(sess, raw, BF16)[:, :, :N], {}
            assert em.dtype == torch.bfloat16 and not em.is_contiguous()
        else:
            em, kw = raw[:, :, :N], ({"dtype": "bf16"} if dt == BF16 else {})
        lse = lse_buf(sess, sum(Ts))
        dec = c.mk()
        got = hyps(dec, em, Ts, N, lm_rows, kind="logits", lse_out=lse, **kw)
        dec.close()
        assert calls[-1] == "fltx_ctc_rows_begin_typed"
        e32 = check_lse(_np(lse).copy()[:sum(Ts)], [raw[b, :Ts[b], :N] for b in range(B)], dt, "logits")
        flat = np.concatenate([e.reshape(-1) for e in e32])
        ref = c.mk()
        want = hyps(ref, flat, Ts, N, lm_rows)
        ref.close()
        assert calls[-1] == "fltx_ctc_rows_begin"  # float32 log-probs from numpy: the existing entry point, as before
        assert len(got) == B and all(got[b] for b in range(B))
        for b in range(B):
            assert [h[3] for h in got[b]] == [h[3] for h in want[b]]
            assert all(_bits_equal(g[:3], w[:3]) for g, w in zip(got[b], want[b]))
    with pytest.raises(TypeError):
        c.mk().begin(np.zeros(N, np.uint16), [1], N, dtype="f16")
    with pytest.raises(ValueError):
        c.mk().begin(np.zeros(N, np.float32), [1], N, kind="probs")
    c.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_CTC_ROWS_TYPED_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
