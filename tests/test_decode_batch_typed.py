"""GPU (-m gpu): fltx_decode_batch_typed -- fp16 / bf16 / float32 frames, log-probs or raw logits, on the word-piece lane
engine (text_amd/csrc/fltx_wlane_typed.h) and, for what that engine hands on, through the widening kernel.

Reference: numpy float64 throughout -- lse = m + log(sum(exp(x - m))), e = float32(float64(x) - lse) -- and the CPU oracle
on e.  Log-probs are exact.  For logits the returned frame_lse is first held to LSE_BOUND of the float64 lse; e is then
formed from the RETURNED lse, and the typed n-best must equal the oracle's on that e and fltx_decode_batch's, bit for bit.
Every row is a seeded permutation of distinct representable values and the oracle must report no tie in any case."""
import ctypes as C

import numpy as np
import pytest

import helpers
from oracle import orclib
from text_amd import _capi

pytestmark = pytest.mark.gpu

F32, F16, BF16 = _capi.DTYPE_F32, _capi.DTYPE_F16, _capi.DTYPE_BF16
DTYPES = {"f32": F32, "f16": F16, "bf16": BF16}
TS = [12, 1, 7]
K, KT, THR = 12, 16, 25.0
# (N, frame_stride): the first word-piece width; odd frame starts and unaligned 16-byte blocks; one past a chunk of 1 024
# with a stride > N; a partial second chunk with an odd stride > N
SHAPES = [(65, 0), (67, 67), (1025, 1032), (1088, 1091)]
# (shape, values, kind) -> a seed the oracle reports no tie for; float32 rows hold bf16's values.  Searched on the CPU --
# for logits also with lse moved by up to 2.5e-8, since e rounds differently when lse differs in its last bits; a seed that
# ties is replaced, not excused
SEEDS = {(65, "bf16", "log_probs"): 0, (65, "bf16", "logits"): 5, (65, "f16", "log_probs"): 0, (65, "f16", "logits"): 9,
         (67, "bf16", "log_probs"): 1, (67, "bf16", "logits"): 1, (67, "f16", "log_probs"): 0, (67, "f16", "logits"): 18,
         (1025, "bf16", "log_probs"): 0, (1025, "bf16", "logits"): 30, (1025, "f16", "log_probs"): 0,
         (1025, "f16", "logits"): 5, (1088, "bf16", "log_probs"): 1, (1088, "bf16", "logits"): 1,
         (1088, "f16", "log_probs"): 0, (1088, "f16", "logits"): 9, ("nan", "bf16", "log_probs"): 0,
         ("nan", "bf16", "logits"): 1, ("nan", "f16", "log_probs"): 0, ("nan", "f16", "logits"): 7}


def seed_of(shape, dt, kind):
    return SEEDS[(shape, "f16" if dt == "f16" else "bf16", kind)]
# The largest |frame_lse - float64 lse| measured on the MI355X over the cases of this file is 1.4e-8
# (profiles/decode_typed/README.md).  The bound is that times 4: the factor covers expf's float32 rounding (2^-24 relative
# per term; the kernel adds the float32 terms in double, numpy adds float64 ones) summed over the N terms of other data.
LSE_BOUND = 4 * 1.4e-8
NAN_BITS = {F32: 0x7FC00000, F16: 0x7E00, BF16: 0x7FC0}
NEG_INF_BITS = {F32: 0xFF800000, F16: 0xFC00, BF16: 0xFF80}


HEAD = 20  # values per row that can reach a token beam of 16


def raw_rows(seed, frames, N, dt):
    """[frames, N] raw elements, every row a seeded permutation of N distinct negative values of the type (float32: of
    bf16's).  Sums of 8-bit and 11-bit significands tie easily when the addends share an exponent, so the HEAD largest
    values of a row have an exponent each (2^-16 .. 2^4, fp16's subnormals among them) under a random significand; the rest
    lie beyond the beam threshold, 64 .. 2^15 in magnitude."""
    rng = np.random.default_rng(seed)
    mb, bias = (10, 15) if dt == F16 else (7, 127)
    rows = []
    for _ in range(frames):
        ex = rng.permutation(np.arange(-16, 5))[:HEAD]
        m = rng.integers(0, 1 << mb, HEAD)
        if dt == F16:  # below 2^-14: subnormals, m * 2^-24 with the leading bit of the significand in m
            sub = ex < -14
            m = np.where(sub, (m | (1 << mb)) >> (-14 - np.minimum(ex, -14)), m)
            ex = np.maximum(ex, -15)
        head = 0x8000 | ((ex + bias) << mb) | m
        tail = 0x8000 + ((6 + bias) << mb) + rng.permutation(9 << mb)[:N - HEAD]
        rows.append(rng.permutation(np.concatenate([head, tail])))
    bits = np.stack(rows)
    return (bits.astype(np.uint32) << 16) if dt == F32 else bits.astype(np.uint16)


def widen(raw, dt):
    if dt == F16:
        return raw.view(np.float16).astype(np.float32)
    return (raw if dt == F32 else raw.astype(np.uint32) << 16).view(np.float32)


def lse64(w):
    """float64 log-sum-exp of every row over its non-NaN entries; the maximum itself when that is not finite"""
    x = w.astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(x).all(axis=1), -np.inf, np.nanmax(np.where(np.isnan(x), -np.inf, x), axis=1))
        s = np.nansum(np.exp(x - m[:, None]), axis=1)
        return np.where(np.isfinite(m), m + np.log(s), m)


class Gpu:
    """device buffers without torch: the HIP runtime the library itself is linked to"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.held = []

    def put(self, a):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert self.hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        self.held.append(p)
        return p.value

    def get(self, ptr, a):
        assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.nbytes), 2) == 0
        return a

    def free(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []


@pytest.fixture
def gpu():
    g = Gpu()
    yield g
    g.free()


def oracle_nbest(orc, es, N):
    opt = orclib.make_options(K, KT, THR)
    lm = orc.lm_zero_create()
    dec = orc.lexfree(opt, lm, 0, N - 1)
    out = []
    for e in es:
        orc.ties(dec, reset=True)
        out.append(orc.decode(dec, e, len(e), N))
        assert not any(orc.last_ties.values()), orc.last_ties
    orc.decoder_destroy(dec)
    orc.lm_destroy(lm)
    return out


def decoder(sess, N):
    return _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, _capi.make_options(K, KT, THR), sess.zero, 0, N - 1)


def run_typed(sess, mem, orc, raw, dt, kind, N, stride, host, widened):
    """raw [sum(TS), N] through the typed call, frames `stride` apart (gaps hold NaN) -> the largest lse gap"""
    S = stride or N
    frames = raw.shape[0]
    buf = np.full(frames * S + 8, NAN_BITS[dt], dtype=raw.dtype)
    for f in range(frames):
        buf[f * S:f * S + N] = raw[f]
    w = widen(raw, dt).reshape(frames, N)
    d = decoder(sess, N)
    lse_dev = mem.put(np.full(frames, 7.0))
    d.decode_batch_typed(buf.ctypes.data if host else mem.put(buf), TS, N, kind=kind, frame_stride=stride,
                         frame_lse=lse_dev, dtype=dt, on_device=0 if host else 1)
    got = [d.results(b) for b in range(len(TS))]
    assert (d.get("wlane"), d.get("typed_widened"), d.get("redone")) == (1, widened, widened)
    lse = mem.get(lse_dev, np.zeros(frames))
    d.close()
    gap = 0.0
    if kind == "logits":
        ref = lse64(w)
        fin = np.isfinite(ref)
        assert np.array_equal(lse[~fin], ref[~fin])  # an all-NaN frame: lse = the maximum, -inf
        gap = float(np.abs(lse[fin] - ref[fin]).max())
        print("lse gap %s %s N=%d: %.3g" % (dt, kind, N, gap))
        assert gap <= LSE_BOUND
        with np.errstate(invalid="ignore"):
            w = (w.astype(np.float64) - lse[:, None]).astype(np.float32)
    else:
        assert (lse == 7.0).all(), "log-probs mode leaves frame_lse untouched"
    es = np.split(w, np.cumsum(TS)[:-1])
    d32 = decoder(sess, N)
    d32.decode_batch(w, TS, N)
    for b, want in enumerate(oracle_nbest(orc, es, N)):
        for other, what in ((want, "oracle"), (d32.results(b), "fltx_decode_batch")):
            ok, why = helpers.hyps_equal(other, got[b])
            assert ok, "utterance %d vs %s: %s" % (b, what, why)
    d32.close()
    return gap


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kind", ["log_probs", "logits"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,stride", SHAPES)
def test_parity(gpu_session, oracle_lib, gpu, N, stride, dt, kind, host):
    raw = raw_rows(seed_of(N, dt, kind), sum(TS), N, DTYPES[dt])
    raw[TS[0] + TS[1], [3, N - 2]] = NEG_INF_BITS[DTYPES[dt]]  # -inf entries: never candidates, nothing in the sum
    run_typed(gpu_session, gpu, oracle_lib, raw, DTYPES[dt], kind, N, stride, host, 0)


@pytest.mark.parametrize("kind", ["log_probs", "logits"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_nan_frames_go_through_the_widening_kernel(gpu_session, oracle_lib, gpu, dt, kind):
    """utterance 0 has a frame with -inf and NaN entries and an all-NaN frame: the word-piece engine gives it up, and it is
    decoded again from the float32 rows the widening kernel writes -- the same e, the same lse"""
    N, stride = 67, 67
    raw = raw_rows(seed_of("nan", dt, kind), sum(TS), N, DTYPES[dt])
    raw[3, [0, 5]] = NEG_INF_BITS[DTYPES[dt]]
    raw[3, [1, 40]] = NAN_BITS[DTYPES[dt]]
    raw[5, :] = NAN_BITS[DTYPES[dt]]
    run_typed(gpu_session, gpu, oracle_lib, raw, DTYPES[dt], kind, N, stride, False, 1)


@pytest.mark.parametrize("what,code", [("dtype", _capi.ERR_INVALID), ("kind", _capi.ERR_INVALID), ("stride", _capi.ERR_INVALID),
                                       ("host_lm", _capi.ERR_STATE), ("stream", _capi.ERR_STATE)])
def test_refusals(gpu_session, what, code):
    N = 65
    e, T = np.zeros(2 * N, np.float32), np.array([2], np.int32)
    lm = gpu_session.zero
    if what == "host_lm":
        lm = gpu_session.lm_for({"lm": ("lastword", 3), "kind": "lexfree", "N": N, "is_lm_token": False}, {})
    d = _capi.BatchDecoder(gpu_session.ctx, _capi.LEXFREE, _capi.make_options(K, KT, THR), lm, 0, N - 1)
    if what == "stream":
        d.stream_begin(1, N, 8)
    rc = d.L.lib.fltx_decode_batch_typed(d.h, e.ctypes.data, 7 if what == "dtype" else F32, 5 if what == "kind" else 0, 0,
                                         None, N - 1 if what == "stride" else 0, T.ctypes.data, 1, N, None)
    assert rc == code
    d.close()
