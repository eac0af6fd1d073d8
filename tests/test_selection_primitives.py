"""The lane engines' selection primitives, each against a plain exact reference of the same operation.

Every decoder-level test checks a whole decode; these check the device helpers that decide which candidates survive a
frame, directly, at the shapes and edges where they can go wrong: slRankBin (the boundary bin's members ranked against
each other), slScan / slBin (the histogram selection), slRowScan and the xlRank all-pairs ranking (slane's token beam and
the frame's best candidate), wlTokBeamRows (the word-piece token beam), slLogAdd, the order keys and the wave
primitives of fltx_rt.h.

The kernels are tests/prim/fltx_prim.cpp, compiled twice from the same source:
  * HIP, by __graft_entry__.build() with the product's flags (tests/prim/libfltx_prim.so): the `gpu` tests run the code
    that ships -- its DPP / readlane primitives, its exec masks, its register allocation;
  * FLTX_EMU, by the module fixture below (tests/prim/libfltx_prim_emu.so): the same bodies on the emulator, whose wave
    primitives are its own (tests/emu/hip_emu.h) -- so the CPU tests check the kernels' logic and the emulator.
Each test runs on both (`emu` unmarked, `gpu` marked, with more configurations); the inputs are seeded.

GPU hygiene: every entry point synchronises and returns its HIP status; the first non-zero one ends the session
(pytest.exit) so that no further kernel starts on a device that has faulted.
"""
import ctypes
import decimal
import fcntl
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIM = os.path.join(ROOT, "tests", "prim")
EMU_LIB = os.path.join(PRIM, "libfltx_prim_emu.so")
HIP_LIB = os.path.join(PRIM, "libfltx_prim.so")
SL_BCAP = 128  # kSlBCap
SL_NB = 256  # kSlNB
NEG_INF = float("-inf")

def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Prim:
    """The entry points of one build of fltx_prim.cpp, with numpy in and out."""

    def __init__(self, path, gpu):
        self.lib = ctypes.CDLL(path)
        self.gpu = gpu
        self.name = "gpu" if gpu else "emu"
        for fn in ("prim_rank", "prim_scan", "prim_bin", "prim_logadd", "prim_keys", "prim_wave", "prim_rowscan",
                   "prim_tokbeam", "prim_rank_pairs", "prim_wl_tokrow_size"):
            getattr(self.lib, fn).restype = ctypes.c_int

    def _check(self, rc, what):
        if rc == 0:
            return
        if self.gpu:  # no further kernel on a device that may have faulted
            pytest.exit("%s: HIP status %d -- stopping before any further kernel starts" % (what, rc), returncode=3)
        raise AssertionError("%s returned %d on the emulator" % (what, rc))

    def rank_pairs(self):
        out = np.zeros(2 * 256, np.int32)
        n = self.lib.prim_rank_pairs(_ptr(out), 256)
        assert 0 < n <= 256
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]

    def rank(self, W, NJ, spill, cfg, slot, key):
        n = len(cfg)
        take = np.zeros((n, W), np.uint32)
        rc = self.lib.prim_rank(W, NJ, int(spill), n, _ptr(np.ascontiguousarray(cfg, np.int32)),
                                _ptr(np.ascontiguousarray(slot, np.uint32)), _ptr(np.ascontiguousarray(key, np.uint64)),
                                _ptr(take))
        assert rc != -1, "no slRankBin kernel for (%d, %d)" % (W, NJ)
        self._check(rc, "slRankBin<%d> (%d threads)" % (NJ, W))
        return take

    def scan(self, hist, kf):
        out = np.zeros((len(hist), 5), np.int32)
        self._check(self.lib.prim_scan(len(hist), _ptr(np.ascontiguousarray(hist, np.uint32)),
                                       _ptr(np.ascontiguousarray(kf, np.int32)), _ptr(out)), "slScan")
        return out

    def bin(self, best, c, sb):
        out = np.zeros((len(best), 2), np.int32)
        self._check(self.lib.prim_bin(len(best), _ptr(np.ascontiguousarray(best, np.float64)),
                                      _ptr(np.ascontiguousarray(c, np.float64)),
                                      _ptr(np.ascontiguousarray(sb, np.int32)), _ptr(out)), "slBin")
        return out

    def logadd(self, hi, lo):
        out = np.zeros(len(hi), np.float64)
        self._check(self.lib.prim_logadd(len(hi), _ptr(np.ascontiguousarray(hi, np.float64)),
                                         _ptr(np.ascontiguousarray(lo, np.float64)), _ptr(out)), "slLogAdd")
        return out

    def keys(self, d, f):
        k64 = np.zeros((len(d), 2), np.uint64)
        k32 = np.zeros((len(d), 2), np.uint32)
        self._check(self.lib.prim_keys(len(d), _ptr(np.ascontiguousarray(d, np.float64)),
                                       _ptr(np.ascontiguousarray(f, np.float32)), _ptr(k64), _ptr(k32)), "f64Key/f32Key")
        return k64, k32

    def wave(self, v, src, mm):
        n = len(v)
        out = np.zeros((n, 23, 64), np.uint64)
        self._check(self.lib.prim_wave(n, _ptr(np.ascontiguousarray(v, np.uint64)), _ptr(np.ascontiguousarray(src, np.int32)),
                                       _ptr(np.ascontiguousarray(mm, np.uint64)), _ptr(out)), "wave primitives")
        return out

    def rowscan(self, cfg, sc, rows):
        out = np.zeros((len(cfg), 7), np.uint64)
        self._check(self.lib.prim_rowscan(len(cfg), _ptr(np.ascontiguousarray(cfg, np.int32)),
                                          _ptr(np.ascontiguousarray(sc, np.float64)),
                                          _ptr(np.ascontiguousarray(rows, np.float32)), _ptr(out)), "slRowScan")
        return out

    def tokbeam(self, em, Kt, criterion, blank, sil):
        B, T, N = em.shape
        assert self.lib.prim_wl_tokrow_size() == TOKROW.itemsize
        rows = np.zeros(B * T, TOKROW)
        self._check(self.lib.prim_tokbeam(B, T, N, Kt, criterion, blank, sil,
                                          _ptr(np.ascontiguousarray(em, np.float32)), _ptr(rows)),
                    "wlTokBeamRows (N %d, Kt %d)" % (N, Kt))
        return rows


TOKROW = np.dtype([("e", "<f4", 64), ("tok", "<u2", 64), ("eBlank", "<f4"), ("eSil", "<f4"), ("ek", "<u4"),
                   ("nList", "<i4"), ("silPos", "<i4"), ("flags", "<u4"), ("pad", "<u4", 2)])


def _emu_sources():
    import glob
    return (glob.glob(os.path.join(ROOT, "text_amd", "csrc", "fltx_*.h")) + [os.path.join(ROOT, "include", "fltx.h")] +
            glob.glob(os.path.join(ROOT, "tests", "emu", "hip_emu.*")) + [os.path.join(PRIM, "fltx_prim.cpp")])


@pytest.fixture(scope="module")
def emu_prim():
    """The emulator build of fltx_prim.cpp (as tests/emu/build.sh builds the decoder's): rebuilt when a source is newer."""
    with open(os.path.join(PRIM, ".build.lock"), "w") as lock:  # (pytest-xdist: one worker builds, the others wait)
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(EMU_LIB) or os.path.getmtime(EMU_LIB) < max(os.path.getmtime(s) for s in _emu_sources()):
            subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-DFLTX_EMU", "-ffp-contract=off", "-Wall",
                            "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                            "-Wno-unused-but-set-variable", "-I" + os.path.join(ROOT, "tests", "emu"),
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "text_amd", "csrc"),
                            os.path.join(PRIM, "fltx_prim.cpp"), os.path.join(ROOT, "tests", "emu", "hip_emu.cpp"),
                            "-o", EMU_LIB[:-3] + ".tmp.so", "-lpthread"], check=True)
            os.replace(EMU_LIB[:-3] + ".tmp.so", EMU_LIB)
    return Prim(EMU_LIB, gpu=False)


def _hip_lib_checked():
    import __graft_entry__ as g
    if not os.path.exists(HIP_LIB) or not os.path.exists(HIP_LIB + ".sha"):
        pytest.fail("%s is missing: run __graft_entry__.build()" % HIP_LIB)
    with open(HIP_LIB + ".sha") as f:
        if f.read().strip() != g.prim_digest():
            pytest.fail("%s is stale (its sources or flags changed since it was built): run __graft_entry__.build()" % HIP_LIB)
    return HIP_LIB


@pytest.fixture(scope="module")
def gpu_prim():
    return Prim(_hip_lib_checked(), gpu=True)


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def prim(request):
    return request.getfixturevalue(request.param + "_prim")


def _scale(prim, emu, gpu):
    return gpu if prim.gpu else emu


# ---- order keys (fltx_rt.h) ----------------------------------------------------------------------------------------
def f32key(x):
    """fltx_rt.h f32Key over the bits of float32 array x"""
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def f32_from_key(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def f64key(x):
    b = np.asarray(x, np.float64).view(np.uint64)
    return np.where(b & np.uint64(1 << 63), ~b, b | np.uint64(1 << 63)).astype(np.uint64)


def _special_doubles():
    fi = np.finfo(np.float64)
    return np.array([0.0, -0.0, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, 5e-324, -5e-324, 1e-310, -1e-310,
                     1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)], np.float64)


def test_order_keys(prim):
    """f64Key / f32Key: the round trip is the identity on the bits and the key order is the value order, over finite
    values, subnormals, +-inf and +-0.  Pinned as it is today: key(-0) < key(+0) although -0 == +0 -- the comment's
    `a > b <=> key(a) > key(b)` holds for a != b only.  Every caller that RANKS values which can be -0 therefore
    normalises them first, which was checked caller by caller:
      * float emissions (which can be -0): xlRankBegin keys f32Key(v + 0.0f), wlTokBeamRow's pairwise list keys
        f32Key(v[k] + 0.0f); slRowScan's readlane fallback and wlTokBeamRow's bins compare floats / float distances
        (-0 == +0); the maxima `ek` / `mxKey` only recover the largest value, equal whichever zero wins;
      * f64Key of candidate scores (slRankBin's members, the beams' sort keys, atomMax64 of the frame's best): a score
        is a sum that starts from the root's +0.0 (decodeBegin), and an IEEE sum is -0 only when both terms are -0, so
        no score is -0."""
    rng = np.random.default_rng(11)
    n = _scale(prim, 4096, 65536)
    bits = rng.integers(0, 1 << 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    d = bits.view(np.float64).copy()
    d[np.isnan(d)] = 0.5
    d[:16] = _special_doubles()
    d[16:48] = rng.integers(-4, 5, 32) * 5e-324  # subnormals next to each other and to 0
    fb = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    f = fb.view(np.float32).copy()
    f[np.isnan(f)] = 0.25
    with np.errstate(over="ignore"):
        f[:16] = _special_doubles().astype(np.float32)  # (+-max double -> +-inf)
    f[16:48] = (rng.integers(-4, 5, 32) * 1.4e-45).astype(np.float32)
    k64, k32 = prim.keys(d, f)
    assert np.array_equal(k64[:, 1], d.view(np.uint64)), "f64FromKey(f64Key(x)) is not x"
    assert np.array_equal(k32[:, 1], f.view(np.uint32)), "f32FromKey(f32Key(x)) is not x"
    assert np.array_equal(k64[:, 0], f64key(d)) and np.array_equal(k32[:, 0], f32key(f))
    for vals, keys in ((d, k64[:, 0]), (f.astype(np.float64), k32[:, 0].astype(np.uint64))):
        o = np.argsort(keys, kind="stable")
        vs = vals[o]
        assert np.all(vs[1:] >= vs[:-1]), "key order is not value order"
        same = vs[1:] == vs[:-1]
        ks = keys[o]
        assert np.all(ks[1:][~same] > ks[:-1][~same])
    z = np.array([-0.0, 0.0])
    kz, kzf = prim.keys(z, z.astype(np.float32))
    assert kz[0, 0] < kz[1, 0] and kzf[0, 0] < kzf[1, 0], "key(-0) < key(+0) (pinned)"


# ---- wave primitives (fltx_rt.h) ------------------------------------------------------------------------------------
def test_wave_primitives(prim):
    """waveInclusiveScan, waveMax64 / 32, waveMin64, wavePrefixCount, waveShfl64, waveShflXor64 and waveRowRor64 for
    every R, per lane against numpy, at 0, the 2^63 boundaries and UINT64_MAX (on the GPU the DPP / readlane code that
    ships; on the emulator tests/emu/hip_emu.h's own versions)."""
    rng = np.random.default_rng(12)
    n = _scale(prim, 64, 2048)
    ext = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1, (1 << 32) - 1, 1 << 32, 0x80000000,
                    0x7FFFFFFF], np.uint64)
    v = rng.integers(0, 1 << 64, (n, 64), dtype=np.uint64, endpoint=False)
    for c in range(n):
        kind = c % 6
        if kind == 1:
            v[c] = ext[rng.integers(0, len(ext), 64)]
        elif kind == 2:
            v[c] = ext[c // 6 % len(ext)]  # all equal
        elif kind == 3:
            v[c] = 0
            v[c, rng.integers(0, 64)] = ext[rng.integers(0, len(ext))]
        elif kind == 4:
            v[c] = (1 << 64) - 1
            v[c, rng.integers(0, 64)] = ext[rng.integers(0, len(ext))]
        elif kind == 5:
            v[c] = rng.integers(0, 4, 64).astype(np.uint64) << np.uint64(62)
    src = rng.integers(0, 64, (n, 64)).astype(np.int32)
    src[0::3] = np.arange(64)[::-1]
    mm = np.zeros((n, 2), np.uint64)
    mm[:, 0] = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)
    mm[0::5, 0] = 0
    mm[1::5, 0] = (1 << 64) - 1
    mm[2::5, 0] = np.uint64(1) << rng.integers(0, 64, len(mm[2::5])).astype(np.uint64)
    mm[:, 1] = np.arange(n) % 64
    got = prim.wave(v, src, mm)
    lanes = np.arange(64)
    low31 = (v & np.uint64(0x7FFFFFFF)).astype(np.uint64)
    want_scan = np.cumsum(low31, axis=1) & np.uint64(0xFFFFFFFF)
    masks = mm[:, 0]
    for c in range(n):
        vc = v[c]
        assert np.array_equal(got[c, 0], want_scan[c]), "waveInclusiveScan, configuration %d" % c
        assert np.all(got[c, 1] == vc.max()), "waveMax64, configuration %d" % c
        assert np.all(got[c, 2] == (vc & np.uint64(0xFFFFFFFF)).max()), "waveMax32, configuration %d" % c
        assert np.all(got[c, 3] == vc.min()), "waveMin64, configuration %d" % c
        m = int(masks[c])
        pc = np.array([bin(m & ((1 << l) - 1)).count("1") for l in range(64)], np.uint64)
        assert np.array_equal(got[c, 4], pc), "wavePrefixCount, configuration %d" % c
        assert np.array_equal(got[c, 5], vc[src[c]]), "waveShfl64, configuration %d" % c
        assert np.array_equal(got[c, 6], vc[lanes ^ int(mm[c, 1])]), "waveShflXor64, configuration %d" % c
        for R in range(16):
            want = vc[(lanes & ~15) | ((lanes - R) & 15)]
            assert np.array_equal(got[c, 7 + R], want), "waveRowRor64<%d>, configuration %d" % (R, c)


# ---- slLogAdd -------------------------------------------------------------------------------------------------------
def _logadd_exact(hi, lo):
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        return D(hi) + (D(1) + (D(lo) - D(hi)).exp()).ln()


def test_log_add(prim):
    """slLogAdd(hi, lo) = hi + log1p(exp(lo - hi)) (Utils.h:186-193) against the exact value (50 digits) at the scores a
    decode meets (|hi| >= 1).  Within 1 ulp of the result wherever the result is not smaller than hi in magnitude by
    more than the log term can move it (|hi| >= 2).  Below that the formula's own last step is the limit: the log term
    (up to ln 2) is rounded to an ulp of its own, which can be a whole ulp of a result that cancelled down to ~0.3;
    there the bound is 1 ulp of the result plus 1 ulp of the log term.  Observed on an MI355X (8 192 samples): 1.36
    ulp of the result at hi = -1.01183, lo = -1.01242 (result -0.319), inside that bound.  The special values follow
    the reference's own formula evaluated with the host's libm."""
    rng = np.random.default_rng(13)
    n = _scale(prim, 512, 8192)
    mag = 10.0 ** rng.uniform(0, 5, n)
    hi = np.where(rng.integers(0, 4, n) == 0, mag, -mag)
    delta = np.where(rng.integers(0, 3, n) == 0, 10.0 ** rng.uniform(-17, 0, n), rng.uniform(0, 60, n))
    delta[:8] = 0.0
    lo = hi - delta
    got = prim.logadd(hi, lo)
    worst = {True: (0.0, None), False: (0.0, None)}  # |hi| >= 2: in ulps of the result; else: in units of the bound
    for i in range(n):
        ref = _logadd_exact(hi[i], lo[i])
        err = abs(decimal.Decimal(float(got[i])) - ref)
        strict = abs(hi[i]) >= 2.0
        unit = math.ulp(float(ref)) + (0.0 if strict else math.ulp(float(ref) - hi[i]))
        e = float(err / decimal.Decimal(unit))
        if e > worst[strict][0]:
            worst[strict] = (e, (hi[i], lo[i], got[i], float(ref)))
    assert worst[True][0] <= 1.0, "slLogAdd: worst error %.3f ulp (|hi| >= 2) at (hi, lo, got, exact) = %r" % worst[True]
    assert worst[False][0] <= 1.0, "slLogAdd: worst error %.3f x (ulp + ulp of the log term) at %r" % worst[False]
    # special values: the reference's formula, host libm
    sp_hi = np.array([-3.5, 0.0, -1e300, -7.25, 12.0, -2.0, 1e5, NEG_INF, -0.0])
    sp_lo = np.array([NEG_INF, NEG_INF, NEG_INF, -7.25, 12.0, -2.0 - 746.0, 1e5 - 800.0, NEG_INF, -0.0])
    got = prim.logadd(sp_hi, sp_lo)
    for h, l, g in zip(sp_hi, sp_lo, got):
        want = h + math.log1p(math.exp(l - h)) if not (math.isinf(h) and math.isinf(l)) else float("nan")
        if math.isnan(want):
            assert math.isnan(g), "slLogAdd(%r, %r) = %r, want NaN" % (h, l, g)
        else:
            assert np.float64(g).tobytes() == np.float64(want).tobytes(), "slLogAdd(%r, %r) = %r, want %r" % (h, l, g, want)


# ---- slBin -----------------------------------------------------------------------------------------------------------
def slbin_ref(best, c, shift, base, above):
    d = np.float32(best - c)  # float64 difference, rounded to nearest float32
    if above:
        d = d if d > 0 else np.float32(0.0)
    u = int(np.float32(d).view(np.uint32)) >> shift
    u = u - (1 << 32) if u >= (1 << 31) else u  # (int) of the shifted bits
    q = u - base
    return 0 if q < 0 else min(q, SL_NB - 1)


def test_slbin(prim):
    """slBin<ABOVE>(best, c, shift, base) = the float bits of fl32(best - c) >> shift, minus base, clamped to the window:
    the coarse window (19, 120 << 4) and refined ones, c above best with ABOVE on and off (off: only with shift >= 1, as
    no caller without logAdd has a candidate above the best), c = -inf, distinct doubles of one float distance."""
    rng = np.random.default_rng(14)
    n = _scale(prim, 4096, 65536)
    best = rng.uniform(-5000, 100, n)
    kind = rng.integers(0, 6, n)
    dist = np.where(kind == 0, 10.0 ** rng.uniform(-12, 12, n), rng.uniform(0, 64, n))
    c = best - dist
    c[kind == 2] = best[kind == 2] + 10.0 ** rng.uniform(-8, 3, (kind == 2).sum())  # above the best
    c[kind == 3] = NEG_INF
    # distinct doubles, one float distance: best - c = 1e-3 and 1e-3 plus a few double ulps
    k4 = np.nonzero(kind == 4)[0]
    c[k4] = best[k4] - (1e-3 + rng.integers(0, 64, len(k4)) * 2.0 ** -60)
    shift = np.full(n, 19, np.int32)
    base = np.full(n, 120 << 4, np.int32)
    ref_win = rng.integers(0, 2, n) == 1
    shift[ref_win] = rng.integers(0, 19, ref_win.sum())
    # a refined window around the float bits of the distance (as the bracket of the selection loop would place it)
    dbits = np.float32(np.where(np.isfinite(best - c), np.abs(best - c), 1.0)).view(np.uint32).astype(np.int64)
    base[ref_win] = np.maximum(0, (dbits[ref_win] >> shift[ref_win]) - rng.integers(-300, 300, ref_win.sum()))
    above_off_ok = (kind != 2) | (shift >= 1)
    got = prim.bin(best, c, np.stack([shift, base], 1))
    for i in range(n):
        for above in (0, 1):
            if not above and not above_off_ok[i]:
                continue
            want = slbin_ref(best[i], c[i], int(shift[i]), int(base[i]), above)
            assert got[i, above] == want, "slBin<%d>(%r, %r, %d, %d) = %d, want %d" % (
                above, best[i], c[i], shift[i], base[i], got[i, above], want)


# ---- slScan ----------------------------------------------------------------------------------------------------------
def slscan_ref(hist, K, noFar):
    h = np.array(hist, np.int64)
    if noFar:
        h[SL_NB - 1] = 0
    inc = np.cumsum(h)
    total = int(inc[-1])
    if total < K:
        return (SL_NB - 1, 0, total, total, 0)
    b = int(np.argmax(inc >= K))
    return (b, int(inc[b] - h[b]), int(h[b]), total, 1)


def test_slscan(prim):
    """slScan(hist, K, noFar): the bin of the K-th candidate, the count before it, in it, the total and whether the
    counts reach K -- total below, equal to and above K; K on the first, last and middle member of a bin and at the
    lanes' 4-bin boundaries; bin 255 populated with noFar on and off."""
    rng = np.random.default_rng(15)
    n = _scale(prim, 2048, 32768)
    hist = np.zeros((n, SL_NB), np.uint32)
    kf = np.zeros((n, 2), np.int32)
    for c in range(n):
        kind = c % 5
        if kind == 0:
            h = rng.integers(0, 3, SL_NB) * (rng.uniform(size=SL_NB) < 0.2)
        elif kind == 1:  # few populated bins, some across 4-bin (lane) boundaries
            h = np.zeros(SL_NB, np.int64)
            for b in rng.integers(0, SL_NB, rng.integers(1, 6)):
                h[b] = rng.integers(1, 300)
            for b in (3, 4, 127, 128, 251, 252):
                if rng.uniform() < 0.3:
                    h[b] = rng.integers(1, 5)
        elif kind == 2:  # crowded
            h = rng.integers(0, 16384, SL_NB) * (rng.uniform(size=SL_NB) < 0.02)
        elif kind == 3:
            h = np.zeros(SL_NB, np.int64)
            h[rng.integers(0, SL_NB)] = rng.integers(1, 60000)
        else:
            h = rng.integers(0, 2, SL_NB)
        if rng.uniform() < 0.4:
            h[SL_NB - 1] = rng.integers(1, 500)
        h = np.asarray(h, np.int64)
        nz = np.nonzero(h)[0]
        inc = np.cumsum(h)
        total = int(inc[-1]) if len(h) else 0
        noFar = int(rng.integers(0, 2))
        tot_eff = total - (int(h[-1]) if noFar else 0)
        pick = rng.integers(0, 6)
        if pick == 0 or len(nz) == 0:
            K = int(rng.integers(1, max(2, tot_eff + 3)))
        elif pick == 1:
            K = max(1, tot_eff + int(rng.integers(-1, 2)))  # total - 1, = total, total + 1
        else:  # first / last / middle member of a populated bin
            b = int(nz[rng.integers(0, len(nz))])
            lo = int(inc[b] - h[b])
            K = [lo + 1, int(inc[b]), lo + max(1, int(h[b]) // 2), lo + 1][pick - 2]
        hist[c] = h
        kf[c] = (max(1, K), noFar)
    got = prim.scan(hist, kf)
    for c in range(n):
        want = slscan_ref(hist[c], int(kf[c, 0]), bool(kf[c, 1]))
        assert tuple(int(x) for x in got[c]) == want, "slScan configuration %d (K %d, noFar %d): got %r, want %r" % (
            c, kf[c, 0], kf[c, 1], tuple(got[c]), want)


# ---- slRankBin -------------------------------------------------------------------------------------------------------
def _rank_configs(rng, W, NJ, n):
    """n configurations for one (threads, NJ) pair: cfg [cnt, need, nUsed], member slots and keys, and the reference."""
    nw = W // 64
    cfg = np.zeros((n, 3), np.int32)
    slot = np.zeros((n, SL_BCAP), np.uint32)
    key = np.zeros((n, SL_BCAP), np.uint64)
    want = np.zeros((n, W), np.uint32)
    fixed = [1, 63, 64, 65, 127, 128, 2, 16, 17]
    for c in range(n):
        nUsed = NJ if (NJ == 1 or rng.uniform() < 0.7) else int(rng.integers(1, NJ))  # ylane: `j < nUsed && ...`
        cnt = fixed[c] if c < len(fixed) else int(rng.integers(1, SL_BCAP + 1))
        where = c % 4
        per = nUsed * 64  # member slots of a wave
        if where == 0:  # spread over the workgroup
            ws = np.arange(nw)
        elif where == 1:  # one wave
            ws = np.array([rng.integers(0, nw)])
        elif where == 3:  # the first and the last wave
            ws = np.unique([0, nw - 1])
        if where != 2:
            idx = rng.choice(len(ws) * per, min(cnt, len(ws) * per), replace=False)
            w_, j_, l_ = ws[idx // per], (idx // 64) % nUsed, idx % 64
        else:  # one lane's slots, the rest in one other wave (waves without members at all)
            w, l0, w2 = int(rng.integers(0, nw)), int(rng.integers(0, 64)), int(rng.integers(0, nw))
            pool = np.arange(per)
            if w2 == w:
                pool = pool[pool % 64 != l0]
            rest = rng.choice(pool, min(max(0, cnt - nUsed), len(pool)), replace=False)
            w_ = np.concatenate([np.full(nUsed, w), np.full(len(rest), w2)])[:cnt]
            j_ = np.concatenate([np.arange(nUsed), (rest // 64) % nUsed])[:cnt]
            l_ = np.concatenate([np.full(nUsed, l0), rest % 64])[:cnt]
        w_, j_, l_ = (np.asarray(a_, np.int64) for a_ in (w_, j_, l_))
        perm = rng.permutation(len(w_))
        w_, j_, l_ = w_[perm], j_[perm], l_[perm]
        cnt = len(w_)
        kk = c % 5
        if kk == 0:  # all equal: the publication order (wave, j, lane) alone decides
            keys = np.full(cnt, rng.integers(0, 1 << 64, dtype=np.uint64, endpoint=False), np.uint64)
        elif kk == 1:  # equal high halves, low halves with and without bit 31
            hi_ = np.uint64(rng.integers(0, 1 << 32)) << np.uint64(32)
            keys = hi_ | rng.choice(np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF], np.uint64), cnt)
        elif kk == 2:  # few distinct values
            keys = rng.choice(rng.integers(0, 1 << 64, 3, dtype=np.uint64, endpoint=False), cnt)
        elif kk == 3:  # candidate scores of one bin: order keys of nearby doubles
            keys = f64key(-100.0 - rng.integers(0, 8, cnt) * 2.0 ** -40)
        else:
            keys = rng.integers(0, 1 << 64, cnt, dtype=np.uint64, endpoint=False)
        need = int(rng.choice([1, cnt, max(1, cnt - 1), int(rng.integers(1, cnt + 1))]))
        cfg[c] = (cnt, need, nUsed)
        slot[c, :cnt] = (w_ * NJ + j_) * 64 + l_
        key[c, :cnt] = keys
        ordv = (w_ << 16) | (j_ << 8) | l_
        order = np.lexsort((ordv, ~np.asarray(keys, np.uint64)))  # key descending, then ord ascending
        for i in order[:need]:
            want[c, w_[i] * 64 + l_[i]] |= np.uint32(1 << int(j_[i]))
    return cfg, slot, key, want


def _check_rank(prim, W, NJ, spill, n, seed):
    cfg, slot, key, want = _rank_configs(np.random.default_rng(seed), W, NJ, n)
    got = prim.rank(W, NJ, spill, cfg, slot, key)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        c = int(bad[0])
        t = int(np.nonzero(got[c] != want[c])[0][0])
        raise AssertionError("slRankBin<%d> (%d threads%s): %d of %d configurations wrong; first: cnt %d need %d nUsed "
                             "%d, thread %d take %#x, want %#x" % (NJ, W, ", SGPR pressure" if spill else "", len(bad), n,
                                                                   cfg[c, 0], cfg[c, 1], cfg[c, 2], t, got[c, t],
                                                                   want[c, t]))


def test_rank_bin(prim):
    """slRankBin<NJ> for every (threads, NJ) pair a caller compiles (slane / tlane, mlane / tmlane, xlane, ylane, and
    wlane's geometries): members published by atomAdd in arbitrary order with ord = wave << 16 | j << 8 | lane, as the
    callers publish them; `take` bit j set iff the candidate is among the `need` first by (key descending, ord
    ascending).  cnt 1 .. kSlBCap, members in one wave, one lane, spread, waves without any; equal keys, keys equal in
    the high half, low halves with bit 31 set; the ylane predicate `j < nUsed && ...`."""
    pairs = sorted(set(prim.rank_pairs()))
    assert {(576, 4), (512, 12), (960, 22), (768, 6), (512, 3), (1024, 4), (576, 8)} <= set(pairs)
    n = _scale(prim, 40, 2000)
    for i, (W, NJ) in enumerate(pairs):
        _check_rank(prim, W, NJ, 0, n, 1000 + i)


def test_rank_bin_under_sgpr_pressure(prim):
    """the same for a kernel whose scalar registers are cut to 24 (amdgpu_num_sgpr): slRankBin's broadcast loop runs
    with SGPR spills, the nearest cheap stand-in for fltx_wlane.h's frame loop (460 SGPRs spilled), where slRankBin once
    returned wrong survivors for token beams of 64.  (On the emulator: the same body.)"""
    _check_rank(prim, 576, 10, 1, _scale(prim, 24, 4000), 77)


def test_rank_bin_spill_variant_spills():
    """The SGPR-pressure kernel in the built library really spills scalar registers (its code object's metadata), so it
    cannot silently stop standing in for the spilling kernels after a compiler update."""
    lib = _hip_lib_checked()
    llvm = "/opt/rocm/llvm/bin"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fb, dev = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.o")
        subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fb, lib], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + dev], check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", dev], check=True, stdout=subprocess.PIPE,
                               text=True).stdout
    spills = {}
    name = None
    for line in notes.splitlines():
        s = line.strip()
        if s.startswith(".name:"):
            name = s.split(":", 1)[1].strip()
        elif s.startswith(".sgpr_spill_count:") and name:
            spills[name] = int(s.split(":", 1)[1])
    sp = [v for k, v in spills.items() if "prim_rank_spill_kernel" in k]
    assert sp, "no SGPR-pressure kernel in %s" % lib
    assert sp[0] > 0, "the SGPR-pressure slRankBin kernel no longer spills"
    plain = [v for k, v in spills.items() if "prim_rank_kernelILi576ELi10E" in k]
    assert plain and plain[0] == 0, "the plain (576, 10) kernel spills: %r" % plain


# ---- slRowScan -------------------------------------------------------------------------------------------------------
def rowscan_ref(v, N, Kt, sil, blank, ctc, mmax, silScore):
    x = np.asarray(v[:N], np.float32)
    if Kt >= N:
        allow = (1 << N) - 1
    elif np.isnan(x).any():  # the readlane fallback, as written: lanes ranked by (o > v || (o == v && m < lane))
        allow = 0
        for l in range(N):
            r = sum(1 for m in range(N) if x[m] > x[l] or (x[m] == x[l] and m < l))
            if r < Kt:
                allow |= 1 << l
    else:  # the Kt largest, ties to the lower index, -0 == +0
        order = np.lexsort((np.arange(N), -(x.astype(np.float64) + 0.0)))
        allow = sum(1 << int(i) for i in order[:Kt])
    keys = [int(f32key(x[l])) for l in range(N) if (allow >> l) & 1 and l != sil and x[l] == x[l]]
    ek = max(keys) if keys else 0
    lm = allow & ~(1 << blank) if ctc else allow
    esil = np.float32(v[sil])
    best, anyc = 0.0, False
    if ek:
        best = float(np.float64(mmax) + np.float64(f32_from_key(np.uint32(ek))))
        anyc = True
    if (allow >> sil) & 1:
        sS = float((np.float64(mmax) + np.float64(esil)) + np.float64(silScore))
        if sS == sS and (not anyc or sS > best):
            best, anyc = sS, True
    dead = (not anyc) or not (best - best == 0.0)
    return allow, lm, best, ek, bin(lm).count("1"), int(dead), int(esil.view(np.uint32))


def _row_configs(rng, n):
    cfg = np.zeros((n, 5), np.int32)
    sc = np.zeros((n, 2), np.float64)
    rows = np.full((n, 64), 3.0e38, np.float32)  # (the lanes past N must not matter)
    for c in range(n):
        N = 1 + c % 64 if c < 64 * 8 else int(rng.integers(1, 65))
        Kt = int(rng.integers(1, N)) if N > 1 and rng.uniform() < 0.9 else int(rng.integers(N, N + 3))
        kind = (c // 64) % 8
        if kind == 0:
            x = rng.normal(-5, 3, N)
        elif kind == 1:  # heavily quantised: many ties at the cut
            x = np.round(rng.normal(-3, 1.5, N) * 2) / 2
        elif kind == 2:  # +-0 at the cut
            x = rng.choice([0.0, -0.0, -1.0, 1.0], N)
        elif kind == 3:
            x = rng.normal(-5, 3, N)
            x[rng.uniform(size=N) < 0.4] = NEG_INF
        elif kind == 4:
            x = np.full(N, NEG_INF)
        elif kind == 5:  # NaN: the fallback
            x = np.round(rng.normal(-3, 1.5, N))
            x[rng.integers(0, N, 1 + N // 16)] = np.nan
        elif kind == 6:
            x = np.full(N, rng.choice([-2.5, 0.0, -0.0]))
        else:
            x = rng.choice([-1.0, -2.0, -0.0, 0.0, NEG_INF], N)
        sil, blank = int(rng.integers(0, N)), int(rng.integers(0, N))
        if rng.uniform() < 0.3:
            x[sil] = np.max(np.where(np.isnan(x), -1e9, x)) + rng.choice([0.0, 1.0])  # sil in the beam
        ctc = int(rng.integers(0, 2))
        mmax = float(rng.choice([0.0, -37.25, rng.normal(-100, 30)]))
        silScore = float(rng.choice([0.0, -2.0, 50.0, 1e3]))  # 50 / 1e3: sil the best
        cfg[c] = (N, Kt, sil, blank, ctc)
        sc[c] = (mmax, silScore)
        rows[c, :N] = x
    return cfg, sc, rows


def test_row_scan(prim):
    """slRowScan: the token beam `allow` (the Kt largest, ties to the lower index, -0 == +0: N <= 32 through the
    all-pairs xlRank path, N > 32 through readlanes, rows with NaN through the fallback), listMask, nList, the frame's
    best candidate, ekey and dead as stated at its definition -- sil in and out of the beam, blank with and without
    CTC, silScore making sil the best; quantised rows, +-0, -inf and all -inf rows."""
    n = _scale(prim, 64 * 8 + 256, 64 * 8 + 8192)
    cfg, sc, rows = _row_configs(np.random.default_rng(16), n)
    got = prim.rowscan(cfg, sc, rows)
    names = ("allow", "listMask", "best", "ekey", "nList", "dead", "esil")
    for c in range(n):
        N, Kt, sil, blank, ctc = (int(x) for x in cfg[c])
        want = rowscan_ref(rows[c], N, Kt, sil, blank, bool(ctc), sc[c, 0], sc[c, 1])
        g = [int(x) for x in got[c]]
        wb = int(np.float64(want[2]).view(np.uint64))
        want = list(want)
        want[2] = wb
        for i, nm in enumerate(names):
            if nm == "best" and want[5]:
                continue  # (dead: best is not read)
            assert g[i] == want[i], "slRowScan configuration %d (N %d Kt %d sil %d blank %d ctc %d row %r): %s %#x, want %#x" % (
                c, N, Kt, sil, blank, ctc, rows[c, :N].tolist(), nm, g[i], want[i])


# ---- wlTokBeamRows ----------------------------------------------------------------------------------------------------
def tokbeam_ref(x, Kt, ctc, blank, sil):
    """the WlTokRow of a row, or None when the row cannot be cut (flags bit 1; the other fields unspecified): a NaN, no
    value above -inf, or more than kSlBCap values sharing the float32 distance rowMax - x at the cut."""
    x = np.asarray(x, np.float32)
    Kt = min(Kt, 64)
    if np.isnan(x).any():
        return None
    cand = np.nonzero(x > -np.inf)[0]
    if len(cand) == 0:
        return None
    vals = x[cand].astype(np.float64) + 0.0
    order = cand[np.lexsort((cand, -vals))]
    sel = np.sort(order[:Kt])
    if len(cand) > Kt:
        rowMax = np.float32(x[cand].max())
        d = (rowMax - x[cand]).astype(np.float32)  # float32 arithmetic, as the kernel's bins
        dstar = np.float32(rowMax - x[order[Kt - 1]])
        n_eq = int((d == dstar).sum())
        n_less = int((d < dstar).sum())
        if n_eq > SL_BCAP and n_less + n_eq != Kt:
            return None
    listed = [int(t) for t in sel if not (ctc and t == blank)]
    sl = set(int(t) for t in sel)
    ks = [int(f32key(x[t])) for t in sel if t != sil]
    return dict(tok=listed, e=x[listed], nList=len(listed), eBlank=(x[blank] if ctc and blank in sl else None),
                silIn=sil in sl, eSil=x[sil], silPos=(listed.index(sil) if sil in listed else -4096),
                ek=max(ks) if ks else 0)


def _tok_rows(rng, N, Kt, nrows):
    rows = []
    kinds = ["normal", "quant", "tie16", "tie17", "tie128", "tie129", "far", "subnormal", "equal", "neginf", "collapse",
             "collapse_fine", "nan", "allneginf", "zeros"]
    for r in range(nrows):
        k = kinds[r % len(kinds)]
        x = rng.normal(-8, 3, N)
        if k == "quant":
            x = np.round(x * 2) / 2
        elif k.startswith("tie"):  # m equal values straddling the cut (kWlPairwise 16 / 17, kSlBCap 128 / 129)
            m = min(int(k[3:]), N)
            above = int(rng.integers(max(0, Kt - m + 1), Kt)) if Kt > 0 else 0
            above = min(above, N - m)
            x = rng.uniform(-30, -20, N)
            idx = rng.permutation(N)
            x[idx[:above]] = rng.uniform(0, 5, above)
            x[idx[above:above + m]] = -10.0
        elif k == "far":  # values 1e30 apart: the cut in the far bin
            x = -1e30 * rng.integers(1, 4, N).astype(np.float64) - rng.uniform(0, 1e29, N)
            x[rng.integers(0, N, max(1, Kt // 2))] = rng.uniform(-1, 0)
        elif k == "subnormal":
            x = rng.integers(-200, 200, N) * 1.4e-45
        elif k == "equal":
            x = np.full(N, -3.0)
        elif k == "neginf":
            x[rng.uniform(size=N) < 0.97] = NEG_INF
        elif k == "collapse":  # |rowMax| >> the differences: distinct values share one float distance
            x = rng.uniform(-1, 1, N)
            x[rng.integers(0, N)] = 3e7
        elif k == "collapse_fine":
            x = rng.uniform(-1, 1, N)
            x[rng.integers(0, N)] = 3e5
        elif k == "nan":
            x[rng.integers(0, N)] = np.nan
        elif k == "allneginf":
            x = np.full(N, NEG_INF)
        elif k == "zeros":
            x = rng.choice([0.0, -0.0, -1.0], N)
        rows.append(np.asarray(x, np.float32))
    return np.stack(rows)


TOK_N = (65, 100, 1023, 1024, 1025, 4096, 8192, 16384)
TOK_KT = (1, 2, 16, 17, 50, 63, 64)


def _check_tokbeam(prim, N, Kt, rows, criterion, blank, sil, what):
    B = 2
    T = len(rows) // B
    got = prim.tokbeam(rows.reshape(B, T, N), Kt, criterion, blank, sil)
    ctc = criterion == 1
    for r in range(B * T):
        g = got[r]
        want = tokbeam_ref(rows[r], Kt, ctc, blank, sil)
        where = "%s: N %d Kt %d row %d (blank %d sil %d ctc %d)" % (what, N, Kt, r, blank, sil, ctc)
        if want is None:
            assert g["flags"] & 2, "%s: the row cannot be cut, flags %#x" % (where, g["flags"])
            continue
        assert not g["flags"] & 2, "%s: flagged as not cuttable" % where
        nl = want["nList"]
        assert g["nList"] == nl, "%s: nList %d, want %d" % (where, g["nList"], nl)
        assert g["tok"][:nl].tolist() == want["tok"], "%s: tokens %r, want %r" % (where, g["tok"][:nl].tolist(), want["tok"])
        assert g["e"][:nl].view(np.uint32).tolist() == want["e"].view(np.uint32).tolist(), "%s: emissions" % where
        if want["eBlank"] is None:
            assert np.isnan(g["eBlank"]), "%s: eBlank %r, want NaN" % (where, g["eBlank"])
        else:
            assert np.float32(g["eBlank"]).view(np.uint32) == np.float32(want["eBlank"]).view(np.uint32), where
        assert bool(g["flags"] & 1) == want["silIn"], "%s: flags %#x" % (where, g["flags"])
        if want["silIn"]:
            assert np.float32(g["eSil"]).view(np.uint32) == np.float32(want["eSil"]).view(np.uint32), "%s: eSil" % where
        assert g["silPos"] == want["silPos"], "%s: silPos %d, want %d" % (where, g["silPos"], want["silPos"])
        assert g["ek"] == want["ek"], "%s: ek %#x, want %#x" % (where, g["ek"], want["ek"])


def test_tok_beam_rows(prim):
    """wlTokBeamRows, launched as fltx_api.cpp launches it, against the contract of WlTokRow: the Kt largest (ties to
    the lower token, -0 == +0, never -inf) in token order without blank, eBlank NaN unless blank is in the beam, ek the
    key of the largest in the beam other than sil's, silPos and flags bit 0; flags bit 1 exactly for a NaN, a row
    without a value above -inf, or more than kSlBCap values of one float32 distance at the cut.  Ties straddling the
    cut with 16 / 17 (kWlPairwise) and 128 / 129 members, values 1e30 apart, subnormals, equal rows, values whose
    distances collapse under a large row maximum."""
    rng = np.random.default_rng(17)
    Kts = TOK_KT if prim.gpu else (1, 16, 17, 50, 64)
    nrows = 30 if prim.gpu else 16
    for N in TOK_N:
        for Kt in Kts:
            criterion = int(rng.integers(0, 2))
            blank, sil = int(rng.integers(0, N)), int(rng.integers(0, N))
            if rng.uniform() < 0.15:
                sil = blank
            rows = _tok_rows(rng, N, Kt, nrows)
            for r in range(0, nrows, 3):  # blank / sil among the largest of some rows
                if np.isfinite(rows[r]).any():
                    rows[r, [blank, sil][r % 2]] = np.nanmax(np.where(np.isfinite(rows[r]), rows[r], -np.inf))
            _check_tokbeam(prim, N, Kt, rows, criterion, blank, sil, prim.name)


def test_tok_beam_row_of_equal_values(prim):
    """The row of test_word_piece_row_without_a_defined_token_beam (300 equal values, Kt 30): the reference flags it,
    and so does the kernel -- the utterance goes to the general engines; 128 equal values are ranked instead."""
    x = np.full((2, 300), -3.0, np.float32)
    assert tokbeam_ref(x[0], 30, True, 0, 1) is None
    y = np.full(300, -20.0, np.float32)
    y[:128] = -3.0
    assert tokbeam_ref(y, 30, True, 0, 1)["tok"] == list(range(1, 30))
    _check_tokbeam(prim, 300, 30, np.stack([x[0], y, x[1], y]), 1, 0, 1, prim.name)
