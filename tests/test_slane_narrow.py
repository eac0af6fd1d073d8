"""The lane = LM state engine (slaneUtterance, fltx_slane.h) with token masks of 32 bits where the token set has at most
32 tokens (the M32 instantiations), and with a token wave's lane prefix counts computed in its build -- which most token
wave-frames do not run -- instead of in every frame.  Neither may change a result: every n-best is compared bit for bit
with the oracle, on the emulator and (`-m gpu`) on the device, at 512 and at 576 threads.

fltx_decoder_get "engine", "redone", "threads" and "slane_m32" say which path a batch took, so that no case passes on
the other kernel: N = 29, 31, 32 must run the 32-bit kernel, N = 33 and 64 the 64-bit one; logAdd and the token-LM
variant keep 64-bit masks.  At N = 32 under ASG nothing is left out of the list: bit 31 is a listed token, and a state's
last token can be 31.

The far-bin case: the histogram counts the candidates beyond its window only when the window holds fewer than the beam
(`slScan` not crossed).  The phase-clock instantiation counts those frames (1e6 each in slot 6 of the profile), which is
how the case proves that it reaches the path -- on the emulator as on the device."""
import functools

import numpy as np
import pytest

import cases
import engine_choices as ec
import helpers
from oracle import orclib
from text_amd import _capi

WHERE = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
THREADS = [512, 576]


@pytest.fixture(params=WHERE)
def sess(request):
    return request.getfixturevalue("emu_session" if request.param == "emu" else "gpu_session")


def _lf(N=29, K=10, T=40, Kt=None, crit="ctc", sil_score=0.0, dist="ctc", la=False, lm="zero", u=0, thr=25.0):
    return cases.case("sn", dist=dist, T=T, N=N, K=K, Kt=Kt, crit=crit, sil_score=sil_score, log_add=la, lm=lm, u=u,
                      thr=thr, trans_seed=(31 + u % 5) if crit == "asg" else None,
                      lm_weight=0.8 if lm != "zero" else 0.0)


def _blank(c):
    return c["N"] - 1 if c["crit"] == "ctc" else -1


@functools.lru_cache(maxsize=None)
def _inputs_of(key):
    return helpers.case_inputs(dict(key))


def _inputs(c):
    return _inputs_of(tuple(sorted(c.items())))


_WANT = {}


def _want(oracle_lib, c, sil, e=None, tag=None):
    """the oracle's n-best of case c with sil at index `sil` (over the emissions `e`, named `tag`, when given) --
    computed once, shared by the thread counts and by emulator and device"""
    key = (tuple(sorted(c.items())), sil, tag)
    if key not in _WANT:
        inp = _inputs(c)
        opt = orclib.make_options(c["K"], c["Kt"], c["thr"], c["lm_weight"], c["word_score"], c["unk_score"],
                                  c["sil_score"], c["log_add"], c["crit"])
        lm = helpers.checker_lm(oracle_lib, c, inp)
        try:
            dec = oracle_lib.lexfree(opt, lm, sil, _blank(c), inp["tr"])
            _WANT[key] = oracle_lib.decode(dec, inp["e"] if e is None else e, c["T"], c["N"])
            oracle_lib.decoder_destroy(dec)
        finally:
            oracle_lib.lm_destroy(lm)
    return _WANT[key]


def _decoder(sess, c, sil, threads):
    inp = _inputs(c)
    opt = _capi.make_options(c["K"], c["Kt"], c["thr"], c["lm_weight"], c["word_score"], c["unk_score"],
                             c["sil_score"], c["log_add"], c["crit"])
    d = _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, opt, sess.lm_for(c, inp), sil, _blank(c), transitions=inp["tr"])
    d.set("slane_threads", threads)
    return d


def _path(d):
    return {k: int(d.get(k)) for k in ("engine", "redone", "why_not_lane", "threads", "tlane", "slane_m32")}


def _m32_of(c):
    return 1 if c["N"] <= 32 and not c["log_add"] and c["lm"] == "zero" else 0


def _check(sess, oracle_lib, c, threads, sil=0, tol=0.0, tlane=0, e=None, tag=None, profile=False):
    """decode case c on the lane engine at `threads` threads -> compared with the oracle, the path asserted; -> the
    profile slots when asked for"""
    d = _decoder(sess, c, sil, threads)
    if profile:
        d.set("profile", 1)
    d.decode_batch(_inputs(c)["e"] if e is None else e, [c["T"]], c["N"])
    got, path = d.results(0), _path(d)
    prof = d.profile() if profile else None
    d.close()
    what = "N %d K %d Kt %d T %d %s %s sil %d silScore %g threads %d" % (
        c["N"], c["K"], c["Kt"], c["T"], c["crit"], c["dist"], sil, c["sil_score"], threads)
    assert path["engine"] == 4 and path["redone"] == 0 and path["why_not_lane"] == 0, (what, path)
    assert path["threads"] == threads and path["tlane"] == tlane, (what, path)
    assert path["slane_m32"] == _m32_of(c), (what, path)
    ok, why = helpers.hyps_equal(_want(oracle_lib, c, sil, e, tag), got, score_tol=tol)
    assert ok, "%s: %s" % (what, why)
    return prof


# ---- which kernel a token set runs, over the beams ---------------------------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("K", [1, 10, 50, 64])
@pytest.mark.parametrize("N", [29, 31, 32, 33, 64])
def test_ctc_by_token_set_and_beam(sess, oracle_lib, N, K, threads):
    """N = 29, 31, 32: 32-bit masks; 33 and 64: 64-bit masks (asserted in _check)"""
    _check(sess, oracle_lib, _lf(N, K, 40, u=N + K), threads)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("K", [10, 64])
@pytest.mark.parametrize("N", [29, 32, 33])
def test_asg_by_token_set(sess, oracle_lib, N, K, threads):
    """no blank: all N tokens are listed; at N = 32 token 31 is listed, and is the last token of states in the beam
    (asserted from the oracle's n-best: some hypothesis holds token 31)"""
    c = _lf(N, K, 40, crit="asg", dist="uniform", u=N)
    # the last token of the set wins frames 5, 6 (a repeat of it) and 20: the `uniform` rows are below zero
    e = np.asarray(_inputs(c)["e"], dtype=np.float32).reshape(-1)[:40 * N].copy()
    e.reshape(40, N)[[5, 6, 20], N - 1] = 0.0
    if N == 32:
        assert any(31 in [int(t) for t in h.tokens] for h in _want(oracle_lib, c, 0, e, "last-token")), "token 31 never decoded"
    _check(sess, oracle_lib, c, threads, e=e, tag="last-token")


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N,crit", [(29, "ctc"), (32, "ctc"), (32, "asg"), (33, "ctc")])
def test_token_beam_of_ten(sess, oracle_lib, N, crit, threads):
    """Kt = 10 < N: the list is made per frame"""
    _check(sess, oracle_lib, _lf(N, 10, 40, Kt=10, crit=crit, sil_score=-0.7, u=3), threads)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N,crit,sils", [(29, "ctc", (0, 14, 27)), (32, "asg", (0, 16, 31)), (64, "ctc", (0, 31, 62))])
def test_sil_score_at_the_first_a_middle_and_the_last_listed_index(sess, oracle_lib, N, crit, sils, threads):
    for sil in sils:
        _check(sess, oracle_lib, _lf(N, 10, 40, crit=crit, sil_score=-0.7, u=N + 1), threads, sil)


# ---- the lane prefix counts in the build ---------------------------------------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N", [29, 33])
def test_many_token_waves_build_in_a_frame(sess, oracle_lib, N, threads):
    """near-flat rows, beam 64: new states in most token waves of most frames"""
    _check(sess, oracle_lib, _lf(N, 64, 40, dist="uniform", u=64), threads)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N", [29, 33])
def test_most_token_waves_build_nothing(sess, oracle_lib, N, threads):
    """the benchmark's distribution: the new states of a frame sit in very few waves"""
    _check(sess, oracle_lib, _lf(N, 50, 40, dist="ctc", u=50), threads)


@pytest.mark.parametrize("threads", THREADS)
def test_ragged_batch(sess, oracle_lib, threads):
    """T = 0, 1, 2, 41 in one batch: no frame, one frame of either parity, the odd tail frame"""
    c0 = _lf(29, 10, 41, sil_score=-0.7, u=21)
    cs = [dict(c0, T=T, u=21 + i) for i, T in enumerate((0, 1, 2, 41))]
    e = np.concatenate([np.asarray(_inputs(c)["e"], dtype=np.float32).reshape(-1)[:c["T"] * 29] for c in cs])
    d = _decoder(sess, c0, 0, threads)
    d.decode_batch(e, [c["T"] for c in cs], 29)
    path = _path(d)
    assert path["engine"] == 4 and path["redone"] == 0 and path["slane_m32"] == 1 and path["threads"] == threads, path
    for b, c in enumerate(cs):
        ok, why = helpers.hyps_equal(_want(oracle_lib, c, 0), d.results(b), score_tol=0.0)
        assert ok, "utterance %d (T = %d): %s" % (b, c["T"], why)
    d.close()


# ---- fewer than K candidates inside the window: the far bin is counted ---------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N", [29, 33])
def test_far_bin_is_counted(sess, oracle_lib, N, threads):
    """rows sixty times as wide as `uniform`'s (emissions down to -600), beam 64, a threshold nothing fails: most
    candidates lie beyond the two octaves of the window, which then holds fewer than 64 -- the frames that count the far
    bin are counted by the phase-clock instantiation (1e6 each in slot 6)"""
    c = _lf(N, 64, 40, dist="uniform", u=7, thr=1e9)
    e = (np.asarray(_inputs(c)["e"], dtype=np.float32) * np.float32(60.0)).astype(np.float32)
    prof = _check(sess, oracle_lib, c, threads, e=e, tag="x60", profile=True)
    assert int(prof[6]) // 1000000 >= 1, prof


# ---- one utterance through the fallback ----------------------------------------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
def test_all_nan_row_in_a_batch_of_three(sess, oracle_lib, threads):
    """the middle utterance has a row of nothing but NaN: it comes back through the generic engine (compared with a
    decode on that engine alone), the other two untouched (compared with the oracle)"""
    c0 = _lf(29, 10, 40, sil_score=-0.7, u=31)
    cs = [dict(c0, u=31 + i) for i in range(3)]
    rows = [np.asarray(_inputs(c)["e"], dtype=np.float32).reshape(-1)[:40 * 29].copy() for c in cs]
    rows[1].reshape(40, 29)[20, :] = np.nan
    e = np.concatenate(rows)
    d = _decoder(sess, c0, 0, threads)
    d.decode_batch(e, [40, 40, 40], 29)
    path = _path(d)
    assert path["engine"] == 4 and path["redone"] >= 1 and path["slane_m32"] == 1, path
    g = _decoder(sess, c0, 0, 0)
    for k in ("slane", "lane", "lean"):
        g.set(k, 0)
    g.decode_batch(e, [40, 40, 40], 29)
    assert g.get("engine") not in (3, 4), g.get("engine")
    for b, c in enumerate(cs):
        want = g.results(b) if b == 1 else _want(oracle_lib, c, 0)
        ok, why = helpers.hyps_equal(want, d.results(b), score_tol=0.0)
        assert ok, "utterance %d: %s" % (b, why)
    d.close()
    g.close()


# ---- the instantiations that share the frame's text and keep 64-bit masks ------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("sil,sil_score", [(0, 0.0), (27, -0.7)])
def test_log_add(sess, oracle_lib, sil, sil_score, threads):
    """(1e-5: log1p / exp differ by a few ulp between the device's library and the host's, as in every logAdd
    comparison of the suite)"""
    _check(sess, oracle_lib, _lf(29, 10, 40, sil_score=sil_score, la=True, u=1), threads, sil, tol=1e-5)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("K", [10, 50])
def test_token_lm(sess, oracle_lib, K, threads):
    _check(sess, oracle_lib, _lf(29, K, 40, sil_score=-0.7, lm=ec.TOK_LM, u=K), threads, tlane=1)
