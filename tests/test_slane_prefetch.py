"""The lane = LM state engine (slaneUtterance, fltx_slane.h) with the next frame's row fetched behind the second barrier
of the frame before (best, thr, a token wave's emissions, the own-groups wave's blank emission and token beam: handed
from frame to frame in registers), and with a token wave's part of the token list read once where a full token beam makes
it the same in every frame.  Neither may change a result: every n-best is compared bit for bit with the oracle, on the
emulator and (`-m gpu`) on the device, at 512 and at 576 threads.

What a stale or misplaced fetch would break, and the case that would show it:
  * the first frame takes the prologue's row, the two parities hand over to each other, the last frame's fetch finds no
    staged row and must never be used: T = 1, 2, 3, 39, 40, and a ragged batch;
  * a list that changes from frame to frame (token beam of 5 and 10: positions past the list are padded, the list is one
    shorter when blank is in the token beam, sil moves its list position) beside the constant list (full token beam) on
    the same emissions; N = 33 and 64 run the 64-bit kernel, which fetches ahead and keeps no list;
  * `dead` (a row without a candidate) returns early with a fetch in flight: the row of NaN sits in the first frame that
    was handed its row, in a frame of either parity and in the last frame;
  * the frames after a re-entry reload records and masks, not the row.
fltx_decoder_get "engine", "redone", "threads", "slane_m32" and "tlane" say which path a batch took.  logAdd, the token-LM
variant and the two stream variants keep their reads where they were and must be unchanged.  Tune bit 1 makes a token
wave read its list in every frame whatever the token beam: one case decodes with either setting."""
import functools

import numpy as np
import pytest

import cases
import engine_choices as ec
import helpers
import stream_scenarios as ss
from oracle import orclib
from text_amd import _capi

WHERE = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
THREADS = [512, 576]


@pytest.fixture(params=WHERE)
def sess(request):
    return request.getfixturevalue("emu_session" if request.param == "emu" else "gpu_session")


def _lf(N=29, K=10, T=40, Kt=None, crit="ctc", sil_score=0.0, dist="ctc", la=False, lm="zero", u=0, thr=25.0):
    return cases.case("sp", dist=dist, T=T, N=N, K=K, Kt=Kt, crit=crit, sil_score=sil_score, log_add=la, lm=lm, u=u,
                      thr=thr, trans_seed=(31 + u % 5) if crit == "asg" else None,
                      lm_weight=0.8 if lm != "zero" else 0.0)


def _blank(c):
    return c["N"] - 1 if c["crit"] == "ctc" else -1


@functools.lru_cache(maxsize=None)
def _inputs_of(key):
    return helpers.case_inputs(dict(key))


def _inputs(c):
    return _inputs_of(tuple(sorted(c.items())))


def _rows(c, T=None):
    T = c["T"] if T is None else T
    return np.asarray(_inputs(c)["e"], dtype=np.float32).reshape(-1)[:T * c["N"]].copy()


_WANT = {}


def _want(oracle_lib, c, sil, e=None, tag=None):
    """the oracle's n-best of case c with sil at index `sil` (over the emissions `e`, named `tag`, when given) --
    computed once, shared by the thread counts and by emulator and device, and left unchanged"""
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


def _decoder(sess, c, sil, threads, tune=0):
    inp = _inputs(c)
    opt = _capi.make_options(c["K"], c["Kt"], c["thr"], c["lm_weight"], c["word_score"], c["unk_score"],
                             c["sil_score"], c["log_add"], c["crit"])
    d = _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, opt, sess.lm_for(c, inp), sil, _blank(c), transitions=inp["tr"])
    d.set("slane_threads", threads)
    if tune:
        d.set("tune", tune)
    return d


def _path(d):
    return {k: int(d.get(k)) for k in ("engine", "redone", "why_not_lane", "threads", "tlane", "slane_m32")}


def _m32_of(c):
    return 1 if c["N"] <= 32 and not c["log_add"] and c["lm"] == "zero" else 0


def _check(sess, oracle_lib, c, threads, sil=0, tol=0.0, tlane=0, e=None, tag=None, profile=False, tune=0):
    """decode case c on the lane engine at `threads` threads -> compared with the oracle, the path asserted; -> the
    n-best and the profile slots (when asked for)"""
    d = _decoder(sess, c, sil, threads, tune)
    if profile:
        d.set("profile", 1)
    d.decode_batch(_inputs(c)["e"] if e is None else e, [c["T"]], c["N"])
    got, path = d.results(0), _path(d)
    prof = d.profile() if profile else None
    d.close()
    what = "N %d K %d Kt %d T %d %s %s sil %d silScore %g threads %d tune %d" % (
        c["N"], c["K"], c["Kt"], c["T"], c["crit"], c["dist"], sil, c["sil_score"], threads, tune)
    assert path["engine"] == 4 and path["redone"] == 0 and path["why_not_lane"] == 0, (what, path)
    assert path["threads"] == threads and path["tlane"] == tlane, (what, path)
    assert path["slane_m32"] == _m32_of(c), (what, path)
    ok, why = helpers.hyps_equal(_want(oracle_lib, c, sil, e, tag), got, score_tol=tol)
    assert ok, "%s: %s" % (what, why)
    return got, prof


# ---- the first frame, the hand-over between the parities, the last frame -------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("T", [1, 2, 3, 39, 40])
@pytest.mark.parametrize("N", [29, 33])
def test_short_utterances(sess, oracle_lib, N, T, threads):
    """T = 1: the prologue's row alone; 2, 3: one hand-over each way; 39 / 40: the odd tail frame / the unrolled pair is
    the last to run, and what it fetched (no row was staged for frame T) is not used by decodeEnd"""
    _check(sess, oracle_lib, _lf(N, 50, T, sil_score=-0.7, u=T), threads, sil=3)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N", [29, 33])
def test_ragged_batch(sess, oracle_lib, N, threads):
    """T = 1, 2, 7, 40 in one batch"""
    c0 = _lf(N, 10, 40, sil_score=-0.7, u=21)
    cs = [dict(c0, T=T, u=21 + i) for i, T in enumerate((1, 2, 7, 40))]
    e = np.concatenate([_rows(c) for c in cs])
    d = _decoder(sess, c0, 0, threads)
    d.decode_batch(e, [c["T"] for c in cs], N)
    path = _path(d)
    assert path["engine"] == 4 and path["redone"] == 0 and path["threads"] == threads, path
    assert path["slane_m32"] == _m32_of(c0) and path["tlane"] == 0, path
    for b, c in enumerate(cs):
        ok, why = helpers.hyps_equal(_want(oracle_lib, c, 0), d.results(b), score_tol=0.0)
        assert ok, "utterance %d (T = %d): %s" % (b, c["T"], why)
    d.close()


# ---- a list that changes every frame beside the constant list, on the same emissions ---------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N", [29, 31, 32, 33, 64])
def test_token_beam_of_five_ten_and_all_on_the_same_rows(sess, oracle_lib, N, threads):
    """Kt = 5, 10: the list is made per frame (positions past it are padded, it is one shorter in the frames whose
    token beam holds blank, sil -- index 2, silScore -0.7 -- moves its list position or is not listed at all); Kt = N:
    the same list in every frame, read once by the 32-bit kernel"""
    base = _lf(N, 10, 40, sil_score=-0.7, u=N)
    for Kt in (5, 10, N):
        c = dict(base, Kt=Kt)
        assert np.array_equal(_rows(c), _rows(base))
        _check(sess, oracle_lib, c, threads, sil=2)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("Kt", [None, 10])
def test_asg_with_bit_31_listed(sess, oracle_lib, Kt, threads):
    """ASG, N = 32: no blank, every token is listed, token 31 (bit 31 of a 32-bit mask) wins frames 5, 6 and 20 and is the
    last token of states in the beam (asserted from the oracle's n-best)"""
    c = _lf(32, 10, 40, Kt=Kt, crit="asg", dist="uniform", u=32)
    e = _rows(c)
    e.reshape(40, 32)[[5, 6, 20], 31] = 0.0
    assert any(31 in [int(t) for t in h.tokens] for h in _want(oracle_lib, c, 0, e, "last-token")), "token 31 never decoded"
    _check(sess, oracle_lib, c, threads, e=e, tag="last-token")


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N,crit,sils", [(29, "ctc", (0, 14, 27)), (32, "asg", (0, 16, 30)), (64, "ctc", (0, 31, 62))])
def test_sil_score_with_sil_first_in_the_middle_and_last_but_one(sess, oracle_lib, N, crit, sils, threads):
    """sil's list position is among the values a token wave keeps: index 0, the middle, N - 2"""
    for sil in sils:
        _check(sess, oracle_lib, _lf(N, 10, 40, crit=crit, sil_score=-0.7, u=N + 1), threads, sil)


# ---- early returns ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("nan_row", [1, 20, 21, 39])
def test_row_of_nan_in_one_utterance_of_three(sess, oracle_lib, nan_row, threads):
    """the middle utterance has a NaN, a row of equal values (ties) and a row of nothing but NaN -- in the first frame
    that was handed its row, in a frame of either parity, in the last frame: `dead` returns with the next row's fetch in flight.  It comes back
    through the generic engine (compared with a decode on that engine alone: the reference's order among tied candidates
    is not a function of its inputs), the other two untouched (compared with the oracle)"""
    c0 = _lf(29, 10, 40, sil_score=-0.7, u=31)
    cs = [dict(c0, u=31 + i) for i in range(3)]
    rows = [_rows(c) for c in cs]
    bad = rows[1].reshape(40, 29)
    bad[7, 3] = np.nan
    bad[12, :] = -3.0
    bad[nan_row, :] = np.nan
    e = np.concatenate(rows)
    d = _decoder(sess, c0, 0, threads)
    d.decode_batch(e, [40, 40, 40], 29)
    path = _path(d)
    # ("threads" is the last launch's, here the generic engine's that decoded the flagged utterance again: the lane
    # engine's thread count shows in test_ragged_batch and in every _check)
    assert path["engine"] == 4 and path["redone"] == 1 and path["slane_m32"] == 1 and path["tlane"] == 0, path
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


# ---- re-entry frames ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N,K,crit", [(5, 10, "ctc"), (6, 50, "ctc"), (5, 10, "asg")])
def test_small_alphabet_states_come_back(sess, oracle_lib, N, K, crit, threads):
    """five or six tokens, near-flat rows, 60 frames: LM states drop out of the beam and are entered again; the frame
    after a re-entry reloads records and masks behind the row it was handed.  (Counted once with a temporary counter in
    the emulator, 512 threads: 3, 2 and 3 frames of these three cases run the re-entry path, and 5 of the 40 frames of
    test_boundary_bin_is_ranked's N = 29 case.)"""
    _check(sess, oracle_lib, _lf(N, K, 60, crit=crit, dist="uniform", sil_score=-0.7, u=N + K), threads, sil=1)


# ---- the far bin and the boundary bin: barriers between the first and the second, nothing behind the second ---------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N", [29, 33])
def test_far_bin_is_counted(sess, oracle_lib, N, threads):
    """test_slane_narrow.py's case: rows sixty times as wide as `uniform`'s, beam 64, a threshold nothing fails -- the
    phase-clock instantiation counts the frames that count the far bin (1e6 each in slot 6)"""
    c = _lf(N, 64, 40, dist="uniform", u=7, thr=1e9)
    e = (np.asarray(_inputs(c)["e"], dtype=np.float32) * np.float32(60.0)).astype(np.float32)
    _, prof = _check(sess, oracle_lib, c, threads, e=e, tag="x60", profile=True)
    assert int(prof[6]) // 1000000 >= 1, prof


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N", [29, 33])
def test_boundary_bin_is_ranked(sess, oracle_lib, N, threads):
    """the benchmark's distribution at beam 50: in some frames only some members of the K-th best's bin survive -- the
    phase-clock instantiation counts those frames (1 each in slot 6)"""
    _, prof = _check(sess, oracle_lib, _lf(N, 50, 40, dist="ctc", u=50), threads, profile=True)
    assert int(prof[6]) % 1000000 >= 1, prof


# ---- the switch: a token wave reads its list in every frame, or once ---------------------------------------------------

@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("N,crit", [(29, "ctc"), (32, "asg")])
def test_list_read_once_or_in_every_frame(sess, oracle_lib, N, crit, threads):
    """full token beam, silScore at a middle index: tune bit 1 set, every frame reads the list; clear, the loop keeps
    the prologue's -- the same n-best, and the oracle's"""
    c = _lf(N, 50, 40, crit=crit, sil_score=-0.7, u=N + 2)
    once, _ = _check(sess, oracle_lib, c, threads, sil=14)
    every, _ = _check(sess, oracle_lib, c, threads, sil=14, tune=2)
    ok, why = helpers.hyps_equal(once, every, score_tol=0.0)
    assert ok, why


# ---- the instantiations that share the frame's text and keep their reads where they were -----------------------------

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


@pytest.mark.parametrize("lm", ["zero", ec.TOK_LM], ids=["zerolm", "toklm"])
def test_streams_in_chunks_of_one_two_and_seven_frames(sess, oracle_lib, lm):
    """chunks of 1, 2 and 7 frames, getBestHypothesis after each and a prune after every second: every chunk has a last
    frame and the next one a restart from the parked beam"""
    c = _lf(29, 10, 40, sil_score=-0.7, lm=lm, u=5)
    inp = _inputs(c)
    chunks = [1, 2, 7] * 4
    want = ss.trace_checker(oracle_lib, c, inp, chunks, [0, 3])
    assert not ss.has_ties(want)
    d = sess.decoder(c, inp)
    d.stream_begin(1, 29, 64)
    on = (int(d.get("sstream")) > 0, int(d.get("tstream")))
    d.close()
    assert on == (True, 0 if lm == "zero" else 1), on
    got, _ = ss.trace_device(sess, c, inp, chunks, [0, 3])
    diff = ss.first_difference(want, got)
    assert diff is None, diff
    assert sess.last_stream_redone == 0
