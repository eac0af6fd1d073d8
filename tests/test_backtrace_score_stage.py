"""The score pass of the narrow back-trace (backtraceNarrow, fltx_kernels.h) with its addends staged by hypothesis:
the waves that do not add write emission[frame][token of hypothesis k] (ASG: the f64 sum with the transition) into LDS
rows by hypothesis a stretch ahead, frames that add nothing and the tails of the rows as -0.0, and an adding wave does
one 16-byte read per four frames, a convert and an f64 addition per frame.  Every hypothesis -- tokens, words, score,
emitting-model score, LM score -- is compared bit for bit with the oracle, on the emulator and (`-m gpu`) on the device.

fltx_decoder_get "engine", "redone", "bt_record_bytes", "bt_walk_waves" and "bt_stretch_frames" say which path and
which geometry a batch took, so that no case passes on another path than the one it names.  The emulator launches a
single wave for beams up to 64 unless "bt_threads" says otherwise, so every case sets it.

Stretch lengths: launchBacktrace takes the longest stretch whose padded rows fit, and a row is padded to whole 16-byte
reads, so with several stretches "bt_stretch_frames" is always a whole number of reads; the padded tail is met by the
LAST stretch of an utterance (the seam test asserts frame counts of 4 n - 1, 4 n and 4 n + 1 there) and by batches whose
single stretch is as long as their longest utterance's rows (T = 40: 42 frames to a row of 44).

Rows without a token: an offline decode returns paths whose only token-less row is the last one (the row decodeEnd
adds, token -1), which lies beyond the frames the score pass adds; hypotheses pruned inside the utterance are not
returned.  So no returned path has a NONE / NOROW row among its decoded frames (test_no_returned_path_skips_a_frame
asserts that from the returned tokens); the -0.0 of a skipped frame is exercised by the tails only."""
import numpy as np
import pytest

import cases
import engine_choices as ec
import helpers

WHERE = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=WHERE)
def sess(request):
    return request.getfixturevalue("emu_session" if request.param == "emu" else "gpu_session")


def _case(c, name, T):
    return dict(c, name=name, T=T)


def _decode(d, cs, inps):
    e = np.concatenate([np.asarray(i["e"], dtype=np.float32).reshape(-1)[:c["T"] * c["N"]] for c, i in zip(cs, inps)])
    d.decode_batch(e, [c["T"] for c in cs], cs[0]["N"])


def _compare(d, oracle_lib, cs, inps, max_hyp=None):
    for b, (c, inp) in enumerate(zip(cs, inps)):
        want = helpers.run_checker(oracle_lib, c, inp)
        if max_hyp is not None:
            want = want[:max_hyp]
        ok, why = helpers.hyps_equal(want, d.results(b, max_hyp), score_tol=0.0)
        assert ok, "%s (utterance %d of %d, T = %d): %s" % (c["name"], b, len(cs), c["T"], why)


def _check_batch(sess, oracle_lib, cs, sets=None, d=None, inps=None, max_hyp=None):
    """decode the cases cs (same options, their own T and emissions) as ONE batch, on the decoder d if one is given
    -> the decoder, after every utterance's n-best has been compared with the oracle's"""
    inps = inps or [helpers.case_inputs(c) for c in cs]
    if d is None:
        d = sess.decoder(cs[0], inps[0])
    for k, v in (sets or {}).items():
        d.set(k, v)
    _decode(d, cs, inps)
    _compare(d, oracle_lib, cs, inps, max_hyp)
    return d


def _path(d):
    return {k: int(d.get(k)) for k in ("engine", "redone", "why_not_lane", "bt_record_bytes", "bt_walk_waves",
                                       "bt_chunk_frames", "bt_stretch_frames")}


@pytest.mark.parametrize("threads,waves", [(256, 4), (64, 1)])
def test_stretch_seams(sess, oracle_lib, threads, waves):
    """bt_lds_kb = 4 at beam 10: stretches of a few dozen frames.  An utterance of 170 frames rides along and holds the
    geometry still (the tile of the longest utterance takes the budget first) while the other one's decoded frames run
    through a contiguous range around two stretches: one below, at and one above a multiple of the reported stretch
    length, so the last stretch has 4 n - 1, 4 n and one frame -- asserted from the reported geometry.  Four waves: three
    of them stage beside the adding wave; one wave: every thread adds, then stages."""
    c, anchor = ec._lf(29, 10), 170
    sets = {"bt_lds_kb": 4, "bt_threads": threads}

    def run(Ts):
        cs = [_case(dict(c, u=c["u"] + i), "seam%d" % i, T) for i, T in enumerate(Ts)]
        d = _check_batch(sess, oracle_lib, cs, sets)
        got = _path(d)
        d.close()
        assert got["engine"] == 4 and got["bt_record_bytes"] == 2 and got["bt_walk_waves"] == waves and got["redone"] == 0, (Ts, got)
        assert got["bt_stretch_frames"] >= 8, (Ts, got)
        return got["bt_stretch_frames"]

    Fe = run([anchor])
    assert 2 * Fe + 2 <= anchor, Fe  # (more than two stretches; the range stays below the anchor)
    seam, tails = set(), set()
    for T in range(2 * Fe - 2, 2 * Fe + 3):
        assert run([anchor, T]) == Fe
        seam.add({Fe - 1: "below", 0: "at", 1: "above"}.get(T % Fe))
        tails.add((T % Fe or Fe) % 4)
    assert {"below", "at", "above"} <= seam, seam
    assert {3, 0, 1} <= tails or Fe % 4, (Fe, tails)  # (the last stretch ends inside a 16-byte read, and on one)


@pytest.mark.parametrize("threads,waves", [(64, 1), (128, 2), (512, 8)])
def test_few_spare_waves_at_beam_50(sess, oracle_lib, threads, waves):
    """no staging wave, one, seven; T = 40 is one stretch of 42 frames to a row of 44"""
    d = _check_batch(sess, oracle_lib, [_case(ec._lf(29, 50), "spare%d" % threads, 40)], {"bt_threads": threads})
    got = _path(d)
    d.close()
    assert got["engine"] == 4 and got["bt_record_bytes"] == 2 and got["bt_walk_waves"] == waves and got["redone"] == 0, got
    assert got["bt_stretch_frames"] == 42, got


def test_every_lane_of_the_adding_wave_is_live(sess, oracle_lib):
    cs = [_case(ec._lf(29, 64, u=2), "k64", 40), _case(ec._lf(29, 64, u=3), "k64b", 33)]
    d = _check_batch(sess, oracle_lib, cs, {"bt_threads": 512, "bt_lds_kb": 16})
    got = _path(d)
    d.close()
    assert got["engine"] == 4 and got["bt_record_bytes"] == 2 and got["bt_walk_waves"] == 8 and got["redone"] == 0, got
    assert 8 <= got["bt_stretch_frames"] < 33, got  # (several stretches)


def test_two_adding_waves_no_staging_wave(sess, oracle_lib):
    """beam 100 at bt_threads = 128: four-byte records, one walk per hypothesis, both waves add, then stage"""
    d = _check_batch(sess, oracle_lib, [_case(ec._lf(29, 100, u=3), "k100", 30)], {"bt_threads": 128, "bt_lds_kb": 24})
    got = _path(d)
    d.close()
    assert got["engine"] == 4 and got["bt_record_bytes"] == 4 and got["bt_walk_waves"] == 1 and got["redone"] == 0, got
    assert 8 <= got["bt_stretch_frames"] < 30, got


def _wide_emissions(T, N, seed):
    """rows whose magnitudes span 2^-20 .. 2^6, exact +0.0 and -0.0 scattered among them.  Half of the rows are
    negative, so their best tokens are the tiny ones (or a zero), half positive, so theirs are the large ones: a path
    adds values near 2^6 and near 2^-20 in turn, and its f64 sum of 24-bit addends needs more than 53 bits."""
    rng = np.random.RandomState(seed)
    e = np.exp2(rng.uniform(-20.0, 6.0, size=(T, N))).astype(np.float32)
    e[rng.uniform(size=T) < 0.5] *= -1.0
    # (at most one zero to a row: two would be tied candidates, on which the reference's order is not defined)
    rows = np.flatnonzero(rng.uniform(size=T) < 0.4)
    e[rows, rng.randint(0, N, size=len(rows))] = np.where(rng.uniform(size=len(rows)) < 0.5, 0.0, -0.0)
    return e


@pytest.fixture(scope="module")
def wide_case(oracle_lib):
    """emissions that show a wrong order of the additions, and what the oracle makes of them -- computed once.  Checked
    here, with the oracle alone: a returned path's addends summed forwards give its emitting-model score, summed
    backwards they give another."""
    c = _case(ec._lf(29, 50, u=9), "wide", 90)
    inp = dict(helpers.case_inputs(c))
    e = _wide_emissions(c["T"], c["N"], 4)
    inp["e"] = e
    want = helpers.run_checker(oracle_lib, c, inp)
    differs = 0
    for h in want:
        tk = np.asarray(h.tokens)[1:c["T"] + 1]
        assert (tk >= 0).all()
        adds = e[np.arange(c["T"]), tk].astype(np.float64)
        fwd = 0.0
        for x in adds:
            fwd += x
        bwd = 0.0
        for x in adds[::-1]:
            bwd += x
        assert fwd == h.am, (fwd.hex(), float(h.am).hex())
        differs += bwd != h.am
    assert differs > 0
    return c, inp, want


@pytest.mark.parametrize("threads,kb", [(512, 12), (64, 12), (256, 0)])
def test_values_that_show_a_wrong_order_or_a_wrong_skip(sess, wide_case, threads, kb):
    c, inp, want = wide_case
    d = sess.decoder(c, inp)
    d.set("bt_threads", threads)
    d.set("bt_lds_kb", kb)
    _decode(d, [c], [inp])
    got = _path(d)
    ok, why = helpers.hyps_equal(want, d.results(0), score_tol=0.0)
    d.close()
    assert ok, why
    assert got["engine"] == 4 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got
    assert got["bt_walk_waves"] == threads // 64, got
    assert (got["bt_stretch_frames"] < c["T"]) == (kb > 0), got


def test_no_returned_path_skips_a_frame(wide_case, oracle_lib):
    """(see the module's docstring) every returned path has a token at every decoded frame"""
    for c, want in ((wide_case[0], wide_case[2]),
                    (_case(ec._lf(29, 10, thr=3.0, u=5), "tight", 60), None)):
        want = want or helpers.run_checker(oracle_lib, c, helpers.case_inputs(c))
        for h in want:
            assert (np.asarray(h.tokens)[1:c["T"] + 1] >= 0).all()


def test_ragged_batch_and_an_nbest_limited_read(sess, oracle_lib):
    c = ec._lf(29, 50)
    cs = [_case(dict(c, u=c["u"] + i), "ragged%d" % i, T) for i, T in enumerate((0, 1, 2, 40))]
    d = _check_batch(sess, oracle_lib, cs, {"bt_threads": 256, "bt_lds_kb": 12})
    got = _path(d)
    _compare(d, oracle_lib, cs, [helpers.case_inputs(x) for x in cs], max_hyp=3)
    d.close()
    assert got["engine"] == 4 and got["bt_walk_waves"] == 4 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got
    assert 8 <= got["bt_stretch_frames"] < 40, got


# (name, case, sets, T, budget KB, record bytes, waves that walk, several stretches)
KINDS = [
    # ASG: the addend is the f64 sum of emission and transition, staged as a double
    ("asg_k50", ec._lf(29, 50, crit="asg"), None, 40, 16, 2, 4, True),
    ("asg_k50_one_wave", ec._lf(29, 50, crit="asg"), {"bt_threads": 64}, 40, 16, 2, 1, True),
    # the lexicon engines (word rows unchanged): ZeroLM and an n-gram
    ("xlane_k10", ec._lx(10), None, 40, 3, 2, 4, True),
    ("ylane_ngram_k100", ec._lx(100, lm=ec.WORD_LM, u=7), None, 30, 0, 2, 1, False),
    # the token LM (C2T's options): the LM chain on a wave of its own (256 threads at beam 50), and on the adding
    # wave where there is none to spare (128 threads: one adds, one stages)
    ("toklm_k50", ec._lf(29, 50, lm=ec.TOK_LM), None, 40, 12, 2, 4, True),
    ("toklm_k50_two_waves", ec._lf(29, 50, lm=ec.TOK_LM), {"bt_threads": 128}, 40, 12, 2, 2, True),
    ("toklm_k16_asg", ec._lf(29, 16, crit="asg", lm=ec.TOK_LM, u=2), None, 40, 8, 2, 4, True),
    ("toklm_k100", ec._lf(29, 100, lm=ec.TOK_LM, u=5), {"bt_threads": 512}, 30, 24, 4, 1, True),
    # 1 024 word pieces: 16-bit tokens, nothing but the addends in LDS
    ("wlane_n1024", ec._lf(1024, 10, Kt=30, u=6), None, 20, 2, 4, 4, True),
]


@pytest.mark.parametrize("name,c,sets,T,kb,rec,waves,several", KINDS, ids=[v[0] for v in KINDS])
def test_other_variants(sess, oracle_lib, name, c, sets, T, kb, rec, waves, several):
    d = _check_batch(sess, oracle_lib, [_case(c, name, T)], dict({"bt_threads": 256, "bt_lds_kb": kb}, **(sets or {})))
    got = _path(d)
    d.close()
    assert got["why_not_lane"] == 0 and got["redone"] == 0, got
    assert got["bt_record_bytes"] == rec and got["bt_walk_waves"] == waves, got
    assert got["bt_stretch_frames"] >= 8 and (got["bt_stretch_frames"] < T) == several, got


def test_a_reused_decoder(sess, oracle_lib):
    """long, short, long on one object: no addend or token of an earlier batch leaks"""
    c = ec._lf(29, 50)
    sets = {"bt_threads": 256, "bt_lds_kb": 12}
    d = _check_batch(sess, oracle_lib, [_case(dict(c, u=i), "long%d" % i, 40) for i in range(3)], sets)
    _check_batch(sess, oracle_lib, [_case(dict(c, u=100 + i), "short%d" % i, T) for i, T in enumerate((5, 2, 9))], d=d)
    _check_batch(sess, oracle_lib, [_case(dict(c, u=200 + i), "again%d" % i, T) for i, T in enumerate((40, 37))], d=d)
    got = _path(d)
    d.close()
    assert got["engine"] == 4 and got["bt_walk_waves"] == 4 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got


def test_the_queued_look(sess, oracle_lib):
    """Two decoder objects with defer_check = 1 take turns at T = 40; the copy of a pending batch's status rows is
    queued behind its back-trace and the settle only waits for it.  In one batch a row of equal values (no defined
    token beam, as in test_gpu_batches.py) sends one utterance to the generic engine: the next decode_batch on that
    object settles it and counts it in unread_redone; reading results with no decode_batch after them settles too.
    The flagged utterance has tied candidates, on which the reference's order is not a function of its inputs (see
    test_backtrace_onepass.py): it is compared with a decode on the generic engine alone, every other utterance with
    the oracle."""
    from text_amd import synth
    N, T, B, flagged = 300, 40, 5, 1
    c = cases.case("wp_look", dist="ctc", T=T, N=N, K=20, Kt=30, u=515)
    batches = [synth.batch("ctc", B, T, N) for _ in range(2)]
    tied = batches[0].copy()
    tied[flagged, 9, :] = -3.0
    g = sess.decoder(c, dict(tr=None))
    g.set("wlane", 0)
    g.decode_batch(tied, [T] * B, N)
    generic = g.results(flagged)
    g.close()

    def check(d, e, flagged_here):
        for b in range(B):
            want = generic if (flagged_here and b == flagged) else \
                helpers.run_checker(oracle_lib, c, dict(e=np.ascontiguousarray(e[b]), tr=None, lex=None))
            ok, why = helpers.hyps_equal(want, d.results(b), score_tol=0.0)
            assert ok, "utterance %d: %s" % (b, why)

    decs = [sess.decoder(c, dict(tr=None)) for _ in range(2)]
    for d in decs:
        d.set("defer_check", 1)
        d.set("bt_threads", 256)
    decs[0].decode_batch(batches[1], [T] * B, N)   # pending on object 0
    decs[1].decode_batch(tied, [T] * B, N)         # pending on object 1: one utterance flagged
    decs[0].decode_batch(batches[1], [T] * B, N)   # settles object 0's first batch, unread: nothing to decode again
    assert decs[0].get("unread_redone") == 0
    decs[1].decode_batch(batches[1], [T] * B, N)   # settles the flagged batch, unread
    assert decs[1].get("unread_redone") == 1
    check(decs[0], batches[1], False)              # reading settles object 0's second batch
    check(decs[1], batches[1], False)
    assert decs[0].get("redone") == 0 and decs[1].get("redone") == 0
    decs[1].decode_batch(tied, [T] * B, N)         # ... and results read with no decode_batch after them settle it
    check(decs[1], tied, True)
    assert decs[1].get("redone") == 1 and decs[1].get("unread_redone") == 1
    assert decs[1].get("engine") == 4 and decs[1].get("bt_record_bytes") == 4
    for d in decs:
        d.close()
