"""The parallel walk of the narrow back-trace (backtraceNarrow<RT, true>, fltx_kernels.h): every wave of the workgroup
walks its own stretch of each record chunk from every slot at once, and the hypotheses are composed through the waves'
exit maps; tokens, words and scores then leave through the entry map.  Every hypothesis -- tokens, words, score,
emitting-model score, LM score -- is compared bit for bit with the oracle, on the emulator and (`-m gpu`) on the device.

fltx_decoder_get "bt_walk_waves" says how many waves walked the last batch's chunks (1 = one walk per hypothesis) and
"bt_record_bytes" which records they walked, so that no case passes on another path than the one it names.  The
emulator launches a single wave for beams up to 64 unless "bt_threads" says otherwise, so every case sets it."""
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
    c0 = cs[0]
    e = np.concatenate([np.asarray(i["e"], dtype=np.float32).reshape(-1)[:c["T"] * c["N"]] for c, i in zip(cs, inps)])
    d.decode_batch(e, [c["T"] for c in cs], c0["N"])


def _compare(d, oracle_lib, cs, inps):
    for b, (c, inp) in enumerate(zip(cs, inps)):
        want = helpers.run_checker(oracle_lib, c, inp)
        ok, why = helpers.hyps_equal(want, d.results(b), score_tol=0.0)
        assert ok, "%s (utterance %d of %d, T = %d): %s" % (c["name"], b, len(cs), c["T"], why)


def _check_batch(sess, oracle_lib, cs, sets=None, d=None):
    """decode the cases cs (same options, their own T and emissions) as ONE batch, on the decoder d if one is given
    -> the decoder, after every utterance's n-best has been compared with the oracle's"""
    inps = [helpers.case_inputs(c) for c in cs]
    if d is None:
        d = sess.decoder(cs[0], inps[0])
    for k, v in (sets or {}).items():
        d.set(k, v)
    _decode(d, cs, inps)
    _compare(d, oracle_lib, cs, inps)
    return d


def _path(d):
    return {k: int(d.get(k)) for k in ("engine", "redone", "why_not_lane", "bt_record_bytes", "bt_walk_waves",
                                       "bt_chunk_frames")}


def _all_results(d, n):
    return [d.results(b) for b in range(n)]


@pytest.mark.parametrize("threads", [128, 256, 512])
def test_wave_counts(sess, oracle_lib, threads):
    """2, 4 and 8 waves: the oracle's results, and the serial walk's on the same inputs"""
    cs = [_case(ec._lf(29, 50), "waves%d" % threads, 40)]
    d = _check_batch(sess, oracle_lib, cs, {"bt_threads": threads})
    got = _path(d)
    par = _all_results(d, 1)
    d.close()
    assert got["bt_walk_waves"] == threads // 64 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got
    s = _check_batch(sess, oracle_lib, cs, {"bt_threads": threads, "bt_walk_waves": 1})
    got = _path(s)
    ser = _all_results(s, 1)
    s.close()
    assert got["bt_walk_waves"] == 1 and got["bt_record_bytes"] == 2, got
    for a, b in zip(par, ser):
        ok, why = helpers.hyps_equal(b, a, score_tol=0.0)
        assert ok, why


def test_chunk_seams_and_short_stretches(sess, oracle_lib):
    """bt_lds_kb = 4 and four waves at beam 10: chunks of a few dozen frames.  The chunk length follows from the
    batch's LONGEST utterance (its tile takes the budget first), so an utterance of 170 frames rides along in every
    batch and holds the geometry still while the other one's T runs through a contiguous range around two chunks of
    history rows (T + 2) -- the range follows from the chunk length the library reports: the rows fall one below, at
    and one above a multiple of the chunk, and the last chunk on fewer frames than waves, on as many and on one more;
    stretches of no frame and of one frame occur.  All of it is asserted from the reported geometry."""
    c, waves, anchor = ec._lf(29, 10), 4, 170
    sets = {"bt_lds_kb": 4, "bt_threads": 64 * waves}

    def run(Ts):
        cs = [_case(dict(c, u=c["u"] + i), "seam%d" % i, T) for i, T in enumerate(Ts)]
        d = _check_batch(sess, oracle_lib, cs, sets)
        got = _path(d)
        d.close()
        assert got["bt_record_bytes"] == 2 and got["bt_walk_waves"] == waves and got["redone"] == 0, (Ts, got)
        assert got["bt_chunk_frames"] >= 8, (Ts, got)
        return got["bt_chunk_frames"]

    F = run([anchor])
    S = (F + waves - 1) // waves  # frames per stretch: wave w walks the chunk's rows w S .. w S + S - 1 from its top
    assert F < anchor + 2 and 2 * F + waves + 1 <= anchor + 2, F  # (more than one chunk; the range stays below the anchor)
    seam, last, stretch = set(), set(), set()
    for rows in range(2 * F - 1, 2 * F + waves + 2):
        assert run([anchor, rows - 2]) == F
        seam.add({F - 1: "below", 0: "at", 1: "above"}.get(rows % F))
        r = rows % F or F  # frames of the last chunk
        last.add("fewer" if r < waves else "as many" if r == waves else "one more" if r == waves + 1 else None)
        stretch.update(max(0, min((w + 1) * S, F, r) - w * S) for w in range(waves))
    assert {"below", "at", "above"} <= seam, seam
    assert {"fewer", "as many", "one more"} <= last, last
    assert {0, 1} <= stretch, stretch


@pytest.mark.parametrize("T", [0, 1, 2])
def test_fewer_hypotheses_than_slots(sess, oracle_lib, T):
    """the shortest utterances at beam 50: most slots of every frame hold no record of this batch"""
    d = _check_batch(sess, oracle_lib, [_case(ec._lf(29, 50), "short", T)], {"bt_threads": 256})
    got = _path(d)
    d.close()
    assert got["bt_walk_waves"] == 4 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got


def test_ragged_batch(sess, oracle_lib):
    c = ec._lf(29, 50)
    cs = [_case(dict(c, u=c["u"] + i), "ragged%d" % i, T) for i, T in enumerate((23, 1, 40, 0, 7, 39))]
    d = _check_batch(sess, oracle_lib, cs, {"bt_threads": 256})
    got = _path(d)
    d.close()
    assert got["bt_walk_waves"] == 4 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got


def test_reused_workspace(sess, oracle_lib):
    """One decoder object decodes a dense batch, then a different and shorter one: the slots that hold no record of the
    second batch hold the first batch's.  The second batch's results are the oracle's."""
    c = ec._lf(29, 50)
    d = _check_batch(sess, oracle_lib, [_case(dict(c, u=i), "dense%d" % i, 40) for i in range(4)], {"bt_threads": 256})
    assert _path(d)["bt_walk_waves"] == 4
    _check_batch(sess, oracle_lib, [_case(dict(c, u=100 + i), "after%d" % i, T) for i, T in enumerate((5, 12, 8, 9))], d=d)
    got = _path(d)
    d.close()
    assert got["bt_walk_waves"] == 4 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got


@pytest.mark.parametrize("K", [63, 64])
def test_a_full_wave_of_slots(sess, oracle_lib, K):
    d = _check_batch(sess, oracle_lib, [_case(ec._lf(29, K, u=2), "k%d" % K, 40)], {"bt_threads": 512})
    got = _path(d)
    d.close()
    assert got["engine"] == 4 and got["bt_walk_waves"] == 8 and got["bt_record_bytes"] == 2 and got["redone"] == 0, got


# (name, case, sets, T, record bytes, waves that walk at 256 threads)
KINDS = [
    # the token-LM variant: the LM score re-added through the entry map (ASG: the transitions too)
    ("tlane", ec._lf(29, 16, crit="asg", lm=ec.TOK_LM), None, 40, 2, 4),
    # the lexicon engines: word rows through the entry map
    ("xlane_k10", ec._lx(10), None, 40, 2, 4),
    ("ylane_k10", ec._lx(10, scores=51, u=1), {"ylane": 2}, 40, 2, 4),
    # beams beyond 64 keep one walk per hypothesis
    ("mlane_k100", ec._lf(29, 100, u=3), None, 30, 4, 1),
    ("ylane_ngram_k100", ec._lx(100, lm=ec.WORD_LM, u=7), None, 30, 2, 1),
    # fltx_wlane.h: 16-bit tokens, emissions gathered along the path
    ("wlane_n1024", ec._lf(1024, 10, Kt=30, u=6), None, 20, 4, 4),
]


@pytest.mark.parametrize("name,c,sets,T,rec,waves", KINDS, ids=[v[0] for v in KINDS])
def test_other_record_kinds(sess, oracle_lib, name, c, sets, T, rec, waves):
    d = _check_batch(sess, oracle_lib, [_case(c, name, T)], dict(sets or {}, bt_threads=256))
    got = _path(d)
    d.close()
    assert got["why_not_lane"] == 0 and got["redone"] == 0, got
    assert got["bt_record_bytes"] == rec and got["bt_walk_waves"] == waves, got


# (name, case, T, record bytes, waves that walk)
FEW_THREADS = [
    ("mlane_k100", ec._lf(29, 100, u=3), 30, 4, 1),
    ("ylane_ngram_k100", ec._lx(100, lm=ec.WORD_LM, u=7), 30, 2, 1),
    ("slane_k50", ec._lf(29, 50), 40, 2, 1),
]


@pytest.mark.parametrize("name,c,T,rec,waves", FEW_THREADS, ids=[v[0] for v in FEW_THREADS])
def test_fewer_threads_asked_than_slots(sess, oracle_lib, name, c, T, rec, waves):
    """"bt_threads" = 64 below the beam: the score passes are one thread per hypothesis, so the workgroup is raised to
    cover the beam -- the batch keeps its narrow records and every hypothesis its scores (at beam 50 one wave is enough
    and is what runs: one walk per hypothesis)"""
    d = _check_batch(sess, oracle_lib, [_case(c, name, T)], {"bt_threads": 64})
    got = _path(d)
    d.close()
    assert got["why_not_lane"] == 0 and got["redone"] == 0, got
    assert got["bt_record_bytes"] == rec and got["bt_walk_waves"] == waves, got


@pytest.mark.parametrize("T", [39, 37])
def test_odd_beam_odd_length_lexicon(sess, oracle_lib, T):
    """beam 15 under a lexicon, two-byte records: a chunk of F x 15 of them ends on an odd half-word when F is odd, and
    the int32 word records lie behind it (tests/cpp/backtrace_walk_san.sh runs such a case under UBSan)"""
    d = _check_batch(sess, oracle_lib, [_case(ec._lx(15), "odd_lex", T)], {"bt_threads": 256})
    got = _path(d)
    d.close()
    assert got["why_not_lane"] == 0 and got["redone"] == 0, got
    assert got["bt_record_bytes"] == 2 and got["bt_walk_waves"] == 4, got
    assert got["bt_chunk_frames"] * 15 % 2 == 1, got


def test_plain_records_beside_packed_ones(sess, oracle_lib):
    """A packed batch in which one utterance was decoded again on the generic engine (as in
    test_backtrace_onepass.py): its plain records take backtraceUtterance inside the parallel walk's launch.  The
    flagged utterance (tied candidates) is compared with a decode on the generic engine alone, the others with the
    oracle."""
    from text_amd import synth
    N, T, B, flagged = 300, 12, 5, 2
    c = cases.case("wp_mixed", dist="ctc", T=T, N=N, K=20, Kt=30, u=515)
    e = synth.batch("ctc", B, T, N)
    e[flagged, 5, :] = -3.0
    d = sess.decoder(c, dict(tr=None))
    d.set("bt_threads", 256)
    d.decode_batch(e, [T] * B, N)
    got = _path(d)
    assert got["redone"] > 0 and got["engine"] == 4 and got["bt_record_bytes"] == 4 and got["bt_walk_waves"] == 4, got
    g = sess.decoder(c, dict(tr=None))
    g.set("wlane", 0)
    g.decode_batch(e, [T] * B, N)
    assert g.get("engine") != 4 and g.get("bt_record_bytes") == 0 and g.get("bt_walk_waves") == 1
    for b in range(B):
        want = g.results(b) if b == flagged else \
            helpers.run_checker(oracle_lib, c, dict(e=np.ascontiguousarray(e[b]), tr=None, lex=None))
        ok, why = helpers.hyps_equal(want, d.results(b), score_tol=0.0)
        assert ok, "utterance %d: %s" % (b, why)
    d.close()
    g.close()
