"""The back-trace of the lane engines' packed history records in one residency (backtraceNarrow, fltx_kernels.h):
records narrowed to 8 + 8 or 16 + 16 bits on the way into LDS, the utterance's token tile resident there, the
emitting-model (and token-LM) score re-added from that tile.  Every hypothesis -- tokens, words, score, emitting-model
score, LM score -- is compared bit for bit with the oracle, on the emulator and (`-m gpu`) on the device.

fltx_decoder_get "bt_record_bytes" (2 / 4 = narrowed, 0 = the chunked back-trace of 8-byte records), "bt_chunk_frames"
and "bt_stretch_frames" say which path and which LDS geometry a batch took, so that no case passes on another path
than the one it names."""
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


def _check_batch(sess, oracle_lib, cs, sets=None):
    """decode the cases cs (same options, their own T and emissions) as ONE batch -> the decoder, after every
    utterance's n-best has been compared with the oracle's"""
    inps = [helpers.case_inputs(c) for c in cs]
    c0 = cs[0]
    d = sess.decoder(c0, inps[0])
    for k, v in (sets or {}).items():
        d.set(k, v)
    e = np.concatenate([np.asarray(i["e"], dtype=np.float32).reshape(-1)[:c["T"] * c["N"]] for c, i in zip(cs, inps)])
    d.decode_batch(e, [c["T"] for c in cs], c0["N"])
    for b, (c, inp) in enumerate(zip(cs, inps)):
        want = helpers.run_checker(oracle_lib, c, inp)
        ok, why = helpers.hyps_equal(want, d.results(b), score_tol=0.0)
        assert ok, "%s (utterance %d of %d, T = %d): %s" % (c["name"], b, len(cs), c["T"], why)
    return d


def _engine(d):
    return {k: int(d.get(k)) for k in ("engine", "slane", "wlane", "tlane", "xlane", "ylane", "lane_groups",
                                       "why_not_lane", "redone", "bt_record_bytes")}


# (name, case, sets, T, what fltx_decoder_get must say afterwards)
VARIANTS = [
    # fltx_slane.h, beam 50: 8-bit slots, 8-bit tokens; CTC and ASG (transitions)
    ("slane_k50_ctc", ec._lf(29, 50), None, 40, dict(engine=4, lane_groups=1, wlane=0, tlane=0, bt_record_bytes=2)),
    ("slane_k50_asg", ec._lf(29, 50, crit="asg"), None, 40, dict(engine=4, lane_groups=1, tlane=0, bt_record_bytes=2)),
    # fltx_mlane.h: 10-bit slots
    ("mlane_k100", ec._lf(29, 100, u=3), None, 30, dict(engine=4, lane_groups=2, tlane=0, bt_record_bytes=4)),
    ("mlane_k300", ec._lf(29, 300, u=4), None, 20, dict(engine=4, lane_groups=8, tlane=0, bt_record_bytes=4)),
    # the token-LM variants (the LM score re-added along the path), one and two lane groups, CTC and ASG
    ("tlane_k10", ec._lf(29, 10, lm=ec.TOK_LM), None, 40, dict(engine=4, lane_groups=1, tlane=1, bt_record_bytes=2)),
    ("tlane_k16_asg", ec._lf(29, 16, crit="asg", lm=ec.TOK_LM, u=2), None, 40, dict(engine=4, tlane=1, bt_record_bytes=2)),
    ("tmlane_k100", ec._lf(29, 100, lm=ec.TOK_LM, u=5), None, 30, dict(engine=4, lane_groups=2, tlane=1, bt_record_bytes=4)),
    # fltx_wlane.h, 1 024 tokens: wide tokens, emissions gathered along the path
    ("wlane_n1024", ec._lf(1024, 10, Kt=30, u=6), None, 20, dict(engine=4, wlane=1, bt_record_bytes=4)),
    # the lexicon engines (word rows): fltx_xlane.h, fltx_ylane.h with one lane group (CTC, ASG) and with four (13-bit slots)
    ("xlane_k10", ec._lx(10), None, 40, dict(engine=5, bt_record_bytes=2)),
    ("ylane_k10", ec._lx(10, scores=51, u=1), {"ylane": 2}, 40, dict(engine=6, ylane=1, bt_record_bytes=2)),
    ("ylane_k10_asg", ec._lx(10, crit="asg", scores=5), {"ylane": 2}, 30, dict(engine=6, ylane=1, bt_record_bytes=2)),
    ("ylane_groups4", ec._lx(10, scores=51, u=1), {"ylane": 2, "yshare": -1, "ylane_groups": 4}, 40,
     dict(engine=6, ylane=4, lane_groups=4, bt_record_bytes=4)),
    ("ylane_ngram_k100", ec._lx(100, lm=ec.WORD_LM, u=7), None, 30, dict(engine=6, bt_record_bytes=2)),
]


@pytest.mark.parametrize("name,c,sets,T,want", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_narrow_variant_is_bit_equal_to_the_oracle(sess, oracle_lib, name, c, sets, T, want):
    d = _check_batch(sess, oracle_lib, [_case(c, name, T)], sets)
    got = _engine(d)
    d.close()
    assert got["why_not_lane"] == 0 and got["redone"] == 0, got
    assert {k: got[k] for k in want} == want, got


@pytest.mark.parametrize("kb", [0, 64])
@pytest.mark.parametrize("T", [1, 2])
def test_shortest_utterances(sess, oracle_lib, T, kb):
    for c in (ec._lf(29, 50), ec._lf(29, 16, crit="asg", lm=ec.TOK_LM), ec._lx(10)):
        d = _check_batch(sess, oracle_lib, [_case(c, "short", T)], {"bt_lds_kb": kb})
        got = _engine(d)
        d.close()
        assert got["bt_record_bytes"] == 2 and got["redone"] == 0, got


@pytest.mark.parametrize("kb", [0, 64])
def test_ragged_batch(sess, oracle_lib, kb):
    """utterances of different lengths in one batch: the tile's rows are sized for the longest"""
    for c in (ec._lf(29, 50), ec._lf(29, 100, lm=ec.TOK_LM), ec._lx(10)):
        cs = [_case(dict(c, u=c["u"] + i), "ragged%d" % i, T) for i, T in enumerate((23, 1, 40, 0, 7, 39))]
        d = _check_batch(sess, oracle_lib, cs, {"bt_lds_kb": kb})
        got = _engine(d)
        d.close()
        assert got["bt_record_bytes"] in (2, 4) and got["redone"] == 0, got


def test_chunk_and_stretch_boundaries(sess, oracle_lib):
    """A small budget (bt_lds_kb = 4; 8 where the ASG transitions take 3.4 KB of it) makes chunks of a few dozen frames at lengths the emulator decodes quickly.  Every
    T of a contiguous range is decoded, so that the history's rows (T + 2) fall one below, at and one above a multiple
    of the record chunk, and the decoded frames (T) one below, at and one above a multiple of the emission stretch --
    asserted from the geometry the library reports, not assumed."""
    for c, kb, walked in ((ec._lf(29, 10), 4, True), (ec._lf(29, 10, crit="asg", lm=ec.TOK_LM, u=1), 8, False)):
        walk, score, most = set(), set(), 0
        for T in range(30, 151):
            d = _check_batch(sess, oracle_lib, [_case(c, "seam", T)], {"bt_lds_kb": kb})
            rec, F, Fe = d.get("bt_record_bytes"), d.get("bt_chunk_frames"), d.get("bt_stretch_frames")
            d.close()
            assert rec == 2 and F >= 8 and Fe >= 8, (T, rec, F, Fe)
            rows = T + 2
            if rows > F:
                walk.add({F - 1: "below", 0: "at", 1: "above"}.get(rows % F))
                most = max(most, (rows + F - 1) // F)
            if T > Fe:
                score.add({Fe - 1: "below", 0: "at", 1: "above"}.get(T % Fe))
        assert {"below", "at", "above"} <= score, score
        if walked:  # (the ASG case's 8 KB hold its whole history in one chunk: the seams of the stretches only)
            assert {"below", "at", "above"} <= walk, walk
            assert most >= 3, most


def test_a_budget_without_a_useful_chunk_yields(sess, oracle_lib):
    """bt_lds_kb = 1 holds fewer than 8 frames per chunk: the tunable yields to the large default, the decode does
    not fail and its results are the oracle's"""
    d = _check_batch(sess, oracle_lib, [_case(ec._lf(29, 50), "yield", 60)], {"bt_lds_kb": 1})
    F = d.get("bt_chunk_frames")
    d.close()
    assert F >= 8, F


def test_a_tile_beyond_the_budget_keeps_the_chunked_back_trace(sess, oracle_lib):
    """a long utterance under a small budget: no room for its token tile -> backtraceUtterance, same results"""
    d = _check_batch(sess, oracle_lib, [_case(ec._lf(29, 10), "long", 600)], {"bt_lds_kb": 4})
    got = _engine(d)
    d.close()
    assert got["bt_record_bytes"] == 0 and got["engine"] == 4, got


def test_plain_records_beside_packed_ones(sess, oracle_lib):
    """A packed batch in which one utterance -- neither the first nor the last -- was decoded again on the generic
    engine: its plain records take backtraceUtterance inside the narrow kernel's launch, the others stay narrow.
    The flagged utterance has a constant emission row, i.e. tied candidates, on which the reference's order is not a
    function of its inputs (the oracle and the generic engine differ there on the parent commit as well): it is
    compared bit for bit with a decode on the generic engine alone, every other utterance with the oracle."""
    from text_amd import synth
    N, T, B, flagged = 300, 12, 5, 2
    c = cases.case("wp_mixed", dist="ctc", T=T, N=N, K=20, Kt=30, u=515)
    e = synth.batch("ctc", B, T, N)
    e[flagged, 5, :] = -3.0
    d = sess.decoder(c, dict(tr=None))
    d.decode_batch(e, [T] * B, N)
    got = _engine(d)
    assert got["redone"] > 0 and got["engine"] == 4 and got["wlane"] == 1 and got["bt_record_bytes"] == 4, got
    g = sess.decoder(c, dict(tr=None))
    g.set("wlane", 0)
    g.decode_batch(e, [T] * B, N)
    assert g.get("engine") != 4 and g.get("bt_record_bytes") == 0
    for b in range(B):
        want = g.results(b) if b == flagged else \
            helpers.run_checker(oracle_lib, c, dict(e=np.ascontiguousarray(e[b]), tr=None, lex=None))
        ok, why = helpers.hyps_equal(want, d.results(b), score_tol=0.0)
        assert ok, "utterance %d: %s" % (b, why)
    d.close()
    g.close()
