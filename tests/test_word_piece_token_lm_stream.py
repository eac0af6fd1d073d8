"""Word-piece stream chunks with a token n-gram LM on the lane = LM state engine (fltx_wlane.h, ST + TL; tunable
"wtstream" = 1): the LM scores and n-gram contexts of the beam restored from and parked in the generic engine's format
around every chunk, the LM asked through the filter and a score memo that lives for one chunk.  Every expectation is the
oracle's trace, event by event -- every getBestHypothesis, every pruned buffer and the final n-best, scores as hex."""
import itertools

import pytest

import cases
import helpers
import stream_scenarios as ss
from test_word_piece_stream import _device, _oracle
from text_amd._capi import FLTX_WHY_STREAM

W1 = [("wtstream", 1)]
PATTERNS = [([1] * 60, [0]), ([3, 9, 1, 12, 20, 30], [0, 2, 0, 5])]
CELLS = list(itertools.product([65, 300, 1025], [1, 7, 64]))
INNER = list(itertools.product([5, 64], [2, 3, 4], [0.8, -0.5], [3.0, float("inf")], ["ctc", "asg"]))
LM3 = dict(dist="ctc", lm=("ngram", 3, 10), lm_weight=0.8)


def _grid(session, oracle_lib, pattern, picks, threads):
    """`picks` = (N, K, index into INNER) configurations under one chunk pattern; with [1] * 60 restore and park run around
    every frame.  A trace with two equal scores in one buffer is left out (their order is not defined): the oracle alone
    over the 2 x 9 cells of 48 leaves out 1 of cell (1025, 64) under either pattern and none elsewhere."""
    chunks, lbs = PATTERNS[pattern]
    ran, bad = 0, []
    for N, K, i in picks:
        Kt, order, lmw, thr, crit = INNER[i]
        c = cases.case("wts%d" % i, dist="ctc", u=800 + i, T=60, N=N, K=K, Kt=Kt, thr=thr, lm_weight=lmw, crit=crit,
                       trans_seed=(31 if crit == "asg" else None), lm=("ngram", order, 7 + order))
        inp = helpers.case_inputs(c)
        want = ss.trace_checker(oracle_lib, c, inp, chunks, lbs)
        if ss.has_ties(want):
            continue
        chosen = _served(session, c, inp, W1, threads)[0]
        got, _ = ss.trace_device(session, c, inp, chunks, lbs, threads, W1)
        ran += 1
        diff = ss.first_difference(want, got)
        if diff or session.last_stream_redone or chosen <= 0:
            bad.append((N, K, Kt, order, lmw, thr, crit, diff, session.last_stream_redone, chosen))
    assert not bad, bad[:3]
    return ran


@pytest.mark.parametrize("pattern", [0, 1])
def test_grid_against_the_oracle_emulated(emu_session, oracle_lib, pattern):
    every = [(N, K, i) for (N, K) in CELLS for i in range(len(INNER))][7 * pattern::61]
    assert _grid(emu_session, oracle_lib, pattern, every, 64) >= len(every) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,cell", list(itertools.product([0, 1], CELLS)))
def test_grid_against_the_oracle(gpu_session, oracle_lib, pattern, cell):
    ran = _grid(gpu_session, oracle_lib, pattern, [cell + (i,) for i in range(len(INNER))], None)
    assert ran >= 44, ran  # (of a cell's 48: at most a tenth left out)


def _served(session, c, inp, sets, threads, B=1):
    """("wtstream", "wstream", "why_not_lane") of a stream just begun under `sets`"""
    d = session.decoder(c, inp, threads)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(B, c["N"], 64)
    out = (d.get("wtstream"), d.get("wstream"), d.get("why_not_lane"))
    d.close()
    return out


FIXTURES = [("emu_session", 64), pytest.param("gpu_session", None, marks=pytest.mark.gpu)]


@pytest.mark.parametrize("fixture,threads", FIXTURES)
def test_ids_recycled_between_chunks(request, oracle_lib, fixture, threads):
    """600 frames in 25-frame chunks with prune(0) through a 208-frame buffer, the LM-state ids renumbered before every
    chunk: every restore reads stateCtx rows that moved with their ids, and a memo entry kept from the chunk before would
    answer for another state."""
    c = cases.case("wts_recycle", u=3, T=600, N=300, K=12, Kt=30, **LM3)
    inp = helpers.case_inputs(c)
    session = request.getfixturevalue(fixture)
    sets = W1 + [("compact_always", 1)]
    _, best, final, redone = _device(session, c, inp, [inp["e"]], [[25]] * 24, 208, sets, 0, threads)
    assert _served(session, c, inp, W1, threads)[0] > 0 and redone == 0
    assert (best[0], final[0]) == _oracle(oracle_lib, c, inp, inp["e"], [25] * 24, 0)


@pytest.mark.parametrize("fixture,threads", FIXTURES)
def test_the_switch(request, oracle_lib, fixture, threads):
    """"wtstream" = 0: the generic engine and the reason of today; 1: the engine, no reason left, the same trace -- the
    oracle's; on a ZeroLM decoder the key changes nothing"""
    session = request.getfixturevalue(fixture)
    c = cases.case("wts_switch", u=43, T=40, N=300, K=20, Kt=30, sil_score=-0.7, **LM3)
    inp = helpers.case_inputs(c)
    plan = [[7], [13], [1], [19]]
    W0 = [("wtstream", 0)]
    off = _device(session, c, inp, [inp["e"]], plan, 44, W0, 0, threads)
    on = _device(session, c, inp, [inp["e"]], plan, 44, W1, 0, threads)
    s0, s1 = _served(session, c, inp, W0, threads), _served(session, c, inp, W1, threads)
    assert s0[:2] == (0, 0) and s0[2] & FLTX_WHY_STREAM, s0
    assert s1[0] > 0 and s1[1:] == (0, 0) and on[3] == 0, (s1, on[3])
    assert on[1:3] == off[1:3]
    assert (on[1][0], on[2][0]) == _oracle(oracle_lib, c, inp, inp["e"], [7, 13, 1, 19], 0)
    z = dict(c, lm="zero", lm_weight=0.0)
    zin = helpers.case_inputs(z)
    z0 = _device(session, z, zin, [zin["e"]], plan, 44, [], 0, threads)
    z1 = _device(session, z, zin, [zin["e"]], plan, 44, W1, 0, threads)
    assert z1 == z0 and _served(session, z, zin, W1, threads)[0] == 0


@pytest.mark.parametrize("fixture,threads", FIXTURES)
def test_fallback(request, oracle_lib, fixture, threads):
    """One frame of stream 1 has all values equal -- no defined token beam: that chunk, and no other, is decoded again on
    the general path; stream 0 equals the oracle, stream 1 the same decoder with "wtstream" 0."""
    session = request.getfixturevalue(fixture)
    c = cases.case("wts_fallback", u=7, T=40, N=300, K=12, Kt=30, **LM3)
    inp = helpers.case_inputs(c)
    es = [inp["e"], helpers.case_inputs(dict(c, u=8))["e"].copy()]
    es[1][17, :] = -3.0
    plan = [[10, 10]] * 4
    _, best, final, redone = _device(session, c, inp, es, plan, 44, W1, 0, threads)
    assert _served(session, c, inp, W1, threads, 2)[0] > 0 and redone == 1
    assert (best[0], final[0]) == _oracle(oracle_lib, c, inp, es[0], [10] * 4, 0)
    _, best0, final0, _ = _device(session, c, inp, es, plan, 44, [("wtstream", 0)], 0, threads)
    assert (best[1], final[1]) == (best0[1], final0[1])
