"""Word-piece CTC / ASG decode with a token n-gram LM on the lane = LM state engine (fltx_wlane.h, TL; tunable
"wtlane" = 1): token sets beyond 64, an LM term per new-token candidate asked through the n-gram tables (filtered,
memoised), the frame's best a reduction, lmWeight x finish in decodeEnd, the LM score of every path carried through the
frames.  Every expectation is the oracle's n-best: tokens exact, score / amScore / lmScore bit for bit."""
import itertools

import pytest

import cases
import helpers
from text_amd._capi import FLTX_WHY_LM

NS, KS, ORDERS, CRITS = [65, 300, 1025], [1, 7, 64], [2, 3, 4], ["ctc", "asg"]
INNER = list(itertools.product([1, 5, 64], [0.8, -0.5], [0.0, -0.7], [3.0, 25.0, float("inf")], [1, 2, 23, 60]))
SERVED = ("engine", "wlane", "wtlane", "redone")
LONG = dict(dist="ctc", K=50, Kt=30, lm=("ngram", 3, 10), lm_weight=0.8)  # (and the switch's and the batch's LM)


def _grid(session, oracle_lib, N, K, order, crit, every):
    """The 144 configurations (token beam x lm_weight x sil_score x thr x T) of one (N, K, order, criterion), every
    `every`-th of them.  A configuration whose oracle n-best holds two equal scores is left out (their order is not
    defined): the oracle alone over the whole grid of 7 776 leaves out 0."""
    ran, bad = 0, []
    for i, (Kt, lmw, sil, thr, T) in list(enumerate(INNER))[::every]:
        c = cases.case("wt%d" % i, dist="ctc", u=700 + i, T=T, N=N, K=K, Kt=Kt, thr=thr, lm_weight=lmw, sil_score=sil,
                       crit=crit, trans_seed=(31 if crit == "asg" else None), lm=("ngram", order, 7 + order))
        inp = helpers.case_inputs(c)
        want = helpers.run_checker(oracle_lib, c, inp)
        if len({h.score for h in want}) != len(want):
            continue
        d = session.decoder(c, inp)
        d.set("wtlane", 1)
        d.decode_batch(inp["e"], [T], N)
        ok, why = helpers.hyps_equal(want, d.results(0))
        served = tuple(d.get(k) for k in SERVED)
        ran += 1
        if not ok or served != (4, 1, 1, 0):
            bad.append((i, Kt, lmw, sil, thr, T, why, served))
        d.close()
    assert not bad, bad[:3]
    assert ran >= (130 if every == 1 else 5), ran  # (of a cell's 144: at most a tenth left out; the emulator's 5: none)


@pytest.mark.parametrize("N,K,order,crit", [(65, 7, 2, "ctc"), (300, 64, 3, "asg"), (1025, 1, 4, "ctc"), (300, 7, 4, "ctc")])
def test_grid_against_the_oracle_emulated(emu_session, oracle_lib, N, K, order, crit):
    _grid(emu_session, oracle_lib, N, K, order, crit, 29)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,order,crit", list(itertools.product(NS, KS, ORDERS, CRITS)))
def test_grid_against_the_oracle(gpu_session, oracle_lib, N, K, order, crit):
    _grid(gpu_session, oracle_lib, N, K, order, crit, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [300, 1024])
def test_states_re_enter_and_the_memo_evicts(gpu_session, oracle_lib, N):
    """200 frames at beam 50, token beam 30: LM states leave and re-enter the beam, the score memo's slots turn over."""
    c = cases.case("wt_long", u=41, T=200, N=N, **LONG)
    inp = helpers.case_inputs(c)
    want = helpers.run_checker(oracle_lib, c, inp)
    assert len({h.score for h in want}) == len(want)
    d = gpu_session.decoder(c, inp)
    d.set("wtlane", 1)
    d.decode_batch(inp["e"], [200], N)
    ok, why = helpers.hyps_equal(want, d.results(0))
    assert ok and tuple(d.get(k) for k in SERVED) == (4, 1, 1, 0), why
    d.close()


@pytest.mark.parametrize("fixture", ["emu_session", pytest.param("gpu_session", marks=pytest.mark.gpu)])
def test_the_switch(request, oracle_lib, fixture):
    """"wtlane" = 0: the generic engine (1) and the reason of today, and the n-best of "wtlane" = 1"""
    session = request.getfixturevalue(fixture)
    c = cases.case("wt_switch", u=43, T=23, N=300, sil_score=-0.7, **dict(LONG, K=20))
    inp = helpers.case_inputs(c)
    out = []
    for on in (0, 1):
        d = session.decoder(c, inp)
        d.set("wtlane", on)
        d.decode_batch(inp["e"], [23], 300)
        out.append((d.results(0), tuple(d.get(k) for k in SERVED), d.get("why_not_lane")))
        d.close()
    assert out[0][1] == (1, 0, 0, 0) and out[0][2] & FLTX_WHY_LM, out[0][1:]
    assert out[1][1] == (4, 1, 1, 0) and out[1][2] == 0, out[1][1:]
    ok, why = helpers.hyps_equal(out[0][0], out[1][0])
    assert ok, why
    ok, why = helpers.hyps_equal(helpers.run_checker(oracle_lib, c, inp), out[1][0])
    assert ok, why


@pytest.mark.gpu
def test_batch_with_a_row_without_a_defined_token_beam(gpu_session, oracle_lib):
    """test_word_piece_row_without_a_defined_token_beam's batch under the token LM: utterance 1 is redone on the general
    engines and equals what they return for the whole batch; the others keep their lane results."""
    from text_amd import synth
    N, T, B = 300, 40, 5
    c = cases.case("wt_ties", u=515, T=T, N=N, **dict(LONG, K=20))
    inp = helpers.case_inputs(c)
    e = synth.batch("ctc", B, T, N)
    e[1, 9, :] = -3.0
    res = []
    for on in (1, 0):
        d = gpu_session.decoder(c, inp)
        d.set("wtlane", on)
        d.decode_batch(e, [T] * B, N)
        res.append([d.results(b) for b in range(B)])
        assert tuple(d.get(k) for k in SERVED) == ((4, 1, 1, 1) if on else (1, 0, 0, 0))
        d.close()
    for b in range(B):
        ok, why = helpers.hyps_equal(res[1][b], res[0][b])
        assert ok, "utterance %d vs the general engines: %s" % (b, why)
    for b in (0, 2, 3, 4):
        want = helpers.run_checker(oracle_lib, c, dict(e=e[b], tr=None, lex=None))
        if len({h.score for h in want}) == len(want):
            ok, why = helpers.hyps_equal(want, res[0][b])
            assert ok, "utterance %d: %s" % (b, why)
