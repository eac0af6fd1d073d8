"""Word-piece CTC / ASG decode with logAdd merges on the lane = LM state engine (fltx_wlane.h, LA; tunable "wlogadd" = 1):
token sets beyond 64, the members of a merge group log-added in descending order, the frame's best priced from the best
surviving score, a state's two hypotheses finished into one -- under ZeroLM and, with "wtlane" = 1, with a token n-gram
LM.  Every expectation is the oracle's n-best with log_add: tokens exact, scores within 1e-5 (the logAdd contract)."""
import itertools

import numpy as np
import pytest

import cases
import helpers
from text_amd._capi import FLTX_WHY_LOGADD

TOL = 1e-5
NS, KS, CRITS = [65, 300, 1025], [1, 7, 64], ["ctc", "asg"]
INNER = list(itertools.product([1, 5, 64], [0.0, -0.7], [3.0, 25.0, float("inf")], [1, 2, 23, 60]))
LMS = list(itertools.product([2, 4], [0.8, -0.5]))
SERVED = ("engine", "wlane", "wlogadd", "redone")
LONG = dict(dist="ctc", K=50, Kt=30, log_add=True)
NGRAM3 = dict(lm=("ngram", 3, 10), lm_weight=0.8)
# Beams of 64 over 300 and more tokens end in 64 scores a few units apart, and a quarter of the seeds 900 + i leave two of
# them within 2e-5.  Searched on the CPU with the oracle alone: per configuration of those cells the first r of 0 .. 9
# whose seed 900 + i + 100 r has no near tie (a seed that ties is replaced, not excused).
RESEED = {(300, "ctc"): "000000000000000000000000001000150016000000010001000000020000004010100000",
          (300, "asg"): "000000000000000000000000001000150016000000010001000000020000004010100000",
          (1025, "ctc"): "000000000000000000000000000100400123000100010011102000000020002110100130",
          (1025, "asg"): "000000000000000000000000000100400123000100010011102000000020002310100130"}


def _near_tie(want):
    """two scores of the oracle's n-best closer than twice the tolerance: within it they may change places"""
    s = sorted(h.score for h in want)
    return any(b - a < 2 * TOL for a, b in zip(s, s[1:]))


def _grid(session, oracle_lib, N, K, crit, every, lms=((None, 0.0),)):
    """The 72 configurations (token beam x sil_score x thr x T) of one (N, K, criterion), times `lms` (n-gram order,
    lm_weight), every `every`-th of them.  A configuration with a near tie in the oracle's n-best is left out, at most a
    tenth of a cell.  The oracle alone over the whole grid: 6 of 1 296 under ZeroLM (at most 2 of a cell's 72), 1 of the
    token-LM cells' 1 728 (at most 1 of a cell's 288)."""
    ran, left, bad = 0, 0, []
    reseed = RESEED[(N, crit)] if (K == 64 and not lms[0][0] and (N, crit) in RESEED) else "0" * len(INNER)
    for i, ((order, lmw), (Kt, sil, thr, T)) in list(enumerate(itertools.product(lms, INNER)))[::every]:
        lm = dict(lm=("ngram", order, 7 + order), lm_weight=lmw) if order else {}
        c = cases.case("wla%d" % i, dist="ctc", u=900 + i + 100 * int(reseed[i % len(INNER)]), T=T, N=N, K=K, Kt=Kt, thr=thr,
                       sil_score=sil, crit=crit, log_add=True, trans_seed=(31 if crit == "asg" else None), **lm)
        inp = helpers.case_inputs(c)
        want = helpers.run_checker(oracle_lib, c, inp)
        if _near_tie(want):
            left += 1
            continue
        d = session.decoder(c, inp)
        d.set("wlogadd", 1)
        d.set("wtlane", 1 if order else 0)
        d.decode_batch(inp["e"], [T], N)
        ok, why = helpers.hyps_equal(want, d.results(0), TOL)
        served = tuple(d.get(k) for k in SERVED) + (d.get("wtlane"),)
        ran += 1
        if not ok or served != (4, 1, 1, 0, 1 if order else 0):
            bad.append((i, order, lmw, Kt, sil, thr, T, why, served))
        d.close()
    assert not bad, bad[:3]
    assert left * 10 <= ran + left, (ran, left)


@pytest.mark.parametrize("N,K,crit,lms", [(65, 7, "ctc", ((None, 0.0),)), (300, 64, "asg", ((None, 0.0),)),
                                          (1025, 1, "ctc", ((None, 0.0),)), (300, 64, "ctc", LMS)])
def test_grid_against_the_oracle_emulated(emu_session, oracle_lib, N, K, crit, lms):
    _grid(emu_session, oracle_lib, N, K, crit, 29, lms)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,crit", list(itertools.product(NS, KS, CRITS)))
def test_grid_against_the_oracle(gpu_session, oracle_lib, N, K, crit):
    _grid(gpu_session, oracle_lib, N, K, crit, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("NK,crit", list(itertools.product([(65, 7), (300, 64), (1025, 1)], CRITS)))
def test_token_lm_grid_against_the_oracle(gpu_session, oracle_lib, NK, crit):
    _grid(gpu_session, oracle_lib, NK[0], NK[1], crit, 1, LMS)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [300, 1024])
@pytest.mark.parametrize("lm", [{}, NGRAM3], ids=["zerolm", "3gram"])
def test_states_re_enter_and_merged_scores_overtake(gpu_session, oracle_lib, N, lm):
    """200 frames at beam 50, token beam 30: LM states leave and re-enter the beam, merged scores pass the frame's candidates"""
    c = cases.case("wla_long", u=54, T=200, N=N, **LONG, **lm)
    inp = helpers.case_inputs(c)
    want = helpers.run_checker(oracle_lib, c, inp)
    assert not _near_tie(want)
    d = gpu_session.decoder(c, inp)
    d.set("wlogadd", 1)
    d.set("wtlane", 1 if lm else 0)
    d.decode_batch(inp["e"], [200], N)
    ok, why = helpers.hyps_equal(want, d.results(0), TOL)
    assert ok and tuple(d.get(k) for k in SERVED) == (4, 1, 1, 0), why
    d.close()


@pytest.mark.parametrize("fixture", ["emu_session", pytest.param("gpu_session", marks=pytest.mark.gpu)])
def test_the_switch(request, oracle_lib, fixture):
    """"wlogadd" = 0: the generic engine (1) and the reason of today; 1: the lane engine, the same n-best, the oracle's"""
    session = request.getfixturevalue(fixture)
    c = cases.case("wla_switch", u=43, T=23, N=300, sil_score=-0.7, **dict(LONG, K=20))
    inp = helpers.case_inputs(c)
    out = []
    for on in (0, 1):
        d = session.decoder(c, inp)
        d.set("wlogadd", on)
        d.decode_batch(inp["e"], [23], 300)
        out.append((d.results(0), tuple(d.get(k) for k in SERVED), d.get("why_not_lane")))
        d.close()
    assert out[0][1] == (1, 0, 0, 0) and out[0][2] & FLTX_WHY_LOGADD, out[0][1:]
    assert out[1][1] == (4, 1, 1, 0) and out[1][2] == 0, out[1][1:]
    ok, why = helpers.hyps_equal(out[0][0], out[1][0], TOL)
    assert ok, why
    ok, why = helpers.hyps_equal(helpers.run_checker(oracle_lib, c, inp), out[1][0], TOL)
    assert ok, why


@pytest.mark.gpu
def test_typed_batch_reaches_the_logadd_kernel(gpu_session):
    """bf16 logits through fltx_decode_batch_typed with the key on, against the float32 decode of the same e (formed from
    the returned frame_lse)"""
    import ctypes as C
    from text_amd._capi import DTYPE_BF16
    N, T = 300, 23
    c = cases.case("wla_typed", u=47, T=T, N=N, **dict(LONG, K=20))
    inp = helpers.case_inputs(c)
    bits = (np.ascontiguousarray(inp["e"], dtype=np.float32).reshape(T, N).view(np.uint32) >> 16).astype(np.uint16)
    hip, lse_dev, lse = C.CDLL("libamdhip64.so"), C.c_void_p(), np.zeros(T)
    assert hip.hipMalloc(C.byref(lse_dev), C.c_size_t(lse.nbytes)) == 0
    res = []
    for typed in (True, False):
        d = gpu_session.decoder(c, inp)
        d.set("wlogadd", 1)
        if typed:
            d.decode_batch_typed(bits.ctypes.data, [T], N, kind="logits", frame_lse=lse_dev.value, dtype=DTYPE_BF16, on_device=0)
        else:
            assert hip.hipMemcpy(C.c_void_p(lse.ctypes.data), lse_dev, C.c_size_t(lse.nbytes), 2) == 0
            x = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
            d.decode_batch((x - lse[:, None]).astype(np.float32), [T], N)
        res.append(d.results(0))
        assert tuple(d.get(k) for k in SERVED) == (4, 1, 1, 0)
        d.close()
    hip.hipFree(lse_dev)
    ok, why = helpers.hyps_equal(res[1], res[0], TOL)
    assert ok and len(res[0]) > 0, why


@pytest.mark.gpu
def test_batch_with_a_row_without_a_defined_token_beam(gpu_session, oracle_lib):
    """Utterance 1 has a frame of equal values: it is redone on the general engines and equals what they return for the
    whole batch; the others keep their lane results."""
    from text_amd import synth
    N, T, B = 300, 40, 5
    c = cases.case("wla_ties", u=515, T=T, N=N, **dict(LONG, K=20))
    inp = helpers.case_inputs(c)
    e = synth.batch("ctc", B, T, N)
    e[1, 9, :] = -3.0
    res = []
    for on in (1, 0):
        d = gpu_session.decoder(c, inp)
        d.set("wlogadd", on)
        d.decode_batch(e, [T] * B, N)
        res.append([d.results(b) for b in range(B)])
        assert tuple(d.get(k) for k in SERVED) == ((4, 1, 1, 1) if on else (1, 0, 0, 0))
        d.close()
    for b in range(B):
        ok, why = helpers.hyps_equal(res[1][b], res[0][b], TOL)
        assert ok, "utterance %d vs the general engines: %s" % (b, why)
    for b in (0, 2, 3, 4):
        want = helpers.run_checker(oracle_lib, c, dict(e=e[b], tr=None, lex=None))
        if not _near_tie(want):
            ok, why = helpers.hyps_equal(want, res[0][b], TOL)
            assert ok, "utterance %d: %s" % (b, why)
