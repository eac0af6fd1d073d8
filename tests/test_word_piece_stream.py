"""Word-piece stream chunks on the lane = LM state engine (fltx_wlane.h, ST; tunable "wstream" = 1): token sets beyond
64, the token beams of a call's rows from the front-end kernel, the beam restored from and parked in the generic engine's
format around every chunk, LM-state ids from its table.  Every expectation is the oracle's trace, event by event --
every getBestHypothesis, every pruned buffer and the final n-best, scores as hex."""
import itertools

import numpy as np
import pytest

import cases
import helpers
import stream_scenarios as ss
from oracle import orclib

W1 = [("wstream", 1)]
PATTERNS = [([3, 9, 1, 12, 20, 30], [0, 2, 0, 5]), ([1] * 60, [0]), ([25, 25, 25], [3, 1])]
GRID = list(itertools.product([1, 3, 20, 50, 64], [2.0, 25.0, float("inf")], [5, 30, 64], [(65, 40), (300, 60)],
                              ["ctc", "uniform"], [0.0, -0.6]))


def _grid(session, oracle_lib, pattern, every, threads):
    """Configurations i = pattern (mod 3) of GRID, every `every`-th of them; with [1] * 60 restore and park run around
    every frame.  A trace with two equal scores in one buffer is left out (their order is not defined): the oracle alone
    over the grid leaves out 3, 5 and 4 of the 120 per pattern."""
    chunks, lbs = PATTERNS[pattern]
    tried, ran, bad = 0, 0, []
    for i, (K, thr, Kt, (N, T), dist, sil) in list(enumerate(GRID))[pattern::3][::every]:
        c = cases.case("ws%d" % i, dist=dist, u=900 + i, T=T, N=N, K=K, Kt=Kt, thr=thr, sil_score=sil)
        inp = helpers.case_inputs(c)
        want = ss.trace_checker(oracle_lib, c, inp, chunks, lbs)
        tried += 1
        if ss.has_ties(want):
            continue
        d = session.decoder(c, inp, threads)
        d.set("wstream", 1)
        d.stream_begin(1, N, T + 4)
        chosen = d.get("wstream")
        d.close()
        got, _ = ss.trace_device(session, c, inp, chunks, lbs, threads, W1)
        ran += 1
        diff = ss.first_difference(want, got)
        if diff or session.last_stream_redone or chosen <= 0:
            bad.append((i, K, thr, Kt, N, T, dist, sil, diff, session.last_stream_redone, chosen))
    assert not bad, bad[:3]
    assert ran >= (110 if every == 1 else 1), (ran, tried)  # (of the 120 of a pattern; the emulator runs 8 of them)


@pytest.mark.parametrize("pattern", [0, 1, 2])
def test_grid_against_the_oracle_emulated(emu_session, oracle_lib, pattern):
    _grid(emu_session, oracle_lib, pattern, 17, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", [0, 1, 2])
def test_grid_against_the_oracle(gpu_session, oracle_lib, pattern):
    _grid(gpu_session, oracle_lib, pattern, 1, None)


def _device(session, c, inp, es, plan, max_frames, sets, prune, threads):
    """B streams of one decoder, stream b fed plan[step][b] frames of es[b] per call: each stream's getBestHypothesis
    after every call, then prune(prune) if not None; the final n-best; "wstream" after begin and the chunks redone."""
    B, N = len(es), c["N"]
    d = session.decoder(c, inp, threads)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(B, N, max_frames)
    chosen, done, best = d.get("wstream"), [0] * B, [[] for _ in range(B)]
    for step, take in enumerate(plan):
        parts = [es[b][done[b]:done[b] + take[b]] for b in range(B)]
        d.stream_step(np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32), list(take))
        for b in range(B):
            done[b] += take[b]
            best[b].append(ss._enc_one(d.best(b, step % 3, 1024)))
        if prune is not None:
            d.stream_prune(prune)
    d.stream_end()
    final = [helpers.encode_hyps(d.results(b), True) for b in range(B)]
    redone = d.get("stream_redone")
    d.close()
    return chosen, best, final, redone


def _oracle(oracle_lib, c, inp, e, takes, prune):
    """... the same for one stream alone on an oracle decoder of its own"""
    od = ss.checker_decoder(oracle_lib, c, inp)[0]
    oracle_lib.decoder_begin(od)
    done, best = 0, []
    for step, n in enumerate(takes):
        if n:
            oracle_lib.decoder_step(od, orclib._fp(np.ascontiguousarray(e[done:done + n])), n, c["N"])
        done += n
        best.append(ss._enc_one(oracle_lib.best(od, step % 3, 1024)))
        if prune is not None:
            oracle_lib.decoder_prune(od, prune)
    oracle_lib.decoder_end(od)
    final = helpers.encode_hyps(oracle_lib.collect(od), True)
    oracle_lib.decoder_destroy(od)
    return best, final


def _ids_recycled(session, oracle_lib, threads):
    """600 frames in 25-frame chunks with prune(0) through a 208-frame buffer, the LM-state ids renumbered before every
    chunk: every restore meets renumbered gState / gSPar."""
    c = cases.case("ws_recycle", u=3, T=600, N=300, K=12, Kt=30)
    inp = helpers.case_inputs(c)
    chosen, best, final, redone = _device(session, c, inp, [inp["e"]], [[25]] * 24, 208, W1 + [("compact_always", 1)],
                                          0, threads)
    assert chosen > 0 and redone == 0
    assert (best[0], final[0]) == _oracle(oracle_lib, c, inp, inp["e"], [25] * 24, 0)


def test_ids_recycled_between_chunks_emulated(emu_session, oracle_lib):
    _ids_recycled(emu_session, oracle_lib, 64)


@pytest.mark.gpu
def test_ids_recycled_between_chunks(gpu_session, oracle_lib):
    _ids_recycled(gpu_session, oracle_lib, None)


RAGGED = [[5, 0, 3, 1], [7, 11, 1, 0], [0, 4, 20, 9], [30, 30, 30, 30], [100, 100, 100, 100]]


@pytest.mark.gpu
def test_ragged_streams_and_wide_rows(gpu_session, oracle_lib):
    """Four streams over 1 100 tokens (two 1 024-token chunks of the front end, tokens beyond a byte), chunk lengths
    differing per stream and call, 0 among them; stream 1 has ended by the last call."""
    c = cases.case("ws_ragged", u=5, T=70, N=1100, K=20, Kt=30)
    inp = helpers.case_inputs(c)
    Ts = [70, 35, 67, 52]
    es = [helpers.case_inputs(dict(c, u=950 + b, T=Ts[b]))["e"] for b in range(4)]
    plan, done = [], [0] * 4
    for row in RAGGED:
        plan.append([min(row[b], Ts[b] - done[b]) for b in range(4)])
        done = [done[b] + plan[-1][b] for b in range(4)]
    chosen, best, final, redone = _device(gpu_session, c, inp, es, plan, max(Ts) + 4, W1, None, None)
    assert chosen > 0 and redone == 0
    for b in range(4):
        assert (best[b], final[b]) == _oracle(oracle_lib, c, inp, es[b], [p[b] for p in plan], None), "stream %d" % b


def _fallback(session, oracle_lib, threads):
    """One frame of stream 1 has all values equal -- no defined token beam: that chunk, and no other, is decoded again on
    the general path; stream 0 equals the oracle, stream 1 the same decoder with "wstream" 0."""
    c = cases.case("ws_fallback", u=7, T=40, N=300, K=12, Kt=30)
    inp = helpers.case_inputs(c)
    es = [inp["e"], helpers.case_inputs(dict(c, u=8))["e"].copy()]
    es[1][17, :] = -3.0
    plan = [[10, 10]] * 4
    chosen, best, final, redone = _device(session, c, inp, es, plan, 44, W1, 0, threads)
    assert chosen > 0 and redone == 1
    assert (best[0], final[0]) == _oracle(oracle_lib, c, inp, es[0], [10] * 4, 0)
    chosen0, best0, final0, _ = _device(session, c, inp, es, plan, 44, [("wstream", 0)], 0, threads)
    assert chosen0 == 0 and (best[1], final[1]) == (best0[1], final0[1])


def test_fallback_emulated(emu_session, oracle_lib):
    _fallback(emu_session, oracle_lib, 64)


@pytest.mark.gpu
def test_fallback(gpu_session, oracle_lib):
    _fallback(gpu_session, oracle_lib, None)
