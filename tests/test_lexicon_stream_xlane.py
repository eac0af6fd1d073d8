"""Lexicon stream chunks on the lane = (LM state, trie node) engine (fltx_xlane.h, ST; tunable "xstream" = 1): the beam
restored from and parked in the generic engine's format around every chunk, LM-state ids from its table.  Expectations:
the compiled reference's own traces (tests/golden/streaming_expected.json.gz) and the oracle, event by event -- every
getBestHypothesis, every pruned buffer and the final n-best, scores as hex."""
import gzip
import itertools
import json
import os

import numpy as np
import pytest

import cases
import helpers
import stream_scenarios as ss
from oracle import orclib

X1 = [("xstream", 1)]


@pytest.fixture(scope="module")
def stream_golden():
    with gzip.open(os.path.join(helpers.GOLDEN_DIR, "streaming_expected.json.gz"), "rt") as f:
        return json.load(f)


def _chosen(session, c, inp, threads=None, sets=X1):
    """"xstream" as fltx_stream_begin leaves it: the positions per token wave of the chunks' kernel, or 0"""
    d = session.decoder(c, inp, threads)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(1, c["N"], c["T"] + 4)
    on = int(d.get("xstream"))
    d.close()
    return on


def _reference_trace(session, stream_golden, name, threads):
    c = cases.BY_NAME[name]
    inp = helpers.case_inputs(c)
    chunks, lbs = ss.SCENARIOS[name]
    assert _chosen(session, c, inp, threads) > 0
    got, _ = ss.trace_device(session, c, inp, chunks, lbs, threads, X1)
    assert ss.first_difference(stream_golden[name], got) is None, ss.first_difference(stream_golden[name], got)
    assert session.last_stream_redone == 0


def test_reference_trace_emulated(emu_session, stream_golden):
    # (threads = 64 is the generic kernels' begin / prune / end; the chunks run at the chosen geometry's 576)
    _reference_trace(emu_session, stream_golden, "lx_spell_t60_k12_full", 64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lx_spell_t60_k12_full", "C3_spell_u0"])
def test_reference_trace(gpu_session, stream_golden, name):
    _reference_trace(gpu_session, stream_golden, name, None)


PATTERNS = [([3, 9, 1, 12, 20, 30], [0, 2, 0, 5]), ([1] * 60, [0]), ([25, 25, 25], [3, 1])]
GRID = list(itertools.product([1, 3, 12, 50, 64], [2.0, 25.0, float("inf")], [None, 5, 10], [7, 60],
                              ["lexspell", "uniform"], [0.0, -0.6]))


def _grid(session, oracle_lib, pattern, every, threads):
    """Configurations i = pattern (mod 3) of GRID, every `every`-th of them (the GPU runs all 120 of each pattern, the
    emulator 8 of them, which still meet every value of every axis): with [1] * 60 every frame is a launch's last, so restore and park run around each frame.  A trace with two equal scores in one buffer would be
    left out (their order is not defined): with these seeds none of the 360 has one (the oracle run alone over the
    grid), so none is."""
    chunks, lbs = PATTERNS[pattern]
    tried, ran, bad = 0, 0, []
    for i, (K, thr, Kt, T, dist, sil) in list(enumerate(GRID))[pattern::3][::every]:
        c = cases.case("xs%d" % i, kind="lexicon", dist=dist, u=700 + i, T=T, N=29, K=K, Kt=Kt, thr=thr, sil_score=sil,
                       lexicon=cases.SMALL_LEX)
        inp = helpers.case_inputs(c)
        want = ss.trace_checker(oracle_lib, c, inp, chunks, lbs)
        tried += 1
        if ss.has_ties(want):
            continue
        got, _ = ss.trace_device(session, c, inp, chunks, lbs, threads, X1)
        ran += 1
        d = ss.first_difference(want, got)
        if d or session.last_stream_redone:
            bad.append((i, K, thr, Kt, T, dist, sil, d, session.last_stream_redone))
    assert not bad, bad[:3]
    assert 4 * ran >= 3 * tried, (ran, tried)


@pytest.mark.parametrize("pattern", [0, 1, 2])
def test_grid_against_the_oracle_emulated(emu_session, oracle_lib, pattern):
    _grid(emu_session, oracle_lib, pattern, 17, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", [0, 1, 2])
def test_grid_against_the_oracle(gpu_session, oracle_lib, pattern):
    _grid(gpu_session, oracle_lib, pattern, 1, None)


def _streams_against_oracles(session, oracle_lib, c, inp, es, plan, max_frames, sets, prune, threads=None):
    """B streams of one decoder, stream b fed plan[step][b] frames of es[b] per call; after every call each stream's
    getBestHypothesis against an oracle decoder run on that stream alone, then prune(prune) if not None; final n-best."""
    B, N = len(es), c["N"]
    ods = [ss.checker_decoder(oracle_lib, c, inp) for _ in range(B)]
    for od, _, _ in ods:
        oracle_lib.decoder_begin(od)
    d = session.decoder(c, inp, threads)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(B, N, max_frames)
    assert d.get("xstream") > 0
    done = [0] * B
    for step, take in enumerate(plan):
        parts = [es[b][done[b]:done[b] + take[b]] for b in range(B)]
        d.stream_step(np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32), list(take))
        for b in range(B):
            if take[b]:
                oracle_lib.decoder_step(ods[b][0], orclib._fp(np.ascontiguousarray(parts[b])), take[b], N)
            done[b] += take[b]
            want, got = oracle_lib.best(ods[b][0], step % 3, 1024), d.best(b, step % 3, 1024)
            assert ss._enc_one(want) == ss._enc_one(got), "stream %d after call %d" % (b, step)
        if prune is not None:
            d.stream_prune(prune)
            for od, _, _ in ods:
                oracle_lib.decoder_prune(od, prune)
    d.stream_end()
    redone = d.get("stream_redone")
    for b in range(B):
        oracle_lib.decoder_end(ods[b][0])
        ok, why = helpers.hyps_equal(oracle_lib.collect(ods[b][0]), d.results(b))
        assert ok, "stream %d: %s" % (b, why)
        oracle_lib.decoder_destroy(ods[b][0])
    d.close()
    assert redone == 0


def _ids_recycled(session, oracle_lib, threads):
    """600 frames in 25-frame chunks with prune(0) through a 208-frame buffer, the LM-state ids renumbered before every
    chunk: every restore meets renumbered gState / gSPar."""
    c = cases.case("xs_recycle", kind="lexicon", dist="lexspell", u=3, T=600, N=29, K=12, lexicon=cases.SMALL_LEX)
    inp = helpers.case_inputs(c)
    _streams_against_oracles(session, oracle_lib, c, inp, [inp["e"]], [[25]] * 24, 208, X1 + [("compact_always", 1)],
                             0, threads)


def test_ids_recycled_between_chunks_emulated(emu_session, oracle_lib):
    _ids_recycled(emu_session, oracle_lib, 64)


@pytest.mark.gpu
def test_ids_recycled_between_chunks(gpu_session, oracle_lib):
    _ids_recycled(gpu_session, oracle_lib, None)


RAGGED = [[5, 0, 3], [7, 11, 1], [0, 4, 20], [30, 30, 30], [100, 100, 100]]


def _ragged(session, oracle_lib, threads):
    """Three streams, chunk lengths differing per stream; streams 0 and 1 are given no frame in one of the calls (T = 0:
    their parked beam stays as it is), and a stream that has ended gets none in the calls that follow."""
    from text_amd import synth
    c = cases.BY_NAME["lx_spell_t60_k12_full"]
    inp = helpers.case_inputs(c)
    Ts = [c["T"], c["T"] // 2, c["T"] - 3]
    es = [synth.emissions(c["dist"], 900 + b, Ts[b], c["N"], lexicon=inp["lex"]) for b in range(3)]
    plan, done = [], [0, 0, 0]
    for row in RAGGED:
        plan.append([min(row[b], Ts[b] - done[b]) for b in range(3)])
        done = [done[b] + plan[-1][b] for b in range(3)]
    _streams_against_oracles(session, oracle_lib, c, inp, es, plan, max(Ts) + 4, X1, None, threads)


def test_ragged_parallel_streams_emulated(emu_session, oracle_lib):
    _ragged(emu_session, oracle_lib, 64)


@pytest.mark.gpu
def test_ragged_parallel_streams(gpu_session, oracle_lib):
    _ragged(gpu_session, oracle_lib, None)


NOT_TAKEN = [("lx_scores_t50", X1), ("ng_word_t40_k10", X1), ("lx_spell_unk", X1), ("lx_spell_t60_k12_logadd", X1),
             ("lx_spell_t60_k12_full", X1 + [("stream_optimistic", 0)]), ("lx_spell_t60_k12_full", [])]


@pytest.mark.parametrize("name,sets", NOT_TAKEN, ids=[n + ("" if s == X1 else str(len(s))) for n, s in NOT_TAKEN])
def test_selection_emulated(emu_session, name, sets):
    """Off unless asked for; asked for, not taken with label scores in the trie, a word n-gram LM, <unk>, logAdd,
    a stream that is not optimistic -- nor at beam 65."""
    c = cases.BY_NAME[name]
    assert _chosen(emu_session, c, helpers.case_inputs(c), 64, sets) == 0
    if name == "lx_spell_t60_k12_full":
        c65 = dict(c, name="xs_k65", K=65)
        assert _chosen(emu_session, c65, helpers.case_inputs(c65), 64, X1) == 0
        assert _chosen(emu_session, c, helpers.case_inputs(c), 64, X1) == 5  # (29 tokens: six waves of five at 576)


def test_not_taken_stream_still_decodes_emulated(emu_session, oracle_lib):
    c = cases.BY_NAME["lx_scores_t50"]
    inp = helpers.case_inputs(c)
    chunks, lbs = ss.SCENARIOS["lx_scores_t50"]
    want = ss.trace_checker(oracle_lib, c, inp, chunks, lbs)
    got, _ = ss.trace_device(emu_session, c, inp, chunks, lbs, 64, X1)
    assert ss.first_difference(want, got) is None
