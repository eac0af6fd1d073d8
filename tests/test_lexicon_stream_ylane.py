"""Lexicon stream chunks with the LM terms on the lane = (LM state, trie node) engine (fltx_ylane.h, ST; tunable
"ystream" = 1): an n-gram word LM and / or a smeared trie, the beam restored from and parked in the generic engine's
format around every chunk, LM-state ids and n-gram contexts in its tables.  Expectations: the compiled reference's own
traces (tests/golden/streaming_expected.json.gz) and the oracle, event by event -- every getBestHypothesis, every pruned
buffer and the final n-best, scores as hex."""
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

Y1 = [("ystream", 1)]
INF = float("inf")


@pytest.fixture(scope="module")
def stream_golden():
    with gzip.open(os.path.join(helpers.GOLDEN_DIR, "streaming_expected.json.gz"), "rt") as f:
        return json.load(f)


def _chosen(session, c, inp, threads=None, sets=Y1, key="ystream"):
    """`key` as fltx_stream_begin leaves it: the lane groups of the chunks' kernel, or 0"""
    d = session.decoder(c, inp, threads)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(1, c["N"], c["T"] + 4)
    on = int(d.get(key))
    d.close()
    return on


def _trace(session, c, want, chunks, lbs, threads, groups):
    inp = helpers.case_inputs(c)
    assert _chosen(session, c, inp, threads) == groups
    got, _ = ss.trace_device(session, c, inp, chunks, lbs, threads, Y1)
    assert ss.first_difference(want, got) is None, ss.first_difference(want, got)
    assert session.last_stream_redone == 0


def test_reference_trace_emulated(emu_session, stream_golden):
    name = "ng_word_t60_k16_4g"
    _trace(emu_session, cases.BY_NAME[name], stream_golden[name], *ss.SCENARIOS[name], 64, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ng_word_t60_k16_4g", "lx_scores_t50"])
def test_reference_trace(gpu_session, stream_golden, name):
    _trace(gpu_session, cases.BY_NAME[name], stream_golden[name], *ss.SCENARIOS[name], None, 1)


@pytest.mark.gpu
def test_c4_shape(gpu_session, oracle_lib):
    """bench.py's C4: the 90k-word trie, the 4-gram, beam 100 (two lane groups), 1 500 frames"""
    c = cases.BY_NAME["C4_spell_u1"]
    chunks, lbs = [200, 100, 300, 150, 250, 500], [0, 20, 5, 50]
    _trace(gpu_session, c, ss.trace_checker(oracle_lib, c, helpers.case_inputs(c), chunks, lbs), chunks, lbs, None, 2)


PATTERNS = [([3, 9, 1, 12, 20, 30], [0, 2, 0, 5]), ([1] * 60, [0]), ([25, 25, 25], [3, 1])]
GRID = list(itertools.product([1, 3, 16, 64, 100, 128], [2.0, 25.0, INF], [None, 5], [7, 60], ["lexspell", "uniform"],
                              [0, 1, 2], [0.0, -0.6]))
LMS = [dict(lm=("ngram", 3, 300), lm_weight=1.3, word_score=0.7), dict(lm=("ngram", 4, 300), lm_weight=2.0, word_score=2.0),
       dict(lm_weight=1.5, word_score=1.0, label_scores=33)]


def _grid(session, oracle_lib, pattern, every, threads):
    """Configurations i = pattern (mod 3) of GRID, every `every`-th of them; with [1] * 60 restore and park run around
    each frame.  None of the 864 has two equal scores in one buffer (the oracle run alone over the grid), so none is
    left out."""
    chunks, lbs = PATTERNS[pattern]
    bad = []
    for i, (K, thr, Kt, T, dist, lm, sil) in list(enumerate(GRID))[pattern::3][::every]:
        kw = dict(LMS[lm])
        if "lm" in kw:
            kw["lm"] = kw["lm"][:2] + (300 + i,)
        c = cases.case("ys%d" % i, kind="lexicon", dist=dist, u=1700 + i, T=T, N=29, K=K, Kt=Kt, thr=thr, sil_score=sil,
                       lexicon=cases.SMALL_LEX, **kw)
        inp = helpers.case_inputs(c)
        want = ss.trace_checker(oracle_lib, c, inp, chunks, lbs)
        assert not ss.has_ties(want), i
        d = session.decoder(c, inp, threads)
        d.set("ystream", 1)
        d.stream_begin(1, c["N"], c["T"] + 4)
        on = int(d.get("ystream"))
        d.close()
        got, _ = ss.trace_device(session, c, inp, chunks, lbs, threads, Y1)
        diff = ss.first_difference(want, got)
        if diff or session.last_stream_redone or on != (1 if K <= 64 else 2):
            bad.append((i, K, thr, Kt, T, dist, lm, sil, on, diff, session.last_stream_redone))
    assert not bad, bad[:3]


@pytest.mark.parametrize("pattern", [0, 1, 2])
def test_grid_against_the_oracle_emulated(emu_session, oracle_lib, pattern):
    _grid(emu_session, oracle_lib, pattern, 35, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", [0, 1, 2])
def test_grid_against_the_oracle(gpu_session, oracle_lib, pattern):
    _grid(gpu_session, oracle_lib, pattern, 5, None)


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
    assert d.get("ystream") == 1
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
    chunk: every restore meets renumbered gState / gSPar, every fresh id may land on a stale stateCtx row."""
    c = cases.case("ys_recycle", kind="lexicon", dist="lexspell", u=3, T=600, N=29, K=12, lexicon=cases.SMALL_LEX,
                   lm=("ngram", 3, 77), lm_weight=1.3, word_score=0.7)
    inp = helpers.case_inputs(c)
    _streams_against_oracles(session, oracle_lib, c, inp, [inp["e"]], [[25]] * 24, 208,
                             Y1 + [("compact_always", 1)], 0, threads)


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
    c = cases.BY_NAME["ng_word_t60_k16_4g"]
    inp = helpers.case_inputs(c)
    Ts = [c["T"], c["T"] // 2, c["T"] - 3]
    es = [synth.emissions(c["dist"], 900 + b, Ts[b], c["N"], lexicon=inp["lex"]) for b in range(3)]
    plan, done = [], [0, 0, 0]
    for row in RAGGED:
        plan.append([min(row[b], Ts[b] - done[b]) for b in range(3)])
        done = [done[b] + plan[-1][b] for b in range(3)]
    _streams_against_oracles(session, oracle_lib, c, inp, es, plan, max(Ts) + 4, Y1, None, threads)


def test_ragged_parallel_streams_emulated(emu_session, oracle_lib):
    _ragged(emu_session, oracle_lib, 64)


@pytest.mark.gpu
def test_ragged_parallel_streams(gpu_session, oracle_lib):
    _ragged(gpu_session, oracle_lib, None)


NOT_TAKEN = [("ng_word_t60_k16_4g", [], {}), ("ng_word_unk_t40", Y1, {}), ("ng_word_logadd_t40", Y1, {}),
             ("ml_word_t60_k16", Y1, {}), ("ng_tok_lexicon_t40", Y1, {}),
             ("ng_word_t60_k16_4g", Y1 + [("stream_optimistic", 0)], {}), ("ng_word_t60_k16_4g", Y1, {"K": 129})]


@pytest.mark.parametrize("name,sets,change", NOT_TAKEN, ids=["%s-%d%s" % (n, len(s), ch.get("K", "")) for n, s, ch in NOT_TAKEN])
def test_not_taken_emulated(emu_session, oracle_lib, name, sets, change):
    """Off unless asked for; asked for, not taken with <unk>, logAdd, several words per spelling, a token-level LM, a
    stream that is not optimistic, beam 129 -- and such a stream still decodes to the oracle's trace."""
    c = dict(cases.BY_NAME[name], **change)
    c["name"] = "%s_ys%d" % (name, len(change))
    inp = helpers.case_inputs(c)
    assert _chosen(emu_session, c, inp, 64, sets) == 0
    if sets:
        chunks, lbs = PATTERNS[2][0] if c["T"] > 60 else [c["T"] // 2, c["T"] - c["T"] // 2], [0, 2]
        want = ss.trace_checker(oracle_lib, c, inp, chunks, lbs)
        got, _ = ss.trace_device(emu_session, c, inp, chunks, lbs, 64, sets)
        assert ss.first_difference(want, got) is None


def test_taken_emulated(emu_session):
    """one lane group up to beam 64, two from 65; where fltx_xlane.h takes the stream as well, it keeps it"""
    c = cases.BY_NAME["ng_word_t60_k16_4g"]
    for K, groups in ((64, 1), (65, 2)):
        ck = dict(c, name="ys_k%d" % K, K=K)
        assert _chosen(emu_session, ck, helpers.case_inputs(ck), 64) == groups
    c = cases.BY_NAME["lx_spell_t60_k12_full"]
    both = Y1 + [("xstream", 1)]
    assert _chosen(emu_session, c, helpers.case_inputs(c), 64, both) == 0
    assert _chosen(emu_session, c, helpers.case_inputs(c), 64, both, "xstream") > 0
