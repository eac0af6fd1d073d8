"""fltx_stream_finish: single streams of a classic stream batch (fltx_stream_* on the lexicon-free and lexicon decoders)
end and restart while the others decode on.  Every scenario is written once and run on the emulator and on the device;
the yardstick is the oracle, run on each utterance alone (stream_scenarios.checker_decoder), never the device."""
import ctypes as C

import numpy as np
import pytest

import cases
import helpers
import stream_scenarios as ss
from oracle import orclib
from text_amd import _capi, synth

ZERO_TIES = dict.fromkeys(orclib.CheckerLib.TIE_KINDS, 0)

# chunk lengths per call and slot, taken in turn: ragged, with empty chunks
PLAN = [[5, 0, 3, 9], [7, 11, 0, 1], [0, 4, 4, 20], [30, 30, 30, 30], [13, 2, 0, 6], [1, 25, 9, 0]]


def _session_lengths(T):
    """2-3 utterances per slot, between 7 frames and the case's T"""
    return [[T, 7, T - 3], [T // 2, T], [7, 9, T // 3], [T - 3, 12]]


class _Oracle:
    """An oracle decoder of one utterance, begun; end() -> its n-best, having checked that it passed no tie."""

    def __init__(self, lib, c, inp, what):
        self.lib, self.N, self.what = lib, c["N"], what
        self.od, self.lm, self.trie = ss.checker_decoder(lib, c, inp)
        lib.decoder_begin(self.od)

    def step(self, rows):
        if len(rows):
            self.lib.decoder_step(self.od, orclib._fp(np.ascontiguousarray(rows)), len(rows), self.N)

    def prune(self, look_back):
        self.lib.decoder_prune(self.od, look_back)

    def best(self, look_back, cap):
        return self.lib.best(self.od, look_back, cap)

    def frames_in_buffer(self):
        return self.lib.decoder_n_frames_in_buffer(self.od)

    def end(self):
        self.lib.decoder_end(self.od)
        hyps = self.lib.collect(self.od)
        # (a comparison on a tied input proves nothing: the seeds are chosen so that there is none)
        assert self.lib.ties(self.od) == ZERO_TIES, "%s: the oracle passed ties %r" % (self.what, self.lib.ties(self.od))
        self.close()
        return hyps

    def close(self):
        self.lib.decoder_destroy(self.od)
        if self.trie is not None:
            self.lib.trie_destroy(self.trie)
        self.lib.lm_destroy(self.lm)


def _emissions(c, inp, seed, T):
    lex = inp["lex"] if c["dist"] == "lexspell" else None
    return synth.emissions(c["dist"], seed, T, c["N"], lexicon=lex)


def _flat(parts):
    n = sum(len(p) for p in parts)
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32) if n else np.zeros(1, np.float32)


def _same(want, got, what):
    ok, why = helpers.hyps_equal(want, got)  # (max-merge cases: bit for bit)
    assert ok, "%s: %s" % (what, why)


def _look(d, oracles, look_back, cap, what):
    """getBestHypothesis(look_back) and the frames in the buffer of every slot against its oracle"""
    for b, o in enumerate(oracles):
        assert ss._enc_one(o.best(look_back, cap)) == ss._enc_one(d.best(b, look_back, cap)), "%s: best of slot %d" % (what, b)
        assert o.frames_in_buffer() == d.frames_in_buffer(b), "%s: frames in buffer of slot %d" % (what, b)


# ---- 1. sessions of unequal length -------------------------------------------------------------------------------------
# (name, tunables, seed, what d.get() must say once the streams are begun)
SESSIONS = [
    ("lf_ctc_t60_k10", (), 3100, {"sstream": True, "family0": True}),
    ("lf_ctc_t60_k10", (("sstream", 0),), 3100, {"sstream": False, "family0": True}),
    ("lf_asg_t40_n29_kt7", (), 3200, {"family0": True}),
    ("lx_spell_t60_k12_full", (), 3300, {"family0": False}),
    ("ng_word_t60_k16_4g", (), 3400, {"family0": False}),
    ("ng_word_t60_k16_4g", (("cut_m", 17), ("stream_defer", 1)), 3400, {"family0": False, "cut": 17}),
    ("ng_word_t60_k16_4g", (("cut_m", 17), ("stream_defer", 0)), 3400, {"family0": False, "cut": 17}),
    ("ng_tok_lexfree_t40", (), 3500, {"tstream": True}),
]
SESSIONS = SESSIONS + [(n, s + (("compact_always", 1),), u, e) for n, s, u, e in SESSIONS]
SESSION_IDS = ["%s-%s" % (n, "-".join("%s%d" % kv for kv in s) or "default") for n, s, _, _ in SESSIONS]


def _unequal_sessions(session, orc, name, sets, seed, expect):
    c = cases.BY_NAME[name]
    inp = helpers.case_inputs(c)
    N, B, T = c["N"], 4, c["T"]
    lens = _session_lengths(T)
    utt = [[_emissions(c, inp, seed + 16 * b + j, n) for j, n in enumerate(lens[b])] for b in range(B)]
    oracles = [_Oracle(orc, c, inp, "%s slot %d utterance 0" % (name, b)) for b in range(B)]
    d = session.decoder(c, inp)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(B, N, T + 4)
    if "sstream" in expect:
        assert (d.get("sstream") > 0) == expect["sstream"]
    if "tstream" in expect:
        assert (d.get("tstream") > 0) == expect["tstream"]
    if "family0" in expect:  # the id family: childTab / maskTab engines count ids, the generic engine has the state table
        assert (d.get("lean") != 0) == expect["family0"]
    if "cut" in expect:
        assert d.get("cut") == expect["cut"]
    cur, done, finished, cap = [0] * B, [0] * B, 0, T + 8

    def left(b):
        return lens[b][cur[b]] - done[b]

    call = 0
    while any(cur[b] + 1 < len(lens[b]) or left(b) > 0 for b in range(B)):
        assert call < 64
        what = "%s call %d" % (name, call)
        take = [min(PLAN[call % len(PLAN)][b], left(b)) for b in range(B)]
        parts = [utt[b][cur[b]][done[b]:done[b] + take[b]] for b in range(B)]
        d.stream_step(_flat(parts), take)
        for b in range(B):
            oracles[b].step(parts[b])
            done[b] += take[b]
        if call % 3 == 2:
            d.stream_prune(1)
            for o in oracles:
                o.prune(1)
        which = [1 if left(b) == 0 and cur[b] + 1 < len(lens[b]) else 0 for b in range(B)]
        if any(which):  # the slots whose utterance is used up, in one call
            fin = d.stream_finish(which)
            assert sorted(fin) == [b for b in range(B) if which[b]]
            for b in sorted(fin):
                _same(oracles[b].end(), fin[b], "%s: finished utterance %d of slot %d" % (what, cur[b], b))
                cur[b], done[b] = cur[b] + 1, 0
                oracles[b] = _Oracle(orc, c, inp, "%s slot %d utterance %d" % (name, b, cur[b]))
                finished += 1
        _look(d, oracles, call % 3, cap, what)  # (the others untouched, the restarted slots at the root)
        call += 1
    assert finished == sum(len(x) - 1 for x in lens)
    d.stream_end()
    for b in range(B):
        _same(oracles[b].end(), d.results(b), "%s: last utterance of slot %d" % (name, b))
    if "cut" in expect:  # (chunks were decoded again: finishes met chunks pending their second pass, or settled ones)
        assert d.get("stream_redone") > 0
    if ("compact_always", 1) in sets:
        assert d.get("compactions") >= call
    d.close()


@pytest.mark.parametrize("name,sets,seed,expect", SESSIONS, ids=SESSION_IDS)
def test_sessions_of_unequal_length_emulated(emu_session, oracle_lib, name, sets, seed, expect):
    _unequal_sessions(emu_session, oracle_lib, name, sets, seed, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("name,sets,seed,expect", SESSIONS, ids=SESSION_IDS)
def test_sessions_of_unequal_length(gpu_session, oracle_lib, name, sets, seed, expect):
    _unequal_sessions(gpu_session, oracle_lib, name, sets, seed, expect)


# ---- 2. ids come back --------------------------------------------------------------------------------------------------
def _states_named(c, hyps):
    """A lower bound of the LM states an utterance names: the distinct non-empty prefixes of the LM inputs of its final
    hypotheses (lexicon-free: a token that differs from the one before and is not the blank moves to a child state,
    LexiconFreeDecoder.cpp:69-72; the states are the trie over those inputs)."""
    blank = c["N"] - 1 if c["crit"] == "ctc" else -1
    seen = set()
    for h in hyps:
        seq, prev = [], int(h.tokens[0])
        for t in (int(t) for t in h.tokens[1:-1]):
            if t != prev and t != blank:
                seq.append(t)
                seen.add(tuple(seq))
            prev = t
    return len(seen)


def _ids_come_back(session, orc, name, seed):
    """Slot 1 is restarted 40 times with 12-frame utterances while slot 0 runs one long utterance throughout; the buffer
    is so small that a stream has fewer ids (id_cap) than the 40 utterances name states, and nothing compacts unless it
    must: a restart has to hand the slot's ids out again.  No stream may stop with a full table (a finish and results()
    raise on a stream's status)."""
    c = cases.BY_NAME[name]
    inp = helpers.case_inputs(c)
    N, n_short, short, chunk, max_frames = c["N"], 40, 12, 6, 16
    long_e = _emissions(c, inp, seed, n_short * short)
    shorts = [_emissions(c, inp, seed + 1 + j, short) for j in range(n_short)]
    named = 0
    for e in shorts:  # (each alone and unpruned on the oracle: a prune drops history, not states)
        named += _states_named(c, helpers.run_checker(orc, dict(c, T=short), dict(inp, e=e)))
    d = session.decoder(c, inp)
    d.set("compact_always", 0)
    d.stream_begin(2, N, max_frames)
    assert 0 < d.get("id_cap") < named, (d.get("id_cap"), named)
    o_long = _Oracle(orc, c, inp, "%s long" % name)
    for j in range(n_short):
        o = _Oracle(orc, c, inp, "%s short %d" % (name, j))
        for k in range(short // chunk):
            at = j * short + k * chunk
            parts = [long_e[at:at + chunk], shorts[j][k * chunk:(k + 1) * chunk]]
            d.stream_step(_flat(parts), [chunk, chunk])
            d.stream_prune(0)  # (the long utterance lives in the 16-frame buffer)
            for x, rows in zip((o_long, o), parts):
                x.step(rows)
                x.prune(0)
        _same(o.end(), d.stream_finish([0, 1])[1], "%s: short utterance %d" % (name, j))
        if j % 8 == 7:
            _look(d, [o_long], 0, max_frames + 8, "%s after restart %d" % (name, j))
    d.stream_end()
    _same(o_long.end(), d.results(0), "%s: the long utterance" % name)
    d.close()


IDS_CASES = ["lf_ctc_t60_k10", "ng_tok_lexfree_t40"]  # the counting engines' ids; the generic engine's state table


@pytest.mark.parametrize("name", IDS_CASES)
def test_ids_come_back_emulated(emu_session, oracle_lib, name):
    _ids_come_back(emu_session, oracle_lib, name, 4100)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS_CASES)
def test_ids_come_back(gpu_session, oracle_lib, name):
    _ids_come_back(gpu_session, oracle_lib, name, 4100)


# ---- 3. edges ----------------------------------------------------------------------------------------------------------
EDGE_CASES = ["lf_ctc_t60_k10", "ng_word_t60_k16_4g"]


def _begun(session, c, inp, B, seed, frames, sets=()):
    """a decoder with B streams begun and `frames` frames of B utterances decoded in one chunk; their oracles"""
    d = session.decoder(c, inp)
    for k, v in sets:
        d.set(k, v)
    d.stream_begin(B, c["N"], c["T"] + 4)
    es = [_emissions(c, inp, seed + b, c["T"]) for b in range(B)]
    if frames:
        d.stream_step(_flat([e[:frames] for e in es]), [frames] * B)
    return d, es


def _edges(session, orc, name):
    c = cases.BY_NAME[name]
    inp = helpers.case_inputs(c)
    N, T, B, cap = c["N"], c["T"], 3, c["T"] + 8
    first, rest = 23, 9

    def oracles(es, n):
        out = [_Oracle(orc, c, inp, "%s edge stream %d" % (name, b)) for b in range(B)]
        for o, e in zip(out, es):
            o.step(e[:n])
        return out

    # a finish naming nobody: every best unchanged, the counts all zero
    d, es = _begun(session, c, inp, B, 5100, first)
    orcs = oracles(es, first)
    _look(d, orcs, 1, cap, "%s before naming nobody" % name)
    assert d.stream_finish([0] * B) == {}
    _look(d, orcs, 1, cap, "%s after naming nobody" % name)
    # a prune immediately followed by a finish: the deferred prune is settled first
    d.stream_prune(2)
    for o in orcs:
        o.prune(2)
    fin = d.stream_finish([0, 1, 0])
    _same(orcs[1].end(), fin[1], "%s: finish behind a prune" % name)
    orcs[1] = _Oracle(orc, c, inp, "%s edge restarted" % name)
    _look(d, orcs, 0, cap, "%s after the finish behind a prune" % name)
    # a finish immediately followed by the partials: a named slot reports first frame 0 and the stable prefix of a stream
    # just begun -- the root's entry alone, no decoded frame -- and the slot not named what it reported before
    d.stream_step(_flat([es[0][first:first + rest], es[1][:rest], es[2][first:first + rest]]), [rest] * B)
    orcs[0].step(es[0][first:first + rest])
    orcs[1].step(es[1][:rest])
    orcs[2].step(es[2][first:first + rest])
    d.stream_prune(0)
    for o in orcs:
        o.prune(0)
    fields = ("length", "stable_frames", "stable_tokens", "stable_words", "first_frame", "status")

    def partials(x):
        r = x.stream_partials(0)
        return {k: np.array(r[k]).reshape(-1).tolist() for k in fields}

    fresh, _ = _begun(session, c, inp, 1, 5100, 0)
    root = partials(fresh)
    fresh.close()
    assert root["first_frame"] == [0] and root["stable_frames"] == [1] and root["status"] == [0]
    before = partials(d)
    assert before["first_frame"][0] > 0 or c["kind"] == "lexicon"  # (the lexicon-free prune cuts to look_back frames)
    fin = d.stream_finish([1, 0, 1])
    after = partials(d)
    for k in fields:
        assert after[k][1] == before[k][1], k
        assert after[k][0] == root[k][0] and after[k][2] == root[k][0], k
    for b in (0, 2):
        _same(orcs[b].end(), fin[b], "%s: finish of stream %d" % (name, b))
        orcs[b] = _Oracle(orc, c, inp, "%s edge restarted %d" % (name, b))
    _look(d, orcs, 0, cap, "%s after the second finish" % name)
    # a finish of a slot with zero frames decoded: what stream_end right after stream_begin returns
    fin = d.stream_finish([1, 0, 0])
    _same(orcs[0].end(), fin[0], "%s: finish of an empty slot" % name)
    orcs[0] = _Oracle(orc, c, inp, "%s edge restarted again" % name)
    e, _ = _begun(session, c, inp, 1, 5100, 0)
    e.stream_end()
    _same(e.results(0), fin[0], "%s: an empty slot against stream_end after stream_begin" % name)
    e.close()
    _look(d, orcs, 0, cap, "%s after finishing an empty slot" % name)
    d.close()
    for o in orcs:
        o.close()
    # a finish naming all B = stream_end followed by stream_begin on a twin: the results, and the next chunk
    d, es = _begun(session, c, inp, B, 5200, first)
    twin, _ = _begun(session, c, inp, B, 5200, first)
    fin = d.stream_finish([1] * B)
    twin.stream_end()
    for b in range(B):
        _same(twin.results(b), fin[b], "%s: all named, stream %d against stream_end" % (name, b))
    twin.stream_begin(B, N, T + 4)
    nxt = _flat([e[first:first + rest] for e in es])
    orcs = oracles([e[first:] for e in es], rest)
    for x in (d, twin):
        x.stream_step(nxt, [rest] * B)
    for b in range(B):
        assert ss._enc_one(twin.best(b, 0, cap)) == ss._enc_one(d.best(b, 0, cap))
        assert twin.frames_in_buffer(b) == d.frames_in_buffer(b)
    _look(d, orcs, 0, cap, "%s: the chunk after naming all" % name)
    d.stream_end()
    twin.stream_end()
    for b in range(B):
        want = orcs[b].end()
        _same(want, d.results(b), "%s: all named, then a chunk, stream %d" % (name, b))
        _same(want, twin.results(b), "%s: the twin, stream %d" % (name, b))
    d.close()
    twin.close()


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edges_emulated(emu_session, oracle_lib, name):
    _edges(emu_session, oracle_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_CASES)
def test_edges(gpu_session, oracle_lib, name):
    _edges(gpu_session, oracle_lib, name)


# ---- 4. device results -------------------------------------------------------------------------------------------------
def _device_results(session, orc, name):
    """results_on_device = 1: tokens / words / row_off / length go to collapse_rows as they are (row b: the best
    hypothesis of stream b, empty for a stream not named); the transcripts are those collapsed from the host results"""
    c = cases.BY_NAME[name]
    inp = helpers.case_inputs(c)
    B, frames, which = 3, 31, [1, 0, 1]
    blank = c["N"] - 1 if c["crit"] == "ctc" else -1
    host, es = _begun(session, c, inp, B, 5300, frames)
    dev, _ = _begun(session, c, inp, B, 5300, frames)
    keys = ("tok_off", "tokens", "timesteps", "word_off", "words", "word_timesteps", "word_tok_end")
    fin = host.stream_finish(which)
    for b in (0, 2):  # (the host results are right ...)
        o = _Oracle(orc, c, inp, "%s device results stream %d" % (name, b))
        o.step(es[b][:frames])
        _same(o.end(), fin[b], "%s: host results of stream %d" % (name, b))
    rows = [fin[b][0] if which[b] and fin[b] else None for b in range(B)]
    want = {k: [] for k in keys}
    want["tok_off"], want["word_off"] = [0], [0]
    for r in rows:  # the rule of fltx_transcripts (include/fltx.h), restated on the host results
        tok = [] if r is None else r.tokens.tolist()
        wrd = [] if r is None or c["kind"] != "lexicon" else r.words.tolist()
        for i, t in enumerate(tok):
            if t >= 0 and t != blank and (i == 0 or t != tok[i - 1]):
                want["tokens"].append(t)
                want["timesteps"].append(i)
            if wrd and wrd[i] >= 0:
                want["words"].append(wrd[i])
                want["word_timesteps"].append(i)
                want["word_tok_end"].append(len(want["tokens"]) - want["tok_off"][-1])
        want["tok_off"].append(len(want["tokens"]))
        want["word_off"].append(len(want["words"]))
    assert want["tok_off"][-1] > 0  # (... and not empty)
    fo = dev.stream_finish(which, device=True)
    assert (fo["words"] is not None) == (c["kind"] == "lexicon")
    got = session.ctx.collapse_rows(fo["tokens"], fo["words"], fo["row_off"], fo["length"], blank, n_rows=B)
    for k in keys:
        assert want[k] == got[k].tolist(), "%s: %s" % (name, k)
    host.close()
    dev.close()


@pytest.mark.parametrize("name", ["lf_ctc_t60_k10", "lx_spell_t60_k12_full"])
def test_device_results_emulated(emu_session, oracle_lib, name):
    _device_results(emu_session, oracle_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lf_ctc_t60_k10", "lx_spell_t60_k12_full"])
def test_device_results(gpu_session, oracle_lib, name):
    _device_results(gpu_session, oracle_lib, name)


# ---- 5. errors ---------------------------------------------------------------------------------------------------------
def _errors(session):
    f, L = session.lib.lib, session.lib
    c = cases.BY_NAME["lf_ctc_t60_k10"]
    inp = helpers.case_inputs(c)
    which = np.array([1, 0], np.int32)
    fo = _capi.FinishedOut()

    def code(d, w=which, out=fo):
        return f.fltx_stream_finish(d.h if d is not None else None, None if w is None else w.ctypes.data,
                                    0, None if out is None else C.byref(out))

    d = session.decoder(c, inp)
    assert code(d) == _capi.ERR_STATE  # outside a stream
    assert "no open stream" in f.fltx_last_error().decode()
    d.decode_batch(inp["e"], [c["T"]], c["N"])
    assert code(d) == _capi.ERR_STATE  # ... after an offline batch too
    d.stream_begin(2, c["N"], 16)
    assert code(d, w=None) == _capi.ERR_INVALID
    assert code(d, out=None) == _capi.ERR_INVALID
    assert code(None) == _capi.ERR_INVALID
    assert code(d) == _capi.FLTX_OK
    d.stream_end()
    assert code(d) == _capi.ERR_STATE  # after fltx_stream_end
    d.close()
    # the step kinds
    rows = _capi.RowsLM(4, None, 3, lib=L)
    s2s = _capi.Seq2SeqBatchDecoder(session.ctx, _capi.make_s2s_options(2, 2), session.zero, 3, 3)
    cr = _capi.CtcRowsBatchDecoder(session.ctx, _capi.make_options(2, 2), rows, 0, 1)
    for x, how in ((s2s, "fltx_s2s_step"), (cr, "fltx_ctc_rows_step")):
        assert code(x) == _capi.ERR_STATE
        assert how in f.fltx_last_error().decode()
        x.close()
    # a host LM: its states are the callee's -- left for later
    c = cases.BY_NAME["hl_lastword_lexfree"]
    inp = helpers.case_inputs(c)
    d = session.decoder(c, inp)
    d.stream_begin(2, c["N"], 16)
    assert code(d) == _capi.ERR_UNSUPPORTED
    assert "host LM" in f.fltx_last_error().decode()
    with pytest.raises(_capi.FltxError):
        d.stream_finish([1, 0])
    d.stream_end()  # (the streams are as they were)
    assert d.count(0)[0] >= 1
    d.close()


def test_errors_emulated(emu_session):
    _errors(emu_session)


@pytest.mark.gpu
def test_errors(gpu_session):
    _errors(gpu_session)
