"""Finish and restart single streams of a CTC rows stream batch (fltx_ctc_rows_stream_finish, text_amd/csrc/
fltx_ctc_rows_stream.h): decodeEnd and decodeBegin of the named slots in one call, the other streams untouched.

The yardstick of a reused slot is a FRESH B = 1 decoder driven through the calls that existed before (stream_begin,
append, step, prune, best, end) on the same chunks and prunes: finished n-best, every best, frames in buffer and every
row list equal bit for bit, ids included.  The yardstick of a bystander is the same script without the finish calls.
Independently of any device code every utterance is held to the float64 restatement of tests/test_ctc_lm_rows_stream.py
(tokens exact, scores bit-identical under max-merge, within 1e-5 under logAdd: that module's bounds).

`Kind` says what differs between the decoder kinds; tests/test_lexicon_ctc_lm_rows_stream_finish.py runs the same checks
on the lexicon kind with a word LM and with a token LM.

Every device test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_CTC_LMROWS_FINISH_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
from golden import make_ctc_lm_rows_golden as G  # noqa: E402
import test_ctc_lm_rows as C0  # noqa: E402
from test_ctc_lm_rows import MIN_GAP, PrefixLM, Stats, _dev, make_dec  # noqa: E402
from test_ctc_lm_rows_recycle import Model, RecyclingStreams  # noqa: E402
from test_ctc_lm_rows_stream import assert_best, restate_stream  # noqa: E402
from test_collapse_rows import read_device  # noqa: E402
from test_stream_partials import collapse, row_of  # noqa: E402
from test_seq2seq_model_output import _bits_equal, _GpuSess, _np, is_gpu  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]


@pytest.fixture(scope="module")
def gpu_sess(gpu_session):
    return _GpuSess(gpu_session)


@pytest.fixture(params=BACKENDS)
def sess(request):
    if request.param == "emu":
        return request.getfixturevalue("emu_session")
    import torch
    g = request.getfixturevalue("gpu_sess")
    torch.cuda.set_stream(g.stream)
    return g


# ---- what differs between the kinds ----------------------------------------------------------------------------------------
class Kind:
    """The lexicon-free kind: N = 5, K = 6, W = 7 as tests/test_ctc_lm_rows_stream.py has them"""
    lexicon = False
    name = "lexfree"

    def __init__(self, log_add=False, K=6, N=5, thr=25.0):
        self.log_add, self.K, self.N, self.W, self.thr = log_add, K, N, 7, thr
        self.sil, self.blank = 0, 1
        self.rl = G.SmRowsLM(91, N, self.W, 41, self.W - 1, 0)
        self.row = lambda p: self.rl.row(list(p))

    def open(self, sess):
        self.sess = sess
        self.lm = _capi.RowsLM(self.W, self.rl.usr_to_lm, self.W - 1, lib=sess.lib)
        return self

    def dec(self, max_states=None):
        d = make_dec(self.sess, self.lm, self.K, self.N, self.thr, 0.7, -0.3, self.sil, self.blank, self.log_add)
        if max_states is not None:
            d.set_max_states(max_states)
        return d

    def close(self):
        self.lm.close()

    def lm_row(self, b, p):
        return self.row(p)

    def emissions(self, seed, T):
        return G.emissions(seed, T, self.N)

    def restate(self, em, script, st):
        lm = PrefixLM(self.row, self.rl.usr_to_lm, self.rl.finish)
        return restate_stream(em, lm, self.K, self.N, self.thr, 0.7, -0.3, self.sil, self.blank, self.log_add, script,
                              st=st)

    assert_final = staticmethod(C0.assert_final)
    assert_rows = staticmethod(C0.assert_rows)

    def clean(self, base, T, script):
        """the first seed from `base` whose restatement of `script` has no tie (under logAdd no gap below MIN_GAP)
        -> (emissions, the restatement's result)"""
        for seed in range(base, base + 200):
            st = Stats()
            em = self.emissions(seed, T)
            res = self.restate(em, script, st)
            if not st.ties and (not self.log_add or st.gap > MIN_GAP):
                return em, res
        raise AssertionError("no tie-free seed from %d" % base)


# ---- the device loop ---------------------------------------------------------------------------------------------------------
class SlotStreams(RecyclingStreams):
    """RecyclingStreams whose slots are finished and reused: the tracker, the model and the row lists of a named slot
    start over, and what they held is kept in self.past[b]"""

    def __init__(self, sess, dec, B, N, W, lm_row, max_frames, lexicon=False):
        self.past = [[] for _ in range(B)]
        RecyclingStreams.__init__(self, sess, dec, B, N, W, lm_row, max_frames, lexicon)

    def _take(self, out, stepped, first=False):
        self.last = out  # (the four lists as the call gave them: what fltx_ctc_rows_plan takes)
        RecyclingStreams._take(self, out, stepped, first)

    def finish(self, which, device=False):
        lists, fin = self.dec.stream_finish(which, self.lm_rows(), device=device)
        self.take_finish(lists, which)
        return fin

    def take_finish(self, lists, which):
        self.last = lists
        if is_gpu(self.sess):
            self.dec.ctx.synchronize()
        tok, src, state, n = [_np(a).copy() for a in lists]
        K = self.K
        for b in range(self.B):
            nb = int(n[b])
            assert (tok[b, nb:] == -1).all() and (src[b, nb:] == -1).all() and (state[b, nb:] == -1).all(), b
            if which[b]:  # the root, as stream_begin lists it
                assert (int(src[b, 0]), int(tok[b, 0]), int(state[b, 0]), nb) == \
                    (-1, -1 if self.lexicon else self.dec.sil, 0, 1), b
                self.past[b].append(dict(rows=self.rows[b], named=self.named[b], prefix=self.prefix[b]))
                self.rows[b], self.named[b], self.prefix[b] = [], [], {0: ()}
                self.model[b] = Model(0)
                self.psid[b, :] = -1
                self.stopped.discard(b)
            else:  # the beam listed again, unchanged
                assert (src[b, :nb] == b * K + np.arange(nb)).all() and (tok[b, :nb] == -1).all(), b
                assert (state[b, :nb] == self.prev_state[b, :nb]).all() and nb == int(self.prev_n[b]), b
        self.prev_state, self.prev_n = state, n


def partial_key(p):
    return (p.score, p.am, p.lm, p.tokens.tolist(), p.timesteps.tolist(), p.words.tolist(), p.length, p.stable_frames,
            p.stable_tokens, p.stable_words, p.first_frame, p.status)


def slot_scripts(ops, B):
    """per slot the B = 1 scripts of its utterances: a finish that names the slot ends one"""
    out = [[[]] for _ in range(B)]
    for op, v in ops:
        for b in range(B):
            if op == "f":
                if v[b]:
                    out[b].append([])
            else:
                out[b][-1].append((op, v[b] if op == "c" else v))
    return out


def run_slots(sess, kind, dec, ops, ems, max_frames):
    """ops for all slots at once: ("c", [T_b]) a chunk, ("b", lb) best, ("p", lb) prune, ("s", lb) partials, ("k", cap)
    collect, ("f", [flag_b]) a finish.  ems[b]: the emissions of slot b's utterances, in turn.  The streams are ended
    after the last op.  -> per slot the records of its utterances: bests, frames (in buffer, after each prune and before
    its end), partials, released, final, status, rows (named: with the states the ids stand for), prefix; and the SlotStreams"""
    B = len(ems)
    ds = SlotStreams(sess, dec, B, kind.N, kind.W, kind.lm_row, max_frames, kind.lexicon)
    new = lambda: dict(bests=[], frames=[], partials=[], released=[], final=None, status=0)  # noqa: E731
    recs = [[new()] for _ in range(B)]
    utt, at = [0] * B, [0] * B

    def close(b, final, status):
        assert at[b] == ems[b][utt[b]].shape[0], (b, utt[b], at[b])
        recs[b][-1].update(final=final, status=status)

    for op, v in ops:
        if op == "c":
            ds.chunk([ems[b][utt[b]][at[b]:at[b] + v[b]] for b in range(B)])
            at = [a + x for a, x in zip(at, v)]
            for b in range(B):
                if int(ds.prev_n[b]) == 0:
                    ds.stopped.add(b)
        elif op == "b":
            for b in range(B):
                try:
                    recs[b][-1]["bests"].append(ds.best(b, v))
                except _capi.FltxError as e:
                    recs[b][-1]["bests"].append(("error", e.code))
        elif op == "p":
            dec.prune(v)
            for b in range(B):
                recs[b][-1]["frames"].append(dec.frames_in_buffer(b))
        elif op == "s":
            for b, p in enumerate(dec.stream_partials_batch(v)):
                recs[b][-1]["partials"].append(partial_key(p))
        elif op == "k":
            for b, ids in enumerate(ds.collect(v)):
                recs[b][-1]["released"].append(ids)
        else:
            fib = [dec.frames_in_buffer(b) for b in range(B)]
            fin = ds.finish(v)
            for b in range(B):
                if not v[b]:
                    assert fin["n_hyp"][b] == 0 and fin["length"][b] == 0 and fin["status"][b] == 0, b
                    assert b not in fin["hyps"]
                    continue
                assert fin["length"][b] == fib[b] + 1, (b, fin["length"][b], fib[b])
                recs[b][-1]["frames"].append(fib[b])
                final = [ds._hyp(h) for h in fin["hyps"][b]]
                assert all(len(h[3]) == fib[b] + 1 for h in final), b
                assert len(final) == (fin["n_hyp"][b] if fin["status"][b] == 0 else 0)
                close(b, final, int(fin["status"][b]))
                recs[b][-1].update(rows=ds.past[b][-1]["rows"], prefix=ds.past[b][-1]["prefix"],
                                   named=ds.past[b][-1]["named"])
                recs[b].append(new())
                utt[b] += 1
                at[b] = 0
    fib = [dec.frames_in_buffer(b) for b in range(B)]
    dec.end(ds.lm_rows())
    for b in range(B):
        recs[b][-1]["frames"].append(fib[b])
        try:
            final, status = [ds._hyp(h) for h in dec.results(b)], 0
        except _capi.FltxError as e:
            final, status = [], e.code
        close(b, final, status)
        recs[b][-1].update(rows=ds.rows[b], prefix=ds.prefix[b], named=ds.named[b])
    return recs, ds


def same_bits(a, b):
    """two hypotheses (or bests: None, an error) equal bit for bit"""
    if a is None or b is None or a[0] == "error" or b[0] == "error":
        return a == b
    return list(a[3:]) == list(b[3:]) and _bits_equal(a[:3], b[:3])


def assert_same_record(want, got, what, ids=True):
    """an utterance of a reused slot against the fresh stream's: bit for bit, ids included.  ids=False: the row lists
    by the states their ids stand for (the threads of a beam wider than a wave take their new ids in no fixed order)"""
    assert got["status"] == want["status"] and got["frames"] == want["frames"], (what, got["frames"], want["frames"])
    assert len(got["final"]) == len(want["final"]), (what, len(got["final"]), len(want["final"]))
    for i, (w, g) in enumerate(zip(want["final"], got["final"])):
        assert same_bits(w, g), (what, "final", i, w, g)
    assert len(got["bests"]) == len(want["bests"])
    for i, (w, g) in enumerate(zip(want["bests"], got["bests"])):
        assert same_bits(w, g), (what, "best", i, w, g)
    assert got["named"] == want["named"] and (not ids or got["rows"] == want["rows"]), (what, "rows")
    assert got["released"] == want["released"], (what, "released")
    assert len(got["partials"]) == len(want["partials"])
    for i, (w, g) in enumerate(zip(want["partials"], got["partials"])):
        assert w[3:] == g[3:] and _bits_equal(w[:3], g[:3]), (what, "partials", i, w, g)


def fresh_record(sess, kind, script, em, max_frames, max_states=None):
    """the utterance on a fresh B = 1 decoder, through the calls that existed before the finish"""
    dec = kind.dec(max_states)
    ops = [(op, [v] if op == "c" else v) for op, v in script]
    recs, _ = run_slots(sess, kind, dec, ops, [[em]], max_frames)
    dec.close()
    return recs[0][0]


def assert_restated(kind, want, rec, what):
    """an utterance against the float64 restatement, by the bounds of the stream tests"""
    w_best, w_frames, w_final, w_rows = want
    assert rec["frames"][:-1] == w_frames, (what, rec["frames"], w_frames)
    assert len(rec["bests"]) == len(w_best)
    for i, (w, g) in enumerate(zip(w_best, rec["bests"])):
        assert_best(w, g, kind.log_add, (what, "best", i), final=kind.assert_final)
    kind.assert_final(w_final, rec["final"], kind.log_add, (what, "final"))
    kind.assert_rows(w_rows, rec["rows"], rec["prefix"])


# ---- 1. a reused slot is a fresh stream, and a bystander sees nothing ---------------------------------------------------------
REUSE_OPS = [("c", [3, 2, 0]), ("b", 0), ("c", [4, 5, 6]), ("p", 2), ("b", 1), ("f", [1, 0, 0]), ("c", [2, 3, 0]),
             ("f", [0, 0, 1]), ("c", [0, 0, 0]), ("b", 0), ("c", [3, 2, 5]), ("p", 1), ("f", [1, 0, 0]), ("f", [1, 0, 0]),
             ("c", [0, 4, 3]), ("b", 2)]
REUSE_TS = [[7, 5, 0, 0], [16], [6, 8]]


def check_reused_slot(sess, kind):
    """Slot 0 decodes A1 (7 frames), A2 (5), A3 (0: two finishes with no frame between them) and is ended on a fourth,
    empty utterance; slot 2 decodes two utterances and finishes in other calls; slot 1 decodes 16 frames throughout.
    Unequal chunks, an empty chunk, prunes and bests between them."""
    kind.open(sess)
    scripts = slot_scripts(REUSE_OPS, 3)
    assert [[sum(v for op, v in s if op == "c") for s in sc] for sc in scripts] == REUSE_TS
    ems, want = [], []
    for b in range(3):
        pairs = [kind.clean(2100 + 300 * b + 40 * u, T, scripts[b][u]) for u, T in enumerate(REUSE_TS[b])]
        ems.append([p[0] for p in pairs])
        want.append([p[1] for p in pairs])
    dec = kind.dec()
    recs, _ = run_slots(sess, kind, dec, REUSE_OPS, ems, 16)
    dec.close()
    assert [len(r) for r in recs] == [4, 1, 2]
    for b in (0, 2):
        for u, rec in enumerate(recs[b]):
            assert_same_record(fresh_record(sess, kind, scripts[b][u], ems[b][u], 16), rec, (b, u))
    # the bystander: the same script without the finish calls (slots 0 and 2 then decode their frames as one utterance)
    plain = [("c", v) if op == "c" else (op, v) for op, v in REUSE_OPS if op != "f"]
    dec = kind.dec()
    joined = [[np.concatenate(e)] for e in ems]
    recs0, _ = run_slots(sess, kind, dec, plain, joined, 16)
    dec.close()
    assert_same_record(recs0[1][0], recs[1][0], "bystander")
    # and every utterance against the restatement
    for b in range(3):
        for u, rec in enumerate(recs[b]):
            assert len(rec["final"]) >= 1
            assert_restated(kind, want[b][u], rec, (b, u))
    kind.close()


@pytest.mark.parametrize("log_add", [False, True], ids=["max", "logadd"])
def test_reused_slot_is_a_fresh_stream_and_a_bystander_sees_nothing(sess, log_add):
    check_reused_slot(sess, Kind(log_add))


# ---- 2. stale ring rows ---------------------------------------------------------------------------------------------------------
STALE_OPS = [("c", [4, 3]), ("p", 1), ("c", [4, 2]), ("p", 1), ("b", 0), ("f", [1, 0]), ("b", 0), ("s", 0),
             ("c", [4, 1]), ("b", 3), ("b", 4), ("b", 9), ("s", 1), ("p", 1), ("c", [4, 0]), ("s", 0), ("p", 1),
             ("c", [3, 0]), ("b", 0), ("b", 1), ("b", 3), ("b", 9), ("s", 0), ("s", 2)]


def check_stale_ring_rows(sess, kind):
    """max_frames = 6: slot 0 is pruned before its finish (base > 0, the ring of 8 rows has wrapped), and its next
    utterance runs longer than the ring -- n-best, best(look_back) up to its own length and past it, and the partials
    are the fresh stream's.  A best right after the finish is the fresh stream's first: the root alone."""
    kind.open(sess)
    scripts = slot_scripts(STALE_OPS, 2)
    Ts = [[sum(v for op, v in s if op == "c") for s in sc] for sc in scripts]
    assert Ts == [[8, 11], [6]]
    plain = lambda b, u: [x for x in scripts[b][u] if x[0] != "s"]  # noqa: E731
    ems = [[kind.clean(2900 + 300 * b + 40 * u, T, plain(b, u))[0] for u, T in enumerate(Ts[b])] for b in range(2)]
    for base in range(2900, 4900, 40):  # (a first utterance whose prunes take frames off: the lexicon's may keep all)
        ems[0][0], res = kind.clean(base, 8, plain(0, 0))
        if res[1][-1] < 8:
            break
    dec = kind.dec()
    recs, _ = run_slots(sess, kind, dec, STALE_OPS, ems, 6)
    dec.close()
    assert recs[0][0]["frames"][1] < 8  # (pruned: the buffer begins behind frame 0)
    first = recs[0][1]["bests"][0]
    if kind.lexicon:
        assert first is None  # LexiconDecoder.cpp:286: nothing before the first frame
    else:
        assert first[3] == [kind.sil] and first[:3] == (0.0, 0.0, 0.0)
    for u in range(2):
        assert_same_record(fresh_record(sess, kind, scripts[0][u], ems[0][u], 6), recs[0][u], u)
    kind.close()


def test_stale_ring_rows(sess):
    check_stale_ring_rows(sess, Kind())


# ---- 3. stopped streams come back -----------------------------------------------------------------------------------------------
def check_table_full_comes_back(sess, kind, base=3300):
    """max_states = 32 and no collect: slot 0 stops with the table full; the finish reports what fltx_ctc_rows_end
    reports for it, the next utterance in the slot decodes as a fresh stream's, and a collect on it releases exactly the
    model's dead set (RecyclingStreams.collect holds the device to Model)."""
    kind.open(sess)
    last3 = lambda b, p: kind.row(p[-3:])  # noqa: E731 (the states stay distinct: the table fills)
    kind.lm_row = last3
    ops = [("c", [30, 3]), ("c", [30, 3]), ("c", [30, 0]), ("b", 0), ("f", [1, 0]), ("c", [5, 2]), ("p", 1), ("k", 32),
           ("c", [4, 0]), ("b", 0), ("k", 32)]
    scripts = slot_scripts(ops, 2)
    ems = [[kind.emissions(base, 90), kind.emissions(base + 1, 9)], [kind.emissions(base + 2, 8)]]
    dec = kind.dec(32)
    recs, ds = run_slots(sess, kind, dec, ops, ems, 96)
    assert recs[0][0]["frames"][-1] < 91  # (the stream stopped before its frames were used up)
    dec.close()
    full = recs[0][0]
    assert full["status"] == _capi.ERR_UNSUPPORTED and full["final"] == [] and full["bests"] == [("error", full["status"])]
    for u in range(2):
        assert_same_record(fresh_record(sess, kind, scripts[0][u], ems[0][u], 96, 32), recs[0][u], u)
    assert recs[0][1]["status"] == 0 and len(recs[0][1]["final"]) >= 1 and any(recs[0][1]["released"])
    assert_same_record(fresh_record(sess, kind, scripts[1][0], ems[1][0], 96, 32), recs[1][0], "bystander")
    kind.close()


def test_table_full_stream_comes_back(sess):
    check_table_full_comes_back(sess, Kind())


def check_empty_beam_comes_back(sess, kind, base=3400):
    """a frame without candidates empties slot 0's beam: n_hyp = 0 and status 0, as fltx_ctc_rows_end gives; then a
    normal utterance follows"""
    kind.open(sess)
    ops = [("c", [4, 4]), ("b", 0), ("f", [1, 0]), ("c", [5, 2]), ("b", 1)]
    scripts = slot_scripts(ops, 2)
    hole = kind.emissions(base, 4)
    hole[2, :] = np.nan
    ems = [[hole, kind.emissions(base + 1, 5)], [kind.emissions(base + 2, 6)]]
    dec = kind.dec()
    recs, _ = run_slots(sess, kind, dec, ops, ems, 8)
    dec.close()
    assert recs[0][0]["status"] == 0 and recs[0][0]["final"] == [] and recs[0][0]["bests"] == [None]
    assert len(recs[0][1]["final"]) >= 1 and len(recs[1][0]["final"]) >= 1
    for u in range(2):
        assert_same_record(fresh_record(sess, kind, scripts[0][u], ems[0][u], 8), recs[0][u], u)
    assert_same_record(fresh_record(sess, kind, scripts[1][0], ems[1][0], 8), recs[1][0], "bystander")
    kind.close()


def test_emptied_stream_comes_back(sess):
    check_empty_beam_comes_back(sess, Kind())


# ---- 4. a beam of 70 ------------------------------------------------------------------------------------------------------------
def check_wide_beam(sess, kind, base=3500):
    """K = 70: the finish's n-best, the reset and the lists cross a wave"""
    kind.open(sess)
    ops = [("c", [6, 5]), ("b", 1), ("f", [1, 0]), ("c", [5, 2]), ("p", 2), ("f", [0, 1]), ("c", [1, 3]), ("b", 0)]
    scripts = slot_scripts(ops, 2)
    Ts = [[sum(v for op, v in s if op == "c") for s in sc] for sc in scripts]
    ems = [[kind.emissions(base + 10 * b + u, T) * np.float32(0.25) for u, T in enumerate(Ts[b])] for b in range(2)]
    dec = kind.dec()
    recs, _ = run_slots(sess, kind, dec, ops, ems, 12)
    dec.close()
    # (flat emissions: the beams the finishes end, and that the bystander lists again, hold more than 64 hypotheses)
    assert len(recs[0][0]["rows"][-1]) > 64 and len(recs[1][0]["rows"][-1]) > 64 and len(recs[0][0]["final"]) > 1
    for b in range(2):
        for u, rec in enumerate(recs[b]):
            assert_same_record(fresh_record(sess, kind, scripts[b][u], ems[b][u], 12), rec, (b, u), ids=False)
    kind.close()


def test_wide_beam(sess):
    check_wide_beam(sess, Kind(K=70, N=6, thr=1e9))


# ---- 5. the planner ---------------------------------------------------------------------------------------------------------------
class PlanModel:
    """The loop of fltx_ctc_rows_plan's contract, with the finish's release rule: streams ascending, ids ascending, a row
    an id has goes on the free stack, every id of the stream is unplanned.  release_on_finish=False: the ids are
    unplanned and their rows are NOT given back -- what a store without the rule comes to."""

    def __init__(self, B, K, cap, release_on_finish=True):
        self.B, self.K, self.cap, self.rel = B, K, cap, release_on_finish
        self.row_of = [dict() for _ in range(B)]
        self.free, self.hw, self.dropped = [], 0, 0
        self.prev = [-1] * (B * K)

    def finish(self, which):
        for b in range(self.B):
            if which[b]:
                for i in sorted(self.row_of[b]):
                    if self.rel and self.row_of[b][i] >= 0:
                        self.free.append(self.row_of[b][i])
                self.row_of[b] = {}

    def plan(self, tok, src, state, n):
        B, K = self.B, self.K
        out = [[-1] * (B * K) for _ in range(5)]
        n_new = 0
        for b in range(B):
            for k in range(int(n[b])):
                r, s = b * K + k, int(state[b, k])
                if s not in self.row_of[b]:
                    if self.free:
                        row = self.free.pop()
                    elif self.hw < self.cap:
                        row = self.hw
                        self.hw += 1
                    else:
                        row = -2
                        self.dropped += 1
                    self.row_of[b][s] = row
                    if row >= 0:
                        sr = int(src[b, k])
                        out[1][n_new], out[2][n_new] = row, -1 if sr < 0 else self.prev[sr]
                        out[3][n_new], out[4][n_new] = -1 if sr < 0 else int(tok[b, k]), r
                        n_new += 1
                out[0][r] = max(self.row_of[b][s], -1)
        self.prev = list(out[0])
        return out, [n_new, self.hw, len(self.free), self.dropped]


def plan_run(sess, kind, dec, model, ops, ems, max_frames, store_rows, log=None):
    """A planned stream batch: every list planned and held to `model`; the LM rows of the new states written into the
    store from the tracker's prefixes.  ops: ("c", [T_b]) / ("f", [flag_b]).  log: receives every planned list and
    every finish, for a replay.  -> (the counts after every plan, the finished n-bests per slot)"""
    B, K, W = len(ems), kind.K, kind.W
    ds = SlotStreams(sess, dec, B, kind.N, W, kind.lm_row, max_frames, kind.lexicon)
    store = np.full((store_rows, W), np.nan, np.float32)
    dec.plan_begin(store_rows)
    counts = []

    def planned():
        """plan the last call's lists -> the device's lm_row_of, held to the model"""
        p = dec.plan(*ds.last)
        if is_gpu(sess):
            dec.ctx.synchronize()
        lists = [_np(a).copy() for a in ds.last]
        if log is not None:
            log.append(("plan", lists))
        got = [_np(a).tolist() for a in (p.lm_row_of, p.new_row, p.new_parent_row, p.new_edge, p.new_dec_row)]
        want, wc = model.plan(*lists)
        assert _np(p.counts).tolist() == wc, (_np(p.counts).tolist(), wc)
        assert got == want, (got, want)
        counts.append(wc)
        for i in range(wc[0]):
            b, k = divmod(want[4][i], K)
            store[want[1][i]] = kind.lm_row(b, ds.prefix[b][int(ds.prev_state[b, k])])
        return p.lm_row_of

    ro = planned()
    utt, at = [0] * B, [0] * B
    finals = [[] for _ in range(B)]
    for op, v in ops:
        if op == "c":
            parts = [ems[b][utt[b]][at[b]:at[b] + v[b]] for b in range(B)]
            flat = np.concatenate([p.reshape(-1) for p in parts]) if sum(v) else np.zeros(0, np.float32)
            for t in range(dec.append(flat, v)):
                ds._take(dec.step(_dev(sess, store), lm_row_of=ro), [t < T for T in v])
                ro = planned()
            at = [a + x for a, x in zip(at, v)]
        else:
            lists, fin = dec.stream_finish(v, _dev(sess, store), lm_row_of=ro)
            ds.take_finish(lists, v)
            model.finish(v)
            if log is not None:
                log.append(("finish", list(v)))
            for b in range(B):
                if v[b]:
                    finals[b].append([ds._hyp(h) for h in fin["hyps"][b]])
                    utt[b] += 1
                    at[b] = 0
            ro = planned()
    return counts, finals


def test_planner_gives_the_rows_of_a_finished_stream_back(sess):
    """The restatement of the planner's loop with the release rule against lm_row_of, the four new_* lists and the counts
    of every plan over a run with finishes; the planned decode equals the unplanned fresh stream's.  Then twenty short
    utterances through one slot in a store sized for one utterance plus the bystanders: the high-water mark stays
    bounded and nothing is dropped -- and, as a control on the CPU, the same loop WITHOUT the release rule overflows
    that store."""
    kind = Kind().open(sess)
    B, K = 3, kind.K
    ops = [("c", [3, 2, 0]), ("c", [2, 3, 4]), ("f", [1, 0, 0]), ("c", [3, 1, 2]), ("f", [1, 0, 1]), ("f", [0, 0, 0]),
           ("c", [2, 2, 2]), ("f", [0, 1, 0])]
    scripts = slot_scripts(ops, B)
    Ts = [[sum(v for op, v in s if op == "c") for s in sc] for sc in scripts]
    ems = [[kind.emissions(3700 + 10 * b + u, T) for u, T in enumerate(Ts[b])] for b in range(B)]
    dec = kind.dec()
    counts, finals = plan_run(sess, kind, dec, PlanModel(B, K, 4096), ops, ems, 16, 4096)
    dec.close()
    assert counts[-1][3] == 0 and any(c[2] > 0 for c in counts)  # (rows came back and were handed out again)
    for b in range(B):
        for u, final in enumerate(finals[b]):
            want = fresh_record(sess, kind, scripts[b][u], ems[b][u], 16)
            assert len(final) == len(want["final"]) and all(same_bits(w, g) for w, g in zip(want["final"], final)), (b, u)
    # twenty utterances through slot 0, the others idle on their roots
    T, n_utt = 6, 20
    ops = [x for _ in range(n_utt) for x in (("c", [T, 0, 0]), ("f", [1, 0, 0]))]
    ems = [[kind.emissions(3800 + u, T) for u in range(n_utt + 1)], [kind.emissions(1, 0)], [kind.emissions(2, 0)]]
    one = PlanModel(B, K, 1 << 20)
    dec = kind.dec()
    plan_run(sess, kind, dec, one, ops[:2], [ems[0][:2]] + ems[1:], 16, 4096)
    dec.close()
    cap = one.hw + 2 * K  # one utterance (and the root that follows it) plus the bystanders
    model = PlanModel(B, K, cap)
    dec = kind.dec()
    log = []
    counts, _ = plan_run(sess, kind, dec, model, ops, ems, 16, cap, log)
    dec.close()
    assert max(c[1] for c in counts) <= cap and counts[-1][3] == 0 and all(c[3] == 0 for c in counts)
    # the control: the same lists and finishes through the loop WITHOUT the release rule overflow that capacity (no
    # device code involved)
    ctl = PlanModel(B, K, cap, release_on_finish=False)
    for what, v in log:
        if what == "plan":
            ctl.plan(*v)
        else:
            ctl.finish(v)
    assert ctl.dropped > 0 and ctl.hw == cap
    kind.close()


# ---- 6. typed chunks after a restart ---------------------------------------------------------------------------------------------
def check_typed_chunk_after_restart(sess, kind, base=3900):
    """one bf16 logits append on a reused slot equals the fresh stream fed the same chunk, frame_lse included"""
    kind.open(sess)
    B, N, T = 2, kind.N, 5
    first = [kind.emissions(base + b, 4) for b in range(B)]
    rng = np.random.RandomState(base)
    logits = (rng.randn(B, T, N) * 2.0).astype(np.float32)
    bits = (logits.view(np.uint32) >> 16).astype(np.uint16)  # (truncated to bfloat16)

    def typed(ds, dec, planes):
        Ts = [T] * len(planes)
        lse = _dev(sess, np.zeros(T * len(planes), np.float64))
        chunk = np.ascontiguousarray(bits[planes]).reshape(-1)
        if is_gpu(sess):
            import torch
            chunk = torch.from_numpy(chunk.view(np.int16)).cuda().view(torch.bfloat16)
            steps = dec.append(chunk, Ts, kind="logits", lse_out=lse)
        else:
            steps = dec.append(chunk, Ts, kind="logits", dtype="bf16", lse_out=lse)
        for t in range(steps):
            ds._take(dec.step(ds.lm_rows()), [True] * len(planes))
        if is_gpu(sess):
            dec.ctx.synchronize()
        return _np(lse).copy()

    dec = kind.dec()
    ds = SlotStreams(sess, dec, B, N, kind.W, kind.lm_row, 16, kind.lexicon)
    ds.chunk(first)
    ds.finish([1, 0])
    lse = typed(ds, dec, [0, 1])
    got = ds.finish([1, 0])["hyps"][0]
    dec.close()
    dec = kind.dec()
    ds1 = SlotStreams(sess, dec, 1, N, kind.W, kind.lm_row, 16, kind.lexicon)
    lse1 = typed(ds1, dec, [0])
    want = ds1.end()[0]
    dec.close()
    assert lse[:T].tobytes() == lse1.tobytes() and np.isfinite(lse1).all()
    assert len(got) == len(want) >= 1 and all(same_bits(w, ds._hyp(g)) for w, g in zip(want, got))
    assert ds.rows[0] == [] and ds.past[0][-1]["rows"] == ds1.rows[0]
    kind.close()


def test_typed_chunk_after_a_restart(sess):
    check_typed_chunk_after_restart(sess, Kind())


# ---- 7. the results ---------------------------------------------------------------------------------------------------------------
def check_results(sess, kind, base=4000):
    """Host mode and device mode give the same bits; the device pointers are fltx_collapse_rows' inputs and give the
    host-side collapse of the host rows; a finish's results outlive three more steps and a prune of the other streams;
    a stream not named has n_hyp = length = 0."""
    kind.open(sess)
    B, K = 3, kind.K
    ems = [kind.emissions(base + b, 9) for b in range(B)]

    def run(device):
        dec = kind.dec()
        ds = SlotStreams(sess, dec, B, kind.N, kind.W, kind.lm_row, 16, kind.lexicon)
        ds.chunk([e[:5] for e in ems])
        dec.prune(2)
        fin = ds.finish([1, 0, 1], device=device)
        return dec, ds, fin

    dec, ds, host = run(False)
    assert host["n_hyp"][1] == 0 and host["length"][1] == 0 and sorted(host["hyps"]) == [0, 2]
    snap = {b: [ds._hyp(h) for h in host["hyps"][b]] for b in (0, 2)}
    # three more steps and a prune of the other streams: the pinned results are what they were
    ds.chunk([e[5:8] for e in ems])
    dec.prune(1)
    dec.close()
    dec, ds, dev = run(True)
    n_hyp, length = read_device(sess, dev["n_hyp"], B, np.int32), read_device(sess, dev["length"], B, np.int32)
    row_off = read_device(sess, dev["row_off"], B, np.int64)
    assert n_hyp.tolist() == host["n_hyp"].tolist() and length.tolist() == host["length"].tolist()
    assert read_device(sess, dev["status"], B, np.int32).tolist() == [0, 0, 0]
    assert (dev["words"] is not None) == kind.lexicon
    ds.chunk([e[5:8] for e in ems])
    dec.prune(1)
    scores = read_device(sess, dev["scores"], 3 * B * K, np.float64)
    for b in (0, 2):
        n, ln = int(n_hyp[b]), int(length[b])
        assert n == len(snap[b]) >= 1
        tok = read_device(sess, dev["tokens"] + 4 * int(row_off[b]), n * ln, np.int32).reshape(n, ln)
        wrd = read_device(sess, dev["words"] + 4 * int(row_off[b]), n * ln, np.int32).reshape(n, ln) if kind.lexicon else None
        for i, h in enumerate(snap[b]):
            assert tok[i].tolist() == h[3] and scores[3 * (b * K + i):3 * (b * K + i) + 3].tobytes() == \
                np.asarray(h[:3], np.float64).tobytes(), (b, i)
            assert wrd is None or wrd[i].tolist() == h[4]
    # the device pointers as they are through fltx_collapse_rows: row b is the first hypothesis of stream b (nothing for a
    # stream not named), against the host-side collapse of the host rows
    got = dec.ctx.collapse_rows(dev["tokens"], dev["words"], dev["row_off"], dev["length"], kind.blank, n_rows=B)
    for b in range(B):
        h = snap[b][0] if b in snap else (0, 0, 0, [], [])
        want = collapse(h[3], h[4] if kind.lexicon else [-1] * len(h[3]), kind.blank)
        assert row_of(got, b) == [w.tolist() for w in want], b
    dec.close()
    kind.close()


def test_results_on_the_host_and_on_the_device(sess):
    check_results(sess, Kind())


# ---- 8. no-op and refusals --------------------------------------------------------------------------------------------------------
def test_a_finish_that_names_nothing_changes_nothing(sess):
    kind = Kind().open(sess)
    ops = [("c", [3, 2]), ("f", [0, 0]), ("b", 0), ("c", [2, 4]), ("p", 1), ("f", [0, 0]), ("f", [0, 0]), ("c", [3, 1]),
           ("b", 1)]
    ems = [[kind.emissions(4100, 8)], [kind.emissions(4101, 7)]]
    dec = kind.dec()
    recs, ds = run_slots(sess, kind, dec, ops, ems, 12)
    # (no LM rows are read: lm_scores may be None)
    dec.close()
    dec = kind.dec()
    recs0, _ = run_slots(sess, kind, dec, [x for x in ops if x[0] != "f"], ems, 12)
    dec.close()
    for b in range(2):
        assert len(recs[b]) == 1
        assert_same_record(recs0[b][0], recs[b][0], b)
    dec = kind.dec()
    ds = SlotStreams(sess, dec, 2, kind.N, kind.W, kind.lm_row, 12, False)
    ds.chunk([e[0][:3] for e in ems])
    lists, fin = dec.stream_finish([0, 0], None)
    ds.take_finish(lists, [0, 0])
    assert fin["hyps"] == {} and not fin["n_hyp"].any()
    dec.close()
    kind.close()


def test_refusals(sess):
    L = sess.lib
    I, S = _capi.ERR_INVALID, _capi.ERR_STATE
    kind = Kind().open(sess)
    N, K, W = kind.N, kind.K, kind.W
    dec = kind.dec()
    dec.B = 1
    po = [dec._addr(o) for o in dec._rows()]
    keep = []

    def ip(*v):
        keep.append(np.asarray(v, np.int32))
        return keep[-1].ctypes.data
    lr = _dev(sess, np.zeros((K, W), np.float32))
    pl = dec._addr(lr)
    out = _capi.FinishedOut()
    fin = L.lib.fltx_ctc_rows_stream_finish

    def call(d, which, lm=pl, dt=0, kd=0, stride=W, lists=po, o=C.byref(out)):
        return fin(d.h, which, lm, dt, kd, stride, None, 0, 1, None, *lists, 0, o)
    em = kind.emissions(4200, 6)
    assert call(dec, ip(1)) == S                                                     # outside a stream
    assert L.lib.fltx_ctc_rows_begin(dec.h, em.ctypes.data, 0, None, ip(3), 1, N, *po) == 0
    assert call(dec, ip(1)) == S                                                     # begun with fltx_ctc_rows_begin
    ok = _capi.make_options(K, N, lm_weight=0.5)
    other = _capi.BatchDecoder(sess.ctx, _capi.LEXFREE, ok, sess.zero, 0, 1)
    s2s = _capi.Seq2SeqBatchDecoder(sess.ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    for o in (other, s2s):                                                           # the other kinds
        assert call(o, ip(1)) == S
        o.close()
    assert L.lib.fltx_ctc_rows_stream_begin(dec.h, 1, N, 8, *po) == 0
    assert L.lib.fltx_ctc_rows_stream_append(dec.h, em.ctypes.data, 0, None, ip(2)) == 0
    assert call(dec, ip(1)) == S and call(dec, ip(0)) == S                           # unstepped frames
    step = L.lib.fltx_ctc_rows_step
    assert step(dec.h, pl, 0, 0, W, None, 0, 1, None, *po) == 0 and call(dec, ip(1)) == S
    assert step(dec.h, pl, 0, 0, W, None, 0, 1, None, *po) == 0
    assert call(dec, None) == I and call(dec, ip(1), o=None) == I                    # NULLs
    for i in range(4):
        assert call(dec, ip(1), lists=po[:i] + [None] + po[i + 1:]) == I
    assert call(dec, ip(1), dt=7) == I and call(dec, ip(1), kd=9) == I               # bad dtype / kind / stride
    assert call(dec, ip(1), stride=W - 1) == I and call(dec, ip(1), lm=None) == I
    assert call(dec, ip(0), lm=None, dt=7, kd=9, stride=0) == 0                      # ... which nobody reads when none is named
    # planning active: a collect without its plan_release
    dec.plan_begin(64)
    rel, n_rel, _ = dec.collect(8)
    assert call(dec, ip(1)) == S and "fltx_ctc_rows_plan_release" in L.lib.fltx_last_error().decode()
    dec.plan_release(rel, n_rel)
    assert call(dec, ip(1)) == 0
    if is_gpu(sess):
        dec.ctx.synchronize()
    n_hyp = _capi._view(out.n_hyp, C.c_int32, 1)
    assert n_hyp[0] >= 1 and _capi._view(out.length, C.c_int32, 1)[0] == 4
    dec.close()
    kind.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_CTC_LMROWS_FINISH_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
