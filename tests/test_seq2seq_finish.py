"""fltx_s2s_finish / fltx_s2s_done_each on the lexicon-free seq2seq decoder (text_amd/csrc/fltx_s2s.h: s2sFinishSlot):
single utterances of a running batch are finished, handed out and their slots restarted or parked, while every other
utterance decodes on as if nothing had happened.

The yardstick throughout is the ordinary batch -- fltx_s2s_begin / step / fltx_s2s_end with one slot per utterance --
which tests/test_seq2seq.py (and its rows-LM siblings) hold to the reference.  Tokens, the three scores and n_hyp compare
bit for bit, the row lists of every local step with next_src_row relative to b*K.  `restate()` of tests/test_seq2seq.py
runs on the CPU only to show that the inputs are tie-free and that the schedules are the ones the tests mean to
exercise (lengths, restart parities, slot reuse).

Every test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first, as tests/test_seq2seq.py arranges it.  tests/test_lexicon_seq2seq_finish.py runs the same
scripts (the classes and functions below) on the lexicon kind.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi, ngram_synth  # noqa: E402

CHILD = os.environ.get("FLTX_S2S_FINISH_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from golden import make_s2s_lm_rows_golden as GR  # noqa: E402
from test_collapse_rows import read_device  # noqa: E402
from test_seq2seq import HostLM, Model, _GpuSess, _np, is_gpu, restate  # noqa: E402
from test_seq2seq_model_output import BF16, F32, NAN_BITS, ref_lse, to_dtype, widen  # noqa: E402

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


def _dev(sess, a, dt=F32):
    """a numpy array as the step takes it on this backend: itself (emulator) or a device tensor"""
    if a is None or not is_gpu(sess):
        return a
    import torch
    t = torch.from_numpy(a.view(np.int16) if dt == BF16 else a).cuda()
    return t.view(torch.bfloat16) if dt == BF16 else t


# ---- decoder configurations --------------------------------------------------------------------------------------------
class Utt:
    """one utterance: the model (row(prefix) -> V float32 or None) and, with a rows LM, lm_row(prefix)"""

    def __init__(self, model, lm=None):
        self.model, self.lm = model, lm

    def row(self, prefix):
        return self.model.row(prefix)

    def dev_row(self, prefix):  # what the device is fed (typed variants: the raw elements)
        return self.model.row(prefix)

    def lm_row(self, prefix):
        return self.lm.row(prefix)


class Setup:
    """A decoder configuration: ZeroLM by default.  utt(seed, eos_bias) makes an utterance, restate_utt its CPU
    restatement, feed() one step of a batch whose rows are `state` {(b, k): (utt, token prefix, word prefix)}."""
    V, K, Kt, eos, maxlen, thr, lmw, eos_score = 24, 4, 8, 3, 6, 1e9, 0.0, 0.0
    drop = 0.0
    # eos biases: an utterance that never proposes eos (it runs into max_output_length), one that ends at once, and
    # one that takes a middling number of steps
    never, quick, mid = -9.0, 9.0, 0.6

    def bias(self, b):
        return getattr(self, b) if isinstance(b, str) else b
    W = None          # a rows LM: the LM rows' width
    dt = F32          # the model rows' element type
    words = False     # the lists carry next_word

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)
        self._lm = None

    # (overridden by the kinds below)
    def lm(self, sess):
        return sess.zero

    def host_lm(self, sess, u):
        return HostLM(None)

    def utt(self, seed, eos_bias):
        return Utt(Model(seed, self.V, self.eos, eos_bias, self.drop))

    def make_dec(self, sess):
        opts = _capi.make_s2s_options(self.K, self.Kt, self.thr, self.lmw, self.eos_score, False)
        return _capi.Seq2SeqBatchDecoder(sess.ctx, opts, self.lm(sess), self.eos, self.maxlen)

    def restate_utt(self, sess, u, ties):
        """-> (final [(score, am, lm, tokens[, words])], rows per step)"""
        return restate(u, self.host_lm(sess, u), self.K, self.Kt, self.thr, self.lmw, self.eos_score, self.eos,
                       self.maxlen, ties=ties)

    def step(self, sess, dec, sc, valid, lr):
        if lr is not None:
            return dec.step(_dev(sess, sc), _dev(sess, valid), lm_scores=_dev(sess, lr))
        return dec.step(_dev(sess, sc), _dev(sess, valid))

    def feed(self, sess, dec, B, state):
        return self.step(sess, dec, *self.matrices(B, state))

    def matrices(self, B, state):
        """-> (model rows, row_valid, LM rows or None) of a step over B slots, as numpy"""
        K = self.K
        if self.dt == BF16:
            sc = np.full((B * K, self.V), NAN_BITS[BF16], dtype=np.uint16)
        else:
            sc = np.full((B * K, self.V), np.nan, dtype=np.float32)
        lr = None if self.W is None else np.full((B * K, self.W), np.nan, dtype=np.float32)
        valid = np.zeros(B * K, dtype=np.uint8)
        for (b, k), (u, pre, wpre) in state.items():
            r = u.dev_row(pre)
            if r is None:
                continue
            sc[b * K + k] = r
            valid[b * K + k] = 1
            if lr is not None:
                lr[b * K + k] = u.lm_row(wpre if self.words else pre)
        return sc, valid, lr

    def close(self):
        pass


class NgramSetup(Setup):
    """a 3-gram over the tokens (ngram_synth), lmWeight != 0"""
    lmw = 0.7

    def lm(self, sess):
        if self._lm is None:
            import tempfile
            self._tmp = tempfile.TemporaryDirectory()
            path = os.path.join(self._tmp.name, "t%d.arpa" % self.V)
            vocab = ngram_synth.words(self.V, "t")
            ngram_synth.write_arpa(path, vocab, 3, (0, 300, 150), 5)
            self._lm = _capi.ArpaLM(path, vocab, lib=sess.lib)
        return self._lm

    def host_lm(self, sess, u):
        return HostLM(self.lm(sess))

    def close(self):
        if self._lm is not None:
            self._lm.close()
            self._tmp.cleanup()
            self._lm = None


class TokenRowsSetup(Setup):
    """a token rows LM (fltx_lm_rows_create): the LM's rows next to the model's, a permuted map, a finish index"""
    lmw, W, perm = 0.7, 31, 77

    def lm(self, sess):
        if self._lm is None:
            rl = GR.SmRowsLM(1, self.V, self.W, self.perm, self.W - 1, self.eos)
            self._lm = _capi.RowsLM(rl.W, rl.usr_to_lm, rl.finish, lib=sess.lib)
        return self._lm

    def utt(self, seed, eos_bias):
        return Utt(Model(seed, self.V, self.eos, eos_bias, self.drop),
                   GR.SmRowsLM(seed ^ 0x77, self.V, self.W, self.perm, self.W - 1, self.eos))

    def host_lm(self, sess, u):
        return GR.PrefixLM(u.lm)

    def close(self):
        if self._lm is not None:
            self._lm.close()
            self._lm = None


class _Bf16Logits:
    """a model whose rows reach the device as bfloat16 logits: row() is what the step makes of them (the widened
    element minus the row's log-sum-exp, for the restatement), dev_row() the bits"""

    def __init__(self, model):
        self.model = model

    def dev_row(self, prefix):
        r = self.model.row(prefix)
        return None if r is None else to_dtype(r.astype(np.float64), BF16)

    def row(self, prefix):
        raw = self.dev_row(prefix)
        if raw is None:
            return None
        w = widen(raw, BF16)
        return (w.astype(np.float64) - ref_lse(w)).astype(np.float32)


class Bf16LogitsSetup(Setup):
    """typed rows: bfloat16 raw logits (fltx_s2s_step_typed)"""
    dt = BF16

    def utt(self, seed, eos_bias):
        m = _Bf16Logits(Model(seed, self.V, self.eos, eos_bias))
        u = Utt(m)
        u.dev_row = m.dev_row
        return u

    def step(self, sess, dec, sc, valid, lr):
        if is_gpu(sess):
            return dec.step(_dev(sess, sc, BF16), _dev(sess, valid), kind="logits")
        return dec.step(sc, valid, kind="logits", dtype="bf16")


# ---- a batch under the script's control --------------------------------------------------------------------------------
def _hyps(hs):
    return [(h.score, h.am, h.lm, h.tokens.tolist(), h.words.tolist()) for h in hs]


def _trim(rows):
    rows = list(rows)
    while rows and rows[-1] == []:
        rows.pop()
    return rows


class Batch:
    """B slots of one decoder.  Keeps, for every listed row, the utterance and the prefix it stands for (so the model
    can be replayed), records each utterance's row lists per local step, and checks what every call lists."""

    def __init__(self, sess, setup, utts, dec=None):
        """utts: [(uid, Utt) or None] per slot (None: the slot holds nothing the script follows)"""
        self.sess, self.setup, self.B, self.K = sess, setup, len(utts), setup.K
        self.own = dec is None
        self.dec = setup.make_dec(sess) if dec is None else dec
        self.uid = [None if x is None else x[0] for x in utts]
        self.rows = {x[0]: [] for x in utts if x is not None}
        self.state = {(b, 0): (x[1], [], []) for b, x in enumerate(utts) if x is not None}
        self.steps = 0
        self.lists = self._host(self.dec.begin(self.B, setup.V))
        if setup.maxlen > 0:
            assert self.lists[3].tolist() == [1] * self.B

    def _host(self, lists):
        if is_gpu(self.sess):
            self.dec.ctx.synchronize()
        return [np.array(_np(a)) for a in lists]

    def slot_lists(self, b):
        """slot b's current lists, next_src_row relative to b*K"""
        tok, beam, src, n = self.lists[:4]
        word = self.lists[4] if len(self.lists) > 4 else None
        return [(int(tok[b, k]), int(beam[b, k]), int(src[b, k]) - b * self.K if src[b, k] >= 0 else None) +
                ((int(word[b, k]),) if word is not None else ()) for k in range(int(n[b]))]

    def _check_padding(self):
        n = self.lists[3]
        for a in self.lists[:3] + self.lists[4:]:
            for b in range(self.B):
                assert (a[b, n[b]:] == -1).all(), (b, n.tolist(), a.tolist())

    def step(self):
        K = self.K
        self.lists = self._host(self.setup.feed(self.sess, self.dec, self.B, self.state))
        self._check_padding()
        tok, src, n = self.lists[0], self.lists[2], self.lists[3]
        word = self.lists[4] if len(self.lists) > 4 else None
        new = {}
        for b in range(self.B):
            if self.uid[b] is None:
                continue
            for k in range(int(n[b])):
                u, pre, wpre = self.state[(b, int(src[b, k]) - b * K)]
                w = int(word[b, k]) if word is not None else -1
                new[(b, k)] = (u, pre + [int(tok[b, k])], wpre + ([w] if w >= 0 else []))
            self.rows[self.uid[b]].append(self.slot_lists(b))
        self.state = new
        self.steps += 1

    def finish(self, which, admit=None, on_device=False):
        """fltx_s2s_finish; admit {b: (uid, Utt)}: the utterances that restarted slots get.  Checks the lists of every
        slot: the root, nothing, or the slot's rows again with next_src_row the row itself."""
        K = self.K
        before = [self.slot_lists(b) for b in range(self.B)]
        lists, fin = self.dec.finish(which, on_device)
        self.lists = self._host(lists)
        self._check_padding()
        n, src = self.lists[3], self.lists[2]
        for b in range(self.B):
            now = self.slot_lists(b)
            if which[b] == 0:
                assert [r[:2] + r[3:] for r in now] == [r[:2] + r[3:] for r in before[b]], (b, now, before[b])
                assert src[b, :n[b]].tolist() == [b * K + k for k in range(int(n[b]))], (b, src[b].tolist())
                continue
            for k in range(K):
                self.state.pop((b, k), None)
            if which[b] == 1:
                assert now == [(-1, -1, None) + ((-1,) if len(self.lists) > 4 else ())], (b, now)
                self.uid[b] = None
                if admit is not None and b in admit:
                    self.uid[b] = admit[b][0]
                    self.rows[admit[b][0]] = []
                    self.state[(b, 0)] = (admit[b][1], [], [])
            else:
                assert now == [], (b, now)
                self.uid[b] = None
        return fin

    def done_each(self):
        return self.dec.done_each()

    def end(self):
        """fltx_s2s_end: -> [hyps] per slot"""
        self.dec.end()
        return [_hyps(self.dec.results(b)) for b in range(self.B)]

    def close(self):
        if self.own:
            self.dec.close()


def ordinary(sess, setup, utts):
    """The yardstick: one slot per utterance, begin / step / end.  -> ({uid: hyps}, {uid: rows per step})"""
    bt = Batch(sess, setup, utts)
    for _ in range(setup.maxlen + 1):
        bt.step()
    assert bt.dec.done() and bt.done_each().all()
    out = bt.end()
    bt.close()
    return {uid: out[b] for b, (uid, _) in enumerate(utts)}, {uid: _trim(r) for uid, r in bt.rows.items()}


def fin_hyps(fin, b):
    assert fin["status"][b] == 0 and fin["n_hyp"][b] == len(fin["hyps"][b])
    return _hyps(fin["hyps"][b])


def n_steps(hyps):
    """the local steps an utterance took: the entries of its (any) hypothesis"""
    return sum(t >= 0 for t in hyps[0][3])


# ---- 1. a queue through few slots ---------------------------------------------------------------------------------------
def simulate(lengths, B):
    """The continuous schedule on the CPU: every slot steps in lock step, a slot whose utterance is done after a step is
    finished and takes the queue's next.  -> (step calls, [(global step of the restart, slot, uid)], uses per slot)"""
    slot = list(range(min(B, len(lengths))))
    left = [lengths[u] for u in slot]
    nxt, g, restarts, uses = len(slot), 0, [], [1] * len(slot)
    while any(u is not None for u in slot):
        g += 1
        for b, u in enumerate(slot):
            if u is None:
                continue
            left[b] -= 1
            if left[b] == 0:
                if nxt < len(lengths):
                    slot[b], left[b] = nxt, lengths[nxt]
                    restarts.append((g, b, nxt))
                    uses[b] += 1
                    nxt += 1
                else:
                    slot[b] = None
    return g, restarts, uses


def run_queue(sess, setup, utts, B):
    """`utts` through B slots with the C ABI's calls: step, fltx_s2s_done_each, fltx_s2s_finish of the done slots (restart
    while the queue has more, park after).  -> ({uid: hyps}, {uid: rows}, step calls, restarts, {uid: steps})"""
    bt = Batch(sess, setup, utts[:B])
    nxt, res, steps, restarts = B, {}, {}, []
    while any(u is not None for u in bt.uid):
        bt.step()
        done = bt.done_each()
        which = np.zeros(B, np.int32)
        admit = {}
        for b in np.flatnonzero(done):
            if bt.uid[b] is None:
                continue
            if nxt < len(utts):
                which[b], admit[int(b)] = 1, utts[nxt]
                restarts.append((bt.steps, int(b), utts[nxt][0]))
                nxt += 1
            else:
                which[b] = 2
        if which.any():
            was = list(bt.uid)
            fin = bt.finish(which, admit)
            for b in np.flatnonzero(which):
                res[was[b]] = fin_hyps(fin, b)
                steps[was[b]] = int(fin["steps"][b])
    assert bt.dec.done() and bt.done_each().all()  # (every slot is parked)
    assert all(h == [] for h in bt.end())
    bt.close()
    return res, {uid: _trim(r) for uid, r in bt.rows.items()}, bt.steps, restarts, steps


# nine utterances: (seed, eos bias by the setup's names)
QUEUE = [(1, "never"), (2, "quick"), (3, "mid"), (4, "quick"), (5, "never"), (6, "quick"), (7, "never"), (8, "quick"),
         (9, "never")]


def queue_utts(setup, queue=QUEUE):
    return [(i, setup.utt(s, setup.bias(eb))) for i, (s, eb) in enumerate(queue)]


def queue_case(sess, setup, queue=QUEUE, B=3):
    utts = queue_utts(setup, queue)
    # the inputs: tie-free, and a schedule worth the name
    lengths = []
    for _, u in utts:
        ties = []
        final, rows = setup.restate_utt(sess, u, ties)
        assert ties == []
        lengths.append(len(rows))
    calls, restarts, uses = simulate(lengths, B)
    assert len(set(lengths)) >= 3, lengths
    assert setup.maxlen in lengths, lengths
    assert {g & 1 for g, _, _ in restarts} == {0, 1}, restarts
    assert calls > 2 * setup.maxlen, calls
    assert max(uses) >= 3, uses
    assert calls < sum(max(lengths[i:i + B]) for i in range(0, len(lengths), B)), (calls, lengths)
    want, want_rows = ordinary(sess, setup, utts)
    got, got_rows, got_calls, got_restarts, steps = run_queue(sess, setup, utts, B)
    assert got_calls == calls and got_restarts == restarts, (got_calls, calls, got_restarts, restarts)
    for uid, _ in utts:
        assert got[uid] == want[uid], (uid, got[uid], want[uid])  # tokens, words, the three scores bit for bit, n_hyp
        assert got_rows[uid] == want_rows[uid], (uid, got_rows[uid], want_rows[uid])
        assert steps[uid] == n_steps(want[uid]), (uid, steps[uid])
    setup.close()


SETUPS = {
    "zero": lambda: Setup(),
    "ngram": lambda: NgramSetup(),
    "token_rows": lambda: TokenRowsSetup(),
    "row_valid": lambda: Setup(drop=0.15, K=5, V=17, Kt=6),
    "bf16_logits": lambda: Bf16LogitsSetup(mid=0.2),
}


@pytest.mark.parametrize("name", sorted(SETUPS))
def test_queue_through_three_slots(sess, name):
    """Nine utterances through three slots: each finished result and each utterance's row lists per local step equal
    the ordinary batch's; the schedule is the simulated one (restarts at odd and even global steps, a slot used three
    times, more global steps than 2 * max_output_length, fewer step calls than three at a time)."""
    queue_case(sess, SETUPS[name]())


# ---- 2. the bystander --------------------------------------------------------------------------------------------------
def bystander_case(sess, setup, seeds=((11, "never"), (12, "quick"), (13, "quick"), (14, "mid"), (15, "quick"))):
    """Slot 1 decodes one long utterance while slots 0 and 2 are finished, restarted and parked around it -- and, in the
    twin run, while they are left alone.  Its lists after every step and its result are the same."""
    by = setup.utt(seeds[0][0], setup.bias(seeds[0][1]))
    others = [setup.utt(s, setup.bias(eb)) for s, eb in seeds[1:]]
    ties = []
    assert len(setup.restate_utt(sess, by, ties)[1]) == setup.maxlen and ties == []
    script = {1: [1, 0, 0], 2: [0, 0, 1], 3: [2, 0, 1], 4: [0, 0, 2], 5: [1, 0, 0]}  # after step g: which
    out = []
    for with_finishes in (True, False):
        bt = Batch(sess, setup, [(1, others[0]), (0, by), (2, others[1])])
        spare = [(3, others[2]), (4, others[3]), (5, others[0]), (6, others[1])]
        for g in range(1, setup.maxlen + 1):
            bt.step()
            if with_finishes and g in script:
                bt.finish(script[g], {b: spare.pop(0) for b, w in enumerate(script[g]) if w == 1})
        assert bt.done_each()[1]
        fin = bt.finish([0, 1, 0])
        out.append((bt.rows[0], fin_hyps(fin, 1), int(fin["steps"][1])))
        bt.close()
    assert out[0] == out[1]
    want, want_rows = ordinary(sess, setup, [(0, by)])
    assert out[0][1] == want[0] and _trim(out[0][0]) == want_rows[0]
    setup.close()


@pytest.mark.parametrize("name", ["zero", "ngram", "token_rows"])
def test_bystander_is_untouched(sess, name):
    bystander_case(sess, SETUPS[name]())


# ---- 3. a reused slot against a fresh decoder -------------------------------------------------------------------------
def reuse_case(sess, setup, seeds=((21, "quick"), (22, "mid"), (23, "mid"))):
    utts = [setup.utt(s, setup.bias(eb)) for s, eb in seeds]
    for u in utts:
        ties = []
        setup.restate_utt(sess, u, ties)
        assert ties == []
    bt = Batch(sess, setup, [(0, utts[0]), None])
    got = {}
    for i in (1, 2, None):
        while not bt.done_each()[0]:
            bt.step()
        fin = bt.finish([1 if i is not None else 2, 0], {0: (i, utts[i])} if i is not None else None)
        got[0 if i == 1 else 1 if i == 2 else 2] = fin_hyps(fin, 0)
    rows = _trim(bt.rows[2])
    bt.close()
    want, want_rows = ordinary(sess, setup, [(2, utts[2])])  # a fresh decoder, B = 1
    assert got[2] == want[2] and rows == want_rows[2]
    setup.close()


@pytest.mark.parametrize("name", ["zero", "ngram"])
def test_third_utterance_of_a_slot_equals_a_fresh_decode(sess, name):
    reuse_case(sess, SETUPS[name]())


# ---- 4. edges --------------------------------------------------------------------------------------------------------
def edges_case(sess, setup):
    """One script over B = 3: a finish naming nothing, a slot finished right after its restart, results on the device
    against those on the host, results that survive later steps, park then restart, all slots named at once,
    fltx_s2s_end after finishes."""
    a, b_, c, d, e = (setup.utt(s, setup.bias(eb)) for s, eb in ((31, "never"), (32, "mid"), (33, "never"), (34, "quick"),
                                                                 (35, "never")))
    for u in (a, b_, c, d, e):
        ties = []
        n = len(setup.restate_utt(sess, u, ties)[1])
        assert ties == [] and (n == setup.maxlen or u in (b_, d))
    bt = Batch(sess, setup, [(0, a), (1, b_), (2, c)])
    bt.step()
    bt.step()
    # naming nothing: legal, changes nothing (Batch.finish checks that every slot lists its rows again)
    fin = bt.finish([0, 0, 0])
    assert fin["n_hyp"].tolist() == [0, 0, 0] and fin["steps"].tolist() == [0, 0, 0] and fin["hyps"] == {}
    # a running utterance aborted (slot 2, after two steps) equals fltx_s2s_end at that step on a twin decoder
    twin = Batch(sess, setup, [(2, c)])
    twin.step()
    twin.step()
    want_abort = twin.end()[0]
    twin.close()
    fin = bt.finish([0, 0, 1], {2: (3, d)})
    assert fin_hyps(fin, 2) == want_abort and fin["steps"][2] == 2 and fin["n_hyp"][:2].tolist() == [0, 0]
    # ... and the same results left on the device, which later steps do not disturb
    bt2 = Batch(sess, setup, [(2, c), (0, a)])
    bt2.step()
    bt2.step()
    _, dv = bt2.dec.finish([2, 0], results_on_device=True)
    assert device_results(sess, setup, dv, 2) == [want_abort, []]
    bt2.step()
    bt2.step()
    assert device_results(sess, setup, dv, 2) == [want_abort, []]
    bt2.close()
    # a slot finished right after its restart: the root alone, no steps; the results survive later steps
    fin = bt.finish([0, 0, 1], {2: (4, d)})
    root = [(0.0, 0.0, 0.0, [-1] * (setup.maxlen + 3), [-1] * (setup.maxlen + 3))]
    assert fin_hyps(fin, 2) == root and fin["steps"][2] == 0 and fin["n_hyp"][2] == 1
    bt.step()
    bt.step()
    # park slot 1, step (it lists nothing, the others go on), restart it
    fin = bt.finish([0, 2, 0])
    parked_result = fin_hyps(fin, 1)
    assert bt.done_each().tolist() == [False, True, bt.done_each()[2]]
    bt.step()
    assert bt.slot_lists(1) == [] and bt.slot_lists(0) != []
    fin = bt.finish([0, 2, 0])  # (parked again: nothing changes, nothing to report)
    assert fin["n_hyp"][1] == 0 and fin["steps"][1] == 0 and fin["status"][1] == 0
    fin = bt.finish([0, 1, 0], {1: (5, e)})
    assert fin["n_hyp"][1] == 0 and fin["steps"][1] == 0 and fin["status"][1] == 0 and fin["hyps"][1] == []
    # restarted at global step 5, the slot still gets its max_output_length steps
    assert bt.steps == 5
    while not bt.done_each().all():
        bt.step()
        assert bt.dec.done() == bool(bt.done_each().all())
    assert bt.steps == 5 + setup.maxlen
    want, want_rows = ordinary(sess, setup, [(0, a), (5, e), (4, d)])
    assert parked_result == twin_prefix(sess, setup, b_, 4)
    assert all(_trim(bt.rows[u]) == want_rows[u] for u in (0, 5, 4))
    # all slots named at once; then fltx_s2s_end: the restarted slots' roots, the parked slot's nothing
    fin = bt.finish([1, 2, 1])
    assert [fin_hyps(fin, b) for b in range(3)] == [want[0], want[5], want[4]]
    assert fin["steps"].tolist() == [setup.maxlen, setup.maxlen, n_steps(want[4])]
    assert bt.end() == [root, [], root]
    assert sess.lib.lib.fltx_s2s_finish(bt.dec.h, None, None, None, None, None, None, 0, None) == _capi.ERR_STATE
    bt.close()
    setup.close()


def twin_prefix(sess, setup, u, steps):
    """fltx_s2s_end after `steps` steps of utterance u alone"""
    t = Batch(sess, setup, [(0, u)])
    for _ in range(steps):
        t.step()
    out = t.end()[0]
    t.close()
    return out


def device_results(sess, setup, dv, B):
    """the results a finish left on the device (its dict of addresses): -> [hyps] per slot"""
    K, ln = setup.K, setup.maxlen + 3
    assert dv["length"] == ln
    n_hyp = read_device(sess, dv["n_hyp"], B, np.int32)
    assert read_device(sess, dv["status"], B, np.int32).tolist() == [0] * B
    sc = read_device(sess, dv["scores"], 3 * B * K, np.float64).reshape(B * K, 3)
    out = []
    for b in range(B):
        n = int(n_hyp[b])
        tk = read_device(sess, dv["tokens"] + 4 * b * K * ln, n * ln, np.int32).reshape(n, ln)
        wd = read_device(sess, dv["words"] + 4 * b * K * ln, n * ln, np.int32).reshape(n, ln) if dv["words"] else \
            np.full((n, ln), -1, np.int32)
        out.append([(float(sc[b * K + i, 0]), float(sc[b * K + i, 1]), float(sc[b * K + i, 2]), tk[i].tolist(),
                     wd[i].tolist()) for i in range(n)])
    return out


@pytest.mark.parametrize("K", [1, 4, 70])
def test_edges(sess, K):
    edges_case(sess, Setup(K=K, V=40, Kt=12, eos=5))


def test_refusals(sess):
    L, ctx = sess.lib.lib, sess.ctx
    setup = Setup()
    dec = setup.make_dec(sess)
    fo = _capi.S2sFinishedOut()
    w = np.zeros(2, np.int32)
    done = np.zeros(2, np.int32)

    def finish(d, which, lists, fo_=fo, word=None):
        a = [None if x is None else _capi.Seq2SeqBatchDecoder._addr(x) for x in lists]
        return L.fltx_s2s_finish(d.h, None if which is None else which.ctypes.data, *a, word, 0,
                                 None if fo_ is None else C.byref(fo_))
    dec.B = 2
    lists = dec._rows()
    assert finish(dec, w, lists) == _capi.ERR_STATE  # before fltx_s2s_begin
    assert L.fltx_s2s_done_each(dec.h, done.ctypes.data) == _capi.ERR_STATE
    dec.begin(2, setup.V)
    assert finish(dec, None, lists) == _capi.ERR_INVALID
    assert finish(dec, w, lists, None) == _capi.ERR_INVALID
    for i in range(4):
        assert finish(dec, w, [None if j == i else x for j, x in enumerate(lists)]) == _capi.ERR_INVALID
    for bad in (3, -1):
        assert finish(dec, np.array([0, bad], np.int32), lists) == _capi.ERR_INVALID
    assert L.fltx_s2s_done_each(dec.h, None) == _capi.ERR_INVALID
    assert finish(dec, w, lists) == _capi.FLTX_OK
    dec.end()
    assert finish(dec, w, lists) == _capi.ERR_STATE  # after fltx_s2s_end
    dec.begin(2, setup.V)
    assert finish(dec, w, lists) == _capi.FLTX_OK
    dec.close()
    bd = _capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(4, 4), sess.zero, 0, 1)
    assert finish(bd, w, lists) == _capi.ERR_STATE  # not a seq2seq decoder
    assert L.fltx_s2s_done_each(bd.h, done.ctypes.data) == _capi.ERR_STATE
    bd.close()


# ---- 5. decode_queue ---------------------------------------------------------------------------------------------------
def decode_queue_case(sess, setup, queue=QUEUE, B=3):
    """Seq2SeqBatchDecoder.decode_queue returns, in queue order, the ordinary batch's results -- and on the GPU what
    decode() returns for the same utterances."""
    utts = queue_utts(setup, queue)
    want, _ = ordinary(sess, setup, utts)
    K = setup.K

    def make_step_fn(slot_of):
        pre = {}

        def step_fn(token, src_row, row_mask, t, slot_utt=None, restarted=None):
            tok, src, mask = _np(token), _np(src_row), _np(row_mask)
            nb = len(tok) // K
            su = slot_of(nb) if slot_utt is None else slot_utt
            new = {}
            for r in np.flatnonzero(mask):
                b = int(r) // K
                if src[r] < 0:
                    assert tok[r] == -1 and (restarted is None or restarted[b])
                    new[int(r)] = []
                else:
                    new[int(r)] = pre[int(src[r])] + [int(tok[r])]
            pre.clear()
            pre.update(new)
            state = {(r // K, r % K): (utts[int(su[r // K])][1], p, []) for r, p in new.items()}
            return tuple(_dev(sess, m) for m in setup.matrices(nb, state) if m is not None)
        return step_fn

    dec = setup.make_dec(sess)
    got = dec.decode_queue(make_step_fn(None), len(utts), B, setup.V, check_every=2)
    assert [_hyps(h) for h in got] == [want[i] for i in range(len(utts))]
    # fewer utterances than slots: the spare slot is parked before the first step, and the roots still arrive as roots
    # (src_row -1: step_fn above asserts it)
    few = dec.decode_queue(make_step_fn(None), B - 1, B, setup.V, check_every=2)
    assert [_hyps(h) for h in few] == [want[i] for i in range(B - 1)]
    if is_gpu(sess) and setup.W is None:  # (decode() takes torch row lists, and no LM rows)
        whole = dec.decode(make_step_fn(lambda nb: np.arange(nb)), len(utts), setup.V)
        assert [_hyps(h) for h in whole] == [_hyps(h) for h in got]
    dec.close()
    setup.close()


@pytest.mark.parametrize("name", ["zero", "token_rows"])
def test_decode_queue(sess, name):
    decode_queue_case(sess, SETUPS[name]())


# ---- the GPU cases, in a fresh process ------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_S2S_FINISH_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
