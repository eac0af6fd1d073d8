"""Recycled LM-state ids on streams of the lexicon-free CTC rows decoder (fltx_ctc_rows_stream_collect,
text_amd/csrc/fltx_ctc_rows_stream.h): a stream that enters more states than its table holds runs to its end when the
caller collects, and decides what the float64 restatement of tests/test_ctc_lm_rows_stream.py decides -- whose states are
token prefixes, which never run out.

`RecyclingStreams` is that module's DeviceStreams with a tracker of the caller's contract (a released id is dropped; an id
it does not hold is a new state, the parent's prefix plus the row's token; any other id names the prefix it had) and a
`Model` of the rules on the tracker's own data: the table is the ids the tracker holds with each id's parent, the beam
the last row list.  After every collect the released list must be the model's dead set exactly -- ascending, -1 behind
it -- and n_live the model's count.

Every device test runs on the emulator library and -- marked `gpu` -- on the HIP library, in a fresh child process that
initialises torch first (as tests/test_seq2seq.py explains).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD = os.environ.get("FLTX_CTC_LMROWS_RECYCLE_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
from golden import make_ctc_lm_rows_golden as G  # noqa: E402
import test_ctc_lm_rows_stream as S0  # noqa: E402
from test_ctc_lm_rows import MIN_GAP, PrefixLM, Stats, _dev, assert_final, make_dec  # noqa: E402
from test_seq2seq_model_output import _bits_equal, _GpuSess, _np, is_gpu  # noqa: E402

MAX_STATES = 32
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


# ---- the rules, on any table ---------------------------------------------------------------------------------------------
class Model:
    """A stream's table as the caller can know it: {id: the parent id of its entry, None: no entry}"""

    def __init__(self, root):
        self.par = {root: None}

    def enter(self, sid, parent):
        assert self.par.setdefault(sid, parent) == parent, (sid, parent, self.par[sid])

    def dead(self, sids, psids):
        """the allocated ids that are neither in R -- the beam's sids and all below them in the table tree -- nor a psid
        of the beam, ascending"""
        kids = {}
        for s, p in self.par.items():
            if p is not None:
                kids.setdefault(p, []).append(s)
        reach, todo = set(sids), list(sids)
        while todo:
            for c in kids.get(todo.pop(), ()):
                if c not in reach:
                    reach.add(c)
                    todo.append(c)
        pinned = reach | set(psids)
        return sorted(s for s in self.par if s not in pinned)

    def release(self, ids):
        """the ids go, and so does every entry below one of them: the child keeps its id and has no entry"""
        ids = set(ids)
        for i in ids:
            del self.par[i]
        for s, p in self.par.items():
            if p in ids:
                self.par[s] = None


def table_profile(rows, collect_at, root=()):
    """The rules on the restatement's own row lists (states are prefixes; a state's parent is the prefix without its last
    edge), collecting after the frame counts in collect_at.
    -> (states ever entered, the largest table between collects, the most released by one collect)"""
    m = Model(root)
    ever, peak, most = {root}, 1, 0
    beam = [root]
    at = sorted(collect_at)
    for t in range(len(rows) + 1):
        if t > 0:
            for _, _, s in rows[t - 1]:
                if s not in m.par:
                    assert s not in ever, "a released state was entered again"
                    ever.add(s)
                    m.enter(s, s[:-1])
            beam = [s for _, _, s in rows[t - 1]]
            peak = max(peak, len(m.par))
        for _ in range(at.count(t)):
            dead = m.dead(beam, [s[:-1] for s in beam if s != root])
            most = max(most, len(dead))
            m.release(dead)
    return len(ever), peak, most


# ---- the device loop with the caller's contract ----------------------------------------------------------------------------
class RecyclingStreams(S0.DeviceStreams):
    """DeviceStreams whose ids come back: self.prefix is the tracker, self.model[b] the rules on what the tracker holds,
    self.psid the parent id each hypothesis of the last row list was made from, self.named[b] the row lists with the
    prefix each id stood for when it was listed"""

    def __init__(self, sess, dec, B, N, W, lm_row, max_frames, lexicon=False):
        self.model = [Model(0) for _ in range(B)]
        self.psid = None
        self.named = [[] for _ in range(B)]
        self.ever = [1] * B
        self.stopped = set()
        S0.DeviceStreams.__init__(self, sess, dec, B, N, W, lm_row, max_frames, lexicon)

    def _take(self, out, stepped, first=False):
        if is_gpu(self.sess):
            self.dec.ctx.synchronize()
        tok, src, state, n = [_np(a).copy() for a in out]
        B, K = self.B, self.K
        psid = np.full((B, K), -1, np.int64) if first else self.psid.copy()
        for b in range(B):
            if first or not stepped[b]:
                continue
            nb = int(n[b])
            for k in range(nb):
                s = int(src[b, k]) - b * K
                par = int(self.prev_state[b, s])
                if tok[b, k] >= 0:
                    psid[b, k] = par
                    if int(state[b, k]) not in self.prefix[b]:  # an id the tracker does not hold: a new state
                        self.ever[b] += int(state[b, k]) not in self.model[b].par
                        self.model[b].enter(int(state[b, k]), par)
                else:
                    psid[b, k] = self.psid[b, s]
            psid[b, nb:] = -1
        S0.DeviceStreams._take(self, out, stepped, first)
        self.psid = psid
        for b in range(B):
            if not first and stepped[b]:
                assert set(self.model[b].par) == set(self.prefix[b]), b
                self.named[b].append([(s, t, self.prefix[b][i]) for s, t, i in self.rows[b][-1]])

    def chunk(self, parts, extra_steps=0, collect_first=False):
        """collect_first: a collect between the append and the chunk's steps"""
        if not collect_first:
            return S0.DeviceStreams.chunk(self, parts, extra_steps)
        Ts = [p.shape[0] for p in parts]
        flat = np.concatenate([p.reshape(-1) for p in parts]) if sum(Ts) else np.zeros(0, np.float32)
        steps = self.dec.append(flat, Ts)
        released = self.collect()
        for t in range(steps + extra_steps):
            self._take(self.dec.step(self.lm_rows()), [t < T for T in Ts])
        return released

    def collect(self, cap=None):
        """dec.collect(cap), held to the model -> the released ids per stream"""
        rel, n_rel, n_live = self.dec.collect(cap)
        if is_gpu(self.sess):
            self.dec.ctx.synchronize()
        rel, n_rel, n_live = _np(rel), _np(n_rel), _np(n_live)
        width = rel.shape[1]
        assert rel.shape == (self.B, self.dec._stream_states if cap is None else cap)
        out = []
        for b in range(self.B):
            want = []
            if b not in self.stopped:
                nb = int(self.prev_n[b])
                dead = self.model[b].dead([int(s) for s in self.prev_state[b, :nb]],
                                          [int(p) for p in self.psid[b, :nb] if p >= 0])
                want = dead[:width]
            print("collect: stream %d releases %s, model %s" % (b, rel[b, :int(n_rel[b])].tolist(), want))
            assert rel[b].tolist() == want + [-1] * (width - len(want)), (b, rel[b].tolist(), want)
            assert int(n_rel[b]) == len(want), b
            self.model[b].release(want)
            for i in want:
                del self.prefix[b][i]
            if b not in self.stopped:
                assert int(n_live[b]) == len(self.model[b].par), (b, int(n_live[b]), len(self.model[b].par))
            out.append(want)
        return out


def run_recycling(sess, dec, ems, N, W, lm_row, cuts, look_back, max_frames, lexicon=False, collect=True, cap=None):
    """Per chunk of `cuts` ([frames of stream b]): the chunk, prune(look_back), collect (held to the model), best(b, 0).
    -> (bests per stream, final per stream, the RecyclingStreams)"""
    B = len(ems)
    ds = RecyclingStreams(sess, dec, B, N, W, lm_row, max_frames, lexicon)
    at = [0] * B
    bests = [[] for _ in range(B)]
    for cut in cuts:
        ds.chunk([ems[b][at[b]:at[b] + cut[b]] for b in range(B)])
        at = [a + c for a, c in zip(at, cut)]
        dec.prune(look_back)
        if collect:
            ds.collect(cap)
        for b in range(B):
            bests[b].append(ds.best(b, 0))
    assert at == [e.shape[0] for e in ems]
    return bests, ds.end(), ds


def stream_cuts(Ts, sizes, late=()):
    """chunks of unequal lengths: stream b takes sizes[b] in turn (0: idle for that chunk) until its T[b] frames are
    used up; a stream in `late` is idle for the first eight chunks"""
    left, cuts, i = list(Ts), [], 0
    while any(left):
        cut = []
        for b, s in enumerate(sizes):
            c = 0 if (b in late and i < 8) else min(left[b], s[i % len(s)])
            cut.append(c)
            left[b] -= c
        cuts.append(cut)
        i += 1
    return cuts


def script_of(cuts, b, look_back):
    return [x for c in cuts for x in (("c", c[b]), ("p", look_back), ("b", 0))]


def collect_points(cuts, b):
    """the frames stream b has decoded at each collect"""
    return list(np.cumsum([c[b] for c in cuts]))


def last3(rl):
    """an LM that reads the last three tokens of the prefix: the states stay distinct, the beam does not narrow"""
    return lambda p: rl.row(list(p[-3:]))


_CASES = {}


def long_case(log_add, K=6, Ts=(300, 150, 80), base=1200):
    """Emissions, restatement and table profile of the long streams; seeds without ties (and, under logAdd, without a
    gap below MIN_GAP), shared by the tests that use the case"""
    key = (log_add, K, Ts, base)
    if key in _CASES:
        return _CASES[key]
    N, W, Kt, sil, blank, lb = 5, 7, 5, 0, 1, 2
    rl = G.SmRowsLM(91, N, W, 41, W - 1, 0)
    sizes = ([7, 13, 10, 20], [5, 0, 10, 10], [4, 6]) if len(Ts) > 1 else ([10],)
    cuts = stream_cuts(Ts, sizes[:len(Ts)], late=(2,))
    ems, want, prof = [], [], []
    for b, T in enumerate(Ts):
        for seed in range(base + 100 * b, base + 100 * b + 60):
            st = Stats()
            em = G.emissions(seed, T, N)
            res = S0.restate_stream(em, PrefixLM(last3(rl), rl.usr_to_lm, rl.finish), K, Kt, 25.0, 0.7, -0.3, sil, blank,
                                    log_add, script_of(cuts, b, lb), st=st)
            if not st.ties and (not log_add or st.gap > MIN_GAP):
                break
        assert not st.ties and (not log_add or st.gap > MIN_GAP), (b, st.ties, st.gap)
        ems.append(em)
        want.append(res)
        prof.append(table_profile(res[3], collect_points(cuts, b)))
    _CASES[key] = dict(N=N, W=W, K=K, Kt=Kt, sil=sil, blank=blank, lb=lb, rl=rl, cuts=cuts, ems=ems, want=want, prof=prof,
                       log_add=log_add)
    return _CASES[key]


def case_dec(sess, c, max_states):
    lm = _capi.RowsLM(c["W"], c["rl"].usr_to_lm, c["W"] - 1, lib=sess.lib)
    dec = make_dec(sess, lm, c["K"], c["Kt"], 25.0, 0.7, -0.3, c["sil"], c["blank"], c["log_add"])
    dec.set_max_states(max_states)
    return lm, dec


def assert_against_restatement(c, bests, final, ds, final_check=assert_final):
    """rows, bests and n-best of every stream against the restatement"""
    for b, (w_best, _, w_final, w_rows) in enumerate(c["want"]):
        assert len(ds.named[b]) == len(w_rows), b
        for t, (wr, gr) in enumerate(zip(w_rows, ds.named[b])):
            assert gr == [tuple(x) for x in wr], (b, t, gr, wr)
        assert len(bests[b]) == len(w_best)
        for i, (w, g) in enumerate(zip(w_best, bests[b])):
            S0.assert_best(w, g, c["log_add"], (b, "best", i), final=final_check)
        final_check(w_final, final[b], c["log_add"], (b, "final"))


# ---- 1. long streams through a small table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("log_add", [False, True])
def test_long_streams_through_a_small_table(sess, log_add):
    """300, 150 and 80 frames (the last stream idle for eight chunks) in tables of 32 ids, prune(2) and collect after
    every chunk: every row list names the restatement's states, every best and the n-best are the restatement's, every
    collect releases the model's dead set."""
    c = long_case(log_add)
    ever, peak, _ = c["prof"][0]
    print("states ever / peak table / most released per stream:", c["prof"])
    assert ever > MAX_STATES, "the stream would pass without recycling"
    assert all(p[1] <= MAX_STATES for p in c["prof"]), "the table must hold what lives between two collects"
    lm, dec = case_dec(sess, c, MAX_STATES)
    bests, final, ds = run_recycling(sess, dec, c["ems"], c["N"], c["W"], lambda b, p: last3(c["rl"])(p), c["cuts"],
                                     c["lb"], 32)
    assert_against_restatement(c, bests, final, ds)
    assert ds.ever[0] == ever and max(max(ds.prefix[b]) for b in range(3)) < MAX_STATES
    dec.close()
    lm.close()


# ---- 2. the default is unchanged -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_add", [False, True])
def test_without_collect_the_table_fills_and_a_large_one_decides_the_same(sess, log_add):
    """No collect at max_states = 32: the long stream stops with "LM-state table full", as it always did.  No collect in
    a large table: bests and n-best bit for bit those of the recycled run."""
    c = long_case(log_add)
    lm, dec = case_dec(sess, c, MAX_STATES)
    ds = S0.DeviceStreams(sess, dec, 3, c["N"], c["W"], lambda b, p: last3(c["rl"])(p), 32)
    at = [0, 0, 0]
    for cut in c["cuts"]:
        ds.chunk([c["ems"][b][at[b]:at[b] + cut[b]] for b in range(3)])
        at = [a + x for a, x in zip(at, cut)]
        dec.prune(c["lb"])
    with pytest.raises(_capi.FltxError) as e:
        dec.best(0)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "LM-state table full" in str(e.value)
    dec.close()
    plain_dec = case_dec(sess, c, 4096)
    plain = run_recycling(sess, plain_dec[1], c["ems"], c["N"], c["W"], lambda b, p: last3(c["rl"])(p), c["cuts"], c["lb"],
                          32, collect=False)
    small_dec = case_dec(sess, c, MAX_STATES)
    small = run_recycling(sess, small_dec[1], c["ems"], c["N"], c["W"], lambda b, p: last3(c["rl"])(p), c["cuts"], c["lb"],
                          32)
    assert plain[2].ever[0] == len(plain[2].prefix[0]) > MAX_STATES
    for b in range(3):
        assert len(plain[0][b]) == len(small[0][b]) and len(plain[1][b]) == len(small[1][b]) > 1
        for p, s in zip(plain[0][b] + plain[1][b], small[0][b] + small[1][b]):
            assert p[3] == s[3] and _bits_equal(p[:3], s[:3]), (b, p, s)
        assert plain[2].named[b] == small[2].named[b]
    for d in plain_dec + small_dec + (lm,):
        d.close()


# ---- 3. a beam wider than a wave -------------------------------------------------------------------------------------------
def test_wide_beam(sess):
    """K = 70, 200 frames in chunks of 10, a table of 256: the marks, the prefix sum and the released list cross waves
    and the rebuild sees many entries"""
    c = long_case(False, K=70, Ts=(200,), base=1600)
    ever, peak, most = c["prof"][0]
    print("states ever / peak table / most released:", c["prof"][0])
    # more states than the table, a table and a beam wider than a wave, a released list longer than a quarter wave
    assert ever > 256 >= peak > 64 and most > 16 and max(len(r) for r in c["want"][0][3]) > 64
    lm, dec = case_dec(sess, c, 256)
    bests, final, ds = run_recycling(sess, dec, c["ems"], c["N"], c["W"], lambda b, p: last3(c["rl"])(p), c["cuts"],
                                     c["lb"], 16)
    assert_against_restatement(c, bests, final, ds)
    assert ds.ever[0] == ever
    dec.close()
    lm.close()


# ---- 3b. a table too large for the kernel's LDS ----------------------------------------------------------------------------
def test_table_beyond_the_lds_bitsets(sess):
    """max_states = 65 600 > 65 536: the collect kernel keeps its mark bits in the HBM scratch, two streams side by side
    (the scratch, the id arrays and the released lists are per stream); held to the model and the restatement as ever.
    set("max_states") is what set_max_states calls, and one given during the stream changes neither the open
    stream's table nor collect's default cap."""
    c = long_case(False, Ts=(120, 80), base=1900)
    lm, dec = case_dec(sess, c, 32)
    dec.set("max_states", 65600)
    ds = RecyclingStreams(sess, dec, 2, c["N"], c["W"], lambda b, p: last3(c["rl"])(p), 32)
    dec.set_max_states(77)  # (for the next begin)
    at, bests, released = [0, 0], [[], []], 0
    for cut in c["cuts"]:
        ds.chunk([c["ems"][b][at[b]:at[b] + cut[b]] for b in range(2)])
        at = [a + x for a, x in zip(at, cut)]
        dec.prune(c["lb"])
        released += sum(len(r) for r in ds.collect())  # (asserts the list's shape: [2, 65 600])
        for b in range(2):
            bests[b].append(ds.best(b, 0))
    assert released > 64 and min(len(ds.collect(5)[b]) for b in range(2)) == 0
    assert_against_restatement(c, bests, ds.end(), ds)
    dec.close()
    lm.close()


# ---- 4. a cap below the dead set -------------------------------------------------------------------------------------------
def test_release_cap_smaller_than_the_dead_set(sess):
    """collect(3): the three lowest dead ids go now, the others at the following calls with no step in between; their
    union is the dead set, and the stream decides what it decides without a cap"""
    c = long_case(False)
    lm, dec = case_dec(sess, c, MAX_STATES)
    B = 3
    ds = RecyclingStreams(sess, dec, B, c["N"], c["W"], lambda b, p: last3(c["rl"])(p), 32)
    at = [0] * B
    bests = [[] for _ in range(B)]
    most = 0
    for cut in c["cuts"]:
        ds.chunk([c["ems"][b][at[b]:at[b] + cut[b]] for b in range(B)])
        at = [a + x for a, x in zip(at, cut)]
        dec.prune(c["lb"])
        dead = [ds.model[b].dead([int(s) for s in ds.prev_state[b, :int(ds.prev_n[b])]],
                                 [int(p) for p in ds.psid[b, :int(ds.prev_n[b])] if p >= 0]) for b in range(B)]
        most = max(most, max(len(d) for d in dead))
        got = [[] for _ in range(B)]
        for call in range(1 + max(len(d) for d in dead) // 3):
            for b, ids in enumerate(ds.collect(3)):
                assert ids == dead[b][3 * call:3 * call + 3], (b, call)
                got[b] += ids
        assert got == dead and ds.collect(3) == [[]] * B
        for b in range(B):
            bests[b].append(ds.best(b, 0))
    assert most > 3
    assert_against_restatement(c, bests, ds.end(), ds)
    dec.close()
    lm.close()


# ---- 5. other call sequences ------------------------------------------------------------------------------------------------
def test_collect_between_append_and_steps_and_twice(sess):
    """A collect between the append and the chunk's steps sees the beam before the chunk; a second collect in a row
    releases nothing; one right after stream_begin releases nothing; after end a new begin starts the ids over."""
    c = long_case(False)
    lm, dec = case_dec(sess, c, MAX_STATES)
    B = 3
    for again in range(2):
        ds = RecyclingStreams(sess, dec, B, c["N"], c["W"], lambda b, p: last3(c["rl"])(p), 32)
        assert ds.collect() == [[]] * B  # (right after begin: the root is the beam)
        at = [0] * B
        bests = [[] for _ in range(B)]
        released = 0
        for i, cut in enumerate(c["cuts"]):
            rel = ds.chunk([c["ems"][b][at[b]:at[b] + cut[b]] for b in range(B)], collect_first=True)
            released += sum(len(r) for r in rel)
            at = [a + x for a, x in zip(at, cut)]
            if i == 0:  # (the ids of a stream that begins: 0, then 1, 2, ... in the first frame's beam)
                assert sorted(ds.prefix[0]) == list(range(len(ds.prefix[0])))
            dec.prune(c["lb"])
            if i % 3 == 2:
                ds.collect()
                assert ds.collect() == [[]] * B
            for b in range(B):
                bests[b].append(ds.best(b, 0))
        assert released > MAX_STATES
        assert_against_restatement(c, bests, ds.end(), ds)
    dec.close()
    lm.close()


def test_collect_leaves_a_stopped_stream_alone(sess):
    """max_states = 4 (tests/test_ctc_lm_rows_stream.py's stopped stream): stream 0 stops on a full table and collect
    neither releases its ids nor clears its status; stream 1 beside it collects and goes on"""
    N, K, W, sil, blank = 4, 6, 4, 0, 1
    flat = np.full((1, N), -5.0, np.float32)
    flat[0, blank] = 0.0
    ems = [G.emissions(800, 9, N) * np.float32(0.25), np.repeat(flat, 9, axis=0)]
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 2.0, 0.7, 0.0, sil, blank, False)
    dec.set_max_states(4)
    dec.stream_begin(2, N, 6)
    lr = _dev(sess, np.zeros((2 * K, W), np.float32))
    at = 0
    for T in (3, 3, 3):
        flat_in = np.concatenate([e[at:at + T].reshape(-1) for e in ems])
        for _ in range(dec.append(flat_in, [T, T])):
            tok, src, state, n = dec.step(lr)
        at += T
        dec.prune(1)
        out = dec.collect()
        dec.ctx.synchronize()
        rel, n_rel, n_live = [_np(a) for a in out]
        assert int(_np(n)[0]) == 0 and int(n_rel[0]) == 0 and (rel[0] == -1).all() and rel.shape == (2, 4)
        assert int(n_live[1]) >= 1 and int(n_rel[1]) == int((rel[1] >= 0).sum())
        with pytest.raises(_capi.FltxError) as e:
            dec.best(0)
        assert e.value.code == _capi.ERR_UNSUPPORTED and "LM-state table full" in str(e.value)
        assert dec.best(1).tokens.tolist()[-1] == blank
    dec.end(lr)
    with pytest.raises(_capi.FltxError) as e:
        dec.count(0)
    assert e.value.code == _capi.ERR_UNSUPPORTED and "LM-state table full" in str(e.value)
    assert dec.results(1)[0].tokens.tolist()[-2:] == [blank, sil]
    dec.close()
    lm.close()


# ---- 7. contract and refusals -----------------------------------------------------------------------------------------------
def test_contract_and_refusals(sess):
    import ctypes as C
    L, ctx = sess.lib, sess.ctx
    I, S = _capi.ERR_INVALID, _capi.ERR_STATE
    N, K = 6, 4
    lm = _capi.RowsLM(N + 1, None, N, lib=L)
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    dec.B = 1
    outs = dec._rows()
    po = [dec._addr(o) for o in outs]
    bufs = [_dev(sess, np.zeros(8, np.int32)) for _ in range(3)]
    pr, pn, pl = [dec._addr(x) for x in bufs]
    em = G.emissions(900, 6, N)
    T3 = np.asarray([3], np.int32)
    collect = L.lib.fltx_ctc_rows_stream_collect
    lr = _dev(sess, np.zeros((K, N + 1), np.float32))
    plr = dec._addr(lr)
    # outside a stream; on a rows decoder begun with fltx_ctc_rows_begin, which decodes as it did
    assert collect(dec.h, 8, pr, pn, pl) == S
    assert L.lib.fltx_ctc_rows_begin(dec.h, em.ctypes.data, 0, None, T3.ctypes.data, 1, N, *po) == 0
    assert collect(dec.h, 8, pr, pn, pl) == S
    for _ in range(3):
        assert L.lib.fltx_ctc_rows_step(dec.h, plr, 0, 0, N + 1, None, 0, 1, None, *po) == 0
    assert L.lib.fltx_ctc_rows_end(dec.h, plr, 0, 0, N + 1, None, 0, 1, None) == 0
    offline = [(h.score, h.tokens.tolist()) for h in dec.results(0)]
    assert offline and collect(dec.h, 8, pr, pn, pl) == S
    # in a stream: the arguments
    assert L.lib.fltx_ctc_rows_stream_begin(dec.h, 1, N, 8, *po) == 0
    assert collect(dec.h, 0, pr, pn, pl) == I and collect(dec.h, -1, pr, pn, pl) == I
    assert collect(dec.h, 8, None, pn, pl) == I and collect(dec.h, 8, pr, None, pl) == I
    assert "fltx_ctc_rows_stream_collect" in L.lib.fltx_last_error().decode()
    assert L.lib.fltx_ctc_rows_stream_append(dec.h, em.ctypes.data, 0, None, T3.ctypes.data) == 0
    for _ in range(3):
        assert L.lib.fltx_ctc_rows_step(dec.h, plr, 0, 0, N + 1, None, 0, 1, None, *po) == 0
    assert collect(dec.h, 8, pr, pn, None) == 0  # n_live may be NULL
    dec.ctx.synchronize()
    first = (_np(bufs[0]).copy(), int(_np(bufs[1])[0]))
    assert collect(dec.h, 8, pr, pn, pl) == 0
    dec.ctx.synchronize()
    assert first[1] == int((first[0] >= 0).sum()) and int(_np(bufs[1])[0]) == 0 and int(_np(bufs[2])[0]) >= 1
    assert L.lib.fltx_ctc_rows_end(dec.h, plr, 0, 0, N + 1, None, 0, 1, None) == 0
    # the same frames, streamed and collected: the offline n-best with decodeEnd's layout
    assert [(h.score, h.tokens.tolist()) for h in dec.results(0)] == offline
    # fltx_stream_* stay refused on this kind; the call is refused on the other kinds
    assert L.lib.fltx_stream_begin(dec.h, 1, N, 10) == S and L.lib.fltx_stream_prune(dec.h, 0) == S
    other = _capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(K, N, lm_weight=0.5), sess.zero, 0, 1)
    s2s = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    for o in (other, s2s):
        assert collect(o.h, 8, pr, pn, pl) == S
        o.close()
    other = _capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(K, N, lm_weight=0.5), sess.zero, 0, 1)
    other.stream_begin(1, N, 10)  # an n-gram stream compacts its own ids, as before
    assert collect(other.h, 8, pr, pn, pl) == S
    other.close()
    assert collect(None, 8, pr, pn, pl) == I
    dec.close()
    lm.close()


# ---- 8. the Python helper ---------------------------------------------------------------------------------------------------
def test_python_helper_collects(sess, monkeypatch):
    """decode_stream(collect_every=1) yields what decode_stream yields; on_release is told every released id, once; the
    lister's store stays within the most rows that live at once, which the plain run's outgrows"""
    c = long_case(False, Ts=(120, 80), base=1900)
    B, N, W, K = 2, c["N"], c["W"], c["K"]
    chunks, at = [], [0, 0]
    for cut in c["cuts"]:
        chunks.append((np.concatenate([c["ems"][b][at[b]:at[b] + cut[b]].reshape(-1) for b in range(B)]), list(cut)))
        at = [a + x for a, x in zip(at, cut)]
    listers = []

    base = _capi._RowLister

    class Lister(base):
        def __init__(self, *a):
            base.__init__(self, *a)
            listers.append(self)
    monkeypatch.setattr(_capi, "_RowLister", Lister)

    def lm_rows(keys):
        return _dev(sess, np.stack([last3(c["rl"])(p) for _, p in keys]))

    def run(**kw):
        lm, dec = case_dec(sess, c, MAX_STATES if kw else 4096)
        seen, told = [], []
        inner = dec.collect

        def spy(*a):
            out = inner(*a)
            dec.ctx.synchronize()
            seen.extend((b, int(i)) for b in range(B) for i in _np(out[0])[b] if i >= 0)
            return out
        dec.collect = spy
        if kw:
            kw["on_release"] = lambda b, ids: told.extend((b, i) for i in ids)
        outs = list(dec.decode_stream(chunks, lm_rows, look_back=c["lb"], N=N, max_frames=32, **kw))
        res = [[(h.score, h.am, h.lm, h.tokens.tolist()) for h in o] for o in outs[:-1]]
        res.append([[(h.score, h.am, h.lm, list(h.tokens)) for h in hyps] for hyps in outs[-1]])
        dec.close()
        lm.close()
        return res, seen, told
    plain, seen0, _ = run()
    got, seen, told = run(collect_every=1)
    assert not seen0 and told == seen and len(seen) > MAX_STATES
    assert got == plain
    for b in range(B):  # and both are the restatement's
        assert_final(c["want"][b][2], got[-1][b], False, b)
    bound = sum(p[1] for p in c["prof"])  # every stream's largest table between two collects
    ever = sum(p[0] for p in c["prof"])
    print("store rows: plain %d, collecting %d; bound %d, states ever %d" % (listers[0].n_store, listers[1].n_store, bound,
                                                                           ever))
    assert listers[1].n_store <= bound < listers[0].n_store == ever
    assert len(listers[1].row_of) == len(listers[1].prefix) <= bound


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_CTC_LMROWS_RECYCLE_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
