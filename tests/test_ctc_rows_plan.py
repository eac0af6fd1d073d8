"""The LM rows of the lexicon-free CTC rows decoder planned on the device (fltx_ctc_rows_plan_begin / _plan /
_plan_release, text_amd/csrc/fltx_ctc_rows_plan.h).

`PlanModel` restates the contract's loop: one dict per utterance, a list as the free stack.  `planned_decode` and
`PlannedStreams` drive real decodes with the planner's lm_row_of -- the LM rows are written into a store at new_row, from
the prefix that (new_parent_row, new_edge) name -- and after EVERY plan every output and the counts must equal the
model's exactly.  The decodes themselves are held to the reference fixtures and to the float64 restatement of
tests/test_ctc_lm_rows.py (tokens exact, scores bit-identical; logAdd within the project's 1e-5).

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

CHILD = os.environ.get("FLTX_CTC_ROWS_PLAN_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
from golden import make_ctc_lm_rows_golden as G  # noqa: E402
import test_ctc_lm_rows as C0  # noqa: E402
import test_ctc_lm_rows_recycle as R  # noqa: E402
from test_ctc_lm_rows import MIN_GAP, PrefixLM, Stats, _dev, assert_final, assert_rows, make_dec  # noqa: E402
from test_seq2seq_model_output import _GpuSess, _np, is_gpu  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
NAMES = ("lm_row_of", "new_row", "new_parent_row", "new_edge", "new_dec_row", "counts")


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


# ---- the contract's loop -------------------------------------------------------------------------------------------------
class PlanModel:
    def __init__(self, B, K, s_max, cap):
        self.B, self.K, self.s_max, self.cap = B, K, s_max, cap
        self.row_of = [dict() for _ in range(B)]
        self.free, self.hw, self.dropped = [], 0, 0
        self.prev = np.full(B * K, -1, np.int32)

    def plan(self, tok, src, state, n):
        """flat lists -> [lm_row_of, new_row, new_parent_row, new_edge, new_dec_row, counts]"""
        B, K = self.B, self.K
        ro, rows, pars, edges, decs = [np.full(B * K, -1, np.int32) for _ in range(5)]
        n_new = 0
        for b in range(B):
            for k in range(int(n[b])):
                i, s = b * K + k, int(state[b * K + k])
                if not 0 <= s < self.s_max:
                    continue
                if s not in self.row_of[b]:
                    if self.free:
                        r = self.free.pop()
                    elif self.hw < self.cap:
                        r, self.hw = self.hw, self.hw + 1
                    else:
                        r, self.dropped = -2, self.dropped + 1
                    self.row_of[b][s] = r
                    if r >= 0:
                        rows[n_new], decs[n_new] = r, i
                        pars[n_new] = -1 if src[i] < 0 else self.prev[src[i]]
                        edges[n_new] = -1 if src[i] < 0 else tok[i]
                        n_new += 1
                ro[i] = max(self.row_of[b][s], -1)
        self.prev = ro
        return [ro, rows, pars, edges, decs, np.asarray([n_new, self.hw, len(self.free), self.dropped], np.int32)]

    def release(self, ids_per_stream):
        for b, ids in enumerate(ids_per_stream):
            for i in ids:
                r = self.row_of[b].pop(int(i), -1)
                if r >= 0:
                    self.free.append(r)


def plan_and_check(sess, dec, pm, lists, what=""):
    """dec.plan(lists) against pm.plan of the same lists -> (the plan, the model's outputs, the lists on the host)"""
    if is_gpu(sess):
        dec.ctx.synchronize()
    host = [_np(a).copy().reshape(-1) for a in lists]
    p = dec.plan(*lists)
    if is_gpu(sess):
        dec.ctx.synchronize()
    want = pm.plan(*host)
    for name, w in zip(NAMES, want):
        g = _np(getattr(p, name))
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        assert g.tolist() == w.tolist(), (what, name, g.tolist(), w.tolist())
    return p, want, host


class Store:
    """The caller's LM-row store, [cap, W]: written at new_row from the prefix the parent row and the edge name"""

    def __init__(self, sess, cap, W, lm_row, K):
        self.sess, self.lm_row, self.K = sess, lm_row, K
        self.rows = _dev(sess, np.full((cap, W), np.nan, np.float32))
        self.prefix = {}  # row -> (utterance, the edges since the start)
        self.asked = []

    def fill(self, want):
        """the model's outputs of a plan (equal to the device's) -> [(dec_row, prefix)] of the new states"""
        _, rows, pars, edges, decs, counts = want
        out = []
        for i in range(int(counts[0])):
            b = int(decs[i]) // self.K
            if pars[i] < 0:
                pre = ()
            else:
                assert self.prefix[int(pars[i])][0] == b, "a parent row of another utterance"
                pre = self.prefix[int(pars[i])][1] + (int(edges[i]),)
            self.prefix[int(rows[i])] = (b, pre)
            self.asked.append((b, pre))
            row = np.asarray(self.lm_row(b, pre), np.float32)
            if is_gpu(self.sess):
                import torch
                self.rows[int(rows[i])] = torch.from_numpy(row).cuda()
            else:
                self.rows[int(rows[i])] = row
            out.append((int(decs[i]), pre))
        return out


def planned_decode(sess, dec, ems, N, W, lm_row, cap, extra_steps=1, lister=None, words=False):
    """C0.decode's loop with the planner in the place of the host bookkeeping.  -> (final, rows per frame per utterance,
    the prefix of every state id per utterance, the PlanModel, every plan's model outputs)"""
    B, K = len(ems), int(dec.options.beam_size)
    Ts = [e.shape[0] for e in ems]
    flat = np.concatenate([e.reshape(-1) for e in ems]) if sum(Ts) else np.zeros(0, np.float32)
    lists = dec.begin(flat, Ts, N)
    dec.plan_begin(cap)
    pm = PlanModel(B, K, min(K * max(Ts) + 2, dec._max_states), cap)
    store = Store(sess, cap, W, lm_row, K)
    prefix, rows, plans = [dict() for _ in range(B)], [[] for _ in range(B)], []
    for t in range(max(Ts) + extra_steps + 1):
        p, want, (tok_h, src_h, st_h, n_h) = plan_and_check(sess, dec, pm, lists, t)
        plans.append(want)
        for dec_row, pre in store.fill(want):
            sid = int(st_h[dec_row])
            assert prefix[dec_row // K].setdefault(sid, pre) == pre, (t, dec_row, "one id, two states")
        if lister is not None:  # the host bookkeeping fed the same lists assigns the same rows
            _, ro = lister.rows(*lists)
            assert _np(ro).tolist() == want[0].tolist(), t
        for b in range(B):
            if 0 < t <= Ts[b]:
                rows[b].append([(int(src_h[b * K + k]) - b * K, int(tok_h[b * K + k]), int(st_h[b * K + k]))
                                for k in range(int(n_h[b]))])
        if t == max(Ts) + extra_steps:
            dec.end(store.rows, lm_row_of=p.lm_row_of)
        else:
            lists = dec.step(store.rows, lm_row_of=p.lm_row_of)
    final = []
    for b in range(B):
        hs = dec.results(b)
        final.append([(h.score, h.am, h.lm, h.tokens.tolist()) + ((h.words.tolist(),) if words else ()) for h in hs])
    return final, rows, prefix, pm, plans


def rows_lm(sess, rl, perm=True):
    return _capi.RowsLM(rl.W, rl.usr_to_lm if perm else None, rl.finish, lib=sess.lib)


# ---- 1. row numbers against the model, decodes against the fixtures and the restatement ------------------------------------
@pytest.mark.parametrize("c", C0._golden(), ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(c, sess):
    st = Stats()
    _, want_rows = C0._case_restate(c, st)
    assert not st.ties and (not c["log_add"] or st.gap > MIN_GAP)
    rl = G.case_lm(c)
    lm = rows_lm(sess, rl, c["perm"])
    dec = make_dec(sess, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["sil_score"], c["sil"], c["blank"], c["log_add"])
    got, rows, prefix, pm, _ = planned_decode(sess, dec, [G.emissions(c["seed"], c["T"], c["N"])], c["N"], rl.W,
                                              lambda b, p: rl.row(list(p)), c["K"] * c["T"] + 2)
    assert_final(c["hyps"], got[0], c["log_add"], c["name"])
    assert_rows(want_rows, rows[0], prefix[0])
    assert pm.dropped == 0 and pm.hw == len(prefix[0])
    dec.close()
    lm.close()


def seeded_batch(base, Ts, N, K, Kt, W, perm, thr, lmw, sil_score, sil, blank, log_add, scale=1.0):
    """C0.batch's cases: per utterance the first tie-free seed -> [(seed, inputs, (final, rows), stats)], [the LMs]"""
    found = []
    for b, T in enumerate(Ts):
        def case_fn(seed, T=T):
            rl = G.SmRowsLM(seed ^ 0x5A5A, N, W, perm, W - 1, 0)
            lm = PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
            return (G.emissions(seed, T, N) * np.float32(scale), lm, K, Kt, thr, lmw, sil_score, sil, blank, log_add)
        found.append(C0.clean(case_fn, base + 1000 * b, log_add))
    return found, [G.SmRowsLM(seed ^ 0x5A5A, N, W, perm, W - 1, 0) for seed, _, _, _ in found]


@pytest.mark.parametrize("log_add", [False, True])
def test_batch_of_unequal_lengths_and_the_host_lister(sess, log_add):
    """B = 3 with T = (10, 0, 6), N = 3, K = 8: states merge and are entered again; every plan equals the model, the
    new states' parent rows and edges name the restatement's prefixes, the n-best is the restatement's -- and
    _RowLister, fed the same lists, assigns the same rows."""
    N, K, W = 3, 8, 5
    found, rls = seeded_batch(100, (10, 0, 6), N, K, 3, W, 31, 25.0, 0.7, 0.0, 1, 0, log_add, scale=0.25)
    lm = _capi.RowsLM(W, rls[0].usr_to_lm, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, 3, 25.0, 0.7, 0.0, 1, 0, log_add)
    lister = _capi._RowLister(dec, 3, K, lambda keys: _dev(sess, np.stack([rls[b].row(list(p)) for b, p in keys])))
    got, rows, prefix, pm, plans = planned_decode(sess, dec, [inp[0] for _, inp, _, _ in found], N, W,
                                                  lambda b, p: rls[b].row(list(p)), 3 * (K * 10 + 2), lister=lister)
    for b, (_, _, (want, want_rows), _) in enumerate(found):
        assert_final(want, got[b], log_add, b)
        assert_rows(want_rows, rows[b], prefix[b])
    assert found[0][3].merges >= 1 and found[0][3].reentered >= 1
    assert pm.hw == sum(len(p) for p in prefix) == lister.n_store and pm.dropped == 0
    assert plans[0][5].tolist() == [3, 3, 0, 0]  # the three roots
    dec.close()
    lm.close()


# ---- 2. a hand-written list: one new state on two rows, an id outside the table ---------------------------------------------
def test_hand_written_list_with_a_pair_and_an_id_out_of_range(sess):
    """After a real begin (B = 2, K = 4; the table holds K * max T + 2 = 14 ids): the list's rows 1 and 3 of utterance 0
    carry the same new state 5 -- listed once, from row 1, both rows name its row; ids 14, -3 and 2^30 read -1, are not
    listed and nothing is written for them; the guard words around every output stay."""
    N, K, W, B = 4, 4, 5, 2
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    ems = [G.emissions(77 + b, 3, N) for b in range(B)]
    lists = dec.begin(np.concatenate([e.reshape(-1) for e in ems]), [3, 3], N)
    dec.plan_begin(6)
    pm = PlanModel(B, K, 14, 6)
    p, _, _ = plan_and_check(sess, dec, pm, lists, "roots")
    dec.step(_dev(sess, np.zeros((6, W), np.float32)), lm_row_of=p.lm_row_of)  # (a list can be planned once)
    tok = np.asarray([[-1, 2, 3, 3], [2, 3, 1, -1]], np.int32)
    src = np.asarray([[0, 0, 0, 0], [4, 4, 4, -1]], np.int32)
    state = np.asarray([[0, 5, 14, 5], [-3, 1 << 30, 13, -1]], np.int32)
    n = np.asarray([4, 3], np.int32)
    want = pm.plan(tok.reshape(-1), src.reshape(-1), state.reshape(-1), n)
    assert want[0].tolist() == [0, 2, -1, 2, -1, -1, 3, -1] and want[5].tolist() == [2, 4, 0, 0]
    assert want[1][:3].tolist() == [2, 3, -1] and want[4][:2].tolist() == [1, 6]  # listed once, from the lower k
    assert want[2][:2].tolist() == [0, 1] and want[3][:2].tolist() == [2, 1]
    # the same call on buffers with guard words on both sides of every output
    G0, BK = 8, B * K
    bufs = [np.full(BK + 2 * G0, 77, np.int32) for _ in range(5)] + [np.full(4 + 2 * G0, 77, np.int32)]
    devs = [_dev(sess, b) for b in bufs]
    ins = [_dev(sess, a) for a in (tok, src, state, n)]
    rc = sess.lib.lib.fltx_ctc_rows_plan(dec.h, *[dec._addr(a) for a in ins], *[dec._addr(d) + 4 * G0 for d in devs])
    assert rc == 0, sess.lib.lib.fltx_last_error()
    dec.ctx.synchronize()
    for name, d, w in zip(NAMES, devs, want):
        g = _np(d)
        assert (g[:G0] == 77).all() and (g[-G0:] == 77).all(), name
        assert g[G0:-G0].tolist() == w.tolist(), (name, g[G0:-G0].tolist(), w.tolist())
    dec.close()
    lm.close()


# ---- 3. the sums over more utterances than a wave; a full workgroup of rows -----------------------------------------------
@pytest.mark.parametrize("B,K,N,T", [(70, 2, 3, 3), (1, 256, 6, 6), (300, 1, 3, 2)])
def test_many_utterances_and_a_full_workgroup(sess, B, K, N, T):
    """B = 70 (and 300: more counts than the workgroup has threads), K = 2: the sums cross waves; B = 1, K = 256, T = 6: a
    thread per row, four waves of rows.  Every plan against the model."""
    W = N + 1
    rl = G.SmRowsLM(5, N, W, 0, W - 1, 0)
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 1e9, 0.7, 0.0, 0, 1, False)
    ems = [G.emissions(3000 + b, T - (b % 3 == 2), N) for b in range(B)]
    got, rows, prefix, pm, plans = planned_decode(sess, dec, ems, N, W, lambda b, p: rl.row(list(p[-2:])), B * (K * T + 2))
    assert all(got) and pm.dropped == 0 and pm.hw == sum(len(p) for p in prefix)
    assert max(int(w[5][0]) for w in plans) > 64  # the new states of one plan: their ranks cross a wave
    if K == 256:
        assert max(len(r) for r in rows[0]) == 256
    dec.close()
    lm.close()


# ---- 4. a store smaller than the states ---------------------------------------------------------------------------------
def test_row_capacity_smaller_than_the_states(sess):
    N, K, W, B, T, cap = 4, 8, 5, 2, 8, 9
    rl = G.SmRowsLM(9, N, W, 0, W - 1, 0)
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 1e9, 0.7, 0.0, 0, 1, False)
    ems = [G.emissions(4100 + b, T, N) * np.float32(0.25) for b in range(B)]
    got, rows, prefix, pm, plans = planned_decode(sess, dec, ems, N, W, lambda b, p: rl.row(list(p)), cap)
    dropped = [{s for s, r in pm.row_of[b].items() if r == -2} for b in range(B)]
    print("dropped states:", dropped, "high water", pm.hw)
    assert pm.dropped == sum(len(d) for d in dropped) > 0 and pm.hw == cap
    first_drop = min(t for t, w in enumerate(plans) if w[5][3] > 0)
    for t, w in enumerate(plans):
        assert all(int(x.max()) < cap for x in w[:3]), t  # no row >= row_capacity anywhere
        assert w[5][3] == 0 or w[5][1] == cap
    for b in range(B):  # a dropped state reads -1 in every list that carries it, and is never listed
        for t, frame in enumerate(rows[b]):
            for k, (_, _, sid) in enumerate(frame):
                if sid in dropped[b]:
                    assert t + 1 >= first_drop and plans[t + 1][0][b * K + k] == -1
                    assert b * K + k not in plans[t + 1][4][:int(plans[t + 1][5][0])].tolist()
        assert not dropped[b] & set(prefix[b])
    assert all(len(g) >= 1 for g in got)  # the decode ended without an error status
    # the helper on the same inputs says so
    store = _dev(sess, np.zeros((cap, W), np.float32))
    with pytest.raises(RuntimeError, match="LM row store full"):
        dec.decode_device(np.concatenate([e.reshape(-1) for e in ems]), [T] * B, N, store, lambda p, n_new: None)
    dec.close()
    lm.close()


# ---- 5. streams with recycling --------------------------------------------------------------------------------------------
class PlannedStreams(R.RecyclingStreams):
    """RecyclingStreams stepped with the planner's rows: every list is planned and held to the PlanModel, the new
    states' (parent row, edge) must name the prefix the tracker has for the id, a collect goes on to plan_release"""

    def __init__(self, sess, dec, B, N, W, lm_row, max_frames, cap, lexicon=False):
        self.cap, self.pm, self.store, self.p, self.high = cap, None, None, None, 0
        self._W, self._lm_row = W, lm_row
        R.RecyclingStreams.__init__(self, sess, dec, B, N, W, lm_row, max_frames, lexicon)

    def _take(self, out, stepped, first=False):
        R.RecyclingStreams._take(self, out, stepped, first)
        if first:
            self.dec.plan_begin(self.cap)
            self.pm = PlanModel(self.B, self.K, self.dec._stream_states, self.cap)
            self.store = Store(self.sess, self.cap, self._W, self._lm_row, self.K)
        self.p, want, host = plan_and_check(self.sess, self.dec, self.pm, out)
        for dec_row, pre in self.store.fill(want):
            assert self.prefix[dec_row // self.K][int(host[2][dec_row])] == pre, dec_row
        self.high = int(want[5][1])

    def chunk(self, parts, extra_steps=0):
        Ts = [p.shape[0] for p in parts]
        flat = np.concatenate([p.reshape(-1) for p in parts]) if sum(Ts) else np.zeros(0, np.float32)
        for t in range(self.dec.append(flat, Ts) + extra_steps):
            self._take(self.dec.step(self.store.rows, lm_row_of=self.p.lm_row_of), [t < T for T in Ts])

    def end(self):
        self.dec.end(self.store.rows, lm_row_of=self.p.lm_row_of)
        return [[self._hyp(h) for h in self.dec.results(b)] for b in range(self.B)]

    def collect(self, cap=None):
        inner, kept = self.dec.collect, []

        def spy(*a):
            kept.append(inner(*a))
            return kept[0]
        self.dec.collect = spy
        try:
            ids = R.RecyclingStreams.collect(self, cap)
        finally:
            del self.dec.collect
        self.dec.plan_release(kept[0][0], kept[0][1])
        self.pm.release(ids)
        return ids


def run_planned_streams(ds, c, every):
    """R.run_recycling's loop with a collect after every `every`-th chunk -> (bests per stream, final per stream)"""
    B = len(c["ems"])
    at, bests = [0] * B, [[] for _ in range(B)]
    for i, cut in enumerate(c["cuts"]):
        ds.chunk([c["ems"][b][at[b]:at[b] + cut[b]] for b in range(B)])
        at = [a + x for a, x in zip(at, cut)]
        ds.dec.prune(c["lb"])
        if i % every == every - 1:
            ds.collect()
        for b in range(B):
            bests[b].append(ds.best(b, 0))
    return bests, ds.end()


def sparse_profile(c, every):
    """R.table_profile of the restatement's lists when only every `every`-th chunk collects"""
    return [R.table_profile(c["want"][b][3], R.collect_points(c["cuts"], b)[every - 1::every])
            for b in range(len(c["ems"]))]


@pytest.mark.parametrize("log_add", [False, True])
def test_long_streams_reuse_their_rows(sess, log_add):
    """The 300 / 150 / 80-frame streams of the recycle tests (chunks of unequal length, prune(2)) in tables of 64 ids
    and a store of 3 * 64 rows, a collect and plan_release after every second chunk: rows equal the model's after every
    plan, the streams decide what the restatement decides, and the store's high-water mark stays far below the states
    ever entered."""
    c = R.long_case(log_add)
    prof = sparse_profile(c, 2)
    print("states ever / peak table / most released per stream:", prof)
    ever = sum(p[0] for p in prof)
    assert all(p[1] <= 64 for p in prof) and ever > 3 * 64, "the model alone must show that rows are reused"
    lm, dec = R.case_dec(sess, c, 64)
    ds = PlannedStreams(sess, dec, 3, c["N"], c["W"], lambda b, p: R.last3(c["rl"])(p), 32, 3 * 64)
    bests, final = run_planned_streams(ds, c, 2)
    R.assert_against_restatement(c, bests, final, ds)
    assert sum(ds.ever) == ever and ds.high == ds.pm.hw <= sum(p[1] for p in prof) < ever and ds.pm.dropped == 0
    assert len(ds.store.asked) == ever  # the LM was asked once per hand-out
    dec.close()
    lm.close()


# ---- 6. contract and refusals -----------------------------------------------------------------------------------------------
def test_contract_and_refusals(sess):
    L, ctx = sess.lib, sess.ctx
    I, S = _capi.ERR_INVALID, _capi.ERR_STATE
    N, K = 6, 4
    lm = _capi.RowsLM(N + 1, None, N, lib=L)
    dec = make_dec(sess, lm, K, N, 25.0, 0.5, 0.0, 0, 1, False)
    dec.B = 1
    lists = dec._rows()
    po = [dec._addr(o) for o in lists]
    outs = [_dev(sess, np.zeros(K, np.int32)) for _ in range(6)]
    pp = [dec._addr(o) for o in outs]
    rel = [_dev(sess, np.zeros(8, np.int32)) for _ in range(3)]
    pr, pn, pl = [dec._addr(x) for x in rel]
    em = G.emissions(900, 6, N)
    T3 = np.asarray([3], np.int32)
    lr = _dev(sess, np.zeros((64, N + 1), np.float32))
    plr = dec._addr(lr)
    begin, plan, release = L.lib.fltx_ctc_rows_plan_begin, L.lib.fltx_ctc_rows_plan, L.lib.fltx_ctc_rows_plan_release

    def step(ro=None):
        return L.lib.fltx_ctc_rows_step(dec.h, plr, 0, 0, N + 1, ro, 64 if ro else 0, 1, None, *po)

    def end(ro=None):
        return L.lib.fltx_ctc_rows_end(dec.h, plr, 0, 0, N + 1, ro, 64 if ro else 0, 1, None)
    # outside a begun decode
    assert begin(dec.h, 8) == S and plan(dec.h, *po, *pp) == S and release(dec.h, pr, pn, 8) == S
    assert begin(None, 8) == I and plan(None, *po, *pp) == I and release(None, pr, pn, 8) == I
    # a decoder that never calls plan_begin steps as before (and plan / release stay refused on it)
    assert L.lib.fltx_ctc_rows_begin(dec.h, em.ctypes.data, 0, None, T3.ctypes.data, 1, N, *po) == 0
    assert plan(dec.h, *po, *pp) == S and "fltx_ctc_rows_plan_begin" in L.lib.fltx_last_error().decode()
    for _ in range(3):
        assert step() == 0
    assert end() == 0
    plain = [(h.score, h.tokens.tolist()) for h in dec.results(0)]
    assert plain and begin(dec.h, 8) == S  # the decode has ended
    # a batch decode with the planner: the arguments, the order of the calls
    assert L.lib.fltx_ctc_rows_begin(dec.h, em.ctypes.data, 0, None, T3.ctypes.data, 1, N, *po) == 0
    assert begin(dec.h, 0) == I and begin(dec.h, -4) == I and plan(dec.h, *po, *pp) == S
    assert begin(dec.h, 64) == 0
    for i in range(4):
        assert plan(dec.h, *(po[:i] + [None] + po[i + 1:]), *pp) == I
    for i in range(6):
        assert plan(dec.h, *po, *(pp[:i] + [None] + pp[i + 1:])) == I
    assert release(dec.h, pr, pn, 8) == S  # not a stream
    assert plan(dec.h, *po, *pp) == 0
    assert plan(dec.h, *po, *pp) == S and "planned already" in L.lib.fltx_last_error().decode()
    assert step(pp[0]) == 0 and plan(dec.h, *po, *pp) == 0
    assert step(pp[0]) == 0 and plan(dec.h, *po, *pp) == 0
    assert step(pp[0]) == 0 and plan(dec.h, *po, *pp) == 0
    assert end(pp[0]) == 0
    assert [(h.score, h.tokens.tolist()) for h in dec.results(0)] == plain  # (a zero LM: the rows do not matter)
    assert plan(dec.h, *po, *pp) == S
    # two steps without a plan in between: refused until the next plan_begin; the steps themselves go on
    assert L.lib.fltx_ctc_rows_begin(dec.h, em.ctypes.data, 0, None, T3.ctypes.data, 1, N, *po) == 0
    assert plan(dec.h, *po, *pp) == S  # a begin ends planning
    assert begin(dec.h, 64) == 0 and plan(dec.h, *po, *pp) == 0
    assert step(pp[0]) == 0 and step() == 0
    assert plan(dec.h, *po, *pp) == S and "never planned" in L.lib.fltx_last_error().decode()
    assert step() == 0 and plan(dec.h, *po, *pp) == S
    assert begin(dec.h, 64) == 0 and plan(dec.h, *po, *pp) == 0 and end(pp[0]) == 0
    # a stream: a collect must be followed by plan_release before the next plan
    assert L.lib.fltx_ctc_rows_stream_begin(dec.h, 1, N, 8, *po) == 0
    assert release(dec.h, pr, pn, 8) == S  # no plan_begin yet
    assert begin(dec.h, 64) == 0 and plan(dec.h, *po, *pp) == 0
    assert L.lib.fltx_ctc_rows_stream_append(dec.h, em.ctypes.data, 0, None, T3.ctypes.data) == 0
    assert step(pp[0]) == 0
    assert L.lib.fltx_ctc_rows_stream_collect(dec.h, 8, pr, pn, pl) == 0
    assert plan(dec.h, *po, *pp) == S and "fltx_ctc_rows_plan_release" in L.lib.fltx_last_error().decode()
    assert release(dec.h, None, pn, 8) == I and release(dec.h, pr, None, 8) == I and release(dec.h, pr, pn, 0) == I
    assert release(dec.h, pr, pn, 8) == 0 and plan(dec.h, *po, *pp) == 0
    assert step(pp[0]) == 0 and plan(dec.h, *po, *pp) == 0 and step(pp[0]) == 0 and plan(dec.h, *po, *pp) == 0
    assert end(pp[0]) == 0
    assert [(h.score, h.tokens.tolist()) for h in dec.results(0)] == plain
    assert release(dec.h, pr, pn, 8) == S  # the stream is over
    # the other kinds
    other = _capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(K, N, lm_weight=0.5), sess.zero, 0, 1)
    s2s = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, 4), sess.zero, 1, 5)
    s2s.begin(1, 5)
    for o in (other, s2s):
        assert begin(o.h, 8) == S and plan(o.h, *po, *pp) == S and release(o.h, pr, pn, 8) == S
        o.close()
    dec.close()
    lm.close()


# ---- 7. the Python helpers ---------------------------------------------------------------------------------------------------
class HostLmNew:
    """lm_new for the tests: reads the plan's lists on the host, keeps the prefix of every row, writes the store"""

    def __init__(self, sess, store, K, lm_row):
        self.sess, self.store, self.K, self.lm_row = sess, store, K, lm_row
        self.prefix, self.asked = {}, []

    def __call__(self, p, n_new):
        rows, pars, edges, decs = [_np(a)[:n_new].tolist() for a in (p.new_row, p.new_parent_row, p.new_edge, p.new_dec_row)]
        out = []
        for r, par, e, d in zip(rows, pars, edges, decs):
            pre = () if par < 0 else self.prefix[par] + (e,)
            self.prefix[r] = pre
            self.asked.append((d // self.K, pre))
            out.append(np.asarray(self.lm_row(d // self.K, pre), np.float32))
        if is_gpu(self.sess):
            import torch
            self.store[torch.as_tensor(rows, device=self.store.device)] = torch.from_numpy(np.stack(out)).cuda()
        else:
            self.store[np.asarray(rows)] = np.stack(out)


def hyps(res):
    return [[(h.score, h.am, h.lm, list(h.tokens)) for h in hs] for hs in res]


def test_decode_device_equals_decode(sess):
    N, K, W, sil, blank, Ts = 4, 6, 5, 0, 1, (6, 0, 4)
    rl = G.SmRowsLM(21, N, W, 0, W - 1, 0)
    lm = _capi.RowsLM(W, None, W - 1, lib=sess.lib)
    dec = make_dec(sess, lm, K, N, 25.0, 0.7, 0.0, sil, blank, True)
    ems = [G.emissions(950 + b, T, N) * np.float32(0.25) for b, T in enumerate(Ts)]
    flat = np.concatenate([e.reshape(-1) for e in ems])
    asked = []

    def lm_rows(keys):
        asked.extend(keys)
        return _dev(sess, np.stack([rl.row(list(p)) for _, p in keys]))
    want = hyps(dec.decode(flat, Ts, N, lm_rows))
    store = _dev(sess, np.full((3 * (K * 6 + 2), W + 2), np.nan, np.float32))  # (rows wider than the LM's)
    lm_new = HostLmNew(sess, store, K, lambda b, p: np.concatenate([rl.row(list(p)), [0, 0]]))
    got = hyps(dec.decode_device(flat, Ts, N, store, lm_new))
    assert got == want and all(want[b] for b in (0, 2))
    assert lm_new.asked == asked and len(set(asked)) == len(asked)  # every (utterance, state), once, in the same order
    dec.close()
    lm.close()


def test_decode_stream_device_equals_decode_stream(sess):
    c = R.long_case(False, Ts=(120, 80), base=1900)
    B, N, W, K = 2, c["N"], c["W"], c["K"]
    chunks, at = [], [0, 0]
    for cut in c["cuts"]:
        chunks.append((np.concatenate([c["ems"][b][at[b]:at[b] + cut[b]].reshape(-1) for b in range(B)]), list(cut)))
        at = [a + x for a, x in zip(at, cut)]
    asked = []

    def lm_rows(keys):
        asked.extend(keys)
        return _dev(sess, np.stack([R.last3(c["rl"])(p) for _, p in keys]))

    def flatten(outs):
        res = [[(h.score, h.am, h.lm, h.tokens.tolist()) for h in o] for o in outs[:-1]]
        return res + [hyps(outs[-1])]
    lm, dec = R.case_dec(sess, c, R.MAX_STATES)
    want = flatten(list(dec.decode_stream(chunks, lm_rows, look_back=c["lb"], N=N, max_frames=32, collect_every=1)))
    store = _dev(sess, np.full((2 * R.MAX_STATES, W), np.nan, np.float32))
    lm_new = HostLmNew(sess, store, K, lambda b, p: R.last3(c["rl"])(p))
    got = flatten(list(dec.decode_stream_device(chunks, store, lm_new, look_back=c["lb"], N=N, max_frames=32,
                                                collect_every=1)))
    assert got == want
    for b in range(B):
        assert_final(c["want"][b][2], got[-1][b], False, b)
    assert lm_new.asked == asked and len(asked) > 2 * R.MAX_STATES  # once per hand-out: more asks than rows
    dec.close()
    lm.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_CTC_ROWS_PLAN_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
