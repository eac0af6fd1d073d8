"""The LM rows of the lexicon CTC rows decoder planned on the device (fltx_ctc_rows_plan_*): tests/test_ctc_rows_plan.py's
model and loops on the lexicon kind, with a word LM and with a token LM -- the reference fixtures, a new state that two
rows of one list carry, and the recycled streams of tests/test_lexicon_ctc_lm_rows_recycle.py.

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

CHILD = os.environ.get("FLTX_LEX_CTC_ROWS_PLAN_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

import test_ctc_lm_rows_recycle as R0  # noqa: E402
import test_ctc_rows_plan as P0  # noqa: E402
import test_lexicon_ctc_lm_rows as L0  # noqa: E402
import test_lexicon_ctc_lm_rows_recycle as LR  # noqa: E402
from golden import make_lex_ctc_lm_rows_golden as G  # noqa: E402
from test_ctc_lm_rows import MIN_GAP, PrefixLM, Stats  # noqa: E402
from test_lexicon_ctc_lm_rows import SMEAR_MAX, Lex, assert_final, assert_rows, dev_lm, make_dec, opts  # noqa: E402
from test_seq2seq_model_output import _GpuSess  # noqa: E402

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


# ---- 1. the reference fixtures, word LM and token LM ----------------------------------------------------------------------
def test_the_fixtures_have_both_lms():
    assert {c["is_lm_token"] for c in L0._golden()} == {0, 1}


@pytest.mark.parametrize("c", L0._golden(), ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(c, sess):
    """every plan equals the model; the new states' parent rows and edges (words or tokens) name the restatement's
    prefixes; the n-best, words included, is the fixture's"""
    o = L0.case_opts(c)
    rl = G.case_lm(c)
    lx = Lex(sess.lib, c["N"], c["sil"], c["lex"], 0 if c["is_lm_token"] else SMEAR_MAX)
    st = Stats()  # (the restatement's trie through the session's own library: a GPU machine has no emulator library)
    _, want_rows = L0.restate(G.emissions(c["seed"], c["T"], c["N"]), lx.nodes,
                              PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish), o, st=st)
    assert not st.ties and (not c["log_add"] or st.gap > MIN_GAP)
    lm = dev_lm(sess, rl, o, mapped=bool(c["perm"]))
    dec = make_dec(sess, lx, lm, o)
    got, rows, prefix, pm, _ = P0.planned_decode(sess, dec, [G.emissions(c["seed"], c["T"], c["N"])], c["N"], rl.W,
                                                 lambda b, p: rl.row(list(p)), c["K"] * c["T"] + 2, words=True)
    assert_final(c["hyps"], got[0], c["log_add"], c["name"])
    assert_rows(want_rows, rows[0], prefix[0])
    assert pm.dropped == 0 and pm.hw == len(prefix[0])
    for d in (dec, lm, lx):
        d.close()


# ---- 2. one new state on two rows of one list ------------------------------------------------------------------------------
PAIR_LEX = [(0, -0.5, [2, 3]), (0, -0.75, [2, 4]), (1, -0.25, [3]), (2, -0.5, [4, 2]), (3, -1.0, [5])]  # word 0: 2 3 / 2 4


def new_pairs(rows):
    """[(frame, state, its rows)] of the states that a list carries on two rows or more and no earlier list carried"""
    seen, out = {()}, []
    for t, frame in enumerate(rows):
        states = [s for _, _, s in frame]
        for s in sorted(set(states) - seen):
            ks = [k for k, x in enumerate(states) if x == s]
            if len(ks) >= 2:
                out.append((t, s, ks))
        seen.update(states)
    return out


def test_one_word_ended_through_two_last_tokens(sess):
    """Word 0 is spelled 2 3 and 2 4: under the word LM a hypothesis inside it can end it through either token in one
    frame, and both candidates -- equal in LM state and node, different in token -- stay in the beam.  The state is
    listed once, from the lower row, and both rows name its row."""
    N, K, W, T, seed = 6, 8, 6, 6, 500
    o = opts(K, N, 25.0, 0.7, 0.25, is_lm_token=False)
    lx = Lex(sess.lib, N, 0, PAIR_LEX)
    rl = G.SmRowsLM(seed ^ 0x5A5A, 4, W, 0, W - 1, 0)
    em = G.emissions(seed, T, N) * np.float32(0.25)
    st = Stats()
    want, want_rows = L0.restate(em, lx.nodes, PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish), o, st=st)
    pairs = new_pairs(want_rows)
    assert not st.ties and pairs, "the seed must show a new state on two rows of one list"
    assert any(len({want_rows[t][k][1] for k in ks}) == 1 and want_rows[t][ks[0]][1] == 0 for t, _, ks in pairs)
    lm = dev_lm(sess, rl, o, mapped=False)
    dec = make_dec(sess, lx, lm, o)
    got, rows, prefix, pm, plans = P0.planned_decode(sess, dec, [em], N, W, lambda b, p: rl.row(list(p)), K * T + 2,
                                                     words=True)
    assert_final(want, got[0], False)
    assert_rows(want_rows, rows[0], prefix[0])
    for t, s, ks in pairs:  # (frame t's list is plan t + 1; the plans were held to the model already)
        ro, new_row, _, _, dec_row, counts = plans[t + 1]
        listed = [i for i in range(int(counts[0])) if int(dec_row[i]) in ks]
        assert [int(dec_row[i]) for i in listed] == [ks[0]], (t, s, ks)
        assert {int(ro[k]) for k in ks} == {int(new_row[listed[0]])}, (t, s, ks)
    for d in (dec, lm, lx):
        d.close()


# ---- 5. streams with recycling --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokl", [False, True], ids=["word_lm", "token_lm"])
def test_lexicon_streams_reuse_their_rows(sess, tokl):
    """The 200 / 120-frame lexicon streams of the recycle tests in tables of 32 ids and a store of 2 * 32 rows, prune(2),
    a collect and plan_release after every chunk: rows equal the model's after every plan, bests and n-best (words
    included) are the restatement's, the high-water mark stays below the states ever entered."""
    c = LR.lex_case(sess, tokl, False)
    ever = sum(p[0] for p in c["prof"])
    assert all(p[1] <= LR.MAX_STATES for p in c["prof"]) and ever > 2 * LR.MAX_STATES, \
        "the model alone must show that rows are reused"
    lx = Lex(sess.lib, LR.N, 0, c["lex"], 0 if tokl else SMEAR_MAX)
    lm = dev_lm(sess, c["rl"], c["o"])
    dec = make_dec(sess, lx, lm, c["o"])
    dec.set_max_states(LR.MAX_STATES)
    ds = P0.PlannedStreams(sess, dec, 2, LR.N, LR.W, lambda b, p: R0.last3(c["rl"])(p), 32, 2 * LR.MAX_STATES, lexicon=True)
    bests, final = P0.run_planned_streams(ds, dict(c, lb=LR.LB), 1)
    R0.assert_against_restatement(c, bests, final, ds, final_check=assert_final)
    assert sum(ds.ever) == ever == len(ds.store.asked)
    assert ds.high == ds.pm.hw <= sum(p[1] for p in c["prof"]) < ever and ds.pm.dropped == 0
    for d in (dec, lm, lx):
        d.close()


# ---- 6. the calls on this kind ------------------------------------------------------------------------------------------
def test_decode_device_on_the_lexicon_kind(sess):
    """decode_device returns decode's n-best bit for bit, words included, and asks about every state once"""
    N, K, W, Ts = 6, 8, 6, (6, 0, 4)
    o = opts(K, N, 25.0, 0.7, 0.25, is_lm_token=False)
    lx = Lex(sess.lib, N, 0, PAIR_LEX)
    rl = G.SmRowsLM(500 ^ 0x5A5A, 4, W, 0, W - 1, 0)
    lm = dev_lm(sess, rl, o, mapped=False)
    dec = make_dec(sess, lx, lm, o)
    ems = [G.emissions(500 + b, T, N) * np.float32(0.25) for b, T in enumerate(Ts)]
    flat = np.concatenate([e.reshape(-1) for e in ems])
    asked = []

    def lm_rows(keys):
        asked.extend((b, p) for b, p, _, _, _ in keys)
        return P0._dev(sess, np.stack([rl.row(list(p)) for _, p, _, _, _ in keys]))

    def hyps(res):
        return [[(h.score, h.am, h.lm, list(h.tokens), list(h.words)) for h in hs] for hs in res]
    want = hyps(dec.decode(flat, Ts, N, lm_rows))
    store = P0._dev(sess, np.full((3 * (K * 6 + 2), W), np.nan, np.float32))
    lm_new = P0.HostLmNew(sess, store, K, lambda b, p: rl.row(list(p)))
    got = hyps(dec.decode_device(flat, Ts, N, store, lm_new))
    assert got == want and want[0] and want[2] and any(w >= 0 for h in want[0] for w in h[4])
    assert lm_new.asked == asked and len(set(asked)) == len(asked)
    for d in (dec, lm, lx):
        d.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_LEX_CTC_ROWS_PLAN_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
