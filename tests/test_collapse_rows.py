"""fltx_collapse_rows (text_amd/csrc/fltx_transcript.h): the count, scan and write kernels on rows chosen where the walk
can go wrong -- tile seams, odd row starts, rows and row counts around the tile and the scan chunk -- held by exact
integer equality to `restate` below, the rule of include/fltx.h written out in NumPy-free Python (not imported from the
package).

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

CHILD = os.environ.get("FLTX_COLLAPSE_ROWS_GPU_CHILD") == "1"
if CHILD:
    import torch
    torch.cuda.init()

from text_amd import _capi  # noqa: E402
from test_seq2seq_model_output import _GpuSess, is_gpu  # noqa: E402

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)] if CHILD else ["emu"]
TILE = 64    # entries per step of a wave's walk
SCAN = 256   # the scan kernel's single workgroup (kTrScanThreads) ...
CHUNK = 2048  # ... and the rows it takes per step, eight per thread (kTrScanChunk): the carry crosses here
JUNK = 7777  # what lies between the rows: a kernel that reads past a row's end or start would keep it
BLANK = 3
KEYS = ("tokens", "timesteps", "words", "word_timesteps", "word_tok_end")


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


# ---- the rule --------------------------------------------------------------------------------------------------------------
def restate(tok, wrd, blank):
    """-> (tokens, timesteps, words, word_timesteps, word_tok_end) of one row"""
    toks, ts, ws, wts, wte = [], [], [], [], []
    for i in range(len(tok)):
        if tok[i] >= 0 and tok[i] != blank and (i == 0 or tok[i] != tok[i - 1]):
            toks.append(int(tok[i]))
            ts.append(i)
        if wrd is not None and wrd[i] >= 0:
            ws.append(int(wrd[i]))
            wts.append(i)
            wte.append(len(toks))
    return toks, ts, ws, wts, wte


def lay_out(rows, wrows):
    """The rows in one flat buffer with JUNK between them: every start odd, the starts mutually unaligned (gaps of one to
    eight entries).  -> (tokens, words or None, row_off int64, row_len int32)"""
    off, at = [], 1
    for i, r in enumerate(rows):
        off.append(at)
        at = (at + len(r) + 1 + 2 * (i % 4)) | 1
    tok = np.full(at + 1, JUNK, np.int32)
    wrd = None if wrows is None else np.full(at + 1, JUNK, np.int32)
    for o, r in zip(off, rows):
        tok[o:o + len(r)] = r
    if wrows is not None:
        for o, r in zip(off, wrows):
            wrd[o:o + len(r)] = r
    return tok, wrd, np.asarray(off, np.int64), np.asarray([len(r) for r in rows], np.int32)


def expected(rows, wrows, blank):
    """the restatement of every row, concatenated -> (dict of the five arrays, tok_off, word_off, rows read)"""
    cat = {k: [] for k in KEYS}
    tok_off, word_off = [0], [0]
    for i, r in enumerate(rows):
        res = restate(list(r), None if wrows is None else list(wrows[i]), blank)
        for k, v in zip(KEYS, res):
            cat[k] += v
        tok_off.append(len(cat["tokens"]))
        word_off.append(len(cat["words"]))
    return cat, tok_off, word_off


def assert_result(got, rows, wrows, blank):
    want, tok_off, word_off = expected(rows, wrows, blank)
    assert got["n_rows"] == len(rows)
    assert got["tok_off"].dtype == np.int64 and got["word_off"].dtype == np.int64
    assert got["tok_off"].tolist() == tok_off and got["word_off"].tolist() == word_off
    assert got["n_tokens"] == tok_off[-1] and got["n_words"] == word_off[-1]
    for k in KEYS:
        assert got[k].dtype == np.int32 and got[k].tolist() == want[k], k
    return want


def collapse(sess, rows, wrows, blank=BLANK):
    tok, wrd, off, ln = lay_out(rows, wrows)
    got = sess.ctx.collapse_rows(tok, wrd, off, ln, blank)
    return assert_result(got, rows, wrows, blank)


def rand_row(rng, n, p_repeat=0.6, alphabet=(BLANK, 0, 1, 2)):
    r = np.empty(n, np.int32)
    for i in range(n):
        r[i] = r[i - 1] if i and rng.random() < p_repeat else alphabet[rng.integers(len(alphabet))]
    return r


def rand_words(rng, n, p=0.15):
    return np.where(rng.random(n) < p, rng.integers(0, 1000, n), -1).astype(np.int32)


# ---- 1. lengths around the tile -------------------------------------------------------------------------------------------
def test_lengths_around_the_tile_at_odd_starts(sess):
    """0, 1, 2, 63, 64, 65, 127, 128, 129 and 200 entries in one call, every row at an odd offset of its own"""
    rng = np.random.default_rng(11)
    lens = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]
    rows = [rand_row(rng, n) for n in lens]
    wrows = [rand_words(rng, n) for n in lens]
    off = lay_out(rows, wrows)[2]
    assert all(o % 2 == 1 for o in off) and len({int(o) % 16 for o in off}) > 4
    want = collapse(sess, rows, wrows)
    assert 0 < len(want["tokens"]) < sum(lens) and len(want["words"]) > 0


# ---- 2. tile seams ----------------------------------------------------------------------------------------------------------
def seam_row(at62, at63, at64, n=130, fill=(0, 1)):
    """a row that alternates 0 1 0 1 ... (every position kept) except at 62, 63, 64"""
    r = np.asarray([fill[i % 2] for i in range(n)], np.int32)
    r[62], r[63], r[64] = at62, at63, at64
    return r


def test_tile_seams(sess):
    x = 2
    rows = [seam_row(0, x, x),        # equal at 63 and 64: once
            seam_row(0, x, 1),        # different at 63 and 64: twice
            seam_row(x, BLANK, x),    # x blank x: two x
            seam_row(0, -1, -1),      # the same three with -1 for the blank / the repeat
            seam_row(x, -1, x),
            seam_row(-1, x, x),
            np.full(200, x, np.int32)]  # one run over three tiles (and a fourth, partial one)
    rows[6][:5] = [0, 1, 0, 1, 0]
    rows[6][195:] = [1, 0, 1, 0, 1]
    want, tok_off, _ = expected(rows, None, BLANK)
    per_row = [list(zip(want["tokens"][a:b], want["timesteps"][a:b])) for a, b in zip(tok_off, tok_off[1:])]
    # what the restatement must say about the seams, spelled out
    assert [p for p in per_row[0] if p[0] == x] == [(x, 63)]
    assert (x, 63) in per_row[1] and (1, 64) in per_row[1]
    assert [p for p in per_row[2] if p[0] == x] == [(x, 62), (x, 64)]
    assert all(t not in (63, 64) for _, t in per_row[3])
    assert [p for p in per_row[4] if p[0] == x] == [(x, 62), (x, 64)]
    assert [p for p in per_row[5] if p[0] == x] == [(x, 63)]
    assert [p for p in per_row[6] if p[0] == x] == [(x, 5)]
    collapse(sess, rows, None)
    # ... and with the rows shifted by one entry, so that the seam falls on other lanes
    collapse(sess, [np.concatenate([[1], r]).astype(np.int32) for r in rows], None)


# ---- 3. degenerate rows -----------------------------------------------------------------------------------------------------
def test_degenerate_rows(sess):
    rows = [np.full(150, BLANK, np.int32), np.full(150, 5, np.int32), np.full(150, -1, np.int32),
            np.asarray([0, 0, 65535, 65535, 0, BLANK, 65535] * 20, np.int32)]
    want = collapse(sess, rows, None)
    assert want["tokens"][:1] == [5] and want["timesteps"][:1] == [0] and 65535 in want["tokens"] and 0 in want["tokens"]
    w2 = collapse(sess, rows, None, blank=-1)  # nothing is a blank
    assert w2["tokens"][:2] == [BLANK, 5] and len(w2["tokens"]) > len(want["tokens"])
    # only empty rows, and rows with nothing to keep: empty arrays
    for rs in ([np.zeros(0, np.int32)] * 3, [np.full(70, -1, np.int32)] * 2):
        tok, wrd, off, ln = lay_out(rs, None)
        got = sess.ctx.collapse_rows(tok, None, off, ln, BLANK)
        assert got["tokens"].size == 0 and got["words"].size == 0 and got["tok_off"].tolist() == [0] * (len(rs) + 1)


# ---- 4. words ----------------------------------------------------------------------------------------------------------------
def test_words(sess):
    rng = np.random.default_rng(5)
    n = 131
    row = rand_row(rng, n)
    row[40:44] = [1, BLANK, BLANK, 2]
    w = np.full(n, -1, np.int32)
    for i, wid in ((0, 10), (63, 11), (64, 12), (n - 1, 13), (20, 14), (21, 15), (41, 16)):  # (41: a dropped position)
        w[i] = wid
    rows, wrows = [row, row[:64].copy(), row.copy()], [w, w[:64].copy(), np.full(n, -1, np.int32)]
    want = collapse(sess, rows, wrows)
    first = restate(list(row), list(w), BLANK)
    assert first[2] == [10, 14, 15, 16, 11, 12, 13] and first[3] == [0, 20, 21, 41, 63, 64, n - 1]
    # word_tok_end by its definition: the kept positions <= the word's
    assert first[4] == [sum(1 for t in first[1] if t <= i) for i in first[3]]
    assert first[4][3] == sum(1 for t in first[1] if t <= 40)  # (the word on the blank ends what was kept before it)
    assert want["words"][:7] == first[2]
    # words = NULL: the same tokens, no words, word_off all 0
    tok, _, off, ln = lay_out(rows, wrows)
    got = sess.ctx.collapse_rows(tok, None, off, ln, BLANK)
    assert got["tokens"].tolist() == want["tokens"] and got["words"].size == 0
    assert got["word_off"].tolist() == [0] * 4 and got["word_off"].dtype == np.int64


# ---- 5. row counts: the scan's chunks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [0, 1, 4, 5, SCAN + 1, 2 * SCAN + 3, CHUNK + 1, 2 * CHUNK + 3])
def test_row_counts(sess, n_rows):
    """lengths 0 .. 3, so that the offsets -- the scan kernel's chunk carry -- are what is tested"""
    rng = np.random.default_rng(100 + n_rows)
    lens = rng.integers(0, 4, n_rows)
    rows = [rand_row(rng, int(n), 0.3) for n in lens]
    wrows = [rand_words(rng, int(n), 0.5) for n in lens]
    want = collapse(sess, rows, wrows)
    if n_rows > SCAN:
        assert len(want["tokens"]) > n_rows // 2 and len(want["words"]) > n_rows // 4


# ---- 6. random rows ---------------------------------------------------------------------------------------------------------
def test_random_rows(sess):
    rng = np.random.default_rng(2024)
    lens = rng.integers(1, 301, 200)
    rows = [rand_row(rng, int(n)) for n in lens]
    wrows = [rand_words(rng, int(n)) for n in lens]
    want = collapse(sess, rows, wrows)
    assert 0 < len(want["tokens"]) < int(lens.sum()), "a vacuous input"
    assert 0 < len(want["words"]) < int(lens.sum())


# ---- 7. results left on the device ---------------------------------------------------------------------------------------------
def read_device(sess, addr, n, dtype):
    """n elements at a device address -> a NumPy array"""
    out = np.zeros(n, dtype)
    if n == 0:
        return out
    if not is_gpu(sess):  # the emulator's "device" memory is host memory
        C.memmove(out.ctypes.data, addr, out.nbytes)
        return out
    hip = C.CDLL("libamdhip64.so.7")  # (the runtime libfltx.so is linked against: already mapped)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    sess.ctx.synchronize()
    assert hip.hipMemcpy(out.ctypes.data, addr, out.nbytes, 2) == 0  # (synchronous D2H)
    return out


def test_device_results_are_the_host_results(sess):
    rng = np.random.default_rng(77)
    lens = [0, 65, 3, 129, 64, 1]
    rows = [rand_row(rng, n) for n in lens]
    wrows = [rand_words(rng, n, 0.3) for n in lens]
    tok, wrd, off, ln = lay_out(rows, wrows)
    d = sess.ctx.collapse_rows(tok, wrd, off, ln, BLANK, device=True)
    assert all(isinstance(d[k], int) for k in KEYS + ("tok_off", "word_off"))
    nt, nw, n = d["n_tokens"], d["n_words"], d["n_rows"]
    got = {"n_rows": n, "n_tokens": nt, "n_words": nw,
           "tok_off": read_device(sess, d["tok_off"], n + 1, np.int64),
           "word_off": read_device(sess, d["word_off"], n + 1, np.int64)}
    for k in KEYS:
        got[k] = read_device(sess, d[k], nt if k in ("tokens", "timesteps") else nw, np.int32)
    want = assert_result(got, rows, wrows, BLANK)
    assert len(want["tokens"]) > 0 and len(want["words"]) > 0
    # all four inputs by device address: n_rows says how many rows
    if is_gpu(sess):
        import torch
        held = [torch.from_numpy(x).cuda() for x in (tok, wrd, off, ln)]
        torch.cuda.current_stream().synchronize()
        at = [x.data_ptr() for x in held]
    else:
        at = [x.ctypes.data for x in (tok, wrd, off, ln)]
    assert_result(sess.ctx.collapse_rows(*at, BLANK, n_rows=len(rows)), rows, wrows, BLANK)
    with pytest.raises(TypeError):
        sess.ctx.collapse_rows(*at, BLANK)  # (row_len by address, no n_rows)


# ---- 8. the buffers grow and are used again ---------------------------------------------------------------------------------------
def test_more_rows_then_fewer_and_no_second_allocation(sess):
    rng = np.random.default_rng(9)
    small = [rand_row(rng, n) for n in (5, 70)]
    big = [rand_row(rng, int(n)) for n in rng.integers(1, 200, 40)]
    wsmall = [rand_words(rng, len(r)) for r in small]
    wbig = [rand_words(rng, len(r), 0.4) for r in big]
    collapse(sess, small, wsmall)
    collapse(sess, big, wbig)
    tok, wrd, off, ln = lay_out(small, wsmall)
    got = sess.ctx.collapse_rows(tok, wrd, off, ln, BLANK)
    assert_result(got, small, wsmall, BLANK)
    where = [got[k].ctypes.data for k in KEYS + ("tok_off",)]
    tok, wrd, off, ln = lay_out(big, wbig)
    again = sess.ctx.collapse_rows(tok, wrd, off, ln, BLANK)
    assert_result(again, big, wbig, BLANK)
    assert [again[k].ctypes.data for k in KEYS + ("tok_off",)] == where, "a call the buffers already hold allocated again"


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_negative_length_and_bad_arguments_are_refused(sess):
    rows = [np.asarray([0, 1, 1], np.int32), np.asarray([2], np.int32), np.asarray([1, 1], np.int32)]
    tok, _, off, ln = lay_out(rows, None)
    bad = ln.copy()
    bad[1] = -1
    with pytest.raises(ValueError) as e:
        sess.ctx.collapse_rows(tok, None, off, bad, BLANK)
    assert "negative" in str(e.value)
    L = sess.lib.lib
    t = _capi.Transcripts()
    assert L.fltx_collapse_rows(sess.ctx.h, None, None, None, None, -1, BLANK, 0, C.byref(t)) == _capi.ERR_INVALID
    assert L.fltx_collapse_rows(sess.ctx.h, None, None, None, None, 0, BLANK, 0, None) == _capi.ERR_INVALID
    assert L.fltx_collapse_rows(None, None, None, None, None, 0, BLANK, 0, C.byref(t)) == _capi.ERR_INVALID
    assert L.fltx_collapse_rows(sess.ctx.h, None, None, None, None, 0, BLANK, 0, C.byref(t)) == 0 and t.n_rows == 0
    collapse(sess, rows, None)  # and the context decodes on


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def _gpu_cases_in_a_fresh_process():
    """Every `gpu` case of this module, on the HIP library, in a child process that initialises torch first."""
    import subprocess
    env = dict(os.environ, FLTX_COLLAPSE_ROWS_GPU_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-2000:]


if not CHILD:
    test_gpu_cases_in_a_fresh_process = _gpu_cases_in_a_fresh_process
