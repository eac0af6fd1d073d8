"""Fixtures of the lexicon CTC rows decoder's streams (tests/golden/lex_ctc_lm_rows_stream_expected.json.gz) from the
reference itself.

Dev container only: compiles the unmodified LexiconDecoder.cpp, Utils.cpp and Trie.cpp of the reference tree (default
/root/reference, or $FLTX_REFERENCE) with lex_ctc_lm_rows_stream_ref_driver.cpp into oracle/_ref/ (kept out of history).
A case is B streams under one list of operations, as make_ctc_lm_rows_stream_golden.py describes them; the reference
decodes every stream on its own, twice under different heap layouts (the two runs must agree).  Recorded per stream: every
best hypothesis with its words (null: an empty result), nDecodedFramesInBuffer after each prune, and the final n-best.
LM, lexicons and emissions are make_lex_ctc_lm_rows_golden.py's; `hold` forces stretches of frames onto one token (the
driver's header says how).  A stream's seed is the first from its base on whose search the float64 restatement of
tests/test_lexicon_ctc_lm_rows_stream.py sees no tie (and, under logAdd, no decision closer than 1e-3) and which shows
what the case is there for (`need`: "extended" -- a best or prune call whose walk went on from look_back to the last word
end; "limited" -- one that look_back + 100 steps ended).  No case is dropped.  The generator asserts that the restatement
reproduces the driver.  No reference source text is copied.

    python tests/golden/make_lex_ctc_lm_rows_stream_golden.py
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_lex_ctc_lm_rows_golden as GL  # noqa: E402
from make_ctc_lm_rows_golden import emissions as _emissions  # noqa: E402
from make_ctc_lm_rows_stream_golden import stream_script  # noqa: E402

OUT = os.path.join(HERE, "lex_ctc_lm_rows_stream_expected.json.gz")
INF = float("inf")

LEX = dict(GL.LEX)
# N = 4 (letters 2 and 3): after 2, 3 the trie node has a child and no label -- a hypothesis held there is inside a word
LEX["n4"] = [(0, -0.5, [2, 3, 2]), (1, -1.0, [3, 2]), (2, -0.75, [2, 2])]


def _rep(n, *ops):
    return [op for _ in range(n) for op in ops]


# (name, Ts, N, K, Kt, thr, lmw, word_score, unk_score, sil_score, sil, blank, log_add, lex, n_map, W, perm, is_lm_token,
#  max_frames, hold, need, ops)
CASES = [
    # best(lb) mid-stream for lb = 0, 1 and more than the buffered frames (empty, and LexiconDecoder.cpp:286); an empty
    # chunk; prune with too few frames
    ("word_chunks_best", [9, 7, 5], 6, 4, 6, 25.0, 0.7, 0.0, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, 0, 12, "-", "",
     [("c", [3, 2, 0]), ("b", 0), ("b", 1), ("b", 99), ("c", [4, 0, 3]), ("b", 0), ("b", 1), ("p", 99),
      ("c", [2, 5, 2]), ("b", 2), ("b", 4)]),
    ("tok_prune", [12, 8], 6, 8, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "b", 6, 7, 0, 1, 12,  "-", "",
     [("c", [5, 1]), ("p", 2), ("b", 0), ("b", 1), ("c", [2, 4]), ("b", 1), ("p", 0), ("c", [5, 3]), ("b", 0), ("p", 2),
      ("b", 1)]),
    # the best ancestor at look_back sits inside a word: the walk goes on to the last word end
    ("word_inside_word", [14], 6, 6, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "long", 5, 6, 0, 0, 14, "-", "extended",
     [("c", [5]), ("b", 1), ("p", 1), ("b", 0), ("c", [4]), ("b", 2), ("p", 2), ("b", 0), ("b", 1), ("c", [5]), ("b", 1),
      ("p", 0), ("b", 0)]),
    ("word_logadd_unk", [10, 6], 6, 8, 5, 25.0, 0.7, 0.25, -0.75, -0.2, 0, 1, True, "a", 7, 9, 84, 0, 10, "-", "",
     [("c", [4, 1]), ("b", 1), ("p", 2), ("c", [3, 5]), ("b", 0), ("p", 1), ("b", 0), ("c", [3, 0]), ("b", 2)]),
    # a non-final letter held for more than 104 frames: look_back + 100 steps end the walk, inside the word; the ring of
    # 8 + 100 + 2 rows wraps (the one long case)
    ("word_hold_limit", [115], 4, 2, 4, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "n4", 3, 4, 0, 0, 8, "0:1:2/1:115:3",
     "limited", _rep(23, ("c", [5]), ("p", 2), ("b", 2))),
]
FIELDS = ["name", "Ts", "N", "K", "Kt", "thr", "lmw", "word_score", "unk_score", "sil_score", "sil", "blank", "log_add",
          "lexname", "n_map", "W", "perm", "is_lm_token", "max_frames", "hold", "need", "ops"]


def all_cases():
    out = []
    for spec in CASES:
        c = dict(zip(FIELDS, spec))
        c["ops"] = [list(o) for o in c["ops"]]
        c["lex"] = [[lab, sc, list(toks)] for lab, sc, toks in LEX[c["lexname"]]]
        tok = c["is_lm_token"]
        c["unk"] = (c["n_map"] - 1) if (not tok and c["unk_score"] > -INF) else (1 + max(w[0] for w in c["lex"]))
        if tok:
            c["n_map"] = c["N"]
        out.append(c)
    return out


def emissions(c, b, seed=None):
    """[T, N] float32 of stream b: the driver's emissions, its holds applied"""
    em = _emissions(c["seeds"][b] if seed is None else seed, c["Ts"][b], c["N"])
    if c["hold"] != "-":
        for part in c["hold"].split("/"):
            t0, t1, tok = map(int, part.split(":"))
            for t in range(t0, t1):
                keep = em[t] - np.float32(8.0)
                keep[tok] = np.float32(0.0)
                em[t] = keep
    return em


def case_lm(c, b, seed=None):
    return GL.SmRowsLM((c["seeds"][b] if seed is None else seed) ^ 0xABCDEF, c["n_map"], c["W"], c["perm"], c["W"] - 1, 0)


def build_driver(ref):
    d = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(d, exist_ok=True)
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "lex_ctc_lm_rows_stream_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref,
                    os.path.join(HERE, "lex_ctc_lm_rows_stream_ref_driver.cpp"), os.path.join(dec, "LexiconDecoder.cpp"),
                    os.path.join(dec, "Utils.cpp"), os.path.join(dec, "Trie.cpp"), "-o", exe], check=True)
    return exe


def parse(out):
    """the driver's lines -> dict(best, frames, final); a hypothesis is [score, am, lm, tokens, words]"""
    res = dict(best=[], frames=[], final=[])
    for line in out.strip().splitlines():
        if line.startswith("P"):
            res["frames"].append(int(line.split()[1]))
            continue
        h = None
        if len(line.split()) > 1:
            a, w = line[1:].split("|")
            f = a.split()
            h = [float(f[0]), float(f[1]), float(f[2]), [int(x) for x in f[3:]], [int(x) for x in w.split()]]
        res["best" if line[0] == "B" else "final"].append(h)
    return res


def run_driver(exe, c, b, seed, lexpath, junk):
    num = GL._num
    script = ",".join("%s%d" % (op, v) for op, v in stream_script(c, b))
    args = [exe, str(seed), str(c["Ts"][b]), str(c["N"]), str(c["K"]), str(c["Kt"]), num(c["thr"]), num(c["lmw"]),
            num(c["word_score"]), num(c["unk_score"]), num(c["sil_score"]), str(c["sil"]), str(c["blank"]),
            str(c["unk"]), str(int(c["log_add"])), str(c["is_lm_token"]), lexpath, str(seed ^ 0xABCDEF), str(c["W"]),
            str(c["perm"]), str(c["W"] - 1), str(c["n_map"]), "0" if c["is_lm_token"] else "1", str(junk), c["hold"], script]
    return parse(subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout)


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_lexicon_ctc_lm_rows_stream as T
    exe = build_driver(os.environ.get("FLTX_REFERENCE", "/root/reference"))
    out = []
    with tempfile.TemporaryDirectory() as d:
        for c in all_cases():
            lexpath = os.path.join(d, c["name"] + ".lex")
            with open(lexpath, "w") as f:
                for lab, sc, toks in c["lex"]:
                    f.write("%d %s %s\n" % (lab, repr(sc), " ".join(map(str, toks))))
            c["seeds"], c["streams"] = [], []
            for b in range(len(c["Ts"])):
                base = 3000 * (len(out) + 1) + 100 * b
                c["seeds"].append(base)
                while True:
                    st = T.Stats()
                    bests, frames, final, _ = T.case_restate(c, b, st)
                    if not st.ties and (not c["log_add"] or st.gap > T.MIN_GAP) and T.shows(c["need"], st):
                        break
                    c["seeds"][b] += 1
                    assert c["seeds"][b] < base + 3000, (c["name"], st.ties[:3])
                a = run_driver(exe, c, b, c["seeds"][b], lexpath, 0)
                assert a == run_driver(exe, c, b, c["seeds"][b], lexpath, 4096), c["name"]
                c["streams"].append(a)
                T.assert_case(c, b, (bests, frames, final), (c["name"], b))
                print(c["name"], b, "seed", c["seeds"][b], "final", len(a["final"]), "merges", st.merges, "gap", st.gap,
                      "frames", a["frames"], "empty bests", sum(1 for h in a["best"] if h is None), "extended",
                      getattr(st, "extended", 0), "limited", getattr(st, "limited", 0),
                      "words", sum(1 for h in a["final"] for w in h[4] if w >= 0))
            out.append(c)
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
