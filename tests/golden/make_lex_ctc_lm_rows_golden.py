"""Fixtures of the lexicon CTC rows decoder (tests/golden/lex_ctc_lm_rows_expected.json.gz) from the reference itself.

Dev container only: compiles the unmodified LexiconDecoder.cpp, Utils.cpp and Trie.cpp of the reference tree (default
/root/reference, or $FLTX_REFERENCE) with lex_ctc_lm_rows_ref_driver.cpp into oracle/_ref/ (kept out of history), and
runs every case twice under different heap layouts (the two runs must agree).  The LM scores a whole vocabulary per state
(make_s2s_lm_rows_golden.SmRowsLM: a splitmix64 function of (seed, prefix, LM index), exact in float32; its state is the
prefix of words, or of tokens with is_lm_token); the emissions are make_ctc_lm_rows_golden.emissions.  A case's seed is
the first from its base on whose search the float64 restatement of tests/test_lexicon_ctc_lm_rows.py sees no tie (and,
under logAdd, no decision closer than 1e-3) and on which the case shows what it is there for (`need`) in its final
n-best: the restatement with that rule broken (tests' MUTATIONS) gives another n-best, so the reference's output pins
the rule; every case of seven frames or more has a word in its n-best.  No case is dropped.  The generator asserts that the restatement reproduces the driver: tokens and words exact, scores bit-equal
under max-merge and within 1e-5 under logAdd.  No reference source text is copied.

    python tests/golden/make_lex_ctc_lm_rows_golden.py
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_ctc_lm_rows_golden import emissions  # noqa: E402,F401
from make_s2s_lm_rows_golden import SmRowsLM  # noqa: E402

OUT = os.path.join(HERE, "lex_ctc_lm_rows_expected.json.gz")
INF = float("inf")

# tokens: 0 sil, 1 blank, 2.. letters.  (label, score, spelling); unk is the id after the last word
LEX = {
    # a one-token word (0), a word that is a prefix of another (0 < 1), a node with two labels (2, 3); b alone is no word
    "a": [(0, -0.5, [2]), (1, -1.25, [2, 3]), (2, -0.75, [3, 2]), (3, -2.0, [3, 2]), (4, -1.5, [4, 5, 2]), (5, -0.25, [5])],
    # the same without the second label (a token LM gives both labels of a node one score: a tie by construction)
    "b": [(0, -0.5, [2]), (1, -1.25, [2, 3]), (2, -0.75, [3, 2]), (4, -1.5, [4, 5, 2]), (5, -0.25, [5])],
    # long words only: a short utterance ends inside a word
    "long": [(0, -0.5, [2, 3, 4]), (1, -1.0, [3, 4, 5]), (2, -0.75, [4, 2, 3]), (3, -1.5, [5, 5, 2]), (4, -0.25, [2, 4, 5])],
    # doubled letters: at node [2], token 2 again cannot move (no blank in between) but does end the word [2, 2]
    "dd": [(0, -0.5, [2]), (1, -1.25, [2, 2]), (2, -0.75, [3, 2]), (3, -1.0, [3, 3]), (4, -0.25, [5])],
    # three letters
    "n5": [(0, -0.5, [2]), (1, -1.0, [2, 3]), (2, -0.75, [3, 4]), (3, -1.5, [4])],
}

# (name, T, N, K, Kt, thr, lmw, word_score, unk_score, sil_score, sil, blank, log_add, lex, n_words, W, perm, need)
WORD = [
    ("t1_k1", 1, 6, 1, 6, 25.0, 0.7, 0.0, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, ""),
    ("root_guard", 8, 6, 8, 6, 25.0, 0.7, 0.0, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, "guard"),
    ("repeat_end", 8, 6, 8, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "dd", 5, 6, 0, "repeat_end"),
    ("two_labels", 7, 6, 8, 6, 25.0, 0.7, 0.0, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, "both_labels"),
    ("prefix_word", 8, 6, 8, 6, 25.0, 0.7, 0.0, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, "label_and_kids"),
    ("kt3_outside", 8, 6, 8, 3, 25.0, 0.7, 0.0, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, "outside"),
    ("tight_thr", 12, 6, 8, 6, 1.5, 0.7, 0.0, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, "tight_thr"),
    ("sil_word_score", 12, 6, 8, 6, 25.0, 0.7, 0.75, -INF, -0.4, 0, 1, False, "a", 6, 7, 0, "scores"),
    ("lmw0", 12, 6, 8, 6, 25.0, 0.0, 0.25, -INF, 0.0, 0, 1, False, "a", 6, 7, 0, ""),
    ("unk", 8, 6, 8, 6, 25.0, 0.7, 0.25, -0.5, 0.0, 0, 1, False, "a", 7, 8, 0, "unk"),
    ("no_root_end", 2, 6, 2, 6, 1.0, 0.7, 0.0, -INF, 0.0, 0, 1, False, "long", 5, 6, 0, "no_root_end"),
    ("smear_n5", 10, 5, 6, 4, 25.0, 1.25, 0.5, -INF, -0.25, 0, 1, False, "n5", 4, 5, 0, "smear"),
    ("perm_wide", 12, 6, 8, 5, 25.0, 0.7, 0.25, -0.75, 0.3, 0, 1, False, "a", 7, 13, 83, ""),
    ("logadd", 10, 6, 8, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, True, "a", 6, 7, 0, "merges"),
    ("logadd_perm_thr", 7, 6, 4, 6, 3.0, 0.7, 0.0, -1.0, -0.2, 0, 1, True, "a", 7, 9, 84, "merges"),
]
# (word_score != 0 throughout: a token LM gives the move to a node and the word end at it one LM entry, so at
# word_score 0 the two tie by construction)
TOKEN = [
    ("t1_k1", 1, 6, 1, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "b", 6, 7, 0, ""),
    ("root_guard", 8, 6, 8, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "b", 6, 7, 0, "guard"),
    ("repeat_end", 8, 6, 8, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "dd", 6, 7, 0, "repeat_end"),
    ("prefix_word", 8, 6, 8, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "b", 6, 7, 0, "label_and_kids"),
    ("kt3_outside", 8, 6, 8, 3, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "b", 6, 7, 0, "outside"),
    ("tight_thr", 12, 6, 8, 6, 1.5, 0.7, 0.25, -INF, 0.0, 0, 1, False, "b", 6, 7, 0, "tight_thr"),
    ("sil_word_score", 12, 6, 8, 6, 25.0, 0.7, 0.75, -INF, -0.4, 0, 1, False, "b", 6, 7, 0, "scores"),
    ("lmw0", 12, 6, 8, 6, 25.0, 0.0, 0.25, -INF, 0.0, 0, 1, False, "b", 6, 7, 0, ""),
    ("unk", 8, 6, 8, 6, 25.0, 0.7, 0.25, -0.5, 0.0, 0, 1, False, "b", 6, 7, 0, "unk"),
    ("no_root_end", 2, 6, 2, 6, 1.0, 0.7, 0.25, -INF, 0.0, 0, 1, False, "long", 6, 7, 0, "no_root_end"),
    ("perm_wide", 12, 6, 8, 5, 25.0, 0.7, 0.25, -0.75, 0.3, 0, 1, False, "b", 6, 13, 83, ""),
    ("logadd", 10, 6, 8, 6, 25.0, 0.7, 0.25, -INF, 0.0, 0, 1, True, "b", 6, 7, 0, "merges"),
    ("logadd_perm_thr", 7, 6, 4, 6, 3.0, 0.7, 0.5, -1.0, -0.2, 0, 1, True, "b", 6, 9, 84, "merges"),
]
FIELDS = ["name", "T", "N", "K", "Kt", "thr", "lmw", "word_score", "unk_score", "sil_score", "sil", "blank", "log_add",
          "lexname", "n_map", "W", "perm", "need"]


def all_cases():
    """the cases without seeds and results: n_map is the LM map's length -- the words (unk, the last id, included when it
    is on) under the word LM, N under the token LM"""
    out = []
    for tok, specs in ((0, WORD), (1, TOKEN)):
        for spec in specs:
            c = dict(zip(FIELDS, spec))
            c["is_lm_token"] = tok
            if c["T"] >= 7:  # (long enough for a word: one must be in the n-best)
                c["need"] = ",".join(filter(None, [c["need"], "words"]))
            c["name"] = ("tok_" if tok else "word_") + c["name"]
            c["lex"] = [[lab, sc, list(toks)] for lab, sc, toks in LEX[c["lexname"]]]
            c["unk"] = (c["n_map"] - 1) if (not tok and c["unk_score"] > -INF) else (1 + max(w[0] for w in c["lex"]))
            if tok:
                c["n_map"] = c["N"]
            out.append(c)
    return out


def case_lm(c, seed=None):
    """the rows LM of a case: .usr_to_lm maps words (tokens with is_lm_token), .finish is the last LM index"""
    return SmRowsLM((c["seed"] if seed is None else seed) ^ 0xABCDEF, c["n_map"], c["W"], c["perm"], c["W"] - 1, 0)


def build_driver(ref):
    d = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(d, exist_ok=True)
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "lex_ctc_lm_rows_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref,
                    os.path.join(HERE, "lex_ctc_lm_rows_ref_driver.cpp"), os.path.join(dec, "LexiconDecoder.cpp"),
                    os.path.join(dec, "Utils.cpp"), os.path.join(dec, "Trie.cpp"), "-o", exe], check=True)
    return exe


def _num(x):
    return "-inf" if x == -INF else repr(x)


def run_driver(exe, c, seed, lexpath, junk):
    args = [exe, str(seed), str(c["T"]), str(c["N"]), str(c["K"]), str(c["Kt"]), _num(c["thr"]), _num(c["lmw"]),
            _num(c["word_score"]), _num(c["unk_score"]), _num(c["sil_score"]), str(c["sil"]), str(c["blank"]),
            str(c["unk"]), str(int(c["log_add"])), str(c["is_lm_token"]), lexpath, str(seed ^ 0xABCDEF), str(c["W"]),
            str(c["perm"]), str(c["W"] - 1), str(c["n_map"]), "0" if c["is_lm_token"] else "1", str(junk)]
    out = subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout
    hyps = []
    for line in out.strip().splitlines():
        a, b = line.split("|")
        f = a.split()
        hyps.append([float(f[0]), float(f[1]), float(f[2]), [int(x) for x in f[3:]], [int(x) for x in b.split()]])
    return hyps


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_lexicon_ctc_lm_rows as T
    exe = build_driver(os.environ.get("FLTX_REFERENCE", "/root/reference"))
    out = []
    with tempfile.TemporaryDirectory() as d:
        for c in all_cases():
            lexpath = os.path.join(d, c["name"] + ".lex")
            with open(lexpath, "w") as f:
                for lab, sc, toks in c["lex"]:
                    f.write("%d %s %s\n" % (lab, repr(sc), " ".join(map(str, toks))))
            seed = 1000 * (len(out) + 1)
            while True:
                st = T.Stats()
                got, _ = T.case_restate(c, st, seed)
                if not st.ties and (not c["log_add"] or st.gap > T.MIN_GAP) and \
                        T.shows(c["need"], st, got, lambda ch: T.case_restate(c, T.Stats(), seed, ch)[0]):
                    break
                seed += 1
                assert seed < 1000 * (len(out) + 1) + 5000, c["name"]
            a = run_driver(exe, c, seed, lexpath, 0)
            b = run_driver(exe, c, seed, lexpath, 4096)
            assert a == b, c["name"]
            T.assert_final(a, got, c["log_add"], c["name"])
            c["seed"] = seed
            c["hyps"] = a
            out.append(c)
            print(c["name"], "seed", seed, "hyps", len(a), "merges", st.merges, "reentered", st.reentered, "gap", st.gap)
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
