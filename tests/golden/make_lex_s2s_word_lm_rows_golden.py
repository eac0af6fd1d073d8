"""Fixtures of the lexicon seq2seq decoder with a word-level rows LM
(tests/golden/lexicon_seq2seq_word_lm_rows_expected.json.gz) from the reference itself.

Dev container only: compiles the unmodified LexiconSeq2SeqDecoder.cpp, Trie.cpp and Utils.cpp of the reference tree
(default /root/reference, or $FLTX_REFERENCE) with lex_s2s_word_lm_rows_ref_driver.cpp into a temporary directory, and
runs every case twice under different heap layouts (the two runs must agree).  The decoder runs with isLmToken = false
on a trie smeared with MAX over non-zero word scores; the LM scores its whole word vocabulary per state
(make_s2s_lm_rows_golden.SmRowsLM over the word ids) and its state is the WORD prefix: a child per word, finish a child
(-1) of its own -- make_lex_s2s_lm_rows_golden.PrefixObjLM names the states the same way for the float64 restatement of
tests/test_lexicon_seq2seq.py (restate_lex with is_lm_token=False), whose merges then are the reference's.  The
discipline is make_lex_s2s_lm_rows_golden.py's: a case's seed is the first from its base on whose search the restatement
sees no tie; a case that must show merges needs the restatement to count some; the homophone case needs two final
hypotheses with the same tokens and different words (both labels of a node survived); a case with -inf LM entries needs
one to have been read and the restatement to reproduce the driver; the case that must end at max_output_length needs an
unfinished hypothesis in the result.  No case is dropped.  The generator asserts that the restatement reproduces the
driver.  No reference source text is copied.

    python tests/golden/make_lex_s2s_word_lm_rows_golden.py
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
import make_lex_s2s_lm_rows_golden as G  # noqa: E402
from make_s2s_lm_rows_golden import SmRowsLM  # noqa: E402

OUT = os.path.join(HERE, "lexicon_seq2seq_word_lm_rows_expected.json.gz")
SMEAR_MAX = 1

# (name, V, K, Kt, thr, lmw, word_score, eos_score, eos, maxlen, eos_bias, drop, log_add,
#  lexicon (n_words, seed, max_len, homophones, respell, single), W, perm, finish, inf_mod, min_merges, unfinished,
#  both_labels)
CASES = [
    ("merge_max", 10, 16, 10, 1e9, 0.6, 0.2, 0.0, 9, 7, 0.5, 0.0, False, (30, 31, 3, 0.0, 0.4, 0.4), 31, 0, 30, 0, 1, 0,
     0),
    ("merge_logadd", 10, 16, 10, 1e9, 0.6, 0.2, 0.0, 9, 7, 0.5, 0.0, True, (30, 31, 3, 0.0, 0.4, 0.4), 31, 0, 30, 0, 1, 0,
     0),
    ("homophones", 11, 16, 11, 1e9, 0.5, 0.3, -0.1, 10, 7, 0.5, 0.0, False, (36, 7, 3, 0.3, 0.3, 0.4), 37, 0, 36, 0, 0, 0,
     1),
    ("perm_wide_finish", 12, 8, 8, 1e9, 0.7, 0.3, -0.2, 11, 7, 0.6, 0.0, False, (40, 5, 3, 0.1, 0.3, 0.3), 57, 77, 19, 0,
     0, 0, 0),
    ("dropped_rows_logadd", 9, 24, 9, 1e9, 0.3, 0.4, 0.0, 0, 8, 0.4, 0.1, True, (30, 12, 3, 0.1, 0.5, 0.3), 35, 78, 33,
     0, 1, 0, 0),
    ("lmw0", 10, 8, 6, 25.0, 0.0, 0.2, 0.0, 9, 6, 0.5, 0.0, False, (30, 31, 3, 0.0, 0.3, 0.4), 31, 0, 30, 0, 0, 0, 0),
    ("lmw0_inf", 10, 8, 8, 25.0, 0.0, 0.2, 0.0, 9, 6, 0.5, 0.0, False, (30, 31, 3, 0.0, 0.3, 0.4), 31, 0, 30, 3, 0, 0, 0),
    ("maxlen_unfinished", 12, 8, 12, 1e9, 0.5, 0.3, 0.0, 11, 6, -2.0, 0.0, False, (40, 5, 4, 0.1, 0.2, 0.3), 41, 0, 40,
     0, 0, 1, 0),
]
FIELDS = G.FIELDS + ["both_labels"]


def lexicon(c):
    return G.lexicon(c)


def n_words(c):
    return int(c["lex"][0])


def case_lm(c, seed=None):
    """the rows LM over the case's word ids: .usr_to_lm is word_to_lm, .finish the finish index"""
    return SmRowsLM((c["seed"] if seed is None else seed) ^ 0xABCDEF, n_words(c), c["W"], c["perm"], c["finish"], 0,
                    c["inf_mod"])


def case_model(c, seed=None):
    return G.case_model(c, seed)


def restate_case(c, nodes, seed=None, ties=None, stats=None):
    """restate_lex on a case (a word LM: is_lm_token False): -> (final, rows per step, the LM adapter)"""
    import test_lexicon_seq2seq as T
    lm = G.PrefixObjLM(case_lm(c, seed))
    final, rows = T.restate_lex(case_model(c, seed), nodes, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"],
                                c["eos_score"], c["eos"], c["maxlen"], c["log_add"], False, ties=ties, stats=stats)
    return final, rows, lm


def both_labels(hyps):
    """two hypotheses with the same tokens and different words"""
    seen = {}
    for h in hyps:
        if seen.setdefault(tuple(h[3]), h[4]) != h[4]:
            return True
    return False


def build_driver(d, ref):
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "lex_s2s_word_lm_rows_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref,
                    os.path.join(HERE, "lex_s2s_word_lm_rows_ref_driver.cpp"),
                    os.path.join(dec, "LexiconSeq2SeqDecoder.cpp"), os.path.join(dec, "Trie.cpp"),
                    os.path.join(dec, "Utils.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, c, seed, lexpath, junk):
    args = [exe, str(seed), str(c["V"]), str(c["K"]), str(c["Kt"]), repr(c["thr"]), repr(c["lmw"]),
            repr(c["word_score"]), repr(c["eos_score"]), str(c["eos"]), str(c["maxlen"]),
            repr(float(np.float32(c["eos_bias"]))), repr(c["drop"]), str(int(c["log_add"])), lexpath,
            str(seed ^ 0xABCDEF), str(c["W"]), str(c["perm"]), str(c["finish"]), str(c["inf_mod"]), str(junk),
            str(n_words(c))]
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
    from text_amd import _capi
    import test_lexicon_seq2seq as T
    ref = os.environ.get("FLTX_REFERENCE", "/root/reference")
    lib = _capi.Lib(os.path.join(ROOT, "tests", "emu", "libfltx_emu.so"))
    out = []
    with tempfile.TemporaryDirectory() as d:
        exe = build_driver(d, ref)
        for spec in CASES:
            c = dict(zip(FIELDS, spec))
            lex = lexicon(c)
            assert max(lab for lab, _, _ in lex) < n_words(c) <= c["W"] and 0 <= c["finish"] < c["W"], c["name"]
            lexpath = os.path.join(d, c["name"] + ".lex")
            with open(lexpath, "w") as f:
                for lab, sc, toks in lex:
                    f.write("%d %s %s\n" % (lab, repr(sc), " ".join(map(str, toks))))
            nodes = T.trie_nodes(T.host_trie(lib, c["V"], lex, SMEAR_MAX))
            assert any(n[2] != 0 for n in nodes[1:]), c["name"]  # (lexMaxScore terms matter)
            seed = 1000 * (len(out) + 1)
            while True:
                ties, stats = [], {}
                got, _, lm = restate_case(c, nodes, seed, ties, stats)
                ok = not ties and stats.get("merges", 0) >= c["min_merges"]
                ok = ok and (not c["inf_mod"] or lm.infs > 0)
                ok = ok and (not c["unfinished"] or any(h[3][-1] != c["eos"] for h in got))
                ok = ok and (not c["both_labels"] or both_labels(got))
                a = None
                if ok and c["inf_mod"]:
                    a = run_driver(exe, c, seed, lexpath, 0)
                    ok = G.same(got, a, c["log_add"])  # (else: a NaN candidate came first in a step)
                if ok:
                    break
                seed += 1
            a = a or run_driver(exe, c, seed, lexpath, 0)
            b = run_driver(exe, c, seed, lexpath, 4096)
            assert a == b, c["name"]
            assert G.same(got, a, c["log_add"]), (c["name"], got[:2], a[:2])
            c["seed"] = seed
            c["merges"] = stats.get("merges", 0)
            c["infs"] = lm.infs
            c["hyps"] = a
            out.append(c)
            print(c["name"], "seed", seed, "hyps", len(a), "merges", c["merges"], "infs", lm.infs)
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
