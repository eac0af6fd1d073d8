"""Fixtures of the lexicon seq2seq decoder (tests/golden/lexicon_seq2seq_expected.json.gz) from the reference itself.

Dev container only: compiles the unmodified LexiconSeq2SeqDecoder.cpp, Trie.cpp, Utils.cpp and ZeroLM.cpp of the
reference tree (default /root/reference, or $FLTX_REFERENCE) with lex_s2s_ref_driver.cpp into a temporary directory,
and runs every case twice under different heap layouts (the two runs must agree).  A case's seed is the first from its
base on whose search the float64 restatement of tests/test_lexicon_seq2seq.py sees no tie (a token-beam cut, equal
members of a merge group, the kept K -- near-ties under 1e-9 where logAdd folded count); a case that must show merges
also needs the restatement to count some.  The model is make_s2s_golden.SmModel; the lexicon
test_lexicon_seq2seq.make_lexicon.  No reference source text is copied.

    python tests/golden/make_lex_s2s_golden.py
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
OUT = os.path.join(HERE, "lexicon_seq2seq_expected.json.gz")

# (name, V, K, Kt, thr, lmw, word_score, eos_score, eos, maxlen, eos_bias, drop, log_add, is_lm_token, smear,
#  lexicon (n_words, seed, max_len, homophones, respell, single), lm: None | (prefix, n, seed), min_merges)
CASES = [
    ("zero_max", 12, 8, 12, 1e9, 0.5, 0.3, 0.0, 11, 7, 0.8, 0.0, False, False, 1, (40, 5, 4, 0.0, 0.2, 0.1), None, 0),
    ("zero_none", 12, 8, 12, 1e9, 0.5, 0.3, 0.0, 11, 6, 0.8, 0.0, False, False, 0, (40, 5, 3, 0.0, 0.2, 0.5), None, 0),
    ("zero_logadd_smear", 12, 8, 6, 1e9, 0.5, -0.2, 0.0, 11, 7, 0.8, 0.0, False, False, 2, (40, 6, 4, 0.0, 0.2, 0.1),
     None, 0),
    ("zero_word_score_thr", 16, 16, 10, 2.0, 1.0, 1.5, -0.5, 3, 7, 0.6, 0.0, False, False, 1, (60, 7, 4, 0.0, 0.2, 0.2),
     None, 0),
    ("merge_max", 8, 32, 8, 1e9, 0.2, 0.5, 0.0, 7, 8, 0.5, 0.0, False, False, 1, (30, 11, 3, 0.0, 0.5, 0.3), None, 1),
    ("merge_logadd", 8, 32, 8, 1e9, 0.2, 0.5, 0.0, 7, 8, 0.5, 0.0, True, False, 1, (30, 11, 3, 0.0, 0.5, 0.3), None, 1),
    ("merge_dropped_rows", 9, 24, 9, 1e9, 0.3, 0.4, 0.0, 0, 8, 0.4, 0.1, True, False, 2, (30, 12, 3, 0.0, 0.5, 0.3),
     None, 1),
    ("merge_word_lm", 10, 24, 10, 1e9, 0.6, 0.2, -0.2, 9, 8, 0.5, 0.0, False, False, 1, (30, 13, 3, 0.1, 0.5, 0.3),
     ("w", 40, 5), 1),
    ("merge_word_lm_logadd", 10, 24, 10, 1e9, 0.6, 0.2, -0.2, 9, 8, 0.5, 0.0, True, False, 1,
     (30, 13, 3, 0.1, 0.5, 0.3), ("w", 40, 5), 1),
    ("token_lm_merge", 10, 16, 10, 1e9, 0.6, 0.2, 0.0, 9, 7, 0.5, 0.0, True, True, 0, (30, 31, 3, 0.0, 0.3, 0.4),
     ("t", 10, 6), 1),
    ("word_lm_homophones", 14, 12, 14, 1e9, 0.8, -0.2, -0.3, 0, 7, 0.6, 0.05, False, False, 1,
     (40, 21, 4, 0.15, 0.3, 0.1), ("w", 40, 5), 0),
    ("word_lm_single_token_words", 14, 12, 7, 5.0, 0.8, 0.3, 0.0, 0, 6, 0.6, 0.0, False, False, 2,
     (40, 22, 3, 0.0, 0.0, 0.8), ("w", 40, 7), 0),
    ("maxlen_unfinished", 12, 8, 12, 1e9, 0.5, 0.3, 0.0, 11, 3, -0.5, 0.0, False, False, 1, (40, 5, 4, 0.0, 0.2, 0.1),
     None, 0),
    ("k1", 12, 1, 4, 1e9, 0.5, 0.3, 0.0, 11, 6, 0.5, 0.0, False, False, 1, (40, 8, 4, 0.0, 0.2, 0.1), None, 0),
    ("dead_ends_v30", 30, 16, 20, 1e9, 0.3, 0.2, 0.0, 29, 7, 0.3, 0.1, False, False, 1, (25, 9, 5, 0.0, 0.0, 0.0),
     None, 0),
    ("large_k_v64", 64, 64, 40, 1e9, 0.4, 0.1, 0.0, 5, 6, 0.5, 0.05, True, False, 1, (300, 10, 4, 0.0, 0.3, 0.1),
     None, 0),
]
FIELDS = ["name", "V", "K", "Kt", "thr", "lmw", "word_score", "eos_score", "eos", "maxlen", "eos_bias", "drop",
          "log_add", "is_lm_token", "smear", "lex", "lm", "min_merges"]


def arpa_file(d, lm):
    """The case's 3-gram over words w0 .. (or tokens t0 ..) (text_amd/ngram_synth.py; deterministic)."""
    from text_amd import ngram_synth
    prefix, n, seed = lm
    path = os.path.join(d, "%s%d_s%d.arpa" % (prefix, n, seed))
    vocab = ngram_synth.words(n, prefix)
    if not os.path.exists(path):
        ngram_synth.write_arpa(path, vocab, 3, (0, 300, 150), seed)
    return path, vocab


def lexicon(c):
    import test_lexicon_seq2seq as T
    n, seed, max_len, hom, resp, single = c["lex"]
    return T.make_lexicon(c["V"], c["eos"], n, seed, max_len, hom, resp, single)


def build_driver(d, ref):
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "lex_s2s_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref, "-I" + os.path.join(ROOT, "oracle"),
                    os.path.join(HERE, "lex_s2s_ref_driver.cpp"), os.path.join(dec, "LexiconSeq2SeqDecoder.cpp"),
                    os.path.join(dec, "Trie.cpp"), os.path.join(dec, "Utils.cpp"), os.path.join(dec, "lm", "ZeroLM.cpp"),
                    "-o", exe], check=True)
    return exe


def run_driver(exe, c, seed, lexpath, arpa, junk):
    args = [exe, str(seed), str(c["V"]), str(c["K"]), str(c["Kt"]), repr(c["thr"]), repr(c["lmw"]),
            repr(c["word_score"]), repr(c["eos_score"]), str(c["eos"]), str(c["maxlen"]),
            repr(float(np.float32(c["eos_bias"]))), repr(c["drop"]), str(int(c["log_add"])), str(int(c["is_lm_token"])),
            lexpath, str(c["smear"]), arpa or "-", c["lm"][0] if c["lm"] else "w", str(junk)]
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
            lexpath = os.path.join(d, c["name"] + ".lex")
            with open(lexpath, "w") as f:
                for lab, sc, toks in lex:
                    f.write("%d %s %s\n" % (lab, repr(sc), " ".join(map(str, toks))))
            arpa, lm = None, None
            if c["lm"]:
                arpa, vocab = arpa_file(d, c["lm"])
                lm = _capi.ArpaLM(arpa, vocab, lib=lib)
            nodes = T.trie_nodes(T.host_trie(lib, c["V"], lex, c["smear"]))
            seed = 1000 * (len(out) + 1)
            while True:
                ties, stats = [], {}
                m = T.sm_model(seed, c["V"], c["eos"], c["eos_bias"], c["drop"])
                T.restate_lex(m, nodes, T.ObjLM(lm), c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"],
                              c["eos_score"], c["eos"], c["maxlen"], c["log_add"], c["is_lm_token"], ties=ties,
                              stats=stats)
                if not ties and stats.get("merges", 0) >= c["min_merges"]:
                    break
                seed += 1
            a = run_driver(exe, c, seed, lexpath, arpa, 0)
            b = run_driver(exe, c, seed, lexpath, arpa, 4096)
            assert a == b, c["name"]
            c["seed"] = seed
            c["merges"] = stats.get("merges", 0)
            c["hyps"] = a
            out.append(c)
            print(c["name"], "seed", seed, "hyps", len(a), "merges", c["merges"])
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
