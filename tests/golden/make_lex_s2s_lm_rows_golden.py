"""Fixtures of the lexicon seq2seq decoder with a rows LM (tests/golden/lexicon_seq2seq_lm_rows_expected.json.gz) from
the reference itself.

Dev container only: compiles the unmodified LexiconSeq2SeqDecoder.cpp, Trie.cpp and Utils.cpp of the reference tree
(default /root/reference, or $FLTX_REFERENCE) with lex_s2s_lm_rows_ref_driver.cpp into a temporary directory, and runs
every case twice under different heap layouts (the two runs must agree).  The decoder runs with isLmToken = true; the LM
scores a whole vocabulary per state (make_s2s_lm_rows_golden.SmRowsLM) and its state is the token prefix: a child per
token, finish a child (-1) of its own -- PrefixObjLM below names the states the same way for the float64 restatement of
tests/test_lexicon_seq2seq.py (restate_lex), whose merges then are the reference's.  A case's seed is the first from its
base on whose search the restatement sees no tie (a token-beam cut, equal members of a merge group, the kept K); a case
that must show merges also needs the restatement to count some; a case with -inf LM entries needs one to have been read
and the restatement to reproduce the driver (its max() is the reference's best only when no step's first candidate is
NaN); the case that must end at max_output_length needs an unfinished hypothesis in the result.  No case is dropped.
The generator asserts that the restatement reproduces the driver.  No reference source text is copied.

    python tests/golden/make_lex_s2s_lm_rows_golden.py
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
from make_s2s_golden import SmModel  # noqa: E402
from make_s2s_lm_rows_golden import SmRowsLM  # noqa: E402

OUT = os.path.join(HERE, "lexicon_seq2seq_lm_rows_expected.json.gz")


class _State:
    __slots__ = ("prefix", "children")

    def __init__(self, prefix):
        self.prefix, self.children = prefix, {}


class PrefixObjLM:
    """The LM restate_lex takes, over a rows LM (SmRowsLM or anything with row(prefix) / usr_to_lm / finish): states
    are objects as the driver's are -- LMState::child hands out the existing child, finish is the child -1 -- and the
    answers are the row's entries as float32.  reads: every (value) read, for the generator's -inf check."""

    def __init__(self, rows_lm):
        self.r = rows_lm
        self.rows = {}
        self.infs = 0

    def start(self):
        return _State(())

    def _at(self, prefix, idx):
        if prefix not in self.rows:
            self.rows[prefix] = self.r.row(list(prefix))
        v = np.float32(self.rows[prefix][idx])
        self.infs += bool(v == -np.inf)
        return v

    def score(self, st, usr):
        c = st.children.get(usr)
        if c is None:
            c = st.children[usr] = _State(st.prefix + (usr,))
        return c, self._at(st.prefix, int(self.r.usr_to_lm[usr]))

    def finish(self, st):
        c = st.children.get(-1)
        if c is None:
            c = st.children[-1] = _State(st.prefix)
        return c, self._at(st.prefix, self.r.finish)


# (name, V, K, Kt, thr, lmw, word_score, eos_score, eos, maxlen, eos_bias, drop, log_add,
#  lexicon (n_words, seed, max_len, homophones, respell, single), W, perm, finish, inf_mod, min_merges, unfinished)
CASES = [
    ("merge_max", 10, 16, 10, 1e9, 0.6, 0.2, 0.0, 9, 7, 0.5, 0.0, False, (30, 31, 3, 0.0, 0.3, 0.4), 10, 0, -1, 0, 1, 0),
    ("merge_logadd", 10, 16, 10, 1e9, 0.6, 0.2, 0.0, 9, 7, 0.5, 0.0, True, (30, 31, 3, 0.0, 0.3, 0.4), 10, 0, -1, 0, 1,
     0),
    ("perm_wide_finish", 12, 8, 8, 1e9, 0.7, 0.3, -0.2, 11, 7, 0.6, 0.0, False, (40, 5, 3, 0.0, 0.3, 0.3), 20, 77, 19, 0,
     0, 0),
    ("dropped_rows_logadd", 9, 24, 9, 1e9, 0.3, 0.4, 0.0, 0, 8, 0.4, 0.1, True, (30, 12, 3, 0.0, 0.5, 0.3), 12, 78, -1,
     0, 1, 0),
    ("lmw0", 10, 8, 6, 25.0, 0.0, 0.2, 0.0, 9, 6, 0.5, 0.0, False, (30, 31, 3, 0.0, 0.3, 0.4), 10, 0, -1, 0, 0, 0),
    ("lmw0_inf", 10, 8, 8, 25.0, 0.0, 0.2, 0.0, 9, 6, 0.5, 0.0, False, (30, 31, 3, 0.0, 0.3, 0.4), 10, 0, -1, 3, 0, 0),
    ("word_score_single_token_words", 14, 12, 7, 5.0, 0.8, 0.5, 0.0, 0, 6, 0.6, 0.0, False, (40, 22, 3, 0.0, 0.0, 0.8),
     14, 0, 13, 0, 0, 0),
    ("maxlen_unfinished", 12, 8, 12, 1e9, 0.5, 0.3, 0.0, 11, 6, -2.0, 0.0, False, (40, 5, 4, 0.0, 0.2, 0.3), 12, 0, -1,
     0, 0, 1),
    ("k1", 12, 1, 4, 1e9, 0.5, 0.3, 0.0, 11, 6, 0.5, 0.0, False, (40, 8, 4, 0.0, 0.2, 0.3), 12, 79, -1, 0, 0, 0),
    ("v300_kt256", 300, 4, 256, 1e9, 0.7, 0.2, 0.0, 7, 3, 0.3, 0.0, True, (400, 9, 3, 0.0, 0.2, 0.3), 320, 80, 319, 0, 0,
     0),
]
FIELDS = ["name", "V", "K", "Kt", "thr", "lmw", "word_score", "eos_score", "eos", "maxlen", "eos_bias", "drop", "log_add",
          "lex", "W", "perm", "finish", "inf_mod", "min_merges", "unfinished"]


def lexicon(c):
    import test_lexicon_seq2seq as T
    n, seed, max_len, hom, resp, single = c["lex"]
    return T.make_lexicon(c["V"], c["eos"], n, seed, max_len, hom, resp, single)


def case_lm(c, seed=None):
    return SmRowsLM((c["seed"] if seed is None else seed) ^ 0xABCDEF, c["V"], c["W"], c["perm"], c["finish"], c["eos"],
                    c["inf_mod"])


def case_model(c, seed=None):
    return SmModel(c["seed"] if seed is None else seed, c["V"], c["eos"], c["eos_bias"], c["drop"])


def restate_case(c, nodes, seed=None, ties=None, stats=None):
    """restate_lex on a case: -> (final, rows per step, the LM adapter)"""
    import test_lexicon_seq2seq as T
    lm = PrefixObjLM(case_lm(c, seed))
    final, rows = T.restate_lex(case_model(c, seed), nodes, lm, c["K"], c["Kt"], c["thr"], c["lmw"], c["word_score"],
                                c["eos_score"], c["eos"], c["maxlen"], c["log_add"], True, ties=ties, stats=stats)
    return final, rows, lm


def build_driver(d, ref):
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "lex_s2s_lm_rows_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref,
                    os.path.join(HERE, "lex_s2s_lm_rows_ref_driver.cpp"), os.path.join(dec, "LexiconSeq2SeqDecoder.cpp"),
                    os.path.join(dec, "Trie.cpp"), os.path.join(dec, "Utils.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, c, seed, lexpath, junk):
    args = [exe, str(seed), str(c["V"]), str(c["K"]), str(c["Kt"]), repr(c["thr"]), repr(c["lmw"]),
            repr(c["word_score"]), repr(c["eos_score"]), str(c["eos"]), str(c["maxlen"]),
            repr(float(np.float32(c["eos_bias"]))), repr(c["drop"]), str(int(c["log_add"])), lexpath,
            str(seed ^ 0xABCDEF), str(c["W"]), str(c["perm"]), str(c["finish"]), str(c["inf_mod"]), str(junk)]
    out = subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout
    hyps = []
    for line in out.strip().splitlines():
        a, b = line.split("|")
        f = a.split()
        hyps.append([float(f[0]), float(f[1]), float(f[2]), [int(x) for x in f[3:]], [int(x) for x in b.split()]])
    return hyps


def same(got, ref, log_add):
    """the restatement against the driver: tokens and words exact; scores bit-equal, within 1e-5 where logAdd folded"""
    if len(got) != len(ref):
        return False
    for g, r in zip(got, ref):
        if g[3] != r[3] or g[4] != r[4]:
            return False
        if log_add and g[5]:
            if any(abs(x - y) > 1e-5 * max(1.0, abs(y)) for x, y in zip(g[:3], r[:3])):
                return False
        elif list(g[:3]) != r[:3]:
            return False
    return True


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
            nodes = T.trie_nodes(T.host_trie(lib, c["V"], lex, 0))
            um = case_lm(c, 0).usr_to_lm
            assert c["finish"] < 0 or c["finish"] != int(um[c["eos"]]), c["name"]
            seed = 1000 * (len(out) + 1)
            while True:
                ties, stats = [], {}
                got, _, lm = restate_case(c, nodes, seed, ties, stats)
                ok = not ties and stats.get("merges", 0) >= c["min_merges"]
                ok = ok and (not c["inf_mod"] or lm.infs > 0)
                ok = ok and (not c["unfinished"] or any(h[3][-1] != c["eos"] for h in got))
                a = None
                if ok and c["inf_mod"]:
                    a = run_driver(exe, c, seed, lexpath, 0)
                    ok = same(got, a, c["log_add"])  # (else: a NaN candidate came first in a step)
                if ok:
                    break
                seed += 1
            a = a or run_driver(exe, c, seed, lexpath, 0)
            b = run_driver(exe, c, seed, lexpath, 4096)
            assert a == b, c["name"]
            assert same(got, a, c["log_add"]), (c["name"], got[:2], a[:2])
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
