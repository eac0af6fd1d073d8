"""Fixtures of the rows LM (tests/golden/seq2seq_lm_rows_expected.json.gz) from the reference itself.

Dev container only: compiles the unmodified LexiconFreeSeq2SeqDecoder.cpp and Utils.cpp of the reference tree (default
/root/reference, or $FLTX_REFERENCE) with s2s_lm_rows_ref_driver.cpp into a temporary directory, and runs every case
twice under different heap layouts (the two runs must agree).  The LM scores a whole vocabulary per state (SmRowsLM: a
splitmix64 function of (seed, prefix, LM index), exact in float32); its state is the prefix.  A case's seed is the first
from its base on whose search the float64 restatement of tests/test_seq2seq.py sees no tie at a token-beam cut or a
K-cut; no case is dropped.  The cases with -inf LM entries (under lm_weight 0 their candidates' scores are NaN: never
candidates) also ask that some -inf entry was read, so that the fixture shows the rule, and that no step's first
candidate is NaN (the restatement's max() is the reference's best only then).  The generator asserts that the
restatement reproduces the driver.  No reference source text is copied.

    python tests/golden/make_s2s_lm_rows_golden.py
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
from make_s2s_golden import M64, SmModel, _sm64_np, sm64  # noqa: E402

OUT = os.path.join(HERE, "seq2seq_lm_rows_expected.json.gz")


def lm_map(V, W, perm):
    """usr_to_lm of a case: the identity, or the first V of [0, W) ordered by a hash (a permutation)"""
    if not perm:
        return np.arange(V, dtype=np.int32)
    keys = [sm64(perm ^ (a + 1)) for a in range(W)]
    return np.asarray(sorted(range(W), key=lambda a: keys[a])[:V], dtype=np.int32)


class SmRowsLM:
    """The driver's LM: row(prefix) -> W float32 answers, one per LM index; a pure function of (seed, prefix)."""

    def __init__(self, seed, V, W, perm, finish, eos, inf_mod=0):
        self.seed, self.W, self.inf_mod = seed, W, inf_mod
        self.usr_to_lm = lm_map(V, W, perm)
        self.finish = finish if finish >= 0 else (int(self.usr_to_lm[eos]) if eos < V else 0)
        self.infs = 0

    def row(self, prefix):
        h = sm64(self.seed ^ 0x5DEECE66D)
        for tok in prefix:
            h = sm64(h ^ ((tok + 1) & M64))
        with np.errstate(over="ignore"):
            v = (np.arange(self.W, dtype=np.uint64) + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)
            x = _sm64_np(np.uint64(h) ^ v)
            r = (-((x >> np.uint64(40)).astype(np.float64) * 2.0 ** -20)).astype(np.float32)
            if self.inf_mod:
                r[_sm64_np(x ^ np.uint64(0xC0FFEE)) % np.uint64(self.inf_mod) == 0] = -np.inf
        return r


class PrefixLM:
    """The host LM restate() takes: the state is the prefix, the answers are the rows LM's."""

    def __init__(self, rows_lm):
        self.r = rows_lm
        self.rows = {}

    def start(self):
        return ()

    def _at(self, ctx, idx):
        if ctx not in self.rows:
            self.rows[ctx] = self.r.row(list(ctx))
        v = float(self.rows[ctx][idx])
        self.r.infs += v == -np.inf
        return v

    def score(self, ctx, n):
        return ctx + (n,), self._at(ctx, int(self.r.usr_to_lm[n]))

    def finish(self, ctx):
        return ctx, self._at(ctx, self.r.finish)


# (name, V, K, Kt, thr, lmw, eos_score, eos, maxlen, eos_bias, drop, log_add, W, perm, finish, inf_mod)
CASES = [
    ("identity", 29, 8, 12, 25.0, 0.7, 0.0, 3, 6, 0.2, 0.0, False, 29, 0, -1, 0),
    ("identity_logadd", 29, 8, 12, 25.0, 0.7, 0.0, 3, 6, 0.2, 0.0, True, 29, 0, -1, 0),
    ("perm_wide", 29, 8, 12, 25.0, 0.7, -0.2, 3, 6, 0.2, 0.05, False, 50, 77, -1, 0),
    ("finish_ne_eos", 29, 8, 29, 25.0, 1.2, 0.0, 5, 6, 0.3, 0.0, False, 40, 78, 39, 0),
    ("lmw0", 29, 8, 12, 25.0, 0.0, 0.0, 3, 6, 0.2, 0.0, False, 29, 0, -1, 0),
    ("lmw0_perm_dropped", 64, 6, 40, 3.0, 0.0, -0.3, 0, 6, 0.3, 0.1, False, 80, 79, 70, 0),
    ("eos_score_thr", 29, 8, 10, 0.5, 0.7, -0.75, 0, 7, 0.3, 0.2, False, 29, 0, 17, 0),
    ("k50", 64, 50, 40, 25.0, 1.2, 0.25, 6, 5, 0.05, 0.05, False, 64, 80, -1, 0),
    ("k50_v1000_kt64", 1000, 50, 64, 25.0, 0.7, 0.0, 11, 4, 0.02, 0.0, False, 1200, 81, 1199, 0),
    ("v1000_lmw0_kt1000", 1000, 8, 1000, 25.0, 0.0, 0.0, 11, 4, 0.02, 0.0, True, 1000, 0, -1, 0),
    ("eos_ge_v", 12, 4, 12, 25.0, 0.7, 0.0, 12, 4, 0.0, 0.0, False, 12, 0, -1, 0),
    ("k1", 29, 1, 5, 25.0, 1.2, 0.0, 3, 6, 0.1, 0.0, False, 29, 82, -1, 0),
    ("nan_lmw0_inf", 12, 4, 5, 25.0, 0.0, 0.0, 2, 5, 0.2, 0.0, False, 12, 0, -1, 3),
    ("inf_lmw", 12, 4, 5, 25.0, 0.7, 0.0, 2, 5, 0.2, 0.0, False, 12, 0, -1, 5),
]
FIELDS = ["name", "V", "K", "Kt", "thr", "lmw", "eos_score", "eos", "maxlen", "eos_bias", "drop", "log_add", "W", "perm",
          "finish", "inf_mod"]


def case_lm(c):
    return SmRowsLM(c["seed"] ^ 0xABCDEF, c["V"], c["W"], c["perm"], c["finish"], c["eos"], c["inf_mod"])


def case_model(c):
    return SmModel(c["seed"], c["V"], c["eos"], c["eos_bias"], c["drop"])


def build_driver(d, ref):
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "s2s_lm_rows_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref,
                    os.path.join(HERE, "s2s_lm_rows_ref_driver.cpp"), os.path.join(dec, "LexiconFreeSeq2SeqDecoder.cpp"),
                    os.path.join(dec, "Utils.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, c, junk):
    args = [exe, str(c["seed"]), str(c["V"]), str(c["K"]), str(c["Kt"]), repr(c["thr"]), repr(c["lmw"]),
            repr(c["eos_score"]), str(c["eos"]), str(c["maxlen"]), repr(float(np.float32(c["eos_bias"]))),
            repr(c["drop"]), str(int(c["log_add"])), str(c["seed"] ^ 0xABCDEF), str(c["W"]), str(c["perm"]),
            str(c["finish"]), str(c["inf_mod"]), str(junk)]
    out = subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout
    hyps = []
    for line in out.strip().splitlines():
        f = line.split()
        hyps.append([float(f[0]), float(f[1]), float(f[2]), [int(x) for x in f[3:]]])
    return hyps


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_seq2seq as T
    ref = os.environ.get("FLTX_REFERENCE", "/root/reference")
    out = []
    with tempfile.TemporaryDirectory() as d:
        exe = build_driver(d, ref)
        for spec in CASES:
            c = dict(zip(FIELDS, spec))
            c["seed"] = 1000 * (len(out) + 1)
            while True:
                ties = []
                lm = case_lm(c)
                got, _ = T.restate(case_model(c), PrefixLM(lm), c["K"], c["Kt"], c["thr"], c["lmw"], c["eos_score"],
                                   c["eos"], c["maxlen"], ties=ties)
                got = [list(h[:3]) + [h[3]] for h in got]
                a = None
                if not ties and c["inf_mod"] and lm.infs > 0:
                    # (restate's max() is only the reference's best when the step's first candidate is not NaN)
                    a = run_driver(exe, c, 0)
                    if a != got:
                        ties.append("a NaN candidate first in a step")
                if not ties and (not c["inf_mod"] or lm.infs > 0):
                    break
                c["seed"] += 1
            a = a or run_driver(exe, c, 0)
            b = run_driver(exe, c, 4096)
            assert a == b, c["name"]
            assert got == a, (c["name"], got[:2], a[:2])
            c["hyps"] = a
            out.append(c)
            print(c["name"], "seed", c["seed"], "hyps", len(a), "infs", lm.infs)
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
