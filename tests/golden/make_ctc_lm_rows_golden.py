"""Fixtures of the CTC rows decoder (tests/golden/ctc_lm_rows_expected.json.gz) from the reference itself.

Dev container only: compiles the unmodified LexiconFreeDecoder.cpp and Utils.cpp of the reference tree (default
/root/reference, or $FLTX_REFERENCE) with ctc_lm_rows_ref_driver.cpp into oracle/_ref/ (kept out of history), and runs
every case twice under different heap layouts (the two runs must agree).  The LM scores a whole vocabulary per state
(make_s2s_lm_rows_golden.SmRowsLM: a splitmix64 function of (seed, prefix, LM index), exact in float32; its state is the
prefix); the emissions are a splitmix64 function of (seed, frame, token), times 1/4.  A case's seed is the first from its
base on whose search the float64 restatement of tests/test_ctc_lm_rows.py sees no tie (and, under logAdd, no decision
closer than 1e-3); no case is dropped.  The generator asserts that the restatement reproduces the driver: tokens exact,
scores bit-equal under max-merge and within 1e-5 under logAdd.  No reference source text is copied.

    python tests/golden/make_ctc_lm_rows_golden.py
"""
import gzip
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_s2s_golden import _sm64_np, sm64  # noqa: E402
from make_s2s_lm_rows_golden import SmRowsLM  # noqa: E402,F401

OUT = os.path.join(HERE, "ctc_lm_rows_expected.json.gz")


def emissions(seed, T, N):
    """[T, N] float32: the driver's emissions"""
    out = np.zeros((T, N), np.float32)
    with np.errstate(over="ignore"):
        v = (np.arange(N, dtype=np.uint64) + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)
        for t in range(T):
            h = sm64(sm64(seed) ^ (t + 1))
            x = _sm64_np(np.uint64(h) ^ v)
            out[t] = (-((x >> np.uint64(40)).astype(np.float64) * 2.0 ** -20)).astype(np.float32) * np.float32(0.25)
    return out


# (name, T, N, K, Kt, thr, lmw, sil_score, sil, blank, log_add, W, perm)
CASES = [
    ("t1_n3_k1", 1, 3, 1, 3, 25.0, 0.7, 0.0, 1, 0, False, 3, 0),
    ("t7_n3_k2", 7, 3, 2, 3, 25.0, 0.7, 0.0, 1, 0, False, 3, 0),
    ("t12_n3_k8", 12, 3, 8, 3, 25.0, 0.7, 0.0, 1, 0, False, 3, 0),
    ("t12_n3_k8_logadd", 12, 3, 8, 3, 25.0, 0.7, 0.0, 1, 0, True, 3, 0),
    ("t7_n6_k8_kt4", 7, 6, 8, 4, 25.0, 0.7, 0.0, 0, 1, False, 6, 0),
    ("t12_n6_k8_thr", 12, 6, 8, 6, 1.5, 0.7, 0.0, 0, 1, False, 6, 0),
    ("t12_n6_k8_sil", 12, 6, 8, 6, 25.0, 0.7, -0.4, 2, 1, False, 6, 0),
    ("t12_n6_k8_lmw0", 12, 6, 8, 6, 25.0, 0.0, 0.0, 0, 1, False, 6, 0),
    ("t12_n6_k8_perm_wide", 12, 6, 8, 5, 25.0, 0.7, 0.3, 0, 5, False, 11, 83),
    ("t7_n6_k2_perm_logadd", 7, 6, 2, 6, 3.0, 0.7, -0.2, 0, 1, True, 9, 84),
    ("t12_n6_k8_logadd_lmw0", 12, 6, 8, 6, 25.0, 0.0, 0.0, 3, 3, True, 6, 0),
    ("t1_n6_k8", 1, 6, 8, 6, 25.0, 0.7, 0.0, 0, 1, False, 7, 85),
]
FIELDS = ["name", "T", "N", "K", "Kt", "thr", "lmw", "sil_score", "sil", "blank", "log_add", "W", "perm"]


def case_lm(c):
    return SmRowsLM(c["seed"] ^ 0xABCDEF, c["N"], c["W"], c["perm"], c["W"] - 1, 0)


def build_driver(ref):
    d = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(d, exist_ok=True)
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "ctc_lm_rows_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref,
                    os.path.join(HERE, "ctc_lm_rows_ref_driver.cpp"), os.path.join(dec, "LexiconFreeDecoder.cpp"),
                    os.path.join(dec, "Utils.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, c, junk):
    args = [exe, str(c["seed"]), str(c["T"]), str(c["N"]), str(c["K"]), str(c["Kt"]), repr(c["thr"]), repr(c["lmw"]),
            repr(c["sil_score"]), str(c["sil"]), str(c["blank"]), str(int(c["log_add"])), str(c["seed"] ^ 0xABCDEF),
            str(c["W"]), str(c["perm"]), str(c["W"] - 1), str(junk)]
    out = subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout
    hyps = []
    for line in out.strip().splitlines():
        f = line.split()
        hyps.append([float(f[0]), float(f[1]), float(f[2]), [int(x) for x in f[3:]]])
    return hyps


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_ctc_lm_rows as T
    exe = build_driver(os.environ.get("FLTX_REFERENCE", "/root/reference"))
    out = []
    for spec in CASES:
        c = dict(zip(FIELDS, spec))
        c["seed"] = 1000 * (len(out) + 1)
        while True:
            st = T.Stats()
            rl = case_lm(c)
            lm = T.PrefixLM(lambda p: rl.row(list(p)), rl.usr_to_lm, rl.finish)
            got, _ = T.restate(emissions(c["seed"], c["T"], c["N"]), lm, c["K"], c["Kt"], c["thr"], c["lmw"],
                               c["sil_score"], c["sil"], c["blank"], c["log_add"], st=st)
            if not st.ties and (not c["log_add"] or st.gap > T.MIN_GAP):
                break
            c["seed"] += 1
        a = run_driver(exe, c, 0)
        b = run_driver(exe, c, 4096)
        assert a == b, c["name"]
        T.assert_final(a, [(g[0], g[1], g[2], list(g[3])) for g in got], c["log_add"], c["name"])
        c["hyps"] = a
        out.append(c)
        print(c["name"], "seed", c["seed"], "hyps", len(a), "merges", st.merges, "reentered", st.reentered, "gap", st.gap)
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
