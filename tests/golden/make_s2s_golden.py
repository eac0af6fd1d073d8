"""Fixtures of the seq2seq decoder (tests/golden/seq2seq_expected.json.gz) from the reference itself.

Dev container only: compiles the unmodified LexiconFreeSeq2SeqDecoder.cpp, Utils.cpp and ZeroLM.cpp of the reference
tree (default /root/reference, or $FLTX_REFERENCE) with s2s_ref_driver.cpp into a temporary directory, and runs every
case twice under different heap layouts (the two runs must agree).  A case's seed is the first from its base on whose
search the float64 restatement of tests/test_seq2seq.py sees no tie at a token-beam cut or a K-cut (ties resolve by
partial_sort's or the heap's order, which nothing needs to reproduce).  No reference source text is copied.

    python tests/golden/make_s2s_golden.py
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
OUT = os.path.join(HERE, "seq2seq_expected.json.gz")
M64 = (1 << 64) - 1


def sm64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _sm64_np(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


class SmModel:
    """The driver's model: a pure function of (seed, prefix); rows of -(h >> 40) * 2^-20 (exact in float32)."""

    def __init__(self, seed, V, eos, eos_bias=0.0, drop=0.0):
        self.seed, self.V, self.eos, self.eos_bias, self.drop = seed, V, eos, eos_bias, drop
        self.width = V

    def row(self, prefix):
        h = sm64(self.seed)
        for tok in prefix:
            h = sm64(h ^ ((tok + 1) & M64))
        if len(prefix) > 0 and (sm64(h ^ 0xA5A5A5A5) % 1000000) < self.drop * 1e6:
            return None
        with np.errstate(over="ignore"):
            v = (np.arange(self.V, dtype=np.uint64) + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)
            x = _sm64_np(np.uint64(h) ^ v)
        r = (-((x >> np.uint64(40)).astype(np.float64) * 2.0 ** -20)).astype(np.float32)
        if self.eos < self.V:
            r[self.eos] = r[self.eos] + np.float32(self.eos_bias)
        return r


# (name, V, K, Kt, thr, lmw, eos_score, eos, maxlen, eos_bias, drop, log_add, lm: None | (V of the ARPA vocab, seed))
CASES = [
    ("ref_test_shape", 4, 2, 4, 1000.0, 0.0, 0.0, 4, 3, 0.0, 0.0, True, None),
    ("k1", 29, 1, 5, 25.0, 0.0, 0.0, 3, 6, 0.1, 0.0, False, None),
    ("k2_kt_gt_v", 29, 2, 40, 25.0, 0.0, 0.0, 7, 6, 0.1, 0.0, False, None),
    ("k8_kt_eq_v", 29, 8, 29, 25.0, 0.0, -0.3, 5, 6, 0.2, 0.1, False, None),
    ("k8_small_thr", 29, 8, 10, 0.05, 0.0, 0.0, 5, 7, 0.05, 0.0, False, None),
    ("k50_v1000", 1000, 50, 60, 25.0, 0.0, 0.25, 11, 5, 0.02, 0.05, False, None),
    ("k50_v1000_kt_eq_v", 1000, 50, 1000, 25.0, 0.0, 0.0, 11, 4, 0.02, 0.0, True, None),
    ("k256_v1000", 1000, 256, 8, 25.0, 0.0, 0.0, 2, 3, 0.01, 0.0, False, None),
    ("k8_v10000", 10000, 8, 10000, 25.0, 0.0, -0.1, 9, 4, 0.01, 0.0, False, None),
    ("eos_ge_v", 4, 4, 4, 25.0, 0.0, 0.0, 4, 4, 0.0, 0.0, False, None),
    ("eos_score", 29, 8, 12, 0.5, 0.0, -0.75, 0, 6, 0.3, 0.2, False, None),
    ("ngram", 29, 8, 12, 25.0, 0.7, -0.2, 3, 6, 0.2, 0.05, False, (29, 5)),
    ("ngram_logadd", 29, 8, 12, 25.0, 0.7, -0.2, 3, 6, 0.2, 0.05, True, (29, 5)),
    ("ngram_k50", 64, 50, 40, 25.0, 1.2, 0.0, 6, 5, 0.05, 0.0, False, (64, 7)),
    ("ngram_lmw0", 29, 8, 29, 25.0, 0.0, 0.0, 3, 5, 0.2, 0.0, False, (29, 5)),
]
FIELDS = ["name", "V", "K", "Kt", "thr", "lmw", "eos_score", "eos", "maxlen", "eos_bias", "drop", "log_add", "lm"]


def arpa_file(d, lm):
    """The case's 3-gram over tokens t0 .. t{V-1} (text_amd/ngram_synth.py; deterministic)."""
    from text_amd import ngram_synth
    Vlm, seed = lm
    path = os.path.join(d, "t%d_s%d.arpa" % (Vlm, seed))
    vocab = ngram_synth.words(Vlm, "t")
    if not os.path.exists(path):
        ngram_synth.write_arpa(path, vocab, 3, (0, 400, 200), seed)
    return path, vocab


def build_driver(d, ref):
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "s2s_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref, "-I" + os.path.join(ROOT, "oracle"),
                    os.path.join(HERE, "s2s_ref_driver.cpp"), os.path.join(dec, "LexiconFreeSeq2SeqDecoder.cpp"),
                    os.path.join(dec, "Utils.cpp"), os.path.join(dec, "lm", "ZeroLM.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, c, seed, arpa, junk):
    args = [exe, str(seed), str(c["V"]), str(c["K"]), str(c["Kt"]), repr(c["thr"]), repr(c["lmw"]),
            repr(c["eos_score"]), str(c["eos"]), str(c["maxlen"]), repr(float(np.float32(c["eos_bias"]))),
            repr(c["drop"]), str(int(c["log_add"])), arpa or "-", str(junk)]
    out = subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout
    hyps = []
    for line in out.strip().splitlines():
        f = line.split()
        hyps.append([float(f[0]), float(f[1]), float(f[2]), [int(x) for x in f[3:]]])
    return hyps


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from text_amd import _capi
    import test_seq2seq as T
    ref = os.environ.get("FLTX_REFERENCE", "/root/reference")
    lib = _capi.Lib(os.path.join(ROOT, "tests", "emu", "libfltx_emu.so"))
    out = []
    with tempfile.TemporaryDirectory() as d:
        exe = build_driver(d, ref)
        for spec in CASES:
            c = dict(zip(FIELDS, spec))
            arpa, hl = None, T.HostLM(None)
            if c["lm"]:
                arpa, vocab = arpa_file(d, c["lm"])
                hl = T.HostLM(_capi.ArpaLM(arpa, vocab, lib=lib))
            seed = 1000 * (len(out) + 1)
            while True:
                ties = []
                m = SmModel(seed, c["V"], c["eos"], c["eos_bias"], c["drop"])
                T.restate(m, hl, c["K"], c["Kt"], c["thr"], c["lmw"], c["eos_score"], c["eos"], c["maxlen"], ties=ties)
                if not ties:
                    break
                seed += 1
            a = run_driver(exe, c, seed, arpa, 0)
            b = run_driver(exe, c, seed, arpa, 4096)
            assert a == b, c["name"]
            c["seed"] = seed
            c["hyps"] = a
            out.append(c)
            print(c["name"], "seed", seed, "hyps", len(a))
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
