"""Fixtures of the CTC rows decoder's streams (tests/golden/ctc_lm_rows_stream_expected.json.gz) from the reference itself.

Dev container only: compiles the unmodified LexiconFreeDecoder.cpp and Utils.cpp of the reference tree (default
/root/reference, or $FLTX_REFERENCE) with ctc_lm_rows_stream_ref_driver.cpp into oracle/_ref/ (kept out of history).  A
case is B streams under one list of operations -- ("c", [frames per stream]): decodeStep on the next chunk, ("b", L):
getBestHypothesis(L), ("p", L): prune(L) -- then decodeEnd; the reference decodes every stream on its own, twice under
different heap layouts (the two runs must agree).  Recorded per stream: every best hypothesis (null: an empty result),
nDecodedFramesInBuffer after each prune, the final n-best, and the frames in the buffer at the end.  LM and emissions are
make_ctc_lm_rows_golden.py's.  A stream's seed is the first from its base on whose search the float64 restatement of
tests/test_ctc_lm_rows_stream.py sees no tie (and, under logAdd, no decision closer than 1e-3); no case is dropped.  The
generator asserts that the restatement reproduces the driver.  No reference source text is copied.

    python tests/golden/make_ctc_lm_rows_stream_golden.py
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "ctc_lm_rows_stream_expected.json.gz")


def _rep(n, *ops):
    return [op for _ in range(n) for op in ops]


# (name, Ts, N, K, Kt, thr, lmw, sil_score, sil, blank, log_add, W, perm, max_frames, ops)
CASES = [
    # best(lb) mid-stream for lb = 0, 1 and more than the buffered frames (empty); an empty chunk; prune with too few frames
    ("chunks_best", [9, 7, 5], 5, 4, 5, 25.0, 0.7, 0.0, 0, 1, False, 5, 0, 12,
     [("c", [3, 2, 0]), ("b", 0), ("b", 1), ("b", 99), ("c", [4, 0, 3]), ("b", 0), ("b", 1), ("p", 99),
      ("c", [2, 5, 2]), ("b", 2)]),
    # prune(2), then best(0) (normalised) and best(1) (the frame before keeps its score); prune(0); decoding goes on
    ("prune_then_best", [10], 4, 6, 4, 25.0, 0.7, 0.0, 0, 1, False, 4, 0, 8,
     [("c", [4]), ("b", 0), ("p", 2), ("b", 0), ("b", 1), ("c", [3]), ("b", 0), ("b", 3), ("p", 0), ("b", 0), ("b", 1),
      ("c", [3]), ("b", 0), ("b", 1)]),
    ("logadd_prune", [12, 8], 3, 8, 3, 25.0, 0.7, 0.0, 1, 0, True, 3, 0, 10,
     [("c", [5, 1]), ("p", 2), ("b", 0), ("c", [2, 4]), ("b", 1), ("p", 0), ("c", [5, 3]), ("b", 0), ("p", 2), ("b", 1)]),
    ("sil_thr_perm", [8, 11], 6, 8, 4, 1.5, 0.7, -0.4, 2, 1, False, 9, 84, 9,
     [("c", [5, 3]), ("b", 1), ("p", 2), ("c", [0, 5]), ("b", 0), ("p", 2), ("c", [3, 3]), ("b", 2)]),
    # max_frames 8, 40 frames in chunks of 4, prune(2) after each: the ring of 10 rows wraps four times
    ("ring_wrap", [40], 4, 4, 4, 25.0, 0.7, 0.0, 0, 1, False, 4, 0, 8, _rep(10, ("c", [4]), ("p", 2), ("b", 0), ("b", 2))),
    # K = 70: the first best of best and prune is taken over more than a wave of hypotheses
    ("wide_beam", [8], 6, 70, 6, 1e9, 0.7, 0.0, 0, 1, False, 6, 0, 8,
     [("c", [5]), ("b", 0), ("b", 1), ("p", 2), ("c", [3]), ("b", 0), ("b", 2)]),
]
FIELDS = ["name", "Ts", "N", "K", "Kt", "thr", "lmw", "sil_score", "sil", "blank", "log_add", "W", "perm", "max_frames",
          "ops"]


def stream_script(c, b):
    """the operations of case c as stream b sees them"""
    return [(op, v[b] if op == "c" else v) for op, v in c["ops"]]


def build_driver(ref):
    d = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(d, exist_ok=True)
    dec = os.path.join(ref, "flashlight", "lib", "text", "decoder")
    exe = os.path.join(d, "ctc_lm_rows_stream_ref_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + ref,
                    os.path.join(HERE, "ctc_lm_rows_stream_ref_driver.cpp"), os.path.join(dec, "LexiconFreeDecoder.cpp"),
                    os.path.join(dec, "Utils.cpp"), "-o", exe], check=True)
    return exe


def parse(out):
    """the driver's lines -> dict(best, frames, final)"""
    res = dict(best=[], frames=[], final=[])
    for line in out.strip().splitlines():
        f = line.split()
        if f[0] == "P":
            res["frames"].append(int(f[1]))
            continue
        h = None if len(f) == 1 else [float(f[1]), float(f[2]), float(f[3]), [int(x) for x in f[4:]]]
        res["best" if f[0] == "B" else "final"].append(h)
    return res


def run_driver(exe, c, b, junk):
    seed = c["seeds"][b]
    script = ",".join("%s%d" % (op, v) for op, v in stream_script(c, b))
    args = [exe, str(seed), str(c["Ts"][b]), str(c["N"]), str(c["K"]), str(c["Kt"]), repr(c["thr"]), repr(c["lmw"]),
            repr(c["sil_score"]), str(c["sil"]), str(c["blank"]), str(int(c["log_add"])), str(seed ^ 0xABCDEF),
            str(c["W"]), str(c["perm"]), str(c["W"] - 1), str(junk), script]
    return parse(subprocess.run(args, check=True, stdout=subprocess.PIPE, text=True).stdout)


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_ctc_lm_rows_stream as T
    exe = build_driver(os.environ.get("FLTX_REFERENCE", "/root/reference"))
    out = []
    for spec in CASES:
        c = dict(zip(FIELDS, spec))
        c["ops"] = [list(o) for o in c["ops"]]
        c["seeds"], c["streams"] = [], []
        for b in range(len(c["Ts"])):
            c["seeds"].append(2000 * (len(out) + 1) + 100 * b)
            while True:
                st = T.Stats()
                bests, frames, final, _ = T.case_restate(c, b, st)
                if not st.ties and (not c["log_add"] or st.gap > T.MIN_GAP):
                    break
                c["seeds"][b] += 1
            a = run_driver(exe, c, b, 0)
            assert a == run_driver(exe, c, b, 4096), c["name"]
            a["end_frames"] = len(a["final"][0][3]) - 1
            c["streams"].append(a)
            T.assert_case(c, b, (bests, frames, final), (c["name"], b))
            print(c["name"], b, "seed", c["seeds"][b], "final", len(a["final"]), "merges", st.merges, "gap", st.gap,
                  "frames", a["frames"], "empty bests", sum(1 for h in a["best"] if h is None))
        out.append(c)
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
