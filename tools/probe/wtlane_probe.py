"""Word pieces with a token n-gram LM: "wtlane" 0 (the generic engine) against 1 (fltx_wlane.h's TL variant) on one
library, in alternating runs -- bench.py --workload WP's shape (N = 1 024, token beam 50, beam 50, T = 1 000, 256
utterances) with a 3-gram token LM from text_amd/ngram_synth.py.

  python tools/probe/wtlane_probe.py [--tokens 1024] [--batch 256] [--runs 3] [--only 0|1] [--stats]

Prints one line per run (kernel / back-trace ms from the library's events), whether the n-best of the two settings are
equal on the timed batch, and with --stats the share of (lane, position) pairs the filter dropped and the memo's hit
rate (a run with the phase clocks on: not a timed one).  --only runs one setting alone (for a kernel trace)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
import helpers  # noqa: E402
from text_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=1024)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--only", type=int, default=-1)
ap.add_argument("--stats", action="store_true")
a = ap.parse_args()

sess = helpers.FltxSession(None)
N, B, T = a.tokens, a.batch, a.frames
c = cases.case("wt_probe", dist="ctc", T=T, N=N, K=50, Kt=50, u=0, lm=("ngram", 3, 11), lm_weight=0.8)
inp = helpers.case_inputs(c)
if B * T * N <= 1 << 28:
    e = synth.batch("ctc", B, T, N)
else:
    # (the project's generator takes 17 s per utterance of 1 000 x 8 192: rows of the same kind from NumPy -- normal logits, a
    # winner 12 above them in every frame, the blank in six frames of ten, log-softmax in float32)
    rng = np.random.default_rng(11)
    e = np.empty((B, T, N), dtype=np.float32)
    for b in range(B):
        x = rng.standard_normal((T, N), dtype=np.float32)
        win = np.where(rng.random(T) < 0.6, N - 1, rng.integers(0, N - 1, T))
        x[np.arange(T), win] += 12.0
        x -= x.max(axis=1, keepdims=True)
        e[b] = x - np.log(np.exp(x).sum(axis=1, keepdims=True, dtype=np.float32))
decs = {}
for on in ((0, 1) if a.only < 0 else (a.only,)):
    decs[on] = sess.decoder(c, inp)
    decs[on].set("wtlane", on)
for run in range(a.runs):
    for on, d in decs.items():
        t0 = time.perf_counter()
        d.decode_batch(e, [T] * B, N)
        sess.ctx.synchronize()
        wall = time.perf_counter() - t0
        print("run", run, "wtlane", on, "engine", d.get("engine"), "served", d.get("wtlane"), "redone", d.get("redone"),
              "why", d.get("why_not_lane"), "wall ms", round(wall * 1e3, 2), "kernel/backtrace ms", d.timing(), flush=True)
if len(decs) == 2:
    bad = [b for b in range(B) if not helpers.hyps_equal(decs[0].results(b), decs[1].results(b))[0]]
    print("n-best of the two settings equal on the timed batch:", not bad, bad[:5])
if a.stats and 1 in decs:
    d = decs[1]
    d.set("profile", 1)
    d.decode_batch(e, [T] * B, N)
    p = d.profile()
    pairs, dropped, asked, hits = int(p[6]) & 0xFFFFFFFF, int(p[6]) >> 32, int(p[7]) & 0xFFFFFFFF, int(p[7]) >> 32
    print("pairs", pairs, "dropped by the filter", dropped, "(%.1f %%)" % (100.0 * dropped / max(1, pairs)), "look-ups", asked,
          "memo hits", hits, "(%.1f %%)" % (100.0 * hits / max(1, asked)), "phase clocks", [int(x) for x in p[:6]])
for d in decs.values():
    d.close()
