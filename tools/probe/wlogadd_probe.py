"""Word pieces with logAdd: "wlogadd" 0 (the generic engine) against 1 (fltx_wlane.h's LA variants) on one library, in
alternating runs -- bench.py --workload WP's shape (N = 1 024, token beam 50, beam 50, T = 1 000, 256 utterances) with
DecoderOptions::logAdd, under ZeroLM and with a 3-gram token LM from text_amd/ngram_synth.py ("wtlane" = 1 in both
settings: alone it refuses logAdd).

  python tools/probe/wlogadd_probe.py [--tokens 1024] [--batch 256] [--frames 1000] [--runs 3] [--lm zero|ngram|both]

One warm-up run per setting, then --runs timed ones each, alternating.  Prints one line per run (kernel / back-trace ms
from the library's events), min - max of the decode kernel per setting, and whether the n-best of all utterances of the
two settings agree within 1e-5 (tokens exact)."""
import argparse
import os
import sys
import time

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
ap.add_argument("--lm", default="both")
a = ap.parse_args()

sess = helpers.FltxSession(None)
N, B, T = a.tokens, a.batch, a.frames
e = synth.batch("ctc", B, T, N)
for name, lm in (("zero", {}), ("ngram", dict(lm=("ngram", 3, 11), lm_weight=0.8))):
    if a.lm not in ("both", name):
        continue
    c = cases.case("wla_probe", dist="ctc", T=T, N=N, K=50, Kt=50, u=0, log_add=True, **lm)
    inp = helpers.case_inputs(c)
    decs, kern = {}, {0: [], 1: []}
    for on in (0, 1):
        decs[on] = sess.decoder(c, inp)
        decs[on].set("wlogadd", on)
        decs[on].set("wtlane", 1 if lm else 0)
    for run in range(-1, a.runs):  # (-1: the warm-up)
        for on, d in decs.items():
            t0 = time.perf_counter()
            d.decode_batch(e, [T] * B, N)
            sess.ctx.synchronize()
            wall = time.perf_counter() - t0
            tm = d.timing()
            if run >= 0:
                kern[on].append(float(tm[0]))
            print("lm", name, "run", run, "wlogadd", on, "engine", d.get("engine"), "served", d.get("wlogadd"), "redone",
                  d.get("redone"), "why", d.get("why_not_lane"), "wall ms", round(wall * 1e3, 2), "kernel/backtrace ms", tm,
                  flush=True)
    for on in (0, 1):
        print("lm", name, "wlogadd", on, "decode kernel ms min - max", round(min(kern[on]), 3), "-", round(max(kern[on]), 3))
    bad = [b for b in range(B) if not helpers.hyps_equal(decs[0].results(b), decs[1].results(b), 1e-5)[0]]
    # (two hypotheses closer than twice the tolerance may change places: such an utterance is named, not counted)
    tied = []
    for b in bad:
        s = sorted(h.score for h in decs[0].results(b))
        if any(y - x < 2e-5 for x, y in zip(s, s[1:])):
            tied.append(b)
    print("lm", name, "n-best of the two settings within 1e-5 on", B - len(bad), "of", B, "utterances; differ:", bad[:8],
          "of which with a near tie in the n-best:", tied[:8], flush=True)
    for d in decs.values():
        d.close()
