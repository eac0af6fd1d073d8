"""What a partial result per chunk costs a streaming recogniser: fltx_stream_partials against the loop of
fltx_result_best over all streams.

B parallel streams of one decoder, T = 1000 frames each in chunks of --chunk = 50 frames, prune(--look-back = 20) after
every chunk; C2's shape (LexiconFreeDecoder, ZeroLM, N = 29, beam 50) and C3's (LexiconDecoder on the 90 000-word
lexicon, beam 50, token beam 10), the emissions of tests/cases.py's generator (16 distinct streams, repeated).  Per chunk,
wall time from the call of fltx_stream_step to the end of a synchronise of the context's stream, of

    a          the chunk's decode and its prune alone
    b          ... plus today's way to a partial result: fltx_result_best(b, 0) for every stream and the collapse of each
               frame row on the host (NumPy: drop repeats and blanks, first index of each token)
    c_host     ... plus one fltx_stream_partials(0) whose arrays land in pinned host memory
    c_device   ... plus one fltx_stream_partials(0, on_device) (the two totals alone cross PCIe)

all four through the same library, so the legs differ in nothing else.  A run is one stream from begin to end in one
leg; the legs take turns, --repeat runs each, after --warmup untimed runs of every leg; the first chunk of a run is left
out (its buffers grow).  One JSON line per (workload, B): the median over chunks and runs per leg, the smallest and the
largest run median (the spread), c - a and b - a, and whether b's and c's transcripts agreed on every chunk.
The kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats` (the program after `--`;
--legs c_device keeps that run to the new call).

    python tools/bench_stream_partials.py [--B 1,16,256] [--workloads C2,C3] [--legs a,b,c_host,c_device] [--repeat 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import helpers  # noqa: E402
from text_amd import synth  # noqa: E402


def collapse(tok, blank):
    """the host-side groupby / drop-blank rule of include/fltx.h -> tokens, timesteps"""
    keep = (tok >= 0) & (tok != blank)
    keep[1:] &= tok[1:] != tok[:-1]
    return tok[keep], np.flatnonzero(keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="1,16,256")
    ap.add_argument("--workloads", default="C2,C3")
    ap.add_argument("--legs", default="a,b,c_host,c_device")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--look-back", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another libfltx (the emulator's, to rehearse the script: its times mean nothing)")
    a = ap.parse_args()
    legs = a.legs.split(",")
    sess = helpers.FltxSession(a.lib)  # (the HIP library: raises without it or without a device)
    T, CH, LB = a.T, a.chunk, a.look_back
    for wl in a.workloads.split(","):
        c = dict(cases.BY_NAME[{"C2": "C2_ctc_u0", "C3": "C3_spell_u0"}[wl]], T=T)
        inp = helpers.case_inputs(c)
        N, blank = c["N"], c["N"] - 1
        lex = inp["lex"] if c["dist"] == "lexspell" else None
        distinct = [synth.emissions(c["dist"], 500 + u, T, N, lexicon=lex) for u in range(16)]
        for B in [int(x) for x in a.B.split(",")]:
            chunks = [np.ascontiguousarray(np.concatenate([distinct[b % 16][t:t + CH].reshape(-1) for b in range(B)]),
                                           dtype=np.float32) for t in range(0, T, CH)]
            Tc = [np.full(B, min(CH, T - t), np.int32) for t in range(0, T, CH)]
            d = sess.decoder(c, inp)
            texts = {}

            def run(leg):
                d.stream_begin(B, N, LB + 100 + CH + 4)
                sess.ctx.synchronize()
                times, text = [], []
                for i, ch in enumerate(chunks):
                    t0 = time.perf_counter()
                    d.stream_step(ch, Tc[i])
                    if leg == "b":
                        rows = [collapse(d.best(b, 0, 2048).tokens, blank) for b in range(B)]
                        text.append([r[0].tolist() for r in rows[:16]])
                    elif leg == "c_host":
                        p = d.stream_partials(0)
                        to = p["tok_off"]
                        text.append([p["tokens"][int(to[b]):int(to[b + 1])].tolist() for b in range(min(B, 16))])
                    elif leg == "c_device":
                        d.stream_partials(0, device=True)
                    d.stream_prune(LB)
                    sess.ctx.synchronize()
                    times.append(time.perf_counter() - t0)
                d.stream_end()
                sess.ctx.synchronize()
                texts[leg] = text
                return statistics.median(times[1:]) * 1e3, times[1:]
            for _ in range(a.warmup):
                for leg in legs:
                    run(leg)
            meds = {leg: [] for leg in legs}
            every = {leg: [] for leg in legs}
            for _ in range(a.repeat):
                for leg in legs:  # (the legs take turns: a drift of the machine meets all of them)
                    m, ts = run(leg)
                    meds[leg].append(m)
                    every[leg].extend(ts)
            out = {leg: {"median_ms": statistics.median(every[leg]) * 1e3, "run_median_min_ms": min(meds[leg]),
                         "run_median_max_ms": max(meds[leg])} for leg in legs}
            for leg in legs:
                if leg != "a" and "a" in out:
                    out[leg]["minus_a_ms"] = out[leg]["median_ms"] - out["a"]["median_ms"]
            if "b" in texts and "c_host" in texts:
                out["b_and_c_agree"] = texts["b"] == texts["c_host"]
            engine = d.get("engine")
            d.close()
            print(json.dumps({"config": {"workload": wl, "B": B, "T": T, "chunk": CH, "look_back": LB, "K": c["K"],
                                         "N": N, "engine": engine, "chunks_timed": len(chunks) - 1, "repeat": a.repeat},
                              "per_chunk": out}), flush=True)


if __name__ == "__main__":
    main()
