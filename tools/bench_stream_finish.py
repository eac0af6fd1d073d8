"""fltx_stream_finish: device time of finishing and restarting streams of a classic stream batch.

One JSON line: the shape bench.py streams (C2 -- LexiconFreeDecoder + ZeroLM, CTC, N = 29, beam K = 50, B = 256 streams,
50-frame chunks from host memory, prune(0) after each, a 208-frame buffer), random float32 log-softmax emissions from a
seed.  Every measurement starts from the same state: stream_begin, --chunks = 2 chunks stepped and pruned, the device
idle.  Device events around the calls, --repeat = 5 runs each after one warm-up round (median, min, max in ms), the
variants taken in turn:
  `finish_1_ms`, `finish_16_ms`, `finish_all_ms`, `finish_0_ms`   stream_finish naming 1, 16, all B and none of the
                       streams, results left on the device (nothing waited for)
  `finish_*_host_ms`   the same with the results copied home (complete on return)
  `end_begin_ms`       the pair a finish of all B replaces on that state: stream_end() followed by stream_begin()
A library without fltx_stream_finish (the parent commit) reports `end_begin_ms` alone: the yardstick for "all 256".
--profile-loop N runs N finishes of 16 streams on that state and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the two kernels' own times.

    python tools/bench_stream_finish.py [--B 256] [--K 50] [--repeat 5] [--profile-loop 0]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi  # noqa: E402
from bench_lex_s2s import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--N", type=int, default=29)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--profile-loop", type=int, default=0)
    a = ap.parse_args()
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    B, K, N, CH = a.B, a.K, a.N, a.chunk
    lm = _capi.ZeroLM(ctx)
    dec = _capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(K, N, 25.0, 0.0, 0.0, float("-inf"), 0.0, False, "ctc"),
                             lm, 0, N - 1)
    pieces = [torch.randn(B, CH, N).log_softmax(-1).contiguous().numpy() for _ in range(a.chunks)]
    Tc = np.full(B, CH, np.int32)
    has_finish = hasattr(ctx.L.lib, "fltx_stream_finish")

    def state():
        dec.stream_begin(B, N, 4 * CH + 8)
        for p in pieces:
            dec.stream_step(p, Tc)
            dec.stream_prune(0)
        ctx.synchronize()

    def finish(n_named, device):
        which = np.zeros(B, np.int32)
        which[:n_named] = 1
        return lambda: dec.stream_finish(which, device=True) if device else dec.stream_finish(which)

    def pair():
        dec.stream_end()
        dec.stream_begin(B, N, 4 * CH + 8)

    if a.profile_loop:
        state()
        for _ in range(a.profile_loop):
            finish(16, True)()
        ctx.synchronize()
        print(json.dumps({"profile_loop": a.profile_loop, "named": 16, "engine": dec.get("engine"),
                          "sstream": dec.get("sstream")}), flush=True)
        return
    variants = {"end_begin_ms": pair}
    if has_finish:
        for n, tag in ((1, "1"), (16, "16"), (B, "all"), (0, "0")):
            variants["finish_%s_ms" % tag] = finish(n, True)
            variants["finish_%s_host_ms" % tag] = finish(n, False)
    runs = {k: [] for k in variants}
    for rep in range(a.repeat + 1):  # (the first round warms up: buffers are allocated and code objects loaded in it)
        for k, fn in variants.items():
            state()
            ms = timed(fn, stream)
            if rep:
                runs[k].append(ms)
    out = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in runs.items()}
    print(json.dumps({"config": {"B": B, "K": K, "N": N, "chunk": CH, "chunks": a.chunks, "max_frames": 4 * CH + 8,
                                 "repeat": a.repeat, "engine": dec.get("engine"), "sstream": dec.get("sstream"),
                                 "has_stream_finish": has_finish}, **out}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
