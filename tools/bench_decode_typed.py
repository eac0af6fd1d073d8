#!/usr/bin/env python3
"""bf16 logits through fltx_decode_batch_typed against the float32 route on the same tensor: torch log_softmax +
.float() + fltx_decode_batch.  The WP shape of bench.py (B = 256, T = 1 000, beam 50, token beam 50, ZeroLM) at the token
sets asked for.  Host clock around work that ends in a synchronise of both streams; the two routes alternate; one JSON
line per token set.  Run under rocprofv3 --kernel-trace --stats (in a run of its own) for the kernels' times:
fltx_tokbeam_typed_kernel is the typed front end, fltx_tokbeam_kernel the float32 one.

    python tools/bench_decode_typed.py --tokens 1024 8192 --reps 5
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

torch.cuda.init()  # (before the library opens the device: see tests/test_seq2seq.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text_amd import _capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = _capi.Context()
    zero = _capi.ZeroLM(ctx)
    T = np.full(a.batch, a.frames, np.int32)
    for N in a.tokens:
        # bench.py's WP emissions ("ctc" rows of text_amd/synth.py) as the model's bf16 output, used as logits; token sets
        # beyond 1 024: that row N / 1 024 times side by side, each copy 1.5 lower than the one before (made on the device:
        # the host generator takes minutes at these sizes)
        base = torch.from_numpy(synth.batch("ctc", a.batch, a.frames, min(N, 1024))).reshape(-1, min(N, 1024)).cuda()
        assert N <= 1024 or N % 1024 == 0, "token sets beyond 1 024: multiples of 1 024"
        logits = torch.cat([base - 1.5 * k for k in range(max(1, N // 1024))], dim=1).to(torch.bfloat16).contiguous()
        del base
        decs = [_capi.BatchDecoder(ctx, _capi.LEXFREE, _capi.make_options(50, 50, 25.0), zero, 0, N - 1) for _ in range(2)]

        def typed():
            decs[0].decode_batch_typed(logits, T, N, kind="logits")
            ctx.synchronize()

        def float32():
            lp = torch.log_softmax(logits, -1).float()
            torch.cuda.synchronize()
            decs[1].decode_batch(None, T, N, device_ptr=lp.data_ptr())
            ctx.synchronize()

        times = {"typed": [], "float32": []}
        for i in range(a.warmup + a.reps):
            for name, fn in (("typed", typed), ("float32", float32)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    times[name].append(time.perf_counter() - t0)
        frames = a.batch * a.frames
        print(json.dumps({"tokens": N, "batch": a.batch, "frames": a.frames, "reps": a.reps,
                          "typed_ms": [round(1e3 * t, 3) for t in times["typed"]],
                          "float32_route_ms": [round(1e3 * t, 3) for t in times["float32"]],
                          "typed_median_mframes_s": round(frames / statistics.median(times["typed"]) / 1e6, 2),
                          "float32_route_median_mframes_s": round(frames / statistics.median(times["float32"]) / 1e6, 2),
                          "typed_engine_wlane": decs[0].get("wlane"), "float32_engine_wlane": decs[1].get("wlane"), "typed_widened": decs[0].get("typed_widened"),
                          "typed_redone": decs[0].get("redone"), "float32_redone": decs[1].get("redone")}), flush=True)
        for d in decs:
            d.close()
        del logits


if __name__ == "__main__":
    main()
