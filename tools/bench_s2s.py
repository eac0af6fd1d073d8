"""Seq2seq decoder step (text_amd/csrc/fltx_s2s.h) against the same step written with torch.topk.

One JSON line per configuration: B = 256 utterances, beam K = 50, token beam Kt = 50, V in {29, 1024, 10000}, 50
steps.  The "model" is a set of score tensors generated before the clock starts (cycled over the steps), so only the
decoder is timed; eos = V (never proposed) keeps every beam full for all steps.  Times are device events on the
stream both run on, after a warm-up.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`
(the front end's GB/s = its bytes per step over fltx_s2s_tokbeam_kernel's time; the line printed here divides the
same bytes by the whole step's time, a lower bound).

    python tools/bench_s2s.py [--steps 50] [--warmup 5] [--V 29,1024,10000]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text_amd import _capi  # noqa: E402


def device_loop(dec, scores, B, V, steps):
    dec.begin(B, V)
    for t in range(steps):
        dec.step(scores[t % len(scores)])


def torch_loop(scores, B, K, Kt, V, steps):
    """The step a PyTorch user writes: top Kt of every row, plus the beam's scores, top K of the flattened candidates,
    the tokens and parents gathered (ZeroLM, no threshold)."""
    beam = torch.zeros(B, K, dtype=torch.float64, device=scores[0].device)
    beam[:, 1:] = -float("inf")
    for t in range(steps):
        s = scores[t % len(scores)].view(B, K, V)
        v, i = torch.topk(s, min(Kt, V), dim=-1)
        cand = (beam[:, :, None] + v.double()).view(B, -1)
        beam, j = torch.topk(cand, K, dim=-1)
        tok = torch.gather(i.view(B, -1), 1, j)
        parent = j // min(Kt, V)
    return tok, parent


def timed(fn, stream, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--Kt", type=int, default=50)
    ap.add_argument("--V", default="29,1024,10000")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    zero = _capi.ZeroLM(ctx)
    B, K, Kt = a.B, a.K, a.Kt
    for V in [int(v) for v in a.V.split(",")]:
        scores = [torch.randn(B * K, V, device="cuda").log_softmax(-1) for _ in range(4)]
        dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 1e9), zero, V, a.steps + 1)
        for _ in range(a.warmup):
            device_loop(dec, scores, B, V, a.steps)
        ms_dev = timed(lambda: device_loop(dec, scores, B, V, a.steps), stream) / a.steps
        dec.end()
        ok = dec.results(0)
        for _ in range(a.warmup):
            torch_loop(scores, B, K, Kt, V, a.steps)
        ms_torch = timed(lambda: torch_loop(scores, B, K, Kt, V, a.steps), stream) / a.steps
        front_bytes = B * K * V * 4
        print(json.dumps({"config": {"B": B, "K": K, "Kt": Kt, "V": V, "steps": a.steps},
                          "device_ms_per_step": ms_dev, "torch_topk_ms_per_step": ms_torch,
                          "speedup_vs_torch": ms_torch / ms_dev,
                          "front_end_bytes_per_step": front_bytes,
                          "front_end_gbps_lower_bound_from_step_time": front_bytes / (ms_dev * 1e-3) / 1e9,
                          "best_hypothesis_length": len(ok[0].tokens) if ok else 0,
                          "facade_b1_ms_per_step": "not measured (no C++ facade; the compat Python class at B = 1 is not timed here)"}), flush=True)
        dec.close()


if __name__ == "__main__":
    main()
