"""Seq2seq step fed straight from the model (fltx_s2s_step_typed) against today's float32 log-prob step.

One JSON line per configuration: B = 256 utterances, beam K = 50, token beam Kt = 50, ZeroLM, eos = V (never
proposed: every beam stays full), V in {1024, 10000, 32000}.  Device-event times per step, after a warm-up, of
  (a) fltx_s2s_step on float32 log-probs;
  (b) bf16 logits -> torch.log_softmax(x.float(), -1) -> fltx_s2s_step (what a caller writes without the typed step);
  (c) fltx_s2s_step_typed on the bf16 logits;
  (d) fltx_s2s_step_typed on bf16 log-probs.
The model's outputs are generated before the clock starts (cycled over the steps), so only the conversion and the
decoder are timed.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_s2s_model_output.py [--steps 30] [--warmup 3] [--V 1024,10000,32000]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text_amd import _capi  # noqa: E402


def loop(dec, inputs, B, V, steps, convert=None, kind="log_probs"):
    dec.begin(B, V)
    for t in range(steps):
        x = inputs[t % len(inputs)]
        if convert is not None:
            x = convert(x)
        dec.step(x, kind=kind)


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--Kt", type=int, default=50)
    ap.add_argument("--V", default="1024,10000,32000")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    zero = _capi.ZeroLM(ctx)
    B, K, Kt = a.B, a.K, a.Kt
    n_in = 2
    for V in [int(v) for v in a.V.split(",")]:
        logits = [(torch.randn(B * K, V, device="cuda") * 3).to(torch.bfloat16) for _ in range(n_in)]
        lp32 = [torch.log_softmax(x.float(), -1) for x in logits]
        lp16 = [x.to(torch.bfloat16) for x in lp32]
        dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 1e9), zero, V, a.steps + 1)
        cases = {
            "a_f32_log_probs_step": lambda: loop(dec, lp32, B, V, a.steps),
            "b_bf16_logits_log_softmax_then_step": lambda: loop(dec, logits, B, V, a.steps,
                                                                convert=lambda x: torch.log_softmax(x.float(), -1)),
            "c_typed_step_bf16_logits": lambda: loop(dec, logits, B, V, a.steps, kind="logits"),
            "d_typed_step_bf16_log_probs": lambda: loop(dec, lp16, B, V, a.steps),
        }
        ms = {}
        for name, fn in cases.items():
            for _ in range(a.warmup):
                fn()
            ms[name] = timed(fn, stream) / a.steps
        out = {"config": {"B": B, "K": K, "Kt": Kt, "V": V, "steps": a.steps, "lm": "zero"},
               "ms_per_step": ms,
               "c_over_a": ms["c_typed_step_bf16_logits"] / ms["a_f32_log_probs_step"],
               "c_over_b": ms["c_typed_step_bf16_logits"] / ms["b_bf16_logits_log_softmax_then_step"],
               "bytes_per_step": {"f32_rows": B * K * V * 4, "bf16_rows": B * K * V * 2}}
        print(json.dumps(out), flush=True)
        dec.close()
        del logits, lp32, lp16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
