"""Seq2seq shallow fusion on the device (fltx_s2s_step_lm_rows) against ZeroLM and against fusing in torch.

One JSON line per configuration: B = 256 utterances, beam K = 50, token beam Kt = 50, lm_weight 0.5, eos = V (never
proposed: every beam stays full), V in {1024, 10000, 32000}, the LM's rows as wide as the model's, as bf16 log-probs
and as bf16 logits.  The model's rows are float32 log-probs in every leg.  Device-event times per step, after a
warm-up, of
  (a) the same model rows under ZeroLM (fltx_s2s_step);
  (b) the fused step (fltx_s2s_step_lm_rows);
  (c) what a caller writes without it: log_softmax(lm.float()) (logits) or lm.float() (log-probs), topk of the model
      row, rows of -inf with model + lm_weight * lm at the kept tokens, then fltx_s2s_step under ZeroLM -- which gives
      up the separate emittingModelScore / lmScore and the reference's double arithmetic.
Both models' outputs are generated before the clock starts (cycled over the steps).  Kernel times come from a separate
run under `rocprofv3 --kernel-trace --stats` (the program after `--`; --only b keeps that run to the fused step).

    python tools/bench_s2s_lm_rows.py [--steps 30] [--warmup 3] [--V 1024,10000,32000] [--only a,b,c]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text_amd import _capi  # noqa: E402


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
    ap.add_argument("--lm-weight", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args()
    only = set(a.only.split(","))
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    zero, rows = _capi.ZeroLM(ctx), _capi.RowsLM()
    B, K, Kt, lmw = a.B, a.K, a.Kt, a.lm_weight
    n_in = 2
    for V in [int(v) for v in a.V.split(",")]:
        model = [torch.log_softmax(torch.randn(B * K, V, device="cuda") * 3, -1) for _ in range(n_in)]
        lm_logits = [(torch.randn(B * K, V, device="cuda") * 3).to(torch.bfloat16) for _ in range(n_in)]
        lm_lp = [torch.log_softmax(x.float(), -1).to(torch.bfloat16) for x in lm_logits]
        dz = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 1e9), zero, V, a.steps + 1)
        dr = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 1e9, lmw), rows, V, a.steps + 1)

        def zero_lm():
            dz.begin(B, V)
            for t in range(a.steps):
                dz.step(model[t % n_in])

        def fused(lm, kind):
            dr.begin(B, V)
            for t in range(a.steps):
                dr.step(model[t % n_in], lm_scores=lm[t % n_in], lm_kind=kind)

        def in_torch(lm, kind):
            dz.begin(B, V)
            for t in range(a.steps):
                m, x = model[t % n_in], lm[t % n_in].float()
                lp = torch.log_softmax(x, -1) if kind == "logits" else x
                top, idx = m.topk(Kt, -1)
                comb = torch.full_like(m, float("-inf")).scatter_(1, idx, top + lmw * lp.gather(1, idx))
                dz.step(comb)

        for kind, lm in (("log_probs", lm_lp), ("logits", lm_logits)):
            cases = {"a_zero_lm_step": zero_lm, "b_fused_step": lambda: fused(lm, kind),
                     "c_torch_fusion_then_step": lambda: in_torch(lm, kind)}
            ms = {}
            for name, fn in cases.items():
                if name[0] not in only:
                    continue
                for _ in range(a.warmup):
                    fn()
                ms[name] = timed(fn, stream) / a.steps
            out = {"config": {"B": B, "K": K, "Kt": Kt, "V": V, "steps": a.steps, "lm_weight": lmw,
                              "lm_rows": "bf16 " + kind},
                   "ms_per_step": ms, "bytes_per_step": {"model_f32_rows": B * K * V * 4, "lm_bf16_rows": B * K * V * 2}}
            if "b_fused_step" in ms and "c_torch_fusion_then_step" in ms:
                out["b_over_c"] = ms["b_fused_step"] / ms["c_torch_fusion_then_step"]
            if "b_fused_step" in ms and "a_zero_lm_step" in ms:
                out["b_minus_a_ms"] = ms["b_fused_step"] - ms["a_zero_lm_step"]
            print(json.dumps(out), flush=True)
        dz.close()
        dr.close()
        del model, lm_logits, lm_lp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
