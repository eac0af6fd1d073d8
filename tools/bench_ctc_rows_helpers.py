"""CtcRowsBatchDecoder.decode() next to decode_device(): wall time of a whole batch with a small torch LM.

B = 64 utterances of T = 200 frames, N = 29 letters, beam K = 50, random float32 log-softmax emissions in HBM.  The LM
reads the last three tokens of a state's prefix: an embedding per position, summed, tanh, a linear layer, log-softmax
(lm_width = N + 1, the last entry the finish entry).
decode() hands the callable (utterance, prefix) keys: it builds the [n, 3] context on the host, copies it over and runs
the LM.  decode_device() hands it the planner's lists: the context of every row of the store is kept on the device
(ctx[new_row] = ctx[new_parent_row] shifted by new_edge) and the LM runs on those n_new rows; the host reads the plan's
four counts per frame.  One JSON line: wall milliseconds of each helper (the median of --reps runs after a warm-up), the
time decode_device spends in plan() + the counts read, in lm_new and in step(), and how far the two n-best agree.

    python tools/bench_ctc_rows_helpers.py [--B 64] [--K 50] [--T 200] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text_amd import _capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--N", type=int, default=29)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    B, K, T, N = a.B, a.K, a.T, a.N
    W, H, C = N + 1, 64, 3
    torch.manual_seed(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    em = torch.randn(B * T, N, device="cuda").log_softmax(-1).contiguous()
    emb = torch.randn(C, N + 1, H, device="cuda") * 0.5  # (index N: no token at this position)
    out = torch.randn(H, W, device="cuda") * 0.5
    Ts = np.full(B, T, np.int32)

    def lm(context):  # [n, 3] int64 on the device -> [n, W] log-probs
        h = sum(emb[i][context[:, i]] for i in range(C))
        return torch.log_softmax(torch.tanh(h) @ out, -1)

    rows_lm = _capi.RowsLM(W, None, N)
    dec = _capi.CtcRowsBatchDecoder(ctx, _capi.make_options(K, N, 25.0, 0.7), rows_lm, 0, 1)

    def lm_rows(keys):
        c = np.full((len(keys), C), N, np.int64)
        for i, (_, p) in enumerate(keys):
            if p:
                c[i, C - min(C, len(p)):] = p[-C:]
        return lm(torch.from_numpy(c).cuda())

    cap = B * (K * T + 2)
    store = torch.zeros(cap, W, device="cuda")
    context = torch.full((cap, C), N, device="cuda", dtype=torch.int64)
    spent = {"lm_new": 0.0}

    def lm_new(p, n_new):
        t0 = time.perf_counter()
        rows, par, edge = p.new_row[:n_new].long(), p.new_parent_row[:n_new].long(), p.new_edge[:n_new].long()
        c = torch.cat([context[par.clamp_min(0)][:, 1:], edge[:, None]], 1)
        c = torch.where((par >= 0)[:, None], c, torch.full_like(c, N))
        context[rows] = c
        store[rows] = lm(c)
        spent["lm_new"] += time.perf_counter() - t0

    def wall(fn):
        ts = []
        for _ in range(a.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), res

    def host():
        return dec.decode(None, Ts, N, lm_rows, device_ptr=em.data_ptr())

    def device():
        return dec.decode_device(None, Ts, N, store, lm_new, device_ptr=em.data_ptr())
    host()
    device()
    host_ms, want = wall(host)
    # where decode_device's time goes: plan() + the counts read, lm_new, step()
    inner_planned, inner_step = dec._planned, dec.step

    def planned(*args):
        t0 = time.perf_counter()
        r = inner_planned(*args)
        spent["planned"] = spent.get("planned", 0.0) + time.perf_counter() - t0
        return r

    def step(*args, **kw):
        t0 = time.perf_counter()
        r = inner_step(*args, **kw)
        spent["step"] = spent.get("step", 0.0) + time.perf_counter() - t0
        return r
    dec._planned, dec.step = planned, step
    spent["lm_new"] = 0.0
    dev_ms, got = wall(device)
    # (the LM's matrix product runs on other batch shapes in the two helpers: the scores may differ in their last bits)
    same = all([list(h.tokens) for h in w] == [list(h.tokens) for h in g] for w, g in zip(want, got))
    diff = max(abs(x.score - y.score) for w, g in zip(want, got) for x, y in zip(w, g))
    split = {k: v * 1e3 / a.reps for k, v in spent.items()}
    split["plan_and_counts_read"] = split.pop("planned") - split["lm_new"]
    print(json.dumps({"config": {"B": B, "K": K, "T": T, "N": N, "lm_hidden": H, "row_capacity": cap},
                      "decode_ms": host_ms, "decode_device_ms": dev_ms, "decode_device_split_ms": split,
                      "same_tokens": bool(same), "max_score_diff": diff}), flush=True)
    dec.close()
    rows_lm.close()


if __name__ == "__main__":
    main()
