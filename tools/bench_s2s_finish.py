"""fltx_s2s_finish: device time of finishing and restarting utterances of a running seq2seq batch, and what continuous
batching saves in step calls.

One JSON line per kind: B = 256 slots, beam K = 50, token beam Kt = 50, random float32 log-softmax rows in HBM, eos = V
(never proposed: every beam stays full).  `lexfree`: V = 1024, ZeroLM.  `lexicon`: letters (V = 29), --words = 50 000
spellings, ZeroLM, the default max_states (the slot's state table, which a restart clears and fltx_s2s_begin memsets,
is sized from min(K * max_output_length + 1, max_states)).  Every measurement starts from the same state: begin, --steps = 10 steps.
Device events around the calls, --repeat = 3 runs each after a warm-up round (median, min, max in ms), the variants taken
in turn:
  `end_begin_ms`       what a caller can do without the call: end() followed by begin(), which restarts every utterance
  `finish_all_ms`      finish naming all B slots (restart), results left on the device
  `finish_16_ms`, `finish_1_ms`, `finish_0_ms`   finish naming 16, 1 and none of the slots
The baseline is a build of an earlier commit: copy this file into a checkout of that commit and run it there, with that
tree's own text_amd package and library -- neither has fltx_s2s_finish, and the tool then gives `end_begin_ms` alone.

--counts needs no GPU: for a queue of --utterances whose lengths are drawn once (seeded: a log-normal around a fifth of
max_output_length = 200, clipped to it; listed in the output), the step calls and the listed model rows summed over the
steps, continuous (a slot takes the queue's next utterance when its own is done; done_each asked every step) against B at
a time.  These are counts, not times: the model's own time per row is not measured here.

    python tools/bench_s2s_finish.py [--kinds lexfree,lexicon] [--repeat 3] [--steps 10]
    python tools/bench_s2s_finish.py --counts [--utterances 1024] [--B 64]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def counts(n_utt, B, K, max_len, seed):
    g = np.random.default_rng(seed)
    lengths = np.clip(np.rint(g.lognormal(np.log(max_len / 5.0), 0.6, n_utt)), 1, max_len).astype(int).tolist()
    # continuous: every slot steps in lock step; a slot whose utterance is done after a step takes the queue's next
    left = lengths[:B]
    nxt, calls, rows = len(left), 0, 0
    while any(x > 0 for x in left):
        calls += 1
        rows += sum(K if x > 0 else 0 for x in left)  # (a full beam's rows per running utterance: an upper bound)
        for b in range(len(left)):
            if left[b] > 0:
                left[b] -= 1
                if left[b] == 0 and nxt < n_utt:
                    left[b] = lengths[nxt]
                    nxt += 1
    batch_calls = sum(max(lengths[i:i + B]) for i in range(0, n_utt, B))
    return {"config": {"utterances": n_utt, "B": B, "K": K, "max_output_length": max_len, "seed": seed},
            "continuous_step_calls": calls, "b_at_a_time_step_calls": batch_calls,
            "listed_rows_summed_over_steps": rows,  # (the same utterances list the same rows under either schedule)
            "continuous_rows_per_step_call": rows / calls, "b_at_a_time_rows_per_step_call": rows / batch_calls,
            "lengths": lengths}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--Kt", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--words", type=int, default=50000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kinds", default="lexfree,lexicon")
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--utterances", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    if a.counts:
        print(json.dumps(counts(a.utterances, a.B or 64, a.K, a.max_len, a.seed)), flush=True)
        return
    import torch
    from text_amd import _capi
    from bench_lex_s2s import lexicon, timed
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    zero = _capi.ZeroLM(ctx)
    B, K, Kt = a.B or 256, a.K, a.Kt
    for kind in a.kinds.split(","):
        lex = kind == "lexicon"
        V = 29 if lex else 1024
        scores = [torch.randn(B * K, V, device="cuda").log_softmax(-1) for _ in range(4)]
        trie = None
        if lex:
            trie = _capi.HostTrie(V, 0)
            g = np.random.default_rng(3)
            for w, toks in enumerate(lexicon(V, a.words, 7, False)):
                trie.insert(toks, w, float(np.float32(-g.random() * 5)))
            trie.smear(1)
            dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, _capi.make_s2s_lex_options(K, Kt, 1e9, 0.5, 0.2), trie, zero, V,
                                                   a.max_len)
        else:
            dec = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 1e9), zero, V, a.max_len)

        def state_s():
            dec.begin(B, V)
            for t in range(a.steps):
                dec.step(scores[t % len(scores)])

        def finish(n_named):
            which = np.zeros(B, np.int32)
            which[:n_named] = 1
            return lambda: dec.finish(which, results_on_device=True)

        def pair():
            dec.end()
            dec.begin(B, V)
        variants = {"end_begin_ms": pair}
        if hasattr(dec, "finish") and hasattr(ctx.L.lib, "fltx_s2s_finish"):  # (else: an earlier commit's package)
            variants.update({"finish_all_ms": finish(B), "finish_16_ms": finish(16), "finish_1_ms": finish(1),
                             "finish_0_ms": finish(0)})
        runs = {k: [] for k in variants}
        for rep in range(a.repeat + 1):  # (the first round warms up: buffers are allocated in it)
            for k, fn in variants.items():
                state_s()
                ms = timed(fn, stream)
                if rep:
                    runs[k].append(ms)
        out = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in runs.items()}
        cfg = {"kind": kind, "B": B, "K": K, "Kt": Kt, "V": V, "steps": a.steps, "max_output_length": a.max_len}
        if lex:
            cfg.update(words=a.words)
        dec.close()
        print(json.dumps({"config": cfg, **out}), flush=True)
        if trie is not None:
            trie.close()


if __name__ == "__main__":
    main()
