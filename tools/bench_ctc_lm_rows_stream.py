"""Streams on the two CTC rows decoders (fltx_ctc_rows_stream_*): device time per frame of a stream, as a ratio to the
offline begin / step / end on the same emissions.

One JSON line per (token set, kind): B = 256 streams of T = 200 frames, beam K = 50, lmWeight 0.7, random float32
log-softmax emissions in HBM, handed over in chunks of --chunk = 20 frames; after each chunk prune(--look-back = 10) and
best(0).  Letters: N = 29, Kt = 29; word pieces: N = 10 000, Kt = 50.  Kinds: `lexfree` (CtcRowsBatchDecoder) and
`lexicon` (LexiconCtcRowsBatchDecoder with the word LM and the lexicons of bench_lex_ctc_lm_rows.py).  The LM is
bench_ctc_lm_rows.py's synthetic device LM: --ctx bf16 log-prob rows, the row of a hypothesis a hash of its stream and its
next_state id, named through lm_row_of.
`stream_ms_per_frame`: device events around stream_begin + the chunks (append, 20 steps, prune, best) + end, after a
warm-up, divided by T.  `offline_ms_per_frame`: the same around begin + T steps + end -- the yardstick, run --repeat
times; its min and max are the run-to-run spread.  `ratio` = stream / offline median.  best() copies its answer to the
host, so a stream waits for the device once per chunk; `stream_no_best_ms_per_frame` is the same loop without best().
`best_all_streams_ms`: wall time of best(b) for all B streams after a chunk (one launch, one copy of the lengths and
scores, then a copy of the tokens per stream).  A stream's LM-state table holds max_states ids, whatever the chunks
bring, and stream_begin clears it: `stream_begin_ms` is its device time at --max-states (default K * T + 2, what the
offline path would size) and `stream_begin_default_ms` at the default of 65 536 ids per stream.
`--collect-every n[,m..]` (off by default): the stream loop again with collect(--release-cap) after every n-th chunk,
after the prune -- `stream_collect_ms_per_frame[n]`, `collect_added_ms_per_call[n]` = (that median - the plain stream's)
* T / calls, and of the last of those runs the ids released in all and the most ids live in any stream after a
collect.  (The LM rows here are a hash of the state id, so a recycled id reads the row it read before: the timing does
not depend on it.)
The medians of the append, prune, best and collect kernels per call come from a separate run under
`rocprofv3 --kernel-trace --stats` (the program after `--`; --only stream keeps that run to the stream).

    python tools/bench_ctc_lm_rows_stream.py [--T 200] [--chunk 20] [--look-back 10] [--sets letters,word_piece]
                                             [--kinds lexfree,lexicon] [--only stream,offline] [--repeat 3]
                                             [--collect-every 1,5] [--release-cap 1024]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi  # noqa: E402
from bench_lex_ctc_lm_rows import lexicons  # noqa: E402
from bench_lex_s2s import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--look-back", type=int, default=10)
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-states", type=int, default=0)
    ap.add_argument("--only", default="stream,offline")
    ap.add_argument("--collect-every", default="")
    ap.add_argument("--release-cap", type=int, default=1024)
    ap.add_argument("--sets", default="letters,word_piece")
    ap.add_argument("--kinds", default="lexfree,lexicon")
    a = ap.parse_args()
    only = set(a.only.split(","))
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    B, K, T, CH, LB = a.B, a.K, a.T, a.chunk, a.look_back
    assert T % CH == 0
    for name, N, Kt, sil, blank in (("letters", 29, 29, 0, 28), ("word_piece", 10000, 50, 0, 1)):
        if name not in a.sets.split(","):
            continue
        em = torch.randn(B * T, N, device="cuda").log_softmax(-1).contiguous()
        Ts = np.full(B, T, np.int32)
        chunk_T = np.full(B, CH, np.int32)
        utt = (torch.arange(B, device="cuda", dtype=torch.int64) * 97)[:, None]
        for kind in a.kinds.split(","):
            lex = kind == "lexicon"
            spell = lexicons(name, N) if lex else None
            W = (len(spell) if lex else N) + 1
            log_probs = torch.log_softmax((torch.randn(a.ctx, W, device="cuda") * 3), -1).to(torch.bfloat16)
            trie = None
            if lex:
                start_row = log_probs[0].float().cpu().numpy()
                trie = _capi.HostTrie(N, sil)
                for w, sp in enumerate(spell):
                    trie.insert(sp, w, float(start_row[w]))
                trie.smear(1)
            lm = (_capi.WordRowsLM if lex else _capi.RowsLM)(W, None, W - 1)
            opts = _capi.make_options(K, Kt, 25.0, 0.7, 0.5)

            def make():
                if lex:
                    return _capi.LexiconCtcRowsBatchDecoder(ctx, opts, trie, lm, sil, blank, -1, False)
                return _capi.CtcRowsBatchDecoder(ctx, opts, lm, sil, blank)

            def row_of(state):  # one LM row per (stream, state id); padding rows (-1) stay out of range
                r = (state.to(torch.int64) * 2654435761 + utt) % a.ctx
                return torch.where(state >= 0, r, torch.full_like(r, -1)).to(torch.int32)
            dec = make()
            seen = {}
            begin_default = timed(lambda: dec.stream_begin(B, N, LB + CH + 2), stream)
            begin_default = timed(lambda: dec.stream_begin(B, N, LB + CH + 2), stream)  # (the second: buffers exist)
            dec.set_max_states(a.max_states or K * T + 2)

            def offline():
                tok, src, state, n = dec.begin(None, Ts, N, device_ptr=em.data_ptr())
                for _ in range(T):
                    tok, src, state, n = dec.step(log_probs, lm_row_of=row_of(state))
                dec.end(log_probs, lm_row_of=row_of(state))

            def streamed(with_best=True, collect_every=0):
                tok, src, state, n = dec.stream_begin(B, N, LB + CH + 2)
                seen["released"], seen["live"] = [], []
                for c in range(T // CH):
                    off = (np.arange(B, dtype=np.int64) * T + c * CH) * N
                    for _ in range(dec.append(None, chunk_T, offsets=off, device_ptr=em.data_ptr())):
                        tok, src, state, n = dec.step(log_probs, lm_row_of=row_of(state))
                    dec.prune(LB)
                    if collect_every and (c + 1) % collect_every == 0:
                        _, n_rel, n_live = dec.collect(a.release_cap)
                        seen["released"].append(n_rel)
                        seen["live"].append(n_live)
                    if with_best:
                        seen["best_len"] = len(dec.best(0, 0).tokens)
                    if with_best == "all" and c == 0:
                        t0 = time.perf_counter()
                        for b in range(B):
                            dec.best(b, 0)
                        seen["best_all_ms"] = (time.perf_counter() - t0) * 1e3
                dec.end(log_probs, lm_row_of=row_of(state))
            out = {}
            if "offline" in only:
                for _ in range(a.warmup):
                    offline()
                runs = [timed(offline, stream) / T for _ in range(a.repeat)]
                out["offline_ms_per_frame"] = {"median": statistics.median(runs), "min": min(runs), "max": max(runs)}
                out["offline_hyps_utt0"] = len(dec.results(0))
            if "stream" in only:
                for _ in range(a.warmup):
                    streamed()
                runs = [timed(streamed, stream) / T for _ in range(a.repeat)]
                out["stream_ms_per_frame"] = {"median": statistics.median(runs), "min": min(runs), "max": max(runs)}
                runs = [timed(lambda: streamed(False), stream) / T for _ in range(a.repeat)]
                out["stream_no_best_ms_per_frame"] = {"median": statistics.median(runs), "min": min(runs),
                                                      "max": max(runs)}
                hyps = dec.results(0)
                out["stream_hyps_utt0"], out["stream_final_len_utt0"] = len(hyps), len(hyps[0].tokens)
                out["best_len_utt0"] = seen.get("best_len")
                streamed("all")
                out["best_all_streams_ms"] = seen.get("best_all_ms")
                out["stream_begin_ms"] = timed(lambda: dec.stream_begin(B, N, LB + CH + 2), stream)
                out["stream_begin_default_ms"] = begin_default
                for ce in [int(x) for x in a.collect_every.split(",") if x]:
                    streamed(True, ce)
                    runs = [timed(lambda: streamed(True, ce), stream) / T for _ in range(a.repeat)]
                    med = statistics.median(runs)
                    out.setdefault("stream_collect_ms_per_frame", {})[ce] = {"median": med, "min": min(runs),
                                                                             "max": max(runs)}
                    calls = (T // CH) // ce
                    out.setdefault("collect_added_ms_per_call", {})[ce] = \
                        (med - out["stream_ms_per_frame"]["median"]) * T / max(calls, 1)
                    stream.synchronize()
                    out.setdefault("collect_released_total", {})[ce] = int(sum(int(r.sum()) for r in seen["released"]))
                    out.setdefault("collect_max_live", {})[ce] = int(max(int(v.max()) for v in seen["live"]))
                    out.setdefault("collect_max_released_one_stream", {})[ce] = \
                        int(max(int(r.max()) for r in seen["released"]))
            if "offline" in only and "stream" in only:
                out["ratio"] = out["stream_ms_per_frame"]["median"] / out["offline_ms_per_frame"]["median"]
                out["ratio_no_best"] = out["stream_no_best_ms_per_frame"]["median"] / out["offline_ms_per_frame"]["median"]
            dec.close()
            print(json.dumps({"config": {"name": name, "kind": kind, "B": B, "K": K, "Kt": Kt, "N": N, "T": T,
                                         "chunk": CH, "look_back": LB, "lm_width": W, "lm_table_rows": a.ctx,
                                         "max_states": a.max_states or K * T + 2, "release_cap": a.release_cap},
                              **out}),
                  flush=True)
            lm.close()
            if trie is not None:
                trie.close()
            del log_probs
            torch.cuda.empty_cache()
        del em
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
