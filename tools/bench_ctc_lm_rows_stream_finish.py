"""fltx_ctc_rows_stream_finish: device time of finishing and restarting streams of a CTC rows stream batch.

One JSON line per (token set, kind, max_states): B = 256 streams, beam K = 50, lmWeight 0.7, random float32 log-softmax
emissions in HBM -- the shapes, LM and lexicons of bench_ctc_lm_rows_stream.py.  Letters: N = 29, Kt = 29; word pieces:
N = 10 000, Kt = 50.  Kinds: `lexfree` and `lexicon` (word LM).  max_states: K * T + 2 (T = 200, what the offline path
would size) and the default of 65 536 ids per stream, whose table slice of about 1.5 MB the finish of a stream clears.
Every measurement starts from the same state: stream_begin, one chunk of --frames = 20 frames stepped, prune(10).  Device
events around the calls, --repeat = 3 runs each (median, min, max in ms), the variants taken in turn:
  `finish_all_ms`      stream_finish naming all B streams, results left on the device
  `end_begin_ms`       the pair it replaces on that state: end() followed by stream_begin()
  `finish_1_ms`, `finish_16_ms`, `finish_0_ms`   stream_finish naming 1, 16 and none of the streams
The share of the table clear is what a figure at the default max_states has over the same figure at K * T + 2.

    python tools/bench_ctc_lm_rows_stream_finish.py [--sets letters,word_piece] [--kinds lexfree,lexicon] [--repeat 3]
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
from bench_lex_ctc_lm_rows import lexicons  # noqa: E402
from bench_lex_s2s import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--look-back", type=int, default=10)
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sets", default="letters,word_piece")
    ap.add_argument("--kinds", default="lexfree,lexicon")
    a = ap.parse_args()
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    B, K, T, CH, LB = a.B, a.K, a.T, a.frames, a.look_back
    for name, N, Kt, sil, blank in (("letters", 29, 29, 0, 28), ("word_piece", 10000, 50, 0, 1)):
        if name not in a.sets.split(","):
            continue
        em = torch.randn(B * CH, N, device="cuda").log_softmax(-1).contiguous()
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

            def row_of(state):  # one LM row per (stream, state id); padding rows (-1) stay out of range
                r = (state.to(torch.int64) * 2654435761 + utt) % a.ctx
                return torch.where(state >= 0, r, torch.full_like(r, -1)).to(torch.int32)
            for max_states in (K * T + 2, 65536):
                if lex:
                    dec = _capi.LexiconCtcRowsBatchDecoder(ctx, opts, trie, lm, sil, blank, -1, False)
                else:
                    dec = _capi.CtcRowsBatchDecoder(ctx, opts, lm, sil, blank)
                dec.set_max_states(max_states)

                def state_s():
                    """the state every measurement starts from -> the lm_row_of of its last list"""
                    tok, src, state, n = dec.stream_begin(B, N, LB + CH + 2)
                    for _ in range(dec.append(None, chunk_T, device_ptr=em.data_ptr())):
                        tok, src, state, n = dec.step(log_probs, lm_row_of=row_of(state))
                    dec.prune(LB)
                    return row_of(state)

                def finish(n_named):
                    which = np.zeros(B, np.int32)
                    which[:n_named] = 1
                    return lambda ro: dec.stream_finish(which, log_probs, lm_row_of=ro, device=True)

                def pair(ro):
                    dec.end(log_probs, lm_row_of=ro)
                    dec.stream_begin(B, N, LB + CH + 2)
                variants = {"finish_all_ms": finish(B), "end_begin_ms": pair, "finish_16_ms": finish(16),
                            "finish_1_ms": finish(1), "finish_0_ms": finish(0)}
                runs = {k: [] for k in variants}
                for rep in range(a.repeat + 1):  # (the first round warms up: buffers are allocated in it)
                    for k, fn in variants.items():
                        ro = state_s()
                        ms = timed(lambda: fn(ro), stream)
                        if rep:
                            runs[k].append(ms)
                out = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in runs.items()}
                dec.close()
                print(json.dumps({"config": {"name": name, "kind": kind, "B": B, "K": K, "Kt": Kt, "N": N,
                                             "frames": CH, "look_back": LB, "lm_width": W, "max_states": max_states},
                                  **out}), flush=True)
            lm.close()
            if trie is not None:
                trie.close()
            del log_probs
            torch.cuda.empty_cache()
        del em
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
