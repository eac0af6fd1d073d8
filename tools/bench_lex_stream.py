"""Lexicon stream chunks: the generic frame loop against a lane engine's stream kernel -- --shape C3 (the default):
"xstream" = 0 against 1 (fltx_xlane.h); --shape C4: "ystream" = 0 against 1 (fltx_ylane.h, the LM terms), on bench.py's C4
workload (the trie with label scores, the synthetic 4-gram, lm_weight 2, word_score 2, sil_score -1, beam 100, token beam
29, T = 1500 unless --T says otherwise); --shape WP: "wstream" = 0 against 1 (fltx_wlane.h) on bench.py's WP workload
(LexiconFreeDecoder + ZeroLM over 1 024 word pieces, beam 50, token beam 50, T = 1000); --shape WP --ngram ORDER:
"wtstream" = 0 against 1 on the same shape with a synthetic token n-gram LM of that order (text_amd/ngram_synth.py,
seed 11) and lm_weight 0.8; --stats adds the (lane, position) pairs the LM filter dropped and the score memo's hit rate,
summed over the streams and chunks (a run of its own with the phase clocks on, not a timed one).  Below, `xstream`
stands for the shape's tunable.

The shape bench.py streams as C3 (its workload table: LexiconDecoder + ZeroLM over the 90k-word trie, CTC, N = 29,
beam 50, token beam 10): --B = 256 streams of --T = 1000 frames in --chunk = 50-frame chunks from host memory,
stream_prune(0) after every chunk, a buffer of 4 chunks + 8 frames, "stream_total_frames" = T.  The two settings are
timed alternately in one process, --repeat = 3 times each after one warm-up stream of each; the clock is the host's,
from stream_begin to a synchronise after stream_end.  One JSON line per run:
  `xstream`, `chosen` (positions per token wave of the chunks' kernel, 0 = the generic loop), `frames_per_s`, `ms`,
  `stream_redone`, `nbest_equal` (the final n-best of a seeded sample of streams, compared with the first run of the
  other setting: must be true)
and a last line with each setting's median, min and max and the ratio of the medians.

    python tools/bench_lex_stream.py [--shape C3|C4|WP] [--B 256] [--T 1000] [--chunk 50] [--repeat 3] [--sample 16]
                                      [--ngram ORDER] [--stats]
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

from text_amd import _capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--shape", choices=["C3", "C4", "WP"], default="C3")
    ap.add_argument("--T", type=int, default=None, help="frames per stream (C3: 1000, C4: 1500)")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--ngram", type=int, default=0, help="--shape WP: a token n-gram LM of this order (\"wtstream\")")
    ap.add_argument("--stats", action="store_true", help="--ngram: filter and memo counters of the last chunk")
    a = ap.parse_args()
    c4, wp = a.shape == "C4", a.shape == "WP"
    if a.ngram and not wp:
        raise SystemExit("--ngram goes with --shape WP")
    key = ("wtstream" if a.ngram else "wstream") if wp else ("ystream" if c4 else "xstream")
    B, T, CH, N = a.B, a.T or (1500 if c4 else 1000), a.chunk, 1024 if wp else 29
    K, Kt = (50, 50) if wp else ((100, 29) if c4 else (50, 10))
    lexicon = None if wp else synth.lexicon()
    W = 0 if wp else len(lexicon[1]) - 1
    e_host = synth.batch("ctc" if wp else "lexspell", B, T, N, lexicon=lexicon, u0=0)
    ctx = _capi.Context(device=0)
    wscore = np.zeros(W, dtype=np.float32)
    if c4:  # (as bench.py sets C4 up: trie label scores = lm.score(start, word))
        from bench import synthetic_arpa
        arpa = synthetic_arpa(W)
        lm = _capi.ArpaLM(arpa[0], arpa[1])
        opt = _capi.make_options(K, Kt, 25.0, 2.0, 2.0, float("-inf"), -1.0, False, "ctc")
        wscore = np.array([lm.score_sequence([w], False)[0][0] for w in range(W)], dtype=np.float32)
    elif a.ngram:
        import tempfile
        from text_amd import ngram_synth
        vocab = ngram_synth.words(N, "t")
        with tempfile.TemporaryDirectory() as tmp:
            ngram_synth.write_arpa(os.path.join(tmp, "lm.arpa"), vocab, a.ngram, (0, 3000, 1500, 800), 11)
            lm = _capi.ArpaLM(os.path.join(tmp, "lm.arpa"), vocab)
        opt = _capi.make_options(K, Kt, 25.0, 0.8, 0.0, float("-inf"), 0.0, False, "ctc")
    else:
        lm = _capi.ZeroLM(ctx)
        opt = _capi.make_options(K, Kt, 25.0, 0.0, 0.0, float("-inf"), 0.0, False, "ctc")
    trie = None
    if not wp:
        ht = _capi.HostTrie(N, 0)
        ht.insert_many(lexicon[0], lexicon[1], np.arange(W), wscore)
        ht.smear(1)
        trie = ht.upload(ctx)
    nchunk = T // CH
    pieces = [np.ascontiguousarray(e_host[:, k * CH:(k + 1) * CH, :]) for k in range(nchunk)]
    Tc = np.full(B, CH, dtype=np.int32)
    sample = sorted(np.random.RandomState(4242).choice(B, min(a.sample, B), replace=False).tolist())
    decs = {}
    for x in (0, 1):
        if wp:
            d = decs[x] = _capi.BatchDecoder(ctx, _capi.LEXFREE, opt, lm, 0, N - 1)
        else:
            d = decs[x] = _capi.BatchDecoder(ctx, _capi.LEXICON, opt, lm, 0, N - 1, unk=W, trie=trie)
        d.set("stream_total_frames", T)
        d.set(key, x)

    def run(x):
        d = decs[x]
        ctx.synchronize()
        t0 = time.perf_counter()
        d.stream_begin(B, N, 4 * CH + 8)
        chosen = int(d.get(key))
        for p in pieces:
            d.stream_step(p, Tc)
            d.stream_prune(0)
        d.stream_end()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        nbest = [[(h.score, list(h.tokens), list(h.words)) for h in d.results(b)] for b in sample]
        return dt, chosen, int(d.get("stream_redone")), nbest

    first, rates = {}, {0: [], 1: []}
    for rep in range(a.repeat + 1):  # (the first round warms up: buffers are allocated and code objects loaded in it)
        for x in (0, 1):
            dt, chosen, redone, nbest = run(x)
            first.setdefault(x, nbest)
            if not rep:
                continue
            rates[x].append(B * nchunk * CH / dt)
            print(json.dumps({key: x, "chosen": chosen, "frames_per_s": rates[x][-1], "ms": dt * 1e3,
                              "stream_redone": redone, "nbest_equal": nbest == first[1 - x] if (1 - x) in first else None}),
                  flush=True)
    med = {x: statistics.median(v) for x, v in rates.items()}
    print(json.dumps({"config": {"shape": a.shape, "B": B, "T": T, "chunk": CH, "K": K, "Kt": Kt, "N": N, "words": W, "repeat": a.repeat,
                                 "sample": sample},
                      key + "_0": {"median": med[0], "min": min(rates[0]), "max": max(rates[0])},
                      key + "_1": {"median": med[1], "min": min(rates[1]), "max": max(rates[1])},
                      "ratio": med[1] / med[0], "nbest_equal": first[0] == first[1]}), flush=True)
    if a.stats and a.ngram:
        d = decs[1]
        d.set("profile", 1)
        d.stream_begin(B, N, 4 * CH + 8)
        tot = np.zeros(4, dtype=np.int64)
        for p in pieces:
            d.stream_step(p, Tc)
            d.stream_prune(0)
            pr = [int(x) for x in d.profile()]  # (summed over the streams: 32-bit halves that stay apart at these sizes)
            tot += [pr[6] & 0xFFFFFFFF, pr[6] >> 32, pr[7] & 0xFFFFFFFF, pr[7] >> 32]
        d.stream_end()
        print(json.dumps({"pairs": int(tot[0]), "filter_dropped": int(tot[1]), "look_ups": int(tot[2]), "memo_hits": int(tot[3]),
                          "memo_hit_rate": float(tot[3]) / max(1, int(tot[2]))}), flush=True)
    for d in decs.values():
        d.close()
    if trie is not None:
        trie.close()
    lm.close()
    ctx.close()
    if first[0] != first[1]:
        raise SystemExit("the two settings' n-best differ")


if __name__ == "__main__":
    main()
