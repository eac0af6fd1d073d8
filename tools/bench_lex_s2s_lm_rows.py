"""Lexicon seq2seq step with a token LM (is_lm_token): the rows LM (fltx_s2s_step_lm_rows) next to token n-gram tables.

One JSON line per lexicon at the shapes of tools/bench_lex_s2s.py: B = 256 utterances, beam K = 50, token beam Kt = 50,
50 steps, lmWeight 0.5, wordScore 0.2, eos = V (never proposed: the beams stay live); the letters lexicon at V = 29 and
the word-piece lexicon at V = 10 000, 50k synthetic words each.  Three legs on the same model rows (float32 log-probs,
generated before the clock starts and cycled over the steps):
  (a) a synthetic token 3-gram as n-gram tables (fltx_s2s_step) -- what the decoder could do before, the yardstick;
  (b) a rows LM whose rows are bf16 log-probs, as wide as the model's (fltx_s2s_step_lm_rows);
  (c) the same as bf16 logits (the step takes each row's log-softmax itself).
The LM rows of (b) and (c) are random, not the 3-gram's: the legs take different search paths, so the comparison is of
cost per step at the same shapes, not of results.  Times are device events on the decoder's stream, after a warm-up.
The split into front end, gather and step kernel comes from a separate run under `rocprofv3 --kernel-trace --stats`
(the program after `--`; --only keeps that run to one leg).  The ARPA files go to --out.

    python tools/bench_lex_s2s_lm_rows.py [--steps 50] [--warmup 3] [--only a,b,c] [--lex letters,word_piece] [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi, ngram_synth  # noqa: E402
from bench_lex_s2s import lexicon, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--Kt", type=int, default=50)
    ap.add_argument("--words", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--lex", default="letters,word_piece")
    ap.add_argument("--out", default=os.path.join(ROOT, "tools", "bench_lex_s2s_out"))
    a = ap.parse_args()
    only = set(a.only.split(","))
    os.makedirs(a.out, exist_ok=True)
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    B, K, Kt = a.B, a.K, a.Kt
    for name, V, wp in (("letters", 29, False), ("word_piece", 10000, True)):
        if name not in a.lex.split(","):
            continue
        trie = _capi.HostTrie(V, 0)
        g = np.random.default_rng(3)
        for w, toks in enumerate(lexicon(V, a.words, 7, wp)):
            trie.insert(toks, w, float(np.float32(-g.random() * 5)))
        trie.smear(1)
        model = [torch.randn(B * K, V, device="cuda").log_softmax(-1) for _ in range(4)]
        lm_logits = [(torch.randn(B * K, V, device="cuda") * 3).to(torch.bfloat16) for _ in range(4)]
        lm_lp = [torch.log_softmax(x.float(), -1).to(torch.bfloat16) for x in lm_logits]
        opts = _capi.make_s2s_lex_options(K, Kt, 1e9, 0.5, 0.2)
        legs = {}
        if "a" in only:
            vocab = ngram_synth.words(V, "t")
            arpa = os.path.join(a.out, "t%d_3gram.arpa" % V)
            if not os.path.exists(arpa):
                ngram_synth.write_arpa(arpa, vocab, 3, (0, min(V * V, 200000), 100000), 1)
            ngram = _capi.ArpaLM(arpa, vocab)
            legs["a_token_3gram_tables"] = (ngram, lambda d, t: d.step(model[t % 4]))
        rows = _capi.RowsLM()
        if "b" in only:
            legs["b_rows_bf16_log_probs"] = (rows, lambda d, t: d.step(model[t % 4], lm_scores=lm_lp[t % 4]))
        if "c" in only:
            legs["c_rows_bf16_logits"] = (rows, lambda d, t: d.step(model[t % 4], lm_scores=lm_logits[t % 4],
                                                                     lm_kind="logits"))
        ms, extra = {}, {}
        for leg, (lm, step) in legs.items():
            dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, opts, trie, lm, V, a.steps + 1, True)

            def loop():
                dec.begin(B, V)
                for t in range(a.steps):
                    step(dec, t)
            for _ in range(a.warmup):
                loop()
            ms[leg] = timed(loop, stream) / a.steps
            info = dec.info()
            dec.end()
            extra[leg] = {"merges_utt0": info["merges"][0], "hyps_utt0": len(dec.results(0))}
            dec.close()
        print(json.dumps({"config": {"name": name, "B": B, "K": K, "Kt": Kt, "V": V, "words": a.words, "steps": a.steps,
                                     "is_lm_token": True, "lm_weight": 0.5, "word_score": 0.2},
                          "ms_per_step": ms, "search": extra,
                          "bytes_per_step": {"model_f32_rows": B * K * V * 4, "lm_bf16_rows": B * K * V * 2,
                                             "lm_entries_gathered": B * K * min(Kt, V)}}), flush=True)
        del model, lm_logits, lm_lp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
