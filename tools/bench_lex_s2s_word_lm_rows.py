"""Lexicon seq2seq step with a word-level LM: word rows (fltx_s2s_step_word_lm_rows) next to word n-gram tables.

One JSON line per lexicon at the shapes of tools/bench_lex_s2s.py: B = 256 utterances, beam K = 50, token beam Kt = 50,
50 steps, lmWeight 0.5, wordScore 0.2, eos = V (never proposed: the beams stay live); the letters lexicon at V = 29 and
the word-piece lexicon at V = 10 000, 50k synthetic words each, so lm_width = 50 000 (+ 1: the finish entry).  Four legs
on the same model rows (float32 log-probs, generated before the clock starts and cycled over the steps):
  (a) a synthetic word 3-gram as n-gram tables (fltx_s2s_step) -- what a caller can do without this step;
  (b) word rows, bf16 log-probs, one LM row per decoder row (identity lm_row_of);
  (c) the same rows through lm_row_of, kept by the caller's recipe on the device: a row that ended no word names the LM
      row its source row named, a row that ended a word gets the row of its own index (the torch gather / where that
      builds lm_row_of runs on the timed stream: it is part of the recipe);
  (d) the rows of (b) as bf16 logits (the step takes each named row's log-softmax itself).
The LM rows are random, not the 3-gram's: the legs take different search paths, so the comparison is of cost per step at
the same shapes, not of results.  Times are device events on the decoder's stream, after a warm-up.  The split into front
end, word gather and step kernel comes from a separate run under `rocprofv3 --kernel-trace --stats` (the program after
`--`; --only keeps that run to one leg).  The ARPA file goes to --out.

    python tools/bench_lex_s2s_word_lm_rows.py [--steps 50] [--warmup 3] [--only a,b,c,d] [--lex letters,word_piece]
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
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--lex", default="letters,word_piece")
    ap.add_argument("--out", default=os.path.join(ROOT, "tools", "bench_lex_s2s_out"))
    a = ap.parse_args()
    only = set(a.only.split(","))
    os.makedirs(a.out, exist_ok=True)
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    B, K, Kt, W = a.B, a.K, a.Kt, a.words + 1
    BK = B * K
    lm_logits = lm_lp = None
    if only & {"b", "c", "d"}:
        lm_logits = [(torch.randn(BK, W, device="cuda") * 3).to(torch.bfloat16) for _ in range(2)]
        if only & {"b", "c"}:
            lm_lp = [torch.log_softmax(x.float(), -1).to(torch.bfloat16) for x in lm_logits]
    ngram = None
    if "a" in only:
        vocab = ngram_synth.words(a.words, "w")
        arpa = os.path.join(a.out, "w%d_3gram.arpa" % a.words)
        if not os.path.exists(arpa):
            ngram_synth.write_arpa(arpa, vocab, 3, (0, 200000, 100000), 1)
        ngram = _capi.ArpaLM(arpa, vocab)
    rows = _capi.WordRowsLM(W, None, a.words)
    own = torch.arange(BK, device="cuda", dtype=torch.int32)
    for name, V, wp in (("letters", 29, False), ("word_piece", 10000, True)):
        if name not in a.lex.split(","):
            continue
        trie = _capi.HostTrie(V, 0)
        g = np.random.default_rng(3)
        for w, toks in enumerate(lexicon(V, a.words, 7, wp)):
            trie.insert(toks, w, float(np.float32(-g.random() * 5)))
        trie.smear(1)
        model = [torch.randn(BK, V, device="cuda").log_softmax(-1) for _ in range(4)]
        opts = _capi.make_s2s_lex_options(K, Kt, 1e9, 0.5, 0.2)
        st = {}

        def step_a(d, t):
            d.step(model[t % 4])

        def step_b(d, t):
            d.step(model[t % 4], lm_scores=lm_lp[t % 2])

        def step_c(d, t):  # the caller's recipe for lm_row_of, from next_src_row and next_word alone
            if t == 0:
                st["row_of"] = torch.zeros(BK, device="cuda", dtype=torch.int32)
            else:
                src, word = st["out"][2].reshape(-1), st["out"][4].reshape(-1)
                kept = st["row_of"].gather(0, src.clamp(min=0).long())
                st["row_of"] = torch.where(word >= 0, own, kept)
            st["out"] = d.step(model[t % 4], lm_scores=lm_lp[t % 2], lm_row_of=st["row_of"])

        def step_d(d, t):
            d.step(model[t % 4], lm_scores=lm_logits[t % 2], lm_kind="logits")
        legs = {}
        if "a" in only:
            legs["a_word_3gram_tables"] = (ngram, step_a)
        if "b" in only:
            legs["b_word_rows_bf16_log_probs"] = (rows, step_b)
        if "c" in only:
            legs["c_word_rows_one_row_per_state"] = (rows, step_c)
        if "d" in only:
            legs["d_word_rows_bf16_logits"] = (rows, step_d)
        ms, extra = {}, {}
        for leg, (lm, step) in legs.items():
            dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, opts, trie, lm, V, a.steps + 1, False)

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
            if leg.startswith("c_"):
                extra[leg]["distinct_lm_rows_last_step"] = int(torch.unique(st["row_of"]).numel())
            dec.close()
        print(json.dumps({"config": {"name": name, "B": B, "K": K, "Kt": Kt, "V": V, "words": a.words, "steps": a.steps,
                                     "is_lm_token": False, "lm_width": W, "lm_weight": 0.5, "word_score": 0.2},
                          "ms_per_step": ms, "search": extra,
                          "bytes_per_step": {"model_f32_rows": BK * V * 4, "lm_bf16_rows": BK * W * 2}}), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
