"""Lexicon seq2seq decoder step (text_amd/csrc/fltx_s2s_lex.h) next to the lexicon-free step at the same shapes.

One JSON line per configuration: B = 256 utterances, beam K = 50, token beam Kt = 50, 50 steps; V = 29 with a 50k-word
synthetic letter lexicon and V = 10 000 with a 50k-word word-piece lexicon, each with ZeroLM and with a word 3-gram
(lmWeight 0.5, wordScore 0.2, smearing MAX).  The "model" is a set of score tensors generated before the clock starts
(cycled over the steps), so only the decoder is timed; eos = V (never proposed) keeps the beams live.  Times are device
events on the stream both decoders run on, after a warm-up.  The front-end / step split comes from a separate run
under `rocprofv3 --kernel-trace --stats`.  The lexicons and ARPA files go to --out (default tools/bench_lex_s2s_out).

    python tools/bench_lex_s2s.py [--steps 50] [--warmup 3] [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text_amd import _capi, ngram_synth  # noqa: E402


def lexicon(V, n_words, seed, word_piece):
    """n_words distinct spellings: letter words of 2-10 tokens (V = 29), or word-piece words of 1-4 pieces."""
    g = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n_words:
        n = int(g.integers(1, 5)) if word_piece else int(g.integers(2, 11))
        toks = tuple(int(x) for x in g.integers(0, V, size=n))
        if toks not in seen:
            seen.add(toks)
            out.append(toks)
    return out


def device_loop(dec, scores, B, V, steps):
    dec.begin(B, V)
    for t in range(steps):
        dec.step(scores[t % len(scores)])


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
    ap.add_argument("--words", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list of config names to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "tools", "bench_lex_s2s_out"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    zero = _capi.ZeroLM(ctx)
    B, K, Kt = a.B, a.K, a.Kt
    vocab = ngram_synth.words(a.words, "w")
    arpa = os.path.join(a.out, "w%d_3gram.arpa" % a.words)
    if not os.path.exists(arpa):
        ngram_synth.write_arpa(arpa, vocab, 3, (0, 200000, 100000), 1)
    ngram = _capi.ArpaLM(arpa, vocab)
    for name, V, wp in (("letters", 29, False), ("word_piece", 10000, True)):
        spell = lexicon(V, a.words, 7, wp)
        with open(os.path.join(a.out, "%s_%d.lex" % (name, a.words)), "w") as f:
            for w, toks in enumerate(spell):
                f.write("w%d %s\n" % (w, " ".join(map(str, toks))))
        trie = _capi.HostTrie(V, 0)
        g = np.random.default_rng(3)
        for w, toks in enumerate(spell):
            trie.insert(toks, w, float(np.float32(-g.random() * 5)))
        trie.smear(1)
        scores = [torch.randn(B * K, V, device="cuda").log_softmax(-1) for _ in range(4)]
        free = _capi.Seq2SeqBatchDecoder(ctx, _capi.make_s2s_options(K, Kt, 1e9), zero, V, a.steps + 1)
        for _ in range(a.warmup):
            device_loop(free, scores, B, V, a.steps)
        ms_free = timed(lambda: device_loop(free, scores, B, V, a.steps), stream) / a.steps
        free.close()
        for lmname, lm in (("zero", zero), ("3gram", ngram)):
            cfg = "%s_%s" % (name, lmname)
            if a.only and cfg not in a.only.split(","):
                continue
            opts = _capi.make_s2s_lex_options(K, Kt, 1e9, 0.5, 0.2)
            dec = _capi.LexiconSeq2SeqBatchDecoder(ctx, opts, trie, lm, V, a.steps + 1)
            for _ in range(a.warmup):
                device_loop(dec, scores, B, V, a.steps)
            ms = timed(lambda: device_loop(dec, scores, B, V, a.steps), stream) / a.steps
            info = dec.info()
            dec.end()
            res = dec.results(0)
            print(json.dumps({"config": {"name": cfg, "B": B, "K": K, "Kt": Kt, "V": V, "words": a.words,
                                         "steps": a.steps},
                              "lexicon_ms_per_step": ms, "lexicon_free_ms_per_step": ms_free,
                              "trie_nodes": info["nodes"], "trie_bytes": info["trie_bytes"],
                              "merges_utt0": info["merges"][0], "hyps_utt0": len(res)}), flush=True)
            dec.close()


if __name__ == "__main__":
    main()
