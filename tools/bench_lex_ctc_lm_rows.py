"""Lexicon CTC with a rows LM (fltx_ctc_rows_lex_decoder_create): device time per frame step, next to the host-LM path
and to the lexicon-free rows step.

One JSON line per (token set, LM level): B = 256 utterances of T = 200 frames, beam K = 50, lmWeight 0.7, wordScore 0.5,
random float32 log-softmax emissions in HBM.  Letters: N = 29 (sil 0, blank 28), every token kept (Kt = 29), the
synthetic 90 000-word lexicon of the C3 workload (text_amd.synth.lexicon(90000, 4242), smeared with MAX over the LM's
start row); word pieces: N = 10 000, Kt = 50, 20 000 words of one to three pieces.  The LM is bench_ctc_lm_rows.py's
synthetic device LM: `--ctx` bf16 rows of lm_width entries (words + 1 for the word LM, N + 1 for the token LM; the last
one the finish entry), the row of a hypothesis a hash of its utterance and its next_state id, named through lm_row_of.
Legs on the same table: (a) bf16 log-probs, (b) bf16 logits; times are device events around begin + T steps + end after
a warm-up, divided by T, `begin_ms` on its own.
(c) the baseline, the parent's code: the same LM behind fltx_lm_host_create on FLTX_DECODER_LEXICON at --host-B
utterances (default 4) of the same emissions, wall time per frame of that smaller batch.
(d) the second yardstick, token LM only: the lexicon-free rows step (CtcRowsBatchDecoder) on the same emissions and
table; `ratio_to_lexfree` is (a) / (d).
The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` (the program after `--`; --only
and --levels keep that run to one leg).

--emissions DTYPE_KIND: the emissions as bench_ctc_lm_rows.py's option names them (default f32_log_probs); anything
else goes through fltx_ctc_rows_begin_typed, and the step reads its blank and same-node emissions from the typed frames.

    python tools/bench_lex_ctc_lm_rows.py [--T 200] [--warmup 1] [--only a,b,c,d] [--sets letters,word_piece]
                                          [--levels word,token] [--emissions bf16_logits]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from text_amd import _capi, synth  # noqa: E402
from bench_ctc_lm_rows import EMISSIONS, TableLM, emissions  # noqa: E402
from bench_lex_s2s import timed  # noqa: E402


def lexicons(name, N):
    """-> [spelling (int32 array)] per word id"""
    if name == "letters":
        sf, so = synth.lexicon(90000, 4242)
        return [sf[so[w]:so[w + 1]] for w in range(len(so) - 1)]
    r = np.random.RandomState(7)
    return [r.randint(2, N, size=1 + r.randint(3)).astype(np.int32) for _ in range(20000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--host-B", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--sets", default="letters,word_piece")
    ap.add_argument("--levels", default="word,token")
    ap.add_argument("--emissions", default="f32_log_probs", choices=EMISSIONS,
                    help="what begin is handed: dtype and kind of the emissions in HBM (bench_ctc_lm_rows.py)")
    a = ap.parse_args()
    only = set(a.only.split(","))
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    B, K, T = a.B, a.K, a.T
    for name, N, Kt, sil, blank in (("letters", 29, 29, 0, 28), ("word_piece", 10000, 50, 0, 1)):
        if name not in a.sets.split(","):
            continue
        spell = lexicons(name, N)
        em, begin = emissions(B * T, N, a.emissions)
        Ts = np.full(B, T, np.int32)
        utt = (torch.arange(B, device="cuda", dtype=torch.int64) * 97)[:, None]
        for level in a.levels.split(","):
            tokl = level == "token"
            W = (N if tokl else len(spell)) + 1
            logits = (torch.randn(a.ctx, W, device="cuda") * 3).to(torch.bfloat16)
            log_probs = torch.log_softmax(logits.float(), -1).to(torch.bfloat16)
            start_row = log_probs[0].float().cpu().numpy()
            trie = _capi.HostTrie(N, sil)
            for w, sp in enumerate(spell):
                trie.insert(sp, w, 0.0 if tokl else float(start_row[w]))
            trie.smear(1)
            lm = (_capi.RowsLM if tokl else _capi.WordRowsLM)(W, None, W - 1)
            opts = _capi.make_options(K, Kt, 25.0, 0.7, 0.5)
            ms, extra = {}, {}

            def row_of(state):  # one LM row per (utterance, state id); padding rows (-1) stay out of range
                r = (state.to(torch.int64) * 2654435761 + utt) % a.ctx
                return torch.where(state >= 0, r, torch.full_like(r, -1)).to(torch.int32)

            def run(dec, rows, kind):
                def loop():
                    tok, src, state, n = begin(dec, Ts)
                    for _ in range(T):
                        tok, src, state, n = dec.step(rows, lm_row_of=row_of(state), lm_kind=kind)
                    dec.end(rows, lm_row_of=row_of(state), lm_kind=kind)
                for _ in range(a.warmup):
                    loop()
                per = timed(loop, stream) / T
                begin_ms = timed(lambda: begin(dec, Ts), stream)
                loop()
                hyps = dec.results(0)
                dec.close()
                return per, {"begin_ms": begin_ms, "hyps_utt0": len(hyps), "best_utt0": hyps[0].score,
                             "words_utt0": int((hyps[0].words >= 0).sum())}
            for leg, rows, kind in (("a_bf16_log_probs", log_probs, "log_probs"), ("b_bf16_logits", logits, "logits")):
                if leg[0] in only:
                    ms[leg], extra[leg] = run(_capi.LexiconCtcRowsBatchDecoder(ctx, opts, trie, lm, sil, blank, -1, tokl),
                                              rows, kind)
            if "d" in only and tokl:
                ms["d_lexfree_rows_step"], extra["d_lexfree_rows_step"] = run(
                    _capi.CtcRowsBatchDecoder(ctx, opts, lm, sil, blank), log_probs, "log_probs")
                if "a_bf16_log_probs" in ms:
                    extra["ratio_to_lexfree"] = ms["a_bf16_log_probs"] / ms["d_lexfree_rows_step"]
            if "c" in only:
                hb = a.host_B
                host = _capi.HostLM(TableLM(log_probs.float().cpu().numpy(), a.ctx))
                dtrie = trie.upload(ctx)
                ref = _capi.BatchDecoder(ctx, _capi.LEXICON, opts, host, sil, blank, -1, trie=dtrie, is_lm_token=tokl)
                e_host = em[:hb * T].float().log_softmax(-1).cpu().numpy()
                ref.decode_batch(e_host, Ts[:hb], N)  # warm-up
                ref.count(0)
                t0 = time.perf_counter()
                ref.decode_batch(e_host, Ts[:hb], N)
                ref.count(0)
                ms["c_host_lm_path"] = (time.perf_counter() - t0) * 1e3 / T
                extra["c_host_lm_path"] = {"B": hb, "lm_calls": host.calls, "hyps_utt0": ref.count(0)[0]}
                ref.close()
                host.close()
            print(json.dumps({"config": {"name": name, "lm": level, "B": B, "K": K, "Kt": Kt, "N": N, "T": T,
                                         "words": len(spell), "trie_nodes": trie.num_nodes(), "lm_width": W,
                                         "lm_table_rows": a.ctx, "lm_weight": 0.7, "word_score": 0.5},
                              "ms_per_frame_step": ms, "search": extra,
                              "emissions": a.emissions,
                              "bytes": {"emissions": em.numel() * em.element_size(), "lm_bf16_table": a.ctx * W * 2}}), flush=True)
            lm.close()
            trie.close()
            del logits, log_probs
            torch.cuda.empty_cache()
        del em
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
