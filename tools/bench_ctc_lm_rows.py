"""Lexicon-free CTC with a rows LM (fltx_ctc_rows_*): device time per frame step, next to the host-LM path.

One JSON line per token set: B = 256 utterances of T = 200 frames, beam K = 50, lmWeight 0.7, random float32 log-softmax
emissions in HBM.  Letters: N = 29, every token kept (Kt = 29); word pieces: N = 10 000, Kt = 50.  The LM is a synthetic
device LM, a table lookup: `--ctx` rows of lm_width = N + 1 entries (the last one the finish entry), and the row of a
hypothesis is a hash of its utterance and its next_state id -- one row per LM state, named through lm_row_of, which a
few torch operations on the timed stream compute from the step's own output (they are part of the caller's recipe).
Two legs on the same table: (a) bf16 log-probs, (b) bf16 logits (the step takes each named row's log-softmax itself).
Times are device events on the decoder's stream around begin + T steps + end, after a warm-up, divided by T; `begin_ms`
(the emissions' token beams, once per batch) is timed on its own as well.
(c) the baseline: the same kind of LM served through the existing host-LM path (fltx_lm_host_create + fltx_decode_batch),
a Python object whose states are memoised children and whose scores are rows of the same table on the host.  That path
asks Python one question per distinct (state, token), so it runs at --host-B utterances (default 4) of the same
emissions; its figure is wall time per frame of that smaller batch.
(p) --plan: the same table behind the device planner (fltx_ctc_rows_plan): every list is planned, the rows new_row of a
bf16 store are filled from the table (the row the hash names for the new state's utterance and id) and the step reads
the store through the planner's lm_row_of -- fixed-shape torch operations, nothing read on the host.  The store of a
batch decode holds every state the decode can enter, B * (K * T + 2) rows; where that is more than --plan-store-gb the
leg runs as B streams instead -- chunks of --plan-chunk frames, a collect and plan_release after each, max_states 1024
per stream -- and says so ("mode").  --plan-read-counts: the leg reads the plan's counts every frame (16 bytes, a
synchronisation) and fills the n_new listed rows only, as a caller with wide LM rows would.
--emissions DTYPE_KIND (f32 / f16 / bf16, log_probs / logits; default f32_log_probs, the float32 entry points) feeds the
legs a, b and p the acoustic model's output as it is, through fltx_ctc_rows_begin_typed.
--front N1,N2,..: the front end alone, on --front-dtype logits of B * T frames per width in HBM -- (typed) the typed
begin; (torch) what a caller did before it: .float().log_softmax(-1), then fltx_ctc_rows_begin -- in alternating runs,
medians with their spread, and the device bytes each holds at its peak (what the driver reports used after the call
above an emptied cache before it: the caching allocator keeps torch's high-water mark, the decoder its buffers).
--front-sweep N1,N2,..: the typed begin per width with the wave-per-frame and with the workgroup-per-frame front end
(fltx_decoder_set "emissions_narrow_max"), alternating: what the switch-over width was chosen from.
The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` (the program after `--`; --only
keeps that run to one leg).

    python tools/bench_ctc_lm_rows.py [--T 200] [--warmup 1] [--only a,b,c] [--sets letters,word_piece] [--plan]
                                      [--emissions bf16_logits] [--front 29,1024,8192] [--front-sweep 29,64,...]
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

from text_amd import _capi  # noqa: E402
from bench_lex_s2s import timed  # noqa: E402


TORCH_DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EMISSIONS = ["%s_%s" % (d, k) for d in TORCH_DTYPES for k in ("log_probs", "logits")]


def emissions(frames, N, spec):
    """[frames, N] emissions in HBM as `spec` names them -> (the tensor, begin(dec, Ts) that hands them to a decoder)"""
    dt, kind = spec.split("_", 1)
    x = torch.randn(frames, N, device="cuda")
    em = (x.log_softmax(-1) if kind == "log_probs" else x * 3).to(TORCH_DTYPES[dt]).contiguous()
    if spec == "f32_log_probs":  # the float32 entry points, as before
        return em, lambda dec, Ts, **kw: dec.begin(None, Ts, N, device_ptr=em.data_ptr(), **kw)
    return em, lambda dec, Ts, **kw: dec.begin(em, Ts, N, kind=kind, **kw)


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def front_end(a, ctx, stream, widths, sweep):
    """--front / --front-sweep: see the module's text"""
    B, T = a.B, a.T
    Ts = np.full(B, T, np.int32)
    dt = TORCH_DTYPES[a.front_dtype]

    def held(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info()[0]
        fn()
        torch.cuda.synchronize()
        return free0 - torch.cuda.mem_get_info()[0]
    for N in sorted(set(widths) | set(sweep)):
        lm = _capi.RowsLM(N + 1, None, N)
        opts = _capi.make_options(a.K, min(N, 50), 25.0, 0.7)
        x = (torch.randn(B * T, N, device="cuda") * 3).to(dt)
        out = {"config": {"N": N, "B": B, "T": T, "dtype": a.front_dtype, "kind": "logits", "runs": a.front_runs,
                          "emissions_bytes": x.numel() * x.element_size()}}
        if N in widths:
            def typed(dec):
                dec.begin(x, Ts, N, kind="logits")

            def torch_then_f32(dec):
                e = x.float().log_softmax(-1)
                dec.begin(None, Ts, N, device_ptr=e.data_ptr())
                return e
            legs = {"typed_begin": typed, "torch_log_softmax_then_begin": torch_then_f32}
            ms, mem = {k: [] for k in legs}, {}
            for k, fn in legs.items():  # a fresh decoder per leg: its buffers are part of what the leg holds
                dec = _capi.CtcRowsBatchDecoder(ctx, opts, lm, 0, 1)
                mem[k] = held(lambda: fn(dec))
                dec.close()
            decs = {k: _capi.CtcRowsBatchDecoder(ctx, opts, lm, 0, 1) for k in legs}
            for k, fn in legs.items():
                fn(decs[k])
            for _ in range(a.front_runs):
                for k, fn in legs.items():
                    ms[k].append(timed(lambda: fn(decs[k]), stream))
            out["begin_ms"] = {k: spread(v) for k, v in ms.items()}
            out["device_bytes_held"] = mem
            for d in decs.values():
                d.close()
        if N in sweep and N <= 1024:
            decs = {}
            for k, nm in (("wave_per_frame", 1024), ("workgroup_per_frame", 0)):
                decs[k] = _capi.CtcRowsBatchDecoder(ctx, opts, lm, 0, 1)
                decs[k].set("emissions_narrow_max", nm)
                decs[k].begin(x, Ts, N, kind="logits")
            ms = {k: [] for k in decs}
            for _ in range(a.front_runs):
                for k, d in decs.items():
                    ms[k].append(timed(lambda: d.begin(x, Ts, N, kind="logits"), stream))
            out["sweep_begin_ms"] = {k: spread(v) for k, v in ms.items()}
            for d in decs.values():
                d.close()
        print(json.dumps(out), flush=True)
        lm.close()
        del x
        torch.cuda.empty_cache()


class TableLM:
    """The host twin for the host-LM path: a state is a memoised child per token; its row is a hash of its id."""

    class State:
        __slots__ = ("kids", "row")

        def __init__(self, row):
            self.kids, self.row = {}, row

    def __init__(self, table, n_ctx):
        self.table, self.n_ctx, self.made = table, n_ctx, 0

    def start(self, _nothing):
        return self.State(0)

    def _child(self, st, idx):
        k = st.kids.get(idx)
        if k is None:
            self.made += 1
            k = st.kids[idx] = self.State((self.made * 2654435761) % self.n_ctx)
        return k

    def score(self, st, idx):
        return self._child(st, idx), float(self.table[st.row, idx])

    def finish(self, st):
        return self._child(st, -1), float(self.table[st.row, -1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--host-B", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--sets", default="letters,word_piece")
    ap.add_argument("--plan", action="store_true", help="add leg p: the device planner in the place of the hash recipe")
    ap.add_argument("--plan-store-gb", type=float, default=8.0)
    ap.add_argument("--plan-chunk", type=int, default=10)
    ap.add_argument("--plan-read-counts", action="store_true",
                    help="leg p reads the plan's counts (16 bytes, a synchronisation per frame) and fills n_new rows only")
    ap.add_argument("--emissions", default="f32_log_probs", choices=EMISSIONS,
                    help="what the legs a, b and p hand to begin: dtype and kind of the emissions in HBM")
    ap.add_argument("--front", default="", help="widths N1,N2,..: time the front end alone, typed against torch + float32")
    ap.add_argument("--front-sweep", default="", help="widths N1,N2,..: wave-per-frame against workgroup-per-frame")
    ap.add_argument("--front-dtype", default="bf16", choices=sorted(TORCH_DTYPES))
    ap.add_argument("--front-runs", type=int, default=9)
    a = ap.parse_args()
    only = set(a.only.split(",")) | ({"p"} if a.plan else set())
    torch.manual_seed(0)
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL: a context given NULL makes its own stream)
    torch.cuda.set_stream(stream)
    ctx = _capi.Context(stream=stream.cuda_stream)
    B, K, T = a.B, a.K, a.T
    if a.front or a.front_sweep:
        front_end(a, ctx, stream, [int(n) for n in a.front.split(",") if n], [int(n) for n in a.front_sweep.split(",") if n])
        return
    for name, N, Kt in (("letters", 29, 29), ("word_piece", 10000, 50)):
        if name not in a.sets.split(","):
            continue
        W = N + 1
        em, begin = emissions(B * T, N, a.emissions)
        logits = (torch.randn(a.ctx, W, device="cuda") * 3).to(torch.bfloat16)
        log_probs = torch.log_softmax(logits.float(), -1).to(torch.bfloat16)
        Ts = np.full(B, T, np.int32)
        utt = (torch.arange(B, device="cuda", dtype=torch.int64) * 97)[:, None]
        lm = _capi.RowsLM(W, None, N)
        opts = _capi.make_options(K, Kt, 25.0, 0.7)
        ms, extra = {}, {}
        for leg, rows, kind in (("a_bf16_log_probs", log_probs, "log_probs"), ("b_bf16_logits", logits, "logits")):
            if leg[0] not in only:
                continue
            dec = _capi.CtcRowsBatchDecoder(ctx, opts, lm, 0, 1)

            def row_of(state):  # one LM row per (utterance, state id); padding rows (-1) stay out of range
                r = (state.to(torch.int64) * 2654435761 + utt) % a.ctx
                return torch.where(state >= 0, r, torch.full_like(r, -1)).to(torch.int32)

            def loop():
                tok, src, state, n = begin(dec, Ts)
                for _ in range(T):
                    tok, src, state, n = dec.step(rows, lm_row_of=row_of(state), lm_kind=kind)
                dec.end(rows, lm_row_of=row_of(state), lm_kind=kind)
            for _ in range(a.warmup):
                loop()
            ms[leg] = timed(loop, stream) / T
            begin_ms = timed(lambda: begin(dec, Ts), stream)
            loop()
            hyps = dec.results(0)
            extra[leg] = {"begin_ms": begin_ms, "hyps_utt0": len(hyps), "best_utt0": hyps[0].score}
            dec.close()
        if "p" in only:
            leg = "p_plan_bf16_log_probs"
            dec = _capi.CtcRowsBatchDecoder(ctx, opts, lm, 0, 1)
            batch = B * (K * T + 2) * W * 2 <= a.plan_store_gb * 2 ** 30
            max_states = 1024
            cap = B * (K * T + 2) if batch else B * max_states
            store = torch.zeros(cap + 1, W, device="cuda", dtype=torch.bfloat16)  # (the last row takes the padding)
            utt_of_row = (torch.arange(B * K, device="cuda", dtype=torch.int64) // K) * 97
            last = {}

            def planned(lists):
                p = dec.plan(*lists)
                n_new = int(p.counts[0]) if a.plan_read_counts else B * K
                dr = p.new_dec_row[:n_new].to(torch.int64).clamp_min(0)
                table_row = (lists[2].reshape(-1)[dr].to(torch.int64) * 2654435761 + utt_of_row[dr]) % a.ctx
                nr = p.new_row[:n_new].to(torch.int64)
                store[torch.where(nr >= 0, nr, torch.full_like(nr, cap))] = log_probs[table_row]
                last["counts"] = p.counts
                return p.lm_row_of

            def plan_loop():
                if batch:
                    lists = begin(dec, Ts)
                    dec.plan_begin(cap)
                    for _ in range(T):
                        lists = dec.step(store[:cap], lm_row_of=planned(lists))
                    dec.end(store[:cap], lm_row_of=planned(lists))
                    return
                dec.set_max_states(max_states)
                lists = dec.stream_begin(B, N, a.plan_chunk)
                dec.plan_begin(cap)
                ro = planned(lists)
                for t0 in range(0, T, a.plan_chunk):  # (utterance-major emissions: a chunk is named by its offsets)
                    n = min(a.plan_chunk, T - t0)
                    off = (np.arange(B, dtype=np.int64) * T + t0) * N
                    tn = np.full(B, n, np.int32)
                    for _ in range(dec.append(None, tn, offsets=off, device_ptr=em.data_ptr()) if a.emissions == "f32_log_probs"
                                   else dec.append(em, tn, offsets=off, kind=a.emissions.split("_", 1)[1])):
                        ro = planned(dec.step(store[:cap], lm_row_of=ro))
                    dec.prune(0)
                    rel, n_rel, _ = dec.collect(max_states)
                    dec.plan_release(rel, n_rel)
                dec.end(store[:cap], lm_row_of=ro)
            for _ in range(a.warmup):
                plan_loop()
            ms[leg] = timed(plan_loop, stream) / T
            plan_loop()
            hyps = dec.results(0)
            counts = last["counts"].cpu().tolist()
            extra[leg] = {"mode": "batch" if batch else "streams", "fill": "n_new rows" if a.plan_read_counts else "B*K rows",
                          "row_capacity": cap, "high_water": counts[1],
                          "n_dropped": counts[3], "hyps_utt0": len(hyps), "best_utt0": hyps[0].score}
            dec.close()
            del store
        if "c" in only:
            hb = a.host_B
            host = _capi.HostLM(TableLM(log_probs[:, :].float().cpu().numpy(), a.ctx))
            ref = _capi.BatchDecoder(ctx, _capi.LEXFREE, opts, host, 0, 1)
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
        print(json.dumps({"config": {"name": name, "B": B, "K": K, "Kt": Kt, "N": N, "T": T, "lm_width": W,
                                     "lm_table_rows": a.ctx, "lm_weight": 0.7, "emissions": a.emissions},
                          "ms_per_frame_step": ms, "search": extra,
                          "bytes": {"emissions": em.numel() * em.element_size(), "lm_bf16_table": a.ctx * W * 2}}),
              flush=True)
        lm.close()
        del em, logits, log_probs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
