#!/usr/bin/env python3
"""From batch to text, two ways, on the C2 and C4 bench shapes with HBM-resident emissions:

  (a) decode_batch + results_arrays_compact() + the NumPy collapse of every fetched hypothesis on the host
      (what callers did: keep where the token changes, drop blank, the indices are the timesteps);
  (b) decode_batch + transcripts(): the collapse on the device (text_amd/csrc/fltx_transcript.h).

At max_hyp = 1 and max_hyp = K.  (a) and (b) run alternately in one process, `--runs` runs of `--steps` batches each
after `--warmup`; per leg it prints the ms per batch of every run, the bytes that crossed PCIe for the results of one
batch, and -- from HIP events around them ("time_transcripts") -- the durations of the three kernels and of
fltx_pack_results_kernel, which reads the same rows when max_hyp = K.  One JSON line per (workload, max_hyp).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def host_collapse(r, dec, max_hyp, blank):
    """(a)'s host part: every fetched hypothesis' tokens, timesteps, words and word timesteps"""
    out = []
    nh, ln, off = r["n_hyp"].tolist(), r["length"].tolist(), r["offsets"].tolist()
    tok8, wrd = r["tokens_u8"], r["words"]
    for b in range(dec.B):
        L = ln[b]
        for i in range(min(nh[b], max_hyp)):
            a = off[b] + i * L
            t = tok8[a:a + L]
            keep = (t != 255) & (t != blank)
            keep[1:] &= t[1:] != t[:-1]
            ts = np.flatnonzero(keep)
            if wrd is not None:
                w = wrd[a:a + L]
                wt = np.flatnonzero(w >= 0)
                out.append((t[ts].astype(np.int32), ts, w[wt], wt))
            else:
                out.append((t[ts].astype(np.int32), ts, None, None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C2,C4")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import torch
    import bench
    torch.cuda.init()
    argv, sys.argv = sys.argv, ["bench.py", "--pipeline", "1"]  # bench.py's own defaults, one decoder object
    try:
        ns = bench.parse()
    finally:
        sys.argv = argv
    for wl in a.workloads.split(","):
        cfg = dict(bench.WORKLOADS[wl])
        B = a.batch or cfg["batch"]
        job = bench.Job(ns, 0, 0, B, cfg)
        dec = job.decoder()
        dec.set("time_transcripts", 1)
        K, N, T = job.K, job.N, job.T
        e_dev = torch.from_numpy(np.ascontiguousarray(job.e_host, dtype=np.float32)).cuda()
        torch.cuda.synchronize()
        blank = job.blank

        def decode():
            dec.decode_batch(None, job.Ts, N, device_ptr=e_dev.data_ptr())

        for mh in (1, K):
            info = {}

            def leg_a():
                decode()
                r = dec.results_arrays_compact()
                res = host_collapse(r, dec, mh, blank)
                total = int(r["offsets"][dec.B])
                info["a_bytes"] = total * (5 if r["words"] is not None else 1) + 24 * B * K + 12 * B
                info["a_rows"] = len(res)
                info["pack_us"] = dec.get("pack_ns") / 1e3
                return res

            def leg_b():
                decode()
                t = dec.transcripts(mh)
                n, nt, nw = t["n_rows"], t["n_tokens"], t["n_words"]
                info["b_bytes"] = 16 + 16 * (n + 1) + 8 * nt + 12 * nw + 24 * B * K + 12 * n
                info["b_rows"], info["b_tokens"], info["b_words"] = n, nt, nw
                info["kernels_us"] = [dec.get("transcript_%s_ns" % k) / 1e3 for k in ("count", "scan", "write")]
                return t

            # the same transcripts both ways, before anything is timed
            ra, tb = leg_a(), leg_b()
            assert len(ra) == tb["n_rows"] > 0, "the batch has no hypothesis"
            for q in (0, len(ra) // 2, len(ra) - 1):
                lo, hi = int(tb["tok_off"][q]), int(tb["tok_off"][q + 1])
                assert ra[q][0].tolist() == tb["tokens"][lo:hi].tolist() and ra[q][1].tolist() == tb["timesteps"][lo:hi].tolist()
            runs = {"a": [], "b": []}
            for run in range(a.runs):
                for name, leg in (("a", leg_a), ("b", leg_b)):
                    for _ in range(a.warmup):
                        leg()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        leg()
                    runs[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
            decode()
            dec.ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                decode()
                dec.count(0)  # (waits for the batch)
            decode_ms = (time.perf_counter() - t0) * 1e3 / a.steps
            print(json.dumps(dict(
                workload=wl, B=B, T=T, K=K, N=N, max_hyp=mh, steps=a.steps, runs=a.runs,
                decode_only_ms=round(decode_ms, 3),
                a_ms_per_batch=[round(x, 3) for x in runs["a"]], b_ms_per_batch=[round(x, 3) for x in runs["b"]],
                a_pcie_bytes=info["a_bytes"], b_pcie_bytes=info["b_bytes"], a_rows_collapsed=info["a_rows"],
                b_rows=info["b_rows"], b_tokens=info["b_tokens"], b_words=info["b_words"],
                transcript_kernels_us=dict(zip(("count", "scan", "write"), info["kernels_us"])),
                transcript_kernels_sum_us=round(sum(info["kernels_us"]), 2), pack_kernel_us=info["pack_us"])), flush=True)
        dec.close()
        job.close()


if __name__ == "__main__":
    main()
