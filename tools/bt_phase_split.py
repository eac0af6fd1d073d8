#!/usr/bin/env python3
"""tools/bt_phase_split.py [--workload C2] [--steps 10] -- where the narrow back-trace spends its shader clocks.

Decodes bench.py's workload with "bt_profile" = 1 and prints fltx_decoder_get "bt_prof_*" (clocks of the marking wave,
summed over the utterances of a batch, as shares of the kernel's own span), for the serial walk ("bt_walk_waves" = 1)
and the parallel walk, each ALONE (one decoder object, every batch waited for) and CO-RESIDENT (two decoder objects
taking turns as in bench.py, so a back-trace shares its CUs with the other object's decode kernel).  The marks cost a
few stores per chunk; the run's own time is not a benchmark figure."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

KEYS = ("copy0", "walk", "wait", "store", "fetch0", "score", "total", "utts", "add", "addwait")
SHOWN = ("copy0", "walk", "wait", "store", "fetch0", "score", "add", "addwait")  # (add + addwait = score: the first
# adding wave's own time in the score loop, and its waits for the staging waves at the stretch barriers)


def split(d):
    return {k: int(d.get("bt_prof_" + k)) for k in KEYS}


def main():
    import torch
    a = bench.parse()
    cfg = dict(bench.WORKLOADS[a.workload])
    B = a.batch or cfg["batch"]
    job = bench.Job(a, 0, 0, B, cfg)
    e_dev = torch.from_numpy(job.e_host).cuda()
    torch.cuda.synchronize()

    def fence():
        job.ctx.synchronize()
        for c in job.more_ctx:
            c.synchronize()

    for walk in (1, -1):
        decs = [job.decoder(), job.decoder(second_stream=True)]
        for d in decs:
            d.set("bt_profile", 1)
            d.set("bt_walk_waves", walk)
        for mode in ("alone", "co-resident"):
            acc = dict.fromkeys(KEYS, 0)
            for d in decs:  # (set-up: each object sizes its workspace)
                d.decode_batch(None, job.Ts, job.N, device_ptr=e_dev.data_ptr())
                fence()
            for i in range(a.steps):
                d = decs[i % 2] if mode == "co-resident" else decs[0]
                d.decode_batch(None, job.Ts, job.N, device_ptr=e_dev.data_ptr())
                if mode == "alone":
                    fence()
                if mode == "alone" or i >= 1:  # co-resident: the object whose batch ran beside this call's decode kernel
                    s = split(decs[(i - 1) % 2] if mode == "co-resident" else d)
                    for k in KEYS:
                        acc[k] += s[k]
            fence()
            n = max(acc["utts"], 1)
            tot = max(acc["total"], 1)
            print("walk_waves %d record_bytes %d chunk_frames %d stretch_frames %d %-11s clocks/utterance %8.0f  " %
                  (decs[0].get("bt_walk_waves"), decs[0].get("bt_record_bytes"), decs[0].get("bt_chunk_frames"),
                   decs[0].get("bt_stretch_frames"), mode,
                   acc["total"] / n) +
                  "  ".join("%s %5.1f%%" % (k, 100.0 * acc[k] / tot) for k in SHOWN), flush=True)
        for d in decs:
            d.close()
    job.close()


if __name__ == "__main__":
    main()
