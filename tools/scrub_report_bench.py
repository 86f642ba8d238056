#!/usr/bin/env python3
"""ec_method_scrub_report_device against copying loc[] to the host (GPU box).

What a scrubber does after ec_method_locate_device, two ways, for 4+2 and 16+4
with every brick available and 2^20 stripes, device buffers, one process:
clean fragments, then one dirty stripe in every 100 (a flipped bit, the bricks
taking turns).  Per repetition, alternating, each timed on the host clock from
before the locate call is queued until the scrubber holds its answer:
  locate   ec_method_locate_device and a wait: the call both ways follow
  report   locate, ec_method_scrub_report_device behind it on the stream, the
           272-byte report copied to pinned memory, a wait, then idx[] and
           val[] of the `listed` entries copied, a wait
  copy     what the library offered before: locate, all of loc[] copied to
           pinned memory, a wait, then ec_method_scrub_report (the host
           variant: one C loop) over the copy
REPS (default 30) repetitions after WARM (default 5); prints the median, min
and max of each, report and copy less the locate median (the added time), the
ratio of the two, the added time as a share of locate, and the bytes each way
moves over PCIe (272 + 12 * listed against 4 * nstripes).  The two answers are
compared on the first repetition.
Usage: python tools/scrub_report_bench.py"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402
from glusterfs_amd import ec_method as m  # noqa: E402

CHUNK = 512
GEOS = [(4, 6), (16, 20)]
NST = 1 << 20
EVERY = 100


def stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def main():
    reps = int(os.environ.get("REPS", "30"))
    warm = int(os.environ.get("WARM", "5"))
    nst = int(os.environ.get("NST", str(NST)))
    cap = nst // 64
    assert torch.cuda.is_available(), "scrub_report_bench needs a GPU"
    assert reps >= 20
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    need = g.scrub_report_work(nst)
    print("scrub_report_bench: %d stripes, cap %d, %d bytes of scratch, %d + %d repetitions" %
          (nst, cap, need, warm, reps))
    for k, n in GEOS:
        fb = nst * CHUNK
        avail = (1 << n) - 1
        with g.ECMatrixList(k, n) as L, torch.cuda.stream(st):
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(n)]
            L.encode_device(0, s, nst, data, frags)
            g.sync_device(0, s)
            del data
            loc = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            rep = torch.zeros(34, dtype=torch.int64, device=dev)
            idx = torch.zeros(cap, dtype=torch.int64, device=dev)
            val = torch.zeros(cap, dtype=torch.int32, device=dev)
            work = torch.zeros(need, dtype=torch.uint8, device=dev)
            h_rep = torch.zeros(34, dtype=torch.int64).pin_memory()
            h_idx = torch.zeros(cap, dtype=torch.int64).pin_memory()
            h_val = torch.zeros(cap, dtype=torch.int32).pin_memory()
            h_loc = torch.zeros(nst, dtype=torch.int32).pin_memory()
            c_rep = m.ScrubReport()
            c_idx, c_val = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)

            def locate():
                L.locate_device(0, s, nst, avail, frags, loc)

            def only_locate():
                locate()
                g.sync_device(0, s)

            def report():
                locate()
                g.scrub_report_device(0, s, nst, loc, rep, cap, idx, val, work)
                h_rep.copy_(rep, non_blocking=True)
                g.sync_device(0, s)
                listed = int(h_rep[2])
                if listed:
                    h_idx[:listed].copy_(idx[:listed], non_blocking=True)
                    h_val[:listed].copy_(val[:listed], non_blocking=True)
                    g.sync_device(0, s)
                return listed

            def copy():
                locate()
                h_loc.copy_(loc, non_blocking=True)
                g.sync_device(0, s)
                rc = m.lib.ec_method_scrub_report(nst, h_loc.data_ptr(), ctypes.addressof(c_rep),
                                                  cap, c_idx.ctypes.data, c_val.ctypes.data)
                assert rc == 0
                return int(c_rep.listed)

            for run in ("clean", "dirty"):
                if run == "dirty":
                    ts = torch.arange(EVERY // 2 + 1, nst, EVERY, device=dev)
                    for b in range(n):
                        tb = ts[b::n]
                        frags[b][tb * CHUNK + 64 * (b % 8) + 9] ^= 1 << (b % 8)
                    g.sync_device(0, s)
                la, lb = report(), copy()
                same = (la == lb and bytes(c_rep) == h_rep.numpy().tobytes() and
                        np.array_equal(h_idx[:la].numpy().view(np.uint64), c_idx[:lb]) and
                        np.array_equal(h_val[:la].numpy().view(np.uint32), c_val[:lb]))
                t = {"locate": [], "report": [], "copy": []}
                for r in range(warm + reps):
                    for name, fn in (("locate", only_locate), ("report", report), ("copy", copy)):
                        t0 = time.perf_counter()
                        fn()
                        dt = (time.perf_counter() - t0) * 1e3
                        if r >= warm:
                            t[name].append(dt)
                lm, l0, l1 = stats(t["locate"])
                rm, r0, r1 = stats(t["report"])
                cm, c0, c1 = stats(t["copy"])
                print("%d+%d %s, %d stripes, nbad %d, listed %d: locate median %.4f ms (min %.4f "
                      "max %.4f); locate + report %.4f ms (min %.4f max %.4f); locate + copy + "
                      "host loop %.4f ms (min %.4f max %.4f)" %
                      (k, n - k, run, nst, int(c_rep.nbad), la, lm, l0, l1, rm, r0, r1, cm, c0, c1))
                print("%d+%d %s: added by report %.4f ms = %.1f %% of locate; added by copy + "
                      "loop %.4f ms = %.1f %% of locate; copy / report (added time) %.2f; PCIe "
                      "bytes report %d, copy %d (%.0f x); same answer %s" %
                      (k, n - k, run, rm - lm, 100 * (rm - lm) / lm, cm - lm,
                       100 * (cm - lm) / lm, (cm - lm) / max(rm - lm, 1e-6), 272 + 12 * la,
                       4 * nst, 4 * nst / (272 + 12 * la), same))
            del frags, loc, rep, idx, val, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
