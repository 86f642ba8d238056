#!/usr/bin/env python3
"""ec_method_locate_device against ec_method_verify_device (GPU box).

The yardstick of the locate call is the consistency check on the same
buffers with mask = the k lowest bricks and check_mask = the others: it reads
the same a * 512 bytes per stripe and writes the same 4.  For 4+2, 8+4 and
16+4 with every brick available, fragments totalling >= 1 GiB per call,
device buffers, one process, two runs: clean fragments, then one dirty
stripe in every 1024 (a flipped bit, the bricks taking turns).  Each run:
>= 150 ms of alternating verify / locate calls as load, then ROUNDS (default
5) rounds of REPS (default 100) verify calls and REPS locate calls, each run
timed by device events on the call's stream.  Prints the ms per call of every
round, verify's round-to-round spread, the ratio of the medians, the bytes
locate reads per second and their share of 8 TB/s (the kernel is bound by
memory).  The fragments are encoded on the device from random data, so loc[]
is validated too: all zero when clean, 1 << brick in the dirty stripes.
Usage: python tools/locate_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
HBM_BPS = 8e12
GEOS = [(4, 6), (8, 12), (16, 20)]
EVERY = 1024


def timed(st, reps, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    rounds = int(os.environ.get("ROUNDS", "5"))
    reps = int(os.environ.get("REPS", "100"))
    total = int(os.environ.get("TOTAL_MIB", "1024")) << 20
    assert torch.cuda.is_available(), "locate_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("locate_bench: %d rounds x %d calls, >= %d MiB of fragments per call" %
          (rounds, reps, total >> 20))
    for k, n in GEOS:
        m = n - k
        nst = (total + n * CHUNK - 1) // (n * CHUNK)
        nst = (nst + 3) // 4 * 4
        fb = nst * CHUNK
        mask, cmask, avail = (1 << k) - 1, ((1 << m) - 1) << k, (1 << n) - 1
        with g.ECMatrixList(k, n) as L:
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(n)]
            torch.cuda.synchronize()
            L.encode_device(0, s, nst, data, frags)
            g.sync_device(0, s)
            del data
            ins, chk = frags[:k], frags[k:]
            bad = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            loc = torch.full((nst,), -1, dtype=torch.int32, device=dev)

            def verify():
                L.verify_device(0, s, nst, mask, ins, cmask, chk, bad)

            def locate():
                L.locate_device(0, s, nst, avail, frags, loc)

            for run in ("clean", "dirty"):
                want = torch.zeros(nst, dtype=torch.int32, device=dev)
                if run == "dirty":
                    ts = torch.arange(EVERY // 2 + 1, nst, EVERY, device=dev)
                    for b in range(n):
                        tb = ts[b::n]
                        frags[b][tb * CHUNK + 64 * (b % 8) + 9] ^= 1 << (b % 8)
                        want[tb] = 1 << b
                    torch.cuda.synchronize()
                locate()
                g.sync_device(0, s)
                ok = bool(torch.equal(loc, want))
                ndirty = int(torch.count_nonzero(want))
                # load: >= 150 ms of back-to-back calls before the timed window
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.2:
                    for _ in range(10):
                        verify()
                        locate()
                    g.sync_device(0, s)
                tv, tl = [], []
                for r in range(rounds):
                    tv.append(timed(st, reps, verify))
                    tl.append(timed(st, reps, locate))
                    print("%d+%d %s round %d: verify %.4f ms  locate %.4f ms" %
                          (k, m, run, r, tv[-1], tl[-1]))
                vs, ls = sorted(tv), sorted(tl)
                vmed, lmed = vs[len(vs) // 2], ls[len(ls) // 2]
                spread = (vs[-1] - vs[0]) / vs[0]
                rd = n * fb
                print("%d+%d %s, %d stripes (%d dirty, %.1f MiB per fragment, %.3f GiB per call): "
                      "verify median %.4f ms (min %.4f max %.4f, spread %.1f %%), locate median "
                      "%.4f ms (min %.4f max %.4f), locate / verify %.3f; locate reads %.0f GB/s = "
                      "%.1f %% of 8 TB/s (memory-bound); loc ok %s" %
                      (k, m, run, nst, ndirty, fb / 2.0**20, rd / 2.0**30, vmed, vs[0], vs[-1],
                       100 * spread, lmed, ls[0], ls[-1], lmed / vmed, rd / (lmed * 1e-3) / 1e9,
                       100 * rd / (lmed * 1e-3) / HBM_BPS, ok))
            del frags, ins, chk, bad, loc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
