#!/usr/bin/env python3
"""ec_method_locate2_device against ec_method_locate_device (GPU box).

The yardstick of the locate2 call is locate on the same buffers: it reads the
same a * 512 bytes per stripe and writes the same 4.  For 8+4 and 16+4 with
every brick available, fragments totalling >= 1 GiB per call, device buffers,
one process, three runs: clean fragments, one stripe in every 1024 with one
damaged chunk (a flipped bit, the bricks taking turns), and one stripe in
every 1024 with two damaged chunks (bricks b and b + 1 + j, taking turns, so
basis + basis, basis + check and check + check pairs all occur).  Each run:
>= 150 ms of alternating locate / locate2 calls as load, then ROUNDS (default
5) rounds of REPS (default 100) locate calls and REPS locate2 calls, each
round timed by device events on the call's stream.  Prints the ms per call of
every round, locate's round-to-round spread, the ratio of the medians and the
bytes locate2 reads per second with their share of 8 TB/s (the kernel is bound
by memory).  The fragments are encoded on the device from random data, so
loc[] of locate2 is validated after every round: all zero when clean, the
damaged bricks' bits in the dirty stripes.  The clean run has a bar: locate2's
median may exceed locate's by locate's own spread in that run plus 2 %.
Usage: python tools/locate2_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
HBM_BPS = 8e12
GEOS = [(8, 12), (16, 20)]
EVERY = 1024


def timed(st, reps, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def damage(frags, want, ts, n, per_stripe):
    """XOR one bit into the chunk of `per_stripe` bricks of every stripe of
    ts (the same call again undoes it); want[] gets the bricks' bits."""
    for j in range(n):
        tb = ts[j::n]
        for i in range(per_stripe):
            b = (j + i * (1 + j % (n - 1))) % n
            frags[b][tb * CHUNK + 64 * (b % 8) + 9 + i] ^= 1 << (b % 8)
            want[tb] |= 1 << b


def main():
    rounds = int(os.environ.get("ROUNDS", "5"))
    reps = int(os.environ.get("REPS", "100"))
    total = int(os.environ.get("TOTAL_MIB", "1024")) << 20
    assert torch.cuda.is_available(), "locate2_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("locate2_bench: %d rounds x %d calls, >= %d MiB of fragments per call" %
          (rounds, reps, total >> 20))
    for k, n in GEOS:
        m = n - k
        nst = (total + n * CHUNK - 1) // (n * CHUNK)
        nst = (nst + 3) // 4 * 4
        fb = nst * CHUNK
        avail = (1 << n) - 1
        with g.ECMatrixList(k, n) as L:
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(n)]
            torch.cuda.synchronize()
            L.encode_device(0, s, nst, data, frags)
            g.sync_device(0, s)
            del data
            loc1 = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            loc = torch.full((nst,), -1, dtype=torch.int32, device=dev)

            def locate():
                L.locate_device(0, s, nst, avail, frags, loc1)

            def locate2():
                L.locate2_device(0, s, nst, avail, frags, loc)

            ts = torch.arange(EVERY // 2 + 1, nst, EVERY, device=dev)
            for run, per_stripe in (("clean", 0), ("single", 1), ("pair", 2)):
                want = torch.zeros(nst, dtype=torch.int32, device=dev)
                damage(frags, want, ts, n, per_stripe)
                torch.cuda.synchronize()
                ndirty = int(torch.count_nonzero(want))
                # load: >= 150 ms of back-to-back calls before the timed window
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.2:
                    for _ in range(10):
                        locate()
                        locate2()
                    g.sync_device(0, s)
                t1, t2, ok = [], [], True
                for r in range(rounds):
                    loc.fill_(-1)
                    torch.cuda.synchronize()
                    t1.append(timed(st, reps, locate))
                    t2.append(timed(st, reps, locate2))
                    ok = ok and bool(torch.equal(loc, want))
                    print("%d+%d %s round %d: locate %.4f ms  locate2 %.4f ms" %
                          (k, m, run, r, t1[-1], t2[-1]))
                s1, s2 = sorted(t1), sorted(t2)
                med1, med2 = s1[len(s1) // 2], s2[len(s2) // 2]
                spread = (s1[-1] - s1[0]) / s1[0]
                rd = n * fb
                bar = ""
                if run == "clean":
                    bar = "; bar locate2 / locate <= %.3f: %s" % (
                        1.02 + spread, "met" if med2 / med1 <= 1.02 + spread else "NOT met")
                print("%d+%d %s, %d stripes (%d dirty, %.1f MiB per fragment, %.3f GiB per call): "
                      "locate median %.4f ms (min %.4f max %.4f, spread %.1f %%), locate2 median "
                      "%.4f ms (min %.4f max %.4f), locate2 / locate %.3f; locate2 reads %.0f GB/s "
                      "= %.1f %% of 8 TB/s (memory-bound); loc ok %s%s" %
                      (k, m, run, nst, ndirty, fb / 2.0**20, rd / 2.0**30, med1, s1[0], s1[-1],
                       100 * spread, med2, s2[0], s2[-1], med2 / med1, rd / (med2 * 1e-3) / 1e9,
                       100 * rd / (med2 * 1e-3) / HBM_BPS, ok, bar))
                damage(frags, want, ts, n, per_stripe)          # undo
            del frags, loc, loc1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
