#!/usr/bin/env python3
"""ec_method_verify_device against ec_method_heal_device (GPU box).

The yardstick of the consistency check is the fused heal with the same
(mask, target_mask = check_mask): it moves the same (k + m) * 512 bytes per
stripe, reading k chunks and writing m, where the check reads k + m and
writes 4 bytes.  For 4+2, 8+4 and 16+4, fragments totalling >= 1 GiB per
call, device buffers, one process: >= 150 ms of alternating heal / verify
calls as load, then ROUNDS (default 5) rounds of REPS (default 100) heal
calls and REPS verify calls, each run timed by device events on the call's
stream.  Prints the ms per call of every round, heal's round-to-round spread,
the bytes the check reads per second and their share of 8 TB/s (the kernel is
bound by memory).  The fragments are encoded on the device from random data,
so the check's flags are validated too: all zero, then one flipped bit.
Usage: python tools/verify_bench.py"""
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
    assert torch.cuda.is_available(), "verify_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("verify_bench: %d rounds x %d calls, >= %d MiB of fragments per call" %
          (rounds, reps, total >> 20))
    for k, n in GEOS:
        m = n - k
        nst = (total + n * CHUNK - 1) // (n * CHUNK)
        nst = (nst + 3) // 4 * 4
        fb = nst * CHUNK
        mask, cmask = (1 << k) - 1, ((1 << m) - 1) << k
        with g.ECMatrixList(k, n) as L:
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(n)]
            torch.cuda.synchronize()
            L.encode_device(0, s, nst, data, frags)
            g.sync_device(0, s)
            del data
            ins, chk = frags[:k], frags[k:]
            outs = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(m)]
            bad = torch.full((nst,), -1, dtype=torch.int32, device=dev)

            def heal():
                L.heal_device(0, s, nst, mask, ins, cmask, outs)

            def verify():
                L.verify_device(0, s, nst, mask, ins, cmask, chk, bad)

            # results first: clean fragments, then one flipped bit
            verify()
            g.sync_device(0, s)
            clean = int(torch.count_nonzero(bad))
            t = nst - 3
            chk[m - 1][t * CHUNK + 77] ^= 4
            torch.cuda.synchronize()
            verify()
            g.sync_device(0, s)
            hit = torch.nonzero(bad).flatten().tolist()
            ok = clean == 0 and hit == [t] and int(bad[t]) == 1 << (n - 1)
            chk[m - 1][t * CHUNK + 77] ^= 4
            torch.cuda.synchronize()
            # load: >= 150 ms of back-to-back calls before the timed window
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:
                for _ in range(10):
                    heal()
                    verify()
                g.sync_device(0, s)
            th, tv = [], []
            for r in range(rounds):
                th.append(timed(st, reps, heal))
                tv.append(timed(st, reps, verify))
                print("%d+%d round %d: heal %.4f ms  verify %.4f ms" % (k, m, r, th[-1], tv[-1]))
            hs, vs = sorted(th), sorted(tv)
            hmed, vmed = hs[len(hs) // 2], vs[len(vs) // 2]
            spread = (hs[-1] - hs[0]) / hs[0]
            rd = n * fb
            print("%d+%d %d stripes (%.1f MiB per fragment, %.3f GiB per call): heal median %.4f ms "
                  "(min %.4f max %.4f, spread %.1f %%), verify median %.4f ms (min %.4f max %.4f), "
                  "verify / heal %.3f; verify reads %.0f GB/s = %.1f %% of 8 TB/s (memory-bound); "
                  "flags ok %s" %
                  (k, m, nst, fb / 2.0**20, rd / 2.0**30, hmed, hs[0], hs[-1], 100 * spread, vmed,
                   vs[0], vs[-1], vmed / hmed, rd / (vmed * 1e-3) / 1e9,
                   100 * rd / (vmed * 1e-3) / HBM_BPS, ok))
            del frags, ins, chk, outs, bad
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
