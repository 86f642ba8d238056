#!/usr/bin/env python3
"""ec_method_heal_mixed_device against what a caller queued before it existed
(GPU box).

Two heal batches with a pattern per 64-stripe group, device buffers, one
process, at 2^18 and at 2^10 stripes:
  4+2   brick 5 rebuilt from the five 4-subsets of bricks 0 .. 4
  16+4  brick 19 rebuilt from 64 distinct 16-subsets of bricks 0 .. 18
Group g uses pattern g mod the number of patterns.
  (a) ec_method_heal_mixed_device, in place on the stored fragments;
  (b) ec_method_decode_mixed_device into a preallocated temporary of nstripes
      * k * 512 bytes, then ec_method_encode_rows_device of the target brick,
both on one stream.  For information, (c) is ec_method_heal_device of the whole
batch with the first pattern alone.  After >= 200 ms of alternating calls as
load, ROUNDS (default 5) rounds alternate REPS calls of (a), (b) and (c), each
block timed by device events on the stream.  After every round the target
fragment is scribbled over, one call of (a) and of (b) runs, and all target
bytes of both are compared with each other and with ec_method_heal_device of
every group (computed once) and with the fragment as it was encoded.  Prints
the ms per call of every round, the medians, each side's round-to-round spread,
(a) / (b), and the chunks each route moves per stripe: k + m against 3 k + m.
Usage: python tools/heal_mixed_bench.py"""
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
GROUP = 64


def timed(st, reps, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def subsets(bricks, k, count):
    """`count` distinct k-subsets of bricks 0 .. bricks - 1 as masks, spread
    over the lexicographic list."""
    every = list(itertools.combinations(range(bricks), k))
    step = max(1, len(every) // count)
    return [sum(1 << b for b in every[i * step]) for i in range(count)]


def stats(ts):
    s = sorted(ts)
    return s[len(s) // 2], s[0], s[-1], 100 * (s[-1] - s[0]) / s[0]


def main():
    rounds = int(os.environ.get("ROUNDS", "5"))
    assert torch.cuda.is_available(), "heal_mixed_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    large = int(os.environ.get("REPS_LARGE", "20"))
    small = int(os.environ.get("REPS_SMALL", "300"))
    for k, n, npat in ((4, 6, 5), (16, 20, 64)):
        target = n - 1
        masks = subsets(n - 1, k, npat)
        assert len(set(masks)) == npat
        for ns, reps in ((1 << 18, large), (1 << 10, small)):
            ngroups = ns // GROUP
            ids = [gr % npat for gr in range(ngroups)]
            with g.ECMatrixList(k, n) as L:
                data = torch.randint(0, 256, (ns * k * CHUNK,), dtype=torch.uint8, device=dev)
                stored = [torch.empty(ns * CHUNK, dtype=torch.uint8, device=dev)
                          for _ in range(n)]
                gp = torch.tensor(ids, dtype=torch.uint8, device=dev)
                tmp = torch.empty(ns * k * CHUNK, dtype=torch.uint8, device=dev)
                out_b = torch.empty(ns * CHUNK, dtype=torch.uint8, device=dev)
                out_c = torch.empty(ns * CHUNK, dtype=torch.uint8, device=dev)
                want = torch.empty(ns * CHUNK, dtype=torch.uint8, device=dev)
                outs_b = [None] * n
                outs_b[target] = out_b
                torch.cuda.synchronize()
                L.encode_device(0, s, ns, data, stored)
                g.sync_device(0, s)
                del data
                encoded = stored[target].clone()
                # ec_method_heal_device of every group, once
                for gr, u in enumerate(ids):
                    lo, hi = gr * GROUP * CHUNK, (gr + 1) * GROUP * CHUNK
                    L.heal_device(0, s, GROUP, masks[u],
                                  [stored[b][lo:hi] for b in range(n) if (masks[u] >> b) & 1],
                                  1 << target, [want[lo:hi]])
                g.sync_device(0, s)
                targets = [1 << target] * npat
                first = [stored[b] for b in range(n) if (masks[0] >> b) & 1]

                def fused():
                    L.heal_mixed_device(0, s, ns, GROUP, gp, masks, targets, stored)

                def parent():
                    L.decode_mixed_device(0, s, ns, GROUP, gp, masks, stored, tmp)
                    L.encode_rows_device(0, s, ns, tmp, 1 << target, outs_b)

                def single():
                    L.heal_device(0, s, ns, masks[0], first, 1 << target, [out_c])

                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.2:
                    for _ in range(10):
                        fused()
                        parent()
                        single()
                    g.sync_device(0, s)
                ta, tb, tc = [], [], []
                ok = True
                what = "%d+%d, %d patterns, %d stripes in groups of %d" % (k, n - k, npat, ns, GROUP)
                for r in range(rounds):
                    ta.append(timed(st, reps, fused))
                    tb.append(timed(st, reps, parent))
                    tc.append(timed(st, reps, single))
                    with torch.cuda.stream(st):
                        stored[target].fill_(0xA5)
                        out_b.fill_(0xA5)
                    fused()
                    parent()
                    g.sync_device(0, s)
                    good = (bool(torch.equal(stored[target], out_b)) and
                            bool(torch.equal(stored[target], want)) and
                            bool(torch.equal(stored[target], encoded)))
                    ok = ok and good
                    print("%s round %d: (a) heal_mixed_device %.4f ms  (b) decode_mixed_device + "
                          "encode_rows_device %.4f ms  (c) heal_device, one pattern %.4f ms  target "
                          "bytes equal each other, heal_device per group and the encode %s" %
                          (what, r, ta[-1], tb[-1], tc[-1], good))
                a, b, c = stats(ta), stats(tb), stats(tc)
                print("%s: (a) median %.4f ms (min %.4f max %.4f, spread %.1f %%), (b) median "
                      "%.4f ms (min %.4f max %.4f, spread %.1f %%), (c) median %.4f ms; (a) / (b) "
                      "%.3f; chunks per stripe %d against %d; all rounds ok %s" %
                      ((what,) + a + b + (c[0], a[0] / b[0], k + 1, 3 * k + 1, ok)))
                if not ok:
                    sys.exit("heal_mixed_bench: a round failed its validation")
                del stored, tmp, out_b, out_c, want, encoded, first, outs_b
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
