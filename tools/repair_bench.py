#!/usr/bin/env python3
"""What ec_method_repair_device adds to a scrub, and its dense worst case
(GPU box).

For 4+2, 8+4 and 16+4 with every brick available, fragments totalling >= 1 GiB
per call, device buffers, one process.  Each run: >= 150 ms of back-to-back
calls as load, then ROUNDS (default 5) alternating rounds of REPS (default
100) calls of every variant, each round timed by device events on the call's
stream.  Results are validated.

scrub, clean fragments.  `locate` = locate_device alone, the yardstick;
`pair` = locate_device followed by repair_device on the same stream, timed
together.

scrub, one dirty stripe in every 1024 (a flipped bit, the bricks taking
turns).  A repair leaves the fragments clean, so a call that is to find them
dirty again has to damage them first: `hit` is one index_put of the damaged
bytes into the buffer that holds all fragments.  `locate` is locate_device
alone on the dirty fragments; `hit+locate` and `hit+pair` carry the same
re-damaging, and what repair adds is their difference.  The expectation is
  (pair - locate) / locate  <=  locate's round-to-round spread + 5 %
with pair - locate = (hit+pair) - (hit+locate) in the dirty run.

dense, no bar: every stripe names brick 0 (loc[] all 1), against
heal_device with mask = the k lowest other bricks and target_mask = brick 0
written in place.  Both move the same k + 1 chunks per stripe.
Usage: python tools/repair_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
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


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return (max(v) - min(v)) / min(v)


def load(s, calls):
    """>= 150 ms of back-to-back calls before a timed window"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.2:
        for _ in range(10):
            for c in calls:
                c()
        g.sync_device(0, s)


def main():
    rounds = int(os.environ.get("ROUNDS", "5"))
    reps = int(os.environ.get("REPS", "100"))
    dense_reps = int(os.environ.get("DENSE_REPS", "20"))
    total = int(os.environ.get("TOTAL_MIB", "1024")) << 20
    assert torch.cuda.is_available(), "repair_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("repair_bench: %d rounds x %d calls (dense: %d), >= %d MiB of fragments per call" %
          (rounds, reps, dense_reps, total >> 20))
    for k, n in GEOS:
        m = n - k
        nst = (total + n * CHUNK - 1) // (n * CHUNK)
        nst = (nst + 3) // 4 * 4
        fb = nst * CHUNK
        avail = (1 << n) - 1
        with g.ECMatrixList(k, n) as L, torch.cuda.stream(st):
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            big = torch.empty(fb * n, dtype=torch.uint8, device=dev)
            frags = [big[b * fb:(b + 1) * fb] for b in range(n)]
            torch.cuda.synchronize()
            L.encode_device(0, s, nst, data, frags)
            g.sync_device(0, s)
            del data
            clean = big.clone()
            loc = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            zero = torch.zeros(nst, dtype=torch.int32, device=dev)

            def locate():
                L.locate_device(0, s, nst, avail, frags, loc)

            def pair():
                L.locate_device(0, s, nst, avail, frags, loc)
                L.repair_device(0, s, nst, avail, frags, loc)

            # ---- scrub, clean
            pair()
            g.sync_device(0, s)
            ok = bool(torch.equal(loc, zero)) and bool(torch.equal(big, clean))
            load(s, (locate, pair))
            tl, tp = [], []
            for r in range(rounds):
                tl.append(timed(st, reps, locate))
                tp.append(timed(st, reps, pair))
                print("%d+%d clean round %d: locate %.4f ms  pair %.4f ms" % (k, m, r, tl[-1], tp[-1]))
            add = (med(tp) - med(tl)) / med(tl)
            print("%d+%d clean, %d stripes (%.3f GiB per call): locate median %.4f ms (spread "
                  "%.1f %%), locate+repair median %.4f ms; repair adds %.1f %% (allowed %.1f %%): "
                  "%s; results ok %s" %
                  (k, m, nst, n * fb / 2.0**30, med(tl), 100 * spread(tl), med(tp), 100 * add,
                   100 * spread(tl) + 5, "met" if add <= spread(tl) + 0.05 else "MISSED", ok))

            # ---- scrub, one dirty stripe in every 1024
            ts = torch.arange(EVERY // 2 + 1, nst, EVERY, device=dev)
            want = torch.zeros(nst, dtype=torch.int32, device=dev)
            idx = []
            for b in range(n):
                tb = ts[b::n]
                idx.append(b * fb + tb * CHUNK + 64 * (b % 8) + 9)
                want[tb] = 1 << b
            idx = torch.cat(idx)
            dmg = clean[idx] ^ torch.cat([torch.full((len(ts[b::n]),), 1 << (b % 8),
                                                     dtype=torch.uint8, device=dev)
                                          for b in range(n)])

            def hit():
                big.index_put_((idx,), dmg)

            def hit_locate():
                hit()
                locate()

            def hit_pair():
                hit()
                pair()

            hit_pair()
            g.sync_device(0, s)
            ok = bool(torch.equal(loc, want)) and bool(torch.equal(big, clean))
            hit()
            g.sync_device(0, s)
            ok = ok and not bool(torch.equal(big, clean))
            load(s, (locate, hit_locate, hit_pair))
            tl, th, tp = [], [], []
            for r in range(rounds):
                hit()
                tl.append(timed(st, reps, locate))
                th.append(timed(st, reps, hit_locate))
                tp.append(timed(st, reps, hit_pair))
                print("%d+%d dirty round %d: locate %.4f ms  hit+locate %.4f ms  hit+pair %.4f ms"
                      % (k, m, r, tl[-1], th[-1], tp[-1]))
            add = (med(tp) - med(th)) / med(tl)
            print("%d+%d dirty, %d stripes (%d dirty): locate median %.4f ms (spread %.1f %%), "
                  "hit+locate median %.4f ms, hit+locate+repair median %.4f ms; repair adds "
                  "%.4f ms = %.1f %% of locate (allowed %.1f %%): %s; results ok %s" %
                  (k, m, nst, int(torch.count_nonzero(want)), med(tl), 100 * spread(tl), med(th),
                   med(tp), med(tp) - med(th), 100 * add, 100 * spread(tl) + 5,
                   "met" if add <= spread(tl) + 0.05 else "MISSED", ok))

            # ---- dense: every stripe names brick 0
            big.copy_(clean)
            loc.fill_(1)
            mask0 = ((1 << (k + 1)) - 1) & ~1
            ins, outs = frags[1:k + 1], [frags[0]]

            def repair():
                L.repair_device(0, s, nst, avail, frags, loc)

            def heal():
                L.heal_device(0, s, nst, mask0, ins, 1, outs)

            ok = True
            for call in (repair, heal):
                frags[0].zero_()
                call()
                g.sync_device(0, s)
                ok = ok and bool(torch.equal(big, clean))
            load(s, (repair, heal))
            tr, th = [], []
            for r in range(rounds):
                th.append(timed(st, dense_reps, heal))
                tr.append(timed(st, dense_reps, repair))
                print("%d+%d dense round %d: heal %.4f ms  repair %.4f ms" % (k, m, r, th[-1], tr[-1]))
            mv = (k + 1) * fb
            print("%d+%d dense, %d stripes all naming brick 0: heal median %.4f ms (%.0f GB/s), "
                  "repair median %.4f ms (%.0f GB/s), repair / heal %.2f; results ok %s" %
                  (k, m, nst, med(th), mv / (med(th) * 1e-3) / 1e9, med(tr),
                   mv / (med(tr) * 1e-3) / 1e9, med(tr) / med(th), ok))
            del frags, ins, outs, big, clean, loc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
