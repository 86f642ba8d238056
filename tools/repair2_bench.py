#!/usr/bin/env python3
"""What ec_method_repair2_device adds to a scrub, what it costs where
ec_method_repair_device would do, and its dense worst case (GPU box).

For 8+4 and 16+4 with every brick available, fragments totalling >= 1 GiB per
call, device buffers, one process.  Each run: >= 150 ms of back-to-back calls
as load, then ROUNDS (default 5) alternating rounds of REPS (default 100)
calls of every variant, each round timed by device events on the call's
stream.  Results are validated after every round.  The yardsticks are the
kernels that were there before: ec_locate2_n, ec_locate_n + ec_repair_n, and
the heal combine.

clean.  `locate2` = locate2_device alone, the yardstick; `pair` =
locate2_device followed by repair2_device on the same stream, timed together.
The expectation is
  (pair - locate2) / locate2  <=  locate2's round-to-round spread + 5 %.

single.  One dirty stripe in every 1024 (a flipped bit, the bricks taking
turns).  A repair leaves the fragments clean, so a call that is to find them
dirty again has to damage them first: `hit` is one index_put of the damaged
bytes into the buffer that holds all fragments, carried by both sides.
`old` = hit, locate_device, repair_device; `new` = hit, locate_device,
repair2_device.  The expectation is
  (new - old) / old  <=  old's round-to-round spread + 5 %.

pairs, no bar.  One stripe in every 1024 with two damaged chunks, two basis
bricks, a basis and a check brick, two check bricks taking turns.  `hit+
locate2` against `hit+locate2+repair2`: what repair2 adds to the locate2 call.

dense, no bar.  Every stripe names bricks 0 and 1, against heal_device with
mask = the k lowest other bricks and target_mask = bricks 0 and 1 written in
place.  Both move the same k + 2 chunks per stripe.
Usage: python tools/repair2_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
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
    assert torch.cuda.is_available(), "repair2_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("repair2_bench: %d rounds x %d calls (dense: %d), >= %d MiB of fragments per call" %
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

            def locate2():
                L.locate2_device(0, s, nst, avail, frags, loc)

            def pair2():
                L.locate2_device(0, s, nst, avail, frags, loc)
                L.repair2_device(0, s, nst, avail, frags, loc)

            def is_clean(want):
                g.sync_device(0, s)
                return bool(torch.equal(loc, want)) and bool(torch.equal(big, clean))

            # ---- clean
            pair2()
            ok = is_clean(zero)
            load(s, (locate2, pair2))
            tl, tp = [], []
            for r in range(rounds):
                tl.append(timed(st, reps, locate2))
                tp.append(timed(st, reps, pair2))
                ok = ok and is_clean(zero)
                print("%d+%d clean round %d: locate2 %.4f ms  pair %.4f ms" %
                      (k, m, r, tl[-1], tp[-1]))
            add = (med(tp) - med(tl)) / med(tl)
            print("%d+%d clean, %d stripes (%.3f GiB per call): locate2 median %.4f ms (spread "
                  "%.1f %%), locate2+repair2 median %.4f ms; repair2 adds %.1f %% (allowed "
                  "%.1f %%): %s; results ok %s" %
                  (k, m, nst, n * fb / 2.0**30, med(tl), 100 * spread(tl), med(tp), 100 * add,
                   100 * spread(tl) + 5, "met" if add <= spread(tl) + 0.05 else "MISSED", ok))

            # ---- single: one dirty stripe in every 1024, one chunk
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

            def old():
                big.index_put_((idx,), dmg)
                L.locate_device(0, s, nst, avail, frags, loc)
                L.repair_device(0, s, nst, avail, frags, loc)

            def new():
                big.index_put_((idx,), dmg)
                L.locate_device(0, s, nst, avail, frags, loc)
                L.repair2_device(0, s, nst, avail, frags, loc)

            ok = True
            for call in (old, new):
                call()
                ok = ok and is_clean(want)
            load(s, (old, new))
            to, tn = [], []
            for r in range(rounds):
                to.append(timed(st, reps, old))
                ok = ok and is_clean(want)
                tn.append(timed(st, reps, new))
                ok = ok and is_clean(want)
                print("%d+%d single round %d: hit+locate+repair %.4f ms  hit+locate+repair2 %.4f ms"
                      % (k, m, r, to[-1], tn[-1]))
            add = (med(tn) - med(to)) / med(to)
            print("%d+%d single, %d stripes (%d dirty): hit+locate+repair median %.4f ms (spread "
                  "%.1f %%), hit+locate+repair2 median %.4f ms; repair2 costs %+.4f ms = %+.1f %% "
                  "(allowed %.1f %%): %s; results ok %s" %
                  (k, m, nst, int(torch.count_nonzero(want)), med(to), 100 * spread(to), med(tn),
                   med(tn) - med(to), 100 * add, 100 * spread(to) + 5,
                   "met" if add <= spread(to) + 0.05 else "MISSED", ok))

            # ---- pairs: one stripe in every 1024 with two damaged chunks
            want = torch.zeros(nst, dtype=torch.int32, device=dev)
            idx, flip = [], []
            tsl = ts.tolist()
            for j, t in enumerate(tsl):
                kind = j % 3
                if kind == 0:
                    pr = (j % (k - 1), j % (k - 1) + 1)
                elif kind == 1:
                    pr = (j % k, k + j % m)
                else:
                    pr = (k + j % (m - 1), k + j % (m - 1) + 1)
                for b in pr:
                    idx.append(b * fb + t * CHUNK + 64 * (b % 8) + 9 + b)
                    flip.append(1 << (b % 8))
                want[t] = (1 << pr[0]) | (1 << pr[1])
            idx = torch.tensor(idx, dtype=torch.int64, device=dev)
            dmg = clean[idx] ^ torch.tensor(flip, dtype=torch.uint8, device=dev)

            def hit():
                big.index_put_((idx,), dmg)

            def hit_locate2():
                hit()
                locate2()

            def hit_pair2():
                hit()
                pair2()

            hit_pair2()
            ok = is_clean(want)
            hit()
            g.sync_device(0, s)
            ok = ok and not bool(torch.equal(big, clean))
            load(s, (locate2, hit_locate2, hit_pair2))
            tl, th, tp = [], [], []
            for r in range(rounds):
                hit()
                tl.append(timed(st, reps, locate2))
                th.append(timed(st, reps, hit_locate2))
                tp.append(timed(st, reps, hit_pair2))
                ok = ok and is_clean(want)
                print("%d+%d pairs round %d: locate2 %.4f ms  hit+locate2 %.4f ms  hit+pair %.4f ms"
                      % (k, m, r, tl[-1], th[-1], tp[-1]))
            add = (med(tp) - med(th)) / med(tl)
            print("%d+%d pairs, %d stripes (%d dirty): locate2 median %.4f ms (spread %.1f %%), "
                  "hit+locate2 median %.4f ms, hit+locate2+repair2 median %.4f ms; repair2 adds "
                  "%.4f ms = %.1f %% of locate2 (no bar); results ok %s" %
                  (k, m, nst, int(torch.count_nonzero(want)), med(tl), 100 * spread(tl), med(th),
                   med(tp), med(tp) - med(th), 100 * add, ok))

            # ---- dense: every stripe names bricks 0 and 1
            big.copy_(clean)
            loc.fill_(3)
            mask01 = ((1 << (k + 2)) - 1) & ~3
            ins, outs = frags[2:k + 2], [frags[0], frags[1]]

            def repair2():
                L.repair2_device(0, s, nst, avail, frags, loc)

            def heal():
                L.heal_device(0, s, nst, mask01, ins, 3, outs)

            ok = True
            for call in (repair2, heal):
                frags[0].zero_()
                frags[1].fill_(0x5A)
                call()
                g.sync_device(0, s)
                ok = ok and bool(torch.equal(big, clean))
            load(s, (repair2, heal))
            tr, th = [], []
            for r in range(rounds):
                th.append(timed(st, dense_reps, heal))
                tr.append(timed(st, dense_reps, repair2))
                g.sync_device(0, s)
                ok = ok and bool(torch.equal(big, clean))
                print("%d+%d dense round %d: heal %.4f ms  repair2 %.4f ms" %
                      (k, m, r, th[-1], tr[-1]))
            mv = (k + 2) * fb
            print("%d+%d dense, %d stripes all naming bricks 0 and 1: heal median %.4f ms "
                  "(%.0f GB/s), repair2 median %.4f ms (%.0f GB/s), repair2 / heal %.2f; results "
                  "ok %s" %
                  (k, m, nst, med(th), mv / (med(th) * 1e-3) / 1e9, med(tr),
                   mv / (med(tr) * 1e-3) / 1e9, med(tr) / med(th), ok))
            del frags, ins, outs, big, clean, loc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
