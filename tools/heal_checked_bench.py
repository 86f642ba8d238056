#!/usr/bin/env python3
"""ec_method_heal_checked_device against what a caller queues today (GPU box).

The yardsticks of the checked heal, on the same buffers in the same session:
  (a) ec_method_heal_device with mask B (the k lowest bricks at hand) followed
      by ec_method_locate_device on one stream, timed together: the unfused
      checked heal, before any second heal of a dirty stripe;
  (b) ec_method_heal_device alone: the trusting heal.
For 8+4 with bricks 4 and 7 to heal (avail_mask 0xF6F) and 16+4 with bricks 1
and 18 (0xBFFFD), source fragments totalling >= 1 GiB per call, device
buffers, one process, two runs: clean fragments, then one dirty stripe in
every 1024 (a flipped bit, the available bricks taking turns).  Each run:
>= 150 ms of alternating calls as load, then ROUNDS (default 5) rounds of REPS
(default 100) calls of (a), of (b) and of the fused call, each timed by device
events on the call's stream.  After every round loc[] is compared over all
entries (zero when clean, 1 << brick in the dirty stripes) and every target
over all bytes with the fragment the encode gave that brick.  Prints the ms
per call of every round, (a)'s round-to-round spread, fused / (a) with the bar
(clean runs: the fused median is no longer than (a)'s by more than that
spread) beside the ratio of the bytes moved, (a + m) / (a + k + m), fused /
(b) beside (a + m) / (k + m), and the bytes the fused call moves per second as
a share of 8 TB/s.
Usage: python tools/heal_checked_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
HBM_BPS = 8e12
GEOS = [(8, 12, 0xF6F, (4, 7)), (16, 20, 0xBFFFD, (1, 18))]
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
    assert torch.cuda.is_available(), "heal_checked_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("heal_checked_bench: %d rounds x %d calls, >= %d MiB of source fragments per call" %
          (rounds, reps, total >> 20))
    for k, n, avail, targets in GEOS:
        bricks = [b for b in range(n) if (avail >> b) & 1]
        a, m = len(bricks), len(targets)
        basis = bricks[:k]
        bmask = sum(1 << b for b in basis)
        tmask = sum(1 << b for b in targets)
        nst = (total + a * CHUNK - 1) // (a * CHUNK)
        nst = (nst + 3) // 4 * 4
        fb = nst * CHUNK
        with g.ECMatrixList(k, n) as L:
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(n)]
            torch.cuda.synchronize()
            L.encode_device(0, s, nst, data, frags)
            g.sync_device(0, s)
            del data
            # the targets' own fragments stay as the encode gave them: the
            # calls never see them (outside avail_mask), the validation does
            srcs = [frags[b] if (avail >> b) & 1 else None for b in range(n)]
            ins = [frags[b] for b in basis]
            out = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in targets]
            out_b = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in targets]
            loc = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            loc_a = torch.full((nst,), -1, dtype=torch.int32, device=dev)

            def both():
                L.heal_device(0, s, nst, bmask, ins, tmask, out_b)
                L.locate_device(0, s, nst, avail, srcs, loc_a)

            def heal():
                L.heal_device(0, s, nst, bmask, ins, tmask, out_b)

            def fused():
                L.heal_checked_device(0, s, nst, avail, srcs, tmask, out, loc)

            for run in ("clean", "dirty"):
                want = torch.zeros(nst, dtype=torch.int32, device=dev)
                if run == "dirty":
                    ts = torch.arange(EVERY // 2 + 1, nst, EVERY, device=dev)
                    for i, b in enumerate(bricks):
                        tb = ts[i::a]
                        frags[b][tb * CHUNK + 64 * (b % 8) + 9] ^= 1 << (b % 8)
                        want[tb] = 1 << b
                    torch.cuda.synchronize()
                ndirty = int(torch.count_nonzero(want))
                # load: >= 150 ms of back-to-back calls before the timed window
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.2:
                    for _ in range(10):
                        both()
                        fused()
                    g.sync_device(0, s)
                ta, tb_, tf = [], [], []
                ok = True
                for r in range(rounds):
                    ta.append(timed(st, reps, both))
                    tb_.append(timed(st, reps, heal))
                    tf.append(timed(st, reps, fused))
                    good = bool(torch.equal(loc, want)) and bool(torch.equal(loc_a, want))
                    for o, j in zip(out, targets):
                        good = good and bool(torch.equal(o, frags[j]))
                    ok = ok and good
                    loc.fill_(-1)
                    for o in out:
                        o.fill_(0xA5)
                    torch.cuda.synchronize()
                    print("%d+%d %s round %d: heal+locate %.4f ms  heal %.4f ms  "
                          "heal_checked %.4f ms  loc and targets ok %s" %
                          (k, n - k, run, r, ta[-1], tb_[-1], tf[-1], good))
                sa, sb, sf = sorted(ta), sorted(tb_), sorted(tf)
                amed, bmed, fmed = sa[len(sa) // 2], sb[len(sb) // 2], sf[len(sf) // 2]
                spread = (sa[-1] - sa[0]) / sa[0]
                moved = (a + m) * fb
                bar = ""
                if run == "clean":
                    bar = "; bar (fused <= (a) + spread) %s" % (
                        "met" if fmed <= amed * (1 + spread) else "MISSED")
                print("%d+%d avail %#x targets %s %s, %d stripes (%d dirty, %.1f MiB per fragment, "
                      "%.3f GiB read per call): (a) heal+locate median %.4f ms (min %.4f max %.4f, "
                      "spread %.1f %%), (b) heal median %.4f ms (min %.4f max %.4f), heal_checked "
                      "median %.4f ms (min %.4f max %.4f); fused / (a) %.3f (bytes %.3f)%s; fused / "
                      "(b) %.3f (bytes %.3f); fused moves %.0f GB/s = %.1f %% of 8 TB/s; all rounds "
                      "ok %s" %
                      (k, n - k, avail, list(targets), run, nst, ndirty, fb / 2.0**20,
                       a * fb / 2.0**30, amed, sa[0], sa[-1], 100 * spread, bmed, sb[0], sb[-1],
                       fmed, sf[0], sf[-1], fmed / amed, (a + m) / float(a + k + m), bar,
                       fmed / bmed, (a + m) / float(k + m), moved / (fmed * 1e-3) / 1e9,
                       100 * moved / (fmed * 1e-3) / HBM_BPS, ok))
                if not ok:
                    sys.exit("heal_checked_bench: a round failed its validation")
            del frags, srcs, ins, out, out_b, loc, loc_a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
