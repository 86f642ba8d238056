#!/usr/bin/env python3
"""ec_method_decode_verified_device and ec_method_heal_verified_device against
what a caller queues today (GPU box).

The yardsticks of the detect-only read and heal, on the same buffers in the
same session:
  (a) ec_method_decode_device (or ec_method_heal_device) with mask B (the k
      lowest bricks at hand) followed by ec_method_verify_device of the other
      bricks against B on one stream, timed together: the two passes;
  (b) the decode or heal alone: the trusting call.
For a 4+2 read and a 4+2 heal of brick 5 from bricks 0...4, a 2+1 read of all
three bricks and an 8+4 read of bricks 0...8, source fragments totalling >= 1
GiB per call, device buffers, one process, two runs each: clean fragments,
then one dirty stripe in every 1024 (a flipped bit, the available bricks
taking turns).  Each run: >= 150 ms of alternating calls as load, then ROUNDS
(default 5) rounds of REPS (default 100) calls of (a), of (b) and of the fused
call, each timed by device events on the call's stream.  After every round
bad[] is compared over all entries (zero when clean; in a dirty stripe the bit
of the damaged check brick, or every check brick's bit for a damaged basis
brick) and every output over all bytes: with (a)'s output, and in the clean
runs also with the encoded data or the fragment the encode gave the target.
Prints the ms per call of every round, (a)'s round-to-round spread, fused /
(a) with the bar (clean runs: the fused median is no longer than (a)'s by more
than that spread) beside the ratio of the bytes moved, (a + w) / (a + k + w)
with w = k chunks written by a read and m by a heal, fused / (b) beside (a +
w) / (k + w), and the bytes the fused call moves per second as a share of
8 TB/s.
Usage: python tools/verified_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
HBM_BPS = 8e12
# (k, n, avail_mask, targets): targets None = the read
GEOS = [(4, 6, 0x1F, None), (4, 6, 0x1F, (5,)), (2, 3, 0x7, None), (8, 12, 0x1FF, None)]
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
    assert torch.cuda.is_available(), "verified_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("verified_bench: %d rounds x %d calls, >= %d MiB of source fragments per call" %
          (rounds, reps, total >> 20))
    for k, n, avail, targets in GEOS:
        bricks = [b for b in range(n) if (avail >> b) & 1]
        a = len(bricks)
        basis, checks = bricks[:k], bricks[k:]
        bmask = sum(1 << b for b in basis)
        cmask = sum(1 << b for b in checks)
        heal = targets is not None
        w = len(targets) if heal else k
        tmask = sum(1 << b for b in targets) if heal else 0
        name = "heal" if heal else "decode"
        nst = (total + a * CHUNK - 1) // (a * CHUNK)
        nst = (nst + 3) // 4 * 4
        fb = nst * CHUNK
        with g.ECMatrixList(k, n) as L:
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(n)]
            torch.cuda.synchronize()
            L.encode_device(0, s, nst, data, frags)
            g.sync_device(0, s)
            # what a clean run must give: the data, or the targets' own
            # fragments, which the calls never see (outside avail_mask)
            clean = [frags[j] for j in targets] if heal else [data]
            srcs = [frags[b] if (avail >> b) & 1 else None for b in range(n)]
            ins = [frags[b] for b in basis]
            chk = [frags[b] for b in checks]
            out = [torch.empty(fb * (1 if heal else k), dtype=torch.uint8, device=dev)
                   for _ in clean]
            out_a = [torch.empty_like(o) for o in out]
            bad = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            bad_a = torch.full((nst,), -1, dtype=torch.int32, device=dev)

            def plain():
                if heal:
                    L.heal_device(0, s, nst, bmask, ins, tmask, out_a)
                else:
                    L.decode_device(0, s, nst, bmask, ins, out_a[0])

            def both():
                plain()
                L.verify_device(0, s, nst, bmask, ins, cmask, chk, bad_a)

            def fused():
                if heal:
                    L.heal_verified_device(0, s, nst, avail, srcs, tmask, out, bad)
                else:
                    L.decode_verified_device(0, s, nst, avail, srcs, out[0], bad)

            for run in ("clean", "dirty"):
                want = torch.zeros(nst, dtype=torch.int32, device=dev)
                if run == "dirty":
                    ts = torch.arange(EVERY // 2 + 1, nst, EVERY, device=dev)
                    for i, b in enumerate(bricks):
                        tb = ts[i::a]
                        frags[b][tb * CHUNK + 64 * (b % 8) + 9] ^= 1 << (b % 8)
                        want[tb] = cmask if b in basis else 1 << b
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
                    tb_.append(timed(st, reps, plain))
                    tf.append(timed(st, reps, fused))
                    good = bool(torch.equal(bad, want)) and bool(torch.equal(bad_a, want))
                    for o, oa, c in zip(out, out_a, clean):
                        good = good and bool(torch.equal(o, oa))
                        if run == "clean":
                            good = good and bool(torch.equal(o, c))
                    ok = ok and good
                    bad.fill_(-1)
                    for o in out:
                        o.fill_(0xA5)
                    torch.cuda.synchronize()
                    print("%d+%d %s %s round %d: %s+verify %.4f ms  %s %.4f ms  "
                          "%s_verified %.4f ms  bad and outputs ok %s" %
                          (k, n - k, name, run, r, name, ta[-1], name, tb_[-1], name, tf[-1],
                           good))
                sa, sb, sf = sorted(ta), sorted(tb_), sorted(tf)
                amed, bmed, fmed = sa[len(sa) // 2], sb[len(sb) // 2], sf[len(sf) // 2]
                spread = (sa[-1] - sa[0]) / sa[0]
                moved = (a + w) * fb
                bar = ""
                if run == "clean":
                    bar = "; bar (fused <= (a) + spread) %s" % (
                        "met" if fmed <= amed * (1 + spread) else "MISSED")
                print("%d+%d avail %#x %s%s %s, %d stripes (%d dirty, %.1f MiB per fragment, "
                      "%.3f GiB read per call): (a) %s+verify median %.4f ms (min %.4f max %.4f, "
                      "spread %.1f %%), (b) %s median %.4f ms (min %.4f max %.4f), %s_verified "
                      "median %.4f ms (min %.4f max %.4f); fused / (a) %.3f (bytes %.3f)%s; fused / "
                      "(b) %.3f (bytes %.3f); fused moves %.0f GB/s = %.1f %% of 8 TB/s; all rounds "
                      "ok %s" %
                      (k, n - k, avail, name, " of %s" % list(targets) if heal else "", run, nst,
                       ndirty, fb / 2.0**20, a * fb / 2.0**30, name, amed, sa[0], sa[-1],
                       100 * spread, name, bmed, sb[0], sb[-1], name, fmed, sf[0], sf[-1],
                       fmed / amed, (a + w) / float(a + k + w), bar, fmed / bmed,
                       (a + w) / float(k + w), moved / (fmed * 1e-3) / 1e9,
                       100 * moved / (fmed * 1e-3) / HBM_BPS, ok))
                if not ok:
                    sys.exit("verified_bench: a round failed its validation")
            del data, frags, srcs, ins, chk, clean, out, out_a, bad, bad_a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
