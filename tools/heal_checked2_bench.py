#!/usr/bin/env python3
"""ec_method_heal_checked2_device against what a caller queues today (GPU box).

The yardsticks of the heal that corrects two chunks, on the same buffers in the
same session, both kernels this call does not touch:
  (a) ec_method_heal_device with mask B (the k lowest bricks at hand) followed
      by ec_method_locate2_device on one stream, timed together: the unfused
      call, before any second heal of a dirty stripe;
  (b) ec_method_heal_checked_device: the heal that corrects one chunk.
For 8+6 with bricks 4 and 7 to heal (avail_mask 0x3F6F) and 16+6 with bricks 1
and 18 (0x3BFFFD), source fragments totalling >= 1 GiB per call, device
buffers, one process, three runs: clean fragments, then one single-dirty stripe
in every 1024 (a flipped bit, the available bricks taking turns), then one
pair-dirty stripe in every 1024 (basis + basis, basis + check and check + check
taking turns); the fragments are encoded again before each run.  Each run:
>= 150 ms of alternating calls as load, then ROUNDS (default 5) rounds of REPS
(default 100) calls of (a), of (b) and of the fused call, each timed by device
events on the call's stream.  After every round the fused call's loc[] and
(a)'s are compared over all entries with the bits of the damaged bricks, and
every target of the fused call over all bytes with the fragment the encode
gave that brick.  Prints the ms per call of every round, (a)'s round-to-round
spread, fused / (a) with the bar (clean runs: the fused median is no longer
than (a)'s by more than that spread) beside the ratio of the bytes moved, (a +
m) / (a + k + m), fused / (b), what a dirty stripe per 1024 adds to the fused
call and to (a) over their clean medians, and the bytes the fused call moves
per second as a share of 8 TB/s.
Usage: python tools/heal_checked2_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
HBM_BPS = 8e12
GEOS = [(8, 14, 0x3F6F, (4, 7)), (16, 22, 0x3BFFFD, (1, 18))]
EVERY = 1024


def timed(st, reps, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def damage(run, frags, want, bricks, k, nst, dev):
    """One dirty stripe in every 1024: a flipped bit per named brick, each
    brick at a byte of its own plane."""
    a = len(bricks)
    basis, checks = bricks[:k], bricks[k:]
    r = len(checks)
    ts = torch.arange(EVERY // 2 + 1, nst, EVERY, device=dev)
    if run == "single":
        sets = [(b,) for b in bricks]
    else:
        sets = []
        for i in range(a):
            sets.append((basis[i % k], basis[(i + 1 + i // k) % k]))       # basis + basis
            sets.append((basis[i % k], checks[i % r]))                     # basis + check
            sets.append((checks[i % r], checks[(i + 1) % r]))              # check + check
    for i, S in enumerate(sets):
        assert len(set(S)) == len(S)
        tb = ts[i::len(sets)]
        for b in S:
            frags[b][tb * CHUNK + 64 * (b % 8) + 9] ^= 1 << (b % 8)
            want[tb] |= 1 << b
    torch.cuda.synchronize()


def main():
    rounds = int(os.environ.get("ROUNDS", "5"))
    reps = int(os.environ.get("REPS", "100"))
    total = int(os.environ.get("TOTAL_MIB", "1024")) << 20
    assert torch.cuda.is_available(), "heal_checked2_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("heal_checked2_bench: %d rounds x %d calls, >= %d MiB of source fragments per call" %
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
            # the targets' own fragments stay as the encode gave them: the
            # calls never see them (outside avail_mask), the validation does
            srcs = [frags[b] if (avail >> b) & 1 else None for b in range(n)]
            ins = [frags[b] for b in basis]
            out = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in targets]
            out_a = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in targets]
            out_b = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in targets]
            loc = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            loc_a = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            loc_b = torch.full((nst,), -1, dtype=torch.int32, device=dev)

            def both():
                L.heal_device(0, s, nst, bmask, ins, tmask, out_a)
                L.locate2_device(0, s, nst, avail, srcs, loc_a)

            def checked():
                L.heal_checked_device(0, s, nst, avail, srcs, tmask, out_b, loc_b)

            def fused():
                L.heal_checked2_device(0, s, nst, avail, srcs, tmask, out, loc)

            clean_med = {}
            for run in ("clean", "single", "pair"):
                torch.cuda.synchronize()
                L.encode_device(0, s, nst, data, frags)
                g.sync_device(0, s)
                want = torch.zeros(nst, dtype=torch.int32, device=dev)
                if run != "clean":
                    damage(run, frags, want, bricks, k, nst, dev)
                ndirty = int(torch.count_nonzero(want))
                # load: >= 150 ms of back-to-back calls before the timed window
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.2:
                    for _ in range(10):
                        both()
                        checked()
                        fused()
                    g.sync_device(0, s)
                ta, tb_, tf = [], [], []
                ok = True
                for r in range(rounds):
                    ta.append(timed(st, reps, both))
                    tb_.append(timed(st, reps, checked))
                    tf.append(timed(st, reps, fused))
                    good = bool(torch.equal(loc, want)) and bool(torch.equal(loc_a, want))
                    for o, j in zip(out, targets):
                        good = good and bool(torch.equal(o, frags[j]))
                    ok = ok and good
                    loc.fill_(-1)
                    loc_a.fill_(-1)
                    for o in out:
                        o.fill_(0xA5)
                    torch.cuda.synchronize()
                    print("%d+%d %s round %d: heal+locate2 %.4f ms  heal_checked %.4f ms  "
                          "heal_checked2 %.4f ms  loc and targets ok %s" %
                          (k, n - k, run, r, ta[-1], tb_[-1], tf[-1], good))
                sa, sb, sf = sorted(ta), sorted(tb_), sorted(tf)
                amed, bmed, fmed = sa[len(sa) // 2], sb[len(sb) // 2], sf[len(sf) // 2]
                spread = (sa[-1] - sa[0]) / sa[0]
                moved = (a + m) * fb
                if run == "clean":
                    clean_med = dict(a=amed, f=fmed)
                    note = "; bar (fused <= (a) + spread) %s" % (
                        "met" if fmed <= amed * (1 + spread) else "MISSED")
                else:
                    note = "; over clean: fused %+.4f ms (%+.1f %%), (a) %+.4f ms (%+.1f %%)" % (
                        fmed - clean_med["f"], 100 * (fmed / clean_med["f"] - 1),
                        amed - clean_med["a"], 100 * (amed / clean_med["a"] - 1))
                print("%d+%d avail %#x targets %s %s, %d stripes (%d dirty, %.1f MiB per fragment, "
                      "%.3f GiB read per call): (a) heal+locate2 median %.4f ms (min %.4f max "
                      "%.4f, spread %.1f %%), (b) heal_checked median %.4f ms (min %.4f max %.4f), "
                      "heal_checked2 median %.4f ms (min %.4f max %.4f); fused / (a) %.3f (bytes "
                      "%.3f)%s; fused / (b) %.3f; fused moves %.0f GB/s = %.1f %% of 8 TB/s; all "
                      "rounds ok %s" %
                      (k, n - k, avail, list(targets), run, nst, ndirty, fb / 2.0**20,
                       a * fb / 2.0**30, amed, sa[0], sa[-1], 100 * spread, bmed, sb[0], sb[-1],
                       fmed, sf[0], sf[-1], fmed / amed, (a + m) / float(a + k + m), note,
                       fmed / bmed, moved / (fmed * 1e-3) / 1e9,
                       100 * moved / (fmed * 1e-3) / HBM_BPS, ok))
                if not ok:
                    sys.exit("heal_checked2_bench: a round failed its validation")
            del data, frags, srcs, ins, out, out_a, out_b, loc, loc_a, loc_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
