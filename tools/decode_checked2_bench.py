#!/usr/bin/env python3
"""ec_method_decode_checked2_device against what a caller queues today (GPU box).

The yardsticks of the read that corrects two chunks, on the same buffers in
the same session:
  (a) ec_method_decode_device with mask B (the k lowest bricks) followed by
      ec_method_locate2_device on one stream, timed together: the unfused
      read, before any re-decode of a dirty stripe;
  (b) ec_method_decode_checked_device: the read that corrects one chunk.
For 8+4 and 16+4 with every brick available, fragments totalling >= 1 GiB per
call, device buffers, one process, three runs: clean fragments, one
single-dirty stripe in every 1024 (a flipped bit, the bricks taking turns),
one pair-dirty stripe in every 1024 (basis + basis, basis + check and check +
check taking turns).  Each run: >= 150 ms of alternating calls as load, then
ROUNDS (default 5) rounds of REPS (default 100) calls of (a), of (b) and of
the fused call, each timed by device events on the call's stream.  After
every round loc[] is compared over all entries (the fused call's and (a)'s
with the bits of the damaged bricks, (b)'s with MANY where those are two) and
the fused call's out over all bytes with the data the fragments were encoded
from.  Prints the ms per call of every round, (a)'s round-to-round spread,
fused / (a) with the bar (clean runs: the fused median is no longer than (a)'s
by more than that spread) beside the ratio of the bytes moved, (a + k) /
(a + 2k), fused / (b), and the bytes the fused call moves per second as a
share of 8 TB/s.
Usage: python tools/decode_checked2_bench.py"""
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
MANY = -(1 << 31)               # EC_MI355X_LOCATE_MANY as int32


def timed(st, reps, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def dirty_sets(run, k, n, count):
    """The bricks damaged in the j-th dirty stripe."""
    sets = []
    for j in range(count):
        if run == "single":
            sets.append((j % n,))
        elif j % 3 == 0:
            sets.append((j % k, (j % k + 1 + (j // k) % (k - 1)) % k))
        elif j % 3 == 1:
            sets.append((j % k, k + j % (n - k)))
        else:
            sets.append((k + j % (n - k), k + (j + 1) % (n - k)))
    return sets


def main():
    rounds = int(os.environ.get("ROUNDS", "5"))
    reps = int(os.environ.get("REPS", "100"))
    total = int(os.environ.get("TOTAL_MIB", "1024")) << 20
    assert torch.cuda.is_available(), "decode_checked2_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    print("decode_checked2_bench: %d rounds x %d calls, >= %d MiB of fragments per call" %
          (rounds, reps, total >> 20))
    for k, n in GEOS:
        m = n - k
        nst = (total + n * CHUNK - 1) // (n * CHUNK)
        nst = (nst + 3) // 4 * 4
        fb = nst * CHUNK
        mask, avail = (1 << k) - 1, (1 << n) - 1
        with g.ECMatrixList(k, n) as L:
            data = torch.randint(0, 256, (fb * k,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(n)]
            ins = frags[:k]
            out = torch.empty(fb * k, dtype=torch.uint8, device=dev)
            out_a = torch.empty(fb * k, dtype=torch.uint8, device=dev)
            out_b = torch.empty(fb * k, dtype=torch.uint8, device=dev)
            loc = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            loc_a = torch.full((nst,), -1, dtype=torch.int32, device=dev)
            loc_b = torch.full((nst,), -1, dtype=torch.int32, device=dev)

            def both():
                L.decode_device(0, s, nst, mask, ins, out_a)
                L.locate2_device(0, s, nst, avail, frags, loc_a)

            def checked():
                L.decode_checked_device(0, s, nst, avail, frags, out_b, loc_b)

            def fused():
                L.decode_checked2_device(0, s, nst, avail, frags, out, loc)

            for run in ("clean", "single", "pair"):
                # every run starts from freshly encoded fragments
                torch.cuda.synchronize()
                L.encode_device(0, s, nst, data, frags)
                g.sync_device(0, s)
                want = torch.zeros(nst, dtype=torch.int32, device=dev)
                want_b = torch.zeros(nst, dtype=torch.int32, device=dev)
                if run != "clean":
                    ts = list(range(EVERY // 2 + 1, nst, EVERY))
                    for t, S in zip(ts, dirty_sets(run, k, n, len(ts))):
                        for i, b in enumerate(S):
                            frags[b][t * CHUNK + 64 * (b % 8) + 9 + i] ^= 1 << (b % 8)
                        want[t] = sum(1 << b for b in S)
                        want_b[t] = MANY if len(S) == 2 else want[t]
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
                    tb_.append(timed(st, reps, checked))
                    tf.append(timed(st, reps, fused))
                    good = (bool(torch.equal(loc, want)) and bool(torch.equal(loc_a, want)) and
                            bool(torch.equal(loc_b, want_b)) and bool(torch.equal(out, data)))
                    ok = ok and good
                    loc.fill_(-1)
                    out.fill_(0xA5)
                    torch.cuda.synchronize()
                    print("%d+%d %s round %d: decode+locate2 %.4f ms  decode_checked %.4f ms  "
                          "decode_checked2 %.4f ms  loc and out ok %s" %
                          (k, m, run, r, ta[-1], tb_[-1], tf[-1], good))
                sa, sb, sf = sorted(ta), sorted(tb_), sorted(tf)
                amed, bmed, fmed = sa[len(sa) // 2], sb[len(sb) // 2], sf[len(sf) // 2]
                spread = (sa[-1] - sa[0]) / sa[0]
                moved = (n + k) * fb
                bar = ""
                if run == "clean":
                    bar = "; bar (fused <= (a) + spread) %s" % (
                        "met" if fmed <= amed * (1 + spread) else "MISSED")
                print("%d+%d %s, %d stripes (%d dirty, %.1f MiB per fragment, %.3f GiB read per "
                      "call): (a) decode+locate2 median %.4f ms (min %.4f max %.4f, spread %.1f %%), "
                      "(b) decode_checked median %.4f ms (min %.4f max %.4f), decode_checked2 "
                      "median %.4f ms (min %.4f max %.4f); fused / (a) %.3f (bytes %.3f)%s; "
                      "fused / (b) %.3f; fused moves %.0f GB/s = %.1f %% of 8 TB/s; "
                      "all rounds ok %s" %
                      (k, m, run, nst, ndirty, fb / 2.0**20, n * fb / 2.0**30, amed, sa[0], sa[-1],
                       100 * spread, bmed, sb[0], sb[-1], fmed, sf[0], sf[-1], fmed / amed,
                       (n + k) / (n + 2.0 * k), bar, fmed / bmed,
                       moved / (fmed * 1e-3) / 1e9, 100 * moved / (fmed * 1e-3) / HBM_BPS, ok))
                if not ok:
                    sys.exit("decode_checked2_bench: a round failed its validation")
            del data, frags, ins, out, out_a, out_b, loc, loc_a, loc_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
