#!/usr/bin/env python3
"""ec_method_readv_decode_device against what a caller queued before it
existed (GPU box).

For a 4+2 read with mask 0x3C of the ranges (head, size) = (100, 2^16 S - 333)
and (100, 4096), S = 2048, device buffers, one process:
  (a) ec_method_readv_decode_device into a buffer of exactly size bytes;
  (b) ec_method_decode_device into a preallocated temporary of ns * S bytes,
      then a device-to-device copy of size bytes from temporary + head
      (torch's copy_ of a contiguous byte view: hipMemcpyAsync),
both on one stream.  After >= 150 ms of alternating calls as load, ROUNDS
(default 5) rounds alternate REPS calls of (a) and of (b) (default 50 for the
large range, 400 for the small one), each block timed by device events on the
stream.  After every round both destinations are compared over all bytes with
the slice of the data that was encoded.  Prints the ms per call of every
round, the medians, each side's round-to-round spread, (a) / (b), the launches
(a) issues and the bytes each route moves.
Usage: python tools/readv_decode_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import glusterfs_amd as g  # noqa: E402

CHUNK = 512
K, N, MASK = 4, 6, 0x3C
S = K * CHUNK


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
    assert torch.cuda.is_available(), "readv_decode_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    bricks = [b for b in range(N) if (MASK >> b) & 1]
    for head, size, reps in ((100, (1 << 16) * S - 333, int(os.environ.get("REPS_LARGE", "50"))),
                             (100, 4096, int(os.environ.get("REPS_SMALL", "400")))):
        end = head + size
        ns = -(-end // S)
        whole = end // S - (1 if head else 0)
        edges = (1 if head or end < S else 0) + (1 if end // S >= 1 and end % S else 0)
        launches = (1 if whole > 0 else 0) + (1 if edges else 0)
        with g.ECMatrixList(K, N) as L:
            data = torch.randint(0, 256, (ns * S,), dtype=torch.uint8, device=dev)
            frags = [torch.empty(ns * CHUNK, dtype=torch.uint8, device=dev) for _ in range(N)]
            torch.cuda.synchronize()
            L.encode_device(0, s, ns, data, frags)
            g.sync_device(0, s)
            ins = [frags[b] for b in bricks]
            want = data[head:end]
            dst_a = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
            dst_b = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
            tmp = torch.empty(ns * S, dtype=torch.uint8, device=dev)
            tmp_view = tmp[head:end]
            torch.cuda.synchronize()

            def fused():
                L.readv_decode_device(0, s, head, size, MASK, ins, dst_a)

            def two_pass():
                L.decode_device(0, s, ns, MASK, ins, tmp)
                with torch.cuda.stream(st):
                    dst_b.copy_(tmp_view, non_blocking=True)

            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:
                for _ in range(10):
                    fused()
                    two_pass()
                g.sync_device(0, s)
            ta, tb = [], []
            ok = True
            for r in range(rounds):
                ta.append(timed(st, reps, fused))
                tb.append(timed(st, reps, two_pass))
                good = bool(torch.equal(dst_a, want)) and bool(torch.equal(dst_b, want))
                ok = ok and good
                dst_a.fill_(0xA5)
                dst_b.fill_(0xA5)
                torch.cuda.synchronize()
                print("4+2 mask %#x range (%d, %d) round %d: (a) readv_decode_device %.4f ms  "
                      "(b) decode_device + copy %.4f ms  both equal the data %s" %
                      (MASK, head, size, r, ta[-1], tb[-1], good))
            sa, sb = sorted(ta), sorted(tb)
            amed, bmed = sa[len(sa) // 2], sb[len(sb) // 2]
            moved_a = ns * S + size
            moved_b = ns * S + ns * S + 2 * size
            print("4+2 mask %#x range (%d, %d): %d stripes, %d whole + %d edge, (a) issues %d "
                  "launch(es); (a) median %.4f ms (min %.4f max %.4f, spread %.1f %%), (b) median "
                  "%.4f ms (min %.4f max %.4f, spread %.1f %%); (a) / (b) %.3f (bytes moved %.3f); "
                  "(a) moves %.0f GB/s; all rounds ok %s" %
                  (MASK, head, size, ns, max(whole, 0), edges, launches, amed, sa[0], sa[-1],
                   100 * (sa[-1] - sa[0]) / sa[0], bmed, sb[0], sb[-1],
                   100 * (sb[-1] - sb[0]) / sb[0], amed / bmed, moved_a / float(moved_b),
                   moved_a / (amed * 1e-3) / 1e9, ok))
            if not ok:
                sys.exit("readv_decode_bench: a round failed its validation")
            del data, frags, ins, want, dst_a, dst_b, tmp, tmp_view
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
