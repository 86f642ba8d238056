#!/usr/bin/env python3
"""ec_method_writev_rmw_device against what a caller queued before it existed
(GPU box).

For a 4+2 write with mask 0x3C of the ranges (head, size) = (100, 4096) and
(100, 2^16 S - 333), S = 2048, device buffers, one process, and the large one
again in place (the outputs are the fragments the old chunks are read from):
  (a) ec_method_writev_rmw_device with the stored chunks of the two edge
      stripes;
  (b) ec_method_decode_device of each edge stripe into a preallocated
      temporary of S bytes, then ec_method_writev_encode_device with them,
both on one stream.  After >= 200 ms of alternating calls as load, ROUNDS
(default 5) rounds alternate REPS calls of (a) and of (b) (default 50 for the
large range, 400 for the small one), each block timed by device events on the
stream.  After every round the fragments of both routes are compared over all
bytes with each other and with ec_method_encode_device of the merged data,
which torch builds from the data that was encoded.  Prints the ms per call of
every round, the medians, each side's round-to-round spread and (a) / (b).
Usage: python tools/writev_rmw_bench.py"""
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
    assert torch.cuda.is_available(), "writev_rmw_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    bricks = [b for b in range(N) if (MASK >> b) & 1]
    large = int(os.environ.get("REPS_LARGE", "50"))
    small = int(os.environ.get("REPS_SMALL", "400"))
    for head, size, reps, in_place in ((100, 4096, small, False),
                                       (100, (1 << 16) * S - 333, large, False),
                                       (100, (1 << 16) * S - 333, large, True)):
        end = head + size
        ns = -(-end // S)
        whole = end // S - (1 if head else 0)
        edges = (1 if head or end < S else 0) + (1 if end // S >= 1 and end % S else 0)
        launches = (1 if whole > 0 else 0) + (1 if edges else 0)
        with g.ECMatrixList(K, N) as L:
            data = torch.randint(0, 256, (ns * S,), dtype=torch.uint8, device=dev)
            user = torch.randint(0, 256, (size + 3,), dtype=torch.uint8, device=dev)[3:]
            stored = [torch.empty(ns * CHUNK, dtype=torch.uint8, device=dev) for _ in range(N)]
            want = [torch.empty(ns * CHUNK, dtype=torch.uint8, device=dev) for _ in range(N)]
            merged = data.clone()
            merged[head:end] = user
            torch.cuda.synchronize()
            L.encode_device(0, s, ns, data, stored)
            L.encode_device(0, s, ns, merged, want)
            g.sync_device(0, s)
            del merged
            # the stored chunks of the edge stripes, as the caller holds them
            if in_place:
                out_a = stored
                old_head = [stored[b][:CHUNK] for b in bricks]
                old_tail = [stored[b][(ns - 1) * CHUNK:] for b in bricks]
            else:
                out_a = [torch.full((ns * CHUNK,), 0xA5, dtype=torch.uint8, device=dev)
                         for _ in range(N)]
                old_head = [stored[b][:CHUNK].clone() for b in bricks]
                old_tail = [stored[b][(ns - 1) * CHUNK:].clone() for b in bricks]
            # route (b) never runs in place: its edges come from copies
            b_head = [stored[b][:CHUNK].clone() for b in bricks]
            b_tail = [stored[b][(ns - 1) * CHUNK:].clone() for b in bricks]
            out_b = [torch.full((ns * CHUNK,), 0xA5, dtype=torch.uint8, device=dev)
                     for _ in range(N)]
            o0 = torch.empty(S, dtype=torch.uint8, device=dev)
            o1 = torch.empty(S, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def fused():
                L.writev_rmw_device(0, s, head, size, user, MASK, old_head, old_tail, out_a)

            def parent():
                L.decode_device(0, s, 1, MASK, b_head, o0)
                L.decode_device(0, s, 1, MASK, b_tail, o1)
                L.writev_encode_device(0, s, head, size, user, o0, o1, out_b)

            def restore():
                """in place, a call changes the chunks the next one reads: the
                second call on would merge into the new stripes, which gives the
                same fragments, so nothing is restored between calls; the
                stored edge chunks are put back before a round is checked
                against a fresh run."""
                if in_place:
                    for b in range(N):
                        stored[b][:CHUNK].copy_(first[b])
                        stored[b][(ns - 1) * CHUNK:].copy_(last[b])

            first = [f[:CHUNK].clone() for f in stored]
            last = [f[(ns - 1) * CHUNK:].clone() for f in stored]
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:
                for _ in range(10):
                    fused()
                    parent()
                g.sync_device(0, s)
            ta, tb = [], []
            ok = True
            for r in range(rounds):
                ta.append(timed(st, reps, fused))
                tb.append(timed(st, reps, parent))
                # one call of each from the stored state, then every byte
                with torch.cuda.stream(st):
                    restore()
                    for o in out_b if in_place else out_a + out_b:
                        o.fill_(0xA5)
                fused()
                parent()
                g.sync_device(0, s)
                good = all(bool(torch.equal(a, b)) and bool(torch.equal(a, w))
                           for a, b, w in zip(out_a, out_b, want))
                ok = ok and good
                print("4+2 mask %#x range (%d, %d)%s round %d: (a) writev_rmw_device %.4f ms  "
                      "(b) 2 x decode_device + writev_encode_device %.4f ms  fragments equal "
                      "each other and the encode of the merged data %s" %
                      (MASK, head, size, " in place" if in_place else "", r, ta[-1], tb[-1], good))
            sa, sb = sorted(ta), sorted(tb)
            amed, bmed = sa[len(sa) // 2], sb[len(sb) // 2]
            print("4+2 mask %#x range (%d, %d)%s: %d stripes, %d whole + %d edge, (a) issues %d "
                  "launch(es); (a) median %.4f ms (min %.4f max %.4f, spread %.1f %%), (b) median "
                  "%.4f ms (min %.4f max %.4f, spread %.1f %%); (a) / (b) %.3f; all rounds ok %s" %
                  (MASK, head, size, " in place" if in_place else "", ns, max(whole, 0), edges,
                   launches, amed, sa[0], sa[-1], 100 * (sa[-1] - sa[0]) / sa[0], bmed, sb[0],
                   sb[-1], 100 * (sb[-1] - sb[0]) / sb[0], amed / bmed, ok))
            if not ok:
                sys.exit("writev_rmw_bench: a round failed its validation")
            del data, user, stored, want, out_a, out_b, old_head, old_tail, b_head, b_tail
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
