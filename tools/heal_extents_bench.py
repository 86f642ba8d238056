#!/usr/bin/env python3
"""ec_method_heal_extents_device against one ec_method_heal_mixed_device per
extent (GPU box).

Two heal batches of 2^18 stripes in device buffers, one process:
  4+2   brick 5 rebuilt from the five 4-subsets of bricks 0 .. 4
  16+4  brick 19 rebuilt from 64 distinct 16-subsets of bricks 0 .. 18
each as 1024 extents of 256 stripes and as 64 extents of 4096 stripes, every
fragment of every extent a device allocation of its own.  Extent e uses pattern
e mod the number of patterns.
  (a)  one ec_method_heal_extents_device call with the host copy of the table
       (every record and fragment address checked);
  (a0) the same call with ext_host == NULL (a table written on the GPU);
  (b)  one ec_method_heal_mixed_device call per extent, the route for such
       buffers before;
  (c)  for information, one ec_method_heal_mixed_device call over the same
       stripes laid contiguously (which these buffers are not).
The library is called through prebuilt ctypes arguments, so a call costs what
it costs a C caller plus the foreign-function call.  After >= 200 ms of
alternating calls as load, ROUNDS (default 5) rounds alternate the routes, each
block timed by device events on the stream.  After every round the target
fragments are scribbled over and healed by (a), scribbled over again and healed
by (b), and all target bytes of both are compared with each other and with the
fragments as they were encoded.  Prints the ms per batch of every round, the
medians with min - max, and (a) / (b), (a) / (c).
Usage: python tools/heal_extents_bench.py"""
import ctypes
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch first: one HIP runtime)
import numpy as np  # noqa: E402
import glusterfs_amd as g  # noqa: E402
import glusterfs_amd.ec_method as ec  # noqa: E402

CHUNK = 512
GROUP = 64
TOTAL = 1 << 18


def timed(st, reps, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def subsets(bricks, k, count):
    every = list(itertools.combinations(range(bricks), k))
    step = max(1, len(every) // count)
    return [sum(1 << b for b in every[i * step]) for i in range(count)]


def stats(ts):
    s = sorted(ts)
    return s[len(s) // 2], s[0], s[-1]


def main():
    rounds = int(os.environ.get("ROUNDS", "5"))
    assert torch.cuda.is_available(), "heal_extents_bench needs a GPU"
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = st.cuda_stream
    lib = ec.lib
    for k, n, npat in ((4, 6, 5), (16, 20, 64)):
        target = n - 1
        masks = subsets(n - 1, k, npat)
        assert len(set(masks)) == npat
        m_arr = (ctypes.c_size_t * npat)(*masks)
        t_arr = (ctypes.c_size_t * npat)(*([1 << target] * npat))
        for ne, reps_b in ((1024, 2), (64, 10)):
            per = TOTAL // ne
            with g.ECMatrixList(k, n) as L:
                lst = ctypes.byref(L._list)
                data = torch.randint(0, 256, (TOTAL * k * CHUNK,), dtype=torch.uint8, device=dev)
                flat = [torch.empty(TOTAL * CHUNK, dtype=torch.uint8, device=dev)
                        for _ in range(n)]
                torch.cuda.synchronize()
                L.encode_device(0, s, TOTAL, data, flat)
                g.sync_device(0, s)
                del data
                encoded = flat[target].clone()
                # every fragment of every extent in an allocation of its own
                frags = [[flat[b][e * per * CHUNK:(e + 1) * per * CHUNK].clone() for b in range(n)]
                         for e in range(ne)]
                table = ec.extent_table([(frags[e], per, e % npat) for e in range(ne)])
                ntiles = ec.extents_layout(table)
                tdev = torch.from_numpy(np.frombuffer(table, np.uint8).copy()).to(dev)
                gp_e = [torch.full((per // GROUP,), u, dtype=torch.uint8, device=dev)
                        for u in range(npat)]
                gp_flat = torch.tensor([(gr * GROUP // per) % npat for gr in range(TOTAL // GROUP)],
                                       dtype=torch.uint8, device=dev)
                fr_e = [ec._ptr_array(frags[e]) for e in range(ne)]
                fr_flat = ec._ptr_array(flat)
                torch.cuda.synchronize()

                def ext_checked():
                    assert lib.ec_method_heal_extents_device(
                        lst, 0, s, ne, ntiles, tdev.data_ptr(), ec.addr(table), npat, m_arr,
                        t_arr) == 0

                def ext_unchecked():
                    assert lib.ec_method_heal_extents_device(
                        lst, 0, s, ne, ntiles, tdev.data_ptr(), None, npat, m_arr, t_arr) == 0

                def per_extent():
                    for e in range(ne):
                        assert lib.ec_method_heal_mixed_device(
                            lst, 0, s, per, GROUP, gp_e[e % npat].data_ptr(), npat, m_arr, t_arr,
                            fr_e[e]) == 0

                def contiguous():
                    assert lib.ec_method_heal_mixed_device(
                        lst, 0, s, TOTAL, GROUP, gp_flat.data_ptr(), npat, m_arr, t_arr,
                        fr_flat) == 0

                def targets():
                    return torch.cat([frags[e][target] for e in range(ne)])

                def scribble():
                    with torch.cuda.stream(st):
                        for e in range(ne):
                            frags[e][target].fill_(0xA5)

                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.2:
                    ext_checked()
                    ext_unchecked()
                    per_extent()
                    contiguous()
                    g.sync_device(0, s)
                ta, t0_, tb, tc = [], [], [], []
                ok = True
                what = "%d+%d, %d patterns, %d extents of %d stripes" % (k, n - k, npat, ne, per)
                for r in range(rounds):
                    ta.append(timed(st, 20, ext_checked))
                    t0_.append(timed(st, 20, ext_unchecked))
                    tb.append(timed(st, reps_b, per_extent))
                    tc.append(timed(st, 20, contiguous))
                    scribble()
                    ext_checked()
                    g.sync_device(0, s)
                    with torch.cuda.stream(st):
                        got_a = targets()
                    scribble()
                    per_extent()
                    g.sync_device(0, s)
                    with torch.cuda.stream(st):
                        got_b = targets()
                    st.synchronize()
                    good = bool(torch.equal(got_a, got_b)) and bool(torch.equal(got_a, encoded))
                    ok = ok and good
                    print("%s round %d: (a) heal_extents_device %.4f ms  (a0) without ext_host "
                          "%.4f ms  (b) heal_mixed_device per extent %.4f ms  (c) heal_mixed_device, "
                          "contiguous %.4f ms  target bytes of (a) and (b) equal each other and "
                          "the encode %s" % (what, r, ta[-1], t0_[-1], tb[-1], tc[-1], good))
                    del got_a, got_b
                a, a0, b, c = stats(ta), stats(t0_), stats(tb), stats(tc)
                print("%s: (a) median %.4f ms (%.4f - %.4f), (a0) median %.4f ms (%.4f - %.4f), "
                      "(b) median %.4f ms (%.4f - %.4f), (c) median %.4f ms (%.4f - %.4f); "
                      "(a) / (b) %.4f, (a0) / (b) %.4f, (a) / (c) %.3f, (a0) / (c) %.3f; all "
                      "rounds ok %s" % ((what,) + a + a0 + b + c +
                                        (a[0] / b[0], a0[0] / b[0], a[0] / c[0], a0[0] / c[0], ok)))
                sys.stdout.flush()
                if not ok:
                    sys.exit("heal_extents_bench: a round failed its validation")
                del frags, flat, encoded, table, tdev, fr_e, fr_flat, gp_e, gp_flat
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
