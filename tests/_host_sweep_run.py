"""Runs the calls of tests/_host_sweep.py through the public host entry points
(encode_batch, encode_rows, decode_batch, decode_mixed, heal, writev_encode)
and checks bytes, guards, inputs and the engine counters; shared by
tests/test_host_sweep.py and tests/test_gpu_host_sweep.py, and the program of
the latter's child processes (not collected by pytest):

    python tests/_host_sweep_run.py table | zcdb0 | batches | split

prints one line per failing call and SWEEP-OK when there is none; `table`
(every call of the default process) also prints one GEOM line per geometry.
"""
import mmap
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _encode_sweep as W      # noqa: E402
import _host_sweep as H        # noqa: E402

NOISE = np.random.default_rng(99).integers(0, 256, 1 << 16, dtype=np.uint8)


class Arenas:
    """One allocation per buffer kind, grown on demand: 'G' pageable, 'P'
    pinned, 'M' pinned (used at +8 bytes), 'R' a registered mapping."""

    def __init__(self, ec, kinds="GPMR"):
        self.ec, self.kinds = ec, kinds
        self.buf, self.own = {}, {}

    def get(self, kind, nbytes):
        if kind not in self.kinds:
            raise AssertionError("no %r buffers in this process" % kind)
        if kind in self.buf and self.buf[kind].size >= nbytes:
            return self.buf[kind]
        self.drop(kind)
        size = (max(nbytes, 1 << 20) * 5 // 4 + 4095) // 4096 * 4096
        if kind == "G":
            self.buf[kind] = W.aligned(size)
        elif kind == "R":
            m = mmap.mmap(-1, size)
            a = np.frombuffer(m, np.uint8)
            r = self.ec.host_registered(a)
            r.__enter__()
            self.buf[kind], self.own[kind] = a, (r, m)
        else:
            p = self.ec.PinnedArray(size)
            self.buf[kind], self.own[kind] = p.array, p
        assert self.buf[kind].ctypes.data % 16 == 0
        return self.buf[kind]

    def drop(self, kind):
        self.buf.pop(kind, None)
        own = self.own.pop(kind, None)
        if own is None:
            return
        if kind == "R":
            own[0].__exit__()
        else:
            own.free()

    def close(self):
        for kind in list(self.buf):
            self.drop(kind)


def _place(arenas, place, ins, wants):
    """Lay the buffers of a call out in the arenas of their kinds: per kind
    the inputs between FLANK noise bytes, then, 4 KiB aligned, the outputs
    with their guards.  Returns (input views, output views, checks)."""
    nin = len(ins)
    views_in, views_out, checks = [None] * nin, [None] * len(wants), []
    for kind in sorted(set(place)):
        off = 8 if kind == "M" else 0
        iidx = [i for i in range(nin) if place[i] == kind]
        oidx = [j for j in range(len(wants)) if place[nin + j] == kind]
        starts, pos = [], 0
        for i in iidx:
            starts.append(pos + H.FLANK + off)
            pos += H.FLANK + 16 + -(-ins[i].size // 16) * 16 + H.FLANK
        in_total = pos
        out_lo = -(-in_total // 4096) * 4096
        lay = H.layout([wants[j].size for j in oidx], off)
        buf = arenas.get(kind, out_lo + lay.total)
        for o in range(0, in_total, NOISE.size):
            buf[o:min(in_total, o + NOISE.size)] = NOISE[:min(NOISE.size, in_total - o)]
        for i, s in zip(iidx, starts):
            buf[s:s + ins[i].size] = ins[i]
            views_in[i] = buf[s:s + ins[i].size]
        before = buf[:in_total].copy()
        obuf = buf[out_lo:out_lo + lay.total]
        obuf[:] = H.FILL
        for j, (_, start, size, _) in zip(oidx, lay.seg):
            views_out[j] = obuf[start:start + size]
        checks.append((kind, buf[:in_total], before, obuf, lay, oidx))
    return views_in, views_out, checks


def run_call(L, B, c, arenas, stats=None, kernels=""):
    """Run call c of Built B on ECMatrixList L; returns the list of what is
    wrong (empty: bytes, guards, inputs and counters are right).  `stats`:
    the module's stats() when the call must run on the GPU."""
    k, n = c.g
    ins, wants = B.io(c)
    kind = c.sh[0]
    if kind == "write":
        _, head, size, oh, ot, niov = c.sh
        user, o1, o2 = B.write(c)[:3]
        packed, st = W.pack_inputs([user, o1, o2], [head % 16, 5, 11], 1)
        keep = packed.copy()
        u = packed[st[0]:st[0] + size]
        form = u if niov == 1 else [u[:size // 3], u[size // 3:2 * size // 3 + 1],
                                    u[2 * size // 3 + 1:]]
    vin, vout, checks = _place(arenas, c.place, ins, wants)
    s0 = stats() if stats else None
    if kind == "enc":
        L.encode_batch(c.nst, vin[0], vout)
    elif kind == "rows":
        it = iter(vout)
        L.encode_rows(c.nst * k * H.CHUNK, vin[0], c.sh[1],
                      [next(it) if (c.sh[1] >> b) & 1 else None for b in range(n)])
    elif kind == "dec":
        L.decode_batch(c.nst, c.sh[1], H.rows_of(c.sh[1]), vin, vout[0])
    elif kind == "heal":
        L.heal(c.nst, c.sh[1], vin, c.sh[2], vout)
    elif kind == "mixed":
        L.decode_mixed(c.nst, c.sh[1].group, H.mixed_masks(c.sh[1]), vin, vout[0])
    else:
        L.writev_encode(head, form, packed[st[1]:st[1] + o1.size] if oh else None,
                        packed[st[2]:st[2] + o2.size] if ot else None, vout)
    errs = []
    if stats:
        s1 = stats()
        if s1["cpu_fallbacks"] != s0["cpu_fallbacks"]:
            errs.append("cpu_fallbacks moved by %d" % (s1["cpu_fallbacks"] - s0["cpu_fallbacks"]))
        if s1["gpu_calls"] != s0["gpu_calls"] + 1:
            errs.append("gpu_calls moved by %d" % (s1["gpu_calls"] - s0["gpu_calls"]))
    if kind == "write" and not np.array_equal(packed, keep):
        errs.append("a write input was written")
    for bk, ibuf, before, obuf, lay, oidx in checks:
        if not np.array_equal(ibuf, before):
            errs.append("kind %s: an input or its flank was written, first at %d"
                        % (bk, int(np.flatnonzero(ibuf != before)[0])))
        for j, what, detail in W.check_outputs(obuf, lay, [wants[j] for j in oidx]):
            errs.append("kind %s: output %d %s: %s" % (bk, oidx[j], what, detail))
    return ["%s [%s]: %s" % (H.call_id(c), kernels, e) for e in errs]


def run_cases(ec, g, B, todo, arenas, stats=None, gen="auto", kern=lambda c: ""):
    errs = []
    with ec.ECMatrixList(g[0], g[1], gen=gen) as L:
        if stats is None:
            assert L.engine.startswith("cpu/"), L.engine
        for c in todo:
            errs += run_call(L, B, c, arenas, stats, kern(c))
    return errs


def main(mode):
    import glusterfs_amd as ec
    assert ec.device_count() >= 1
    stats = ec.ec_method.stats
    arenas = Arenas(ec)
    errs, ran = [], 0
    try:
        if mode == "table":
            for g in H.GEOMS:
                todo = H.cases(g)
                ran += len(todo)
                e = run_cases(ec, g, H.built(g), todo, arenas, stats,
                              kern=lambda c: "".join(sorted(H.kernels_of(c))))
                errs += e
                print("GEOM %s calls=%d failures=%d" % (H.geom_id(g), len(todo), len(e)),
                      flush=True)
        elif mode == "zcdb0":
            # branch E for every K, single and MIXED: the table's calls with
            # k + rows <= 32, all pinned, all pageable and the mixes
            for g in H.GEOMS:
                todo = [c for c in H.cases(g)
                        if c.series in ("small", "mixed") and set(c.place) <= set("PG") and
                        H.kernels_of(c, zcdb=False) == {"E"} and
                        (c.series == "mixed" or c.nst in (1, 2, 5, 8, 9, 16, 17, 41))]
                ran += len(todo)
                errs += run_cases(ec, g, H.built(g), todo, arenas, stats,
                                  kern=lambda c: "".join(sorted(H.kernels_of(c, zcdb=False))))
        else:
            for g in H.BATCH_GEOMS:
                todo = H.batch_cases(g)
                if mode == "split":
                    x = [c for c in H.cases(g) if c.series == "mixed" and c.place[0] in "PG"]
                    one = [c for c in H.cases(g) if c.series == "small" and c.nst in (1, 2, 9) and
                           set(c.place) <= set("PG")]
                    todo = todo + x + one
                ran += len(todo)
                B = H.Built(H.built(g).O, g, todo)
                errs += run_cases(ec, g, B, todo, arenas, stats,
                                  kern=lambda c: "".join(sorted(H.kernels_of(c, batch_mb=1))))
    finally:
        arenas.close()
    for e in errs[:200]:
        print("FAIL " + e)
    print("%d calls, %d failures" % (ran, len(errs)))
    if not errs and ran:
        print("SWEEP-OK")
    return 1 if errs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
