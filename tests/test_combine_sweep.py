"""The combine family on host buffers over every k from 1 to 16
(tests/_combine_sweep.py): decode, heal, mixed decode, encode and row-masked
encode, with the row counts and mask sets that tests/test_gpu_combine_sweep.py
gives the device kernels.  No GPU is needed: with gen = none / avx the host
entry points run on the calling thread's CPU engine, which gets here the
k x rows sweep that tests/test_cpu_engine.py lacks, and the table and its
expected values are proved on a machine without a device.

The expected values come from the oracle, never from the library.  Outputs
are pre-filled with 0xA5 and followed by a guard chunk, and the inputs are
compared with their bytes from before after the calls.
"""
import numpy as np
import pytest

import _combine_sweep as W

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def new_out(chunks):
    return np.full(W.CHUNK * (chunks + 1), W.FILL, np.uint8)


def read_out(out, chunks):
    assert (out[W.CHUNK * chunks:] == W.FILL).all(), "guard chunk written"
    return out[:W.CHUNK * chunks]


def same(got, want, width, what):
    d = np.flatnonzero((got.reshape(-1, width) != want.reshape(-1, width)).any(axis=1))
    assert d.size == 0, (what, "stripes", d[:8].tolist())


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", W.GEOMS, ids=W.geom_id)
def test_combine_sweep_host(ec, geom, gen):
    S = W.built(geom)
    k, n, C, nst = S.k, S.n, S.C, W.NST
    kc = k * W.CHUNK
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        fr = [f.copy() for f in S.frags]
        for m in C.decode:
            out = new_out(k * nst)
            L.decode(W.CHUNK * nst, m, W.rows_of(m), [fr[b] for b in W.bits(m)], out)
            same(read_out(out, k * nst), S.dec[m], kc, ("decode", hex(m)))
        for m, t in C.heal:
            outs = [new_out(nst) for _ in W.bits(t)]
            L.heal(nst, m, [fr[b] for b in W.bits(m)], t, outs)
            for b, o, want in zip(W.bits(t), outs, S.heal[m, t]):
                same(read_out(o, nst), want, W.CHUNK, ("heal", hex(m), hex(t), b))
        for f, want in zip(fr, S.frags):
            assert np.array_equal(f, want), "a fragment was written"

        data = S.data.copy()
        outs = [new_out(nst) for _ in range(n)]
        L.encode(kc * nst, data, outs)
        for b, o in enumerate(outs):
            same(read_out(o, nst), S.enc[b], W.CHUNK, ("encode", b))
        for rm in C.row_masks:
            outs = [new_out(nst) if (rm >> b) & 1 else None for b in range(n)]
            L.encode_rows(kc * nst, data, rm, outs)
            for b in W.bits(rm):
                same(read_out(outs[b], nst), S.enc[b], W.CHUNK, ("encode_rows", hex(rm), b))
        assert np.array_equal(data, S.data), "the data was written"

        mfr = [f.copy() for f in S.mfr]
        for x, want in zip(C.mixed, S.mixed):
            out = new_out(k * x.nst)
            gm = [x.masks[min(i, len(x.masks) - 1)] for i in x.ids.tolist()]
            L.decode_mixed(x.nst, x.group, gm, mfr, out)
            same(read_out(out, k * x.nst), want, kc, ("mixed", x.group, len(x.masks)))
        for f, want in zip(mfr, S.mfr):
            assert np.array_equal(f, want), "a fragment was written"
