"""The encode family on host buffers (tests/_encode_sweep.py): plain encodes of
2+1, 4+2, 8+4 and 16+4 at every stripe count, input shift and output offset
that tests/test_gpu_encode_sweep.py gives the device encoders, and the
partial-stripe writes of those four, 5+2 and 10+3 at every head, end, old
content and user alignment of the table, as one buffer and as three iovecs.
No GPU is needed: with gen = none / avx ec_method_encode and
ec_method_writev_encode run on the calling thread's CPU engine
(ecc_encode_gather for the writes), and the table, its expected values and its
guard helper are proved on a machine without a device.

The expected values come from the oracle, never from the library.  Every
output is a slice of one allocation pre-filled with 0xA5, with 2 KiB of guard
on both sides, and the inputs are compared with their bytes from before.
"""
import numpy as np
import pytest

import _encode_sweep as W

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def host_copy(x):
    """A writable, 64-byte aligned copy of a case's packed input buffer."""
    buf = W.aligned(x.ibuf.size)
    buf[:] = x.ibuf
    return buf


def outputs(x):
    buf = W.new_outputs(x.lay)
    return buf, [buf[start:start + size] for _, start, size, _ in x.lay.seg]


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", W.ENC_GEOMS, ids=W.geom_id)
def test_encode_sweep_host(ec, geom, gen):
    S = W.built(geom)
    with ec.ECMatrixList(S.k, S.n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        for x in S.plain:
            ibuf = host_copy(x)
            size = S.S * x.c.nst
            inp = ibuf[x.iseg[0]:x.iseg[0] + size]
            obuf, outs = outputs(x)
            assert inp.ctypes.data % 16 == x.c.off
            assert [o.ctypes.data % 16 for o in outs] == list(x.c.outs)
            L.encode(size, inp, outs)
            assert W.check_outputs(obuf, x.lay, x.want) == [], W.plain_id(x.c)
            assert np.array_equal(ibuf, x.ibuf), (W.plain_id(x.c), "the input was written")


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("geom", W.WRITE_GEOMS, ids=W.geom_id)
def test_writev_sweep_host(ec, geom, gen):
    S = W.built(geom)
    with ec.ECMatrixList(S.k, S.n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        for x in S.writes:
            c = x.c
            ibuf = host_copy(x)
            user = ibuf[x.user:x.user + c.size]
            oh = ibuf[x.oh:x.oh + S.S] if c.oh else None
            ot = ibuf[x.ot:x.ot + S.S] if c.ot else None
            assert user.ctypes.data % 16 == c.mis
            forms = [user]
            if c.size >= 3:                             # a writev iovec list
                a, b = c.size // 3, 2 * c.size // 3 + 1
                forms.append([user[:a], user[a:b], user[b:]])
            for form in forms:
                obuf, outs = outputs(x)
                L.writev_encode(c.head, form, oh, ot, outs)
                what = (W.write_id(c), "iovecs" if form is not user else "one buffer")
                assert W.check_outputs(obuf, x.lay, x.want) == [], what
                assert np.array_equal(ibuf, x.ibuf), (what, "an input was written")


# --- the guard helper itself -------------------------------------------------

def _filled():
    """Three outputs of 3, 1 and 2 chunks at offsets 0, 5 and 15, holding
    what is expected."""
    rng = np.random.default_rng(11)
    wants = [rng.integers(0, 256, W.CHUNK * c, dtype=np.uint8) for c in (3, 1, 2)]
    lay = W.layout([w.size for w in wants], [0, 5, 15])
    buf = W.new_outputs(lay)
    for (_, start, size, _), w in zip(lay.seg, wants):
        buf[start:start + size] = w
    return lay, buf, wants


def test_layout_guards_and_offsets():
    lay, buf, wants = _filled()
    assert buf.ctypes.data % 16 == 0 and lay.total == buf.size
    end = 0
    for (lo, start, size, hi), off in zip(lay.seg, (0, 5, 15)):
        assert lo == end and start % 16 == off
        assert start - lo >= W.GUARD and hi - (start + size) >= W.GUARD
        end = hi
    assert end == lay.total
    assert W.check_outputs(buf, lay, wants) == []


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("where", ["front guard", "back guard", "payload"])
@pytest.mark.parametrize("edge", ["near", "far"])
def test_guard_helper_sees_one_byte(i, where, edge):
    """One byte changed anywhere -- next to the payload or a whole guard away,
    in the first and the last byte of the payload -- is reported, for the
    right output and the right region, and nothing else is."""
    lay, buf, wants = _filled()
    lo, start, size, hi = lay.seg[i]
    at = {("front guard", "near"): start - 1, ("front guard", "far"): lo,
          ("back guard", "near"): start + size, ("back guard", "far"): hi - 1,
          ("payload", "near"): start, ("payload", "far"): start + size - 1}[where, edge]
    buf[at] ^= 0x01
    errs = W.check_outputs(buf, lay, wants)
    assert [(e[0], e[1]) for e in errs] == [(i, where)], errs


def test_guard_helper_sees_a_stray_row_run():
    """A 2 KiB run (one tile's row) written behind output 0 stays inside its
    back guard and is reported as that."""
    lay, buf, wants = _filled()
    _, start, size, _ = lay.seg[0]
    buf[start + size:start + size + W.GUARD] = 0
    errs = W.check_outputs(buf, lay, wants)
    assert [(e[0], e[1]) for e in errs] == [(0, "back guard")], errs


def test_pack_inputs_offsets_and_flanks():
    arrs = [np.full(5, 1, np.uint8), np.full(512, 2, np.uint8), np.full(16, 3, np.uint8)]
    buf, starts = W.pack_inputs(arrs, [3, 0, 15], 7)
    assert [s % 16 for s in starts] == [3, 0, 15]
    assert starts[0] >= W.FLANK and buf.size - (starts[2] + 16) >= W.FLANK
    for a, s, nxt in zip(arrs, starts, starts[1:] + [buf.size + W.FLANK]):
        assert np.array_equal(buf[s:s + a.size], a) and nxt - (s + a.size) >= 2 * W.FLANK
