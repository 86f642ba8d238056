"""ec_method_decode_checked2 on host buffers: a read that checks the a >= k + 4
fragments at hand, names up to two bad bricks per stripe and decodes around
them.  No GPU is needed: the host entry point runs on the calling thread's CPU
engine for every gen.

Expected values come from the oracle and the contract (tests/
_decode_checked2_cases.py): loc[] is ec_method_locate2's, out is the oracle's
decode with mask B, or B_S where loc names the bricks of S.  The geometries
and sizes of tests/test_locate2.py; clean fragments, the single-brick classes
of tests/test_decode_checked.py, the seven kinds of pair damaged in four ways,
a pair whose check brick is c0, the pair of the first and the last basis
brick, three bricks at one symbol, a tile of four different outcomes with a
pair in the next tile, two pairs in one tile, a pair in a ragged last tile
and every stripe dirty.  out is pre-filled with 0xA5 and followed by a guard
chunk, loc[] with 0xFFFFFFFF and guard words; no fragment may change.
"""
import ctypes
import errno

import numpy as np
import pytest

import _decode_checked2_cases as C

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def host_runner(L, k, nst, avail_mask):
    basis = C.bits(avail_mask)[:k]
    bmask = C.mask_of(basis)

    def run(frags):
        copies = [None if f is None else f.copy() for f in frags]
        out = np.full(C.CHUNK * (k * nst + 1), C.FILL, np.uint8)
        loc = np.full(nst + C.GUARD, C.SENTINEL, np.uint32)
        nbad, nmany = L.decode_checked2(nst, avail_mask, frags, out, loc)
        assert (loc[nst:] == C.SENTINEL).all(), "guard words written"
        assert (out[C.CHUNK * k * nst:] == C.FILL).all(), "guard chunk written"
        for f, c in zip(frags, copies):
            assert f is None or np.array_equal(f, c), "a fragment was written"
        loc2_ref = np.full(nst, C.SENTINEL, np.uint32)
        L.locate2(nst, avail_mask, frags, loc2_ref)
        loc1_ref = np.full(nst, C.SENTINEL, np.uint32)
        out1_ref = np.full(C.CHUNK * k * nst, C.FILL, np.uint8)
        L.decode_checked(nst, avail_mask, frags, out1_ref, loc1_ref)
        dec_ref = np.empty(C.CHUNK * k * nst, np.uint8)
        L.decode_batch(nst, bmask, [b + 1 for b in basis], [frags[b] for b in basis], dec_ref)
        return dict(loc=loc[:nst], out=out[:C.CHUNK * k * nst], nbad=nbad, nmany=nmany,
                    loc2_ref=loc2_ref, loc1_ref=loc1_ref, out1_ref=out1_ref, dec_ref=dec_ref)
    return run


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("nst", C.SIZES)
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_decode_checked2_matches_contract(ec, oracle, geom, nst, gen):
    k, n, avail_mask = geom
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        C.run_geometry(host_runner(L, k, nst, avail_mask), oracle, k, n, avail_mask, nst)


def _mixed(oracle, k, n, nst):
    """Stripe 1: a basis pair; 2: one basis brick; 4: three bricks at three
    symbols (MANY)."""
    frags = list(C.fragments(oracle, k, n, nst))
    frags[0] = C.flipped(frags[0], 1, 100, 1)
    frags[k - 1] = C.flipped(frags[k - 1], 1, 101, 2)
    frags[1] = C.flipped(frags[1], 2, 100, 1)
    frags[0] = C.flipped(frags[0], 4, 7, 1)
    frags[2] = C.flipped(frags[2], 4, 8, 1)
    frags[n - 1] = C.flipped(frags[n - 1], 4, 9, 1)
    return frags, [0, 1 | 1 << (k - 1), 1 << 1, 0, C.MANY]


def test_decode_checked2_leaves_stats_alone(ec, oracle):
    """Clean, corrected and MANY stripes in one call, on a gen=none and on a
    gen=auto volume: ec_method_stats_t does not move."""
    k, n, nst = 8, 12, 5
    frags, want = _mixed(oracle, k, n, nst)
    data = C.user_data(oracle, k, n, nst).reshape(nst, -1)
    out = np.full(C.CHUNK * k * nst, C.FILL, np.uint8)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    for gen in ("none", None):
        with (ec.ECMatrixList(k, n, gen=gen) if gen else ec.ECMatrixList(k, n)) as L:
            s0 = ec.stats()
            assert L.decode_checked2(nst, 0xFFF, frags, out, loc) == (3, 1)
            assert ec.stats() == s0, "ec_method_decode_checked2 touched ec_method_stats_t"
        assert loc.tolist() == want
        assert np.array_equal(out.reshape(nst, -1)[:4], data[:4])


def test_decode_checked2_zero_stripes_is_a_noop(ec):
    frags = [np.zeros(C.CHUNK, np.uint8) for _ in range(12)]
    out = np.full(C.CHUNK, C.FILL, np.uint8)
    loc = np.full(4, C.SENTINEL, np.uint32)
    nbad, nmany = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(8, 12, gen="none") as L:
        rc = ec.lib.ec_method_decode_checked2(ctypes.byref(L._list), 0, 0xFFF,
                                              ec._ptr_array(frags), out.ctypes.data,
                                              loc.ctypes.data, ctypes.byref(nbad),
                                              ctypes.byref(nmany))
        assert rc == 0
        # the argument checks come first
        for mask, o in ((0x7FF, out.ctypes.data), (0xFFF, None)):
            rc = ec.lib.ec_method_decode_checked2(ctypes.byref(L._list), 0, mask,
                                                  ec._ptr_array(frags), o, loc.ctypes.data,
                                                  ctypes.byref(nbad), ctypes.byref(nmany))
            assert rc == -errno.EINVAL
    assert (loc == C.SENTINEL).all() and (out == C.FILL).all()
    assert nbad.value == 77 and nmany.value == 78


@pytest.mark.parametrize("null", ["nbad", "nmany", "both"])
def test_decode_checked2_counters_may_be_null(ec, oracle, null):
    k, n, nst = 8, 12, 5
    frags, want = _mixed(oracle, k, n, nst)
    data = C.user_data(oracle, k, n, nst).reshape(nst, -1)
    out = np.full(C.CHUNK * k * nst, C.FILL, np.uint8)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    nbad, nmany = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(k, n, gen="none") as L:
        rc = ec.lib.ec_method_decode_checked2(
            ctypes.byref(L._list), nst, 0xFFF, ec._ptr_array(frags), out.ctypes.data,
            loc.ctypes.data, None if null in ("nbad", "both") else ctypes.byref(nbad),
            None if null in ("nmany", "both") else ctypes.byref(nmany))
    assert rc == 0
    assert loc.tolist() == want
    assert np.array_equal(out.reshape(nst, -1)[:4], data[:4])
    assert nbad.value == (77 if null in ("nbad", "both") else 3)
    assert nmany.value == (78 if null in ("nmany", "both") else 1)


def _einval_cases():
    """(name, k, n, overrides) of a valid call with every brick available."""
    return [
        ("list NULL", 8, 12, dict(list_null=True)),
        ("frags NULL", 8, 12, dict(frags=None)),
        ("out NULL", 8, 12, dict(out=None)),
        ("loc NULL", 8, 12, dict(loc=None)),
        ("loc not 4-byte aligned", 8, 12, dict(loc_off=2)),
        ("avail_mask with a brick at n", 8, 12, dict(mask=0x1FFF)),
        ("avail_mask above n only", 8, 12, dict(mask=0xFFF000)),
        ("k + 3 bricks", 8, 12, dict(mask=0x7FF)),
        ("k + 3 bricks, a high set", 8, 12, dict(mask=0xFFE)),
        ("k + 2 bricks", 8, 12, dict(mask=0x3FF)),
        ("k bricks", 8, 12, dict(mask=0x0FF)),
        ("empty avail_mask", 8, 12, dict(mask=0)),
        ("frags[0] NULL", 8, 12, dict(null=0)),
        ("frags[11] NULL", 8, 12, dict(null=11)),
        ("4+2 volume, every brick", 4, 6, dict(mask=0x3F)),
        ("2+1 volume, every brick", 2, 3, dict(mask=0x7)),
        ("16+4 with k + 3 bricks", 16, 20, dict(mask=0x7FFFF)),
    ]


@pytest.mark.parametrize("name,k,n,ov", _einval_cases(), ids=[c[0] for c in _einval_cases()])
def test_decode_checked2_einval(ec, name, k, n, ov):
    nst = 2
    frags = [np.zeros(C.CHUNK * nst, np.uint8) for _ in range(n)]
    store = np.full(nst + 2, C.SENTINEL, np.uint32)
    obuf = np.full(C.CHUNK * k * nst, C.FILL, np.uint8)
    if "null" in ov:
        frags[ov["null"]] = None
    fr = None if "frags" in ov else ec._ptr_array(frags)
    loc = None if "loc" in ov else store.ctypes.data + ov.get("loc_off", 0)
    out = None if "out" in ov else obuf.ctypes.data
    nbad, nmany = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(k, n, gen="none") as L:
        lst = None if ov.get("list_null") else ctypes.byref(L._list)
        rc = ec.lib.ec_method_decode_checked2(lst, nst, ov.get("mask", (1 << n) - 1), fr, out,
                                              loc, ctypes.byref(nbad), ctypes.byref(nmany))
        err = (ec.lib.ec_method_last_error() or b"").decode()
    assert rc == -errno.EINVAL, (name, rc)
    assert "ec_method_decode_checked2" in err and "ec_method_decode_checked2_device" not in err, err
    assert (store == C.SENTINEL).all() and (obuf == C.FILL).all(), "a rejected call wrote"
    assert nbad.value == 77 and nmany.value == 78, "a rejected call wrote its counters"


def test_decode_checked2_ignores_entries_outside_avail_mask(ec, oracle):
    """Bricks outside avail_mask are not read: a NULL entry and a damaged
    fragment there change nothing."""
    k, n, avail_mask = C.GEOMS[4]                   # 16+6 without bricks 1 and 18
    nst = 5
    frags = list(C.fragments(oracle, k, n, nst))
    frags[1] = None
    frags[18] = np.full(C.CHUNK * nst, 0xA5, np.uint8)
    out = np.full(C.CHUNK * k * nst, C.FILL, np.uint8)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        assert L.decode_checked2(nst, avail_mask, frags, out, loc) == (0, 0)
    assert not loc.any()
    assert np.array_equal(out, C.user_data(oracle, k, n, nst))


def test_decode_checked2_device_rejects_host_buffers(ec):
    """Host buffers given to the device entry point: -EINVAL, GPU or not."""
    nst = 2
    frags = [np.zeros(C.CHUNK * nst, np.uint8) for _ in range(12)]
    out = np.full(C.CHUNK * 8 * nst, C.FILL, np.uint8)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(8, 12, gen="none") as L:
        with pytest.raises(OSError) as e:
            L.decode_checked2_device(0, None, nst, 0xFFF, frags, out, loc)
    assert e.value.errno == errno.EINVAL
    assert "ec_method_decode_checked2_device" in str(e.value)
    assert (loc == C.SENTINEL).all() and (out == C.FILL).all()
