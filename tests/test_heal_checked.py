"""ec_method_heal_checked on host buffers: a heal that checks the a >= k + 2
source fragments at hand, names the bad brick per stripe and regenerates the
target fragments around it.  No GPU is needed: the host entry point runs on
the calling thread's CPU engine for every gen.

Expected values come from the oracle and the contract (tests/
_heal_checked_cases.py): loc[] is ec_method_locate's, out[j] is the oracle's
encode of its decode with mask B, or B_i where loc names basis brick i.  The
sizes and corruptions of tests/test_decode_checked.py on geometries with holes
in avail_mask for the targets.  Every out[j] is pre-filled with 0xA5 and
followed by a guard chunk, loc[] with 0xFFFFFFFF and guard words; no fragment
may change, nor the buffer of any brick outside avail_mask.
"""
import ctypes
import errno

import numpy as np
import pytest

import _heal_checked_cases as C

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def host_runner(L, k, n, nst, avail_mask, targets):
    avail = C.bits(avail_mask)
    basis = avail[:k]
    tmask = C.mask_of(targets)

    def run(frags):
        # bricks outside avail_mask, the targets among them, get a buffer of
        # their own in frags[]: nothing may read or write it
        given = [np.full(C.CHUNK * nst, 0x3C, np.uint8) if f is None else f for f in frags]
        copies = [f.copy() for f in given]
        out = [np.full(C.CHUNK * (nst + 1), C.FILL, np.uint8) for _ in targets]
        loc = np.full(nst + C.GUARD, C.SENTINEL, np.uint32)
        nbad, nmany = L.heal_checked(nst, avail_mask, given, tmask, out, loc)
        assert (loc[nst:] == C.SENTINEL).all(), "guard words written"
        for o in out:
            assert (o[C.CHUNK * nst:] == C.FILL).all(), "guard chunk written"
        for b, (f, c) in enumerate(zip(given, copies)):
            assert np.array_equal(f, c), "the buffer of brick %d was written" % b
        loc_ref = np.full(nst, C.SENTINEL, np.uint32)
        L.locate(nst, avail_mask, frags, loc_ref)
        heal_ref = [np.empty(C.CHUNK * nst, np.uint8) for _ in targets]
        L.heal(nst, C.mask_of(basis), [frags[b] for b in basis], tmask, heal_ref)
        return dict(loc=loc[:nst], out=[o[:C.CHUNK * nst] for o in out], nbad=nbad, nmany=nmany,
                    loc_ref=loc_ref, heal_ref=heal_ref)
    return run


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("nst", C.SIZES)
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_heal_checked_matches_contract(ec, oracle, geom, nst, gen):
    k, n, avail_mask, targets = geom
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        C.run_geometry(host_runner(L, k, n, nst, avail_mask, targets), oracle, k, n, avail_mask,
                       targets, nst)


def _mixed(oracle):
    """8+4 with bricks 4 and 7 to heal, 5 stripes: clean, clean, basis brick
    1, clean, MANY (basis brick 0 and check brick 11)."""
    k, n, nst = 8, 12, 5
    clean = C.fragments(oracle, k, n, nst)
    frags = list(clean)
    frags[1] = C.flipped(frags[1], 2, 100, 1)
    frags[0] = C.flipped(frags[0], 4, 7, 1)
    frags[11] = C.flipped(frags[11], 4, 8, 1)
    frags[4] = frags[7] = None
    return k, n, nst, clean, frags


def test_heal_checked_leaves_stats_alone(ec, oracle):
    """Clean, corrected and MANY stripes in one call, on a gen=none and on a
    gen=auto volume: ec_method_get_stats does not move."""
    k, n, nst, clean, frags = _mixed(oracle)
    out = [np.full(C.CHUNK * nst, C.FILL, np.uint8) for _ in range(2)]
    loc = np.full(nst, C.SENTINEL, np.uint32)
    for gen in ("none", None):
        with (ec.ECMatrixList(k, n, gen=gen) if gen else ec.ECMatrixList(k, n)) as L:
            s0 = ec.stats()
            assert L.heal_checked(nst, 0xF6F, frags, 0x90, out, loc) == (2, 1)
            assert ec.stats() == s0, "ec_method_heal_checked touched ec_method_stats_t"
        assert loc.tolist() == [0, 0, 1 << 1, 0, C.MANY]
        for o, j in zip(out, (4, 7)):
            assert np.array_equal(o[:4 * C.CHUNK], clean[j][:4 * C.CHUNK])
            assert not np.array_equal(o[4 * C.CHUNK:], clean[j][4 * C.CHUNK:])


def _call(ec, L, nst, mask, frags, tmask, out, loc, nbad, nmany):
    return ec.lib.ec_method_heal_checked(
        ctypes.byref(L._list) if L is not None else None, nst, mask,
        None if frags is None else ec._ptr_array(frags), tmask,
        None if out is None else ec._ptr_array(out), loc,
        None if nbad is None else ctypes.byref(nbad),
        None if nmany is None else ctypes.byref(nmany))


def test_heal_checked_zero_stripes_is_a_noop(ec):
    frags = [np.zeros(C.CHUNK, np.uint8) for _ in range(12)]
    out = [np.full(C.CHUNK, C.FILL, np.uint8) for _ in range(2)]
    loc = np.full(4, C.SENTINEL, np.uint32)
    nbad, nmany = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(8, 12, gen="none") as L:
        assert _call(ec, L, 0, 0xF6F, frags, 0x90, out, loc.ctypes.data, nbad, nmany) == 0
        # the argument checks come first
        for mask, tmask, o in ((0x16F, 0x90, out), (0xF6F, 0, out), (0xF6F, 0x91, out),
                               (0xF6F, 0x90, None), (0xF6F, 0x90, [out[0], None])):
            rc = _call(ec, L, 0, mask, frags, tmask, o, loc.ctypes.data, nbad, nmany)
            assert rc == -errno.EINVAL, (hex(mask), hex(tmask))
    assert (loc == C.SENTINEL).all() and all((o == C.FILL).all() for o in out)
    assert nbad.value == 77 and nmany.value == 78


@pytest.mark.parametrize("null", ["nbad", "nmany", "both"])
def test_heal_checked_counters_may_be_null(ec, oracle, null):
    k, n, nst, clean, frags = _mixed(oracle)
    out = [np.full(C.CHUNK * nst, C.FILL, np.uint8) for _ in range(2)]
    loc = np.full(nst, C.SENTINEL, np.uint32)
    nbad, nmany = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(k, n, gen="none") as L:
        rc = _call(ec, L, nst, 0xF6F, frags, 0x90, out, loc.ctypes.data,
                   None if null in ("nbad", "both") else nbad,
                   None if null in ("nmany", "both") else nmany)
    assert rc == 0
    assert loc.tolist() == [0, 0, 1 << 1, 0, C.MANY]
    for o, j in zip(out, (4, 7)):
        assert np.array_equal(o[:4 * C.CHUNK], clean[j][:4 * C.CHUNK])
    assert nbad.value == (77 if null in ("nbad", "both") else 2)
    assert nmany.value == (78 if null in ("nmany", "both") else 1)


def _einval_cases():
    """(name, k, n, overrides) of a valid call: every brick but the highest
    available, the highest one healed."""
    return [
        ("list NULL", 8, 12, dict(list_null=True)),
        ("frags NULL", 8, 12, dict(frags=None)),
        ("out NULL", 8, 12, dict(out=None)),
        ("out[0] NULL", 8, 12, dict(mask=0xF6F, tmask=0x90, out_null=0)),
        ("out[1] NULL", 8, 12, dict(mask=0xF6F, tmask=0x90, out_null=1)),
        ("loc NULL", 8, 12, dict(loc=None)),
        ("loc not 4-byte aligned", 8, 12, dict(loc_off=2)),
        ("avail_mask with a brick at n", 8, 12, dict(mask=0x13FF)),
        ("avail_mask above n only", 8, 12, dict(mask=0xFFF000)),
        ("k + 1 bricks", 8, 12, dict(mask=0x1FF)),
        ("k + 1 bricks, a high set", 8, 12, dict(mask=0x7FC)),
        ("k bricks", 8, 12, dict(mask=0xFF)),
        ("empty avail_mask", 8, 12, dict(mask=0)),
        ("frags[0] NULL", 8, 12, dict(null=0)),
        ("frags[10] NULL", 8, 12, dict(null=10)),
        ("empty target_mask", 8, 12, dict(tmask=0)),
        ("target_mask with a brick at n", 8, 12, dict(tmask=0x1800)),
        ("target_mask above n only", 8, 12, dict(tmask=0x1000)),
        ("target_mask overlaps a basis brick", 8, 12, dict(tmask=0x801)),
        ("target_mask overlaps a check brick", 8, 12, dict(tmask=0xC00)),
        ("target_mask inside avail_mask", 8, 12, dict(tmask=0x400)),
        ("4+2 volume, every brick, a target above n", 4, 6, dict(mask=0x3F, tmask=0x40)),
        ("4+2 volume, k + 1 bricks", 4, 6, dict(mask=0x1F, tmask=0x20)),
        ("4+2 volume, k + 2 bricks overlapped", 4, 6, dict(mask=0x3F, tmask=0x20)),
        ("2+1 volume, every brick", 2, 3, dict(mask=0x7, tmask=0x4)),
        ("2+1 volume, two bricks", 2, 3, dict(mask=0x3, tmask=0x4)),
        ("4+3 volume, k + 1 bricks", 4, 7, dict(mask=0x37, tmask=0x48)),
    ]


@pytest.mark.parametrize("name,k,n,ov", _einval_cases(), ids=[c[0] for c in _einval_cases()])
def test_heal_checked_einval(ec, name, k, n, ov):
    nst = 2
    frags = [np.zeros(C.CHUNK * nst, np.uint8) for _ in range(n)]
    store = np.full(nst + 2, C.SENTINEL, np.uint32)
    mask = ov.get("mask", (1 << (n - 1)) - 1)
    tmask = ov.get("tmask", 1 << (n - 1))
    obufs = [np.full(C.CHUNK * nst, C.FILL, np.uint8) for _ in range(max(1, bin(tmask).count("1")))]
    out = None if "out" in ov else list(obufs)
    if "out_null" in ov:
        out[ov["out_null"]] = None
    if "null" in ov:
        frags[ov["null"]] = None
    loc = None if "loc" in ov else store.ctypes.data + ov.get("loc_off", 0)
    nbad, nmany = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(k, n, gen="none") as L:
        rc = _call(ec, None if ov.get("list_null") else L, nst, mask,
                   None if "frags" in ov else frags, tmask, out, loc, nbad, nmany)
        err = (ec.lib.ec_method_last_error() or b"").decode()
    assert rc == -errno.EINVAL, (name, rc)
    assert "ec_method_heal_checked" in err and "ec_method_heal_checked_device" not in err, err
    assert (store == C.SENTINEL).all(), "a rejected call wrote loc"
    assert all((o == C.FILL).all() for o in obufs), "a rejected call wrote a target"
    assert nbad.value == 77 and nmany.value == 78, "a rejected call wrote its counters"


def test_heal_checked_ignores_entries_outside_avail_mask(ec, oracle):
    """Bricks outside avail_mask are not read: a NULL entry and a damaged
    fragment there change nothing, whether the brick is a target or not."""
    k, n, nst, avail_mask = 8, 12, 5, 0xF6F
    clean = C.fragments(oracle, k, n, nst)
    frags = list(clean)
    frags[4] = None
    frags[7] = np.full(C.CHUNK * nst, 0xA5, np.uint8)
    out = [np.full(C.CHUNK * nst, C.FILL, np.uint8)]
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        for j in (4, 7):
            assert L.heal_checked(nst, avail_mask, frags, 1 << j, out, loc) == (0, 0)
            assert not loc.any()
            assert np.array_equal(out[0], clean[j])


def test_heal_checked_device_rejects_host_buffers(ec):
    """Host buffers given to the device entry point: -EINVAL, GPU or not."""
    nst = 2
    frags = [np.zeros(C.CHUNK * nst, np.uint8) for _ in range(12)]
    out = [np.full(C.CHUNK * nst, C.FILL, np.uint8) for _ in range(2)]
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(8, 12, gen="none") as L:
        with pytest.raises(OSError) as e:
            L.heal_checked_device(0, None, nst, 0xF6F, frags, 0x90, out, loc)
    assert e.value.errno == errno.EINVAL
    assert "ec_method_heal_checked_device" in str(e.value)
    assert (loc == C.SENTINEL).all() and all((o == C.FILL).all() for o in out)
