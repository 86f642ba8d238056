"""ec_method_locate on host buffers: which brick's chunk is wrong, per stripe,
in one pass.  No GPU is needed: the host entry point runs on the calling
thread's CPU engine for every gen.

Expected values come from the oracle and the definition (tests/
_locate_cases.py).  Geometries 4+2, 8+4 and 16+4 with every brick and with
bricks missing (a non-contiguous basis); 1, 3, 4, 5 and 67 stripes; clean
fragments, single-bit flips in every plane in the first and last basis brick
and the first and last check brick, whole random chunks, two damaged bricks
at different and at the same symbol, a tile of four different outcomes and a
dirty ragged last tile.  loc[] is pre-filled with 0xFFFFFFFF and followed by
guard words that must not change.
"""
import ctypes
import errno

import numpy as np
import pytest

import _locate_cases as C

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def host_runner(L, nst, avail_mask):
    def run(frags):
        loc = np.full(nst + C.GUARD, C.SENTINEL, np.uint32)
        nbad = L.locate(nst, avail_mask, frags, loc)
        assert (loc[nst:] == C.SENTINEL).all(), "guard words written"
        return loc[:nst], nbad
    return run


def test_many_is_the_header_value(ec):
    assert ec.EC_MI355X_LOCATE_MANY == C.MANY


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("nst", C.SIZES)
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_locate_matches_definition(ec, oracle, geom, nst, gen):
    k, n, avail_mask = geom
    s0 = ec.stats()
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        C.run_geometry(host_runner(L, nst, avail_mask), oracle, k, n, avail_mask, nst)
    assert ec.stats() == s0, "ec_method_locate touched ec_method_stats_t"


def test_locate_runs_on_cpu_engine_for_auto_volume(ec, oracle):
    """A gen=auto volume (GPU visible or not) locates in host buffers on the
    CPU engine too, without counting an engine run."""
    k, n, avail_mask, nst = 4, 6, 0x3F, 5
    s0 = ec.stats()
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(host_runner(L, nst, avail_mask), oracle, k, n, avail_mask, nst)
    assert ec.stats() == s0


def test_locate_zero_stripes_is_a_noop(ec):
    frags = [np.zeros(C.CHUNK, np.uint8) for _ in range(6)]
    loc = np.full(4, C.SENTINEL, np.uint32)
    nbad = ctypes.c_uint64(77)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        rc = ec.lib.ec_method_locate(ctypes.byref(L._list), 0, 0x3F, ec._ptr_array(frags),
                                     loc.ctypes.data, ctypes.byref(nbad))
        assert rc == 0
        # the argument checks come first
        rc = ec.lib.ec_method_locate(ctypes.byref(L._list), 0, 0x1F, ec._ptr_array(frags),
                                     loc.ctypes.data, ctypes.byref(nbad))
        assert rc == -errno.EINVAL
    assert (loc == C.SENTINEL).all() and nbad.value == 77


def test_locate_nbad_may_be_null(ec, oracle):
    k, n, nst = 4, 6, 3
    frags = list(C.fragments(oracle, k, n, nst))
    frags[1] = C.flipped(frags[1], 2, 100, 1)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        rc = ec.lib.ec_method_locate(ctypes.byref(L._list), nst, 0x3F, ec._ptr_array(frags),
                                     loc.ctypes.data, None)
    assert rc == 0
    assert loc.tolist() == [0, 0, 1 << 1]


def _einval_cases():
    """(name, k, n, overrides) of a valid call with every brick available."""
    return [
        ("list NULL", 4, 6, dict(list_null=True)),
        ("frags NULL", 4, 6, dict(frags=None)),
        ("loc NULL", 4, 6, dict(loc=None)),
        ("loc not 4-byte aligned", 4, 6, dict(loc_off=2)),
        ("avail_mask with a brick at n", 4, 6, dict(mask=0x7F)),
        ("avail_mask above n only", 4, 6, dict(mask=0xFC0)),
        ("k + 1 bricks", 4, 6, dict(mask=0x1F)),
        ("k + 1 bricks, a high set", 4, 6, dict(mask=0x3E)),
        ("k bricks", 4, 6, dict(mask=0x0F)),
        ("empty avail_mask", 4, 6, dict(mask=0)),
        ("frags[0] NULL", 4, 6, dict(null=0)),
        ("frags[5] NULL", 4, 6, dict(null=5)),
        ("2+1 volume, every brick", 2, 3, dict(mask=0x7)),
        ("2+1 volume, two bricks", 2, 3, dict(mask=0x3)),
        ("8+4 with k + 1 bricks", 8, 12, dict(mask=0x1FF)),
    ]


@pytest.mark.parametrize("name,k,n,ov", _einval_cases(), ids=[c[0] for c in _einval_cases()])
def test_locate_einval(ec, name, k, n, ov):
    nst = 2
    frags = [np.zeros(C.CHUNK * nst, np.uint8) for _ in range(n)]
    store = np.full(nst + 2, C.SENTINEL, np.uint32)
    if "null" in ov:
        frags[ov["null"]] = None
    fr = None if "frags" in ov else ec._ptr_array(frags)
    loc = None if "loc" in ov else store.ctypes.data + ov.get("loc_off", 0)
    nbad = ctypes.c_uint64(77)
    with ec.ECMatrixList(k, n, gen="none") as L:
        lst = None if ov.get("list_null") else ctypes.byref(L._list)
        rc = ec.lib.ec_method_locate(lst, nst, ov.get("mask", (1 << n) - 1), fr, loc,
                                     ctypes.byref(nbad))
        err = (ec.lib.ec_method_last_error() or b"").decode()
    assert rc == -errno.EINVAL, (name, rc)
    assert "ec_method_locate" in err and "ec_method_locate_device" not in err, err
    assert (store == C.SENTINEL).all() and nbad.value == 77, "a rejected call wrote its outputs"


def test_locate_ignores_entries_outside_avail_mask(ec, oracle):
    """Bricks outside avail_mask are not read: a NULL entry and a damaged
    fragment there change nothing."""
    k, n, nst, avail_mask = 8, 12, 5, 0xF6F
    frags = list(C.fragments(oracle, k, n, nst))
    frags[4] = None
    frags[7] = np.full(C.CHUNK * nst, 0xA5, np.uint8)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        assert L.locate(nst, avail_mask, frags, loc) == 0
    assert not loc.any()


def test_locate_device_rejects_host_buffers(ec):
    """Host buffers given to the device entry point: -EINVAL, GPU or not."""
    nst = 2
    frags = [np.zeros(C.CHUNK * nst, np.uint8) for _ in range(6)]
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        with pytest.raises(OSError) as e:
            L.locate_device(0, None, nst, 0x3F, frags, loc)
    assert e.value.errno == errno.EINVAL
    assert "ec_method_locate_device" in str(e.value)
    assert (loc == C.SENTINEL).all()
