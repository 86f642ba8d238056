"""ec_method_locate2 on host buffers: which one or two bricks' chunks are
wrong, per stripe, in one pass.  No GPU is needed: the host entry point runs
on the calling thread's CPU engine for every gen.

Expected values come from the oracle and the definition (tests/
_locate2_cases.py).  Geometries 5+4, 4+4, 8+4 and 16+4 with every brick and
16+6 with two bricks missing (a - k = 4 throughout); 1, 3, 4, 5 and 67
stripes; clean fragments, locate's single-brick cases, pairs of every kind
(basis + basis, basis + check, check + check) damaged at different symbols, at
one symbol, in different planes and as whole random chunks, three damaged
bricks, a tile of four different outcomes and a pair in a ragged last tile.
Every case is also given to ec_method_locate and the two answers compared as
the header promises.  loc[] is pre-filled with 0xFFFFFFFF and followed by
guard words that must not change.  One round trip per geometry heals the pair
locate2 names with ec_method_heal, as the header documents.
"""
import ctypes
import errno

import numpy as np
import pytest

import _locate2_cases as C

GENS = ["none", "avx"]


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def host_runner(L, nst, avail_mask):
    def run(frags):
        loc = np.full(nst + C.GUARD, C.SENTINEL, np.uint32)
        nbad = L.locate2(nst, avail_mask, frags, loc)
        assert (loc[nst:] == C.SENTINEL).all(), "guard words written"
        loc1 = np.full(nst, C.SENTINEL, np.uint32)
        L.locate(nst, avail_mask, frags, loc1)
        return loc[:nst], nbad, loc1
    return run


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("nst", C.SIZES)
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_locate2_matches_definition(ec, oracle, geom, nst, gen):
    k, n, avail_mask = geom
    s0 = ec.stats()
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        C.run_geometry(host_runner(L, nst, avail_mask), oracle, k, n, avail_mask, nst)
    assert ec.stats() == s0, "ec_method_locate2 touched ec_method_stats_t"


def test_locate2_runs_on_cpu_engine_for_auto_volume(ec, oracle):
    """A gen=auto volume (GPU visible or not) locates in host buffers on the
    CPU engine too, without counting an engine run."""
    k, n, avail_mask, nst = 5, 9, 0x1FF, 5
    s0 = ec.stats()
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(host_runner(L, nst, avail_mask), oracle, k, n, avail_mask, nst)
    assert ec.stats() == s0


def heal_pair(heal, k, avail_mask, frag_addr, t, loc_t):
    """Act on loc[t] = two bits as include/ec_method.h documents: heal that
    one stripe from the k lowest other bricks of avail_mask, in place."""
    named = C.bits(loc_t)
    assert len(named) == 2
    src = [b for b in C.bits(avail_mask) if b not in named][:k]
    off = t * C.CHUNK
    heal(1, sum(1 << b for b in src), [frag_addr[b] + off for b in src],
         loc_t, [frag_addr[b] + off for b in named])


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_locate2_then_heal_round_trip(ec, oracle, geom):
    k, n, avail_mask = geom
    nst = 5
    clean = C.fragments(oracle, k, n, nst)
    avail = C.bits(avail_mask)
    rng = np.random.default_rng(5 * k + n)
    frags = [clean[b].copy() if b in avail else None for b in range(n)]
    t, b1, b2 = 3, avail[1], avail[k + 1]            # a basis and a check brick
    for b in (b1, b2):
        frags[b][t * C.CHUNK:(t + 1) * C.CHUNK] = rng.integers(0, 256, C.CHUNK, dtype=np.uint8)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        assert L.locate2(nst, avail_mask, frags, loc) == 1
        want = np.zeros(nst, np.uint32)
        want[t] = 1 << b1 | 1 << b2
        assert np.array_equal(loc, want)
        heal_pair(L.heal, k, avail_mask, {b: frags[b].ctypes.data for b in avail}, t,
                  int(loc[t]))
        for b in avail:
            assert np.array_equal(frags[b], clean[b]), b
        assert L.locate2(nst, avail_mask, frags, loc) == 0
    assert not loc.any()


def test_locate2_zero_stripes_is_a_noop(ec):
    frags = [np.zeros(C.CHUNK, np.uint8) for _ in range(9)]
    loc = np.full(4, C.SENTINEL, np.uint32)
    nbad = ctypes.c_uint64(77)
    with ec.ECMatrixList(5, 9, gen="none") as L:
        rc = ec.lib.ec_method_locate2(ctypes.byref(L._list), 0, 0x1FF, ec._ptr_array(frags),
                                      loc.ctypes.data, ctypes.byref(nbad))
        assert rc == 0
        # the argument checks come first
        rc = ec.lib.ec_method_locate2(ctypes.byref(L._list), 0, 0xFF, ec._ptr_array(frags),
                                      loc.ctypes.data, ctypes.byref(nbad))
        assert rc == -errno.EINVAL
    assert (loc == C.SENTINEL).all() and nbad.value == 77


def test_locate2_nbad_may_be_null(ec, oracle):
    k, n, nst = 5, 9, 3
    frags = list(C.fragments(oracle, k, n, nst))
    frags[1] = C.flipped(frags[1], 2, 100, 1)
    frags[7] = C.flipped(frags[7], 2, 101, 1)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        rc = ec.lib.ec_method_locate2(ctypes.byref(L._list), nst, 0x1FF, ec._ptr_array(frags),
                                      loc.ctypes.data, None)
    assert rc == 0
    assert loc.tolist() == [0, 0, 1 << 1 | 1 << 7]


def _einval_cases():
    """(name, k, n, overrides) of a valid call with every brick available."""
    return [
        ("list NULL", 5, 9, dict(list_null=True)),
        ("frags NULL", 5, 9, dict(frags=None)),
        ("loc NULL", 5, 9, dict(loc=None)),
        ("loc not 4-byte aligned", 5, 9, dict(loc_off=2)),
        ("avail_mask with a brick at n", 5, 9, dict(mask=0x3FF)),
        ("avail_mask above n only", 5, 9, dict(mask=0x3FE00)),
        ("k + 3 bricks", 5, 9, dict(mask=0xFF)),
        ("k + 3 bricks, a high set", 5, 9, dict(mask=0x1FE)),
        ("k + 2 bricks", 5, 9, dict(mask=0x7F)),
        ("k bricks", 5, 9, dict(mask=0x1F)),
        ("empty avail_mask", 5, 9, dict(mask=0)),
        ("frags[0] NULL", 5, 9, dict(null=0)),
        ("frags[8] NULL", 5, 9, dict(null=8)),
        ("4+2 volume, every brick", 4, 6, dict(mask=0x3F)),
        ("2+1 volume, every brick", 2, 3, dict(mask=0x7)),
        ("8+4 with k + 3 bricks", 8, 12, dict(mask=0x7FF)),
        ("16+4 with k + 3 bricks", 16, 20, dict(mask=0xFFFFE)),
    ]


@pytest.mark.parametrize("name,k,n,ov", _einval_cases(), ids=[c[0] for c in _einval_cases()])
def test_locate2_einval(ec, name, k, n, ov):
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
        rc = ec.lib.ec_method_locate2(lst, nst, ov.get("mask", (1 << n) - 1), fr, loc,
                                      ctypes.byref(nbad))
        err = (ec.lib.ec_method_last_error() or b"").decode()
    assert rc == -errno.EINVAL, (name, rc)
    assert "ec_method_locate2" in err and "ec_method_locate2_device" not in err, err
    assert (store == C.SENTINEL).all() and nbad.value == 77, "a rejected call wrote its outputs"


def test_locate2_ignores_entries_outside_avail_mask(ec, oracle):
    """Bricks outside avail_mask are not read: a NULL entry and a damaged
    fragment there change nothing."""
    k, n, nst, avail_mask = 16, 22, 5, 0x3BFFFD
    frags = list(C.fragments(oracle, k, n, nst))
    frags[1] = None
    frags[18] = np.full(C.CHUNK * nst, 0xA5, np.uint8)
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        assert L.locate2(nst, avail_mask, frags, loc) == 0
    assert not loc.any()


def test_locate2_device_rejects_host_buffers(ec):
    """Host buffers given to the device entry point: -EINVAL, GPU or not."""
    nst = 2
    frags = [np.zeros(C.CHUNK * nst, np.uint8) for _ in range(9)]
    loc = np.full(nst, C.SENTINEL, np.uint32)
    with ec.ECMatrixList(5, 9, gen="none") as L:
        with pytest.raises(OSError) as e:
            L.locate2_device(0, None, nst, 0x1FF, frags, loc)
    assert e.value.errno == errno.EINVAL
    assert "ec_method_locate2_device" in str(e.value)
    assert (loc == C.SENTINEL).all()
