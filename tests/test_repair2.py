"""ec_method_repair2 on host buffers: rewrite the one or two chunks loc[]
names, and only those.  No GPU is needed: the host entry point runs on the
calling thread's CPU engine for every gen.

Expected bytes come from the oracle (tests/_repair2_cases.py).  Geometries
4+2 with every brick and 8+4 with two bricks missing (a = k + 2, hand-made
loc[]), 5+4, 4+4, 8+4, 16+4 with every brick and 16+6 with two missing
(locate2 -> repair2 -> locate2); 1, 3, 4, 5 and 67 stripes; the seven kinds of
pair damaged in four ways, locate's single-brick classes, MANY stripes left
alone, hand-made loc[] that pins the basis rule, single bits against
ec_method_repair, values that must be ignored, and the dense loc[] arrays that
exercise the kernel's wave logic on the GPU.  Every fragment is compared
whole, with a guard chunk behind it.
"""
import ctypes
import errno

import numpy as np
import pytest

import _repair2_cases as R2

GENS = ["none", "avx"]
CHUNK = R2.CHUNK


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


class HostOps:
    def __init__(self, L, nst, avail_mask):
        self.L, self.nst, self.mask = L, nst, avail_mask

    def _bufs(self, frags):
        full = [None if f is None else R2.with_guard(f) for f in frags]
        return full, [None if f is None else f[:self.nst * CHUNK] for f in full]

    def repair2(self, frags, loc):
        full, view = self._bufs(frags)
        counts = self.L.repair2(self.nst, self.mask, view, loc)
        return full, loc, counts

    def repair(self, frags, loc):
        full, view = self._bufs(frags)
        counts = self.L.repair(self.nst, self.mask, view, loc)
        return full, loc, counts

    def scrub2(self, frags):
        full, view = self._bufs(frags)
        loc = np.full(self.nst, 0xFFFFFFFF, np.uint32)
        loc2 = loc.copy()
        self.L.locate2(self.nst, self.mask, view, loc)
        keep = loc.copy()
        counts = self.L.repair2(self.nst, self.mask, view, loc)
        assert np.array_equal(loc, keep), "loc[] written"
        self.L.locate2(self.nst, self.mask, view, loc2)
        return loc, full, loc2, counts


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("nst", R2.SIZES)
@pytest.mark.parametrize("geom", R2.GEOMS, ids=R2.geom_id)
def test_repair2_matches_oracle(ec, oracle, geom, nst, gen):
    k, n, avail_mask = geom
    s0 = ec.stats()
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        R2.run_geometry(HostOps(L, nst, avail_mask), oracle, k, n, avail_mask, nst)
    assert ec.stats() == s0, "ec_method_repair2 touched ec_method_stats_t"


def test_repair2_runs_on_cpu_engine_for_auto_volume(ec, oracle):
    k, n, avail_mask, nst = 4, 8, 0xFF, 5
    s0 = ec.stats()
    with ec.ECMatrixList(k, n) as L:
        R2.run_geometry(HostOps(L, nst, avail_mask), oracle, k, n, avail_mask, nst)
    assert ec.stats() == s0


def _call(ec, L, nst, mask, frags, loc, done, skipped):
    return ec.lib.ec_method_repair2(ctypes.byref(L._list), nst, mask, ec._ptr_array(frags), loc,
                                    done, skipped)


def test_repair2_zero_stripes_is_a_noop(ec):
    frags = [np.full(CHUNK, 0x5A, np.uint8) for _ in range(6)]
    loc = np.full(4, 3, np.uint32)
    done, skipped = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        assert _call(ec, L, 0, 0x3F, frags, loc.ctypes.data, ctypes.byref(done),
                     ctypes.byref(skipped)) == 0
        # the argument checks come first: a = k + 1
        assert _call(ec, L, 0, 0x1F, frags, loc.ctypes.data, ctypes.byref(done),
                     ctypes.byref(skipped)) == -errno.EINVAL
    assert all((f == 0x5A).all() for f in frags) and (loc == 3).all()
    assert (done.value, skipped.value) == (77, 78)


def test_repair2_counters_may_be_null(ec, oracle):
    k, n, nst = 4, 6, 3
    clean = R2.fragments(oracle, k, n, nst)

    def hurt():
        fr = [f.copy() for f in clean]
        fr[1] = R2.flipped(fr[1], 2, 100, 1)
        fr[4] = R2.flipped(fr[4], 2, 101, 1)
        return fr

    loc = np.array([0, R2.MANY, 1 << 1 | 1 << 4], np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        frags = hurt()
        assert _call(ec, L, nst, 0x3F, frags, loc.ctypes.data, None, None) == 0
        for b in range(n):
            assert np.array_equal(frags[b], clean[b])
        frags, done, skipped = hurt(), ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert _call(ec, L, nst, 0x3F, frags, loc.ctypes.data, ctypes.byref(done), None) == 0
        assert done.value == 1
        frags = hurt()
        assert _call(ec, L, nst, 0x3F, frags, loc.ctypes.data, None, ctypes.byref(skipped)) == 0
        assert skipped.value == 1
    for b in range(n):
        assert np.array_equal(frags[b], clean[b])


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
def test_repair2_einval(ec, name, k, n, ov):
    nst = 2
    frags = [np.full(CHUNK * nst, 0x5A, np.uint8) for _ in range(n)]
    keep = list(frags)
    store = np.full(nst + 2, 3, np.uint32)
    if "null" in ov:
        frags[ov["null"]] = None
    fr = None if "frags" in ov else ec._ptr_array(frags)
    loc = None if "loc" in ov else store.ctypes.data + ov.get("loc_off", 0)
    done, skipped = ctypes.c_uint64(77), ctypes.c_uint64(78)
    with ec.ECMatrixList(k, n, gen="none") as L:
        lst = None if ov.get("list_null") else ctypes.byref(L._list)
        rc = ec.lib.ec_method_repair2(lst, nst, ov.get("mask", (1 << n) - 1), fr, loc,
                                      ctypes.byref(done), ctypes.byref(skipped))
        err = (ec.lib.ec_method_last_error() or b"").decode()
    assert rc == -errno.EINVAL, (name, rc)
    assert "ec_method_repair2" in err and "ec_method_repair2_device" not in err, err
    assert all((f == 0x5A).all() for f in keep) and (store == 3).all(), "a rejected call wrote"
    assert (done.value, skipped.value) == (77, 78)


def test_repair2_k_plus_two_bricks_is_enough(ec, oracle):
    """A 4+2 volume with every brick, which locate2 rejects: a = k + 2.  Every
    pair of bricks, damaged and named by the caller."""
    k, n, nst = 4, 6, 5
    clean = R2.fragments(oracle, k, n, nst)
    with ec.ECMatrixList(k, n, gen="none") as L:
        for i in range(n):
            for j in range(i + 1, n):
                frags = [f.copy() for f in clean]
                frags[i] = R2.flipped(frags[i], 3, 511, 7)
                frags[j] = R2.flipped(frags[j], 3, 0, 0)
                loc = np.zeros(nst, np.uint32)
                loc[3] = 1 << i | 1 << j
                assert L.repair2(nst, 0x3F, frags, loc) == (1, 0)
                for b in range(n):
                    assert np.array_equal(frags[b], clean[b]), (i, j, b)


def test_repair2_ignores_entries_outside_avail_mask(ec, oracle):
    """Bricks outside avail_mask are neither read nor written: a NULL entry
    and a damaged fragment there change nothing, and a pair naming one of
    them is ignored."""
    k, n, nst, avail_mask = 8, 12, 5, 0xF6F
    clean = R2.fragments(oracle, k, n, nst)
    frags = [f.copy() for f in clean]
    frags[4] = None
    frags[7] = np.full(CHUNK * nst, 0xA5, np.uint8)
    frags[0] = R2.flipped(frags[0], 1, 0, 0)
    frags[11] = R2.flipped(frags[11], 1, 1, 0)
    frags[3] = R2.flipped(frags[3], 2, 5, 5)
    loc = np.array([1 << 4 | 1 << 0, 1 << 0 | 1 << 11, 1 << 3 | 1 << 7, 0, 1 << 4 | 1 << 7],
                   np.uint32)
    with ec.ECMatrixList(k, n, gen="none") as L:
        assert L.repair2(nst, avail_mask, frags, loc) == (1, 3)
    assert (frags[7] == 0xA5).all()
    assert np.array_equal(frags[3], R2.flipped(clean[3], 2, 5, 5))
    for b in R2.bits(avail_mask):
        if b != 3:
            assert np.array_equal(frags[b], clean[b]), b


def test_repair2_device_rejects_host_buffers(ec):
    """Host buffers given to the device entry point: -EINVAL, GPU or not."""
    nst = 2
    frags = [np.full(CHUNK * nst, 0x5A, np.uint8) for _ in range(6)]
    loc = np.full(nst, 3, np.uint32)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        with pytest.raises(OSError) as e:
            L.repair2_device(0, None, nst, 0x3F, frags, loc)
    assert e.value.errno == errno.EINVAL
    assert "ec_method_repair2_device" in str(e.value)
    assert all((f == 0x5A).all() for f in frags)
