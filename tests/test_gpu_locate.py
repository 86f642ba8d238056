"""ec_method_locate_device: the damaged brick per stripe on device-resident
fragments (ec_locate_n, ec_kernels_impl.h).  The geometries, sizes and
corruptions of tests/test_locate.py on torch device tensors, with expected
values from the oracle and the definition (tests/_locate_cases.py), plus what
only the kernel can get wrong: many blocks with a ragged last tile (1027
stripes), tiles that take the early out beside tiles that do not, four
different outcomes inside one tile, fragments at an odd byte address, the
largest tile (16+15: 31 inputs, 15 syndromes, 62 KiB of LDS), a caller's
stream, and 2^15 stripes so that every CU holds several tiles.  loc[] is
pre-filled with 0xFFFFFFFF and followed by guard words that must not change.
"""
import errno

import numpy as np
import pytest

import _locate_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def dev(a, offset=0):
    """A device copy of numpy array `a`, starting `offset` bytes into its
    allocation."""
    import torch
    t = torch.empty(a.nbytes + offset, dtype=torch.uint8, device=DEV)
    v = t[offset:]
    v.copy_(torch.from_numpy(np.array(a, dtype=np.uint8)))    # (a may be read-only)
    return v


def new_loc(nst):
    import torch
    return torch.full((nst + C.GUARD,), -1, dtype=torch.int32, device=DEV)


def read_loc(loc, nst):
    got = loc.cpu().numpy().view(np.uint32)
    assert (got[nst:] == C.SENTINEL).all(), "guard words written"
    return got[:nst].copy()


def device_runner(ec, L, nst, avail_mask, stream=None, offsets=None):
    """Clean fragments are uploaded once and shared by the cases; a case's
    corrupted copies are uploaded for that call."""
    import torch
    offs = offsets or {}
    kept = {}

    def run(frags):
        dfr = []
        for b, a in enumerate(frags):
            if a is None:
                dfr.append(None)
            elif not a.flags.writeable:                      # a clean, shared fragment
                if b not in kept:
                    kept[b] = dev(a, offs.get(b, 0))
                dfr.append(kept[b])
            else:
                dfr.append(dev(a, offs.get(b, 0)))
        loc = new_loc(nst)
        torch.cuda.synchronize()
        L.locate_device(0, stream, nst, avail_mask, dfr, loc)
        ec.sync_device(0, stream)
        return read_loc(loc, nst), None
    return run


@pytest.mark.parametrize("nst", C.SIZES + [1027])
@pytest.mark.parametrize("geom", C.GEOMS + [C.GEOM_LARGEST], ids=C.geom_id)
def test_locate_device_matches_definition(ec, oracle, geom, nst):
    k, n, avail_mask = geom
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_locate_device_fragments_at_odd_addresses(ec, oracle):
    """16+4 with a basis fragment and a check fragment starting 1 byte into
    their allocations: LDS-DMA stages them in place."""
    k, n, avail_mask, nst = 16, 20, 0xBFFFD, 67
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask, offsets={5: 1, 19: 1}), oracle, k, n,
                       avail_mask, nst)


def test_locate_device_largest_tile(ec, oracle):
    """A 16+15 volume with every brick: 31 staged inputs, 15 syndromes."""
    k, n, avail_mask = C.GEOM_LARGEST
    nst = 9
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_locate_device_on_a_callers_stream(ec, oracle):
    import torch
    k, n, avail_mask, nst = 8, 12, 0xF6F, 67
    st = torch.cuda.Stream()
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask, stream=st.cuda_stream), oracle, k, n,
                       avail_mask, nst)


def test_locate_device_at_scale(ec, oracle):
    """8+4 with all 12 bricks, 2^15 stripes (16 MiB per fragment, several
    tiles per CU), 97 seeded single-bit flips in distinct stripes spread over
    all 12 bricks.  The fragments are oracle-encoded once; the expectation is
    the MDS rule: one damaged chunk in brick b gives 1 << b.  All 2^15 entries
    are compared."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 1 << 15
    frags = C.fragments(oracle, k, n, nst)
    dfr = [dev(f) for f in frags]
    rng = np.random.default_rng(97)
    stripes = rng.choice(nst, size=97, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    want = np.zeros(nst, np.uint32)
    for j, t in enumerate(stripes.tolist()):
        b = j % n
        off = t * C.CHUNK + int(rng.integers(0, C.CHUNK))
        dfr[b][off] ^= 1 << int(rng.integers(0, 8))
        want[t] = 1 << b
    assert np.count_nonzero(want) == 97
    loc = new_loc(nst)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.locate_device(0, None, nst, avail_mask, dfr, loc)
        ec.sync_device(0)
    got = read_loc(loc, nst)
    C._frag_cache.pop((k, n, nst))          # 192 MiB: not kept for the session
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:16]


def test_locate_rejects_mixed_host_and_device_buffers(ec, oracle):
    """Device tensors given to the host entry point, host arrays to the device
    entry point, all of them or mixed: -EINVAL, nothing written."""
    k, n, nst = 4, 6, 4
    frags = list(C.fragments(oracle, k, n, nst))
    dfr = [dev(f) for f in frags]
    hloc = np.full(nst, C.SENTINEL, np.uint32)
    dloc = new_loc(nst)
    with ec.ECMatrixList(k, n) as L:
        for fr, loc in (
                (dfr, dloc),                                   # all on the device
                (dfr, hloc),
                ([frags[0], dfr[1]] + frags[2:], hloc),        # a basis brick
                (frags[:5] + [dfr[5]], hloc),                  # a check brick
                (frags, dloc)):
            with pytest.raises(OSError) as e:
                L.locate(nst, 0x3F, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_locate" in str(e.value)
        for fr, loc in (
                ([dfr[0], frags[1]] + dfr[2:], dloc),
                (dfr[:4] + [frags[4], dfr[5]], dloc),
                (dfr, hloc)):
            with pytest.raises(OSError) as e:
                L.locate_device(0, None, nst, 0x3F, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_locate_device" in str(e.value)
        ec.sync_device(0)
    assert (hloc == C.SENTINEL).all()
    assert (dloc.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
