"""ec_method_verify_device: the consistency check on device-resident
fragments (ec_verify_n, ec_kernels_impl.h).  The geometries, masks, sizes and
corruptions of tests/test_verify.py on torch device tensors, with expected
flags from the oracle (tests/_verify_cases.py), plus what only the kernel can
get wrong: many blocks with a ragged last tile (1027 stripes), fragments at an
odd byte address, the largest tile (16+15: 31 inputs, 62 KiB of LDS), a
caller's stream, and 2^15 stripes so that every CU holds several tiles.
bad[] is pre-filled with 0xFFFFFFFF and followed by guard words that must not
change.
"""
import errno

import numpy as np
import pytest

import _verify_cases as V

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


def new_bad(nst):
    import torch
    return torch.full((nst + V.GUARD,), -1, dtype=torch.int32, device=DEV)


def read_bad(bad, nst):
    got = bad.cpu().numpy().view(np.uint32)
    assert (got[nst:] == V.SENTINEL).all(), "guard words written"
    return got[:nst].copy()


def device_runner(ec, L, nst, mask, check_mask, stream=None, offsets=None):
    import torch

    def run(ins, checks):
        offs = offsets or {}
        dins = [dev(a, offs.get(("in", p), 0)) for p, a in enumerate(ins)]
        dchk = [dev(a, offs.get(("check", j), 0)) for j, a in enumerate(checks)]
        bad = new_bad(nst)
        torch.cuda.synchronize()
        L.verify_device(0, stream, nst, mask, dins, check_mask, dchk, bad)
        ec.sync_device(0, stream)
        return read_bad(bad, nst), None
    return run


@pytest.mark.parametrize("nst", V.SIZES + [1027])
@pytest.mark.parametrize("geom", V.GEOMS, ids=V.geom_id)
def test_verify_device_matches_oracle(ec, oracle, geom, nst):
    k, n, mask, check_mask = geom
    with ec.ECMatrixList(k, n) as L:
        V.run_geometry(device_runner(ec, L, nst, mask, check_mask), oracle, k, n, mask,
                       check_mask, nst)


def test_verify_device_fragments_at_odd_addresses(ec, oracle):
    """16+4 with a basis fragment and a check fragment starting 1 byte into
    their allocations: LDS-DMA stages them in place."""
    k, n, mask, check_mask, nst = 16, 20, 0xFFFF0, 0x0000F, 67
    offsets = {("in", 5): 1, ("check", 2): 1}
    with ec.ECMatrixList(k, n) as L:
        V.run_geometry(device_runner(ec, L, nst, mask, check_mask, offsets=offsets), oracle, k, n,
                       mask, check_mask, nst)


def test_verify_device_largest_tile(ec, oracle):
    """A 16+15 volume, all 15 redundancy bricks checked: 31 staged inputs."""
    k, n, mask, check_mask, nst = 16, 31, 0xFFFF, 0x7FFF0000, 9
    with ec.ECMatrixList(k, n) as L:
        V.run_geometry(device_runner(ec, L, nst, mask, check_mask), oracle, k, n, mask,
                       check_mask, nst)


def test_verify_device_on_a_callers_stream(ec, oracle):
    import torch
    k, n, mask, check_mask, nst = 8, 12, 0xD6B, 0x294, 67
    st = torch.cuda.Stream()
    with ec.ECMatrixList(k, n) as L:
        V.run_geometry(device_runner(ec, L, nst, mask, check_mask, stream=st.cuda_stream), oracle,
                       k, n, mask, check_mask, nst)


def test_verify_device_at_scale(ec, oracle):
    """8+4, 2^15 stripes (16 MiB per fragment, several tiles per CU), 97 seeded
    single-bit flips in distinct stripes over basis and check bricks.  The
    fragments are oracle-encoded once; the expected flags follow from the MDS
    rules: a flip in a check brick sets that brick's bit, a flip in a basis
    brick every check brick's bit.  All 2^15 entries are compared."""
    import torch
    k, n, mask, check_mask, nst = 8, 12, 0xD6B, 0x294, 1 << 15
    basis, cb = V.bits(mask), V.bits(check_mask)
    frags = V.fragments(oracle, k, n, nst)
    dfr = {b: dev(frags[b]) for b in basis + cb}
    rng = np.random.default_rng(97)
    stripes = rng.choice(nst, size=97, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    want = np.zeros(nst, np.uint32)
    for j, t in enumerate(stripes.tolist()):
        on_check = bool(j % 2)
        b = (cb if on_check else basis)[int(rng.integers(0, len(cb if on_check else basis)))]
        off = t * V.CHUNK + int(rng.integers(0, V.CHUNK))
        dfr[b][off] ^= 1 << int(rng.integers(0, 8))
        want[t] |= (1 << b) if on_check else check_mask
    assert np.count_nonzero(want) == 97
    bad = new_bad(nst)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.verify_device(0, None, nst, mask, [dfr[b] for b in basis], check_mask,
                        [dfr[b] for b in cb], bad)
        ec.sync_device(0)
    got = read_bad(bad, nst)
    V._frag_cache.pop((k, n, nst))          # 192 MiB: not kept for the session
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:16]


def test_verify_host_entry_rejects_device_buffers(ec, oracle):
    """Device tensors given to the host entry point, all of them or mixed
    with host arrays: -EINVAL, nothing written."""
    k, n, nst = 4, 6, 4
    frags = V.fragments(oracle, k, n, nst)
    dfr = [dev(f) for f in frags]
    hbad = np.full(nst, V.SENTINEL, np.uint32)
    dbad = new_bad(nst)
    with ec.ECMatrixList(k, n) as L:
        for ins, checks, bad in (
                (dfr[:4], dfr[4:], dbad),                        # all on the device
                (dfr[:4], dfr[4:], hbad),
                ([frags[0], dfr[1], frags[2], frags[3]], frags[4:], hbad),   # mixed
                (frags[:4], [frags[4], dfr[5]], hbad),
                (frags[:4], frags[4:], dbad)):
            with pytest.raises(OSError) as e:
                L.verify(nst, 0x0F, ins, 0x30, checks, bad)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_verify" in str(e.value)
        # and host arrays mixed into a device call
        with pytest.raises(OSError) as e:
            L.verify_device(0, None, nst, 0x0F, [dfr[0], frags[1], dfr[2], dfr[3]], 0x30, dfr[4:],
                            dbad)
        assert e.value.errno == errno.EINVAL
        with pytest.raises(OSError) as e:
            L.verify_device(0, None, nst, 0x0F, dfr[:4], 0x30, dfr[4:], hbad)
        assert e.value.errno == errno.EINVAL
        ec.sync_device(0)
    assert (hbad == V.SENTINEL).all()
    assert (dbad.cpu().numpy().view(np.uint32) == V.SENTINEL).all()
