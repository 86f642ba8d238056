"""ec_method_decode_checked2_device: the read that corrects up to two chunks
on device-resident fragments (ec_decode_checked2_n, ec_kernels_impl.h).  The
geometries, sizes and corruptions of tests/test_decode_checked2.py on torch
device tensors, with expected values from the oracle and the contract (tests/
_decode_checked2_cases.py), plus what only the kernel can get wrong: many
blocks with a ragged last tile (1027 stripes), clean tiles beside corrected
ones, four different outcomes inside one tile, two pairs in one tile,
fragments and out at odd byte addresses, the largest tile (16+15: 31 inputs,
62 KiB of LDS), a caller's stream with a repair2 queued behind the read, and
2^15 stripes so that every CU holds several tiles.  out is pre-filled with
0xA5 and followed by a guard chunk, loc[] with 0xFFFFFFFF and guard words; no
fragment may change.
"""
import errno

import numpy as np
import pytest

import _decode_checked2_cases as C

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


def new_out(k, nst, offset=0):
    """nst * k chunks and a guard chunk of 0xA5, `offset` bytes into the
    allocation."""
    import torch
    t = torch.full((C.CHUNK * (k * nst + 1) + offset,), C.FILL, dtype=torch.uint8, device=DEV)
    return t[offset:]


def read_out(out, k, nst):
    got = out.cpu().numpy()
    assert (got[C.CHUNK * k * nst:] == C.FILL).all(), "guard chunk written"
    return got[:C.CHUNK * k * nst].copy()


def device_runner(ec, L, k, nst, avail_mask, stream=None, offsets=None, out_offset=0):
    """Clean fragments are uploaded once and shared by the cases; a case's
    corrupted copies are uploaded for that call."""
    import torch
    offs = offsets or {}
    kept = {}
    basis = C.bits(avail_mask)[:k]
    bmask = C.mask_of(basis)

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
        loc, out = new_loc(nst), new_out(k, nst, out_offset)
        loc2_ref, loc1_ref, out1_ref = new_loc(nst), new_loc(nst), new_out(k, nst)
        dec_ref = torch.empty(C.CHUNK * k * nst, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        L.decode_checked2_device(0, stream, nst, avail_mask, dfr, out, loc)
        L.locate2_device(0, stream, nst, avail_mask, dfr, loc2_ref)
        L.decode_checked_device(0, stream, nst, avail_mask, dfr, out1_ref, loc1_ref)
        L.decode_device(0, stream, nst, bmask, [dfr[b] for b in basis], dec_ref)
        ec.sync_device(0, stream)
        for b, a in enumerate(frags):
            assert a is None or np.array_equal(dfr[b].cpu().numpy(), a), "a fragment was written"
        return dict(loc=read_loc(loc, nst), out=read_out(out, k, nst), nbad=None, nmany=None,
                    loc2_ref=read_loc(loc2_ref, nst), loc1_ref=read_loc(loc1_ref, nst),
                    out1_ref=read_out(out1_ref, k, nst), dec_ref=dec_ref.cpu().numpy())
    return run


@pytest.mark.parametrize("nst", C.SIZES + [1027])
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_decode_checked2_device_matches_contract(ec, oracle, geom, nst):
    k, n, avail_mask = geom
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_decode_checked2_device_largest_tile(ec, oracle):
    """A 16+15 volume with every brick: 31 staged inputs, 15 syndromes, 62 KiB
    of LDS and the words; a - k >= 5, so three bricks are MANY."""
    k, n, avail_mask = C.GEOM_LARGEST
    nst = 9
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_decode_checked2_device_buffers_at_odd_addresses(ec, oracle):
    """16+6 with every fragment starting 1 byte into its allocation (LDS-DMA
    stages them in place) and out 1 byte into its own: like
    ec_method_decode_device's, out may sit at any byte address."""
    k, n, avail_mask = C.GEOMS[4]
    nst = 67
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, nst, avail_mask,
                                     offsets={b: 1 for b in range(n)}, out_offset=1),
                       oracle, k, n, avail_mask, nst)


def _seeded(rng, n, nst, count):
    """`count` distinct dirty stripes: singles and the three kinds of pair
    taking turns over all n bricks of a k = n - 4 volume.  {stripe: bricks}."""
    k = n - 4
    stripes = rng.choice(nst, size=count, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    sets = {}
    for j, t in enumerate(stripes.tolist()):
        kind = j % 4
        if kind == 0:
            S = (j % n,)
        elif kind == 1:
            S = (j % k, (j % k + 1 + (j // k) % (k - 1)) % k)    # basis + basis
        elif kind == 2:
            S = (j % k, k + j % 4)                           # basis + check
        else:
            S = (k + j % 4, k + (j + 1) % 4)                 # check + check
        assert len(set(S)) == len(S)
        sets[t] = S
    return sets


def test_decode_checked2_then_repair2_on_one_stream(ec, oracle):
    """decode_checked2_device -> repair2_device -> locate2_device queued back
    to back on a caller's stream on the read's loc[], one sync: the read
    returned the user data, the fragments are the clean ones again and the
    second locate2 gives all zero."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 67
    clean = C.fragments(oracle, k, n, nst)
    data = C.user_data(oracle, k, n, nst)
    frags = [f.copy() for f in clean]
    want = np.zeros(nst, np.uint32)
    for t, S in _seeded(np.random.default_rng(5), n, nst, 23).items():
        for i, b in enumerate(S):
            frags[b] = C.flipped(frags[b], t, (41 * t + 9 + 64 * i) % C.CHUNK, t % 8)
        want[t] = C.mask_of(S)
    dfr = [dev(f) for f in frags]
    loc, loc2, out = new_loc(nst), new_loc(nst), new_out(k, nst)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.decode_checked2_device(0, st.cuda_stream, nst, avail_mask, dfr, out, loc)
        L.repair2_device(0, st.cuda_stream, nst, avail_mask, dfr, loc)
        L.locate2_device(0, st.cuda_stream, nst, avail_mask, dfr, loc2)
        ec.sync_device(0, st.cuda_stream)
    assert np.array_equal(read_loc(loc, nst), want)
    assert np.array_equal(read_out(out, k, nst), data)
    assert not read_loc(loc2, nst).any()
    for b in range(n):
        assert np.array_equal(dfr[b].cpu().numpy(), clean[b]), "brick %d" % b


def test_decode_checked2_device_at_scale(ec, oracle):
    """8+4 with all 12 bricks, 2^15 stripes (16 MiB per fragment, several
    tiles per CU), 97 seeded dirty stripes, singles and pairs over all 12
    bricks.  The fragments are oracle-encoded once; the expectation is the MDS
    rule: damaged chunks in one or two bricks give exactly those bits and the
    user data.  All 2^15 entries of loc[] and all 128 MiB of out are compared."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 1 << 15
    frags = C.fragments(oracle, k, n, nst)
    data = C.user_data(oracle, k, n, nst)
    dfr = [dev(f) for f in frags]
    rng = np.random.default_rng(97)
    want = np.zeros(nst, np.uint32)
    for t, S in _seeded(rng, n, nst, 97).items():
        for b in S:
            off = t * C.CHUNK + int(rng.integers(0, C.CHUNK))
            dfr[b][off] ^= 1 << int(rng.integers(0, 8))
        want[t] = C.mask_of(S)
    assert np.count_nonzero(want) == 97
    loc, out = new_loc(nst), new_out(k, nst)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.decode_checked2_device(0, None, nst, avail_mask, dfr, out, loc)
        ec.sync_device(0)
    got, gout = read_loc(loc, nst), read_out(out, k, nst)
    C._frag_cache.pop((k, n, nst))          # 192 MiB: not kept for the session
    C._data_cache.pop((k, n, nst))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:16]
    bad = np.flatnonzero((gout.reshape(nst, -1) != data.reshape(nst, -1)).any(axis=1))
    assert bad.size == 0, (bad[:16], want[bad[:16]])


def test_decode_checked2_rejects_mixed_host_and_device_buffers(ec, oracle):
    """Device tensors given to the host entry point, host arrays to the device
    entry point, all of them or mixed: -EINVAL, nothing written."""
    k, n, nst, mask = 4, 8, 4, 0xFF
    frags = list(C.fragments(oracle, k, n, nst))
    dfr = [dev(f) for f in frags]
    hloc = np.full(nst, C.SENTINEL, np.uint32)
    dloc = new_loc(nst)
    hout = np.full(C.CHUNK * k * nst, C.FILL, np.uint8)
    dout = new_out(k, nst)
    with ec.ECMatrixList(k, n) as L:
        for fr, out, loc in (
                (dfr, dout, dloc),                                   # all on the device
                (dfr, hout, hloc),
                ([frags[0], dfr[1]] + frags[2:], hout, hloc),        # a basis brick
                (frags[:7] + [dfr[7]], hout, hloc),                  # a check brick
                (frags, dout, hloc),
                (frags, hout, dloc)):
            with pytest.raises(OSError) as e:
                L.decode_checked2(nst, mask, fr, out, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_decode_checked2" in str(e.value)
        for fr, out, loc in (
                ([dfr[0], frags[1]] + dfr[2:], dout, dloc),
                (dfr[:6] + [frags[6], dfr[7]], dout, dloc),
                (dfr, hout, dloc),
                (dfr, dout, hloc)):
            with pytest.raises(OSError) as e:
                L.decode_checked2_device(0, None, nst, mask, fr, out, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_decode_checked2_device" in str(e.value)
        ec.sync_device(0)
    assert (hloc == C.SENTINEL).all() and (hout == C.FILL).all()
    assert (dloc.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
    assert (dout.cpu().numpy() == C.FILL).all()
