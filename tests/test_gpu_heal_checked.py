"""ec_method_heal_checked_device: the checked and corrected heal on
device-resident fragments (ec_heal_checked_n, ec_kernels_impl.h).  The
geometries, sizes and corruptions of tests/test_heal_checked.py on torch
device tensors, with expected values from the oracle and the contract (tests/
_heal_checked_cases.py), plus what only the kernel can get wrong: many blocks
with a ragged last tile (1027 stripes), clean tiles beside corrected ones, four
different outcomes inside one tile, fragments and targets at odd byte
addresses, the most target rows and the largest tile of a 16+15 volume, a
caller's stream with a repair and a second locate queued behind the heal, and
2^15 stripes so that every CU holds several tiles.  Every out[j] is pre-filled
with 0xA5 and followed by a guard chunk, loc[] with 0xFFFFFFFF and guard
words; no fragment may change, nor the buffer of any brick outside avail_mask.
"""
import errno

import numpy as np
import pytest

import _heal_checked_cases as C

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


def new_out(nst, offset=0):
    """nst chunks and a guard chunk of 0xA5, `offset` bytes into the
    allocation."""
    import torch
    t = torch.full((C.CHUNK * (nst + 1) + offset,), C.FILL, dtype=torch.uint8, device=DEV)
    return t[offset:]


def read_out(out, nst):
    got = out.cpu().numpy()
    assert (got[C.CHUNK * nst:] == C.FILL).all(), "guard chunk written"
    return got[:C.CHUNK * nst].copy()


def device_runner(ec, L, k, n, nst, avail_mask, targets, stream=None, offset=0):
    """Clean fragments are uploaded once and shared by the cases; a case's
    corrupted copies are uploaded for that call.  Bricks outside avail_mask,
    the targets among them, get a buffer of their own in frags[]."""
    import torch
    kept = {}
    basis = C.bits(avail_mask)[:k]
    bmask, tmask = C.mask_of(basis), C.mask_of(targets)
    filler = np.full(C.CHUNK * nst, 0x3C, np.uint8)
    others = {b: dev(filler, offset) for b in range(n) if not (avail_mask >> b) & 1}

    def run(frags):
        dfr = []
        for b, a in enumerate(frags):
            if a is None:
                dfr.append(others[b])
            elif not a.flags.writeable:                      # a clean, shared fragment
                if b not in kept:
                    kept[b] = dev(a, offset)
                dfr.append(kept[b])
            else:
                dfr.append(dev(a, offset))
        loc, loc_ref = new_loc(nst), new_loc(nst)
        out = [new_out(nst, offset) for _ in targets]
        heal_ref = [torch.empty(C.CHUNK * nst, dtype=torch.uint8, device=DEV) for _ in targets]
        torch.cuda.synchronize()
        L.heal_checked_device(0, stream, nst, avail_mask, dfr, tmask, out, loc)
        L.locate_device(0, stream, nst, avail_mask, dfr, loc_ref)
        L.heal_device(0, stream, nst, bmask, [dfr[b] for b in basis], tmask, heal_ref)
        ec.sync_device(0, stream)
        for b, a in enumerate(frags):
            assert np.array_equal(dfr[b].cpu().numpy(), filler if a is None else a), \
                "the buffer of brick %d was written" % b
        return dict(loc=read_loc(loc, nst), out=[read_out(o, nst) for o in out], nbad=None,
                    nmany=None, loc_ref=read_loc(loc_ref, nst),
                    heal_ref=[h.cpu().numpy() for h in heal_ref])
    return run


@pytest.mark.parametrize("nst", C.SIZES + [1027])
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_heal_checked_device_matches_contract(ec, oracle, geom, nst):
    k, n, avail_mask, targets = geom
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets), oracle, k, n,
                       avail_mask, targets, nst)


@pytest.mark.parametrize("geom", [C.GEOM_MOST_ROWS, C.GEOM_LARGEST], ids=C.geom_id)
def test_heal_checked_device_16_plus_15(ec, oracle, geom):
    """A 16+15 volume: 18 bricks at hand and the other 13 healed (the most
    target rows a call can have at k = 16), and 29 bricks at hand (29 staged
    inputs, 13 syndromes, 58 KiB of LDS and the words) with 2 healed."""
    k, n, avail_mask, targets = geom
    nst = 9
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets), oracle, k, n,
                       avail_mask, targets, nst)


def test_heal_checked_device_buffers_at_odd_addresses(ec, oracle):
    """16+4 with every fragment starting 1 byte into its allocation (LDS-DMA
    stages them in place) and every out[j] 1 byte into its own."""
    k, n, avail_mask, targets = C.GEOMS[2]
    nst = 67
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets, offset=1), oracle, k,
                       n, avail_mask, targets, nst)


def test_heal_checked_then_repair_then_locate_on_one_stream(ec, oracle):
    """heal_checked_device -> repair_device -> locate_device queued back to
    back on a caller's stream on the heal's loc[], one sync: the targets are
    the clean fragments, the sources are clean again and the second locate is
    all zero."""
    import torch
    k, n, avail_mask, targets = C.GEOMS[0]
    nst = 67
    avail = C.bits(avail_mask)
    clean = C.fragments(oracle, k, n, nst)
    frags = [clean[b].copy() if b in avail else None for b in range(n)]
    want = np.zeros(nst, np.uint32)
    for t in range(0, nst, 3):
        b = avail[(t // 3) % len(avail)]
        frags[b] = C.flipped(frags[b], t, (41 * t + 9) % C.CHUNK, t % 8)
        want[t] = 1 << b
    dfr = [None if f is None else dev(f) for f in frags]
    loc, loc2 = new_loc(nst), new_loc(nst)
    out = [new_out(nst) for _ in targets]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.heal_checked_device(0, st.cuda_stream, nst, avail_mask, dfr, C.mask_of(targets), out,
                              loc)
        L.repair_device(0, st.cuda_stream, nst, avail_mask, dfr, loc)
        L.locate_device(0, st.cuda_stream, nst, avail_mask, dfr, loc2)
        ec.sync_device(0, st.cuda_stream)
    assert np.array_equal(read_loc(loc, nst), want)
    for o, j in zip(out, targets):
        assert np.array_equal(read_out(o, nst), clean[j]), "target %d" % j
    assert not read_loc(loc2, nst).any()
    for b in avail:
        assert np.array_equal(dfr[b].cpu().numpy(), clean[b]), "brick %d" % b


def test_heal_checked_device_at_scale(ec, oracle):
    """8+4 with bricks 4 and 7 to heal, 2^15 stripes (16 MiB per fragment,
    several tiles per CU), 97 seeded single-bit flips in distinct stripes
    spread over the 10 available bricks.  The fragments are oracle-encoded
    once; the expectation is the MDS rule: one damaged chunk in brick b gives
    1 << b and the clean target chunks.  All 2^15 entries of loc[] and all of
    both targets are compared."""
    import torch
    k, n, avail_mask, targets = C.GEOMS[0]
    nst = 1 << 15
    avail = C.bits(avail_mask)
    frags = C.fragments(oracle, k, n, nst)
    dfr = [dev(frags[b]) if b in avail else None for b in range(n)]
    rng = np.random.default_rng(97)
    stripes = rng.choice(nst, size=97, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    want = np.zeros(nst, np.uint32)
    for j, t in enumerate(stripes.tolist()):
        b = avail[j % len(avail)]
        off = t * C.CHUNK + int(rng.integers(0, C.CHUNK))
        dfr[b][off] ^= 1 << int(rng.integers(0, 8))
        want[t] = 1 << b
    assert np.count_nonzero(want) == 97
    loc = new_loc(nst)
    out = [new_out(nst) for _ in targets]
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.heal_checked_device(0, None, nst, avail_mask, dfr, C.mask_of(targets), out, loc)
        ec.sync_device(0)
    got = read_loc(loc, nst)
    gout = [read_out(o, nst) for o in out]
    C._frag_cache.pop((k, n, nst))          # 192 MiB: not kept for the session
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:16]
    for o, j in zip(gout, targets):
        bad = np.flatnonzero((o.reshape(nst, -1) != frags[j].reshape(nst, -1)).any(axis=1))
        assert bad.size == 0, (j, bad[:16], want[bad[:16]])


def test_heal_checked_rejects_mixed_host_and_device_buffers(ec, oracle):
    """Device tensors given to the host entry point, host arrays to the device
    entry point, all of them or mixed: -EINVAL, nothing written."""
    k, n, avail_mask, targets = C.GEOMS[0]
    nst, tmask = 4, C.mask_of(targets)
    avail = C.bits(avail_mask)
    clean = C.fragments(oracle, k, n, nst)
    frags = [clean[b] if b in avail else None for b in range(n)]
    dfr = [None if f is None else dev(f) for f in frags]
    hloc = np.full(nst, C.SENTINEL, np.uint32)
    dloc = new_loc(nst)
    hout = [np.full(C.CHUNK * nst, C.FILL, np.uint8) for _ in targets]
    dout = [new_out(nst) for _ in targets]

    def swap(lst, b, other):
        return lst[:b] + [other[b]] + lst[b + 1:]

    with ec.ECMatrixList(k, n) as L:
        for fr, out, loc in (
                (dfr, dout, dloc),                                   # all on the device
                (dfr, hout, hloc),
                (swap(frags, 1, dfr), hout, hloc),                   # a basis brick
                (swap(frags, 11, dfr), hout, hloc),                  # a check brick
                (frags, dout, hloc),
                (frags, [hout[0], dout[1]], hloc),
                (frags, hout, dloc)):
            with pytest.raises(OSError) as e:
                L.heal_checked(nst, avail_mask, fr, tmask, out, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_heal_checked" in str(e.value)
        for fr, out, loc in (
                (swap(dfr, 1, frags), dout, dloc),
                (swap(dfr, 10, frags), dout, dloc),
                (dfr, hout, dloc),
                (dfr, [dout[0], hout[1]], dloc),
                (dfr, dout, hloc)):
            with pytest.raises(OSError) as e:
                L.heal_checked_device(0, None, nst, avail_mask, fr, tmask, out, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_heal_checked_device" in str(e.value)
        ec.sync_device(0)
    assert (hloc == C.SENTINEL).all() and all((o == C.FILL).all() for o in hout)
    assert (dloc.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
    assert all((o.cpu().numpy() == C.FILL).all() for o in dout)
