"""ec_method_locate2_device: the one or two damaged bricks per stripe on
device-resident fragments (ec_locate2_n, ec_kernels_impl.h).  The geometries,
sizes and corruptions of tests/test_locate2.py on torch device tensors, with
expected values from the oracle and the definition (tests/_locate2_cases.py),
plus what only the kernel can get wrong: many blocks with a ragged last tile
(1027 stripes), tiles that leave after phase 1 or phase 2 beside tiles that
run phase 3, four different outcomes inside one tile, fragments at an odd byte
address, the largest tile and pair table (16+15: 31 inputs, 15 syndromes, 152
candidates), a caller's stream, the heal round trip queued behind locate2 on
one stream, and 2^15 stripes so that every CU holds several tiles.  loc[] is
pre-filled with 0xFFFFFFFF and followed by guard words that must not change.
"""
import errno

import numpy as np
import pytest

import _locate2_cases as C

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
        loc, loc1 = new_loc(nst), new_loc(nst)
        torch.cuda.synchronize()
        L.locate2_device(0, stream, nst, avail_mask, dfr, loc)
        L.locate_device(0, stream, nst, avail_mask, dfr, loc1)
        ec.sync_device(0, stream)
        return read_loc(loc, nst), None, read_loc(loc1, nst)
    return run


@pytest.mark.parametrize("nst", C.SIZES + [1027])
@pytest.mark.parametrize("geom", C.GEOMS + [C.GEOM_LARGEST], ids=C.geom_id)
def test_locate2_device_matches_definition(ec, oracle, geom, nst):
    k, n, avail_mask = geom
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_locate2_device_fragments_at_odd_addresses(ec, oracle):
    """16+6 with a basis fragment and a check fragment starting 1 byte into
    their allocations: LDS-DMA stages them in place."""
    k, n, avail_mask, nst = 16, 22, 0x3BFFFD, 67
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask, offsets={5: 1, 19: 1}), oracle, k, n,
                       avail_mask, nst)


def test_locate2_device_largest_tile(ec, oracle):
    """A 16+15 volume with every brick: 31 staged inputs, 15 syndromes, 32
    single-position and 120 pair candidates."""
    k, n, avail_mask = C.GEOM_LARGEST
    nst = 9
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_locate2_device_on_a_callers_stream(ec, oracle):
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 67
    st = torch.cuda.Stream()
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, nst, avail_mask, stream=st.cuda_stream), oracle, k, n,
                       avail_mask, nst)


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_locate2_device_then_heal_round_trip(ec, oracle, geom):
    """Damage two chunks, locate2, heal the named stripe with
    ec_method_heal_device as include/ec_method.h documents, all on one
    caller's stream; the fragments equal the clean ones again and a second
    locate2 gives 0."""
    import torch
    k, n, avail_mask = geom
    nst = 5
    clean = C.fragments(oracle, k, n, nst)
    avail = C.bits(avail_mask)
    rng = np.random.default_rng(5 * k + n)
    host = {b: clean[b].copy() for b in avail}
    t, b1, b2 = 3, avail[1], avail[k + 1]            # a basis and a check brick
    for b in (b1, b2):
        host[b][t * C.CHUNK:(t + 1) * C.CHUNK] = rng.integers(0, 256, C.CHUNK, dtype=np.uint8)
    dfr = [dev(host[b]) if b in avail else None for b in range(n)]
    loc = new_loc(nst)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.locate2_device(0, st.cuda_stream, nst, avail_mask, dfr, loc)
        ec.sync_device(0, st.cuda_stream)
        got = read_loc(loc, nst)
        want = np.zeros(nst, np.uint32)
        want[t] = 1 << b1 | 1 << b2
        assert np.array_equal(got, want)
        named = C.bits(int(got[t]))
        src = [b for b in avail if b not in named][:k]
        off = t * C.CHUNK
        L.heal_device(0, st.cuda_stream, 1, sum(1 << b for b in src),
                      [dfr[b].data_ptr() + off for b in src], int(got[t]),
                      [dfr[b].data_ptr() + off for b in named])
        L.locate2_device(0, st.cuda_stream, nst, avail_mask, dfr, loc)
        ec.sync_device(0, st.cuda_stream)
    for b in avail:
        assert np.array_equal(dfr[b].cpu().numpy(), clean[b]), b
    assert not read_loc(loc, nst).any()


def test_locate2_device_at_scale(ec, oracle):
    """8+4 with all 12 bricks, 2^15 stripes (16 MiB per fragment, several
    tiles per CU), 97 seeded dirty stripes, roughly half with one damaged
    chunk and half with two, spread over all 12 bricks.  The fragments are
    oracle-encoded once; the expectation is the MDS rule (damaged chunks in
    one or two bricks give exactly those bits), and the oracle's definition is
    evaluated on 8 of the dirty stripes.  All 2^15 entries are compared."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 1 << 15
    frags = C.fragments(oracle, k, n, nst)
    dfr = [dev(f) for f in frags]
    rng = np.random.default_rng(97)
    stripes = rng.choice(nst, size=97, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    want = np.zeros(nst, np.uint32)
    changed = {}
    for j, t in enumerate(stripes.tolist()):
        bricks = [j % n] if j % 2 == 0 else [j % n, (j % n + 1 + j // n) % n]
        assert len(set(bricks)) == len(bricks)
        for b in bricks:
            off = t * C.CHUNK + int(rng.integers(0, C.CHUNK))
            bit = 1 << int(rng.integers(0, 8))
            dfr[b][off] ^= bit
            changed.setdefault(t, []).append((b, off, bit))
            want[t] |= 1 << b
    assert np.count_nonzero(want) == 97
    assert sum(bin(v).count("1") == 2 for v in want.tolist()) == 48
    loc = new_loc(nst)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.locate2_device(0, None, nst, avail_mask, dfr, loc)
        ec.sync_device(0)
    got = read_loc(loc, nst)
    # the definition on 8 of them, on host copies of those stripes' chunks
    for t in stripes[:8].tolist():
        one = [f[t * C.CHUNK:(t + 1) * C.CHUNK].copy() for f in frags]
        for b, off, bit in changed[t]:
            one[b][off - t * C.CHUNK] ^= bit
        assert C.expected_loc2(oracle, k, n, C.bits(avail_mask), one, 0) == want[t], t
    C.drop_fragments((k, n, nst))           # 192 MiB: not kept for the session
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:16]


def test_locate2_rejects_mixed_host_and_device_buffers(ec, oracle):
    """Device tensors given to the host entry point, host arrays to the device
    entry point, all of them or mixed: -EINVAL, nothing written."""
    k, n, nst, mask = 5, 9, 4, 0x1FF
    frags = list(C.fragments(oracle, k, n, nst))
    dfr = [dev(f) for f in frags]
    hloc = np.full(nst, C.SENTINEL, np.uint32)
    dloc = new_loc(nst)
    with ec.ECMatrixList(k, n) as L:
        for fr, loc in (
                (dfr, dloc),                                   # all on the device
                (dfr, hloc),
                ([frags[0], dfr[1]] + frags[2:], hloc),        # a basis brick
                (frags[:8] + [dfr[8]], hloc),                  # a check brick
                (frags, dloc)):
            with pytest.raises(OSError) as e:
                L.locate2(nst, mask, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_locate2" in str(e.value)
        for fr, loc in (
                ([dfr[0], frags[1]] + dfr[2:], dloc),
                (dfr[:7] + [frags[7], dfr[8]], dloc),
                (dfr, hloc)):
            with pytest.raises(OSError) as e:
                L.locate2_device(0, None, nst, mask, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_locate2_device" in str(e.value)
        # a - k = 3 is refused on the device entry point too
        with pytest.raises(OSError) as e:
            L.locate2_device(0, None, nst, 0xFF, dfr, dloc)
        assert e.value.errno == errno.EINVAL
        ec.sync_device(0)
    assert (hloc == C.SENTINEL).all()
    assert (dloc.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
