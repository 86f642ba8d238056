"""ec_method_repair2_device: rewrite the one or two chunks loc[] names on
device-resident fragments (ec_repair2_n, ec_kernels_impl.h).  The geometries,
sizes and cases of tests/test_repair2.py on torch device tensors, with
expected bytes from the oracle (tests/_repair2_cases.py), plus what only the
kernel can get wrong: 1027 stripes (several blocks, a ragged last wave) with
every stripe dirty and the pairs taking turns inside one wave's 64 words,
every stripe naming one pair (groups of four), singles, pairs and ignored
values mixed in one wave, a dirty stripe in lane 63 beside one in lane 0 of
the next wave, 16+15, fragments at odd byte addresses including the ones
written, a caller's stream with locate2 -> repair2 -> locate2 queued back to
back, and 2^15 stripes.  Every fragment is followed by a guard chunk that must
not change.
"""
import errno

import numpy as np
import pytest

import _repair2_cases as R2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = R2.CHUNK


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


class DeviceOps:
    """Every call uploads its fragments, guard chunk included, and reads all
    of them back after one synchronisation."""

    def __init__(self, ec, L, nst, avail_mask, stream=None, offsets=None):
        self.ec, self.L, self.nst, self.mask = ec, L, nst, avail_mask
        self.stream, self.offs = stream, offsets or {}

    def _upload(self, frags):
        full = [None if f is None else dev(R2.with_guard(f), self.offs.get(b, 0))
                for b, f in enumerate(frags)]
        return full, [None if f is None else f[:self.nst * CHUNK] for f in full]

    def _loc(self, fill=None):
        import torch
        if fill is None:
            return torch.full((self.nst,), -1, dtype=torch.int32, device=DEV)
        return torch.from_numpy(fill.view(np.int32).copy()).to(DEV)

    @staticmethod
    def _host(full):
        return [None if f is None else f.cpu().numpy() for f in full]

    def _repair(self, call, frags, loc):
        import torch
        full, view = self._upload(frags)
        dloc = self._loc(loc)
        torch.cuda.synchronize()
        call(0, self.stream, self.nst, self.mask, view, dloc)
        self.ec.sync_device(0, self.stream)
        return self._host(full), dloc.cpu().numpy().view(np.uint32), None

    def repair2(self, frags, loc):
        return self._repair(self.L.repair2_device, frags, loc)

    def repair(self, frags, loc):
        return self._repair(self.L.repair_device, frags, loc)

    def scrub2(self, frags):
        import torch
        full, view = self._upload(frags)
        loc, loc2 = self._loc(), self._loc()
        torch.cuda.synchronize()
        # queued back to back: no host synchronisation between the three
        self.L.locate2_device(0, self.stream, self.nst, self.mask, view, loc)
        self.L.repair2_device(0, self.stream, self.nst, self.mask, view, loc)
        self.L.locate2_device(0, self.stream, self.nst, self.mask, view, loc2)
        self.ec.sync_device(0, self.stream)
        return (loc.cpu().numpy().view(np.uint32), self._host(full),
                loc2.cpu().numpy().view(np.uint32), None)


@pytest.mark.parametrize("nst", R2.SIZES + [1027])
@pytest.mark.parametrize("geom", R2.GEOMS, ids=R2.geom_id)
def test_repair2_device_matches_oracle(ec, oracle, geom, nst):
    k, n, avail_mask = geom
    with ec.ECMatrixList(k, n) as L:
        R2.run_geometry(DeviceOps(ec, L, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_repair2_device_largest_geometry(ec, oracle):
    """16+15 with every brick: 15 check rows, 120 basis pairs."""
    k, n, avail_mask = R2.GEOM_LARGEST
    nst = R2.SIZE_LARGEST
    with ec.ECMatrixList(k, n) as L:
        R2.run_geometry(DeviceOps(ec, L, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_repair2_device_fragments_at_odd_addresses(ec, oracle):
    """Every fragment 1 byte into its allocation (4+4), and a mix of byte
    offsets 1, 0, 3, 2 over the bricks (8+4 with a = k + 2): inputs and the
    written fragments at byte addresses."""
    k, n, avail_mask, nst = 4, 8, 0xFF, 67
    with ec.ECMatrixList(k, n) as L:
        R2.run_geometry(DeviceOps(ec, L, nst, avail_mask, offsets={b: 1 for b in range(n)}),
                        oracle, k, n, avail_mask, nst)
    k, n, avail_mask, nst = 8, 12, 0xF6F, 5
    with ec.ECMatrixList(k, n) as L:
        offs = {b: (1, 0, 3, 2)[j % 4] for j, b in enumerate(R2.bits(avail_mask))}
        R2.run_geometry(DeviceOps(ec, L, nst, avail_mask, offsets=offs), oracle, k, n,
                        avail_mask, nst)


def test_repair2_device_on_a_callers_stream(ec, oracle):
    """locate2 -> repair2 -> locate2 on a caller's stream, one sync at the end."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 67
    st = torch.cuda.Stream()
    with ec.ECMatrixList(k, n) as L:
        R2.run_geometry(DeviceOps(ec, L, nst, avail_mask, stream=st.cuda_stream), oracle, k, n,
                        avail_mask, nst)


def test_repair2_device_at_scale(ec, oracle):
    """8+4 with all 12 bricks, 2^15 stripes, 97 seeded dirty stripes, singles
    and pairs spread over all 12 bricks: locate2, repair2, and every fragment
    equals the oracle's clean one over all bytes."""
    import torch
    k, n, avail_mask, nst = 8, 12, 0xFFF, 1 << 15
    frags = R2.fragments(oracle, k, n, nst)
    full = [dev(R2.with_guard(f)) for f in frags]
    dfr = [f[:nst * CHUNK] for f in full]
    rng = np.random.default_rng(97)
    stripes = rng.choice(nst, size=97, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    want = np.zeros(nst, np.uint32)
    for j, t in enumerate(stripes.tolist()):
        named = (j % n,) if j % 3 == 0 else (j % n, (j % n + 1 + j // n) % n)
        for b in named:
            off = t * CHUNK + int(rng.integers(0, CHUNK))
            dfr[b][off] ^= 1 << int(rng.integers(0, 8))
            want[t] |= 1 << b
    loc = torch.full((nst,), -1, dtype=torch.int32, device=DEV)
    loc2 = torch.full((nst,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.locate2_device(0, None, nst, avail_mask, dfr, loc)
        L.repair2_device(0, None, nst, avail_mask, dfr, loc)
        L.locate2_device(0, None, nst, avail_mask, dfr, loc2)
        ec.sync_device(0)
    assert np.array_equal(loc.cpu().numpy().view(np.uint32), want)
    assert not loc2.cpu().numpy().any()
    try:
        R2.check_frags("at scale", list(range(n)), nst, [f.cpu().numpy() for f in full], frags)
    finally:
        from _locate_cases import _frag_cache
        _frag_cache.pop((k, n, nst), None)      # 192 MiB: not kept for the session


def test_repair2_rejects_mixed_host_and_device_buffers(ec, oracle):
    """Device tensors given to the host entry point, host arrays to the device
    entry point, all of them or mixed: -EINVAL, nothing written."""
    import torch
    k, n, nst = 4, 6, 4
    clean = R2.fragments(oracle, k, n, nst)
    frags = [R2.flipped(f, 1, 9, 1) for f in clean]
    keep = [f.copy() for f in frags]
    dfr = [dev(f) for f in frags]
    hloc = np.full(nst, 1 << 1 | 1 << 4, np.uint32)
    dloc = torch.from_numpy(hloc.view(np.int32).copy()).to(DEV)
    with ec.ECMatrixList(k, n) as L:
        for fr, loc in (
                (dfr, dloc),                                   # all on the device
                (dfr, hloc),
                ([frags[0], dfr[1]] + frags[2:], hloc),        # a named brick
                (frags[:5] + [dfr[5]], hloc),                  # a brick of B_ij
                (frags, dloc)):
            with pytest.raises(OSError) as e:
                L.repair2(nst, 0x3F, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_repair2" in str(e.value)
        for fr, loc in (
                ([dfr[0], frags[1]] + dfr[2:], dloc),
                (dfr[:5] + [frags[5]], dloc),
                (dfr, hloc)):
            with pytest.raises(OSError) as e:
                L.repair2_device(0, None, nst, 0x3F, fr, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_repair2_device" in str(e.value)
        # a = k + 1 is too few on the device as well
        with pytest.raises(OSError) as e:
            L.repair2_device(0, None, nst, 0x1F, dfr, dloc)
        assert e.value.errno == errno.EINVAL
        ec.sync_device(0)
    for b in range(n):
        assert np.array_equal(frags[b], keep[b])
        assert np.array_equal(dfr[b].cpu().numpy(), keep[b])
    assert (hloc == (1 << 1 | 1 << 4)).all()
    assert (dloc.cpu().numpy().view(np.uint32) == (1 << 1 | 1 << 4)).all()
