"""ec_method_readv_decode_device: the read of an unaligned byte range into a
device buffer of exactly `size` bytes, over the whole table of
tests/_readv_decode_cases.py: every K bucket of the edge kernel ec_decode_clip
(with the run-time k below the bucket), ranges inside one stripe, over two
stripes with no interior, and with interior stripes for the whole-stripe
combine, whose output then starts head bytes in front of a stripe boundary.

The expected bytes are the oracle's decode of the stripes, sliced [head : head
+ size], never the library's.  dst is carved from a tensor with 2 KiB of 0xA5
on each side, which must stay as they are, at a byte offset that rotates
through 0 .. 15 over the cases; the fragment tensors are exactly ns * 512
bytes and may not change.  One geometry per bucket runs the cases (65, 3) and
(100, 5 S + 33) at all 16 offsets and the whole table again with every
fragment 1 byte into its allocation.  The calls of one mask are queued on one
side stream with one sync.
"""
import errno

import numpy as np
import pytest

import _readv_decode_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 2048


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


def new_dst(size, offset):
    """(the whole tensor, dst): size bytes between two guards of 0xA5, dst
    `offset` bytes past a 16-byte boundary."""
    import torch
    t = torch.full((GUARD + offset + size + GUARD,), C.FILL, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t, t[GUARD + offset:GUARD + offset + size]


def check_dst(t, size, offset, want, what):
    got = t.cpu().numpy()
    lo = GUARD + offset
    assert (got[:lo] == C.FILL).all(), what + ": bytes in front of dst were written"
    assert (got[lo + size:] == C.FILL).all(), what + ": bytes behind dst were written"
    assert np.array_equal(got[lo:lo + size], want), what + ": dst differs"


def run_cases(ec, oracle, k, n, mask, cases, frag_offset=0):
    """cases: (head, size, dst offset).  All queued on one side stream, then
    one sync and the checks."""
    import torch
    held = []
    for i, (head, size, off) in enumerate(cases):
        ins, want = C.case(oracle, k, n, mask, head, size, C.window(k, head, size, i))
        assert all(f.nbytes == C.stripes(k, head, size) * C.CHUNK for f in ins)
        held.append((head, size, off, ins, want, [dev(f, frag_offset) for f in ins],
                     new_dst(size, off)))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        for head, size, off, ins, want, dins, (t, dst) in held:
            assert L.readv_decode_device(0, st.cuda_stream, head, size, mask, dins, dst) == 0
        ec.sync_device(0, st.cuda_stream)
    for head, size, off, ins, want, dins, (t, dst) in held:
        what = "%d+%d mask %#x range (%d, %d) dst + %d" % (k, n - k, mask, head, size, off)
        check_dst(t, size, off, want, what)
        for f, d in zip(ins, dins):
            assert np.array_equal(d.cpu().numpy(), f), what + ": a fragment was written"


GEOM_MASKS = [(k, n, m) for k, n in C.GEOMS for m in range(3)]


@pytest.mark.parametrize("k,n,m", GEOM_MASKS,
                         ids=["%d+%d-mask%d" % (k, n - k, m) for k, n, m in GEOM_MASKS])
def test_readv_decode_device_matches_oracle_slice(ec, oracle, k, n, m):
    ranges = C.ranges(k)
    first = len(ranges) * GEOM_MASKS.index((k, n, m))   # the offsets go on where the last left
    cases = [(head, size, (first + i) % 16) for i, (head, size) in enumerate(ranges)]
    run_cases(ec, oracle, k, n, C.masks(k, n)[m], cases)


@pytest.mark.parametrize("k,n", C.BUCKET_GEOMS, ids=lambda v: str(v))
def test_readv_decode_device_at_every_dst_offset(ec, oracle, k, n):
    cases = [(head, size, off) for head, size in C.offset_ranges(k) for off in range(16)]
    run_cases(ec, oracle, k, n, C.masks(k, n)[2], cases)


@pytest.mark.parametrize("k,n", C.BUCKET_GEOMS, ids=lambda v: str(v))
def test_readv_decode_device_fragments_off_alignment(ec, oracle, k, n):
    cases = [(head, size, (5 + i) % 16) for i, (head, size) in enumerate(C.ranges(k))]
    run_cases(ec, oracle, k, n, C.masks(k, n)[1], cases, frag_offset=1)


@pytest.mark.parametrize("k,n", C.GEOMS, ids=lambda v: str(v))
def test_aligned_ranges_equal_decode_device(ec, oracle, k, n):
    import torch
    S = C.CHUNK * k
    with ec.ECMatrixList(k, n) as L:
        for mask in C.masks(k, n):
            for nst in (1, 3):
                ins, want = C.case(oracle, k, n, mask, 0, nst * S)
                dins = [dev(f) for f in ins]
                t, dst = new_dst(nst * S, 0)
                ref = torch.full((nst * S,), C.FILL, dtype=torch.uint8, device=DEV)
                torch.cuda.synchronize()
                assert L.readv_decode_device(0, None, 0, nst * S, mask, dins, dst) == 0
                L.decode_device(0, None, nst, mask, dins, ref)
                ec.sync_device(0)
                check_dst(t, nst * S, 0, want, "aligned")
                assert torch.equal(dst, ref)


def test_readv_decode_device_follows_encode_on_the_stream(ec, oracle):
    """encode_device, then readv_decode_device of the fragments it writes, on
    one stream with no synchronisation between them."""
    import torch
    k, n, nst, mask = 4, 6, 9, 0x3C
    S = C.CHUNK * k
    head, size = 100, 5 * S + 33
    win = 2
    data = oracle.fill_xorshift(S * nst, seed=oracle.SEED + 99)
    din = dev(data)
    frags = [torch.zeros(C.CHUNK * nst, dtype=torch.uint8, device=DEV) for _ in range(n)]
    t, dst = new_dst(size, 3)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.encode_device(0, st.cuda_stream, nst, din, frags)
        ins = [frags[b][win * C.CHUNK:] for b in range(n) if (mask >> b) & 1]
        L.readv_decode_device(0, st.cuda_stream, head, size, mask, ins, dst)
        ec.sync_device(0, st.cuda_stream)
    check_dst(t, size, 3, data[win * S + head:win * S + head + size], "after encode")


def test_empty_range_on_device(ec, oracle):
    k, n, mask = 4, 6, 0x3C
    ins, _ = C.case(oracle, k, n, mask, 0, 1)
    dins = [dev(f) for f in ins]
    t, dst = new_dst(16, 0)
    with ec.ECMatrixList(k, n) as L:
        assert L.readv_decode_device(0, None, 5, 0, mask, dins, dst) == 0
        ec.sync_device(0)
    assert (t.cpu().numpy() == C.FILL).all()


def test_readv_decode_device_argument_errors(ec, oracle):
    k, n, mask, head, size = 4, 6, 0x3C, 100, 3000
    ins, want = C.case(oracle, k, n, mask, head, size)
    dins = [dev(f) for f in ins]
    t, dst = new_dst(size, 1)
    hdst = np.full(size, C.FILL, np.uint8)

    def rejected(L, call, *args):
        with pytest.raises(OSError) as e:
            call(*args)
        assert e.value.errno == errno.EINVAL, e.value

    with ec.ECMatrixList(k, n) as L:
        d = L.readv_decode_device
        # host pointers given to the device entry point, all or some
        rejected(L, d, 0, None, head, size, mask, ins, hdst)
        rejected(L, d, 0, None, head, size, mask, dins, hdst)
        rejected(L, d, 0, None, head, size, mask, ins, dst)
        rejected(L, d, 0, None, head, size, mask, dins[:3] + ins[3:], dst)
        # device pointers given to the host entry point, all or some
        rejected(L, L.readv_decode, head, mask, dins, dst)
        rejected(L, L.readv_decode, head, mask, ins, dst)
        rejected(L, L.readv_decode, head, mask, dins, hdst)
        # head outside the first stripe
        rejected(L, d, 0, None, C.CHUNK * k, size, mask, dins, dst)
        # masks of k - 1 and k + 1 bricks, with a brick at n, and none
        for bad in (0x1C, 0x3E, 0x4E, 0):
            rejected(L, d, 0, None, head, size, bad, dins, dst)
        rejected(L, d, 0, None, head, size, mask, dins[:3] + [None], dst)
        rejected(L, d, 0, None, head, size, mask, dins, None)
        ec.sync_device(0)
        assert (t.cpu().numpy() == C.FILL).all() and (hdst == C.FILL).all()
        # and the call they all fall short of
        assert d(0, None, head, size, mask, dins, dst) == 0
        ec.sync_device(0)
    check_dst(t, size, 1, want, "valid")
