"""ec_method_scrub_report_device: the counts and the ordered list of the dirty
stripes of a device-resident loc[] / bad[] (ec_report_count, ec_report_scan,
ec_report_scatter, ec_kernels_impl.h).  The case table of
tests/_scrub_report_cases.py on torch device tensors, against numpy, with the
report, idx[], val[] and the scratch each followed by 16 guard words in one
sentinel-filled arena; loc[] at every dword alignment; the scratch at exactly
the size ec_method_scrub_report_work names; one large case with more tiles
than the scan block has threads; the same input twice, byte for byte, and
against the host variant; locate, verify and locate2 followed by the report on
one stream with nothing between them; and the argument errors that need a
device.

Every device step of a case is queued on one torch stream, the library's calls
included, and the copy of the arena back to the host is the one wait.
"""
import errno

import numpy as np
import pytest

import _locate2_cases as C2
import _locate_cases as CL
import _scrub_report_cases as C
import _verify_cases as CV

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(device=DEV)


def dev(a, offset=0):
    """A device copy of numpy array `a`, starting `offset` bytes into its
    allocation (on the current torch stream)."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.empty(a.nbytes + offset, dtype=torch.uint8, device=DEV)
    v = t[offset:]
    v.copy_(torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)))   # (a may be read-only)
    return v


def report(ec, st, dloc, nst, cap, with_val=True, work_bytes=None):
    """One call on stream `st` into a fresh sentinel-filled arena: report, idx,
    val and the scratch, each with its guard.  Returns (Outputs, the arena on
    the device).  Nothing waits here."""
    import torch
    need = ec.scrub_report_work(nst)
    out = C.Outputs(cap, extra=need + 8 * C.GUARD)
    arena = torch.full((out.nbytes,), C.SENTINEL8, dtype=torch.uint8, device=DEV)
    base = arena.data_ptr()
    assert base % 16 == 0
    ec.scrub_report_device(0, st.cuda_stream, nst, dloc, base + out.report, cap,
                           base + out.idx if cap else None,
                           base + out.val if cap and with_val else None,
                           base + out.extra, work_bytes=need if work_bytes is None else work_bytes)
    return out, arena


def check(out, arena, loc, nst, ec, with_val=True, what=None):
    """Copy the arena back (the wait) and compare with numpy."""
    got = arena.cpu().numpy()
    out.check(got, loc, with_val=with_val, what=what)
    need = ec.scrub_report_work(nst)
    assert (got[out.extra + need:] == C.SENTINEL8).all(), (what, "written past work")
    return got


@pytest.mark.parametrize("kind", C.FILLS, ids=lambda v: v.replace(" ", "_"))
def test_device_report_matches_numpy(ec, stream, kind):
    import torch
    with torch.cuda.stream(stream):
        for nst in C.SIZES:
            loc = C.fill(nst, kind)
            dloc = dev(loc)
            caps = C.caps(loc)
            for cap in caps:
                out, arena = report(ec, stream, dloc, nst, cap)
                check(out, arena, loc, nst, ec, what=(kind, nst, cap))
            # indices only: val = NULL
            out, arena = report(ec, stream, dloc, nst, caps[-1], with_val=False)
            check(out, arena, loc, nst, ec, with_val=False, what=(kind, nst, "val = NULL"))
            assert np.array_equal(dloc.cpu().numpy().view(np.uint32), loc), "loc[] written"


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_loc_at_every_dword_alignment(ec, stream, offset):
    """loc[] starting 4, 8 and 12 bytes past a 16-byte boundary."""
    import torch
    with torch.cuda.stream(stream):
        for nst in (1, 63, 130, C.TILE - 1, C.TILE + 1, 2 * C.TILE + 3):
            for kind in ("1 in 64", "all dirty"):
                loc = C.fill(nst, kind) if nst in C.SIZES else _fresh(nst, kind)
                dloc = dev(loc, offset=offset)
                assert dloc.data_ptr() % 16 == offset
                cap = int(np.count_nonzero(loc)) + 1
                out, arena = report(ec, stream, dloc, nst, cap)
                check(out, arena, loc, nst, ec, what=(offset, nst, kind))


def _fresh(nst, kind, density=None):
    """A fill of a size outside the table (fixed seed)."""
    rng = np.random.default_rng(77 + nst)
    loc = np.zeros(nst, np.uint32)
    p = density if density is not None else {"1 in 64": 1 / 64, "all dirty": 1.0}[kind]
    dirty = np.flatnonzero(rng.random(nst) < p) if p < 1 else np.arange(nst)
    loc[dirty] = rng.choice(C.POOL, size=len(dirty))
    return loc


# The large case: 2^22 + 5 stripes are 1025 tiles of 4096 stripes, the last of
# 5: more tiles than the 256 threads of the scan block, which walks them in
# five rounds, the last of one tile.
LARGE = (1 << 22) + 5


@pytest.fixture(scope="module")
def large():
    assert -(-LARGE // C.TILE) == 1025 > C.SCAN
    return {"1 in 1000": _fresh(LARGE, None, density=1 / 1000),
            "all dirty": _fresh(LARGE, "all dirty"), "clean": np.zeros(LARGE, np.uint32)}


@pytest.mark.parametrize("kind", ["1 in 1000", "all dirty", "clean"],
                         ids=lambda v: v.replace(" ", "_"))
def test_more_tiles_than_scan_threads(ec, stream, large, kind):
    import torch
    loc = large[kind]
    nbad = int(np.count_nonzero(loc))
    cap = LARGE if kind == "all dirty" else nbad + 7
    with torch.cuda.stream(stream):
        dloc = dev(loc)
        out, arena = report(ec, stream, dloc, LARGE, cap)
        check(out, arena, loc, LARGE, ec, what=kind)


def test_same_input_twice_and_host_variant(ec, stream, large):
    """The result is a function of the input alone: two runs into fresh
    buffers and the host variant give the same bytes of report, idx and val."""
    import torch
    for loc, cap in ((large["1 in 1000"], 3000), (C.fill(65537, "1 in 2"), 40000),
                     (C.fill(4097, "tile edge"), 5)):
        nst = len(loc)
        with torch.cuda.stream(stream):
            dloc = dev(loc)
            out, a1 = report(ec, stream, dloc, nst, cap)
            _, a2 = report(ec, stream, dloc, nst, cap)
            g1, g2 = a1.cpu().numpy(), a2.cpu().numpy()
        assert np.array_equal(g1[:out.extra], g2[:out.extra])
        host = np.full(out.extra, C.SENTINEL8, np.uint8)
        assert ec.lib.ec_method_scrub_report(nst, loc.ctypes.data, host.ctypes.data + out.report,
                                             cap, host.ctypes.data + out.idx,
                                             host.ctypes.data + out.val) == 0
        assert np.array_equal(g1[:out.extra], host)
        out.check(g1, loc)


# ---- chains: the call that writes loc[] / bad[] and the report behind it on
# one stream, nothing between them; the corruptions are those of the locate,
# verify and locate2 tests, the expectation is the host call's array reduced
# by numpy

def _upload(frags, kept):
    """Clean (read-only, shared) fragments are uploaded once per runner."""
    out = []
    for b, a in enumerate(frags):
        if a is None:
            out.append(None)
        elif not a.flags.writeable:
            if b not in kept:
                kept[b] = dev(a)
            out.append(kept[b])
        else:
            out.append(dev(a))
    return out


def _words(nst):
    import torch
    return torch.full((nst + C.GUARD,), -1, dtype=torch.int32, device=DEV)


def _chain_result(ec, out, arena, dwords, nst, host_words, host_nbad, what):
    got = check(out, arena, host_words, nst, ec, what=what)
    words = dwords.cpu().numpy().view(np.uint32)
    assert (words[nst:] == 0xFFFFFFFF).all(), "guard words written"
    assert np.array_equal(words[:nst], host_words), what
    nbad = int(got[out.report:out.report + 8].view(np.uint64)[0])
    assert nbad == host_nbad, (what, nbad, host_nbad)
    return words[:nst].copy(), nbad


def locate_chain(ec, L, st, nst, avail_mask, two=False):
    import torch
    kept = {}

    def run(frags):
        with torch.cuda.stream(st):
            dfr = _upload(frags, kept)
            dloc = _words(nst)
            (L.locate2_device if two else L.locate_device)(0, st.cuda_stream, nst, avail_mask,
                                                           dfr, dloc)
            out, arena = report(ec, st, dloc, nst, nst)
            hloc = np.full(nst, 0xFFFFFFFF, np.uint32)
            hbad = (L.locate2 if two else L.locate)(nst, avail_mask, frags, hloc)
            loc, nbad = _chain_result(ec, out, arena, dloc, nst, hloc, hbad, "locate chain")
        if not two:
            return loc, nbad
        loc1 = np.full(nst, 0xFFFFFFFF, np.uint32)
        L.locate(nst, avail_mask, frags, loc1)
        return loc, nbad, loc1
    return run


def test_locate_then_report_on_one_stream(ec, oracle, stream):
    k, n, avail_mask, nst = 4, 6, 0x3F, 67
    with ec.ECMatrixList(k, n) as L:
        CL.run_geometry(locate_chain(ec, L, stream, nst, avail_mask), oracle, k, n, avail_mask, nst)


def test_locate2_then_report_on_one_stream(ec, oracle, stream):
    k, n, avail_mask, nst = 4, 8, 0xFF, 5
    with ec.ECMatrixList(k, n) as L:
        C2.run_geometry(locate_chain(ec, L, stream, nst, avail_mask, two=True), oracle, k, n,
                        avail_mask, nst)


def test_verify_then_report_on_one_stream(ec, oracle, stream):
    import torch
    k, n, mask, check_mask, nst = 4, 6, 0x0F, 0x30, 67
    kept_in, kept_ch = {}, {}
    with ec.ECMatrixList(k, n) as L:
        def run(ins, checks):
            with torch.cuda.stream(stream):
                din, dch = _upload(ins, kept_in), _upload(checks, kept_ch)
                dbad = _words(nst)
                L.verify_device(0, stream.cuda_stream, nst, mask, din, check_mask, dch, dbad)
                out, arena = report(ec, stream, dbad, nst, nst)
                hbad = np.full(nst, 0xFFFFFFFF, np.uint32)
                hn = L.verify(nst, mask, ins, check_mask, checks, hbad)
                return _chain_result(ec, out, arena, dbad, nst, hbad, hn, "verify chain")
        CV.run_geometry(run, oracle, k, n, mask, check_mask, nst)


# ---- the argument errors that need a device

def test_rejects_buffers_on_the_wrong_side(ec, stream):
    """A host loc[] at the device entry point, a device loc[] at the host entry
    point, and a scratch one byte short: -EINVAL, nothing written."""
    import torch
    nst, cap = 130, 8
    loc = C.fill(nst, "1 in 2")
    need = ec.scrub_report_work(nst)
    with torch.cuda.stream(stream):
        dloc = dev(loc)
        out = C.Outputs(cap, extra=need + 8 * C.GUARD)
        arena = torch.full((out.nbytes,), C.SENTINEL8, dtype=torch.uint8, device=DEV)
        base = arena.data_ptr()
        harena = np.full(out.nbytes, C.SENTINEL8, np.uint8)
        hbase = harena.ctypes.data

        def device_call(loc_ptr, work_bytes):
            return ec.lib.ec_method_scrub_report_device(
                0, stream.cuda_stream, nst, loc_ptr, base + out.report, cap, base + out.idx,
                base + out.val, base + out.extra, work_bytes)

        assert device_call(loc.ctypes.data, need) == -errno.EINVAL
        assert b"ec_method_scrub_report_device" in ec.lib.ec_method_last_error()
        assert device_call(dloc.data_ptr(), need - 1) == -errno.EINVAL
        # the host entry point: loc on the device, then an output on the device
        assert ec.lib.ec_method_scrub_report(nst, dloc.data_ptr(), hbase + out.report, cap,
                                             hbase + out.idx, hbase + out.val) == -errno.EINVAL
        assert b"ec_method_scrub_report:" in ec.lib.ec_method_last_error()
        assert ec.lib.ec_method_scrub_report(nst, loc.ctypes.data, hbase + out.report, cap,
                                             base + out.idx, hbase + out.val) == -errno.EINVAL
        got = arena.cpu().numpy()
    assert (got == C.SENTINEL8).all() and (harena == C.SENTINEL8).all()
