"""ec_method_heal_checked2_device: the heal that corrects up to two chunks on
device-resident fragments (ec_heal_checked2_n, ec_kernels_impl.h).  The
geometries, sizes and corruptions of tests/test_heal_checked2.py on torch
device tensors, with expected values from the oracle and the contract (tests/
_heal_checked2_cases.py), plus what only the kernel can get wrong: many blocks
with a ragged last tile (1027 stripes), clean tiles beside corrected ones, four
different outcomes inside one tile, two pairs in one tile, fragments and
targets at odd byte addresses, the most target rows and the largest tile of a
16+15 volume (the target pointers travel behind the inputs in one list of 31),
a caller's stream with a repair2 and a second locate2 queued behind the heal,
the non-temporal staging instantiations, and the 4-wave kernel above 2^17
stripes.  Every out[j] is pre-filled with 0xA5 and followed by a guard chunk,
loc[] with 0xFFFFFFFF and guard words; no fragment may change, nor the buffer
of any brick outside avail_mask.
"""
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import _heal_checked2_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
        loc, loc2_ref, loc1_ref = new_loc(nst), new_loc(nst), new_loc(nst)
        out = [new_out(nst, offset) for _ in targets]
        out1_ref = [new_out(nst) for _ in targets]
        heal_ref = [torch.empty(C.CHUNK * nst, dtype=torch.uint8, device=DEV) for _ in targets]
        torch.cuda.synchronize()
        L.heal_checked2_device(0, stream, nst, avail_mask, dfr, tmask, out, loc)
        L.locate2_device(0, stream, nst, avail_mask, dfr, loc2_ref)
        L.heal_checked_device(0, stream, nst, avail_mask, dfr, tmask, out1_ref, loc1_ref)
        L.heal_device(0, stream, nst, bmask, [dfr[b] for b in basis], tmask, heal_ref)
        ec.sync_device(0, stream)
        for b, a in enumerate(frags):
            assert np.array_equal(dfr[b].cpu().numpy(), filler if a is None else a), \
                "the buffer of brick %d was written" % b
        return dict(loc=read_loc(loc, nst), out=[read_out(o, nst) for o in out], nbad=None,
                    nmany=None, loc2_ref=read_loc(loc2_ref, nst),
                    loc1_ref=read_loc(loc1_ref, nst),
                    out1_ref=[read_out(o, nst) for o in out1_ref],
                    heal_ref=[h.cpu().numpy() for h in heal_ref])
    return run


@pytest.mark.parametrize("nst", C.SIZES + [1027])
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_heal_checked2_device_matches_contract(ec, oracle, geom, nst):
    k, n, avail_mask, targets = geom
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets), oracle, k, n,
                       avail_mask, targets, nst)


@pytest.mark.parametrize("geom", [C.GEOM_MOST_ROWS, C.GEOM_LARGEST], ids=C.geom_id)
def test_heal_checked2_device_16_plus_15(ec, oracle, geom):
    """A 16+15 volume: 20 bricks at hand and the other 11 healed (the most
    target rows a call can have at k = 16: 44 words of T, and all 31 slots of
    the pointer list in use), and 29 bricks at hand (29 staged inputs, 13
    syndromes, 58 KiB of LDS and the words) with 2 healed."""
    k, n, avail_mask, targets = geom
    nst = 9
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets), oracle, k, n,
                       avail_mask, targets, nst)


def test_heal_checked2_device_buffers_at_odd_addresses(ec, oracle):
    """16+6 with every fragment starting 1 byte into its allocation (LDS-DMA
    stages them in place) and every out[j] 1 byte into its own."""
    k, n, avail_mask, targets = C.GEOMS[2]
    nst = 67
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets, offset=1), oracle, k,
                       n, avail_mask, targets, nst)


def _seeded(rng, avail, k, nst, count):
    """`count` distinct dirty stripes: singles and the three kinds of pair
    taking turns over the bricks of avail.  {stripe: bricks}."""
    basis, checks = avail[:k], avail[k:]
    r = len(checks)
    stripes = rng.choice(nst, size=count, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    sets = {}
    for j, t in enumerate(stripes.tolist()):
        kind = j % 4
        if kind == 0:
            S = (avail[j % len(avail)],)
        elif kind == 1:
            S = (basis[j % k], basis[(j % k + 1 + (j // k) % (k - 1)) % k])   # basis + basis
        elif kind == 2:
            S = (basis[j % k], checks[j % r])                                # basis + check
        else:
            S = (checks[j % r], checks[(j + 1) % r])                         # check + check
        assert len(set(S)) == len(S)
        sets[t] = S
    return sets


def test_heal_checked2_then_repair2_then_locate2_on_one_stream(ec, oracle):
    """heal_checked2_device -> repair2_device -> locate2_device queued back to
    back on a caller's stream on the heal's loc[], one sync: the targets are
    the clean fragments, the sources are clean again and the second locate2 is
    all zero."""
    import torch
    k, n, avail_mask, targets = C.GEOMS[0]
    nst = 67
    avail = C.bits(avail_mask)
    clean = C.fragments(oracle, k, n, nst)
    frags = [clean[b].copy() if b in avail else None for b in range(n)]
    want = np.zeros(nst, np.uint32)
    for t, S in _seeded(np.random.default_rng(5), avail, k, nst, 23).items():
        for i, b in enumerate(S):
            frags[b] = C.flipped(frags[b], t, (41 * t + 9 + 64 * i) % C.CHUNK, t % 8)
        want[t] = C.mask_of(S)
    dfr = [None if f is None else dev(f) for f in frags]
    loc, loc2 = new_loc(nst), new_loc(nst)
    out = [new_out(nst) for _ in targets]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.heal_checked2_device(0, st.cuda_stream, nst, avail_mask, dfr, C.mask_of(targets), out,
                               loc)
        L.repair2_device(0, st.cuda_stream, nst, avail_mask, dfr, loc)
        L.locate2_device(0, st.cuda_stream, nst, avail_mask, dfr, loc2)
        ec.sync_device(0, st.cuda_stream)
    assert np.array_equal(read_loc(loc, nst), want)
    for o, j in zip(out, targets):
        assert np.array_equal(read_out(o, nst), clean[j]), "target %d" % j
    assert not read_loc(loc2, nst).any()
    for b in avail:
        assert np.array_equal(dfr[b].cpu().numpy(), clean[b]), "brick %d" % b


def test_heal_checked2_device_four_wave_kernel_above_2_17(ec, oracle):
    """6+6 with 0xFDF and brick 5 healed at 2^17 + 5 stripes: k <= 8 runs the
    4-wave <8, 4> instantiation above 2^17 stripes (64 MiB per fragment, about
    0.8 GiB moved once).  101 seeded dirty stripes, singles and the three kinds
    of pair over the 11 available bricks.  The fragments are oracle-encoded
    once; the expectation is the MDS rule: damaged chunks in one or two bricks
    give exactly those bits and the clean target chunks.  All entries of loc[]
    and all of the target are compared."""
    import torch
    k, n, avail_mask, targets = C.GEOMS[6]
    nst = (1 << 17) + 5
    avail = C.bits(avail_mask)
    frags = C.fragments(oracle, k, n, nst)
    dfr = [dev(frags[b]) if b in avail else None for b in range(n)]
    rng = np.random.default_rng(101)
    want = np.zeros(nst, np.uint32)
    for t, S in _seeded(rng, avail, k, nst, 101).items():
        for b in S:
            off = t * C.CHUNK + int(rng.integers(0, C.CHUNK))
            dfr[b][off] ^= 1 << int(rng.integers(0, 8))
        want[t] = C.mask_of(S)
    assert np.count_nonzero(want) == 101
    loc = new_loc(nst)
    out = [new_out(nst) for _ in targets]
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.heal_checked2_device(0, None, nst, avail_mask, dfr, C.mask_of(targets), out, loc)
        ec.sync_device(0)
    got = read_loc(loc, nst)
    gout = [read_out(o, nst) for o in out]
    C._frag_cache.pop((k, n, nst))          # 768 MiB: not kept for the session
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:16]
    for o, j in zip(gout, targets):
        bad = np.flatnonzero((o.reshape(nst, -1) != frags[j].reshape(nst, -1)).any(axis=1))
        assert bad.size == 0, (j, bad[:16], want[bad[:16]])


NT_SCRIPT = r"""
import sys
sys.path.insert(0, "oracle")
import numpy as np, torch
import glusterfs_amd as g
import oracle as O           # the checker

rng = np.random.default_rng(12)
def dev(a):
    return torch.from_numpy(a).cuda()
def u32(t):
    return t.cpu().numpy().view(np.uint32)
def bits(m):
    return [i for i in range(32) if (m >> i) & 1]

# 13 stripes (three full tiles and a ragged one) of the three K buckets: a
# damaged basis chunk, a pair of basis chunks, a basis chunk and the chunk of
# check row 0, and two check chunks in the ragged tile.  Expected values are
# the MDS rule on oracle-encoded fragments: the bits of the damaged bricks and
# the clean target.
for k, n, avail, target in ((4, 9, 0x1F7, 3), (8, 14, 0x3F6F, 7), (16, 22, 0x3BFFFD, 18)):
    sn = 13
    data = rng.integers(0, 256, 512 * k * sn, dtype=np.uint8)
    clean = O.encode(k, n, data)
    av = bits(avail)
    basis, checks = av[:k], av[k:]
    fr = [clean[b].copy() if b in av else None for b in range(n)]
    want = np.zeros(sn, np.uint32)
    for t, S in ((2, (basis[1],)), (5, (basis[0], basis[k - 1])), (6, (basis[2], checks[0])),
                 (12, (checks[1], checks[3]))):
        for i, b in enumerate(S):
            fr[b][t * 512 + 37 + 64 * i] ^= 0x10 << i
            want[t] |= 1 << b
    sd = [None if f is None else dev(f) for f in fr]
    loc = torch.full((sn,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((512 * sn,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with g.ECMatrixList(k, n) as L:
        L.heal_checked2_device(0, None, sn, avail, sd, 1 << target, [out], loc)
        g.sync_device(0)
    assert np.array_equal(u32(loc), want), ("heal_checked2 loc", k, u32(loc))
    assert np.array_equal(out.cpu().numpy(), clean[target]), ("heal_checked2 out", k)
    for b in av:
        assert np.array_equal(sd[b].cpu().numpy(), fr[b]), ("a fragment was written", k, b)
print("ok")
"""


def test_heal_checked2_device_non_temporal_instantiations():
    """EC_MI355X_LDSNT=1 (read when the library loads) stages these small
    calls with non-temporal loads: the kernel at K = 4, 8 and 16 (4+5, 8+6,
    16+6), in a process of their own."""
    env = dict(os.environ, EC_MI355X_QUIET="1", EC_MI355X_LDSNT="1")
    r = subprocess.run([sys.executable, "-c", NT_SCRIPT], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


def test_heal_checked2_rejects_mixed_host_and_device_buffers(ec, oracle):
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
                (swap(frags, 13, dfr), hout, hloc),                  # a check brick
                (frags, dout, hloc),
                (frags, [hout[0], dout[1]], hloc),
                (frags, hout, dloc)):
            with pytest.raises(OSError) as e:
                L.heal_checked2(nst, avail_mask, fr, tmask, out, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_heal_checked2" in str(e.value)
        for fr, out, loc in (
                (swap(dfr, 1, frags), dout, dloc),
                (swap(dfr, 12, frags), dout, dloc),
                (dfr, hout, dloc),
                (dfr, [dout[0], hout[1]], dloc),
                (dfr, dout, hloc)):
            with pytest.raises(OSError) as e:
                L.heal_checked2_device(0, None, nst, avail_mask, fr, tmask, out, loc)
            assert e.value.errno == errno.EINVAL
            assert "ec_method_heal_checked2_device" in str(e.value)
        ec.sync_device(0)
    assert (hloc == C.SENTINEL).all() and all((o == C.FILL).all() for o in hout)
    assert (dloc.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
    assert all((o.cpu().numpy() == C.FILL).all() for o in dout)
