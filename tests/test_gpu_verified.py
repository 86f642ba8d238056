"""ec_method_decode_verified_device and ec_method_heal_verified_device: the
read and the heal that only detect, on device-resident fragments
(ec_decode_verified_n and ec_heal_verified_n, ec_kernels_impl.h).  The
geometries, sizes and corruptions of tests/test_verified.py on torch device
tensors, with expected values from the oracle and the rule (tests/
_verified_cases.py), plus what only the kernels can get wrong: many blocks
with a ragged last tile (1027 stripes), four different outcomes inside one
tile, fragments and outputs at odd byte addresses, the 62 KiB tile and the
most output rows of a 16+15 volume, a caller's stream, 2^17 + 5 stripes (the
4-wave bucket of 5 <= k <= 8) and the non-temporal instantiations.  Every
output is pre-filled with 0xA5 and followed by a guard chunk, bad[] with
0xFFFFFFFF and guard words; no fragment may change, nor the buffer of any
brick outside avail_mask.
"""
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import _verified_cases as C

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


def new_bad(nst):
    import torch
    return torch.full((nst + C.GUARD,), -1, dtype=torch.int32, device=DEV)


def read_bad(bad, nst):
    got = bad.cpu().numpy().view(np.uint32)
    assert (got[nst:] == C.SENTINEL).all(), "guard words written"
    return got[:nst].copy()


def new_out(chunks, offset=0):
    """`chunks` chunks and a guard chunk of 0xA5, `offset` bytes into the
    allocation."""
    import torch
    t = torch.full((C.CHUNK * (chunks + 1) + offset,), C.FILL, dtype=torch.uint8, device=DEV)
    return t[offset:]


def read_out(out, chunks):
    got = out.cpu().numpy()
    assert (got[C.CHUNK * chunks:] == C.FILL).all(), "guard chunk written"
    return got[:C.CHUNK * chunks].copy()


def device_runner(ec, L, k, n, nst, avail_mask, targets, stream=None, offset=0):
    """Clean fragments are uploaded once and shared by the cases; a case's
    corrupted copies are uploaded for that call.  Bricks outside avail_mask,
    the targets among them, get a buffer of their own in frags[]."""
    import torch
    kept = {}
    basis, checks, bmask, cmask = C.split(k, avail_mask)
    per = k if targets is None else 1
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
        bad, bad_ref = new_bad(nst), new_bad(nst)
        out = [new_out(per * nst, offset) for _ in (targets or (0,))]
        ref = [torch.empty(C.CHUNK * per * nst, dtype=torch.uint8, device=DEV) for _ in out]
        ins = [dfr[b] for b in basis]
        torch.cuda.synchronize()
        if targets is None:
            L.decode_verified_device(0, stream, nst, avail_mask, dfr, out[0], bad)
            L.decode_device(0, stream, nst, bmask, ins, ref[0])
        else:
            L.heal_verified_device(0, stream, nst, avail_mask, dfr, C.mask_of(targets), out, bad)
            L.heal_device(0, stream, nst, bmask, ins, C.mask_of(targets), ref)
        L.verify_device(0, stream, nst, bmask, ins, cmask, [dfr[b] for b in checks], bad_ref)
        ec.sync_device(0, stream)
        for b, a in enumerate(frags):
            assert np.array_equal(dfr[b].cpu().numpy(), filler if a is None else a), \
                "the buffer of brick %d was written" % b
        return dict(bad=read_bad(bad, nst), out=[read_out(o, per * nst) for o in out], nbad=None,
                    bad_ref=read_bad(bad_ref, nst), out_ref=[h.cpu().numpy() for h in ref])
    return run


@pytest.mark.parametrize("nst", C.SIZES + [1027])
@pytest.mark.parametrize("geom", C.DECODE_GEOMS + C.HEAL_GEOMS, ids=C.geom_id)
def test_verified_device_matches_rule(ec, oracle, geom, nst):
    k, n, avail_mask, targets = geom
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets), oracle, k, n,
                       avail_mask, targets, nst)


@pytest.mark.parametrize("geom", [C.GEOM_ALL_31, C.GEOM_MOST_ROWS, C.GEOM_29], ids=C.geom_id)
def test_verified_device_16_plus_15(ec, oracle, geom):
    """A 16+15 volume, 9 stripes: a read of all 31 bricks (31 staged inputs,
    15 check rows and 16 output rows: the 62 KiB tile and 124 words of
    coefficients), a heal from 17 bricks of the other 14 (the most rows of a
    heal) and one from 29 bricks of the other 2 (its largest tile)."""
    k, n, avail_mask, targets = geom
    nst = 9
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets), oracle, k, n,
                       avail_mask, targets, nst)


@pytest.mark.parametrize("geom", [C.DECODE_GEOMS[1], C.DECODE_GEOMS[8], C.HEAL_GEOMS[0],
                                  C.HEAL_GEOMS[3]], ids=C.geom_id)
def test_verified_device_buffers_at_odd_addresses(ec, oracle, geom):
    """Every fragment starting 1 byte into its allocation (LDS-DMA stages them
    in place) and every output 1 byte into its own."""
    k, n, avail_mask, targets = geom
    nst = 67
    with ec.ECMatrixList(k, n) as L:
        C.run_geometry(device_runner(ec, L, k, n, nst, avail_mask, targets, offset=1), oracle, k,
                       n, avail_mask, targets, nst)


def test_verified_device_on_a_callers_stream(ec, oracle):
    """decode_verified_device and heal_verified_device of a degraded 4+2
    queued back to back on a caller's stream, one sync."""
    import torch
    k, n, nst, avail_mask = 4, 6, 67, 0x1F
    clean, data = C.clean_state(oracle, k, n, avail_mask, nst)
    frags = [clean[b].copy() for b in range(5)] + [None]
    want = np.zeros(nst, np.uint32)
    for t in range(0, nst, 3):                               # check brick 4 only
        frags[4] = C.flipped(frags[4], t, (41 * t + 9) % C.CHUNK, t % 8)
        want[t] = 1 << 4
    dfr = [None if f is None else dev(f) for f in frags]
    bad, bad2 = new_bad(nst), new_bad(nst)
    out, outh = new_out(k * nst), new_out(nst)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.decode_verified_device(0, st.cuda_stream, nst, avail_mask, dfr, out, bad)
        L.heal_verified_device(0, st.cuda_stream, nst, avail_mask, dfr, 1 << 5, [outh], bad2)
        ec.sync_device(0, st.cuda_stream)
    assert np.array_equal(read_bad(bad, nst), want)
    assert np.array_equal(read_bad(bad2, nst), want)
    assert np.array_equal(read_out(out, k * nst), data)
    assert np.array_equal(read_out(outh, nst), clean[5])


BIG = (6, 8, (1 << 17) + 5)


@pytest.fixture(scope="module")
def big(oracle):
    """6+2 fragments of 2^17 + 5 stripes, oracle-encoded once for both runs,
    and about 100 seeded single-bit flips in distinct stripes (stripe 0 and
    the last one among them) spread over bricks 0...6, each with the oracle's
    decode and heal of brick 7 from the stored chunks of bricks 0...5."""
    from types import SimpleNamespace
    k, n, nst = BIG
    rng = np.random.default_rng(829)
    data = rng.integers(0, 256, C.CHUNK * k * nst, dtype=np.uint8)
    frags = oracle.encode(k, n, data, nthreads=8)
    stripes = rng.choice(nst, size=100, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    dirty = []
    for j, t in enumerate(sorted(set(stripes.tolist()))):
        b = j % 7
        byte, bit = int(rng.integers(0, C.CHUNK)), 1 << int(rng.integers(0, 8))
        chunks = [f[t * C.CHUNK:(t + 1) * C.CHUNK].copy() for f in frags[:6]]
        if b < 6:
            chunks[b][byte] ^= np.uint8(bit)
        d = oracle.decode(k, list(range(1, 7)), chunks)
        h = oracle.encode(k, n, d)[7]
        # the MDS rule beside the oracle: a basis chunk spoils the outputs
        assert np.array_equal(d, data[t * k * C.CHUNK:(t + 1) * k * C.CHUNK]) == (b == 6), t
        assert np.array_equal(h, frags[7][t * C.CHUNK:(t + 1) * C.CHUNK]) == (b == 6), t
        dirty.append(dict(t=t, b=b, byte=byte, bit=bit, out=d, heal=h))
    assert {c["b"] for c in dirty} == set(range(7))
    return SimpleNamespace(data=data, frags=frags, dirty=dirty)     # dropped with the module


@pytest.mark.parametrize("off", [0, 1], ids=["aligned-nt", "offset-default"])
def test_verified_device_at_scale(ec, big, off):
    """6+2 with seven bricks, 2^17 + 5 stripes (64 MiB per fragment): above
    2^17 stripes k in 5...8 runs 4 waves per block.  Aligned fragments: the
    call reads more than 256 MiB and stages with non-temporal loads; fragments
    1 byte off: default-policy loads.  The outputs are compared on the
    device."""
    import torch
    k, n, nst = BIG
    kc = k * C.CHUNK
    dfr = [dev(f, off) for f in big.frags[:7]] + [None]
    want = np.zeros(nst, np.uint32)
    exp = torch.from_numpy(big.data).to(DEV)
    exph = torch.from_numpy(big.frags[7]).to(DEV).clone()
    for c in big.dirty:
        t = c["t"]
        dfr[c["b"]][t * C.CHUNK + c["byte"]] ^= c["bit"]
        want[t] = 0x40                                       # brick 6, the one check brick
        exp[t * kc:(t + 1) * kc] = torch.from_numpy(c["out"]).to(DEV)
        exph[t * C.CHUNK:(t + 1) * C.CHUNK] = torch.from_numpy(c["heal"]).to(DEV)
    bad, badh = new_bad(nst), new_bad(nst)
    out, outh = new_out(k * nst, off), new_out(nst, off)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.decode_verified_device(0, None, nst, 0x7F, dfr, out, bad)
        L.heal_verified_device(0, None, nst, 0x7F, dfr, 0x80, [outh], badh)
        ec.sync_device(0)
    assert torch.equal(out[:kc * nst], exp), "decode_verified out"
    assert (out[kc * nst:] == C.FILL).all(), "guard chunk written"
    assert torch.equal(outh[:C.CHUNK * nst], exph), "heal_verified out"
    assert (outh[C.CHUNK * nst:] == C.FILL).all(), "guard chunk written"
    del exp, exph, out, outh
    for c in big.dirty:                                      # undo the damage: as uploaded?
        dfr[c["b"]][c["t"] * C.CHUNK + c["byte"]] ^= c["bit"]
    for b in range(7):
        assert torch.equal(dfr[b], torch.from_numpy(big.frags[b]).to(DEV)), \
            "fragment %d was written" % b
    del dfr
    for name, got in (("decode_verified", bad), ("heal_verified", badh)):
        g = read_bad(got, nst)
        assert np.array_equal(g, want), (name, np.flatnonzero(g != want)[:16])
    torch.cuda.empty_cache()


def test_verified_rejects_mixed_host_and_device_buffers(ec, oracle):
    """Device tensors given to the host entry points, host arrays to the
    device entry points, all of them or mixed: -EINVAL, nothing written."""
    k, n, avail_mask, targets = C.HEAL_GEOMS[3]              # 8+4, 0x2FF, {8, 10, 11}
    nst, tmask = 4, C.mask_of(targets)
    clean = C.fragments(oracle, k, n, nst)
    frags = [clean[b] if (avail_mask >> b) & 1 else None for b in range(n)]
    dfr = [None if f is None else dev(f) for f in frags]
    hbad = np.full(nst, C.SENTINEL, np.uint32)
    dbad = new_bad(nst)
    hout = [np.full(C.CHUNK * nst, C.FILL, np.uint8) for _ in targets]
    dout = [new_out(nst) for _ in targets]
    hdec = np.full(k * C.CHUNK * nst, C.FILL, np.uint8)
    ddec = new_out(k * nst)

    def swap(lst, b, other):
        return lst[:b] + [other[b]] + lst[b + 1:]

    def rejected(fn, name, *args):
        with pytest.raises(OSError) as e:
            fn(*args)
        assert e.value.errno == errno.EINVAL
        assert name in str(e.value)

    with ec.ECMatrixList(k, n) as L:
        for fr, out, dec, bad in (
                (dfr, dout, ddec, dbad),                             # all on the device
                (dfr, hout, hdec, hbad),
                (swap(frags, 1, dfr), hout, hdec, hbad),             # a basis brick
                (swap(frags, 9, dfr), hout, hdec, hbad),             # the check brick
                (frags, dout, ddec, hbad),
                (frags, hout, hdec, dbad)):
            rejected(L.heal_verified, "ec_method_heal_verified", nst, avail_mask, fr, tmask, out,
                     bad)
            rejected(L.decode_verified, "ec_method_decode_verified", nst, avail_mask, fr, dec, bad)
        rejected(L.heal_verified, "ec_method_heal_verified", nst, avail_mask, frags,
                 tmask, [hout[0], dout[1], hout[2]], hbad)
        for fr, out, dec, bad in (
                (swap(dfr, 1, frags), dout, ddec, dbad),
                (swap(dfr, 9, frags), dout, ddec, dbad),
                (dfr, hout, hdec, dbad),
                (dfr, dout, ddec, hbad)):
            rejected(L.heal_verified_device, "ec_method_heal_verified_device", 0, None, nst,
                     avail_mask, fr, tmask, out, bad)
            rejected(L.decode_verified_device, "ec_method_decode_verified_device", 0, None, nst,
                     avail_mask, fr, dec, bad)
        rejected(L.heal_verified_device, "ec_method_heal_verified_device", 0, None, nst,
                 avail_mask, dfr, tmask, [dout[0], hout[1], dout[2]], dbad)
        ec.sync_device(0)
    assert (hbad == C.SENTINEL).all() and all((o == C.FILL).all() for o in hout + [hdec])
    assert (dbad.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
    assert all((o.cpu().numpy() == C.FILL).all() for o in dout + [ddec])


NT_SCRIPT = r"""
import sys
sys.path.insert(0, "oracle")
import numpy as np, torch
import glusterfs_amd as g
import oracle as O           # the checker

rng = np.random.default_rng(11)
def dev(a):
    return torch.from_numpy(a).cuda()
def u32(t):
    return t.cpu().numpy().view(np.uint32)

# 13 stripes (three full tiles and a ragged one) of the three K buckets, from
# the k + 1 lowest bricks: a damaged basis chunk, and a damaged check chunk in
# the ragged tile.  Expected values from the oracle on the chunks as stored.
for k, n in ((4, 6), (8, 12), (16, 20)):
    sn = 13
    data = rng.integers(0, 256, 512 * k * sn, dtype=np.uint8)
    clean = O.encode(k, n, data)
    fr = [f.copy() for f in clean]
    fr[1][2 * 512 + 37] ^= 0x10
    fr[k][12 * 512 + 300] ^= 0x01
    rows = list(range(1, k + 1))
    want_out = O.decode(k, rows, fr[:k])
    want_heal = O.encode(k, n, want_out)[n - 1]
    want_bad = np.zeros(sn, np.uint32)
    want_bad[2] = want_bad[12] = 1 << k
    same = np.ones(sn, bool)
    same[2] = False
    assert (want_out.reshape(sn, -1) == data.reshape(sn, -1)).all(axis=1).tolist() == same.tolist()
    assert (want_heal.reshape(sn, -1) == clean[n - 1].reshape(sn, -1)).all(axis=1).tolist() == \
        same.tolist()
    sd = [dev(f) for f in fr[:k + 1]] + [None] * (n - k - 1)
    bad = torch.full((sn,), -1, dtype=torch.int32, device="cuda")
    badh = bad.clone()
    out = torch.full((512 * k * sn,), 0xA5, dtype=torch.uint8, device="cuda")
    outh = torch.full((512 * sn,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with g.ECMatrixList(k, n) as L:
        L.decode_verified_device(0, None, sn, (2 << k) - 1, sd, out, bad)
        L.heal_verified_device(0, None, sn, (2 << k) - 1, sd, 1 << (n - 1), [outh], badh)
        g.sync_device(0)
    assert np.array_equal(u32(bad), want_bad), ("decode_verified bad", k, u32(bad))
    assert np.array_equal(u32(badh), want_bad), ("heal_verified bad", k, u32(badh))
    assert np.array_equal(out.cpu().numpy(), want_out), ("decode_verified out", k)
    assert np.array_equal(outh.cpu().numpy(), want_heal), ("heal_verified out", k)
print("ok")
"""


def test_verified_device_non_temporal_instantiations():
    """EC_MI355X_LDSNT=1 (read when the library loads) stages these small
    calls with non-temporal loads: both kernels at K = 4, 8 and 16, in a
    process of their own."""
    env = dict(os.environ, EC_MI355X_QUIET="1", EC_MI355X_LDSNT="1")
    r = subprocess.run([sys.executable, "-c", NT_SCRIPT], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
