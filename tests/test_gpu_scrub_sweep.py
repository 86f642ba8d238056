"""The eight scrub entry points on device buffers over every brick, every pair
of bricks and every k from 2 to 16 (tests/_scrub_sweep.py): the six tile
kernels (ec_verify_n, ec_locate_n, ec_locate2_n, ec_decode_checked_n,
ec_decode_checked2_n, ec_heal_checked_n) and ec_repair_n / ec_repair2_n, with
the run-time k at every value of each K bucket (2...4, 5...8, 9...16), every
entry of the pair tables that travel in the kernel arguments, drawn
avail_masks with a basis above brick 24, and every buffer 1 byte into its
allocation for one geometry per bucket.  test_scrub_at_scale launches the
4-wave instantiations (5 <= k <= 8 above 2^17 stripes) with the non-temporal
staging (aligned fragments, more than 256 MiB read) and with the default one
(fragments 1 byte off).

The expected values come from the oracle and include/ec_method.h, never from
the library.  loc[] / bad[] are pre-filled with 0xFFFFFFFF and followed by
guard words, outputs with 0xA5 and a guard chunk, and no fragment may change
in a call that only reads.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import _scrub_sweep as W

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
    return torch.full((nst + W.GUARD,), -1, dtype=torch.int32, device=DEV)


def read_loc(loc, nst):
    got = loc.cpu().numpy().view(np.uint32)
    assert (got[nst:] == W.SENTINEL).all(), "guard words written"
    return got[:nst].copy()


def new_out(chunks, offset=0):
    """`chunks` chunks and a guard chunk of 0xA5, `offset` bytes into the
    allocation."""
    import torch
    t = torch.full((W.CHUNK * (chunks + 1) + offset,), W.FILL, dtype=torch.uint8, device=DEV)
    return t[offset:]


def read_out(out, chunks):
    got = out.cpu().numpy()
    assert (got[W.CHUNK * chunks:] == W.FILL).all(), "guard chunk written"
    return got[:W.CHUNK * chunks].copy()


def same_loc(got, want, S, what):
    d = np.flatnonzero(got != want)
    assert d.size == 0, (what, [(t, S.cases[t], hex(got[t]), hex(want[t])) for t in d[:8]])


def same_stripes(got, want, width, S, what):
    d = np.flatnonzero((got.reshape(S.nst, width) != want.reshape(S.nst, width)).any(axis=1))
    assert d.size == 0, (what, [(t, S.cases[t]) for t in d[:8]])


def upload(frags, off):
    return [None if f is None else dev(f, off) for f in frags]


def same_fragments(dfr, want, S, what):
    for b, (d, w) in enumerate(zip(dfr, want)):
        if w is not None:
            same_stripes(d.cpu().numpy(), w, W.CHUNK, S, (what, "brick %d" % b))


def sweep(ec, geom, off):
    """All eight device calls of one geometry; every fragment and every
    output starts `off` bytes into its allocation (loc[] wants 4)."""
    import torch
    S = W.built(geom)
    k, n, nst, am = S.k, S.n, S.nst, S.avail_mask
    targets = W.targets_of(geom)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    with ec.ECMatrixList(k, n) as L:
        # the calls that only read, queued on one stream, one sync
        dfr = upload(S.frags, off)
        bad, loc1, locd1, loch, loc2, locd2 = (new_loc(nst) for _ in range(6))
        out1, out2 = new_out(k * nst, off), new_out(k * nst, off)
        outh = [new_out(nst, off) for _ in targets]
        torch.cuda.synchronize()
        L.verify_device(0, s, nst, W.mask_of(S.basis), [dfr[b] for b in S.basis],
                        W.mask_of(S.checks), [dfr[b] for b in S.checks], bad)
        L.locate_device(0, s, nst, am, dfr, loc1)
        if S.two:
            L.locate2_device(0, s, nst, am, dfr, loc2)
        L.decode_checked_device(0, s, nst, am, dfr, out1, locd1)
        if S.two:
            L.decode_checked2_device(0, s, nst, am, dfr, out2, locd2)
        if targets:
            L.heal_checked_device(0, s, nst, am, dfr, W.mask_of(targets), outh, loch)
        ec.sync_device(0, s)
        same_loc(read_loc(bad, nst), S.bad, S, "verify")
        same_loc(read_loc(loc1, nst), S.loc1, S, "locate")
        same_loc(read_loc(locd1, nst), S.loc1, S, "decode_checked loc")
        same_stripes(read_out(out1, k * nst), S.out1, k * W.CHUNK, S, "decode_checked out")
        if S.two:
            same_loc(read_loc(loc2, nst), S.loc2, S, "locate2")
            same_loc(read_loc(locd2, nst), S.loc2, S, "decode_checked2 loc")
            same_stripes(read_out(out2, k * nst), S.data, k * W.CHUNK, S, "decode_checked2 out")
        if targets:
            same_loc(read_loc(loch, nst), S.loc1, S, "heal_checked loc")
            for j, o in zip(targets, outh):
                same_stripes(read_out(o, nst), S.heal1[j], W.CHUNK, S, ("heal_checked", j))
        same_fragments(dfr, S.frags, S, "a call that only reads")

        # repair on locate's answer, then locate: zero wherever a brick was named
        loc, again = new_loc(nst), new_loc(nst)
        loc[:nst].copy_(torch.from_numpy(S.loc1.view(np.int32).copy()))
        torch.cuda.synchronize()
        L.repair_device(0, s, nst, am, dfr, loc)
        L.locate_device(0, s, nst, am, dfr, again)
        ec.sync_device(0, s)
        assert np.array_equal(read_loc(loc, nst), S.loc1), "repair wrote loc"
        same_fragments(dfr, S.rep1, S, "repair")
        same_loc(read_loc(again, nst), np.where(S.loc1 == W.MANY, S.loc1, 0), S,
                 "locate after repair")

        # repair2 on the bits of the damaged bricks (locate2's answer where it
        # can run), then locate2 (locate beside fewer than k + 4 bricks): zero
        dfr = upload(S.frags, off)
        loc, again = new_loc(nst), new_loc(nst)
        loc[:nst].copy_(torch.from_numpy(S.loc2.view(np.int32).copy()))
        torch.cuda.synchronize()
        L.repair2_device(0, s, nst, am, dfr, loc)
        (L.locate2_device if S.two else L.locate_device)(0, s, nst, am, dfr, again)
        ec.sync_device(0, s)
        assert np.array_equal(read_loc(loc, nst), S.loc2), "repair2 wrote loc"
        same_fragments(dfr, [S.clean[b] if f is not None else None
                             for b, f in enumerate(S.frags)], S, "repair2")
        assert not read_loc(again, nst).any(), "locate after repair2"

        if S.two:           # and with k + 2 of the bricks, on the pairs inside them
            dfr = upload(S.frags, off)
            loc[:nst].copy_(torch.from_numpy(S.loc_sub.view(np.int32).copy()))
            torch.cuda.synchronize()
            L.repair2_device(0, s, nst, S.sub_mask, dfr, loc)
            ec.sync_device(0, s)
            same_fragments(dfr, S.rep_sub, S, "repair2 on k + 2 bricks")


@pytest.mark.parametrize("geom", W.SWEEP, ids=W.geom_id)
def test_scrub_sweep_device(ec, geom):
    sweep(ec, geom, 0)


@pytest.mark.parametrize("geom", W.offset_geoms(), ids=W.geom_id)
def test_scrub_sweep_device_buffers_at_odd_addresses(ec, geom):
    sweep(ec, geom, 1)


# --- the 4-wave bucket: 5 <= k <= 8 above 2^17 stripes -----------------------

BIG = (6, 11, (1 << 17) + 5)


@pytest.fixture(scope="module")
def big(oracle):
    """6+5 fragments of 2^17 + 5 stripes, oracle-encoded once for both runs,
    about 100 seeded dirty stripes (stripe 0 and the last one among them) with
    one or two damaged chunks spread over bricks 0...9, and per dirty stripe
    the expected values of every call: the rule for locate2 and
    decode_checked2 on bricks 0...9, the definition (evaluated on that
    stripe's chunks by the oracle) for the calls on bricks 0...7."""
    k, n, nst = BIG
    rng = np.random.default_rng(617)
    data = rng.integers(0, 256, W.CHUNK * k * nst, dtype=np.uint8)
    frags = oracle.encode(k, n, data, nthreads=8)
    stripes = rng.choice(nst, size=100, replace=False)
    stripes[0], stripes[1] = 0, nst - 1
    stripes = sorted(set(stripes.tolist()))
    av10, av8 = list(range(10)), list(range(8))
    dirty = []
    for j, t in enumerate(stripes):
        b = j // 2 % 10
        bricks = [b] if j % 2 == 0 else [b, (b + 1 + j // 20 % 9) % 10]
        assert len(set(bricks)) == len(bricks)
        flips = [(x, int(rng.integers(0, W.CHUNK)), 1 << int(rng.integers(0, 8))) for x in bricks]
        chunks = [W.chunk(f, t).copy() for f in frags]
        for x, byte, bit in flips:
            chunks[x][byte] ^= np.uint8(bit)
        loc, bad, d, e = W.expected_stripe(oracle, k, n, av8, chunks)
        in8 = [x for x in bricks if x < 8]
        # the rule, beside the definition: one damaged chunk among 0...7 is
        # named and decoded around; none leaves the stripe clean
        if len(in8) < 2:
            assert loc == W.mask_of(in8), (t, bricks, hex(loc))
            assert np.array_equal(d, data[t * k * W.CHUNK:(t + 1) * k * W.CHUNK]), t
        dirty.append(dict(t=t, flips=flips, loc2=W.mask_of(bricks), loc1=loc, bad=bad, out1=d,
                          heal1=e[10]))
    # the definition of locate2 on 8 of them
    import _locate2_cases as L2
    for c in dirty[:8]:
        chunks = [W.chunk(f, c["t"]).copy() for f in frags]
        for x, byte, bit in c["flips"]:
            chunks[x][byte] ^= np.uint8(bit)
        assert L2.expected_loc2(oracle, k, n, av10, chunks, 0) == c["loc2"], c["t"]
    assert sum(len(c["flips"]) == 2 for c in dirty) >= 40
    assert {x for c in dirty for x, _, _ in c["flips"]} == set(av10)
    return SimpleNamespace(data=data, frags=frags, dirty=dirty)     # dropped with the module


@pytest.mark.parametrize("off", [0, 1], ids=["aligned-nt", "offset-default"])
def test_scrub_at_scale(ec, big, off):
    """6+5, 2^17 + 5 stripes (64 MiB per fragment): above 2^17 stripes k in
    5...8 runs 4 waves per block.  Aligned fragments: every call reads more
    than 256 MiB and stages with non-temporal loads; fragments 1 byte off:
    default-policy loads.  The big outputs are compared on the device."""
    import torch
    k, n, nst = BIG
    kc = k * W.CHUNK
    am10, am8 = 0x3FF, 0xFF
    dfr = [dev(f, off) for f in big.frags]
    for c in big.dirty:
        for x, byte, bit in c["flips"]:
            dfr[x][c["t"] * W.CHUNK + byte] ^= bit
    want2 = np.zeros(nst, np.uint32)
    want1, wbad = want2.copy(), want2.copy()
    exp = torch.from_numpy(big.data).to(DEV)                 # decode_checked2: the data
    exph = torch.from_numpy(big.frags[10]).to(DEV).clone()   # heal_checked: clean brick 10
    for c in big.dirty:
        want2[c["t"]], want1[c["t"]], wbad[c["t"]] = c["loc2"], c["loc1"], c["bad"]
        exph[c["t"] * W.CHUNK:(c["t"] + 1) * W.CHUNK] = torch.from_numpy(c["heal1"]).to(DEV)
    bad, loc1, locd1, loch, loc2, locd2 = (new_loc(nst) for _ in range(6))
    out, outh = new_out(k * nst, off), new_out(nst, off)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        L.locate2_device(0, None, nst, am10, dfr, loc2)
        L.decode_checked2_device(0, None, nst, am10, dfr, out, locd2)
        ec.sync_device(0)
        assert torch.equal(out[:kc * nst], exp), "decode_checked2 out"
        assert (out[kc * nst:] == W.FILL).all(), "guard chunk written"
        out.fill_(W.FILL)
        for c in big.dirty:                                  # decode_checked: by the definition
            exp[c["t"] * kc:(c["t"] + 1) * kc] = torch.from_numpy(c["out1"]).to(DEV)
        torch.cuda.synchronize()
        L.verify_device(0, None, nst, 0x3F, dfr[:6], 0xC0, dfr[6:8], bad)
        L.locate_device(0, None, nst, am8, dfr, loc1)
        L.decode_checked_device(0, None, nst, am8, dfr, out, locd1)
        L.heal_checked_device(0, None, nst, am8, dfr, 1 << 10, [outh], loch)
        ec.sync_device(0)
    assert torch.equal(out[:kc * nst], exp), "decode_checked out"
    assert (out[kc * nst:] == W.FILL).all(), "guard chunk written"
    assert torch.equal(outh[:W.CHUNK * nst], exph), "heal_checked out"
    assert (outh[W.CHUNK * nst:] == W.FILL).all(), "guard chunk written"
    del exp, exph, out, outh
    for c in big.dirty:                                      # undo the damage: as uploaded?
        for x, byte, bit in c["flips"]:
            dfr[x][c["t"] * W.CHUNK + byte] ^= bit
    for b in range(n):
        assert torch.equal(dfr[b], torch.from_numpy(big.frags[b]).to(DEV)), \
            "fragment %d was written" % b
    del dfr
    for name, got, want in (("locate2", loc2, want2), ("decode_checked2 loc", locd2, want2),
                            ("verify", bad, wbad), ("locate", loc1, want1),
                            ("decode_checked loc", locd1, want1),
                            ("heal_checked loc", loch, want1)):
        g = read_loc(got, nst)
        assert np.array_equal(g, want), (name, np.flatnonzero(g != want)[:16])
    torch.cuda.empty_cache()
