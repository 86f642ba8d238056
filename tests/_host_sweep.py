"""Shared case table of tests/test_host_sweep.py (CPU engine) and
tests/test_gpu_host_sweep.py (the GPU pipeline): the fourth kernel family, host
buffers coded over PCIe.  Its parts are ecdk_combine_host and its kernels
(ec_combine_zc<4|8|16>, ec_combine_zc_db<4|8|16, 8, MIXED, 8> and
ec_combine_zc_db<16, 8, MIXED, 4>), the register encoder ec_encode_vander_zc,
and the batching of ec_device.hip (run_encode_dev, run_decode_dev,
run_pipeline, staged_batch, the Region / slot arithmetic, add_gather).

Nothing here calls the library.  All fragments are random bytes and the
expected values are the oracle's: decode = oracle.decode, encode =
oracle.encode, heal and row-masked encode of brick b = oracle.encode(k, n,
oracle.decode(k, rows, sources))[b], write = oracle.encode(k, n,
oracle.writev_merge(...)); k = 1 follows tests/_combine_sweep.py (the decode
of a fragment is that fragment).  Coding is stripe by stripe, so a series of
calls shares one reference computed at its largest count: a call of c stripes
expects the first c stripes of it.

Which kernel a call launches is counted by restated predicates, plain-Python
copies of the library's decisions:
  branch(k, rows, launch, zcdb, group, npat)  ecdk_combine_host: A zc_db<4>,
      B zc_db<8>, C zc_db<16> with 8-stripe tiles, D zc_db<16, .., 4>,
      E ec_combine_zc<K>, F combine_any<false>;
  encoder(k, n, launch, zcenc16)  launch_encode / launch_vander: "vander"
      (one pass), "vander_zc" or "combine";
  launches(...)  the stripe counts of a call's launches: B of run_encode_dev /
      run_decode_dev with staged_batch.

The host mixed decode takes one mask per group and numbers the distinct ones
itself, so no id is past the list there; the id past the list of
_combine_sweep._mixed becomes the last mask.

A buffer is 'P' pinned and 16-byte aligned (coded in place), 'G' pageable,
'M' pinned at +8 bytes (must stage) or 'R' inside a registered page-exact
mapping (in place).  A call's `place` names the kind of every buffer: the
inputs in order, then the outputs.

Coverage clauses, asserted at the end of the module:
  H1  every k from 1 to 16 with k + 2 bricks and with 31; 2+1, 4+2, 8+4, 16+4;
  H2  every call shape of every geometry at 1...17, 23, 24, 25, 33 and 41
      stripes, each all-pinned, all-pageable, at +8 and registered;
  H3  per geometry and call kind every buffer position once the only staged
      one and once the only mapped one;
  H4  decode rows = k; heals of 1, 2 and all n - k bricks; row masks of one
      bit and of all n;
  H5  by default every branch A...F is launched by a single-pattern call, and
      A, B, C, D, E (K = 4, 8, 16) and F by a mixed one; with ZCDB=0 branch E
      by single and mixed calls of every K;
  H6  the named geometries: 8+12 and 4+22 encodes (E, more than 64 KiB of
      LDS), 9+12 (rows 21: C) and 9+13 (rows 22: E), 16+4 heals of 1 and 4
      rows and 16+8 heals of 7 (C) and 8 rows (E), 16+15 at 2053 (D, 2k + rows
      = 63) and at 41 stripes (F), 12+19 (F);
  H7  D beside its 2048-stripe edge: 2047, 2048, 2049, 2053 for every k > 8;
  H8  the encoders beside T = 8192 / 4096 / 2048 (T - 1, T, T + 1, T + 259)
      and 16+4 at 8191, 8192, 8195, all pinned: both sides of every switch;
  H9  mixed decodes with groups of 1, 2, 4 (F), 8, 16, 64 (MIXED kernels), and
      for k = 3, 7, 15 exactly fit(k) masks and one more (-E2BIG: F);
  H10 staged calls that staged_batch cuts in 2, 3 and 4;
  H11 writes of 4+2, 8+4, 5+2, 10+3: heads {0, 1, 17, S - 1}, ends {0, 1,
      S - 1}, 1, 2, 3 and 9 merged stripes;
  H12 (small batches, EC_PIPE_BATCH_MB=1) every call kind as 1, 2, 3 and 5
      staged batches with a last batch of 1, B - 1 and B stripes, mapped calls
      of B - 1, B and B + 1, mixed calls whose B is rounded down to the group
      with a partial last group, a write whose segments straddle batch
      boundaries, and every staged 16+4 encode launch below 2048 stripes.
"""
import functools
from types import SimpleNamespace

import numpy as np

import _combine_sweep as CS

CHUNK = 512
FILL = 0xA5
GUARD = 4096                    # one 8-stripe row run of a tile
FLANK = 64
COUNTS = tuple(range(1, 18)) + (23, 24, 25, 33, 41)
D_COUNTS = (2047, 2048, 2049, 2053)
TILE_ENCODER = CS.TILE_ENCODER
VANDER_W = {2: 4, 4: 2, 8: 1, 16: 1}            # launch_vander<K, N, W>
THRESHOLD = {(2, 3): 8192, (4, 6): 4096, (8, 12): 2048}
ENC16 = (8191, 8192, 8195)
MAPPED = "PR"

bits, mask_of, rows_of, geom_id = CS.bits, CS.mask_of, CS.rows_of, CS.geom_id

SPECIAL = [(8, 20), (4, 26), (9, 21), (9, 22), (16, 24)]
GEOMS = sorted({(k, n) for k in range(1, 17) for n in (k + 2, 31)} | TILE_ENCODER | set(SPECIAL))
WRITE_GEOMS = [(4, 6), (8, 12), (5, 7), (10, 13)]
EXTRA_HEAL = {(16, 20): (4,), (16, 24): (7, 8)}
CUT_COUNTS = {1024 + 3: 2, 1536 + 1: 3, 2048 + 5: 4}       # 4+2, pageable: batches


# --- the restated predicates -------------------------------------------------

def branch(k, rows, launch, zcdb=True, group=0, npat=1):
    """ecdk_combine_host's decision for one launch of `launch` stripes."""
    e2big = CS.pwords(k, rows) * npat > CS.ARG_WORDS
    db4 = k > 8 and launch >= 2048 and 2 * k + rows <= 64
    wide = k + rows > 32 and not (zcdb and db4)
    if e2big or wide or 0 < group < 8:
        return "F"
    if zcdb:
        db16 = k > 8 and 2 * k + rows <= 39
        if not db16 and db4:
            return "D"
        if k <= 8 and 2 * k + rows <= 32:
            return "A" if k <= 4 else "B"
        if db16:
            return "C"
    return "E"


def lds_e(k, rows):
    """Dynamic LDS of branch E."""
    return (k + rows) * 8 * CHUNK


def encoder(k, n, launch, zcenc16=True):
    """launch_encode's decision for one launch of a plain host encode."""
    if (k, n) not in TILE_ENCODER:
        return "combine"
    if k > 8 and 2048 <= launch < 8192 and zcenc16:
        return "combine"
    return "vander_zc" if launch * (16 // VANDER_W[k]) > 4 * 32 * 256 else "vander"


def staged_batch(full, count, in_stripe, unit=1, split=4):
    if split <= 1 or count > full:
        return full
    min_st = max(1, (1 << 20) // in_stripe)
    nb = min(split, count // min_st)
    if nb <= 1:
        return full
    b = -(-count // nb)
    return max(-(-b // unit) * unit, unit)


def batch(encode, count, in_stripe, all_direct, batch_mb=32, group=1):
    """B of run_encode_dev (encode) / run_decode_dev: stripes per batch."""
    full = max(1, (8 if all_direct else 1) * (batch_mb << 20) // in_stripe)
    if encode:
        B = min(count, full)
        return B if all_direct else min(count, staged_batch(B, count, in_stripe))
    B = full if all_direct else staged_batch(full, count, in_stripe)
    return max(group, B // group * group) if group > 1 else B


def cut(count, B):
    return [min(B, count - a) for a in range(0, count, B)]


# --- calls -------------------------------------------------------------------

def shape_rows(g, sh):
    k, n = g
    return {"enc": n, "dec": k, "mixed": k, "write": n}.get(sh[0]) or len(bits(sh[-1]))


def npos(g, sh):
    """Buffers of a call: (inputs, outputs)."""
    k, n = g
    kind = sh[0]
    if kind in ("enc", "rows"):
        return 1, shape_rows(g, sh)
    if kind == "write":
        return 0, n
    return (n if kind == "mixed" else k), (1 if kind in ("dec", "mixed") else shape_rows(g, sh))


def call(g, sh, nst, place, series):
    return SimpleNamespace(g=g, sh=sh, nst=nst, place=place, series=series)


def call_id(c):
    return "%s %s: %d stripes, buffers %s" % (geom_id(c.g), shape_id(c.sh), c.nst, c.place)


def shape_id(sh):
    if sh[0] == "mixed":
        return "mixed[groups of %d, %d masks]" % (sh[1].group, len(sh[1].masks))
    if sh[0] == "write":
        return "write[head %d, %d bytes, old %s/%s, %d iovecs]" % sh[1:]
    return sh[0] + "".join("[%#x]" % m for m in sh[1:])


def launches_of(c, batch_mb=32):
    """The stripe counts of the launches of call c."""
    k, n = c.g
    kind = c.sh[0]
    direct = all(p in MAPPED for p in c.place)
    if kind in ("enc", "rows", "write"):
        # a write's padded input is always gathered into the staging slots
        return cut(c.nst, batch(True, c.nst, k * CHUNK, direct and kind != "write", batch_mb))
    if kind == "mixed":
        return cut(c.nst, batch(False, c.nst, n * CHUNK, direct, batch_mb, c.sh[1].group))
    return cut(c.nst, batch(False, c.nst, k * CHUNK, direct, batch_mb))


def kernels_of(c, zcdb=True, batch_mb=32, zcenc16=True):
    """What the launches of call c run: a set of "A"..."F" / "vander" /
    "vander_zc" (a 16+4 encode as a combine counts as its branch)."""
    k, n = c.g
    out = set()
    # (a row mask of all n bricks is ec_method_encode itself)
    plain = c.sh[0] in ("enc", "write") or (c.sh[0] == "rows" and c.sh[1] == (1 << n) - 1)
    for ln in launches_of(c, batch_mb):
        if plain and encoder(k, n, ln, zcenc16) != "combine":
            out.add(encoder(k, n, ln, zcenc16))
        elif c.sh[0] == "mixed":
            out.add(branch(k, k, ln, zcdb, c.sh[1].group, len(set(c.sh[1].masks))))
        else:
            out.add(branch(k, shape_rows(c.g, c.sh), ln, zcdb))
    return out


def _rng(k, n, salt):
    return np.random.default_rng((k * 64 + n) * 100 + 7000 + salt)


def _shapes(g):
    """The count-independent calls of a geometry."""
    k, n = g
    rng = _rng(k, n, 1)
    out = [("enc",)]
    drawn = mask_of(rng.choice(n, size=int(rng.integers(2, n)), replace=False))
    out += [("rows", m) for m in dict.fromkeys([1 << int(rng.integers(0, n)), drawn, (1 << n) - 1])]
    masks = CS.draw_masks(k, n, 3, 41)
    dec = list(dict.fromkeys([masks[0], masks[-1]]))
    out += [("dec", m) for m in dec]
    m = dec[-1]
    outside = [b for b in range(n) if not (m >> b) & 1]
    sizes = [1, 2, len(outside)] + ([int(rng.integers(3, len(outside)))] if len(outside) > 3 else [])
    sizes += list(EXTRA_HEAL.get(g, ()))
    for s in dict.fromkeys(x for x in sizes if x <= len(outside)):
        t = outside if s == len(outside) else sorted(rng.choice(outside, size=s, replace=False))
        out.append(("heal", m, mask_of(t)))
    return out


def _mixes(np_in, np_out):
    """Every position once the only staged and once the only mapped buffer."""
    P = np_in + np_out
    out = []
    for p in range(P):
        out.append("".join("G" if i == p else "P" for i in range(P)))
        out.append("".join("P" if i == p else "G" for i in range(P)))
    return out if P > 1 else ["P", "G"]


def _small(g, sh, counts=COUNTS, series="small"):
    a, b = npos(g, sh)
    P = a + b
    mixes = _mixes(a, b)
    per = -(-len(mixes) // len(counts))
    out = []
    for i, nst in enumerate(counts):
        for kind in "PGMR":
            out.append(call(g, sh, nst, kind * P, series))
        for j in range(per):
            out.append(call(g, sh, nst, mixes[(i * per + j) % len(mixes)], series))
    return out


def _mixed_shapes(g):
    k, n = g
    out = [("mixed", CS._mixed(k, n, grp, 5, 50 + grp)) for grp in (1, 2, 4, 8, 16, 64)]
    if n == 31 and k in CS.EDGE_K:
        out += [("mixed", CS._mixed(k, n, 8, CS.fit(k) + past, 70 + past)) for past in (0, 1)]
    return out


def _reaches_d(g, sh):
    return g[0] > 8 and branch(g[0], shape_rows(g, sh), 2048) == "D"


@functools.lru_cache(maxsize=None)
def cases(g):
    """Every call of a geometry in the default process; no data yet."""
    k, n = g
    out = []
    shapes = _shapes(g)
    for sh in shapes:
        out += _small(g, sh)
    for sh in _mixed_shapes(g):
        a, b = npos(g, sh)
        mx = _mixes(a, b)
        r = int(_rng(k, n, sh[1].group).integers(0, len(mx) // 2))
        out += [call(g, sh, sh[1].nst, p, "mixed")
                for p in ["P" * (a + b), "G" * (a + b), "M" * (a + b), "R" * (a + b),
                          mx[2 * r], mx[2 * r + 1]]]
    # D beside its edge: one single-pattern shape per geometry with k > 8, all
    # pinned so that the launch is the call, and for 16+4 a mixed decode with
    # groups of 8 (D's MIXED instantiation: 2 tiles per group)
    dsh = [sh for sh in shapes if _reaches_d(g, sh)]
    if dsh and (n == 31 or g == (16, 20)):
        pick = [sh for sh in dsh if sh[0] == ("enc" if g == (16, 31) else dsh[0][0])][:1]
        if g == (16, 20):
            pick = [sh for sh in dsh if sh[0] == "dec"][:1]
        for sh in pick:
            P = sum(npos(g, sh))
            out += [call(g, sh, c, "P" * P, "d") for c in D_COUNTS]
    if g == (16, 20):
        x = CS._mixed(16, 20, 8, 5, 90)
        full = 2048 // 8 + 6
        rng = _rng(16, 20, 90)
        ids = list(range(1, 5)) + rng.integers(1, 5, full - 4).tolist()
        x = SimpleNamespace(group=8, masks=x.masks, last=5, nst=full * 8 + 5, table=False,
                            sorted=False, ids=np.array([ids[i] for i in rng.permutation(full)] + [0],
                                                       np.uint8))
        out += [call(g, ("mixed", x), x.nst, p * 21, "dmixed") for p in "PG"]
        out += [call(g, ("enc",), c, "P" * 21, "thr") for c in ENC16]
    if g in THRESHOLD:
        T = THRESHOLD[g]
        out += [call(g, ("enc",), c, "P" * (1 + n), "thr") for c in (T - 1, T, T + 1, T + 259)]
    if g == (4, 6):
        out += [call(g, ("enc",), c, p, "cut") for c in CUT_COUNTS
                for p in ("G" * 7, "GPPPPPP", "PPPGPPP")]
        sh = [s for s in shapes if s[0] == "dec"][0]
        out += [call(g, sh, c, p, "cut") for c in CUT_COUNTS for p in ("G" * 5, "PPPPG")]
    if g in WRITE_GEOMS:
        out += _writes(g)
    return out


def _writes(g):
    k, n = g
    S = CHUNK * k
    out, p = [], 0
    for nst in (1, 2, 3, 9):
        for head in (0, 1, 17, S - 1):
            for end in (0, 1, S - 1):
                b2 = (nst - 1) * S + (end or S)
                if b2 <= head:
                    continue
                oh, ot = [(True, True), (True, False), (False, True), (False, False)][p % 4]
                iov = 3 if (p % 2 and b2 - head >= 3) else 1
                out.append(call(g, ("write", head, b2 - head, oh, ot, iov), nst,
                                ("G" * n, "P" * n, "PG" * n)[p % 3][:n], "write"))
                p += 1
    return out


@functools.lru_cache(maxsize=None)
def batch_cases(g):
    """The calls of the EC_PIPE_BATCH_MB=1 process (clause H12)."""
    k, n = g
    out = []
    sh = {s[0]: s for s in _shapes(g)}
    for kind in ("enc", "rows", "dec", "heal"):
        s = sh[kind]
        a, b = npos(g, s)
        P = a + b
        B = batch(kind in ("enc", "rows"), 1 << 40, k * CHUNK, False, 1)
        for nb in (1, 2, 3, 5):
            for last in (1, B - 1, B):
                c = (nb - 1) * B + last
                if c * k * CHUNK <= 8 << 20:
                    out.append(call(g, s, c, "G" * P, "batch"))
                    out.append(call(g, s, c, _mixes(a, b)[(nb + last) % (2 * P)], "batch"))
        Bm = batch(kind in ("enc", "rows"), 1 << 40, k * CHUNK, True, 1)
        if kind in ("enc", "dec"):
            out += [call(g, s, c, "P" * P, "batch") for c in (Bm - 1, Bm, Bm + 1)]
    Bn = (1 << 20) // (n * CHUNK)
    for grp in (8, 64):
        x0 = CS._mixed(k, n, grp, 5, 50 + grp)
        full = 2 * (Bn // grp) + 2
        rng = _rng(k, n, grp)
        x = SimpleNamespace(group=grp, masks=x0.masks, last=5, nst=full * grp + 5,
                            ids=np.array(rng.integers(1, len(x0.masks), full).tolist() + [0],
                                         np.uint8))
        out += [call(g, ("mixed", x), x.nst, p * (n + 1), "bmixed") for p in "GP"]
    if g in WRITE_GEOMS:
        S = k * CHUNK
        B = (1 << 20) // S
        # old head | user | zero fill or old tail, each across a batch boundary:
        # the head ends inside batch 0 ... the user data ends inside the last
        nst = 3 * B + 1
        out.append(call(g, ("write", S - 1, (nst - 1) * S + 2 - (S - 1), True, True, 3), nst,
                        "G" * n, "bwrite"))
        out.append(call(g, ("write", 17, B * S + 1 - 17, True, False, 1), B + 1, "P" * n,
                        "bwrite"))
    return out


BATCH_GEOMS = [(4, 6), (8, 12), (16, 20), (5, 7), (10, 13), (3, 31)]


# --- buffers: layout with 4 KiB guards (checked by _encode_sweep.check_outputs)

def layout(sizes, off=0):
    seg, pos = [], 0
    for size in sizes:
        hi = pos + GUARD + 16 + -(-size // 16) * 16 + GUARD
        seg.append((pos, pos + GUARD + off, size, hi))
        pos = hi
    return SimpleNamespace(total=pos, seg=seg)


# --- data and expected values ------------------------------------------------

class Built:
    """The random inputs and oracle values of a geometry, per series, computed
    once at the series' largest count and handed out read-only."""

    def __init__(self, O, g, all_cases):
        self.O, self.g = O, g
        self.k, self.n = g
        self.max = {}
        for c in all_cases:
            self.max[c.series] = max(self.max.get(c.series, 0), c.nst)
        self.memo = {}

    def _ro(self, a):
        for x in (a if isinstance(a, list) else [a]):
            x.setflags(write=False)
        return a

    def _get(self, key, make):
        if key not in self.memo:
            self.memo[key] = self._ro(make())
        return self.memo[key]

    def _raw(self, series, what, nbytes, salt):
        return self._get((series, what), lambda: _rng(
            self.k, self.n, 100 + salt + sum(map(ord, series))).integers(0, 256, nbytes,
                                                                        dtype=np.uint8))

    def data(self, s):
        return self._raw(s, "data", CHUNK * self.k * self.max[s], 0)

    def frag(self, s, b):
        return self._raw(s, ("frag", b), CHUNK * self.max[s], 1 + b)

    def enc(self, s):
        return self._get((s, "enc"), lambda: self.O.encode(self.k, self.n, self.data(s), nthreads=8))

    def dec(self, s, m):
        return self._get((s, "dec", m), lambda: CS.decode(
            self.O, self.k, m, {b: self.frag(s, b) for b in bits(m)}))

    def healed(self, s, m):
        return self._get((s, "heal", m), lambda: self.O.encode(self.k, self.n, self.dec(s, m),
                                                               nthreads=8))

    def mixed(self, s, x):
        def make():
            k = self.k
            out = np.empty(CHUNK * k * x.nst, np.uint8)
            for gi, i in enumerate(x.ids.tolist()):
                a0, a1 = gi * x.group * CHUNK, min(x.nst, (gi + 1) * x.group) * CHUNK
                m = x.masks[min(i, len(x.masks) - 1)]
                out[a0 * k:a1 * k] = CS.decode(self.O, k, m, {b: self.frag(s, b)[a0:a1]
                                                              for b in bits(m)})
            return out
        return self._get((s, "mixed", id(x)), make)

    def write(self, c):
        _, head, size, oh, ot, _ = c.sh

        def make():
            S = CHUNK * self.k
            rng = _rng(self.k, self.n, 500 + head % 97 + size % 89 + c.nst)
            user = rng.integers(0, 256, size, dtype=np.uint8)
            o1 = rng.integers(0, 256, S, dtype=np.uint8) if oh else None
            o2 = rng.integers(0, 256, S, dtype=np.uint8) if ot else None
            merged = self.O.writev_merge(self.k, head, user, o1, o2)
            assert merged.size == c.nst * S
            want = self.O.encode(self.k, self.n, merged)
            return [user, o1 if oh else np.empty(0, np.uint8),
                    o2 if ot else np.empty(0, np.uint8)] + want
        return self._get(("write", c.sh, c.nst), make)

    def io(self, c):
        """(input arrays, expected output arrays) of call c, in place order."""
        k, n, s, nst = self.k, self.n, c.series, c.nst
        kind = c.sh[0]
        if kind == "enc":
            return [self.data(s)[:CHUNK * k * nst]], [f[:CHUNK * nst] for f in self.enc(s)]
        if kind == "rows":
            return [self.data(s)[:CHUNK * k * nst]], [self.enc(s)[b][:CHUNK * nst]
                                                     for b in bits(c.sh[1])]
        if kind == "dec":
            return ([self.frag(s, b)[:CHUNK * nst] for b in bits(c.sh[1])],
                    [self.dec(s, c.sh[1])[:CHUNK * k * nst]])
        if kind == "heal":
            return ([self.frag(s, b)[:CHUNK * nst] for b in bits(c.sh[1])],
                    [self.healed(s, c.sh[1])[b][:CHUNK * nst] for b in bits(c.sh[2])])
        if kind == "mixed":
            return [self.frag(s, b)[:CHUNK * nst] for b in range(n)], [self.mixed(s, c.sh[1])]
        return [], self.write(c)[3:]


@functools.lru_cache(maxsize=2)
def built(g, which="default"):
    """Built of a geometry: shared, read-only, the last two kept."""
    import oracle as O
    O.lib()
    return Built(O, g, cases(g) if which == "default" else batch_cases(g))


def mixed_masks(x):
    """The mask of every group, as ec_method_decode_mixed takes them."""
    return [x.masks[min(i, len(x.masks) - 1)] for i in x.ids.tolist()]


# --- what a later edit (or a change of seed) must not lose -------------------

def _check_table():
    single, mixed, single0, mixed0 = {}, {}, {}, {}
    for g in GEOMS:
        k, n = g
        C = cases(g)
        small = [c for c in C if c.series == "small"]
        shapes = {c.sh for c in small}
        for sh in shapes:                                               # H2
            a, b = npos(g, sh)
            for kind in "PGMR":
                assert {c.nst for c in small if c.sh == sh and c.place == kind * (a + b)} == \
                    set(COUNTS), (g, sh, kind)
        for kind in ("enc", "rows", "dec", "heal"):                     # H3
            for sh in [s for s in shapes if s[0] == kind]:
                a, b = npos(g, sh)
                places = {c.place for c in small if c.sh == sh}
                assert set(_mixes(a, b)) <= places, (g, sh)
        heal = {len(bits(sh[2])) for sh in shapes if sh[0] == "heal"}    # H4
        assert {1, min(2, n - k), n - k} <= heal, g
        rows = {len(bits(sh[1])) for sh in shapes if sh[0] == "rows"}
        assert {1, n} <= rows, g
        assert all(len(bits(sh[1])) == k for sh in shapes if sh[0] == "dec"), g
        for c in C:
            assert len(c.place) == sum(npos(g, c.sh)), call_id(c)
            for zc, s1, m1 in ((True, single, mixed), (False, single0, mixed0)):
                for br in kernels_of(c, zcdb=zc):
                    K = CS.bucket(k)
                    (m1 if c.sh[0] == "mixed" else s1).setdefault((br, K), c)
    assert {k for k, _ in GEOMS} == set(range(1, 17))                   # H1
    assert all({k + 2, 31} <= {n for kk, n in GEOMS if kk == k} for k in range(1, 17))
    assert TILE_ENCODER <= set(GEOMS)
    # H5
    want = {("A", 4), ("B", 8), ("C", 16), ("D", 16), ("E", 4), ("E", 8), ("E", 16),
            ("F", 4), ("F", 8), ("F", 16)}
    assert want <= set(single), want - set(single)
    # (a mixed call has rows = k, so for k <= 8 it always fits A / B by
    # default: E's MIXED instantiations of K = 4 and 8 run with ZCDB=0 only)
    assert want - {("E", 4), ("E", 8)} <= set(mixed), want - set(mixed)
    assert {("E", 4), ("E", 8), ("E", 16)} <= set(single0) and \
        {("E", 4), ("E", 8), ("E", 16)} <= set(mixed0)
    assert {"vander", "vander_zc"} <= {b for b, _ in single}

    def kern(g, kind, nst, rows=None):
        return [kernels_of(c) for c in cases(g) if c.sh[0] == kind and c.nst == nst and
                (rows is None or shape_rows(g, c.sh) == rows)]

    # H6
    assert {"E"} in kern((8, 20), "enc", 13) and lds_e(8, 20) > 64 << 10
    assert {"E"} in kern((4, 26), "enc", 13) and lds_e(4, 26) > 64 << 10
    assert {"E"} in kern((1, 31), "enc", 13) and lds_e(1, 31) == 128 << 10
    assert {"C"} in kern((9, 21), "enc", 13) and {"E"} in kern((9, 22), "enc", 13)
    assert {"C"} in kern((16, 20), "heal", 13, 1) and {"C"} in kern((16, 20), "heal", 13, 4)
    assert {"C"} in kern((16, 24), "heal", 13, 7) and {"E"} in kern((16, 24), "heal", 13, 8)
    assert kern((16, 31), "enc", 2053) == [{"D"}] and 2 * 16 + 31 == 63
    assert {"F"} in kern((16, 31), "enc", 41) and {"F"} in kern((12, 31), "enc", 13)
    # H7
    for k in range(9, 17):
        ds = [c for g in GEOMS if g[0] == k for c in cases(g) if c.series == "d"]
        assert {c.nst for c in ds} == set(D_COUNTS), k
        assert all(kernels_of(c) == ({"D"} if c.nst >= 2048 else
                                     {branch(k, shape_rows(c.g, c.sh), c.nst)} - {"D"})
                   for c in ds), k
    assert {"D"} in [kernels_of(c) for c in cases((16, 20)) if c.series == "dmixed"]
    # H8
    for g, T in THRESHOLD.items():
        assert [kernels_of(c) for c in cases(g) if c.series == "thr"] == \
            [{"vander"}, {"vander"}, {"vander_zc"}, {"vander_zc"}], g
    assert [kernels_of(c) for c in cases((16, 20)) if c.series == "thr"] == \
        [{"D"}, {"vander_zc"}, {"vander_zc"}]
    assert {"vander"} in kern((16, 20), "enc", 41)
    assert [kernels_of(c) for c in cases((16, 20)) if c.series == "d" and c.sh[0] == "dec"]
    # H9
    for g in GEOMS:
        mx = [c.sh[1] for c in cases(g) if c.series == "mixed"]
        assert {x.group for x in mx} >= {1, 2, 4, 8, 16, 64}, g
        assert all((x.group == 1 or x.nst % x.group) and x.ids[-1] == 0 for x in mx), g
    for k in CS.EDGE_K:
        edge = [c for c in cases((k, 31)) if c.series == "mixed" and len(c.sh[1].masks) > 5]
        assert {len(set(c.sh[1].masks)) for c in edge} == {CS.fit(k), CS.fit(k) + 1}, k
        assert {frozenset(kernels_of(c)) for c in edge if len(c.sh[1].masks) > CS.fit(k)} == \
            {frozenset("F")}, k
        assert all(kernels_of(c) != {"F"} for c in edge if len(c.sh[1].masks) == CS.fit(k)), k
    # H10
    for c in [c for c in cases((4, 6)) if c.series == "cut"]:
        assert len(launches_of(c)) == CUT_COUNTS[c.nst], call_id(c)
    # H11
    for g in WRITE_GEOMS:
        S = CHUNK * g[0]
        W = [c for c in cases(g) if c.series == "write"]
        assert {c.nst for c in W} == {1, 2, 3, 9}, g
        assert {c.sh[1] for c in W} == {0, 1, 17, S - 1}, g
        assert {(c.sh[1] + c.sh[2]) % S for c in W} == {0, 1, S - 1}, g
        assert {c.sh[5] for c in W} == {1, 3}, g
    # H12
    for g in BATCH_GEOMS:
        k, n = g
        C = batch_cases(g)
        for kind in ("enc", "rows", "dec", "heal"):
            st = [c for c in C if c.sh[0] == kind and "G" in c.place]
            B = (1 << 20) // (k * CHUNK)
            L = [launches_of(c, 1) for c in st]
            assert {len(x) for x in L} == {1, 2, 3, 5}, (g, kind)
            assert {x[-1] for x in L} >= {1, B - 1, B}, (g, kind)
            assert all(c.nst * k * CHUNK <= 8 << 20 for c in st), (g, kind)
        for kind in ("enc", "dec"):
            mp = [launches_of(c, 1) for c in C if c.sh[0] == kind and c.place.strip("P") == ""]
            B = (8 << 20) // (k * CHUNK)
            assert [B - 1] in mp and [B] in mp and [B, 1] in mp, (g, kind)
        for c in [c for c in C if c.series == "bmixed" and "G" in c.place]:
            x, L = c.sh[1], launches_of(c, 1)
            assert len(L) >= 2 and L[0] % x.group == 0 and L[-1] % x.group == 5, call_id(c)
        if g == (16, 20):
            assert all(max(launches_of(c, 1)) < 2048 and kernels_of(c, batch_mb=1) == {"vander"}
                       for c in C if c.sh[0] == "enc" and "G" in c.place)
        for c in [c for c in C if c.series == "bwrite"]:
            assert len(launches_of(c, 1)) >= 2, call_id(c)
    assert any(len(launches_of(c, 1)) == 5 for c in batch_cases((4, 6)))


_check_table()
