"""The programs the run-time compiled kernels execute (emit_program in
glusterfs_amd/csrc/ec_jit.hip) are the matrix product, checked without a
device and without the GPU compiler.

For every matrix below, the text of prog0 and prog1 is cut out of
ec_method_jit_source -- exactly the text the kernel compiler reads -- and
compiled with the host C compiler behind a shim: LDW(off) reads a host copy
of the tile's LDS image, xr3(a, b, c) is a ^ b ^ c, the scheduling barrier is
a no-op, __device__ and __forceinline__ are empty, and the one
`asm volatile("" : "+v"(col));` line (an optimisation barrier, no
computation) is removed.  The program's own statements run; nothing is
re-derived from the coefficients.  The LDS image is built as the kernel body
stages it (input p, plane b, stripe s at ((p * 8 + b) * T + s) * 64, T from
the source's #define), the programs run for every column
col = s * 64 + cc * 4, and acc[o] is placed as the body places it: stripe s,
row rb + o / 8, plane o % 8, dword cc, with rb = 0 for prog0 and R0 for prog1
(only the first nr * 8 entries of each, as the body's store loop).

Two references, every comparison bit-exact:
  * for arbitrary matrices, a plain GF(2^8) product on the bit-plane layout
    (DESIGN 2): bit b of an output symbol is the XOR of the input bits j for
    which bit b of c * x^j is set, with this file's own shift-and-reduce
    multiply (modulus 0x11D), as a 0/1 matrix product modulo 2;
  * for real inverses, oracle.decode on one tile of random fragments, and
    oracle.encode for the 12 parity rows of 16+12.

Matrices: dense random ones for every (k, rows) split the body treats
differently (k = 1 and 2, odd rows, rows < k, rows > k), half-zero, all-zero
rows in each half (they must come out as zeros), an all-zero column, the
identity, all ones, and a set of 16 x 16 matrices in which every constant
1..255 is the first non-zero term of some row and a later term of some row
(asserted below)."""
import ctypes
import itertools
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ASM_LINE = '    asm volatile("" : "+v"(col));\n'
PROG_RE = re.compile(r"__device__ __forceinline__ void prog([01])\(u32 col, u32 \*acc\)\n\{\n"
                     r".*?\n\}\n", re.S)
SHARDS = 8
POISON = 0xEEEEEEEE

SHIM = r"""
#include <stdint.h>
typedef uint32_t u32;
static const unsigned char *lds_base;
#define LDW(off) (*(const u32 *)(lds_base + (off)))
#define __device__ static
#define __forceinline__
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
static u32 xr3(u32 a, u32 b, u32 c) { return a ^ b ^ c; }
"""

# accs[((s * 16 + cc) * na) + o] = acc[o] of program `fn` at column s * 64 + cc * 4
DRIVER = r"""
typedef void (*prog_t)(u32, u32 *);
static const prog_t progs[] = { %s };
int run(u32 fn, const unsigned char *lds, u32 T, u32 na, u32 *accs)
{
    if (fn >= sizeof progs / sizeof progs[0])
        return -1;
    lds_base = lds;
    for (u32 s = 0; s < T; ++s)
        for (u32 cc = 0; cc < 16; ++cc) {
            u32 *acc = accs + (s * 16 + cc) * na;
            for (u32 o = 0; o < na; ++o)
                acc[o] = 0xEEEEEEEEu;
            progs[fn](s * 64 + cc * 4, acc);
        }
    return 0;
}
"""


# ------------------------------------------------------------- references

def gf_mul(a, b):
    """Shift-and-reduce product in GF(2^8), modulus x^8 + x^4 + x^3 + x^2 + 1."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
        b >>= 1
    return r


def bit_matrix(coef):
    """The (rows * 8) x (k * 8) GF(2) matrix of a rows x k GF(2^8) matrix:
    entry (r * 8 + b, p * 8 + j) is bit b of coef[r, p] * x^j."""
    rows, k = coef.shape
    m = np.zeros((rows * 8, k * 8), np.int64)
    for r in range(rows):
        for p in range(k):
            c = int(coef[r, p])
            for j in range(8):
                v = gf_mul(c, 1 << j)
                for b in range(8):
                    m[r * 8 + b, p * 8 + j] = (v >> b) & 1
    return m


def product_tile(coef, planes):
    """planes: uint8 [k, 8, T, 64] (input p, plane b, stripe s) -> the output
    tile uint8 [T, rows, 8, 64] (stripe s, row r, plane b)."""
    k, _, T, _ = planes.shape
    rows = coef.shape[0]
    bits = np.unpackbits(planes.reshape(k * 8, T * 64), axis=1, bitorder="little").astype(np.int64)
    out = ((bit_matrix(coef) @ bits) & 1).astype(np.uint8)
    out = np.packbits(out, axis=1, bitorder="little").reshape(rows, 8, T, 64)
    return np.ascontiguousarray(out.transpose(2, 0, 1, 3))


# --------------------------------------------------------------- matrices

def _constant_matrices():
    """16 matrices of 16 x 16: row r of matrix m starts (after zeros) with
    the constant 16 * m + r + 1 in column (r + m) % 16; the columns behind
    it cycle through 1..255."""
    out, nxt = [], 0
    for m in range(16):
        a = np.zeros((16, 16), np.uint8)
        for r in range(16):
            c = 16 * m + r + 1
            j = (r + m) % 16
            if c > 255:
                c, j = 1 + (r * 37) % 255, 0
            a[r, j] = c
            for jj in range(j + 1, 16):
                a[r, jj] = 1 + nxt % 255
                nxt += 1
        out.append(a)
    return out


def _first_later(mats):
    first, later = set(), set()
    for a in mats:
        for row in a:
            nz = [int(c) for c in row if c]
            if nz:
                first.add(nz[0])
                later.update(nz[1:])
    return first, later


DENSE = [(1, 2), (2, 3), (12, 12), (13, 13), (15, 15), (16, 13), (16, 15), (12, 16), (16, 16)]


def _generic_matrices():
    """name -> rows x k uint8 matrix: the arbitrary (non-inverse) matrices."""
    rng = np.random.default_rng(0x11D)
    mats = {}
    for k, rows in DENSE:
        mats["dense_k%d_r%d" % (k, rows)] = rng.integers(1, 256, (rows, k), dtype=np.uint8)
    half = rng.integers(1, 256, (16, 16), dtype=np.uint8)
    half[rng.random((16, 16)) < 0.5] = 0
    mats["half_zero"] = half
    zr = rng.integers(1, 256, (16, 16), dtype=np.uint8)
    zr[3] = 0              # in prog0's half (rows 0..7)
    zr[11] = 0             # in prog1's half
    mats["zero_rows"] = zr
    zr15 = rng.integers(1, 256, (15, 16), dtype=np.uint8)
    zr15[0] = 0
    zr15[14] = 0           # the last row of the shorter half (R0 = 8, 7 rows)
    mats["zero_rows_15"] = zr15
    zc = rng.integers(1, 256, (16, 16), dtype=np.uint8)
    zc[:, 5] = 0
    mats["zero_column"] = zc
    zc0 = rng.integers(1, 256, (16, 16), dtype=np.uint8)
    zc0[:, 0] = 0          # the first term of every row is not input 0's
    mats["zero_first_column"] = zc0
    mats["identity"] = np.eye(16, dtype=np.uint8)
    mats["ones"] = np.ones((16, 16), np.uint8)
    for i, a in enumerate(_constant_matrices()):
        mats["const_%02d" % i] = a
    return mats


def _inverse_cases(oracle):
    """name -> (k, rows list): sampled masks of 16+4 (30) and 12+4 (10)."""
    rng = np.random.default_rng(164)
    cases = {}
    for k, n, count in ((16, 20, 30), (12, 16, 10)):
        allm = list(itertools.combinations(range(1, n + 1), k))
        picks = [allm[0], allm[-1]] + [allm[1 + i] for i in rng.choice(len(allm) - 2, count - 2,
                                                                      replace=False)]
        for rows in picks:
            cases["inv_%d+%d_%05x" % (k, n - k, sum(1 << (r - 1) for r in rows))] = \
                (k, [int(r) for r in rows])
    assert len(cases) == 40
    return cases


# ---------------------------------------------------------- host programs

class Program:
    def __init__(self, name, coef, text):
        self.name, self.coef, self.text = name, coef, text
        self.rows, self.k = coef.shape
        d = dict((m.group(1), int(m.group(2)))
                 for m in re.finditer(r"^#define (K|ROWS|R0|NA|T) (\d+)u$", text, re.M))
        assert d["K"] == self.k and d["ROWS"] == self.rows, (name, d)
        assert d["R0"] == (self.rows + 1) // 2 and d["NA"] == d["R0"] * 8, (name, d)
        self.T, self.R0, self.NA = d["T"], d["R0"], d["NA"]
        progs = dict((int(m.group(1)), m.group(0)) for m in PROG_RE.finditer(text))
        assert sorted(progs) == [0, 1], name
        self.progs = [progs[0], progs[1]]
        self.lib = self.fn = None

    def host_text(self, idx):
        """prog0 / prog1 as host functions m<idx>_prog0 / m<idx>_prog1."""
        out = []
        for w, p in enumerate(self.progs):
            assert p.count(ASM_LINE) == 1 and "asm" not in p.replace(ASM_LINE, ""), self.name
            p = p.replace(ASM_LINE, "")
            head = "void prog%d(" % w
            assert p.count(head) == 1
            out.append(p.replace(head, "void m%d_prog%d(" % (idx, w)))
        return "".join(out)

    def ops_in_text(self):
        """XOR and xr3 statements of both programs."""
        n = 0
        for p in self.progs:
            for line in p.splitlines():
                x = line.count(" ^ ") + line.count(" ^= ") + line.count("xr3(")
                assert x <= 1, line
                n += x
        return n

    def lds_image(self, planes):
        """planes uint8 [k, 8, T, 64] -> the tile as the body stages it: input
        p, plane b, stripe s at ((p * 8 + b) * T + s) * 64."""
        assert planes.shape == (self.k, 8, self.T, 64)
        img = np.zeros(self.k * 8 * self.T * 64, np.uint8)
        for p in range(self.k):
            for b in range(8):
                for s in range(self.T):
                    at = ((p * 8 + b) * self.T + s) * 64
                    img[at:at + 64] = planes[p, b, s]
        return img

    def run(self, planes):
        """Both programs over every column of the tile; the output tile
        uint8 [T, rows, 8, 64] as the body lays it out (stripe s, row r at
        (s * ROWS + r) * 512, plane b at + b * 64, dword cc at + cc * 4)."""
        img = self.lds_image(planes)
        tile = np.full((self.T, self.rows, 8, 16), 0xA5A5A5A5, np.uint32)
        for half in (0, 1):
            accs = np.zeros((self.T, 16, self.NA), np.uint32)
            rc = self.lib.run(self.fn + half, img.ctypes.data, self.T, self.NA, accs.ctypes.data)
            assert rc == 0
            rb = 0 if half == 0 else self.R0
            nr = self.R0 if half == 0 else self.rows - self.R0
            for o in range(self.NA):
                if o < nr * 8:
                    tile[:, rb + o // 8, o % 8, :] = accs[:, :, o]
        return tile.view(np.uint8).reshape(self.T, self.rows, 8, 64)


def _compile_shard(path, progs, first_idx):
    names = []
    src = [SHIM]
    for i, p in enumerate(progs):
        src.append(p.host_text(first_idx + i))
        names += ["m%d_prog0" % (first_idx + i), "m%d_prog1" % (first_idx + i)]
    src.append(DRIVER % ", ".join(names))
    with open(path + ".c", "w") as f:
        f.write("".join(src))
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11", "-O0", "-w", "-shared", "-fPIC",
                    path + ".c", "-o", path + ".so"], check=True)
    lib = ctypes.CDLL(path + ".so")
    lib.run.restype = ctypes.c_int
    lib.run.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                        ctypes.c_void_p]
    for i, p in enumerate(progs):
        p.lib, p.fn = lib, 2 * i
    return lib


@pytest.fixture(scope="module")
def programs(oracle, tmp_path_factory):
    """name -> Program, for every matrix of this file: the sources generated
    once and compiled for the host as a few shared objects side by side."""
    import glusterfs_amd as g
    mats = dict(_generic_matrices())
    for name, (k, rows) in _inverse_cases(oracle).items():
        mats[name] = oracle.inverse_matrix(rows).astype(np.uint8)
    mats["parity_16+12"] = oracle.encode_matrix(16, 28)[16:28].astype(np.uint8)
    progs = [Program(name, a, g.jit_source(a.shape[1], a.shape[0], a)) for name, a in mats.items()]
    d = str(tmp_path_factory.mktemp("jitprog"))
    shards = [progs[i::SHARDS] for i in range(SHARDS)]
    with ThreadPoolExecutor(SHARDS) as ex:
        list(ex.map(lambda a: _compile_shard(os.path.join(d, "shard%d" % a[0]), a[1], 1000 * a[0]),
                    enumerate(shards)))
    return {p.name: p for p in progs}


def _planes(seed, k, T):
    return np.random.default_rng(seed).integers(0, 256, (k, 8, T, 64), dtype=np.uint8)


# ------------------------------------------------------------------ tests

def test_source_hook_geometry_and_length():
    """jit_source: -EINVAL exactly where jit_compile_check rejects; the C
    entry returns the bytes needed and truncates with a terminator."""
    import glusterfs_amd as g
    for k, rows in ((17, 16), (16, 1), (0, 4), (16, 17)):
        with pytest.raises(ValueError):
            g.jit_source(k, rows, np.ones(max(1, k * rows), np.uint8)[:k * rows])
    lib = g.ec_method.lib
    coef = np.arange(1, 7, dtype=np.uint8)
    assert lib.ec_method_jit_source(2, 3, None, None, 0) == -22
    need = lib.ec_method_jit_source(2, 3, coef.ctypes.data, None, 0)
    text = g.jit_source(2, 3, coef)
    assert need == len(text.encode()) + 1
    buf = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.ec_method_jit_source(2, 3, coef.ctypes.data, buf, 32) == need
    assert buf.raw[:32] == text.encode()[:31] + b"\0" and buf.raw[32:] == b"\xff" * 32
    assert "#define K 2u" in text and "#define ROWS 3u" in text
    assert text == g.jit_source(2, 3, coef.reshape(3, 2))


def test_source_is_the_text_the_compiler_gets(tmp_path):
    """The text checked here is the text that is compiled: the source
    ec_method_jit_compile_check writes out (EC_MI355X_JIT_DUMP) for a matrix
    equals jit_source of that matrix."""
    import glusterfs_amd as g
    coef = np.random.default_rng(5).integers(0, 256, (13, 12), dtype=np.uint8)
    prefix = str(tmp_path / "dump")
    os.environ["EC_MI355X_JIT_DUMP"] = prefix
    try:
        size, _ = g.jit_compile_check(12, 13, coef)
    finally:
        del os.environ["EC_MI355X_JIT_DUMP"]
    if size == -38:
        pytest.skip("no kernel compiler in this image")
    assert size > 0, size
    assert open(prefix + ".hip").read() == g.jit_source(12, 13, coef)


@pytest.mark.parametrize("name", sorted(n for n in _generic_matrices() if not n.startswith("const_")))
def test_program_is_the_gf_product(programs, name):
    p = programs[name]
    planes = _planes(len(name) * 131 + p.k, p.k, p.T)
    got = p.run(planes)
    want = product_tile(p.coef, planes)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
    if name.startswith("zero_rows"):
        zero = [r for r in range(p.rows) if not p.coef[r].any()]
        assert len(zero) == 2 and zero[0] < p.R0 <= zero[1]
        assert not got[:, zero].any()
    if name == "identity":
        assert np.array_equal(got, planes.transpose(2, 0, 1, 3))


def test_every_constant_first_and_later_terms(programs):
    """All 255 constants through the `a = ...` statements of a row's first
    non-zero term and through the `^=` / xr3 statements of its later terms."""
    mats = _constant_matrices()
    first, later = _first_later(mats)
    assert len(first) == 255 and len(later) == 255, (len(first), len(later))
    for i, a in enumerate(mats):
        p = programs["const_%02d" % i]
        assert np.array_equal(p.coef, a)
        planes = _planes(700 + i, 16, p.T)
        got = p.run(planes)
        want = product_tile(a, planes)
        assert np.array_equal(got, want), (i, np.argwhere(got != want)[:4].tolist())


def test_real_inverses_match_oracle_decode(programs, oracle):
    """30 masks of 16+4 and 10 of 12+4: the programs of the inverse decode one
    tile of random (non-codeword) fragments as oracle.decode does."""
    cases = _inverse_cases(oracle)
    assert sum(k == 16 for k, _ in cases.values()) >= 30
    assert sum(k == 12 for k, _ in cases.values()) >= 10
    for i, (name, (k, rows)) in enumerate(cases.items()):
        p = programs[name]
        rng = np.random.default_rng(9000 + i)
        frags = [rng.integers(0, 256, 512 * p.T, dtype=np.uint8) for _ in range(k)]
        # fragment p: stripe s at s * 512, plane b at + b * 64
        planes = np.stack([f.reshape(p.T, 8, 64).transpose(1, 0, 2) for f in frags])
        got = p.run(planes)
        want = oracle.decode(k, rows, frags)           # stripe-major: (s * k + r) * 512
        assert np.array_equal(got.reshape(-1), want), (name, rows)


def test_parity_rows_match_oracle_encode(programs, oracle):
    """The 12 parity rows of 16+12 over one tile of random data."""
    p = programs["parity_16+12"]
    data = np.random.default_rng(1612).integers(0, 256, 512 * 16 * p.T, dtype=np.uint8)
    want = oracle.encode(16, 28, data)
    planes = np.ascontiguousarray(data.reshape(p.T, 16, 8, 64).transpose(1, 2, 0, 3))
    got = p.run(planes)
    for r in range(12):
        assert np.array_equal(got[:, r].reshape(-1), want[16 + r]), r


def test_reported_ops_equal_the_statements_in_the_text(programs):
    """The XOR instructions per column that jit_compile_check reports (the
    figure DESIGN quotes) are the XOR and xr3 statements of the text."""
    import glusterfs_amd as g
    first = next(iter(programs.values()))
    if g.jit_compile_check(first.k, first.rows, first.coef)[0] == -38:
        pytest.skip("no kernel compiler in this image")
    with ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as ex:
        res = list(ex.map(lambda p: g.jit_compile_check(p.k, p.rows, p.coef),
                          programs.values()))
    for p, (size, ops) in zip(programs.values(), res):
        assert size > 0, (p.name, size)
        assert ops == p.ops_in_text(), (p.name, ops, p.ops_in_text())
