"""GPU parity of the run-time compiled whole-matrix kernels (r06,
glusterfs_amd/csrc/ec_jit.hip): a single-pattern device combine of a wide
code (k >= 12, >= 12 output rows) runs a kernel compiled for its coefficient
matrix once the code exists.  Every result is compared with the oracle:

  * 16+4 decodes of device fragments for the contiguous masks and scattered
    ones, tile-aligned and ragged stripe counts, fragments at an odd byte
    address (LDS-DMA reads them in place), with EC_MI355X_JIT_SYNC=1 so the
    first call compiles and every call runs the compiled kernel;
  * 12+4 decodes (12 rows: programs of 6 rows per wave) and a 16+12
    row-masked encode of 12 rows (fragment-major outputs, 512-byte runs);
  * 1 GiB calls (non-temporal staging), five per mask, as round trips;
  * the default asynchronous mode: the first call of a matrix runs the
    shipped kernel while a library thread compiles, later calls the
    compiled one -- exact both ways;
  * a process exiting while its matrix compiles exits cleanly;
  * EC_MI355X_JIT=0: never compiled, never launched;
  * the kernel body's edges, with EC_MI355X_JIT_MIN_STRIPES=1 so that counts
    below one 4-stripe tile reach the compiled kernel: 1, 2, 3, 4, 5 and 9
    stripes through both store forms (a decode's contiguous run, and the
    512-byte row runs of a 16 -> 13 heal and a 12-row encode), outputs
    pre-filled and followed by a guard stripe that must stay untouched; the
    same through the non-temporal entry (EC_MI355X_LDSNT=1); odd row counts
    (13+3 and 15+2 decodes, 13 and 15 rows of 16 inputs) and more rows than
    inputs (16 rows of 12+16); every fragment at its own byte offset; an
    output that is only 8-byte aligned (ineligible: the shipped kernel codes
    it, launches unchanged); four threads meeting one matrix for the first
    time; a caller's stream.  Every case asserts the exact jit_stats deltas,
    so a silent fall-back to the shipped kernel cannot pass for the compiled
    one.  (The programs themselves are checked on the CPU for many more
    matrices, tests/test_jit_program.py.)
Each case runs in its own process through the C ABI (the settings are read
once per process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = r"""
import itertools, sys, time
sys.path.insert(0, "oracle")
import numpy as np, torch
import glusterfs_amd as g
import oracle as O           # the checker

rng = np.random.default_rng(11)
def rb(n):
    return rng.integers(0, 256, n, dtype=np.uint8)
def dev(a, off=0):
    if off == 0:
        return torch.from_numpy(a).cuda()
    t = torch.empty(a.size + off, dtype=torch.uint8, device="cuda")
    t[off:] = torch.from_numpy(a).cuda()
    return t[off:]

def decode_check(L, k, n, nst, mask, off=0):
    frags = [rb(512 * nst) for _ in range(n)]
    rows = O.mask_rows(mask)
    out = torch.empty(512 * k * nst, dtype=torch.uint8, device="cuda")
    out.fill_(0xA5)
    L.decode_batch(nst, mask, rows, [dev(frags[r - 1], off) for r in rows], out)
    exp = O.decode(k, rows, [frags[r - 1] for r in rows])
    assert np.array_equal(out.cpu().numpy(), exp), ("dec", k, n, nst, hex(mask), off)
"""

SYNC = COMMON + r"""
s0 = g.jit_stats()
with g.ECMatrixList(16, 20) as L:
    allm = [sum(1 << b for b in c) for c in itertools.combinations(range(20), 16)]
    masks = [0xFFFF0, 0x0FFFF, 0xF0FFF] + [allm[i] for i in rng.choice(len(allm), 3, replace=False)]
    for m in masks:
        for nst in (1024, 4099):
            decode_check(L, 16, 20, nst, m)
    decode_check(L, 16, 20, 2051, masks[3], off=3)
    decode_check(L, 16, 20, 1000, masks[0])          # below the threshold: shipped kernel
with g.ECMatrixList(12, 16) as L:
    decode_check(L, 12, 16, 1030, 0xFFF0)
    decode_check(L, 12, 16, 1030, 0x7BDE)
# a row-masked encode of 12 rows of a 16+12 volume: fragment-major outputs
with g.ECMatrixList(16, 28) as L:
    nst = 1027
    data = rb(512 * 16 * nst)
    want = O.encode(16, 28, data)
    rm = sum(1 << i for i in range(16, 28))
    outs = [torch.empty(512 * nst, dtype=torch.uint8, device="cuda") if (rm >> i) & 1 else None
            for i in range(28)]
    L.encode_rows_device(0, None, nst, dev(data), rm, outs)
    g.sync_device(0)
    for i in range(16, 28):
        assert np.array_equal(outs[i].cpu().numpy(), want[i]), ("rows", i)
s1 = g.jit_stats()
d = {k: s1[k] - s0[k] for k in s1}
print("JIT", d)
assert d["failed"] == 0, d
assert d["compiled"] >= len(masks) + 3, d
# every eligible call ran a compiled kernel (sync mode): 6 masks x 2 sizes,
# the odd-offset call, two 12+4 decodes and the 12-row encode
assert d["launches"] >= 2 * len(masks) + 1 + 2 + 1, d
print("ok")
"""

ASYNC = COMMON + r"""
with g.ECMatrixList(16, 20) as L:
    decode_check(L, 16, 20, 2048, 0xFFFF0)          # first sight: queued, shipped kernel
    s = g.jit_stats()
    assert s["launches"] == 0, s
    t0 = time.time()
    while g.jit_stats()["compiled"] + g.jit_stats()["failed"] < 1 and time.time() - t0 < 60:
        time.sleep(0.05)
    s = g.jit_stats()
    assert s["compiled"] == 1 and s["failed"] == 0, s
    for _ in range(3):
        decode_check(L, 16, 20, 2048, 0xFFFF0)
    s = g.jit_stats()
    assert s["launches"] == 3, s
print("ok", s)
"""

# 1 GiB of user data per call (the size the bench decodes, non-temporal
# staging): the round trip data -> shipped encode -> compiled decode == data,
# five calls per mask (a tile read before every wave's staging landed shows
# as a mismatch somewhere in 131,072 stripes)
FULL = COMMON + r"""
k, n = 16, 20
nst = (1 << 30) // (512 * k)
data = torch.randint(0, 256, (512 * k * nst,), dtype=torch.uint8, device="cuda")
frags = [torch.empty(512 * nst, dtype=torch.uint8, device="cuda") for _ in range(n)]
out = torch.empty_like(data)
with g.ECMatrixList(k, n) as L:
    L.encode_batch(nst, data, frags)
    for m in (0xFFFF0, 0xF0FFF, 0x5FFF5):
        rows = O.mask_rows(m)
        for _ in range(5):
            out.fill_(0)
            L.decode_batch(nst, m, rows, [frags[r - 1] for r in rows], out)
            assert torch.equal(out, data), hex(m)
s = g.jit_stats()
assert s["launches"] >= 15 and s["failed"] == 0, s
print("ok", s)
"""

# a process that exits while its matrix is still being compiled: the compile
# runs in a child process (ec_jitc), and the library thread that waits for it
# is neither stopped nor joined at exit, so the exit tears nothing down under
# a compile (the child finishes on its own or is orphaned)
EXIT = COMMON + r"""
with g.ECMatrixList(16, 20) as L:
    decode_check(L, 16, 20, 2048, 0xFFFF0)
print("ok", g.jit_stats())
"""

OFF = COMMON + r"""
with g.ECMatrixList(16, 20) as L:
    for _ in range(2):
        decode_check(L, 16, 20, 2048, 0xFFFF0)
s = g.jit_stats()
assert s["compiled"] == 0 and s["launches"] == 0 and s["lookups"] == 0, s
print("ok")
"""


# ---- the body's edges (EC_MI355X_JIT_MIN_STRIPES=1, EC_MI355X_JIT_SYNC=1) ----
EDGE_COMMON = COMMON + r"""
GUARD = 0xA5
def guarded(nbytes, guard, off=0):
    # nbytes of output pre-filled with 0xA5, a guard of `guard` bytes behind it
    raw = torch.empty(off + nbytes + guard, dtype=torch.uint8, device="cuda")
    raw.fill_(GUARD)
    return raw[off:]
def guard_ok(t, nbytes, what):
    tail = t[nbytes:].cpu().numpy()
    assert tail.size and (tail == GUARD).all(), ("guard overwritten", what)
def delta(s0):
    s1 = g.jit_stats()
    return {k: s1[k] - s0[k] for k in s1}

def decode_edge(L, k, nst, mask, offs=None, out_off=0, stream=None):
    rows = O.mask_rows(mask)
    frags = [rb(512 * nst) for _ in rows]
    out = guarded(512 * k * nst, 512 * k, out_off)
    assert out.data_ptr() % 16 == out_off
    L.decode_batch(nst, mask, rows, [dev(f, offs[i] if offs else 0) for i, f in enumerate(frags)],
                   out)
    exp = O.decode(k, rows, frags)
    assert np.array_equal(out[:exp.size].cpu().numpy(), exp), ("dec", k, nst, hex(mask))
    guard_ok(out, exp.size, ("dec", k, nst))

def heal_edge(L, k, n, nst, mask, target):
    # the fused heal of non-codeword fragments: encode(decode(good)) rows
    rows = O.mask_rows(mask)
    frags = [rb(512 * nst) for _ in rows]
    tgt = [b for b in range(n) if (target >> b) & 1]
    outs = [guarded(512 * nst, 512) for _ in tgt]
    L.heal_device(0, None, nst, mask, [dev(f) for f in frags], target, outs)
    g.sync_device(0)
    want = O.encode(k, n, O.decode(k, rows, frags))
    for o, b in zip(outs, tgt):
        assert np.array_equal(o[:512 * nst].cpu().numpy(), want[b]), ("heal", nst, b)
        guard_ok(o, 512 * nst, ("heal", nst, b))

def rows_edge(L, k, n, nst, rm):
    data = rb(512 * k * nst)
    want = O.encode(k, n, data)
    outs = [guarded(512 * nst, 512) if (rm >> i) & 1 else None for i in range(n)]
    L.encode_rows_device(0, None, nst, dev(data), rm, outs)
    g.sync_device(0)
    for i in range(n):
        if outs[i] is not None:
            assert np.array_equal(outs[i][:512 * nst].cpu().numpy(), want[i]), ("rows", nst, i)
            guard_ok(outs[i], 512 * nst, ("rows", nst, i))

HEAL_MASK = 0x2AAB5555                         # 16 of the 31 bricks of 16+15
assert bin(HEAL_MASK).count("1") == 16
HEAL_13 = [b for b in range(31) if not (HEAL_MASK >> b) & 1][:13]
HEAL_TARGET = sum(1 << b for b in HEAL_13)
"""

# ns == 1 tiles, counts below one tile, both store forms: three matrices
RAGGED = EDGE_COMMON + r"""
COUNTS = (1, 2, 3, 4, 5, 9)
s0 = g.jit_stats()
with g.ECMatrixList(16, 20) as L:
    for nst in COUNTS:
        decode_edge(L, 16, nst, 0xF3FF3)                 # contiguous run store
with g.ECMatrixList(16, 31) as L:
    for nst in COUNTS:
        heal_edge(L, 16, 31, nst, HEAL_MASK, HEAL_TARGET)  # 13 rows, 512-byte row runs
with g.ECMatrixList(16, 28) as L:
    for nst in COUNTS:
        rows_edge(L, 16, 28, nst, sum(1 << i for i in range(16, 28)))
d = delta(s0)
print("JIT", d)
assert d["failed"] == 0 and d["compiled"] == 3, d
assert d["lookups"] == 3 * len(COUNTS) and d["launches"] == 3 * len(COUNTS), d
print("ok")
"""

# odd row counts (uneven halves), k of 13 and 15, rows > k: five matrices
SHAPES = EDGE_COMMON + r"""
nst = 9
s0 = g.jit_stats()
with g.ECMatrixList(13, 16) as L:
    decode_edge(L, 13, nst, 0xDFF6)                      # k = rows = 13
with g.ECMatrixList(15, 17) as L:
    decode_edge(L, 15, nst, 0x1FDFB)                     # k = rows = 15
with g.ECMatrixList(16, 31) as L:
    heal_edge(L, 16, 31, nst, HEAL_MASK, HEAL_TARGET)    # 16 -> 13
    rows_edge(L, 16, 31, nst, sum(1 << i for i in range(16, 31)))   # 16 -> 15
with g.ECMatrixList(12, 28) as L:
    rows_edge(L, 12, 28, nst, sum(1 << i for i in range(12, 28)))   # 12 -> 16, in_stride 512 * 12
d = delta(s0)
print("JIT", d)
assert d["failed"] == 0 and d["compiled"] == 5 and d["lookups"] == 5 and d["launches"] == 5, d
print("ok")
"""

ALIGN = EDGE_COMMON + r"""
s0 = g.jit_stats()
with g.ECMatrixList(16, 20) as L:
    # every fragment at its own byte offset 1..15: LDS-DMA reads them in place
    for nst in (9, 130):
        decode_edge(L, 16, nst, 0xFFF0F, offs=[1 + i % 15 for i in range(16)])
    d = delta(s0)
    assert d["failed"] == 0 and d["compiled"] == 1 and d["lookups"] == 2 and d["launches"] == 2, d
    # the output 8 bytes past a 16-byte boundary: not eligible (16-byte lane
    # stores), the shipped kernel codes the call
    for nst in (9, 130):
        decode_edge(L, 16, nst, 0xFFF0F, out_off=8)
    d2 = delta(s0)
    assert d2["failed"] == 0 and d2["compiled"] == 1 and d2["lookups"] == 2, d2
    assert d2["launches"] == 2, d2
print("ok", d2)
"""

# four threads meet one matrix for the first time, each on its own
# (per-thread) stream: the first to arrive compiles, the others run the
# shipped kernel until the code exists.  All threads pass a barrier after
# their first call, so the 8 later calls are made after the compile finished
# and must launch the compiled kernel, as must the compiling thread's first.
THREADS = EDGE_COMMON + r"""
import threading
k, nst, mask = 16, 64, 0x7EBFE
rows = O.mask_rows(mask)
frags = [rb(512 * nst) for _ in rows]
dfr = [dev(f) for f in frags]
exp = O.decode(k, rows, frags)
outs = [[guarded(512 * k * nst, 512 * k) for _ in range(3)] for _ in range(4)]
torch.cuda.synchronize()
start, first_done = threading.Barrier(4), threading.Barrier(4)
errors = []
s0 = g.jit_stats()
with g.ECMatrixList(16, 20) as L:
    def worker(t):
        try:
            start.wait()
            for c in range(3):
                L.decode_device(0, None, nst, mask, dfr, outs[t][c])
                g.sync_device(0)
                if c == 0:
                    first_done.wait()
        except Exception as e:
            errors.append(repr(e))
            start.abort()
            first_done.abort()
    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
assert not errors, errors
for t in range(4):
    for c in range(3):
        assert np.array_equal(outs[t][c][:exp.size].cpu().numpy(), exp), ("thread", t, "call", c)
        guard_ok(outs[t][c], exp.size, ("thread", t, c))
d = delta(s0)
print("JIT", d)
assert d["failed"] == 0 and d["compiled"] == 1 and d["lookups"] == 12, d
assert d["launches"] >= 4, d
assert 9 <= d["launches"] <= 12, d
print("ok")
"""

# a caller's stream: the fragments are written on a non-default torch stream
# behind work that keeps it busy, the decode is queued on that stream's
# handle and the result read back on it, with no device-wide synchronisation
# in between; a kernel launched on any other stream would read the zeros the
# fragment buffers held before
STREAM = EDGE_COMMON + r"""
k, nst, mask = 16, 2048, 0xBDFF5
rows = O.mask_rows(mask)
frags = [rb(512 * nst) for _ in rows]
src = [dev(f) for f in frags]
dst = [torch.zeros(512 * nst, dtype=torch.uint8, device="cuda") for _ in rows]
busy = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
exp = O.decode(k, rows, frags)
torch.cuda.synchronize()
s0 = g.jit_stats()
st = torch.cuda.Stream()
with g.ECMatrixList(16, 20) as L:
    L.decode_batch(nst, mask, rows, src, guarded(512 * k * nst, 512 * k))   # compiles the matrix
    with torch.cuda.stream(st):
        out = guarded(512 * k * nst, 512 * k)
        for _ in range(8):
            busy.add_(1)
        for a, b in zip(dst, src):
            a.copy_(b)
        L.decode_device(0, st.cuda_stream, nst, mask, dst, out)
        got = out.cpu().numpy()
assert np.array_equal(got[:exp.size], exp)
assert (got[exp.size:] == GUARD).all()
d = delta(s0)
print("JIT", d)
assert d["failed"] == 0 and d["compiled"] == 1 and d["lookups"] == 2 and d["launches"] == 2, d
print("ok")
"""


def _run(script, **env):
    e = dict(os.environ, EC_MI355X_QUIET="1", EC_GPU_ALWAYS="1")
    e.update(env)
    r = subprocess.run([sys.executable, "-c", script], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_jit_kernels_match_oracle():
    print(_run(SYNC, EC_MI355X_JIT_SYNC="1"))


def test_jit_full_size_round_trip():
    print(_run(FULL, EC_MI355X_JIT_SYNC="1"))


def test_jit_async_first_call_shipped_then_compiled():
    print(_run(ASYNC))


def test_jit_exit_while_compiling():
    print(_run(EXIT))


def test_jit_off():
    _run(OFF, EC_MI355X_JIT="0")


EDGE_ENV = dict(EC_MI355X_JIT_SYNC="1", EC_MI355X_JIT_MIN_STRIPES="1")


def test_jit_ragged_and_sub_tile_counts():
    print(_run(RAGGED, **EDGE_ENV))


def test_jit_non_temporal_entry_small_counts():
    """The same counts through ec_jit_combine_nt (aligned inputs)."""
    print(_run(RAGGED, EC_MI355X_LDSNT="1", **EDGE_ENV))


def test_jit_odd_rows_and_rows_above_k():
    print(_run(SHAPES, **EDGE_ENV))


def test_jit_fragment_offsets_and_ineligible_output():
    print(_run(ALIGN, **EDGE_ENV))


def test_jit_first_sight_from_four_threads():
    print(_run(THREADS, **EDGE_ENV))


def test_jit_callers_stream():
    print(_run(STREAM, **EDGE_ENV))
