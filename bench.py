#!/usr/bin/env python3
"""Benchmark of the MI355X disperse coder (BASELINE.json metric).

One "step" = one pass of the hot path over one batch resident in HBM:
decoding 1 GiB of user data of a disperse 4+2 volume with 2 fragments
missing (mask 0x3C: bricks 0 and 1 lost) -- BASELINE.json configs[1].
With --gpus N (one process per GPU under torch.distributed.run) every rank
decodes its own 1 GiB stripe range of an N GiB job (weak scaling): stripes
are independent, so no collective touches the data path; the only
collectives are the barrier around the timed region, the max over ranks of
the elapsed time and an all-ranks parity flag (glusterfs_amd/dist.py).

A plain run (`--gpus N --steps K --warmup W`) does only what the headline
figure needs: it generates and encodes the input, warms up, times the K
steps, compares the decoded output with the input on the GPU (parity_ok),
writes the output under --dump-outputs if given, and prints the JSON line.
That line carries
  ms_per_step   the wall time of the K timed steps / K, in milliseconds
  roofline      the decode kernel against the 8 TB/s HBM peak: algorithmic
                bytes per launch (2*S: read k fragments = S, write S) over the
                average launch time of the same K steps, measured with HIP
                events on the launch stream; `traffic` = PMC-measured HBM
                bytes per launch from the committed rocprofv3 run
                (profiles/traffic.json)
Everything else is measured only with --full, which adds
  fullsize_sha256_check  the SHA-256 fixture comparison described below
  cpu_baseline  the CPU oracle (oracle/, C restatement of the reference
                algorithm) on the host's usable cores and on one thread:
                BASELINE configs[0] (4+2 encode of 1 GiB) and the bench
                workload (4+2 decode), rank 0 at N=1 only
  extra         (N=1) the other BASELINE configs measured the same way, a
                copy calibration, PCIe-inclusive end-to-end rates and the
                library's own CPU engine; for N > 1 the per-N 16+4 encode /
                self-heal / PCIe lines instead
--extra / --no-extra, --no-cpu and --no-dist-extra narrow a --full run.

--dump-outputs DIR writes what the last timed step decoded (the `out` buffer
a caller of decode_device receives) as float32 / float64 .npy files, see
dump_outputs().  The input is a fixed stream, so two builds run with the same
arguments can be compared file for file.

Input data is the xorshift64 stream of SURVEY.md 8(d), generated on the
GPU (glusterfs_amd/synth.py); rank r of an N-GPU job owns the r-th slice of
one stream.  With --full, full-size results are checked against the SHA-256
fixtures of tests/golden/fullsize_sha256.json (oracle-generated in the
container): input, every encoded fragment, and decode outputs (= the input).
"""
import argparse
import hashlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "EC encode/decode user-data GB/s (4+2, 8+4) at 1/2/4/8 MI355X; % HBM roofline"
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
CHUNK = 512
EXTRA_WARMUP = 20  # untimed launches before each `extra` config (extra_configs)
SUSTAIN_MS = 150.0  # continuous load before the `sustained` headline figure
DUMP_SEED = 20240607       # --dump-outputs: which bytes of a large output are kept
DUMP_SAMPLE = 8 << 20      # ... and how many (float32: 32 MiB)
DUMP_SUMS = 1 << 21        # ... and at most this many stripe-group sums (float64: 16 MiB)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="GPUs (one rank each); without WORLD_SIZE in the environment and "
                         "N > 1 the bench starts the N ranks itself (torch.distributed.run)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="user data per GPU per step")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: the SHA-256 "
                         "fixtures, the other BASELINE configs (`extra`), the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's decoded output to DIR/<name>.npy")
    ap.add_argument("--extra", dest="extra", action="store_true", default=None,
                    help="--full: the `extra` configs also for N > 1")
    ap.add_argument("--no-extra", dest="extra", action="store_false",
                    help="--full: without the `extra` configs")
    ap.add_argument("--no-cpu", action="store_true", help="--full: without the CPU baseline")
    ap.add_argument("--no-dist-extra", action="store_true",
                    help="N > 1: skip the per-N 16+4 encode / self-heal / PCIe lines")
    ap.add_argument("--heal-sweep", default=None, choices=("auto", "gpu", "cpu"),
                    help="child mode of the heal-sweep extra: one engine setting, JSON out")
    ap.add_argument("--warm-ms", type=float, default=0.0,
                    help="--only: keep launching for this long before the timed launches "
                         "(past the first ~10 ms clock transient of a compute-heavy kernel)")
    ap.add_argument("--only", default=None,
                    help="profiling helper: enc:K+R | dec:K+R:MASKHEX | mixed:K+R[:NMASKS[:GROUP]] | heal:K+R | "
                         "rmw:K+R")
    return ap.parse_args()


def gbps(nbytes, seconds):
    return nbytes / seconds / 1e9


def rand_u8(torch, nbytes, seed, device):
    """Random bytes for the configs without a fixture (partial writes)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    x = torch.randint(-2**62, 2**62, (nbytes // 8,), dtype=torch.int64, device=device,
                      generator=g)
    return x.view(torch.uint8)


_FIX = None


def fixture(case, rank):
    """Full-size SHA-256 fixture of `case` for `rank`, or None."""
    global _FIX
    if _FIX is None:
        try:
            with open(os.path.join(ROOT, "tests", "golden", "fullsize_sha256.json")) as f:
                _FIX = json.load(f)["cases"]
        except (OSError, ValueError, KeyError):
            _FIX = {}
    return _FIX.get("%s_r%d" % (case, rank))


def sha_dev(t):
    return hashlib.sha256(memoryview(t.cpu().numpy())).hexdigest()


def timed(torch, fn, steps, warmup, group=None, warm_ms=0.0):
    """Warmup, then exactly `steps` launches between two HIP events on the
    launch stream, bracketed by barrier + synchronize.  warm_ms > 0 (the
    `extra` configs only): keep warming until that much time has passed too,
    so short kernels are timed past the clock transient as long ones are."""
    # one call and a drain before the warm-up clock starts: a first call pays
    # one-time setup (a decode matrix, a run-time compiled kernel of a wide
    # code: ~1-2 s, ec_jit.hip) that must not eat the time-based warm-up
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    pending = []                 # events 8 launches apart: the queue never drains
    while n < warmup or (warm_ms and (time.perf_counter() - t0) * 1e3 < warm_ms):
        fn()
        n += 1
        if warm_ms and n % 8 == 0:
            ev = torch.cuda.Event()
            ev.record()
            pending.append(ev)
            if len(pending) > 2:
                pending.pop(0).synchronize()
    torch.cuda.synchronize()
    if group:
        group.barrier()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if group:
        group.barrier()
    return wall, ev0.elapsed_time(ev1) / 1e3 / steps


class Ctx:
    def __init__(self, g, torch, dev, rank=0, fixtures=True):
        self.g, self.torch, self.dev, self.rank = g, torch, dev, rank
        self.fixtures = fixtures   # compare full-size results with the SHA-256 fixtures
        self.sp = torch.cuda.current_stream(dev).cuda_stream
        self.checks = {}
        self.warm_ms = 0.0     # time-based warm-up (extra / dist configs only)

    def encoded(self, k, n, nbytes, case=None, word0=None):
        """This rank's slice of the xorshift stream (words from `word0`,
        default rank * slice), encoded on the GPU; with a fixture, the input
        and every fragment are checked by SHA-256."""
        from glusterfs_amd import synth
        torch = self.torch
        nst = nbytes // (CHUNK * k)
        user = nst * CHUNK * k
        w0 = self.rank * user // 8 if word0 is None else word0
        data = synth.fill_device(torch, user, self.dev, word0=w0)
        stagger = int(os.environ.get("EC_BENCH_FRAG_STAGGER", "0"))   # A/B: placement
        if stagger:
            # the n fragments as views of one allocation, bases `stagger`
            # bytes off a multiple of the fragment size
            span = nst * CHUNK + stagger
            blob = torch.empty(span * n, dtype=torch.uint8, device=self.dev)
            frags = [blob[i * span:i * span + nst * CHUNK] for i in range(n)]
        else:
            frags = [torch.empty(nst * CHUNK, dtype=torch.uint8, device=self.dev) for _ in range(n)]
        L = self.g.ECMatrixList(k, n)
        L.encode_device(self.dev.index, self.sp, nst, data, frags)
        fx = fixture(case, self.rank) if case and self.fixtures else None
        if fx and fx["bytes"] == user and fx["k"] == k and fx["word0"] == w0:
            torch.cuda.synchronize()
            ok = sha_dev(data) == fx["data"]
            if "frags" in fx:
                ok = ok and all(sha_dev(f) == h for f, h in zip(frags, fx["frags"]))
            self.checks["%s_r%d" % (case, self.rank)] = ok
        return L, data, frags, nst


def sustained(c, fn, steps):
    """The same launches timed again after SUSTAIN_MS of back-to-back load
    (clocks and HBM settle lower under continuous work): the
    figure a self-heal sweep or a long rebuild sees."""
    _, kt = timed(c.torch, fn, max(steps, 10), 1, None, SUSTAIN_MS)
    return kt


def run_decode(c, k, n, nbytes, mask, steps, warmup, case=None, group=None, sus=False):
    L, data, frags, nst = c.encoded(k, n, nbytes, case)
    rows = c.g.mask_rows(mask)
    ins = [frags[r - 1] for r in rows]
    out = c.torch.empty_like(data)
    fn = lambda: L.decode_device(c.dev.index, c.sp, nst, mask, ins, out)  # noqa: E731
    wall, kt = timed(c.torch, fn, steps, warmup, group, c.warm_ms)
    ks = sustained(c, fn, steps) if sus else None
    ok = bool(c.torch.equal(out, data)) and c.checks.get("%s_r%d" % (case, c.rank), True)
    return dict(wall=wall, kernel_s=kt, kernel_s_sus=ks, ok=ok, user=nst * CHUNK * k, nst=nst,
                frags=frags, rows=rows, out=out)


def dump_outputs(torch, dirname, rank, out, stripe):
    """--dump-outputs: the decoded bytes of the last timed step, as a caller
    of decode_device receives them in `out`, written as
      decoded.npy              every byte, float32 -- when there are at most
                               DUMP_SAMPLE of them; otherwise
      decoded_sample.npy       the bytes at DUMP_SAMPLE positions drawn once
                               from numpy's default_rng(DUMP_SEED), ascending,
                               float32, and
      decoded_stripe_sums.npy  the byte sum of every stripe (of groups of G
                               consecutive stripes where there are more than
                               DUMP_SUMS stripes), float64, exact -- so every
                               output byte bears on the dump.
    Ranks above 0 append _rank<r> to the names.  Returns the file names."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    sfx = "_rank%d" % rank if rank else ""
    n = out.numel()
    files = {}
    if n <= DUMP_SAMPLE:
        files["decoded"] = out.cpu().numpy().astype(np.float32)
    else:
        idx = np.sort(np.random.default_rng(DUMP_SEED).integers(0, n, DUMP_SAMPLE, dtype=np.int64))
        pick = out[torch.from_numpy(idx).to(out.device)]
        files["decoded_sample"] = pick.cpu().numpy().astype(np.float32)
        sums = out.view(-1, stripe).sum(dim=1, dtype=torch.int64).cpu().numpy()
        group = -(-len(sums) // DUMP_SUMS)
        if group > 1:
            sums = np.add.reduceat(sums, np.arange(0, len(sums), group))
        files["decoded_stripe_sums"] = sums.astype(np.float64)
    names = []
    for name, a in files.items():
        names.append(name + sfx + ".npy")
        np.save(os.path.join(dirname, names[-1]), a)
    return names


def run_encode(c, k, n, nbytes, steps, warmup, case=None, group=None, sus=False, word0=None):
    torch = c.torch
    L, data, frags, nst = c.encoded(k, n, nbytes, case, word0)
    fn = lambda: L.encode_device(c.dev.index, c.sp, nst, data, frags)  # noqa: E731
    wall, kt = timed(torch, fn, steps, warmup, group, c.warm_ms)
    ks = sustained(c, fn, steps) if sus else None
    fx = fixture(case, c.rank) if case and c.fixtures else None
    if fx and "frags" in fx and fx["bytes"] == nst * CHUNK * k:
        torch.cuda.synchronize()        # the timed launches rewrote the fragments
        ok = all(sha_dev(f) == h for f, h in zip(frags, fx["frags"]))
    else:
        rows = list(range(n - k + 1, n + 1))
        out = torch.empty_like(data)
        L.decode_device(c.dev.index, c.sp, nst, sum(1 << (r - 1) for r in rows),
                        [frags[r - 1] for r in rows], out)
        torch.cuda.synchronize()
        ok = bool(torch.equal(out, data))
    return dict(wall=wall, kernel_s=kt, kernel_s_sus=ks, ok=ok, user=nst * CHUNK * k)


def run_mixed(c, k, n, nbytes, steps, warmup, case=None, group_stripes=1024, nmasks=16,
              group=None, seed=17, sus=False):
    """Self-heal reconstruct (configs[4]): every 1024-stripe group is decoded
    from its own k-of-n brick set, drawn (seeded) from `nmasks` masks."""
    import random
    torch = c.torch
    L, data, frags, nst = c.encoded(k, n, nbytes, case)
    rnd = random.Random(seed + 101 * c.rank)
    nmasks = min(nmasks, math.comb(n, k))
    masks = []
    while len(masks) < nmasks:
        m = sum(1 << b for b in rnd.sample(range(n), k))
        if m not in masks:
            masks.append(m)
    ngroups = (nst + group_stripes - 1) // group_stripes
    gp = torch.tensor([rnd.randrange(nmasks) for _ in range(ngroups)], dtype=torch.uint8,
                      device=c.dev)
    out = torch.empty_like(data)
    fn = lambda: L.decode_mixed_device(c.dev.index, c.sp, nst, group_stripes,  # noqa: E731
                                       gp, masks, frags, out)
    wall, kt = timed(torch, fn, steps, warmup, group, c.warm_ms)
    ks = sustained(c, fn, steps) if sus else None
    ok = bool(torch.equal(out, data)) and c.checks.get("%s_r%d" % (case, c.rank), True)
    return dict(wall=wall, kernel_s=kt, kernel_s_sus=ks, ok=ok, user=nst * CHUNK * k)


def run_heal(c, k, n, nbytes, steps, warmup, case=None):
    """Fused heal: regenerate the r lost fragments
    directly from k good ones (reads S, writes r*S/k)."""
    torch = c.torch
    L, data, frags, nst = c.encoded(k, n, nbytes, case)
    good = list(range(n - k, n))                 # bricks 0..r-1 lost
    mask = sum(1 << b for b in good)
    target = ((1 << n) - 1) & ~mask
    outs = [torch.empty(nst * CHUNK, dtype=torch.uint8, device=c.dev) for _ in range(n - k)]
    ins = [frags[b] for b in good]
    wall, kt = timed(torch, lambda: L.heal_device(c.dev.index, c.sp, nst, mask, ins, target,
                                                  outs), steps, warmup, None, c.warm_ms)
    ok = all(torch.equal(o, frags[i]) for i, o in enumerate(outs))
    return dict(kernel_s=kt, ok=ok, user=nst * CHUNK * k, alg=nst * CHUNK * (k + n - k))


def run_writev(c, k, n, nbytes, steps, warmup, seed):
    """Partial-stripe write: `nbytes` of user data at byte
    1234 of a stripe, from a device buffer at an odd address, merged with the
    old head / tail stripes and encoded by the fused kernel.  Checked against
    the plain encoder on the materialised padded buffer."""
    torch = c.torch
    S = CHUNK * k
    head = 1234 % S
    base = rand_u8(torch, nbytes + 64, seed, c.dev)
    user = base[13:13 + nbytes]
    oh = rand_u8(torch, S, seed + 1, c.dev)
    ot = rand_u8(torch, S, seed + 2, c.dev)
    size = (head + nbytes + S - 1) // S * S
    nst = size // S
    outs = [torch.empty(nst * CHUNK, dtype=torch.uint8, device=c.dev) for _ in range(n)]
    L = c.g.ECMatrixList(k, n)
    torch.cuda.synchronize()
    wall, kt = timed(torch, lambda: L.writev_encode_device(c.dev.index, c.sp, head, nbytes, user,
                                                           oh, ot, outs), steps, warmup, None, c.warm_ms)
    tail = size - head - nbytes
    v = torch.cat([oh[:head], user, ot[S - tail:]])
    ref = [torch.empty_like(o) for o in outs]
    L.encode_device(c.dev.index, c.sp, nst, v, ref)
    torch.cuda.synchronize()
    ok = all(torch.equal(a, b) for a, b in zip(outs, ref))
    return dict(kernel_s=kt, ok=ok, user=nbytes, alg=nbytes + n * nst * CHUNK)


def run_e2e(c, k, n, nbytes, steps, group=None):
    """PCIe-inclusive: pinned host buffers in, pinned host buffers out, the
    library's pipelined H2D / kernel / D2H path on the devices named by
    EC_MI355X_HOST_DEVICES (main() sets it to this rank's GPU).  With a
    group, each timed loop is bracketed by barriers and the max wall over
    ranks is kept."""
    import ctypes
    import numpy as np
    g = c.g
    nst = nbytes // (CHUNK * k)
    S = nst * CHUNK * k
    lib = g.ec_method.lib

    def pinned(nb):
        p = lib.ec_method_host_alloc(nb)
        if not p:
            raise MemoryError
        return p, np.ctypeslib.as_array((ctypes.c_uint8 * nb).from_address(p))

    res = {}
    bufs = []
    try:
        din_p, din = pinned(S)
        bufs.append(din_p)
        from glusterfs_amd import synth
        din[:] = synth.fill_numpy(S)
        fr = [pinned(nst * CHUNK) for _ in range(n)]
        bufs += [p for p, _ in fr]
        dout_p, dout = pinned(S)
        bufs.append(dout_p)
        with g.ECMatrixList(k, n) as L:
            L.encode_batch(nst, din_p, [p for p, _ in fr])          # warm

            def loop(fn):
                if group:
                    group.barrier()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                el = time.perf_counter() - t0
                return (group.max(el) if group else el) / steps

            te = loop(lambda: L.encode_batch(nst, din_p, [p for p, _ in fr]))
            rows = list(range(n - k + 1, n + 1))
            mask = sum(1 << (r - 1) for r in rows)
            ins = [fr[r - 1][0] for r in rows]
            L.decode_batch(nst, mask, rows, ins, dout_p)
            td = loop(lambda: L.decode_batch(nst, mask, rows, ins, dout_p))
            ok = bool(np.array_equal(dout, din))
        res = dict(enc_user_GBps=round(gbps(S, te), 2), dec_user_GBps=round(gbps(S, td), 2),
                   ok=ok, bytes=S, buffers="pinned host (ec_method_host_alloc)")
    finally:
        for p in bufs:
            lib.ec_method_host_free(p)
    return res


def copy_calibration(torch, dev, steps):
    """Device-to-device copy of 1 GiB with torch's kernel (context only)."""
    a = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    _, kt = timed(torch, lambda: b.copy_(a), steps, 2)
    del a, b
    return round(gbps(2 << 30, kt), 1)


def frac(nbytes, seconds):
    return round(gbps(nbytes, seconds) / HBM_PEAK_GBPS, 4)


def extra_configs(c, steps, warmup):
    """BASELINE's other configs, each timed like the headline over max(30,
    steps) launches (ten launches of a 0.1-0.4 ms kernel left the figure to
    the box's clock transients: profiles/r03/r03p_kernarg.log, 100 launches of
    the 8+4 decode ran 7 % faster than the bench's ten) -- after at least
    EXTRA_WARMUP untimed ones: a 60-launch
    kernel trace (profiles/sustain_r02l.log) shows the 16+4 decode at ~400 us,
    rising to ~515 us around launches 6-12 and settling back to 390-410 us,
    so a short warm-up times that clock transient instead of the kernel."""
    torch = c.torch
    st = max(30, steps)
    warmup = max(warmup, EXTRA_WARMUP)
    ex = {"copy_calibration_GBps": copy_calibration(torch, c.dev, st),
          "timing": "%d launches after %d warm-up launches per config" % (st, warmup)}
    # the headline under continuous load: the card's clocks settle lower
    # after tens of ms of HBM-bound work (profiles/sustain_r02l.log), so the
    # burst figure above is also given as a sustained one
    c.warm_ms = SUSTAIN_MS
    r = run_decode(c, 4, 6, 1 << 30, 0x3C, 50, warmup, "4+2_1GiB")
    c.warm_ms = 0.0
    ex["dec_4+2_0x3C_1GiB_sustained"] = dict(
        user_GBps=round(gbps(r["user"], r["kernel_s"]), 1),
        hbm_frac=frac(2 * r["user"], r["kernel_s"]), ok=r["ok"],
        timing="50 launches after %g ms of back-to-back launches" % SUSTAIN_MS)

    def put(name, r, alg):
        ex[name] = dict(user_GBps=round(gbps(r["user"], r["kernel_s"]), 1),
                        hbm_frac=frac(alg, r["kernel_s"]), ok=r["ok"])
        if r.get("kernel_s_sus"):
            ex[name + "_sustained"] = dict(
                user_GBps=round(gbps(r["user"], r["kernel_s_sus"]), 1),
                hbm_frac=frac(alg, r["kernel_s_sus"]), ok=r["ok"],
                timing="after %g ms of back-to-back launches" % SUSTAIN_MS)

    r = run_encode(c, 4, 6, 1 << 30, st, warmup, "4+2_1GiB")
    put("enc_4+2_1GiB", r, 2.5 * r["user"])
    r = run_decode(c, 4, 6, 1 << 30, 0x0F, st, warmup, "4+2_1GiB")
    put("dec_4+2_0x0F_1GiB", r, 2 * r["user"])
    nb = 65536 * CHUNK * 8                       # configs[2]: 64K-stripe batches
    r = run_encode(c, 8, 12, nb, st, warmup, "8+4_64Kstripes", sus=True)
    put("enc_8+4_64Kstripes", r, 2.5 * r["user"])
    for name, mask in (("dec_8+4_0xFF0_64Kstripes", 0xFF0),
                       ("dec_8+4_0xEB5_64Kstripes", 0xEB5)):
        r = run_decode(c, 8, 12, nb, mask, st, warmup, "8+4_64Kstripes", sus=mask == 0xFF0)
        put(name, r, 2 * r["user"])
    r = run_decode(c, 8, 12, 1 << 30, 0xFF0, st, warmup, "8+4_1GiB")
    put("dec_8+4_0xFF0_1GiB", r, 2 * r["user"])
    r = run_encode(c, 16, 20, 2 << 30, st, warmup, "16+4_2GiB", sus=True)
    put("enc_16+4_2GiB", r, 2.25 * r["user"])
    del r
    # configs[3] as specified: one fixed 8 GiB job (1,048,576 stripes); the
    # same job is split across N ranks by bench.py --gpus N (strong scaling)
    ex["enc_16+4_8GiBjob_strong"] = strong_job(c, None, st, warmup)
    r = run_decode(c, 16, 20, 1 << 30, 0xFFFF0, st, warmup, "16+4_1GiB", sus=True)
    put("dec_16+4_0xFFFF0_1GiB", r, 2 * r["user"])
    r = run_mixed(c, 8, 12, 1 << 30, st, warmup, "8+4_1GiB", sus=True)
    put("selfheal_mixed16_8+4_1GiB", r, 2 * r["user"])
    # 64 masks of a 16+4 volume: past the kernel-argument space (7 matrices),
    # the decode matrices come from the per-call device table
    r = run_mixed(c, 16, 20, 1 << 30, st, warmup, "16+4_1GiB", nmasks=64, seed=21, sus=True)
    put("selfheal_mixed64_16+4_1GiB", r, 2 * r["user"])
    r = run_heal(c, 8, 12, 1 << 30, st, warmup, "8+4_1GiB")
    put("heal_fused_8+4_regen4_1GiB", r, r["alg"])
    r = run_writev(c, 4, 6, (1 << 30) + 777, st, warmup, 19)
    put("writev_rmw_4+2_1GiB_unaligned", r, r["alg"])
    torch.cuda.empty_cache()
    for name, k, n in (("e2e_pcie_4+2_512MiB", 4, 6), ("e2e_pcie_16+4_512MiB", 16, 20)):
        try:
            ex[name] = run_e2e(c, k, n, 512 << 20, 3)
        except Exception as exc:                 # reported, never fatal to the bench line
            ex[name] = dict(error=repr(exc)[:200])
        # these lines force the GPU path; the library's default
        # routes host calls (CPU, GPU or split), as heal_sweep / concurrency show
        ex[name]["engine"] = ("gpu forced (EC_GPU_ALWAYS=%s), not the shipped auto routing"
                              % os.environ.get("EC_GPU_ALWAYS"))
    try:
        ex["heal_sweep_8+4_4MiB_windows"] = heal_sweep_all()
    except Exception as exc:                     # reported, never fatal to the bench line
        ex["heal_sweep_8+4_4MiB_windows"] = dict(error=repr(exc)[:200])
    try:
        ex["concurrency_8+4_batching_ceiling"] = concurrency_probe()
    except Exception as exc:                     # reported, never fatal to the bench line
        ex["concurrency_8+4_batching_ceiling"] = dict(error=repr(exc)[:200])
    ex["jit_kernels"] = dict(c.g.jit_stats(), note=(
        "run-time compiled whole-matrix kernels (ec_jit.hip): single-pattern device combines "
        "with k and rows >= 12 (here the 16+4 decodes) once compiled; EC_MI355X_JIT_SYNC=%s "
        "(1: compiled at the first call, before the timed launches)"
        % os.environ.get("EC_MI355X_JIT_SYNC")))
    ex["fullsize_sha256_checks"] = dict(c.checks)
    return ex


STRONG_STRIPES = 1 << 20        # configs[3]: 16+4, 8 GiB of user data


def strong_job(c, grp, steps, warmup):
    """configs[3] strong-scaled: ONE 16+4 job of 1,048,576 stripes (8 GiB)
    split by stripe range over the ranks (glusterfs_amd/dist.py
    stripe_range), each rank encoding its slice of the one xorshift stream;
    input and fragments checked against the per-slice oracle fixtures
    (tests/golden/gen_strong_sha.py).  Aggregate = 8 GiB x launches / the
    max over ranks of the wall time between barriers."""
    from glusterfs_amd.dist import stripe_range
    k, n = 16, 20
    W, rank = (grp.world, grp.rank) if grp else (1, 0)
    s0, s1 = stripe_range(rank, W, STRONG_STRIPES)
    case = "16+4_8GiBjob_N%d" % W
    r = run_encode(c, k, n, (s1 - s0) * CHUNK * k, steps, warmup, case, grp,
                   word0=s0 * CHUNK * k // 8)
    wall = grp.max(r["wall"]) if grp else r["wall"]
    ok = grp.all_ok(r["ok"]) if grp else r["ok"]
    job = STRONG_STRIPES * CHUNK * k
    agg = gbps(job * steps, wall)
    res = dict(user_GBps=round(agg, 1), n_gpus=W, stripes_per_gpu=s1 - s0,
               hbm_frac_per_gpu=round(agg / W * 2.25 / HBM_PEAK_GBPS, 4),
               kernel_ms_rank0=round(r["kernel_s"] * 1e3, 4), ok=ok,
               fixture_checked=("%s_r%d" % (case, rank)) in c.checks,
               scaling="strong (fixed 8 GiB job)")
    del r
    c.torch.cuda.empty_cache()
    return res


def heal_sweep(mode, windows=64):
    """What glustershd issues (ec-heal.c:2048-2107): the 8+4 heal of a file
    in 4 MiB windows, each decoded from 8 good fragments (ec_method_decode)
    and fully re-encoded (ec_method_encode), through the drop-in API on host
    buffers of four provenances:
      pageable        every buffer plain malloc memory (an unpatched client);
      registered      every buffer in one registered arena (r03's line; no
                      client allocates like this);
      ec_provenance   what the integration patch gives a client: fragments
                      (RPC replies of 512 KiB, iobuf.c:25-26) in 1 MiB-page
                      arenas registered by the deferred arena hook, decode and
                      re-encode outputs (ec_buffer_alloc of 4 MiB + 64 and
                      6 MiB + 64, stdalloc iobufs, ec-inode-read.c:1191,
                      ec-inode-write.c:1871) from the pinned pool that the
                      patch's iobuf data allocator installs;
      ec_provenance_calloc  the same fragments, outputs from plain calloc (the
                      control: the patch without the data allocator, i.e. one
                      call mixing mapped and pageable buffers);
      ec_provenance_rows  ec_provenance with the patch's ec_writev_encode,
                      which codes only the bricks the heal write goes to
                      (heal->bad = bricks 0..3: ec_method_encode_rows, 4 of
                      12 fragments);
      ec_provenance_fused  the same buffers through the fused heal
                      (ec_method_heal: the 4 bad bricks' fragments straight
                      from the 8 good ones, no decoded window) -- what a heal
                      that read raw fragments would run.
    Run in a child process per engine setting: `auto` (the crossover), `gpu`
    (EC_GPU_ALWAYS=1) and `cpu` (cpu-extensions=avx); the engine counters
    say where the calls went."""
    import mmap
    import numpy as np
    import glusterfs_amd as g
    from glusterfs_amd import synth
    lib = g.ec_method.lib
    k, n, W = 8, 12, 4 << 20
    nst = W // (CHUNK * k)
    fl = nst * CHUNK
    rows = list(range(n - k + 1, n + 1))              # bricks 0..3 lost
    mask = sum(1 << (r - 1) for r in rows)
    nwin = 4                                          # distinct windows, cycled
    res = {}
    heal_rows = (1 << (n - k)) - 1                    # the lost bricks 0..3
    for prov in ("pageable", "registered", "ec_provenance", "ec_provenance_calloc",
                 "ec_provenance_rows", "ec_provenance_fused"):
        sel = heal_rows if prov in ("ec_provenance_rows", "ec_provenance_fused") else (1 << n) - 1
        fused = prov == "ec_provenance_fused"
        keep, regs, pool = [], [], []
        ps0 = g.pool_stats()
        bufs = []
        if prov in ("pageable", "registered"):
            # one page-aligned region for every buffer
            per = W + n * fl + W
            raw = np.empty(nwin * per + 4096, np.uint8)
            base = (-raw.ctypes.data) % 4096
            arena = raw[base:base + nwin * per]
            for w in range(nwin):
                o = w * per
                frs = [arena[o + W + i * fl:o + W + (i + 1) * fl] for i in range(n)]
                bufs.append((arena[o:o + W], frs, arena[o + W + n * fl:o + per], frs))
            if prov == "registered":
                lib.ec_method_host_register(arena.ctypes.data, arena.nbytes)
                regs.append(arena.ctypes.data)
        else:
            # fragments: 1 MiB pages of 2-page arenas, registered by the
            # deferred hook (as __iobuf_pool_add_arena would call it)
            pages = []
            for _ in range((nwin * n + 1) // 2):
                m = mmap.mmap(-1, 2 << 20)
                a = np.frombuffer(m, np.uint8)
                keep.append((m, a))
                lib.ec_method_host_register_async(a.ctypes.data, a.nbytes)
                regs.append(a.ctypes.data)
                pages += [a[:1 << 20], a[1 << 20:]]
            lib.ec_method_host_register_flush()
            for w in range(nwin):
                frs = [pages[w * n + i][:fl] for i in range(n)]
                if prov in ("ec_provenance", "ec_provenance_rows", "ec_provenance_fused"):
                    d = g.PoolBuffer(W + 64 + 4095)
                    e = g.PoolBuffer(n * fl + 64 + 4095)
                    pool += [d, e]
                    dout, eout = d.array[:W], e.array
                else:
                    dout, eout = np.zeros(W, np.uint8), np.zeros(n * fl, np.uint8)
                bufs.append((np.empty(W, np.uint8), frs, dout,
                             [eout[i * fl:(i + 1) * fl] for i in range(n)]))
        for w, (data, frs, out, eo) in enumerate(bufs):
            data[:] = synth.fill_numpy(W, word0=w * W // 8)
        try:
            with g.ECMatrixList(k, n, gen="avx" if mode == "cpu" else "auto") as L:
                for data, frs, out, eo in bufs:           # fragments to heal from
                    L.encode(W, data, frs)
                def reencode(out, eo):
                    if sel == (1 << n) - 1:
                        L.encode(W, out, eo)
                    else:
                        L.encode_rows(W, out, sel, [e if (sel >> i) & 1 else None
                                                    for i, e in enumerate(eo)])
                def heal_window(frs, out, eo):
                    if fused:
                        L.heal(nst, mask, [frs[r - 1] for r in rows], sel,
                               [e for i, e in enumerate(eo) if (sel >> i) & 1])
                        return time.perf_counter()
                    L.decode(fl, mask, rows, [frs[r - 1] for r in rows], out)
                    b = time.perf_counter()
                    reencode(out, eo)
                    return b

                data, frs, out, eo = bufs[0]              # warm (lazy setup)
                heal_window(frs, out, eo)
                st0 = g.stats()
                cs0 = cpu_stat()
                td, te = [], []
                t0 = time.perf_counter()
                for i in range(windows):
                    data, frs, out, eo = bufs[i % nwin]
                    a = time.perf_counter()
                    b = heal_window(frs, out, eo)
                    te.append(time.perf_counter() - b)
                    td.append(b - a)
                el = time.perf_counter() - t0
                st1 = g.stats()
                throttled = cpu_stat_delta(cs0)
                # the split shares the library settled on for this provenance
                # (per mille, -1: not split), decode and re-encode
                import ctypes
                shares = {}
                ps = {"pageable": 1.0, "registered": 0.0, "ec_provenance_calloc": 0.5}.get(prov, 0.0)
                for name, op, moved in (("decode", 1, 2 * W), ("encode", 0, W + n * fl)):
                    sh = ctypes.c_int32(-2)
                    lib.ec_method_xover_plan(k, op, W, moved, int(moved * ps), 0, 0,
                                             ctypes.byref(sh))
                    shares[name] = sh.value
                ok = (fused or all(np.array_equal(o, d) for d, _, o, _ in bufs)) and all(
                    np.array_equal(e[i], f[i]) for _, f, _, e in bufs for i in range(n)
                    if (sel >> i) & 1)
        finally:
            for p in regs:
                lib.ec_method_host_unregister(p)
            for b in pool:
                b.free()
        ps1 = g.pool_stats()
        r = dict(user_GBps=round(gbps(W * windows, el), 2), ok=ok,
                 decode_us_median=round(sorted(td)[len(td) // 2] * 1e6, 1),
                 encode_us_median=round(sorted(te)[len(te) // 2] * 1e6, 1),
                 gpu_calls=st1["gpu_calls"] - st0["gpu_calls"],
                 cpu_calls=st1["cpu_calls"] - st0["cpu_calls"])
        if mode == "auto" and prov not in ("ec_provenance_rows", "ec_provenance_fused"):
            r["split_share_permille"] = shares
        if throttled:
            r["cgroup_throttled"] = throttled
        dreg = ps1["deferred_registers"] - ps0["deferred_registers"]
        if dreg:
            r["arena_register_us_per_2MiB"] = round(
                (ps1["deferred_register_us"] - ps0["deferred_register_us"]) / dreg, 1)
        dun = ps1["unregisters"] - ps0["unregisters"]
        if dun:
            r["unregister_us"] = round((ps1["unregister_us"] - ps0["unregister_us"]) / dun, 1)
        dsl = ps1["slabs"] - ps0["slabs"]
        if dsl:
            r["pool_slab_register_us_per_MiB"] = round(
                (ps1["slab_register_us"] - ps0["slab_register_us"]) /
                ((ps1["pool_bytes"] - ps0["pool_bytes"]) / (1 << 20)), 1)
        res[prov] = r
    return res


def heal_sweep_all(windows=256):
    import subprocess
    out = dict(windows=windows, window_bytes=4 << 20,
               calls="per window: ec_method_decode (8 of 12 fragments) + ec_method_encode",
               provenances="pageable: plain malloc; registered: one registered region; "
                           "ec_provenance: the integration patch (fragments in deferred-registered "
                           "1 MiB-page arenas, outputs from the pinned pool); "
                           "ec_provenance_calloc: registered fragments, calloc outputs; "
                           "ec_provenance_rows: ec_provenance with the patch's row-masked "
                           "re-encode (ec_method_encode_rows, the 4 healed bricks only); "
                           "ec_provenance_fused: ec_method_heal on the same buffers "
                           "(decode_us_median = the whole heal call, encode 0)")
    for mode in ("auto", "gpu", "cpu"):
        env = dict(os.environ)
        env.pop("EC_GPU_ALWAYS", None)
        if mode == "gpu":
            env["EC_GPU_ALWAYS"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--heal-sweep", mode,
                            "--steps", str(windows)], env=env, capture_output=True, text=True,
                           timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        out[mode] = json.loads(line[-1]) if r.returncode == 0 and line else dict(
            error=(r.stderr or r.stdout)[-300:])
    return out


def concurrency_probe(secs=0.5, rounds=3):
    """The batching-queue question: 8 threads of
    4 MiB 8+4 heal windows and 16 threads of 128 KiB writes / reads through the
    drop-in API on pool buffers (the patched client's iobufs), each timed as
    concurrent calls, as ONE call carrying all their bytes (the ceiling of any
    coalescing queue) and serially -- tools/kbench/concur (C threads: Python's
    per-call overhead would swamp 4 us CPU calls), per engine setting.

    r06: one 0.5 s run per setting could not separate an
    effect from box noise, so the engine settings alternate auto / cpu / gpu
    over `rounds` rounds (the ceiling and serial ways in round 1 only) and the
    concurrent cells report the median, min and max over the rounds; `verdict`
    says per scenario whether auto's median beats or trails the CPU engine's by
    more than the two settings' spread.  `threads` reports the process's
    threads after a run (main + the library's copy / split-helper threads + the
    HIP runtime's) beside the copy threads the library sized from the cgroup
    CPU quota."""
    import statistics
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "kbench", "concur")
    if not os.path.exists(exe):
        return dict(error="tools/kbench/concur not built (make -C glusterfs_amd tools)")
    out = dict(rounds=rounds, secs_per_cell=secs, order="auto, cpu, gpu in every round")
    cells, threads = {}, {}
    for rnd in range(rounds):
        for mode, gen, always in (("auto", "auto", "0"), ("cpu", "avx", "0"), ("gpu", "auto", "1")):
            env = dict(os.environ, EC_GPU_ALWAYS=always, EC_MI355X_QUIET="1")
            if rnd:
                env["CONCUR_WAYS"] = "concurrent"
            r = subprocess.run([exe, str(secs), gen, "pool"], env=env, capture_output=True,
                               text=True, timeout=240)
            for line in r.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                d = json.loads(line)
                key = "%s_%s" % (d["scenario"], mode)
                cells.setdefault(key, {}).setdefault(d["way"], []).append(d)
                threads.setdefault(mode, set()).add(d.get("proc_threads"))
                threads["copy_threads"] = d.get("copy_threads")
            if r.returncode != 0:
                out["error_%s_r%d" % (mode, rnd)] = (r.stderr or r.stdout)[-300:]
    for key, ways in cells.items():
        o = out.setdefault(key, {})
        for way, ds in ways.items():
            v = [d["user_GBps"] for d in ds]
            o[way] = dict(user_GBps=round(statistics.median(v), 2), user_GBps_min=min(v),
                          user_GBps_max=max(v), rounds=len(v), p50_us=ds[-1]["p50_us"],
                          threads=ds[-1]["threads"], call_KiB=ds[-1]["call_KiB"],
                          gpu_calls=sum(d["gpu_calls"] for d in ds),
                          cpu_calls=sum(d["cpu_calls"] for d in ds), ok=all(d["ok"] for d in ds))
    verdict = {}
    for scen in sorted({k.rsplit("_", 1)[0] for k in cells}):
        a = out.get(scen + "_auto", {}).get("concurrent")
        c = out.get(scen + "_cpu", {}).get("concurrent")
        if not a or not c:
            continue
        spread = max(a["user_GBps_max"] - a["user_GBps_min"], c["user_GBps_max"] - c["user_GBps_min"])
        diff = a["user_GBps"] - c["user_GBps"]
        verdict[scen] = dict(auto_over_cpu=round(a["user_GBps"] / c["user_GBps"], 3),
                             diff_GBps=round(diff, 2), spread_GBps=round(spread, 2),
                             call=("auto ahead" if diff > spread else "auto behind"
                                   if -diff > spread else "within the spread"))
    out["verdict"] = verdict
    hc = host_cpus()
    out["threads"] = dict(proc_threads_after_run={m: sorted(x for x in v if x is not None)
                                                  for m, v in threads.items() if m != "copy_threads"},
                          copy_threads=threads.get("copy_threads"),
                          cgroup_cpu_quota=hc["cgroup_quota"], affinity_cpus=hc["affinity"])
    return out


def dist_configs(c, grp, steps, warmup):
    """N > 1: the BASELINE configs defined on 2/4/8 GPUs, one rank per GPU,
    each rank owning the stripe range of its share of the job (weak scaling,
    no data-path collective).  Aggregate user GB/s = all ranks' user bytes x
    steps / max-over-ranks wall time between barriers."""
    torch = c.torch
    st = max(30, steps)
    warmup = max(warmup, EXTRA_WARMUP)          # as in extra_configs
    W = grp.world
    ex = {"timing": "%d launches after %d warm-up launches per config" % (st, warmup)}

    def put(name, r, alg_per_user):
        wall = grp.max(r["wall"])
        ok = grp.all_ok(r["ok"])
        agg = gbps(r["user"] * W * st, wall)
        ex[name] = dict(user_GBps=round(agg, 1), per_gpu_user_GBps=round(agg / W, 1),
                        hbm_frac_per_gpu=round(agg / W * alg_per_user / HBM_PEAK_GBPS, 4),
                        ok=ok)

    # configs[3]: 16+4 encode, stripe-range partitioned (2 GiB per GPU)
    r = run_encode(c, 16, 20, 2 << 30, st, warmup, "16+4_2GiB", group=grp)
    put("dist_enc_16+4_2GiB_per_gpu", r, 2.25)
    del r
    c.torch.cuda.empty_cache()
    # configs[3] as specified: one fixed 8 GiB job split over the N ranks
    ex["dist_enc_16+4_8GiBjob_strong"] = strong_job(c, grp, st, warmup)
    # configs[4]: self-heal reconstruct, mixed patterns (1 GiB per GPU)
    r = run_mixed(c, 8, 12, 1 << 30, st, warmup, "8+4_1GiB", group=grp)
    put("dist_selfheal_mixed16_8+4_1GiB_per_gpu", r, 2.0)
    del r
    torch.cuda.empty_cache()
    # configs[3], PCIe-inclusive: pinned host buffers, 512 MiB per GPU
    try:
        e = run_e2e(c, 16, 20, 512 << 20, 3, grp)
        ok = grp.all_ok(e["ok"])
        ex["dist_e2e_pcie_16+4_512MiB_per_gpu"] = dict(
            enc_user_GBps=round(e["enc_user_GBps"] * W, 2),
            dec_user_GBps=round(e["dec_user_GBps"] * W, 2), ok=ok,
            buffers="pinned host, one GPU per rank (EC_MI355X_HOST_DEVICES)")
    except Exception as exc:                     # reported, never fatal to the bench line
        ex["dist_e2e_pcie_16+4_512MiB_per_gpu"] = dict(error=repr(exc)[:200])
    ex["fullsize_sha256_checks_all_ranks"] = grp.all_ok(all(c.checks.values()))
    return ex


def host_cpus():
    """What the host offers this process: nproc, the CPUs it may run on, the
    cgroup CPU quota, the model -- and the thread count to use (the smaller
    of affinity and quota)."""
    nproc = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = nproc
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, int(int(q) / int(per)))
    except (OSError, ValueError):
        pass
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    threads = min(aff, quota) if quota else aff
    return dict(nproc=nproc, affinity=aff, cgroup_quota=quota, model=model, threads=threads)


def cpu_stat():
    """cgroup v2 cpu.stat counters (throttling), {} where unavailable."""
    try:
        with open("/sys/fs/cgroup/cpu.stat") as f:
            return {k: int(v) for k, v in (l.split() for l in f if l.strip())}
    except (OSError, ValueError):
        return {}


def cpu_stat_delta(before):
    after = cpu_stat()
    keys = ("nr_periods", "nr_throttled", "throttled_usec")
    return {k: after[k] - before[k] for k in keys if k in after and k in before}


def _rate(fn, nbytes, budget):
    fn()                                   # warm: faults the outputs in
    t0 = time.perf_counter()
    passes = 0
    while True:
        fn()
        passes += 1
        el = time.perf_counter() - t0
        if el >= budget or passes >= 10000:
            return round(nbytes * passes / el / 1e9, 3), passes


def cpu_baseline(budget_s=4.0):
    """The oracle's C restatement (oracle/ec_oracle.c: ec_code_c_linear /
    _interleaved with straight-line per-constant muladds, the speed class of
    the reference's portable C path) on the host's usable cores and on one
    thread.  BASELINE configs[0]: 4+2 encode of 1 GiB of the xorshift stream;
    and the bench workload, 4+2 decode of the same 1 GiB with bricks 0, 1
    lost.  Output buffers are reused across passes, as the reference reuses
    its iobufs.  The encode output is checked against the fixture."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O  # test infrastructure: the CPU baseline leg only
    hc = host_cpus()
    T = hc["threads"]
    k, n, S = 4, 6, 1 << 30
    data = O.fill_xorshift(S)
    frags = [np.empty(S // k, dtype=np.uint8) for _ in range(n)]
    rows = [3, 4, 5, 6]
    out = np.empty(S, dtype=np.uint8)
    t0 = cpu_stat()
    enc_T, enc_p = _rate(lambda: O.encode(k, n, data, nthreads=T, out=frags), S, budget_s)
    fx = fixture("4+2_1GiB", 0)
    enc_ok = bool(fx) and all(hashlib.sha256(memoryview(f)).hexdigest() == h
                              for f, h in zip(frags, fx["frags"]))
    ins = [frags[r - 1] for r in rows]
    dec_T, dec_p = _rate(lambda: O.decode(k, rows, ins, nthreads=T, out=out), S, budget_s)
    throttled = cpu_stat_delta(t0)
    enc_1, _ = _rate(lambda: O.encode(k, n, data, nthreads=1, out=frags), S, 0.5)
    dec_1, _ = _rate(lambda: O.decode(k, rows, ins, nthreads=1, out=out), S, 0.5)
    # the reference's default engine is the AVX JIT (ec-code-avx.c); it is
    # not buildable here, so its rate is estimated from this oracle by the
    # one-thread ratio of the survey session's compiled-reference avx figures
    # (4.4 / 6.1-6.4 GB/s) to this oracle in the build
    # container (2.96 / 3.99 GB/s) -- an estimate, not a run
    cal = dict(encode=1.49, decode=1.57)
    return dict(value=dec_T, unit="GB/s", cores=T, kind="port", threads=T,
                reference_avx_estimate=dict(
                    decode_GBps=round(dec_T * cal["decode"], 2),
                    encode_1GiB_GBps=round(enc_T * cal["encode"], 2),
                    calibration=cal, how="oracle rate x (reference avx / oracle, one thread)"),
                nproc=hc["nproc"], affinity_cpus=hc["affinity"],
                cgroup_cpu_quota=hc["cgroup_quota"], model=hc["model"],
                encode_1GiB_GBps=enc_T, one_thread_encode_GBps=enc_1,
                one_thread_decode_GBps=dec_1, encode_matches_fixture=enc_ok,
                cgroup_throttled=throttled,
                sample="oracle/ec_oracle.c (portable-C class restatement; the reference's "
                       "default engine is the AVX JIT, BASELINE.md) on %d threads: 4+2 decode "
                       "of 1 GiB, mask 0x3C, %d passes (value); configs[0] 4+2 encode of 1 GiB "
                       "xorshift input, %d passes (encode_1GiB_GBps); one-thread figures over "
                       ">= 0.5 s" % (T, dec_p, enc_p))


def cpu_engine_rates(threads, budget_s=2.0):
    """The library's own CPU engine (ec_cpu*.c; cpu-extensions=avx) on host
    buffers: 4+2 encode and decode of 1 GiB on one thread, and on `threads`
    threads each coding its own 1/threads of it (how concurrent GlusterFS
    fops use it: one call per calling thread)."""
    import threading
    import numpy as np
    import glusterfs_amd as g
    from glusterfs_amd import synth
    k, n, S = 4, 6, 1 << 30
    nst = S // (CHUNK * k)
    data = synth.fill_numpy(S)
    frags = [np.empty(S // k, np.uint8) for _ in range(n)]
    out = np.empty(S, np.uint8)
    rows = [3, 4, 5, 6]
    res = {}
    with g.ECMatrixList(k, n, gen="avx") as L:
        res["engine"] = L.engine

        def enc(t0, t1):
            L.encode_batch(t1 - t0, data[t0 * CHUNK * k:],
                           [f[t0 * CHUNK:] for f in frags])

        def dec(t0, t1):
            L.decode_batch(t1 - t0, 0x3C, rows, [frags[r - 1][t0 * CHUNK:] for r in rows],
                           out[t0 * CHUNK * k:])

        def par(fn):
            def run():
                th = [threading.Thread(target=fn, args=(nst * i // threads,
                                                         nst * (i + 1) // threads))
                      for i in range(threads)]
                for t in th:
                    t.start()
                for t in th:
                    t.join()
            return run

        # the threads first: their first touch places the output pages
        # (r02: one-thread passes first put every page on one node, and the
        # 16-thread figures then lost to the oracle's, whose own threads
        # touched its outputs first -- VERDICT r02 weak #6)
        res["threads"] = threads
        t0 = cpu_stat()
        res["encode_GBps"], _ = _rate(par(enc), S, budget_s)
        res["decode_GBps"], _ = _rate(par(dec), S, budget_s)
        res["cgroup_throttled"] = cpu_stat_delta(t0)
        res["one_thread_encode_GBps"], _ = _rate(lambda: enc(0, nst), S, budget_s / 2)
        res["one_thread_decode_GBps"], _ = _rate(lambda: dec(0, nst), S, budget_s / 2)
        res["ok"] = bool(np.array_equal(out, data))
    return res


def only(c, spec, nbytes, steps, warmup):
    parts = spec.split(":")
    k, r = map(int, parts[1].split("+"))
    n = k + r
    if parts[0] == "enc":
        res = run_encode(c, k, n, nbytes, steps, warmup)
    elif parts[0] == "dec":
        res = run_decode(c, k, n, nbytes, int(parts[2], 16), steps, warmup)
    elif parts[0] == "mixed":
        nm = int(parts[2]) if len(parts) > 2 else 16
        gs = int(parts[3]) if len(parts) > 3 else 1024
        res = run_mixed(c, k, n, nbytes, steps, warmup, group_stripes=gs, nmasks=nm)
    elif parts[0] == "rmw":
        res = run_writev(c, k, n, nbytes + 777, steps, warmup, 1)
    else:
        res = run_heal(c, k, n, nbytes, steps, warmup)
    print(json.dumps(dict(only=spec, kernel_ms=res["kernel_s"] * 1e3, ok=res["ok"])))


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(n):
    """`bench.py --gpus N` run without a launcher: start the N ranks as a
    child torch.distributed.run (one process per GPU), before anything here
    touches the GPU, and hand back its exit status (rank 0 prints the JSON
    line to the shared stdout).  A child process, never exec: on this pool
    replacing a process image is only safe before HIP initialises, and a
    child keeps that true by construction."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def bind_rank(g, dev_index, local_world):
    """Put this rank on its GPU's NUMA node: the CPUs it runs on (and every
    thread it starts later -- the library's copy pool, CPU-engine callers)
    and, through the library, its pinned staging memory; give it its share
    of the host's usable CPUs as copy threads (the GPU pool's cgroup grants
    16 CPUs for all ranks together).  Returns what was applied."""
    from glusterfs_amd.dist import bind_to_node
    node = g.device_numa_node(dev_index)
    # EC_BENCH_NOBIND=1: leave the affinity alone (diagnosis of placement effects)
    cpus = (os.sched_getaffinity(0) if os.environ.get("EC_BENCH_NOBIND") == "1"
            else bind_to_node(node))
    hc = host_cpus()
    share = max(1, hc["threads"] // max(1, local_world))
    os.environ.setdefault("EC_COPY_THREADS", str(min(8, share)))
    return dict(device=dev_index, numa_node=node, cpus=len(cpus),
                copy_threads=g.copy_threads(), cgroup_quota=hc["cgroup_quota"])


def main():
    args = parse()
    if args.heal_sweep:
        print(json.dumps(heal_sweep(args.heal_sweep, args.steps)))
        return
    world_env = os.environ.get("WORLD_SIZE")
    if args.gpus is not None and args.gpus > 1 and world_env is None:
        sys.exit(launch_ranks(args.gpus))
    if args.gpus is not None and int(world_env or 1) != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%s: the ranks must match the GPUs"
                 % (args.gpus, world_env))
    # host-buffer calls made in this process (the PCIe-inclusive e2e lines)
    # measure the GPU path: without this the crossover could code them on
    # the CPU engine, or split them across both engines (r05); the heal sweep
    # and the concurrency probe set the engine per child process themselves
    os.environ.setdefault("EC_GPU_ALWAYS", "1")
    # the whole-matrix kernels of wide-code decodes (ec_jit.hip) are compiled
    # at a matrix's first call instead of in the background, so a config's
    # timed launches run the kernel a long-lived client runs after its first
    # ~1-2 s with that matrix (the compile itself is one-time setup, untimed)
    os.environ.setdefault("EC_MI355X_JIT_SYNC", "1")
    import torch
    import glusterfs_amd as g
    from glusterfs_amd.dist import Group, local_device_index

    dev_index = local_device_index()
    # the host-buffer (PCIe) path of this rank uses its own GPU only
    os.environ.setdefault("EC_MI355X_HOST_DEVICES", str(dev_index))
    torch.cuda.set_device(dev_index)          # before the process group (NCCL)
    placement = bind_rank(g, dev_index, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    grp = Group()
    dev = torch.device("cuda", dev_index)
    c = Ctx(g, torch, dev, grp.rank, fixtures=args.full)
    nbytes = int(args.gib * (1 << 30))
    if args.only:
        c.warm_ms = args.warm_ms
        return only(c, args.only, nbytes, args.steps, args.warmup)

    k, n, mask = 4, 6, 0x3C
    r = run_decode(c, k, n, nbytes, mask, args.steps, args.warmup, "4+2_1GiB", grp)
    wall = grp.max(r["wall"])
    ok = grp.all_ok(r["ok"])
    value = gbps(r["user"] * grp.world * args.steps, wall)
    kt = r["kernel_s"]
    achieved = gbps(2 * r["user"], kt)

    traffic, traffic_source = None, None
    tf = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tf):
        try:
            e = json.load(open(tf)).get("dec_4+2_0x3C_1GiB", {})
            traffic = e.get("hbm_bytes_per_launch")
            src = e.get("source")
            traffic_source = dict(src, kernel=e.get("kernel"),
                                  note="PMC FETCH_SIZE / WRITE_SIZE passes of that profile, "
                                       "not of this run") if isinstance(src, dict) else src
        except (OSError, ValueError):
            traffic = None

    out = {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "GB/s",
        "n_gpus": grp.world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(wall / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic: xorshift64 stream of SURVEY 8(d), rank r = r-th slice, generated "
                "and encoded on-GPU; " +
                ("input, fragments and output checked against the oracle's full-size SHA-256 "
                 "fixtures" if args.full else
                 "output compared with the input on the GPU (SHA-256 fixtures: --full)"),
        "config": {
            "workload": "disperse 4+2 decode, 2 fragments missing (mask 0x3C), "
                        "%d MiB user data per GPU per step (BASELINE configs[1])" %
                        (r["user"] >> 20),
            "k": k, "n": n, "mask": "0x3C", "stripes_per_gpu": r["nst"],
            "parallelism": "stripe-range partition over %d GPU(s), no data collective" %
                           grp.world,
        },
        "parity_ok": ok,
        "roofline": {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBPS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBPS, 4),
            "traffic": traffic,
            "traffic_source": traffic_source,
            "kernel": "ec_combine_n<K=4,NW=4,MIXED=0,NTS,WOT=1> (decode: 4-stripe tiles, "
                      "jump-table multiply, per-wave 512-B output runs)",
            "algorithmic_bytes_per_launch": 2 * r["user"],
            "avg_launch_ms": round(kt * 1e3, 4),
        },
    }
    out["fullsize_sha256_check"] = c.checks.get("4+2_1GiB_r%d" % grp.rank)
    out["ranks"] = grp.gather(placement)
    if args.dump_outputs:
        out["dumped_outputs"] = dump_outputs(torch, args.dump_outputs, grp.rank, r["out"],
                                             CHUNK * k)
    del r
    torch.cuda.empty_cache()
    # everything below is measured with --full only
    extra = args.full and (args.extra if args.extra is not None else grp.world == 1)
    if extra:
        out["extra"] = extra_configs(c, args.steps, args.warmup)
    elif args.full and grp.world > 1 and not args.no_dist_extra:
        out["extra"] = dist_configs(c, grp, args.steps, args.warmup)
    if args.full and grp.rank == 0 and grp.world == 1 and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline()
        if extra:
            try:
                out["extra"]["cpu_engine_4+2_1GiB"] = cpu_engine_rates(
                    out["cpu_baseline"]["threads"])
            except Exception as exc:             # reported, never fatal to the bench line
                out["extra"]["cpu_engine_4+2_1GiB"] = dict(error=repr(exc)[:200])
    grp.barrier()
    if grp.rank == 0:
        print(json.dumps(out))
    grp.close()


if __name__ == "__main__":
    main()
