/*
 * ec_kernels.hip -- launchers of the gfx950 kernels in ec_kernels_impl.h
 * (see that header for the kernels and the reference functions they replace).
 *
 * Shipped configuration (r03; one-process A/Bs in tools/kbench/kb3.hip,
 * profiles/kb3_r03*.log, and round 1-2's tools/kbench/kbench.hip):
 *   encode   4+2, 8+4: narrow-tile encoders (ec_encode_tile_t, 4-stripe
 *            tiles, per-wave 2 KiB row runs); 16+4: the row-group encoder
 *            (ec_encode_tile_rb, 2 rows per wave), at any input alignment
 *            (LDS-DMA); 2+1 and pinned-host (zero-copy) calls: the
 *            register-resident ec_encode_vander
 *   combine  k <= 8 (decode, heal, mixed, sorted slots, device pattern
 *            table): the narrow-tile ec_combine_n, 4 or 8 waves; k > 8: the
 *            8-stripe ec_combine, 16 waves (two blocks fill a CU's 32 wave
 *            slots); both stage by LDS-DMA into a plane-major tile and
 *            multiply by a jump into the searched XOR programs
 *   scrub    seven kernels on one narrow tile, the check fragments staged
 *            beside the basis, put together from phases that are each
 *            written once (ec_kernels_impl.h) and launched by one launcher
 *            (launch_scrub_tile):
 *   verify   the consistency check: ec_verify_n, phase 1 (the syndromes),
 *            4 bytes out per stripe
 *   locate   the damaged brick per stripe: ec_locate_n, the syndromes kept
 *            in LDS and phase 2 (the single position) for dirty tiles
 *   locate2  up to two damaged bricks per stripe: ec_locate2_n, and phase 3
 *            (the candidate pairs) for open tiles
 *   checked  a read that checks and corrects: ec_decode_checked_n, phases 1
 *   decode   and 2, the named basis chunk corrected in LDS, one dense decode
 *   checked2 the same read around up to two chunks: ec_decode_checked2_n,
 *   decode   phases 1 to 3, at most four products XORed into the named basis
 *            chunks in LDS, one dense decode
 *   checked  a heal that checks its sources: ec_heal_checked_n, the checked
 *   heal     decode with the targets' heal matrix for inv(B), a row per target
 *   checked2 the same heal around up to two chunks: ec_heal_checked2_n, the
 *   heal     checked2 decode with the heal matrix, the target pointers in the
 *            tail of the input list
 *   verified a read and a heal that only detect, from k + 1 fragments:
 *            ec_decode_verified_n and ec_heal_verified_n on the same tile,
 *            the check rows and the output rows in one loop (scrub_verified)
 *   repair  the chunks locate named: ec_repair_n, a ballot scan of loc[]
 *            and up to four dirty stripes of one brick per wave, no LDS
 *   repair2  the one or two chunks locate2 named: ec_repair2_n, the same
 *            scan, a pair rebuilt from the syndromes and locate2's tables
 *   stores   non-temporal on every device-path kernel except the 2+1 / 4+2
 *            register encoders (profiles/kbench_r01_nts.log)
 *   staging  LDS-DMA loads non-temporal for calls whose input exceeds the
 *            MALL (256 MiB), default policy up to it (nt_staging)
 *   host     pinned buffers: the zero-copy kernels (ec_combine_zc,
 *            ec_encode_vander_zc), 1 KiB requests over PCIe
 */
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

#include <cstddef>
#include <cstring>

#include "ec_kernels.h"
#include "ec_kernels_impl.h"
#include "ec_jit.h"

using namespace ecdev;

/* LDS-DMA staging policy override for A/B runs: -1 = by size (shipped),
 * 0 = default policy always, 2 = non-temporal always.  EC_MI355X_LDSNT=0/1
 * sets it at load; tools/kbench/kb3.hip sets it directly. */
int ecdk_ldsnt_override = [] {
    const char *e = getenv("EC_MI355X_LDSNT");
    return e && *e ? (*e == '0' ? kLdsDmaDefault : kLdsDmaNT) : -1;
}();

namespace {

/* Status of the launch just issued on this thread: the entry points clear
 * any stale error first (ec_device.hip clear_stale_error), so a failure here
 * is the launch's, and it is recorded under the kernel's name. */
int launch_ok(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ecd_hip_fail(what, e);
}

/* Check a HIP call whose failure fails the call: recorded, -EIO. */
int hip_ok(hipError_t e, const char *what)
{
    if (e == hipSuccess)
        return 0;
    (void)hipGetLastError();
    return ecd_hip_fail(what, e);
}

/* Non-temporal staging loads for a call that reads more than 256 MiB, the
 * MALL's capacity: none of its input can still be cached when the same data
 * comes round again, and default-policy allocation only costs.  Below that,
 * input a previous call (or producer) left in the MALL is hit.  Same process,
 * shipped / default / nt interleaved (tools/kbench/kb3.hip group ldsnt,
 * profiles/r03/kb3_r03y_ldsnt.log, kb3_r03z_ldsnt_sizes.log), ms:
 *   1 GiB    decode 4+2 0.355 -> 0.327, 8+4 0.356 -> 0.334, 16+4 0.388 ->
 *            0.376; encoders within 0.5 %
 *   320 MiB  decode 4+2 0.109 -> 0.105, 16+4 0.138 -> 0.129; encoders tie
 *   256 MiB  default wins: decode 4+2 0.077 vs 0.086, encode 4+2 0.093 vs
 *            0.107 (a 64K-stripe 8+4 batch is 256 MiB: configs[2])
 *   <= 128 MiB default wins or ties, except small 4+2 decodes */
constexpr uint64_t kNtStagingBytes = 256ull << 20;

/* every input base (and the stride) 16-byte aligned: no staging piece
 * straddles a cache line (see encode_tiles) */
bool inputs_aligned(const CombineArgs &a)
{
    uintptr_t o = (uintptr_t)a.in_stride;
    for (u32 p = 0; p < ECD_MAX_ROWS; ++p)   /* unused entries are null */
        o |= (uintptr_t)a.in_base[p];
    return (o & 15u) == 0;
}

bool nt_staging(uint64_t in_bytes)
{
    if (ecdk_ldsnt_override >= 0)
        return ecdk_ldsnt_override == kLdsDmaNT;
    return in_bytes > kNtStagingBytes;
}

/* Tile order of the tile encoders: block b codes tile b, except for 16+4
 * encodes of >= 4 GiB of input, where each XCD walks its own contiguous run
 * of tiles (blocks go round-robin to the 8 XCDs; ec_kernels_impl.h
 * enc_tile<true>).  A 16+4 encode depends on where its 20 fragments sit (up
 * to +-12 %); at 4-8 GiB the XCD runs were faster for seven
 * placements of eight (4 % on average, the worst placement 7 %), at 2 GiB
 * slower for five of six (3 % on average).  Medians of three rounds after
 * 150 ms of load, ms per call, tile b / XCD runs (profiles/r05/
 * r05at_permab.log, r05au_permab.log, r05av_permab.log):
 *   8 GiB, 6 placements  3.194-3.559 / 3.170-3.296 (mean 3.352 / 3.208)
 *   4 GiB, 2 placements  1.667, 1.604 / 1.627, 1.585
 *   2 GiB, 6 placements  0.801-0.913 / 0.812-0.944 (mean 0.834 / 0.859)
 * For 4+2 and 8+4 at 8 GiB the sign depends on the placement (+-7 %), so
 * they keep tile b.  (Measured and retired in r05/r06: golden-ratio order,
 * 20-28 % slower everywhere, r05as_permab.log; launches cut into 512 MiB /
 * 1 GiB pieces, a third of the 8 GiB 16+4 loss back but every other call
 * slower, r05ao_chunkab.log, r05ap_chunkab.log.) */
constexpr uint64_t kXcdTilesBytes = 4ull << 30;

/* hipFuncAttributeMaxDynamicSharedMemorySize is per device: set it once per
 * (kernel, device), for the device current on the launching thread (a
 * process-wide once-flag left every GPU but the first unconfigured). */
int ensure_lds_limit(const void *kern, int bytes)
{
    static std::mutex mu;
    static std::vector<std::pair<const void *, int>> done;
    int dev = 0;
    if (int rc = hip_ok(hipGetDevice(&dev), "hipGetDevice"))
        return rc;
    std::lock_guard<std::mutex> g(mu);
    for (const auto &e : done)
        if (e.first == kern && e.second == dev)
            return 0;
    if (int rc = hip_ok(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes),
                        "hipFuncSetAttribute(MaxDynamicSharedMemorySize)"))
        return rc;
    done.emplace_back(kern, dev);
    return 0;
}

template <int K, int N, int W, bool NTS = false>
int launch_vander(hipStream_t s, uint64_t nstripes, const void *in, void *const *out, bool zc)
{
    FragPtrs f;
    for (int i = 0; i < N; ++i)
        f.p[i] = static_cast<uint8_t *>(out[i]);
    if (zc && vander_use_zc<W>(nstripes)) {
        hipLaunchKernelGGL((ec_encode_vander_zc<K, N, W>), dim3((u32)kZcBlocks), dim3(kBlock), 0,
                           s, static_cast<const uint8_t *>(in), f, nstripes);
        return launch_ok("launch_vander");
    }
    const uint64_t g = vander_grid<W>(nstripes);
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    hipLaunchKernelGGL((ec_encode_vander<K, N, W, NTS>), dim3((u32)g), dim3(kBlock), 0, s,
                       static_cast<const uint8_t *>(in), f, nstripes);
    return launch_ok("launch_vander");
}

/* The 8-stripe ec_combine (k > 8): single pattern, mixed patterns (kernel
 * arguments or, PG, the device table), or sorted slots (SL). */
template <int K, int NW, bool NTS, bool SL = false, int LA = kLdsDmaDefault>
int launch_combine(hipStream_t s, const CombineArgs &a)
{
    /* sorted slots: every pattern's run may carry up to 7 padding slots */
    const uint64_t g = SL ? (a.nstripes + 8ull * a.npatterns) / 8 + 1 : combine_grid<1>(a.nstripes);
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    const size_t lds = combine_lds<1>(a.k);
    if (a.patg) {
        hipLaunchKernelGGL((ec_combine<K, 1, NW, true, NTS, 2, true, true, 1, SL, 1, LA>), dim3((u32)g),
                           dim3(NW * 64), lds, s, a);
    } else if (a.group_pattern) {
        hipLaunchKernelGGL((ec_combine<K, 1, NW, true, NTS, 2, false, true, 1, SL, 1, LA>), dim3((u32)g),
                           dim3(NW * 64), lds, s, a);
    } else {
        hipLaunchKernelGGL((ec_combine<K, 1, NW, false, NTS, 2, false, true, 1, false, 1, LA>), dim3((u32)g),
                           dim3(NW * 64), lds, s, a);
    }
    return launch_ok("launch_combine");
}

} // namespace

int ecdk_has_vander(uint32_t k, uint32_t n)
{
    return (k == 2 && n == 3) || (k == 4 && n == 6) || (k == 8 && n == 12) ||
           (k == 16 && n == 20);
}

/* EC_MI355X_ENC=0 keeps the register-resident encoder for every geometry
 * (A/B runs); unset = the tile encoders. */
static bool enc_tiles()
{
    static const bool v = [] {
        const char *e = getenv("EC_MI355X_ENC");
        return !(e && *e == '0');
    }();
    return v;
}

namespace {

/* Narrow-tile encoder (ec_encode_tile_t): 4-stripe tiles, NW waves, each
 * fragment row's 4 chunks stored as one 2 KiB run (tools/kbench/kb3.hip,
 * profiles/kb3_r03*.log).  SM: staging mode (ec_kernels_impl.h
 * stage_encode_tile; 1 = partial-stripe write). */
template <int K, int N, int NW, bool DIRECT, int SM, int LA>
int launch_encode_narrow(hipStream_t s, uint64_t nstripes, EncSrc src, void *const *out)
{
    FragPtrs f;
    for (int i = 0; i < N; ++i)
        f.p[i] = static_cast<uint8_t *>(out[i]);
    const uint64_t g = (nstripes + 3) / 4;
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    hipLaunchKernelGGL((ec_encode_tile_t<K, N, 4, NW, true, DIRECT, true, SM, LA>), dim3((u32)g),
                       dim3(NW * 64), (encode_tile_t_lds<4, NW, true>(K)), s, src, f, nstripes);
    return launch_ok("launch_encode_narrow");
}

/* Row-group encoder (ec_encode_tile_rb): 4-stripe tiles, RB rows per wave,
 * so the tile is read from LDS N / RB times instead of N times.  XR: XCD
 * tile runs (kXcdTilesBytes). */
template <int K, int N, int RB, int SM, int LA, bool XR = false>
int launch_encode_rb(hipStream_t s, uint64_t nstripes, EncSrc src, void *const *out)
{
    FragPtrs f;
    for (int i = 0; i < N; ++i)
        f.p[i] = static_cast<uint8_t *>(out[i]);
    const uint64_t g = (nstripes + 3) / 4;
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    hipLaunchKernelGGL((ec_encode_tile_rb<K, N, 4, RB, true, true, SM, LA, XR>), dim3((u32)g),
                       dim3((N / RB) * 64), (encode_tile_rb_lds<N, 4, RB, true>(K)), s, src, f,
                       nstripes);
    return launch_ok("launch_encode_rb");
}

/* The shipped tile encoder of a geometry (4+2, 8+4, 16+4), -ENOTSUP else. */
template <int SM, int LA>
int encode_tiles_la(hipStream_t s, uint32_t k, uint32_t n, uint64_t nstripes, EncSrc src,
                    void *const *out)
{
    if (k == 4 && n == 6)
        return launch_encode_narrow<4, 6, 6, true, SM, LA>(s, nstripes, src, out);
    if (k == 8 && n == 12)
        return launch_encode_narrow<8, 12, 12, false, SM, LA>(s, nstripes, src, out);
    if (k == 16 && n == 20) {
        if constexpr (SM == 0 && LA == kLdsDmaNT)
            if (nstripes * 16 * ECD_CHUNK >= kXcdTilesBytes)
                return launch_encode_rb<16, 20, 2, SM, LA, true>(s, nstripes, src, out);
        return launch_encode_rb<16, 20, 2, SM, LA>(s, nstripes, src, out);
    }
    return -ENOTSUP;
}

/* Partial-stripe writes (SM = 1) keep the default policy: their interior is
 * read at the caller's byte alignment, so neighbouring 16-byte pieces share
 * cache lines, and the non-temporal loads lost there (kb3 ldsnt,
 * profiles/r03/kb3_r03ac_ldsnt_rmw.log, 1 GiB at +3 bytes: 4+2 0.450 ->
 * 0.464 ms, 16+4 0.441 -> 0.447); so do misaligned device inputs. */
template <int SM>
int encode_tiles(hipStream_t s, uint32_t k, uint32_t n, uint64_t nstripes, EncSrc src,
                 void *const *out)
{
    const bool aligned = ((uintptr_t)src.in & 15u) == 0;
    if constexpr (SM == 0)
        if (aligned && nt_staging(nstripes * k * ECD_CHUNK))
            return encode_tiles_la<SM, kLdsDmaNT>(s, k, n, nstripes, src, out);
    /* a byte-misaligned input (a partial write's interior, or a device
     * buffer at an odd offset): dword-aligned loads shifted through
     * registers (SM = 3, ec_kernels_impl.h stage_tile_shift) instead of
     * LDS-DMA at the caller's byte address, whose loads do not coalesce.
     * One process, 1 GiB partial writes, interior 3 bytes off, LDS-DMA ->
     * shift staging (profiles/r05/kb3_r05i_rmw.log; aligned encode beside):
     * 4+2 0.455 -> 0.431 ms (0.429), 8+4 0.513 -> 0.447 (0.419), 16+4 0.440
     * -> 0.424 (0.403).  (With ds_bpermute for the neighbour's dword instead
     * of DPP, 16+4 lost: 0.445 -> 0.455, kb3_r05h_rmw.log -- its row-group
     * encoder is short of LDS cycles.) */
    if (((uintptr_t)src.in & 3u) != 0)
        return encode_tiles_la<3, kLdsDmaDefault>(s, k, n, nstripes, src, out);
    return encode_tiles_la<SM, kLdsDmaDefault>(s, k, n, nstripes, src, out);
}

} // namespace

int ecdk_encode_vander(hipStream_t s, uint32_t k, uint32_t n, uint64_t nstripes,
                       const void *in, void *const *out, bool zc)
{
    /* narrow-tile encoders, kb3 A/B against round 2's encoders (ms per GiB
     * unless noted, profiles/kb3_r03d.log): 4+2 0.438 -> 0.423 (6 waves,
     * direct products), 8+4 0.443 -> 0.411 and 64K-stripe batches 0.126 ->
     * 0.095 ms (12 waves, Horner: one row per wave; the 2 KiB row runs also
     * remove the 64-B segment writes of the register encoder, PMC 1.10x);
     * 16+4: row groups, 2 rows per wave, 10 waves (profiles/r03/
     * kb3_r03j_rowgroups_ct.log: 1 GiB 0.492 -> 0.401 ms, 32K stripes 0.103
     * -> 0.092 against the 8-stripe one-row tile encoder).  They stage by
     * LDS-DMA, which takes any source alignment (a tensor slice at an odd
     * offset; tools/kbench/ldsdma_align.hip). */
    if (!zc && enc_tiles() && ecdk_has_vander(k, n) && k != 2)
        return encode_tiles<0>(s, k, n, nstripes, EncSrc{static_cast<const uint8_t *>(in), nullptr},
                               out);
    if (k == 2 && n == 3)
        return launch_vander<2, 3, 4>(s, nstripes, in, out, zc);
    if (k == 4 && n == 6)
        return launch_vander<4, 6, 2>(s, nstripes, in, out, zc);
    if (k == 8 && n == 12)
        return launch_vander<8, 12, 1, true>(s, nstripes, in, out, zc);
    if (k == 16 && n == 20)
        return launch_vander<16, 20, 1, true>(s, nstripes, in, out, zc);
    return -ENOTSUP;
}

int ecdk_rmw_gather(hipStream_t s, const uint8_t *head, const uint8_t *user, const uint8_t *tail,
                    uint64_t b1, uint64_t b2, uint64_t o0, uint64_t n, uint8_t *dst)
{
    if (n % 16 || ((uintptr_t)dst & 15))
        return -EINVAL;
    const uint64_t g = (n / 16 + kBlock - 1) / kBlock;
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    RmwSrc v{head, user, tail, b1, b2};
    hipLaunchKernelGGL(ec_rmw_gather, dim3((u32)g), dim3(kBlock), 0, s, v, o0, n, dst);
    return launch_ok("ecdk_rmw_gather");
}

template <int K, int N, int W, int LM>
int launch_vander_rmw(hipStream_t s, uint64_t nstripes, const uint8_t *edge,
                      const uint8_t *user_shift, void *const *out)
{
    FragPtrs f;
    for (int i = 0; i < N; ++i)
        f.p[i] = static_cast<uint8_t *>(out[i]);
    const uint64_t g = vander_grid<W>(nstripes);
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    hipLaunchKernelGGL((ec_encode_vander_rmw<K, N, W, LM>), dim3((u32)g), dim3(kBlock), 0, s, edge,
                       user_shift, f, nstripes);
    return launch_ok("launch_vander_rmw");
}

/* LM = 1: dword-aligned loads + v_alignbyte for the interior stripes.
 * Same box, against byte-address loads (profiles/kbench_r02m.log,
 * kbench_r02o.log): 4+2 0.556 -> 0.516 ms per GiB (aligned encoder 0.494),
 * 8+4 0.560 -> 0.548, 16+4 0.535 -> 0.474. */
int ecdk_encode_vander_rmw(hipStream_t s, uint32_t k, uint32_t n, uint64_t nstripes,
                           const uint8_t *edge, const uint8_t *user_shift, void *const *out)
{
    /* the tile encoders (r03): the edges from `edge`, the interior in place
     * at any alignment, both by LDS-DMA.  One process, 1 GiB, interior 3
     * bytes off (profiles/r03/kb3_r03q_ldsdma_unaligned.log): 4+2 0.515 ->
     * 0.453 ms, 8+4 0.545 -> 0.512, 16+4 0.475 -> 0.440 against the
     * register kernel, which 2+1 keeps */
    if (enc_tiles() && k != 2 && ecdk_has_vander(k, n))
        return encode_tiles<1>(s, k, n, nstripes, EncSrc{user_shift, edge}, out);
    if (k == 2 && n == 3)
        return launch_vander_rmw<2, 3, 4, 1>(s, nstripes, edge, user_shift, out);
    if (k == 4 && n == 6)
        return launch_vander_rmw<4, 6, 2, 1>(s, nstripes, edge, user_shift, out);
    if (k == 8 && n == 12)
        return launch_vander_rmw<8, 12, 1, 1>(s, nstripes, edge, user_shift, out);
    if (k == 16 && n == 20)
        return launch_vander_rmw<16, 20, 1, 1>(s, nstripes, edge, user_shift, out);
    return -ENOTSUP;
}

namespace {

const uint8_t *desc_pats(const ecd_combine_desc_t *d)
{
    return d->pat_ext ? d->pat_ext : d->pat;
}

/* Re-lay the packed byte patterns {src[k], coef[rows][k]} out in words:
 * src[] then one word-aligned row per output, pwords words per pattern. */
void pack_words(const ecd_combine_desc_t *d, u32 kw, u32 pwords, u32 *words)
{
    uint8_t *pb = reinterpret_cast<uint8_t *>(words);
    const uint8_t *pats = desc_pats(d);
    for (u32 q = 0; q < d->npatterns; ++q) {
        const uint8_t *src = pats + (size_t)q * d->pat_bytes;
        uint8_t *dst = pb + (size_t)q * pwords * 4;
        memcpy(dst, src, d->k);
        for (u32 r = 0; r < d->rows; ++r)
            memcpy(dst + (size_t)(1 + r) * kw * 4, src + d->k + (size_t)r * d->k, d->k);
    }
}

/* One upload of up to kPatWords pattern words into the device table, the
 * words travelling in the kernel-argument segment (copied at launch, so the
 * host buffer may go away; stream-ordered before the combine that reads it). */
struct PatChunk {
    u32 *dst;
    u32 n;
    u32 w[kPatWords];
};

__global__ __launch_bounds__(256) void ec_pat_upload(const PatChunk c)
{
    for (u32 i = threadIdx.x; i < c.n; i += 256u)
        c.dst[i] = c.w[i];
}

/* Enqueue the upload of `w` into the device table `tab` on `s`. */
int enqueue_upload(hipStream_t s, const std::vector<u32> &w, u32 *tab)
{
    PatChunk c;
    for (size_t o = 0; o < w.size(); o += kPatWords) {
        c.dst = tab + o;
        c.n = (u32)std::min<size_t>(kPatWords, w.size() - o);
        memcpy(c.w, w.data() + o, (size_t)c.n * 4);
        hipLaunchKernelGGL(ec_pat_upload, dim3(1), dim3(256), 0, s, c);
    }
    return launch_ok("enqueue_upload");
}

/* Mixed calls whose patterns exceed the 2 KiB argument space read their
 * decode matrices from a device table.  A self-heal sweep passes the same
 * mask set call after call, so the tables of recent calls stay on the
 * device (per device, LRU): a repeated call skips the allocation and the
 * upload launches (one per 2 KiB: ~9 for 64 masks of 16+4, ~50 us of
 * stream time per call).  An entry is reused only for identical words, and
 * evicted (LRU) only when no call holds it.
 *
 * Ordering is all on the device; no call waits on the host (r05):
 *   - a table is uploaded on the stream of the call that missed, which
 *     records the entry's `ready` event; a call that hits makes its stream
 *     wait for `ready`;
 *   - every stream that read the table records its own reader event at
 *     release(); a reader is a (stream, thread) pair, because
 *     hipStreamPerThread is one handle for a different stream in every
 *     thread, and re-recording a reader's event for its next call is exact
 *     (one in-order stream);
 *   - eviction makes the evicting call's stream wait for every reader event,
 *     then frees the old table and allocates the new one stream-ordered
 *     (hipFreeAsync / hipMallocAsync) on that stream, so the memory is reused
 *     only after every read of it;
 *   - the reader list stays bounded without a wait: entries whose event has
 *     completed are dropped, and past kMaxReaders live readers the oldest is
 *     folded into the releasing stream (it waits for that event, so the
 *     event it records next covers both).
 * r04 waited on the host instead (hipEventSynchronize + hipFree with the
 * lock dropped at eviction, hipEventSynchronize under the lock at the fold)
 * and ignored those calls' errors; one of them failed under the 4-thread
 * evict/hit/upload test on a fresh box and surfaced as a launch -EIO. */
class PatTableCache {
  public:
    struct Ref {
        int slot = -1;
        u32 *ptr = nullptr;
    };

    /* A table holding `w` on the current device, ordered before work that
     * `s` runs after this call; release() it once that work is enqueued. */
    int acquire(hipStream_t s, const std::vector<u32> &w, Ref &ref)
    {
        static const bool off = [] {   /* EC_MI355X_PATCACHE=0: per-call tables (A/B) */
            const char *e = getenv("EC_MI355X_PATCACHE");
            return e && *e == '0';
        }();
        if (off)
            return -EBUSY;
        int dev = 0;
        if (int rc = hip_ok(hipGetDevice(&dev), "hipGetDevice"))
            return rc;
        uint64_t h = 1469598103934665603ull;     /* FNV-1a over the words */
        for (u32 x : w)
            h = (h ^ x) * 1099511628211ull;
        std::lock_guard<std::mutex> g(mu_);
        int victim = -1;
        for (int i = 0; i < kEntries; ++i) {
            Entry &e = e_[i];
            if (e.ptr && e.dev == dev && e.hash == h && e.words == w) {
                if (int rc = hip_ok(hipStreamWaitEvent(s, e.ready, 0),
                                    "hipStreamWaitEvent(pattern table ready)"))
                    return rc;
                ++e.inflight;
                e.tick = ++tick_;
                ref.slot = i;
                ref.ptr = e.ptr;
                return 0;
            }
            if (e.inflight == 0 && (e.dev == dev || !e.ptr) &&
                (victim < 0 || !e.ptr || (e_[victim].ptr && e.tick < e_[victim].tick)))
                victim = i;
        }
        if (victim < 0)
            return -EBUSY;                    /* every entry in use: per call */
        Entry &e = e_[victim];
        if (e.ptr) {
            /* evict: s waits for every reader, then frees the old table */
            for (const Reader &r : e.readers)
                if (int rc = hip_ok(hipStreamWaitEvent(s, r.ev, 0),
                                    "hipStreamWaitEvent(pattern table reader)"))
                    return rc;                /* entry left as it was */
            if (int rc = hip_ok(hipFreeAsync(e.ptr, s), "hipFreeAsync(pattern table)"))
                return rc;
            e.ptr = nullptr;
            e.hash = 0;
            e.words.clear();
            drop_readers(e);                  /* their reads are waited for by s */
        }
        if (e.dev != dev) {                   /* an empty entry moves device */
            drop_readers(e);
            if (e.ready)
                (void)hipEventDestroy(e.ready);
            (void)hipGetLastError();
            e.ready = nullptr;
            e.dev = -1;
            if (int rc = hip_ok(hipEventCreateWithFlags(&e.ready, hipEventDisableTiming),
                                "hipEventCreate(pattern table)")) {
                e.ready = nullptr;
                return rc;
            }
            e.dev = dev;
        }
        u32 *p = nullptr;
        if (hipMallocAsync(reinterpret_cast<void **>(&p), w.size() * 4, s) != hipSuccess) {
            (void)hipGetLastError();
            return -EBUSY;                    /* the per-call table says why */
        }
        int rc = enqueue_upload(s, w, p);
        if (rc == 0)
            rc = hip_ok(hipEventRecord(e.ready, s), "hipEventRecord(pattern table ready)");
        if (rc) {
            (void)hipFreeAsync(p, s);
            (void)hipGetLastError();
            return rc;
        }
        e.ptr = p;
        e.hash = h;
        e.words = w;
        e.tick = ++tick_;
        e.inflight = 1;
        ref.slot = victim;
        ref.ptr = p;
        return 0;
    }

    /* The work that reads the table has been enqueued on `s`.  0, or the
     * error that made release() drain `s` instead of tracking it. */
    int release(const Ref &ref, hipStream_t s)
    {
        const uint64_t tok = s == hipStreamPerThread ? thread_token() : 0;
        int rc = 0;
        {
            std::lock_guard<std::mutex> g(mu_);
            Entry &e = e_[ref.slot];
            hipEvent_t ev = nullptr;
            for (const Reader &r : e.readers)
                if (r.s == s && r.tok == tok)
                    ev = r.ev;
            if (!ev) {
                prune_readers(e, s);
                rc = hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming),
                            "hipEventCreate(pattern table reader)");
                if (rc == 0)
                    e.readers.push_back({s, tok, ev});
                else
                    ev = nullptr;
            }
            if (ev)
                rc = hip_ok(hipEventRecord(ev, s), "hipEventRecord(pattern table reader)");
            --e.inflight;
        }
        if (rc)                                /* untracked: drain the stream */
            (void)hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize");
        return rc;
    }

  private:
    struct Reader {
        hipStream_t s;
        uint64_t tok;        /* thread token for hipStreamPerThread, else 0 */
        hipEvent_t ev;
    };
    struct Entry {
        int dev = -1;
        uint64_t hash = 0, tick = 0;
        std::vector<u32> words;
        u32 *ptr = nullptr;
        hipEvent_t ready = nullptr;           /* the upload has landed */
        std::vector<Reader> readers;
        int inflight = 0;
    };

    /* a token per thread, never reused (a thread id can be) */
    static uint64_t thread_token()
    {
        static std::atomic<uint64_t> next{1};
        static thread_local const uint64_t tok = next.fetch_add(1);
        return tok;
    }

    /* events may be destroyed with work pending on them: the runtime frees
     * them once the work completes, and waits already enqueued still hold */
    static void drop_readers(Entry &e)
    {
        for (const Reader &r : e.readers)
            (void)hipEventDestroy(r.ev);
        e.readers.clear();
        (void)hipGetLastError();
    }

    /* Make room for a new reader without a host wait: drop readers whose
     * reads have completed; if kMaxReaders are still live, `s` waits for the
     * oldest, whose reads the event `s` records next then covers. */
    void prune_readers(Entry &e, hipStream_t s)
    {
        if (e.readers.size() < kMaxReaders)
            return;
        size_t o = 0;
        for (size_t i = 0; i < e.readers.size(); ++i) {
            const hipError_t q = hipEventQuery(e.readers[i].ev);
            if (q == hipSuccess)
                (void)hipEventDestroy(e.readers[i].ev);
            else
                e.readers[o++] = e.readers[i];
        }
        e.readers.resize(o);
        (void)hipGetLastError();              /* hipErrorNotReady is no error */
        if (e.readers.size() >= kMaxReaders &&
            hipStreamWaitEvent(s, e.readers.front().ev, 0) == hipSuccess) {
            (void)hipEventDestroy(e.readers.front().ev);
            e.readers.erase(e.readers.begin());
        }
        (void)hipGetLastError();
    }

    static constexpr int kEntries = 16;
    static constexpr size_t kMaxReaders = 16;
    std::mutex mu_;
    Entry e_[kEntries];
    uint64_t tick_ = 0;
};

/* never destroyed: tables and events would be freed after the runtime */
PatTableCache &pat_tables()
{
    static PatTableCache *c = new PatTableCache;
    return *c;
}

/* The device table of a mixed call: from the cache, or (all entries busy)
 * a per-call table (stream-ordered allocation, freed after the combine). */
int upload_table(hipStream_t s, const ecd_combine_desc_t *d, CombineArgs &a, u32 **tab,
                 PatTableCache::Ref &ref)
{
    /* one zero word behind the last pattern: the k > 8 kernel fetches a row's
     * words rw + 1 ... rw + 3 by its compile-time K, so with kw = 3 (k = 9 ...
     * 12) the last row of the last pattern reads one word past its end */
    const size_t nw = (size_t)a.pwords * a.npatterns + 1;
    std::vector<u32> w(nw, 0u);
    pack_words(d, a.kw, a.pwords, w.data());
    const int rc = pat_tables().acquire(s, w, ref);
    if (rc == 0) {
        a.patg = ref.ptr;
        return 0;
    }
    if (rc != -EBUSY)
        return rc;
    if (const hipError_t e = hipMallocAsync(reinterpret_cast<void **>(tab), nw * 4, s)) {
        *tab = nullptr;
        (void)hip_ok(e, "hipMallocAsync(per-call pattern table)");
        return -ENOMEM;
    }
    a.patg = *tab;
    return enqueue_upload(s, w, *tab);
}

/* Pattern groups below one tile: sort the stripes by pattern into slot
 * runs padded to 8 (ec_slots_*), then tiles(stream, args-with-slots). */
template <bool NTS, typename F>
int sorted_slots(hipStream_t s, const CombineArgs &a0, F tiles)
{
    if (a0.nstripes == 0)
        return 0;
    if (a0.nstripes + 8ull * a0.npatterns >= 0xFFFFFFFFull)
        return -EINVAL;                 /* slots hold 32-bit stripe numbers */
    const uint64_t nslots_max = a0.nstripes + 8ull * a0.npatterns;
    u32 *ws = nullptr;
    const size_t bytes = (size_t)(512 + 1 + nslots_max) * 4;
    if (const hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&ws), bytes, s)) {
        (void)hip_ok(e, "hipMallocAsync(slot workspace)");
        return -ENOMEM;
    }
    u32 *counts = ws, *cursors = ws + 256, *total = ws + 512, *slots = ws + 513;
    CombineArgs a = a0;
    a.slot_stripe = slots;
    a.slot_count = total;
    const uint64_t nb = (a.nstripes + kSlotBlock * kSlotPerThread - 1) / (kSlotBlock * kSlotPerThread);
    int rc = 0;
    rc = hip_ok(hipMemsetAsync(counts, 0, 256 * 4, s), "hipMemsetAsync(slot counts)");
    if (rc == 0)
        rc = hip_ok(hipMemsetAsync(slots, 0xFF, nslots_max * 4, s), "hipMemsetAsync(slots)");
    if (rc == 0) {
        hipLaunchKernelGGL(ec_slots_count, dim3((u32)nb), dim3(kSlotBlock), 0, s, a, counts);
        hipLaunchKernelGGL(ec_slots_scan, dim3(1), dim3(256), 0, s, counts, cursors, total);
        hipLaunchKernelGGL(ec_slots_scatter, dim3((u32)nb), dim3(kSlotBlock), 0, s, a, cursors,
                           slots);
        rc = launch_ok("sorted_slots");
    }
    if (rc == 0)
        rc = tiles(s, a);
    const int frc = hip_ok(hipFreeAsync(ws, s), "hipFreeAsync(slot workspace)");
    return rc ? rc : frc;
}

/* ------------------------------------------------ narrow tiles (r03) */

template <int K, int NW, bool MIXED, bool NTS, int WOT, bool PG, bool SL, int LA>
int launch_n1(hipStream_t s, const CombineArgs &a, uint64_t g)
{
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    const size_t lds = combine_n_lds<NW, WOT>((int)a.k);
    hipLaunchKernelGGL((ec_combine_n<K, NW, MIXED, NTS, WOT, PG, SL, 1, LA>), dim3((u32)g),
                       dim3(NW * 64), lds, s, a);
    return launch_ok("launch_n1");
}

/* one k-bucket: single pattern, mixed, device pattern table, sorted slots */
template <int K, int NW, int WOT, bool NTS, int LA>
int launch_narrow_k(hipStream_t s, const CombineArgs &a)
{
    if (!a.group_pattern)
        return launch_n1<K, NW, false, NTS, WOT, false, false, LA>(s, a, (a.nstripes + 3) / 4);
    if (a.group_shift >= 2)          /* groups of >= 4 stripes: a tile is one pattern's */
        return a.patg ? launch_n1<K, NW, true, NTS, WOT, true, false, LA>(s, a, (a.nstripes + 3) / 4)
                      : launch_n1<K, NW, true, NTS, WOT, false, false, LA>(s, a, (a.nstripes + 3) / 4);
    return sorted_slots<NTS>(s, a, [](hipStream_t st, const CombineArgs &b) {
        /* runs padded to multiples of 8 slots: worst case 7 per pattern */
        const uint64_t g = (b.nstripes + 8ull * b.npatterns) / 4 + 1;
        return b.patg ? launch_n1<K, NW, true, NTS, WOT, true, true, LA>(st, b, g)
                      : launch_n1<K, NW, true, NTS, WOT, false, true, LA>(st, b, g);
    });
}

/* The device combine for k <= 8: narrow tiles with per-wave output staging
 * (tools/kbench/kb3.hip, one process, 7 interleaved rounds against the
 * round-2 dispatch, profiles/kb3_r03d.log, ms per GiB unless noted):
 *   4+2 decode (dense)      0.366 -> 0.350   4 waves
 *   8+4 decode              0.371 -> 0.350   4 waves
 *   8+4 decode, 64K stripes 0.096 -> 0.083   8 waves (small batches)
 *   8+4 heal (4 rows)       0.316 -> 0.263   4 waves
 *   8+4 mixed, 16 masks     0.395 -> 0.375   4 waves
 * k = 16 keeps the 8-stripe ec_combine with 16 waves: 16+4 decode 0.406
 * against 0.421 at best narrow (8 waves, register stores), mixed 0.395
 * against 0.442.  Groups below a tile (8 stripes for ec_combine, 4 for the
 * narrow tiles) are sorted into slots first. */
template <bool NTS, int LA>
int launch_combine_k(hipStream_t s, const CombineArgs &a)
{
    if (a.k <= 4)
        return launch_narrow_k<4, 4, 1, NTS, LA>(s, a);
    if (a.k <= 8)
        return a.nstripes <= (1u << 17) ? launch_narrow_k<8, 8, 1, NTS, LA>(s, a)
                                        : launch_narrow_k<8, 4, 1, NTS, LA>(s, a);
    if (a.group_pattern && a.group_shift < 3)
        return sorted_slots<NTS>(s, a, [](hipStream_t st, const CombineArgs &b) {
            return launch_combine<16, 16, NTS, true, LA>(st, b);
        });
    return launch_combine<16, 16, NTS, false, LA>(s, a);
}

/* pack, then launch; -E2BIG from the packer means "use a device table" */
template <bool NTS>
int combine_any(hipStream_t s, const ecd_combine_desc_t *d)
{
    CombineArgs a;
    int rc = ecdk_pack_args(d, &a);
    u32 *tab = nullptr;
    PatTableCache::Ref ref;
    if (rc == -E2BIG && d->group_pattern)
        rc = upload_table(s, d, a, &tab, ref);
    /* staging policy by the call's input bytes; the host-buffer fallback
     * (NTS = false: pinned memory over PCIe) keeps the default policy */
    if (rc == 0) {
        if constexpr (NTS) {
            const bool nt = nt_staging(a.nstripes * a.k * ECD_CHUNK) && inputs_aligned(a);
            rc = nt ? launch_combine_k<NTS, kLdsDmaNT>(s, a)
                    : launch_combine_k<NTS, kLdsDmaDefault>(s, a);
        } else {
            rc = launch_combine_k<NTS, kLdsDmaDefault>(s, a);
        }
    }
    if (ref.slot >= 0)
        (void)pat_tables().release(ref, s);   /* a failure drained s: the call stands */
    if (tab) {
        const int frc = hip_ok(hipFreeAsync(tab, s), "hipFreeAsync(per-call pattern table)");
        rc = rc ? rc : frc;
    }
    return rc;
}

} // namespace

/* Validate and fill the kernel arguments.  Returns -E2BIG (header filled,
 * patterns not packed) when the patterns exceed the argument space. */
int ecdk_pack_args(const ecd_combine_desc_t *d, CombineArgs *a)
{
    if (d->k == 0 || d->k > ECD_MAX_K || d->rows == 0 || d->rows > ECD_MAX_ROWS)
        return -EINVAL;
    if (d->group_pattern && d->group_shift > 40)
        return -EINVAL; /* groups below 8 stripes run through sorted slots */
    if (d->npatterns == 0 || d->npatterns > ECD_MAX_PATTERNS ||
        (!d->pat_ext && (uint64_t)d->npatterns * d->pat_bytes > ECD_MAX_PAT_BYTES) ||
        d->pat_bytes < d->k + d->rows * d->k)
        return -EINVAL;
    memcpy(a->in_base, d->in_base, sizeof(a->in_base));
    memcpy(a->out_base, d->out_base, sizeof(a->out_base));
    a->in_stride = d->in_stride;
    a->out_stride = d->out_stride;
    a->nstripes = d->nstripes;
    a->group_pattern = d->group_pattern;
    a->patg = nullptr;
    a->slot_stripe = nullptr;
    a->slot_count = nullptr;
    a->k = d->k;
    a->kw = (d->k + 3) / 4;
    a->rows = d->rows;
    a->group_shift = d->group_shift;
    a->pwords = a->kw * (1 + d->rows);
    a->npatterns = d->npatterns;
    if (a->pwords > kMaxPatWords)
        return -EINVAL;
    if ((uint64_t)a->pwords * d->npatterns > kPatWords)
        return -E2BIG;
    memset(a->pat, 0, sizeof(a->pat));
    pack_words(d, a->kw, a->pwords, a->pat);
    return 0;
}

/* Every combine stages its inputs by LDS-DMA (global_load_lds_dwordx4), which
 * takes any source alignment (tools/kbench/ldsdma_align.hip,
 * profiles/r03/ldsdma_align.log): fragments at odd offsets (torch slices)
 * are read in place.  (Round 2 copied them to aligned scratch first.) */
/* A single-pattern combine of a wide code whose coefficient matrix has a
 * compiled whole-matrix kernel (ec_jit.hip, r06) runs that; every other
 * call, and the calls of a matrix whose code is still being compiled, run
 * the shipped kernels. */
int ecdk_combine(hipStream_t s, const ecd_combine_desc_t *d)
{
    if (ecj_eligible(d)) {
        uintptr_t o = (uintptr_t)d->in_stride;
        const uint8_t *pat = d->pat_ext ? d->pat_ext : d->pat;
        for (u32 p = 0; p < d->k; ++p)
            o |= (uintptr_t)d->in_base[pat[p]];
        const bool nt = nt_staging(d->nstripes * d->k * ECD_CHUNK) && (o & 15u) == 0;
        if (ecj_launch(s, d, nt) == 0)
            return 0;
    }
    return combine_any<true>(s, d);
}

/* ------------------------------------------- consistency check (scrub) */

namespace {

/* the template arguments of one instantiation of a scrub tile kernel */
template <int K_, int NW_, int LA_>
struct ScrubCfg {
    static constexpr int K = K_, NW = NW_, LA = LA_;
};

/* The launch of a four-stripe scrub tile kernel, for all of them.
 * kernel(ScrubCfg<K, NW, LA>{}) gives the instantiation to run on the packed
 * arguments a; k, rows and nstripes are the geometry in a, align the OR of
 * its input addresses, nf the kernel's words per stripe, and a failed launch
 * is recorded under `what`. */
template <typename Args, typename Kernel>
int launch_scrub_tile(hipStream_t s, const Args &a, u32 k, u32 rows, uint64_t nstripes,
                      uintptr_t align, u32 nf, const char *what, Kernel kernel)
{
    const uint64_t g = (nstripes + 3) / 4;
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    /* at most 31 inputs (the ecdk_ functions check): 62 KiB + 48 with three
     * words per stripe, under the 64 KiB a launch takes without raising the
     * kernel's dynamic LDS limit */
    const size_t lds = scrub_tile_lds(k + rows, nf);
    auto launch = [&](auto cfg) {
        const auto fn = kernel(cfg);
        hipLaunchKernelGGL(fn, dim3((u32)g), dim3(decltype(cfg)::NW * 64), lds, s, a);
        return launch_ok(what);
    };
    /* the k -> K buckets and wave counts of launch_combine_k's narrow tiles;
     * k > 8 runs 8 waves (two 62 KiB tiles of a 16+15 volume share a CU) */
    auto bucket = [&](auto la) {
        constexpr int LA = decltype(la)::value;
        if (k <= 4)
            return launch(ScrubCfg<4, 4, LA>{});
        if (k <= 8)
            return nstripes <= (1u << 17) ? launch(ScrubCfg<8, 8, LA>{})
                                          : launch(ScrubCfg<8, 4, LA>{});
        return launch(ScrubCfg<16, 8, LA>{});
    };
    /* the staging policy of ecdk_combine, by the bytes the call reads */
    const bool nt = nt_staging(nstripes * (k + rows) * ECD_CHUNK) && (align & 15u) == 0;
    return nt ? bucket(std::integral_constant<int, kLdsDmaNT>{})
              : bucket(std::integral_constant<int, kLdsDmaDefault>{});
}

} // namespace

/* d: the heal combination of the check rows (k inputs, d->rows coefficient
 * rows, one pattern in d->pat); check[r] / check_brick[r]: the stored
 * fragment and brick index of row r; bad: nstripes device dwords. */
int ecdk_verify(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                const uint8_t *check_brick, uint32_t *bad)
{
    VerifyArgs a;
    if (d->k == 0 || d->k > ECD_MAX_K || d->rows == 0 || d->k + d->rows >= ECD_MAX_ROWS ||
        d->npatterns != 1 || d->pat_ext || d->group_pattern ||
        d->pat_bytes < d->k + d->rows * d->k || d->in_stride != ECD_CHUNK || !check ||
        !check_brick || !bad || ((uintptr_t)bad & 3u))
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = d->k;
    a.kw = (d->k + 3) / 4;
    a.rows = d->rows;
    a.nstripes = d->nstripes;
    a.bad = bad;
    if (a.kw * a.rows > kMaxPatWords)
        return -EINVAL;
    uintptr_t o = 0;
    for (u32 p = 0; p < a.k; ++p) {
        const uint8_t src = d->pat[p];
        if (src >= ECD_MAX_ROWS || !d->in_base[src])
            return -EINVAL;
        a.in[p] = static_cast<const uint8_t *>(d->in_base[src]);
        o |= (uintptr_t)a.in[p];
    }
    for (u32 r = 0; r < a.rows; ++r) {
        if (!check[r] || check_brick[r] >= 32)
            return -EINVAL;
        a.in[a.k + r] = static_cast<const uint8_t *>(check[r]);
        o |= (uintptr_t)check[r];
        a.brick[r >> 2] |= (u32)check_brick[r] << ((r & 3u) * 8u);
        for (u32 p = 0; p < a.k; ++p)
            a.coef[r * a.kw + (p >> 2)] |= (u32)d->pat[a.k + r * a.k + p] << ((p & 3u) * 8u);
    }
    return launch_scrub_tile(s, a, a.k, a.rows, a.nstripes, o, 1, "launch_verify", [](auto c) {
        using C = decltype(c);
        return &ec_verify_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------------- locating the damaged brick */

/* The arguments of ec_locate_n from what ecdk_locate is given; *align gets
 * the OR of the input addresses (the staging policy wants it). */
static int pack_locate(const ecd_combine_desc_t *d, const void *const *check,
                       const uint8_t *check_brick, const uint8_t *basis_brick,
                       const uint8_t *ratio, uint32_t *loc, LocateArgs &a, uintptr_t *align)
{
    if (d->k == 0 || d->k > ECD_MAX_K || d->rows < 2 || d->k + d->rows >= ECD_MAX_ROWS ||
        d->npatterns != 1 || d->pat_ext || d->group_pattern ||
        d->pat_bytes < d->k + d->rows * d->k || d->in_stride != ECD_CHUNK || !check ||
        !check_brick || !basis_brick || !ratio || !loc || ((uintptr_t)loc & 3u))
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = d->k;
    a.kw = (d->k + 3) / 4;
    a.rows = d->rows;
    a.nstripes = d->nstripes;
    a.loc = loc;
    if (a.kw * a.rows > kLocateWords)
        return -EINVAL;
    uintptr_t o = 0;
    for (u32 p = 0; p < a.k; ++p) {
        const uint8_t src = d->pat[p];
        if (src >= ECD_MAX_ROWS || !d->in_base[src] || basis_brick[p] >= 31)
            return -EINVAL;
        a.in[p] = static_cast<const uint8_t *>(d->in_base[src]);
        o |= (uintptr_t)a.in[p];
        a.bbrick[p >> 2] |= (u32)basis_brick[p] << ((p & 3u) * 8u);
    }
    for (u32 r = 0; r < a.rows; ++r) {
        if (!check[r] || check_brick[r] >= 31)
            return -EINVAL;
        a.in[a.k + r] = static_cast<const uint8_t *>(check[r]);
        o |= (uintptr_t)check[r];
        a.cbrick[r >> 2] |= (u32)check_brick[r] << ((r & 3u) * 8u);
        for (u32 p = 0; p < a.k; ++p) {
            a.coef[r * a.kw + (p >> 2)] |= (u32)d->pat[a.k + r * a.k + p] << ((p & 3u) * 8u);
            if (r > 0)
                a.ratio[(r - 1) * a.kw + (p >> 2)] |= (u32)ratio[(r - 1) * a.k + p]
                                                      << ((p & 3u) * 8u);
        }
    }
    *align = o;
    return 0;
}

/* d, check, check_brick: as ecdk_verify, with at least two rows;
 * basis_brick[p]: brick index of input p; ratio: (rows - 1) x k bytes,
 * coefficient of row r over that of row 0; loc: nstripes device dwords. */
int ecdk_locate(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                const uint8_t *check_brick, const uint8_t *basis_brick, const uint8_t *ratio,
                uint32_t *loc)
{
    LocateArgs a;
    uintptr_t o = 0;
    if (int rc = pack_locate(d, check, check_brick, basis_brick, ratio, loc, a, &o))
        return rc;
    return launch_scrub_tile(s, a, a.k, a.rows, a.nstripes, o, 2, "launch_locate", [](auto c) {
        using C = decltype(c);
        return &ec_locate_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------------- a read that checks and corrects */

/* As ecdk_locate, then inv: k x k bytes, the decode matrix of the basis (row
 * j gives output chunk j); ginv: k bytes, 1 / coefficient of row 0; out:
 * nstripes * k * 512 device bytes at any alignment.  Every table travels in
 * the kernel arguments: nothing is uploaded. */
int ecdk_decode_checked(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                        const uint8_t *check_brick, const uint8_t *basis_brick,
                        const uint8_t *ratio, const uint8_t *inv, const uint8_t *ginv, void *out,
                        uint32_t *loc)
{
    static_assert(sizeof(DecodeCheckedArgs) <= 2048, "the tables must fit the kernel arguments");
    DecodeCheckedArgs a;
    uintptr_t o = 0;
    if (!inv || !ginv || !out)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    if (int rc = pack_locate(d, check, check_brick, basis_brick, ratio, loc, a.l, &o))
        return rc;
    const u32 k = a.l.k, kw = a.l.kw;
    a.out = static_cast<uint8_t *>(out);
    for (u32 p = 0; p < k; ++p) {
        if (ginv[p] == 0)
            return -EINVAL;
        a.bmask |= 1u << basis_brick[p];
        a.ginv[p >> 2] |= (u32)ginv[p] << ((p & 3u) * 8u);
        for (u32 j = 0; j < k; ++j)
            a.inv[j * kw + (p >> 2)] |= (u32)inv[j * k + p] << ((p & 3u) * 8u);
    }
    return launch_scrub_tile(s, a, k, a.l.rows, a.l.nstripes, o, 2, "launch_decode_checked",
                             [](auto c) {
        using C = decltype(c);
        return &ec_decode_checked_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------------- a heal that checks its sources */

/* As ecdk_locate, then ntargets: the m targets; heal: m x k bytes, the heal
 * matrix of the targets from the basis (row j gives the chunk of target j);
 * ginv: k bytes, 1 / coefficient of row 0; out: the m target fragments,
 * nstripes * 512 device bytes each at any alignment.  Every table travels in
 * the kernel arguments: nothing is uploaded. */
int ecdk_heal_checked(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                      const uint8_t *check_brick, const uint8_t *basis_brick,
                      const uint8_t *ratio, uint32_t ntargets, const uint8_t *heal,
                      const uint8_t *ginv, void *const *out, uint32_t *loc)
{
    static_assert(sizeof(HealCheckedArgs) <= 2048, "the tables must fit the kernel arguments");
    HealCheckedArgs a;
    uintptr_t o = 0;
    if (!heal || !ginv || !out || ntargets == 0)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    if (int rc = pack_locate(d, check, check_brick, basis_brick, ratio, loc, a.l, &o))
        return rc;
    const u32 k = a.l.k, kw = a.l.kw;
    /* the inputs and the targets are different bricks of at most 31 */
    if (k + a.l.rows + ntargets >= ECD_MAX_ROWS || kw * ntargets > kLocateWords)
        return -EINVAL;
    a.m = ntargets;
    for (u32 j = 0; j < ntargets; ++j) {
        if (!out[j])
            return -EINVAL;
        a.out[j] = static_cast<uint8_t *>(out[j]);
        for (u32 p = 0; p < k; ++p)
            a.heal[j * kw + (p >> 2)] |= (u32)heal[j * k + p] << ((p & 3u) * 8u);
    }
    for (u32 p = 0; p < k; ++p) {
        if (ginv[p] == 0)
            return -EINVAL;
        a.bmask |= 1u << basis_brick[p];
        a.ginv[p >> 2] |= (u32)ginv[p] << ((p & 3u) * 8u);
    }
    return launch_scrub_tile(s, a, k, a.l.rows, a.l.nstripes, o, 2, "launch_heal_checked",
                             [](auto c) {
        using C = decltype(c);
        return &ec_heal_checked_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------------- detect-only from k + 1 */

/* VerifyArgs' fields of DecodeVerifiedArgs or HealVerifiedArgs from what
 * ecdk_verify is given; *align gets the OR of the input addresses. */
template <typename A>
static int pack_verified(const ecd_combine_desc_t *d, const void *const *check,
                         const uint8_t *check_brick, uint32_t *bad, A &a, uintptr_t *align)
{
    if (d->k == 0 || d->k > ECD_MAX_K || d->rows == 0 || d->k + d->rows >= ECD_MAX_ROWS ||
        d->npatterns != 1 || d->pat_ext || d->group_pattern ||
        d->pat_bytes < d->k + d->rows * d->k || d->in_stride != ECD_CHUNK || !check ||
        !check_brick || !bad || ((uintptr_t)bad & 3u))
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = d->k;
    a.kw = (d->k + 3) / 4;
    a.rows = d->rows;
    a.nstripes = d->nstripes;
    a.bad = bad;
    uintptr_t o = 0;
    for (u32 p = 0; p < a.k; ++p) {
        const uint8_t src = d->pat[p];
        if (src >= ECD_MAX_ROWS || !d->in_base[src])
            return -EINVAL;
        a.in[p] = static_cast<const uint8_t *>(d->in_base[src]);
        o |= (uintptr_t)a.in[p];
    }
    for (u32 r = 0; r < a.rows; ++r) {
        if (!check[r] || check_brick[r] >= 31)
            return -EINVAL;
        a.in[a.k + r] = static_cast<const uint8_t *>(check[r]);
        o |= (uintptr_t)check[r];
        a.brick[r >> 2] |= (u32)check_brick[r] << ((r & 3u) * 8u);
    }
    *align = o;
    return 0;
}

/* rows [r0, r0 + n) of a scrub coefficient table from n x k bytes */
static void pack_rows(u32 *coef, u32 r0, u32 n, u32 k, u32 kw, const uint8_t *m)
{
    for (u32 r = 0; r < n; ++r)
        for (u32 p = 0; p < k; ++p)
            coef[(r0 + r) * kw + (p >> 2)] |= (u32)m[r * k + p] << ((p & 3u) * 8u);
}

/* As ecdk_verify, then inv: k x k bytes, the decode matrix of the basis (row
 * j gives output chunk j); out: nstripes * k * 512 device bytes at any
 * alignment.  Every table travels in the kernel arguments: nothing is
 * uploaded. */
int ecdk_decode_verified(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                         const uint8_t *check_brick, const uint8_t *inv, void *out,
                         uint32_t *bad)
{
    static_assert(sizeof(DecodeVerifiedArgs) <= 2048, "the tables must fit the kernel arguments");
    static_assert((ECD_MAX_ROWS - 1) * (ECD_MAX_K / 4) <= kMaxPatWords,
                  "check rows and inv(B) share one table");
    DecodeVerifiedArgs a;
    uintptr_t o = 0;
    if (!inv || !out)
        return -EINVAL;
    if (int rc = pack_verified(d, check, check_brick, bad, a, &o))
        return rc;
    /* a rows of kw words: at most 31 * 4 */
    pack_rows(a.coef, 0, a.rows, a.k, a.kw, d->pat + a.k);
    pack_rows(a.coef, a.rows, a.k, a.k, a.kw, inv);
    a.out = static_cast<uint8_t *>(out);
    return launch_scrub_tile(s, a, a.k, a.rows, a.nstripes, o, 1, "launch_decode_verified",
                             [](auto c) {
        using C = decltype(c);
        return &ec_decode_verified_n<C::K, C::NW, C::LA>;
    });
}

/* As ecdk_verify, then ntargets: the m targets; heal: m x k bytes, the heal
 * matrix of the targets from the basis (row j gives the chunk of target j);
 * out: the m target fragments, nstripes * 512 device bytes each at any
 * alignment.  Every table travels in the kernel arguments: nothing is
 * uploaded. */
int ecdk_heal_verified(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                       const uint8_t *check_brick, uint32_t ntargets, const uint8_t *heal,
                       void *const *out, uint32_t *bad)
{
    static_assert(sizeof(HealVerifiedArgs) <= 2048, "the tables must fit the kernel arguments");
    HealVerifiedArgs a;
    uintptr_t o = 0;
    if (!heal || !out || ntargets == 0)
        return -EINVAL;
    if (int rc = pack_verified(d, check, check_brick, bad, a, &o))
        return rc;
    /* the inputs and the targets are different bricks of at most 31, so the
     * table has at most 31 - k rows: 72 words at k = 13 */
    if (a.k + a.rows + ntargets >= ECD_MAX_ROWS)
        return -EINVAL;
    a.m = ntargets;
    pack_rows(a.coef, 0, a.rows, a.k, a.kw, d->pat + a.k);
    pack_rows(a.coef, a.rows, ntargets, a.k, a.kw, heal);
    for (u32 j = 0; j < ntargets; ++j) {
        if (!out[j])
            return -EINVAL;
        a.out[j] = static_cast<uint8_t *>(out[j]);
    }
    return launch_scrub_tile(s, a, a.k, a.rows, a.nstripes, o, 1, "launch_heal_verified",
                             [](auto c) {
        using C = decltype(c);
        return &ec_heal_verified_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------- fused heal with per-group patterns */

namespace {

/* the instantiation of ec_heal_mixed_n for k, where the patterns are and the
 * staging policy: the K buckets and wave counts of ecdk_decode_clip */
template <bool PG, int LA>
int launch_heal_mixed(hipStream_t s, const HealMixedArgs &a, u32 g)
{
    const size_t lds = scrub_tile_lds(a.k, 0);
    if (a.k <= 4)
        hipLaunchKernelGGL((ec_heal_mixed_n<4, 4, PG, LA>), dim3(g), dim3(4 * 64), lds, s, a);
    else if (a.k <= 8)
        hipLaunchKernelGGL((ec_heal_mixed_n<8, 8, PG, LA>), dim3(g), dim3(8 * 64), lds, s, a);
    else
        hipLaunchKernelGGL((ec_heal_mixed_n<16, 8, PG, LA>), dim3(g), dim3(8 * 64), lds, s, a);
    return launch_ok("launch_heal_mixed");
}

} // namespace

/* pats: npatterns packed patterns of k + 1 + mmax + mmax * k bytes each:
 * src[k], m, dst[mmax], coef[mmax][k] (m <= mmax rows used).  frags: 32
 * pointers indexed by brick.  One launch; the patterns travel in the kernel
 * arguments when they fit and in a table of the pattern cache when not. */
int ecdk_heal_mixed(hipStream_t s, uint32_t k, uint64_t nstripes, const uint8_t *group_pattern,
                    uint32_t group_shift, uint32_t npatterns, uint32_t mmax, const uint8_t *pats,
                    void *const *frags)
{
    static_assert(sizeof(HealMixedArgs) <= 2048, "the arguments keep to 2 KiB");
    static_assert(offsetof(HealMixedArgs, pat) == 304, "the header the tests count");
    HealMixedArgs a;
    if (k == 0 || k > ECD_MAX_K || !group_pattern || group_shift < 2 || group_shift > 40 ||
        npatterns == 0 || npatterns > ECD_MAX_PATTERNS || mmax >= 16 || !pats || !frags)
        return -EINVAL;
    const uint64_t g = (nstripes + kScrubT - 1) / kScrubT;
    if (g == 0 || mmax == 0)
        return 0;               /* no stripe, or no pattern with a target */
    if (g > 0x7fffffffull)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = k;
    a.kw = (k + 3) / 4;
    a.nstripes = nstripes;
    a.group_pattern = group_pattern;
    a.group_shift = group_shift;
    a.npatterns = npatterns;
    a.dw = (mmax + 3) / 4;
    a.pwords = a.kw + 1 + a.dw + mmax * a.kw;
    uintptr_t align = 0;
    for (u32 i = 0; i < ECD_MAX_ROWS; ++i) {
        a.frag[i] = static_cast<uint8_t *>(frags[i]);
        align |= (uintptr_t)frags[i];
    }
    const size_t pbytes = (size_t)k + 1 + mmax + (size_t)mmax * k;
    const size_t nw = (size_t)a.pwords * npatterns;
    const bool pg = nw > (size_t)kHealMixedPatWords;
    std::vector<u32> table(pg ? nw : 0, 0u);
    u32 *words = pg ? table.data() : a.pat;
    for (u32 q = 0; q < npatterns; ++q) {
        const uint8_t *src = pats + q * pbytes;
        uint8_t *dst = reinterpret_cast<uint8_t *>(words + (size_t)q * a.pwords);
        const u32 m = src[k];
        if (m > mmax)
            return -EINVAL;
        for (u32 p = 0; p < k; ++p)
            if (src[p] >= ECD_MAX_ROWS || (m && !frags[src[p]]))
                return -EINVAL;
        memcpy(dst, src, k);
        dst[4 * a.kw] = (uint8_t)m;
        for (u32 j = 0; j < m; ++j) {
            if (src[k + 1 + j] >= ECD_MAX_ROWS || !frags[src[k + 1 + j]])
                return -EINVAL;
            dst[4 * (a.kw + 1) + j] = src[k + 1 + j];
            memcpy(dst + 4 * (a.kw + 1 + a.dw + (size_t)j * a.kw), src + k + 1 + mmax + j * k, k);
        }
    }
    u32 *tab = nullptr;
    PatTableCache::Ref ref;
    int rc = 0;
    if (pg) {
        rc = pat_tables().acquire(s, table, ref);
        if (rc == 0) {
            a.patg = ref.ptr;
        } else if (rc == -EBUSY) {
            /* every cache entry in use: a table of this call's own */
            if (const hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&tab), nw * 4, s)) {
                (void)hip_ok(e, "hipMallocAsync(per-call pattern table)");
                return -ENOMEM;
            }
            a.patg = tab;
            rc = enqueue_upload(s, table, tab);
        }
    }
    if (rc == 0) {
        /* the staging policy of launch_scrub_tile, by the bytes the call reads */
        const bool nt = nt_staging(nstripes * k * ECD_CHUNK) && (align & 15u) == 0;
        if (pg)
            rc = nt ? launch_heal_mixed<true, kLdsDmaNT>(s, a, (u32)g)
                    : launch_heal_mixed<true, kLdsDmaDefault>(s, a, (u32)g);
        else
            rc = nt ? launch_heal_mixed<false, kLdsDmaNT>(s, a, (u32)g)
                    : launch_heal_mixed<false, kLdsDmaDefault>(s, a, (u32)g);
    }
    if (ref.slot >= 0)
        (void)pat_tables().release(ref, s);   /* a failure drained s: the call stands */
    if (tab) {
        const int frc = hip_ok(hipFreeAsync(tab, s), "hipFreeAsync(per-call pattern table)");
        rc = rc ? rc : frc;
    }
    return rc;
}

/* ---------------------------------------- fused heal over a table of extents */

namespace {

/* the instantiation of ec_heal_extents_n, as launch_heal_mixed */
template <bool PG, int LA>
int launch_heal_extents(hipStream_t s, const HealExtentsArgs &a, u32 g)
{
    const size_t lds = scrub_tile_lds(a.k, 0);
    if (a.k <= 4)
        hipLaunchKernelGGL((ec_heal_extents_n<4, 4, PG, LA>), dim3(g), dim3(4 * 64), lds, s, a);
    else if (a.k <= 8)
        hipLaunchKernelGGL((ec_heal_extents_n<8, 8, PG, LA>), dim3(g), dim3(8 * 64), lds, s, a);
    else
        hipLaunchKernelGGL((ec_heal_extents_n<16, 8, PG, LA>), dim3(g), dim3(8 * 64), lds, s, a);
    return launch_ok("launch_heal_extents");
}

} // namespace

/* pats: as for ecdk_heal_mixed.  One launch of ntiles blocks; the patterns
 * travel in the kernel arguments when they fit and in a table of the pattern
 * cache when not.  The fragment addresses stay in the caller's table. */
int ecdk_heal_extents(hipStream_t s, uint32_t k, uint64_t nextents, uint64_t ntiles,
                      const void *ext_dev, uint32_t npatterns, uint32_t mmax,
                      const uint8_t *pats, uint64_t in_bytes, int aligned)
{
    static_assert(sizeof(HealExtentsArgs) <= 2048, "the arguments keep to 2 KiB");
    static_assert(offsetof(HealExtentsArgs, pat) == 40, "the header the tests count");
    HealExtentsArgs a;
    if (k == 0 || k > ECD_MAX_K || !ext_dev || ((uintptr_t)ext_dev & 7u) || npatterns == 0 ||
        npatterns > ECD_MAX_PATTERNS || mmax >= 16 || !pats || nextents > ntiles ||
        ntiles > 0x7fffffffull)
        return -EINVAL;
    if (nextents == 0 || mmax == 0)
        return 0;               /* no extent, or no pattern with a target */
    memset(&a, 0, sizeof(a));
    a.ext = static_cast<const uint8_t *>(ext_dev);
    a.nextents = (u32)nextents;
    a.k = k;
    a.kw = (k + 3) / 4;
    a.npatterns = npatterns;
    a.dw = (mmax + 3) / 4;
    a.pwords = a.kw + 1 + a.dw + mmax * a.kw;
    const size_t pbytes = (size_t)k + 1 + mmax + (size_t)mmax * k;
    const size_t nw = (size_t)a.pwords * npatterns;
    const bool pg = nw > (size_t)kHealExtentsPatWords;
    std::vector<u32> table(pg ? nw : 0, 0u);
    u32 *words = pg ? table.data() : a.pat;
    for (u32 q = 0; q < npatterns; ++q) {
        const uint8_t *src = pats + q * pbytes;
        uint8_t *dst = reinterpret_cast<uint8_t *>(words + (size_t)q * a.pwords);
        const u32 m = src[k];
        if (m > mmax)
            return -EINVAL;
        for (u32 p = 0; p < k; ++p)
            if (src[p] >= ECD_MAX_ROWS)
                return -EINVAL;
        memcpy(dst, src, k);
        dst[4 * a.kw] = (uint8_t)m;
        for (u32 j = 0; j < m; ++j) {
            if (src[k + 1 + j] >= ECD_MAX_ROWS)
                return -EINVAL;
            dst[4 * (a.kw + 1) + j] = src[k + 1 + j];
            memcpy(dst + 4 * (a.kw + 1 + a.dw + (size_t)j * a.kw), src + k + 1 + mmax + j * k, k);
        }
    }
    u32 *tab = nullptr;
    PatTableCache::Ref ref;
    int rc = 0;
    if (pg) {
        rc = pat_tables().acquire(s, table, ref);
        if (rc == 0) {
            a.patg = ref.ptr;
        } else if (rc == -EBUSY) {
            /* every cache entry in use: a table of this call's own */
            if (const hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&tab), nw * 4, s)) {
                (void)hip_ok(e, "hipMallocAsync(per-call pattern table)");
                return -ENOMEM;
            }
            a.patg = tab;
            rc = enqueue_upload(s, table, tab);
        }
    }
    if (rc == 0) {
        /* the staging policy of ecdk_heal_mixed; a caller that cannot tell
         * where its fragments lie gets the default policy */
        const bool nt = aligned && nt_staging(in_bytes);
        if (pg)
            rc = nt ? launch_heal_extents<true, kLdsDmaNT>(s, a, (u32)ntiles)
                    : launch_heal_extents<true, kLdsDmaDefault>(s, a, (u32)ntiles);
        else
            rc = nt ? launch_heal_extents<false, kLdsDmaNT>(s, a, (u32)ntiles)
                    : launch_heal_extents<false, kLdsDmaDefault>(s, a, (u32)ntiles);
    }
    if (ref.slot >= 0)
        (void)pat_tables().release(ref, s);   /* a failure drained s: the call stands */
    if (tab) {
        const int frc = hip_ok(hipFreeAsync(tab, s), "hipFreeAsync(per-call pattern table)");
        rc = rc ? rc : frc;
    }
    return rc;
}

/* ------------------------------------------- ranged read: the edge stripes */

/* in: the k fragments (device memory, any byte alignment); inv: k x k bytes,
 * the decode matrix of those fragments; edge[0 .. nedges): the one or two
 * stripes to decode and the bytes of each to store.  One launch of one block
 * per edge; inv and the clips travel in the kernel arguments. */
int ecdk_decode_clip(hipStream_t s, uint32_t k, const void *const *in, const uint8_t *inv,
                     uint32_t nedges, const ecdk_clip_edge_t *edge)
{
    static_assert(sizeof(DecodeClipArgs) <= 2048, "inv must fit the kernel arguments");
    DecodeClipArgs a;
    if (k == 0 || k > ECD_MAX_K || !in || !inv || !edge || nedges == 0 || nedges > 2)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = k;
    a.kw = (k + 3) / 4;
    for (u32 p = 0; p < k; ++p) {
        if (!in[p])
            return -EINVAL;
        a.in[p] = static_cast<const uint8_t *>(in[p]);
    }
    for (u32 e = 0; e < nedges; ++e) {
        if (edge[e].lo >= edge[e].hi || edge[e].hi > k * ECD_CHUNK)
            return -EINVAL;
        a.t[e] = edge[e].t;
        a.base[e] = edge[e].base;
        a.lo[e] = edge[e].lo;
        a.hi[e] = edge[e].hi;
    }
    pack_rows(a.inv, 0, k, k, a.kw, inv);
    /* one stripe in slot 0 of a scrub tile: at most 32 KiB */
    const size_t lds = scrub_tile_lds(k, 0);
    /* the k -> K buckets and wave counts of launch_scrub_tile */
    if (k <= 4)
        hipLaunchKernelGGL((ec_decode_clip<4, 4>), dim3(nedges), dim3(4 * 64), lds, s, a);
    else if (k <= 8)
        hipLaunchKernelGGL((ec_decode_clip<8, 8>), dim3(nedges), dim3(8 * 64), lds, s, a);
    else
        hipLaunchKernelGGL((ec_decode_clip<16, 8>), dim3(nedges), dim3(8 * 64), lds, s, a);
    return launch_ok("launch_decode_clip");
}

/* ----------------------------------------- ranged write: the edge stripes */

int ecdk_encode_any_alignment(uint32_t k, uint32_t n)
{
    return enc_tiles() && ecdk_has_vander(k, n) && k != 2;
}

/* edge[0 .. nedges): the one or two stripes to merge and encode.  One launch
 * of one block per edge; the old chunk pointers, inv, the encode matrix, the
 * fragment pointers and the clips travel in the kernel arguments. */
int ecdk_rmw_edge(hipStream_t s, uint32_t k, uint32_t n, const uint8_t *inv, const uint8_t *enc,
                  const uint8_t *user0, void *const *out, uint32_t nedges,
                  const ecdk_rmw_edge_t *edge)
{
    static_assert(sizeof(RmwEdgeArgs) <= 2048, "the tables must fit the kernel arguments");
    RmwEdgeArgs a;
    if (k == 0 || k > ECD_MAX_K || n == 0 || n >= ECD_MAX_ROWS || !enc || !out || !edge ||
        nedges == 0 || nedges > 2)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = k;
    a.kw = (k + 3) / 4;
    a.n = n;
    a.user = user0;
    for (u32 i = 0; i < n; ++i) {
        if (!out[i])
            return -EINVAL;
        a.out[i] = static_cast<uint8_t *>(out[i]);
    }
    bool any_old = false;
    for (u32 e = 0; e < nedges; ++e) {
        if (edge[e].lo >= edge[e].hi || edge[e].hi > k * ECD_CHUNK)
            return -EINVAL;
        a.t[e] = edge[e].t;
        a.lo[e] = edge[e].lo;
        a.hi[e] = edge[e].hi;
        if (!edge[e].old)
            continue;
        any_old = true;
        for (u32 p = 0; p < k; ++p) {
            if (!edge[e].old[p])
                return -EINVAL;
            a.old[e * ECD_MAX_K + p] = static_cast<const uint8_t *>(edge[e].old[p]);
        }
    }
    if (any_old) {
        if (!inv)
            return -EINVAL;
        pack_rows(a.inv, 0, k, k, a.kw, inv);
    }
    pack_rows(a.enc, 0, n, k, a.kw, enc);
    /* the old chunks in slot 0 and the merged stripe in slot 1 of one scrub
     * tile: at most 32 KiB */
    const size_t lds = scrub_tile_lds(k, 0);
    /* the k -> K buckets and wave counts of ecdk_decode_clip */
    if (k <= 4)
        hipLaunchKernelGGL((ec_rmw_edge<4, 4>), dim3(nedges), dim3(4 * 64), lds, s, a);
    else if (k <= 8)
        hipLaunchKernelGGL((ec_rmw_edge<8, 8>), dim3(nedges), dim3(8 * 64), lds, s, a);
    else
        hipLaunchKernelGGL((ec_rmw_edge<16, 8>), dim3(nedges), dim3(8 * 64), lds, s, a);
    return launch_ok("launch_rmw_edge");
}

/* ------------------------------------------ locating up to two bricks */

/* The arguments of ec_locate2_n from what ecdk_locate2 is given: pack_locate,
 * then ratio1, the pairs' inverses and their positions. */
static int pack_locate2(const ecd_combine_desc_t *d, const void *const *check,
                        const uint8_t *check_brick, const uint8_t *basis_brick,
                        const uint8_t *ratio, const uint8_t *ratio1, const uint8_t *pair_inv,
                        uint32_t *loc, Locate2Args &a, uintptr_t *align)
{
    if (!ratio1 || !pair_inv || d->rows < 4)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    if (int rc = pack_locate(d, check, check_brick, basis_brick, ratio, loc, a.l, align))
        return rc;
    const u32 k = a.l.k, kw = a.l.kw;
    for (u32 r = 2; r < a.l.rows; ++r)
        for (u32 p = 0; p < k; ++p)
            a.ratio1[(r - 2) * kw + (p >> 2)] |= (u32)ratio1[(r - 2) * k + p] << ((p & 3u) * 8u);
    u32 i = 0;
    for (u32 p = 0; p < k; ++p)
        for (u32 q = p + 1; q < k; ++q, ++i) {
            memcpy(&a.pinv[i], pair_inv + 4u * i, 4);
            a.ppq[i >> 2] |= (p << 4 | q) << ((i & 3u) * 8u);
        }
    a.npairs = i;
    return 0;
}

/* As ecdk_locate, with at least four rows.  ratio1: (rows - 2) x k bytes,
 * coefficient of row r over that of row 1, for r >= 2; pair_inv: 4 bytes
 * {a, b, c, d} per basis pair p < q in lexicographic order, the inverse of
 * rows 0 and 1 of columns p and q (ec_kernels_impl.h, Locate2Args).  Every
 * table travels in the kernel arguments: nothing is uploaded. */
int ecdk_locate2(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                 const uint8_t *check_brick, const uint8_t *basis_brick, const uint8_t *ratio,
                 const uint8_t *ratio1, const uint8_t *pair_inv, uint32_t *loc)
{
    static_assert(sizeof(Locate2Args) <= 2048, "the tables must fit the kernel arguments");
    Locate2Args a;
    uintptr_t o = 0;
    if (int rc = pack_locate2(d, check, check_brick, basis_brick, ratio, ratio1, pair_inv, loc, a,
                              &o))
        return rc;
    return launch_scrub_tile(s, a, a.l.k, a.l.rows, a.l.nstripes, o, 3, "launch_locate2",
                             [](auto c) {
        using C = decltype(c);
        return &ec_locate2_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------- a read that corrects up to two chunks */

/* As ecdk_locate2, then inv: k x k bytes, the decode matrix of the basis (row
 * j gives output chunk j); ginv: 2 x k bytes, 1 / coefficient of row 0, then
 * of row 1; out: nstripes * k * 512 device bytes at any alignment.  Every
 * table travels in the kernel arguments: nothing is uploaded. */
int ecdk_decode_checked2(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                         const uint8_t *check_brick, const uint8_t *basis_brick,
                         const uint8_t *ratio, const uint8_t *ratio1, const uint8_t *pair_inv,
                         const uint8_t *inv, const uint8_t *ginv, void *out, uint32_t *loc)
{
    static_assert(sizeof(DecodeChecked2Args) <= 2048, "the tables must fit the kernel arguments");
    DecodeChecked2Args a;
    uintptr_t o = 0;
    if (!inv || !ginv || !out)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    if (int rc = pack_locate2(d, check, check_brick, basis_brick, ratio, ratio1, pair_inv, loc,
                              a.l2, &o))
        return rc;
    const u32 k = a.l2.l.k, kw = a.l2.l.kw;
    a.out = static_cast<uint8_t *>(out);
    for (u32 p = 0; p < k; ++p) {
        if (ginv[p] == 0 || ginv[k + p] == 0)
            return -EINVAL;
        a.bmask |= 1u << basis_brick[p];
        a.ginv[p >> 2] |= (u32)ginv[p] << ((p & 3u) * 8u);
        a.ginv[ECD_MAX_K / 4 + (p >> 2)] |= (u32)ginv[k + p] << ((p & 3u) * 8u);
        for (u32 j = 0; j < k; ++j)
            a.inv[j * kw + (p >> 2)] |= (u32)inv[j * k + p] << ((p & 3u) * 8u);
    }
    return launch_scrub_tile(s, a, k, a.l2.l.rows, a.l2.l.nstripes, o, 3, "launch_decode_checked2",
                             [](auto c) {
        using C = decltype(c);
        return &ec_decode_checked2_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------- a heal that corrects up to two chunks */

/* As ecdk_locate2, then ntargets: the m targets; heal: m x k bytes, the heal
 * matrix of the targets from the basis (row j gives the chunk of target j);
 * ginv: 2 x k bytes, 1 / coefficient of row 0, then of row 1; out: the m
 * target fragments, nstripes * 512 device bytes each at any alignment.  Every
 * table travels in the kernel arguments: nothing is uploaded.  The target
 * pointers take the slots of the input list behind the k + rows inputs
 * (HealChecked2Args): a geometry whose inputs and targets are not different
 * bricks of at most 31 does not fit and is -EINVAL. */
int ecdk_heal_checked2(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                       const uint8_t *check_brick, const uint8_t *basis_brick,
                       const uint8_t *ratio, const uint8_t *ratio1, const uint8_t *pair_inv,
                       uint32_t ntargets, const uint8_t *heal, const uint8_t *ginv,
                       void *const *out, uint32_t *loc)
{
    static_assert(sizeof(HealChecked2Args) <= 2048, "the tables must fit the kernel arguments");
    HealChecked2Args a;
    uintptr_t o = 0;
    if (!heal || !ginv || !out || ntargets == 0)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    if (int rc = pack_locate2(d, check, check_brick, basis_brick, ratio, ratio1, pair_inv, loc,
                              a.l2, &o))
        return rc;
    LocateArgs &l = a.l2.l;
    const u32 k = l.k, kw = l.kw, ni = k + l.rows;
    if (ni + ntargets >= ECD_MAX_ROWS || kw * ntargets > kLocateWords)
        return -EINVAL;
    a.m = ntargets;
    for (u32 j = 0; j < ntargets; ++j) {
        if (!out[j])
            return -EINVAL;
        l.in[ni + j] = static_cast<const uint8_t *>(out[j]);
        for (u32 p = 0; p < k; ++p)
            a.heal[j * kw + (p >> 2)] |= (u32)heal[j * k + p] << ((p & 3u) * 8u);
    }
    for (u32 p = 0; p < k; ++p) {
        if (ginv[p] == 0 || ginv[k + p] == 0)
            return -EINVAL;
        a.bmask |= 1u << basis_brick[p];
        a.ginv[p >> 2] |= (u32)ginv[p] << ((p & 3u) * 8u);
        a.ginv[ECD_MAX_K / 4 + (p >> 2)] |= (u32)ginv[k + p] << ((p & 3u) * 8u);
    }
    return launch_scrub_tile(s, a, k, l.rows, l.nstripes, o, 3, "launch_heal_checked2",
                             [](auto c) {
        using C = decltype(c);
        return &ec_heal_checked2_n<C::K, C::NW, C::LA>;
    });
}

/* ------------------------------------------- repairing the named chunks */

static int cu_count();

/* k, nstripes: the geometry; frags: by brick, read for the bits of avail;
 * bset: the k + 1 brick indices of the basis and c0, ascending; coef[i * k +
 * p]: coefficient of input p of B_i for every brick i of avail; loc: nstripes
 * device dwords, read only. */
int ecdk_repair(hipStream_t s, uint32_t k, uint64_t nstripes, void *const *frags, uint32_t avail,
                const uint8_t *bset, const uint8_t *coef, const uint32_t *loc)
{
    RepairArgs a;
    if (k == 0 || k > ECD_MAX_K || !frags || !bset || !coef || !loc || ((uintptr_t)loc & 3u) ||
        (avail >> 31) != 0)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = k;
    a.avail = avail;
    a.nstripes = nstripes;
    a.loc = loc;
    /* bset is the k + 1 lowest bricks of avail in ascending order */
    u32 rest = avail;
    for (u32 p = 0; p <= k; ++p) {
        if (rest == 0 || bset[p] != (u32)__builtin_ctz(rest))
            return -EINVAL;
        rest &= rest - 1u;
        if (p < k)
            a.bmask |= 1u << bset[p];
        a.bset[p >> 2] |= (u32)bset[p] << ((p & 3u) * 8u);
    }
    for (u32 i = 0; i < 31; ++i) {
        if (!((avail >> i) & 1u))
            continue;
        if (!frags[i])
            return -EINVAL;
        a.frag[i] = static_cast<uint8_t *>(frags[i]);
        for (u32 p = 0; p < k; ++p)
            a.coef[i][p >> 2] |= (u32)coef[i * k + p] << ((p & 3u) * 8u);
    }
    if (nstripes == 0)
        return 0;
    /* one lane per loc word; a few blocks per CU stride over the rest */
    uint64_t g = (nstripes + kRepairThreads - 1) / kRepairThreads;
    const uint64_t cap = (uint64_t)cu_count() * 8u;
    if (g > cap)
        g = cap;
    hipLaunchKernelGGL(ec_repair_n, dim3((u32)g), dim3(kRepairThreads), 0, s, a);
    return launch_ok("launch_repair");
}

/* k, nstripes, frags, avail, loc: as ecdk_repair, with at least k + 2 bits in
 * avail; rows = those bits less k; g: rows x k bytes, the heal matrix of the
 * check bricks (the bricks of avail after its k lowest, ascending) from the k
 * lowest; ginv: 2 x k bytes, 1 / g of its rows 0 and 1; pair_inv: as
 * ecdk_locate2.  Every table travels in the kernel arguments: nothing is
 * uploaded. */
int ecdk_repair2(hipStream_t s, uint32_t k, uint64_t nstripes, void *const *frags, uint32_t avail,
                 uint32_t rows, const uint8_t *g, const uint8_t *ginv, const uint8_t *pair_inv,
                 const uint32_t *loc)
{
    static_assert(sizeof(Repair2Args) <= 2048, "the tables must fit the kernel arguments");
    Repair2Args a;
    if (k == 0 || k > ECD_MAX_K || !frags || !g || !ginv || !pair_inv || !loc ||
        ((uintptr_t)loc & 3u) || (avail >> 31) != 0 || rows < 2 ||
        (u32)__builtin_popcount(avail) != k + rows)
        return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.k = k;
    a.kw = (k + 3) / 4;
    a.avail = avail;
    a.nstripes = nstripes;
    a.loc = loc;
    if (a.kw * rows > kRepair2Words)
        return -EINVAL;
    u32 nb = 0, nr = 0;
    for (u32 i = 0; i < 31; ++i) {
        if (!((avail >> i) & 1u))
            continue;
        if (!frags[i])
            return -EINVAL;
        a.frag[i] = static_cast<uint8_t *>(frags[i]);
        if (nb < k) {
            a.bmask |= 1u << i;
            a.bbrick[nb >> 2] |= i << ((nb & 3u) * 8u);
            ++nb;
        } else {
            a.cbrick[nr >> 2] |= i << ((nr & 3u) * 8u);
            ++nr;
        }
    }
    for (u32 r = 0; r < rows; ++r)
        for (u32 p = 0; p < k; ++p) {
            const u32 c = g[r * k + p];
            if (c == 0)                 /* the code is MDS */
                return -EINVAL;
            a.g[r * a.kw + (p >> 2)] |= c << ((p & 3u) * 8u);
            if (r < 2)
                a.ginv[r][p >> 2] |= (u32)ginv[r * k + p] << ((p & 3u) * 8u);
        }
    memcpy(a.pinv, pair_inv, 4u * (k * (k - 1u) / 2u));
    if (nstripes == 0)
        return 0;
    /* one lane per loc word; a few blocks per CU stride over the rest */
    uint64_t grid = (nstripes + kRepairThreads - 1) / kRepairThreads;
    const uint64_t cap = (uint64_t)cu_count() * 8u;
    if (grid > cap)
        grid = cap;
    hipLaunchKernelGGL(ec_repair2_n, dim3((u32)grid), dim3(kRepairThreads), 0, s, a);
    return launch_ok("launch_repair2");
}

/* loc: nstripes device dwords, read only; report: 34 device words; idx / val:
 * cap entries each (idx may be NULL when cap == 0, val always); work:
 * ECD_REPORT_WORK(nstripes) device bytes.  Count, scan and, when anything can
 * be listed, scatter, back to back on s. */
int ecdk_scrub_report(hipStream_t s, uint64_t nstripes, const uint32_t *loc, uint64_t *report,
                      uint64_t cap, uint64_t *idx, uint32_t *val, void *work)
{
    ReportArgs a;
    if (!loc || !report || ((uintptr_t)loc & 3u) || ((uintptr_t)val & 3u) ||
        (((uintptr_t)report | (uintptr_t)idx | (uintptr_t)work) & 7u) || (cap > 0 && !idx) ||
        nstripes > ECD_REPORT_MAX_STRIPES)
        return -EINVAL;
    if (nstripes == 0)
        return 0;
    if (!work)
        return -EINVAL;
    a.loc = loc;
    a.nstripes = nstripes;
    a.ntiles = ECD_REPORT_TILES(nstripes);
    a.cap = cap;
    a.off = static_cast<uint64_t *>(work);
    a.part = reinterpret_cast<u32 *>(a.off + a.ntiles);
    a.report = report;
    a.idx = idx;
    a.val = val;
    /* a block per tile; a few blocks per CU stride over the rest */
    uint64_t g = a.ntiles;
    const uint64_t most = (uint64_t)cu_count() * 8u;
    if (g > most)
        g = most;
    hipLaunchKernelGGL(ec_report_count, dim3((u32)g), dim3(kReportThreads), 0, s, a);
    int rc = launch_ok("launch_report_count");
    if (rc)
        return rc;
    hipLaunchKernelGGL(ec_report_scan, dim3(1), dim3(kReportThreads), 0, s, a);
    rc = launch_ok("launch_report_scan");
    if (rc || cap == 0)
        return rc;
    hipLaunchKernelGGL(ec_report_scatter, dim3((u32)g), dim3(kReportThreads), 0, s, a);
    return launch_ok("launch_report_scatter");
}

/* Host-buffer combines with k <= 8 run the persistent double-buffered
 * ec_combine_zc_db (default since r04; EC_MI355X_ZCDB=0 keeps one tile per
 * block, ec_combine_zc, for A/B runs).  Pinned 8+4 / 4+2 decodes, same
 * process alternating (tools/zc_sizes.py, profiles/r03/r03af_zcsizes.log), us
 * per call one tile per block -> double-buffered: 4 MiB 177-197 -> 174 / 174
 * -> 162, 16 MiB 572 -> 518-526 / 554-568 -> 530, 64 MiB 1765-1790 -> 1757 /
 * 1760 -> 1674-1683, 256 MiB 6350 -> 6245 / 6390 -> 6178; never slower,
 * bit-exact in the knob test (ZCDB=0 and =1: decode, heal and mixed host
 * calls) and at every size probed. */
static bool zc_double_buffered()
{
    static const bool v = [] {
        const char *e = getenv("EC_MI355X_ZCDB");
        return !(e && *e == '0');
    }();
    return v;
}

/* LDS of one gfx950 CU (MI355X_MICROARCH.md): the largest block LDS */
constexpr size_t kLdsPerCu = 160u << 10;

/* A/B knobs of the persistent zero-copy combine's grid (read once):
 * EC_ZC_TPB = fixed tiles per block (r03's rule was 4), EC_ZC_INFLIGHT_KB =
 * the input bytes one round of tiles keeps in flight (default 2048). */
static uint64_t zc_env(const char *name, long lo, long hi, long dflt)
{
    const char *e = getenv(name);
    const long v = e ? atol(e) : dflt;
    return (uint64_t)(v >= lo && v <= hi ? v : dflt);
}

static uint64_t zc_fixed_tpb()
{
    static const uint64_t v = zc_env("EC_ZC_TPB", 1, 1024, 0);
    return v;
}

static uint64_t zc_inflight_bytes()
{
    static const uint64_t v = zc_env("EC_ZC_INFLIGHT_KB", 64, 1 << 20, 2048) << 10;
    return v;
}

/* CUs of the current device, queried once per device */
static int cu_count()
{
    static std::atomic<int> cus[64];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0)
        return 256;
    if (dev < 64 && (n = cus[dev].load(std::memory_order_relaxed)) > 0)
        return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        return 256;
    if (dev < 64)
        cus[dev].store(n, std::memory_order_relaxed);
    return n;
}

/* k > 8 with >= 2048 stripes (16 MiB of a 16+4 call): the 4-stripe tiles of
 * ec_combine_zc_db, two input tiles and the output tile in LDS */
static bool zc_db4_fits(const ecd_combine_desc_t *d)
{
    const size_t lds_db4 = (size_t)(2 * d->k + d->rows) * 4 * ECD_CHUNK + 8 * ECD_MAX_ROWS;
    return d->k > 8 && d->nstripes >= 2048 && lds_db4 <= (128u << 10) + 8 * ECD_MAX_ROWS;
}

/* Host-buffer path: every buffer is pinned host memory read / written over
 * PCIe (ec_device.hip run_pipeline), so the zero-copy combine with whole
 * 1 KiB request runs; default (not non-temporal) stores there, which cost
 * 12 % on the link (profiles/kbench_r01_zc.log). */
int ecdk_combine_host(hipStream_t s, const ecd_combine_desc_t *d)
{
    CombineArgs a;
    int rc = ecdk_pack_args(d, &a);
    /* more than 32 inputs + rows fit only the 4-stripe double-buffered tile
     * below (a 16+4 encode as a combine: 16 inputs, 20 rows, r06) */
    const bool wide = d->k + d->rows > 32 && !(zc_double_buffered() && zc_db4_fits(d));
    if (rc == -E2BIG || (rc == 0 && (wide || (d->group_pattern && d->group_shift < 3))))
        return combine_any<false>(s, d);   /* device pattern table / LDS limit / small groups */
    if (rc)
        return rc;
    const uint64_t g = (a.nstripes + 7) / 8;
    if (g == 0)
        return 0;
    if (g > 0x7fffffffull)
        return -EINVAL;
    const size_t lds = (size_t)(d->k + d->rows) * 8 * ECD_CHUNK;
    constexpr int NW = 8;
    const size_t lds_db = (size_t)(2 * d->k + d->rows) * 8 * ECD_CHUNK + 8 * ECD_MAX_ROWS;
    const bool db16 = d->k > 8 && lds_db <= kLdsPerCu;   /* 16+4 heal / row-masked encode */
    /* the 16-row decode of a 16+4 volume: 4-stripe tiles (half the LDS).
     * Pinned 16+4 decodes (profiles/r04/r04s_zcheal.log, one tile per block
     * -> this): 16 MiB 570-576 -> 525 us, 64 MiB 1793-1797 -> 1639; at 4 MiB
     * 172 -> 177, so calls below 2048 stripes (16 MiB) keep ec_combine_zc */
    const size_t lds_db4 = (size_t)(2 * d->k + d->rows) * 4 * ECD_CHUNK + 8 * ECD_MAX_ROWS;
    const bool db16t4 = !db16 && zc_db4_fits(d);
    if (zc_double_buffered() && db16t4) {
        const uint64_t g4 = (a.nstripes + 3) / 4;
        const uint64_t tpb = zc_fixed_tpb();
        const uint64_t want = tpb ? g4 / tpb
                                  : std::min<uint64_t>(g4 / 2, zc_inflight_bytes() /
                                                                   ((uint64_t)d->k * 4 * ECD_CHUNK));
        const uint64_t gdb = std::min<uint64_t>(std::max<uint64_t>(want, 1), (uint64_t)cu_count());
        const void *kern = a.group_pattern ? (const void *)ec_combine_zc_db<16, NW, true, 4>
                                           : (const void *)ec_combine_zc_db<16, NW, false, 4>;
        if (lds_db4 > (64u << 10) &&
            ensure_lds_limit(kern, (int)((128u << 10) + 8 * ECD_MAX_ROWS)) != 0)
            return -EIO;
        void *args[] = {&a};
        return hip_ok(hipLaunchKernel(kern, dim3((u32)gdb), dim3(NW * 64), args, lds_db4, s),
                      "hipLaunchKernel(ec_combine_zc_db)");
    }
    if (zc_double_buffered() &&
        ((d->k <= 8 && lds_db <= (128u << 10) + 8 * ECD_MAX_ROWS) || db16)) {
        /* persistent, at most one block per CU, >= 2 tiles per block so its
         * reads of tile i + 1 and writes of tile i overlap, and as many
         * blocks as keep ~2 MiB of input in flight: more only queue on the
         * link, fewer leave it idle while each block's first tile lands.
         * Pinned 8+4 / 4+2 calls, us (decode; profiles/r04/r04m_zctpb.log,
         * r03's 4 tiles per block -> this): 8+4 1 MiB 81 -> 69, 4 MiB 173
         * -> 164, 16 MiB 516 -> 505; 4+2 16 MiB 533 -> 489. */
        const uint64_t tpb = zc_fixed_tpb();
        const uint64_t want =
            tpb ? g / tpb : std::min<uint64_t>(g / 2, zc_inflight_bytes() / ((uint64_t)d->k * 8 * ECD_CHUNK));
        const uint64_t gdb = std::min<uint64_t>(std::max<uint64_t>(want, 1), (uint64_t)cu_count());
        const void *kern =
            db16 ? (a.group_pattern ? (const void *)ec_combine_zc_db<16, NW, true>
                                    : (const void *)ec_combine_zc_db<16, NW, false>)
            : d->k <= 4 ? (a.group_pattern ? (const void *)ec_combine_zc_db<4, NW, true>
                                           : (const void *)ec_combine_zc_db<4, NW, false>)
                        : (a.group_pattern ? (const void *)ec_combine_zc_db<8, NW, true>
                                           : (const void *)ec_combine_zc_db<8, NW, false>);
        if (lds_db > (64u << 10) &&
            ensure_lds_limit(kern, db16 ? (int)kLdsPerCu : (int)((128u << 10) + 8 * ECD_MAX_ROWS)) != 0)
            return -EIO;
        void *args[] = {&a};
        return hip_ok(hipLaunchKernel(kern, dim3((u32)gdb), dim3(NW * 64), args, lds_db, s),
                      "hipLaunchKernel(ec_combine_zc_db)");
    }
    if (d->k <= 4) {
        if (a.group_pattern)
            hipLaunchKernelGGL((ec_combine_zc<4, NW, true>), dim3((u32)g), dim3(NW * 64), lds, s, a);
        else
            hipLaunchKernelGGL((ec_combine_zc<4, NW, false>), dim3((u32)g), dim3(NW * 64), lds, s, a);
    } else if (d->k <= 8) {
        if (a.group_pattern)
            hipLaunchKernelGGL((ec_combine_zc<8, NW, true>), dim3((u32)g), dim3(NW * 64), lds, s, a);
        else
            hipLaunchKernelGGL((ec_combine_zc<8, NW, false>), dim3((u32)g), dim3(NW * 64), lds, s, a);
    } else {
        /* up to (16 + 16) * 4 KiB = 128 KiB of the CU's 160 KiB */
        if (lds > (64u << 10) &&
            ensure_lds_limit(a.group_pattern ? (const void *)ec_combine_zc<16, NW, true>
                                             : (const void *)ec_combine_zc<16, NW, false>,
                             128 << 10) != 0)
            return -EIO;
        if (a.group_pattern)
            hipLaunchKernelGGL((ec_combine_zc<16, NW, true>), dim3((u32)g), dim3(NW * 64), lds, s, a);
        else
            hipLaunchKernelGGL((ec_combine_zc<16, NW, false>), dim3((u32)g), dim3(NW * 64), lds, s, a);
    }
    return launch_ok("ecdk_combine_host");
}
