/* ec_kernels.h -- launch wrappers exported by ec_kernels.hip (C++ only). */
#ifndef EC_MI355X_KERNELS_H
#define EC_MI355X_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ec_device.h"

/* Record `what` failed with HIP error `hip_error` as the calling thread's
 * last error (ec_device.hip); returns -EIO. */
extern "C" int ecd_hip_fail(const char *what, int hip_error);

int ecdk_has_vander(uint32_t k, uint32_t n);
/* zc: buffers are pinned host memory coded over PCIe (ec_encode_vander_zc) */
int ecdk_encode_vander(hipStream_t s, uint32_t k, uint32_t n, uint64_t nstripes,
                       const void *in, void *const *out, bool zc = false);
int ecdk_combine(hipStream_t s, const ecd_combine_desc_t *d);
/* the same on pinned host memory (host-buffer path, zero-copy over PCIe) */
int ecdk_combine_host(hipStream_t s, const ecd_combine_desc_t *d);
/* consistency check of ecd_verify (ec_verify_n) */
int ecdk_verify(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                const uint8_t *check_brick, uint32_t *bad);
/* the damaged brick per stripe of ecd_locate (ec_locate_n) */
int ecdk_locate(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                const uint8_t *check_brick, const uint8_t *basis_brick, const uint8_t *ratio,
                uint32_t *loc);
/* the checked and corrected decode of ecd_decode_checked (ec_decode_checked_n) */
int ecdk_decode_checked(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                        const uint8_t *check_brick, const uint8_t *basis_brick,
                        const uint8_t *ratio, const uint8_t *inv, const uint8_t *ginv, void *out,
                        uint32_t *loc);
/* the checked and corrected heal of ecd_heal_checked (ec_heal_checked_n) */
int ecdk_heal_checked(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                      const uint8_t *check_brick, const uint8_t *basis_brick,
                      const uint8_t *ratio, uint32_t ntargets, const uint8_t *heal,
                      const uint8_t *ginv, void *const *out, uint32_t *loc);
/* the decode that only detects of ecd_decode_verified (ec_decode_verified_n) */
int ecdk_decode_verified(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                         const uint8_t *check_brick, const uint8_t *inv, void *out,
                         uint32_t *bad);
/* the heal that only detects of ecd_heal_verified (ec_heal_verified_n) */
int ecdk_heal_verified(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                       const uint8_t *check_brick, uint32_t ntargets, const uint8_t *heal,
                       void *const *out, uint32_t *bad);
/* The partly covered stripes of ecd_readv_decode_device (ec_decode_clip):
 * stripe t of the k fragments is decoded and bytes [lo, hi) of its k * 512 go
 * to base + lo .. base + hi, nothing else is written.  base is where byte 0 of
 * the stripe would lie and may point in front of the caller's buffer. */
typedef struct ecdk_clip_edge {
    uint64_t t;
    uint8_t *base;
    uint32_t lo, hi;
} ecdk_clip_edge_t;
int ecdk_decode_clip(hipStream_t s, uint32_t k, const void *const *in, const uint8_t *inv,
                     uint32_t nedges, const ecdk_clip_edge_t *edge);
/* The partly covered stripes of ecd_writev_rmw_device (ec_rmw_edge): the k
 * stored chunks old[0 .. k) of stripe t (old null: zeros) are decoded with
 * inv, bytes [lo, hi) of the stripe's k * 512 are replaced by user0[t * k * 512
 * + lo ..] and the n chunks of the result go to out[i] + t * 512.  inv: k x k
 * bytes (not read when no edge has old chunks); enc: n x k bytes, the encode
 * matrix.  An old chunk may be the chunk of out that replaces it. */
typedef struct ecdk_rmw_edge {
    uint64_t t;
    const void *const *old;
    uint32_t lo, hi;
} ecdk_rmw_edge_t;
int ecdk_rmw_edge(hipStream_t s, uint32_t k, uint32_t n, const uint8_t *inv, const uint8_t *enc,
                  const uint8_t *user0, void *const *out, uint32_t nedges,
                  const ecdk_rmw_edge_t *edge);
/* The fused heal with per-group patterns of ecd_heal_mixed (ec_heal_mixed_n):
 * stripe group g of 1 << group_shift stripes (>= 4) uses pattern
 * group_pattern[g], ids past the last clamped to it.  pats: npatterns packed
 * patterns of k + 1 + mmax + mmax * k bytes each -- src[k], m, dst[mmax],
 * coef[mmax][k], of which a pattern uses its m <= mmax < 16 first targets and
 * rows; frags: ECD_MAX_ROWS pointers indexed by brick.  For every stripe t of
 * a group with m > 0, chunk t of frags[dst[j]] = XOR_p coef[j][p] * chunk t of
 * frags[src[p]]. */
int ecdk_heal_mixed(hipStream_t s, uint32_t k, uint64_t nstripes, const uint8_t *group_pattern,
                    uint32_t group_shift, uint32_t npatterns, uint32_t mmax, const uint8_t *pats,
                    void *const *frags);
/* The fused heal over a table of extents of ecd_heal_extents
 * (ec_heal_extents_n): tile b of the ntiles belongs to the last record of
 * ext_dev whose `first` is at most b.  pats as for ecdk_heal_mixed. */
int ecdk_heal_extents(hipStream_t s, uint32_t k, uint64_t nextents, uint64_t ntiles,
                      const void *ext_dev, uint32_t npatterns, uint32_t mmax,
                      const uint8_t *pats, uint64_t in_bytes, int aligned);
/* 1 when ecdk_encode_vander(k, n) reads its input at any byte alignment (the
 * tile encoders), 0 when it wants 16-byte alignment (the register encoder) */
int ecdk_encode_any_alignment(uint32_t k, uint32_t n);
/* the one or two damaged bricks per stripe of ecd_locate2 (ec_locate2_n) */
int ecdk_locate2(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                 const uint8_t *check_brick, const uint8_t *basis_brick, const uint8_t *ratio,
                 const uint8_t *ratio1, const uint8_t *pair_inv, uint32_t *loc);
/* the decode corrected around up to two chunks of ecd_decode_checked2
 * (ec_decode_checked2_n) */
int ecdk_decode_checked2(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                         const uint8_t *check_brick, const uint8_t *basis_brick,
                         const uint8_t *ratio, const uint8_t *ratio1, const uint8_t *pair_inv,
                         const uint8_t *inv, const uint8_t *ginv, void *out, uint32_t *loc);
/* the heal corrected around up to two chunks of ecd_heal_checked2
 * (ec_heal_checked2_n) */
int ecdk_heal_checked2(hipStream_t s, const ecd_combine_desc_t *d, const void *const *check,
                       const uint8_t *check_brick, const uint8_t *basis_brick,
                       const uint8_t *ratio, const uint8_t *ratio1, const uint8_t *pair_inv,
                       uint32_t ntargets, const uint8_t *heal, const uint8_t *ginv,
                       void *const *out, uint32_t *loc);
/* rewriting the chunks loc[] names, of ecd_repair (ec_repair_n) */
int ecdk_repair(hipStream_t s, uint32_t k, uint64_t nstripes, void *const *frags, uint32_t avail,
                const uint8_t *bset, const uint8_t *coef, const uint32_t *loc);
/* rewriting the one or two chunks loc[] names, of ecd_repair2 (ec_repair2_n) */
int ecdk_repair2(hipStream_t s, uint32_t k, uint64_t nstripes, void *const *frags, uint32_t avail,
                 uint32_t rows, const uint8_t *g, const uint8_t *ginv, const uint8_t *pair_inv,
                 const uint32_t *loc);
/* the counts and the ordered list of the non-zero words of loc[], of
 * ecd_scrub_report (ec_report_count, ec_report_scan, ec_report_scatter) */
int ecdk_scrub_report(hipStream_t s, uint64_t nstripes, const uint32_t *loc, uint64_t *report,
                      uint64_t cap, uint64_t *idx, uint32_t *val, void *work);
/* Partial-stripe writes: materialise bytes [o0, o0+n) (n % 16 == 0) of the
 * virtual input {head[0:b1) | user[0:b2-b1) | tail[...]} into dst, and the
 * fused Vandermonde encode that reads interior stripes from user directly. */
int ecdk_rmw_gather(hipStream_t s, const uint8_t *head, const uint8_t *user, const uint8_t *tail,
                    uint64_t b1, uint64_t b2, uint64_t o0, uint64_t n, uint8_t *dst);
int ecdk_encode_vander_rmw(hipStream_t s, uint32_t k, uint32_t n, uint64_t nstripes,
                           const uint8_t *edge, const uint8_t *user_shift, void *const *out);

namespace ecdev {
struct CombineArgs;
}
int ecdk_pack_args(const ecd_combine_desc_t *d, ecdev::CombineArgs *a);

#endif
