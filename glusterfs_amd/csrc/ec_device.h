/*
 * ec_device.h -- internal boundary between the C host layer (ec_method.c) and
 * the HIP device layer (ec_device.hip, ec_kernels.hip).  C-compatible; no HIP
 * types leak into the C side (streams are opaque void pointers).
 */
#ifndef EC_MI355X_DEVICE_H
#define EC_MI355X_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECD_CHUNK 512u      /* EC_METHOD_CHUNK_SIZE (ec-method.h:29) */
#define ECD_MAX_K 16u       /* EC_METHOD_MAX_FRAGMENTS (ec-method.h:23) */
#define ECD_MAX_ROWS 32u    /* >= EC_MAX_NODES (31, ec.h:27-32) */
#define ECD_MAX_PAT_BYTES 2048u
#define ECD_MAX_PATTERNS 256u /* pattern ids are bytes */

/* One launch of the generic GF(2^8) combination kernel:
 *   for every stripe t < nstripes and row r < rows:
 *     out_base[r] + t*out_stride = XOR_p coef[r][p] * (in_base[src[p]] + t*in_stride)
 * on 512-byte bit-sliced chunks.  A "pattern" is the packed byte string
 * {src[k], coef[rows][k]}; with group_pattern != NULL, stripe t uses pattern
 * group_pattern[t >> group_shift] (mixed per-stripe-range erasure patterns),
 * otherwise pattern 0; ids >= npatterns are clamped to the last pattern. */
typedef struct ecd_combine_desc {
    uint32_t k;             /* inputs per stripe (kernel template parameter) */
    uint32_t rows;          /* output rows per stripe                        */
    uint64_t nstripes;
    uint64_t in_stride;     /* bytes between consecutive stripes of an input */
    uint64_t out_stride;    /* bytes between consecutive stripes of a row    */
    const void *in_base[ECD_MAX_ROWS];
    void *out_base[ECD_MAX_ROWS];
    const uint8_t *group_pattern; /* device array, or NULL                   */
    uint32_t group_shift;         /* log2(stripes per pattern group)         */
    uint32_t npatterns;
    uint32_t pat_bytes;           /* bytes per packed pattern = k + rows*k   */
    uint32_t pad;
    /* when non-NULL, the npatterns (<= ECD_MAX_PATTERNS) packed patterns are
     * read from here instead of pat[] (host memory, read during the call);
     * patterns beyond the kernel-argument space go to a device table */
    const uint8_t *pat_ext;
    uint8_t pat[ECD_MAX_PAT_BYTES];
} ecd_combine_desc_t;

/* Number of usable gfx950 devices (0 when none: the host layer then codes
 * with its CPU engine, ec_cpu.h). */
int ecd_device_count(void);
/* The calling thread's last failure ("" if none; on a node without a device,
 * why).  ecd_error_seq counts the failures the thread has recorded, so a
 * caller can tell whether a failing call said why; ecd_set_error records a
 * failure of the host layer (argument errors and the like). */
const char *ecd_last_error(void);
uint64_t ecd_error_seq(void);
void ecd_set_error(const char *text);

/* ---- device-pointer entry points: asynchronous on `stream` (NULL = the
 * calling thread's per-thread default stream of `device`); 0 or -errno. */

/* Compile-time specialised Vandermonde encode (k+r in the shipped table). */
int ecd_has_vander(uint32_t k, uint32_t n);
int ecd_encode_vander(int device, void *stream, uint32_t k, uint32_t n,
                      uint64_t nstripes, const void *in, void *const *out);
/* Generic combination (decode, mixed decode, generic encode, heal). */
int ecd_combine(int device, void *stream, const ecd_combine_desc_t *d);
/* Consistency check (ec_method_verify_device): d is the heal combination
 * that predicts the fragments of d->rows bricks from its k inputs (one
 * pattern in d->pat, in_stride 512; its outputs are unused), check[r] the
 * stored fragment of row r and check_brick[r] its brick index.  bad[t]
 * (device memory, one dword per stripe, all written) gets bit check_brick[r]
 * set where stripe t's stored chunk of row r differs from the prediction. */
int ecd_verify(int device, void *stream, const ecd_combine_desc_t *d, const void *const *check,
               const uint8_t *check_brick, uint32_t *bad);
/* Locating the damaged brick (ec_method_locate_device): d, check and
 * check_brick as for ecd_verify, with d->rows >= 2; basis_brick[p] is the
 * brick index of input p and ratio[(r - 1) * k + p] = G[r][p] / G[0][p] for
 * the rows after the first (G = the coefficients in d->pat, none zero).
 * loc[t] (device memory, one dword per stripe, all written) gets 0, the bit
 * of the one brick that explains stripe t's mismatch, or bit 31 for none. */
int ecd_locate(int device, void *stream, const ecd_combine_desc_t *d, const void *const *check,
               const uint8_t *check_brick, const uint8_t *basis_brick, const uint8_t *ratio,
               uint32_t *loc);
/* A read that checks and corrects (ec_method_decode_checked_device): the
 * arguments of ecd_locate with basis_brick ascending, then inv[j * k + p],
 * the decode matrix of the k inputs (row j gives chunk j of a stripe's data),
 * and ginv[p] = 1 / G[0][p].  loc[t] is ecd_locate's.  out (device memory,
 * nstripes * k * 512 bytes, stripe-major like ecd_combine's decode output,
 * any byte alignment) gets the decode of stripe t's k inputs, after the one
 * input loc[t] names, if any, has been corrected to agree with the others. */
int ecd_decode_checked(int device, void *stream, const ecd_combine_desc_t *d,
                       const void *const *check, const uint8_t *check_brick,
                       const uint8_t *basis_brick, const uint8_t *ratio, const uint8_t *inv,
                       const uint8_t *ginv, void *out, uint32_t *loc);
/* A heal that checks its sources (ec_method_heal_checked_device): the
 * arguments of ecd_locate with basis_brick ascending, then the m = ntargets
 * rows heal[j * k + p] of the heal matrix of the targets from the k inputs
 * (row j gives the chunk of target j), ginv[p] = 1 / G[0][p], and the m target
 * fragments out[j] (device memory, nstripes * 512 bytes each, any byte
 * alignment).  loc[t] is ecd_locate's.  Chunk t of out[j] gets row j applied
 * to stripe t's k inputs, after the one input loc[t] names, if any, has been
 * corrected to agree with the others. */
int ecd_heal_checked(int device, void *stream, const ecd_combine_desc_t *d,
                     const void *const *check, const uint8_t *check_brick,
                     const uint8_t *basis_brick, const uint8_t *ratio, uint32_t ntargets,
                     const uint8_t *heal, const uint8_t *ginv, void *const *out, uint32_t *loc);
/* A read that only detects (ec_method_decode_verified_device): the arguments
 * of ecd_verify with d->rows >= 1, then inv[j * k + p], the decode matrix of
 * the k inputs.  bad[t] is ecd_verify's; out (as for ecd_decode_checked) gets
 * the decode of stripe t's k inputs as stored. */
int ecd_decode_verified(int device, void *stream, const ecd_combine_desc_t *d,
                        const void *const *check, const uint8_t *check_brick,
                        const uint8_t *inv, void *out, uint32_t *bad);
/* A heal that only detects (ec_method_heal_verified_device): the arguments
 * of ecd_verify, then the m = ntargets rows heal[j * k + p] of the heal matrix
 * of the targets from the k inputs and the m target fragments out[j] (as for
 * ecd_heal_checked).  bad[t] is ecd_verify's; chunk t of out[j] gets row j
 * applied to stripe t's k inputs as stored. */
int ecd_heal_verified(int device, void *stream, const ecd_combine_desc_t *d,
                      const void *const *check, const uint8_t *check_brick, uint32_t ntargets,
                      const uint8_t *heal, void *const *out, uint32_t *bad);
/* Locating up to two damaged bricks (ec_method_locate2_device): the
 * arguments of ecd_locate with d->rows >= 4, then ratio1[(r - 2) * k + p] =
 * G[r][p] / G[1][p] for the rows after the second, and for every pair of
 * inputs p < q, in lexicographic order, the 4 bytes {a, b, c, d} of
 * inv([[G[0][p], G[0][q]], [G[1][p], G[1][q]]]) in pair_inv.  loc[t] gets 0,
 * the bits of the one or two bricks that explain stripe t's mismatch, or bit
 * 31 for none. */
int ecd_locate2(int device, void *stream, const ecd_combine_desc_t *d, const void *const *check,
                const uint8_t *check_brick, const uint8_t *basis_brick, const uint8_t *ratio,
                const uint8_t *ratio1, const uint8_t *pair_inv, uint32_t *loc);
/* A read that corrects up to two chunks (ec_method_decode_checked2_device):
 * the arguments of ecd_locate2 with basis_brick ascending, then inv[j * k +
 * p] as for ecd_decode_checked and ginv[r * k + p] = 1 / G[r][p] for rows 0
 * and 1.  loc[t] is ecd_locate2's.  out (as for ecd_decode_checked) gets the
 * decode of stripe t's k inputs, after the one or two inputs loc[t] names, if
 * any, have been corrected to agree with the bricks it does not name. */
int ecd_decode_checked2(int device, void *stream, const ecd_combine_desc_t *d,
                        const void *const *check, const uint8_t *check_brick,
                        const uint8_t *basis_brick, const uint8_t *ratio, const uint8_t *ratio1,
                        const uint8_t *pair_inv, const uint8_t *inv, const uint8_t *ginv,
                        void *out, uint32_t *loc);
/* A heal that corrects up to two chunks (ec_method_heal_checked2_device): the
 * arguments of ecd_locate2 with basis_brick ascending, then ntargets, heal
 * and out as for ecd_heal_checked and ginv as for ecd_decode_checked2.  The k
 * + d->rows inputs and the m targets are different bricks of at most 31.
 * loc[t] is ecd_locate2's.  Chunk t of out[j] gets row j applied to stripe t's
 * k inputs, after the one or two inputs loc[t] names, if any, have been
 * corrected to agree with the bricks it does not name. */
int ecd_heal_checked2(int device, void *stream, const ecd_combine_desc_t *d,
                      const void *const *check, const uint8_t *check_brick,
                      const uint8_t *basis_brick, const uint8_t *ratio, const uint8_t *ratio1,
                      const uint8_t *pair_inv, uint32_t ntargets, const uint8_t *heal,
                      const uint8_t *ginv, void *const *out, uint32_t *loc);
/* Repairing what locate named (ec_method_repair_device): frags[] is indexed
 * by brick and read for the bits of avail (no bit at or above 31); bset is
 * the k + 1 lowest bricks of avail, ascending: the basis B of ecd_locate and
 * c0; coef[i * k + p], for every brick i of avail, is the coefficient of
 * input p of B_i, the k lowest bricks of avail other than i.  Where loc[t]
 * (device memory, read only) is 1 << i for a brick i of avail, chunk t of
 * frags[i] is overwritten with the prediction from B_i; any other value
 * leaves stripe t alone. */
int ecd_repair(int device, void *stream, uint32_t k, uint64_t nstripes, void *const *frags,
               uint32_t avail, const uint8_t *bset, const uint8_t *coef, const uint32_t *loc);
/* Repairing what locate2 named (ec_method_repair2_device): frags, avail and
 * loc as for ecd_repair, with at least k + 2 bits in avail.  B is its k lowest
 * bricks and the `rows` others, ascending, are the check bricks; g[r * k + p]
 * is the heal matrix of the check bricks from B (the G of ecd_locate),
 * ginv[r * k + p] = 1 / g[r * k + p] for rows 0 and 1, and pair_inv is
 * ecd_locate2's.  Where loc[t] has one or two bits, all of bricks of avail,
 * the named chunks of stripe t are overwritten with the prediction from the k
 * lowest bricks of avail outside the named ones; any other value leaves
 * stripe t alone. */
int ecd_repair2(int device, void *stream, uint32_t k, uint64_t nstripes, void *const *frags,
                uint32_t avail, uint32_t rows, const uint8_t *g, const uint8_t *ginv,
                const uint8_t *pair_inv, const uint32_t *loc);
/* Summary and ordered compaction of a loc[] / bad[] array
 * (ec_method_scrub_report_device): every buffer is device memory.  loc
 * (nstripes dwords) is read only.  report gets the 34 words of
 * ec_method_scrub_report_t: stripes with a non-zero word, those of them with
 * bit 31, min(the first, cap), and per bit i < 31 the stripes that have it.
 * idx[r] (may be NULL when cap == 0) gets the index of the r-th non-zero word
 * in ascending order and val[r] (may be NULL) the word, for r < cap; nothing
 * at or past min(count, cap) is written.  work is scratch of
 * ECD_REPORT_WORK(nstripes) bytes, 8-byte aligned: per tile of
 * ECD_REPORT_TILE stripes one 64-bit offset, then ECD_REPORT_COUNTERS planes
 * of one dword per tile (non-zero words, bit 31, bits 0..30).  Three launches
 * (two when cap == 0), no global atomics, no block waits on another.
 * -EINVAL above ECD_REPORT_MAX_STRIPES. */
#define ECD_REPORT_TILE 4096u
#define ECD_REPORT_COUNTERS 33u
#define ECD_REPORT_MAX_STRIPES ((uint64_t)1 << 40)
#define ECD_REPORT_TILES(nstripes) \
    ((uint64_t)(nstripes) / ECD_REPORT_TILE + ((uint64_t)(nstripes) % ECD_REPORT_TILE != 0))
#define ECD_REPORT_WORK(nstripes) \
    ((ECD_REPORT_TILES(nstripes) * (8u + 4u * ECD_REPORT_COUNTERS) + 7u) & ~(uint64_t)7u)
int ecd_scrub_report(int device, void *stream, uint64_t nstripes, const uint32_t *loc,
                     uint64_t *report, uint64_t cap, uint64_t *idx, uint32_t *val, void *work);
int ecd_sync(int device, void *stream);

/* ---- host-memory entry points: stripes are partitioned across `ndev`
 * devices (0 = all visible), each device moves its range over PCIe with
 * pinned staging and overlapped H2D / compute / D2H, and the call blocks.
 * Buffers may be pageable or pinned host memory. */

/* Encode: in = nstripes*k*512 bytes, out[i] = nstripes*512 bytes.  enc_pat
 * (k + n*k bytes, direct coefficients) is used when no specialised encoder
 * exists for k+n. */
int ecd_encode_host(int ndev, uint32_t k, uint32_t n, uint64_t nstripes,
                    const void *in, void *const *out, const uint8_t *enc_pat);
/* The same for `rows` arbitrary encode-matrix rows (ec_method_encode_rows):
 * always the generic combination with `pat` (k + rows*k bytes), never the
 * specialised encoders -- rows == 20 of a 16+8 volume are not the 16+4
 * Vandermonde rows. */
int ecd_encode_host_rows(int ndev, uint32_t k, uint32_t rows, uint64_t nstripes,
                         const void *in, void *const *out, const uint8_t *pat);

/* Encode of a virtual input: the concatenation of nsegs segments
 * (seg_ptr[i] == NULL: seg_len[i] zero bytes), nstripes*k*512 bytes in
 * total, gathered into the pinned staging slots by the copy threads --
 * the padded buffer of a partial-stripe write without a separate copy. */
int ecd_encode_host_gather(int ndev, uint32_t k, uint32_t n, uint64_t nstripes, uint32_t nsegs,
                           const void *const *seg_ptr, const uint64_t *seg_len,
                           void *const *out, const uint8_t *enc_pat);

/* Partial-stripe write on device memory (asynchronous on `stream`): encode
 * the padded buffer {old_head[0:head) | user[0:user_size) | old tail bytes}
 * (NULL old stripes = zeros; one-stripe writes take both ends from old_head,
 * or old_tail when old_head is NULL) into out[0..n), ceil((head +
 * user_size) / (512k)) chunks each.  user may have any alignment. */
int ecd_writev_encode_device(int device, void *stream, uint32_t k, uint32_t n, uint64_t head,
                             uint64_t user_size, const void *user, const void *old_head,
                             const void *old_tail, void *const *out, const uint8_t *enc_pat);

/* Read of an unaligned byte range on device memory (asynchronous on
 * `stream`; ec_method_readv_decode_device): with S = 512 k and ns = ceil((head
 * + size) / S), in[0..k) are fragments of ns * 512 bytes, inv[j * k + p] their
 * decode matrix, and dst[0 .. size) gets bytes [head, head + size) of the ns *
 * S bytes they decode to (head < S, size > 0).  The stripes wholly inside the
 * range run ecd_combine's launch with the output at dst + t * S - head; the
 * first and the last stripe, where the range covers them in part, run one
 * launch of ec_decode_clip, which stores the covered bytes alone.  Nothing
 * outside dst[0 .. size) is written, nothing is allocated or uploaded; in and
 * dst may have any byte alignment. */
int ecd_readv_decode_device(int device, void *stream, uint32_t k, uint64_t head, uint64_t size,
                            const void *const *in, const uint8_t *inv, void *dst);

/* Write of an unaligned byte range over stored fragments, on device memory
 * (asynchronous on `stream`; ec_method_writev_rmw_device): with S = 512 k, end
 * = head + size and ns = ceil(end / S), user[0 .. size) replaces bytes [head,
 * end) of ns stripes and out[0..n) get the ns chunks of their encode.
 * old_head[0..k) / old_tail[0..k) are the stored chunks of the first / last
 * stripe on the k bricks that inv (k x k bytes, inv[j * k + p]) decodes, or
 * NULL for a stripe of zeros; with ns == 1 the stripe's old content is
 * old_head, or old_tail when old_head is NULL.  enc_pat: src[k] then the n x k
 * encode matrix.  The stripes that the write covers wholly run the launch of
 * ec_method_encode_device on user + t * S - head (the combine with the encode
 * rows where that encoder wants an aligned input); the first and the last
 * stripe, where the write covers them in part, run one launch of ec_rmw_edge.
 * Nothing is allocated or uploaded; an old chunk may be the chunk of out[]
 * that replaces it (head < S, size > 0). */
int ecd_writev_rmw_device(int device, void *stream, uint32_t k, uint32_t n, uint64_t head,
                          uint64_t size, const void *user, const void *const *old_head,
                          const void *const *old_tail, const uint8_t *inv, void *const *out,
                          const uint8_t *enc_pat);

/* Fused heal with per-group patterns, on device memory (asynchronous on
 * `stream`; ec_method_heal_mixed_device): frags[0 .. ECD_MAX_ROWS) is indexed
 * by brick (NULL for a brick that no pattern with targets names), nstripes *
 * 512 bytes each.  Stripe group g of 1 << group_shift stripes (>= 4) uses
 * pattern group_pattern[g] (device memory; ids >= npatterns clamp to the last
 * pattern).  pats (host memory, read during the call): npatterns packed
 * patterns of k + 1 + mmax + mmax * k bytes -- src[k], m, dst[mmax],
 * coef[mmax][k] with m <= mmax < 16.  For every stripe t of a group whose
 * pattern has m > 0 and every j < m, chunk t of frags[dst[j]] becomes the sum
 * over p of coef[j][p] * chunk t of frags[src[p]]; nothing else is written,
 * and a group with m == 0 is not read.  One launch of ec_heal_mixed_n; pattern
 * sets beyond its kernel arguments go to a table of the pattern cache. */
int ecd_heal_mixed(int device, void *stream, uint32_t k, uint64_t nstripes,
                   const uint8_t *group_pattern, uint32_t group_shift, uint32_t npatterns,
                   uint32_t mmax, const uint8_t *pats, void *const *frags);

/* ec_method_extent_t as the device layer reads it: 32 fragment addresses
 * indexed by brick, then first, nstripes, pattern and a zero word. */
#define ECD_EXTENT_BYTES 272u
#define ECD_EXTENT_FIRST 256u

/* Fused heal over a table of extents, on device memory (asynchronous on
 * `stream`; ec_method_heal_extents_device): ext_dev is nextents records of
 * ECD_EXTENT_BYTES in memory of `device`, 8-byte aligned, whose `first` fields
 * are the running sum of ceil(nstripes / 4) and add up to ntiles.  pats
 * (host memory, read during the call): npatterns packed patterns as for
 * ecd_heal_mixed.  For every extent whose pattern has m > 0, every stripe t of
 * it and every j < m, chunk t of its frag[dst[j]] becomes the sum over p of
 * coef[j][p] * chunk t of its frag[src[p]]; nothing else is written.  in_bytes
 * (the bytes the call reads, 0: unknown) and aligned (every fragment address
 * is a multiple of 16) choose the staging policy, as ecd_heal_mixed does from
 * its own arguments.  One launch of ec_heal_extents_n. */
int ecd_heal_extents(int device, void *stream, uint32_t k, uint64_t nextents, uint64_t ntiles,
                     const void *ext_dev, uint32_t npatterns, uint32_t mmax,
                     const uint8_t *pats, uint64_t in_bytes, int aligned);

/* Decode / reconstruct: frags[0..nfrags) are fragment buffers of
 * nstripes*512 bytes (NULL for fragments no pattern reads).  Output: when
 * outs is NULL, out = nstripes*rows*512 bytes, stripe-major (decoded data);
 * otherwise outs[r] = nstripes*512 bytes per row (regenerated fragments).  pats
 * holds npatterns packed patterns of k + rows*k bytes whose src[] index
 * frags[]; group_pattern (host, nstripes >> group_shift entries) selects a
 * pattern per stripe group, or NULL for pattern 0 everywhere. */
int ecd_decode_host(int ndev, uint32_t k, uint32_t rows, uint64_t nstripes,
                    uint32_t nfrags, const void *const *frags, void *out,
                    void *const *outs, uint32_t npatterns, const uint8_t *pats,
                    const uint8_t *group_pattern, uint32_t group_shift);

/* Bytes of host-buffer work in flight on the least-loaded host device
 * (UINT64_MAX without a device): the queue a new call would wait behind. */
uint64_t ecd_host_inflight(void);

/* 1 when [p, p + n) lies in pinned, device-mapped host memory (the
 * zero-copy path), 0 for pageable memory or without a device. */
int ecd_host_mapped(const void *p, size_t n);

/* Test hook: the next n host-buffer submissions fail with -EIO before
 * touching a device (exercises the CPU fallback). */
void ecd_inject_faults(uint32_t n);

/* Pointer classification: index of the (gfx950) device owning device
 * memory `p`, or -1 for host memory (pageable or pinned). */
int ecd_ptr_device(const void *p);

/* Pinned host allocation helpers (zero-copy PCIe transfers); allocations
 * are placed on the NUMA node of the first host-buffer device. */
void *ecd_host_alloc(size_t bytes);
/* NUMA node of device index `device` (-1: unknown / single node). */
int ecd_device_numa_node(int device);
/* Staging copy threads this process uses (EC_COPY_THREADS, else at most 8
 * and at most the usable CPUs). */
int ecd_copy_threads(void);
void ecd_host_free(void *p);
int ecd_host_register(void *p, size_t bytes);
/* unregisters a registered range, or drops it from the deferred queue */
int ecd_host_unregister(void *p);
/* queue [p, p + bytes) for registration by the library's thread */
int ecd_host_register_async(void *p, size_t bytes);
/* wait until every queued registration has run */
void ecd_host_register_flush(void);

/* Pinned buffer pool (ec_device.hip BufPool): NULL when no device, too
 * large, or the pool's range is used up; put returns 1 for pool buffers. */
void *ecd_buffer_get(size_t bytes);
int ecd_buffer_put(void *p);

typedef struct ecd_pool_stats {
    uint64_t pool_bytes, in_use_bytes, gets, misses, slabs, slab_register_us;
    uint64_t deferred_registers, deferred_register_us, deferred_register_failures;
    uint64_t unregisters, unregister_us;
} ecd_pool_stats_t;
void ecd_pool_stats(ecd_pool_stats_t *s);

/* Per-pattern whole-matrix kernels compiled at run time (ec_jit.hip, r06). */
typedef struct ecd_jit_stats {
    uint64_t compiled, failed, launches, compile_us, lookups, entries;
} ecd_jit_stats_t;
void ecd_jit_stats(ecd_jit_stats_t *s);
/* Generate and compile the kernel of one coefficient matrix (rows x k bytes)
 * without loading it: its code size, or -errno (-ENOSYS without hiprtc);
 * *ops = v_xor / v_bitop3 instructions per dword column; log = compiler
 * output on failure. */
int ecd_jit_compile_check(uint32_t k, uint32_t rows, const uint8_t *coef, uint32_t *ops,
                          char *log, size_t log_len);
/* the source ecd_jit_compile_check would compile, 0-terminated, truncated to
 * len: the bytes needed (terminator included), or -EINVAL */
int ecd_jit_source(uint32_t k, uint32_t rows, const uint8_t *coef, char *buf, size_t len);
/* queue (or, EC_MI355X_JIT_SYNC=1, compile now) the kernel of a matrix */
int ecd_jit_prepare(uint32_t k, uint32_t rows, const uint8_t *coef);

#ifdef __cplusplus
}
#endif

#endif
