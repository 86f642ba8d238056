/*
 * ec_method.h -- drop-in C ABI of the MI355X (gfx950) disperse coder.
 *
 * This library (glusterfs_amd/lib/libec_mi355x.so) replaces the coding layer
 * of GlusterFS's disperse translator: ec-method.c, ec-code*.c, ec-galois.c and
 * ec-gf8.c in xlators/cluster/ec/src.  The five ec_method_* prototypes below
 * are exactly those of ec-method.h:31-46, with the same argument meaning,
 * return conventions (0 / negative errno) and data layout (512-byte chunks of
 * 8 bit-planes x 64 bytes, EC_METHOD_CHUNK_SIZE), so ec.c, ec-inode-write.c,
 * ec-inode-read.c and ec-heal.c link against it unchanged.
 *
 * Data buffers may be host memory (pageable or pinned) or MI355X device
 * memory; host data crosses PCIe inside the call, or is coded on the calling
 * thread by the library's CPU engine: on nodes without a gfx950 device, for
 * cpu-extensions = none / x64 / sse / avx, for host calls below the
 * CPU/GPU crossover or while every GPU is saturated, and as the fallback
 * when a device submission fails (the reference coder never fails).
 */
#ifndef EC_MI355X_EC_METHOD_H
#define EC_MI355X_EC_METHOD_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <sys/uio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Constants of ec-method.h:17-29. */
#define EC_GF_BITS 8
#define EC_GF_MOD 0x11D
#define EC_GF_SIZE (1 << EC_GF_BITS)
#define EC_METHOD_MAX_FRAGMENTS 16
#define EC_METHOD_MAX_NODES (EC_GF_SIZE - 1)
#define EC_METHOD_WORD_SIZE 64
#define EC_METHOD_CHUNK_SIZE (EC_METHOD_WORD_SIZE * EC_GF_BITS)

/* Largest brick count the library accepts (EC_MAX_NODES, ec.h:27-32). */
#define EC_MI355X_MAX_NODES 31

#ifndef __EC_TYPES_H__
/* On-disk coding parameters stored in each fragment file's
 * trusted.ec.config xattr (ec-types.h:145-152). */
typedef struct _ec_config ec_config_t;
struct _ec_config {
    uint32_t version;
    uint8_t algorithm;
    uint8_t gf_word_size;
    uint8_t bricks;
    uint8_t redundancy;
    uint32_t chunk_size;
};

/* Standalone declarations.  Inside GlusterFS, ec-types.h (included first)
 * provides the real definitions; the layout below is byte-compatible with
 * ec-types.h:549-562 (sizeof == 120 on LP64, same field offsets), which is
 * the only storage the library uses: the caller embeds the list by value in
 * ec_t (ec-types.h:677). */
typedef struct _xlator xlator_t;
typedef struct _ec_matrix_list ec_matrix_list_t;

struct _ec_matrix_list {
    void *lru[2];           /* struct list_head lru           @0   */
    pthread_mutex_t lock;   /* gf_lock_t lock                 @16  */
    uint32_t columns;       /* k                              @56  */
    uint32_t rows;          /* n                              @60  */
    uint32_t max;           /* decode-matrix cache capacity   @64  */
    uint32_t count;         /* cached decode matrices         @68  */
    uint32_t stripe;        /* EC_METHOD_CHUNK_SIZE * k       @72  */
    void *pool;             /* struct mem_pool *pool          @80  */
    void *gf;               /* ec_gf_t *gf                    @88  */
    void *code;             /* ec_code_t *code                @96  */
    void *encode;           /* ec_matrix_t *encode            @104 */
    void **objects;         /* ec_matrix_t **objects          @112 */
};
#endif

/* ------------------------------------------------------------------------
 * Drop-in entry points (ec-method.h:31-46).
 * --------------------------------------------------------------------- */

/* Replaces ec-method.c:299-353, called from ec.c:837.  columns = k data
 * fragments, rows = n bricks, max = decode matrix cache size (2n in ec.c),
 * gen = the disperse.cpu-extensions value (ec.c:1786-1794) or "hip":
 *   auto, hip        gfx950 engine when a device is visible (with the CPU
 *                    engine for small calls and as the fallback), else CPU
 *   none, x64, sse   CPU engine, base x86-64 code
 *   avx              CPU engine, best AVX level of the host (AVX2/AVX-512)
 * Unknown values warn and act as auto (ec-code.c:1007-1013).  Returns 0,
 * -EINVAL (bad geometry) or -ENOMEM. */
int32_t ec_method_init(xlator_t *xl, ec_matrix_list_t *list, uint32_t columns,
                       uint32_t rows, uint32_t max, const char *gen);

/* Replaces ec-method.c:355-383 (ec.c:198).  Safe on a list whose init failed. */
void ec_method_fini(ec_matrix_list_t *list);

/* Replaces ec-method.c:385-391 (ec.c:293): a no-op returning 0, as in the
 * reference (changing the engine needs a remount there too). */
int32_t ec_method_update(xlator_t *xl, ec_matrix_list_t *list, const char *gen);

/* Replaces ec-method.c:393-408 (ec-inode-write.c:2136).  size: user bytes,
 * a multiple of EC_METHOD_CHUNK_SIZE * k.  out[i] receives size/k bytes of
 * fragment i and, as in the reference, each out[i] is advanced by size/k.
 * Like the reference it cannot fail on host buffers: a device error is redone
 * by the CPU engine.  Invalid arguments, or a fault with caller-provided
 * device buffers, abort with a diagnostic (ec_method_encode_batch returns an
 * error code instead). */
void ec_method_encode(ec_matrix_list_t *list, uint64_t size, void *in, void **out);

/* Replaces ec-method.c:410-433 (ec-inode-read.c:1196).  size: bytes per
 * fragment (multiple of EC_METHOD_CHUNK_SIZE).  mask: the k bricks used;
 * rows[p] = brick index + 1 of in[p], ascending.  out: size * k bytes.
 * Returns 0, -EINVAL, -ENOMEM or -EIO. */
int32_t ec_method_decode(ec_matrix_list_t *list, uint64_t size, uintptr_t mask,
                         uint32_t *rows, void **in, void *out);

/* ------------------------------------------------------------------------
 * Batched / device-resident entry points (new).
 * --------------------------------------------------------------------- */

/* Encode nstripes stripes; in = nstripes*k*512 bytes, out[i] = nstripes*512
 * bytes.  Host buffers are split by stripe range across all visible MI355X
 * devices with overlapped PCIe transfers; device buffers run on device 0.
 * Does not modify out[].  Returns 0 or -errno. */
int32_t ec_method_encode_batch(ec_matrix_list_t *list, uint64_t nstripes,
                               const void *in, void *const *out);

/* Decode nstripes stripes with one mask (as ec_method_decode, sizes in
 * stripes).  Returns 0 or -errno. */
int32_t ec_method_decode_batch(ec_matrix_list_t *list, uint64_t nstripes,
                               uintptr_t mask, const uint32_t *rows,
                               const void *const *in, void *out);

/* Self-heal style reconstruction with mixed erasure patterns: frags[0..n)
 * are all n fragment buffers (nstripes*512 bytes each; entries of bricks no
 * group reads may be NULL), group g = stripes [g*group_stripes,
 * (g+1)*group_stripes) is decoded from the k bricks in group_masks[g].
 * group_stripes is a power of two (groups of 1, 2 or 4 stripes are sorted
 * by pattern into 8-stripe tiles on the device first).
 * out = nstripes*k*512 bytes.
 * Up to 256 distinct masks per call (-E2BIG beyond). */
int32_t ec_method_decode_mixed(ec_matrix_list_t *list, uint64_t nstripes,
                               uint64_t group_stripes, const uintptr_t *group_masks,
                               const void *const *frags, void *out);

/* Encode of selected fragments: ec_method_encode restricted to the fragments
 * whose bit i is set in row_mask (bit i = brick i, the numbering of decode
 * masks).  A heal write goes to the bad bricks only (ec-heal.c:327-329:
 * ec_writev with heal->bad) and a degraded write skips the bricks that are
 * down, yet ec_writev_encode (ec-inode-write.c:2125-2138) computes all n
 * fragments; this computes |row_mask| of them, i.e. writes m*size/k instead
 * of n*size/k bytes and does m/n of the arithmetic.  out[] is indexed by
 * brick as in ec_method_encode: out[i] is read and advanced by size/k only for
 * the bits of row_mask (the others may be NULL and are left alone).  A full
 * row_mask is ec_method_encode, an empty one a no-op.  Cannot fail on host buffers; invalid
 * arguments abort with a diagnostic, as ec_method_encode. */
void ec_method_encode_rows(ec_matrix_list_t *list, uint64_t size, void *in,
                           uintptr_t row_mask, void **out);

/* Fused heal: regenerate the fragments of the bricks
 * in `target_mask` straight from the k fragments in `mask`, without
 * materialising the decoded data: out[j] (nstripes*512 bytes) is the fragment
 * of the j-th set bit of target_mask.  Returns 0 or -errno. */
int32_t ec_method_heal(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t mask,
                       const void *const *in, uintptr_t target_mask,
                       void *const *out);

/* Fused heal with a pattern per stripe group: ec_method_heal for a batch in
 * which the missing bricks -- and with them the bricks to read -- change from
 * group to group, as ec_method_decode_mixed is for decodes.  frags[0..n) is
 * indexed by brick (nstripes*512 bytes each).  Group g is the stripes
 * [g*group_stripes, min((g+1)*group_stripes, nstripes)); group_stripes is a
 * power of two of at least 4 (the device kernel's tile, which must have one
 * pattern; the host call keeps the same rule).  For every stripe t of group g
 * and every brick i in group_targets[g], chunk t of frags[i] becomes what
 * ec_method_heal gives for that stripe from the k bricks in group_masks[g].
 * Nothing else is written and the source chunks are only read, so the call
 * works in place on the stored fragments: a target mask may not overlap its
 * mask, and groups touch different stripes.  A group with an empty target mask
 * is left alone and none of its chunks are read.  frags[i] may be NULL for a
 * brick that no group names, or only groups with an empty target mask.
 * Runs on the calling thread's CPU engine whatever the volume's engine is, and
 * leaves ec_method_get_stats alone: it is the byte-exact specification of the
 * device call below.
 * -EINVAL (with the reason in ec_method_last_error()): list, frags, group_masks
 * or group_targets NULL; group_stripes not a power of two or below 4; a mask
 * that is not k bricks of the volume; a target mask with a bit at or above n,
 * a bit of its mask or more than 15 bits; a NULL fragment for a brick of a
 * mask or target mask whose target mask is not empty; a fragment in device
 * memory.  -E2BIG: more than 256 distinct (mask, target mask) pairs.
 * nstripes == 0 returns 0 after the first checks and touches nothing. */
int32_t ec_method_heal_mixed(ec_matrix_list_t *list, uint64_t nstripes, uint64_t group_stripes,
                             const uintptr_t *group_masks, const uintptr_t *group_targets,
                             void *const *frags);

/* Consistency check: do the fragments of the bricks in check_mask agree with
 * the k fragments in mask?  in[p] = fragment of the p-th set bit of mask,
 * check[j] = stored fragment of the j-th set bit of check_mask (nstripes*512
 * bytes each).  bad[t] (uint32, one per stripe) gets bit i set when brick i
 * is in check_mask and its stored chunk of stripe t differs from the chunk
 * the k fragments imply (E_i * inv(mask) applied to in[]); 0 = consistent.
 * Every bad[0..nstripes) is written.  *nbad (may be NULL) = stripes with
 * bad[t] != 0.  Nothing is decoded or regenerated to memory.
 *
 * The code is MDS, so one damaged chunk of a check brick sets that brick's
 * bit alone, and one damaged chunk of a basis brick (mask) sets the bit of
 * every check brick: to tell which basis brick it is, call again with
 * another mask (or ec_method_locate below, in one pass).  One mask per call.
 *
 * -EINVAL: mask is not exactly k bricks below n; check_mask is empty, has a
 * bit at or above n or overlaps mask; a NULL pointer; bad not 4-byte
 * aligned; host and device buffers mixed, or given to the wrong entry point.
 * nstripes == 0 returns 0 and writes nothing.
 *
 * The host variant runs on the calling thread's CPU engine whatever the
 * volume's engine is, and leaves ec_method_stats_t and the router alone.
 * The device variant takes device pointers on `device` (bad[] included) and
 * is asynchronous on `stream` like the calls below: matrices travel in the
 * kernel arguments, each bad[t] is written by one plain store, nothing is
 * pre-zeroed and nothing is counted on the device -- the caller reduces
 * bad[] (4 bytes per (k + m) * 512 read). */
int32_t ec_method_verify(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t mask,
                         const void *const *in, uintptr_t check_mask,
                         const void *const *check, uint32_t *bad, uint64_t *nbad);
int32_t ec_method_verify_device(ec_matrix_list_t *list, int device, void *stream,
                                uint64_t nstripes, uintptr_t mask, const void *const *in,
                                uintptr_t check_mask, const void *const *check,
                                uint32_t *bad);

/* Locating the damaged brick: one pass over the stored fragments that names,
 * per stripe, the brick whose chunk is wrong, so that ec_method_heal can be
 * given a mask without it.  frags[0..n) is indexed by brick as in
 * ec_method_decode_mixed (nstripes*512 bytes each); entries of bricks outside
 * avail_mask are not read and may be NULL.  avail_mask names the a >= k + 2
 * bricks whose stored fragments are at hand.  loc[t] (uint32, one per stripe,
 * every loc[0..nstripes) written) is
 *   0                       the a chunks of stripe t are mutually consistent
 *                           (any k of them imply the others);
 *   1u << i                 they are not, and brick i of avail_mask is the one
 *                           brick whose removal leaves the other a - 1 chunks
 *                           mutually consistent;
 *   EC_MI355X_LOCATE_MANY   they are not, and no single brick explains it.
 * With a >= k + 2 at most one brick can qualify (two would give two codewords
 * that agree on a - 2 >= k positions, hence one codeword), so exactly one of
 * the three holds.  *nbad (host variant, may be NULL) = stripes with
 * loc[t] != 0.
 *
 * What the code can promise: one damaged chunk per stripe is always named
 * correctly.  With a - k >= 3, two damaged chunks in a stripe are always
 * MANY (distance >= 4).  With a - k == 2 two damaged chunks can imitate a
 * single error in a third brick: the code then has distance 3, so this is a
 * property of the code, not of the call.
 *
 * -EINVAL: a NULL list, frags or loc; loc not 4-byte aligned; a bit of
 * avail_mask at or above n; fewer than k + 2 bits (so every call on a 2+1
 * volume); a NULL frags[i] for a set bit; host and device buffers mixed, or
 * given to the wrong entry point (the device variant wants every buffer, loc
 * included, on `device`).  nstripes == 0 returns 0 after these checks and
 * writes nothing.  One avail_mask per call.
 *
 * Like ec_method_verify, the host variant runs on the calling thread's CPU
 * engine whatever the volume's engine is and leaves ec_method_stats_t, the
 * router and the run-time compiler alone; the device variant is asynchronous
 * on `stream`, pre-zeroes nothing, uses no global atomics and writes each
 * loc[t] by one plain store (-ENODEV where the device layer lacks it). */
#define EC_MI355X_LOCATE_MANY 0x80000000u /* bit 31: EC_MI355X_MAX_NODES is 31 */
int32_t ec_method_locate(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t avail_mask,
                         const void *const *frags, uint32_t *loc, uint64_t *nbad);
int32_t ec_method_locate_device(ec_matrix_list_t *list, int device, void *stream,
                                uint64_t nstripes, uintptr_t avail_mask,
                                const void *const *frags, uint32_t *loc);

/* A read that checks and corrects: ec_method_decode and ec_method_locate in
 * one pass over the fragments.  ec_method_decode takes exactly k fragments
 * and trusts them, so one silently damaged chunk comes back as k*512 bytes of
 * wrong data with return code 0; this call reads the a >= k + 2 fragments at
 * hand, names the bad brick per stripe and decodes around it.  frags,
 * avail_mask and loc as for ec_method_locate; out receives nstripes*k*512
 * bytes, stripe t at out + t*k*512: the layout of ec_method_decode_device's
 * out, and like it the device variant takes out at any byte alignment (loc
 * wants 4).
 *
 * Let B be the k lowest bricks of avail_mask and B_i the k lowest bricks of
 * avail_mask other than i (ec_method_repair's B_i).  loc[t] is exactly what
 * ec_method_locate gives on the same arguments, every loc[0..nstripes)
 * written, and stripe t of out is, from the stored chunks,
 *   loc[t] == 0                      ec_method_decode with mask B (the chunks
 *                                    are consistent: any k give the same);
 *   loc[t] == 1u << i                ec_method_decode with mask B_i.  For a
 *                                    check brick B_i = B and the bad chunk
 *                                    changes nothing; for a basis brick the
 *                                    damaged chunk is not used;
 *   loc[t] == EC_MI355X_LOCATE_MANY  ec_method_decode with mask B as stored:
 *                                    defined bytes, but the caller must treat
 *                                    the stripe as -EIO.
 * So wherever at most one chunk of a stripe is damaged, out is the data the
 * fragments were encoded from.  The a - k == 2 caveat of ec_method_locate
 * carries over: two damaged chunks can imitate one, and out is then what the
 * code implies.  Nothing in frags is written, and nothing past
 * out + nstripes*k*512.
 *
 * *nbad (host variant, may be NULL) = stripes with loc[t] != 0; *nmany (may
 * be NULL) = stripes with loc[t] == EC_MI355X_LOCATE_MANY.  The device
 * variant counts nothing: the caller reduces loc[].
 *
 * -EINVAL: as ec_method_locate, and a NULL out (the device variant wants out
 * on `device` too).  nstripes == 0 returns 0 after these checks and writes
 * nothing.
 *
 * Like ec_method_locate, the host variant runs on the calling thread's CPU
 * engine whatever the volume's engine is and leaves ec_method_stats_t, the
 * router and the run-time compiler alone; the device variant is asynchronous
 * on `stream` with no host synchronisation (inv(B) and every other table
 * travel in the kernel arguments), reads a and writes k chunks per stripe,
 * pre-zeroes nothing, uses no global atomics and writes each loc[t] by one
 * plain store (-ENODEV where the device layer lacks it). */
int32_t ec_method_decode_checked(ec_matrix_list_t *list, uint64_t nstripes,
                                 uintptr_t avail_mask, const void *const *frags, void *out,
                                 uint32_t *loc, uint64_t *nbad, uint64_t *nmany);
int32_t ec_method_decode_checked_device(ec_matrix_list_t *list, int device, void *stream,
                                        uint64_t nstripes, uintptr_t avail_mask,
                                        const void *const *frags, void *out, uint32_t *loc);

/* A heal that checks its sources: ec_method_heal and ec_method_locate in one
 * pass over the fragments.  ec_method_heal takes exactly k source fragments
 * and trusts them, so one silently damaged chunk in a source comes back as a
 * wrong chunk in every healed fragment with return code 0, and is then
 * written to a new brick; this call reads the a >= k + 2 fragments at hand,
 * names the bad brick per stripe and heals around it.  frags, avail_mask,
 * loc, nbad and nmany as for ec_method_decode_checked; target_mask and out as
 * for ec_method_heal: out[j] (nstripes*512 bytes) is the fragment of the j-th
 * set bit of target_mask, and the device variant takes each out[j] at any byte
 * alignment (loc wants 4).
 *
 * Let B be the k lowest bricks of avail_mask and B_i the k lowest bricks of
 * avail_mask other than i.  loc[t] is exactly what ec_method_locate gives on
 * the same arguments, every loc[0..nstripes) written, and chunk t of every
 * out[j] is, from the stored chunks, what ec_method_heal gives for that stripe
 * with the same target_mask and
 *   loc[t] == 0                      mask B (the chunks are consistent: any k
 *                                    give the same);
 *   loc[t] == 1u << i                mask B_i.  For a check brick B_i = B and
 *                                    the bad chunk changes nothing; for a
 *                                    basis brick the damaged chunk is not
 *                                    used;
 *   loc[t] == EC_MI355X_LOCATE_MANY  mask B as stored: defined bytes, but the
 *                                    caller must treat the stripe as -EIO.
 * So wherever at most one chunk of a stripe is damaged, every out[j] chunk is
 * the chunk the original data encodes to.  The a - k == 2 caveat of
 * ec_method_locate carries over: two damaged chunks can imitate one, and the
 * targets are then what the code implies.  Nothing in frags is written, nothing
 * past nstripes*512 of any out[j], and only the out[j] of target_mask.
 *
 * The device variant can be followed on one stream, with no host
 * synchronisation, by ec_method_repair_device on the same loc and then
 * ec_method_locate_device: afterwards the sources are clean, the targets are
 * right and the second locate is all zero.
 *
 * -EINVAL: everything ec_method_locate rejects; an empty target_mask, one
 * with a bit at or above n, or one that overlaps avail_mask; a NULL out or a
 * NULL out[j]; host and device buffers mixed, or given to the wrong entry
 * point (the device variant wants every out[j] on `device` too).  A target
 * beside k + 2 available bricks takes n - k >= 3, so every call on a 2+1 or a
 * 4+2 volume is -EINVAL.  nstripes == 0 returns 0 after these checks and
 * writes nothing.
 *
 * Like ec_method_decode_checked, the host variant runs on the calling
 * thread's CPU engine whatever the volume's engine is and leaves
 * ec_method_stats_t, the router and the run-time compiler alone; the device
 * variant is asynchronous on `stream` with no host synchronisation (the heal
 * matrix of the targets from B and every other table travel in the kernel
 * arguments, nothing is uploaded), reads a and writes m = |target_mask| chunks
 * per stripe, pre-zeroes nothing, uses no global atomics, writes each loc[t]
 * by one plain store and counts nothing (-ENODEV where the device layer lacks
 * it). */
int32_t ec_method_heal_checked(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t avail_mask,
                               const void *const *frags, uintptr_t target_mask,
                               void *const *out, uint32_t *loc, uint64_t *nbad,
                               uint64_t *nmany);
int32_t ec_method_heal_checked_device(ec_matrix_list_t *list, int device, void *stream,
                                      uint64_t nstripes, uintptr_t avail_mask,
                                      const void *const *frags, uintptr_t target_mask,
                                      void *const *out, uint32_t *loc);

/* A heal that corrects two chunks: ec_method_heal and ec_method_locate2 in
 * one pass over the fragments.  ec_method_heal_checked answers
 * EC_MI355X_LOCATE_MANY for a stripe with two damaged source chunks and heals
 * it from B as stored, which is wrong bytes in every target; with a >= k + 4
 * fragments at hand such a stripe still has exactly one nearest codeword, and
 * this call heals around the pair.  Everything is ec_method_heal_checked's --
 * arguments, buffer rules, asynchrony, alignment (the device variant takes
 * each out[j] at any byte alignment, loc wants 4), counters and error codes --
 * except:
 *
 * avail_mask must name a >= k + 4 bricks, as for ec_method_locate2; fewer are
 * -EINVAL.  A target beside k + 4 available bricks takes n - k >= 5, so every
 * call on a 2+1, 4+2, 8+4 or 16+4 volume is -EINVAL.
 *
 * loc[t] is exactly what ec_method_locate2 gives on the same arguments, every
 * loc[0..nstripes) written, each by one plain store.
 *
 * With B the k lowest bricks of avail_mask and B_S the k lowest bricks of
 * avail_mask not in the set S, chunk t of every out[j] is, from the stored
 * chunks, what ec_method_heal gives for that stripe with the same target_mask
 * and
 *   loc[t] == 0                      mask B;
 *   loc[t] has the one or two bits   mask B_S.  For one bit this is
 *   of S                             ec_method_heal_checked's answer, byte for
 *                                    byte; for two check bricks B_S = B; for
 *                                    basis + check and basis + basis the
 *                                    damaged chunks are not used;
 *   loc[t] == EC_MI355X_LOCATE_MANY  mask B as stored: defined bytes, but the
 *                                    caller must treat the stripe as -EIO.
 * So wherever at most two chunks of a stripe are damaged, every out[j] chunk
 * is the chunk the original data encodes to, and wherever
 * ec_method_heal_checked gives 0 or one bit both calls give the same loc[t]
 * and the same target bytes.  The a - k == 4 caveat of ec_method_locate2
 * carries over.  Nothing in frags is written, nothing past nstripes*512 of any
 * out[j], and only the out[j] of target_mask.  nstripes == 0 returns 0 after
 * the argument checks and writes nothing.
 *
 * The device variant can be followed on one stream, with no host
 * synchronisation, by ec_method_repair2_device on the same loc and then
 * ec_method_locate2_device: afterwards the sources are clean, the targets are
 * right and the second locate2 is all zero.  It uploads nothing (locate2's
 * tables, the heal matrix of the targets from B and the target pointers all
 * travel in the kernel arguments), pre-zeroes nothing, uses no global atomics
 * and counts nothing (-ENODEV where the device layer lacks it); the host
 * variant runs on the calling thread's CPU engine whatever the volume's
 * engine is and leaves ec_method_stats_t, the router and the run-time
 * compiler alone. */
int32_t ec_method_heal_checked2(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t avail_mask,
                                const void *const *frags, uintptr_t target_mask,
                                void *const *out, uint32_t *loc, uint64_t *nbad,
                                uint64_t *nmany);
int32_t ec_method_heal_checked2_device(ec_matrix_list_t *list, int device, void *stream,
                                       uint64_t nstripes, uintptr_t avail_mask,
                                       const void *const *frags, uintptr_t target_mask,
                                       void *const *out, uint32_t *loc);

/* A read and a heal that only detect, from k + 1 fragments.  The checked
 * calls above want a >= k + 2 fragments, which leaves out every 2+1 volume, a
 * 4+2 read with one brick down and the ordinary 4+2 heal (five sources, one
 * target).  With a = k + 1 the code cannot name the bad brick, but it can say
 * that a stripe is inconsistent: these calls are ec_method_decode (or
 * ec_method_heal) and ec_method_verify in one pass over the fragments, so
 * that a caller can answer -EIO instead of wrong bytes.  frags and avail_mask
 * are ec_method_locate's, indexed by brick -- entries outside avail_mask are
 * not read and may be NULL -- except that a >= k + 1 bricks are enough.
 *
 * Let B be the k lowest bricks of avail_mask and C the others (a - k >= 1).
 *   bad[t]   exactly what ec_method_verify gives with mask = B and check_mask
 *            = C on the same buffers: bit i is set when brick i is in C and
 *            its stored chunk t differs from what the chunks of B imply.
 *            Every bad[0..nstripes) is written, each by one plain store.
 *            *nbad (host variants, may be NULL) = stripes with bad[t] != 0.
 *   out      of decode_verified: nstripes*k*512 bytes, stripe t at out +
 *            t*k*512, the layout of ec_method_decode_device's out (any byte
 *            alignment on the device).  Stripe t is always ec_method_decode
 *            with mask B as stored, byte for byte.
 *   out[j]   of heal_verified: the fragment of the j-th set bit of
 *            target_mask, chunk t at out[j] + t*512, as in ec_method_heal
 *            (any byte alignment on the device).  It is always ec_method_heal
 *            with mask B and the same target_mask, as stored.
 * Nothing is corrected, so:
 *   bad[t] == 0   the a chunks are mutually consistent and the output is
 *                 right;
 *   otherwise     with a == k + 1 the stripe cannot be trusted and is to be
 *                 treated as -EIO.  With a >= k + 2 a single bit means that
 *                 check brick alone is bad and the output is right; every
 *                 bit of C set means a basis chunk is damaged (or several
 *                 chunks are) and the output is wrong.  A caller that holds
 *                 k + 2 fragments or more then runs ec_method_decode_checked
 *                 or ec_method_heal_checked.
 * Nothing in frags is written, nothing past out + nstripes*k*512, nothing
 * past nstripes*512 of any out[j], and only the out[j] of target_mask.
 *
 * -EINVAL: a NULL list, frags, bad or out; bad not 4-byte aligned; a bit of
 * avail_mask at or above n; fewer than k + 1 bits; a NULL frags[i] for a set
 * bit; host and device buffers mixed, or given to the wrong entry point (the
 * device variants want every buffer, bad and the outputs included, on
 * `device`); for the heal also an empty target_mask, one with a bit at or
 * above n, one that overlaps avail_mask, or a NULL out[j].  A target beside
 * k + 1 sources takes n - k >= 2, so every heal_verified call on a 2+1 volume
 * is -EINVAL.  nstripes == 0 returns 0 after these checks and writes nothing.
 * One avail_mask per call.
 *
 * Like ec_method_verify, the host variants run on the calling thread's CPU
 * engine whatever the volume's engine is and leave ec_method_stats_t, the
 * router and the run-time compiler alone; the device variants are
 * asynchronous on `stream` with no host synchronisation (every table travels
 * in the kernel arguments, nothing is uploaded), read a and write k or m =
 * |target_mask| chunks per stripe, pre-zero nothing, use no global atomics
 * and count nothing (-ENODEV where the device layer lacks the call). */
int32_t ec_method_decode_verified(ec_matrix_list_t *list, uint64_t nstripes,
                                  uintptr_t avail_mask, const void *const *frags, void *out,
                                  uint32_t *bad, uint64_t *nbad);
int32_t ec_method_decode_verified_device(ec_matrix_list_t *list, int device, void *stream,
                                         uint64_t nstripes, uintptr_t avail_mask,
                                         const void *const *frags, void *out, uint32_t *bad);
int32_t ec_method_heal_verified(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t avail_mask,
                                const void *const *frags, uintptr_t target_mask,
                                void *const *out, uint32_t *bad, uint64_t *nbad);
int32_t ec_method_heal_verified_device(ec_matrix_list_t *list, int device, void *stream,
                                       uint64_t nstripes, uintptr_t avail_mask,
                                       const void *const *frags, uintptr_t target_mask,
                                       void *const *out, uint32_t *bad);

/* Locating up to two damaged bricks.  Arguments, buffer rules, asynchrony
 * and error codes are ec_method_locate's, except that avail_mask must name
 * a >= k + 4 bricks: fewer bits are -EINVAL (so every call on a 2+1 or 4+2
 * volume).  Restricted to those a bricks the code has distance a - k + 1 >=
 * 5, so at most one codeword lies within two chunk positions of the a stored
 * chunks of stripe t.  loc[t] (every loc[0..nstripes) written) is
 *   0                       the a chunks are mutually consistent;
 *   the OR of 1u << i       over the one or two bricks where the stored
 *                           chunks differ from that codeword, when it exists:
 *                           the smallest set S, |S| <= 2, whose removal
 *                           leaves the other a - |S| chunks consistent;
 *   EC_MI355X_LOCATE_MANY   otherwise.
 * S is unique: two such sets would give codewords that agree on >= a - 4 >= k
 * positions, hence one codeword, and the stored chunks would differ from it
 * only on the intersection, a smaller set.  *nbad (host variant, may be NULL)
 * = stripes with loc[t] != 0.
 *
 * What follows:
 *   - wherever ec_method_locate on the same arguments gives 0 or a single
 *     bit, ec_method_locate2 gives the same value;
 *   - wherever locate gives MANY, locate2 gives two bits or MANY;
 *   - one or two damaged chunks per stripe are always named correctly;
 *   - with a - k >= 5, three damaged chunks are always MANY;
 *   - with a - k == 4 three damaged chunks can imitate a pair (distance 5):
 *     a property of the code, as the a - k == 2 caveat is for locate.
 *
 * Acting on a pair: ec_method_repair leaves a stripe with two bits alone;
 * ec_method_repair2[_device], below, consumes loc[] where it lies and rewrites
 * both chunks.  Its result for one stripe is that of ec_method_heal[_device]
 * on that stripe with mask = the k lowest bricks of avail_mask other than the
 * named ones and target_mask = the named ones.
 *
 * Like ec_method_locate, the host variant runs on the calling thread's CPU
 * engine whatever the volume's engine is and leaves ec_method_stats_t, the
 * router and the run-time compiler alone; the device variant is asynchronous
 * on `stream` with no host synchronisation (every table travels in the
 * kernel arguments), pre-zeroes nothing, uses no global atomics and writes
 * each loc[t] by one plain store (-ENODEV where the device layer lacks it). */
int32_t ec_method_locate2(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t avail_mask,
                          const void *const *frags, uint32_t *loc, uint64_t *nbad);
int32_t ec_method_locate2_device(ec_matrix_list_t *list, int device, void *stream,
                                 uint64_t nstripes, uintptr_t avail_mask,
                                 const void *const *frags, uint32_t *loc);

/* A read that corrects two chunks: ec_method_decode_checked with
 * ec_method_locate2's answer in place of ec_method_locate's.  Arguments,
 * buffer rules, asynchrony, alignment and error codes are those of
 * ec_method_decode_checked, except that avail_mask must name a >= k + 4
 * bricks, as for ec_method_locate2: fewer bits are -EINVAL (so every call on
 * a 2+1 or 4+2 volume).  out takes any byte alignment on the device, loc
 * wants 4.  Nothing in frags is written, and nothing past
 * out + nstripes*k*512.  nstripes == 0 returns 0 after the argument checks
 * and writes nothing.
 *
 * Let B be the k lowest bricks of avail_mask and, for a set S of bricks, B_S
 * the k lowest bricks of avail_mask not in S.  loc[t] is exactly what
 * ec_method_locate2 gives on the same arguments, every loc[0..nstripes)
 * written, and stripe t of out is, from the stored chunks,
 *   loc[t] == 0                      ec_method_decode with mask B;
 *   loc[t] == one or two bits, the   ec_method_decode with mask B_S.  For one
 *             bricks of S            bit this is ec_method_decode_checked's
 *                                    answer; for two check bricks B_S = B; for
 *                                    basis + check and basis + basis the
 *                                    damaged chunks are not used;
 *   loc[t] == EC_MI355X_LOCATE_MANY  ec_method_decode with mask B as stored:
 *                                    defined bytes, but the caller must treat
 *                                    the stripe as -EIO.
 * What follows:
 *   - wherever at most two chunks of a stripe are damaged, out is the data
 *     the fragments were encoded from;
 *   - wherever ec_method_decode_checked on the same arguments gives 0 or a
 *     single bit, loc[t] and stripe t of out are byte for byte the same here;
 *   - the a - k == 4 caveat of ec_method_locate2 carries over: three damaged
 *     chunks can imitate a pair, and out is then what the code implies.
 *
 * *nbad (host variant, may be NULL) = stripes with loc[t] != 0; *nmany (may
 * be NULL) = stripes with loc[t] == EC_MI355X_LOCATE_MANY.  The device
 * variant counts nothing: the caller reduces loc[].
 *
 * The host variant runs on the calling thread's CPU engine whatever the
 * volume's engine is, leaves ec_method_stats_t, the router and the run-time
 * compiler alone, and answers -EINVAL to a device pointer; the device variant
 * is asynchronous on `stream` with no host synchronisation (inv(B), the
 * tables of locate2 and the inverses the correction needs travel in the
 * kernel arguments), reads a and writes k chunks per stripe, pre-zeroes
 * nothing, uses no global atomics and writes each loc[t] by one plain store
 * (-ENODEV where the device layer lacks it). */
int32_t ec_method_decode_checked2(ec_matrix_list_t *list, uint64_t nstripes,
                                  uintptr_t avail_mask, const void *const *frags, void *out,
                                  uint32_t *loc, uint64_t *nbad, uint64_t *nmany);
int32_t ec_method_decode_checked2_device(ec_matrix_list_t *list, int device, void *stream,
                                         uint64_t nstripes, uintptr_t avail_mask,
                                         const void *const *frags, void *out, uint32_t *loc);

/* Repairing what locate named: one call that consumes loc[] where it lies and
 * rewrites only the named chunks, closing verify -> locate -> repair.  frags
 * and avail_mask as for ec_method_locate, except that a >= k + 1 bricks are
 * enough (k others determine a chunk), so a caller that learned the bad brick
 * another way, a checksum for example, can use it with k + 1 fragments.
 * loc[t] is read and never written.
 *
 * Where loc[t] == 1u << i with brick i in avail_mask, chunk t of frags[i] is
 * overwritten with E_i * inv(B_i) applied to the chunks of B_i, the k lowest
 * bricks of avail_mask other than i (the encode of the decode of those k
 * chunks, row i).  Every other value leaves stripe t byte for byte as it was:
 * 0, EC_MI355X_LOCATE_MANY alone or ORed with anything, two or more bits, the
 * bit of a brick outside avail_mask or at or above n.  None of these is an
 * error: the device variant sees them only on the GPU, so neither engine
 * reports them.  Only chunk t of the named brick is written: nothing past
 * nstripes*512, no other brick.
 *
 * With loc[] from ec_method_locate on the same frags and avail_mask, every
 * stripe that locate named with a single brick is mutually consistent again
 * and a second locate gives 0 for it.  As said there, with a - k == 2 two
 * damaged chunks can imitate one: repair then writes what the code implies,
 * not what was originally stored.  A wholly bad brick is ec_method_heal's
 * job (one pattern, dense streaming); this call is for what a scrub finds.
 *
 * *nrepaired (host variant, may be NULL) = stripes rewritten; *nskipped (may
 * be NULL) = stripes with loc[t] != 0 that were left alone.  The device
 * variant counts nothing: the caller already holds loc[].
 *
 * -EINVAL: a NULL list, frags or loc; loc not 4-byte aligned; a bit of
 * avail_mask at or above n; fewer than k + 1 bits; a NULL frags[i] for a set
 * bit; host and device buffers mixed, or given to the wrong entry point (the
 * device variant wants every buffer, loc included, on `device`).
 * nstripes == 0 returns 0 after these checks and touches nothing.
 *
 * Like ec_method_locate, the host variant runs on the calling thread's CPU
 * engine whatever the volume's engine is and leaves ec_method_stats_t, the
 * router and the run-time compiler alone; the device variant is asynchronous
 * on `stream` (locate and repair can be queued back to back with no host
 * synchronisation between them), pre-zeroes nothing and uses no global
 * atomics (-ENODEV where the device layer lacks it). */
int32_t ec_method_repair(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t avail_mask,
                         void *const *frags, const uint32_t *loc,
                         uint64_t *nrepaired, uint64_t *nskipped);
int32_t ec_method_repair_device(ec_matrix_list_t *list, int device, void *stream,
                                uint64_t nstripes, uintptr_t avail_mask,
                                void *const *frags, const uint32_t *loc);

/* Repairing what locate2 named: ec_method_repair for loc[] values of one or
 * two bits, closing verify -> locate2 -> repair2 on one stream.  Arguments,
 * buffer rules, asynchrony and error codes are ec_method_repair's, except that
 * avail_mask must name a >= k + 2 bricks (k others must remain once a pair is
 * removed): fewer bits are -EINVAL, so every call on a 2+1 volume.  a = k + 2
 * is enough: a caller that learned the pair another way, from checksums for
 * example, can use the call where ec_method_locate2 (a >= k + 4) cannot run,
 * on a 4+2 volume with every brick for instance.  loc[t] is read and never
 * written.
 *
 * Let S be the set of bricks whose bits are set in loc[t].
 *   |S| = 1, the brick in avail_mask: exactly what ec_method_repair does,
 *       byte for byte (B_i = the k lowest bricks of avail_mask other than i).
 *   |S| = 2, both bricks i < j in avail_mask: chunk t of frags[i] and chunk t
 *       of frags[j] are overwritten with rows i and j of E * inv(B_ij)
 *       applied to the stored chunks of B_ij, the k lowest bricks of
 *       avail_mask other than i and j (the encode of the decode of those k
 *       chunks).  For one stripe that is ec_method_heal with mask = B_ij and
 *       target_mask = S.
 *   Every other value leaves stripe t byte for byte as it was: 0,
 *       EC_MI355X_LOCATE_MANY alone or ORed with anything, three or more
 *       bits, a pair with one brick outside avail_mask or at or above n.
 *       None of these is an error.
 * Only the named chunks are written: no other brick, nothing past
 * nstripes*512.
 *
 * With loc[] from ec_method_locate2 on the same frags and avail_mask, every
 * stripe that locate2 named with one or two bits is mutually consistent
 * afterwards and a second locate2 gives 0 for it.  With loc[] from
 * ec_method_locate, repair2 does what ec_method_repair does.  The a - k == 4
 * caveat of ec_method_locate2 carries over: three damaged chunks can imitate
 * a pair, and repair2 then writes what the code implies, not what was
 * originally stored.
 *
 * *nrepaired (host variant, may be NULL) = stripes rewritten, with one or two
 * chunks; *nskipped (may be NULL) = stripes with loc[t] != 0 that were left
 * alone.  The device variant counts nothing.
 *
 * -EINVAL: as ec_method_repair, with fewer than k + 2 bits in avail_mask.
 * nstripes == 0 returns 0 after these checks and touches nothing.
 *
 * The host variant runs on the calling thread's CPU engine whatever the
 * volume's engine is and leaves ec_method_stats_t, the router and the
 * run-time compiler alone; the device variant is asynchronous on `stream`
 * with no host synchronisation (every table travels in the kernel arguments,
 * so locate2 and repair2 can be queued back to back), pre-zeroes nothing and
 * uses no global atomics (-ENODEV where the device layer lacks it). */
int32_t ec_method_repair2(ec_matrix_list_t *list, uint64_t nstripes, uintptr_t avail_mask,
                          void *const *frags, const uint32_t *loc,
                          uint64_t *nrepaired, uint64_t *nskipped);
int32_t ec_method_repair2_device(ec_matrix_list_t *list, int device, void *stream,
                                 uint64_t nstripes, uintptr_t avail_mask,
                                 void *const *frags, const uint32_t *loc);

/* The report of a scrub: the last stage behind any call above that writes
 * loc[] or bad[].  Their device variants count nothing, which left a caller
 * to copy 4 bytes per stripe to the host, or to write a kernel, to learn what
 * it acts on: how many stripes are dirty, how many of them are
 * EC_MI355X_LOCATE_MANY (its -EIO), and which ones they are.  This call gives
 * exactly that, where loc[] lies.  It takes no list: loc[0..nstripes) is any
 * array of the family, from any volume (bad[] simply never has bit 31), and
 * is read and never written.
 *
 *   report->nbad      stripes with loc[t] != 0
 *   report->nmany     of those, stripes with bit 31 (EC_MI355X_LOCATE_MANY) set
 *   report->brick[i]  stripes with bit i of loc[t] set, i < 31
 *   report->listed    min(nbad, cap): the entries written to idx[] and val[]
 *   idx[r]            the index t of the r-th dirty stripe, ascending, r < listed
 *   val[r]            loc[idx[r]], r < listed
 * The counts are over all nstripes whatever cap is, so listed < nbad says that
 * the list was cut.  Nothing at or past listed is written.  val may be NULL
 * (indices only); idx may be NULL only when cap == 0 (counts only).  A word
 * with bit 31 and other bits counts once in nbad, once in nmany and in the
 * brick[i] of every bit it has, and is listed as it is.  The result is a
 * function of loc[] and cap alone, byte for byte: from run to run, and
 * between the host and the device variant.
 *
 * The device variant takes every buffer on `device` -- loc, report, idx, val
 * and work -- and is asynchronous on `stream`: it can be queued right behind
 * the call that writes loc[] with no host synchronisation, and the host then
 * copies 272 + 12 * listed bytes instead of 4 * nstripes.  It pre-zeroes
 * nothing, uploads nothing, allocates nothing and uses no global atomics, and
 * no block of it waits on another; every output word is written by one plain
 * store.  work is scratch of at least ec_method_scrub_report_work(nstripes)
 * bytes, 8-byte aligned; its content is undefined before and after the call,
 * and calls that may overlap in time need distinct work.
 * ec_method_scrub_report_work needs no device, is non-decreasing in nstripes
 * and is 0 only for nstripes == 0 (140 bytes per 4096 stripes, DESIGN.md
 * 3.24).
 *
 * -EINVAL: a NULL loc or report; loc or val not 4-byte aligned; report, idx
 * or work not 8-byte aligned; cap > 0 with a NULL idx; nstripes > 0 with a
 * NULL work or work_bytes too small; nstripes above 2^40 (device variant);
 * host and device buffers mixed, or given to the wrong entry point.
 * nstripes == 0 returns 0 after these checks and writes nothing, the report
 * included.  -ENODEV where the device layer lacks the call.
 *
 * The host variant is one loop on the calling thread; like the other scrub
 * host calls it leaves ec_method_stats_t, the router and the run-time
 * compiler alone. */
typedef struct {
    uint64_t nbad;    /* stripes with loc[t] != 0 */
    uint64_t nmany;   /* of those, stripes with EC_MI355X_LOCATE_MANY (bit 31) set */
    uint64_t listed;  /* entries written to idx[] / val[]: min(nbad, cap) */
    uint64_t brick[EC_MI355X_MAX_NODES]; /* brick[i] = stripes with bit i of loc[t] set */
} ec_method_scrub_report_t;              /* 272 bytes, no padding */

size_t ec_method_scrub_report_work(uint64_t nstripes);
int32_t ec_method_scrub_report(uint64_t nstripes, const uint32_t *loc,
                               ec_method_scrub_report_t *report, uint64_t cap, uint64_t *idx,
                               uint32_t *val);
int32_t ec_method_scrub_report_device(int device, void *stream, uint64_t nstripes,
                                      const uint32_t *loc, ec_method_scrub_report_t *report,
                                      uint64_t cap, uint64_t *idx, uint32_t *val, void *work,
                                      size_t work_bytes);

/* Partial-stripe write: the read-modify-write of
 * ec_writev_start (ec-inode-write.c:1987-2085) fused with ec_writev_encode.
 * The write's user data is the iovec list iov[0..count) (as the writev fop
 * carries it) and starts `head` bytes into its first stripe (fop->head =
 * offset % stripe, ec-inode-write.c:1833).  The encoded range is the
 * padded buffer of ec_writev_prepare_buffers (:1825-1848):
 *   bytes [0, head)                 old_head[0, head)      (head merge, :1883)
 *   bytes [head, head + user bytes) the user data
 *   the rest of the last stripe     the same bytes of old_tail (tail merge,
 *                                   :1898-1908)
 * old_head / old_tail are the current (decoded) contents of the first / last
 * stripe -- from the stripe cache or a read -- or NULL beyond end of file
 * (zeros, :2007-2008).  When the write lies in one stripe its old content
 * fills both ends (old_head, or old_tail when old_head is NULL).  out[i]
 * receives ceil((head + user bytes) / (512k)) chunks of fragment i.  The
 * merge happens in the staging copy for host buffers and inside the
 * kernel for device buffers (count must be 1 there); the interior of the
 * write is never copied separately.  Returns 0 or -errno. */
int32_t ec_method_writev_encode(ec_matrix_list_t *list, uint64_t head, const struct iovec *iov,
                                int count, const void *old_head, const void *old_tail,
                                void *const *out);

/* Read of an unaligned byte range: the read counterpart of the call above.
 * ec_readv rounds the offset of a read down to its stripe and keeps fop->head
 * = offset % stripe (ec-inode-read.c:1360-1362); after the decode it trims the
 * answer to the user's range by pointer arithmetic into its own buffer
 * (:1202-1217).  A caller whose destination is a buffer of exactly `size`
 * bytes, in device memory above all, has no such trick, and the whole-stripe
 * decode would write `head` bytes in front of it and the padding behind it.
 * These calls decode the stripes the range touches and write the bytes of the
 * range, no byte more.
 *
 * S = 512 * k is the stripe.  head < S is the offset of the first user byte
 * inside its stripe (fop->head); size is the sum of the iov_len (host
 * variant) or the argument (device variant), and ns = ceil((head + size) / S)
 * stripes are touched.  mask and in are as for the device-resident decode
 * below: mask has exactly k bits below n, in[p] is the fragment of the p-th
 * set bit, ns * 512 bytes long, and starts at the chunk of the stripe that
 * holds the first user byte.  With D the ns * S bytes that the whole-stripe
 * decode gives for those fragments and that mask, the call writes D[head ..
 * head + size): to dst[0 .. size) (device variant), or to the segments
 * iov[0 .. count) in order (host variant; segments of length 0 are allowed).
 *
 * No byte outside [dst, dst + size), or outside the segments, is written;
 * nothing of in[p] is read at or past ns * 512, and nothing in `in` is
 * written.  dst, every iov_base and the fragments may have any byte
 * alignment.  head == 0 with size % S == 0 is byte for byte the
 * device-resident decode and runs the same launch; every other range gives
 * the bytes that a decode into a temporary followed by a copy would give.
 * size == 0 returns 0 after the argument checks and writes nothing.
 *
 * -EINVAL: a NULL list, in, dst, or iov with count > 0; count < 0; a NULL
 * in[p]; a NULL iov_base with a non-zero length; head >= S; a mask that is
 * not exactly k bricks below n; host and device buffers mixed, or given to the
 * wrong entry point.  -ENODEV where the device layer lacks the call.
 *
 * The device variant is asynchronous on `stream` with no host
 * synchronisation.  It allocates nothing and uploads nothing -- inv(mask) and
 * the clip travel in the kernel arguments -- pre-zeroes nothing, uses no
 * global atomics and issues at most two launches: the whole-stripe combine
 * for the stripes that lie inside the range, unchanged, with its output at
 * dst + t * S - head, and one small kernel for the first and the last stripe
 * where the range covers them in part, which stores the covered bytes alone.
 *
 * The host variant runs on the calling thread's CPU engine whatever the
 * volume's engine is; like the scrub family's host calls it leaves
 * ec_method_stats_t, the router and the run-time compiler alone.  Interior
 * stripes that lie whole inside one segment are decoded straight into it; an
 * edge stripe, or one that a segment boundary cuts, is decoded into an S-byte
 * buffer on the stack and its live bytes are copied out.  It does not go to
 * the GPU because the host read of the xlator trims for free
 * (ec-inode-read.c:1202): this variant is the byte-exact specification, the
 * path of a CPU-only node and what runs without a GPU.  Large host reads keep
 * using the whole-stripe decode. */
int32_t ec_method_readv_decode(ec_matrix_list_t *list, uint64_t head, uintptr_t mask,
                               const void *const *in, const struct iovec *iov, int count);

/* Write of an unaligned byte range over stored fragments: the partial-stripe
 * write above for a caller that holds no decoded stripes.  ec_writev_start
 * takes the old content of the first and the last stripe from the stripe
 * cache or from an ec_readv (ec-inode-write.c:1987-2085); a caller that keeps
 * a file as fragments, in device memory above all, holds the stored chunks
 * and would decode each edge stripe into a temporary before
 * ec_method_writev_encode.  These calls take the old chunks as they are
 * stored, from any k bricks, decode what the write does not cover, merge and
 * encode in one pass, and may write the result over the chunks they read.
 *
 * S = 512 * k is the stripe.  head < S is the offset of the first user byte
 * inside its stripe (fop->head); size is the sum of the iov_len (host
 * variant) or the argument (device variant); end = head + size and ns =
 * ceil(end / S) stripes are written.  mask has exactly k bits below n, the
 * numbering of every decode mask.  old_head[p] is 512 bytes, the stored chunk
 * of the write's first stripe on the brick of the p-th set bit of mask, and
 * old_tail[p] the same for the last stripe.  Either array may be NULL: the
 * stripe then lies beyond end of file and reads as zeros (:2007-2008).  When
 * ns == 1 the stripe's old content is old_head, or old_tail when old_head is
 * NULL, the rule of ec_method_writev_encode.
 *
 * The first stripe, when head != 0 or end < S, is O0 -- the S bytes that
 * ec_method_decode gives for old_head and mask, or zeros -- with bytes [head,
 * min(end, S)) replaced by user bytes.  The last stripe, when ns > 1 and end %
 * S != 0, is O1 (from old_tail) with bytes [0, end % S) replaced.  Every other
 * stripe is user bytes alone.  out[i], i < n, indexed by brick, receives ns
 * chunks of fragment i, the encode of those ns * S bytes: byte for byte what
 * ec_method_writev_encode gives when handed the decoded O0 and O1.  out[] is
 * not modified.
 *
 * An old array is read only if its stripe is an edge in the sense above; each
 * old_*[p] is read for exactly 512 bytes and never written through that
 * pointer; nothing is written outside [out[i], out[i] + ns * 512).  The host
 * variant reads exactly the iov_len bytes of each segment.  The device variant
 * reads no byte of user outside the aligned dwords that hold the size bytes:
 * where the stripes that the write covers wholly do not start on a dword, the
 * encoder loads the dwords that cover them, as ec_method_writev_encode_device
 * does, so up to 3 bytes on either side, never another page; the edge stripes
 * read the user bytes alone.  user, every old_*[p] and every out[i] may have
 * any byte alignment.  n <= 31 (EC_MI355X_MAX_NODES), which ec_method_init
 * enforces for every list.
 *
 * In place: for a brick b in mask at position p, old_head[p] == out[b] is
 * allowed, and so is old_tail[p] == out[b] + (ns - 1) * 512 (with ns == 1 that
 * is old_tail[p] == out[b]): the stored chunk is then replaced by the new one.
 * Any other overlap between an old chunk and an output range, or between user
 * bytes and an output range, is undefined.
 *
 * mask is checked when either old array is non-NULL; with both NULL it is
 * ignored.  size == 0 returns 0 after the argument checks and writes nothing.
 * head == 0 with size % S == 0 reads no old chunk and is byte for byte
 * ec_method_encode_device (or _batch) of the user bytes.
 *
 * -EINVAL: a NULL list, out, out[i] (i < n), or user / iov with bytes to
 * write; count < 0; a NULL iov_base with a non-zero length; head >= S; an old
 * array given with a mask that is not exactly k bricks below n; a NULL entry
 * in an old array that is given; host and device buffers mixed, or given to
 * the wrong entry point.  Each leaves its reason in ec_method_last_error().
 * -ENODEV where the device layer lacks the call.
 *
 * The device variant is asynchronous on `stream` with no host
 * synchronisation.  It allocates nothing and uploads nothing -- the old chunk
 * pointers, inv(mask), the encode matrix and the clips travel in the kernel
 * arguments -- pre-zeroes nothing, uses no global atomics and issues at most
 * two launches: the encoder of ec_method_encode_device for the stripes that
 * the write covers wholly, its input at user + t * S - head, and one small
 * kernel for the first and the last stripe where the write covers them in
 * part.
 *
 * The host variant runs on the calling thread's CPU engine whatever the
 * volume's engine is; like ec_method_readv_decode it leaves
 * ec_method_stats_t, the router and the run-time compiler alone.  It decodes
 * both edge stripes into S-byte buffers on the stack before it writes any
 * output, then encodes the old head bytes, the segments in order (segments of
 * length 0 are allowed) and the old tail bytes with the CPU engine's gather
 * encoder; no interior byte is copied.  It is the byte-exact specification
 * and what runs without a GPU. */
int32_t ec_method_writev_rmw(ec_matrix_list_t *list, uint64_t head, const struct iovec *iov,
                             int count, uintptr_t mask, const void *const *old_head,
                             const void *const *old_tail, void *const *out);

/* Device-resident, asynchronous variants for callers that keep stripes in
 * MI355X memory: all buffers are device pointers on `device` (index among
 * the visible gfx950 devices), work is queued on `stream` (a hipStream_t;
 * NULL = the calling thread's per-thread default stream) and the call returns
 * without waiting.  The decode matrix travels in the kernel arguments, so no
 * host state outlives the call. */
int32_t ec_method_encode_device(ec_matrix_list_t *list, int device, void *stream,
                                uint64_t nstripes, const void *in, void *const *out);
int32_t ec_method_decode_device(ec_matrix_list_t *list, int device, void *stream,
                                uint64_t nstripes, uintptr_t mask,
                                const void *const *in, void *out);
/* group_pattern: device array of nstripes/group_stripes bytes indexing
 * masks[0..nmasks), nmasks <= 256 (ids >= nmasks are clamped to the last
 * mask).  Decode matrices that fit the 2 KiB kernel-argument segment travel
 * there; more go to a per-call device table, asynchronously on `stream`. */
int32_t ec_method_decode_mixed_device(ec_matrix_list_t *list, int device,
                                      void *stream, uint64_t nstripes,
                                      uint64_t group_stripes,
                                      const uint8_t *group_pattern,
                                      uint32_t nmasks, const uintptr_t *masks,
                                      const void *const *frags, void *out);
int32_t ec_method_heal_device(ec_matrix_list_t *list, int device, void *stream,
                              uint64_t nstripes, uintptr_t mask,
                              const void *const *in, uintptr_t target_mask,
                              void *const *out);
/* ec_method_encode_rows on device buffers: out[i] (indexed by brick) is
 * written for the bits of row_mask only; out[] is not modified. */
int32_t ec_method_encode_rows_device(ec_matrix_list_t *list, int device, void *stream,
                                     uint64_t nstripes, const void *in, uintptr_t row_mask,
                                     void *const *out);
int32_t ec_method_writev_encode_device(ec_matrix_list_t *list, int device, void *stream,
                                       uint64_t head, uint64_t size, const void *user,
                                       const void *old_head, const void *old_tail,
                                       void *const *out);
/* the unaligned read above on device buffers: dst gets exactly size bytes */
int32_t ec_method_readv_decode_device(ec_matrix_list_t *list, int device, void *stream,
                                      uint64_t head, uint64_t size, uintptr_t mask,
                                      const void *const *in, void *dst);
/* the unaligned write above on device buffers: user gives exactly size bytes */
int32_t ec_method_writev_rmw_device(ec_matrix_list_t *list, int device, void *stream,
                                    uint64_t head, uint64_t size, const void *user,
                                    uintptr_t mask, const void *const *old_head,
                                    const void *const *old_tail, void *const *out);
/* ec_method_heal_mixed on device buffers.  Group g uses pattern
 * group_pattern[g], a device array of a byte per group as for
 * ec_method_decode_mixed_device (ids >= npatterns are clamped to the last
 * pattern); pattern u is the pair (masks[u], target_masks[u]), host arrays
 * read during the call, npatterns <= 256 (-E2BIG beyond, -EINVAL for 0).
 * Every pattern is checked as the host call checks a group's pair, whether a
 * group uses it or not; every non-NULL fragment and group_pattern must be
 * memory of `device` (-EINVAL), and -ENODEV where the device layer lacks the
 * call.  One launch of one kernel, asynchronous on `stream`, with no host
 * synchronisation, no pre-zeroing and no atomics; patterns with different
 * numbers of targets may share a call.  Pattern sets that fit the 2 KiB
 * kernel-argument segment travel there; larger ones (64 masks of 16+4, up to
 * all 256 patterns of any geometry) go to a cached device table, uploaded on
 * `stream` the first time a set is seen. */
int32_t ec_method_heal_mixed_device(ec_matrix_list_t *list, int device, void *stream,
                                    uint64_t nstripes, uint64_t group_stripes,
                                    const uint8_t *group_pattern, uint32_t npatterns,
                                    const uintptr_t *masks, const uintptr_t *target_masks,
                                    void *const *frags);

/* Fused heal of many files in one call: ec_method_heal_mixed for windows that
 * arrive in buffers of their own (per-file reads, a pool of window buffers)
 * and cannot be laid end to end in one allocation per brick.  An extent is
 * one such window: nstripes stripes, the address of its fragment of every
 * brick, and the pattern -- the pair (masks[pattern], target_masks[pattern])
 * -- that heals it.  Its tiles of EC_MI355X_EXTENT_TILE stripes are numbered
 * after those of all earlier extents: `first` is their count, which
 * ec_method_extents_layout fills. */
#define EC_MI355X_EXTENT_TILE 4u          /* stripes per tile of an extent */

typedef struct {
    uint64_t frag[EC_MI355X_MAX_NODES + 1]; /* frag[i]: address of this extent's fragment of
                                               brick i (nstripes * 512 bytes), 0 = none */
    uint32_t first;     /* tiles of all earlier extents: sum of ceil(nstripes / 4) */
    uint32_t nstripes;  /* > 0 */
    uint32_t pattern;   /* index into masks[] / target_masks[] */
    uint32_t zero;      /* 0 */
} ec_method_extent_t;   /* 272 bytes, no padding */

/* Fill ext[e].first for e < nextents and return the total tile count.
 * Returns 0 for nextents == 0, and -EINVAL for NULL, nstripes == 0, or a total
 * above 2^31 - 1 (the table is then left as it was).  Needs no device. */
int64_t ec_method_extents_layout(uint64_t nextents, ec_method_extent_t *ext);

/* For every extent e, every stripe t < ext[e].nstripes and every brick i in
 * target_masks[ext[e].pattern], chunk t of ext[e].frag[i] becomes what
 * ec_method_heal gives for that stripe from the k bricks in
 * masks[ext[e].pattern], read from ext[e].frag[].  Nothing else is written and
 * source chunks are only read.  An extent whose pattern has an empty target
 * mask is neither read nor written, and all of its frag[] may be 0.  Extents
 * may come in any address order and may share source buffers that no extent
 * writes; a target chunk of one extent that is a source or target chunk of
 * another is undefined.
 * Pattern u is (masks[u], target_masks[u]), host arrays, npatterns <= 256; the
 * rules are those of ec_method_heal_mixed_device, and every pattern is checked
 * whether an extent uses it or not.
 * Host variant: ext and every fragment are host memory.  Runs on the calling
 * thread's CPU engine whatever the volume's engine is, extent by extent, and
 * leaves ec_method_get_stats alone: it is the byte-exact specification of the
 * device call below.
 * -EINVAL (with the reason in ec_method_last_error()): list, ext, masks or
 * target_masks NULL; npatterns == 0; a bad pattern; a record with nstripes ==
 * 0, a non-zero `zero`, a pattern at or above npatterns or a `first` that is
 * not the running sum; more than 2^31 - 1 tiles; frag[i] == 0 for a brick in
 * the mask or target mask of a pattern with targets; the table or such a
 * fragment in device memory.  -E2BIG: npatterns above 256.  nextents == 0
 * returns 0 after the pattern checks and touches nothing. */
int32_t ec_method_heal_extents(ec_matrix_list_t *list, uint64_t nextents,
                               const ec_method_extent_t *ext, uint32_t npatterns,
                               const uintptr_t *masks, const uintptr_t *target_masks);

/* ec_method_heal_extents on device buffers.  ext_dev: nextents records in
 * memory of `device` (8-byte aligned) that hold addresses on `device`; ntiles:
 * what ec_method_extents_layout returned for the table.  ext_host, when not
 * NULL, is the caller's host copy of the same table: it is checked in full as
 * the host call checks its table (fragments must be memory of `device`), and
 * ntiles must be its total; the caller promises that ext_dev holds the same
 * bytes.  ext_host == NULL is for tables written on the GPU: only the
 * patterns, nextents <= ntiles <= 2^31 - 1 and the table's own address are
 * checked, and a TABLE THAT BREAKS THE RULES ABOVE IS UNDEFINED BEHAVIOUR --
 * wrong `first` or nstripes, a 0 or foreign address for a brick that the
 * pattern names, overlapping targets.  Only a `pattern` at or above npatterns
 * is defined: it is clamped to the last pattern, as group_pattern ids are.
 * One launch of one kernel (ec_heal_extents_n, a block per tile, which finds
 * its extent by a binary search of the table), asynchronous on `stream`: no
 * host synchronisation, no allocation beyond the cached device table of a
 * pattern set that does not fit the 2 KiB kernel arguments, no pre-zeroing,
 * no atomics, and no block waits on another.  A call whose patterns all have
 * empty targets launches nothing.  ext_dev and the fragments must stay as they
 * are until the stream has run the call.  Non-temporal staging (calls that
 * read more than 256 MiB from 16-byte aligned fragments) needs ext_host.
 * -ENODEV where the device layer lacks the call; -EINVAL also for a table, a
 * host copy or a fragment on the wrong side. */
int32_t ec_method_heal_extents_device(ec_matrix_list_t *list, int device, void *stream,
                                      uint64_t nextents, uint64_t ntiles,
                                      const ec_method_extent_t *ext_dev,
                                      const ec_method_extent_t *ext_host,
                                      uint32_t npatterns, const uintptr_t *masks,
                                      const uintptr_t *target_masks);
int32_t ec_method_sync_device(int device, void *stream);

/* ------------------------------------------------------------------------
 * On-disk format guard (trusted.ec.config).
 *
 * The fragments this library writes are the reference's on-disk format bit
 * for bit: config version 0 (EC_CONFIG_VERSION, ec-common.h:22), algorithm 0
 * (the non-systematic Vandermonde code, ec-common.h:24), 8-bit GF words and
 * 512-byte chunks.  These helpers produce and check the xattr exactly as the
 * xlator does, so a volume coded on MI355X stays readable by CPU clients and
 * a brick written with any other layout is refused before it is decoded.
 * They need no GPU.
 * --------------------------------------------------------------------- */

/* The config a write stores for a volume of `bricks` = n bricks with
 * `redundancy` = n - k (ec-dir-write.c:144-151, ec-heal.c:1268-1275). */
void ec_method_config_fill(uint32_t bricks, uint32_t redundancy, ec_config_t *config);
/* Serialise to the 8-byte big-endian xattr value (ec_dict_set_config,
 * ec-helpers.c:298-330).  Returns 0, or -EINVAL for a version newer than 0. */
int32_t ec_method_config_pack(const ec_config_t *config, uint8_t value[8]);
/* Parse an xattr value (ec_dict_del_config, ec-helpers.c:333-380).  Returns 0,
 * -EINVAL (length != 8 or unsupported version) or -ENODATA (all zeros: the
 * xattr is absent, as the reference treats it). */
int32_t ec_method_config_unpack(const void *value, size_t len, ec_config_t *config);
/* ec_config_check (ec-common.c:1151-1195) for a volume of `bricks` bricks
 * with `redundancy` redundancy: 0 when the fragment layout is the one this
 * coder reads and writes, -EINVAL when the config is invalid or corrupted
 * (redundancy < 1, 2*redundancy >= bricks, gf_word_size not a power of two,
 * chunk bits not a multiple of word size x data bricks), -ENOTSUP when it is
 * well formed but describes another layout or geometry. */
int32_t ec_method_config_check(uint32_t bricks, uint32_t redundancy,
                               const ec_config_t *config);

/* ------------------------------------------------------------------------
 * Utilities.
 * --------------------------------------------------------------------- */

/* Number of visible gfx950 devices (0 = CPU engine only). */
int32_t ec_method_device_count(void);
/* NUMA node of gfx950 device `device` (-1: unknown or a one-node host,
 * -ENODEV: no such device): where a client should run the threads that
 * fill its buffers, and where ec_method_host_alloc places its pages. */
int32_t ec_method_device_numa_node(int32_t device);
/* CPU threads the library uses to stage pageable buffers: EC_COPY_THREADS,
 * else min(8, CPUs usable by the process -- affinity and cgroup quota). */
int32_t ec_method_copy_threads(void);
/* The engine a volume's coder runs ("gfx950 x8 + cpu/avx512", "cpu/avx2"...),
 * as logged by ec_method_init (cf. ec-code.c:1048-1053). */
const char *ec_method_engine(const ec_matrix_list_t *list);

/* Process-wide engine counters: host-buffer calls coded on a GPU, calls
 * coded by the CPU engine, and, among the latter, fallbacks after a failed
 * device submission.  A split call (r05: a GPU codes the first share of its
 * stripes, the calling thread's CPU engine the rest) adds 1 to both
 * gpu_calls and cpu_calls, so gpu_calls + cpu_calls counts engine runs, not
 * API calls; when its GPU share fails and is redone on the CPU engine,
 * cpu_fallbacks goes up and cpu_calls stays as the split left it. */
typedef struct {
    uint64_t gpu_calls;
    uint64_t cpu_calls;
    uint64_t cpu_fallbacks;
} ec_method_stats_t;
void ec_method_get_stats(ec_method_stats_t *stats);
/* Fault injection for tests (cf. debug/error-gen): the next `count`
 * host-buffer device submissions fail with -EIO before touching a device,
 * so the CPU fallback runs. */
void ec_method_inject_device_faults(uint32_t count);
/* HIP errors and the caller: every device entry point first clears any
 * non-sticky HIP error left pending on the calling thread
 * (hipGetLastError), so that its own launch checks see only its own
 * launches.  A caller that shares the thread's HIP runtime (torch, a
 * client's own kernels) must read its own pending error before calling in:
 * the library consumes it, and records it nowhere.
 *
 * Why the calling thread's last failing call failed (diagnostics): the
 * device layer's record (the HIP call or kernel and its error), or the
 * entry point and errno of a failure it did not record (an argument error).
 * Per thread: a client's epoll threads each read their own.  The text stays
 * until the thread's next failure ("" if it never failed; on a node without
 * a device, why none was used).  The pointer is valid until that thread's
 * next call into the library. */
const char *ec_method_last_error(void);
/* Pinned, device-mapped host memory.  Host buffers in such memory (16-byte
 * aligned) are coded in place by the GPU over PCIe with no staging copy;
 * pageable buffers are staged through pinned slots by CPU threads.  The
 * pages are placed on the NUMA node of the first host-buffer GPU
 * (EC_MI355X_HOST_DEVICES), as are the staging slots of each GPU. */
void *ec_method_host_alloc(size_t bytes);
void ec_method_host_free(void *p);
/* Pin and map an existing host range (e.g. a GlusterFS iobuf arena, see
 * INTEGRATION.md) so buffers inside it take the zero-copy path.  Returns 0
 * or -errno; -EEXIST for a range sharing a page with a live registration
 * (or inside the pinned pool): pages are mapped whole, and unregistering one
 * of two registrations of a page would unmap it under the other.  Unregister
 * before freeing the memory. */
int32_t ec_method_host_register(void *p, size_t bytes);
/* Unregister a range registered by either call below or above (a range still
 * waiting in the deferred queue is dropped; one being registered is waited
 * for).  Returns 0 or -errno. */
int32_t ec_method_host_unregister(void *p);
/* Deferred registration: queue the range for a library thread and return at
 * once (0 or -errno, -EEXIST as above, checked at once).  For callers holding a lock, such as GlusterFS's arena
 * hook, which runs under iobuf_pool->mutex (iobuf.c:157): until the thread has
 * registered the range, buffers in it are coded as pageable memory. */
int32_t ec_method_host_register_async(void *p, size_t bytes);
/* Wait until every queued registration has been done (tests, benchmarks). */
void ec_method_host_register_flush(void);

/* Pinned buffer pool for a client's own I/O buffers (the integration patch's
 * iobuf data allocator): pinned, device-mapped buffers of
 * any size up to 128 MiB, recycled by size class (4 KiB .. 1 MiB powers of
 * two, then 2 MiB steps), so hipHostRegister runs once per 2 MiB slab as the
 * pool grows and never per buffer.  At least 4 KiB aligned, contents not
 * cleared.  Returns NULL without a gfx950 device, for larger requests, or once
 * the pool's range (EC_POOL_MB, default 2048 MiB) is used up -- the caller
 * then allocates as it would without the pool. */
void *ec_method_buffer_get(size_t bytes);
/* Release a buffer: returns 1 when p came from ec_method_buffer_get (it is
 * back in the pool), 0 when it did not (the caller frees it). */
int32_t ec_method_buffer_put(void *p);

/* Host-call crossover probes (tests and tuning; no device needed).
 * ec_method_xover_route: would a host call of a volume with k data bricks go
 * to the CPU engine (1) or a GPU (0)?  op 0 = encode, 1 = decode-type; user
 * = user bytes, moved = bytes read + written, staged = bytes of its buffers
 * that are not pinned and mapped, inflight = bytes queued on the GPU.
 * ec_method_xover_observe feeds the router one completed call (engine 0 =
 * CPU, 1 = GPU with every buffer mapped, 2 = every buffer staged, 3 = some of
 * each; ns = its duration), as the library does after calls of >= 256 KiB;
 * ec_method_xover_reset forgets every observation.  -EINVAL on bad args. */
int32_t ec_method_xover_route(uint32_t k, int32_t op, uint64_t user, uint64_t moved,
                              uint64_t staged, uint64_t inflight);
/* Split calls (r05): the share of such a call's stripes, in thousandths, that
 * a GPU codes while the calling thread codes the rest on the CPU engine, or
 * -1 when the call stays whole (below 1 MiB of user data, one engine would
 * take under 15 %, or -- costed as if other large calls were in flight -- a
 * buffer that is not pinned and mapped: a real call with staged buffers
 * splits only while it is the only large host call).  Same arguments as
 * ec_method_xover_route. */
int32_t ec_method_xover_split(uint32_t k, int32_t op, uint64_t user, uint64_t moved,
                              uint64_t staged, uint64_t inflight);
/* Both decisions for a call with `others` large (>= 1 MiB) host calls in
 * flight beside it (r05): returns 0 (a GPU) or nonzero (the CPU engine; 2
 * when the call stages buffers and its staging copies would take at least the
 * CPU time coding it on the calling thread takes -- with other callers busy
 * the GPU route then frees no CPU; EC_STAGE_COPY_GBPS, default 10, is the
 * copy rate assumed, 0 turns the rule off), and, when `share` is not NULL,
 * the split share as ec_method_xover_split gives it (staged calls split only
 * when `others` is 0).  -EINVAL on bad args. */
int32_t ec_method_xover_plan(uint32_t k, int32_t op, uint64_t user, uint64_t moved,
                             uint64_t staged, uint64_t inflight, uint32_t others,
                             int32_t *share);
/* A split call as the library records one (r05, tests): `gpu_share` per
 * mille of the call's stripes took `gpu_ns` on a GPU from the hand-off, the
 * rest `cpu_ns` on the CPU engine.  The share later calls of this class,
 * width, size and provenance get moves toward the one that would have
 * balanced the two (ec_method.c share_learn; the first sample of a slot is
 * a cold start and dropped; ec_method_xover_reset forgets them).  -EINVAL on
 * bad args. */
int32_t ec_method_xover_observe_split(int32_t op, uint32_t k, uint64_t user, uint64_t moved,
                                      uint64_t staged, uint32_t gpu_share, uint64_t gpu_ns,
                                      uint64_t cpu_ns);
/* One engine's share of a split call as the library records it (r06, tests):
 * `part` of the call's `user` bytes took `ns` on `engine` (as in
 * ec_method_xover_observe).  The CPU's share is a sample of its rate inside
 * calls of `user` bytes; a GPU share, whose time holds the GPU's fixed latency
 * once, is recorded as the time the whole call would have taken (latency
 * from `staged` / `moved` as the router models it).  -EINVAL on bad args. */
int32_t ec_method_xover_observe_part(int32_t engine, int32_t op, uint32_t k, uint64_t user,
                                     uint64_t part, uint64_t ns, uint64_t staged,
                                     uint64_t moved);
int32_t ec_method_xover_observe(int32_t engine, int32_t op, uint32_t k, uint64_t user,
                                uint64_t ns);
void ec_method_xover_reset(void);

/* Pool and deferred-registration counters (times in microseconds). */
typedef struct {
    uint64_t pool_bytes;           /* pinned bytes the pool has grown to      */
    uint64_t in_use_bytes;         /* of which handed out now (class sizes)   */
    uint64_t gets;                 /* ec_method_buffer_get calls              */
    uint64_t misses;               /* of which returned NULL                  */
    uint64_t slabs;                /* slabs registered                        */
    uint64_t slab_register_us;     /* time to map, fault in and register them */
    uint64_t deferred_registers;   /* ranges registered by the library thread */
    uint64_t deferred_register_us; /* hipHostRegister time of those           */
    uint64_t deferred_register_failures;
    uint64_t unregisters;          /* ec_method_host_unregister calls done    */
    uint64_t unregister_us;        /* hipHostUnregister time of those         */
} ec_method_pool_stats_t;
void ec_method_pool_stats(ec_method_pool_stats_t *stats);

/* Per-pattern kernels compiled at run time (r06; the counterpart of the
 * reference's per-row JIT, ec-code.c:722-809).  A device-buffer combine with
 * one erasure pattern of a wide code (k >= 12 data and >= 12 output rows,
 * e.g. a 16+4 decode; >= EC_MI355X_JIT_MIN_STRIPES stripes, default 1024)
 * queues its coefficient matrix for compilation as one straight-line XOR
 * program over the whole matrix, and runs the shipped kernel until that code
 * exists; later calls of the matrix run it.  The compiler is a child process
 * (ec_jitc, installed next to the library; it alone loads hiprtc), one per
 * matrix, ~1-2 s; one library thread starts it and waits for it.  That thread
 * is neither stopped nor joined at exit: a process that exits mid-compile
 * leaves the child to finish on its own, and nothing of the compiler lives
 * in the client's address space.  Results are identical either way.
 * EC_MI355X_JIT=0 turns this off, EC_MI355X_JIT_SYNC=1 starts and waits for
 * the compiler on the calling thread.  Counters: */
typedef struct {
    uint64_t compiled;    /* matrices compiled                          */
    uint64_t failed;      /* compilations that failed (shipped kernel)  */
    uint64_t launches;    /* calls that ran a compiled kernel           */
    uint64_t compile_us;  /* time spent compiling                       */
    uint64_t lookups;     /* eligible calls                             */
    uint64_t entries;     /* matrices in the cache now (<= 32)          */
} ec_method_jit_stats_t;
void ec_method_jit_stats(ec_method_jit_stats_t *stats);
/* Queue the kernel of a rows x k coefficient matrix for compilation before
 * its first call (e.g. a heal daemon that knows the bricks it will read):
 * 0, -EPERM (EC_MI355X_JIT=0), -ENOSYS (no hiprtc), -ENOSPC (the per-process
 * compile budget is spent), -EINVAL.  Needs no device. */
int32_t ec_method_jit_prepare(uint32_t k, uint32_t rows, const uint8_t *coef);
/* Generate and compile (without loading) the kernel of a rows x k matrix of
 * GF(2^8) coefficients (row-major): returns its code size in bytes, or
 * -errno (-ENOSYS without hiprtc, -EIO when the compiler failed); *ops, when
 * not NULL, gets the program's XOR instructions per dword column.  Needs no
 * device (tests). */
int32_t ec_method_jit_compile_check(uint32_t k, uint32_t rows, const uint8_t *coef,
                                    uint32_t *ops);
/* The kernel source the compiler would read for a rows x k matrix, as text:
 * copies at most len - 1 bytes and a terminating 0 into buf (buf may be NULL
 * when len is 0) and returns the bytes needed, the terminator included, or
 * -EINVAL for the geometries ec_method_jit_compile_check rejects.  Pure text
 * generation: needs no compiler and no device (tests run the programs of
 * this text on the host, tests/test_jit_program.py). */
int32_t ec_method_jit_source(uint32_t k, uint32_t rows, const uint8_t *coef, char *buf,
                             size_t len);

/* Host-side matrix helpers, exported for tests and tools: the n x k encode
 * matrix (ec-method.c:22-36) and the k x k inverse for ascending rows
 * (ec-method.c:38-72), as uint32 values in [0, 255].  Return 0 or -EINVAL. */
int32_t ec_method_encode_matrix(uint32_t columns, uint32_t rows, uint32_t *matrix);
int32_t ec_method_inverse_matrix(uint32_t columns, const uint32_t *rows,
                                 uint32_t *matrix);
uint32_t ec_method_gf_mul(uint32_t a, uint32_t b);
uint32_t ec_method_gf_div(uint32_t a, uint32_t b);

#ifdef __cplusplus
}
#endif

#endif /* EC_MI355X_EC_METHOD_H */
