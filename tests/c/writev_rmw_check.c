/* Stand-alone driver of the host variant of the ranged write
 * (ec_method_writev_rmw) for sanitizer builds of the host layer around the
 * device-layer stub (tests/c/ecd_stub.c; see
 * tests/test_writev_rmw_sanitized.py).  Every buffer is a heap block of
 * exactly the size the contract names: an old chunk is 512 bytes, an output ns
 * * 512, a segment its iov_len, so a byte read or written outside them is an
 * error report.  The fragments are compared with ec_method_encode_batch of the
 * merged stripes, which this program builds from ec_method_decode_batch of the
 * old chunks; the in-place form runs on the fragments of a whole file. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/uio.h>

#include "ec_method.h"

#define CHUNK 512u
#define WINDOW 2u /* the write starts this many stripes into the file */
#define NST 48u   /* stripes of the file */

static int failures;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            failures++;                                                            \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);                \
        }                                                                          \
    } while (0)

static void *
xmalloc(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (!p)
        abort();
    return p;
}

static void
fill(uint8_t *p, size_t n)
{
    size_t i;

    for (i = 0; i < n; i++)
        p[i] = (uint8_t)(rand() >> 7);
}

/* the S bytes that k old chunks decode to, or zeros without them */
static void
old_stripe(ec_matrix_list_t *list, uint32_t k, uintptr_t mask, const uint32_t *rows,
           uint8_t *const *old, uint8_t *dst)
{
    if (!old) {
        memset(dst, 0, (size_t)k * CHUNK);
        return;
    }
    CHECK(ec_method_decode_batch(list, 1, mask, rows, (const void *const *)old, dst) == 0);
}

/* One range of one mask.  variant 0: the old chunks are those of the file;
 * 1: arbitrary bytes; 2, 3, 4: no old_head, no old_tail, neither.  Each with
 * one segment, then cut at two places around an empty segment. */
static void
run_range(ec_matrix_list_t *list, uint32_t k, uint32_t n, uintptr_t mask, const uint32_t *rows,
          uint8_t *const *full, uint64_t head, uint64_t size, int variant)
{
    const uint64_t S = (uint64_t)k * CHUNK, end = head + size, ns = (end + S - 1) / S;
    uint8_t *oh[16], *ot[16], **ohp = oh, **otp = ot, *merged, *user, *seg[4];
    uint8_t *got[32], *ref[32];
    void *outs[32], *refs[32];
    struct iovec iov[4];
    uint64_t len[4], c1, c2, at;
    uint32_t p, i;
    int v, nseg, s;

    for (p = 0; p < k; p++) {
        oh[p] = xmalloc(CHUNK);
        ot[p] = xmalloc(CHUNK);
        if (variant == 0) {
            memcpy(oh[p], full[p] + WINDOW * CHUNK, CHUNK);
            memcpy(ot[p], full[p] + (WINDOW + ns - 1) * CHUNK, CHUNK);
        } else {
            fill(oh[p], CHUNK);
            fill(ot[p], CHUNK);
        }
    }
    if (variant == 2 || variant == 4)
        ohp = NULL;
    if (variant == 3 || variant == 4)
        otp = NULL;
    user = xmalloc(size);
    fill(user, size);
    /* what the call must encode */
    merged = xmalloc(ns * S);
    if (ns == 1) {
        old_stripe(list, k, mask, rows, ohp ? ohp : otp, merged);
    } else {
        old_stripe(list, k, mask, rows, ohp, merged);
        old_stripe(list, k, mask, rows, otp, merged + (ns - 1) * S);
    }
    memcpy(merged + head, user, size);
    for (i = 0; i < n; i++) {
        refs[i] = ref[i] = xmalloc(ns * CHUNK);
        outs[i] = got[i] = xmalloc(ns * CHUNK);
    }
    CHECK(ec_method_encode_batch(list, ns, merged, refs) == 0);
    c1 = size / 3;
    c2 = c1 + (size - c1) / 2;
    for (v = 0; v < 2; v++) {
        nseg = v ? 4 : 1;
        len[0] = v ? c1 : size;
        len[1] = 0;
        len[2] = c2 - c1;
        len[3] = size - c2;
        for (s = 0, at = 0; s < nseg; at += len[s++]) {
            seg[s] = xmalloc(len[s]);
            memcpy(seg[s], user + at, len[s]);
            iov[s].iov_base = seg[s];
            iov[s].iov_len = len[s];
        }
        for (i = 0; i < n; i++)
            memset(got[i], 0xA5, ns * CHUNK);
        CHECK(ec_method_writev_rmw(list, head, iov, nseg, variant == 4 ? 0 : mask,
                                   (const void *const *)ohp, (const void *const *)otp,
                                   outs) == 0);
        for (i = 0; i < n; i++)
            CHECK(memcmp(got[i], ref[i], ns * CHUNK) == 0);
        for (s = 0; s < nseg; s++)
            free(seg[s]);
    }
    for (i = 0; i < n; i++) {
        free(ref[i]);
        free(got[i]);
    }
    for (p = 0; p < k; p++) {
        free(oh[p]);
        free(ot[p]);
    }
    free(merged);
    free(user);
}

/* More segments than the call keeps on its stack: 70 of them, every third one
 * empty, the others of growing lengths with the rest in the last. */
static void
run_many_segments(ec_matrix_list_t *list, uint32_t k, uint32_t n, uintptr_t mask,
                  const uint32_t *rows, uint8_t *const *full)
{
    enum { NSEG = 70 };
    const uint64_t S = (uint64_t)k * CHUNK, head = 100, size = 5 * S + 33, ns = 6;
    uint8_t *oh[16], *ot[16], *merged, *user, *seg[NSEG], *got[32], *ref[32];
    void *outs[32], *refs[32];
    struct iovec iov[NSEG];
    uint64_t at = 0, len;
    uint32_t p, i;
    int s;

    for (p = 0; p < k; p++) {
        oh[p] = xmalloc(CHUNK);
        ot[p] = xmalloc(CHUNK);
        memcpy(oh[p], full[p] + WINDOW * CHUNK, CHUNK);
        memcpy(ot[p], full[p] + (WINDOW + ns - 1) * CHUNK, CHUNK);
    }
    user = xmalloc(size);
    fill(user, size);
    merged = xmalloc(ns * S);
    old_stripe(list, k, mask, rows, oh, merged);
    old_stripe(list, k, mask, rows, ot, merged + (ns - 1) * S);
    memcpy(merged + head, user, size);
    for (i = 0; i < n; i++) {
        refs[i] = ref[i] = xmalloc(ns * CHUNK);
        outs[i] = got[i] = xmalloc(ns * CHUNK);
        memset(got[i], 0xA5, ns * CHUNK);
    }
    CHECK(ec_method_encode_batch(list, ns, merged, refs) == 0);
    for (s = 0; s < NSEG; s++) {
        len = s == NSEG - 1 ? size - at : (s % 3 == 1 ? 0 : (uint64_t)(2 * s + 1));
        seg[s] = xmalloc(len);
        memcpy(seg[s], user + at, len);
        iov[s].iov_base = seg[s];
        iov[s].iov_len = len;
        at += len;
    }
    CHECK(at == size);
    CHECK(ec_method_writev_rmw(list, head, iov, NSEG, mask, (const void *const *)oh,
                               (const void *const *)ot, outs) == 0);
    for (i = 0; i < n; i++) {
        CHECK(memcmp(got[i], ref[i], ns * CHUNK) == 0);
        free(ref[i]);
        free(got[i]);
    }
    for (s = 0; s < NSEG; s++)
        free(seg[s]);
    for (p = 0; p < k; p++) {
        free(oh[p]);
        free(ot[p]);
    }
    free(merged);
    free(user);
}

/* the in-place form: out[b] points into the fragments of the whole file and
 * the old chunks are the chunks the call replaces */
static void
run_in_place(ec_matrix_list_t *list, uint32_t k, uint32_t n, uintptr_t mask, uint8_t *data,
             uint8_t *const *frag, uint64_t head, uint64_t size)
{
    const uint64_t S = (uint64_t)k * CHUNK, ns = (head + size + S - 1) / S;
    const void *oh[16], *ot[16];
    uint8_t *ref[32], *user;
    void *outs[32], *refs[32];
    struct iovec iov;
    uint32_t i, p;

    user = xmalloc(size);
    fill(user, size);
    memcpy(data + WINDOW * S + head, user, size);
    for (i = 0, p = 0; i < n; i++) {
        refs[i] = ref[i] = xmalloc(NST * CHUNK);
        outs[i] = frag[i] + WINDOW * CHUNK;
        if ((mask >> i) & 1) {
            oh[p] = frag[i] + WINDOW * CHUNK;
            ot[p++] = frag[i] + (WINDOW + ns - 1) * CHUNK;
        }
    }
    CHECK(ec_method_encode_batch(list, NST, data, refs) == 0);
    iov.iov_base = user;
    iov.iov_len = size;
    CHECK(ec_method_writev_rmw(list, head, &iov, 1, mask, oh, ot, outs) == 0);
    for (i = 0; i < n; i++) {
        CHECK(memcmp(frag[i], ref[i], NST * CHUNK) == 0);
        free(ref[i]);
    }
    free(user);
}

/* one geometry: encode a file, then every range with the k lowest bricks, the
 * k highest and a mask with a gap */
static void
run(uint32_t k, uint32_t n, const char *gen)
{
    const uint64_t S = (uint64_t)k * CHUNK;
    const uint64_t ranges[][2] = {
        {0, S}, {0, 3 * S},
        {0, 1}, {S - 1, 1}, {1, S - 2}, {3, 1}, {2, 4}, {4, 4}, {63, 2}, {64, 1}, {65, 3},
        {511, 2}, {512, 1}, {513, 510}, {10, 53}, {60, 4}, {10, 501}, {500, 12},
        {S - 1, 2}, {1, S - 1}, {5, 2 * S - 5}, {0, S + 1}, {0, 2 * S - 3},
        {7, 2 * S}, {S - 1, S + 2}, {100, 5 * S + 33}, {S / 2, 7 * S}, {333, 40 * S + 4095},
    };
    const uintptr_t low = ((uintptr_t)1 << k) - 1;
    const uintptr_t masks[3] = {low, low << (n - k), (((uintptr_t)1 << (k + 1)) - 1) & ~(uintptr_t)2};
    ec_matrix_list_t list;
    uint8_t *data, *frag[32], *full[16];
    void *outs[32];
    uint32_t rows[16], i, m, p;
    size_t r;
    int variant;
    struct iovec none = {NULL, 0};

    memset(&list, 0, sizeof(list));
    CHECK(ec_method_init(NULL, &list, k, n, 2 * n, gen) == 0);
    data = xmalloc(NST * S);
    fill(data, NST * S);
    for (i = 0; i < n; i++)
        outs[i] = frag[i] = xmalloc(NST * CHUNK);
    CHECK(ec_method_encode_batch(&list, NST, data, outs) == 0);
    for (m = 0; m < 3; m++) {
        for (i = 0, p = 0; i < n; i++)
            if ((masks[m] >> i) & 1) {
                rows[p] = i + 1;
                full[p++] = frag[i];
            }
        CHECK(p == k);
        for (r = 0; r < sizeof(ranges) / sizeof(ranges[0]); r++)
            for (variant = 0; variant < 5; variant++)
                run_range(&list, k, n, masks[m], rows, full, ranges[r][0], ranges[r][1],
                          variant);
        run_many_segments(&list, k, n, masks[m], rows, full);
        /* the empty write, and what is rejected before it */
        CHECK(ec_method_writev_rmw(&list, 5, &none, 1, masks[m], (const void *const *)full,
                                   NULL, outs) == 0);
        CHECK(ec_method_writev_rmw(&list, 5, NULL, 0, 0, NULL, NULL, outs) == 0);
        CHECK(ec_method_writev_rmw(&list, S, &none, 1, masks[m], (const void *const *)full,
                                   NULL, outs) == -EINVAL);
        CHECK(ec_method_writev_rmw(&list, 5, &none, 1, masks[m] | ((uintptr_t)1 << n),
                                   (const void *const *)full, NULL, outs) == -EINVAL);
        CHECK(ec_method_writev_rmw(&list, 5, &none, 1, ~(uintptr_t)0, NULL,
                                   (const void *const *)full, outs) == -EINVAL);
    }
    /* in place, last: every call changes the file */
    for (m = 0; m < 3; m++)
        for (r = 0; r < sizeof(ranges) / sizeof(ranges[0]); r++)
            run_in_place(&list, k, n, masks[m], data, frag, ranges[r][0], ranges[r][1]);
    free(data);
    for (i = 0; i < n; i++)
        free(frag[i]);
    ec_method_fini(&list);
}

int
main(void)
{
    static const char *gens[] = {"none", "auto"};
    unsigned g;

    srand(7);
    for (g = 0; g < 2; g++) {
        run(2, 3, gens[g]);
        run(3, 5, gens[g]);
        run(4, 6, gens[g]);
        run(5, 7, gens[g]);
        run(8, 12, gens[g]);
        run(16, 20, gens[g]);
    }
    printf("failures=%d\n", failures);
    return failures != 0;
}
