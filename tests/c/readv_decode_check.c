/* Stand-alone driver of the host variant of the ranged read
 * (ec_method_readv_decode) for sanitizer builds of the host layer around the
 * device-layer stub (tests/c/ecd_stub.c; see
 * tests/test_readv_decode_sanitized.py).  Every buffer is a heap block of
 * exactly the size the contract names: a fragment is ns * 512 bytes and a
 * segment its iov_len, so a byte read at or past ns * 512 of a fragment or
 * written outside a segment is an error report.  The bytes are compared with
 * ec_method_decode_batch of the same fragments into a temporary, sliced
 * [head, head + size), and with the data that was encoded. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/uio.h>

#include "ec_method.h"

#define CHUNK 512u
#define WINDOW 2u /* the fragments start this many chunks into the file */

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

/* one range of one mask: with one segment, then cut at two places into three
 * segments with an empty one between them */
static void
run_range(ec_matrix_list_t *list, uint32_t k, uintptr_t mask, const uint32_t *rows,
          uint8_t *const *full, const uint8_t *data, uint64_t head, uint64_t size)
{
    const uint64_t S = (uint64_t)k * CHUNK, ns = (head + size + S - 1) / S;
    const uint64_t first = head ? 1 : 0, whole = (head + size) / S;
    uint8_t *frag[16], *ref, *seg[4];
    const void *in[16];
    struct iovec iov[4];
    uint64_t len[4], c1, c2, at;
    uint32_t p;
    int v, i, n;

    for (p = 0; p < k; p++) {
        frag[p] = xmalloc(ns * CHUNK);
        memcpy(frag[p], full[p] + WINDOW * CHUNK, ns * CHUNK);
        in[p] = frag[p];
    }
    ref = xmalloc(ns * S);
    CHECK(ec_method_decode_batch(list, ns, mask, rows, in, ref) == 0);
    CHECK(memcmp(ref, data + WINDOW * S, ns * S) == 0);
    c1 = whole > first ? first * S - head + S / 2 + 1 : size / 3;
    c2 = c1 + (size - c1) / 2;
    for (v = 0; v < 2; v++) {
        n = v ? 4 : 1;
        len[0] = v ? c1 : size;
        len[1] = 0;
        len[2] = c2 - c1;
        len[3] = size - c2;
        for (i = 0; i < n; i++) {
            seg[i] = xmalloc(len[i]);
            memset(seg[i], 0xA5, len[i]);
            iov[i].iov_base = seg[i];
            iov[i].iov_len = len[i];
        }
        CHECK(ec_method_readv_decode(list, head, mask, in, iov, n) == 0);
        for (i = 0, at = head; i < n; at += len[i++])
            CHECK(memcmp(seg[i], ref + at, len[i]) == 0);
        CHECK(at == head + size);
        for (i = 0; i < n; i++)
            free(seg[i]);
    }
    for (p = 0; p < k; p++)
        CHECK(memcmp(frag[p], full[p] + WINDOW * CHUNK, ns * CHUNK) == 0);
    free(ref);
    for (p = 0; p < k; p++)
        free(frag[p]);
}

/* one geometry: encode a file, then every range with the k lowest bricks, the
 * k highest and a mask with a gap */
static void
run(uint32_t k, uint32_t n, const char *gen)
{
    const uint64_t S = (uint64_t)k * CHUNK, nst = 48;
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
    struct iovec none = {NULL, 0};

    memset(&list, 0, sizeof(list));
    CHECK(ec_method_init(NULL, &list, k, n, 2 * n, gen) == 0);
    data = xmalloc(nst * S);
    for (r = 0; r < nst * S; r++)
        data[r] = (uint8_t)(rand() >> 7);
    for (i = 0; i < n; i++)
        outs[i] = frag[i] = xmalloc(nst * CHUNK);
    CHECK(ec_method_encode_batch(&list, nst, data, outs) == 0);
    for (m = 0; m < 3; m++) {
        for (i = 0, p = 0; i < n; i++)
            if ((masks[m] >> i) & 1) {
                rows[p] = i + 1;
                full[p++] = frag[i];
            }
        CHECK(p == k);
        for (r = 0; r < sizeof(ranges) / sizeof(ranges[0]); r++)
            run_range(&list, k, masks[m], rows, full, data, ranges[r][0], ranges[r][1]);
        /* the empty range, and what is rejected before it */
        CHECK(ec_method_readv_decode(&list, 5, masks[m], (const void *const *)full, &none, 1) == 0);
        CHECK(ec_method_readv_decode(&list, 5, masks[m], (const void *const *)full, NULL, 0) == 0);
        CHECK(ec_method_readv_decode(&list, S, masks[m], (const void *const *)full, &none, 1) ==
              -EINVAL);
        CHECK(ec_method_readv_decode(&list, 5, masks[m] | ((uintptr_t)1 << n),
                                     (const void *const *)full, &none, 1) == -EINVAL);
    }
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
