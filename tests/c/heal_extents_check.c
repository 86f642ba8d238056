/* Stand-alone driver of the host variant of the extent heal
 * (ec_method_heal_extents, ec_method_extents_layout) for sanitizer builds of
 * the host layer around the device-layer stub (tests/c/ecd_stub.c; see
 * tests/test_heal_extents_sanitized.py).  Every buffer is a heap block of
 * exactly the size the contract names: a fragment is its extent's nstripes *
 * 512 bytes, the table is nextents records, the mask and target arrays have
 * npatterns entries, and a brick that an extent's pattern does not name has no
 * buffer at all (frag[i] = 0), so a byte read or written outside them is an
 * error report.  Extents of 1, 2, 3, 4, 5, 7, 8 and 9 stripes on the pairs of
 * tests/_heal_mixed_cases.py, with an extent without targets and without
 * fragments among them; each target fragment is compared with ec_method_heal
 * of its extent, every other byte with a copy made before. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ec_method.h"

#define CHUNK 512u

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

/* the pairs of tests/_heal_mixed_cases.py patterns(k, n), duplicates included */
static uint32_t
table_pairs(uint32_t k, uint32_t n, uintptr_t *mask, uintptr_t *target)
{
    const uintptr_t low = ((uintptr_t)1 << k) - 1;
    const uintptr_t masks[3] = {low, low << (n - k), (low & ~(uintptr_t)2) | ((uintptr_t)1 << k)};
    uint32_t rest[32], nr, m, i, j, c = 0, end;

    for (i = 0; i < 3; i++) {
        for (j = 0, nr = 0; j < n; j++)
            if (!((masks[i] >> j) & 1))
                rest[nr++] = j;
        for (m = 0; m <= nr; m++)
            for (end = 0; end < 2; end++) {
                mask[c] = masks[i];
                target[c] = 0;
                for (j = 0; j < m; j++)
                    target[c] |= (uintptr_t)1 << rest[end ? nr - m + j : j];
                c++;
            }
    }
    return c;
}

/* One call: extent e has ns[e] stripes and pattern ids[e]. */
static void
run_call(ec_matrix_list_t *list, uint32_t n, uint32_t np, const uintptr_t *mask,
         const uintptr_t *target, uint32_t ne, const uint32_t *ns, const uint32_t *ids)
{
    ec_method_extent_t *ext = xmalloc(ne * sizeof(*ext));
    uintptr_t *pm = xmalloc(np * sizeof(*pm)), *pt = xmalloc(np * sizeof(*pt));
    uint8_t **was = xmalloc((size_t)ne * n * sizeof(*was));
    const void *in[16];
    void *out[32];
    uint8_t *ref[32];
    int64_t tiles = 0;
    uint32_t e, b, p, j;

    memcpy(pm, mask, np * sizeof(*pm));
    memcpy(pt, target, np * sizeof(*pt));
    memset(ext, 0, ne * sizeof(*ext));
    for (e = 0; e < ne; e++) {
        const uintptr_t need = pt[ids[e]] ? pm[ids[e]] | pt[ids[e]] : 0;

        ext[e].nstripes = ns[e];
        ext[e].pattern = ids[e];
        ext[e].first = 0xdeadbeef;
        tiles += (ns[e] + 3) / 4;
        for (b = 0; b < n; b++) {
            was[e * n + b] = NULL;
            if (!((need >> b) & 1))
                continue;
            was[e * n + b] = xmalloc(ns[e] * CHUNK);
            fill(was[e * n + b], ns[e] * CHUNK);
            ext[e].frag[b] = (uint64_t)(uintptr_t)xmalloc(ns[e] * CHUNK);
            memcpy((void *)(uintptr_t)ext[e].frag[b], was[e * n + b], ns[e] * CHUNK);
        }
    }
    CHECK(ec_method_extents_layout(ne, ext) == tiles);
    CHECK(ec_method_heal_extents(list, ne, ext, np, pm, pt) == 0);
    for (e = 0; e < ne; e++) {
        const uintptr_t gm = pm[ids[e]], gt = pt[ids[e]];

        if (gt) {
            for (b = 0, p = 0, j = 0; b < n; b++) {
                if ((gm >> b) & 1)
                    in[p++] = was[e * n + b];
                if ((gt >> b) & 1)
                    out[j++] = ref[b] = xmalloc(ns[e] * CHUNK);
            }
            CHECK(ec_method_heal(list, ns[e], gm, in, gt, out) == 0);
            for (b = 0; b < n; b++)
                if ((gt >> b) & 1) {
                    memcpy(was[e * n + b], ref[b], ns[e] * CHUNK);
                    free(ref[b]);
                }
        }
        for (b = 0; b < n; b++) {
            if (was[e * n + b])
                CHECK(memcmp((void *)(uintptr_t)ext[e].frag[b], was[e * n + b], ns[e] * CHUNK) ==
                      0);
            else
                CHECK(ext[e].frag[b] == 0);
            free((void *)(uintptr_t)ext[e].frag[b]);
            free(was[e * n + b]);
        }
    }
    free(was);
    free(pm);
    free(pt);
    free(ext);
}

static void
run(uint32_t k, uint32_t n, const char *gen)
{
    static const uint32_t sizes[] = {1, 2, 3, 6, 4, 5, 7, 8, 9};
    uintptr_t mask[3 * 2 * 17], target[3 * 2 * 17], *m257, *t257;
    ec_matrix_list_t list;
    ec_method_extent_t one, *two;
    uint32_t ids[9], many_ns[130], many_ids[130], np, e, c;

    memset(&list, 0, sizeof(list));
    CHECK(ec_method_init(NULL, &list, k, n, 2 * n, gen) == 0);
    np = table_pairs(k, n, mask, target);
    /* neighbours on different patterns, and pattern 0 (no target) fourth */
    for (e = 0; e < 9; e++)
        ids[e] = e == 3 ? 0 : (np - 1 - e * 3) % np;
    CHECK(target[0] == 0);
    run_call(&list, n, np, mask, target, 9, sizes, ids);
    /* one extent, and many small ones */
    run_call(&list, n, np, mask, target, 1, sizes + 8, ids + 8);
    for (e = 0; e < 130; e++) {
        many_ns[e] = 1 + e % 2;
        many_ids[e] = (e * 5 + 1) % np;
    }
    run_call(&list, n, np, mask, target, 130, many_ns, many_ids);
    /* no extents: the patterns are still checked, the table is not read */
    CHECK(ec_method_heal_extents(&list, 0, &one, np, mask, target) == 0);
    CHECK(ec_method_extents_layout(0, NULL) == 0);
    CHECK(ec_method_extents_layout(1, NULL) == -EINVAL);
    CHECK(ec_method_heal_extents(NULL, 0, &one, np, mask, target) == -EINVAL);
    CHECK(ec_method_heal_extents(&list, 0, NULL, np, mask, target) == -EINVAL);
    CHECK(ec_method_heal_extents(&list, 0, &one, np, NULL, target) == -EINVAL);
    CHECK(ec_method_heal_extents(&list, 0, &one, np, mask, NULL) == -EINVAL);
    CHECK(ec_method_heal_extents(&list, 0, &one, 0, mask, target) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "no patterns") != NULL);
    /* the records */
    memset(&one, 0, sizeof(one));
    one.nstripes = 1;
    one.pattern = 0;                      /* no target: no fragment is needed */
    CHECK(ec_method_heal_extents(&list, 1, &one, np, mask, target) == 0);
    one.pattern = np;
    CHECK(ec_method_heal_extents(&list, 1, &one, np, mask, target) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "not below npatterns") != NULL);
    one.pattern = 2;                      /* a target, and every fragment 0 */
    CHECK(ec_method_heal_extents(&list, 1, &one, np, mask, target) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "is 0") != NULL);
    one.pattern = 0;
    one.zero = 7;
    CHECK(ec_method_heal_extents(&list, 1, &one, np, mask, target) == -EINVAL);
    one.zero = 0;
    one.first = 1;
    CHECK(ec_method_heal_extents(&list, 1, &one, np, mask, target) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "tiles before it") != NULL);
    one.first = 0;
    one.nstripes = 0;
    CHECK(ec_method_heal_extents(&list, 1, &one, np, mask, target) == -EINVAL);
    CHECK(ec_method_extents_layout(1, &one) == -EINVAL);
    two = xmalloc(2 * sizeof(*two));
    memset(two, 0, 2 * sizeof(*two));
    two[0].nstripes = two[1].nstripes = 0xffffffffu;
    two[1].first = 3;
    CHECK(ec_method_extents_layout(2, two) == -EINVAL && two[1].first == 3);
    two[1].nstripes = 0xfffffffcu;
    CHECK(ec_method_extents_layout(2, two) == 0x7fffffff && two[1].first == 0x40000000u);
    free(two);
    /* a target in its mask, and 257 patterns */
    m257 = xmalloc(257 * sizeof(*m257));
    t257 = xmalloc(257 * sizeof(*t257));
    for (c = 0; c < 257; c++) {
        m257[c] = mask[0];
        t257[c] = 0;
    }
    one.nstripes = 1;
    CHECK(ec_method_heal_extents(&list, 1, &one, 256, m257, t257) == 0);
    CHECK(ec_method_heal_extents(&list, 1, &one, 257, m257, t257) == -E2BIG);
    t257[255] = 1;
    CHECK(ec_method_heal_extents(&list, 1, &one, 256, m257, t257) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "ec_method_heal_extents: a target mask overlaps") != NULL);
    free(m257);
    free(t257);
    ec_method_fini(&list);
}

int
main(void)
{
    static const char *gens[] = {"none", "auto"};
    unsigned g;

    srand(13);
    for (g = 0; g < 2; g++) {
        run(2, 3, gens[g]);
        run(4, 6, gens[g]);
        run(5, 7, gens[g]);
        run(8, 12, gens[g]);
        run(16, 20, gens[g]);
    }
    printf("failures=%d\n", failures);
    return failures != 0;
}
