/* Stand-alone driver of the host variant of the mixed heal
 * (ec_method_heal_mixed) for sanitizer builds of the host layer around the
 * device-layer stub (tests/c/ecd_stub.c; see
 * tests/test_heal_mixed_sanitized.py).  Every buffer is a heap block of
 * exactly the size the contract names: a fragment is nstripes * 512 bytes, the
 * mask and target arrays have one entry per group and the fragment list n, so
 * a byte read or written outside them is an error report.  The table is the
 * one of tests/_heal_mixed_cases.py: six geometries, three masks, target sets
 * of every size from both ends of the bricks outside the mask, six stripe
 * counts and three group sizes.  Each target chunk is compared with
 * ec_method_heal of its group, every other byte with a copy made before. */
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

typedef struct {
    uintptr_t mask, target;
} pair_t;

/* the pairs of tests/_heal_mixed_cases.py patterns(k, n), duplicates included */
static uint32_t
table_pairs(uint32_t k, uint32_t n, pair_t *out)
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
                out[c].mask = masks[i];
                out[c].target = 0;
                for (j = 0; j < m; j++)
                    out[c].target |= (uintptr_t)1 << rest[end ? nr - m + j : j];
                c++;
            }
    }
    return c;
}

/* One call: group g has pair ids[g].  `spare` frees the list entries of the
 * bricks that no group with a target names, which then are NULL. */
static void
run_call(ec_matrix_list_t *list, uint32_t k, uint32_t n, const pair_t *pairs, const uint32_t *ids,
         uint64_t ns, uint64_t gs, int spare)
{
    const uint64_t ng = (ns + gs - 1) / gs;
    uintptr_t *gm = xmalloc(ng * sizeof(*gm)), *gt = xmalloc(ng * sizeof(*gt)), used = 0;
    void **frags = xmalloc(n * sizeof(*frags));
    uint8_t *was[32], *ref[32];
    const void *in[16];
    void *out[32];
    uint64_t g, lo, cnt;
    uint32_t b, p, j;

    for (g = 0; g < ng; g++) {
        gm[g] = pairs[ids[g]].mask;
        gt[g] = pairs[ids[g]].target;
        if (gt[g])
            used |= gm[g] | gt[g];
    }
    for (b = 0; b < n; b++) {
        was[b] = xmalloc(ns * CHUNK);
        fill(was[b], ns * CHUNK);
        frags[b] = NULL;
        if (!spare || ((used >> b) & 1)) {
            frags[b] = xmalloc(ns * CHUNK);
            memcpy(frags[b], was[b], ns * CHUNK);
        }
    }
    CHECK(ec_method_heal_mixed(list, ns, gs, gm, gt, frags) == 0);
    for (g = 0; g < ng; g++) {
        lo = g * gs;
        cnt = lo + gs < ns ? gs : ns - lo;
        if (!gt[g])
            continue;
        for (b = 0, p = 0, j = 0; b < n; b++) {
            if ((gm[g] >> b) & 1)
                in[p++] = was[b] + lo * CHUNK;
            if ((gt[g] >> b) & 1)
                out[j++] = ref[b] = xmalloc(cnt * CHUNK);
        }
        CHECK(ec_method_heal(list, cnt, gm[g], in, gt[g], out) == 0);
        for (b = 0; b < n; b++)
            if ((gt[g] >> b) & 1) {
                CHECK(memcmp((uint8_t *)frags[b] + lo * CHUNK, ref[b], cnt * CHUNK) == 0);
                /* the rest of the fragment is compared with `was` below */
                memcpy(was[b] + lo * CHUNK, ref[b], cnt * CHUNK);
                free(ref[b]);
            }
    }
    for (b = 0; b < n; b++) {
        if (frags[b])
            CHECK(memcmp(frags[b], was[b], ns * CHUNK) == 0);
        free(frags[b]);
        free(was[b]);
    }
    free(frags);
    free(gm);
    free(gt);
}

static void
run(uint32_t k, uint32_t n, const char *gen)
{
    static const uint64_t stripes[] = {4, 5, 7, 8, 37, 67}, groups[] = {4, 8, 16};
    pair_t pairs[3 * 2 * 17], *many;
    ec_matrix_list_t list;
    uint32_t ids[67], np, s, q, g, shape = 0, c;
    uintptr_t m, t;
    void *one[32] = {NULL};
    uintptr_t gm1, gt1;

    memset(&list, 0, sizeof(list));
    CHECK(ec_method_init(NULL, &list, k, n, 2 * n, gen) == 0);
    np = table_pairs(k, n, pairs);
    for (s = 0; s < 6; s++)
        for (q = 0; q < 3; q++, shape++) {
            for (g = 0; g < 67; g++)
                ids[g] = g == 1 ? 0 : (np - 1 + np * 67 - (g / 2) * (1 + np / 7) - shape) % np;
            run_call(&list, k, n, pairs, ids, stripes[s], groups[q], 0);
            run_call(&list, k, n, pairs, ids, stripes[s], groups[q], 1);
        }
    /* groups without targets only: no fragment at all */
    gm1 = pairs[0].mask;
    gt1 = 0;
    CHECK(ec_method_heal_mixed(&list, 4, 4, &gm1, &gt1, one) == 0);
    /* no stripes, and what is rejected before that */
    gt1 = (uintptr_t)1 << k;
    CHECK(ec_method_heal_mixed(&list, 0, 4, &gm1, &gt1, one) == 0);
    CHECK(ec_method_heal_mixed(&list, 0, 2, &gm1, &gt1, one) == -EINVAL);
    CHECK(ec_method_heal_mixed(&list, 0, 12, &gm1, &gt1, one) == -EINVAL);
    CHECK(ec_method_heal_mixed(&list, 0, 4, NULL, &gt1, one) == -EINVAL);
    CHECK(ec_method_heal_mixed(&list, 0, 4, &gm1, NULL, one) == -EINVAL);
    CHECK(ec_method_heal_mixed(&list, 0, 4, &gm1, &gt1, NULL) == -EINVAL);
    /* a NULL fragment, a target in its mask or outside the volume, a short mask */
    CHECK(ec_method_heal_mixed(&list, 4, 4, &gm1, &gt1, one) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "is NULL") != NULL);
    gt1 = 1;
    CHECK(ec_method_heal_mixed(&list, 4, 4, &gm1, &gt1, one) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "overlaps") != NULL);
    gt1 = (uintptr_t)1 << n;
    CHECK(ec_method_heal_mixed(&list, 4, 4, &gm1, &gt1, one) == -EINVAL);
    gm1 &= gm1 - 1;
    gt1 = 0;
    CHECK(ec_method_heal_mixed(&list, 4, 4, &gm1, &gt1, one) == -EINVAL);
    /* 256 distinct pairs pass and 257 are too many, where the geometry has them */
    if (k == 8) {
        many = xmalloc(257 * sizeof(*many));
        for (c = 0, m = 0; c < 257; m++) {
            for (t = m, g = 0; t; t &= t - 1)
                g++;
            if (g != k || (m >> n))
                continue;
            /* every brick outside the mask, or the lowest of them */
            t = (((uintptr_t)1 << n) - 1) & ~m;
            many[c].mask = m;
            many[c].target = c % 2 ? t : t & (~t + 1);
            c++;
        }
        {
            uint32_t *idm = xmalloc(257 * sizeof(*idm));
            uintptr_t *gm = xmalloc(257 * sizeof(*gm)), *gt = xmalloc(257 * sizeof(*gt));
            void *fr[32];

            for (c = 0; c < 257; c++) {
                idm[c] = c;
                gm[c] = many[c].mask;
                gt[c] = many[c].target;
            }
            run_call(&list, k, n, many, idm, 256 * 4, 4, 0);
            for (c = 0; c < n; c++)
                fr[c] = xmalloc(257 * 4 * CHUNK);
            CHECK(ec_method_heal_mixed(&list, 257 * 4, 4, gm, gt, fr) == -E2BIG);
            for (c = 0; c < n; c++)
                free(fr[c]);
            free(idm);
            free(gm);
            free(gt);
        }
        free(many);
    }
    ec_method_fini(&list);
}

int
main(void)
{
    static const char *gens[] = {"none", "auto"};
    unsigned g;

    srand(11);
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
