/* Stand-alone driver of ec_method_scrub_report, the host variant of the
 * report of a scrub, for sanitizer builds of the host layer around the
 * device-layer stub (tests/c/ecd_stub.c; see
 * tests/test_scrub_report_sanitized.py).  loc, idx and val are heap blocks of
 * exactly nstripes, cap and cap entries, so a read or a write one entry past
 * any of them is an error of the sanitizer; the report is a heap block of
 * exactly its 272 bytes.  Sizes on both sides of a wave (64) and of the device
 * tile (4096), which the host loop must not care about; clean, all dirty,
 * every 7th and first-and-last fills; caps 0, 1, nbad - 1, nbad, nbad + 7; val
 * NULL; a call of no stripes.  Expected values are counted here, one quantity
 * per loop.
 *
 * Mode `enodev` (any build around the stub): the stub has no ecd_scrub_report,
 * so the weak reference of ec_method.c is NULL and
 * ec_method_scrub_report_device answers -ENODEV for an otherwise valid call,
 * and 0 for one of no stripes. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ec_method.h"

#define MANY EC_MI355X_LOCATE_MANY

_Static_assert(sizeof(ec_method_scrub_report_t) == 272, "ec_method_scrub_report_t");

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

/* the dirty values: single bits, a pair, MANY, MANY with bits, all bits */
static const uint32_t values[] = {
    1u, 1u << 30, 1u << 5 | 1u << 17, MANY, MANY | 1u, MANY | 0x7FFFFFFFu, 0xFFFFFFFFu, 1u << 12,
};

static void
fill(uint32_t *loc, uint64_t n, int kind)
{
    uint64_t t;

    memset(loc, 0, n * sizeof(*loc));
    for (t = 0; t < n; t++) {
        const uint32_t v = values[(t * 5 + 3) % (sizeof(values) / sizeof(values[0]))];
        if (kind == 1 || (kind == 2 && t % 7 == 3) || (kind == 3 && (t == 0 || t == n - 1)))
            loc[t] = v;
    }
}

static void
one_call(const uint32_t *loc, uint64_t n, uint64_t cap, int with_val)
{
    ec_method_scrub_report_t *rep = xmalloc(sizeof(*rep));
    uint64_t *idx = cap ? xmalloc(cap * sizeof(*idx)) : NULL;
    uint32_t *val = cap && with_val ? xmalloc(cap * sizeof(*val)) : NULL;
    uint64_t t, r, nbad = 0, nmany = 0, listed;
    uint32_t i;

    memset(rep, 0xA5, sizeof(*rep));
    if (idx)
        memset(idx, 0xA5, cap * sizeof(*idx));
    if (val)
        memset(val, 0xA5, cap * sizeof(*val));
    CHECK(ec_method_scrub_report(n, loc, rep, cap, idx, val) == 0);

    for (t = 0; t < n; t++)
        nbad += loc[t] != 0;
    for (t = 0; t < n; t++)
        nmany += (loc[t] & MANY) != 0;
    listed = nbad < cap ? nbad : cap;
    CHECK(rep->nbad == nbad);
    CHECK(rep->nmany == nmany);
    CHECK(rep->listed == listed);
    for (i = 0; i < EC_MI355X_MAX_NODES; i++) {
        uint64_t c = 0;
        for (t = 0; t < n; t++)
            c += (loc[t] >> i) & 1u;
        CHECK(rep->brick[i] == c);
    }
    for (t = 0, r = 0; t < n && r < listed; t++) {
        if (loc[t] == 0)
            continue;
        CHECK(idx[r] == t);
        if (val)
            CHECK(val[r] == loc[t]);
        r++;
    }
    CHECK(r == listed);
    for (r = listed; r < cap; r++) {
        CHECK(idx[r] == 0xA5A5A5A5A5A5A5A5ull);
        if (val)
            CHECK(val[r] == 0xA5A5A5A5u);
    }
    free(val);
    free(idx);
    free(rep);
}

static void
host_variant(void)
{
    static const uint64_t sizes[] = {1, 2, 63, 64, 65, 4095, 4096, 4097, 8193};
    ec_method_scrub_report_t rep;
    uint64_t nbad, t, caps[5], idx1 = 7;
    uint32_t s, c, *loc;
    int kind;

    for (s = 0; s < sizeof(sizes) / sizeof(sizes[0]); s++) {
        const uint64_t n = sizes[s];
        loc = xmalloc(n * sizeof(*loc));
        for (kind = 0; kind < 4; kind++) {
            fill(loc, n, kind);
            for (t = 0, nbad = 0; t < n; t++)
                nbad += loc[t] != 0;
            caps[0] = 0;
            caps[1] = 1;
            caps[2] = nbad ? nbad - 1 : 0;
            caps[3] = nbad;
            caps[4] = nbad + 7;
            for (c = 0; c < 5; c++) {
                one_call(loc, n, caps[c], 1);
                one_call(loc, n, caps[c], 0);
            }
        }
        free(loc);
    }
    /* no stripes: 0, and nothing is written (loc is not read either) */
    loc = xmalloc(0);
    memset(&rep, 0xA5, sizeof(rep));
    CHECK(ec_method_scrub_report(0, loc, &rep, 1, &idx1, NULL) == 0);
    CHECK(rep.nbad == 0xA5A5A5A5A5A5A5A5ull && rep.brick[30] == 0xA5A5A5A5A5A5A5A5ull);
    CHECK(idx1 == 7);
    free(loc);
    /* the argument errors leave a reason behind */
    CHECK(ec_method_scrub_report(1, NULL, &rep, 0, NULL, NULL) == -EINVAL);
    CHECK(strstr(ec_method_last_error(), "ec_method_scrub_report") != NULL);
}

static void
enodev(void)
{
    ec_method_scrub_report_t rep;
    uint32_t loc[8] = {0, 1, 0, MANY, 0, 0, 2, 0}, val[4];
    uint64_t idx[4], work[64];
    const size_t need = ec_method_scrub_report_work(8);

    CHECK(need > 0 && need <= sizeof(work));
    memset(&rep, 0xA5, sizeof(rep));
    CHECK(ec_method_scrub_report_device(0, NULL, 8, loc, &rep, 4, idx, val, work, sizeof(work)) ==
          -ENODEV);
    CHECK(strstr(ec_method_last_error(), "ec_method_scrub_report_device") != NULL);
    CHECK(rep.nbad == 0xA5A5A5A5A5A5A5A5ull);
    /* the argument checks and the zero-stripes return come first */
    CHECK(ec_method_scrub_report_device(0, NULL, 8, loc, &rep, 4, NULL, val, work, sizeof(work)) ==
          -EINVAL);
    CHECK(ec_method_scrub_report_device(0, NULL, 8, loc, &rep, 4, idx, val, work, need - 1) ==
          -EINVAL);
    CHECK(ec_method_scrub_report_device(0, NULL, 0, loc, &rep, 4, idx, val, NULL, 0) == 0);
}

int
main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "enodev") == 0) {
        enodev();
        if (failures == 0)
            printf("enodev ok\n");
    } else {
        host_variant();
        enodev();
    }
    printf("failures=%d\n", failures);
    return failures != 0;
}
