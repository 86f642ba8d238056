/* Stand-alone driver of the host variant of ec_method_heal_checked2 for
 * sanitizer builds of the host layer around the device-layer stub
 * (tests/c/ecd_stub.c; see tests/test_heal_checked2_sanitized.py), shaped like
 * tests/c/scrub_check.c.  Every buffer is a heap block of exactly the size the
 * contract names.  k = 2 on a 2+5 volume with bricks 0..5 at hand (a = k + 4)
 * and brick 6 healed; 0, 1, 32 and 33 stripes, that is no stripe, one window
 * of the check pass, an exactly full one and a one-stripe tail; damage at
 * stripes 0, 31 and 32; neighbouring stripes that name different sets, so a
 * run ends and the pattern is rebuilt; a pair of basis bricks, a pair of check
 * bricks, a basis and a check brick, one single brick, and one stripe with
 * three damaged chunks, which the call cannot name.  Expected data come from
 * ec_method_heal on the undamaged fragments and, for that stripe, on the
 * fragments as stored.  The stub has no device, so the device entry point must
 * turn host buffers away. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ec_method.h"

#define CHUNK 512u
#define K 2u
#define N 7u
#define A 6u
#define MANY EC_MI355X_LOCATE_MANY

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

/* what one stripe is damaged with: the bricks of `bricks`, each at a byte of
 * its own, and what the call must say about it */
static const struct {
    uint64_t stripe;
    uint32_t bricks, want;
} dmg[] = {
    {0, 0x3, 0x3}, {1, 0x20, 0x20}, {5, 0x7, MANY}, {31, 0x22, 0x22}, {32, 0x14, 0x14},
};

static void
run(uint64_t nst, const char *gen)
{
    const uintptr_t avail = ((uintptr_t)1 << A) - 1, bmask = 0x3, tmask = (uintptr_t)1 << A;
    const size_t fb = (size_t)nst * CHUNK;
    ec_matrix_list_t list;
    uint8_t *data, *frag[N], *orig[N], *hout, *href, *hasis;
    const void *frags[N], *in[K];
    void *outs[N], *ho[1];
    uint32_t *loc, *loc2, *want, i, b;
    uint64_t nbad, nmany, t, wbad = 0, wmany = 0;

    memset(&list, 0, sizeof(list));
    CHECK(ec_method_init(NULL, &list, K, N, 2 * N, gen) == 0);
    data = xmalloc(fb * K);
    for (i = 0; i < fb * K; i++)
        data[i] = (uint8_t)(rand() >> 7);
    for (i = 0; i < N; i++) {
        outs[i] = frag[i] = xmalloc(fb);
        orig[i] = xmalloc(fb);
    }
    CHECK(ec_method_encode_batch(&list, nst, data, outs) == 0);
    for (i = 0; i < N; i++) {
        memcpy(orig[i], frag[i], fb);
        frags[i] = i < A ? frag[i] : NULL;
        if (i < K)
            in[i] = frag[i];
    }
    loc = xmalloc(nst * sizeof(*loc));
    loc2 = xmalloc(nst * sizeof(*loc));
    want = xmalloc(nst * sizeof(*loc));
    hout = xmalloc(fb);
    href = xmalloc(fb);
    hasis = xmalloc(fb);
    ho[0] = href;
    CHECK(ec_method_heal(&list, nst, bmask, in, tmask, ho) == 0);
    CHECK(memcmp(href, orig[A], fb) == 0);

    memset(want, 0, nst * sizeof(*want));
    for (i = 0; i < 5; i++) {
        if (dmg[i].stripe >= nst)
            continue;
        for (b = 0; b < A; b++)
            if ((dmg[i].bricks >> b) & 1)
                frag[b][dmg[i].stripe * CHUNK + 7 + 40 * b] ^= 0x5a;
        want[dmg[i].stripe] = dmg[i].want;
        wbad++;
        wmany += dmg[i].want == MANY;
    }
    /* what mask B gives from the chunks as stored: the answer for MANY */
    ho[0] = hasis;
    CHECK(ec_method_heal(&list, nst, bmask, in, tmask, ho) == 0);

    ho[0] = hout;
    nbad = nmany = 77;
    memset(loc, 0xff, nst * sizeof(*loc));
    CHECK(ec_method_heal_checked2(&list, nst, avail, frags, tmask, ho, loc, &nbad, &nmany) == 0);
    CHECK(nbad == (nst ? wbad : 77) && nmany == (nst ? wmany : 77));
    CHECK(memcmp(loc, want, nst * sizeof(*loc)) == 0);
    for (t = 0; t < nst; t++) {
        CHECK(memcmp(hout + t * CHUNK, (want[t] == MANY ? hasis : href) + t * CHUNK, CHUNK) == 0);
        CHECK((want[t] == MANY) ==
              (memcmp(hout + t * CHUNK, orig[A] + t * CHUNK, CHUNK) != 0));
    }
    CHECK(ec_method_heal_checked2(&list, nst, avail, frags, tmask, ho, loc, NULL, NULL) == 0);
    /* its loc is locate2's */
    CHECK(ec_method_locate2(&list, nst, avail, frags, loc2, NULL) == 0);
    CHECK(memcmp(loc, loc2, nst * sizeof(*loc)) == 0);
    /* nothing but the target and loc was written */
    for (i = 0; i < A; i++)
        for (t = 0; t < nst; t++)
            CHECK((memcmp(frag[i] + t * CHUNK, orig[i] + t * CHUNK, CHUNK) != 0) ==
                  (want[t] != 0 && ((want[t] == MANY ? dmg[2].bricks : want[t]) >> i) & 1));
    /* a = k + 3 is too few, whatever the number of stripes */
    CHECK(ec_method_heal_checked2(&list, nst, avail >> 1, frags, tmask, ho, loc, NULL, NULL) ==
          -EINVAL);
    /* the device entry point: its argument checks, then host buffers are
     * turned away (no pointer is on a device here) */
    CHECK(ec_method_heal_checked2_device(&list, 0, NULL, 0, avail, frags, tmask, ho, loc) == 0);
    CHECK(ec_method_heal_checked2_device(&list, 0, NULL, 0, avail >> 1, frags, tmask, ho, loc) ==
          -EINVAL);
    if (nst)
        CHECK(ec_method_heal_checked2_device(&list, 0, NULL, nst, avail, frags, tmask, ho, loc) ==
              -EINVAL);

    free(loc);
    free(loc2);
    free(want);
    free(hout);
    free(href);
    free(hasis);
    free(data);
    for (i = 0; i < N; i++) {
        free(frag[i]);
        free(orig[i]);
    }
    ec_method_fini(&list);
}

int
main(void)
{
    static const char *gens[] = {"none", "auto"};
    static const uint64_t sizes[] = {0, 1, 32, 33};
    unsigned g, s;

    srand(11);
    for (g = 0; g < 2; g++)
        for (s = 0; s < 4; s++)
            run(sizes[s], gens[g]);
    printf("failures=%d\n", failures);
    return failures != 0;
}
