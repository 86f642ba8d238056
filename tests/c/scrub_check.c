/* Stand-alone driver of the host variants of the scrub family that
 * tests/c/verified_check.c does not reach (ec_method_verify, locate, locate2,
 * repair, repair2, decode_checked, decode_checked2, heal_checked) for
 * sanitizer builds of the host layer around the device-layer stub
 * (tests/c/ecd_stub.c; see tests/test_scrub_sanitized.py).  Every buffer is a
 * heap block of exactly the size the contract names.  The shapes are the
 * smallest at which the steps these calls share can go wrong: k = 2 with a =
 * k + 2 (a = k + 4 for the `2` calls); 1, 32 and 33 stripes, that is one
 * window of the check pass, an exactly full one and a one-stripe tail; damage
 * at stripes 0, 31 and 32; neighbouring stripes that name different bricks,
 * so a run ends and the pattern is rebuilt; one stripe with more damage than
 * the call can name; and a call of zero stripes.  Expected data come from
 * ec_method_decode_batch / ec_method_heal on the undamaged fragments. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ec_method.h"

#define CHUNK 512u
#define K 2u
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
 * its own (so that no two errors can imitate one), and what the call under
 * test must say about it */
typedef struct {
    uint64_t stripe;
    uint32_t bricks, want;
} damage_t;

/* a = k + 2 = bricks 0..3, B = {0, 1}: one brick per stripe, 0 | 1 is MANY */
static const damage_t one_brick[] = {
    {0, 0x1, 0x1}, {1, 0x2, 0x2}, {5, 0x3, MANY}, {31, 0x4, 0x4}, {32, 0x2, 0x2},
};
/* a = k + 4 = bricks 0..5: pairs, one single brick, three bricks are MANY */
static const damage_t two_bricks[] = {
    {0, 0x3, 0x3}, {1, 0x20, 0x20}, {5, 0x7, MANY}, {31, 0x22, 0x22}, {32, 0x14, 0x14},
};

/* `two`: the calls for up to two bricks on n = 6 with every brick at hand;
 * else the single-brick calls on n = 5 with bricks 0..3 at hand and brick 4
 * the target of the heal */
static void
run(int two, uint64_t nst, const char *gen)
{
    const uint32_t n = two ? 6 : 5, a = two ? 6 : 4;
    const uintptr_t avail = ((uintptr_t)1 << a) - 1, bmask = 0x3, cmask = avail & ~bmask;
    const uintptr_t tmask = two ? 0 : 0x10;
    const damage_t *dmg = two ? two_bricks : one_brick;
    const size_t fb = (size_t)nst * CHUNK;
    ec_matrix_list_t list;
    uint8_t *data, *frag[6], *orig[6], *out, *asis, *hout, *href, *hasis;
    const void *frags[6], *in[K], *check[4], *nul[K];
    void *outs[6], *ho[1];
    uint32_t rows[K] = {1, 2}, *loc, *loc2, *bad, *want, i, b;
    uint64_t nbad, nmany, ndone, nskip, t, wbad = 0, wmany = 0;

    memset(&list, 0, sizeof(list));
    CHECK(ec_method_init(NULL, &list, K, n, 2 * n, gen) == 0);
    data = xmalloc(fb * K);
    for (i = 0; i < fb * K; i++)
        data[i] = (uint8_t)(rand() >> 7);
    for (i = 0; i < n; i++) {
        outs[i] = frag[i] = xmalloc(fb);
        orig[i] = xmalloc(fb);
    }
    CHECK(ec_method_encode_batch(&list, nst, data, outs) == 0);
    for (i = 0; i < n; i++) {
        memcpy(orig[i], frag[i], fb);
        frags[i] = i < a ? frag[i] : NULL;
        if (i < K)
            in[i] = frag[i];
        else if (i < a)
            check[i - K] = frag[i];
    }
    loc = xmalloc(nst * sizeof(*loc));
    loc2 = xmalloc(nst * sizeof(*loc));
    bad = xmalloc(nst * sizeof(*loc));
    want = xmalloc(nst * sizeof(*loc));
    out = xmalloc(fb * K);
    asis = xmalloc(fb * K);
    hout = xmalloc(fb);
    href = xmalloc(fb);
    hasis = xmalloc(fb);
    ho[0] = href;
    if (tmask)
        CHECK(ec_method_heal(&list, nst, bmask, in, tmask, ho) == 0);

    memset(want, 0, nst * sizeof(*want));
    for (i = 0; i < 5; i++) {
        if (dmg[i].stripe >= nst)
            continue;
        for (b = 0; b < a; b++)
            if ((dmg[i].bricks >> b) & 1)
                frag[b][dmg[i].stripe * CHUNK + 7 + 40 * b] ^= 0x5a;
        want[dmg[i].stripe] = dmg[i].want;
        wbad++;
        wmany += dmg[i].want == MANY;
    }
    /* what mask B gives from the chunks as stored: the answer for MANY */
    CHECK(ec_method_decode_batch(&list, nst, bmask, rows, in, asis) == 0);
    ho[0] = hasis;
    if (tmask)
        CHECK(ec_method_heal(&list, nst, bmask, in, tmask, ho) == 0);

    /* verify: damage in B sets every bit of C, damage in C its own bit */
    nbad = 77;
    CHECK(ec_method_verify(&list, nst, bmask, in, cmask, check, bad, &nbad) == 0);
    CHECK(nbad == (nst ? wbad : 77));
    for (i = 0; i < 5; i++)
        if (dmg[i].stripe < nst)
            CHECK(bad[dmg[i].stripe] ==
                  ((dmg[i].bricks & bmask) ? cmask : (dmg[i].bricks & cmask)));
    for (t = 0; t < nst; t++)
        CHECK((bad[t] != 0) == (want[t] != 0));
    CHECK(ec_method_verify(&list, nst, bmask, in, cmask, check, bad, NULL) == 0);
    /* a NULL entry: verify's argument check does not look, so zero stripes
     * return 0 and one stripe is -EINVAL */
    nul[0] = in[0];
    nul[1] = NULL;
    nbad = 77;
    CHECK(ec_method_verify(&list, 0, bmask, nul, cmask, check, bad, &nbad) == 0);
    CHECK(ec_method_verify(&list, 0, bmask, in, cmask, nul, bad, &nbad) == 0);
    if (nst) {
        CHECK(ec_method_verify(&list, nst, bmask, nul, cmask, check, bad, &nbad) == -EINVAL);
        CHECK(ec_method_verify(&list, nst, bmask, in, cmask, nul, bad, &nbad) == -EINVAL);
    }
    CHECK(nbad == 77);

    /* locate / locate2 */
    nbad = 77;
    CHECK((two ? ec_method_locate2 : ec_method_locate)(&list, nst, avail, frags, loc, &nbad) == 0);
    CHECK(nbad == (nst ? wbad : 77));
    CHECK(memcmp(loc, want, nst * sizeof(*loc)) == 0);
    CHECK((two ? ec_method_locate2 : ec_method_locate)(&list, nst, avail, frags, loc, NULL) == 0);

    /* decode_checked / decode_checked2 */
    nbad = nmany = 77;
    CHECK((two ? ec_method_decode_checked2 : ec_method_decode_checked)(
              &list, nst, avail, frags, out, loc2, &nbad, &nmany) == 0);
    CHECK(nbad == (nst ? wbad : 77) && nmany == (nst ? wmany : 77));
    CHECK(memcmp(loc2, want, nst * sizeof(*loc)) == 0);
    for (t = 0; t < nst; t++)
        CHECK(memcmp(out + t * K * CHUNK, (want[t] == MANY ? asis : data) + t * K * CHUNK,
                     K * CHUNK) == 0);
    CHECK((two ? ec_method_decode_checked2 : ec_method_decode_checked)(
              &list, nst, avail, frags, out, loc2, NULL, NULL) == 0);

    /* heal_checked */
    if (tmask) {
        ho[0] = hout;
        nbad = nmany = 77;
        memset(loc2, 0xff, nst * sizeof(*loc));
        CHECK(ec_method_heal_checked(&list, nst, avail, frags, tmask, ho, loc2, &nbad, &nmany) ==
              0);
        CHECK(nbad == (nst ? wbad : 77) && nmany == (nst ? wmany : 77));
        CHECK(memcmp(loc2, want, nst * sizeof(*loc)) == 0);
        for (t = 0; t < nst; t++)
            CHECK(memcmp(hout + t * CHUNK, (want[t] == MANY ? hasis : href) + t * CHUNK,
                         CHUNK) == 0);
        for (t = 0; t < nst; t++)
            CHECK(want[t] == MANY || memcmp(hout + t * CHUNK, orig[4] + t * CHUNK, CHUNK) == 0);
    }

    /* repair / repair2: what was named is as encoded again, MANY stays */
    ndone = nskip = 77;
    CHECK((two ? ec_method_repair2 : ec_method_repair)(&list, nst, avail, outs, loc, &ndone,
                                                        &nskip) == 0);
    CHECK(ndone == (nst ? wbad - wmany : 77) && nskip == (nst ? wmany : 77));
    for (i = 0; i < n; i++)
        for (t = 0; t < nst; t++)
            CHECK((memcmp(frag[i] + t * CHUNK, orig[i] + t * CHUNK, CHUNK) == 0) ==
                  !(want[t] == MANY && ((dmg[2].bricks >> i) & 1)));
    nbad = 77;
    CHECK((two ? ec_method_locate2 : ec_method_locate)(&list, nst, avail, frags, loc, &nbad) == 0);
    CHECK(nbad == (nst ? wmany : 77));
    for (t = 0; t < nst; t++)
        CHECK(loc[t] == (want[t] == MANY ? MANY : 0));

    free(loc);
    free(loc2);
    free(bad);
    free(want);
    free(out);
    free(asis);
    free(hout);
    free(href);
    free(hasis);
    free(data);
    for (i = 0; i < n; i++) {
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

    srand(7);
    for (g = 0; g < 2; g++)
        for (s = 0; s < 4; s++) {
            run(0, sizes[s], gens[g]);
            run(1, sizes[s], gens[g]);
        }
    printf("failures=%d\n", failures);
    return failures != 0;
}
