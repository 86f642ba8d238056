/* Stand-alone driver of the host variants of the detect-only read and heal
 * (ec_method_decode_verified, ec_method_heal_verified) for sanitizer builds
 * of the host layer around the device-layer stub (tests/c/ecd_stub.c; see
 * tests/test_verified_sanitized.py).  Every buffer is a heap block of exactly
 * the size the contract names, so a byte written past out + nstripes*k*512,
 * past nstripes*512 of an out[j] or past bad[nstripes) is an error report.
 * The results are compared with ec_method_decode_batch / ec_method_heal with
 * mask B and ec_method_verify with B and C on the same buffers. */
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

/* one geometry: encode, damage a basis chunk, a check chunk and the last
 * stripe, run both calls, compare */
static void
run(uint32_t k, uint32_t n, uintptr_t avail, uintptr_t tmask, uint64_t nst, const char *gen)
{
    ec_matrix_list_t list;
    uint8_t *data, *frag[32], *out, *ref, *hout[32], *href[32];
    const void *frags[32], *in[16], *check[32];
    void *outs[32], *refs[32];
    uint32_t rows[16], *bad, *badh, *badr, nb = 0, nc = 0, nt = 0, i, j;
    uintptr_t bmask = 0, cmask = 0;
    uint64_t nbad = 77, nbadh = 77, nbadr = 77, t;
    size_t fb = (size_t)nst * CHUNK;

    memset(&list, 0, sizeof(list));
    CHECK(ec_method_init(NULL, &list, k, n, 2 * n, gen) == 0);
    data = xmalloc(fb * k);
    for (i = 0; i < fb * k; i++)
        data[i] = (uint8_t)(rand() >> 7);
    for (i = 0; i < n; i++)
        outs[i] = frag[i] = xmalloc(fb);
    CHECK(ec_method_encode_batch(&list, nst, data, outs) == 0);
    for (i = 0; i < n; i++) {
        frags[i] = NULL;
        if (!((avail >> i) & 1))
            continue;
        frags[i] = frag[i];
        if (nb < k) {
            bmask |= (uintptr_t)1 << i;
            rows[nb] = i + 1;
            in[nb++] = frag[i];
        } else {
            cmask |= (uintptr_t)1 << i;
            check[nc++] = frag[i];
        }
    }
    if (nst > 0) {
        ((uint8_t *)in[k - 1])[(nst / 2) * CHUNK + 77] ^= 0x20;
        ((uint8_t *)check[nc - 1])[(nst - 1) * CHUNK + 511] ^= 0x01;
    }
    bad = xmalloc(nst * sizeof(*bad));
    badh = xmalloc(nst * sizeof(*bad));
    badr = xmalloc(nst * sizeof(*bad));
    out = xmalloc(fb * k);
    ref = xmalloc(fb * k);

    CHECK(ec_method_decode_verified(&list, nst, avail, frags, out, bad, &nbad) == 0);
    CHECK(ec_method_decode_batch(&list, nst, bmask, rows, in, ref) == 0);
    CHECK(ec_method_verify(&list, nst, bmask, in, cmask, check, badr, &nbadr) == 0);
    if (nst > 0) {
        CHECK(memcmp(out, ref, fb * k) == 0);
        CHECK(memcmp(bad, badr, nst * sizeof(*bad)) == 0);
        CHECK(nbad == nbadr && nbad == (nst > 1 ? 2u : 1u));
        CHECK(bad[nst / 2] == (uint32_t)cmask);
        for (t = 0; t < nst; t++)
            CHECK((memcmp(out + t * k * CHUNK, data + t * k * CHUNK, k * CHUNK) == 0) ==
                  (t != nst / 2));
    } else {
        CHECK(nbad == 77);
    }
    CHECK(ec_method_decode_verified(&list, nst, avail, frags, out, bad, NULL) == 0);

    if (tmask) {
        for (j = 0; j < n; j++)
            if ((tmask >> j) & 1) {
                outs[nt] = hout[nt] = xmalloc(fb);
                refs[nt] = href[nt] = xmalloc(fb);
                nt++;
            }
        CHECK(ec_method_heal_verified(&list, nst, avail, frags, tmask, outs, badh, &nbadh) == 0);
        CHECK(ec_method_heal(&list, nst, bmask, in, tmask, refs) == 0);
        if (nst > 0) {
            CHECK(memcmp(badh, badr, nst * sizeof(*bad)) == 0);
            CHECK(nbadh == nbadr);
            for (j = 0; j < nt; j++)
                CHECK(memcmp(hout[j], href[j], fb) == 0);
        }
        for (j = 0; j < nt; j++) {
            free(hout[j]);
            free(href[j]);
        }
    } else {
        /* no brick is left to heal: the heal is rejected and writes nothing */
        outs[0] = out;
        CHECK(ec_method_heal_verified(&list, nst, avail, frags, (uintptr_t)1 << (n - 1), outs,
                                      badh, &nbadh) == -EINVAL);
        CHECK(nbadh == 77);
    }
    /* a = k: both are rejected */
    outs[0] = out;
    CHECK(ec_method_decode_verified(&list, nst, bmask, frags, out, bad, &nbad) == -EINVAL);
    CHECK(ec_method_heal_verified(&list, nst, bmask, frags, cmask, outs, bad, &nbad) == -EINVAL);

    free(bad);
    free(badh);
    free(badr);
    free(out);
    free(ref);
    free(data);
    for (i = 0; i < n; i++)
        free(frag[i]);
    ec_method_fini(&list);
}

int
main(void)
{
    static const char *gens[] = {"none", "auto"};
    static const uint64_t sizes[] = {0, 1, 5, 67};
    unsigned g, s;

    srand(5);
    for (g = 0; g < 2; g++)
        for (s = 0; s < 4; s++) {
            run(2, 3, 0x7, 0, sizes[s], gens[g]);
            run(4, 6, 0x1F, 0x20, sizes[s], gens[g]);
            run(4, 6, 0x37, 0x08, sizes[s], gens[g]);
            run(4, 6, 0x3F, 0, sizes[s], gens[g]);
            run(8, 12, 0x2FF, 0xD00, sizes[s], gens[g]);
            run(9, 11, 0x3FF, 0x400, sizes[s], gens[g]);
            run(16, 20, 0xFFFFE, 0x1, sizes[s], gens[g]);
            run(16, 31, 0x1FFFF, 0x7FFE0000, sizes[s], gens[g]);
        }
    printf("failures=%d\n", failures);
    return failures != 0;
}
