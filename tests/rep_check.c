/* tests/rep_check.c -- serial, engine-independent checker of sfx_repeat_lens_* on large inputs.
 * usage: rep_check SCOPE text starts sa lcp da rep src      (raw little-endian files; da may be empty unless SCOPE = 2)
 * Recomputes rep from (SA, LCP, DA) with linear sweeps that share nothing with the engine's searches:
 *   0 ANY        the two neighbouring LCP values;
 *   1 EARLIER    the ancestor-stack sweep of the LPF array (Crochemore & Ilie 2008): a rank leaves the stack when a
 *                smaller position arrives, with the minimum LCP it has seen on either side;
 *   2 OTHER_DOC  two passes carrying the minimum LCP since the current run of one document began;
 * and validates every witness src[p] against the text: allowed by the scope, rep[p] equal bytes, inside both documents
 * (bytes compared directly up to 256 of them, longer matches by polynomial prefix hashes modulo 2^61 - 1 plus their
 * first and last 128 bytes: "a" x 2^20 has 2^39 matching bytes in all).
 * Prints "ok ..." or the first fault; exit status 0 unless a file cannot be read. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void* slurp(const char* path, size_t elem, uint64_t* count)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    void* p = malloc(bytes > 0 ? (size_t)bytes : 1);
    if (!p || (bytes > 0 && fread(p, 1, (size_t)bytes, f) != (size_t)bytes)) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    *count = (uint64_t)bytes / elem;
    return p;
}

static const uint64_t kMod = (1ull << 61) - 1, kBase = 0x1F3D5B79A2C4E681ull % ((1ull << 61) - 1);
static uint64_t mulmod(uint64_t a, uint64_t b)
{
    const __uint128_t t = (__uint128_t)a * b;
    uint64_t r = (uint64_t)(t & kMod) + (uint64_t)(t >> 61);
    while (r >= kMod) r -= kMod;
    return r;
}
static uint64_t *H, *PW;                                   /* H[i] = hash of text[0, i), PW[i] = base^i */
static uint64_t hash_of(uint64_t b, uint64_t len)
{
    const uint64_t x = H[b + len] + kMod - mulmod(H[b], PW[len]);
    return x >= kMod ? x - kMod : x;
}
static int same_bytes(const uint8_t* text, uint64_t p, uint64_t q, uint64_t k)
{
    if (k <= 256) return memcmp(text + p, text + q, k) == 0;
    return memcmp(text + p, text + q, 128) == 0 && memcmp(text + p + k - 128, text + q + k - 128, 128) == 0 &&
           hash_of(p, k) == hash_of(q, k);
}

static uint32_t min32(uint32_t a, uint32_t b) { return a < b ? a : b; }
static uint32_t max32(uint32_t a, uint32_t b) { return a > b ? a : b; }

int main(int argc, char** argv)
{
    if (argc != 9) { fprintf(stderr, "usage: rep_check SCOPE text starts sa lcp da rep src\n"); return 2; }
    const int scope = atoi(argv[1]);
    uint64_t n, nd, c;
    const uint8_t* text = slurp(argv[2], 1, &n);
    const uint64_t* starts = slurp(argv[3], 8, &nd);
    const uint32_t* sa = slurp(argv[4], 4, &c);
    if (c != n) { printf("FAIL sa holds %llu entries, text %llu\n", (unsigned long long)c, (unsigned long long)n); return 0; }
    const uint32_t* lcp = slurp(argv[5], 4, &c);
    if (c != n) { printf("FAIL lcp size\n"); return 0; }
    const uint32_t* da = slurp(argv[6], 4, &c);
    if (scope == 2 && c != n) { printf("FAIL da size\n"); return 0; }
    const uint32_t* rep = slurp(argv[7], 4, &c);
    if (c != n) { printf("FAIL rep size\n"); return 0; }
    const uint32_t* src = slurp(argv[8], 4, &c);
    if (c != n) { printf("FAIL src size\n"); return 0; }
    if (n == 0) { printf("ok n=0\n"); return 0; }

    /* document of every position and its end (one document when no starts are given) */
    uint32_t* doc = malloc(n * sizeof(uint32_t));
    uint32_t* dend = malloc(n * sizeof(uint32_t));
    if (nd == 0) {
        for (uint64_t p = 0; p < n; p++) { doc[p] = 0; dend[p] = (uint32_t)n; }
    } else {
        for (uint64_t d = 0; d < nd; d++) {
            const uint64_t b = starts[d], e = d + 1 < nd ? starts[d + 1] : n;
            for (uint64_t p = b; p < e; p++) { doc[p] = (uint32_t)d; dend[p] = (uint32_t)e; }
        }
    }

    uint32_t* exp = calloc(n, sizeof(uint32_t));
    if (scope == 0) {
        for (uint64_t r = 0; r < n; r++)
            exp[sa[r]] = max32(r ? lcp[r] : 0, r + 1 < n ? lcp[r + 1] : 0);
    } else if (scope == 1) {
        uint32_t* spos = malloc(n * sizeof(uint32_t));
        uint32_t* slcp = malloc(n * sizeof(uint32_t));
        uint64_t top = 0;
        for (uint64_t r = 0; r <= n; r++) {
            uint32_t cur = (r == 0 || r == n) ? 0 : lcp[r];
            const int64_t pos = r < n ? (int64_t)sa[r] : -1;
            while (top && pos < (int64_t)spos[top - 1]) {
                exp[spos[top - 1]] = max32(slcp[top - 1], cur);
                cur = min32(slcp[top - 1], cur);
                top--;
            }
            if (r < n) { spos[top] = sa[r]; slcp[top] = cur; top++; }
        }
        free(spos);
        free(slcp);
    } else if (scope == 2) {
        uint32_t* left = malloc(n * sizeof(uint32_t));
        uint32_t m = 0;                                    /* min LCP since the run began; 0: the run began at rank 0 */
        for (uint64_t r = 0; r < n; r++) {
            if (r == 0) m = 0;
            else if (da[r] != da[r - 1]) m = lcp[r];
            else m = min32(m, lcp[r]);
            left[r] = m;
        }
        m = 0;                                             /* from the right: min LCP up to the next run's first rank */
        for (uint64_t r = n; r-- > 0;) {
            if (r + 1 == n) m = 0;
            else if (da[r + 1] != da[r]) m = lcp[r + 1];
            else m = min32(m, lcp[r + 1]);
            exp[sa[r]] = max32(left[r], m);
        }
        free(left);
    } else {
        printf("FAIL unknown scope %d\n", scope);
        return 0;
    }

    H = malloc((n + 1) * sizeof(uint64_t));
    PW = malloc((n + 1) * sizeof(uint64_t));
    H[0] = 0;
    PW[0] = 1;
    for (uint64_t i = 0; i < n; i++) {
        H[i + 1] = mulmod(H[i], kBase) + text[i] + 1;
        if (H[i + 1] >= kMod) H[i + 1] -= kMod;
        PW[i + 1] = mulmod(PW[i], kBase);
    }
    uint64_t covered = 0, witnesses = 0;
    for (uint64_t p = 0; p < n; p++) {
        const uint32_t k = rep[p], q = src[p];
        if (k != exp[p]) { printf("FAIL rep[%llu] = %u, expected %u\n", (unsigned long long)p, k, exp[p]); return 0; }
        if (k == 0) {
            if (q != 0xFFFFFFFFu) { printf("FAIL src[%llu] = %u with rep 0\n", (unsigned long long)p, q); return 0; }
            continue;
        }
        covered++;
        if (q >= n) { printf("FAIL src[%llu] = %u out of range\n", (unsigned long long)p, q); return 0; }
        const int allowed = scope == 0 ? q != p : scope == 1 ? q < p : doc[q] != doc[p];
        if (!allowed) { printf("FAIL src[%llu] = %u is not allowed by scope %d\n", (unsigned long long)p, q, scope); return 0; }
        if ((uint64_t)p + k > dend[p] || (uint64_t)q + k > dend[q] || !same_bytes(text, p, q, k)) {
            printf("FAIL src[%llu] = %u does not share %u bytes\n", (unsigned long long)p, q, k);
            return 0;
        }
        witnesses++;
    }
    printf("ok n=%llu scope=%d nonzero=%llu witnesses=%llu\n", (unsigned long long)n, scope, (unsigned long long)covered,
           (unsigned long long)witnesses);
    return 0;
}
