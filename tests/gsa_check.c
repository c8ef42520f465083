/* tests/gsa_check.c -- checks a generalized suffix array without the engine (test_gpu_gsa.py compiles and runs it).
 *   gsa_check TEXT STARTS SA DA LCP     (raw files: u8 text, u64 doc starts, u32 table, u32 document array, u32 LCP)
 * Verifies: SA is a permutation of [0, n); DA[r] = the document holding SA[r] (binary search of the starts);
 * LCP[0] = 0; for every adjacent pair (a, b) the first LCP[r] bytes are equal (compared by polynomial prefix hashes
 * modulo 2^61 - 1, so the cost does not grow with the LCP values), LCP[r] <= both lengths left in their documents,
 * and the pair is in order: the next byte is smaller, or the first suffix ends there and the second does not, or both
 * end there and the first belongs to the earlier document.  Exit status 0 and "ok ..." on success. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static void* slurp(const char* path, size_t elem, size_t* count)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    void* p = malloc(bytes ? (size_t)bytes : 1);
    if (!p || fread(p, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    *count = (size_t)bytes / elem;
    return p;
}

static const uint64_t MOD = (1ull << 61) - 1;
static uint64_t mulmod(uint64_t a, uint64_t b)
{
    unsigned __int128 x = (unsigned __int128)a * b;
    uint64_t lo = (uint64_t)(x & MOD), hi = (uint64_t)(x >> 61);
    uint64_t r = lo + hi;
    return r >= MOD ? r - MOD : r;
}
static uint64_t *H, *PW;
static uint64_t hash_of(uint64_t s, uint64_t len)             /* of text[s .. s + len) */
{
    uint64_t h = H[s + len] + MOD - mulmod(H[s], PW[len]);
    return h >= MOD ? h - MOD : h;
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

int main(int argc, char** argv)
{
    if (argc != 6) { fprintf(stderr, "usage: gsa_check TEXT STARTS SA DA LCP\n"); return 2; }
    size_t n, nd, nsa, nda, nlcp;
    const uint8_t* t = slurp(argv[1], 1, &n);
    const uint64_t* st = slurp(argv[2], 8, &nd);
    const uint32_t* sa = slurp(argv[3], 4, &nsa);
    const uint32_t* da = slurp(argv[4], 4, &nda);
    const uint32_t* lcp = slurp(argv[5], 4, &nlcp);
    if (nsa != n || nda != n || nlcp != n) FAIL("sizes differ: n %zu sa %zu da %zu lcp %zu", n, nsa, nda, nlcp);
    if (nd == 0 || st[0] != 0) FAIL("bad doc starts");
    for (size_t i = 1; i < nd; i++) if (st[i] < st[i - 1] || st[i] > n) FAIL("bad doc starts at %zu", i);
    uint8_t* seen = calloc(n ? n : 1, 1);
    for (size_t r = 0; r < n; r++) {
        if (sa[r] >= n || seen[sa[r]]) FAIL("not a permutation at rank %zu", r);
        seen[sa[r]] = 1;
        size_t lo = 0, hi = nd;                                   /* first start > position */
        while (lo < hi) { size_t mid = (lo + hi) / 2; if (st[mid] <= sa[r]) lo = mid + 1; else hi = mid; }
        if (da[r] != lo - 1) FAIL("DA[%zu] = %u, expected %zu", r, da[r], lo - 1);
    }
    H = malloc((n + 1) * 8);
    PW = malloc((n + 1) * 8);
    H[0] = 0;
    PW[0] = 1;
    const uint64_t B = 1000003;
    for (size_t i = 0; i < n; i++) {
        H[i + 1] = mulmod(H[i], B) + t[i] + 1;
        if (H[i + 1] >= MOD) H[i + 1] -= MOD;
        PW[i + 1] = mulmod(PW[i], B);
    }
    if (n && lcp[0] != 0) FAIL("LCP[0] = %u", lcp[0]);
    uint64_t sum_lcp = 0;
    for (size_t r = 1; r < n; r++) {
        const uint64_t a = sa[r - 1], b = sa[r], l = lcp[r];
        const uint64_t ea = da[r - 1] + 1 < nd ? st[da[r - 1] + 1] : n, eb = da[r] + 1 < nd ? st[da[r] + 1] : n;
        const uint64_t la = ea - a, lb = eb - b;
        if (l > la || l > lb) FAIL("LCP[%zu] = %llu past a document end (%llu, %llu)", r, (unsigned long long)l,
                                   (unsigned long long)la, (unsigned long long)lb);
        if (hash_of(a, l) != hash_of(b, l)) FAIL("LCP[%zu] = %llu: prefixes differ", r, (unsigned long long)l);
        if (l < la && l < lb) {
            if (t[a + l] >= t[b + l]) FAIL("rank %zu: next bytes out of order (or equal: LCP too small)", r);
        } else if (l == la && l == lb) {
            if (da[r - 1] >= da[r]) FAIL("rank %zu: equal truncated suffixes not in document order", r);
        } else if (l == lb) {
            FAIL("rank %zu: a proper prefix sorts after its extension", r);
        }
        sum_lcp += l;
    }
    printf("ok n=%zu docs=%zu mean_lcp=%.2f\n", n, nd, n > 1 ? (double)sum_lcp / (double)(n - 1) : 0.0);
    return 0;
}
