/* tests/lz_check.c -- serial, engine-independent checker of sfx_lz_parse_* / sfx_lz77_u32 on large inputs.
 * usage: lz_check MIN_LEN text rep len src lit       (raw little-endian files: u8, u32, u32, u32, u8)
 * rep is a reference longest-previous-factor array: the brute force on small texts, the engine's EARLIER array on
 * large ones once tests/rep_check.c has accepted it.  Checked, phrase by phrase from position 0:
 *   the phrases tile [0, n): begin = the sum of the lengths so far, the last one ends at n;
 *   every length and every literal / copy decision equals the rule over rep: r = min(rep[b], n - b), a copy of r bytes
 *   when r >= MIN_LEN, else one literal;
 *   a literal has src = UINT32_MAX and lit = text[b]; a copy has lit = 0, src < b and len equal bytes (memcmp: the
 *   lengths sum to n, so n bytes in all);
 *   a serial decode of (len, src, lit) alone reproduces the text.
 * Prints "ok z=... literals=... longest=..." or the first fault; exit status 0 unless a file cannot be read. */
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

int main(int argc, char** argv)
{
    if (argc != 7) { fprintf(stderr, "usage: lz_check MIN_LEN text rep len src lit\n"); return 2; }
    const uint64_t min_len = strtoull(argv[1], NULL, 10);
    uint64_t n, nrep, z, zs, zl;
    const uint8_t* text = slurp(argv[2], 1, &n);
    const uint32_t* rep = slurp(argv[3], 4, &nrep);
    const uint32_t* len = slurp(argv[4], 4, &z);
    const uint32_t* src = slurp(argv[5], 4, &zs);
    const uint8_t* lit = slurp(argv[6], 1, &zl);
    if (min_len == 0 || nrep != n || zs != z || zl != z) { printf("fault: sizes n=%llu rep=%llu z=%llu/%llu/%llu\n",
        (unsigned long long)n, (unsigned long long)nrep, (unsigned long long)z, (unsigned long long)zs, (unsigned long long)zl); return 0; }
    uint8_t* out = malloc(n ? n : 1);
    uint64_t b = 0, literals = 0, longest = 0;
    for (uint64_t k = 0; k < z; k++) {
        if (b >= n) { printf("fault: phrase %llu begins at %llu, behind the text\n", (unsigned long long)k, (unsigned long long)b); return 0; }
        uint64_t r = rep[b];
        if (r > n - b) r = n - b;
        const int copy = r >= min_len;
        const uint64_t want = copy ? r : 1;
        if (len[k] != want) { printf("fault: phrase %llu at %llu has len %u, the rule gives %llu\n", (unsigned long long)k,
                                     (unsigned long long)b, len[k], (unsigned long long)want); return 0; }
        if (!copy) {
            if (src[k] != 0xFFFFFFFFu || lit[k] != text[b]) { printf("fault: literal %llu at %llu has src %u lit %u\n",
                (unsigned long long)k, (unsigned long long)b, src[k], lit[k]); return 0; }
            out[b] = lit[k];
            literals++;
        } else {
            if (lit[k] != 0 || src[k] >= b) { printf("fault: copy %llu at %llu has src %u lit %u\n", (unsigned long long)k,
                (unsigned long long)b, src[k], lit[k]); return 0; }
            if (memcmp(text + src[k], text + b, want) != 0) { printf("fault: copy %llu at %llu from %u: %llu bytes are not equal\n",
                (unsigned long long)k, (unsigned long long)b, src[k], (unsigned long long)want); return 0; }
            for (uint64_t i = 0; i < want; i++) out[b + i] = out[src[k] + i];          /* (byte by byte: it may overlap itself) */
        }
        if (want > longest) longest = want;
        b += want;
    }
    if (b != n) { printf("fault: the phrases end at %llu, the text at %llu\n", (unsigned long long)b, (unsigned long long)n); return 0; }
    if (n && memcmp(out, text, n) != 0) { printf("fault: the serial decode differs from the text\n"); return 0; }
    printf("ok z=%llu literals=%llu longest=%llu\n", (unsigned long long)z, (unsigned long long)literals, (unsigned long long)longest);
    return 0;
}
