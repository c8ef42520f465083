/* dc_check.c -- serial, engine-independent checker of sfx_doc_counts_* (DESIGN.md section 23).
 *
 *   dc_check da.bin lcp.bin df.bin dup_prefix.bin        (raw little-endian uint32 arrays of one length n)
 *
 * Recomputes both outputs from (da, lcp) by methods that share nothing with the engine's sort, min-tree and prefix sums:
 *   df          one left-to-right sweep over lcp with a stack of the open lcp-intervals (depth, left end, pairs charged).
 *               After boundary r has been handled the stack holds exactly the intervals that contain ranks r - 1 and r,
 *               left ends ascending; the rank r of a document seen before at rank q charges the DEEPEST of them whose left
 *               end is <= q (bisection over the stack).  An interval that closes hands its total to its parent, and
 *               df = size - total.  Every boundary remembers which interval it joined.
 *   dup_prefix  from the definition: a second stack holds the boundaries whose value is smaller than every value to
 *               their right up to r (ties: the right one stays), so the rightmost minimum of (q, r] is the first entry
 *               above q; dup_prefix is the running sum of the hits per boundary.
 * lcp[0] counts as 0.  Prints "ok ..." (exit 0) or the first differing index of the first array that differs (exit 1). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static uint32_t* load(const char* path, uint64_t* n_out)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "dc_check: cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint32_t* a = (uint32_t*)malloc(bytes > 0 ? (size_t)bytes : 4);
    if (!a || (bytes > 0 && fread(a, 1, (size_t)bytes, f) != (size_t)bytes)) { fprintf(stderr, "dc_check: cannot read %s\n", path); exit(2); }
    fclose(f);
    *n_out = (uint64_t)bytes / 4;
    return a;
}

typedef struct { uint32_t depth; uint64_t lb, pairs, id; } open_t;

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: dc_check da.bin lcp.bin df.bin dup_prefix.bin\n"); return 2; }
    uint64_t n, n1, n2, n3;
    uint32_t* da = load(argv[1], &n);
    uint32_t* lcp = load(argv[2], &n1);
    uint32_t* df = load(argv[3], &n2);
    uint32_t* dup = load(argv[4], &n3);
    if (n1 != n || n2 != n || n3 != n) { printf("lengths differ: %llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)n1,
                                                (unsigned long long)n2, (unsigned long long)n3); return 1; }
    if (n == 0) { printf("ok n=0\n"); return 0; }
    uint32_t maxd = 0;
    for (uint64_t r = 0; r < n; r++) if (da[r] > maxd) maxd = da[r];
    int64_t* last = (int64_t*)malloc(((size_t)maxd + 1) * sizeof(int64_t));
    for (uint64_t d = 0; d <= maxd; d++) last[d] = -1;
    open_t* st = (open_t*)malloc((n + 2) * sizeof(open_t));          /* open intervals */
    uint64_t* joined = (uint64_t*)malloc(n * sizeof(uint64_t));       /* boundary -> interval id */
    uint32_t* iv_df = (uint32_t*)malloc((n + 1) * sizeof(uint32_t)); /* interval id -> df */
    uint64_t* ms = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));     /* boundaries smaller than everything to their right */
    uint64_t* hits = (uint64_t*)calloc(n, sizeof(uint64_t));
    if (!last || !st || !joined || !iv_df || !ms || !hits) { fprintf(stderr, "dc_check: out of memory\n"); return 2; }
    uint64_t top = 0, ids = 1, mtop = 0, nonempty = 0;
    st[0].depth = 0; st[0].lb = 0; st[0].pairs = 0; st[0].id = 0;
    joined[0] = 0;
    for (uint64_t i = 0; i <= n; i++) {
        /* boundary i (its value: 0 at both ends), then rank i */
        const uint32_t v = (i == 0 || i == n) ? 0u : lcp[i];
        if (i > 0) {
            uint64_t lb = i - 1, carried = 0;
            while (st[top].depth > v) {                               /* closes with right end i - 1 */
                const uint64_t total = st[top].pairs + carried;
                iv_df[st[top].id] = (uint32_t)((i - st[top].lb) - total);
                carried = total;
                lb = st[top].lb;
                top--;
            }
            if (st[top].depth < v) {
                top++;
                st[top].depth = v; st[top].lb = lb; st[top].pairs = 0; st[top].id = ids++;
            }
            st[top].pairs += carried;
            if (i < n) joined[i] = st[top].id;
        }
        if (i == n) break;
        if (i > 0) {
            while (mtop > 0 && lcp[ms[mtop - 1]] >= v) mtop--;
            ms[mtop++] = i;
        }
        const int64_t q = last[da[i]];
        if (q < 0) {
            nonempty++;
        } else {
            uint64_t lo = 0, hi = top;                                /* deepest open interval with lb <= q */
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) / 2;
                if (st[mid].lb <= (uint64_t)q) lo = mid; else hi = mid - 1;
            }
            st[lo].pairs++;
            uint64_t a = 0, b = mtop - 1;                             /* first entry above q (the last one is i) */
            while (a < b) {
                const uint64_t mid = (a + b) / 2;
                if (ms[mid] > (uint64_t)q) b = mid; else a = mid + 1;
            }
            hits[ms[a]]++;
        }
        last[da[i]] = (int64_t)i;
    }
    /* (the root closed at i == n: depth 0 is never popped, so finish it here) */
    iv_df[0] = (uint32_t)(n - st[0].pairs);
    if (iv_df[0] != nonempty) { printf("internal: the root has %u documents, %llu were seen\n", iv_df[0], (unsigned long long)nonempty); return 3; }
    for (uint64_t p = 0; p < n; p++) {
        const uint32_t want = iv_df[joined[p]];
        if (df[p] != want) { printf("df differs at %llu: reported %u, expected %u\n", (unsigned long long)p, df[p], want); return 1; }
    }
    uint64_t run = 0;
    for (uint64_t x = 0; x < n; x++) {
        run += hits[x];
        if (dup[x] != (uint32_t)run) { printf("dup_prefix differs at %llu: reported %u, expected %llu\n", (unsigned long long)x, dup[x],
                                              (unsigned long long)run); return 1; }
    }
    printf("ok n=%llu intervals=%llu documents=%llu pairs=%llu\n", (unsigned long long)n, (unsigned long long)ids, (unsigned long long)nonempty,
           (unsigned long long)run);
    return 0;
}
