/* tests/tree_check.c -- serial, engine-independent builder of the suffix-tree node table (include/suffix_hip.h:
 * sfx_suffix_tree_dev) for large inputs.
 * usage: tree_check text sa lcp outdir          (raw little-endian files; writes outdir/<array>.bin, prints "m C")
 * One left-to-right sweep over the boundaries with a stack of open lcp-intervals: the node a boundary opens gets the
 * next id, so dense ids are creation order = ascending leftmost boundary; a leaf is attached when the boundary behind it
 * is seen, an interval when it is closed, and both go to the END of their parent's linked list of children -- children
 * of one node are disjoint rank ranges that end in ascending order, so the lists come out in rank order without a sort.
 * A leaf whose suffix ends exactly at its parent (n - sa[r] == depth) is that node's terminal, not a child.
 * It shares nothing with the engine's nearest-smaller searches, counters and segment ordering. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NONE 0xFFFFFFFFu

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
static void dump(const char* dir, const char* name, const void* p, size_t bytes)
{
    char path[4096];
    snprintf(path, sizeof path, "%s/%s.bin", dir, name);
    FILE* f = fopen(path, "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}

static uint64_t n, m;
static const uint8_t* text;
static const uint32_t *sa, *lcp;
static uint32_t *node_lb, *node_rb, *node_depth, *node_parent, *node_terminal, *leaf_parent;
static uint32_t *first, *last, *next;            /* children: items 0 .. n-1 are leaves (by rank), n + k is node k */

static uint32_t new_node(uint32_t lb, uint32_t depth)
{
    const uint32_t k = (uint32_t)m++;
    node_lb[k] = lb;
    node_depth[k] = depth;
    node_parent[k] = NONE;
    node_terminal[k] = NONE;
    first[k] = last[k] = NONE;
    return k;
}
static void append(uint32_t v, uint32_t item)
{
    next[item] = NONE;
    if (first[v] == NONE) first[v] = item; else next[last[v]] = item;
    last[v] = item;
}
static void attach_leaf(uint32_t v, uint32_t r)
{
    leaf_parent[r] = v;
    if (n - sa[r] == node_depth[v]) node_terminal[v] = sa[r];
    else append(v, r);
}
static void attach_node(uint32_t v, uint32_t k)
{
    node_parent[k] = v;
    append(v, (uint32_t)n + k);
}

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: tree_check text sa lcp outdir\n"); return 2; }
    uint64_t c1, c2;
    text = slurp(argv[1], 1, &n);
    sa = slurp(argv[2], 4, &c1);
    lcp = slurp(argv[3], 4, &c2);
    if (c1 != n || c2 != n || n == 0) { fprintf(stderr, "lengths differ\n"); return 2; }
    node_lb = malloc(n * 4); node_rb = malloc(n * 4); node_depth = malloc(n * 4); node_parent = malloc(n * 4);
    node_terminal = malloc(n * 4); leaf_parent = malloc(n * 4);
    first = malloc(n * 4); last = malloc(n * 4); next = malloc(2 * n * 4);
    uint32_t* stack = malloc((n + 1) * 4);
    uint64_t top = 0;
    stack[top++] = new_node(0, 0);                                    /* the root */
    for (uint64_t i = 1; i <= n; i++) {
        const uint32_t prev = i - 1 > 0 ? lcp[i - 1] : 0, cur = i < n ? lcp[i] : 0;
        if (cur > prev) {                                             /* boundary i opens a node whose first child is leaf i - 1 */
            const uint32_t k = new_node((uint32_t)(i - 1), cur);
            stack[top++] = k;
            attach_leaf(k, (uint32_t)(i - 1));
            continue;
        }
        attach_leaf(stack[top - 1], (uint32_t)(i - 1));
        while (node_depth[stack[top - 1]] > cur) {
            const uint32_t x = stack[--top];
            node_rb[x] = (uint32_t)(i - 1);
            if (node_depth[stack[top - 1]] >= cur) {
                attach_node(stack[top - 1], x);
            } else {                                                  /* a node of depth cur between the two: x is its first child */
                const uint32_t k = new_node(node_lb[x], cur);
                attach_node(k, x);
                stack[top++] = k;
            }
        }
    }
    node_rb[0] = (uint32_t)(n - 1);
    uint64_t* child_off = malloc((m + 1) * 8);
    uint32_t *child_lb = malloc(2 * n * 4), *child_node = malloc(2 * n * 4);
    uint8_t* child_byte = malloc(2 * n);
    uint64_t c = 0;
    for (uint64_t k = 0; k < m; k++) {
        child_off[k] = c;
        for (uint32_t it = first[k]; it != NONE; it = next[it]) {
            const uint32_t lb = it < n ? it : node_lb[it - n];
            child_lb[c] = lb;
            child_node[c] = it < n ? NONE : (uint32_t)(it - n);
            child_byte[c] = text[(uint64_t)sa[lb] + node_depth[k]];
            c++;
        }
    }
    child_off[m] = c;
    dump(argv[4], "node_lb", node_lb, m * 4);
    dump(argv[4], "node_rb", node_rb, m * 4);
    dump(argv[4], "node_depth", node_depth, m * 4);
    dump(argv[4], "node_parent", node_parent, m * 4);
    dump(argv[4], "node_terminal", node_terminal, m * 4);
    dump(argv[4], "child_off", child_off, (m + 1) * 8);
    dump(argv[4], "child_lb", child_lb, c * 4);
    dump(argv[4], "child_node", child_node, c * 4);
    dump(argv[4], "child_byte", child_byte, c);
    dump(argv[4], "leaf_parent", leaf_parent, n * 4);
    printf("%llu %llu\n", (unsigned long long)m, (unsigned long long)c);
    return 0;
}
