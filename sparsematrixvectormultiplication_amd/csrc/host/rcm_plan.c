/*
 * rcm_plan.c -- spmv_rcm_plan_build: the reverse Cuthill-McKee ordering of include/spmv_hip.h, as the serial loop that
 * defines it.  One thread, no device: the device build (spmv_reorder.hip) is held to this byte for byte.
 *
 *   graph     neighbour lists of A + A^T without the diagonal, repeats dropped, each list sorted by (deg, index)
 *   starts    the nodes sorted by (deg, index) and a cursor that skips visited ones: isolated nodes come first, in
 *             index order, and cost one step each
 *   search    a breadth-first search over the unvisited nodes (the start's component): levels and the last level
 *   order     the Cuthill-McKee queue: a node's unvisited neighbours are appended in their list's order
 */
#include <stdlib.h>
#include <string.h>

#include "spmv_hip.h"

static int cmp_int(const void *a, const void *b) {
    const int x = *(const int *)a, y = *(const int *)b;
    return (x > y) - (x < y);
}
static int cmp_ll(const void *a, const void *b) {
    const long long x = *(const long long *)a, y = *(const long long *)b;
    return (x > y) - (x < y);
}

typedef struct {
    const int *ptr, *adj, *deg;
    const unsigned char *visited;
    int *mark, *queue; /* mark[v] == stamp: reached by the running search */
    int stamp;
} Search;

/* levels of the search from s; *smallest = the smallest (deg, index) node of its last level */
static int search_from(Search *S, int s, int *smallest) {
    int head = 0, tail = 0, depth = 0, first = 0;
    S->stamp++;
    S->mark[s] = S->stamp;
    S->queue[tail++] = s;
    while (head < tail) {
        const int end = tail;
        first = head;
        ++depth;
        for (; head < end; ++head) {
            const int u = S->queue[head];
            for (int e = S->ptr[u]; e < S->ptr[u + 1]; ++e) {
                const int w = S->adj[e];
                if (S->visited[w] || S->mark[w] == S->stamp) continue;
                S->mark[w] = S->stamp;
                S->queue[tail++] = w;
            }
        }
    }
    int t = S->queue[first];
    for (int k = first + 1; k < tail; ++k) {
        const int w = S->queue[k];
        if (S->deg[w] < S->deg[t] || (S->deg[w] == S->deg[t] && w < t)) t = w;
    }
    *smallest = t;
    return depth;
}

int spmv_rcm_plan_build(int n, const int *row_ptr, const int *col, int peripheral, int *perm, long long *stats) {
    if (n < 0 || !row_ptr || (n && !perm) || peripheral < 0 || peripheral > SPMV_RCM_MAX_PERIPHERAL) return -1;
    if (row_ptr[0] != 0) return -1;
    for (int i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return -1;
    const int nz = n ? row_ptr[n] : 0;
    if (nz && !col) return -1;
    for (int e = 0; e < nz; ++e)
        if (col[e] < 0 || col[e] >= n) return -1;
    long long st[SPMV_RCM_STATS] = {0};
    if (!n) {
        if (stats) memcpy(stats, st, sizeof(st));
        return 0;
    }
    int rc = -2;
    int *ptr = calloc((size_t)n + 2, sizeof(int));
    int *deg = malloc((size_t)n * sizeof(int));
    int *mark = calloc((size_t)n, sizeof(int));
    int *queue = malloc((size_t)n * sizeof(int));
    int *seq = malloc((size_t)n * sizeof(int));
    int *inv = malloc((size_t)n * sizeof(int));
    long long *keys = malloc((size_t)n * sizeof(long long));
    unsigned char *visited = calloc((size_t)n, 1);
    int *adj = NULL;
    if (!ptr || !deg || !mark || !queue || !seq || !inv || !keys || !visited) goto done;

    /* ---- graph: both directions of every off-diagonal entry, each list sorted, repeats dropped */
    long long before = 0;
    for (int i = 0; i < n; ++i)
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int j = col[e];
            const long long d = i > j ? (long long)i - j : (long long)j - i;
            if (d > before) before = d;
            if (j != i) ptr[i + 2]++, ptr[j + 2]++;
        }
    for (int i = 0; i < n; ++i) {
        if ((long long)ptr[i + 1] + ptr[i + 2] > 0x7fffffff) goto done;
        ptr[i + 2] += ptr[i + 1];
    }
    adj = malloc(((size_t)ptr[n + 1] + 1) * sizeof(int));
    if (!adj) goto done;
    for (int i = 0; i < n; ++i) /* ptr[i + 1] is row i's fill mark and ends as its end */
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int j = col[e];
            if (j != i) adj[ptr[i + 1]++] = j, adj[ptr[j + 1]++] = i;
        }
    int out = 0;
    for (int i = 0; i < n; ++i) {
        const int b = ptr[i], e1 = ptr[i + 1];
        qsort(adj + b, (size_t)(e1 - b), sizeof(int), cmp_int);
        ptr[i] = out;
        for (int e = b; e < e1; ++e)
            if (e == b || adj[e] != adj[e - 1]) adj[out++] = adj[e];
        deg[i] = out - ptr[i];
    }
    ptr[n] = out;
    for (int i = 0; i < n; ++i) { /* each list by (deg, index) */
        const int b = ptr[i], k = deg[i];
        for (int e = 0; e < k; ++e) keys[e] = ((long long)deg[adj[b + e]] << 32) | (unsigned)adj[b + e];
        qsort(keys, (size_t)k, sizeof(long long), cmp_ll);
        for (int e = 0; e < k; ++e) adj[b + e] = (int)(unsigned)keys[e];
    }

    /* ---- start nodes: one sort of all nodes by (deg, index) */
    int *by_key = inv; /* (inv is free until the end) */
    for (int i = 0; i < n; ++i) keys[i] = ((long long)deg[i] << 32) | (unsigned)i;
    qsort(keys, (size_t)n, sizeof(long long), cmp_ll);
    for (int i = 0; i < n; ++i) by_key[i] = (int)(unsigned)keys[i];

    Search S = {ptr, adj, deg, visited, mark, queue, 0};
    int filled = 0;
    for (int cursor = 0; cursor < n; ++cursor) {
        int s = by_key[cursor];
        if (visited[s]) continue;
        st[0]++;
        if (!deg[s]) { /* isolated: no search */
            st[1]++;
            visited[s] = 1;
            seq[filled++] = s;
            continue;
        }
        if (peripheral > 0) {
            int t, t2;
            int depth_s = search_from(&S, s, &t);
            st[6]++;
            for (int pass = 0; pass < peripheral; ++pass) {
                const int depth_t = search_from(&S, t, &t2);
                st[6]++;
                if (depth_t <= depth_s) break;
                s = t, depth_s = depth_t, t = t2;
            }
        }
        int head = filled, level_end;
        visited[s] = 1;
        seq[filled++] = s;
        while (head < filled) {
            st[2]++;
            for (level_end = filled; head < level_end; ++head) {
                const int v = seq[head];
                for (int e = ptr[v]; e < ptr[v + 1]; ++e) {
                    const int w = adj[e];
                    if (visited[w]) continue;
                    visited[w] = 1;
                    seq[filled++] = w;
                }
            }
        }
    }
    for (int i = 0; i < n; ++i) perm[i] = seq[n - 1 - i];
    for (int i = 0; i < n; ++i) inv[perm[i]] = i;
    long long after = 0;
    for (int i = 0; i < n; ++i)
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const long long d = inv[i] > inv[col[e]] ? (long long)inv[i] - inv[col[e]] : (long long)inv[col[e]] - inv[i];
            if (d > after) after = d;
        }
    st[7] = before, st[8] = after;
    if (stats) memcpy(stats, st, sizeof(st));
    rc = 0;
done:
    free(ptr), free(deg), free(mark), free(queue), free(seq), free(inv), free(keys), free(visited), free(adj);
    return rc;
}
