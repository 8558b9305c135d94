// graph_part.cpp -- k-way row partition of a square CSR by recursive breadth-first bisection, and the host path of the
// symmetric permutation P A P^T (graph_part.h, include/crp_part.h).
//
// The reference's example programs offer METIS (METIS_PartGraphKway, 5 % imbalance) as part-method 1; METIS is not
// part of this build.  The partition here is the level-structure bisection that locality.cpp already uses for the
// kernels' row orders, made k-way and weighted by nonzeros:
//   1. row groups (consecutive rows with identical column lists) are the vertices of the graph of A + A^T
//      (graph_bfs.h); vertex weight = the nonzeros of the group's rows;
//   2. a vertex set meant for k ranks is put in breadth-first order from pseudo-peripheral roots, one component after
//      the other, and cut where the running weight passes floor(k/2)/k of its total; the two halves recurse with
//      floor(k/2) and k - floor(k/2) ranks.  A part is a slab between two level fronts, so the B rows another part
//      needs are the few planes along the cut;
//   3. the leaves, concatenated, are a row sequence in which every rank's share is one contiguous stretch.  The final
//      cuts are taken on ROWS of that sequence: row t goes to part floor(P * (prefix_t + nnz_t / 2) / nnz), so a part
//      holds at most nnz / P + (largest row nnz) -- inside the 5 % the reference gives METIS plus one row;
//   4. inside a part the rows keep their original relative order (the reference's sort by part id).
// Everything is serial and deterministic.  Cost: O(nnz) per bisection level plus a few breadth-first searches per
// component.
#include <algorithm>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "crp_part.h"
#include "graph_bfs.h"
#include "graph_part.h"
#include "par.h"

namespace crp {

namespace {

struct Bisector
{
    const gbfs::Graph &g;
    std::vector<int> part, mark, level, placed, scratch;
    int stamp = 0, next_id = 1;
    std::vector<int> seq;           // the leaves' vertices, leaf after leaf

    explicit Bisector(const gbfs::Graph &g_)
        : g(g_), part((size_t) g_.n, 0), mark((size_t) g_.n, 0), level((size_t) g_.n, 0), placed((size_t) g_.n, 0)
    {
        seq.reserve((size_t) g_.n);
    }

    // the vertices `members` (all with part[] == pid) for k ranks
    void split(int pid, const std::vector<int> &members, int k)
    {
        if (k <= 1 || members.size() <= 1)
        {
            seq.insert(seq.end(), members.begin(), members.end());
            return;
        }
        std::vector<int> order;
        gbfs::part_order(g, part, pid, members, false, stamp, mark, level, placed, scratch, order);
        const int kl = k / 2;
        long long total = 0, run = 0;
        for (int v : order) total += g.weight[(size_t) v];
        size_t cut = 0;
        // a vertex goes left while its weighted midpoint lies before floor(k/2)/k of the total
        while (cut < order.size() && (2 * run + g.weight[(size_t) order[cut]]) * k < 2 * total * kl) run += g.weight[(size_t) order[cut++]];
        std::vector<int> left(order.begin(), order.begin() + (long) cut), right(order.begin() + (long) cut, order.end());
        order.clear();
        order.shrink_to_fit();
        const int lid = next_id++, rid = next_id++;
        for (int v : left) part[(size_t) v] = lid;
        for (int v : right) part[(size_t) v] = rid;
        split(lid, left, kl);
        split(rid, right, k - kl);
    }
};

// rowptr starts at 0 and never decreases, every column lies in [0, nrow): 0, CRP_PART_EPTR or CRP_PART_ECOL
int check_csr(int nrow, const int *rowptr, const int *colidx)
{
    if (rowptr[0] != 0) return CRP_PART_EPTR;
    for (int i = 0; i < nrow; i++)
        if (rowptr[i + 1] < rowptr[i]) return CRP_PART_EPTR;
    const int nnz = rowptr[nrow];
    for (int p = 0; p < nnz; p++)
        if (colidx[p] < 0 || colidx[p] >= nrow) return CRP_PART_ECOL;
    return 0;
}

}  // namespace

int graph_row_order(int nrow, int nproc, const int *rowptr, const int *colidx, int *perm, int *row_displs)
{
    if (nrow < 0 || nproc < 1 || rowptr == NULL || perm == NULL || row_displs == NULL) return CRP_PART_EARG;
    const int nnz = rowptr[nrow];
    if (nnz > 0 && colidx == NULL) return CRP_PART_EARG;
    if (const int rc = check_csr(nrow, rowptr, colidx)) return rc;

    // ---- 1., 2.: the row sequence
    std::vector<int> rows_seq;
    rows_seq.reserve((size_t) nrow);
    if (nproc == 1 || nrow <= 1)
        for (int i = 0; i < nrow; i++) rows_seq.push_back(i);
    else
    {
        std::vector<int> grp, rep;
        gbfs::Graph g;
        gbfs::group_graph(nrow, rowptr, colidx, &grp, &rep, &g);
        const std::vector<int> nrows_of = g.weight;
        if (nnz > 0)
            for (int s = 0; s < g.n; s++)
                g.weight[(size_t) s] = rowptr[rep[(size_t) s] + nrows_of[(size_t) s]] - rowptr[rep[(size_t) s]];
        Bisector b(g);
        std::vector<int> all((size_t) g.n);
        for (int s = 0; s < g.n; s++) all[(size_t) s] = s;
        b.split(0, all, nproc);
        for (int s : b.seq)
            for (int r = rep[(size_t) s]; r < rep[(size_t) s] + nrows_of[(size_t) s]; r++) rows_seq.push_back(r);
    }
    if ((int) rows_seq.size() != nrow) return CRP_PART_EARG;       // (cannot happen: every vertex lands in one leaf)

    // ---- 3. cuts on rows: a row belongs to the part its weighted midpoint falls in (all rows empty: by row count)
    std::vector<int> part_of((size_t) nrow);
    const long long W = nnz > 0 ? nnz : nrow;
    long long prefix = 0;
    for (int t = 0; t < nrow; t++)
    {
        const int r = rows_seq[(size_t) t];
        const long long w = nnz > 0 ? rowptr[r + 1] - rowptr[r] : 1;
        const long long q = (2 * prefix + w) * nproc / (2 * W);
        part_of[(size_t) r] = (int) std::min<long long>(q, nproc - 1);
        prefix += w;
    }
    // ---- 4. part by part, original order inside a part
    std::vector<int> cnt((size_t) nproc + 1, 0);
    for (int i = 0; i < nrow; i++) cnt[(size_t) part_of[(size_t) i] + 1]++;
    for (int q = 0; q < nproc; q++) cnt[(size_t) q + 1] += cnt[(size_t) q];
    memcpy(row_displs, cnt.data(), sizeof(int) * ((size_t) nproc + 1));
    for (int i = 0; i < nrow; i++) perm[i] = cnt[(size_t) part_of[(size_t) i]]++;
    return 0;
}

int csr_permute_sym_host(int nrow, const int *rowptr, const int *colidx, const double *val, const int *perm, int *rowptr1,
                         int *colidx1, double *val1)
{
    if (nrow < 0 || rowptr == NULL || perm == NULL || rowptr1 == NULL) return CRP_PART_EARG;
    if (nrow > 0 && rowptr[nrow] > 0 && (colidx == NULL || val == NULL || colidx1 == NULL || val1 == NULL)) return CRP_PART_EARG;
    if (const int rc = check_csr(nrow, rowptr, colidx)) return rc;
    std::vector<char> hit((size_t) nrow, 0);
    for (int i = 0; i < nrow; i++)
    {
        const int t = perm[i];
        if (t < 0 || t >= nrow || hit[(size_t) t]) return CRP_PART_EPERM;
        hit[(size_t) t] = 1;
    }
    // row lengths at their new places, then the offsets
    std::vector<int> len1((size_t) nrow + 1, 0);
    for (int i = 0; i < nrow; i++) len1[(size_t) perm[i]] = rowptr[i + 1] - rowptr[i];
    rowptr1[0] = 0;
    for (int i = 0; i < nrow; i++) rowptr1[i + 1] = rowptr1[i] + len1[(size_t) i];
    // every row on its own: (new column, position) keys sorted, then the entries moved in that order
    parallel_chunks(nrow, 2048, [&](long long b, long long e, int) {
        std::vector<uint64_t> key;
        for (long long i = b; i < e; i++)
        {
            const int in = rowptr[i], len = rowptr[i + 1] - in, out = rowptr1[perm[i]];
            key.resize((size_t) len);
            for (int t = 0; t < len; t++) key[(size_t) t] = ((uint64_t) (uint32_t) perm[colidx[in + t]] << 32) | (uint32_t) t;
            std::sort(key.begin(), key.end());
            for (int t = 0; t < len; t++)
            {
                colidx1[out + t] = (int) (key[(size_t) t] >> 32);
                val1[out + t] = val[in + (int) (uint32_t) key[(size_t) t]];
            }
        }
    });
    return 0;
}

}  // namespace crp

extern "C" int crp_graph_row_order(int nrow, int nproc, const int *rowptr, const int *colidx, int *perm, int *row_displs)
{
    return crp::graph_row_order(nrow, nproc, rowptr, colidx, perm, row_displs);
}
