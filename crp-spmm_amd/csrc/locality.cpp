// locality.cpp -- processing order of the rows of A for B-row locality (locality.h).
//
// The reference leaves the inspector step to MKL (mkl_sparse_d_mm, /root/reference/src/rowpara_spmm.c:398-408)
// and offers a METIS re-partitioning only in its examples (/root/reference/examples/metis_mat_part.c:31-113,
// third-party, absent here).  What the GPU kernels need is narrower than a partition of the matrix: rows that
// are processed together (one row panel, one team, the waves in flight on one XCD) should read the same B
// rows.  The ROWS of A are only re-ordered for processing -- B is read in place by column index and C is
// written through a row map -- so the order is free.
//
//   1. row groups: consecutive rows with identical column lists (the unknowns of one node of a finite-element
//      mesh) stay together; the graph below has one vertex per group;
//   2. the vertices are cut into `nparts` parts of equal row count by recursive bisection along the
//      breadth-first level structure rooted at a pseudo-peripheral vertex (George & Liu): a part is a slab
//      between two level fronts, and the kernels hand every XCD one contiguous range of the order, so
//      every XCD's L2 sees one slab;
//   3. inside a part: reverse Cuthill-McKee from a pseudo-peripheral vertex of the part, which sweeps the slab
//      along its LONG axis -- the front it moves is the slab's narrow cross-section, i.e. the set of B rows
//      that has to stay in L2 is small.
// Cost: O(nnz) per bisection level plus a handful of breadth-first searches.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string.h>
#include "graph_bfs.h"
#include "locality.h"

namespace crp {

namespace {

using gbfs::Graph;
using gbfs::part_order;

// Steps 2 and 3 of the header comment on any weighted graph: `nparts` (a power of two) parts of equal weight by
// recursive bisection along breadth-first level structures, reverse Cuthill-McKee inside every part.
// -> the vertices part after part; first[q] = where part q starts in that order (nparts + 1 entries).
void slab_order(const Graph &g, int nparts, std::vector<int> *gorder_out, std::vector<int> *first)
{
    const int ng = g.n;
    int depth = 0;
    while ((1 << depth) < nparts) depth++;
    std::vector<int> part((size_t) ng, 0), mark((size_t) ng, 0), level((size_t) ng, 0), placed((size_t) ng, 0), scratch, order;
    int stamp = 0;
    std::vector<std::vector<int>> members(1);
    members[0].resize((size_t) ng);
    std::iota(members[0].begin(), members[0].end(), 0);
    for (int d = 0; d < depth; d++)
    {
        std::vector<std::vector<int>> next(members.size() * 2);
        for (size_t pid = 0; pid < members.size(); pid++)
        {
            // (part ids are re-assigned after every level: vertex v of part pid goes to 2 pid or 2 pid + 1)
            part_order(g, part, (int) pid, members[pid], false, stamp, mark, level, placed, scratch, order);
            long long total = 0, run = 0;
            for (int v : order) total += g.weight[(size_t) v];
            size_t cut = 0;
            while (cut < order.size() && (run + g.weight[(size_t) order[cut]] / 2) * 2 < total) run += g.weight[(size_t) order[cut++]];
            next[2 * pid].assign(order.begin(), order.begin() + (long) cut);
            next[2 * pid + 1].assign(order.begin() + (long) cut, order.end());
        }
        members.swap(next);
        for (size_t pid = 0; pid < members.size(); pid++)
            for (int v : members[pid]) part[(size_t) v] = (int) pid;
    }
    // ---- 3. reverse Cuthill-McKee inside every part
    std::vector<int> &gorder = *gorder_out;
    gorder.clear();
    if (first) first->assign(1, 0);
    gorder.reserve((size_t) ng);
    for (size_t pid = 0; pid < members.size(); pid++)
    {
        part_order(g, part, (int) pid, members[pid], true, stamp, mark, level, placed, scratch, order);
        gorder.insert(gorder.end(), order.begin(), order.end());
        if (first) first->push_back((int) gorder.size());
    }
}

}  // namespace

bool locality_reorder(int nrow, int ncol, const int *rowptr, const int *colidx, int nparts, std::vector<int> *perm,
                      LocalityInfo *info)
{
    perm->clear();
    if (nrow != ncol || nrow < 64 || rowptr[nrow] <= 0) return false;
    const long long nnz = rowptr[nrow];
    for (long long p = 0; p < nnz; p++)
        if (colidx[p] < 0 || colidx[p] >= nrow) return false;        // two-source or rectangular column space
    // ---- 1. row groups; quotient graph, symmetrised (weight = rows of the group)
    std::vector<int> grp, rep;
    Graph g;
    gbfs::group_graph(nrow, rowptr, colidx, &grp, &rep, &g);
    const int ng = g.n;

    // ---- 2., 3.
    std::vector<int> gorder;
    std::vector<int> first;
    slab_order(g, nparts, &gorder, &first);
    if ((int) gorder.size() != ng) return false;
    // ---- rows of the groups in that order
    std::vector<int> gstart((size_t) ng + 1, 0);
    for (int s = 0; s < ng; s++) gstart[(size_t) s + 1] = gstart[(size_t) s] + g.weight[(size_t) s];
    perm->reserve((size_t) nrow);
    for (int s : gorder)
        for (int r = rep[(size_t) s]; r < rep[(size_t) s] + g.weight[(size_t) s]; r++) perm->push_back(r);
    if (info != nullptr)
    {
        info->groups = ng;
        info->parts = (int) first.size() - 1;
        // mean distance, in the new order, between a row and the rows its columns name: what the sweep has to keep
        std::vector<int> pos((size_t) nrow);
        for (int i = 0; i < nrow; i++) pos[(size_t) (*perm)[(size_t) i]] = i;
        double before = 0.0, after = 0.0;
        for (int r = 0; r < nrow; r++)
            for (int p = rowptr[r]; p < rowptr[r + 1]; p++)
            {
                before += std::abs((double) colidx[p] - r);
                after += std::abs((double) pos[(size_t) colidx[p]] - pos[(size_t) r]);
            }
        info->mean_dist_before = before / (double) nnz;
        info->mean_dist_after = after / (double) nnz;
    }
    return true;
}

bool graph_slab_order(int n, const std::vector<int> &ptr, const std::vector<int> &adj, const std::vector<int> &weight, int nparts,
                      std::vector<int> *order, std::vector<int> *first)
{
    if (n <= 0 || (int) ptr.size() != n + 1 || (int) weight.size() != n) return false;
    Graph g;
    g.n = n;
    g.ptr = ptr;
    g.adj = adj;
    g.weight = weight;
    slab_order(g, nparts, order, first);
    return (int) order->size() == n;
}

}  // namespace crp
