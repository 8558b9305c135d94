// graph_bfs.h -- breadth-first machinery shared by the row orders of locality.cpp and the k-way row partition of
// graph_part.cpp (internal): the symmetric quotient graph of the row groups of a square CSR, breadth-first level
// structures restricted to one part, pseudo-peripheral roots (George & Liu) and the component-by-component
// breadth-first order of a part.
#pragma once
#include <algorithm>
#include <string.h>
#include <vector>

namespace crp {
namespace gbfs {

struct Graph
{
    int n = 0;
    std::vector<int> ptr, adj, weight;       // symmetric adjacency without self loops; weight of the vertex (rows or nonzeros)
};

// Breadth-first levels of the vertices with part[v] == pid reachable from root; returns the visit order and
// fills level[] for the visited vertices.  `mark` must hold a value != stamp for unvisited vertices.
inline void bfs(const Graph &g, const std::vector<int> &part, int pid, int root, int stamp, std::vector<int> &mark,
         std::vector<int> &level, std::vector<int> &order)
{
    order.clear();
    order.push_back(root);
    mark[(size_t) root] = stamp;
    level[(size_t) root] = 0;
    for (size_t head = 0; head < order.size(); head++)
    {
        const int u = order[head];
        for (int t = g.ptr[(size_t) u]; t < g.ptr[(size_t) u + 1]; t++)
        {
            const int v = g.adj[(size_t) t];
            if (part[(size_t) v] != pid || mark[(size_t) v] == stamp) continue;
            mark[(size_t) v] = stamp;
            level[(size_t) v] = level[(size_t) u] + 1;
            order.push_back(v);
        }
    }
}

// pseudo-peripheral vertex of the component of `start` inside part pid
inline int pseudo_peripheral(const Graph &g, const std::vector<int> &part, int pid, int start, int &stamp, std::vector<int> &mark,
                      std::vector<int> &level, std::vector<int> &order)
{
    int root = start, ecc = -1;
    for (int iter = 0; iter < 8; iter++)
    {
        bfs(g, part, pid, root, ++stamp, mark, level, order);
        const int e = level[(size_t) order.back()];
        if (e <= ecc) break;
        ecc = e;
        // a vertex of smallest degree in the last level
        int best = order.back(), bestdeg = g.ptr[(size_t) best + 1] - g.ptr[(size_t) best];
        for (size_t t = order.size(); t-- > 0;)
        {
            const int v = order[t];
            if (level[(size_t) v] != e) break;
            const int d = g.ptr[(size_t) v + 1] - g.ptr[(size_t) v];
            if (d < bestdeg) { best = v; bestdeg = d; }
        }
        if (best == root) break;
        root = best;
    }
    return root;
}

// All vertices of part pid in breadth-first order from pseudo-peripheral roots (one component after the other).
// rcm = true: neighbours are visited by ascending degree and every component's order is reversed.
// `placed` (one int per vertex, any content) marks with a fresh stamp what is already in `out`.
inline void part_order(const Graph &g, const std::vector<int> &part, int pid, const std::vector<int> &members, bool rcm, int &stamp,
                std::vector<int> &mark, std::vector<int> &level, std::vector<int> &placed, std::vector<int> &scratch,
                std::vector<int> &out)
{
    out.clear();
    std::vector<int> nb;
    const int pstamp = ++stamp;
    for (int m0 : members)
    {
        if (placed[(size_t) m0] == pstamp) continue;
        const int root = pseudo_peripheral(g, part, pid, m0, stamp, mark, level, scratch);
        const int st = ++stamp;
        const size_t first = out.size();
        out.push_back(root);
        mark[(size_t) root] = st;
        for (size_t head = first; head < out.size(); head++)
        {
            const int u = out[head];
            nb.clear();
            for (int t = g.ptr[(size_t) u]; t < g.ptr[(size_t) u + 1]; t++)
            {
                const int v = g.adj[(size_t) t];
                if (part[(size_t) v] != pid || mark[(size_t) v] == st) continue;
                mark[(size_t) v] = st;
                nb.push_back(v);
            }
            if (rcm)
                std::sort(nb.begin(), nb.end(), [&](int a, int b) {
                    const int da = g.ptr[(size_t) a + 1] - g.ptr[(size_t) a], db = g.ptr[(size_t) b + 1] - g.ptr[(size_t) b];
                    return da != db ? da < db : a < b;
                });
            out.insert(out.end(), nb.begin(), nb.end());
        }
        for (size_t t = first; t < out.size(); t++) placed[(size_t) out[t]] = pstamp;
        if (rcm) std::reverse(out.begin() + (long) first, out.end());
    }
}

// Row groups of a square CSR (consecutive rows with identical, non-empty column lists) and the quotient graph of the
// pattern of A + A^T over them, without self loops.  grp[r] = group of row r, rep[s] = first row of group s; the
// rows of group s are rep[s] .. rep[s] + weight[s] - 1 (weight = row count).  Columns must lie in [0, nrow).
inline void group_graph(int nrow, const int *rowptr, const int *colidx, std::vector<int> *grp_out, std::vector<int> *rep_out,
                        Graph *gp)
{
    Graph &g = *gp;
    std::vector<int> &grp = *grp_out, &rep = *rep_out;
    grp.assign((size_t) nrow, 0);
    int ng = 0;
    for (int r = 0; r < nrow; r++)
    {
        bool same = false;
        if (r > 0)
        {
            const int la = rowptr[r] - rowptr[r - 1], lb = rowptr[r + 1] - rowptr[r];
            same = (la == lb) && lb > 0 && memcmp(colidx + rowptr[r - 1], colidx + rowptr[r], sizeof(int) * (size_t) lb) == 0;
        }
        if (!same) ng++;
        grp[(size_t) r] = ng - 1;
    }
    g.n = ng;
    g.weight.assign((size_t) ng, 0);
    rep.assign((size_t) ng, 0);
    for (int r = nrow - 1; r >= 0; r--) { g.weight[(size_t) grp[(size_t) r]]++; rep[(size_t) grp[(size_t) r]] = r; }
    std::vector<std::vector<int>> nbr((size_t) ng);
    {
        std::vector<int> last((size_t) ng, -1);
        for (int s = 0; s < ng; s++)
        {
            const int r = rep[(size_t) s];
            for (int p = rowptr[r]; p < rowptr[r + 1]; p++)
            {
                const int t = grp[(size_t) colidx[p]];
                if (t == s || last[(size_t) t] == s) continue;
                last[(size_t) t] = s;
                nbr[(size_t) s].push_back(t);
            }
        }
        std::vector<std::vector<int>> rev((size_t) ng);
        for (int s = 0; s < ng; s++)
            for (int t : nbr[(size_t) s]) rev[(size_t) t].push_back(s);
        for (int s = 0; s < ng; s++)
        {
            std::vector<int> &v = nbr[(size_t) s];
            v.insert(v.end(), rev[(size_t) s].begin(), rev[(size_t) s].end());
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
        }
    }
    g.ptr.assign((size_t) ng + 1, 0);
    for (int s = 0; s < ng; s++) g.ptr[(size_t) s + 1] = g.ptr[(size_t) s] + (int) nbr[(size_t) s].size();
    g.adj.resize((size_t) g.ptr[(size_t) ng]);
    for (int s = 0; s < ng; s++) std::copy(nbr[(size_t) s].begin(), nbr[(size_t) s].end(), g.adj.begin() + g.ptr[(size_t) s]);
}

}  // namespace gbfs
}  // namespace crp
