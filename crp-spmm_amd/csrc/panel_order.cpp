// panel_order.cpp -- processing orders of the row panels: stride-lattice detection and order, breadth-first groups (panel_format.h).
#include <algorithm>
#include <cmath>
#include "panel_format.h"
#include "par.h"

namespace crp {

bool detect_stride_lattice(int nrow, const int *rowptr, const int *colidx, int R, double *D1_, double *D2_, int *M_)
{
    if (nrow < 4096) return false;
    // histogram of |col - row| over the locally owned columns, 64-row buckets
    // 8-row buckets up to 2 M rows (the strides of a grid with short lines -- 56 nodes x 3 unknowns = 168 rows -- then
    // separate from the near band: fem3d stand-in, lattice teams of 2 x 2 lines x 2 panels need 5.7 union entries per row
    // against 6.95 for clusters, 0.913 -> 0.838 ms at n = 256), 64-row buckets beyond (one histogram per thread).
    const int SH = nrow <= (1 << 21) ? 3 : 6;                   // log2 of the bucket width
    const size_t nb = ((size_t) nrow >> SH) + 2;
    const int nt = host_threads();
    std::vector<std::vector<long long>> cnt_t((size_t) nt, std::vector<long long>(nb, 0)), sum_t(cnt_t);
    parallel_chunks(nrow, 4096, [&](long long b, long long e, int tid) {
        std::vector<long long> &cnt = cnt_t[(size_t) tid], &sum = sum_t[(size_t) tid];
        for (long long r = b; r < e; r++)
            for (int p = rowptr[r]; p < rowptr[r + 1]; p++)
            {
                const int c = colidx[p];
                if (c < 0) continue;
                long long d = (long long) c - r;
                if (d < 0) d = -d;
                const size_t k = std::min((size_t) (d >> SH), nb - 1);
                cnt[k]++;
                sum[k] += d;
            }
    });
    std::vector<long long> cnt(nb, 0), sum(nb, 0);
    long long total = 0;
    for (int t = 0; t < nt; t++)
        for (size_t k = 0; k < nb; k++) { cnt[k] += cnt_t[(size_t) t][k]; sum[k] += sum_t[(size_t) t][k]; }
    for (size_t k = 0; k < nb; k++) total += cnt[k];
    if (total == 0) return false;
    // runs of non-empty buckets (one empty bucket allowed inside a run)
    struct Run { long long w; double center; };
    std::vector<Run> far;
    for (size_t k = 0; k < nb;)
    {
        if (cnt[k] == 0) { k++; continue; }
        size_t e = k;
        long long w = 0, sm = 0;
        while (e < nb && (cnt[e] > 0 || (e + 1 < nb && cnt[e + 1] > 0)))
        {
            w += cnt[e];
            sm += sum[e];
            e++;
        }
        if (k > 0 && w * 100 >= total * 2) far.push_back({w, (double) sm / (double) w});
        k = e;
    }
    // D1 = the nearest far cluster that carries >= 6 % of the nonzeros.  The outer stride may show up as
    // several clusters (a 27-point stencil has nx*ny - nx, nx*ny, nx*ny + nx): clusters within 1.5 D1 of
    // each other are one group, D2 = centre of mass of the heaviest group beyond D1 (>= 6 % as well).
    // Anything between the two, or beyond the second, means another shape: left alone.
    size_t i1 = far.size();
    for (size_t t = 0; t < far.size(); t++)
        if (far[t].w * 100 >= total * 6) { i1 = t; break; }
    if (i1 > 0 || i1 + 1 >= far.size()) return false;        // (a light cluster in front of D1 would be a third stride)
    const double D1 = far[0].center;
    double D2 = 0.0;
    {
        long long gw = 0;
        double gs = 0.0, first = far[1].center, last = far[1].center;
        for (size_t t = 1; t < far.size(); t++)
        {
            if (far[t].center - last > 1.5 * D1) return false;          // a second group further out
            gw += far[t].w;
            gs += far[t].center * (double) far[t].w;
            last = far[t].center;
        }
        if (gw * 100 < total * 6 || last - first > 3.0 * D1) return false;
        D2 = gs / (double) gw;
    }
    const double ratio = D2 / D1;
    const int M = (int) (ratio + 0.5);
    const double d1min = 8.0;                                   // teeth of >= 8 panels
    if (D1 < d1min * R || M < 2 || std::abs(ratio - M) > 0.02 * M || D2 * 2 > nrow) return false;
    *D1_ = D1;
    *D2_ = D2;
    *M_ = M;
    return true;
}

void lattice_coords(int panel, int R, double D1, double D2, int M, int *i_, int *j_, int *t_)
{
    const double r = (double) panel * R;
    const int j = (int) (r / D2);
    const double rem = r - j * D2;
    int i = (int) (rem / D1);
    if (i > M) i = M;
    *i_ = i;
    *j_ = j;
    *t_ = (int) ((rem - i * D1) / R);
}

bool stride_lattice_order(int nrow, const int *rowptr, const int *colidx, int R, int npanel, int chunk,
                          std::vector<int> *order)
{
    if (npanel < 64 || chunk < 1) return false;
    double D1, D2;
    int M;
    if (!detect_stride_lattice(nrow, rowptr, colidx, R, &D1, &D2, &M)) return false;

    // tooth coordinates of every panel
    struct Key { int i, j, t, p; };
    std::vector<Key> keys((size_t) npanel);
    for (int p = 0; p < npanel; p++)
    {
        int i, j, t;
        lattice_coords(p, R, D1, D2, M, &i, &j, &t);
        keys[(size_t) p] = {i, j, t, p};
    }
    // XCD blocks: consecutive teeth in (i, j) order, cut every `chunk` panels
    std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {
        if (a.i != b.i) return a.i < b.i;
        if (a.j != b.j) return a.j < b.j;
        return a.p < b.p;
    });
    // lockstep sweep along t inside every block
    for (size_t s0 = 0; s0 < keys.size(); s0 += (size_t) chunk)
    {
        const size_t s1 = std::min(keys.size(), s0 + (size_t) chunk);
        std::sort(keys.begin() + (long) s0, keys.begin() + (long) s1, [](const Key &a, const Key &b) {
            if (a.t != b.t) return a.t < b.t;
            return a.p < b.p;
        });
    }
    order->resize((size_t) npanel);
    for (int q = 0; q < npanel; q++) (*order)[(size_t) q] = keys[(size_t) q].p;
    return true;
}

void locality_order(const PanelHost &p, int group, std::vector<int> *order)
{
    const int np = p.npanel;
    order->resize((size_t) np);
    if (group < 1) group = 1;
    const int ng = (np + group - 1) / group;
    if (ng <= 2)
    {
        for (int i = 0; i < np; i++) (*order)[i] = i;
        return;
    }
    // distinct B rows per group (column codes folded to a dense id space)
    int max_loc = -1, max_rem = -1;
    for (int c : p.pcol)
    {
        if (c >= 0) { if (c > max_loc) max_loc = c; }
        else if (~c > max_rem) max_rem = ~c;
    }
    const long long nb = (long long) max_loc + 1 + (long long) max_rem + 1;
    auto bid = [&](int c) -> long long { return c >= 0 ? c : (long long) max_loc + 1 + (~c); };
    std::vector<std::vector<int>> rows_of((size_t) ng);
    parallel_chunks(ng, 64, [&](long long b, long long e, int) {
        for (long long g = b; g < e; g++)
        {
            const int pa = (int) g * group, pb = std::min(np, pa + group);
            std::vector<int> &v = rows_of[(size_t) g];
            for (int q = p.pptr[pa]; q < p.pptr[pb]; q++) v.push_back((int) bid(p.pcol[(size_t) q]));
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
        }
    });
    // inverted index: B row -> groups touching it
    std::vector<int> deg((size_t) nb + 1, 0);
    for (int g = 0; g < ng; g++)
        for (int c : rows_of[(size_t) g]) deg[(size_t) c + 1]++;
    for (long long c = 0; c < nb; c++) deg[(size_t) c + 1] += deg[(size_t) c];
    std::vector<int> inv((size_t) deg[(size_t) nb]), fillp(deg.begin(), deg.end() - 1);
    for (int g = 0; g < ng; g++)
        for (int c : rows_of[(size_t) g]) inv[(size_t) fillp[(size_t) c]++] = g;
    // breadth-first over groups; B rows shared by very many groups (dense columns) say nothing
    // about locality and are skipped
    const int hub = 64;
    std::vector<char> seen((size_t) ng, 0);
    std::vector<int> gorder, nbrs;
    gorder.reserve((size_t) ng);
    size_t head = 0;
    for (int start = 0; start < ng; start++)
    {
        if (seen[(size_t) start]) continue;
        seen[(size_t) start] = 1;
        gorder.push_back(start);
        while (head < gorder.size())
        {
            const int u = gorder[head++];
            nbrs.clear();
            for (int c : rows_of[(size_t) u])
            {
                const int d0 = deg[(size_t) c], d1 = deg[(size_t) c + 1];
                if (d1 - d0 > hub) continue;
                for (int t = d0; t < d1; t++)
                    if (!seen[(size_t) inv[(size_t) t]])
                    {
                        seen[(size_t) inv[(size_t) t]] = 1;
                        nbrs.push_back(inv[(size_t) t]);
                    }
            }
            std::sort(nbrs.begin(), nbrs.end());
            gorder.insert(gorder.end(), nbrs.begin(), nbrs.end());
        }
    }
    size_t w = 0;
    for (int g : gorder)
        for (int pn = g * group; pn < std::min(np, (g + 1) * group); pn++) (*order)[w++] = pn;
}

}  // namespace crp
