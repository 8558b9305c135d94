// panel_format.cpp -- host construction of the row-panel format (panel_format.h): the panels themselves.  Their processing
// orders are in panel_order.cpp, the team formats built on them in team_format.cpp, team2_format.cpp and team2r_format.cpp.
#include <algorithm>
#include <string.h>
#include "panel_format.h"
#include "team_stages.h"
#include "knobs.h"
#include "par.h"

namespace crp {

namespace {

struct Trip
{
    uint32_t key;
    int      col;
    int      r;
    int      p;    // position in the CSR arrays (keeps duplicates in input order)
};

// Visits the entries of one panel in order; fn(col, rmask, pos[R]) with pos[r] = CSR
// position of row r's value or -1.
template <typename F>
void panel_entries(int nrow, const int *rowptr, const int *colidx, int R, int panel, std::vector<Trip> &tmp, F fn)
{
    const int r0 = panel * R, r1 = std::min(nrow, r0 + R);
    tmp.clear();
    for (int r = r0; r < r1; r++)
        for (int p = rowptr[r]; p < rowptr[r + 1]; p++) tmp.push_back({col_key(colidx[p]), colidx[p], r - r0, p});
    std::sort(tmp.begin(), tmp.end(), [](const Trip &a, const Trip &b) {
        if (a.key != b.key) return a.key < b.key;
        if (a.r != b.r) return a.r < b.r;
        return a.p < b.p;
    });
    int pos[16];
    size_t i = 0;
    while (i < tmp.size())
    {
        // [i, j): every (row, value) of one column, ordered by (row, input position).
        // The k-th occurrence of the column inside a row goes to the k-th entry, so a
        // row that repeats a column (duplicates are legal: examples/mmio_utils.c keeps
        // them) opens further entries and keeps its input order.
        size_t j = i;
        int max_occ = 0, occ = 0;
        const uint32_t k0 = tmp[i].key;
        while (j < tmp.size() && tmp[j].key == k0)
        {
            occ = (j > i && tmp[j - 1].r == tmp[j].r) ? occ + 1 : 0;
            tmp[j].key = (uint32_t) occ;      // key is not needed any more inside the group
            if (occ > max_occ) max_occ = occ;
            j++;
        }
        for (int e = 0; e <= max_occ; e++)
        {
            unsigned mask = 0;
            for (int r = 0; r < R; r++) pos[r] = -1;
            for (size_t t = i; t < j; t++)
                if ((int) tmp[t].key == e)
                {
                    mask |= 1u << tmp[t].r;
                    pos[tmp[t].r] = tmp[t].p;
                }
            fn(tmp[i].col, mask, pos);
        }
        i = j;
    }
}

}  // namespace

double PanelHost::fill() const
{
    return real_entries > 0 ? (double) nnz / ((double) real_entries * R) : 1.0;
}

bool build_compact_values(PanelHost *p)
{
    if (p->R != 8) return false;
    const int np = p->npanel;
    p->cbase.assign((size_t) np + 1, 0);
    std::vector<long long> cnt((size_t) np, 0);
    bool fits = true;
    parallel_chunks(np, 4096, [&](long long b, long long e, int) {
        for (long long pn = b; pn < e; pn++)
        {
            long long c = 0;
            for (int q = p->pptr[(size_t) pn]; q < p->pptr[(size_t) pn + 1]; q++) c += __builtin_popcount(entry_mask(*p, (size_t) q));
            cnt[(size_t) pn] = c;
        }
    });
    for (int pn = 0; pn < np; pn++)
    {
        if (cnt[(size_t) pn] >= (1LL << 24)) fits = false;
        p->cbase[(size_t) pn + 1] = p->cbase[(size_t) pn] + cnt[(size_t) pn];
    }
    const long long total = p->cbase[(size_t) np];
    if (!fits || total >= (1LL << 32)) { p->cbase.clear(); return false; }
    const size_t nent = p->pcol.size();
    p->cmo.resize(nent);
    parallel_fill(p->cval, (size_t) total + 16, 0.0);
    big_vector<uint32_t> ebase;                       // absolute index of every entry's first value
    ebase.resize(nent);
    parallel_chunks(np, 4096, [&](long long b, long long e, int) {
        for (long long pn = b; pn < e; pn++)
        {
            long long off = 0;
            for (int q = p->pptr[(size_t) pn]; q < p->pptr[(size_t) pn + 1]; q++)
            {
                const unsigned m = entry_mask(*p, (size_t) q);
                p->cmo[(size_t) q] = m | ((uint32_t) off << 8);
                ebase[(size_t) q] = (uint32_t) (p->cbase[(size_t) pn] + off);
                for (int r = 0; r < 8; r++)
                    if ((m >> r) & 1u) p->cval[(size_t) (p->cbase[(size_t) pn] + off++)] = p->pval[(size_t) q * 8 + (size_t) r];
            }
        }
    });
    p->cmap.resize(p->pmap.size());
    parallel_chunks((long long) p->pmap.size(), 1 << 18, [&](long long b, long long e, int) {
        for (long long nz = b; nz < e; nz++)
        {
            const uint32_t sl = p->pmap[(size_t) nz];
            const size_t q = sl >> 3;
            const unsigned r = sl & 7u;
            p->cmap[(size_t) nz] = ebase[q] + (uint32_t) __builtin_popcount(entry_mask(*p, q) & ((1u << r) - 1u));
        }
    });
    return true;
}

long long count_panel_entries(int nrow, const int *rowptr, const int *colidx, int R)
{
    const int npanel = (nrow + R - 1) / R;
    std::vector<long long> part((size_t) host_threads(), 0);
    parallel_chunks(npanel, 512, [&](long long b, long long e, int tid) {
        std::vector<Trip> tmp;
        long long cnt = 0;
        for (long long pn = b; pn < e; pn++)
            panel_entries(nrow, rowptr, colidx, R, (int) pn, tmp, [&](int, unsigned, const int *) { cnt++; });
        part[(size_t) tid] += cnt;
    });
    long long tot = 0;
    for (long long v : part) tot += v;
    return tot;
}

long long count_block_union(int nrow, const int *rowptr, const int *colidx, int block)
{
    const int nblk = (nrow + block - 1) / block;
    std::vector<long long> part((size_t) host_threads(), 0);
    parallel_chunks(nblk, 256, [&](long long b, long long e, int tid) {
        std::vector<int> tmp;
        long long cnt = 0;
        for (long long g = b; g < e; g++)
        {
            const int r0 = (int) g * block, r1 = std::min(nrow, r0 + block);
            tmp.assign(colidx + rowptr[r0], colidx + rowptr[r1]);
            std::sort(tmp.begin(), tmp.end());
            cnt += (long long) (std::unique(tmp.begin(), tmp.end()) - tmp.begin());
        }
        part[(size_t) tid] += cnt;
    });
    long long tot = 0;
    for (long long v : part) tot += v;
    return tot;
}

void build_panels(int nrow, const int *rowptr, const int *colidx, const double *val, int R, PanelHost *out,
                  bool team_schedule, bool need_order)
{
    const int npanel = (nrow + R - 1) / R;
    out->R = R;
    out->npanel = npanel;
    out->nnz = rowptr[nrow];
    out->pptr.assign((size_t) npanel + 1, 0);
    // pass 1: entry counts per panel
    std::vector<int> cnt((size_t) npanel, 0);
    parallel_chunks(npanel, 512, [&](long long b, long long e, int) {
        std::vector<Trip> tmp;
        for (long long pn = b; pn < e; pn++)
        {
            int c = 0;
            panel_entries(nrow, rowptr, colidx, R, (int) pn, tmp, [&](int, unsigned, const int *) { c++; });
            cnt[(size_t) pn] = c;
        }
    });
    long long real = 0;
    for (int pn = 0; pn < npanel; pn++)
    {
        real += cnt[pn];
        const int padded = (cnt[pn] + PANEL_PAD - 1) / PANEL_PAD * PANEL_PAD;
        out->pptr[pn + 1] = out->pptr[pn] + padded;
    }
    out->real_entries = real;
    const size_t total = (size_t) out->pptr[npanel];
    parallel_fill(out->pcol, total, 0);
    parallel_fill(out->pmask4, total / 4 + 2, 0u);
    const bool with_vals = val != nullptr;
    if (with_vals) parallel_fill(out->pval, total * (size_t) R, 0.0);
    parallel_fill(out->pmap, (size_t) rowptr[nrow], 0u);
    // pass 2: fill
    parallel_chunks(npanel, 512, [&](long long b, long long e, int) {
        std::vector<Trip> tmp;
        for (long long pn = b; pn < e; pn++)
        {
            size_t q = (size_t) out->pptr[pn];
            const size_t qend = (size_t) out->pptr[pn + 1];
            int last_col = 0;
            panel_entries(nrow, rowptr, colidx, R, (int) pn, tmp, [&](int col, unsigned mask, const int *pos) {
                out->pcol[q] = col;
                // pmask4 words are private to a panel: panel starts are multiples of 4
                out->pmask4[q >> 2] |= (mask & 0xFFu) << (8 * (q & 3));
                for (int r = 0; r < R; r++)
                    if (pos[r] >= 0)
                    {
                        if (with_vals) out->pval[q * (size_t) R + r] = val[pos[r]];
                        out->pmap[(size_t) pos[r]] = (uint32_t) (q * (size_t) R + r);
                    }
                last_col = col;
                q++;
            });
            for (; q < qend; q++) out->pcol[q] = last_col;   // padding: valid address, mask 0
        }
    });
    // processing order.  CRPSPMM_PANEL_ORDER: 0 natural, 1 breadth-first groups, 2 stride lattice of panels,
    // 3 team schedule (2 and 3 only when the matrix has a stride lattice, else natural); unset = team
    // schedule (R = 8) or panel lattice (R = 4) when a lattice is detected, else breadth-first groups.
    out->porder.clear();
    out->psync.clear();
    if (!need_order) return;
    const int group = 16;                                       // panels per breadth-first group
    const int mode = knobs().panel_order;
    const int chunk = ((((npanel + 3) / 4) + 7) / 8) * 4;      // order positions per XCD (the kernels' block -> XCD map)
    bool done = false;
    out->psync.clear();
    if ((mode == 3 || mode == -1) && R == 8 && team_schedule && npanel >= 64)
    {
        double D1, D2;
        int M;
        if (detect_stride_lattice(nrow, rowptr, colidx, R, &D1, &D2, &M))
        {
            // workgroups of four waves = 2 x 2 teeth (six-wave workgroups, 3 x 2 teeth, were measured slower in round 1: 0.44
            // against 0.34 ms on the pwtk stand-in -- at 3 waves per SIMD only one six-wave workgroup fits a CU)
            TeamHost th;
            build_teams(*out, nrow, rowptr, colidx, &th, 4);
            apply_team_schedule(out, th);
            done = true;
        }
    }
    if (!done && (mode == 2 || mode == 3 || mode == -1))
        done = stride_lattice_order(nrow, rowptr, colidx, R, npanel, chunk, &out->porder);
    if (!done && (mode == 0 || mode == 2 || mode == 3))
    {
        out->porder.resize((size_t) npanel);
        for (int i = 0; i < npanel; i++) out->porder[(size_t) i] = i;
        done = true;
    }
    if (!done) locality_order(*out, group, &out->porder);
}

void apply_team_schedule(PanelHost *p, const TeamHost &t)
{
    const int R = p->R, T = t.T;
    big_vector<int> ncol(p->pcol.size(), 0);
    big_vector<uint32_t> nmask4(p->pmask4.size(), 0u);
    big_vector<double> nval(p->pval.size(), 0.0);
    std::vector<long long> moved(p->pcol.size(), -1);        // old entry -> new entry
    for (int g = 0; g < t.nteam; g++)
        for (int w = 0; w < T; w++)
        {
            const int panel = t.tpanel[(size_t) g * T + w];
            if (panel < 0) continue;
            size_t dst = (size_t) p->pptr[panel];
            int last = 0;
            for (int q = t.tptr[(size_t) g]; q < t.tptr[(size_t) g + 1]; q++)
            {
                const int src = t.tsrc[(size_t) q * T + w];
                if (src < 0) continue;
                ncol[dst] = p->pcol[(size_t) src];
                nmask4[dst >> 2] |= entry_mask(*p, (size_t) src) << (8 * (dst & 3));
                memcpy(&nval[dst * R], &p->pval[(size_t) src * R], sizeof(double) * R);
                moved[(size_t) src] = (long long) dst;
                last = ncol[dst];
                dst++;
            }
            for (; dst < (size_t) p->pptr[panel + 1]; dst++) ncol[dst] = last;       // padding: valid row, mask 0
        }
    for (uint32_t &slot : p->pmap) slot = (uint32_t) (moved[slot / R] * R + slot % R);
    p->pcol.swap(ncol);
    p->pmask4.swap(nmask4);
    p->pval.swap(nval);
    p->porder.assign((size_t) t.nteam * T, -1);
    p->psync.assign((size_t) t.nteam, 0);
    for (int pos = 0; pos < t.nteam; pos++)
    {
        int minnr = 1 << 30;
        for (int w = 0; w < T; w++)
        {
            const int panel = t.tpanel[(size_t) t.torder[(size_t) pos] * T + w];
            p->porder[(size_t) pos * T + w] = panel;
            if (panel >= 0) minnr = std::min(minnr, (p->pptr[panel + 1] - p->pptr[panel]) / PANEL_PAD);
        }
        p->psync[(size_t) pos] = (minnr == (1 << 30) || minnr < 2) ? 0 : minnr - 1;
    }
}

}  // namespace crp
