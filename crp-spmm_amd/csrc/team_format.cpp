// team_format.cpp -- teams of panels whose B rows one workgroup loads once (panel_format.h, TeamHost): which panels form a
// team, the union of their entries, and the order in which the teams are processed.  build_teams() at the end of the file is the
// list of the stages (the greedy clustering two of them use is in team_cluster.cpp); team2_format.cpp and team2r_format.cpp build
// their streams on its result.
#include <algorithm>
#include <cmath>
#include <string.h>
#include "locality.h"
#include "panel_format.h"
#include "team_cluster.h"
#include "team_stages.h"
#include "par.h"

namespace crp {

// ---- build_teams, stage by stage ----------------------------------------------------------------------------------------

namespace {

constexpr int TMAX = 8;
// shape of a lattice team in tooth coordinates: LAT_SI x LAT_SJ teeth x st consecutive panels along the teeth.  Teams of eight
// (team2): 2 x 2 teeth x 2 consecutive panels -- 4.98 union entries per row on the pwtk stand-in, against 6.5 for
// 4 x 2 x 1 and 5.4 for eight consecutive panels (0.351 / 0.418 / 0.424 ms with the first team2 kernel)
constexpr int LAT_SI = 2, LAT_SJ = 2;

struct Lattice { double D1 = 0, D2 = 0; int M = 0, R = 8, st = 1; };       // a detected stride lattice and the team's extent along the teeth

// team column (a, b), position tt along the teeth and slot inside the team of a panel
struct LatticePlace { int a, b, tt, slot; long long key() const { return ((long long) a << 40) | ((long long) b << 24) | (long long) tt; } };
LatticePlace lattice_place(const Lattice &la, int panel)
{
    int i, j, t;
    lattice_coords(panel, la.R, la.D1, la.D2, la.M, &i, &j, &t);
    return {i / LAT_SI, j / LAT_SJ, t / la.st, (i % LAT_SI) + LAT_SI * ((j % LAT_SJ) + LAT_SJ * (t % la.st))};
}

// ---- stage: entries of every panel before its padding (counted once, by all threads: the builders ask several times per panel)
std::vector<int> real_entry_counts(const PanelHost &p)
{
    std::vector<int> rcount((size_t) p.npanel, 0);
    parallel_chunks(p.npanel, 4096, [&](long long b, long long e, int) {
        for (long long panel = b; panel < e; panel++)
        {
            int c = 0;
            for (int q = p.pptr[(size_t) panel]; q < p.pptr[(size_t) panel + 1]; q++)
            {
                if (entry_mask(p, (size_t) q) == 0) break;          // padding starts here: real entries always carry a row
                c++;
            }
            rcount[(size_t) panel] = c;
        }
    });
    return rcount;
}

// ---- stage: grouping -- which panels form a team
struct Grouping
{
    bool lattice = false, clustered = false;
    bool seeded = false;                       // taken from the teams of an earlier format of the same panels
    std::vector<int> team_of, slot_of;         // clustered teams: team and slot of every panel
};

// The panels are of two kinds: at least 15 % of them hold under half the mean number of entries.
bool two_kinds_of_panels(const std::vector<int> &rcount)
{
    const int np = (int) rcount.size();
    long long tot = 0;
    for (int q = 0; q < np; q++) tot += rcount[(size_t) q];
    long long small = 0;
    for (int q = 0; q < np; q++) small += (2LL * rcount[(size_t) q] * np < tot);
    return small * 100 >= 15LL * np;
}

// the panels in the order of their MEDIAN column (ties: row order)
void median_column_order(const PanelHost &p, const std::vector<int> &rcount, std::vector<int> *pord)
{
    const int np = p.npanel;
    std::vector<uint32_t> med((size_t) np, 0);
    parallel_chunks(np, 4096, [&](long long b, long long e, int) {
        for (long long q = b; q < e; q++)
        {
            const int e0 = p.pptr[(size_t) q], cnt = rcount[(size_t) q];
            med[(size_t) q] = cnt > 0 ? col_key(p.pcol[(size_t) (e0 + cnt / 2)]) : 0xFFFFFFFFu;      // (entries are in column order)
        }
    });
    std::stable_sort(pord->begin(), pord->end(), [&](int x, int y) { return med[(size_t) x] < med[(size_t) y]; });
}

// Union entries of a grouping = distinct (group, column) pairs; item_of[panel] = the panel's item in the key CSR.
template <typename GroupFn>
long long union_total(int np, const std::vector<int> &item_of, const std::vector<long long> &iptr, const big_vector<uint32_t> &ikey, GroupFn group_of_panel)
{
    std::vector<std::pair<long long, int>> ord((size_t) np);
    for (int q = 0; q < np; q++) ord[(size_t) q] = {group_of_panel(q), q};
    std::sort(ord.begin(), ord.end());
    std::vector<size_t> gs;
    for (size_t t = 0; t < ord.size(); t++)
        if (t == 0 || ord[t].first != ord[t - 1].first) gs.push_back(t);
    gs.push_back(ord.size());
    const int ngr = (int) gs.size() - 1;
    std::vector<long long> part((size_t) ngr, 0);
    parallel_chunks(ngr, 256, [&](long long b, long long e, int) {
        std::vector<uint32_t> keys;
        for (long long g = b; g < e; g++)
        {
            keys.clear();
            for (size_t t = gs[(size_t) g]; t < gs[(size_t) g + 1]; t++)
            {
                const int q = item_of[(size_t) ord[t].second];
                keys.insert(keys.end(), ikey.begin() + (long) iptr[(size_t) q], ikey.begin() + (long) iptr[(size_t) q + 1]);
            }
            std::sort(keys.begin(), keys.end());
            part[(size_t) g] = (long long) (std::unique(keys.begin(), keys.end()) - keys.begin());
        }
    });
    long long tot = 0;
    for (long long v : part) tot += v;
    return tot;
}

// Off a lattice, teams of eight are CLUSTERED: the eight panels of a team are picked for the columns they share
// (greedy_cluster), not for being consecutive -- on a 3-D stencil in natural order eight consecutive panels are
// a thin strip of one grid line (9.9 union entries per row on the 27-point fem3d stand-in), a cluster is a
// compact block (6.9); nlpkkt stand-in 7.1 (its lattice teams) -> 4.4.  `lattice_found`: la holds a detected lattice.
Grouping group_panels(const PanelHost &p, const std::vector<int> &rcount, int T, bool lattice_found, const Lattice &la, TeamSeed *seed)
{
    const int np = p.npanel;
    Grouping gr;
    gr.lattice = lattice_found;
    gr.clustered = T >= 8 && np >= 2 * T;
    gr.seeded = seed != nullptr && seed->valid && seed->T == T && seed->np == np;
    if (gr.seeded)
    {
        gr.clustered = seed->clustered;
        gr.lattice = seed->lattice;
        gr.team_of = seed->team_of;
        gr.slot_of = seed->slot_of;
        return gr;
    }
    if (gr.clustered)
    {
        std::vector<long long> iptr;
        big_vector<uint32_t> ikey;
        // The clustering works on ranges of consecutive items: the panels are taken in the order of their MEDIAN column,
        // so that panels far apart in the row numbering that read the same B rows (the dual rows of a KKT system and the
        // primal rows of the same nodes) fall into one range; for a mesh numbered along its own lines that is the row order.
        // Taken when the panels are of two kinds -- at least 15 % of them hold under half the mean number of entries --;
        // with panels of one size the rule changes nothing but the ties, and the row order is the better seed order
        // (shell stand-in 0.264 -> 0.275 ms with it, nlpkkt stand-in 2.39 -> 2.12).
        const bool mix = two_kinds_of_panels(rcount);
        std::vector<int> pord((size_t) np);
        for (int q = 0; q < np; q++) pord[(size_t) q] = q;
        if (mix) median_column_order(p, rcount, &pord);
        build_key_csr(np, [&](int i, big_vector<uint32_t> &buf) {
            const int q = pord[(size_t) i];
            const int e0 = p.pptr[q], e1 = e0 + rcount[(size_t) q];
            for (int e = e0; e < e1; e++) buf.push_back(col_key(p.pcol[(size_t) e]));
        }, &iptr, &ikey);
        {
            int ng = 0;
            std::vector<int> tof, sof;
            greedy_cluster(np, iptr, ikey, T, 1 << 15, &tof, &sof, &ng, mix);
            gr.team_of.assign((size_t) np, 0);
            gr.slot_of.assign((size_t) np, 0);
            for (int i = 0; i < np; i++) { gr.team_of[(size_t) pord[(size_t) i]] = tof[(size_t) i]; gr.slot_of[(size_t) pord[(size_t) i]] = sof[(size_t) i]; }
        }
        if (lattice_found)
        {
            // A lattice has both: its tooth-shaped teams sweep in lockstep along the teeth and re-fetch less (pwtk
            // stand-in: 1.8 x B against 2.1 x B for clusters with 5.0 / 4.9 union entries per row), so they stay
            // unless the clusters need clearly fewer B rows (nlpkkt stand-in: 7.1 -> 4.5 entries per row).
            std::vector<int> item_of((size_t) np);                 // panel -> its item in the key CSR
            for (int i = 0; i < np; i++) item_of[(size_t) pord[(size_t) i]] = i;
            const long long u_cl = union_total(np, item_of, iptr, ikey, [&](int q) { return (long long) gr.team_of[(size_t) q]; });
            const long long u_la = union_total(np, item_of, iptr, ikey, [&](int q) { return lattice_place(la, q).key(); });
            if ((double) u_la <= 1.15 * (double) u_cl) gr.clustered = false;
            else gr.lattice = false;
        }
    }
    if (seed != nullptr)
    {
        seed->T = T;
        seed->np = np;
        seed->clustered = gr.clustered;
        seed->lattice = gr.lattice;
        if (gr.clustered) { seed->team_of = gr.team_of; seed->slot_of = gr.slot_of; }
    }
    return gr;
}

// ---- stage: team formation -- the membership records (team key, slot) sorted into tpanel; teams come in key order, a slot that
// is taken twice (irregular tooth ends) opens a new team.  -> the key of every team.
struct TeamKey { int a, b, t; };
std::vector<TeamKey> form_teams(int np, int T, const Grouping &gr, const Lattice &la, std::vector<int> *tpanel)
{
    struct Mem { long long key; int slot, panel, a, b, t; };
    std::vector<Mem> mem((size_t) np);
    for (int q = 0; q < np; q++)
    {
        if (gr.clustered) mem[(size_t) q] = {(long long) gr.team_of[(size_t) q], gr.slot_of[(size_t) q], q, 0, 0, gr.team_of[(size_t) q]};
        else if (gr.lattice)
        {
            const LatticePlace lp = lattice_place(la, q);
            mem[(size_t) q] = {lp.key(), lp.slot, q, lp.a, lp.b, lp.tt};
        }
        else mem[(size_t) q] = {(long long) (q / T), q % T, q, 0, 0, q / T};
    }
    std::sort(mem.begin(), mem.end(), [](const Mem &x, const Mem &y) {
        if (x.key != y.key) return x.key < y.key;
        if (x.slot != y.slot) return x.slot < y.slot;
        return x.panel < y.panel;      // (cannot happen in exact arithmetic -- a panel's (team, slot) is its own --: makes the order total)
    });
    std::vector<TeamKey> tk;
    tpanel->clear();
    for (size_t s0 = 0; s0 < mem.size();)
    {
        size_t s1 = s0;
        int slots[TMAX];
        for (int w = 0; w < TMAX; w++) slots[w] = -1;
        while (s1 < mem.size() && mem[s1].key == mem[s0].key && slots[mem[s1].slot] < 0)
        {
            slots[mem[s1].slot] = mem[s1].panel;
            s1++;
        }
        for (int w = 0; w < T; w++) tpanel->push_back(slots[w]);
        tk.push_back({mem[s0].a, mem[s0].b, mem[s0].t});
        s0 = s1;
    }
    return tk;
}

// ---- stage: union merge.  Nodes: the union of the panels' entry lists, equal (column, occurrence) keys merged.
struct Node { int col; uint32_t mask; int src[TMAX]; int users; bool done; };

// The unions of `upool` consecutive teams share three arrays (teams_per_pool, team_stages.h), sized by the teams' panel entries, an
// upper bound on their union entries.  Team g: cnt[g] union entries at ucol[g] / umask[g], T * cnt[g] panel entries at usrc[g].
struct UnionPool { big_vector<int> col; big_vector<uint32_t> mask; big_vector<int> src; };
struct Unions
{
    int upool = 64;
    std::vector<UnionPool> pools;
    std::vector<int> cnt;
    std::vector<const int *> ucol, usrc;
    std::vector<const uint32_t *> umask;
};

// where the union entries of the team being merged go: the next free entries of its pool
struct UnionWriter
{
    int T;
    int *uc;
    uint32_t *um;
    int *us;                  // per union entry: panel entry of wave 0 .. T - 1 (or -1)
    size_t un = 0;            // union entries of the team so far
    void put(const Node &nd)
    {
        uc[un] = nd.col;
        um[un] = nd.mask;
        for (int u = 0; u < T; u++) us[un * (size_t) T + (size_t) u] = nd.src[u];
        un++;
    }
};

// Rounds of 8 union entries end at a barrier, so a round costs what its busiest wave
// costs; a wave's columns are clustered, and in column order the four waves would work
// one after the other.  The order inside a team is free (a row's products are summed in
// the order its wave meets them), so the entries are dealt out in balanced passes.
// Passes: every pass hands each wave that still has entries exactly ONE of them -- a set of open
// nodes whose user sets are disjoint and cover the waves (a node shared by A and B plus one
// shared by C and D; or four private nodes; ...).  All waves then meet a shared node after
// exactly the same number of own entries, i.e. in the same ring slot of the same round.
// list[w] = node ids of wave w, in column order.
void balanced_passes(std::vector<Node> &nodes, const std::vector<int> *list, int T, UnionWriter &out)
{
    int cursor[TMAX];
    for (int w = 0; w < TMAX; w++) cursor[w] = 0;
    size_t left = nodes.size();
    auto emit = [&](int id) {
        nodes[(size_t) id].done = true;
        left--;
        out.put(nodes[(size_t) id]);
    };
    while (left > 0)
    {
        bool covered[TMAX];
        for (int w = 0; w < TMAX; w++) covered[w] = false;
        for (int w = 0; w < T; w++)
        {
            if (covered[w]) continue;
            while (cursor[w] < (int) list[w].size() && nodes[(size_t) list[w][(size_t) cursor[w]]].done) cursor[w]++;
            // among the wave's next open nodes: the one with the most users, all of them uncovered
            int pick = -1, pick_users = 0;
            for (int t = cursor[w], seen = 0; t < (int) list[w].size() && seen < 96; t++)
            {
                const int id = list[w][(size_t) t];
                const Node &nd = nodes[(size_t) id];
                if (nd.done) continue;
                seen++;
                bool ok = true;
                for (int u = 0; u < T; u++)
                    if (nd.src[u] >= 0 && covered[u]) ok = false;
                if (ok && nd.users > pick_users) { pick = id; pick_users = nd.users; if (nd.users >= 3) break; }
            }
            if (pick < 0) continue;              // everything this wave has left is shared with a covered wave
            for (int u = 0; u < T; u++)
                if (nodes[(size_t) pick].src[u] >= 0) covered[u] = true;
            emit(pick);
        }
        // a pass that could place nothing would loop forever: take any open node (cannot happen while
        // a wave has an open node at all, its first open node is always eligible when it comes first)
        bool any_cov = false;
        for (int w = 0; w < T; w++) any_cov = any_cov || covered[w];
        if (!any_cov)
            for (size_t id = 0; id < nodes.size(); id++)
                if (!nodes[id].done) { emit((int) id); break; }
    }
}

// the nodes of team g: T-way merge of its panels' entry lists by (column key, occurrence inside the panel)
void merge_team_nodes(const PanelHost &p, const std::vector<int> &rcount, const int *tpanel, int T, std::vector<Node> &nodes, std::vector<int> *list)
{
    int head[TMAX], end[TMAX], occ[TMAX];
    for (int w = 0; w < T; w++)
    {
        const int panel = tpanel[w];
        head[w] = panel >= 0 ? p.pptr[panel] : 0;
        end[w] = panel >= 0 ? head[w] + rcount[(size_t) panel] : 0;
        occ[w] = 0;
    }
    nodes.clear();
    for (int w = 0; w < T; w++) list[w].clear();
    for (;;)
    {
        bool any = false;
        uint64_t best = 0;
        for (int w = 0; w < T; w++)
            if (head[w] < end[w])
            {
                const uint64_t k = ((uint64_t) col_key(p.pcol[(size_t) head[w]]) << 8) | (uint64_t) occ[w];
                if (!any || k < best) best = k;
                any = true;
            }
        if (!any) break;
        Node nd;
        nd.col = 0; nd.mask = 0; nd.users = 0; nd.done = false;
        for (int w = 0; w < T; w++) nd.src[w] = -1;
        for (int w = 0; w < T; w++)
            if (head[w] < end[w])
            {
                const int c = p.pcol[(size_t) head[w]];
                const uint64_t k = ((uint64_t) col_key(c) << 8) | (uint64_t) occ[w];
                if (k != best) continue;
                const int q = head[w];
                if (w < 4) nd.mask |= entry_mask(p, (size_t) q) << (8 * w);
                nd.col = c;
                nd.src[w] = q;
                nd.users++;
                list[w].push_back((int) nodes.size());
                head[w]++;
                occ[w] = (head[w] < end[w] && p.pcol[(size_t) head[w]] == c) ? occ[w] + 1 : 0;
            }
        nodes.push_back(nd);
    }
}

// passes = false: the union entries stay in column order -- the caller orders the union itself (build_team2 by the phase key), and
// the passes were a fifth of the nlpkkt240-size format's build time.
void merge_unions(const PanelHost &p, const std::vector<int> &rcount, const std::vector<int> &tpanel, int T, int nteam, bool passes, Unions *u)
{
    u->cnt.assign((size_t) nteam, 0);
    u->upool = teams_per_pool(nteam, 64);
    const int upool = u->upool, npool = (nteam + upool - 1) / upool;
    u->pools.resize((size_t) npool);
    u->ucol.assign((size_t) nteam, nullptr);
    u->usrc.assign((size_t) nteam, nullptr);
    u->umask.assign((size_t) nteam, nullptr);
    parallel_chunks(npool, 1, [&](long long pb, long long pe, int) {
        std::vector<Node> nodes;                               // (scratch of the builder thread, not of the team)
        std::vector<int> list[TMAX];                           // node ids of every wave, in column order
        for (long long pl = pb; pl < pe; pl++)
        {
            const long long b = pl * upool, e = std::min<long long>(nteam, b + upool);
            UnionPool &pool = u->pools[(size_t) pl];
            size_t cap = 0;
            for (long long g = b; g < e; g++)
                for (int w = 0; w < T; w++)
                {
                    const int panel = tpanel[(size_t) g * T + w];
                    if (panel >= 0) cap += (size_t) (p.pptr[panel + 1] - p.pptr[panel]);
                }
            pool.col.resize(cap);
            pool.mask.resize(cap);
            pool.src.resize(cap * (size_t) T);
            size_t pat = 0;                                    // union entries of the pool so far
            for (long long g = b; g < e; g++)
            {
                merge_team_nodes(p, rcount, &tpanel[(size_t) g * T], T, nodes, list);
                UnionWriter uw{T, pool.col.data() + pat, pool.mask.data() + pat, pool.src.data() + pat * (size_t) T};
                if (passes) balanced_passes(nodes, list, T, uw);
                else
                    for (const Node &nd : nodes) uw.put(nd);
                u->cnt[(size_t) g] = (int) uw.un;
                u->ucol[(size_t) g] = uw.uc;
                u->umask[(size_t) g] = uw.um;
                u->usrc[(size_t) g] = uw.us;
                pat += uw.un;
            }
        }
    });
}

// ---- stage: layout -- tptr, tcol, tmask, tsrc and the padding (filled by all threads: these arrays hold gigabytes on the
// nlpkkt240-size matrix, and the serial version of this stage was the longest single piece of its format build)
void layout_unions(const Unions &u, int T, TeamHost *out)
{
    const int nteam = out->nteam;
    out->tptr.assign((size_t) nteam + 1, 0);
    long long real = 0;
    for (int g = 0; g < nteam; g++)
    {
        real += u.cnt[(size_t) g];
        out->tptr[(size_t) g + 1] = out->tptr[(size_t) g] + (u.cnt[(size_t) g] + PANEL_PAD - 1) / PANEL_PAD * PANEL_PAD;
    }
    out->real_entries = real;
    const size_t total = (size_t) out->tptr[(size_t) nteam];
    out->tcol.resize(total);
    out->tmask.resize(total);
    out->tsrc.resize(total * (size_t) T);
    parallel_chunks(nteam, 256, [&](long long b, long long e, int) {
        for (long long g = b; g < e; g++)
        {
            const size_t cnt = (size_t) u.cnt[(size_t) g];
            size_t q = (size_t) out->tptr[(size_t) g];
            int last = 0;
            for (size_t t = 0; t < cnt; t++, q++)
            {
                out->tcol[q] = u.ucol[(size_t) g][t];
                out->tmask[q] = u.umask[(size_t) g][t];
                last = out->tcol[q];
            }
            int *ts = &out->tsrc[(size_t) out->tptr[(size_t) g] * T];
            if (cnt > 0) memcpy(ts, u.usrc[(size_t) g], sizeof(int) * cnt * (size_t) T);
            for (; q < (size_t) out->tptr[(size_t) g + 1]; q++)
            {
                out->tcol[q] = last;      // padding: valid row, no reader
                out->tmask[q] = 0u;
                for (int w = 0; w < T; w++) out->tsrc[q * (size_t) T + (size_t) w] = -1;
            }
        }
    });
}

// ---- stage: value offsets (T < 8 only: the team2 streams have their own) -- wave w of team g reads 8 values per own entry
// from entry tvoff[T g + w] on, in the order it meets its entries
void value_offsets(const Unions &u, int T, TeamHost *out)
{
    const int nteam = out->nteam;
    out->tvoff.assign((size_t) nteam * T + 1, 0);
    if (T >= 8) return;
    long long run = 0;
    for (int g = 0; g < nteam; g++)
        for (int w = 0; w < T; w++)
        {
            out->tvoff[(size_t) g * T + w] = run;
            const int *us = u.usrc[(size_t) g];
            for (size_t t = 0; t < (size_t) u.cnt[(size_t) g]; t++) run += us[t * (size_t) T + (size_t) w] >= 0;
        }
    out->tvoff[(size_t) nteam * T] = run;
}

// ---- stage: processing order of clustered teams.  The workgroups resident on an XCD at one time (64: 32 CUs x 2) start
// together and walk their unions by the same phase key, so rows shared INSIDE such a generation are requested together and
// served by the XCD's L2 once.  Generations = super-teams of 64 teams clustered by shared columns, again greedily; the kernel
// deals the order to the XCDs in eight contiguous runs.
// Order of the super-teams: the slab order of locality.cpp on their graph (two super-teams are adjacent when they share a B
// row; weight = union entries) -- eight slabs, one per XCD, each swept along its long axis, so that an XCD's L2 sees one compact
// region and consecutive generations are neighbours.
// (key, super-team) pairs are sorted per range of teams, in parallel -- the ranges greedy_cluster() worked on, so a super-team lies
// inside one; edges between super-teams of different ranges are left out except for a link between the last of a range and the
// first of the next, which keeps the slabs in range order.  -> rank of every super-team
std::vector<int> super_team_ranks(int nteam, int ns, const std::vector<int> &super_of, const std::vector<long long> &iptr, const big_vector<uint32_t> &ikey, int span)
{
    const int nrange = (nteam + span - 1) / span;
    std::vector<int> weight((size_t) ns, 0);
    std::vector<std::vector<std::pair<int, int>>> redges((size_t) nrange);
    parallel_chunks(nrange, 1, [&](long long rb, long long re, int) {
        for (long long rg = rb; rg < re; rg++)
        {
            const int g0 = (int) rg * span, g1 = std::min(nteam, g0 + span);
            std::vector<std::pair<uint32_t, int>> ks;
            ks.reserve((size_t) (iptr[(size_t) g1] - iptr[(size_t) g0]));
            for (int g = g0; g < g1; g++)
                for (long long q = iptr[(size_t) g]; q < iptr[(size_t) g + 1]; q++) ks.push_back({ikey[(size_t) q], super_of[(size_t) g]});
            std::sort(ks.begin(), ks.end());
            ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
            std::vector<std::pair<int, int>> &edges = redges[(size_t) rg];
            for (size_t a = 0; a < ks.size();)
            {
                size_t b = a;
                while (b < ks.size() && ks[b].first == ks[a].first) b++;
                for (size_t x = a; x < b; x++)
                {
                    weight[(size_t) ks[x].second]++;            // (a super-team belongs to one range: no race)
                    for (size_t y = a; y < b; y++)
                        if (x != y) edges.push_back({ks[x].second, ks[y].second});
                }
                a = b;
                if (edges.size() > (size_t) 1 << 22) { std::sort(edges.begin(), edges.end()); edges.erase(std::unique(edges.begin(), edges.end()), edges.end()); }
            }
            std::sort(edges.begin(), edges.end());
            edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
        }
    });
    std::vector<std::pair<int, int>> edges;
    for (int rg = 0; rg < nrange; rg++)
    {
        edges.insert(edges.end(), redges[(size_t) rg].begin(), redges[(size_t) rg].end());
        if (rg + 1 < nrange)
        {
            const int last = super_of[(size_t) std::min(nteam, (rg + 1) * span) - 1], first = super_of[(size_t) (rg + 1) * span];
            if (last != first) { edges.push_back({last, first}); edges.push_back({first, last}); }
        }
        redges[(size_t) rg].clear();
        redges[(size_t) rg].shrink_to_fit();
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    std::vector<int> gp((size_t) ns + 1, 0), ga(edges.size());
    for (size_t e = 0; e < edges.size(); e++) { gp[(size_t) edges[e].first + 1]++; ga[e] = edges[e].second; }
    for (int q = 0; q < ns; q++) gp[(size_t) q + 1] += gp[(size_t) q];
    std::vector<int> so;
    if (ns < 16 || !graph_slab_order(ns, gp, ga, weight, 8, &so))
    {
        so.resize((size_t) ns);
        for (int q = 0; q < ns; q++) so[(size_t) q] = q;
    }
    std::vector<int> srank((size_t) ns);
    for (int q = 0; q < ns; q++) srank[(size_t) so[(size_t) q]] = q;
    return srank;
}

void super_team_order(const Unions &u, int nteam, std::vector<int> *torder)
{
    constexpr int span = 1 << 13;                                    // teams per range of the clustering
    std::vector<long long> iptr;
    big_vector<uint32_t> ikey;
    build_key_csr(nteam, [&](int g, big_vector<uint32_t> &buf) {
        for (int t = 0; t < u.cnt[(size_t) g]; t++) buf.push_back(col_key(u.ucol[(size_t) g][t]));
    }, &iptr, &ikey);
    std::vector<int> super_of, sslot;
    int ns = 0;
    greedy_cluster(nteam, iptr, ikey, 64, span, &super_of, &sslot, &ns);   // the workgroups resident on an XCD
    const std::vector<int> srank = super_team_ranks(nteam, ns, super_of, iptr, ikey, span);
    std::sort(torder->begin(), torder->end(), [&](int x, int y) {
        if (super_of[(size_t) x] != super_of[(size_t) y]) return srank[(size_t) super_of[(size_t) x]] < srank[(size_t) super_of[(size_t) y]];
        return sslot[(size_t) x] < sslot[(size_t) y];
    });
}

// ---- stage: processing order of lattice teams -- XCD blocks of neighbouring team columns swept in lockstep along t
void lattice_strip_order(const std::vector<TeamKey> &tk, std::vector<int> *torder)
{
    const int chunk = ((int) torder->size() + 7) / 8;
    std::sort(torder->begin(), torder->end(), [&](int x, int y) {
        if (tk[(size_t) x].a != tk[(size_t) y].a) return tk[(size_t) x].a < tk[(size_t) y].a;
        if (tk[(size_t) x].b != tk[(size_t) y].b) return tk[(size_t) x].b < tk[(size_t) y].b;
        return x < y;
    });
    for (size_t s0 = 0; s0 < torder->size(); s0 += (size_t) chunk)
    {
        const size_t s1 = std::min(torder->size(), s0 + (size_t) chunk);
        std::sort(torder->begin() + (long) s0, torder->begin() + (long) s1, [&](int x, int y) {
            if (tk[(size_t) x].t != tk[(size_t) y].t) return tk[(size_t) x].t < tk[(size_t) y].t;
            return x < y;
        });
    }
}

}  // namespace

void build_teams(const PanelHost &p, int nrow, const int *rowptr, const int *colidx, TeamHost *out, int T, bool balanced, TeamSeed *seed)
{
    if (T != 8) T = 4;
    out->T = T;
    const int np = p.npanel;
    PhaseClock clk;
    Lattice la;
    la.R = p.R;
    la.st = out->st = T / 4;
    const bool lattice_found = (np >= 64) && detect_stride_lattice(nrow, rowptr, colidx, p.R, &la.D1, &la.D2, &la.M);
    clk.lap("build_teams: lattice detection");

    const std::vector<int> rcount = real_entry_counts(p);
    const Grouping gr = group_panels(p, rcount, T, lattice_found, la, seed);
    out->lattice = gr.lattice;
    out->clustered = gr.clustered;
    if (gr.clustered) out->plocal = gr.slot_of;
    clk.lap(gr.seeded ? "build_teams: panel clustering (from the seed)" : "build_teams: panel clustering (+ lattice choice)");

    const std::vector<TeamKey> tk = form_teams(np, T, gr, la, &out->tpanel);
    const int nteam = out->nteam = (int) tk.size();
    out->lat_key.clear();
    if (gr.lattice)
    {
        out->lat_key.resize((size_t) nteam * 3);
        for (int g = 0; g < nteam; g++) { out->lat_key[(size_t) g * 3] = tk[(size_t) g].a; out->lat_key[(size_t) g * 3 + 1] = tk[(size_t) g].b; out->lat_key[(size_t) g * 3 + 2] = tk[(size_t) g].t; }
    }
    // (Clustered teams without the passes too: their phase key has 128 values for some 440 nodes, the ties the passes would order
    //  are few -- nlpkkt / fem3d / shell stand-ins at n = 128 .. 1024 within 0.1 % either way, profiles/r04_build_time.txt -- and
    //  the passes were 1.3 s of the nlpkkt240-size build.)
    Unions unions;
    merge_unions(p, rcount, out->tpanel, T, nteam, balanced && !gr.clustered, &unions);
    clk.lap("build_teams: union lists + balanced passes");

    layout_unions(unions, T, out);
    value_offsets(unions, T, out);
    clk.lap("build_teams: layout (tcol, tsrc, value streams)");

    // (A recursive bisection of the team graph with generation-wide absolute rounds and a generation start barrier in the kernel
    //  was built and measured in round 3 -- profiles/r03_schedule_matrix.txt: the bytes fetched beyond L2 fall as the L2 model
    //  predicts, nlpkkt stand-in 10.3 -> 7.9 GB, but the slots that wait for their generation cost more time than the bytes
    //  save, +13 % / +33 %; without the barrier the alignment is gone within a few generations -- and removed in round 4.)
    if (gr.seeded && seed->torder.size() == (size_t) nteam) out->torder = seed->torder;
    else
    {
        out->torder.resize((size_t) nteam);
        for (int g = 0; g < nteam; g++) out->torder[(size_t) g] = g;
        if (gr.clustered && nteam >= 128) super_team_order(unions, nteam, &out->torder);
        if (gr.lattice) lattice_strip_order(tk, &out->torder);
    }
    if (seed != nullptr && !gr.seeded) { seed->torder = out->torder; seed->valid = true; }
    clk.lap(gr.seeded ? "build_teams: processing order (from the seed)" : "build_teams: processing order (super-teams)");
    release_pools(unions.pools);
}

}  // namespace crp
