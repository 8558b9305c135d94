// team_stages.h -- internal to the format builders (panel_format.cpp, team_format.cpp, team2_format.cpp, team2r_format.cpp): the
// stages that the builders of the team formats share, each written once.  Templates and inlines only, no state.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "panel_format.h"
#include "par.h"

namespace crp {

// ordering key of a two-source column index: receive-buffer rows (c < 0, ~c ascending)
// first, then local rows ascending.  With one rank this is plain column order, i.e. the
// CSR order of the reference.
inline uint32_t col_key(int c) { return c < 0 ? (uint32_t) (~c) : ((uint32_t) c | 0x80000000u); }

// row mask of entry q of the panel format (byte q & 3 of word q / 4)
inline uint32_t entry_mask(const PanelHost &p, size_t q) { return (p.pmask4[q >> 2] >> (8 * (q & 3))) & 0xFFu; }

// ---- the common prelude of build_team2 / build_team2r: the teams (from the seed when it holds them), what the format copies of
// them, and whether the panels came with values (structure-only panels: the caller scatters the values through vmap).  *th stays
// with its owner, a released_async of the caller.
template <typename Out>
bool team_prelude(const PanelHost &p, int nrow, const int *rowptr, const int *colidx, bool balanced, TeamSeed *seed, TeamHost *th, Out *out)
{
    build_teams(p, nrow, rowptr, colidx, th, TEAM2_T, balanced, seed);
    out->nteam = th->nteam;
    out->lattice = th->lattice;
    out->tpanel = th->tpanel;
    out->torder = th->torder;
    return !p.pval.empty() || p.pcol.empty();
}

// ---- the real union entries of team g (tsrc has a user: not padding), ascending
inline void team_union_nodes(const TeamHost &th, int g, std::vector<int> &nodes)
{
    const int T = th.T;
    nodes.clear();
    for (int q = th.tptr[(size_t) g]; q < th.tptr[(size_t) g + 1]; q++)
    {
        bool used = false;
        for (int w = 0; w < T; w++) used = used || th.tsrc[(size_t) q * T + (size_t) w] >= 0;
        if (used) nodes.push_back(q);
    }
}

// ... and their stable order by key(node): (key, node) pairs are sorted -- the key is looked up once per node, not per comparison;
// nodes come in ascending order, so ties keep it, as a stable sort by key would.  `keyed` is scratch of the builder thread.
template <typename K, typename KeyFn>
void sort_nodes_by_key(std::vector<int> &nodes, std::vector<std::pair<K, int>> &keyed, KeyFn key)
{
    keyed.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); i++) keyed[i] = {key(nodes[i]), nodes[i]};
    std::sort(keyed.begin(), keyed.end());
    for (size_t i = 0; i < nodes.size(); i++) nodes[i] = keyed[i].second;
}

// ---- the launch grid: the order cut into 8 contiguous pieces of equal work, one per XCD -- pieces of equal team COUNT leave XCDs
// idle when the teams differ (KKT systems: 27-point primal rows, short dual rows).  work(g) = what team g costs.
template <typename WorkFn>
void xcd_cuts(const std::vector<int> &torder, WorkFn work, int cut[9])
{
    const int nteam = (int) torder.size();
    for (int q = 0; q <= 8; q++) cut[q] = nteam;
    long long total = 0;
    for (int g = 0; g < nteam; g++) total += work(g);
    cut[0] = 0;
    long long acc = 0;
    int x = 1;
    for (int i = 0; i < nteam && x < 8; i++)
    {
        acc += work(torder[(size_t) i]);
        while (x < 8 && acc * 8 >= total * x) cut[x++] = i + 1;
    }
}

// run x of tgrid = what XCD x processes, in order (-1 = no team)
inline void build_tgrid(const int cut[9], const std::vector<int> &torder, std::vector<int> *tgrid)
{
    int cpx = 1;
    for (int q = 0; q < 8; q++) cpx = std::max(cpx, cut[q + 1] - cut[q]);
    tgrid->assign((size_t) cpx * 8, -1);
    for (int q = 0; q < 8; q++)
        for (int i = cut[q]; i < cut[q + 1]; i++) (*tgrid)[(size_t) q * cpx + (size_t) (i - cut[q])] = torder[(size_t) i];
}

// ---- vmap through the panel format's slot map: pmap[nz] = q * 8 + row of the panel format, slot_of = where that (entry, row)
// pair went in the format's value stream
inline void build_vmap(const PanelHost &p, const big_vector<uint32_t> &slot_of, std::vector<uint32_t> *vmap)
{
    vmap->resize(p.pmap.size());
    parallel_chunks((long long) p.pmap.size(), 1 << 18, [&](long long b, long long e, int) {
        for (long long nz = b; nz < e; nz++) (*vmap)[(size_t) nz] = slot_of[(size_t) p.pmap[(size_t) nz]];
    });
}

// ---- pools: the unions (floor 64) and the rounds (floor 32) of this many consecutive teams share their arrays -- one vector of
// each kind per TEAM was 1.3 M small allocations on the nlpkkt240-size matrix, whose fresh 4 KiB pages were faulted in no faster by
// 16 threads than by 4.
inline int teams_per_pool(int nteam, int floor)
{
    return (int) std::min<long long>(2048, std::max<long long>(floor, nteam / (4LL * host_threads())));
}

// (released by all threads, not by the one that leaves the function)
template <typename Pool>
void release_pools(std::vector<Pool> &pools)
{
    parallel_chunks((long long) pools.size(), 1, [&](long long b, long long e, int) {
        for (long long pl = b; pl < e; pl++)
        {
            Pool freed;
            std::swap(freed, pools[(size_t) pl]);
        }
    });
}

}  // namespace crp
