// team2r_format.cpp -- the streams of the row-owner team kernel (panel_format.h, Team2RHost; csrc/team2r_kernel.hip): the rounds
// of every team, the launch grid, records, value / offset blocks with their headers, and the entry table.  build_team2r() at the
// end of the file is the list of the stages.
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include "panel_format.h"
#include "team_stages.h"
#include "par.h"

namespace crp {

namespace {

constexpr int W = 8, T = 8;
constexpr int RD = TEAM2R_ROWDMA;

// what the lane grouping G fixes: slots of a round, bytes of a slot, slots a wave fetches
struct Shape
{
    int S, SLOTB, PERW;
    explicit Shape(int G) : S(8 * G * RD), SLOTB(1024 / G), PERW(G * RD) {}
};

struct ItemR { unsigned char slot; int src; };                            // a panel entry of a wave placed on a slot of the round
struct TeamOutR
{
    int nr = 0, anycol = 0;
    size_t ocol = 0, oiptr = 0, oitem = 0, olp = 0;     // where the team's arrays start in its pool
    long long wunits[8] = {0, 0, 0, 0, 0, 0, 0, 0}, steps = 0, filled = 0;   // 16-byte units of every wave's stream, padded steps, filled slots
    const int *col = nullptr;             // nr * S (TEAM2_NOCOL = empty)
    const int *iptr = nullptr;            // (nr * W) + 1: items of (round, wave)
    const ItemR *items = nullptr;
    const unsigned char *lp = nullptr;    // nr * W: padded steps
};
// (pools of consecutive teams instead of four vectors per team: see build_team2)
struct RoundPoolR { big_vector<int> col, iptr; big_vector<ItemR> items; big_vector<unsigned char> lp; };
// scratch of a builder thread: the rounds of the team being built, and the items of every wave of the round being filled
struct TeamScratchR
{
    std::vector<int> col, iptr;
    std::vector<ItemR> items;
    std::vector<unsigned char> lp;
    std::vector<std::vector<ItemR>> wl = std::vector<std::vector<ItemR>>((size_t) W);
};

// Round scheduler of one team: `nodes` in the order they are to be met; <= S slots per round, look-ahead 3 S nodes, and a round is
// closed before a row of a panel would pass TEAM2R_LCAP steps.  -> the team's rounds in tv, their number in to.nr
// (dealing the ordered entries out to the rounds like cards, so that the waves of a round have equal steps -- mean / max
//  0.59 -> 0.86 -- was 15 % slower: consecutive columns in a round are consecutive B rows in time for every team of the XCD)
void schedule_team_r(const PanelHost &p, const TeamHost &th, const std::vector<int> &nodes, int S, TeamScratchR &tv, TeamOutR &to)
{
    tv.col.clear(); tv.iptr.clear(); tv.items.clear(); tv.lp.clear();
    to.anycol = nodes.empty() ? 0 : th.tcol[(size_t) nodes[0]];
    tv.iptr.push_back(0);
    const size_t nn = nodes.size();
    std::vector<char> taken(nn, 0);
    size_t head = 0, left = nn;
    while (left > 0)
    {
        int cnt[W][8];
        for (int w = 0; w < W; w++)
            for (int r = 0; r < 8; r++) cnt[w][r] = 0;
        for (int w = 0; w < W; w++) tv.wl[(size_t) w].clear();
        int nslot = 0;
        const size_t base_col = tv.col.size();
        tv.col.resize(base_col + (size_t) S, TEAM2_NOCOL);
        while (head < nn && taken[head]) head++;
        int seen = 0;
        for (size_t t = head; t < nn && nslot < S && seen < 3 * S; t++)
        {
            if (taken[t]) continue;
            seen++;
            const int q = nodes[t];
            bool fits = true;
            for (int w = 0; w < W && fits; w++)
            {
                const int src = th.tsrc[(size_t) q * T + (size_t) w];
                if (src < 0) continue;
                const unsigned mk = entry_mask(p, (size_t) src);
                for (int r = 0; r < 8; r++)
                    if (((mk >> r) & 1) && cnt[w][r] + 1 > TEAM2R_LCAP) fits = false;
            }
            if (!fits) continue;
            for (int w = 0; w < W; w++)
            {
                const int src = th.tsrc[(size_t) q * T + (size_t) w];
                if (src < 0) continue;
                const unsigned mk = entry_mask(p, (size_t) src);
                for (int r = 0; r < 8; r++) cnt[w][r] += (mk >> r) & 1;
                ItemR it;
                it.slot = (unsigned char) nslot;
                it.src = src;
                tv.wl[(size_t) w].push_back(it);
            }
            tv.col[base_col + (size_t) nslot] = th.tcol[(size_t) q];
            nslot++;
            taken[t] = 1;
            left--;
        }
        if (nslot == 0) { fprintf(stderr, "[FATAL] team2r scheduler: a round placed nothing\n"); abort(); }
        for (int w = 0; w < W; w++)
        {
            int mx = 0;
            for (int r = 0; r < 8; r++) mx = std::max(mx, cnt[w][r]);
            tv.lp.push_back((unsigned char) ((mx + 1) / 2 * 2));           // steps come in pairs (the kernel's half chunk)
            tv.items.insert(tv.items.end(), tv.wl[(size_t) w].begin(), tv.wl[(size_t) w].end());
            tv.iptr.push_back((int) tv.items.size());
        }
        to.nr++;
    }
    if (to.nr == 0)                                                   // no nonzero in 64 rows: one empty round (the kernel's pipeline wants one)
    {
        tv.col.assign((size_t) S, TEAM2_NOCOL);
        for (int w = 0; w < W; w++)
        {
            tv.lp.push_back(0);
            tv.iptr.push_back(0);
        }
        to.nr = 1;
    }
}

// the team's rounds join its pool
void append_to_pool(const TeamScratchR &tv, RoundPoolR &pool, TeamOutR &to)
{
    to.ocol = pool.col.size(); to.oiptr = pool.iptr.size(); to.oitem = pool.items.size(); to.olp = pool.lp.size();
    pool.col.insert(pool.col.end(), tv.col.begin(), tv.col.end());
    pool.iptr.insert(pool.iptr.end(), tv.iptr.begin(), tv.iptr.end());
    pool.items.insert(pool.items.end(), tv.items.begin(), tv.items.end());
    pool.lp.insert(pool.lp.end(), tv.lp.begin(), tv.lp.end());
}

// the pool's arrays have stopped growing: the team's pointers into them, the units of its streams, its steps and filled slots
void bind_and_measure(const RoundPoolR &pool, int S, TeamOutR &to)
{
    to.col = pool.col.data() + to.ocol; to.iptr = pool.iptr.data() + to.oiptr; to.items = pool.items.data() + to.oitem; to.lp = pool.lp.data() + to.olp;
    for (int w = 0; w < W; w++)
        for (int r = 0; r < to.nr; r++)
        {
            to.wunits[w] += 5LL * to.lp[(size_t) r * W + (size_t) w] + 4;   // 80 Lp bytes of values and offsets + the 64-byte header
            to.steps += to.lp[(size_t) r * W + (size_t) w];
        }
    for (size_t i = 0; i < (size_t) to.nr * (size_t) S; i++) to.filled += to.col[i] != TEAM2_NOCOL;
}

// ---- stage: the rounds of every team, pool by pool -- its union in the order of key(), round scheduler
template <typename KeyFn>
void schedule_rounds_r(const PanelHost &p, const TeamHost &th, KeyFn key, int S, int rpool, std::vector<RoundPoolR> &rpools, std::vector<TeamOutR> &res)
{
    const int nteam = th.nteam;
    parallel_chunks((long long) rpools.size(), 1, [&](long long pb, long long pe, int) {
        std::vector<int> nodes;
        std::vector<std::pair<long long, int>> keyed;
        TeamScratchR tv;
        for (long long pl = pb; pl < pe; pl++)
        {
            RoundPoolR &pool = rpools[(size_t) pl];
            const long long b = pl * rpool, e = std::min<long long>(nteam, b + rpool);
            for (long long g = b; g < e; g++)
            {
                team_union_nodes(th, (int) g, nodes);
                sort_nodes_by_key(nodes, keyed, key);
                schedule_team_r(p, th, nodes, S, tv, res[(size_t) g]);
                append_to_pool(tv, pool, res[(size_t) g]);
            }
            for (long long g = b; g < e; g++) bind_and_measure(pool, S, res[(size_t) g]);
        }
    });
}

// ---- stage: layout -- tinfo (rounds, first record), the first 16-byte unit of every wave's stream (tvoff) and the totals.
// false: the streams would pass what their 32-bit offsets address
bool layout_streams_r(const std::vector<TeamOutR> &res, Team2RHost *out)
{
    const int nteam = out->nteam;
    out->tinfo.assign((size_t) nteam * 2, 0);
    out->tvoff.assign((size_t) nteam * W + 1, 0);
    long long rec0 = 0, run = 0;                                              // run: units of 16 bytes
    out->rounds = out->steps = out->nnz = out->slots_filled = 0;
    for (int g = 0; g < nteam; g++)
    {
        const TeamOutR &to = res[(size_t) g];
        out->tinfo[(size_t) g * 2] = to.nr;
        out->tinfo[(size_t) g * 2 + 1] = (int) rec0;
        rec0 += to.nr;
        out->rounds += to.nr;
        for (int w = 0; w < W; w++)
        {
            out->tvoff[(size_t) g * W + (size_t) w] = run;
            run += to.wunits[w];
        }
        out->steps += to.steps;
        out->slots_filled += to.filled;
    }
    out->tvoff[(size_t) nteam * W] = run;
    out->nwords = run * 2;
    return !(rec0 >= (1LL << 31) / 128 || run >= (1LL << 31));
}

// ---- stage: records, value / offset blocks and headers of wave w of team g (layout: panel_format.h); slot_of = the 8-byte word of
// tval where every (entry, row) pair of the panel format went
struct StreamWriterR
{
    const PanelHost &p;
    Team2RHost *out;
    Shape sh;
    big_vector<uint32_t> &slot_of;
    bool with_vals;

    uint32_t *record(int g, int r, int w) const { return &out->trec[((size_t) out->tinfo[(size_t) g * 2 + 1] + (size_t) r) * 128 + (size_t) w * 16]; }

    void wave(const TeamOutR &to, int g, int w) const
    {
        const int ZERO = team2r_zero(RD);
        long long at16 = 0;                                           // units of 16 bytes inside the wave's stream
        const long long w0 = out->tvoff[(size_t) g * W + (size_t) w] * 2;   // first 8-byte word of the stream
        for (int r = 0; r < to.nr; r++)
        {
            uint32_t *rec = record(g, r, w);
            const int Lp = to.lp[(size_t) r * W + (size_t) w];
            rec[0] = (uint32_t) Lp;
            rec[1] = (uint32_t) at16;
            for (int j = 0; j < sh.PERW; j++)
            {
                const int c = to.col[(size_t) r * sh.S + (size_t) (w * sh.PERW + j)];
                rec[2 + j] = (uint32_t) (c != TEAM2_NOCOL ? c : to.anycol);
            }
            double *vals = &out->tval[(size_t) (w0 + at16 * 2)];                         // [8][Lp]
            uint16_t *offs = reinterpret_cast<uint16_t *>(vals + (size_t) 8 * Lp);       // [8][Lp]
            for (int i = 0; i < 8 * Lp; i++) offs[i] = (uint16_t) ZERO;
            int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = to.iptr[(size_t) r * W + (size_t) w]; i < to.iptr[(size_t) r * W + (size_t) w + 1]; i++)
            {
                const ItemR &it = to.items[(size_t) i];
                const unsigned mk = entry_mask(p, (size_t) it.src);
                for (int rr = 0; rr < 8; rr++)
                    if ((mk >> rr) & 1)
                    {
                        const int st = fill[rr]++;
                        if (with_vals) vals[(size_t) rr * Lp + (size_t) st] = p.pval[(size_t) it.src * 8 + (size_t) rr];
                        offs[(size_t) rr * Lp + (size_t) st] = (uint16_t) (it.slot * sh.SLOTB);
                        slot_of[(size_t) it.src * 8 + (size_t) rr] = (uint32_t) (w0 + at16 * 2 + (long long) rr * Lp + st);
                    }
            }
            at16 += 5LL * Lp + 4;
        }
        // headers: the record of round r + 2 behind the block of round r
        for (int r = 0; r + 2 < to.nr; r++)
        {
            const uint32_t *rec = record(g, r, w);
            const uint32_t *rec2 = rec + 2 * 128;
            uint32_t *hdr = reinterpret_cast<uint32_t *>(&out->tval[(size_t) (w0 + (long long) rec[1] * 2 + 10LL * rec[0])]);
            for (int i = 0; i < 16; i++) hdr[i] = rec2[i];
        }
    }
};

// ---- stage: the entry table -- what a workgroup needs when it turns to an entry of the launch grid
void build_entry_table(Team2RHost *out)
{
    parallel_fill(out->tent, out->tgrid.size() * 256, 0u);
    parallel_chunks((long long) out->tgrid.size(), 256, [&](long long b, long long e, int) {
        for (long long en = b; en < e; en++)
        {
            const int g = out->tgrid[(size_t) en];
            if (g < 0) continue;
            const int nr = out->tinfo[(size_t) g * 2];
            for (int w = 0; w < W; w++)
            {
                uint32_t *t = &out->tent[((size_t) en * 8 + (size_t) w) * 32];
                const uint32_t *rec = &out->trec[(size_t) out->tinfo[(size_t) g * 2 + 1] * 128 + (size_t) w * 16];
                const long long vo = out->tvoff[(size_t) g * W + (size_t) w];
                t[0] = (uint32_t) nr;
                t[1] = (uint32_t) out->tpanel[(size_t) g * W + (size_t) w];
                t[2] = (uint32_t) (vo & 0xFFFFFFFFLL);
                t[3] = (uint32_t) (vo >> 32);
                for (int i = 0; i < 10; i++) t[4 + i] = rec[i];
                if (nr > 1)
                    for (int i = 0; i < 10; i++) t[14 + i] = rec[128 + i];
                for (int i = 0; i < 8; i++) t[24 + i] = 0xFFFFFFFFu;
            }
        }
    });
}

}  // namespace

bool build_team2r(const PanelHost &p, int nrow, const int *rowptr, const int *colidx, Team2RHost *out, const int *colpos, TeamSeed *seed)
{
    const int G = out->G == 2 ? 2 : 4;
    out->G = G;
    const Shape sh(G);
    PhaseClock clk;
    released_async<TeamHost> th_owner;
    TeamHost &th = *th_owner;
    // (teams as team2 builds them, KKT systems' primal + dual mixes included: the B rows both kinds share are fetched once --
    //  teams of one kind of panel give the waves of a round more equal steps (useful / issued row slots 0.53 against 0.32) and are
    //  slower all the same: nlpkkt stand-in n = 32 0.533 against 0.500 ms, at nlpkkt240 size 8.96 against 7.83, where the kernel is
    //  bound by what it fetches from beyond L2)
    const bool with_vals = team_prelude(p, nrow, rowptr, colidx, false, seed, &th, out);
    clk.lap("build_team2r: build_teams total");
    const int nteam = th.nteam;
    // Order of a team's union entries over its rounds.  team2 sorts by a PHASE (position mod 8 first) so that its parts are
    // contiguous row ranges; here a round should give every row of a panel about the same number of nonzeros (a wave's steps are
    // the maximum over its 8 rows): the natural order of the columns does that -- a run of consecutive columns is one mesh line,
    // which the 8 consecutive rows of a panel touch alike -- where the phase order gives a round the columns that only one or two
    // of the 8 rows have (nlpkkt stand-in: 2.7 padded steps per nonzero against 1.3 with this order).
    auto key = [&](int q) -> long long {
        const int c = th.tcol[(size_t) q];
        return c >= 0 ? (long long) (colpos ? colpos[c] : c) : (1LL << 40) + (long long) (~c);
    };
    const int rpool = teams_per_pool(nteam, 32);
    std::vector<RoundPoolR> rpools((size_t) ((nteam + rpool - 1) / rpool));
    std::vector<TeamOutR> res((size_t) nteam);
    schedule_rounds_r(p, th, key, sh.S, rpool, rpools, res);
    clk.lap("build_team2r: rounds");
    if (!layout_streams_r(res, out)) return false;                        // (the caller falls back to the row-panel kernels)
    int cut[9];
    xcd_cuts(out->torder, [&](int g) { return res[(size_t) g].nr + 1; }, cut);
    build_tgrid(cut, out->torder, &out->tgrid);
    parallel_fill(out->trec, (size_t) (out->rounds + 1) * 128, 0u);
    parallel_fill(out->tval, (size_t) out->nwords + 512, 0.0);
    big_vector<uint32_t> slot_of;
    slot_of.resize(p.pcol.size() * 8);
    const StreamWriterR writer{p, out, sh, slot_of, with_vals};
    parallel_chunks(nteam, 32, [&](long long b, long long e, int) {
        for (long long g = b; g < e; g++)
            for (int w = 0; w < W; w++) writer.wave(res[(size_t) g], (int) g, w);
    });
    build_entry_table(out);
    clk.lap("build_team2r: records, streams, entry table");
    out->nnz = (long long) p.pmap.size();
    build_vmap(p, slot_of, &out->vmap);
    clk.lap("build_team2r: value-update map");
    release_pools(rpools);
    clk.lap("build_team2r: release");
    return true;
}

}  // namespace crp
