// team2_format.cpp -- the streams of the LDS-sharing team kernel (panel_format.h, Team2Host; csrc/team2_kernel.hip): the rounds of
// every team (phase order, list scheduler, balance pass), the launch grid, record blocks and value streams.  build_team2() at the
// end of the file is the list of the stages.
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include "panel_format.h"
#include "team_order.h"
#include "team_stages.h"
#include "knobs.h"
#include "par.h"

namespace crp {

namespace {

constexpr int D = TEAM2_D, CAP = TEAM2_CAP, T = TEAM2_T, W = TEAM2_T;   // panels of a team = waves = slots of a round
constexpr int sbits = 3, fbase = 16;                                    // slot bits and first flag bit of record word 0
constexpr size_t blkw = (size_t) 32 * W;                                // words of a record block (8 rounds x W waves x 4)
constexpr int WGS = 64;                                                 // workgroups resident on an XCD = a generation

struct Part { int src; unsigned char slot, first, len; };               // (8 bytes: the parts of the nlpkkt240-size format are 24 M rounds x 32)
struct TeamOut
{
    int nr = 0, filled = 0, nparts = 0;
    int anycol = 0;                             // a column of the team (a valid row for the prologue's empty slots)
    size_t r0 = 0;                              // rounds of the pool in front of this team's
    int *col = nullptr;                         // nr * W slot columns (TEAM2_NOCOL = empty slot)
    // parts of wave w in round r: ownp[(r * W + w) * CAP .. + ownc[r * W + w])  (flat: one small vector per
    // (round, wave) was 126 M heap allocations on the nlpkkt240-size matrix)
    Part *ownp = nullptr;
    unsigned char *ownc = nullptr;
};
// (The rounds of `rpool` consecutive teams share three arrays, like the unions of build_teams: three vectors per team were 1.3 M
//  allocations whose pages no number of threads faulted in faster; col / ownp / ownc of a team point into its pool.)
struct RoundPool
{
    big_vector<int> col; big_vector<Part> ownp; big_vector<unsigned char> ownc;
    void bind(TeamOut &to)
    {
        to.col = col.data() + to.r0 * (size_t) W;
        to.ownp = ownp.data() + to.r0 * (size_t) W * CAP;
        to.ownc = ownc.data() + to.r0 * (size_t) W;
    }
};
struct SchedScratch { std::vector<unsigned char> rk, rr; std::vector<char> taken; };    // (one per builder thread, not one per team)

// contiguous row ranges of a row mask
int row_ranges(unsigned m, Part *dst)
{
    int n = 0;
    for (int r = 0; r < 8;)
    {
        if (!((m >> r) & 1u)) { r++; continue; }
        int l = 1;
        while (r + l < 8 && ((m >> (r + l)) & 1u)) l++;
        dst[n].first = (unsigned char) r; dst[n].len = (unsigned char) l; n++;
        r += l;
    }
    return n;
}

// List scheduler of one team: `nodes` in the order they are to be met; <= W slots per round, <= CAP parts per wave and
// round, look-ahead 4 W nodes.  Empty slots are marked TEAM2_NOCOL here and written to the records as a row of the team
// (a fetch nobody reads).  (Measured and removed: a scheduler that picks by the busiest wave's load, a cap on a wave's
// load per round -- round 3)  The team's rounds are appended to the pool.
void schedule_team(const PanelHost &p, const TeamHost &th, const std::vector<int> &nodes, SchedScratch &scr, RoundPool &pool, TeamOut &to)
{
    to.r0 = pool.ownc.size() / (size_t) W;
    to.anycol = nodes.empty() ? 0 : th.tcol[(size_t) nodes[0]];
    // the row ranges of every (node, wave), once: byte = first << 4 | len, up to 4 per wave (the look-ahead visits a
    // node several times before it fits)
    const size_t nn = nodes.size();
    std::vector<unsigned char> &rk = scr.rk, &rr = scr.rr;
    rk.assign(nn * (size_t) T, 0);
    rr.resize(nn * (size_t) T * 4);                                    // (read only where rk says an entry exists)
    for (size_t t = 0; t < nn; t++)
        for (int w = 0; w < T; w++)
        {
            const int src = th.tsrc[(size_t) nodes[t] * T + (size_t) w];
            if (src < 0) continue;
            Part tmp[4];
            const int kk = row_ranges(entry_mask(p, (size_t) src), tmp);
            rk[t * (size_t) T + (size_t) w] = (unsigned char) kk;
            for (int i = 0; i < kk; i++) rr[(t * (size_t) T + (size_t) w) * 4 + (size_t) i] = (unsigned char) (tmp[i].first << 4 | tmp[i].len);
        }
    std::vector<char> &taken = scr.taken;
    taken.assign(nn, 0);
    size_t head = 0, left = nn;
    while (left > 0)
    {
        int cnt[W];
        for (int w = 0; w < W; w++) cnt[w] = 0;
        int nslot = 0;
        const size_t base_col = (to.r0 + (size_t) to.nr) * (size_t) W;
        pool.col.resize(base_col + (size_t) W, TEAM2_NOCOL);
        pool.ownp.resize((base_col + (size_t) W) * CAP);
        pool.ownc.resize(base_col + (size_t) W, 0);
        while (head < nn && taken[head]) head++;
        int seen = 0;
        for (size_t t = head; t < nn && nslot < W && seen < 4 * W; t++)
        {
            if (taken[t]) continue;
            seen++;
            const unsigned char *kk = &rk[t * (size_t) T];
            bool fits = true;
            for (int w = 0; w < W; w++)
                if (cnt[w] + kk[w] > CAP) fits = false;
            if (!fits) continue;
            const int q = nodes[t];
            for (int w = 0; w < W; w++)
                for (int i = 0; i < kk[w]; i++)
                {
                    const unsigned char b = rr[(t * (size_t) T + (size_t) w) * 4 + (size_t) i];
                    Part pt;
                    pt.first = (unsigned char) (b >> 4);
                    pt.len = (unsigned char) (b & 15);
                    pt.slot = (unsigned char) nslot;
                    pt.src = th.tsrc[(size_t) q * T + (size_t) w];
                    pool.ownp[(base_col + (size_t) w) * CAP + (size_t) cnt[w]] = pt;
                    pool.ownc[base_col + (size_t) w]++;
                    cnt[w]++;
                    to.nparts++;
                }
            pool.col[base_col + (size_t) nslot] = th.tcol[(size_t) q];
            nslot++;
            taken[t] = 1;
            left--;
        }
        if (nslot == 0)
        {
            // (cannot happen: the first open node of an empty round always fits -- a panel has at most 4 row ranges)
            fprintf(stderr, "[FATAL] team2 scheduler: a round placed nothing\n");
            abort();
        }
        to.filled += nslot;
        to.nr++;
    }
}

// Balance pass over a team's finished rounds: a round lasts as long as its busiest wave (one barrier per round), so for
// every pair of consecutive rounds the exchange of one slot of each that lowers (busiest wave of r) + (busiest wave of
// r + 1) most is made -- rounds stay full (an empty slot is a fetch), a node moves by one round at most per pass (the phase
// order it was placed by has that much slack).  Work of a part = 3 + its rows.
void balance_rounds(TeamOut &to)
{
    const int nr = to.nr;
    if (nr < 2) return;
    // work[(r * W + slot) * W + w], count likewise: what slot `slot` of round r gives wave w
    std::vector<unsigned char> swork((size_t) nr * W * W, 0), scnt((size_t) nr * W * W, 0);
    std::vector<int> load((size_t) nr * W, 0), cnt((size_t) nr * W, 0);
    for (int r = 0; r < nr; r++)
        for (int w = 0; w < W; w++)
        {
            const Part *ow = &to.ownp[((size_t) r * W + (size_t) w) * CAP];
            const int c = to.ownc[(size_t) r * W + (size_t) w];
            cnt[(size_t) r * W + (size_t) w] = c;
            for (int i = 0; i < c; i++)
            {
                swork[((size_t) r * W + (size_t) ow[i].slot) * W + (size_t) w] += (unsigned char) (3 + ow[i].len);
                scnt[((size_t) r * W + (size_t) ow[i].slot) * W + (size_t) w]++;
                load[(size_t) r * W + (size_t) w] += 3 + ow[i].len;
            }
        }
    auto maxload = [&](int r) { int m = 0; for (int w = 0; w < W; w++) m = std::max(m, load[(size_t) r * W + (size_t) w]); return m; };
    for (int pass = 0; pass < 2; pass++)
        for (int r = 0; r + 1 < nr; r++)
        {
            const int cur = maxload(r) + maxload(r + 1);
            int best = cur, bi = -1, bj = -1;
            for (int i = 0; i < W; i++)
            {
                if (to.col[(size_t) r * W + (size_t) i] == TEAM2_NOCOL) continue;
                const unsigned char *wa = &swork[((size_t) r * W + (size_t) i) * W], *ca = &scnt[((size_t) r * W + (size_t) i) * W];
                for (int j = 0; j < W; j++)
                {
                    if (to.col[(size_t) (r + 1) * W + (size_t) j] == TEAM2_NOCOL) continue;
                    const unsigned char *wb = &swork[((size_t) (r + 1) * W + (size_t) j) * W], *cb = &scnt[((size_t) (r + 1) * W + (size_t) j) * W];
                    int m0 = 0, m1 = 0;
                    bool ok = true;
                    for (int w = 0; w < W; w++)
                    {
                        if (cnt[(size_t) r * W + (size_t) w] - ca[w] + cb[w] > CAP || cnt[(size_t) (r + 1) * W + (size_t) w] - cb[w] + ca[w] > CAP) { ok = false; break; }
                        m0 = std::max(m0, load[(size_t) r * W + (size_t) w] - wa[w] + wb[w]);
                        m1 = std::max(m1, load[(size_t) (r + 1) * W + (size_t) w] - wb[w] + wa[w]);
                    }
                    if (ok && m0 + m1 < best) { best = m0 + m1; bi = i; bj = j; }
                }
            }
            if (bi < 0) continue;
            // exchange slot bi of round r with slot bj of round r + 1
            std::swap(to.col[(size_t) r * W + (size_t) bi], to.col[(size_t) (r + 1) * W + (size_t) bj]);
            for (int w = 0; w < W; w++)
            {
                Part *p0 = &to.ownp[((size_t) r * W + (size_t) w) * CAP], *p1 = &to.ownp[((size_t) (r + 1) * W + (size_t) w) * CAP];
                Part keep0[4], keep1[4], mv0[4], mv1[4];
                int k0 = 0, k1 = 0, n0 = 0, n1 = 0;
                for (int i = 0; i < (int) to.ownc[(size_t) r * W + (size_t) w]; i++) { if (p0[i].slot == bi) mv0[n0++] = p0[i]; else keep0[k0++] = p0[i]; }
                for (int i = 0; i < (int) to.ownc[(size_t) (r + 1) * W + (size_t) w]; i++) { if (p1[i].slot == bj) mv1[n1++] = p1[i]; else keep1[k1++] = p1[i]; }
                for (int i = 0; i < n1; i++) { mv1[i].slot = (unsigned char) bi; keep0[k0++] = mv1[i]; }
                for (int i = 0; i < n0; i++) { mv0[i].slot = (unsigned char) bj; keep1[k1++] = mv0[i]; }
                for (int i = 0; i < k0; i++) p0[i] = keep0[i];
                for (int i = 0; i < k1; i++) p1[i] = keep1[i];
                to.ownc[(size_t) r * W + (size_t) w] = (unsigned char) k0;
                to.ownc[(size_t) (r + 1) * W + (size_t) w] = (unsigned char) k1;
                const int wa = swork[((size_t) r * W + (size_t) bi) * W + (size_t) w], wb = swork[((size_t) (r + 1) * W + (size_t) bj) * W + (size_t) w];
                const int ca = scnt[((size_t) r * W + (size_t) bi) * W + (size_t) w], cb = scnt[((size_t) (r + 1) * W + (size_t) bj) * W + (size_t) w];
                load[(size_t) r * W + (size_t) w] += wb - wa;
                load[(size_t) (r + 1) * W + (size_t) w] += wa - wb;
                cnt[(size_t) r * W + (size_t) w] += cb - ca;
                cnt[(size_t) (r + 1) * W + (size_t) w] += ca - cb;
                std::swap(swork[((size_t) r * W + (size_t) bi) * W + (size_t) w], swork[((size_t) (r + 1) * W + (size_t) bj) * W + (size_t) w]);
                std::swap(scnt[((size_t) r * W + (size_t) bi) * W + (size_t) w], scnt[((size_t) (r + 1) * W + (size_t) bj) * W + (size_t) w]);
            }
        }
}

// ---- stage: union nodes per team (the work measure of the launch grid and of the pools' reserve)
std::vector<int> count_team_nodes(const TeamHost &th)
{
    std::vector<int> nn((size_t) th.nteam, 0);
    parallel_chunks(th.nteam, 256, [&](long long b, long long e, int) {
        std::vector<int> nodes;
        for (long long g = b; g < e; g++) { team_union_nodes(th, (int) g, nodes); nn[(size_t) g] = (int) nodes.size(); }
    });
    return nn;
}

// ---- stage: the rounds of every team, pool by pool -- its union in the order of the phase key, list scheduler, balance pass
// (off beyond 120 k teams: it costs 2 s per 100 k teams on 16 CPUs)
template <typename KeyFn>
void schedule_rounds(const PanelHost &p, const TeamHost &th, const std::vector<int> &nn, KeyFn key, int rpool, std::vector<RoundPool> &rpools, std::vector<TeamOut> &res)
{
    const int nteam = th.nteam;
    const bool swap_on = nteam <= 120000;
    parallel_chunks((long long) rpools.size(), 1, [&](long long pb, long long pe, int) {
        std::vector<int> nodes;
        std::vector<std::pair<int, int>> keyed;
        SchedScratch scr;
        for (long long pl = pb; pl < pe; pl++)
        {
            RoundPool &pool = rpools[(size_t) pl];
            const long long b = pl * rpool, e = std::min<long long>(nteam, b + rpool);
            size_t est = 0;                                 // rounds: an eighth of the nodes, a quarter more for rounds left partly empty
            for (long long g = b; g < e; g++) est += (size_t) nn[(size_t) g] / (size_t) W + (size_t) nn[(size_t) g] / (size_t) (4 * W) + 2;
            pool.col.reserve(est * (size_t) W);
            pool.ownp.reserve(est * (size_t) W * CAP);
            pool.ownc.reserve(est * (size_t) W);
            for (long long g = b; g < e; g++)
            {
                team_union_nodes(th, (int) g, nodes);
                sort_nodes_by_key(nodes, keyed, key);
                schedule_team(p, th, nodes, scr, pool, res[(size_t) g]);
                if (swap_on) { pool.bind(res[(size_t) g]); balance_rounds(res[(size_t) g]); }
            }
            for (long long g = b; g < e; g++) pool.bind(res[(size_t) g]);          // (the pool's arrays have stopped growing)
        }
    });
}

// ---- stage: lattice teams -- the processing order by search over block orders against an L2 model (team_order.h).
// CRPSPMM_T2_LATORDER=0 keeps the round-2 order (strips of team columns swept along the teeth).  -> the order changed
bool search_lattice_order(const TeamHost &th, const std::vector<TeamOut> &res, bool report, std::vector<int> *torder)
{
    const int nteam = th.nteam;
    std::vector<const int *> cols((size_t) nteam);
    std::vector<int> nrs((size_t) nteam);
    for (int g = 0; g < nteam; g++) { cols[(size_t) g] = res[(size_t) g].col; nrs[(size_t) g] = res[(size_t) g].nr; }
    LatticeOrderInfo li;
    // an XCD's 4 MiB of L2 in row slices of the widest tile (2 KiB); a generation = the workgroups resident on an XCD
    const bool changed = lattice_block_order(nteam, th.lat_key.data(), W, WGS, 2048, TEAM2_NOCOL, cols.data(), nrs.data(), torder, &li);
    if (report)
        fprintf(stderr, "[crpspmm timing] lattice order: %d candidates, model misses %.0f (given) -> %.0f (boxes %d x %d, blocks %d x %d x %d, flags %d)%s\n",
                li.candidates, li.miss_given, li.miss_best, li.pa, li.pb, li.bt, li.ba, li.bb, li.flags, changed ? "" : " -- kept the given order");
    return changed;
}

// values of the block of round r of wave w: its parts' rows (compact) or 8 per part
int round_values(const TeamOut &to, int r, int w, bool compact)
{
    int nv = 0;
    const Part *ow = &to.ownp[((size_t) r * W + (size_t) w) * CAP];
    for (int i = 0; i < (int) to.ownc[(size_t) r * W + (size_t) w]; i++) nv += compact ? ow[i].len : 8;
    return nv;
}

// ---- stage: layout -- tinfo, the first record block of every team (-> blk0), the first value unit of every wave's stream
// (tvoff) and the totals
std::vector<int> layout_streams(const std::vector<TeamOut> &res, Team2Host *out)
{
    const int nteam = out->nteam;
    const bool compact = out->compact;
    out->tinfo.assign((size_t) nteam * 4, 0);
    out->tpro.assign((size_t) nteam * D * W * 2, 0);
    out->tvoff.assign((size_t) nteam * W + 1, 0);
    std::vector<int> blk0((size_t) nteam + 1, 0);
    out->real_entries = out->slots = out->parts = 0;
    // value units (TEAM2_VUNIT values) of every wave's stream: its rounds' blocks, each padded
    std::vector<long long> wunits((size_t) nteam * W, 0);
    parallel_chunks(nteam, 256, [&](long long b, long long e, int) {
        for (long long g = b; g < e; g++)
        {
            const TeamOut &to = res[(size_t) g];
            for (int w = 0; w < W; w++)
            {
                long long u = 0;
                for (int r = 0; r < to.nr; r++) u += (round_values(to, r, w, compact) + TEAM2_VUNIT - 1) / TEAM2_VUNIT;
                wunits[(size_t) g * W + (size_t) w] = u;
            }
        }
    });
    long long run = 0;
    for (int g = 0; g < nteam; g++)
    {
        const TeamOut &to = res[(size_t) g];
        blk0[(size_t) g + 1] = blk0[(size_t) g] + (to.nr + 7) / 8;
        out->tinfo[(size_t) g * 4] = to.nr;
        out->tinfo[(size_t) g * 4 + 1] = blk0[(size_t) g];
        out->tinfo[(size_t) g * 4 + 2] = to.nparts;
        out->tinfo[(size_t) g * 4 + 3] = to.filled;
        out->real_entries += to.filled;
        out->slots += (long long) to.nr * W;
        out->parts += to.nparts;
        for (int w = 0; w < W; w++)
        {
            out->tvoff[(size_t) g * W + (size_t) w] = run;
            run += wunits[(size_t) g * W + (size_t) w];
        }
    }
    out->tvoff[(size_t) nteam * W] = run;
    out->nvalues = run * TEAM2_VUNIT;
    return blk0;
}

// ---- stage: records, prologue and values of wave w of team g (record layout: panel_format.h); slot_of = where every (entry, row)
// pair of the panel format went in tval
struct StreamWriter
{
    const PanelHost &p;
    Team2Host *out;
    const std::vector<int> &blk0;
    big_vector<uint32_t> &slot_of;
    bool with_vals;

    uint32_t *record(int g, int r, int w) const { return &out->trec[((size_t) blk0[(size_t) g] + (size_t) (r >> 3)) * blkw + (size_t) (r & 7) * 4 * W + (size_t) w * 4]; }

    void wave(const TeamOut &to, int g, int w) const
    {
        const bool compact = out->compact;
        // value units of every round of this wave (prefix), then the records
        std::vector<long long> voff((size_t) to.nr + 1, 0);
        std::vector<int> nvals((size_t) to.nr + 1, 0);
        for (int r = 0; r < to.nr; r++)
        {
            nvals[(size_t) r] = round_values(to, r, w, compact);
            voff[(size_t) r + 1] = voff[(size_t) r] + (nvals[(size_t) r] + TEAM2_VUNIT - 1) / TEAM2_VUNIT;
        }
        if (voff[(size_t) to.nr] >= (1LL << 20)) { fprintf(stderr, "[FATAL] team2 format: a wave's value stream exceeds 2^20 units\n"); abort(); }
        const long long e0 = out->tvoff[(size_t) g * W + (size_t) w] * TEAM2_VUNIT;     // first value of the wave's stream
        for (int r = 0; r < to.nr; r++)
        {
            const Part *ow = &to.ownp[((size_t) r * W + (size_t) w) * CAP];
            const size_t nown = to.ownc[(size_t) r * W + (size_t) w];
            uint32_t x = (uint32_t) nown, y = 0, z = 0;
            long long e = e0 + voff[(size_t) r] * TEAM2_VUNIT;       // where the round's block starts
            int prefix = 0;
            for (size_t i = 0; i < nown; i++)
            {
                const Part &pt = ow[i];
                x |= (uint32_t) pt.slot << (4 + sbits * (int) i);
                y |= (uint32_t) (pt.first * 8 + pt.len - 1) << (6 * i);
                // value position of the part: prefix + 7 - first (tools/gen_team2_asm.py); full groups: the part's 8
                // values start at 8 i, row r at 8 i + r, i.e. "prefix" = 8 i + first
                if (!compact) prefix = 8 * (int) i + pt.first;
                const uint32_t pos = (uint32_t) (prefix + 7 - pt.first);
                if (i == 0) x |= pos << (fbase + 5);
                else if (i == 1) y |= pos << 24;
                else if (i == 2) z |= pos << 20;
                else z |= pos << 26;
                for (int rr = pt.first; rr < pt.first + pt.len; rr++)
                {
                    const size_t at = (size_t) (e + prefix + (rr - pt.first));
                    if (with_vals) out->tval[at] = p.pval[(size_t) pt.src * 8 + (size_t) rr];
                    slot_of[(size_t) pt.src * 8 + (size_t) rr] = (uint32_t) at;
                }
                prefix += pt.len;
            }
            uint32_t *rec = record(g, r, w);
            rec[0] = x;
            rec[1] = y;
            rec[2] = z;
        }
        // what is fetched D rounds ahead: value block (offset, size class), column
        for (int r = 0; r < to.nr; r++)
        {
            const int rd = r + D;
            uint32_t *rec = record(g, r, w);
            rec[2] |= (uint32_t) (rd < to.nr ? voff[(size_t) rd] : voff[(size_t) to.nr]);
            if (rd < to.nr && nvals[(size_t) rd] > 0) rec[1] |= (uint32_t) ((nvals[(size_t) rd] + 7) / 8 - 1) << 30;
            // (an empty slot fetches a row of the team that nobody reads: testing for it in the kernel's issue block, behind
            //  the barrier and on the CU's one scalar unit, cost more than the few fetches of the default schedules)
            rec[3] = (uint32_t) ((rd < to.nr && to.col[(size_t) rd * W + (size_t) w] != TEAM2_NOCOL) ? to.col[(size_t) rd * W + (size_t) w] : to.anycol);
            // flags that steer the kernel's round (tools/gen_team2_asm.py)
            if (rd < to.nr) rec[0] |= 1u << fbase;                                   // ISSUE: fetch for round r + D
            if (r + D - 1 >= to.nr) rec[0] |= 1u << (fbase + 1);                           // TAIL: fewer than D-1 younger rounds in flight
            if (r == to.nr - 1) rec[0] |= 1u << (fbase + 2);                               // LAST
            if (w == 0 && (r & 7) == 0 && (r >> 3) + 1 < (to.nr + 7) / 8) rec[0] |= 1u << (fbase + 3);   // RECS: fetch the next record block
        }
        for (int d = 0; d < D; d++)
        {
            int *pr = &out->tpro[(((size_t) g * D + (size_t) d) * W + (size_t) w) * 2];
            // (the prologue's fetches are compiled code with a fixed DMA count: an empty slot fetches a valid row)
            pr[0] = (d < to.nr && to.col[(size_t) d * W + (size_t) w] != TEAM2_NOCOL) ? to.col[(size_t) d * W + (size_t) w] : to.anycol;
            pr[1] = (int) ((d < to.nr) ? voff[(size_t) d] : voff[(size_t) to.nr]);
        }
    }
};

}  // namespace

void build_team2(const PanelHost &p, int nrow, const int *rowptr, const int *colidx, Team2Host *out, const int *colpos, TeamSeed *seed)
{
    PhaseClock clk;
    released_async<TeamHost> th_owner;                                      // (freed by a background thread)
    TeamHost &th = *th_owner;
    // The balanced passes of build_teams break the ties of the phase key (a lattice team has twenty nodes per key value): in
    // plain column order the nodes of one wave come in runs, the rounds then hold four parts of one wave and none of another,
    // and a round lasts as long as its busiest wave -- pwtk stand-in 0.304 -> 0.315 ms at n = 256, 0.199 -> 0.210 at n = 128.
    const bool with_vals = team_prelude(p, nrow, rowptr, colidx, true, seed, &th, out);
    clk.lap("build_team2: build_teams total");
    const int nteam = th.nteam;
    // Phase key of a union entry: (position of its B row in the processing order) mod S, S = rows a team advances
    // along its sweep (8 x the consecutive panels of a lattice team, 64 for eight consecutive panels).  Teams are
    // dealt to the workgroups of an XCD in order and start a fraction of a microsecond apart; a B row shared by
    // neighbouring teams sits S positions further in the next one.  Walking every team's union by this key makes
    // all its readers ask for it at the same point of their lives, i.e. within the few microseconds a line
    // survives in the XCD's L2 -- instead of at unrelated moments of 35-microsecond lives.
    const int S = th.lattice ? 8 * th.st : 8 * T;
    auto key = [&](int q) {
        const int c = th.tcol[(size_t) q];
        const long long ps = c >= 0 ? (colpos ? colpos[c] : c) : (long long) (~c);
        // clustered teams (square part): where the row of A with this number sits inside ITS team
        if (th.clustered && c >= 0 && ps / 8 < (long long) th.plocal.size()) return (int) (ps % 8) * 16 + th.plocal[(size_t) (ps / 8)];      // (row of the panel, slot): neighbours in the order belong to different waves
        return (int) (ps % S);
    };
    // the launch grid's cuts: work of a team = union entries / W + a fixed cost
    const std::vector<int> nn = count_team_nodes(th);
    auto work = [&](int g) { return (nn[(size_t) g] + W - 1) / W + 4; };
    int cut[9];
    xcd_cuts(out->torder, work, cut);
    const int rpool = teams_per_pool(nteam, 32);
    std::vector<RoundPool> rpools((size_t) ((nteam + rpool - 1) / rpool));
    std::vector<TeamOut> res((size_t) nteam);
    schedule_rounds(p, th, nn, key, rpool, rpools, res);
    clk.lap("build_team2: rounds (phase sort, list scheduler)");
    if (th.lattice && th.lat_key.size() == (size_t) nteam * 3 && knobs().t2_latorder)
    {
        if (search_lattice_order(th, res, clk.on, &out->torder)) xcd_cuts(out->torder, work, cut);
        clk.lap("build_team2: lattice order search");
    }
    const std::vector<int> blk0 = layout_streams(res, out);
    build_tgrid(cut, out->torder, &out->tgrid);
    parallel_fill(out->trec, (size_t) blk0[(size_t) nteam] * blkw + blkw, 0u);
    if (with_vals) parallel_fill(out->tval, (size_t) out->nvalues, 0.0);
    else big_vector<double>().swap(out->tval);
    big_vector<uint32_t> slot_of;                                          // panel-format value slot -> tval slot
    slot_of.resize(p.pcol.size() * 8);          // (only the (entry, row) pairs that exist are written below and read through pmap)
    const StreamWriter writer{p, out, blk0, slot_of, with_vals};
    parallel_chunks(nteam, 32, [&](long long b, long long e, int) {
        for (long long g = b; g < e; g++)
            for (int w = 0; w < W; w++) writer.wave(res[(size_t) g], (int) g, w);
    });
    clk.lap("build_team2: records, value streams");
    build_vmap(p, slot_of, &out->vmap);
    clk.lap("build_team2: value-update map");
    release_pools(rpools);
    clk.lap("build_team2: release");
}

}  // namespace crp
