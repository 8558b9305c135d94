// Digest of everything the host format builders produce (CPU only; built and run by tests/test_format_digest.py).
// The builders are deterministic -- the same bytes whatever the number of threads --, so the output of this program
// compared between two commits ON ONE MACHINE is a complete test of a change that is meant to leave the formats alone:
// build it against both trees with the same compiler and flags and compare the outputs.  No digest value is committed:
// std::sort may place equal elements differently in another standard library.
// It uses the public header only (panel_format.h, locality.h) and, like host_asan.cpp, stubs the device ABI.
//
//   host_format_digest [first [last]]   one line per (matrix, format): FNV-1a of every output array, sizes included
//   host_format_digest --time stencil|kkt
//       the device path's builds (structure-only panels, one seed for team2, team2r G = 4 and G = 2) on a large input:
//       27-point stencil on 128^3 in natural order (lattice teams) / the KKT-like generator at two million rows
//       (clustered teams of two kinds of panels, super-teams); total seconds on stdout, CRPSPMM_TIMING=1 gives the laps
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <vector>
#include "locality.h"
#include "panel_format.h"

extern "C" {
int crp_dev_malloc(void **p, size_t) { *p = NULL; return -1; }
int crp_dev_free(void *) { return -1; }
int crp_dev_memset(void *, int, size_t, void *) { return -1; }
int crp_dev_memcpy(void *, const void *, size_t, int, void *) { return -1; }
int crp_dev_memcpy2d(void *, size_t, const void *, size_t, size_t, size_t, int, void *) { return -1; }
int crp_host_malloc(void **p, size_t) { *p = NULL; return -1; }
int crp_host_free(void *) { return -1; }
int crp_stream_sync(void *) { return -1; }
}

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t) (rng_state >> 11);
}

struct Csr { int m, k; std::vector<int> rp, ci; std::vector<double> va; };

static std::vector<int> both_signs(const std::vector<int> &offs)
{
    std::vector<int> all;
    for (int d : offs) { all.push_back(d); all.push_back(-d); }
    all.push_back(0);
    std::sort(all.begin(), all.end());
    return all;
}

// the generators of host_asan.cpp (same sequence of random numbers when called in the same order)
static Csr banded(int m, const std::vector<int> &offs)
{
    Csr a; a.m = a.k = m; a.rp.assign(m + 1, 0);
    const std::vector<int> all = both_signs(offs);
    for (int i = 0; i < m; i++)
    {
        for (int d : all)
            if (i + d >= 0 && i + d < m) { a.ci.push_back(i + d); a.va.push_back(1.0 + (rnd() % 100) * 0.01); }
        a.rp[i + 1] = (int) a.ci.size();
    }
    return a;
}

static Csr random_csr(int m, int k, int maxdeg, bool dup, bool two_source)
{
    Csr a; a.m = m; a.k = k; a.rp.assign(m + 1, 0);
    for (int i = 0; i < m; i++)
    {
        const int deg = (i % 7 == 3) ? 0 : (int) (rnd() % (maxdeg + 1));
        std::vector<int> c;
        for (int t = 0; t < deg; t++) c.push_back((int) (rnd() % k));
        std::sort(c.begin(), c.end());
        if (!dup) c.erase(std::unique(c.begin(), c.end()), c.end());
        for (int x : c)
        {
            a.ci.push_back(two_source && x >= k / 2 ? ~(x - k / 2) : x);
            a.va.push_back((rnd() % 2000) * 0.001 - 1.0);
        }
        a.rp[i + 1] = (int) a.ci.size();
    }
    return a;
}

// KKT-like, two kinds of rows: n0 primal rows -- a banded block plus one column in the dual range -- followed by n0 dual
// rows of three entries in the primal range.  The dual panels hold under half the mean number of entries, so the teams
// are clustered in the order of the panels' median columns (build_teams, `mix`).
static Csr kkt_like(int n0, const std::vector<int> &offs)
{
    Csr a; a.m = a.k = 2 * n0; a.rp.assign(2 * (size_t) n0 + 1, 0);
    const std::vector<int> all = both_signs(offs);
    for (int i = 0; i < n0; i++)
    {
        for (int d : all)
            if (i + d >= 0 && i + d < n0) { a.ci.push_back(i + d); a.va.push_back(1.0 + (rnd() % 100) * 0.01); }
        a.ci.push_back(n0 + i); a.va.push_back(0.5);
        a.rp[i + 1] = (int) a.ci.size();
    }
    for (int i = 0; i < n0; i++)
    {
        for (int d : {-1, 0, 1})
            if (i + d >= 0 && i + d < n0) { a.ci.push_back(i + d); a.va.push_back(0.25 + d); }
        a.rp[n0 + i + 1] = (int) a.ci.size();
    }
    return a;
}

// rows 0 .. nfilled - 1 of a random matrix, the rest empty: with fewer than 16 panels the teams are consecutive panels, and a
// team of empty panels gets the one empty round the team2r kernel's pipeline wants
static Csr top_rows_only(int m, int k, int maxdeg, int nfilled)
{
    Csr a = random_csr(nfilled, k, maxdeg, false, false);
    a.m = m;
    a.rp.resize((size_t) m + 1, a.rp.back());
    return a;
}

// a near band of `near` diagonals on either side and two thin far bands on nested strides: a stride lattice is detected, and
// the clustered teams need clearly fewer union entries than its tooth-shaped teams (build_teams: u_la > 1.15 u_cl)
static Csr wide_band_lattice(int m, int near, int d1, int d2)
{
    std::vector<int> offs;
    for (int i = 1; i <= near; i++) offs.push_back(i);
    for (int d = -2; d <= 2; d++) { offs.push_back(d1 + d); offs.push_back(d2 + d); }
    return banded(m, offs);
}

// 27-point stencil on a g^3 grid in natural order, structure only (the timing mode builds without values)
static Csr stencil27(int g)
{
    Csr a; a.m = a.k = g * g * g; a.rp.assign((size_t) a.m + 1, 0);
    a.ci.reserve((size_t) 27 * a.m);
    for (int z = 0; z < g; z++)
        for (int y = 0; y < g; y++)
            for (int x = 0; x < g; x++)
            {
                for (int dz = -1; dz <= 1; dz++)
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++)
                            if (x + dx >= 0 && x + dx < g && y + dy >= 0 && y + dy < g && z + dz >= 0 && z + dz < g)
                                a.ci.push_back(((z + dz) * g + (y + dy)) * g + (x + dx));
                a.rp[(size_t) ((z * g + y) * g + x) + 1] = (int) a.ci.size();
            }
    return a;
}

// ---- one output line: "<matrix> <format> [key=value ...] name=digest ..."
static uint64_t fnv(uint64_t h, const void *data, size_t bytes)
{
    const unsigned char *p = (const unsigned char *) data;
    for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
template <class V>
static void dig(const char *name, const V &v)
{
    const uint64_t n = v.size();
    uint64_t h = fnv(1469598103934665603ull, &n, sizeof(n));
    if (n > 0) h = fnv(h, v.data(), sizeof(v[0]) * v.size());
    printf(" %s=%016llx", name, (unsigned long long) h);
}

static void dig_panels(const crp::PanelHost &h)
{
    dig("pptr", h.pptr); dig("pcol", h.pcol); dig("pmask4", h.pmask4); dig("pval", h.pval); dig("pmap", h.pmap); dig("porder", h.porder); dig("psync", h.psync);
    printf("\n");
}
static void dig_team2(const crp::Team2Host &t)
{
    printf(" nteam=%d lattice=%d", t.nteam, (int) t.lattice);
    dig("tpanel", t.tpanel); dig("torder", t.torder); dig("tgrid", t.tgrid); dig("tinfo", t.tinfo); dig("tpro", t.tpro); dig("trec", t.trec);
    dig("tvoff", t.tvoff); dig("tval", t.tval); dig("vmap", t.vmap);
    printf("\n");
}
static void dig_team2r(const crp::Team2RHost &t, bool ok)
{
    printf(" ok=%d nteam=%d", (int) ok, t.nteam);
    dig("tpanel", t.tpanel); dig("torder", t.torder); dig("tgrid", t.tgrid); dig("tinfo", t.tinfo); dig("trec", t.trec); dig("tent", t.tent);
    dig("tvoff", t.tvoff); dig("tval", t.tval); dig("vmap", t.vmap);
    printf("\n");
}

// what the device path builds: panels without values or order, the teams of team2 seed both team2r formats
static void device_path(const Csr &a, const int *colpos, const char *tag)
{
    crp::PanelHost sk;
    crp::build_panels(a.m, a.rp.data(), a.ci.data(), nullptr, 8, &sk, false, false);
    crp::TeamSeed seed;
    {
        crp::Team2Host t;
        crp::build_team2(sk, a.m, a.rp.data(), a.ci.data(), &t, colpos, &seed);
        printf("%s dev.team2  ", tag);
        dig_team2(t);
    }
    for (int G : {4, 2})
    {
        crp::Team2RHost t;
        t.G = G;
        const bool ok = crp::build_team2r(sk, a.m, a.rp.data(), a.ci.data(), &t, colpos, &seed);
        printf("%s dev.team2r%d", tag, G);
        dig_team2r(t, ok);
    }
}

static void all_formats(const Csr &a, int mi)
{
    char tag[16];
    snprintf(tag, sizeof(tag), "%2d", mi);
    for (int R : {4, 8})
    {
        crp::PanelHost h;
        crp::build_panels(a.m, a.rp.data(), a.ci.data(), a.va.data(), R, &h);
        printf("%s panel%d     ", tag, R);
        dig_panels(h);
    }
    crp::PanelHost h8;
    crp::build_panels(a.m, a.rp.data(), a.ci.data(), a.va.data(), 8, &h8, false);
    {
        // the cheap counting passes and the compact values of the narrow-operand kernel
        printf("%s panel8.cv   entries4=%lld entries8=%lld union64=%lld", tag, crp::count_panel_entries(a.m, a.rp.data(), a.ci.data(), 4),
               crp::count_panel_entries(a.m, a.rp.data(), a.ci.data(), 8), crp::count_block_union(a.m, a.rp.data(), a.ci.data(), 64));
        crp::PanelHost hc = h8;
        printf(" ok=%d fill=%.6f", (int) crp::build_compact_values(&hc), hc.fill());
        dig("cmo", hc.cmo); dig("cbase", hc.cbase); dig("cval", hc.cval); dig("cmap", hc.cmap);
        printf("\n");
    }
    {
        crp::TeamHost t;
        crp::build_teams(h8, a.m, a.rp.data(), a.ci.data(), &t);
        printf("%s teams4      nteam=%d lattice=%d", tag, t.nteam, (int) t.lattice);
        dig("tpanel", t.tpanel); dig("tptr", t.tptr); dig("tcol", t.tcol); dig("tmask", t.tmask); dig("torder", t.torder); dig("tvoff", t.tvoff);
        dig("tsrc", t.tsrc); dig("lat_key", t.lat_key);
        printf("\n");
    }
    std::vector<int> perm, pos;
    bool square = a.m == a.k;
    for (int c : a.ci) square = square && c >= 0;
    if (square && crp::locality_reorder(a.m, a.k, a.rp.data(), a.ci.data(), 8, &perm))
    {
        pos.assign((size_t) a.m, -1);
        for (int i = 0; i < a.m; i++) pos[(size_t) perm[(size_t) i]] = i;
    }
    const int *colpos = pos.empty() ? nullptr : pos.data();
    for (int compact : {1, 0})
    {
        crp::Team2Host t;
        t.compact = compact != 0;
        crp::build_team2(h8, a.m, a.rp.data(), a.ci.data(), &t, colpos);
        printf("%s team2%c     ", tag, compact ? 'c' : 'f');
        dig_team2(t);
    }
    for (int G : {4, 2})
    {
        crp::Team2RHost t;
        t.G = G;
        const bool ok = crp::build_team2r(h8, a.m, a.rp.data(), a.ci.data(), &t, colpos);
        printf("%s team2r%d    ", tag, G);
        dig_team2r(t, ok);
    }
    device_path(a, colpos, tag);
}

int main(int argc, char **argv)
{
    if (argc >= 3 && strcmp(argv[1], "--time") == 0)
    {
        const bool kkt = strcmp(argv[2], "kkt") == 0;
        const Csr a = kkt ? kkt_like(100 * 100 * 100, {1, 2, 100, 101, 10000, 10001}) : stencil27(128);
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        device_path(a, nullptr, kkt ? "kkt" : "stencil");
        clock_gettime(CLOCK_MONOTONIC, &t1);
        // (the digests are inside the interval: the same work on both sides of a comparison)
        printf("%s total %.3f s\n", kkt ? "kkt" : "stencil", (double) (t1.tv_sec - t0.tv_sec) + 1e-9 * (double) (t1.tv_nsec - t0.tv_nsec));
        return 0;
    }
    std::vector<Csr> mats;
    // host_asan.cpp's `mats` ...
    mats.push_back(banded(300 * 8 * 5 + 13, {1, 2, 3, 300, 301, 2400, 2401}));       // stride lattice, ragged end
    mats.push_back(banded(5000, {1, 2, 3, 40, 900}));
    mats.push_back(random_csr(777, 1234, 40, true, false));
    mats.push_back(random_csr(301, 500, 9, false, true));
    mats.push_back(random_csr(5, 9, 3, false, false));
    mats.push_back(random_csr(0, 4, 3, false, false));
    // ... its `t2` additions ...
    mats.push_back(banded(9120, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 304, 305, 306, 307, 308, 309, 3040, 3041, 3042, 3043, 3044, 3045}));
    mats.push_back(banded(300 * 40 + 5, {1, 2, 300, 301, 302}));                     // clustered teams, super-teams (>= 128 teams)
    mats.push_back(banded(96 * 32 * 32 + 3, {1, 2, 3, 96, 97, 96 * 32, 96 * 32 + 1}));   // a lattice with >= 1024 teams: the order search
    // ... two kinds of rows: median order, 600 clustered teams
    mats.push_back(kkt_like(40 * 40 * 12, {1, 2, 40, 41, 1600, 1601}));
    // ... a lattice that is detected and loses against the clusters; a team without a nonzero
    mats.push_back(wide_band_lattice(300 * 8 * 5 + 13, 32, 300, 2400));
    mats.push_back(top_rows_only(120, 200, 6, 64));
    const int first = argc > 1 ? atoi(argv[1]) : 0, last = argc > 2 ? atoi(argv[2]) : (argc > 1 ? first : (int) mats.size() - 1);
    for (int mi = first; mi <= last && mi < (int) mats.size(); mi++) all_formats(mats[(size_t) mi], mi);
    return 0;
}
