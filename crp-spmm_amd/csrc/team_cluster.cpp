// team_cluster.cpp -- greedy clustering by shared keys (team_cluster.h): panels into teams, teams into super-teams.
#include <algorithm>
#include <cmath>
#include "team_cluster.h"

namespace crp {

// (One function of 110 lines: the growth loop works on a dozen arrays of the range it has just indexed.)
void greedy_cluster(int n, const std::vector<long long> &iptr, const big_vector<uint32_t> &ikey, int G, int span,
                           std::vector<int> *group_of, std::vector<int> *slot_of, int *ngroups, bool ratio)
{
    group_of->assign((size_t) n, -1);
    slot_of->assign((size_t) n, 0);
    const int nrange = (n + span - 1) / span;
    std::vector<int> range_groups((size_t) nrange, 0);
    parallel_chunks(nrange, 1, [&](long long rb, long long re, int) {
        for (long long rg = rb; rg < re; rg++)
        {
            const int i0 = (int) rg * span, i1 = std::min(n, i0 + span), cnt = i1 - i0;
            // inverted index of the range: (key, item) pairs sorted by key
            big_vector<std::pair<uint32_t, int>> pairs;          // (big_vector: huge pages for the range's tens of megabytes, par.h)
            pairs.reserve((size_t) (iptr[(size_t) i1] - iptr[(size_t) i0]));
            for (int i = i0; i < i1; i++)
                for (long long q = iptr[(size_t) i]; q < iptr[(size_t) i + 1]; q++) pairs.push_back({ikey[(size_t) q], i - i0});
            std::sort(pairs.begin(), pairs.end());
            // dense local key ids
            std::vector<long long> kptr;
            big_vector<int> kitem(pairs.size());
            big_vector<int> lkey(pairs.size());                 // per pair (in item order below): local key id
            for (size_t t = 0; t < pairs.size(); t++)
            {
                if (t == 0 || pairs[t].first != pairs[t - 1].first) kptr.push_back((long long) t);
                kitem[t] = pairs[t].second;
            }
            kptr.push_back((long long) pairs.size());
            // item -> local key ids (same order as ikey)
            std::vector<long long> lptr((size_t) cnt + 1, 0);
            for (int i = 0; i < cnt; i++) lptr[(size_t) i + 1] = lptr[(size_t) i] + (iptr[(size_t) (i0 + i) + 1] - iptr[(size_t) (i0 + i)]);
            {
                std::vector<long long> fill(lptr.begin(), lptr.end() - 1);
                const int nk = (int) kptr.size() - 1;
                for (int kk = 0; kk < nk; kk++)
                    for (long long t = kptr[(size_t) kk]; t < kptr[(size_t) kk + 1]; t++) lkey[(size_t) fill[(size_t) kitem[(size_t) t]]++] = kk;
            }
            const int nk = (int) kptr.size() - 1;
            std::vector<char> assigned((size_t) cnt, 0), inkey((size_t) nk, 0);
            std::vector<int> cc((size_t) cnt, 0), touched, ukeys;
            int seed = 0, groups = 0;
            auto add = [&](int it) {
                for (long long q = lptr[(size_t) it]; q < lptr[(size_t) it + 1]; q++)
                {
                    const int kk = lkey[(size_t) q];
                    if (inkey[(size_t) kk]) continue;
                    inkey[(size_t) kk] = 1;
                    ukeys.push_back(kk);
                    for (long long t = kptr[(size_t) kk]; t < kptr[(size_t) kk + 1]; t++)
                    {
                        const int r = kitem[(size_t) t];
                        if (assigned[(size_t) r]) continue;
                        if (cc[(size_t) r]++ == 0) touched.push_back(r);
                    }
                }
            };
            for (;;)
            {
                while (seed < cnt && assigned[(size_t) seed]) seed++;
                if (seed >= cnt) break;
                const int gid = groups++;
                int members = 0;
                auto take = [&](int it) {
                    assigned[(size_t) it] = 1;
                    (*group_of)[(size_t) (i0 + it)] = gid;          // range-local id, made global below
                    (*slot_of)[(size_t) (i0 + it)] = members++;
                    add(it);
                };
                take(seed);
                while (members < G)
                {
                    int best = -1, bo = 0;
                    long long bsz = 1;
                    for (int r : touched)
                    {
                        if (assigned[(size_t) r]) continue;
                        const int o = cc[(size_t) r];
                        if (!ratio)
                        {
                            if (o > bo || (o == bo && best >= 0 && std::abs(r - seed) < std::abs(best - seed))) { best = r; bo = o; }
                            continue;
                        }
                        const long long sz = std::max<long long>(1, lptr[(size_t) r + 1] - lptr[(size_t) r]);
                        // o / sz against bo / bsz
                        const long long lhs = (long long) o * bsz, rhs = (long long) bo * sz;
                        if (best < 0 || lhs > rhs || (lhs == rhs && (o > bo || (o == bo && std::abs(r - seed) < std::abs(best - seed))))) { best = r; bo = o; bsz = sz; }
                    }
                    if (best < 0)
                    {
                        // nothing shares a key with the group (isolated rows, empty panels): the next unassigned item
                        int nx = seed;
                        while (nx < cnt && assigned[(size_t) nx]) nx++;
                        if (nx >= cnt) break;
                        best = nx;
                    }
                    take(best);
                }
                for (int r : touched) cc[(size_t) r] = 0;
                touched.clear();
                for (int kk : ukeys) inkey[(size_t) kk] = 0;
                ukeys.clear();
            }
            range_groups[(size_t) rg] = groups;
        }
    });
    std::vector<int> base((size_t) nrange + 1, 0);
    for (int rg = 0; rg < nrange; rg++) base[(size_t) rg + 1] = base[(size_t) rg] + range_groups[(size_t) rg];
    parallel_chunks(n, 1 << 16, [&](long long b, long long e, int) {
        for (long long i = b; i < e; i++) (*group_of)[(size_t) i] += base[(size_t) (i / span)];
    });
    *ngroups = base[(size_t) nrange];
}

}  // namespace crp
