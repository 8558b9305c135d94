// team_cluster.h -- internal to team_format.cpp: items with lists of keys, clustered greedily by the keys they share.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "par.h"

namespace crp {

// ---- greedy clustering (teams of panels, super-teams of teams) -----------------------------------------
// Items carry sorted lists of distinct keys (CSR iptr / ikey).  Groups of up to G items are grown from the lowest
// unassigned item by repeatedly adding the unassigned item that shares most keys with the group's union (ties: the
// nearest index).  Work per group: the union's keys times the items per key.  Items are handled in independent
// ranges of `span` items (threads), a group never crosses a range.  -> group of every item, in creation order;
// slot = its position inside the group.
// ratio = true: the item that has the largest FRACTION of its own keys in the union already (ties: more shared keys) --
// an item whose keys are a subset of the group's costs the group nothing, however short its list (the 7-point dual
// rows of a KKT system next to the 27-point primal rows of the same nodes).
void greedy_cluster(int n, const std::vector<long long> &iptr, const big_vector<uint32_t> &ikey, int G, int span,
                    std::vector<int> *group_of, std::vector<int> *slot_of, int *ngroups, bool ratio = false);

// CSR of sorted distinct keys per item, built in parallel: raw(i, buf) appends item i's keys to buf.
template <typename F>
void build_key_csr(int n, F raw, std::vector<long long> *iptr, big_vector<uint32_t> *ikey)
{
    constexpr int CH = 2048;
    const int nch = (n + CH - 1) / CH;
    iptr->assign((size_t) n + 1, 0);
    std::vector<big_vector<uint32_t>> cbuf((size_t) nch);
    parallel_chunks(nch, 1, [&](long long cb, long long ce, int) {
        for (long long c = cb; c < ce; c++)
        {
            big_vector<uint32_t> &buf = cbuf[(size_t) c];
            const int i0 = (int) c * CH, i1 = std::min(n, i0 + CH);
            for (int i = i0; i < i1; i++)
            {
                const size_t at = buf.size();
                raw(i, buf);
                std::sort(buf.begin() + (long) at, buf.end());
                buf.erase(std::unique(buf.begin() + (long) at, buf.end()), buf.end());
                (*iptr)[(size_t) i + 1] = (long long) (buf.size() - at);
            }
        }
    });
    for (int i = 0; i < n; i++) (*iptr)[(size_t) i + 1] += (*iptr)[(size_t) i];
    ikey->resize((size_t) (*iptr)[(size_t) n]);
    parallel_chunks(nch, 1, [&](long long cb, long long ce, int) {
        for (long long c = cb; c < ce; c++)
            if (!cbuf[(size_t) c].empty())
                memcpy(ikey->data() + (*iptr)[(size_t) c * CH], cbuf[(size_t) c].data(), sizeof(uint32_t) * cbuf[(size_t) c].size());
    });
}

}  // namespace crp
