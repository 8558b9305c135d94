// dropout.h -- the attention-dropout mask of the fused GAT / GATv2 calls: plain integer code for host and device.
// The keep bit of edge (r, c) and head h is a pure function of (seed, r, c, h), so the forward, both sides of the backward and
// crp_dropout_mask_csr re-form it and nothing nnz-sized is stored between forward and backward.
//
// GENERATOR.  Philox4x32-10 (Salmon et al., SC'11; the generator behind torch's device dropout): multipliers 0xD2511F53 and
// 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds of
//     c = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
// with the key bumped after each round.
//
// DRAW.  key = (seed low word, seed high word), counter = (r, c, h, 0), x = output word 0; the edge is kept iff x >= thr with
// thr = (uint32) floor(drop 2^32), formed once on the host in double (the product is exact for 0 <= drop < 1).  For
// 0 < drop < 2^-32 the threshold is 0 and every edge is kept.  r is the row of O / el / XT / lse the entry belongs to (on a handle
// of A: after the handle's row map; on a handle of A^T: the entry's column index), c the 32-bit column code as stored (on a handle
// of A: the entry's code, a second-source code as its bit pattern; on a handle of A^T: the handle's row after its row map).  On a
// one-source pair both handles therefore draw the same bit for the same edge.  Duplicate (r, c) entries share a bit.
#ifndef CRP_DROPOUT_H
#define CRP_DROPOUT_H
#include <stdint.h>

#if defined(__HIP__)
#define CRP_DROPOUT_HD __host__ __device__
#else
#define CRP_DROPOUT_HD
#endif

namespace crp {

// out = Philox4x32-10 of counter c and key (k0, k1)
CRP_DROPOUT_HD inline void philox4x32_10(const uint32_t (&c)[4], uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int round = 0; round < 10; round++)
    {
        const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t) (p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t) (p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t) p1;
        c3 = (uint32_t) p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// thr of a rate 0 <= drop < 1
inline uint32_t dropout_threshold(double drop) { return (uint32_t) (drop * 4294967296.0); }

// the keep bit of edge (r, c), head h
CRP_DROPOUT_HD inline bool dropout_keep(uint32_t seed_lo, uint32_t seed_hi, uint32_t r, uint32_t c, uint32_t h, uint32_t thr)
{
    const uint32_t ctr[4] = {r, c, h, 0u};
    uint32_t x[4];
    philox4x32_10(ctr, seed_lo, seed_hi, x);
    return x[0] >= thr;
}

// what a kernel takes: set by the entry points, read by the DROP instances only
template <typename T> struct DropArgs
{
    bool     on = false;    // drop > 0: the launchers take the DROP instances
    uint32_t thr = 0;
    uint32_t seed_lo = 0, seed_hi = 0;
    T        rs = (T) 1;    // (T) (1 / (1 - drop)), formed in double and rounded once
};
template <typename T> inline DropArgs<T> dropout_args(double drop, unsigned long long seed)
{
    DropArgs<T> d;
    d.on = drop > 0.0;
    d.thr = dropout_threshold(drop);
    d.seed_lo = (uint32_t) seed;
    d.seed_hi = (uint32_t) (seed >> 32);
    d.rs = (T) (1.0 / (1.0 - drop));
    return d;
}

}  // namespace crp
#endif
