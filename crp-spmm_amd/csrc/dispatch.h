// dispatch.h -- which kernel a product runs (internal; host-only, no HIP types).  The create-time traits of a matrix, the
// operand checks of the kernels and the rules that pick the variant live here and nowhere else: hip_api.hip asks them, and so
// does crp_spmm_plan_host() (the CPU tests of the policy).
#pragma once
#include <stdint.h>
#include <vector>
#include "knobs.h"

namespace crp {

// The locality order of the rows for the derived formats (locality.h): perm[i] = original row at position i, f_* = the CSR in
// that order, f_nz[p'] = original position of its nonzero p'.  Empty perm = the caller's order.
struct FormatOrder
{
    std::vector<int>      perm, f_rowptr, f_colidx;
    std::vector<uint32_t> f_nz;
};
FormatOrder format_order(int nrow, int ncol, const int *rowptr, const int *colidx, bool two_source);

// What create time decides, from the CSR in format order
struct MatrixTraits
{
    int       nrow = 0;
    long long nnz = 0;
    int       auto_variant = 1;   // what variant 0 resolves to below the team kernel's widths (1 rowgroup, 2 panel R4, 3 panel R8)
    bool      team2_pays = false; // 64 consecutive rows share columns: variant 0 takes team2 from team2_min_n columns on
    int       team2_min_n = 96;
    bool      panels_sparse = false;   // fewer than 35 % of the (row, entry) pairs of the R = 8 panels are present (KKT systems)
};
MatrixTraits matrix_traits(int nrow, const int *rowptr, const int *colidx);

// A row-major operand: widths, row strides, whether B1 is there and whether B0, B1 and C are 16-byte aligned
struct Operand
{
    int       n = 0;
    long long ldB0 = 0, ldB1 = 0, ldC = 0;
    bool      has_b1 = false;
    bool      aligned16 = true;
};
bool panel_applicable(const Operand &op);
bool team2r_applicable(const Operand &op, int G);
template <typename T> bool team2_applicable(const Operand &op);

// The variant an fp64 product launches (1, 2, 3, 5 or 7).  team2r_refused: a variant-0 product found the row-owner streams of
// this matrix too large (crp_spmm_csr_f64).
int resolve_f64(const MatrixTraits &t, const Operand &op, int variant, bool team2r_refused, const Knobs &k);
// ... an fp32 product (1 or 5)
int resolve_f32(const MatrixTraits &t, const Operand &op, int variant);

// whether the team kernel's value blocks hold only the values that exist (Team2Host::compact)
bool team2_compact(double fill, bool for_f32);

}  // namespace crp
