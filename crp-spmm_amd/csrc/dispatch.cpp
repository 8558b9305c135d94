// dispatch.cpp -- see dispatch.h
#include "dispatch.h"
#include "locality.h"
#include "panel_format.h"

namespace crp {

// fp64 columns from which auto picks variant 5.  Round 4: the one-piece instances (n <= 128) run THREE workgroups per CU (80
// VGPRs, 43 KiB of LDS) -- pwtk stand-in n = 128 0.181 -> 0.163 ms, nlpkkt stand-in n = 96 1.18 -> 0.98 -- and the crossover against
// the row-panel kernel moved down (profiles/r04_team2_min_n.txt, variant 3 / 5: pwtk stand-in n = 80 0.138 / 0.146, n = 96 0.155 /
// 0.151, n = 112 0.167 / 0.154; shell n = 64 0.120 / 0.119, n = 96 0.166 / 0.137; Queen stand-in n = 64 0.447 / 0.403, n = 96 0.531 / 0.444).
constexpr int TEAM2_MIN_N = 96;
// ... and for a FULL half-piece tile (61 .. 64 columns) since the value blocks are compact (round 4, item 7): the half-piece instance takes the
// same time from 48 to 64 columns, the row-panel kernel's grows with them -- pwtk stand-in, variant 3 / 5: n = 48 0.0929 / 0.1093 ms, n = 64
// 0.1134 / 0.1096, n = 80 0.1389 / 0.1378, n = 96 0.1546 / 0.1547 (profiles/r04_compact_ab.txt).
constexpr int TEAM2_HALF_FULL_LO = 61, TEAM2_HALF_FULL_HI = 64;
// ... where the row-panel format asks for more than 12 B row slices per row of A (Queen stand-in: 17.3; pwtk: 10.4), or the matrix has
// no stride lattice (the row-panel kernel then runs without its team schedule).
// From 48 columns since the HALF-piece instances (operands of at most 64 fp64 / 128 fp32 columns: 8 bytes per lane, one FMA per row
// and part, four workgroups per CU; profiles/r04_half_piece_instances.txt, variant 3 / 5: Queen stand-in n = 48 0.424 / 0.339 ms,
// n = 64 0.451 / 0.361; shell n = 64 0.124 / 0.108; pwtk stand-in n = 64 0.119 / 0.126: stays with the row-panel kernel).
constexpr int TEAM2_MIN_N_NOLATTICE = 48;
// ... dense row-panel formats from 33 columns: the half-piece instance takes the same time from 34 to 64 columns (Queen stand-in, variant 3 / 5,
// compact values: n = 34 0.409 / 0.323 ms, n = 40 0.404 / 0.326; the shell stand-in, no lattice and 9 slices per row: 0.097 / 0.099 at both -- it
// keeps 48); at 32 columns the narrow kernel is ahead (0.235 / 0.314).
constexpr int TEAM2_MIN_N_DENSE = 33;
// ... when fewer than 35 % of the (row, entry) pairs of the R = 8 panels are present (KKT systems): the row-panel format then stores mostly
// zeros (8 values per entry) while the team kernel's value streams are compact.  From 33 columns since the half-piece instances and three
// workgroups per CU (round 4): up to 32 columns the row-owner team kernel (variant 7, four rows' slices per wave instruction) is 2 x ahead;
// above, variant 3 / 5 / 7 on the nlpkkt stand-in (profiles/r04_team2r_probes.txt): n = 34 0.971 / 0.784 / 0.833 ms, n = 48 1.016 / 0.801 /
// 0.834, n = 64 1.096 / 0.849 / 0.839, n = 72 1.148 / 0.930 / -; at nlpkkt240 size variant 5 / 7: n = 40 12.81 / 13.53, n = 48 13.27 / 13.35,
// n = 56 13.83 / 13.49, n = 64 13.72 / 13.91 -- the two-rows-per-lane-group format of variant 7 (n <= 64) buys nothing that the team format
// the matrix has anyway does not, and costs 4 s of build and 4 GB of HBM at that size: variant 0 no longer takes it (it was 80 in round 3).
constexpr int TEAM2_MIN_N_SPARSE = 33;
// fp32: the only other fp32 kernel is the CSR row-group one.  Since the half-piece instances (at most 128 fp32 columns: one time from 32 to
// 128) the team kernel is level or ahead from 32 columns -- row-group / team, ms (profiles/r04_compact_ab.txt, fp32 block): Queen stand-in n = 24
// 0.377 / 0.311, 32 0.385 / 0.310, 48 0.643 / 0.312, 64 0.662 / 0.316; shell 32 0.116 / 0.097, 48 0.177 / 0.098; pwtk stand-in 24 0.102 / 0.107, 32 0.107 /
// 0.108, 48 0.167 / 0.108 -- except on mostly-hole panels, where a part is 1.8 rows: nlpkkt stand-in 32 0.385 / 0.720, 48 0.664 / 0.734, 64 0.706 /
// 0.742, 96 1.301 / 0.789, 128 1.365 / 0.842 (it was 64 for every matrix).
constexpr int TEAM2_MIN_N_F32 = 32, TEAM2_MIN_N_F32_SPARSE = 65;

FormatOrder format_order(int nrow, int ncol, const int *rowptr, const int *colidx, bool two_source)
{
    // Locality order of the rows (locality.h) for the derived formats: taken when it lets rows of a panel share
    // more columns than the caller's order does (fewer R = 8 panel entries).  A mesh numbered along its own lines
    // (the stride-lattice matrices) keeps the caller's order -- consecutive rows there are neighbours already and
    // the lattice schedules build on that.  CRPSPMM_REORDER=0 never, =1 whenever the matrix qualifies.
    FormatOrder o;
    const long long nnz = rowptr[nrow];
    if (!(nnz > 0 && nrow >= 2048 && nrow == ncol && !two_source && nnz <= 200000000LL))    // (the graph of a larger matrix costs tens of GB)
        return o;
    const int mode = knobs().reorder;
    std::vector<int> perm;
    if (mode == 0 || !locality_reorder(nrow, ncol, rowptr, colidx, 8, &perm)) return o;
    o.f_rowptr.assign((size_t) nrow + 1, 0);
    for (int i = 0; i < nrow; i++) o.f_rowptr[(size_t) i + 1] = o.f_rowptr[(size_t) i] + (rowptr[perm[(size_t) i] + 1] - rowptr[perm[(size_t) i]]);
    o.f_colidx.resize((size_t) nnz);
    o.f_nz.resize((size_t) nnz);
    for (int i = 0; i < nrow; i++)
    {
        const int r = perm[(size_t) i];
        int q = o.f_rowptr[(size_t) i];
        for (int pz = rowptr[r]; pz < rowptr[r + 1]; pz++, q++)
        {
            o.f_colidx[(size_t) q] = colidx[pz];
            o.f_nz[(size_t) q] = (uint32_t) pz;
        }
    }
    const long long e_nat = count_panel_entries(nrow, rowptr, colidx, 8);
    const long long e_loc = count_panel_entries(nrow, o.f_rowptr.data(), o.f_colidx.data(), 8);
    if (mode == 1 || (double) e_loc < 0.9 * (double) e_nat) o.perm.swap(perm);
    else o = FormatOrder();
    return o;
}

MatrixTraits matrix_traits(int nrow, const int *rowptr, const int *colidx)
{
    MatrixTraits t;
    const long long nnz = rowptr[nrow];
    t.nrow = nrow;
    t.nnz = nnz;
    t.team2_min_n = TEAM2_MIN_N;
    // Pick the kernel family variant 0 resolves to.  The panel kernels pay off when rows of a
    // panel share columns (banded / FEM / block structure); with no sharing (fill -> 1/R) the
    // plain CSR kernel moves fewer bytes.  CRPSPMM_SPMM_VARIANT overrides (1, 2 or 3).
    if (nnz > 0 && nrow >= 8)
    {
        const long long e4 = count_panel_entries(nrow, rowptr, colidx, 4);
        const long long e8 = count_panel_entries(nrow, rowptr, colidx, 8);
        const double fill4 = (double) nnz / (4.0 * (double) e4);
        if (fill4 >= 0.45) t.auto_variant = ((double) e8 <= 0.72 * (double) e4) ? 3 : 2;
        // R = 8 panels also when an entry serves 1.7 rows or more on average, whatever R = 4 would do: the nlpkkt stand-in
        // (fill4 0.42, e8 / e4 0.89, e8 = 0.53 nnz) runs 0.63 / 1.04 / 1.32 ms at n = 32 / 64 / 96 on R = 8 panels against
        // 0.73 / 1.34 / 1.95 through CSR and 1.00 / 1.10 / 1.45 on R = 4; the shell stand-in 0.106 / 0.129 against 0.135 / 0.144
        // on R = 4.  Erdos-Renyi (e8 = nnz) stays with CSR.
        if ((double) e8 <= 0.6 * (double) nnz) t.auto_variant = 3;
        // ... or has no lattice team schedule to time its panels' shared rows in L2 (shell stand-in, locality order: n = 64 0.122 ms on the
        // row-panel kernel, 0.103 on the team kernel; the pwtk stand-in, a lattice with 10.4 slices per row: 0.115 / 0.120)
        {
            double D1 = 0, D2 = 0;
            int M = 0;
            const bool lat = nrow >= 4096 && detect_stride_lattice(nrow, rowptr, colidx, 8, &D1, &D2, &M);
            if (!lat) t.team2_min_n = TEAM2_MIN_N_NOLATTICE;
            if ((double) e8 > 12.0 * (double) nrow) t.team2_min_n = TEAM2_MIN_N_DENSE;
        }
        if ((double) nnz < 0.35 * 8.0 * (double) e8)
        {
            t.team2_min_n = TEAM2_MIN_N_SPARSE;
            // ... and at 24 .. 32 columns (24 .. 64 until the team kernel's half-piece instances: TEAM2_MIN_N_SPARSE) such panels go to the row-owner team kernel (variant 7, csrc/team2r_kernel.hip): nlpkkt
            // stand-in 0.388 / 0.839 ms at n = 32 / 64 against 0.546 / 1.04 of the narrow and row-panel kernels, at nlpkkt240 size
            // 6.58 / 14.0 against 8.85 / 18.2 (pwtk stand-in, fill 0.61: 0.075 against 0.062 -- stays).  CRPSPMM_TEAM2R=0|1 forces.
            t.panels_sparse = true;
        }
    }
    // The LDS-sharing team kernel fetches a B row once per team of 64 rows: it pays when those rows name far fewer
    // distinct columns than they have nonzeros (pwtk stand-in 0.10, shell 0.09, kkt 0.27, fem3d 0.13 of the nonzeros;
    // Erdos-Renyi 0.99, where the CSR kernel stays).
    if (nnz > 0 && nrow >= 64)
        t.team2_pays = (double) count_block_union(nrow, rowptr, colidx, 64) <= 0.6 * (double) nnz;
    if (knobs().spmm_variant >= 1 && knobs().spmm_variant <= 3) t.auto_variant = knobs().spmm_variant;
    return t;
}

bool panel_applicable(const Operand &op) { return op.n >= 24; }

// 24 <= n <= 128 / G (even), 16-byte aligned operands
bool team2r_applicable(const Operand &op, int G)
{
    return op.n >= 24 && op.n <= 128 / G && (op.n % 2 == 0) && (op.ldB0 % 2 == 0) && (op.ldC % 2 == 0) && (!op.has_b1 || op.ldB1 % 2 == 0) &&
           op.aligned16;
}

template <typename T> bool team2_applicable(const Operand &op)
{
    constexpr int VW = 16 / (int) sizeof(T);
    // (row strides are handed to the kernel as 32-bit byte counts)
    return op.n >= 24 && (op.n % VW == 0) && (op.ldB0 % VW == 0) && (op.ldC % VW == 0) && (!op.has_b1 || op.ldB1 % VW == 0) &&
           op.aligned16 && op.ldB0 * (long long) sizeof(T) < (1ll << 32) && (!op.has_b1 || op.ldB1 * (long long) sizeof(T) < (1ll << 32));
}
template bool team2_applicable<double>(const Operand &);
template bool team2_applicable<float>(const Operand &);

// the widths at which variant 0 takes the team kernel on this matrix (fp64): from its class's threshold on, and a full half-piece tile
static bool team2_width(const MatrixTraits &t, int n)
{
    return n >= t.team2_min_n || (t.team2_min_n == TEAM2_MIN_N && n >= TEAM2_HALF_FULL_LO && n <= TEAM2_HALF_FULL_HI);
}

int resolve_f64(const MatrixTraits &t, const Operand &op, int variant, bool team2r_refused, const Knobs &k)
{
    const int n = op.n;
    const bool rows = t.nnz > 0 && t.nrow >= 8;
    int v = (variant == 0) ? t.auto_variant : variant;
    // auto: from TEAM2_MIN_N columns on the LDS-sharing team kernel wherever teams share columns (against the best
    // other variant on the pwtk / shell / fem3d stand-ins: n = 128: 1.00 / 0.81 / 0.73 of its time, n = 256: 0.85 /
    // 0.65 / 0.63; at n = 96 -- a tile of 128 columns three quarters used -- 1.17 / 1.00 / 0.94, at n = 32 1.6 x)
    if (variant == 0 && t.team2_pays && team2_width(t, n) && team2_applicable<double>(op)) v = 5;
    // (an explicit 5 or 7 that does not apply falls back to the row-panel kernel, and that to the CSR kernel: 5 -> 3 -> 1)
    const int panel_or_csr = panel_applicable(op) && t.nnz > 0 ? 3 : 1;
    if (v == 5) return team2_applicable<double>(op) && rows ? 5 : panel_or_csr;
    // narrow operands (24 <= n <= 64) whose R = 8 panels are mostly holes: the team kernel whose lane groups own rows (variant 7;
    // CRPSPMM_TEAM2R=0|1 forces).  Once its streams were refused (past their 32-bit offsets), variant 0 goes on with the
    // row-panel kernels, for good: the create-time choice, or 3 where the knob forces the row-owner kernel.
    const int G = n <= 32 ? 4 : 2;
    const bool team2r_auto = k.team2r >= 0 ? k.team2r != 0 : (t.panels_sparse && !team2r_refused);
    if (variant == 0 && t.team2_pays && team2r_auto && n <= 64 && rows && team2r_applicable(op, G)) v = team2r_refused ? 3 : 7;
    if (v == 7) return team2r_applicable(op, G) && rows ? 7 : panel_or_csr;
    if (v >= 2 && (!panel_applicable(op) || t.nnz == 0)) v = 1;   // narrow / unaligned operands
    return v;
}

int resolve_f32(const MatrixTraits &t, const Operand &op, int variant)
{
    const int min_n = t.panels_sparse ? TEAM2_MIN_N_F32_SPARSE : TEAM2_MIN_N_F32;
    const bool team = (variant == 5 || (variant == 0 && t.team2_pays && op.n >= min_n)) && t.nnz > 0 && t.nrow >= 8 &&
                      team2_applicable<float>(op);
    return team ? 5 : 1;
}

bool team2_compact(double fill, bool for_f32)
{
    // Value blocks: compact (only the values that exist), or 8 per part -- the kernel instance for full groups decodes no value position
    // (two instructions per part and three per round fewer) and streams up to 64 % more value bytes.  Mostly-hole panels (under 40 % of the
    // (row, entry) pairs exist: KKT systems) are always compact: nlpkkt stand-in 1.91 against 2.05 ms, 13 GB smaller at nlpkkt240 size.  On
    // filled panels it used to be a wash that full groups won by 1 %; since the round-4 loop (fewer scalar instructions per round) the
    // kernels run at the speed of their memory schedule and the bytes decide -- fp64, compact against full, same box
    // (profiles/r04_compact_ab.txt): pwtk stand-in n = 256 0.2724 / 0.2776 ms, n = 1024 1.077 / 1.104, n = 128 0.1687 / 0.1697, shell n = 128
    // 0.1432 / 0.1481, n = 64 0.0986 / 0.1024, Queen stand-in n = 256 0.7917 / 0.8066, n = 64 0.3472 / 0.3581, n = 1024 3.170 / 3.161.  In
    // fp32 a value is 4 bytes and the decoding costs the same: full groups stay 0.3 - 0.8 % ahead (Queen stand-in n = 128 / 256 / 1024), so a
    // format that is first built for the fp32 path keeps them.  CRPSPMM_TEAM2_COMPACT=0|1 forces.
    return knobs().team2_compact >= 0 ? knobs().team2_compact != 0 : (fill < 0.4 || !for_f32);
}

}  // namespace crp
