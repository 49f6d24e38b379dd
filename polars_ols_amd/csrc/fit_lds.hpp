// fit_lds.hpp -- the dynamic-LDS layouts of the one-wave solve kernels of K14, K16, K17 and K18 and of K19's table kernel: offsets in doubles and their total.  Each
// is ONE function, called by the kernel (its offsets) and by the launcher (its total), so the two cannot drift apart.  Plain C++ when
// compiled without HIP: tests/carve_check.cpp checks order, disjointness and the totals on the CPU.
#pragma once

#ifdef __HIPCC__
#define FIT_HD __host__ __device__
#else
#define FIT_HD
#endif

namespace pols {

// K14 (k14_iv.hip): kx regressors, L instruments (both incl. the intercept), T staged columns
struct K14Lds { int Gs, A, d0, B, Gm2, A2, rhs2, d02, Ri, tmp, total; };
FIT_HD static inline K14Lds k14_lds(int kx, int L, int T) {
    K14Lds o;
    int at = 0;
    o.Gs = at;   at += (T + 1) * (T + 2) / 2 + 1;      // the summed moments (packed upper triangle), then n
    o.A = at;    at += L * (L + 1);                    // Z~'Z~, then its factor R in the lower triangle
    o.d0 = at;   at += L;
    o.B = at;    at += L * (kx + 1);                   // [C | Z~'y~] -> [Q | r] -> Pi in the first kx columns
    o.Gm2 = at;  at += (kx + 1) * (kx + 2) / 2;        // packed [M, Q'r; ., r'r]
    o.A2 = at;   at += kx * (kx + 1);                  // M, then its factor
    o.rhs2 = at; at += kx;                             // Q'r -> b
    o.d02 = at;  at += kx;
    o.Ri = at;   at += kx * kx;                        // the inverse of M's factor
    o.tmp = at;  at += L;                              // the Sargan terms
    o.total = at;
    return o;
}

// K16 (k16_absorb.hip) and K17 (k17_absorb2.hip), k columns: the summed partials -- `tail` doubles follow the packed triangle of
// [X~ | y~]'[X~ | y~] and begin with the k raw second moments T_jj -- then the work of k16_solve_core
struct AbsorbLds { int Gs, T, A, d0, rhs, Ri, total; };
FIT_HD static inline AbsorbLds absorb_lds(int k, int tail) {
    const int ne = (k + 1) * (k + 2) / 2;
    AbsorbLds o;
    int at = 0;
    o.Gs = at;  at += ne;                 // the packed upper triangle
    o.T = at;   at += tail;               // T_jj, then what else the entry sums per item
    o.A = at;   at += k * (k + 1);        // X~'X~, then its factor
    o.d0 = at;  at += k;
    o.rhs = at; at += k;                  // X~'y~ -> b
    o.Ri = at;  at += k * k;              // the inverse of the factor
    o.total = at;
    return o;
}
FIT_HD static inline AbsorbLds k16_lds(int k) { return absorb_lds(k, k + 1); }   // T_jj, then n
FIT_HD static inline AbsorbLds k17_lds(int k) { return absorb_lds(k, k); }       // T_jj (from the demean launch's records)

// K18 (k18_glsar.hip): kt columns incl. the intercept
struct K18Lds { int Ss, Cs, z1, zn, Gm, A, rhs, d0, b0, vv, tn, td, Ri, ij, total; };
FIT_HD static inline K18Lds k18_lds(int kt) {
    const int TT = kt + 1, ne = TT * (TT + 1) / 2;
    K18Lds o;
    int at = 0;
    o.Ss = at;  at += ne;                 // the summed S (packed upper triangle)
    o.Cs = at;  at += TT * TT;            // the summed C, right behind S as in the partials: the kernel sums both as one run
    o.z1 = at;  at += TT;
    o.zn = at;  at += TT;
    o.Gm = at;  at += ne;                 // A(rho), packed as fit_chol_solve reads it
    o.A = at;   at += kt * (kt + 1);      // its X-block, then the factor
    o.rhs = at; at += kt;                 // the y-column -> b
    o.d0 = at;  at += kt;
    o.b0 = at;  at += kt;                 // b at rho = 0
    o.vv = at;  at += TT;                 // v = (-b, 1)
    o.tn = at;  at += TT;                 // lane i's term of v'C v ...
    o.td = at;  at += TT;                 // ... and of v'S_n v
    o.Ri = at;  at += kt * kt;            // the inverse of the last factor
    o.ij = at;  at += (ne + 1) / 2;       // (i, j) of every packed entry, as int32
    o.total = at;
    return o;
}

// K19 (k19_random_effects.hip), the table kernel: k features, kc = k + intercept columns, `rows` rows of K16's category table held
// resident (0: the global route reads the table where it lies).  nz = kc + 1 counts the ybar column of the packed triangles.
struct K19Lds { int tab, q, part, Gw, Gs, T, A, d0, rhs, Ri, Minv, bb, D, dz, dv, red, sc, total; };
FIT_HD static inline K19Lds k19_lds(int k, int kc, int rows) {
    const int nz = kc + 1, ne = nz * (nz + 1) / 2, nw = (k + 1) * (k + 2) / 2;
    K19Lds o;
    int at = 0;
    o.tab = at;  at += rows * (k + 3);        // the group's rows of the category table, as K16 lays them out
    o.q = at;    at += rows;                  // q_c = T_c (1 - theta_c)^2
    o.part = at; at += ne > 256 ? ne : 256;   // the partitions of a table sum before they meet
    o.Gw = at;   at += nw + k + 1;            // the within moments summed over the items: the triangle, T_jj, n
    o.Gs = at;   at += ne;                    // packed [B g; g' .], later [M v; v' .]
    o.T = at;    at += kc;                    // what the pivots of M are held against
    o.A = at;    at += kc * (kc + 1);         // the matrix, then its factor
    o.d0 = at;   at += kc;
    o.rhs = at;  at += kc;                    // the right-hand side -> the coefficients
    o.Ri = at;   at += kc * kc;               // the inverse of the factor
    o.Minv = at; at += kc * kc;               // M^-1
    o.bb = at;   at += kc;                    // the between coefficients
    o.D = at;    at += k * (k + 1);           // Hausman's D, then its factor
    o.dz = at;   at += k;                     // zeros: its pivots are held against 0
    o.dv = at;   at += k;                     // b_w - b -> L^-1 (b_w - b)
    o.red = at;  at += 4;                     // fit_block_sum
    o.sc = at;   at += 4;                     // flags of wave 0 for the others
    o.total = at;
    return o;
}
// the rows of the table a resident workgroup can hold under `budget` bytes of LDS (<= 0: none)
FIT_HD static inline long long k19_resident_rows(int k, int kc, long long budget) {
    const long long fixed = k19_lds(k, kc, 0).total;
    return (budget / 8 - fixed) / (k + 4);
}

}  // namespace pols
