// fit_tile.inl -- the device primitives shared by the per-group fit kernels K10 .. K14 and K16 (k10_ridge_path.hip, k11_rlm.hip,
// k12_enet_cv.hip, k13_glm.hip, k14_iv.hip, k16_absorb.hip): the workgroup's item and its 256-row tile grid, the tile load and K10's staging policy, the packed upper
// triangle of a Gram matrix spread over 256 threads with its accumulate and reduce steps, a block sum and the walk of a prediction
// pass.  Everything sums in a fixed order and uses no floating-point atomics.  The one-wave Cholesky solve is in fit_solve.inl, the
// host side of a launch in fit_launch.hpp.
#pragma once
#include "common.hpp"

namespace pols {

constexpr int FIT_TILE = 256;         // rows of a tile: one per thread
constexpr int FIT_TS = 257;           // column stride of a tile whose columns are read across threads (odd: conflict-free across columns)
constexpr double FIT_DBL_MAX = 1.79769313486231570815e308;
constexpr double FIT_EPS = 2.220446049250313e-16;

__device__ __forceinline__ double fit_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---------------------------------------------------------------- the item and its tiles
// the first row of the tile grid of an item that starts at row s: the tiles sit on the columns' 16-byte grid
template <typename T>
__host__ __device__ inline int64_t fit_base(const int64_t s) { return s & ~(int64_t)(Vec16<T>::N - 1); }
// the 256-row tiles of the item [s, e)
template <typename T>
__host__ __device__ inline int64_t fit_tiles(const int64_t s, const int64_t e) { return e > s ? (e - fit_base<T>(s) + FIT_TILE - 1) / FIT_TILE : 0; }

// the item of this workgroup: its group, its rows, the first row of its tile grid and its tiles.  Args: offs, seg_offs, seg_map.
template <typename T, typename Args>
__device__ __forceinline__ void fit_item(const Args &a, int64_t &g, int64_t &s, int64_t &e, int64_t &base, int64_t &ntiles) {
    const int64_t sgi = blockIdx.x;
    g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    s = a.seg_offs ? a.seg_offs[sgi] : a.offs[g];
    e = a.seg_offs ? a.seg_offs[sgi + 1] : a.offs[g + 1];
    base = fit_base<T>(s);
    ntiles = fit_tiles<T>(s, e);
}

// ---------------------------------------------------------------- the packed upper triangle
// index of entry (i, j), i <= j, in the packed upper triangle of an nz x nz matrix (row i holds the entries (i, i) .. (i, nz - 1))
__host__ __device__ inline int tri_index(const int i, const int j, const int nz) { return i * nz - i * (i - 1) / 2 + (j - i); }
// ... and the entry (i, j) at index en
__device__ __forceinline__ void tri_unpack(const int en, const int nz, int &i, int &j) {
    int t = en;
    i = 0;
    while (t >= nz - i) { t -= nz - i; ++i; }
    j = i + t;
}

// the entries of a symmetric nz x nz cross-product that thread `tid` of 256 accumulates: (ei, ej) of slot q, ei <= ej, in the order of
// the packed upper triangle.  With ne = nz (nz + 1) / 2 < 256 entries `parts` = 256 / ne row partitions share an entry (slot 0 only,
// this thread's partition is `part`), beyond that up to three entries per thread (parts = 1).
struct TriSpread {
    int ei[3], ej[3];
    bool on[3];
    int ne, parts, part;
};
__device__ __forceinline__ TriSpread tri_spread(const int nz, const int tid) {
    TriSpread sp;
    const int ne = nz * (nz + 1) / 2;
    sp.ne = ne;
    sp.parts = ne < 256 ? 256 / ne : 1;
    sp.part = sp.parts > 1 ? tid / ne : 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int en = sp.parts > 1 ? tid - sp.part * ne : tid + 256 * q;
        sp.on[q] = sp.parts > 1 ? (q == 0 && sp.part < sp.parts) : en < ne;
        tri_unpack(sp.on[q] ? en : 0, nz, sp.ei[q], sp.ej[q]);
    }
    return sp;
}

// acc[q] += the sum of c_i[r] c_j[r] over this thread's rows r = r0 + part, r0 + part + parts, ... below r1; column c of `cols` starts
// at cols + c ts.  The loop is left to the compiler: an unroll by 4, as K11's own loops ask for, would cost the Gram launches of K10,
// K12 and K14 occupancy (52 -> 87 VGPRs in k10_gram_kernel).
__device__ __forceinline__ void tri_accumulate(const TriSpread &sp, double (&acc)[3], const double *cols, const int ts, const int r0, const int r1) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (!sp.on[q]) continue;
        const double *ci = cols + (size_t)sp.ei[q] * ts, *cj = cols + (size_t)sp.ej[q] * ts;
        double v = acc[q];
        for (int r = r0 + sp.part; r < r1; r += sp.parts) v = fma(ci[r], cj[r], v);
        acc[q] = v;
    }
}

// acc -> out[0 .. ne) (LDS or global), the row partitions summed in partition order; acc is zeroed.  gp: 256 doubles of LDS.  Ends on a
// barrier.
__device__ __forceinline__ void tri_reduce(const TriSpread &sp, double (&acc)[3], double *gp, double *out) {
    const int tid = threadIdx.x, ne = sp.ne;
    if (sp.parts > 1) {
        if (sp.on[0]) gp[tid] = acc[0];                            // (tid = part ne + entry)
        __syncthreads();
        if (tid < ne) {
            double v = 0.0;
            for (int p = 0; p < sp.parts; ++p) v += gp[p * ne + tid];
            out[tid] = v;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (sp.on[q]) out[tid + 256 * q] = acc[q];
    }
    acc[0] = acc[1] = acc[2] = 0.0;
    __syncthreads();
}

// the sum of v over the 256 threads in a fixed order, in every thread; red: four doubles.  Two barriers.
__device__ __forceinline__ double fit_block_sum(double v, double *red, const int lane, const int wv) {
    v = wave_sum_row3(v);
    if (lane == 63) red[wv] = v;
    __syncthreads();
    const double r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------- the tile
// rows [t0, t0 + 256) of the item [s, e) into xs (column stride ts) as f64: 16-byte loads on the columns' 16-byte grid (column q of the
// tile is one wave's work, every load of a lane issued before the first use), then the thread of a row applies the null policy and
// sqrt(w).  Features 0 .. ku - 1, the ones column at ku (kt > ku), y~ at kt; column kt + 1 holds the raw weights in between.  Args:
// RidgeCvArgs, RlmArgs, EnetCvArgs, IvArgs or AbsorbArgs -- y, w, x, n_rows, valid, null_policy, k_user, kt.  Returns whether this thread's row
// (t0 + tid) is a fitted row.  Ends on a barrier.
template <typename T, bool STREAM, typename Args>
__device__ __forceinline__ bool fit_stage(const Args &a, const int64_t s, const int64_t e, const int64_t t0, double *xs, const int ts) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Vec16<T>::N, CH = FIT_TILE / VEC;
    const int tid = threadIdx.x, ku = a.k_user, kt = a.kt;
    const int nld = ku + 1 + (a.w ? 1 : 0);
    for (int p = tid; p < nld * CH; p += 256) {
        const int q = __builtin_amdgcn_readfirstlane(p / CH), ch = p - q * CH;     // (CH is 64 or 128: a wave stays inside one column)
        const int64_t row0 = t0 + (int64_t)ch * VEC;
        if (row0 >= e) continue;
        const void *col = q == ku ? a.y : a.w;                       // (a run-time index into the kernel arguments would put them in scratch)
#pragma unroll
        for (int j = 0; j < POLS_MAX_FEATURES; ++j) col = (j == q && j < ku) ? a.x[j] : col;
        const T *src = static_cast<const T *>(col);
        double *dst = xs + (size_t)(q < ku ? q : (q == ku ? kt : kt + 1)) * ts + ch * VEC;
        if (row0 + VEC <= a.n_rows) {                              // (the columns are 16-byte aligned and row0 sits on their grid)
            const V v = STREAM ? load_stream(reinterpret_cast<const V *>(src + row0)) : *reinterpret_cast<const V *>(src + row0);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = (double)vget<T>(v, i);
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = row0 + i < a.n_rows ? (double)src[row0 + i] : 0.0;
        }
    }
    __syncthreads();
    const int64_t row = t0 + tid;
    const int pol = a.null_policy;
    bool fit = row >= s && row < e;
    if (fit && pol != POLS_NULL_IGNORE) {                          // which rows leave the fit (compute_is_valid_mask, ex.rs:201-228)
        if (a.valid && null_checks_y(pol)) fit = a.valid[row] != 0;
        if (null_checks_y(pol)) { const double v = xs[(size_t)kt * ts + tid]; fit = fit && v == v; }
        if (null_checks_x(pol))
            for (int c = 0; c < ku; ++c) { const double v = xs[(size_t)c * ts + tid]; fit = fit && v == v; }
    }
    const double sw = !fit ? 0.0 : (a.w ? sqrt(xs[(size_t)(kt + 1) * ts + tid]) : 1.0);
    for (int c = 0; c < ku; ++c) {
        double v = xs[(size_t)c * ts + tid];
        if (pol != POLS_NULL_IGNORE && v != v) v = 0.0;           // handle_nulls (ex.rs:257-296)
        xs[(size_t)c * ts + tid] = fit ? v * sw : 0.0;
    }
    if (kt > ku) xs[(size_t)ku * ts + tid] = sw;
    {
        double v = xs[(size_t)kt * ts + tid];
        if (pol != POLS_NULL_IGNORE && v != v) v = 0.0;
        xs[(size_t)kt * ts + tid] = fit ? v * sw : 0.0;
    }
    __syncthreads();
    return fit;
}

// ---------------------------------------------------------------- the prediction pass
// the walk of a prediction launch over the item [s, e) whose tile grid starts at base: a lane owns 16 bytes of every column (streaming
// loads, all issued before the first use), sums  lin = icpt + sum_j fill(x_j) cg[j] [+ fill(add)]  in f64 (features and the additive
// column `add`, nullptr for none, zero-filled under every policy but "ignore") and hands every row to
//   row(lin, y, r, in, fit, o)   in: r is a row of the item; fit: false for a row that "drop" kept out of the fit (ex.rs:409-417);
// which fills o[k], the value of out[k] (NO of them, any may be nullptr) at row r.  Whole chunks inside the item go out as 16-byte streaming
// stores, the others row by row.  Args: y, x, n_rows, valid, null_policy, k_user.
template <typename T, int NO, typename Args, typename Row>
__device__ __forceinline__ void fit_predict_rows(const Args &a, const int64_t s, const int64_t e, const int64_t base, const double *cg,
                                                 const double icpt, const T *add, T *const (&out)[NO], Row &&row) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Vec16<T>::N;
    const int tid = threadIdx.x, ku = a.k_user, pol = a.null_policy;
    const T *yp = static_cast<const T *>(a.y);
    const int64_t nch = (e - base + VEC - 1) / VEC;
    for (int64_t c = tid; c < nch; c += 256) {
        const int64_t row0 = base + c * VEC;
        const bool whole = row0 + VEC <= a.n_rows;                 // (else: the one chunk across the end of the columns, row by row)
        const bool full = whole && row0 >= s && row0 + VEC <= e;
        double p[VEC];
        bool nullx[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) { p[v] = icpt; nullx[v] = false; }
#pragma unroll
        for (int j = 0; j <= POLS_MAX_FEATURES; ++j) {             // (the last turn: the additive column)
            const bool off = j == POLS_MAX_FEATURES;
            if (off ? add != nullptr : j < ku) {
                const T *xp = off ? add : static_cast<const T *>(a.x[j < POLS_MAX_FEATURES ? j : 0]);
                const double cj = off ? 1.0 : cg[j < POLS_MAX_FEATURES ? j : 0];
                T xv[VEC];
                if (whole) {
                    const V ld = load_stream(reinterpret_cast<const V *>(xp + row0));
#pragma unroll
                    for (int v = 0; v < VEC; ++v) xv[v] = vget<T>(ld, v);
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) xv[v] = row0 + v < a.n_rows ? xp[row0 + v] : T(0);
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    nullx[v] = nullx[v] || xv[v] != xv[v];
                    if (off) p[v] += (double)null_fill<T>(pol, xv[v]);
                    else p[v] = fma((double)null_fill<T>(pol, xv[v]), cj, p[v]);
                }
            }
        }
        T ov[NO][VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int64_t r = row0 + v;
            const bool in = r >= s && r < e;
            const T yv = in ? yp[r] : T(0);
            const bool fit = pol != POLS_NULL_DROP || (!(a.valid && in && !a.valid[r]) && yv == yv && !nullx[v]);
            double o[NO] = {};
            row(p[v], (double)yv, r, in, fit, o);
#pragma unroll
            for (int k = 0; k < NO; ++k) ov[k][v] = (T)o[k];
        }
#pragma unroll
        for (int k = 0; k < NO; ++k) {
            if (!out[k]) continue;
            if (full) {
                if constexpr (VEC == 4) store_stream(reinterpret_cast<V *>(out[k] + row0), V{ov[k][0], ov[k][1], ov[k][2], ov[k][3]});
                else store_stream(reinterpret_cast<V *>(out[k] + row0), V{ov[k][0], ov[k][1]});
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const int64_t r = row0 + v;
                    if (r >= s && r < e) out[k][r] = ov[k][v];
                }
            }
        }
    }
}

}  // namespace pols
