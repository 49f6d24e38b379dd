// k7c_cluster.hip -- K7c: cluster-robust standard errors of mode="statistics" (pols_least_squares_statistics_cluster).
//
// Per group, on the rows the null policy leaves, scaled by sqrt(w), the ones column last (as K7 / K7r):
//   A = X'X + lambda I,  b = A^-1 X'y,  e_i = y_i - x_i'b,  u_i = e_i x_i;
//   one clustering c: s_c = sum_{i in c} u_i,  z_c = A^-1 s_c,  sum_c z_cj^2 (only diag V: never the kt x kt meat);
//   one-way V_jj = q_A S_A,  two-way V_jj = q_A S_A + q_B S_B - q_AB S_AB,  q = G / (G - 1) (N - 1) / df (use_correction) or 1;
//   se_j = sqrt(V_jj), t_j = b_j / se_j, p_j two-sided Student-t with G - 1 (two-way: min(G_A, G_B) - 1) degrees of freedom.
// The launches:
//   prepare  K7r's prepare kernel: A^-1, b, trace(A^-1), ok per group;
//   runs     per clustering (A; two-way also B and AB) the positions of every group in ascending id order.  A probe checks whether the
//            ids are already non-decreasing inside every group (comparisons across group starts ignored): then nothing moves and a
//            cluster starts where the id changes or a group starts.  Otherwise stable LSD radix passes (K9's rocPRIM sort, k9_sort.hpp)
//            on the row iota -- by the id (for AB first by b, then by a), then by the group index -- give the order, each pass on only
//            the bits of its key's range;
//   scores   one 256-thread workgroup per segment of a long group (ensure_segments) or per group: 256-position tiles of u staged in
//            LDS through the order, run starts compacted by ballot, the run pieces summed in frame order (kt FMAs per row for e and u);
//            a run that starts and ends inside the segment gets z = A^-1 s (A^-1 in LDS) and adds z^2 to the segment's partial.  A run
//            cut by a segment end is not squared: the segment writes its piece -- H, the run it starts inside of, T, the run that
//            goes on into the next segment (a run over the whole segment is H alone);
//   finish   one workgroup per group: segments in chunks of 256 / kt, thread (segment, column): the partial, and where a segment's head
//            closes a run, T of the segment the run started in + H of every segment after it up to here, in segment order, then z^2;
//            the chunks meet in a fixed order -- the same sums whatever ran first, and no floating-point atomics anywhere;
//   output   one wave per group: q per clustering, V, se / t / p, the cluster counts.
// Everything is f64, like K7.
#include "k7c_cluster.hpp"
#include "k7r_robust.hpp"
#include "k9_sort.hpp"

#include <algorithm>

namespace pols {

// position i of the clustering: the row behind it, and whether a cluster starts there (a group start, or another id than position i - 1)
__device__ __forceinline__ int64_t k7c_row(const ClusterWay &w, int64_t i) { return w.order ? (int64_t)w.order[i] : i; }
__device__ __forceinline__ bool k7c_starts(const ClusterWay &w, int64_t gs, int64_t i) {
    if (i == gs) return true;
    const int64_t r = k7c_row(w, i), q = k7c_row(w, i - 1);
    return w.k1[r] != w.k1[q] || (w.k2 && w.k2[r] != w.k2[q]);
}

template <typename T>
__global__ void __launch_bounds__(256) k7c_scores_kernel(const ClusterArgs c, const ClusterWay w) {
    extern __shared__ double lds[];
    __shared__ int pos[K7C_TILE + 1];                              // the tile's piece starts, then its row count
    __shared__ int wcnt[4];
    __shared__ int tile_cont0, tile_closed;
    const StatsArgs &a = c.s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = a.kt, ku = a.k_user, E = kt * kt;
    const int64_t sgi = blockIdx.x, g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    const int64_t gs = a.offs[g], ge = a.offs[g + 1];
    const int64_t s = a.seg_offs ? a.seg_offs[sgi] : gs, e = a.seg_offs ? a.seg_offs[sgi + 1] : ge;
    // LDS: [A^-1] [b] [carry: the open piece of the previous tile] [U: u of the tile's rows, then z^2 of its closed runs] [PS: piece sums]
    double *Ainv = lds, *binv = Ainv + E, *carry = binv + kt, *U = carry + kt, *PS = U + (size_t)K7C_TILE * kt;
    const double *P = c.prep + (size_t)g * k7r_prep_stride(kt);
    for (int q = tid; q < E; q += 256) Ainv[q] = P[q];
    if (tid < kt) { binv[tid] = P[E + tid]; carry[tid] = 0.0; }
    const T *yp = static_cast<const T *>(a.y), *wp = static_cast<const T *>(a.w);
    double *out = w.part + (size_t)sgi * k7c_part_stride(kt);
    const bool head_open = s < e && s != gs && !k7c_starts(w, gs, s);   // the segment starts inside a run of an earlier segment
    bool carry_head = head_open;                                   // the open piece belongs to that run
    bool head_closes = false;
    double acc = 0.0;                                              // thread j < kt: sum z_j^2 of the runs inside the segment
    int64_t cnt = 0;
    __syncthreads();
    for (int64_t tb = s; tb < e; tb += K7C_TILE) {
        const int nr = (int)std::min<int64_t>(K7C_TILE, e - tb);
        bool st = false;
        if (tid < nr) {
            const int64_t i = tb + tid, r = k7c_row(w, i);
            st = k7c_starts(w, gs, i);
            const double sw = wp ? sqrt((double)wp[r]) : 1.0;
            double *ur = U + (size_t)tid * kt;
            double pr = 0.0;
            for (int j = 0; j < kt; ++j) {
                const double x = ((j < ku) ? (double)static_cast<const T *>(a.x[j])[r] : 1.0) * sw;
                ur[j] = x;
                pr = fma(x, binv[j], pr);
            }
            const double f = (double)yp[r] * sw - pr;
            for (int j = 0; j < kt; ++j) ur[j] *= f;
        }
        const unsigned long long m = __ballot(st);
        if (lane == 0) wcnt[wv] = __popcll(m);
        if (tid == 0) {
            tile_cont0 = st ? 0 : 1;                               // the tile's first piece continues the carry
            const int64_t ie = tb + nr;
            tile_closed = (ie == ge || k7c_starts(w, gs, ie)) ? 1 : 0;   // a run starts right behind the tile: its last piece is whole
        }
        __syncthreads();
        const int cont0 = tile_cont0;
        int before = 0, nst = 0;
        for (int q = 0; q < 4; ++q) { before += q < wv ? wcnt[q] : 0; nst += wcnt[q]; }
        if (st) pos[cont0 + before + __popcll(m & ((1ull << lane) - 1ull))] = tid;
        const int np = cont0 + nst;
        if (tid == 0) { if (cont0) pos[0] = 0; pos[np] = nr; }
        __syncthreads();
        for (int q = tid; q < np * kt; q += 256) {                 // piece k, column j: its rows in frame order
            const int k = q / kt, j = q - k * kt;
            double v = 0.0;
            for (int p = pos[k]; p < pos[k + 1]; ++p) v += U[(size_t)p * kt + j];
            PS[q] = (k == 0 && cont0) ? carry[j] + v : v;
        }
        __syncthreads();
        const bool closed = tile_closed != 0;
        const int nclosed = closed ? np : np - 1;
        const bool head0 = cont0 && carry_head;                    // piece 0 ends (or goes on with) the run the segment started inside of
        for (int q = tid; q < nclosed * kt; q += 256) {            // z = A^-1 s of every run that ends in the tile, z^2 over U
            const int k = q / kt, j = q - k * kt;
            double zz = 0.0;
            if (!(k == 0 && head0)) {
                const double *sk = PS + (size_t)k * kt;
                double z = 0.0;
                for (int mm = 0; mm < kt; ++mm) z = fma(Ainv[j * kt + mm], sk[mm], z);
                zz = z * z;
            }
            U[q] = zz;
        }
        if (head0 && nclosed > 0 && tid < kt) out[kt + tid] = PS[tid];                 // H: closed in this segment, squared by the finish
        if (nclosed < np && tid < kt) carry[tid] = PS[(size_t)(np - 1) * kt + tid];
        __syncthreads();
        if (tid < kt)
            for (int k = 0; k < nclosed; ++k) acc += U[(size_t)k * kt + tid];
        head_closes = head_closes || (head0 && nclosed > 0);
        carry_head = nclosed < np && np == 1 && head0;
        cnt += nst;
        __syncthreads();
    }
    // the segment ends inside a run: its open piece goes to the finish, as H (the whole segment is one run's middle) or T
    const bool open_end = s < e && !(e == ge || k7c_starts(w, gs, e));
    if (open_end && tid < kt) out[(carry_head ? kt : 2 * kt) + tid] = carry[tid];
    if (tid < kt) out[tid] = acc;
    if (tid == 0) {
        out[3 * kt] = (double)cnt;
        out[3 * kt + 1] = head_open ? 1.0 : 0.0;
        out[3 * kt + 2] = head_closes ? 1.0 : 0.0;
        out[3 * kt + 3] = (open_end && !carry_head) ? 1.0 : 0.0;
    }
}

__global__ void __launch_bounds__(256) k7c_finish_kernel(const ClusterArgs c, const ClusterWay w) {
    __shared__ double Ainv[K7_KMAX * K7_KMAX], cur[256], zz[256], cntv[256];
    const StatsArgs &a = c.s;
    const int tid = threadIdx.x, kt = a.kt, E = kt * kt;
    const int64_t g = blockIdx.x;
    const int64_t v0 = a.seg_offs ? a.seg_first[g] : g, v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
    const double *P = c.prep + (size_t)g * k7r_prep_stride(kt);
    for (int q = tid; q < E; q += 256) Ainv[q] = P[q];
    const size_t ps = k7c_part_stride(kt);
    const int C = 256 / kt, ei = tid / kt, j = tid - ei * kt;     // thread (segment ei of the chunk, column j)
    const bool slot = ei < C;
    double acc = 0.0, G = 0.0;
    __syncthreads();
    for (int64_t c0 = v0; c0 < v1; c0 += C) {
        const int64_t v = c0 + ei;
        const bool live = slot && v < v1;
        double val = 0.0;
        bool closes = false;
        if (live) {
            const double *pv = w.part + (size_t)v * ps;
            val = pv[j];
            closes = pv[3 * kt + 2] != 0.0;
            if (closes) {                                          // the run began in the last segment before v with an open tail
                int64_t u = v - 1;
                while (u > v0 && w.part[(size_t)u * ps + 3 * kt + 3] == 0.0) --u;
                double sum = w.part[(size_t)u * ps + 2 * kt + j];
                for (int64_t x = u + 1; x <= v; ++x) sum += w.part[(size_t)x * ps + kt + j];
                cur[tid] = sum;
            }
            if (j == 0) cntv[ei] = pv[3 * kt];
        } else if (slot && j == 0) {
            cntv[ei] = 0.0;
        }
        __syncthreads();
        if (closes) {
            double z = 0.0;
            for (int mm = 0; mm < kt; ++mm) z = fma(Ainv[j * kt + mm], cur[ei * kt + mm], z);
            val += z * z;
        }
        if (slot) zz[tid] = val;
        __syncthreads();
        if (tid < kt)
            for (int q = 0; q < C; ++q) acc += zz[q * kt + tid];
        if (tid == 0)
            for (int q = 0; q < C; ++q) G += cntv[q];
        __syncthreads();
    }
    double *o = w.sums + (size_t)g * (kt + 1);
    if (tid < kt) o[tid] = acc;
    if (tid == 0) o[kt] = G;
}

__global__ void __launch_bounds__(64) k7c_output_kernel(const ClusterArgs c, const double *sums) {
    const StatsArgs &a = c.s;
    const int lane = threadIdx.x, kt = a.kt, E = kt * kt;
    const int64_t g = blockIdx.x;
    const double *P = c.prep + (size_t)g * k7r_prep_stride(kt);
    const double nn = (double)(a.offs[g + 1] - a.offs[g]), trace = P[E + kt];
    const double df = (a.lambda > 0.0) ? nn - trace : nn - (double)kt;          // K7's df
    const bool ok = P[E + kt + 1] != 0.0;
    const size_t gst = (size_t)a.n_groups * (kt + 1);
    const double *sa = sums + (size_t)g * (kt + 1), *sb = sa + gst, *sab = sb + gst;
    const bool two = c.ways == 2;
    const double GA = sa[kt], GB = two ? sb[kt] : GA, GAB = two ? sab[kt] : GA;
    auto qf = [&](double G) { return c.use_correction ? G / (G - 1.0) * (nn - 1.0) / df : 1.0; };
    const double gmin = std::min(GA, GB);
    const bool good = ok && gmin >= 2.0 && !(c.use_correction && !(df > 0.0));
    if (lane < kt) {
        double v = qf(GA) * sa[lane];
        if (two) v = v + qf(GB) * sb[lane] - qf(GAB) * sab[lane];
        const double nanv = __longlong_as_double(0x7ff8000000000000LL);
        double se = nanv, tv = nanv, pv = nanv;
        if (good && v >= 0.0) {
            const double dfp = gmin - 1.0;                         // Stata / statsmodels: G - 1, not K7's df
            se = sqrt(v);
            tv = P[E + lane] / se;
            pv = (tv != tv) ? nanv : k7_betai(0.5 * dfp, 0.5, dfp / (dfp + tv * tv));
        }
        if (a.se) a.se[g * kt + lane] = se;
        if (a.tv) a.tv[g * kt + lane] = tv;
        if (a.pv) a.pv[g * kt + lane] = pv;
    }
    if (c.n_clusters && lane == 0) {
        if (two) { c.n_clusters[2 * g] = (int64_t)GA; c.n_clusters[2 * g + 1] = (int64_t)GB; }
        else c.n_clusters[g] = (int64_t)GA;
    }
}

// ---- runs: probe, row -> group, radix keys
struct ClusterProbe { long long mn[2], mx[2]; int uns[3], pad; };   // per workgroup: id ranges, "decreasing inside a group" for A, B, AB

__device__ __forceinline__ bool k7c_group_start(const int64_t *offs, int64_t n_groups, int64_t i) {
    int64_t lo = 0, hi = n_groups;                                 // largest g with offs[g] <= i
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    return offs[lo] == i;
}

__global__ void __launch_bounds__(256) k7c_probe_kernel(const int64_t *__restrict__ a, const int64_t *__restrict__ b, const int64_t *offs,
                                                        int64_t n_groups, int64_t n, ClusterProbe *__restrict__ out) {
    __shared__ ClusterProbe red[4];
    long long mn0 = 0x7fffffffffffffffLL, mx0 = -0x7fffffffffffffffLL - 1, mn1 = mn0, mx1 = mx0;
    int u0 = 0, u1 = 0, u2 = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const long long ka = a[i];
        mn0 = ka < mn0 ? ka : mn0; mx0 = ka > mx0 ? ka : mx0;
        bool va = false, vb = false, vab = false;
        const long long pa = i ? a[i - 1] : ka;
        va = ka < pa;
        if (b) {
            const long long kb = b[i], pb = i ? b[i - 1] : kb;
            mn1 = kb < mn1 ? kb : mn1; mx1 = kb > mx1 ? kb : mx1;
            vb = kb < pb;
            vab = ka < pa || (ka == pa && kb < pb);
        }
        if ((va || vb || vab) && !k7c_group_start(offs, n_groups, i)) { u0 |= va; u1 |= vb; u2 |= vab; }
    }
    for (int off = 32; off; off >>= 1) {
        long long t;
        t = __shfl_xor(mn0, off); mn0 = t < mn0 ? t : mn0;
        t = __shfl_xor(mx0, off); mx0 = t > mx0 ? t : mx0;
        t = __shfl_xor(mn1, off); mn1 = t < mn1 ? t : mn1;
        t = __shfl_xor(mx1, off); mx1 = t > mx1 ? t : mx1;
        u0 |= __shfl_xor(u0, off); u1 |= __shfl_xor(u1, off); u2 |= __shfl_xor(u2, off);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        ClusterProbe r;
        r.mn[0] = mn0; r.mx[0] = mx0; r.mn[1] = mn1; r.mx[1] = mx1; r.uns[0] = u0; r.uns[1] = u1; r.uns[2] = u2; r.pad = 0;
        red[wv] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ClusterProbe r = red[0];
        for (int q = 1; q < 4; ++q)
            for (int h = 0; h < 2; ++h) {
                r.mn[h] = red[q].mn[h] < r.mn[h] ? red[q].mn[h] : r.mn[h];
                r.mx[h] = red[q].mx[h] > r.mx[h] ? red[q].mx[h] : r.mx[h];
            }
        for (int q = 1; q < 4; ++q)
            for (int h = 0; h < 3; ++h) r.uns[h] |= red[q].uns[h];
        out[blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(256) k7c_rowgroup_kernel(const int64_t *__restrict__ offs, int64_t n_groups, int64_t n, uint32_t *__restrict__ rg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    rg[i] = (uint32_t)lo;
}

// keys[i] = col[perm[i]] - mn on the radix bits, perm == nullptr: the row iota (also written to iota)
template <typename U, typename S>
__global__ void __launch_bounds__(256) k7c_key_kernel(const S *__restrict__ col, const uint32_t *__restrict__ perm, int64_t mn, int64_t n,
                                                      U *__restrict__ keys, uint32_t *__restrict__ iota) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = perm ? (int64_t)perm[i] : i;
    keys[i] = (U)((uint64_t)(int64_t)col[r] - (uint64_t)mn);
    if (!perm) iota[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k7c_gather_ids_kernel(const int32_t *__restrict__ src, int64_t n, const int64_t *__restrict__ a,
                                                             const int64_t *__restrict__ b, int64_t *__restrict__ oa, int64_t *__restrict__ ob) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = src[i];
    oa[i] = a[r];
    if (b) ob[i] = b[r];
}

static inline unsigned k7c_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
static int k7c_bits(uint64_t range) {
    int bits = 1;
    while (bits < 64 && (range >> bits)) ++bits;
    return bits;
}

int k7c_gather_ids_launch(pols_ctx *ctx, const int32_t *src, int64_t n, const int64_t *const *in, int64_t *const *out, int ways) {
    if (n == 0) return POLS_OK;
    hipLaunchKernelGGL(k7c_gather_ids_kernel, dim3(k7c_blocks(n)), dim3(256), 0, ctx->stream, src, n, in[0], ways > 1 ? in[1] : nullptr,
                       out[0], ways > 1 ? out[1] : nullptr);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

namespace {
struct SortBufs {
    void *keys_in, *keys_out, *tmp;
    uint32_t *vals[2], *rowgroup;
    size_t tmp_bytes;
    int64_t n;
};

// one stable radix pass: by col (rows through perm_in, nullptr = the iota) - mn on `bits` bits into perm_out
template <typename S>
int k7c_sort_pass(pols_ctx *ctx, const SortBufs &sb, const S *col, int64_t mn, int bits, const uint32_t *perm_in, uint32_t *perm_out) {
    const uint32_t *vin = perm_in ? perm_in : sb.vals[0];
    size_t t = sb.tmp_bytes;
    if (bits <= 32) {
        hipLaunchKernelGGL((k7c_key_kernel<uint32_t, S>), dim3(k7c_blocks(sb.n)), dim3(256), 0, ctx->stream, col, perm_in, mn, sb.n,
                           static_cast<uint32_t *>(sb.keys_in), sb.vals[0]);
        POLS_HIP(hipGetLastError());
        return k9_radix_sort_pairs<uint32_t>(ctx, sb.tmp, &t, static_cast<const uint32_t *>(sb.keys_in), static_cast<uint32_t *>(sb.keys_out),
                                             vin, perm_out, sb.n, bits);
    }
    hipLaunchKernelGGL((k7c_key_kernel<uint64_t, S>), dim3(k7c_blocks(sb.n)), dim3(256), 0, ctx->stream, col, perm_in, mn, sb.n,
                       static_cast<uint64_t *>(sb.keys_in), sb.vals[0]);
    POLS_HIP(hipGetLastError());
    return k9_radix_sort_pairs<uint64_t>(ctx, sb.tmp, &t, static_cast<const uint64_t *>(sb.keys_in), static_cast<uint64_t *>(sb.keys_out),
                                         vin, perm_out, sb.n, bits);
}

// The order builder of one call: the work areas of every clustering at once (growing one later would free memory a queued kernel
// still reads), then one probe for the ranges of both ids and the order of A, B and AB inside every group.
struct OrderPlan {
    SortBufs sb;
    uint32_t *order;
    ClusterProbe h;
};

// idb: the second id column, or nullptr
int k7c_order_prepare(pols_ctx *ctx, const int64_t *ida, const int64_t *idb, const int64_t *offs, int64_t G, int64_t n, OrderPlan *pl) {
    SortBufs &sb = pl->sb;
    ClusterProbe &h = pl->h;
    std::memset(&sb, 0, sizeof(sb));
    sb.n = n;
    pl->order = nullptr;
    std::memset(&h, 0, sizeof(h));
    if (n > 0) {
        size_t t32 = 0, t64 = 0;
        int rc = k9_radix_sort_pairs<uint32_t>(ctx, nullptr, &t32, nullptr, nullptr, nullptr, nullptr, n, 32);
        if (!rc) rc = k9_radix_sort_pairs<uint64_t>(ctx, nullptr, &t64, nullptr, nullptr, nullptr, nullptr, n, 64);
        if (rc) return rc;
        sb.tmp_bytes = round256(std::max(t32, t64));
        const unsigned nblk = std::min<unsigned>(k7c_blocks(n), (unsigned)std::max(ctx->num_cus, 1) * 8);
        const size_t kb = round256(sizeof(uint64_t) * (size_t)n), ib = round256(sizeof(uint32_t) * (size_t)n),
                     pb = round256(sizeof(ClusterProbe) * nblk);
        void *base = nullptr, *ob = nullptr;
        if ((rc = ensure_scratch(ctx, Work::ClusterSort, 2 * kb + 3 * ib + pb + sb.tmp_bytes, &base))) return rc;
        if ((rc = ensure_scratch(ctx, Work::ClusterOrder, ib, &ob))) return rc;
        char *p = static_cast<char *>(base);
        sb.keys_in = p; p += kb;
        sb.keys_out = p; p += kb;
        sb.vals[0] = reinterpret_cast<uint32_t *>(p); p += ib;
        sb.vals[1] = reinterpret_cast<uint32_t *>(p); p += ib;
        sb.rowgroup = reinterpret_cast<uint32_t *>(p); p += ib;
        ClusterProbe *dprobe = reinterpret_cast<ClusterProbe *>(p); p += pb;
        sb.tmp = p;
        pl->order = static_cast<uint32_t *>(ob);
        std::vector<ClusterProbe> part(nblk);
        hipLaunchKernelGGL(k7c_probe_kernel, dim3(nblk), dim3(256), 0, ctx->stream, ida, idb, offs, G, n, dprobe);
        POLS_HIP(hipGetLastError());
        POLS_HIP(hipMemcpyAsync(part.data(), dprobe, sizeof(ClusterProbe) * nblk, hipMemcpyDeviceToHost, ctx->stream));
        POLS_HIP(hipStreamSynchronize(ctx->stream));
        h = part[0];
        for (unsigned q = 1; q < nblk; ++q) {
            for (int w = 0; w < 2; ++w) { h.mn[w] = std::min(h.mn[w], part[q].mn[w]); h.mx[w] = std::max(h.mx[w], part[q].mx[w]); }
            for (int w = 0; w < 3; ++w) h.uns[w] |= part[q].uns[w];
        }
        if ((h.uns[0] || h.uns[1] || h.uns[2]) && G > 1) {
            hipLaunchKernelGGL(k7c_rowgroup_kernel, dim3(k7c_blocks(n)), dim3(256), 0, ctx->stream, offs, G, n, sb.rowgroup);
            POLS_HIP(hipGetLastError());
        }
    }
    return POLS_OK;
}

// the order of clustering wi (0: ids[0], 1: ids[1], 2: the pairs); *out = nullptr where the probe found its ids in order already
int k7c_order_way(pols_ctx *ctx, const OrderPlan &pl, const int64_t *const *ids, int wi, int64_t G, const uint32_t **out) {
    const SortBufs &sb = pl.sb;
    const ClusterProbe &h = pl.h;
    *out = nullptr;
    if (sb.n > 0 && h.uns[wi]) {
        // LSD: the least significant key first; every pass is stable, so ties keep the order of the passes before
        struct Pass { const int64_t *col; int64_t mn; int bits; };
        Pass passes[2];
        int np = 0;
        const int ia = wi == 1 ? 1 : 0;
        if (wi == 2) passes[np++] = {ids[1], h.mn[1], k7c_bits((uint64_t)h.mx[1] - (uint64_t)h.mn[1])};
        passes[np++] = {ids[ia], h.mn[ia], k7c_bits((uint64_t)h.mx[ia] - (uint64_t)h.mn[ia])};
        const int total = np + (G > 1 ? 1 : 0);
        const uint32_t *cur = nullptr;
        for (int q = 0; q < total; ++q) {
            uint32_t *dst = q == total - 1 ? pl.order : (cur == sb.vals[1] ? sb.vals[0] : sb.vals[1]);
            int rc = q < np ? k7c_sort_pass<int64_t>(ctx, sb, passes[q].col, passes[q].mn, passes[q].bits, cur, dst)
                            : k7c_sort_pass<uint32_t>(ctx, sb, sb.rowgroup, 0, k7c_bits((uint64_t)(G - 1)), cur, dst);
            if (rc) return rc;
            cur = dst;
        }
        *out = pl.order;
    }
    return POLS_OK;
}
}  // namespace

int k7c_order_launch(pols_ctx *ctx, const int64_t *ids, const int64_t *offs, int64_t n_groups, int64_t n_rows, const uint32_t **order) {
    OrderPlan pl;
    int rc = k7c_order_prepare(ctx, ids, nullptr, offs, n_groups, n_rows, &pl);
    if (rc) return rc;
    const int64_t *cols[2] = {ids, nullptr};
    return k7c_order_way(ctx, pl, cols, 0, n_groups, order);
}

constexpr size_t K7C_LDS_BUDGET = 160 * 1024 - 2048;   // dynamic LDS of the scores kernel (its static piece table aside)

static size_t k7c_lds_bytes(int kt) { return sizeof(double) * ((size_t)kt * kt + 2 * (size_t)kt + 2 * (size_t)K7C_TILE * kt); }

template <typename T>
static int k7c_launch_t(pols_ctx *ctx, const ClusterArgs &c) {
    const StatsArgs &a = c.s;
    const int kt = a.kt;
    const int64_t G = a.n_groups, n = c.n_rows, n_items = a.seg_offs ? a.n_seg : G;
    const size_t lds = k7c_lds_bytes(kt);
    if (lds > K7C_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "cluster statistics: %d columns exceed the LDS of a workgroup", kt);
    static OncePerDevice attr_once;
    if (attr_once.needed(ctx->device)) {
        POLS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k7c_scores_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)K7C_LDS_BUDGET));
        attr_once.done(ctx->device);
    }
    {
        RobustArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.s = a;
        ra.prep = c.prep;
        int rc = k7r_prepare_launch(ctx, sizeof(T) == 4 ? POLS_F32 : POLS_F64, ra);
        if (rc) return rc;
    }
    OrderPlan pl;
    int rc = k7c_order_prepare(ctx, c.ids[0], c.ways > 1 ? c.ids[1] : nullptr, a.offs, G, n, &pl);
    if (rc) return rc;
    double *sums = c.part + (size_t)n_items * k7c_part_stride(kt);
    const int n_ways = c.ways == 2 ? 3 : 1;
    for (int wi = 0; wi < n_ways; ++wi) {
        ClusterWay w;
        w.k1 = c.ids[wi == 1 ? 1 : 0];
        w.k2 = wi == 2 ? c.ids[1] : nullptr;
        w.part = c.part;
        w.sums = sums + (size_t)wi * G * (kt + 1);
        if ((rc = k7c_order_way(ctx, pl, c.ids, wi, G, &w.order))) return rc;
        hipLaunchKernelGGL(k7c_scores_kernel<T>, dim3((unsigned)n_items), dim3(256), lds, ctx->stream, c, w);
        hipLaunchKernelGGL(k7c_finish_kernel, dim3((unsigned)G), dim3(256), 0, ctx->stream, c, w);
        POLS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k7c_output_kernel, dim3((unsigned)G), dim3(64), 0, ctx->stream, c, (const double *)sums);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

int k7c_cluster_launch(pols_ctx *ctx, int dtype, const ClusterArgs &c) {
    if (c.s.kt > K7_KMAX) return fail(POLS_ERR_UNSUPPORTED, "cluster statistics: %d features (incl. intercept) > %d", c.s.kt, K7_KMAX);
    if (c.ways != 1 && c.ways != 2) return fail(POLS_ERR_INVALID, "cluster statistics: %d ways", c.ways);
    if (c.s.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k7c_launch_t<float>(ctx, c) : k7c_launch_t<double>(ctx, c);
}

}  // namespace pols
