// Channels-last SINGLE-LAUNCH Instance-Batch normalisation (round 7): y = act(Norm(X)), X = x [+ addend], on a [n][h][w][c] tensor
// in ONE persistent launch per direction — the IBN layers of the reference's best model (models/imagenet/resnet_ibn_cnsn.py:24-44:
// IBN = InstanceNorm2d on channels [0, half) + BatchNorm2d on [half, C), :63; the IBN-b stem and block ends: nn.InstanceNorm2d on
// every channel, :65,:117-121,:138-139), each followed by the block's ReLU.
//
// Same structure as the SelfNorm kernels of cnsn_nhwc_fused_kernels.h (tiles, grid barrier, write-through side arrays, give-up):
//   A  column sums of X per plane about the plane's shift (nhwc_fwd_phase_a, unchanged)
//   -- barrier --
//   B  a workgroup per GC adjacent channels (all InstanceNorm or all BatchNorm: half % GC == 0), a thread per instance:
//        IN  per plane: mean, BIASED variance over H*W -> r = 1/sqrt(var + eps_in), a = w*r
//        BN  per channel: the planes' moments combined over n in double (mean of the means; sum of the planes' centred sums of
//            squares + M*(mean_p - mean_c)^2), biased variance normalises, the unbiased one goes to running_var (momentum as
//            given: the caller resolves momentum=None), num_batches_tracked += 1; eval: the running statistics
//      apply coefficients per plane y = a*(X - xr) + b with xr = float(mean), b = bias - a*(mean - xr)
//   -- barrier --
//   C  the tiles in reverse order: y = act(a*(X - xr) + b)
// Backward (G' = G masked by the ReLU, recomputed from X and the saved coefficients with the forward's own expression: equals y > 0):
//   A' per plane sums of G' and G'*(X - xr)
//   -- barrier --
//   B' the second sum shifted to the mean itself (- lo*sum G'); IN per plane, BN per channel (the planes' sums added over n: every
//      plane of a BN channel has the same xr); dw = sum G'*xhat, db = sum G'; dX coefficients cX, c0
//   -- barrier --
//   C' dX = a*G' + cX*(X - xr) + c0  (= r*w*(G' - mean(G') - xhat*mean(G'*xhat)); eval BN: r*w*G')
// Tensor passes: forward 3 (x twice, y once; + the addend twice), backward 5 (G and x twice, dX once; + the addend twice).  With an
// addend dX is the gradient of both x and the addend (the caller aliases it).
//
// `saved` (IB_ROWS floats per plane, plane order p = n*C + c): a, xr, b (the apply coefficients — phase C reads them from there),
// r (the plane's 1/std; a BN channel's in each of its planes) and lo = mean - xr.
#pragma once
#include "cnsn_nhwc_bnhead_kernels.h"
#include "cnsn_nhwc_fused_kernels.h"

namespace cnsn {

enum IbnRow { IB_A = 0, IB_XR, IB_B, IB_R, IB_LO, IB_ROWS };

struct NhwcIbnArgs {
    NhwcFusedArgs f;     // geometry, partial sums (f.part), shift (f.kshift), dX coefficients (f.coefb), barrier, training, relu
    int half;            // channels [0, half): InstanceNorm2d; [half, C): BatchNorm2d
    float eps_in;
    const float* in_w;   // (half) or null: affine=False
    const float* in_b;
    BnHeadDev bn;        // channels [half, C), indexed c - half (unused when half == C)
    double inv_r, unbias_r;  // 1 / (N*H*W), R / (R - 1)
    float* coef;         // forward: [3][P] a, xr, b — rows IB_A..IB_B of `saved` when there is one
    float* saved;        // forward: written (may be null); backward: read
    float* d_in_w;       // backward: written (any of the four may be null)
    float* d_in_b;
    float* d_bn_w;
    float* d_bn_b;
};

// ================================================================================================
// forward
// ================================================================================================
template <typename T, int VEC, int ADD, bool KEEP>
__global__ __launch_bounds__(kBlock, CNSN_NHWC_WG_PER_CU) void nhwc_ibn_fwd_kernel(NhwcIbnArgs a, const T* __restrict__ x,
                                                                                    const T* __restrict__ addend, T* __restrict__ y) {
    extern __shared__ float lds[];
    __shared__ double red[4 * CNSN_NHWC_GC];
    __shared__ int bar_flag;
    constexpr int GC = CNSN_NHWC_GC;
    const NhwcGeom& g = a.f.g;

    // ---- A: partial moments of every tile
    nhwc_fwd_phase_a<T, VEC, ADD, KEEP, false>(a.f, x, addend, nullptr, lds);
    if (!grid_barrier(a.f.bar, 1, &bar_flag)) {
        nhwc_mark_owed<T, VEC>(g, a.f.ntiles, y);
        return;
    }

    // ---- B: coefficients, GC adjacent channels per workgroup, thread n = instance n (N <= 256)
    const CohBuf cf(a.coef);
    for (int slot = blockIdx.x; slot < a.f.ngroups; slot += gridDim.x) {
        const int grp = phase_b_group(slot, a.f.ngroups);
        const int c0 = grp * GC, n = threadIdx.x;
        const bool live = n < g.N, in = c0 < a.half;  // (uniform over the workgroup)
        const size_t p0 = (size_t)(live ? n : 0) * g.C + c0;
        double s1[GC], s2[GC], mu[GC], r[GC];
#pragma unroll
        for (int j = 0; j < GC; ++j) s1[j] = s2[j] = 0.0;
        const CohBuf pb(a.f.part);
        for (int s = 0; s < g.S; ++s) {
            add_group_coh<GC>(pb, ((size_t)s * 2 + 0) * g.P + p0, s1);
            add_group_coh<GC>(pb, ((size_t)s * 2 + 1) * g.P + p0, s2);
        }
        load_group_coh<GC>(CohBuf(a.f.kshift), p0, mu);
        const double M = (double)g.M;
#pragma unroll
        for (int j = 0; j < GC; ++j) {
            const double m2 = s2[j] - s1[j] * s1[j] / M;
            mu[j] += s1[j] / M;              // the plane's mean
            s2[j] = m2 > 0.0 ? m2 : 0.0;     // ... and its centred sum of squares
        }
        if (in) {  // nn.InstanceNorm2d: biased variance of the plane
#pragma unroll
            for (int j = 0; j < GC; ++j) r[j] = 1.0 / sqrt(s2[j] / M + (double)a.eps_in);
        } else if (a.f.training) {  // nn.BatchNorm2d: the channel's batch moments over (N, H, W)
#pragma unroll
            for (int j = 0; j < GC; ++j) s1[j] = live ? mu[j] : 0.0;
            block_sum_d<GC>(s1, red);
#pragma unroll
            for (int j = 0; j < GC; ++j) {
                const double mc = s1[j] * a.f.inv_n, d = mu[j] - mc;  // (every plane holds M pixels)
                s1[j] = live ? s2[j] + M * d * d : 0.0;
                mu[j] = mc;
            }
            block_sum_d<GC>(s1, red);
#pragma unroll
            for (int j = 0; j < GC; ++j) r[j] = 1.0 / sqrt(s1[j] * a.inv_r + (double)a.bn.eps);
            if (threadIdx.x < GC) {
                const int j = threadIdx.x, cb = c0 + j - a.half;
                const double mj = pick<GC>(mu, j), vj = pick<GC>(s1, j) * a.inv_r, mom = (double)a.bn.momentum;
                a.bn.run_mean[cb] = (float)((1.0 - mom) * (double)a.bn.run_mean[cb] + mom * mj);
                a.bn.run_var[cb] = (float)((1.0 - mom) * (double)a.bn.run_var[cb] + mom * vj * a.unbias_r);
                if (cb == 0) bump_batches_tracked(a.bn.nbt);
            }
        } else {  // eval: the running statistics
#pragma unroll
            for (int j = 0; j < GC; ++j) {
                const int cb = c0 + j - a.half;
                mu[j] = (double)a.bn.run_mean[cb];
                r[j] = 1.0 / sqrt((double)a.bn.run_var[cb] + (double)a.bn.eps);
            }
        }
        if (live) {
            float o_a[GC], o_xr[GC], o_b[GC], o_r[GC], o_lo[GC];
#pragma unroll
            for (int j = 0; j < GC; ++j) {
                const int c = c0 + j;
                double w, b;
                if (in) {
                    w = a.in_w ? (double)a.in_w[c] : 1.0;
                    b = a.in_b ? (double)a.in_b[c] : 0.0;
                } else {
                    w = (double)a.bn.weight[c - a.half];
                    b = (double)a.bn.bias[c - a.half];
                }
                const double av = w * r[j];
                o_xr[j] = (float)mu[j];
                const double lo = mu[j] - (double)o_xr[j];
                o_a[j] = (float)av;
                o_b[j] = (float)(b - av * lo);
                o_r[j] = (float)r[j];
                o_lo[j] = (float)lo;
            }
            cf.store<GC>((size_t)IB_A * g.P + p0, o_a);  // (phase C reads them)
            cf.store<GC>((size_t)IB_XR * g.P + p0, o_xr);
            cf.store<GC>((size_t)IB_B * g.P + p0, o_b);
            if (a.saved) {
                store_group<GC>(a.saved + (size_t)IB_R * g.P + p0, o_r);
                store_group<GC>(a.saved + (size_t)IB_LO * g.P + p0, o_lo);
            }
        }
        __syncthreads();  // (red is the next group's)
    }
    if (!grid_barrier(a.f.bar, 2, &bar_flag)) {
        nhwc_mark_owed<T, VEC>(g, a.f.ntiles, y);
        return;
    }

    // ---- C: y = act(a*(X - xr) + b); the tiles in reverse order (the second read finds what the first one left in the caches)
    const int mine = a.f.ntiles > (int)blockIdx.x ? (a.f.ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x : -1;
    const int relu = a.f.relu;
    for (int i = mine; i >= 0; --i) {
        const int tile = blockIdx.x + i * gridDim.x;
        const NhwcThread<VEC> t(g, tile);
        if (!t.active) continue;
        const size_t pl = t.plane0(g);
        float ca[VEC], cx[VEC], cb[VEC];
        cf.load<VEC>((size_t)IB_A * g.P + pl, ca);
        cf.load<VEC>((size_t)IB_XR * g.P + pl, cx);
        cf.load<VEC>((size_t)IB_B * g.P + pl, cb);
        constexpr int U = ADD == ADD_PRE ? 2 : 4;
        auto emit = [&](const Vec<T, VEC>& va, const Vec<T, VEC>& vb, size_t e) {
            Vec<T, VEC> o;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float f = to_float(va.v[j]);
                if constexpr (ADD == ADD_PRE) f = sum_t<T>(f, to_float(vb.v[j]));
                const float v = fmaf(ca[j], f - cx[j], cb[j]);  // (the backward's mask: nhwc_pair, same expression)
                o.v[j] = from_float<T>(relu ? fmaxf(v, 0.f) : v);
            }
            store_vec_nt<T, VEC>(y + e, o);
        };
        const int cnt = (t.p1 - t.p0 - t.r + g.rows - 1) / g.rows;  // pixels of this thread in the chunk, walked backwards
        int q = cnt - 1;
        for (; q - (U - 1) >= 0; q -= U) {
            Vec<T, VEC> va[U], vb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t e = t.elem(g, t.p0 + t.r + (q - u) * g.rows);
                va[u] = load_vec_nt<T, VEC>(x + e);
                if constexpr (ADD == ADD_PRE) vb[u] = load_vec_nt<T, VEC>(addend + e);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) emit(va[u], ADD == ADD_PRE ? vb[u] : va[u], t.elem(g, t.p0 + t.r + (q - u) * g.rows));
        }
        for (; q >= 0; --q) {
            const size_t e = t.elem(g, t.p0 + t.r + q * g.rows);
            const Vec<T, VEC> va = load_vec_nt<T, VEC>(x + e);
            Vec<T, VEC> vb = va;
            if constexpr (ADD == ADD_PRE) vb = load_vec_nt<T, VEC>(addend + e);
            emit(va, vb, e);
        }
    }
}

// ================================================================================================
// backward
// ================================================================================================
// a backward that gave up at its first barrier: the parameter gradients of the channel groups this workgroup owns read NaN
__device__ __forceinline__ void ibn_mark_params_owed(const NhwcIbnArgs& a, int gc) {
    if ((int)threadIdx.x >= gc) return;
    const float nan = __builtin_nanf("");
    for (int slot = blockIdx.x; slot < a.f.ngroups; slot += gridDim.x) {
        const int c = phase_b_group(slot, a.f.ngroups) * gc + (int)threadIdx.x;
        if (c < a.half) {
            if (a.d_in_w) a.d_in_w[c] = nan;
            if (a.d_in_b) a.d_in_b[c] = nan;
        } else {
            if (a.d_bn_w) a.d_bn_w[c - a.half] = nan;
            if (a.d_bn_b) a.d_bn_b[c - a.half] = nan;
        }
    }
}

template <typename T, int VEC, int ADD, bool KEEP>
__global__ __launch_bounds__(kBlock, CNSN_NHWC_WG_PER_CU) void nhwc_ibn_bwd_kernel(NhwcIbnArgs a, const T* __restrict__ gy,
                                                                                    const T* __restrict__ x,
                                                                                    const T* __restrict__ addend, T* __restrict__ dx) {
    extern __shared__ float lds[];
    __shared__ double red[4 * 2 * CNSN_NHWC_GC_BWD];
    __shared__ int bar_flag;
    constexpr int GC = CNSN_NHWC_GC_BWD;
    const NhwcGeom& g = a.f.g;
    const float* __restrict__ row_a = a.saved + (size_t)IB_A * g.P;
    const float* __restrict__ row_xr = a.saved + (size_t)IB_XR * g.P;
    const float* __restrict__ row_b = a.saved + (size_t)IB_B * g.P;
    const int relu = a.f.relu;

    // ---- A': per-(n, c) sums of G' and G' * (X - xr) over a pixel chunk
    for (int tile = blockIdx.x; tile < a.f.ntiles; tile += gridDim.x) {
        const NhwcThread<VEC> t(g, tile);
        float acc[2][VEC], ca[VEC], cx[VEC], cb[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[0][j] = acc[1][j] = ca[j] = cx[j] = cb[j] = 0.f;
        if (t.active) {
            const size_t pl = t.plane0(g);
            load_planes<VEC>(row_xr + pl, cx);
            if (relu) {
                load_planes<VEC>(row_a + pl, ca);
                load_planes<VEC>(row_b + pl, cb);
            }
            constexpr int U = CNSN_NHWC_UB;
            auto eat = [&](const Vec<T, VEC>& vg, const Vec<T, VEC>& vx, const Vec<T, VEC>& vb) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    float G, X;
                    nhwc_pair<T, ADD>(to_float(vg.v[j]), to_float(vx.v[j]), to_float(vb.v[j]), ca[j], cx[j], cb[j], relu, G, X);
                    acc[0][j] += G;
                    acc[1][j] = fmaf(G, X - cx[j], acc[1][j]);
                }
            };
            int p = t.p0 + t.r;
            for (; p + (U - 1) * g.rows < t.p1; p += U * g.rows) {
                Vec<T, VEC> vg[U], vx[U], vb[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const size_t e = t.elem(g, p + u * g.rows);
                    vg[u] = nhwc_ld<T, VEC, !KEEP>(gy + e);
                    vx[u] = nhwc_ld<T, VEC, !KEEP>(x + e);
                    if constexpr (ADD != ADD_NONE) vb[u] = nhwc_ld<T, VEC, !KEEP>(addend + e);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) eat(vg[u], vx[u], ADD != ADD_NONE ? vb[u] : vx[u]);
            }
            for (; p < t.p1; p += g.rows) {
                const size_t e = t.elem(g, p);
                const Vec<T, VEC> vg = nhwc_ld<T, VEC, !KEEP>(gy + e), vx = nhwc_ld<T, VEC, !KEEP>(x + e);
                Vec<T, VEC> vb = vx;
                if constexpr (ADD != ADD_NONE) vb = nhwc_ld<T, VEC, !KEEP>(addend + e);
                eat(vg, vx, vb);
            }
        }
        nhwc_rows_sum<VEC, 2, true>(g, t, acc, lds, a.f.part);
        __syncthreads();
    }
    if (!grid_barrier(a.f.bar, 1, &bar_flag)) {
        nhwc_mark_owed<T, VEC>(g, a.f.ntiles, dx);
        ibn_mark_params_owed(a, GC);
        return;
    }

    // ---- B': parameter gradients and the dX coefficients, GC adjacent channels per workgroup, thread n = instance n
    for (int slot = blockIdx.x; slot < a.f.ngroups; slot += gridDim.x) {
        const int grp = phase_b_group(slot, a.f.ngroups);
        const int c0 = grp * GC, n = threadIdx.x;
        const bool live = n < g.N, in = c0 < a.half;  // (uniform over the workgroup)
        const size_t p0 = (size_t)(live ? n : 0) * g.C + c0;
        double S1[GC], S2[GC], av[GC], r[GC], lo[GC], acc[2 * GC];
#pragma unroll
        for (int j = 0; j < GC; ++j) S1[j] = S2[j] = 0.0;
        const CohBuf pb(a.f.part);
        for (int s = 0; s < g.S; ++s) {
            add_group_coh<GC>(pb, ((size_t)s * 2 + 0) * g.P + p0, S1);
            add_group_coh<GC>(pb, ((size_t)s * 2 + 1) * g.P + p0, S2);
        }
        load_group<GC>(row_a + p0, av);
        load_group<GC>(a.saved + (size_t)IB_R * g.P + p0, r);
        load_group<GC>(a.saved + (size_t)IB_LO * g.P + p0, lo);
#pragma unroll
        for (int j = 0; j < GC; ++j) {
            S2[j] -= lo[j] * S1[j];  // sum G' * (X - mean) = sum G' * (X - xr) - (mean - xr) * sum G'
            acc[j] = live ? S1[j] : 0.0;
            acc[GC + j] = live ? (in ? r[j] * S2[j] : S2[j]) : 0.0;  // IN: the plane's sum G' * xhat
        }
        block_sum_d<2 * GC>(acc, red);  // IN: the parameter gradients (sums over n); BN: the channel's two sums
        float o_cx[GC], o_c0[GC];
#pragma unroll
        for (int j = 0; j < GC; ++j) {
            double cxj = 0.0, c0j = 0.0;
            if (in) {
                const double sgx = r[j] * S2[j], inv_m = 1.0 / (double)g.M;  // sum G' * xhat of the plane
                cxj = -av[j] * r[j] * sgx * inv_m;
                c0j = -av[j] * S1[j] * inv_m;
            } else if (a.f.training) {
                const double sgx = r[j] * acc[GC + j];
                cxj = -av[j] * r[j] * sgx * a.inv_r;
                c0j = -av[j] * acc[j] * a.inv_r;
            }
            o_cx[j] = (float)cxj;
            o_c0[j] = (float)(c0j - cxj * lo[j]);  // evaluated as cX*(X - xr) + c0: the rounding of the reference point folded in
        }
        if (threadIdx.x < GC) {
            const int j = threadIdx.x, c = c0 + j;
            const double sg = pick<2 * GC>(acc, j), sgx = in ? pick<2 * GC>(acc, GC + j) : pick<GC>(r, j) * pick<2 * GC>(acc, GC + j);
            if (in) {
                if (a.d_in_w) a.d_in_w[c] = (float)sgx;
                if (a.d_in_b) a.d_in_b[c] = (float)sg;
            } else {
                if (a.d_bn_w) a.d_bn_w[c - a.half] = (float)sgx;
                if (a.d_bn_b) a.d_bn_b[c - a.half] = (float)sg;
            }
        }
        if (live) {
            const CohBuf cb(a.f.coefb);  // (phase C' reads them)
            cb.store<GC>(p0, o_cx);
            cb.store<GC>(g.P + p0, o_c0);
        }
        __syncthreads();
    }
    if (!grid_barrier(a.f.bar, 2, &bar_flag)) {
        nhwc_mark_owed<T, VEC>(g, a.f.ntiles, dx);
        return;
    }

    // ---- C': dX = a*G' + cX*(X - xr) + c0, tiles in reverse
    const int mine = a.f.ntiles > (int)blockIdx.x ? (a.f.ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x : -1;
    for (int i = mine; i >= 0; --i) {
        const int tile = blockIdx.x + i * gridDim.x;
        const NhwcThread<VEC> t(g, tile);
        if (!t.active) continue;
        const size_t pl = t.plane0(g);
        float ca[VEC], cx[VEC], cb[VEC], kx[VEC], k0[VEC];
        load_planes<VEC>(row_a + pl, ca);
        load_planes<VEC>(row_xr + pl, cx);
        load_planes<VEC>(row_b + pl, cb);
        const CohBuf cbuf(a.f.coefb);
        cbuf.load<VEC>(pl, kx);
        cbuf.load<VEC>(g.P + pl, k0);
        auto emit = [&](const Vec<T, VEC>& vg, const Vec<T, VEC>& vx, const Vec<T, VEC>& vb, size_t e) {
            Vec<T, VEC> o;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float G, X;
                nhwc_pair<T, ADD>(to_float(vg.v[j]), to_float(vx.v[j]), to_float(vb.v[j]), ca[j], cx[j], cb[j], relu, G, X);
                o.v[j] = from_float<T>(fmaf(ca[j], G, fmaf(kx[j], X - cx[j], k0[j])));
            }
            store_vec_nt<T, VEC>(dx + e, o);
        };
        constexpr int U = CNSN_NHWC_UB;
        const int cnt = (t.p1 - t.p0 - t.r + g.rows - 1) / g.rows;
        int q = cnt - 1;
        for (; q - (U - 1) >= 0; q -= U) {
            Vec<T, VEC> vg[U], vx[U], vb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t e = t.elem(g, t.p0 + t.r + (q - u) * g.rows);
                vg[u] = load_vec_nt<T, VEC>(gy + e);
                vx[u] = load_vec_nt<T, VEC>(x + e);
                if constexpr (ADD != ADD_NONE) vb[u] = load_vec_nt<T, VEC>(addend + e);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) emit(vg[u], vx[u], ADD != ADD_NONE ? vb[u] : vx[u], t.elem(g, t.p0 + t.r + (q - u) * g.rows));
        }
        for (; q >= 0; --q) {
            const size_t e = t.elem(g, t.p0 + t.r + q * g.rows);
            const Vec<T, VEC> vg = load_vec_nt<T, VEC>(gy + e), vx = load_vec_nt<T, VEC>(x + e);
            Vec<T, VEC> vb = vx;
            if constexpr (ADD != ADD_NONE) vb = load_vec_nt<T, VEC>(addend + e);
            emit(vg, vx, vb, e);
        }
    }
}

}  // namespace cnsn
