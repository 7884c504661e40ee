// BatchNorm2d (+ add) + ReLU on NCHW tensors (round 12): y = act(BatchNorm2d(x) [+ addend]), act = ReLU or the identity, in TWO
// ordinary launches per direction — the plain form of the channels-last single launch (cnsn_nhwc_bn_kernels.h): no persistent
// grid, no grid barrier, no wait, no context.  The same 3 + 5 tensor passes, one launch more per direction, and the launches can
// be recorded under stream capture.
//
// A channel of an NCHW tensor is N planes of P = H*W contiguous elements at stride C*P.  A TILE is one channel x a range of
// instances x a range of the plane (NchwBnGeom: several instances per tile where planes are small, several tiles per plane where
// they are large), a workgroup per tile, grid = C * tiles; the geometry is a function of the shape and the element size alone.
// A thread takes SLOTS of a tile's (instance, plane range): slot 0 is the scalar head up to the first 16-byte boundary of the
// range, every further slot 16 aligned bytes — one vector access when it lies inside the range, scalar accesses where the range
// ends in it.  No access falls outside [range start, range end).
//   forward 1   per tile sum(x - s) and sum((x - s)^2), s = the channel's first element (the shift of the one-pass sums:
//               cnsn_device.h) -> part[c][tile]
//   forward 2   every workgroup adds ITS channel's partials in double, in one fixed order: all tiles of a channel hold
//               bit-identical mean / rstd.  Then its tile: v = a*(x - mean) + bias, a = weight*rstd, y = act(T(v) [+ addend]) —
//               bn_act_value, the channels-last kernels' expression.  Tile 0 writes `saved` and the running buffers, channel 0
//               counts the step.
//   backward 1  per tile sum G' and sum G'*(x - mean), G' = grad_y masked by the ReLU (the mask recomputed from x, the addend,
//               weight, bias and `saved` with the forward's expression; y is never read)
//   backward 2  the channel's sums as in the forward; dx = a*G' + kx*(x - mean) + k0, d_addend = G' behind a ReLU; tile 0 writes
//               d_weight = rstd * sum G'(x - mean) and d_bias = sum G'
//   eval        a and mean from the running statistics, one launch over the same tiles
// No atomics: two calls on the same input are bit-identical.
#pragma once
#include "cnsn_nhwc_bn_kernels.h"

namespace cnsn {

struct NchwBnGeom {
    int N, C, P;   // instances, channels, elements per plane
    int ipt;       // instances per tile
    int epr;       // elements per plane range (a multiple of the vector when a plane has several)
    int spp;       // ranges per plane
    int tpc;       // tiles per channel: ceil(N / ipt) * spp
};

struct NchwBnArgs {
    NchwBnGeom g;
    int relu;
    BnHeadDev bn;
    double inv_r, unbias_r;  // 1 / (N*P), N*P / (N*P - 1)
    float* part;             // [C][tpc][2] the tiles' sums
    float* stat;             // forward: [2][C] mean, rstd (`saved`) or null
    const float* saved;      // backward: [2][C]
    float* d_w;              // backward: (C) or null
    float* d_b;
};

// the workgroup's tile and the walk over its slots
template <int VEC>
struct NchwBnTile {
    int c, t, n0, ni, e0, len, nslot;
    __device__ __forceinline__ NchwBnTile(const NchwBnGeom& g) {
        c = (int)blockIdx.x / g.tpc;
        t = (int)blockIdx.x - c * g.tpc;
        const int ig = t / g.spp, s = t - ig * g.spp;
        n0 = ig * g.ipt;
        ni = g.N - n0 < g.ipt ? g.N - n0 : g.ipt;
        e0 = s * g.epr;
        len = g.P - e0 < g.epr ? g.P - e0 : g.epr;
        nslot = 1 + (len + VEC - 1) / VEC;
    }
    // vec(e): VEC elements at the 16-byte aligned element offset e; one(e): the element at e
    template <typename FV, typename FS>
    __device__ __forceinline__ void walk(const NchwBnGeom& g, FV&& vec, FS&& one) const {
        const int total = ni * nslot;
        for (int i = threadIdx.x; i < total; i += kBlock) {
            const int q = ni == 1 ? 0 : i / nslot, k = i - q * nslot;
            const size_t lo = ((size_t)(n0 + q) * g.C + c) * g.P + e0, hi = lo + len;
            const size_t body = (lo + VEC - 1) & ~(size_t)(VEC - 1);
            if (k == 0) {
                const size_t end = body < hi ? body : hi;
                for (size_t e = lo; e < end; ++e) one(e);
            } else {
                const size_t b = body + (size_t)(k - 1) * VEC;
                if (b + VEC <= hi)
                    vec(b);
                else
                    for (size_t e = b; e < hi; ++e) one(e);
            }
        }
    }
};

// the tile's two sums -> part[c][t]
__device__ __forceinline__ void nchw_bn_put(const NchwBnGeom& g, int c, int t, float s0, float s1, float* part, double* red) {
    double acc[2] = {(double)s0, (double)s1};
    block_sum_d<2>(acc, red);
    if (threadIdx.x == 0) *reinterpret_cast<float2*>(part + ((size_t)c * g.tpc + t) * 2) = make_float2((float)acc[0], (float)acc[1]);
}

// the channel's two sums: thread j adds tiles j, j + 256, .. in double, then the block; the same order in every workgroup
__device__ __forceinline__ void nchw_bn_gather(const NchwBnGeom& g, int c, const float* part, double (&acc)[2], double* red) {
    acc[0] = acc[1] = 0.0;
    for (int j = threadIdx.x; j < g.tpc; j += kBlock) {
        const float2 v = *reinterpret_cast<const float2*>(part + ((size_t)c * g.tpc + j) * 2);
        acc[0] += (double)v.x;
        acc[1] += (double)v.y;
    }
    block_sum_d<2>(acc, red);
}

// ================================================================================================
// forward, training
// ================================================================================================
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void nchw_bnact_fwd_stats_kernel(NchwBnArgs a, const T* __restrict__ x) {
    __shared__ double red[4 * 2];
    const NchwBnGeom& g = a.g;
    const NchwBnTile<VEC> tl(g);
    const float s = to_float(x[(size_t)tl.c * g.P]);
    float s0 = 0.f, s1 = 0.f;
    auto eat = [&](float v) {
        const float d = v - s;
        s0 += d;
        s1 = fmaf(d, d, s1);
    };
    tl.walk(
        g,
        [&](size_t e) {
            const Vec<T, VEC> v = load_vec<T, VEC>(x + e);  // (default policy: launch 2 reads it again)
#pragma unroll
            for (int j = 0; j < VEC; ++j) eat(to_float(v.v[j]));
        },
        [&](size_t e) { eat(to_float(x[e])); });
    nchw_bn_put(g, tl.c, tl.t, s0, s1, a.part, red);
}

template <typename T, int VEC, bool ADD>
__global__ __launch_bounds__(kBlock) void nchw_bnact_fwd_apply_kernel(NchwBnArgs a, const T* __restrict__ x,
                                                                      const T* __restrict__ addend, T* __restrict__ y) {
    __shared__ double red[4 * 2];
    const NchwBnGeom& g = a.g;
    const NchwBnTile<VEC> tl(g);
    const int c = tl.c;
    double acc[2];
    nchw_bn_gather(g, c, a.part, acc, red);
    const double mean = (double)to_float(x[(size_t)c * g.P]) + acc[0] * a.inv_r;
    const double m2 = acc[1] - acc[0] * acc[0] * a.inv_r;
    const double var = (m2 > 0.0 ? m2 : 0.0) * a.inv_r;  // biased: what normalises (torch)
    const double rstd = 1.0 / sqrt(var + (double)a.bn.eps);
    const float xr = (float)mean, rs = (float)rstd;
    if (tl.t == 0 && threadIdx.x == 0) {
        running_update(a.bn.run_mean, a.bn.run_var, a.bn.nbt, c, mean, var, a.unbias_r, (double)a.bn.momentum);
        if (a.stat) {
            a.stat[c] = xr;
            a.stat[g.C + c] = rs;
        }
    }
    const float ca = __fmul_rn(a.bn.weight[c], rs), cb = a.bn.bias[c];
    const int relu = a.relu;
    auto value = [&](float X, float B) {
        const float v = bn_act_value<T, ADD>(X, B, ca, xr, cb);
        return from_float<T>(relu ? fmaxf(v, 0.f) : v);
    };
    tl.walk(
        g,
        [&](size_t e) {
            const Vec<T, VEC> va = load_vec_nt<T, VEC>(x + e);
            Vec<T, VEC> vb = va, o;
            if constexpr (ADD) vb = load_vec_nt<T, VEC>(addend + e);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o.v[j] = value(to_float(va.v[j]), to_float(vb.v[j]));
            store_vec_nt<T, VEC>(y + e, o);
        },
        [&](size_t e) {
            const float X = to_float(x[e]);
            float B = X;
            if constexpr (ADD) B = to_float(addend[e]);
            y[e] = value(X, B);
        });
}

// ================================================================================================
// forward, eval: the running statistics
// ================================================================================================
template <typename T, int VEC, bool ADD>
__global__ __launch_bounds__(kBlock) void nchw_bnact_eval_kernel(NchwBnGeom g, BnHeadDev bn, int relu, const T* __restrict__ x,
                                                                 const T* __restrict__ addend, T* __restrict__ y) {
    const NchwBnTile<VEC> tl(g);
    const int c = tl.c;
    const float xr = bn.run_mean[c], cb = bn.bias[c];
    const float ca = __fmul_rn(bn.weight[c], (float)(1.0 / sqrt((double)bn.run_var[c] + (double)bn.eps)));
    auto value = [&](float X, float B) {
        const float v = bn_act_value<T, ADD>(X, B, ca, xr, cb);
        return from_float<T>(relu ? fmaxf(v, 0.f) : v);
    };
    tl.walk(
        g,
        [&](size_t e) {
            const Vec<T, VEC> va = load_vec_nt<T, VEC>(x + e);
            Vec<T, VEC> vb = va, o;
            if constexpr (ADD) vb = load_vec_nt<T, VEC>(addend + e);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o.v[j] = value(to_float(va.v[j]), to_float(vb.v[j]));
            store_vec_nt<T, VEC>(y + e, o);
        },
        [&](size_t e) {
            const float X = to_float(x[e]);
            float B = X;
            if constexpr (ADD) B = to_float(addend[e]);
            y[e] = value(X, B);
        });
}

// ================================================================================================
// backward, training.  ADD: ReLU behind an addend — the addend is read for the mask and d_addend = G' is written
// ================================================================================================
// the masked gradient of one element
template <typename T, bool ADD>
__device__ __forceinline__ float nchw_bn_masked(int relu, float G, float X, float B, float ca, float xr, float cb) {
    if (!relu) return G;
    return relu_open<T>(bn_act_value<T, ADD>(X, B, ca, xr, cb)) ? G : 0.f;
}

template <typename T, int VEC, bool ADD>
__global__ __launch_bounds__(kBlock) void nchw_bnact_bwd_stats_kernel(NchwBnArgs a, const T* __restrict__ gy,
                                                                      const T* __restrict__ x, const T* __restrict__ addend) {
    __shared__ double red[4 * 2];
    const NchwBnGeom& g = a.g;
    const NchwBnTile<VEC> tl(g);
    const int c = tl.c, relu = a.relu;
    const float xr = a.saved[c];
    const float ca = __fmul_rn(a.bn.weight[c], a.saved[g.C + c]), cb = a.bn.bias[c];
    float s0 = 0.f, s1 = 0.f;
    auto eat = [&](float Gin, float X, float B) {
        const float G = nchw_bn_masked<T, ADD>(relu, Gin, X, B, ca, xr, cb);
        s0 += G;
        s1 = fmaf(G, X - xr, s1);
    };
    tl.walk(
        g,
        [&](size_t e) {
            const Vec<T, VEC> vg = load_vec<T, VEC>(gy + e), vx = load_vec<T, VEC>(x + e);
            Vec<T, VEC> vb = vx;
            if constexpr (ADD) vb = load_vec<T, VEC>(addend + e);
#pragma unroll
            for (int j = 0; j < VEC; ++j) eat(to_float(vg.v[j]), to_float(vx.v[j]), to_float(vb.v[j]));
        },
        [&](size_t e) {
            const float X = to_float(x[e]);
            float B = X;
            if constexpr (ADD) B = to_float(addend[e]);
            eat(to_float(gy[e]), X, B);
        });
    nchw_bn_put(g, c, tl.t, s0, s1, a.part, red);
}

template <typename T, int VEC, bool ADD>
__global__ __launch_bounds__(kBlock) void nchw_bnact_bwd_apply_kernel(NchwBnArgs a, const T* __restrict__ gy,
                                                                      const T* __restrict__ x, const T* __restrict__ addend,
                                                                      T* __restrict__ dx, T* __restrict__ d_addend) {
    __shared__ double red[4 * 2];
    const NchwBnGeom& g = a.g;
    const NchwBnTile<VEC> tl(g);
    const int c = tl.c, relu = a.relu;
    double acc[2];
    nchw_bn_gather(g, c, a.part, acc, red);
    const float xr = a.saved[c], rs = a.saved[g.C + c];
    const float ca = __fmul_rn(a.bn.weight[c], rs), cb = a.bn.bias[c];
    const double rstd = (double)rs, av = (double)ca;
    if (tl.t == 0 && threadIdx.x == 0) {
        if (a.d_b) a.d_b[c] = (float)acc[0];
        if (a.d_w) a.d_w[c] = (float)(rstd * acc[1]);
    }
    const float kx = (float)(-av * rstd * rstd * acc[1] * a.inv_r), k0 = (float)(-av * acc[0] * a.inv_r);
    tl.walk(
        g,
        [&](size_t e) {
            const Vec<T, VEC> vg = load_vec_nt<T, VEC>(gy + e), vx = load_vec_nt<T, VEC>(x + e);
            Vec<T, VEC> vb = vx, o, om;
            if constexpr (ADD) vb = load_vec_nt<T, VEC>(addend + e);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float X = to_float(vx.v[j]);
                const float G = nchw_bn_masked<T, ADD>(relu, to_float(vg.v[j]), X, to_float(vb.v[j]), ca, xr, cb);
                o.v[j] = from_float<T>(fmaf(ca, G, fmaf(kx, X - xr, k0)));
                om.v[j] = from_float<T>(G);
            }
            store_vec_nt<T, VEC>(dx + e, o);
            if constexpr (ADD) store_vec_nt<T, VEC>(d_addend + e, om);
        },
        [&](size_t e) {
            const float X = to_float(x[e]);
            float B = X;
            if constexpr (ADD) B = to_float(addend[e]);
            const float G = nchw_bn_masked<T, ADD>(relu, to_float(gy[e]), X, B, ca, xr, cb);
            dx[e] = from_float<T>(fmaf(ca, G, fmaf(kx, X - xr, k0)));
            if constexpr (ADD) d_addend[e] = from_float<T>(G);
        });
}

}  // namespace cnsn
