// Channels-last SINGLE-LAUNCH BatchNorm2d (+ add) + ReLU (round 8): y = act(BatchNorm2d(x) [+ addend]), act = ReLU or the identity,
// on a [n][h][w][c] tensor in ONE persistent launch per direction — the plainest pattern of the backbones, `relu(bn(conv(x)))`
// (models/imagenet/resnet_cnsn.py:104-110: bn1, bn2; :257-259: the stem) and the plain block end `relu(bn3(h) + identity)`.
//
// BatchNorm2d has no per-plane algebra: the tensor is an R x C matrix (R = N*H*W rows) and EVERYTHING on the side is per channel.
// Tiles are (row chunk, column block) of that matrix; the geometry (BnActGeom) is a function of the shape alone, so the partial
// sums — and with them every result — do not depend on how many workgroups the grid got.  With a grid that is a multiple of the
// column blocks (1, 2, 4 or 8 for every width of a ResNet; the grid is a multiple of 8) a workgroup's tiles share a column block.
// A thread owns VEC adjacent channels of a row and walks `rows` apart: statistics are in-lane column sums.
//   A  every tile: sum(x - k_c) and sum((x - k_c)^2) over its rows, k_c = the median of x[row, c] over three rows
//      (BnActGeom::ks: a pixel inside the plane of three images spread over the batch — the shift of cnsn_device.h; no border
//      pixel and no single image can make it atypical) — a shift every workgroup reads for itself, so the tiles' sums merge by
//      plain addition (in double): no Chan merge, no shift array.  Rows merged in LDS, ONE 16-byte write-through record per
//      tile and four channels: side traffic tiles x 2 x C/ncb floats
//   -- barrier --
//   B  a workgroup per four adjacent channels: the tiles' sums added in double -> mean, BIASED variance, rstd; running_mean,
//      running_var (unbiased, momentum as given), num_batches_tracked += 1; mean and rstd written through (to `saved` when the
//      caller keeps it)
//   -- barrier --
//   C  the tiles in reverse order (the tail of A is still in L2 / the Infinity Cache): v = a*(x - mean) + bias, a = weight*rstd
//      (all float, the expression the backward repeats), y = act(T(v) [+ addend]) — rounded where the un-fused sequence rounds:
//      BatchNorm2d's output, then the sum.  3 tensor passes (x twice, y once); the addend is read once, here.
// Backward (G' = gy masked by the ReLU, the mask recomputed from x (and the addend), weight, bias and `saved` with the forward's
// own expression: equals y > 0, y is never read):
//   A' per tile sum G' and sum G'*(x - mean)
//   -- barrier --
//   B' d_bias = sum G', d_weight = rstd * sum G'*(x - mean); kx = -a*rstd^2*sum G'(x - mean)/R, k0 = -a*sum G'/R
//   -- barrier --
//   C' dx = a*G' + kx*(x - mean) + k0; with an addend and ReLU d_addend = G' is a second output.  5 passes (gy, x twice; dx once).
// Eval mode: a and mean from the running statistics, one plain element-wise launch (no barrier, no context), forward only.
//
// Two barriers (phase B on its own), as the IBN kernel: doing B redundantly in every consumer would have each of ~1 000 workgroups
// add ~1 000 partial records per channel of its column block — more side reads than the tensor itself at the wide sites.
//
// `saved`: 2*C floats — the batch mean (rounded to float: what y was evaluated with) and rstd of every channel.
#pragma once
#include "cnsn_nhwc_bnhead_kernels.h"
#include "cnsn_nhwc_fused_kernels.h"

namespace cnsn {

constexpr int kBnActTiles = 1024;    // tiles the geometry aims at: four workgroups on each of 256 compute units
constexpr int kBnActMinRows = 64;    // rows of a tile at least (a tile's side record costs as much as 16 / sizeof(T) of its rows)
constexpr int kBnActEvalIters = 8;   // rows a thread of the eval kernel takes

struct BnActGeom {
    int R, C;     // rows N*H*W, channels
    int tc;       // vector columns of the matrix: C / VEC
    int tcb;      // vector columns of a column block
    int rows;     // rows a workgroup walks in parallel: 256 / tcb
    int ncb;      // column blocks
    int wpc;      // row chunks (tiles per column block)
    int chunk;    // rows per chunk (the last one may be shorter, none is empty)
    int ks[3];    // the rows the shift of the sums is the median of
};

struct BnActArgs {
    BnActGeom g;
    int ntiles;   // ncb * wpc
    int relu, keep;
    BnHeadDev bn;
    double inv_r, unbias_r;  // 1 / R, R / (R - 1)
    float* part;    // [2][wpc][C] the tiles' sums
    float* stat;    // forward: [2][C] mean, rstd as phase C reads them (`saved` when the caller keeps it)
    float* coef;    // backward: [2][C] kx, k0
    const float* saved;  // backward: [2][C]
    float* d_w;     // backward: (C) or null
    float* d_b;
    GridBar bar;
};

template <int VEC>
struct BnActTile {
    int cb, j, col, r, vc, p0, p1;
    bool active;
    __device__ __forceinline__ BnActTile(const BnActGeom& g, int tile) {
        cb = tile % g.ncb;
        j = tile / g.ncb;
        col = (int)threadIdx.x % g.tcb;
        r = (int)threadIdx.x / g.tcb;
        vc = cb * g.tcb + col;
        active = r < g.rows && vc < g.tc;
        p0 = j * g.chunk;
        p1 = p0 + g.chunk < g.R ? p0 + g.chunk : g.R;
    }
    __device__ __forceinline__ int ch() const { return vc * VEC; }  // first channel of the thread's vector
    __device__ __forceinline__ size_t elem(const BnActGeom& g, int p) const { return (size_t)p * g.C + (size_t)vc * VEC; }
};

// the rows of a tile -> one value per channel and accumulator, added in a fixed order, 16-byte write-through stores:
// part[k][j][channel]; lds: [NACC][rows][tcb*VEC] floats
template <int VEC, int NACC>
__device__ __forceinline__ void bn_act_rows_sum(const BnActGeom& g, const BnActTile<VEC>& t, const float (&acc)[NACC][VEC], float* lds,
                                                float* part) {
    const int width = g.tcb * VEC;
    if (t.r < g.rows) {
#pragma unroll
        for (int k = 0; k < NACC; ++k)
#pragma unroll
            for (int j = 0; j < VEC; ++j) lds[((size_t)k * g.rows + t.r) * width + t.col * VEC + j] = t.active ? acc[k][j] : 0.f;
    }
    __syncthreads();
    const CohBuf pb(part);
    const int total = NACC * width, first = t.cb * g.tcb * VEC;  // channel of the tile's first column
    for (int ch = (int)threadIdx.x * 4; ch < total; ch += kBlock * 4) {
        const int k = ch / width, off = ch - k * width;
        if (first + off >= g.C) continue;  // (the last column block may be partly outside the matrix; C % 4 == 0)
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = 0; q < g.rows; ++q) {
            const float4 w = *reinterpret_cast<const float4*>(lds + ((size_t)k * g.rows + q) * width + off);
            v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
        }
        pb.st4(((size_t)k * g.wpc + t.j) * g.C + first + off, v.x, v.y, v.z, v.w);
    }
    __syncthreads();  // (the staging area is the next tile's)
}

// the shift of channel c (phase A: per vector; phase B: per channel)
template <typename T>
__device__ __forceinline__ float bn_act_shift(const BnActGeom& g, const T* __restrict__ x, int c) {
    return median3(to_float(x[(size_t)g.ks[0] * g.C + c]), to_float(x[(size_t)g.ks[1] * g.C + c]),
                   to_float(x[(size_t)g.ks[2] * g.C + c]));
}

// phase B / B': the tiles' two sums of four adjacent channels, added over the tiles in double by the whole workgroup
__device__ __forceinline__ void bn_act_gather(const BnActArgs& a, int c0, double (&acc)[8], double* red) {
    const BnActGeom& g = a.g;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const CohBuf pb(a.part);
    for (int j = threadIdx.x; j < g.wpc; j += kBlock) {
        float f[4], h[4];
        pb.load<4>((size_t)j * g.C + c0, f);
        pb.load<4>(((size_t)g.wpc + j) * g.C + c0, h);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += (double)f[q], acc[4 + q] += (double)h[q];
    }
    block_sum_d<8>(acc, red);
}

// a launch that gave up: the first row of every tile this workgroup owns reads NaN (loud on the same step)
template <typename T, int VEC>
__device__ __forceinline__ void bn_act_mark_owed(const BnActArgs& a, T* __restrict__ out) {
    Vec<T, VEC> nanv;
#pragma unroll
    for (int j = 0; j < VEC; ++j) nanv.v[j] = from_float<T>(__builtin_nanf(""));
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const BnActTile<VEC> t(a.g, tile);
        if (t.active && t.r == 0) store_vec<T, VEC>(out + t.elem(a.g, t.p0), nanv);
    }
}

// v = a*(x - mean) + bias, then the sum with the addend, as the un-fused sequence rounds them; the value whose sign is the mask
template <typename T, bool ADD>
__device__ __forceinline__ float bn_act_value(float x, float b, float ca, float xr, float bias) {
    const float v = fmaf(ca, x - xr, bias);
    if constexpr (ADD)
        return sum_t<T>(to_float(from_float<T>(v)), b);
    else
        return v;
}

// the thread's per-channel values: a = weight*rstd (one float product, both directions) and the bias
template <int VEC>
__device__ __forceinline__ void bn_act_coefs(const BnHeadDev& bn, int ch, const float (&rstd)[VEC], float (&ca)[VEC],
                                             float (&cb)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        ca[j] = __fmul_rn(bn.weight[ch + j], rstd[j]);
        cb[j] = bn.bias[ch + j];
    }
}

// ================================================================================================
// forward, training
// ================================================================================================
template <typename T, int VEC, bool ADD, bool KEEP>
__global__ __launch_bounds__(kBlock, CNSN_NHWC_WG_PER_CU) void nhwc_bnact_fwd_kernel(BnActArgs a, const T* __restrict__ x,
                                                                                      const T* __restrict__ addend, T* __restrict__ y) {
    extern __shared__ float lds[];
    __shared__ double red[4 * 8];
    __shared__ int bar_flag;
    const BnActGeom& g = a.g;

    // ---- A: the two sums of every tile about the channels' shift
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const BnActTile<VEC> t(g, tile);
        float K[VEC], acc[2][VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) K[j] = acc[0][j] = acc[1][j] = 0.f;
        if (t.active) {
            const Vec<T, VEC> k0 = load_vec<T, VEC>(x + t.elem(g, g.ks[0])), k1 = load_vec<T, VEC>(x + t.elem(g, g.ks[1])),
                              k2 = load_vec<T, VEC>(x + t.elem(g, g.ks[2]));
#pragma unroll
            for (int j = 0; j < VEC; ++j) K[j] = median3(to_float(k0.v[j]), to_float(k1.v[j]), to_float(k2.v[j]));
            auto eat = [&](const Vec<T, VEC>& va) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float d = to_float(va.v[j]) - K[j];
                    acc[0][j] += d;
                    acc[1][j] = fmaf(d, d, acc[1][j]);
                }
            };
            constexpr int U = 4;
            int p = t.p0 + t.r;
            for (; p + (U - 1) * g.rows < t.p1; p += U * g.rows) {
                Vec<T, VEC> va[U];
#pragma unroll
                for (int u = 0; u < U; ++u) va[u] = nhwc_ld<T, VEC, !KEEP>(x + t.elem(g, p + u * g.rows));
#pragma unroll
                for (int u = 0; u < U; ++u) eat(va[u]);
            }
            for (; p < t.p1; p += g.rows) eat(nhwc_ld<T, VEC, !KEEP>(x + t.elem(g, p)));
        }
        bn_act_rows_sum<VEC, 2>(g, t, acc, lds, a.part);
    }
    if (!grid_barrier(a.bar, 1, &bar_flag)) {
        bn_act_mark_owed<T, VEC>(a, y);
        return;
    }

    // ---- B: per channel mean, biased variance, rstd; the running buffers
    const int ngroups = g.C / 4;
    for (int slot = blockIdx.x; slot < ngroups; slot += gridDim.x) {
        const int c0 = phase_b_group(slot, ngroups) * 4;
        double acc[8];
        bn_act_gather(a, c0, acc, red);
        if (threadIdx.x == 0) {
            float o_m[4], o_r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + q;
                const double s1 = acc[q], s2 = acc[4 + q];
                const double mean = (double)bn_act_shift<T>(g, x, c) + s1 * a.inv_r;
                const double m2 = s2 - s1 * s1 * a.inv_r;
                const double var = (m2 > 0.0 ? m2 : 0.0) * a.inv_r;  // biased: what normalises (torch)
                const double rstd = 1.0 / sqrt(var + (double)a.bn.eps);
                running_update(a.bn.run_mean, a.bn.run_var, a.bn.nbt, c, mean, var, a.unbias_r, (double)a.bn.momentum);
                o_m[q] = (float)mean;
                o_r[q] = (float)rstd;
            }
            const CohBuf sb(a.stat);  // (phase C reads them)
            sb.st4((size_t)c0, o_m[0], o_m[1], o_m[2], o_m[3]);
            sb.st4((size_t)g.C + c0, o_r[0], o_r[1], o_r[2], o_r[3]);
        }
        __syncthreads();  // (red is the next group's)
    }
    if (!grid_barrier(a.bar, 2, &bar_flag)) {
        bn_act_mark_owed<T, VEC>(a, y);
        return;
    }

    // ---- C: y = act(T(a*(x - mean) + bias) [+ addend]); the tiles in reverse order, every tile backwards
    const int mine = a.ntiles > (int)blockIdx.x ? (a.ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x : -1;
    const int relu = a.relu;
    const CohBuf sb(a.stat);
    for (int i = mine; i >= 0; --i) {
        const BnActTile<VEC> t(g, (int)blockIdx.x + i * (int)gridDim.x);
        if (!t.active) continue;
        float xr[VEC], rs[VEC], ca[VEC], cb[VEC];
        sb.load<VEC>((size_t)t.ch(), xr);
        sb.load<VEC>((size_t)g.C + t.ch(), rs);
        bn_act_coefs<VEC>(a.bn, t.ch(), rs, ca, cb);
        auto emit = [&](const Vec<T, VEC>& va, const Vec<T, VEC>& vb, size_t e) {
            Vec<T, VEC> o;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float v = bn_act_value<T, ADD>(to_float(va.v[j]), to_float(vb.v[j]), ca[j], xr[j], cb[j]);
                o.v[j] = from_float<T>(relu ? fmaxf(v, 0.f) : v);
            }
            store_vec_nt<T, VEC>(y + e, o);
        };
        constexpr int U = ADD ? 2 : 4;
        const int cnt = (t.p1 - t.p0 - t.r + g.rows - 1) / g.rows;  // rows of this thread in the tile
        int q = cnt - 1;
        for (; q - (U - 1) >= 0; q -= U) {
            Vec<T, VEC> va[U], vb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t e = t.elem(g, t.p0 + t.r + (q - u) * g.rows);
                va[u] = load_vec_nt<T, VEC>(x + e);
                if constexpr (ADD) vb[u] = load_vec_nt<T, VEC>(addend + e);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) emit(va[u], ADD ? vb[u] : va[u], t.elem(g, t.p0 + t.r + (q - u) * g.rows));
        }
        for (; q >= 0; --q) {
            const size_t e = t.elem(g, t.p0 + t.r + q * g.rows);
            const Vec<T, VEC> va = load_vec_nt<T, VEC>(x + e);
            Vec<T, VEC> vb = va;
            if constexpr (ADD) vb = load_vec_nt<T, VEC>(addend + e);
            emit(va, vb, e);
        }
    }
}

// ================================================================================================
// forward, eval: the running statistics, one plain element-wise launch (a workgroup per tile of g; no barrier)
// ================================================================================================
template <typename T, int VEC, bool ADD>
__global__ __launch_bounds__(kBlock) void nhwc_bnact_eval_kernel(BnActGeom g, BnHeadDev bn, int relu, const T* __restrict__ x,
                                                                 const T* __restrict__ addend, T* __restrict__ y) {
    const BnActTile<VEC> t(g, (int)blockIdx.x);
    if (!t.active) return;
    float xr[VEC], ca[VEC], cb[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int c = t.ch() + j;
        xr[j] = bn.run_mean[c];
        ca[j] = __fmul_rn(bn.weight[c], (float)(1.0 / sqrt((double)bn.run_var[c] + (double)bn.eps)));
        cb[j] = bn.bias[c];
    }
    for (int p = t.p0 + t.r; p < t.p1; p += g.rows) {
        const size_t e = t.elem(g, p);
        const Vec<T, VEC> va = load_vec_nt<T, VEC>(x + e);
        Vec<T, VEC> vb = va, o;
        if constexpr (ADD) vb = load_vec_nt<T, VEC>(addend + e);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float v = bn_act_value<T, ADD>(to_float(va.v[j]), to_float(vb.v[j]), ca[j], xr[j], cb[j]);
            o.v[j] = from_float<T>(relu ? fmaxf(v, 0.f) : v);
        }
        store_vec_nt<T, VEC>(y + e, o);
    }
}

// ================================================================================================
// backward, training
// ================================================================================================
// ADD: ReLU behind an addend — the addend is read for the mask and d_addend = G' is written
template <typename T, int VEC, bool ADD, bool KEEP>
__global__ __launch_bounds__(kBlock, CNSN_NHWC_WG_PER_CU) void nhwc_bnact_bwd_kernel(BnActArgs a, const T* __restrict__ gy,
                                                                                      const T* __restrict__ x,
                                                                                      const T* __restrict__ addend, T* __restrict__ dx,
                                                                                      T* __restrict__ d_addend) {
    extern __shared__ float lds[];
    __shared__ double red[4 * 8];
    __shared__ int bar_flag;
    const BnActGeom& g = a.g;
    const int relu = a.relu;
    const float* __restrict__ row_m = a.saved;
    const float* __restrict__ row_r = a.saved + g.C;

    // the masked gradient of one element
    auto masked = [&](float G, float X, float B, float ca, float xr, float cb) {
        if (!relu) return G;
        return relu_open<T>(bn_act_value<T, ADD>(X, B, ca, xr, cb)) ? G : 0.f;
    };

    // ---- A': sum G' and sum G'*(x - mean) of every tile
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const BnActTile<VEC> t(g, tile);
        float acc[2][VEC], xr[VEC], rs[VEC], ca[VEC], cb[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[0][j] = acc[1][j] = xr[j] = rs[j] = ca[j] = cb[j] = 0.f;
        if (t.active) {
            load_planes<VEC>(row_m + t.ch(), xr);
            if (relu) {
                load_planes<VEC>(row_r + t.ch(), rs);
                bn_act_coefs<VEC>(a.bn, t.ch(), rs, ca, cb);
            }
            auto eat = [&](const Vec<T, VEC>& vg, const Vec<T, VEC>& vx, const Vec<T, VEC>& vb) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float X = to_float(vx.v[j]);
                    const float G = masked(to_float(vg.v[j]), X, to_float(vb.v[j]), ca[j], xr[j], cb[j]);
                    acc[0][j] += G;
                    acc[1][j] = fmaf(G, X - xr[j], acc[1][j]);
                }
            };
            constexpr int U = CNSN_NHWC_UB;
            int p = t.p0 + t.r;
            for (; p + (U - 1) * g.rows < t.p1; p += U * g.rows) {
                Vec<T, VEC> vg[U], vx[U], vb[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const size_t e = t.elem(g, p + u * g.rows);
                    vg[u] = nhwc_ld<T, VEC, !KEEP>(gy + e);
                    vx[u] = nhwc_ld<T, VEC, !KEEP>(x + e);
                    if constexpr (ADD) vb[u] = nhwc_ld<T, VEC, !KEEP>(addend + e);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) eat(vg[u], vx[u], ADD ? vb[u] : vx[u]);
            }
            for (; p < t.p1; p += g.rows) {
                const size_t e = t.elem(g, p);
                const Vec<T, VEC> vg = nhwc_ld<T, VEC, !KEEP>(gy + e), vx = nhwc_ld<T, VEC, !KEEP>(x + e);
                Vec<T, VEC> vb = vx;
                if constexpr (ADD) vb = nhwc_ld<T, VEC, !KEEP>(addend + e);
                eat(vg, vx, vb);
            }
        }
        bn_act_rows_sum<VEC, 2>(g, t, acc, lds, a.part);
    }
    const int ngroups = g.C / 4;
    if (!grid_barrier(a.bar, 1, &bar_flag)) {
        bn_act_mark_owed<T, VEC>(a, dx);
        if (threadIdx.x < 4) {  // the parameter gradients of the channel groups this workgroup owns
            const float nan = __builtin_nanf("");
            for (int slot = blockIdx.x; slot < ngroups; slot += gridDim.x) {
                const int c = phase_b_group(slot, ngroups) * 4 + (int)threadIdx.x;
                if (a.d_w) a.d_w[c] = nan;
                if (a.d_b) a.d_b[c] = nan;
            }
        }
        return;
    }

    // ---- B': the parameter gradients and the two dx coefficients per channel
    for (int slot = blockIdx.x; slot < ngroups; slot += gridDim.x) {
        const int c0 = phase_b_group(slot, ngroups) * 4;
        double acc[8];
        bn_act_gather(a, c0, acc, red);
        if (threadIdx.x == 0) {
            float o_x[4], o_0[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + q;
                const double S1 = acc[q], S2 = acc[4 + q], rstd = (double)row_r[c];
                const double av = (double)__fmul_rn(a.bn.weight[c], row_r[c]);
                if (a.d_b) a.d_b[c] = (float)S1;
                if (a.d_w) a.d_w[c] = (float)(rstd * S2);
                o_x[q] = (float)(-av * rstd * rstd * S2 * a.inv_r);
                o_0[q] = (float)(-av * S1 * a.inv_r);
            }
            const CohBuf cf(a.coef);  // (phase C' reads them)
            cf.st4((size_t)c0, o_x[0], o_x[1], o_x[2], o_x[3]);
            cf.st4((size_t)g.C + c0, o_0[0], o_0[1], o_0[2], o_0[3]);
        }
        __syncthreads();
    }
    if (!grid_barrier(a.bar, 2, &bar_flag)) {
        bn_act_mark_owed<T, VEC>(a, dx);
        return;
    }

    // ---- C': dx = a*G' + kx*(x - mean) + k0 (and d_addend = G'); the tiles in reverse order, every tile backwards
    const int mine = a.ntiles > (int)blockIdx.x ? (a.ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x : -1;
    const CohBuf cf(a.coef);
    for (int i = mine; i >= 0; --i) {
        const BnActTile<VEC> t(g, (int)blockIdx.x + i * (int)gridDim.x);
        if (!t.active) continue;
        float xr[VEC], rs[VEC], ca[VEC], cb[VEC], kx[VEC], k0[VEC];
        load_planes<VEC>(row_m + t.ch(), xr);
        load_planes<VEC>(row_r + t.ch(), rs);
        bn_act_coefs<VEC>(a.bn, t.ch(), rs, ca, cb);
        cf.load<VEC>((size_t)t.ch(), kx);
        cf.load<VEC>((size_t)g.C + t.ch(), k0);
        auto emit = [&](const Vec<T, VEC>& vg, const Vec<T, VEC>& vx, const Vec<T, VEC>& vb, size_t e) {
            Vec<T, VEC> o, om;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float X = to_float(vx.v[j]);
                const float G = masked(to_float(vg.v[j]), X, to_float(vb.v[j]), ca[j], xr[j], cb[j]);
                o.v[j] = from_float<T>(fmaf(ca[j], G, fmaf(kx[j], X - xr[j], k0[j])));
                om.v[j] = from_float<T>(G);
            }
            store_vec_nt<T, VEC>(dx + e, o);
            if constexpr (ADD) store_vec_nt<T, VEC>(d_addend + e, om);
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
                if constexpr (ADD) vb[u] = load_vec_nt<T, VEC>(addend + e);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) emit(vg[u], vx[u], ADD ? vb[u] : vx[u], t.elem(g, t.p0 + t.r + (q - u) * g.rows));
        }
        for (; q >= 0; --q) {
            const size_t e = t.elem(g, t.p0 + t.r + q * g.rows);
            const Vec<T, VEC> vg = load_vec_nt<T, VEC>(gy + e), vx = load_vec_nt<T, VEC>(x + e);
            Vec<T, VEC> vb = vx;
            if constexpr (ADD) vb = load_vec_nt<T, VEC>(addend + e);
            emit(vg, vx, vb, e);
        }
    }
}

}  // namespace cnsn
