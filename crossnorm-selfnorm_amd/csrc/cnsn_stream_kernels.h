// Streaming ("two-pass") kernels: every tensor pass of the fused op as one bandwidth-bound launch.
//
//   forward : plane_stats_kernel (read x)  -> mid_fwd_kernel (N*C scalars) -> apply_fwd_kernel (read x, write y)
//   backward: bwd_reduce_kernel (read G,x) -> mid_bwd_a/b (N*C scalars)    -> apply_bwd_kernel (read G,x, write dx)
//
// Thread mapping (all kernels): a plane (H*W contiguous elements of one (n,c)) is owned by LPP
// consecutive lanes — 16 (one DPP row), 64 (one wave) or 256 (the block) — chosen on the host from
// the plane size so that every lane issues full-width vector loads (VEC elements = up to 16 B) and
// the per-plane reduction never leaves registers/DPP for LPP <= 64.  Loads are issued UNROLL at a
// time before any is consumed, so each lane keeps UNROLL*16 B in flight.
//
// T = double instantiates the float64 path: the same kernels with every accumulator, coefficient and side array double
// (acc_t<T>, cnsn_device.h).  Eight-byte elements halve the elements per load, not the bytes.
#pragma once
#include <type_traits>

#include "cnsn_device.h"
#include "cnsn_layout.h"

namespace cnsn {

#ifndef CNSN_UNROLL
#define CNSN_UNROLL 4
#endif
constexpr int kUnroll = CNSN_UNROLL;

// stream one plane: consume(vec, vec_index)
template <typename T, int VEC, int LPP, bool NT = false, typename Consume>
__device__ __forceinline__ void stream1(const T* __restrict__ base, int nvec, int lane, Consume&& consume, bool keep = false) {
    // keep (workgroup-uniform): default cache policy although NT — the first pass over a tensor small enough for the
    // second pass to find it in L2 / the Infinity Cache
    if (NT && keep) {
        stream1<T, VEC, LPP, false>(base, nvec, lane, consume);
        return;
    }
    int i = lane;
    for (; i + (kUnroll - 1) * LPP < nvec; i += kUnroll * LPP) {
        Vec<T, VEC> v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            v[u] = NT ? load_vec_nt<T, VEC>(base + (size_t)(i + u * LPP) * VEC) : load_vec<T, VEC>(base + (size_t)(i + u * LPP) * VEC);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) consume(v[u], i + u * LPP);
    }
    for (; i < nvec; i += LPP) {
        Vec<T, VEC> v = NT ? load_vec_nt<T, VEC>(base + (size_t)i * VEC) : load_vec<T, VEC>(base + (size_t)i * VEC);
        consume(v, i);
    }
}

// stream two planes in lock step: consume(vecA, vecB, vec_index)
template <typename T, int VEC, int LPP, bool NT = false, typename Consume>
__device__ __forceinline__ void stream2(const T* __restrict__ a, const T* __restrict__ b, int nvec, int lane,
                                        Consume&& consume, bool keep = false) {
    if (NT && keep) {
        stream2<T, VEC, LPP, false>(a, b, nvec, lane, consume);
        return;
    }
    constexpr int U = kUnroll / 2;
    int i = lane;
    for (; i + (U - 1) * LPP < nvec; i += U * LPP) {
        Vec<T, VEC> va[U], vb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            va[u] = NT ? load_vec_nt<T, VEC>(a + (size_t)(i + u * LPP) * VEC) : load_vec<T, VEC>(a + (size_t)(i + u * LPP) * VEC);
            vb[u] = NT ? load_vec_nt<T, VEC>(b + (size_t)(i + u * LPP) * VEC) : load_vec<T, VEC>(b + (size_t)(i + u * LPP) * VEC);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) consume(va[u], vb[u], i + u * LPP);
    }
    for (; i < nvec; i += LPP) {
        Vec<T, VEC> va = NT ? load_vec_nt<T, VEC>(a + (size_t)i * VEC) : load_vec<T, VEC>(a + (size_t)i * VEC);
        Vec<T, VEC> vb = NT ? load_vec_nt<T, VEC>(b + (size_t)i * VEC) : load_vec<T, VEC>(b + (size_t)i * VEC);
        consume(va, vb, i);
    }
}

typedef float pk2f __attribute__((ext_vector_type(2)));

template <int LPP>
struct PlaneId {
    int p;       // plane index (clamped so that idle lanes still take part in reductions)
    int lane;    // lane within the plane's group
    bool valid;  // p is a real plane
    __device__ __forceinline__ explicit PlaneId(int P) {
        constexpr int PPB = kBlock / LPP;
        const int q = blockIdx.x * PPB + threadIdx.x / LPP;
        lane = threadIdx.x % LPP;
        valid = q < P;
        p = valid ? q : P - 1;
    }
};

// ------------------------------------------------------------------------------------------------
// pass A: plane statistics (reference: calc_ins_mean_std, models/cnsn.py:14-16)
//   un-boxed: out[0]=mean, out[1]=M2 of the whole plane
//   boxed   : out[0..5] = mean/M2 inside the content box, outside it, inside the style box
//   fin != NULL: fin[0]=mean, fin[1]=sqrt(M2/(cnt-1)+eps) of the (content-box) region, as acc_t<T>
//   moments are written as double: the mid kernels keep every per-plane scalar in double
// Sums are taken about a per-plane shift K so that S2 - S1^2/cnt does not cancel for planes with
// |mean| >> std (post-ReLU activations): the median of the means of the three vectors that hold the plane's
// sample pixels (plane_shift; the shift of cnsn_device.h).
// ------------------------------------------------------------------------------------------------
// the shift of a plane's sums; load(e): the mean of the VEC elements from element e of the plane (e a multiple of VEC, and VEC
// divides the plane: the vector lies inside it)
template <int VEC, typename Load>
__device__ __forceinline__ auto plane_shift(const Geom& g, Load&& load) {
    decltype(load((size_t)0)) s[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) s[i] = load((size_t)(shift_sample_pixel(g.M / g.Wd, g.Wd, i) / VEC) * VEC);
    return median3(s[0], s[1], s[2]);
}

template <typename T, int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void plane_stats_kernel(const T* __restrict__ x, Geom g,
                                                             double* __restrict__ mom, acc_t<T>* __restrict__ fin,
                                                             acc_t<T> eps) {
    using A = acc_t<T>;
    constexpr int NACC = BOXED ? 6 : 2;
    __shared__ A lds[4 * NACC];
    const PlaneId<LPP> id(g.P);
    const T* base = x + (size_t)id.p * g.M;

    const A K = plane_shift<VEC>(g, [&](size_t e) {
        const Vec<T, VEC> f = load_vec<T, VEC>(base + e);
        A m = 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) m += to_acc(f.v[j]);
        return m * (A(1) / VEC);
    });
    // one accumulator per vector slot: VEC short chains instead of one long one (rounding error of
    // a sequential fp32 sum grows with its length), folded pairwise afterwards
    A part[NACC][VEC];
#pragma unroll
    for (int k = 0; k < NACC; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[k][j] = 0;

    stream1<T, VEC, LPP, true>(base, g.nvec, id.lane, [&](const Vec<T, VEC>& v, int i) {
        if constexpr (!BOXED) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const A d = to_acc(v.v[j]) - K;
                part[0][j] += d;
                part[1][j] = fma(d, d, part[1][j]);
            }
        } else {
            // boxed: the kernel is VALU-bound for 16-bit tensors, so the per-element work is kept minimal — the row
            // tests are per vector (VEC divides the width: a vector lies in one row), membership becomes a 0/1
            // factor, and the sums OUTSIDE the content box are obtained as (whole plane) - (inside) afterwards
            // (all sums are about the same shift K, so the subtraction does not cancel catastrophically; what it
            // loses is scaled by the weight Mo/M the outside region has in the merged statistics)
            const int e = i * VEC;
            const int r = e / g.Wd, c = e - r * g.Wd;
            const bool row_c = (unsigned)(r - g.cb.r0) < (unsigned)(g.cb.r1 - g.cb.r0);
            const bool row_s = (unsigned)(r - g.sb.r0) < (unsigned)(g.sb.r1 - g.sb.r0);
            const unsigned wc = row_c ? (unsigned)(g.cb.c1 - g.cb.c0) : 0u, ws = row_s ? (unsigned)(g.sb.c1 - g.sb.c0) : 0u;
            const int cc = c - g.cb.c0, cs = c - g.sb.c0;
            if constexpr (VEC >= 2 && std::is_same_v<A, float>) {
                // two elements per instruction (v_pk_add/mul/fma_f32): the accumulators of slots j, j+1 as a pair
#pragma unroll
                for (int j = 0; j < VEC; j += 2) {
                    const pk2f d = pk2f{to_float(v.v[j]), to_float(v.v[j + 1])} - pk2f{K, K};
                    const pk2f d2 = d * d;
                    const pk2f mc = {(unsigned)(cc + j) < wc ? 1.f : 0.f, (unsigned)(cc + j + 1) < wc ? 1.f : 0.f};
                    const pk2f ms = {(unsigned)(cs + j) < ws ? 1.f : 0.f, (unsigned)(cs + j + 1) < ws ? 1.f : 0.f};
                    pk2f a0 = {part[0][j], part[0][j + 1]}, a1 = {part[1][j], part[1][j + 1]};
                    pk2f a2 = {part[2][j], part[2][j + 1]}, a3 = {part[3][j], part[3][j + 1]};
                    pk2f a4 = {part[4][j], part[4][j + 1]}, a5 = {part[5][j], part[5][j + 1]};
                    a0 = __builtin_elementwise_fma(mc, d, a0);
                    a1 = __builtin_elementwise_fma(mc, d2, a1);
                    a2 += d;   // whole plane here; the inside is subtracted below
                    a3 += d2;
                    a4 = __builtin_elementwise_fma(ms, d, a4);
                    a5 = __builtin_elementwise_fma(ms, d2, a5);
                    part[0][j] = a0.x, part[0][j + 1] = a0.y, part[1][j] = a1.x, part[1][j + 1] = a1.y;
                    part[2][j] = a2.x, part[2][j + 1] = a2.y, part[3][j] = a3.x, part[3][j + 1] = a3.y;
                    part[4][j] = a4.x, part[4][j + 1] = a4.y, part[5][j] = a5.x, part[5][j + 1] = a5.y;
                }
            } else {  // one-element vectors, and double (no packed double instructions)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const A d = to_acc(v.v[j]) - K;
                    const A d2 = d * d;
                    const A mc = (unsigned)(cc + j) < wc ? A(1) : A(0), ms = (unsigned)(cs + j) < ws ? A(1) : A(0);
                    part[0][j] = fma(mc, d, part[0][j]);
                    part[1][j] = fma(mc, d2, part[1][j]);
                    part[2][j] += d;
                    part[3][j] += d2;
                    part[4][j] = fma(ms, d, part[4][j]);
                    part[5][j] = fma(ms, d2, part[5][j]);
                }
            }
        }
    }, g.keep != 0);
    A acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
#pragma unroll
        for (int w = VEC / 2; w > 0; w >>= 1)
#pragma unroll
            for (int j = 0; j < w; ++j) part[k][j] += part[k][j + w];
        acc[k] = part[k][0];
    }
    group_sum<LPP, NACC>(acc, lds);
    if constexpr (BOXED) {  // outside = whole plane - inside
        acc[2] -= acc[0];
        acc[3] -= acc[1];
    }

    if (id.lane == 0 && id.valid) {
        auto moments = [&](A s1, A s2, int cnt, double& mean, double& m2) {
            if (cnt <= 0) {
                mean = 0.0;
                m2 = 0.0;
                return;
            }
            const double d1 = s1, d2 = s2;
            mean = double(K) + d1 / cnt;
            const double t = d2 - d1 * d1 / cnt;
            m2 = t > 0.0 ? t : 0.0;
        };
        const size_t P = g.P;
        const int Mc = BOXED ? g.cb.area() : g.M;
        double mean, m2;
        moments(acc[0], acc[1], Mc, mean, m2);
        if (fin) {  // stand-alone calc_ins_mean_std: (mean, std) of the (boxed) region
            fin[id.p] = (A)mean;
            fin[P + id.p] = (A)sqrt(m2 / double(Mc - 1) + (double)eps);
        } else {
            mom[id.p] = mean;
            mom[P + id.p] = m2;
            if constexpr (BOXED) {
                moments(acc[2], acc[3], g.M - Mc, mean, m2);
                mom[2 * P + id.p] = mean;
                mom[3 * P + id.p] = m2;
                moments(acc[4], acc[5], g.sb.area(), mean, m2);
                mom[4 * P + id.p] = mean;
                mom[5 * P + id.p] = m2;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// pass B: y = a_in*(x - xr) + b_in inside the content box, a_out*x + b_out outside
// (reference: instance_norm_mix :27-29, the box paste :75-82, the lam blend :87, SelfNorm :148/:150
//  — all folded into five per-plane coefficients by mid_fwd_kernel).  xr may be NULL (= 0).
// ------------------------------------------------------------------------------------------------
template <typename S>
struct ApplyCoefT {
    const S* a_in;
    const S* xr;
    const S* b_in;
    const S* a_out;
    const S* b_out;
};
using ApplyCoef = ApplyCoefT<float>;

template <typename T, int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void apply_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, Geom g,
                                                           ApplyCoefT<acc_t<T>> cf) {
    using A = acc_t<T>;
    const PlaneId<LPP> id(g.P);
    if (!id.valid) return;
    const size_t off = (size_t)id.p * g.M;
    const A a_in = cf.a_in[id.p], xr = cf.xr ? cf.xr[id.p] : A(0), b_in = cf.b_in[id.p];
    A a_out = 0, b_out = 0;
    if constexpr (BOXED) {
        a_out = cf.a_out[id.p];
        b_out = cf.b_out[id.p];
    }
    T* yb = y + off;
    stream1<T, VEC, LPP, true>(x + off, g.nvec, id.lane, [&](const Vec<T, VEC>& v, int i) {
        Vec<T, VEC> o;
        if constexpr (!BOXED) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) o.v[j] = from_acc<T>(fma(a_in, to_acc(v.v[j]) - xr, b_in));
        } else {
            const int e = i * VEC;
            const int r = e / g.Wd, c = e - r * g.Wd;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const A f = to_acc(v.v[j]);
                o.v[j] = from_acc<T>(g.cb.has(r, c + j) ? fma(a_in, f - xr, b_in) : fma(a_out, f, b_out));
            }
        }
        store_vec_nt<T, VEC>(yb + (size_t)i * VEC, o);
    });
}

// ------------------------------------------------------------------------------------------------
// pass A': per-plane sums of the upstream gradient G against x
//   un-boxed: out[0]=sum G, out[1]=sum G*(x-shift_in)
//   boxed   : out[0..3] = the same inside the content box (shift_in) and outside it (shift_out)
// shift pointers may be NULL (= 0).  The shifts are rounded to acc_t<T> (T = double: not at all); fix_sums undoes the rounding.
// ------------------------------------------------------------------------------------------------
template <typename T, int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void bwd_reduce_kernel(const T* __restrict__ gy, const T* __restrict__ x, Geom g,
                                                            const double* __restrict__ shift_in,
                                                            const double* __restrict__ shift_out, int shift_stride,
                                                            acc_t<T>* __restrict__ out) {
    using A = acc_t<T>;
    constexpr int NACC = BOXED ? 4 : 2;
    __shared__ A lds[4 * NACC];
    const PlaneId<LPP> id(g.P);
    const size_t off = (size_t)id.p * g.M;
    // shifts: a plain array over the planes (shift_stride 1), or rows of `saved` (shift_stride 0: the pointers are the
    // rows' starts, cnsn_layout.h); mid_bwd_a undoes the rounding
    const size_t srec = shift_stride == 1 ? (size_t)id.p : sv_rec_of_plane((size_t)id.p, g.N, g.C).base;
    const A si = shift_in ? (A)shift_in[srec] : A(0);
    const A so = (BOXED && shift_out) ? (A)shift_out[srec] : A(0);
    A part[NACC][VEC];
#pragma unroll
    for (int k = 0; k < NACC; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[k][j] = 0;
    stream2<T, VEC, LPP, true>(gy + off, x + off, g.nvec, id.lane,
                         [&](const Vec<T, VEC>& vg, const Vec<T, VEC>& vx, int i) {
                             if constexpr (!BOXED) {
#pragma unroll
                                 for (int j = 0; j < VEC; ++j) {
                                     const A G = to_acc(vg.v[j]);
                                     part[0][j] += G;
                                     part[1][j] = fma(G, to_acc(vx.v[j]) - si, part[1][j]);
                                 }
                             } else {  // (see plane_stats_kernel: row test per vector, 0/1 factor, outside = whole - inside)
                                 const int e = i * VEC;
                                 const int r = e / g.Wd, c = e - r * g.Wd;
                                 const unsigned wc = (unsigned)(r - g.cb.r0) < (unsigned)(g.cb.r1 - g.cb.r0)
                                                         ? (unsigned)(g.cb.c1 - g.cb.c0)
                                                         : 0u;
#pragma unroll
                                 for (int j = 0; j < VEC; ++j) {
                                     const A G = to_acc(vg.v[j]), X = to_acc(vx.v[j]);
                                     const A mc = (unsigned)(c + j - g.cb.c0) < wc ? A(1) : A(0);
                                     const A pr = G * (X - si);
                                     part[0][j] = fma(mc, G, part[0][j]);
                                     part[1][j] = fma(mc, pr, part[1][j]);
                                     part[2][j] += G;
                                     part[3][j] += pr;
                                 }
                             }
                         }, g.keep != 0);
    A acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
#pragma unroll
        for (int w = VEC / 2; w > 0; w >>= 1)
#pragma unroll
            for (int j = 0; j < w; ++j) part[k][j] += part[k][j + w];
        acc[k] = part[k][0];
    }
    group_sum<LPP, NACC>(acc, lds);
    if constexpr (BOXED) {  // sum_out G*(X-so) = sum_out G*(X-si) - (so-si)*sum_out G
        acc[2] -= acc[0];
        acc[3] = (acc[3] - acc[1]) - (so - si) * acc[2];
    }
    if (id.lane == 0 && id.valid) {
#pragma unroll
        for (int k = 0; k < NACC; ++k) out[(size_t)k * g.P + id.p] = acc[k];
    }
}

// ------------------------------------------------------------------------------------------------
// pass B': dx = cG*G + cX*(x - xr) + c0, coefficients by region (inside / outside the content
// box), plus eS*(x - xs) + e0 inside the style box (the gradient a plane receives for having been
// another instance's style source).  Coefficients: the BC_* rows of `coef`, stride P (see mid_bwd_b).
// ------------------------------------------------------------------------------------------------
template <typename T, int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void apply_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                                                           T* __restrict__ dx, Geom g,
                                                           const acc_t<T>* __restrict__ coef) {
    using A = acc_t<T>;
    const PlaneId<LPP> id(g.P);
    if (!id.valid) return;
    const size_t off = (size_t)id.p * g.M;
    const size_t P = g.P;
    const A cG_i = coef[BC_CG_IN * P + id.p], cX_i = coef[BC_CX_IN * P + id.p], xr_i = coef[BC_XR_IN * P + id.p],
            c0_i = coef[BC_C0_IN * P + id.p];
    A cG_o = 0, cX_o = 0, xr_o = 0, c0_o = 0, eS = 0, xs = 0, e0 = 0;
    if constexpr (BOXED) {
        cG_o = coef[BC_CG_OUT * P + id.p];
        cX_o = coef[BC_CX_OUT * P + id.p];
        xr_o = coef[BC_XR_OUT * P + id.p];
        c0_o = coef[BC_C0_OUT * P + id.p];
        eS = coef[BC_ES * P + id.p];
        xs = coef[BC_XS * P + id.p];
        e0 = coef[BC_E0 * P + id.p];
    }
    T* db = dx + off;
    stream2<T, VEC, LPP, true>(gy + off, x + off, g.nvec, id.lane,
                         [&](const Vec<T, VEC>& vg, const Vec<T, VEC>& vx, int i) {
                             Vec<T, VEC> o;
                             if constexpr (!BOXED) {
#pragma unroll
                                 for (int j = 0; j < VEC; ++j) {
                                     const A G = to_acc(vg.v[j]), X = to_acc(vx.v[j]);
                                     o.v[j] = from_acc<T>(fma(cG_i, G, fma(cX_i, X - xr_i, c0_i)));
                                 }
                             } else {
                                 const int e = i * VEC;
                                 const int r = e / g.Wd, c = e - r * g.Wd;
#pragma unroll
                                 for (int j = 0; j < VEC; ++j) {
                                     const A G = to_acc(vg.v[j]), X = to_acc(vx.v[j]);
                                     const bool ic = g.cb.has(r, c + j), is = g.sb.has(r, c + j);
                                     A d = ic ? fma(cG_i, G, fma(cX_i, X - xr_i, c0_i)) : fma(cG_o, G, fma(cX_o, X - xr_o, c0_o));
                                     d += is ? fma(eS, X - xs, e0) : A(0);
                                     o.v[j] = from_acc<T>(d);
                                 }
                             }
                             store_vec_nt<T, VEC>(db + (size_t)i * VEC, o);
                         });
}

// ------------------------------------------------------------------------------------------------
// backward of calc_ins_mean_std alone: dx = dmean/cnt + dstd*(x-mean)/(std*(cnt-1)) in the box, else 0
// ------------------------------------------------------------------------------------------------
template <typename T, int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void plane_stats_bwd_kernel(const T* __restrict__ x, T* __restrict__ dx, Geom g,
                                                                 const acc_t<T>* __restrict__ mean,
                                                                 const acc_t<T>* __restrict__ std,
                                                                 const acc_t<T>* __restrict__ dmean,
                                                                 const acc_t<T>* __restrict__ dstd) {
    using A = acc_t<T>;
    const PlaneId<LPP> id(g.P);
    if (!id.valid) return;
    const size_t off = (size_t)id.p * g.M;
    const int cnt = BOXED ? g.cb.area() : g.M;
    const A mu = mean[id.p];
    const A cX = dstd[id.p] / (std[id.p] * A(cnt - 1));
    const A c0 = dmean[id.p] / A(cnt);
    T* db = dx + off;
    stream1<T, VEC, LPP, true>(x + off, g.nvec, id.lane, [&](const Vec<T, VEC>& v, int i) {
        Vec<T, VEC> o;
        const int e = i * VEC;
        const int r = BOXED ? e / g.Wd : 0, c = BOXED ? e - r * g.Wd : 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const A d = fma(cX, to_acc(v.v[j]) - mu, c0);
            o.v[j] = from_acc<T>((!BOXED || g.cb.has(r, c + j)) ? d : A(0));
        }
        store_vec_nt<T, VEC>(db + (size_t)i * VEC, o);
    });
}

}  // namespace cnsn
