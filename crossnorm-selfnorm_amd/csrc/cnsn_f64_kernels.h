// The float64 path: the two-pass streaming scheme of cnsn_stream_kernels.h / cnsn_mid_kernels.h for `double` tensors.
//
//   forward : plane_stats_f64_kernel (read x)  -> mid_fwd_f64_kernel (N*C scalars) -> apply_fwd_f64_kernel (read x, write y)
//   backward: bwd_reduce_f64_kernel (read G,x) -> mid_bwd_a/b_f64 (N*C scalars)    -> apply_bwd_f64_kernel (read G,x, write dx)
//
// Same thread mapping (LPP lanes per plane, UNROLL loads of 16 bytes in flight per lane: stream1 / stream2 with T = double, VEC = 2
// where the plane — with crop boxes: the row — is even, else 1), same cache policy (non-temporal second pass, keep_first_read).
// What differs from the float kernels: every accumulator, every per-plane coefficient, the gate's parameters, the running
// statistics, the parameter gradients and the scalars of the launch are double, so nothing between the tensor and the R = double
// algebra of cnsn_algebra.h is rounded to float.  Eight-byte elements halve the elements per load, not the bytes: the kernels
// stay bound by memory (a plane element costs a handful of double FMAs against 8-24 bytes of traffic).
#pragma once
#include "cnsn_algebra.h"
#include "cnsn_device.h"
#include "cnsn_layout.h"
#include "cnsn_stream_kernels.h"

namespace cnsn {

// MidArgs with double scalars: float(0.3) is 1e-8 away from 0.3
struct MidArgsD {
    int N, C, M;
    int Mc, Ms;
    int cn_active, boxed, sn_active, sn_two, sn_training;
    double lam, eps_cn, eps_sn, eps_bn, momentum;
    double inv_n;
    double unbias_n;
    int save_coefs;
};

struct GateDevD {
    const double* w;
    const double* gamma;
    const double* beta;
    double* run_mean;
    double* run_var;
    long long* nbt;
};
struct GateGradDevD {
    double* dw;
    double* dgamma;
    double* dbeta;
};

__device__ __forceinline__ double median3_d(double a, double b, double c) { return fmax(fmin(a, b), fmin(fmax(a, b), c)); }

// Sum NACC doubles over the LPP lanes that share a plane; `lds` needs 4*NACC doubles when LPP == 256.  Every lane of the
// group gets the result, and every lane of a group adds in the same order: the sums do not depend on the grid.
template <int LPP, int NACC>
__device__ __forceinline__ void group_sum_d(double (&acc)[NACC], double* lds) {
    constexpr int W = LPP < 64 ? LPP : 64;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        acc[k] = v;
    }
    if constexpr (LPP == 256) {
        const int wave = threadIdx.x >> 6;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < NACC; ++k) lds[wave * NACC + k] = acc[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[k] = (lds[k] + lds[NACC + k]) + (lds[2 * NACC + k] + lds[3 * NACC + k]);
    } else {
        static_assert(LPP == 16 || LPP == 64, "lanes per plane must be 16, 64 or 256");
    }
}

// ------------------------------------------------------------------------------------------------
// pass A: plane statistics in double about the median-of-three shift (cnsn_device.h).  Outputs as plane_stats_kernel:
//   mom[0..1] (boxed: [0..5]) = mean / M2 of the content box, outside it, the style box; or fin = (mean, std), double.
// The sums outside the content box are accumulated for themselves (a second 0/1 factor), not as whole - inside.
// ------------------------------------------------------------------------------------------------
template <int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void plane_stats_f64_kernel(const double* __restrict__ x, Geom g, double* __restrict__ mom,
                                                                 double* __restrict__ fin, double eps) {
    constexpr int NACC = BOXED ? 6 : 2;
    __shared__ double lds[4 * NACC];
    const PlaneId<LPP> id(g.P);
    const double* base = x + (size_t)id.p * g.M;

    double s[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const Vec<double, VEC> f = load_vec<double, VEC>(base + (size_t)(shift_sample_pixel(g.M / g.Wd, g.Wd, i) / VEC) * VEC);
        double m = 0.0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) m += f.v[j];
        s[i] = m * (1.0 / VEC);
    }
    const double K = median3_d(s[0], s[1], s[2]);

    double part[NACC][VEC];
#pragma unroll
    for (int k = 0; k < NACC; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[k][j] = 0.0;

    stream1<double, VEC, LPP, true>(base, g.nvec, id.lane, [&](const Vec<double, VEC>& v, int i) {
        if constexpr (!BOXED) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const double d = v.v[j] - K;
                part[0][j] += d;
                part[1][j] = fma(d, d, part[1][j]);
            }
        } else {  // (VEC divides the width: a vector lies in one row)
            const int e = i * VEC;
            const int r = e / g.Wd, c = e - r * g.Wd;
            const bool row_c = (unsigned)(r - g.cb.r0) < (unsigned)(g.cb.r1 - g.cb.r0);
            const bool row_s = (unsigned)(r - g.sb.r0) < (unsigned)(g.sb.r1 - g.sb.r0);
            const unsigned wc = row_c ? (unsigned)(g.cb.c1 - g.cb.c0) : 0u, ws = row_s ? (unsigned)(g.sb.c1 - g.sb.c0) : 0u;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const double d = v.v[j] - K, d2 = d * d;
                const double mc = (unsigned)(c + j - g.cb.c0) < wc ? 1.0 : 0.0, mo = 1.0 - mc;
                const double ms = (unsigned)(c + j - g.sb.c0) < ws ? 1.0 : 0.0;
                part[0][j] = fma(mc, d, part[0][j]);
                part[1][j] = fma(mc, d2, part[1][j]);
                part[2][j] = fma(mo, d, part[2][j]);
                part[3][j] = fma(mo, d2, part[3][j]);
                part[4][j] = fma(ms, d, part[4][j]);
                part[5][j] = fma(ms, d2, part[5][j]);
            }
        }
    }, g.keep != 0);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        acc[k] = part[k][0];
#pragma unroll
        for (int j = 1; j < VEC; ++j) acc[k] += part[k][j];
    }
    group_sum_d<LPP, NACC>(acc, lds);

    if (id.lane == 0 && id.valid) {
        auto moments = [&](double s1, double s2, int cnt, double& mean, double& m2) {
            if (cnt <= 0) {
                mean = 0.0;
                m2 = 0.0;
                return;
            }
            mean = K + s1 / cnt;
            const double t = s2 - s1 * s1 / cnt;
            m2 = t > 0.0 ? t : 0.0;
        };
        const size_t P = g.P;
        const int Mc = BOXED ? g.cb.area() : g.M;
        double mean, m2;
        moments(acc[0], acc[1], Mc, mean, m2);
        if (fin) {
            fin[id.p] = mean;
            fin[P + id.p] = sqrt(m2 / double(Mc - 1) + eps);
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
// pass B: y = a_in*(x - xr) + b_in inside the content box, a_out*x + b_out outside.  xr may be NULL (= 0).
// ------------------------------------------------------------------------------------------------
struct ApplyCoefD {
    const double* a_in;
    const double* xr;
    const double* b_in;
    const double* a_out;
    const double* b_out;
};

template <int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void apply_fwd_f64_kernel(const double* __restrict__ x, double* __restrict__ y, Geom g,
                                                               ApplyCoefD cf) {
    const PlaneId<LPP> id(g.P);
    if (!id.valid) return;
    const size_t off = (size_t)id.p * g.M;
    const double a_in = cf.a_in[id.p], xr = cf.xr ? cf.xr[id.p] : 0.0, b_in = cf.b_in[id.p];
    double a_out = 0.0, b_out = 0.0;
    if constexpr (BOXED) {
        a_out = cf.a_out[id.p];
        b_out = cf.b_out[id.p];
    }
    double* yb = y + off;
    stream1<double, VEC, LPP, true>(x + off, g.nvec, id.lane, [&](const Vec<double, VEC>& v, int i) {
        Vec<double, VEC> o;
        if constexpr (!BOXED) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) o.v[j] = fma(a_in, v.v[j] - xr, b_in);
        } else {
            const int e = i * VEC;
            const int r = e / g.Wd, c = e - r * g.Wd;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                o.v[j] = g.cb.has(r, c + j) ? fma(a_in, v.v[j] - xr, b_in) : fma(a_out, v.v[j], b_out);
        }
        store_vec_nt<double, VEC>(yb + (size_t)i * VEC, o);
    });
}

// ------------------------------------------------------------------------------------------------
// pass A': per-plane sums of the upstream gradient G against x
//   un-boxed: out[0] = sum G, out[1] = sum G*(x - shift_in)
//   boxed   : out[0..3] = the same inside the content box (shift_in) and outside it (shift_out)
// The shifts are the plane means as doubles: nothing for the mid kernel to undo.  Pointers may be NULL (= 0); shift_stride as
// in bwd_reduce_kernel (1: a plain array over the planes, 0: rows of `saved`).
// ------------------------------------------------------------------------------------------------
template <int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void bwd_reduce_f64_kernel(const double* __restrict__ gy, const double* __restrict__ x, Geom g,
                                                                const double* __restrict__ shift_in,
                                                                const double* __restrict__ shift_out, int shift_stride,
                                                                double* __restrict__ out) {
    constexpr int NACC = BOXED ? 4 : 2;
    __shared__ double lds[4 * NACC];
    const PlaneId<LPP> id(g.P);
    const size_t off = (size_t)id.p * g.M;
    const size_t srec = shift_stride == 1 ? (size_t)id.p : sv_rec_of_plane((size_t)id.p, g.N, g.C).base;
    const double si = shift_in ? shift_in[srec] : 0.0;
    const double so = (BOXED && shift_out) ? shift_out[srec] : 0.0;
    double part[NACC][VEC];
#pragma unroll
    for (int k = 0; k < NACC; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[k][j] = 0.0;
    stream2<double, VEC, LPP, true>(gy + off, x + off, g.nvec, id.lane,
                                    [&](const Vec<double, VEC>& vg, const Vec<double, VEC>& vx, int i) {
                                        if constexpr (!BOXED) {
#pragma unroll
                                            for (int j = 0; j < VEC; ++j) {
                                                part[0][j] += vg.v[j];
                                                part[1][j] = fma(vg.v[j], vx.v[j] - si, part[1][j]);
                                            }
                                        } else {
                                            const int e = i * VEC;
                                            const int r = e / g.Wd, c = e - r * g.Wd;
                                            const unsigned wc = (unsigned)(r - g.cb.r0) < (unsigned)(g.cb.r1 - g.cb.r0)
                                                                    ? (unsigned)(g.cb.c1 - g.cb.c0)
                                                                    : 0u;
#pragma unroll
                                            for (int j = 0; j < VEC; ++j) {
                                                const double G = vg.v[j], X = vx.v[j];
                                                const bool in = (unsigned)(c + j - g.cb.c0) < wc;
                                                const double Gi = in ? G : 0.0, Go = in ? 0.0 : G;
                                                part[0][j] += Gi;
                                                part[1][j] = fma(Gi, X - si, part[1][j]);
                                                part[2][j] += Go;
                                                part[3][j] = fma(Go, X - so, part[3][j]);
                                            }
                                        }
                                    }, g.keep != 0);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        acc[k] = part[k][0];
#pragma unroll
        for (int j = 1; j < VEC; ++j) acc[k] += part[k][j];
    }
    group_sum_d<LPP, NACC>(acc, lds);
    if (id.lane == 0 && id.valid) {
#pragma unroll
        for (int k = 0; k < NACC; ++k) out[(size_t)k * g.P + id.p] = acc[k];
    }
}

// ------------------------------------------------------------------------------------------------
// pass B': dx = cG*G + cX*(x - xr) + c0 by region, + eS*(x - xs) + e0 inside the style box; coef: BC_ROWS rows of P doubles
// ------------------------------------------------------------------------------------------------
template <int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void apply_bwd_f64_kernel(const double* __restrict__ gy, const double* __restrict__ x,
                                                               double* __restrict__ dx, Geom g, const double* __restrict__ coef) {
    const PlaneId<LPP> id(g.P);
    if (!id.valid) return;
    const size_t off = (size_t)id.p * g.M;
    const size_t P = g.P;
    const double cG_i = coef[BC_CG_IN * P + id.p], cX_i = coef[BC_CX_IN * P + id.p], xr_i = coef[BC_XR_IN * P + id.p],
                 c0_i = coef[BC_C0_IN * P + id.p];
    double cG_o = 0.0, cX_o = 0.0, xr_o = 0.0, c0_o = 0.0, eS = 0.0, xs = 0.0, e0 = 0.0;
    if constexpr (BOXED) {
        cG_o = coef[BC_CG_OUT * P + id.p];
        cX_o = coef[BC_CX_OUT * P + id.p];
        xr_o = coef[BC_XR_OUT * P + id.p];
        c0_o = coef[BC_C0_OUT * P + id.p];
        eS = coef[BC_ES * P + id.p];
        xs = coef[BC_XS * P + id.p];
        e0 = coef[BC_E0 * P + id.p];
    }
    double* db = dx + off;
    stream2<double, VEC, LPP, true>(gy + off, x + off, g.nvec, id.lane,
                                    [&](const Vec<double, VEC>& vg, const Vec<double, VEC>& vx, int i) {
                                        Vec<double, VEC> o;
                                        if constexpr (!BOXED) {
#pragma unroll
                                            for (int j = 0; j < VEC; ++j)
                                                o.v[j] = fma(cG_i, vg.v[j], fma(cX_i, vx.v[j] - xr_i, c0_i));
                                        } else {
                                            const int e = i * VEC;
                                            const int r = e / g.Wd, c = e - r * g.Wd;
#pragma unroll
                                            for (int j = 0; j < VEC; ++j) {
                                                const double G = vg.v[j], X = vx.v[j];
                                                double d = g.cb.has(r, c + j) ? fma(cG_i, G, fma(cX_i, X - xr_i, c0_i))
                                                                              : fma(cG_o, G, fma(cX_o, X - xr_o, c0_o));
                                                d += g.sb.has(r, c + j) ? fma(eS, X - xs, e0) : 0.0;
                                                o.v[j] = d;
                                            }
                                        }
                                        store_vec_nt<double, VEC>(db + (size_t)i * VEC, o);
                                    });
}

// backward of calc_ins_mean_std alone: dx = dmean/cnt + dstd*(x-mean)/(std*(cnt-1)) in the box, else 0
template <int VEC, int LPP, bool BOXED>
__global__ __launch_bounds__(kBlock) void plane_stats_bwd_f64_kernel(const double* __restrict__ x, double* __restrict__ dx, Geom g,
                                                                     const double* __restrict__ mean, const double* __restrict__ std,
                                                                     const double* __restrict__ dmean,
                                                                     const double* __restrict__ dstd) {
    const PlaneId<LPP> id(g.P);
    if (!id.valid) return;
    const size_t off = (size_t)id.p * g.M;
    const int cnt = BOXED ? g.cb.area() : g.M;
    const double mu = mean[id.p];
    const double cX = dstd[id.p] / (std[id.p] * double(cnt - 1));
    const double c0 = dmean[id.p] / double(cnt);
    double* db = dx + off;
    stream1<double, VEC, LPP, true>(x + off, g.nvec, id.lane, [&](const Vec<double, VEC>& v, int i) {
        Vec<double, VEC> o;
        const int e = i * VEC;
        const int r = BOXED ? e / g.Wd : 0, c = BOXED ? e - r * g.Wd : 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) o.v[j] = (!BOXED || g.cb.has(r, c + j)) ? fma(cX, v.v[j] - mu, c0) : 0.0;
        store_vec_nt<double, VEC>(db + (size_t)i * VEC, o);
    });
}

// ------------------------------------------------------------------------------------------------
// mid kernels: the sweeps of cnsn_mid_kernels.h, one workgroup of kBlock threads per channel (thread t: instances t, t + 256, ...:
// any N), around the same R = double algebra; sums in, coefficients out, gate parameters, running statistics and parameter
// gradients are double.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mid_fwd_f64_kernel(MidArgsD a, const double* __restrict__ mom,
                                                             const int64_t* __restrict__ perm,
                                                             const int64_t* __restrict__ chan_perm, GateDevD gg, GateDevD gf,
                                                             double* __restrict__ coef, double* __restrict__ saved) {
    __shared__ double red[(kBlock / 64) * 2];
    const int n0 = threadIdx.x;
    const bool lead = n0 == 0;
    const int c = blockIdx.x;
    const size_t P = (size_t)a.N * a.C;
    const int cs = (a.cn_active && chan_perm) ? (int)chan_perm[c] : c;

    // nn.BatchNorm1d.forward's num_batches_tracked.add_(1): ONE thread of the launch.  Here and not next to the running
    // statistics below: the two counters' addresses are then dead before the sweeps, and the kernel needs no stack frame
    if (a.sn_active && a.sn_training && lead && c == 0) {
        bump_batches_tracked(gg.nbt);
        if (a.sn_two) bump_batches_tracked(gf.nbt);
    }
    double wg0 = 0, wg1 = 0, wf0 = 0, wf1 = 0;
    if (a.sn_active) {
        wg0 = gg.w[2 * c];
        wg1 = gg.w[2 * c + 1];
        if (a.sn_two) {
            wf0 = gf.w[2 * c];
            wf1 = gf.w[2 * c + 1];
        }
    }

    // ---- sweep 1: CrossNorm algebra per plane, SelfNorm pre-activations z, sum z over the batch
    double sz[2] = {0.0, 0.0};
    for (int n = n0; n < a.N; n += kBlock) {
        const size_t p = (size_t)n * a.C + c;
        const SvRec ps = sv_rec(n, c, a.N);
        Moments o;
        o.mu_c = mom[p];
        o.M2c = mom[P + p];
        o.mu_o = a.boxed ? mom[2 * P + p] : 0.0;
        o.M2o = a.boxed ? mom[3 * P + p] : 0.0;
        o.mu_s = a.boxed ? mom[4 * P + p] : o.mu_c;
        o.M2s = a.boxed ? mom[5 * P + p] : o.M2c;
        double mu_sq = 0.0, M2_sq = 0.0;
        if (a.cn_active) {
            const size_t q = (size_t)perm[n] * a.C + cs;  // style source plane (cnsn.py:66-72)
            mu_sq = a.boxed ? mom[4 * P + q] : mom[q];
            M2_sq = a.boxed ? mom[5 * P + q] : mom[P + q];
        }
        const FwdPlane f = fwd_plane<double>(a, o, mu_sq, M2_sq);
        store_fwd_plane(saved, P, ps, f, a.cn_active);
        if (a.sn_active) {
            const double zg = wg0 * f.mu_p + wg1 * f.sig_p;  // Conv1d k=2 groups=C (cnsn.py:137)
            const double zf = wf0 * f.mu_p + wf1 * f.sig_p;
            saved[sv_at(ps, SV_ZH_G)] = zg;  // parked here until normalised in sweep 3
            saved[sv_at(ps, SV_ZH_F)] = zf;
            sz[0] += zg;
            sz[1] += zf;
        }
    }

    double mg = 0, mf = 0, rg = 1, rf = 1;
    if (a.sn_active) {
        if (a.sn_training) {
            // ---- BatchNorm1d batch statistics over N (biased variance for normalising, :138)
            block_sum_d<2>(sz, red);
            mg = sz[0] * a.inv_n;
            mf = sz[1] * a.inv_n;
            double sv[2] = {0.0, 0.0};
            for (int n = n0; n < a.N; n += kBlock) {
                const SvRec ps = sv_rec(n, c, a.N);
                const double dg = saved[sv_at(ps, SV_ZH_G)] - mg;
                const double df = saved[sv_at(ps, SV_ZH_F)] - mf;
                sv[0] += dg * dg;
                sv[1] += df * df;
            }
            block_sum_d<2>(sv, red);
            const double vg = sv[0] * a.inv_n, vf = sv[1] * a.inv_n;
            rg = 1.0 / sqrt(vg + a.eps_bn);
            rf = 1.0 / sqrt(vf + a.eps_bn);
            if (lead) {
                const double mom_ = a.momentum;
                gg.run_mean[c] = (1.0 - mom_) * gg.run_mean[c] + mom_ * mg;
                gg.run_var[c] = (1.0 - mom_) * gg.run_var[c] + mom_ * (vg * a.unbias_n);
                if (a.sn_two) {
                    gf.run_mean[c] = (1.0 - mom_) * gf.run_mean[c] + mom_ * mf;
                    gf.run_var[c] = (1.0 - mom_) * gf.run_var[c] + mom_ * (vf * a.unbias_n);
                }
            }
        } else {
            mg = gg.run_mean[c];
            rg = 1.0 / sqrt(gg.run_var[c] + a.eps_bn);
            if (a.sn_two) {
                mf = gf.run_mean[c];
                rf = 1.0 / sqrt(gf.run_var[c] + a.eps_bn);
            }
        }
        if (lead) {
            saved[SV_ROWS * P + c] = rg;
            saved[SV_ROWS * P + a.C + c] = rf;
        }
    }

    // ---- sweep 3: gates and the five forward coefficients of every plane of this channel
    const double gam_g = a.sn_active ? gg.gamma[c] : 0.0, bet_g = a.sn_active ? gg.beta[c] : 0.0;
    const double gam_f = a.sn_two ? gf.gamma[c] : 0.0, bet_f = a.sn_two ? gf.beta[c] : 0.0;
    for (int n = n0; n < a.N; n += kBlock) {
        const size_t p = (size_t)n * a.C + c;
        const SvRec ps = sv_rec(n, c, a.N);
        double g = 1.0, f = 1.0, zhg = 0.0, zhf = 0.0;
        if (a.sn_active) {
            zhg = (saved[sv_at(ps, SV_ZH_G)] - mg) * rg;
            g = sigmoid_d(gam_g * zhg + bet_g);
            if (a.sn_two) {
                zhf = (saved[sv_at(ps, SV_ZH_F)] - mf) * rf;
                f = sigmoid_d(gam_f * zhf + bet_f);
            }
        }
        saved[sv_at(ps, SV_G)] = g;
        saved[sv_at(ps, SV_ZH_G)] = zhg;
        saved[sv_at(ps, SV_F)] = f;
        saved[sv_at(ps, SV_ZH_F)] = zhf;
        FwdPlane fp;
        fp.mu_c = saved[sv_at(ps, SV_MU_C)];
        const CnRowsT<double> cr = load_cn_rows<double>(a, saved, ps, fp.mu_c);
        fp.a1 = cr.a1;
        fp.m_in = cr.m_in;
        fp.mu_p = saved[sv_at(ps, SV_MU_P)];
        const FwdCoefsT<double> k = fwd_coefs<double, double>(a, fp, g, f);
        coef[FC_A_IN * P + p] = k.a_in;
        coef[FC_XR * P + p] = k.xr;
        coef[FC_B_IN * P + p] = k.b_in;
        coef[FC_A_OUT * P + p] = k.a_out;
        coef[FC_B_OUT * P + p] = k.b_out;
    }
}

__device__ __forceinline__ void store_bwd_coefs_d(double* __restrict__ coef, size_t P, size_t p, const BwdCoefsT<double>& k,
                                                  int boxed) {
    coef[BC_CG_IN * P + p] = k.cG_in;
    coef[BC_CX_IN * P + p] = k.cX_in;
    coef[BC_XR_IN * P + p] = k.xr_in;
    coef[BC_C0_IN * P + p] = k.c0_in;
    if (boxed) {
        coef[BC_CG_OUT * P + p] = k.cG_out;
        coef[BC_CX_OUT * P + p] = k.cX_out;
        coef[BC_XR_OUT * P + p] = k.xr_out;
        coef[BC_C0_OUT * P + p] = k.c0_out;
        coef[BC_ES * P + p] = k.eS;
        coef[BC_XS * P + p] = k.xs;
        coef[BC_E0 * P + p] = k.e0;
    }
}

// per channel: gate / BatchNorm backward, parameter gradients, statistic gradients per plane; scatters the style-statistic
// gradients to the planes that lent their statistics.
__global__ __launch_bounds__(kBlock) void mid_bwd_a_f64_kernel(MidArgsD a, const double* __restrict__ sums,
                                                               const double* __restrict__ saved,
                                                               const int64_t* __restrict__ perm,
                                                               const int64_t* __restrict__ chan_perm, GateDevD gg, GateDevD gf,
                                                               GateGradDevD dg, GateGradDevD df, double* __restrict__ tmp,
                                                               double* __restrict__ coef) {
    __shared__ double red[(kBlock / 64) * 4];
    const int n0 = threadIdx.x;
    const bool lead = n0 == 0;
    const int c = blockIdx.x;
    const size_t P = (size_t)a.N * a.C;
    const int cs = (a.cn_active && chan_perm) ? (int)chan_perm[c] : c;

    auto sums_of = [&](size_t p) {  // pass A' shifted by the means themselves: nothing to undo (fix_sums)
        BwdSums s;
        s.S1in = sums[p];
        s.S2in = sums[P + p];
        s.S1out = a.boxed ? sums[2 * P + p] : 0.0;
        s.S2out = a.boxed ? sums[3 * P + p] : 0.0;
        return s;
    };

    // ---- sweep 1: dL/dgate -> through the sigmoid; batch sums for BatchNorm backward
    double s[4] = {0, 0, 0, 0};  // sum dt_g, sum dt_g*zh_g, sum dt_f, sum dt_f*zh_f
    if (a.sn_active) {
        for (int n = n0; n < a.N; n += kBlock) {
            const size_t p = (size_t)n * a.C + c;
            const SvRec ps = sv_rec(n, c, a.N);
            double dtg, dtf;
            const CnRowsT<double> cr = load_cn_rows<double>(a, saved, ps, saved[sv_at(ps, SV_MU_C)]);
            gate_dt<double>(a, sums_of(p), cr.a1, cr.m_in, cr.mu_o, saved[sv_at(ps, SV_MU_P)], saved[sv_at(ps, SV_G)],
                            saved[sv_at(ps, SV_F)], dtg, dtf);
            s[0] += dtg;
            s[1] += dtg * saved[sv_at(ps, SV_ZH_G)];
            s[2] += dtf;
            s[3] += dtf * saved[sv_at(ps, SV_ZH_F)];
            tmp[BT_DT_G * P + p] = dtg;
            tmp[BT_DT_F * P + p] = dtf;
        }
        block_sum_d<4>(s, red);
        if (lead) {
            dg.dgamma[c] = s[1];
            dg.dbeta[c] = s[0];
            if (a.sn_two) {
                df.dgamma[c] = s[3];
                df.dbeta[c] = s[2];
            }
        }
    }

    // ---- sweep 2: dz, dw, gradient of the plane statistics, CrossNorm statistic gradients
    BnBwd b{};
    b.s_dt_g = s[0];
    b.s_dtz_g = s[1];
    b.s_dt_f = s[2];
    b.s_dtz_f = s[3];
    if (a.sn_active) {
        b.wg0 = gg.w[2 * c];
        b.wg1 = gg.w[2 * c + 1];
        b.kg = gg.gamma[c] * saved[SV_ROWS * P + c];
        if (a.sn_two) {
            b.wf0 = gf.w[2 * c];
            b.wf1 = gf.w[2 * c + 1];
            b.kf = gf.gamma[c] * saved[SV_ROWS * P + a.C + c];
        }
    }
    double sw[4] = {0, 0, 0, 0};  // sum dz_g*mu_p, dz_g*sig_p, dz_f*mu_p, dz_f*sig_p
    for (int n = n0; n < a.N; n += kBlock) {
        const size_t p = (size_t)n * a.C + c;
        const SvRec ps = sv_rec(n, c, a.N);
        const double mu_p = saved[sv_at(ps, SV_MU_P)], sig_p = saved[sv_at(ps, SV_SIG_P)];
        const CnRowsT<double> cr = load_cn_rows<double>(a, saved, ps, saved[sv_at(ps, SV_MU_C)]);
        const BwdPlane o =
            bwd_plane<double>(a, b, sums_of(p), a.sn_active ? tmp[BT_DT_G * P + p] : 0.0, a.sn_active ? tmp[BT_DT_F * P + p] : 0.0,
                              saved[sv_at(ps, SV_ZH_G)], saved[sv_at(ps, SV_ZH_F)], saved[sv_at(ps, SV_G)], saved[sv_at(ps, SV_F)],
                              cr.aa, cr.a1, cr.m_in, mu_p, sig_p, cr.sig_c, cr.M2c);
        sw[0] += o.dz_g * mu_p;
        sw[1] += o.dz_g * sig_p;
        sw[2] += o.dz_f * mu_p;
        sw[3] += o.dz_f * sig_p;
        if (!a.cn_active) {  // no plane lends statistics to another one: the coefficients of dx are complete here
            const BwdCoefsT<double> k =
                bwd_coefs<double, double>(a, o, 0.0, 0.0, saved[sv_at(ps, SV_G)], cr.a1, cr.m_in, mu_p, saved[sv_at(ps, SV_MU_C)],
                                          cr.sig_c, cr.mu_s, cr.sig_s);
            store_bwd_coefs_d(coef, P, p, k, a.boxed);
        } else {
            tmp[BT_DMU_P * P + p] = o.dmu_p;
            tmp[BT_K * P + p] = o.k;
            tmp[BT_DMU_C * P + p] = o.Dmu_c;
            tmp[BT_DSIG_C * P + p] = o.Dsig_c;
            const size_t q = (size_t)perm[n] * a.C + cs;  // the plane whose statistics were borrowed
            tmp[BT_E_MU * P + q] = o.Emu;
            tmp[BT_E_SIG * P + q] = o.Esig;
        }
    }
    if (a.sn_active) {
        block_sum_d<4>(sw, red);
        if (lead) {
            dg.dw[2 * c] = sw[0];
            dg.dw[2 * c + 1] = sw[1];
            if (a.sn_two) {
                df.dw[2 * c] = sw[2];
                df.dw[2 * c + 1] = sw[3];
            }
        }
    }
}

// per plane: assemble the coefficients of dx (CrossNorm calls only: mid_bwd_a has written them otherwise)
__global__ __launch_bounds__(kBlock) void mid_bwd_b_f64_kernel(MidArgsD a, const double* __restrict__ saved,
                                                               const double* __restrict__ tmp, double* __restrict__ coef) {
    const size_t P = (size_t)a.N * a.C;
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const SvRec ps = sv_rec_of_plane(p, a.N, a.C);
    BwdPlane o{};
    o.dmu_p = tmp[BT_DMU_P * P + p];
    o.k = tmp[BT_K * P + p];
    o.Dmu_c = tmp[BT_DMU_C * P + p];
    o.Dsig_c = tmp[BT_DSIG_C * P + p];
    const double Emu = tmp[BT_E_MU * P + p], Esig = tmp[BT_E_SIG * P + p];
    const CnRowsT<double> cr = load_cn_rows<double>(a, saved, ps, saved[sv_at(ps, SV_MU_C)]);
    const BwdCoefsT<double> k = bwd_coefs<double, double>(a, o, Emu, Esig, saved[sv_at(ps, SV_G)], cr.a1, cr.m_in,
                                                          saved[sv_at(ps, SV_MU_P)], saved[sv_at(ps, SV_MU_C)], cr.sig_c, cr.mu_s,
                                                          cr.sig_s);
    store_bwd_coefs_d(coef, P, p, k, a.boxed);
}

}  // namespace cnsn
