// The float64 entry points of include/cnsn_hip.h (cnsn_*_f64): the two-pass streaming kernels of cnsn_stream_kernels.h and the
// mid kernels of cnsn_mid_kernels.h instantiated for T = double, behind the host plan every other entry point uses.  No
// persistent grid, no barrier, no context: three or four launches per direction.
#include "../../include/cnsn_hip.h"
#include "cnsn_env.h"

#include <hip/hip_runtime.h>

#include "cnsn_host_plan.h"
#include "cnsn_mid_kernels.h"
#include "cnsn_stream_kernels.h"

using namespace cnsn;

namespace {

using PlanD = PlanT<double>;

// call f(IntTag<VEC>, IntTag<LPP>, IntTag<BOXED>): 16-byte loads, two doubles where the plane (with crop boxes: the row) is even
template <typename F>
void dispatch_f64(Shape s, bool boxed, F&& f) {
    dispatch_vl<double>(s.vec, s.lpp, [&](auto, auto vt, auto lt) {
        if (boxed)
            f(vt, lt, IntTag<1>{});
        else
            f(vt, lt, IntTag<0>{});
    });
}

// `sc` may be NULL for the size query alone
int make_plan_f64(const cnsn_problem_t* prob, const cnsn_f64_scalars_t* sc, PlanD& pl) {
    if (!prob) return CNSN_E_NULL;
    if (prob->struct_bytes != (int32_t)sizeof(cnsn_problem_t)) return CNSN_E_STRUCT;
    if (sc && sc->struct_bytes != (int32_t)sizeof(cnsn_f64_scalars_t)) return CNSN_E_STRUCT;
    if (prob->dtype == CNSN_F64 && prob->layout != CNSN_LAYOUT_NCHW) return CNSN_E_UNSUPPORTED;
    return make_plan(prob, sc, pl);
}

// the gates a call needs are there and carry this library's struct sizes
int check_gates_f64(const cnsn_problem_t& p, const cnsn_gate_f64_t* g, const cnsn_gate_f64_t* f) {
    if (!p.sn_active) return CNSN_OK;
    if (!gate_ok(g) || (p.sn_two && !gate_ok(f))) return CNSN_E_NULL;
    if (g->struct_bytes != (int32_t)sizeof(cnsn_gate_f64_t)) return CNSN_E_STRUCT;
    if (p.sn_two && f->struct_bytes != (int32_t)sizeof(cnsn_gate_f64_t)) return CNSN_E_STRUCT;
    return CNSN_OK;
}
int check_gate_grads_f64(const cnsn_problem_t& p, const cnsn_gate_grad_f64_t* dg, const cnsn_gate_grad_f64_t* df) {
    if (!p.sn_active) return CNSN_OK;
    if (!gate_grad_ok(dg) || (p.sn_two && !gate_grad_ok(df))) return CNSN_E_NULL;
    if (dg->struct_bytes != (int32_t)sizeof(cnsn_gate_grad_f64_t)) return CNSN_E_STRUCT;
    if (p.sn_two && df->struct_bytes != (int32_t)sizeof(cnsn_gate_grad_f64_t)) return CNSN_E_STRUCT;
    return CNSN_OK;
}

int check_tensor_f64(const void* p, int N, int C, int H, int W) { return check_tensor(p, CNSN_F64, N, C, H, W, true); }

}  // namespace

extern "C" {

size_t cnsn_workspace_bytes_f64(const cnsn_problem_t* prob) {
    PlanD pl;
    if (make_plan_f64(prob, nullptr, pl) != CNSN_OK) return 0;
    return workspace_bytes_of(pl);
}

int cnsn_forward_f64(const cnsn_problem_t* prob, const cnsn_f64_scalars_t* sc, const double* x, const int64_t* perm,
                     const int64_t* chan_perm, const cnsn_gate_f64_t* g, const cnsn_gate_f64_t* f, double* y, float* saved,
                     void* workspace, size_t workspace_bytes, void* stream_) {
    if (!sc) return CNSN_E_NULL;
    PlanD pl;
    int st = make_plan_f64(prob, sc, pl);
    if (st) return st;
    const cnsn_problem_t& p = pl.pr;
    if (!x || !y || !workspace) return CNSN_E_NULL;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)workspace) & 15u) != 0) return CNSN_E_ALIGN;
    if (p.cn_active && !perm) return CNSN_E_NULL;
    st = check_gates_f64(p, g, f);
    if (st) return st;
    if (workspace_bytes < workspace_bytes_of(pl)) return CNSN_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;

    const size_t P = pl.P;
    double* mom = (double*)workspace;
    double* saved_d = saved ? (double*)saved : mom + 6 * P;
    double* coef = mom + 6 * P + saved_doubles_of(pl);
    const int blocks = blocks_for(pl.geom.P, pl.shape.lpp);
    dispatch_f64(pl.shape, pl.boxed, [&](auto vt, auto lt, auto bt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value, BOXED = decltype(bt)::value;
        plane_stats_kernel<double, VEC, LPP, BOXED != 0><<<blocks, kBlock, 0, stream>>>(x, pl.geom, mom, nullptr, 0.0);
    });
    // one workgroup per channel (a tiled double mid kernel is not built)
    mid_fwd_kernel<double, 1, kBlock><<<p.C, kBlock, 0, stream>>>(pl.mid, mom, perm, chan_perm, gate_dev(g), gate_dev(f), coef, saved_d);
    const ApplyCoefT<double> cf{coef + FC_A_IN * P, coef + FC_XR * P, coef + FC_B_IN * P, coef + FC_A_OUT * P, coef + FC_B_OUT * P};
    dispatch_f64(pl.shape, pl.boxed, [&](auto vt, auto lt, auto bt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value, BOXED = decltype(bt)::value;
        apply_fwd_kernel<double, VEC, LPP, BOXED != 0><<<blocks, kBlock, 0, stream>>>(x, y, pl.geom, cf);
    });
    return launch_status();
}

int cnsn_backward_f64(const cnsn_problem_t* prob, const cnsn_f64_scalars_t* sc, const double* grad_y, const double* x,
                      const int64_t* perm, const int64_t* chan_perm, const cnsn_gate_f64_t* g, const cnsn_gate_f64_t* f,
                      const float* saved, double* grad_x, const cnsn_gate_grad_f64_t* dg, const cnsn_gate_grad_f64_t* df,
                      void* workspace, size_t workspace_bytes, void* stream_) {
    if (!sc) return CNSN_E_NULL;
    PlanD pl;
    int st = make_plan_f64(prob, sc, pl);
    if (st) return st;
    const cnsn_problem_t& p = pl.pr;
    if (!grad_y || !x || !grad_x || !saved || !workspace) return CNSN_E_NULL;
    if ((((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)grad_x | (uintptr_t)workspace) & 15u) != 0) return CNSN_E_ALIGN;
    if (p.cn_active && !perm) return CNSN_E_NULL;
    st = check_gates_f64(p, g, f);
    if (st) return st;
    st = check_gate_grads_f64(p, dg, df);
    if (st) return st;
    if (workspace_bytes < workspace_bytes_of(pl)) return CNSN_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;

    const size_t P = pl.P;
    double* tmp = (double*)workspace;
    double* sums = tmp + BT_ROWS * P;
    double* coef = sums + 4 * P;
    const double* saved_d = (const double*)saved;
    const double* mu_c = saved_d + (size_t)SV_MU_C * p.N;  // rows of `saved` (shift_stride 0)
    const double* mu_o = pl.boxed ? saved_d + (size_t)SV_MU_O * p.N : nullptr;
    const int blocks = blocks_for(pl.geom.P, pl.shape.lpp);
    dispatch_f64(pl.shape, pl.boxed, [&](auto vt, auto lt, auto bt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value, BOXED = decltype(bt)::value;
        bwd_reduce_kernel<double, VEC, LPP, BOXED != 0><<<blocks, kBlock, 0, stream>>>(grad_y, x, pl.geom, mu_c, mu_o, 0, sums);
    });
    mid_bwd_a_kernel<double, 1, kBlock><<<p.C, kBlock, 0, stream>>>(pl.mid, sums, saved_d, perm, chan_perm, gate_dev(g), gate_dev(f),
                                                                    gate_grad_dev(dg), gate_grad_dev(df), tmp, coef);
    if (pl.mid.cn_active)  // (without CrossNorm mid_bwd_a has written the coefficients itself)
        mid_bwd_b_kernel<double><<<(int)((P + kBlock - 1) / kBlock), kBlock, 0, stream>>>(pl.mid, saved_d, tmp, coef);
    dispatch_f64(pl.shape, pl.boxed, [&](auto vt, auto lt, auto bt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value, BOXED = decltype(bt)::value;
        apply_bwd_kernel<double, VEC, LPP, BOXED != 0><<<blocks, kBlock, 0, stream>>>(grad_y, x, grad_x, pl.geom, coef);
    });
    return launch_status();
}

int cnsn_plane_stats_f64(const double* x, int N, int C, int H, int W, const int32_t* box, double eps, double* mean_std,
                         void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    if (!mean_std) return CNSN_E_NULL;
    PlaneCall pc;
    st = plane_call(CNSN_F64, N, C, H, W, box, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    dispatch_f64(pc.s, pc.boxed, [&](auto vt, auto lt, auto bt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value, BOXED = decltype(bt)::value;
        plane_stats_kernel<double, VEC, LPP, BOXED != 0><<<pc.blocks, kBlock, 0, stream>>>(x, pc.g, nullptr, mean_std, eps);
    });
    return launch_status();
}

int cnsn_plane_stats_backward_f64(const double* x, int N, int C, int H, int W, const int32_t* box, const double* mean,
                                  const double* std, const double* dmean, const double* dstd, double* dx, void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    if (!mean || !std || !dmean || !dstd || !dx) return CNSN_E_NULL;
    if (((uintptr_t)dx & 15u) != 0) return CNSN_E_ALIGN;
    PlaneCall pc;
    st = plane_call(CNSN_F64, N, C, H, W, box, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    dispatch_f64(pc.s, pc.boxed, [&](auto vt, auto lt, auto bt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value, BOXED = decltype(bt)::value;
        plane_stats_bwd_kernel<double, VEC, LPP, BOXED != 0><<<pc.blocks, kBlock, 0, stream>>>(x, dx, pc.g, mean, std, dmean, dstd);
    });
    return launch_status();
}

int cnsn_plane_affine_f64(const double* x, int N, int C, int H, int W, const double* scale, const double* shift, double* y,
                          void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    if (!scale || !shift || !y) return CNSN_E_NULL;
    if (((uintptr_t)y & 15u) != 0) return CNSN_E_ALIGN;
    PlaneCall pc;
    st = plane_call(CNSN_F64, N, C, H, W, nullptr, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    const ApplyCoefT<double> cf{scale, nullptr, shift, nullptr, nullptr};
    dispatch_f64(pc.s, false, [&](auto vt, auto lt, auto) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        apply_fwd_kernel<double, VEC, LPP, false><<<pc.blocks, kBlock, 0, stream>>>(x, y, pc.g, cf);
    });
    return launch_status();
}

int cnsn_plane_dot_f64(const double* gr, const double* x, int N, int C, int H, int W, double* sums, void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    st = check_tensor_f64(gr, N, C, H, W);
    if (st) return st;
    if (!sums) return CNSN_E_NULL;
    PlaneCall pc;
    st = plane_call(CNSN_F64, N, C, H, W, nullptr, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    dispatch_f64(pc.s, false, [&](auto vt, auto lt, auto) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        bwd_reduce_kernel<double, VEC, LPP, false><<<pc.blocks, kBlock, 0, stream>>>(gr, x, pc.g, nullptr, nullptr, 1, sums);
    });
    return launch_status();
}

}  // extern "C"
