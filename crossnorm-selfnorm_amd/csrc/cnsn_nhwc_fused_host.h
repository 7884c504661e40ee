// Host helpers of the channels-last single-launch kernels, shared by their translation units (cnsn_nhwc_fused.hip: SelfNorm and the
// bottleneck tail; cnsn_nhwc_ibn.hip: Instance-Batch normalisation; cnsn_nhwc_bn.hip: BatchNorm2d + ReLU): the switches a forward
// asks, the descriptors' common checks, a caller's BatchNorm2d as the kernels take it, the launch arguments every family starts
// from, and the co-resident launch with its barrier booking.  (Dtype dispatch, the workspace carver and the keep rule: cnsn_nhwc.h.)
#pragma once
#include <cstdio>
#include <cstdlib>

#include "cnsn_env.h"
#include "cnsn_nhwc.h"
#include "cnsn_nhwc_bnhead_kernels.h"
#include "cnsn_nhwc_fused_kernels.h"
#include "cnsn_resident_host.h"

namespace cnsn {

// tiles of a channels-last single launch (cnsn_nhwc_fused.hip): column blocks, pixel chunks, two per workgroup of the grid
NhwcGeom nhwc_fused_geom(const Plan& pl);

namespace nhwc_host {

// 0 never, 1 the AUTO rule (default), 2 wherever the kernels apply, n > 2: AUTO for tensors of at most n MiB (CNSN_NHWC_FUSED)
inline int fused_mode() {
    const char* e = knob(K_NHWC_FUSED);
    if (!e) return 1;
    const int v = atoi(e);
    return v < 0 ? 0 : v;
}

inline size_t tensor_bytes(const Plan& pl) { return pl.P * (size_t)(pl.pr.H * pl.pr.W) * elem_bytes(pl.pr.dtype); }

// what the forward of the IBN and BatchNorm2d + ReLU single launches asks of the switches: CNSN_NHWC_FUSED not 0, the co-resident
// kernels allowed (resident_auto_enabled: switched on and not degraded) and, with CNSN_NHWC_FUSED above 2, the tensor within that many MiB
inline bool single_launch_allowed(size_t tensor_bytes) {
    const int mode = fused_mode();
    if (mode == 0 || !resident_auto_enabled()) return false;
    return !(mode > 2 && tensor_bytes > ((size_t)mode << 20));
}

// the head of a descriptor's checks (cnsn_ibn_t, cnsn_bn_act_t), in the order the status codes are documented in
template <typename D>
int parse_desc_head(const D* d) {
    if (!d) return CNSN_E_NULL;
    if (d->struct_bytes != (int32_t)sizeof(D)) return CNSN_E_STRUCT;
    if (d->dtype != CNSN_F32 && d->dtype != CNSN_BF16 && d->dtype != CNSN_F16) return CNSN_E_DTYPE;
    if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0) return CNSN_E_SHAPE;
    return CNSN_OK;
}
inline int parse_bn_tail(const cnsn_bn_tail_t& bn) { return bn.struct_bytes == (int32_t)sizeof(cnsn_bn_tail_t) ? CNSN_OK : CNSN_E_STRUCT; }

// a caller's BatchNorm2d as the kernels take it; `counts` false: the eval launch, which passes no counter
inline BnHeadDev bn_head_dev(const cnsn_bn_tail_t& bn, bool counts = true) {
    return BnHeadDev{bn.weight, bn.bias, bn.running_mean, bn.running_var, counts ? (long long*)bn.num_batches_tracked : nullptr, bn.eps,
                     bn.momentum};
}
// 1 / R and R / (R - 1) of a BatchNorm2d over R values per channel (NhwcBnArgs, NhwcIbnArgs, BnActArgs)
template <typename A>
void set_bn_count(A& a, double R) {
    a.inv_r = 1.0 / R;
    a.unbias_r = R > 1.0 ? R / (R - 1.0) : 1.0;
}

// the barrier's host-side fields (bounded wait, give-up protocol, the tests' fault switch)
inline void init_grid_bar(GridBar& bar) {
    bar.host_flag = resident_host_flag();
    bar.wait_ticks = resident_wait_ticks();
    const char* fi = knob(K_FAULT_INJECT);
    bar.fault = (fi && fi[0] == '1') ? 1 : 0;
    bar.ctl_idle = 0u;
}

inline NhwcFusedArgs make_args(const Plan& pl, const NhwcGeom& ng, int relu, int gc) {
    const cnsn_problem_t& p = pl.pr;
    NhwcFusedArgs a{};
    a.g = ng;
    a.ntiles = ng.N * ng.S * ng.ncb;
    a.ngroups = p.C / gc;
    a.training = p.sn_training ? 1 : 0;
    a.relu = relu;
    a.eps_sn = p.eps_sn;
    a.eps_bn = p.eps_bn;
    a.momentum = p.momentum;
    a.inv_n = pl.mid.inv_n;
    a.unbias_n = pl.mid.unbias_n;
    init_grid_bar(a.bar);
    return a;
}

// issue `kern` with a co-resident grid (a multiple of 8: the barrier's groups are equal) of at most `ntiles` workgroups; the two
// barriers are booked on the context before the launch.  `a`: the kernel's first argument, `bar` the GridBar inside it;
// `grid_out` (may be null): the grid that was chosen, for the caller's debug line
template <typename A, typename Kern, typename... Args>
int launch_coresident(const cnsn_problem_t& pr, Kern kern, size_t lds, A& a, GridBar& bar, int ntiles, void* ws_bar,
                      hipStream_t stream, int* grid_out, Args... args) {
    const int grid = reshost::grid_for(kern, lds, 8, ntiles & ~7);
    if (grid_out) *grid_out = grid;
    if (grid < 8) return CNSN_E_UNSUPPORTED;
    ResidentChain chain(stream);  // persistent grids of different streams never overlap
    const BarArea ba = resident_bar_area(pr, ws_bar, stream, grid, 2);
    if (ba.need_fill) {
        const hipError_t e = hipMemsetAsync(ws_bar, 0, kBarBlock, stream);
        if (e != hipSuccess) return (int)e;
    }
    bar.ctl = ba.ctl;
    bar.block = ba.block;
    bar.group_base = ba.group_base;
    bar.bar_base = ba.bar_base;
    kern<<<grid, kBlock, lds, stream>>>(a, args...);
    return launch_status();
}

// ... for the kernels whose first argument is, or holds, a NhwcFusedArgs (`fa`)
template <typename A, typename Kern, typename... Args>
int launch_fused(const Plan& pl, Kern kern, size_t lds, A& a, NhwcFusedArgs& fa, void* ws_bar, hipStream_t stream, Args... args) {
    return launch_coresident(pl.pr, kern, lds, a, fa.bar, fa.ntiles, ws_bar, stream, (int*)nullptr, args...);
}

}  // namespace nhwc_host
}  // namespace cnsn
