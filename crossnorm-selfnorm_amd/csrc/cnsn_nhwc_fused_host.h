// Host helpers of the channels-last single-launch kernels, shared by their translation units (cnsn_nhwc_fused.hip: SelfNorm and the
// bottleneck tail; cnsn_nhwc_ibn.hip: Instance-Batch normalisation; cnsn_nhwc_bn.hip: BatchNorm2d + ReLU): dtype dispatch, the launch arguments every family starts from,
// and the co-resident launch with its barrier booking.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "cnsn_env.h"
#include "cnsn_nhwc.h"
#include "cnsn_nhwc_fused_kernels.h"
#include "cnsn_resident_host.h"

namespace cnsn {

// tiles of a channels-last single launch (cnsn_nhwc_fused.hip): column blocks, pixel chunks, two per workgroup of the grid
NhwcGeom nhwc_fused_geom(const Plan& pl);

namespace nhwc_host {

inline int vec_of(int dtype) { return 16 / elem_bytes(dtype); }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// 0 never, 1 the AUTO rule (default), 2 wherever the kernels apply, n > 2: AUTO for tensors of at most n MiB (CNSN_NHWC_FUSED)
inline int fused_mode() {
    const char* e = knob(K_NHWC_FUSED);
    if (!e) return 1;
    const int v = atoi(e);
    return v < 0 ? 0 : v;
}

template <typename F>
bool dispatch_t(int dtype, F&& f) {
    if (dtype == CNSN_F32) {
        f(TypeTag<float>{}, IntTag<4>{});
        return true;
    }
    if (dtype == CNSN_BF16) {
        f(TypeTag<bf16_t>{}, IntTag<8>{});
        return true;
    }
    if (dtype == CNSN_F16) {
        f(TypeTag<_Float16>{}, IntTag<8>{});
        return true;
    }
    return false;
}

template <typename F>
void with_add(int add, F&& f) {
    if (add == ADD_PRE)
        f(IntTag<ADD_PRE>{});
    else if (add == ADD_POST)
        f(IntTag<ADD_POST>{});
    else
        f(IntTag<ADD_NONE>{});
}

inline NhwcFusedArgs make_args(const Plan& pl, const NhwcGeom& ng, int relu, int gc) {
    const cnsn_problem_t& p = pl.pr;
    NhwcFusedArgs a{};
    a.g = ng;
    a.ntiles = ng.N * ng.S * ng.ncb;
    a.ngroups = p.C / gc;
    a.training = p.sn_training ? 1 : 0;
    a.relu = relu;
    a.keep = 0;
    a.eps_sn = p.eps_sn;
    a.eps_bn = p.eps_bn;
    a.momentum = p.momentum;
    a.inv_n = pl.mid.inv_n;
    a.unbias_n = pl.mid.unbias_n;
    a.bar.host_flag = resident_host_flag();
    a.bar.wait_ticks = resident_wait_ticks();
    const char* fi = knob(K_FAULT_INJECT);
    a.bar.fault = (fi && fi[0] == '1') ? 1 : 0;
    a.bar.ctl_idle = 0u;
    return a;
}

// issue `kern` with a co-resident grid (a multiple of 8: the barrier's groups are equal) of at most `ntiles` workgroups; the two
// barriers are booked on the context before the launch.  `a`: the kernel's first argument, `bar` the GridBar inside it
template <typename A, typename Kern, typename... Args>
int launch_coresident(const cnsn_problem_t& pr, Kern kern, size_t lds, A& a, GridBar& bar, int ntiles, void* ws_bar,
                      hipStream_t stream, Args... args) {
    const int grid = reshost::grid_for(kern, lds, 8, ntiles & ~7);
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
    return launch_coresident(pl.pr, kern, lds, a, fa.bar, fa.ntiles, ws_bar, stream, args...);
}

// the barrier's host-side fields (bounded wait, give-up protocol, the tests' fault switch)
inline void init_grid_bar(GridBar& bar) {
    bar.host_flag = resident_host_flag();
    bar.wait_ticks = resident_wait_ticks();
    const char* fi = knob(K_FAULT_INJECT);
    bar.fault = (fi && fi[0] == '1') ? 1 : 0;
    bar.ctl_idle = 0u;
}

}  // namespace nhwc_host
}  // namespace cnsn
