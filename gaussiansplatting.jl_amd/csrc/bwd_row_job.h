// The row-independent job of the compositing backward, device-only: what the per-Gaussian backward needs that depends on
// nothing composite_bwd produces, done by extra single-wave workgroups of composite_bwd's own launch (composite.hip:
// composite_bwd_kernel_rgb_bg0) — that kernel is bound by VALU issue and leaves the memory pipe idle, the per-Gaussian backward
// is bound by its bytes.  Per Gaussian of the workgroup's slice:
//   visible : the nine floats of d rgb / d dir before the clamp (splat_math.h: view_dir and sh_dir_jacobian, the definitions
//             pergauss_bwd evaluates otherwise) into job.jac — 36 bytes it reads back instead of up to 180 of SH bands;
//   culled  : the zeros of every gradient array, the values pergauss_bwd writes otherwise.
// No LDS, no atomics, no flags: nothing in the launch depends on it and it depends on nothing the launch writes.
//
// composite.hip is compiled with FMA contraction; this text is included under `#pragma clang fp contract(off)` there, so that
// the floats are the ones pergauss.hip (-ffp-contract=off) computes.
#pragma once
#include "splat_math.h"

namespace gsr {

template <int DEG>
__device__ __forceinline__ void bwd_row_job_slice(const GsrRowJob& job, uint32_t w, int lane) {
    using namespace gsr::splat;
    const int K3 = 3 * job.K;
    const int64_t begin = (int64_t)w * job.slice;
    const int end = (int)(begin + job.slice < (int64_t)job.n ? begin + job.slice : (int64_t)job.n);
    for (int base = (int)begin; base < end; base += 64) {  // (begin < n: n_wg = ceil(n / slice))
        const int i = base + lane;
        const bool mine = i < end;
        const bool visible = mine && job.radii[i] > 0;
        if (DEG > 0 && visible) {
            const float p[3] = {job.means[3 * (size_t)i], job.means[3 * (size_t)i + 1], job.means[3 * (size_t)i + 2]};
            float d0[3], dir[3], dcx[3], dcy[3], dcz[3];
            view_dir(p, job.center, d0, dir);
            sh_dir_jacobian<DEG>(job.shs + (size_t)K3 * i + 3, dir, dcx, dcy, dcz);
            float* j9 = job.jac + 9 * (size_t)i;
#pragma unroll
            for (int c = 0; c < 3; c++) { j9[c] = dcx[c]; j9[3 + c] = dcy[c]; j9[6 + c] = dcz[c]; }
        }
        if (mine && !visible) {
#pragma unroll
            for (int c = 0; c < 3; c++) { job.vmeans[3 * (size_t)i + c] = 0.0f; job.vscales[3 * (size_t)i + c] = 0.0f; }
            job.vrots[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            job.vopac[i] = 0.0f;
        }
        // the ∇shs row of a culled Gaussian (K3 <= 48 floats), one store of the whole wave per row
        unsigned long long culled = __builtin_amdgcn_ballot_w64(mine && !visible);
        while (culled) {
            const int src = __builtin_ctzll(culled);
            culled &= culled - 1ull;
            if (lane < K3) job.vshs[(size_t)K3 * (base + src) + lane] = 0.0f;
        }
    }
}

__device__ __forceinline__ void bwd_row_job_run(const GsrRowJob& job, uint32_t w, int lane) {
    switch (job.degree) {
        case 0: bwd_row_job_slice<0>(job, w, lane); break;
        case 1: bwd_row_job_slice<1>(job, w, lane); break;
        case 2: bwd_row_job_slice<2>(job, w, lane); break;
        default: bwd_row_job_slice<3>(job, w, lane); break;
    }
}

}  // namespace gsr
