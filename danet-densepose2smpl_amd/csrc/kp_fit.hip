// Keypoint fit for gfx950 (DESIGN.md "fit rule"): SMPLify-style refinement of (cam, betas, 24 rotations in 6D) against 2D
// keypoints.  ONE launch per fit, ONE workgroup of 256 threads per person, every iteration inside the kernel: the unknowns, the
// Adam moments and every intermediate of an iteration live in LDS and registers; global memory sees the read-only tables, the
// inputs, the outputs and v_posed of the support (a caller-owned workspace, written in the forward sweep and read back in the
// reverse sweep by the same workgroup).  No atomics, every reduction in a fixed order: a person's result does not depend on the
// other people of the batch, and two runs give the same bits.
//
// The kernel is fit_kernel<false, danet_kp_fit_args> of fit_kernel.h, which describes an iteration; the dense fit (dense_fit.hip)
// launches the same text with its landmark term switched on.  This unit holds the keypoint fit's entry points.
#include "fit_kernel.h"

extern "C" size_t danet_kp_fit_ws_floats(int P, int Sp) {
    return P > 0 && Sp > 0 ? (size_t)P * (size_t)Sp * 3 : 0;
}

extern "C" int danet_kp_fit(const danet_kp_fit_args* a, size_t ws_floats, void* stream)
{
    DANET_ENTER();
    if (const int e = danet_fit::fit_check_args("kp_fit", a)) return e;
    if (ws_floats < danet_kp_fit_ws_floats(a->P, a->Sp))
        return danet::fail(DANET_ERR_WORKSPACE, "kp_fit: workspace %zu < %zu floats", ws_floats, danet_kp_fit_ws_floats(a->P, a->Sp));
    hipLaunchKernelGGL((danet_fit::fit_kernel<false, danet_kp_fit_args>), dim3(a->P), dim3(danet_fit::NT), 0, (hipStream_t)stream, *a);
    DANET_CHECK_LAUNCH("fit_kernel<false, danet_kp_fit_args> (kp_fit)");
    return DANET_OK;
}
