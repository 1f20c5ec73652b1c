// The fused RMSNorm of the decode projections, shared by gemv.hip (fp16 weights) and gemv_w8.hip (e4m3 weights): both normalise the
// activation vector with the SAME arithmetic in the SAME order, so the two weight formats see the same fp16 vector.
#pragma once
#include "sc_common.h"

// Qwen2 RMSNorm of the activation vector, ONCE per workgroup, into LDS (fp16, HF's rounding: gamma * fp16(x * rstd)): the 256 threads
// share the sum of squares (fixed reduction order: 8-element chunks t, t + 256, ... per thread, xor-shuffle tree per wave, the four
// wave sums added in order) and each writes its chunks of the normalised vector.  Before (round 2) every WAVE recomputed the norm and
// re-normalised x in every K-step of its weight stream - ~40 VALU instructions per 16-byte weight load in an in-order loop, and the
// weight loads could not start before the wave's own reduction was done (k_decode_qkv: 2.6 TB/s, gate/up: 51 us against 44 without
// the fused norm).  Shared by k_gemv<NORM> and k_decode_qkv so that the eager decode step and the captured graph stay bit-identical.
__device__ __forceinline__ void block_rmsnorm_to_lds(const _Float16* __restrict__ x, const _Float16* __restrict__ gamma, int K, float eps, _Float16* xn,
                                                     float* red) {
    // The reduction order is that of 256 VIRTUAL threads whatever the workgroup size (2, 3 or 4 waves: the launchers pick the wave count
    // that deals the rows evenly over the CUs): virtual thread v sums the 8-element chunks v, v + 256, ...; a virtual wave is reduced
    // with the xor-shuffle tree; the four virtual-wave sums are added in order.
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;
    for (int vw = wave; vw < 4; vw += nw) {
        float ss = 0.f;
        for (int k = (vw * 64 + lane) * 8; k < K; k += 2048) {
            const sc_h8 xv = *reinterpret_cast<const sc_h8*>(x + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += (float)xv[e] * (float)xv[e];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
        if (lane == 0) red[vw] = ss;
    }
    __syncthreads();
    const float rstd = rsqrtf((((red[0] + red[1]) + red[2]) + red[3]) / (float)K + eps);
    for (int k = t * 8; k < K; k += (int)blockDim.x * 8) {
        const sc_h8 xv = *reinterpret_cast<const sc_h8*>(x + k), gv = *reinterpret_cast<const sc_h8*>(gamma + k);
        sc_h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (_Float16)((float)gv[e] * (float)(_Float16)((float)xv[e] * rstd));
        *reinterpret_cast<sc_h8*>(xn + k) = o;
    }
    __syncthreads();
}
