// What the classification heads share (head.hip: the BatchNorm head of TRI_MBT_VSLTCLS, 512 or 256 columns wide; head3.hip: the
// three-row LayerNorm head; headr.hip: the row head):
// the `ie_demo` chain and layer_norms_after_concat on 256-wide rows, the dW1 and dx loops, the `ie_demo` backward,
// and the slab reduction that writes the row-summed gradients to their destinations.
// Blocks, not kernels: the BatchNorm head reduces over the samples inside a wave, the LayerNorm head over the features, so each
// file keeps its own kernels and composes them from the force-inlined pieces below.  A block's arithmetic (fmaf / mul / add choices,
// reduction order, order of the block_sum calls) is part of its contract: both heads' results depend on it bit for bit.
#pragma once
#include "common.hip.h"

namespace {

constexpr int D = 256, DX = 512, MAXB = 256, FPW = 4;  // d_model, head input width, most rows (samples) per call, features per workgroup
inline int rows_per_lane(int B) { return B <= 64 ? 1 : (B <= 128 ? 2 : 4); }

MTMP_DEV float block_sum(float v, float* red, int tid) {   // 256 threads -> every thread gets the sum
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

struct Shared3 {      // ie_demo.{0.weight[256][2],0.bias,1.weight,1.bias}, layer_norms_after_concat.{weight,bias}
    const float* demo_w; const float* demo_b; const float* demo_g; const float* demo_be; const float* ln_g; const float* ln_b;
};
inline Shared3 shared_of(const void* const* q) {      // the first six entries of either head's parameter table
    return Shared3{(const float*)q[0], (const float*)q[1], (const float*)q[2], (const float*)q[3], (const float*)q[4], (const float*)q[5]};
}

// ---- forward, one wave per 256-wide row: lane owns columns c = 4 lane .. c + 3 ----
// LayerNorm statistics of the row v (`sum` = the lane's v[0] + .. + v[3], added in the caller's order): d = v - mean, returns rstd
MTMP_DEV float wave_ln4(const f32x4& v, float sum, float eps, float (&d)[4]) {
    const float mean = wave_sum(sum) * (1.0f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { d[i] = v[i] - mean; sq += d[i] * d[i]; }
    return rsqrtf(wave_sum(sq) * (1.0f / D) + eps);
}

// LN(cls row) of layer_norms_after_concat
template <typename TC> MTMP_DEV f32x4 cls_row_fwd(const TC* row, const Shared3& p, int c, float eps) {
    const f32x4 v = load4<TC>(row + c);
    float d[4];
    const float rstd = wave_ln4(v, v[0] + v[1] + v[2] + v[3], eps, d);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = fmaf(d[i] * rstd, p.ln_g[c + i], p.ln_b[c + i]);
    return o;
}

// ie_demo: ReLU(LN(age * w[:,0] + gender * w[:,1] + b))
MTMP_DEV f32x4 demo_row_fwd(float a, float g, const Shared3& p, int c, float eps) {
    f32x4 u;
    float d[4], su = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { u[i] = fmaf(a, p.demo_w[2 * (c + i)], fmaf(g, p.demo_w[2 * (c + i) + 1], p.demo_b[c + i])); su += u[i]; }
    const float rstd = wave_ln4(u, su, eps, d);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = fmaxf(fmaf(d[i] * rstd, p.demo_g[c + i], p.demo_be[c + i]), 0.f);
    return o;
}

// ---- feature-parallel kernels: a workgroup owns FPW features, a wave one of them x all rows, R = 1, 2 or 4 rows per lane ----
// (The 512 -> 256 product on the transposed 64-column tile is NOT a block here: it stands, loop for loop, in head_fc_kernel,
//  head3_fc_kernel and headr_fc_kernel.  As an inlined function -- whole, or split into the tile load and the fma loop -- the compiler unrolls its loops
//  in another way (head_fc_kernel<2>: 1809 -> 454 instructions, 44 -> 54 VGPRs), the bits stay, and the replayed three-row head at
//  B = 256 measured 1 us slower than the parent, outside the parent's own spread (profiles/head_shared.txt).  A change to one copy
//  goes into the others.)

// dW1[j][k] = sum_b dh[b][j] x[b][k] for the workgroup's four features (dhs[f][b], zero past B): thread t owns columns t (s0) and
// t + 256 (s1) of those four rows of W1.  (Rows of 512: the 256-wide head.hip keeps the one-half loop in its kernel.)
template <int NB>
MTMP_DEV void dw1_rows(const float (&dhs)[FPW][NB], const float* x, int B, float (&s0)[FPW], float (&s1)[FPW]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int f = 0; f < FPW; ++f) s0[f] = s1[f] = 0.f;
    for (int r = 0; r < B; ++r) {
        const float x0 = x[(size_t)r * DX + tid], x1 = x[(size_t)r * DX + D + tid];
#pragma unroll
        for (int f = 0; f < FPW; ++f) { s0[f] = fmaf(dhs[f][r], x0, s0[f]); s1[f] = fmaf(dhs[f][r], x1, s1[f]); }
    }
}

// ---- backward, one workgroup per row of x: thread = column k of each half ----
// dx = dh W1 at columns k (the LN(cls) half) and 256 + k (the ie_demo half); dhr = the row of dh in LDS
MTMP_DEV void dx_row(const float* dhr, const float* w1, int k, float& dxc, float& dxd) {
    dxc = 0.f; dxd = 0.f;
    for (int j = 0; j < D; ++j) {
        const float g = dhr[j];
        dxc = fmaf(g, w1[(size_t)j * DX + k], dxc);
        dxd = fmaf(g, w1[(size_t)j * DX + D + k], dxd);
    }
}

// (The LayerNorm(cls) backward between dx_row and demo_row_bwd is NOT a block here: it stands, equal, in head_x_bwd_kernel,
//  head3_x_bwd_kernel and headr_x_bwd_kernel.  Under -ffp-contract=fast the compiler takes gy = dxc * ln_g into the first step of block_sum(gy) as one fma
//  where the code stands in the kernel, and as a rounded product plus an add where it is an inlined function: d cls then differs in
//  the last bit, and a bf16 training run drifts away from what it computed before (profiles/head_shared.txt).  A change to one
//  copy goes into the others.)

// ie_demo backward at column k (dxd = the gradient of the demo half of x), written to blocks 2 .. 6 of the slab row
//     [dln_g | dln_b | ddemo_g | ddemo_be | ddemo_w0 | ddemo_w1 | ddemo_b] = 7 x 256
// WIL: the two columns of ie_demo.0.weight's gradient interleaved in the slab row ([256][2], the parameter's own layout) instead of
// as two rows of 256 -- the reduction then writes the parameter's gradient slice as it stands.
template <bool WIL> MTMP_DEV void demo_row_bwd(float a, float g, const Shared3& p, float dxd, float eps, float* red, int k, float* row) {
    const float u = fmaf(a, p.demo_w[2 * k], fmaf(g, p.demo_w[2 * k + 1], p.demo_b[k]));
    const float mean = block_sum(u, red, k) * (1.0f / D);
    const float d = u - mean;
    const float rstd = rsqrtf(block_sum(d * d, red, k) * (1.0f / D) + eps);
    const float xh = d * rstd;
    const float dyd = fmaf(xh, p.demo_g[k], p.demo_be[k]) > 0.f ? dxd : 0.f;
    const float gy = dyd * p.demo_g[k];
    const float m1 = block_sum(gy, red, k) * (1.0f / D), m2 = block_sum(gy * xh, red, k) * (1.0f / D);
    const float du = rstd * (gy - m1 - xh * m2);
    row[2 * D + k] = dyd * xh;
    row[3 * D + k] = dyd;
    if (WIL) {
        row[4 * D + 2 * k] = du * a;
        row[4 * D + 2 * k + 1] = du * g;
    } else {
        row[4 * D + k] = du * a;
        row[5 * D + k] = du * g;
    }
    row[6 * D + k] = du;
}

// column sums of the slab, every 256-column block to a destination of its own (block i -> d[i]; blocks 4 and 5 are the interleaved
// ie_demo.0.weight gradient: one destination of 512, d[5] unused)
struct RowDst { float* d[7]; };
// (a block = 64 columns x 4 row lanes combined in a fixed order: 28 blocks -- as 7 blocks of 256 columns walking all rows one after
//  the other this launch took 16 us on the chain between the loss and the backward)
__global__ __launch_bounds__(256) void rows_scatter_kernel(const float* slab, int rows, RowDst t) {
    __shared__ float part[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    float s0 = 0.f, s1 = 0.f;
    int r = rl;
    for (; r + 4 < rows; r += 8) {
        s0 += slab[(size_t)r * 7 * D + c];
        s1 += slab[(size_t)(r + 4) * 7 * D + c];
    }
    if (r < rows) s0 += slab[(size_t)r * 7 * D + c];
    part[rl][cl] = s0 + s1;
    __syncthreads();
    if (rl == 0) {
        const float s = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
        const int blk = c / D, k = c - blk * D;
        if (blk == 5) t.d[4][D + k] = s;
        else t.d[blk][k] = s;
    }
}
// slab blocks: dln_g, dln_b, ddemo_g, ddemo_be, ddemo_w (two blocks, interleaved), ddemo_b; dst = the gradients' destinations in
// parameter order (the six Shared3 parameters first)
inline void launch_rows_scatter(const float* slab, int rows, float* const* dst, hipStream_t st) {
    RowDst t{{dst[4], dst[5], dst[2], dst[3], dst[0], nullptr, dst[1]}};
    hipLaunchKernelGGL(rows_scatter_kernel, dim3(7 * D / 64), dim3(256), 0, st, slab, rows, t);
}

}  // namespace
