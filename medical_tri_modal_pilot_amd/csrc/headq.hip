// Classification head of TRI_MBT_VSLTCLS with --vslt-type QIE (tri_mbt_vsltcls.py:148-151, 248-250) for gfx950: the demographic
// embedding went into the streams' tokens (qie.hip), so nothing is concatenated in front of the head and it reads 256 columns:
//     x = LN(cls)                                                                layer_norms_after_concat
//     h = x W1^T + b1 ;  y = BatchNorm1d(h) ;  a = ReLU(y) ;  out = a W2^T + b2   fc_list.{0,1,2,3}, W1 [256][256]
// The BatchNorm head of head.hip minus its ie_demo half: the same six launches, interface forms (CLS rows in the stack's type, the
// batch counter on the device, running statistics in place, training / eval, B <= 256, one / two / four rows per lane) and
// arithmetic, on rows of 256.
//   forward : headq_x (one wave per row) -> headq_fc (4 features per workgroup, a wave = one feature x all rows) -> headq_out
//   backward: headq_fc_bwd (BatchNorm / Linear weight gradients, dh) -> headq_x_bwd (dx = dh W1, LayerNorm backward, per-row
//             partials of d layer_norms_after_concat) -> rows_scatter (head_common.hip.h; the slab row keeps its 7 x 256 layout, the
//             first two blocks are summed)
// From head_common.hip.h: cls_row_fwd, block_sum, wave reductions, rows_scatter_kernel.  The blocks that walk x or W1 with a row
// stride of 512 (dw1_rows, dx_row) do not apply to a 256-wide x; their loops stand here on 256 columns.  The tile product and the
// LayerNorm(cls) backward are the copies head_common.hip.h's two "NOT a block" notes speak of: a change to head.hip's goes in here.
// fp32 throughout.  Deterministic: no float atomics.
#include "head_common.hip.h"

namespace {

struct HeadQParams {
    Shared3 s;                                                                              // layer_norms_after_concat (no ie_demo)
    const float* w1; const float* b1;                                                       // fc_list.0 [256][256]
    const float* bn_g; const float* bn_b; float* run_mean; float* run_var;                  // fc_list.1
    const float* w2; const float* b2;                                                       // fc_list.3 [1][256]
};
inline HeadQParams headq_params_of(const void* const* q) {      // the 10 device pointers of include/mtmp.h, in this order
    return HeadQParams{Shared3{nullptr, nullptr, nullptr, nullptr, (const float*)q[0], (const float*)q[1]},
                       (const float*)q[2], (const float*)q[3], (const float*)q[4], (const float*)q[5], (float*)q[6], (float*)q[7],
                       (const float*)q[8], (const float*)q[9]};
}

// x[b] = LN(cls[b]); one wave per row, lane owns 4 columns
template <typename TC>
__global__ __launch_bounds__(256) void headq_x_kernel(const TC* cls, HeadQParams p, float* x, int B, float eps, long long* nbt) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;          // BatchNorm1d.num_batches_tracked
    if (b >= B) return;
    const int c = 4 * lane;
    *reinterpret_cast<f32x4*>(x + (size_t)b * D + c) = cls_row_fwd(cls + (size_t)b * D, p.s, c, eps);
}

// workgroup g owns features 4g..4g+3; thread = (rows b = lane + 64 rr for rr < R, feature jj = wave)
template <int R>
__global__ __launch_bounds__(256) void headq_fc_kernel(const float* x, HeadQParams p, float* hhat, float* rstd_out, float* partial,
                                                       int B, float eps, float momentum, int training) {
    constexpr int NB = 64 * R;                  // row capacity of this instantiation
    __shared__ float xT[64][NB + 1];            // one 64-column chunk of x, transposed: xT[k][b]
    __shared__ float pl[FPW][NB];
    const int tid = threadIdx.x, lane = tid & 63, jj = __builtin_amdgcn_readfirstlane(tid >> 6), j = blockIdx.x * FPW + jj;
    const float* wrow = p.w1 + (size_t)j * D;
    float acc[R];           // the tile product of head_fc_kernel on 256 columns (head_common.hip.h: not a block)
#pragma unroll
    for (int rr = 0; rr < R; ++rr) acc[rr] = 0.f;
    for (int k0 = 0; k0 < D; k0 += 64) {
        __syncthreads();
        // NB rows x 64 columns: thread t loads rows (t>>2) + 64 rr, columns 16*(t&3) .. +15
        const int cs = 16 * (tid & 3);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int r = (tid >> 2) + 64 * rr;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (r < B) v = *reinterpret_cast<const f32x4*>(x + (size_t)r * D + k0 + cs + 4 * q);
#pragma unroll
                for (int i = 0; i < 4; ++i) xT[cs + 4 * q + i][r] = v[i];
            }
        }
        __syncthreads();
#pragma unroll 16
        for (int kk = 0; kk < 64; ++kk) {
            const float wv = wrow[k0 + kk];
#pragma unroll
            for (int rr = 0; rr < R; ++rr) acc[rr] = fmaf(xT[kk][lane + 64 * rr], wv, acc[rr]);
        }
    }
    float h[R];
    bool live[R];
    float sh = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        h[rr] = acc[rr] + p.b1[j];
        live[rr] = lane + 64 * rr < B;
        sh += live[rr] ? h[rr] : 0.f;
    }
    float mean, var;
    if (training) {
        mean = wave_sum(sh) / (float)B;
        float sv = 0.f;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) { const float dv = live[rr] ? h[rr] - mean : 0.f; sv += dv * dv; }
        var = wave_sum(sv) / (float)B;                                         // biased, used for normalisation
        if (lane == 0) {                                                       // running statistics (unbiased variance)
            p.run_mean[j] = (1.0f - momentum) * p.run_mean[j] + momentum * mean;
            p.run_var[j] = (1.0f - momentum) * p.run_var[j] + momentum * var * ((float)B / (float)max(B - 1, 1));
        }
    } else {
        mean = p.run_mean[j];
        var = p.run_var[j];
    }
    const float rstd = rsqrtf(var + eps);
    if (lane == 0) rstd_out[j] = rstd;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int b = lane + 64 * rr;
        const float hh = (h[rr] - mean) * rstd;
        const float a = fmaxf(fmaf(hh, p.bn_g[j], p.bn_b[j]), 0.f);
        if (live[rr]) hhat[(size_t)b * D + j] = hh;
        pl[jj][b] = live[rr] ? a * p.w2[j] : 0.f;
    }
    __syncthreads();
    for (int t = tid; t < NB; t += 256) partial[(size_t)blockIdx.x * NB + t] = pl[0][t] + pl[1][t] + pl[2][t] + pl[3][t];
}

__global__ __launch_bounds__(256) void headq_out_kernel(const float* partial, const float* b2, float* out, int B, int nb) {
    const int b = threadIdx.x;                  // nb = row stride of `partial` (64 x rows per lane)
    if (b >= B) return;
    float s = 0.f;
    for (int g = 0; g < D / FPW; ++g) s += partial[(size_t)g * nb + b];
    out[b] = s + b2[0];
}

// feature-parallel backward: dW2, db2, dbn_g, dbn_b, db1, dW1, dh[b][j]
template <int R>
__global__ __launch_bounds__(256) void headq_fc_bwd_kernel(const float* dout, const float* x, const float* hhat, const float* rstd_in,
                                                           HeadQParams p, float* dh_out, float* dw1, float* db1, float* dbn_g,
                                                           float* dbn_b, float* dw2, float* db2, int B, int training) {
    constexpr int NB = 64 * R;
    __shared__ float dhs[FPW][NB];
    const int tid = threadIdx.x, lane = tid & 63, jj = __builtin_amdgcn_readfirstlane(tid >> 6), j = blockIdx.x * FPW + jj;
    const float gam = p.bn_g[j], rstd = rstd_in[j];
    float dl[R], hh[R], dy[R];
    bool live[R];
    float t_w2 = 0.f, t_g = 0.f, t_b = 0.f, t_dl = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int b = lane + 64 * rr;
        live[rr] = b < B;
        dl[rr] = live[rr] ? dout[b] : 0.f;
        hh[rr] = live[rr] ? hhat[(size_t)b * D + j] : 0.f;
        const float y = fmaf(hh[rr], gam, p.bn_b[j]);
        const float a = fmaxf(y, 0.f);
        dy[rr] = (live[rr] && y > 0.f) ? dl[rr] * p.w2[j] : 0.f;
        t_w2 += dl[rr] * a; t_g += dy[rr] * hh[rr]; t_b += dy[rr]; t_dl += dl[rr];
    }
    const float s_w2 = wave_sum(t_w2), s_g = wave_sum(t_g), s_b = wave_sum(t_b);
    float t_b1 = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int b = lane + 64 * rr;
        const float dh = training ? gam * rstd * (dy[rr] - s_b / (float)B - hh[rr] * s_g / (float)B) : gam * rstd * dy[rr];
        const float dhl = live[rr] ? dh : 0.f;
        t_b1 += dhl;
        if (live[rr]) dh_out[(size_t)b * D + j] = dh;
        dhs[jj][b] = dhl;
    }
    const float s_b1 = wave_sum(t_b1);
    if (lane == 0) { dw2[j] = s_w2; dbn_g[j] = s_g; dbn_b[j] = s_b; db1[j] = s_b1; }
    if (blockIdx.x == 0 && jj == 0) {
        const float s = wave_sum(t_dl);
        if (lane == 0) db2[0] = s;
    }
    __syncthreads();
    // dW1[j][k] = sum_b dh[b][j] x[b][k] for the workgroup's four features: thread t owns column t of those four rows of W1
    float s0[FPW];
#pragma unroll
    for (int f = 0; f < FPW; ++f) s0[f] = 0.f;
    for (int r = 0; r < B; ++r) {
        const float x0 = x[(size_t)r * D + tid];
#pragma unroll
        for (int f = 0; f < FPW; ++f) s0[f] = fmaf(dhs[f][r], x0, s0[f]);
    }
#pragma unroll
    for (int f = 0; f < FPW; ++f) dw1[(size_t)(blockIdx.x * FPW + f) * D + tid] = s0[f];
}

// row-parallel backward: workgroup = row b, thread = column k of x.  Slab row b: [dln_g | dln_b | five unused blocks] = 7 x 256.
template <typename TC>
__global__ __launch_bounds__(256) void headq_x_bwd_kernel(const float* dh, const TC* cls, HeadQParams p, TC* dcls, float* slab, float eps) {
    __shared__ float dhr[D];
    __shared__ float red[4];
    const int b = blockIdx.x, k = threadIdx.x;
    dhr[k] = dh[(size_t)b * D + k];
    __syncthreads();
    float dxc = 0.f;                                      // dx = dh W1 at column k
    for (int j = 0; j < D; ++j) dxc = fmaf(dhr[j], p.w1[(size_t)j * D + k], dxc);
    float* row = slab + (size_t)b * 7 * D;
    // LayerNorm(cls) backward: head_x_bwd_kernel's, inline (head_common.hip.h: not a block)
    {
        const float v = to_f32(cls[(size_t)b * D + k]);
        const float mean = block_sum(v, red, k) * (1.0f / D);
        const float d = v - mean;
        const float rstd = rsqrtf(block_sum(d * d, red, k) * (1.0f / D) + eps);
        const float xh = d * rstd, gy = dxc * p.s.ln_g[k];
        const float m1 = block_sum(gy, red, k) * (1.0f / D), m2 = block_sum(gy * xh, red, k) * (1.0f / D);
        dcls[(size_t)b * D + k] = from_f32<TC>(rstd * (gy - m1 - xh * m2));
        row[k] = dxc * xh;
        row[D + k] = dxc;
    }
}

}  // namespace

// ws_fwd: x[B][256] + hhat[B][256] + rstd[256] + partial[64][64 x rows per lane] floats (kept for the backward)
extern "C" int mtmp_headq_ws_floats(int B) { return 2 * B * D + D + (D / FPW) * 64 * rows_per_lane(B); }

// params: 10 device pointers in HeadQParams order (float; run_mean / run_var are updated in place when training).
// cls [B][256] in cls_dtype; out float[B]; B <= 256; num_batches_tracked (int64 on the device, may be NULL) is incremented by the
// first launch.
extern "C" int mtmp_headq_fwd_t(int cls_dtype, const void* cls, const void* const* params, float* out, float* ws, int B, float ln_eps,
                                float bn_eps, float momentum, int training, long long* num_batches_tracked, void* stream) {
    MTMP_CHECK_ARG(cls && params && out && ws && B > 0 && B <= MAXB && (training == 0 || B > 1) && (cls_dtype == 0 || cls_dtype == 1),
                   "mtmp_headq_fwd_t: bad argument (B=%d, needs 1 <= B <= %d, and B > 1 in training mode; dtype %d)", B, MAXB, cls_dtype);
    for (int i = 0; i < 10; ++i) MTMP_CHECK_ARG(params[i], "mtmp_headq_fwd_t: parameter %d is NULL", i);
    const HeadQParams p = headq_params_of(params);
    hipStream_t st = (hipStream_t)stream;
    float* x = ws; float* hhat = x + (size_t)B * D; float* rstd = hhat + (size_t)B * D; float* partial = rstd + D;
    if (cls_dtype == 0)
        hipLaunchKernelGGL(headq_x_kernel<float>, dim3((B + 3) / 4), dim3(256), 0, st, (const float*)cls, p, x, B, ln_eps, num_batches_tracked);
    else
        hipLaunchKernelGGL(headq_x_kernel<bf16>, dim3((B + 3) / 4), dim3(256), 0, st, (const bf16*)cls, p, x, B, ln_eps, num_batches_tracked);
    MTMP_CHECK_LAUNCH("mtmp_headq_fwd_t(x)");
    const int R = rows_per_lane(B);
    auto fc = R == 1 ? headq_fc_kernel<1> : (R == 2 ? headq_fc_kernel<2> : headq_fc_kernel<4>);
    hipLaunchKernelGGL(fc, dim3(D / FPW), dim3(256), 0, st, (const float*)x, p, hhat, rstd, partial, B, bn_eps, momentum, training);
    MTMP_CHECK_LAUNCH("mtmp_headq_fwd_t(fc)");
    hipLaunchKernelGGL(headq_out_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, p.b2, out, B, 64 * R);
    MTMP_CHECK_LAUNCH("mtmp_headq_fwd_t(out)");
    return MTMP_OK;
}

// dcls [B][256] in cls_dtype; dst[8]: the gradients of the eight trained parameters in the order of `params` without the running
// statistics (layer_norms_after_concat.{weight,bias}, fc_list.0.{weight [256][256], bias}, fc_list.1.{weight, bias},
// fc_list.3.{weight, bias}), overwritten: slices of the flat gradient buffer, or scratch.  ws_bwd: B*256 + B*7*256 floats.
extern "C" int mtmp_headq_bwd_scatter(int cls_dtype, const float* d_out, const void* cls, const void* const* params, const float* ws_fwd,
                                      void* dcls, float* const* dst, float* ws_bwd, int B, float ln_eps, int training, void* stream) {
    MTMP_CHECK_ARG(d_out && cls && params && ws_fwd && dcls && dst && ws_bwd && B > 0 && B <= MAXB && (cls_dtype == 0 || cls_dtype == 1),
                   "mtmp_headq_bwd_scatter: bad argument (B=%d dtype %d)", B, cls_dtype);
    for (int i = 0; i < 10; ++i) MTMP_CHECK_ARG(params[i], "mtmp_headq_bwd_scatter: parameter %d is NULL", i);
    for (int i = 0; i < 8; ++i) MTMP_CHECK_ARG(dst[i], "mtmp_headq_bwd_scatter: destination %d is NULL", i);
    const HeadQParams p = headq_params_of(params);
    hipStream_t st = (hipStream_t)stream;
    const float* x = ws_fwd; const float* hhat = x + (size_t)B * D; const float* rstd = hhat + (size_t)B * D;
    float* dh = ws_bwd; float* slab = dh + (size_t)B * D;
    const int R = rows_per_lane(B);
    auto fcb = R == 1 ? headq_fc_bwd_kernel<1> : (R == 2 ? headq_fc_bwd_kernel<2> : headq_fc_bwd_kernel<4>);
    hipLaunchKernelGGL(fcb, dim3(D / FPW), dim3(256), 0, st, d_out, x, hhat, rstd, p, dh, dst[2], dst[3], dst[4], dst[5], dst[6], dst[7], B,
                       training);
    MTMP_CHECK_LAUNCH("mtmp_headq_bwd_scatter(fc)");
    if (cls_dtype == 0)
        hipLaunchKernelGGL(headq_x_bwd_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)dh, (const float*)cls, p, (float*)dcls, slab, ln_eps);
    else
        hipLaunchKernelGGL(headq_x_bwd_kernel<bf16>, dim3(B), dim3(256), 0, st, (const float*)dh, (const bf16*)cls, p, (bf16*)dcls, slab, ln_eps);
    MTMP_CHECK_LAUNCH("mtmp_headq_bwd_scatter(x)");
    // the first two 256-column blocks of the slab rows: d layer_norms_after_concat.{weight, bias}
    const RowDst t{{dst[0], dst[1], nullptr, nullptr, nullptr, nullptr, nullptr}};
    hipLaunchKernelGGL(rows_scatter_kernel, dim3(2 * D / 64), dim3(256), 0, st, (const float*)slab, B, t);
    MTMP_CHECK_LAUNCH("mtmp_headq_bwd_scatter(reduce)");
    return MTMP_OK;
}
