// Classification head of TRI_MBT_VSLTCLS (K10, tri_mbt_vsltcls.py:59-76 `ie_demo`, :248-255 head) for gfx950:
//     demo = ReLU(LN(age * w[:,0] + gender * w[:,1] + b))                         ie_demo (Linear(2,256), LayerNorm, ReLU)
//     x    = [ LN(cls) | demo ]                                                   layer_norms_after_concat, torch.cat
//     h    = x W1^T + b1 ;  y = BatchNorm1d(h) ;  a = ReLU(y) ;  out = a W2^T + b2  fc_list.{0,1,2,3}
// Everything here is a few hundred KFLOP on B <= 256 rows: the torch modules cost ~65 launches of ~5 us forward +
// backward, all of them on the critical path between the forward and the backward of the step.  Six launches here.
//   forward : head_x (one wave per row: the two LayerNorms) -> head_fc (feature-parallel: 4 features per workgroup,
//             a wave = one feature x all rows -- R = 1, 2 or 4 rows per lane --, so the BatchNorm statistics are wave reductions) -> head_out
//   backward: head_fc_bwd (feature-parallel: BatchNorm / Linear weight gradients, dh) -> head_x_bwd (row-parallel:
//             dx = dh W1, both LayerNorm backwards, per-row partials of the row-summed gradients) -> slab reduce
// fp32 throughout (the reference runs the head in fp32 under autocast too).  Deterministic: no float atomics.
// The pieces this head shares with the three-row LayerNorm head (head3.hip) -- the ie_demo row each way, the LN(cls) row forward, the
// dW1 and dx loops, the slab scatter -- are the blocks of head_common.hip.h; the kernels are this file's.
// Two input widths W, one set of kernels.  W == DX (512) is the head above.  W == D (256) is the head of --vslt-type QIE
// (tri_mbt_vsltcls.py:148-151, 248-250): the demographic embedding went into the streams' tokens (qie.hip), nothing is concatenated,
// x = LN(cls) and fc_list.0 is [256][256].  Same launches, interface forms and arithmetic; `if constexpr (W == DX)` stands where the
// ie_demo half exists, and the blocks that walk x or W1 with a row stride of 512 (dw1_rows, dx_row) give way to one-half loops.
#include <string>

#include "head_common.hip.h"

namespace {

struct HeadParams {
    Shared3 s;                                                                              // ie_demo (null at W == D), ln_after_concat
    const float* w1; const float* b1;                                                       // fc_list.0 [256][W]
    const float* bn_g; const float* bn_b; float* run_mean; float* run_var;                  // fc_list.1
    const float* w2; const float* b2;                                                       // fc_list.3 [1][256]
};
template <int W> constexpr int NPARAMS = W == DX ? 14 : 10;   // device pointers in the parameter table of include/mtmp.h
// the table is in HeadParams order, at W == D without ie_demo's four
template <int W> inline HeadParams head_params_of(const void* const* q) {
    const Shared3 s = W == DX ? shared_of(q) : Shared3{nullptr, nullptr, nullptr, nullptr, (const float*)q[0], (const float*)q[1]};
    q += NPARAMS<W> - 8;
    return HeadParams{s, (const float*)q[0], (const float*)q[1], (const float*)q[2], (const float*)q[3],
                      (float*)q[4], (float*)q[5], (const float*)q[6], (const float*)q[7]};
}

// x[b] = [LN(cls[b]) | ReLU(LN(age*w0 + gen*w1 + b))]; one wave per row, lane owns 4 columns of each half (W == D: of LN(cls[b]);
// age and gen are not read).
template <typename TC, int W>
__global__ __launch_bounds__(256) void head_x_kernel(const TC* cls, const float* age, const float* gen, HeadParams p,
                                                     float* x, int B, float eps, long long* nbt) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;          // BatchNorm1d.num_batches_tracked (one launch less in front of the head)
    if (b >= B) return;
    const int c = 4 * lane;
    *reinterpret_cast<f32x4*>(x + (size_t)b * W + c) = cls_row_fwd(cls + (size_t)b * D, p.s, c, eps);
    if constexpr (W == DX) *reinterpret_cast<f32x4*>(x + (size_t)b * W + D + c) = demo_row_fwd(age[b], gen[b], p.s, c, eps);
}

// workgroup g owns features 4g..4g+3; thread = (rows b = lane + 64 rr for rr < R, feature jj = wave)
template <int R, int W>
__global__ __launch_bounds__(256) void head_fc_kernel(const float* x, HeadParams p, float* hhat, float* rstd_out, float* partial,
                                                      int B, float eps, float momentum, int training) {
    constexpr int NB = 64 * R;                  // row capacity of this instantiation
    __shared__ float xT[64][NB + 1];            // one 64-column chunk of x, transposed: xT[k][b]
    __shared__ float pl[FPW][NB];
    const int tid = threadIdx.x, lane = tid & 63, jj = __builtin_amdgcn_readfirstlane(tid >> 6), j = blockIdx.x * FPW + jj;
    const float* wrow = p.w1 + (size_t)j * W;
    float acc[R];           // the tile product: inline here, in head3_fc_kernel and headr_fc_kernel, not a block (head_common.hip.h)
#pragma unroll
    for (int rr = 0; rr < R; ++rr) acc[rr] = 0.f;
    for (int k0 = 0; k0 < W; k0 += 64) {
        __syncthreads();
        // NB rows x 64 columns: thread t loads rows (t>>2) + 64 rr, columns 16*(t&3) .. +15
        const int cs = 16 * (tid & 3);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int r = (tid >> 2) + 64 * rr;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (r < B) v = *reinterpret_cast<const f32x4*>(x + (size_t)r * W + k0 + cs + 4 * q);
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

__global__ __launch_bounds__(256) void head_out_kernel(const float* partial, const float* b2, float* out, int B, int nb) {
    const int b = threadIdx.x;                  // nb = row stride of `partial` (64 x rows per lane)
    if (b >= B) return;
    float s = 0.f;
    for (int g = 0; g < D / FPW; ++g) s += partial[(size_t)g * nb + b];
    out[b] = s + b2[0];
}

// feature-parallel backward: dW2, db2, dbn_g, dbn_b, db1, dW1, dh[b][j]
template <int R, int W>
__global__ __launch_bounds__(256) void head_fc_bwd_kernel(const float* dout, const float* x, const float* hhat, const float* rstd_in,
                                                          HeadParams p, float* dh_out, float* dw1, float* db1, float* dbn_g,
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
    if constexpr (W == DX) {
        float s0[FPW], s1[FPW];
        dw1_rows(dhs, x, B, s0, s1);
#pragma unroll
        for (int f = 0; f < FPW; ++f) {
            dw1[(size_t)(blockIdx.x * FPW + f) * DX + tid] = s0[f];
            dw1[(size_t)(blockIdx.x * FPW + f) * DX + D + tid] = s1[f];
        }
    } else {            // dw1_rows on one half: thread t owns column t of the workgroup's four rows of W1
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
}

// row-parallel backward: workgroup = row b, thread = column k of each half of x.  Slab row b and WIL: demo_row_bwd (W == D: the
// row keeps its 7 x 256 layout, blocks 2 .. 6 are not written and not read).
template <typename TC, bool WIL, int W>
__global__ __launch_bounds__(256) void head_x_bwd_kernel(const float* dh, const TC* cls, const float* age, const float* gen,
                                                         HeadParams p, TC* dcls, float* slab, float eps) {
    __shared__ float dhr[D];
    __shared__ float red[4];
    const int b = blockIdx.x, k = threadIdx.x;
    dhr[k] = dh[(size_t)b * D + k];
    __syncthreads();
    float dxc = 0.f, dxd = 0.f;
    if constexpr (W == DX) dx_row(dhr, p.w1, k, dxc, dxd);
    else for (int j = 0; j < D; ++j) dxc = fmaf(dhr[j], p.w1[(size_t)j * D + k], dxc);        // dx_row on one half
    float* row = slab + (size_t)b * 7 * D;
    // LayerNorm(cls) backward: inline here, in head3_x_bwd_kernel and headr_x_bwd_kernel, not a block (head_common.hip.h says why)
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
    if constexpr (W == DX) demo_row_bwd<WIL>(age[b], gen[b], p.s, dxd, eps, red, k, row);
}

// out[c] = sum_r slab[r][c], r < rows <= 256: 256 threads over columns
__global__ __launch_bounds__(256) void head_rows_reduce_kernel(const float* slab, int rows, int cols, float* out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += slab[(size_t)r * cols + c];
    out[c] = s;
}

// BCEWithLogitsLoss(reduction="mean") (2_train.py:76, trainer.py:128): loss = mean_b [max(o,0) - o t + log(1 + exp(-|o|))];
// dlogit[b] = (sigmoid(o) - t) / n is produced alongside (the backward is a scale by the incoming scalar).
__global__ __launch_bounds__(256) void bce_logits_kernel(const float* o, const float* t, float* loss, float* dlogit, int n) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float x = o[i], y = t[i];
        s += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
        dlogit[i] = (1.0f / (1.0f + expf(-x)) - y) / (float)n;
    }
    s = block_sum(s, red, threadIdx.x);
    if (threadIdx.x == 0) loss[0] = s / (float)n;
}

}  // namespace

extern "C" int mtmp_bce_logits_mean(const float* logits, const float* target, float* loss, float* dlogit, int n, void* stream) {
    MTMP_CHECK_ARG(logits && target && loss && dlogit && n > 0, "mtmp_bce_logits_mean: bad argument");
    hipLaunchKernelGGL(bce_logits_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, target, loss, dlogit, n);
    MTMP_CHECK_LAUNCH("mtmp_bce_logits_mean");
    return MTMP_OK;
}

// ---- host side: one set of templates for both widths; `who` = the exported entry that was called, named in every message ----
#define HEAD_CHECK_LAUNCH(who, stage) MTMP_CHECK_LAUNCH((std::string(who) + "(" stage ")").c_str())

// ws_fwd: x[B][W] + hhat[B][256] + rstd[256] + partial[64][64 x rows per lane] floats (kept for the backward)
template <int W> static int head_ws_floats(int B) { return B * W + B * D + D + (D / FPW) * 64 * rows_per_lane(B); }
extern "C" int mtmp_head_ws_floats(int B) { return head_ws_floats<DX>(B); }
extern "C" int mtmp_headq_ws_floats(int B) { return head_ws_floats<D>(B); }

// The argument checks of every entry.  ptrs: the entry's own pointer arguments are all there.  1 <= B <= 256 (one, two or four rows
// per lane); the forward (`fwd`) wants B > 1 in training mode; the CLS type; every pointer of the parameter table.
template <int W>
static int head_check(const char* who, bool fwd, bool ptrs, const void* const* params, int B, int training, int cls_dtype) {
    const bool ok = ptrs && params && B > 0 && B <= MAXB && (cls_dtype == 0 || cls_dtype == 1);
    if (fwd)
        MTMP_CHECK_ARG(ok && (training == 0 || B > 1),
                       "%s: bad argument (B=%d, needs 1 <= B <= %d, and B > 1 in training mode; dtype %d)", who, B, MAXB, cls_dtype);
    else
        MTMP_CHECK_ARG(ok, "%s: bad argument (B=%d dtype %d)", who, B, cls_dtype);
    for (int i = 0; i < NPARAMS<W>; ++i) MTMP_CHECK_ARG(params[i], "%s: parameter %d is NULL", who, i);
    return MTMP_OK;
}

// the three forward launches; num_batches_tracked (int64 on the device, may be NULL) is incremented by the first.  age / gender are
// NULL at W == D.
template <int W>
static int head_fwd(const char* who, int cls_dtype, const void* cls, const float* age, const float* gender, const void* const* params,
                    float* out, float* ws, int B, float ln_eps, float bn_eps, float momentum, int training,
                    long long* num_batches_tracked, hipStream_t st) {
    const int rc = head_check<W>(who, true, cls && (W == D || (age && gender)) && out && ws, params, B, training, cls_dtype);
    if (rc != MTMP_OK) return rc;
    const HeadParams p = head_params_of<W>(params);
    float* x = ws; float* hhat = x + (size_t)B * W; float* rstd = hhat + (size_t)B * D; float* partial = rstd + D;
    if (cls_dtype == 0)
        hipLaunchKernelGGL((head_x_kernel<float, W>), dim3((B + 3) / 4), dim3(256), 0, st, (const float*)cls, age, gender, p, x, B, ln_eps,
                           num_batches_tracked);
    else
        hipLaunchKernelGGL((head_x_kernel<bf16, W>), dim3((B + 3) / 4), dim3(256), 0, st, (const bf16*)cls, age, gender, p, x, B, ln_eps,
                           num_batches_tracked);
    HEAD_CHECK_LAUNCH(who, "x");
    const int R = rows_per_lane(B);
    auto fc = R == 1 ? head_fc_kernel<1, W> : (R == 2 ? head_fc_kernel<2, W> : head_fc_kernel<4, W>);
    hipLaunchKernelGGL(fc, dim3(D / FPW), dim3(256), 0, st, (const float*)x, p, hhat, rstd, partial, B, bn_eps, momentum, training);
    HEAD_CHECK_LAUNCH(who, "fc");
    hipLaunchKernelGGL(head_out_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, p.b2, out, B, 64 * R);
    HEAD_CHECK_LAUNCH(who, "out");
    return MTMP_OK;
}

// the first two backward launches: the feature-parallel kernel writes dW1, db1, dbn_g, dbn_b, dW2, db2 to feat[0..5], the
// row-parallel one d cls and the slab (ws_bwd + B*256) that the caller's last launch reduces.  ws_bwd: B*256 + B*7*256 floats.
template <int W, bool WIL>
static int head_bwd_rows(const char* who, int cls_dtype, const float* d_out, const void* cls, const float* age, const float* gender,
                         const void* const* params, const float* ws_fwd, void* dcls, float* const* feat, float* ws_bwd, int B,
                         float ln_eps, int training, hipStream_t st) {
    const HeadParams p = head_params_of<W>(params);
    const float* x = ws_fwd; const float* hhat = x + (size_t)B * W; const float* rstd = hhat + (size_t)B * D;
    float* dh = ws_bwd; float* slab = dh + (size_t)B * D;
    const int R = rows_per_lane(B);
    auto fcb = R == 1 ? head_fc_bwd_kernel<1, W> : (R == 2 ? head_fc_bwd_kernel<2, W> : head_fc_bwd_kernel<4, W>);
    hipLaunchKernelGGL(fcb, dim3(D / FPW), dim3(256), 0, st, d_out, x, hhat, rstd, p, dh, feat[0], feat[1], feat[2], feat[3], feat[4],
                       feat[5], B, training);
    HEAD_CHECK_LAUNCH(who, "fc");
    if (cls_dtype == 0)
        hipLaunchKernelGGL((head_x_bwd_kernel<float, WIL, W>), dim3(B), dim3(256), 0, st, (const float*)dh, (const float*)cls, age, gender,
                           p, (float*)dcls, slab, ln_eps);
    else if constexpr (WIL)                                    // (mtmp_head_bwd, the form without WIL, takes float rows only)
        hipLaunchKernelGGL((head_x_bwd_kernel<bf16, WIL, W>), dim3(B), dim3(256), 0, st, (const float*)dh, (const bf16*)cls, age, gender,
                           p, (bf16*)dcls, slab, ln_eps);
    HEAD_CHECK_LAUNCH(who, "x");
    return MTMP_OK;
}

// the whole backward with every trained parameter's gradient written to a destination of its own: dst in the order of the
// parameter table without the two running statistics (12 at W == DX, 8 at W == D)
template <int W>
static int head_bwd_scatter(const char* who, int cls_dtype, const float* d_out, const void* cls, const float* age, const float* gender,
                            const void* const* params, const float* ws_fwd, void* dcls, float* const* dst, float* ws_bwd, int B,
                            float ln_eps, int training, hipStream_t st) {
    constexpr int ND = NPARAMS<W> - 2;
    int rc = head_check<W>(who, false, d_out && cls && (W == D || (age && gender)) && ws_fwd && dcls && dst && ws_bwd, params, B, training,
                           cls_dtype);
    if (rc != MTMP_OK) return rc;
    for (int i = 0; i < ND; ++i) MTMP_CHECK_ARG(dst[i], "%s: destination %d is NULL", who, i);
    rc = head_bwd_rows<W, true>(who, cls_dtype, d_out, cls, age, gender, params, ws_fwd, dcls, dst + ND - 6, ws_bwd, B, ln_eps, training, st);
    if (rc != MTMP_OK) return rc;
    const float* slab = ws_bwd + (size_t)B * D;
    if constexpr (W == DX) {
        launch_rows_scatter(slab, B, dst, st);
    } else {            // the first two 256-column blocks of the slab rows: d layer_norms_after_concat.{weight, bias}
        const RowDst t{{dst[0], dst[1], nullptr, nullptr, nullptr, nullptr, nullptr}};
        hipLaunchKernelGGL(rows_scatter_kernel, dim3(2 * D / 64), dim3(256), 0, st, slab, B, t);
    }
    HEAD_CHECK_LAUNCH(who, "reduce");
    return MTMP_OK;
}

// params: 14 device pointers in HeadParams order (float; run_mean / run_var are updated in place when training).
// cls float[B][256], age / gender float[B]; out float[B]; B <= 256 (one, two or four rows per lane).
extern "C" int mtmp_head_fwd(const float* cls, const float* age, const float* gender, const void* const* params, float* out,
                             float* ws, int B, float ln_eps, float bn_eps, float momentum, int training, void* stream) {
    return head_fwd<DX>("mtmp_head_fwd", 0, cls, age, gender, params, out, ws, B, ln_eps, bn_eps, momentum, training, nullptr,
                        (hipStream_t)stream);
}

// grads (float, overwritten): dcls[B][256]; g_rows[7][256] = dln_g, dln_b, ddemo_g, ddemo_be, ddemo_w[:,0], ddemo_w[:,1],
// ddemo_b; dw1[256][512]; g_feat[4][256] = db1, dbn_g, dbn_b, dw2; db2[1].  ws_bwd: B*256 + B*7*256 floats.
extern "C" int mtmp_head_bwd(const float* d_out, const float* cls, const float* age, const float* gender,
                             const void* const* params, const float* ws_fwd, float* dcls, float* g_rows, float* dw1,
                             float* g_feat, float* db2, float* ws_bwd, int B, float ln_eps, int training, void* stream) {
    const char* who = "mtmp_head_bwd";
    int rc = head_check<DX>(who, false, d_out && cls && age && gender && ws_fwd && dcls && g_rows && dw1 && g_feat && db2 && ws_bwd,
                            params, B, training, 0);
    if (rc != MTMP_OK) return rc;
    float* const feat[6] = {dw1, g_feat, g_feat + D, g_feat + 2 * D, g_feat + 3 * D, db2};
    hipStream_t st = (hipStream_t)stream;
    rc = head_bwd_rows<DX, false>(who, 0, d_out, cls, age, gender, params, ws_fwd, dcls, feat, ws_bwd, B, ln_eps, training, st);
    if (rc != MTMP_OK) return rc;
    hipLaunchKernelGGL(head_rows_reduce_kernel, dim3(7), dim3(256), 0, st, (const float*)(ws_bwd + (size_t)B * D), B, 7 * D, g_rows);
    HEAD_CHECK_LAUNCH(who, "reduce");
    return MTMP_OK;
}

// The head with the CLS vectors in the fusion stack's own type (ABI 6): cls / dcls [B][256] in `cls_dtype` (MTMP_F32 | MTMP_BF16: no
// cast launch on either side of the head), num_batches_tracked (int64 on the device, may be NULL) incremented by the first launch,
// and every parameter's gradient written to a destination of its own -- dst[12] in the order of the 12 trained parameters
// (ie_demo.0.weight [256][2], ie_demo.0.bias, ie_demo.1.weight, ie_demo.1.bias, layer_norms_after_concat.{weight,bias},
// fc_list.0.{weight [256][512], bias}, fc_list.1.{weight, bias}, fc_list.3.{weight, bias}): slices of the flat gradient buffer,
// or scratch.  ws_bwd: B*256 + B*7*256 floats.
extern "C" int mtmp_head_fwd_t(int cls_dtype, const void* cls, const float* age, const float* gender, const void* const* params,
                               float* out, float* ws, int B, float ln_eps, float bn_eps, float momentum, int training,
                               long long* num_batches_tracked, void* stream) {
    return head_fwd<DX>("mtmp_head_fwd_t", cls_dtype, cls, age, gender, params, out, ws, B, ln_eps, bn_eps, momentum, training,
                        num_batches_tracked, (hipStream_t)stream);
}
extern "C" int mtmp_head_bwd_scatter(int cls_dtype, const float* d_out, const void* cls, const float* age, const float* gender,
                                     const void* const* params, const float* ws_fwd, void* dcls, float* const* dst, float* ws_bwd,
                                     int B, float ln_eps, int training, void* stream) {
    return head_bwd_scatter<DX>("mtmp_head_bwd_scatter", cls_dtype, d_out, cls, age, gender, params, ws_fwd, dcls, dst, ws_bwd, B, ln_eps,
                                training, (hipStream_t)stream);
}

// The same two entries at W == D (--vslt-type QIE): no age / gender, params: 10 device pointers (HeadParams order without ie_demo's
// four), dst[8]: layer_norms_after_concat.{weight,bias}, fc_list.0.{weight [256][256], bias}, fc_list.1.{weight, bias},
// fc_list.3.{weight, bias}.  The slab row keeps its 7 x 256 layout; its first two blocks are summed.
extern "C" int mtmp_headq_fwd_t(int cls_dtype, const void* cls, const void* const* params, float* out, float* ws, int B, float ln_eps,
                                float bn_eps, float momentum, int training, long long* num_batches_tracked, void* stream) {
    return head_fwd<D>("mtmp_headq_fwd_t", cls_dtype, cls, nullptr, nullptr, params, out, ws, B, ln_eps, bn_eps, momentum, training,
                       num_batches_tracked, (hipStream_t)stream);
}
extern "C" int mtmp_headq_bwd_scatter(int cls_dtype, const float* d_out, const void* cls, const void* const* params, const float* ws_fwd,
                                      void* dcls, float* const* dst, float* ws_bwd, int B, float ln_eps, int training, void* stream) {
    return head_bwd_scatter<D>("mtmp_headq_bwd_scatter", cls_dtype, d_out, cls, nullptr, nullptr, params, ws_fwd, dcls, dst, ws_bwd, B, ln_eps,
                               training, (hipStream_t)stream);
}
