// Three-row LayerNorm head of TRI_MBT_V1 / TRI_MBT_VNOSHAVGTR / TRI_MBT_VNOSHNOAVGTR (tri_mbt_v1.py:154-159,271-281,
// tri_mbt_vnoshavgtr.py:160-164,262-277, tri_mbt_vnoshnoavgtr.py:259-281) for gfx950, rows m = 0, 1, 2 = vslt, image, text:
//     demo[b]  = ReLU(LN(age[b] * w[:,0] + gender[b] * w[:,1] + b))               ie_demo, shared by the three rows
//     x[m,b]   = [ LN(cls_m[b]) | demo[b] ]                                       layer_norms_after_concat, torch.cat (512 wide)
//     h        = x[m,b] W1_m^T + b1_m ;  a = ReLU(LN(h; g_m, be_m)) ;  o[m,b] = a . w2_m + b2_m
// with one parameter set (W1, b1, g, be, w2, b2) per row, or ONE set shared by the three rows (the same pointers three times:
// its gradients are then the three rows' contributions summed in the fixed order m = 0, 1, 2 inside the kernels).
// The torch modules cost ~60 launches forward + backward on the critical path between the fusion stack's forward and its
// backward.  Here:
//   forward  (3): head3_x (one wave per row: the 3 B + B LayerNorms) -> head3_fc (feature-parallel 512 -> 256 product, 4 features
//                 per workgroup, a wave = one feature x all rows) -> head3_out (one wave per row: LayerNorm, ReLU, dot with w2)
//   backward (4): head3_row_bwd (one wave per row: dh through ReLU and LayerNorm) -> head3_fc_bwd (feature-parallel: every
//                 per-feature gradient and dW1) -> head3_x_bwd (workgroup per sample: dx = dh W1, the LayerNorm backwards, d cls_m,
//                 per-sample partials of the row-summed gradients) -> rows_scatter (slab -> destinations, fixed order)
// plus the candidate mean over the present modalities (one launch each way) and the masked mean BCE over the present
// (row, sample) pairs (one launch: loss and dlogit).  fp32 throughout.  Deterministic: no float atomics.
// The pieces this head shares with the BatchNorm head (head.hip) -- the ie_demo row each way, the LN(cls) row forward, the dW1 and
// dx loops, the slab scatter -- are the blocks of head_common.hip.h; the kernels are this file's.
#include "head_common.hip.h"

namespace {

struct HeadSet {      // Linear(512,256), LayerNorm(256), Linear(256,1) of one row
    const float* w1; const float* b1; const float* g; const float* be; const float* w2; const float* b2;
};
struct Sets3 { HeadSet s[3]; };
struct SetGrads { float* w1; float* b1; float* g; float* be; float* w2; float* b2; };
struct Grads3 { SetGrads s[3]; };
template <typename TC> struct Cls3 { const TC* p[3]; long long ld[3]; };     // CLS rows: p[m] + b * ld[m], 256 contiguous values
template <typename TC> struct DCls3 { TC* p[3]; };                            // [B][256] contiguous each

// rows 0 .. 3B-1: x[m][b][0:256] = LN(cls_m[b]); rows 3B .. 4B-1: demo[b] -> x[0..2][b][256:512].  One wave per row.
template <typename TC>
__global__ __launch_bounds__(256) void head3_x_kernel(Cls3<TC> cls, const float* age, const float* gen, Shared3 p, float* x, int B,
                                                      float eps) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= 4 * B) return;
    const int c = 4 * lane;
    if (r < 3 * B) {
        const int m = r / B, b = r - m * B;
        *reinterpret_cast<f32x4*>(x + ((size_t)m * B + b) * DX + c) = cls_row_fwd(cls.p[m] + (size_t)b * cls.ld[m], p, c, eps);
    } else {
        const int b = r - 3 * B;
        const f32x4 o = demo_row_fwd(age[b], gen[b], p, c, eps);
#pragma unroll
        for (int m = 0; m < 3; ++m) *reinterpret_cast<f32x4*>(x + ((size_t)m * B + b) * DX + D + c) = o;
    }
}

// workgroup (g, m) owns features 4g..4g+3 of row m; thread = (samples b = lane + 64 rr for rr < R, feature jj = wave)
template <int R>
__global__ __launch_bounds__(256) void head3_fc_kernel(const float* x, Sets3 ps, float* h, int B) {
    constexpr int NB = 64 * R;                  // sample capacity of this instantiation
    __shared__ float xT[64][NB + 1];            // one 64-column chunk of x[m], transposed: xT[k][b]
    const int tid = threadIdx.x, lane = tid & 63, jj = __builtin_amdgcn_readfirstlane(tid >> 6), j = blockIdx.x * FPW + jj;
    const int m = blockIdx.y;
    const HeadSet p = ps.s[m];
    const float* xm = x + (size_t)m * B * DX;
    const float* wrow = p.w1 + (size_t)j * DX;
    float acc[R];           // the tile product: inline here and in head_fc_kernel, not a block (head_common.hip.h says why)
#pragma unroll
    for (int rr = 0; rr < R; ++rr) acc[rr] = 0.f;
    for (int k0 = 0; k0 < DX; k0 += 64) {
        __syncthreads();
        // NB samples x 64 columns: thread t loads samples (t>>2) + 64 rr, columns 16*(t&3) .. +15
        const int cs = 16 * (tid & 3);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int r = (tid >> 2) + 64 * rr;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (r < B) v = *reinterpret_cast<const f32x4*>(xm + (size_t)r * DX + k0 + cs + 4 * q);
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
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int b = lane + 64 * rr;
        if (b < B) h[((size_t)m * B + b) * D + j] = acc[rr] + p.b1[j];
    }
}

// one wave per row (m, b): hhat = LN(h) written in place of h, rstd kept, o = ReLU(hhat g + be) . w2 + b2
__global__ __launch_bounds__(256) void head3_out_kernel(float* h, float* rstd_out, Sets3 ps, float* out, int B, float eps) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= 3 * B) return;
    const HeadSet p = ps.s[r / B];
    const int c = 4 * lane;
    float* row = h + (size_t)r * D + c;
    const f32x4 v = *reinterpret_cast<const f32x4*>(row);
    float d[4];
    const float rstd = wave_ln4(v, v[0] + v[1] + v[2] + v[3], eps, d);
    f32x4 hh;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hh[i] = d[i] * rstd;
        s = fmaf(fmaxf(fmaf(hh[i], p.g[c + i], p.be[c + i]), 0.f), p.w2[c + i], s);
    }
    *reinterpret_cast<f32x4*>(row) = hh;
    s = wave_sum(s);
    if (lane == 0) { out[r] = s + p.b2[0]; rstd_out[r] = rstd; }
}

// one wave per row (m, b): dh = LayerNorm backward of dy = [hhat g + be > 0] * do[m,b] * w2
__global__ __launch_bounds__(256) void head3_row_bwd_kernel(const float* d_o, const float* hhat, const float* rstd_in, Sets3 ps,
                                                            float* dh, int B) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= 3 * B) return;
    const HeadSet p = ps.s[r / B];
    const int c = 4 * lane;
    const f32x4 hh = *reinterpret_cast<const f32x4*>(hhat + (size_t)r * D + c);
    const float dl = d_o[r], rstd = rstd_in[r];
    float gy[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float gam = p.g[c + i];
        const float dy = fmaf(hh[i], gam, p.be[c + i]) > 0.f ? dl * p.w2[c + i] : 0.f;
        gy[i] = dy * gam;
        s1 += gy[i];
        s2 = fmaf(gy[i], hh[i], s2);
    }
    const float m1 = wave_sum(s1) * (1.0f / D), m2 = wave_sum(s2) * (1.0f / D);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = rstd * (gy[i] - m1 - hh[i] * m2);
    *reinterpret_cast<f32x4*>(dh + (size_t)r * D + c) = o;
}

// feature-parallel backward: workgroup (g, s) owns features 4g..4g+3 of parameter set s and walks the `cnt` rows m0 .. m0+cnt-1 that
// use it (one row per set, or the three rows of a shared set): every row's sums are finished on their own and then added in the
// order m = 0, 1, 2, so a shared set's gradient is bit for bit (g_0 + g_1) + g_2 of three separate sets with equal weights.
template <int R>
__global__ __launch_bounds__(256) void head3_fc_bwd_kernel(const float* d_o, const float* x, const float* hhat, const float* dh,
                                                           Sets3 ps, Grads3 gs, int B, int cnt) {
    constexpr int NB = 64 * R;
    __shared__ float dhs[FPW][NB];
    const int tid = threadIdx.x, lane = tid & 63, jj = __builtin_amdgcn_readfirstlane(tid >> 6), j = blockIdx.x * FPW + jj;
    const int m0 = blockIdx.y;                                         // (cnt == 3: gridDim.y == 1, m0 == 0)
    const HeadSet p = ps.s[m0];
    const SetGrads gr = gs.s[m0];
    const float gam = p.g[j], bet = p.be[j], w2j = p.w2[j];
    float a_w2 = 0.f, a_g = 0.f, a_b = 0.f, a_b1 = 0.f, a_dl = 0.f;
    float t0[FPW] = {0.f, 0.f, 0.f, 0.f}, t1[FPW] = {0.f, 0.f, 0.f, 0.f};
    for (int m = m0; m < m0 + cnt; ++m) {
        float t_w2 = 0.f, t_g = 0.f, t_b = 0.f, t_b1 = 0.f, t_dl = 0.f;
        __syncthreads();                                               // the previous row's dW1 loop is done with dhs
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int b = lane + 64 * rr;
            const bool live = b < B;
            const size_t row = (size_t)m * B + (live ? b : 0);
            const float dl = live ? d_o[row] : 0.f;
            const float hh = live ? hhat[row * D + j] : 0.f;
            const float dhv = live ? dh[row * D + j] : 0.f;
            const float y = fmaf(hh, gam, bet);
            const float dy = (live && y > 0.f) ? dl * w2j : 0.f;
            t_w2 = fmaf(dl, fmaxf(y, 0.f), t_w2);
            t_g = fmaf(dy, hh, t_g);
            t_b += dy; t_b1 += dhv; t_dl += dl;
            dhs[jj][b] = dhv;
        }
        a_w2 += wave_sum(t_w2); a_g += wave_sum(t_g); a_b += wave_sum(t_b); a_b1 += wave_sum(t_b1); a_dl += wave_sum(t_dl);
        __syncthreads();
        float s0[FPW], s1[FPW];
        dw1_rows(dhs, x + (size_t)m * B * DX, B, s0, s1);     // this row's dW1, finished on its own
#pragma unroll
        for (int f = 0; f < FPW; ++f) { t0[f] += s0[f]; t1[f] += s1[f]; }
    }
    if (lane == 0) { gr.w2[j] = a_w2; gr.g[j] = a_g; gr.be[j] = a_b; gr.b1[j] = a_b1; }
    if (blockIdx.x == 0 && tid == 0) gr.b2[0] = a_dl;
#pragma unroll
    for (int f = 0; f < FPW; ++f) {
        gr.w1[(size_t)(blockIdx.x * FPW + f) * DX + tid] = t0[f];
        gr.w1[(size_t)(blockIdx.x * FPW + f) * DX + D + tid] = t1[f];
    }
}

// sample-parallel backward: workgroup = sample b, thread = column k of each half of x; the three rows one after the other.
// Slab row b: demo_row_bwd, with ddemo_w interleaved.
template <typename TC>
__global__ __launch_bounds__(256) void head3_x_bwd_kernel(const float* dh, Cls3<TC> cls, const float* age, const float* gen,
                                                          Shared3 p, Sets3 ps, DCls3<TC> dcls, float* slab, int B, float eps) {
    __shared__ float dhr[D];
    __shared__ float red[4];
    const int b = blockIdx.x, k = threadIdx.x;
    float dxd = 0.f, s_g = 0.f, s_b = 0.f;
    const float lng = p.ln_g[k];
    for (int m = 0; m < 3; ++m) {
        __syncthreads();
        dhr[k] = dh[((size_t)m * B + b) * D + k];
        __syncthreads();
        float dxc, dd;
        dx_row(dhr, ps.s[m].w1, k, dxc, dd);
        dxd += dd;
        // LayerNorm(cls_m) backward: inline here and in head_x_bwd_kernel, not a block (head_common.hip.h says why)
        const float v = to_f32(cls.p[m][(size_t)b * cls.ld[m] + k]);
        const float mean = block_sum(v, red, k) * (1.0f / D);
        const float d = v - mean;
        const float rstd = rsqrtf(block_sum(d * d, red, k) * (1.0f / D) + eps);
        const float xh = d * rstd, gy = dxc * lng;
        const float m1 = block_sum(gy, red, k) * (1.0f / D), m2 = block_sum(gy * xh, red, k) * (1.0f / D);
        dcls.p[m][(size_t)b * D + k] = from_f32<TC>(rstd * (gy - m1 - xh * m2));
        s_g += dxc * xh;
        s_b += dxc;
    }
    float* row = slab + (size_t)b * 7 * D;
    row[k] = s_g;
    row[D + k] = s_b;
    demo_row_bwd<true>(age[b], gen[b], p, dxd, eps, red, k, row);
}

// modalities present under pattern id c (trainer.py:68-77: 0 = all, 1 = report missing, 2 = image missing, 3 = both missing):
// row 0 always, row 1 iff c < 2, row 2 iff c is even.  Any id is reduced with & 3 first: nothing is indexed by it.
MTMP_DEV void present(long long id, bool& img, bool& txt) {
    const int c = (int)(id & 3);
    img = c < 2;
    txt = (c & 1) == 0;
}

// out[b] = mean of o[m][b] over the present rows (tri_mbt_v1.py:272-281, trainer.py:224-229)
__global__ __launch_bounds__(256) void cand_mean_kernel(const float* o, const long long* mnum, float* out, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    bool img, txt;
    present(mnum[b], img, txt);
    const float o0 = o[b], o1 = o[B + b], o2 = o[2 * (size_t)B + b];
    out[b] = img ? (txt ? ((o0 + o1) + o2) / 3.0f : (o0 + o1) / 2.0f) : (txt ? (o0 + o2) / 2.0f : o0);
}
__global__ __launch_bounds__(256) void cand_mean_bwd_kernel(const float* d_out, const long long* mnum, float* d_o, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    bool img, txt;
    present(mnum[b], img, txt);
    const float g = d_out[b] / (float)(1 + (int)img + (int)txt);
    d_o[b] = g;
    d_o[B + b] = img ? g : 0.f;
    d_o[2 * (size_t)B + b] = txt ? g : 0.f;
}

// loss = (1/n) sum over the present (m, b) of [max(o,0) - o y + log(1 + exp(-|o|))], n = their number, counted here;
// dlogit[m][b] = (sigmoid(o) - y) / n on the present pairs, 0 elsewhere.  One workgroup.
__global__ __launch_bounds__(256) void bce_masked_kernel(const float* o, const float* y, const long long* mnum, float* loss,
                                                         float* dlogit, int B) {
    __shared__ float red[4];
    float cnt = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        bool img, txt;
        present(mnum[b], img, txt);
        cnt += (float)(1 + (int)img + (int)txt);
    }
    const float n = block_sum(cnt, red, threadIdx.x);          // (small integers: exact in any order)
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        bool on[3] = {true, false, false};
        present(mnum[b], on[1], on[2]);
        const float t = y[b];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const size_t i = (size_t)m * B + b;
            const float v = o[i];
            s += on[m] ? fmaxf(v, 0.f) - v * t + log1pf(expf(-fabsf(v))) : 0.f;
            dlogit[i] = on[m] ? (1.0f / (1.0f + expf(-v)) - t) / n : 0.f;
        }
    }
    s = block_sum(s, red, threadIdx.x);
    if (threadIdx.x == 0) loss[0] = s / n;
}

// The same over R <= 4 logit rows with a trained-rows table: bit 4 * pattern + row of `table` set = row `row` is trained on a
// sample whose pattern id is `pattern` (the multi-token models: trainer.py:79-83, missing_multitoken == 0).  loss = the mean over
// the selected (row, sample) pairs, counted here; dlogit = (sigmoid(o) - y) / n on them, 0 elsewhere.  One workgroup.
__global__ __launch_bounds__(256) void bce_rows_masked_kernel(const float* o, const float* y, const long long* mnum, unsigned table,
                                                              float* loss, float* dlogit, int R, int B) {
    __shared__ float red[4];
    const unsigned rows_all = (1u << R) - 1u;
    float cnt = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) cnt += (float)__popc((table >> (4 * (int)(mnum[b] & 3))) & rows_all);
    const float n = block_sum(cnt, red, threadIdx.x);          // (small integers: exact in any order)
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const unsigned on = (table >> (4 * (int)(mnum[b] & 3))) & rows_all;
        const float t = y[b];
        for (int m = 0; m < R; ++m) {
            const size_t i = (size_t)m * B + b;
            const float v = o[i];
            const bool sel = (on >> m) & 1u;
            s += sel ? fmaxf(v, 0.f) - v * t + log1pf(expf(-fabsf(v))) : 0.f;
            dlogit[i] = sel ? (1.0f / (1.0f + expf(-v)) - t) / n : 0.f;
        }
    }
    s = block_sum(s, red, threadIdx.x);
    if (threadIdx.x == 0) loss[0] = s / n;
}

inline Sets3 sets_of(const void* const* q, int n_sets) {
    Sets3 s;
    for (int m = 0; m < 3; ++m) {
        const void* const* r = q + 6 + (n_sets == 3 ? 6 * m : 0);
        s.s[m] = HeadSet{(const float*)r[0], (const float*)r[1], (const float*)r[2], (const float*)r[3], (const float*)r[4], (const float*)r[5]};
    }
    return s;
}

}  // namespace

// ws_fwd: x[3][B][512] + hhat[3][B][256] + rstd[3][B] floats (kept for the backward)
extern "C" int mtmp_head3_ws_floats(int B) { return 3 * B * (DX + D + 1); }
// ws_bwd: dh[3][B][256] + slab[B][7 x 256] floats
extern "C" int mtmp_head3_bwd_ws_floats(int B) { return 3 * B * D + B * 7 * D; }

extern "C" int mtmp_head3_fwd(int cls_dtype, const void* const* cls, const long long* cls_ld, const float* age, const float* gender,
                              const void* const* params, int n_sets, float* out, float* ws, int B, float ln_eps, void* stream) {
    MTMP_CHECK_ARG(cls && cls_ld && age && gender && params && out && ws && B > 0 && B <= MAXB && (n_sets == 1 || n_sets == 3) &&
                       (cls_dtype == 0 || cls_dtype == 1),
                   "mtmp_head3_fwd: bad argument (B=%d, needs 1 <= B <= %d; n_sets %d is 1 or 3; dtype %d)", B, MAXB, n_sets, cls_dtype);
    for (int m = 0; m < 3; ++m)
        MTMP_CHECK_ARG(cls[m] && cls_ld[m] >= D && cls_ld[m] % 4 == 0 && ((uintptr_t)cls[m] & 15) == 0,
                       "mtmp_head3_fwd: CLS rows %d need a 16-byte aligned base and a row stride >= 256 that is a multiple of 4", m);
    for (int i = 0; i < 6 + 6 * n_sets; ++i) MTMP_CHECK_ARG(params[i], "mtmp_head3_fwd: parameter %d is NULL", i);
    const Shared3 p = shared_of(params);
    const Sets3 ps = sets_of(params, n_sets);
    hipStream_t st = (hipStream_t)stream;
    float* x = ws; float* hh = x + (size_t)3 * B * DX; float* rstd = hh + (size_t)3 * B * D;
    if (cls_dtype == 0) {
        Cls3<float> c{{(const float*)cls[0], (const float*)cls[1], (const float*)cls[2]}, {cls_ld[0], cls_ld[1], cls_ld[2]}};
        hipLaunchKernelGGL(head3_x_kernel<float>, dim3(B), dim3(256), 0, st, c, age, gender, p, x, B, ln_eps);
    } else {
        Cls3<bf16> c{{(const bf16*)cls[0], (const bf16*)cls[1], (const bf16*)cls[2]}, {cls_ld[0], cls_ld[1], cls_ld[2]}};
        hipLaunchKernelGGL(head3_x_kernel<bf16>, dim3(B), dim3(256), 0, st, c, age, gender, p, x, B, ln_eps);
    }
    MTMP_CHECK_LAUNCH("mtmp_head3_fwd(x)");
    const int R = rows_per_lane(B);
    auto fc = R == 1 ? head3_fc_kernel<1> : (R == 2 ? head3_fc_kernel<2> : head3_fc_kernel<4>);
    hipLaunchKernelGGL(fc, dim3(D / FPW, 3), dim3(256), 0, st, (const float*)x, ps, hh, B);
    MTMP_CHECK_LAUNCH("mtmp_head3_fwd(fc)");
    hipLaunchKernelGGL(head3_out_kernel, dim3((3 * B + 3) / 4), dim3(256), 0, st, hh, rstd, ps, out, B, ln_eps);
    MTMP_CHECK_LAUNCH("mtmp_head3_fwd(out)");
    return MTMP_OK;
}

extern "C" int mtmp_head3_bwd(int cls_dtype, const float* d_out, const void* const* cls, const long long* cls_ld, const float* age,
                              const float* gender, const void* const* params, int n_sets, const float* ws_fwd, void* const* dcls,
                              float* const* dst, float* ws_bwd, int B, float ln_eps, void* stream) {
    MTMP_CHECK_ARG(d_out && cls && cls_ld && age && gender && params && ws_fwd && dcls && dst && ws_bwd && B > 0 && B <= MAXB &&
                       (n_sets == 1 || n_sets == 3) && (cls_dtype == 0 || cls_dtype == 1),
                   "mtmp_head3_bwd: bad argument (B=%d n_sets %d dtype %d)", B, n_sets, cls_dtype);
    for (int m = 0; m < 3; ++m)
        MTMP_CHECK_ARG(cls[m] && dcls[m] && cls_ld[m] >= D, "mtmp_head3_bwd: CLS rows %d: NULL or row stride < 256", m);
    for (int i = 0; i < 6 + 6 * n_sets; ++i) MTMP_CHECK_ARG(params[i] && dst[i], "mtmp_head3_bwd: parameter / destination %d is NULL", i);
    const Shared3 p = shared_of(params);
    const Sets3 ps = sets_of(params, n_sets);
    Grads3 gs;
    for (int m = 0; m < 3; ++m) {
        float* const* r = dst + 6 + (n_sets == 3 ? 6 * m : 0);
        gs.s[m] = SetGrads{r[0], r[1], r[2], r[3], r[4], r[5]};
    }
    hipStream_t st = (hipStream_t)stream;
    const float* x = ws_fwd; const float* hh = x + (size_t)3 * B * DX; const float* rstd = hh + (size_t)3 * B * D;
    float* dh = ws_bwd; float* slab = dh + (size_t)3 * B * D;
    hipLaunchKernelGGL(head3_row_bwd_kernel, dim3((3 * B + 3) / 4), dim3(256), 0, st, d_out, hh, rstd, ps, dh, B);
    MTMP_CHECK_LAUNCH("mtmp_head3_bwd(row)");
    const int R = rows_per_lane(B);
    auto fcb = R == 1 ? head3_fc_bwd_kernel<1> : (R == 2 ? head3_fc_bwd_kernel<2> : head3_fc_bwd_kernel<4>);
    hipLaunchKernelGGL(fcb, dim3(D / FPW, n_sets), dim3(256), 0, st, d_out, x, hh, (const float*)dh, ps, gs, B, n_sets == 3 ? 1 : 3);
    MTMP_CHECK_LAUNCH("mtmp_head3_bwd(fc)");
    if (cls_dtype == 0) {
        Cls3<float> c{{(const float*)cls[0], (const float*)cls[1], (const float*)cls[2]}, {cls_ld[0], cls_ld[1], cls_ld[2]}};
        DCls3<float> dc{{(float*)dcls[0], (float*)dcls[1], (float*)dcls[2]}};
        hipLaunchKernelGGL(head3_x_bwd_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)dh, c, age, gender, p, ps, dc, slab, B, ln_eps);
    } else {
        Cls3<bf16> c{{(const bf16*)cls[0], (const bf16*)cls[1], (const bf16*)cls[2]}, {cls_ld[0], cls_ld[1], cls_ld[2]}};
        DCls3<bf16> dc{{(bf16*)dcls[0], (bf16*)dcls[1], (bf16*)dcls[2]}};
        hipLaunchKernelGGL(head3_x_bwd_kernel<bf16>, dim3(B), dim3(256), 0, st, (const float*)dh, c, age, gender, p, ps, dc, slab, B, ln_eps);
    }
    MTMP_CHECK_LAUNCH("mtmp_head3_bwd(x)");
    launch_rows_scatter(slab, B, dst, st);
    MTMP_CHECK_LAUNCH("mtmp_head3_bwd(scatter)");
    return MTMP_OK;
}

extern "C" int mtmp_candidate_mean_fwd(const float* o, const long long* missing_num, float* out, int B, void* stream) {
    MTMP_CHECK_ARG(o && missing_num && out && B > 0, "mtmp_candidate_mean_fwd: bad argument (B=%d)", B);
    hipLaunchKernelGGL(cand_mean_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, o, missing_num, out, B);
    MTMP_CHECK_LAUNCH("mtmp_candidate_mean_fwd");
    return MTMP_OK;
}

extern "C" int mtmp_candidate_mean_bwd(const float* d_out, const long long* missing_num, float* d_o, int B, void* stream) {
    MTMP_CHECK_ARG(d_out && missing_num && d_o && B > 0, "mtmp_candidate_mean_bwd: bad argument (B=%d)", B);
    hipLaunchKernelGGL(cand_mean_bwd_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_out, missing_num, d_o, B);
    MTMP_CHECK_LAUNCH("mtmp_candidate_mean_bwd");
    return MTMP_OK;
}

extern "C" int mtmp_bce_masked_mean(const float* logits, const float* target, const long long* missing_num, float* loss,
                                    float* dlogit, int B, void* stream) {
    MTMP_CHECK_ARG(logits && target && missing_num && loss && dlogit && B > 0, "mtmp_bce_masked_mean: bad argument (B=%d)", B);
    hipLaunchKernelGGL(bce_masked_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, target, missing_num, loss, dlogit, B);
    MTMP_CHECK_LAUNCH("mtmp_bce_masked_mean");
    return MTMP_OK;
}

// loss[0] = mean over the trained (row, sample) pairs of BCE-with-logits(logits[row][b], target[b]), dlogit [R, B] = its gradient
// (0 on the other pairs).  logits / dlogit fp32 [R, B], R <= 4; missing_num int64[B]; table: bit 4 * pattern + row = row trained
// under that pattern id (ids are taken & 3).
extern "C" int mtmp_bce_rows_masked_mean(const float* logits, const float* target, const long long* missing_num, unsigned table,
                                         float* loss, float* dlogit, int R, int B, void* stream) {
    MTMP_CHECK_ARG(logits && target && missing_num && loss && dlogit && B > 0 && R >= 1 && R <= 4,
                   "mtmp_bce_rows_masked_mean: bad argument (R=%d B=%d)", R, B);
    MTMP_CHECK_ARG(table <= 0xFFFFu, "mtmp_bce_rows_masked_mean: table has bits outside 4 patterns x 4 rows (%#x)", table);
    hipLaunchKernelGGL(bce_rows_masked_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, target, missing_num, table, loss,
                       dlogit, R, B);
    MTMP_CHECK_LAUNCH("mtmp_bce_rows_masked_mean");
    return MTMP_OK;
}
