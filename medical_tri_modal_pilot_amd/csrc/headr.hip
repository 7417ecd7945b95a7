// R-row LayerNorm head (1 <= R <= 4) of the flexible and multi-token models for gfx950 -- head3.hip's math:
//     demo[b]  = ReLU(LN(age[b] * w[:,0] + gender[b] * w[:,1] + b))               ie_demo, shared by the rows
//     v[m,b]   = the fp32 mean ((a + b) + c) / n of head row m's n = 1, 2 or 3 source rows
//     x[m,b]   = [ LN(v[m,b]) | demo[b] ]                                         layer_norms_after_concat, torch.cat (512 wide)
//     h        = x[m,b] W1_m^T + b1_m ;  a = ReLU(LN(h; g_m, be_m)) ;  o[m,b] = a . w2_m + b2_m
// with one parameter set per row, or ONE set shared by the R rows (gradients summed in the fixed order m = 0 .. R-1).
// Inputs are BLOCKS, not rows: up to three strided views [B, P_s, 256] (P_s <= 4; base, sample stride, row stride), and a source
// table names the (block, row) pairs every head row reads:
//     tri_mbt_vflexible*, bi*_mbt_vflexible1   outputs[m][:, 0, :]: R blocks with P = 1, head row m = block m
//     tri_mbt_vmultivslt                       outputs[0][:, :4, :]: one block with P = 4, head row i = row i
//     tri_mbt_vmulti2                          (v0 i0 t0) / 3, (v1 i1) / 2, (v2 t1) / 2, v3 of three blocks (tri_mbt_vmulti2.py:161-165)
// A (block, row) pair feeds at most one head row, so the backward writes every row of every gradient block exactly once: a source
// row d(head row) / n, any other row zeros.  The launch structure is head3.hip's: three launches forward, four backward.  fp32
// throughout, no float atomics.  The shared pieces are the blocks of head_common.hip.h; the 512 -> 256 tile product and the
// LayerNorm backward stand inline here as in head3.hip (head_common.hip.h says why).
// Also here: the flexible models' learned weighting of the logits over the present modalities (mtmp_flex_combine_*).
#include "head_common.hip.h"

namespace {

constexpr int MAXR = 4, MAXBLK = 3, MAXP = 4, MAXSRC = 3;

struct HeadSet {      // Linear(512,256), LayerNorm(256), Linear(256,1) of one row
    const float* w1; const float* b1; const float* g; const float* be; const float* w2; const float* b2;
};
struct SetsR { HeadSet s[MAXR]; };
struct SetGrads { float* w1; float* b1; float* g; float* be; float* w2; float* b2; };
struct GradsR { SetGrads s[MAXR]; };
// block s: p[s] + b * sb[s] + row * sr[s], 256 contiguous values
// (four slots: a two-bit block number read out of the source table always names one; slot 3 is never named by a checked table)
template <typename TC> struct Blocks { const TC* p[4]; long long sb[4]; long long sr[4]; };
// gradient blocks [B][rows[s]][256] contiguous; `sources`: bit 4 s + row set = that row feeds a head row
template <typename TC> struct DBlocks { TC* p[MAXBLK]; int rows[MAXBLK]; unsigned sources; };

// The source table in one word, 16 bits per head row: n in bits 0-1, source i's block in bits 2 + 4 i .. 3 + 4 i and its row in
// bits 4 + 4 i .. 5 + 4 i.  The host checks every entry (plan_rows); the kernels index nothing by it but the four block slots.
MTMP_DEV unsigned row_code(unsigned long long tab, int m) { return (unsigned)(tab >> (16 * m)) & 0xFFFFu; }
template <typename TC> MTMP_DEV const TC* src_ptr(const Blocks<TC>& bl, unsigned code, int i, int b) {
    const int s = (code >> (2 + 4 * i)) & 3, r = (code >> (4 + 4 * i)) & 3;
    return bl.p[s] + (size_t)b * bl.sb[s] + (size_t)r * bl.sr[s];
}

// rows 0 .. RB-1: x[m][b][0:256] = LN(v[m][b]); rows RB .. RB+B-1: demo[b] -> x[0..R-1][b][256:512].  One wave per row.
template <typename TC>
__global__ __launch_bounds__(256) void headr_x_kernel(Blocks<TC> bl, unsigned long long tab, const float* age, const float* gen,
                                                      Shared3 p, float* x, int R, int B, float eps) {
    // (r is the same in every lane of a wave; said so, the source table's selections stay in scalar registers)
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= (R + 1) * B) return;
    const int c = 4 * lane;
    if (r < R * B) {
        const int m = r / B, b = r - m * B;
        const unsigned code = row_code(tab, m);
        const int n = code & 3;
        f32x4 o;
        if (n == 1) {
            o = cls_row_fwd(src_ptr(bl, code, 0, b), p, c, eps);
        } else {
            f32x4 v = load4<TC>(src_ptr(bl, code, 0, b) + c);
            const f32x4 v1 = load4<TC>(src_ptr(bl, code, 1, b) + c);
            f32x4 v2 = {0.f, 0.f, 0.f, 0.f};
            if (n == 3) v2 = load4<TC>(src_ptr(bl, code, 2, b) + c);
            const float fn = (float)n;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = n == 3 ? ((v[i] + v1[i]) + v2[i]) / fn : (v[i] + v1[i]) / fn;
            float d[4];
            const float rstd = wave_ln4(v, v[0] + v[1] + v[2] + v[3], eps, d);
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = fmaf(d[i] * rstd, p.ln_g[c + i], p.ln_b[c + i]);
        }
        *reinterpret_cast<f32x4*>(x + ((size_t)m * B + b) * DX + c) = o;
    } else {
        const int b = r - R * B;
        const f32x4 o = demo_row_fwd(age[b], gen[b], p, c, eps);
        for (int m = 0; m < R; ++m) *reinterpret_cast<f32x4*>(x + ((size_t)m * B + b) * DX + D + c) = o;
    }
}

// workgroup (g, m) owns features 4g..4g+3 of row m; thread = (samples b = lane + 64 rr for rr < RPL, feature jj = wave)
template <int RPL>
__global__ __launch_bounds__(256) void headr_fc_kernel(const float* x, SetsR ps, float* h, int B) {
    constexpr int NB = 64 * RPL;                // sample capacity of this instantiation
    __shared__ float xT[64][NB + 1];            // one 64-column chunk of x[m], transposed: xT[k][b]
    const int tid = threadIdx.x, lane = tid & 63, jj = __builtin_amdgcn_readfirstlane(tid >> 6), j = blockIdx.x * FPW + jj;
    const int m = blockIdx.y;
    const HeadSet p = ps.s[m];
    const float* xm = x + (size_t)m * B * DX;
    const float* wrow = p.w1 + (size_t)j * DX;
    float acc[RPL];         // the tile product: inline here, in head_fc_kernel and in head3_fc_kernel (head_common.hip.h says why)
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) acc[rr] = 0.f;
    for (int k0 = 0; k0 < DX; k0 += 64) {
        __syncthreads();
        // NB samples x 64 columns: thread t loads samples (t>>2) + 64 rr, columns 16*(t&3) .. +15
        const int cs = 16 * (tid & 3);
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
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
            for (int rr = 0; rr < RPL; ++rr) acc[rr] = fmaf(xT[kk][lane + 64 * rr], wv, acc[rr]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < RPL; ++rr) {
        const int b = lane + 64 * rr;
        if (b < B) h[((size_t)m * B + b) * D + j] = acc[rr] + p.b1[j];
    }
}

// one wave per row (m, b): hhat = LN(h) written in place of h, rstd kept, o = ReLU(hhat g + be) . w2 + b2
__global__ __launch_bounds__(256) void headr_out_kernel(float* h, float* rstd_out, SetsR ps, float* out, int R, int B, float eps) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R * B) return;
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
__global__ __launch_bounds__(256) void headr_row_bwd_kernel(const float* d_o, const float* hhat, const float* rstd_in, SetsR ps,
                                                            float* dh, int R, int B) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R * B) return;
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
// use it (one row per set, or the R rows of a shared set): every row's sums are finished on their own and then added in the
// order m = 0 .. R-1, so a shared set's gradient is bit for bit ((g_0 + g_1) + g_2) + g_3 of separate sets with equal weights.
template <int RPL>
__global__ __launch_bounds__(256) void headr_fc_bwd_kernel(const float* d_o, const float* x, const float* hhat, const float* dh,
                                                           SetsR ps, GradsR gs, int B, int cnt) {
    constexpr int NB = 64 * RPL;
    __shared__ float dhs[FPW][NB];
    const int tid = threadIdx.x, lane = tid & 63, jj = __builtin_amdgcn_readfirstlane(tid >> 6), j = blockIdx.x * FPW + jj;
    const int m0 = blockIdx.y;                                         // (a shared set: gridDim.y == 1, m0 == 0)
    const HeadSet p = ps.s[m0];
    const SetGrads gr = gs.s[m0];
    const float gam = p.g[j], bet = p.be[j], w2j = p.w2[j];
    float a_w2 = 0.f, a_g = 0.f, a_b = 0.f, a_b1 = 0.f, a_dl = 0.f;
    float t0[FPW] = {0.f, 0.f, 0.f, 0.f}, t1[FPW] = {0.f, 0.f, 0.f, 0.f};
    for (int m = m0; m < m0 + cnt; ++m) {
        float t_w2 = 0.f, t_g = 0.f, t_b = 0.f, t_b1 = 0.f, t_dl = 0.f;
        __syncthreads();                                               // the previous row's dW1 loop is done with dhs
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
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

// sample-parallel backward: workgroup = sample b, thread = column k of each half of x; the R rows one after the other.
// d v[m] / n goes to each of row m's sources, zeros to the rows of the gradient blocks that are no source.
// Slab row b: demo_row_bwd, with ddemo_w interleaved.
template <typename TC>
__global__ __launch_bounds__(256) void headr_x_bwd_kernel(const float* dh, Blocks<TC> bl, unsigned long long tab, const float* age,
                                                          const float* gen, Shared3 p, SetsR ps, DBlocks<TC> dbl, float* slab, int R,
                                                          int B, float eps) {
    __shared__ float dhr[D];
    __shared__ float red[4];
    const int b = blockIdx.x, k = threadIdx.x;
    float dxd = 0.f, s_g = 0.f, s_b = 0.f;
    const float lng = p.ln_g[k];
    for (int m = 0; m < R; ++m) {
        __syncthreads();
        dhr[k] = dh[((size_t)m * B + b) * D + k];
        __syncthreads();
        float dxc, dd;
        dx_row(dhr, ps.s[m].w1, k, dxc, dd);
        dxd += dd;
        const unsigned code = row_code(tab, m);
        const int n = code & 3;
        float v = to_f32(src_ptr(bl, code, 0, b)[k]);
        if (n > 1) {
            v += to_f32(src_ptr(bl, code, 1, b)[k]);
            if (n > 2) v += to_f32(src_ptr(bl, code, 2, b)[k]);
            v = v / (float)n;
        }
        // LayerNorm(v) backward: inline here, in head_x_bwd_kernel and in head3_x_bwd_kernel (head_common.hip.h says why)
        const float mean = block_sum(v, red, k) * (1.0f / D);
        const float d = v - mean;
        const float rstd = rsqrtf(block_sum(d * d, red, k) * (1.0f / D) + eps);
        const float xh = d * rstd, gy = dxc * lng;
        const float m1 = block_sum(gy, red, k) * (1.0f / D), m2 = block_sum(gy * xh, red, k) * (1.0f / D);
        float dv = rstd * (gy - m1 - xh * m2);
        if (n > 1) dv = dv / (float)n;
        for (int i = 0; i < n; ++i) {
            const int s = (code >> (2 + 4 * i)) & 3, r = (code >> (4 + 4 * i)) & 3;
            TC* dp = s == 0 ? dbl.p[0] : (s == 1 ? dbl.p[1] : dbl.p[2]);
            const int rows = s == 0 ? dbl.rows[0] : (s == 1 ? dbl.rows[1] : dbl.rows[2]);
            dp[((size_t)b * rows + r) * D + k] = from_f32<TC>(dv);
        }
        s_g += dxc * xh;
        s_b += dxc;
    }
#pragma unroll
    for (int s = 0; s < MAXBLK; ++s)
        for (int r = 0; r < dbl.rows[s]; ++r)
            if (!((dbl.sources >> (4 * s + r)) & 1u)) dbl.p[s][((size_t)b * dbl.rows[s] + r) * D + k] = from_f32<TC>(0.f);
    float* row = slab + (size_t)b * 7 * D;
    row[k] = s_g;
    row[D + k] = s_b;
    demo_row_bwd<true>(age[b], gen[b], p, dxd, eps, red, k, row);
}

// ---- the flexible combine (tri_mbt_vflexible.py:276-286): p[m][b] = softmax over the present rows of T a[m], 0 on absent rows
struct Flex { float p[MAXR]; float out; };
MTMP_DEV Flex flex_row(const float* o, const float* a, float T, unsigned on, int R, int B, int b) {
    Flex f;
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < MAXR; ++m) {
        const bool sel = m < R && ((on >> m) & 1u);
        f.p[m] = sel ? T * a[m] : 0.f;
        mx = sel ? fmaxf(mx, f.p[m]) : mx;
    }
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < MAXR; ++m) {
        const bool sel = m < R && ((on >> m) & 1u);
        f.p[m] = sel ? expf(f.p[m] - mx) : 0.f;
        sum += f.p[m];
    }
    f.out = 0.f;
#pragma unroll
    for (int m = 0; m < MAXR; ++m) {
        const bool sel = m < R && ((on >> m) & 1u);
        f.p[m] = sel ? f.p[m] / sum : 0.f;
        f.out += sel ? f.p[m] * o[(size_t)m * B + b] : 0.f;
    }
    return f;
}

__global__ __launch_bounds__(256) void flex_combine_kernel(const float* o, const float* a, float T, const long long* mnum,
                                                           unsigned table, float* out, int R, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const unsigned on = (table >> (4 * (int)(mnum[b] & 3))) & ((1u << R) - 1u);
    out[b] = flex_row(o, a, T, on, R, B, b).out;
}

// d_o[m][b] = p g, d_a[m] = T sum_b p g (o[m][b] - out[b]): one workgroup, thread t sums its samples b = t, t + 256, .. in that
// order, then the 256 partial sums are combined by block_sum -- a fixed order for any B
__global__ __launch_bounds__(256) void flex_combine_bwd_kernel(const float* g, const float* o, const float* a, float T,
                                                               const long long* mnum, unsigned table, float* d_o, float* d_a,
                                                               int R, int B) {
    __shared__ float red[4];
    float acc[MAXR] = {0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < B; b += 256) {
        const unsigned on = (table >> (4 * (int)(mnum[b] & 3))) & ((1u << R) - 1u);
        const Flex f = flex_row(o, a, T, on, R, B, b);
        const float gb = g[b];
        float ov[MAXR];
#pragma unroll
        for (int m = 0; m < MAXR; ++m) ov[m] = (m < R && ((on >> m) & 1u)) ? o[(size_t)m * B + b] : 0.f;
#pragma unroll
        for (int m = 0; m < MAXR; ++m) {
            if (m < R) {
                const bool sel = (on >> m) & 1u;
                const float pg = sel ? f.p[m] * gb : 0.f;
                d_o[(size_t)m * B + b] = pg;
                // o[m] - out as sum_j p[j] (o[m] - o[j]): where one weight is close to 1, o[m] - out cancels to the rounding
                // of out; the differences of the logits themselves do not
                float diff = 0.f;
#pragma unroll
                for (int j = 0; j < MAXR; ++j) diff += (j != m) ? f.p[j] * (ov[m] - ov[j]) : 0.f;      // (p[j] = 0 on absent rows)
                acc[m] += sel ? pg * diff : 0.f;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MAXR; ++m) {
        const float s = block_sum(acc[m], red, threadIdx.x);
        if (m < R && threadIdx.x == 0) d_a[m] = T * s;
    }
}

inline SetsR sets_of(const void* const* q, int n_sets, int R) {
    SetsR s;
    for (int m = 0; m < MAXR; ++m) {
        const void* const* r = q + 6 + (n_sets == 1 ? 0 : 6 * (m < R ? m : 0));
        s.s[m] = HeadSet{(const float*)r[0], (const float*)r[1], (const float*)r[2], (const float*)r[3], (const float*)r[4], (const float*)r[5]};
    }
    return s;
}

// The checked description of a call's blocks and sources.
struct RowPlan {
    const void* p[MAXBLK]; long long sb[MAXBLK], sr[MAXBLK]; int rows[MAXBLK];
    unsigned long long tab; unsigned sources;
};

int plan_rows(const char* who, int dtype, int n_blocks, const void* const* blk, const long long* blk_ld, const long long* row_ld,
              const int* blk_rows, int R, const int* n_src, const int* src, int n_sets, int B, RowPlan& pl) {
    MTMP_CHECK_ARG(blk && blk_ld && row_ld && blk_rows && n_src && src, "%s: a NULL table", who);
    MTMP_CHECK_ARG(B > 0 && B <= MAXB && R >= 1 && R <= MAXR && n_blocks >= 1 && n_blocks <= MAXBLK && (n_sets == 1 || n_sets == R) &&
                       (dtype == 0 || dtype == 1),
                   "%s: bad argument (B=%d, needs 1 <= B <= %d; R=%d, needs 1 <= R <= %d; %d blocks, 1 .. %d; n_sets %d is 1 or R; dtype %d)",
                   who, B, MAXB, R, MAXR, n_blocks, MAXBLK, n_sets, dtype);
    for (int s = 0; s < MAXBLK; ++s) { pl.p[s] = nullptr; pl.sb[s] = pl.sr[s] = 0; pl.rows[s] = 0; }
    for (int s = 0; s < n_blocks; ++s) {
        MTMP_CHECK_ARG(blk[s] && ((uintptr_t)blk[s] & 15) == 0 && blk_rows[s] >= 1 && blk_rows[s] <= MAXP && blk_ld[s] >= D &&
                           blk_ld[s] % 4 == 0 && row_ld[s] >= D && row_ld[s] % 4 == 0,
                       "%s: block %d needs a 16-byte aligned base, 1 .. %d rows, and sample and row strides >= 256 that are multiples of 4",
                       who, s, MAXP);
        pl.p[s] = blk[s]; pl.sb[s] = blk_ld[s]; pl.sr[s] = row_ld[s]; pl.rows[s] = blk_rows[s];
    }
    pl.tab = 0; pl.sources = 0;
    for (int m = 0; m < R; ++m) {
        MTMP_CHECK_ARG(n_src[m] >= 1 && n_src[m] <= MAXSRC, "%s: head row %d reads %d sources (1 .. %d)", who, m, n_src[m], MAXSRC);
        unsigned long long code = (unsigned)n_src[m];
        for (int i = 0; i < n_src[m]; ++i) {
            const int s = src[2 * (MAXSRC * m + i)], r = src[2 * (MAXSRC * m + i) + 1];
            MTMP_CHECK_ARG(s >= 0 && s < n_blocks && r >= 0 && r < pl.rows[s], "%s: head row %d source %d names (block %d, row %d), which is not there",
                           who, m, i, s, r);
            MTMP_CHECK_ARG(!((pl.sources >> (4 * s + r)) & 1u),
                           "%s: (block %d, row %d) feeds more than one head row: a source row may feed at most one", who, s, r);
            pl.sources |= 1u << (4 * s + r);
            code |= (unsigned long long)s << (2 + 4 * i) | (unsigned long long)r << (4 + 4 * i);
        }
        pl.tab |= code << (16 * m);
    }
    return MTMP_OK;
}

template <typename TC> Blocks<TC> blocks_of(const RowPlan& pl) {
    return Blocks<TC>{{(const TC*)pl.p[0], (const TC*)pl.p[1], (const TC*)pl.p[2], nullptr}, {pl.sb[0], pl.sb[1], pl.sb[2], 0},
                      {pl.sr[0], pl.sr[1], pl.sr[2], 0}};
}

}  // namespace

// ws_fwd: x[R][B][512] + hhat[R][B][256] + rstd[R][B] floats (kept for the backward)
extern "C" int mtmp_headr_ws_floats(int R, int B) { return R * B * (DX + D + 1); }
// ws_bwd: dh[R][B][256] + slab[B][7 x 256] floats
extern "C" int mtmp_headr_bwd_ws_floats(int R, int B) { return R * B * D + B * 7 * D; }

extern "C" int mtmp_headr_fwd(int dtype, int n_blocks, const void* const* blocks, const long long* block_ld, const long long* row_ld,
                              const int* block_rows, int R, const int* n_src, const int* src, const float* age, const float* gender,
                              const void* const* params, int n_sets, float* out, float* ws, int B, float ln_eps, void* stream) {
    RowPlan pl;
    if (int rc = plan_rows("mtmp_headr_fwd", dtype, n_blocks, blocks, block_ld, row_ld, block_rows, R, n_src, src, n_sets, B, pl)) return rc;
    MTMP_CHECK_ARG(age && gender && params && out && ws, "mtmp_headr_fwd: a NULL argument");
    for (int i = 0; i < 6 + 6 * n_sets; ++i) MTMP_CHECK_ARG(params[i], "mtmp_headr_fwd: parameter %d is NULL", i);
    const Shared3 p = shared_of(params);
    const SetsR ps = sets_of(params, n_sets, R);
    hipStream_t st = (hipStream_t)stream;
    float* x = ws; float* hh = x + (size_t)R * B * DX; float* rstd = hh + (size_t)R * B * D;
    const dim3 gx(((R + 1) * B + 3) / 4);
    if (dtype == 0)
        hipLaunchKernelGGL(headr_x_kernel<float>, gx, dim3(256), 0, st, blocks_of<float>(pl), pl.tab, age, gender, p, x, R, B, ln_eps);
    else
        hipLaunchKernelGGL(headr_x_kernel<bf16>, gx, dim3(256), 0, st, blocks_of<bf16>(pl), pl.tab, age, gender, p, x, R, B, ln_eps);
    MTMP_CHECK_LAUNCH("mtmp_headr_fwd(x)");
    const int rpl = rows_per_lane(B);
    auto fc = rpl == 1 ? headr_fc_kernel<1> : (rpl == 2 ? headr_fc_kernel<2> : headr_fc_kernel<4>);
    hipLaunchKernelGGL(fc, dim3(D / FPW, R), dim3(256), 0, st, (const float*)x, ps, hh, B);
    MTMP_CHECK_LAUNCH("mtmp_headr_fwd(fc)");
    hipLaunchKernelGGL(headr_out_kernel, dim3((R * B + 3) / 4), dim3(256), 0, st, hh, rstd, ps, out, R, B, ln_eps);
    MTMP_CHECK_LAUNCH("mtmp_headr_fwd(out)");
    return MTMP_OK;
}

extern "C" int mtmp_headr_bwd(int dtype, const float* d_out, int n_blocks, const void* const* blocks, const long long* block_ld,
                              const long long* row_ld, const int* block_rows, int R, const int* n_src, const int* src, const float* age,
                              const float* gender, const void* const* params, int n_sets, const float* ws_fwd, void* const* dblocks,
                              float* const* dst, float* ws_bwd, int B, float ln_eps, void* stream) {
    RowPlan pl;
    if (int rc = plan_rows("mtmp_headr_bwd", dtype, n_blocks, blocks, block_ld, row_ld, block_rows, R, n_src, src, n_sets, B, pl)) return rc;
    MTMP_CHECK_ARG(d_out && age && gender && params && ws_fwd && dblocks && dst && ws_bwd, "mtmp_headr_bwd: a NULL argument");
    for (int s = 0; s < n_blocks; ++s) MTMP_CHECK_ARG(dblocks[s], "mtmp_headr_bwd: gradient block %d is NULL", s);
    for (int i = 0; i < 6 + 6 * n_sets; ++i) MTMP_CHECK_ARG(params[i] && dst[i], "mtmp_headr_bwd: parameter / destination %d is NULL", i);
    const Shared3 p = shared_of(params);
    const SetsR ps = sets_of(params, n_sets, R);
    GradsR gs;
    for (int m = 0; m < MAXR; ++m) {
        float* const* r = dst + 6 + (n_sets == 1 ? 0 : 6 * (m < R ? m : 0));
        gs.s[m] = SetGrads{r[0], r[1], r[2], r[3], r[4], r[5]};
    }
    hipStream_t st = (hipStream_t)stream;
    const float* x = ws_fwd; const float* hh = x + (size_t)R * B * DX; const float* rstd = hh + (size_t)R * B * D;
    float* dh = ws_bwd; float* slab = dh + (size_t)R * B * D;
    hipLaunchKernelGGL(headr_row_bwd_kernel, dim3((R * B + 3) / 4), dim3(256), 0, st, d_out, hh, rstd, ps, dh, R, B);
    MTMP_CHECK_LAUNCH("mtmp_headr_bwd(row)");
    const int rpl = rows_per_lane(B);
    auto fcb = rpl == 1 ? headr_fc_bwd_kernel<1> : (rpl == 2 ? headr_fc_bwd_kernel<2> : headr_fc_bwd_kernel<4>);
    const bool shared = n_sets == 1;
    hipLaunchKernelGGL(fcb, dim3(D / FPW, shared ? 1 : R), dim3(256), 0, st, d_out, x, hh, (const float*)dh, ps, gs, B, shared ? R : 1);
    MTMP_CHECK_LAUNCH("mtmp_headr_bwd(fc)");
    if (dtype == 0) {
        DBlocks<float> d{{(float*)dblocks[0], n_blocks > 1 ? (float*)dblocks[1] : nullptr, n_blocks > 2 ? (float*)dblocks[2] : nullptr},
                         {pl.rows[0], pl.rows[1], pl.rows[2]}, pl.sources};
        hipLaunchKernelGGL(headr_x_bwd_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)dh, blocks_of<float>(pl), pl.tab, age, gender,
                           p, ps, d, slab, R, B, ln_eps);
    } else {
        DBlocks<bf16> d{{(bf16*)dblocks[0], n_blocks > 1 ? (bf16*)dblocks[1] : nullptr, n_blocks > 2 ? (bf16*)dblocks[2] : nullptr},
                        {pl.rows[0], pl.rows[1], pl.rows[2]}, pl.sources};
        hipLaunchKernelGGL(headr_x_bwd_kernel<bf16>, dim3(B), dim3(256), 0, st, (const float*)dh, blocks_of<bf16>(pl), pl.tab, age, gender,
                           p, ps, d, slab, R, B, ln_eps);
    }
    MTMP_CHECK_LAUNCH("mtmp_headr_bwd(x)");
    launch_rows_scatter(slab, B, dst, st);
    MTMP_CHECK_LAUNCH("mtmp_headr_bwd(scatter)");
    return MTMP_OK;
}

extern "C" int mtmp_flex_combine_fwd(const float* o, const float* a, float temperature, const long long* missing_num, unsigned table,
                                     float* out, int R, int B, void* stream) {
    MTMP_CHECK_ARG(o && a && missing_num && out && B > 0 && R >= 1 && R <= MAXR, "mtmp_flex_combine_fwd: bad argument (R=%d B=%d)", R, B);
    MTMP_CHECK_ARG(table <= 0xFFFFu, "mtmp_flex_combine_fwd: table has bits outside 4 patterns x 4 rows (%#x)", table);
    hipLaunchKernelGGL(flex_combine_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, o, a, temperature, missing_num,
                       table, out, R, B);
    MTMP_CHECK_LAUNCH("mtmp_flex_combine_fwd");
    return MTMP_OK;
}

extern "C" int mtmp_flex_combine_bwd(const float* d_out, const float* o, const float* a, float temperature, const long long* missing_num,
                                     unsigned table, float* d_o, float* d_a, int R, int B, void* stream) {
    MTMP_CHECK_ARG(d_out && o && a && missing_num && d_o && d_a && B > 0 && R >= 1 && R <= MAXR,
                   "mtmp_flex_combine_bwd: bad argument (R=%d B=%d)", R, B);
    MTMP_CHECK_ARG(table <= 0xFFFFu, "mtmp_flex_combine_bwd: table has bits outside 4 patterns x 4 rows (%#x)", table);
    hipLaunchKernelGGL(flex_combine_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_out, o, a, temperature, missing_num, table,
                       d_o, d_a, R, B);
    MTMP_CHECK_LAUNCH("mtmp_flex_combine_bwd");
    return MTMP_OK;
}
