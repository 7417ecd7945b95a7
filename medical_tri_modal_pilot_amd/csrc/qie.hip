// The QIE input of TRI_MBT_VSLTCLS (--vslt-type QIE, tri_mbt_vsltcls.py:191-198, 216-221) for gfx950: the demographic embedding
//     demo[b] = ReLU(LN(age[b] * w[:,0] + gender[b] * w[:,1] + b))                      ie_demo (Linear(2,256), LayerNorm, ReLU)
// is added to EVERY token of the three streams instead of being concatenated in front of the head:
//     add_v[b] = demo[b]      add_i[b] = it[b] + demo[b]      add_t[b] = tt[b] + demo[b]
// (it / tt: the time + modality embedding of sample b's image / report).  The three rows per sample are what the stream-input
// kernels add to their tokens (mtmp_stream_input_fwd_add, add_L = the stream's token count), so the [B,T,256] broadcast add, its
// summing backward and the ie_demo torch chain are gone from the step.
//   forward : qie_adds_fwd   one wave per sample (demo_row_fwd of head_common.hip.h), fp32, rounded once to the stream's type
//   backward: qie_sums       partial sums over the token axis of the three streams' input gradients
//             qie_combine    d_demo[b] in fp32 -> demo_row_bwd -> one slab row per sample; the workgroup that finishes LAST sums the
//                            slab rows into the four parameter gradients' destinations
// Nothing is kept for the backward: demo_row_bwd recomputes the LayerNorm of ie_demo from (age, gender) as the heads do.
// Deterministic: no float atomics, every sum in a fixed order (the one integer atomic counts finished workgroups; WHICH workgroup
// comes last changes nothing, the slab rows are always summed in the order b = 0 .. B-1).
#include "head_common.hip.h"

namespace {

// ---- the token split of the backward ----
// Sample b's work is S = SV + (2 when the image / text gradients are given) chunks, one workgroup each (grid B * S):
//   chunks 0 .. SV-1, SV = ceil(N_v / 64): tokens 64 c .. min(64 c + 64, n_live) - 1 of dx_v[b], n_live = N_v, or for a packed
//       stream min(N_v, max(kv_len[b] - kv_off, 0)) -- the rows past it are zeros and are not read;
//   chunk SV: all N_i tokens of dx_i[b];  chunk SV + 1: all N_t tokens of dx_t[b].
// Inside a chunk of L tokens wave w sums tokens w, w + 4, w + 8, ... with two rows in flight (t and t + 4, step 8, one single row
// behind the loop), in fp32; the four waves' sums are combined as (0 + 1) + (2 + 3) -- for the image / text chunk this is
// mtmp_token_sums' order, so d_it / d_tt (that sum rounded to the streams' type) have its bits.
// Loop edges this creates: L <= 4 (waves without a row), L = 5 and 9 (the first pair / the single row behind a pair), L = 8 (pairs
// only), N_v = 64 / 65 and 128 / 129 (a full last chunk / a chunk of one token), a packed sample with n_live = 1 beside one with
// n_live = N_v (empty chunks write zeros).  B = 64, N_v = 1000: 64 * 18 = 1152 workgroups for 256 CUs.
constexpr int CH = 64;

struct QieSums {
    const void *dx_v, *dx_i, *dx_t;      // [B][N_*][256] in the streams' type; dx_i / dx_t NULL together
    const int* kv_len; int kv_off;       // packed vital-sign stream: rows in use per sample (bottleneck + CLS rows included), or NULL
    void *d_it, *d_tt;                   // [B][256] in the streams' type
    float* partial;                      // [B][S][256]
    unsigned* counter;                   // finished workgroups of qie_combine: zeroed here, in front of it on the stream
    int B, N_v, N_i, N_t, SV, S;
};

template <typename T>
__global__ __launch_bounds__(256) void qie_sums_kernel(QieSums q) {
    __shared__ __attribute__((aligned(16))) float part[4][D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = (int)blockIdx.x / q.S, c = (int)blockIdx.x - b * q.S;
    if (blockIdx.x == 0 && threadIdx.x == 0) *q.counter = 0u;
    const T* base;
    int L;
    if (c < q.SV) {
        const int n_live = q.kv_len ? min(q.N_v, max(q.kv_len[b] - q.kv_off, 0)) : q.N_v;
        L = max(min(CH, n_live - c * CH), 0);
        base = (const T*)q.dx_v + ((size_t)b * q.N_v + (size_t)c * CH) * D;
    } else if (c == q.SV) {
        L = q.N_i;
        base = (const T*)q.dx_i + (size_t)b * q.N_i * D;
    } else {
        L = q.N_t;
        base = (const T*)q.dx_t + (size_t)b * q.N_t * D;
    }
    base += 4 * lane;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
    int t = wave;
    for (; t + 4 < L; t += 8) {                                    // two rows in flight per wave
        a0 += load4<T>(base + (size_t)t * D);
        a1 += load4<T>(base + (size_t)(t + 4) * D);
    }
    if (t < L) a0 += load4<T>(base + (size_t)t * D);
    *reinterpret_cast<f32x4*>(&part[wave][4 * lane]) = a0 + a1;
    __syncthreads();
    if (wave == 0) {
        const f32x4 v = (*reinterpret_cast<const f32x4*>(&part[0][4 * lane]) + *reinterpret_cast<const f32x4*>(&part[1][4 * lane])) +
                        (*reinterpret_cast<const f32x4*>(&part[2][4 * lane]) + *reinterpret_cast<const f32x4*>(&part[3][4 * lane]));
        *reinterpret_cast<f32x4*>(q.partial + ((size_t)b * q.S + c) * D + 4 * lane) = v;          // fp32: d_demo is never rounded
        if (c >= q.SV) store4<T>((T*)(c == q.SV ? q.d_it : q.d_tt) + (size_t)b * D + 4 * lane, v[0], v[1], v[2], v[3]);
    }
}

struct QieDst { float *w, *b, *g, *be; };      // d ie_demo.0.weight [256][2], d ie_demo.0.bias, d ie_demo.1.weight, d ie_demo.1.bias

// workgroup = sample b, thread = column k: d_demo[b][k] = the S partial sums in chunk order, the ie_demo backward into slab row b
// (blocks 2 .. 6 of a 7 x 256 row, ie_demo.0.weight's two columns interleaved), and -- in the workgroup that finishes last -- the
// column sums of the B slab rows in the order b = 0 .. B-1 (four running sums over b mod 4, combined as (0 + 1) + (2 + 3)).
__global__ __launch_bounds__(256) void qie_combine_kernel(const float* partial, const float* age, const float* gen, Shared3 p,
                                                          float* slab, unsigned* counter, QieDst dst, int S, float eps) {
    __shared__ float red[4];
    __shared__ int last;
    const int b = blockIdx.x, k = threadIdx.x, B = gridDim.x;
    float dd = 0.f;
    for (int c = 0; c < S; ++c) dd += partial[((size_t)b * S + c) * D + k];
    demo_row_bwd<true>(age[b], gen[b], p, dd, eps, red, k, slab + (size_t)b * 7 * D);
    __threadfence();                              // this workgroup's slab row is visible to the device before its ticket is drawn
    __syncthreads();
    if (k == 0) last = atomicAdd(counter, 1u) == (unsigned)(B - 1) ? 1 : 0;
    __syncthreads();
    if (!last) return;
    __threadfence();                              // the other workgroups' rows, written before their tickets
    float s[5][4];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[m][i] = 0.f;
    const float* col = slab + 2 * D + k;
    int r = 0;
    for (; r + 4 <= B; r += 4)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 0; m < 5; ++m) s[m][i] += col[(size_t)(r + i) * 7 * D + m * D];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (r + i < B)
#pragma unroll
            for (int m = 0; m < 5; ++m) s[m][i] += col[(size_t)(r + i) * 7 * D + m * D];
    float o[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) o[m] = (s[m][0] + s[m][1]) + (s[m][2] + s[m][3]);
    dst.g[k] = o[0];
    dst.be[k] = o[1];
    dst.w[k] = o[2];
    dst.w[D + k] = o[3];
    dst.b[k] = o[4];
}

// one wave per sample, lane owns columns 4 lane .. 4 lane + 3
template <typename T>
__global__ __launch_bounds__(256) void qie_adds_fwd_kernel(const float* age, const float* gen, Shared3 p, const T* it, const T* tt,
                                                           T* add_v, T* add_i, T* add_t, int B, float eps) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                                          // (wave-uniform)
    const int c = 4 * lane;
    const f32x4 d = demo_row_fwd(age[b], gen[b], p, c, eps);
    const size_t o = (size_t)b * D + c;
    store4<T>(add_v + o, d[0], d[1], d[2], d[3]);
    if (it) {
        const f32x4 a = load4<T>(it + o), t = load4<T>(tt + o);
        store4<T>(add_i + o, a[0] + d[0], a[1] + d[1], a[2] + d[2], a[3] + d[3]);
        store4<T>(add_t + o, t[0] + d[0], t[1] + d[1], t[2] + d[2], t[3] + d[3]);
    }
}

inline Shared3 demo_params_of(const void* const* q) {      // ie_demo.{0.weight [256][2], 0.bias, 1.weight, 1.bias}; no head LayerNorm here
    return Shared3{(const float*)q[0], (const float*)q[1], (const float*)q[2], (const float*)q[3], nullptr, nullptr};
}
inline int qie_chunks(int N_v, int with_time) { return (N_v + CH - 1) / CH + (with_time ? 2 : 0); }

}  // namespace

// params: the four ie_demo device pointers (float).  age / gender float[B].  it / tt [B][256] in `dtype` or NULL TOGETHER
// (--imgtxt-time 0: add_i / add_t are then neither read nor written).  add_v / add_i / add_t [B][256] in `dtype`.
extern "C" int mtmp_qie_adds_fwd(int dtype, const float* age, const float* gender, const void* const* params, const void* it,
                                 const void* tt, void* add_v, void* add_i, void* add_t, int B, float ln_eps, void* stream) {
    MTMP_CHECK_ARG(age && gender && params && add_v && B > 0 && (!it) == (!tt) && (!it || (add_i && add_t)),
                   "mtmp_qie_adds_fwd: bad argument (B=%d; it and tt are given together, with add_i and add_t)", B);
    for (int i = 0; i < 4; ++i) MTMP_CHECK_ARG(params[i], "mtmp_qie_adds_fwd: parameter %d is NULL", i);
    const Shared3 p = demo_params_of(params);
    return with_dtype(dtype, "mtmp_qie_adds_fwd", [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(qie_adds_fwd_kernel<T>, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, age, gender, p, (const T*)it,
                           (const T*)tt, (T*)add_v, (T*)add_i, (T*)add_t, B, ln_eps);
        MTMP_CHECK_LAUNCH("mtmp_qie_adds_fwd");
        return MTMP_OK;
    });
}

// ws: B * (chunks + 7) * 256 + 1 floats, chunks = ceil(N_v / 64) + (2 with dx_i / dx_t)
extern "C" long long mtmp_qie_adds_bwd_ws_floats(int B, int N_v, int with_time) {
    return (long long)B * (qie_chunks(N_v, with_time) + 7) * D + 1;
}

// dx_v [B][N_v][256], dx_i [B][N_i][256], dx_t [B][N_t][256] in `dtype` (dx_i / dx_t NULL together, with d_it / d_tt); kv_len
// (device int32[B], may be NULL): sample b's dx_v rows from max(kv_len[b] - kv_off, 0) on are zeros and are skipped.
// d_it / d_tt [B][256] in `dtype`; dst[4]: the gradients of the four ie_demo parameters in the order of `params` (overwritten).
extern "C" int mtmp_qie_adds_bwd(int dtype, const void* dx_v, const void* dx_i, const void* dx_t, const int32_t* kv_len, int kv_off,
                                 const float* age, const float* gender, const void* const* params, void* d_it, void* d_tt,
                                 float* const* dst, float* ws, int B, int N_v, int N_i, int N_t, float ln_eps, void* stream) {
    MTMP_CHECK_ARG(dx_v && age && gender && params && dst && ws && B > 0 && N_v > 0 && kv_off >= 0 && (!dx_i) == (!dx_t) &&
                       (!dx_i || (d_it && d_tt && N_i > 0 && N_t > 0)) && (long long)B * N_v < (1ll << 25) &&
                       (!dx_i || ((long long)B * N_i < (1ll << 25) && (long long)B * N_t < (1ll << 25))),
                   "mtmp_qie_adds_bwd: bad argument (B=%d N_v=%d N_i=%d N_t=%d; dx_i, dx_t, d_it and d_tt are given together)", B, N_v,
                   N_i, N_t);
    for (int i = 0; i < 4; ++i) MTMP_CHECK_ARG(params[i] && dst[i], "mtmp_qie_adds_bwd: parameter or destination %d is NULL", i);
    const Shared3 p = demo_params_of(params);
    QieSums q;
    q.dx_v = dx_v; q.dx_i = dx_i; q.dx_t = dx_t; q.kv_len = kv_len; q.kv_off = kv_off; q.d_it = d_it; q.d_tt = d_tt;
    q.B = B; q.N_v = N_v; q.N_i = N_i; q.N_t = N_t;
    q.SV = (N_v + CH - 1) / CH;
    q.S = qie_chunks(N_v, dx_i != nullptr);
    q.partial = ws;
    float* slab = ws + (size_t)B * q.S * D;
    q.counter = reinterpret_cast<unsigned*>(slab + (size_t)B * 7 * D);
    MTMP_CHECK_ARG((long long)B * q.S < (1ll << 30), "mtmp_qie_adds_bwd: grid of %lld workgroups", (long long)B * q.S);
    hipStream_t st = (hipStream_t)stream;
    const QieDst d{dst[0], dst[1], dst[2], dst[3]};
    return with_dtype(dtype, "mtmp_qie_adds_bwd", [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(qie_sums_kernel<T>, dim3(B * q.S), dim3(256), 0, st, q);
        MTMP_CHECK_LAUNCH("mtmp_qie_adds_bwd(sums)");
        hipLaunchKernelGGL(qie_combine_kernel, dim3(B), dim3(256), 0, st, (const float*)q.partial, age, gender, p, slab, q.counter, d, q.S,
                           ln_eps);
        MTMP_CHECK_LAUNCH("mtmp_qie_adds_bwd(combine)");
        return MTMP_OK;
    });
}
