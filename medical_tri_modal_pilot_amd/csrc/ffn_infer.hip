// The position-wise FFN block of an encoder layer as ONE launch, for forwards that nobody differentiates (gfx950):
//
//     out[M,256] = x + relu(LN(x) W1^T + c1) W2^T + c2          (module.py:138-144, :74-80 without dropout, encoder.py:32)
//
// The training forward runs this as mtmp_ln_gemm_signs + mtmp_gemm_nt and writes what only a backward reads: LN(x), its row
// statistics, the sign bits and the [M,1024] hidden activation h, which the second launch reads back.  Here h never leaves the
// register file and the kernel writes nothing but `out`.
//
// Geometry (both dtypes): a workgroup owns 128 token rows, a wave 32 of them.  As in the row-panel kernels of gemm.hip a TOKEN is
// a lane: the wave keeps its 32 normalised rows as 16 operand fragments in registers for the whole kernel, and both products are
// computed as weight-rows x token-columns.  The hidden index is walked in 32 GROUPS of 32 features:
//     first product   hacc[32 features][32 tokens] = c1 + W1[32 g .., :] xn^T              16 MFMA k-steps over d_model
//     hand-over       W1's rows are read through swz23 (common.hip.h), so registers 8s..8s+7 of hacc are, after ReLU and the
//                     rounding to T, the k-step-s operand fragment of the second product: no lane movement, no LDS
//     second product  oacc[t] += W2[32 t .., 32 g ..] h^T   for the 8 output tiles t, 2 k-steps each   (128 accumulator registers)
// i.e. 16 + 16 MFMAs per group and one 16-byte LDS read per MFMA (bf16).  One wave per SIMD: 64 operand + 128 + 16 accumulator
// registers leave no room for a second one, and the weight ring below takes most of a CU's LDS anyway.
//
// Weights stream through LDS by LDS-DMA (dma16: 1 KiB of contiguous LDS per wave instruction, the SOURCE address is per lane) in
// UNITS of one loop step: unit u = { W1 rows of group u | the W2 columns of group u - 1 }, because step u multiplies group u's first
// product and group u - 1's second one (the conversion of one group then sits between MFMAs of two others).  Steps 0 and 32 have
// only one of the two; their unused half repeats a neighbour's, which keeps the DMA count per step static.
//   W1 part  [32 rows][256 k], 16-byte chunk c of row R at position c ^ (R & 15)       (as PanelDma in gemm.hip: conflict-free b128)
//   W2 part  pieces of RP rows: chunk p of row o at slot 64 (o / RP) + RP p + o % RP  -- a read instruction's lanes (32 rows, one
//            chunk) hit 16 different 16-byte slots per service group, and a DMA instruction still reads whole 64 / 128-byte row
//            segments of W2 (lane l: row l % RP of its piece, chunk l / RP)
// The ring holds NST units (bf16: 4 x 32 KiB, unit u + 3 is issued at the top of step u and waited for, by a COUNTED vmcnt that
// leaves the two younger units in flight, at the end of step u + 2; fp32, the parity build: 2 x 64 KiB, one unit ahead).  Nothing
// else touches vector memory inside the loop, so the counts are exact.  The ring is as deep as a CU's LDS allows because the
// loop is bound by the latency of the weight stream: with three units a step took 1.27 us (32 MFMAs are 0.45), i.e. two units
// = 64 KiB in flight per CU per ~2.5 us.
//
// Epilogue: y = T(oacc + c2) is parked in an LDS tile [128 tokens][256] that reuses the ring, then all threads walk it row-wise,
// add the residual from equally coalesced loads of x (out = T(y + x), the rounding points of mtmp_gemm_nt's epilogue) and store
// whole 512 / 1024-byte rows.  Loads and stores are unconditional: rows >= M replicate row M - 1 (recomputed and rewritten with
// the same values).
#include "common.hip.h"
#include <type_traits>

namespace {
template <int N> using ffn_int = std::integral_constant<int, N>;
using FfnYes = std::true_type;
using FfnNo = std::false_type;


template <typename T> struct FfnArgs {
    const T* x; const float* gamma; const float* beta; const T* w1; const float* c1; const T* w2; const float* c2; T* out;
    int M, ldx, ldo;
    float eps;
    const int* m_live;       // packed stream: device word holding the rows in use (<= M); common.hip.h live_rows
};

constexpr int FD = 256, FH = 1024, FNG = FH / 32, FBM = 128;     // d_model, hidden width, hidden groups, rows per workgroup

template <typename T> struct FfnGeom {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int NST = ES == 2 ? 4 : 2;                          // units in the ring
    static constexpr int ROWB1 = FD * ES, CPR1 = ROWB1 / 16;             // W1 row: bytes, 16-byte chunks
    static constexpr unsigned w1_bytes = 32u * ROWB1, w2_bytes = (unsigned)FD * 32u * ES, unit_bytes = w1_bytes + w2_bytes;
    static constexpr int CH2 = 32 * ES / 16, RP = 64 / CH2;              // W2 part: chunks per row, rows per 1 KiB piece
    static constexpr int ND1 = w1_bytes / 4096, ND2 = w2_bytes / 4096, ND = ND1 + ND2;   // DMA pieces per wave and unit
    static constexpr int LDT = FD + 16 / ES;                             // staging row (elements): 16 B pad
    static constexpr unsigned tile_bytes = (unsigned)FBM * LDT * ES, ring_bytes = NST * unit_bytes;
    static constexpr unsigned gb_off = ring_bytes > tile_bytes ? ring_bytes : tile_bytes;    // gamma | beta (prologue)
    static constexpr unsigned c1_off = gb_off + 2 * FD * 4, c2_off = c1_off + FH * 4;
    static constexpr size_t lds_bytes = c2_off + FD * 4;
    static_assert(lds_bytes <= 160 * 1024, "one workgroup's LDS");
};

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"      // (m0 is "reserved"; naming it as clobbered is exactly the point)
MTMP_DEV void ffn_dma16(unsigned voff, const void* sbase, unsigned lds_off) {
    asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_off) : "memory", "m0");
}
#pragma clang diagnostic pop
template <int N> MTMP_DEV void ffn_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// 8 consecutive k of one weight row out of an LDS image: bf16 one 16-byte chunk `ch`, fp32 the chunks ch and ch + 1; at(ch) = the
// chunk's byte offset from the lane's row pointer after the image's permutation
template <typename T, typename F> MTMP_DEV Frag<T> ffn_wfrag(const char* rowp, int ch, F at) {
    Frag<T> f;
    if constexpr (sizeof(T) == 2) {
        f.v = *reinterpret_cast<const bf16x8*>(rowp + at(ch));
    } else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(rowp + at(ch));
        const f32x4 b = *reinterpret_cast<const f32x4*>(rowp + at(ch + 1));
        f.v = f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    }
    return f;
}

template <typename T>
__global__ __launch_bounds__(256, 1) void ffn_block_kernel(Grouped<FfnArgs<T>> grp) {
    using G = FfnGeom<T>;
    constexpr int ES = G::ES, NST = G::NST;
    const int seg = grp_find(grp, (int)blockIdx.x);          // row blocks of up to three token streams in one grid (common.hip.h)
    const FfnArgs<T>& p = grp.seg[seg];
    const int bx = (int)blockIdx.x - grp.first[seg];
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, half = lane >> 5;
    float* sG = reinterpret_cast<float*>(smem_raw + G::gb_off);
    float* sC1 = reinterpret_cast<float*>(smem_raw + G::c1_off);
    float* sC2 = reinterpret_cast<float*>(smem_raw + G::c2_off);
    const int M = live_rows(p.M, p.m_live);
    if (bx * FBM >= M) return;                // (packed stream: row blocks past the rows in use)
    const int m_wave = bx * FBM + wave * 32;
    const int row = min(m_wave + r, M - 1);
    // DMA sources of this lane, bytes from the unit's first W1 row / first W2 column.  Piece i of wave w fills LDS bytes
    // [1024 (ND w + i), +1024) of its part; the lane's slot there is 16 bytes.
    unsigned d1[G::ND1], d2[G::ND2];
#pragma unroll
    for (int i = 0; i < G::ND1; ++i) {
        const unsigned q = 64u * (unsigned)(G::ND1 * wave + i) + (unsigned)lane, prow = q / G::CPR1, pos = q % G::CPR1;
        d1[i] = prow * (unsigned)G::ROWB1 + 16u * (pos ^ (prow & 15u));
    }
#pragma unroll
    for (int i = 0; i < G::ND2; ++i) {
        const unsigned o = (unsigned)(G::ND2 * wave + i) * G::RP + (unsigned)lane % G::RP, ch = (unsigned)lane / G::RP;
        d2[i] = o * (unsigned)(FH * ES) + 16u * ch;
    }
    auto unit_dma = [&](int u, int buf) __attribute__((always_inline)) {
        const char* s1 = reinterpret_cast<const char*>(p.w1 + (size_t)min(u, FNG - 1) * 32 * FD);
        const char* s2 = reinterpret_cast<const char*>(p.w2 + (size_t)max(u - 1, 0) * 32);
        const unsigned base = lds0 + (unsigned)buf * G::unit_bytes;
#pragma unroll
        for (int i = 0; i < G::ND1; ++i) ffn_dma16(d1[i], s1, base + (unsigned)(G::ND1 * wave + i) * 1024u);
#pragma unroll
        for (int i = 0; i < G::ND2; ++i) ffn_dma16(d2[i], s2, base + G::w1_bytes + (unsigned)(G::ND2 * wave + i) * 1024u);
    };
#pragma unroll
    for (int u = 0; u < NST - 1; ++u) unit_dma(u, u);
    sG[tid] = p.gamma[tid];
    sG[FD + tid] = p.beta[tid];
#pragma unroll
    for (int i = 0; i < FH / 256; ++i) sC1[256 * i + tid] = p.c1[256 * i + tid];
    sC2[tid] = p.c2[tid];
    // ---- LayerNorm prologue, in registers: lane (r, half) holds k = 16c + 8*half + j of row r
    Frag<T> af[16];
    const T* arow = p.x + (size_t)row * p.ldx + 8 * half;
#pragma unroll
    for (int c = 0; c < 16; ++c) af[c] = frag_load<T>(arow + 16 * c);
    {
        float s1 = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) s1 += to_f32(af[c].v[j]);
        s1 += __shfl_xor(s1, 32, 64);
        const float mean = s1 * (1.0f / FD);
        float s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = to_f32(af[c].v[j]) - mean; s2 = fmaf(d, d, s2); }
        s2 += __shfl_xor(s2, 32, 64);
        const float rs = 1.0f / (sqrtf(s2 * (1.0f / (FD - 1))) + p.eps);       // torch.std (Bessel-corrected), eps added to it
        __syncthreads();                                                        // sG ready
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int k = 16 * c + 8 * half;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                af[c].v[j] = from_f32<T>(fmaf(sG[k + j], (to_f32(af[c].v[j]) - mean) * rs, sG[FD + k + j]));
        }
    }
    // readers.  W1 part: row swz23(r) of the group, k-step c -> chunks from (16c + 8 half) ES / 16, XOR-ed with the row's low bits.
    // W2 part: row 32t + swz23(r), k-step s -> chunk(s) from (16s + 8 half) ES / 16 of the slot formula above.
    const int rsw = swz23(r), x15 = rsw & 15;
    const char* rd1 = smem_raw + rsw * G::ROWB1;
    const char* rd2 = smem_raw + G::w1_bytes + 16 * (64 * (rsw / G::RP) + rsw % G::RP);
    const int kch = 8 * half * ES / 16;                                        // the lane half's first chunk inside a k-step
    auto at1 = [&](int ch) __attribute__((always_inline)) { return 16 * (ch ^ x15); };
    auto at2 = [&](int ch) __attribute__((always_inline)) { return 16 * G::RP * ch; };
    ffn_wait<0>();                                               // units 0 .. NST-2 landed (this wave's share)
    __syncthreads();                                             // ... everyone's; sC1 / sC2 written
    f32x16 oacc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) oacc[t] = f32x16{0};
    Frag<T> hf[2];
    hf[0] = frag_zero<T>();
    hf[1] = frag_zero<T>();
    // step u: [unit u + NST - 1 -> ring] [first product of group u] [second product of group u - 1] [hand-over of group u];
    // FIRST / SECOND: steps 0 and 32 have one product only (compile-time, so that a step is one basic block to schedule)
    auto step = [&](int u, auto buf_tag, auto first_tag, auto second_tag) __attribute__((always_inline)) {
        constexpr int BUF = decltype(buf_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value, SECOND = decltype(second_tag)::value;
        unit_dma(min(u + NST - 1, FNG), (BUF + NST - 1) % NST);  // (a harmless repeat at the end keeps vmcnt static)
        constexpr unsigned cur = BUF * G::unit_bytes;
        f32x16 hacc;
        if constexpr (FIRST) {
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {                     // c1 as the initial accumulator, in the lane's register order
                const f32x4 v = *reinterpret_cast<const f32x4*>(sC1 + 32 * u + 16 * (i4 >> 1) + 8 * half + 4 * (i4 & 1));
                hacc[4 * i4] = v[0]; hacc[4 * i4 + 1] = v[1]; hacc[4 * i4 + 2] = v[2]; hacc[4 * i4 + 3] = v[3];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) mma<T>(hacc, ffn_wfrag<T>(rd1 + cur, c * ES + kch, at1), af[c]);
        }
        if constexpr (SECOND) {
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    mma<T>(oacc[t], ffn_wfrag<T>(rd2 + cur + t * (32 / G::RP) * 1024, s * ES + kch, at2), hf[s]);
        }
        if constexpr (FIRST) {
#pragma unroll
            for (int j = 0; j < 16; ++j) hacc[j] = relu1(hacc[j]);
            hf[0] = frag_from_acc<T>(hacc, 0);
            hf[1] = frag_from_acc<T>(hacc, 1);
        }
        ffn_wait<(NST - 2) * G::ND>();                           // unit u + 1 landed (this wave's share)
        __syncthreads();                                         // ... everyone's; unit u's buffer is free
    };
    // unit u lives in ring buffer u % NST; the buffer index is a compile-time constant of every step
    if constexpr (NST == 4) {
        step(0, ffn_int<0>{}, FfnYes{}, FfnNo{});
        step(1, ffn_int<1>{}, FfnYes{}, FfnYes{});
        step(2, ffn_int<2>{}, FfnYes{}, FfnYes{});
        step(3, ffn_int<3>{}, FfnYes{}, FfnYes{});
        for (int u0 = 4; u0 < FNG; u0 += 4) {                    // 4 .. 31
            step(u0, ffn_int<0>{}, FfnYes{}, FfnYes{});
            step(u0 + 1, ffn_int<1>{}, FfnYes{}, FfnYes{});
            step(u0 + 2, ffn_int<2>{}, FfnYes{}, FfnYes{});
            step(u0 + 3, ffn_int<3>{}, FfnYes{}, FfnYes{});
        }
        step(FNG, ffn_int<0>{}, FfnNo{}, FfnYes{});
    } else {
        static_assert(NST == 2, "the step list below is written for a ring of two");
        step(0, ffn_int<0>{}, FfnYes{}, FfnNo{});
        step(1, ffn_int<1>{}, FfnYes{}, FfnYes{});
        for (int u0 = 2; u0 < FNG; u0 += 2) {                    // 2 .. 31
            step(u0, ffn_int<0>{}, FfnYes{}, FfnYes{});
            step(u0 + 1, ffn_int<1>{}, FfnYes{}, FfnYes{});
        }
        step(FNG, ffn_int<0>{}, FfnNo{}, FfnYes{});
    }
    ffn_wait<0>();                                               // (the repeated last units must not land in the staging tile)
    __syncthreads();
    // ---- epilogue 1: y = T(oacc + c2) into the staging tile; registers 8s..8s+7 of tile t = features 32t + 16s + 8 half + j
    T* sT = reinterpret_cast<T*>(smem_raw);
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f0 = 32 * t + 16 * s + 8 * half;
            const f32x4 ca = *reinterpret_cast<const f32x4*>(sC2 + f0), cb = *reinterpret_cast<const f32x4*>(sC2 + f0 + 4);
            Frag<T> y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                y.v[j] = from_f32<T>(oacc[t][8 * s + j] + ca[j]);
                y.v[j + 4] = from_f32<T>(oacc[t][8 * s + 4 + j] + cb[j]);
            }
            frag_store<T>(sT + (32 * wave + r) * G::LDT + f0, y);
        }
    __syncthreads();
    // ---- epilogue 2: whole rows, residual from x
    constexpr int PS = FBM / 8;
    const int c8 = (tid & 31) * 8;
#pragma unroll 4
    for (int ps = 0; ps < PS; ++ps) {
        const int rl = (tid >> 5) + 8 * ps;
        const size_t grow = (size_t)min(bx * FBM + rl, M - 1);
        const Frag<T> y = frag_load<T>(sT + rl * G::LDT + c8), xr = frag_load<T>(p.x + grow * p.ldx + c8);
        Frag<T> o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = from_f32<T>(to_f32(y.v[j]) + to_f32(xr.v[j]));
        frag_store<T>(p.out + grow * p.ldo + c8, o);
    }
}

// ---- host side ("Where an entry's host code lives"): one builder, one launcher
template <typename T>
int ffn_args(FfnArgs<T>& a, const char* who, int i, const void* x, const float* gamma, const float* beta, const void* w1,
             const float* c1, const void* w2, const float* c2, void* out, int M, int ldx, int ldo, float eps, const int* m_live) {
    MTMP_CHECK_ARG(x && gamma && beta && w1 && c1 && w2 && c2 && out, "%s: null pointer (stream %d)", who, i);
    MTMP_CHECK_ARG(M > 0 && ldx >= FD && ldx % 8 == 0 && ldo >= FD && ldo % 8 == 0,
                   "%s: bad shape M=%d ldx=%d ldo=%d (d_model is fixed at 256, the hidden width at 1024; stream %d)", who, M, ldx, ldo, i);
    const char* xb = (const char*)x;
    const char* ob = (const char*)out;
    const size_t xe = ((size_t)(M - 1) * ldx + FD) * sizeof(T), oe = ((size_t)(M - 1) * ldo + FD) * sizeof(T);
    MTMP_CHECK_ARG(ob + oe <= xb || xb + xe <= ob, "%s: out aliases x (a row's residual is read after other rows are written; stream %d)",
                   who, i);
    a = FfnArgs<T>{};
    a.x = (const T*)x; a.gamma = gamma; a.beta = beta; a.w1 = (const T*)w1; a.c1 = c1; a.w2 = (const T*)w2; a.c2 = c2; a.out = (T*)out;
    a.M = M; a.ldx = ldx; a.ldo = ldo; a.eps = eps; a.m_live = m_live;
    return MTMP_OK;
}

template <typename T> int launch_ffn_block(const char* who, int n, const FfnArgs<T>* segs, hipStream_t st) {
    const auto kern = ffn_block_kernel<T>;
    if (int e = raise_lds(who, kern, FfnGeom<T>::lds_bytes)) return e;
    int nwg;
    const Grouped<FfnArgs<T>> g = make_group(n, segs, [](const FfnArgs<T>& a) { return (a.M + FBM - 1) / FBM; }, nwg);
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), FfnGeom<T>::lds_bytes, st, g);
    MTMP_CHECK_LAUNCH(who);
    return MTMP_OK;
}
}  // namespace

extern "C" int mtmp_ffn_block(int dtype, const void* x, int ldx, const float* gamma, const float* beta, const void* w1, const float* c1,
                              const void* w2, const float* c2, void* out, int ldo, int M, float eps, void* stream) {
    const char* who = "mtmp_ffn_block";
    return with_dtype(dtype, who, [&](auto tag) {
        using T = typename decltype(tag)::type;
        FfnArgs<T> a;
        if (int e = ffn_args<T>(a, who, 0, x, gamma, beta, w1, c1, w2, c2, out, M, ldx, ldo, eps, nullptr)) return e;
        return launch_ffn_block<T>(who, 1, &a, (hipStream_t)stream);
    });
}

// up to three token streams in one grid (bf16), rows_live as in the grouped row kernels of gemm.hip
extern "C" int mtmp_ffn_block_grouped(int dtype, int n, const void* const* x, const int* ldx, const float* const* gamma,
                                      const float* const* beta, const void* const* w1, const float* const* c1, const void* const* w2,
                                      const float* const* c2, void* const* out, const int* ldo, const int* M, float eps,
                                      const int32_t* const* rows_live, void* stream) {
    const char* who = "mtmp_ffn_block_grouped";
    MTMP_CHECK_ARG(n >= 1 && n <= GRP_MAX && dtype == 1, "%s: 1..%d streams, bf16 only (n=%d dtype=%d)", who, GRP_MAX, n, dtype);
    MTMP_CHECK_ARG(x && ldx && gamma && beta && w1 && c1 && w2 && c2 && out && ldo && M, "%s: null argument array", who);
    FfnArgs<bf16> a[GRP_MAX];
    for (int i = 0; i < n; ++i)
        if (int e = ffn_args<bf16>(a[i], who, i, x[i], gamma[i], beta[i], w1[i], c1[i], w2[i], c2[i], out[i], M[i], ldx[i], ldo[i], eps,
                                   rows_live ? rows_live[i] : nullptr)) return e;
    return launch_ffn_block<bf16>(who, n, a, (hipStream_t)stream);
}
