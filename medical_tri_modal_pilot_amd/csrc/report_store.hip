// Report token embeddings from a device-resident embedding store (builder/data/report_store.py holds the store and the host plan).
//
// mtmp_report_gather   one launch per batch.  The reference's loader (dataset_new.py:2135-2155) reads a report's [len, 768]
//   embeddings, appends zeros up to [128, 768] and the collate stacks [B, 128, 768].  The store keeps every report's rows back to
//   back, so sample b of the batch is ONE contiguous run of n_b * W elements (from row first_b of the store) followed by
//   (L - n_b) * W zeros: a copy of a run and a fill, per sample, with an optional change of type on the way.
//   Geometry: a lane moves "pieces" of 16 bytes of the WIDER of the two types -- 4 elements for f32 -> f32, 8 otherwise
//   (bf16 -> bf16: one 16-byte load, one 16-byte store; f32 -> bf16: two loads, one store; bf16 -> f32: one load, two stores), so
//   every global access is 16 bytes per lane and a wave-instruction covers 1 KiB (or, at two accesses per piece, two
//   instructions cover 2 KiB) of contiguous memory whatever W is; W % 8 == 0 makes a row a whole number of pieces in both types.
//   A workgroup of 256 lanes takes CHUNK = 4 x 256 consecutive pieces of one sample: 16 KiB of bf16 output, four (eight)
//   independent loads per lane in flight before the first store.  At B 64, L 128, W 768 that is 12 chunks per sample = 768
//   workgroups, three per CU, 12 waves per CU -- the kernel has no reuse and no arithmetic to hide, what it needs is enough
//   bytes in flight per CU and whole cache lines per instruction.  A chunk that lies wholly in the run takes the unguarded
//   path (all loads, then all stores), a chunk wholly behind it only stores zeros and reads NOTHING from the store, the one
//   chunk per sample that holds the boundary guards each piece.  The zeros are written here: no memset in front, no pad
//   launch behind.  Every index is 64-bit.  A descriptor row outside [0, total_tokens] or with n > L makes its sample zeros.
//   f32 -> bf16 rounds to nearest even on the bits, the way torch's .to(torch.bfloat16) does (NaN stays NaN: the
//   quiet 0x7FC0); bf16 -> f32 is a 16-bit shift.  The kernel never interprets a value as a float: no denormal mode can touch it.
#include "common.hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int UNROLL = 4;
constexpr int CHUNK = THREADS * UNROLL;      // pieces per workgroup
constexpr int DESC_WORDS = 2;                // first token row, token count

MTMP_DEV u32x4_t ld16(const void* p) { return *reinterpret_cast<const u32x4_t*>(p); }
MTMP_DEV void st16(void* p, u32x4_t v) { *reinterpret_cast<u32x4_t*>(p) = v; }

// float32 bits -> bfloat16 bits, round to nearest even; a NaN becomes the quiet NaN 0x7FC0 (c10::BFloat16's rule, both)
MTMP_DEV unsigned bf16_bits(unsigned x) {
    const unsigned r = (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
    return (x & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC0u : r;
}

// one piece: ESZ-byte elements in, OSZ-byte elements out (2 = bf16, 4 = f32)
template <int ESZ, int OSZ> struct Piece {
    static constexpr int ELEMS = (ESZ == 4 && OSZ == 4) ? 4 : 8;
    static constexpr int NLOAD = ELEMS * ESZ / 16, NSTORE = ELEMS * OSZ / 16;
    u32x4_t v[NLOAD];

    MTMP_DEV void load(const char* src, long long piece) {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) v[i] = ld16(src + (piece * NLOAD + i) * 16);
    }
    MTMP_DEV void zero() {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) v[i] = u32x4_t{0u, 0u, 0u, 0u};
    }
    MTMP_DEV void store(char* dst, long long piece) const {
        char* p = dst + piece * NSTORE * 16;
        if constexpr (ESZ == OSZ) {
            st16(p, v[0]);
        } else if constexpr (ESZ == 4) {         // f32 -> bf16: element 2j in the low half of word j
            const unsigned w[8] = {v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3]};
            u32x4_t o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = bf16_bits(w[2 * j]) | (bf16_bits(w[2 * j + 1]) << 16);
            st16(p, o);
        } else {                                 // bf16 -> f32: exact
            st16(p, u32x4_t{v[0][0] << 16, v[0][0] & 0xFFFF0000u, v[0][1] << 16, v[0][1] & 0xFFFF0000u});
            st16(p + 16, u32x4_t{v[0][2] << 16, v[0][2] & 0xFFFF0000u, v[0][3] << 16, v[0][3] & 0xFFFF0000u});
        }
    }
};

template <int ESZ, int OSZ>
__global__ __launch_bounds__(THREADS) void report_gather_kernel(const char* __restrict__ emb, long long total_tokens,
                                                                const long long* __restrict__ desc, char* __restrict__ out, int L,
                                                                int W, int chunks) {
    using P = Piece<ESZ, OSZ>;
    const long long b = blockIdx.x / (unsigned)chunks;
    const long long chunk0 = (long long)(blockIdx.x % (unsigned)chunks) * CHUNK;
    const long long first = desc[b * DESC_WORDS], n_raw = desc[b * DESC_WORDS + 1];
    const bool sane = first >= 0 && n_raw >= 0 && n_raw <= L && first <= total_tokens - n_raw;
    const long long n = sane ? n_raw : 0;
    const long long pieces = (long long)L * W / P::ELEMS;        // of the sample
    const long long live = n * W / P::ELEMS;                     // ... of which the store fills the first
    const char* src = emb + (sane ? first : 0) * W * ESZ;
    char* dst = out + b * L * W * OSZ;
    const long long p0 = chunk0 + threadIdx.x;
    P pc[UNROLL];
    if (chunk0 + CHUNK <= live) {                                // wholly inside the run
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) pc[u].load(src, p0 + u * THREADS);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) pc[u].store(dst, p0 + u * THREADS);
    } else if (chunk0 >= live) {                                 // wholly behind it: zeros, nothing is read
        pc[0].zero();
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            if (p0 + u * THREADS < pieces) pc[0].store(dst, p0 + u * THREADS);
    } else {                                                     // the boundary chunk
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            pc[u].zero();
            if (p0 + u * THREADS < live) pc[u].load(src, p0 + u * THREADS);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            if (p0 + u * THREADS < pieces) pc[u].store(dst, p0 + u * THREADS);
    }
}

}  // namespace

extern "C" int mtmp_report_gather(const void* emb, int emb_dtype, long long total_tokens, const long long* desc, void* out,
                                  int out_dtype, int B, int L, int W, void* stream) {
    MTMP_CHECK_ARG(desc && out && (emb || total_tokens == 0), "mtmp_report_gather: null pointer");
    MTMP_CHECK_ARG((emb_dtype == 0 || emb_dtype == 1) && (out_dtype == 0 || out_dtype == 1),
                   "mtmp_report_gather: dtype codes %d -> %d (MTMP_F32 = 0, MTMP_BF16 = 1)", emb_dtype, out_dtype);
    MTMP_CHECK_ARG(W >= 8 && W % 8 == 0, "mtmp_report_gather: width %d is not a positive multiple of 8", W);
    MTMP_CHECK_ARG(B > 0 && B <= (1 << 20) && L > 0 && L <= (1 << 16) && total_tokens >= 0,
                   "mtmp_report_gather: bad argument (B=%d L=%d tokens=%lld)", B, L, total_tokens);
    MTMP_CHECK_ARG(((uintptr_t)emb & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0,
                   "mtmp_report_gather: emb and out must be 16-byte aligned, desc 8-byte");
    const int elems = (emb_dtype == 0 && out_dtype == 0) ? 4 : 8;
    const long long pieces = (long long)L * W / elems;
    const long long chunks = (pieces + CHUNK - 1) / CHUNK;
    const long long blocks = (long long)B * chunks;
    MTMP_CHECK_ARG(blocks * THREADS <= 0xffffffffLL, "mtmp_report_gather: %lld workgroups of %d lanes are more than a grid holds",
                   blocks, THREADS);
    const dim3 grid((unsigned)blocks), block(THREADS);
    hipStream_t st = (hipStream_t)stream;
    const char* e = (const char*)emb;
    char* o = (char*)out;
    if (emb_dtype == 0 && out_dtype == 0)
        hipLaunchKernelGGL((report_gather_kernel<4, 4>), grid, block, 0, st, e, total_tokens, desc, o, L, W, (int)chunks);
    else if (emb_dtype == 1 && out_dtype == 1)
        hipLaunchKernelGGL((report_gather_kernel<2, 2>), grid, block, 0, st, e, total_tokens, desc, o, L, W, (int)chunks);
    else if (emb_dtype == 0)
        hipLaunchKernelGGL((report_gather_kernel<4, 2>), grid, block, 0, st, e, total_tokens, desc, o, L, W, (int)chunks);
    else
        hipLaunchKernelGGL((report_gather_kernel<2, 4>), grid, block, 0, st, e, total_tokens, desc, o, L, W, (int)chunks);
    MTMP_CHECK_LAUNCH("mtmp_report_gather");
    return MTMP_OK;
}
