// Token-id reports (--berttype bert): the ids of a batch from a device-resident store, the lookup in the trained
// nn.Embedding(30000, 256) and its gradient (builder/data/report_store.py holds TokenReportStore and the host plan).
//
// mtmp_report_ids_gather   one launch per batch writes int32 [B][L].  The reference's loader (dataset_new.py:2157-2175 with
//   clinical_note_transform :186-192) puts a BOS (2) in front of a report's n ids, trims to L - 2 of them, appends an EOS (3),
//   pads with 1 and then replaces every 1 by 0.  In closed form, with k = min(n, L - 2):
//       out[b] = [2, t_0 .. t_{k-1}, 3, 0 .. 0]   with every t_i == 1 written as 0;   all zeros when n == 0 (a missing report).
//   A lane writes four consecutive elements of the flat [B * L] output as one 16-byte store (the tail of an output that is no
//   multiple of four elements: single words); it reads at most four ids of the store, one word each.  Every element is written
//   here: no memset in front.  A descriptor row with first < 0, n < 0 or first + n > total has its sample written as zeros.
//
// mtmp_token_embed_fwd     out[t] = table[ids[t]] for D = 256, converted as mtmp_report_gather converts (f32 -> bf16 rounds to
//   nearest even on the bits, bf16 -> f32 is a shift, equal types copy).  A lane moves one piece of 16 bytes of the WIDER of the two
//   types -- 4 elements f32 -> f32, else 8 -- so every global access is 16 bytes per lane and a row is 64 or 32 lanes.  An id
//   outside [0, V) reads NOTHING and writes a zero row.
//
// mtmp_token_embed_bwd     dw[v] = sum over {t : ids[t] == v} of dy[t], float32, for the rows v that have a token and no other.
//   No float atomics: the order of every sum depends on the positions t alone, so two runs give the same bits.  Two launches.
//   (1) embed_index_kernel sorts the positions by (id, t) -- a stable counting sort.  One wave owns a slab of SLAB consecutive
//       ids.  It reads all T ids twice (32 KB at T 8192: they stay in L2): the first pass counts its slab's ids per bin (LDS
//       integer atomics -- a count has no order) and the valid ids BELOW its slab, which is where its part of the sorted array
//       begins, so no wave waits for another; the second pass places 64 positions at a time in ascending t, the rank inside a
//       bin from a ballot.  Per sorted slot i it leaves the position perm[i], the id, the rank r of the position in its id's
//       list and the list's length n.  The heavy ids -- 0 holds the pad, every missing sample and the genuine 1s, a third to
//       a half of all rows; 2 and 3 hold B rows each -- cost their slab's wave the same two passes as any other.
//   (2) embed_sum_kernel: one wave per sorted slot; the wave of a slot with r % CHUNK == 0 sums its chunk, rows perm[i ..
//       i + min(CHUNK, n - r)), in ascending t, lane l the columns 4l .. 4l+3 (a 1 KiB float32 row is one 16-byte load per lane),
//       the others leave at once.  A list of at most CHUNK rows is one chunk and its sum is dw[v].  A longer list's chunks run
//       on as many waves as it has chunks, on whatever CUs: each stores its partial sum in the workspace, and the wave that
//       arrives last at the list's counter adds the partials in chunk order -- a fixed order whoever arrives last.  The
//       hand-over is one agent-scope release in front of the counter add and one agent-scope acquire behind it (the XCDs' L2s
//       are private), the partials are read back by plain vector loads.  The counters are zeroed by launch (1).
//   Ids outside [0, V) take no slot of the sorted array; the slots behind the valid ones are marked r = -1.
#include "common.hip.h"

namespace {

constexpr int D = 256;                       // the model dimension: the only table width
constexpr int THREADS = 256;
constexpr int SLAB = 32;                     // ids per wave of the index kernel
constexpr int CHUNK = 64;                    // rows of one partial sum (ops.token_embed_chunk())
constexpr int PREFETCH = 8;                  // id loads (index kernel) and partial-sum loads (combine) in flight per lane
constexpr int DESC_WORDS = 2;                // first id of the report in the store, number of ids

MTMP_DEV u32x4_t ld16(const void* p) { return *reinterpret_cast<const u32x4_t*>(p); }
MTMP_DEV void st16(void* p, u32x4_t v) { *reinterpret_cast<u32x4_t*>(p) = v; }

// float32 bits -> bfloat16 bits, round to nearest even; a NaN becomes the quiet NaN 0x7FC0 (c10::BFloat16's rule, both)
MTMP_DEV unsigned bf16_bits(unsigned x) {
    const unsigned r = (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
    return (x & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC0u : r;
}

// ------------------------------------------------------------------------------------------------------------ ids gather
MTMP_DEV int report_id(const int* __restrict__ ids, long long total, const long long* __restrict__ desc, long long e, int L) {
    const long long b = e / L;
    const int j = (int)(e - b * L);
    const long long first = desc[b * DESC_WORDS], n = desc[b * DESC_WORDS + 1];
    if (!(first >= 0 && n > 0 && first <= total - n)) return 0;
    const long long k = n < L - 2 ? n : L - 2;
    if (j == 0) return 2;
    if (j <= k) {
        const int v = ids[first + j - 1];
        return v == 1 ? 0 : v;
    }
    return j == k + 1 ? 3 : 0;
}

__global__ __launch_bounds__(THREADS) void report_ids_kernel(const int* __restrict__ ids, long long total,
                                                             const long long* __restrict__ desc, int* __restrict__ out,
                                                             long long elems, int L) {
    const long long e0 = ((long long)blockIdx.x * THREADS + threadIdx.x) * 4;
    if (e0 + 4 <= elems) {
        u32x4_t v;
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (unsigned)report_id(ids, total, desc, e0 + u, L);
        st16(out + e0, v);
    } else {
        for (long long e = e0; e < elems; ++e) out[e] = report_id(ids, total, desc, e, L);
    }
}

// --------------------------------------------------------------------------------------------------------------- forward
template <int ESZ, int OSZ>
__global__ __launch_bounds__(THREADS) void token_embed_fwd_kernel(const int* __restrict__ ids, long long T,
                                                                  const char* __restrict__ table, char* __restrict__ out, int V) {
    constexpr int ELEMS = (ESZ == 4 && OSZ == 4) ? 4 : 8;
    constexpr int PPR = D / ELEMS;                           // pieces per row
    constexpr int NLOAD = ELEMS * ESZ / 16, NSTORE = ELEMS * OSZ / 16;
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    const long long t = p / PPR;
    const int c = (int)(p % PPR);
    if (t >= T) return;
    const int id = ids[t];
    u32x4_t v[NLOAD];
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) v[i] = u32x4_t{0u, 0u, 0u, 0u};
    if ((unsigned)id < (unsigned)V) {                        // an id outside the table never becomes an address
        const char* src = table + ((long long)id * D + (long long)c * ELEMS) * ESZ;
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) v[i] = ld16(src + 16 * i);
    }
    char* dst = out + (t * D + (long long)c * ELEMS) * OSZ;
    if constexpr (ESZ == OSZ) {
        st16(dst, v[0]);
    } else if constexpr (ESZ == 4) {                         // f32 -> bf16: element 2j in the low half of word j
        const unsigned w[8] = {v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3]};
        u32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = bf16_bits(w[2 * j]) | (bf16_bits(w[2 * j + 1]) << 16);
        st16(dst, o);
    } else {                                                 // bf16 -> f32: exact
        static_assert(NSTORE == 2, "one bf16 piece is two float32 stores");
        st16(dst, u32x4_t{v[0][0] << 16, v[0][0] & 0xFFFF0000u, v[0][1] << 16, v[0][1] & 0xFFFF0000u});
        st16(dst + 16, u32x4_t{v[0][2] << 16, v[0][2] & 0xFFFF0000u, v[0][3] << 16, v[0][3] & 0xFFFF0000u});
    }
}

// -------------------------------------------------------------------------------------------------------------- backward
// the workspace: four int32 [T] arrays, the counters, then (16-byte aligned) the partial sums
struct BwdWs {
    int *perm, *idv, *rnk, *cntv, *counters;
    float* part;
    int ncounters;
    long long bytes;
};
BwdWs bwd_workspace(void* base, long long T) {
    BwdWs w;
    const long long nc = (T + CHUNK - 1) / CHUNK;
    const long long ints = (4 * T + nc + 3) / 4 * 4;
    w.perm = (int*)base;
    w.idv = w.perm + T;
    w.rnk = w.idv + T;
    w.cntv = w.rnk + T;
    w.counters = w.cntv + T;
    w.part = (float*)(w.perm + ints);
    w.ncounters = (int)nc;
    w.bytes = ints * 4 + 2 * nc * D * 4;
    return w;
}

__global__ __launch_bounds__(64) void embed_index_kernel(const int* __restrict__ ids, int T, int V, int* __restrict__ perm,
                                                         int* __restrict__ idv, int* __restrict__ rnk, int* __restrict__ cntv,
                                                         int* __restrict__ counters, int ncounters) {
    __shared__ int cnt[SLAB];
    const int lane = threadIdx.x;
    const int slab0 = blockIdx.x * SLAB;
    if (lane < SLAB) cnt[lane] = 0;
    if (blockIdx.x == 0)
        for (int i = lane; i < ncounters; i += 64) counters[i] = 0;
    __syncthreads();
    int below = 0;                                           // valid ids in front of the slab (the same in every lane)
    for (int t0 = 0; t0 < T; t0 += 64 * PREFETCH) {          // PREFETCH independent loads in flight, then their work in order
        int idp[PREFETCH];
#pragma unroll
        for (int u = 0; u < PREFETCH; ++u) {
            const int t = t0 + 64 * u + lane;
            idp[u] = t < T ? ids[t] : -1;
        }
#pragma unroll
        for (int u = 0; u < PREFETCH; ++u) {
            const int id = idp[u];
            const bool ok = (unsigned)id < (unsigned)V;
            below += __popcll(__builtin_amdgcn_ballot_w64(ok && id < slab0));
            if (ok && (unsigned)(id - slab0) < (unsigned)SLAB) atomicAdd(&cnt[id - slab0], 1);
        }
    }
    __syncthreads();
    // lane b < SLAB keeps bin b's list: its length, where it begins in the sorted array, and the cursor of the second pass
    int my_n = 0, my_start = below;
    if (lane < SLAB) {
        my_n = cnt[lane];
        for (int j = 0; j < lane; ++j) my_start += cnt[j];
    }
    int my_cur = my_start;
    const int slab_end = __builtin_amdgcn_readlane(my_start + my_n, SLAB - 1);       // first sorted slot behind the slab's
    if (slab_end > below) {
        for (int t0 = 0; t0 < T; t0 += 64 * PREFETCH) {
          int idp[PREFETCH];
#pragma unroll
          for (int u = 0; u < PREFETCH; ++u) {
              const int t = t0 + 64 * u + lane;
              idp[u] = t < T ? ids[t] : -1;
          }
#pragma unroll
          for (int u = 0; u < PREFETCH; ++u) {               // 64 positions at a time, in ascending t
            const int t = t0 + 64 * u + lane;
            const int id = idp[u];
            const int bin = id - slab0;
            const bool mine = (unsigned)id < (unsigned)V && (unsigned)bin < (unsigned)SLAB;
            unsigned long long rem = __builtin_amdgcn_ballot_w64(mine);
            while (rem) {                                    // one turn per distinct bin among these 64 positions
                const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
                const int b = __builtin_amdgcn_readlane(bin, leader);
                const bool sel = mine && bin == b;
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(sel);
                const int cur = __builtin_amdgcn_readlane(my_cur, b);
                const int start = __builtin_amdgcn_readlane(my_start, b);
                const int n = __builtin_amdgcn_readlane(my_n, b);
                if (sel) {
                    const int dest = cur + __popcll(mask & ((1ull << lane) - 1ull));     // ascending t inside the bin
                    if ((unsigned)dest < (unsigned)T) {      // (always: the two passes read the same ids)
                        perm[dest] = t;
                        idv[dest] = id;
                        rnk[dest] = dest - start;
                        cntv[dest] = n;
                    }
                }
                if (lane == b) my_cur += __popcll(mask);
                rem &= ~mask;
            }
          }
        }
    }
    if (blockIdx.x == gridDim.x - 1)                         // the slots no valid id takes
        for (int i = slab_end + lane; i < T; i += 64) rnk[i] = -1;
}

template <typename TY>
__global__ __launch_bounds__(THREADS) void embed_sum_kernel(const int* __restrict__ perm, const int* __restrict__ idv,
                                                            const int* __restrict__ rnk, const int* __restrict__ cntv,
                                                            int* counters, float* part, const TY* __restrict__ dy, float* dw, int T,
                                                            int V) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (THREADS / 64) + wave;
    if (i >= T) return;
    const int r = rnk[i];
    if (r < 0 || r % CHUNK) return;
    const int v = idv[i], n = cntv[i];
    if ((unsigned)v >= (unsigned)V || n <= r || r > i) return;               // (never: the index kernel wrote them)
    int m = n - r < CHUNK ? n - r : CHUNK;
    m = m < T - i ? m : T - i;
    int my_t = lane < m ? perm[i + lane] : 0;
    my_t = (unsigned)my_t < (unsigned)T ? my_t : 0;          // (never out of range; a row of dy whatever the workspace holds)
    f32x4 acc = load4<TY>(dy + (long long)__builtin_amdgcn_readlane(my_t, 0) * D + 4 * lane);
    int j = 1;
    for (; j + 8 <= m; j += 8) {                             // eight independent loads in flight, added in ascending t
        f32x4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = load4<TY>(dy + (long long)__builtin_amdgcn_readlane(my_t, j + u) * D + 4 * lane);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += x[u];
    }
    for (; j < m; ++j) acc += load4<TY>(dy + (long long)__builtin_amdgcn_readlane(my_t, j) * D + 4 * lane);
    float* dst = dw + (long long)v * D + 4 * lane;
    if (n <= CHUNK) {
        *reinterpret_cast<f32x4*>(dst) = acc;
        return;
    }
    // a chunk of a long list: the partial sum goes to the workspace, the last wave to arrive combines in chunk order
    const int start = i - r, nch = (n + CHUNK - 1) / CHUNK;
    *reinterpret_cast<f32x4*>(part + (long long)(2 * (i / CHUNK) + (r > 0 ? 1 : 0)) * D + 4 * lane) = acc;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(counters + start / CHUNK, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != nch - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    f32x4 sum = *reinterpret_cast<const f32x4*>(part + (long long)(2 * (start / CHUNK)) * D + 4 * lane);
    int k = 1;
    for (; k + PREFETCH <= nch; k += PREFETCH) {             // independent loads in flight, added in chunk order
        f32x4 x[PREFETCH];
#pragma unroll
        for (int u = 0; u < PREFETCH; ++u)
            x[u] = *reinterpret_cast<const f32x4*>(part + (long long)(2 * ((start + (k + u) * CHUNK) / CHUNK) + 1) * D + 4 * lane);
#pragma unroll
        for (int u = 0; u < PREFETCH; ++u) sum += x[u];
    }
    for (; k < nch; ++k)
        sum += *reinterpret_cast<const f32x4*>(part + (long long)(2 * ((start + k * CHUNK) / CHUNK) + 1) * D + 4 * lane);
    *reinterpret_cast<f32x4*>(dst) = sum;
}

}  // namespace

extern "C" int mtmp_report_ids_gather(const int32_t* ids, long long total, const long long* desc, int32_t* out, int B, int L,
                                      void* stream) {
    MTMP_CHECK_ARG(desc && out && (ids || total == 0), "mtmp_report_ids_gather: null pointer");
    MTMP_CHECK_ARG(B > 0 && B <= (1 << 20) && L >= 3 && L <= (1 << 16) && total >= 0,
                   "mtmp_report_ids_gather: bad argument (B=%d L=%d, L >= 3: BOS, one id, EOS; ids=%lld)", B, L, total);
    MTMP_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0 && ((uintptr_t)ids & 3) == 0,
                   "mtmp_report_ids_gather: out must be 16-byte aligned, desc 8-byte, ids 4-byte");
    const long long elems = (long long)B * L;
    const long long blocks = ((elems + 3) / 4 + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(report_ids_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, ids, total, desc, out,
                       elems, L);
    MTMP_CHECK_LAUNCH("mtmp_report_ids_gather");
    return MTMP_OK;
}

extern "C" int mtmp_token_embed_fwd(const int32_t* ids, long long T, const void* table, int table_dtype, void* out, int out_dtype,
                                    int V, int Dm, void* stream) {
    MTMP_CHECK_ARG(ids && table && out, "mtmp_token_embed_fwd: null pointer");
    MTMP_CHECK_ARG((table_dtype == 0 || table_dtype == 1) && (out_dtype == 0 || out_dtype == 1),
                   "mtmp_token_embed_fwd: dtype codes %d -> %d (MTMP_F32 = 0, MTMP_BF16 = 1)", table_dtype, out_dtype);
    MTMP_CHECK_ARG(Dm == D, "mtmp_token_embed_fwd: D = %d, the kernels are built for the model dimension %d only", Dm, D);
    MTMP_CHECK_ARG(T > 0 && T <= (1LL << 24) && V > 0, "mtmp_token_embed_fwd: bad argument (T=%lld V=%d)", T, V);
    MTMP_CHECK_ARG(((uintptr_t)table & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)ids & 3) == 0,
                   "mtmp_token_embed_fwd: table and out must be 16-byte aligned, ids 4-byte");
    const int elems = (table_dtype == 0 && out_dtype == 0) ? 4 : 8;
    const long long blocks = (T * (D / elems) + THREADS - 1) / THREADS;
    const dim3 grid((unsigned)blocks), block(THREADS);
    hipStream_t st = (hipStream_t)stream;
    const char* w = (const char*)table;
    char* o = (char*)out;
    if (table_dtype == 0 && out_dtype == 0)
        hipLaunchKernelGGL((token_embed_fwd_kernel<4, 4>), grid, block, 0, st, ids, T, w, o, V);
    else if (table_dtype == 1 && out_dtype == 1)
        hipLaunchKernelGGL((token_embed_fwd_kernel<2, 2>), grid, block, 0, st, ids, T, w, o, V);
    else if (table_dtype == 0)
        hipLaunchKernelGGL((token_embed_fwd_kernel<4, 2>), grid, block, 0, st, ids, T, w, o, V);
    else
        hipLaunchKernelGGL((token_embed_fwd_kernel<2, 4>), grid, block, 0, st, ids, T, w, o, V);
    MTMP_CHECK_LAUNCH("mtmp_token_embed_fwd");
    return MTMP_OK;
}

extern "C" long long mtmp_token_embed_bwd_workspace(long long T, int V) {
    (void)V;
    return T > 0 && T <= (1LL << 24) ? bwd_workspace(nullptr, T).bytes : 0;
}

extern "C" int mtmp_token_embed_bwd_chunk(void) { return CHUNK; }

extern "C" int mtmp_token_embed_bwd(const int32_t* ids, long long T, const void* dy, int dy_dtype, float* dw, void* workspace,
                                    int V, int Dm, void* stream) {
    MTMP_CHECK_ARG(ids && dy && dw && workspace, "mtmp_token_embed_bwd: null pointer");
    MTMP_CHECK_ARG(dy_dtype == 0 || dy_dtype == 1, "mtmp_token_embed_bwd: dtype code %d (MTMP_F32 = 0, MTMP_BF16 = 1)", dy_dtype);
    MTMP_CHECK_ARG(Dm == D, "mtmp_token_embed_bwd: D = %d, the kernels are built for the model dimension %d only", Dm, D);
    MTMP_CHECK_ARG(T > 0 && T <= (1LL << 24) && V > 0 && V <= (1 << 30), "mtmp_token_embed_bwd: bad argument (T=%lld V=%d)", T, V);
    MTMP_CHECK_ARG(((uintptr_t)dy & 15) == 0 && ((uintptr_t)dw & 15) == 0 && ((uintptr_t)workspace & 15) == 0 &&
                       ((uintptr_t)ids & 3) == 0,
                   "mtmp_token_embed_bwd: dy, dw and the workspace must be 16-byte aligned, ids 4-byte");
    const BwdWs w = bwd_workspace(workspace, T);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)T;
    hipLaunchKernelGGL(embed_index_kernel, dim3((unsigned)((V + SLAB - 1) / SLAB)), dim3(64), 0, st, ids, n, V, w.perm, w.idv, w.rnk,
                       w.cntv, w.counters, w.ncounters);
    MTMP_CHECK_LAUNCH("mtmp_token_embed_bwd (index)");
    const dim3 grid((unsigned)((T + THREADS / 64 - 1) / (THREADS / 64))), block(THREADS);
    if (dy_dtype == 0)
        hipLaunchKernelGGL(embed_sum_kernel<float>, grid, block, 0, st, w.perm, w.idv, w.rnk, w.cntv, w.counters, w.part,
                           (const float*)dy, dw, n, V);
    else
        hipLaunchKernelGGL(embed_sum_kernel<bf16>, grid, block, 0, st, w.perm, w.idv, w.rnk, w.cntv, w.counters, w.part,
                           (const bf16*)dy, dw, n, V);
    MTMP_CHECK_LAUNCH("mtmp_token_embed_bwd (sum)");
    return MTMP_OK;
}
