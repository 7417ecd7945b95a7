// The device-side evaluator of a validation pass (builder/utils/device_evaluator.py owns the state, builder/trainer/validate.py
// drives it): predictions are collected on the device, one small capturable launch per batch, and the metrics of
// builder/utils/metrics.py -- exact AUROC and average precision over the DISTINCT prediction values, F1 at 0.01, the best F1 of
// the 0.01 .. 0.99 sweep, the mean batch loss -- are computed on the device at the end of the pass; the host copies 64 bytes.
//
// mtmp_eval_append   ONE workgroup.  The cursor lives in ctr[0] on the device and is read there, so the launch has no argument that
//   changes from batch to batch and can be replayed from a hipGraph.  Every lane reads the cursor, a barrier, lane 0 writes the
//   new one (and the drop count, the loss sum, the batch count); element i goes to slot cursor + i if that is below capacity and is
//   dropped (counted in ctr[2]) otherwise -- nothing is written out of range.  Logits mode stores 1 / (1 + exp(-x)) evaluated in
//   float64 and rounded ONCE to float32; both modes then apply torch.nan_to_num (NaN -> 0, +-inf -> +-FLT_MAX) and store -0.0 as
//   +0.0 (torch's tie test p[1:] != p[:-1] calls the two equal, a sort on bits would not).
//
// mtmp_eval_metrics  a stable LSD radix sort (four 8-bit digits) of a DESCENDING order-preserving key made of the float's bits, the
//   target byte as the value; then a scan of the targets and the tie-group ends; then the sums.
//     key      a = bits ^ (sign ? 0xFFFFFFFF : 0x80000000) ascends with the float (negatives and denormals included), key = ~a.
//     a pass   histogram per tile -> exclusive scan of the [digit][tile] table -> scatter.  Each is its OWN launch: a step that
//              needs every workgroup of the step before it never waits for them inside a kernel (no look-back, no flags, no spin).
//              The scatter ranks a tile stably without atomics: a wave owns a contiguous quarter of the tile and walks it in rounds
//              of 64 keys; the lanes of a round that hold the same digit find each other with eight 64-bit ballots, the rank is
//              the wave's running count of that digit plus the number of lower lanes in the match.
//     AUROC    2 P N AUROC = sum over tie groups of fp_g (2 tp_before_g + tp_g), in uint64 (exact below n = 2^31), one float64
//              division at the end.  0 when a class is absent.
//     AP       sum over tie-group ends of (R_e - R_prev) * P_e in float64, in a FIXED order: a lane's ends in index order, a
//              tile's lanes by a fixed tree, the tiles' partial sums by lane chunks in tile order and the same tree.  The terms sit
//              at the group ends and depend on the sorted keys and on the counts at the ends alone, so two runs, or a run on the
//              shuffled input, agree bit for bit.  NaN without positives.
//     F1       the array is sorted, so #{p >= thr} is a binary search and the true positives among them one look-up of the scan:
//              2 tp / (predicted + positives), 0 when that is 0, thr = i / 100.0 compared with (double)p.
//   No float atomics anywhere; integer atomics only in LDS (the tile histogram).
#include "common.hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int ITEMS = 8;
constexpr int TILE = THREADS * ITEMS;        // keys per workgroup of a sort pass (mtmp_eval_sort_tile)
constexpr int WAVES = THREADS / 64;
constexpr int WAVE_KEYS = TILE / WAVES;      // the contiguous run of a tile one wave ranks
constexpr int ROUNDS = WAVE_KEYS / 64;
constexpr int RADIX = 256;
constexpr int SCAN_THREADS = 1024;
constexpr long long MAX_N = 1ll << 24;

typedef unsigned long long u64;

MTMP_DEV unsigned key_of(float p) {
    const unsigned b = __float_as_uint(p);
    return ~(b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u));
}
MTMP_DEV float float_of(unsigned key) {
    const unsigned a = ~key;
    return __uint_as_float((a >> 31) ? (a ^ 0x80000000u) : ~a);
}

// torch.nan_to_num on float32, then -0.0 -> +0.0
MTMP_DEV float settle(float v) {
    unsigned b = __float_as_uint(v);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0u;                             // NaN
    else if ((b & 0x7FFFFFFFu) == 0x7F800000u) b = (b & 0x80000000u) | 0x7F7FFFFFu;   // +-inf -> +-FLT_MAX
    if ((b << 1) == 0u) b = 0u;
    return __uint_as_float(b);
}

__global__ __launch_bounds__(THREADS) void eval_append_kernel(const float* __restrict__ values, const float* __restrict__ targets,
                                                              long long count, int mode, const float* __restrict__ loss,
                                                              float* __restrict__ pred, unsigned char* __restrict__ tgt,
                                                              float* __restrict__ logit, long long capacity, long long* ctr,
                                                              double* loss_sum) {
    const long long cursor = ctr[0];
    const long long room = (cursor >= 0 && cursor < capacity) ? capacity - cursor : 0;
    const long long take = count < room ? count : room;
    __syncthreads();
    if (threadIdx.x == 0) {
        ctr[0] = cursor + take;
        ctr[2] += count - take;
        if (loss) {
            *loss_sum += (double)*loss;
            ctr[1] += 1;
        }
    }
    for (long long i = threadIdx.x; i < take; i += THREADS) {
        const float x = values[i];
        float p = x;
        if (mode == 0) p = (float)(1.0 / (1.0 + exp(-(double)x)));
        pred[cursor + i] = settle(p);
        tgt[cursor + i] = targets[i] != 0.0f ? 1 : 0;
        if (logit && mode == 0) logit[cursor + i] = x;
    }
}

// ---- block helpers: Hillis-Steele scan and a fixed tree, both in LDS, both a function of the lane index alone ----
template <int N, typename T, typename Op> MTMP_DEV T block_scan_excl(T v, T identity, T* lds, Op op, T& total) {
    const int tid = threadIdx.x;
    T* a = lds;
    T* b = lds + N;
    a[tid] = v;
    __syncthreads();
    for (int s = 1; s < N; s <<= 1) {
        T x = a[tid];
        if (tid >= s) x = op(a[tid - s], x);
        b[tid] = x;
        __syncthreads();
        T* t = a; a = b; b = t;
    }
    total = a[N - 1];
    const T r = tid ? a[tid - 1] : identity;
    __syncthreads();
    return r;
}

template <int N, typename T, typename Op> MTMP_DEV T block_tree(T v, T* lds, Op op) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) lds[tid] = op(lds[tid], lds[tid + s]);
        __syncthreads();
    }
    const T r = lds[0];
    __syncthreads();
    return r;
}

struct AddU { MTMP_DEV unsigned operator()(unsigned a, unsigned b) const { return a + b; } };
struct MaxI { MTMP_DEV int operator()(int a, int b) const { return a > b ? a : b; } };
struct AddD { MTMP_DEV double operator()(double a, double b) const { return a + b; } };
struct MaxD { MTMP_DEV double operator()(double a, double b) const { return a > b ? a : b; } };
struct AddQ { MTMP_DEV u64 operator()(u64 a, u64 b) const { return a + b; } };

// ---- the sort ----
__global__ __launch_bounds__(THREADS) void eval_keys_kernel(const float* __restrict__ pred, const unsigned char* __restrict__ tgt,
                                                            int n, unsigned* __restrict__ keys, unsigned char* __restrict__ vals) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < n) {
        keys[i] = key_of(pred[i]);
        vals[i] = tgt[i] ? 1 : 0;
    }
}

__global__ __launch_bounds__(THREADS) void eval_hist_kernel(const unsigned* __restrict__ keys, int n, int shift,
                                                            unsigned* __restrict__ hist, int n_tiles) {
    __shared__ unsigned h[RADIX];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int base = blockIdx.x * TILE;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int i = base + j * THREADS + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of m uint32 in place, ONE workgroup: a lane sums a contiguous chunk, the chunks' sums are scanned, the chunk is rewritten
__global__ __launch_bounds__(SCAN_THREADS) void eval_scan_kernel(unsigned* __restrict__ data, int m) {
    __shared__ unsigned lds[2 * SCAN_THREADS];
    const int per = (m + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min(m, (int)threadIdx.x * per), hi = min(m, lo + per);
    unsigned s = 0u;
    for (int i = lo; i < hi; ++i) s += data[i];
    unsigned total;
    unsigned run = block_scan_excl<SCAN_THREADS>(s, 0u, lds, AddU(), total);
    for (int i = lo; i < hi; ++i) {
        const unsigned v = data[i];
        data[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(THREADS) void eval_scatter_kernel(const unsigned* __restrict__ keys_in,
                                                               const unsigned char* __restrict__ vals_in, int n, int shift,
                                                               const unsigned* __restrict__ offs, int n_tiles,
                                                               unsigned* __restrict__ keys_out, unsigned char* __restrict__ vals_out) {
    __shared__ unsigned cnt[WAVES][RADIX];       // first the waves' digit counts, then their first output slots
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) cnt[w][tid] = 0u;
    __syncthreads();
    const int base = blockIdx.x * TILE + wave * WAVE_KEYS + lane;
    unsigned key[ROUNDS], rank[ROUNDS];
    unsigned char val[ROUNDS];
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int i = base + r * 64;
        const bool valid = i < n;
        key[r] = valid ? keys_in[i] : 0u;
        val[r] = valid ? vals_in[i] : (unsigned char)0;
        const unsigned d = (key[r] >> shift) & (RADIX - 1);
        u64 m = __builtin_amdgcn_ballot_w64(valid);                 // 64 bits wide: one bit per lane of the wave
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 bb = __builtin_amdgcn_ballot_w64(bit);
            m &= bit ? bb : ~bb;
        }
        const unsigned before = (unsigned)__popcll(m & below);
        unsigned c = 0u;
        if (valid) c = cnt[wave][d];
        rank[r] = c + before;
        __syncthreads();                         // every read of the round before the writes of the round
        if (valid && before == 0u) cnt[wave][d] = c + (unsigned)__popcll(m);
        __syncthreads();
    }
    // digit tid: the tile's first slot in the output, then each wave's
    {
        unsigned run = offs[(long long)tid * n_tiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const unsigned c = cnt[w][tid];
            cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int i = base + r * 64;
        if (i < n) {
            const unsigned d = (key[r] >> shift) & (RADIX - 1);
            const unsigned pos = cnt[wave][d] + rank[r];
            if (pos < (unsigned)n) {             // always true for a consistent table; an index is never trusted unchecked
                keys_out[pos] = key[r];
                vals_out[pos] = val[r];
            }
        }
    }
}

// ---- the curves ----
MTMP_DEV bool group_end(const unsigned* keys, int i, int n) { return i == n - 1 || keys[i + 1] != keys[i]; }

// per tile: positives, and the last tie-group end in it (-1: none)
__global__ __launch_bounds__(THREADS) void eval_tile_reduce_kernel(const unsigned* __restrict__ keys,
                                                                   const unsigned char* __restrict__ vals, int n,
                                                                   unsigned* __restrict__ tp_tile, int* __restrict__ end_tile) {
    __shared__ unsigned su[THREADS];
    __shared__ int si[THREADS];
    const int i0 = blockIdx.x * TILE + threadIdx.x * ITEMS;
    unsigned tp = 0u;
    int last = -1;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int i = i0 + j;
        if (i < n) {
            tp += vals[i];
            if (group_end(keys, i, n)) last = i;
        }
    }
    tp = block_tree<THREADS>(tp, su, AddU());
    last = block_tree<THREADS>(last, si, MaxI());
    if (threadIdx.x == 0) {
        tp_tile[blockIdx.x] = tp;
        end_tile[blockIdx.x] = last;
    }
}

// ONE workgroup: exclusive sum of the tiles' positives, exclusive running maximum of their last ends, the total of positives
__global__ __launch_bounds__(SCAN_THREADS) void eval_tile_scan_kernel(const unsigned* __restrict__ tp_tile,
                                                                      const int* __restrict__ end_tile, int n_tiles,
                                                                      unsigned* __restrict__ tp_base, int* __restrict__ end_base,
                                                                      unsigned* __restrict__ totals) {
    __shared__ unsigned su[2 * SCAN_THREADS];
    __shared__ int si[2 * SCAN_THREADS];
    const int per = (n_tiles + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min(n_tiles, (int)threadIdx.x * per), hi = min(n_tiles, lo + per);
    unsigned s = 0u;
    int e = -1;
    for (int t = lo; t < hi; ++t) {
        s += tp_tile[t];
        e = max(e, end_tile[t]);
    }
    unsigned total;
    int etotal;
    unsigned run = block_scan_excl<SCAN_THREADS>(s, 0u, su, AddU(), total);
    int erun = block_scan_excl<SCAN_THREADS>(e, -1, si, MaxI(), etotal);
    for (int t = lo; t < hi; ++t) {
        tp_base[t] = run;
        end_base[t] = erun;
        run += tp_tile[t];
        erun = max(erun, end_tile[t]);
    }
    if (threadIdx.x == 0) totals[0] = total;
}

// inclusive count of positives at every sorted position
__global__ __launch_bounds__(THREADS) void eval_tile_apply_kernel(const unsigned char* __restrict__ vals, int n,
                                                                  const unsigned* __restrict__ tp_base, unsigned* __restrict__ tps) {
    __shared__ unsigned su[2 * THREADS];
    const int i0 = blockIdx.x * TILE + threadIdx.x * ITEMS;
    unsigned v[ITEMS], s = 0u;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        v[j] = (i0 + j < n) ? vals[i0 + j] : 0u;
        s += v[j];
    }
    unsigned total;
    unsigned run = tp_base[blockIdx.x] + block_scan_excl<THREADS>(s, 0u, su, AddU(), total);
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        run += v[j];
        if (i0 + j < n) tps[i0 + j] = run;
    }
}

// per tile: the AUROC numerator and the AP terms of the tie groups that END in it
__global__ __launch_bounds__(THREADS) void eval_tile_sums_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ tps,
                                                                 int n, const int* __restrict__ end_base,
                                                                 const unsigned* __restrict__ totals, double* __restrict__ ap_part,
                                                                 u64* __restrict__ au_part) {
    __shared__ int si[2 * THREADS];
    __shared__ double sd[THREADS];
    __shared__ u64 sq[THREADS];
    const int i0 = blockIdx.x * TILE + threadIdx.x * ITEMS;
    bool is_end[ITEMS];
    int last = -1;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int i = i0 + j;
        is_end[j] = i < n && group_end(keys, i, n);
        if (is_end[j]) last = i;
    }
    int etotal;
    int prev = max(end_base[blockIdx.x], block_scan_excl<THREADS>(last, -1, si, MaxI(), etotal));
    const double P = (double)totals[0];
    double ap = 0.0;
    u64 au = 0ull;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        if (is_end[j]) {
            const int i = i0 + j;
            const unsigned tp_e = tps[i], tp_p = prev >= 0 ? tps[prev] : 0u;
            const unsigned tp_g = tp_e - tp_p, fp_g = (unsigned)(i - prev) - tp_g;
            au += (u64)fp_g * (u64)(2u * tp_p + tp_g);
            ap += ((double)tp_e / P - (double)tp_p / P) * ((double)tp_e / (double)(i + 1));
            prev = i;
        }
    }
    ap = block_tree<THREADS>(ap, sd, AddD());
    au = block_tree<THREADS>(au, sq, AddQ());
    if (threadIdx.x == 0) {
        ap_part[blockIdx.x] = ap;
        au_part[blockIdx.x] = au;
    }
}

// ONE workgroup: the tiles' partial sums in tile order, the F1 counts by binary search, the eight outputs
__global__ __launch_bounds__(THREADS) void eval_finalize_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ tps,
                                                                int n, int n_tiles, const double* __restrict__ ap_part,
                                                                const u64* __restrict__ au_part, const unsigned* __restrict__ totals,
                                                                const long long* __restrict__ ctr,
                                                                const double* __restrict__ loss_sum, double* __restrict__ out) {
    __shared__ double sd[THREADS];
    __shared__ u64 sq[THREADS];
    const int tid = threadIdx.x;
    const int per = (n_tiles + THREADS - 1) / THREADS;
    const int lo = min(n_tiles, tid * per), hi = min(n_tiles, lo + per);
    double ap = 0.0;
    u64 au = 0ull;
    for (int t = lo; t < hi; ++t) {
        ap += ap_part[t];
        au += au_part[t];
    }
    ap = block_tree<THREADS>(ap, sd, AddD());
    au = block_tree<THREADS>(au, sq, AddQ());
    const u64 P = n > 0 ? totals[0] : 0u, N = (u64)n - P;
    double f1 = 0.0;
    if (tid < 99 && n > 0) {
        const double thr = (double)(tid + 1) / 100.0;
        int a = 0, b = n;                        // descending: the first position whose value is below thr
        while (a < b) {
            const int mid = (a + b) >> 1;
            if ((double)float_of(keys[mid]) >= thr) a = mid + 1;
            else b = mid;
        }
        const u64 tp = a > 0 ? tps[a - 1] : 0u, denom = (u64)a + P;
        f1 = denom > 0 ? 2.0 * (double)tp / (double)denom : 0.0;
    }
    const double best = block_tree<THREADS>(f1, sd, MaxD());
    if (tid == 0) {
        const long long stored = ctr[0], batches = ctr[1], dropped = ctr[2];
        out[0] = (P > 0 && N > 0) ? (double)au / (double)(2ull * P * N) : 0.0;
        out[1] = P > 0 ? ap : __longlong_as_double(0x7FF8000000000000ll);
        out[2] = f1;
        out[3] = best;
        out[4] = batches > 0 ? *loss_sum / (double)batches : __longlong_as_double(0x7FF8000000000000ll);
        out[5] = (double)n;
        out[6] = (double)P;
        out[7] = (double)((stored != (long long)n ? 1 : 0) + (dropped != 0 ? 2 : 0));
    }
}

struct Layout {
    long long k0, k1, v0, v1, hist, tp_tile, end_tile, tp_base, end_base, ap, au, totals, bytes;
    int n_tiles;
};

Layout layout_of(long long n) {
    Layout L;
    const long long nt = (n + TILE - 1) / TILE;
    long long at = 0;
    auto take = [&at](long long bytes) {
        const long long here = at;
        at += (bytes + 15) & ~15ll;
        return here;
    };
    L.n_tiles = (int)nt;
    L.k0 = take(4 * n);
    L.k1 = take(4 * n);
    L.v0 = take(n);
    L.v1 = take(n);
    L.hist = take(4ll * RADIX * nt);
    L.tp_tile = take(4 * nt);
    L.end_tile = take(4 * nt);
    L.tp_base = take(4 * nt);
    L.end_base = take(4 * nt);
    L.ap = take(8 * nt);
    L.au = take(8 * nt);
    L.totals = take(16);
    L.bytes = at;
    return L;
}

}  // namespace

extern "C" int mtmp_eval_sort_tile(void) { return TILE; }

extern "C" long long mtmp_eval_workspace_bytes(long long n) {
    if (n < 0 || n > MAX_N) return -1;
    return layout_of(n).bytes;
}

extern "C" int mtmp_eval_append(const float* values, const float* targets, long long count, int mode, const float* loss, float* pred,
                                uint8_t* tgt, float* logit, long long capacity, long long* ctr, double* loss_sum, void* stream) {
    MTMP_CHECK_ARG(values && targets && pred && tgt && ctr && loss_sum, "mtmp_eval_append: null pointer");
    MTMP_CHECK_ARG(count >= 1 && count <= MAX_N, "mtmp_eval_append: count %lld is not in 1 .. 2^24", count);
    MTMP_CHECK_ARG(capacity >= 1 && capacity <= MAX_N, "mtmp_eval_append: capacity %lld is not in 1 .. 2^24", capacity);
    MTMP_CHECK_ARG(mode == 0 || mode == 1, "mtmp_eval_append: mode %d (0 = logits, 1 = probabilities)", mode);
    MTMP_CHECK_ARG(((uintptr_t)values & 3) == 0 && ((uintptr_t)targets & 3) == 0 && ((uintptr_t)pred & 3) == 0 &&
                       ((uintptr_t)logit & 3) == 0 && ((uintptr_t)loss & 3) == 0 && ((uintptr_t)ctr & 7) == 0 &&
                       ((uintptr_t)loss_sum & 7) == 0,
                   "mtmp_eval_append: float buffers must be 4-byte aligned, ctr and loss_sum 8-byte");
    hipLaunchKernelGGL(eval_append_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, values, targets, count, mode, loss, pred,
                       (unsigned char*)tgt, logit, capacity, ctr, loss_sum);
    MTMP_CHECK_LAUNCH("mtmp_eval_append");
    return MTMP_OK;
}

extern "C" int mtmp_eval_metrics(const float* pred, const uint8_t* tgt, long long n, const long long* ctr, const double* loss_sum,
                                 void* workspace, long long workspace_bytes, double* out, void* stream) {
    MTMP_CHECK_ARG(pred && tgt && ctr && loss_sum && workspace && out, "mtmp_eval_metrics: null pointer");
    MTMP_CHECK_ARG(n >= 0 && n <= MAX_N, "mtmp_eval_metrics: n %lld is not in 0 .. 2^24", n);
    MTMP_CHECK_ARG(((uintptr_t)pred & 3) == 0 && ((uintptr_t)ctr & 7) == 0 && ((uintptr_t)loss_sum & 7) == 0 &&
                       ((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 15) == 0,
                   "mtmp_eval_metrics: pred must be 4-byte aligned, ctr, loss_sum and out 8-byte, the workspace 16-byte");
    const Layout L = layout_of(n);
    MTMP_CHECK_ARG(workspace_bytes >= L.bytes, "mtmp_eval_metrics: the workspace holds %lld bytes, %lld predictions need %lld",
                   workspace_bytes, n, L.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned* k[2] = {(unsigned*)(ws + L.k0), (unsigned*)(ws + L.k1)};
    unsigned char* v[2] = {(unsigned char*)(ws + L.v0), (unsigned char*)(ws + L.v1)};
    unsigned* hist = (unsigned*)(ws + L.hist);
    unsigned *tp_tile = (unsigned*)(ws + L.tp_tile), *tp_base = (unsigned*)(ws + L.tp_base), *totals = (unsigned*)(ws + L.totals);
    int *end_tile = (int*)(ws + L.end_tile), *end_base = (int*)(ws + L.end_base);
    double* ap = (double*)(ws + L.ap);
    u64* au = (u64*)(ws + L.au);
    const int ni = (int)n, nt = L.n_tiles;
    if (ni > 0) {
        const dim3 tiles((unsigned)nt), block(THREADS);
        hipLaunchKernelGGL(eval_keys_kernel, dim3((unsigned)((ni + THREADS - 1) / THREADS)), block, 0, st, pred,
                           (const unsigned char*)tgt, ni, k[0], v[0]);
        for (int pass = 0; pass < 4; ++pass) {       // k0 -> k1 -> k0 -> k1 -> k0
            const int src = pass & 1, dst = src ^ 1, shift = 8 * pass;
            hipLaunchKernelGGL(eval_hist_kernel, tiles, block, 0, st, k[src], ni, shift, hist, nt);
            hipLaunchKernelGGL(eval_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, hist, RADIX * nt);
            hipLaunchKernelGGL(eval_scatter_kernel, tiles, block, 0, st, k[src], v[src], ni, shift, hist, nt, k[dst], v[dst]);
        }
        // sorted: k0 / v0; k1 becomes the inclusive count of positives
        hipLaunchKernelGGL(eval_tile_reduce_kernel, tiles, block, 0, st, k[0], v[0], ni, tp_tile, end_tile);
        hipLaunchKernelGGL(eval_tile_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, tp_tile, end_tile, nt, tp_base, end_base, totals);
        hipLaunchKernelGGL(eval_tile_apply_kernel, tiles, block, 0, st, v[0], ni, tp_base, k[1]);
        hipLaunchKernelGGL(eval_tile_sums_kernel, tiles, block, 0, st, k[0], k[1], ni, end_base, totals, ap, au);
    }
    hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(THREADS), 0, st, k[0], k[1], ni, ni > 0 ? nt : 0, ap, au, totals, ctr,
                       loss_sum, out);
    MTMP_CHECK_LAUNCH("mtmp_eval_metrics");
    return MTMP_OK;
}
