// TIE event windows from a device-resident event store (builder/data/tie_store.py holds the store and the host plan).
//
// mtmp_tie_window_gather   one launch per batch.  After the trimming of the reference's loader (dataset_new.py:1986-2026) a
//   window is at most 18 carried-forward "initial" rows -- the features whose last measurement lies before the window, one per
//   set bit of the sample's mask -- followed by a CONTIGUOUS run of the patient's events, all times shifted by one scalar.  A
//   workgroup writes one chunk of CHUNK_ROWS rows of one sample: the chunk's 3 CHUNK_ROWS floats are contiguous in both output
//   forms, so lane i stores floats i, i + 256, i + 512 of the chunk (one dword each: a wave's store is 256 contiguous bytes,
//   whatever the 12-byte row pitch) and loads the one column it stores -- the float64 time, the float32 value or the uint8
//   feature index of row (float index) / 3.  Arithmetic in the reference's order: time - shift in float64, then float32, then
//   (round_fp16) float32 -> fp16 -> float32 as two roundings, the trainer's .half().float().  shift = the moved prediction hour
//   (realtime 1) or the minimum time over all rows of the UNtruncated window, which every workgroup of the sample recomputes
//   from the surviving initial rows and the per-hour minima (18 + the window's hours numbers, one wave); NaN propagates through
//   that minimum as it does through numpy's.  The zeros behind cu_seqlens[B] (packed) or behind a sample's length (padded) are
//   written here too: no memset in front, no pad launch behind.  Every index is 64-bit; a descriptor that points outside the
//   store's arrays makes its sample's rows zeros instead of a read out of bounds.
#include "common.hip.h"

namespace {

constexpr int CHUNK_ROWS = 256;
constexpr int THREADS = 256;
constexpr int N_FEAT = 18;
constexpr int DESC_WORDS = 8;     // first event, events, hour of the initial rows, first hour, hours, feature mask, t0, prediction hour

struct TieStore {
    const double* ev_time;
    const float* ev_val;
    const uint8_t* ev_feat;
    const float* norm;
    const double* delta;
    const double* hour_min;
    long long n_events, n_hours;
};

// numpy's minimum: a NaN on either side stays
MTMP_DEV double min_nan(double a, double b) { return (b < a || b != b) ? b : a; }

MTMP_DEV float round_out(float v, int round_fp16) { return round_fp16 ? (float)(_Float16)v : v; }

__global__ __launch_bounds__(THREADS) void tie_window_gather_kernel(TieStore st, const long long* __restrict__ desc,
                                                                    const int* __restrict__ cu, float* __restrict__ out, int B,
                                                                    int chunks, int t_pad, long long out_rows, int padded,
                                                                    int realtime, int round_fp16) {
    __shared__ double s_shift;
    const int tid = threadIdx.x;
    const long long blk = blockIdx.x;
    if (blk >= (long long)B * chunks) {                          // packed form: zeros from cu[B] to the end of the buffer
        const long long first = ((long long)cu[B] + (blk - (long long)B * chunks) * CHUNK_ROWS) * 3, end = out_rows * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long e = first + tid + j * THREADS;
            if (e >= 0 && e < end) out[e] = 0.f;
        }
        return;
    }
    const int b = (int)(blk / chunks), chunk = (int)(blk % chunks);
    const long long* d = desc + (long long)b * DESC_WORDS;
    const long long first_event = d[0], n_ev = d[1], init_hour = d[2], first_hour = d[3], n_hours = d[4], t0 = d[6], key = d[7];
    const unsigned mask = (unsigned)d[5] & ((1u << N_FEAT) - 1u);
    const int n_init = __builtin_popcount(mask);
    const long long row0 = cu[b];
    long long rows = (long long)cu[b + 1] - row0;                // what the batch's layout gives the sample
    if (rows < 0 || row0 < 0) rows = 0;
    long long len = rows;                                        // ... and how many of them the store can fill
    const bool sane = first_event >= 0 && n_ev >= 0 && first_event <= st.n_events - n_ev && init_hour >= 0 && init_hour < st.n_hours &&
                      first_hour >= 0 && n_hours >= 0 && first_hour <= st.n_hours - n_hours;
    if (!sane) len = 0;
    if (len > n_init + n_ev) len = n_init + n_ev;
    const long long chunk_row = (long long)chunk * CHUNK_ROWS;
    const long long limit = padded ? (long long)t_pad : rows;    // rows of this sample the launch writes (zeros from len on)
    if (chunk_row >= limit) return;

    const double* delta = st.delta + init_hour * N_FEAT;
    const double t_first = (double)(t0 + 1);
    double shift = (double)key;
    if (realtime != 1 && chunk_row < len) {                      // uniform over the workgroup
        if (tid < 64) {
            double m = __builtin_inf();
            for (long long i = tid; i < N_FEAT + n_hours; i += 64) {
                if (i < N_FEAT) {
                    if (mask >> i & 1u) m = min_nan(m, -delta[i] + t_first);
                } else {
                    m = min_nan(m, st.hour_min[first_hour + (i - N_FEAT)]);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = min_nan(m, __shfl_xor(m, o, 64));
            if (tid == 0) s_shift = m;
        }
        __syncthreads();
        shift = s_shift;
    }

    float* dst = out + (padded ? (long long)b * t_pad : row0) * 3;
    const long long row_end = padded ? (long long)t_pad : out_rows - row0;      // no store behind the buffer
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int e = tid + j * THREADS;
        const long long r = chunk_row + e / 3;
        const int col = e % 3;
        if (r >= limit || r >= row_end) continue;
        float v = 0.f;
        if (r >= len) {                                          // behind the sample (padded form), or a refused descriptor
        } else if (r < n_init) {
            int k = 0, seen = 0;
#pragma unroll
            for (int f = 0; f < N_FEAT; ++f) {
                const int s = mask >> f & 1u;
                if (s && seen == (int)r) k = f;
                seen += s;
            }
            v = col == 0 ? (float)((-delta[k] + t_first) - shift) : col == 1 ? st.norm[init_hour * N_FEAT + k] : (float)k;
        } else {
            const long long i = first_event + (r - n_init);
            v = col == 0 ? (float)(st.ev_time[i] - shift) : col == 1 ? st.ev_val[i] : (float)st.ev_feat[i];
        }
        dst[r * 3 + col] = round_out(v, round_fp16);
    }
}

// mtmp_hourly_window_gather   the hourly carry-forward windows (--vslt-type carryforward) from the same store: sample b is rows
//   first_row .. first_row + n_rows - 1 of `norm`, the columns whose bits are set in keep_bits, then zero rows up to W.  One thread
//   per output float; every element of out is written (no memset in front).
__global__ __launch_bounds__(THREADS) void hourly_window_gather_kernel(const float* __restrict__ norm, long long n_hours,
                                                                       const long long* __restrict__ desc, float* __restrict__ out,
                                                                       long long total, int W, int F, unsigned keep_bits,
                                                                       int round_fp16) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e % F);
    const long long t = e / F;
    const int r = (int)(t % W);
    const long long b = t / W;
    const long long first = desc[2 * b], n = desc[2 * b + 1];
    const bool sane = first >= 0 && n >= 0 && n <= W && first <= n_hours - n;
    float v = 0.f;
    if (sane && r < n) {
        int k = 0, seen = 0;
#pragma unroll
        for (int f = 0; f < N_FEAT; ++f) {
            const int s = keep_bits >> f & 1u;
            if (s && seen == j) k = f;
            seen += s;
        }
        v = round_out(norm[(first + r) * N_FEAT + k], round_fp16);
    }
    out[e] = v;
}

}  // namespace

extern "C" int mtmp_hourly_window_gather(const float* norm, long long n_hours, const long long* desc, float* out, int B, int W, int F,
                                         unsigned keep_bits, int round_fp16, void* stream) {
    MTMP_CHECK_ARG(norm && desc && out, "mtmp_hourly_window_gather: null pointer");
    MTMP_CHECK_ARG(B > 0 && B <= (1 << 20) && n_hours > 0 && W >= 1 && W <= (1 << 16) && F >= 1 && F <= N_FEAT,
                   "mtmp_hourly_window_gather: bad argument (B=%d hours=%lld W=%d F=%d)", B, n_hours, W, F);
    MTMP_CHECK_ARG((keep_bits >> N_FEAT) == 0 && __builtin_popcount(keep_bits) == F,
                   "mtmp_hourly_window_gather: keep_bits 0x%x does not select F=%d of the %d columns", keep_bits, F, N_FEAT);
    const long long total = (long long)B * W * F;
    const long long blocks = (total + THREADS - 1) / THREADS;
    MTMP_CHECK_ARG(blocks <= 0x7fffffffLL, "mtmp_hourly_window_gather: %lld workgroups", blocks);
    hipLaunchKernelGGL(hourly_window_gather_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, norm, n_hours,
                       desc, out, total, W, F, keep_bits, round_fp16);
    MTMP_CHECK_LAUNCH("mtmp_hourly_window_gather");
    return MTMP_OK;
}

extern "C" int mtmp_tie_window_gather(const double* ev_time, const float* ev_val, const uint8_t* ev_feat, const float* norm,
                                      const double* delta, const double* hour_min, long long n_events, long long n_hours,
                                      const long long* desc, const int32_t* cu_seqlens, float* out, int B, int max_len, int t_pad,
                                      long long total_rows, long long out_rows, int padded, int realtime, int round_fp16,
                                      void* stream) {
    MTMP_CHECK_ARG(norm && delta && hour_min && desc && cu_seqlens && out && (n_events == 0 || (ev_time && ev_val && ev_feat)),
                   "mtmp_tie_window_gather: null pointer");
    MTMP_CHECK_ARG(B > 0 && B <= (1 << 20) && n_events >= 0 && n_hours > 0 && max_len >= 1 && total_rows >= 1 &&
                       total_rows <= (long long)B * max_len,
                   "mtmp_tie_window_gather: bad argument (B=%d events=%lld hours=%lld max_len=%d total_rows=%lld)", B, n_events,
                   n_hours, max_len, total_rows);
    long long blocks;
    int chunks;
    if (padded) {
        MTMP_CHECK_ARG(t_pad >= max_len, "mtmp_tie_window_gather: t_pad %d is smaller than the longest sample (%d rows)", t_pad,
                       max_len);
        chunks = (t_pad + CHUNK_ROWS - 1) / CHUNK_ROWS;
        blocks = (long long)B * chunks;
    } else {
        MTMP_CHECK_ARG(out_rows >= total_rows, "mtmp_tie_window_gather: the event buffer holds %lld rows, the batch has %lld",
                       out_rows, total_rows);
        chunks = (max_len + CHUNK_ROWS - 1) / CHUNK_ROWS;
        blocks = (long long)B * chunks + (out_rows - total_rows + CHUNK_ROWS - 1) / CHUNK_ROWS;
    }
    MTMP_CHECK_ARG(blocks <= 0x7fffffffLL, "mtmp_tie_window_gather: %lld workgroups", blocks);
    const TieStore st{ev_time, ev_val, ev_feat, norm, delta, hour_min, n_events, n_hours};
    hipLaunchKernelGGL(tie_window_gather_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, st,
                       (const long long*)desc, cu_seqlens, out, B, chunks, t_pad, out_rows, padded, realtime, round_fp16);
    MTMP_CHECK_LAUNCH("mtmp_tie_window_gather");
    return MTMP_OK;
}
